// augment.hip -- training augmentation of the device patch queue (dataloader.py:69-86, config.aug=True):
//   Compose([RandomBiasField(), ZNormalization(), RandomNoise(), RandomFlip(axes=(0,)),
//            OneOf({RandomAffine(): 0.8, RandomElasticDeformation(): 0.2})])
// as a resampling gather over the cached RAW volume.  The intensity chain is never materialised: the value of the
// transformed volume at source voxel q of channel c is
//   V(c, q) = (x(c, q) * b(q) - mu) * rho + sigma * g(seed, c * S + q)          (four fp32 operations, each rounded once)
// with b the bias field, (mu, rho) the z-normalisation of x * b over every voxel and g a counter-based standard normal.
// Two families of kernels:
//   statistics of a visit (3 launches): fp64 partial sums of x*b -> min V per block (every block finalises the same (mu, rho) from
//     the partials in the same fixed order) -> one block that writes (mu, rho, min V, sigma).  No atomics; bitwise reproducible.
//   sampling (1 launch per batch): one workgroup row per patch descriptor (blockIdx.y), lanes contiguous along W of the OUTPUT, one
//     output voxel per lane (a wave stores 256 contiguous bytes; four voxels per lane with 16-byte stores took 256 VGPRs, two waves
//     per SIMD, and measured 0-8 % slower); per voxel the 3x4 output->source map (+ the cubic B-spline displacement from the 7x7x7
//     control grid held in LDS), then the 8 clamped corners of V (bias once per corner, noise once per corner and channel) and
//     the nearest label.
#include "common.h"

namespace seg {

constexpr int kAugThreads = 256;
static_assert(kAugThreads == kReduceThreads, "the block size of reduce.h");
constexpr int kAugMaxBlocks = 1024;
constexpr int kAugWords = MI355SEG_AUG_DESC_WORDS;      // int32 words per patch descriptor
constexpr int kAugCp = 343;                             // 7 * 7 * 7 control points

struct AugBias { float c[20]; };

// ---- Philox-4x32-10 (Salmon et al., SC'11) keyed by the visit's seed, counter = the element's linear index in [C,D,H,W];
// Box-Muller on the first two words.  Stateless: the same value whichever thread, patch or kernel asks.
__device__ __forceinline__ float aug_gauss(unsigned k0, unsigned k1, long long elem) {
    unsigned c0 = (unsigned)elem, c1 = (unsigned)((unsigned long long)elem >> 32), c2 = 0u, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const float u0 = (float)((c0 >> 8) + 1u) * 0x1p-24f;          // (0, 1]: |g| <= sqrt(48 ln 2) = 5.77
    const float u1 = (float)(c1 >> 8) * 0x1p-24f;                 // [0, 1) revolutions
    return sqrtf(-1.3862943611198906f * __log2f(u0)) * __builtin_amdgcn_cosf(u1);
}

// ---- bias field exp(sum c_ijk a0^i a1^j a2^k), i + j + k <= 3, coefficients in torchio's loop order (i outer, k inner).
// The (a0, a1) part is collapsed into the four coefficients of a cubic in a2, shared by the voxels of a row.
template <class CO>
__device__ __forceinline__ void aug_bias_row(const CO& c, float a0, float a1, float (&K)[4]) {
    const float p0[4] = {1.f, a0, a0 * a0, a0 * a0 * a0}, p1[4] = {1.f, a1, a1 * a1, a1 * a1 * a1};
    K[0] = K[1] = K[2] = K[3] = 0.f;
    int n = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4 - i; ++j)
#pragma unroll
            for (int k = 0; k < 4 - i - j; ++k) K[k] = fmaf(c[n++], p0[i] * p1[j], K[k]);
}
__device__ __forceinline__ float aug_bias_at(const float (&K)[4], float a2) {
    return expf(fmaf(fmaf(fmaf(K[3], a2, K[2]), a2, K[1]), a2, K[0]));
}
// normalised coordinate (2 q + 1 - n) / (n - 1) in [-1, 1]
__device__ __forceinline__ float aug_unit(int q, int n, float rinv) { return (float)(2 * q + 1 - n) * rinv; }

// V = (x b - mu) rho + sigma g with every operation rounded on its own (no contraction): the statistics pass and the sampling pass
// evaluate bit-identical values, and the identity map reproduces (x - mu) * rho exactly
__device__ __forceinline__ float aug_value(float x, float b, float mu, float rho, float sigma, float g) {
    return __fadd_rn(__fmul_rn(__fsub_rn(__fmul_rn(x, b), mu), rho), __fmul_rn(sigma, g));
}

struct AugVol { const float* x; long long n, S; int C, D, H, W; float r0, r1, r2; };

// the pivot of the sums: x * b at element 0 (keeps sum d^2 - (sum d)^2 / n well conditioned for CT-like offsets, as znorm_sums_kernel)
__device__ __forceinline__ float aug_pivot(const AugVol& v, const AugBias& co) {
    float K[4];
    aug_bias_row(co.c, aug_unit(0, v.D, v.r0), aug_unit(0, v.H, v.r1), K);
    return __fmul_rn(v.x[0], aug_bias_at(K, aug_unit(0, v.W, v.r2)));
}

// visits every element once: f(element index, x, b).  VEC = 4: W % 4 == 0 and x 16-byte aligned, so a group of four lies in one row.
template <int VEC, class F>
__device__ __forceinline__ void aug_for_each(const AugVol& v, const AugBias& co, F&& f) {
    const long long groups = v.n / VEC;
    for (long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += (long long)gridDim.x * blockDim.x) {
        const long long e = gi * VEC;
        const int s = (int)(e % v.S);
        const int q2 = s % v.W, q1 = (s / v.W) % v.H, q0 = s / (v.W * v.H);
        float K[4];
        aug_bias_row(co.c, aug_unit(q0, v.D, v.r0), aug_unit(q1, v.H, v.r1), K);
        if constexpr (VEC == 4) {
            const f32x4_t xv = *reinterpret_cast<const f32x4_t*>(v.x + e);
#pragma unroll
            for (int j = 0; j < 4; ++j) f(e + j, xv[j], aug_bias_at(K, aug_unit(q2 + j, v.W, v.r2)));
        } else {
            f(e, v.x[e], aug_bias_at(K, aug_unit(q2, v.W, v.r2)));
        }
    }
}

template <int VEC>
__global__ __launch_bounds__(kAugThreads) void aug_sums_kernel(AugVol v, AugBias co, double* __restrict__ part) {
    const float pv = aug_pivot(v, co);
    double acc[2] = {0.0, 0.0};
    aug_for_each<VEC>(v, co, [&](long long, float x, float b) {
        const float d = __fsub_rn(__fmul_rn(x, b), pv);
        acc[0] += (double)d;
        acc[1] += (double)d * (double)d;
    });
    block_sum(acc);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = acc[0]; part[2 * blockIdx.x + 1] = acc[1]; }
}

// (mu, rho) from the block partials, fixed order; every thread of the block gets the same two floats
__device__ __forceinline__ void aug_mu_rho(const double* __restrict__ part, int nblk, float pv, long long n, float& mu, float& rho) {
    __shared__ float mr[2];
    double acc[2] = {0.0, 0.0};
    partials_reduce<OpSum>(part, nblk, acc);
    block_sum(acc);
    if (threadIdx.x == 0) pivoted_mean_rstd((double)pv, acc[0], acc[1], n, mr[0], mr[1]);
    __syncthreads();
    mu = mr[0]; rho = mr[1];
}

template <int VEC>
__global__ __launch_bounds__(kAugThreads) void aug_min_kernel(AugVol v, AugBias co, const double* __restrict__ part, int nblk_sums,
                                                              float sigma, unsigned k0, unsigned k1, float* __restrict__ minpart) {
    float mu, rho;
    aug_mu_rho(part, nblk_sums, aug_pivot(v, co), v.n, mu, rho);
    float m = INFINITY;
    aug_for_each<VEC>(v, co, [&](long long e, float x, float b) { m = fminf(m, aug_value(x, b, mu, rho, sigma, aug_gauss(k0, k1, e))); });
    m = block_reduce_one<OpMin>(m);
    if (threadIdx.x == 0) minpart[blockIdx.x] = m;
}

__global__ __launch_bounds__(kAugThreads) void aug_finalize_kernel(AugVol v, AugBias co, const double* __restrict__ part, int nblk_sums,
                                                                   const float* __restrict__ minpart, int nblk_min, float sigma,
                                                                   float* __restrict__ stats) {
    float mu, rho;
    aug_mu_rho(part, nblk_sums, aug_pivot(v, co), v.n, mu, rho);
    float m[1] = {INFINITY};
    partials_reduce<OpMin>(minpart, nblk_min, m);
    block_reduce<OpMin>(m);
    if (threadIdx.x == 0) {
        stats[0] = mu; stats[1] = rho;
        stats[2] = m[0];
        stats[3] = sigma;
    }
}

// ---- sampling -------------------------------------------------------------------------------------------------------------
// descriptor words (int32 [count][MI355SEG_AUG_DESC_WORDS], see mi355seg.h); everything read from it is wave-uniform
__device__ __forceinline__ float aug_wf(const int* d, int i) { return __builtin_bit_cast(float, d[i]); }
template <class T>
__device__ __forceinline__ T* aug_wp(const int* d, int i) {
    return reinterpret_cast<T*>((uintptr_t)(((unsigned long long)(unsigned)d[i + 1] << 32) | (unsigned long long)(unsigned)d[i]));
}

struct AugCoef {                    // operator[] over the descriptor's 20 bias words
    const int* d;
    __device__ __forceinline__ float operator[](int i) const { return __builtin_bit_cast(float, d[28 + i]); }
};

// uniform cubic B-spline basis at f in [0, 1]
__device__ __forceinline__ void aug_bspline(float f, float (&B)[4]) {
    const float f2 = f * f, f3 = f2 * f, g = 1.f - f;
    B[0] = g * g * g * (1.f / 6.f);
    B[1] = (3.f * f3 - 6.f * f2 + 4.f) * (1.f / 6.f);
    B[2] = (-3.f * f3 + 3.f * f2 + 3.f * f + 1.f) * (1.f / 6.f);
    B[3] = f3 * (1.f / 6.f);
}

template <int MODE>
__device__ __forceinline__ void aug_sample_body(const int* __restrict__ d, int C, int Cy, int pd, int ph, int pw,
                                                float* __restrict__ ox, float* __restrict__ oy, const float4* cps) {
    const float* __restrict__ img = aug_wp<const float>(d, 0);
    const float* __restrict__ lbl = aug_wp<const float>(d, 2);
    const float* __restrict__ st = aug_wp<const float>(d, 4);
    const int D = d[8], H = d[9], W = d[10], oz = d[11], oyy = d[12], oxx = d[13];
    const long long S = (long long)D * H * W;
    const float mu = st[0], rho = st[1], pad = st[2], sigma = aug_wf(d, 48);
    const unsigned k0 = (unsigned)d[50], k1 = (unsigned)d[51];
    float M[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) M[i] = aug_wf(d, 16 + i);
    const AugCoef co{d};
    const float r0 = 1.f / (float)(D - 1), r1 = 1.f / (float)(H - 1), r2 = 1.f / (float)(W - 1);

    const long long pS = (long long)pd * ph * pw;
    const int it = blockIdx.x * kAugThreads + threadIdx.x;          // the output voxel of this lane, W fastest
    if (it >= pd * ph * pw) return;
    const int xv = it % pw, yv = (it / pw) % ph, zv = it / (pw * ph);
    const float p0 = (float)(oz + zv), p1 = (float)(oyy + yv), p2 = (float)(oxx + xv);

    float wgt[8], bia[8];
    int off[8], loff;
    bool inside;
    {
        float t[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) t[a] = fmaf(M[4 * a], p0, fmaf(M[4 * a + 1], p1, fmaf(M[4 * a + 2], p2, M[4 * a + 3])));
        if constexpr (MODE == 1) {
            // u_a = 4 p_a / (n_a - 1), cell i_a = min(floor(u_a), 3), separable basis weights
            float B0[4], B1[4], B2[4];
            const float u0 = p0 * (4.f * r0), u1 = p1 * (4.f * r1), u2 = p2 * (4.f * r2);
            const int i0 = min(max((int)floorf(u0), 0), 3), i1 = min(max((int)floorf(u1), 0), 3), i2 = min(max((int)floorf(u2), 0), 3);
            aug_bspline(u0 - (float)i0, B0); aug_bspline(u1 - (float)i1, B1); aug_bspline(u2 - (float)i2, B2);
            float dz = 0.f, dy = 0.f, dx = 0.f;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float wab = B0[a] * B1[b];
                    float sz = 0.f, sy = 0.f, sx = 0.f;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float4 cp = cps[((i0 + a) * 7 + (i1 + b)) * 7 + (i2 + c)];
                        sz = fmaf(B2[c], cp.x, sz); sy = fmaf(B2[c], cp.y, sy); sx = fmaf(B2[c], cp.z, sx);
                    }
                    dz = fmaf(wab, sz, dz); dy = fmaf(wab, sy, dy); dx = fmaf(wab, sx, dx);
                }
            t[0] += dz; t[1] += dy; t[2] += dx;
        }
        inside = t[0] >= -0.5f && t[0] < (float)D - 0.5f && t[1] >= -0.5f && t[1] < (float)H - 0.5f && t[2] >= -0.5f && t[2] < (float)W - 0.5f;
        // out-of-domain (and non-finite) coordinates are pulled to the volume first, so every index below stays inside it
        const float tz = fminf(fmaxf(t[0], -0.5f), (float)D - 0.5f), ty = fminf(fmaxf(t[1], -0.5f), (float)H - 0.5f),
                    tx = fminf(fmaxf(t[2], -0.5f), (float)W - 0.5f);
        const float fz0 = floorf(tz), fy0 = floorf(ty), fx0 = floorf(tx);
        const float fz = tz - fz0, fy = ty - fy0, fx = tx - fx0;
        const int z0 = min(max((int)fz0, 0), D - 1), z1 = min(max((int)fz0 + 1, 0), D - 1);
        const int y0 = min(max((int)fy0, 0), H - 1), y1 = min(max((int)fy0 + 1, 0), H - 1);
        const int x0 = min(max((int)fx0, 0), W - 1), x1 = min(max((int)fx0 + 1, 0), W - 1);
        const float a20 = aug_unit(x0, W, r2), a21 = aug_unit(x1, W, r2);
#pragma unroll
        for (int k = 0; k < 4; ++k) {                  // the four (z, y) rows of the cell: bias cubic once per row
            const int zz = (k & 2) ? z1 : z0, yy = (k & 1) ? y1 : y0;
            const float wzy = ((k & 2) ? fz : 1.f - fz) * ((k & 1) ? fy : 1.f - fy);
            float K[4];
            aug_bias_row(co, aug_unit(zz, D, r0), aug_unit(yy, H, r1), K);
            const int row = (zz * H + yy) * W;
            off[2 * k] = row + x0; off[2 * k + 1] = row + x1;
            wgt[2 * k] = wzy * (1.f - fx); wgt[2 * k + 1] = wzy * fx;
            bia[2 * k] = aug_bias_at(K, a20); bia[2 * k + 1] = aug_bias_at(K, a21);
        }
        const int lz = min(max((int)floorf(tz + 0.5f), 0), D - 1), ly = min(max((int)floorf(ty + 0.5f), 0), H - 1),
                  lx = min(max((int)floorf(tx + 0.5f), 0), W - 1);
        loff = (lz * H + ly) * W + lx;
    }

    for (int c = 0; c < C; ++c) {
        const float* __restrict__ src = img + (long long)c * S;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float val = aug_value(src[off[k]], bia[k], mu, rho, sigma, aug_gauss(k0, k1, (long long)c * S + off[k]));
            acc = fmaf(wgt[k], val, acc);
        }
        ox[(long long)c * pS + it] = inside ? acc : pad;
    }
    for (int c = 0; c < Cy; ++c) {
        oy[(long long)c * pS + it] = inside ? lbl[(long long)c * S + loff] : 0.f;
    }
}

__global__ __launch_bounds__(kAugThreads) void aug_sample_kernel(const int* __restrict__ table, int C, int Cy, int pd, int ph, int pw,
                                                                 float* __restrict__ out_x, float* __restrict__ out_y) {
    __shared__ float4 cps[kAugCp];
    const int* __restrict__ d = table + (long long)blockIdx.y * kAugWords;
    const long long pS = (long long)pd * ph * pw;
    float* ox = out_x + (long long)blockIdx.y * C * pS;
    float* oy = out_y + (long long)blockIdx.y * Cy * pS;
    if (d[14] == 1) {              // wave-uniform: one branch per workgroup, none per voxel
        const float* __restrict__ cp = aug_wp<const float>(d, 6);
        for (int i = threadIdx.x; i < kAugCp; i += kAugThreads) cps[i] = make_float4(cp[i], cp[kAugCp + i], cp[2 * kAugCp + i], 0.f);
        __syncthreads();
        aug_sample_body<1>(d, C, Cy, pd, ph, pw, ox, oy, cps);
    } else {
        aug_sample_body<0>(d, C, Cy, pd, ph, pw, ox, oy, cps);
    }
}

}  // namespace seg

using namespace seg;

extern "C" {

size_t mi355seg_augment_ws_bytes(long long n) {
    (void)n;
    return (size_t)kAugMaxBlocks * 2 * sizeof(double) + (size_t)kAugMaxBlocks * sizeof(float) + 512;
}

int mi355seg_augment_stats_f32(const float* x, int C, int D, int H, int W, const float* bias_host, float sigma, long long seed,
                               float* stats, void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(x && bias_host && stats && C > 0 && D > 1 && H > 1 && W > 1, "augment_stats: bad arguments (C >= 1, every spatial dim >= 2)");
    SEG_CHECK_ARG((long long)D * H * W < (1ll << 31), "augment_stats: a channel of %dx%dx%d voxels exceeds 2^31 - 1", D, H, W);
    SEG_CHECK_ARG(sigma >= 0.f && sigma == sigma, "augment_stats: sigma must be >= 0");
    const long long S = (long long)D * H * W, n = S * C;
    SEG_CHECK_WS(mi355seg_augment_ws_bytes(n), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, 8.0 * n, st);
    Carver cv(ws);
    double* part = cv.take<double>((size_t)kAugMaxBlocks * 2);
    float* minpart = cv.take<float>(kAugMaxBlocks);
    AugVol v{x, n, S, C, D, H, W, 1.f / (float)(D - 1), 1.f / (float)(H - 1), 1.f / (float)(W - 1)};
    AugBias co;
    for (int i = 0; i < 20; ++i) co.c[i] = bias_host[i];
    const unsigned k0 = (unsigned)((unsigned long long)seed & 0xffffffffull), k1 = (unsigned)((unsigned long long)seed >> 32);
    const bool vec = (W % 4 == 0) && ((uintptr_t)x % 16 == 0);
    const int nblk = stream_grid(vec ? n / 4 : n, kAugThreads, kAugMaxBlocks);
    if (vec) {
        hipLaunchKernelGGL(aug_sums_kernel<4>, dim3(nblk), dim3(kAugThreads), 0, st, v, co, part);
        SEG_CHECK_LAUNCH();
        hipLaunchKernelGGL(aug_min_kernel<4>, dim3(nblk), dim3(kAugThreads), 0, st, v, co, (const double*)part, nblk, sigma, k0, k1, minpart);
    } else {
        hipLaunchKernelGGL(aug_sums_kernel<1>, dim3(nblk), dim3(kAugThreads), 0, st, v, co, part);
        SEG_CHECK_LAUNCH();
        hipLaunchKernelGGL(aug_min_kernel<1>, dim3(nblk), dim3(kAugThreads), 0, st, v, co, (const double*)part, nblk, sigma, k0, k1, minpart);
    }
    SEG_CHECK_LAUNCH();
    hipLaunchKernelGGL(aug_finalize_kernel, dim3(1), dim3(kAugThreads), 0, st, v, co, (const double*)part, nblk, (const float*)minpart, nblk, sigma, stats);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int mi355seg_augment_sample_f32(const int* table, int count, int C, int Cy, int pd, int ph, int pw, float* out_x, float* out_y,
                                void* stream) {
    SEG_CHECK_ARG(table && out_x && out_y && count > 0 && count <= 65535 && C > 0 && Cy > 0 && pd > 0 && ph > 0 && pw > 0,
                  "augment_sample: bad arguments (1 <= count <= 65535, C, Cy >= 1, patch %dx%dx%d)", pd, ph, pw);
    SEG_CHECK_ARG((long long)pd * ph * pw < (1ll << 31), "augment_sample: a patch of %dx%dx%d voxels exceeds 2^31 - 1", pd, ph, pw);
    SEG_CHECK_ARG((uintptr_t)table % 16 == 0, "augment_sample: the descriptor table must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long pS = (long long)pd * ph * pw;
    ProfScope ps(PF_LOSS, 0.0, 4.0 * count * (C * 2 + Cy * 2) * pS, st);
    const dim3 grid((unsigned)((pS + kAugThreads - 1) / kAugThreads), (unsigned)count);
    hipLaunchKernelGGL(aug_sample_kernel, grid, dim3(kAugThreads), 0, st, table, C, Cy, pd, ph, pw, out_x, out_y);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

}  // extern "C"
