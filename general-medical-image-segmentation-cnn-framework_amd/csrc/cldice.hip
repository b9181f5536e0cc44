// cldice.hip -- the soft-clDice loss term (Shit et al., CVPR 2021): the soft skeleton as one LDS-tiled stencil
// launch per iteration, forward and backward, the four sums of the term in one pass, a one-block finalise that also forms the
// coefficients of the backward, and the head and tail of the backward.  No atomics anywhere: every output element is written by
// exactly one thread and every sum has one order, so equal inputs give equal bits.
//
// Replaces (official clDice, soft_skeleton.py / cldice.py): soft_erode = min of three 3-tap -max_pool3d(-x), soft_dilate =
// max_pool3d(x, 3, 1, 1), soft_open, soft_skel's loop and soft_cldice's four sums, restated as one uniform step per level j:
//   E_{j+1} = erode(E_j);  delta = relu(E_j - dilate(E_{j+1}));  skel = skel + relu(delta - skel * delta),   j = 0 .. iters.
// Neighbours outside the volume never take part (the -inf / +inf padding of the pools).
// Subgradient at ties: a minimum or maximum routes its whole gradient to the tied candidate with the lowest raster index (z, y, x).
#include "common.h"
#include "loss_math.h"

// The forward promises the bits of the ATen composition, where every product, difference and sum is rounded once: no FMA
// contraction in this file (the __f*_rn intrinsics are plain operators here and contract like them).
#pragma clang fp contract(off)

namespace seg {

constexpr int kSkelThreads = 256;
static_assert(kSkelThreads == kReduceThreads, "the block size of reduce.h");
constexpr int kSkelMaxIters = 32;
constexpr long long kSkelMaxVoxels = 2147483647LL;
constexpr int kCldiceMaxBlocks = 2048;

// forward tile (z, y, x) and its staged boxes: E_j on tile + 2, E_{j+1} on tile + 1, the x-maximum on (tile + 1 in z, y) x tile
constexpr int FZ = 8, FY = 8, FX = 32;
constexpr int FE_Y = FY + 4, FE_X = FX + 4, FE_N = (FZ + 4) * FE_Y * FE_X;
constexpr int FN_Y = FY + 2, FN_X = FX + 2, FN_N = (FZ + 2) * FN_Y * FN_X;
constexpr int FM_N = (FZ + 2) * FN_Y * FX;
// backward tile: E_{j+1} on tile + 3, E_j and g_delta on tile + 2, g_E_{j+1} on tile + 1
constexpr int BZ = 4, BY = 8, BX = 32;
constexpr int BA_Y = BY + 6, BA_X = BX + 6, BA_N = (BZ + 6) * BA_Y * BA_X;
constexpr int BB_Y = BY + 4, BB_X = BX + 4, BB_N = (BZ + 4) * BB_Y * BB_X;
constexpr int BD_Y = BY + 2, BD_X = BX + 2, BD_N = (BZ + 2) * BD_Y * BD_X;
static_assert((BA_N + 2 * BB_N + BD_N) * 4 + BB_N + BD_N <= 65536, "the backward's boxes fit the static LDS limit");

struct SkelTile { long long base; int z0, y0, x0; };

// block -> (plane, tile origin); tiles run x fastest, planes slowest
template <int TZ, int TY, int TX>
__device__ __forceinline__ SkelTile skel_tile(int D, int H, int W) {
    const int txn = (W + TX - 1) / TX, tyn = (H + TY - 1) / TY, tzn = (D + TZ - 1) / TZ;
    long long b = blockIdx.x;
    SkelTile t;
    t.x0 = (int)(b % txn) * TX; b /= txn;
    t.y0 = (int)(b % tyn) * TY; b /= tyn;
    t.z0 = (int)(b % tzn) * TZ; b /= tzn;
    t.base = b * D * H * W;
    return t;
}
template <int TZ, int TY, int TX>
static long long skel_blocks(long long NC, int D, int H, int W) {
    return NC * ((D + TZ - 1) / TZ) * ((H + TY - 1) / TY) * ((W + TX - 1) / TX);
}

__device__ __forceinline__ bool skel_inside(int z, int y, int x, int D, int H, int W) {
    return (unsigned)z < (unsigned)D && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
}

// skel + relu(delta - skel * delta): product, difference and sum each rounded once (no FMA), as the ATen composition rounds them
__device__ __forceinline__ float skel_residual(float s, float d) { return d - s * d; }

// One level of the forward.  kFirst: skel_in is zero (j = 0) and is not read.
template <bool kFirst>
__global__ __launch_bounds__(kSkelThreads) void soft_skel_fwd_kernel(const float* __restrict__ e0, const float* __restrict__ sin,
        float* __restrict__ e1, float* __restrict__ sout, int D, int H, int W) {
    __shared__ float sE[FE_N];
    __shared__ float sN[FN_N];
    __shared__ float sM[FM_N];
    const SkelTile t = skel_tile<FZ, FY, FX>(D, H, W);
    const int tid = threadIdx.x;
    for (int i = tid; i < FE_N; i += kSkelThreads) {
        const int lx = i % FE_X, ly = (i / FE_X) % FE_Y, lz = i / (FE_X * FE_Y);
        const int z = t.z0 + lz - 2, y = t.y0 + ly - 2, x = t.x0 + lx - 2;
        sE[i] = skel_inside(z, y, x, D, H, W) ? e0[t.base + ((long long)z * H + y) * W + x] : INFINITY;
    }
    __syncthreads();
    // E_{j+1} = the 7-minimum, on tile + 1; outside the volume -inf, the maximum's padding
    for (int i = tid; i < FN_N; i += kSkelThreads) {
        const int lx = i % FN_X, ly = (i / FN_X) % FN_Y, lz = i / (FN_X * FN_Y);
        const int z = t.z0 + lz - 1, y = t.y0 + ly - 1, x = t.x0 + lx - 1;
        const int c = ((lz + 1) * FE_Y + ly + 1) * FE_X + lx + 1;
        float m = fminf(fminf(sE[c - FE_X * FE_Y], sE[c - FE_X]), fminf(sE[c - 1], sE[c]));
        m = fminf(m, fminf(fminf(sE[c + 1], sE[c + FE_X]), sE[c + FE_X * FE_Y]));
        const bool in = skel_inside(z, y, x, D, H, W);
        sN[i] = in ? m : -INFINITY;
        if (in && lz >= 1 && lz <= FZ && ly >= 1 && ly <= FY && lx >= 1 && lx <= FX) e1[t.base + ((long long)z * H + y) * W + x] = m;
    }
    __syncthreads();
    // the 27-maximum, separably: along x here, along y and z below
    for (int i = tid; i < FM_N; i += kSkelThreads) {
        const int lx = i % FX, r = i / FX, c = r * FN_X + lx;
        sM[i] = fmaxf(fmaxf(sN[c], sN[c + 1]), sN[c + 2]);
    }
    __syncthreads();
    for (int i = tid; i < FZ * FY * FX; i += kSkelThreads) {
        const int lx = i % FX, ly = (i / FX) % FY, lz = i / (FX * FY);
        const int z = t.z0 + lz, y = t.y0 + ly, x = t.x0 + lx;
        if (!skel_inside(z, y, x, D, H, W)) continue;
        float m = -INFINITY;
#pragma unroll
        for (int dz = 0; dz < 3; ++dz)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) m = fmaxf(m, sM[((lz + dz) * FN_Y + ly + dy) * FX + lx]);
        const float pre = sE[((lz + 2) * FE_Y + ly + 2) * FE_X + lx + 2] - m;
        const float d = pre > 0.f ? pre : 0.f;
        const long long g = t.base + ((long long)z * H + y) * W + x;
        if (kFirst) {
            sout[g] = d;                                  // 0 + relu(d - 0 * d)
        } else {
            const float s = sin[g], u = skel_residual(s, d);
            sout[g] = s + (u > 0.f ? u : 0.f);
        }
    }
}

// One level of the backward, in gather form.  Recomputes the arg-max of the 27-maximum and the arg-min of the 7-minimum from the
// saved E_j (e0) and E_{j+1} (e1): first candidate in raster order wins.  kFirst: skel_in is zero and g_skel_in is not written.
// ge1 (the gradient that later levels sent to E_{j+1}) may be null: zero.
template <bool kFirst>
__global__ __launch_bounds__(kSkelThreads) void soft_skel_bwd_kernel(const float* __restrict__ e0, const float* __restrict__ e1,
        const float* __restrict__ sin, const float* __restrict__ gso, const float* __restrict__ ge1,
        float* __restrict__ ge0, float* __restrict__ gsin, int D, int H, int W) {
    __shared__ float sA[BA_N];           // E_{j+1}, tile + 3, -inf outside
    __shared__ float sB[BB_N];           // E_j, tile + 2, +inf outside
    __shared__ float sC[BB_N];           // g_pre = g_delta [delta > 0], tile + 2
    __shared__ float sD[BD_N];           // g_E_{j+1}, tile + 1
    __shared__ signed char cA[BB_N];     // arg-max of the 27 box (0..26 in raster order; -1: nothing to route)
    __shared__ signed char cI[BD_N];     // arg-min of the 7 cross (0..6 in raster order; -1: outside)
    const SkelTile t = skel_tile<BZ, BY, BX>(D, H, W);
    const int tid = threadIdx.x;
    for (int i = tid; i < BA_N; i += kSkelThreads) {
        const int lx = i % BA_X, ly = (i / BA_X) % BA_Y, lz = i / (BA_X * BA_Y);
        const int z = t.z0 + lz - 3, y = t.y0 + ly - 3, x = t.x0 + lx - 3;
        sA[i] = skel_inside(z, y, x, D, H, W) ? e1[t.base + ((long long)z * H + y) * W + x] : -INFINITY;
    }
    for (int i = tid; i < BB_N; i += kSkelThreads) {
        const int lx = i % BB_X, ly = (i / BB_X) % BB_Y, lz = i / (BB_X * BB_Y);
        const int z = t.z0 + lz - 2, y = t.y0 + ly - 2, x = t.x0 + lx - 2;
        sB[i] = skel_inside(z, y, x, D, H, W) ? e0[t.base + ((long long)z * H + y) * W + x] : INFINITY;
    }
    __syncthreads();
    // g_pre and the arg-max on tile + 2; g_skel_in on the tile itself
    for (int i = tid; i < BB_N; i += kSkelThreads) {
        const int lx = i % BB_X, ly = (i / BB_X) % BB_Y, lz = i / (BB_X * BB_Y);
        const int z = t.z0 + lz - 2, y = t.y0 + ly - 2, x = t.x0 + lx - 2;
        float gpre = 0.f;
        int code = -1;
        if (skel_inside(z, y, x, D, H, W)) {
            const int c = ((lz + 1) * BA_Y + ly + 1) * BA_X + lx + 1;
            float best = -INFINITY;
            int k = 0;
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx, ++k) {
                        const float v = sA[c + (dz * BA_Y + dy) * BA_X + dx];
                        if (v > best) { best = v; code = k; }
                    }
            const long long g = t.base + ((long long)z * H + y) * W + x;
            const float pre = sB[i] - best, d = pre > 0.f ? pre : 0.f;
            const float s = kFirst ? 0.f : sin[g], go = gso[g];
            const float gu = skel_residual(s, d) > 0.f ? go : 0.f;
            gpre = pre > 0.f ? gu - gu * s : 0.f;
            if (!kFirst && lz >= 2 && lz < BZ + 2 && ly >= 2 && ly < BY + 2 && lx >= 2 && lx < BX + 2)
                gsin[g] = go - gu * d;
            if (gpre == 0.f) code = -1;
        }
        sC[i] = gpre;
        cA[i] = (signed char)code;
    }
    __syncthreads();
    // g_E_{j+1} = incoming - (what the 27-maxima route here), and the arg-min, on tile + 1
    for (int i = tid; i < BD_N; i += kSkelThreads) {
        const int lx = i % BD_X, ly = (i / BD_X) % BD_Y, lz = i / (BD_X * BD_Y);
        const int z = t.z0 + lz - 1, y = t.y0 + ly - 1, x = t.x0 + lx - 1;
        float out = 0.f;
        int code = -1;
        if (skel_inside(z, y, x, D, H, W)) {
            double acc = ge1 ? (double)ge1[t.base + ((long long)z * H + y) * W + x] : 0.0;
            const int c = ((lz + 1) * BB_Y + ly + 1) * BB_X + lx + 1;
            int k = 0;
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx, ++k) {
                        const int q = c + (dz * BB_Y + dy) * BB_X + dx;
                        if (cA[q] == 26 - k) acc -= (double)sC[q];          // the neighbour's maximum sits here
                    }
            out = (float)acc;
            const int off[7] = {-BB_X * BB_Y, -BB_X, -1, 0, 1, BB_X, BB_X * BB_Y};
            float best = INFINITY;
#pragma unroll
            for (int m = 0; m < 7; ++m) {
                const float v = sB[c + off[m]];
                if (v < best) { best = v; code = m; }
            }
        }
        sD[i] = out;
        cI[i] = (signed char)code;
    }
    __syncthreads();
    for (int i = tid; i < BZ * BY * BX; i += kSkelThreads) {
        const int lx = i % BX, ly = (i / BX) % BY, lz = i / (BX * BY);
        const int z = t.z0 + lz, y = t.y0 + ly, x = t.x0 + lx;
        if (!skel_inside(z, y, x, D, H, W)) continue;
        double acc = (double)sC[((lz + 2) * BB_Y + ly + 2) * BB_X + lx + 2];
        const int c = ((lz + 1) * BD_Y + ly + 1) * BD_X + lx + 1;
        const int off[7] = {-BD_X * BD_Y, -BD_X, -1, 0, 1, BD_X, BD_X * BD_Y};
#pragma unroll
        for (int m = 0; m < 7; ++m)
            if (cI[c + off[m]] == 6 - m) acc += (double)sD[c + off[m]];     // the neighbour's minimum sits here
        ge0[t.base + ((long long)z * H + y) * W + x] = (float)acc;
    }
}

static int cldice_grid(long long items) { return stream_grid(items, kSkelThreads, kCldiceMaxBlocks); }

// P = sigmoid(logits[:, c0:]), T = target[:, c0:], contiguous [N, K - c0, S]
__global__ __launch_bounds__(kSkelThreads) void cldice_probs_kernel(const float* __restrict__ x, const float* __restrict__ t,
        long long n, long long KpS, long long KS, long long c0S, float* __restrict__ P, float* __restrict__ T) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / KpS, src = b * KS + c0S + (i - b * KpS);
        P[i] = sigmoid(x[src]);
        T[i] = t[src];
    }
}

// part[block][4] = sum S_P T, sum S_P, sum S_T P, sum S_T
__global__ __launch_bounds__(kSkelThreads) void cldice_sums_kernel(const float* __restrict__ sp, const float* __restrict__ st,
        const float* __restrict__ p, const float* __restrict__ t, long long n, double* __restrict__ part) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float a = sp[i], b = st[i];
        acc[0] += (double)a * (double)t[i]; acc[1] += (double)a;
        acc[2] += (double)b * (double)p[i]; acc[3] += (double)b;
    }
    block_sum(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) part[(long long)blockIdx.x * 4 + j] = acc[j];
    }
}

// out fp64[3] = cldice, tprec, tsens; coef fp64[3] = a, b, c with dcldice/dS_P = a T + b and the direct dcldice/dP = c S_T
__global__ __launch_bounds__(kSkelThreads) void cldice_finalize_kernel(const double* __restrict__ part, int nblk, double smooth,
        float* __restrict__ loss, double* __restrict__ out, double* __restrict__ coef) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    partials_reduce<OpSum>(part, nblk, acc);
    block_sum(acc);
    if (threadIdx.x != 0) return;
    const double dp = acc[1] + smooth, ds = acc[3] + smooth;
    const double tprec = (acc[0] + smooth) / dp, tsens = (acc[2] + smooth) / ds, sum = tprec + tsens;
    const double cl = 1.0 - 2.0 * tprec * tsens / sum;
    const double dtp = -2.0 * tsens * tsens / (sum * sum), dts = -2.0 * tprec * tprec / (sum * sum);
    loss[0] = (float)cl;
    out[0] = cl; out[1] = tprec; out[2] = tsens;
    coef[0] = dtp / dp;
    coef[1] = -dtp * tprec / dp;
    coef[2] = dts / ds;
}

__global__ __launch_bounds__(kSkelThreads) void cldice_bwd_head_kernel(const float* __restrict__ t, const double* __restrict__ coef,
        long long n, float* __restrict__ gs) {
    const double a = coef[0], b = coef[1];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        gs[i] = (float)(a * (double)t[i] + b);
}

// dlogits[:, c0:] = gscale (g_P + c S_T) P (1 - P); channel 0 (when there is one) gets zeros
__global__ __launch_bounds__(kSkelThreads) void cldice_bwd_tail_kernel(const float* __restrict__ gp, const float* __restrict__ st,
        const float* __restrict__ p, const double* __restrict__ coef, const float* __restrict__ gscale,
        long long total, long long KpS, long long KS, long long c0S, float* __restrict__ dx) {
    const double c = coef[2], gs = (double)gscale[0];
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
        const long long b = o / KS, r = o - b * KS;
        float v = 0.f;
        if (r >= c0S) {
            const long long i = b * KpS + (r - c0S);
            const double q = (double)p[i];
            v = (float)(gs * ((double)gp[i] + c * (double)st[i]) * (q * (1.0 - q)));
        }
        dx[o] = v;
    }
}

// the level stack a soft skeleton keeps: E_1 .. E_{iters+1}, then skel_1 .. skel_{iters+1} (skel_j = the skeleton after level j - 1)
static size_t skel_slot_bytes(long long vox) { return align_up((size_t)vox * sizeof(float), 256); }
static float* skel_E(void* ws, long long vox, int iters, int j) { return (float*)((char*)ws + (size_t)(j - 1) * skel_slot_bytes(vox)); }
static float* skel_S(void* ws, long long vox, int iters, int j) { return (float*)((char*)ws + (size_t)(iters + j) * skel_slot_bytes(vox)); }

}  // namespace seg

using namespace seg;

#define SKEL_CHECK_GEOM(what)                                                                                                        \
    do {                                                                                                                             \
        SEG_CHECK_ARG(NC > 0 && D > 0 && H > 0 && W > 0, what ": bad extents NC=%lld D=%d H=%d W=%d", NC, D, H, W);                  \
        SEG_CHECK_ARG(NC <= kSkelMaxVoxels / D / H / W, what ": more than 2^31 - 1 voxels (NC=%lld D=%d H=%d W=%d)", NC, D, H, W);   \
        SEG_CHECK_ARG(iters >= 1 && iters <= kSkelMaxIters, what ": iters must be in 1..%d, got %d", kSkelMaxIters, iters);          \
        SEG_CHECK_ARG(j >= 0 && j <= iters, what ": level j must be in 0..iters = %d, got %d", iters, j);                            \
    } while (0)

extern "C" {

size_t mi355seg_soft_skel_ws_bytes(long long NC, int D, int H, int W, int iters) {
    if (NC < 1 || D < 1 || H < 1 || W < 1 || iters < 1 || iters > kSkelMaxIters || NC > kSkelMaxVoxels / D / H / W) return 0;
    return (size_t)(2 * (iters + 1)) * skel_slot_bytes(NC * D * H * W);
}

int mi355seg_soft_skel_step_fwd_f32(const float* x, long long NC, int D, int H, int W, int iters, int j,
                                    void* ws, size_t ws_bytes, void* stream) {
    SKEL_CHECK_GEOM("soft_skel_step_fwd");
    SEG_CHECK_ARG(x && ws, "soft_skel_step_fwd: null pointer");
    SEG_CHECK_ARG(((uintptr_t)ws % 4) == 0, "soft_skel_step_fwd: the workspace must be 4-byte aligned");
    SEG_CHECK_WS(mi355seg_soft_skel_ws_bytes(NC, D, H, W, iters), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    const long long vox = NC * D * H * W;
    ProfScope ps(PF_LOSS, 0.0, (j ? 16.0 : 12.0) * vox, st);
    const float* e0 = j ? skel_E(ws, vox, iters, j) : x;
    float* e1 = skel_E(ws, vox, iters, j + 1);
    float* sout = skel_S(ws, vox, iters, j + 1);
    const unsigned nblk = (unsigned)skel_blocks<FZ, FY, FX>(NC, D, H, W);
    if (j == 0) hipLaunchKernelGGL(soft_skel_fwd_kernel<true>, dim3(nblk), dim3(kSkelThreads), 0, st, e0, (const float*)nullptr, e1, sout, D, H, W);
    else hipLaunchKernelGGL(soft_skel_fwd_kernel<false>, dim3(nblk), dim3(kSkelThreads), 0, st, e0, (const float*)skel_S(ws, vox, iters, j), e1, sout, D, H, W);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int mi355seg_soft_skel_step_bwd_f32(const float* x, const float* g_skel_out, const float* g_e_next, float* g_e, float* g_skel_in,
                                    long long NC, int D, int H, int W, int iters, int j,
                                    const void* ws, size_t ws_bytes, void* stream) {
    SKEL_CHECK_GEOM("soft_skel_step_bwd");
    SEG_CHECK_ARG(x && g_skel_out && g_e && ws && (j == 0 || g_skel_in), "soft_skel_step_bwd: null pointer");
    SEG_CHECK_ARG(g_e != g_e_next && g_skel_in != g_skel_out, "soft_skel_step_bwd: an output aliases an input (the gather reads halos)");
    SEG_CHECK_ARG(((uintptr_t)ws % 4) == 0, "soft_skel_step_bwd: the workspace must be 4-byte aligned");
    SEG_CHECK_WS(mi355seg_soft_skel_ws_bytes(NC, D, H, W, iters), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    const long long vox = NC * D * H * W;
    ProfScope ps(PF_LOSS, 0.0, 28.0 * vox, st);
    void* w = const_cast<void*>(ws);
    const float* e0 = j ? skel_E(w, vox, iters, j) : x;
    const float* e1 = skel_E(w, vox, iters, j + 1);
    const unsigned nblk = (unsigned)skel_blocks<BZ, BY, BX>(NC, D, H, W);
    if (j == 0) hipLaunchKernelGGL(soft_skel_bwd_kernel<true>, dim3(nblk), dim3(kSkelThreads), 0, st, e0, e1, (const float*)nullptr, g_skel_out, g_e_next, g_e, (float*)nullptr, D, H, W);
    else hipLaunchKernelGGL(soft_skel_bwd_kernel<false>, dim3(nblk), dim3(kSkelThreads), 0, st, e0, e1, (const float*)skel_S(w, vox, iters, j), g_skel_out, g_e_next, g_e, g_skel_in, D, H, W);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int mi355seg_cldice_probs_f32(const float* logits, const float* target, long long N, int K, long long S,
                              float* P, float* T, void* stream) {
    SEG_CHECK_ARG(N > 0 && K > 0 && S > 0, "cldice_probs: bad extents N=%lld K=%d S=%lld", N, K, S);
    SEG_CHECK_ARG(N <= kSkelMaxVoxels / K / S, "cldice_probs: more than 2^31 - 1 elements (N=%lld K=%d S=%lld)", N, K, S);
    SEG_CHECK_ARG(logits && target && P && T, "cldice_probs: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int c0 = K > 1 ? 1 : 0;
    const long long n = N * (K - c0) * S;
    ProfScope ps(PF_LOSS, 0.0, 16.0 * n, st);
    hipLaunchKernelGGL(cldice_probs_kernel, dim3(cldice_grid(n)), dim3(kSkelThreads), 0, st, logits, target, n, (long long)(K - c0) * S, (long long)K * S, (long long)c0 * S, P, T);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

size_t mi355seg_cldice_ws_bytes(long long n) {
    if (n < 1 || n > kSkelMaxVoxels) return 0;
    return (size_t)cldice_grid(n) * 4 * sizeof(double);
}

int mi355seg_cldice_sums_f32(const float* skel_p, const float* skel_t, const float* P, const float* T, long long n,
                             void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(n > 0 && n <= kSkelMaxVoxels, "cldice_sums: bad extent n=%lld", n);
    SEG_CHECK_ARG(skel_p && skel_t && P && T && ws, "cldice_sums: null pointer");
    SEG_CHECK_ARG(((uintptr_t)ws % 8) == 0, "cldice_sums: the workspace must be 8-byte aligned");
    SEG_CHECK_WS(mi355seg_cldice_ws_bytes(n), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, 16.0 * n, st);
    hipLaunchKernelGGL(cldice_sums_kernel, dim3(cldice_grid(n)), dim3(kSkelThreads), 0, st, skel_p, skel_t, P, T, n, (double*)ws);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int mi355seg_cldice_finalize(const void* ws, size_t ws_bytes, long long n, float smooth,
                             float* loss, double* parts, double* coef, void* stream) {
    SEG_CHECK_ARG(n > 0 && n <= kSkelMaxVoxels, "cldice_finalize: bad extent n=%lld", n);
    SEG_CHECK_ARG(smooth > 0.f, "cldice_finalize: smooth must be > 0, got %g", (double)smooth);
    SEG_CHECK_ARG(ws && loss && parts && coef, "cldice_finalize: null pointer");
    SEG_CHECK_ARG(((uintptr_t)ws % 8) == 0, "cldice_finalize: the workspace must be 8-byte aligned");
    SEG_CHECK_WS(mi355seg_cldice_ws_bytes(n), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cldice_finalize_kernel, dim3(1), dim3(kSkelThreads), 0, st, (const double*)ws, cldice_grid(n), (double)smooth, loss, parts, coef);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int mi355seg_cldice_bwd_head_f32(const float* T, const double* coef, long long n, float* g_skel, void* stream) {
    SEG_CHECK_ARG(n > 0 && n <= kSkelMaxVoxels, "cldice_bwd_head: bad extent n=%lld", n);
    SEG_CHECK_ARG(T && coef && g_skel, "cldice_bwd_head: null pointer");
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, 8.0 * n, st);
    hipLaunchKernelGGL(cldice_bwd_head_kernel, dim3(cldice_grid(n)), dim3(kSkelThreads), 0, st, T, coef, n, g_skel);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int mi355seg_cldice_bwd_tail_f32(const float* g_p, const float* skel_t, const float* P, const double* coef, const float* gscale,
                                 long long N, int K, long long S, float* dlogits, void* stream) {
    SEG_CHECK_ARG(N > 0 && K > 0 && S > 0, "cldice_bwd_tail: bad extents N=%lld K=%d S=%lld", N, K, S);
    SEG_CHECK_ARG(N <= kSkelMaxVoxels / K / S, "cldice_bwd_tail: more than 2^31 - 1 elements (N=%lld K=%d S=%lld)", N, K, S);
    SEG_CHECK_ARG(g_p && skel_t && P && coef && gscale && dlogits, "cldice_bwd_tail: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int c0 = K > 1 ? 1 : 0;
    const long long total = N * K * S;
    ProfScope ps(PF_LOSS, 0.0, 20.0 * total, st);
    hipLaunchKernelGGL(cldice_bwd_tail_kernel, dim3(cldice_grid(total)), dim3(kSkelThreads), 0, st, g_p, skel_t, P, coef, gscale, total,
                       (long long)(K - c0) * S, (long long)K * S, (long long)c0 * S, dlogits);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

}  // extern "C"
