// boundary.hip -- the boundary loss term (Kervadec et al., MIDL 2019): the signed Euclidean distance map phi of every
// class of a one-hot target patch as three separable fp32 passes, and the term mean(sigmoid(logit) * phi) forward and backward.
// No atomics anywhere: every output element is written by exactly one thread and every sum has one order, so equal inputs give
// equal bits.  No fp64 in the distance passes (the partial sums of the loss are fp64 through reduce.h, as everywhere).
//
// Replaces (official boundary-loss, utils.py one_hot2dist and losses.py SurfaceLoss): per class k with membership target > 0.5,
//   phi = +dist(v, nearest voxel of the class)                  outside the class
//   phi = -(dist(v, nearest voxel not of the class) - offset)   inside the class
//   phi = 0 for the whole (n, k) volume where the opposite set is empty inside the patch (class absent, or class fills the patch)
// with Euclidean distances under the voxel spacing (sz, sy, sx), taken inside the patch only.
// DEVIATION from the official code: its inside branch is (posdist - 1), right at unit spacing only (at spacing 0.7 the innermost
// boundary voxel gets +0.3, the wrong sign).  Here `offset` is an argument and Python passes min(sz, sy, sx), the smallest distance
// an inside voxel can have: at unit spacing the official negdist * neg - (posdist - 1) * pos exactly, and never positive inside.
//
// The passes.  W: a wave per line turns the line's membership into 64-bit ballots and every lane finds the nearest member and the
// nearest non-member with clz / ctz (both polarities at once; uint16 offsets, 0xFFFF = none in this line).  H: the min-plus step
// g(i) = min_j f(j) + (s i - s j)^2 for both polarities, the source line passing through LDS kSdmTJ rows at a time so that global
// loads and stores run along W.  D: the same step for the ONE polarity the voxel's own membership selects, then sqrt, sign and
// offset; an infinite distance (the opposite set is empty) becomes 0, so the rule above needs no reduction and no host round trip.
// At unit spacing every squared distance is an integer below 2^24 (3 * 2047^2 < 2^24): fp32 is exact there.
#include "common.h"
#include "edt.h"
#include "loss_math.h"
#include "reduce.h"

namespace seg {

constexpr int kSdmThreads = 256;
static_assert(kSdmThreads == kReduceThreads, "the block size of reduce.h");
constexpr long long kSdmMaxVoxels = 2147483647LL;
constexpr int kSdmMaxAxis = 2047;                       // uint16 offsets with 0xFFFF free, and 3 * 2047^2 < 2^24
constexpr int kSdmMaxK = 16;
constexpr long long kSdmMaxTotal = 1LL << 56;            // N * K * S: what keeps every byte count inside 64 bits
constexpr long long kSdmMaxBlocks = 2147483647LL;       // one block per tile: a launch's grid limit
constexpr int kBoundaryMaxBlocks = 2048;
constexpr unsigned short kSdmNone = 0xFFFFu;

// pass W: one wave per line, the line's ballots in LDS
constexpr int kSdmLines = kSdmThreads / kWave;
constexpr int kSdmWords = (kSdmMaxAxis + kWave - 1) / kWave;
// passes H and D: a block owns kSdmTW columns and kSdmRows = kSdmRI * kSdmTY output rows (each thread kSdmRI rows of one column in
// registers); all 64 lanes of a wave read one LDS row of 64 consecutive floats: no bank conflict
constexpr int kSdmTW = 64, kSdmTY = kSdmThreads / kSdmTW, kSdmRI = 8, kSdmRows = kSdmRI * kSdmTY, kSdmTJ = 32;

__global__ __launch_bounds__(kSdmThreads) void sdm_pass_w_kernel(const float* __restrict__ target, long long lines, int Kp, int K, int c0,
        int DH, int W, unsigned short* __restrict__ off_m, unsigned short* __restrict__ off_n) {
    __shared__ unsigned long long sbits[kSdmLines][2][kSdmWords];
    const int nw = (W + kWave - 1) / kWave, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    unsigned long long* bm = sbits[wave][0];
    unsigned long long* bn = sbits[wave][1];
    const long long l = (long long)blockIdx.x * kSdmLines + wave;
    const bool live = l < lines;
    const long long o = live ? l / DH : 0, r = live ? l - o * DH : 0;          // o = n * Kp + k
    const float* __restrict__ src = target + (((o / Kp) * K + c0 + o % Kp) * DH + r) * W;
    for (int k = 0; k < nw; ++k) {
        const int x = k * kWave + lane;
        const bool in = live && x < W;
        const bool mem = in && src[x] > 0.5f;
        const unsigned long long b = __ballot(mem), v = __ballot(in);
        if (lane == 0) { bm[k] = b; bn[k] = v & ~b; }
    }
    __syncthreads();
    for (int p = 0; p < 2; ++p) {
        const unsigned long long* bits = p ? bn : bm;
        unsigned short* __restrict__ dst = (p ? off_n : off_m) + l * W;
        for (int k = 0; k < nw; ++k) {
            const int x = k * kWave + lane, best = nearest_set_bit(bits, nw, k, lane);
            if (live && x < W) dst[x] = best < 0 ? kSdmNone : (unsigned short)best;
        }
    }
}

__device__ __forceinline__ float sdm_load(const unsigned short* p, float s) {
    const unsigned short v = *p;
    const float d = s * (float)v;
    return v == kSdmNone ? INFINITY : d * d;
}
__device__ __forceinline__ float sdm_load(const float* p, float) { return *p; }

// sqrt(a) - offset rounded once, for a > 0: s = fl(sqrt(a)) carries up to half an ulp of sqrt(a), which the subtraction would turn
// into several ulps of the (smaller) difference.  So: the residual a - s^2 (exact, one fma) gives the correction c = (a - s^2) / 2s,
// s - offset is split into hi + lo without error (two-sum), and the three are added small to large.  fp32 only.  sqrtf is the
// correctly rounded one (hipcc's default; the __fsqrt_rn intrinsic is the 1-ulp native instruction in this toolchain).
__device__ __forceinline__ float sdm_sqrt_minus(float a, float offset) {
#pragma clang fp contract(off)
    const float s = sqrtf(a), c = fmaf(-s, s, a) / (2.f * s);
    const float hi = s - offset, bb = hi - s, lo = (s - (hi - bb)) + (-offset - bb);
    return fmaxf(hi + (lo + c), 0.f);           // (an inside voxel is at least `offset` from the outside: the rounding of `a` must not flip the sign)
}

// Passes H and D: g(i) = min_j f(j) + (s i - s j)^2 along an axis of `n` elements with element stride `stride`; `inner` contiguous
// columns share the axis, `outer` slabs of `outer_stride` elements repeat it.  in_m / in_n: the two polarities (nearest member,
// nearest non-member).  kLast = false writes both (out_m, out_n); kLast = true computes the polarity that target > 0.5 selects at
// the output voxel and writes phi.  One block per tile; tiles run columns fastest, slabs slowest.
template <typename InT, bool kLast>
__global__ __launch_bounds__(kSdmThreads) void sdm_pass_axis_kernel(const InT* __restrict__ in_m, const InT* __restrict__ in_n,
        float* __restrict__ out_m, float* __restrict__ out_n, const float* __restrict__ target, int Kp, int K, int c0,
        int n, long long stride, int inner, long long outer_stride, float s, float s_in, float offset) {
    const int tx = threadIdx.x % kSdmTW, ty = threadIdx.x / kSdmTW;
    const int ncb = (inner + kSdmTW - 1) / kSdmTW, nrb = (n + kSdmRows - 1) / kSdmRows;
    const long long b = blockIdx.x;
    const int cb = (int)(b % ncb);
    const long long q = b / ncb;
    const int rb = (int)(q % nrb);
    const long long o = q / nrb, base = o * outer_stride;
    const int col = cb * kSdmTW + tx, i0 = rb * kSdmRows + ty * kSdmRI;
    const bool live = col < inner;
    float acc[kLast ? 1 : 2][kSdmRI];       // kLast: the polarity mem[r] selects; else [0] member, [1] non-member
    bool mem[kSdmRI];
#pragma unroll
    for (int r = 0; r < kSdmRI; ++r) {
        mem[r] = false;
        if (kLast && live && i0 + r < n)
            mem[r] = target[((o / Kp) * K + c0 + o % Kp) * outer_stride + (long long)(i0 + r) * stride + col] > 0.5f;
    }
    const auto load = [=](int p, int j) { return live ? sdm_load((p ? in_n : in_m) + base + (long long)j * stride + col, s_in) : INFINITY; };
    minplus_axis<float, 2, kLast, kSdmTW, kSdmTY, kSdmTJ, kSdmRI>(acc, mem, load, n, s, i0, tx, ty);
    if (live) {
#pragma unroll
        for (int r = 0; r < kSdmRI; ++r) {
            if (i0 + r >= n) continue;
            const long long g = base + (long long)(i0 + r) * stride + col;
            if constexpr (kLast) {
                out_m[g] = acc[0][r] == INFINITY ? 0.f : (mem[r] ? -sdm_sqrt_minus(acc[0][r], offset) : sqrtf(acc[0][r]));
            } else {
                out_m[g] = acc[0][r];
                out_n[g] = acc[1][r];
            }
        }
    }
}

static int boundary_grid(long long items) { return stream_grid(items, kSdmThreads, kBoundaryMaxBlocks); }

// d sigmoid / dx = e / (1 + e)^2 with e = exp(-|x|): keeps its relative accuracy where 1 - p would round to 0
__device__ __forceinline__ float sigmoid_slope(float x) {
    const float e = expf(-fabsf(x)), q = 1.f + e;
    return e / (q * q);
}

// part[block] = sum sigmoid(logits[:, c0:]) * phi over this block's grid-stride walk
__global__ __launch_bounds__(kSdmThreads) void boundary_fwd_kernel(const float* __restrict__ x, const float* __restrict__ phi,
        long long n, long long KpS, long long KS, long long c0S, double* __restrict__ part) {
    double acc[1] = {0.0};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / KpS, src = b * KS + c0S + (i - b * KpS);
        acc[0] += (double)sigmoid(x[src]) * (double)phi[i];
    }
    block_sum(acc);
    if (threadIdx.x == 0) part[blockIdx.x] = acc[0];
}

// loss fp32[1] = sum / M, parts fp64[1] = the same in fp64, coef fp64[1] = 1 / M
__global__ __launch_bounds__(kSdmThreads) void boundary_finalize_kernel(const double* __restrict__ part, int nblk, long long M,
        float* __restrict__ loss, double* __restrict__ parts, double* __restrict__ coef) {
    double acc[1] = {0.0};
    partials_reduce<OpSum>(part, nblk, acc);
    block_sum(acc);
    if (threadIdx.x != 0) return;
    const double v = acc[0] / (double)M;
    loss[0] = (float)v;
    parts[0] = v;
    coef[0] = 1.0 / (double)M;
}

// dlogits[:, c0:] = gscale coef phi p (1 - p); channel 0 (when there is one) gets zeros.  V = 4: 16-byte accesses (S % 4 == 0, so a
// group of four never crosses a channel)
template <int V>
__global__ __launch_bounds__(kSdmThreads) void boundary_bwd_kernel(const float* __restrict__ x, const float* __restrict__ phi,
        const double* __restrict__ coef, const float* __restrict__ gscale, long long total, long long KpS, long long KS, long long c0S,
        float* __restrict__ dx) {
    const double gc = (double)gscale[0] * coef[0];
    const long long groups = total / V;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
        const long long o = g * V, b = o / KS, r = o - b * KS;
        float xv[V], pv[V], out[V];
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = 0.f;
        if (r >= c0S) {
            const long long i = b * KpS + (r - c0S);
            if constexpr (V == 4) {
                const float4 a = *reinterpret_cast<const float4*>(x + o), f = *reinterpret_cast<const float4*>(phi + i);
                xv[0] = a.x; xv[1] = a.y; xv[2] = a.z; xv[3] = a.w;
                pv[0] = f.x; pv[1] = f.y; pv[2] = f.z; pv[3] = f.w;
            } else {
                xv[0] = x[o]; pv[0] = phi[i];
            }
#pragma unroll
            for (int j = 0; j < V; ++j) out[j] = (float)(gc * (double)pv[j] * (double)sigmoid_slope(xv[j]));
        }
        if constexpr (V == 4) *reinterpret_cast<float4*>(dx + o) = make_float4(out[0], out[1], out[2], out[3]);
        else dx[o] = out[0];
    }
}

static bool boundary_aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

// the workspace of the map: uint16 offsets of pass W (member, non-member), then the fp32 squared distances of pass H (the same two)
struct SdmWs { unsigned short *off_m, *off_n; float *sq_m, *sq_n; size_t bytes; };
static SdmWs sdm_carve(void* ws, long long total) {
    Carver c{(char*)ws};
    SdmWs w;
    w.off_m = c.take<unsigned short>((size_t)total);
    w.off_n = c.take<unsigned short>((size_t)total);
    w.sq_m = c.take<float>((size_t)total);
    w.sq_n = c.take<float>((size_t)total);
    w.bytes = c.used();
    return w;
}

// blocks of the three launches: kSdmLines lines each, then one per (slab, row block, column block)
struct SdmGrid { long long w, h, d; };
static SdmGrid sdm_grid(long long NK, int D, int H, int W) {
    return {(NK * D * H + kSdmLines - 1) / kSdmLines, NK * D * cdiv(H, kSdmRows) * cdiv(W, kSdmTW),
            NK * cdiv(D, kSdmRows) * cdiv((long long)H * W, kSdmTW)};
}
static bool sdm_grid_ok(const SdmGrid& g) { return g.w <= kSdmMaxBlocks && g.h <= kSdmMaxBlocks && g.d <= kSdmMaxBlocks; }

static bool sdm_geom_ok(long long N, int K, int D, int H, int W) {
    return N > 0 && K >= 1 && K <= kSdmMaxK && D > 0 && H > 0 && W > 0 && D <= kSdmMaxAxis && H <= kSdmMaxAxis && W <= kSdmMaxAxis &&
           (long long)D * H * W <= kSdmMaxVoxels && N <= kSdmMaxTotal / K / ((long long)D * H * W) &&
           sdm_grid_ok(sdm_grid(N * (K - (K > 1 ? 1 : 0)), D, H, W));
}

}  // namespace seg

using namespace seg;

#define SDM_CHECK_GEOM(what)                                                                                                       \
    do {                                                                                                                           \
        SEG_CHECK_ARG(N > 0 && D > 0 && H > 0 && W > 0, what ": bad extents N=%lld D=%d H=%d W=%d", N, D, H, W);                   \
        SEG_CHECK_ARG(K >= 1 && K <= kSdmMaxK, what ": K must be in 1..%d, got %d", kSdmMaxK, K);                                  \
        SEG_CHECK_ARG(D <= kSdmMaxAxis && H <= kSdmMaxAxis && W <= kSdmMaxAxis, what ": an axis is longer than %d (D=%d H=%d W=%d)", \
                      kSdmMaxAxis, D, H, W);                                                                                       \
        SEG_CHECK_ARG((long long)D * H * W <= kSdmMaxVoxels, what ": more than 2^31 - 1 voxels per volume (D=%d H=%d W=%d)", D, H, W); \
        SEG_CHECK_ARG(N <= kSdmMaxTotal / K / ((long long)D * H * W), what ": N * K * D * H * W exceeds 2^56 (N=%lld K=%d)", N, K);   \
        SEG_CHECK_ARG(sdm_grid_ok(sdm_grid(N * (K - (K > 1 ? 1 : 0)), D, H, W)), what ": more than 2^31 - 1 tiles in one launch (N=%lld K=%d D=%d H=%d W=%d)", N, K, D, H, W); \
    } while (0)

#define BOUNDARY_CHECK_GEOM(what)                                                                                                  \
    do {                                                                                                                           \
        SEG_CHECK_ARG(N > 0 && S > 0, what ": bad extents N=%lld S=%lld", N, S);                                                    \
        SEG_CHECK_ARG(K >= 1 && K <= kSdmMaxK, what ": K must be in 1..%d, got %d", kSdmMaxK, K);                                  \
        SEG_CHECK_ARG(S <= kSdmMaxVoxels, what ": more than 2^31 - 1 voxels per volume (S=%lld)", S);                              \
    } while (0)

extern "C" {

size_t mi355seg_sdm_ws_bytes(long long N, int K, int D, int H, int W) {
    if (!sdm_geom_ok(N, K, D, H, W)) return 0;
    return sdm_carve(nullptr, N * (K - (K > 1 ? 1 : 0)) * D * H * W).bytes;
}

static int sdm_run(const float* target, long long N, int K, int D, int H, int W, float sz, float sy, float sx, float offset,
                   float* phi, void* ws, size_t ws_bytes, int steps, void* stream) {
    SDM_CHECK_GEOM("sdm");
    SEG_CHECK_ARG(sz > 0.f && sy > 0.f && sx > 0.f && sz < INFINITY && sy < INFINITY && sx < INFINITY,
                  "sdm: the spacing must be positive and finite, got (%g, %g, %g)", (double)sz, (double)sy, (double)sx);
    SEG_CHECK_ARG(offset >= 0.f && offset < INFINITY, "sdm: the offset must be >= 0 and finite, got %g", (double)offset);
    SEG_CHECK_ARG(steps >= 1 && steps <= 3, "sdm: steps must be in 1..3, got %d", steps);
    SEG_CHECK_ARG(target && phi && ws, "sdm: null pointer");
    SEG_CHECK_ARG(((uintptr_t)ws % 4) == 0, "sdm: the workspace must be 4-byte aligned");
    SEG_CHECK_WS(mi355seg_sdm_ws_bytes(N, K, D, H, W), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    const int c0 = K > 1 ? 1 : 0, Kp = K - c0;
    const long long S = (long long)D * H * W, NK = N * Kp, total = NK * S;
    const SdmWs w = sdm_carve(ws, total);
    ProfScope ps(PF_LOSS, 0.0, 32.0 * total, st);
    const SdmGrid grid = sdm_grid(NK, D, H, W);
    hipLaunchKernelGGL(sdm_pass_w_kernel, dim3((unsigned)grid.w), dim3(kSdmThreads), 0, st,
                       target, NK * D * H, Kp, K, c0, D * H, W, w.off_m, w.off_n);
    SEG_CHECK_LAUNCH();
    if (steps < 2) return MI355SEG_OK;
    hipLaunchKernelGGL((sdm_pass_axis_kernel<unsigned short, false>), dim3((unsigned)grid.h), dim3(kSdmThreads), 0, st,
                       (const unsigned short*)w.off_m, (const unsigned short*)w.off_n, w.sq_m, w.sq_n, (const float*)nullptr, Kp, K, c0,
                       H, (long long)W, W, (long long)H * W, sy, sx, 0.f);
    SEG_CHECK_LAUNCH();
    if (steps < 3) return MI355SEG_OK;
    hipLaunchKernelGGL((sdm_pass_axis_kernel<float, true>), dim3((unsigned)grid.d), dim3(kSdmThreads), 0, st,
                       (const float*)w.sq_m, (const float*)w.sq_n, phi, (float*)nullptr, target, Kp, K, c0,
                       D, (long long)H * W, H * W, S, sz, 0.f, offset);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int mi355seg_sdm_f32(const float* target, long long N, int K, int D, int H, int W, float sz, float sy, float sx, float offset,
                     float* phi, void* ws, size_t ws_bytes, void* stream) {
    return sdm_run(target, N, K, D, H, W, sz, sy, sx, offset, phi, ws, ws_bytes, 3, stream);
}

int mi355seg_sdm_steps_f32(const float* target, long long N, int K, int D, int H, int W, float sz, float sy, float sx, float offset,
                           float* phi, void* ws, size_t ws_bytes, int steps, void* stream) {
    return sdm_run(target, N, K, D, H, W, sz, sy, sx, offset, phi, ws, ws_bytes, steps, stream);
}

size_t mi355seg_boundary_ws_bytes(long long n) {
    if (n < 1) return 0;
    return (size_t)boundary_grid(n) * sizeof(double);
}

int mi355seg_boundary_fwd_f32(const float* logits, const float* phi, long long N, int K, long long S,
                              float* loss, double* parts, double* coef, void* ws, size_t ws_bytes, void* stream) {
    BOUNDARY_CHECK_GEOM("boundary_fwd");
    SEG_CHECK_ARG(logits && phi && loss && parts && coef && ws, "boundary_fwd: null pointer");
    SEG_CHECK_ARG(((uintptr_t)ws % 8) == 0, "boundary_fwd: the workspace must be 8-byte aligned");
    const int c0 = K > 1 ? 1 : 0;
    SEG_CHECK_ARG(N <= kSdmMaxTotal / K / S, "boundary_fwd: N * K * S exceeds 2^56 (N=%lld K=%d S=%lld)", N, K, S);
    const long long n = N * (K - c0) * S;
    SEG_CHECK_WS(mi355seg_boundary_ws_bytes(n), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, 8.0 * n, st);
    const int nblk = boundary_grid(n);
    hipLaunchKernelGGL(boundary_fwd_kernel, dim3(nblk), dim3(kSdmThreads), 0, st, logits, phi, n, (long long)(K - c0) * S, (long long)K * S,
                       (long long)c0 * S, (double*)ws);
    SEG_CHECK_LAUNCH();
    hipLaunchKernelGGL(boundary_finalize_kernel, dim3(1), dim3(kSdmThreads), 0, st, (const double*)ws, nblk, n, loss, parts, coef);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int mi355seg_boundary_bwd_f32(const float* logits, const float* phi, const double* coef, const float* gscale,
                              long long N, int K, long long S, float* dlogits, void* stream) {
    BOUNDARY_CHECK_GEOM("boundary_bwd");
    SEG_CHECK_ARG(logits && phi && coef && gscale && dlogits, "boundary_bwd: null pointer");
    SEG_CHECK_ARG(N <= kSdmMaxTotal / K / S, "boundary_bwd: N * K * S exceeds 2^56 (N=%lld K=%d S=%lld)", N, K, S);
    hipStream_t st = (hipStream_t)stream;
    const int c0 = K > 1 ? 1 : 0;
    const long long total = N * K * S, KpS = (long long)(K - c0) * S, KS = (long long)K * S, c0S = (long long)c0 * S;
    ProfScope ps(PF_LOSS, 0.0, 12.0 * total, st);
    if (S % 4 == 0 && boundary_aligned16(logits) && boundary_aligned16(phi) && boundary_aligned16(dlogits))
        hipLaunchKernelGGL(boundary_bwd_kernel<4>, dim3(boundary_grid(total / 4)), dim3(kSdmThreads), 0, st, logits, phi, coef, gscale, total, KpS, KS, c0S, dlogits);
    else
        hipLaunchKernelGGL(boundary_bwd_kernel<1>, dim3(boundary_grid(total)), dim3(kSdmThreads), 0, st, logits, phi, coef, gscale, total, KpS, KS, c0S, dlogits);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

}  // extern "C"
