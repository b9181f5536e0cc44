// aggregate.hip -- soft aggregation of sliding-window patches on the device: torchio's GridAggregator in its 'average' and 'hann'
// modes (predict.py:117 GridAggregator, :141 add_batch, :146 get_output_tensor), with any separable window the host hands over.
// The network's logits go in, the class probabilities are blended, the argmax comes last.
//
//   aggregate_patches   acc[k, v] = fmaf(w_p(v), softmax_k(logits_p(v)), acc[k, v]) for every patch p of the batch that covers the
//                       volume voxel v, IN ASCENDING PATCH INDEX (torchio's add_batch order).  One launch per batch.
//   aggregate_finalize  labels[v] = argmax_k acc[k, v]; prob[k, v] = acc[k, v] / ((sz[z] * sy[y]) * sx[x]).  One launch per volume.
//
// ORDER.  Rows of one batch may overlap each other, and a sum of floats depends on its order, so float atomics are out: the result
// would change from run to run and with the batch size.  Instead one thread stands for one (patch of the batch, patch voxel) and
// works only where its patch is the LOWEST-indexed patch of the batch that covers the volume voxel.  That thread reads the
// accumulator once, adds its own patch, walks the later patches of the batch in ascending index, adds those that cover the voxel,
// and writes the accumulator once.  Every accumulator element has exactly one writer per launch, launches on one stream are
// ordered, and batches hold ascending patch indices: per element the fmafs happen in ascending patch index whatever the batch
// size is, and two runs are bitwise equal.  No workgroup waits for another one.
//
// The softmax is fp32 with the maximum subtracted (exponents <= 0: logits of +-1e4 neither overflow nor give NaN); probabilities
// live in registers only.  The window weight of patch voxel (z, y, x) is (wz[z] * wy[y]) * wx[x], formed in that order.
//
// Rows along x are contiguous in logits and in acc.  Where the patch width and W are multiples of 4 and both bases are 16-byte
// aligned, a thread owns four consecutive x (128-bit loads and stores), provided every patch of the batch starts at an x that is
// a multiple of 4: then the four voxels are covered by the same patches.  A batch with another origin takes the same kernel one
// voxel at a time; every other shape takes the scalar kernel.  The arithmetic per element is the same in all three.
//
// MIRROR TEST-TIME AUGMENTATION (aggregate_patches_flip; not in the reference, whose predict.py:133 calls the model once per patch).
// The logits are those of a patch that was read mirrored (gather_patches_flip, api.hip), flip code 0..7: bit 2 mirrors z, bit 1 y,
// bit 0 x.  The FLIP instantiations un-mirror them as they read them -- softmax over logits[b, :, m_z(z), m_y(y), m_x(x)] -- while
// the weight and the destination keep (z, y, x); with the x bit a thread that owns four x loads the mirrored quad and reverses it in
// registers.  Everything else is the code above, so the result is bitwise aggregate_patches on flipped logits.  The caller loops
// over the flips OUTSIDE its walk of the grid: per element the order is (flip, patch), still independent of the batch size.
#include "common.h"
#include "internal.h"

namespace seg {

constexpr int kAggThreads = 256;
constexpr int kAggMaxK = 16;

static int agg_grid(long long items) { return stream_grid(items, kAggThreads, 8192); }

struct AggGeom {
    int K, first, count, pd, ph, pw, D, H, W;
    int flip;                                                 // read by the FLIP kernels only: bit 2 mirrors z, bit 1 y, bit 0 x
};

// origin of patch `first + c`, and whether the whole patch lies inside the volume (a row that does not is skipped: nothing is
// read or written outside the buffers whatever the table holds)
__device__ __forceinline__ bool agg_origin(const int* __restrict__ table, const AggGeom& g, int c, int& oz, int& oy, int& ox) {
    const int* t = table + (long long)(g.first + c) * 9;
    oz = t[0]; oy = t[1]; ox = t[2];
    return oz >= 0 && oy >= 0 && ox >= 0 && oz <= g.D - g.pd && oy <= g.H - g.ph && ox <= g.W - g.pw;
}

// acc[k] = fmaf(w, softmax_k, acc[k]) for V consecutive x of patch c at patch coordinates (z, y, x ..).
// FLIP: the logits are read at the mirrored coordinates (pd-1-z, ph-1-y, pw-1-x on the axes whose bit of g.flip is set); the window
// weight keeps (z, y, x).  With the x bit the V = 4 mirrored voxels are the aligned quad at pw-4-x, reversed in registers.
template <int KMAX, int V, bool FLIP>
__device__ __forceinline__ void agg_add(const float* __restrict__ logits, const AggGeom& g, int c, int z, int y, int x,
                                        const float* __restrict__ wz, const float* __restrict__ wy, const float* __restrict__ wx,
                                        float (&a)[KMAX][V]) {
    const long long S = (long long)g.pd * g.ph * g.pw;
    const bool rev = FLIP && (g.flip & 1);
    const int sz = FLIP && (g.flip & 4) ? g.pd - 1 - z : z, sy = FLIP && (g.flip & 2) ? g.ph - 1 - y : y, sx = rev ? g.pw - V - x : x;
    const float* p = logits + (long long)c * g.K * S + ((long long)sz * g.ph + sy) * g.pw + sx;
    float e[KMAX][V], m[V], s[V], w[V];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < g.K) {
            if constexpr (V == 4) {
                const f32x4_t v = ld4(p + (long long)k * S);
#pragma unroll
                for (int j = 0; j < V; ++j) e[k][j] = rev ? v[V - 1 - j] : v[j];
            } else {
                e[k][0] = p[(long long)k * S];
            }
        }
    }
    const float wzy = wz[z] * wy[y];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        w[j] = wzy * wx[x + j];
        m[j] = e[0][j];
    }
#pragma unroll
    for (int k = 1; k < KMAX; ++k)
        if (k < g.K) {
#pragma unroll
            for (int j = 0; j < V; ++j) m[j] = fmaxf(m[j], e[k][j]);
        }
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < g.K) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                e[k][j] = __expf(e[k][j] - m[j]);
                s[j] += e[k][j];
            }
        }
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = 1.f / s[j];            // s >= 1: the maximum contributes exp(0)
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < g.K) {
#pragma unroll
            for (int j = 0; j < V; ++j) a[k][j] = fmaf(w[j], e[k][j] * s[j], a[k][j]);
        }
}

// V consecutive x of patch b, starting at patch coordinates (z, y, x); all V volume voxels are covered by the same patches
template <int KMAX, int V, bool FLIP>
__device__ __forceinline__ void agg_voxels(const float* __restrict__ logits, const int* __restrict__ table, const AggGeom& g,
                                           int b, int z, int y, int x, const float* __restrict__ wz, const float* __restrict__ wy,
                                           const float* __restrict__ wx, float* __restrict__ acc) {
    int oz, oy, ox;
    if (!agg_origin(table, g, b, oz, oy, ox)) return;
    const int vz = oz + z, vy = oy + y, vx = ox + x;
    for (int c = 0; c < b; ++c) {                             // an earlier patch of the batch covers the voxel: it does the work
        int cz, cy, cx;
        if (!agg_origin(table, g, c, cz, cy, cx)) continue;
        if (vz >= cz && vz < cz + g.pd && vy >= cy && vy < cy + g.ph && vx >= cx && vx < cx + g.pw) return;
    }
    const long long VS = (long long)g.D * g.H * g.W;
    float* q = acc + ((long long)vz * g.H + vy) * g.W + vx;
    float a[KMAX][V];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < g.K) {
            if constexpr (V == 4) {
                const f32x4_t v = ld4(q + (long long)k * VS);
#pragma unroll
                for (int j = 0; j < V; ++j) a[k][j] = v[j];
            } else {
                a[k][0] = q[(long long)k * VS];
            }
        }
    }
    agg_add<KMAX, V, FLIP>(logits, g, b, z, y, x, wz, wy, wx, a);
    for (int c = b + 1; c < g.count; ++c) {                   // ascending patch index
        int cz, cy, cx;
        if (!agg_origin(table, g, c, cz, cy, cx)) continue;
        if (vz >= cz && vz < cz + g.pd && vy >= cy && vy < cy + g.ph && vx >= cx && vx < cx + g.pw)
            agg_add<KMAX, V, FLIP>(logits, g, c, vz - cz, vy - cy, vx - cx, wz, wy, wx, a);
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < g.K) {
            if constexpr (V == 4) st4(q + (long long)k * VS, f32x4_t{a[k][0], a[k][1], a[k][2], a[k][3]});
            else q[(long long)k * VS] = a[k][0];
        }
    }
}

template <int KMAX, int V, bool FLIP>
__global__ __launch_bounds__(kAggThreads) void aggregate_patches_kernel(const float* __restrict__ logits, const int* __restrict__ table,
        AggGeom g, const float* __restrict__ wz, const float* __restrict__ wy, const float* __restrict__ wx, float* __restrict__ acc) {
    const int xw = g.pw / V;                                  // V == 4: the host checked pw % 4 == 0
    const long long per = (long long)g.pd * g.ph * xw, total = per * g.count;
    bool quads = V == 4;
    if (V == 4)
        for (int c = 0; c < g.count; ++c) quads = quads && (table[(long long)(g.first + c) * 9 + 2] & 3) == 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / per);
        long long r = i - (long long)b * per;
        const int x = (int)(r % xw) * V; r /= xw;
        const int y = (int)(r % g.ph);
        const int z = (int)(r / g.ph);
        if (V == 1 || quads) {
            agg_voxels<KMAX, V, FLIP>(logits, table, g, b, z, y, x, wz, wy, wx, acc);
        } else {
            for (int j = 0; j < V; ++j) agg_voxels<KMAX, 1, FLIP>(logits, table, g, b, z, y, x + j, wz, wy, wx, acc);
        }
    }
}

// the comparison of argmax_kernel (loss.hip): first maximum wins, a NaN beats every number and the first NaN wins
__device__ __forceinline__ bool agg_first_gt(float v, float best) { return v > best || (v != v && best == best); }

template <int V, bool Prob>
__global__ __launch_bounds__(kAggThreads) void aggregate_finalize_kernel(const float* __restrict__ acc, int K, int D, int H, int W,
        const float* __restrict__ sz, const float* __restrict__ sy, const float* __restrict__ sx, long long* __restrict__ labels,
        float* __restrict__ prob) {
    const long long VS = (long long)D * H * W, total = VS / V;          // V == 4: the host checked W % 4 == 0
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long v = i * V;
        const int x = (int)(v % W);
        const long long r = v / W;
        const int y = (int)(r % H), z = (int)(r / H);
        float best[V], n[V];
        long long bi[V];
        const float szy = Prob ? sz[z] * sy[y] : 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) n[j] = Prob ? szy * sx[x + j] : 0.f;
        for (int k = 0; k < K; ++k) {
            float a[V];
            if constexpr (V == 4) {
                const f32x4_t t = ld4(acc + (long long)k * VS + v);
#pragma unroll
                for (int j = 0; j < V; ++j) a[j] = t[j];
            } else {
                a[0] = acc[(long long)k * VS + v];
            }
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (k == 0 || agg_first_gt(a[j], best[j])) { best[j] = a[j]; bi[j] = k; }
            if (Prob) {
                if constexpr (V == 4) st4(prob + (long long)k * VS + v, f32x4_t{a[0] / n[0], a[1] / n[1], a[2] / n[2], a[3] / n[3]});
                else prob[(long long)k * VS + v] = a[0] / n[0];
            }
        }
        if constexpr (V == 4) {
            *reinterpret_cast<longlong2*>(labels + v) = make_longlong2(bi[0], bi[1]);
            *reinterpret_cast<longlong2*>(labels + v + 2) = make_longlong2(bi[2], bi[3]);
        } else {
            labels[v] = bi[0];
        }
    }
}

}  // namespace seg

using namespace seg;

extern "C" {

// flip < 0: the un-mirrored kernels (the instantiations that never look at g.flip)
static int aggregate_patches_launch(const char* name, const float* logits, int K, const int* table, int first, int count, int pd, int ph,
                                    int pw, const float* wz, const float* wy, const float* wx, int flip, float* acc, int D, int H, int W,
                                    void* stream) {
    SEG_CHECK_ARG(K >= 2 && K <= kAggMaxK, "%s: K must lie in 2..%d, got %d", name, kAggMaxK, K);
    SEG_CHECK_ARG(count > 0 && first >= 0 && pd > 0 && ph > 0 && pw > 0, "%s: bad arguments (first %d, count %d, patch %dx%dx%d)", name,
                  first, count, pd, ph, pw);
    SEG_CHECK_ARG(pd <= D && ph <= H && pw <= W, "%s: patch %dx%dx%d larger than the volume %dx%dx%d", name, pd, ph, pw, D, H, W);
    SEG_CHECK_ARG(logits && table && wz && wy && wx && acc, "%s: null pointer", name);
    hipStream_t st = (hipStream_t)stream;
    const AggGeom g{K, first, count, pd, ph, pw, D, H, W, flip < 0 ? 0 : flip};
    const double per = (double)pd * ph * pw;
    // logits read, and one read and one write of the covered accumulator (counted as if no two patches of the batch overlapped)
    ProfScope ps(PF_LOSS, 0.0, 12.0 * K * count * per, st);
    const bool vec = pw % 4 == 0 && W % 4 == 0 && ((uintptr_t)logits | (uintptr_t)acc) % 16 == 0;
    const long long items = (long long)count * pd * ph * (vec ? pw / 4 : pw);
    const dim3 grid(agg_grid(items)), block(kAggThreads);
#define SEG_AGG_LAUNCH(KMAX, V, FLIP) \
    hipLaunchKernelGGL((aggregate_patches_kernel<KMAX, V, FLIP>), grid, block, 0, st, logits, table, g, wz, wy, wx, acc)
    if (flip < 0) {
        if (vec && K <= 4) SEG_AGG_LAUNCH(4, 4, false);
        else if (vec) SEG_AGG_LAUNCH(kAggMaxK, 4, false);
        else if (K <= 4) SEG_AGG_LAUNCH(4, 1, false);
        else SEG_AGG_LAUNCH(kAggMaxK, 1, false);
    } else {
        if (vec && K <= 4) SEG_AGG_LAUNCH(4, 4, true);
        else if (vec) SEG_AGG_LAUNCH(kAggMaxK, 4, true);
        else if (K <= 4) SEG_AGG_LAUNCH(4, 1, true);
        else SEG_AGG_LAUNCH(kAggMaxK, 1, true);
    }
#undef SEG_AGG_LAUNCH
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int mi355seg_aggregate_patches_f32(const float* logits, int K, const int* table, int first, int count, int pd, int ph, int pw,
                                   const float* wz, const float* wy, const float* wx, float* acc, int D, int H, int W, void* stream) {
    return aggregate_patches_launch("aggregate_patches", logits, K, table, first, count, pd, ph, pw, wz, wy, wx, -1, acc, D, H, W, stream);
}

int mi355seg_aggregate_patches_flip_f32(const float* logits, int K, const int* table, int first, int count, int pd, int ph, int pw,
                                        const float* wz, const float* wy, const float* wx, int flip, float* acc, int D, int H, int W,
                                        void* stream) {
    SEG_CHECK_ARG(flip >= 0 && flip <= 7, "aggregate_patches_flip: flip must lie in 0..7 (bit 2 z, bit 1 y, bit 0 x), got %d", flip);
    return aggregate_patches_launch("aggregate_patches_flip", logits, K, table, first, count, pd, ph, pw, wz, wy, wx, flip, acc, D, H, W,
                                    stream);
}

int mi355seg_aggregate_finalize_f32(const float* acc, int K, int D, int H, int W, const float* sz, const float* sy, const float* sx,
                                    int64_t* labels, float* prob, void* stream) {
    SEG_CHECK_ARG(K >= 2 && K <= kAggMaxK, "aggregate_finalize: K must lie in 2..%d, got %d", kAggMaxK, K);
    SEG_CHECK_ARG(D > 0 && H > 0 && W > 0, "aggregate_finalize: extents must be positive, got %d x %d x %d", D, H, W);
    SEG_CHECK_ARG(acc && labels && (!prob || (sz && sy && sx)), "aggregate_finalize: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const long long VS = (long long)D * H * W;
    ProfScope ps(PF_LOSS, 0.0, (4.0 * K + 8.0 + (prob ? 4.0 * K : 0.0)) * VS, st);
    const bool vec = W % 4 == 0 && ((uintptr_t)acc | (uintptr_t)labels | (uintptr_t)prob) % 16 == 0;
    const dim3 grid(agg_grid(vec ? VS / 4 : VS)), block(kAggThreads);
    long long* lab = (long long*)labels;
    if (vec && prob) hipLaunchKernelGGL((aggregate_finalize_kernel<4, true>), grid, block, 0, st, acc, K, D, H, W, sz, sy, sx, lab, prob);
    else if (vec) hipLaunchKernelGGL((aggregate_finalize_kernel<4, false>), grid, block, 0, st, acc, K, D, H, W, sz, sy, sx, lab, prob);
    else if (prob) hipLaunchKernelGGL((aggregate_finalize_kernel<1, true>), grid, block, 0, st, acc, K, D, H, W, sz, sy, sx, lab, prob);
    else hipLaunchKernelGGL((aggregate_finalize_kernel<1, false>), grid, block, 0, st, acc, K, D, H, W, sz, sy, sx, lab, prob);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

}  // extern "C"
