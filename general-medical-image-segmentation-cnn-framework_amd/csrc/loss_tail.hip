// loss_tail.hip -- the train step's tail for the compound losses (config.loss): a voxel term (BCE, focal, cross-entropy) plus a
// region term (Dice, Tversky), the argmax mask and the four Dice counters from ONE pass over logits and target, a one-block
// finalise that also forms the coefficients of the backward, and ONE backward pass.  Discipline of loss.hip: 256 threads, at most
// 2,048 blocks, grid-stride loop, per-thread fp64 accumulators, wavefront sum -> one LDS hop -> per-block partials, fixed-order
// fp64 / int64 finalise (here one block of 1,024 threads over all columns of the partial table at once), no atomics.
//
// The target comes in two forms, a float one-hot volume [N,K,S] or a uint8 label map [N,S] (config.multiclass).
// Both run ONE text: every kernel and every entry-point body below is written once and instantiated with OneHotTarget and with
// LabelTarget, which hold what differs (the forward's accumulator set, the one thing more, sits behind `if constexpr` in it).
//
// Reference: nn.BCEWithLogitsLoss train.py:115,209; cross_entropy_3D loss_function.py:8-16; DiceLoss loss_function.py:121-130;
// pred.argmax(dim=1, keepdim=True) train.py:204; metric() utils/metric.py:20-75.  Focal (Lin et al.) and Tversky (Salehi et al.)
// are the project's own definitions.
#include "common.h"
#include "loss_math.h"

namespace seg {

constexpr int kTailThreads = 256;
static_assert(kTailThreads == kReduceThreads, "the block size of reduce.h");
constexpr int kTailMaxBlocks = 2048;
constexpr int kTailMaxClasses = 16;
constexpr double kTailEps = 1e-5;            // DiceLoss.eplison, loss_function.py:119

enum { TAIL_V_NONE = 0, TAIL_V_BCE = 1, TAIL_V_FOCAL = 2, TAIL_V_CE = 3 };
enum { TAIL_R_NONE = 0, TAIL_R_DICE = 1, TAIL_R_TVERSKY = 2 };

static int tail_grid(long long items) { return stream_grid(items, kTailThreads, kTailMaxBlocks); }
static bool tail_aligned(const void* p, unsigned bytes) { return ((uintptr_t)p % bytes) == 0; }

// q^g for g = 1, 2 (exact products) or any g >= 1
__device__ __forceinline__ float tail_pow(float q, float g) { return g == 1.f ? q : (g == 2.f ? q * q : powf(q, g)); }
// q^(g-1), g >= 1
__device__ __forceinline__ float tail_pow_m1(float q, float g) { return g == 1.f ? 1.f : (g == 2.f ? q : powf(q, g - 1.f)); }

// V consecutive voxels of channel k: one 16-byte load for V = 4
template <int V>
__device__ __forceinline__ void tail_load(const float* __restrict__ p, float (&v)[V]) {
    if constexpr (V == 4) {
        const float4 a = *reinterpret_cast<const float4*>(p);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
        v[0] = p[0];
    }
}

// the labels of V consecutive voxels: one 4-byte load for V = 4
template <int V>
__device__ __forceinline__ void tail_load_lab(const uint8_t* __restrict__ p, int (&v)[V]) {
    if constexpr (V == 4) {
        const uint32_t a = *reinterpret_cast<const uint32_t*>(p);
        v[0] = a & 255u; v[1] = (a >> 8) & 255u; v[2] = (a >> 16) & 255u; v[3] = a >> 24;
    } else {
        v[0] = p[0];
    }
}

__device__ __forceinline__ float tail_opaque(float b) {
    asm("" : "+v"(b));
    return b;
}

// ----------------------------------------------------------------------------- the target policies
// A policy says what the kernels and the entry points below do not.  For the device: Elem (what the target pointer points to) and
// Voxels<KT, V>, what a thread holds of the target of its V voxels -- how it is loaded, value(k, j) (the target value b of class k),
// and the class of the four Dice counters and of the ce label, the NaN-first argmax of the column, as a running Best: first(j, K),
// then best = next(best, k, j) for k = 1 .. K-1.  For the host: the alignment rule and the bytes a launch moves.
//
// CONTRACT (4.22): for labels in [0, K) LabelTarget gives every output the bits OneHotTarget gives on onehot(labels); a label >= K
// is the all-zero column (argmax 0, member of no class).  The thread-to-voxel map, the per-thread accumulation order, the partial
// table and the finalise are shared by construction: there is one text.  What the label policy adds to that: value() passes
// b = (label == k) through tail_opaque, so that the compiler meets an unknown float where the one-hot form meets a load and forms
// the per-element expressions (and their fused multiply-adds) the same way.  Class membership is a comparison, never an index.

struct OneHotTarget {
    using Elem = float;                          // [N,K,S]
    static constexpr bool kLabels = false;
    // a misaligned pointer is served by the scalar path
    static constexpr bool kRefuseMisaligned = false;
    static bool aligned(const float* t) { return tail_aligned(t, 16); }
    static double fwd_bytes(int K) { return 8.0 * K + 8.0; }
    static double bwd_bytes(int K) { return 12.0 * K; }

    template <int KT, int V>
    struct Voxels {
        float tv[KT][V];
        struct Best { float v; int k; };
        const float* pt;                         // the next class of the thread's voxels
        // base: the offset of (n, class 0, s) in [N,K,S]
        __device__ __forceinline__ Voxels(const float* __restrict__ t, long long base, long long) : pt(t + base) {}
        // class k (called in the class loop, beside the load of the logits)
        __device__ __forceinline__ void load_class(int k, long long S) { tail_load<V>(pt, tv[k]); pt += S; }
        __device__ __forceinline__ void load_voxels() {}
        __device__ __forceinline__ float value(int k, int j) const { return tv[k][j]; }
        __device__ __forceinline__ Best first(int j, int K) const { return {tv[0][j], 0}; }
        __device__ __forceinline__ Best next(Best m, int k, int j) const {
            if (nan_first_gt(tv[k][j], m.v)) { m.v = tv[k][j]; m.k = k; }
            return m;
        }
    };
};

struct LabelTarget {
    using Elem = uint8_t;                        // [N,S]
    static constexpr bool kLabels = true;
    // the label form takes the path (16-byte or scalar) the one-hot form takes at the same S, or the bits would differ: where
    // S % 4 == 0 and K <= 4 a misaligned pointer is refused, not served by the other path
    static constexpr bool kRefuseMisaligned = true;
    static bool aligned(const uint8_t* t) { return tail_aligned(t, 4); }
    static double fwd_bytes(int K) { return 4.0 * K + 9.0; }
    static double bwd_bytes(int K) { return 8.0 * K + 1.0; }

    template <int KT, int V>
    struct Voxels {
        int lb[V];
        struct Best { int k; };
        const uint8_t* pv;                       // the labels of the thread's voxels
        // v0: the offset of (n, s) in [N,S]
        __device__ __forceinline__ Voxels(const uint8_t* __restrict__ t, long long, long long v0) : pv(t + v0) {}
        __device__ __forceinline__ void load_class(int, long long) {}
        // (called after the class loop)
        __device__ __forceinline__ void load_voxels() { tail_load_lab<V>(pv, lb); }
        __device__ __forceinline__ bool is(int k, int j) const { return lb[j] == k; }
        __device__ __forceinline__ float value(int k, int j) const { return tail_opaque(is(k, j) ? 1.f : 0.f); }
        __device__ __forceinline__ Best first(int j, int K) const { return {lb[j] < K ? lb[j] : 0}; }
        __device__ __forceinline__ Best next(Best m, int, int) const { return m; }
    };
};

// up to this capacity the label forward counts tp and pred itself; above it tail_lab_counts_kernel does, in a launch of its own
// (measured, DESIGN.md 4.22: inside the 16-slot kernel the two counters cost more than the two fp64 accumulators the label form drops)
#ifndef TAIL_LAB_FUSED_COUNT_MAX_KT
#define TAIL_LAB_FUSED_COUNT_MAX_KT 4
#endif
constexpr int kTailLabFusedCountMaxKT = TAIL_LAB_FUSED_COUNT_MAX_KT;

// KT: the compile-time class capacity (K == KT for KT <= 4, K <= KT above); V: voxels per thread and trip (4: 16-byte loads, needs
// S % 4 == 0 and aligned pointers).  part: per block 1 + 5 * K doubles (voxel-term sum; per class I, P, T, sum a^2, sum t^2);
// cpart: per block the four counters.
// The label form: sum t and sum t^2 are the integer gt_k, exact in fp64 in any order, so two of the five fp64 accumulators per class
// become one 32-bit counter, and the room goes to the class counters tp_k, pred_k (a thread sees fewer than 2^31 voxels; they are
// widened to int64 in the block reduction).  kpart: per block 3 K counters (per class tp, pred, gt; null for the one-hot form).
// CNT: tp and pred are counted here; without it this kernel fills only the gt column and tail_lab_counts_kernel, on the same grid,
// the two others (the 8- and 16-slot kernels run two wavefronts per SIMD and pay for every instruction).
template <int KT, int V, class Target, bool CNT>
__global__ __launch_bounds__(kTailThreads) void loss_tail_fwd_kernel(const float* __restrict__ x, const typename Target::Elem* __restrict__ t,
        long long N, int Krt, long long S, int vmode, float gamma, int64_t* __restrict__ mask,
        double* __restrict__ part, long long* __restrict__ cpart, long long* __restrict__ kpart) {
    constexpr bool kLab = Target::kLabels;
    constexpr int NS = kLab ? 3 : 5;             // one-hot: sum p t, sum p, sum t, sum p^2, sum t^2; labels: sum p t, sum p, sum p^2
    static_assert(kLab || !CNT, "the class counters belong to the label form");
    const int K = KT <= 4 ? KT : Krt;
    double vacc = 0.0;
    double sacc[KT][NS];
    unsigned kacc[KT][3];                        // labels: tp, pred, gt (tp and pred stay 0 without CNT)
#pragma unroll
    for (int k = 0; k < KT; ++k) {
#pragma unroll
        for (int j = 0; j < NS; ++j) sacc[k][j] = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) kacc[k][j] = 0u;
    }
    long long cacc[4] = {0, 0, 0, 0};
    const long long groups = N * S / V;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
        const long long v0 = g * V, n = v0 / S, s = v0 - n * S;
        const float* px = x + n * K * S + s;
        float xv[KT][V];
        typename Target::template Voxels<KT, V> tgt(t, n * K * S + s, v0);
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < K) { tail_load<V>(px, xv[k]); tgt.load_class(k, S); px += S; }
        tgt.load_voxels();
        long long mk[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            auto best = tgt.first(j, K);
            float bx = xv[0][j];
            int ix = 0;
            float l = 0.f;
#pragma unroll
            for (int k = 0; k < KT; ++k)
                if (k < K) {
                    const float a = xv[k][j], b = tgt.value(k, j);
                    if (k > 0) {
                        if (nan_first_gt(a, bx)) { bx = a; ix = k; }
                        best = tgt.next(best, k, j);
                    }
                    const float p = sigmoid(a);
                    sacc[k][0] += (double)(p * b); sacc[k][1] += (double)p;
                    if constexpr (kLab) {
                        sacc[k][2] += (double)(p * p);
                        kacc[k][2] += tgt.is(k, j);
                    } else {
                        sacc[k][2] += (double)b; sacc[k][3] += (double)(p * p); sacc[k][4] += (double)(b * b);
                    }
                    if (vmode == TAIL_V_BCE) {
                        l += bce_term(a, b);
                    } else if (vmode == TAIL_V_FOCAL) {
                        const float q = p + b - 2.f * p * b;
                        l += tail_pow(q, gamma) * bce_term(a, b);
                    }
                }
            const int it = best.k;
            if (vmode == TAIL_V_CE) {
                // logsumexp_k x - x[label], label = argmax_k t; log_softmax's order: rounds at the size of the term (ce3d_fwd_kernel)
                float m = -INFINITY, xl = xv[0][j];
#pragma unroll
                for (int k = 0; k < KT; ++k)
                    if (k < K) { m = fmaxf(m, xv[k][j]); if (k == it) xl = xv[k][j]; }
                float sum = 0.f;
#pragma unroll
                for (int k = 0; k < KT; ++k)
                    if (k < K) sum += expf(xv[k][j] - m);
                l = logf(sum) - (xl - m);
            }
            vacc += (double)l;
            mk[j] = ix;
            if constexpr (CNT) {
#pragma unroll
                for (int k = 0; k < KT; ++k)
                    if (k < K) { kacc[k][1] += (ix == k); kacc[k][0] += (ix == k && tgt.is(k, j)); }
            }
            cacc[0] += it; cacc[1] += ix;
            cacc[2] += ((it & ix) != 0); cacc[3] += ((it | ix) != 0);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) mask[v0 + j] = mk[j];
    }
    const int R = 1 + 5 * K;
    double* prow = part + (long long)blockIdx.x * R;
    long long* krow = kLab ? kpart + (long long)blockIdx.x * 3 * K : nullptr;
    double s = block_reduce_one<OpSum, true>(vacc);
    if (threadIdx.x == 0) prow[0] = s;
#pragma unroll
    for (int k = 0; k < KT; ++k)
        if (k < K) {
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                s = block_reduce_one<OpSum, true>(sacc[k][j]);
                if (threadIdx.x == 0) prow[1 + 5 * k + (kLab && j == 2 ? 3 : j)] = s;
            }
            if constexpr (kLab) {
#pragma unroll
                for (int j = CNT ? 0 : 2; j < 3; ++j) {
                    const long long c = block_reduce_one<OpSum, true>((long long)kacc[k][j]);
                    if (threadIdx.x == 0) {
                        krow[3 * k + j] = c;
                        if (j == 2) { prow[1 + 5 * k + 2] = (double)c; prow[1 + 5 * k + 4] = (double)c; }      // sum t = sum t^2 = gt_k
                    }
                }
            }
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long c = block_reduce_one<OpSum, true>(cacc[j]);
        if (threadIdx.x == 0) cpart[(long long)blockIdx.x * 4 + j] = c;
    }
}

// the tp and pred columns of kpart from the labels and the mask the forward wrote, for the label forwards without CNT: the same
// grid (block b fills row b, a block without voxels zeros)
template <int KT>
__global__ __launch_bounds__(kTailThreads) void tail_lab_counts_kernel(const uint8_t* __restrict__ lab, const int64_t* __restrict__ mask,
                                                                       long long n, int K, long long* __restrict__ kpart) {
    unsigned acc[KT][2];
#pragma unroll
    for (int k = 0; k < KT; ++k) { acc[k][0] = 0u; acc[k][1] = 0u; }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int lj = lab[i], ix = (int)mask[i];
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < K) { acc[k][1] += (ix == k); acc[k][0] += (ix == k && lj == k); }
    }
    long long* krow = kpart + (long long)blockIdx.x * 3 * K;
#pragma unroll
    for (int k = 0; k < KT; ++k)
        if (k < K) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const long long c = block_reduce_one<OpSum, true>((long long)acc[k][j]);
                if (threadIdx.x == 0) krow[3 * k + j] = c;
            }
        }
}

// One block of 1,024 threads.  Reduces the partials in a fixed order and writes loss (fp32), terms (fp64[2]: voxel, region,
// unweighted), sums (fp64[K][5]), counts (int64[4]) and coef (fp64[1 + 2 K]): coef[0] = w_v (the backward divides by M or V itself),
// coef[1 + 2k] = w_r * dRegion/dI_k, coef[2 + 2k] = w_r * dRegion/dP_k.
// A thread stands for (row group g, column j) of the partial table [nblk][R], R = 1 + 5 K: it adds the rows g, g + G, ... of its
// column (G = 1024 / R groups; neighbouring threads read neighbouring doubles), and column j's G group sums are then added in
// ascending g by one thread -- all columns at once, independent loads, one barrier; the counters likewise as 4 columns x 256 groups.
// CLS (the label form): the class counters' partial table kpart [nblk][3 K] is reduced beside the two others, the same way (3 K
// columns x 1024 / (3 K) groups, then one thread per column in ascending group), into class_counts int64[3 K].
constexpr int kTailFinThreads = 1024;
template <bool CLS>
__global__ __launch_bounds__(kTailFinThreads) void loss_tail_finalize_kernel(const double* __restrict__ part, const long long* __restrict__ cpart,
        const long long* __restrict__ kpart, int nblk, int K, int vmode, int rmode, double alpha, double beta, double wv, double wr,
        double M, double Vox, float* __restrict__ loss, double* __restrict__ terms, double* __restrict__ sums,
        int64_t* __restrict__ counts, double* __restrict__ coef, int64_t* __restrict__ class_counts) {
    __shared__ double red[kTailFinThreads];
    __shared__ long long redc[kTailFinThreads];
    __shared__ double tot[1 + 5 * kTailMaxClasses];
    if constexpr (CLS) {
        __shared__ long long redk[kTailFinThreads];
        const int C = 3 * K, GK = kTailFinThreads / C, jk = threadIdx.x % C, gk = threadIdx.x / C;
        long long ck = 0;
        if (gk < GK)
            for (int i = gk; i < nblk; i += GK) ck += kpart[(long long)i * C + jk];
        redk[threadIdx.x] = ck;
        __syncthreads();
        if (threadIdx.x >= 192 && threadIdx.x < 192 + C) {          // (a wavefront of its own, as the four counters below)
            const int col = threadIdx.x - 192;
            long long s = redk[col];
            for (int q = 1; q < GK; ++q) s += redk[q * C + col];
            class_counts[col] = s;
        }
    }
    const int R = 1 + 5 * K, G = kTailFinThreads / R;
    const int tid = threadIdx.x, j = tid % R, g = tid / R;
    double a = 0.0;
    if (g < G)
        for (int i = g; i < nblk; i += G) a += part[(long long)i * R + j];
    red[tid] = a;
    long long c = 0;
    for (int i = tid >> 2; i < nblk; i += kTailFinThreads / 4) c += cpart[(long long)i * 4 + (tid & 3)];
    redc[tid] = c;
    __syncthreads();
    if (tid < R) {
        double s = red[tid];
        for (int q = 1; q < G; ++q) s += red[q * R + tid];
        tot[tid] = s;
    } else if (tid >= 128 && tid < 132) {                 // (another wavefront: beside the sums above)
        long long s = redc[tid - 128];
        for (int q = 1; q < kTailFinThreads / 4; ++q) s += redc[q * 4 + tid - 128];
        counts[tid - 128] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int j = 0; j < 5 * K; ++j) sums[j] = tot[1 + j];
    const double div = vmode == TAIL_V_CE ? Vox : M;
    const double voxel = vmode == TAIL_V_NONE ? 0.0 : tot[0] / div;
    coef[0] = wv;
    double region = 0.0;
    if (rmode == TAIL_R_DICE) {
        // 1 - 2 (sum I + eps) / (sum P + sum T + eps), pooled over classes and samples (loss_function.py:121-130)
        double I = 0.0, P = 0.0, T = 0.0;
        for (int k = 0; k < K; ++k) { I += tot[1 + 5 * k]; P += tot[2 + 5 * k]; T += tot[3 + 5 * k]; }
        const double num = I + kTailEps, den = P + T + kTailEps;
        region = 1.0 - 2.0 * num / den;
        // ((2 num / den) / den: the order of torch's backward of the division in DiceLoss, see loss_tail_bwd_kernel)
        for (int k = 0; k < K; ++k) { coef[1 + 2 * k] = wr * (-2.0 / den); coef[2 + 2 * k] = wr * ((2.0 * num / den) / den); }
    } else if (rmode == TAIL_R_TVERSKY) {
        // 1 - (1/K) sum_k (I_k + eps) / (I_k + alpha (P_k - I_k) + beta (T_k - I_k) + eps)
        double acc = 0.0;
        const double c = 1.0 - alpha - beta;
        for (int k = 0; k < K; ++k) {
            const double I = tot[1 + 5 * k], P = tot[2 + 5 * k], T = tot[3 + 5 * k];
            const double num = I + kTailEps, den = c * I + alpha * P + beta * T + kTailEps;
            acc += num / den;
            coef[1 + 2 * k] = wr * (-(den - num * c) / (den * den)) / (double)K;
            coef[2 + 2 * k] = wr * (num * alpha / (den * den)) / (double)K;
        }
        region = 1.0 - acc / (double)K;
    } else {
        for (int k = 0; k < K; ++k) { coef[1 + 2 * k] = 0.0; coef[2 + 2 * k] = 0.0; }
    }
    terms[0] = voxel;
    terms[1] = region;
    loss[0] = (float)(wv * voxel + wr * region);
}

// a + b with both operands already rounded to fp32: the addition is not contracted with the product that formed an operand
__device__ __forceinline__ float tail_add_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// dlogits = gscale[0] * (w_v dVoxel/dx + w_r dRegion/dx), one pass: reads x and t, writes dx.
// The two terms' gradients are formed with the expressions and the scales of the kernels of the unfused criterion (bce_bwd_kernel,
// ce3d_bwd_kernel, dice_sums_bwd_kernel), each rounded to fp32, and then added, as autograd adds the gradients of two losses: at
// unit weights dice_bce and dice_ce give the BITS of DiceLoss + BCEWithLogitsLoss and cross_entropy_3D + DiceLoss.  That matters
// beyond tidiness: a network holds parameters whose exact gradient is zero (a convolution bias ahead of a BatchNorm), what a step
// returns for them is the rounding residue of the whole backward, and a last-bit change of dlogits redraws it.
template <int KT, int V, class Target>
__global__ __launch_bounds__(kTailThreads) void loss_tail_bwd_kernel(const float* __restrict__ x, const typename Target::Elem* __restrict__ t,
        const double* __restrict__ coef, const float* __restrict__ gscale, long long N, int Krt, long long S,
        int vmode, int rmode, float gamma, float* __restrict__ dx) {
    const int K = KT <= 4 ? KT : Krt;
    const double gs = (double)gscale[0];
    const float gw = gscale[0] * (float)coef[0];
    // bce_bwd_kernel: gscale / (float)numel; ce3d_bwd_kernel: gscale * (1.f / (float)voxels)
    const float sv = vmode == TAIL_V_CE ? gw * (1.f / (float)(N * S)) : gw / (float)(N * K * S);
    float cI[KT], cP[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        cI[k] = 0.f; cP[k] = 0.f;
        if (k < K) { cI[k] = (float)(gs * coef[1 + 2 * k]); cP[k] = (float)(gs * coef[2 + 2 * k]); }
    }
    const long long groups = N * S / V;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
        const long long v0 = g * V, n = v0 / S, s = v0 - n * S, base = n * K * S + s;
        const float* px = x + base;
        float* pd = dx + base;
        float xv[KT][V];
        typename Target::template Voxels<KT, V> tgt(t, base, v0);
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < K) { tail_load<V>(px, xv[k]); tgt.load_class(k, S); px += S; }
        tgt.load_voxels();
        float m[V], inv[V];
        int lab[V];
        if (vmode == TAIL_V_CE) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                auto best = tgt.first(j, K);
                float mm = -INFINITY;
#pragma unroll
                for (int k = 0; k < KT; ++k)
                    if (k < K) {
                        mm = fmaxf(mm, xv[k][j]);
                        if (k > 0) best = tgt.next(best, k, j);
                    }
                float sum = 0.f;
#pragma unroll
                for (int k = 0; k < KT; ++k)
                    if (k < K) sum += expf(xv[k][j] - mm);
                m[j] = mm; inv[j] = 1.f / sum; lab[j] = best.k;
            }
        }
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < K) {
                float o[V];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float a = xv[k][j], b = tgt.value(k, j);
                    const float p = sigmoid(a), dp = p * (1.f - p);
                    float d = 0.f;
                    if (vmode == TAIL_V_BCE) {
                        d = (p - b) * sv;
                    } else if (vmode == TAIL_V_FOCAL) {
                        const float q = p + b - 2.f * p * b;
                        d = (gamma * tail_pow_m1(q, gamma) * (1.f - 2.f * b) * dp * bce_term(a, b) + tail_pow(q, gamma) * (p - b)) * sv;
                    } else if (vmode == TAIL_V_CE) {
                        d = sv * (expf(a - m[j]) * inv[j] - (k == lab[j] ? 1.f : 0.f));
                    }
                    if (rmode != TAIL_R_NONE) {
                        const float dr = (cI[k] * b + cP[k]) * dp;
                        d = vmode == TAIL_V_NONE ? dr : tail_add_rounded(dr, d);
                    }
                    o[j] = d;
                }
                if constexpr (V == 4) *reinterpret_cast<float4*>(pd) = make_float4(o[0], o[1], o[2], o[3]);
                else pd[0] = o[0];
                pd += S;
            }
    }
}

// float label map -> uint8 labels; a value that is no integer in [0, K) is stored as 255 and counted.  The counter is touched only
// by a block that met such a value (one 64-bit integer add per block: the sum does not depend on the order).
template <int V>
__global__ __launch_bounds__(kTailThreads) void labels_u8_kernel(const float* __restrict__ gt, long long n, int K, uint8_t* __restrict__ out,
                                                                 unsigned long long* __restrict__ bad) {
    long long nb = 0;
    const float fk = (float)K;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n / V; g += (long long)gridDim.x * blockDim.x) {
        float v[V];
        tail_load<V>(gt + g * V, v);
        unsigned w = 0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const bool ok = v[j] >= 0.f && v[j] < fk && v[j] == truncf(v[j]);       // (a NaN fails the first comparison)
            nb += !ok;
            w |= (ok ? (unsigned)(int)v[j] : 255u) << (8 * j);
        }
        if constexpr (V == 4) *reinterpret_cast<uint32_t*>(out + g * 4) = w;
        else out[g] = (uint8_t)w;
    }
    const long long c = block_reduce_one<OpSum>(nb);
    if (threadIdx.x == 0 && c != 0) atomicAdd(bad, (unsigned long long)c);
}

// out[n][k][s] = (labels[n][s] == k), float
template <int V>
__global__ __launch_bounds__(kTailThreads) void onehot_u8_kernel(const uint8_t* __restrict__ lab, long long N, int K, long long S,
                                                                 float* __restrict__ out) {
    const long long groups = N * S / V;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
        const long long v0 = g * V, n = v0 / S, s = v0 - n * S;
        int lb[V];
        tail_load_lab<V>(lab + v0, lb);
        float* po = out + n * K * S + s;
        for (int k = 0; k < K; ++k, po += S) {
            if constexpr (V == 4) *reinterpret_cast<float4*>(po) = make_float4(lb[0] == k ? 1.f : 0.f, lb[1] == k ? 1.f : 0.f, lb[2] == k ? 1.f : 0.f, lb[3] == k ? 1.f : 0.f);
            else po[0] = lb[0] == k ? 1.f : 0.f;
        }
    }
}

// per class tp, pred, gt of two int64 label volumes; part [3 K][nblk] (one row per counter: the rows of sums_finalize_kernel)
template <int KT>
__global__ __launch_bounds__(kTailThreads) void class_counts_kernel(const int64_t* __restrict__ gt, const int64_t* __restrict__ pred,
                                                                    long long n, int K, long long* __restrict__ part) {
    unsigned acc[KT][3];
#pragma unroll
    for (int k = 0; k < KT; ++k) { acc[k][0] = 0u; acc[k][1] = 0u; acc[k][2] = 0u; }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long g = gt[i], p = pred[i];
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < K) { acc[k][0] += (g == k && p == k); acc[k][1] += (p == k); acc[k][2] += (g == k); }
    }
#pragma unroll
    for (int k = 0; k < KT; ++k)
        if (k < K) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const long long c = block_reduce_one<OpSum, true>((long long)acc[k][j]);
                if (threadIdx.x == 0) part[(long long)(3 * k + j) * gridDim.x + blockIdx.x] = c;
            }
        }
}

// ----------------------------------------------------------------------------- launch
template <int I>
using TailInt = std::integral_constant<int, I>;

static int tail_capacity(int K) { return K <= 4 ? K : (K <= 8 ? 8 : 16); }

// the runtime (class capacity, 16-byte path) as the compile-time <KT, V> of the tail kernels: f(TailInt<KT>, TailInt<V>).
// More than four classes: one voxel per thread (the 4-voxel form would spill), so `vec` is only ever set for KT <= 4.
template <class F>
static void tail_dispatch(int KT, bool vec, F f) {
    auto pick_v = [&](auto kt) { vec ? f(kt, TailInt<4>{}) : f(kt, TailInt<1>{}); };
    switch (KT) {
        case 1: pick_v(TailInt<1>{}); break;
        case 2: pick_v(TailInt<2>{}); break;
        case 3: pick_v(TailInt<3>{}); break;
        case 4: pick_v(TailInt<4>{}); break;
        case 8: f(TailInt<8>{}, TailInt<1>{}); break;
        default: f(TailInt<16>{}, TailInt<1>{}); break;
    }
}

// the counting kernels' slots for K classes: f(TailInt<4 | 8 | 16>)
template <class F>
static void tail_dispatch_slots(int K, F f) {
    if (K <= 4) f(TailInt<4>{});
    else if (K <= 8) f(TailInt<8>{});
    else f(TailInt<16>{});
}

static size_t tail_ws_bytes(long long N, int K, long long S, bool labels) {
    if (N < 1 || S < 1 || K < 1 || K > kTailMaxClasses) return 0;
    return (size_t)tail_grid(N * S) * ((size_t)(1 + 5 * K) * sizeof(double) + (size_t)(4 + (labels ? 3 * K : 0)) * sizeof(long long));
}

// the refusals that forward and backward share; `what` prefixes the message
static int tail_check_spec(const char* what, long long N, int K, long long S, int voxel_term, int region_term, float gamma) {
    SEG_CHECK_ARG(K >= 1 && K <= kTailMaxClasses, "%s: K must be in 1..%d, got %d", what, kTailMaxClasses, K);
    SEG_CHECK_ARG(voxel_term >= TAIL_V_NONE && voxel_term <= TAIL_V_CE, "%s: unknown voxel term %d (0 none, 1 bce, 2 focal, 3 ce)", what, voxel_term);
    SEG_CHECK_ARG(region_term >= TAIL_R_NONE && region_term <= TAIL_R_TVERSKY, "%s: unknown region term %d (0 none, 1 dice, 2 tversky)", what, region_term);
    SEG_CHECK_ARG(voxel_term != TAIL_V_NONE || region_term != TAIL_R_NONE, "%s: both terms absent", what);
    SEG_CHECK_ARG(voxel_term != TAIL_V_CE || K >= 2, "%s: the ce term needs K >= 2, got %d", what, K);
    SEG_CHECK_ARG(gamma == 0.f || (gamma >= 1.f && gamma <= 8.f), "%s: gamma must be 0 or in [1, 8], got %g", what, (double)gamma);
    SEG_CHECK_ARG(N > 0 && S > 0, "%s: bad extents N=%lld S=%lld", what, N, S);
    return MI355SEG_OK;
}

// The path of a launch: the class capacity, the 16-byte path (K <= 4, S % 4 == 0 and every pointer aligned; floats_aligned: the
// call's float pointers are) and the grid.  Where the policy says so, a misaligned pointer on that path is refused.
struct TailPath {
    int KT, nblk;
    bool vec;
};

template <class Target>
static int tail_path(const char* what, long long N, int K, long long S, bool floats_aligned, const typename Target::Elem* target, TailPath& p) {
    p.KT = tail_capacity(K);
    const bool fits = p.KT <= 4 && S % 4 == 0, aligned = floats_aligned && Target::aligned(target);
    SEG_CHECK_ARG(!(Target::kRefuseMisaligned && fits) || aligned,
                  "%s: with S %% 4 == 0 and K <= 4 the float pointers must be 16-byte and labels 4-byte aligned", what);
    p.vec = fits && aligned;
    p.nblk = tail_grid(p.vec ? N * S / 4 : N * S);
    return MI355SEG_OK;
}

// mi355seg_loss_tail_fwd_f32 and mi355seg_loss_tail_fwd_lab_f32 (class_counts: the label form's, null for the one-hot form)
template <class Target>
static int tail_forward(const char* what, const float* logits, const typename Target::Elem* target, long long N, int K, long long S,
                        int voxel_term, int region_term, float gamma, float alpha, float beta, float w_voxel, float w_region,
                        float* loss, double* terms, double* sums, int64_t* mask, int64_t* counts, double* coef,
                        int64_t* class_counts, void* ws, size_t ws_bytes, void* stream) {
    constexpr bool kLabels = Target::kLabels;
    if (int rc = tail_check_spec(what, N, K, S, voxel_term, region_term, gamma)) return rc;
    SEG_CHECK_ARG(alpha >= 0.f && beta >= 0.f, "%s: alpha and beta must be >= 0, got %g, %g", what, (double)alpha, (double)beta);
    SEG_CHECK_ARG(region_term != TAIL_R_TVERSKY || alpha + beta > 0.f, "%s: tversky needs alpha + beta > 0", what);
    SEG_CHECK_ARG(w_voxel >= 0.f && w_region >= 0.f, "%s: the weights must be >= 0, got %g, %g", what, (double)w_voxel, (double)w_region);
    SEG_CHECK_ARG(logits && target && loss && terms && sums && mask && counts && coef && (class_counts || !kLabels) && ws, "%s: null pointer", what);
    SEG_CHECK_ARG(tail_aligned(ws, 8), "%s: the workspace must be 8-byte aligned", what);
    SEG_CHECK_WS(tail_ws_bytes(N, K, S, kLabels), ws_bytes);
    TailPath p;
    if (int rc = tail_path<Target>(what, N, K, S, tail_aligned(logits, 16), target, p)) return rc;      // (the mask goes out in 8-byte stores)
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, Target::fwd_bytes(K) * N * S, st);
    if (voxel_term == TAIL_V_FOCAL && gamma == 0.f) voxel_term = TAIL_V_BCE;      // q^0 = 1: the bce code path
    const int nblk = p.nblk;
    double* part = (double*)ws;
    long long* cpart = (long long*)(part + (size_t)nblk * (1 + 5 * K));
    long long* kpart = kLabels ? cpart + (size_t)nblk * 4 : nullptr;
    tail_dispatch(p.KT, p.vec, [&](auto kt, auto v) {
        constexpr int KT = decltype(kt)::value, V = decltype(v)::value;
        hipLaunchKernelGGL((loss_tail_fwd_kernel<KT, V, Target, (kLabels && KT <= kTailLabFusedCountMaxKT)>), dim3(nblk), dim3(kTailThreads), 0, st,
                           logits, target, N, K, S, voxel_term, gamma, mask, part, cpart, kpart);
    });
    SEG_CHECK_LAUNCH();
    if constexpr (kLabels) {
        if (p.KT > kTailLabFusedCountMaxKT) {
            tail_dispatch_slots(K, [&](auto kt) {
                hipLaunchKernelGGL(tail_lab_counts_kernel<decltype(kt)::value>, dim3(nblk), dim3(kTailThreads), 0, st, target, (const int64_t*)mask, N * S, K, kpart);
            });
            SEG_CHECK_LAUNCH();
        }
    }
    hipLaunchKernelGGL(loss_tail_finalize_kernel<kLabels>, dim3(1), dim3(kTailFinThreads), 0, st, (const double*)part, (const long long*)cpart,
                       (const long long*)kpart, nblk, K, voxel_term, region_term, (double)alpha, (double)beta,
                       voxel_term == TAIL_V_NONE ? 0.0 : (double)w_voxel, region_term == TAIL_R_NONE ? 0.0 : (double)w_region,
                       (double)N * K * S, (double)N * S, loss, terms, sums, counts, coef, class_counts);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

// mi355seg_loss_tail_bwd_f32 and mi355seg_loss_tail_bwd_lab_f32
template <class Target>
static int tail_backward(const char* what, const float* logits, const typename Target::Elem* target, const double* coef, const float* gscale,
                         long long N, int K, long long S, int voxel_term, int region_term, float gamma, float* dlogits, void* stream) {
    if (int rc = tail_check_spec(what, N, K, S, voxel_term, region_term, gamma)) return rc;
    SEG_CHECK_ARG(logits && target && coef && gscale && dlogits, "%s: null pointer", what);
    TailPath p;
    if (int rc = tail_path<Target>(what, N, K, S, tail_aligned(logits, 16) && tail_aligned(dlogits, 16), target, p)) return rc;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, Target::bwd_bytes(K) * N * S, st);
    if (voxel_term == TAIL_V_FOCAL && gamma == 0.f) voxel_term = TAIL_V_BCE;
    tail_dispatch(p.KT, p.vec, [&](auto kt, auto v) {
        hipLaunchKernelGGL((loss_tail_bwd_kernel<decltype(kt)::value, decltype(v)::value, Target>), dim3(p.nblk), dim3(kTailThreads), 0, st,
                           logits, target, coef, gscale, N, K, S, voxel_term, region_term, gamma, dlogits);
    });
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

}  // namespace seg

using namespace seg;

extern "C" {

size_t mi355seg_loss_tail_ws_bytes(long long N, int K, long long S) { return tail_ws_bytes(N, K, S, false); }
size_t mi355seg_loss_tail_lab_ws_bytes(long long N, int K, long long S) { return tail_ws_bytes(N, K, S, true); }

int mi355seg_loss_tail_fwd_f32(const float* logits, const float* target, long long N, int K, long long S,
                               int voxel_term, int region_term, float gamma, float alpha, float beta, float w_voxel, float w_region,
                               float* loss, double* terms, double* sums, int64_t* mask, int64_t* counts, double* coef,
                               void* ws, size_t ws_bytes, void* stream) {
    return tail_forward<OneHotTarget>("loss_tail_fwd", logits, target, N, K, S, voxel_term, region_term, gamma, alpha, beta, w_voxel, w_region,
                                      loss, terms, sums, mask, counts, coef, nullptr, ws, ws_bytes, stream);
}

int mi355seg_loss_tail_fwd_lab_f32(const float* logits, const uint8_t* labels, long long N, int K, long long S,
                                   int voxel_term, int region_term, float gamma, float alpha, float beta, float w_voxel, float w_region,
                                   float* loss, double* terms, double* sums, int64_t* mask, int64_t* counts, double* coef,
                                   int64_t* class_counts, void* ws, size_t ws_bytes, void* stream) {
    return tail_forward<LabelTarget>("loss_tail_fwd_lab", logits, labels, N, K, S, voxel_term, region_term, gamma, alpha, beta, w_voxel, w_region,
                                     loss, terms, sums, mask, counts, coef, class_counts, ws, ws_bytes, stream);
}

int mi355seg_loss_tail_bwd_f32(const float* logits, const float* target, const double* coef, const float* gscale,
                               long long N, int K, long long S, int voxel_term, int region_term, float gamma,
                               float* dlogits, void* stream) {
    return tail_backward<OneHotTarget>("loss_tail_bwd", logits, target, coef, gscale, N, K, S, voxel_term, region_term, gamma, dlogits, stream);
}

int mi355seg_loss_tail_bwd_lab_f32(const float* logits, const uint8_t* labels, const double* coef, const float* gscale,
                                   long long N, int K, long long S, int voxel_term, int region_term, float gamma,
                                   float* dlogits, void* stream) {
    return tail_backward<LabelTarget>("loss_tail_bwd_lab", logits, labels, coef, gscale, N, K, S, voxel_term, region_term, gamma, dlogits, stream);
}

int mi355seg_labels_u8_f32(const float* gt, long long n, int K, uint8_t* labels_u8, int64_t* bad, void* stream) {
    SEG_CHECK_ARG(K >= 1 && K <= kTailMaxClasses, "labels_u8: K must be in 1..%d, got %d", kTailMaxClasses, K);
    SEG_CHECK_ARG(n > 0, "labels_u8: bad extent n=%lld", n);
    SEG_CHECK_ARG(gt && labels_u8 && bad, "labels_u8: null pointer");
    SEG_CHECK_ARG(tail_aligned(bad, 8), "labels_u8: the counter must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, 5.0 * n, st);
    const bool vec = n % 4 == 0 && tail_aligned(gt, 16) && tail_aligned(labels_u8, 4);
    if (vec) hipLaunchKernelGGL(labels_u8_kernel<4>, dim3(tail_grid(n / 4)), dim3(kTailThreads), 0, st, gt, n, K, labels_u8, (unsigned long long*)bad);
    else hipLaunchKernelGGL(labels_u8_kernel<1>, dim3(tail_grid(n)), dim3(kTailThreads), 0, st, gt, n, K, labels_u8, (unsigned long long*)bad);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int mi355seg_onehot_u8_f32(const uint8_t* labels_u8, long long N, int K, long long S, float* out, void* stream) {
    SEG_CHECK_ARG(K >= 1 && K <= kTailMaxClasses, "onehot_u8: K must be in 1..%d, got %d", kTailMaxClasses, K);
    SEG_CHECK_ARG(N > 0 && S > 0, "onehot_u8: bad extents N=%lld S=%lld", N, S);
    SEG_CHECK_ARG(labels_u8 && out, "onehot_u8: null pointer");
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, (4.0 * K + 1.0) * N * S, st);
    const bool vec = S % 4 == 0 && tail_aligned(out, 16) && tail_aligned(labels_u8, 4);
    if (vec) hipLaunchKernelGGL(onehot_u8_kernel<4>, dim3(tail_grid(N * S / 4)), dim3(kTailThreads), 0, st, labels_u8, N, K, S, out);
    else hipLaunchKernelGGL(onehot_u8_kernel<1>, dim3(tail_grid(N * S)), dim3(kTailThreads), 0, st, labels_u8, N, K, S, out);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

size_t mi355seg_class_counts_ws_bytes(long long n, int K) {
    if (n < 1 || K < 1 || K > kTailMaxClasses) return 0;
    return (size_t)tail_grid(n) * (size_t)(3 * K) * sizeof(long long);
}

int mi355seg_class_counts_i64(const int64_t* gt_labels, const int64_t* pred_labels, long long n, int K, int64_t* out,
                              void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(K >= 1 && K <= kTailMaxClasses, "class_counts: K must be in 1..%d, got %d", kTailMaxClasses, K);
    SEG_CHECK_ARG(n > 0, "class_counts: bad extent n=%lld", n);
    SEG_CHECK_ARG(gt_labels && pred_labels && out && ws, "class_counts: null pointer");
    SEG_CHECK_ARG(tail_aligned(ws, 8), "class_counts: the workspace must be 8-byte aligned");
    SEG_CHECK_WS(mi355seg_class_counts_ws_bytes(n, K), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, 16.0 * n, st);
    const int nblk = tail_grid(n);
    long long* part = (long long*)ws;
    tail_dispatch_slots(K, [&](auto kt) {
        hipLaunchKernelGGL(class_counts_kernel<decltype(kt)::value>, dim3(nblk), dim3(kTailThreads), 0, st, gt_labels, pred_labels, n, K, part);
    });
    SEG_CHECK_LAUNCH();
    launch_sums_finalize<1>((const long long*)part, nblk, (long long*)out, st, (unsigned)(3 * K));
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

}  // extern "C"
