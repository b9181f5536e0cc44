// loss_tail.hip -- the train step's tail for the compound losses (config.loss): a voxel term (BCE, focal, cross-entropy) plus a
// region term (Dice, Tversky), the argmax mask and the four Dice counters from ONE pass over logits and target, a one-block
// finalise that also forms the coefficients of the backward, and ONE backward pass.  Discipline of loss.hip: 256 threads, at most
// 2,048 blocks, grid-stride loop, per-thread fp64 accumulators, wavefront sum -> one LDS hop -> per-block partials, fixed-order
// fp64 / int64 finalise (here one block of 1,024 threads over all columns of the partial table at once), no atomics.
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

// KT: the compile-time class capacity (K == KT for KT <= 4, K <= KT above); V: voxels per thread and trip (4: 16-byte loads, needs
// S % 4 == 0 and aligned pointers).  part: per block 1 + 5 * K doubles (voxel-term sum; per class I, P, T, sum a^2, sum t^2);
// cpart: per block the four counters.
template <int KT, int V>
__global__ __launch_bounds__(kTailThreads) void loss_tail_fwd_kernel(const float* __restrict__ x, const float* __restrict__ t,
        long long N, int Krt, long long S, int vmode, float gamma, int64_t* __restrict__ mask,
        double* __restrict__ part, long long* __restrict__ cpart) {
    const int K = KT <= 4 ? KT : Krt;
    double vacc = 0.0;
    double sacc[KT][5];
#pragma unroll
    for (int k = 0; k < KT; ++k)
#pragma unroll
        for (int j = 0; j < 5; ++j) sacc[k][j] = 0.0;
    long long cacc[4] = {0, 0, 0, 0};
    const long long groups = N * S / V;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
        const long long v0 = g * V, n = v0 / S, s = v0 - n * S;
        const float* px = x + n * K * S + s;
        const float* pt = t + n * K * S + s;
        float xv[KT][V], tv[KT][V];
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < K) { tail_load<V>(px, xv[k]); tail_load<V>(pt, tv[k]); px += S; pt += S; }
        long long mk[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float bx = xv[0][j], bt = tv[0][j];
            int ix = 0, it = 0;
            float l = 0.f;
#pragma unroll
            for (int k = 0; k < KT; ++k)
                if (k < K) {
                    const float a = xv[k][j], b = tv[k][j];
                    if (k > 0) {
                        if (nan_first_gt(a, bx)) { bx = a; ix = k; }
                        if (nan_first_gt(b, bt)) { bt = b; it = k; }
                    }
                    const float p = sigmoid(a);
                    sacc[k][0] += (double)(p * b); sacc[k][1] += (double)p; sacc[k][2] += (double)b;
                    sacc[k][3] += (double)(p * p); sacc[k][4] += (double)(b * b);
                    if (vmode == TAIL_V_BCE) {
                        l += bce_term(a, b);
                    } else if (vmode == TAIL_V_FOCAL) {
                        const float q = p + b - 2.f * p * b;
                        l += tail_pow(q, gamma) * bce_term(a, b);
                    }
                }
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
            cacc[0] += it; cacc[1] += ix;
            cacc[2] += ((it & ix) != 0); cacc[3] += ((it | ix) != 0);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) mask[v0 + j] = mk[j];
    }
    const int R = 1 + 5 * K;
    double* prow = part + (long long)blockIdx.x * R;
    double s = block_reduce_one<OpSum, true>(vacc);
    if (threadIdx.x == 0) prow[0] = s;
#pragma unroll
    for (int k = 0; k < KT; ++k)
        if (k < K) {
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                s = block_reduce_one<OpSum, true>(sacc[k][j]);
                if (threadIdx.x == 0) prow[1 + 5 * k + j] = s;
            }
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long c = block_reduce_one<OpSum, true>(cacc[j]);
        if (threadIdx.x == 0) cpart[(long long)blockIdx.x * 4 + j] = c;
    }
}

// One block of 1,024 threads.  Reduces the partials in a fixed order and writes loss (fp32), terms (fp64[2]: voxel, region,
// unweighted), sums (fp64[K][5]), counts (int64[4]) and coef (fp64[1 + 2 K]): coef[0] = w_v (the backward divides by M or V itself),
// coef[1 + 2k] = w_r * dRegion/dI_k, coef[2 + 2k] = w_r * dRegion/dP_k.
// A thread stands for (row group g, column j) of the partial table [nblk][R], R = 1 + 5 K: it adds the rows g, g + G, ... of its
// column (G = 1024 / R groups; neighbouring threads read neighbouring doubles), and column j's G group sums are then added in
// ascending g by one thread -- all columns at once, independent loads, one barrier; the counters likewise as 4 columns x 256 groups.
constexpr int kTailFinThreads = 1024;
__global__ __launch_bounds__(kTailFinThreads) void loss_tail_finalize_kernel(const double* __restrict__ part, const long long* __restrict__ cpart,
        int nblk, int K, int vmode, int rmode, double alpha, double beta, double wv, double wr, double M, double Vox,
        float* __restrict__ loss, double* __restrict__ terms, double* __restrict__ sums, int64_t* __restrict__ counts,
        double* __restrict__ coef) {
    __shared__ double red[kTailFinThreads];
    __shared__ long long redc[kTailFinThreads];
    __shared__ double tot[1 + 5 * kTailMaxClasses];
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
template <int KT, int V>
__global__ __launch_bounds__(kTailThreads) void loss_tail_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t,
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
        const float* pt = t + base;
        float* pd = dx + base;
        float xv[KT][V], tv[KT][V];
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < K) { tail_load<V>(px, xv[k]); tail_load<V>(pt, tv[k]); px += S; pt += S; }
        float m[V], inv[V];
        int lab[V];
        if (vmode == TAIL_V_CE) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                float bt = tv[0][j], mm = -INFINITY;
                int it = 0;
#pragma unroll
                for (int k = 0; k < KT; ++k)
                    if (k < K) {
                        mm = fmaxf(mm, xv[k][j]);
                        if (k > 0 && nan_first_gt(tv[k][j], bt)) { bt = tv[k][j]; it = k; }
                    }
                float sum = 0.f;
#pragma unroll
                for (int k = 0; k < KT; ++k)
                    if (k < K) sum += expf(xv[k][j] - mm);
                m[j] = mm; inv[j] = 1.f / sum; lab[j] = it;
            }
        }
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < K) {
                float o[V];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float a = xv[k][j], b = tv[k][j];
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

static int tail_capacity(int K) { return K <= 4 ? K : (K <= 8 ? 8 : 16); }

template <int V>
static void tail_launch_fwd(int KT, int nblk, hipStream_t st, const float* x, const float* t, long long N, int K, long long S, int vmode,
                            float gamma, int64_t* mask, double* part, long long* cpart) {
#define TAIL_FWD(kt) hipLaunchKernelGGL((loss_tail_fwd_kernel<kt, V>), dim3(nblk), dim3(kTailThreads), 0, st, x, t, N, K, S, vmode, gamma, mask, part, cpart)
    switch (KT) {
        case 1: TAIL_FWD(1); break;
        case 2: TAIL_FWD(2); break;
        case 3: TAIL_FWD(3); break;
        case 4: TAIL_FWD(4); break;
        default:
            if constexpr (V == 1) {                       // more than four classes: one voxel per thread (the 4-voxel form would spill)
                if (KT == 8) TAIL_FWD(8); else TAIL_FWD(16);
            }
            break;
    }
#undef TAIL_FWD
}
template <int V>
static void tail_launch_bwd(int KT, int nblk, hipStream_t st, const float* x, const float* t, const double* coef, const float* gscale,
                            long long N, int K, long long S, int vmode, int rmode, float gamma, float* dx) {
#define TAIL_BWD(kt) hipLaunchKernelGGL((loss_tail_bwd_kernel<kt, V>), dim3(nblk), dim3(kTailThreads), 0, st, x, t, coef, gscale, N, K, S, vmode, rmode, gamma, dx)
    switch (KT) {
        case 1: TAIL_BWD(1); break;
        case 2: TAIL_BWD(2); break;
        case 3: TAIL_BWD(3); break;
        case 4: TAIL_BWD(4); break;
        default:
            if constexpr (V == 1) {                       // more than four classes: one voxel per thread (the 4-voxel form would spill)
                if (KT == 8) TAIL_BWD(8); else TAIL_BWD(16);
            }
            break;
    }
#undef TAIL_BWD
}

static bool tail_aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace seg

using namespace seg;

// the refusals that forward and backward share; `what` prefixes the message
#define TAIL_CHECK_SPEC(what)                                                                                                        \
    do {                                                                                                                             \
        SEG_CHECK_ARG(K >= 1 && K <= kTailMaxClasses, what ": K must be in 1..%d, got %d", kTailMaxClasses, K);                       \
        SEG_CHECK_ARG(voxel_term >= TAIL_V_NONE && voxel_term <= TAIL_V_CE, what ": unknown voxel term %d (0 none, 1 bce, 2 focal, 3 ce)", voxel_term); \
        SEG_CHECK_ARG(region_term >= TAIL_R_NONE && region_term <= TAIL_R_TVERSKY, what ": unknown region term %d (0 none, 1 dice, 2 tversky)", region_term); \
        SEG_CHECK_ARG(voxel_term != TAIL_V_NONE || region_term != TAIL_R_NONE, what ": both terms absent");                          \
        SEG_CHECK_ARG(voxel_term != TAIL_V_CE || K >= 2, what ": the ce term needs K >= 2, got %d", K);                               \
        SEG_CHECK_ARG(gamma == 0.f || (gamma >= 1.f && gamma <= 8.f), what ": gamma must be 0 or in [1, 8], got %g", (double)gamma);  \
        SEG_CHECK_ARG(N > 0 && S > 0, what ": bad extents N=%lld S=%lld", N, S);                                                     \
    } while (0)

extern "C" {

size_t mi355seg_loss_tail_ws_bytes(long long N, int K, long long S) {
    if (N < 1 || S < 1 || K < 1 || K > kTailMaxClasses) return 0;
    return (size_t)tail_grid(N * S) * ((size_t)(1 + 5 * K) * sizeof(double) + 4 * sizeof(long long));
}

int mi355seg_loss_tail_fwd_f32(const float* logits, const float* target, long long N, int K, long long S,
                               int voxel_term, int region_term, float gamma, float alpha, float beta, float w_voxel, float w_region,
                               float* loss, double* terms, double* sums, int64_t* mask, int64_t* counts, double* coef,
                               void* ws, size_t ws_bytes, void* stream) {
    TAIL_CHECK_SPEC("loss_tail_fwd");
    SEG_CHECK_ARG(alpha >= 0.f && beta >= 0.f, "loss_tail_fwd: alpha and beta must be >= 0, got %g, %g", (double)alpha, (double)beta);
    SEG_CHECK_ARG(region_term != TAIL_R_TVERSKY || alpha + beta > 0.f, "loss_tail_fwd: tversky needs alpha + beta > 0");
    SEG_CHECK_ARG(w_voxel >= 0.f && w_region >= 0.f, "loss_tail_fwd: the weights must be >= 0, got %g, %g", (double)w_voxel, (double)w_region);
    SEG_CHECK_ARG(logits && target && loss && terms && sums && mask && counts && coef && ws, "loss_tail_fwd: null pointer");
    SEG_CHECK_ARG(((uintptr_t)ws % 8) == 0, "loss_tail_fwd: the workspace must be 8-byte aligned");
    SEG_CHECK_WS(mi355seg_loss_tail_ws_bytes(N, K, S), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, (8.0 * K + 8.0) * N * S, st);
    if (voxel_term == TAIL_V_FOCAL && gamma == 0.f) voxel_term = TAIL_V_BCE;      // q^0 = 1: the bce code path
    const int KT = tail_capacity(K);
    const bool vec = KT <= 4 && S % 4 == 0 && tail_aligned16(logits) && tail_aligned16(target);       // (the mask goes out in 8-byte stores)
    const int nblk = tail_grid(vec ? N * S / 4 : N * S);
    double* part = (double*)ws;
    long long* cpart = (long long*)(part + (size_t)nblk * (1 + 5 * K));
    if (vec) tail_launch_fwd<4>(KT, nblk, st, logits, target, N, K, S, voxel_term, gamma, mask, part, cpart);
    else tail_launch_fwd<1>(KT, nblk, st, logits, target, N, K, S, voxel_term, gamma, mask, part, cpart);
    SEG_CHECK_LAUNCH();
    hipLaunchKernelGGL(loss_tail_finalize_kernel, dim3(1), dim3(kTailFinThreads), 0, st, (const double*)part, (const long long*)cpart, nblk, K,
                       voxel_term, region_term, (double)alpha, (double)beta, voxel_term == TAIL_V_NONE ? 0.0 : (double)w_voxel,
                       region_term == TAIL_R_NONE ? 0.0 : (double)w_region, (double)N * K * S, (double)N * S, loss, terms, sums, counts, coef);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int mi355seg_loss_tail_bwd_f32(const float* logits, const float* target, const double* coef, const float* gscale,
                               long long N, int K, long long S, int voxel_term, int region_term, float gamma,
                               float* dlogits, void* stream) {
    TAIL_CHECK_SPEC("loss_tail_bwd");
    SEG_CHECK_ARG(logits && target && coef && gscale && dlogits, "loss_tail_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, 12.0 * K * N * S, st);
    if (voxel_term == TAIL_V_FOCAL && gamma == 0.f) voxel_term = TAIL_V_BCE;
    const int KT = tail_capacity(K);
    const bool vec = KT <= 4 && S % 4 == 0 && tail_aligned16(logits) && tail_aligned16(target) && tail_aligned16(dlogits);
    const int nblk = tail_grid(vec ? N * S / 4 : N * S);
    if (vec) tail_launch_bwd<4>(KT, nblk, st, logits, target, coef, gscale, N, K, S, voxel_term, region_term, gamma, dlogits);
    else tail_launch_bwd<1>(KT, nblk, st, logits, target, coef, gscale, N, K, S, voxel_term, region_term, gamma, dlogits);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

}  // extern "C"
