// intensity.hip -- per-volume intensity normalisation beyond the plain z-score (config.intensity): exact percentiles of a volume by
// radix select, moments of the mapped masked voxels, and the piecewise-linear map itself.  The reference's dataloader.py:19 imports
// RescaleIntensity and HistogramStandardization beside ZNormalization and wires neither in; UNPINNED, as the rest of the data path:
// the definitions in include/mi355seg.h ("Intensity normalisation") are the specification.
//
// (a) Percentiles.  Every fp32 voxel becomes an order-preserving 32-bit key (-0.0 -> +0.0, then: sign bit flipped for non-negatives,
//     all bits flipped for negatives), and the requested order statistics are found most-significant digit first in FOUR passes of
//     8 bits.  Why 8/8/8/8: passes 2-4 keep one 256-bin histogram per distinct key prefix still alive, and 2 * 16 ranks can be alive at
//     once: 32 * 256 * 4 B = 32 KB of LDS per workgroup, so four workgroups fit a CU's 160 KB (11/11/10 would need 32 * 2048 * 4 B
//     = 256 KB, 14/9/9 leaves two workgroups per CU and needs a 16,384-bin scan).  A pass is one histogram launch over the volume and
//     one single-workgroup launch that scans the histograms (a wave each, shuffles only), moves every rank into its bin
//     (prefix <<= 8 | bin, rank -= bins below) and lists the distinct prefixes for the next pass; the first scan also forms the
//     ranks from the masked count m (the total of the first histogram), in fp64, on the device.  Nine launches (one memset), no
//     host round trip.
//     Counts are integers throughout: LDS histogram per workgroup by LDS integer atomics, then one global integer atomicAdd per
//     non-zero bin -- exact, so bitwise reproducible; no float atomics, and no workgroup waits for another.
//     A medical volume is mostly ONE value (air), so all 64 lanes of a wave hit one bin in every pass: each wave therefore compares
//     its lanes' bins against the first live lane's (ballot) and adds the popcount once, twice over; only what is left after those
//     two rounds goes to LDS one atomic per lane.  A voxel finds its prefix through a 256-entry table on the prefix's last digit
//     (1 KB of LDS more), so the search does not grow with the number of ranks, and every thread has four 16-byte loads in flight
//     before it uses the first (one workgroup's tile: 4,096 voxels).
// (b) Moments: count, sum and sum of squares of map(x) - pivot over the voxels with x > mask_gt, fp64, block partials in a fixed order
//     and a one-block finalise (the form of znorm_sums_kernel; no atomics).
// (c) Map: x' = min(max(x, clip_lo), clip_hi); j = number of interior knots kx[1 .. nk-2] that are <= x';
//          y = fmaf(x' - kx[j], slope[j], ky[j])
//     in fp32: the subtraction rounds once, the multiply-add is FUSED (one rounding).  16-byte loads and stores, in place allowed.
//     Instantiated for nk = 2 (rescale, clip + z-score) and nk = 11 (Nyul) with the knot search unrolled over kernel arguments; any
//     other nk in 2 .. 12 takes the run-time loop.
#include "common.h"

namespace seg {

constexpr int kIntThreads = 256;
static_assert(kIntThreads == kReduceThreads, "the block size of reduce.h");
constexpr int kSelMaxBlocks = 1024;          // every workgroup flushes up to 32 * 256 bins: four workgroups per CU is all it takes
constexpr int kSelBins = 256;
constexpr int kSelUnroll = 4;                // 16-byte loads in flight per thread
constexpr int kSelTile = kIntThreads * kSelUnroll * 4;       // voxels of one workgroup's trip
constexpr int kSelMaxQ = MI355SEG_PERCENTILES_MAX;
constexpr int kSelMaxRanks = 2 * kSelMaxQ;
constexpr int kMomMaxBlocks = 2048;
static_assert(kSelMaxRanks == 32 && kSelBins == 256, "four bins per lane in the scan; 32 KB of LDS per histogram workgroup, one filter entry per thread");

static int int_grid(long long items, int cap) { return stream_grid(items, kIntThreads, cap); }

// ------------------------------------------------------------------------------------------------ (a) radix select
__device__ __forceinline__ unsigned sel_key(float v) {
    unsigned u = __builtin_bit_cast(unsigned, v);
    if (u == 0x80000000u) u = 0u;                            // -0.0 sorts with +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sel_unkey(unsigned k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ bool sel_nonfinite(float v) { return (__builtin_bit_cast(unsigned, v) & 0x7f800000u) == 0x7f800000u; }

// the chain's device state (zeroed with the histograms before the first pass)
struct SelState {
    unsigned long long nonfinite;
    unsigned m;                              // masked, finite voxels
    unsigned nu;                             // distinct prefixes alive
    unsigned uprefix[kSelMaxRanks];          // their values (the key's bits above the current digit)
    unsigned prefix[kSelMaxRanks];           // per rank
    unsigned rank[kSelMaxRanks];             // per rank: what is left of it inside its prefix
    unsigned slot[kSelMaxRanks];             // per rank: index of its prefix in uprefix
    double t[kSelMaxQ];                      // per percentile: fractional part of its position
};
struct SelQ { double q[kSelMaxQ]; int nq; };

// Add one count per lane to sh[idx] (idx < 0: nothing).  The whole wave must call it together.  Two rounds of "who shares the first
// live lane's bin" take the equal lanes out with ONE LDS atomic each (the second is skipped once no lane is left); the rest add
// singly.  Four rounds measured slower on the Gaussian and on the 70 %-one-value volume (+6 % and +4 % on the chain at 256^3).
__device__ __forceinline__ void wave_hist_add(unsigned* sh, int idx) {
    const int lane = threadIdx.x & 63;
    unsigned long long live = __ballot(idx >= 0);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (!live) return;                                   // wave-uniform
        const int leader = __ffsll((long long)live) - 1;
        const int lidx = __shfl(idx, leader, 64);
        const unsigned long long same = __ballot(idx == lidx);
        if (lane == leader) atomicAdd(&sh[lidx], (unsigned)__popcll(same));
        if (idx == lidx) idx = -1;
        live &= ~same;
    }
    if (idx >= 0) atomicAdd(&sh[idx], 1u);
}

// bin of one voxel in the current pass, -1 when it takes no part: masked out, non-finite, or under no live prefix.  filt[d] holds the
// live prefixes whose LAST digit is d as a bit mask, so a voxel costs one LDS read unless it shares that digit with a live prefix
// (in the second pass the last digit is the whole prefix): the cost does not grow with the number of percentiles.
template <bool FIRST>
__device__ __forceinline__ int sel_bin(float v, bool valid, int use_mask, float mask_gt, int shift, const unsigned* filt, const unsigned* up, unsigned& nonfin) {
    if (!valid) return -1;
    if (sel_nonfinite(v)) { nonfin += 1u; return -1; }
    if (use_mask && !(v > mask_gt)) return -1;
    const unsigned k = sel_key(v);
    if (FIRST) return (int)(k >> 24);
    const unsigned pk = k >> (shift + 8);
    unsigned cand = filt[pk & 255u];
    int s = -1;
    while (cand) {                                           // the prefixes are distinct: at most one matches
        const int u = __ffs((int)cand) - 1;
        cand &= cand - 1u;
        s = (up[u] == pk) ? u : s;
    }
    return s < 0 ? -1 : s * kSelBins + (int)((k >> shift) & 255u);
}

// one histogram pass: digit (key >> shift) & 255 of the voxels under each live prefix (FIRST: of every masked voxel, shift = 24).
// A workgroup's tile is kSelTile voxels: kSelUnroll independent 16-byte loads per thread are in flight before the first is used.
template <bool FIRST>
__global__ __launch_bounds__(kIntThreads) void sel_hist_kernel(const float* __restrict__ x, long long n, int use_mask, float mask_gt,
                                                                int shift, SelState* __restrict__ st, unsigned* __restrict__ ghist) {
    __shared__ unsigned sh[FIRST ? kSelBins : kSelMaxRanks * kSelBins];
    __shared__ unsigned up[kSelMaxRanks];
    __shared__ unsigned filt[kSelBins];
    int nu = 1;
    if (!FIRST) {
        nu = (int)st->nu;
        nu = nu > kSelMaxRanks ? kSelMaxRanks : nu;
        if (threadIdx.x < kSelMaxRanks) up[threadIdx.x] = st->uprefix[threadIdx.x];
        filt[threadIdx.x] = 0u;
    }
    for (int i = threadIdx.x; i < nu * kSelBins; i += kIntThreads) sh[i] = 0u;
    __syncthreads();
    if (!FIRST) {
        if ((int)threadIdx.x < nu) atomicOr(&filt[up[threadIdx.x] & 255u], 1u << threadIdx.x);
        __syncthreads();
    }
    unsigned nonfin = 0u;
    const long long n4 = n / 4;
    // the trip count is the same for every thread of the workgroup: the ballots inside need whole waves
    for (long long base = (long long)blockIdx.x * (kIntThreads * kSelUnroll); base < n4; base += (long long)gridDim.x * (kIntThreads * kSelUnroll)) {
        float4 v[kSelUnroll];
        bool valid[kSelUnroll];
#pragma unroll
        for (int u = 0; u < kSelUnroll; ++u) {
            const long long i = base + u * kIntThreads + threadIdx.x;
            valid[u] = i < n4;
            v[u] = valid[u] ? reinterpret_cast<const float4*>(x)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        int idx[4 * kSelUnroll];                             // every bin first (independent table reads), then the wave-wide adds
#pragma unroll
        for (int u = 0; u < kSelUnroll; ++u) {
            idx[4 * u] = sel_bin<FIRST>(v[u].x, valid[u], use_mask, mask_gt, shift, filt, up, nonfin);
            idx[4 * u + 1] = sel_bin<FIRST>(v[u].y, valid[u], use_mask, mask_gt, shift, filt, up, nonfin);
            idx[4 * u + 2] = sel_bin<FIRST>(v[u].z, valid[u], use_mask, mask_gt, shift, filt, up, nonfin);
            idx[4 * u + 3] = sel_bin<FIRST>(v[u].w, valid[u], use_mask, mask_gt, shift, filt, up, nonfin);
        }
#pragma unroll
        for (int e = 0; e < 4 * kSelUnroll; ++e) wave_hist_add(sh, idx[e]);
    }
    if (blockIdx.x == 0) {                                   // the n % 4 tail, as znorm_sums_kernel: the first threads of block 0
        const bool valid = threadIdx.x < (unsigned)(n & 3);
        const float v = valid ? x[n4 * 4 + threadIdx.x] : 0.f;
        wave_hist_add(sh, sel_bin<FIRST>(v, valid, use_mask, mask_gt, shift, filt, up, nonfin));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nu * kSelBins; i += kIntThreads) {
        const unsigned c = sh[i];
        if (c) atomicAdd(&ghist[i], c);
    }
    if (FIRST) {
        const long long w = wave_sum((long long)nonfin);
        if ((threadIdx.x & 63) == 0 && w) atomicAdd(&st->nonfinite, (unsigned long long)w);
    }
}

// inclusive scan of one 256-bin histogram by ONE wave: lane l holds bins 4 l .. 4 l + 3 (c: the counts, incl: their inclusive
// prefix sums over the whole histogram); returns the total.  Shuffles only: no barrier, so the waves of the scan kernel work on
// different histograms side by side.
__device__ __forceinline__ unsigned wave_scan_bins(const unsigned* __restrict__ h, int lane, unsigned (&c)[4], unsigned (&incl)[4]) {
    const uint4 q = reinterpret_cast<const uint4*>(h)[lane];
    c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
    incl[0] = c[0]; incl[1] = incl[0] + c[1]; incl[2] = incl[1] + c[2]; incl[3] = incl[2] + c[3];
    unsigned run = incl[3];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned a = __shfl_up(run, o, 64);
        if (lane >= o) run += a;
    }
    const unsigned before = run - incl[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) incl[j] += before;
    return __shfl(run, 63, 64);
}

// after pass `pass` (0 .. 3): scan the histograms (one wave each), move every rank into its bin, list the distinct prefixes; the
// last one writes the results.  One workgroup of kScanThreads threads.
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void sel_scan_kernel(int pass, SelQ q, SelState* __restrict__ st, const unsigned* __restrict__ ghist,
                                                                 double* __restrict__ values, float* __restrict__ order, long long* __restrict__ counts) {
    __shared__ unsigned rk[kSelMaxRanks], pf[kSelMaxRanks], sl[kSelMaxRanks], nrk[kSelMaxRanks], npf[kSelMaxRanks];
    __shared__ unsigned sh_m, sh_nu;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, R = 2 * q.nq;
    const int nslots = pass == 0 ? 1 : (int)(st->nu > (unsigned)kSelMaxRanks ? (unsigned)kSelMaxRanks : st->nu);
    if (tid < kSelMaxRanks) { rk[tid] = st->rank[tid]; pf[tid] = st->prefix[tid]; sl[tid] = 0u; nrk[tid] = 0u; npf[tid] = 0u; }
    if (pass != 0 && tid < kSelMaxRanks) sl[tid] = st->slot[tid];
    if (tid == 0) sh_m = st->m;
    unsigned c[4], incl[4];
    if (pass == 0 && wid == 0) {
        // the ranks: position q / 100 * (m - 1) in fp64, its floor and the +1 neighbour clamped to m - 1, its fractional part
        const unsigned m = wave_scan_bins(ghist, lane, c, incl);
        if (lane < q.nq) {
            const double top = m > 0u ? (double)(m - 1u) : 0.0;
            const double pos = q.q[lane] / 100.0 * top;
            double lo = floor(pos);
            lo = lo < 0.0 ? 0.0 : (lo > top ? top : lo);
            const double hi = lo + 1.0 > top ? top : lo + 1.0;
            rk[2 * lane] = (unsigned)lo;
            rk[2 * lane + 1] = (unsigned)hi;
            st->t[lane] = pos - lo;
        }
        if (lane == 0) sh_m = m;
    }
    __syncthreads();
    for (int s = wid; s < nslots; s += kScanThreads / 64) {     // wave-uniform
        wave_scan_bins(ghist + s * kSelBins, lane, c, incl);
        for (int r = 0; r < R; ++r) {
            if ((int)sl[r] != s) continue;                       // uniform: sl is shared (all zero in the first pass)
            const unsigned want = rk[r];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned excl = incl[j] - c[j];
                if (excl <= want && want < incl[j]) { nrk[r] = want - excl; npf[r] = (pf[r] << 8) | (unsigned)(4 * lane + j); }
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        unsigned nu = 0u;
        for (int r = 0; r < R; ++r) {                            // the distinct prefixes, in LDS (rk is free now): no global read in the loop
            const unsigned p = npf[r];
            unsigned u = 0u;
            while (u < nu && rk[u] != p) ++u;
            if (u == nu) { rk[nu] = p; ++nu; }
            sl[r] = u;
        }
        sh_nu = nu;
    }
    __syncthreads();
    if (tid < kSelMaxRanks) { st->uprefix[tid] = rk[tid]; st->prefix[tid] = npf[tid]; st->rank[tid] = nrk[tid]; st->slot[tid] = sl[tid]; }
    if (tid == 0) {
        st->nu = sh_nu;
        st->m = sh_m;
        if (pass == 3) {
            for (int r = 0; r < R; ++r) order[r] = sel_unkey(npf[r]);
            for (int k = 0; k < q.nq; ++k) {
                const double lo = (double)sel_unkey(npf[2 * k]), hi = (double)sel_unkey(npf[2 * k + 1]);
                values[k] = lo + (hi - lo) * st->t[k];
            }
            counts[0] = (long long)sh_m;
            counts[1] = (long long)st->nonfinite;
        }
    }
}

// ------------------------------------------------------------------------------------------------ (c) the map, shared with (b)
constexpr int kMapMaxKnots = MI355SEG_INTENSITY_KNOTS_MAX;
struct MapParams { float kx[kMapMaxKnots], ky[kMapMaxKnots], slope[kMapMaxKnots]; float clip_lo, clip_hi; int nk; };

// NK > 0: the knot count is a compile-time constant and the search unrolls over kernel arguments; NK == 0: run-time nk
template <int NK>
__device__ __forceinline__ float map_eval(float x, const MapParams& P) {
    const float xc = fminf(fmaxf(x, P.clip_lo), P.clip_hi);
    float bx = P.kx[0], by = P.ky[0], s = P.slope[0];
    if (NK > 0) {
#pragma unroll
        for (int i = 1; i < NK - 1; ++i) {
            const bool in = P.kx[i] <= xc;                   // knots ascend: the last one that holds is segment j
            bx = in ? P.kx[i] : bx; by = in ? P.ky[i] : by; s = in ? P.slope[i] : s;
        }
    } else {
        for (int i = 1; i < P.nk - 1; ++i) {
            const bool in = P.kx[i] <= xc;
            bx = in ? P.kx[i] : bx; by = in ? P.ky[i] : by; s = in ? P.slope[i] : s;
        }
    }
    return __builtin_fmaf(xc - bx, s, by);
}

template <int NK>
__global__ __launch_bounds__(kIntThreads) void intensity_map_kernel(const float* x, MapParams P, long long n, float* y) {
    const long long n4 = n / 4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 v = ldf4(x + 4 * i);
        v.x = map_eval<NK>(v.x, P); v.y = map_eval<NK>(v.y, P); v.z = map_eval<NK>(v.z, P); v.w = map_eval<NK>(v.w, P);
        stf4(y + 4 * i, v);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) y[n4 * 4 + threadIdx.x] = map_eval<NK>(x[n4 * 4 + threadIdx.x], P);
}

// ------------------------------------------------------------------------------------------------ (b) moments
template <int NK>
__device__ __forceinline__ void mom_add(float x, const MapParams& P, int use_mask, float mask_gt, double pivot, double (&acc)[3]) {
    if (use_mask && !(x > mask_gt)) return;
    const double d = (double)map_eval<NK>(x, P) - pivot;     // exact: both are doubles
    acc[0] += 1.0; acc[1] += d; acc[2] += d * d;
}
template <int NK>
__global__ __launch_bounds__(kIntThreads) void intensity_moments_kernel(const float* __restrict__ x, MapParams P, long long n, int use_mask, float mask_gt,
                                                                         double pivot, double* __restrict__ part) {
    double acc[3] = {0.0, 0.0, 0.0};
    const long long n4 = n / 4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        mom_add<NK>(v.x, P, use_mask, mask_gt, pivot, acc); mom_add<NK>(v.y, P, use_mask, mask_gt, pivot, acc);
        mom_add<NK>(v.z, P, use_mask, mask_gt, pivot, acc); mom_add<NK>(v.w, P, use_mask, mask_gt, pivot, acc);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) mom_add<NK>(x[n4 * 4 + threadIdx.x], P, use_mask, mask_gt, pivot, acc);
    block_sum(acc);
    if (threadIdx.x == 0) { part[3 * blockIdx.x] = acc[0]; part[3 * blockIdx.x + 1] = acc[1]; part[3 * blockIdx.x + 2] = acc[2]; }
}
// out: count, mean, unbiased variance (NaN below two voxels), sum of (map(x) - pivot)
__global__ __launch_bounds__(kIntThreads) void intensity_moments_finalize_kernel(const double* __restrict__ part, int nblk, double pivot, double* __restrict__ out) {
    double acc[3] = {0.0, 0.0, 0.0};
    partials_reduce<OpSum>(part, nblk, acc);
    block_sum(acc);
    if (threadIdx.x == 0) {
        const double c = acc[0], md = c > 0.0 ? acc[1] / c : 0.0;
        out[0] = c;
        out[1] = pivot + md;
        out[2] = c > 1.0 ? (acc[2] - acc[1] * md) / (c - 1.0) : __builtin_nan("");
        out[3] = acc[1];
    }
}

static bool map_params(const float* kx, const float* ky, const float* slope, int nk, float clip_lo, float clip_hi, MapParams& P) {
    if (!kx || !ky || !slope || nk < 2 || nk > kMapMaxKnots || !(clip_lo <= clip_hi)) return false;
    for (int i = 0; i < kMapMaxKnots; ++i) {
        const int j = i < nk ? i : nk - 1;
        P.kx[i] = kx[j]; P.ky[i] = ky[j]; P.slope[i] = slope[j < nk - 1 ? j : nk - 2];
        if (!(P.kx[i] == P.kx[i]) || !(P.ky[i] == P.ky[i]) || !(P.slope[i] == P.slope[i])) return false;
        if (i > 0 && i < nk && kx[i] < kx[i - 1]) return false;
    }
    P.clip_lo = clip_lo; P.clip_hi = clip_hi; P.nk = nk;
    return true;
}

}  // namespace seg

using namespace seg;

extern "C" {

size_t mi355seg_percentiles_ws_bytes(long long n) {
    (void)n;
    return align_up(sizeof(SelState), 256) + (size_t)(kSelBins + 3 * kSelMaxRanks * kSelBins) * sizeof(unsigned);
}
int mi355seg_percentiles_f32(const float* x, long long n, const double* q, int nq, int use_mask, float mask_gt,
                             double* values, float* order, long long* counts, void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(x && q && values && order && counts && n > 0, "percentiles: bad arguments (n > 0)");
    SEG_CHECK_ARG(n < (1ll << 31), "percentiles: n = %lld is not below 2^31", n);
    SEG_CHECK_ARG(nq >= 1 && nq <= kSelMaxQ, "percentiles: %d percentiles asked for, 1 .. %d per call", nq, kSelMaxQ);
    SEG_CHECK_ARG(((uintptr_t)x % 16) == 0, "percentiles: the volume must be 16-byte aligned");
    SEG_CHECK_ARG(!use_mask || mask_gt == mask_gt, "percentiles: mask_gt is NaN");
    SelQ sq;
    sq.nq = nq;
    for (int i = 0; i < kSelMaxQ; ++i) {
        sq.q[i] = i < nq ? q[i] : 0.0;
        SEG_CHECK_ARG(sq.q[i] >= 0.0 && sq.q[i] <= 100.0, "percentiles: percentile %d = %g is outside 0 .. 100", i, sq.q[i]);
    }
    SEG_CHECK_WS(mi355seg_percentiles_ws_bytes(n), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, 16.0 * n, st);
    SelState* state = (SelState*)ws;
    unsigned* hist = (unsigned*)((char*)ws + align_up(sizeof(SelState), 256));
    if (hipMemsetAsync(ws, 0, mi355seg_percentiles_ws_bytes(n), st) != hipSuccess) {
        set_error("percentiles: hipMemsetAsync failed");
        return MI355SEG_EHIP;
    }
    const int nblk = int_grid((n / 4 + 1 + kSelUnroll - 1) / kSelUnroll, kSelMaxBlocks);
    hipLaunchKernelGGL(sel_hist_kernel<true>, dim3(nblk), dim3(kIntThreads), 0, st, x, n, use_mask, mask_gt, 24, state, hist);
    SEG_CHECK_LAUNCH();
    hipLaunchKernelGGL(sel_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, 0, sq, state, (const unsigned*)hist, values, order, counts);
    SEG_CHECK_LAUNCH();
    for (int pass = 1; pass < 4; ++pass) {
        unsigned* h = hist + kSelBins + (size_t)(pass - 1) * kSelMaxRanks * kSelBins;
        hipLaunchKernelGGL(sel_hist_kernel<false>, dim3(nblk), dim3(kIntThreads), 0, st, x, n, use_mask, mask_gt, 24 - 8 * pass, state, h);
        SEG_CHECK_LAUNCH();
        hipLaunchKernelGGL(sel_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, pass, sq, state, (const unsigned*)h, values, order, counts);
        SEG_CHECK_LAUNCH();
    }
    return MI355SEG_OK;
}

size_t mi355seg_intensity_moments_ws_bytes(long long n) { (void)n; return (size_t)kMomMaxBlocks * 3 * sizeof(double); }
int mi355seg_intensity_moments_f32(const float* x, long long n, const float* kx, const float* ky, const float* slope, int nk,
                                   float clip_lo, float clip_hi, int use_mask, float mask_gt, double pivot, double* out,
                                   void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(x && out && n > 0, "intensity_moments: bad arguments (n > 0)");
    SEG_CHECK_ARG(((uintptr_t)x % 16) == 0, "intensity_moments: the volume must be 16-byte aligned");
    SEG_CHECK_ARG(pivot == pivot && (!use_mask || mask_gt == mask_gt), "intensity_moments: pivot or mask_gt is NaN");
    MapParams P;
    SEG_CHECK_ARG(map_params(kx, ky, slope, nk, clip_lo, clip_hi, P),
                  "intensity_moments: bad map (2 .. %d ascending knots, no NaN, clip_lo <= clip_hi)", kMapMaxKnots);
    SEG_CHECK_WS(mi355seg_intensity_moments_ws_bytes(n), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, 4.0 * n, st);
    double* part = (double*)ws;
    const int nblk = int_grid(n / 4 + 1, kMomMaxBlocks);
    if (nk == 2) hipLaunchKernelGGL(intensity_moments_kernel<2>, dim3(nblk), dim3(kIntThreads), 0, st, x, P, n, use_mask, mask_gt, pivot, part);
    else if (nk == 11) hipLaunchKernelGGL(intensity_moments_kernel<11>, dim3(nblk), dim3(kIntThreads), 0, st, x, P, n, use_mask, mask_gt, pivot, part);
    else hipLaunchKernelGGL(intensity_moments_kernel<0>, dim3(nblk), dim3(kIntThreads), 0, st, x, P, n, use_mask, mask_gt, pivot, part);
    SEG_CHECK_LAUNCH();
    hipLaunchKernelGGL(intensity_moments_finalize_kernel, dim3(1), dim3(kIntThreads), 0, st, (const double*)part, nblk, pivot, out);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int mi355seg_intensity_map_f32(const float* x, long long n, const float* kx, const float* ky, const float* slope, int nk,
                               float clip_lo, float clip_hi, float* y, void* stream) {
    SEG_CHECK_ARG(x && y && n > 0, "intensity_map: bad arguments (n > 0)");
    SEG_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0, "intensity_map: pointers must be 16-byte aligned");
    MapParams P;
    SEG_CHECK_ARG(map_params(kx, ky, slope, nk, clip_lo, clip_hi, P),
                  "intensity_map: bad map (2 .. %d ascending knots, no NaN, clip_lo <= clip_hi)", kMapMaxKnots);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, 8.0 * n, st);
    const int nblk = int_grid(n / 4 + 1, 2048) * 2;
    if (nk == 2) hipLaunchKernelGGL(intensity_map_kernel<2>, dim3(nblk), dim3(kIntThreads), 0, st, x, P, n, y);
    else if (nk == 11) hipLaunchKernelGGL(intensity_map_kernel<11>, dim3(nblk), dim3(kIntThreads), 0, st, x, P, n, y);
    else hipLaunchKernelGGL(intensity_map_kernel<0>, dim3(nblk), dim3(kIntThreads), 0, st, x, P, n, y);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

}  // extern "C"
