// sampler.hip -- label-balanced patch sampling of the device patch queue (tio.LabelSampler; the reference imports it beside
// UniformSampler, dataloader.py:19; config.sampler=label).  UNPINNED: torchio is absent and the reference holds no fixture of its data
// pipeline, so the definitions in include/mi355seg.h ("Label-balanced patch sampling") are the specification.
//
// The host cost of a label sampler is a cumulative sum over every voxel of the label map per subject visit.  Here that becomes
//   build  (once per subject and patch size, 2 launches): the region R of valid patch centres is cut into chunks of kSmpChunk consecutive
//          region-linear voxels; one workgroup per chunk counts its voxels per class (16 classes + the `bad` bin) with wave ballots,
//          then one workgroup per class turns that class's per-chunk counts into exclusive int64 prefixes, in place, and writes the total;
//   select (1 launch per visit, one workgroup per pick): binary search of the rank in the class's chunk prefixes, re-read of that one
//          chunk, ballot prefix count to the voxel with the remaining rank, whose region coordinates are the patch origin.
// Integer arithmetic only, no atomics, every sum in a fixed order: equal inputs give bitwise equal outputs, and the result is exact.
//
// Order inside a chunk (shared by both kernels, and it IS the region-linear order): pass j = 0 .. kSmpPasses-1, wave w = 0 .. 3, lane:
//   e = chunk * kSmpChunk + j * kSmpThreads + w * 64 + lane.
// Index layout: int64 [17][nchunks], class-major, so a class's prefixes are contiguous for the scan and the binary search.
#include "common.h"

namespace seg {

constexpr int kSmpThreads = 256;
constexpr int kSmpWaves = kSmpThreads / kWave;
constexpr int kSmpPasses = 4;
constexpr int kSmpChunk = MI355SEG_LABEL_CHUNK;          // region-linear voxels per chunk
constexpr int kSmpBins = MI355SEG_LABEL_BINS;            // 16 classes + bad
constexpr int kSmpScanBatch = 8;                         // independent loads in flight per thread of the prefix scan
static_assert(kSmpChunk == kSmpThreads * kSmpPasses, "a chunk is kSmpPasses passes of one workgroup");
static_assert(kSmpBins == 17 && kSmpBins <= kWave, "one lane per bin in the reduce");

// the region of valid patch centres inside the label volume: extents m, start s (= patch // 2), n = m0 * m1 * m2 voxels
struct SmpGeom { int H, W, m1, m2, s0, s1, s2; long long n; int nchunks; };

// class of a label value: the integer itself in [0, 16), else the `bad` bin (non-integers, negatives, >= 16, NaN, infinities)
__device__ __forceinline__ int smp_class(float v) {
    return (v >= 0.f && v < 16.f && v == floorf(v)) ? (int)v : 16;
}

// region-linear index e < g.n < 2^31 -> region coordinates (z, y, x): 32-bit divisions
__device__ __forceinline__ void smp_coords(const SmpGeom& g, unsigned e, int& z, int& y, int& x) {
    const unsigned t = e / (unsigned)g.m2;
    x = (int)(e - t * (unsigned)g.m2);
    z = (int)(t / (unsigned)g.m1);
    y = (int)(t - (unsigned)z * (unsigned)g.m1);
}

// the label at region-linear index e (e < g.n, so the address lies inside the volume, whose voxel count is below 2^31 too)
__device__ __forceinline__ float smp_load(const float* __restrict__ labels, const SmpGeom& g, unsigned e) {
    int z, y, x;
    smp_coords(g, e, z, y, x);
    return labels[((z + g.s0) * g.H + (y + g.s1)) * g.W + (x + g.s2)];
}

// classes of this thread's kSmpPasses voxels of chunk `chunk` (-1 past the end of the region)
__device__ __forceinline__ void smp_chunk_classes(const float* __restrict__ labels, const SmpGeom& g, int chunk, int (&cls)[kSmpPasses]) {
    const long long base = (long long)chunk * kSmpChunk + threadIdx.x;
#pragma unroll
    for (int j = 0; j < kSmpPasses; ++j) {
        const long long e = base + j * kSmpThreads;
        cls[j] = e < g.n ? smp_class(smp_load(labels, g, (unsigned)e)) : -1;
    }
}

__global__ __launch_bounds__(kSmpThreads) void smp_count_kernel(const float* __restrict__ labels, SmpGeom g, long long* __restrict__ index) {
    __shared__ int sh[kSmpWaves][kSmpBins];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int cls[kSmpPasses];
    smp_chunk_classes(labels, g, (int)blockIdx.x, cls);
    int mine = 0;                                           // lane b < 17 ends up with its wave's count of bin b
#pragma unroll
    for (int b = 0; b < kSmpBins; ++b) {
        int c = 0;
#pragma unroll
        for (int j = 0; j < kSmpPasses; ++j) c += __popcll(__ballot(cls[j] == b));
        if (lane == b) mine = c;
    }
    if (lane < kSmpBins) sh[wid][lane] = mine;
    __syncthreads();
    if (threadIdx.x < kSmpBins) {
        const int b = threadIdx.x;
        index[(long long)b * g.nchunks + blockIdx.x] = (long long)(((sh[0][b] + sh[1][b]) + sh[2][b]) + sh[3][b]);
    }
}

// one workgroup per bin: counts -> exclusive prefixes in place (thread t owns the contiguous segment [t * seg, (t + 1) * seg)), total out
__global__ __launch_bounds__(kSmpThreads) void smp_scan_kernel(long long* __restrict__ index, int nchunks, long long* __restrict__ counts) {
    __shared__ long long shw[kSmpWaves];
    long long* __restrict__ row = index + (long long)blockIdx.x * nchunks;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int seg = (nchunks + kSmpThreads - 1) / kSmpThreads;
    const long long lo = (long long)threadIdx.x * seg;
    const long long hi = lo + seg < nchunks ? lo + seg : nchunks;
    // a thread's walk over its segment is serial; kSmpScanBatch independent loads per step keep it from paying one memory latency per chunk
    long long s = 0;
    for (long long i = lo; i < hi; i += kSmpScanBatch) {
        long long v[kSmpScanBatch];
#pragma unroll
        for (int k = 0; k < kSmpScanBatch; ++k) v[k] = i + k < hi ? row[i + k] : 0;
#pragma unroll
        for (int k = 0; k < kSmpScanBatch; ++k) s += v[k];
    }
    long long inc = s;                                      // inclusive scan over the wave, then over the four wave totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) shw[wid] = inc;
    __syncthreads();
    long long before = 0;
#pragma unroll
    for (int w = 0; w < kSmpWaves; ++w)
        if (w < wid) before += shw[w];
    long long run = before + inc - s;                       // exclusive prefix of this thread's segment
    for (long long i = lo; i < hi; i += kSmpScanBatch) {
        long long v[kSmpScanBatch];
#pragma unroll
        for (int k = 0; k < kSmpScanBatch; ++k) v[k] = i + k < hi ? row[i + k] : 0;
#pragma unroll
        for (int k = 0; k < kSmpScanBatch; ++k) {
            if (i + k < hi) row[i + k] = run;
            run += v[k];
        }
    }
    if (threadIdx.x == kSmpThreads - 1) counts[blockIdx.x] = run;
}

__global__ __launch_bounds__(kSmpThreads) void smp_select_kernel(const float* __restrict__ labels, SmpGeom g, const long long* __restrict__ index,
                                                                 const long long* __restrict__ picks, int* __restrict__ origins) {
    __shared__ int sh[kSmpPasses][kSmpWaves];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long long cl = picks[2 * (long long)blockIdx.x], rank = picks[2 * (long long)blockIdx.x + 1];
    if (cl < 0 || cl >= kSmpBins) return;                   // workgroup-uniform; the caller guarantees class < 16 (see mi355seg.h)
    const long long* __restrict__ row = index + cl * g.nchunks;
    int lo = 0, hi = g.nchunks - 1;                         // the last chunk whose exclusive prefix is <= rank holds the voxel
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (row[mid] <= rank) lo = mid; else hi = mid - 1;
    }
    const long long rem0 = rank - row[lo];
    int cls[kSmpPasses];
    smp_chunk_classes(labels, g, lo, cls);
    unsigned long long mask[kSmpPasses];
#pragma unroll
    for (int j = 0; j < kSmpPasses; ++j) {
        mask[j] = __ballot(cls[j] == (int)cl);
        if (lane == 0) sh[j][wid] = __popcll(mask[j]);
    }
    __syncthreads();
    long long rem = rem0;                                   // walk the 16 (pass, wave) segments in region-linear order
    bool done = rem < 0;
#pragma unroll
    for (int j = 0; j < kSmpPasses; ++j)
#pragma unroll
        for (int w = 0; w < kSmpWaves; ++w) {
            const int c = sh[j][w];
            if (!done && rem < c) {
                done = true;
                const unsigned long long below = mask[j] & ((1ull << lane) - 1ull);
                if (w == wid && ((mask[j] >> lane) & 1ull) && __popcll(below) == (int)rem) {
                    int* __restrict__ o = origins + 3 * (long long)blockIdx.x;      // a matching lane has e < g.n
                    smp_coords(g, (unsigned)lo * kSmpChunk + j * kSmpThreads + threadIdx.x, o[0], o[1], o[2]);
                }
            }
            if (!done) rem -= c;
        }
}

// shared argument checks; fills g.  Returns 0 or an error code with the message set.
static int smp_geom(const char* what, const float* labels, int D, int H, int W, int pd, int ph, int pw, SmpGeom& g) {
    SEG_CHECK_ARG(labels, "%s: labels is null", what);
    SEG_CHECK_ARG(D > 0 && H > 0 && W > 0 && pd > 0 && ph > 0 && pw > 0, "%s: bad arguments (volume %dx%dx%d, patch %dx%dx%d)", what, D, H, W, pd, ph, pw);
    SEG_CHECK_ARG((long long)D * H * W < (1ll << 31), "%s: a label volume of %dx%dx%d voxels exceeds 2^31 - 1", what, D, H, W);
    SEG_CHECK_ARG(pd <= D && ph <= H && pw <= W, "%s: the patch %dx%dx%d is larger than the volume %dx%dx%d", what, pd, ph, pw, D, H, W);
    const int m0 = D - pd + 1, m1 = H - ph + 1, m2 = W - pw + 1;
    g.H = H; g.W = W; g.m1 = m1; g.m2 = m2;
    g.s0 = pd / 2; g.s1 = ph / 2; g.s2 = pw / 2;
    g.n = (long long)m0 * m1 * m2;
    g.nchunks = (int)((g.n + kSmpChunk - 1) / kSmpChunk);
    return MI355SEG_OK;
}

}  // namespace seg

using namespace seg;

extern "C" {

size_t mi355seg_label_index_bytes(int D, int H, int W, int pd, int ph, int pw) {
    if (D <= 0 || H <= 0 || W <= 0 || pd <= 0 || ph <= 0 || pw <= 0 || pd > D || ph > H || pw > W) return 0;
    const long long n = (long long)(D - pd + 1) * (H - ph + 1) * (W - pw + 1);
    return (size_t)((n + kSmpChunk - 1) / kSmpChunk) * kSmpBins * sizeof(long long);
}

int mi355seg_label_index_build_f32(const float* labels, int D, int H, int W, int pd, int ph, int pw, void* index, size_t index_bytes,
                                   long long* counts17, void* stream) {
    SmpGeom g;
    if (const int rc = smp_geom("label_index_build", labels, D, H, W, pd, ph, pw, g)) return rc;
    SEG_CHECK_ARG(index && counts17, "label_index_build: index or counts17 is null");
    SEG_CHECK_ARG((uintptr_t)index % 8 == 0 && (uintptr_t)counts17 % 8 == 0, "label_index_build: index and counts17 must be 8-byte aligned");
    const size_t need = mi355seg_label_index_bytes(D, H, W, pd, ph, pw);
    SEG_CHECK_ARG(index_bytes >= need, "label_index_build: index_bytes too small: need %zu bytes, have %zu", need, index_bytes);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, 4.0 * g.n + 3.0 * need, st);
    hipLaunchKernelGGL(smp_count_kernel, dim3(g.nchunks), dim3(kSmpThreads), 0, st, labels, g, (long long*)index);
    SEG_CHECK_LAUNCH();
    hipLaunchKernelGGL(smp_scan_kernel, dim3(kSmpBins), dim3(kSmpThreads), 0, st, (long long*)index, g.nchunks, counts17);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int mi355seg_label_index_select(const float* labels, int D, int H, int W, int pd, int ph, int pw, const void* index,
                                const long long* picks, int n, int* origins, void* stream) {
    SmpGeom g;
    if (const int rc = smp_geom("label_index_select", labels, D, H, W, pd, ph, pw, g)) return rc;
    SEG_CHECK_ARG(index && picks && origins, "label_index_select: index, picks or origins is null");
    SEG_CHECK_ARG((uintptr_t)index % 8 == 0 && (uintptr_t)picks % 8 == 0, "label_index_select: index and picks must be 8-byte aligned");
    SEG_CHECK_ARG(n > 0, "label_index_select: n = %d picks (expected >= 1)", n);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, (double)n * (4.0 * kSmpChunk + 28.0), st);
    hipLaunchKernelGGL(smp_select_kernel, dim3(n), dim3(kSmpThreads), 0, st, labels, g, (const long long*)index, picks, origins);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

}  // extern "C"
