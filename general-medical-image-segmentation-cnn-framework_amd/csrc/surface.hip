// surface.hip -- the predict-time metrics beside Dice on the device: mask edges + bounding box, the exact anisotropic
// Euclidean distance transform (three separable passes, fp64), the surface-distance gather and the confusion counters
// (utils/metric.py:29-32,45-59 with spacing; monai's compute_hausdorff_distance restated, see utils/metric.py of the package).
//
// EDT form: the plain min-plus step g(i) = min_j f(j) + (s*i - s*j)^2 with every j, no lower envelope.  Lines are a few hundred
// voxels and every (i, j) pair costs one fp64 subtract, one fma and one min: at 256^3 the two strided passes are bound by the fp64
// rate, not by HBM (1.2 ms each), and the whole metric stays an order of magnitude below the forward it grades.
#include "common.h"
#include "edt.h"
#include "internal.h"

namespace seg {

constexpr int kSurfThreads = 256;
static_assert(kSurfThreads == kReduceThreads, "the block size of reduce.h");

static int surf_grid(long long items) { return stream_grid(items, kSurfThreads, 4096); }

// info[8] = n_edge(gt), n_edge(pred), box lo z, y, x, box hi z, y, x (hi exclusive) of edge(gt) | edge(pred); an empty union leaves
// lo = extent and hi = 0
__global__ void edge_info_init_kernel(long long* __restrict__ info, int D, int H, int W) {
    if (threadIdx.x == 0) {
        info[0] = 0; info[1] = 0;
        info[2] = D; info[3] = H; info[4] = W;
        info[5] = 0; info[6] = 0; info[7] = 0;
    }
}

// the operation per entry of info: counts add, the box's low corner takes the minimum, its high corner the maximum
struct OpEdgeInfo {
    static __device__ __forceinline__ long long apply(long long a, long long b, int j) { return j < 2 ? a + b : j < 5 ? (b < a ? b : a) : (b > a ? b : a); }
};

// edge(m) = m & ~erode6(m): a foreground voxel with a background face neighbour, outside the array = background
// (scipy.ndimage.binary_erosion(m) ^ m, default cross, border_value = 0).  One pass: both edge maps, their counts, the joint box.
__global__ __launch_bounds__(kSurfThreads) void mask_edges_kernel(const int64_t* __restrict__ gt, const int64_t* __restrict__ pr,
        int D, int H, int W, uint8_t* __restrict__ edges, long long* __restrict__ info) {
    const long long HW = (long long)H * W, total = (long long)D * HW;
    long long cnt[2] = {0, 0};
    int lo[3] = {D, H, W}, hi[3] = {0, 0, 0};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int z = (int)(i / HW);
        const unsigned rem = (unsigned)(i - z * HW);        // H * W < 2^31 (checked by the entry point)
        const int y = (int)(rem / (unsigned)W), x = (int)(rem - (unsigned)y * (unsigned)W);
        bool any = false;
        for (int m = 0; m < 2; ++m) {
            const int64_t* __restrict__ v = m ? pr : gt;
            bool e = false;
            if (v[i] != 0) {
                e = x == 0 || x == W - 1 || y == 0 || y == H - 1 || z == 0 || z == D - 1;
                if (!e) e = v[i - 1] == 0 || v[i + 1] == 0 || v[i - W] == 0 || v[i + W] == 0 || v[i - HW] == 0 || v[i + HW] == 0;
            }
            edges[m * total + i] = e;
            cnt[m] += e;
            any |= e;
        }
        if (any) {
            lo[0] = min(lo[0], z); lo[1] = min(lo[1], y); lo[2] = min(lo[2], x);
            hi[0] = max(hi[0], z + 1); hi[1] = max(hi[1], y + 1); hi[2] = max(hi[2], x + 1);
        }
    }
    // integer reductions: any order gives the same result.  The eight values of info in one pass, then one set of atomics per block
    for (int m = 0; m < 2; ++m) cnt[m] = wave_sum(cnt[m]);
    for (int a = 0; a < 3; ++a) { lo[a] = wave_reduce<OpMin>(lo[a]); hi[a] = wave_reduce<OpMax>(hi[a]); }      // (as ints)
    long long v[8] = {cnt[0], cnt[1], lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
    block_combine<OpEdgeInfo>(v);
    // lane j of the first wave commits entry j: the eight entries share a cache line, and eight lanes of one instruction are one
    // request to it where eight instructions of thread 0 are eight (every block's atomics queue on that line)
    if (threadIdx.x < kWave) {
        long long mine = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            // thread 0's value through the scalar unit (the whole first wave is here, so its first lane is thread 0)
            const unsigned long long t0 = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(v[j] >> 32)) << 32) |
                                          (unsigned)__builtin_amdgcn_readfirstlane((int)v[j]);
            if ((int)threadIdx.x == j) mine = (long long)t0;
        }
        const int j = threadIdx.x;
        if (j < 2) { if (mine) atomicAdd((unsigned long long*)&info[j], (unsigned long long)mine); }
        else if (j < 5) atomicMin(&info[j], mine);       // a block without edge voxels holds lo = extent, hi = 0: no effect
        else if (j < 8) atomicMax(&info[j], mine);
    }
}

// EDT pass 1, along W (contiguous): |x - nearest site in the line| as int32, -1 where the line holds no site.  One wave per line:
// the line's site bits go to LDS as 64-bit ballots, each lane then finds the nearest set bit on either side (edt.h).
// Box-relative output [2][bd][bh][bw]; the input is the full-volume edge map.
__global__ __launch_bounds__(kSurfThreads) void edt_pass_w_kernel(const uint8_t* __restrict__ sites, long long mask_stride, int H, int W,
        int z0, int y0, int x0, int bd, int bh, int bw, int* __restrict__ out) {
    extern __shared__ unsigned long long edt_bits[];
    constexpr int kLines = kSurfThreads / kWave;
    const int nw = (bw + kWave - 1) / kWave, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    unsigned long long* bits = edt_bits + wave * nw;
    const long long slab = (long long)bd * bh, lines = 2 * slab, box = slab * bw;
    for (long long lb = (long long)blockIdx.x * kLines; lb < lines; lb += (long long)gridDim.x * kLines) {     // block-uniform trip count
        const long long l = lb + wave;
        const bool live = l < lines;
        const int m = live ? (int)(l / slab) : 0;
        const long long r = live ? l - m * slab : 0;
        const int z = (int)(r / bh), y = (int)(r - (long long)z * bh);
        const uint8_t* __restrict__ src = sites + m * mask_stride + ((long long)(z + z0) * H + (y + y0)) * W + x0;
        for (int k = 0; k < nw; ++k) {
            const int x = k * kWave + lane;
            const unsigned long long b = __ballot(live && x < bw && src[x] != 0);
            if (lane == 0) bits[k] = b;
        }
        __syncthreads();
        int* __restrict__ dst = out + m * box + r * bw;
        for (int k = 0; k < nw; ++k) {
            const int x = k * kWave + lane;
            if (live && x < bw) dst[x] = nearest_set_bit(bits, nw, k, lane);
        }
        __syncthreads();
    }
}

constexpr int kEdtTW = 32;      // columns of W per block: 256 contiguous bytes of fp64 per row of the tile
constexpr int kEdtTY = kSurfThreads / kEdtTW;
constexpr int kEdtTJ = 64;      // rows of the source line staged in LDS per step (16 KiB); a line of any length walks through it

__device__ __forceinline__ double edt_load(const int* p, double s) {
    const int v = *p;
    const double d = s * (double)v;
    return v < 0 ? HUGE_VAL : d * d;
}
__device__ __forceinline__ double edt_load(const double* p, double) { return *p; }

// EDT passes 2 and 3: g(i) = min_j f(j) + (s*i - s*j)^2 along an axis of `n` elements with element stride `stride`; `inner`
// contiguous columns (any count) share the axis, `outer` slabs of `outer_stride` elements repeat it.
// A block owns kEdtTW columns and RI * kEdtTY output rows, each thread RI rows of one column in registers; the source line passes
// through LDS kEdtTJ rows at a time, so global loads and stores run along W.  InT = int takes pass 1's offsets and squares them
// with `s_in` on the way in.
template <typename InT, int RI>
__global__ __launch_bounds__(kSurfThreads) void edt_pass_axis_kernel(const InT* __restrict__ in, double* __restrict__ out, int n, long long stride,
        int inner, long long outer_stride, double s, double s_in) {
    const int tx = threadIdx.x % kEdtTW, ty = threadIdx.x / kEdtTW;
    const int col = blockIdx.x * kEdtTW + tx;
    const int i0 = blockIdx.y * (RI * kEdtTY) + ty * RI;
    const long long base = (long long)blockIdx.z * outer_stride;
    const bool live = col < inner;
    double acc[1][RI];
    const bool none[RI] = {};           // one plane: no row selects
    const auto load = [=](int, int j) { return live ? edt_load(in + base + (long long)j * stride + col, s_in) : HUGE_VAL; };
    minplus_axis<double, 1, false, kEdtTW, kEdtTY, kEdtTJ, RI>(acc, none, load, n, s, i0, tx, ty);
    if (live) {
#pragma unroll
        for (int r = 0; r < RI; ++r)
            if (i0 + r < n) out[base + (long long)(i0 + r) * stride + col] = acc[0][r];
    }
}

// sqrt(dt2) of the OTHER mask's sites at this mask's edge voxels, compacted: dist[0][..n_gt) = distance to edge(pred) at edge(gt),
// dist[1][..n_pred) = distance to edge(gt) at edge(pred).  A block owns kGatherPer * 256 consecutive voxels of the box, counts its
// edge voxels, takes its slots with ONE atomic per mask and ranks its threads with a scan; blocks finish in any order, so the order
// inside a row is not fixed; the percentile sorts it.
constexpr int kGatherPer = 16;
__global__ __launch_bounds__(kSurfThreads) void surface_gather_kernel(const uint8_t* __restrict__ edges, long long mask_stride, int H, int W,
        int z0, int y0, int x0, int bd, int bh, int bw, const double* __restrict__ dt2, double* __restrict__ dist, long long row_stride,
        long long cap0, long long cap1, unsigned long long* __restrict__ cursor) {
    __shared__ unsigned wave_cnt[2][kSurfThreads / kWave];
    __shared__ unsigned long long block_base[2];
    const long long box = (long long)bd * bh * bw, chunk0 = (long long)blockIdx.x * (kGatherPer * kSurfThreads);
    const unsigned hw = (unsigned)bh * (unsigned)bw;        // < 2^31 (box_ok)
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    unsigned flags[2] = {0u, 0u};
    for (int k = 0; k < kGatherPer; ++k) {
        const long long i = chunk0 + k * kSurfThreads + threadIdx.x;
        if (i >= box) break;
        const int z = (int)(i / hw);
        const unsigned rem = (unsigned)(i - (long long)z * hw);
        const int y = (int)(rem / (unsigned)bw), x = (int)(rem - (unsigned)y * (unsigned)bw);
        const long long full = ((long long)(z + z0) * H + (y + y0)) * W + (x + x0);
        for (int m = 0; m < 2; ++m) flags[m] |= (edges[m * mask_stride + full] != 0 ? 1u : 0u) << k;
    }
    unsigned rank[2];
    for (int m = 0; m < 2; ++m) {
        unsigned v = __popc(flags[m]);                      // inclusive scan across the wave
        for (int o = 1; o < kWave; o <<= 1) {
            const unsigned u = __shfl_up(v, o, kWave);
            if (lane >= o) v += u;
        }
        rank[m] = v - __popc(flags[m]);
        if (lane == kWave - 1) wave_cnt[m][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned total = 0;
        for (int w = 0; w < kSurfThreads / kWave; ++w) total += wave_cnt[threadIdx.x][w];
        block_base[threadIdx.x] = total ? atomicAdd(&cursor[threadIdx.x], (unsigned long long)total) : 0ull;
    }
    __syncthreads();
    for (int m = 0; m < 2; ++m) {
        long long slot = (long long)block_base[m] + rank[m];
        for (int w = 0; w < wave; ++w) slot += wave_cnt[m][w];
        const long long cap = m ? cap1 : cap0;
        for (int k = 0; k < kGatherPer; ++k)
            if ((flags[m] >> k) & 1u) {
                const long long i = chunk0 + k * kSurfThreads + threadIdx.x;
                if (slot < cap) dist[m * row_stride + slot] = sqrt(dt2[(1 - m) * box + i]);
                ++slot;
            }
    }
}

// utils/metric.py:34-43,45-55: the four Dice counters and tp, fp, fn, tn (value sums of the arrays the reference builds)
__global__ __launch_bounds__(kSurfThreads) void confusion_counts_kernel(const int64_t* __restrict__ gt, const int64_t* __restrict__ pr,
        long long numel, long long* __restrict__ part) {
    long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (long long)gridDim.x * blockDim.x) {
        const long long g = gt[i], p = pr[i];
        acc[0] += g; acc[1] += p;
        acc[2] += ((g & p) != 0); acc[3] += ((g | p) != 0);
        acc[4] += g & p;
        acc[5] += (p - g < 1) ? 0 : p;
        acc[6] += (g - p < 1) ? 0 : g;
        acc[7] += 1 - (g | p);
    }
    block_sum(acc);
    if (threadIdx.x == 0) for (int j = 0; j < 8; ++j) part[(long long)blockIdx.x * 8 + j] = acc[j];
}

template <typename InT>
static void launch_axis(const InT* in, double* out, int n, long long stride, int inner, int outer, long long outer_stride,
                        double s, double s_in, hipStream_t st) {
    if (n <= 8 * kEdtTY) {
        dim3 g(cdiv(inner, kEdtTW), cdiv(n, 8 * kEdtTY), outer);
        hipLaunchKernelGGL((edt_pass_axis_kernel<InT, 8>), g, dim3(kSurfThreads), 0, st, in, out, n, stride, inner, outer_stride, s, s_in);
    } else {
        dim3 g(cdiv(inner, kEdtTW), cdiv(n, 32 * kEdtTY), outer);
        hipLaunchKernelGGL((edt_pass_axis_kernel<InT, 32>), g, dim3(kSurfThreads), 0, st, in, out, n, stride, inner, outer_stride, s, s_in);
    }
}

static bool box_ok(int D, int H, int W, int z0, int y0, int x0, int bd, int bh, int bw) {
    return D > 0 && H > 0 && W > 0 && bd > 0 && bh > 0 && bw > 0 && z0 >= 0 && y0 >= 0 && x0 >= 0 &&
           (long long)z0 + bd <= D && (long long)y0 + bh <= H && (long long)x0 + bw <= W && 2ll * bd <= 65535 &&
           (long long)bh * bw < (1ll << 31) - kEdtTW;
}

}  // namespace seg

using namespace seg;

extern "C" {

int mi355seg_mask_edges_i64(const int64_t* gt, const int64_t* pred, int D, int H, int W, uint8_t* edges, int64_t* info, void* stream) {
    SEG_CHECK_ARG(gt && pred && edges && info && D > 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 31), "mask_edges: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)D * H * W;
    ProfScope ps(PF_LOSS, 0.0, 18.0 * total, st);
    hipLaunchKernelGGL(edge_info_init_kernel, dim3(1), dim3(kWave), 0, st, (long long*)info, D, H, W);
    SEG_CHECK_LAUNCH();
    hipLaunchKernelGGL(mask_edges_kernel, dim3(surf_grid(total)), dim3(kSurfThreads), 0, st, gt, pred, D, H, W, edges, (long long*)info);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

size_t mi355seg_edt3d_ws_bytes(int bd, int bh, int bw) {
    const size_t box = (size_t)bd * bh * bw;
    return align_up(2 * box * sizeof(int), 256) + align_up(2 * box * sizeof(double), 256);
}

int mi355seg_edt3d_f64(const uint8_t* sites, int D, int H, int W, int z0, int y0, int x0, int bd, int bh, int bw,
                       double sz, double sy, double sx, double* dt2, void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(sites && dt2 && box_ok(D, H, W, z0, y0, x0, bd, bh, bw), "edt3d: bad arguments (the box lies inside the volume and has at most 32767 slices)");
    SEG_CHECK_ARG(sz > 0 && sy > 0 && sx > 0, "edt3d: spacing must be positive");
    SEG_CHECK_WS(mi355seg_edt3d_ws_bytes(bd, bh, bw), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    const long long box = (long long)bd * bh * bw;
    ProfScope ps(PF_LOSS, 6.0 * box * (bh + bd), 2.0 * box * (1 + 4 + 4 + 8 + 8 + 8), st);
    Carver cv(ws);
    int* off = cv.take<int>(2 * box);
    double* tmp = cv.take<double>(2 * box);
    const int nw = cdiv(bw, kWave);
    const size_t lds = (size_t)(kSurfThreads / kWave) * nw * sizeof(unsigned long long);
    SEG_CHECK_ARG(lds <= 48 * 1024, "edt3d: box wider than 98304 voxels");
    hipLaunchKernelGGL(edt_pass_w_kernel, dim3(surf_grid(2ll * bd * bh * kWave)), dim3(kSurfThreads), lds, st, sites, (long long)D * H * W, H, W,
                       z0, y0, x0, bd, bh, bw, off);
    SEG_CHECK_LAUNCH();
    // along H: [2 * bd] slabs of [bh][bw]; along D: [2] slabs of [bd][bh * bw]
    launch_axis<int>(off, tmp, bh, bw, bw, 2 * bd, (long long)bh * bw, sy, sx, st);
    SEG_CHECK_LAUNCH();
    launch_axis<double>(tmp, dt2, bd, (long long)bh * bw, (int)((long long)bh * bw), 2, box, sz, 0.0, st);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int mi355seg_surface_distances_f64(const uint8_t* edges, int D, int H, int W, int z0, int y0, int x0, int bd, int bh, int bw,
                                   const double* dt2, long long n_gt, long long n_pred, double* dist, long long row_stride,
                                   int64_t* cursor, void* stream) {
    SEG_CHECK_ARG(edges && dt2 && dist && cursor && box_ok(D, H, W, z0, y0, x0, bd, bh, bw) && n_gt >= 0 && n_pred >= 0 &&
                  row_stride >= n_gt && row_stride >= n_pred, "surface_distances: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const long long box = (long long)bd * bh * bw;
    ProfScope ps(PF_LOSS, 0.0, 2.0 * box + 16.0 * (n_gt + n_pred), st);
    if (hipMemsetAsync(cursor, 0, 2 * sizeof(int64_t), st) != hipSuccess) { set_error("surface_distances: hipMemsetAsync failed"); return MI355SEG_EHIP; }
    hipLaunchKernelGGL(surface_gather_kernel, dim3(cdiv(box, (long long)kGatherPer * kSurfThreads)), dim3(kSurfThreads), 0, st, edges, (long long)D * H * W, H, W, z0, y0, x0,
                       bd, bh, bw, dt2, dist, row_stride, n_gt, n_pred, (unsigned long long*)cursor);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

size_t mi355seg_confusion_counts_ws_bytes(long long numel) { return (size_t)surf_grid(numel) * 8 * sizeof(long long); }

int mi355seg_confusion_counts_i64(const int64_t* gt, const int64_t* pred, long long numel, int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(gt && pred && counts && numel > 0, "confusion_counts: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, 16.0 * numel, st);
    const int nblk = surf_grid(numel);
    SEG_CHECK_WS(mi355seg_confusion_counts_ws_bytes(numel), ws_bytes);
    hipLaunchKernelGGL(confusion_counts_kernel, dim3(nblk), dim3(kSurfThreads), 0, st, gt, pred, numel, (long long*)ws);
    SEG_CHECK_LAUNCH();
    launch_sums_finalize<8>((const long long*)ws, nblk, (long long*)counts, st);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

}  // extern "C"
