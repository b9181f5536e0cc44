// resample.hip -- whole-volume resampling to a target voxel spacing (config.resample_spacing): the cubic B-spline prefilter, the
// size-changing separable gather at order 0 / 1 / 3, the label resampler that interpolates class membership, and the fused
// trilinear resample + argmax of the way back.  The reference's dataloader.py:10 imports tio.Resample and never wires it in; UNPINNED,
// as the rest of the data path: the definitions in include/mi355seg.h ("Resampling") are the specification, scipy.ndimage the oracle.
//
// The map is axis-aligned and separable, so the HOST forms one table per axis in fp64 (base index and fraction per output index)
// and no coordinate arithmetic happens here: order 0 is exact by construction.  The three tables of a call are packed z, y, x in one
// int32 array (base) and one fp32 array (frac), each Do + Ho + Wo long.
//
// (a) Prefilter: pole z = sqrt(3) - 2, gain 6 per axis, whole-sample-symmetric boundary (scipy's "mirror"); per line
//       c+[0] = g0 * sum_{k < K} z^k s[m(k)],  c+[i] = fma(z, c+[i-1], 6 s[i]);   c[n-1] = fma(z, c+[n-2], c+[n-1]) * z / (z^2 - 1),
//       c[i] = z * (c[i+1] - c+[i])
//     with K = 14, g0 = 6 for n >= 14 (|z|^14 < 2^-25) and the exact mirrored period K = 2n - 2, g0 = 6 / (1 - z^(2n-2)) below.
//     Along H and D: one thread per line, lanes adjacent in W (coalesced), the causal pass leaves c+ in the output, the anticausal
//     pass re-reads it; eight loads are in flight before the first is used.  Along W: one wave per 64 lines, 64-column chunks staged
//     in LDS at a pitch of 65 floats (lane t walks row t: bank (t + j) mod 32, conflict-free; the chunk loads and stores are 256 B per
//     row), the causal carry rides in a register from chunk to chunk in order, the anticausal pass walks the chunks backwards; the
//     last chunk stays in LDS between the two.  No bound on W.  fp32, FMA in a fixed order: bitwise reproducible, in place allowed.
//     The recursion STATE is a pair of floats (value + what its rounding lost: two-sum and FMA product residuals, all fp32), because a
//     plain fp32 state carries every step's rounding at the gain-scaled magnitude forward through the pole and measured 5.3e-6
//     against the fp64 filter where the bound of the tests is 4.8e-6; with the pair the error is the rounding of the stored c+ and
//     of the result.  The nested sums of the order-3 gather keep such a pair at every level, and its weights are pairs too.
// (b) Gather, order 0 / 1: one thread per output, 1 / 8 taps through the cache;  w = (wz * wy) * wx, an FMA chain over the corners
//     in the order (z, y, x) = 000, 001, 010, ... 111.
//     Order 3: a workgroup owns a box of outputs (4 x 8 x 32 unless the footprint says otherwise) and stages the source box its 64-tap
//     stencils touch in LDS, MIRRORED while it is staged, so the taps are contiguous there; the footprint follows from the first
//     and the last base of the box, and the host halves the box along its widest footprint until the tile fits 64 KB.  Per output
//     the three 4-weight vectors are formed once and the sum is nested x, then y, then z.
// (c) Labels: per output the weight of class k is the sum of the corner weights whose corner holds k; the largest wins, the lowest
//     class on a tie.  Written as a compare-and-add over the 8 corners (64 compares and selects; 16 accumulators would be 128), in a
//     fixed order so that equal classes get bitwise equal totals.  Output voxels that read a value that is no integer in 0 .. 15
//     are counted: block partials in a fixed order and a one-block finalise, no atomics.
// (d) Way back: K <= 16 channels, the trilinear value of (b) per class, first maximum wins; optionally the values are stored.
#include "common.h"
#include <math.h>

namespace seg {

constexpr int kRsThreads = 256;
static_assert(kRsThreads == kReduceThreads, "the block size of reduce.h");
constexpr int kRsMaxBlocks = 4096;                           // of the label kernel: one partial count each
constexpr float kPole = -0.26794919243112270647f;            // sqrt(3) - 2
constexpr float kAntiInit = 0.28867513459481288225f;         // z / (z^2 - 1)
constexpr int kInitTerms = MI355SEG_BSPLINE_INIT_TERMS;
constexpr int kWLines = 64, kWChunk = 64, kWPitch = 65;
constexpr int kBatch = 8;                                    // loads in flight per thread in the strided passes
constexpr int kCubicLdsFloats = 16384;                       // 64 KB

struct LineInit { int terms; float gain0; };
static LineInit line_init(int n) {
    if (n >= kInitTerms) return {kInitTerms, 6.f};
    const double z = sqrt(3.0) - 2.0;
    return {2 * n - 2, (float)(6.0 / (1.0 - pow(z, 2.0 * n - 2.0)))};
}

// ------------------------------------------------------------------------------------------------ (a) prefilter
// (h, l) <- z * (h + l) + 6 s, with h + l the unevaluated sum of two floats: the product and the sum give up their rounding errors
// exactly (FMA residual, two-sum), which l collects.  No contraction in here: the two-sum needs the plain rounded sum.
__device__ __forceinline__ void causal_step(float& h, float& l, float s) {
#pragma clang fp contract(off)
    const float p = kPole * h, pe = __builtin_fmaf(kPole, h, -p);
    const float g = 6.f * s, ge = __builtin_fmaf(6.f, s, -g);
    const float sh = p + g, bb = sh - p, se = (p - (sh - bb)) + (g - bb);
    const float lo = __builtin_fmaf(kPole, l, (se + pe) + ge);
    h = sh + lo;
    l = lo - (h - sh);
}
// (h, l) <- z * ((h + l) - (cp + cpl))
__device__ __forceinline__ void anticausal_step(float& h, float& l, float cp, float cpl) {
#pragma clang fp contract(off)
    const float d = h - cp, bb = d - h, de = (h - (d - bb)) - (cp + bb);
    const float p = kPole * d, pe = __builtin_fmaf(kPole, d, -p);
    const float lo = __builtin_fmaf(kPole, (de + l) - cpl, pe);
    h = p + lo;
    l = lo - (h - p);
}
// c[n-1] from the last two causal states (h2 + l2 = c+[n-2], h1 + l1 = c+[n-1])
__device__ __forceinline__ float anticausal_start(float h2, float l2, float h1, float l1) {
#pragma clang fp contract(off)
    return (__builtin_fmaf(kPole, h2, h1) + __builtin_fmaf(kPole, l2, l1)) * kAntiInit;
}
// (h, l) += w * v, the product's and the sum's rounding errors collected in l
__device__ __forceinline__ void pair_fma(float w, float v, float& h, float& l) {
#pragma clang fp contract(off)
    const float p = w * v, pe = __builtin_fmaf(w, v, -p);
    const float s = h + p, bb = s - h, se = (h - (s - bb)) + (p - bb);
    l += se + pe;
    h = s;
}

// lines of n elements at stride `inner`: line g = (o, in) starts at o * n * inner + in
__global__ __launch_bounds__(kRsThreads) void prefilter_strided_kernel(const float* x, float* y, float* lw, long long nlines, int n, long long inner,
                                                                       int terms, float gain0) {
    const long long g = (long long)blockIdx.x * kRsThreads + threadIdx.x;
    if (g >= nlines) return;
    const long long o = g / inner, in = g - o * inner;
    const float* px = x + o * n * inner + in;
    float* py = y + o * n * inner + in;
    float* pl = lw + o * n * inner + in;                    // the low halves of c+ between the two passes
    float sum = 0.f, zk = 1.f;
    for (int k = 0; k < terms; ++k) {
        const int idx = k < n ? k : 2 * n - 2 - k;
        sum = __builtin_fmaf(zk, px[idx * inner], sum);
        zk *= kPole;
    }
    float h = sum * gain0, l = 0.f, h2 = 0.f, l2 = 0.f;
    py[0] = h;
    pl[0] = 0.f;
    float v[kBatch], vl[kBatch];
    for (int i = 1; i < n; i += kBatch) {
#pragma unroll
        for (int u = 0; u < kBatch; ++u) v[u] = i + u < n ? px[(i + u) * inner] : 0.f;
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            if (i + u < n) {
                h2 = h; l2 = l;
                causal_step(h, l, v[u]);
                py[(i + u) * inner] = h;
                pl[(i + u) * inner] = l;
            }
        }
    }
    h = anticausal_start(h2, l2, h, l);
    l = 0.f;
    py[(long long)(n - 1) * inner] = h;
    for (int i = n - 2; i >= 0; i -= kBatch) {
#pragma unroll
        for (int u = 0; u < kBatch; ++u) { v[u] = i - u >= 0 ? py[(i - u) * inner] : 0.f; vl[u] = i - u >= 0 ? pl[(i - u) * inner] : 0.f; }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            if (i - u >= 0) {
                anticausal_step(h, l, v[u], vl[u]);
                py[(i - u) * inner] = h;
            }
        }
    }
}

// contiguous lines (along W): one wave per kWLines lines, chunks of kWChunk columns through LDS
__global__ __launch_bounds__(kWLines) void prefilter_w_kernel(const float* x, float* y, float* lw, long long nlines, int n, int terms, float gain0) {
    __shared__ float sh[kWLines * kWPitch], shl[kWLines * kWPitch];
    const int lane = threadIdx.x;
    const long long line0 = (long long)blockIdx.x * kWLines;
    const int nl = (int)(nlines - line0 < kWLines ? nlines - line0 : kWLines);
    const int nch = (n + kWChunk - 1) / kWChunk;
    const bool own = lane < nl;
    float* row = sh + lane * kWPitch;
    float* rowl = shl + lane * kWPitch;
    float h = 0.f, l = 0.f, h2 = 0.f, l2 = 0.f;
    for (int ch = 0; ch < nch; ++ch) {
        const int c0 = ch * kWChunk, cw = n - c0 < kWChunk ? n - c0 : kWChunk;
        if (lane < cw)
            for (int r = 0; r < nl; ++r) sh[r * kWPitch + lane] = x[(line0 + r) * n + c0 + lane];
        __syncthreads();
        if (own) {
            int j = 0;
            if (ch == 0) {                                   // n < 14 < kWChunk or K = 14: every term is in the first chunk
                float sum = 0.f, zk = 1.f;
                for (int k = 0; k < terms; ++k) {
                    sum = __builtin_fmaf(zk, row[k < n ? k : 2 * n - 2 - k], sum);
                    zk *= kPole;
                }
                h = sum * gain0;
                row[0] = h;
                rowl[0] = 0.f;
                j = 1;
            }
            for (; j < cw; ++j) {
                h2 = h; l2 = l;
                causal_step(h, l, row[j]);
                row[j] = h;
                rowl[j] = l;
            }
        }
        __syncthreads();
        if (ch != nch - 1) {                                 // the last chunk stays in LDS for the way back
            if (lane < cw)
                for (int r = 0; r < nl; ++r) {
                    y[(line0 + r) * n + c0 + lane] = sh[r * kWPitch + lane];
                    lw[(line0 + r) * n + c0 + lane] = shl[r * kWPitch + lane];
                }
            __syncthreads();
        }
    }
    for (int ch = nch - 1; ch >= 0; --ch) {
        const int c0 = ch * kWChunk, cw = n - c0 < kWChunk ? n - c0 : kWChunk;
        if (ch != nch - 1) {
            if (lane < cw)
                for (int r = 0; r < nl; ++r) {
                    sh[r * kWPitch + lane] = y[(line0 + r) * n + c0 + lane];
                    shl[r * kWPitch + lane] = lw[(line0 + r) * n + c0 + lane];
                }
            __syncthreads();
        }
        if (own) {
            int j = cw - 1;
            if (ch == nch - 1) {
                h = anticausal_start(h2, l2, h, l);
                l = 0.f;
                row[j] = h;
                --j;
            }
            for (; j >= 0; --j) {
                anticausal_step(h, l, row[j], rowl[j]);
                row[j] = h;
            }
        }
        __syncthreads();
        if (lane < cw)
            for (int r = 0; r < nl; ++r) y[(line0 + r) * n + c0 + lane] = sh[r * kWPitch + lane];
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ (b) gathers
// the eight corners of an output voxel: offsets into one source channel and the weights (wz * wy) * wx, corner order zyx = 000 .. 111
struct Corners { int off[8]; float w[8]; };
__device__ __forceinline__ void corners_of(const int* __restrict__ base, const float* __restrict__ frac, int oz, int oy, int ox,
                                           int D, int H, int W, int Do, int Ho, Corners& c) {
    const int z0 = base[oz], y0 = base[Do + oy], x0 = base[Do + Ho + ox];
    const float fz = frac[oz], fy = frac[Do + oy], fx = frac[Do + Ho + ox];
    const int z1 = z0 + 1 < D ? z0 + 1 : D - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1, x1 = x0 + 1 < W ? x0 + 1 : W - 1;
    const float wz[2] = {1.f - fz, fz}, wy[2] = {1.f - fy, fy}, wx[2] = {1.f - fx, fx};
    const int zz[2] = {z0, z1}, yy[2] = {y0, y1}, xx[2] = {x0, x1};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int a = i >> 2, b = (i >> 1) & 1, d = i & 1;
        c.off[i] = (zz[a] * H + yy[b]) * W + xx[d];
        c.w[i] = (wz[a] * wy[b]) * wx[d];
    }
}
__device__ __forceinline__ float trilinear(const float* __restrict__ p, const Corners& c) {
    float acc = c.w[0] * p[c.off[0]];
#pragma unroll
    for (int i = 1; i < 8; ++i) acc = __builtin_fmaf(c.w[i], p[c.off[i]], acc);
    return acc;
}

template <int ORDER>
__global__ __launch_bounds__(kRsThreads) void resample_kernel(const float* __restrict__ x, int D, int H, int W, const int* __restrict__ base,
                                                              const float* __restrict__ frac, float* __restrict__ y, int Do, int Ho, int Wo,
                                                              unsigned total) {
    const unsigned i = blockIdx.x * (unsigned)kRsThreads + threadIdx.x;
    if (i >= total) return;
    const unsigned ox = i % (unsigned)Wo, r1 = i / (unsigned)Wo, oy = r1 % (unsigned)Ho, r2 = r1 / (unsigned)Ho, oz = r2 % (unsigned)Do, c = r2 / (unsigned)Do;
    const float* p = x + (size_t)c * D * H * W;
    if (ORDER == 0) {
        y[i] = p[(base[oz] * H + base[Do + oy]) * W + base[Do + Ho + ox]];
    } else {
        Corners cn;
        corners_of(base, frac, (int)oz, (int)oy, (int)ox, D, H, W, Do, Ho, cn);
        y[i] = trilinear(p, cn);
    }
}

__device__ __forceinline__ int mirror_index(int i, int n) {
    if (n == 1) return 0;
    i = i < 0 ? -i : i;
    i = i > n - 1 ? 2 * (n - 1) - i : i;
    return i < 0 ? -i : i;
}
// the four weights of the taps base - 1 .. base + 2 at fraction t, each as a pair of floats: formed in fp64 from the fp32 fraction (a
// dozen fp64 operations per output beside 84 compensated fp32 multiply-adds) and split, because weights rounded to fp32 were the
// largest part of the order-3 error on data that is not smooth at the voxel scale (1.3e-6 of 1.6e-6 on the tests' volume input)
__device__ __forceinline__ void bspline3_weights(float tf, float (&w)[4], float (&wl)[4]) {
    const double t = tf, u = 1.0 - t;
    const double d[4] = {u * u * u / 6.0, t * t * (0.5 * t - 1.0) + 2.0 / 3.0, u * u * (0.5 * u - 1.0) + 2.0 / 3.0, t * t * t / 6.0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        w[k] = (float)d[k];
        wl[k] = (float)(d[k] - (double)w[k]);
    }
}

// the output box of a workgroup is (1 << sz) x (1 << sy) x (1 << sx); `pitch` is the LDS row pitch (odd, at least the widest footprint)
struct CubicTiling { int sz, sy, sx, ntz, nty, ntx, pitch; };
__global__ __launch_bounds__(kRsThreads) void resample_cubic_kernel(const float* __restrict__ x, int D, int H, int W, const int* __restrict__ base,
                                                                    const float* __restrict__ frac, float* __restrict__ y, int Do, int Ho, int Wo,
                                                                    CubicTiling t) {
    extern __shared__ float sh[];
    unsigned b = blockIdx.x;
    const int tx = (int)(b % (unsigned)t.ntx); b /= (unsigned)t.ntx;
    const int ty = (int)(b % (unsigned)t.nty); b /= (unsigned)t.nty;
    const int tz = (int)(b % (unsigned)t.ntz);
    const int c = (int)(b / (unsigned)t.ntz);
    const int oz0 = tz << t.sz, oy0 = ty << t.sy, ox0 = tx << t.sx;
    const int oz1 = (oz0 + (1 << t.sz) < Do ? oz0 + (1 << t.sz) : Do) - 1;
    const int oy1 = (oy0 + (1 << t.sy) < Ho ? oy0 + (1 << t.sy) : Ho) - 1;
    const int ox1 = (ox0 + (1 << t.sx) < Wo ? ox0 + (1 << t.sx) : Wo) - 1;
    const int* bz = base;
    const int* by = base + Do;
    const int* bx = base + Do + Ho;
    const int lz = bz[oz0] - 1, ly = by[oy0] - 1, lx = bx[ox0] - 1;             // first tap of the box, before mirroring
    const int nz = bz[oz1] + 2 - lz + 1, ny = by[oy1] + 2 - ly + 1, nx = bx[ox1] + 2 - lx + 1;
    const float* p = x + (size_t)c * D * H * W;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int row = wid; row < nz * ny; row += kRsThreads / 64) {
        const int zz = row / ny, yy = row - zz * ny;
        const float* srow = p + ((size_t)mirror_index(lz + zz, D) * H + mirror_index(ly + yy, H)) * W;
        for (int xx = lane; xx < nx; xx += 64) sh[row * t.pitch + xx] = srow[mirror_index(lx + xx, W)];
    }
    __syncthreads();
    const int nto = 1 << (t.sz + t.sy + t.sx);
    for (int o = threadIdx.x; o < nto; o += kRsThreads) {
        const int ox = ox0 + (o & ((1 << t.sx) - 1)), oy = oy0 + ((o >> t.sx) & ((1 << t.sy) - 1)), oz = oz0 + (o >> (t.sx + t.sy));
        if (ox > ox1 || oy > oy1 || oz > oz1) continue;
        float wz[4], wy[4], wx[4], wzl[4], wyl[4], wxl[4];
        bspline3_weights(frac[oz], wz, wzl);
        bspline3_weights(frac[Do + oy], wy, wyl);
        bspline3_weights(frac[Do + Ho + ox], wx, wxl);
        const int az = bz[oz] - 1 - lz, ay = by[oy] - 1 - ly, ax = bx[ox] - 1 - lx;
        float acc = 0.f, acc_l = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            float plane = 0.f, plane_l = 0.f;
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) {
                const float* s = sh + ((az + a) * ny + ay + bb) * t.pitch + ax;
                float line = 0.f, line_l = 0.f;
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    pair_fma(wx[d], s[d], line, line_l);
                    line_l = __builtin_fmaf(wxl[d], s[d], line_l);
                }
                pair_fma(wy[bb], line, plane, plane_l);
                plane_l = __builtin_fmaf(wy[bb], line_l, __builtin_fmaf(wyl[bb], line, plane_l));
            }
            pair_fma(wz[a], plane, acc, acc_l);
            acc_l = __builtin_fmaf(wz[a], plane_l, __builtin_fmaf(wzl[a], plane, acc_l));
        }
        y[(((size_t)c * Do + oz) * Ho + oy) * Wo + ox] = acc + acc_l;
    }
}

// ------------------------------------------------------------------------------------------------ (c) labels
__device__ __forceinline__ bool label_ok(float v) { return v >= 0.f && v <= 15.f && v == floorf(v); }
__device__ __forceinline__ bool label_ok(long long v) { return v >= 0 && v <= 15; }

template <typename T>
__global__ __launch_bounds__(kRsThreads) void resample_labels_kernel(const T* __restrict__ x, int D, int H, int W, const int* __restrict__ base,
                                                                     const float* __restrict__ frac, int linear, T* __restrict__ y, int Do, int Ho,
                                                                     int Wo, unsigned total, long long* __restrict__ block_bad) {
    long long bad = 0;
    for (unsigned i = blockIdx.x * (unsigned)kRsThreads + threadIdx.x; i < total; i += gridDim.x * (unsigned)kRsThreads) {
        const unsigned ox = i % (unsigned)Wo, r1 = i / (unsigned)Wo, oy = r1 % (unsigned)Ho, r2 = r1 / (unsigned)Ho, oz = r2 % (unsigned)Do, c = r2 / (unsigned)Do;
        const T* p = x + (size_t)c * D * H * W;
        if (!linear) {
            const T v = p[(base[oz] * H + base[Do + oy]) * W + base[Do + Ho + ox]];
            bad += label_ok(v) ? 0 : 1;
            y[i] = v;
            continue;
        }
        Corners cn;
        corners_of(base, frac, (int)oz, (int)oy, (int)ox, D, H, W, Do, Ho, cn);
        T l[8];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 8; ++j) { l[j] = p[cn.off[j]]; ok = ok && label_ok(l[j]); }
        T best = l[0];
        float best_w = -1.f;
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            float tot = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) tot += l[j] == l[a] ? cn.w[j] : 0.f;
            const bool take = tot > best_w || (tot == best_w && l[a] < best);
            best = take ? l[a] : best;
            best_w = take ? tot : best_w;
        }
        bad += ok ? 0 : 1;
        y[i] = best;
    }
    bad = block_reduce_one<OpSum>(bad);
    if (threadIdx.x == 0) block_bad[blockIdx.x] = bad;
}

// ------------------------------------------------------------------------------------------------ (d) way back
__global__ __launch_bounds__(kRsThreads) void resample_argmax_kernel(const float* __restrict__ prob, int K, int D, int H, int W,
                                                                     const int* __restrict__ base, const float* __restrict__ frac,
                                                                     long long* __restrict__ labels, float* __restrict__ prob_out, int Do, int Ho,
                                                                     int Wo, unsigned total) {
    const unsigned i = blockIdx.x * (unsigned)kRsThreads + threadIdx.x;
    if (i >= total) return;
    const unsigned ox = i % (unsigned)Wo, r1 = i / (unsigned)Wo, oy = r1 % (unsigned)Ho, oz = r1 / (unsigned)Ho;
    Corners cn;
    corners_of(base, frac, (int)oz, (int)oy, (int)ox, D, H, W, Do, Ho, cn);
    const size_t plane = (size_t)D * H * W;
    float best = trilinear(prob, cn);
    int arg = 0;
    if (prob_out) prob_out[i] = best;
    for (int k = 1; k < K; ++k) {
        const float v = trilinear(prob + k * plane, cn);
        if (prob_out) prob_out[(size_t)k * total + i] = v;
        if (v > best) { best = v; arg = k; }
    }
    labels[i] = arg;
}

// ------------------------------------------------------------------------------------------------ host side
// nullptr, or what is wrong with the shapes / the host copy of the base tables (the kernels trust the device copy)
static const char* tables_error(int order, const int* base_host, int C, int D, int H, int W, int Do, int Ho, int Wo) {
    if (C < 1 || D < 1 || H < 1 || W < 1 || Do < 1 || Ho < 1 || Wo < 1) return "sizes must be positive";
    if ((double)C * D * H * W >= 2147483648.0 || (double)C * Do * Ho * Wo >= 2147483648.0) return "a volume of 2^31 elements or more";
    if (!base_host) return "null table";
    const int n_in[3] = {D, H, W}, n_out[3] = {Do, Ho, Wo};
    const int* b = base_host;
    for (int a = 0; a < 3; ++a) {
        for (int o = 0; o < n_out[a]; ++o) {
            if (b[o] < 0 || b[o] >= n_in[a]) return "a table base outside the source";
            if (order == 3 && o > 0 && b[o] < b[o - 1]) return "a descending table (order 3 needs ascending bases)";
        }
        b += n_out[a];
    }
    return nullptr;
}
static bool aligned4(const void* p) { return ((uintptr_t)p % 4) == 0; }
static bool aligned8(const void* p) { return ((uintptr_t)p % 8) == 0; }

// the widest footprint along one axis of boxes of 1 << s outputs
static int axis_footprint(const int* b, int n_out, int s) {
    int f = 0;
    for (int o0 = 0; o0 < n_out; o0 += 1 << s) {
        const int o1 = (o0 + (1 << s) < n_out ? o0 + (1 << s) : n_out) - 1;
        const int w = b[o1] - b[o0] + 4;
        f = w > f ? w : f;
    }
    return f;
}

template <typename T>
static int resample_labels_launch(const char* who, const T* x, int C, int D, int H, int W, int mode, const int* base, const float* frac,
                                  const int* base_host, T* y, int Do, int Ho, int Wo, long long* bad, void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(mode == MI355SEG_RESAMPLE_LABELS_NEAREST || mode == MI355SEG_RESAMPLE_LABELS_LINEAR, "%s: mode %d is not 0 (nearest) or 1 (linear)", who, mode);
    SEG_CHECK_ARG(x && y && base && bad && ws && (frac || mode == MI355SEG_RESAMPLE_LABELS_NEAREST), "%s: null pointer", who);
    SEG_CHECK_ARG(((uintptr_t)x % sizeof(T)) == 0 && ((uintptr_t)y % sizeof(T)) == 0 && aligned4(base) && aligned4(frac) && aligned8(bad) && aligned8(ws),
                  "%s: misaligned pointer", who);
    SEG_CHECK_ARG(x != y, "%s: in place is not possible", who);
    const char* err = tables_error(mode, base_host, C, D, H, W, Do, Ho, Wo);
    SEG_CHECK_ARG(!err, "%s: %s", who, err);
    SEG_CHECK_WS(mi355seg_resample3d_labels_ws_bytes(), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    const unsigned total = (unsigned)((long long)C * Do * Ho * Wo);
    ProfScope ps(PF_POOL, 0.0, (double)sizeof(T) * ((double)C * D * H * W + total), st);
    const int nblk = stream_grid(total, kRsThreads, kRsMaxBlocks);
    hipLaunchKernelGGL(resample_labels_kernel<T>, dim3(nblk), dim3(kRsThreads), 0, st, x, D, H, W, base, frac, mode, y, Do, Ho, Wo, total, (long long*)ws);
    SEG_CHECK_LAUNCH();
    launch_sums_finalize<1>((const long long*)ws, nblk, bad, st);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}
}  // namespace seg

using namespace seg;

extern "C" {

size_t mi355seg_bspline3_prefilter_ws_bytes(int C, int D, int H, int W) {
    return C < 1 || D < 1 || H < 1 || W < 1 ? 0 : (size_t)C * D * H * W * sizeof(float);
}
int mi355seg_bspline3_prefilter_f32(const float* x, int C, int D, int H, int W, float* y, void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(x && y && ws, "bspline3_prefilter: null pointer");
    SEG_CHECK_ARG(aligned4(x) && aligned4(y) && aligned4(ws), "bspline3_prefilter: pointers must be 4-byte aligned");
    SEG_CHECK_ARG(C >= 1 && D >= 1 && H >= 1 && W >= 1, "bspline3_prefilter: sizes must be positive, got C %d D %d H %d W %d", C, D, H, W);
    SEG_CHECK_ARG((double)C * D * H * W < 2147483648.0, "bspline3_prefilter: the tensor has 2^31 elements or more");
    SEG_CHECK_WS(mi355seg_bspline3_prefilter_ws_bytes(C, D, H, W), ws_bytes);
    float* lw = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)C * D * H * W;
    ProfScope ps(PF_POOL, 0.0, 8.0 * total * ((W > 1) + 2 * (H > 1) + 2 * (D > 1)), st);
    const float* src = x;                                    // the first pass reads x, the rest work in place on y
    if (W > 1) {
        const LineInit li = line_init(W);
        const long long nlines = (long long)C * D * H;
        hipLaunchKernelGGL(prefilter_w_kernel, dim3(cdiv(nlines, kWLines)), dim3(kWLines), 0, st, src, y, lw, nlines, W, li.terms, li.gain0);
        SEG_CHECK_LAUNCH();
        src = y;
    }
    if (H > 1) {
        const LineInit li = line_init(H);
        const long long nlines = (long long)C * D * W;
        hipLaunchKernelGGL(prefilter_strided_kernel, dim3(cdiv(nlines, kRsThreads)), dim3(kRsThreads), 0, st, src, y, lw, nlines, H, (long long)W, li.terms, li.gain0);
        SEG_CHECK_LAUNCH();
        src = y;
    }
    if (D > 1) {
        const LineInit li = line_init(D);
        const long long nlines = (long long)C * H * W;
        hipLaunchKernelGGL(prefilter_strided_kernel, dim3(cdiv(nlines, kRsThreads)), dim3(kRsThreads), 0, st, src, y, lw, nlines, D, (long long)H * W, li.terms, li.gain0);
        SEG_CHECK_LAUNCH();
        src = y;
    }
    if (src == x && x != y && hipMemcpyAsync(y, x, (size_t)total * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
        set_error("bspline3_prefilter: hipMemcpyAsync failed");
        return MI355SEG_EHIP;
    }
    return MI355SEG_OK;
}

int mi355seg_bspline3_prefilter_axis_f32(const float* x, int C, int D, int H, int W, int axis, float* y, void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(x && y && ws, "bspline3_prefilter_axis: null pointer");
    SEG_CHECK_ARG(aligned4(x) && aligned4(y) && aligned4(ws), "bspline3_prefilter_axis: pointers must be 4-byte aligned");
    SEG_CHECK_ARG(C >= 1 && D >= 1 && H >= 1 && W >= 1, "bspline3_prefilter_axis: sizes must be positive, got C %d D %d H %d W %d", C, D, H, W);
    SEG_CHECK_ARG((double)C * D * H * W < 2147483648.0, "bspline3_prefilter_axis: the tensor has 2^31 elements or more");
    SEG_CHECK_ARG(axis >= 0 && axis <= 2, "bspline3_prefilter_axis: axis %d is not 0 (D), 1 (H) or 2 (W)", axis);
    const int n = axis == 0 ? D : axis == 1 ? H : W;
    SEG_CHECK_ARG(n >= 2, "bspline3_prefilter_axis: axis %d has length %d: a line of one sample is its own coefficient", axis, n);
    SEG_CHECK_WS(mi355seg_bspline3_prefilter_ws_bytes(C, D, H, W), ws_bytes);
    float* lw = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)C * D * H * W, nlines = total / n;
    ProfScope ps(PF_POOL, 0.0, (axis == 2 ? 8.0 : 16.0) * total, st);
    const LineInit li = line_init(n);
    if (axis == 2)
        hipLaunchKernelGGL(prefilter_w_kernel, dim3(cdiv(nlines, kWLines)), dim3(kWLines), 0, st, x, y, lw, nlines, W, li.terms, li.gain0);
    else
        hipLaunchKernelGGL(prefilter_strided_kernel, dim3(cdiv(nlines, kRsThreads)), dim3(kRsThreads), 0, st, x, y, lw, nlines, n,
                           axis == 1 ? (long long)W : (long long)H * W, li.terms, li.gain0);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int mi355seg_resample3d_f32(const float* x, int C, int D, int H, int W, int order, const int* base, const float* frac, const int* base_host,
                            float* y, int Do, int Ho, int Wo, void* stream) {
    SEG_CHECK_ARG(order == 0 || order == 1 || order == 3, "resample3d: order %d is not 0, 1 or 3", order);
    SEG_CHECK_ARG(x && y && base && (frac || order == 0), "resample3d: null pointer");
    SEG_CHECK_ARG(aligned4(x) && aligned4(y) && aligned4(base) && aligned4(frac), "resample3d: pointers must be 4-byte aligned");
    SEG_CHECK_ARG(x != y, "resample3d: in place is not possible");
    const char* err = tables_error(order, base_host, C, D, H, W, Do, Ho, Wo);
    SEG_CHECK_ARG(!err, "resample3d: %s", err);
    hipStream_t st = (hipStream_t)stream;
    const unsigned total = (unsigned)((long long)C * Do * Ho * Wo);
    ProfScope ps(PF_POOL, 0.0, 4.0 * ((double)C * D * H * W + total), st);
    if (order == 0) {
        hipLaunchKernelGGL(resample_kernel<0>, dim3(cdiv(total, kRsThreads)), dim3(kRsThreads), 0, st, x, D, H, W, base, frac, y, Do, Ho, Wo, total);
    } else if (order == 1) {
        hipLaunchKernelGGL(resample_kernel<1>, dim3(cdiv(total, kRsThreads)), dim3(kRsThreads), 0, st, x, D, H, W, base, frac, y, Do, Ho, Wo, total);
    } else {
        CubicTiling t;
        t.sz = 2; t.sy = 3; t.sx = 5;
        int fz, fy, fx;
        for (;;) {                                           // halve the box along its widest footprint until the tile fits
            fz = axis_footprint(base_host, Do, t.sz);
            fy = axis_footprint(base_host + Do, Ho, t.sy);
            fx = axis_footprint(base_host + Do + Ho, Wo, t.sx);
            t.pitch = fx | 1;
            if ((long long)fz * fy * t.pitch <= kCubicLdsFloats) break;
            if (fx >= fy && fx >= fz && t.sx > 0) --t.sx;
            else if (fy >= fz && t.sy > 0) --t.sy;
            else if (t.sz > 0) --t.sz;
            else if (t.sy > 0) --t.sy;
            else --t.sx;                                     // a box of one output needs 4 x 4 x 5 floats: the loop ends before this can underflow
        }
        t.ntz = cdiv(Do, 1 << t.sz); t.nty = cdiv(Ho, 1 << t.sy); t.ntx = cdiv(Wo, 1 << t.sx);
        const long long nblk = (long long)C * t.ntz * t.nty * t.ntx;
        SEG_CHECK_ARG(nblk < 2147483648ll, "resample3d: too many output boxes");
        const size_t lds = (size_t)fz * fy * t.pitch * sizeof(float);
        SEG_SET_LDS(resample_cubic_kernel, kCubicLdsFloats * sizeof(float));
        hipLaunchKernelGGL(resample_cubic_kernel, dim3((unsigned)nblk), dim3(kRsThreads), lds, st, x, D, H, W, base, frac, y, Do, Ho, Wo, t);
    }
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

size_t mi355seg_resample3d_labels_ws_bytes(void) { return (size_t)kRsMaxBlocks * sizeof(long long); }

int mi355seg_resample3d_labels_f32(const float* x, int C, int D, int H, int W, int mode, const int* base, const float* frac, const int* base_host,
                                   float* y, int Do, int Ho, int Wo, long long* bad, void* ws, size_t ws_bytes, void* stream) {
    return resample_labels_launch<float>("resample3d_labels_f32", x, C, D, H, W, mode, base, frac, base_host, y, Do, Ho, Wo, bad, ws, ws_bytes, stream);
}
int mi355seg_resample3d_labels_i64(const long long* x, int C, int D, int H, int W, int mode, const int* base, const float* frac, const int* base_host,
                                   long long* y, int Do, int Ho, int Wo, long long* bad, void* ws, size_t ws_bytes, void* stream) {
    return resample_labels_launch<long long>("resample3d_labels_i64", x, C, D, H, W, mode, base, frac, base_host, y, Do, Ho, Wo, bad, ws, ws_bytes, stream);
}

int mi355seg_resample3d_argmax_f32(const float* prob, int K, int D, int H, int W, const int* base, const float* frac, const int* base_host,
                                   long long* labels, float* prob_out, int Do, int Ho, int Wo, void* stream) {
    SEG_CHECK_ARG(prob && labels && base && frac, "resample3d_argmax: null pointer");
    SEG_CHECK_ARG(aligned4(prob) && aligned4(prob_out) && aligned4(base) && aligned4(frac) && aligned8(labels), "resample3d_argmax: misaligned pointer");
    SEG_CHECK_ARG(K >= 1 && K <= MI355SEG_RESAMPLE_MAX_CLASSES, "resample3d_argmax: K = %d is outside 1 .. %d", K, MI355SEG_RESAMPLE_MAX_CLASSES);
    SEG_CHECK_ARG(prob != prob_out, "resample3d_argmax: in place is not possible");
    const char* err = tables_error(1, base_host, K, D, H, W, Do, Ho, Wo);
    SEG_CHECK_ARG(!err, "resample3d_argmax: %s", err);
    hipStream_t st = (hipStream_t)stream;
    const unsigned total = (unsigned)((long long)Do * Ho * Wo);
    ProfScope ps(PF_POOL, 0.0, 4.0 * K * (double)D * H * W + (8.0 + (prob_out ? 4.0 * K : 0.0)) * total, st);
    hipLaunchKernelGGL(resample_argmax_kernel, dim3(cdiv(total, kRsThreads)), dim3(kRsThreads), 0, st, prob, K, D, H, W, base, frac, labels, prob_out,
                       Do, Ho, Wo, total);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

}  // extern "C"
