// band.hip -- the IS network's low-pass / high-pass input split (train.py:76-88,198-201: low_pass_torch / high_pass_torch at limit 0.04)
// as a low-rank projection.  The reference masks the 2-D spectrum of every [H,W] slice with an outer product of per-axis masks, so
//   low  = P_H X P_W          high = (I - E_H) X (I - E_W)
// with P_n the orthogonal projector onto the real Fourier modes of length n below the limit and E_n the one onto the modes not above
// it.  With orthonormal basis rows Eh [qH,H], Ew [qW,W] (the first r rows span P) and U = X Ew^T [H,qW], V = Eh X [qH,W], A = Eh U:
//   low  = Eh[:r]^T (A[:r,:r] Ew[:r])               = Eh[:r]^T L
//   high = X - Eh^T (V - A Ew) - U Ew               = X - Eh^T V' - U Ew
// One workgroup per output slice, one launch per call.  The slice (for B or C = 2: the sum / difference the reference's all-axes
// forward transform leaves on those axes, formed while loading) is staged in LDS in row chunks -- one chunk when it fits, which it
// does up to 160x192 -- and each chunk gives its rows of U and its share of V.  A, L and V' follow from U and V alone; then the chunks
// are visited again (re-staged from L2 only when there is more than one) and low / high leave as 16-byte stores.  Every sum runs in
// fp32 in a fixed order (four interleaved partial sums per dot product; the lanes that share a dot product of A add up in a
// fixed tree), no atomics: bitwise reproducible.
//   waves share the U / V work as a task list: a U task is 64 rows (one per lane; the row pitch is 4 mod 8 words, so the 16-byte
//     reads of eight lanes fall on different banks) x 4 basis rows, a V task is 64 columns x 4 basis rows; the basis values of a
//     task are wave-uniform and come through the scalar cache;
//   the output pass gives a thread 4 rows x 4 columns: per basis row two 16-byte LDS reads and one 16-byte basis load feed 32 FMAs.
#include "common.h"

namespace seg {

constexpr int kBandThreads = 1024;                  // 4 waves per SIMD: the phases are chains of dependent loads, so waves hide them
constexpr int kBandWaves = kBandThreads / kWave;
constexpr int kBandMaxN = 256;                      // longest filtered axis
constexpr int kBandMaxQ = 32;                       // most basis rows per axis
static_assert(kBandMaxQ * kBandMaxQ <= kBandThreads, "A = Eh U: one thread (or more) per element");
constexpr int kBandLdsFloats = 160 * 1024 / 4;      // one workgroup may take the whole LDS of a CU
constexpr int kBandT = 4;                           // basis rows per U / V task

struct BandArgs {
    const float* x; const float* eh; const float* ew; float* low; float* high;
    int B, C, D, H, W, rH, qH, rW, qW;
    int W4, P, UP, CH, nchunks;                     // W rounded up to 4; pitch of a staged row; pitch of U; rows per chunk; chunks
    int ehvec;                                      // Eh rows can be read 16 bytes at a time
};

// LDS plan for a shape: false when even a four-row chunk does not fit (never for a supported shape)
static bool band_plan(BandArgs& a) {
    a.W4 = (a.W + 3) & ~3;
    a.P = (a.W4 % 8 == 0) ? a.W4 + 4 : a.W4;
    a.UP = a.qW | 1;
    const int aux = (a.qH + a.rH) * a.W4 + a.H * a.UP + a.qH * a.qW + 4;
    const int chmax = ((kBandLdsFloats - aux) / a.P) & ~3;
    if (chmax < 4) return false;
    if (chmax >= a.H) { a.nchunks = 1; a.CH = a.H; return true; }
    a.nchunks = (a.H + chmax - 1) / chmax;
    a.CH = (((a.H + a.nchunks - 1) / a.nchunks) + 3) & ~3;
    return true;
}
static size_t band_lds_bytes(const BandArgs& a) {
    return sizeof(float) * ((size_t)a.CH * a.P + (size_t)(a.qH + a.rH) * a.W4 + (size_t)a.H * a.UP + (size_t)a.qH * a.qW + 4);
}

// four consecutive values of a basis row of length n from column j (j % 4 == 0); beyond the row: 0
template <bool VEC>
__device__ __forceinline__ f32x4_t band_row4(const float* __restrict__ row, int n, int j) {
    if constexpr (VEC) {
        return *reinterpret_cast<const f32x4_t*>(row + j);
    } else {
        f32x4_t v;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = (j + c < n) ? row[j + c] : 0.f;
        return v;
    }
}

// rows [row0, row0 + nrows) of the slice this workgroup filters -> Xs (pitch P, columns W .. W4-1 zero)
template <bool VEC>
__device__ __forceinline__ void band_stage(const BandArgs& a, int b, int c, int d, int row0, int nrows, float* __restrict__ Xs) {
    const long long HW = (long long)a.H * a.W;
    const int ng = a.W4 >> 2;
    const int total = nrows * ng;
    for (int g0 = threadIdx.x; g0 < total; g0 += 4 * kBandThreads) {          // four 16-byte groups in flight per thread
        f32x4_t acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int g = g0 + u * kBandThreads;
            if (g >= total) break;
            const int i = g / ng, j = (g - i * ng) << 2;
            for (int bb = 0; bb < a.B; ++bb)
                for (int cc = 0; cc < a.C; ++cc) {
                    // a length-2 forward transform that is never inverted: element 0 holds x0 + x1, element 1 holds x0 - x1
                    const float sg = (((b & bb) ^ (c & cc)) & 1) ? -1.f : 1.f;
                    const float* __restrict__ src = a.x + (((long long)bb * a.C + cc) * a.D + d) * HW + (long long)(row0 + i) * a.W;
                    const f32x4_t v = band_row4<VEC>(src, a.W, j);
                    if (bb == 0 && cc == 0) acc[u] = v;
                    else acc[u] += sg * v;
                }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int g = g0 + u * kBandThreads;
            if (g >= total) break;
            const int i = g / ng, j = (g - i * ng) << 2;
            *reinterpret_cast<f32x4_t*>(Xs + i * a.P + j) = acc[u];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kBandThreads) void band_split_kernel(BandArgs a) {
    extern __shared__ __align__(16) float band_lds[];
    float* __restrict__ Xs = band_lds;
    float* __restrict__ Vs = Xs + a.CH * a.P;           // V, then V' = V - A Ew          [qH][W4]
    float* __restrict__ Ls = Vs + a.qH * a.W4;          // L = A[:rH,:rW] Ew[:rW]         [rH][W4]
    float* __restrict__ Us = Ls + a.rH * a.W4;          // U                              [H][UP]
    float* __restrict__ As = Us + a.H * a.UP;           // A                              [qH][qW]
    const int slice = blockIdx.x;
    const int d = slice % a.D, c = (slice / a.D) % a.C, b = slice / (a.D * a.C);
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int H = a.H, W = a.W, W4 = a.W4, P = a.P, UP = a.UP, qH = a.qH, qW = a.qW, rH = a.rH, rW = a.rW;
    const float* __restrict__ eh = a.eh;
    const float* __restrict__ ew = a.ew;

    // ---- pass 1: U = X Ew^T (the chunk's rows) and V = Eh X (summed over the chunks in their order)
    for (int ch = 0; ch < a.nchunks; ++ch) {
        const int row0 = ch * a.CH, nrows = min(a.CH, H - row0);
        if (ch > 0) __syncthreads();
        band_stage<VEC>(a, b, c, d, row0, nrows, Xs);
        __syncthreads();
        const int nrb = (nrows + 63) >> 6, nUt = nrb * ((qW + kBandT - 1) / kBandT);
        const int ncb = (W4 + 63) >> 6, nVt = ncb * ((qH + kBandT - 1) / kBandT);
        for (int t = wid; t < nUt + nVt; t += kBandWaves) {
            float acc[kBandT][4];
#pragma unroll
            for (int e = 0; e < kBandT; ++e) acc[e][0] = acc[e][1] = acc[e][2] = acc[e][3] = 0.f;
            if (t < nUt) {
                const int m0 = (t / nrb) * kBandT, il = (t % nrb) * 64 + lane;
                const float* __restrict__ xr = Xs + min(il, nrows - 1) * P;
#pragma unroll 2
                for (int j = 0; j < W4; j += 4) {
                    const f32x4_t xv = *reinterpret_cast<const f32x4_t*>(xr + j);
#pragma unroll
                    for (int e = 0; e < kBandT; ++e) {
                        const f32x4_t ev = band_row4<VEC>(ew + (long long)min(m0 + e, qW - 1) * W, W, j);
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[e][q] = fmaf(xv[q], ev[q], acc[e][q]);
                    }
                }
                if (il < nrows) {
#pragma unroll
                    for (int e = 0; e < kBandT; ++e)
                        if (m0 + e < qW) Us[(row0 + il) * UP + m0 + e] = (acc[e][0] + acc[e][1]) + (acc[e][2] + acc[e][3]);
                }
            } else {
                const int tv = t - nUt, k0 = (tv / ncb) * kBandT, j = (tv % ncb) * 64 + lane;
                const float* __restrict__ xc = Xs + min(j, W4 - 1);
                int i = 0;
                for (; i + 4 <= nrows; i += 4) {
                    float xv[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) xv[q] = xc[(i + q) * P];
#pragma unroll
                    for (int e = 0; e < kBandT; ++e) {
                        const float* __restrict__ er = eh + (long long)min(k0 + e, qH - 1) * H + row0 + i;
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[e][q] = fmaf(er[q], xv[q], acc[e][q]);
                    }
                }
                for (; i < nrows; ++i) {
                    const float xv = xc[i * P];
#pragma unroll
                    for (int e = 0; e < kBandT; ++e) acc[e][0] = fmaf(eh[(long long)min(k0 + e, qH - 1) * H + row0 + i], xv, acc[e][0]);
                }
                if (j < W4) {
#pragma unroll
                    for (int e = 0; e < kBandT; ++e)
                        if (k0 + e < qH) {
                            const float v = (acc[e][0] + acc[e][1]) + (acc[e][2] + acc[e][3]);
                            float* p = Vs + (k0 + e) * W4 + j;
                            *p = ch == 0 ? v : *p + v;
                        }
                }
            }
        }
    }
    __syncthreads();

    // ---- A = Eh U
    // (qH qW <= 1024 dot products of length H: ns adjacent lanes take every ns-th term of one, then add up in a fixed tree)
    {
        int ns = 1;
        while (ns < 64 && 2 * ns * qH * qW <= kBandThreads) ns *= 2;
        const int idx = threadIdx.x / ns, part = threadIdx.x % ns;
        const bool live = idx < qH * qW;
        const int k = live ? idx / qW : 0, m = live ? idx - k * qW : 0;
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            const float* __restrict__ er = eh + (long long)k * H;
            int i = part;
            for (; i + 3 * ns < H; i += 4 * ns) {
#pragma unroll
                for (int q = 0; q < 4; ++q) s[q] = fmaf(er[i + q * ns], Us[(i + q * ns) * UP + m], s[q]);
            }
            for (; i < H; i += ns) s[0] = fmaf(er[i], Us[i * UP + m], s[0]);
        }
        float v = (s[0] + s[1]) + (s[2] + s[3]);
        for (int o = ns >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (live && part == 0) As[idx] = v;
    }
    __syncthreads();

    // ---- L = A[:rH,:rW] Ew[:rW] and V' = V - A Ew (columns W .. W4-1 are zero)
    for (int idx = threadIdx.x; idx < qH * W4; idx += kBandThreads) {
        const int k = idx / W4, j = idx - k * W4;
        float s = 0.f, sl = 0.f;
        if (j < W) {
            for (int m0 = 0; m0 < qW; m0 += 4) {
                float e[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) e[u] = ew[(long long)min(m0 + u, qW - 1) * W + j];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (m0 + u == rW) sl = s;
                    if (m0 + u < qW) s = fmaf(As[k * qW + m0 + u], e[u], s);
                }
            }
            if (rW == qW) sl = s;
        }
        Vs[idx] = j < W ? Vs[idx] - s : 0.f;
        if (k < rH) Ls[idx] = sl;
    }
    __syncthreads();

    // ---- pass 2: low = Eh[:rH]^T L, high = X - Eh^T V' - U Ew
    const long long HW = (long long)H * W;
    float* __restrict__ lo = a.low + (long long)slice * HW;
    float* __restrict__ hi = a.high + (long long)slice * HW;
    const int ncg = W4 >> 2;
    for (int ch = 0; ch < a.nchunks; ++ch) {
        const int row0 = ch * a.CH, nrows = min(a.CH, H - row0);
        if (a.nchunks > 1) {
            __syncthreads();
            band_stage<VEC>(a, b, c, d, row0, nrows, Xs);
            __syncthreads();
        }
        const int ntile = ((nrows + 3) >> 2) * ncg;
        for (int tile = threadIdx.x; tile < ntile; tile += kBandThreads) {
            const int rb = tile / ncg, j = (tile - rb * ncg) << 2;
            const int i0 = row0 + rb * 4;                       // a multiple of 4: every chunk starts on one
            int ir[4];
            f32x4_t h[4], l[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ir[r] = min(i0 + r, H - 1);
                h[r] = *reinterpret_cast<const f32x4_t*>(Xs + (ir[r] - row0) * P + j);
                l[r] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            }
            for (int k0 = 0; k0 < qH; k0 += 4) {                // four basis rows in flight (indices clamped, sums guarded)
                f32x4_t e[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float* __restrict__ er = eh + (long long)min(k0 + u, qH - 1) * H;
                    if (a.ehvec) e[u] = *reinterpret_cast<const f32x4_t*>(er + i0);
                    else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) e[u][r] = er[ir[r]];
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = k0 + u;
                    if (k >= qH) break;
                    const f32x4_t vv = *reinterpret_cast<const f32x4_t*>(Vs + k * W4 + j);
#pragma unroll
                    for (int r = 0; r < 4; ++r) h[r] -= e[u][r] * vv;
                    if (k < rH) {
                        const f32x4_t lv = *reinterpret_cast<const f32x4_t*>(Ls + k * W4 + j);
#pragma unroll
                        for (int r = 0; r < 4; ++r) l[r] += e[u][r] * lv;
                    }
                }
            }
            for (int m0 = 0; m0 < qW; m0 += 4) {
                f32x4_t ev[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) ev[u] = band_row4<VEC>(ew + (long long)min(m0 + u, qW - 1) * W, W, j);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int m = m0 + u;
                    if (m >= qW) break;
#pragma unroll
                    for (int r = 0; r < 4; ++r) h[r] -= Us[ir[r] * UP + m] * ev[u];
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (i0 + r >= H) break;
                const long long o = (long long)(i0 + r) * W + j;
                if constexpr (VEC) {
                    *reinterpret_cast<f32x4_t*>(lo + o) = l[r];
                    *reinterpret_cast<f32x4_t*>(hi + o) = h[r];
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (j + q < W) { lo[o + q] = l[r][q]; hi[o + q] = h[r][q]; }
                }
            }
        }
    }
}

static bool band_shape_ok(int B, int C, int D, int H, int W, int rH, int qH, int rW, int qW) {
    return (B == 1 || B == 2) && (C == 1 || C == 2) && D >= 1 && H >= 1 && H <= kBandMaxN && W >= 1 && W <= kBandMaxN
        && rH >= 0 && rH <= qH && qH <= (H < kBandMaxQ ? H : kBandMaxQ) && rW >= 0 && rW <= qW && qW <= (W < kBandMaxQ ? W : kBandMaxQ)
        && (long long)B * C * D < (1ll << 31);
}

}  // namespace seg

using namespace seg;

extern "C" {

int mi355seg_band_split_supported(int B, int C, int D, int H, int W, int rH, int qH, int rW, int qW) {
    if (!band_shape_ok(B, C, D, H, W, rH, qH, rW, qW)) return 0;
    BandArgs a{};
    a.H = H; a.W = W; a.rH = rH; a.qH = qH; a.rW = rW; a.qW = qW;
    return band_plan(a) ? a.nchunks : 0;
}

int mi355seg_band_split_f32(const float* x, int B, int C, int D, int H, int W, const float* basis_h, int rH, int qH,
                            const float* basis_w, int rW, int qW, float* low, float* high, void* stream) {
    SEG_CHECK_ARG(x && low && high && (basis_h || qH == 0) && (basis_w || qW == 0), "band_split: null pointer");
    SEG_CHECK_ARG(band_shape_ok(B, C, D, H, W, rH, qH, rW, qW),
                  "band_split: unsupported shape [%d,%d,%d,%d,%d] with (r, q) = (%d, %d) / (%d, %d): B, C in {1, 2} (the reference's forward "
                  "transform also covers the batch and channel axes, defined for lengths 1 and 2 only), D >= 1, 1 <= H, W <= %d, "
                  "0 <= r <= q <= min(n, %d)", B, C, D, H, W, rH, qH, rW, qW, kBandMaxN, kBandMaxQ);
    BandArgs a{};
    a.x = x; a.eh = basis_h; a.ew = basis_w; a.low = low; a.high = high;
    a.B = B; a.C = C; a.D = D; a.H = H; a.W = W; a.rH = rH; a.qH = qH; a.rW = rW; a.qW = qW;
    SEG_CHECK_ARG(band_plan(a), "band_split: no LDS plan for %dx%d slices with %d / %d basis rows", H, W, qH, qW);
    a.ehvec = (H % 4 == 0) && ((uintptr_t)basis_h % 16 == 0);
    const bool vec = (W % 4 == 0) && ((uintptr_t)x % 16 == 0) && ((uintptr_t)low % 16 == 0) && ((uintptr_t)high % 16 == 0)
                     && ((uintptr_t)basis_w % 16 == 0);
    hipStream_t st = (hipStream_t)stream;
    const double n = (double)B * C * D * H * W;
    ProfScope ps(PF_LOSS, 2.0 * n * (rH + 2 * qH + 2 * qW), 12.0 * n, st);
    const size_t lds = band_lds_bytes(a);
    const dim3 grid((unsigned)(B * C * D));
    if (vec) {
        SEG_SET_LDS((band_split_kernel<true>), kBandLdsFloats * 4);
        hipLaunchKernelGGL(band_split_kernel<true>, grid, dim3(kBandThreads), lds, st, a);
    } else {
        SEG_SET_LDS((band_split_kernel<false>), kBandLdsFloats * 4);
        hipLaunchKernelGGL(band_split_kernel<false>, grid, dim3(kBandThreads), lds, st, a);
    }
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

}  // extern "C"
