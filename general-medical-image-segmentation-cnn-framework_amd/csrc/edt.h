// edt.h -- the two steps that the separable Euclidean distance transforms of surface.hip (fp64, exact, HD95) and boundary.hip (fp32,
// both polarities, the boundary loss) share.  Both families promise bits (exact against brute force; float32 of the fp64 reference
// at unit spacing), and the promises rest on details of these steps, so each has ONE definition.  What differs between the
// families stays with them: the block -> tile map, the source addressing and its "no site" encoding, the epilogues.
#pragma once
#include "common.h"

namespace seg {

// Pass W, a wave per line: the line's site bits lie in bits[0..nw) as 64-bit ballots.  The distance from bit k * 64 + lane to the
// nearest set bit on either side, by clz / ctz on the lane's own word and a walk over whole words; -1 where no bit is set.
__device__ __forceinline__ int nearest_set_bit(const unsigned long long* bits, int nw, int k, int lane) {
    const int x = k * kWave + lane;
    const unsigned long long own = bits[k];
    const unsigned long long le = own & (~0ull >> (kWave - 1 - lane));     // bits 0..lane
    const unsigned long long ge = own & (~0ull << lane);                  // bits lane..63
    int left = -1, right = -1;
    if (le) left = lane - (63 - __clzll((long long)le));
    else
        for (int q = k - 1; q >= 0; --q)
            if (bits[q]) { left = x - (q * kWave + 63 - __clzll((long long)bits[q])); break; }
    if (ge) right = (__ffsll((long long)ge) - 1) - lane;
    else
        for (int q = k + 1; q < nw; ++q)
            if (bits[q]) { right = q * kWave + (__ffsll((long long)bits[q]) - 1) - x; break; }
    return left < 0 ? right : (right < 0 ? left : min(left, right));
}

// Passes H and D, the plain min-plus step g(i) = min_j f(j) + (s*i - s*j)^2 with every j of an axis of `n` elements, no lower
// envelope.  A block of TW * TY threads owns TW columns and RI * TY output rows; thread (tx, ty) holds rows i0 .. i0 + RI of
// column tx in registers.  The source line passes through LDS TJ rows at a time, so that the caller's loads run along W:
// load(p, j) is f(j) of plane p in this thread's column, +inf for "no site" and for a column outside the volume.  P planes are
// staged side by side.  kSelect = false: acc[p][r] = g of plane p.  kSelect = true (P = 2): ONE accumulator, acc[0][r] = g of
// plane sel[r] ? 1 : 0 -- both planes are staged because the rows of a tile choose differently.
template <typename T, int P, bool kSelect, int TW, int TY, int TJ, int RI, class Load>
__device__ __forceinline__ void minplus_axis(T (&acc)[kSelect ? 1 : P][RI], const bool (&sel)[RI], Load load, int n, T s, int i0, int tx, int ty) {
    // s*i and s*j are each rounded on their own, never contracted into the subtraction, so that i == j gives exactly 0
#pragma clang fp contract(off)
    static_assert(!kSelect || P == 2, "a bool selects between two planes");
    constexpr int A = kSelect ? 1 : P;
    __shared__ T tile[P][TJ][TW];
    // the minima are kept in an array of this function and handed over at the end: accumulated through the caller's reference,
    // every one of them is carried round the chunk loop twice (RI = 32 in fp64: 256 VGPRs where this form takes 234)
    T a[A][RI], si[RI];
#pragma unroll
    for (int r = 0; r < RI; ++r) {
#pragma unroll
        for (int p = 0; p < A; ++p) a[p][r] = (T)INFINITY;
        si[r] = s * (T)(i0 + r);
    }
    for (int j0 = 0; j0 < n; j0 += TJ) {
        const int nj = min(TJ, n - j0);
        __syncthreads();
        for (int j = ty; j < nj; j += TY) {
#pragma unroll
            for (int p = 0; p < P; ++p) tile[p][j][tx] = load(p, j0 + j);
        }
        __syncthreads();
        for (int j = 0; j < nj; ++j) {
            const T sj = s * (T)(j0 + j);
#pragma unroll
            for (int r = 0; r < RI; ++r) {
                const T d = si[r] - sj;
                if constexpr (kSelect) {
                    // both planes read outside the choice: the unrolled rows then share one pair of LDS reads per j (read under the
                    // choice they cannot, and the pass takes half as long again)
                    const T f0 = tile[0][j][tx], f1 = tile[1][j][tx];
                    a[0][r] = fmin(a[0][r], fma(d, d, sel[r] ? f1 : f0));
                } else {
#pragma unroll
                    for (int p = 0; p < P; ++p) a[p][r] = fmin(a[p][r], fma(d, d, tile[p][j][tx]));
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < A; ++p)
#pragma unroll
        for (int r = 0; r < RI; ++r) acc[p][r] = a[p][r];
}

}  // namespace seg
