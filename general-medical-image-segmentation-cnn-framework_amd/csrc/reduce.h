// reduce.h -- the one two-stage reduction of the kernels that turn a volume into a few scalars.
//
// Stage 1, `stream_grid` blocks: every thread accumulates over its ascending grid-stride walk, `block_reduce` combines the block
// (xor butterfly 32, 16, ... 1 inside a wave, then the waves in ascending index, left to right, by thread 0) and thread 0 writes one
// partial row.  Stage 2, one block: thread t combines partial rows t, t + 256, ... in ascending order (`partials_reduce`) and the
// block is reduced once more.  No atomics and nothing that depends on the batch size: a floating-point sum has ONE order.
// Every kernel that calls the block helpers runs kReduceThreads threads: the wave count is a compile-time constant, so thread 0's
// reads of the other waves' slots are issued together (a loop over blockDim.x >> 6 makes them one LDS round trip each).
#pragma once
#include <hip/hip_runtime.h>

namespace seg {

// blocks of a grid-stride pass over `items` work items: ceil(items / threads), at least 1, at most `cap`
static inline int stream_grid(long long items, int threads, int cap) {
    const long long b = (items + threads - 1) / threads;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// An operation is apply(a, b, j): j is the value's index in the array being reduced (a constant once the loops are unrolled), so
// that a kernel can give its own Op that sums some entries and takes the minimum or maximum of others in ONE pass.
struct OpSum {
    template <typename T> static __device__ __forceinline__ T apply(T a, T b, int = 0) { return a + b; }
};
struct OpMin {
    template <typename T> static __device__ __forceinline__ T apply(T a, T b, int = 0) { return b < a ? b : a; }
    static __device__ __forceinline__ float apply(float a, float b, int = 0) { return fminf(a, b); }      // a NaN loses, as fminf
};
struct OpMax {
    template <typename T> static __device__ __forceinline__ T apply(T a, T b, int = 0) { return b > a ? b : a; }
    static __device__ __forceinline__ float apply(float a, float b, int = 0) { return fmaxf(a, b); }
};

// Combine across the 64 lanes of a wavefront (result valid in every lane).
template <class Op, typename T>
__device__ __forceinline__ T wave_reduce(T v, int j = 0) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = Op::apply(v, __shfl_xor(v, o, 64), j);
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_sum(T v) { return wave_reduce<OpSum>(v); }

// Combine NV values across the workgroup; the result is valid in thread 0.  Every thread must call it.
// THE WORKGROUP MUST BE kReduceThreads = 256 THREADS: thread 0 reads exactly kReduceWaves slots, so a smaller block would leave
// slots unwritten and a larger one would write past the array (each family static_asserts its block size against kReduceThreads).
// The LDS belongs to the helper, one array per instantiation (Op, Again, NV, T).  A kernel that calls the SAME instantiation more
// than once passes Again = true in every such call: a barrier then waits for the previous call's reads before the slots are
// rewritten.  Calls of different instantiations never share slots and need no such barrier.
constexpr int kReduceThreads = 256;
constexpr int kReduceWaves = kReduceThreads / 64;
// block_combine is the stage after the wave butterfly: v holds wave results (for values that were reduced per wave in narrower
// types of their own, as mask_edges_kernel's box); block_reduce is the butterfly followed by it.
template <class Op, bool Again = false, int NV, typename T>
__device__ __forceinline__ void block_combine(T (&v)[NV]) {
    __shared__ T sh[kReduceWaves * NV];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (Again) __syncthreads();                       // the previous call's reads of sh are done
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) sh[wid * NV + j] = v[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            T s = sh[j];
#pragma unroll
            for (int w = 1; w < kReduceWaves; ++w) s = Op::apply(s, sh[w * NV + j], j);
            v[j] = s;
        }
    }
}
template <class Op, bool Again = false, int NV, typename T>
__device__ __forceinline__ void block_reduce(T (&v)[NV]) {
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = wave_reduce<Op>(v[j], j);
    block_combine<Op, Again>(v);
}
template <int NV, typename T>
__device__ __forceinline__ void block_sum(T (&v)[NV]) { block_reduce<OpSum>(v); }
// one value, through one LDS slot per wave; with Again = true for a kernel that reduces many values one after the other
template <class Op, bool Again = false, typename T>
__device__ __forceinline__ T block_reduce_one(T v) {
    T a[1] = {v};
    block_reduce<Op, Again>(a);
    return a[0];
}

// First half of a finalize: thread t combines rows t, t + kReduceThreads, ... of part[nblk][NV] into acc, ascending.
template <class Op, int NV, typename T>
__device__ __forceinline__ void partials_reduce(const T* __restrict__ part, int nblk, T (&acc)[NV]) {
    for (int i = threadIdx.x; i < nblk; i += kReduceThreads) {
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j] = Op::apply(acc[j], part[(long long)i * NV + j], j);
    }
}

// The finalize without an epilogue: block r writes the NV sums of part[r][nblk][NV] to out[r][NV].
template <int NV, typename T>
__global__ __launch_bounds__(kReduceThreads) void sums_finalize_kernel(const T* __restrict__ part, int nblk, T* __restrict__ out) {
    T acc[NV] = {};
    partials_reduce<OpSum>(part + (long long)blockIdx.x * nblk * NV, nblk, acc);
    block_sum(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) out[(long long)blockIdx.x * NV + j] = acc[j];
    }
}
template <int NV, typename T>
static inline void launch_sums_finalize(const T* part, int nblk, T* out, hipStream_t st, unsigned rows = 1) {
    hipLaunchKernelGGL((sums_finalize_kernel<NV, T>), dim3(rows), dim3(kReduceThreads), 0, st, part, nblk, out);
}

// (mean, 1 / std) of n values from the fp64 sums of d = x - pivot and d^2; unbiased std
__device__ __forceinline__ void pivoted_mean_rstd(double pivot, double sum_d, double sum_d2, long long n, float& mean, float& rstd) {
    const double md = sum_d / (double)n, var = (sum_d2 - sum_d * md) / (double)(n - 1);
    mean = (float)(pivot + md);
    rstd = (float)(1.0 / sqrt(var));
}

}  // namespace seg
