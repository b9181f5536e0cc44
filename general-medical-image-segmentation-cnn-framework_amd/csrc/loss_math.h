// loss_math.h -- the per-element arithmetic that loss.hip and loss_tail.hip share.  The fused tail's backward promises the bits of
// the unfused criteria (loss_tail_bwd_kernel), so each expression has ONE definition.
#pragma once
#include <hip/hip_runtime.h>

namespace seg {

__device__ __forceinline__ float bce_term(float x, float t) {
    // max(x,0) - x*t + log1p(exp(-|x|))
    return fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
}

__device__ __forceinline__ float sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// torch.argmax's order: the first maximum in scan order wins and a NaN beats every number (the first NaN wins), as
// maxpool2_fwd_kernel (pool.hip) does for its window
__device__ __forceinline__ bool nan_first_gt(float v, float best) { return v > best || (v != v && best == best); }

}  // namespace seg
