/*
 * mi355seg.h -- C-ABI of libmi355seg.so: the MI355X (gfx950) hot path for 3D
 * segmentation training (U-Net family forward/backward + loss/Dice reductions).
 *
 * The reference (QingYunA/General-Medical-Image-Segmentation-CNN-Framework) has no
 * FFI: its seam for this path is torch.nn leaf modules.  Each entry point below names
 * the reference call it replaces (file:line under /root/reference) -- that is what a
 * ctypes binding on the reference side would bind.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless the name ends in _host;
 *   - activations are NDHWC fp32: element (n,d,h,w,c) of a tensor with channel pitch
 *     `ld` lives at ((((n*D+d)*H+h)*W+w)*ld + c); ld >= C lets a producer write into a
 *     channel slice of a wider (concat) buffer;
 *   - weights keep the PyTorch logical layouts: Conv3d (Cout,Cin,kD,kH,kW),
 *     ConvTranspose3d (Cin,Cout,kD,kH,kW), contiguous;
 *   - `stream` is a hipStream_t passed as void*; all work is stream-ordered, nothing
 *     synchronises, allocates or frees; scratch comes from the caller (`ws`), so the
 *     entry points may be called from several threads at once -- except the seven
 *     mi355seg_prepack_* ones, which share one per-process bracket (see there);
 *   - return value: 0 on success, a negative MI355SEG_E* code otherwise;
 *     mi355seg_last_error() returns a static message for the calling thread.
 */
#ifndef MI355SEG_H
#define MI355SEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 16-bit brain-float storage element of the *_bf16 entry points (same bits as torch.bfloat16).  The HIP compiler sees its
 * native __bf16, a plain C / C++ host compiler an opaque 16-bit integer: one ABI, one storage format. */
#if defined(__HIP__) || defined(__HIPCC__)
typedef __bf16 mi355seg_bf16;
#else
typedef uint16_t mi355seg_bf16;
#endif

#define MI355SEG_OK 0
#define MI355SEG_EINVAL (-1)   /* bad shape / unsupported argument combination */
#define MI355SEG_EWORKSPACE (-2) /* workspace too small */
#define MI355SEG_EHIP (-3)     /* a HIP launch failed */

/* activation codes for the norm/activation entry points */
#define MI355SEG_ACT_NONE 0
#define MI355SEG_ACT_RELU 1   /* nn.ReLU            (unet3d.py:89,101)            */
#define MI355SEG_ACT_ELU 2    /* nn.ELU(alpha=1)    (vnet3d.py:14-18)             */
#define MI355SEG_ACT_LRELU 3  /* nn.LeakyReLU(slope) (residual_unet3d.py:17)      */
#define MI355SEG_ACT_SIGMOID 4 /* torch.sigmoid       (RE_net.py:160, ER_net.py)    */

const char* mi355seg_last_error(void);
int mi355seg_version(void);

/* Arithmetic of the MFMA convolutions (k3 / k5 Conv3d forward, input gradient and weight gradient) on fp32 tensors.  The
 * reference's arithmetic for these is ATen fp32 (unet3d.py:80-98 through nn.Conv3d); both modes accumulate in fp32:
 *   FP32   -- v_mfma_f32_32x32x2_f32, exact fp32 products;
 *   BF16X6 -- every fp32 operand is split into three bf16 parts (x = h + m + l, 24 mantissa bits) and six
 *             v_mfma_f32_32x32x16_bf16 (hh, hm, mh, mm, hl, lh) form each product: fp32-level accuracy (the dropped
 *             terms are below 2^-23 of a product) at 2.7x the fp32 matrix rate;
 *   F16X3  -- every fp32 operand, scaled by a per-tensor power of two 2^s that places the tensor's largest magnitude in
 *             [2^14, 2^15), is split into two fp16 parts (v 2^s = h + l: 11 + 11 mantissa bits and the sign of l) and three
 *             v_mfma_f32_16x16x32_f16 (hh, hl, lh) form each product; the result is scaled back by 2^-(sx + sw).  The dropped
 *             l*l term is <= 2^-22 of a product (2^-24.6 rms); values more than 2^18 below their tensor's maximum keep an
 *             absolute error of 2^-40 of that maximum.  Same fp64-graded accuracy tests as BF16X6 at half its MFMA count.
 *             The maxima are measured on the device (one pass per tensor) unless the caller hands them over (*_amax entry
 *             points).  Covers the k3 s1 forward / input gradient / weight gradient; layers without that form run BF16X6;
 * (bf16 TENSORS have their own entry points, *_bf16: there the products are plain bf16 MFMAs.)
 * Process-wide, read at each launch.  Initial value: environment MI355SEG_CONV_MATH = fp32 | bf16x6 | f16x3, else the default. */
#define MI355SEG_MATH_FP32 0
#define MI355SEG_MATH_BF16X6 2
#define MI355SEG_MATH_F16X3 3
#define MI355SEG_MATH_DEFAULT MI355SEG_MATH_F16X3
int mi355seg_set_conv_math(int mode);
int mi355seg_get_conv_math(void);
/* MFMA shape of the BF16X6 forward / input-gradient kernels: 16 = v_mfma_f32_16x16x32_bf16 (conv_x3s.hip; the default: the
 * chip holds a higher clock under it, +8-12 % on the cfg-2 layers), 32 = v_mfma_f32_32x32x16_bf16 (the generic kernel).  Same six
 * products per fp32 product either way; layers the 16-wide tiles do not cover use 32 regardless.  Process-wide, read at each
 * launch.  Initial value: environment MI355SEG_X3_SHAPE = 16 | 32. */
int mi355seg_set_x3_shape(int shape);
int mi355seg_get_x3_shape(void);
/* Tiling of the k3 / k5 stride-1 convolutions on bf16 TENSORS (forward and input gradient): 0 = automatic (the
 * v_mfma_f32_16x16x32_bf16 kernel of conv_b16s.hip -- eight 16-voxel lines x 32 channels per wave -- where a layer cuts enough
 * tiles to fill the chip, the generic 32x32x16 tiles with split-K otherwise), 1 = conv_b16s.hip wherever its geometry applies,
 * 2 = the generic tiles only.  Process-wide, read at each launch (A/B timing, tests of both kernels on one shape). */
int mi355seg_set_b16_tiles(int mode);
int mi355seg_get_b16_tiles(void);
/* The f16x3 weight gradient of k3 s1 convolutions with Cout % 64 == 0 has a second kernel (conv_wgrad_f16w_kernel: four waves, one per
 * SIMD, a 32 x 64 channel block per workgroup -- half the LDS fragment reads per MFMA).  0: never, 1 (default): where the strip of
 * tiles per workgroup is long enough for it to pay, 2: wherever the geometry allows.  Same results contract either way. */
int mi355seg_set_wgrad_wide(int mode);
int mi355seg_get_wgrad_wide(void);

/* ------------------------------------------------------------------ Conv3d
 * Replaces nn.Conv3d forward/backward (ATen convolution / convolution_backward):
 * unet3d.py:80-98 (k3 s1 p1), :46-48 (k1 head); vnet3d.py:25,47,111 (k5 p2), :65 (k2 s2);
 * residual_unet3d.py:22-79 (k3 s1/s2 p1, k1, bias=False); unetr.py:134 (k16 s16).
 * Cubic kernel k, isotropic stride/pad.  Output extent Do = (D + 2*pad - k)/stride + 1.
 */
size_t mi355seg_conv3d_ws_bytes(int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad);

/* y = conv(x, w) + bias.  bias may be NULL.  If stats_sum/stats_sq are non-NULL they
 * receive, per output channel, sum(y) and sum(y*y) over all N*Do*Ho*Wo voxels as
 * doubles (the BatchNorm batch statistics, fused into the conv epilogue). */
int mi355seg_conv3d_fwd_f32(const float* x, int ldx, const float* w, const float* bias,
                            float* y, int ldy, int N, int D, int H, int W, int Cin, int Cout,
                            int k, int stride, int pad, double* stats_sum, double* stats_sq,
                            void* ws, size_t ws_bytes, void* stream);

/* F16X3 operand maxima.  The two-piece fp16 split needs an upper bound of max |.| of both operands of a convolution (a device
 * scalar each).  The plain entry points measure them (one pass over each operand per call); the *_ax forms take them from the
 * caller, who usually has them for free: mi355seg_norm_act_fwd_ax_f32 / mi355seg_norm_act_bwd_*_ax_f32 emit the maximum of the
 * tensor they write, a max-pool keeps its input's maximum, a parameter's maximum changes once per optimiser step
 * (mi355seg_amax_f32).  A bound above the true maximum by a factor 2^j costs j bits of headroom above the fp16 underflow; a
 * bound BELOW the true maximum by more than 2x overflows fp16 (non-finite results).  NULL = measure.  Ignored by the other maths.
 * mi355seg_conv_math_takes_amax() != 0 while the selected math uses them. */
int mi355seg_conv_math_takes_amax(void);
/* which passes of this layer read operand maxima under the selected math: bit 0 forward (x, w), bit 1 input gradient (dy, w),
 * bit 2 weight gradient (dy, x); 0 = none (hand nothing over, nothing is measured either) */
int mi355seg_conv3d_amax_use_f32(int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad);
int mi355seg_amax_f32(const float* x, int ld, long long rows, int C, float* amax /* max-combined into; zero it first */, void* stream);
int mi355seg_conv3d_fwd_ax_f32(const float* x, int ldx, const float* w, const float* bias,
                               float* y, int ldy, int N, int D, int H, int W, int Cin, int Cout,
                               int k, int stride, int pad, double* stats_sum, double* stats_sq, const float* x_amax, const float* w_amax,
                               void* ws, size_t ws_bytes, void* stream);
int mi355seg_conv3d_dgrad_ax_f32(const float* dy, int lddy, const float* w, float* dx, int lddx,
                                 int N, int D, int H, int W, int Cin, int Cout,
                                 int k, int stride, int pad, const float* dy_amax, const float* w_amax, void* ws, size_t ws_bytes, void* stream);
int mi355seg_conv3d_dgrad_bnsums_ax_f32(const float* dy, int lddy, const float* w, float* dx, int lddx,
                                        int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                                        const float* bn_x, int ld_bnx, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                        int act, float slope, float* s1, float* s2, float* dgamma, float* dbeta, const float* dy_amax, const float* w_amax,
                                        void* ws, size_t ws_bytes, void* stream);
int mi355seg_conv3d_wgrad_ax_f32(const float* dy, int lddy, const float* x, int ldx,
                                 float* dw, float* db, int N, int D, int H, int W, int Cin, int Cout,
                                 int k, int stride, int pad, int accumulate, const float* dy_amax, const float* x_amax,
                                 void* ws, size_t ws_bytes, void* stream);

/* Inference forward (predict.py:79-81,133: model.eval()): eval-mode BatchNorm and the activation that follows it folded into the
 * convolution -- y = act(conv(x, w) * oscale[co] + oshift[co]).  oscale is multiplied into the packed weights, oshift takes the
 * bias slot and the activation runs in the MFMA kernel's epilogue: no normalise pass over y.  mi355seg_bn_fold_f32 builds the two
 * vectors from the BatchNorm parameters, running statistics and the convolution's bias.  Matrix-core layers only: ask
 * *_fused_supported_* first (non-zero = yes) and keep convolution + norm_act_fwd for the other layers. */
int mi355seg_bn_fold_f32(const float* gamma, const float* beta, const float* mean, const float* var, const float* conv_bias,
                         float eps, int C, float* scale, float* shift, void* stream);
int mi355seg_conv3d_fused_supported_f32(int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad, int ldx, int ldy);
int mi355seg_conv3d_fwd_fused_f32(const float* x, int ldx, const float* w, const float* oscale, const float* oshift, int act, float slope,
                                  float* y, int ldy, int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                                  void* ws, size_t ws_bytes, void* stream);
int mi355seg_conv3d_fused_supported_bf16(int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad, int ldx, int ldy);
int mi355seg_conv3d_fwd_fused_bf16(const mi355seg_bf16* x, int ldx, const float* w, const float* oscale, const float* oshift, int act, float slope,
                                   mi355seg_bf16* y, int ldy, int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                                   void* ws, size_t ws_bytes, void* stream);

/* ---- conv2 of a double-conv block on conv1's RAW output (/root/reference/models/three_d/unet3d.py:80-101: conv1 -> norm1 -> relu1 ->
 * conv2): norm1 + relu1 run as a PROLOGUE of conv2's tile staging, in its forward and in its weight gradient, so the activation between
 * the two convolutions is never written or re-read.  f16x3 math, k3 s1 p1, act none / relu / leaky relu.
 *   mi355seg_conv3d_fwd_yamax_ax_f32   conv1's forward, also handing back max |y| (zeroed device scalar, max-combined into)
 *   mi355seg_norm_fold_f32             norm_stats_from_sums + the folded normalisation al = rstd gamma, be = beta - mean al (+ running
 *                                      statistics) + a_amax >= max |act(al x + be)| from x_amax = max |x|
 *   mi355seg_conv3d_fwd_pro_ax_f32     y = conv3d(act(pro_al[c] x + pro_be[c]), w) + bias (+ batch statistics of y); x_amax bounds the prologue's output
 *   mi355seg_conv3d_wgrad_pro_ax_f32   dw (+ db) of that convolution, the same prologue on its x operand
 * Same values as norm_act_fwd followed by the plain entry points (the prologue is the same fma + activation per element). */
int mi355seg_conv3d_pro_supported_f32(int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad, int act);
int mi355seg_conv3d_fwd_yamax_ax_f32(const float* x, int ldx, const float* w, const float* bias,
                                     float* y, int ldy, int N, int D, int H, int W, int Cin, int Cout,
                                     int k, int stride, int pad, double* stats_sum, double* stats_sq, const float* x_amax, const float* w_amax,
                                     float* y_amax, void* ws, size_t ws_bytes, void* stream);
int mi355seg_norm_fold_f32(const double* sum, const double* sq, long long rows, int C, float eps, const float* gamma, const float* beta, int act,
                           float* mean, float* rstd, float* running_mean, float* running_var, float momentum,
                           const float* x_amax, float* al, float* be, float* a_amax, void* stream);
int mi355seg_conv3d_fwd_pro_ax_f32(const float* x, int ldx, const float* pro_al, const float* pro_be, int pro_act, float pro_slope,
                                   const float* w, const float* bias, float* y, int ldy, int N, int D, int H, int W, int Cin, int Cout,
                                   int k, int stride, int pad, double* stats_sum, double* stats_sq, const float* x_amax, const float* w_amax,
                                   void* ws, size_t ws_bytes, void* stream);
int mi355seg_conv3d_wgrad_pro_ax_f32(const float* dy, int lddy, const float* x, int ldx, const float* pro_al, const float* pro_be, int pro_act, float pro_slope,
                                     float* dw, float* db, int N, int D, int H, int W, int Cin, int Cout,
                                     int k, int stride, int pad, int accumulate, const float* dy_amax, const float* x_amax,
                                     void* ws, size_t ws_bytes, void* stream);

/* The 1-channel stem of a double-conv block (/root/reference/models/three_d/unet3d.py:80-89: enc1conv1 -> enc1norm1 -> enc1relu1) when the block's
 * input needs no gradient: dw (+ db) of the stem straight from da = d(activation) and the pre-norm tensor y.  The norm backward's apply half
 * (dy = rstd gamma (dz - s1 / rows - xhat s2 / rows), dz = da act'(z); s1 / s2 = its column sums, e.g. from mi355seg_conv3d_dgrad_bnsums_f32) is
 * formed inside the weight-gradient kernel: the same values as mi355seg_norm_act_bwd_apply_f32 + mi355seg_conv3d_wgrad_f32 without writing dy. */
int mi355seg_stem_wgrad_bnbwd_supported_f32(int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad);
int mi355seg_stem_wgrad_bnbwd_f32(const float* da, int ldda, const float* y, int ldy, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                  int act, float slope, const float* s1, const float* s2, const float* x, int ldx, float* dw, float* db,
                                  int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad, void* ws, size_t ws_bytes, void* stream);

/* dx = conv_backward_input(dy, w).  D,H,W are the INPUT extents (of x/dx). */
int mi355seg_conv3d_dgrad_f32(const float* dy, int lddy, const float* w, float* dx, int lddx,
                              int N, int D, int H, int W, int Cin, int Cout,
                              int k, int stride, int pad, void* ws, size_t ws_bytes, void* stream);

/* The same input gradient for a convolution whose input was act(BatchNorm(bn_x)) of the layer in front (conv2 of a double-conv
 * block, unet3d.py:92-101 behind :80-89), plus the two column sums that layer's norm backward starts with: s1[c] = sum dz,
 * s2[c] = sum dz * xhat with dz = dx * act'(z) (dgamma = s2, dbeta = s1; may be NULL).  On the bf16x6 k3 path the sums come out of
 * the input-gradient kernel's epilogue (one read of bn_x, no pass over dx); elsewhere this is conv3d_dgrad followed by
 * norm_act_bwd_sums.  Finish the layer in front with mi355seg_norm_act_bwd_apply_f32.  ws: max(conv3d_ws_bytes, norm_ws_bytes). */
int mi355seg_conv3d_dgrad_bnsums_f32(const float* dy, int lddy, const float* w, float* dx, int lddx,
                                     int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                                     const float* bn_x, int ld_bnx, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                     int act, float slope, float* s1, float* s2, float* dgamma, float* dbeta,
                                     void* ws, size_t ws_bytes, void* stream);

/* dw (Cout,Cin,k,k,k) and db (Cout, may be NULL) = conv_backward_weight(dy, x).
 * Deterministic (two-stage reduction, no atomics).  accumulate!=0 adds into dw/db
 * (weight sharing, residual_unet3d.py:126,128). */
int mi355seg_conv3d_wgrad_f32(const float* dy, int lddy, const float* x, int ldx,
                              float* dw, float* db, int N, int D, int H, int W, int Cin, int Cout,
                              int k, int stride, int pad, int accumulate,
                              void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ ConvTranspose3d k2 s2
 * Replaces nn.ConvTranspose3d(kernel_size=2, stride=2): unet3d.py:29-43, vnet3d.py:86,
 * unetr.py:11.  x is [N,D,H,W,Cin]; y is [N,2D,2H,2W,Cout]; w is (Cin,Cout,2,2,2).
 */
size_t mi355seg_convt3d_k2s2_ws_bytes(int N, int D, int H, int W, int Cin, int Cout);
int mi355seg_convt3d_k2s2_fwd_f32(const float* x, int ldx, const float* w, const float* bias,
                                  float* y, int ldy, int N, int D, int H, int W, int Cin, int Cout,
                                  void* ws, size_t ws_bytes, void* stream);
/* the same with max |y| as a by-product (F16X3 operand maxima: the up-convolution half of a decoder's concat buffer) */
int mi355seg_convt3d_k2s2_fwd_ax_f32(const float* x, int ldx, const float* w, const float* bias,
                                  float* y, int ldy, int N, int D, int H, int W, int Cin, int Cout,
                                  float* y_amax,
                                     void* ws, size_t ws_bytes, void* stream);
int mi355seg_convt3d_k2s2_dgrad_f32(const float* dy, int lddy, const float* w, float* dx, int lddx,
                                    int N, int D, int H, int W, int Cin, int Cout,
                                    void* ws, size_t ws_bytes, void* stream);
int mi355seg_convt3d_k2s2_wgrad_f32(const float* dy, int lddy, const float* x, int ldx,
                                    float* dw, float* db, int N, int D, int H, int W, int Cin, int Cout,
                                    void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ which branch ran
 * Every fp32 Conv3d / ConvTranspose3d k2 s2 dispatcher (mi355seg_conv3d_{fwd,dgrad,wgrad}[_ax|_pro_ax|_yamax_ax]_f32,
 * mi355seg_conv3d_fwd_fused_f32, mi355seg_conv3d_dgrad_bnsums[_ax]_f32, mi355seg_convt3d_k2s2_{fwd,dgrad,wgrad}[_ax]_f32) records the branch of its if-chain it took in one host-side integer before it
 * launches: a test asks after the call and so knows which kernel it has graded (tests/test_gpu_conv_paths.py).  One code per
 * branch; a branch that chooses between kernels has one per kernel.  Process-wide like the conv math, not thread-local;
 * mi355seg_stem_wgrad_bnbwd_f32 (one kernel, no choice) does not record.  0 before the first call.
 * The bf16-storage entry points (mi355seg_conv3d_{fwd,fwd_fused,fwd_res,dgrad,dgrad_res,wgrad}_bf16,
 * mi355seg_convt3d_k2s2_{fwd,fwd_ax,dgrad,wgrad}_bf16) record MI355SEG_PATH_B16_* codes (tests/test_gpu_bf16_paths.py): the family
 * their ladder chose (a demoted call reports the family it was demoted to), inside the igemm / gather / transposing-read families
 * the tiles and the K form.  After the cast fall-back the code is *_CAST, not the branch the fp32 entry point took on the staged
 * copies (it is stored after that call returns). */
enum {
    MI355SEG_PATH_NONE = 0,
    /* mi355seg_conv3d_fwd*_f32 */
    MI355SEG_PATH_FWD_MFMA_X3S = 1,          /* split-precision igemm, 16x16x32 tiles (conv_x3s.hip) */
    MI355SEG_PATH_FWD_MFMA_X3 = 2,           /* split-precision igemm, generic 32x32x16 tiles */
    MI355SEG_PATH_FWD_MFMA_F32 = 3,          /* fp32 MFMA igemm */
    MI355SEG_PATH_FWD_PATCH_EMBED = 4,       /* kernel = stride as one GEMM */
    MI355SEG_PATH_FWD_GATHER = 5,            /* gather igemm (strided / even kernels) */
    MI355SEG_PATH_FWD_HEADK = 6,             /* z-marching head, Cout = 2 */
    MI355SEG_PATH_FWD_STEMK = 7,             /* z-marching k5 stem, Cin = 1 | 2 */
    MI355SEG_PATH_FWD_STEM_TILED_STATS = 8,  /* k3 stem, LDS-tiled 1-channel kernel with in-kernel statistics */
    MI355SEG_PATH_FWD_STEM_TILED = 9,        /* k3 stem, LDS-tiled 1-channel kernel */
    MI355SEG_PATH_FWD_STEM_C1 = 10,          /* k3 stem, direct kernel, Cin = 1 */
    MI355SEG_PATH_FWD_STEM_C2 = 11,
    MI355SEG_PATH_FWD_STEM_C4 = 12,
    MI355SEG_PATH_FWD_TINYPW = 13,           /* k1, at most 4 channels on either side */
    MI355SEG_PATH_FWD_HEAD = 14,             /* k1 head, Cout = 2 | 4 */
    MI355SEG_PATH_FWD_GENERIC = 15,
    MI355SEG_PATH_FWD_PRO_X3S = 16,          /* mi355seg_conv3d_fwd_pro_ax_f32 */
    /* mi355seg_conv3d_dgrad*_f32 */
    MI355SEG_PATH_DGRAD_MFMA_X3S = 20,
    MI355SEG_PATH_DGRAD_MFMA_X3 = 21,
    MI355SEG_PATH_DGRAD_MFMA_F32 = 22,
    MI355SEG_PATH_DGRAD_GATHER = 23,
    MI355SEG_PATH_DGRAD_HEADK = 24,
    MI355SEG_PATH_DGRAD_HEAD = 25,
    MI355SEG_PATH_DGRAD_TINYPW = 26,
    MI355SEG_PATH_DGRAD_K2S2_CONVT = 27,     /* k2 s2 p0 as the forward of ConvTranspose3d k2 s2 */
    MI355SEG_PATH_DGRAD_GENERIC = 28,
    /* mi355seg_conv3d_wgrad*_f32 */
    MI355SEG_PATH_WGRAD_PATCH_EMBED = 40,
    MI355SEG_PATH_WGRAD_LOWP_WIDE = 41,      /* conv_wgrad_lowp, 32 x 64 channel blocks */
    MI355SEG_PATH_WGRAD_LOWP_SWAPPED = 42,   /* conv_wgrad_lowp, the wide kernel with the operands' roles swapped */
    MI355SEG_PATH_WGRAD_LOWP_NARROW = 43,    /* conv_wgrad_lowp, 32 x 32 channel blocks */
    MI355SEG_PATH_WGRAD_MFMA = 44,           /* fp32 MFMA, k3 / k5 s1 */
    MI355SEG_PATH_WGRAD_PW_LOWP = 45,        /* k1, split-precision planes */
    MI355SEG_PATH_WGRAD_PW_MFMA = 46,        /* k1, fp32 MFMA */
    MI355SEG_PATH_WGRAD_TINYPW = 47,
    MI355SEG_PATH_WGRAD_STEM_TILED = 48,     /* k3 stem, LDS-tiled 1-channel kernel */
    MI355SEG_PATH_WGRAD_STEM_C4 = 49,        /* k3 stem, stem4_wgrad_kernel */
    MI355SEG_PATH_WGRAD_STEM = 50,           /* k3 stem, direct kernel */
    MI355SEG_PATH_WGRAD_HEAD = 51,
    MI355SEG_PATH_WGRAD_HEADK = 52,
    MI355SEG_PATH_WGRAD_SMALLCIN_K5_TILED = 53,
    MI355SEG_PATH_WGRAD_SMALLCIN = 54,
    MI355SEG_PATH_WGRAD_SMALLCOUT = 55,
    MI355SEG_PATH_WGRAD_GWGRAD = 56,         /* MFMA gather weight gradient */
    MI355SEG_PATH_WGRAD_GENERIC = 57,
    /* mi355seg_convt3d_k2s2_*_f32 */
    MI355SEG_PATH_CONVT_FWD_DIRECT = 60,
    MI355SEG_PATH_CONVT_FWD_MFMA = 61,
    MI355SEG_PATH_CONVT_FWD_PLAIN = 62,
    MI355SEG_PATH_CONVT_DGRAD_DIRECT = 63,
    MI355SEG_PATH_CONVT_DGRAD_MFMA = 64,
    MI355SEG_PATH_CONVT_DGRAD_PLAIN = 65,
    MI355SEG_PATH_CONVT_WGRAD_LOWP = 66,
    MI355SEG_PATH_CONVT_WGRAD_MFMA = 67,
    MI355SEG_PATH_CONVT_WGRAD_PLAIN = 68,
    /* mi355seg_conv3d_fwd[_fused|_res]_bf16 */
    MI355SEG_PATH_B16_FWD_IGEMM_S = 100,         /* igemm, 16x16x32 tiles (conv_b16s.hip), whole K */
    MI355SEG_PATH_B16_FWD_IGEMM_S_SPLITK = 101,  /* ... fp32 slabs + splitk_reduce_kernel */
    MI355SEG_PATH_B16_FWD_IGEMM_G = 102,         /* igemm, generic 32x32x16 tiles, whole K */
    MI355SEG_PATH_B16_FWD_IGEMM_G_SPLITK = 103,
    MI355SEG_PATH_B16_FWD_GATHER = 104,          /* gather igemm, whole K */
    MI355SEG_PATH_B16_FWD_GATHER_SPLITK = 105,
    MI355SEG_PATH_B16_FWD_HEAD2 = 106,           /* k5 head, Cout = 2 (conv_head2_lowp.hip) */
    MI355SEG_PATH_B16_FWD_STEM1K5 = 107,         /* k5 stem, Cin = 1 (conv_stem1k5_lowp.hip) */
    MI355SEG_PATH_B16_FWD_STEM4 = 108,           /* k3 stem, Cin = 4 on the matrix cores (conv_stem4_lowp.hip) */
    MI355SEG_PATH_B16_FWD_STEM = 109,            /* k3 stem, direct kernels */
    MI355SEG_PATH_B16_FWD_HEADPW = 110,          /* k1 head on the matrix cores (conv_headpw_lowp.hip) */
    MI355SEG_PATH_B16_FWD_HEAD = 111,            /* k1 head, plain kernel */
    MI355SEG_PATH_B16_FWD_TINYPW = 112,
    MI355SEG_PATH_B16_FWD_CAST = 113,            /* fp32 copies staged in the workspace, the fp32 entry point on them */
    /* mi355seg_conv3d_dgrad[_res]_bf16 */
    MI355SEG_PATH_B16_DGRAD_IGEMM_S = 120,
    MI355SEG_PATH_B16_DGRAD_IGEMM_S_SPLITK = 121,
    MI355SEG_PATH_B16_DGRAD_IGEMM_G = 122,
    MI355SEG_PATH_B16_DGRAD_IGEMM_G_SPLITK = 123,
    MI355SEG_PATH_B16_DGRAD_GATHER_PHASES = 124, /* gather igemm, every phase in one launch */
    MI355SEG_PATH_B16_DGRAD_GATHER = 125,        /* gather igemm, one launch per phase */
    MI355SEG_PATH_B16_DGRAD_HEAD2 = 126,
    MI355SEG_PATH_B16_DGRAD_HEAD = 127,
    MI355SEG_PATH_B16_DGRAD_TINYPW = 128,
    MI355SEG_PATH_B16_DGRAD_K2S2_CONVT = 129,    /* k2 s2 p0 as the forward of ConvTranspose3d k2 s2 (igemm) */
    MI355SEG_PATH_B16_DGRAD_CAST = 130,
    /* mi355seg_conv3d_wgrad_bf16 */
    MI355SEG_PATH_B16_WGRAD_LOWP_NARROW = 140,   /* conv_wgrad_lowp, 32 x 32 channel blocks */
    MI355SEG_PATH_B16_WGRAD_LOWP_WIDE = 141,     /* conv_wgrad_lowp, 32 x 64 channel blocks */
    MI355SEG_PATH_B16_WGRAD_LOWP_SWAPPED = 142,  /* (the swapped-role form exists on fp32 tensors only: never recorded) */
    MI355SEG_PATH_B16_WGRAD_HEAD2 = 143,
    MI355SEG_PATH_B16_WGRAD_STEM1K5 = 144,
    MI355SEG_PATH_B16_WGRAD_K2S2_CONVT = 145,    /* k2 s2 p0 as a ConvTranspose3d k2 s2 weight gradient with the roles swapped */
    MI355SEG_PATH_B16_WGRAD_TINYPW = 146,
    MI355SEG_PATH_B16_WGRAD_PW_LOWP = 147,       /* k1 on the bf16 matrix cores */
    MI355SEG_PATH_B16_WGRAD_PW_MFMA = 148,       /* k1, bf16 loads, fp32 MFMA */
    MI355SEG_PATH_B16_WGRAD_STEM4 = 149,
    MI355SEG_PATH_B16_WGRAD_STEM = 150,
    MI355SEG_PATH_B16_WGRAD_HEADPW = 151,
    MI355SEG_PATH_B16_WGRAD_HEAD = 152,
    MI355SEG_PATH_B16_WGRAD_SMALLCIN = 153,
    MI355SEG_PATH_B16_WGRAD_SMALLCOUT = 154,
    MI355SEG_PATH_B16_WGRAD_GWGRAD = 155,        /* MFMA gather weight gradient */
    MI355SEG_PATH_B16_WGRAD_CAST = 156,
    /* mi355seg_convt3d_k2s2_*_bf16: the fp32 codes + 100, and the streaming form of the direct kernels */
    MI355SEG_PATH_B16_CONVT_FWD_DIRECT = 160,    /* convt_direct, GEMM form */
    MI355SEG_PATH_B16_CONVT_FWD_MFMA = 161,
    MI355SEG_PATH_B16_CONVT_FWD_PLAIN = 162,
    MI355SEG_PATH_B16_CONVT_DGRAD_DIRECT = 163,
    MI355SEG_PATH_B16_CONVT_DGRAD_MFMA = 164,
    MI355SEG_PATH_B16_CONVT_DGRAD_PLAIN = 165,
    MI355SEG_PATH_B16_CONVT_WGRAD_LOWP = 166,
    MI355SEG_PATH_B16_CONVT_WGRAD_MFMA = 167,
    MI355SEG_PATH_B16_CONVT_WGRAD_PLAIN = 168,
    MI355SEG_PATH_B16_CONVT_FWD_STREAM = 169,    /* convt_direct, streaming form (K = 64 | 128 | 256, whole 32-voxel tiles) */
    MI355SEG_PATH_B16_CONVT_DGRAD_STREAM = 170
};
int mi355seg_last_conv_path(void);

/* ------------------------------------------------------------------ Batch / Instance norm
 * Replaces nn.BatchNorm3d in training mode (native_batch_norm, unet3d.py:88,100;
 * vnet3d.py:27,49,66,88,112) and nn.InstanceNorm3d (residual_unet3d.py:27..106), fused
 * with the activation that follows it and an optional residual add in front of the
 * activation (vnet3d.py:57-58,79,103).
 * rows = voxels per statistics group, groups = 1 (BatchNorm: rows = N*D*H*W) or N
 * (InstanceNorm: rows = D*H*W).  mean/rstd are [groups*C] floats.
 */
size_t mi355seg_norm_ws_bytes(long long rows, int groups, int C);

/* Batch statistics of x: mean and rstd = 1/sqrt(var_biased + eps).  If running_mean /
 * running_var are non-NULL (groups must be 1) they are updated in place with
 * `momentum`, running_var with the UNBIASED variance (PyTorch semantics). */
int mi355seg_norm_stats_f32(const float* x, int ldx, long long rows, int groups, int C, float eps,
                            float* mean, float* rstd, float* running_mean, float* running_var,
                            float momentum, void* ws, size_t ws_bytes, void* stream);

/* Same, but from per-channel sum / sum-of-squares (as produced by the conv epilogue). */
int mi355seg_norm_stats_from_sums_f32(const double* sum, const double* sq, long long rows, int C, float eps,
                                      float* mean, float* rstd, float* running_mean, float* running_var,
                                      float momentum, void* stream);

/* y = act( (x-mean)*rstd*gamma + beta  [+ res] ).  gamma/beta/res may be NULL. */
int mi355seg_norm_act_fwd_f32(const float* x, int ldx, const float* mean, const float* rstd,
                              const float* gamma, const float* beta, const float* res, int ldres,
                              float* y, int ldy, long long rows, int groups, int C,
                              int act, float slope, void* stream);

/* Backward of the above.  Inputs: dy (grad of the activation output), x (the norm
 * input).  Outputs: dx; dgamma/dbeta [C] (NULL when the norm has no affine); dres (grad
 * of the residual = grad at the activation input; NULL if no residual). */
int mi355seg_norm_act_bwd_f32(const float* dy, int lddy, const float* x, int ldx,
                              const float* mean, const float* rstd, const float* gamma, const float* beta,
                              const float* res, int ldres,
                              float* dx, int lddx, float* dgamma, float* dbeta, float* dres, int lddres,
                              long long rows, int groups, int C, int act, float slope,
                              void* ws, size_t ws_bytes, void* stream);

/* Same, and additionally dx_colsum[c] = sum over rows of dx[r, c] (groups == 1): when the norm follows a
 * convolution that is exactly the convolution's bias gradient, so the separate reduction pass over dy is saved. */
int mi355seg_norm_act_bwd_colsum_f32(const float* dy, int lddy, const float* x, int ldx,
                                     const float* mean, const float* rstd, const float* gamma, const float* beta,
                                     const float* res, int ldres,
                                     float* dx, int lddx, float* dgamma, float* dbeta, float* dres, int lddres, float* dx_colsum,
                                     long long rows, int groups, int C, int act, float slope,
                                     void* ws, size_t ws_bytes, void* stream);

/* BatchNorm + activation of the LAST double-conv block fused with the 1x1x1 output head (/root/reference/models/three_d/unet3d.py:46-48,
 * 68-71: ``self.conv(dec1)`` behind decoder1's norm2 (:100) + relu2 (:101); head = nn.Conv3d(features, out_channels, kernel_size=1)).
 * The activation a = act(BN(y)) has the head as its only consumer and is never written:
 *   fwd        logits[r, k] = bh[k] + sum_c wh[k, c] * act(gamma[c] * xhat[r, c] + beta[c])          (same bits as norm_act_fwd + conv3d_fwd k1)
 *   bwd_sums   one pass over (y, dlogits): s1 / s2 of the norm backward (dz = (sum_k dlogits[r, k] wh[k, c]) * act'(z)), dgamma = s2,
 *              dbeta = s1, AND the head's gradients dwh[k, c] = sum_r dlogits[r, k] a[r, c], dbh[k] = sum_r dlogits[r, k]
 *   bwd_apply  dy = rstd gamma (dz - s1 / rows - xhat s2 / rows), dy_colsum[c] = sum_r dy (bias gradient of the convolution in front),
 *              dy_amax (f16x3 operand maximum; max-combined into a zeroed scalar).  C a power of two in 4..256, K = 1..4, fp32.
 * ws: mi355seg_bn_act_head_ws_bytes(C, K). */
int mi355seg_bn_act_head_supported_f32(long long rows, int C, int K, int ldy);
size_t mi355seg_bn_act_head_ws_bytes(int C, int K);
int mi355seg_bn_act_head_fwd_f32(const float* y, int ldy, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                 int act, float slope, const float* wh, const float* bh, float* logits, int ldl,
                                 long long rows, int C, int K, void* stream);
int mi355seg_bn_act_head_bwd_sums_f32(const float* dlogits, int lddl, const float* y, int ldy, const float* mean, const float* rstd,
                                      const float* gamma, const float* beta, int act, float slope, const float* wh,
                                      float* s1, float* s2, float* dgamma, float* dbeta, float* dwh, float* dbh,
                                      long long rows, int C, int K, void* ws, size_t ws_bytes, void* stream);
int mi355seg_bn_act_head_bwd_apply_f32(const float* dlogits, int lddl, const float* y, int ldy, const float* mean, const float* rstd,
                                       const float* gamma, const float* beta, int act, float slope, const float* wh,
                                       const float* s1, const float* s2, float* dy, int lddy, float* dy_colsum, float* dy_amax,
                                       long long rows, int C, int K, void* ws, size_t ws_bytes, void* stream);

/* BatchNorm + activation of an ENCODER block fused with the MaxPool3d(2, 2) behind it (/root/reference/models/three_d/unet3d.py:19-25,
 * 51-58: ``self.pool1(enc1)`` with enc1 = relu2(norm2(.)) also kept for the skip concatenation :59-68).  fwd: one kernel writes the
 * activation a (pitch lda: a channel slice of the level's concat buffer), the pooled tensor [N, D/2, H/2, W/2, C] and the 3-bit argmax
 * codes (nn.MaxPool3d's first-maximum / NaN rule), + max |a| into a zeroed scalar (may be NULL).  bwd: the norm backward with
 * d(a) = dskip + maxpool_backward(dpooled, idx) formed on the fly -- no pool-backward pass, no d(a) tensor: s1 / s2 (dgamma = s2,
 * dbeta = s1; may be NULL), dy, dy_colsum (may be NULL), dy_amax (may be NULL).  D, H, W even, C a power of two in 4..256, fp32. */
int mi355seg_bn_act_pool_supported_f32(int N, int D, int H, int W, int C, int ldy);
size_t mi355seg_bn_act_pool_ws_bytes(int C);
int mi355seg_bn_act_pool_fwd_f32(const float* y, int ldy, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                 int act, float slope, float* a, int lda, float* pooled, unsigned char* idx, float* a_amax,
                                 int N, int D, int H, int W, int C, void* stream);
int mi355seg_bn_act_pool_bwd_f32(const float* dskip, int ldds, const float* dpooled, const unsigned char* idx, const float* y, int ldy,
                                 const float* mean, const float* rstd, const float* gamma, const float* beta, int act, float slope,
                                 float* s1, float* s2, float* dgamma, float* dbeta, float* dy, int lddy, float* dy_colsum, float* dy_amax,
                                 int N, int D, int H, int W, int C, void* ws, size_t ws_bytes, void* stream);

/* The same backward in its two halves (the conv -> BN -> ReLU -> conv chains of unet3d.py:73-104: the first half can ride in the
 * epilogue of the kernel that produces dy, see mi355seg_conv3d_dgrad_bnsums_f32):
 *   sums:  s1[g, c] = sum_rows dz, s2[g, c] = sum_rows dz * xhat, dz = dy * act'(z)  (+ dgamma = s2, dbeta = s1; groups == 1)
 *   apply: dx = rstd * gamma * (dz - s1 / rows - xhat * s2 / rows)  (+ dres = dz; + dx_colsum[c] = sum_rows dx[r, c]) */
int mi355seg_norm_act_bwd_sums_f32(const float* dy, int lddy, const float* x, int ldx,
                                   const float* mean, const float* rstd, const float* gamma, const float* beta,
                                   const float* res, int ldres, float* s1, float* s2, float* dgamma, float* dbeta,
                                   long long rows, int groups, int C, int act, float slope,
                                   void* ws, size_t ws_bytes, void* stream);
int mi355seg_norm_act_bwd_apply_f32(const float* dy, int lddy, const float* x, int ldx,
                                    const float* mean, const float* rstd, const float* gamma, const float* beta,
                                    const float* res, int ldres, const float* s1, const float* s2,
                                    float* dx, int lddx, float* dres, int lddres, float* dx_colsum,
                                    long long rows, int groups, int C, int act, float slope,
                                    void* ws, size_t ws_bytes, void* stream);

/* The same three with the maximum magnitude of the tensor they WRITE as a by-product (F16X3 operand maxima, see
 * mi355seg_conv3d_fwd_ax_f32): max |y| resp. max |dx| is max-combined into the device scalar the last pointer names (zeroed by the
 * caller; NULL = not wanted).  One compare per element in kernels that are HBM-bound, one atomic max per workgroup. */
int mi355seg_norm_act_fwd_ax_f32(const float* x, int ldx, const float* mean, const float* rstd,
                                 const float* gamma, const float* beta, const float* res, int ldres,
                                 float* y, int ldy, long long rows, int groups, int C,
                                 int act, float slope, float* y_amax, void* stream);
int mi355seg_norm_act_bwd_colsum_ax_f32(const float* dy, int lddy, const float* x, int ldx,
                                        const float* mean, const float* rstd, const float* gamma, const float* beta,
                                        const float* res, int ldres,
                                        float* dx, int lddx, float* dgamma, float* dbeta, float* dres, int lddres, float* dx_colsum, float* dx_amax,
                                        long long rows, int groups, int C, int act, float slope,
                                        void* ws, size_t ws_bytes, void* stream);
int mi355seg_norm_act_bwd_apply_ax_f32(const float* dy, int lddy, const float* x, int ldx,
                                       const float* mean, const float* rstd, const float* gamma, const float* beta,
                                       const float* res, int ldres, const float* s1, const float* s2,
                                       float* dx, int lddx, float* dres, int lddres, float* dx_colsum, float* dx_amax,
                                       long long rows, int groups, int C, int act, float slope,
                                       void* ws, size_t ws_bytes, void* stream);

/* Eval-mode BatchNorm (running stats) is norm_act_fwd with mean=running_mean and
 * rstd = 1/sqrt(running_var+eps) computed by: */
int mi355seg_rstd_from_var_f32(const float* var, float eps, float* rstd, int C, void* stream);

/* Stand-alone activation (residual_unet3d.py:112,116 LeakyReLU; vnet ELU): y = act(x [+ res]) */
/* dx = addend + dy * act'(x + res) (r5): an activation's backward together with the sum of a SECOND gradient of the same tensor -- the
 * residual forks of /root/reference/models/three_d/residual_unet3d.py:110-121 (the level's tensor feeds a LeakyReLU and, unchanged, the
 * block sum): one pass instead of the activation backward and autograd's add.  addend NULL: mi355seg_act_bwd. */
int mi355seg_act_bwd_add_f32(const float* dy, int lddy, const float* x, int ldx, const float* res, int ldres, const float* addend, int ldadd,
                             float* dx, int lddx, long long rows, int C, int act, float slope, void* stream);
int mi355seg_act_fwd_f32(const float* x, int ldx, const float* res, int ldres, float* y, int ldy,
                         long long rows, int C, int act, float slope, void* stream);
/* dx = dy * act'(x [+ res]) */
int mi355seg_act_bwd_f32(const float* dy, int lddy, const float* x, int ldx, const float* res, int ldres,
                         float* dx, int lddx, long long rows, int C, int act, float slope, void* stream);

/* nn.PReLU(C) -- V-Net's elu=False branch (vnet3d.py:14-18): y = max(z, 0) + slope[c] * min(z, 0), z = x [+ res].
 * Backward: dx = dy * (z > 0 ? 1 : slope[c]); dslope[c] = sum over rows of dy * min(z, 0) (two-stage, deterministic).
 * ws for the backward: mi355seg_norm_ws_bytes(rows, 1, C). */
int mi355seg_prelu_fwd_f32(const float* x, int ldx, const float* res, int ldres, const float* slope, float* y, int ldy,
                           long long rows, int C, void* stream);
int mi355seg_prelu_bwd_f32(const float* dy, int lddy, const float* x, int ldx, const float* res, int ldres, const float* slope,
                           float* dx, int lddx, float* dslope, long long rows, int C, void* ws, size_t ws_bytes, void* stream);

/* nn.Dropout3d (vnet3d.py:90,99; residual_unet3d.py:18): y[r,c] = x[r,c] * scale[g*C + c], the per-(sample,
 * channel) keep-mask / (1-p) being supplied by the caller (device RNG in production, the oracle's mask in
 * parity tests).  The backward is the same call on dy. */
int mi355seg_scale_channels_f32(const float* x, int ldx, const float* scale, float* y, int ldy,
                                long long rows, int groups, int C, void* stream);

/* ------------------------------------------------------------------ Pool / upsample
 * nn.MaxPool3d(2,2) (unet3d.py:19-25): y [N,D/2,H/2,W/2,C]; idx = 3-bit argmax code
 * (dz*4+dy*2+dx of the first maximum in PyTorch scan order) per output element. */
int mi355seg_maxpool2_fwd_f32(const float* x, int ldx, float* y, int ldy, uint8_t* idx,
                              int N, int D, int H, int W, int C, void* stream);
int mi355seg_maxpool2_bwd_f32(const float* dy, int lddy, const uint8_t* idx, float* dx, int lddx,
                              int N, int D, int H, int W, int C, void* stream);
/* dx = maxpool_backward(dy) + add: the encoder activation feeds both the pool and the skip connection
 * (unet3d.py:51-54,59-68); this folds autograd's gradient accumulation of the two branches into the pool backward. */
int mi355seg_maxpool2_bwd_add_f32(const float* dy, int lddy, const uint8_t* idx, const float* add, int ldadd, float* dx, int lddx,
                                  int N, int D, int H, int W, int C, void* stream);
/* nn.Upsample(scale_factor=2, mode='nearest') (residual_unet3d.py:19,103) */
int mi355seg_upsample2_fwd_f32(const float* x, int ldx, float* y, int ldy,
                               int N, int D, int H, int W, int C, void* stream);
int mi355seg_upsample2_bwd_f32(const float* dy, int lddy, float* dx, int lddx,
                               int N, int D, int H, int W, int C, void* stream);

/* ------------------------------------------------------------------ Loss / argmax / Dice
 * All take NCDHW-contiguous logits/targets [N,K,S] (S = D*H*W), as train.py hands them.
 */
size_t mi355seg_loss_ws_bytes(long long numel);

/* nn.BCEWithLogitsLoss() mean (train.py:115,209; loss_function.py:19-41):
 * loss[0] = mean( max(x,0) - x*t + log1p(exp(-|x|)) ). */
int mi355seg_bce_logits_fwd_f32(const float* logits, const float* target, long long numel,
                                float* loss, void* ws, size_t ws_bytes, void* stream);
/* dlogits = (sigmoid(x) - t) * gscale[0] / numel   (gscale = upstream grad, device scalar) */
int mi355seg_bce_logits_bwd_f32(const float* logits, const float* target, const float* gscale,
                                long long numel, float* dlogits, void* stream);

/* pred.argmax(dim=1, keepdim=True) (train.py:204, predict.py:139): first max wins, a NaN beats every number and the first NaN
 * wins (torch.argmax's order; mi355seg_bce_argmax_dice_f32 follows it for both of its argmaxes); int64 out [N,1,S] */
int mi355seg_argmax_ch_f32(const float* logits, long long N, int K, long long S, int64_t* mask, void* stream);

/* Integer counters of utils/metric.py:34-43 on two int64 label volumes:
 * counts[0]=sum(gt) counts[1]=sum(pred) counts[2]=nnz(gt&pred) counts[3]=nnz(gt|pred). */
int mi355seg_dice_counts_i64(const int64_t* gt, const int64_t* pred, long long numel,
                             int64_t* counts, void* ws, size_t ws_bytes, void* stream);

/* The predict-time metrics beside Dice: metric(gt_t, pred_t, spacing) of predict.py:154 (utils/metric.py:29-32,45-59,72-73).
 * All volumes are int64 label volumes [D,H,W]; foreground is != 0.
 *
 * counts[0..3] as mi355seg_dice_counts_i64; counts[4..7] = tp, fp, fn, tn of utils/metric.py:45-55: VALUE sums of gdth & pred,
 * of pred where pred - gdth >= 1, of gdth where gdth - pred >= 1, and of 1 - (gdth | pred).
 * ws: mi355seg_confusion_counts_ws_bytes(numel). */
size_t mi355seg_confusion_counts_ws_bytes(long long numel);
int mi355seg_confusion_counts_i64(const int64_t* gt, const int64_t* pred, long long numel,
                                  int64_t* counts, void* ws, size_t ws_bytes, void* stream);

/* Surface voxels of both masks in one pass (the get_mask_edges step of monai's compute_hausdorff_distance, utils/metric.py:32):
 * a foreground voxel is an edge voxel when one of its six face neighbours is background; outside the array is background.
 * edges: uint8 [2][D][H][W] (0 = gt, 1 = pred).  info: int64[8] = edge voxels of gt, of pred, then the bounding box of both edge
 * sets together, lo z, y, x and hi z, y, x (hi exclusive); with no edge voxel at all lo = (D, H, W) and hi = 0. */
int mi355seg_mask_edges_i64(const int64_t* gt, const int64_t* pred, int D, int H, int W, uint8_t* edges, int64_t* info, void* stream);

/* Exact Euclidean distance transform with voxel spacing (sz, sy, sx), the distance_transform_edt step of the same call, for both
 * edge maps at once, restricted to the box [z0, z0+bd) x [y0, y0+bh) x [x0, x0+bw) of the volume (every site must lie inside it):
 * dt2[m][z][y][x] (fp64, box-relative, [2][bd][bh][bw]) = min over the sites s of sites[m] of (sz*dz)^2 + (sy*dy)^2 + (sx*dx)^2,
 * the SQUARED distance; +inf where sites[m] is empty.  sites: uint8 [2][D][H][W] as mi355seg_mask_edges_i64 writes it.
 * ws: mi355seg_edt3d_ws_bytes(bd, bh, bw). */
size_t mi355seg_edt3d_ws_bytes(int bd, int bh, int bw);
int mi355seg_edt3d_f64(const uint8_t* sites, int D, int H, int W, int z0, int y0, int x0, int bd, int bh, int bw,
                       double sz, double sy, double sx, double* dt2, void* ws, size_t ws_bytes, void* stream);

/* The two directed surface-distance sets of the same call: dist[0][0..n_gt) = sqrt(dt2[1]) at the edge voxels of gt,
 * dist[1][0..n_pred) = sqrt(dt2[0]) at the edge voxels of pred; rows are row_stride doubles apart and the order inside a row is
 * unspecified (the percentile sorts).  n_gt / n_pred are info[0] / info[1] of mi355seg_mask_edges_i64; cursor: int64[2] scratch. */
int mi355seg_surface_distances_f64(const uint8_t* edges, int D, int H, int W, int z0, int y0, int x0, int bd, int bh, int bw,
                                   const double* dt2, long long n_gt, long long n_pred, double* dist, long long row_stride,
                                   int64_t* cursor, void* stream);

/* Connected components of a label volume: the clean-up of the mask between predict.py:139-147 and predict.py:151/154 (drop small
 * islands, keep the K largest structures); semantics of scipy.ndimage.label with generate_binary_structure(3, 1 / 2 / 3).
 * Foreground is != 0 whatever the label value, two foreground voxels are joined when they are neighbours under `connectivity`
 * 6 (faces), 18 (+ edges) or 26 (+ corners), outside the array is background.  csrc/components.hip, DESIGN.md section 4.14.
 *
 * labels: int32 [D][H][W], 0 on background, on foreground 1 + the z,y,x raster index of the FIRST voxel of the voxel's component:
 * independent of scheduling, so two runs are bitwise equal.  D*H*W <= 2^31 - 2, larger volumes are refused.
 * sizes: int32 [D*H*W]; sizes[r] = voxels of the component whose label is r + 1, 0 in every other slot.
 * info: int64[4] = foreground voxels, components, size of the largest component, its label (equal sizes: the smaller label;
 * 0, 0 for an empty mask).  labels and sizes 16-byte aligned.  ws: mi355seg_components_ws_bytes(D, H, W) (0 for bad extents).
 * mi355seg_components_tile_extent(axis): the extent along z (0), y (1), x (2) of the tiles the volume is cut into, each labelled by
 * one workgroup before the tiles are merged (0 for any other axis); for tests that place structures across tile borders. */
int mi355seg_components_tile_extent(int axis);
size_t mi355seg_components_ws_bytes(int D, int H, int W);
int mi355seg_components_label_i64(const int64_t* mask, int D, int H, int W, int connectivity,
                                  int32_t* labels, int32_t* sizes, int64_t* info,
                                  void* ws, size_t ws_bytes, void* stream);
/* The same call cut short after its first `steps` of five launches (local, merge, flatten, info, info-finalise): the outputs are
 * complete only with steps = 5.  For tools/bench_components.py, which times each launch as the difference of two prefixes. */
int mi355seg_components_label_steps_i64(const int64_t* mask, int D, int H, int W, int connectivity,
                                        int32_t* labels, int32_t* sizes, int64_t* info,
                                        void* ws, size_t ws_bytes, int steps, void* stream);

/* out[v] = keep(labels[v]) ? mask[v] : 0 with labels / sizes of mi355seg_components_label_i64: a component is kept when
 * sizes[label - 1] >= min_voxels and, where a keep list is given, its label is one of keep_labels[0..n_keep) (int32 on the device,
 * 0 <= n_keep <= 16; keep_labels == NULL: no list; a list of 0 labels keeps nothing).  Mask values are preserved.  out may be
 * mask itself.  removed: int64[1] = the number of voxels set to 0.  labels 8-byte aligned. */
int mi355seg_components_filter_i64(const int64_t* mask, const int32_t* labels, const int32_t* sizes, long long numel,
                                   long long min_voxels, const int32_t* keep_labels, int n_keep,
                                   int64_t* out, int64_t* removed, void* stream);

/* The class-aware labelling: two voxels are joined only when they are neighbours under `connectivity` AND
 * carry the same value 1..255; the reference is scipy.ndimage.label(mask == k, ...) for every value k != 0 that occurs.  All
 * classes are labelled by one call.  Arguments, labels and sizes as mi355seg_components_label_i64: a component is a component of
 * one class, components of different classes have different first voxels, so one labels volume holds them all; the class of a
 * component is the mask value at its first voxel.  0 and every value outside 0..255 is background.
 * info: int64[8] = slots 0..3 as mi355seg_components_label_i64 over all classes, slot 4 = voxels whose value lies outside 0..255
 * (the caller's refusal; they are background in labels and sizes), slots 5..7 = 0.  8-byte aligned.
 * ws: mi355seg_components_classes_ws_bytes(D, H, W) (0 for bad extents): the binary call's plus one byte per voxel.
 * _steps_: the call cut short after its first `steps` of five launches, as above, for tools/bench_class_components.py. */
size_t mi355seg_components_classes_ws_bytes(int D, int H, int W);
int mi355seg_components_label_classes_i64(const int64_t* mask, int D, int H, int W, int connectivity,
                                          int32_t* labels, int32_t* sizes, int64_t* info,
                                          void* ws, size_t ws_bytes, void* stream);
int mi355seg_components_label_classes_steps_i64(const int64_t* mask, int D, int H, int W, int connectivity,
                                                int32_t* labels, int32_t* sizes, int64_t* info,
                                                void* ws, size_t ws_bytes, int steps, void* stream);

/* The compact table of the n components of a labelling (either form), ranked by first voxel in raster order -- the order in which
 * scipy.ndimage.label numbers them --, and the consecutive labels: first[k] = raster index of the first voxel, size[k] = voxels,
 * cls[k] = mask value at the first voxel of the component of rank k (int32[n], int32[n], int64[n]);
 * labels_consecutive: int32 [numel] = rank + 1 of the voxel's component, 0 on background.  n = info[1] of the labelling call, read
 * back by the caller: it sizes the three tables, and a component whose rank is not below n writes none of them.  n = 0: the tables
 * may be NULL.  labels, sizes, labels_consecutive and ws 16-byte aligned.  ws: mi355seg_components_table_ws_bytes(numel). */
size_t mi355seg_components_table_ws_bytes(long long numel);
int mi355seg_components_table_i64(const int64_t* mask, const int32_t* labels, const int32_t* sizes, long long numel, long long n,
                                  int32_t* labels_consecutive, int32_t* first, int32_t* size, int64_t* cls,
                                  void* ws, size_t ws_bytes, void* stream);

/* out[v] = (labels_consecutive[v] == 0 || keep[labels_consecutive[v] - 1]) ? mask[v] : 0 with one flag per component of the
 * table (uint8[n] on the device, non-zero = keep; n = 0: keep may be NULL; a label above n is not kept).  Mask values are preserved.
 * out may be mask itself.  removed: int64[1] = the number of voxels set to 0.  labels_consecutive 8-byte aligned. */
int mi355seg_components_filter_table_i64(const int64_t* mask, const int32_t* labels_consecutive, const uint8_t* keep, long long n,
                                         long long numel, int64_t* out, int64_t* removed, void* stream);

/* The 2-channel target of the live loop (train.py:190-193): out[n][0] = (gt[n] == 0), out[n][1] = gt[n], float [N,2,S]. */
int mi355seg_two_channel_gt_f32(const float* gt, float* out, long long N, long long S, void* stream);

/* Fused train-step tail (train.py:204,209,221 in one pass over the logits):
 * BCE mean loss, argmax mask (int64), gt.argmax and the four Dice counters.
 * target is the K-channel float one-hot [N,K,S]. */
int mi355seg_bce_argmax_dice_f32(const float* logits, const float* target, long long N, int K, long long S,
                                 float* loss, int64_t* mask, int64_t* counts,
                                 void* ws, size_t ws_bytes, void* stream);

/* Fused train-step tail for the compound losses (config.loss; csrc/loss_tail.hip): loss = w_voxel * voxel + w_region * region,
 * the argmax mask, gt.argmax and the four Dice counters (train.py:204,221; same order, NaN rule and counter arithmetic as
 * mi355seg_bce_argmax_dice_f32) from ONE pass over logits and target [N,K,S], 1 <= K <= 16, plus a one-block finalise.
 *   voxel_term: 0 none | 1 bce   (nn.BCEWithLogitsLoss, train.py:115,209: mean over N*K*S of max(x,0) - x t + log1p(exp(-|x|)))
 *                      | 2 focal (no reference line; Lin et al.: mean of q^gamma * bce, q = p + t - 2 p t, p = sigmoid(x);
 *                                 gamma = 0 or 1 <= gamma <= 8, gamma = 0 is the bce path)
 *                      | 3 ce    (cross_entropy_3D, loss_function.py:8-16, size_average=True, label = argmax_k target; K >= 2)
 *   region_term: 0 none | 1 dice    (DiceLoss, loss_function.py:121-130: 1 - 2 (sum I + eps) / (sum P + sum T + eps), eps = 1e-5)
 *                       | 2 tversky (no reference line; Salehi et al.: 1 - (1/K) sum_k (I_k + eps) / (I_k + alpha (P_k - I_k)
 *                                    + beta (T_k - I_k) + eps), alpha, beta >= 0, alpha + beta > 0)
 * with per class I_k = sum p t, P_k = sum p, T_k = sum t over the batch.  Outputs (device): loss fp32[1]; terms fp64[2] (voxel,
 * region, unweighted; 0 for an absent term); sums fp64[K][5] (the five sums of mi355seg_dice_sums_f32 with the sigmoid, per
 * class); mask int64 [N,1,S]; counts int64[4]; coef fp64[1 + 2 K], what the backward needs (w_voxel, w_region *
 * dRegion/dI_k, w_region * dRegion/dP_k).  Nothing passes through the host; deterministic (fixed-order partials, no atomics).
 * Refused before any launch: null pointers, K outside 1..16, an unknown term, both terms absent, ce with K = 1, gamma outside
 * {0} u [1,8], negative alpha / beta / weights, a workspace below mi355seg_loss_tail_ws_bytes (which is 0 for bad extents). */
size_t mi355seg_loss_tail_ws_bytes(long long N, int K, long long S);
int mi355seg_loss_tail_fwd_f32(const float* logits, const float* target, long long N, int K, long long S,
                               int voxel_term, int region_term, float gamma, float alpha, float beta, float w_voxel, float w_region,
                               float* loss, double* terms, double* sums, int64_t* mask, int64_t* counts, double* coef,
                               void* ws, size_t ws_bytes, void* stream);
/* dlogits = gscale[0] * dloss/dlogits in ONE pass over logits and target (16-byte loads when S % 4 == 0 and the pointers are
 * aligned); coef from the forward, gscale the upstream scalar on the device.  No workspace.  Each term's gradient is rounded to
 * fp32 as the kernels of the unfused criterion round it (mi355seg_bce_logits_bwd_f32, mi355seg_ce3d_bwd_f32,
 * mi355seg_dice_sums_bwd_f32) and the two are then added: with 0 / 1 targets and unit weights bce + dice and ce + dice have the
 * bits of those kernels' summed outputs. */
int mi355seg_loss_tail_bwd_f32(const float* logits, const float* target, const double* coef, const float* gscale,
                               long long N, int K, long long S, int voxel_term, int region_term, float gamma,
                               float* dlogits, void* stream);

/* Label-map targets (config.multiclass; csrc/loss_tail.hip).
 * labels_u8[i] = (uint8) gt[i] for the float label map gt[n] ([N,1,S] as the patch queue delivers it), K classes, 1 <= K <= 16.  A
 * value that is not an integer in [0, K) (a NaN included) is stored as 255 and counted: the number of such voxels is ADDED to the
 * device counter bad (int64[1], 8-byte aligned; the caller zeroes it once and reads it when it likes).  One streaming launch; the
 * counter is written only by a block that met such a value (one integer add per block, order-free).
 * Refused before any launch: null pointers, K outside 1..16, n < 1, a misaligned counter. */
int mi355seg_labels_u8_f32(const float* gt, long long n, int K, uint8_t* labels_u8, int64_t* bad, void* stream);
/* out[n][k][s] = (labels_u8[n][s] == k) as float, [N,K,S]; a label >= K (255) gives an all-zero column.  For the terms that take a
 * one-hot target (cldice, boundary) and for tests.  Refused before any launch: null pointers, K outside 1..16, N or S < 1. */
int mi355seg_onehot_u8_f32(const uint8_t* labels_u8, long long N, int K, long long S, float* out, void* stream);

/* mi355seg_loss_tail_fwd_f32 / _bwd_f32 with the uint8 label map labels [N,S] in place of the float one-hot target [N,K,S]: the
 * same terms, weights and outputs, and one more output, class_counts int64[3 K] = per class k (tp_k, pred_k, gt_k): voxels with
 * argmax logits == k and label == k, with argmax logits == k, with label == k.  Class membership is the comparison label == k,
 * never an index: a label >= K belongs to no class, and gt.argmax of the four Dice counters (and the ce label) is then 0, what
 * the one-hot form gives for an all-zero column.
 * CONTRACT: for labels in [0, K) every output that the one-hot entry points also produce (loss, terms, sums, mask, counts, coef,
 * dlogits) has the bits they produce on mi355seg_onehot_u8_f32(labels).  Deterministic (fixed-order partials, no atomics),
 * nothing passes through the host, capturable in a HIP graph; 16-byte logit loads and 4-byte label loads when S % 4 == 0, K <= 4.
 * The forward is the pass and the one-block finalise; above four classes one more launch counts tp_k and pred_k from the labels
 * and the mask the pass wrote.
 * Refused before any launch: what mi355seg_loss_tail_fwd_f32 refuses (null pointers, K outside 1..16, an unknown term, both terms
 * absent, ce with K = 1, gamma outside {0} u [1,8], negative alpha / beta / weights), a workspace below
 * mi355seg_loss_tail_lab_ws_bytes (0 for bad extents), and, where S % 4 == 0 and K <= 4, logits / dlogits not 16-byte or labels
 * not 4-byte aligned (the one-hot form would take its scalar path there; this form refuses, so that its path follows from S). */
size_t mi355seg_loss_tail_lab_ws_bytes(long long N, int K, long long S);
int mi355seg_loss_tail_fwd_lab_f32(const float* logits, const uint8_t* labels, long long N, int K, long long S,
                                   int voxel_term, int region_term, float gamma, float alpha, float beta, float w_voxel, float w_region,
                                   float* loss, double* terms, double* sums, int64_t* mask, int64_t* counts, double* coef,
                                   int64_t* class_counts, void* ws, size_t ws_bytes, void* stream);
int mi355seg_loss_tail_bwd_lab_f32(const float* logits, const uint8_t* labels, const double* coef, const float* gscale,
                                   long long N, int K, long long S, int voxel_term, int region_term, float gamma,
                                   float* dlogits, void* stream);

/* The same int64[3 K] (per class tp_k, pred_k, gt_k) from two int64 label volumes of n voxels, where no loss runs (predict.py):
 * one pass plus the shared partials finalise.  A value outside [0, K) in either volume belongs to no class.
 * Refused before any launch: null pointers, K outside 1..16, n < 1, a workspace below mi355seg_class_counts_ws_bytes or not
 * 8-byte aligned. */
size_t mi355seg_class_counts_ws_bytes(long long n, int K);
int mi355seg_class_counts_i64(const int64_t* gt_labels, const int64_t* pred_labels, long long n, int K, int64_t* out,
                              void* ws, size_t ws_bytes, void* stream);

/* Soft-clDice loss term (csrc/cldice.hip; no reference line in this project's model: the official clDice of Shit
 * et al., CVPR 2021 -- soft_skeleton.py's soft_erode / soft_dilate / soft_open / soft_skel and cldice.py's soft_cldice).
 * Volumes are [NC, D, H, W] fp32, W fastest, at most 2^31 - 1 voxels per call; iters in 1..32.
 *
 * The soft skeleton (replaces soft_skel's chain of max_pool3d, minima, subtractions and ReLUs) is iters + 1 levels j = 0 .. iters:
 *   E_{j+1} = erode(E_j) (minimum over the voxel and its 6 face neighbours), delta = relu(E_j - dilate(E_{j+1})) (dilate: maximum
 *   over the 3x3x3 box), skel = skel + relu(delta - skel * delta), with E_0 = x and skel = 0; voxels outside the volume never take
 *   part.  The forward has the bits of that composition in ATen fp32 (no FMA contraction).
 * mi355seg_soft_skel_ws_bytes: the size of the level stack the caller keeps from the forward to the backward, 2 (iters + 1) volumes
 *   (E_1 .. E_{iters+1}, then the skeleton after each level; each slot rounded up to 256 bytes; 0 for bad arguments).  The finished
 *   skeleton is the LAST slot, at byte offset (2 iters + 1) * slot.
 * mi355seg_soft_skel_step_fwd_f32: level j, one launch: reads E_j (x for j = 0) and the skeleton so far (taken as zero for j = 0:
 *   no memset), writes E_{j+1} and the new skeleton into the stack.  Call it for j = 0, 1, .., iters.
 * mi355seg_soft_skel_step_bwd_f32: level j of the backward, one launch in gather form, called for j = iters, .., 1, 0:
 *   g_skel_out = the gradient of the skeleton after level j, g_e_next = the gradient later levels sent to E_{j+1} (NULL: zero, as at
 *   j = iters); writes g_e = the gradient of E_j and g_skel_in = the gradient of the skeleton before level j (not written and may be
 *   NULL at j = 0).  Arg-max and arg-min are recomputed from the stack; a tie routes the whole gradient to the candidate with the
 *   lowest raster index (z, then y, then x) -- what ATen does for the 27-maximum, not what it does for the minimum of three pools.
 *   An output must not alias an input.
 * mi355seg_cldice_probs_f32: P = sigmoid(logits[:, c0:]), T = target[:, c0:] as contiguous [N, K - c0, S], c0 = 1 for K > 1 (the
 *   background channel is left out), 0 for K = 1 (replaces y_pred[:, 1:] / y_true[:, 1:] of soft_dice_cldice).
 * mi355seg_cldice_sums_f32: sum S_P T, sum S_P, sum S_T P, sum S_T over n elements as fp64 partials in fixed order, one pass
 *   (replaces the four torch.sum of soft_cldice); ws of mi355seg_cldice_ws_bytes(n).
 * mi355seg_cldice_finalize: one block: tprec = (sum S_P T + smooth) / (sum S_P + smooth), tsens = (sum S_T P + smooth) /
 *   (sum S_T + smooth), cldice = 1 - 2 tprec tsens / (tprec + tsens); loss fp32[1] = cldice, parts fp64[3] = (cldice, tprec, tsens),
 *   coef fp64[3] = (a, b, c) of the backward, all on the device (nothing passes through the host: capturable in a HIP graph).
 * mi355seg_cldice_bwd_head_f32: g_skel = a T + b, the gradient of cldice with respect to S_P.
 * mi355seg_cldice_bwd_tail_f32: dlogits[:, c0:] = gscale[0] (g_p + c S_T) P (1 - P) with g_p the gradient that the skeleton's
 *   backward returned for P; channel 0 (K > 1) gets zeros.  dlogits is [N, K, S].
 * Refused before any launch, with mi355seg_last_error: null pointers, non-positive extents, more than 2^31 - 1 elements, iters
 * outside 1..32, j outside 0..iters, smooth <= 0, a workspace that is too small. */
size_t mi355seg_soft_skel_ws_bytes(long long NC, int D, int H, int W, int iters);
int mi355seg_soft_skel_step_fwd_f32(const float* x, long long NC, int D, int H, int W, int iters, int j,
                                    void* ws, size_t ws_bytes, void* stream);
int mi355seg_soft_skel_step_bwd_f32(const float* x, const float* g_skel_out, const float* g_e_next, float* g_e, float* g_skel_in,
                                    long long NC, int D, int H, int W, int iters, int j,
                                    const void* ws, size_t ws_bytes, void* stream);
int mi355seg_cldice_probs_f32(const float* logits, const float* target, long long N, int K, long long S,
                              float* P, float* T, void* stream);
size_t mi355seg_cldice_ws_bytes(long long n);
int mi355seg_cldice_sums_f32(const float* skel_p, const float* skel_t, const float* P, const float* T, long long n,
                             void* ws, size_t ws_bytes, void* stream);
int mi355seg_cldice_finalize(const void* ws, size_t ws_bytes, long long n, float smooth,
                             float* loss, double* parts, double* coef, void* stream);
int mi355seg_cldice_bwd_head_f32(const float* T, const double* coef, long long n, float* g_skel, void* stream);
int mi355seg_cldice_bwd_tail_f32(const float* g_p, const float* skel_t, const float* P, const double* coef, const float* gscale,
                                 long long N, int K, long long S, float* dlogits, void* stream);

/* Boundary loss term (csrc/boundary.hip; no reference line in this project's model: the official boundary-loss of
 * Kervadec et al., MIDL 2019 -- utils.py's one_hot2dist and losses.py's SurfaceLoss).  Channels c0 .. K - 1 take part, c0 = 1 for
 * K > 1 (the background channel is left out), 0 for K = 1, as in mi355seg_cldice_probs_f32; 1 <= K <= 16.
 *
 * mi355seg_sdm_f32: the signed Euclidean distance map of every class of the float one-hot target [N, K, D, H, W] (W fastest;
 *   voxel v belongs to class k when target[n, k, v] > 0.5) under the voxel spacing (sz, sy, sx): phi fp32 [N, K - c0, D, H, W] with
 *     phi = +dist(v, nearest voxel of the class)                 outside the class,
 *     phi = -(dist(v, nearest voxel not of the class) - offset)  inside the class,
 *     phi = 0 for the whole (n, k) volume where the opposite set is empty (class absent from the patch, or class fills it).
 *   Distances are taken inside the patch only.  DEVIATION from one_hot2dist, whose inside branch is (posdist - 1): that is right at
 *   unit spacing only (at spacing 0.7 it gives +0.3 on the inner boundary, the wrong sign).  Callers pass offset = min(sz, sy, sx),
 *   the smallest distance an inside voxel can have: the official map at unit spacing, and never positive inside at any spacing.
 *   Three separable fp32 passes (W from wave ballots, H and D as min-plus steps through LDS), no fp64, no atomics: two runs are
 *   bitwise equal and a batched run has the bits of single-volume runs.  At unit spacing every squared distance is an integer below
 *   2^24, so the map is the correctly rounded square root of the exact squared distance.  Each axis at most 2047.
 *   ws: mi355seg_sdm_ws_bytes(N, K, D, H, W) (0 for bad arguments): 12 bytes per voxel of phi.
 * mi355seg_sdm_steps_f32: the same call cut short after its first `steps` of three launches (W, H, D): phi is written only with
 *   steps = 3.  For tools/bench_boundary.py, which times each launch as the difference of two prefixes.
 * mi355seg_boundary_fwd_f32: sum sigmoid(logits[:, c0:]) * phi over n = N (K - c0) S elements as fp64 partials in fixed order, one
 *   pass, then one block: loss fp32[1] = sum / n, parts fp64[1] = the same in fp64, coef fp64[1] = 1 / n, all on the device
 *   (nothing passes through the host: capturable in a HIP graph).  logits [N, K, S], phi [N, K - c0, S].
 *   ws: mi355seg_boundary_ws_bytes(n) (0 for n < 1).
 * mi355seg_boundary_bwd_f32: dlogits[:, c0:] = gscale[0] coef[0] phi p (1 - p), p = sigmoid(logits), in one pass (16-byte accesses
 *   when S % 4 == 0 and the pointers are aligned); channel 0 (K > 1) gets zeros.  dlogits is [N, K, S].
 * Refused before any launch, with mi355seg_last_error: null pointers, non-positive extents or spacing, a negative offset, K outside
 * 1..16, an axis above 2047, more than 2^31 - 1 voxels per (n, k) volume or tiles per launch (one block per 64 x 32 tile: beyond
 * any memory), steps outside 1..3, a workspace that is too small. */
size_t mi355seg_sdm_ws_bytes(long long N, int K, int D, int H, int W);
int mi355seg_sdm_f32(const float* target, long long N, int K, int D, int H, int W, float sz, float sy, float sx, float offset,
                     float* phi, void* ws, size_t ws_bytes, void* stream);
int mi355seg_sdm_steps_f32(const float* target, long long N, int K, int D, int H, int W, float sz, float sy, float sx, float offset,
                           float* phi, void* ws, size_t ws_bytes, int steps, void* stream);
size_t mi355seg_boundary_ws_bytes(long long n);
int mi355seg_boundary_fwd_f32(const float* logits, const float* phi, long long N, int K, long long S,
                              float* loss, double* parts, double* coef, void* ws, size_t ws_bytes, void* stream);
int mi355seg_boundary_bwd_f32(const float* logits, const float* phi, const double* coef, const float* gscale,
                              long long N, int K, long long S, float* dlogits, void* stream);

/* Sum-type reductions for the library losses (loss_function.py:61-185):
 * out[0]=sum(a*b) out[1]=sum(a) out[2]=sum(b) out[3]=sum(a*a) out[4]=sum(b*b), a = sigmoid(x) if
 * apply_sigmoid else x.  Deterministic wavefront-shuffle + two-stage reduce. */
int mi355seg_dice_sums_f32(const float* x, const float* t, long long numel, int apply_sigmoid,
                           double* out5, void* ws, size_t ws_bytes, void* stream);

/* d/dx of  L(S0..S4)  with S = dice_sums(x, t): dx[i] = (g[0]*t + g[1] + 2*g[3]*a) * da/dx, a = sigmoid(x) or x.
 * g = dL/dS as 5 device doubles (g[2], g[4] multiply target-only sums and do not reach x). */
int mi355seg_dice_sums_bwd_f32(const float* x, const float* t, const double* g5, long long numel, int apply_sigmoid,
                               float* dx, void* stream);

/* The same five sums for `rows` contiguous rows of `len` elements in ONE launch: out[r*5 + j].  BinaryDiceLoss reduces per
 * sample (loss_function.py:78-83: predict.view(N, -1)), DiceLossss per (sample, class) (loss_function.py:160-183).  `p` is
 * BinaryDiceLoss's denominator exponent (loss_function.py:82, any value): out[r*5+3] = sum a^p, out[r*5+4] = sum b^p. */
size_t mi355seg_dice_rows_ws_bytes(long long rows, long long len);
int mi355seg_dice_rows_f32(const float* x, const float* t, long long rows, long long len, int apply_sigmoid, float p,
                           double* out, void* ws, size_t ws_bytes, void* stream);
/* dx[r][i] = (g[r*5+0]*t + g[r*5+1] + g[r*5+3] * p * a^(p-1)) * da/dx */
int mi355seg_dice_rows_bwd_f32(const float* x, const float* t, const double* g, long long rows, long long len, int apply_sigmoid,
                               float p, float* dx, void* stream);

/* tio.ZNormalization() of one volume (dataloader.py:94): y = (x - mean) / std over all n voxels, unbiased std, fp64 sums;
 * in place (y == x) allowed.  The device patch queue normalises each uploaded volume once with it. */
size_t mi355seg_znorm_ws_bytes(long long n);
int mi355seg_znorm_f32(const float* x, long long n, float* y, void* ws, size_t ws_bytes, void* stream);

/* softmax over the channel dim of an NCDHW tensor [N,K,S] (DiceLossss softmax=True, loss_function.py:170-171) */
int mi355seg_softmax_ch_f32(const float* x, float* y, long long N, int K, long long S, void* stream);
/* dx = y * (dy - sum_k dy*y) */
int mi355seg_softmax_ch_bwd_f32(const float* y, const float* dy, float* dx, long long N, int K, long long S, void* stream);

/* cross_entropy_3D (loss_function.py:8-16): loss[0] = sum_v w[label_v] * (logsumexp_k x[v,k] - x[v,label_v]),
 * divided by the voxel count when size_average.  logits NCDHW [N,K,S], labels int64 [N,S], weight [K] or NULL.
 * A voxel whose label is outside [0, K) (F.nll_loss's ignore_index -100 among them) is ignored: no term in the sum, a zero
 * gradient row, the divisor unchanged; no label value indexes the logits or the weights. */
int mi355seg_ce3d_fwd_f32(const float* logits, const int64_t* labels, const float* weight, long long N, int K, long long S,
                          int size_average, float* loss, void* ws, size_t ws_bytes, void* stream);
int mi355seg_ce3d_bwd_f32(const float* logits, const int64_t* labels, const float* weight, const float* gscale,
                          long long N, int K, long long S, int size_average, float* dlogits, void* stream);

/* ------------------------------------------------------------------ UNETR encoder (unetr.py:54-168)
 * Strided, batched fp32 GEMM on the MFMA:  C[b0,b1][m][n] (+)= alpha * sum_k A[..][m][k] * B[..][k][n]  (+ bias[n]) (relu).
 * Element strides: A(m,k) at a_rs*m + a_cs*k + a_b0*b0 + a_b1*b1, B(k,n) likewise, C(m,n) at c_rs*m + n + c_b0*b0 + c_b1*b1.
 * Replaces nn.Linear (unetr.py:61-66,120-121), torch.matmul of the attention (unetr.py:88,94) and their backward. */
int mi355seg_gemm_f32(const float* A, long long a_rs, long long a_cs, long long a_b0, long long a_b1,
                      const float* B, long long b_rs, long long b_cs, long long b_b0, long long b_b1,
                      float* C, long long c_rs, long long c_b0, long long c_b1, const float* bias,
                      int M, int N, int K, int nb0, int nb1, float alpha, int relu, int accumulate,
                      void* ws, size_t ws_bytes, void* stream);
/* The same GEMM with its products on the bf16 matrix cores: fp32 operands rounded to bf16 (RNE) in registers, v_mfma_f32_32x32x16_bf16,
 * fp32 accumulation and result -- the arithmetic of the reference's nn.Linear / matmul under torch.autocast(bfloat16)
 * (/root/reference/models/three_d/unetr.py:59-138), used by the token path inside functional.autocast(torch.bfloat16).  Few-hundred-row
 * shapes run the small-GEMM kernel on the bf16 matrix cores; other shapes (K % 8 != 0, an operand that is not 16-byte aligned, more than
 * 4,096 32x32 tiles) run the 64x64-tile kernel of mi355seg_gemm_f32 on operands rounded to bf16 in the same way: the same arithmetic
 * (a product of two bf16 values is exact in fp32), so the result does not depend on which kernel a shape or an address selects. */
int mi355seg_gemm_lowp_f32(const float* A, long long a_rs, long long a_cs, long long a_b0, long long a_b1,
                      const float* B, long long b_rs, long long b_cs, long long b_b0, long long b_b1,
                      float* C, long long c_rs, long long c_b0, long long c_b1, const float* bias,
                      int M, int N, int K, int nb0, int nb1, float alpha, int relu, int accumulate,
                      void* ws, size_t ws_bytes, void* stream);
/* nn.Linear forward with the element-wise operations that follow it in the token encoder in the GEMM's epilogue (r5;
 * /root/reference/models/three_d/unetr.py:98-100,120-138,159-166): y[M][N] = (relu?)(x W^T + b) * emul + eadd, emul = a dropout layer's
 * keep / (1 - p) factors, eadd = the residual stream the block adds its output to, both [M][N] at pitch N, either may be NULL.  One launch
 * on the few-hundred-row shapes (each of the two was a launch of its own); other shapes: the GEMM, then the element-wise kernels in place.
 * lowp != 0: products on the bf16 matrix cores (mi355seg_gemm_lowp_f32).  ws: mi355seg_gemm_ws_bytes(M, N, K, 1, 1). */
int mi355seg_linear_fwd_f32(int lowp, const float* x, int ldx, const float* w, const float* b, int relu, const float* emul, const float* eadd,
                            float* y, int M, int N, int K, void* ws, size_t ws_bytes, void* stream);
/* Weight and bias gradient of nn.Linear in one call (r5; /root/reference/models/three_d/unetr.py:61-66,120-121 backward):
 * dw[N][K] = dy^T x and db[n] = sum_m dy[m][n] -- on the few-hundred-row shapes of the token encoder the bias gradient is summed by the
 * weight-gradient GEMM's first column of tiles from the dy values it loads anyway (one launch instead of two per layer; fixed
 * summation order); other shapes run the GEMM and mi355seg_colsum_f32.  lowp != 0: products on the bf16 matrix cores
 * (mi355seg_gemm_lowp_f32).  db may be NULL.  ws: max(mi355seg_gemm_ws_bytes(N, K, M, 1, 1), mi355seg_norm_ws_bytes(M, 1, N)). */
int mi355seg_linear_wgrad_f32(int lowp, const float* dy, int lddy, const float* x, int ldx, float* dw, float* db, int M, int N, int K,
                              void* ws, size_t ws_bytes, void* stream);
/* The backward of nn.Linear as ONE launch (r6; /root/reference/models/three_d/unetr.py:61-66,98-100,120-138 backward): with
 * dyf = dy * dmul * [dgate > 0] (dmul: the keep / (1 - p) factors of the dropout layer behind the Linear, dgate: the ReLU's saved output; either
 * may be NULL) it writes dx[M][K] = dyf W, dw[N][K] = dyf^T x and db[n] = sum_m dyf[m][n] (db may be NULL).  The two GEMMs are independent and
 * latency-bound at the token encoder's sizes (216 rows): they run as two problems of one grid, the element-wise factors folded into their loads
 * of dy (they were an element-wise launch each), every result bit-identical to the separate launches'.  bf16 products (lowp != 0) on shapes
 * mi355seg_linear_bwd_supported_f32 accepts; the caller runs mi355seg_gemm_lowp_f32 + mi355seg_linear_wgrad_f32 otherwise. */
int mi355seg_linear_bwd_supported_f32(int lowp, int M, int N, int K);
int mi355seg_linear_bwd_f32(int lowp, const float* dy, int lddy, const float* dmul, const float* dgate, const float* x, int ldx, const float* w,
                            float* dx, float* dw, float* db, int M, int N, int K, void* stream);
/* Two independent batched small GEMMs C_p[b0][b1] = alpha_p A_p B_p (p = 0, 1; nb0 x nb1 batches each, own strides) in one launch (r6:
 * the pairs of attention's backward, dP = dO V^T with dV = Pd^T dO and dQ = dS K with dK = dS^T Q, unetr.py:74-98 backward).  bf16 products,
 * fp32 accumulation; each result bit-identical to mi355seg_gemm_lowp_f32's.  Shapes: mi355seg_gemm_pair_supported_f32. */
int mi355seg_gemm_pair_supported_f32(int M0, int N0, int K0, int M1, int N1, int K1, int nb0, int nb1);
int mi355seg_gemm_pair_lowp_f32(const float* A0, long long a0_rs, long long a0_cs, long long a0_b0, long long a0_b1,
                                const float* B0, long long b0_rs, long long b0_cs, long long b0_b0, long long b0_b1,
                                float* C0, long long c0_rs, long long c0_b0, long long c0_b1, int M0, int N0, int K0, float alpha0,
                                const float* A1, long long a1_rs, long long a1_cs, long long a1_b0, long long a1_b1,
                                const float* B1, long long b1_rs, long long b1_cs, long long b1_b0, long long b1_b1,
                                float* C1, long long c1_rs, long long c1_b0, long long c1_b1, int M1, int N1, int K1, float alpha1,
                                int nb0, int nb1, void* stream);
/* Scratch for the deterministic split-K path (single-batch GEMMs with too few 64x64 tiles to fill 256 CUs); 0 when
 * the shape is not split.  With a smaller / NULL workspace the GEMM runs unsplit. */
size_t mi355seg_gemm_ws_bytes(int M, int N, int K, int nb0, int nb1);
/* nn.LayerNorm(E, eps) over the last dim of [rows, E] (unetr.py:151-152); mean/rstd [rows] are saved for backward */
int mi355seg_layernorm_fwd_f32(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                               long long rows, int E, float eps, void* stream);
int mi355seg_layernorm_bwd_f32(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                               float* dx, float* dgamma, float* dbeta, long long rows, int E, void* stream);
/* The same with dx = addend + (LayerNorm backward of dy): `addend` is a second gradient of x -- the residual stream that bypasses the norm in a
 * pre-norm transformer block (x + f(LN(x)), /root/reference/models/three_d/unetr.py:159-166) -- summed in the kernel that writes dx instead of
 * by a separate add (r5).  addend NULL: mi355seg_layernorm_bwd_f32. */
int mi355seg_layernorm_bwd_add_f32(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, const float* addend,
                                   float* dx, float* dgamma, float* dbeta, long long rows, int E, void* stream);
/* nn.Softmax(dim=-1) on [rows, L] (unetr.py:71,90) and its backward dx = y * (dy - sum(dy*y)) */
int mi355seg_softmax_rows_f32(const float* x, float* y, long long rows, int L, void* stream);
int mi355seg_softmax_rows_bwd_f32(const float* y, const float* dy, float* dx, long long rows, int L, void* stream);
/* softmax over the last dim followed by an elementwise factor (the attention dropout of /root/reference/models/three_d/unetr.py:92-93,
 * keep = mask / (1 - p)): y = softmax(x) and yk = y * keep from one pass over x; backward of the pair from d(yk): dx = y (dy - sum y dy),
 * dy = dyk * keep (r5: three launches per attention layer and direction were softmax, mask product, [mask product]). */
int mi355seg_softmax_rows_keep_f32(const float* x, const float* keep, float* y, float* yk, long long rows, int L, void* stream);
int mi355seg_softmax_rows_keep_bwd_f32(const float* y, const float* dyk, const float* keep, float* dx, long long rows, int L, void* stream);
/* out[c] = sum over rows of x[r, c] (bias gradient of nn.Linear); ws >= mi355seg_norm_ws_bytes(rows, 1, C) */
int mi355seg_colsum_f32(const float* x, int ldx, long long rows, int C, float* out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ In-library kernel timing
 * Optional HIP-event timing of the kernel families, on the stream each kernel is launched
 * on (used by bench.py for the live roofline numbers; off by default, zero cost when off).
 * Families: 0 conv implicit-GEMM (fwd+dgrad), 1 conv wgrad MFMA, 2 conv generic, 3 convT,
 * 4 norm/act, 5 pool/upsample, 6 loss/metric, 7 stem/head direct conv.
 * prof_read synchronises the recorded events and returns, per family f:
 *   out[4*f+0] = launches, out[4*f+1] = total milliseconds,
 *   out[4*f+2] = total algorithmic FLOPs, out[4*f+3] = total algorithmic bytes. */
#define MI355SEG_PROF_FAMILIES 8
/* on: 0 = off, 1 = every family, otherwise 2 * (bit mask of families): only those launches are bracketed, so the
 * event records do not serialise the many small kernels of a step that is being timed as a whole. */
int mi355seg_prof_enable(int on);
int mi355seg_prof_reset(void);
int mi355seg_prof_read(double* out_host, int n_doubles);
/* per-launch records: writes up to max_records rows of 4 doubles (family, ms, flops, bytes); returns the
 * number of rows through *n_host (call after prof_read, which synchronises). */
int mi355seg_prof_records(double* out_host, int max_records, int* n_host);

/* ------------------------------------------------------------------ Sliding-window inference (predict.py:98-147)
 * tio.inference.GridSampler patches of one volume [C,D,H,W] as a device-resident batch [count,C,pd,ph,pw], and
 * tio.inference.GridAggregator(overlap_mode='crop') of their int64 label maps [count,pd,ph,pw] into the output volume [D,H,W]: one
 * launch each.  table = int32 [P][9] on the device: patch origin z,y,x, then the crop window inside the patch, lo z,y,x and
 * hi z,y,x (exclusive); the launch handles patches first .. first+count-1.  (Overlapping crop windows are disjoint by
 * construction, so the paste needs no ordering.) */
int mi355seg_gather_patches_f32(const float* vol, int C, int D, int H, int W, const int* table, int first, int count,
                                int pd, int ph, int pw, float* out, void* stream);
int mi355seg_paste_labels_i64(const int64_t* labels, const int* table, int first, int count, int pd, int ph, int pw,
                              int64_t* out, int D, int H, int W, void* stream);
/* Mirror test-time augmentation (not in the reference: predict.py:133 calls the model once per patch).  A flip code is an integer
 * 0..7: bit 2 (value 4) mirrors z, bit 1 (value 2) mirrors y, bit 0 (value 1) mirrors x, inside the patch; m_z(z) = pd-1-z where
 * the z bit is set, else z, and m_y, m_x likewise.  gather_patches_flip reads the batch mirrored,
 * out[b,c,z,y,x] = vol[c, oz + m_z(z), oy + m_y(y), ox + m_x(x)], in one launch; flip = 0 gives the bytes of
 * mi355seg_gather_patches_f32, a flip outside 0..7 is an argument error. */
int mi355seg_gather_patches_flip_f32(const float* vol, int C, int D, int H, int W, const int* table, int first, int count,
                                     int pd, int ph, int pw, int flip, float* out, void* stream);

/* Soft aggregation (predict.py:117,141,146: tio.inference.GridAggregator, add_batch, get_output_tensor; the reference keeps
 * the aggregator's default, overlap_mode='crop'; these are its other modes): the class PROBABILITIES of the patches are blended with a
 * window weight and the argmax is taken afterwards.
 * aggregate_patches restates add_batch of overlap_mode='average' (window of ones) and 'hann' (torchio's separable Hann window) for
 * any separable window wz[pd], wy[ph], wx[pw]: for every patch b = first .. first+count-1 of the table (origin columns only) and
 * every patch voxel (z,y,x), p = softmax over the K channels of logits [count,K,pd,ph,pw] at that voxel (fp32, maximum
 * subtracted) and acc[k, oz+z, oy+y, ox+x] = fmaf((wz[z] * wy[y]) * wx[x], p_k, acc[...]).  acc is fp32 [K,D,H,W], zeroed by the
 * caller before the first batch.  Rows of one batch may overlap each other; per accumulator element the fmafs happen in ascending
 * patch index (add_batch's order), so the result does not depend on the batch size and is bitwise reproducible.  One launch.
 * 2 <= K <= 16. */
int mi355seg_aggregate_patches_f32(const float* logits, int K, const int* table, int first, int count,
                                   int pd, int ph, int pw, const float* wz, const float* wy, const float* wx,
                                   float* acc, int D, int H, int W, void* stream);
/* The accumulate half of mirror test-time augmentation (flip codes: mi355seg_gather_patches_flip_f32): aggregate_patches with the
 * softmax taken over logits[b, :, m_z(z), m_y(y), m_x(x)] -- the prediction of a mirrored patch, un-mirrored as it is read.  The
 * weight (wz[z] * wy[y]) * wx[x] and the destination acc[k, oz+z, oy+y, ox+x] keep the un-mirrored coordinates.  Arithmetic, order,
 * owner rule and kernel choice are those of mi355seg_aggregate_patches_f32 (a thread that owns four consecutive x loads the
 * mirrored quad and reverses it in registers), so the result is bitwise that entry point's on logits flipped along the same axes;
 * flip = 0 gives its bytes.  A caller that adds F flips of every patch into one accumulator hands F * sz to aggregate_finalize.
 * A flip outside 0..7 is an argument error.  One launch. */
int mi355seg_aggregate_patches_flip_f32(const float* logits, int K, const int* table, int first, int count,
                                        int pd, int ph, int pw, const float* wz, const float* wy, const float* wx, int flip,
                                        float* acc, int D, int H, int W, void* stream);
/* get_output_tensor of those modes, then predict.py:139's argmax on the blended volume: labels[z,y,x] = argmax_k acc[k] (int64
 * [D,H,W]; first maximum wins, as mi355seg_argmax_ch_f32) and, where prob != NULL, prob[k] = acc[k] / ((sz[z] * sy[y]) * sx[x])
 * (fp32 [K,D,H,W]).  sz[D], sy[H], sx[W]: per axis the sum of the window over the patch origins that cover the coordinate; the
 * patch grid is a product of per-axis origins, so their product IS torchio's accumulated weight volume and none is kept.
 * sz, sy, sx may be NULL when prob is.  One launch. */
int mi355seg_aggregate_finalize_f32(const float* acc, int K, int D, int H, int W, const float* sz, const float* sy, const float* sx,
                                    int64_t* labels, float* prob, void* stream);

/* ------------------------------------------------------------------ Training augmentation of the patch queue (dataloader.py:69-86)
 * config.aug=True: Compose([RandomBiasField(), ZNormalization(), RandomNoise(), RandomFlip(axes=(0,)), OneOf({RandomAffine(): 0.8,
 * RandomElasticDeformation(): 0.2})]) as ONE resampling gather per batch over the cached raw volumes x [C,D,H,W] / labels [Cy,D,H,W].
 * UNPINNED (torchio is absent and the reference holds no fixture of its data pipeline): the definitions here are the specification.
 *   b(q)    = exp(sum c_ijk a0^i a1^j a2^k), i,j,k >= 0, i+j+k <= 3 (20 coefficients, i outermost, k innermost), a_d = (2 q_d + 1 - n_d) / (n_d - 1)
 *   mu, rho = mean and 1 / (unbiased std) of x * b over every voxel of every channel (fp64 sums)
 *   g(seed, e): standard normal, Philox-4x32-10 (counter = e, the linear element index in [C,D,H,W]; key = seed) + Box-Muller
 *   V(e)    = (x(e) * b(q) - mu) * rho + sigma * g(seed, e), each of the four fp32 operations rounded once; never materialised
 * mi355seg_augment_stats_f32 (dataloader.py:71-73, the intensity transforms of one subject visit): three launches -- fixed-order fp64
 * partial sums, min V per block, finalise -- write stats[0..3] = (mu, rho, min V, sigma) on the DEVICE; bitwise reproducible (no atomics).
 * bias_host: the 20 coefficients in HOST memory (read during the call).  Spatial dims >= 2, D*H*W < 2^31.
 * mi355seg_augment_sample_f32 (dataloader.py:74-84, flip + affine / elastic, then the queue's patch cut): one launch writes the batch
 * out_x [count,C,pd,ph,pw] and out_y [count,Cy,pd,ph,pw] from a device table of int32 [count][MI355SEG_AUG_DESC_WORDS], one descriptor per
 * patch (patches of a batch may come from different subjects; pointers as lo, hi words; floats as their bit patterns):
 *   0-1 x   2-3 labels   4-5 stats (the four floats above)   6-7 control points float [3][7][7][7] (mode 1, else unused)
 *   8-10 D, H, W   11-13 patch origin z, y, x   14 mode (0 affine, 1 elastic)   16-27 M, the 3x4 output -> source map (row-major)
 *   28-47 the 20 bias coefficients   48 sigma   50-51 seed lo, hi   (15, 49, 52-63 reserved)
 * For the output voxel p = origin + offset: t = M [p; 1] (+ the uniform cubic B-spline displacement of the control grid in mode 1:
 * u_d = 4 p_d / (n_d - 1), i_d = min(floor(u_d), 3), f_d = u_d - i_d, sum B_a(f_0) B_b(f_1) B_c(f_2) cp[:, i_0+a, i_1+b, i_2+c]);
 * inside when -0.5 <= t_d < n_d - 0.5 on every axis.  Image: trilinear interpolation of V over the 8 corners (indices clamped to the
 * volume) inside, stats[2] (torchio's default_pad_value='minimum') outside; label: the source label at floor(t + 0.5) inside, 0 outside.
 * Neither entry point allocates or synchronises; the caller guarantees that every descriptor tells the truth about its volume. */
#define MI355SEG_AUG_DESC_WORDS 64
size_t mi355seg_augment_ws_bytes(long long n);
int mi355seg_augment_stats_f32(const float* x, int C, int D, int H, int W, const float* bias_host, float sigma, long long seed,
                               float* stats, void* ws, size_t ws_bytes, void* stream);
int mi355seg_augment_sample_f32(const int* table, int count, int C, int Cy, int pd, int ph, int pw, float* out_x, float* out_y,
                                void* stream);

/* ------------------------------------------------------------------ Label-balanced patch sampling (tio.LabelSampler, dataloader.py:19)
 * config.sampler=label: where the queue cuts its patches is drawn from the label map instead of uniformly.  UNPINNED (torchio is
 * absent and the reference holds no fixture of its data pipeline): the definitions here are the specification.
 *   labels  y [1,D,H,W] = [D,H,W], fp32 holding integers (as the queue caches them); n = (D, H, W); patch p = (pd, ph, pw), p_d <= n_d
 *   origin  o is valid when 0 <= o_d <= n_d - p_d; its centre is c = o + p // 2 (torchio: crop_ini = p // 2, crop_fin = (p - 1) // 2,
 *           index_ini = centre - p // 2)
 *   region  R, the box of valid centres: extents m_d = n_d - p_d + 1, start p_d // 2.  The region-linear index of a voxel of R is
 *           e = (z * m_h + y) * m_w + x with (z, y, x) relative to R's start; the origin of the patch centred there is exactly (z, y, x)
 *   classes the integers 0 .. 15; count[l] = the number of voxels of R with label l; a voxel of R whose value is not an integer in
 *           [0, 16) (NaN and the infinities included) is counted in a 17th bin, bad = count[16].  Voxels outside R are never read.
 *   pick    (class l, rank r), 0 <= r < count[l]: the voxel of class l with rank r in region-linear order
 * The host turns two random draws into a pick from count[] (class masses: count[l] for l >= 1 and 0 for l = 0 without
 * label_probabilities; else w_l where count[l] > 0, renormalised); everything on the device is integer arithmetic, so a result is
 * exact, and without atomics equal inputs give bitwise equal outputs.
 * R is cut into chunks of MI355SEG_LABEL_CHUNK consecutive region-linear voxels (the last one ragged).
 * mi355seg_label_index_bytes: the size of the index of one (volume, patch) pair, chunks * 17 * 8 bytes (0 for bad arguments).
 * mi355seg_label_index_build_f32, once per (subject, patch size), two launches: one workgroup per chunk counts its 17 bins (wave
 * ballots), then one workgroup per bin turns the per-chunk counts into exclusive prefixes.  index: int64 [17][chunks] on the device,
 * index[l][k] = the number of voxels of class l in chunks 0 .. k-1; counts17: int64 [17] on the DEVICE, the totals count[0..15], bad.
 * mi355seg_label_index_select, one launch, one workgroup per pick: picks = int64 [n][2] (class, rank) on the device; binary search of
 * the rank in the class's prefixes, one re-read of that chunk, ballot prefix count; writes origins int32 [n][3] = (z, y, x).  The
 * select trusts class < 16 and rank < count[class] -- the caller holds the counts; for a pick outside that the origin is left
 * unwritten (no access leaves the index or the volume).  labels, geometry and index must be the ones of the build.
 * Bad arguments (null pointers, p_d > n_d, D*H*W >= 2^31, too small an index_bytes, n < 1) return an error code with
 * mi355seg_last_error.  Neither entry point allocates or synchronises. */
#define MI355SEG_LABEL_CHUNK 1024
#define MI355SEG_LABEL_BINS 17
size_t mi355seg_label_index_bytes(int D, int H, int W, int pd, int ph, int pw);
int mi355seg_label_index_build_f32(const float* labels, int D, int H, int W, int pd, int ph, int pw,
                                   void* index, size_t index_bytes, long long* counts17, void* stream);
int mi355seg_label_index_select(const float* labels, int D, int H, int W, int pd, int ph, int pw, const void* index,
                                const long long* picks, int n, int* origins, void* stream);

/* ------------------------------------------------------------------ Intensity normalisation (config.intensity; csrc/intensity.hip)
 * The reference's dataloader.py:19 imports RescaleIntensity and HistogramStandardization beside ZNormalization and wires neither in.
 * UNPINNED (torchio is absent and the reference holds no fixture of its data pipeline): the definitions here are the specification.
 *
 * mi355seg_percentiles_f32: np.percentile(v, q, method="linear") of the taking-part voxels v of one volume x[n] -- all finite voxels,
 * or with use_mask != 0 the finite voxels with x > mask_gt (the masks of tio.RescaleIntensity / ZNormalization / HistogramStandardization
 * are of that form).  With m = their number and s = sort(v): position pos = q / 100 * (m - 1) in fp64, lo = floor(pos),
 * hi = min(lo + 1, m - 1), t = pos - lo.  Outputs on the DEVICE: order fp32 [nq][2] = (s[lo], s[hi]), EXACT (voxel values; -0.0 is
 * reported as +0.0); values fp64 [nq] = s[lo] + (s[hi] - s[lo]) * t; counts int64 [2] = (m, the number of non-finite voxels of x,
 * masked or not).  q: nq doubles on the HOST.  Radix select, four 8-bit passes, integer counts only: exact, and equal inputs give
 * bitwise equal outputs.  Nine launches (one of them a memset), no synchronisation, no host round trip.  With m == 0 order and values
 * hold no information; m == 1 gives that voxel.  Refused before any launch: null pointers, n < 1, n >= 2^31, nq outside
 * 1 .. MI355SEG_PERCENTILES_MAX, a percentile outside 0 .. 100 (NaN included), a NaN mask_gt with use_mask, x not 16-byte aligned, a
 * workspace below mi355seg_percentiles_ws_bytes.
 *
 * The map (tio.RescaleIntensity, the clip + z-score and tio.HistogramStandardization's np.interp all are of this form): a continuous
 * piecewise-linear function with nk knots, 2 <= nk <= MI355SEG_INTENSITY_KNOTS_MAX, kx ascending (equal neighbours allowed):
 *   x' = min(max(x, clip_lo), clip_hi);  j = the number of interior knots kx[1 .. nk-2] that are <= x';
 *   y  = fmaf(x' - kx[j], slope[j], ky[j])                 (fp32; the subtraction rounds once, the multiply-add is fused)
 * so the first and the last segment extrapolate; clip_lo = -inf / clip_hi = +inf switch the clamp off.  kx[nk], ky[nk], slope[nk-1]
 * are HOST arrays (computed by the caller in fp64, passed as fp32).
 * mi355seg_intensity_map_f32: y[i] = map(x[i]) for all n voxels in one streaming pass; y == x allowed.
 * mi355seg_intensity_moments_f32: over the voxels with x > mask_gt (the RAW x; all voxels with use_mask == 0), with d = map(x) - pivot
 * in fp64: out fp64 [4] on the DEVICE = (count, pivot + sum d / count, (sum d^2 - (sum d)^2 / count) / (count - 1), sum d) -- the
 * count, the mean and the unbiased variance of the mapped voxels (variance NaN below two voxels; mean = pivot for none).  pivot: any
 * value near the data, as znorm pivots on x[0].  Block partials in a fixed order and a one-block finalise: no atomics, bitwise
 * reproducible.  Two launches.
 * Both refuse before any launch: null pointers, n < 1, nk outside 2 .. 12, descending knots, a NaN knot / value / slope / pivot /
 * mask_gt, clip_lo > clip_hi (NaN included), pointers not 16-byte aligned, a workspace below mi355seg_intensity_moments_ws_bytes. */
#define MI355SEG_PERCENTILES_MAX 16
#define MI355SEG_INTENSITY_KNOTS_MAX 12
size_t mi355seg_percentiles_ws_bytes(long long n);
int mi355seg_percentiles_f32(const float* x, long long n, const double* q, int nq, int use_mask, float mask_gt,
                             double* values, float* order, long long* counts, void* ws, size_t ws_bytes, void* stream);
size_t mi355seg_intensity_moments_ws_bytes(long long n);
int mi355seg_intensity_moments_f32(const float* x, long long n, const float* kx, const float* ky, const float* slope, int nk,
                                   float clip_lo, float clip_hi, int use_mask, float mask_gt, double pivot, double* out,
                                   void* ws, size_t ws_bytes, void* stream);
int mi355seg_intensity_map_f32(const float* x, long long n, const float* kx, const float* ky, const float* slope, int nk,
                               float clip_lo, float clip_hi, float* y, void* stream);

/* ------------------------------------------------------------------ Resampling to a target voxel spacing (config.resample_spacing; csrc/resample.hip)
 * The reference's dataloader.py:10 imports tio.Resample and never wires it in.  UNPINNED (torchio and SimpleITK are absent and the
 * reference holds no fixture of its data pipeline): the definitions here are the specification, scipy.ndimage in fp64 the oracle.
 *
 * Geometry: axis-aligned and corner-aligned, per axis independently.  With input spacing s, target spacing t, input length n and
 * r = t / s: output length n' = max(1, ceil(n * s / t - 1e-6)); output index o reads the input coordinate
 * c(o) = clamp((o + 0.5) * r - 0.5, 0, n - 1).  The way back uses r = s / t and is GIVEN its output length.  The caller forms one
 * table per axis in fp64 (functional.resample_axis_table) and packs them z, y, x: `base` int32 [Do + Ho + Wo] and `frac` fp32
 * [Do + Ho + Wo] on the device, `base_host` the host copy of `base`.  Order 0: base = floor(c + 0.5) (half up), frac unused (may be
 * NULL).  Orders 1 and 3: base = floor(c), frac = c - base.  No coordinate arithmetic happens on the device.  The wrappers validate
 * `base_host` (the kernels trust `base` to hold the same numbers): 0 <= base < n on every axis, and for order 3 ascending per axis.
 *
 * mi355seg_bspline3_prefilter_f32: x [C,D,H,W] -> cubic B-spline coefficients y [C,D,H,W], scipy.ndimage.spline_filter(order=3,
 * mode='mirror') per channel: along W, then H, then D the recursive filter with pole z = sqrt(3) - 2, gain 6 and a
 * whole-sample-symmetric boundary; per line s[0 .. n-1]
 *   c+[0] = g0 * sum_{k < K} z^k s[m(k)],   c+[i] = z c+[i-1] + 6 s[i],
 *   c[n-1] = (z c+[n-2] + c+[n-1]) * z / (z^2 - 1),   c[i] = z * (c[i+1] - c+[i])
 * (the running value of both recursions is a pair of floats, value + rounding residual, all fp32 arithmetic; the residuals of c+ wait
 * in the workspace, one float per element: ws >= mi355seg_bspline3_prefilter_ws_bytes) where for n >= MI355SEG_BSPLINE_INIT_TERMS the sum is truncated, K = 14, g0 = 6 (|z|^14 < 2^-25), and below that it is the exact
 * mirrored period: K = 2n - 2, m(k) = k < n ? k : 2n - 2 - k, g0 = 6 / (1 - z^(2n-2)).  An axis of length 1 is the identity.  No
 * bound on any axis: lines along W go through LDS in chunks of 64 columns with the causal carry passed on in order.  fp32, FMA
 * in a fixed order: equal inputs give bitwise equal outputs; y == x allowed, with bitwise the same result.  Up to three launches.
 * mi355seg_bspline3_prefilter_axis_f32: ONE of the three passes (axis 0 = D, 1 = H, 2 = W; its length must be at least 2); the three
 * in the order 2, 1, 0 are mi355seg_bspline3_prefilter_f32 bitwise.
 * Both refuse: null or misaligned pointers, non-positive sizes, 2^31 elements or more, an axis outside 0 .. 2 or of length 1, a
 * workspace too small.
 *
 * mi355seg_resample3d_f32: x [C,D,H,W] -> y [C,Do,Ho,Wo] in one launch.
 *   order 0: y = x[base_z, base_y, base_x], exact.
 *   order 1: trilinear over the corners (base, min(base + 1, n - 1)) per axis: corner weight (wz * wy) * wx with w = (1 - frac, frac),
 *            summed by an FMA chain in the corner order zyx = 000, 001, ... 111.
 *   order 3: x must hold the COEFFICIENTS of mi355seg_bspline3_prefilter_f32.  Taps base - 1 .. base + 2 per axis, mirrored into the
 *            source (whole-sample symmetric), weights of t = frac: ((1-t)^3 / 6, t^2 (t/2 - 1) + 2/3, (1-t)^2 ((1-t)/2 - 1) + 2/3,
 *            t^3 / 6), formed in fp64 from the fp32 fraction and used as pairs of floats; the sum is nested x, then y, then z,
 *            every level carrying its rounding errors along (a pair of floats, fp32 arithmetic).  With the prefilter this is
 *            scipy.ndimage.map_coordinates(order=3, mode='mirror') on the clamped coordinates.
 * Refused: an order outside {0, 1, 3}, null or misaligned pointers (frac may be NULL at order 0), y == x, non-positive sizes, 2^31
 * elements or more on either side, a base outside the source, a descending table at order 3.
 *
 * mi355seg_resample3d_labels_f32 / _i64: label volumes (fp32 holding integers, or int64) [C,D,H,W] -> [C,Do,Ho,Wo].
 *   MI355SEG_RESAMPLE_LABELS_NEAREST: the order-0 table, tio.Resample's rule for label maps.
 *   MI355SEG_RESAMPLE_LABELS_LINEAR: the order-1 table; the weight of class k is the sum of the corner weights (as order 1 above)
 *   whose corner holds k, added in the corner order; the class of largest weight wins, the LOWEST class on a tie -- the argmax of the
 *   trilinearly resampled one-hot volume (nnU-Net's way) in one pass, without that volume.
 * bad[0] (int64, device): the number of output voxels that read a value that is no integer in 0 .. 15; such a value takes part as
 * itself.  Block partials in a fixed order and a one-block finalise: no atomics.  Two launches; ws >= mi355seg_resample3d_labels_ws_bytes.
 * Refused: a mode outside {0, 1}, what mi355seg_resample3d_f32 refuses, a null `bad` or workspace, a workspace too small.
 *
 * mi355seg_resample3d_argmax_f32: the way back of a blending mode.  prob [K,D,H,W] (class probabilities or logits on the resampled
 * grid), the order-1 tables -> labels int64 [Do,Ho,Wo]: per class the order-1 value above, the first maximum wins (lowest class on
 * ties, class 0 if nothing compares greater); prob_out, when not NULL, receives the K interpolated volumes [K,Do,Ho,Wo], and the
 * labels are bitwise the same with and without it.  One launch.  Refused: K outside 1 .. MI355SEG_RESAMPLE_MAX_CLASSES, and what
 * order 1 of mi355seg_resample3d_f32 refuses. */
#define MI355SEG_BSPLINE_INIT_TERMS 14
#define MI355SEG_RESAMPLE_MAX_CLASSES 16
#define MI355SEG_RESAMPLE_LABELS_NEAREST 0
#define MI355SEG_RESAMPLE_LABELS_LINEAR 1
size_t mi355seg_bspline3_prefilter_ws_bytes(int C, int D, int H, int W);
int mi355seg_bspline3_prefilter_f32(const float* x, int C, int D, int H, int W, float* y, void* ws, size_t ws_bytes, void* stream);
int mi355seg_bspline3_prefilter_axis_f32(const float* x, int C, int D, int H, int W, int axis, float* y, void* ws, size_t ws_bytes, void* stream);
int mi355seg_resample3d_f32(const float* x, int C, int D, int H, int W, int order, const int* base, const float* frac, const int* base_host,
                            float* y, int Do, int Ho, int Wo, void* stream);
size_t mi355seg_resample3d_labels_ws_bytes(void);
int mi355seg_resample3d_labels_f32(const float* x, int C, int D, int H, int W, int mode, const int* base, const float* frac, const int* base_host,
                                   float* y, int Do, int Ho, int Wo, long long* bad, void* ws, size_t ws_bytes, void* stream);
int mi355seg_resample3d_labels_i64(const long long* x, int C, int D, int H, int W, int mode, const int* base, const float* frac, const int* base_host,
                                   long long* y, int Do, int Ho, int Wo, long long* bad, void* ws, size_t ws_bytes, void* stream);
int mi355seg_resample3d_argmax_f32(const float* prob, int K, int D, int H, int W, const int* base, const float* frac, const int* base_host,
                                   long long* labels, float* prob_out, int Do, int Ho, int Wo, void* stream);

/* ------------------------------------------------------------------ Frequency-band split of the IS network (train.py:76-88,198-201)
 * low_pass_torch / high_pass_torch at `limit`: the reference masks the spectrum of x [B,C,D,H,W] on its last two axes with the outer
 * product of (|fftfreq(H)| < limit, |rfftfreq(W)| < limit) for the low band and of the two `> limit` masks for the high band.  Per
 * [H,W] slice X that is
 *   low = P_H X P_W          high = (I - E_H) X (I - E_W)          (high is NOT x - low: the cross terms are dropped, as upstream)
 * with P_n the orthogonal projector onto the real Fourier modes of length n with |f| < limit and E_n the one onto the modes that are
 * not > limit (the low modes plus any mode exactly at the limit; membership is the reference's own float32 comparison, which the
 * CALLER evaluates).  The caller passes orthonormal basis rows basis_h [qH,H] and basis_w [qW,W] whose first rH / rW rows span P:
 * per kept mode k, 1/sqrt(n) for k = 0, (-1)^j/sqrt(n) for 2k = n, else the pair sqrt(2/n) cos(2 pi k j / n), sqrt(2/n) sin(2 pi k j / n).
 * With U = X Ew^T, V = Eh X, A = Eh U:  low = Eh[:r]^T A[:r,:r] Ew[:r],  high = X - Eh^T V - U Ew + Eh^T A Ew.
 * Upstream quirk, kept: the forward transform also covers the batch and channel axes and is never inverted there, so for B = 2
 * (C = 2 likewise, independently) slice 0 filters x0 + x1 and slice 1 filters x0 - x1; longer axes are backend-defined upstream and
 * refused here.  Supported: B, C in {1, 2}, D >= 1, 1 <= H, W <= 256, 0 <= r <= q <= min(n, 32).
 * One launch, one workgroup per output slice, fixed-order fp32 sums and no atomics (bitwise reproducible); neither allocates nor
 * synchronises.  mi355seg_band_split_supported: 0 for an unsupported shape, else the number of row chunks a slice is staged in
 * (1: the slice stays in LDS between the two passes; more: the second pass re-reads it). */
int mi355seg_band_split_supported(int B, int C, int D, int H, int W, int rH, int qH, int rW, int qW);
int mi355seg_band_split_f32(const float* x, int B, int C, int D, int H, int W, const float* basis_h, int rH, int qH,
                            const float* basis_w, int rW, int qW, float* low, float* high, void* stream);

/* ------------------------------------------------------------------ Layout helpers */
int mi355seg_ncdhw_to_ndhwc_f32(const float* src, float* dst, int lddst, long long N, int C, long long S, void* stream);
int mi355seg_ndhwc_to_ncdhw_f32(const float* src, int ldsrc, float* dst, long long N, int C, long long S, void* stream);
/* strided channel-slice copy: dst[r, 0:C] = src[r, 0:C] */
int mi355seg_copy_rows_f32(const float* src, int ldsrc, float* dst, int lddst, long long rows, int C, void* stream);
/* dst[r, 0:C] += src[r, 0:C] */
int mi355seg_add_rows_f32(const float* src, int ldsrc, float* dst, int lddst, long long rows, int C, void* stream);
/* x.repeat(1, rep, 1, 1, 1) in channel-last form (vnet3d.py:55-56): y[r, j*C + c] = x[r, c], and its adjoint
 * dx[r, c] = sum_j dy[r, j*C + c]. */
int mi355seg_repeat_channels_f32(const float* x, int ldx, float* y, int ldy, long long rows, int C, int rep, void* stream);
int mi355seg_repeat_channels_bwd_f32(const float* dy, int lddy, float* dx, int lddx, long long rows, int C, int rep, void* stream);
/* Reverse-attention gate of RE_Net / ER_Net (RE_net.py:104-107,114-117,123-126):
 *   y[r, c] = enc[r, c] * (2 - sigmoid(t[r]))        (= (1 - sigmoid(t)).expand(C) * enc + enc; t has one channel)
 * backward: denc[r, c] = dy[r, c] * (2 - s_r),  dt[r] = -s_r (1 - s_r) * sum_c dy[r, c] enc[r, c].   C % 4 == 0. */
int mi355seg_gate_fwd_f32(const float* enc, int ldenc, const float* t, int ldt, float* y, int ldy, long long rows, int C, void* stream);
int mi355seg_gate_bwd_f32(const float* dy, int lddy, const float* enc, int ldenc, const float* t, int ldt,
                          float* denc, int lddenc, float* dt, long long rows, int C, void* stream);
/* Selective-fusion pieces of ER_Net's SFConv (ER_net.py:36-70); rows are grouped per sample (group g = rows [g*rows, (g+1)*rows)):
 *   group_sums:         out[g, c] (+)= alpha * sum_r x[g, r, c]           (fea_U.mean over the voxels; adjoint of the mix)
 *   mix_channels:       y[g, r, c] = x1[g, r, c] * a[g, c] + x2[g, r, c] * b[g, c]   ((feas * attention_vectors).sum(dim=1))
 *   broadcast_channels: y[g, r, c] = alpha * v[g, c]                      (adjoint of the spatial mean)
 * group_sums needs mi355seg_norm_ws_bytes(rows, 1, C) of workspace. */
int mi355seg_group_sums_f32(const float* x, int ldx, long long rows, int groups, int C, float alpha, float* out, int accumulate,
                            void* ws, size_t ws_bytes, void* stream);
int mi355seg_mix_channels_f32(const float* x1, int ld1, const float* a, const float* x2, int ld2, const float* b, float* y, int ldy,
                              long long rows, int groups, int C, void* stream);
int mi355seg_broadcast_channels_f32(const float* v, float alpha, float* y, int ldy, long long rows, int groups, int C, void* stream);
/* y[r, c] += bias[c] in place (bias of a ConvTranspose3d computed as the adjoint of a bias-free convolution). */
int mi355seg_add_bias_f32(float* y, int ldy, const float* bias, long long rows, int C, void* stream);
/* out[i] = a[i] * b[i] (attention-probability dropout mask, unetr.py:112; out may alias a). */
int mi355seg_mul_f32(const float* a, const float* b, float* out, long long n, void* stream);


/* ------------------------------------------------------------------ bf16 tensors (BASELINE cfg 3-5: V-Net / Residual U-Net / UNETR in bf16)
 * What torch autocast(bfloat16) does for the reference's modules (vnet3d.py:21-121, residual_unet3d.py:82-107,
 * unetr.py:8-51): activations and activation gradients are bf16 NDHWC tensors in HBM, parameters, parameter gradients,
 * norm statistics and the loss stay fp32, every convolution product is a bf16 MFMA with fp32 accumulation, every
 * elementwise / norm / pool kernel loads bf16, computes in fp32 registers and rounds once (RNE) on the store.
 * Each mi355seg_<op>_bf16 below has the contract of mi355seg_<op>_f32 above with the tensor pointers retyped; pitches
 * (ld*) count ELEMENTS.  Conv3d shapes without a native bf16 kernel run through the fp32 entry point on fp32 copies
 * made in the workspace (mi355seg_conv3d_ws_bytes_bf16 sizes for that). */
int mi355seg_norm_stats_bf16(const mi355seg_bf16* x, int ldx, long long rows, int groups, int C, float eps, float* mean, float* rstd, float* running_mean, float* running_var, float momentum, void* ws, size_t ws_bytes, void* stream);
int mi355seg_norm_act_fwd_ax_bf16(const mi355seg_bf16* x, int ldx, const float* mean, const float* rstd, const float* gamma, const float* beta, const mi355seg_bf16* res, int ldres, mi355seg_bf16* y, int ldy, long long rows, int groups, int C, int act, float slope, float* y_amax, void* stream);
int mi355seg_norm_act_bwd_colsum_ax_bf16(const mi355seg_bf16* dy, int lddy, const mi355seg_bf16* x, int ldx, const float* mean, const float* rstd, const float* gamma, const float* beta, const mi355seg_bf16* res, int ldres, mi355seg_bf16* dx, int lddx, float* dgamma, float* dbeta, mi355seg_bf16* dres, int lddres, float* dx_colsum, float* dx_amax, long long rows, int groups, int C, int act, float slope, void* ws, size_t ws_bytes, void* stream);
int mi355seg_norm_act_bwd_apply_ax_bf16(const mi355seg_bf16* dy, int lddy, const mi355seg_bf16* x, int ldx, const float* mean, const float* rstd, const float* gamma, const float* beta, const mi355seg_bf16* res, int ldres, const float* s1, const float* s2, mi355seg_bf16* dx, int lddx, mi355seg_bf16* dres, int lddres, float* dx_colsum, float* dx_amax, long long rows, int groups, int C, int act, float slope, void* ws, size_t ws_bytes, void* stream);
int mi355seg_norm_act_fwd_bf16(const mi355seg_bf16* x, int ldx, const float* mean, const float* rstd, const float* gamma, const float* beta, const mi355seg_bf16* res, int ldres, mi355seg_bf16* y, int ldy, long long rows, int groups, int C, int act, float slope, void* stream);
int mi355seg_norm_act_bwd_bf16(const mi355seg_bf16* dy, int lddy, const mi355seg_bf16* x, int ldx, const float* mean, const float* rstd, const float* gamma, const float* beta, const mi355seg_bf16* res, int ldres, mi355seg_bf16* dx, int lddx, float* dgamma, float* dbeta, mi355seg_bf16* dres, int lddres, long long rows, int groups, int C, int act, float slope, void* ws, size_t ws_bytes, void* stream);
int mi355seg_norm_act_bwd_colsum_bf16(const mi355seg_bf16* dy, int lddy, const mi355seg_bf16* x, int ldx, const float* mean, const float* rstd, const float* gamma, const float* beta, const mi355seg_bf16* res, int ldres, mi355seg_bf16* dx, int lddx, float* dgamma, float* dbeta, mi355seg_bf16* dres, int lddres, float* dx_colsum, long long rows, int groups, int C, int act, float slope, void* ws, size_t ws_bytes, void* stream);
int mi355seg_norm_act_bwd_sums_bf16(const mi355seg_bf16* dy, int lddy, const mi355seg_bf16* x, int ldx, const float* mean, const float* rstd, const float* gamma, const float* beta, const mi355seg_bf16* res, int ldres, float* s1, float* s2, float* dgamma, float* dbeta, long long rows, int groups, int C, int act, float slope, void* ws, size_t ws_bytes, void* stream);
int mi355seg_norm_act_bwd_apply_bf16(const mi355seg_bf16* dy, int lddy, const mi355seg_bf16* x, int ldx, const float* mean, const float* rstd, const float* gamma, const float* beta, const mi355seg_bf16* res, int ldres, const float* s1, const float* s2, mi355seg_bf16* dx, int lddx, mi355seg_bf16* dres, int lddres, float* dx_colsum, long long rows, int groups, int C, int act, float slope, void* ws, size_t ws_bytes, void* stream);
int mi355seg_scale_channels_bf16(const mi355seg_bf16* x, int ldx, const float* scale, mi355seg_bf16* y, int ldy, long long rows, int groups, int C, void* stream);
int mi355seg_act_fwd_bf16(const mi355seg_bf16* x, int ldx, const mi355seg_bf16* res, int ldres, mi355seg_bf16* y, int ldy, long long rows, int C, int act, float slope, void* stream);
int mi355seg_act_bwd_add_bf16(const mi355seg_bf16* dy, int lddy, const mi355seg_bf16* x, int ldx, const mi355seg_bf16* res, int ldres, const mi355seg_bf16* addend, int ldadd, mi355seg_bf16* dx, int lddx, long long rows, int C, int act, float slope, void* stream);
int mi355seg_act_bwd_bf16(const mi355seg_bf16* dy, int lddy, const mi355seg_bf16* x, int ldx, const mi355seg_bf16* res, int ldres, mi355seg_bf16* dx, int lddx, long long rows, int C, int act, float slope, void* stream);
int mi355seg_prelu_fwd_bf16(const mi355seg_bf16* x, int ldx, const mi355seg_bf16* res, int ldres, const float* slope, mi355seg_bf16* y, int ldy, long long rows, int C, void* stream);
int mi355seg_prelu_bwd_bf16(const mi355seg_bf16* dy, int lddy, const mi355seg_bf16* x, int ldx, const mi355seg_bf16* res, int ldres, const float* slope, mi355seg_bf16* dx, int lddx, float* dslope, long long rows, int C, void* ws, size_t ws_bytes, void* stream);
int mi355seg_maxpool2_fwd_bf16(const mi355seg_bf16* x, int ldx, mi355seg_bf16* y, int ldy, uint8_t* idx, int N, int D, int H, int W, int C, void* stream);
int mi355seg_maxpool2_bwd_bf16(const mi355seg_bf16* dy, int lddy, const uint8_t* idx, mi355seg_bf16* dx, int lddx, int N, int D, int H, int W, int C, void* stream);
int mi355seg_maxpool2_bwd_add_bf16(const mi355seg_bf16* dy, int lddy, const uint8_t* idx, const mi355seg_bf16* add, int ldadd, mi355seg_bf16* dx, int lddx, int N, int D, int H, int W, int C, void* stream);
int mi355seg_upsample2_fwd_bf16(const mi355seg_bf16* x, int ldx, mi355seg_bf16* y, int ldy, int N, int D, int H, int W, int C, void* stream);
int mi355seg_upsample2_bwd_bf16(const mi355seg_bf16* dy, int lddy, mi355seg_bf16* dx, int lddx, int N, int D, int H, int W, int C, void* stream);
int mi355seg_convt3d_k2s2_fwd_ax_bf16(const mi355seg_bf16* x, int ldx, const float* w, const float* bias, mi355seg_bf16* y, int ldy, int N, int D, int H, int W, int Cin, int Cout, float* y_amax, void* ws, size_t ws_bytes, void* stream);
int mi355seg_convt3d_k2s2_fwd_bf16(const mi355seg_bf16* x, int ldx, const float* w, const float* bias, mi355seg_bf16* y, int ldy, int N, int D, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
int mi355seg_convt3d_k2s2_dgrad_bf16(const mi355seg_bf16* dy, int lddy, const float* w, mi355seg_bf16* dx, int lddx, int N, int D, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
int mi355seg_convt3d_k2s2_wgrad_bf16(const mi355seg_bf16* dy, int lddy, const mi355seg_bf16* x, int ldx, float* dw, float* db, int N, int D, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
int mi355seg_ncdhw_f32_to_ndhwc_bf16(const float* src, mi355seg_bf16* dst, int lddst, long long N, int C, long long S, void* stream);
int mi355seg_ndhwc_bf16_to_ncdhw_f32(const mi355seg_bf16* src, int ldsrc, float* dst, long long N, int C, long long S, void* stream);
int mi355seg_copy_rows_bf16(const mi355seg_bf16* src, int ldsrc, mi355seg_bf16* dst, int lddst, long long rows, int C, void* stream);
int mi355seg_add_rows_bf16(const mi355seg_bf16* src, int ldsrc, mi355seg_bf16* dst, int lddst, long long rows, int C, void* stream);
int mi355seg_repeat_channels_bf16(const mi355seg_bf16* x, int ldx, mi355seg_bf16* y, int ldy, long long rows, int C, int rep, void* stream);
int mi355seg_repeat_channels_bwd_bf16(const mi355seg_bf16* dy, int lddy, mi355seg_bf16* dx, int lddx, long long rows, int C, int rep, void* stream);
int mi355seg_add_bias_bf16(mi355seg_bf16* y, int ldy, const float* bias, long long rows, int C, void* stream);
size_t mi355seg_conv3d_ws_bytes_bf16(int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad);
int mi355seg_conv3d_fwd_bf16(const mi355seg_bf16* x, int ldx, const float* w, const float* bias, mi355seg_bf16* y, int ldy, int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad, double* stats_sum, double* stats_sq, void* ws, size_t ws_bytes, void* stream);
/* y = conv(x) + res on bf16 tensors, each of the two operations rounded to bf16 as the reference's `conv(...) + residual` under autocast
 * (/root/reference/models/three_d/residual_unet3d.py:121,140-168): the sum rides in the convolution's epilogue where the launch allows
 * (k3 / k5 s1 on the 16x16x32 tiles, whole-K), else the library adds it in place after the convolution.  res: y's geometry at pitch ldres. */
int mi355seg_conv3d_fwd_res_bf16(const mi355seg_bf16* x, int ldx, const float* w, const float* bias, const mi355seg_bf16* res, int ldres, mi355seg_bf16* y, int ldy, int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad, void* ws, size_t ws_bytes, void* stream);
int mi355seg_conv3d_dgrad_bf16(const mi355seg_bf16* dy, int lddy, const float* w, mi355seg_bf16* dx, int lddx, int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad, void* ws, size_t ws_bytes, void* stream);
/* dx = conv3d_dgrad(dy) + res on bf16 tensors (r5): a convolution's input gradient together with the sum of a SECOND gradient of its input --
 * the residual blocks of /root/reference/models/three_d/vnet3d.py:61-104 (`down` / the concat feed the first k5 unit AND the block's final
 * sum) -- each of the two operations rounded to bf16 as autograd's own sum of the two gradients would be (bit-identical to
 * mi355seg_conv3d_dgrad_bf16 followed by the sum); in the input-gradient kernel's epilogue on the 16x16x32 tiles, in place after it elsewhere. */
int mi355seg_conv3d_dgrad_res_bf16(const mi355seg_bf16* dy, int lddy, const float* w, const mi355seg_bf16* res, int ldres, mi355seg_bf16* dx, int lddx, int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad, void* ws, size_t ws_bytes, void* stream);
int mi355seg_conv3d_wgrad_bf16(const mi355seg_bf16* dy, int lddy, const mi355seg_bf16* x, int ldx, float* dw, float* db, int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad, int accumulate, void* ws, size_t ws_bytes, void* stream);
int mi355seg_cast_f32_to_bf16(const float* src, int ldsrc, mi355seg_bf16* dst, int lddst, long long rows, int C, void* stream);
int mi355seg_cast_bf16_to_f32(const mi355seg_bf16* src, int ldsrc, float* dst, int lddst, long long rows, int C, void* stream);

/* ---- every weight packing of a training step in ONE launch (r6; csrc/prepack.hip).  Every matrix-core convolution reads its fp32 master
 * weights (the reference's nn.Conv3d / nn.ConvTranspose3d parameters, /root/reference/models/three_d/unet3d.py:29-43,80-101) in a
 * packed form that its entry point builds right in front of the launch: 44 small launches per cfg-2 step.  A training step can have
 * them built all at once instead:
 *   record_begin ... one full step through the ordinary entry points ... record_end  -> plan id + arena size (once per model and shape);
 *   each later step: prepack_run(plan, arena, bytes, stream) at its top -- one memset, one launch measuring max |w| where a packing scales
 *   by it (f16x3) and ONE launch that forms every recorded packing in the caller's arena, all on `stream`; until prepack_done an entry
 *   point that finds its (weight pointer, layout) in the plan reads the arena copy and launches no packing of its own.
 * Anything not found packs as before; results are bit-identical either way.  A plan keeps only the packings of weights that lie inside
 * the caller's parameter storage: record_end takes it as nparams host arrays of base pointers and byte counts (the model's parameters)
 * and drops every recorded weight pointer outside them (a contiguous copy, a weight computed in the forward: freed by the next step).
 * The caller guarantees that those parameters stay alive while the plan exists and that the weights do not change between
 * prepack_run and their last use in the step.  (The first prepack_run
 * with an arena writes the job table into it with a blocking copy; called first inside a stream capture it leaves the plan inactive.)
 * These seven entry points share ONE bracket per process -- a recording (record_begin .. record_end) or a replay (prepack_run ..
 * prepack_done), whichever threads run the step inside it -- and serialise on one lock.  A record_begin or prepack_run while a bracket
 * is open fails with MI355SEG_EINVAL, names the open bracket in mi355seg_last_error() and leaves it intact. */
int mi355seg_prepack_record_begin(void);
int mi355seg_prepack_record_end(int* plan, size_t* arena_bytes, const void* const* param_base_host, const size_t* param_bytes_host, int nparams);
int mi355seg_prepack_jobs(int plan);
int mi355seg_prepack_run(int plan, void* arena, size_t arena_bytes, void* stream);
int mi355seg_prepack_done(void* stream);
int mi355seg_prepack_active(void);      /* != 0 between a prepack_run that activated its plan and prepack_done */
int mi355seg_prepack_free(int plan);

#ifdef __cplusplus
}
#endif
#endif /* MI355SEG_H */
