// conv_bf16_api.hip -- Conv3d forward / input gradient / weight gradient on bf16 NDHWC tensors (the bf16 configurations:
// V-Net vnet3d.py:21-121, Residual U-Net residual_unet3d.py:22-107, UNETR decoder unetr.py:8-51).  Activations and
// activation gradients are bf16 in HBM, weights / bias / weight gradients stay fp32 masters (what torch autocast does for
// the reference), every product is a bf16 MFMA with fp32 accumulation.
//
// Native bf16 kernels: the implicit-GEMM kernel (k1 / k3 / k5 stride 1, gather mode for strided / even kernels), the
// transposing-read wgrad (k3 / k5), the K = voxels wgrads (k1, any-geometry gather wgrad: bf16 loads, fp32 MFMA) and the
// HBM-bound small-channel stems / heads.  Any other shape (V-Net's two-channel k5 head and one-channel k5 stem, tiny
// or ragged channel counts) runs through the fp32 entry point on fp32 copies made in the workspace: one extra read +
// write of tensors that are a few channels wide -- correct for every geometry, never the hot layers.
#include "common.h"
#include "internal.h"
#include "igemm_kernel.h"

namespace seg {

template <typename TS, typename TD>
__global__ __launch_bounds__(256) void cast_rows_kernel(const TS* __restrict__ src, int lds, TD* __restrict__ dst, int ldd, long long rows, int C) {
    const bool v = (C % 4 == 0) && (lds % 4 == 0) && (ldd % 4 == 0) && ((uintptr_t)src % (4 * sizeof(TS)) == 0) && ((uintptr_t)dst % (4 * sizeof(TD)) == 0);
    const int cw = v ? C / 4 : C;
    const long long total = rows * cw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / cw;
        const int c = (int)(i - r * cw);
        if (v) st4(dst + r * ldd + c * 4, ld4(src + r * lds + c * 4));
        else st1(dst + r * ldd + c, ld1(src + r * lds + c));
    }
}

template <typename TS, typename TD>
static void cast_rows(const TS* src, int lds, TD* dst, int ldd, long long rows, int C, hipStream_t st) {
    long long b = (rows * C / 4 + 255) / 256;
    const int grid = (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
    hipLaunchKernelGGL((cast_rows_kernel<TS, TD>), dim3(grid), dim3(256), 0, st, src, lds, dst, ldd, rows, C);
}

// ---- the three bf16 choosers.  Families of native kernels, NB_CAST = the fp32 entry point on fp32 copies staged in the workspace.
// Unlike the fp32 ladders (conv_generic.hip), the FIRST rung that fits the geometry and pitches owns the call: its kernel runs if `aligned`
// (the launcher's demands on the addresses modulo 16 -- ax: x or dx, ay: y or dy -- and on accumulate) holds too, else the `demote` rung's if
// that one fits and is aligned, else the cast fall-back -- never a family further down.
enum { NB_CAST = 0, NB_IGEMM, NB_GATHER, NB_STEM1K5, NB_PWL, NB_HEADPW, NB_K2S2W, NB_HEAD2, NB_STEM4, NB_STEM, NB_HEAD, NB_LOWP, NB_PW, NB_SMALLCIN, NB_SMALLCOUT, NB_GW, NB_TINY, NB_CONVT };
static bool k2s2(const ConvGeom& g) { return g.k == 2 && g.stride == 2 && g.pad == 0; }
static bool k2s2_even(const ConvGeom& g) { return k2s2(g) && g.D % 2 == 0 && g.H % 2 == 0 && g.W % 2 == 0; }
static bool al16(const ConvKey& k) { return k.ax == 0 && k.ay == 0; }
static bool al8(const ConvKey& k) { return k.ax % 8 == 0 && k.ay % 8 == 0; }
static size_t ws_head2(const ConvGeom& g) { return head2_lowp_ws_bytes(g.Cin); }
static size_t ws_stem1k5(const ConvGeom& g) { return stem1k5_lowp_ws_bytes(g.Cout); }
static size_t ws_stem4(const ConvGeom& g) { return stem4_lowp_ws_bytes(g.Cout); }
static size_t ws_headpw(const ConvGeom& g) { return headpw_lowp_ws_bytes(g.Cin, g.Cout); }
// (rungs without a `ws`: kernels shared with the fp32 ladders, whose terms the bf16 query starts from)
static const Rung FWD_B16[] = {
    {NB_IGEMM, RUNG(conv_mfma_supported(MATH_B16, GEOM9(g), k.ldx, k.ldy)), nullptr, nullptr, RUNG(k.ax == 0)},
    {NB_GATHER, RUNG(conv_gather_fwd_supported(MATH_B16, GEOM9(g), k.ldx, k.ldy)), nullptr, nullptr, RUNG(k.ax == 0)},
    {NB_HEAD2, RUNG(head2_lowp_supported(SHAPE5(g), k.ldx, k.ldy)), ws_head2, nullptr, RUNG(k.ax == 0 && k.ay % 4 == 0)},
    {NB_STEM1K5, RUNG(stem1k5_lowp_supported(SHAPE5(g), k.ldx, k.ldy)), ws_stem1k5, nullptr, RUNG(k.ay % 8 == 0)},
    {NB_STEM4, RUNG(stem4_lowp_supported(SHAPE5(g), k.ldx, k.ldy)), ws_stem4, nullptr, al8, NB_STEM},
    {NB_STEM, RUNG(stem_supported(SHAPE5(g), k.ldy)), nullptr, nullptr, RUNG(k.ay % 8 == 0)},
    {NB_HEADPW, RUNG(headpw_lowp_supported(SHAPE5(g), k.ldx, k.ldy)), ws_headpw, nullptr, RUNG(k.ax == 0 && k.ay % (2 * g.Cout) == 0), NB_HEAD},
    {NB_HEAD, RUNG(head_supported(SHAPE5(g), k.ldx)), nullptr, nullptr, RUNG(k.ax % 8 == 0)},
    {NB_TINY, RUNG(tinypw_supported(SHAPE5(g)))},
    {NB_CAST}};
static const Rung DGRAD_B16[] = {
    {NB_IGEMM, RUNG(conv_mfma_supported(MATH_B16, GEOM9_T(g), k.ldy, k.ldx)), nullptr, nullptr, RUNG(k.ay == 0)},
    {NB_GATHER, RUNG(conv_gather_dgrad_supported(MATH_B16, GEOM9(g), k.ldy, k.ldx)), nullptr, nullptr, RUNG(k.ay == 0)},
    {NB_HEAD2, RUNG(head2_lowp_supported(SHAPE5(g), k.ldx, k.ldy)), ws_head2, nullptr, RUNG(k.ay % 4 == 0 && k.ax % 8 == 0)},
    {NB_HEAD, RUNG(head_supported(SHAPE5(g), k.ldx)), nullptr, nullptr, RUNG(k.ax % 8 == 0)},
    {NB_TINY, RUNG(tinypw_supported(SHAPE5(g)))},
    // k2 s2 p0: the input gradient is the forward of ConvTranspose3d k2 s2 with the same weight tensor (conv_generic.hip)
    {NB_CONVT, RUNG(k2s2_even(g) && convt_mfma_supported(MATH_B16, g.N, g.D / 2, g.H / 2, g.W / 2, g.Cout, g.Cin, k.ldy, k.ldx)), nullptr, nullptr, RUNG(k.ay == 0)},
    {NB_CAST}};
static const Rung WGRAD_B16[] = {
    {NB_LOWP, RUNG(wgrad_lowp_supported(MATH_B16, GEOM9(g), k.ldx, k.ldy)), nullptr, nullptr, al16},
    {NB_HEAD2, RUNG(head2_lowp_supported(SHAPE5(g), k.ldx, k.ldy)), ws_head2, nullptr, RUNG(k.ax == 0 && k.ay % 4 == 0)},
    {NB_STEM1K5, RUNG(stem1k5_lowp_supported(SHAPE5(g), k.ldx, k.ldy)), ws_stem1k5, nullptr, RUNG(k.ay == 0)},
    // k2 s2 down-convolution (V-Net): its weight gradient IS a ConvTranspose k2 s2 weight gradient with the roles swapped
    // (base voxels = the coarse dy, children = the fine x), and (Cout, Cin, 2, 2, 2) is that kernel's output layout; it cannot accumulate.
    // conservative: counted for every k2 s2 p0 geometry
    {NB_K2S2W, RUNG(k2s2_even(g) && convt_wgrad_lowp_supported(conv_vin(g) / 8, g.Cout, g.Cin, k.ldy, k.ldx, 2)),
     WS(convt_wgrad_lowp_ws_bytes((long long)g.N * (g.D / 2) * (g.H / 2) * (g.W / 2), g.Cout, g.Cin)), k2s2, RUNG(al16(k) && !k.accumulate)},
    // V-Net's two-channel k5 head off the head2 rung: the fp32 z-marching kernel (conv_headk.hip) behind the cast fall-back is 8x faster than
    // the generic small-channel wgrad below (the one-channel k5 stem has its own LDS-tiled kernel inside smallcin_wgrad)
    {NB_CAST, RUNG(headk_wgrad_supported(SHAPE5(g), g.Cin, g.Cout))},
    {NB_TINY, RUNG(tinypw_supported(SHAPE5(g)))},
    // conservative: counted for every pointwise geometry
    {NB_PWL, RUNG(pointwise(g) && pw_wgrad_lowp_supported(conv_vin(g), g.Cin, g.Cout, k.ldx, k.ldy, 2)), WS(pw_wgrad_lowp_ws_bytes(conv_vin(g), g.Cin, g.Cout)), pointwise, al16, NB_PW},
    {NB_PW, RUNG(pointwise(g) && pw_wgrad_supported(conv_vin(g), g.Cin, g.Cout, 1, k.ldx, k.ldy)), nullptr, nullptr, al8},
    {NB_STEM4, RUNG(stem4_lowp_supported(SHAPE5(g), k.ldx, k.ldy)), ws_stem4, nullptr, al16, NB_STEM},
    {NB_STEM, RUNG(stem_supported(SHAPE5(g), k.ldy)), nullptr, nullptr, al8},
    {NB_HEADPW, RUNG(headpw_lowp_supported(SHAPE5(g), k.ldx, k.ldy)), ws_headpw, nullptr, al16, NB_HEAD},
    {NB_HEAD, RUNG(head_supported(SHAPE5(g), k.ldx)), nullptr, nullptr, al8},
    {NB_SMALLCIN, RUNG(smallcin_wgrad_supported(g.Cin, g.Cout, g.k)), nullptr, nullptr, al8},
    {NB_SMALLCOUT, RUNG(smallcout_wgrad_supported(g.Cin, g.Cout, g.k, k.ldx)), nullptr, nullptr, al8},
    {NB_GW, RUNG(gwgrad_supported(GEOM9(g), k.ldx, k.ldy)), nullptr, nullptr, al8},
    {NB_CAST}};
static int choose_b16(const Rung* r, const ConvKey& k) {
    while (r->fits && !r->fits(k)) ++r;
    if (!r->aligned || r->aligned(k)) return r->family;
    for (const Rung* d = r + 1; r->demote && d->fits; ++d)
        if (d->family == r->demote) return d->fits(k) && d->aligned(k) ? d->family : NB_CAST;
    return NB_CAST;
}

// What mi355seg_last_conv_path reports for a family (MI355SEG_PATH_B16_*), one host-side store per call.  The igemm, gather and
// transposing-read launchers record themselves (conv_fwd_mfma, conv_gather_*_mfma, conv_wgrad_lowp: only they know the tiles and the K
// form), so their families map to 0 = "not here".  The cast fall-back records AFTER the staged fp32 entry point returned, over that call's
// fp32 code: the report says "cast", never the branch taken on the staged copies.
static void note_b16(int pass, int family) {
    static const int code[3][NB_CONVT + 1] = {
        {MI355SEG_PATH_B16_FWD_CAST, 0, 0, MI355SEG_PATH_B16_FWD_STEM1K5, 0, MI355SEG_PATH_B16_FWD_HEADPW, 0, MI355SEG_PATH_B16_FWD_HEAD2, MI355SEG_PATH_B16_FWD_STEM4,
         MI355SEG_PATH_B16_FWD_STEM, MI355SEG_PATH_B16_FWD_HEAD, 0, 0, 0, 0, 0, MI355SEG_PATH_B16_FWD_TINYPW, 0},
        {MI355SEG_PATH_B16_DGRAD_CAST, 0, 0, 0, 0, 0, 0, MI355SEG_PATH_B16_DGRAD_HEAD2, 0, 0, MI355SEG_PATH_B16_DGRAD_HEAD, 0, 0, 0, 0, 0, MI355SEG_PATH_B16_DGRAD_TINYPW,
         MI355SEG_PATH_B16_DGRAD_K2S2_CONVT},
        {MI355SEG_PATH_B16_WGRAD_CAST, 0, 0, MI355SEG_PATH_B16_WGRAD_STEM1K5, MI355SEG_PATH_B16_WGRAD_PW_LOWP, MI355SEG_PATH_B16_WGRAD_HEADPW, MI355SEG_PATH_B16_WGRAD_K2S2_CONVT,
         MI355SEG_PATH_B16_WGRAD_HEAD2, MI355SEG_PATH_B16_WGRAD_STEM4, MI355SEG_PATH_B16_WGRAD_STEM, MI355SEG_PATH_B16_WGRAD_HEAD, 0, MI355SEG_PATH_B16_WGRAD_PW_MFMA,
         MI355SEG_PATH_B16_WGRAD_SMALLCIN, MI355SEG_PATH_B16_WGRAD_SMALLCOUT, MI355SEG_PATH_B16_WGRAD_GWGRAD, MI355SEG_PATH_B16_WGRAD_TINYPW, 0}};
    if (code[pass][family]) note_conv_path(code[pass][family]);
}

// the cast fall-back: fp32 copies of x (or dx) and y (or dy) in the workspace, `run` on them with the rest of it, the written one cast back
template <typename F>
static int staged(const ConvCall& c, bool x_in, bool y_in, F run) {
    const ConvGeom& g = c.g;
    Carver cv(c.ws);
    float* xf = cv.take<float>((size_t)c.vin() * g.Cin);
    float* yf = cv.take<float>((size_t)c.vout() * g.Cout);
    const size_t used = cv.used();
    SEG_CHECK_WS(used + mi355seg_conv3d_ws_bytes(GEOM9(g)), c.ws_bytes);
    if (x_in) cast_rows((const bf16*)c.x, c.ldx, xf, g.Cin, c.vin(), g.Cin, c.st);
    if (y_in) cast_rows((const bf16*)c.y, c.ldy, yf, g.Cout, c.vout(), g.Cout, c.st);
    SEG_CHECK_LAUNCH();
    int rc = run(xf, yf, (char*)c.ws + used, c.ws_bytes - used);
    note_b16(x_in && y_in ? 2 : (x_in ? 0 : 1), NB_CAST);
    if (rc || (x_in && y_in)) return rc;
    if (x_in) cast_rows(yf, g.Cout, (bf16*)c.y, c.ldy, c.vout(), g.Cout, c.st);
    else cast_rows(xf, g.Cin, (bf16*)c.x, c.ldx, c.vin(), g.Cin, c.st);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

}  // namespace seg

using namespace seg;

extern "C" {

int mi355seg_set_b16_tiles(int mode) {
    SEG_CHECK_ARG(mode >= 0 && mode <= 2, "set_b16_tiles: 0 (auto), 1 (16x16x32 tiles wherever possible) or 2 (generic tiles), got %d", mode);
    set_b16_tiles(mode);
    return MI355SEG_OK;
}
int mi355seg_get_b16_tiles(void) { return get_b16_tiles(); }

int mi355seg_set_wgrad_wide(int mode) {
    SEG_CHECK_ARG(mode >= 0 && mode <= 2, "set_wgrad_wide: 0 (never), 1 (where it pays) or 2 (wherever the geometry allows), got %d", mode);
    set_wgrad_wide(mode);
    return MI355SEG_OK;
}
int mi355seg_get_wgrad_wide(void) { return get_wgrad_wide(); }

// workspace of the three bf16 Conv3d entry points for one layer geometry: the fp32 query, the rungs of the bf16 ladders the geometry can
// reach, and the staging copies of the cast fall-back
size_t mi355seg_conv3d_ws_bytes_bf16(int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad) {
    size_t base = mi355seg_conv3d_ws_bytes(N, D, H, W, Cin, Cout, k, stride, pad);
    if (D + 2 * pad < k || H + 2 * pad < k || W + 2 * pad < k) return base;
    const ConvGeom g{N, D, H, W, Cin, Cout, k, stride, pad, (D + 2 * pad - k) / stride + 1, (H + 2 * pad - k) / stride + 1, (W + 2 * pad - k) / stride + 1};
    for (const Rung* ladder : {FWD_B16, DGRAD_B16, WGRAD_B16})
        if (ladder_ws_bytes(ladder, g) > base) base = ladder_ws_bytes(ladder, g);
    // the fp32 staging copies of the fall-back: for shapes that take it with contiguous, aligned tensors, and -- while they stay under
    // 512 MB -- for every shape, because an entry point also falls back when a POINTER is not 16-byte aligned (a bf16 channel slice at an
    // 8-byte offset) or a k2 s2 weight gradient is asked to accumulate, which this query cannot see
    const ConvKey d = dense_key(g);
    const bool fb = !choose_b16(FWD_B16, d) || !choose_b16(DGRAD_B16, d) || !choose_b16(WGRAD_B16, d);
    const size_t stage = align_up((size_t)N * D * H * W * Cin * 4, 256) + align_up((size_t)N * g.Do * g.Ho * g.Wo * Cout * 4, 256) + 512;
    if (fb || stage <= ((size_t)512 << 20)) base += stage;
    return base;
}

int mi355seg_conv3d_fused_supported_bf16(int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad, int ldx, int ldy) {
    return choose_b16(FWD_B16, ConvKey{{N, D, H, W, Cin, Cout, k, stride, pad, 0, 0, 0}, ldx, ldy, 0, 0, 0}) == NB_IGEMM;
}
int mi355seg_conv3d_fwd_fused_bf16(const mi355seg_bf16* x, int ldx, const float* w, const float* oscale, const float* oshift, int act, float slope,
                                   mi355seg_bf16* y, int ldy, int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                                   void* ws, size_t ws_bytes, void* stream) {
    ConvCall c;
    int rc = conv_call(&c, "conv3d_fwd_fused_bf16", x, ldx, w, y, ldy, N, D, H, W, Cin, Cout, k, stride, pad, ws, ws_bytes, stream);
    if (rc) return rc;
    SEG_CHECK_ARG(oscale && oshift, "conv3d_fwd_fused_bf16: null pointer or pitch < channels");
    SEG_CHECK_ARG(choose_b16(FWD_B16, conv_key(c)) == NB_IGEMM, "conv3d_fwd_fused_bf16: no fused form for this shape / alignment (ask mi355seg_conv3d_fused_supported_bf16)");
    MfmaOpts o;
    o.oscale = oscale; o.act = act; o.slope = slope;
    return conv_fwd_mfma(MATH_B16, x, ldx, w, oshift, y, ldy, N, D, H, W, Cin, Cout, k, /*dgrad=*/0, nullptr, nullptr, ws, ws_bytes, c.st, o);
}

// y = conv(x) + res as the reference's two bf16 operations give it (each rounded to bf16): the sum rides in the convolution's epilogue
// where the launch allows (conv_b16s tiles, whole-K), else the activation kernel adds it in place
int mi355seg_conv3d_fwd_res_bf16(const mi355seg_bf16* x, int ldx, const float* w, const float* bias, const mi355seg_bf16* res, int ldres,
                                 mi355seg_bf16* y, int ldy, int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                                 void* ws, size_t ws_bytes, void* stream) {
    ConvCall c;
    int rc = conv_call(&c, "conv3d_fwd_res_bf16", x, ldx, w, y, ldy, N, D, H, W, Cin, Cout, k, stride, pad, ws, ws_bytes, stream);
    if (rc) return rc;
    SEG_CHECK_ARG(res && ldres >= Cout, "conv3d_fwd_res_bf16: null residual or pitch < channels");
    int fused = 0;
    if (choose_b16(FWD_B16, conv_key(c)) == NB_IGEMM) {
        MfmaOpts o;
        o.res = res; o.ldres = ldres; o.res_fused = &fused;
        rc = conv_fwd_mfma(MATH_B16, x, ldx, w, bias, y, ldy, N, D, H, W, Cin, Cout, k, /*dgrad=*/0, nullptr, nullptr, ws, ws_bytes, c.st, o);
    } else {
        rc = mi355seg_conv3d_fwd_bf16(x, ldx, w, bias, y, ldy, N, D, H, W, Cin, Cout, k, stride, pad, nullptr, nullptr, ws, ws_bytes, stream);
    }
    if (rc || fused) return rc;
    return mi355seg_act_fwd_bf16(y, ldy, res, ldres, y, ldy, c.vout(), Cout, 0, 0.f, stream);
}

int mi355seg_conv3d_fwd_bf16(const mi355seg_bf16* x, int ldx, const float* w, const float* bias, mi355seg_bf16* y, int ldy,
                             int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                             double* stats_sum, double* stats_sq, void* ws, size_t ws_bytes, void* stream) {
    ConvCall c;
    int rc = conv_call(&c, "conv3d_fwd_bf16", x, ldx, w, y, ldy, N, D, H, W, Cin, Cout, k, stride, pad, ws, ws_bytes, stream);
    if (rc) return rc;
    SEG_CHECK_ARG((stats_sum == nullptr) == (stats_sq == nullptr), "conv3d_fwd_bf16: stats_sum/stats_sq must come together");
    hipStream_t st = c.st;
    const int family = choose_b16(FWD_B16, conv_key(c));
    if (family != NB_CAST) note_b16(0, family);
    switch (family) {
    case NB_IGEMM: return conv_fwd_mfma(MATH_B16, x, ldx, w, bias, y, ldy, N, D, H, W, Cin, Cout, k, /*dgrad=*/0, stats_sum, stats_sq, ws, ws_bytes, st);
    case NB_GATHER: return conv_gather_fwd_mfma(MATH_B16, x, ldx, w, bias, y, ldy, N, D, H, W, Cin, Cout, k, stride, pad, stats_sum, stats_sq, ws, ws_bytes, st);
    case NB_HEAD2: return conv_stats_tail<bf16>(head2_fwd_lowp(x, ldx, w, bias, y, ldy, N, D, H, W, Cin, ws, ws_bytes, st), c, stats_sum, stats_sq);
    case NB_STEM1K5: return conv_stats_tail<bf16>(stem1k5_fwd_lowp(x, w, bias, y, ldy, N, D, H, W, Cout, ws, ws_bytes, st), c, stats_sum, stats_sq);
    case NB_STEM4: return conv_stats_tail<bf16>(stem4_fwd_lowp(x, w, bias, y, ldy, N, D, H, W, Cout, ws, ws_bytes, st), c, stats_sum, stats_sq);
    case NB_STEM: return stem_fwd(x, ldx, w, bias, y, ldy, N, D, H, W, Cin, Cout, stats_sum, stats_sq, ws, ws_bytes, st);
    case NB_HEADPW: return conv_stats_tail<bf16>(headpw_fwd_lowp(x, ldx, w, bias, y, ldy, c.vout(), Cin, Cout, st), c, stats_sum, stats_sq);
    case NB_HEAD: return conv_stats_tail<bf16>(head_fwd(x, ldx, w, bias, y, ldy, N, D, H, W, Cin, Cout, st), c, stats_sum, stats_sq);
    case NB_TINY: return conv_stats_tail<bf16>(tinypw_fwd(x, ldx, w, bias, y, ldy, c.vout(), Cin, Cout, st), c, stats_sum, stats_sq);
    default:
        return staged(c, true, false, [&](float* xf, float* yf, void* rest, size_t rest_bytes) {
            return mi355seg_conv3d_fwd_f32(xf, Cin, w, bias, yf, Cout, N, D, H, W, Cin, Cout, k, stride, pad, stats_sum, stats_sq, rest, rest_bytes, stream);
        });
    }
}

int mi355seg_conv3d_dgrad_bf16(const mi355seg_bf16* dy, int lddy, const float* w, mi355seg_bf16* dx, int lddx,
                               int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                               void* ws, size_t ws_bytes, void* stream) {
    ConvCall c;
    int rc = conv_call(&c, "conv3d_dgrad_bf16", dx, lddx, w, dy, lddy, N, D, H, W, Cin, Cout, k, stride, pad, ws, ws_bytes, stream);
    if (rc) return rc;
    hipStream_t st = c.st;
    const int family = choose_b16(DGRAD_B16, conv_key(c));
    if (family != NB_CAST) note_b16(1, family);
    switch (family) {
    case NB_IGEMM: return conv_fwd_mfma(MATH_B16, dy, lddy, w, nullptr, dx, lddx, N, D, H, W, Cout, Cin, k, /*dgrad=*/1, nullptr, nullptr, ws, ws_bytes, st);
    case NB_GATHER: return conv_gather_dgrad_mfma(MATH_B16, dy, lddy, w, dx, lddx, N, D, H, W, Cin, Cout, k, stride, pad, ws, ws_bytes, st);
    case NB_HEAD2: return head2_dgrad_lowp(dy, lddy, w, dx, lddx, N, D, H, W, Cin, ws, ws_bytes, st);
    case NB_HEAD: return head_dgrad(dy, lddy, w, dx, lddx, N, D, H, W, Cin, Cout, st);
    case NB_TINY: return tinypw_dgrad(dy, lddy, w, dx, lddx, c.vin(), Cin, Cout, st);
    case NB_CONVT: return convt_fwd_mfma(MATH_B16, dy, lddy, w, nullptr, dx, lddx, N, D / 2, H / 2, W / 2, Cout, Cin, ws, ws_bytes, st);
    default:
        return staged(c, false, true, [&](float* dxf, float* dyf, void* rest, size_t rest_bytes) {
            return mi355seg_conv3d_dgrad_f32(dyf, Cout, w, dxf, Cin, N, D, H, W, Cin, Cout, k, stride, pad, rest, rest_bytes, stream);
        });
    }
}

// dx = conv3d_dgrad(dy) + res on bf16 tensors, each of the two operations rounded to bf16 (what autograd's sum of the two gradients of a
// forked tensor computes): the sum rides in the input-gradient kernel's epilogue on the k3 / k5 stride-1 16x16x32 tiles (whole-K launches),
// else the library adds it in place after the input gradient.  res: dx's geometry at pitch ldres.
int mi355seg_conv3d_dgrad_res_bf16(const mi355seg_bf16* dy, int lddy, const float* w, const mi355seg_bf16* res, int ldres, mi355seg_bf16* dx, int lddx,
                                   int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                                   void* ws, size_t ws_bytes, void* stream) {
    ConvCall c;
    int rc = conv_call(&c, "conv3d_dgrad_res_bf16", dx, lddx, w, dy, lddy, N, D, H, W, Cin, Cout, k, stride, pad, ws, ws_bytes, stream);
    if (rc) return rc;
    SEG_CHECK_ARG(res && ldres >= Cin, "conv3d_dgrad_res_bf16: null residual or pitch < channels");
    int fused = 0;
    if (stride == 1 && 2 * pad == k - 1 && choose_b16(DGRAD_B16, conv_key(c)) == NB_IGEMM) {
        MfmaOpts o;
        o.res = res; o.ldres = ldres; o.res_fused = &fused;
        rc = conv_fwd_mfma(MATH_B16, dy, lddy, w, nullptr, dx, lddx, N, D, H, W, Cout, Cin, k, /*dgrad=*/1, nullptr, nullptr, ws, ws_bytes, c.st, o);
    } else {
        rc = mi355seg_conv3d_dgrad_bf16(dy, lddy, w, dx, lddx, N, D, H, W, Cin, Cout, k, stride, pad, ws, ws_bytes, stream);
    }
    if (rc || fused) return rc;
    return mi355seg_act_fwd_bf16(dx, lddx, res, ldres, dx, lddx, c.vin(), Cin, 0, 0.f, stream);
}

int mi355seg_conv3d_wgrad_bf16(const mi355seg_bf16* dy, int lddy, const mi355seg_bf16* x, int ldx, float* dw, float* db,
                               int N, int D, int H, int W, int Cin, int Cout, int k, int stride, int pad, int accumulate,
                               void* ws, size_t ws_bytes, void* stream) {
    ConvCall c;
    int rc = conv_call(&c, "conv3d_wgrad_bf16", x, ldx, dw, dy, lddy, N, D, H, W, Cin, Cout, k, stride, pad, ws, ws_bytes, stream);
    if (rc) return rc;
    hipStream_t st = c.st;
    if (db) {
        rc = channel_sums(dy, lddy, c.vout(), Cout, nullptr, nullptr, db, accumulate, ws, ws_bytes, st);
        if (rc) return rc;
    }
    float* part; int nstrips;
    const int family = choose_b16(WGRAD_B16, conv_key(c, accumulate));
    if (family != NB_CAST) note_b16(2, family);
    switch (family) {
    case NB_LOWP: return conv_wgrad_lowp(MATH_B16, dy, lddy, x, ldx, dw, N, D, H, W, Cin, Cout, k, stride, accumulate, ws, ws_bytes, st);
    case NB_HEAD2: return head2_wgrad_lowp(dy, lddy, x, ldx, dw, N, D, H, W, Cin, accumulate, ws, ws_bytes, st);
    case NB_STEM1K5: return stem1k5_wgrad_lowp(dy, lddy, x, dw, N, D, H, W, Cout, accumulate, ws, ws_bytes, st);
    case NB_K2S2W:
        rc = convt_wgrad_lowp(x, ldx, dy, lddy, N, D / 2, H / 2, W / 2, Cout, Cin, &part, &nstrips, ws, ws_bytes, st);
        if (rc) return rc;
        convt_wgrad_reduce(part, dw, nstrips, Cout, Cin, st);
        SEG_CHECK_LAUNCH();
        return MI355SEG_OK;
    case NB_TINY: return tinypw_wgrad(dy, lddy, x, ldx, dw, c.vin(), Cin, Cout, accumulate, ws, ws_bytes, st);
    case NB_PWL: return wgrad_strips_tail(pw_wgrad_lowp(dy, lddy, x, ldx, N, D, H, W, Cin, Cout, &part, &nstrips, ws, ws_bytes, st), part, nstrips, c, accumulate);
    case NB_PW: return wgrad_strips_tail(pw_wgrad_mfma(dy, lddy, x, ldx, N, D, H, W, Cin, Cout, 1, &part, &nstrips, ws, ws_bytes, st), part, nstrips, c, accumulate);
    case NB_STEM4: return stem4_wgrad_lowp(dy, lddy, x, dw, N, D, H, W, Cout, accumulate, ws, ws_bytes, st);
    case NB_STEM: return stem_wgrad(dy, lddy, x, ldx, dw, N, D, H, W, Cin, Cout, accumulate, ws, ws_bytes, st);
    case NB_HEADPW: return headpw_wgrad_lowp(dy, lddy, x, ldx, dw, c.vin(), Cin, Cout, accumulate, ws, ws_bytes, st);
    case NB_HEAD: return head_wgrad(dy, lddy, x, ldx, dw, N, D, H, W, Cin, Cout, accumulate, ws, ws_bytes, st);
    case NB_SMALLCIN: return smallcin_wgrad(dy, lddy, x, ldx, dw, N, D, H, W, Cin, Cout, k, stride, pad, accumulate, ws, ws_bytes, st);
    case NB_SMALLCOUT: return smallcout_wgrad(dy, lddy, x, ldx, dw, N, D, H, W, Cin, Cout, k, stride, pad, accumulate, ws, ws_bytes, st);
    case NB_GW: return conv_gwgrad(dy, lddy, x, ldx, dw, N, D, H, W, Cin, Cout, k, stride, pad, accumulate, ws, ws_bytes, st);
    default:
        return staged(c, true, true, [&](float* xf, float* dyf, void* rest, size_t rest_bytes) {
            return mi355seg_conv3d_wgrad_f32(dyf, Cout, xf, Cin, dw, nullptr, N, D, H, W, Cin, Cout, k, stride, pad, accumulate, rest, rest_bytes, stream);
        });
    }
}

// dtype casts of [rows, C] matrices with row pitches (autocast boundaries: fp32 <-> bf16 activations)
int mi355seg_cast_f32_to_bf16(const float* src, int ldsrc, mi355seg_bf16* dst, int lddst, long long rows, int C, void* stream) {
    SEG_CHECK_ARG(src && dst && rows > 0 && C > 0 && ldsrc >= C && lddst >= C, "cast_f32_to_bf16: bad arguments");
    cast_rows(src, ldsrc, dst, lddst, rows, C, (hipStream_t)stream);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}
int mi355seg_cast_bf16_to_f32(const mi355seg_bf16* src, int ldsrc, float* dst, int lddst, long long rows, int C, void* stream) {
    SEG_CHECK_ARG(src && dst && rows > 0 && C > 0 && ldsrc >= C && lddst >= C, "cast_bf16_to_f32: bad arguments");
    cast_rows(src, ldsrc, dst, lddst, rows, C, (hipStream_t)stream);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

}  // extern "C"
