// convt_api.inc -- ConvTranspose3d k2 s2 entry points, compiled once per storage type (TT = float with TT_MATH = MATH_F32,
// TT = bf16 with TT_MATH = MATH_B16).  Weights, bias and weight gradients are always fp32.
// Every entry point records the branch it takes (mi355seg_last_conv_path): MI355SEG_PATH_CONVT_* on fp32 tensors, the same code in the
// MI355SEG_PATH_B16_CONVT_* block on bf16 ones -- where convt_direct itself records which of its two forms runs (GEMM or streaming).
#define CONVT_B16 (MI355SEG_PATH_B16_CONVT_FWD_DIRECT - MI355SEG_PATH_CONVT_FWD_DIRECT)
#define CONVT_NOTE(code) note_conv_path(sizeof(TT) == 4 ? (code) : (code) + CONVT_B16)
int FN(convt3d_k2s2_fwd)(const TT* x, int ldx, const float* w, const float* bias,
                                  TT* y, int ldy, int N, int D, int H, int W, int Cin, int Cout,
                                  void* ws, size_t ws_bytes, void* stream) {
    return FN(convt3d_k2s2_fwd_ax)(x, ldx, w, bias, y, ldy, N, D, H, W, Cin, Cout, nullptr, ws, ws_bytes, stream);
}
// y_amax (optional, fp32 tensors): max |y| max-combined into the zeroed device scalar (the f16x3 scale of the convolution that reads y or
// the concat buffer y is a slice of), from the kernel's epilogue where it has one, else by a pass over y
int FN(convt3d_k2s2_fwd_ax)(const TT* x, int ldx, const float* w, const float* bias,
                                  TT* y, int ldy, int N, int D, int H, int W, int Cin, int Cout, float* y_amax,
                                  void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(x && w && y && N > 0 && D > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && ldx >= Cin && ldy >= Cout,
                  "convt3d_k2s2_fwd: bad arguments");
    SEG_CHECK_ARG(!(y_amax && sizeof(TT) != 4), "convt3d_k2s2_fwd_ax: y_amax is for fp32 tensors");
    hipStream_t st = (hipStream_t)stream;
    if ((sizeof(TT) == 2 || f32_conv_policy() == MATH_X3) && convt_direct_supported((int)sizeof(TT), false, N, D, H, W, Cin, Cout, ldx, ldy) &&
        ((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0 && ((uintptr_t)bias % 16) == 0) {
        CONVT_NOTE(MI355SEG_PATH_CONVT_FWD_DIRECT);
        return convt_direct<TT>(false, x, ldx, w, bias, y, ldy, N, D, H, W, Cin, Cout, ws, ws_bytes, st, y_amax);
    }
    struct AmaxAfter {                        // the other forms have no such epilogue: one pass over what they wrote
        const TT* y; int ldy; long long rows; int C; float* slot; hipStream_t st;
        ~AmaxAfter() { if constexpr (sizeof(TT) == 4) { if (slot) tensor_amax((const float*)y, ldy, rows, C, nullptr, slot, st); } }
    } after{y, ldy, (long long)N * 8 * D * H * W, Cout, y_amax, st};
    if (convt_mfma_supported(TT_MATH, N, D, H, W, Cin, Cout, ldx, ldy) && ((uintptr_t)x % 16) == 0) {
        CONVT_NOTE(MI355SEG_PATH_CONVT_FWD_MFMA);
        return convt_fwd_mfma(TT_MATH, x, ldx, w, bias, y, ldy, N, D, H, W, Cin, Cout, ws, ws_bytes, st);
    }
    CONVT_NOTE(MI355SEG_PATH_CONVT_FWD_PLAIN);
    Carver cv(ws);
    float* wp = cv.take<float>((size_t)8 * Cin * Cout);
    SEG_CHECK_WS(cv.used(), ws_bytes);
    hipLaunchKernelGGL(convt_pack_kernel, dim3(tgrid((long long)8 * Cin * Cout)), dim3(256), 0, st, w, wp, (float*)nullptr, Cin, Cout);
    SEG_CHECK_LAUNCH();
    long long total = (long long)N * D * H * W * 8 * Cout;
    hipLaunchKernelGGL(convt_fwd_kernel<TT>, dim3(tgrid(total)), dim3(256), 0, st, x, ldx, wp, bias, y, ldy, N, D, H, W, Cin, Cout);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int FN(convt3d_k2s2_dgrad)(const TT* dy, int lddy, const float* w, TT* dx, int lddx,
                                    int N, int D, int H, int W, int Cin, int Cout,
                                    void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(dy && w && dx && N > 0 && D > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && lddy >= Cout && lddx >= Cin,
                  "convt3d_k2s2_dgrad: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if ((sizeof(TT) == 2 || f32_conv_policy() == MATH_X3) && convt_direct_supported((int)sizeof(TT), true, N, D, H, W, Cin, Cout, lddx, lddy) &&
        ((uintptr_t)dy % 16) == 0 && ((uintptr_t)dx % 16) == 0) {
        CONVT_NOTE(MI355SEG_PATH_CONVT_DGRAD_DIRECT);
        return convt_direct<TT>(true, dy, lddy, w, nullptr, dx, lddx, N, D, H, W, Cin, Cout, ws, ws_bytes, st);
    }
    if (convt_mfma_supported(TT_MATH, N, D, H, W, Cin, Cout, lddx, lddy) && ((uintptr_t)dy % 16) == 0) {
        CONVT_NOTE(MI355SEG_PATH_CONVT_DGRAD_MFMA);
        return convt_dgrad_mfma(TT_MATH, dy, lddy, w, dx, lddx, N, D, H, W, Cin, Cout, ws, ws_bytes, st);
    }
    CONVT_NOTE(MI355SEG_PATH_CONVT_DGRAD_PLAIN);
    Carver cv(ws);
    float* wd = cv.take<float>((size_t)8 * Cin * Cout);
    SEG_CHECK_WS(cv.used(), ws_bytes);
    hipLaunchKernelGGL(convt_pack_kernel, dim3(tgrid((long long)8 * Cin * Cout)), dim3(256), 0, st, w, (float*)nullptr, wd, Cin, Cout);
    SEG_CHECK_LAUNCH();
    long long total = (long long)N * D * H * W * Cin;
    hipLaunchKernelGGL(convt_dgrad_kernel<TT>, dim3(tgrid(total)), dim3(256), 0, st, dy, lddy, wd, dx, lddx, N, D, H, W, Cin, Cout);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int FN(convt3d_k2s2_wgrad)(const TT* dy, int lddy, const TT* x, int ldx,
                                    float* dw, float* db, int N, int D, int H, int W, int Cin, int Cout,
                                    void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(dy && x && dw && N > 0 && D > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && lddy >= Cout && ldx >= Cin,
                  "convt3d_k2s2_wgrad: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const long long nvox = (long long)N * D * H * W;
    if (db) {
        int rc = channel_sums(dy, lddy, nvox * 8, Cout, nullptr, nullptr, db, 0, ws, ws_bytes, st);
        if (rc) return rc;
    }
    // bf16 tensors, or fp32 tensors under the bf16x6 conv math: the bf16 matrix cores (convt_wgrad_lowp.hip)
    if ((sizeof(TT) == 2 || f32_conv_policy() == MATH_X3) && convt_wgrad_lowp_supported(nvox, Cin, Cout, ldx, lddy, (int)sizeof(TT)) &&
        ((uintptr_t)x % 16) == 0 && ((uintptr_t)dy % 16) == 0) {
        float* part; int nstrips;
        CONVT_NOTE(MI355SEG_PATH_CONVT_WGRAD_LOWP);
        int rc = convt_wgrad_lowp(dy, lddy, x, ldx, N, D, H, W, Cin, Cout, &part, &nstrips, ws, ws_bytes, st);
        if (rc) return rc;
        convt_wgrad_reduce(part, dw, nstrips, Cin, Cout, st);
        SEG_CHECK_LAUNCH();
        return MI355SEG_OK;
    }
    if (pw_wgrad_supported(nvox, Cin, Cout, 8, ldx, lddy) && ((uintptr_t)x % (4 * sizeof(TT))) == 0 && ((uintptr_t)dy % (4 * sizeof(TT))) == 0) {
        float* part; int nstrips;
        CONVT_NOTE(MI355SEG_PATH_CONVT_WGRAD_MFMA);
        int rc = pw_wgrad_mfma(dy, lddy, x, ldx, N, D, H, W, Cin, Cout, 8, &part, &nstrips, ws, ws_bytes, st);
        if (rc) return rc;
        convt_wgrad_reduce(part, dw, nstrips, Cin, Cout, st);
        SEG_CHECK_LAUNCH();
        return MI355SEG_OK;
    }
    CONVT_NOTE(MI355SEG_PATH_CONVT_WGRAD_PLAIN);
    const int splits = convt_splits(nvox, Cin, Cout);
    Carver cv(ws);
    float* part = cv.take<float>((size_t)splits * 8 * Cin * Cout);
    SEG_CHECK_WS(cv.used(), ws_bytes);
    long long vps = (nvox + splits - 1) / splits;
    dim3 grid(cdiv((long long)Cin * Cout, 256), 8, splits);
    hipLaunchKernelGGL(convt_wgrad_kernel<TT>, grid, dim3(256), 0, st, dy, lddy, x, ldx, part, N, D, H, W, Cin, Cout, vps);
    SEG_CHECK_LAUNCH();
    convt_wgrad_reduce(part, dw, splits, Cin, Cout, st);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

#undef CONVT_NOTE
#undef CONVT_B16
