// norm_api.inc -- the tensor-typed entry points of norm.hip, compiled once per storage type (TT = float / bf16, FN(name) =
// mi355seg_<name>_f32 / _bf16).  Included from norm.hip inside extern "C".



int FN(norm_stats)(const TT* x, int ldx, long long rows, int groups, int C, float eps,
                            float* mean, float* rstd, float* running_mean, float* running_var,
                            float momentum, void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(x && mean && rstd && rows > 0 && groups > 0 && C > 0 && ldx >= C, "norm_stats: bad arguments");
    SEG_CHECK_ARG(!(running_mean && groups != 1), "norm_stats: running stats need groups == 1");
    SEG_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "norm_stats: running_mean/var must come together");
    RedPlan p;
    SEG_CHECK_ARG(red_plan(rows, C, ldx, &p), "norm_stats: unsupported channel count C=%d", C);
    size_t need = (size_t)groups * p.nblk * C * 2 * sizeof(float);
    SEG_CHECK_WS(need, ws_bytes);
    float* part = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    StatsF<TT> f{x, ldx, rows};
    ProfScope ps(PF_NORM, 0.0, (double)sizeof(TT) * rows * groups * C, st);
    int rc = launch_colreduce2(f, rows, groups, C, ldx, part, &p, st);
    if (rc) return rc;
    hipLaunchKernelGGL(stats_finalize_kernel<TT>, dim3(groups * C), dim3(64), 0, st, part, p.nblk, C,
                       groups, (double)rows, eps, mean, rstd, running_mean, running_var, momentum, x, ldx);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}


// y_amax (optional): max |y| max-combined into the device scalar *y_amax (zeroed by the caller) -- the f16x3 scale of the
// convolution that reads y, taken while y is written instead of by a pass of its own
int FN(norm_act_fwd_ax)(const TT* x, int ldx, const float* mean, const float* rstd,
                              const float* gamma, const float* beta, const TT* res, int ldres,
                              TT* y, int ldy, long long rows, int groups, int C,
                              int act, float slope, float* y_amax, void* stream) {
    SEG_CHECK_ARG(x && y && mean && rstd && rows > 0 && groups > 0 && C > 0, "norm_act_fwd: bad arguments");
    SEG_CHECK_ARG(act >= 0 && act <= 4, "norm_act_fwd: bad activation code %d", act);
    hipStream_t st = (hipStream_t)stream;
    bool v = vec_ok(C, {ldx, ldy, res ? ldres : 4});
    RowMap rm = ew_map(C, v);
    dim3 grid(row_grid(rows, rm.rpi), groups);
    ProfScope ps(PF_NORM, 0.0, (double)sizeof(TT) * rows * groups * C * (res ? 3.0 : 2.0), st);
    // 16-byte accesses for bf16 (+7 % on the Res-U-Net's InstanceNorms); for fp32 the 4-wide form already moves 16 bytes per
    // lane and two float4 per lane measured 13 % slower
    unsigned* ao = reinterpret_cast<unsigned*>(y_amax);
    if (sizeof(TT) == 2 && !ao && vec8_ok(C, {ldx, ldy, res ? ldres : 8}) && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)(res ? res : x)) % (8 * sizeof(TT))) == 0) {
        RowMap r8 = ew_map8(C);
        dim3 grid8(row_grid(rows, r8.rpi), groups);
        act_host_dispatch(act, [&](auto A_) { hipLaunchKernelGGL((norm_act_fwd8_kernel<TT, decltype(A_)::value>), grid8, dim3(256), 0, st, x, ldx, mean, rstd, gamma,
                           beta, res, ldres, y, ldy, rows, C, r8.lanes, r8.rpi, act, slope); });
    } else if (v)
        act_host_dispatch(act, [&](auto A_) { hipLaunchKernelGGL((norm_act_fwd_kernel<TT, true, decltype(A_)::value>), grid, dim3(256), 0, st, x, ldx, mean, rstd, gamma,
                           beta, res, ldres, y, ldy, rows, C, rm.lanes, rm.rpi, act, slope, ao); });
    else
        act_host_dispatch(act, [&](auto A_) { hipLaunchKernelGGL((norm_act_fwd_kernel<TT, false, decltype(A_)::value>), grid, dim3(256), 0, st, x, ldx, mean, rstd, gamma,
                           beta, res, ldres, y, ldy, rows, C, rm.lanes, rm.rpi, act, slope, ao); });
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}
int FN(norm_act_fwd)(const TT* x, int ldx, const float* mean, const float* rstd,
                              const float* gamma, const float* beta, const TT* res, int ldres,
                              TT* y, int ldy, long long rows, int groups, int C,
                              int act, float slope, void* stream) {
    return FN(norm_act_fwd_ax)(x, ldx, mean, rstd, gamma, beta, res, ldres, y, ldy, rows, groups, C, act, slope, nullptr, stream);
}

// ---- BatchNorm / InstanceNorm + activation backward in two halves, so that the first one (the two column sums) can instead come
// out of the epilogue of the kernel that PRODUCES dy (mi355seg_conv3d_dgrad_bnsums_f32) ----
// sums:   s1[g, c] = sum dz, s2[g, c] = sum dz * xhat  with dz = dy * act'(z)   (+ dgamma = s2, dbeta = s1 when groups == 1)
int FN(norm_act_bwd_sums)(const TT* dy, int lddy, const TT* x, int ldx,
                          const float* mean, const float* rstd, const float* gamma, const float* beta, const TT* res, int ldres,
                          float* s1, float* s2, float* dgamma, float* dbeta,
                          long long rows, int groups, int C, int act, float slope, void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(dy && x && mean && rstd && s1 && s2 && rows > 0 && groups > 0 && C > 0, "norm_act_bwd_sums: bad arguments");
    SEG_CHECK_ARG(!(dgamma && groups != 1), "norm_act_bwd_sums: affine grads need groups == 1");
    SEG_CHECK_ARG((dgamma == nullptr) == (dbeta == nullptr), "norm_act_bwd_sums: dgamma/dbeta must come together");
    RedPlan p;
    int ldmin = 4;
    if ((lddy % 4) || (ldx % 4) || (res && (ldres % 4))) ldmin = 1;
    SEG_CHECK_ARG(red_plan(rows, C, ldmin, &p), "norm_act_bwd_sums: unsupported channel count C=%d", C);
    Carver cv(ws);
    float* part = cv.take<float>((size_t)groups * p.nblk * C * 2);
    SEG_CHECK_WS(cv.used(), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    int rc = MI355SEG_OK;
    {
        ProfScope ps(PF_NORM, 0.0, (double)sizeof(TT) * rows * groups * C * (res ? 3.0 : 2.0), st);
        act_host_dispatch(act, [&](auto A_) {
            BwdF<TT, decltype(A_)::value> f{dy, lddy, x, ldx, mean, rstd, gamma, beta, res, ldres, act, slope};
            rc = launch_colreduce2(f, rows, groups, C, ldmin, part, &p, st);
        });
    }
    if (rc) return rc;
    hipLaunchKernelGGL(bwd_finalize_kernel, dim3(groups * C), dim3(64), 0, st, part, p.nblk, C, groups, s1, s2, dgamma, dbeta);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

// apply:  dx = rstd * gamma * (dz - s1 / rows - xhat * s2 / rows)  (+ dres = dz, + dx_colsum[c] = sum dx: the bias gradient of the
// convolution in front of the norm)
// dx_amax (optional): max |dx| max-combined into the zeroed device scalar *dx_amax (the f16x3 scale of the convolution gradients that read dx)
int FN(norm_act_bwd_apply_ax)(const TT* dy, int lddy, const TT* x, int ldx,
                           const float* mean, const float* rstd, const float* gamma, const float* beta, const TT* res, int ldres,
                           const float* s1, const float* s2, TT* dx, int lddx, TT* dres, int lddres, float* dx_colsum, float* dx_amax,
                           long long rows, int groups, int C, int act, float slope, void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(dy && x && mean && rstd && s1 && s2 && dx && rows > 0 && groups > 0 && C > 0, "norm_act_bwd_apply: bad arguments");
    SEG_CHECK_ARG(!(dx_colsum && groups != 1), "norm_act_bwd_apply: dx column sums need groups == 1");
    bool v = vec_ok(C, {lddy, ldx, lddx, res ? ldres : 4, dres ? lddres : 4});
    RowMap rm = ew_map(C, v);
    int nrb = row_grid(rows, rm.rpi);
    if (dx_colsum && nrb > 1024) nrb = 1024;       // bounds the per-block partials the column-sum finalise walks
    const bool fused_sum = dx_colsum && rm.lanes == (v ? C / 4 : C) && (256 % rm.lanes) == 0;
    Carver cv(ws);
    float* dxpart = fused_sum ? cv.take<float>((size_t)nrb * C * 2) : nullptr;
    SEG_CHECK_WS(cv.used(), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(nrb, groups);
    unsigned* ao = reinterpret_cast<unsigned*>(dx_amax);
    {
        ProfScope ps(PF_NORM, 0.0, (double)sizeof(TT) * rows * groups * C * 3.0, st);
        if (v)
            act_host_dispatch(act, [&](auto A_) { hipLaunchKernelGGL((norm_act_bwd_apply_kernel<TT, true, decltype(A_)::value>), grid, dim3(256), 0, st, dy, lddy, x, ldx, mean,
                               rstd, gamma, beta, res, ldres, s1, s2, dx, lddx, dres, lddres, rows, C, rm.lanes, rm.rpi, act, slope, dxpart, ao); });
        else
            act_host_dispatch(act, [&](auto A_) { hipLaunchKernelGGL((norm_act_bwd_apply_kernel<TT, false, decltype(A_)::value>), grid, dim3(256), 0, st, dy, lddy, x, ldx, mean,
                               rstd, gamma, beta, res, ldres, s1, s2, dx, lddx, dres, lddres, rows, C, rm.lanes, rm.rpi, act, slope, dxpart, ao); });
        SEG_CHECK_LAUNCH();
    }
    if (dx_colsum) {
        if (fused_sum) {
            hipLaunchKernelGGL(sums_finalize_kernel<float>, dim3(C), dim3(64), 0, st, dxpart, nrb, C, (double*)nullptr, (double*)nullptr, dx_colsum, 0,
                               (const float*)nullptr, 0, 0LL, 0);
            SEG_CHECK_LAUNCH();
        } else {
            return channel_sums(dx, lddx, rows, C, nullptr, nullptr, dx_colsum, 0, ws, ws_bytes, st);
        }
    }
    return MI355SEG_OK;
}

int FN(norm_act_bwd_apply)(const TT* dy, int lddy, const TT* x, int ldx,
                           const float* mean, const float* rstd, const float* gamma, const float* beta, const TT* res, int ldres,
                           const float* s1, const float* s2, TT* dx, int lddx, TT* dres, int lddres, float* dx_colsum,
                           long long rows, int groups, int C, int act, float slope, void* ws, size_t ws_bytes, void* stream) {
    return FN(norm_act_bwd_apply_ax)(dy, lddy, x, ldx, mean, rstd, gamma, beta, res, ldres, s1, s2, dx, lddx, dres, lddres, dx_colsum, nullptr,
                                     rows, groups, C, act, slope, ws, ws_bytes, stream);
}

static int NORM_IMPL(const TT* dy, int lddy, const TT* x, int ldx,
                             const float* mean, const float* rstd, const float* gamma, const float* beta,
                             const TT* res, int ldres,
                             TT* dx, int lddx, float* dgamma, float* dbeta, TT* dres, int lddres, float* dx_colsum,
                             long long rows, int groups, int C, int act, float slope,
                             void* ws, size_t ws_bytes, void* stream, float* dx_amax = nullptr) {
    SEG_CHECK_ARG(dy && x && mean && rstd && dx && rows > 0 && groups > 0 && C > 0, "norm_act_bwd: bad arguments");
    SEG_CHECK_ARG(!(dgamma && groups != 1), "norm_act_bwd: affine grads need groups == 1");
    SEG_CHECK_ARG(!(dx_colsum && groups != 1), "norm_act_bwd: dx column sums need groups == 1");
    SEG_CHECK_ARG((dgamma == nullptr) == (dbeta == nullptr), "norm_act_bwd: dgamma/dbeta must come together");
    // s1 / s2 live at the END of the workspace, behind everything the two halves carve from its front
    const size_t sb = align_up((size_t)groups * C * sizeof(float), 256);
    SEG_CHECK_WS(2 * sb + 256, ws_bytes);
    char* tail = (char*)ws + ((ws_bytes - 2 * sb) & ~(size_t)255);
    float* s1 = (float*)tail;
    float* s2 = (float*)(tail + sb);
    const size_t front = (size_t)(tail - (char*)ws);
    int rc = FN(norm_act_bwd_sums)(dy, lddy, x, ldx, mean, rstd, gamma, beta, res, ldres, s1, s2, dgamma, dbeta, rows, groups, C, act, slope,
                                   ws, front, stream);
    if (rc) return rc;
    return FN(norm_act_bwd_apply_ax)(dy, lddy, x, ldx, mean, rstd, gamma, beta, res, ldres, s1, s2, dx, lddx, dres, lddres, dx_colsum, dx_amax,
                                     rows, groups, C, act, slope, ws, front, stream);
}

int FN(norm_act_bwd)(const TT* dy, int lddy, const TT* x, int ldx,
                              const float* mean, const float* rstd, const float* gamma, const float* beta,
                              const TT* res, int ldres,
                              TT* dx, int lddx, float* dgamma, float* dbeta, TT* dres, int lddres,
                              long long rows, int groups, int C, int act, float slope,
                              void* ws, size_t ws_bytes, void* stream) {
    return NORM_IMPL(dy, lddy, x, ldx, mean, rstd, gamma, beta, res, ldres, dx, lddx, dgamma, dbeta, dres, lddres, nullptr,
                             rows, groups, C, act, slope, ws, ws_bytes, stream);
}

int FN(norm_act_bwd_colsum)(const TT* dy, int lddy, const TT* x, int ldx,
                                     const float* mean, const float* rstd, const float* gamma, const float* beta,
                                     const TT* res, int ldres,
                                     TT* dx, int lddx, float* dgamma, float* dbeta, TT* dres, int lddres, float* dx_colsum,
                                     long long rows, int groups, int C, int act, float slope,
                                     void* ws, size_t ws_bytes, void* stream) {
    return NORM_IMPL(dy, lddy, x, ldx, mean, rstd, gamma, beta, res, ldres, dx, lddx, dgamma, dbeta, dres, lddres, dx_colsum,
                             rows, groups, C, act, slope, ws, ws_bytes, stream);
}

int FN(norm_act_bwd_colsum_ax)(const TT* dy, int lddy, const TT* x, int ldx,
                                     const float* mean, const float* rstd, const float* gamma, const float* beta,
                                     const TT* res, int ldres,
                                     TT* dx, int lddx, float* dgamma, float* dbeta, TT* dres, int lddres, float* dx_colsum, float* dx_amax,
                                     long long rows, int groups, int C, int act, float slope,
                                     void* ws, size_t ws_bytes, void* stream) {
    return NORM_IMPL(dy, lddy, x, ldx, mean, rstd, gamma, beta, res, ldres, dx, lddx, dgamma, dbeta, dres, lddres, dx_colsum,
                             rows, groups, C, act, slope, ws, ws_bytes, stream, dx_amax);
}


// nn.PReLU(C) (vnet3d.py:14-18, the elu=False branch): y = max(z, 0) + slope[c] * min(z, 0), z = x (+ res)
int FN(prelu_fwd)(const TT* x, int ldx, const TT* res, int ldres, const float* slope, TT* y, int ldy,
                  long long rows, int C, void* stream) {
    SEG_CHECK_ARG(x && y && slope && rows > 0 && C > 0, "prelu_fwd: bad arguments");
    bool v = vec_ok(C, {ldx, ldy, res ? ldres : 4});
    RowMap rm = ew_map(C, v);
    dim3 grid(row_grid(rows, rm.rpi));
    ProfScope ps(PF_NORM, 0.0, (double)sizeof(TT) * rows * C * (res ? 3.0 : 2.0), (hipStream_t)stream);
    if (v)
        act_host_dispatch(MI355SEG_ACT_LRELU, [&](auto A_) { hipLaunchKernelGGL((act_kernel<TT, true, false, decltype(A_)::value>), grid, dim3(256), 0, (hipStream_t)stream, (const TT*)nullptr, 0, x,
                           ldx, res, ldres, y, ldy, rows, C, rm.lanes, rm.rpi, MI355SEG_ACT_LRELU, 0.f, slope); });
    else
        act_host_dispatch(MI355SEG_ACT_LRELU, [&](auto A_) { hipLaunchKernelGGL((act_kernel<TT, false, false, decltype(A_)::value>), grid, dim3(256), 0, (hipStream_t)stream, (const TT*)nullptr, 0, x,
                           ldx, res, ldres, y, ldy, rows, C, rm.lanes, rm.rpi, MI355SEG_ACT_LRELU, 0.f, slope); });
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

// dx = dy * (z > 0 ? 1 : slope[c]);  dslope[c] = sum_rows dy * min(z, 0)   (two-stage, fixed order).  ws: norm_ws_bytes(rows, 1, C)
int FN(prelu_bwd)(const TT* dy, int lddy, const TT* x, int ldx, const TT* res, int ldres, const float* slope,
                  TT* dx, int lddx, float* dslope, long long rows, int C, void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(dy && x && dx && slope && dslope && rows > 0 && C > 0, "prelu_bwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    RedPlan p;
    int ldmin = 4;
    if ((lddy % 4) || (ldx % 4) || (res && (ldres % 4))) ldmin = 1;
    SEG_CHECK_ARG(red_plan(rows, C, ldmin, &p), "prelu_bwd: unsupported channel count C=%d", C);
    Carver cv(ws);
    float* part = cv.take<float>((size_t)p.nblk * C * 2);
    float* unused = cv.take<float>((size_t)C);
    SEG_CHECK_WS(cv.used(), ws_bytes);
    PreluF<TT> f{dy, lddy, x, ldx, res, ldres};
    int rc;
    {
        ProfScope ps(PF_NORM, 0.0, (double)sizeof(TT) * rows * C * (res ? 3.0 : 2.0), st);
        rc = launch_colreduce2(f, rows, 1, C, ldmin, part, &p, st);
    }
    if (rc) return rc;
    hipLaunchKernelGGL(bwd_finalize_kernel, dim3(C), dim3(64), 0, st, part, p.nblk, C, 1, dslope, unused, (float*)nullptr, (float*)nullptr);
    SEG_CHECK_LAUNCH();
    bool v = vec_ok(C, {lddy, ldx, lddx, res ? ldres : 4});
    RowMap rm = ew_map(C, v);
    dim3 grid(row_grid(rows, rm.rpi));
    ProfScope ps(PF_NORM, 0.0, (double)sizeof(TT) * rows * C * (res ? 4.0 : 3.0), st);
    if (v)
        act_host_dispatch(MI355SEG_ACT_LRELU, [&](auto A_) { hipLaunchKernelGGL((act_kernel<TT, true, true, decltype(A_)::value>), grid, dim3(256), 0, st, dy, lddy, x, ldx,
                           res, ldres, dx, lddx, rows, C, rm.lanes, rm.rpi, MI355SEG_ACT_LRELU, 0.f, slope); });
    else
        act_host_dispatch(MI355SEG_ACT_LRELU, [&](auto A_) { hipLaunchKernelGGL((act_kernel<TT, false, true, decltype(A_)::value>), grid, dim3(256), 0, st, dy, lddy, x,
                           ldx, res, ldres, dx, lddx, rows, C, rm.lanes, rm.rpi, MI355SEG_ACT_LRELU, 0.f, slope); });
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int FN(scale_channels)(const TT* x, int ldx, const float* scale, TT* y, int ldy,
                                long long rows, int groups, int C, void* stream) {
    SEG_CHECK_ARG(x && scale && y && rows > 0 && groups > 0 && C > 0 && ldx >= C && ldy >= C, "scale_channels: bad arguments");
    bool v = vec_ok(C, {ldx, ldy});
    RowMap rm = ew_map(C, v);
    dim3 grid(row_grid(rows, rm.rpi), groups);
    ProfScope ps(PF_NORM, 0.0, (double)sizeof(TT) * rows * groups * C * 2.0, (hipStream_t)stream);
    if (v) hipLaunchKernelGGL((scale_channels_kernel<TT, true>), grid, dim3(256), 0, (hipStream_t)stream, x, ldx, scale, y, ldy, rows, C, rm.lanes, rm.rpi);
    else hipLaunchKernelGGL((scale_channels_kernel<TT, false>), grid, dim3(256), 0, (hipStream_t)stream, x, ldx, scale, y, ldy, rows, C, rm.lanes, rm.rpi);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int FN(act_bwd)(const TT* dy, int lddy, const TT* x, int ldx, const TT* res, int ldres,
                         TT* dx, int lddx, long long rows, int C, int act, float slope, void* stream);
int FN(act_fwd)(const TT* x, int ldx, const TT* res, int ldres, TT* y, int ldy,
                         long long rows, int C, int act, float slope, void* stream) {
    SEG_CHECK_ARG(x && y && rows > 0 && C > 0 && act >= 0 && act <= 4, "act_fwd: bad arguments");
    if (sizeof(TT) == 2 && vec8_ok(C, {ldx, ldy, res ? ldres : 8}) && ((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0 && (!res || ((uintptr_t)res % 16) == 0)) {
        RowMap rm = ew_map8(C);            // bf16: 16-byte accesses
        ProfScope ps(PF_NORM, 0.0, (double)sizeof(TT) * rows * C * (res ? 3.0 : 2.0), (hipStream_t)stream);
        act_host_dispatch(act, [&](auto A_) { hipLaunchKernelGGL((act8_kernel<TT, false, decltype(A_)::value>), dim3(row_grid(rows, rm.rpi)), dim3(256), 0, (hipStream_t)stream, (const TT*)nullptr, 0, x, ldx, res, ldres,
                           (const TT*)nullptr, 0, y, ldy, rows, C, rm.lanes, rm.rpi, act, slope); });
        SEG_CHECK_LAUNCH();
        return MI355SEG_OK;
    }
    bool v = vec_ok(C, {ldx, ldy, res ? ldres : 4});
    RowMap rm = ew_map(C, v);
    dim3 grid(row_grid(rows, rm.rpi));
    ProfScope ps(PF_NORM, 0.0, (double)sizeof(TT) * rows * C * (res ? 3.0 : 2.0), (hipStream_t)stream);
    if (v)
        act_host_dispatch(act, [&](auto A_) { hipLaunchKernelGGL((act_kernel<TT, true, false, decltype(A_)::value>), grid, dim3(256), 0, (hipStream_t)stream, (const TT*)nullptr, 0, x,
                           ldx, res, ldres, y, ldy, rows, C, rm.lanes, rm.rpi, act, slope, (const float*)nullptr); });
    else
        act_host_dispatch(act, [&](auto A_) { hipLaunchKernelGGL((act_kernel<TT, false, false, decltype(A_)::value>), grid, dim3(256), 0, (hipStream_t)stream, (const TT*)nullptr, 0, x,
                           ldx, res, ldres, y, ldy, rows, C, rm.lanes, rm.rpi, act, slope, (const float*)nullptr); });
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

// dx = addend + dy * act'(x + res): the activation's backward together with the sum of a second gradient of the same tensor (a residual
// fork: x feeds the activation AND, unchanged, a later sum).  addend NULL: mi355seg_act_bwd.  Eight channels per thread where the geometry
// allows (C % 8, pitches % 8, 16-byte pointers), else the 4-wide / scalar activation backward with the sum inside it: one store of dx.
int FN(act_bwd_add)(const TT* dy, int lddy, const TT* x, int ldx, const TT* res, int ldres, const TT* addend, int ldadd,
                             TT* dx, int lddx, long long rows, int C, int act, float slope, void* stream) {
    SEG_CHECK_ARG(dy && x && dx && rows > 0 && C > 0 && act >= 0 && act <= 4, "act_bwd_add: bad arguments");
    const size_t al = sizeof(TT) == 2 ? 16 : 16;
    if (vec8_ok(C, {lddy, ldx, lddx, res ? ldres : 8, addend ? ldadd : 8}) && ((uintptr_t)dy % al) == 0 && ((uintptr_t)x % al) == 0 && ((uintptr_t)dx % al) == 0 &&
        (!res || ((uintptr_t)res % al) == 0) && (!addend || ((uintptr_t)addend % al) == 0)) {
        RowMap rm = ew_map8(C);
        ProfScope ps(PF_NORM, 0.0, (double)sizeof(TT) * rows * C * (3.0 + (res ? 1.0 : 0.0) + (addend ? 1.0 : 0.0)), (hipStream_t)stream);
        act_host_dispatch(act, [&](auto A_) { hipLaunchKernelGGL((act8_kernel<TT, true, decltype(A_)::value>), dim3(row_grid(rows, rm.rpi)), dim3(256), 0, (hipStream_t)stream, dy, lddy, x, ldx, res, ldres,
                           addend, ldadd, dx, lddx, rows, C, rm.lanes, rm.rpi, act, slope); });
        SEG_CHECK_LAUNCH();
        return MI355SEG_OK;
    }
    return act_bwd_rows(dy, lddy, x, ldx, res, ldres, addend, ldadd, dx, lddx, rows, C, act, slope, (hipStream_t)stream);
}

int FN(act_bwd)(const TT* dy, int lddy, const TT* x, int ldx, const TT* res, int ldres,
                         TT* dx, int lddx, long long rows, int C, int act, float slope, void* stream) {
    SEG_CHECK_ARG(dy && x && dx && rows > 0 && C > 0 && act >= 0 && act <= 4, "act_bwd: bad arguments");
    if (sizeof(TT) == 2 && vec8_ok(C, {lddy, ldx, lddx, res ? ldres : 8}) && ((uintptr_t)dy % 16) == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)dx % 16) == 0 &&
        (!res || ((uintptr_t)res % 16) == 0))
        return FN(act_bwd_add)(dy, lddy, x, ldx, res, ldres, nullptr, 0, dx, lddx, rows, C, act, slope, stream);      // bf16: 16-byte accesses
    return act_bwd_rows(dy, lddy, x, ldx, res, ldres, (const TT*)nullptr, 0, dx, lddx, rows, C, act, slope, (hipStream_t)stream);
}

