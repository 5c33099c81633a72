// api_predict.inc -- part of api.hip (ONE translation unit: included from there, in this order; the parts share struct gpt_ctx and
// static helpers).  Gpt_predict, gpt_cov_sample, gpt_solve_L / gpt_cho_solve, gpt_potrf_host / gpt_gemm_nt_host.
// ------------------------------------------------------------------------------------------------
// predict
// ------------------------------------------------------------------------------------------------
extern "C" int gpt_predict(gpt_ctx *c, const double *Xstar, const int32_t *nstar, int64_t M, int want,
                           const double *noise_params, const int32_t *noise_n, double *mean_out, double *std_out,
                           double *cov_out)
{
    CTX_ENTER(c);
    NEED_FACTOR(c);
    if (!c->have_kernel) {
        gpt_set_error("gpt_predict needs a factorisation produced by gpt_fit");
        return GPT_E_STATE;
    }
    if (M <= 0 || !Xstar || !nstar || !mean_out || want < 0 || want > 2 || (want == 1 && !std_out)) {
        gpt_set_error("gpt_predict: bad arguments");
        return GPT_E_ARG;
    }
    if (M > 65535 * 32) return GPT_E_ARG;
    const int D = c->D;
    const int64_t N = c->N, n128 = round_up(N, 128), MP = round_up(M, 64);
    const int64_t Nx = c->Nx;
    const ModelKernel &model = c->model;
    const bool warp = c->warp.nlayers > 0;
    GPT_TRY(check_test_orders(model, c->n_maxsum, c->n_colmax, warp, nstar, M, D));
    hipStream_t st = c->stream;
    double *dXs, *dKst, *dmean;
    int32_t *dns;
    GPT_TRY(ensure(c, SLOT_XS, (size_t)M * D * sizeof(double), (void **)&dXs));
    GPT_TRY(ensure(c, SLOT_NS, (size_t)M * D * sizeof(int32_t), (void **)&dns));
    GPT_TRY(ensure(c, SLOT_KST, (size_t)MP * n128 * sizeof(double), (void **)&dKst));
    GPT_TRY(ensure(c, SLOT_VEC, (size_t)MP * 2 * sizeof(double), (void **)&dmean));
    double *dvar = dmean + MP;
    GPT_HIP_CHECK(hipMemcpyAsync(dXs, Xstar, (size_t)M * D * sizeof(double), hipMemcpyHostToDevice, st));
    GPT_HIP_CHECK(hipMemcpyAsync(dns, nstar, (size_t)M * D * sizeof(int32_t), hipMemcpyHostToDevice, st));
    // warp layers set (gpt_set_warp): the model kernel sees w(X*) and the slope factors of X*; the noise term below keeps X* itself
    const double *mXs = dXs, *dSs = nullptr;
    if (warp) {
        double *w, *s;
        GPT_TRY(ensure(c, SLOT_XSW, (size_t)M * D * sizeof(double), (void **)&w));
        GPT_TRY(ensure(c, SLOT_SS, (size_t)M * sizeof(double), (void **)&s));
        GPT_TRY(launch_warp_points(st, c->warp, dXs, dns, M, w, s));
        mXs = w;
        dSs = s;
    }
    const double *mX = model_X(c), *mS = model_S(c);
    // Kstar^T: row a = test point a, column i = training point i  (k is symmetric under swapping its
    // two (point, derivative-order) arguments, so this equals Kstar[i][a] of ref :966)
    GPT_TRY(launch_zero2d(st, MP, n128, dKst, n128));
    if (c->dT) {
        // with a transform the training side is T f(X): Kstar^T <- k(Xstar, X) T^T  (ref :966-970)
        double *dKx;
        GPT_TRY(ensure(c, SLOT_TK, (size_t)MP * c->NxP * sizeof(double), (void **)&dKx));
        GPT_TRY(launch_zero2d(st, MP, c->NxP, dKx, c->NxP));
        GPT_TRY(kbuild_terms(st, model, 0, mXs, dns, M, mX, c->dn, Nx, 0, 0, 0, nullptr, 0.0, 0.0, dKx, c->NxP, dSs, mS));
        GPT_TRY(gemm_nt(c, st, MP, round_up(N, 64), c->NxP, 1.0, dKx, c->NxP, c->dT, c->NxP, 0.0, dKst, n128, 0));
    } else
    GPT_TRY(kbuild_terms(st, model, 0, mXs, dns, M, mX, c->dn, N, 0, 0, 0, nullptr, 0.0, 0.0, dKst, n128, dSs, mS));
    GPT_TRY(ensure_alpha(c));
    GPT_TRY(launch_gemv_n(st, M, N, dKst, n128, c->d_alpha, dmean));
    GPT_HIP_CHECK(hipMemcpyAsync(mean_out, dmean, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
    if (want >= 1) {
        double *dV;                                                               // V' = Kstar^T L^-T (Kstar^T is consumed)
        GPT_TRY(ensure(c, SLOT_BTMP, (size_t)MP * n128 * sizeof(double), (void **)&dV));
        GPT_TRY(solve_rows_resident(c, st, MP, n128, dKst, n128, dV, n128));
        KParams kn;
        if (noise_params) GPT_TRY(make_kparams(GPT_KERNEL_DIAGNOISE, noise_params, 1, D, -1, 1, noise_n, &kn));
        if (want == 1) {
            double *dkd;
            GPT_TRY(ensure(c, SLOT_VEC2, (size_t)M * sizeof(double), (void **)&dkd));
            for (int t = 0; t < model.nterms; t++) {
                KParams ks = model.f1[t];
                ks.symmetric = 1;
                ks.hyper_deriv = -1;
                GPT_TRY(launch_kpairs(st, ks, mXs, mXs, dns, dns, M, dkd, t > 0 ? 1 : 0, model.second(t)));
            }
            if (warp) GPT_TRY(launch_warp_scale_diag(st, dkd, dSs, M));
            GPT_TRY(launch_rowsumsq_sub(st, M, n128, dV, n128, dkd, dvar));
            GPT_HIP_CHECK(hipMemcpyAsync(std_out, dvar, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
            GPT_HIP_CHECK(hipStreamSynchronize(st));
            double nv = 0.0;
            for (int64_t a = 0; a < M; a++) {
                if (noise_params) {          // diagonal of the symmetric noise term (ref: noise.py:103-104)
                    bool hit = true;
                    for (int d = 0; d < D; d++) hit = hit && nstar[a * D + d] == kn.noise_n[d];
                    nv = hit ? noise_params[0] * noise_params[0] : 0.0;
                }
                std_out[a] = sqrt(std_out[a] + nv);
            }
            return GPT_OK;
        }
        // cov = K(Xstar, Xstar) - V' V'^T.  Only the lower triangle is computed (SYRK flops, not GEMM's), one 512-wide block
        // column at a time; behind each block column a mirror kernel completes ITS block row (the transposes of the rows
        // below it), and that block row starts for the host on a second stream while the next block column is computed: the
        // M^2 doubles of the result cross PCIe under the SYRK (M = 4096, N = 8192: 18.3 -> ~10 ms).
        // cov_out == NULL: the covariance stays on the device (lower triangle, SLOT_KSS) for gpt_cov_sample; nothing moves.
        double *dcov;
        // (row stride LDC = M rounded up to 128: gpt_cov_sample factors this matrix in place, padded to whole 128-blocks)
        const int64_t LDC = round_up(M, 128);
        GPT_TRY(ensure(c, SLOT_KSS, (size_t)LDC * LDC * sizeof(double), (void **)&dcov));
        GPT_TRY(launch_zero2d(st, LDC, LDC, dcov, LDC));
        GPT_TRY(kbuild_terms(st, model, 1, mXs, dns, M, mXs, dns, M, 0, 0, 0, nullptr, 0.0, 0.0, dcov, LDC, dSs, dSs));
        if (noise_params) GPT_TRY(launch_add_noise_sym(st, kn, dXs, dns, M, dcov, LDC));
        c->cov_M = 0;
        const int64_t CB = 512;
        const int64_t nblk = (MP + CB - 1) / CB;
        if (cov_out && !c->copy_stream) {
            GPT_HIP_CHECK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
            for (auto &e : c->cev) GPT_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        for (int64_t q = 0; q < nblk; q++) {
            const int64_t c0 = q * CB, w = (MP - c0 < CB) ? MP - c0 : CB;
            if (MP <= 256)
                GPT_TRY(gemm_nt_few(c, st, MP, MP, n128, -1.0, dV, n128, dV, n128, 1.0, dcov, LDC, 1));
            else
                GPT_TRY(gemm_nt(c, st, MP - c0, w, n128, -1.0, dV + c0 * n128, n128, dV + c0 * n128, n128, 1.0, dcov + c0 * LDC + c0, LDC, 1));
            if (!cov_out) continue;
            GPT_TRY(launch_mirror_rows(st, dcov, LDC, c0, w, MP));
            hipEvent_t e = get_event(c, 100 + (size_t)q);
            if (!e) return GPT_E_HIP;
            GPT_HIP_CHECK(hipEventRecord(e, st));
        }
        if (!cov_out) {
            GPT_TRY(launch_diag_gather(st, dcov, LDC, M, dvar));
            if (std_out) GPT_HIP_CHECK(hipMemcpyAsync(std_out, dvar, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
            GPT_HIP_CHECK(hipStreamSynchronize(st));
            if (std_out)
                for (int64_t a = 0; a < M; a++) std_out[a] = sqrt(std_out[a]);
            c->cov_M = M;
            return GPT_OK;
        }
        for (int64_t q = 0; q < nblk; q++) {
            const int64_t c0 = q * CB;
            if (c0 >= M) break;
            const int64_t rows = (M - c0 < CB) ? M - c0 : CB;
            GPT_HIP_CHECK(hipStreamWaitEvent(c->copy_stream, get_event(c, 100 + (size_t)q), 0));
            GPT_TRY(d2h_rows(c, cov_out + c0 * M, M, dcov + c0 * LDC, LDC, rows, M));
        }
        GPT_TRY(d2h_finish(c));
        GPT_HIP_CHECK(hipStreamSynchronize(st));
        if (std_out)
            for (int64_t a = 0; a < M; a++) std_out[a] = sqrt(cov_out[a * M + a]);
        return GPT_OK;
    }
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    return GPT_OK;
}

// Posterior samples from the device-resident predictive covariance (ref: gaussian_process.py:1295-1300, :1330, draw_sample
// with rand_vars and method='cholesky'): after gpt_predict(want = 2, cov_out = NULL),
//   L = cholesky(cov + diag_add I) in place on the device,  out (M x S) = L rand (M x S)
// -- the M x M covariance never crosses PCIe (the caller adds the mean).  The resident factor of the fit is untouched (the
// factorisation here has its own workspace).  Status > 0: that leading minor of the loaded covariance is not positive definite.
extern "C" int gpt_cov_sample(gpt_ctx *c, int64_t M_rows, double diag_add, const double *rand, int64_t S, double *out)
{
    CTX_ENTER(c);
    if (c->cov_M <= 0) {
        gpt_set_error("gpt_cov_sample: call gpt_predict(want = 2, cov_out = NULL) first");
        return GPT_E_STATE;
    }
    if (!rand || !out || S <= 0) return GPT_E_ARG;
    if (M_rows != c->cov_M) {
        gpt_set_error("gpt_cov_sample: rand has %lld rows, the resident covariance %lld", (long long)M_rows, (long long)c->cov_M);
        return GPT_E_ARG;
    }
    const int64_t M = c->cov_M, LDC = round_up(M, 128), SP = round_up(S, 64);
    hipStream_t st = c->stream;
    double *dcov = (double *)c->slots[SLOT_KSS].p, *dzero, *ws, *dlow, *dRt, *dOut;
    GPT_TRY(ensure(c, SLOT_ZERO, (size_t)M * sizeof(double), (void **)&dzero));
    GPT_TRY(ensure(c, SLOT_BATCH_WS, ((size_t)(LDC / 128) * GPT_WS_BLOCK + 8) * sizeof(double), (void **)&ws));
    int32_t *dinfo = reinterpret_cast<int32_t *>(ws + (LDC / 128) * GPT_WS_BLOCK);
    GPT_TRY(ensure(c, SLOT_LOW, (size_t)LDC * LDC * sizeof(double), (void **)&dlow));
    GPT_TRY(ensure(c, SLOT_RHS, (size_t)SP * LDC * sizeof(double), (void **)&dRt));
    GPT_TRY(ensure(c, SLOT_OUT, (size_t)LDC * SP * sizeof(double), (void **)&dOut));
    c->cov_M = 0;                                                    // (the covariance is consumed)
    c->batch_gen++;                                                  // (SLOT_BATCH_WS is reused below: no batch resident any more)
    EvalScope scope(c, true);                                        // counted like an evaluation in flight, on event edges
    GPT_HIP_CHECK(hipMemsetAsync(dzero, 0, (size_t)M * sizeof(double), st));
    GPT_HIP_CHECK(hipMemsetAsync(dinfo, 0, sizeof(int32_t), st));
    GPT_TRY(launch_add_diag(st, dcov, LDC, M, dzero, diag_add));
    GPT_TRY(launch_fill_pad(st, dcov, LDC, M, LDC, nullptr, 0.0));      // unit diagonal on the padding rows
    // rand^T, zero padded: the GEMM wants the contraction index (rows of rand) contiguous
    std::vector<double> Rt((size_t)SP * LDC, 0.0);
    for (int64_t k = 0; k < M; k++)
        for (int64_t s_ = 0; s_ < S; s_++) Rt[(size_t)s_ * LDC + k] = rand[(size_t)k * S + s_];
    GPT_HIP_CHECK(hipMemcpyAsync(dRt, Rt.data(), Rt.size() * sizeof(double), hipMemcpyHostToDevice, st));
    GPT_TRY(potrf_run(c, LDC, dcov, LDC, ws, dinfo));
    GPT_TRY(launch_extract_lower(st, dcov, LDC, LDC, dlow, LDC));
    GPT_TRY(gemm_nt(c, st, LDC, SP, LDC, 1.0, dlow, LDC, dRt, LDC, 0.0, dOut, SP, 0));
    int32_t info = 0;
    GPT_HIP_CHECK(hipMemcpyAsync(&info, dinfo, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipMemcpy2DAsync(out, (size_t)S * sizeof(double), dOut, (size_t)SP * sizeof(double), (size_t)S * sizeof(double),
                                   (size_t)M, hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    if (info != 0) {
        gpt_set_error("%d-th leading minor of the array is not positive definite", (int)info);
        return (int)(info > M ? M : info);
    }
    return GPT_OK;
}

// ------------------------------------------------------------------------------------------------
// generic solves against the resident factor
// ------------------------------------------------------------------------------------------------
static int solve_common(gpt_ctx *c, double *B, int64_t nrhs, bool full)
{
    CTX_ENTER(c);
    NEED_FACTOR(c);
    if (!B || nrhs <= 0) return GPT_E_ARG;
    const int64_t N = c->N, n128 = round_up(N, 128), RP = round_up(nrhs, 64);
    hipStream_t st = c->stream;
    double *dBt;
    GPT_TRY(ensure(c, SLOT_RHS, (size_t)RP * n128 * sizeof(double), (void **)&dBt));
    std::vector<double> Bt((size_t)nrhs * N);
    for (int64_t i = 0; i < N; i++)
        for (int64_t r = 0; r < nrhs; r++) Bt[(size_t)r * N + i] = B[(size_t)i * nrhs + r];
    GPT_TRY(launch_zero2d(st, RP, n128, dBt, n128));
    GPT_HIP_CHECK(hipMemcpy2DAsync(dBt, (size_t)n128 * sizeof(double), Bt.data(), (size_t)N * sizeof(double),
                                   (size_t)N * sizeof(double), (size_t)nrhs, hipMemcpyHostToDevice, st));
    {
        double *dIn = dBt;                                                        // rows: (L^-1 b_r)^T, out of place
        GPT_TRY(ensure(c, SLOT_BTMP, (size_t)RP * n128 * sizeof(double), (void **)&dBt));
        GPT_TRY(solve_rows_resident(c, st, RP, n128, dIn, n128, dBt, n128));
    }
    if (full)
        for (int64_t r = 0; r < nrhs; r++) {
            // the padded tail of each row is (numerically) zero except a ~1e-150 entry in the augmented
            // column; clear it so the backward substitution sees an exact zero there
            if (n128 > N) GPT_HIP_CHECK(hipMemsetAsync(dBt + r * n128 + N, 0, (size_t)(n128 - N) * sizeof(double), st));
            GPT_TRY(launch_trsv_lt(st, n128, c->dA, c->NP, c->d_invd, dBt + r * n128));
        }
    GPT_HIP_CHECK(hipMemcpy2DAsync(Bt.data(), (size_t)N * sizeof(double), dBt, (size_t)n128 * sizeof(double),
                                   (size_t)N * sizeof(double), (size_t)nrhs, hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    for (int64_t i = 0; i < N; i++)
        for (int64_t r = 0; r < nrhs; r++) B[(size_t)i * nrhs + r] = Bt[(size_t)r * N + i];
    return GPT_OK;
}

extern "C" int gpt_solve_L(gpt_ctx *c, double *B, int64_t nrhs) { return solve_common(c, B, nrhs, false); }
extern "C" int gpt_cho_solve(gpt_ctx *c, double *B, int64_t nrhs) { return solve_common(c, B, nrhs, true); }

// ------------------------------------------------------------------------------------------------
// standalone dense entry points on host matrices
// ------------------------------------------------------------------------------------------------
extern "C" int gpt_potrf_host(gpt_ctx *c, double *A, int64_t N)
{
    CTX_ENTER(c);
    if (!A || N <= 0) return GPT_E_ARG;
    std::vector<double> y((size_t)N, 0.0);
    double ll, ld;
    int rc = gpt_fit_matrix(c, A, N, y.data(), &ll, &ld);
    if (rc != GPT_OK) return rc;
    return gpt_get_L(c, A);
}

extern "C" int gpt_gemm_nt_host(gpt_ctx *c, int64_t m, int64_t n, int64_t k, double alpha, const double *A,
                                const double *B, double beta, double *C)
{
    CTX_ENTER(c);
    if (m <= 0 || n <= 0 || k <= 0 || !A || !B || !C) return GPT_E_ARG;
    const int64_t mp = round_up(m, 64), np = round_up(n, 64), kp = round_up(k, 64);
    double *dA, *dB, *dC;
    GPT_TRY(ensure(c, SLOT_KST, (size_t)mp * kp * sizeof(double), (void **)&dA));
    GPT_TRY(ensure(c, SLOT_KSS, (size_t)np * kp * sizeof(double), (void **)&dB));
    GPT_TRY(ensure(c, SLOT_RHS, (size_t)mp * np * sizeof(double), (void **)&dC));
    hipStream_t st = c->stream;
    GPT_TRY(launch_zero2d(st, mp, kp, dA, kp));
    GPT_TRY(launch_zero2d(st, np, kp, dB, kp));
    GPT_TRY(launch_zero2d(st, mp, np, dC, np));
    GPT_HIP_CHECK(hipMemcpy2DAsync(dA, kp * sizeof(double), A, k * sizeof(double), k * sizeof(double), m, hipMemcpyHostToDevice, st));
    GPT_HIP_CHECK(hipMemcpy2DAsync(dB, kp * sizeof(double), B, k * sizeof(double), k * sizeof(double), n, hipMemcpyHostToDevice, st));
    GPT_HIP_CHECK(hipMemcpy2DAsync(dC, np * sizeof(double), C, n * sizeof(double), n * sizeof(double), m, hipMemcpyHostToDevice, st));
    GPT_TRY(gemm_nt(c, st, mp, np, kp, alpha, dA, kp, dB, kp, beta, dC, np, 0));
    GPT_HIP_CHECK(hipMemcpy2DAsync(C, n * sizeof(double), dC, np * sizeof(double), n * sizeof(double), m, hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    return GPT_OK;
}
