// api_sparse_grad.inc -- part of api.hip (ONE translation unit: included from there, in this order; the parts share struct gpt_ctx and
// static helpers).  The gradient of the inducing-point objective (DESIGN.md sections 18.8, 18.9): gpt_sparse_grad_diff, gpt_sparse_grad_z
// (the same pass with d ll / d Z), and the device API of their kernels, gpt_dev_sparse_grad_rows / _grad_pairs / _grad_dz_pairs
// (gpt_dev_sparse_gram2 stands beside gpt_dev_sparse_gram, api_sparse.inc).  The
// stencil is read by grad_stencil.inc, as for the dense gradients; the chunk front end, the view of the resident factors and the upload
// of y are api_sparse.inc's, shared with the fit and the prediction.
// ------------------------------------------------------------------------------------------------
// With the notation of api_sparse.inc, r = y - mu(X), s_i = noise_var + err_y_i^2:
//     t = L_B^-T c     beta = L_u^-T t     alpha_i = (r_i - v_i.t) / Lambda_i     w_i = L_B^-1 v_i
//     W_ii = alpha_i^2 - 1 / Lambda_i + |w_i|^2 / Lambda_i^2          e_i = W_ii (fitc), -1 / s_i (vfe), 0 (dtc)
//     g_i = W_ii / 2 (+ (k_i - q_i) / (2 s_i^2), vfe)                  d ll / d noise_var = sum_i g_i
//     A_fu[i,:] = alpha_i beta^T - (1 / Lambda_i) v_i^T B^-1 L_u^-1 - e_i v_i^T L_u^-1
//     A_uu = -1/2 (beta beta^T - S),   S = L_u^-T (I - B^-1 + V diag(e) V^T) L_u^-1      (V diag(e) V^T = -(B - I) for vfe, 0 for dtc)
//     d ll = sum A_uu dK_uu + sum A_fu dK_fu + 1/2 sum_i e_i dk_i + sum_i g_i ds_i
// dK is the term's central difference taken per pair, divided by denom once per parameter on the host (kgrad.hip, kgrad_rect.hip).
// One second pass over the chunks of the fit: four chunk x LDV buffers (V^T; W^T, then A_fu in its place; the two scaled copies of
// V^T), so the size rule gives the gradient half the fit's rows per chunk; device memory stays O(M^2 + chunk M).
// ------------------------------------------------------------------------------------------------

// The orders the pair pass of gpt_sparse_grad_z meets on the inducing side are n_Z + e_d (DESIGN.md 18.9): the resident model against the
// raised bounds -- sp_zmaxsum + 1, sp_zcolmax[d] + 1 for every d -- through the rules of parse_model (the Gibbs limit of its coordinate,
// the chain / product limit, the periodic / spectral per-dimension rule), and a Matern52 factor checks the raised rows as the fit
// checks the rows themselves.  Before any launch; the statuses and messages are those functions'.
static int sparse_dz_orders(const gpt_ctx *c, const ModelKernel &m)
{
    const int D = c->D;
    long colmax[GPT_MAX_DIM];
    const long maxsum = c->n_maxsum > c->sp_zmaxsum + 1 ? c->n_maxsum : c->sp_zmaxsum + 1;
    for (int d = 0; d < GPT_MAX_DIM; d++) colmax[d] = c->n_colmax[d] > c->sp_zcolmax[d] + 1 ? c->n_colmax[d] : c->sp_zcolmax[d] + 1;
    for (int t = 0; t < m.nterms; t++) {
        const int k1 = m.f1[t].kernel_id, k2 = m.second(t) ? m.f2[t].kernel_id : -1;
        GPT_TRY(check_train_orders(k1, k2, maxsum, train_gibbs_max(m.abi_id1[t], D, maxsum, colmax),
                                   k2 >= 0 ? train_gibbs_max(m.abi_id2[t], D, maxsum, colmax) : 0));
        if (per_form_kid(k1) || per_form_kid(k2)) GPT_TRY(check_periodic_colmax(colmax, colmax, D, per_form_name(k1, k2)));
    }
    if (m.has_m52) {
        std::vector<int32_t> hz((size_t)c->sp_M * D);
        GPT_HIP_CHECK(hipMemcpy(hz.data(), sparse_nZ(c), hz.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < c->sp_M; i++) hz[i * D] += 1;      // (the rule reads a row's sum: e_0 stands for every e_d)
        GPT_TRY(check_m52_orders(hz.data(), c->sp_M, D));
    }
    return GPT_OK;
}

// The ONE body of gpt_sparse_grad_diff (dz_out NULL) and gpt_sparse_grad_z: with dz_out the adjoints A_fu and A_uu are formed whatever nh
// is, one launch_kgrad_dz per model term follows A_fu in every chunk, and the Z-Z pass runs the same kernel with 2 A_uu after the chunks.
// Without it every launch, its place and its operands are what gpt_sparse_grad_diff's always were.
static int sparse_grad_body(gpt_ctx *c, const char *who, int nh, const int *term_idx, const double *params_a, const double *params_b,
                            const double *denom, const double *y, const double *err_y, double *out, double *alpha_out, double *dz_out)
{
    GPT_TRY(sparse_refusals(c, who, true));
    if (nh < 0 || (nh > 0 && (!term_idx || !params_a || !params_b || !denom)) || !y || !err_y || !out) {
        gpt_set_error("%s: bad arguments", who);
        return GPT_E_ARG;
    }
    const ModelKernel &model = c->sp_model;
    const int D = c->D, method = c->sp_method;
    const int64_t N = c->Nx;
    long maxsum, colmax[GPT_MAX_DIM];
    sparse_order_bounds(c, &maxsum, colmax);
    GradStencil gs;
    GPT_TRY(grad_stencil_build(who, D, maxsum, colmax, model, nh, term_idx, params_a, params_b, denom, &gs));
    if (dz_out) GPT_TRY(sparse_dz_orders(c, model));
    const std::vector<KParams> &kp1 = gs.kp1, &kp2 = gs.kp2;
    const std::vector<int> &where = gs.where;
    const int total = (int)where.size();
    const bool adj = total > 0 || dz_out != nullptr;      // the adjoints A_fu, A_uu are needed
    const SparseResident res = sparse_resident(c);
    const int64_t M = res.d.M, MPU = res.d.MPU, BP = res.d.BP, LDV = res.d.LDV, ME = round_up(M, 64);
    int64_t chunk;
    GPT_TRY(sparse_chunk(res.d, c->sp_chunk_rows, N, &chunk, 4));
    int nslices = 1;
    if (method == GPT_SPARSE_FITC) GPT_TRY(sparse_slices(c, ME, chunk < N ? chunk : N, &nslices));
    hipStream_t st = c->stream;
    const double *dLu = res.Lu, *dLb = res.Lb, *ws_u = res.ws_u, *ws_b = res.ws_b, *d_c = res.c, *dZ = res.Z;
    const int32_t *dnZ = res.nZ;
    double *dV, *dW, *dS1, *dS2, *dGM, *dvec, *dY, *dPart = nullptr, *dpart = nullptr, *dzz = nullptr, *dzpart = nullptr, *ddz = nullptr;
    KParams *dkp = nullptr;
    GPT_TRY(ensure(c, SLOT_SP_V, (size_t)chunk * LDV * sizeof(double), (void **)&dV));
    GPT_TRY(ensure(c, SLOT_SP_W, (size_t)chunk * LDV * sizeof(double), (void **)&dW));
    GPT_TRY(ensure(c, SLOT_SP_S1, (size_t)chunk * LDV * sizeof(double), (void **)&dS1));
    GPT_TRY(ensure(c, SLOT_SP_S2, (size_t)chunk * LDV * sizeof(double), (void **)&dS2));
    // the matrices of order M: U_u = L_u^-T, P2 = L_u^-T B^-1, B^-1 (MPU x MPU each), three scratch matrices of order BP, the signed Gram
    GPT_TRY(ensure(c, SLOT_SP_GM, ((size_t)3 * MPU * MPU + (size_t)3 * BP * BP + (size_t)ME * ME) * sizeof(double), (void **)&dGM));
    double *Uu = dGM, *P2 = Uu + MPU * MPU, *Binv = P2 + MPU * MPU, *T0 = Binv + MPU * MPU, *T1 = T0 + BP * BP, *T2 = T1 + BP * BP,
           *dE = T2 + BP * BP;
    // vectors: [0, 2) the running sums of g (and the unused second sum of sparse_rowsum_kernel), [2, 4) the "bad Lambda" word, then one
    // running sum per stencil entry, t and beta (MPU each), and per chunk k_i, alpha_i, e_i and the two rows of g's values
    const size_t nacc = (size_t)(total > 0 ? total : 1), head = 4 + nacc + 2 * (size_t)MPU;
    GPT_TRY(ensure(c, SLOT_SP_GVEC, (head + 5 * (size_t)chunk) * sizeof(double), (void **)&dvec));
    double *dsum = dvec, *dacc = dvec + 4, *dt = dacc + nacc, *dbeta = dt + MPU, *dkd = dvec + head, *dalpha = dkd + chunk, *de = dalpha + chunk,
           *dgval = de + chunk;
    int32_t *d_bad = reinterpret_cast<int32_t *>(dvec + 2);
    GradPartials hzz(grad_reduce_blocks(M));
    if (total > 0) {
        const int64_t nblk = kgrad_rect_blocks(chunk < N ? chunk : N, M);
        GPT_TRY(ensure(c, SLOT_SP_GPART, (size_t)nblk * GPT_GRAD_MAXH * sizeof(double), (void **)&dpart));
        GPT_TRY(ensure(c, SLOT_GPART, hzz.bytes(), (void **)&dzz));
        GPT_TRY(ensure(c, SLOT_GKP, 2 * kp1.size() * sizeof(KParams), (void **)&dkp));
        GPT_HIP_CHECK(hipMemcpyAsync(dkp, kp1.data(), kp1.size() * sizeof(KParams), hipMemcpyHostToDevice, st));
        GPT_HIP_CHECK(hipMemcpyAsync(dkp + kp1.size(), kp2.data(), kp2.size() * sizeof(KParams), hipMemcpyHostToDevice, st));
    }
    if (adj && method == GPT_SPARSE_FITC) GPT_TRY(sparse_part(c, nslices, ME, &dPart));
    if (dz_out) {
        // the row tiles' partial sums of one launch_kgrad_dz -- a chunk against Z, or Z against Z -- and the running dz (M x D)
        const int64_t crows = chunk < N ? chunk : N, ntile = kgrad_dz_tiles(crows > M ? crows : M);
        GPT_TRY(ensure(c, SLOT_SP_DZPART, (size_t)ntile * M * D * sizeof(double), (void **)&dzpart));
        GPT_TRY(ensure(c, SLOT_SP_DZ, (size_t)M * D * sizeof(double), (void **)&ddz));
        GPT_HIP_CHECK(hipMemsetAsync(ddz, 0, (size_t)M * D * sizeof(double), st));
    }
    const KParams *dkp2 = dkp ? dkp + kp1.size() : nullptr;
    GPT_TRY(sparse_upload_y(c, st, y, err_y, N, &dY));
    GPT_HIP_CHECK(hipMemsetAsync(dvec, 0, head * sizeof(double), st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));      // (pageable sources: the vectors may not change before the copies are through)
    // ---- once, at order M: U_B = L_B^-T (the identity through the right-side solve, as gpt_dev_trinv), t = U_B c, beta = U_u t
    GPT_TRY(launch_zero2d(st, BP, BP, T0, BP));
    hipLaunchKernelGGL(eye_blocks_kernel, dim3((unsigned)((BP + 255) / 256)), dim3(256), 0, st, T0, BP, BP, (int64_t)0);
    GPT_LAUNCH_CHECK();
    GPT_TRY(trsm_rlt(c, st, BP, BP, dLb, BP, ws_b, T0, BP));
    GPT_TRY(launch_zero2d(st, MPU, MPU, T1, MPU));                   // (the leading M x M block alone: no augmented row or column)
    GPT_TRY(launch_copy2d(st, M, M, T0, BP, T1, MPU));
    GPT_TRY(launch_gemv_n(st, M, M, T1, MPU, d_c, dt));
    if (adj) {
        GPT_TRY(launch_zero2d(st, MPU, MPU, Uu, MPU));
        hipLaunchKernelGGL(eye_blocks_kernel, dim3((unsigned)((MPU + 255) / 256)), dim3(256), 0, st, Uu, MPU, MPU, (int64_t)0);
        GPT_LAUNCH_CHECK();
        GPT_TRY(trsm_rlt(c, st, MPU, MPU, dLu, MPU, ws_u, Uu, MPU));
        GPT_TRY(launch_gemv_n(st, M, M, Uu, MPU, dt, dbeta));
        // B^-1 = U_B U_B^T (whole, symmetric) and the second operand of the chunks' GEMMs, P2 = U_u B^-1
        GPT_TRY(gemm_nt(c, st, MPU, MPU, MPU, 1.0, T1, MPU, T1, MPU, 0.0, Binv, MPU, 0));
        GPT_TRY(gemm_nt(c, st, MPU, MPU, MPU, 1.0, Uu, MPU, Binv, MPU, 0.0, P2, MPU, 0));
        if (method == GPT_SPARSE_FITC) GPT_TRY(launch_zero2d(st, ME, ME, dE, ME));
        // (rows past a chunk's end take part in the GEMMs and are never read: they hold finite numbers from here on)
        GPT_HIP_CHECK(hipMemsetAsync(dS1, 0, (size_t)chunk * LDV * sizeof(double), st));
        GPT_HIP_CHECK(hipMemsetAsync(dS2, 0, (size_t)chunk * LDV * sizeof(double), st));
    }
    // ---- the chunks, in ascending order
    for (int64_t r0 = 0; r0 < N; r0 += chunk) {
        const int64_t rows = (N - r0 < chunk) ? N - r0 : chunk, CP = round_up(rows, 64);
        const double *dXc = c->dX + r0 * D;
        const int32_t *dnc = c->dn + r0 * D;
        GPT_TRY(sparse_chunk_vw(c, st, model, res, dXc, dnc, rows, dV, dW));
        if (method != GPT_SPARSE_DTC) GPT_TRY(sparse_kdiag(st, model, dXc, dnc, rows, dkd));
        GPT_TRY(launch_sparse_grad_rows(st, dV, dW, LDV, rows, M, method, dkd, dY + r0, dY + N + r0, c->sp_noise_var, dt, dalpha, de, dgval,
                                        chunk, dS1, dS2, d_bad));
        GPT_TRY(launch_sparse_rowsum(st, dgval, chunk, rows, dsum));
        if (alpha_out) GPT_HIP_CHECK(hipMemcpyAsync(alpha_out + r0, dalpha, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, st));
        if (!adj) continue;
        // A_fu of the chunk, in the place of W^T
        GPT_TRY(gemm_nt(c, st, CP, MPU, MPU, -1.0, dS1, LDV, P2, MPU, 0.0, dW, LDV, 0));
        if (method != GPT_SPARSE_DTC) GPT_TRY(gemm_nt(c, st, CP, MPU, MPU, -1.0, dS2, LDV, Uu, MPU, 1.0, dW, LDV, 0));
        GPT_TRY(launch_sparse_rank1(st, dW, LDV, rows, M, dalpha, dbeta));
        if (dz_out)
            for (int t = 0; t < model.nterms; t++)
                GPT_TRY(launch_kgrad_dz(st, model.f1[t].kernel_id, model.second(t) ? model.f2[t].kernel_id : -1, D, model.f1[t], model.second(t),
                                        dXc, dnc, rows, dZ, dnZ, M, dW, LDV, 0, dzpart, ddz));
        GPT_TRY(for_each_group(gs, [&](int b0, int cnt, int t) {
            return launch_kgrad_rect_diff(st, model.f1[t].kernel_id, model.second(t) ? model.f2[t].kernel_id : -1, D, dkp + 2 * b0, dkp2 + 2 * b0,
                                          cnt, dXc, dnc, rows, dZ, dnZ, M, dW, LDV, method != GPT_SPARSE_DTC ? de : nullptr, dpart, dacc + b0);
        }));
        if (method == GPT_SPARSE_FITC) GPT_TRY(launch_sparse_gram(st, dS2, dV, LDV, rows, ME, nslices, dPart, dE, ME));
    }
    std::vector<double> hacc(nacc, 0.0), zz((size_t)total, 0.0);
    if (adj) {
        // ---- A_uu: S = U_u (I - B^-1 + V diag(e) V^T) U_u^T, then the Z-Z pair pass with beta for alpha and S for W
        if (method == GPT_SPARSE_VFE) {
            GPT_TRY(launch_sparse_tril(st, dLb, BP, M, T0, MPU, MPU));
            GPT_TRY(gemm_nt(c, st, MPU, MPU, MPU, 1.0, T0, MPU, T0, MPU, 0.0, T1, MPU, 0));      // B = L_B L_B^T
            GPT_TRY(launch_sparse_grad_mid(st, Binv, MPU, T1, MPU, M, 1, T2, MPU));
        } else {
            GPT_TRY(launch_sparse_grad_mid(st, Binv, MPU, method == GPT_SPARSE_FITC ? dE : nullptr, ME, M, method == GPT_SPARSE_FITC ? 0 : 2, T2,
                                           MPU));
        }
        GPT_TRY(gemm_nt(c, st, MPU, MPU, MPU, 1.0, Uu, MPU, T2, MPU, 0.0, T0, MPU, 0));
        GPT_TRY(gemm_nt(c, st, MPU, MPU, MPU, 1.0, T0, MPU, Uu, MPU, 0.0, T1, MPU, 1));
        GPT_TRY(for_each_group(gs, [&](int b0, int cnt, int t) -> int {
            GPT_TRY(launch_kgrad_diff(st, model.f1[t].kernel_id, model.second(t) ? model.f2[t].kernel_id : -1, D, dkp + 2 * b0, dkp2 + 2 * b0, cnt,
                                      dZ, dnZ, M, dbeta, T1, MPU, dzz, 1, nullptr));
            GPT_TRY(hzz.fetch(st, dzz));
            for (int q = 0; q < cnt; q++) zz[b0 + q] = 0.5 * hzz.sum(q);
            return GPT_OK;
        }));
        if (total > 0) GPT_HIP_CHECK(hipMemcpyAsync(hacc.data(), dacc, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, st));
        if (dz_out) {
            // ---- the Z-Z pass: 2 A_uu = S - beta beta^T whole (S stands in T1's lower triangle), the same kernel with X := Z and without
            // the pairs m' = m
            GPT_TRY(launch_sparse_auu2(st, T1, MPU, M, dbeta, T2, MPU));
            for (int t = 0; t < model.nterms; t++)
                GPT_TRY(launch_kgrad_dz(st, model.f1[t].kernel_id, model.second(t) ? model.f2[t].kernel_id : -1, D, model.f1[t], model.second(t),
                                        dZ, dnZ, M, dZ, dnZ, M, T2, MPU, 1, dzpart, ddz));
            GPT_HIP_CHECK(hipMemcpyAsync(dz_out, ddz, (size_t)M * D * sizeof(double), hipMemcpyDeviceToHost, st));
        }
    }
    double sums[2];
    int32_t bad = 0;
    GPT_HIP_CHECK(hipMemcpyAsync(sums, dsum, sizeof(sums), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    if (bad != 0) {
        gpt_set_error("%s: a Lambda_i is not a positive finite number", who);
        return GPT_E_VALUE;
    }
    // sum A_uu dK_uu = -1/2 sum (beta beta^T - S) dK_uu: the Z-Z pass, negated
    for (int q = 0; q < total; q++) out[where[q]] = (hacc[q] - zz[q]) / denom[where[q]];
    out[nh] = sums[0];
    return GPT_OK;
}

extern "C" int gpt_sparse_grad_diff(gpt_ctx *c, int nh, const int *term_idx, const double *params_a, const double *params_b,
                                    const double *denom, const double *y, const double *err_y, double *out, double *alpha_out)
{
    CTX_ENTER(c);
    return sparse_grad_body(c, "gpt_sparse_grad_diff", nh, term_idx, params_a, params_b, denom, y, err_y, out, alpha_out, nullptr);
}

// gpt_sparse_grad_diff and, from the same pass, d ll / d Z (DESIGN.md 18.9): dz_out (M x D, row-major, host) receives
//     sum_i A_fu[i,m] k(x_i, z_m; n_i, n_m + e_d) + 2 sum_{m' != m} A_uu[m',m] k(z_m', z_m; n_m', n_m + e_d)
// over the model's terms -- the running sums of the device, nothing divided by a step.  A non-finite entry is returned as it is.
extern "C" int gpt_sparse_grad_z(gpt_ctx *c, int nh, const int *term_idx, const double *params_a, const double *params_b, const double *denom,
                                 const double *y, const double *err_y, double *out, double *alpha_out, double *dz_out)
{
    CTX_ENTER(c);
    if (!dz_out) {
        gpt_set_error("gpt_sparse_grad_z: bad arguments (dz_out is NULL: gpt_sparse_grad_diff is that call)");
        return GPT_E_ARG;
    }
    return sparse_grad_body(c, "gpt_sparse_grad_z", nh, term_idx, params_a, params_b, denom, y, err_y, out, alpha_out, dz_out);
}

// ---- the kernels of the gradient on raw device pointers (device API, on the context's stream) ------------------------------------------
// sparse_grad_rows_kernel (ksparse.hip): nothing added but the refusal of null pointers and of orders the launcher would read or write
// past.  dV, dW, dS1, dS2: rows x ld; d_t: M; d_alpha, d_e: rows; d_gval: 2 x ldr.
extern "C" int gpt_dev_sparse_grad_rows(gpt_ctx *c, const double *dV, const double *dW, int64_t ld, int64_t rows, int64_t M, int method,
                                        const double *d_kdiag, const double *d_r, const double *d_err, double noise_var, const double *d_t,
                                        double *d_alpha, double *d_e, double *d_gval, int64_t ldr, double *dS1, double *dS2, int32_t *d_bad)
{
    CTX_ENTER(c);
    if (!dV || !dW || !d_kdiag || !d_r || !d_err || !d_t || !d_alpha || !d_e || !d_gval || !dS1 || !dS2 || !d_bad || rows <= 0 || M < 1 ||
        method < GPT_SPARSE_FITC || method > GPT_SPARSE_DTC) {
        gpt_set_error("gpt_dev_sparse_grad_rows: bad arguments (rows=%lld, M=%lld, method %d)", (long long)rows, (long long)M, method);
        return GPT_E_ARG;
    }
    return launch_sparse_grad_rows(c->stream, dV, dW, ld, rows, M, method, d_kdiag, d_r, d_err, noise_var, d_t, d_alpha, d_e, d_gval, ldr, dS1,
                                   dS2, d_bad);
}

// The rectangular pair pass alone: out[h] = sum_im dA[i][m] (k_b - k_a)(x_i, z_m) + 1/2 sum_i d_e[i] (k_b - k_a)(x_i, x_i), h < nh (any
// number: GPT_GRAD_MAXH per launch), for ONE term kernel_id (* kernel_id2 where >= 0) of num_dim D with nparams parameters (nparams1 of
// them the first factor's) at the stencil points params_a / params_b (nh x nparams each, host).  max_order: the largest sum of
// derivative orders of a point among dX and dZ (the order rules of parse_model).  d_e NULL: no diagonal part.  Not divided by a step.
extern "C" int gpt_dev_sparse_grad_pairs(gpt_ctx *c, int kernel_id, int kernel_id2, int D, int max_order, int nh, const double *params_a,
                                         const double *params_b, int nparams, int nparams1, const double *dX, const int32_t *dnx, int64_t rows,
                                         const double *dZ, const int32_t *dnz, int64_t M, const double *dA, int64_t lda, const double *d_e,
                                         double *out)
{
    CTX_ENTER(c);
    if (nh < 1 || !params_a || !params_b || !out || nparams < 1 || max_order < 0 || D < 1 || D > GPT_MAX_DIM) {
        gpt_set_error("gpt_dev_sparse_grad_pairs: bad arguments");
        return GPT_E_ARG;
    }
    long colmax[GPT_MAX_DIM];
    for (int d = 0; d < GPT_MAX_DIM; d++) colmax[d] = max_order;
    // nh entries of a model of this one term: no steps to check, and the launch order is the caller's
    ModelKernel one_term;
    one_term.nterms = 1;
    one_term.abi_id1[0] = kernel_id;
    one_term.abi_id2[0] = kernel_id2;
    one_term.np[0] = nparams;
    one_term.np1[0] = nparams1;
    const std::vector<int> term_idx((size_t)nh, 0);
    GradStencil gs;
    GPT_TRY(grad_stencil_build("gpt_dev_sparse_grad_pairs", D, max_order, colmax, one_term, nh, term_idx.data(), params_a, params_b, nullptr, &gs));
    const std::vector<KParams> &kp1 = gs.kp1, &kp2 = gs.kp2;
    hipStream_t st = c->stream;
    KParams *dkp;
    double *dpart, *dacc;
    GPT_TRY(ensure(c, SLOT_GKP, 2 * kp1.size() * sizeof(KParams), (void **)&dkp));
    GPT_TRY(ensure(c, SLOT_SP_GPART, ((size_t)kgrad_rect_blocks(rows > 0 ? rows : 1, M > 0 ? M : 1) * GPT_GRAD_MAXH + (size_t)nh) * sizeof(double),
                   (void **)&dpart));
    dacc = dpart + kgrad_rect_blocks(rows > 0 ? rows : 1, M > 0 ? M : 1) * GPT_GRAD_MAXH;
    GPT_HIP_CHECK(hipMemcpyAsync(dkp, kp1.data(), kp1.size() * sizeof(KParams), hipMemcpyHostToDevice, st));
    GPT_HIP_CHECK(hipMemcpyAsync(dkp + kp1.size(), kp2.data(), kp2.size() * sizeof(KParams), hipMemcpyHostToDevice, st));
    GPT_HIP_CHECK(hipMemsetAsync(dacc, 0, (size_t)nh * sizeof(double), st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    const KParams &f1 = kp1[0], &f2 = kp2[0];
    GPT_TRY(for_each_group(gs, [&](int b0, int cnt, int) {
        return launch_kgrad_rect_diff(st, f1.kernel_id, f2.kernel_id >= 0 ? f2.kernel_id : -1, D, dkp + 2 * b0, dkp + kp1.size() + 2 * b0, cnt, dX,
                                      dnx, rows, dZ, dnz, M, dA, lda, d_e, dpart, dacc + b0);
    }));
    GPT_HIP_CHECK(hipMemcpyAsync(out, dacc, (size_t)nh * sizeof(double), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    return GPT_OK;
}

// launch_kgrad_dz alone for ONE term, kernel_id (* kernel_id2 where >= 0) of num_dim D with nparams parameters (nparams1 of them the first
// factor's) at `params` (host): out[m][d] = sum_i dA[i][m] k(x_i, z_m; n_i, n_m + e_d), written, not accumulated (M x D, host).  max_order:
// the largest sum of derivative orders of a point of the pass, the raised n_Z + e_d included (the order rules of parse_model).
// skip_diag: without the pairs i == m.
extern "C" int gpt_dev_sparse_grad_dz_pairs(gpt_ctx *c, int kernel_id, int kernel_id2, int D, int max_order, const double *params, int nparams,
                                            int nparams1, const double *dX, const int32_t *dnx, int64_t rows, const double *dZ,
                                            const int32_t *dnz, int64_t M, const double *dA, int64_t lda, int skip_diag, double *out)
{
    CTX_ENTER(c);
    if (!params || !out || nparams < 1 || max_order < 0 || D < 1 || D > GPT_MAX_DIM || rows <= 0 || M <= 0) {
        gpt_set_error("gpt_dev_sparse_grad_dz_pairs: bad arguments");
        return GPT_E_ARG;
    }
    long colmax[GPT_MAX_DIM];
    for (int d = 0; d < GPT_MAX_DIM; d++) colmax[d] = max_order;
    ModelKernel one;
    GPT_TRY(parse_model(D, max_order, colmax, 1, &kernel_id, kernel_id2 >= 0 ? &kernel_id2 : nullptr, params, &nparams, &nparams1, &one));
    hipStream_t st = c->stream;
    double *dzpart, *ddz;
    GPT_TRY(ensure(c, SLOT_SP_DZPART, (size_t)kgrad_dz_tiles(rows) * M * D * sizeof(double), (void **)&dzpart));
    GPT_TRY(ensure(c, SLOT_SP_DZ, (size_t)M * D * sizeof(double), (void **)&ddz));
    GPT_HIP_CHECK(hipMemsetAsync(ddz, 0, (size_t)M * D * sizeof(double), st));
    GPT_TRY(launch_kgrad_dz(st, one.f1[0].kernel_id, one.second(0) ? one.f2[0].kernel_id : -1, D, one.f1[0], one.second(0), dX, dnx, rows, dZ, dnz,
                            M, dA, lda, skip_diag, dzpart, ddz));
    GPT_HIP_CHECK(hipMemcpyAsync(out, ddz, (size_t)M * D * sizeof(double), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    return GPT_OK;
}
