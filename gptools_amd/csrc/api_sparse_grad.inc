// api_sparse_grad.inc -- part of api.hip (ONE translation unit: included from there, in this order; the parts share struct gpt_ctx and
// static helpers).  The gradient of the inducing-point objective (DESIGN.md section 18.8): gpt_sparse_grad_diff, and the device API of
// its kernels, gpt_dev_sparse_grad_rows / _gram2 / _grad_pairs.
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

// The stencil points of nh entries, term by term, as grad_diff_run parses them (api_grad.inc): kp1 / kp2 hold [a, b] per parameter in
// launch order, where[] the caller's index of each, term_of[] its term
static int sparse_grad_stencil(const char *who, int D, long maxsum, const long *colmax, const ModelKernel &m, int nh, const int *term_idx,
                               const double *params_a, const double *params_b, const double *denom, std::vector<KParams> *kp1,
                               std::vector<KParams> *kp2, std::vector<int> *where, std::vector<int> *term_of)
{
    std::vector<size_t> off((size_t)nh + 1, 0);
    for (int h = 0; h < nh; h++) {
        if (term_idx[h] < 0 || term_idx[h] >= m.nterms) return GPT_E_ARG;
        if (!(denom[h] != 0.0) || std::isinf(denom[h])) {
            gpt_set_error("%s: denom[%d] = %g", who, h, denom[h]);
            return GPT_E_ARG;
        }
        off[h + 1] = off[h] + (size_t)m.np[term_idx[h]];
    }
    for (int t = 0; t < m.nterms; t++)
        for (int h = 0; h < nh; h++) {
            if (term_idx[h] != t) continue;
            const bool prod = m.abi_id2[t] >= 0;
            for (const double *p : {params_a + off[h], params_b + off[h]}) {
                ModelKernel one;
                GPT_TRY(parse_model(D, maxsum, colmax, 1, &m.abi_id1[t], prod ? &m.abi_id2[t] : nullptr, p, &m.np[t],
                                    prod ? &m.np1[t] : nullptr, &one));
                kp1->push_back(one.f1[0]);
                kp2->push_back(one.f2[0]);
            }
            where->push_back(h);
            term_of->push_back(t);
        }
    return GPT_OK;
}

extern "C" int gpt_sparse_grad_diff(gpt_ctx *c, int nh, const int *term_idx, const double *params_a, const double *params_b,
                                    const double *denom, const double *y, const double *err_y, double *out, double *alpha_out)
{
    CTX_ENTER(c);
    GPT_TRY(sparse_refusals(c, "gpt_sparse_grad_diff", true));
    if (nh < 0 || (nh > 0 && (!term_idx || !params_a || !params_b || !denom)) || !y || !err_y || !out) {
        gpt_set_error("gpt_sparse_grad_diff: bad arguments");
        return GPT_E_ARG;
    }
    const ModelKernel &model = c->sp_model;
    const int D = c->D, method = c->sp_method;
    const int64_t N = c->Nx;
    long maxsum, colmax[GPT_MAX_DIM];
    sparse_order_bounds(c, &maxsum, colmax);
    std::vector<KParams> kp1, kp2;
    std::vector<int> where, term_of;
    GPT_TRY(sparse_grad_stencil("gpt_sparse_grad_diff", D, maxsum, colmax, model, nh, term_idx, params_a, params_b, denom, &kp1, &kp2, &where,
                                &term_of));
    const int total = (int)where.size();
    const SparseDims sd = sparse_dims(c->sp_M);
    const int64_t M = sd.M, MPU = sd.MPU, BP = sd.BP, LDV = sd.LDV, ME = round_up(M, 64);
    int64_t chunk;
    GPT_TRY(sparse_chunk(sd, c->sp_chunk_rows, N, &chunk, 4));
    int nslices = 1;
    if (method == GPT_SPARSE_FITC) GPT_TRY(sparse_slices(c, ME, chunk < N ? chunk : N, &nslices));
    const int64_t ntiles = (ME / 64) * (ME / 64 + 1) / 2;
    hipStream_t st = c->stream;
    const double *dLu = (const double *)c->slots[SLOT_SP_LU].p, *dLb = (const double *)c->slots[SLOT_SP_LB].p;
    const double *ws_u = dLu + MPU * MPU, *ws_b = dLb + BP * BP, *d_c = ws_b + (BP / 128) * GPT_WS_BLOCK;
    const double *dZ = sparse_Z(c);
    const int32_t *dnZ = sparse_nZ(c);
    double *dV, *dW, *dS1, *dS2, *dGM, *dvec, *dY, *dPart = nullptr, *dpart = nullptr, *dzz = nullptr;
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
    GPT_TRY(ensure(c, SLOT_SP_Y, (size_t)2 * N * sizeof(double), (void **)&dY));
    const int nblk_zz = grad_reduce_blocks(M);
    if (total > 0) {
        const int64_t nblk = kgrad_rect_blocks(chunk < N ? chunk : N, M);
        GPT_TRY(ensure(c, SLOT_SP_GPART, (size_t)nblk * GPT_GRAD_MAXH * sizeof(double), (void **)&dpart));
        GPT_TRY(ensure(c, SLOT_GPART, (size_t)nblk_zz * (GPT_GRAD_MAXH + 1) * sizeof(double), (void **)&dzz));
        GPT_TRY(ensure(c, SLOT_GKP, 2 * kp1.size() * sizeof(KParams), (void **)&dkp));
        if (method == GPT_SPARSE_FITC)
            GPT_TRY(ensure(c, SLOT_SP_PART, (size_t)nslices * ntiles * 4096 * sizeof(double), (void **)&dPart));
        GPT_HIP_CHECK(hipMemcpyAsync(dkp, kp1.data(), kp1.size() * sizeof(KParams), hipMemcpyHostToDevice, st));
        GPT_HIP_CHECK(hipMemcpyAsync(dkp + kp1.size(), kp2.data(), kp2.size() * sizeof(KParams), hipMemcpyHostToDevice, st));
    }
    const KParams *dkp2 = dkp ? dkp + kp1.size() : nullptr;
    GPT_HIP_CHECK(hipMemcpyAsync(dY, y, (size_t)N * sizeof(double), hipMemcpyHostToDevice, st));
    GPT_HIP_CHECK(hipMemcpyAsync(dY + N, err_y, (size_t)N * sizeof(double), hipMemcpyHostToDevice, st));
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
    if (total > 0) {
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
        GPT_TRY(launch_zero2d(st, CP, LDV, dV, LDV));
        GPT_TRY(kbuild_terms(st, model, 0, dXc, dnc, rows, dZ, dnZ, M, 0, 0, 0, nullptr, 0.0, 0.0, dV, LDV));
        GPT_TRY(trsm_rlt(c, st, CP, MPU, dLu, MPU, ws_u, dV, LDV));
        GPT_TRY(launch_copy2d(st, CP, LDV, dV, LDV, dW, LDV));
        GPT_TRY(trsm_rlt(c, st, CP, BP, dLb, BP, ws_b, dW, LDV));      // (column M: the augmented row's, not read)
        if (method != GPT_SPARSE_DTC) GPT_TRY(sparse_kdiag(st, model, dXc, dnc, rows, dkd));
        GPT_TRY(launch_sparse_grad_rows(st, dV, dW, LDV, rows, M, method, dkd, dY + r0, dY + N + r0, c->sp_noise_var, dt, dalpha, de, dgval,
                                        chunk, dS1, dS2, d_bad));
        GPT_TRY(launch_sparse_rowsum(st, dgval, chunk, rows, dsum));
        if (alpha_out) GPT_HIP_CHECK(hipMemcpyAsync(alpha_out + r0, dalpha, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, st));
        if (total == 0) continue;
        // A_fu of the chunk, in the place of W^T
        GPT_TRY(gemm_nt(c, st, CP, MPU, MPU, -1.0, dS1, LDV, P2, MPU, 0.0, dW, LDV, 0));
        if (method != GPT_SPARSE_DTC) GPT_TRY(gemm_nt(c, st, CP, MPU, MPU, -1.0, dS2, LDV, Uu, MPU, 1.0, dW, LDV, 0));
        GPT_TRY(launch_sparse_rank1(st, dW, LDV, rows, M, dalpha, dbeta));
        for (int b0 = 0; b0 < total;) {
            const int t = term_of[b0];
            int cnt = 0;
            while (b0 + cnt < total && cnt < GPT_GRAD_MAXH && term_of[b0 + cnt] == t) cnt++;
            GPT_TRY(launch_kgrad_rect_diff(st, model.f1[t].kernel_id, model.second(t) ? model.f2[t].kernel_id : -1, D, dkp + 2 * b0, dkp2 + 2 * b0,
                                           cnt, dXc, dnc, rows, dZ, dnZ, M, dW, LDV, method != GPT_SPARSE_DTC ? de : nullptr, dpart, dacc + b0));
            b0 += cnt;
        }
        if (method == GPT_SPARSE_FITC) GPT_TRY(launch_sparse_gram2(st, dS2, dV, LDV, rows, ME, nslices, dPart, dE, ME));
    }
    std::vector<double> hacc(nacc, 0.0), zz((size_t)total, 0.0);
    if (total > 0) {
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
        std::vector<double> hpart((size_t)nblk_zz * (GPT_GRAD_MAXH + 1));
        for (int b0 = 0; b0 < total;) {
            const int t = term_of[b0];
            int cnt = 0;
            while (b0 + cnt < total && cnt < GPT_GRAD_MAXH && term_of[b0 + cnt] == t) cnt++;
            GPT_TRY(launch_kgrad_diff(st, model.f1[t].kernel_id, model.second(t) ? model.f2[t].kernel_id : -1, D, dkp + 2 * b0, dkp2 + 2 * b0, cnt,
                                      dZ, dnZ, M, dbeta, T1, MPU, dzz, 1, nullptr));
            GPT_HIP_CHECK(hipMemcpyAsync(hpart.data(), dzz, hpart.size() * sizeof(double), hipMemcpyDeviceToHost, st));
            GPT_HIP_CHECK(hipStreamSynchronize(st));
            for (int q = 0; q < cnt; q++) {
                double sum = 0.0;
                for (int b = 0; b < nblk_zz; b++) sum += hpart[(size_t)b * (GPT_GRAD_MAXH + 1) + q];
                zz[b0 + q] = 0.5 * sum;
            }
            b0 += cnt;
        }
        GPT_HIP_CHECK(hipMemcpyAsync(hacc.data(), dacc, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    double sums[2];
    int32_t bad = 0;
    GPT_HIP_CHECK(hipMemcpyAsync(sums, dsum, sizeof(sums), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    if (bad != 0) {
        gpt_set_error("gpt_sparse_grad_diff: a Lambda_i is not a positive finite number");
        return GPT_E_VALUE;
    }
    // sum A_uu dK_uu = -1/2 sum (beta beta^T - S) dK_uu: the Z-Z pass, negated
    for (int q = 0; q < total; q++) out[where[q]] = (hacc[q] - zz[q]) / denom[where[q]];
    out[nh] = sums[0];
    return GPT_OK;
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

// dG (mg x mg, lower 64 x 64 tiles) += dA^T dV over `rows` rows (both rows x ldv).  nslices = 0: the fit's own choice.
extern "C" int gpt_dev_sparse_gram2(gpt_ctx *c, const double *dA, const double *dV, int64_t ldv, int64_t rows, int64_t mg, int nslices,
                                    double *dG, int64_t ldg)
{
    CTX_ENTER(c);
    if (!dA || !dV || !dG || rows <= 0 || mg <= 0 || mg % 64) {
        gpt_set_error("gpt_dev_sparse_gram2: bad arguments (rows=%lld, order %lld: a positive multiple of 64)", (long long)rows, (long long)mg);
        return GPT_E_ARG;
    }
    if (nslices <= 0) GPT_TRY(sparse_slices(c, mg, rows, &nslices));
    const int64_t ntiles = (mg / 64) * (mg / 64 + 1) / 2;
    double *dPart;
    GPT_TRY(ensure(c, SLOT_SP_PART, (size_t)nslices * ntiles * 4096 * sizeof(double), (void **)&dPart));
    return launch_sparse_gram2(c->stream, dA, dV, ldv, rows, mg, nslices, dPart, dG, ldg);
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
    std::vector<KParams> kp1, kp2;
    for (int h = 0; h < nh; h++)
        for (const double *p : {params_a + (size_t)h * nparams, params_b + (size_t)h * nparams}) {
            ModelKernel one;
            GPT_TRY(parse_model(D, max_order, colmax, 1, &kernel_id, kernel_id2 >= 0 ? &kernel_id2 : nullptr, p, &nparams,
                                kernel_id2 >= 0 ? &nparams1 : nullptr, &one));
            kp1.push_back(one.f1[0]);
            kp2.push_back(one.f2[0]);
        }
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
    for (int b0 = 0; b0 < nh; b0 += GPT_GRAD_MAXH) {
        const int cnt = nh - b0 < GPT_GRAD_MAXH ? nh - b0 : GPT_GRAD_MAXH;
        GPT_TRY(launch_kgrad_rect_diff(st, f1.kernel_id, f2.kernel_id >= 0 ? f2.kernel_id : -1, D, dkp + 2 * b0, dkp + kp1.size() + 2 * b0, cnt, dX,
                                       dnx, rows, dZ, dnz, M, dA, lda, d_e, dpart, dacc + b0));
    }
    GPT_HIP_CHECK(hipMemcpyAsync(out, dacc, (size_t)nh * sizeof(double), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    return GPT_OK;
}
