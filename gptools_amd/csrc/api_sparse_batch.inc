// api_sparse_batch.inc -- part of api.hip (ONE translation unit: included from there, behind api_sparse.inc).  gpt_sparse_fit_batch: nbatch
// evaluations of the inducing-point objective in one launch sequence, and the device API of its four batched kernel groups
// (gpt_dev_sparse_*_batch).  DESIGN.md section 18.11.
// ------------------------------------------------------------------------------------------------
// Layout.  Element b of the batch has the dimensions of the single fit (api_sparse.inc: MPU, BP, LDV, MG) and, in slots of its own,
//   SLOT_SPB_LU    its K_uu + jitter I / L_u at b MPU^2, behind the nbatch matrices the leaves' packed workspaces, b (MPU / 128) blocks;
//   SLOT_SPB_LB    its B / L_B at b BP^2 and the workspaces likewise;
//   SLOT_SPB_V     its chunk buffer at b chunk LDV (chunk: the rows per pass of the single fit for the same chunk_rows);
//   SLOT_SPB_G     its Gram at b MG^2;  SLOT_SPB_PART its (slices x tiles) partial tiles;
//   SLOT_SPB_MISC  the small inputs and per-row values (below).
// The chain is gpt_sparse_fit's with every kernel carrying the batch in a grid dimension: the batched builders (kbuild_batch.hip), the
// leaf loop of gpt_fit_batch* (batch_leaf_loop), trsm_rlt's recursion on batched launches, the batched row pass, sums, Gram and assembly
// (ksparse.hip: the single fit's kernel sources, run with strides) and launch_batch_logdet_dot.  Same kernels or kernels with the same
// arithmetic, the same chunk boundaries, the one slice partition (sparse_gram_slicing), the same summation orders and the one host
// expression (sparse_outcome, api_sparse.inc): an element's ll and parts carry the bits gpt_sparse_fit returns for it alone.  A failed
// element (K_uu, a Lambda_i, B) runs through the same launches on whatever its numbers have become; its words say so at the end and
// nobody else reads its buffers.
// ------------------------------------------------------------------------------------------------

// B_b (m x n per element, bstride apart) <- B_b L_b^-T, n a multiple of 128: trsm_rlt with every launch batched (L_b lstride apart, its
// leaves' workspaces wstride apart).  A copy of trsm_rlt's recursion, on purpose for now: the single form goes through gemm_nt(c, ...) with
// its flop accounting and schedule state, and folding the two belongs to a change of its own.
static int trsm_rlt_batch(hipStream_t st, int64_t nbatch, int64_t m, int64_t n, const double *L, int64_t ldl, int64_t lstride, const double *invd,
                          int64_t wstride, double *B, int64_t ldb, int64_t bstride)
{
    if (n == 128) return launch_trsm_panel(st, m, L, ldl, invd, B, ldb, nullptr, EdgeSig(), nbatch, bstride, wstride);
    const int64_t h = (n / 256) * 128 > 0 ? (n / 256) * 128 : 128;
    GPT_TRY(trsm_rlt_batch(st, nbatch, m, h, L, ldl, lstride, invd, wstride, B, ldb, bstride));
    GPT_TRY(launch_gemm_nt(st, m, n - h, h, -1.0, B, ldb, L + h * ldl, ldl, 1.0, B + h, ldb, 0, 0, 0, nullptr, nullptr, 0, EdgeSig(), EdgeSig(), 0,
                           nbatch, bstride, EdgeSig(), lstride, bstride));
    return trsm_rlt_batch(st, nbatch, m, n - h, L + h * ldl + h, ldl, lstride, invd + (h / 128) * GPT_WS_BLOCK, wstride, B + h, ldb, bstride);
}

extern "C" int gpt_sparse_fit_batch(gpt_ctx *c, int nbatch, int method, int nterms, const int *kernel_ids, const int *kernel_ids2,
                                    const double *params, const int *nparams, const int *nparams1, const double *noise_var, const double *y,
                                    const double *err_y, double jitter, int64_t chunk_rows, double *ll_out, double *parts_out,
                                    int32_t *info_out, int32_t *which_out)
{
    CTX_ENTER(c);
    GPT_TRY(sparse_refusals(c, "gpt_sparse_fit_batch", false));
    if (nbatch < 1 || nbatch > 65535) {
        gpt_set_error("gpt_sparse_fit_batch: nbatch must lie in 1 ... 65535, got %d", nbatch);
        return GPT_E_ARG;
    }
    if (!y || !err_y || !kernel_ids2 || !nparams1 || !noise_var || !ll_out || !info_out || !which_out) return GPT_E_ARG;
    GPT_TRY(sparse_fit_refusals("gpt_sparse_fit_batch", method, jitter, noise_var, nbatch));
    const int D = c->D;
    const int64_t N = c->Nx;
    long maxsum, colmax[GPT_MAX_DIM];
    sparse_order_bounds(c, &maxsum, colmax);
    // every element has the first one's kernels: its parse decides the layout (and refuses what any element's would)
    ModelKernel m0, mb;
    GPT_TRY(parse_model(D, maxsum, colmax, nterms, kernel_ids, kernel_ids2, params, nparams, nparams1, &m0));
    const SparseDims sd = sparse_dims(c->sp_M);
    const int64_t M = sd.M, MPU = sd.MPU, BP = sd.BP, LDV = sd.LDV, MG = sd.MG;
    int64_t chunk;
    GPT_TRY(sparse_chunk(sd, chunk_rows, N, &chunk));
    if (m0.has_m52) {
        std::vector<int32_t> hz((size_t)M * D);
        GPT_HIP_CHECK(hipMemcpy(hz.data(), sparse_nZ(c), hz.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        GPT_TRY(check_m52_orders(hz.data(), M, D));
    }
    int nslices;
    GPT_TRY(sparse_slices(c, MG, chunk < N ? chunk : N, &nslices));            // (of the single fit: not a function of nbatch)
    // pinned staging: [y: nbatch N | err: N | noise: nbatch | KParams: nterms x nbatch (| second factors: the same)] go to the device in
    // one copy; behind them the results [logdet, c.c, info of B, -: 4 nbatch | sums: 4 nbatch | words: 3 nbatch int32]
    const bool any_prod = m0.any_prod;
    static_assert(sizeof(KParams) % 8 == 0, "KParams is copied as an array of doubles");
    const size_t kp_doubles = sizeof(KParams) / 8, nb = (size_t)nbatch;
    const size_t nkp = (size_t)nterms * nb * kp_doubles * (any_prod ? 2 : 1);
    const size_t off_err = nb * N, off_nv = off_err + (size_t)N, off_kp = off_nv + nb, n_in = off_kp + nkp;
    const size_t off_res = n_in, off_sums = off_res + 4 * nb, off_words = off_sums + 4 * nb, n_host = off_words + (3 * nb + 1) / 2;
    const size_t need = n_host * sizeof(double);
    if (c->h_batch_cap < need) {
        if (c->h_batch) GPT_HIP_CHECK(hipHostFree(c->h_batch));
        c->h_batch = nullptr;
        c->h_batch_cap = 0;
        GPT_HIP_CHECK(hipHostMalloc((void **)&c->h_batch, need + need / 4, hipHostMallocDefault));
        c->h_batch_cap = need + need / 4;
    }
    double *h = c->h_batch;
    memcpy(h, y, nb * N * sizeof(double));
    memcpy(h + off_err, err_y, (size_t)N * sizeof(double));
    memcpy(h + off_nv, noise_var, nb * sizeof(double));
    char *hkp = reinterpret_cast<char *>(h + off_kp), *hkp2 = hkp + (size_t)nterms * nb * kp_doubles * 8;
    for (int b = 0; b < nbatch; b++) {
        if (b > 0) GPT_TRY(parse_model(D, maxsum, colmax, nterms, kernel_ids, kernel_ids2, params + (size_t)b * m0.nparams, nparams, nparams1, &mb));
        const ModelKernel &m = b > 0 ? mb : m0;
        for (int t = 0; t < nterms; t++) {                                  // term-major on the device: [t][b]
            memcpy(hkp + ((size_t)t * nb + (size_t)b) * kp_doubles * 8, &m.f1[t], sizeof(KParams));
            if (any_prod) memcpy(hkp2 + ((size_t)t * nb + (size_t)b) * kp_doubles * 8, &m.f2[t], sizeof(KParams));
        }
    }
    // device slots of the batch
    const int64_t us = MPU * MPU, uws = (MPU / 128) * GPT_WS_BLOCK, bs = BP * BP, bws = (BP / 128) * GPT_WS_BLOCK, vs = chunk * LDV, gs = MG * MG;
    const int64_t ps = sparse_gram_part_doubles(MG, nslices);
    double *dLu, *dLb, *dV, *dG, *dPart, *dmisc;
    GPT_TRY(ensure(c, SLOT_SPB_LU, nb * (size_t)(us + uws) * sizeof(double), (void **)&dLu));
    GPT_TRY(ensure(c, SLOT_SPB_LB, nb * (size_t)(bs + bws) * sizeof(double), (void **)&dLb));
    GPT_TRY(ensure(c, SLOT_SPB_V, nb * (size_t)vs * sizeof(double), (void **)&dV));
    GPT_TRY(ensure(c, SLOT_SPB_G, nb * (size_t)gs * sizeof(double), (void **)&dG));
    GPT_TRY(ensure(c, SLOT_SPB_PART, nb * (size_t)ps * sizeof(double), (void **)&dPart));
    double *dwsu = dLu + nb * us, *dwsb = dLb + nb * bs;
    // misc: the staged inputs as above, then (cleared in every call) [zeros: nbatch + MPU -- the noise and the err of K_uu's diagonal
    // epilogue | sums: 4 nbatch (0: sum log Lambda, 1: the VFE trace term) | words: info of K_uu, info of B, "a Lambda_i was not
    // positive", nbatch each | k(x_i, x_i): nbatch chunk], then the two per-row values, nbatch x 2 chunk
    const size_t d_zero = n_in, d_sums = d_zero + nb + (size_t)MPU, d_words = d_sums + 4 * nb, d_kd = d_words + (3 * nb + 1) / 2,
                 d_row = d_kd + nb * (size_t)chunk, d_end = d_row + 2 * nb * (size_t)chunk;
    GPT_TRY(ensure(c, SLOT_SPB_MISC, d_end * sizeof(double), (void **)&dmisc));
    const double *dY = dmisc, *derr = dmisc + off_err, *dnv = dmisc + off_nv;
    const KParams *dkp = reinterpret_cast<const KParams *>(dmisc + off_kp);
    const KParams *dkp2 = any_prod ? dkp + (size_t)nterms * nb : nullptr;
    const double *dzero_nv = dmisc + d_zero, *dzero_err = dzero_nv + nb;
    double *dsums = dmisc + d_sums, *dkd = dmisc + d_kd, *drow = dmisc + d_row;
    int32_t *dinfo_u = reinterpret_cast<int32_t *>(dmisc + d_words), *dinfo_b = dinfo_u + nb, *dbad = dinfo_b + nb;
    const double *dZ = sparse_Z(c);
    const int32_t *dnZ = sparse_nZ(c);
    EvalScope scope(c, true);                // (in flight like an evaluation for the flag-edge accounting; has no flag edges)
    // everything on the panel stream, as gpt_fit_batch*: unmasked, the main stream is idle here
    hipStream_t st = c->panel_stream;
    GPT_TRY(stream_follows(c, c->stream, st, 0));
    GPT_HIP_CHECK(hipMemcpyAsync(dmisc, h, n_in * sizeof(double), hipMemcpyHostToDevice, st));
    GPT_HIP_CHECK(hipMemsetAsync(dmisc + d_zero, 0, (d_row - d_zero) * sizeof(double), st));
    auto term_kp2 = [&](int t) -> const KParams * { return m0.second(t) ? dkp2 + (size_t)t * nb : nullptr; };
    const int gform = m0.gibbs_form();
    // ---- L_u = chol(k(Z, Z) + jitter I) of every element
    GPT_TRY(launch_zero2d(st, (int64_t)nbatch * MPU, MPU, dLu, MPU));
    for (int t = 0; t < nterms; t++)                                        // (as kbuild_terms: the last term carries the diagonal epilogue)
        GPT_TRY(launch_kbuild_batch(st, m0.f1[t].kernel_id, D, dkp + (size_t)t * nb, dzero_nv, nbatch, dZ, dnZ, M, t + 1 == nterms ? dzero_err : nullptr,
                                    jitter, dLu, MPU, us, t > 0 ? 1 : 0, 0, term_kp2(t), 0, nullptr, 0, gform));
    GPT_TRY(launch_sparse_unit_pad_batch(st, nbatch, dLu, MPU, us, M, MPU));
    GPT_TRY(batch_leaf_loop(st, MPU, dLu, us, dwsu, uws, dinfo_u, nbatch));
    // ---- the chunks, in ascending order
    GPT_TRY(launch_zero2d(st, (int64_t)nbatch * MG, MG, dG, MG));
    for (int64_t r0 = 0; r0 < N; r0 += chunk) {
        const int64_t rows = (N - r0 < chunk) ? N - r0 : chunk, CP = round_up(rows, 64);
        const double *dXc = c->dX + r0 * D;
        const int32_t *dnc = c->dn + r0 * D;
        if (CP == chunk) GPT_TRY(launch_zero2d(st, (int64_t)nbatch * chunk, LDV, dV, LDV));
        else
            for (int b = 0; b < nbatch; b++) GPT_TRY(launch_zero2d(st, CP, LDV, dV + (int64_t)b * vs, LDV));
        for (int t = 0; t < nterms; t++)
            GPT_TRY(launch_kbuild_batch_cross(st, m0.f1[t].kernel_id, D, dkp + (size_t)t * nb, dnv, nbatch, dXc, dnc, rows, dZ, dnZ, M, dV, LDV, vs,
                                              t > 0 ? 1 : 0, term_kp2(t), gform));
        GPT_TRY(trsm_rlt_batch(st, nbatch, CP, MPU, dLu, MPU, us, dwsu, uws, dV, LDV, vs));
        if (method != GPT_SPARSE_DTC) GPT_TRY(launch_kdiag_batch(st, D, nterms, dkp, dkp2, nbatch, dXc, dnc, rows, dkd, chunk, gform));
        GPT_TRY(launch_sparse_lambda_batch(st, nbatch, dV, LDV, vs, rows, M, method, dkd, chunk, dY + r0, N, derr + r0, dnv, drow, chunk, 2 * chunk,
                                           dbad));
        GPT_TRY(launch_sparse_rowsum_batch(st, nbatch, drow, chunk, 2 * chunk, rows, dsums, 4));
        GPT_TRY(launch_sparse_gram_batch(st, nbatch, dV, LDV, vs, rows, MG, nslices, dPart, ps, dG, MG, gs));
    }
    // ---- B = I + G, augmented; L_B; the scalars
    GPT_TRY(launch_sparse_assemble_b_batch(st, nbatch, dG, MG, gs, M, dLb, BP, bs, 1e300));
    GPT_TRY(batch_leaf_loop(st, BP, dLb, bs, dwsb, bws, dinfo_b, nbatch));
    GPT_TRY(launch_batch_logdet_dot(st, dLb, BP, bs, M, nbatch, dinfo_b, h + off_res));
    // r^T Lambda^-1 r as the Gram left it: G_b[M][M] into sums[4 b + 2]
    GPT_TRY(launch_copy2d(st, nbatch, 1, dG + M * MG + M, gs, dsums + 2, 4));
    GPT_HIP_CHECK(hipMemcpyAsync(h + off_sums, dsums, (4 * nb + (3 * nb + 1) / 2) * sizeof(double), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    const int32_t *hw = reinterpret_cast<const int32_t *>(h + off_words);
    for (int b = 0; b < nbatch; b++) {
        const double *res = h + off_res + 4 * (size_t)b, *sums = h + off_sums + 4 * (size_t)b;
        const SparseOutcome o = sparse_outcome(method, N, M, sums, res[0], res[1], hw[b], hw[2 * nb + b], (int32_t)res[2]);
        ll_out[b] = o.ll;
        info_out[b] = o.info;
        which_out[b] = o.which;
        if (parts_out) memcpy(parts_out + 5 * (size_t)b, o.parts, sizeof(o.parts));
    }
    return GPT_OK;
}

// ---- device API: the batched kernel groups on raw device pointers, on the context's stream (tests/test_gpu_sparse_batch.py checks each alone)
extern "C" int gpt_dev_sparse_lambda_batch(gpt_ctx *c, int64_t nbatch, double *dV, int64_t ldv, int64_t vstride, int64_t rows, int64_t M, int method,
                                           const double *d_kdiag, int64_t kstride, const double *d_r, int64_t rstride, const double *d_err,
                                           const double *d_noise_var, double *d_rowval, int64_t ldr, int64_t rvstride, int32_t *d_bad)
{
    CTX_ENTER(c);
    if (!dV || !d_kdiag || !d_r || !d_err || !d_noise_var || !d_rowval || !d_bad || nbatch < 1 || rows <= 0 || M < 1 ||
        method < GPT_SPARSE_FITC || method > GPT_SPARSE_DTC || kstride < 0 || rstride < 0) {
        gpt_set_error("gpt_dev_sparse_lambda_batch: bad arguments (nbatch=%lld, rows=%lld, M=%lld, method %d)", (long long)nbatch, (long long)rows,
                      (long long)M, method);
        return GPT_E_ARG;
    }
    return launch_sparse_lambda_batch(c->stream, nbatch, dV, ldv, vstride, rows, M, method, d_kdiag, kstride, d_r, rstride, d_err, d_noise_var,
                                      d_rowval, ldr, rvstride, d_bad);
}

extern "C" int gpt_dev_sparse_rowsum_batch(gpt_ctx *c, int64_t nbatch, const double *d_rowval, int64_t ldr, int64_t rvstride, int64_t rows,
                                           double *d_acc, int64_t astride)
{
    CTX_ENTER(c);
    if (!d_rowval || !d_acc || nbatch < 1 || nbatch > 65535 || rows <= 0) {
        gpt_set_error("gpt_dev_sparse_rowsum_batch: bad arguments (nbatch=%lld, rows=%lld)", (long long)nbatch, (long long)rows);
        return GPT_E_ARG;
    }
    return launch_sparse_rowsum_batch(c->stream, nbatch, d_rowval, ldr, rvstride, rows, d_acc, astride);
}

// (nslices = 0: the fit's own choice for one element; the partial tiles go to the batch's workspace slot)
extern "C" int gpt_dev_sparse_gram_batch(gpt_ctx *c, int64_t nbatch, const double *dV, int64_t ldv, int64_t vstride, int64_t rows, int64_t mg,
                                         int nslices, double *dG, int64_t ldg, int64_t gstride)
{
    CTX_ENTER(c);
    if (!dV || !dG || nbatch < 1 || nbatch > 65535 || rows <= 0 || mg <= 0 || mg % 64) {
        gpt_set_error("gpt_dev_sparse_gram_batch: bad arguments (nbatch=%lld, rows=%lld, order %lld: a positive multiple of 64)", (long long)nbatch,
                      (long long)rows, (long long)mg);
        return GPT_E_ARG;
    }
    if (nslices <= 0) GPT_TRY(sparse_slices(c, mg, rows, &nslices));
    const int64_t ps = sparse_gram_part_doubles(mg, nslices);
    double *dPart;
    GPT_TRY(ensure(c, SLOT_SPB_PART, (size_t)nbatch * ps * sizeof(double), (void **)&dPart));
    return launch_sparse_gram_batch(c->stream, nbatch, dV, ldv, vstride, rows, mg, nslices, dPart, ps, dG, ldg, gstride);
}

extern "C" int gpt_dev_sparse_assemble_b_batch(gpt_ctx *c, int64_t nbatch, const double *dG, int64_t ldg, int64_t gstride, int64_t M, double *dB,
                                               int64_t bp, int64_t bstride, double big)
{
    CTX_ENTER(c);
    if (!dG || !dB || nbatch < 1) {
        gpt_set_error("gpt_dev_sparse_assemble_b_batch: bad arguments");
        return GPT_E_ARG;
    }
    return launch_sparse_assemble_b_batch(c->stream, nbatch, dG, ldg, gstride, M, dB, bp, bstride, big);
}
