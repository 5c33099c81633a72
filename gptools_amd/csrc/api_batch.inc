// api_batch.inc -- part of api.hip (ONE translation unit: included from there, in this order; the parts share struct gpt_ctx and
// static helpers).  Batched small fits (gpt_fit_batch*), timings / GEMM profile read-out, gpt_get_L, alpha (gpt_get_alpha).
// ------------------------------------------------------------------------------------------------
// batched small fits
// ------------------------------------------------------------------------------------------------
// nbatch independent LML evaluations of the resident data set -- the reference's likelihood grids and random starts
// (ref: gaussian_process.py:1607-1692, :723-735; gp_utils.py:98-115) live at N of a few hundred to a few thousand, where ONE
// evaluation cannot fill the GPU: its chain of 128-column leaves (diagonal block 20 us on one CU, TRSM, rank-128 update) is
// pure latency and the host's launch rate bounds it (0.37 ms at N = 1024).  Here every kernel of that chain carries the
// whole batch in a grid dimension: element b works on its own matrix A + b NP^2 with its own hyperparameters, the
// diagonal-block kernel runs nbatch workgroups on nbatch CUs at once, and the launch sequence (3 launches per leaf) is paid
// once per batch.  No look-ahead, one stream, left-looking leaves: the parallelism is across the batch.  Same kernels, same tile choice and the
// same summation orders as gpt_fit, so an element's ll / log-determinant carry the very bits gpt_fit returns for it alone
// (tests/test_gpu_parity.py::test_fit_batch_*).  N <= GPT_BATCH_MAX_N; one native kernel, no transform.
#define GPT_BATCH_MAX_N 8192
static int fit_batch_impl(gpt_ctx *c, int nbatch, int nterms, const int *kernel_ids, const int *kernel_ids2, const double *params,
                          const int *nparams_t, const int *nparams1_t, const double *noise_var, const double *y, const double *err_y,
                          double diag_add, double *ll_data_out, double *logdet_half_out, int32_t *info_out);

extern "C" int gpt_fit_batch(gpt_ctx *c, int nbatch, int kernel_id, const double *params, int nparams,
                             const double *noise_var, const double *y, const double *err_y, double diag_add,
                             double *ll_data_out, double *logdet_half_out, int32_t *info_out)
{
    return fit_batch_impl(c, nbatch, 1, &kernel_id, nullptr, params, &nparams, nullptr, noise_var, y, err_y, diag_add, ll_data_out,
                          logdet_half_out, info_out);
}

// The same for a SumKernel of native kernels (ref: kernel/core.py:549-584): element b's parameters are the terms' parameters
// concatenated (ptot = sum of nparams_t doubles per element); one accumulating builder pass per term for the whole batch, as
// gpt_fit_sum does for one matrix -- same kernels, same order: bit-identical to gpt_fit_sum per element.
extern "C" int gpt_fit_batch_sum(gpt_ctx *c, int nbatch, int nterms, const int *kernel_ids, const double *params,
                                 const int *nparams_t, const double *noise_var, const double *y, const double *err_y,
                                 double diag_add, double *ll_data_out, double *logdet_half_out, int32_t *info_out)
{
    return fit_batch_impl(c, nbatch, nterms, kernel_ids, nullptr, params, nparams_t, nullptr, noise_var, y, err_y, diag_add, ll_data_out,
                          logdet_half_out, info_out);
}

// ... and for every model gpt_fit_terms takes (VERDICT r3 #7; the reference's likelihood grid works for any model, ref
// gaussian_process.py:1607-1692, gp_utils.py:98-115): PRODUCT terms (kernel_ids2[t] >= 0: term t is kernel_ids[t] *
// kernel_ids2[t], the first nparams1[t] of its nparams[t] parameters the first factor's) and, when gpt_set_T has set one, the
// linear TRANSFORM -- every element's full K over the latent points, then T K T^T as two batched fp64-MFMA GEMMs with the shared,
// resident T (batch stride 0), the diagonal loading and the factorisation as above over the Ny observations.  Same kernels and
// summation orders as gpt_fit_terms: bit-identical per element.
extern "C" int gpt_fit_batch_terms(gpt_ctx *c, int nbatch, int nterms, const int *kernel_ids, const int *kernel_ids2,
                                   const double *params, const int *nparams_t, const int *nparams1_t, const double *noise_var,
                                   const double *y, const double *err_y, double diag_add, double *ll_data_out,
                                   double *logdet_half_out, int32_t *info_out)
{
    return fit_batch_impl(c, nbatch, nterms, kernel_ids, kernel_ids2, params, nparams_t, nparams1_t, noise_var, y, err_y, diag_add,
                          ll_data_out, logdet_half_out, info_out);
}

// The factorisation of nbatch matrices of order NP (a multiple of 128), element b at dA + b bs with the leaves' packed workspaces at dws +
// b bws and its info word at dinfo[b] (zero on entry): the leaf loop of gpt_fit_batch*, shared with gpt_sparse_fit_batch
// (api_sparse_batch.inc), which factors its K_uu + jitter I and its B through it.
static int batch_leaf_loop(hipStream_t st, int64_t NP, double *dA, int64_t bs, double *dws, int64_t bws, int32_t *dinfo, int nbatch)
{
    // LEFT-looking over the 128-column leaves: leaf j first receives the update of ALL leaves before it in one launch
    // (k = 128 j; element by element the same sums in the same order as the right-looking rank-128 updates of gpt_fit, whose
    // accumulators also start from C and walk k upwards: bit-identical), then its diagonal block and TRSM.  A right-looking
    // batch re-reads and re-writes every element of every trailing matrix once per leaf (16 bytes per 256 flops at k = 128):
    // 0.77 of the 1.31 ms of a 64 x N = 1024 batch were those updates; here every element of the factor is written once.
    // (GPT_BATCH_RIGHT=1: the right-looking form, for comparison)
    // Measured, 64 elements: N = 1024 1.376 against 1.412 ms, N = 2048 5.79 against 6.22 ms, N = 256 0.247 against 0.237 ms.
    // Larger N (round 3, bit-identical throughout): N = 3000 x 32 elements 7.8 ms (4100 evaluations/s against 1109 one by one and
    // 1848 with two contexts in two threads), N = 4096 x 32 18.2 ms (1755 / 774 / 1168), N = 8192 x 8 34.3 ms (233 / 224 / 248: a
    // single evaluation fills the chip there -- GaussianProcess.ll_batch takes this path up to N = 4096).
    static const bool force_right = getenv("GPT_BATCH_RIGHT") != nullptr;
    const bool right_looking = force_right || NP <= 512;
    for (int64_t lc = 0; lc < NP; lc += 128) {
        if (!right_looking && lc > 0)
            GPT_TRY(launch_gemm_nt(st, NP - lc, 128, lc, -1.0, dA + lc * NP, NP, dA + lc * NP, NP, 1.0, dA + lc * NP + lc, NP, 1, 0, 0,
                                   nullptr, nullptr, 0, EdgeSig(), EdgeSig(), 0, nbatch, bs));
        GPT_TRY(launch_potf2_diag(st, dA + lc * NP + lc, NP, dws + (lc / 128) * GPT_WS_BLOCK, dinfo, lc, EdgeSig(), nbatch, bs, bws));
        const int64_t r1 = lc + 128, m = NP - r1;
        if (m <= 0) break;
        GPT_TRY(launch_trsm_panel(st, m, dA + lc * NP + lc, NP, dws + (lc / 128) * GPT_WS_BLOCK, dA + r1 * NP + lc, NP, nullptr,
                                  EdgeSig(), nbatch, bs, bws));
        if (right_looking)
            GPT_TRY(launch_gemm_nt(st, m, m, 128, -1.0, dA + r1 * NP + lc, NP, dA + r1 * NP + lc, NP, 1.0, dA + r1 * NP + r1, NP, 1, 0, 0,
                                   nullptr, nullptr, 0, EdgeSig(), EdgeSig(), 0, nbatch, bs));
    }
    return GPT_OK;
}

static int fit_batch_impl(gpt_ctx *c, int nbatch, int nterms, const int *kernel_ids, const int *kernel_ids2, const double *params,
                          const int *nparams_t, const int *nparams1_t, const double *noise_var, const double *y, const double *err_y,
                          double diag_add, double *ll_data_out, double *logdet_half_out, int32_t *info_out)
{
    CTX_ENTER(c);
    // warps: a batch's elements have their own (gpt_set_warp_batch, consumed here); the context's single layers are not a batch's
    const int wb = c->warpb_nbatch;
    c->warpb_nbatch = 0;
    if (wb == 0) GPT_TRY(refuse_warp(c, "gpt_fit_batch without gpt_set_warp_batch"));
    if (wb != 0 && wb != nbatch) {
        gpt_set_error("gpt_fit_batch: %d elements, but gpt_set_warp_batch set the warps of %d", nbatch, wb);
        return GPT_E_ARG;
    }
    if (!c->dX) {
        gpt_set_error("gpt_fit_batch: call gpt_set_data first");
        return GPT_E_STATE;
    }
    if (nbatch < 1 || nbatch > 65535 || !noise_var || !y || !err_y || !ll_data_out || !info_out) return GPT_E_ARG;
    const int64_t Nx = c->Nx, N = c->dT ? c->Ny : Nx;                   // latent points / order of K_tot
    if (Nx > GPT_BATCH_MAX_N || N > GPT_BATCH_MAX_N) {
        gpt_set_error("gpt_fit_batch: needs N <= %d (N = %lld)", GPT_BATCH_MAX_N, (long long)(Nx > N ? Nx : N));
        return GPT_E_ARG;
    }
    // every element has the first one's kernels: its parse decides the layout (and refuses what any element's would)
    ModelKernel m0, mb;
    GPT_TRY(parse_model(c->D, c->n_maxsum, c->n_colmax, nterms, kernel_ids, kernel_ids2, params, nparams_t, nparams1_t, &m0));
    const bool any_prod = m0.any_prod;
    const int64_t NP = round_up(N + 1, 128), nleaf = NP / 128, bs = NP * NP, bws = nleaf * GPT_WS_BLOCK;
    // pinned staging: [y: nbatch N | err: N | noise: nbatch | KParams: nterms x nbatch (| second factors: the same) | results: 4
    // nbatch]; err .. KParams go to the device in one copy
    static_assert(sizeof(KParams) % 8 == 0, "KParams is copied as an array of doubles");
    const size_t kp_doubles = sizeof(KParams) / 8;
    const size_t nkp = (size_t)nterms * nbatch * kp_doubles * (any_prod ? 2 : 1);
    const size_t off_err = (size_t)nbatch * N, off_nv = off_err + (size_t)N, off_kp = off_nv + (size_t)nbatch, off_res = off_kp + nkp;
    const size_t need = (off_res + 4 * (size_t)nbatch) * sizeof(double);
    if (c->h_batch_cap < need) {
        if (c->h_batch) GPT_HIP_CHECK(hipHostFree(c->h_batch));
        c->h_batch = nullptr;
        c->h_batch_cap = 0;
        GPT_HIP_CHECK(hipHostMalloc((void **)&c->h_batch, need + need / 4, hipHostMallocDefault));
        c->h_batch_cap = need + need / 4;
    }
    double *h = c->h_batch;
    memcpy(h, y, (size_t)nbatch * N * sizeof(double));
    memcpy(h + off_err, err_y, (size_t)N * sizeof(double));
    memcpy(h + off_nv, noise_var, (size_t)nbatch * sizeof(double));
    char *hkp = reinterpret_cast<char *>(h + off_kp), *hkp2 = hkp + (size_t)nterms * nbatch * kp_doubles * 8;
    for (int b = 0; b < nbatch; b++) {
        if (b > 0) GPT_TRY(parse_model(c->D, c->n_maxsum, c->n_colmax, nterms, kernel_ids, kernel_ids2, params + (size_t)b * m0.nparams, nparams_t, nparams1_t, &mb));
        const ModelKernel &m = b > 0 ? mb : m0;
        for (int t = 0; t < nterms; t++) {                                  // term-major on the device: [t][b]
            memcpy(hkp + ((size_t)t * nbatch + (size_t)b) * kp_doubles * 8, &m.f1[t], sizeof(KParams));
            if (any_prod) memcpy(hkp2 + ((size_t)t * nbatch + (size_t)b) * kp_doubles * 8, &m.f2[t], sizeof(KParams));
        }
    }
    c->batch_gen++;                          // (the resident batch is overwritten: valid again once this call has succeeded)
    // device scratch: the nbatch matrices to factor (+ with a transform every element's K over the latent points and T K)
    const int64_t NxP = c->dT ? c->NxP : 0, NyP = c->dT ? round_up(N, 64) : 0;
    const size_t kfull = (size_t)NxP * NxP, tk = (size_t)NyP * NxP;
    double *dA, *dws, *dmisc;
    GPT_TRY(ensure(c, SLOT_BATCH_A, ((size_t)nbatch * bs + (size_t)nbatch * (kfull + tk)) * sizeof(double), (void **)&dA));
    double *dKf = dA + (size_t)nbatch * bs, *dTK = dKf + (size_t)nbatch * kfull;
    GPT_TRY(ensure(c, SLOT_BATCH_WS, (size_t)nbatch * bws * sizeof(double), (void **)&dws));
    // device side of the small inputs: [err: N | noise: nbatch | KParams (| second factors) | info: nbatch | zeros: Nx]
    const size_t d_off_nv = (size_t)N, d_off_kp = d_off_nv + (size_t)nbatch, d_off_info = d_off_kp + nkp,
                 d_off_zero = d_off_info + (size_t)nbatch;
    GPT_TRY(ensure(c, SLOT_BATCH_MISC, (d_off_zero + (size_t)(c->dT ? Nx : 0)) * sizeof(double), (void **)&dmisc));
    int32_t *dinfo = reinterpret_cast<int32_t *>(dmisc + d_off_info);
    const KParams *dkp = reinterpret_cast<const KParams *>(dmisc + d_off_kp);
    const KParams *dkp2 = any_prod ? dkp + (size_t)nterms * nbatch : nullptr;
    // a warped batch: element b's points at bX + b * xstr, its slope factors at bS + b * sstr; else the shared resident points
    const double *bX = c->dX, *bS = nullptr;
    int64_t xstr = 0, sstr = 0;
    if (wb) {
        bX = (const double *)c->slots[SLOT_WB_X].p;
        bS = (const double *)c->slots[SLOT_WB_S].p;
        xstr = Nx * c->D;
        sstr = Nx;
    }
    EvalScope scope(c, true);                // (in flight like an evaluation for the flag-edge accounting; has no flag edges)
    // everything on the panel stream: unmasked (all 256 CUs), the main stream is idle here
    hipStream_t st = c->panel_stream;
    GPT_TRY(stream_follows(c, c->stream, st, 0));
    GPT_HIP_CHECK(hipMemcpyAsync(dmisc, h + off_err, ((size_t)N + (size_t)nbatch + nkp) * sizeof(double), hipMemcpyHostToDevice, st));
    auto term_kp2 = [&](int t) -> const KParams * { return m0.second(t) ? dkp2 + (size_t)t * nbatch : nullptr; };
    if (c->dT) {
        // K_tot = T (K + noise_var I) T^T + diag(err_y^2) + diag_add I per element (ref :1443-1451), as fit_terms_once does for one
        double *dzero = dmisc + d_off_zero;
        GPT_HIP_CHECK(hipMemsetAsync(dzero, 0, (size_t)Nx * sizeof(double), st));
        if (NxP > Nx) GPT_HIP_CHECK(hipMemsetAsync(dKf, 0, (size_t)nbatch * kfull * sizeof(double), st));
        for (int t = 0; t < nterms; t++)
            GPT_TRY(launch_kbuild_batch(st, m0.f1[t].kernel_id, c->D, dkp + (size_t)t * nbatch, dmisc + d_off_nv, nbatch, bX, c->dn, Nx,
                                        t + 1 == nterms ? dzero : nullptr, 0.0, dKf, NxP, (int64_t)kfull, t > 0 ? 1 : 0, 1, term_kp2(t),
                                        xstr, bS, sstr, m0.gibbs_form()));
        GPT_TRY(launch_gemm_nt(st, NyP, NxP, NxP, 1.0, c->dT, NxP, dKf, NxP, 0.0, dTK, NxP, 0, 0, 0, nullptr, nullptr, 0, EdgeSig(),
                               EdgeSig(), 0, nbatch, 0, EdgeSig(), (int64_t)kfull, (int64_t)tk));
        GPT_TRY(launch_gemm_nt(st, NyP, NyP, NxP, 1.0, dTK, NxP, c->dT, NxP, 0.0, dA, NP, 1, 0, 0, nullptr, nullptr, 0, EdgeSig(),
                               EdgeSig(), 0, nbatch, (int64_t)tk, EdgeSig(), 0, bs));
        GPT_TRY(launch_add_diag(st, dA, NP, N, dmisc, diag_add, nbatch, bs));
        GPT_TRY(launch_batch_pad(st, h, nbatch, dA, NP, bs, N, NP, 1e300, dinfo));
    } else {
        GPT_TRY(launch_batch_pad(st, h, nbatch, dA, NP, bs, N, NP, 1e300, dinfo));
        for (int t = 0; t < nterms; t++)                                    // (as kbuild_terms: later terms accumulate, the last
            GPT_TRY(launch_kbuild_batch(st, m0.f1[t].kernel_id, c->D, dkp + (size_t)t * nbatch, dmisc + d_off_nv, nbatch,   //  one carries the
                                        bX, c->dn, N, t + 1 == nterms ? dmisc : nullptr, diag_add, dA, NP, bs,     //  diagonal epilogue)
                                        t > 0 ? 1 : 0, 0, term_kp2(t), xstr, bS, sstr, m0.gibbs_form()));
    }
    GPT_TRY(batch_leaf_loop(st, NP, dA, bs, dws, bws, dinfo, nbatch));
    GPT_TRY(launch_batch_logdet_dot(st, dA, NP, bs, N, nbatch, dinfo, h + off_res));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    for (int b = 0; b < nbatch; b++) {
        const double logdet_half = h[off_res + 4 * b], zz = h[off_res + 4 * b + 1];
        int32_t info = (int32_t)h[off_res + 4 * b + 2];
        if (info > N) info = (int32_t)N;                       // only the augmented pivot failed (non-finite data)
        const double ll = -0.5 * zz - logdet_half - 0.5 * (double)N * log(2.0 * M_PI);
        if (info == 0 && !(ll == ll)) info = (int32_t)N;
        info_out[b] = info;
        ll_data_out[b] = ll;
        if (logdet_half_out) logdet_half_out[b] = logdet_half;
    }
    // the batch is resident now (gpt_predict_batch): its KParams and noise variances as the device got them
    const KParams *hk = reinterpret_cast<const KParams *>(hkp);
    c->rb_kp.assign(hk, hk + (size_t)nterms * nbatch);
    if (any_prod) c->rb_kp2.assign(hk + (size_t)nterms * nbatch, hk + 2 * (size_t)nterms * nbatch);
    else c->rb_kp2.clear();
    c->rb_nv.assign(noise_var, noise_var + nbatch);
    c->rb_nbatch = nbatch;
    c->rb_model = m0;
    c->rb_N = N;
    c->rb_gen = c->batch_gen;
    c->rb_warped = wb != 0;
    return GPT_OK;
}

// ------------------------------------------------------------------------------------------------
// the predictive half of a resident batch
// ------------------------------------------------------------------------------------------------
// Prediction at M test points from every element of the batch the last gpt_fit_batch* left resident -- the reference's
// marginalisation over a hyperparameter trace (ref: gaussian_process.py:1840-1987, :2144-2254: one update_hyperparameters + predict
// per trace row) at the sizes where one prediction cannot fill the GPU.  Per element b (as gpt_predict, the mean from z_b):
//   V_b = K*_b^T L_b^-T,  mean_b = V_b z_b,  var_b = diag K**_b - rowsumsq(V_b),  cov_b = K**_b - V_b V_b^T.
// Layout: V is MP x (nbatch NP), element b in columns [b NP, (b + 1) NP) -- so that the summed covariance
//   sum_b keep_b cov_b = (sum_b keep_b K**_b) - V V^T
// is ONE lower-triangular GEMM whose contraction runs over (b, i).  Launches, all batched over the elements:
//   the cross-covariance K*_b^T into V (builder, one launch per term); the forward substitution left-looking over the 128-column
//   leaves (GEMM against the leaves before, then the panel TRSM against the workspace the fit left; the same kernels as the fit);
//   diag K**_b (pair kernel); one fused read of V for mean and variance, which also zeroes the columns >= N of every row (the
//   augmented column and the padding of the last leaf) and the rows of skipped elements; then either the summed covariance
//   (one pass over the M x M triangle for sum_b K**_b, the GEMM, a mirror) or the per-element covariances (batched builder +
//   batched GEMM).
static int gemm_nt_few(gpt_ctx *c, hipStream_t st, int64_t m, int64_t n, int64_t k, double alpha, const double *A, int64_t lda,
                       const double *B, int64_t ldb, double beta, double *C, int64_t ldc, int tri);      // (api_solve.inc)
extern "C" int gpt_predict_batch(gpt_ctx *c, const double *Xstar, const int32_t *nstar, int64_t M, const int32_t *noise_n,
                                 const int32_t *keep, double *mean_out, double *var_out, double *cov_out, double *cov_sum_out)
{
    CTX_ENTER(c);
    GPT_TRY(refuse_warp(c, "gpt_predict_batch"));
    if (c->rb_warped && c->rb_nbatch > 0 && c->rb_gen == c->batch_gen) {
        gpt_set_error("gpt_predict_batch is not available for a batch that was fitted with warps (gpt_set_warp_batch)");
        return GPT_E_NOTIMPL;
    }
    if (c->rb_nbatch <= 0 || c->rb_gen != c->batch_gen) {
        gpt_set_error("gpt_predict_batch: no batch resident (call gpt_fit_batch* first; gpt_set_data, gpt_set_T, gpt_cov_sample and "
                      "gpt_release_batch_scratch end its residency)");
        return GPT_E_STATE;
    }
    if (c->dT) {
        gpt_set_error("gpt_predict_batch: not implemented with a linear transform (gpt_set_T)");
        return GPT_E_NOTIMPL;
    }
    if (M <= 0 || M > 65535 * 32 || !Xstar || !nstar || !keep || !mean_out) {
        gpt_set_error("gpt_predict_batch: bad arguments");
        return GPT_E_ARG;
    }
    const ModelKernel &model = c->rb_model;
    const int D = c->D, nbatch = c->rb_nbatch, nterms = model.nterms;
    const int64_t N = c->rb_N, NP = round_up(N + 1, 128), nleaf = NP / 128, bs = NP * NP, bws = nleaf * GPT_WS_BLOCK;
    const int64_t MP = round_up(M, 64), ldv = (int64_t)nbatch * NP;
    GPT_TRY(check_test_orders(model, c->n_maxsum, c->n_colmax, false, nstar, M, D));
    double noise_sum = 0.0;
    for (int b = 0; b < nbatch; b++)
        if (keep[b]) noise_sum += c->rb_nv[b];
    std::vector<int32_t> hit((size_t)M, 0);
    if (noise_n)
        for (int64_t a = 0; a < M; a++) {
            bool h = true;
            for (int d = 0; d < D; d++) h = h && nstar[a * D + d] == noise_n[d];
            hit[a] = h ? 1 : 0;
        }
    // device inputs in one slot: [KParams (| second factors) | noise variances: nbatch | keep: nbatch | hit: M | X*: M D | n*: M D],
    // then [mean | var]
    const size_t nkp = (size_t)nterms * nbatch * (model.any_prod ? 2 : 1);
    const size_t b_kp = nkp * sizeof(KParams) + (size_t)nbatch * 8, b_keep = round_up(nbatch, 2) * 4, b_hit = round_up(M, 2) * 4,
                 b_xs = (size_t)M * D * 8, b_ns = round_up(M * D, 2) * 4;
    const size_t o_keep = b_kp, o_hit = o_keep + b_keep, o_xs = o_hit + b_hit, o_ns = o_xs + b_xs, o_mv = o_ns + b_ns;
    const size_t b_mv = 2 * (size_t)nbatch * MP * 8;
    char *dmisc;
    GPT_TRY(ensure(c, SLOT_PB_MISC, o_mv + b_mv, (void **)&dmisc));
    std::vector<char> hin(o_mv);
    memcpy(hin.data(), c->rb_kp.data(), (size_t)nterms * nbatch * sizeof(KParams));
    if (model.any_prod) memcpy(hin.data() + (size_t)nterms * nbatch * sizeof(KParams), c->rb_kp2.data(), (size_t)nterms * nbatch * sizeof(KParams));
    memcpy(hin.data() + nkp * sizeof(KParams), c->rb_nv.data(), (size_t)nbatch * 8);
    memcpy(hin.data() + o_keep, keep, (size_t)nbatch * 4);
    memcpy(hin.data() + o_hit, hit.data(), (size_t)M * 4);
    memcpy(hin.data() + o_xs, Xstar, b_xs);
    memcpy(hin.data() + o_ns, nstar, (size_t)M * D * 4);
    const KParams *dkp = reinterpret_cast<const KParams *>(dmisc);
    const KParams *dkp2 = model.any_prod ? dkp + (size_t)nterms * nbatch : nullptr;
    const double *dnv = reinterpret_cast<const double *>(dmisc + nkp * sizeof(KParams));
    const int32_t *dkeep = reinterpret_cast<const int32_t *>(dmisc + o_keep), *dhit = reinterpret_cast<const int32_t *>(dmisc + o_hit);
    const double *dXs = reinterpret_cast<const double *>(dmisc + o_xs);
    const int32_t *dns = reinterpret_cast<const int32_t *>(dmisc + o_ns);
    double *dmean = reinterpret_cast<double *>(dmisc + o_mv), *dvar = dmean + (size_t)nbatch * MP;
    double *dV, *dC = nullptr;
    GPT_TRY(ensure(c, SLOT_PB_V, (size_t)MP * ldv * sizeof(double), (void **)&dV));
    const bool want_cov = cov_out != nullptr, want_sum = cov_sum_out != nullptr;
    if (want_cov || want_sum)
        GPT_TRY(ensure(c, SLOT_PB_COV, (want_cov ? (size_t)nbatch : 1) * MP * MP * sizeof(double), (void **)&dC));
    const double *dA = (const double *)c->slots[SLOT_BATCH_A].p, *dws = (const double *)c->slots[SLOT_BATCH_WS].p;
    EvalScope scope(c, true);
    hipStream_t st = c->panel_stream;                      // (unmasked, as the fit)
    GPT_TRY(stream_follows(c, c->stream, st, 0));
    GPT_HIP_CHECK(hipMemcpyAsync(dmisc, hin.data(), o_mv, hipMemcpyHostToDevice, st));
    auto term_kp2 = [&](int t) -> const KParams * { return model.second(t) ? dkp2 + (size_t)t * nbatch : nullptr; };
    // K*_b^T (M x N per element) into V, zeros elsewhere
    GPT_TRY(launch_zero2d(st, MP, ldv, dV, ldv));
    for (int t = 0; t < nterms; t++)
        GPT_TRY(launch_kbuild_batch_cross(st, model.f1[t].kernel_id, D, dkp + (size_t)t * nbatch, dnv, nbatch, dXs, dns,
                                          M, c->dX, c->dn, N, dV, ldv, NP, t > 0 ? 1 : 0, term_kp2(t), model.gibbs_form()));
    // V_b = K*_b^T L_b^-T, left-looking over the leaves: leaf j first receives the update of all leaves before it
    for (int64_t lc = 0; lc < NP; lc += 128) {
        if (lc > 0)
            GPT_TRY(launch_gemm_nt(st, MP, 128, lc, -1.0, dV, ldv, dA + lc * NP, NP, 1.0, dV + lc, ldv, 0, 0, 0, nullptr, nullptr, 0,
                                   EdgeSig(), EdgeSig(), 0, nbatch, NP, EdgeSig(), bs, NP));
        GPT_TRY(launch_trsm_panel(st, MP, nullptr, 0, dws + (lc / 128) * GPT_WS_BLOCK, dV + lc, ldv, nullptr, EdgeSig(), nbatch, NP, bws));
    }
    GPT_TRY(launch_kdiag_batch(st, D, nterms, dkp, dkp2, nbatch, dXs, dns, M, dvar, MP, model.gibbs_form()));
    GPT_TRY(launch_batch_meanvar(st, M, MP, N, NP, nbatch, dV, ldv, dA, bs, dkeep, dmean, dvar, MP));
    std::vector<double> hmv(2 * (size_t)nbatch * MP);
    GPT_HIP_CHECK(hipMemcpyAsync(hmv.data(), dmean, hmv.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    if (want_sum) {
        GPT_TRY(launch_zero2d(st, MP, MP, dC, MP));
        GPT_TRY(launch_kss_sum(st, D, nterms, dkp, dkp2, nbatch, dkeep, dXs, dns, M, MP, noise_n ? dhit : nullptr, noise_sum, dC, MP, model.gibbs_form()));
        // (k = nbatch NP against few output tiles: split along k where that pays, as the few-rows solves do)
        GPT_TRY(gemm_nt_few(c, st, MP, MP, ldv, -1.0, dV, ldv, dV, ldv, 1.0, dC, MP, 1));
        GPT_TRY(launch_mirror_rows(st, dC, MP, 0, MP, MP));
        GPT_HIP_CHECK(hipMemcpy2DAsync(cov_sum_out, (size_t)M * sizeof(double), dC, (size_t)MP * sizeof(double), (size_t)M * sizeof(double),
                                       (size_t)M, hipMemcpyDeviceToHost, st));
    }
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    if (want_cov) {
        // per element: K**_b (whole square, batched builder) - V_b V_b^T (batched GEMM)
        const int64_t cs = MP * MP;
        GPT_TRY(launch_zero2d(st, (int64_t)nbatch * MP, MP, dC, MP));
        for (int t = 0; t < nterms; t++)
            GPT_TRY(launch_kbuild_batch_cross(st, model.f1[t].kernel_id, D, dkp + (size_t)t * nbatch, dnv, nbatch, dXs,
                                              dns, M, dXs, dns, M, dC, MP, cs, t > 0 ? 1 : 0, term_kp2(t), model.gibbs_form()));
        GPT_TRY(launch_gemm_nt(st, MP, MP, NP, -1.0, dV, ldv, dV, ldv, 1.0, dC, MP, 0, 0, 0, nullptr, nullptr, 0, EdgeSig(), EdgeSig(), 0,
                               nbatch, NP, EdgeSig(), NP, cs));
        for (int b = 0; b < nbatch; b++)
            if (keep[b])
                GPT_HIP_CHECK(hipMemcpy2DAsync(cov_out + (size_t)b * M * M, (size_t)M * sizeof(double), dC + (size_t)b * cs,
                                               (size_t)MP * sizeof(double), (size_t)M * sizeof(double), (size_t)M, hipMemcpyDeviceToHost, st));
        GPT_HIP_CHECK(hipStreamSynchronize(st));
    }
    for (int b = 0; b < nbatch; b++) {
        if (!keep[b]) continue;
        const double *hm = hmv.data() + (size_t)b * MP, *hv = hm + (size_t)nbatch * MP;
        memcpy(mean_out + (size_t)b * M, hm, (size_t)M * sizeof(double));
        const double nv = c->rb_nv[b];
        if (var_out)
            for (int64_t a = 0; a < M; a++) var_out[(size_t)b * M + a] = hv[a] + (hit[a] ? nv : 0.0);
        if (cov_out && noise_n)
            for (int64_t a = 0; a < M; a++)
                if (hit[a]) cov_out[(size_t)b * M * M + (size_t)a * M + a] += nv;
    }
    return GPT_OK;
}

extern "C" int gpt_last_timings(gpt_ctx *c, double *out_ms, int n)
{
    if (!c || !out_ms) return GPT_E_ARG;
    const int cnt = n < 5 ? n : 5;
    for (int i = 0; i < cnt; i++) out_ms[i] = c->timings[i];
    return cnt;
}

// Fold the finished launches' event pairs into the running sums.  Must run after the streams have drained and before
// the next factorisation re-records the edge events that double as stop events.
static int harvest_gemm_profile(gpt_ctx *c)
{
    for (size_t i = 0; i < c->gprof_used; i++) {
        float t = 0;
        GPT_HIP_CHECK(hipEventElapsedTime(&t, c->gprof[i].e0, c->gprof[i].stop));
        c->prof_ms += t;
        c->prof_flops += c->gprof[i].flops;
        c->prof_bytes += c->gprof[i].bytes;
    }
    c->prof_count += (double)c->gprof_used;
    c->gprof_used = 0;
    return GPT_OK;
}

static int gemm_profile_read(gpt_ctx *c, double *out, int n)
{
    if (!out || n < 3) return GPT_E_ARG;
    GPT_HIP_CHECK(hipStreamSynchronize(c->stream));
    GPT_HIP_CHECK(hipStreamSynchronize(c->panel_stream));
    GPT_TRY(harvest_gemm_profile(c));
    out[0] = c->prof_flops;
    out[1] = c->prof_ms;
    out[2] = c->prof_count;
    if (n > 3) out[3] = c->prof_bytes;
    c->prof_flops = c->prof_ms = c->prof_count = c->prof_bytes = 0.0;
    return GPT_OK;
}

extern "C" int gpt_gemm_profile_read(gpt_ctx *c, double *out3)
{
    CTX_ENTER(c);
    return gemm_profile_read(c, out3, 3);
}

extern "C" int gpt_gemm_profile_read4(gpt_ctx *c, double *out4)
{
    CTX_ENTER(c);
    return gemm_profile_read(c, out4, 4);
}

#define NEED_FACTOR(c)                                                        \
    do {                                                                      \
        if (!(c)->factored) {                                                 \
            gpt_set_error("no valid factorisation resident (call gpt_fit)");  \
            return GPT_E_STATE;                                               \
        }                                                                     \
    } while (0)

extern "C" int gpt_get_L(gpt_ctx *c, double *L_out)
{
    CTX_ENTER(c);
    NEED_FACTOR(c);
    if (!L_out) return GPT_E_ARG;
    const int64_t N = c->N;
    double *dlow;
    GPT_TRY(ensure(c, SLOT_LOW, (size_t)N * N * sizeof(double), (void **)&dlow));
    GPT_TRY(launch_extract_lower(c->stream, c->dA, c->NP, N, dlow, N));
    GPT_HIP_CHECK(hipMemcpyAsync(L_out, dlow, (size_t)N * N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    GPT_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GPT_OK;
}

// alpha = L^-T z with z = the augmented row (z = L^-1 y)   (ref: gaussian_process.py:1462, the second half of cho_solve)
// In 512-wide steps against the inverse transposes of the factor's 512 x 512 diagonal blocks (solve.hip launch_trsv_lt_wide;
// the blocks' inverses are the ones predict and the gradient use, built once per factorisation -- by ONE launch since round 5,
// trinv512_kernel): 2 N / 512 dependent launches instead of 2 N / 128.  N = 8192: 128-wide 1.0 ms; 512-wide with the inverses
// from 15 batched launches (rounds 2-4) 0.43 ms; now 0.34 ms, 0.24 of them the 31 launches of the substitution.  What is left of
// the order beyond the last whole 512-block falls in 128-wide steps first (last rows first).
// (Round 5 also built 1024-wide steps -- the off-diagonal quadrant of a 1024-block's inverse transpose, U12 = -(U11 L21^T) U22,
// from two batched GEMMs: 15 launches instead of 31 save 95 us, the two GEMMs are 2 x 2.1 GFLOP = 119 us.  Removed.)
// GPT_ALPHA_NARROW=1 (measurement aid): the 128-wide form throughout.  Option binv_launches = 1: the inverses by rounds 2-4's launches.
static int ensure_block_inverses(gpt_ctx *c, int64_t nb, int64_t nfull, double **out, double **out_u = nullptr, hipStream_t on = nullptr);
// on: the stream the substitution runs on (default: the context's main stream).  An eager evaluation passes the stream its
// factorisation ENDS on (the panel stream): no event edge between the factorisation and alpha's first kernel.
static int ensure_alpha(gpt_ctx *c, hipStream_t on = nullptr)
{
    if (c->alpha_valid) return GPT_OK;
    const int64_t N = c->N, NP = c->NP, n128 = round_up(N, 128);
    hipStream_t st = on ? on : c->stream;
    static const bool narrow = getenv("GPT_ALPHA_NARROW") != nullptr;
    const int64_t nwide = (n128 / 512) * 512;
    double *w = c->d_alpha + NP;
    const double *z = c->dA + N * NP;                     // the augmented row: z = L^-1 y
    if (!narrow && nwide == N && nwide >= 1024) {
        // N a multiple of 512 (C3, C2, C5, C4): every entry of alpha is written by the 512-wide steps and the first step reads z
        // where the factorisation left it -- nothing in front of the substitution but the inverse of the block(s) that were not
        // built under the last panel
        double *W = nullptr, *U = nullptr;
        GPT_TRY(ensure_block_inverses(c, 512, nwide, &W, &U, st));
        GPT_TRY(launch_trsv_lt_wide(st, nwide, c->dA, NP, U, w, c->d_alpha, z));
        c->alpha_valid = true;
        return GPT_OK;
    }
    // alpha = 0, w = z padded with zeros (one launch: solve.hip alpha_init_kernel)
    GPT_TRY(launch_alpha_init(st, N, NP, z, w, c->d_alpha));
    if (narrow || nwide < 1024) {
        GPT_HIP_CHECK(hipMemcpyAsync(c->d_alpha, w, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, st));
        GPT_TRY(launch_trsv_lt(st, n128, c->dA, NP, c->d_invd, c->d_alpha));
        c->alpha_valid = true;
        return GPT_OK;
    }
    double *W = nullptr, *U = nullptr;
    GPT_TRY(ensure_block_inverses(c, 512, nwide, &W, &U, st));
    if (n128 > nwide) {
        GPT_TRY(launch_trsv_lt(st, n128, c->dA, NP, c->d_invd, w, nwide / 128));
        GPT_HIP_CHECK(hipMemcpyAsync(c->d_alpha + nwide, w + nwide, (size_t)(n128 - nwide) * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    GPT_TRY(launch_trsv_lt_wide(st, nwide, c->dA, NP, U, w, c->d_alpha));
    c->alpha_valid = true;
    return GPT_OK;
}

// alpha to the pinned landing buffer, behind whatever computes it (valid for the host after that stream's next sync)
static int alpha_to_host(gpt_ctx *c, hipStream_t on)
{
    hipStream_t st = on ? on : c->stream;
    GPT_TRY(ensure_alpha(c, st));
    if (c->h_alpha_valid) return GPT_OK;
    GPT_HIP_CHECK(hipMemcpyAsync(c->h_alpha, c->d_alpha, (size_t)c->N * sizeof(double), hipMemcpyDeviceToHost, st));
    c->h_alpha_valid = true;
    return GPT_OK;
}

extern "C" int gpt_get_alpha(gpt_ctx *c, double *alpha_out)
{
    CTX_ENTER(c);
    NEED_FACTOR(c);
    if (!alpha_out) return GPT_E_ARG;
    const bool landed = c->alpha_valid && c->h_alpha_valid;      // (an eager evaluation: the fit's own sync covered the copy)
    if (!landed) {
        GPT_TRY(alpha_to_host(c));
        GPT_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    memcpy(alpha_out, c->h_alpha, (size_t)c->N * sizeof(double));
    return GPT_OK;
}
