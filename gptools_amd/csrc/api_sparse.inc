// api_sparse.inc -- part of api.hip (ONE translation unit: included from there, in this order; the parts share struct gpt_ctx and
// static helpers).  Inducing-point approximations (FITC / VFE / DTC; DESIGN.md section 18): gpt_sparse_set_inducing, gpt_sparse_fit,
// gpt_sparse_predict, gpt_sparse_get_c, gpt_dev_sparse_gram / _gram2 / _lambda / _rowsum / _var / _assemble_b.
// ------------------------------------------------------------------------------------------------
// Layout.  M inducing points.  MPU = M rounded up to 128 is the order of the factored K_uu + jitter I (unit diagonal on the padding
// rows, so the padding columns of V^T = K_fu L_u^-T stay zero).  BP = (M + 1) rounded up to 128 is the order of the AUGMENTED B: rows
// < M hold I + G, row M holds b^T = (V Lambda^-1 r)^T with 1e300 on its diagonal -- after the factorisation it holds c^T = (L_B^-1 b)^T,
// as the dense fit's augmented row holds z^T (DESIGN section 3) -- and the rows behind it a unit diagonal.  A chunk of rows is a
// (rows rounded up to 64) x LDV row-major block, LDV = BP >= MPU: wide enough for both right-side solves and for the r~ column at M.
// The Gram G has order MG = (M + 1) rounded up to 64.
// ------------------------------------------------------------------------------------------------
#define GPT_SPARSE_CHUNK_BYTES (512ll << 20)      // what the two chunk x LDV buffers of a fit / a prediction may take together

struct SparseDims {
    int64_t M, MPU, BP, LDV, MG;
};

static SparseDims sparse_dims(int64_t M)
{
    SparseDims d;
    d.M = M;
    d.MPU = round_up(M, 128);
    d.BP = round_up(M + 1, 128);
    d.LDV = d.BP;
    d.MG = round_up(M + 1, 64);
    return d;
}

// rows per chunk: the caller's (a positive multiple of 64), or what keeps nbuf chunk x LDV buffers within GPT_SPARSE_CHUNK_BYTES (two for a
// fit or a prediction, four for the gradient: api_sparse_grad.inc)
static int sparse_chunk(const SparseDims &d, int64_t chunk_rows, int64_t n, int64_t *out, int64_t nbuf = 2)
{
    if (chunk_rows < 0 || chunk_rows % 64) {
        gpt_set_error("gpt_sparse: chunk_rows must be 0 (chosen by size) or a positive multiple of 64, got %lld", (long long)chunk_rows);
        return GPT_E_ARG;
    }
    int64_t ch = chunk_rows;
    if (ch == 0) {
        ch = GPT_SPARSE_CHUNK_BYTES / (nbuf * d.LDV * (int64_t)sizeof(double)) / 64 * 64;
        if (ch < 64) ch = 64;
    }
    if (ch > round_up(n, 64)) ch = round_up(n, 64);
    *out = ch;
    return GPT_OK;
}

// slices per 64 x 64 tile of the Gram: (lower tiles) x slices is about SIX times the number of compute units.  Measured (DESIGN 18.6,
// M = 1024, a 29120-row chunk, 153 tiles): 3 slices (twice the CUs) 1.19 ms, 5: 0.97, 10: 0.88, 13: 0.93; M = 256 (15 tiles): 34 slices
// 0.274 ms, 102: 0.257 -- the kernel reads its operands straight from global memory and wants the four workgroups a CU holds.
static int sparse_slices(gpt_ctx *c, int64_t mg, int64_t rows, int *out)
{
    if (c->sp_ncu <= 0) GPT_HIP_CHECK(hipDeviceGetAttribute(&c->sp_ncu, hipDeviceAttributeMultiprocessorCount, c->device));
    const int64_t ntiles = sparse_gram_tiles(mg);
    int64_t s = (6 * (int64_t)c->sp_ncu + ntiles / 2) / ntiles;
    if (s > (rows + 3) / 4) s = (rows + 3) / 4;
    if (s < 1) s = 1;
    if (s > 1024) s = 1024;
    *out = (int)s;
    return GPT_OK;
}

static int sparse_refusals(const gpt_ctx *c, const char *who, bool need_fit)
{
    if (!c->dX) {
        gpt_set_error("%s: call gpt_set_data first", who);
        return GPT_E_STATE;
    }
    if (c->dT) {
        gpt_set_error("%s is not available with a linear transform set (gpt_set_T)", who);
        return GPT_E_NOTIMPL;
    }
    GPT_TRY(refuse_warp(c, who));
    if (c->sp_M <= 0) {
        gpt_set_error("%s: call gpt_sparse_set_inducing first", who);
        return GPT_E_STATE;
    }
    if (need_fit && !c->sp_fitted) {
        gpt_set_error("%s needs a sparse fit (gpt_sparse_fit) that succeeded", who);
        return GPT_E_STATE;
    }
    return GPT_OK;
}

static double *sparse_Z(const gpt_ctx *c) { return (double *)c->slots[SLOT_SP_Z].p; }
static int32_t *sparse_nZ(const gpt_ctx *c) { return reinterpret_cast<int32_t *>(sparse_Z(c) + c->sp_M * c->D); }

// The resident state of a sparse fit as pointers: SLOT_SP_LU holds L_u (MPU x MPU) and behind it the packed workspaces of its leaves,
// SLOT_SP_LB L_B (BP x BP), its workspaces and c (M); SLOT_SP_Z the inducing inputs and their derivative orders.  The fit writes
// through these pointers (after it has sized the slots), every other entry point only reads.
struct SparseResident {
    SparseDims d;
    double *Lu, *ws_u, *Lb, *ws_b, *c;
    const double *Z;
    const int32_t *nZ;
};

static SparseResident sparse_resident(const gpt_ctx *c)
{
    SparseResident r;
    r.d = sparse_dims(c->sp_M);
    r.Lu = (double *)c->slots[SLOT_SP_LU].p;
    r.ws_u = r.Lu + r.d.MPU * r.d.MPU;
    r.Lb = (double *)c->slots[SLOT_SP_LB].p;
    r.ws_b = r.Lb + r.d.BP * r.d.BP;
    r.c = r.ws_b + (r.d.BP / 128) * GPT_WS_BLOCK;
    r.Z = sparse_Z(c);
    r.nZ = sparse_nZ(c);
    return r;
}

// y and err_y of the N training points into SLOT_SP_Y, [y | err_y], on `st` (pageable sources: the caller synchronises before it returns)
static int sparse_upload_y(gpt_ctx *c, hipStream_t st, const double *y, const double *err_y, int64_t N, double **dY)
{
    GPT_TRY(ensure(c, SLOT_SP_Y, (size_t)2 * N * sizeof(double), (void **)dY));
    GPT_HIP_CHECK(hipMemcpyAsync(*dY, y, (size_t)N * sizeof(double), hipMemcpyHostToDevice, st));
    GPT_HIP_CHECK(hipMemcpyAsync(*dY + N, err_y, (size_t)N * sizeof(double), hipMemcpyHostToDevice, st));
    return GPT_OK;
}

// The workspace of a Gram of order mg in nslices slices: one 64 x 64 partial tile per (slice, lower tile)
static int sparse_part(gpt_ctx *c, int nslices, int64_t mg, double **dPart)
{
    return ensure(c, SLOT_SP_PART, (size_t)sparse_gram_part_doubles(mg, nslices) * sizeof(double), (void **)dPart);
}

// What gpt_sparse_fit and gpt_sparse_fit_batch refuse alike: a method out of range, a negative (or NaN) jitter or noise variance
// (noise_var: one per element)
static int sparse_fit_refusals(const char *who, int method, double jitter, const double *noise_var, int nbatch)
{
    if (method != GPT_SPARSE_FITC && method != GPT_SPARSE_VFE && method != GPT_SPARSE_DTC) {
        gpt_set_error("%s: method must be GPT_SPARSE_FITC, GPT_SPARSE_VFE or GPT_SPARSE_DTC, got %d", who, method);
        return GPT_E_ARG;
    }
    bool nv_ok = true;
    for (int b = 0; b < nbatch; b++) nv_ok = nv_ok && noise_var[b] >= 0.0;
    if (!(jitter >= 0.0) || !nv_ok) {
        gpt_set_error("%s: jitter and every noise_var must be non-negative", who);
        return GPT_E_ARG;
    }
    return GPT_OK;
}

// The leading minor a failed factorisation of order > M reports, as the fits return it: at most M (a word > M: only the augmented /
// padding pivots failed)
static int32_t sparse_clamp_info(int32_t info, int64_t M) { return info > M ? (int32_t)M : info; }

// What one fit's numbers say, for the single fit and for every element of a batch: which step failed first, in the order the fit meets
// them -- 1 K_uu + jitter I (info_u), 2 a Lambda_i was not positive and finite (bad), 3 B (info_b), 0 none -- with `info` the leading
// minor of 1 and 3 (sparse_clamp_info); and the objective with its five parts, formed whatever failed.  sums: sum log Lambda, the VFE
// trace term, r^T Lambda^-1 r.  The ONE statement of the expression: the batch's bit rule (DESIGN.md 18.11) rests on it.
struct SparseOutcome {
    double ll, parts[5];
    int32_t which, info;
};
static SparseOutcome sparse_outcome(int method, int64_t N, int64_t M, const double *sums, double logdet_lb, double cc, int32_t info_u, int32_t bad,
                                    int32_t info_b)
{
    SparseOutcome o;
    o.which = info_u != 0 ? 1 : bad != 0 ? 2 : info_b != 0 ? 3 : 0;
    o.info = sparse_clamp_info(o.which == 1 ? info_u : o.which == 3 ? info_b : 0, M);
    const double sum_log_lambda = sums[0], trace = sums[1], rlr = sums[2];
    o.ll = -0.5 * ((((sum_log_lambda + 2.0 * logdet_lb) + rlr) - cc) + (double)N * log(2.0 * M_PI));
    if (method == GPT_SPARSE_VFE) o.ll -= 0.5 * trace;
    o.parts[0] = sum_log_lambda;
    o.parts[1] = logdet_lb;
    o.parts[2] = rlr;
    o.parts[3] = cc;
    o.parts[4] = trace;
    return o;
}

extern "C" int gpt_sparse_set_inducing(gpt_ctx *c, const double *Z, const int32_t *nZ, int64_t M)
{
    CTX_ENTER(c);
    c->sp_fitted = false;
    c->sp_chunk_rows = 0;
    c->sp_M = 0;
    if (!c->dX) {
        gpt_set_error("gpt_sparse_set_inducing: call gpt_set_data first");
        return GPT_E_STATE;
    }
    if (!Z || M < 1 || M > 65000) {
        gpt_set_error("gpt_sparse_set_inducing: bad arguments (M=%lld)", (long long)M);
        return GPT_E_ARG;
    }
    const int D = c->D;
    std::vector<int32_t> zero;
    if (!nZ) {
        zero.assign((size_t)M * D, 0);
        nZ = zero.data();
    }
    c->sp_zmaxsum = 0;
    for (int d = 0; d < GPT_MAX_DIM; d++) c->sp_zcolmax[d] = 0;
    for (int64_t i = 0; i < M; i++) {
        long sn = 0;
        for (int d = 0; d < D; d++) {
            if (nZ[i * D + d] < 0) {
                gpt_set_error("gpt_sparse_set_inducing: negative derivative order");
                return GPT_E_ARG;
            }
            sn += nZ[i * D + d];
            if (nZ[i * D + d] > c->sp_zcolmax[d]) c->sp_zcolmax[d] = nZ[i * D + d];
        }
        if (sn > c->sp_zmaxsum) c->sp_zmaxsum = sn;
    }
    double *dZ;
    GPT_HIP_CHECK(hipStreamSynchronize(c->stream));
    GPT_TRY(ensure(c, SLOT_SP_Z, (size_t)M * D * (sizeof(double) + sizeof(int32_t)), (void **)&dZ));
    GPT_HIP_CHECK(hipMemcpyAsync(dZ, Z, (size_t)M * D * sizeof(double), hipMemcpyHostToDevice, c->stream));
    GPT_HIP_CHECK(hipMemcpyAsync(dZ + M * D, nZ, (size_t)M * D * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    GPT_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->sp_M = M;
    return GPT_OK;
}

// The order rules of a sparse model: every pair the builders meet is (x, z), (z, z), (x, x) on the diagonal or, in a prediction,
// (x*, z) / (x*, x*) -- so the model is parsed against the larger of the training and the inducing orders, and a Matern52 factor
// checks the inducing rows as it checks test rows.
static void sparse_order_bounds(const gpt_ctx *c, long *maxsum, long *colmax)
{
    *maxsum = c->n_maxsum > c->sp_zmaxsum ? c->n_maxsum : c->sp_zmaxsum;
    for (int d = 0; d < GPT_MAX_DIM; d++) colmax[d] = c->n_colmax[d] > c->sp_zcolmax[d] ? c->n_colmax[d] : c->sp_zcolmax[d];
}

// k(x_i, x_i) of `rows` points into dkd (the pair-diagonal pass of gpt_predict)
static int sparse_kdiag(hipStream_t st, const ModelKernel &model, const double *dXp, const int32_t *dnp, int64_t rows, double *dkd)
{
    for (int t = 0; t < model.nterms; t++) {
        KParams ks = model.f1[t];
        ks.symmetric = 1;
        ks.hyper_deriv = -1;
        GPT_TRY(launch_kpairs(st, ks, dXp, dXp, dnp, dnp, rows, dkd, t > 0 ? 1 : 0, model.second(t)));
    }
    return GPT_OK;
}

// The front end of one chunk of `rows` points (dXc, dnc), as the fit, the prediction and the gradient run it: V^T = K_fu L_u^-T into dV
// (rows rounded up to 64, x LDV) and, with dW given, W^T = V^T L_B^-T into dW.  L_B is the augmented factor: column M of W comes out
// as -(w.c) / 1e150 and the columns behind it stay zero; only the columns < M are read.  Enqueues on `st` and nothing else: no
// synchronisation, no allocation.  mark(0) after the build, mark(1) after the solve by L_u: the fit's phase marks.
template <class Mark>
static int sparse_chunk_vw(gpt_ctx *c, hipStream_t st, const ModelKernel &model, const SparseResident &r, const double *dXc, const int32_t *dnc,
                           int64_t rows, double *dV, double *dW, Mark &&mark)
{
    const int64_t CP = round_up(rows, 64), LDV = r.d.LDV;
    GPT_TRY(launch_zero2d(st, CP, LDV, dV, LDV));
    GPT_TRY(kbuild_terms(st, model, 0, dXc, dnc, rows, r.Z, r.nZ, r.d.M, 0, 0, 0, nullptr, 0.0, 0.0, dV, LDV));
    GPT_TRY(mark(0));
    GPT_TRY(trsm_rlt(c, st, CP, r.d.MPU, r.Lu, r.d.MPU, r.ws_u, dV, LDV));
    GPT_TRY(mark(1));
    if (!dW) return GPT_OK;
    GPT_TRY(launch_copy2d(st, CP, LDV, dV, LDV, dW, LDV));
    return trsm_rlt(c, st, CP, r.d.BP, r.Lb, r.d.BP, r.ws_b, dW, LDV);
}

static int sparse_chunk_vw(gpt_ctx *c, hipStream_t st, const ModelKernel &model, const SparseResident &r, const double *dXc, const int32_t *dnc,
                           int64_t rows, double *dV, double *dW)
{
    return sparse_chunk_vw(c, st, model, r, dXc, dnc, rows, dV, dW, [](int) { return GPT_OK; });
}

extern "C" int gpt_sparse_fit(gpt_ctx *c, int method, int nterms, const int *kernel_ids, const int *kernel_ids2, const double *params,
                              const int *nparams, const int *nparams1, double noise_var, const double *y, const double *err_y,
                              double jitter, int64_t chunk_rows, double *ll_out, double *parts_out)
{
    CTX_ENTER(c);
    GPT_TRY(sparse_refusals(c, "gpt_sparse_fit", false));
    if (!y || !err_y || !kernel_ids2 || !nparams1 || !ll_out) return GPT_E_ARG;
    GPT_TRY(sparse_fit_refusals("gpt_sparse_fit", method, jitter, &noise_var, 1));
    c->sp_fitted = false;
    c->sp_chunk_rows = 0;
    const int D = c->D;
    const int64_t N = c->Nx;
    long maxsum, colmax[GPT_MAX_DIM];
    sparse_order_bounds(c, &maxsum, colmax);
    ModelKernel model;
    GPT_TRY(parse_model(D, maxsum, colmax, nterms, kernel_ids, kernel_ids2, params, nparams, nparams1, &model));
    const SparseDims sd = sparse_dims(c->sp_M);
    const int64_t M = sd.M, MPU = sd.MPU, BP = sd.BP, LDV = sd.LDV, MG = sd.MG;
    int64_t chunk;
    GPT_TRY(sparse_chunk(sd, chunk_rows, N, &chunk));
    if (model.has_m52) {
        std::vector<int32_t> hz((size_t)M * D);
        GPT_HIP_CHECK(hipMemcpy(hz.data(), sparse_nZ(c), hz.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        GPT_TRY(check_m52_orders(hz.data(), M, D));
    }
    int nslices;
    GPT_TRY(sparse_slices(c, MG, chunk < N ? chunk : N, &nslices));
    hipStream_t st = c->stream;
    double *dLu, *dLb, *dV, *dG, *dPart, *dMisc, *dY;
    GPT_TRY(ensure(c, SLOT_SP_LU, ((size_t)MPU * MPU + (size_t)(MPU / 128) * GPT_WS_BLOCK) * sizeof(double), (void **)&dLu));
    GPT_TRY(ensure(c, SLOT_SP_LB, ((size_t)BP * BP + (size_t)(BP / 128) * GPT_WS_BLOCK + BP) * sizeof(double), (void **)&dLb));
    GPT_TRY(ensure(c, SLOT_SP_V, (size_t)chunk * LDV * sizeof(double), (void **)&dV));
    GPT_TRY(ensure(c, SLOT_SP_G, (size_t)MG * MG * sizeof(double), (void **)&dG));
    GPT_TRY(sparse_part(c, nslices, MG, &dPart));
    // misc: [0, 8) the running sums (0: sum log Lambda, 1: the VFE trace term, 2: r^T Lambda^-1 r as the Gram left it);
    // [8, 16) three 32-bit words: info of K_uu, info of B, "a Lambda_i was not positive"; then k(x_i, x_i), the two per-row values
    // (chunk each) and MPU zeros (the err of K_uu's diagonal epilogue)
    GPT_TRY(ensure(c, SLOT_SP_MISC, (size_t)(16 + 3 * chunk + MPU) * sizeof(double), (void **)&dMisc));
    const SparseResident res = sparse_resident(c);                   // (after the slots are sized: the fit writes through it)
    int32_t *d_words = reinterpret_cast<int32_t *>(dMisc + 8);
    double *dkd = dMisc + 16, *drow = dkd + chunk, *dzero = drow + 2 * chunk;
    EvalScope scope(c, true);                                        // counted like an evaluation in flight, on event edges
    // phase timing (option "timing"): events at the phase boundaries of every chunk, summed after the fit into gpt_last_timings:
    // [0] K_fu build, [1] right-side solve, [2] the row pass (k_i, Lambda, scaling, sums), [3] the Gram, [4] the two factorisations
    size_t nev = 0;
    std::vector<int> ev_phase;
    auto mark = [&](int phase) -> int {                              // phase: what ENDS here (-1: a start mark)
        if (!c->timing) return GPT_OK;
        if (c->sp_events.size() <= nev) {
            hipEvent_t fresh = nullptr;
            GPT_HIP_CHECK(hipEventCreate(&fresh));
            c->sp_events.push_back(fresh);
        }
        hipEvent_t e = c->sp_events[nev];
        GPT_HIP_CHECK(hipEventRecord(e, st));
        ev_phase.push_back(phase);
        nev++;
        return GPT_OK;
    };
    GPT_TRY(sparse_upload_y(c, st, y, err_y, N, &dY));
    GPT_HIP_CHECK(hipMemsetAsync(dMisc, 0, (size_t)(16 + 3 * chunk + MPU) * sizeof(double), st));
    // ---- L_u = chol(k(Z, Z) + jitter I)
    GPT_TRY(mark(-1));
    GPT_TRY(launch_zero2d(st, MPU, MPU, dLu, MPU));
    GPT_TRY(kbuild_terms(st, model, 1, res.Z, res.nZ, M, res.Z, res.nZ, M, 1, 0, 0, dzero, 0.0, jitter, dLu, MPU));
    GPT_TRY(launch_fill_pad(st, dLu, MPU, M, MPU, nullptr, 0.0));      // unit diagonal on the padding rows
    GPT_TRY(potrf_run(c, MPU, dLu, MPU, res.ws_u, d_words + 0));
    GPT_TRY(mark(4));
    GPT_HIP_CHECK(hipMemcpyAsync(c->h_info, d_words + 0, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    if (*c->h_info != 0) {
        const int info = sparse_clamp_info(*c->h_info, M);
        gpt_set_error("K_uu + jitter I: %d-th leading minor of the array is not positive definite", info);
        return info;
    }
    // ---- the chunks, in ascending order
    GPT_TRY(launch_zero2d(st, MG, MG, dG, MG));
    for (int64_t r0 = 0; r0 < N; r0 += chunk) {
        const int64_t rows = (N - r0 < chunk) ? N - r0 : chunk;
        const double *dXc = c->dX + r0 * D;
        const int32_t *dnc = c->dn + r0 * D;
        GPT_TRY(mark(-1));
        GPT_TRY(sparse_chunk_vw(c, st, model, res, dXc, dnc, rows, dV, nullptr, mark));
        if (method != GPT_SPARSE_DTC) GPT_TRY(sparse_kdiag(st, model, dXc, dnc, rows, dkd));
        GPT_TRY(launch_sparse_lambda(st, dV, LDV, rows, M, method, dkd, dY + r0, dY + N + r0, noise_var, drow, chunk, d_words + 2));
        GPT_TRY(launch_sparse_rowsum(st, drow, chunk, rows, dMisc));
        GPT_TRY(mark(2));
        GPT_TRY(launch_sparse_gram(st, nullptr, dV, LDV, rows, MG, nslices, dPart, dG, MG));
        GPT_TRY(mark(3));
    }
    // ---- B = I + G, augmented; L_B, c
    GPT_TRY(mark(-1));
    GPT_TRY(launch_sparse_assemble_b(st, dG, MG, M, dLb, BP, 1e300));
    GPT_TRY(potrf_run(c, BP, dLb, BP, res.ws_b, d_words + 1));
    GPT_TRY(mark(4));
    GPT_TRY(launch_logdet_dot(st, dLb, BP, M, d_words + 1, c->d_scal, c->h_scal));
    GPT_TRY(launch_copy2d(st, 1, M, dLb + M * BP, BP, res.c, M));
    GPT_TRY(launch_copy2d(st, 1, 1, dG + M * MG + M, MG, dMisc + 2, 1));
    double sums[3];
    int32_t words[3];
    GPT_HIP_CHECK(hipMemcpyAsync(sums, dMisc, sizeof(sums), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipMemcpyAsync(words, d_words, sizeof(words), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    if (c->timing) {
        for (int i = 0; i < 5; i++) c->timings[i] = 0.0;
        for (size_t i = 1; i < nev; i++)
            if (ev_phase[i] >= 0) {
                float ms = 0;
                GPT_HIP_CHECK(hipEventElapsedTime(&ms, c->sp_events[i - 1], c->sp_events[i]));
                c->timings[ev_phase[i]] += ms;
            }
    }
    const int32_t info_b = (int32_t)c->h_scal[2];
    const SparseOutcome o = sparse_outcome(method, N, M, sums, c->h_scal[0], c->h_scal[1], 0, words[2], info_b);
    if (o.which == 2) {
        gpt_set_error("gpt_sparse_fit: a Lambda_i is not a positive finite number (k_i - q_i + noise_var + err_y_i^2 for fitc, "
                      "noise_var + err_y_i^2 for vfe / dtc)");
        return GPT_E_VALUE;
    }
    if (o.which == 3) {
        if (info_b > M) gpt_set_error("B = I + V Lambda^-1 V^T: factorisation failed in the augmented row (non-finite data?)");      // c.c overflowed
        else gpt_set_error("B = I + V Lambda^-1 V^T: %d-th leading minor of the array is not positive definite", (int)o.info);
        return (int)o.info;
    }
    *ll_out = o.ll;
    if (parts_out) memcpy(parts_out, o.parts, sizeof(o.parts));
    c->sp_model = model;
    c->sp_method = method;
    c->sp_noise_var = noise_var;
    c->sp_jitter = jitter;
    c->sp_chunk_rows = chunk_rows;
    c->sp_fitted = true;
    return GPT_OK;
}

extern "C" int gpt_sparse_get_c(gpt_ctx *c, double *c_out)
{
    CTX_ENTER(c);
    GPT_TRY(sparse_refusals(c, "gpt_sparse_get_c", true));
    if (!c_out) return GPT_E_ARG;
    const SparseResident res = sparse_resident(c);
    GPT_HIP_CHECK(hipMemcpyAsync(c_out, res.c, (size_t)res.d.M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    GPT_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GPT_OK;
}

// v = L_u^-1 k(Z, x*), w = L_B^-1 v, mean = w.c, cov = k(x*, x*') - v.v' + w.w'.  want <= 1: the test points go through in the chunks
// of the resident fit -- its chunk_rows argument (sp_chunk_rows), 0: the size rule -- so a caller who bounded the fit's memory by
// chunk_rows bounds the prediction's too (two chunk x LDV buffers, V and W, where the fit holds one); want == 2 needs every pair of
// rows, so V and W hold all Ms rows whatever chunk_rows was (the result is Ms x Ms anyway).
extern "C" int gpt_sparse_predict(gpt_ctx *c, const double *Xstar, const int32_t *nstar, int64_t Ms, int want,
                                  const double *noise_params, const int32_t *noise_n, double *mean_out, double *std_out,
                                  double *cov_out)
{
    CTX_ENTER(c);
    GPT_TRY(sparse_refusals(c, "gpt_sparse_predict", true));
    if (Ms <= 0 || !Xstar || !nstar || !mean_out || want < 0 || want > 2 || (want == 1 && !std_out) || (want == 2 && !cov_out)) {
        gpt_set_error("gpt_sparse_predict: bad arguments");
        return GPT_E_ARG;
    }
    if (want == 2 && Ms > 65535 * 32) return GPT_E_ARG;
    const int D = c->D;
    const ModelKernel &model = c->sp_model;
    long maxsum, colmax[GPT_MAX_DIM];
    sparse_order_bounds(c, &maxsum, colmax);
    GPT_TRY(check_test_orders(model, maxsum, colmax, false, nstar, Ms, D));
    const SparseResident res = sparse_resident(c);
    const int64_t M = res.d.M, MPU = res.d.MPU, LDV = res.d.LDV;
    int64_t chunk;
    GPT_TRY(sparse_chunk(res.d, c->sp_chunk_rows, Ms, &chunk));
    if (want == 2) chunk = round_up(Ms, 64);
    hipStream_t st = c->stream;
    double *dXs, *dV, *dW, *dvec;
    int32_t *dns;
    GPT_TRY(ensure(c, SLOT_XS, (size_t)Ms * D * sizeof(double), (void **)&dXs));
    GPT_TRY(ensure(c, SLOT_NS, (size_t)Ms * D * sizeof(int32_t), (void **)&dns));
    GPT_TRY(ensure(c, SLOT_SP_V, (size_t)chunk * LDV * sizeof(double), (void **)&dV));
    GPT_TRY(ensure(c, SLOT_SP_W, (size_t)chunk * LDV * sizeof(double), (void **)&dW));
    GPT_TRY(ensure(c, SLOT_VEC, (size_t)3 * chunk * sizeof(double), (void **)&dvec));
    double *dmean = dvec, *dkd = dvec + chunk, *dvar = dvec + 2 * chunk;
    GPT_HIP_CHECK(hipMemcpyAsync(dXs, Xstar, (size_t)Ms * D * sizeof(double), hipMemcpyHostToDevice, st));
    GPT_HIP_CHECK(hipMemcpyAsync(dns, nstar, (size_t)Ms * D * sizeof(int32_t), hipMemcpyHostToDevice, st));
    KParams kn;
    if (noise_params) GPT_TRY(make_kparams(GPT_KERNEL_DIAGNOISE, noise_params, 1, D, -1, 1, noise_n, &kn));
    for (int64_t r0 = 0; r0 < Ms; r0 += chunk) {
        const int64_t rows = (Ms - r0 < chunk) ? Ms - r0 : chunk;
        const double *dXc = dXs + r0 * D;
        const int32_t *dnc = dns + r0 * D;
        GPT_TRY(sparse_chunk_vw(c, st, model, res, dXc, dnc, rows, dV, dW));
        GPT_TRY(launch_gemv_n(st, rows, M, dW, LDV, res.c, dmean));
        GPT_HIP_CHECK(hipMemcpyAsync(mean_out + r0, dmean, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, st));
        if (want == 1) {
            GPT_TRY(sparse_kdiag(st, model, dXc, dnc, rows, dkd));
            GPT_TRY(launch_sparse_var(st, dV, dW, LDV, rows, M, dkd, dvar));
            GPT_HIP_CHECK(hipMemcpyAsync(std_out + r0, dvar, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        // (the copies leave the chunk's buffers before the next chunk overwrites them: same stream)
    }
    if (want == 1) {
        GPT_HIP_CHECK(hipStreamSynchronize(st));
        double nv = 0.0;
        for (int64_t a = 0; a < Ms; a++) {
            if (noise_params) {          // diagonal of the symmetric noise term (ref: noise.py:103-104)
                bool hit = true;
                for (int d = 0; d < D; d++) hit = hit && nstar[a * D + d] == kn.noise_n[d];
                nv = hit ? noise_params[0] * noise_params[0] : 0.0;
            }
            std_out[a] = sqrt(std_out[a] + nv);
        }
        return GPT_OK;
    }
    if (want == 2) {
        // cov = K(X*, X*) - V V^T + W W^T, lower triangle by two SYRK-shaped GEMMs, then mirrored
        const int64_t SP = round_up(Ms, 64);
        double *dcov;
        GPT_TRY(ensure(c, SLOT_KSS, (size_t)SP * SP * sizeof(double), (void **)&dcov));
        c->cov_M = 0;                                                // (SLOT_KSS no longer holds gpt_predict's covariance)
        GPT_TRY(launch_zero2d(st, SP, SP, dcov, SP));
        GPT_TRY(kbuild_terms(st, model, 1, dXs, dns, Ms, dXs, dns, Ms, 0, 0, 0, nullptr, 0.0, 0.0, dcov, SP));
        if (noise_params) GPT_TRY(launch_add_noise_sym(st, kn, dXs, dns, Ms, dcov, SP));
        GPT_HIP_CHECK(hipMemset2DAsync(dW + M, (size_t)LDV * sizeof(double), 0, sizeof(double), (size_t)SP, st));      // the augmented column
        GPT_TRY(gemm_nt(c, st, SP, SP, MPU, -1.0, dV, LDV, dV, LDV, 1.0, dcov, SP, 1));
        GPT_TRY(gemm_nt(c, st, SP, SP, MPU, 1.0, dW, LDV, dW, LDV, 1.0, dcov, SP, 1));
        GPT_TRY(launch_mirror_rows(st, dcov, SP, 0, SP, SP));
        GPT_HIP_CHECK(hipMemcpy2DAsync(cov_out, (size_t)Ms * sizeof(double), dcov, (size_t)SP * sizeof(double), (size_t)Ms * sizeof(double),
                                       (size_t)Ms, hipMemcpyDeviceToHost, st));
        GPT_HIP_CHECK(hipStreamSynchronize(st));
        if (std_out)
            for (int64_t a = 0; a < Ms; a++) std_out[a] = sqrt(cov_out[a * Ms + a]);
        return GPT_OK;
    }
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    return GPT_OK;
}

// The Gram kernel on raw device pointers (device API, on the context's stream): dG (mg x mg, lower 64 x 64 tiles) += dV^T dV over
// `rows` rows.  nslices = 0: the fit's own choice.  The partial tiles go to the context's workspace.  gpt_dev_sparse_gram2 (the gradient's
// signed-weight Gram, DESIGN.md 18.8): dG += dA^T dV, both rows x ldv.  One body: `two` says which entry point speaks.
static int dev_sparse_gram(gpt_ctx *c, bool two, const double *dA, const double *dV, int64_t ldv, int64_t rows, int64_t mg, int nslices,
                           double *dG, int64_t ldg)
{
    CTX_ENTER(c);
    if ((two && !dA) || !dV || !dG || rows <= 0 || mg <= 0 || mg % 64) {
        gpt_set_error("%s: bad arguments (rows=%lld, order %lld: a positive multiple of 64)", two ? "gpt_dev_sparse_gram2" : "gpt_dev_sparse_gram",
                      (long long)rows, (long long)mg);
        return GPT_E_ARG;
    }
    if (nslices <= 0) GPT_TRY(sparse_slices(c, mg, rows, &nslices));
    double *dPart;
    GPT_TRY(sparse_part(c, nslices, mg, &dPart));
    return launch_sparse_gram(c->stream, two ? dA : nullptr, dV, ldv, rows, mg, nslices, dPart, dG, ldg);
}

extern "C" int gpt_dev_sparse_gram(gpt_ctx *c, const double *dV, int64_t ldv, int64_t rows, int64_t mg, int nslices, double *dG,
                                   int64_t ldg)
{
    return dev_sparse_gram(c, false, nullptr, dV, ldv, rows, mg, nslices, dG, ldg);
}

extern "C" int gpt_dev_sparse_gram2(gpt_ctx *c, const double *dA, const double *dV, int64_t ldv, int64_t rows, int64_t mg, int nslices,
                                    double *dG, int64_t ldg)
{
    return dev_sparse_gram(c, true, dA, dV, ldv, rows, mg, nslices, dG, ldg);
}

// The four other kernels of ksparse.hip on raw device pointers (device API, on the context's stream): one launcher each, nothing
// added but the refusal of null pointers and of orders the launcher would read or write past (tests/test_gpu_sparse.py checks each
// kernel alone through these).
extern "C" int gpt_dev_sparse_lambda(gpt_ctx *c, double *dV, int64_t ldv, int64_t rows, int64_t M, int method, const double *d_kdiag,
                                     const double *d_r, const double *d_err, double noise_var, double *d_rowval, int64_t ldr,
                                     int32_t *d_bad)
{
    CTX_ENTER(c);
    if (!dV || !d_kdiag || !d_r || !d_err || !d_rowval || !d_bad || rows <= 0 || M < 1 || method < GPT_SPARSE_FITC ||
        method > GPT_SPARSE_DTC) {
        gpt_set_error("gpt_dev_sparse_lambda: bad arguments (rows=%lld, M=%lld, method %d)", (long long)rows, (long long)M, method);
        return GPT_E_ARG;
    }
    return launch_sparse_lambda(c->stream, dV, ldv, rows, M, method, d_kdiag, d_r, d_err, noise_var, d_rowval, ldr, d_bad);
}

extern "C" int gpt_dev_sparse_rowsum(gpt_ctx *c, const double *d_rowval, int64_t ldr, int64_t rows, double *d_acc)
{
    CTX_ENTER(c);
    if (!d_rowval || !d_acc || rows <= 0 || rows > ldr) {
        gpt_set_error("gpt_dev_sparse_rowsum: bad arguments (rows=%lld, row stride %lld)", (long long)rows, (long long)ldr);
        return GPT_E_ARG;
    }
    return launch_sparse_rowsum(c->stream, d_rowval, ldr, rows, d_acc);
}

extern "C" int gpt_dev_sparse_var(gpt_ctx *c, const double *dV, const double *dW, int64_t ld, int64_t rows, int64_t M,
                                  const double *d_kdiag, double *d_var)
{
    CTX_ENTER(c);
    if (!dV || !dW || !d_kdiag || !d_var || rows <= 0 || M < 1 || M > ld) {
        gpt_set_error("gpt_dev_sparse_var: bad arguments (rows=%lld, M=%lld, row stride %lld)", (long long)rows, (long long)M, (long long)ld);
        return GPT_E_ARG;
    }
    return launch_sparse_var(c->stream, dV, dW, ld, rows, M, d_kdiag, d_var);
}

extern "C" int gpt_dev_sparse_assemble_b(gpt_ctx *c, const double *dG, int64_t ldg, int64_t M, double *dB, int64_t bp, double big)
{
    CTX_ENTER(c);
    if (!dG || !dB) {
        gpt_set_error("gpt_dev_sparse_assemble_b: bad arguments");
        return GPT_E_ARG;
    }
    return launch_sparse_assemble_b(c->stream, dG, ldg, M, dB, bp, big);
}
