// api_sparse_select.inc -- part of api.hip (ONE translation unit: included from there, behind api_sparse.inc).  Greedy
// conditional-variance choice of the inducing inputs (DESIGN.md section 18.10): gpt_sparse_select_inducing and the device API of its two
// kernels, gpt_dev_greedy_update / gpt_dev_greedy_pick (kgreedy.hip).
// ------------------------------------------------------------------------------------------------
// Layout.  The candidates are gathered into a point set of their own (SLOT_SP_SEL_X: Xc, ncand x D, their all-zero orders and the row
// indices), so the builder and the pair pass see ncand plain points.  The factor (SLOT_SP_SEL_L) is column-major, CP = ncand rounded up
// to 64 rows by M columns; the rows [ncand, CP) are never read or written.  SLOT_SP_SEL_MISC holds the residuals, the partials, the two
// scalars, the staging point x_p and the staging row L[p, 0:j), the three outputs, the marks, the words and D zero orders for x_p.
// Neither the dense factor nor a resident sparse fit (SLOT_SP_Z / _LU / _LB and what a fit or a prediction sizes) is touched.
// ------------------------------------------------------------------------------------------------

// ensure() for the selection's slots: a failed allocation answers GPT_E_NOMEM with the byte count
static int select_ensure(gpt_ctx *c, int slot, size_t bytes, const char *what, void **out)
{
    const int rc = ensure(c, slot, bytes, out);
    if (rc == GPT_E_NOMEM) {
        (void)hipGetLastError();
        gpt_set_error("gpt_sparse_select_inducing: cannot allocate %zu bytes of device memory for %s", bytes, what);
    }
    return rc;
}

extern "C" int gpt_sparse_select_inducing(gpt_ctx *c, int nterms, const int *kernel_ids, const int *kernel_ids2, const double *params,
                                          const int *nparams, const int *nparams1, const int32_t *cand, int64_t ncand, int64_t M, double tol,
                                          int32_t *idx_out, double *dmax_out, double *trace_out, int64_t *count_out)
{
    CTX_ENTER(c);
    const char *who = "gpt_sparse_select_inducing";
    if (!c->dX) {
        gpt_set_error("%s: call gpt_set_data first", who);
        return GPT_E_STATE;
    }
    if (c->dT) {
        gpt_set_error("%s is not available with a linear transform set (gpt_set_T)", who);
        return GPT_E_NOTIMPL;
    }
    GPT_TRY(refuse_warp(c, who));
    if (!kernel_ids || !kernel_ids2 || !params || !nparams || !nparams1 || !idx_out || !dmax_out || !trace_out || !count_out) {
        gpt_set_error("%s: a NULL argument", who);
        return GPT_E_ARG;
    }
    if (M < 1 || M > 65000 || !(tol >= 0.0)) {
        gpt_set_error("%s: bad arguments (M=%lld: 1 .. 65000, tol=%g: non-negative)", who, (long long)M, tol);
        return GPT_E_ARG;
    }
    const int D = c->D;
    const int64_t N = c->Nx;
    hipStream_t st = c->stream;
    // ---- the candidates: rows with all orders zero
    std::vector<int32_t> hn((size_t)N * D), hc;
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    GPT_HIP_CHECK(hipMemcpy(hn.data(), c->dn, hn.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    auto plain = [&](int64_t i) {
        for (int d = 0; d < D; d++)
            if (hn[(size_t)i * D + d] != 0) return false;
        return true;
    };
    if (!cand) {
        for (int64_t i = 0; i < N; i++)
            if (plain(i)) hc.push_back((int32_t)i);
    } else {
        if (ncand < 1) {
            gpt_set_error("%s: an empty candidate list", who);
            return GPT_E_ARG;
        }
        for (int64_t r = 0; r < ncand; r++) {
            if (cand[r] < 0 || cand[r] >= N || (r > 0 && cand[r] <= cand[r - 1])) {
                gpt_set_error("%s: candidate %lld is row %d: the list must be strictly ascending within [0, %lld)", who, (long long)r, (int)cand[r],
                              (long long)N);
                return GPT_E_ARG;
            }
            if (!plain(cand[r])) {
                gpt_set_error("%s: candidate row %d has a non-zero derivative order (only value rows can be inducing inputs here)", who,
                              (int)cand[r]);
                return GPT_E_ARG;
            }
        }
        hc.assign(cand, cand + ncand);
    }
    ncand = (int64_t)hc.size();
    if (M > ncand) {
        gpt_set_error("%s: M = %lld exceeds the %lld candidates", who, (long long)M, (long long)ncand);
        return GPT_E_ARG;
    }
    ModelKernel model;
    GPT_TRY(parse_model(D, c->n_maxsum, c->n_colmax, nterms, kernel_ids, kernel_ids2, params, nparams, nparams1, &model));
    // ---- device memory
    const int64_t CP = round_up(ncand, 64), nparts = greedy_blocks(ncand);
    double *dL, *dXc, *dMisc;
    GPT_TRY(select_ensure(c, SLOT_SP_SEL_L, (size_t)CP * M * sizeof(double), "the factor (candidates rounded up to 64, times M doubles)",
                          (void **)&dL));
    GPT_TRY(select_ensure(c, SLOT_SP_SEL_X, (size_t)ncand * D * (sizeof(double) + sizeof(int32_t)) + (size_t)ncand * sizeof(int32_t),
                          "the candidates", (void **)&dXc));
    int32_t *dnc = reinterpret_cast<int32_t *>(dXc + ncand * D), *dcand = dnc + ncand * D;
    // doubles: residuals (CP), partials (2 nparts), scalars (2), x_p (GPT_MAX_DIM), the pivot's row (M), dmax (M), trace (M + 1); then
    // int32: marks (CP), the partials' rows (nparts), words (4), zero orders of x_p (GPT_MAX_DIM), idx (M)
    const size_t ndbl = (size_t)CP + 2 * nparts + 2 + GPT_MAX_DIM + 3 * M + 1, nint = (size_t)CP + nparts + 4 + GPT_MAX_DIM + M;
    GPT_TRY(select_ensure(c, SLOT_SP_SEL_MISC, ndbl * sizeof(double) + nint * sizeof(int32_t), "the residuals and partials", (void **)&dMisc));
    double *dres = dMisc, *dpart = dres + CP, *dscal = dpart + 2 * nparts, *dxp = dscal + 2, *dprow = dxp + GPT_MAX_DIM, *ddmax = dprow + M,
           *dtrace = ddmax + M;
    int32_t *dmark = reinterpret_cast<int32_t *>(dMisc + ndbl), *dpidx = dmark + CP, *dwords = dpidx + nparts, *dnp = dwords + 4,
            *didx = dnp + GPT_MAX_DIM;
    EvalScope scope(c, true);                                        // counted like an evaluation in flight, on event edges
    GPT_HIP_CHECK(hipMemcpyAsync(dcand, hc.data(), (size_t)ncand * sizeof(int32_t), hipMemcpyHostToDevice, st));
    GPT_HIP_CHECK(hipMemsetAsync(dscal, 0, (2 + GPT_MAX_DIM) * sizeof(double), st));
    GPT_HIP_CHECK(hipMemsetAsync(dwords, 0, (4 + GPT_MAX_DIM) * sizeof(int32_t), st));
    GPT_TRY(launch_greedy_gather(st, c->dX, dcand, ncand, D, dXc, dnc));
    // ---- d_i = k(x_i, x_i), then M times pick / column / update, and the closing pick for trace_M: no host synchronisation in between
    GPT_TRY(sparse_kdiag(st, model, dXc, dnc, ncand, dres));
    GPT_TRY(launch_greedy_init(st, ncand, dres, dmark, dpart, dpidx));
    for (int64_t j = 0; j <= M; j++) {
        GPT_TRY(launch_greedy_pick(st, j, M, tol, dpart, dpidx, nparts, dcand, dXc, D, dL, CP, dmark, dscal, dwords, didx, ddmax, dtrace, dxp,
                                   dprow));
        if (j == M) break;
        // column j = k(x_p, x_i) over the candidates: ONE row of the builder (the pivot) against ncand columns (its lanes), every term of the
        // model through kbuild_terms as the fits build K_fu.  After a stop the column holds pairs of a stale pivot; nothing reads it.
        GPT_TRY(kbuild_terms(st, model, 0, dxp, dnp, 1, dXc, dnc, ncand, 0, 0, 0, nullptr, 0.0, 0.0, dL + j * CP, CP));
        GPT_TRY(launch_greedy_update(st, dL, CP, ncand, j, dL + j * CP, dres, dmark, dprow, dscal, dwords, dpart, dpidx));
    }
    int32_t words[4];
    GPT_HIP_CHECK(hipMemcpyAsync(idx_out, didx, (size_t)M * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipMemcpyAsync(dmax_out, ddmax, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipMemcpyAsync(trace_out, dtrace, (size_t)(M + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipMemcpyAsync(words, dwords, sizeof(words), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    const int64_t count = words[GPT_GREEDY_W_COUNT];
    for (int64_t k = count; k < M; k++) {
        idx_out[k] = -1;
        dmax_out[k] = NAN;
        trace_out[k + 1] = NAN;
    }
    *count_out = count;
    if (words[GPT_GREEDY_W_BAD] != 0 || count < 1) {
        gpt_set_error("%s: the largest k(x_i, x_i) of the candidates is not a positive finite number", who);
        return GPT_E_VALUE;
    }
    return GPT_OK;
}

// The two kernels of kgreedy.hip on raw device pointers (device API, on the context's stream): the launchers, nothing added but the
// refusal of null pointers (tests/test_gpu_greedy.py checks each kernel alone through these)
extern "C" int64_t gpt_dev_greedy_parts(int64_t rows) { return greedy_blocks(rows); }

extern "C" int gpt_dev_greedy_update(gpt_ctx *c, const double *dL, int64_t ld, int64_t rows, int64_t j, double *d_col, double *d_resid,
                                     const int32_t *d_mark, const double *d_prow, const double *d_scal, const int32_t *d_words, double *d_part,
                                     int32_t *d_pidx)
{
    CTX_ENTER(c);
    if (!dL || !d_col || !d_resid || !d_mark || !d_prow || !d_scal || !d_words || !d_part || !d_pidx) {
        gpt_set_error("gpt_dev_greedy_update: a NULL argument");
        return GPT_E_ARG;
    }
    return launch_greedy_update(c->stream, dL, ld, rows, j, d_col, d_resid, d_mark, d_prow, d_scal, d_words, d_part, d_pidx);
}

extern "C" int gpt_dev_greedy_pick(gpt_ctx *c, int64_t j, int64_t M, double tol, const double *d_part, const int32_t *d_pidx, int64_t nparts,
                                   const int32_t *d_cand, const double *dX, int D, const double *dL, int64_t ld, int32_t *d_mark,
                                   double *d_scal, int32_t *d_words, int32_t *d_idx, double *d_dmax, double *d_trace, double *d_xp,
                                   double *d_prow)
{
    CTX_ENTER(c);
    if (!d_part || !d_pidx || !dX || !dL || !d_mark || !d_scal || !d_words || !d_idx || !d_dmax || !d_trace || !d_xp || !d_prow) {
        gpt_set_error("gpt_dev_greedy_pick: a NULL argument");
        return GPT_E_ARG;
    }
    return launch_greedy_pick(c->stream, j, M, tol, d_part, d_pidx, nparts, d_cand, dX, D, dL, ld, d_mark, d_scal, d_words, d_idx, d_dmax,
                              d_trace, d_xp, d_prow);
}
