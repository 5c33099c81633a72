// api_fit.inc -- part of api.hip (ONE translation unit: included from there, in this order; the parts share struct gpt_ctx and
// static helpers).  Data residency and the fit: gpt_set_data, gpt_set_T, gpt_fit, gpt_fit_sum, gpt_fit_terms, gpt_fit_matrix.
// ------------------------------------------------------------------------------------------------
// data residency + fit
// ------------------------------------------------------------------------------------------------
extern "C" int gpt_set_data(gpt_ctx *c, const double *X, const int32_t *n, int64_t N, int D)
{
    CTX_ENTER(c);
    if (N <= 0 || !X || !n || D < 1 || D > GPT_MAX_DIM) {
        gpt_set_error("set_data: bad arguments (N=%lld, D=%d)", (long long)N, D);
        return GPT_E_ARG;
    }
    GPT_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (c->dX) hipFree(c->dX);
    if (c->dn) hipFree(c->dn);
    c->dX = nullptr;
    c->dn = nullptr;
    if (c->dXw) hipFree(c->dXw);       // warp layers belong to one data set
    if (c->dS) hipFree(c->dS);
    c->dXw = c->dS = nullptr;
    c->warp.nlayers = 0;
    c->warpb_nbatch = 0;
    GPT_HIP_CHECK(hipMalloc(&c->dX, (size_t)N * D * sizeof(double)));
    GPT_HIP_CHECK(hipMalloc(&c->dn, (size_t)N * D * sizeof(int32_t)));
    GPT_HIP_CHECK(hipMemcpyAsync(c->dX, X, (size_t)N * D * sizeof(double), hipMemcpyHostToDevice, c->stream));
    GPT_HIP_CHECK(hipMemcpyAsync(c->dn, n, (size_t)N * D * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    GPT_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->N = N;
    c->Nx = N;
    c->D = D;
    c->n_maxsum = c->n_maxord = 0;
    for (int d = 0; d < GPT_MAX_DIM; d++) c->n_colmax[d] = 0;
    for (int64_t i = 0; i < N; i++) {
        long sn = 0;
        for (int d = 0; d < D; d++) {
            sn += n[i * D + d];
            if (n[i * D + d] > c->n_maxord) c->n_maxord = n[i * D + d];
            if (n[i * D + d] > c->n_colmax[d]) c->n_colmax[d] = n[i * D + d];
        }
        if (sn > c->n_maxsum) c->n_maxsum = sn;
    }
    invalidate_factor(c);
    c->have_kernel = false;
    c->batch_gen++;                     // (the resident batch was fitted to the old data)
    c->sp_M = 0;                        // (the inducing points and the sparse fit belong to one data set: gpt_sparse_set_inducing)
    c->sp_fitted = false;
    c->sp_chunk_rows = 0;
    if (c->dT) hipFree(c->dT);          // a transform belongs to one data set
    c->dT = nullptr;
    c->Ny = 0;
    return GPT_OK;
}

// Linear transform of the latent values (ref: gptools/gaussian_process.py:376-503 `T`, :1443-1446): the observations are
// y = T f(X) + noise, K_tot = T (K + noise_K) T^T + diag(err_y^2) + diag_add I  (Ny x Ny).  T stays resident until the
// data change; T == NULL removes it.
extern "C" int gpt_set_T(gpt_ctx *c, const double *T, int64_t Ny)
{
    CTX_ENTER(c);
    if (!c->dX) {
        gpt_set_error("gpt_set_T: call gpt_set_data first");
        return GPT_E_STATE;
    }
    GPT_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (c->dT) hipFree(c->dT);
    c->dT = nullptr;
    c->Ny = 0;
    invalidate_factor(c);
    c->have_kernel = false;
    c->batch_gen++;
    if (!T || Ny <= 0) return GPT_OK;
    const int64_t NyP = round_up(Ny, 64), NxP = round_up(c->Nx, 16);
    GPT_HIP_CHECK(hipMalloc(&c->dT, (size_t)NyP * NxP * sizeof(double)));
    GPT_HIP_CHECK(hipMemsetAsync(c->dT, 0, (size_t)NyP * NxP * sizeof(double), c->stream));
    GPT_HIP_CHECK(hipMemcpy2DAsync(c->dT, (size_t)NxP * sizeof(double), T, (size_t)c->Nx * sizeof(double),
                                   (size_t)c->Nx * sizeof(double), (size_t)Ny, hipMemcpyHostToDevice, c->stream));
    GPT_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->Ny = Ny;
    c->NxP = NxP;
    return GPT_OK;
}

// Input warp (include/gpt_hip.h): the layers by value in the context, the warped resident points and their slope factors next
// to dX.  Recomputed by every call -- warp parameters are hyperparameters -- on the context's stream, in front of the next build.
extern "C" int gpt_set_warp(gpt_ctx *c, int nlayers, const int *types, const double *params)
{
    CTX_ENTER(c);
    if (nlayers == 0 && c->warp.nlayers == 0) return GPT_OK;      // nothing set, nothing to clear: the resident factor stays
    invalidate_factor(c);
    c->have_kernel = false;
    c->cov_M = 0;
    if (nlayers == 0) {
        c->warp.nlayers = 0;
        return GPT_OK;
    }
    if (!c->dX) {
        gpt_set_error("gpt_set_warp: call gpt_set_data first");
        return GPT_E_STATE;
    }
    if (nlayers < 0 || nlayers > GPT_WARP_MAX_LAYERS || !types || !params) {
        gpt_set_error("gpt_set_warp: %d layers (at most %d)", nlayers, GPT_WARP_MAX_LAYERS);
        return GPT_E_ARG;
    }
    WarpLayers wl = WarpLayers();
    wl.nlayers = nlayers;
    wl.D = c->D;
    for (int l = 0; l < nlayers; l++) {
        if (types[l] != GPT_WARP_LINEAR && types[l] != GPT_WARP_BETA) {
            gpt_set_error("gpt_set_warp: unknown warp type %d", types[l]);
            return GPT_E_ARG;
        }
        wl.type[l] = types[l];
        memcpy(wl.p[l], params + (size_t)l * 2 * c->D, (size_t)2 * c->D * sizeof(double));
    }
    c->warp.nlayers = 0;                       // (nothing half set should an allocation or the launch fail)
    if (c->n_maxord > 1) {
        gpt_set_error("%s", WARP_ORDER_MSG);
        return GPT_E_VALUE;
    }
    if (!c->dXw) GPT_HIP_CHECK(hipMalloc(&c->dXw, (size_t)c->Nx * c->D * sizeof(double)));
    if (!c->dS) GPT_HIP_CHECK(hipMalloc(&c->dS, (size_t)c->Nx * sizeof(double)));
    if (c->debug_poison) {                     // (test aid: whatever the warp kernel does not write shows up as NaN)
        GPT_HIP_CHECK(hipMemsetAsync(c->dXw, 0xff, (size_t)c->Nx * c->D * sizeof(double), c->stream));
        GPT_HIP_CHECK(hipMemsetAsync(c->dS, 0xff, (size_t)c->Nx * sizeof(double), c->stream));
    }
    GPT_TRY(launch_warp_points(c->stream, wl, c->dX, c->dn, c->Nx, c->dXw, c->dS));
    c->warp = wl;
    return GPT_OK;
}

// Per-element warps of a batch (include/gpt_hip.h): one launch fills nbatch x Nx x D warped points and nbatch x Nx slope factors;
// the next gpt_fit_batch* of nbatch elements builds element b from its own.  The resident single factorisation is untouched.
extern "C" int gpt_set_warp_batch(gpt_ctx *c, int nbatch, int nlayers, const int *types, const double *params)
{
    CTX_ENTER(c);
    c->warpb_nbatch = 0;
    if (nlayers == 0 || nbatch == 0) return GPT_OK;
    if (!c->dX) {
        gpt_set_error("gpt_set_warp_batch: call gpt_set_data first");
        return GPT_E_STATE;
    }
    if (nbatch < 0 || nbatch > 65535 || nlayers < 0 || nlayers > GPT_WARP_MAX_LAYERS || !types || !params) {
        gpt_set_error("gpt_set_warp_batch: %d elements, %d layers (at most %d)", nbatch, nlayers, GPT_WARP_MAX_LAYERS);
        return GPT_E_ARG;
    }
    WarpLayers wl = WarpLayers();
    wl.nlayers = nlayers;
    wl.D = c->D;
    for (int l = 0; l < nlayers; l++) {
        if (types[l] != GPT_WARP_LINEAR && types[l] != GPT_WARP_BETA) {
            gpt_set_error("gpt_set_warp_batch: unknown warp type %d", types[l]);
            return GPT_E_ARG;
        }
        wl.type[l] = types[l];
    }
    if (c->n_maxord > 1) {
        gpt_set_error("%s", WARP_ORDER_MSG);
        return GPT_E_VALUE;
    }
    const size_t np = (size_t)nbatch * nlayers * 2 * c->D, nx = (size_t)nbatch * c->Nx * c->D, ns = (size_t)nbatch * c->Nx;
    double *dP, *dXb, *dSb;
    GPT_TRY(ensure(c, SLOT_WB_P, np * sizeof(double), (void **)&dP));
    GPT_TRY(ensure(c, SLOT_WB_X, nx * sizeof(double), (void **)&dXb));
    GPT_TRY(ensure(c, SLOT_WB_S, ns * sizeof(double), (void **)&dSb));
    hipStream_t st = c->stream;
    // (the caller's array is pageable: the copy has left it when the call returns)
    GPT_HIP_CHECK(hipMemcpyAsync(dP, params, np * sizeof(double), hipMemcpyHostToDevice, st));
    if (c->debug_poison) {
        GPT_HIP_CHECK(hipMemsetAsync(dXb, 0xff, nx * sizeof(double), st));
        GPT_HIP_CHECK(hipMemsetAsync(dSb, 0xff, ns * sizeof(double), st));
    }
    GPT_TRY(launch_warp_points_batch(st, wl, dP, nbatch, c->dX, c->dn, c->Nx, dXb, dSb));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    c->warpb_nbatch = nbatch;
    return GPT_OK;
}

// the points / slope factors the builders take for the resident data: warped while layers are set
static inline const double *model_X(const gpt_ctx *c) { return c->warp.nlayers > 0 ? c->dXw : c->dX; }
static inline const double *model_S(const gpt_ctx *c) { return c->warp.nlayers > 0 ? c->dS : nullptr; }

static int refuse_warp(const gpt_ctx *c, const char *what)
{
    if (c->warp.nlayers > 0) {
        gpt_set_error("%s is not available while warp layers are set (gpt_set_warp)", what);
        return GPT_E_NOTIMPL;
    }
    return GPT_OK;
}

static int ensure_factor_storage(gpt_ctx *c, int64_t N)
{
    const int64_t NP = round_up(N + 1, 128);
    if (c->NP == NP && c->dA) return GPT_OK;
    GPT_HIP_CHECK(hipStreamSynchronize(c->stream));
    free_factor(c);
    GPT_HIP_CHECK(hipMalloc(&c->dA, (size_t)NP * NP * sizeof(double)));
    GPT_HIP_CHECK(hipMalloc(&c->d_invd, (size_t)(NP / 128) * GPT_WS_BLOCK * sizeof(double)));
    GPT_HIP_CHECK(hipMalloc(&c->d_y, (size_t)2 * NP * sizeof(double)));          // y | err_y, one upload per evaluation
    c->d_erry = c->d_y + NP;
    GPT_HIP_CHECK(hipHostMalloc((void **)&c->h_yerr, (size_t)2 * NP * sizeof(double), hipHostMallocDefault));
    GPT_HIP_CHECK(hipHostMalloc((void **)&c->h_alpha, (size_t)NP * sizeof(double), hipHostMallocDefault));
    GPT_HIP_CHECK(hipMalloc(&c->d_alpha, (size_t)2 * NP * sizeof(double)));      // alpha | work vector of its substitution
    c->NP = NP;
    return GPT_OK;
}

// Factor the (already assembled, lower) N x N matrix in dA, with y in d_y; produce ll terms.
static int harvest_gemm_profile(gpt_ctx *c);
static int alpha_to_host(gpt_ctx *c, hipStream_t on = nullptr);

// `req`: what the caller knows about the K build in front of the factorisation (PotrfRequest::head_event / head_wait)
static int factor_and_ll(gpt_ctx *c, int64_t N, double *ll_data_out, double *logdet_half_out, bool padded = false,
                         PotrfRequest req = PotrfRequest())
{
    hipStream_t st = c->stream;
    const int64_t NP = c->NP;
    if (!padded) {
        GPT_HIP_CHECK(hipMemsetAsync(c->d_info, 0, sizeof(int32_t), st));
        GPT_TRY(launch_fill_pad(st, c->dA, NP, N, NP, c->d_y, 1e300));
    }
    if (c->timing) GPT_HIP_CHECK(hipEventRecord(c->tev[2], st));
    // The factorisation ends on the panel stream (its last leaf); the reduction over the diagonal and the augmented row
    // and the 24-byte copy follow it THERE -- handing back to the main stream first cost an event edge (~20 us of a 5 ms
    // evaluation) -- and the main stream is joined behind them, off the host's critical path.
    req.defer_join = true;
    c->binv_early = 0;
    req.want_early_binv = c->eager_alpha != 0 && !c->use_graph;
    // (the eager substitution's fast path -- ensure_alpha: N a multiple of 512, at least 1024 -- reads nothing of the last leaf then)
    req.defer_pad_leaf = req.want_early_binv && c->defer_pad && N % 512 == 0 && N >= 1024 && NP == N + 128;
    req.live_rows = N + 1;                 // the data rows and the augmented row; rows N+1 ... NP-1 are padding (fill_pad_kernel)
    PotrfResult fac;
    GPT_TRY(potrf_run(c, NP, c->dA, NP, c->d_invd, c->d_info, req, &fac));
    const bool pad_on_main = fac.pad_leaf_deferred;
    hipStream_t tl = fac.tail_stream ? fac.tail_stream : st;
    // (the three results go straight to pinned host memory, and the two timing events ride on the kernel's dispatch packet:
    // a copy kernel and two barrier packets less on the tail of every evaluation, ~15 us)
    // (only a STOP event: a start event on the packet holds the kernel back ~7 us like a barrier packet would)
    // Eager alpha: the reduction and the substitution are independent of each other -- the reduction then goes to the MAIN stream
    // (idle by now; one event edge, off alpha's path) and the substitution's first kernel follows the factorisation's last one
    // directly on the tail stream.
    bool joined = false;
    hipStream_t red_st = tl;
    if (pad_on_main && tl != st) {
        // the pad leaf is on the main stream already (behind an event of the last real leaf): the reduction follows it there,
        // the substitution follows the last real leaf on the tail stream -- no further edge
        red_st = st;
        joined = true;
    } else if (c->eager_alpha && tl != st) {
        GPT_TRY(stream_follows(c, tl, st, 1));
        red_st = st;
        joined = true;
    }
    GPT_TRY(launch_logdet_dot(red_st, c->dA, NP, N, c->d_info, c->d_scal, c->h_scal, nullptr, c->timing ? c->tev[4] : nullptr,
                              c->flags_now ? c->d_edge + 60 : nullptr));
    invalidate_factor(c);                  // (c->factored is false already: every caller drops it in front of its build)
    // option eager_alpha (the reference computes alpha in every evaluation, gaussian_process.py:1462): the substitution goes behind
    // the factorisation at once, ON THE STREAM THE FACTORISATION ENDS ON (no event edge in front of its first kernel; the block
    // inverses left of the last panel were built under that panel, enqueue_early_block_inverses);
    // alpha lands in pinned memory by one copy behind the last step -- gpt_get_alpha is then a host copy.
    // (on a failed factorisation: finite work on garbage, flags reset below.  Should the enqueue itself fail, both streams are
    // still drained before the error leaves -- nothing of this evaluation stays in flight -- and alpha is not marked valid: ADVICE r5.
    // The device timings of gpt_last_timings end at the reduction kernel: an eager evaluation's alpha is not in them, see bench.py.)
    int rc_alpha = c->eager_alpha ? alpha_to_host(c, tl) : GPT_OK;
    c->binv_early = 0;                     // (whatever was built early has been taken up by now, or is not going to be)
    if (tl != st && !joined) GPT_TRY(stream_follows(c, tl, st, 1));
    if (rc_alpha != GPT_OK) {
        invalidate_factor(c);
        if (tl != st) (void)hipStreamSynchronize(tl);
        (void)hipStreamSynchronize(st);
        return rc_alpha;
    }
    if (tl != st) GPT_HIP_CHECK(hipStreamSynchronize(tl));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    if (c->gprof_used) GPT_TRY(harvest_gemm_profile(c));
    if (c->timing) {
        float ms = 0;
        for (int i = 0; i < 2; i++) {
            hipEventElapsedTime(&ms, c->tev[i], c->tev[i + 1]);
            c->timings[i] = ms;
        }
        hipEventElapsedTime(&ms, c->tev[2], c->tev[4]);      // factorisation + the reduction kernel behind it (~5 us)
        c->timings[2] = ms;
        c->timings[3] = 0.0;
        hipEventElapsedTime(&ms, c->tev[0], c->tev[4]);
        c->timings[4] = ms;
    }
    if (c->flags_now && c->h_scal[3] != 0.0) {
        // a flag wait of this evaluation timed out (common.hpp): its numbers mean nothing; the caller repeats it on events
        invalidate_factor(c);
        return GPT_I_EDGE_TIMEOUT;
    }
    const int32_t info = (int32_t)c->h_scal[2];
    if (info != 0) {
        invalidate_factor(c);
        if (info > N) {          // only the augmented / padding pivots failed: z.z overflowed
            gpt_set_error("factorisation failed in the augmented row (non-finite data?)");
            return (int)N;
        }
        gpt_set_error("%d-th leading minor of the array is not positive definite", (int)info);
        return (int)info;
    }
    c->factored = true;
    const double logdet_half = c->h_scal[0], zz = c->h_scal[1];
    if (logdet_half_out) *logdet_half_out = logdet_half;
    if (ll_data_out) *ll_data_out = -0.5 * zz - logdet_half - 0.5 * (double)N * log(2.0 * M_PI);
    return GPT_OK;
}

// K block of the model kernel = the sum of its terms (SumKernel, ref: gptools/kernel/core.py:549-584): one builder pass per
// term (a product term brings its second factor), later passes accumulate; the diagonal epilogue (err != nullptr) rides on the
// last pass, after the sum.
static int kbuild_terms(hipStream_t st, const ModelKernel &m, int symmetric, const double *dXi, const int32_t *dni, int64_t M,
                        const double *dXj, const int32_t *dnj, int64_t P, int lower_only, int64_t i0, int64_t j0,
                        const double *d_err, double noise_var, double diag_add, double *dK, int64_t ldk,
                        const double *dSi = nullptr, const double *dSj = nullptr)
{
    for (int t = 0; t < m.nterms; t++) {
        KParams kp = m.f1[t];
        kp.symmetric = symmetric;
        kp.hyper_deriv = -1;
        const bool last = t + 1 == m.nterms;
        GPT_TRY(launch_kbuild(st, kp, m.second(t), {dXi, dni, M, dXj, dnj, P, lower_only, i0, j0, last ? d_err : nullptr, noise_var,
                                                    diag_add, dK, ldk, t > 0 ? 1 : 0, dSi, dSj}));
    }
    return GPT_OK;
}

static int fit_terms(gpt_ctx *c, const ModelKernel &model, double noise_var, const double *y, const double *err_y,
                     double diag_add, double *ll_data_out, double *logdet_half_out);

extern "C" int gpt_fit(gpt_ctx *c, int kernel_id, const double *params, int nparams, double noise_var,
                       const double *y, const double *err_y, double diag_add, double *ll_data_out,
                       double *logdet_half_out)
{
    return gpt_fit_sum(c, 1, &kernel_id, params, &nparams, noise_var, y, err_y, diag_add, ll_data_out, logdet_half_out);
}

// gpt_fit_sum (no product terms: kernel_ids2 == NULL) and gpt_fit_terms (need_ids2: both product arrays are part of its contract)
static int fit_model(gpt_ctx *c, int nterms, const int *kernel_ids, const int *kernel_ids2, bool need_ids2, const double *params,
                     const int *nparams, const int *nparams1, double noise_var, const double *y, const double *err_y, double diag_add,
                     double *ll_data_out, double *logdet_half_out)
{
    if (!c->dX) {
        gpt_set_error("gpt_fit: call gpt_set_data first");
        return GPT_E_STATE;
    }
    if (!y || !err_y || (need_ids2 && (!kernel_ids2 || !nparams1))) return GPT_E_ARG;
    ModelKernel model;
    GPT_TRY(parse_model(c->D, c->n_maxsum, c->n_colmax, nterms, kernel_ids, kernel_ids2, params, nparams, nparams1, &model));
    return fit_terms(c, model, noise_var, y, err_y, diag_add, ll_data_out, logdet_half_out);
}

extern "C" int gpt_fit_sum(gpt_ctx *c, int nterms, const int *kernel_ids, const double *params, const int *nparams,
                           double noise_var, const double *y, const double *err_y, double diag_add,
                           double *ll_data_out, double *logdet_half_out)
{
    CTX_ENTER(c);
    return fit_model(c, nterms, kernel_ids, nullptr, false, params, nparams, nullptr, noise_var, y, err_y, diag_add, ll_data_out,
                     logdet_half_out);
}

// The same with product terms (include/gpt_hip.h)
extern "C" int gpt_fit_terms(gpt_ctx *c, int nterms, const int *kernel_ids, const int *kernel_ids2, const double *params,
                             const int *nparams, const int *nparams1, double noise_var, const double *y, const double *err_y,
                             double diag_add, double *ll_data_out, double *logdet_half_out)
{
    CTX_ENTER(c);
    return fit_model(c, nterms, kernel_ids, kernel_ids2, true, params, nparams, nparams1, noise_var, y, err_y, diag_add, ll_data_out,
                     logdet_half_out);
}

static int fit_terms_once(gpt_ctx *c, const ModelKernel &model, double noise_var, const double *y,
                          const double *err_y, double diag_add, double *ll_data_out, double *logdet_half_out);

// An evaluation whose flag wait timed out: the process goes to event edges for good and the evaluation runs again.
static int edge_timeout_fallback(gpt_ctx *c)
{
    g_flags_tripped.store(true);
    hipStreamSynchronize(c->stream);
    hipStreamSynchronize(c->panel_stream);
    static bool told = false;
    if (!told) {
        told = true;
        fprintf(stderr, "libgpt_hip: a flag-edge wait timed out (GPU shared with other work, or kernels serialised by a tool); "
                        "this process uses event edges from now on (GPT_EDGE_FLAGS=0 avoids the attempt)\n");
    }
    return GPT_OK;
}

static int fit_terms(gpt_ctx *c, const ModelKernel &model, double noise_var, const double *y, const double *err_y,
                     double diag_add, double *ll_data_out, double *logdet_half_out)
{
    int rc;
    {
        EvalScope scope(c);
        rc = fit_terms_once(c, model, noise_var, y, err_y, diag_add, ll_data_out, logdet_half_out);
    }
    if (rc == GPT_I_EDGE_TIMEOUT) {
        edge_timeout_fallback(c);
        EvalScope scope(c);
        rc = fit_terms_once(c, model, noise_var, y, err_y, diag_add, ll_data_out, logdet_half_out);
    }
    return rc;
}

static int fit_terms_once(gpt_ctx *c, const ModelKernel &model, double noise_var, const double *y,
                          const double *err_y, double diag_add, double *ll_data_out, double *logdet_half_out)
{
    const int64_t Nx = c->Nx;
    const int64_t N = c->dT ? c->Ny : Nx;          // order of K_tot
    const double *mX = model_X(c), *mS = model_S(c);      // (warp layers set: the warped points and their slope factors)
    c->N = N;
    GPT_TRY(ensure_factor_storage(c, N));
    hipStream_t st = c->stream;
    c->factored = false;
    if (c->timing) GPT_HIP_CHECK(hipEventRecord(c->tev[0], st));
    memcpy(c->h_yerr, y, (size_t)N * sizeof(double));
    memcpy(c->h_yerr + c->NP, err_y, (size_t)N * sizeof(double));
    const int64_t NP = c->NP;
    // (kernel path without T: upload, info = 0 and the padding rows are one launch, see upload_pad_kernel)
    const bool one_launch = (c->dT == nullptr) && NP > N;
    if (!one_launch) {
        GPT_HIP_CHECK(hipMemcpyAsync(c->d_y, c->h_yerr, (size_t)(c->NP + N) * sizeof(double), hipMemcpyHostToDevice, st));
        if (c->timing) GPT_HIP_CHECK(hipEventRecord(c->tev[1], st));
        GPT_HIP_CHECK(hipMemsetAsync(c->d_info, 0, sizeof(int32_t), st));
    }
    c->model = model;
    if (c->dT) {
        // ---- T path: K_tot = T (K + noise_var I) T^T + diag(err_y^2) + diag_add I, assembled on the device by the
        // K-builder (full symmetric K over the Nx latent points) and two fp64-MFMA GEMMs (ref :1443-1451)
        const int64_t NxP = c->NxP, NyP = round_up(N, 64);
        double *dK, *dTK, *dzero;
        GPT_TRY(ensure(c, SLOT_KFULL, (size_t)NxP * NxP * sizeof(double), (void **)&dK));
        GPT_TRY(ensure(c, SLOT_TK, (size_t)NyP * NxP * sizeof(double), (void **)&dTK));
        GPT_TRY(ensure(c, SLOT_ZERO, (size_t)Nx * sizeof(double), (void **)&dzero));
        GPT_HIP_CHECK(hipMemsetAsync(dzero, 0, (size_t)Nx * sizeof(double), st));
        if (NxP > Nx) GPT_HIP_CHECK(hipMemsetAsync(dK, 0, (size_t)NxP * NxP * sizeof(double), st));   // zero padding of k
        // (K + noise_K): the builder's diagonal epilogue with err = 0, diag_add = 0 adds exactly noise_var
        GPT_TRY(kbuild_terms(st, c->model, 1, mX, c->dn, Nx, mX, c->dn, Nx, 0, 0, 0, dzero, noise_var, 0.0, dK, NxP, mS, mS));
        GPT_TRY(gemm_nt(c, st, NyP, NxP, NxP, 1.0, c->dT, NxP, dK, NxP, 0.0, dTK, NxP, 0));          // T K  (K = K^T)
        GPT_TRY(gemm_nt(c, st, NyP, NyP, NxP, 1.0, dTK, NxP, c->dT, NxP, 0.0, c->dA, NP, 1));        // (T K) T^T, lower
        GPT_TRY(launch_add_diag(st, c->dA, NP, N, c->d_erry, diag_add));
        GPT_TRY(launch_fill_pad(st, c->dA, NP, N, NP, c->d_y, 1e300));
        c->have_kernel = true;
        return factor_and_ll(c, N, ll_data_out, logdet_half_out, true);
    }
    // The columns the first panel touches are built first so that its pivot chain overlaps the rest of the build.
    if (one_launch) {
        GPT_TRY(launch_upload_pad(st, c->h_yerr, c->d_y, NP + N, c->d_info, c->dA, NP, N, NP, 1e300));
        if (c->timing) GPT_HIP_CHECK(hipEventRecord(c->tev[1], st));
    } else {
        GPT_TRY(launch_fill_pad(st, c->dA, NP, N, NP, c->d_y, 1e300));
    }
    const int64_t w0 = (c->nb_early > outer_width(c, NP)) ? c->nb_early : outer_width(c, NP);
    int64_t head = round_up((c->ramp ? 128 : w0) + GPT_PANEL_EXT, 256);   // what panel 0 touches
    PotrfRequest req;                // (how panel 0 learns that the head is built: an event, or a flag word)
    hipEvent_t e_head = nullptr;
    const bool head_flag = c->flags_now && c->edge_seq < 0xf0000000u;
    if (c->lookahead && !c->use_graph && head < N && (head_flag || (e_head = get_event(c, 0)) != nullptr)) {
        GPT_TRY(kbuild_terms(st, c->model, 1, mX, c->dn, N, mX, c->dn, head, 1, 0, 0, c->d_erry, noise_var, diag_add,
                             c->dA, NP, mS, mS));
        if (head_flag) {
            // "the head columns are built" as a flag word raised from this stream (a one-thread kernel behind the build);
            // the first diagonal-block kernel of the panel stream polls it itself: no event record here, no event wait there
            req.head_wait = new_edge(c, 48);
            // (option "edge_test_stall", test aid: the flag is NOT raised, once -- the waiter must time out, the evaluation be
            // repeated on events and give the right numbers: tests/test_gpu_a_dist_processes.py.  An explicit option of the
            // context, not an environment variable: a stray variable must not be able to push a process off its flag edges)
            if (c->edge_test_stall) c->edge_test_stall = 0;
            else GPT_TRY(launch_set_flag(st, req.head_wait.word, req.head_wait.value));
        } else {
            GPT_HIP_CHECK(hipEventRecord(e_head, st));
        }
        GPT_TRY(kbuild_terms(st, c->model, 1, mX + head * c->D, c->dn + head * c->D, N - head, mX + head * c->D,
                             c->dn + head * c->D, N - head, 1, head, head, c->d_erry, noise_var, diag_add,
                             c->dA + head * NP + head, NP, mS ? mS + head : nullptr, mS ? mS + head : nullptr));
    } else {
        GPT_TRY(kbuild_terms(st, c->model, 1, mX, c->dn, N, mX, c->dn, N, 1, 0, 0, c->d_erry, noise_var, diag_add,
                             c->dA, NP, mS, mS));
    }
    c->have_kernel = true;
    req.head_event = e_head;
    return factor_and_ll(c, N, ll_data_out, logdet_half_out, true, req);
}

static int fit_matrix_once(gpt_ctx *c, const double *K_tot, int64_t N, const double *y, double *ll_data_out,
                           double *logdet_half_out);

extern "C" int gpt_fit_matrix(gpt_ctx *c, const double *K_tot, int64_t N, const double *y, double *ll_data_out,
                              double *logdet_half_out)
{
    CTX_ENTER(c);
    if (!K_tot || !y || N <= 0) return GPT_E_ARG;
    int rc;
    {
        EvalScope scope(c);
        rc = fit_matrix_once(c, K_tot, N, y, ll_data_out, logdet_half_out);
    }
    if (rc == GPT_I_EDGE_TIMEOUT) {
        edge_timeout_fallback(c);
        EvalScope scope(c);
        rc = fit_matrix_once(c, K_tot, N, y, ll_data_out, logdet_half_out);
    }
    return rc;
}

static int fit_matrix_once(gpt_ctx *c, const double *K_tot, int64_t N, const double *y, double *ll_data_out,
                           double *logdet_half_out)
{
    GPT_TRY(ensure_factor_storage(c, N));
    hipStream_t st = c->stream;
    c->factored = false;
    c->have_kernel = false;
    c->N = N;
    if (c->timing) {
        GPT_HIP_CHECK(hipEventRecord(c->tev[0], st));
        GPT_HIP_CHECK(hipEventRecord(c->tev[1], st));
    }
    GPT_HIP_CHECK(hipMemcpyAsync(c->d_y, y, (size_t)N * sizeof(double), hipMemcpyHostToDevice, st));
    GPT_HIP_CHECK(hipMemcpy2DAsync(c->dA, (size_t)c->NP * sizeof(double), K_tot, (size_t)N * sizeof(double),
                                   (size_t)N * sizeof(double), (size_t)N, hipMemcpyHostToDevice, st));
    return factor_and_ll(c, N, ll_data_out, logdet_half_out);
}
