// api_ensemble.inc -- part of api.hip (ONE translation unit: included from there).  gpt_ensemble_run: the whole loop of an
// affine-invariant ensemble sampler over the free hyperparameters of the resident data set's model, inside the library.
// ------------------------------------------------------------------------------------------------
// One ensemble step is two dependent batches of nwalkers / 2 independent log-posterior evaluations -- the batched fit's shape
// (fit_batch_impl, api_batch.inc: 1.4 us an evaluation at N = 256).  Driven from Python, every one of those evaluations first costs
// the host 40 us to milliseconds of per-walker preparation (kernel objects, hyperprior, job tuples); here nothing runs between two
// launch sequences but the stepping arithmetic (ensemble.hpp, host only and shared with the CPU test aid), a box test, a scatter
// into the model's parameter vector and parse_model.  No kernel of its own: the device work IS fit_batch_impl's launch sequence.
#include "ensemble.hpp"

extern "C" int gpt_ensemble_run(gpt_ctx *c, int nterms, const int *kernel_ids, const int *kernel_ids2, const int *nparams_t,
                                const int *nparams1_t, const double *base_params, int nfree, const int32_t *free_idx, const double *lo,
                                const double *hi, double log_prior, const double *y, const double *err_y, double diag_add,
                                double noise_var, int nwalkers, int nsteps, double a, const double *u_stretch, const int32_t *partner,
                                const double *u_accept, int max_chunk, double *pos, double *lnp, double *chain, double *lnp_chain,
                                int32_t *naccept)
{
    CTX_ENTER(c);
    if (!c->dX) {
        gpt_set_error("gpt_ensemble_run: call gpt_set_data first");
        return GPT_E_STATE;
    }
    if (nterms < 1 || nterms > GPT_MAX_TERMS || !kernel_ids || !nparams_t || (kernel_ids2 && !nparams1_t) || !base_params || !free_idx ||
        !y || !err_y || max_chunk < 1) {
        gpt_set_error("gpt_ensemble_run: bad arguments");
        return GPT_E_ARG;
    }
    int ptot = 0;
    for (int t = 0; t < nterms; t++) {
        if (nparams_t[t] < 1) return GPT_E_ARG;
        ptot += nparams_t[t];
    }
    int noise_at = -1;                                       // the free parameter that is the noise sigma, if one is
    for (int f = 0; f < nfree; f++) {
        if (free_idx[f] < 0 || free_idx[f] > ptot || (free_idx[f] == ptot && noise_at >= 0)) {
            gpt_set_error("gpt_ensemble_run: free parameter %d has index %d, the model has %d parameters (+ the noise)", f, free_idx[f], ptot);
            return GPT_E_ARG;
        }
        if (free_idx[f] == ptot) noise_at = f;
    }
    EnsembleRun r;
    r.nwalkers = nwalkers;
    r.nfree = nfree;
    r.nsteps = nsteps;
    r.a = a;
    r.lo = lo;
    r.hi = hi;
    r.u_stretch = u_stretch;
    r.partner = partner;
    r.u_accept = u_accept;
    r.pos = pos;
    r.lnp = lnp;
    r.chain = chain;
    r.lnp_chain = lnp_chain;
    r.naccept = naccept;
    if (ensemble_check(r) != 0) {
        gpt_set_error("gpt_ensemble_run: needs an even nwalkers >= 2, nfree >= 1, a > 1, every array, and partners inside their half");
        return GPT_E_ARG;
    }
    const int64_t N = c->dT ? c->Ny : c->Nx;                 // the targets of one element
    const int h = nwalkers / 2;
    std::vector<double> params((size_t)h * ptot), nv(h), ys((size_t)h * N), ll(h);
    std::vector<int32_t> info(h);
    std::vector<int> where(h);
    for (int k = 0; k < h; k++) memcpy(&ys[(size_t)k * N], y, (size_t)N * sizeof(double));      // (no mean function: every element's targets)
    // sigma^2 as GaussianProcess._noise_var forms it: through pow, which an optimiser would otherwise replace by sigma * sigma (the
    // two agree unless the library's pow misrounds -- the host route's bits are the contract)
    static volatile double two = 2.0;
    int chunk_max = max_chunk;
    ModelKernel mk;
    auto eval = [&](int count, const double *q, double *out) -> int {
        int n = 0;
        for (int k = 0; k < count; k++) {
            double *pk = &params[(size_t)n * ptot];
            memcpy(pk, base_params, (size_t)ptot * sizeof(double));
            for (int f = 0; f < nfree; f++)
                if (f != noise_at) pk[free_idx[f]] = q[(size_t)k * nfree + f];
            out[k] = -INFINITY;
            // (a parameter outside its kernel's domain: this proposal is impossible, as ll_batch's rejected chunk ends for it)
            if (parse_model(c->D, c->n_maxsum, c->n_colmax, nterms, kernel_ids, kernel_ids2, pk, nparams_t, nparams1_t, &mk) != GPT_OK) continue;
            nv[n] = noise_at >= 0 ? pow(q[(size_t)k * nfree + noise_at], two) : noise_var;
            where[n++] = k;
        }
        for (int s0 = 0; s0 < n;) {
            const int m = n - s0 < chunk_max ? n - s0 : chunk_max;
            const int rc = fit_batch_impl(c, m, nterms, kernel_ids, kernel_ids2, &params[(size_t)s0 * ptot], nparams_t, nparams1_t, &nv[s0],
                                          ys.data(), err_y, diag_add, &ll[s0], nullptr, &info[s0]);
            if (rc == GPT_E_NOMEM && m > 1) {                // (as _fit_batched: the scratch back, half as many elements)
                GPT_TRY(gpt_release_batch_scratch(c));
                chunk_max = m / 2;
                continue;
            }
            if (rc != GPT_OK) return rc;
            s0 += m;
        }
        for (int k = 0; k < n; k++)
            if (info[k] == 0 && ll[k] == ll[k]) out[where[k]] = ll[k] + log_prior;
        return 0;
    };
    const int rc = ensemble_run(r, eval);
    if (rc == GPT_OK) gpt_set_error("%s", "");               // (refusals of single proposals are no error of the run)
    return rc;
}
