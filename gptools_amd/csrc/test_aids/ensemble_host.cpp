// ensemble_host.cpp -- test aid (not part of the product library): the ensemble loop of ensemble.hpp (what gpt_ensemble_run steps
// with) compiled by the host compiler with a callback as the evaluator, so that tests/test_sampler_host.py can compare it with
// the Python loop of gptools_amd/sampler.py on a CPU.  With -DENSEMBLE_HOST_MAIN: a stand-alone program that runs the loop (for
// the address / undefined-behaviour sanitizers; exit status 0 when its own checks hold).
#include "../ensemble.hpp"

typedef int (*gpt_host_lnprob_fn)(int count, const double *q, double *out);

extern "C" int gpt_host_ensemble_run(int nwalkers, int nfree, int nsteps, double a, const double *lo, const double *hi,
                                     const double *u_stretch, const int32_t *partner, const double *u_accept, double *pos, double *lnp,
                                     double *chain, double *lnp_chain, int32_t *naccept, gpt_host_lnprob_fn fn)
{
    if (!fn) return -1;
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
    return ensemble_run(r, [&](int count, const double *q, double *out) { return fn(count, q, out); });
}

#ifdef ENSEMBLE_HOST_MAIN
#include <stdio.h>

// a unit Gaussian centred on the box's edge, refused (-inf, as a proposal parse_model rejects) in a strip inside the box
static int n_eval = 0, n_refused = 0;
static int target(int count, const double *q, double *out)
{
    for (int k = 0; k < count; k++) {
        const double x = q[2 * k], y = q[2 * k + 1];
        n_eval++;
        if (x > 0.4 && x < 0.6) {
            out[k] = -INFINITY;
            n_refused++;
        } else
            out[k] = -0.5 * (x * x + y * y);
    }
    return 0;
}

int main()
{
    const int K = 16, p = 2, S = 50;
    std::vector<double> us((size_t)S * K), ua((size_t)S * K), pos((size_t)K * p), lnp(K), chain((size_t)S * K * p), lc((size_t)S * K);
    std::vector<int32_t> pj((size_t)S * K), nacc(K);
    uint64_t state = 88172645463325252ull;
    auto uni = [&]() {
        state ^= state << 13;
        state ^= state >> 7;
        state ^= state << 17;
        return (double)(state >> 11) / 9007199254740992.0;
    };
    for (size_t i = 0; i < us.size(); i++) {
        us[i] = uni();
        ua[i] = uni();
        pj[i] = (int32_t)(uni() * (K / 2));
    }
    const double lo[2] = {0.0, -3.0}, hi[2] = {3.0, 3.0};
    for (int w = 0; w < K; w++) {
        pos[2 * w] = 0.05 + 2.9 * uni();
        pos[2 * w + 1] = -2.9 + 5.8 * uni();
    }
    target(K, pos.data(), lnp.data());
    n_eval = n_refused = 0;
    const int rc = gpt_host_ensemble_run(K, p, S, 2.0, lo, hi, us.data(), pj.data(), ua.data(), pos.data(), lnp.data(), chain.data(),
                                         lc.data(), nacc.data(), target);
    int total = 0, outside = 2 * S * (K / 2) - n_eval, bad = 0;
    for (int w = 0; w < K; w++) total += nacc[w];
    for (size_t i = 0; i < chain.size(); i += 2)
        if (!(chain[i] >= lo[0] && chain[i] <= hi[0] && chain[i + 1] >= lo[1] && chain[i + 1] <= hi[1])) bad++;
    printf("rc %d: %d proposals evaluated, %d outside the box, %d refused, %d accepted, %d stored positions outside the box\n", rc, n_eval,
           outside, n_refused, total, bad);
    pj[3] = K / 2;                                           // a partner outside its half: refused, nothing is read
    const int rc2 = gpt_host_ensemble_run(K, p, S, 2.0, lo, hi, us.data(), pj.data(), ua.data(), pos.data(), lnp.data(), chain.data(),
                                          lc.data(), nacc.data(), target);
    return (rc == 0 && rc2 == -1 && outside > 0 && n_refused > 0 && total > 0 && bad == 0) ? 0 : 1;
}
#endif
