// ensemble.hpp -- host only (no HIP): the stepping arithmetic of the affine-invariant ensemble sampler (Goodman & Weare's stretch
// move), a function template over the evaluator.  api_ensemble.inc instantiates it with the batched fit (gpt_ensemble_run),
// test_aids/ensemble_host.cpp with a callback, built by the host compiler: tests/test_sampler_host.py compares that loop with the
// Python loop of gptools_amd/sampler.py, which this file restates operation by operation -- every sum, product and comparison in
// the same order on the same doubles, so that both produce the same chain bit for bit from the same variates:
//   one step handles the halves (first, second), then (second, first); for walker w of the half S against the other half C
//     t = (a - 1) u_stretch[w] + 1,  z = t t / a,  q = C[j] - z (C[j] - S[w])  with j = partner[w],
//     accept where (nfree - 1) log z + lnp(q) - lnp(S[w]) > log u_accept[w];
//   a proposal outside the box [lo, hi] (both ends inside, as UniformJointPrior.__call__: lo <= v <= hi; a NaN is outside) has
//   lnp = -inf and never reaches the evaluator; a NaN from the evaluator counts as -inf.
// All proposals of a half are formed from the positions as the half found them.  (Build with -ffp-contract=off.)
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>

struct EnsembleRun {
    int nwalkers = 0, nfree = 0, nsteps = 0;
    double a = 2.0;
    const double *lo = nullptr, *hi = nullptr;               // the box, nfree each
    const double *u_stretch = nullptr, *u_accept = nullptr;  // (nsteps, nwalkers) uniform variates, indexed by walker
    const int32_t *partner = nullptr;                        // (nsteps, nwalkers): index INTO the complementary half
    double *pos = nullptr, *lnp = nullptr;                   // (nwalkers, nfree), (nwalkers): in and out
    double *chain = nullptr, *lnp_chain = nullptr;           // (nsteps, nwalkers, nfree), (nsteps, nwalkers)
    int32_t *naccept = nullptr;                              // (nwalkers): accepted moves of this run
};

// 0: the arguments are usable; else -1 (a null array, an odd or too small ensemble, a partner outside its half)
static inline int ensemble_check(const EnsembleRun &r)
{
    if (r.nwalkers < 2 || r.nwalkers % 2 || r.nfree < 1 || r.nsteps < 0 || !(r.a > 1.0) || !r.lo || !r.hi || !r.u_stretch || !r.u_accept ||
        !r.partner || !r.pos || !r.lnp || !r.chain || !r.lnp_chain || !r.naccept)
        return -1;
    const int64_t n = (int64_t)r.nsteps * r.nwalkers, h = r.nwalkers / 2;
    for (int64_t i = 0; i < n; i++)
        if (r.partner[i] < 0 || r.partner[i] >= h) return -1;
    return 0;
}

// eval(count, q, out): the log-probabilities out[0 .. count) of the count >= 1 proposals q (count x nfree, all inside the box);
// returns 0, or a status that ends the run and is returned (pos / lnp then hold the state after the last completed half).
template <class Eval>
static int ensemble_run(const EnsembleRun &r, Eval &&eval)
{
    if (ensemble_check(r) != 0) return -1;
    const int K = r.nwalkers, h = K / 2, p = r.nfree;
    const double a = r.a, ninf = -INFINITY;
    std::vector<double> q((size_t)h * p), qin((size_t)h * p), lq(h), lin(h), logz(h);
    std::vector<int> where(h);
    for (int w = 0; w < K; w++) r.naccept[w] = 0;
    for (int s = 0; s < r.nsteps; s++) {
        const double *us = r.u_stretch + (size_t)s * K, *ua = r.u_accept + (size_t)s * K;
        const int32_t *pj = r.partner + (size_t)s * K;
        for (int half = 0; half < 2; half++) {
            const int s0 = half ? h : 0, c0 = half ? 0 : h;
            int nin = 0;
            for (int i = 0; i < h; i++) {
                const int w = s0 + i;
                const double t = (a - 1.0) * us[w] + 1.0, z = t * t / a;
                logz[i] = log(z);
                const double *cj = r.pos + (size_t)(c0 + pj[w]) * p, *sw = r.pos + (size_t)w * p;
                bool inside = true;
                for (int d = 0; d < p; d++) {
                    const double v = cj[d] - z * (cj[d] - sw[d]);
                    q[(size_t)i * p + d] = v;
                    if (!(r.lo[d] <= v && v <= r.hi[d])) inside = false;
                }
                lq[i] = ninf;
                if (inside) {
                    memcpy(&qin[(size_t)nin * p], &q[(size_t)i * p], (size_t)p * sizeof(double));
                    where[nin++] = i;
                }
            }
            if (nin > 0) {
                const int rc = eval(nin, (const double *)qin.data(), lin.data());
                if (rc != 0) return rc;
                for (int k = 0; k < nin; k++) lq[where[k]] = lin[k] == lin[k] ? lin[k] : ninf;
            }
            for (int i = 0; i < h; i++) {
                const int w = s0 + i;
                const double diff = (double)(p - 1) * logz[i] + lq[i] - r.lnp[w];
                if (diff > log(ua[w])) {                     // (a NaN difference, -inf against -inf, is no acceptance)
                    memcpy(r.pos + (size_t)w * p, &q[(size_t)i * p], (size_t)p * sizeof(double));
                    r.lnp[w] = lq[i];
                    r.naccept[w]++;
                }
            }
        }
        memcpy(r.chain + (size_t)s * K * p, r.pos, (size_t)K * p * sizeof(double));
        memcpy(r.lnp_chain + (size_t)s * K, r.lnp, (size_t)K * sizeof(double));
    }
    return 0;
}
