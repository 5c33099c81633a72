// spectral.hpp -- the per-pair chain of ONE component of the spectral mixture kernel (Wilson & Adams, ICML 2013),
// GPT_KERNEL_SPECTRAL (include/gpt_hip.h):
//     k(x, x') = sigma_f^2 exp(-sum_d tau_d^2 / (2 l_d^2)) cos(2 pi sum_d mu_d tau_d),   tau = x - x'
// (one cosine of the dot product, not a product of cosines).  The functions are __host__ __device__ and need nothing of HIP, so
// that the ordinary host compiler can build them into a test aid (test_aids/spectral_host.cpp, tests/test_spectral_host.py); the
// device pair function is spectral_pair (kpair.hpp), which adds sigma_f^2 and the one exponential of a pair.
//
// k = sigma_f^2 Re prod_d f_d(tau_d),  f_d(tau) = exp(-a tau^2 / 2 + i w tau),  a = 1 / l_d^2,  w = 2 pi mu_d.  With
// s = -a tau + i w the n-th derivative of f_d is f_d H_n,
//     H_0 = 1,   H_1 = s,   H_(m+1) = s H_m - a m H_(m-1)
// (complex Hermite-like polynomials; two running complex values, no arrays), so a pair with derivative orders ni, nj is
//     sigma_f^2 (-1)^(sum nj) exp(-sum_d a_d tau_d^2 / 2) Re[ exp(2 pi i phi) prod_d H_(ni_d + nj_d) ],   phi = sum_d mu_d tau_d:
// one exponential and one sine / cosine per pair whatever the number of dimensions; the recurrence runs only in the dimensions
// that carry an order.
//
// Arithmetic.  The phase is kept in CYCLES and reduced before any sine is taken.  Each product mu_d tau_d is formed with its
// rounding error (one fma), reduced by its nearest integer -- exact -- and only then summed, so phi carries an absolute error of a
// few 1e-17 cycles however many cycles tau spans; the sum is reduced once more (|phi| <= 1/2) and sin / cos of pi phi come from
// gpt_per_sincospi (periodic.hpp), those of 2 pi phi from the double-angle forms 2 s c and 1 - 2 s^2, whose absolute error is
// a rounding of 1.  A masked-out dimension has a = 0 and w = 0: s = 0 exactly, so H_n = 0.0 exactly for n >= 1, and without an
// order it adds exactly 0.0 to the exponent and to the phase.
#pragma once
#include "periodic.hpp"

#define GPT_SPEC_MAXORD 16      // largest combined order ni_d + nj_d of ONE dimension (the host refuses more: api_kparams.inc)

// H_n(s) of one dimension, n >= 1, as (re, im); s = sr + i si, a = 1 / l^2
GPT_PER_HD inline void gpt_spec_H(double a, double sr, double si, int n, double *re, double *im)
{
    double pr = 1.0, pi = 0.0, hr = sr, hi = si;      // H_(m-1), H_m at m = 1
    for (int m = 1; m < n; m++) {
        const double am = a * (double)m;
        const double nr = __builtin_fma(-am, pr, __builtin_fma(sr, hr, -(si * hi)));
        const double nim = __builtin_fma(-am, pi, __builtin_fma(sr, hi, si * hr));
        pr = hr;
        pi = hi;
        hr = nr;
        hi = nim;
    }
    *re = hr;
    *im = hi;
}

// Everything of a pair but sigma_f^2 and the exponential: returns (-1)^(sum nj) Re[exp(2 pi i phi) prod_d H_(n_d)] and leaves the
// exponent's argument sum_d a_d tau_d^2 / 2 >= 0 in *E.  mu[d] in cycles per unit, a[d] = 1 / l_d^2.
template <int D>
GPT_PER_HD inline double gpt_spectral_chain(const double *mu, const double *a, const double *xi, const double *xj, const int *ni,
                                            const int *nj, double *E)
{
    double e = 0.0, phi = 0.0, qr = 1.0, qi = 0.0;
    int njs = 0;
    bool any = false;
#pragma unroll
    for (int d = 0; d < D; d++) {
        const double tau = xi[d] - xj[d];
        const double at = a[d] * tau;
        e = __builtin_fma(0.5 * at, tau, e);
        const double p = mu[d] * tau;
        const double perr = __builtin_fma(mu[d], tau, -p);      // mu tau = p + perr exactly
        phi += (p - __builtin_rint(p)) + perr;
        const int n = ni[d] + nj[d];
        if (n > 0) {
            double hr, hi;
            gpt_spec_H(a[d], -at, (2.0 * GPT_PER_PI) * mu[d], n, &hr, &hi);
            const double tr = __builtin_fma(qr, hr, -(qi * hi));
            qi = __builtin_fma(qr, hi, qi * hr);
            qr = tr;
            njs += nj[d];
            any = true;
        }
    }
    *E = e;
    phi -= __builtin_rint(phi);
    double s, c;
    gpt_per_sincospi(phi, &s, &c);
    const double c2 = __builtin_fma(-2.0 * s, s, 1.0), s2 = 2.0 * s * c;
    if (!any) return c2;
    const double v = __builtin_fma(c2, qr, -(s2 * qi));
    return (njs & 1) ? -v : v;
}
