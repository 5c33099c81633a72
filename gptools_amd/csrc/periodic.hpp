// periodic.hpp -- the per-dimension chain of the periodic (exp-sine-squared) kernel, GPT_KERNEL_PERIODIC (include/gpt_hip.h):
//     k(x, x') = sigma_f^2 prod_d f_d(tau_d),   f_d(tau) = exp(-2 sin^2(pi tau / p_d) / l_d^2),   tau = x - x'.
// The functions are __host__ __device__ and need nothing of HIP, so that the ordinary host compiler can build them into a test
// aid (test_aids/periodic_host.cpp, tests/test_periodic_host.py); the device pair function is periodic_pair (kpair.hpp), which
// adds sigma_f^2 and the one exponential of a pair.
//
// With a = 1 / l^2 and w = 2 pi / p:  f = exp(g - a),  g(tau) = a cos(w tau),  so  f^(m) = f P_m  with
//     P_0 = 1,   P_(m+1) = sum_(k = 0 .. m) C(m, k) g^(k+1) P_(m-k),   g^(k) = a w^k cos(w tau + k pi / 2)
// (the derivatives of g cycle through cos, -sin, -cos, sin).  A pair with derivative orders ni, nj is
//     sigma_f^2 exp(-sum_d 2 a_d sin^2(pi t_d)) prod_d (-1)^(nj_d) P_(n_d),   n_d = ni_d + nj_d,
// one exponential whatever the number of dimensions; the recurrence runs only in the dimensions that carry an order.
//
// Arithmetic.  The argument is reduced in units of the PERIOD: t = tau (1 / p), t -= rint(t), so |t| <= 1/2 and the kernel is
// periodic to rounding (exactly, where tau / p is formed exactly); sin(pi t) and cos(pi t) come from polynomials on
// [0, pi / 4] (|t| > 1/4: the complementary angle 1/2 - |t|, which is exact).  The VALUE uses sin^2 -- cos - 1 would cancel near
// tau = 0 -- and the derivatives of g use cos(w tau) = 1 - 2 sin^2(pi t), sin(w tau) = 2 sin(pi t) cos(pi t), whose absolute
// error is a rounding of 1.  A masked-out dimension has a = 0 (l = +inf): its term of the exponent is exactly 0.0, its g^(k) and
// with them every P_n, n >= 1, exactly 0.0.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define GPT_PER_HD __host__ __device__
#define GPT_PER_NOINLINE __attribute__((noinline))
#else
#define GPT_PER_HD
#define GPT_PER_NOINLINE
#endif

#define GPT_PER_MAXORD 16      // largest combined order ni_d + nj_d of ONE dimension (the host refuses more: api_kparams.inc)
#define GPT_PER_PI 3.14159265358979323846

// sin(pi t), cos(pi t) for |t| <= 1/2 (what t - rint(t) leaves).  q = |t| or 1/2 - |t| in [0, 1/4], x = pi q in [0, pi / 4];
// the two polynomials are the minimax ones of the freely distributable fdlibm's k_sin.c / k_cos.c (error below 2^-58 there).
GPT_PER_HD inline void gpt_per_sincospi(double t, double *s, double *c)
{
    const double r = fabs(t);
    const bool swap = r > 0.25;
    const double x = GPT_PER_PI * (swap ? 0.5 - r : r);
    const double z = x * x;
    double ps = 1.58969099521155010221e-10;
    ps = __builtin_fma(ps, z, -2.50507602534068634195e-08);
    ps = __builtin_fma(ps, z, 2.75573137070700676789e-06);
    ps = __builtin_fma(ps, z, -1.98412698298579493134e-04);
    ps = __builtin_fma(ps, z, 8.33333333332248946124e-03);
    ps = __builtin_fma(ps, z, -1.66666666666666324348e-01);
    const double sx = __builtin_fma(x * z, ps, x);
    double pc = -1.13596475577881948265e-11;
    pc = __builtin_fma(pc, z, 2.08757232129817482790e-09);
    pc = __builtin_fma(pc, z, -2.75573143513906633035e-07);
    pc = __builtin_fma(pc, z, 2.48015872894767294178e-05);
    pc = __builtin_fma(pc, z, -1.38888888888741095749e-03);
    pc = __builtin_fma(pc, z, 4.16666666666666019037e-02);
    const double cx = __builtin_fma(z * z, pc, __builtin_fma(-0.5, z, 1.0));
    const double sa = swap ? cx : sx;
    *s = (t < 0.0) ? -sa : sa;
    *c = swap ? sx : cx;
}

// P_n, 3 <= n <= GPT_PER_MAXORD, by the recurrence; sn = sin(w tau), cs = cos(w tau).  row[] is line m of Pascal's triangle,
// moved on in place.  Out of line on the device: the arrays are indexed at run time and live in scratch, which only the pairs
// with such an order should pay for (orders 1 and 2 are closed forms in gpt_per_P).
GPT_PER_HD GPT_PER_NOINLINE inline double gpt_per_P_general(double a, double w, double sn, double cs, int n)
{
    if (n > GPT_PER_MAXORD) return (double)NAN;
    double G[GPT_PER_MAXORD + 1], P[GPT_PER_MAXORD + 1], row[GPT_PER_MAXORD + 1];
    double wp = a;
    for (int k = 1; k <= n; k++) {
        wp *= w;
        const int r = k & 3;
        G[k] = wp * ((r == 0) ? cs : (r == 1) ? -sn : (r == 2) ? -cs : sn);
    }
    P[0] = 1.0;
    row[0] = 1.0;
    for (int m = 0; m < n; m++) {
        double acc = 0.0;
        for (int k = 0; k <= m; k++) acc = __builtin_fma(row[k] * G[k + 1], P[m - k], acc);
        P[m + 1] = acc;
        row[m + 1] = 1.0;
        for (int k = m; k >= 1; k--) row[k] += row[k - 1];
    }
    return P[n];
}

// P_n of one dimension, n >= 1
GPT_PER_HD inline double gpt_per_P(double a, double w, double sn, double cs, int n)
{
    const double g1 = (a * w) * -sn;
    if (n == 1) return g1;
    if (n == 2) return __builtin_fma(g1, g1, ((a * w) * w) * -cs);
    return gpt_per_P_general(a, w, sn, cs, n);
}

// Everything of a pair but sigma_f^2 and the exponential: returns prod_d (-1)^(nj_d) P_(n_d) (exactly 1.0 for a value pair) and
// leaves the exponent's argument sum_d 2 a_d sin^2(pi t_d) >= 0 in *E.  inv_p[d] = 1 / p_d, a[d] = 1 / l_d^2.
template <int D>
GPT_PER_HD inline double gpt_periodic_chain(const double *inv_p, const double *a, const double *xi, const double *xj, const int *ni,
                                            const int *nj, double *E)
{
    double e = 0.0, prod = 1.0;
    int njs = 0;
#pragma unroll
    for (int d = 0; d < D; d++) {
        double t = (xi[d] - xj[d]) * inv_p[d];
        t -= __builtin_rint(t);
        double s, c;
        gpt_per_sincospi(t, &s, &c);
        e = __builtin_fma(2.0 * a[d], s * s, e);
        const int n = ni[d] + nj[d];
        if (n > 0) {
            prod *= gpt_per_P(a[d], (2.0 * GPT_PER_PI) * inv_p[d], 2.0 * s * c, __builtin_fma(-2.0 * s, s, 1.0), n);
            njs += nj[d];
        }
    }
    *E = e;
    return (njs & 1) ? -prod : prod;
}
