// warp.hpp -- input warps of the native kernels (gpt_set_warp, include/gpt_hip.h; ref: gptools/kernel/warping.py:315-402):
// per dimension d a chain of layers  x -> w_0(x) -> w_1(w_0(x)) ...  with the chain-rule slope  prod_l w_l'(input of layer l).
//   GPT_WARP_LINEAR  w = (x - a)/(b - a),  w' = 1/(b - a)
//   GPT_WARP_BETA    w = I_x(alpha, beta) (regularised incomplete beta function),  w' = x^(alpha-1) (1-x)^(beta-1) / B(alpha, beta)
// The functions are __host__ __device__ and need nothing of HIP, so that the ordinary host compiler can build them into a test
// aid (test_aids/warp_host.cpp) and a CPU-only test can compare them with scipy.special.betainc.
#pragma once
#include <math.h>
#include "../../include/gpt_hip.h"

#ifdef __HIPCC__
#define GPT_HD __host__ __device__
#else
#define GPT_HD
#endif

struct WarpLayers {
    int nlayers;                                       // 0: no warp
    int D;
    int type[GPT_WARP_MAX_LAYERS];
    double p[GPT_WARP_MAX_LAYERS][2 * GPT_MAX_DIM];    // layer l, dimension d: p[l][2 d], p[l][2 d + 1]
};

// Stirling's correction  lgamma(z) - [(z - 1/2) log z - z + log(2 pi)/2]  for z >= 10 (the first neglected term is 3e-17 there)
GPT_HD static inline double gpt_lgamma_corr(double z)
{
    const double r = 1.0 / z, r2 = r * r;
    return r * (1.0 / 12.0 + r2 * (-1.0 / 360.0 + r2 * (1.0 / 1260.0 + r2 * (-1.0 / 1680.0 + r2 * (1.0 / 1188.0 +
           r2 * (-691.0 / 360360.0 + r2 * (1.0 / 156.0)))))));
}

// log B(a, b).  With an argument of 10 or more the difference lgamma(p) - lgamma(p + q) would cancel most of two large numbers
// (an error of |lgamma(p)| ulp, which the reflection of gpt_betainc multiplies again): there the large terms are combined
// analytically through Stirling's formula, as R's lbeta does.
GPT_HD static inline double gpt_lbeta(double a, double b)
{
    const double p = a > b ? a : b, q = a > b ? b : a;          // p >= q
    if (p < 10.0) return (lgamma(a) + lgamma(b)) - lgamma(a + b);
    const double corr = gpt_lgamma_corr(p) - gpt_lgamma_corr(p + q);
    if (q < 10.0) return lgamma(q) + (corr - ((p - 0.5) * log1p(q / p) + q * (log(p + q) - 1.0)));
    return ((-0.5 * log(q) + 0.91893853320467274178) + (corr + gpt_lgamma_corr(q))) +
           ((p - 0.5) * log(p / (p + q)) + q * log(q / (p + q)));
}

// Continued fraction of the incomplete beta function (Numerical Recipes' betacf), evaluated by the modified Lentz method;
// converges in O(sqrt(max(a, b))) steps for x < (a + 1)/(a + b + 2).
GPT_HD static inline double gpt_betacf(double a, double b, double x)
{
    const double tiny = 1e-300, eps = 1.2e-16;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 1000; m++) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) <= eps) break;
    }
    return h;
}

// I_x(a, b): exactly 0 / 1 at x = 0 / 1, NaN outside [0, 1] and for a <= 0 or b <= 0 (and for NaN arguments).
GPT_HD static inline double gpt_betainc(double a, double b, double x)
{
    if (!(a > 0.0) || !(b > 0.0) || !(x >= 0.0) || !(x <= 1.0)) return NAN;
    if (x == 0.0) return 0.0;
    if (x == 1.0) return 1.0;
    // prefactor x^a (1-x)^b / B(a, b) by pow (below an ulp whatever the exponent; exp(a log x + ...) would lose |a log x| ulp),
    // as the square of the half powers so that a product near the denormals keeps its bits until 1/B has been applied
    const double hp = pow(x, 0.5 * a) * pow(1.0 - x, 0.5 * b);
    const double bt = (hp * exp(-gpt_lbeta(a, b))) * hp;
    if (x > (a + 1.0) / (a + b + 2.0)) return 1.0 - bt * gpt_betacf(b, a, 1.0 - x) / b;      // reflection I_x(a,b) = 1 - I_{1-x}(b,a)
    return bt * gpt_betacf(a, b, x) / a;
}

// d/dx I_x(a, b); NaN where the value is NaN
GPT_HD static inline double gpt_betainc_slope(double a, double b, double x)
{
    if (!(a > 0.0) || !(b > 0.0) || !(x >= 0.0) || !(x <= 1.0)) return NAN;
    return pow(x, a - 1.0) * pow(1.0 - x, b - 1.0) / exp(gpt_lbeta(a, b));
}

// one coordinate of dimension d through all layers: returns the warped coordinate, *slope = product of the layers' slopes.
// Layer l's parameters at p + l * stride (the context's WarpLayers, or one element's row of a batch in device memory): one
// function for both, so that an element of a batch carries the bits of the single warp.
GPT_HD static inline double gpt_warp_chain(int nlayers, const int *type, const double *p, int stride, int d, double x, double *slope)
{
    double s = 1.0;
    for (int l = 0; l < nlayers; l++) {
        const double p0 = p[l * stride + 2 * d], p1 = p[l * stride + 2 * d + 1];
        if (type[l] == GPT_WARP_LINEAR) {
            s *= 1.0 / (p1 - p0);
            x = (x - p0) / (p1 - p0);
        } else {
            s *= gpt_betainc_slope(p0, p1, x);
            x = gpt_betainc(p0, p1, x);
        }
    }
    *slope = s;
    return x;
}

GPT_HD static inline double gpt_warp_coord(const WarpLayers &wl, int d, double x, double *slope)
{
    return gpt_warp_chain(wl.nlayers, wl.type, &wl.p[0][0], 2 * GPT_MAX_DIM, d, x, slope);
}

#ifdef __HIPCC__
// Xw (N x D) = the warped points, S (N) = per point the product of the slopes over the dimensions where its order is 1 (exactly
// 1.0 for a value point).  Xw == X is allowed (in place).  Asynchronous on `st`.
int launch_warp_points(hipStream_t st, const WarpLayers &wl, const double *dX, const int32_t *dn, int64_t N, double *dXw,
                       double *dS);
// The same for a batch in ONE launch: element b's layers have the parameters d_params + b * nlayers * 2 D (device memory, layer-major;
// types and D from `wl`), its warped points go to dXw + b * N * D, its slope factors to dS + b * N.
int launch_warp_points_batch(hipStream_t st, const WarpLayers &wl, const double *d_params, int64_t nbatch, const double *dX,
                             const int32_t *dn, int64_t N, double *dXw, double *dS);
// v[a] *= S[a]^2: the diagonal of a warped K(X*, X*) from the inner kernel's
int launch_warp_scale_diag(hipStream_t st, double *dv, const double *dS, int64_t M);
#endif
