// gibbs_lfunc.hpp -- the closed-form length-scale functions l(x), l'(x) of the bucket, exp-Gauss, B-spline and nested-GP Gibbs kernels
// (GPT_KERNEL_GIBBS_CUBIC / _QUINTIC / _EXPGAUSS / _BSPLINE / _GP, include/gpt_hip.h; ref: gptools/kernel/gibbs.py:603-651, :695-760,
// :804-855, :905-992, :995-1095),
// from the raw parameters after sigma_f.  The functions are __host__ __device__ and need nothing of HIP, so that the ordinary
// host compiler can build them into a test aid (test_aids/gibbs_host.cpp) and a CPU-only test can compare them with the numpy
// functions of gptools_amd/kernel/gibbs.py.  kpair.hpp (gibbs_point) calls them once per point, never per pair.
//
// The buckets are the reference's arithmetic LITERALLY: the section ends in its order of operations, every section value
// formed everywhere and multiplied by its 0/1 mask, the products summed left to right.  The reference is DEFINED by that sum: a
// point exactly at a section end belongs to exactly one mask; a non-finite section polynomial times a zero mask is NaN (w_1 = 0:
// NaN everywhere; a width so small that the quintic's fifth power overflows: NaN outside that section); negative widths make
// the masks overlap or leave gaps.  A branch that picked one section would give other numbers in each of these cases.  Integer
// powers are repeated multiplication (within 2 ulp of the reference's pow, and not the ~100 instructions of a device pow).
#pragma once
#include <math.h>
#include "../../include/gpt_hip.h"

#ifndef GPT_HD
#ifdef __HIPCC__
#define GPT_HD __host__ __device__
#else
#define GPT_HD
#endif
#endif

// the five 0/1 masks of a bucket with section ends e0 < e1 <= e2 < e3 (for positive widths), gibbs.py:633-639
struct GibbsBucketMasks {
    double left, join1, mid, join2, right;
};

GPT_HD static inline GibbsBucketMasks gpt_gibbs_bucket_masks(double x, double x1, double x2, double w1, double w3)
{
    GibbsBucketMasks m;
    m.left = (x <= (x1 - w1 / 2.0)) ? 1.0 : 0.0;
    m.join1 = ((x > (x1 - w1 / 2.0)) && (x < (x1 + w1 / 2.0))) ? 1.0 : 0.0;
    m.mid = ((x >= (x1 + w1 / 2.0)) && (x <= x2 - w3 / 2.0)) ? 1.0 : 0.0;
    m.join2 = ((x > (x2 - w3 / 2.0)) && (x < (x2 + w3 / 2.0))) ? 1.0 : 0.0;
    m.right = (x >= (x2 + w3 / 2.0)) ? 1.0 : 0.0;
    return m;
}

// p = [l_1, l_2, l_3, x_0, w_1, w_2, w_3]
GPT_HD static inline void gpt_gibbs_cubic_bucket(const double *p, double x, double *l, double *dl)
{
    const double l1 = p[0], l2 = p[1], l3 = p[2], x0 = p[3], w1 = p[4], w2 = p[5], w3 = p[6];
    const double x1 = x0 - w2 / 2.0 - w1 / 2.0;
    const double x2 = x0 + w2 / 2.0 + w3 / 2.0;
    const double s1 = (x - x1 + w1 / 2.0) / w1;
    const double s2 = (x - x2 + w3 / 2.0) / w3;
    const GibbsBucketMasks m = gpt_gibbs_bucket_masks(x, x1, x2, w1, w3);
    const double s1q = s1 * s1, s2q = s2 * s2;
    *l = l1 * m.left + (-2.0 * (l2 - l1) * (s1q * s1 - 3.0 / 2.0 * s1q) + l1) * m.join1 + l2 * m.mid +
         (-2.0 * (l3 - l2) * (s2q * s2 - 3.0 / 2.0 * s2q) + l2) * m.join2 + l3 * m.right;
    *dl = (-2.0 * (l2 - l1) * (3.0 * s1q - 3.0 * s1) / w1) * m.join1 + (-2.0 * (l3 - l2) * (3.0 * s2q - 3.0 * s2) / w3) * m.join2;
}

// p as for the cubic bucket
GPT_HD static inline void gpt_gibbs_quintic_bucket(const double *p, double x, double *l, double *dl)
{
    const double l1 = p[0], l2 = p[1], l3 = p[2], x0 = p[3], w1 = p[4], w2 = p[5], w3 = p[6];
    const double x1 = x0 - w2 / 2.0 - w1 / 2.0;
    const double x2 = x0 + w2 / 2.0 + w3 / 2.0;
    const double s1 = 2.0 * (x - x1) / w1;
    const double s3 = 2.0 * (x - x2) / w3;
    const GibbsBucketMasks m = gpt_gibbs_bucket_masks(x, x1, x2, w1, w3);
    const double s1q = s1 * s1, s1c = s1q * s1, s1f = s1q * s1q, s1v = s1f * s1;
    const double s3q = s3 * s3, s3c = s3q * s3, s3f = s3q * s3q, s3v = s3f * s3;
    *l = l1 * m.left + (0.5 * (l2 - l1) * (3.0 / 8.0 * s1v - 5.0 / 4.0 * s1c + 15.0 / 8.0 * s1) + (l1 + l2) / 2.0) * m.join1 +
         l2 * m.mid + (0.5 * (l3 - l2) * (3.0 / 8.0 * s3v - 5.0 / 4.0 * s3c + 15.0 / 8.0 * s3) + (l2 + l3) / 2.0) * m.join2 +
         l3 * m.right;
    *dl = (0.5 * (l2 - l1) * (5.0 * 3.0 / 8.0 * s1f - 3.0 * 5.0 / 4.0 * s1q + 15.0 / 8.0) / w1) * m.join1 +
          (0.5 * (l3 - l2) * (5.0 * 3.0 / 8.0 * s3f - 3.0 * 5.0 / 4.0 * s3q + 15.0 / 8.0) / w3) * m.join2;
}

// p = [l_0, mu_1 .. mu_G, sigma_1 .. sigma_G, beta_1 .. beta_G]:  S1 = sum_i beta_i exp(-(x - mu_i)^2 / (2 sigma_i^2)),
// S2 = sum_i beta_i exp(..) (x - mu_i) / sigma_i^2 in the reference's loop order;  l = l_0 exp(S1),  l' = -l_0 exp(S1) S2
GPT_HD static inline void gpt_gibbs_exp_gauss(const double *p, int G, double x, double *l, double *dl)
{
    const double l0 = p[0];
    double S1 = 0.0, S2 = 0.0;
    for (int i = 0; i < G; i++) {
        const double d = x - p[1 + i], s = p[1 + G + i], b = p[1 + 2 * G + i];
        const double term = b * exp(-(d * d) / (2.0 * (s * s)));
        S1 += term;
        S2 += term * d / (s * s);
    }
    const double e = exp(S1);
    *l = l0 * e;
    *dl = -l0 * e * S2;
}

// B-spline length scale (GPT_KERNEL_GIBBS_BSPLINE; ref: gptools/kernel/gibbs.py:905-992 through gptools/splines.py:5-146; the
// numpy statement is gptools_amd/splines.py).  p = [t_1 .. t_nt, C_1 .. C_{nt+2}], cubic, knots in increasing order (the parser
// refuses anything else), 2 <= nt <= GPT_GIBBS_MAX_KNOTS.  l = sum_i C_i B_{i,3}(x) over the knots padded with three copies of
// t_1 and t_nt; l' = sum_i (C_{i+1} - C_i) M_{i,2}(x) over the knots padded with two -- the reference's coefficient differencing.
//
// The reference fills the whole Cox-de Boor table, (nt + 5) x 4 entries per point.  Of those only the triangle above the span
// that holds x is non-zero, four cubic B-splines and three quadratic M-splines, and the rest are exact zeros that it adds; so
// the triangle alone gives its numbers, in its order of operations: each term (x - t_i) B / (t_{i+d} - t_i) as product then
// quotient, a term whose knot difference is zero left out, the first term added before the second, the M-spline level scaled by
// (d + 1) / (d (t_{i+d+1} - t_i)).  The span rule is the reference's: t_s <= x < t_{s+1}, the last span closed on the right;
// an empty span (repeated knot) holds no point.  No span (x outside [t_1, t_nt]): l = l' = 0, NaN for a non-finite x (the
// reference's 0 * x).
//
// How the span's operands are found: a UNIFORM loop over the at most GPT_GIBBS_MAX_KNOTS - 1 spans that keeps, under the span's
// 0/1 mask, the six knots and four coefficients of the triangle in registers.  Every index into p is then the same in all
// lanes (scalar loads from the kernel arguments) and nothing depends on how a compiler lowers a lane-varying index into the
// by-value KParams of the single-matrix builders; a per-lane span search measured the same (both forms'
// registers, scratch and times).
GPT_HD static inline void gpt_gibbs_bspline(const double *p, int nt, double x, double *l, double *dl)
{
    const double *t = p, *C = p + nt;
    const double tlast = t[nt - 1];
    // k[m]: padded knot mu - 2 + m of the span mu that holds x, i.e. t[s - 2 + m] with the index held inside [0, nt - 1];
    // c[r]: coefficient s + r (the B-splines mu - 3 .. mu)
    double k[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, c[4] = {0.0, 0.0, 0.0, 0.0};
    bool hit = false;
#pragma unroll
    for (int s = 0; s < GPT_GIBBS_MAX_KNOTS - 1; s++) {
        if (s < nt - 1) {
            const bool in = (t[s] <= x) && ((x < t[s + 1]) || ((s == nt - 2) && (x == tlast)));
            if (in) {
#pragma unroll
                for (int m = 0; m < 6; m++) {
                    const int q = s - 2 + m;
                    k[m] = t[q < 0 ? 0 : (q > nt - 1 ? nt - 1 : q)];
                }
#pragma unroll
                for (int r = 0; r < 4; r++) c[r] = C[s + r];
                hit = true;
            }
        }
    }
    if (!hit) {
        *l = *dl = x - x;
        return;
    }
    // level d holds the functions mu - d .. mu as N[0 .. d]; function mu - d + r needs, of the padded knots, i -> k[2 - d + r],
    // i + d -> k[2 + r], i + d + 1 -> k[3 + r], i + 1 -> k[3 - d + r]
    double N[4] = {1.0, 0.0, 0.0, 0.0}, M[3] = {1.0 / (k[3] - k[2]), 0.0, 0.0};
#pragma unroll
    for (int d = 1; d <= 3; d++) {
        double Nn[4] = {0.0, 0.0, 0.0, 0.0}, Mn[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r <= d; r++) {
            double v = 0.0, w = 0.0;
            if (r >= 1 && k[2 + r] != k[2 - d + r]) {
                v += ((x - k[2 - d + r]) * N[r - 1]) / (k[2 + r] - k[2 - d + r]);
                if (d <= 2) w += (x - k[2 - d + r]) * M[r - 1];
            }
            if (r <= d - 1 && k[3 + r] != k[3 - d + r]) {
                v += ((k[3 + r] - x) * N[r]) / (k[3 + r] - k[3 - d + r]);
                if (d <= 2) w += (k[3 + r] - x) * M[r];
            }
            Nn[r] = v;
            if (d <= 2) {
                if (k[3 + r] != k[2 - d + r]) w *= (double)(d + 1) / ((double)d * (k[3 + r] - k[2 - d + r]));
                Mn[r] = w;
            }
        }
#pragma unroll
        for (int r = 0; r <= d; r++) N[r] = Nn[r];
        if (d <= 2) {
#pragma unroll
            for (int r = 0; r <= d; r++) M[r] = Mn[r];
        }
    }
    *l = ((N[0] * c[0] + N[1] * c[1]) + N[2] * c[2]) + N[3] * c[3];
    *dl = (M[0] * (c[1] - c[0]) + M[1] * (c[2] - c[1])) + M[2] * (c[3] - c[2]);
}

// Nested-GP length scale (GPT_KERNEL_GIBBS_GP; ref: gptools/kernel/gibbs.py:995-1095; the numpy statement is GPWarp in
// gptools_amd/kernel/gibbs.py).  p = [l, x_1 .. x_m, c_1 .. c_m], 1 <= m <= GPT_GIBBS_MAX_GP_POINTS: the mean of a noiseless GP with a
// squared-exponential kernel of length scale l through the points, whose weights c the host has solved for (gpt_hip.h) --
// S1 = sum_j c_j exp(-(x - x_j)^2 / (2 l^2)), S2 = sum_j c_j exp(..) (x - x_j) / l^2, terms added in index order as the numpy
// statement adds them;  l(x) = S1,  l'(x) = -S2.  One exponential per term serves both.  ONE uniform loop over m: every index
// into p is the same in all lanes (the rule of the B-spline above), so the by-value KParams stays on scalar loads.
GPT_HD static inline void gpt_gibbs_gp(const double *p, int m, double x, double *l, double *dl)
{
    const double s = p[0];
    double S1 = 0.0, S2 = 0.0;
    for (int j = 0; j < m; j++) {
        const double d = x - p[1 + j], c = p[1 + m + j];
        const double term = c * exp(-(d * d) / (2.0 * (s * s)));
        S1 += term;
        S2 += term * d / (s * s);
    }
    *l = S1;
    *dl = -S2;
}
