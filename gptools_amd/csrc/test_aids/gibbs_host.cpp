// gibbs_host.cpp -- test aid (not part of the product library): the length-scale functions of gibbs_lfunc.hpp compiled by the
// host compiler, so that tests/test_gibbs_more_host.py and tests/test_splines_host.py can compare what the device evaluates with the numpy functions on a CPU.
#include "../gibbs_lfunc.hpp"

// kind 0: cubic bucket, 1: quintic bucket (p: the 7 parameters after sigma_f), 2: exp-Gauss (p: the 3 G + 1 after sigma_f);
// l[m], dl[m] at x[m]
extern "C" int gpt_host_gibbs_l(int kind, const double *p, int G, const double *x, long M, double *l, double *dl)
{
    if (kind < 0 || kind > 2 || (kind == 2 && (G < 1 || G > GPT_GIBBS_MAX_GAUSS))) return -1;
    for (long m = 0; m < M; m++) {
        if (kind == 0) gpt_gibbs_cubic_bucket(p, x[m], l + m, dl + m);
        else if (kind == 1) gpt_gibbs_quintic_bucket(p, x[m], l + m, dl + m);
        else gpt_gibbs_exp_gauss(p, G, x[m], l + m, dl + m);
    }
    return 0;
}

// the B-spline (p: the nt knots, then the nt + 2 coefficients); knots in increasing order are the caller's business, as on the device
extern "C" int gpt_host_gibbs_bspline(const double *p, int nt, const double *x, long M, double *l, double *dl)
{
    if (nt < 2 || nt > GPT_GIBBS_MAX_KNOTS) return -1;
    for (long m = 0; m < M; m++) gpt_gibbs_bspline(p, nt, x[m], l + m, dl + m);
    return 0;
}

// the nested GP (p: the length scale, the m points, the m weights)
extern "C" int gpt_host_gibbs_gp(const double *p, int m, const double *x, long M, double *l, double *dl)
{
    if (m < 1 || m > GPT_GIBBS_MAX_GP_POINTS) return -1;
    for (long q = 0; q < M; q++) gpt_gibbs_gp(p, m, x[q], l + q, dl + q);
    return 0;
}
