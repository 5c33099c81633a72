// spectral_host.cpp -- test aid (not part of the product library): the spectral-mixture component's chain of spectral.hpp compiled
// by the host compiler, so that tests/test_spectral_host.py can compare it with the mpmath fixture on a CPU and the GPU tests can
// use it as the pair-by-pair statement of the kernel.  The exponential is the host's (std::exp); the device uses its own exp(-x).
#include <cmath>
#include <cstdint>
#include "../spectral.hpp"

template <int D>
static void pairs(const double *params, const double *Xi, const double *Xj, const int32_t *ni, const int32_t *nj, int64_t M, double *out)
{
    // params = [sigma_f, mu_1 .. mu_D, l_1 .. l_D]; 1 / l^2 formed as make_kparams forms it
    double mu[D], a[D];
    for (int d = 0; d < D; d++) {
        mu[d] = params[1 + d];
        a[d] = 1.0 / (params[1 + D + d] * params[1 + D + d]);
    }
    for (int64_t m = 0; m < M; m++) {
        int nir[D], njr[D];
        for (int d = 0; d < D; d++) {
            nir[d] = ni[m * D + d];
            njr[d] = nj[m * D + d];
        }
        double E;
        const double poly = gpt_spectral_chain<D>(mu, a, Xi + m * D, Xj + m * D, nir, njr, &E);
        out[m] = ((params[0] * params[0]) * std::exp(-E)) * poly;
    }
}

template <int D>
static int by_dim(int num_dim, const double *params, const double *Xi, const double *Xj, const int32_t *ni, const int32_t *nj, int64_t M,
                  double *out)
{
    if constexpr (D > 16) {
        return -1;
    } else {
        if (num_dim == D) {
            pairs<D>(params, Xi, Xj, ni, nj, M, out);
            return 0;
        }
        return by_dim<D + 1>(num_dim, params, Xi, Xj, ni, nj, M, out);
    }
}

// out[m] = k((Xi[m], ni[m]), (Xj[m], nj[m])) for M pairs of num_dim-dimensional points (row-major); 0, or -1 for a num_dim
// outside 1 .. 16
extern "C" int gpt_host_spectral_pairs(int num_dim, const double *params, const double *Xi, const double *Xj, const int32_t *ni,
                                       const int32_t *nj, int64_t M, double *out)
{
    return by_dim<1>(num_dim, params, Xi, Xj, ni, nj, M, out);
}
