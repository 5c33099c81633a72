// warp_host.cpp -- test aid (not part of the product library): the warp functions of warp.hpp compiled by the host compiler,
// so that tests/test_warp_host.py can compare the device's incomplete beta function with scipy.special.betainc on a CPU.
#include "../warp.hpp"

extern "C" double gpt_host_betainc(double a, double b, double x) { return gpt_betainc(a, b, x); }
extern "C" double gpt_host_betainc_slope(double a, double b, double x) { return gpt_betainc_slope(a, b, x); }

// one coordinate of dimension d through `nlayers` layers (types / params as gpt_set_warp takes them, D dimensions)
extern "C" double gpt_host_warp_coord(int nlayers, const int *types, const double *params, int D, int d, double x, double *slope)
{
    WarpLayers wl = WarpLayers();
    wl.nlayers = nlayers;
    wl.D = D;
    for (int l = 0; l < nlayers && l < GPT_WARP_MAX_LAYERS; l++) {
        wl.type[l] = types[l];
        for (int q = 0; q < 2 * D; q++) wl.p[l][q] = params[l * 2 * D + q];
    }
    return gpt_warp_coord(wl, d, x, slope);
}
