"""Bucket and exp-Gauss Gibbs kernels on the host (no GPU): the numpy length-scale functions and the host GibbsKernel1d route
against the reference fixture (g17_gibbs_more.npz, from tests/golden/gen_g17_gibbs_more.py), names / counts / errors / pickling
of the native classes, and the device's length-scale functions (csrc/gibbs_lfunc.hpp) compiled for the CPU against the numpy
ones."""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, assert_close_nan

sys.path.insert(0, GOLDEN)
import gen_g17_gibbs_more as G17      # noqa: E402

import gptools_amd as g               # noqa: E402
from gptools_amd import _lib          # noqa: E402
from gptools_amd.kernel.gibbs import (GibbsKernel1d, cubic_bucket_warp, exp_gauss_warp,      # noqa: E402
                                      quintic_bucket_warp)

PAIR_CASES = sorted(G17.PAIR_CASES)
WARPS = {"cubic": cubic_bucket_warp, "quintic": quintic_bucket_warp, "expgauss": exp_gauss_warp}


def _pairs(golden, case):
    G = golden("g17_gibbs_more")
    return {k: G["pairs_%s__%s" % (case, k)] for k in ("xi", "xj", "ni", "nj", "params", "k")}


@pytest.mark.parametrize("case", PAIR_CASES)
def test_host_pairs_match_reference(golden, case):
    p = _pairs(golden, case)
    kind = G17.PAIR_CASES[case][0]
    k = GibbsKernel1d(WARPS[kind], num_params=len(p["params"]), initial_params=p["params"],
                      param_bounds=[(-10.0, 10.0)] * len(p["params"]))
    got = k(p["xi"][:, None], p["xj"][:, None], p["ni"][:, None], p["nj"][:, None])
    for a in (0, 1):
        for b in (0, 1):
            sel = (p["ni"] == a) & (p["nj"] == b)
            assert sel.any()
            assert_close_nan(got[sel], p["k"][sel], msg="%s class %d%d" % (case, a, b))


def test_fixture_matches_generator_inputs_and_holds_the_edge_cases(golden):
    for case in PAIR_CASES:
        p = _pairs(golden, case)
        xi, xj, ni, nj = G17.pair_data(case)
        for key, v in (("xi", xi), ("xj", xj), ("ni", ni), ("nj", nj), ("params", G17.PAIR_CASES[case][1])):
            np.testing.assert_array_equal(p[key], v, err_msg="%s %s" % (case, key))
        assert (p["xi"] == p["xj"]).any()
    for kk in ("c", "q"):
        base = _pairs(golden, kk + "_base")
        assert np.isfinite(base["k"]).all() and base["params"][0] != 1.0
        for e in (0.6, 0.8, 1.2, 1.5):
            assert (base["xi"] == e).any() and (base["xj"] == e).any()
        for e in G17.bucket_ends(base["params"]):
            assert (base["xi"] == e).any() and (base["xj"] == e).any()
        neg = _pairs(golden, kk + "_neg")
        assert np.isnan(neg["k"]).any() and np.isfinite(neg["k"]).any()
        assert np.isnan(_pairs(golden, kk + "_w10")["k"]).all()
        assert np.isfinite(_pairs(golden, kk + "_wneg")["k"]).all()
    # the tiny width: the quintic's fifth power overflows outside the section (NaN), the cubic stays finite
    assert np.isfinite(_pairs(golden, "c_tiny")["k"]).all()
    qt = _pairs(golden, "q_tiny")["k"]
    assert np.isnan(qt).sum() > 300 and np.isfinite(qt).any()
    assert [(len(G17.PAIR_CASES[c][1]) - 2) // 3 for c in ("e_g1", "e_g2", "e_g8")] == [1, 2, _lib.GIBBS_MAX_GAUSS]
    assert G17.MAX_GAUSS == _lib.GIBBS_MAX_GAUSS
    und = _pairs(golden, "e_under")
    s = und["params"][4:6].max()
    assert (np.abs(und["xi"][:, None] - und["params"][2:4]).min(axis=1) ** 2 / (2 * s * s) > 750).any()      # exp() underflows to 0
    assert np.isfinite(und["k"]).all()


def test_base_bucket_at_its_section_ends():
    """The base case at the decimal section ends 0.6, 0.8, 1.2, 1.5: l = l_1, l_2, l_2, l_3 and a zero slope, to rounding (the
    ends the reference computes differ from some of the decimals by an ulp, so a point may lie a hair inside a join)."""
    x = np.array([0.6, 0.8, 1.2, 1.5])
    for warp in (cubic_bucket_warp, quintic_bucket_warp):
        np.testing.assert_allclose(warp(x, 0, *G17.BASE[1:]), [1.0, 0.3, 0.3, 0.7], rtol=1e-15)
        np.testing.assert_allclose(warp(x, 1, *G17.BASE[1:]), 0.0, rtol=0, atol=1e-14)
        ends = G17.bucket_ends(G17.BASE)
        np.testing.assert_array_equal(warp(ends, 0, *G17.BASE[1:]), [1.0, 0.3, 0.3, 0.7])       # exactly one mask each
        np.testing.assert_array_equal(warp(ends, 1, *G17.BASE[1:]), [0.0, 0.0, 0.0, 0.0])


def test_warp_slope_is_derivative():
    """Cubic bucket and exp-Gauss: l' is the derivative of l.  The quintic bucket's l' is HALF of it: the reference differentiates
    in the shifted variable 2 (x - x_1)/w_1 and divides by w_1 where the chain rule gives 2/w_1 (gibbs.py:744-755).  A drop-in
    gives the reference's numbers, so the factor is reproduced, and pinned here."""
    x = np.linspace(-0.2, 2.2, 97) + 1e-3      # (off the section ends)
    h = 1e-6
    for kind, factor in (("cubic", 1.0), ("quintic", 0.5), ("expgauss", 1.0)):
        p = G17.TERM_PARAMS[kind][1:]
        fd = (WARPS[kind](x + h, 0, *p) - WARPS[kind](x - h, 0, *p)) / (2 * h)
        np.testing.assert_allclose(WARPS[kind](x, 1, *p), factor * fd, rtol=1e-6, atol=1e-8, err_msg=kind)


def test_names_counts_and_errors():
    bn = [r"\sigma_f", "l_1", "l_2", "l_3", "x_0", "w_1", "w_2", "w_3"]
    for cls, warp, kid in ((g.GibbsKernel1dCubicBucket, cubic_bucket_warp, _lib.KERNEL_GIBBS_CUBIC),
                           (g.GibbsKernel1dQuinticBucket, quintic_bucket_warp, _lib.KERNEL_GIBBS_QUINTIC)):
        k = cls(param_bounds=[(0, 1)] * 8)
        assert k.num_params == 8 and list(k.param_names) == bn and k.l_func is warp and k._gpt_kernel_id == kid
        assert type(k).__call__ is g.Kernel.__call__
        with pytest.raises(ValueError, match="only supports 1d"):
            cls(num_dim=2)
    k = g.GibbsKernel1dExpGauss(2, param_bounds=[(0, 1)] * 8)
    assert k.num_params == 8 and k.l_func is exp_gauss_warp and k._gpt_kernel_id == _lib.KERNEL_GIBBS_EXPGAUSS
    assert list(k.param_names) == [r"\sigma_f", "l_0", r"\mu_{1}", r"\mu_{2}", r"\sigma_{1}", r"\sigma_{2}", r"\beta_{1}", r"\beta_{2}"]
    assert type(k) is g.GibbsKernel1dExpGauss and type(k).__call__ is g.Kernel.__call__
    assert (_lib.KERNEL_GIBBS_CUBIC, _lib.KERNEL_GIBBS_QUINTIC, _lib.KERNEL_GIBBS_EXPGAUSS) == (9, 10, 11)
    x = np.array([0.5, 1.5])
    for warp, p in ((cubic_bucket_warp, G17.BASE[1:]), (quintic_bucket_warp, G17.BASE[1:])):
        with pytest.raises(NotImplementedError, match="Only up to first derivatives are supported!"):
            warp(x, 2, *p)
    with pytest.raises(NotImplementedError, match="Only n <= 1 is supported!"):
        exp_gauss_warp(x, 2, 0.5, 1.0, 0.3, 0.8)
    for name in ("GibbsKernel1dCubicBucket", "GibbsKernel1dQuinticBucket", "GibbsKernel1dExpGauss", "cubic_bucket_warp",
                 "quintic_bucket_warp", "exp_gauss_warp"):
        assert hasattr(g, name)


def test_exp_gauss_over_the_cap_is_a_host_kernel():
    G = _lib.GIBBS_MAX_GAUSS + 1
    k = g.GibbsKernel1dExpGauss(G, param_bounds=[(-10, 10)] * (3 * G + 2))
    assert isinstance(k, g.GibbsKernel1dExpGauss) and k.num_params == 3 * G + 2
    assert type(k).__call__ is GibbsKernel1d.__call__                     # a Python kernel: the host route
    gp = g.GaussianProcess(k)
    assert gp._native_terms() is None
    assert (k * g.SquaredExponentialKernel(num_dim=1, param_bounds=[(0, 1)] * 2))._native_factors() is None
    # ... and its numbers are the formula's: a zero-weight Gaussian more than the cap changes nothing
    rs = np.random.RandomState(5)
    p8 = np.asarray(G17.E_G8)
    p9 = np.concatenate((p8[:2], p8[2:10], [0.4], p8[10:18], [0.2], p8[18:26], [0.0]))
    k.set_hyperparams(p9)
    host8 = GibbsKernel1d(exp_gauss_warp, num_params=26, initial_params=p8, param_bounds=[(-10, 10)] * 26)
    xi, xj = rs.uniform(0, 2, (50, 1)), rs.uniform(0, 2, (50, 1))
    ni, nj = rs.randint(0, 2, (50, 1)), rs.randint(0, 2, (50, 1))
    np.testing.assert_array_equal(k(xi, xj, ni, nj), host8(xi, xj, ni, nj))
    k2 = pickle.loads(pickle.dumps(k))
    assert type(k2) is type(k) and k2.num_params == k.num_params
    np.testing.assert_array_equal(k2.params, k.params)


@pytest.mark.parametrize("kind", G17.KINDS)
def test_pickle_round_trip(golden, kind):
    G = golden("g17_gibbs_more")
    td = {k[len("terms__"):]: v for k, v in G.items() if k.startswith("terms__")}
    gp = G17.make_terms_gp(g, kind + "_sum_se", td)
    gp2 = pickle.loads(pickle.dumps(gp))
    k1, k2 = gp.k.k1, gp2.k.k1
    assert type(k2) is type(k1) and k2._gpt_kernel_id == k1._gpt_kernel_id and k2.l_func is k1.l_func
    np.testing.assert_array_equal(gp2.k.params, gp.k.params)
    assert list(k2.param_names) == list(k1.param_names)
    np.testing.assert_array_equal(gp2.X, gp.X)
    assert gp2._native_terms() is not None and [t[0] for t in gp2._native_terms()] == [t[0] for t in gp._native_terms()]


def test_compute_l_from_mcmc(golden):
    G = golden("g17_gibbs_more")
    td = {k[len("terms__"):]: v for k, v in G.items() if k.startswith("terms__")}
    gp = G17.make_terms_gp(g, "cubic_alone", td)
    trace, X = G["lmcmc__trace"], G["lmcmc__X"]
    l0 = gp.compute_l_from_MCMC(X, n=0, flat_trace=trace)
    l1 = gp.compute_l_from_MCMC(X, n=1, flat_trace=trace)
    assert l0.shape == (12, 50) and l1.shape == (12, 50)
    np.testing.assert_allclose(l0, G["lmcmc__l0"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(l1, G["lmcmc__l1"], rtol=1e-13, atol=1e-300)


# ---- the device's length-scale functions, compiled for the CPU ------------------------------------------------------------------
# Both sides are the same double-precision expression in the same order; they differ in the integer powers (repeated multiplication
# on the device, pow in numpy: <= 2 ulp of a term) and in exp (two libm builds, <= 1 ulp each).  Inside a join |shift| <= 1 and
# every term of the polynomial is within a factor 2 of the result's scale, so a dozen operations stay below 1e-14 of the largest
# value; relative to each value that fails only where l crosses zero (the *_neg cases), which the absolute term covers.
LFUNC_RTOL = 1e-14
LFUNC_ATOL_SCALE = 1e-14


@pytest.fixture(scope="module")
def gibbs_host():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gptools_amd", "csrc")
    subprocess.run(["make", "-C", here, "gibbs_host"], check=True, stdout=subprocess.DEVNULL)
    L = ctypes.CDLL(os.path.join(here, "build", "libgibbs_host.so"))
    dp = ctypes.POINTER(ctypes.c_double)
    L.gpt_host_gibbs_l.restype = ctypes.c_int
    L.gpt_host_gibbs_l.argtypes = [ctypes.c_int, dp, ctypes.c_int, dp, ctypes.c_long, dp, dp]

    def run(kind, params, x):
        p = np.ascontiguousarray(params[1:], dtype=float)
        x = np.ascontiguousarray(x, dtype=float)
        l, dl = np.empty_like(x), np.empty_like(x)
        G = (len(params) - 2) // 3 if kind == "expgauss" else 0
        rc = L.gpt_host_gibbs_l(G17.KINDS.index(kind), p.ctypes.data_as(dp), G, x.ctypes.data_as(dp), len(x),
                                l.ctypes.data_as(dp), dl.ctypes.data_as(dp))
        assert rc == 0
        return l, dl
    return run


@pytest.mark.parametrize("case", PAIR_CASES)
def test_device_length_scale_functions_against_numpy(golden, gibbs_host, case):
    p = _pairs(golden, case)
    kind = G17.PAIR_CASES[case][0]
    x = np.concatenate((p["xi"], p["xj"]))
    l, dl = gibbs_host(kind, p["params"], x)
    want_l, want_dl = WARPS[kind](x, 0, *p["params"][1:]), WARPS[kind](x, 1, *p["params"][1:])
    assert_close_nan(l, want_l, rtol=LFUNC_RTOL, atol_scale=LFUNC_ATOL_SCALE, msg=case + " l")
    assert_close_nan(dl, want_dl, rtol=LFUNC_RTOL, atol_scale=LFUNC_ATOL_SCALE, msg=case + " l'")
    if kind != "expgauss" and case.endswith("_base"):
        ends = G17.bucket_ends(p["params"])
        le, dle = gibbs_host(kind, p["params"], ends)
        np.testing.assert_array_equal(le, [1.0, 0.3, 0.3, 0.7])
        np.testing.assert_array_equal(dle, [0.0, 0.0, 0.0, 0.0])
