"""Input-warped kernels on the host (gptools_amd/kernel/warping.py), no GPU: the host class around stand-in inner kernels that
evaluate pairs through the CPU oracle, against the reference's outputs (tests/golden/g16_warp.npz, gen_g16_warp.py); the warp
functions, the parameter plumbing, the errors, compute_w_from_MCMC, pickling; and the device's incomplete beta function
(csrc/warp.hpp) compiled for the CPU against scipy.special.betainc."""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import scipy.special
import scipy.stats

from conftest import GOLDEN, assert_close, assert_close_nan

sys.path.insert(0, GOLDEN)
import gen_g16_warp as G16      # noqa: E402

# the tolerance tests/test_oracle_golden.py uses for the same inner kernel (the warp itself is the reference's own scipy call)
PAIR_TOL = {"se": dict(rtol=1e-11), "m52": dict(rtol=1e-12), "rq": dict(rtol=2e-12, atol_scale=1e-14),
            "sum": dict(rtol=1e-11), "prod": dict(rtol=1e-11)}


@pytest.fixture(scope="module")
def g():
    import gptools_amd
    return gptools_amd


@pytest.fixture(scope="module")
def factory(oracle):
    from gptools_amd.kernel.core import Kernel

    class OracleKernel(Kernel):
        """A Python kernel whose pairs the CPU oracle evaluates (stand-in for the GPU pair list)."""

        def __init__(self, name, D, params):
            Kernel.__init__(self, num_dim=D, num_params=len(params), initial_params=list(params),
                            param_bounds=[G16.B] * len(params))
            self.name = name

        def __call__(self, Xi, Xj, ni, nj, hyper_deriv=None, symmetric=False):
            return oracle.kpairs(self.name, self.params, Xi, Xj, ni, nj, hyper_deriv=hyper_deriv, symmetric=symmetric)

    def make(g, name, D):
        return OracleKernel(name, D, G16.native(g, name, D).params)
    return make


@pytest.mark.parametrize("D", G16.DIMS)
@pytest.mark.parametrize("warp", G16.WARPS)
@pytest.mark.parametrize("inner", G16.INNERS)
def test_pairs_match_reference(g, golden, factory, inner, warp, D):
    G = golden("g16_warp")
    p = {k: G["pairs_%s_%s_d%d__%s" % (inner, warp, D, k)] for k in ("xi", "xj", "ni", "nj", "k")}
    k = G16.make_kernel(g, inner, warp, D, factory)
    assert_close(k(p["xi"], p["xj"], p["ni"].astype(int), p["nj"].astype(int)), p["k"], msg="%s %s %d" % (inner, warp, D),
                 **PAIR_TOL[inner])


@pytest.mark.parametrize("D", G16.DIMS)
def test_edges_of_the_unit_interval(g, golden, factory, D):
    G = golden("g16_warp")
    k = G16.make_kernel(g, "se", "beta", D, factory)
    z = np.zeros((12, D), dtype=int)
    got = k(G["edge_d%d__xi" % D], G["edge_d%d__xj" % D], z, z)
    assert np.isnan(G["edge_d%d__k" % D]).sum() == 3
    assert_close_nan(got, G["edge_d%d__k" % D], rtol=1e-11)
    assert g.beta_cdf_warp(np.array([0.0, 1.0]), 0, 0, 0.4, 2.2).tolist() == [0.0, 1.0]
    assert np.isnan(g.beta_cdf_warp(np.array([-0.1, 1.1]), 0, 0, 0.4, 2.2)).all()


@pytest.mark.parametrize("D", G16.DIMS)
@pytest.mark.parametrize("warp", G16.WARPS)
def test_warp_functions_against_reference(g, golden, factory, warp, D):
    G = golden("g16_warp")
    k = G16.make_kernel(g, "se", warp, D, factory)
    x = G["wfun_%s_d%d__x" % (warp, D)]
    np.testing.assert_allclose(k.w_func(x, 0, 0), G["wfun_%s_d%d__w" % (warp, D)], rtol=1e-15, atol=0)
    if warp in ("beta", "lin"):
        np.testing.assert_allclose(k.w_func(x, 0, 1), G["wfun_%s_d%d__w1" % (warp, D)], rtol=1e-15, atol=0)
    # the slope of the whole (nested) warp is the derivative of its value: central difference, O(h^2) + rounding / h
    h = 1e-6 * (G16.LIN_B[0] - G16.LIN_A[0] if warp.startswith("lin") else 1.0)
    fd = (k.w_func(x + h, 0, 0) - k.w_func(x - h, 0, 0)) / (2 * h)
    np.testing.assert_allclose(k.w_func(x, 0, 1), fd, rtol=1e-7)


def test_nesting_order(g, factory):
    """WarpedKernel(WarpedKernel(k, w_in), w_out) applies w_out first; each slope at its own layer's input."""
    D = 1
    k = G16.make_kernel(g, "se", "lin_beta", D, factory)
    a, b = G16.LIN_A[0], G16.LIN_B[0]
    al, be = G16.BETA_P[:2]
    x = np.linspace(a + 0.1, b - 0.1, 7)
    u = (x - a) / (b - a)
    np.testing.assert_allclose(k.w_func(x, 0, 0), scipy.special.betainc(al, be, u), rtol=1e-15)
    np.testing.assert_allclose(k.w_func(x, 0, 1), g.beta_cdf_warp(u, 0, 1, al, be) / (b - a), rtol=1e-15)
    assert [str(s) for s in k.param_names] == ["", "", "\\alpha_0", "\\beta_0", "a_0", "b_0"]
    k2 = G16.make_kernel(g, "se", "beta_lin", D, factory)
    x2 = np.linspace(0.1, 0.9, 7)
    np.testing.assert_allclose(k2.w_func(x2, 0, 0), (scipy.special.betainc(al, be, x2) - a) / (b - a), rtol=1e-15)
    assert [str(s) for s in k2.param_names][2:] == ["a_0", "b_0", "\\alpha_0", "\\beta_0"]


@pytest.mark.parametrize("D", G16.DIMS)
@pytest.mark.parametrize("case", [c for c in G16.FIT_CASES if c != "T"])
def test_gram_ll_alpha_match_reference(g, golden, oracle, factory, case, D):
    G = golden("g16_warp")
    d = {k[len("fit_d%d__" % D):]: v for k, v in G.items() if k.startswith("fit_d%d__" % D)}
    key = "fit_%s_d%d__" % (case, D)
    gp = G16.make_fit_gp(g, case, D, d, factory)
    K = gp.compute_Kij(gp.X, None, gp.n, None)
    inner = "se" if case == "noise" else case.split("_")[0]
    assert_close(K, G[key + "K"], msg=key + "K", **PAIR_TOL[inner])
    N = len(gp.y)
    noise = gp.noise_k.params[0] ** 2 if case == "noise" else 0.0
    K_tot = K + (noise + gp.diag_factor * sys.float_info.epsilon) * np.eye(N) + np.diag(gp.err_y ** 2)
    L = oracle.potrf_lower(K_tot)
    z = oracle.solve_lower(L, gp.y[:, None])
    alpha = oracle.solve_lower(L, z, trans=True).ravel()
    ll = -0.5 * float(z.ravel().dot(z.ravel())) - np.log(np.diag(L)).sum() - 0.5 * N * np.log(2 * np.pi) + gp.hyperprior(gp.params)
    assert abs(ll - G[key + "ll"]) <= 1e-8 * abs(G[key + "ll"])          # (the unwarped fits: test_g8_rational_quadratic_gram_fit_predict)
    assert_close(alpha, G[key + "alpha"], rtol=1e-7, atol_scale=1e-8, msg=key + "alpha")


def test_parameter_plumbing(g, factory):
    k = G16.make_kernel(g, "se", "lin_beta", 2, factory)
    assert k.num_params == 3 + 4 + 4 and len(k.params) == 11
    assert list(k.params[3:7]) == G16.BETA_P[:4] and list(k.params[7:]) == [-1.0, 3.0, 2.0, 2.5]
    assert list(k.fixed_params) == [False] * 7 + [True] * 4
    assert [str(s) for s in k.param_names][3:] == ["\\alpha_0", "\\beta_0", "\\alpha_1", "\\beta_1", "a_0", "b_0", "a_1", "b_1"]
    assert len(k.free_params) == 7 and k.num_free_params == 7
    lo, hi = k.param_bounds[7]
    assert abs(lo - (-1.0 - 1e-3)) < 1e-15 and abs(hi - (-1.0 + 1e-3)) < 1e-15
    new = np.arange(1.0, 8.0) / 4.0
    k.set_hyperparams(new)
    assert list(k.k.k.params) == list(new[:3]) and list(k.k.w.params) == list(new[3:])       # split [k | w]
    assert list(k.free_params[:]) == list(new) and list(k.params[7:]) == [-1.0, 3.0, 2.0, 2.5]
    k.free_params = new * 2
    assert list(k.free_params[:]) == list(new * 2)
    with pytest.raises(ValueError):
        k.set_hyperparams(new[:-1])
    k.enforce_bounds = True
    assert k.k.enforce_bounds and k.w.enforce_bounds and k.k.w.enforce_bounds and k.k.k.enforce_bounds
    k.set_hyperparams([1e9] * 7)
    assert list(k.params[3:7]) == [1e2] * 4                              # clamped onto the beta layer's bounds
    # default prior of the beta warp: log-normal(0, 0.5) per parameter; hyperprior = product of the parts'
    kb = g.BetaWarpedKernel(factory(g, "se", 2))
    assert isinstance(kb.w.hyperprior, g.LogNormalJointPrior) and len(kb.w.hyperprior.bounds) == 4
    assert list(kb.w.params) == [1.0] * 4 and not kb.w.fixed_params.any()
    th = np.array(kb.params, dtype=float)
    assert abs(kb.hyperprior(th) - (kb.k.hyperprior(th[:3]) + kb.w.hyperprior(th[3:]))) < 1e-14
    ref = np.sum(np.log(scipy.stats.lognorm.pdf(th[3:], 0.5, loc=0, scale=1.0)))
    assert abs(kb.w.hyperprior(th[3:]) - ref) < 1e-12
    # a user warp function: parameters counted from its signature
    wk = g.WarpedKernel(factory(g, "se", 1), lambda X, d, n, p, q: X * p + q if n == 0 else p * np.ones_like(X))
    assert wk.w.num_params == 2 and wk.num_params == 4


def test_errors(g, factory):
    k = G16.make_kernel(g, "se", "beta", 2, factory)
    X = np.full((3, 2), 0.5)
    n2 = np.array([[0, 0], [2, 0], [0, 1]])
    with pytest.raises(ValueError, match="greater than one"):
        k(X, X, n2, np.zeros((3, 2), int))
    with pytest.raises(ValueError, match="greater than one"):
        k(X, X, np.zeros((3, 2), int), n2)
    with pytest.raises(ValueError, match="same number of dimensions"):
        g.WarpedKernel(factory(g, "se", 2), g.WarpingFunction(g.linear_warp, num_dim=1, num_params=2))
    with pytest.raises(ValueError):
        g.LinearWarpedKernel(factory(g, "se", 2), [0.0], [1.0, 1.0])
    with pytest.raises(ValueError):
        k.w_func(np.array([0.5]), 0, 2)


def test_compute_w_from_mcmc(g, golden, factory):
    G = golden("g16_warp")
    d = {k[len("fit_d1__"):]: v for k, v in G.items() if k.startswith("fit_d1__")}
    gp = G16.make_fit_gp(g, "se_beta", 1, d, factory)
    before = list(gp.k.params)
    trace, X = G["wmcmc__trace"], G["wmcmc__X"]
    w0 = gp.compute_w_from_MCMC(X, n=0, flat_trace=trace)
    assert w0.shape == (12, 20)
    np.testing.assert_allclose(w0, G["wmcmc__w0"], rtol=1e-15)
    np.testing.assert_allclose(gp.compute_w_from_MCMC(X, n=1, flat_trace=trace), G["wmcmc__w1"], rtol=1e-15)
    np.testing.assert_allclose(gp.compute_w_from_MCMC(X, n=0, flat_trace=trace, burn=2, thin=3), G["wmcmc__w0_bt"], rtol=1e-15)
    assert list(gp.k.params) == before
    bad = trace.copy()
    bad[3, 2] = np.nan
    wn = gp.compute_w_from_MCMC(X, flat_trace=bad)
    assert np.isnan(wn[3]).all() and np.isfinite(np.delete(wn, 3, axis=0)).all()

    class Sampler(object):
        chain = trace.reshape(3, 4, 4)
    np.testing.assert_array_equal(gp.compute_w_from_MCMC(X, sampler=Sampler(), burn=1), gp.compute_w_from_MCMC(
        X, flat_trace=trace.reshape(3, 4, 4)[:, 1:, :].reshape(-1, 4)))
    with pytest.raises(NotImplementedError, match="flat_trace"):
        gp.compute_w_from_MCMC(X)


def test_gp_with_warped_kernel_pickles(g):
    k = g.BetaWarpedKernel(g.LinearWarpedKernel(g.SquaredExponentialKernel(num_dim=2, initial_params=[1, 0.5, 0.5],
                                                                           param_bounds=[(0, 10)] * 3), [0, 0], [2, 2]))
    gp = g.GaussianProcess(k, X=np.random.rand(5, 2), y=np.random.rand(5), err_y=0.1)
    gp2 = pickle.loads(pickle.dumps(gp))
    assert gp2._ctx_obj is None and gp2.K_up_to_date is False
    assert list(gp2.k.params) == list(gp.k.params) and list(gp2.k.fixed_params) == list(gp.k.fixed_params)
    assert gp2.k.w.fun is g.beta_cdf_warp and gp2._device_model() is not None


def test_device_model_peels_outer_layers_only(g):
    se = lambda: g.SquaredExponentialKernel(num_dim=1, initial_params=[1, 0.5], param_bounds=[(0, 10)] * 2)      # noqa: E731
    gp = g.GaussianProcess(g.LinearWarpedKernel(g.BetaWarpedKernel(se() + se()), [0.0], [2.0]))
    terms, layers = gp._device_model()
    assert len(terms) == 2 and [t for t, _ in layers] == [1, 2] and list(layers[0][1]) == [0.0, 2.0]
    assert gp._native_terms() is None and not gp._partitioned_possible()
    assert g.GaussianProcess(g.BetaWarpedKernel(se()) + se())._device_model() is None          # a warped term of a sum
    assert g.GaussianProcess(g.WarpedKernel(se(), lambda X, d, n, p: X * p))._device_model() is None      # a user warp

    class Mine(g.BetaWarpedKernel):
        def __call__(self, *a, **kw):
            return g.BetaWarpedKernel.__call__(self, *a, **kw)
    assert g.GaussianProcess(Mine(se()))._device_model() is None
    assert g.GaussianProcess(se())._device_model()[1] == []


# ---- the device's incomplete beta function, compiled for the CPU -------------------------------------------------------------
# Measured on the grid below: largest relative deviation from scipy.special.betainc 2.9e-14 (at the reflection point
# x = (a + 1)/(a + b + 2) with a = 9.3, b = 0.63, where 1 - I_{1-x}(b, a) cancels a digit), slope 7.4e-15; asserted with a factor 4.
BETAINC_RTOL = 4 * 2.9e-14
SLOPE_RTOL = 4 * 7.4e-15


@pytest.fixture(scope="module")
def warp_host():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gptools_amd", "csrc")
    subprocess.run(["make", "-C", here, "warp_host"], check=True, stdout=subprocess.DEVNULL)
    L = ctypes.CDLL(os.path.join(here, "build", "libwarp_host.so"))
    for f in (L.gpt_host_betainc, L.gpt_host_betainc_slope):
        f.restype, f.argtypes = ctypes.c_double, [ctypes.c_double] * 3
    return L


def test_device_betainc_against_scipy(warp_host):
    ab = np.exp(np.linspace(np.log(0.2), np.log(20.0), 25))
    worst = worst_s = 0.0
    for a in ab:
        for b in ab:
            xr = (a + 1) / (a + b + 2)
            xs = np.concatenate(([0.0, 1e-300, 1e-100, 1e-10, 1 - 2.0 ** -53, 1.0, xr, np.nextafter(xr, 1)],
                                 np.linspace(0.001, 0.999, 41)))
            for x in xs:
                want, got = scipy.special.betainc(a, b, x), warp_host.gpt_host_betainc(a, b, x)
                if want < 1e-290:                   # underflow: no relative statement
                    assert 0.0 <= got < 1e-280, (a, b, x, got, want)
                    continue
                worst = max(worst, abs(got - want) / want)
                if 0.0 < x < 1.0:
                    ws = (1 - x) ** (b - 1) * x ** (a - 1) / scipy.special.beta(a, b)
                    if 1e-290 < ws < np.inf:
                        worst_s = max(worst_s, abs(warp_host.gpt_host_betainc_slope(a, b, x) - ws) / ws)
    print("betainc: worst relative deviation %.3g, slope %.3g" % (worst, worst_s))
    assert worst <= BETAINC_RTOL and worst_s <= SLOPE_RTOL
    assert warp_host.gpt_host_betainc(2.0, 3.0, 0.0) == 0.0 and warp_host.gpt_host_betainc(2.0, 3.0, 1.0) == 1.0
    for a, b, x in ((2.0, 3.0, -0.1), (2.0, 3.0, 1.1), (0.0, 3.0, 0.5), (2.0, -1.0, 0.5), (2.0, 3.0, np.nan)):
        assert np.isnan(warp_host.gpt_host_betainc(a, b, x)) and np.isnan(warp_host.gpt_host_betainc_slope(a, b, x))
