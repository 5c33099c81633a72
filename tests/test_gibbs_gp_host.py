"""GibbsKernel1dGP / GPWarp on the host (no GPU): construction, routing, the numpy closed form against the reference fixture
(g20_gibbs_gp.npz, from tests/golden/gen_g20_gibbs_gp.py) and the device's length-scale function (csrc/gibbs_lfunc.hpp,
gpt_gibbs_gp) compiled for the CPU against the numpy one."""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg

from conftest import GOLDEN, assert_close_nan

sys.path.insert(0, GOLDEN)
import gen_g20_gibbs_gp as G20        # noqa: E402

import gptools_amd as g               # noqa: E402
from gptools_amd import _lib          # noqa: E402
from gptools_amd.kernel.gibbs import GibbsKernel1d, GPWarp      # noqa: E402

CASES = sorted(G20.CASES)
# the bounds tests/test_gibbs_more_host.py uses for the other length-scale functions: a sum of at most 12 terms; relative to each
# value that fails only where the terms cancel (outside the points, m5wide between them), which the absolute term covers
LFUNC_RTOL = 1e-14
LFUNC_ATOL_SCALE = 1e-14


def _pairs(golden, case):
    G = golden("g20_gibbs_gp")
    return {k: G["pairs_%s__%s" % (case, k)] for k in ("xi", "xj", "ni", "nj", "params", "sigma_n", "k", "l", "dl")}


def assert_pairs(got, want, ins, rtol=1e-12, atol_scale=1e-13, msg=""):
    """Rows inside the hull of the points: rtol plus atol_scale of the largest value; rows outside (the nested mean is a
    cancellation residue there): the absolute part alone; NaN for NaN everywhere."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=msg + " (NaN pattern)")
    fin = np.isfinite(want)
    scale = np.abs(want[fin]).max()
    np.testing.assert_allclose(got[fin & ins], want[fin & ins], rtol=rtol, atol=atol_scale * scale, err_msg=msg)
    np.testing.assert_allclose(got[fin & ~ins], want[fin & ~ins], rtol=0, atol=atol_scale * scale, err_msg=msg + " (outside)")


def _weights(case):
    """The statement of the issue, written out: c = sigma_n^2 (sigma_n^2 E + 1e2 eps I)^-1 y."""
    x, l, y, sn = G20.CASES[case]
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    E = np.exp(-(x[:, None] - x[None, :]) ** 2.0 / (2.0 * l ** 2.0))
    K_tot = sn ** 2.0 * E + 1e2 * sys.float_info.epsilon * np.eye(len(x))
    return sn ** 2.0 * scipy.linalg.cho_solve(scipy.linalg.cho_factor(K_tot, lower=True), y)


# ---- construction ---------------------------------------------------------------------------------------------------------------
def test_count_names_and_default_nested_kernel():
    k = G20.gp_kernel(g, "m5")
    assert type(k) is g.GibbsKernel1dGP and k.num_params == 1 + 1 + 2 * 5 and k.num_dim == 1
    assert list(k.param_names) == ([r"\sigma_f", "l_1"] + ["x_{%d}" % i for i in range(1, 6)] + ["y_{%d}" % i for i in range(1, 6)])
    assert isinstance(k.l_func, GPWarp) and k.l_func.npts == 5 and k._gpt_kernel_id == _lib.KERNEL_GIBBS_GP == 13
    assert type(k).__call__ is g.Kernel.__call__
    assert g.kernel.GibbsKernel1dGP is g.GibbsKernel1dGP and g.kernel.GPWarp is g.GPWarp
    # k=None: the default the reference documents (and cannot construct): SE, sigma_f = 1 fixed, l_1 = 1 free
    kd = g.GibbsKernel1dGP(3, param_bounds=[(0, 10)] * 8)
    nk = kd.l_func.k
    assert type(kd) is g.GibbsKernel1dGP and type(nk) is g.SquaredExponentialKernel and nk.num_dim == 1
    np.testing.assert_array_equal(nk.params, [1.0, 1.0])
    np.testing.assert_array_equal(nk.fixed_params, [True, False])
    assert [tuple(b) for b in nk.param_bounds] == [(0.0, 1e16)] * 2
    assert kd.num_params == 8 and list(kd.param_names)[:2] == [r"\sigma_f", "l_1"]
    # two free nested parameters: both are hyperparameters of the outer kernel, in the nested kernel's order
    k2 = g.GibbsKernel1dGP(2, k=g.SquaredExponentialKernel(param_bounds=[(0, 10)] * 2), param_bounds=[(0, 10)] * 7)
    assert k2.num_params == 7 and list(k2.param_names)[:3] == [r"\sigma_f", r"\sigma_f", "l_1"]
    with pytest.raises(ValueError, match="only supports 1d"):
        g.GibbsKernel1dGP(3, num_dim=2)
    with pytest.raises(ValueError, match="only supports 1d"):
        GPWarp(3, k=g.SquaredExponentialKernel(num_dim=2, param_bounds=[(0, 10)] * 3))


def test_orders_and_hyper_deriv_are_refused():
    k = G20.gp_kernel(g, "m5")
    with pytest.raises(NotImplementedError, match="Only derivatives up to order 1 are supported!"):
        k.l_func(np.zeros(3), 2, *k.params[1:])
    kh = GibbsKernel1d(k.l_func, num_params=12, initial_params=k.params, param_bounds=[(-10, 10)] * 12)
    x = np.array([[0.5]])
    with pytest.raises(NotImplementedError, match="Hyperparameter derivatives have not been implemented!"):
        kh(x, x, [[0]], [[0]], hyper_deriv=1)
    with pytest.raises(NotImplementedError, match=r"Derivatives greater than \[1, 1\] are not supported!"):
        kh(x, x, [[2]], [[0]])


@pytest.mark.parametrize("case", ["m5", "host"])
def test_pickle_round_trip(case):
    if case == "host":
        m = _lib.GIBBS_MAX_GP_POINTS + 1
        k = g.GibbsKernel1dGP(m, initial_params=[1.1, 0.3] + list(np.linspace(0, 2, m)) + [0.5] * m, param_bounds=[(0, 10)] * (2 * m + 2))
    else:
        k = G20.gp_kernel(g, case)
    k2 = pickle.loads(pickle.dumps(k))
    assert type(k2) is type(k) and k2._gpt_kernel_id == k._gpt_kernel_id and k2.l_func.npts == k.l_func.npts
    np.testing.assert_array_equal(k2.params, k.params)
    assert list(k2.param_names) == list(k.param_names)
    x = np.linspace(0.0, 2.0, 7)
    np.testing.assert_array_equal(k2.l_func(x, 0, *k2.params[1:]), k.l_func(x, 0, *k.params[1:]))


# ---- routing (no library call) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_native_terms_carry_the_weights(case):
    k = G20.gp_kernel(g, case)
    terms = g.GaussianProcess(k)._native_terms()
    m = len(G20.CASES[case][0])
    assert terms is not None and len(terms) == 1 and terms[0][0] == 13 and len(terms[0][1]) == 2 * m + 2
    p = terms[0][1]
    np.testing.assert_array_equal(p[:2 + m], [G20.SIGMA_F, G20.CASES[case][1]] + list(G20.CASES[case][0]))
    np.testing.assert_array_equal(p[2 + m:], _weights(case))
    # ... and as a product factor, and masked onto one coordinate
    se = g.SquaredExponentialKernel(num_dim=1, param_bounds=[(0, 10)] * 2)
    f = (k * se)._native_factors()
    assert f is not None and f[0] == 13 and f[2] == _lib.KERNEL_SE
    np.testing.assert_array_equal(f[1], p)
    t = g.MaskedKernel(k, total_dim=2, mask=[1])._native_term()
    assert t is not None and t[0] == _lib.kernel_on_dim(13, 1) and t[2] == _lib.KERNEL_SE
    np.testing.assert_array_equal(t[1], p)


def test_host_subclass_for_what_the_device_does_not_carry():
    m = _lib.GIBBS_MAX_GP_POINTS + 1
    se = g.SquaredExponentialKernel(num_dim=1, param_bounds=[(0, 10)] * 2)
    many = g.GibbsKernel1dGP(m, k=G20.nested_se(g), param_bounds=[(0, 10)] * (2 * m + 2))
    m52 = g.GibbsKernel1dGP(3, k=g.Matern52Kernel(initial_params=[1.0, 0.5], fixed_params=[True, False], param_bounds=[(0, 10)] * 2),
                            param_bounds=[(0, 10)] * 8)
    free_sigma = g.GibbsKernel1dGP(3, k=g.SquaredExponentialKernel(param_bounds=[(0, 10)] * 2), param_bounds=[(0, 10)] * 9)

    class Mine(g.GibbsKernel1dGP):
        __call__ = GibbsKernel1d.__call__
    mine = Mine(3, k=G20.nested_se(g), param_bounds=[(0, 10)] * 8)
    for k in (many, m52, free_sigma, mine):
        assert isinstance(k, g.GibbsKernel1dGP) and type(k) is not g.GibbsKernel1dGP
        assert type(k).__call__ is GibbsKernel1d.__call__
        assert g.GaussianProcess(k)._native_terms() is None
        assert (k * se)._native_factors() is None
        assert g.MaskedKernel(k, total_dim=2, mask=[0])._native_term() is None
    assert many.num_params == 2 * m + 2 and free_sigma.num_params == 9


def test_general_nested_kernel_equals_the_closed_form():
    """A Python subclass of the squared exponential as the nested kernel goes through that kernel's own __call__ (here numpy): the
    same numbers as the closed form, to rounding."""
    class PySE(g.SquaredExponentialKernel):
        def __call__(self, Xi, Xj, ni, nj, hyper_deriv=None, symmetric=False):
            d = np.asarray(Xi, dtype=float)[:, 0] - np.asarray(Xj, dtype=float)[:, 0]
            s, l = self.params
            k = s ** 2 * np.exp(-d ** 2 / (2 * l ** 2))
            ni, nj = np.asarray(ni)[:, 0], np.asarray(nj)[:, 0]
            assert (nj == 0).all() and (ni <= 1).all()
            return np.where(ni == 1, -d / l ** 2 * k, k)
    x, l, y, sn = G20.CASES["m5"]
    w = GPWarp(5, k=PySE(initial_params=[1.7, 0.9], fixed_params=[True, False], param_bounds=[(0, 10)] * 2))
    ref = GPWarp(5, k=G20.nested_se(g, 1.7, 0.9))
    assert not w._closed_form() and ref._closed_form()
    X = np.linspace(-0.3, 2.3, 41)
    for n in (0, 1):
        got, want = w(X, n, l, *(list(x) + list(y))), ref(X, n, l, *(list(x) + list(y)))
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13 * np.abs(want).max())
    np.testing.assert_array_equal(w.k.params, [1.7, 0.9])          # a pure function: the nested kernel keeps its own parameters


# ---- the numpy closed form against the reference --------------------------------------------------------------------------------
def test_fixture_matches_generator_inputs(golden):
    for case in CASES:
        p = _pairs(golden, case)
        xi, xj, ni, nj = G20.pair_data(case)
        for key, v in (("xi", xi), ("xj", xj), ("ni", ni), ("nj", nj), ("params", G20.case_params(case))):
            np.testing.assert_array_equal(p[key], v, err_msg="%s %s" % (case, key))
        assert (p["xi"] == p["xj"]).sum() >= 10 and (~G20.inside(p["xi"])).sum() == 4
        for xg in G20.CASES[case][0]:
            assert (p["xi"] == xg).any()
    w = _pairs(golden, "m5wide")
    assert np.isnan(w["k"]).any() and (w["l"] < 0).any()          # the NaN classes are in the fixture


@pytest.mark.parametrize("case", CASES)
def test_gpwarp_matches_reference(golden, case):
    p = _pairs(golden, case)
    k = G20.gp_kernel(g, case)
    l, dl = k.l_func(p["xi"], 0, *p["params"][1:]), k.l_func(p["xi"], 1, *p["params"][1:])
    for name, got, want in (("l", l, p["l"]), ("l'", dl, p["dl"])):
        scale = np.abs(want).max()
        print("%s %s: worst relative deviation %.3g, worst as a fraction of the largest value %.3g"
              % (case, name, np.abs(got / want - 1).max(), np.abs(got - want).max() / scale))
        assert_close_nan(got, want, rtol=LFUNC_RTOL, atol_scale=LFUNC_ATOL_SCALE, msg="%s %s" % (case, name))
    assert l.shape == p["xi"].shape and k.l_func(p["xi"][:, None], 0, *p["params"][1:]).shape == (len(p["xi"]), 1)


@pytest.mark.parametrize("case", CASES)
def test_host_pairs_match_reference(golden, case):
    """The CPU statement of the kernel -- GibbsKernel1d around GPWarp, what the device is compared with -- against the reference."""
    p = _pairs(golden, case)
    m = len(G20.CASES[case][0])
    kh = GibbsKernel1d(GPWarp(m, k=G20.nested_se(g, float(p["sigma_n"]))), num_params=2 * m + 2, initial_params=p["params"],
                       param_bounds=[(-10.0, 10.0)] * (2 * m + 2))
    got = kh(p["xi"][:, None], p["xj"][:, None], p["ni"][:, None], p["nj"][:, None])
    ins = G20.inside(p["xi"]) & G20.inside(p["xj"])
    for a in (0, 1):
        for b in (0, 1):
            sel = (p["ni"] == a) & (p["nj"] == b)
            assert sel.any()
            assert_pairs(got[sel], p["k"][sel], ins[sel], msg="%s class %d%d" % (case, a, b))


def test_nested_amplitude_cancels():
    x, l, y, _ = G20.CASES["m12"]
    X = np.linspace(0.0, 2.0, 101)
    a = GPWarp(12, k=G20.nested_se(g, 1.0))(X, 0, l, *(list(x) + list(y)))
    b = GPWarp(12, k=G20.nested_se(g, 2.5))(X, 0, l, *(list(x) + list(y)))
    np.testing.assert_allclose(a, b, rtol=1e-12)
    np.testing.assert_allclose(GPWarp(12, k=G20.nested_se(g))(np.asarray(x), 0, l, *(list(x) + list(y))), y, rtol=1e-12)      # it interpolates


def test_slope_is_derivative():
    X = np.linspace(-0.2, 2.2, 97) + 1e-3
    h = 1e-6
    for case in CASES:
        k = G20.gp_kernel(g, case)
        p = k.params[1:]
        fd = (k.l_func(X + h, 0, *p) - k.l_func(X - h, 0, *p)) / (2 * h)
        np.testing.assert_allclose(k.l_func(X, 1, *p), fd, rtol=1e-6, atol=1e-8, err_msg=case)


def test_duplicated_point_never_gives_stale_numbers():
    """x_2 = x_3 with different values: the nested matrix factors only by the 1e2 eps on its diagonal (pivot sqrt(2e2 eps)), which
    GPWarp refuses -- LinAlgError or non-finite values, never the numbers of the call before.  So does a location that is NaN."""
    k = G20.gp_kernel(g, "m5")
    X = np.linspace(0.0, 2.0, 9)
    good = k.l_func(X, 0, *k.params[1:])
    assert np.isfinite(good).all()
    for value in (k.params[4], k.params[4] + 1e-9, np.nan):          # exactly coincident, coincident to 2e-9 l, NaN
        bad = np.array(k.params[1:])
        bad[2] = value
        for n in (0, 1):
            try:
                got = k.l_func(X, n, *bad)
            except np.linalg.LinAlgError:
                got = None
            assert got is None or not np.isfinite(got).all()
        q = np.array(k.params)
        q[3] = value
        k2 = G20.gp_kernel(g, "m5")
        k2.params = q
        with pytest.raises(np.linalg.LinAlgError):
            k2._native_params()
        with pytest.raises(np.linalg.LinAlgError):
            g.GaussianProcess(k2)._native_terms()       # (update_hyperparameters turns that into +inf: tests/test_gpu_gibbs_gp.py)
    # the rule is far from the matrices an optimiser meets: points 1e-3 l apart with equal values still evaluate
    near = np.array(k.params[1:])
    near[2] = near[3] - 1e-3 * near[0]
    near[7] = near[8]
    assert np.isfinite(k.l_func(X, 0, *near)).all()
    np.testing.assert_array_equal(k.l_func(X, 0, *k.params[1:]), good)


def test_native_subclass_with_another_nested_kernel_is_refused_not_miscomputed():
    """The switch to the host class is made for GibbsKernel1dGP itself.  A user subclass that keeps the native __call__ with a
    nested kernel the device does not carry must not send squared-exponential weights under id 13: ValueError."""
    class Native(g.GibbsKernel1dGP):
        pass
    m52 = g.Matern52Kernel(initial_params=[1.0, 0.5], fixed_params=[True, False], param_bounds=[(0, 10)] * 2)
    for nested in (m52, g.SquaredExponentialKernel(initial_params=[1.0, 0.5], param_bounds=[(0, 10)] * 2)):
        k = Native(3, k=nested, param_bounds=[(0, 10)] * (7 + nested.num_free_params))
        assert type(k).__call__ is g.Kernel.__call__
        with pytest.raises(ValueError, match="nested 1-D SquaredExponentialKernel"):
            k._native_params()
        with pytest.raises(ValueError, match="nested 1-D SquaredExponentialKernel"):
            g.GaussianProcess(k)._native_terms()
    with pytest.raises(ValueError, match="closed form"):
        GPWarp(3, k=m52).weights(0.5, 0.0, 1.0, 2.0, 0.5, 0.6, 0.7)
    ok = Native(3, k=G20.nested_se(g), initial_params=[1.0, 0.5, 0.0, 1.0, 2.0, 0.5, 0.6, 0.7], param_bounds=[(0, 10)] * 8)
    assert len(ok._native_params()) == 8
    with pytest.raises(TypeError, match="k must be an instance of type Kernel!"):
        g.GibbsKernel1dGP(3, k="se")


class _FakeContext(object):
    """Stands in for the library's context: records what the batched routes hand over and answers, per element, with that
    element's sigma_f -- so a mis-indexed row would show."""
    _warp_key = None

    def __init__(self):
        self.batches = []

    def set_data(self, X, n):
        pass

    def set_warp(self, layers):
        pass

    def set_option(self, key, value):
        pass

    def mem_info(self):
        return (1 << 40, 1 << 40)

    def release_batch_scratch(self):
        pass

    def fit_batch_terms(self, terms_list, noise_var, y, err_y, diag_add):
        self.sigmas = np.array([t[0][1][0] for t in terms_list])
        self.batches.append(self.sigmas)
        return self.sigmas.copy(), np.zeros(len(terms_list)), np.zeros(len(terms_list), dtype=int)

    def predict_batch(self, Xs, ns, keep, noise_n=None, want_var=True, want_cov=False, want_cov_sum=False):
        M = len(Xs)
        mean = self.sigmas[:, None] * np.ones((1, M))
        return mean, (mean.copy() if want_var else None), None, None


def _gp_and_rows():
    """The m5 fit model and four rows of free parameters with different sigma_f; row 1 has x_2 = x_3 (its weights do not solve)."""
    gp = G20.make_fit_gp(g, G20.fit_data())
    base = np.array(gp.free_params[:], dtype=float)
    rows = []
    for i in range(4):
        q = base.copy()
        q[0] = 1.0 + 0.25 * i
        rows.append(q)
    rows[1][3] = rows[1][4]
    gp._ctx_obj = _FakeContext()
    return gp, base, rows


def test_ll_batch_drops_a_row_whose_weights_do_not_solve():
    gp, base, rows = _gp_and_rows()
    out = gp.ll_batch(rows)
    assert len(gp._ctx.batches) == 1
    np.testing.assert_array_equal(gp._ctx.batches[0], [1.0, 1.5, 1.75])          # rows 0, 2, 3 reached the library, in order
    assert out[1] == -np.inf and np.isfinite(out[[0, 2, 3]]).all()
    np.testing.assert_allclose(out[[2, 3]] - out[0], [0.5, 0.75], rtol=0, atol=1e-12)      # each row got ITS element's answer
    np.testing.assert_array_equal(gp.free_params[:], base)


def test_compute_from_mcmc_drops_a_row_whose_weights_do_not_solve():
    gp, base, rows = _gp_and_rows()
    Xs = np.linspace(0.1, 1.9, 7)
    out = gp.compute_from_MCMC(Xs, flat_trace=np.array(rows), return_std=True)
    np.testing.assert_array_equal(gp._ctx.batches[0], [1.0, 1.5, 1.75])
    assert len(out["mean"]) == 3                                                  # row 1 is dropped, nothing shifts
    for got, want in zip(out["mean"], [1.0, 1.5, 1.75]):
        np.testing.assert_array_equal(got, np.full(7, want))
    np.testing.assert_array_equal(gp.free_params[:], base)


def test_compute_l_from_mcmc():
    d = G20.fit_data()
    gp = G20.make_fit_gp(g, d)
    base = np.array(gp.k.params)
    rs = np.random.RandomState(3)
    trace = np.array([np.concatenate((base * (1.0 + 0.05 * rs.rand(len(base))), [0.0] * (len(gp.free_params) - len(base))))
                      for _ in range(3)])
    X = np.linspace(0.0, 2.0, 11)
    for n in (0, 1):
        got = gp.compute_l_from_MCMC(X, n=n, flat_trace=trace)
        assert got.shape == (3, 11)
        for row, t in zip(got, trace):
            np.testing.assert_array_equal(row, gp.k.l_func(X, n, *t[1:len(base)]))
    np.testing.assert_array_equal(gp.k.params, base)


# ---- the device's length-scale function, compiled for the CPU -------------------------------------------------------------------
@pytest.fixture(scope="module")
def gibbs_gp_host():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gptools_amd", "csrc")
    subprocess.run(["make", "-C", here, "gibbs_host"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(here, "build", "libgibbs_host.so"))
    dp = ctypes.POINTER(ctypes.c_double)
    lib.gpt_host_gibbs_gp.restype = ctypes.c_int
    lib.gpt_host_gibbs_gp.argtypes = [dp, ctypes.c_int, dp, ctypes.c_long, dp, dp]

    def call(p, m, x):
        p = np.ascontiguousarray(p, dtype=float)
        x = np.ascontiguousarray(x, dtype=float)
        l, dl = np.empty_like(x), np.empty_like(x)
        rc = lib.gpt_host_gibbs_gp(p.ctypes.data_as(dp), int(m), x.ctypes.data_as(dp), len(x), l.ctypes.data_as(dp), dl.ctypes.data_as(dp))
        return rc, l, dl
    return call


@pytest.mark.parametrize("case", CASES + ["m1"])
def test_device_length_scale_function_against_numpy(golden, gibbs_gp_host, case):
    if case == "m1":
        k = g.GibbsKernel1dGP(1, k=G20.nested_se(g), initial_params=[1.0, 0.6, 0.9, 0.7], param_bounds=[(0, 10)] * 4)
        x = np.concatenate((np.linspace(-1.0, 3.0, 201), [0.9]))
    else:
        p = _pairs(golden, case)
        k = G20.gp_kernel(g, case)
        x = np.concatenate((p["xi"], p["xj"]))
    m = k.l_func.npts
    rc, l, dl = gibbs_gp_host(k._native_params()[1:], m, x)
    assert rc == 0
    want_l, want_dl = k.l_func(x, 0, *k.params[1:]), k.l_func(x, 1, *k.params[1:])
    assert_close_nan(l, want_l, rtol=LFUNC_RTOL, atol_scale=LFUNC_ATOL_SCALE, msg=case + " l")
    assert_close_nan(dl, want_dl, rtol=LFUNC_RTOL, atol_scale=LFUNC_ATOL_SCALE, msg=case + " l'")
    assert gibbs_gp_host(k._native_params()[1:], _lib.GIBBS_MAX_GP_POINTS + 1, x)[0] == -1
