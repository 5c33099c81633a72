"""The spline module and the kernels built on it, on the host (no GPU): ``spev`` against the reference's tables, ``BSplineWarp`` and
the host route ``GibbsKernel1d(BSplineWarp())`` against the reference's pair lists, ``ISplineWarp`` / ``ISplineWarpedKernel``
(tests/golden/g18_gibbs_bspline.npz, from tests/golden/gen_g18_gibbs_bspline.py), the class surface of ``GibbsKernel1dBSpline``,
and the device's B-spline length scale (csrc/gibbs_lfunc.hpp: gpt_gibbs_bspline) compiled for the CPU against the numpy one."""
import copy
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, assert_close_nan

sys.path.insert(0, GOLDEN)
import gen_g18_gibbs_bspline as G18      # noqa: E402

import gptools_amd as g                  # noqa: E402
from gptools_amd import _lib             # noqa: E402
from gptools_amd.kernel.gibbs import BSplineWarp, GibbsKernel1d      # noqa: E402
from gptools_amd.kernel.warping import ISplineWarp                   # noqa: E402
from gptools_amd.splines import spev                                 # noqa: E402

PAIR_CASES = sorted(G18.PAIR_CASES)
FORMS = (("B", {}), ("M", dict(M_spline=True)), ("I", dict(I_spline=True)))


def _pairs(golden, case):
    G = golden("g18_gibbs_bspline")
    return {k: G["pairs_%s__%s" % (case, k)] for k in ("xi", "xj", "ni", "nj", "params", "k")}


def _host_kernel(params, k=3):
    return GibbsKernel1d(BSplineWarp(k=k), num_params=len(params), initial_params=list(params),
                         param_bounds=[(-10.0, 10.0)] * len(params))


# ---- spev ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", sorted(G18.SPEV_GRIDS))
def test_spev_matches_reference_tables(golden, grid):
    """B, M and I forms, degrees 1 to 3, orders 0 .. deg + 1, at the knots, the boundaries and outside.  spev sums the basis
    functions in their order where the reference leaves the order to a matrix product: the project's pair-list tolerance."""
    G = golden("g18_gibbs_bspline")
    t, x = G["spev__t_" + grid], G["spev__x_" + grid]
    np.testing.assert_array_equal(t, G18.SPEV_GRIDS[grid])
    np.testing.assert_array_equal(x, G18.spev_x(t))
    for deg in (1, 2, 3):
        C = G["spev__C_%s_d%d" % (grid, deg)]
        np.testing.assert_array_equal(C, G18.spev_coeffs(grid, deg))
        for form, kw in FORMS:
            for n in range(deg + 2):
                want = G["spev_%s_%s_d%d_n%d" % (grid, form, deg, n)]
                with np.errstate(all="ignore"):
                    got = spev(t, C, deg, x, n=n, **kw)
                assert_close_nan(got, want, msg="%s %s deg %d n %d" % (grid, form, deg, n))
                if n > deg:
                    assert not got.any() and not want.any()
                elif form != "I" or n > 0:
                    # zero outside the knot range (the I-spline itself carries its constant and its integral beyond the last knot)
                    out = (x < t[0]) | (x > t[-1])
                    assert out.sum() >= 2 and not got[out].any()


def test_spev_fixture_holds_the_edge_points(golden):
    G = golden("g18_gibbs_bspline")
    for grid, t in G18.SPEV_GRIDS.items():
        x = G["spev__x_" + grid]
        assert len(x) == 60 and all((x == k).any() for k in t) and (x < t[0]).any() and (x > t[-1]).any()
    assert len(set(G18.SPEV_GRIDS["r"])) < len(G18.SPEV_GRIDS["r"])      # a repeated internal knot
    assert np.isfinite(G["spev_r_B_d3_n0"]).all() and np.isfinite(G["spev_r_B_d3_n1"]).all()


def test_spev_right_edge_and_partition_of_unity():
    t = np.array(G18.T6)
    x = np.concatenate((t, np.linspace(t[0], t[-1], 41)))
    for deg in (1, 2, 3):
        ones = np.ones(len(t) + deg - 1)
        np.testing.assert_allclose(spev(t, ones, deg, x), 1.0, rtol=0, atol=4e-16)      # the last knot included
        # the I-spline of the unit coefficient vector e_0 is the constant 1; every other one runs from 0 to 1
        for i in range(len(ones)):
            e = np.zeros(len(ones))
            e[i] = 1.0
            v = spev(t, e, deg, np.array([t[0], t[-1]]), I_spline=True)
            np.testing.assert_allclose(v, [1.0 if i == 0 else 0.0, 1.0], rtol=0, atol=1e-15)


def test_spev_covariance(golden):
    G = golden("g18_gibbs_bspline")
    var, cov = G18.spev_cov_inputs()
    np.testing.assert_array_equal(var, G["spev_cov1__var"])
    np.testing.assert_array_equal(cov, G["spev_cov2__cov_C"])
    x, C = G["spev__x_u"], G["spev__C_u_d3"]
    y, cy = spev(G18.T6, C, 3, x, cov_C=var)
    assert_close_nan(y, G["spev_cov1__y"])
    assert_close_nan(cy, G["spev_cov1__cov"])
    y, cy = spev(G18.T6, C, 3, x, cov_C=cov, I_spline=True, n=1)
    assert_close_nan(y, G["spev_cov2__y"])
    assert_close_nan(cy, G["spev_cov2__cov"])
    assert cy.shape == (60, 60)
    # an I-spline itself keeps the whole covariance, the constant's entries included: B cov B^T with the I-spline basis
    y0, c0 = spev(G18.T6, C, 3, x, cov_C=cov, I_spline=True)
    np.testing.assert_array_equal(y0, spev(G18.T6, C, 3, x, I_spline=True))
    basis = np.array([spev(G18.T6, e, 3, x, I_spline=True) for e in np.eye(len(C))]).T
    np.testing.assert_allclose(c0, basis.dot(cov).dot(basis.T), rtol=1e-13, atol=1e-15)
    _, c1 = spev(G18.T6, C, 3, x, cov_C=var, I_spline=True)
    np.testing.assert_allclose(c1, (basis * var).dot(basis.T), rtol=1e-13, atol=1e-15)


def test_spev_errors():
    x = np.linspace(0.0, 2.0, 5)
    with pytest.raises(ValueError, match="Knots must be in increasing order!"):
        spev([0.0, 1.0, 0.5, 2.0], np.ones(6), 3, x)
    with pytest.raises(ValueError, match=r"Length of C must be equal to M \+ deg - 1!"):
        spev([0.0, 0.5, 1.0, 2.0], np.ones(5), 3, x)
    np.testing.assert_array_equal(spev([0.0, 1.0, 0.5, 2.0][:2], np.ones(4), 3, x, n=4), np.zeros(5))


# ---- BSplineWarp and the host route --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PAIR_CASES)
def test_host_pairs_match_reference(golden, case):
    p = _pairs(golden, case)
    k = _host_kernel(p["params"])
    got = k(p["xi"][:, None], p["xj"][:, None], p["ni"][:, None], p["nj"][:, None])
    for a in (0, 1):
        for b in (0, 1):
            sel = (p["ni"] == a) & (p["nj"] == b)
            assert sel.any()
            assert_close_nan(got[sel], p["k"][sel], msg="%s class %d%d" % (case, a, b))


def test_fixture_matches_generator_inputs_and_holds_the_edge_cases(golden):
    w = BSplineWarp()
    for case in PAIR_CASES:
        p = _pairs(golden, case)
        xi, xj, ni, nj = G18.pair_data(case)
        for key, v in (("xi", xi), ("xj", xj), ("ni", ni), ("nj", nj), ("params", G18.PAIR_CASES[case])):
            np.testing.assert_array_equal(p[key], v, err_msg="%s %s" % (case, key))
        assert len(xi) == 1200 and (p["xi"] == p["xj"]).any()
        assert all(((p["ni"] == a) & (p["nj"] == b)).any() for a in (0, 1) for b in (0, 1))
    assert [G18.nt_of(G18.PAIR_CASES[c]) for c in ("nt2", "nt6", "nt11")] == [2, 6, _lib.GIBBS_MAX_KNOTS]
    assert G18.MAX_KNOTS == _lib.GIBBS_MAX_KNOTS
    for case in ("nt2", "nt6", "nt11", "rep", "knots"):
        assert np.isfinite(_pairs(golden, case)["k"]).all(), case
    assert _pairs(golden, "nt6")["params"][0] != 1.0
    rep = _pairs(golden, "rep")["params"][1:7]
    assert (np.diff(rep) == 0).sum() == 1 and np.diff(rep)[0] > 0 and np.diff(rep)[-1] > 0
    kn = _pairs(golden, "knots")
    for t in kn["params"][1:7]:
        assert (kn["xi"] == t).any() and (kn["xj"] == t).any()
    # outside the knots l = l' = 0: both points outside NaN; one outside 0 in the value class, NaN in the derivative classes
    out = _pairs(golden, "out")
    oi, oj = (out["xi"] < 0.0) | (out["xi"] > 2.0), (out["xj"] < 0.0) | (out["xj"] > 2.0)
    val = (out["ni"] == 0) & (out["nj"] == 0)
    assert (oi & oj).any() and np.isnan(out["k"][oi & oj]).all()
    assert ((oi ^ oj) & val).any() and not out["k"][(oi ^ oj) & val].any()
    assert ((oi ^ oj) & ~val).any() and np.isnan(out["k"][(oi ^ oj) & ~val]).all()
    assert np.isfinite(out["k"][~oi & ~oj]).all()
    neg = _pairs(golden, "neg")
    l = w(np.concatenate((neg["xi"], neg["xj"])), 0, *neg["params"][1:])
    assert (l < 0).any() and (l > 0).any() and np.isnan(neg["k"]).any() and np.isfinite(neg["k"]).any()


def test_zero_length_scale_rule_is_the_bspline_warps_alone():
    """Where a length scale is exactly zero the B-spline route gives NaN in the derivative classes (the reference's 0/0); a host
    kernel with another length-scale function keeps 0 * finite = 0 in the class that differentiates at the other point, the
    number it had and the number the older device kernels give."""
    def ramp(x, n, a):
        return np.maximum(a * x, 0.0) if n == 0 else np.where(x > 0.0, a, 0.0)
    k = GibbsKernel1d(ramp, initial_params=[1.0, 0.5], param_bounds=[(-10.0, 10.0)] * 2)
    xi, xj = np.array([[-0.5], [-0.5], [1.0], [-0.5]]), np.array([[1.0], [1.0], [-0.5], [1.0]])
    ni, nj = np.array([[0], [0], [1], [1]]), np.array([[0], [1], [0], [0]])
    with np.errstate(all="ignore"):
        got = k(xi, xj, ni, nj)
    assert got[0] == 0.0 and got[1] == 0.0 and got[2] == 0.0 and np.isnan(got[3])
    p = G18.PAIR_CASES["out"]
    with np.errstate(all="ignore"):
        got = _host_kernel(p)(xi, xj, ni, nj)
    assert got[0] == 0.0 and np.isnan(got[1:]).all()


def test_bspline_warp_surface():
    w = BSplineWarp()
    assert w.k == 3 and BSplineWarp(k=2).k == 2
    p = G18.PAIR_CASES["nt6"][1:]
    X = np.linspace(0.0, 2.0, 7)
    np.testing.assert_array_equal(w(X, 0, *p), spev(p[:6], p[6:], 3, X))
    np.testing.assert_array_equal(w(X, 1, *p), spev(p[:6], p[6:], 3, X, n=1))
    X2 = np.column_stack((X, 5.0 + X))                      # the first column of a 2-D X, in X's shape
    assert w(X2[:, :1], 0, *p).shape == (7, 1)
    np.testing.assert_array_equal(w(X2[:, :1], 0, *p)[:, 0], w(X, 0, *p))
    # at the boundary knots the spline takes the first and the last coefficient; outside it is zero with a zero slope
    np.testing.assert_allclose(w(np.array([0.0, 2.0]), 0, *p), [p[6], p[-1]], rtol=1e-15)
    for n in (0, 1):
        np.testing.assert_array_equal(w(np.array([-0.1, 2.1]), n, *p), [0.0, 0.0])
    with pytest.raises(ValueError, match="Knots must be in increasing order!"):
        w(X, 0, *([0.0, 0.7, 0.3, 1.1, 1.6, 2.0] + list(p[6:])))
    # another degree: nt from the parameter count
    p2 = [0.0, 1.0, 2.0] + [0.5, 0.7, 0.9, 0.4]
    np.testing.assert_array_equal(BSplineWarp(k=2)(X, 0, *p2), spev(p2[:3], p2[3:], 2, X))


def test_warp_slope_is_derivative():
    h = 1e-6
    w = BSplineWarp()
    for case in ("nt2", "nt6", "nt11", "rep", "neg"):
        p = G18.PAIR_CASES[case][1:]
        t = np.asarray(p[:G18.nt_of(G18.PAIR_CASES[case])])
        x = np.linspace(0.0, 2.0, 203)[1:-1]
        x = x[np.abs(x[:, None] - t[None, :]).min(axis=1) > 1e-3]      # off the knots
        fd = (w(x + h, 0, *p) - w(x - h, 0, *p)) / (2 * h)
        np.testing.assert_allclose(w(x, 1, *p), fd, rtol=1e-6, atol=1e-8, err_msg=case)


# ---- the I-spline warp -------------------------------------------------------------------------------------------------------------------
def test_isplinewarp_origin_and_monotone():
    for nt, k, args in ((4, 3, [0.0, 0.3, 0.6, 1.0, 0.5, 1.0, 0.8, 1.5, 0.7]), (3, 2, [-1.0, 0.0, 2.0, 0.4, 0.9, 0.2])):
        w = ISplineWarp(nt, k=k)
        t = np.asarray(args[:nt])
        x = np.linspace(t[0], t[-1], 101)
        v = w(x, 0, 0, *args)
        assert v[0] == 0.0                                   # w(t_1) = 0: the constant's coefficient is 0
        assert (np.diff(v) > 0).all()                         # positive coefficients: monotone
        np.testing.assert_allclose(v[-1], np.sum(args[nt:]), rtol=1e-14)      # every I-spline reaches 1 at the last knot
        assert (w(x, 0, 1, *args) >= 0).all()
        xm = x[1:-1][np.abs(x[1:-1, None] - t[None, :]).min(axis=1) > 1e-3]
        h = 1e-6
        np.testing.assert_allclose(w(xm, 0, 1, *args), (w(xm + h, 0, 0, *args) - w(xm - h, 0, 0, *args)) / (2 * h), rtol=1e-6)
    # dimension 1 of a warp with 4 and 3 knots reads its own block of the parameters
    w = ISplineWarp(G18.ISW_NT)
    x = np.linspace(0.0, 1.0, 9)
    np.testing.assert_array_equal(w(x, 1, 0, *G18.ISW_W_PARAMS), ISplineWarp(3)(x, 0, 0, *G18.ISW_W_PARAMS[9:]))


def test_isplinewarped_kernel_warp_matches_reference(golden):
    G = golden("g18_gibbs_bspline")
    k = G18.isw_kernel(g)
    Xi, Xj, ni, nj = G18.isw_data()
    for key, v in (("Xi", Xi), ("Xj", Xj), ("ni", ni), ("nj", nj)):
        np.testing.assert_array_equal(G["isw__" + key], v)
    assert k.num_params == 3 + 16 and isinstance(k, g.WarpedKernel)
    assert list(k.param_names)[3:8] == ["t_{0,1}", "t_{0,2}", "t_{0,3}", "t_{0,4}", "C_{0,1}"]
    assert list(k.param_names)[12:16] == ["t_{1,1}", "t_{1,2}", "t_{1,3}", "C_{1,1}"]
    assert ((ni.sum(axis=1) + nj.sum(axis=1)) > 1).any() and (Xi[20:24, 0] == G18.ISW_W_PARAMS[:4]).all()
    # the warp and its derivatives per dimension (the pair list itself needs the inner kernel's device: tests/test_gpu_gibbs_bspline.py)
    for d in (0, 1):
        for n in (0, 1, 2):
            assert_close_nan(k.w(Xi[:, d], d, n), G["isw__w%d_n%d" % (d, n)], msg="dimension %d order %d" % (d, n))
        np.testing.assert_array_equal(k.w_func(Xi[:, d], d, 1), k.w(Xi[:, d], d, 1))
    with pytest.raises(ValueError) as e:
        k(Xi[:2], Xj[:2], 2 * np.ones((2, 2), dtype=int), nj[:2])
    assert str(e.value) == str(G["isw__order2_error"])
    # nt: one int for every dimension, or one per dimension
    se = g.SquaredExponentialKernel(num_dim=2, param_bounds=[(0, 1)] * 3)
    k1 = g.ISplineWarpedKernel(se, 3, param_bounds=[(0, 1)] * 14)
    assert k1.num_params == 3 + 2 * (3 + 4) and list(k1.w.fun.nt) == [3, 3] and k1.w.fun.k == 3
    assert g.ISplineWarpedKernel(se, 3, k_deg=2, param_bounds=[(0, 1)] * 12).num_params == 3 + 2 * (3 + 3)
    with pytest.raises(ValueError, match="nt must have length equal to k.num_dim!"):
        g.ISplineWarpedKernel(se, [3, 3, 3], param_bounds=[(0, 1)] * 21)
    # a host kernel: no device model, the Python-kernel route
    assert g.GaussianProcess(k)._native_terms() is None


# ---- the class surface -------------------------------------------------------------------------------------------------------------------
def test_names_counts_and_device_eligibility():
    assert _lib.KERNEL_GIBBS_BSPLINE == 12 and _lib.GIBBS_MAX_KNOTS == 11
    k = g.GibbsKernel1dBSpline(3, param_bounds=[(0, 1)] * 9)
    assert type(k) is g.GibbsKernel1dBSpline and k.num_params == 9 and k._gpt_kernel_id == _lib.KERNEL_GIBBS_BSPLINE
    assert list(k.param_names) == [r"\sigma_f", "t_{1}", "t_{2}", "t_{3}", "C_{1}", "C_{2}", "C_{3}", "C_{4}", "C_{5}"]
    assert isinstance(k.l_func, BSplineWarp) and k.l_func.k == 3 and type(k).__call__ is g.Kernel.__call__
    for nt in (2, _lib.GIBBS_MAX_KNOTS):
        k = g.GibbsKernel1dBSpline(nt, param_bounds=[(0, 1)] * (2 * nt + 3))
        assert type(k) is g.GibbsKernel1dBSpline and k.num_params == 2 * nt + 3
        assert g.GaussianProcess(k)._native_terms() is not None
    with pytest.raises(ValueError, match="only supports 1d"):
        g.GibbsKernel1dBSpline(3, num_dim=2)
    for name in ("GibbsKernel1dBSpline", "BSplineWarp", "ISplineWarp", "ISplineWarpedKernel"):
        assert hasattr(g, name) and hasattr(g.kernel, name)
    assert g.splines.spev is spev
    # another degree, or more knots than the device kernel carries: a host subclass with the same numbers
    rs = np.random.RandomState(7)
    xi, xj = rs.uniform(0, 2, (50, 1)), rs.uniform(0, 2, (50, 1))
    ni, nj = rs.randint(0, 2, (50, 1)), rs.randint(0, 2, (50, 1))
    nt12 = _lib.GIBBS_MAX_KNOTS + 1
    p12 = [1.2] + list(np.linspace(0.0, 2.0, nt12)) + list(rs.uniform(0.3, 1.0, nt12 + 2))
    p2 = [0.9] + G18.T6 + G18.C6[:7]
    for nt, deg, p in ((nt12, 3, p12), (6, 2, p2), (1, 3, None)):
        k = g.GibbsKernel1dBSpline(nt, k=deg, param_bounds=[(-10, 10)] * (2 * nt + deg))
        assert isinstance(k, g.GibbsKernel1dBSpline) and type(k) is not g.GibbsKernel1dBSpline
        assert type(k).__call__ is GibbsKernel1d.__call__ and k.num_params == 2 * nt + deg and k.l_func.k == deg
        assert g.GaussianProcess(k)._native_terms() is None
        assert (k * g.SquaredExponentialKernel(num_dim=1, param_bounds=[(0, 1)] * 2))._native_factors() is None
        if p is not None:
            k.set_hyperparams(np.array(p))
            np.testing.assert_array_equal(k(xi, xj, ni, nj), _host_kernel(p, k=deg)(xi, xj, ni, nj))
            k2 = pickle.loads(pickle.dumps(k))
            assert type(k2) is type(k) and k2.l_func.k == deg
            np.testing.assert_array_equal(k2.params, k.params)

    # a user subclass keeps the native route whatever it asks for (the library refuses beyond the cap), like the exp-Gauss rule
    class Mine(g.GibbsKernel1dBSpline):
        pass
    assert type(Mine(nt12, param_bounds=[(0, 1)] * (2 * nt12 + 3))) is Mine


def test_pickle_and_copy_round_trip(golden):
    G = golden("g18_gibbs_bspline")
    td = {k[len("terms__"):]: v for k, v in G.items() if k.startswith("terms__")}
    gp = G18.make_terms_gp(g, "sum_se", td)
    for gp2 in (pickle.loads(pickle.dumps(gp)), copy.deepcopy(gp)):
        k1, k2 = gp.k.k1, gp2.k.k1
        assert type(k2) is type(k1) and k2._gpt_kernel_id == k1._gpt_kernel_id and k2.l_func.k == 3
        np.testing.assert_array_equal(gp2.k.params, gp.k.params)
        assert list(k2.param_names) == list(k1.param_names)
        np.testing.assert_array_equal(gp2.X, gp.X)
        assert gp2._native_terms() is not None and [t[0] for t in gp2._native_terms()] == [t[0] for t in gp._native_terms()]
    k = copy.copy(gp.k.k1)
    assert type(k) is g.GibbsKernel1dBSpline and k.num_params == 15


# ---- the device's length-scale function, compiled for the CPU --------------------------------------------------------------------------
# Both sides are the same double-precision expressions in the same order (no contraction on either side): the Cox-de Boor triangle
# above x's span term by term, the sum over the basis functions left to right.  They agree to the bit on this machine; the bound
# leaves room for a compiler that orders a commutative product differently.
@pytest.fixture(scope="module")
def bspline_host():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gptools_amd", "csrc")
    subprocess.run(["make", "-C", here, "gibbs_host"], check=True, stdout=subprocess.DEVNULL)
    L = ctypes.CDLL(os.path.join(here, "build", "libgibbs_host.so"))
    dp = ctypes.POINTER(ctypes.c_double)
    L.gpt_host_gibbs_bspline.restype = ctypes.c_int
    L.gpt_host_gibbs_bspline.argtypes = [dp, ctypes.c_int, dp, ctypes.c_long, dp, dp]

    def run(params, x):
        p = np.ascontiguousarray(params[1:], dtype=float)
        x = np.ascontiguousarray(x, dtype=float)
        l, dl = np.empty_like(x), np.empty_like(x)
        rc = L.gpt_host_gibbs_bspline(p.ctypes.data_as(dp), G18.nt_of(params), x.ctypes.data_as(dp), len(x), l.ctypes.data_as(dp),
                                      dl.ctypes.data_as(dp))
        assert rc == 0
        return l, dl
    run.lib = L
    return run


@pytest.mark.parametrize("case", PAIR_CASES)
def test_device_length_scale_function_against_numpy(golden, bspline_host, case):
    p = _pairs(golden, case)
    w = BSplineWarp()
    x = np.concatenate((p["xi"], p["xj"], np.linspace(-0.5, 2.5, 10000)))
    l, dl = bspline_host(p["params"], x)
    want_l, want_dl = w(x, 0, *p["params"][1:]), w(x, 1, *p["params"][1:])
    for got, want in ((l, want_l), (dl, want_dl)):
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_array_equal(got == 0.0, want == 0.0)
    assert (want_l == 0.0).sum() > 3000 and (want_l != 0.0).sum() > 6000        # the sweep leaves the knot range on both sides
    nz = want_l != 0.0
    print("%s: l max rel dev %.3g, l' max abs dev / max|l'| %.3g" % (
        case, np.max(np.abs(l[nz] - want_l[nz]) / np.abs(want_l[nz])), np.abs(dl - want_dl).max() / np.abs(want_dl).max()))
    np.testing.assert_allclose(l, want_l, rtol=1e-14, atol=0)
    np.testing.assert_allclose(dl, want_dl, rtol=0, atol=1e-14 * np.abs(want_dl).max())
    t = p["params"][1:1 + G18.nt_of(p["params"])]
    lk, _ = bspline_host(p["params"], np.array([t[0], t[-1]]))
    if case != "neg":
        np.testing.assert_allclose(lk, [p["params"][1 + len(t)], p["params"][-1]], rtol=1e-15)      # first / last coefficient


def test_device_function_refuses_knot_counts_beyond_the_cap(bspline_host):
    dp = ctypes.POINTER(ctypes.c_double)
    buf = np.zeros(64)
    for nt in (1, _lib.GIBBS_MAX_KNOTS + 1):
        assert bspline_host.lib.gpt_host_gibbs_bspline(buf.ctypes.data_as(dp), nt, buf.ctypes.data_as(dp), 1, buf.ctypes.data_as(dp),
                                                       buf.ctypes.data_as(dp)) == -1
