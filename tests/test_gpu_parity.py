"""GPU suite (-m gpu): the HIP path, called through the C ABI (gptools_amd._lib -> libgpt_hip.so) and
through the reference-shaped GaussianProcess / Kernel API, against
  (1) the committed golden vectors generated from the reference (tests/golden/*.npz),
  (2) the CPU oracle (oracle/) on seeded inputs at sizes it finishes in seconds,
  (3) size-independent properties at BASELINE.json's full sizes.
Tolerances (fp64): K entries 1e-12 relative (+1e-13 of the matrix scale); log|K| 1e-10; LML 1e-8
relative (north_star), tightened to 1e-9 on the fixtures; predictive mean/variance 1e-6 of sigma_f^2.
"""
import sys
import warnings

import gc
import os

import numpy as np
import pytest

from conftest import assert_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("se", "m52")
KID = {"se": 0, "m52": 1}
EPS = sys.float_info.epsilon


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


@pytest.fixture(scope="module")
def ctx():
    from gptools_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def make_kernel(g, kern, d, params, **kw):
    cls = g.SquaredExponentialKernel if kern == "se" else g.Matern52Kernel
    kw.setdefault("param_bounds", [(0.0, 1e3)] * (d + 1))
    return cls(num_dim=d, initial_params=list(params), **kw)


@pytest.mark.parametrize("d", [1, 3])
def test_m52_pairs_over_the_whole_range_of_r(g, oracle, d):
    """The Matern-5/2 builder carries its own exp(-x) and 1/sqrt (kpair.hpp: exp_neg, v_rsq + Newton): every derivative
    class against the oracle from r = 1e-150 to the underflow of exp(-sqrt5 r) and beyond (the clamp at x = 800), with
    coincident points, denormal distances and non-finite inputs mixed in.  Tolerance where the oracle's value is normal:
    1e-13 + 1e-15 x relative, x = sqrt5 r -- exp(-x) turns the rounding of its own argument (a few ulp of x on either
    side) into a relative error of that many ulp TIMES x, for the library exp as for this one (matern.c:61-186 restated
    in oracle/gpt_oracle.c; the reference's own C code when oracle/_ref exists)."""
    rs = np.random.RandomState(77 + d)
    M = 6000
    ell = np.array([0.7, 1.3, 0.4])[:d]
    p = np.concatenate([[1.7], ell])
    Xi = rs.rand(M, d)
    # distances log-uniform over 1e-150 .. 1e4 length scales, random direction
    u = rs.randn(M, d)
    u /= np.sqrt((u * u).sum(1))[:, None]
    r = 10.0 ** rs.uniform(-150, 4, M)
    r[:200] = 10.0 ** rs.uniform(1.8, 2.8, 200)          # around the underflow of exp(-sqrt5 r): r = 330 .. 360
    Xj = Xi + (r[:, None] * u) * ell
    Xj[200:260] = Xi[200:260]                            # coincident points
    ni = np.zeros((M, d), dtype=int)
    nj = np.zeros((M, d), dtype=int)
    cls = rs.randint(0, 4, M)
    for m in range(M):
        if cls[m] & 1:
            ni[m, rs.randint(d)] = 1
        if cls[m] & 2:
            nj[m, rs.randint(d)] = 1
    k = make_kernel(g, "m52", d, p)
    got = k(Xi, Xj, ni, nj)
    want = oracle.kpairs("m52", p, Xi, Xj, ni, nj)
    assert np.all(np.isfinite(want))
    normal = np.abs(want) > 1e-290
    x = np.sqrt(5.0 * (((Xi - Xj) / ell) ** 2).sum(1))
    tol = 1e-13 + 1e-15 * x
    # derivative x derivative pairs in DIFFERENT dimensions: the reference's own expression (matern.c:143-146, term1 +
    # term2) cancels to ~5 r^2 of its terms as r -> 0, so below r ~ 1e-7 its value IS rounding noise of size
    # eps * (5/3) sigma^2 / l_i l_j -- compared absolutely there
    atol = np.where(cls == 3, 4e-15 * p[0] ** 2 / ell.min() ** 2, 0.0)
    bad = normal & (np.abs(got - want) > tol * np.abs(want) + atol)
    assert not bad.any(), (np.where(bad)[0][:5], got[bad][:5], want[bad][:5], x[bad][:5])
    assert np.all(np.abs(got[~normal]) <= 1e-289)        # underflow region: both (sub)normal-small or zero
    if oracle.have_ref():
        ref = p[0] ** 2 * oracle.ref_matern52(Xi, Xj, ni, nj, p[1:] ** 2)
        nr = np.abs(ref) > 1e-290
        assert not (nr & (np.abs(got - ref) > tol * np.abs(ref) + atol)).any()
    # every lane of a wave in ONE class (the branch the K builder takes nearly everywhere) gives the same numbers
    for c in range(4):
        sel = np.where(cls == c)[0][:640]
        np.testing.assert_array_equal(k(Xi[sel], Xj[sel], ni[sel], nj[sel]), got[sel])
    # non-finite inputs propagate (the clamp of exp_neg must not hide a NaN)
    Xn = Xi[:8].copy()
    Xn[0, 0] = np.nan
    Xn[1, 0] = np.inf
    out = k(Xn, Xj[:8], ni[:8], nj[:8])
    assert np.isnan(out[0]) and (np.isnan(out[1]) or out[1] == 0.0)
    np.testing.assert_array_equal(out[2:], got[2:8])



# ---------------------------------------------------------------- G1: Kernel.__call__ ---------
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_g1_kernel_call_se(g, golden, d):
    G = golden("g1_pairs")
    p = G["se_d%d_params" % d]
    Xi, Xj, ni, nj = (G["se_d%d_%s" % (d, s)] for s in ("Xi", "Xj", "ni", "nj"))
    k = make_kernel(g, "se", d, p)
    assert_close(k(Xi, Xj, ni, nj), G["se_d%d_k" % d], rtol=1e-12, msg="k")
    assert_close(k(Xi, Xj, 0 * ni, 0 * nj), G["se_d%d_k0" % d], rtol=1e-12, msg="k0")
    assert_close(k(Xi, Xj, G["se_d%d_nih" % d], G["se_d%d_njh" % d]), G["se_d%d_kh" % d], rtol=1e-10, msg="orders<=8")
    for hd in range(d + 1):
        assert_close(k(Xi, Xj, ni, nj, hyper_deriv=hd), G["se_d%d_hd%d" % (d, hd)], rtol=1e-9, msg="hd %d" % hd)
        assert_close(k(Xi, Xj, 0 * ni, 0 * nj, hyper_deriv=hd), G["se_d%d_k0_hd%d" % (d, hd)], rtol=1e-12)


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_g1_kernel_call_m52(g, golden, oracle, d):
    G = golden("g1_pairs")
    p = G["se_d%d_params" % d]
    Xi, Xj = G["se_d%d_Xi" % d], G["se_d%d_Xj" % d]
    ni, nj = G["m52_d%d_ni" % d], G["m52_d%d_nj" % d]
    k = make_kernel(g, "m52", d, p)
    got = k(Xi, Xj, ni, nj)
    assert_close(got, G["m52_d%d_k" % d], rtol=1e-12, msg="vs golden")
    if oracle.have_ref():      # the reference's own C code, compiled into oracle/_ref
        assert_close(got, p[0] ** 2 * oracle.ref_matern52(Xi, Xj, ni, nj, p[1:] ** 2), rtol=1e-12, msg="vs _ref")
    # exact r == 0 limits (matern.c:83-84,100-101,123-127)
    z = np.zeros((4, d))
    e0 = np.zeros((4, d), int)
    e0[:, 0] = 1
    assert np.array_equal(k(z, z, 0 * e0, 0 * e0), np.full(4, p[0] ** 2))
    assert np.array_equal(k(z, z, e0, 0 * e0), np.zeros(4))
    np.testing.assert_allclose(k(z, z, e0, e0), np.full(4, p[0] ** 2 * (5.0 / 3.0) / p[1] ** 2), rtol=1e-15)


def test_kernel_error_contract(g):
    k = make_kernel(g, "m52", 2, [1, 1, 1])
    X = np.zeros((3, 2))
    n0 = np.zeros((3, 2), int)
    n2 = n0.copy()
    n2[1, 0] = 2
    n11 = n0.copy()
    n11[2] = 1
    with pytest.raises(ValueError):
        k(X, X, n2, n0)
    with pytest.raises(ValueError):
        k(X, X, n0, n11)
    with pytest.raises(NotImplementedError):
        k(X, X, n0, n0, hyper_deriv=0)
    with pytest.raises(ValueError):
        k(X, X[:2], n0, n0)
    with pytest.raises(NotImplementedError):
        g.Kernel(num_dim=1, num_params=0)(X, X, n0, n0)
    nk = g.DiagonalNoiseKernel(num_dim=2, initial_noise=0.3, noise_bound=(0, 1))
    Xr = np.random.RandomState(0).rand(3, 2)
    np.testing.assert_array_equal(nk(Xr, Xr, n0, n0, symmetric=True), [0.09, 0.09, 0.09])
    np.testing.assert_array_equal(nk(Xr, Xr, n0, n0, symmetric=False), [0, 0, 0])
    np.testing.assert_array_equal(nk(Xr, Xr, n0, n11, symmetric=True), [0.09, 0.09, 0])
    np.testing.assert_allclose(nk(Xr, Xr, n0, n0, hyper_deriv=0, symmetric=True), [0.6] * 3)
    assert g.ZeroKernel(2)(Xr, Xr, n0, n0).tolist() == [0, 0, 0]


@pytest.mark.parametrize("l0", [0.0, 1e-310])
def test_se_zero_and_subnormal_length_scale(g, oracle, l0):
    """core.py:416: a 0 / 0 term of the scaled distance counts as 0, and a SUBNORMAL length scale (1 / l = inf as well)
    divides 0 / l = 0: coincident points give sigma_f^2, distinct ones exp(-inf) = 0 -- never NaN."""
    rs = np.random.RandomState(3)
    d = 2
    Xi = rs.rand(40, d)
    Xj = Xi.copy()
    Xj[::3] = rs.rand(len(Xj[::3]), d)            # a third of the pairs distinct in both dimensions
    Xj[1::3, 1] += 0.25                            # a third distinct in the dimension with the ordinary length scale only
    z = np.zeros((40, d), int)
    p = np.array([1.7, l0, 0.4])
    k = make_kernel(g, "se", d, p)
    got = k(Xi, Xj, z, z)
    assert np.all(np.isfinite(got))
    exp = np.where((Xi[:, 0] == Xj[:, 0]), p[0] ** 2 * np.exp(-0.5 * ((Xi[:, 1] - Xj[:, 1]) / p[2]) ** 2), 0.0)
    assert_close(got, exp, rtol=1e-13, msg="se, l_1 = %g" % l0)
    assert_close(got, oracle.kpairs("se", p, Xi, Xj, z, z), rtol=1e-13, msg="vs oracle")
    # ... and on the diagonal of a Gram matrix
    gp = g.GaussianProcess(k)
    K = gp.compute_Kij(Xi, None, z, None)
    assert np.all(np.isfinite(K)) and np.allclose(np.diag(K), p[0] ** 2, rtol=1e-15)


def test_kernel_call_ragged_and_empty(g, oracle):
    rs = np.random.RandomState(5)
    for kern in KERNELS:
        for M in (1, 63, 64, 65, 257, 1000):
            d = 3
            Xi, Xj = rs.rand(M, d), rs.rand(M, d)
            ni = (rs.rand(M, d) < 0.1).astype(int)
            ni[ni.sum(1) > 1] = 0
            nj = np.roll(ni, 1, axis=0)
            p = [1.2, 0.3, 0.5, 0.7]
            assert_close(make_kernel(g, kern, d, p)(Xi, Xj, ni, nj), oracle.kpairs(kern, p, Xi, Xj, ni, nj), rtol=1e-12)
    k = make_kernel(g, "se", 2, [1, 1, 1])
    assert k(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 2), int), np.zeros((0, 2), int)).shape == (0,)


# ---------------------------------------------------------------- G2: compute_Kij -------------
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("d", [1, 2, 3])
def test_g2_compute_Kij(g, golden, kern, d):
    G = golden("g2_gram")
    key = "%s_d%d_" % (kern, d)
    p, X, Xs, n, ns = (G[key + s] for s in ("params", "X", "Xs", "n", "ns"))
    gp = g.GaussianProcess(make_kernel(g, kern, d, p))
    assert_close(gp.compute_Kij(X, None, n, None), G[key + "K"], rtol=1e-12, msg="K")
    assert_close(gp.compute_Kij(X, Xs, n, ns), G[key + "Ks"], rtol=1e-12, msg="Ks")
    assert_close(gp.compute_Kij(Xs, None, ns, None), G[key + "Kss"], rtol=1e-12, msg="Kss")
    if kern == "se":
        for hd in range(d + 1):
            assert_close(gp.compute_Kij(X, None, n, None, hyper_deriv=hd), G[key + "K_hd%d" % hd], rtol=1e-9)
            assert_close(gp.compute_Kij(X, None, 0 * n, None, hyper_deriv=hd), G[key + "K0_hd%d" % hd], rtol=1e-12)
    else:
        with pytest.raises(NotImplementedError):
            gp.compute_Kij(X, None, n, None, hyper_deriv=0)


def test_g7_reference_test_matern(g, golden):
    """The reference's only unit test (tests/test_matern.py:4-31), seeded: 8 decimals vs mpmath."""
    G = golden("g7_test_matern")
    gp = g.GaussianProcess(make_kernel(g, "m52", 2, [10.0] + list(G["length_scales"])))
    K = gp.compute_Kij(G["X"], None, G["n"], None)
    np.testing.assert_array_almost_equal(K, G["K_arb"], decimal=8)
    assert_close(K, G["K_m52"], rtol=1e-12)


def test_python_plugin_kernel_still_works(g):
    """A user Kernel subclass written in Python goes through the pair-list path of compute_Kij."""
    class Lin(g.Kernel):
        def __call__(self, Xi, Xj, ni, nj, hyper_deriv=None, symmetric=False):
            return self.params[0] ** 2 * (Xi * Xj).sum(axis=1) + (1.0 if symmetric else 0.0)
    gp = g.GaussianProcess(Lin(num_dim=2, num_params=1, initial_params=[2.0], param_bounds=[(0, 10)]))
    X = np.random.RandomState(1).rand(5, 2)
    n = np.zeros((5, 2), int)
    np.testing.assert_allclose(gp.compute_Kij(X, None, n, None), 4.0 * X.dot(X.T) + 1.0)
    np.testing.assert_allclose(gp.compute_Kij(X, X[:3], n, n[:3]), 4.0 * X.dot(X[:3].T))
    gp.add_data(X, np.arange(5.0), err_y=0.3)
    gp.compute_K_L_alpha_ll()
    Kt = 4.0 * X.dot(X.T) + 1.0 + 0.09 * np.eye(5) + 1e2 * EPS * np.eye(5)
    np.testing.assert_allclose(gp.L, np.linalg.cholesky(Kt), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(gp.alpha.ravel(), np.linalg.solve(Kt, np.arange(5.0)), rtol=1e-10)


# ---------------------------------------------------------------- G8: rational-quadratic kernel
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_g8_rational_quadratic_kernel_call(g, golden, oracle, d):
    """RationalQuadraticKernel.__call__ on the device (kpair.hpp rq_pair) against the reference's outputs (golden g8:
    derivative orders 0..2 per point and dimension, combined order up to 6, alpha 1.7 / 2 / 0.35, tau == 0 rows) and
    against the CPU oracle on fresh random pairs with the largest supported combined order."""
    G = golden("g8_rq")
    for tag in "abc":
        key = "pairs_d%d%s_" % (d, tag)
        p = G[key + "params"]
        k = g.RationalQuadraticKernel(num_dim=d, initial_params=list(p), param_bounds=[(0.0, 1e3)] * (d + 2))
        got = k(G[key + "Xi"], G[key + "Xj"], G[key + "ni"], G[key + "nj"])
        assert_close(got, G[key + "k"], rtol=1e-11, atol_scale=1e-13, msg=key)
    rs = np.random.RandomState(80 + d)
    M = 300
    Xi, Xj = rs.rand(M, d), rs.rand(M, d)
    ni, nj = np.zeros((M, d), int), np.zeros((M, d), int)
    for tot in (8, 12, 16):                  # combined order exactly 8 / 12 / 16 (the device builder's limit), spread at random
        ni[:], nj[:] = 0, 0
        for m in range(M):
            for _ in range(tot):
                (ni if rs.rand() < 0.5 else nj)[m, rs.randint(d)] += 1
        assert_close(k(Xi, Xj, ni, nj), oracle.kpairs("rq", p, Xi, Xj, ni, nj), rtol=1e-10, atol_scale=1e-13, msg="order %d" % tot)
    ni[0, 0] += 1
    with pytest.raises(ValueError):          # beyond what the device builder carries
        k(Xi, Xj, ni, nj)
    with pytest.raises(NotImplementedError):  # ref: core.py:723-726
        k(Xi, Xj, 0 * ni, 0 * nj, hyper_deriv=1)


def test_g11_high_derivative_orders(g, golden, oracle):
    """Combined derivative orders 9 .. 12 of a pair (round 5: GPT_RQ_MAXORD 8 -> 16) against outputs of the reference itself
    (golden g11: the reference walks every set partition, minutes per pair at order 12): rational-quadratic, general-order
    Matern and the product SE * RQ.  The reference's Matern sums lose digits with the order (Bell polynomials of kvp with
    alternating signs): there the device is held to the oracle's closed form and to the reference at what it delivers."""
    G = golden("g11_high_orders")
    for d in (2, 3):
        key = "rq_d%d_" % d
        p = G[key + "params"]
        k = g.RationalQuadraticKernel(num_dim=d, initial_params=list(p), param_bounds=[(0.0, 1e3)] * (d + 2))
        got = k(G[key + "Xi"], G[key + "Xj"], G[key + "ni"], G[key + "nj"])
        assert_close(got, G[key + "k"], rtol=1e-9, atol_scale=1e-13, msg=key)
        assert_close(got, oracle.kpairs("rq", p, G[key + "Xi"], G[key + "Xj"], G[key + "ni"], G[key + "nj"]), rtol=1e-10, msg=key + "oracle")
    key = "matern_d2_"
    p = G[key + "params"]
    k = g.MaternKernel(num_dim=2, initial_params=list(p), param_bounds=[(0.0, 1e3)] * 4)
    got = k(G[key + "Xi"], G[key + "Xj"], G[key + "ni"], G[key + "nj"])
    assert_close(got, oracle.kpairs("matern", p, G[key + "Xi"], G[key + "Xj"], G[key + "ni"], G[key + "nj"]), rtol=1e-9, msg=key + "oracle")
    assert_close(got, G[key + "k"], rtol=1e-4, msg=key)
    key = "prod_d2_"
    k = (g.SquaredExponentialKernel(num_dim=2, initial_params=list(G["prod_d2_p1"]), param_bounds=[(0.0, 1e3)] * 3) *
         g.RationalQuadraticKernel(num_dim=2, initial_params=list(G["prod_d2_p2"]), param_bounds=[(0.0, 1e3)] * 4))
    got = k(G[key + "Xi"], G[key + "Xj"], G[key + "ni"], G[key + "nj"])
    assert_close(got, G[key + "k"], rtol=1e-9, atol_scale=1e-13, msg=key)


def test_g13_orders_13_to_16_against_mpmath(g, golden, oracle):
    """Combined derivative orders 13 .. 16 of a pair on the device (GPT_RQ_MAXORD = 16) against the independent 90-digit values of
    tests/golden/gen_g13_mpmath.py (multivariate Taylor arithmetic in mpmath; ADVICE r5: orders above 12 were held to the oracle
    only, which shares the device's regrouped sums): rational-quadratic, general-order Matern (nu = 0.6 .. 25, close points) and
    the product SE * RQ, 1e-9 relative; the oracle agrees with the same values to 1e-11 (CPU suite)."""
    G = golden("g13_high_orders_mpmath")
    for ci in range(int(G["ncases"])):
        key = "c%d_" % ci
        name, p = str(G[key + "kernel"]), G[key + "params"]
        d = G[key + "Xi"].shape[1]
        if name == "rq":
            k = g.RationalQuadraticKernel(num_dim=d, initial_params=list(p), param_bounds=[(0.0, 1e3)] * (d + 2))
        elif name == "matern":
            k = g.MaternKernel(num_dim=d, initial_params=list(p), param_bounds=[(0.0, 1e3)] * (d + 2))
        else:
            k = (g.SquaredExponentialKernel(num_dim=d, initial_params=list(p[:1 + d]), param_bounds=[(0.0, 1e3)] * (d + 1)) *
                 g.RationalQuadraticKernel(num_dim=d, initial_params=list(p[1 + d:]), param_bounds=[(0.0, 1e3)] * (d + 2)))
        got = k(G[key + "Xi"], G[key + "Xj"], G[key + "ni"], G[key + "nj"])
        assert_close(got, G[key + "k"], rtol=1e-9, atol_scale=0.0, msg=key + name)
    # one order beyond the limit is refused, not computed
    k = g.RationalQuadraticKernel(num_dim=2, initial_params=[1.0, 1.5, 0.5, 0.5], param_bounds=[(0.0, 1e3)] * 4)
    with pytest.raises(ValueError):
        k(np.array([[0.1, 0.2]]), np.array([[0.3, 0.5]]), np.array([[9, 0]]), np.array([[0, 8]]))


@pytest.mark.parametrize("d", [1, 2, 3])
def test_g10_matern_general_nu_pairs(g, golden, oracle, d):
    """General-order MaternKernel on the device (kpair.hpp matern_pair: Temme's K_nu, closed-form derivatives, the
    reference's behaviour at / near tau = 0) against fixtures generated by the reference (kernel/matern.py:251-465) and,
    at derivative orders where the reference's own sums lose digits, against the CPU oracle."""
    from conftest import assert_close_nan
    G = golden("g10_matern")
    for tag in "abcdefg":
        key = "pairs_d%d%s_" % (d, tag)
        p = G[key + "params"]
        k = g.MaternKernel(num_dim=d, initial_params=list(p), param_bounds=[(0.0, 1e3)] * (d + 2))
        got = k(G[key + "Xi"], G[key + "Xj"], G[key + "ni"], G[key + "nj"])
        assert_close_nan(got, G[key + "k"], rtol=5e-11, atol_scale=1e-13, msg=key)
        assert k.nu == p[1]
    rs = np.random.RandomState(100 + d)
    for nu in (0.8, 2.5, 3.0, 6.3):
        M = 300
        p = np.concatenate(([1.1, nu], 0.3 + 0.5 * rs.rand(d)))
        k = g.MaternKernel(num_dim=d, initial_params=list(p), param_bounds=[(0.0, 1e3)] * (d + 2))
        Xi, Xj = rs.rand(M, d), rs.rand(M, d)
        Xj[:20] = Xi[:20]
        Xj[20:40] = Xi[20:40] + 1e-3 * (rs.rand(20, d) - 0.5)
        ni, nj = np.zeros((M, d), int), np.zeros((M, d), int)
        for m in range(M):                       # combined order 0 .. 8, spread at random
            # (rows 20..39 lie in the reference's series region 0 < y <= 5e-4, where its one-term series adds terms of
            # size y^(nu - m) with alternating signs: beyond order 2 the sum is cancellation noise in ANY arithmetic)
            for _ in range(rs.randint(0, 3 if 20 <= m < 40 else 9)):
                (ni if rs.rand() < 0.5 else nj)[m, rs.randint(d)] += 1
        yv = 2.0 * nu * (((Xi - Xj) / p[2:]) ** 2).sum(axis=1)
        keep = (yv > 5e-4) | (yv == 0.0) | ((ni + nj).sum(axis=1) <= 2)      # (random rows can fall into that region too)
        assert keep.sum() > 280
        assert_close_nan(k(Xi, Xj, ni, nj)[keep], oracle.kpairs("matern", p, Xi, Xj, ni, nj)[keep], rtol=1e-9,
                         atol_scale=1e-12, msg="nu %g, orders <= 8" % nu)
    ni[0, 0] += 17
    with pytest.raises(ValueError):          # beyond what the device builder carries
        k(Xi, Xj, ni, nj)
    with pytest.raises(NotImplementedError):  # ref: core.py:723-726
        k(Xi, Xj, 0 * ni, 0 * nj, hyper_deriv=1)


def test_g10_matern_general_nu_gram_fit_predict(g, golden, oracle):
    G = golden("g10_matern")
    for d in (1, 2, 3):
        key = "gram_d%d_" % d
        p, X, Xs, n, ns = (G[key + s] for s in ("params", "X", "Xs", "n", "ns"))
        gp = g.GaussianProcess(g.MaternKernel(num_dim=d, initial_params=list(p), param_bounds=[(0.0, 1e3)] * (d + 2)))
        assert_close(gp.compute_Kij(X, None, n, None), G[key + "K"], rtol=5e-11, atol_scale=1e-13, msg=key + "K")
        assert_close(gp.compute_Kij(X, Xs, n, ns), G[key + "Ks"], rtol=5e-11, atol_scale=1e-13, msg=key + "Ks")
    for N, d in ((64, 2), (160, 3)):
        key = "fit_N%d_d%d_" % (N, d)
        p, X, y, n = (G[key + s] for s in ("params", "X", "y", "n"))
        k = g.MaternKernel(num_dim=d, initial_params=list(p), param_bounds=[(0.0, 1e3)] * (d + 2))
        gp = g.GaussianProcess(k, X=X, y=y, err_y=0.05, n=n)
        gp.compute_K_L_alpha_ll()
        assert gp._fast_fit_possible()              # the fused device path, not the pair-list fallback
        assert abs(gp.ll - G[key + "ll"]) <= 1e-9 * abs(G[key + "ll"])
        assert abs(np.log(np.diag(gp.L)).sum() - G[key + "logdet_half"]) <= 1e-10 * abs(G[key + "logdet_half"])
        mean, std = gp.predict(G[key + "Xs"], n=G[key + "ns"])
        np.testing.assert_allclose(mean, G[key + "mean"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(std ** 2, G[key + "std"] ** 2, rtol=0, atol=1e-6)
        # a new order nu through update_hyperparameters: same number as the CPU oracle
        p2 = p * np.array([1.1, 1.3] + [1.05] * d)
        negll = gp.update_hyperparameters(p2)
        ref = oracle.fit("matern", p2, X, n, y, 0.05 * np.ones(N))
        ll_ref = ref["ll_data"] + gp.hyperprior(gp.params)
        assert abs(-negll - ll_ref) <= 1e-9 * abs(ll_ref)
    # nu = 5/2: the same Gram matrix as the native Matern52Kernel
    key = "fit_N64_d2_"
    p, X, n = G[key + "params"], G[key + "X"], G[key + "n"]
    gp52 = g.GaussianProcess(g.Matern52Kernel(num_dim=2, initial_params=[p[0], p[2], p[3]], param_bounds=[(0.0, 1e3)] * 3))
    gpm = g.GaussianProcess(g.MaternKernel(num_dim=2, initial_params=list(p), param_bounds=[(0.0, 1e3)] * 4))
    assert_close(gpm.compute_Kij(X, None, n, None), gp52.compute_Kij(X, None, n, None), rtol=1e-10, atol_scale=1e-13)


def test_g8_rational_quadratic_gram_fit_predict(g, golden, oracle):
    G = golden("g8_rq")
    for d in (1, 2, 3):
        key = "gram_d%d_" % d
        p, X, Xs, n, ns = (G[key + s] for s in ("params", "X", "Xs", "n", "ns"))
        gp = g.GaussianProcess(g.RationalQuadraticKernel(num_dim=d, initial_params=list(p), param_bounds=[(0.0, 1e3)] * (d + 2)))
        assert_close(gp.compute_Kij(X, None, n, None), G[key + "K"], rtol=1e-11, atol_scale=1e-13, msg=key + "K")
        assert_close(gp.compute_Kij(X, Xs, n, ns), G[key + "Ks"], rtol=1e-11, atol_scale=1e-13, msg=key + "Ks")
    for N, d in ((64, 2), (200, 3)):
        key = "fit_N%d_d%d_" % (N, d)
        p, X, y, n = (G[key + s] for s in ("params", "X", "y", "n"))
        k = g.RationalQuadraticKernel(num_dim=d, initial_params=list(p), param_bounds=[(0.0, 1e3)] * (d + 2))
        gp = g.GaussianProcess(k, X=X, y=y, err_y=0.05, n=n)
        gp.compute_K_L_alpha_ll()
        assert gp._fast_fit_possible()              # the fused device path, not the pair-list fallback
        assert abs(gp.ll - G[key + "ll"]) <= 1e-9 * abs(G[key + "ll"])
        assert abs(np.log(np.diag(gp.L)).sum() - G[key + "logdet_half"]) <= 1e-10 * abs(G[key + "logdet_half"])
        assert_close(gp.alpha.ravel(), G[key + "alpha"], rtol=1e-6, atol_scale=1e-7, msg="alpha")
        mean, std = gp.predict(G[key + "Xs"], n=G[key + "ns"])
        np.testing.assert_allclose(mean, G[key + "mean"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(std ** 2, G[key + "std"] ** 2, rtol=0, atol=1e-6)
        # a new alpha through update_hyperparameters: same number as the CPU oracle
        p2 = p * np.array([1.1, 0.8] + [1.05] * d)
        negll = gp.update_hyperparameters(p2)
        ref = oracle.fit("rq", p2, X, n, y, 0.05 * np.ones(N))
        ll_ref = ref["ll_data"] + gp.hyperprior(gp.params)
        assert abs(-negll - ll_ref) <= 1e-9 * abs(ll_ref)
    # SumKernel of native terms including the new one stays on the device
    ks = g.SquaredExponentialKernel(num_dim=d, initial_params=[0.5, 0.4, 0.4, 0.4], param_bounds=[(0.0, 1e3)] * 4) + k
    gps = g.GaussianProcess(ks, X=X, y=y, err_y=0.05, n=n)
    gps.compute_K_L_alpha_ll()
    assert gps._fast_fit_possible()
    Kref = oracle.kbuild("se", [0.5, 0.4, 0.4, 0.4], X, n) + oracle.kbuild("rq", gp.k.params, X, n)
    assert_close(gps.K, Kref, rtol=1e-11, atol_scale=1e-13, msg="SE + RQ")


def test_g9_product_kernel_on_device_factors(g, golden):
    """k1 * k2 (ref: kernel/core.py:587-671) with both factors evaluated by the GPU pair list; K assembled from those
    calls, factorisation / solves / predict on the device."""
    G = golden("g9_product")
    mk = lambda cls, p: cls(num_dim=2, initial_params=list(p), param_bounds=[(0.0, 1e3)] * 3)
    k = mk(g.SquaredExponentialKernel, G["sese_p1"]) * mk(g.SquaredExponentialKernel, G["sese_p2"])
    assert_close(k(G["sese_Xi"], G["sese_Xj"], G["sese_ni"], G["sese_nj"]), G["sese_k"], rtol=1e-11, msg="SE * SE")
    k = mk(g.SquaredExponentialKernel, G["sese_p1"]) * mk(g.Matern52Kernel, G["sese_p2"])
    assert_close(k(G["sese_Xi"], G["sese_Xj"], G["sem_ni"], G["sem_nj"]), G["sem_k"], rtol=1e-11, msg="SE * M52")
    gp = g.GaussianProcess(k, X=G["fit_X"], y=G["fit_y"], err_y=0.05, n=G["fit_n"])
    gp.compute_K_L_alpha_ll()
    assert abs(gp.ll - G["fit_ll"]) <= 1e-9 * abs(G["fit_ll"])
    assert_close(gp.alpha.ravel(), G["fit_alpha"], rtol=1e-6, atol_scale=1e-7, msg="alpha")
    mean, std = gp.predict(G["fit_Xs"], n=G["fit_ns"])
    np.testing.assert_allclose(mean, G["fit_mean"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(std ** 2, G["fit_std"] ** 2, rtol=0, atol=1e-6)


# ---------------------------------------------------------------- G3/G4: fit + predict --------
FIT_CASES = [(k, N, d) for k in KERNELS for (N, d) in ((16, 1), (64, 2), (256, 3), (512, 2))]


@pytest.mark.parametrize("kern,N,d", FIT_CASES)
def test_g3_fit_g4_predict(g, golden, kern, N, d):
    G3, G4 = golden("g3_fit"), golden("g4_predict")
    key = "%s_N%d_d%d_" % (kern, N, d)
    p, X, y, n, err = (G3[key + s] for s in ("params", "X", "y", "n", "err_y"))
    gp = g.GaussianProcess(make_kernel(g, kern, d, p), X=X, y=y, err_y=err, n=n)
    gp.compute_K_L_alpha_ll()
    assert gp.K_up_to_date
    assert abs(gp.ll - G3[key + "ll"]) <= 1e-9 * abs(G3[key + "ll"])
    assert abs(np.log(np.diag(gp.L)).sum() - G3[key + "logdet_half"]) <= 1e-10 * abs(G3[key + "logdet_half"]) + 1e-10
    assert gp.alpha.shape == (N, 1)
    assert_close(gp.alpha.ravel(), G3[key + "alpha"], rtol=1e-6, atol_scale=1e-7, msg="alpha")
    if key + "L" in G3:
        assert_close(gp.L, G3[key + "L"], rtol=1e-7, atol_scale=1e-11, msg="L")
        assert np.array_equal(np.triu(gp.L, 1), np.zeros_like(gp.L))
    sf2 = p[0] ** 2
    Xs, ns = G4[key + "Xs"], G4[key + "ns"]
    mean, std = gp.predict(Xs, n=ns)
    np.testing.assert_allclose(mean, G4[key + "mean"], rtol=0, atol=1e-6 * sf2)
    np.testing.assert_allclose(std ** 2, G4[key + "std"] ** 2, rtol=0, atol=1e-6 * sf2)
    mean2, cov = gp.predict(Xs, n=ns, return_cov=True)
    np.testing.assert_allclose(cov, G4[key + "cov"], rtol=0, atol=1e-6 * sf2)
    np.testing.assert_allclose(mean2, mean, rtol=0, atol=1e-12)
    m0, s0 = gp.predict(Xs, n=0)
    np.testing.assert_allclose(m0, G4[key + "mean_n0"], rtol=0, atol=1e-6 * sf2)
    np.testing.assert_allclose(s0 ** 2, G4[key + "std_n0"] ** 2, rtol=0, atol=1e-6 * sf2)
    mo, co = gp.predict(Xs, n=ns, return_cov=True, output_transform=G4[key + "OT"])
    np.testing.assert_allclose(mo, G4[key + "mean_ot"], rtol=0, atol=1e-5 * sf2)
    np.testing.assert_allclose(co, G4[key + "cov_ot"], rtol=0, atol=1e-4 * sf2)
    assert np.array_equal(gp.predict(Xs, n=ns, return_std=False), mean)
    full = gp.predict(Xs, n=ns, full_output=True)
    assert set(full) == {"mean", "std", "cov"}
    # reading K after the fit gives the noise-free covariance, noise_K the zeros of ZeroKernel
    assert_close(gp.K, gp.compute_Kij(X, None, n, None), rtol=0, atol_scale=0)
    assert not gp.noise_K.any()


@pytest.mark.parametrize("kern", KERNELS)
def test_g3_noise_kernel_and_predict_noise(g, golden, kern):
    G3, G4 = golden("g3_fit"), golden("g4_predict")
    key = "%s_noise_" % kern
    p, X, y, n, err = (G3[key + s] for s in ("params", "X", "y", "n", "err_y"))
    nk = g.DiagonalNoiseKernel(num_dim=2, initial_noise=float(G3[key + "noise"]), noise_bound=(0.0, 5.0))
    gp = g.GaussianProcess(make_kernel(g, kern, 2, p), noise_k=nk, X=X, y=y, err_y=err, n=n)
    gp.compute_K_L_alpha_ll()
    assert abs(gp.ll - G3[key + "ll"]) <= 1e-9 * abs(G3[key + "ll"])
    assert_close(gp.L, G3[key + "L"], rtol=1e-8, atol_scale=1e-12)
    np.testing.assert_allclose(gp.noise_K, float(G3[key + "noise"]) ** 2 * np.eye(len(y)))
    Xs, ns = G4[key + "Xs"], G4[key + "ns"]
    mean, cov = gp.predict(Xs, n=ns, noise=True, return_cov=True)
    np.testing.assert_allclose(mean, G4[key + "mean"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(cov, G4[key + "cov"], rtol=0, atol=1e-7)
    _, cov0 = gp.predict(Xs, n=ns, noise=False, return_cov=True)
    np.testing.assert_allclose(cov0, G4[key + "cov_nonoise"], rtol=0, atol=1e-7)
    _, std = gp.predict(Xs, n=ns, noise=True)
    np.testing.assert_allclose(std ** 2, np.diag(G4[key + "cov"]), rtol=0, atol=1e-7)


def test_g3_mean_function_and_T(g, golden):
    G3, G4 = golden("g3_fit"), golden("g4_predict")
    key = "se_mu_"
    mu = g.ConstantMeanFunction(initial_params=[float(G3[key + "mu"])])
    gp = g.GaussianProcess(make_kernel(g, "se", 1, G3[key + "params"]), mu=mu, X=G3[key + "X"], y=G3[key + "y"],
                           err_y=G3[key + "err_y"])
    gp.compute_K_L_alpha_ll()
    assert abs(gp.ll - G3[key + "ll"]) <= 1e-9 * abs(G3[key + "ll"])
    mean, std = gp.predict(G4[key + "Xs"], n=G4[key + "ns"])
    np.testing.assert_allclose(mean, G4[key + "mean"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(std ** 2, G4[key + "std"] ** 2, rtol=0, atol=1e-7)
    key = "se_T_"
    gp = g.GaussianProcess(make_kernel(g, "se", 1, G3[key + "params"]))
    gp.add_data(G3[key + "Xp"], G3[key + "yp"], err_y=0.01)
    gp.add_data(G3[key + "Xq"], G3[key + "yT"], err_y=0.01, T=G3[key + "T"])
    np.testing.assert_array_equal(gp.T, G3[key + "Tfull"])
    gp.compute_K_L_alpha_ll()
    assert abs(gp.ll - G3[key + "ll"]) <= 1e-9 * abs(G3[key + "ll"])
    assert_close(gp.L, G3[key + "L"], rtol=1e-7, atol_scale=1e-11)
    assert_close(gp.alpha.ravel(), G3[key + "alpha"], rtol=1e-6, atol_scale=1e-8)
    mean, std = gp.predict(G4[key + "Xs"])
    np.testing.assert_allclose(mean, G4[key + "mean"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(std ** 2, G4[key + "std"] ** 2, rtol=0, atol=1e-7)


def test_g3_analytic_ll_gradient(g, golden):
    G3 = golden("g3_fit")
    key = "se_hd_"
    nk = g.DiagonalNoiseKernel(num_dim=2, initial_noise=float(G3[key + "noise"]), noise_bound=(0.0, 5.0))
    gp = g.GaussianProcess(make_kernel(g, "se", 2, G3[key + "params"]), noise_k=nk, X=G3[key + "X"], y=G3[key + "y"],
                           err_y=0.02, use_hyper_deriv=True)
    val, grad = gp.update_hyperparameters(list(G3[key + "params"]) + [float(G3[key + "noise"])])
    assert abs(-val - G3[key + "ll"]) <= 1e-9 * abs(G3[key + "ll"])
    assert_close(-grad, G3[key + "ll_deriv"], rtol=1e-7, atol_scale=1e-9)


# ---------------------------------------------------------------- G5: update_hyperparameters --
@pytest.mark.parametrize("kern", KERNELS)
def test_g5_update_hyperparameters_sweep(g, golden, kern):
    G = golden("g5_update")
    cls = g.SquaredExponentialKernel if kern == "se" else g.Matern52Kernel
    k = cls(num_dim=2, initial_params=[1.0, 0.3, 0.3], param_bounds=[(1e-3, 10.0)] * 3)
    gp = g.GaussianProcess(k, X=G["X"], y=G["y"], err_y=float(G["err_y"]), n=G["n"])
    for theta, want in zip(G[kern + "_thetas"], G[kern + "_negll"]):
        got = gp.update_hyperparameters(theta)
        if np.isinf(want):
            assert got == np.inf
        else:
            assert abs(got - want) <= 1e-8 * abs(want), (theta, got, want)


def test_g5_not_positive_definite(g, golden):
    G = golden("g5_update")
    k = g.SquaredExponentialKernel(num_dim=2, initial_params=[1.0, 0.3, 0.3], param_bounds=[(1e-3, 10.0)] * 3)
    gp = g.GaussianProcess(k, X=G["nonpd_X"], y=G["nonpd_y"], err_y=0.0, diag_factor=0.0)
    assert np.isinf(G["nonpd_negll"]) and gp.update_hyperparameters([1.0, 0.3, 0.3]) == np.inf
    gp.K_up_to_date = False
    with pytest.raises(np.linalg.LinAlgError):        # propagates when called directly
        gp.compute_K_L_alpha_ll()
    with pytest.raises(np.linalg.LinAlgError):
        gp.update_hyperparameters([1.0, 0.3, 0.3], inf_on_error=False)


# ---------------------------------------------------------------- G6: demo (config 1) ---------
def _demo_gp(g, G):
    hp = g.UniformJointPrior(0, 20) * g.GammaJointPriorAlt(1, 0.7)
    gp = g.GaussianProcess(g.SquaredExponentialKernel(hyperprior=hp))
    gp.add_data(G["core_X"], G["core_y"], err_y=G["core_err_y"])
    gp.add_data(0, 0, n=1)
    return gp


def test_g6_demo_known_answer_and_predictions(g, golden):
    G = golden("g6_demo")
    gp = _demo_gp(g, G)
    negll = gp.update_hyperparameters(G["demo_params"])
    assert abs(negll - 38.7782559807733) < 1e-8            # demo/demo.py:191 (probed in SURVEY.md section 4)
    assert abs(negll - float(G["negll_demo"])) < 1e-8
    assert_close(gp.alpha.ravel(), G["alpha_demo"], rtol=1e-8, atol_scale=1e-10)
    assert_close(gp.L, G["L_demo"], rtol=1e-9, atol_scale=1e-12)
    Xs = G["X_star"]
    y_star, err_y_star = gp.predict(Xs)
    np.testing.assert_allclose(y_star, G["y_star"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(err_y_star ** 2, G["err_y_star"] ** 2, rtol=0, atol=1e-8)
    gy, egy = gp.predict(Xs, n=1)
    np.testing.assert_allclose(gy, G["grad_y_star"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(egy ** 2, G["err_grad_y_star"] ** 2, rtol=0, atol=1e-7)
    out = gp.predict(np.concatenate((Xs, Xs)), n=np.concatenate((np.zeros_like(Xs), np.ones_like(Xs))),
                     full_output=True)
    np.testing.assert_allclose(out["mean"], G["full_mean"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(np.diag(out["cov"]), G["full_cov_diag"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(out["cov"][[0, 199, 400, 799], :], G["full_cov_rows"], rtol=0, atol=1e-7)


@pytest.mark.parametrize("method", ["SLSQP", "L-BFGS-B"])
def test_g6_demo_map_estimate(g, golden, method):
    G = golden("g6_demo")
    gp = _demo_gp(g, G)
    gp.update_hyperparameters(np.array([1.0, 1.0]))
    res, nres = gp.optimize_hyperparameters(method=method, random_starts=0, num_proc=0)
    tag = method.replace("-", "")
    assert nres == 1
    assert abs(res.fun - float(G["map_%s_fun" % tag])) < 1e-6
    np.testing.assert_allclose(res.x, G["map_%s_x" % tag], rtol=0, atol=2e-4)
    np.testing.assert_allclose(gp.params[:], [1.8849006111246833, 0.97760159723344708, 0.0], rtol=0, atol=1e-3)


def test_g6_demo_fitted_noise(g, golden):
    G = golden("g6_demo")
    hp = g.UniformJointPrior(0, 20) * g.GammaJointPriorAlt(1, 0.7)
    gpn = g.GaussianProcess(g.SquaredExponentialKernel(hyperprior=hp),
                            noise_k=g.DiagonalNoiseKernel(noise_bound=[0, 5]))
    gpn.add_data(G["core_X"], G["core_y"])
    gpn.add_data(0, 0, n=1)
    assert abs(gpn.update_hyperparameters(G["demo_noise_params"]) - float(G["negll_demo_noise"])) < 1e-9
    y, e = gpn.predict(G["X_star"])
    np.testing.assert_allclose(y, G["y_star_noise"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(e ** 2, G["err_y_star_noise"] ** 2, rtol=0, atol=1e-9)


# ---------------------------------------------------------------- oracle parity, seeded -------
def c3_inputs(N, d, seed=1234):
    """SURVEY.md section 8(d) synthetic inputs, C3 pattern: last quarter first-derivative rows."""
    rs = np.random.RandomState(seed)
    X = rs.rand(N, d)
    s = X.sum(1)
    n = np.zeros((N, d), dtype=int)
    y = np.sin(s)
    for i in range(3 * N // 4, N):
        n[i, i % d] = 1
        y[i] = np.cos(s[i])
    return X, n, y + 0.05 * rs.randn(N)


@pytest.mark.parametrize("kern,N,d,deriv", [("se", 1000, 2, False), ("m52", 1300, 3, True), ("se", 2049, 4, True),
                                            ("m52", 127, 1, True), ("se", 128, 2, False), ("m52", 129, 2, True)])
def test_fit_matches_oracle(ctx, oracle, kern, N, d, deriv):
    X, n, y = c3_inputs(N, d)
    if not deriv:
        n[:] = 0
    p = np.concatenate(([1.0], 0.3 * np.ones(d)))
    err = 0.05 * np.ones(N)
    ref = oracle.fit(kern, p, X, n, y, err, chol="scipy")
    ctx.set_data(X, n)
    for opts in ({"lookahead": 0, "nb_outer": 128}, {"lookahead": 1, "nb_outer": 256}, {"lookahead": 1, "nb_outer": 512},
                 {"lookahead": 1, "nb_outer": 256, "graph": 1}):
        for k_, v_ in dict({"graph": 0}, **opts).items():
            ctx.set_option(k_, v_)
        ll, ld = ctx.fit(KID[kern], p, 0.0, y, err, 1e2 * EPS)
        assert abs(ll - ref["ll_data"]) <= 1e-8 * abs(ref["ll_data"]), opts
        assert abs(ld - ref["logdet_half"]) <= 1e-10 * abs(ref["logdet_half"]), opts
    ctx.set_option("graph", 0)
    ctx.set_option("nb_outer", 0)
    assert_close(ctx.get_L(N), ref["L"], rtol=1e-6, atol_scale=1e-10)
    Xs = np.random.RandomState(7).rand(64, d)
    ns = np.zeros((64, d), int)
    ns[32:, 0] = 1
    mr, sr, cr = oracle.predict(kern, p, X, n, ref["L"], ref["alpha"], Xs, ns)
    m, s, c = ctx.predict(Xs, ns, 2)
    np.testing.assert_allclose(m, mr, rtol=0, atol=1e-6)
    np.testing.assert_allclose(c, cr, rtol=0, atol=1e-6)


@pytest.mark.parametrize("kern", ["se", "m52"])
def test_tiny_and_wide_inputs(ctx, oracle, kern):
    """Edge shapes: one to a handful of points (every matrix is padding + the augmented row) and up to the
    maximum input dimension (GPT_MAX_DIM = 16): ll, log|K|, alpha and predict against the oracle."""
    rs = np.random.RandomState(5)
    for N in (1, 2, 3, 17, 130):
        for D in (1, 5, 16):
            X = rs.rand(N, D)
            n = np.zeros((N, D), dtype=np.int32)
            if N > 2:
                n[N - 1, D - 1] = 1
            y = rs.randn(N)
            err = 0.1 * np.ones(N)
            p = np.concatenate(([1.3], 0.5 + rs.rand(D)))
            ref = oracle.fit(kern, p, X, n, y, err, chol="c")
            ctx.set_data(X, n)
            ll, ld = ctx.fit(KID[kern], p, 0.0, y, err, 1e2 * EPS)
            assert abs(ll - ref["ll_data"]) <= 1e-10 * max(1.0, abs(ref["ll_data"])), (N, D)
            assert abs(ld - ref["logdet_half"]) <= 1e-10 * max(1.0, abs(ref["logdet_half"])), (N, D)
            np.testing.assert_allclose(ctx.get_alpha(N), ref["alpha"].ravel(), rtol=1e-9, atol=1e-10)
            Xs = rs.rand(3, D)
            ns = np.zeros((3, D), dtype=np.int32)
            m, s, c = ctx.predict(Xs, ns, 2)
            mr, sr, cr = oracle.predict(kern, p, X, n, ref["L"], ref["alpha"], Xs, ns)
            np.testing.assert_allclose(m, mr, rtol=0, atol=1e-9)
            np.testing.assert_allclose(c, cr, rtol=0, atol=1e-9)


def test_staircase_update_against_numpy():
    """gpt_dev_gemm_nt_stair (the block-cyclic trailing update in one launch) on torch tensors against numpy:
    every column segment gets C -= P[rows] P[segment rows]^T on and below its own diagonal block, nothing above."""
    import torch
    from gptools_amd.dist import HipPanelOps
    ops = HipPanelOps(0)
    rs = np.random.RandomState(2)
    for (nb, W, nseg, k, tail) in ((128, 2, 3, 128, 64), (256, 3, 2, 256, 0), (512, 8, 2, 512, 1024)):
        m = (nseg - 1) * W * nb + nb + tail               # rows from the first segment's diagonal block down
        P = rs.randn(m, k)
        C0 = rs.randn(m, nseg * nb)
        with ops.queue("main"):
            dP = torch.from_numpy(P).cuda()
            dC = torch.from_numpy(C0).cuda()
            ops.gemm_nt_stair(m, nseg, nb, k, -1.0, dP.data_ptr(), k, dP.data_ptr(), k, W * nb, W * nb, 1.0,
                              dC.data_ptr(), nseg * nb)
            got = dC.cpu().numpy()
        ops.synchronize()
        for s_ in range(nseg):
            r0 = s_ * W * nb
            ref = C0[r0:, s_ * nb:(s_ + 1) * nb] - P[r0:].dot(P[r0:r0 + nb].T)
            blk = got[r0:, s_ * nb:(s_ + 1) * nb]
            low = np.tril(np.ones((nb, nb), bool))
            np.testing.assert_allclose(blk[:nb][low], ref[:nb][low], rtol=0, atol=1e-11 * k)      # diagonal block: lower part
            np.testing.assert_allclose(blk[nb:], ref[nb:], rtol=0, atol=1e-11 * k)
            # rows above a segment's diagonal block belong to other ranks' work: never touched (64x64 tile granularity
            # may rewrite the strictly-upper part of the diagonal tiles only)
            np.testing.assert_array_equal(got[:r0, s_ * nb:(s_ + 1) * nb], C0[:r0, s_ * nb:(s_ + 1) * nb])


def test_graph_capture_with_fresh_tile_tables(ctx):
    """hipGraph option at a size whose trailing updates need XCD tile-order tables that do not exist yet: the
    tables are uploaded while the stream is capturing.  Same ll as the eager schedule, twice (graph replay)."""
    N, d = 4480, 2
    X, n, y = c3_inputs(N, d)
    n[:] = 0
    p = np.array([1.0, 0.3, 0.3])
    err = 0.05 * np.ones(N)
    ctx.set_data(X, n)
    try:
        for k_, v_ in {"lookahead": 1, "nb_outer": 384, "graph": 1}.items():
            ctx.set_option(k_, v_)
        g1 = ctx.fit(0, p, 0.0, y, err, 1e2 * EPS)
        g2 = ctx.fit(0, p, 0.0, y, err, 1e2 * EPS)
        ctx.set_option("graph", 0)
        e1 = ctx.fit(0, p, 0.0, y, err, 1e2 * EPS)
    finally:
        ctx.set_option("graph", 0)
        ctx.set_option("nb_outer", 0)
    assert g1 == g2
    assert abs(g1[0] - e1[0]) <= 1e-11 * abs(e1[0]) and abs(g1[1] - e1[1]) <= 1e-12 * abs(e1[1])


def test_dense_kernels_against_numpy(ctx):
    rs = np.random.RandomState(11)
    for (m, n, k) in ((64, 64, 64), (200, 130, 70), (640, 384, 256), (1024, 1024, 512)):
        A, B, C0 = rs.randn(m, k), rs.randn(n, k), rs.randn(m, n)
        res = {}
        for tile in (64, 32, 0):
            ctx.set_option("tile", tile)
            got = ctx.gemm_nt_host(-1.0, A, B, 1.0, C0)
            np.testing.assert_allclose(got, C0 - A.dot(B.T), rtol=0, atol=1e-11 * k)
            res[tile] = got
            got = ctx.gemm_nt_host(2.0, A, B, 0.0, C0)
            np.testing.assert_allclose(got, 2.0 * A.dot(B.T), rtol=0, atol=1e-11 * k)
        # (64x64 and 32x32 tiles: the same sums in the same order -- what lets the library pick the tile by launch size)
        np.testing.assert_array_equal(res[64], res[32])
        np.testing.assert_array_equal(res[64], res[0])
    ctx.set_option("tile", 0)
    for N in (1, 17, 128, 129, 640, 1500):
        A = rs.randn(N, N)
        A = A.dot(A.T) + N * np.eye(N)
        L = ctx.potrf_host(A)
        np.testing.assert_allclose(L, np.linalg.cholesky(A), rtol=1e-11, atol=1e-11)
        B = rs.randn(N, 5)
        ctx.fit_matrix(A, np.zeros(N))
        np.testing.assert_allclose(ctx.solve_L(B), np.linalg.solve(np.linalg.cholesky(A), B), rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(ctx.cho_solve(B), np.linalg.solve(A, B), rtol=1e-9, atol=1e-11)
    with pytest.raises(np.linalg.LinAlgError) as ei:
        ctx.potrf_host(np.array([[4.0, 2.0, 0], [2.0, 1.0, 0], [0, 0, 1.0]]))
    assert "2-th leading minor" in str(ei.value)


def test_diagonal_block_kernel_look_ahead_body(ctx):
    """The 128-column leaf kernel's waves hand over through flags in LDS (potrf.hip, potf2_body_la: chain wave, ride-along
    waves, workers, store wave -- no workgroup barrier inside its loop).  A missing hand-over would show as a result that
    depends on the waves' timing: the same matrices factored 200 times must give the same bits every time, and LAPACK's factor
    to rounding; the first column that is not positive definite is reported wherever it lies in the block (first / inner /
    last column of a 16-column pivot block, first and last block, second 128-block behind a fused TRSM)."""
    rs = np.random.RandomState(2024)
    for N in (128, 640):
        A = rs.randn(N, N)
        A = A.dot(A.T) + N * np.eye(N)
        ref = np.linalg.cholesky(A)
        first = None
        for rep in range(200 if N == 128 else 40):
            L = ctx.potrf_host(A)
            if first is None:
                first = L.copy()
                np.testing.assert_allclose(L, ref, rtol=1e-11, atol=1e-11)
            else:
                assert np.array_equal(L, first), "run %d of N = %d differs from the first" % (rep, N)
        for col in (0, 1, 15, 16, 37, 111, 112, 127) + ((128, 200, 639) if N == 640 else ()):
            B = A.copy()
            B[col, col] = -1.0
            with pytest.raises(np.linalg.LinAlgError) as ei:
                ctx.potrf_host(B)
            assert ("%d-th leading minor" % (col + 1)) in str(ei.value), (N, col, str(ei.value))
    # the lock-step body (the 256-column leaf kernel keeps it) agrees to rounding: another process, GPT_POTF2_LA=0
    import subprocess
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from gptools_amd import _lib\n"
        "c = _lib.Context(0)\n"
        "rs = np.random.RandomState(7)\n"
        "A = rs.randn(384, 384); A = A.dot(A.T) + 384 * np.eye(384)\n"
        "L = c.potrf_host(A)\n"
        "print('RESULT', repr(float(np.abs(L - np.linalg.cholesky(A)).max())), repr(float(L.sum())))\n") % (ROOT,)
    res = {}
    for la in ("0", "1"):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GPT_POTF2_LA=la), stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        line = [l.split() for l in out.stdout.splitlines() if l.startswith("RESULT")][0]
        res[la] = (float(line[1]), float(line[2]))
        assert res[la][0] < 1e-11
    assert abs(res["0"][1] - res["1"][1]) <= 1e-10 * abs(res["0"][1])


def test_single_gpu_schedule_under_stream_jitter(ctx):
    """Missing-edge detector for the look-ahead schedule of gpt_fit (main / panel / helper streams): with GPT_JITTER set
    the library puts a delay kernel of random length in front of every dense launch.  Every dependency is an event, so
    the factorisation must come out bit-identical to the undisturbed run -- at a size that uses the fused diagonal-block
    kernel, and at one where the helper stream takes a slice of the updates."""
    import subprocess
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from gptools_amd import _lib\n"
        "from test_gpu_parity import c3_inputs\n"
        "c = _lib.Context(0)\n"
        "for N, d, reps in ((3000, 3, 6), (12800, 2, 2)):\n"
        "    X, n, y = c3_inputs(N, d)\n"
        "    c.set_data(X, n)\n"
        "    for rep in range(reps):\n"
        "        ll, ld = c.fit(1, np.concatenate(([1.0], 0.3 * np.ones(d))), 0.0, y, 0.05 * np.ones(N), 1e2 * sys.float_info.epsilon)\n"
        "        print('RESULT', N, repr(ll), repr(ld))\n"
        # an eager evaluation whose N is a multiple of 512: the pad leaf and the reduction on the main stream, alpha's substitution
        # behind the last real leaf on the panel stream (option defer_pad), the early block inverses in between
        "import hashlib\n"
        "c.set_option('eager_alpha', 1)\n"
        "X, n, y = c3_inputs(4096, 2)\n"
        "c.set_data(X, n)\n"
        "for rep in range(5):\n"
        "    ll, ld = c.fit(1, np.array([1.0, 0.3, 0.3]), 0.0, y, 0.05 * np.ones(4096), 1e2 * sys.float_info.epsilon)\n"
        "    print('EAGER', repr(ll), repr(ld), hashlib.sha1(c.get_alpha(4096).tobytes()).hexdigest())\n") % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GPT_JITTER="120"), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [l.split()[1:] for l in out.stdout.splitlines() if l.startswith("RESULT")]
    assert len(got) == 8
    import hashlib
    eager = [l.split()[1:] for l in out.stdout.splitlines() if l.startswith("EAGER")]
    assert len(eager) == 5
    X, n, y = c3_inputs(4096, 2)
    ctx.set_data(X, n)
    ctx.set_option("eager_alpha", 1)
    try:
        ll, ld = ctx.fit(1, np.array([1.0, 0.3, 0.3]), 0.0, y, 0.05 * np.ones(4096), 1e2 * EPS)
        digest = hashlib.sha1(ctx.get_alpha(4096).tobytes()).hexdigest()
    finally:
        ctx.set_option("eager_alpha", 0)
    for e_ in eager:
        assert float(e_[0]) == ll and float(e_[1]) == ld and e_[2] == digest, (e_, ll, ld, digest)
    for N, d in ((3000, 3), (12800, 2)):
        X, n, y = c3_inputs(N, d)
        ctx.set_data(X, n)
        ll, ld = ctx.fit(1, np.concatenate(([1.0], 0.3 * np.ones(d))), 0.0, y, 0.05 * np.ones(N), 1e2 * EPS)
        for g_ in got:
            if int(g_[0]) == N:
                assert float(g_[1]) == ll and float(g_[2]) == ld, (N, g_, ll, ld)


def test_schedule_options_agree_with_default(ctx, oracle):
    """The schedule variants kept behind options (NOTES_r02.md) -- left-looking panels, the deferred rest,
    the panel-stream urgent update on / off, variable panel widths, event edges, the consumer workgroup sizes of the fused
    leaf kernel, the unfused leaf -- factor the same matrix: ll / log|K| within 1e-11 of the default schedule and of the CPU
    oracle, at a size with several panels and a ragged end; the variants that only regroup the same sums, bit for bit."""
    N, d = 3000, 3
    X, n, y = c3_inputs(N, d)
    p = np.array([1.0, 0.3, 0.3, 0.3])
    err = 0.05 * np.ones(N)
    ref = oracle.fit("m52", p, X, n, y, err, chol="scipy")
    ctx.set_data(X, n)
    base = ctx.fit(1, p, 0.0, y, err, 1e2 * EPS)
    assert abs(base[0] - ref["ll_data"]) <= 1e-9 * abs(ref["ll_data"])
    variants = ({"nb_outer": 256}, {"nb_outer": 512}, {"inner": 1}, {"inner": 2},
                {"defer_rows": 4608}, {"purg_rows": 0}, {"purg_rows": 1024}, {"nb_early": 512, "nb_switch_rows": 1500},
                {"purg_rows": 1024, "defer_rows": 4608},
                # a 128-wide first panel is factored before the rest of K is built: the panel stream's first update beyond
                # the head columns has to wait for the build (it once did not: "8064-th leading minor ...")
                {"ramp": 1, "purg_rows": 1024}, {"ramp": 1, "purg_rows": 0}, {"edge_flags": 0}, {"edge_flags": 0, "ramp": 1, "purg_rows": 512},
                # 128-row consumer workgroups everywhere / 64-row ones everywhere / where the default has 32-row ones, 32-row ones
                # everywhere, 16-row ones, a mix; the unfused leaf (diagonal-block kernel + panel TRSM)
                {"fuse_rows64": 0}, {"fuse_rows64": 8192}, {"fuse_rows32": 0}, {"fuse_rows32": 8192}, {"fuse_rows16": 8192},
                {"fuse_rows32": 3000, "fuse_rows16": 1000, "fuse_rows64": 5000}, {"fuse_trsm": 0}, {"merge_urgent": 0},
                # the schedule bench.py times its roofline with (profile_gemm drops the tail wait), on flag and on event edges
                {"tail_wait": 0}, {"tail_wait": 0, "edge_flags": 0})
    defaults = {"nb_outer": 0, "inner": 0, "defer_rows": 0, "purg_rows": 6144, "nb_early": 0, "nb_switch_rows": 4608,
                "ramp": 0, "edge_flags": 1, "fuse_rows64": 2048, "fuse_rows32": 2048, "fuse_rows16": 0, "fuse_trsm": 8192, "merge_urgent": 1,
                "tail_wait": 1}
    # (bit-identical to the default schedule by construction: same sums in the same order; the tail wait moves a wait, not a sum)
    exact = ("fuse_rows64", "fuse_rows32", "fuse_rows16", "merge_urgent", "tail_wait")
    try:
        for v in variants:
            for k_, d_ in defaults.items():
                ctx.set_option(k_, d_)
            for k_, v_ in v.items():
                ctx.set_option(k_, v_)
            for rep in range(2):                  # (twice: the flag word of the fused kernels carries over between launches)
                got = ctx.fit(1, p, 0.0, y, err, 1e2 * EPS)
                assert abs(got[0] - base[0]) <= 1e-11 * abs(base[0]), v
                assert abs(got[1] - base[1]) <= 1e-12 * abs(base[1]), v
                if all(k_ in exact for k_ in v):
                    assert got == base, v
        for k_, d_ in defaults.items():
            ctx.set_option(k_, d_)
        # the timed evaluation of bench.py's roofline: every large main-stream launch carries timing events
        ctx.gemm_profile_read()
        ctx.set_option("profile_gemm", 1)
        got = ctx.fit(1, p, 0.0, y, err, 1e2 * EPS)
        assert got == base
        assert ctx.gemm_profile_read()[2] > 0          # (the launches were timed)
    finally:
        for k_, d_ in defaults.items():
            ctx.set_option(k_, d_)
        ctx.set_option("profile_gemm", 0)
    # options that were removed with the code behind them (round 6) are refused, not ignored
    for gone in ("fuse_upd", "pair_rows", "leaf256", "early_rows", "late_rows", "late_pad", "late_pad_rows", "panel_prio",
                 "head_wait_wgs", "purg_rows_flags", "merge_min_tiles", "inner_rows"):
        with pytest.raises(Exception):
            ctx.set_option(gone, 1)
    with pytest.raises(Exception):
        ctx.set_option("tile", 128)
    # dense matrices of awkward sizes against LAPACK, and the position of a failing pivot
    rs = np.random.RandomState(7)
    try:
        for Nd in (255, 256, 300, 640, 1000):
            for nb in (256, 384):
                ctx.set_option("nb_outer", nb)
                A = rs.randn(Nd, Nd)
                A = A.dot(A.T) + Nd * np.eye(Nd)
                np.testing.assert_allclose(np.tril(ctx.potrf_host(A)), np.linalg.cholesky(A), rtol=1e-11, atol=1e-11)
        with pytest.raises(np.linalg.LinAlgError) as ei:      # not positive definite inside the second 128-column leaf
            A = np.eye(300)
            A[200, 200] = -1.0
            ctx.potrf_host(A)
        assert "201-th leading minor" in str(ei.value)
    finally:
        ctx.set_option("nb_outer", 0)


def test_fused_leaf_publication_is_repeatable_and_matches_the_unfused_leaf(ctx):
    """The fused diagonal-block + TRSM kernel publishes the packed workspace block by block with PIPELINED write-through stores:
    flag jb goes up once `s_waitcnt vmcnt(32 - 4 jb)` says that step jb - 1's stores are in memory (potrf.hip, store wave; the
    store count per step is fixed by explicit store instructions and a static_assert -- ADVICE r5).  A flag raised early would let
    a consumer read a stale inverse block or packed block: timing-dependent, so the same factorisation is repeated many times --
    every repetition must return the bits of the first -- at sizes with 32-, 64- and 128-row consumer workgroups, and must agree
    with the UNFUSED leaf (potf2_diag_kernel + trsm_panel_kernel: no in-launch publication at all) to rounding."""
    for N, d, reps in ((1500, 2, 150), (2600, 3, 100), (5000, 3, 40)):
        X, n, y = c3_inputs(N, d)
        p = np.concatenate(([1.0], 0.3 * np.ones(d)))
        err = 0.05 * np.ones(N)
        ctx.set_data(X, n)
        try:
            ctx.set_option("fuse_trsm", 0)
            plain = ctx.fit(1, p, 0.0, y, err, 1e2 * EPS)
        finally:
            ctx.set_option("fuse_trsm", 8192)
        first = ctx.fit(1, p, 0.0, y, err, 1e2 * EPS)
        assert abs(first[0] - plain[0]) <= 1e-11 * abs(plain[0]) and abs(first[1] - plain[1]) <= 1e-12 * abs(plain[1]), N
        L0 = ctx.get_L(N)
        for rep in range(reps):
            assert ctx.fit(1, p, 0.0, y, err, 1e2 * EPS) == first, (N, rep)
        np.testing.assert_array_equal(ctx.get_L(N), L0)


def test_panel_inverse_and_gemm_solve_against_numpy():
    """gpt_dev_potrf_panel on the diagonal block, gpt_dev_trinv, then the rows below as ONE GEMM against the inverse --
    the tail chunks of the row-chunked multi-GPU schedule -- against numpy (L^-1 itself and X = B L^-T)."""
    import torch
    from gptools_amd.dist import HipPanelOps
    ops = HipPanelOps(0)
    rs = np.random.RandomState(5)
    for nb, m in ((128, 256), (512, 1536)):
        A = rs.randn(nb, nb)
        A = A.dot(A.T) + nb * np.eye(nb)
        Bm = rs.randn(m, nb)
        with ops.queue("panel"):
            P = torch.from_numpy(np.vstack([A, Bm])).cuda()
            invd = torch.empty(((nb // 128) * 9216,), dtype=torch.float64, device="cuda")
            info = torch.zeros((1,), dtype=torch.int32, device="cuda")
            W = torch.empty((nb, nb), dtype=torch.float64, device="cuda")
            Xo = torch.empty((m, nb), dtype=torch.float64, device="cuda")
            ops.potrf_panel(nb, nb, P.data_ptr(), nb, invd, info, 0)
            ops.trinv(nb, P.data_ptr(), nb, invd, W.data_ptr(), nb)
            ops.gemm_nt(m, nb, nb, 1.0, P.data_ptr() + nb * nb * 8, nb, W.data_ptr(), nb, 0.0, Xo.data_ptr(), nb, 0, q="panel")
        ops.synchronize()
        L = np.linalg.cholesky(A)
        assert int(info.cpu()[0]) == 0
        np.testing.assert_allclose(W.cpu().numpy(), np.linalg.inv(L), rtol=0, atol=1e-12)
        np.testing.assert_allclose(Xo.cpu().numpy(), np.linalg.solve(L, Bm.T).T, rtol=0, atol=1e-11)


# ---------------------------------------------------------------- full BASELINE sizes ---------
@pytest.mark.parametrize("cfg", ["C2", "C3"])
def test_full_size_properties(ctx, oracle, cfg):
    """BASELINE configs[1] (SE, N=4096, d=2) and configs[2] (Matern52 + derivative rows, N=8192, d=3):
    (a) LML and log|K| vs the CPU path (oracle K-build + LAPACK Cholesky) within 1e-8 relative;
    (b) reconstruction: (L L^T) x == K_tot x for random x (matrix-free, through gpt_kbuild row blocks);
    (c) K_tot alpha == y; (d) same answer with and without look-ahead / graph replay."""
    if cfg == "C2":
        kern, N, d = "se", 4096, 2
        X, n, y = c3_inputs(N, d)
        n[:] = 0
    else:
        kern, N, d = "m52", 8192, 3
        X, n, y = c3_inputs(N, d)
    p = np.concatenate(([1.0], 0.3 * np.ones(d)))
    err = 0.05 * np.ones(N)
    ctx.set_data(X, n)
    res = []
    for opts in ({"lookahead": 1, "graph": 0}, {"lookahead": 0, "graph": 0}, {"lookahead": 1, "graph": 1}):
        for k_, v_ in opts.items():
            ctx.set_option(k_, v_)
        res.append(ctx.fit(KID[kern], p, 0.0, y, err, 1e2 * EPS))
    ctx.set_option("graph", 0)
    for r in res[1:]:
        assert abs(r[0] - res[0][0]) <= 1e-11 * abs(res[0][0]) and abs(r[1] - res[0][1]) <= 1e-12 * abs(res[0][1])
    ll, ld = res[-1]
    ref = oracle.fit(kern, p, X, n, y, err, chol="scipy")
    assert abs(ll - ref["ll_data"]) <= 1e-8 * abs(ref["ll_data"])
    assert abs(ld - ref["logdet_half"]) <= 1e-8 * abs(ref["logdet_half"])
    L = ctx.get_L(N)
    alpha = ctx.get_alpha(N)
    assert np.array_equal(np.triu(L, 1)[:64, :64], np.zeros((64, 64)))
    Kt = ctx.kbuild(KID[kern], p, X, n)
    Kt[np.arange(N), np.arange(N)] += err ** 2 + 1e2 * EPS
    np.testing.assert_allclose(Kt, Kt.T, rtol=0, atol=1e-13)           # symmetry of the builder
    x = np.random.RandomState(3).randn(N, 4)
    np.testing.assert_allclose(L.dot(L.T.dot(x)), Kt.dot(x), rtol=0, atol=1e-9 * np.abs(Kt.dot(x)).max())
    np.testing.assert_allclose(Kt.dot(alpha), y, rtol=0, atol=1e-7)
    assert_close(alpha, ref["alpha"], rtol=1e-5, atol_scale=1e-7)
    Xs = np.random.RandomState(64).rand(64, d)
    ns = np.zeros((64, d), int)
    mr, sr, _ = oracle.predict(kern, p, X, n, ref["L"], ref["alpha"], Xs, ns, want_cov=False)
    m, s, _ = ctx.predict(Xs, ns, 1)
    np.testing.assert_allclose(m, mr, rtol=0, atol=1e-6)
    np.testing.assert_allclose(s ** 2, sr ** 2, rtol=0, atol=1e-6)


def test_full_size_c5_fit_and_map_loop(g, ctx, oracle):
    """BASELINE configs[4]: the MAP loop at N=16384 (SquaredExponential, d=2) through the plugin API --
    ``optimize_hyperparameters(method='L-BFGS-B', maxiter=50, random_starts=0)`` (ref gaussian_process.py:623-783),
    every objective evaluation a K rebuild + Cholesky on the GPU (ref :1418-1469).
    (a) one evaluation at the start point vs the CPU path (oracle K-build + LAPACK) within 1e-8 relative;
    (b) the optimiser's accepted iterates decrease monotonically and stay inside the bounds;
    (c) the value it returns equals the CPU path's log-posterior at the returned hyperparameters within 1e-8;
    (d) the GP is left at the optimum, and the optimum beats the start."""
    N, d = 16384, 2
    X, n, y = c3_inputs(N, d)
    n[:] = 0
    err = 0.05 * np.ones(N)
    p0 = np.array([1.0, 0.3, 0.3])
    ctx.set_data(X, n)
    ll, ld = ctx.fit(KID["se"], p0, 0.0, y, err, 1e2 * EPS)
    ref = oracle.fit("se", p0, X, n, y, err, chol="scipy")
    assert abs(ll - ref["ll_data"]) <= 1e-8 * abs(ref["ll_data"])
    assert abs(ld - ref["logdet_half"]) <= 1e-8 * abs(ref["logdet_half"])
    del ref
    k = g.SquaredExponentialKernel(num_dim=d, initial_params=list(p0), param_bounds=[(1e-3, 10.0)] * 3)
    gp = g.GaussianProcess(k, X=X, y=y, err_y=0.05)
    v0 = gp.update_hyperparameters(p0)
    assert abs(-v0 - gp.hyperprior(gp.params) - ll) <= 1e-12 * abs(ll)       # plugin API == C ABI, same evaluation
    seen, iterates = {}, []
    inner = gp.update_hyperparameters

    def recording(p_, *a, **kw):
        v = inner(p_, *a, **kw)
        if not a and not kw:
            seen[np.asarray(p_, dtype=float).tobytes()] = v
        return v
    gp.update_hyperparameters = recording
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res, nres = gp.optimize_hyperparameters(
            method="L-BFGS-B", random_starts=0, num_proc=0,
            opt_kwargs={"options": {"maxiter": 50}, "callback": lambda xk: iterates.append(np.array(xk, dtype=float))})
    gp.update_hyperparameters = inner
    assert nres == 1 and 1 <= res.nit <= 50 and len(iterates) == res.nit
    vals = [v0] + [seen[x.tobytes()] for x in iterates]        # every accepted iterate was an objective evaluation
    assert all(b <= a for a, b in zip(vals, vals[1:])), vals
    assert res.fun == vals[-1] and res.fun < v0 - 1.0
    assert np.all(res.x >= 1e-3) and np.all(res.x <= 10.0)
    np.testing.assert_array_equal(gp.free_params[:], res.x)
    ref = oracle.fit("se", res.x, X, n, y, err, chol="scipy")
    post = ref["ll_data"] + gp.hyperprior(gp.params)
    assert abs(-res.fun - post) <= 1e-8 * abs(post)
    # the factor at the optimum: K_tot alpha = y on a sample of rows
    alpha = gp.alpha[:, 0]
    rows = np.arange(0, N, 1021)
    Kr = ctx.kbuild(KID["se"], res.x, X[rows], n[rows], X, n)
    Kr[np.arange(len(rows)), rows] += err[rows] ** 2 + 1e2 * EPS
    np.testing.assert_allclose(Kr.dot(alpha), y[rows], rtol=0, atol=1e-6)


def test_full_size_c4_single_gpu_and_block_cyclic(ctx, oracle):
    """BASELINE configs[3]: SquaredExponential, N=32768, d=4, no derivative rows (K_tot = 8.6 GB).
    (a) single-context path (gpt_fit) vs the CPU path (oracle K-build on the host cores + LAPACK) within 1e-8 relative
        on ll and log|K|, alpha against cho_solve on a sample;
    (b) the block-cyclic engine (gptools_amd.dist.DistributedLML, product ops, world size 1) at the same size, both
        schedules (whole panels / row chunks): same ll and log|K|;
    (c) size-independent properties: K_tot alpha = y on sampled rows (rows rebuilt by the pair kernel),
        (L L^T) x = K_tot x on sampled rows, predictive mean / variance at 64 points against the CPU path."""
    from gptools_amd.dist import DistributedLML
    N, d = 32768, 4
    X, n, y = c3_inputs(N, d)
    n[:] = 0
    p = np.concatenate(([1.0], 0.3 * np.ones(d)))
    err = 0.05 * np.ones(N)
    ctx.set_data(X, n)
    ll, ld = ctx.fit(KID["se"], p, 0.0, y, err, 1e2 * EPS)
    ref = oracle.fit("se", p, X, n, y, err, chol="scipy")
    assert abs(ll - ref["ll_data"]) <= 1e-8 * abs(ref["ll_data"])
    assert abs(ld - ref["logdet_half"]) <= 1e-8 * abs(ref["logdet_half"])
    alpha = ctx.get_alpha(N)
    assert_close(alpha, ref["alpha"], rtol=1e-5, atol_scale=1e-7)
    rows = np.arange(0, N, 1499)
    Kr = ctx.kbuild(KID["se"], p, X[rows], n[rows], X, n)
    Kr[np.arange(len(rows)), rows] += err[rows] ** 2 + 1e2 * EPS
    np.testing.assert_allclose(Kr.dot(alpha), y[rows], rtol=0, atol=1e-6)
    Xs = np.random.RandomState(64).rand(64, d)
    ns = np.zeros((64, d), int)
    m, s, _ = ctx.predict(Xs, ns, 1)
    mr, sr, _ = oracle.predict("se", p, X, n, ref["L"], ref["alpha"], Xs, ns, want_cov=False)
    np.testing.assert_allclose(m, mr, rtol=0, atol=1e-6)
    np.testing.assert_allclose(s ** 2, sr ** 2, rtol=0, atol=1e-6)
    del ref, mr, sr
    gc.collect()
    L = ctx.get_L(N)
    x = np.random.RandomState(3).randn(N, 2)
    Ltx = L.T.dot(x)
    np.testing.assert_allclose(L[rows].dot(Ltx), Kr.dot(x), rtol=0, atol=1e-9 * np.abs(Kr.dot(x)).max())
    assert np.array_equal(np.triu(L[:256, :256], 1), np.zeros((256, 256)))
    del L, Ltx
    gc.collect()
    from gptools_amd.dist import GridLML
    for make in (lambda: DistributedLML(X, n, nb=512, device=0), lambda: GridLML(X, n, (1, 1), nb=512, device=0)):
        plan = make()
        ll2, ld2 = plan.fit(KID["se"], p, y, err)
        assert abs(ll2 - ll) <= 1e-10 * abs(ll), type(plan).__name__
        assert abs(ld2 - ld) <= 1e-11 * abs(ld), type(plan).__name__
        del plan
        gc.collect()


def test_distributed_plan_on_one_gpu(ctx, oracle):
    """gptools_amd.dist with the product ops (HipPanelOps, device API of the C ABI) and world_size 1:
    same ll / log|K| as the single-context path and the oracle."""
    from gptools_amd.dist import DistributedLML, GridLML
    X, n, y = c3_inputs(1500, 3)
    p = np.array([1.0, 0.3, 0.3, 0.3])
    err = 0.05 * np.ones(1500)
    ref = oracle.fit("m52", p, X, n, y, err, chol="scipy")
    for nb, kw in ((128, {"schedule": "bcast"}), (256, {"schedule": "bcast"}), (512, {"schedule": "bcast"}),
                   (128, {"schedule": "bcast", "inv_min_rows": 0}), (512, {"schedule": "bcast", "inv_min_rows": 0}),
                   (128, {"grid": (1, 1)}), (256, {"grid": (1, 1), "lookahead": False}), (512, {"grid": (1, 1)})):
        kw = dict(kw)
        plan = (GridLML(X, n, kw.pop("grid"), nb=nb, device=0, **kw) if "grid" in kw else
                DistributedLML(X, n, nb=nb, device=0, **kw))
        ll, ld = plan.fit(1, p, y, err)
        assert abs(ll - ref["ll_data"]) <= 1e-9 * abs(ref["ll_data"]), (nb, kw)
        assert abs(ld - ref["logdet_half"]) <= 1e-10 * abs(ref["logdet_half"]), (nb, kw)
        ll2, _ = plan.fit(1, p, y, err)
        assert ll2 == ll
        del plan                # (its streams go with it: every plan owns two library contexts)
        gc.collect()


def test_compiled_schedule_native_replay_matches_the_step_loop(ctx, oracle):
    """Compiled schedules: the 1-D engine's step loop recorded once as an op list and replayed by gpt_plan_run (a C
    loop over the list, csrc/api_plan.inc), by the Python interpreter of the same list, and the step loop issuing every operation
    itself give the same bits -- same kernels on the same buffers in the same order -- and agree with the oracle; a second
    evaluation with other hyperparameters reuses the plan (only the K-block ops see them); look-ahead off and the
    explicit-inverse route for tall panels are plans of their own."""
    from gptools_amd.dist import DistributedLML, HipPanelOps
    X, n, y = c3_inputs(2300, 3)
    p = np.array([1.0, 0.3, 0.3, 0.3])
    err = 0.05 * np.ones(2300)
    ref = oracle.fit("m52", p, X, n, y, err, chol="scipy")
    ref2 = oracle.fit("m52", 1.1 * p, X, n, y, err, chol="scipy")
    ops = HipPanelOps(0)
    for nb, kw in ((256, {}), (512, {"inv_min_rows": 0}), (128, {"lookahead": False})):
        got = {}
        for mode in ("native", "python", False):
            plan = DistributedLML(X, n, nb=nb, ops=ops, compiled=mode, **kw)
            assert plan.compiled == mode
            got[mode] = (plan.fit(1, p, y, err), plan.fit(1, 1.1 * p, y, err), plan.fit(1, p, y, err))
            if mode:
                assert len(plan._plans) == 1 and plan.timings["plan_ops"] > 20
            if mode == "native":
                assert 0.0 < plan.timings["native_enqueue_ms"] < 200.0
            del plan
            gc.collect()
        assert got["native"] == got["python"] == got[False], (nb, kw, got)
        a, b, c_ = got["native"]
        assert a == c_
        assert abs(a[0] - ref["ll_data"]) <= 1e-9 * abs(ref["ll_data"]) and abs(a[1] - ref["logdet_half"]) <= 1e-10 * abs(ref["logdet_half"])
        assert abs(b[0] - ref2["ll_data"]) <= 1e-9 * abs(ref2["ll_data"])
    # not positive definite: reported through the plan like through the step loop
    Xd = X.copy()
    Xd[1] = Xd[0]
    nd = np.zeros_like(n)
    plan = DistributedLML(Xd, nd, nb=256, ops=ops, compiled="native")
    with pytest.raises(np.linalg.LinAlgError):
        plan.fit(0, p, y, 0.0, diag_factor=0.0)


def test_compiled_grid_schedule_native_replay_matches_the_step_loop(oracle):
    """The 2-D engine's compiled schedule: GridLML's step loop recorded once and replayed by gpt_plan_run, by the Python interpreter
    of the list and issued by the step loop itself -- same bits, equal to the oracle, at 1 x 1 (look-ahead on / off).  And for a
    rank PLACED in a 2 x 4 / 4 x 2 / 2 x 3 grid (its schedule of a multi-rank job on the one GPU there is: the five channels'
    broadcasts are in the list, nothing is sent, the receive buffers hold a constant): the rank's matrix after the evaluation is
    bit-identical across the three drivers -- every grid-only op (K rectangle, row_sumsq, the grid staircase update with its
    offsets) is encoded as the step loop issues it."""
    import torch
    from gptools_amd.dist import GridLML, HipPanelOps
    X, n, y = c3_inputs(2300, 3)
    p = np.array([1.0, 0.3, 0.3, 0.3])
    err = 0.05 * np.ones(2300)
    ref = oracle.fit("m52", p, X, n, y, err, chol="scipy")
    ref2 = oracle.fit("m52", 1.1 * p, X, n, y, err, chol="scipy")
    ops = HipPanelOps(0)
    for nb, kw in ((256, {}), (128, {"lookahead": False})):
        got = {}
        for mode in ("native", "python", False):
            plan = GridLML(X, n, (1, 1), nb=nb, ops=ops, compiled=mode, **kw)
            assert plan.compiled == mode
            got[mode] = (plan.fit(1, p, y, err), plan.fit(1, 1.1 * p, y, err), plan.fit(1, p, y, err))
            if mode:
                assert len(plan._plans) == 1 and plan.timings["plan_ops"] > 20
            del plan
            gc.collect()
        assert got["native"] == got["python"] == got[False], (nb, kw, got)
        a, b, c_ = got["native"]
        assert a == c_
        assert abs(a[0] - ref["ll_data"]) <= 1e-9 * abs(ref["ll_data"]) and abs(a[1] - ref["logdet_half"]) <= 1e-10 * abs(ref["logdet_half"])
        assert abs(b[0] - ref2["ll_data"]) <= 1e-9 * abs(ref2["ll_data"])
    assert GridLML(X, n, (1, 1), nb=256, ops=ops).compiled == "native"          # the default on one rank

    class Placed(GridLML):
        def _on(self, size):
            return size > 1

        def _xbcast(self, kind, k, buf, src, group, size):
            return GridLML._xbcast(self, kind, k, buf, src, group, size) if self._rec is not None else []

        def _plan_collective(self, opcode, buf, what):
            return []

        def _allreduce(self, t, op):
            pass

    for grid, rank in (((2, 4), 5), ((4, 2), 2), ((2, 3), 4)):
        bits = {}
        for mode in ("native", "python", False):
            plan = Placed(X, n, grid, nb=128, ops=ops, layout=rank, compiled=mode)
            for t in plan.R + plan.C + plan.H + plan.W + [q_ for ps in plan.piece for q_ in ps]:
                t.fill_(1e-3)
            plan.A.zero_()
            for rep in range(2):
                try:
                    plan.fit(1, p, y, err)
                except np.linalg.LinAlgError:
                    pass
                torch.cuda.synchronize()
                bits[mode, rep] = (plan.A.view(torch.int64).clone(), plan.red.view(torch.int64).clone())
            if mode:
                (cp,) = plan._plans.values()
                assert sum(1 for o in cp.ops if o[0] == 10) > 10        # the broadcasts are part of the list
            del plan
            gc.collect()
        for rep in range(2):
            for mode in ("python", False):
                assert torch.equal(bits["native", rep][0], bits[mode, rep][0]), (grid, rank, mode, rep)
                assert torch.equal(bits["native", rep][1], bits[mode, rep][1]), (grid, rank, mode, rep)


def test_replicated_random_starts_two_ranks_one_gpu():
    """SURVEY 8f-2 / the reference's pool over random starts (gaussian_process.py:723-735): two gloo ranks, both on
    cuda:0, split four starts of optimize_hyperparameters; both return the same optimum, equal to the one a single
    process finds from the same draws."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import os, sys, json, warnings, numpy as np\n"
        "warnings.simplefilter('ignore')\n"
        "sys.path.insert(0, %r)\n"
        "rank, world = int(sys.argv[1]), int(sys.argv[2])\n"
        "if world > 1:\n"
        "    import torch.distributed as dist\n"
        "    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='29519')\n"
        "    dist.init_process_group('gloo', rank=rank, world_size=world)\n"
        "import gptools_amd as g\n"
        "rs = np.random.RandomState(3)\n"
        "X = rs.rand(300, 2); y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(300)\n"
        "k = g.SquaredExponentialKernel(num_dim=2, initial_params=[1.0, 0.5, 0.5], param_bounds=[(0.05, 10.0)] * 3)\n"
        "gp = g.GaussianProcess(k, X=X, y=y, err_y=0.05)\n"
        "np.random.seed(11)                       # the draws come from numpy's global state: same on every rank\n"
        "res, nres = gp.optimize_hyperparameters(method='L-BFGS-B', random_starts=4, opt_kwargs={'options': {'maxiter': 30}})\n"
        "print('RESULT', json.dumps({'rank': rank, 'fun': float(res.fun), 'x': [float(v) for v in res.x], 'n': nres,\n"
        "                            'params': [float(v) for v in gp.free_params[:]]}))\n"
        "if world > 1: dist.destroy_process_group()\n"
    ) % root

    def launch(rank, world):
        return subprocess.Popen([sys.executable, "-c", code, str(rank), str(world)], stdout=subprocess.PIPE,
                                stderr=subprocess.PIPE, text=True)

    def result(proc):
        out, err = proc.communicate(timeout=600)
        assert proc.returncode == 0, err[-2000:]
        return json.loads([l for l in out.splitlines() if l.startswith("RESULT")][-1].split(" ", 1)[1])

    import json
    single = result(launch(0, 1))
    procs = [launch(r, 2) for r in range(2)]
    r0, r1 = sorted((result(p) for p in procs), key=lambda d: d["rank"])
    assert r0["n"] == r1["n"] == single["n"] == 4
    assert r0["fun"] == r1["fun"] and r0["x"] == r1["x"]                 # every rank ends with the same optimum
    assert abs(r0["fun"] - single["fun"]) <= 1e-9 * abs(single["fun"])    # ... the one a single process finds
    np.testing.assert_allclose(r0["x"], single["x"], rtol=1e-6)
    np.testing.assert_allclose(r0["params"], r0["x"], rtol=0, atol=0)     # and the GP is left at it


def test_compute_ll_matrix_batched_equals_sequential():
    """compute_ll_matrix (ref gaussian_process.py:1607-1692) through the batched evaluator (two evaluations in flight
    on the GPU) against one update_hyperparameters call per grid point; out-of-bounds points give -inf in both, the
    GP's hyperparameters are restored, and data added afterwards reaches every pooled context."""
    import warnings
    import gptools_amd as g
    rs = np.random.RandomState(8)
    X = rs.rand(400, 2)
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(400)
    k = g.SquaredExponentialKernel(num_dim=2, initial_params=[1.0, 0.4, 0.6], fixed_params=[False, False, True],
                                   param_bounds=[(0.2, 5.0), (0.05, 2.0), (0.05, 2.0)])
    gp = g.GaussianProcess(k, X=X, y=y, err_y=0.05)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ll, pv = gp.compute_ll_matrix([(0.1, 3.0), (0.1, 1.0)], [4, 5])       # sigma_f = 0.1 lies outside its bounds
        assert ll.shape == (4, 5) and len(pv) == 2
        np.testing.assert_array_equal(gp.free_params[:], [1.0, 0.4])
        seq = np.array([[-gp.update_hyperparameters([a, b]) for b in pv[1]] for a in pv[0]])
        assert np.all(np.isneginf(ll[0])) and np.all(np.isneginf(seq[0]))
        np.testing.assert_allclose(ll[1:], seq[1:], rtol=1e-12, atol=0)
        gp.batch_concurrency = 1
        ll1, _ = gp.compute_ll_matrix([(0.1, 3.0), (0.1, 1.0)], [4, 5])
        np.testing.assert_allclose(ll1[1:], seq[1:], rtol=1e-12, atol=0)
        gp.batch_concurrency = 2
        gp.add_data(rs.rand(50, 2), rs.randn(50), err_y=0.05)
        b = gp.ll_batch([[1.0, 0.4], [1.5, 0.3], [2.0, 0.2]])
        s = np.array([-gp.update_hyperparameters(p) for p in ([1.0, 0.4], [1.5, 0.3], [2.0, 0.2])])
        np.testing.assert_allclose(b, s, rtol=1e-12, atol=0)


def test_batched_finite_difference_map_matches_scipy_fd():
    """optimize_hyperparameters with the batched forward-difference gradient (two perturbed evaluations in flight)
    takes the same L-BFGS-B / SLSQP path as scipy's own finite differences: same points, same formula."""
    import warnings
    import gptools_amd as g
    rs = np.random.RandomState(9)
    X = rs.rand(500, 2)
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(500)
    for method in ("L-BFGS-B", "SLSQP"):
        res = {}
        for batch in (True, False):
            k = g.SquaredExponentialKernel(num_dim=2, initial_params=[1.0, 0.5, 0.5], param_bounds=[(0.05, 10.0)] * 3)
            gp = g.GaussianProcess(k, X=X, y=y, err_y=0.05)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                r, _ = gp.optimize_hyperparameters(method=method, random_starts=0, batch_fd=batch,
                                                   opt_kwargs={"options": {"maxiter": 25}})
            res[batch] = r
        assert res[True].nit == res[False].nit, method
        np.testing.assert_allclose(res[True].x, res[False].x, rtol=1e-9, err_msg=method)
        np.testing.assert_allclose(res[True].fun, res[False].fun, rtol=1e-12, err_msg=method)
        assert res[True].nfev < res[False].nfev          # the perturbed points no longer count as objective calls


def test_helper_stream_schedule_agrees_with_sequential(ctx):
    """Above n = 12288 a slice of every large trailing update runs on the helper stream (third HIP stream on the
    reserved CUs).  Same ll / log|K| as the schedule without it and as the sequential (no look-ahead) schedule; the
    factor reproduces K_tot."""
    N, d = 12800, 2
    X, n, y = c3_inputs(N, d)
    n[:] = 0
    p = np.array([1.0, 0.3, 0.3])
    err = 0.05 * np.ones(N)
    ctx.set_data(X, n)
    try:
        with_helper = ctx.fit(0, p, 0.0, y, err, 1e2 * EPS)
        alpha = ctx.get_alpha(N)
        ctx.set_option("helper_tf", 0)
        without = ctx.fit(0, p, 0.0, y, err, 1e2 * EPS)
        ctx.set_option("lookahead", 0)
        seq = ctx.fit(0, p, 0.0, y, err, 1e2 * EPS)
    finally:
        ctx.set_option("helper_tf", 35)
        ctx.set_option("lookahead", 1)
    for other in (without, seq):
        assert abs(with_helper[0] - other[0]) <= 1e-11 * abs(other[0])
        assert abs(with_helper[1] - other[1]) <= 1e-12 * abs(other[1])
    # K_tot alpha = y on a sample of rows (K rows rebuilt by the pair kernel)
    rows = np.arange(0, N, 997)
    Kr = ctx.kbuild(0, p, X[rows], n[rows], X, n)
    Kr[np.arange(len(rows)), rows] += err[rows] ** 2 + 1e2 * EPS
    np.testing.assert_allclose(Kr.dot(alpha), y[rows], rtol=0, atol=1e-7)


@pytest.mark.parametrize("kern", ["se", "m52"])
def test_linear_transform_path_on_device(g, oracle, kern):
    """`T` (line-integral style observations, ref gaussian_process.py:1443-1451, :966-970) assembled on the device --
    K-builder + two MFMA GEMMs -- against the host formula T (K + noise) T^T + diag(err^2) + eps I built from the
    oracle's K and factored by LAPACK; then predict (mean, covariance) against the same host algebra."""
    import scipy.linalg
    rs = np.random.RandomState(12)
    Nx, Ny, d = 1111, 203, 2                    # neither a multiple of 16 / 64: exercises every padding
    X = rs.rand(Nx, d)
    n = np.zeros((Nx, d), dtype=int)
    if kern == "m52":
        n[-50:, 0] = 1                          # some latent derivative values take part in the transform too
    T = rs.rand(Ny, Nx) / Nx
    f = np.sin(3 * X.sum(1))
    y = T.dot(f) + 1e-3 * rs.randn(Ny)
    p = np.array([1.1, 0.35, 0.45])
    noise = 0.02
    nk = g.DiagonalNoiseKernel(num_dim=d, initial_noise=noise, noise_bound=(0.0, 1.0))
    gp = g.GaussianProcess(make_kernel(g, kern, d, p), noise_k=nk)
    gp.add_data(X, y, err_y=1e-3, n=n, T=T)
    gp.compute_K_L_alpha_ll()
    assert gp._fit_mode == "kernel"             # the device path, not gpt_fit_matrix
    K = oracle.kbuild(kern, p, X, n)
    Ktot = T.dot(K + noise ** 2 * np.eye(Nx)).dot(T.T) + 1e-6 * np.eye(Ny) + 1e2 * EPS * np.eye(Ny)
    L = scipy.linalg.cholesky(Ktot, lower=True)
    alpha = scipy.linalg.cho_solve((L, True), y)
    ll = -0.5 * y.dot(alpha) - np.log(np.diag(L)).sum() - 0.5 * Ny * np.log(2 * np.pi)
    assert abs(gp.ll - gp.hyperprior(gp.params) - ll) <= 1e-8 * abs(ll)      # gp.ll is the log-posterior
    assert_close(gp.L, L, rtol=1e-6, atol_scale=1e-9)
    Xs = rs.rand(40, d)
    ns = np.zeros((40, d), dtype=int)
    ns[20:, 1] = 1 if kern == "se" else 0
    mean, cov = gp.predict(Xs, n=ns, return_cov=True)
    Ks = T.dot(oracle.kbuild(kern, p, X, n, Xs, ns))                       # (Ny, M)
    v = scipy.linalg.solve_triangular(L, Ks, lower=True)
    np.testing.assert_allclose(mean, Ks.T.dot(alpha), rtol=0, atol=1e-7)
    np.testing.assert_allclose(cov, oracle.kbuild(kern, p, Xs, ns) - v.T.dot(v), rtol=0, atol=1e-7)
    # hyperparameter update keeps T resident; adding data re-uploads it
    v0 = gp.update_hyperparameters([1.0, 0.3, 0.4, 0.03])
    gp.add_data(rs.rand(5, d), rs.randn(5) * 0.01, err_y=1e-3)
    v1 = gp.update_hyperparameters([1.0, 0.3, 0.4, 0.03])
    assert np.isfinite(v0) and np.isfinite(v1) and gp.T.shape == (Ny + 5, Nx + 5)


def test_sum_of_native_kernels_on_device(g, oracle):
    """k1 + k2 (SumKernel, ref kernel/core.py:549-584) of native kernels: accumulated builder passes on the device
    (gpt_fit_sum) against the oracle's K1 + K2 factored by LAPACK; predict uses the same sum; the batched evaluator
    goes through it too."""
    import scipy.linalg
    rs = np.random.RandomState(21)
    N, d = 900, 2
    X = rs.rand(N, d)
    n = np.zeros((N, d), dtype=int)
    n[-100:, 1] = 1
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(N)
    p1, p2 = np.array([1.0, 0.3, 0.5]), np.array([0.4, 1.5, 2.0])
    k = make_kernel(g, "se", d, p1) + make_kernel(g, "m52", d, p2)
    gp = g.GaussianProcess(k, X=X, y=y, err_y=0.05, n=n)
    gp.compute_K_L_alpha_ll()
    assert gp._fit_mode == "kernel" and len(gp._native_terms()) == 2
    K = oracle.kbuild("se", p1, X, n) + oracle.kbuild("m52", p2, X, n)
    Ktot = K + (0.05 ** 2 + 1e2 * EPS) * np.eye(N)
    L = scipy.linalg.cholesky(Ktot, lower=True)
    alpha = scipy.linalg.cho_solve((L, True), y)
    ll = -0.5 * y.dot(alpha) - np.log(np.diag(L)).sum() - 0.5 * N * np.log(2 * np.pi)
    assert abs(gp.ll - gp.hyperprior(gp.params) - ll) <= 1e-8 * abs(ll)
    assert_close(gp.L, L, rtol=1e-6, atol_scale=1e-9)
    Xs = rs.rand(30, d)
    ns = np.zeros((30, d), dtype=int)
    ns[15:, 0] = 1
    Ks = oracle.kbuild("se", p1, X, n, Xs, ns) + oracle.kbuild("m52", p2, X, n, Xs, ns)
    v = scipy.linalg.solve_triangular(L, Ks, lower=True)
    Kss = oracle.kbuild("se", p1, Xs, ns) + oracle.kbuild("m52", p2, Xs, ns)
    mean, std = gp.predict(Xs, n=ns)
    np.testing.assert_allclose(mean, Ks.T.dot(alpha), rtol=0, atol=1e-7)
    np.testing.assert_allclose(std ** 2, np.diag(Kss - v.T.dot(v)), rtol=0, atol=1e-7)
    mean2, cov = gp.predict(Xs, n=ns, return_cov=True)
    np.testing.assert_allclose(cov, Kss - v.T.dot(v), rtol=0, atol=1e-7)
    thetas = [list(p1) + list(p2), list(1.1 * p1) + list(0.9 * p2), list(0.8 * p1) + list(1.3 * p2)]
    b = gp.ll_batch(thetas)                          # gpt_fit_batch_sum: the sum in the batched evaluator, one launch sequence
    s = np.array([-gp.update_hyperparameters(t) for t in thetas])
    assert np.array_equal(b, s), (b, s)
    gp.batch_grid_max_n = 10                         # (the thread route gives the same bits)
    assert np.array_equal(gp.ll_batch(thetas), s)
    # the C ABI directly: per-element noise variances and targets, a non-positive-definite element reported alone
    from gptools_amd import _lib
    c = _lib.Context(0)
    c.set_data(X, n)
    P = np.array(thetas)
    nv = np.array([0.0, 0.02, -50.0])
    Y = np.vstack([y, y + 0.01, y])
    llb, ldb, info = c.fit_batch_sum([KID["se"], KID["m52"]], P, [3, 3], nv, Y, np.full(N, 0.05), 1e2 * EPS)
    assert info[2] > 0 and info[0] == 0 and info[1] == 0
    for e in (0, 1):
        l1, d1 = c.fit_sum([KID["se"], KID["m52"]], [P[e, :3], P[e, 3:]], nv[e], Y[e], np.full(N, 0.05), 1e2 * EPS)
        assert (l1, d1) == (llb[e], ldb[e])
    c.close()


def test_draw_sample_cholesky_and_eig(g):
    """draw_sample (ref gaussian_process.py:1155-1330): with given random variables the samples are
    mean + L u with L the lower Cholesky factor (GPU) of cov + diag_factor eps I, or Q sqrt(Lambda); the resident
    factor of the fit is untouched; predict(return_samples=True) returns them in the full_output dict."""
    import scipy.linalg
    rs = np.random.RandomState(4)
    X = rs.rand(200, 1)
    y = np.sin(6 * X[:, 0]) + 0.05 * rs.randn(200)
    gp = g.GaussianProcess(make_kernel(g, "se", 1, [1.0, 0.2]), X=X, y=y, err_y=0.05)
    Xs = np.linspace(0, 1, 150)[:, None]
    out = gp.predict(Xs, full_output=True)
    u = rs.randn(150, 7)
    loaded = out["cov"] + 1e3 * EPS * np.eye(150)
    # with the identity as "random variables" the call returns mean + L: L is lower triangular and L L^T is the loaded
    # covariance (the matrix is numerically singular, so L itself is compared through that product, not entrywise)
    L = gp.draw_sample(Xs, rand_vars=np.eye(150)) - out["mean"][:, None]
    assert np.abs(np.triu(L, 1)).max() == 0.0
    np.testing.assert_allclose(L.dot(L.T), loaded, rtol=0, atol=1e-12)
    s_chol = gp.draw_sample(Xs, rand_vars=u)
    np.testing.assert_allclose(s_chol, out["mean"][:, None] + L.dot(u), rtol=0, atol=1e-12)
    s_eig = gp.draw_sample(Xs, rand_vars=u, method="eig", num_eig=10, modify_sign="left value")
    assert s_eig.shape == (150, 7)
    # the eigen square root reproduces the covariance restricted to its 10 leading modes
    lam, Q = scipy.linalg.eigh(loaded, subset_by_index=(140, 149))
    Q[:, Q[0, :] < 0] *= -1
    np.testing.assert_allclose(s_eig, out["mean"][:, None] + (Q * np.sqrt(lam)).dot(u[:10]), rtol=0, atol=1e-8)
    uu = rs.rand(150, 3)
    s_uni = gp.draw_sample(Xs, rand_vars=uu, rand_type="uniform")
    import scipy.stats
    np.testing.assert_allclose(s_uni, out["mean"][:, None] + L.dot(scipy.stats.norm.ppf(uu)), rtol=0, atol=1e-8)
    again = gp.predict(Xs, full_output=True)                       # the fit's factor is still resident and valid
    np.testing.assert_array_equal(again["mean"], out["mean"])
    np.random.seed(5)
    full = gp.predict(Xs, full_output=True, return_samples=True, num_samples=4)
    assert full["samp"].shape == (150, 4)
    assert np.abs(full["samp"] - out["mean"][:, None]).max() < 6 * out["std"].max() + 1e-6
    with pytest.raises(ValueError):
        gp.draw_sample(Xs, rand_vars=u, rand_type="triangular")


def test_draw_sample_device_route_matches_host_route(g):
    """gpt_cov_sample: draw_sample(rand_vars=...) keeps the predictive covariance on the device (gpt_predict with
    cov_out NULL), factors it there and returns mean + L u; the host route (mean= and cov= handed in, factor through
    gpt_potrf_host) is the same arithmetic on the same matrix.  M not a multiple of 128, derivative rows, noise=True,
    and the fit's factor survives."""
    rs = np.random.RandomState(14)
    X = rs.rand(700, 2)
    y = np.sin(4 * X[:, 0]) * np.cos(3 * X[:, 1]) + 0.05 * rs.randn(700)
    k = make_kernel(g, "se", 2, [1.3, 0.35, 0.5])
    nk = g.DiagonalNoiseKernel(2, initial_noise=0.08, fixed_noise=True)
    gp = g.GaussianProcess(k, noise_k=nk, X=X, y=y, err_y=0.03)
    ll0 = gp.update_hyperparameters(gp.free_params[:]) if hasattr(gp, "update_hyperparameters") else None
    M = 333
    Xs = rs.rand(M, 2)
    ns = np.zeros((M, 2), dtype=int)
    ns[::7, 0] = 1
    u = rs.randn(M, 5)
    for noise in (False, True):
        out = gp.predict(Xs, n=ns, noise=noise, full_output=True)
        host = gp.draw_sample(Xs, n=ns, rand_vars=u, mean=out["mean"], cov=out["cov"])
        dev = gp.draw_sample(Xs, n=ns, rand_vars=u, noise=noise)
        assert dev.shape == (M, 5)
        # (the loaded covariance is close to singular without the noise term: compare at the size of the jitter's root)
        np.testing.assert_allclose(dev, host, rtol=0, atol=1e-6 if not noise else 1e-10)
        Ld = gp.draw_sample(Xs, n=ns, rand_vars=np.eye(M), noise=noise) - out["mean"][:, None]
        assert np.abs(np.triu(Ld, 1)).max() == 0.0
        np.testing.assert_allclose(Ld.dot(Ld.T), out["cov"] + 1e3 * EPS * np.eye(M), rtol=0, atol=1e-11)
        with pytest.raises(ValueError):                      # (M x M) . (40 x 5): the reference's own shape error
            gp.draw_sample(Xs, n=ns, rand_vars=u, num_eig=40, noise=noise)
    if ll0 is not None:
        assert gp.update_hyperparameters(gp.free_params[:]) == ll0
    again = gp.predict(Xs, n=ns, full_output=True)
    np.testing.assert_array_equal(again["mean"], gp.predict(Xs, n=ns, return_std=False))
    # the C-ABI refuses a second draw from a covariance that was consumed
    with pytest.raises(Exception):
        gp._ctx.cov_sample(0.0, u)
    gp._ctx.predict(Xs, ns, 2, device_cov=True)
    with pytest.raises(Exception):                           # wrong number of rows for the resident covariance
        gp._ctx.cov_sample(0.0, u[:100])


def test_device_ll_gradient_against_host_path_and_finite_differences(g):
    """gpt_ll_grad (K_tot^-1 on the device + fused pair pass) against the reference-shaped host path
    (dK per parameter, two triangular solves each, ref gaussian_process.py:1471-1520) and against central finite
    differences of ll; SE with derivative rows, a free noise parameter, and a two-term sum."""
    import warnings
    rs = np.random.RandomState(31)
    N, d = 700, 2
    X = rs.rand(N, d)
    n = np.zeros((N, d), dtype=int)
    n[-60:, 0] = 1
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(N)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for build in ("single", "sum"):
            def make():
                k = make_kernel(g, "se", d, [1.1, 0.4, 0.6])
                if build == "sum":
                    k = k + make_kernel(g, "se", d, [0.3, 1.5, 2.5])
                nk = g.DiagonalNoiseKernel(num_dim=d, initial_noise=0.1, noise_bound=(0.0, 5.0))
                return g.GaussianProcess(k, noise_k=nk, X=X, y=y, err_y=0.02, n=n, use_hyper_deriv=True)
            gp = make()
            theta = np.array(gp.free_params[:], dtype=float)
            val, grad = gp.update_hyperparameters(theta)
            # host path: force it by pretending the fit was not a native one
            gp2 = make()
            gp2.use_hyper_deriv = False
            gp2.update_hyperparameters(theta)
            gp2._fit_mode = "matrix"
            gp2._compute_ll_deriv()
            assert_close(-grad, gp2.ll_deriv, rtol=1e-7, atol_scale=1e-9)
            # central differences of the log-posterior
            gp3 = make()
            gp3.use_hyper_deriv = False
            fd = np.zeros_like(theta)
            for i in range(len(theta)):
                h = 1e-5 * max(1.0, abs(theta[i]))
                tp, tm = theta.copy(), theta.copy()
                tp[i] += h
                tm[i] -= h
                fd[i] = (-gp3.update_hyperparameters(tp) + gp3.update_hyperparameters(tm)) / (2 * h)
            np.testing.assert_allclose(-grad, fd, rtol=2e-5, atol=1e-4 * np.abs(fd).max())


def test_panel_stream_update_waits_for_a_slow_k_build(g, oracle):
    """Look-ahead with the panel stream applying the first update itself (purg_rows) while the K build is SLOW (general-order
    Matern: Temme's K_nu per pair) and the first panel quick (ramp: 128 columns): the update must not touch columns the
    build has not written yet.  ll against the CPU oracle."""
    from gptools_amd import _lib
    N, d = 6800, 2
    X, n, y = c3_inputs(N, d)
    n[:] = 0
    p = np.array([1.0, 1.3, 0.35, 0.3])           # sigma_f, nu, l_1, l_2
    err = 0.05 * np.ones(N)
    ref = oracle.fit("matern", p, X, n, y, err, chol="scipy")
    c = _lib.Context(0)
    c.set_data(X, n)
    for opts in ({}, {"ramp": 1, "purg_rows": 1024}, {"ramp": 1, "purg_rows": 1024, "edge_flags": 0}):
        for k_, v_ in opts.items():
            c.set_option(k_, v_)
        for rep in range(2):
            got = c.fit(_lib.KERNEL_MATERN, p, 0.0, y, err, 1e2 * EPS)
            assert abs(got[0] - ref["ll_data"]) <= 1e-8 * abs(ref["ll_data"]), (opts, got, ref["ll_data"])


@pytest.mark.parametrize("kern,N,d,M", [("m52", 4200, 3, 5), ("se", 1500, 2, 700), ("m52", 2300, 3, 1100)])
def test_predict_result_paths_agree_and_match_the_oracle(oracle, kern, N, d, M):
    """gpt_predict's covariance goes to the host by three routes -- asynchronous DMA into pinned memory (gpt_host_alloc),
    the pinned staging ring for pageable memory, or not at all (cov_out = NULL: device-resident) -- and is computed as a
    lower-triangular SYRK in block columns with a mirror kernel per block row: same numbers on every route, exactly
    symmetric, std = sqrt(diag), and mean / variance / covariance within 1e-6 sigma_f^2 of the CPU oracle (ref
    gaussian_process.py:965-1006).  M = 5 at N = 4200 takes the few-rows solve (1024-wide block inverses), M = 700 / 1100
    cross block-column and 64-padding boundaries."""
    from gptools_amd import _lib
    X, n, y = c3_inputs(N, d)
    if kern == "se":
        n[:] = 0
    err = np.full(N, 0.05)
    p = np.concatenate(([1.0], 0.3 * np.ones(d)))
    c = _lib.Context(0)
    c.set_data(X, n)
    c.fit(KID[kern], p, 0.0, y, err, 1e2 * EPS)
    rs = np.random.RandomState(M)
    Xs = rs.rand(M, d)
    ns = np.zeros((M, d), dtype=np.int32)
    if kern == "m52":
        ns[::7, 0] = 1
    Xs_, ns_ = _lib.f64(Xs), _lib.i32(ns)
    out = {}
    for route in ("pageable", "pinned", "device"):
        mean, std = np.full(M, np.nan), np.full(M, np.nan)
        cov = {"pageable": np.full((M, M), np.nan), "pinned": _lib.pinned_empty((M, M), min_bytes=0), "device": None}[route]
        _lib.check(c._lib.gpt_predict(c.handle, _lib.dptr(Xs_), _lib.iptr(ns_), M, 2, None, None, _lib.dptr(mean),
                                      _lib.dptr(std), None if cov is None else _lib.dptr(cov)))
        out[route] = (mean, std, None if cov is None else np.array(cov))
    m1, s1, _ = c.predict(Xs, ns, 1)
    ref = oracle.fit(kern, p, X, n, y, err, chol="scipy")
    mr, sr, cr = oracle.predict(kern, p, X, n, ref["L"], ref["alpha"], Xs, ns, want_cov=True)
    cov = out["pageable"][2]
    assert np.array_equal(cov, out["pinned"][2]) and np.array_equal(cov, cov.T)
    for route in out:
        assert np.array_equal(out[route][0], out["pageable"][0]) and np.array_equal(out[route][1], out["pageable"][1])
    assert np.array_equal(out["pageable"][1], np.sqrt(np.diag(cov)))
    assert np.abs(out["pageable"][0] - mr).max() <= 1e-6 and np.abs(m1 - mr).max() <= 1e-6
    assert np.abs(cov - cr).max() <= 1e-6 and np.abs(s1 ** 2 - sr ** 2).max() <= 1e-6
    c.close()


@pytest.mark.parametrize("N,M", [(4200, 40), (8300, 64), (8300, 7), (8300, 200)])
def test_few_rows_solve_split_along_k_repeats_and_agrees_with_the_unsplit_sums(N, M):
    """Triangular solves with at most 128 right-hand sides split their long-k GEMMs into chunks summed in chunk order (option
    splitk, api.hip gemm_nt_few): the same bits on every call, and variance / covariance within 1e-11 sigma_f^2 of the unsplit
    sums (the oracle comparison of the split path is test_predict_result_paths_agree_and_match_the_oracle at N = 4200, M = 5).
    N = 4200 uses the 1024-wide block inverses, N = 8300 the 2048-wide ones with a ragged rest; at M = 200 the solve is the
    halving recursion of many-row solves and only the covariance's V V^T (k = N against 7 x 7 tiles) is split."""
    from gptools_amd import _lib
    d = 2
    X, n, y = c3_inputs(N, d)
    err = np.full(N, 0.05)
    p = np.array([1.0, 0.3, 0.3])
    c = _lib.Context(0)
    c.set_data(X, n)
    c.fit(KID["m52"], p, 0.0, y, err, 1e2 * EPS)
    rs = np.random.RandomState(N + M)
    Xs, ns = rs.rand(M, d), np.zeros((M, d), dtype=np.int32)
    ns[::5, 1] = 1
    res = {}
    for sk in (512, 0, 512):
        c.set_option("splitk", sk)
        res.setdefault(sk, []).append(c.predict(Xs, ns, 2))
    a, b = res[512]
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    u = res[0][0]
    assert np.array_equal(a[0], u[0])                          # the mean does not pass through the solve
    assert np.abs(a[2] - u[2]).max() <= 1e-11 and np.abs(a[1] ** 2 - u[1] ** 2).max() <= 1e-11
    assert not np.array_equal(a[2], u[2])                      # (the split path did run)
    c.close()


@pytest.mark.parametrize("case", ["T", "mixed_sum_fixed_m52", "large_block_path"])
def test_device_ll_gradient_with_transform_mixed_sum_and_block_inverses(g, case):
    """gpt_ll_grad beyond plain squared-exponential fits (VERDICT r2 missing #3; ref gaussian_process.py:1471-1520):
    with a linear transform T (the pair pass over the latent points against T^T K_tot^-1 T), with a SumKernel whose
    non-SE term has all its parameters fixed, and at a size where the triangular inverse takes the GEMM-only route
    (512-wide block inverses, ragged last block) -- each against the reference-shaped host path (dK per parameter, two
    triangular solves) and, for T, central differences of the log-posterior."""
    rs = np.random.RandomState(5)
    d = 2
    if case == "T":
        Nx, Ny = 900, 330
        X = rs.rand(Nx, d)
        n = np.zeros((Nx, d), dtype=int)
        n[-40:, 1] = 1
        T = rs.rand(Ny, Nx) / Nx
        y = T.dot(np.sin(3 * X.sum(1))) + 1e-3 * rs.randn(Ny)
    else:
        Nx = 2900 if case == "large_block_path" else 800
        X = rs.rand(Nx, d)
        n = np.zeros((Nx, d), dtype=int)
        n[-70:, 0] = 1
        T = None
        y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(Nx)

    def make():
        k = make_kernel(g, "se", d, [1.1, 0.4, 0.6])
        if case == "mixed_sum_fixed_m52":
            k = k + make_kernel(g, "m52", d, [0.4, 1.5, 2.0], fixed_params=[True, True, True])
        nk = g.DiagonalNoiseKernel(num_dim=d, initial_noise=0.05, noise_bound=(0.0, 5.0))
        gp_ = g.GaussianProcess(k, noise_k=nk, use_hyper_deriv=True)
        gp_.add_data(X, y, err_y=0.02 if T is None else 1e-3, n=n, T=T)
        return gp_
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = make()
        theta = np.array(gp.free_params[:], dtype=float)
        assert len(theta) == 4
        val, grad = gp.update_hyperparameters(theta)
        assert gp._fit_mode == "kernel"
        gp2 = make()
        gp2.use_hyper_deriv = False
        gp2.update_hyperparameters(theta)
        gp2._fit_mode = "matrix"                     # forces the host path of _compute_ll_deriv
        gp2._compute_ll_deriv()
        assert_close(-grad, gp2.ll_deriv, rtol=1e-6, atol_scale=1e-8)
        if case == "T":
            gp3 = make()
            gp3.use_hyper_deriv = False
            fd = np.zeros_like(theta)
            for i in range(len(theta)):
                h = 1e-5 * max(1.0, abs(theta[i]))
                tp, tm = theta.copy(), theta.copy()
                tp[i] += h
                tm[i] -= h
                fd[i] = (-gp3.update_hyperparameters(tp) + gp3.update_hyperparameters(tm)) / (2 * h)
            # kernel parameters only: for the noise parameter the reference differentiates 2 sigma_n I over the observations
            # WITHOUT the transform (ref :1482-1488) although K_tot holds T (sigma_n^2 I) T^T -- reproduced (drop-in), so that
            # entry follows the reference's formula (checked against the host path above), not the function's slope
            np.testing.assert_allclose(-grad[:3], fd[:3], rtol=5e-5, atol=1e-4 * np.abs(fd[:3]).max())


@pytest.mark.parametrize("kern,N,d,deriv", [("m52", 700, 3, True), ("se", 1100, 2, False), ("se", 130, 1, False),
                                            ("m52", 2700, 2, True)])
def test_fit_batch_is_bit_identical_to_single_fits(oracle, kern, N, d, deriv):
    """gpt_fit_batch (every kernel of the small-N factorisation carries the batch in a grid dimension; SURVEY 8f-2, ref
    gaussian_process.py:1607-1692 / :723-735) against one gpt_fit per hyperparameter vector: ll and log-determinant
    bit for bit (same kernels, same tile choice, same summation orders), per-element targets and noise variances, an element
    that is not positive definite reported through info without disturbing the others; elements of the batch also against
    the CPU oracle (ll 1e-9, log-determinant 1e-10)."""
    from gptools_amd import _lib
    X, n, y = c3_inputs(N, d)
    if not deriv:
        n[:] = 0
    err = np.full(N, 0.05)
    rs = np.random.RandomState(N)
    B = 23 if N < 2048 else 7
    P = np.column_stack([0.5 + rs.rand(B)] + [0.1 + 0.6 * rs.rand(B) for _ in range(d)])
    nv = 0.01 * rs.rand(B)
    Y = y[None, :] + 0.01 * rs.randn(B, N)
    nv[5] = -10.0                                     # K + noise_var I is not positive definite
    c = _lib.Context(0)
    c.set_data(X, n)
    ll, ld, info = c.fit_batch(KID[kern], P, nv, Y, err, 1e2 * EPS)
    assert info[5] > 0 and (np.delete(info, 5) == 0).all()
    for b in range(B):
        if b == 5:
            with pytest.raises(np.linalg.LinAlgError):
                c.fit(KID[kern], P[b], nv[b], Y[b], err, 1e2 * EPS)
            continue
        l1, d1 = c.fit(KID[kern], P[b], nv[b], Y[b], err, 1e2 * EPS)
        assert (l1, d1) == (ll[b], ld[b]), (b, l1 - ll[b], d1 - ld[b])
        if b % 4 == 0 or N <= 600:           # ... and every (N <= 600) / every fourth element against the CPU oracle
            ref = oracle.fit(kern, P[b], X, n, Y[b], err, noise_var=nv[b], chol="c" if N <= 600 else "scipy")
            assert abs(ll[b] - ref["ll_data"]) <= 1e-9 * abs(ref["ll_data"]), (b, ll[b], ref["ll_data"])
            assert abs(ld[b] - ref["logdet_half"]) <= 1e-10 * max(1.0, abs(ref["logdet_half"])), b
    # a second batch of another size on the same context, after single fits
    ll2, ld2, info2 = c.fit_batch(KID[kern], P[:3], nv[:3], Y[:3], err, 1e2 * EPS)
    assert np.array_equal(ll2, ll[:3]) and np.array_equal(ld2, ld[:3]) and not info2.any()
    c.close()


def test_product_kernel_is_a_native_term_of_the_fused_builder(g, golden, oracle):
    """k1 * k2 of two native kernels (ref kernel/core.py:587-671) as GPT_KERNEL_PRODUCT: the Leibniz sum runs per pair on the
    device -- pair list (gpt_kpairs2) and Gram matrix (gpt_kbuild2) against the golden g9 vectors from the reference and against
    the host product rule over the oracle's factors; the model (k1 * k2 + k3) fits through the fused builder (gpt_fit_terms:
    fit mode "kernel", no host-assembled K_tot), predicts, and ll_batch agrees with sequential evaluation."""
    from gptools_amd import _lib
    G = golden("g9_product")
    mk = lambda cls, p, **kw: cls(num_dim=2, initial_params=list(p), param_bounds=[(0.0, 1e3)] * len(p), **kw)
    k = mk(g.SquaredExponentialKernel, G["sese_p1"]) * mk(g.SquaredExponentialKernel, G["sese_p2"])
    assert k._native_factors() is not None
    assert_close(k(G["sese_Xi"], G["sese_Xj"], G["sese_ni"], G["sese_nj"]), G["sese_k"], rtol=1e-11, msg="SE * SE pairs")
    ks = mk(g.SquaredExponentialKernel, G["sese_p1"]) * mk(g.Matern52Kernel, G["sese_p2"])
    assert_close(ks(G["sese_Xi"], G["sese_Xj"], G["sem_ni"], G["sem_nj"]), G["sem_k"], rtol=1e-11, msg="SE * M52 pairs")
    with pytest.raises(NotImplementedError):
        ks(G["sese_Xi"], G["sese_Xj"], G["sem_ni"], G["sem_nj"], hyper_deriv=0)
    with pytest.raises(ValueError):                       # Matern52 factor: order 2 in a point (ref matern.py:545-546)
        ks(G["sese_Xi"][:2], G["sese_Xj"][:2], np.array([[2, 0], [0, 0]]), np.zeros((2, 2), int))
    # Gram matrix: device product against products of the oracle's factor matrices (no derivatives) and, with derivative
    # rows, against the device pair list
    rs = np.random.RandomState(3)
    N, d = 500, 2
    X = rs.rand(N, d)
    n = np.zeros((N, d), dtype=int)
    n[-60:, 1] = 1
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(N)
    p1, p2, p3 = [1.2, 0.5, 0.7], [0.8, 0.3, 0.9], [0.4, 1.5, 2.0]
    gp0 = g.GaussianProcess(mk(g.SquaredExponentialKernel, p1) * mk(g.Matern52Kernel, p2))
    Kd = gp0.compute_Kij(X, None, n, None)
    n0 = np.zeros_like(n)
    K00 = gp0.compute_Kij(X, None, n0, None)
    assert_close(K00, oracle.kbuild("se", p1, X, n0) * oracle.kbuild("m52", p2, X, n0), rtol=1e-12, msg="Gram, no derivatives")
    ii, jj = np.meshgrid(np.arange(N - 80, N), np.arange(0, N, 7), indexing="ij")
    pl = gp0.k(X[ii.ravel()], X[jj.ravel()], n[ii.ravel()], n[jj.ravel()])
    assert_close(Kd[ii.ravel(), jj.ravel()], pl, rtol=1e-13, msg="Gram vs pair list")
    # the host product rule over GPU factor calls (what round 2 did for every product) gives the same numbers
    class Host(g.ProductKernel):
        def _native_factors(self):
            return None
    kh = Host(mk(g.SquaredExponentialKernel, p1), mk(g.Matern52Kernel, p2))
    assert_close(pl, kh(X[ii.ravel()], X[jj.ravel()], n[ii.ravel()], n[jj.ravel()]), rtol=1e-12, msg="device vs host Leibniz")
    # fit / predict / batch with k1 * k2 + k3
    kern = mk(g.SquaredExponentialKernel, p1) * mk(g.Matern52Kernel, p2) + mk(g.SquaredExponentialKernel, p3)
    gp = g.GaussianProcess(kern, X=X, y=y, err_y=0.05, n=n)
    gp.compute_K_L_alpha_ll()
    assert gp._fit_mode == "kernel"
    Kh = kh(np.repeat(X, N, 0), np.tile(X, (N, 1)), np.repeat(n, N, 0), np.tile(n, (N, 1))).reshape(N, N) + oracle.kbuild("se", p3, X, n)
    import scipy.linalg
    Kt = Kh + (0.05 ** 2 + 1e2 * EPS) * np.eye(N)
    L = scipy.linalg.cholesky(Kt, lower=True)
    alpha = scipy.linalg.cho_solve((L, True), y)
    ll = -0.5 * y.dot(alpha) - np.log(np.diag(L)).sum() - 0.5 * N * np.log(2 * np.pi)
    assert abs(gp.ll - gp.hyperprior(gp.params) - ll) <= 1e-9 * abs(ll)
    Xs = rs.rand(30, d)
    ns = np.zeros((30, d), dtype=int)
    ns[::5, 0] = 1
    mean, std = gp.predict(Xs, n=ns)
    Ks = (kh(np.repeat(X, 30, 0), np.tile(Xs, (N, 1)), np.repeat(n, 30, 0), np.tile(ns, (N, 1))).reshape(N, 30) +
          oracle.kbuild("se", p3, X, n, Xs, ns))
    np.testing.assert_allclose(mean, Ks.T.dot(alpha), rtol=0, atol=1e-7)
    theta = np.array(gp.free_params[:], dtype=float)
    pts = [theta, theta * 1.05, theta * 0.97]
    np.testing.assert_allclose(gp.ll_batch(pts), [-gp.update_hyperparameters(p) for p in pts], rtol=1e-12)


def test_ll_batch_grid_path_and_thread_path_agree(g):
    """GaussianProcess.ll_batch at small N goes through gpt_fit_batch (one launch sequence for the whole list); above
    ``batch_grid_max_n`` -- forced here -- through one context and host thread per evaluation in flight.  Same numbers bit for
    bit on both routes and from one update_hyperparameters call per vector, for a Matern-5/2 GP with derivative rows and a
    free noise parameter, a rational-quadratic GP, out-of-bounds vectors (-inf) and a non-positive-definite one (-inf)."""
    rs = np.random.RandomState(17)
    N, d = 600, 2
    X = rs.rand(N, d)
    n = np.zeros((N, d), dtype=int)
    n[-50:, 0] = 1
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(N)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for kind in ("m52", "rq"):
            if kind == "m52":
                k = make_kernel(g, "m52", d, [1.0, 0.4, 0.6], param_bounds=[(0.2, 5.0), (0.05, 2.0), (0.05, 2.0)])
                nk = g.DiagonalNoiseKernel(num_dim=d, initial_noise=0.05, noise_bound=(0.0, 1.0))
                pts = [[1.0, 0.4, 0.6, 0.05], [1.3, 0.3, 0.5, 0.02], [0.1, 0.4, 0.6, 0.05], [0.9, 0.5, 0.7, 0.0]]
            else:
                k = g.RationalQuadraticKernel(num_dim=d, initial_params=[1.0, 1.7, 0.4, 0.6],
                                              param_bounds=[(0.2, 5.0), (0.1, 10.0), (0.05, 2.0), (0.05, 2.0)])
                nk = None
                pts = [[1.0, 1.7, 0.4, 0.6], [1.2, 2.5, 0.3, 0.5], [1.0, 0.05, 0.4, 0.6]]
            gp = g.GaussianProcess(k, noise_k=nk, X=X, y=y, err_y=0.03, n=n)
            grid = gp.ll_batch(pts)
            gp.batch_grid_max_n = 10                    # forces the two-contexts / two-threads route
            thr = gp.ll_batch(pts)
            gp.batch_grid_max_n = 4096
            gp.batch_grid_bytes = 3 * 8 * 640 * 640     # (chunks of 3: the memory cap of the grid route)
            assert np.array_equal(gp.ll_batch(pts), grid)
            seq = np.array([-gp.update_hyperparameters(p) for p in pts])
            assert np.array_equal(grid, thr) and np.array_equal(grid, seq), (kind, grid, thr, seq)
            assert np.isneginf(grid[2]) and np.isfinite(grid[:2]).all()
    # an element that is not positive definite inside a batch: -inf for it alone (duplicate points, no noise, no jitter)
    X2 = np.vstack([X[:200], X[:1]])
    y2 = np.concatenate([y[:200], y[:1] + 1.0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        k = make_kernel(g, "se", d, [1.0, 0.4, 0.6], param_bounds=[(0.2, 5.0), (0.05, 2.0), (0.05, 2.0)])
        nk = g.DiagonalNoiseKernel(num_dim=d, initial_noise=0.05, noise_bound=(0.0, 1.0))
        gp = g.GaussianProcess(k, noise_k=nk, X=X2, y=y2, err_y=0.0, diag_factor=0.0)
        out = gp.ll_batch([[1.0, 0.4, 0.6, 0.05], [1.0, 0.4, 0.6, 0.0], [1.1, 0.5, 0.6, 0.02]])
        assert np.isfinite(out[0]) and np.isneginf(out[1]) and np.isfinite(out[2])


def test_flag_mode_fit_beside_a_batch_on_another_thread_keeps_flag_edges():
    """gpt_fit_batch (EvalScope never_flags) started while a flag-mode evaluation is in flight waits for it instead of
    filling the chip beside its spinning kernels; afterwards a lone evaluation still runs on flag edges (no bounded wait tripped)
    and every result is the sequential one."""
    import threading
    from gptools_amd import _lib
    a, b = _lib.Context(0), _lib.Context(0)
    N, d = 2500, 2
    X, n, y = c3_inputs(N, d)
    p = np.array([1.0, 0.3, 0.3])
    err = 0.05 * np.ones(N)
    a.set_data(X, n)
    Nb = 700
    b.set_data(X[:Nb], n[:Nb])
    P = np.tile(np.array([1.0, 0.3, 0.4]), (16, 1)) * (1.0 + 0.01 * np.arange(16))[:, None]
    Yb = np.tile(y[:Nb], (16, 1))
    ref_a = a.fit(1, p, 0.0, y, err, 1e2 * EPS)
    ref_b = b.fit_batch(1, P, np.zeros(16), Yb, err[:Nb], 1e2 * EPS)
    out, errs = {"a": [], "b": []}, []

    def run_a():
        try:
            for _ in range(40):
                out["a"].append(a.fit(1, p, 0.0, y, err, 1e2 * EPS))
        except Exception as e:          # noqa
            errs.append(e)

    def run_b():
        try:
            for _ in range(40):
                out["b"].append(b.fit_batch(1, P, np.zeros(16), Yb, err[:Nb], 1e2 * EPS))
        except Exception as e:          # noqa
            errs.append(e)

    ta, tb = threading.Thread(target=run_a), threading.Thread(target=run_b)
    ta.start(); tb.start(); ta.join(); tb.join()
    assert not errs, errs
    assert all(r == ref_a for r in out["a"])
    assert all(all(np.array_equal(u, v) for u, v in zip(r, ref_b)) for r in out["b"])
    import time
    time.sleep(0.15)                                  # (the contention window of un-announced overlap)
    e0 = a.edge_count
    assert a.fit(1, p, 0.0, y, err, 1e2 * EPS) == ref_a
    assert a.edge_count > e0, "the process left flag edges for good"
    a.close(); b.close()


@pytest.mark.parametrize("kern,N,d", [("m52", 1408, 3), ("se", 2047, 2), ("se", 3000, 2), ("m52", 1024, 3), ("se", 1100, 2)])
def test_alpha_by_wide_steps_matches_the_oracle_and_the_narrow_form(oracle, kern, N, d):
    """alpha = L^-T z (ref gaussian_process.py:1462) in 512-wide steps against the batched block inverses (api.hip ensure_alpha,
    solve.hip launch_trsv_lt_wide), with a ragged tail of 128-wide steps (N = 1408, 3000), exactly whole blocks (1024) and just
    below a block (2047): against the oracle's alpha, against K_tot alpha = y, and the block inverses themselves through
    cho_solve / solve_L of a few right-hand sides."""
    from gptools_amd import _lib
    X, n, y = c3_inputs(N, d)
    p = np.concatenate(([1.0], 0.3 * np.ones(d)))
    err = 0.05 * np.ones(N)
    ref = oracle.fit(kern, p, X, n, y, err, chol="scipy")
    c = _lib.Context(0)
    try:
        c.set_data(X, n)
        c.fit(KID[kern], p, 0.0, y, err, 1e2 * EPS)
        a = c.get_alpha(N)
        scale = np.abs(ref["alpha"]).max()
        np.testing.assert_allclose(a, ref["alpha"], rtol=0, atol=2e-7 * scale)
        K = oracle.kbuild(kern, p, X, n)
        K[np.diag_indices(N)] += err ** 2 + 1e2 * EPS
        np.testing.assert_allclose(K.dot(a), y, rtol=0, atol=1e-7 * max(1.0, np.abs(y).max()))
        B = np.random.RandomState(3).randn(N, 3)
        Z = c.cho_solve(B.copy())
        np.testing.assert_allclose(K.dot(Z), B, rtol=0, atol=1e-6 * np.abs(B).max())
    finally:
        c.close()


@pytest.mark.parametrize("N", [1408, 3000, 4608])
def test_eager_alpha_and_the_one_launch_block_inverses(oracle, N):
    """Option eager_alpha: the fit itself enqueues alpha behind the factorisation and lands it in pinned memory (ref
    gaussian_process.py:1462 computes alpha in every evaluation) -- the same bits as gpt_get_alpha after a plain fit, also when a
    non-positive-definite evaluation came in between.  The 512-wide block inverses behind it come out of one launch
    (solve.hip trinv512_kernel; N = 4608: nine blocks, 288 workgroups): against rounds 2-4's recursion over 15 launches (option
    binv_launches) alpha, a solve and a many-points predict agree to rounding, and alpha matches the oracle."""
    from gptools_amd import _lib
    d = 2
    X, n, y = c3_inputs(N, d)
    p = np.array([1.0, 0.3, 0.3])
    err = 0.05 * np.ones(N)
    ref = oracle.fit("m52", p, X, n, y, err, chol="scipy")
    scale = np.abs(ref["alpha"]).max()
    rs = np.random.RandomState(N)
    Xs, ns = rs.rand(300, d), np.zeros((300, d), dtype=np.int32)
    B = rs.randn(N, 2)
    c = _lib.Context(0)
    try:
        c.set_data(X, n)
        out = {}
        for mode in (0, 1):
            c.set_option("binv_launches", mode)
            c.fit(KID["m52"], p, 0.0, y, err, 1e2 * EPS)
            out[mode] = (c.get_alpha(N), c.cho_solve(B.copy()), c.predict(Xs, ns, 1)[1])
        np.testing.assert_allclose(out[0][0], ref["alpha"], rtol=0, atol=2e-7 * scale)
        for u, v in zip(out[0], out[1]):
            assert np.abs(u - v).max() <= 1e-10 * max(1.0, np.abs(v).max())
        c.set_option("binv_launches", 0)
        c.set_option("eager_alpha", 1)
        ll = c.fit(KID["m52"], p, 0.0, y, err, 1e2 * EPS)
        assert np.array_equal(c.get_alpha(N), out[0][0])
        with pytest.raises(np.linalg.LinAlgError):
            c.fit(KID["m52"], p, 0.0, y, 0.0 * err, -2.0)          # K - 2 I: not positive definite
        with pytest.raises(Exception):
            c.get_alpha(N)                                        # (no factor, no alpha)
        assert c.fit(KID["m52"], p, 0.0, y, err, 1e2 * EPS) == ll
        assert np.array_equal(c.get_alpha(N), out[0][0])
        assert np.array_equal(c.predict(Xs, ns, 1)[1], out[0][2])
    finally:
        c.close()


@pytest.mark.parametrize("N", [1024, 2048, 2560, 1920])
def test_eager_alpha_pad_leaf_beside_the_substitution(oracle, N):
    """Option defer_pad (default on; eager evaluations with N a multiple of 512): the last 128 columns of the padded factor -- the
    augmented row and the padding -- are factored on the main stream beside alpha's substitution, which starts behind the last REAL
    leaf.  Same bits as with everything on the panel stream: ll, alpha, L, a predict -- and, with the squared-exponential kernel, the
    analytic gradient (gpt_ll_grad inverts the WHOLE padded factor, pad block included); a failed pivot and non-finite data are still
    reported; N = 1920 (not a multiple of 512) takes the old route either way."""
    from gptools_amd import _lib
    d = 2
    X, n, y = c3_inputs(N, d)
    p = np.array([1.0, 0.3, 0.3])
    err = 0.05 * np.ones(N)
    ref = oracle.fit("m52", p, X, n, y, err, chol="scipy")
    rs = np.random.RandomState(N)
    Xs, ns = rs.rand(50, d), np.zeros((50, d), dtype=np.int32)
    c = _lib.Context(0)
    try:
        c.set_data(X, n)
        c.set_option("eager_alpha", 1)
        out = {}
        for mode in (0, 1, 0, 1):
            c.set_option("defer_pad", mode)
            ll = c.fit(KID["m52"], p, 0.0, y, err, 1e2 * EPS)
            got = (ll, c.get_alpha(N), c.get_L(N), c.predict(Xs, ns, 1)[1])
            if mode in out:
                for u, v in zip(out[mode], got):
                    assert np.array_equal(np.asarray(u), np.asarray(v))
            out[mode] = got
            with pytest.raises(np.linalg.LinAlgError):
                c.fit(KID["m52"], p, 0.0, y, 0.0 * err, -2.0)          # K - 2 I: not positive definite
            ybad = y.copy()
            ybad[N // 2] = np.inf
            with pytest.raises(np.linalg.LinAlgError):
                c.fit(KID["m52"], p, 0.0, ybad, err, 1e2 * EPS)        # non-finite data: the augmented row's pivot fails
            with pytest.raises(np.linalg.LinAlgError):
                c.fit(KID["m52"], p, 0.0, 1e160 * y, err, 1e2 * EPS)   # z.z overflows the pad pivot
        for u, v in zip(out[0], out[1]):
            assert np.array_equal(np.asarray(u), np.asarray(v))
        assert abs(out[1][0][0] - ref["ll_data"]) <= 1e-9 * abs(ref["ll_data"])
        np.testing.assert_allclose(out[1][1], ref["alpha"], rtol=0, atol=2e-7 * np.abs(ref["alpha"]).max())
        # the event schedule (flag edges off): the pad leaf moves there too, same bits with and without
        c.set_option("edge_flags", 0)
        ev = []
        for mode in (0, 1):
            c.set_option("defer_pad", mode)
            ev.append((c.fit(KID["m52"], p, 0.0, y, err, 1e2 * EPS), c.get_alpha(N), c.get_L(N)))
        assert ev[0][0] == ev[1][0] and np.array_equal(ev[0][1], ev[1][1]) and np.array_equal(ev[0][2], ev[1][2])
        assert abs(ev[1][0][0] - ref["ll_data"]) <= 1e-9 * abs(ref["ll_data"])
        c.set_option("edge_flags", 1)
        n0 = np.zeros_like(n)
        c.set_data(X, n0)
        grads = []
        for mode in (0, 1):
            c.set_option("defer_pad", mode)
            ll = c.fit(KID["se"], p, 0.0, y, err, 1e2 * EPS)
            grads.append((ll, c.ll_grad([0, 0, 0], [0, 1, 2])))
        assert grads[0][0] == grads[1][0] and np.array_equal(grads[0][1], grads[1][1])
    finally:
        c.close()


# ---------------------------------------------------------------- eager alpha by panel geometry -------
# The panel geometry of the look-ahead factorisation at the default schedule options (ramp 0, nb_early 0, inner 0), mirrored from
# gptools_amd/csrc/api_schedule.inc (potrf_enqueue) and api_solve.inc (enqueue_early_block_inverses): the schedule's edge cases
# live at particular geometries, not at particular sizes, so the cases below are chosen by the class they reach, and the test
# asserts that class through the mirror before it touches the GPU.
PANEL_EXT = 128          # GPT_PANEL_EXT (api_schedule.inc)
BINV_NB = 512            # GPT_BINV_NB (api_grad.inc): the early block inverses are whole 512 x 512 diagonal blocks


def sched_outer_width(NP, nb_outer=0):
    """outer_width(): the panel width, by size unless set."""
    if nb_outer > 0:
        return nb_outer
    return 256 if NP <= 5120 else 384 if NP <= 12288 else 640


def sched_geometry(N, nb_outer=0):
    """What potrf_enqueue does at the padded order NP of N points: the panel widths (the widths loop), the end column of the last
    panel the main stream waits for (it does so only for a panel whose update reaches a column, u0 = c0 + w + EXT < n), how many
    early block inverses an eager evaluation builds -- `early`: the whole 512-blocks left of the last panel, unless all of them
    (enqueue_early_block_inverses), and no further than that wait -- and how many the schedule built before it capped them there
    (`early_unawaited`), and, where factor_and_ll sets defer_pad_leaf, how many real leaves hold back an update of the pad block
    (panel_ext: cend == n)."""
    NP = -(-(N + 1) // 128) * 128
    nbo = sched_outer_width(NP, nb_outer)
    widths, c0 = [], 0
    while c0 < NP:
        widths.append(min(nbo, NP - c0))
        c0 += widths[-1]
    awaited, c0 = 0, 0
    for w in widths:
        if c0 + w + PANEL_EXT < NP:
            awaited = c0 + w
        c0 += w

    nblk, b = NP // BINV_NB, (NP - widths[-1]) // BINV_NB
    early_unawaited = b if len(widths) >= 2 and nblk >= 2 and 0 < b < nblk else 0
    early = min(early_unawaited, awaited // BINV_NB)
    defer_pad = N % 512 == 0 and N >= 1024 and NP == N + 128 and len(widths) >= 2
    pad_leaves, c0 = 0, 0
    for w in widths:
        if min(c0 + w + PANEL_EXT, NP) == NP:
            pad_leaves += sum(1 for lc in range(c0, c0 + w, 128) if lc + 128 < NP)
        c0 += w
    return dict(NP=NP, widths=widths, awaited=awaited, early=early, early_unawaited=early_unawaited,
                defer_pad=defer_pad, pad_leaves=pad_leaves if defer_pad else 0, helper=NP > 12288)


def sched_class(geo):
    """race: early block inverses over columns of a panel the main stream has not waited for (before the fix); pad_cap: more
    real leaves reach the pad block than the eight the schedule used to hold back; control: neither."""
    assert geo["early"] * BINV_NB <= geo["awaited"] and geo["early"] <= geo["early_unawaited"]
    if geo["early_unawaited"] != geo["early"]:
        return "race"
    return "pad_cap" if geo["pad_leaves"] > 8 else "control"


GEOMETRY_CASES = [
    # (N, nb_outer, class, what else the case is meant to hit)
    pytest.param(2000, 640, "race", lambda g_: g_["widths"][-1] == 128 and g_["NP"] % 512 == 0, id="race-2000-640"),
    pytest.param(3500, 1152, "race", lambda g_: g_["widths"][-1] == 128, id="race-3500-1152"),
    pytest.param(1000, 896, "race", lambda g_: g_["widths"] == [896, 128] and g_["awaited"] == 0, id="race-1000-896-no-update"),
    pytest.param(14720, 0, "race", lambda g_: g_["helper"] and g_["widths"][0] == 640, id="race-14720-helper"),
    pytest.param(32700, 0, "race", lambda g_: g_["NP"] == 32768, id="race-32700"),
    pytest.param(2560, 1280, "pad_cap", lambda g_: g_["pad_leaves"] == 10, id="padcap-2560-1280"),
    pytest.param(4608, 1152, "pad_cap", lambda g_: g_["pad_leaves"] == 9, id="padcap-4608-1152"),
    pytest.param(2100, 640, "control", lambda g_: g_["widths"][-1] == 256, id="control-2100-640"),
    pytest.param(2560, 640, "control", lambda g_: g_["widths"][-1] == 128 and g_["defer_pad"], id="control-2560-640-pad-alone"),
    pytest.param(14848, 0, "control", lambda g_: g_["helper"] and g_["defer_pad"], id="control-14848"),
    pytest.param(4000, 768, "control", lambda g_: g_["NP"] % 768 == 256, id="control-4000-768"),
    pytest.param(3000, 0, "control", lambda g_: not g_["defer_pad"], id="control-3000"),
    pytest.param(4608, 0, "control", lambda g_: g_["defer_pad"] and g_["widths"][-1] == 128, id="control-4608"),
]


def test_schedule_geometry_mirror_at_the_benchmark_sizes():
    """The mirror itself: the early block inverses change only where the race was -- at the benchmark's sizes (C2-C5, with the
    default widths and bench.py --nb's usual values) an eager evaluation keeps its schedule; and the classes the table relies on
    are where the mirror says they are (every 2560 rows with the default widths above 12288)."""
    for N in (4096, 8192, 16384, 32768):
        for nb in (0, 256, 384, 512, 640):
            geo = sched_geometry(N, nb)
            assert geo["early"] == geo["early_unawaited"] and geo["pad_leaves"] <= 8, (N, nb, geo)
    races = [N for N in range(12800, 33000, 128) if sched_class(sched_geometry(N)) == "race"]
    assert races == list(range(14720, 32768, 2560)), races


def _lbits(L):
    """A digest of a factor (get_L of N = 32700 is 8.5 GB: one at a time)."""
    import hashlib
    return hashlib.sha1(np.ascontiguousarray(L).view(np.uint8)).hexdigest()


def _eager_case_inputs(N, d=2):
    X, n, y = c3_inputs(N, d)
    rs = np.random.RandomState(N)
    return X, n, y, np.array([1.0, 0.3, 0.3]), 0.05 * np.ones(N), rs.randn(N, 2), rs.rand(64, d), np.zeros((64, d), dtype=np.int32)


@pytest.mark.parametrize("N,nb_outer,cls,pin", GEOMETRY_CASES)
def test_eager_alpha_at_every_panel_geometry(oracle, N, nb_outer, cls, pin):
    """an eager evaluation builds the inverses of the 512-wide diagonal blocks under the last panel, on the main stream;
    they must cover only columns of panels the main stream has waited for -- not the second-to-last panel in front of a 128-wide
    last one, which nothing waits for -- and the pad block's held-back updates must be all of them, in leaf order.  At every class
    of geometry (race / pad_cap / control, sched_geometry), on flag and on event edges (and at N = 14720 without the helper stream):
    the eager fit's ll, L, alpha and the cho_solve and predict behind it are the plain route's bits; where the pad leaf moves to the
    main stream (N % 512 == 0) defer_pad 0 and 1 agree bit for bit, the analytic gradient included; ll and alpha match the oracle
    up to N = 14720 (8 s on 8 CPU cores; at N = 32700 the plain route is the reference)."""
    geo = sched_geometry(N, nb_outer)
    assert sched_class(geo) == cls and pin(geo), geo
    from gptools_amd import _lib
    X, n, y, p, err, B, Xs, ns = _eager_case_inputs(N)

    def route(c, eager):
        c.set_option("eager_alpha", eager)
        ll = c.fit(KID["m52"], p, 0.0, y, err, 1e2 * EPS)
        out = {"ll": ll, "alpha": c.get_alpha(N), "cho_solve": c.cho_solve(B.copy())}
        out["mean"], out["std"], _ = c.predict(Xs, ns, 1)
        out["L"] = _lbits(c.get_L(N))
        return out

    def same(got, want, what):
        for k_, v_ in want.items():
            assert np.array_equal(np.asarray(got[k_]), np.asarray(v_)), "%s: %s differs (N = %d, nb_outer = %d, %s)" % (
                what, k_, N, nb_outer, cls)

    c = _lib.Context(0)
    try:
        c.set_data(X, n)
        c.set_option("nb_outer", nb_outer)
        first = None
        for ef in (1, 0):
            c.set_option("edge_flags", ef)
            for helper_tf in ((None, 0) if N == 14720 else (None,)):
                if helper_tf is not None:
                    c.set_option("helper_tf", helper_tf)
                plain = route(c, 0)
                eager = route(c, 1)
                same(eager, plain, "eager against plain, edge_flags %d%s" % (ef, "" if helper_tf is None else ", helper_tf 0"))
                if geo["defer_pad"]:
                    c.set_option("defer_pad", 0)
                    same(route(c, 1), eager, "eager, defer_pad 0 against 1, edge_flags %d" % ef)
                    c.set_option("defer_pad", 1)
                if helper_tf is not None:
                    c.set_option("helper_tf", 45)          # (the default, api.hip)
                first = first or eager
        c.set_option("edge_flags", 1)
        if geo["defer_pad"]:
            c.set_data(X, np.zeros_like(n))
            grads = []
            for mode in (0, 1):
                c.set_option("defer_pad", mode)
                ll = c.fit(KID["se"], p, 0.0, y, err, 1e2 * EPS)
                grads.append((ll, c.ll_grad([0, 0, 0], [0, 1, 2])))
            assert grads[0][0] == grads[1][0] and np.array_equal(grads[0][1], grads[1][1])
    finally:
        c.close()
    if N <= 14720:
        ref = oracle.fit("m52", p, X, n, y, err, chol="scipy")
        assert abs(first["ll"][0] - ref["ll_data"]) <= 1e-9 * abs(ref["ll_data"])
        np.testing.assert_allclose(first["alpha"], ref["alpha"], rtol=0, atol=2e-7 * np.abs(ref["alpha"]).max())


def test_eager_alpha_race_geometries_under_stream_jitter():
    """The race and pad_cap geometries under GPT_JITTER (a delay kernel of up to 1 ms in front of every dense launch, ~0.25 ms on
    average): the second-to-last panel's leaves -- two delayed launches each -- then fall milliseconds behind the main stream's
    last update, the window in which the early block inverses used to read them.  Eager evaluations in a fresh process, three
    each: alpha and a cho_solve must hash to the undisturbed plain route's bits."""
    import hashlib
    import subprocess
    cases = [tuple(c_.values[:2]) for c_ in GEOMETRY_CASES if c_.values[2] in ("race", "pad_cap") and c_.values[0] < 20000]
    code = (
        "import sys, hashlib, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from gptools_amd import _lib\n"
        "from test_gpu_parity import _eager_case_inputs\n"
        "c = _lib.Context(0)\n"
        "c.set_option('eager_alpha', 1)\n"
        "for N, nb in %r:\n"
        "    X, n, y, p, err, B, Xs, ns = _eager_case_inputs(N)\n"
        "    c.set_data(X, n)\n"
        "    c.set_option('nb_outer', nb)\n"
        "    for rep in range(3):\n"
        "        ll, ld = c.fit(1, p, 0.0, y, err, 1e2 * sys.float_info.epsilon)\n"
        "        print('EAGER', N, nb, repr(ll), repr(ld), hashlib.sha1(c.get_alpha(N).tobytes()).hexdigest(),\n"
        "              hashlib.sha1(c.cho_solve(B.copy()).tobytes()).hexdigest(), flush=True)\n") % (ROOT, os.path.join(ROOT, "tests"), cases)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GPT_JITTER="1000"), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [l.split()[1:] for l in out.stdout.splitlines() if l.startswith("EAGER")]
    assert len(got) == 3 * len(cases)
    from gptools_amd import _lib
    c = _lib.Context(0)
    try:
        for N, nb in cases:
            X, n, y, p, err, B, Xs, ns = _eager_case_inputs(N)
            c.set_data(X, n)
            c.set_option("nb_outer", nb)
            ll, ld = c.fit(KID["m52"], p, 0.0, y, err, 1e2 * EPS)
            want = [repr(ll), repr(ld), hashlib.sha1(c.get_alpha(N).tobytes()).hexdigest(),
                    hashlib.sha1(c.cho_solve(B.copy()).tobytes()).hexdigest()]
            for g_ in got:
                if (int(g_[0]), int(g_[1])) == (N, nb):
                    assert g_[2:] == want, ((N, nb), g_, want)
    finally:
        c.close()


def test_block_inverse_extents_fit_predict_then_gradient(g):
    """at N = 512 k - 128 the solves (predict with std) and gpt_ll_grad ask for block inverses over different
    extents; fit -> predict(std) -> ll_grad must give the gradient ll_grad gives straight after the fit."""
    N, d = 1408, 2
    rs = np.random.RandomState(11)
    X = rs.rand(N, d)
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(N)
    from gptools_amd import _lib
    p = np.array([1.1, 0.4, 0.6])
    err = 0.05 * np.ones(N)
    n = np.zeros((N, d), dtype=int)
    res = []
    for with_predict in (False, True):
        c = _lib.Context(0)
        try:
            c.set_data(X, n)
            c.fit(0, p, 0.0, y, err, 1e2 * EPS)
            if with_predict:
                c.predict(rs.rand(300, d), np.zeros((300, d), int), 1)
                c.solve_L(rs.randn(N, 2))
            res.append(c.ll_grad([0, 0, 0], [0, 1, 2]))
        finally:
            c.close()
    np.testing.assert_array_equal(res[0], res[1])
    assert np.all(np.isfinite(res[0]))


def test_transform_gradient_does_not_read_unwritten_scratch(g):
    """with a transform and N % 64 != 0 the T^T W T product reads W up to round_up(N, 64); the scratch matrix is
    pre-filled with NaN (context option debug_poison) and the gradient must still be the clean one."""
    rs = np.random.RandomState(5)
    d, Nx, Ny = 2, 700, 330
    X = rs.rand(Nx, d)
    n = np.zeros((Nx, d), dtype=int)
    T = rs.rand(Ny, Nx) / Nx
    y = T.dot(np.sin(3 * X.sum(1))) + 1e-3 * rs.randn(Ny)
    grads = []
    for poison in (0, 1):
        k = make_kernel(g, "se", d, [1.1, 0.4, 0.6])
        nk = g.DiagonalNoiseKernel(num_dim=d, initial_noise=0.05, noise_bound=(0.0, 5.0))
        gp = g.GaussianProcess(k, noise_k=nk, use_hyper_deriv=True)
        gp.add_data(X, y, err_y=1e-3, n=n, T=T)
        gp._ctx.set_option("debug_poison", poison)
        val, grad = gp.update_hyperparameters(np.array(gp.free_params[:], dtype=float))
        grads.append(np.array(grad))
    assert np.all(np.isfinite(grads[1]))
    np.testing.assert_array_equal(grads[0], grads[1])


@pytest.mark.parametrize("case", ["product_plus_term", "transform", "transform_product"])
def test_fit_batch_terms_products_and_transform_bit_identical(g, case):
    """gpt_fit_batch_terms: a batch of evaluations of a model with a PRODUCT term (k1 * k2 + k3) and / or a
    linear TRANSFORM T (K_tot = T (K + noise) T^T + ..., two batched GEMMs with the shared T) carries, per element, the very
    bits one gpt_fit_terms call returns; and GaussianProcess.ll_batch routes such models through it (same values as one
    update_hyperparameters per vector).  ref: gaussian_process.py:1607-1692 (the reference's grids take any model)."""
    from gptools_amd import _lib
    rs = np.random.RandomState(21)
    d, Nx = 2, 700
    X = rs.rand(Nx, d)
    n = np.zeros((Nx, d), dtype=int)
    n[-50:, 0] = 1
    with_T = case.startswith("transform")
    Ny = 260 if with_T else Nx
    T = rs.rand(Ny, Nx) / Nx if with_T else None
    f = np.sin(3 * X.sum(1))
    y = (T.dot(f) if with_T else f) + 1e-2 * rs.randn(Ny)
    err = np.full(Ny, 0.02)
    B = 9

    def terms(b):
        s = 1.0 + 0.05 * b
        if case == "transform":
            return [(0, np.array([1.1 * s, 0.4, 0.6]))]
        return [(0, np.array([1.1 * s, 0.4, 0.6]), 1, np.array([0.9, 1.5 * s, 2.0])), (4, np.array([0.3, 1.7, 0.8 * s, 0.9]))]
    c = _lib.Context(0)
    try:
        c.set_data(X, n)
        if with_T:
            c.set_T(T)
        nv = 1e-3 * (1.0 + np.arange(B))
        Y = y[None, :] + 1e-3 * rs.randn(B, Ny)
        ll, ld, info = c.fit_batch_terms([terms(b) for b in range(B)], nv, Y, err, 1e2 * EPS)
        assert not info.any()
        for b in range(B):
            l1, d1 = c.fit_terms(terms(b), nv[b], Y[b], err, 1e2 * EPS)
            assert (l1, d1) == (ll[b], ld[b]), (case, b, l1 - ll[b], d1 - ld[b])
    finally:
        c.close()
    # through the plugin API: ll_batch == one update_hyperparameters per vector
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        k = make_kernel(g, "se", d, [1.1, 0.4, 0.6])
        if case != "transform":
            k = k * make_kernel(g, "m52", d, [0.9, 1.5, 2.0]) + g.RationalQuadraticKernel(
                num_dim=d, initial_params=[0.3, 1.7, 0.8, 0.9], param_bounds=[(0.0, 1e3)] * 4)
        gp = g.GaussianProcess(k, noise_k=g.DiagonalNoiseKernel(num_dim=d, initial_noise=0.03, noise_bound=(0.0, 5.0)))
        gp.add_data(X, y, err_y=0.02, n=n, T=T)
        theta = np.array(gp.free_params[:], dtype=float)
        pts = [theta * (1.0 + 0.02 * i) for i in range(5)]
        calls = []
        orig = gp._ctx.fit_batch_terms
        gp._ctx.fit_batch_terms = lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1]
        vals = gp.ll_batch(pts)
        assert calls, "ll_batch did not take the batched evaluator for case %s" % case
        one = np.array([-gp.update_hyperparameters(p) for p in pts])
        np.testing.assert_array_equal(vals, one)



# ---------------------------------------------------------------- G12: independent evaluations and samples against the reference
def _g12_grid_gp(g, G, kern):
    cls = g.SquaredExponentialKernel if kern == "se" else g.Matern52Kernel
    k = cls(num_dim=2, initial_params=[1.2, 0.35, 0.4], param_bounds=[(1e-3, 10.0)] * 3, fixed_params=[False, False, True])
    return g.GaussianProcess(k, X=G["grid_X"], y=G["grid_y"], err_y=0.05, n=G["grid_n"])


@pytest.mark.parametrize("kern", KERNELS)
def test_g12_compute_ll_matrix_against_the_reference(g, golden, oracle, kern):
    """compute_ll_matrix (ref gaussian_process.py:1607-1692) on the grid the REFERENCE walked (tests/golden/gen_golden.py g12):
    same grid axes, same shape (first free parameter = first axis), the out-of-bounds row -inf, the log-posterior at every
    other point to 1e-9, the GP left at its hyperparameters with its own ll -- through each of the three evaluators
    (one launch sequence for the batch = gpt_fit_batch_terms, two contexts in flight, one call per point), and the C-ABI
    batch entry itself (gpt_fit_batch) against the fixture's data term and the CPU oracle."""
    G = golden("g12_batch_samples")
    want = G["grid_%s_ll" % kern]
    for mode in ("grid", "threads", "sequential"):
        gp = _g12_grid_gp(g, G, kern)
        if mode == "threads":
            gp.batch_grid = 1
        elif mode == "sequential":
            gp.batch_concurrency = 1
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ll, pv = gp.compute_ll_matrix([(0.4, 12.0), (0.1, 0.9)], [5, 4])
        assert ll.shape == want.shape == (5, 4)
        np.testing.assert_array_equal(pv[0], G["grid_%s_p0" % kern])
        np.testing.assert_array_equal(pv[1], G["grid_%s_p1" % kern])
        np.testing.assert_array_equal(np.isneginf(ll), np.isneginf(want), err_msg=mode)
        assert np.isneginf(want[4]).all() and np.isfinite(want[:4]).all()
        assert_close(ll, want, rtol=1e-9, atol_scale=0.0, msg=mode)
        np.testing.assert_array_equal(gp.free_params[:], G["grid_%s_free_after" % kern])
        assert abs(gp.ll - G["grid_%s_ll_after" % kern]) <= 1e-9 * abs(G["grid_%s_ll_after" % kern])
    # the C ABI's batch entry on the same grid: data term = fixture - log prior (uniform over the bounds: a constant)
    gp = _g12_grid_gp(g, G, kern)
    prior = gp.hyperprior(gp.params)
    pts = [(a, b) for a in G["grid_%s_p0" % kern][:4] for b in G["grid_%s_p1" % kern]]
    P = np.array([[a, b, 0.4] for a, b in pts])
    X, n, y = G["grid_X"], G["grid_n"], G["grid_y"]
    from gptools_amd import _lib
    c = _lib.Context(0)
    c.set_data(X, n)
    ll, ld, info = c.fit_batch(KID[kern], P, np.zeros(len(P)), np.tile(y, (len(P), 1)), np.full(len(y), 0.05), 1e2 * EPS)
    c.close()
    assert not info.any()
    assert_close(ll + prior, want[:4].ravel(), rtol=1e-9, atol_scale=0.0, msg="gpt_fit_batch vs reference")
    for b in range(len(P)):
        ref = oracle.fit(kern, P[b], X, n, y, np.full(len(y), 0.05))
        assert abs(ll[b] - ref["ll_data"]) <= 1e-9 * abs(ref["ll_data"])
        assert abs(ld[b] - ref["logdet_half"]) <= 1e-10 * max(1.0, abs(ref["logdet_half"]))


def test_g12_ll_matrix_three_free_parameters_noise_kernel_gamma_prior(g, golden):
    """compute_ll_matrix with ONE (bounds, num_pts) pair for three free parameters -- sigma_f, l_1 and the noise kernel's
    sigma_n -- under a Gamma hyperprior (the prior term varies over the grid): reference fixture, 1e-9."""
    G = golden("g12_batch_samples")
    k = g.SquaredExponentialKernel(num_dim=2, initial_params=[1.0, 0.3, 0.5], fixed_params=[False, False, True],
                                   hyperprior=g.GammaJointPriorAlt([1.0, 0.4, 0.5], [0.5, 0.2, 0.3]))
    nk = g.DiagonalNoiseKernel(num_dim=2, initial_noise=0.1, fixed_noise=False, noise_bound=(1e-3, 1.0))
    for conc in (2, 1):
        gp = g.GaussianProcess(k, noise_k=nk, X=G["grid_X"], y=G["grid_y"], err_y=0.02, n=G["grid_n"])
        gp.batch_concurrency = conc
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ll, pv = gp.compute_ll_matrix((0.05, 0.8), 3)
        assert ll.shape == (3, 3, 3)
        np.testing.assert_array_equal(np.asarray(pv), G["grid3_p"])
        assert_close(ll, G["grid3_ll"], rtol=1e-9, atol_scale=0.0)


@pytest.mark.parametrize("tag", ["fd", "hd"])
def test_g12_random_starts_against_the_reference(g, golden, tag):
    """optimize_hyperparameters(random_starts=5) (ref gaussian_process.py:689-735, :2443-2486): with numpy's global state
    seeded like the generator's, the starts drawn from the hyperprior are the reference's draws bit for bit; each start's
    SLSQP run ends where the reference's did; the start with the lowest objective is the one returned, all five count as
    completed, and the GP is left at that optimum.  'fd': scipy's finite differences (through the batched evaluator
    here), 'hd': use_hyper_deriv=True (the analytic gradient, gpt_ll_grad).  Tolerances: objective 2e-6 absolute -- SLSQP's own
    stopping rule is ftol = 1e-6 on the objective, and forward differences with h = 1.5e-8 turn the 1e-12 agreement of two ll
    values into 1e-4 of gradient, so two correct implementations stop within that of each other, not closer -- and location
    2e-3 relative (the objective is flat to ~1e-6 over that range)."""
    G = golden("g12_batch_samples")

    def make():
        k = g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 0.3], param_bounds=[(0.05, 20.0), (0.02, 3.0)])
        return g.GaussianProcess(k, X=G["rs_X"], y=G["rs_y"], err_y=0.05, n=G["rs_n"], use_hyper_deriv=(tag == "hd"))
    gp = make()
    np.random.seed(4242)
    free = ~np.asarray(gp.fixed_params[:], dtype=bool)
    draws = np.atleast_2d(gp.hyperprior.random_draw(size=5).T)[:, free]
    np.testing.assert_array_equal(draws, G["rs_%s_draws" % tag])
    per = G["rs_%s_per_start" % tag]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for s, want in zip(draws, per):                     # one start at a time: where each of them ends
            gp1 = make()
            gp1.free_params = s
            r, cnt = gp1.optimize_hyperparameters(method="SLSQP", random_starts=0)
            assert cnt == 1 and bool(r.success) == bool(want[3])
            assert abs(r.fun - want[2]) <= 2e-6, (s, r.fun, want[2])
            np.testing.assert_allclose(r.x, want[:2], rtol=2e-3)
        np.random.seed(4242)
        res, count = gp.optimize_hyperparameters(method="SLSQP", random_starts=5, num_proc=0)
    assert count == int(G["rs_%s_count" % tag]) == 5
    assert abs(res.fun - G["rs_%s_fun" % tag]) <= 2e-6
    np.testing.assert_allclose(res.x, G["rs_%s_x" % tag], rtol=2e-3)
    assert res.fun <= per[:, 2].min() + 2e-6                                   # the best start is the one returned
    np.testing.assert_array_equal(gp.free_params[:], res.x)                     # ... and the GP is left there
    assert abs(gp.ll - G["rs_%s_ll_after" % tag]) <= 2e-6
    assert abs(gp.ll + res.fun) <= 1e-12 * abs(res.fun)


@pytest.mark.parametrize("kern", KERNELS)
def test_g12_draw_sample_and_predict_samples_against_the_reference(g, golden, kern):
    """draw_sample(rand_vars=u) (ref gaussian_process.py:1155-1330) and predict(return_samples / full_MC) (:990-1005)
    against samples the REFERENCE produced from the same u: Cholesky route (device: gpt_predict with the covariance left in
    HBM + gpt_cov_sample; host route with mean= / cov=), diag_factor, noise=True, uniform variates through the normal
    quantile, scalar n, the eigen route with every modify_sign option and num_eig, the full_output dict, the seeded
    multivariate_normal route and full_MC's sample moments.  Tolerances: the Cholesky factor of cov + 1e3 eps I amplifies the
    1e-13 agreement of the covariances by the factor's condition -- 1e-7 absolute without the noise term, 1e-10 with it."""
    G = golden("g12_batch_samples")
    cls = g.SquaredExponentialKernel if kern == "se" else g.Matern52Kernel
    k = cls(num_dim=2, initial_params=[1.1, 0.4, 0.3], param_bounds=[(1e-3, 10.0)] * 3)
    nk = g.DiagonalNoiseKernel(num_dim=2, initial_noise=0.07, fixed_noise=True)
    gp = g.GaussianProcess(k, noise_k=nk, X=G["samp_X"], y=G["samp_y"], err_y=0.05, n=G["samp_n"])
    Xs, ns, u, uu, u6 = G["samp_Xs"], G["samp_ns"], G["samp_u"], G["samp_uu"], G["samp_u6"]
    key = "samp_%s_" % kern

    def close(a, b, atol, msg):
        a = np.asarray(a)
        assert a.shape == b.shape, msg
        np.testing.assert_allclose(a, b, rtol=0, atol=atol, err_msg=msg)
    o = gp.predict(Xs, n=ns, full_output=True, return_samples=True, samp_kwargs={"rand_vars": u})
    assert set(o) == {"mean", "std", "cov", "samp"}
    close(o["mean"], G[key + "pred_mean"], 1e-9, "mean")
    close(o["cov"], G[key + "pred_cov"], 1e-10, "cov")
    close(o["std"] ** 2, G[key + "pred_std"] ** 2, 1e-10, "std")
    close(o["samp"], G[key + "pred_samp"], 1e-7, "predict(return_samples) host route")
    np.testing.assert_array_equal(G[key + "pred_samp"], G[key + "chol"])        # (the reference's two spellings agree)
    close(gp.draw_sample(Xs, n=ns, rand_vars=u), G[key + "chol"], 1e-7, "device route")
    close(gp.draw_sample(Xs, n=ns, rand_vars=u, mean=o["mean"], cov=o["cov"]), G[key + "chol"], 1e-7, "host route")
    close(gp.draw_sample(Xs, n=ns, rand_vars=u, noise=True), G[key + "chol_noise"], 1e-10, "noise")
    close(gp.draw_sample(Xs, n=ns, rand_vars=u, diag_factor=1e6), G[key + "chol_df"], 1e-7, "diag_factor")
    close(gp.draw_sample(Xs, n=ns, rand_vars=uu, rand_type="uniform"), G[key + "chol_uniform"], 1e-7, "uniform")
    close(gp.draw_sample(Xs, n=0, rand_vars=u), G[key + "chol_scalar_n"], 1e-7, "scalar n")
    for ms in (None, "left value", "right value", "left slope", "right slope", "left concavity", "right concavity"):
        tagm = "none" if ms is None else ms.replace(" ", "_")
        got = gp.draw_sample(Xs, n=0, rand_vars=u, method="eig", modify_sign=ms, noise=True)
        if ms is None:
            # LAPACK leaves the sign of an eigenvector open; the reference does not fix it either: compare the sample's
            # deviation from the mean mode by mode only through what IS determined -- L L^T
            pm = gp.predict(Xs, n=0, noise=True, full_output=True)
            dev_g, dev_w = got - pm["mean"][:, None], G[key + "eig_none"] - pm["mean"][:, None]
            lam, Q = np.linalg.eigh(pm["cov"] + 1e3 * EPS * np.eye(len(Xs)))
            cg, cw = Q.T.dot(dev_g), Q.T.dot(dev_w)                 # = +- sqrt(lam_i) u_i row by row
            np.testing.assert_allclose(np.abs(cg), np.abs(cw), rtol=0, atol=1e-9)
            np.testing.assert_allclose(np.abs(cw), np.sqrt(lam)[:, None] * np.abs(u), rtol=0, atol=1e-9)
        else:
            close(got, G[key + "eig_" + tagm], 1e-9, "eig " + tagm)
    close(gp.draw_sample(Xs, n=0, rand_vars=u, method="eig", num_eig=5, modify_sign="left value", noise=True),
          G[key + "eig_num5"], 1e-9, "num_eig")
    np.random.seed(99)
    o = gp.predict(Xs, n=0, noise=True, full_output=True, return_samples=True, num_samples=4)
    close(o["cov"], G[key + "pred_mvn_cov"], 1e-10, "mvn cov")
    close(o["samp"], G[key + "pred_mvn_samp"], 1e-8, "seeded multivariate_normal route")
    o = gp.predict(Xs, n=0, noise=True, full_output=True, full_MC=True, num_samples=6, samp_kwargs={"rand_vars": u6}, ddof=1)
    close(o["samp"], G[key + "mc_samp"], 1e-10, "full_MC samples")
    close(o["mean"], G[key + "mc_mean"], 1e-10, "full_MC mean")
    close(o["cov"], G[key + "mc_cov"], 1e-10, "full_MC cov")
    close(o["std"], np.sqrt(np.diag(G[key + "mc_cov"])), 1e-10, "full_MC std")


# ---------------------------------------------------------------- refusals of the C ABI, entry point by entry point ----
# One rule, every entry point that carries it, through _lib.Context (the C status decides the exception class: GPT_E_ARG /
# GPT_E_VALUE -> ValueError, GPT_E_NOTIMPL -> NotImplementedError).  Everything here is refused on the host in front of any launch,
# or is a valid call.
_SE, _M52, _NOISE, _RQ, _MAT, _GIBBS = 0, 1, 2, 4, 5, 7
_P = {_SE: [1.0, 2.0], _M52: [1.0, 2.0], _RQ: [1.0, 1.5, 2.0], _MAT: [1.0, 10.5, 2.0], _GIBBS: [1.1, 0.8, 0.6, 0.3, 0.5], _NOISE: [0.1]}
_NFIT = 24


def _fit_routes(c, product):
    """name -> callable(terms) for the fit entry points that can carry `terms` (as Context.fit_terms takes them)."""
    rs = np.random.RandomState(11)
    y, err = rs.randn(_NFIT), np.full(_NFIT, 0.1)
    Y, nv = np.tile(y, (2, 1)), np.zeros(2)

    def flat(terms):
        return [np.asarray(t[1], dtype=float) for t in terms]
    routes = {
        "fit_terms": lambda terms: c.fit_terms(terms, 0.0, y, err, 0.0),
        "fit_batch_terms": lambda terms: c.fit_batch_terms([terms, terms], nv, Y, err, 0.0),
    }
    if not product:
        routes["fit_sum"] = lambda terms: c.fit_sum([t[0] for t in terms], flat(terms), 0.0, y, err, 0.0)
        routes["fit_batch_sum"] = lambda terms: c.fit_batch_sum(
            [t[0] for t in terms], np.tile(np.concatenate(flat(terms)), (2, 1)), [len(t[1]) for t in terms], nv, Y, err, 0.0)
    return routes


def _single_routes(c):
    rs = np.random.RandomState(11)
    y, err = rs.randn(_NFIT), np.full(_NFIT, 0.1)
    return {
        "fit": lambda kid, p: c.fit(kid, p, 0.0, y, err, 0.0),
        "fit_batch": lambda kid, p: c.fit_batch(kid, np.tile(np.asarray(p, dtype=float), (2, 1)), np.zeros(2), np.tile(y, (2, 1)), err, 0.0),
    }


def _refused(exc, terms, c, tag):
    """`terms` is refused with `exc` by every fit entry point that can carry it (a single non-product term: all six)."""
    product = any(len(t) == 4 for t in terms)
    for name, call in _fit_routes(c, product).items():
        with pytest.raises(exc):
            call(terms)
            pytest.fail("%s: %s accepted %r" % (tag, name, [t[0::2] for t in terms]))
    if len(terms) == 1 and not product:
        for name, call in _single_routes(c).items():
            with pytest.raises(exc):
                call(terms[0][0], terms[0][1])
                pytest.fail("%s: %s accepted kernel %d" % (tag, name, terms[0][0]))


def _fits(terms, c, tag):
    product = any(len(t) == 4 for t in terms)
    for name, call in _fit_routes(c, product).items():
        out = call(terms)
        assert np.all(np.isfinite(out[0])), (tag, name, out)
    if len(terms) == 1 and not product:
        for name, call in _single_routes(c).items():
            out = call(terms[0][0], terms[0][1])
            assert np.all(np.isfinite(out[0])), (tag, name, out)


def _points_1d(top_order, N=_NFIT):
    """N points in [0, 1], 1-D: mostly values, two first derivatives and ONE row of order `top_order` (the last)."""
    X = np.linspace(0.0, 1.0, N)[:, None]
    n = np.zeros((N, 1), dtype=int)
    n[3] = n[N // 2] = 1
    n[-1] = top_order
    return X, n


def test_fit_refusals_agree_across_the_six_fit_entry_points():
    from gptools_amd import _lib
    c = _lib.Context(0)
    try:
        t = lambda kid: (kid, _P[kid])
        prod = lambda k1, k2: (k1, _P[k1], k2, _P[k2])
        # --- orders <= 1: ids and parameter counts
        c.set_data(*_points_1d(1))
        _fits([t(_SE)], c, "plain")
        _fits([t(_RQ), prod(_SE, _GIBBS)], c, "plain sum with a product")
        _refused(ValueError, [t(_NOISE)], c, "not a native fit kernel")
        _refused(ValueError, [t(_SE), t(_NOISE)], c, "not a native fit kernel, second term")
        _refused(ValueError, [prod(_SE, _NOISE)], c, "not a native fit kernel as second factor")
        _refused(ValueError, [(_SE, [1.0, 2.0, 3.0])], c, "parameter count")
        _refused(ValueError, [(_RQ, [1.0, 2.0])], c, "parameter count")
        _refused(ValueError, [t(_SE), (_GIBBS, _P[_GIBBS][:4])], c, "parameter count, second term")
        _refused(ValueError, [(_SE, _P[_SE], _SE, [1.0])], c, "parameter count of a second factor")
        _refused(ValueError, [(_SE, [], _SE, _P[_SE])], c, "product split nparams1 = 0")
        # --- a training row of order 2: Gibbs terms
        c.set_data(*_points_1d(2))
        _fits([t(_RQ)], c, "order 2 without Gibbs")
        _refused(NotImplementedError, [t(_GIBBS)], c, "Gibbs, order 2")
        _refused(NotImplementedError, [t(_SE), t(_GIBBS)], c, "Gibbs second term, order 2")
        _refused(NotImplementedError, [prod(_SE, _GIBBS)], c, "Gibbs as second factor, order 2")
        # --- a training row of order 9: 2 * n_maxsum = 18 > GPT_RQ_MAXORD = 16
        c.set_data(*_points_1d(9))
        _refused(ValueError, [t(_RQ)], c, "RQ, order 9")
        _refused(ValueError, [t(_MAT)], c, "Matern, order 9")
        _refused(ValueError, [t(_SE), t(_RQ)], c, "RQ second term, order 9")
        _refused(ValueError, [prod(_SE, _SE)], c, "SE * SE, order 9")
        _fits([t(_SE)], c, "a lone SE term is not subject to the limit")
        # which refusal wins is decided term by term
        _refused(ValueError, [t(_RQ), t(_GIBBS)], c, "[RQ, Gibbs], order 9")
        _refused(NotImplementedError, [t(_GIBBS), t(_RQ)], c, "[Gibbs, RQ], order 9")
        # --- order 8: 16 is within the limit
        c.set_data(*_points_1d(8))
        _fits([t(_RQ)], c, "RQ, order 8")
    finally:
        c.close()


def test_test_point_refusals_agree_between_predict_and_predict_batch():
    from gptools_amd import _lib
    c = _lib.Context(0)
    rs = np.random.RandomState(12)
    y, err = rs.randn(_NFIT), np.full(_NFIT, 0.1)
    Xs = np.array([[0.21], [0.47], [0.83]])

    def ns(order):
        return np.array([[0], [order], [1]])

    def routes(terms):
        """the same model resident for gpt_predict (after gpt_fit_terms) and for gpt_predict_batch (after gpt_fit_batch_terms)"""
        c.fit_terms(terms, 0.0, y, err, 0.0)
        c.fit_batch_terms([terms, terms], np.zeros(2), np.tile(y, (2, 1)), err, 0.0)
        return {"predict": lambda n: c.predict(Xs, n, 0)[0],
                "predict_batch": lambda n: c.predict_batch(Xs, n, [1, 1], want_var=False)[0]}
    try:
        t = lambda kid: (kid, _P[kid])
        prod = lambda k1, k2: (k1, _P[k1], k2, _P[k2])
        c.set_data(*_points_1d(1))
        for terms, exc, tag in (([t(_M52)], ValueError, "M52"), ([t(_SE), prod(_SE, _M52)], ValueError, "M52 second factor"),
                                ([t(_GIBBS)], NotImplementedError, "Gibbs"),
                                ([t(_SE), prod(_SE, _GIBBS)], NotImplementedError, "Gibbs second factor")):
            for name, call in routes(terms).items():
                assert np.all(np.isfinite(call(ns(1)))), (tag, name)
                with pytest.raises(exc):
                    call(ns(2))
                    pytest.fail("%s: %s accepted a test row of order 2" % (tag, name))
        # training orders up to 7: a test row of order 9 meets 9 + max(9, 7) = 18 > 16, one of order 8 exactly 16
        c.set_data(*_points_1d(7))
        for terms, tag in (([t(_RQ)], "RQ"), ([t(_MAT)], "Matern"), ([t(_SE), prod(_SE, _SE)], "product"),
                           ([prod(_SE, _RQ)], "RQ second factor")):
            for name, call in routes(terms).items():
                assert np.all(np.isfinite(call(ns(8)))), (tag, name)
                with pytest.raises(ValueError):
                    call(ns(9))
                    pytest.fail("%s: %s accepted a test row of order 9" % (tag, name))
        c.fit_terms([t(_SE)], 0.0, y, err, 0.0)
        assert np.all(np.isfinite(c.predict(Xs, ns(9), 0)[0]))            # (a sum of lone SE terms has no such limit)
    finally:
        c.close()


def test_pair_list_and_gram_block_refusals_agree_across_kpairs_and_kbuild():
    from gptools_amd import _lib
    c = _lib.Context(0)
    M = 5
    X, Xo = np.linspace(0.0, 1.0, M)[:, None], np.linspace(0.1, 0.9, M)[:, None]

    def orders(**rows):
        n = np.zeros((M, 1), dtype=int)
        for r, o in rows.items():
            n[int(r[1:])] = o
        return n
    z = orders()

    def calls(k1, k2):
        """name -> callable(ni, nj) for the one-kernel (k2 None) or product entry points; `pairs`: rows matched one to one"""
        if k2 is None:
            return {"kpairs": lambda ni, nj: c.kpairs(k1, _P[k1], X, Xo, ni, nj),
                    "kbuild": lambda ni, nj: c.kbuild(k1, _P[k1], X, ni, Xo, nj),
                    "kbuild sym": lambda ni, nj: c.kbuild(k1, _P[k1], X, ni)}
        return {"kpairs": lambda ni, nj: c.kpairs2(k1, _P[k1], k2, _P[k2], X, Xo, ni, nj),
                "kbuild": lambda ni, nj: c.kbuild2(k1, _P[k1], k2, _P[k2], X, ni, Xo, nj),
                "kbuild sym": lambda ni, nj: c.kbuild2(k1, _P[k1], k2, _P[k2], X, ni)}

    def check(k1, k2, ni, nj, exc, only=None):
        for name, call in calls(k1, k2).items():
            if only and name not in only:
                continue
            if exc is None:
                assert np.all(np.isfinite(call(ni, nj))), (k1, k2, name)
            else:
                with pytest.raises(exc):
                    call(ni, nj)
                    pytest.fail("kernels (%s, %s): %s accepted the orders" % (k1, k2, name))
    try:
        for k1, k2 in ((_M52, None), (_SE, _M52), (_M52, _SE)):                      # M52: a row summing to 2
            check(k1, k2, orders(r1=1), orders(r2=1), None)
            check(k1, k2, orders(r1=2), z, ValueError)
            check(k1, k2, z, orders(r1=2), ValueError, only=("kpairs", "kbuild"))
        for k1, k2 in ((_GIBBS, None), (_SE, _GIBBS), (_GIBBS, _RQ)):                # Gibbs: an order of 2
            check(k1, k2, orders(r1=1), orders(r2=1), None)
            check(k1, k2, orders(r1=2), z, NotImplementedError)
            check(k1, k2, z, orders(r1=2), NotImplementedError, only=("kpairs", "kbuild"))
        for k1, k2 in ((_RQ, None), (_MAT, None), (_SE, _SE), (_SE, _RQ)):           # GPT_RQ_MAXORD = 16
            # a pair list meets row i with row i, a Gram block the worst row with the worst column
            check(k1, k2, orders(r1=9), orders(r1=8), ValueError, only=("kpairs", "kbuild"))          # 17 either way
            check(k1, k2, orders(r1=9), orders(r2=8), None, only=("kpairs",))                          # pairs: 9 and 8
            check(k1, k2, orders(r1=9), orders(r2=8), ValueError, only=("kbuild",))                    # block: 9 + 8
            check(k1, k2, orders(r1=8), orders(r1=8), None, only=("kpairs", "kbuild"))                 # 16
            check(k1, k2, orders(r1=9), z, ValueError, only=("kbuild sym",))                           # 18
            check(k1, k2, orders(r1=8), z, None, only=("kbuild sym",))                                 # 16
        # no points: valid parameters give an empty result, a wrong parameter count is still refused
        e, ez = np.zeros((0, 1)), np.zeros((0, 1), dtype=int)
        good, bad = _P[_RQ], _P[_RQ][:2]
        assert c.kpairs(_RQ, good, e, e, ez, ez).shape == (0,)
        assert c.kpairs2(_SE, _P[_SE], _RQ, good, e, e, ez, ez).shape == (0,)
        assert c.kbuild(_RQ, good, e, ez).shape == (0, 0)
        assert c.kbuild(_RQ, good, e, ez, X, z).shape == (0, M)
        assert c.kbuild(_RQ, good, X, z, e, ez).shape == (M, 0)
        assert c.kbuild2(_SE, _P[_SE], _RQ, good, e, ez).shape == (0, 0)
        assert c.kbuild2(_SE, _P[_SE], _RQ, good, e, ez, X, z).shape == (0, M)
        assert c.kbuild2(_SE, _P[_SE], _RQ, good, X, z, e, ez).shape == (M, 0)
        # ... and the points of an empty block are not looked at: no pair could break an order rule
        assert c.kbuild(_RQ, good, X, orders(r1=9), e, ez).shape == (M, 0)
        assert c.kbuild(_GIBBS, _P[_GIBBS], e, ez, X, orders(r1=2)).shape == (0, M)
        assert c.kbuild2(_SE, _P[_SE], _M52, _P[_M52], X, orders(r1=2), e, ez).shape == (M, 0)
        assert c.kbuild2(_GIBBS, _P[_GIBBS], _RQ, good, e, ez, X, orders(r1=9)).shape == (0, M)
        for call in (lambda: c.kpairs(_RQ, bad, e, e, ez, ez), lambda: c.kpairs2(_SE, _P[_SE], _RQ, bad, e, e, ez, ez),
                     lambda: c.kpairs2(_SE, [1.0], _RQ, good, e, e, ez, ez), lambda: c.kbuild(_RQ, bad, e, ez),
                     lambda: c.kbuild(_RQ, bad, e, ez, X, z), lambda: c.kbuild2(_SE, _P[_SE], _RQ, bad, e, ez),
                     lambda: c.kbuild2(_SE, _P[_SE], _RQ, bad, X, z, e, ez)):
            with pytest.raises(ValueError):
                call()
    finally:
        c.close()
