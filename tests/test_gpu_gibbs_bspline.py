"""GPU suite: the Gibbs kernel with a B-spline length scale (GibbsKernel1dBSpline, GPT_KERNEL_GIBBS_BSPLINE) on the device -- pair
lists and Gram matrices against the reference (tests/golden/g18_gibbs_bspline.npz), the fused builder against the pair list, sums /
products / T, a fit against the host GibbsKernel1d(BSplineWarp()) route, the batched fit and MCMC routes, the host route beyond the
device kernel's cap, the refusals through the C ABI; and the I-spline warped kernel (a host kernel around a device one)."""
import sys
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, assert_close, assert_close_nan

sys.path.insert(0, GOLDEN)
import gen_g18_gibbs_bspline as G18      # noqa: E402

pytestmark = pytest.mark.gpu

PAIR_CASES = sorted(G18.PAIR_CASES)
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def g():
    import gptools_amd
    return gptools_amd


def _terms(golden):
    G = golden("g18_gibbs_bspline")
    return G, {k[len("terms__"):]: v for k, v in G.items() if k.startswith("terms__")}


def _host_kernel(g, params, k=3, bounds=(-10.0, 10.0)):
    return g.GibbsKernel1d(g.BSplineWarp(k=k), num_params=len(params), initial_params=list(params),
                           param_bounds=[bounds] * len(params))


@pytest.mark.parametrize("case", PAIR_CASES)
def test_device_pairs_match_reference(g, golden, case):
    G = golden("g18_gibbs_bspline")
    p = {k: G["pairs_%s__%s" % (case, k)] for k in ("xi", "xj", "ni", "nj", "params", "k")}
    k = G18.bspline(g, p["params"])
    assert type(k) is g.GibbsKernel1dBSpline
    got = k(p["xi"][:, None], p["xj"][:, None], p["ni"][:, None], p["nj"][:, None])
    for a in (0, 1):
        for b in (0, 1):
            sel = (p["ni"] == a) & (p["nj"] == b)
            assert sel.any()
            fin = np.isfinite(p["k"][sel]) & np.isfinite(got[sel]) & (p["k"][sel] != 0)
            if fin.any():
                print("%s class %d%d: max rel dev %.3g" % (case, a, b, np.max(
                    np.abs(got[sel][fin] - p["k"][sel][fin]) / np.abs(p["k"][sel][fin]))))
            assert_close_nan(got[sel], p["k"][sel], rtol=1e-12, atol_scale=1e-13, msg="%s class %d%d" % (case, a, b))


@pytest.mark.parametrize("case", PAIR_CASES)
def test_builder_matches_pair_list(g, golden, case):
    """The fused builder (the spline hoisted out of the pair loop, plain tiles) gives the pair function's numbers, every NaN and
    zero of the points outside the knots included: 800 points = 25 row tiles x 4 column tiles, the last column tile 32 wide; the
    first half value points, so plain tiles occur."""
    G = golden("g18_gibbs_bspline")
    p = {k: G["pairs_%s__%s" % (case, k)] for k in ("xi", "xj", "ni", "nj", "params")}
    k = G18.bspline(g, p["params"])
    gp = g.GaussianProcess(k)
    X = np.concatenate((p["xi"][:400], p["xj"][:400]))[:, None]
    n = np.concatenate((np.zeros(400, int), p["nj"][:400]))[:, None]
    K = gp.compute_Kij(X, None, n, None)
    M = len(X)
    pairs = k(np.repeat(X, M, axis=0), np.tile(X, (M, 1)), np.repeat(n, M, axis=0), np.tile(n, (M, 1))).reshape(M, M)
    if case == "out":
        assert np.isnan(pairs).any() and (pairs == 0).any() and np.isfinite(pairs).any()
    assert_close_nan(K, pairs, rtol=1e-15, atol_scale=0.0, msg=case)
    # a rectangle whose rows and columns end inside a tile (45 rows: 1 + a ragged row tile; 300 columns: 1 + a ragged column tile)
    Kr = gp.compute_Kij(X[380:425], X[200:500], n[380:425], n[200:500])
    assert_close_nan(Kr, pairs[380:425, 200:500], rtol=1e-15, atol_scale=0.0, msg=case + " rect")


def test_gram_matrices_match_reference(g, golden):
    G = golden("g18_gibbs_bspline")
    gp = g.GaussianProcess(G18.bspline(g, G18.PAIR_CASES[G18.KIJ_CASE]))
    X, n, Xj, nj = (G["kij__" + s] for s in ("X", "n", "Xj", "nj"))
    for a, b in zip((X, n, Xj, nj), G18.kij_data()):
        np.testing.assert_array_equal(a, b)
    assert_close_nan(gp.compute_Kij(X[:, None], None, n[:, None], None), G["kij__sym"], msg="sym")
    assert_close_nan(gp.compute_Kij(X[:30, None], Xj[:, None], n[:30, None], nj[:, None]), G["kij__rect"], msg="rect")


@pytest.mark.parametrize("case", G18.TERM_CASES)
def test_sums_products_and_transform(g, golden, case):
    """The tolerances of test_gpu_gibbs.py's terms block."""
    G, td = _terms(golden)
    gp = G18.make_terms_gp(g, case, td)
    gp.compute_K_L_alpha_ll()
    assert gp._fit_mode == "kernel"                            # (T too: the device applies it, gpt_set_T)
    want = float(G["terms_%s__ll" % case])
    print("%s: ll %.17g, reference %.17g" % (case, gp.ll, want))
    assert abs(gp.ll - want) <= 1e-9 * max(1.0, abs(want))
    assert_close(gp.alpha.ravel(), G["terms_%s__alpha" % case], rtol=1e-8, atol_scale=1e-10)
    for nn in (0, 1):
        m, s = gp.predict(td["Xs"], n=nn)
        mw, sw = G["terms_%s__mean%d" % (case, nn)], G["terms_%s__std%d" % (case, nn)]
        assert np.isfinite(mw).all() and np.isfinite(sw).all()
        np.testing.assert_allclose(m, mw, rtol=0, atol=1e-8 * max(1.0, np.abs(mw).max()))
        np.testing.assert_allclose(s ** 2, sw ** 2, rtol=0, atol=1e-8 * max(1.0, (sw ** 2).max()))


def test_product_pairs_match_host_product_rule(g):
    """The B-spline kernel as the first and as the second factor; points outside the knots among them (the zero-length-scale
    rule inside a product)."""
    rs = np.random.RandomState(3)
    M = 400
    xi, xj = rs.uniform(-0.4, 2.4, (M, 1)), rs.uniform(-0.4, 2.4, (M, 1))
    ni, nj = rs.randint(0, 2, (M, 1)), rs.randint(0, 2, (M, 1))
    p = G18.TERM_PARAMS
    se = g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 1.5], param_bounds=[(1e-3, 10.0)] * 2)
    native = G18.bspline(g, p) * se
    host = _host_kernel(g, p) * se
    assert native._native_factors() is not None and host._native_factors() is None
    want = host(xi, xj, ni, nj)
    assert np.isnan(want).any() and np.isfinite(want).any()
    assert_close_nan(native(xi, xj, ni, nj), want, rtol=1e-12, atol_scale=1e-13)
    native2 = se * G18.bspline(g, p)
    assert native2._native_factors() is not None
    assert_close_nan(native2(xi, xj, ni, nj), want, rtol=1e-12, atol_scale=1e-13)


def _fit_model(g, k, N=130):
    rs = np.random.RandomState(130)
    X = np.sort(rs.uniform(0.0, 2.0, N))
    n = np.zeros(N, dtype=int)
    n[3 * N // 4:] = 1
    y = np.tanh(3.0 * (X - 1.0)) + 0.05 * rs.randn(N)
    gp = g.GaussianProcess(k)
    gp.add_data(X, y, err_y=0.1, n=n)
    return gp


def test_native_fit_equals_host_route(g):
    """N = 130 (two 128-column leaves), the last quarter slopes: the native fit against the same model through the host pair list
    and fit_matrix -- the two matrices agree to ~1e-14 of their scale and the noise floor err_y^2 = 1e-2 bounds the condition
    number, the bound of test_gpu_gibbs_more.py's fit."""
    p = G18.TERM_PARAMS
    nat = _fit_model(g, G18.bspline(g, p))
    host = _fit_model(g, _host_kernel(g, p))
    nat.compute_K_L_alpha_ll()
    host.compute_K_L_alpha_ll()
    assert nat._fit_mode == "kernel" and host._fit_mode == "matrix"
    print("ll %.17g native, %.17g host" % (nat.ll, host.ll))
    assert abs(nat.ll - host.ll) <= 1e-9 * abs(host.ll), (nat.ll, host.ll)
    a, h = nat.alpha.ravel(), host.alpha.ravel()
    assert np.abs(a - h).max() <= 1e-9 * np.abs(h).max()
    Xs = np.linspace(0.0, 2.0, 40)
    for nn in (0, 1):
        for u, v in zip(nat.predict(Xs, n=nn), host.predict(Xs, n=nn)):
            np.testing.assert_allclose(u, v, rtol=0, atol=1e-8 * max(1.0, np.abs(v).max()))


@pytest.mark.parametrize("nt, deg", [(12, 3), (6, 2)])
def test_beyond_the_device_kernel_takes_the_host_route(g, nt, deg):
    """One knot more than the device carries, and another degree: the host route, with the numbers of GibbsKernel1d(BSplineWarp(k))."""
    rs = np.random.RandomState(nt)
    p = [1.1] + list(np.linspace(-0.1, 2.1, nt)) + list(rs.uniform(0.3, 0.9, nt + deg - 1))
    k = g.GibbsKernel1dBSpline(nt, k=deg, initial_params=p, param_bounds=[(-10.0, 10.0)] * len(p))
    assert type(k) is not g.GibbsKernel1dBSpline and isinstance(k, g.GibbsKernel1dBSpline)
    a, b = _fit_model(g, k), _fit_model(g, _host_kernel(g, p, k=deg))
    a.compute_K_L_alpha_ll()
    b.compute_K_L_alpha_ll()
    assert a._fit_mode == "matrix" and b._fit_mode == "matrix"
    assert a.ll == b.ll
    np.testing.assert_array_equal(a.alpha, b.alpha)
    Xs = np.linspace(0.0, 2.0, 20)
    for u, v in zip(a.predict(Xs, n=1), b.predict(Xs, n=1)):
        np.testing.assert_array_equal(u, v)


def _variants():
    """Three parameter vectors that differ in knots and coefficients, and one with its knots out of order."""
    base = np.array(G18.TERM_PARAMS)
    out = []
    for i in range(3):
        q = base.copy()
        q[2:6] += 0.03 * (i + 1) * np.array([1.0, -1.0, 0.5, -0.5])      # the internal knots
        q[7:] *= 1.0 + 0.05 * (i + 1) * np.cos(np.arange(8) + i)          # the coefficients
        out.append(q)
    bad = base.copy()
    bad[2], bad[3] = base[3], base[2]
    return out, bad


def test_ll_batch_equals_single_evaluations(g, golden):
    G, td = _terms(golden)
    gp = G18.make_terms_gp(g, "alone", td)
    good, bad = _variants()
    calls = []
    orig = gp._ctx.fit_batch_terms
    gp._ctx.fit_batch_terms = lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vals = gp.ll_batch(good)
        assert calls, "ll_batch did not take the batched evaluator"
        one = np.array([-gp.update_hyperparameters(q) for q in good])
        np.testing.assert_array_equal(vals, one)
        assert np.isfinite(vals).all() and len(set(vals)) == 3
        # unsorted knots in one row: the library refuses the chunk (ValueError), the rows are evaluated one by one and only
        # that row is lost (update_hyperparameters gives +inf there, ll_batch its negative)
        mixed = gp.ll_batch(good[:2] + [bad] + good[2:])
        np.testing.assert_array_equal(mixed[[0, 1, 3]], one)
        assert mixed[2] == -np.inf
        assert gp.update_hyperparameters(bad) == np.inf
        with pytest.raises(ValueError, match="Knots must be in increasing order!"):
            gp.update_hyperparameters(bad, inf_on_error=False)


def test_compute_from_mcmc_batched_equals_loop(g, golden):
    G, td = _terms(golden)
    gp = G18.make_terms_gp(g, "alone", td)
    good, _ = _variants()
    trace = np.array(good + [np.array(G18.TERM_PARAMS)])
    assert trace.shape == (4, 15) and len(gp.free_params[:]) == 15
    ns = np.zeros(len(td["Xs"]), dtype=int)
    ns[-10:] = 1
    calls = []
    orig = gp._ctx.fit_batch_terms
    gp._ctx.fit_batch_terms = lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1]
    gp.mcmc_batch_min_rows = 2
    batched = gp.compute_from_MCMC(td["Xs"], n=ns, flat_trace=trace, return_cov=True)
    assert calls, "compute_from_MCMC did not take the batched route"
    del calls[:]
    gp.mcmc_batch_min_rows = 10 ** 9                           # forces the loop route
    loop = gp.compute_from_MCMC(td["Xs"], n=ns, flat_trace=trace, return_cov=True)
    assert not calls
    for key in loop:
        a, b = np.asarray(batched[key]), np.asarray(loop[key])
        assert a.shape == b.shape
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-10 * max(1.0, np.abs(b).max()), err_msg=key)


def test_refusals_through_the_c_abi(g, golden):
    """Every refusal leaves the context usable: a good call follows each."""
    from gptools_amd import _lib
    kid = _lib.KERNEL_GIBBS_BSPLINE
    x = np.array([[0.5], [1.5]])
    one = np.ones((2, 1), dtype=int)
    zero = np.zeros((2, 1), dtype=int)
    ctx = _lib.default_context()
    p = np.array(G18.PAIR_CASES["nt6"])
    want = ctx.kpairs(kid, p, x, x[::-1], one, zero)
    assert np.isfinite(want).all()

    def still_usable():
        np.testing.assert_array_equal(ctx.kpairs(kid, p, x, x[::-1], one, zero), want)
    with pytest.raises(ValueError, match="GPT_GIBBS_MAX_KNOTS = 11"):
        ctx.kpairs(kid, p[:-1], x, x, one, one)                                        # an even parameter count
    still_usable()
    with pytest.raises(ValueError, match="GPT_GIBBS_MAX_KNOTS"):
        ctx.kpairs(kid, np.array([1.0, 0.0, 0.5, 0.5, 0.5]), x, x, one, one)           # nt = 1
    still_usable()
    nt12 = _lib.GIBBS_MAX_KNOTS + 1
    p12 = np.concatenate(([1.0], np.linspace(0.0, 2.0, nt12), np.full(nt12 + 2, 0.5)))
    for call in (lambda: ctx.kpairs(kid, p12, x, x, one, one), lambda: ctx.kbuild(kid, p12, x, one, None, None),
                 lambda: ctx.kpairs2(_lib.KERNEL_SE, np.array([1.0, 1.0]), kid, p12, x, x, one, one)):
        with pytest.raises(ValueError, match="GPT_GIBBS_MAX_KNOTS = 11"):
            call()
        still_usable()
    x2 = np.ones((2, 2))
    with pytest.raises(ValueError, match="only supports 1d"):
        ctx.kpairs(kid, p, x2, x2, 0 * x2.astype(int), 0 * x2.astype(int))              # num_dim 2
    still_usable()
    bad = p.copy()
    bad[2], bad[3] = p[3], p[2]
    nan = p.copy()
    nan[3] = np.nan
    for q in (bad, nan):
        for call in (lambda: ctx.kpairs(kid, q, x, x, one, one), lambda: ctx.kbuild(kid, q, x, one, None, None),
                     lambda: ctx.kpairs2(kid, q, _lib.KERNEL_SE, np.array([1.0, 1.0]), x, x, one, one)):
            with pytest.raises(ValueError, match="Knots must be in increasing order!"):
                call()
            still_usable()
    k = G18.bspline(g, p)
    with pytest.raises(NotImplementedError, match=r"Derivatives greater than \[1, 1\] are not supported!"):
        k(x, x, 2 * one, one)
    still_usable()
    with pytest.raises(NotImplementedError, match="Hyperparameter derivatives have not been implemented!"):
        k(x, x, one, one, hyper_deriv=1)
    still_usable()
    gp = g.GaussianProcess(k)
    with pytest.raises(NotImplementedError):
        gp.compute_Kij(x, None, np.array([[0], [2]]), None)
    with pytest.raises(NotImplementedError):
        gp.compute_Kij(x, None, one, None, hyper_deriv=0)
    # fits and predictions
    G, td = _terms(golden)
    n2 = td["n"].copy()
    n2[-1] = 2
    gp = g.GaussianProcess(G18.bspline(g, G18.TERM_PARAMS))
    gp.add_data(td["X"], td["y"], err_y=0.05, n=n2)
    with pytest.raises(NotImplementedError):
        gp.compute_K_L_alpha_ll()
    gp = G18.make_terms_gp(g, "alone", td)
    with pytest.raises(NotImplementedError):
        gp.predict(td["Xs"][:3], n=2)
    gp.compute_K_L_alpha_ll()
    assert np.isfinite(gp.ll)
    c = _lib.Context(0)
    try:
        c.set_data(td["X"][:, None], td["n"][:, None])
        err = np.full(len(td["y"]), 0.05)
        tp = np.array(G18.TERM_PARAMS)
        tbad = tp.copy()
        tbad[2], tbad[3] = tp[3], tp[2]
        with pytest.raises(ValueError, match="Knots must be in increasing order!"):
            c.fit_terms([(kid, tbad)], 0.0, td["y"], err, 1e-14)
        with pytest.raises(ValueError, match="Knots must be in increasing order!"):
            c.fit_batch_terms([[(kid, tp)], [(kid, tbad)]], np.zeros(2), np.tile(td["y"], (2, 1)), err, 1e-14)
        with pytest.raises(ValueError, match="GPT_GIBBS_MAX_KNOTS"):
            c.fit_terms([(kid, p12)], 0.0, td["y"], err, 1e-14)
        ll, ld = c.fit_terms([(kid, tp)], 0.0, td["y"], err, 1e-14)
        assert np.isfinite(ll) and np.isfinite(ld)
    finally:
        c.close()
    still_usable()


def test_partitioned_route_is_not_taken(g, golden):
    G, td = _terms(golden)
    gp = G18.make_terms_gp(g, "alone", td)
    gp.partitioned = True
    assert not gp._partitioned_possible()


def test_isplinewarped_kernel_matches_reference(g, golden):
    """A host warp around a device kernel: the pair list against the reference, and a fit through the Python-kernel route."""
    G = golden("g18_gibbs_bspline")
    k = G18.isw_kernel(g)
    Xi, Xj, ni, nj = (G["isw__" + s] for s in ("Xi", "Xj", "ni", "nj"))
    assert_close_nan(k(Xi, Xj, ni, nj), G["isw__k"], rtol=1e-12, atol_scale=1e-13)
    rs = np.random.RandomState(2)
    X = rs.uniform(0.05, 0.95, (60, 2))
    y = np.sin(3.0 * X[:, 0]) * X[:, 1] + 0.05 * rs.randn(60)
    gp = g.GaussianProcess(k)
    gp.add_data(X, y, err_y=0.05)
    gp.compute_K_L_alpha_ll()
    assert gp._fit_mode == "matrix" and np.isfinite(gp.ll)
    m, s = gp.predict(X[:5])
    assert np.isfinite(m).all() and np.isfinite(s).all()
