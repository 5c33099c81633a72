"""GPU suite: the Gibbs kernels with the bucket and exp-Gauss length scales (GibbsKernel1dCubicBucket, GibbsKernel1dQuinticBucket,
GibbsKernel1dExpGauss) on the device -- pair lists and Gram matrices against the reference (tests/golden/g17_gibbs_more.npz),
the fused builder against the pair list, sums / products / T, a fit against the host GibbsKernel1d route, the batched fit and
MCMC routes, exp-Gauss beyond the device cap, the Python-kernel rule and the errors through the C ABI."""
import pickle
import sys
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, assert_close, assert_close_nan

sys.path.insert(0, GOLDEN)
import gen_g17_gibbs_more as G17      # noqa: E402

pytestmark = pytest.mark.gpu

PAIR_CASES = sorted(G17.PAIR_CASES)
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def g():
    import gptools_amd
    return gptools_amd


def _terms(golden):
    G = golden("g17_gibbs_more")
    return G, {k[len("terms__"):]: v for k, v in G.items() if k.startswith("terms__")}


def _host_warp(g, kind):
    return {"cubic": g.cubic_bucket_warp, "quintic": g.quintic_bucket_warp, "expgauss": g.exp_gauss_warp}[kind]


def _host_kernel(g, kind, params, bounds=(-10.0, 10.0)):
    return g.GibbsKernel1d(_host_warp(g, kind), num_params=len(params), initial_params=list(params),
                           param_bounds=[bounds] * len(params))


@pytest.mark.parametrize("case", PAIR_CASES)
def test_device_pairs_match_reference(g, golden, case):
    G = golden("g17_gibbs_more")
    p = {k: G["pairs_%s__%s" % (case, k)] for k in ("xi", "xj", "ni", "nj", "params", "k")}
    k = G17.gibbs(g, G17.PAIR_CASES[case][0], p["params"])
    got = k(p["xi"][:, None], p["xj"][:, None], p["ni"][:, None], p["nj"][:, None])
    for a in (0, 1):
        for b in (0, 1):
            sel = (p["ni"] == a) & (p["nj"] == b)
            assert sel.any()
            fin = np.isfinite(p["k"][sel]) & np.isfinite(got[sel])
            if fin.any():
                print("%s class %d%d: max rel dev %.3g" % (case, a, b, np.max(
                    np.abs(got[sel][fin] - p["k"][sel][fin]) / np.maximum(np.abs(p["k"][sel][fin]), 1e-300))))
            assert_close_nan(got[sel], p["k"][sel], rtol=1e-12, atol_scale=1e-13, msg="%s class %d%d" % (case, a, b))


@pytest.mark.parametrize("case", PAIR_CASES)
def test_builder_matches_pair_list(g, golden, case):
    """The fused builder (length-scale functions hoisted, plain tiles) gives the pair function's numbers, every NaN included:
    800 points = 25 row tiles x 4 column tiles, the last column tile 32 wide; the first half value points, so plain tiles occur."""
    G = golden("g17_gibbs_more")
    p = {k: G["pairs_%s__%s" % (case, k)] for k in ("xi", "xj", "ni", "nj", "params")}
    k = G17.gibbs(g, G17.PAIR_CASES[case][0], p["params"])
    gp = g.GaussianProcess(k)
    X = np.concatenate((p["xi"], p["xj"]))[:, None]
    n = np.concatenate((np.zeros(G17.M_PAIRS, int), p["nj"]))[:, None]
    K = gp.compute_Kij(X, None, n, None)
    M = len(X)
    pairs = k(np.repeat(X, M, axis=0), np.tile(X, (M, 1)), np.repeat(n, M, axis=0), np.tile(n, (M, 1))).reshape(M, M)
    assert_close_nan(K, pairs, rtol=1e-15, atol_scale=0.0, msg=case)
    # a rectangle whose rows and columns end inside a tile (45 rows: 1 + a ragged row tile; 300 columns: 1 + a ragged column tile)
    Kr = gp.compute_Kij(X[380:425], X[200:500], n[380:425], n[200:500])
    assert_close_nan(Kr, pairs[380:425, 200:500], rtol=1e-15, atol_scale=0.0, msg=case + " rect")


@pytest.mark.parametrize("case", G17.KIJ_CASES)
def test_gram_matrices_match_reference(g, golden, case):
    G = golden("g17_gibbs_more")
    kind, params = G17.PAIR_CASES[case]
    gp = g.GaussianProcess(G17.gibbs(g, kind, params))
    X, n, Xj, nj = (G["kij_%s__%s" % (case, s)] for s in ("X", "n", "Xj", "nj"))
    assert_close_nan(gp.compute_Kij(X[:, None], None, n[:, None], None), G["kij_%s__sym" % case], msg="sym")
    assert_close_nan(gp.compute_Kij(X[:30, None], Xj[:, None], n[:30, None], nj[:, None]), G["kij_%s__rect" % case], msg="rect")


@pytest.mark.parametrize("case", G17.TERM_CASES)
def test_sums_products_and_transform(g, golden, case):
    """The tolerances of test_gpu_gibbs.py's terms block."""
    G, td = _terms(golden)
    gp = G17.make_terms_gp(g, case, td)
    gp.compute_K_L_alpha_ll()
    assert gp._fit_mode == "kernel"                            # (T too: the device applies it, gpt_set_T)
    assert abs(gp.ll - float(G["terms_%s__ll" % case])) <= 1e-9 * max(1.0, abs(float(G["terms_%s__ll" % case])))
    assert_close(gp.alpha.ravel(), G["terms_%s__alpha" % case], rtol=1e-8, atol_scale=1e-10)
    for nn in (0, 1):
        m, s = gp.predict(td["Xs"], n=nn)
        mw, sw = G["terms_%s__mean%d" % (case, nn)], G["terms_%s__std%d" % (case, nn)]
        np.testing.assert_allclose(m, mw, rtol=0, atol=1e-8 * max(1.0, np.abs(mw).max()))
        np.testing.assert_allclose(s ** 2, sw ** 2, rtol=0, atol=1e-8 * max(1.0, (sw ** 2).max()))


@pytest.mark.parametrize("kind", G17.KINDS)
def test_product_pairs_match_host_product_rule(g, kind):
    rs = np.random.RandomState(3)
    M = 400
    xi, xj = rs.uniform(0, 2, (M, 1)), rs.uniform(0, 2, (M, 1))
    ni, nj = rs.randint(0, 2, (M, 1)), rs.randint(0, 2, (M, 1))
    p = G17.TERM_PARAMS[kind]
    se = g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 1.5], param_bounds=[(1e-3, 10.0)] * 2)
    native = G17.gibbs(g, kind, p) * se
    host = _host_kernel(g, kind, p) * se
    assert native._native_factors() is not None and host._native_factors() is None
    assert_close_nan(native(xi, xj, ni, nj), host(xi, xj, ni, nj), rtol=1e-12, atol_scale=1e-13)
    # ... and with the Gibbs kernel as the second factor
    native2 = se * G17.gibbs(g, kind, p)
    assert native2._native_factors() is not None
    assert_close_nan(native2(xi, xj, ni, nj), host(xi, xj, ni, nj), rtol=1e-12, atol_scale=1e-13)


def _host_subclass(g, kind):
    """The native class wrapped in a subclass that overrides __call__: a Python kernel (pair list on the host, fit_matrix)."""
    base = {"cubic": g.GibbsKernel1dCubicBucket, "quintic": g.GibbsKernel1dQuinticBucket, "expgauss": g.GibbsKernel1dExpGauss}[kind]
    calls = []

    class Wrapped(base):
        def __call__(self, *a, **kw):
            calls.append(1)
            return g.GibbsKernel1d.__call__(self, *a, **kw)
    return Wrapped, calls


def _scale_model(g, k):
    rs = np.random.RandomState(1000)
    N = 1000
    X = np.sort(rs.uniform(0.0, 2.0, N))
    n = np.zeros(N, dtype=int)
    n[3 * N // 4:] = 1
    y = np.tanh(3.0 * (X - 1.0)) + 0.05 * rs.randn(N)
    gp = g.GaussianProcess(k)
    gp.add_data(X, y, err_y=0.1, n=n)
    return gp


@pytest.mark.parametrize("kind", G17.KINDS)
def test_native_fit_equals_host_route(g, kind):
    """N = 1000, the last quarter slopes: the native fit (fused builder) against the same kernel through the host pair list and
    fit_matrix -- ll and alpha within 1e-9 relative (the bound of test_gpu_gibbs.py's fit at N = 4096: the two matrices agree
    to ~1e-14 of their scale and the noise floor err_y^2 = 1e-2 bounds the condition number by ~1e5 N)."""
    p = G17.TERM_PARAMS[kind]
    b = [(-10.0, 10.0)] * len(p)
    Wrapped, calls = _host_subclass(g, kind)
    kw = dict(initial_params=p, param_bounds=b)
    nat = _scale_model(g, G17.gibbs(g, kind, p))
    host = _scale_model(g, Wrapped(2, **kw) if kind == "expgauss" else Wrapped(**kw))
    nat.compute_K_L_alpha_ll()
    host.compute_K_L_alpha_ll()
    assert nat._fit_mode == "kernel" and host._fit_mode == "matrix" and calls
    print("%s: ll %.17g native, %.17g host" % (kind, nat.ll, host.ll))
    assert abs(nat.ll - host.ll) <= 1e-9 * abs(host.ll), (nat.ll, host.ll)
    a, h = nat.alpha.ravel(), host.alpha.ravel()
    assert np.abs(a - h).max() <= 1e-9 * np.abs(h).max()
    assert (Wrapped(2, **kw) if kind == "expgauss" else Wrapped(**kw))._gpt_kernel_id is not None
    se = g.SquaredExponentialKernel(num_dim=1, param_bounds=[(0, 1)] * 2)
    assert ((Wrapped(2, **kw) if kind == "expgauss" else Wrapped(**kw)) * se)._native_factors() is None


@pytest.mark.parametrize("kind", G17.KINDS)
def test_fit_batch_terms_bit_identical_to_single_fits(g, golden, kind):
    """gpt_fit_batch_terms carries, per element, the very bits one gpt_fit_terms call returns -- the kernel alone and in a product
    plus a second term -- and GaussianProcess.ll_batch takes that route."""
    from gptools_amd import _lib
    kid = G17.gibbs(g, kind, G17.TERM_PARAMS[kind])._gpt_kernel_id
    rs = np.random.RandomState(23)
    N, B = 300, 6
    X = np.sort(rs.uniform(0.0, 2.0, N))[:, None]
    n = np.zeros((N, 1), dtype=int)
    n[-40:] = 1
    y = np.tanh(3.0 * (X[:, 0] - 1.0)) + 1e-2 * rs.randn(N)
    err = np.full(N, 0.05)
    base = np.array(G17.TERM_PARAMS[kind])

    def terms(b, prod):
        q = base.copy()
        q[:2] *= 1.0 + 0.05 * b
        if not prod:
            return [(kid, q)]
        return [(kid, q, _lib.KERNEL_SE, np.array([1.0, 1.5 + 0.1 * b])), (_lib.KERNEL_SE, np.array([0.3, 0.5]))]
    c = _lib.Context(0)
    try:
        c.set_data(X, n)
        nv = 1e-3 * (1.0 + np.arange(B))
        Y = y[None, :] + 1e-3 * rs.randn(B, N)
        for prod in (False, True):
            ll, ld, info = c.fit_batch_terms([terms(b, prod) for b in range(B)], nv, Y, err, 1e2 * EPS)
            assert not info.any()
            for b in range(B):
                l1, d1 = c.fit_terms(terms(b, prod), nv[b], Y[b], err, 1e2 * EPS)
                assert (l1, d1) == (ll[b], ld[b]), (kind, prod, b, l1 - ll[b], d1 - ld[b])
    finally:
        c.close()
    G, td = _terms(golden)
    gp = G17.make_terms_gp(g, kind + "_noise", td)
    theta = np.array(gp.free_params[:], dtype=float)
    pts = [theta * (1.0 + 0.02 * i) for i in range(5)]
    calls = []
    orig = gp._ctx.fit_batch_terms
    gp._ctx.fit_batch_terms = lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vals = gp.ll_batch(pts)
        assert calls, "ll_batch did not take the batched evaluator"
        one = np.array([-gp.update_hyperparameters(q) for q in pts])
    np.testing.assert_array_equal(vals, one)


@pytest.mark.parametrize("kind", G17.KINDS)
def test_compute_from_mcmc_batched_equals_loop(g, golden, kind):
    G, td = _terms(golden)
    gp = G17.make_terms_gp(g, kind + "_noise", td)
    rs = np.random.RandomState(11)
    theta = np.array(gp.free_params[:], dtype=float)
    trace = theta[None, :] * (1.0 + 0.05 * rs.uniform(-1.0, 1.0, (8, len(theta))))
    ns = np.zeros(len(td["Xs"]), dtype=int)
    ns[-10:] = 1
    batched = gp.compute_from_MCMC(td["Xs"], n=ns, flat_trace=trace, return_cov=True)
    gp.batch_grid_max_n = 0                                    # forces the loop route
    loop = gp.compute_from_MCMC(td["Xs"], n=ns, flat_trace=trace, return_cov=True)
    for key in loop:
        a, b = np.asarray(batched[key]), np.asarray(loop[key])
        assert a.shape == b.shape
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-10 * max(1.0, np.abs(b).max()), err_msg=key)


def test_compute_l_from_mcmc(g, golden):
    G, td = _terms(golden)
    gp = G17.make_terms_gp(g, "cubic_alone", td)
    np.testing.assert_allclose(gp.compute_l_from_MCMC(G["lmcmc__X"], n=0, flat_trace=G["lmcmc__trace"]), G["lmcmc__l0"],
                               rtol=1e-14, atol=0)


def test_exp_gauss_over_the_cap_takes_the_host_route(g, golden):
    """One Gaussian more than the device carries: the host route (pair list, fit_matrix), and the numbers of the formula -- the
    ninth Gaussian has weight zero, so the capped-size native kernel with the other eight is the same function."""
    from gptools_amd import _lib
    G, td = _terms(golden)
    p8 = np.asarray(G17.E_G8)
    p9 = np.concatenate((p8[:2], p8[2:10], [0.4], p8[10:18], [0.2], p8[18:26], [0.0]))
    k9 = g.GibbsKernel1dExpGauss(_lib.GIBBS_MAX_GAUSS + 1, initial_params=p9, param_bounds=[(-10.0, 10.0)] * 29)
    k8 = g.GibbsKernel1dExpGauss(_lib.GIBBS_MAX_GAUSS, initial_params=p8, param_bounds=[(-10.0, 10.0)] * 26)
    out = []
    for k in (k9, k8):
        gp = g.GaussianProcess(k)
        gp.add_data(td["X"], td["y"], err_y=0.05, n=td["n"])
        gp.compute_K_L_alpha_ll()
        # (gp.ll carries the hyperprior: uniform over the bounds, three more parameters -> 3 log 20 apart; the data term is compared)
        out.append((gp._fit_mode, gp.ll - gp.hyperprior(gp.params), gp.predict(td["Xs"], n=1)))
    assert out[0][0] == "matrix" and out[1][0] == "kernel"
    assert abs(out[0][1] - out[1][1]) <= 1e-10 * abs(out[1][1])
    for a, b in zip(out[0][2], out[1][2]):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-8 * max(1.0, np.abs(b).max()))
    rs = np.random.RandomState(5)
    xi, xj = rs.uniform(0, 2, (200, 1)), rs.uniform(0, 2, (200, 1))
    ni, nj = rs.randint(0, 2, (200, 1)), rs.randint(0, 2, (200, 1))
    assert_close_nan(k9(xi, xj, ni, nj), k8(xi, xj, ni, nj), rtol=1e-12, atol_scale=1e-13)


def test_pickled_gp_fits_the_same(g, golden):
    G, td = _terms(golden)
    for case in ("cubic_prod_se", "quintic_noise", "expgauss_sum_se"):
        gp = G17.make_terms_gp(g, case, td)
        gp2 = pickle.loads(pickle.dumps(gp))
        gp.compute_K_L_alpha_ll()
        gp2.compute_K_L_alpha_ll()
        assert gp2._fit_mode == "kernel" and gp2.ll == gp.ll


def test_errors_through_the_c_abi(g, golden):
    from gptools_amd import _lib
    x = np.array([[0.5], [1.5]])
    one = np.ones((2, 1), dtype=int)
    ctx = _lib.default_context()
    G, td = _terms(golden)
    for kind in G17.KINDS:
        p = G17.TERM_PARAMS[kind]
        k = G17.gibbs(g, kind, p)
        kid = k._gpt_kernel_id
        with pytest.raises(NotImplementedError, match=r"greater than \[1, 1\]"):
            k(x, x, 2 * one, one)
        with pytest.raises(NotImplementedError, match="Hyperparameter derivatives have not been implemented!"):
            k(x, x, one, one, hyper_deriv=1)
        gp = g.GaussianProcess(k)
        with pytest.raises(NotImplementedError):
            gp.compute_Kij(x, None, np.array([[0], [2]]), None)
        with pytest.raises(NotImplementedError):
            gp.compute_Kij(x, None, one, None, hyper_deriv=0)
        with pytest.raises(ValueError):
            ctx.kpairs(kid, np.array(p[:-1]), x, x, one, one)                          # parameter count
        with pytest.raises(ValueError):
            ctx.kpairs(kid, np.array(list(p) + [0.1]), x, x, one, one)
        x2 = np.ones((2, 2))
        with pytest.raises(ValueError, match="only supports 1d"):
            ctx.kpairs(kid, np.array(p), x2, x2, 0 * x2.astype(int), 0 * x2.astype(int))   # num_dim 2
        # fits and predictions
        n2 = td["n"].copy()
        n2[-1] = 2
        gp = g.GaussianProcess(G17.gibbs(g, kind, p))
        gp.add_data(td["X"], td["y"], err_y=0.05, n=n2)
        with pytest.raises(NotImplementedError):
            gp.compute_K_L_alpha_ll()
        gp = g.GaussianProcess(G17.gibbs(g, kind, p))
        gp.add_data(td["X"], td["y"], err_y=0.05, n=td["n"])
        with pytest.raises(NotImplementedError):
            gp.predict(td["Xs"][:3], n=2)
        c = _lib.Context(0)
        try:
            c.set_data(td["X"][:, None], n2[:, None])
            with pytest.raises(NotImplementedError):
                c.fit_batch(kid, np.array([p, p]), np.zeros(2), np.tile(td["y"], (2, 1)), np.full(len(td["y"]), 0.05), 1e-14)
        finally:
            c.close()
    # exp-Gauss: one Gaussian more than the cap, through every entry point that takes parameters
    G9 = _lib.GIBBS_MAX_GAUSS + 1
    p9 = np.concatenate(([1.0, 0.5], np.linspace(0.1, 1.9, G9), np.full(G9, 0.3), np.full(G9, 0.1)))
    with pytest.raises(ValueError, match="GPT_GIBBS_MAX_GAUSS = %d" % _lib.GIBBS_MAX_GAUSS):
        ctx.kpairs(_lib.KERNEL_GIBBS_EXPGAUSS, p9, x, x, one, one)
    with pytest.raises(ValueError, match="GPT_GIBBS_MAX_GAUSS"):
        ctx.kbuild(_lib.KERNEL_GIBBS_EXPGAUSS, p9, x, one, None, None)
    with pytest.raises(ValueError, match="GPT_GIBBS_MAX_GAUSS"):
        ctx.kpairs2(_lib.KERNEL_SE, np.array([1.0, 1.0]), _lib.KERNEL_GIBBS_EXPGAUSS, p9, x, x, one, one)
    c = _lib.Context(0)
    try:
        c.set_data(td["X"][:, None], td["n"][:, None])
        with pytest.raises(ValueError, match="GPT_GIBBS_MAX_GAUSS"):
            c.fit_terms([(_lib.KERNEL_GIBBS_EXPGAUSS, p9)], 0.0, td["y"], np.full(len(td["y"]), 0.05), 1e-14)
    finally:
        c.close()
    with pytest.raises(ValueError, match="3 G \\+ 2"):
        ctx.kpairs(_lib.KERNEL_GIBBS_EXPGAUSS, np.array([1.0, 0.5]), x, x, one, one)      # no Gaussian at all
    # use_hyper_deriv: the objective's rule (a failure counts as +inf)
    p = G17.TERM_PARAMS["cubic"]
    gp = g.GaussianProcess(G17.gibbs(g, "cubic", p), use_hyper_deriv=True)
    gp.add_data(td["X"], td["y"], err_y=0.05, n=td["n"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(NotImplementedError):
            gp.update_hyperparameters(np.array(p), inf_on_error=False)
        assert gp.update_hyperparameters(np.array(p))[0] == np.inf


def test_partitioned_route_is_not_taken(g, golden):
    G, td = _terms(golden)
    for kind in G17.KINDS:
        gp = G17.make_terms_gp(g, kind + "_noise", td)
        gp.partitioned = True
        assert not gp._partitioned_possible()
