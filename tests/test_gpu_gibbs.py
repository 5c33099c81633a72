"""GPU suite: the Gibbs kernels with tanh warps (GibbsKernel1dTanh, GibbsKernel1dDoubleTanh) on the device -- pair lists and
Gram matrices against the reference (tests/golden/g15_gibbs.npz), the demo's Gibbs section, compute_ll_matrix and the MAP,
sums / products / T, a large fit against the host GibbsKernel1d route, the batched fit and MCMC routes, the Python-kernel
rule and the errors through the C ABI."""
import sys
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, assert_close, assert_close_nan

sys.path.insert(0, GOLDEN)
import gen_g15_gibbs as G15      # noqa: E402

pytestmark = pytest.mark.gpu

PAIR_CASES = sorted(G15.PAIR_CASES)


@pytest.fixture(scope="module")
def g():
    import gptools_amd
    return gptools_amd


def _demo(golden):
    G = golden("g15_gibbs")
    return G, {k[len("demo__"):]: v for k, v in G.items() if k.startswith("demo__")}


def _terms(golden):
    G = golden("g15_gibbs")
    return G, {k[len("terms__"):]: v for k, v in G.items() if k.startswith("terms__")}


@pytest.mark.parametrize("case", PAIR_CASES)
def test_device_pairs_match_reference(g, golden, case):
    G = golden("g15_gibbs")
    p = {k: G["pairs_%s__%s" % (case, k)] for k in ("xi", "xj", "ni", "nj", "params", "k")}
    warp, _ = G15.PAIR_CASES[case]
    k = G15.gibbs(g, warp, p["params"])
    got = k(p["xi"][:, None], p["xj"][:, None], p["ni"][:, None], p["nj"][:, None])
    for a in (0, 1):
        for b in (0, 1):
            sel = (p["ni"] == a) & (p["nj"] == b)
            assert_close_nan(got[sel], p["k"][sel], rtol=1e-12, atol_scale=1e-13, msg="%s class %d%d" % (case, a, b))


@pytest.mark.parametrize("case", PAIR_CASES)
def test_builder_matches_pair_list(g, golden, case):
    """The fused builder (warps hoisted, plain tiles) gives the pair function's numbers, every NaN included."""
    G = golden("g15_gibbs")
    p = {k: G["pairs_%s__%s" % (case, k)] for k in ("xi", "xj", "ni", "nj", "params")}
    warp, _ = G15.PAIR_CASES[case]
    k = G15.gibbs(g, warp, p["params"])
    gp = g.GaussianProcess(k)
    X = np.concatenate((p["xi"], p["xj"]))[:, None]
    n = np.concatenate((np.zeros(240, int), p["nj"]))[:, None]        # first half value rows: plain tiles exist
    K = gp.compute_Kij(X, None, n, None)
    M = len(X)
    pairs = k(np.repeat(X, M, axis=0), np.tile(X, (M, 1)), np.repeat(n, M, axis=0), np.tile(n, (M, 1))).reshape(M, M)
    assert_close_nan(K, pairs, rtol=1e-15, atol_scale=0.0, msg=case)


@pytest.mark.parametrize("case", ["t_base", "d_base", "t_neg"])
def test_gram_matrices_match_reference(g, golden, case):
    G = golden("g15_gibbs")
    warp, params = G15.PAIR_CASES[case]
    gp = g.GaussianProcess(G15.gibbs(g, warp, params))
    X, n, Xj, nj = (G["kij_%s__%s" % (case, s)] for s in ("X", "n", "Xj", "nj"))
    assert_close_nan(gp.compute_Kij(X[:, None], None, n[:, None], None), G["kij_%s__sym" % case], msg="sym")
    assert_close_nan(gp.compute_Kij(X[:30, None], Xj[:, None], n[:30, None], nj[:, None]), G["kij_%s__rect" % case], msg="rect")


def test_demo_fit_predict_sample(g, golden):
    """demo/demo.py:381-406 at fixed parameters: ll, alpha, L, predictions of the profile and its gradient, covariances and
    samples (the g6 demo test's tolerances)."""
    G, d = _demo(golden)
    gp = G15.make_demo_gp(g, d)
    negll = gp.update_hyperparameters(d["params"])
    assert gp._fit_mode == "kernel"
    assert abs(negll - float(d["negll"])) < 1e-8
    assert abs(gp.ll - float(d["ll"])) < 1e-8
    assert_close(gp.alpha.ravel(), d["alpha"], rtol=1e-8, atol_scale=1e-10)
    assert_close(gp.L, d["L"], rtol=1e-9, atol_scale=1e-12)
    m0, s0 = gp.predict(d["Xs"])
    np.testing.assert_allclose(m0, d["mean0"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(s0 ** 2, d["std0"] ** 2, rtol=0, atol=1e-8)
    m1, s1 = gp.predict(d["Xs"], n=1)
    np.testing.assert_allclose(m1, d["mean1"], rtol=0, atol=1e-7 * np.abs(d["mean1"]).max())
    np.testing.assert_allclose(s1 ** 2, d["std1"] ** 2, rtol=0, atol=1e-7 * (d["std1"] ** 2).max())
    for nn in (0, 1):
        m, c = gp.predict(d["Xc"], n=nn, return_std=False, return_cov=True)
        sc = np.abs(d["cov%d" % nn]).max()
        np.testing.assert_allclose(m, d["cmean%d" % nn], rtol=0, atol=1e-7 * max(1.0, np.abs(d["cmean%d" % nn]).max()))
        np.testing.assert_allclose(c, d["cov%d" % nn], rtol=0, atol=1e-7 * sc)
    s = gp.draw_sample(d["Xd"], rand_vars=d["u"])
    np.testing.assert_allclose(s, d["samp0"], rtol=0, atol=1e-6 * np.abs(d["samp0"]).max())
    s = gp.draw_sample(d["Xd"], n=1, rand_vars=d["u"])
    np.testing.assert_allclose(s, d["samp1"], rtol=0, atol=1e-6 * np.abs(d["samp1"]).max())


def test_demo_map_and_ll_matrix(g, golden):
    G, d = _demo(golden)
    gp = G15.make_demo_gp(g, d)
    gp.update_hyperparameters(np.array([1.0, 1.0, 0.5, 0.05, 1.0]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res, nres = gp.optimize_hyperparameters(method="SLSQP", random_starts=0, num_proc=0)
    assert nres == 1
    assert abs(res.fun - float(d["map_fun"])) < 2e-6
    np.testing.assert_allclose(res.x, d["map_x"], rtol=2e-3)
    gp = G15.make_demo_gp(g, d, fixed=[True, False, False, True, True])
    ll, pv = gp.compute_ll_matrix([(0.8, 1.6), (0.3, 0.8)], [4, 3])
    np.testing.assert_array_equal(pv[0], d["grid_p0"])
    np.testing.assert_array_equal(pv[1], d["grid_p1"])
    assert_close(ll, d["grid_ll"], rtol=1e-9, atol_scale=0.0)


def test_demo_random_starts(g, golden):
    """g12's scheme: the hyperprior's draws under np.random.seed(4242), one SLSQP run per start, the best kept."""
    G, d = _demo(golden)
    gp = G15.make_demo_gp(g, d)
    gp.update_hyperparameters(np.array([1.0, 1.0, 0.5, 0.05, 1.0]))
    np.random.seed(4242)
    draws = np.asarray(gp.hyperprior.random_draw(size=3).T, dtype=float)
    np.testing.assert_array_equal(draws, d["rs_draws"])
    np.random.seed(4242)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res, count = gp.optimize_hyperparameters(method="SLSQP", random_starts=3, num_proc=0)
    assert count == int(d["rs_count"])
    assert abs(res.fun - float(d["rs_fun"])) <= 2e-6
    np.testing.assert_allclose(res.x, d["rs_x"], rtol=2e-3)


@pytest.mark.parametrize("case", G15.TERM_CASES)
def test_sums_products_and_transform(g, golden, case):
    G, td = _terms(golden)
    gp = G15.make_terms_gp(g, case, td)
    gp.compute_K_L_alpha_ll()
    assert gp._fit_mode == "kernel"                            # (T too: the device applies it, gpt_set_T)
    assert abs(gp.ll - float(G["terms_%s__ll" % case])) <= 1e-9 * max(1.0, abs(float(G["terms_%s__ll" % case])))
    assert_close(gp.alpha.ravel(), G["terms_%s__alpha" % case], rtol=1e-8, atol_scale=1e-10)
    for nn in (0, 1):
        m, s = gp.predict(td["Xs"], n=nn)
        mw, sw = G["terms_%s__mean%d" % (case, nn)], G["terms_%s__std%d" % (case, nn)]
        np.testing.assert_allclose(m, mw, rtol=0, atol=1e-8 * max(1.0, np.abs(mw).max()))
        np.testing.assert_allclose(s ** 2, sw ** 2, rtol=0, atol=1e-8 * max(1.0, (sw ** 2).max()))


def test_product_pairs_match_host_product_rule(g):
    rs = np.random.RandomState(3)
    M = 400
    xi, xj = rs.uniform(0, 2, (M, 1)), rs.uniform(0, 2, (M, 1))
    ni, nj = rs.randint(0, 2, (M, 1)), rs.randint(0, 2, (M, 1))
    p = [1.1, 0.8, 0.3, 0.2, 1.0]
    se = g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 1.5], param_bounds=[(1e-3, 10.0)] * 2)
    native = g.GibbsKernel1dTanh(initial_params=p, param_bounds=[(1e-3, 10.0)] * 5) * se
    host = g.GibbsKernel1d(g.tanh_warp, initial_params=p, param_bounds=[(1e-3, 10.0)] * 5) * se
    assert native._native_factors() is not None and host._native_factors() is None
    assert_close_nan(native(xi, xj, ni, nj), host(xi, xj, ni, nj), rtol=1e-12, atol_scale=1e-13)


def _scale_model(g, cls_args):
    rs = np.random.RandomState(4096)
    N = 4096
    X = np.sort(rs.uniform(0.0, 2.0, N))
    n = np.zeros(N, dtype=int)
    n[3 * N // 4:] = 1
    y = np.tanh(3.0 * (X - 1.0)) + 0.05 * rs.randn(N)
    gp = g.GaussianProcess(cls_args)
    gp.add_data(X, y, err_y=0.1, n=n)
    return gp


def test_at_scale_native_fit_equals_host_route(g):
    """N = 4096, the last quarter slopes: the native fit (fused builder) against the same model through the host
    GibbsKernel1d(tanh_warp) pair list and fit_matrix -- ll and alpha within 1e-9 relative."""
    p = [1.1, 0.8, 0.3, 0.2, 1.0]
    b = [(1e-3, 10.0)] * 5
    nat = _scale_model(g, g.GibbsKernel1dTanh(initial_params=p, param_bounds=b))
    host = _scale_model(g, g.GibbsKernel1d(g.tanh_warp, initial_params=p, param_bounds=b))
    nat.compute_K_L_alpha_ll()
    host.compute_K_L_alpha_ll()
    assert nat._fit_mode == "kernel" and host._fit_mode == "matrix"
    assert abs(nat.ll - host.ll) <= 1e-9 * abs(host.ll), (nat.ll, host.ll)
    a, h = nat.alpha.ravel(), host.alpha.ravel()
    assert np.abs(a - h).max() <= 1e-9 * np.abs(h).max()


@pytest.mark.parametrize("warp", ["tanh", "dtanh"])
def test_batched_fit_equals_single_fits(g, golden, warp):
    G, td = _terms(golden)
    case = "dtanh" if warp == "dtanh" else "noise"
    gp = G15.make_terms_gp(g, case, td)
    rs = np.random.RandomState(7)
    base = np.array(gp.free_params[:], dtype=float)
    pts = [base * (1.0 + 0.1 * rs.randn(len(base))) for _ in range(6)]
    pts = [np.clip(q, 1e-2, None) for q in pts]
    batch = gp.ll_batch(pts)
    single = [-gp.update_hyperparameters(q) for q in pts]
    np.testing.assert_allclose(batch, single, rtol=1e-12)


def test_compute_from_mcmc_batched_equals_loop(g, golden):
    G, td = _terms(golden)
    gp = G15.make_terms_gp(g, "noise", td)
    rs = np.random.RandomState(11)
    trace = np.column_stack([rs.uniform(0.9, 1.3, 8), rs.uniform(0.6, 1.0, 8), rs.uniform(0.2, 0.4, 8),
                             rs.uniform(0.1, 0.3, 8), rs.uniform(0.9, 1.1, 8), rs.uniform(0.05, 0.15, 8)])
    ns = np.zeros(len(td["Xs"]), dtype=int)
    ns[-10:] = 1
    batched = gp.compute_from_MCMC(td["Xs"], n=ns, flat_trace=trace, return_cov=True)
    gp.batch_grid_max_n = 0                                    # forces the loop route
    loop = gp.compute_from_MCMC(td["Xs"], n=ns, flat_trace=trace, return_cov=True)
    for key in loop:
        a, b = np.asarray(batched[key]), np.asarray(loop[key])
        assert a.shape == b.shape
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-10 * max(1.0, np.abs(b).max()), err_msg=key)


def test_python_subclass_takes_the_host_route(g, golden):
    calls = []

    class MyGibbs(g.GibbsKernel1dTanh):
        def __call__(self, *a, **kw):
            calls.append(1)
            return g.GibbsKernel1d.__call__(self, *a, **kw)

    G, td = _terms(golden)
    p = [1.1, 0.8, 0.3, 0.2, 1.0]
    b = [(1e-3, 10.0)] * 5
    out = []
    for k in (MyGibbs(initial_params=p, param_bounds=b), g.GibbsKernel1dTanh(initial_params=p, param_bounds=b)):
        gp = g.GaussianProcess(k)
        gp.add_data(td["X"], td["y"], err_y=0.05, n=td["n"])
        gp.compute_K_L_alpha_ll()
        out.append((gp._fit_mode, gp.ll))
    assert calls and out[0][0] == "matrix" and out[1][0] == "kernel"
    assert abs(out[0][1] - out[1][1]) <= 1e-10 * abs(out[1][1])
    assert (MyGibbs(initial_params=p, param_bounds=b) * g.SquaredExponentialKernel(num_dim=1, param_bounds=[(0, 1)] * 2)
            )._native_factors() is None


def test_errors_through_the_c_abi(g, golden):
    from gptools_amd import _lib
    p = [1.1, 0.8, 0.3, 0.2, 1.0]
    b = [(1e-3, 10.0)] * 5
    k = g.GibbsKernel1dTanh(initial_params=p, param_bounds=b)
    x = np.array([[0.5], [1.5]])
    one = np.ones((2, 1), dtype=int)
    with pytest.raises(NotImplementedError, match=r"greater than \[1, 1\]"):
        k(x, x, 2 * one, one)
    with pytest.raises(NotImplementedError):
        k(x, x, one, one, hyper_deriv=1)
    gp = g.GaussianProcess(k)
    with pytest.raises(NotImplementedError):
        gp.compute_Kij(x, None, np.array([[0], [2]]), None)
    with pytest.raises(NotImplementedError):
        gp.compute_Kij(x, None, one, None, hyper_deriv=0)
    ctx = _lib.default_context()
    with pytest.raises(ValueError):
        ctx.kpairs(_lib.KERNEL_GIBBS_TANH, np.array(p[:4]), x, x, one, one)       # parameter count
    with pytest.raises(ValueError):
        ctx.kpairs(_lib.KERNEL_GIBBS_DTANH, np.array(p), x, x, one, one)
    x2 = np.ones((2, 2))
    with pytest.raises(ValueError):
        ctx.kpairs(_lib.KERNEL_GIBBS_TANH, np.array(p), x2, x2, 0 * x2.astype(int), 0 * x2.astype(int))   # num_dim 2
    # fits and predictions
    G, td = _terms(golden)
    gp = g.GaussianProcess(g.GibbsKernel1dTanh(initial_params=p, param_bounds=b))
    n2 = td["n"].copy()
    n2[-1] = 2
    gp.add_data(td["X"], td["y"], err_y=0.05, n=n2)
    with pytest.raises(NotImplementedError):
        gp.compute_K_L_alpha_ll()
    gp = g.GaussianProcess(g.GibbsKernel1dTanh(initial_params=p, param_bounds=b))
    gp.add_data(td["X"], td["y"], err_y=0.05, n=td["n"])
    with pytest.raises(NotImplementedError):
        gp.predict(td["Xs"][:3], n=2)
    with pytest.raises(NotImplementedError):
        _batch_with_orders(td, p, n2)
    gp = g.GaussianProcess(g.GibbsKernel1dTanh(initial_params=p, param_bounds=b), use_hyper_deriv=True)
    gp.add_data(td["X"], td["y"], err_y=0.05, n=td["n"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(NotImplementedError):
            gp.update_hyperparameters(np.array(p), inf_on_error=False)
        assert gp.update_hyperparameters(np.array(p))[0] == np.inf         # (the objective's rule: a failure counts as +inf)


def _batch_with_orders(td, p, n2):
    from gptools_amd import _lib
    c = _lib.Context(0)
    try:
        c.set_data(td["X"][:, None], n2[:, None])
        P = np.array([p, p])
        c.fit_batch(_lib.KERNEL_GIBBS_TANH, P, np.zeros(2), np.tile(td["y"], (2, 1)), np.full(len(td["y"]), 0.05), 1e-14)
    finally:
        c.close()


def test_partitioned_route_is_not_taken(g, golden):
    G, td = _terms(golden)
    gp = G15.make_terms_gp(g, "noise", td)
    gp.partitioned = True
    assert not gp._partitioned_possible()
