"""GPU suite: GibbsKernel1dGP (GPT_KERNEL_GIBBS_GP, the Gibbs kernel whose length scale is the mean of a nested Gaussian process) on
the device -- pair lists against the reference (tests/golden/g20_gibbs_gp.npz) and against the host twin
``GibbsKernel1d(GPWarp(m, k=nk), num_params=2m+2)``, the fused builder against the pair list, fit + predict, sums and products, the
kernel on one coordinate of a 2-D model, the batched fit and MCMC routes, a linear warp layer, debug_poison and the refusals of the
C ABI.  The tolerances are those of tests/test_gpu_gibbs_more.py for the kernel ids 9-11, quantity for quantity.

Largest deviations the GPU run printed (MI355X):
  * device pairs against the reference, as a fraction of the class's largest value: at most 2.5e-15 (m2), 1.7e-15 (m5), 1.7e-15 (m12),
    7.6e-15 (m5wide); relative to each non-zero value inside the hull at most 9.7e-13 (m2, class 11), 2.6e-13 (m5, classes 01 and
    11), 7.5e-13 (m12, class 10) and 2.7e-12 (m5wide, class 11: entries that are small against the class's scale, so the absolute
    part of the bound, 1e-13 of that scale, covers them);
  * builder against pair list: within 1e-15 relative, NaN for NaN;
  * fit at N = 60: ll -584.44826487429 against the reference's -584.44826487413 (2.7e-13 relative) and the host twin's
    -584.44826487411; predictive mean within 1.9e-12, covariance within 1.1e-14 of the reference's;
  * 2-D masked product: pairs within 1.2e-15 of the scale, ll -414.491359579527 against -414.491359579528;
  * sum / product with SE against the host twin: ll 3e-13 / 2.4e-13 relative; under the linear warp 1.2e-13.
No bound taken from tests/test_gpu_gibbs_more.py had to be changed.
"""
import sys
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, assert_close, assert_close_nan

sys.path.insert(0, GOLDEN)
import gen_g20_gibbs_gp as G20        # noqa: E402

pytestmark = pytest.mark.gpu

CASES = sorted(G20.CASES)
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def g():
    import gptools_amd
    return gptools_amd


def _pairs(golden, case):
    G = golden("g20_gibbs_gp")
    return {k: G["pairs_%s__%s" % (case, k)] for k in ("xi", "xj", "ni", "nj", "params", "sigma_n", "k")}


def _block(golden, prefix):
    G = golden("g20_gibbs_gp")
    return {k[len(prefix) + 2:]: v for k, v in G.items() if k.startswith(prefix + "__")}


def _host_twin(g, case, params=None):
    """The same kernel on the host route: GibbsKernel1d around the numpy GPWarp (pair list on the host, fit_matrix)."""
    x, l, y, sn = G20.CASES[case]
    p = list(G20.case_params(case) if params is None else params)
    return g.GibbsKernel1d(g.GPWarp(len(x), k=G20.nested_se(g, sn, l)), num_params=len(p), initial_params=p,
                           param_bounds=[(-10.0, 10.0)] * len(p))


def _assert_pairs(got, want, ins, rtol=1e-12, atol_scale=1e-13, msg=""):
    """Rows inside the hull of the points: rtol plus atol_scale of the largest value; rows outside: the absolute part alone (the
    fixture's generator says why); NaN for NaN everywhere."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=msg + " (NaN pattern)")
    fin = np.isfinite(want)
    scale = np.abs(want[fin]).max()
    nz = fin & ins & (want != 0.0)
    print("%s: max rel dev inside %.3g, max abs dev / scale %.3g" % (
        msg, (np.abs(got[nz] - want[nz]) / np.abs(want[nz])).max() if nz.any() else 0.0, np.abs(got[fin] - want[fin]).max() / scale))
    np.testing.assert_allclose(got[fin & ins], want[fin & ins], rtol=rtol, atol=atol_scale * scale, err_msg=msg)
    np.testing.assert_allclose(got[fin & ~ins], want[fin & ~ins], rtol=0, atol=atol_scale * scale, err_msg=msg + " (outside)")


@pytest.mark.parametrize("case", CASES)
def test_device_pairs_match_reference_and_host_twin(g, golden, case):
    p = _pairs(golden, case)
    k = G20.gp_kernel(g, case)
    assert type(k) is g.GibbsKernel1dGP
    args = (p["xi"][:, None], p["xj"][:, None], p["ni"][:, None], p["nj"][:, None])
    got = k(*args)
    twin = _host_twin(g, case)(*args)
    ins = G20.inside(p["xi"]) & G20.inside(p["xj"])
    for a in (0, 1):
        for b in (0, 1):
            sel = (p["ni"] == a) & (p["nj"] == b)
            assert sel.any()
            _assert_pairs(got[sel], p["k"][sel], ins[sel], msg="%s class %d%d vs reference" % (case, a, b))
            assert_close_nan(got[sel], twin[sel], rtol=1e-12, atol_scale=1e-13, msg="%s class %d%d vs host twin" % (case, a, b))


@pytest.mark.parametrize("case", CASES)
def test_builder_matches_pair_list(g, case):
    """The fused builder (the length scale hoisted out of the pair loop, plain tiles) gives the pair function's numbers, every NaN
    included: 500 sorted points = 16 row tiles x 2 column tiles, both ragged, the last quarter with order 1 (so plain tiles occur)."""
    rs = np.random.RandomState(40 + CASES.index(case))
    N = 500
    X = np.sort(rs.uniform(0.0, 2.0, N))[:, None]
    n = np.zeros((N, 1), dtype=int)
    n[3 * N // 4:] = 1
    k = G20.gp_kernel(g, case)
    gp = g.GaussianProcess(k)
    K = gp.compute_Kij(X, None, n, None)
    pairs = k(np.repeat(X, N, axis=0), np.tile(X, (N, 1)), np.repeat(n, N, axis=0), np.tile(n, (N, 1))).reshape(N, N)
    assert_close_nan(K, pairs, rtol=1e-15, atol_scale=0.0, msg=case)
    # a rectangle whose corners are no multiples of 64 (45 rows: 1 + a ragged row tile; 300 columns: 1 + a ragged column tile)
    Kr = gp.compute_Kij(X[380:425], X[200:500], n[380:425], n[200:500])
    assert_close_nan(Kr, pairs[380:425, 200:500], rtol=1e-15, atol_scale=0.0, msg=case + " rect")


def test_fit_and_predict_match_reference_and_host_twin(g, golden):
    d = _block(golden, "fit")
    gp = G20.make_fit_gp(g, d)
    gp.compute_K_L_alpha_ll()
    assert gp._fit_mode == "kernel"
    print("ll %.17g, reference %.17g" % (gp.ll, float(d["ll"])))
    assert abs(gp.ll - float(d["ll"])) <= 1e-9 * max(1.0, abs(float(d["ll"])))
    assert_close(gp.K, d["K"], rtol=1e-12, atol_scale=1e-13, msg="K")
    assert_close(gp.alpha.ravel(), d["alpha"], rtol=1e-8, atol_scale=1e-10, msg="alpha")
    mean, cov = gp.predict(d["Xs"], n=d["ns"], return_std=False, return_cov=True)
    std = gp.predict(d["Xs"], n=d["ns"])[1]
    print("mean dev %.3g, cov dev %.3g" % (np.abs(mean - d["mean"]).max(), np.abs(cov - d["cov"]).max()))
    np.testing.assert_allclose(mean, d["mean"], rtol=0, atol=1e-8 * max(1.0, np.abs(d["mean"]).max()))
    np.testing.assert_allclose(cov, d["cov"], rtol=0, atol=1e-8 * max(1.0, np.abs(d["cov"]).max()))
    np.testing.assert_allclose(std ** 2, d["std"] ** 2, rtol=0, atol=1e-8 * max(1.0, (d["std"] ** 2).max()))
    gh = g.GaussianProcess(_host_twin(g, G20.FIT_CASE))
    gh.add_data(d["X"], d["y"], err_y=G20.ERR_Y, n=d["n"])
    gh.compute_K_L_alpha_ll()
    assert gh._fit_mode == "matrix"
    print("ll %.17g native, %.17g host" % (gp.ll, gh.ll))
    assert abs(gp.ll - gh.ll) <= 1e-9 * abs(gh.ll)
    a, h = gp.alpha.ravel(), gh.alpha.ravel()
    assert np.abs(a - h).max() <= 1e-9 * np.abs(h).max()


@pytest.mark.parametrize("op", ["sum", "prod"])
def test_sum_and_product_against_host_twin(g, golden, op):
    d = _block(golden, "fit")
    se = lambda: g.SquaredExponentialKernel(num_dim=1, initial_params=[0.5, 0.7] if op == "sum" else [1.0, 1.5],
                                            param_bounds=[(1e-3, 10.0)] * 2)
    join = (lambda a, b: a + b) if op == "sum" else (lambda a, b: a * b)
    gp = g.GaussianProcess(join(G20.gp_kernel(g, G20.FIT_CASE), se()))
    gh = g.GaussianProcess(join(_host_twin(g, G20.FIT_CASE), se()))
    for m in (gp, gh):
        m.add_data(d["X"], d["y"], err_y=G20.ERR_Y, n=d["n"])
        m.compute_K_L_alpha_ll()
    assert gp._fit_mode == "kernel" and gh._fit_mode == "matrix"
    print("%s: ll %.17g native, %.17g host" % (op, gp.ll, gh.ll))
    assert abs(gp.ll - gh.ll) <= 1e-9 * abs(gh.ll)
    assert np.abs(gp.alpha - gh.alpha).max() <= 1e-9 * np.abs(gh.alpha).max()
    mean, std = gp.predict(d["Xs"], n=d["ns"])
    mh, sh = gh.predict(d["Xs"], n=d["ns"])
    np.testing.assert_allclose(mean, mh, rtol=0, atol=1e-8 * max(1.0, np.abs(mh).max()))
    np.testing.assert_allclose(std ** 2, sh ** 2, rtol=0, atol=1e-8 * max(1.0, (sh ** 2).max()))
    if op == "prod":
        rs = np.random.RandomState(3)
        xi, xj = rs.uniform(0, 2, (400, 1)), rs.uniform(0, 2, (400, 1))
        ni, nj = rs.randint(0, 2, (400, 1)), rs.randint(0, 2, (400, 1))
        assert gp.k._native_factors() is not None and gh.k._native_factors() is None
        assert_close_nan(gp.k(xi, xj, ni, nj), gh.k(xi, xj, ni, nj), rtol=1e-12, atol_scale=1e-13)
        swapped = se() * G20.gp_kernel(g, G20.FIT_CASE)
        assert_close_nan(swapped(xi, xj, ni, nj), gh.k(xi, xj, ni, nj), rtol=1e-12, atol_scale=1e-13)


def test_masked_product_in_two_dimensions(g, golden):
    """Masked(GibbsKernel1dGP, [0]) * Masked(SE, [1]) against the reference: the pair list and a fit whose data hold n = [1, 1] and a
    second derivative n = [0, 2] in the SE coordinate; n = [2, 0] is the Gibbs coordinate's and is refused."""
    d = _block(golden, "m2d")
    k = G20.make_2d_kernel(g)
    assert k._native_factors() is not None
    got = k(d["Xi"], d["Xj"], d["ni"], d["nj"])
    assert_close_nan(got, d["k"], rtol=1e-12, atol_scale=1e-13, msg="2-D pairs")
    print("2-D pairs: max abs dev / scale %.3g" % (np.abs(got - d["k"]).max() / np.abs(d["k"]).max()))
    assert (d["n"] == [0, 2]).all(axis=1).any()
    gp = g.GaussianProcess(k)
    gp.add_data(d["X"], d["y"], err_y=0.05, n=d["n"])
    gp.compute_K_L_alpha_ll()
    assert gp._fit_mode == "kernel"
    print("2-D ll %.17g, reference %.17g" % (gp.ll, float(d["ll"])))
    assert abs(gp.ll - float(d["ll"])) <= 1e-9 * max(1.0, abs(float(d["ll"])))
    n2 = d["n"].copy()
    n2[0] = [2, 0]
    bad = g.GaussianProcess(G20.make_2d_kernel(g))
    bad.add_data(d["X"], d["y"], err_y=0.05, n=n2)
    with pytest.raises(NotImplementedError, match=r"greater than \[1, 1\]"):
        bad.compute_K_L_alpha_ll()
    with pytest.raises(NotImplementedError, match=r"greater than \[1, 1\]"):
        k(d["X"][:2], d["X"][:2], np.array([[2, 0], [0, 0]]), np.zeros((2, 2), dtype=int))


def _rows(base, count):
    """`count` different parameter rows of the m5 kernel: amplitude, nested length scale, locations and values all moved."""
    rows = []
    for b in range(count):
        q = np.array(base, dtype=float)
        q[0] *= 1.0 + 0.03 * b
        q[1] *= 1.0 + 0.02 * b
        q[2:7] += 0.01 * b * np.array([0.0, 1.0, -1.0, 0.5, 0.0])
        q[7:12] *= 1.0 + 0.04 * b * np.cos(np.arange(5) + b)
        rows.append(q)
    return rows


def test_fit_batch_terms_bit_identical_to_single_fits(g):
    from gptools_amd import _lib
    rs = np.random.RandomState(23)
    N, B = 200, 5
    X = np.sort(rs.uniform(0.0, 2.0, N))[:, None]
    n = np.zeros((N, 1), dtype=int)
    n[-30:] = 1
    y = np.tanh(3.0 * (X[:, 0] - 1.0)) + 1e-2 * rs.randn(N)
    err = np.full(N, 0.05)
    kernels = []
    for q in _rows(G20.case_params("m5"), B):
        k = G20.gp_kernel(g, "m5")
        k.params = q
        kernels.append(k._native_params())
    assert len({tuple(p) for p in kernels}) == B

    def terms(b, prod):
        if not prod:
            return [(_lib.KERNEL_GIBBS_GP, kernels[b])]
        return [(_lib.KERNEL_GIBBS_GP, kernels[b], _lib.KERNEL_SE, np.array([1.0, 1.5 + 0.1 * b])), (_lib.KERNEL_SE, np.array([0.3, 0.5]))]
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
                assert (l1, d1) == (ll[b], ld[b]), (prod, b, l1 - ll[b], d1 - ld[b])
    finally:
        c.close()


def test_compute_from_mcmc_batched_equals_loop(g, golden):
    d = _block(golden, "fit")
    gp = G20.make_fit_gp(g, d)
    trace = np.array(_rows(np.array(gp.free_params[:], dtype=float), 6))
    calls = []
    orig = gp._ctx.predict_batch
    gp._ctx.predict_batch = lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp.mcmc_batch_min_rows = 2
        batched = gp.compute_from_MCMC(d["Xs"], n=d["ns"], flat_trace=trace, return_cov=True)
        assert calls, "compute_from_MCMC did not take the batched route"
        del calls[:]
        gp.batch_grid_max_n = 0                                    # forces the loop route
        loop = gp.compute_from_MCMC(d["Xs"], n=d["ns"], flat_trace=trace, return_cov=True)
        assert not calls
    for key in loop:
        a, b = np.asarray(batched[key]), np.asarray(loop[key])
        assert a.shape == b.shape and a.shape[0] == 6
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-10 * max(1.0, np.abs(b).max()), err_msg=key)


def test_linear_warp_device_route_against_host_route(g, golden):
    d = _block(golden, "fit")
    gw = g.GaussianProcess(g.LinearWarpedKernel(G20.gp_kernel(g, G20.FIT_CASE), [0.0], [2.0]))
    gh = g.GaussianProcess(g.LinearWarpedKernel(_host_twin(g, G20.FIT_CASE), [0.0], [2.0]))
    for m in (gw, gh):
        m.add_data(d["X"], d["y"], err_y=G20.ERR_Y, n=d["n"])
    assert len(gw._device_model()[1]) == 1 and gh._device_model() is None
    gw.compute_K_L_alpha_ll()
    gh.compute_K_L_alpha_ll()
    assert gw._fit_mode == "kernel" and gh._fit_mode == "matrix"
    print("warped: ll %.17g device, %.17g host" % (gw.ll, gh.ll))
    assert abs(gh.ll - gw.ll) <= 1e-9 * abs(gw.ll)
    mean, cov = gw.predict(d["Xs"], n=d["ns"], return_std=False, return_cov=True)
    mh, ch = gh.predict(d["Xs"], n=d["ns"], return_std=False, return_cov=True)
    np.testing.assert_allclose(mh, mean, rtol=0, atol=1e-9 * max(1.0, np.max(np.abs(mean))))
    np.testing.assert_allclose(ch, cov, rtol=0, atol=2e-10 * max(1.0, np.max(np.abs(cov))))


def test_debug_poison_leaves_everything_finite(g, golden):
    from gptools_amd import _lib
    d = _block(golden, "fit")
    p = G20.gp_kernel(g, G20.FIT_CASE)._native_params()
    ctx = _lib.Context(0)
    try:
        ctx.set_option("debug_poison", 1)
        ctx.set_data(d["X"][:, None], d["n"][:, None])
        err = np.full(len(d["y"]), G20.ERR_Y)
        for terms in ([(_lib.KERNEL_GIBBS_GP, p)], [(_lib.KERNEL_GIBBS_GP, p, _lib.KERNEL_SE, np.array([1.0, 1.5]))]):
            ll, ld = ctx.fit_terms(terms, 0.0, d["y"], err, 1e2 * EPS)
            assert np.isfinite(ll) and np.isfinite(ld)
            assert np.isfinite(ctx.get_alpha(len(d["y"]))).all() and np.isfinite(ctx.get_L(len(d["y"]))).all()
            mean, std, _ = ctx.predict(d["Xs"][:, None], d["ns"][:, None], 1)
            assert np.isfinite(mean).all() and np.isfinite(std).all()
            llb, _, info = ctx.fit_batch_terms([terms, terms], np.zeros(2), np.tile(d["y"], (2, 1)), err, 1e2 * EPS)
            assert (info == 0).all() and np.isfinite(llb).all() and llb[0] == ll
            out = ctx.predict_batch(d["Xs"][:, None], d["ns"][:, None], np.ones(2, dtype=np.int32), None, True, True, True)
            assert all(np.isfinite(o).all() for o in out if o is not None)
    finally:
        ctx.close()


def test_update_hyperparameters_counts_a_failed_nested_solve_as_inf(g, golden):
    d = _block(golden, "fit")
    gp = G20.make_fit_gp(g, d)
    q = np.array(gp.free_params[:], dtype=float)
    assert np.isfinite(gp.update_hyperparameters(q))
    for value in (np.nan, q[4]):                             # a location of the nested GP: NaN, or on top of its neighbour
        bad = q.copy()
        bad[3] = value
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with pytest.raises(np.linalg.LinAlgError):
                gp.update_hyperparameters(bad, inf_on_error=False, exit_on_bounds=False)
            assert gp.update_hyperparameters(bad, exit_on_bounds=False) == np.inf
    assert np.isfinite(gp.update_hyperparameters(q))


def test_refusals_through_the_c_abi(g, golden):
    from gptools_amd import _lib
    d = _block(golden, "fit")
    x = np.array([[0.5], [1.5]])
    one = np.ones((2, 1), dtype=int)
    ctx = _lib.default_context()
    kid = _lib.KERNEL_GIBBS_GP
    p = G20.gp_kernel(g, G20.FIT_CASE)._native_params()
    m13 = _lib.GIBBS_MAX_GP_POINTS + 1
    p13 = np.concatenate(([1.0, 0.3], np.linspace(0.0, 2.0, m13), np.full(m13, 0.1)))
    with pytest.raises(ValueError, match="GPT_GIBBS_MAX_GP_POINTS = %d" % _lib.GIBBS_MAX_GP_POINTS):
        ctx.kpairs(kid, p13, x, x, one, one)
    with pytest.raises(ValueError, match="GPT_GIBBS_MAX_GP_POINTS"):
        ctx.kbuild(kid, p13, x, one, None, None)
    with pytest.raises(ValueError, match="GPT_GIBBS_MAX_GP_POINTS"):
        ctx.kpairs2(_lib.KERNEL_SE, np.array([1.0, 1.0]), kid, p13, x, x, one, one)
    with pytest.raises(ValueError, match=r"2 m \+ 2"):
        ctx.kpairs(kid, p[:-1], x, x, one, one)              # an odd parameter count
    with pytest.raises(ValueError, match=r"2 m \+ 2"):
        ctx.kpairs(kid, p[:2], x, x, one, one)               # no point at all
    x2 = np.ones((2, 2))
    z2 = np.zeros((2, 2), dtype=int)
    with pytest.raises(ValueError, match="only supports 1d"):
        ctx.kpairs(kid, p, x2, x2, z2, z2)                   # the plain id at num_dim 2
    with pytest.raises(ValueError):
        ctx.kpairs(_lib.kernel_on_dim(kid, 0), p, x2, x2, z2, z2)      # a coordinate outside a product
    k = G20.gp_kernel(g, G20.FIT_CASE)
    with pytest.raises(NotImplementedError, match=r"greater than \[1, 1\]"):
        k(x, x, 2 * one, one)
    with pytest.raises(NotImplementedError, match="Hyperparameter derivatives have not been implemented!"):
        k(x, x, one, one, hyper_deriv=1)
    n2 = d["n"].copy()
    n2[-1] = 2
    gp = g.GaussianProcess(G20.gp_kernel(g, G20.FIT_CASE))
    gp.add_data(d["X"], d["y"], err_y=G20.ERR_Y, n=n2)
    with pytest.raises(NotImplementedError, match=r"greater than \[1, 1\]"):
        gp.compute_K_L_alpha_ll()
    gp = G20.make_fit_gp(g, d)
    with pytest.raises(NotImplementedError):
        gp.predict(d["Xs"][:3], n=2)
    # a non-positive nested length scale is not refused: NaN through the arithmetic
    q = p.copy()
    q[1] = 0.0
    assert np.isnan(ctx.kpairs(kid, q, x, x + 0.25, 0 * one, 0 * one)).all()
