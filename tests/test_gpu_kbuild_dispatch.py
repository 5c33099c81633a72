"""GPU suite: every covariance launcher at every num_dim (1 .. GPT_MAX_DIM = 16).

The host code in front of the builders turns the run-time (kernel_id, num_dim) into one instantiation of a kernel template
(gptools_amd/csrc/kbuild_kernel.hpp); a slip there shows at ONE num_dim of ONE launcher only.  So each route is driven at
each num_dim, with a different length scale per dimension and first-derivative orders in the LAST dimension (a wrong D then
changes the numbers): pair list and builder (rectangular and lower-triangle launch) against the CPU oracle, the product
kernels against the product of the oracle's factors, the noise term of a prediction, the gradient pass, and the batched
builders (fit, cross-covariance, diagonal, covariance sum) against single fits.  Shapes are the smallest that cross the tile
edges (KB_ROWS = 32, KB_COLS = 256): 40 x 300 blocks, 300 points, 300 pairs; fits at N = 130 (two 128-column leaves).
Tolerances are those of the tests that make the same comparisons at a few num_dim (named at each use).
"""
import sys
import warnings

import numpy as np
import pytest

from conftest import assert_close, assert_close_nan

pytestmark = pytest.mark.gpu
EPS = sys.float_info.epsilon
DIMS = list(range(1, 17))
SE, M52, NOISE, RQ, MATERN, GIBBS = 0, 1, 2, 4, 5, 7
KID = {"se": SE, "m52": M52, "rq": RQ, "matern": MATERN}
# tests/test_gpu_parity.py: test_g2_compute_Kij / test_fit_matches_oracle (se, m52), test_g8_rational_quadratic_kernel_call (rq),
# test_g10_matern_general_nu_pairs (matern)
TOL = {"se": dict(rtol=1e-12), "m52": dict(rtol=1e-12), "rq": dict(rtol=1e-10, atol_scale=1e-13),
       "matern": dict(rtol=1e-9, atol_scale=1e-12)}
NFIT = 130


@pytest.fixture(scope="module")
def ctx():
    from gptools_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2():
    from gptools_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _params(kern, D, rs):
    """[sigma_f, (alpha | nu), l_1 .. l_D] with a different length scale per dimension"""
    head = {"se": [1.3], "m52": [1.3], "rq": [1.1, 1.7], "matern": [1.1, 2.2]}[kern]
    return np.concatenate((head, 0.5 + rs.rand(D)))


def _points(rs, M, D, every):
    """M points in [0, 1]^D; every `every`-th one is a first derivative along the LAST dimension"""
    X = rs.rand(M, D)
    n = np.zeros((M, D), dtype=np.int32)
    n[every - 1::every, D - 1] = 1
    return X, n


def _close(kern, got, want, msg):
    (assert_close_nan if kern == "matern" else assert_close)(got, want, msg=msg, **TOL[kern])


@pytest.mark.parametrize("kern", ["se", "m52", "rq", "matern"])
@pytest.mark.parametrize("D", DIMS)
def test_pair_list_and_builder_against_the_oracle(ctx, oracle, kern, D):
    rs = np.random.RandomState(100 * D + KID[kern])
    p = _params(kern, D, rs)
    Xi, ni = _points(rs, 300, D, 7)
    Xj, nj = _points(rs, 300, D, 5)
    _close(kern, ctx.kpairs(KID[kern], p, Xi, Xj, ni, nj), oracle.kpairs(kern, p, Xi, Xj, ni, nj), "kpairs %s D=%d" % (kern, D))
    _close(kern, ctx.kbuild(KID[kern], p, Xi[:40], ni[:40], Xj, nj), oracle.kbuild(kern, p, Xi[:40], ni[:40], Xj, nj),
           "kbuild 40 x 300 %s D=%d" % (kern, D))
    _close(kern, ctx.kbuild(KID[kern], p, Xi, ni), oracle.kbuild(kern, p, Xi, ni), "kbuild 300, Xj omitted %s D=%d" % (kern, D))


@pytest.mark.parametrize("D", DIMS)
def test_product_pair_list_and_builder_against_the_product_of_the_oracle_factors(ctx, oracle, D):
    """SE * RQ, all orders zero: the element-wise product of the oracle's two results; rtol (and the absolute floor) the sum of the
    two factors' tolerances above."""
    rs = np.random.RandomState(300 + D)
    p1, p2 = _params("se", D, rs), _params("rq", D, rs)
    Xi, Xj = rs.rand(300, D), rs.rand(300, D)
    z = np.zeros((300, D), dtype=np.int32)
    tol = dict(rtol=2e-10, atol_scale=2e-13)
    assert_close(ctx.kpairs2(SE, p1, RQ, p2, Xi, Xj, z, z), oracle.kpairs("se", p1, Xi, Xj, z, z) * oracle.kpairs("rq", p2, Xi, Xj, z, z),
                 msg="kpairs2 D=%d" % D, **tol)
    assert_close(ctx.kbuild2(SE, p1, RQ, p2, Xi[:40], z[:40], Xj, z),
                 oracle.kbuild("se", p1, Xi[:40], z[:40], Xj, z) * oracle.kbuild("rq", p2, Xi[:40], z[:40], Xj, z),
                 msg="kbuild2 40 x 300 D=%d" % D, **tol)
    assert_close(ctx.kbuild2(SE, p1, RQ, p2, Xi, z), oracle.kbuild("se", p1, Xi, z) * oracle.kbuild("rq", p2, Xi, z),
                 msg="kbuild2 300, Xj omitted D=%d" % D, **tol)


@pytest.mark.parametrize("D", DIMS)
def test_noise_term_of_a_prediction(ctx, oracle, D):
    """predict(noise=True) adds the noise kernel over the test points (launch_add_noise_sym); comparison and tolerance of
    test_g3_noise_kernel_and_predict_noise (absolute 1e-7).  Test points 0 and 2 coincide (the noise couples them), point 1
    differs from point 0 in the last dimension only, point 3 is a derivative in the last dimension (no noise on it)."""
    rs = np.random.RandomState(500 + D)
    N, M, sn = 17, 9, 0.3
    X, n = _points(rs, N, D, 6)
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(N)
    err = np.full(N, 0.05)
    p = _params("se", D, rs)
    Xs, ns = _points(rs, M, D, M + 1)
    Xs[2] = Xs[0]
    Xs[1] = Xs[0]
    Xs[1, D - 1] += 0.25
    ns[3, D - 1] = 1
    ref = oracle.fit("se", p, X, n, y, err, noise_var=sn ** 2)
    nn = np.zeros(D, dtype=np.int32)
    mr, sr, cr = oracle.predict("se", p, X, n, ref["L"], ref["alpha"], Xs, ns, noise_params=[sn], noise_n=nn)
    _, _, cr0 = oracle.predict("se", p, X, n, ref["L"], ref["alpha"], Xs, ns)
    assert abs((cr - cr0)[0, 2] - sn ** 2) < 1e-12 and (cr - cr0)[0, 1] == 0 and (cr - cr0)[3, 3] == 0      # (the case is what it says)
    ctx.set_data(X, n)
    ctx.fit(SE, p, sn ** 2, y, err, 1e2 * EPS)
    mean, std, cov = ctx.predict(Xs, ns, 2, noise_params=[sn], noise_n=nn)
    np.testing.assert_allclose(mean, mr, rtol=0, atol=1e-7)
    np.testing.assert_allclose(cov, cr, rtol=0, atol=1e-7)
    np.testing.assert_allclose(std ** 2, np.diag(cr), rtol=0, atol=1e-7)
    _, _, cov0 = ctx.predict(Xs, ns, 2)
    np.testing.assert_allclose(cov0, cr0, rtol=0, atol=1e-7)


@pytest.mark.parametrize("D", DIMS)
def test_gradient_pass(D):
    """gpt_ll_grad (launch_grad_reduce) through update_hyperparameters; comparison and tolerances of
    test_device_ll_gradient_against_host_path_and_finite_differences: the reference-shaped host path and central differences."""
    import gptools_amd as g
    rs = np.random.RandomState(700 + D)
    X, n = _points(rs, NFIT, D, 9)
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(NFIT)
    p = _params("se", D, rs)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")

        def make():
            k = g.SquaredExponentialKernel(num_dim=D, initial_params=list(p), param_bounds=[(0.0, 1e3)] * (D + 1))
            nk = g.DiagonalNoiseKernel(num_dim=D, initial_noise=0.1, noise_bound=(0.0, 5.0))
            return g.GaussianProcess(k, noise_k=nk, X=X, y=y, err_y=0.02, n=n, use_hyper_deriv=True)
        gp = make()
        theta = np.array(gp.free_params[:], dtype=float)
        calls = []
        orig = gp._ctx.ll_grad
        gp._ctx.ll_grad = lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1]
        val, grad = gp.update_hyperparameters(theta)
        gp._ctx.ll_grad = orig
        assert calls, "the gradient did not take the device pass"
        gp2 = make()
        gp2.use_hyper_deriv = False
        gp2.update_hyperparameters(theta)
        gp2._fit_mode = "matrix"
        gp2._compute_ll_deriv()
        assert_close(-grad, gp2.ll_deriv, rtol=1e-7, atol_scale=1e-9)
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


def _cmp(got, want, tol, msg):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (msg, got.shape, want.shape)
    np.testing.assert_allclose(got, want, rtol=0, atol=tol, err_msg=msg)


@pytest.mark.parametrize("model", ["se", "se*rq"])
@pytest.mark.parametrize("D", DIMS)
def test_batched_fit_and_prediction_against_single_fits(ctx, ctx2, model, D):
    """Three elements: fit_batch (SE) / fit_batch_terms (SE * RQ) bit for bit the three single fits
    (test_fit_batch_is_bit_identical_to_single_fits, test_fit_batch_terms_products_and_transform_bit_identical); predict_batch
    -- cross builder, kdiag_batch, kss_sum -- against fit + predict per element with the comparison of
    test_cabi_predict_batch_matches_fit_and_predict_per_element (absolute 1e-10 max(1, sigma_f^2))."""
    rs = np.random.RandomState(900 + D)
    B, M = 3, 33
    X, n = _points(rs, NFIT, D, 9)
    Xs, ns = _points(rs, M, D, 8)
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(NFIT)
    err = np.full(NFIT, 0.05)
    Y = y[None, :] + 0.01 * rs.randn(B, NFIT)
    sn = np.array([0.1, 0.05, 0.2])
    nv = sn ** 2
    P1 = [_params("se", D, rs) for _ in range(B)]
    P2 = [_params("rq", D, rs) for _ in range(B)]
    terms = [[(SE, P1[b])] if model == "se" else [(SE, P1[b], RQ, P2[b])] for b in range(B)]
    ctx.set_data(X, n)
    ctx2.set_data(X, n)
    if model == "se":
        ll, ld, info = ctx.fit_batch(SE, np.array(P1), nv, Y, err, 1e2 * EPS)
    else:
        ll, ld, info = ctx.fit_batch_terms(terms, nv, Y, err, 1e2 * EPS)
    assert not info.any()
    nn = np.zeros(D, dtype=np.int32)
    mean, var, cov, cov_sum = ctx.predict_batch(Xs, ns, np.ones(B, dtype=np.int32), nn, True, True, True)
    total = np.zeros_like(cov_sum)
    sf2 = 1.0
    for b in range(B):
        if model == "se":
            l1, d1 = ctx2.fit(SE, P1[b], nv[b], Y[b], err, 1e2 * EPS)
        else:
            l1, d1 = ctx2.fit_terms(terms[b], nv[b], Y[b], err, 1e2 * EPS)
        assert (l1, d1) == (ll[b], ld[b]), (model, D, b, l1 - ll[b], d1 - ld[b])
        m1, s1, c1 = ctx2.predict(Xs, ns, 2, noise_params=[sn[b]], noise_n=nn)
        s2 = P1[b][0] ** 2 * (1.0 if model == "se" else P2[b][0] ** 2)
        sf2 = max(sf2, s2)
        tol = 1e-10 * max(1.0, s2)
        _cmp(mean[b], m1, tol, "mean %d" % b)
        _cmp(var[b], s1 ** 2, tol, "var %d" % b)
        _cmp(cov[b], c1, tol, "cov %d" % b)
        total += cov[b]
    _cmp(cov_sum, total, 1e-10 * sf2 * B, "cov_sum")


def test_refusals_leave_the_context_usable(ctx):
    """What the dispatch (or the C ABI in front of it) refuses, with the exception the C status maps to, and one valid call on the
    same context after each."""
    rs = np.random.RandomState(3)
    X2, n2 = _points(rs, 40, 2, 7)
    y, err = rs.randn(40), np.full(40, 0.1)
    p_se = [1.0, 0.7, 0.9]

    def still_works():
        out = ctx.kbuild(SE, p_se, X2, n2)
        assert out.shape == (40, 40) and np.all(np.isfinite(out))
    with pytest.raises(ValueError):                       # a Gibbs id (1-D kernels) with 2-D points
        ctx.kbuild(GIBBS, [1.1, 0.8, 0.6, 0.3, 0.5], X2, n2)
    still_works()
    with pytest.raises(ValueError):
        ctx.kpairs(GIBBS, [1.1, 0.8, 0.6, 0.3, 0.5], X2, X2, n2, n2)
    still_works()
    for kid in (6, 12, 99, -1):                           # unknown (6, GPT_KERNEL_PRODUCT, is not a kernel a caller may name)
        with pytest.raises(ValueError):
            ctx.kbuild(kid, p_se, X2, n2)
        with pytest.raises(ValueError):
            ctx.kpairs(kid, p_se, X2, X2, n2, n2)
        still_works()
    ctx.set_data(X2, n2)
    with pytest.raises(ValueError):                       # the noise kernel is no term of a batched fit
        ctx.fit_batch(NOISE, np.array([[0.1], [0.2]]), np.zeros(2), np.tile(y, (2, 1)), err, 0.0)
    with pytest.raises(ValueError):
        ctx.fit_batch_terms([[(SE, p_se), (NOISE, [0.1])]] * 2, np.zeros(2), np.tile(y, (2, 1)), err, 0.0)
    still_works()
    ll = ctx.fit_batch(SE, np.array([p_se, p_se]), np.zeros(2), np.tile(y, (2, 1)), err, 1e2 * EPS)[0]
    assert np.all(np.isfinite(ll))
    # warp layers set: the noise kernel takes no slopes -- as a term of a warped fit it is refused, and its own Gram block is
    # built unwarped (the layers do not apply to it)
    from gptools_amd import _lib
    ctx.set_warp([(_lib.WARP_LINEAR, np.array([0.0, 1.5, -0.5, 2.0]))])
    try:
        with pytest.raises(ValueError):
            ctx.fit_terms([(SE, p_se), (NOISE, [0.1])], 0.0, y, err, 1e2 * EPS)
        plain = np.where(np.equal.outer(np.arange(40), np.arange(40)) & (n2.sum(1) == 0)[:, None], 0.1 ** 2, 0.0)
        np.testing.assert_array_equal(ctx.kbuild(NOISE, [0.1], X2, n2), plain)
        assert np.all(np.isfinite(ctx.fit_terms([(SE, p_se)], 0.0, y, err, 1e2 * EPS)))
    finally:
        ctx.set_warp(None)
    still_works()
