"""GPU suite (-m gpu): SpectralKernel, one component of the spectral mixture (GPT_KERNEL_SPECTRAL, kpair.hpp spectral_pair /
spectral.hpp), and spectral_mixture on the device -- the pair list against the mpmath fixture g22, Gram matrices at the builder's tile
edges against the host build of the same header, the masked-out dimension, mu = 0 against the squared exponential, the linear-warp
identity, fit and predict against a CPU statement, the products, the batched fit, marginalised prediction, the device gradient,
library-side ensemble stepping, the block-cyclic engine and the refusals.

Yardstick for pair values: the deviation as a fraction of the entry's SCALE (sigma_f^2 times the product over the dimensions of the
largest magnitude |H_n| exp(-a tau^2 / 2) takes), bound 10 x HOST_DEV, the host aid's own measured deviation from mpmath
(tests/test_spectral_host.py): the device's exp(-x) and its contraction-free arithmetic differ from the host's by an ulp."""
import warnings

import numpy as np
import pytest
import scipy.linalg

from conftest import assert_close
from test_spectral_host import HOST_DEV, fixture_cases, load_aid, masked_dims, pair_scales, scaled_dev

pytestmark = pytest.mark.gpu

DEV_BOUND = 10 * HOST_DEV
EPS = np.finfo(float).eps
B = [(-1e3, 1e3)]


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


@pytest.fixture(scope="module")
def aid():
    return load_aid()


@pytest.fixture(scope="module")
def lib():
    from gptools_amd import _lib
    return _lib


def spectral(g, D, p):
    return g.SpectralKernel(num_dim=D, initial_params=list(p), param_bounds=B * (2 * D + 1))


def mixture(g, D, rows):
    return g.spectral_mixture(num_dim=D, num_mixtures=len(rows), initial_params=rows, param_bounds=B * (2 * D + 1))


def gram_pairs(X, n, Xs=None, ns=None):
    """The pair list of a Gram block: rows (Xs, ns) -- default the points themselves -- against columns (X, n)."""
    Xs, ns = (X, n) if Xs is None else (Xs, ns)
    M, P = len(Xs), len(X)
    return np.repeat(Xs, P, axis=0), np.tile(X, (M, 1)), np.repeat(ns, P, axis=0), np.tile(n, (M, 1))


def aid_gram(aid, rows, X, n, Xs=None, ns=None):
    """The Gram block of the mixture whose components are `rows` (one row: a single component), by the test aid."""
    Xi, Xj, ni, nj = gram_pairs(X, n, Xs, ns)
    rows = np.atleast_2d(rows)
    return sum(aid(p, Xi, Xj, ni, nj) for p in rows).reshape(len(X) if Xs is None else len(Xs), len(X))


def data(N, D, seed, nder=None, orders=(1,), lo=-2.0, hi=2.0):
    """N points in [lo, hi]^D, the last quarter (or nder) derivative rows with one order of `orders` in one dimension."""
    rs = np.random.RandomState(seed)
    X = rs.uniform(lo, hi, (N, D))
    n = np.zeros((N, D), dtype=int)
    nder = N // 4 if nder is None else nder
    for r in range(N - nder, N):
        n[r, rs.randint(D)] = orders[r % len(orders)]
    y = np.sin(2.0 * np.pi * X.sum(1) / 0.8) + 0.05 * rs.randn(N)
    return X, n, y


# ---- pair list -------------------------------------------------------------------------------------------------------------------
def test_pair_list_against_the_mpmath_fixture(g, lib, golden):
    """Every case of g22 (D = 1, 2, 3, 16; combined orders 0 .. 16 per dimension; tau = 0; phases of hundreds of cycles; mu = 0;
    infinite length scales; a masked-out dimension) through gpt_kpairs.  The measured worst scaled deviation on MI355X is printed
    (recorded in DESIGN.md)."""
    ctx = lib.default_context()
    worst = 0.0
    for c, D, f in fixture_cases(golden("g22_spectral")):
        got = ctx.kpairs(lib.KERNEL_SPECTRAL, f["params"], f["Xi"], f["Xj"], f["ni"], f["nj"])
        dev = scaled_dev(got, f["k"], f["scale"])
        print("case %d, D = %d: worst scaled deviation %.3g (order %s)" % (c, D, dev.max(), (f["ni"] + f["nj"])[dev.argmax()].max()))
        worst = max(worst, dev.max())
        masked = masked_dims(f["params"], D)
        if masked.any():
            hit = ((f["ni"] + f["nj"])[:, masked] > 0).any(axis=1)
            assert np.all(got[hit] == 0.0)
        assert np.array_equal(spectral(g, D, f["params"])(f["Xi"], f["Xj"], f["ni"], f["nj"]), got)      # the class gives the same bits
    print("worst scaled deviation from mpmath: %.3g (bound %.3g)" % (worst, DEV_BOUND))
    assert worst <= DEV_BOUND


# ---- Gram matrices at the tile edges of the 32 x 256 builder -------------------------------------------------------------------
@pytest.mark.parametrize("N,D", [(33, 1), (300, 1), (33, 3), (300, 3)])
def test_gram_matrix_against_the_test_aid(lib, aid, N, D):
    params = np.array([1.3, 0.75, 0.7]) if D == 1 else np.array([1.3, 0.75, -0.4, 1.1, 0.7, 1.6, 0.9])
    X, n, _ = data(N, D, 40 + N + D, nder=N // 2, orders=(1, 2))
    K = lib.default_context().kbuild(lib.KERNEL_SPECTRAL, params, X, n)
    assert K.shape == (N, N) and np.array_equal(K, K.T)
    Xi, Xj, ni, nj = gram_pairs(X, n)
    ref = aid(params, Xi, Xj, ni, nj).reshape(N, N)
    dev = np.abs(K - ref) / pair_scales(params, ni, nj).reshape(N, N)
    print("N = %d, D = %d: worst scaled deviation from the test aid %.3g" % (N, D, dev.max()))
    assert dev.max() <= DEV_BOUND
    # a rectangular block (every tile, not the lower triangle) holds the same numbers
    M = min(N, 40)
    assert np.array_equal(lib.default_context().kbuild(lib.KERNEL_SPECTRAL, params, X, n, X[:M], n[:M]), K[:, :M])


def test_masked_out_dimension_gives_the_bits_of_the_kernel_without_it(g, lib):
    X, n, _ = data(300, 2, 7, orders=(1, 2))
    n[:, 1] = 0
    n[-75:, 0] = np.where(n[-75:, 0] > 0, n[-75:, 0], 1)
    ctx = lib.default_context()
    K2 = ctx.kbuild(lib.KERNEL_SPECTRAL, [1.2, 0.9, 0.0, 0.6, np.inf], X, n)
    K1 = ctx.kbuild(lib.KERNEL_SPECTRAL, [1.2, 0.9, 0.6], X[:, :1], n[:, :1])
    assert np.array_equal(K2, K1) and np.ptp(K1) > 0
    # an order in the masked-out dimension: exactly zero, on either point
    n2 = n.copy()
    n2[::3, 1] = 1
    K0 = ctx.kbuild(lib.KERNEL_SPECTRAL, [1.2, 0.9, 0.0, 0.6, np.inf], X, n2)
    out = (n2[:, 1] > 0)
    assert np.all(K0[out] == 0.0) and np.all(K0[:, out] == 0.0) and np.array_equal(K0[~out][:, ~out], K1[~out][:, ~out])
    # ... which is what MaskedKernel hands over
    mk = g.MaskedKernel(spectral(g, 1, [1.2, 0.9, 0.6]), total_dim=2, mask=[0])
    Xi, Xj, ni, nj = gram_pairs(X[:40], n2[:40])
    assert np.array_equal(mk(Xi, Xj, ni, nj).reshape(40, 40), K0[:40, :40])


def test_zero_frequency_against_the_squared_exponential(lib):
    """mu = 0 is KERNEL_SE: the same pairs, orders 0 - 2, to the device bound as a fraction of the entry's scale."""
    ctx = lib.default_context()
    for D in (1, 3):
        X, n, _ = data(300, D, 19 + D, nder=150, orders=(1, 2))
        ls = np.array([0.7, 1.6, 0.9])[:D]
        p = np.concatenate(([1.3], np.zeros(D), ls))
        K = ctx.kbuild(lib.KERNEL_SPECTRAL, p, X, n)
        Kse = ctx.kbuild(lib.KERNEL_SE, np.concatenate(([1.3], ls)), X, n)
        Xi, Xj, ni, nj = gram_pairs(X, n)
        dev = np.abs(K - Kse) / pair_scales(p, ni, nj).reshape(300, 300)
        print("D = %d: mu = 0 against KERNEL_SE, worst scaled deviation %.3g" % (D, dev.max()))
        assert dev.max() <= DEV_BOUND and np.ptp(Kse) > 0


# ---- linear warp ---------------------------------------------------------------------------------------------------------------
# the bounds tests/test_gpu_warp.py applies to its own linear-layer identity (ll relative; alpha, L as a fraction of the largest entry)
LIN_LL, LIN_ALPHA, LIN_L = 9e-15, 3.1e-13, 7.6e-14


def _scaled(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b))


def _raw_fit(ctx, terms, layers, X, n, y, err, noise_var=0.09, diag_add=1e-9):
    ctx.set_data(X, n)
    ctx.set_warp(layers)
    ll, ld = ctx.fit_terms(terms, noise_var, y, err, diag_add)
    return ll, ld, ctx.get_alpha(len(y)), ctx.get_L(len(y))


def test_linear_warp_is_the_kernel_with_rescaled_scales(lib):
    """LinearWarpedKernel(Spectral; a, b) = Spectral with length scales l (b - a) and frequencies mu / (b - a), derivative rows
    included; data, layers, method and bounds of test_linear_warp_is_the_kernel_with_rescaled_periods (tests/test_gpu_periodic.py).
    Measured on MI355X: ll 8.45e-15, alpha 1.07e-13, L 1.67e-14.  The two routes differ by one rounding of every coordinate, which
    the fit sees through the kernel's slope: an absolute 1e-11 in ll at these sizes, which is the ll bound itself.  With shorter
    scales (mu = (1.5, -0.8), l = (0.3, 0.4)) the identity held ll to 1.2e-14 only, and with data the kernel describes in the place
    of white noise |ll| falls faster than the deviation (3.0e-12 of 194: 1.5e-14) -- see DESIGN.md section 16."""
    D, N = 2, 300
    rs = np.random.RandomState(78)
    X = rs.uniform(0.05, 0.95, (N, D))
    n = np.zeros((N, D), dtype=int)
    for r, d in zip(range(N - 75, N), rs.randint(0, D, 75)):
        n[r, d] = 1
    y, err = rs.randn(N), rs.uniform(0.05, 0.2, N)
    sf, mu, l = 1.2, np.array([0.75, -0.4]), np.array([0.5, 0.8])
    a, b = np.array([-1.0, 2.0]), np.array([2.0, 2.7])                 # (b - a no power of two: the two routes round differently)
    Xr = a + X * (b - a)
    ctx = lib.Context(0)
    lin = _raw_fit(ctx, [(lib.KERNEL_SPECTRAL, np.concatenate(([sf], mu, l)))], [(lib.WARP_LINEAR, np.column_stack((a, b)).ravel())],
                   Xr, n, y, err)
    wide = _raw_fit(ctx, [(lib.KERNEL_SPECTRAL, np.concatenate(([sf], mu / (b - a), l * (b - a))))], None, Xr, n, y, err)
    print("linear layer vs rescaled scales: ll %.3g alpha %.3g L %.3g" % (abs(lin[0] - wide[0]) / abs(wide[0]), _scaled(lin[2], wide[2]),
                                                                         _scaled(lin[3], wide[3])))
    assert abs(lin[0] - wide[0]) <= LIN_LL * abs(wide[0])
    assert _scaled(lin[2], wide[2]) <= LIN_ALPHA and _scaled(lin[3], wide[3]) <= LIN_L


# ---- fit and predict against the CPU statement ----------------------------------------------------------------------------------
def test_fit_and_predict_against_the_cpu_statement(g, aid):
    """A 2-component mixture at N = 300, D = 1, points in [0, 2], mu <= 3, noise 0.1, derivative rows of order 1: ll, alpha, mean,
    std and cov -- test points with n = 1 among them, noise=True -- against K from the test aid, a LAPACK Cholesky on the host and the
    same diagonal loading; bounds: those of the Periodic kernel's fit and predict."""
    N = 300
    rows = np.array([[1.1, 1.25, 0.9], [0.6, 3.0, 1.7]])
    X, n, y = data(N, 1, 11, orders=(1,), lo=0.0, hi=2.0)
    err = 0.05 * np.ones(N)
    nk = g.DiagonalNoiseKernel(1, initial_noise=0.1, fixed_noise=True)
    gp = g.GaussianProcess(mixture(g, 1, rows), noise_k=nk, X=X, y=y, err_y=err, n=n)
    gp.compute_K_L_alpha_ll()
    assert gp._fit_mode == "kernel"
    K = aid_gram(aid, rows, X, n)
    Ktot = K.copy()
    Ktot[np.diag_indices(N)] = ((np.diag(K) + 0.1 ** 2) + err ** 2) + gp.diag_factor * EPS
    L = scipy.linalg.cholesky(Ktot, lower=True)
    alpha = scipy.linalg.cho_solve((L, True), y)
    ll_ref = -0.5 * y.dot(alpha) - np.log(np.diag(L)).sum() - 0.5 * N * np.log(2.0 * np.pi) + gp.hyperprior(gp.params)
    assert abs(gp.ll - ll_ref) <= 1e-9 * abs(ll_ref)
    assert abs(np.log(np.diag(gp.L)).sum() - np.log(np.diag(L)).sum()) <= 1e-10 * abs(np.log(np.diag(L)).sum())
    assert_close(gp.alpha.ravel(), alpha, rtol=1e-6, atol_scale=1e-7, msg="alpha")
    rs = np.random.RandomState(3)
    Xs = rs.uniform(0.0, 2.0, (40, 1))
    ns = np.zeros((40, 1), dtype=int)
    ns[30:] = 1
    Ks = aid_gram(aid, rows, X, n, Xs, ns)
    V = scipy.linalg.solve_triangular(L, Ks.T, lower=True)
    mean_ref, cov_ref = Ks.dot(alpha), aid_gram(aid, rows, Xs, ns) - V.T.dot(V)
    for noise in (False, True):
        mean, cov = gp.predict(Xs, n=ns, noise=noise, return_std=False, return_cov=True)
        _, std = gp.predict(Xs, n=ns, noise=noise)
        # (the noise kernel fires where both orders are its own, 0: the value rows of the diagonal)
        want = cov_ref + (np.diag(np.where(ns[:, 0] == 0, 0.1 ** 2, 0.0)) if noise else 0.0)
        np.testing.assert_allclose(mean, mean_ref, rtol=0, atol=1e-6)
        np.testing.assert_allclose(cov, want, rtol=0, atol=1e-6)
        np.testing.assert_allclose(std ** 2, np.diag(want), rtol=0, atol=1e-6)
    # a test set of derivative rows alone (n = 1), with noise=True: no noise reaches them
    one = np.ones((10, 1), dtype=int)
    mean1, cov1 = gp.predict(Xs[30:], n=one, noise=True, return_std=False, return_cov=True)
    np.testing.assert_allclose(mean1, mean_ref[30:], rtol=0, atol=1e-6)
    np.testing.assert_allclose(cov1, cov_ref[30:, 30:], rtol=0, atol=1e-6)
    # the other users of the resident factor
    s = gp.draw_sample(Xs[:30], rand_vars=rs.randn(30, 2))
    assert s.shape == (30, 2) and np.all(np.isfinite(s))
    assert np.isfinite(gp.update_hyperparameters(rows.ravel() * 1.05)) and gp._fit_mode == "kernel"


# ---- products ------------------------------------------------------------------------------------------------------------------
def test_products_against_the_leibniz_sum(g, aid, oracle):
    """SE * Spectral, Spectral * Periodic (orders <= 2 per point) and Spectral * Spectral + Matern52 (orders <= 1, Matern52's rule)
    at N = 257, D = 2: K against the general Leibniz rule formed on the host from the factors' pair lists (test aids, CPU oracle).
    Bound: the relative tolerance the suite holds device products to (1e-11), plus the pair bound as a fraction of the matrix's
    largest entry.  Spectral * Gibbs takes the matrix route and agrees with it."""
    from gptools_amd.kernel.core import Kernel
    from test_periodic_host import load_aid as load_periodic_aid

    class HostKernel(Kernel):
        def __init__(self, fn, D, params):
            Kernel.__init__(self, num_dim=D, num_params=len(params), initial_params=list(params), param_bounds=B * len(params))
            self.fn = fn

        def __call__(self, Xi, Xj, ni, nj, hyper_deriv=None, symmetric=False):
            return self.fn(self.params, Xi, Xj, ni, nj)

    N, D = 257, 2
    pse, pspec, pspec2, pper, pm = [1.1, 1.5, 2.0], [0.9, 0.7, -0.4, 1.1, 1.3], [1.2, -0.3, 0.55, 2.1, 0.8], [0.9, 0.8, 1.1, 0.7, 1.3], [0.4, 0.9, 1.2]
    per_aid = load_periodic_aid()
    se_host = HostKernel(lambda p, *a: oracle.kpairs("se", p, *a), D, pse)
    spec_host, spec2_host = HostKernel(lambda p, *a: aid(p, *a), D, pspec), HostKernel(lambda p, *a: aid(p, *a), D, pspec2)
    per_host = HostKernel(lambda p, *a: per_aid(p, *a), D, pper)
    se = g.SquaredExponentialKernel(num_dim=D, initial_params=pse, param_bounds=B * 3)
    per = g.PeriodicKernel(num_dim=D, initial_params=pper, param_bounds=B * 5)
    m52 = g.Matern52Kernel(num_dim=D, initial_params=pm, param_bounds=B * 3)
    for label, orders, k, host, extra in (("se * spectral", (1, 2), se * spectral(g, D, pspec), se_host * spec_host, None),
                                          ("spectral * periodic", (1, 2), spectral(g, D, pspec) * per, spec_host * per_host, None),
                                          ("spectral * spectral + m52", (1,), spectral(g, D, pspec) * spectral(g, D, pspec2),
                                           spec_host * spec2_host, m52)):
        X, n, y = data(N, D, 23, orders=orders)
        assert k._native_factors() is not None and host._native_factors() is None
        if extra is not None:
            k = k + extra
        gp = g.GaussianProcess(k, X=X, y=y, err_y=0.1, n=n)
        gp.compute_K_L_alpha_ll()
        assert gp._fit_mode == "kernel" and np.isfinite(gp.ll)
        Xi, Xj, ni, nj = gram_pairs(X, n)
        ref = host(Xi, Xj, ni, nj)
        if extra is not None:
            ref = ref + oracle.kpairs("m52", pm, Xi, Xj, ni, nj)
        ref = ref.reshape(N, N)
        K = gp.K
        err = np.abs(K - ref) - 1e-11 * np.abs(ref)
        print("%s: max|K - ref| / max|ref| = %.3g" % (label, np.abs(K - ref).max() / np.abs(ref).max()))
        assert err.max() <= DEV_BOUND * np.abs(ref).max()
        # (the Leibniz sum runs over the slots in another order for the mirrored pair: symmetric to rounding, not to the bit)
        assert np.abs(K - K.T).max() <= DEV_BOUND * np.abs(ref).max()
    # Spectral * Gibbs: no device product; the matrix route combines the two factors' device pair lists on the host
    X, n, y = data(N, 1, 29, orders=(1,), lo=0.0, hi=2.0)
    gib = g.GibbsKernel1dTanh(initial_params=[1.0, 0.5, 1.0, 0.3, 0.5], param_bounds=B * 5)
    p1 = [0.9, 1.25, 1.1]
    k = spectral(g, 1, p1) * gib
    assert k._native_factors() is None
    gp = g.GaussianProcess(k, X=X, y=y, err_y=0.1, n=n)
    gp.compute_K_L_alpha_ll()
    assert gp._fit_mode == "matrix" and np.isfinite(gp.ll)
    Xi, Xj, ni, nj = gram_pairs(X, n)
    ref = (HostKernel(lambda p, *a: aid(p, *a), 1, p1) * gib)(Xi, Xj, ni, nj).reshape(N, N)
    print("spectral * gibbs: max|K - ref| / max|ref| = %.3g" % (np.abs(gp.K - ref).max() / np.abs(ref).max()))
    assert (np.abs(gp.K - ref) - 1e-11 * np.abs(ref)).max() <= DEV_BOUND * np.abs(ref).max()


# ---- the partitioned engine ------------------------------------------------------------------------------------------------------
def test_block_cyclic_engine_on_one_rank_gives_the_single_fit(lib):
    """DistributedLML builds its blocks through gpt_dev_kbuild: the same ll as gpt_fit to 1e-9 (the bound the suite holds the two
    engines to for the other kernels), and the parameter refusals reach it too."""
    from gptools_amd.dist import DistributedLML
    X, n, y = data(1500, 2, 1, nder=300)
    err = 0.05 * np.ones(1500)
    p = np.array([1.1, 0.7, -0.4, 0.9, 1.3])
    ctx = lib.Context(0)
    ctx.set_data(X, n)
    ll0, ld0 = ctx.fit(lib.KERNEL_SPECTRAL, p, 0.01, y, err, 1e2 * EPS)
    eng = DistributedLML(X, n, nb=512, device=0)
    ll1, ld1 = eng.fit(lib.KERNEL_SPECTRAL, p, y, err, noise_var=0.01, diag_factor=1e2)
    assert abs(ll1 - ll0) <= 1e-9 * abs(ll0) and abs(ld1 - ld0) <= 1e-9 * abs(ld0)
    with pytest.raises(ValueError):
        eng.fit(lib.KERNEL_SPECTRAL, [1.1, 0.7, -0.4, 0.0, 1.3], y, err, noise_var=0.01)


# ---- batched fit ---------------------------------------------------------------------------------------------------------------
def _make_gp(g, model, X, n, y, err_y=0.05, noise=0.1):
    D = X.shape[1]
    if model == "mixture":
        k = mixture(g, D, [[1.1, 1.25] + [0.9] * D, [0.6, 2.5] + [1.7] * D] if D == 1 else
                    [[1.1, 1.25, -0.4, 0.9, 1.3], [0.6, 0.5, 0.8, 1.7, 1.1]])
    else:
        k = g.SquaredExponentialKernel(num_dim=1, initial_params=[0.9, 2.5], param_bounds=B * 2) * spectral(g, 1, [1.1, 1.25, 0.9])
    return g.GaussianProcess(k, noise_k=g.DiagonalNoiseKernel(D, initial_noise=noise, noise_bound=(0.0, 5.0)), X=X, y=y, err_y=err_y, n=n)


@pytest.mark.parametrize("model", ["mixture", "se * spectral"])
def test_ll_batch_is_bit_identical_to_single_fits(g, model):
    X, n, y = data(200, 1, 5)
    gp = _make_gp(g, model, X, n, y)
    theta = np.array(gp.free_params[:], dtype=float)
    rs = np.random.RandomState(9)
    pts = [theta * (1.0 + 0.04 * rs.uniform(-1, 1, len(theta))) for _ in range(5)]
    ll = gp.ll_batch(pts)
    for i, p in enumerate(pts):
        single = _make_gp(g, model, X, n, y)
        v = single.update_hyperparameters(p)
        assert single._fit_mode == "kernel" and np.isfinite(v)
        assert ll[i] == -v, (model, i, ll[i], -v)
    assert len(set(ll)) == 5


# ---- marginalised prediction -----------------------------------------------------------------------------------------------------
def test_compute_from_mcmc_agrees_with_the_row_by_row_loop(g):
    """compute_from_MCMC over a 4-row flat_trace on the batched device route against the loop over single fits; tolerance: that of
    tests/test_gpu_mcmc_predict.py for the two routes, 1e-10 times a bound on the mixture's sigma_f^2 sum."""
    X, n, y = data(120, 1, 15, nder=20, lo=0.0, hi=2.0)
    gp = _make_gp(g, "mixture", X, n, y)
    theta = np.array(gp.free_params[:], dtype=float)
    rs = np.random.RandomState(2)
    trace = theta * (1.0 + 0.03 * rs.uniform(-1, 1, (4, len(theta))))
    Xs = rs.uniform(0.0, 2.0, (25, 1))
    ns = np.zeros((25, 1), dtype=int)
    ns[20:] = 1
    batched = gp.compute_from_MCMC(Xs, n=ns, flat_trace=trace, return_cov=True)
    gp.batch_grid_max_n = 0                                    # forces the loop route
    loop = gp.compute_from_MCMC(Xs, n=ns, flat_trace=trace, return_cov=True)
    sf2 = 2.0                                                  # (1.1^2 + 0.6^2) (1.03)^2 < 2
    assert set(batched) == set(loop) and "mean" in loop and "cov" in loop
    for key in loop:
        a, b = np.asarray(batched[key], dtype=float), np.asarray(loop[key], dtype=float)
        assert a.shape == b.shape
        print("%s: max|batched - loop| = %.3g" % (key, np.abs(a - b).max() if a.size else 0.0))
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-10 * sf2, err_msg=key)
    assert np.asarray(loop["mean"]).shape[0] == 4 and np.ptp(np.asarray(loop["mean"]), axis=0).max() > 0


# ---- gradient ------------------------------------------------------------------------------------------------------------------
def _fd_gradient(gp, theta):
    fd = np.zeros_like(theta)
    for i in range(len(theta)):
        h = 1e-5 * max(1.0, abs(theta[i]))
        tp, tm = theta.copy(), theta.copy()
        tp[i] += h
        tm[i] -= h
        fd[i] = (-gp.update_hyperparameters(tp) + gp.update_hyperparameters(tm)) / (2 * h)
    return fd


@pytest.mark.parametrize("model", ["mixture", "se * spectral"])
def test_ll_gradient_against_central_differences(g, model):
    """ll_gradient() against central differences of the device log-posterior, exactly the rule of
    test_ll_gradient_against_central_differences in tests/test_gpu_periodic.py: h = 1e-5 max(1, |theta|), rtol 2e-5,
    atol 1e-4 max|fd|; then ll_gradient_batch at three points row by row -- ll bit for bit, the gradient to the same tolerance."""
    X, n, y = data(300, 1, 31, nder=60)
    make = lambda: _make_gp(g, model, X, n, y, err_y=0.02)
    gp = make()
    theta = np.array(gp.free_params[:], dtype=float)
    assert np.isfinite(gp.update_hyperparameters(theta)) and gp._fit_mode == "kernel"
    grad = gp.ll_gradient()
    assert np.array_equal(np.array(gp.free_params[:], dtype=float), theta) and gp.K_up_to_date
    fd = _fd_gradient(make(), theta)
    print("%s: max|fd| = %.4g, max|grad - fd| / max|fd| = %.3g, grad = %s" % (model, np.abs(fd).max(), np.abs(grad - fd).max() / np.abs(fd).max(), grad))
    np.testing.assert_allclose(grad, fd, rtol=2e-5, atol=1e-4 * np.abs(fd).max(), err_msg=model)
    freqs = [1, 4] if model == "mixture" else [3]
    assert np.all(grad[freqs] != 0.0)
    rs = np.random.RandomState(7)
    pts = [theta * (1.0 + 0.04 * rs.uniform(-1, 1, len(theta))) for _ in range(3)]
    ll, gb = gp.ll_gradient_batch(pts)
    for i, p in enumerate(pts):
        single = make()
        v = single.update_hyperparameters(p)
        assert ll[i] == -v
        ref = single.ll_gradient()
        print("%s, point %d: max|grad_batch - grad_single| / max|grad_single| = %.3g" % (model, i, np.abs(gb[i] - ref).max() / np.abs(ref).max()))
        np.testing.assert_allclose(gb[i], ref, rtol=2e-5, atol=1e-4 * np.abs(ref).max(), err_msg="%s, point %d" % (model, i))


# ---- library-side ensemble stepping ----------------------------------------------------------------------------------------------
def test_library_stepping_gives_the_host_loops_chain(g):
    X, n, y = data(64, 1, 13, nder=16)
    # (one component: 3 parameters and the noise -- the sampler wants at least twice as many walkers as dimensions)
    box = [(0.2, 3.0), (0.2, 3.0), (0.3, 3.0), (1e-3, 1.0)]
    k = g.SpectralKernel(num_dim=1, initial_params=[1.0, 1.25, 0.9], param_bounds=box[:3])
    gp = g.GaussianProcess(k, noise_k=g.DiagonalNoiseKernel(1, initial_noise=0.05, noise_bound=box[3]), X=X, y=y, err_y=0.02, n=n)
    box = np.array(box)
    theta0 = np.random.RandomState(41).uniform(box[:, 0], box[:, 1], size=(8, 4))
    host = gp.sample_hyperparameter_posterior(nwalkers=8, nsamp=3, theta0=theta0, random_state=41, stepping="host")
    libs = gp.sample_hyperparameter_posterior(nwalkers=8, nsamp=3, theta0=theta0, random_state=41, stepping="library")
    assert host.route == "host" and libs.route == "library" and host.chain.shape == (8, 3, 4)
    np.testing.assert_array_equal(libs.chain, host.chain)
    np.testing.assert_array_equal(libs.lnprobability, host.lnprobability)
    np.testing.assert_array_equal(libs.acceptance_fraction, host.acceptance_fraction)
    assert np.isfinite(host.lnprobability[:, -1]).any() and (np.diff(host.chain, axis=1) != 0).any()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch_and_leave_the_context_usable(g, lib):
    X, n, y = data(64, 2, 17, nder=16)
    err = 0.05 * np.ones(64)
    ok = [1.1, 0.7, -0.4, 0.9, 1.3]
    ctx = lib.Context(0)
    ctx.set_data(X, n)
    ll0, _ = ctx.fit_terms([(lib.KERNEL_SPECTRAL, ok)], 0.01, y, err, 1e-12)
    alpha0 = ctx.get_alpha(64)

    def still_fine():
        ll1, _ = ctx.fit_terms([(lib.KERNEL_SPECTRAL, ok)], 0.01, y, err, 1e-12)
        assert ll1 == ll0 and np.array_equal(ctx.get_alpha(64), alpha0)
    # NaN or infinite mu; l = 0 or NaN
    for bad in ([1.1, np.nan, -0.4, 0.9, 1.3], [1.1, 0.7, np.inf, 0.9, 1.3], [1.1, 0.7, -np.inf, 0.9, 1.3], [1.1, 0.7, -0.4, 0.0, 1.3],
                [1.1, 0.7, -0.4, 0.9, np.nan]):
        with pytest.raises(ValueError):
            ctx.fit_terms([(lib.KERNEL_SPECTRAL, bad)], 0.01, y, err, 1e-12)
        with pytest.raises(ValueError):
            ctx.kbuild(lib.KERNEL_SPECTRAL, bad, X, n)
        with pytest.raises(ValueError):
            ctx.fit_batch_terms([[(lib.KERNEL_SPECTRAL, ok)], [(lib.KERNEL_SPECTRAL, bad)]], np.full(2, 0.01), np.tile(y, (2, 1)), err, 1e-12)
        # the refused fits left the resident factor alone, and a valid call succeeds
        assert np.array_equal(ctx.get_alpha(64), alpha0)
        still_fine()
    # l = inf is legal: no envelope in that dimension
    assert np.all(np.isfinite(ctx.kbuild(lib.KERNEL_SPECTRAL, [1.1, 0.7, -0.4, np.inf, 1.3], X, n)))
    # a combined order of 17 in one dimension: pair lists, Gram blocks, training data (2 x 9), test points
    k = spectral(g, 2, ok)
    one = np.zeros((1, 2))
    with pytest.raises(ValueError, match="SpectralKernel"):
        k(one, one + 0.3, np.array([[17, 0]]), np.array([[0, 0]]))
    with pytest.raises(ValueError):
        k(one, one + 0.3, np.array([[9, 0]]), np.array([[8, 3]]))
    assert np.isfinite(k(one, one + 0.3, np.array([[16, 3]]), np.array([[0, 13]]))).all()      # 16 per dimension is the limit, not the sum
    n9 = n.copy()
    n9[-1] = [9, 0]
    with pytest.raises(ValueError):
        ctx.kbuild(lib.KERNEL_SPECTRAL, ok, X, n9)
    ctx.set_data(X, n9)
    with pytest.raises(ValueError):
        ctx.fit_terms([(lib.KERNEL_SPECTRAL, ok)], 0.01, y, err, 1e-12)
    ctx.set_data(X, n)
    still_fine()
    with pytest.raises(ValueError):
        ctx.predict(X[:3], np.array([[16, 0], [0, 0], [0, 0]]), 0)
    mean = ctx.predict(X[:3], np.array([[8, 0], [0, 8], [0, 0]]), 0)[0]
    assert np.all(np.isfinite(mean))
    # a Spectral x Gibbs product is not a device model, and the library says so
    for ids in ((lib.KERNEL_SPECTRAL, [1.0, 0.9, 0.8], lib.KERNEL_GIBBS_TANH, [1.0, 0.5, 1.0, 0.3, 0.5]),
                (lib.KERNEL_GIBBS_TANH, [1.0, 0.5, 1.0, 0.3, 0.5], lib.KERNEL_SPECTRAL, [1.0, 0.9, 0.8])):
        with pytest.raises(ValueError, match="Spectral x Gibbs"):
            ctx.kpairs2(ids[0], ids[1], ids[2], ids[3], one[:, :1], one[:, :1] + 0.3, np.zeros((1, 1), int), np.zeros((1, 1), int))
    still_fine()
    # ... and through GaussianProcess: the next fit succeeds
    gp = g.GaussianProcess(spectral(g, 2, ok), X=X, y=y, err_y=err, n=n)
    assert np.isfinite(gp.update_hyperparameters(ok))
