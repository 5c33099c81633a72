"""GPU suite (-m gpu): the gradient half of a resident batch -- gpt_ll_grad_diff_batch (kgrad.hip, api_grad_batch.inc) through
Context.ll_grad_diff_batch, GaussianProcess.ll_gradient_batch and optimize_hyperparameters(batch_starts=True).

Yardstick for "equals the single route": gp.ll_gradient() of a fresh GP at the same point, within the bound both routes are held to
against central differences in tests/test_gpu_grad_diff.py: rtol 2e-5, atol 1e-4 max|grad_single|.  ll must be
-update_hyperparameters(p) bit for bit.  Per-element independence, residency and the refusals are exact statements."""
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


def inputs(N, d, nder=60, seed=31):
    """The inputs rule of tests/test_gpu_grad_diff.py (its own copy)."""
    rs = np.random.RandomState(seed)
    X = rs.rand(N, d)
    n = np.zeros((N, d), dtype=int)
    if nder:
        n[-nder:, 0] = 1
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(N)
    return X, n, y


def noise(g, d, free=True):
    return g.DiagonalNoiseKernel(num_dim=d, initial_noise=0.1, noise_bound=(0.0, 5.0), fixed_noise=not free)


def points_around(gp, B, seed=7, spread=0.04):
    """B points within +-4 % of the initial values (all well inside the bounds the models below use)."""
    theta = np.array(gp.free_params[:], dtype=float)
    rs = np.random.RandomState(seed)
    return [theta * (1.0 + spread * rs.uniform(-1.0, 1.0, len(theta))) for _ in range(B)]


def check_against_single(make, label, B=5):
    gp = make()
    own = np.array(gp.free_params[:], dtype=float)
    pts = points_around(gp, B)
    ll, grad = gp.ll_gradient_batch(pts)
    assert np.array_equal(np.array(gp.free_params[:], dtype=float), own)
    assert ll.shape == (B,) and grad.shape == (B, len(own))
    worst = 0.0
    for i, p in enumerate(pts):
        single = make()
        v = single.update_hyperparameters(p)
        assert single._fit_mode == "kernel" and np.isfinite(v)
        assert ll[i] == -v, (label, i, ll[i], -v)
        ref = single.ll_gradient()
        scale = np.abs(ref).max()
        worst = max(worst, np.abs(grad[i] - ref).max() / scale)
        np.testing.assert_allclose(grad[i], ref, rtol=2e-5, atol=1e-4 * scale, err_msg="%s, point %d" % (label, i))
    print("%s: p = %d, B = %d, N = %d: max|grad_batch - grad_single| / max|grad_single| = %.3g" % (label, len(own), B, len(gp.y), worst))
    return gp, pts, ll, grad


def m52(g, N, d=2, nder=None):
    X, n, y = inputs(N, d, nder=min(60, N // 4) if nder is None else nder)
    return lambda: g.GaussianProcess(
        g.Matern52Kernel(num_dim=d, initial_params=[1.1, 0.4, 0.6, 0.9][:d + 1], param_bounds=[(0.0, 1e3)] * (d + 1)), noise_k=noise(g, d),
        X=X, y=y, err_y=0.02, n=n)


# ---- models -------------------------------------------------------------------------------------------------------------------
def test_m52_3d_with_derivative_rows_and_free_noise(g):
    check_against_single(m52(g, 300, d=3, nder=60), "m52 d=3")


def test_rq_plus_se_sum(g):
    X, n, y = inputs(300, 2)
    check_against_single(lambda: g.GaussianProcess(
        g.RationalQuadraticKernel(num_dim=2, initial_params=[1.0, 1.7, 0.4, 0.6], param_bounds=[(0.0, 1e3)] * 4) +
        g.SquaredExponentialKernel(num_dim=2, initial_params=[0.3, 1.5, 2.5], param_bounds=[(0.0, 1e3)] * 3), noise_k=noise(g, 2),
        X=X, y=y, err_y=0.02, n=n), "rq + se")


def test_se_times_m52_product(g):
    X, n, y = inputs(300, 2)
    check_against_single(lambda: g.GaussianProcess(
        g.SquaredExponentialKernel(num_dim=2, initial_params=[1.1, 0.8, 1.2], param_bounds=[(0.0, 1e3)] * 3) *
        g.Matern52Kernel(num_dim=2, initial_params=[0.9, 0.7, 0.9], param_bounds=[(0.0, 1e3)] * 3), noise_k=noise(g, 2), X=X, y=y,
        err_y=0.02, n=n), "se * m52")


def test_gibbs_exp_gauss_eleven_parameters_take_two_launch_groups(g):
    X, n, y = inputs(300, 1, nder=30)
    p = [1.1, 0.35, 0.2, 0.5, 0.8, 0.15, 0.2, 0.1, 0.4, -0.5, 0.3]
    _, _, _, grad = check_against_single(lambda: g.GaussianProcess(
        g.GibbsKernel1dExpGauss(3, initial_params=p, param_bounds=[(-10.0, 10.0)] * 11), noise_k=noise(g, 1, free=False), X=X, y=y,
        err_y=0.05, n=n), "gibbs exp-gauss")
    assert grad.shape[1] == 11 and np.all(grad != 0.0)


def test_masked_gibbs_tanh_times_se(g):
    X, n, y = inputs(257, 2)

    def make():
        gib = g.GibbsKernel1dTanh(initial_params=[1.2, 0.3, 0.8, 0.2, 0.5], param_bounds=[(1e-3, 10.0)] * 5)
        se = g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 0.6], fixed_params=[True, False], param_bounds=[(0.0, 10.0)] * 2)
        return g.GaussianProcess(g.MaskedKernel(gib, 2, [0]) * g.MaskedKernel(se, 2, [1]), noise_k=noise(g, 2), X=X, y=y, err_y=0.02, n=n)
    check_against_single(make, "masked gibbs-tanh * se")


def test_constant_mean_with_a_free_parameter(g):
    X, n, y = inputs(300, 2, nder=0)
    _, _, _, grad = check_against_single(lambda: g.GaussianProcess(
        g.Matern52Kernel(num_dim=2, initial_params=[1.1, 0.4, 0.6], param_bounds=[(0.0, 1e3)] * 3), noise_k=noise(g, 2),
        mu=g.ConstantMeanFunction(initial_params=[0.3]), X=X, y=y + 0.5, err_y=0.02, n=n), "m52 + constant mean")
    assert grad.shape[1] == 5


# ---- edges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [33, 127, 128, 257])
def test_tile_and_leaf_edges(g, N, B):
    """N = 33: one ragged tile, one leaf; 127: the augmented row is the last row of the only leaf; 128: it opens a second leaf;
    257: one column into the second 256-column tile."""
    check_against_single(m52(g, N), "m52 N=%d" % N, B=B)


# ---- independence -------------------------------------------------------------------------------------------------------------
def test_an_elements_rows_do_not_depend_on_the_batch_around_it(g):
    make = m52(g, 300)
    gp = make()
    p, q, r = points_around(gp, 3, seed=11)
    ll3, g3 = gp.ll_gradient_batch([p, q, r])
    ll2, g2 = gp.ll_gradient_batch([r, p])
    ll1, g1 = gp.ll_gradient_batch([q])
    assert np.all(np.isfinite(g3))
    assert np.array_equal(g3[0], g2[1]) and np.array_equal(g3[2], g2[0]) and np.array_equal(g3[1], g1[0])
    assert ll3[0] == ll2[1] and ll3[2] == ll2[0] and ll3[1] == ll1[0]


def test_the_chunk_size_does_not_show(g):
    make = m52(g, 300)
    pts = points_around(make(), 5, seed=12)
    res = {}
    for grid in (2, 8):
        gp = make()
        gp.batch_grid = grid
        res[grid] = gp.ll_gradient_batch(pts)
    assert np.all(np.isfinite(res[8][1]))
    assert np.array_equal(res[2][0], res[8][0]) and np.array_equal(res[2][1], res[8][1])


# ---- Context level ------------------------------------------------------------------------------------------------------------
DIAG_ADD = 1e2 * sys.float_info.epsilon


def m52_stencil(params, rel=6e-6):
    pa, pb, dn = [], [], []
    for i in range(len(params)):
        eps = rel * max(1.0, abs(params[i]))
        a, b = np.array(params, dtype=float), np.array(params, dtype=float)
        a[i] -= eps
        b[i] += eps
        pa.append(a)
        pb.append(b)
        dn.append(b[i] - a[i])
    return pa, pb, np.array(dn)


def resident(g, ctx, params_list, y_rows, X, n, kid=None):
    kid = g._lib.KERNEL_M52 if kid is None else kid
    ll, _, info = ctx.fit_batch_terms([[(kid, np.array(p, dtype=float))] for p in params_list], np.full(len(params_list), 0.01),
                                      np.array(y_rows), np.full(X.shape[0], 0.02), DIAG_ADD)
    return ll, info


def test_a_bad_element_is_nan_and_its_neighbours_do_not_notice(g):
    X, n, y = inputs(200, 2, nder=20)
    ctx = g._lib.Context(0)
    ctx.set_data(X, n)
    ps = [[1.1, 0.4, 0.6], [0.9, 0.5, 0.7], [1.2, 0.35, 0.55]]
    sts = [m52_stencil(p) for p in ps]
    ybad = y.copy()
    ybad[17] = np.nan
    _, info = resident(g, ctx, ps, [y, ybad, y], X, n)
    assert info[0] == 0 and info[2] == 0 and info[1] == len(y)
    out3, alpha3 = ctx.ll_grad_diff_batch([0, 0, 0], [s[0] for s in sts], [s[1] for s in sts], [s[2] for s in sts], info == 0,
                                          want_alpha=True)
    assert np.all(np.isnan(out3[1])) and np.all(np.isnan(alpha3[1]))
    assert np.all(np.isfinite(out3[[0, 2]])) and np.all(np.isfinite(alpha3[[0, 2]]))
    _, info2 = resident(g, ctx, [ps[0], ps[2]], [y, y], X, n)
    assert np.all(info2 == 0)
    out2, alpha2 = ctx.ll_grad_diff_batch([0, 0, 0], [sts[0][0], sts[2][0]], [sts[0][1], sts[2][1]], [sts[0][2], sts[2][2]], info2 == 0,
                                          want_alpha=True)
    assert np.array_equal(out3[[0, 2]], out2) and np.array_equal(alpha3[[0, 2]], alpha2)
    # the single route's numbers at element 0, within its own yardstick; the noise trace and alpha from the same factor
    ctx.fit(g._lib.KERNEL_M52, np.array(ps[0]), 0.01, y, np.full(len(y), 0.02), DIAG_ADD)
    single = ctx.ll_grad_diff([0, 0, 0], *sts[0])
    np.testing.assert_allclose(out2[0], single, rtol=2e-5, atol=1e-4 * np.abs(single).max())
    np.testing.assert_allclose(alpha2[0], ctx.get_alpha(len(y)), rtol=1e-9, atol=1e-9 * np.abs(alpha2[0]).max())
    # all elements skipped: NaN rows, nothing launched
    out0, _ = ctx.ll_grad_diff_batch([0, 0, 0], [sts[0][0], sts[2][0]], [sts[0][1], sts[2][1]], [sts[0][2], sts[2][2]], [0, 0])
    assert np.all(np.isnan(out0))
    # no entries: the noise trace alone, the same bits
    outt, _ = ctx.ll_grad_diff_batch([], [[], []], [[], []], np.zeros((2, 0)), [1, 1])
    assert outt.shape == (2, 1) and np.array_equal(outt[:, 0], out2[:, -1])


def test_state_residency_and_refusals(g):
    X, n, y = inputs(200, 2, nder=20)
    ctx = g._lib.Context(0)
    ctx.set_data(X, n)
    ps = [[1.1, 0.4, 0.6], [0.9, 0.5, 0.7]]
    sts = [m52_stencil(p) for p in ps]
    args = ([0, 0, 0], [s[0] for s in sts], [s[1] for s in sts], [s[2] for s in sts], [1, 1])
    with pytest.raises(g._lib.GPTBackendError):
        ctx.ll_grad_diff_batch(*args)                          # nothing fitted on this context yet
    _, info = resident(g, ctx, ps, [y, y], X, n)
    assert np.all(info == 0)
    Xs, ns = np.random.RandomState(2).rand(7, 2), np.zeros((7, 2), dtype=int)
    before = ctx.predict_batch(Xs, ns, [1, 1], want_cov=True)
    out = ctx.ll_grad_diff_batch(*args)[0]
    after = ctx.predict_batch(Xs, ns, [1, 1], want_cov=True)
    for a, b in zip(before[:3], after[:3]):
        assert np.array_equal(a, b)
    assert np.array_equal(ctx.ll_grad_diff_batch(*args)[0], out)      # repeat calls: the same bits
    # length checks of the binding
    with pytest.raises(ValueError, match="parameters"):
        ctx.ll_grad_diff_batch(args[0], [[p[:-1] for p in s[0]] for s in sts], args[2], args[3], args[4])
    with pytest.raises(ValueError, match="elements"):
        ctx.ll_grad_diff_batch(args[0], args[1][:1], args[2][:1], args[3][:1], [1])
    with pytest.raises(ValueError):
        ctx.ll_grad_diff_batch([3, 0, 0], *args[1:])
    with pytest.raises(ValueError):
        ctx.ll_grad_diff_batch(args[0], args[1], args[2], np.zeros((2, 3)), args[4])      # a zero step
    assert np.array_equal(ctx.ll_grad_diff_batch(*args)[0], out)
    # the end of the batch's residency
    ctx.release_batch_scratch()
    with pytest.raises(g._lib.GPTBackendError, match="no batch resident"):
        ctx.ll_grad_diff_batch(*args)
    resident(g, ctx, ps, [y, y], X, n)
    assert np.array_equal(ctx.ll_grad_diff_batch(*args)[0], out)
    ctx.set_data(X, n)
    with pytest.raises(g._lib.GPTBackendError, match="no batch resident"):
        ctx.ll_grad_diff_batch(*args)
    # a batch fitted with warps
    layers = [(g._lib.WARP_LINEAR, np.array([0.0, 1.5, 0.0, 1.5]))]
    ctx.set_warp_batch([layers, layers])
    resident(g, ctx, ps, [y, y], X, n)
    with pytest.raises(NotImplementedError, match="warps"):
        ctx.ll_grad_diff_batch(*args)
    # a linear transform
    T = np.random.RandomState(3).rand(50, len(y)) / len(y)
    ctx.set_T(T)
    ctx.fit_batch_terms([[(g._lib.KERNEL_M52, np.array(p))] for p in ps], np.full(2, 0.01), np.array([T.dot(y)] * 2), np.full(50, 0.02),
                        DIAG_ADD)
    with pytest.raises(NotImplementedError, match="transform"):
        ctx.ll_grad_diff_batch(*args)
    ctx.set_T(None)
    resident(g, ctx, ps, [y, y], X, n)
    assert np.array_equal(ctx.ll_grad_diff_batch(*args)[0], out)


def test_a_stencil_point_the_fit_would_refuse_is_refused_before_any_launch(g):
    X, n, y = inputs(200, 2, nder=0)
    ctx = g._lib.Context(0)
    ctx.set_data(X, n)
    ps = [[1.0, 1.3, 0.35, 0.3], [0.9, 1.4, 0.4, 0.35]]       # general Matern: sigma_f, nu, l_1, l_2
    sts = [m52_stencil(p) for p in ps]
    _, info = resident(g, ctx, ps, [y, y], X, n, kid=g._lib.KERNEL_MATERN)
    assert np.all(info == 0)
    args = ([0, 0, 0, 0], [s[0] for s in sts], [s[1] for s in sts], [s[2] for s in sts], [1, 1])
    out = ctx.ll_grad_diff_batch(*args)[0]
    assert np.all(np.isfinite(out))
    for nu in (70.0, 0.0, np.nan):
        bad = [[p.copy() for p in s[1]] for s in sts]
        bad[1][3][1] = nu                                      # the LAST element's last entry, its upper stencil point
        with pytest.raises(ValueError, match="nu"):
            ctx.ll_grad_diff_batch(args[0], args[1], bad, args[3], args[4])
    # ... but not where the element is skipped: its stencil is not read
    assert np.array_equal(ctx.ll_grad_diff_batch(args[0], args[1], bad, args[3], [1, 0])[0][0], out[0])
    assert np.array_equal(ctx.ll_grad_diff_batch(*args)[0], out)


# ---- the optimiser ------------------------------------------------------------------------------------------------------------
def test_optimiser_in_lockstep_reaches_the_sequential_starts_optimum(g):
    """The Matern-5/2 problem of test_optimiser_with_the_device_gradient_reaches_the_default_routes_optimum (N = 300, SLSQP, ftol
    1e-6), four random starts drawn from the same seed, gradient="device" with batch_starts on and off: the same number of starts
    complete, best.fun agrees within ftol (absolute, as SLSQP applies it), and the GP ends at the lockstep run's best.x."""
    X, n, y = inputs(300, 2, nder=0)
    ftol = 1e-6
    res = {}
    for lockstep in (False, True):
        gp = g.GaussianProcess(g.Matern52Kernel(num_dim=2, initial_params=[1.0, 0.5, 0.5], param_bounds=[(1e-2, 10.0)] * 3),
                               noise_k=g.DiagonalNoiseKernel(num_dim=2, initial_noise=0.1, noise_bound=(1e-3, 5.0)), X=X, y=y, err_y=0.02, n=n)
        np.random.seed(1234)
        best, done = gp.optimize_hyperparameters(random_starts=4, opt_kwargs={"options": {"ftol": ftol}}, gradient="device",
                                                 batch_starts=lockstep)
        assert best.success, best
        res[lockstep] = (best, done, np.array(gp.free_params[:], dtype=float))
    print("sequential %.12g (%d starts), lockstep %.12g (%d starts)" % (res[False][0].fun, res[False][1], res[True][0].fun, res[True][1]))
    assert res[True][1] == res[False][1]
    assert abs(res[True][0].fun - res[False][0].fun) <= ftol
    assert np.array_equal(res[True][2], res[True][0].x)
