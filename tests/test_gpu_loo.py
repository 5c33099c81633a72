"""GPU suite (-m gpu): leave-one-out cross-validation on the device -- gpt_loo and gpt_loo_grad_diff (kloo.hip, kgrad.hip) through
GaussianProcess.loo_predict, loo_log_likelihood, loo_gradient, optimize_hyperparameters(objective="loo") and remove_outliers.

Every yardstick is the host's: K_tot = K + noise_K + diag(err_y^2) + diag_factor eps I with K from compute_Kij (the K-builder, not
the fit) and LAPACK for the rest -- the device LOO is never compared with another output of the code under test, except where a
test is about bits.  The bounds on the values are ten times the host's own discrepancy between two routes to the same number,
measured on the CPU at these inputs (the named constants below; the ten covers the device's other summation order); the gradient
is held to the yardstick of tests/test_gpu_grad_diff.py."""
import sys
import warnings

import numpy as np
import pytest
import scipy.linalg

pytestmark = pytest.mark.gpu

#: brute force (N refits, cho_solve) against the closed form (inv) on the host, SE d = 2, N = 40 with 8 derivative rows, the inputs of
#: test_brute_force (K from the CPU oracle): largest difference of the means relative to max|y|, of the standard deviations relative
#: to their largest, of L_LOO relative to |L_LOO| -- the largest of the three
#: measured: 1.94e-13
HOST_BRUTE_ERR = 1.94e-13
#: closed form by inv(K_tot) against closed form by cho_solve on the identity, same three figures, the largest over N = 33, 127, 128,
#: 257 and 1100 (SE d = 2, K from the CPU oracle)
#: measured: 1.6e-13, 5.4e-13, 1.6e-12, 1.9e-12 and 8.48e-12 (cond K_tot = 3.2e3 ... 7.5e4)
HOST_CLOSED_ERR = 8.48e-12
#: the same at the warped model's inputs (N = 257) 1.4e-12 and at the Python-defined kernel's (N = 128) 6.8e-14: inside HOST_CLOSED_ERR,
#: which bounds them too; at the transformed model's inputs (100 observations of 260 latent points, cond K_tot = 1.4e7): 1.04e-10
HOST_T_ERR = 1.04e-10
#: the host formula of the gradient, sum_ab G_ab dK_ab, SE sum at N = 257, K from the CPU oracle and LAPACK for G -- the convention of
#: ORACLE_DIFF_ERR in tests/test_gpu_grad_diff.py: with dK the per-pair central difference (eps = 6e-6 max(1, |theta|)) against the
#: same formula with the analytic dK, the largest difference over the kernel-parameter entries relative to the largest of them
#: (587.1): 3.18e-7.  It is the rounding of K at the two stencil points over the step, which every differenced dK carries.  (G from
#: inv against G from cho_solve with the SAME dK moves those entries by 2.9e-12 only: a first version of this file took that for the
#: host's figure, which leaves out the very error the compared quantity has -- white noise of one ulp on the host's K at the
#: stencil points moves the host formula by 2e-6 ... 9e-6 absolute, 1e-8 of 587.)
HOST_GRAD_DIFF_ERR = 3.18e-7
#: the noise entry has no dK: G from inv against G from cho_solve, relative to the entry (4.98e4): 4.3e-13
HOST_GRAD_NOISE_ERR = 4.3e-13


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


def inputs(N, d, nder=60, seed=31):
    """The inputs of tests/test_gpu_grad_diff.py: seeded, any size."""
    rs = np.random.RandomState(seed)
    X = rs.rand(N, d)
    n = np.zeros((N, d), dtype=int)
    if nder:
        n[-nder:, 0] = 1
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(N)
    return X, n, y


def noise(g, d, free=True):
    return g.DiagonalNoiseKernel(num_dim=d, initial_noise=0.1, noise_bound=(0.0, 5.0), fixed_noise=not free)


# ---- the host's formulas (numpy / LAPACK only) -------------------------------------------------------------------------------
def k_tot(K, noise_var, err_y, diag_factor=1e2, T=None):
    KnK = K + noise_var * np.eye(K.shape[0])
    if T is not None:
        KnK = T.dot(KnK).dot(T.T)
    return KnK + np.diag(err_y ** 2.0) + diag_factor * sys.float_info.epsilon * np.eye(KnK.shape[0])


def inverse(Kt, route):
    if route == "inv":
        return np.linalg.inv(Kt)
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(Kt, lower=True), np.eye(Kt.shape[0]))


def loo_closed(Kt, res, route="inv"):
    """(r, s, L_LOO) in closed form: the LOO residuals r = y - m, the standard deviations and the value."""
    W = inverse(Kt, route)
    alpha, d = W.dot(res), np.diag(W).copy()
    r = alpha / d
    return r, np.sqrt(1.0 / d), np.sum(0.5 * np.log(d) - 0.5 * alpha ** 2 / d - 0.5 * np.log(2 * np.pi))


def loo_brute(Kt, res):
    """The same by N refits, each with one row and column removed."""
    N = Kt.shape[0]
    r, s = np.empty(N), np.empty(N)
    for i in range(N):
        keep = np.arange(N) != i
        cf = scipy.linalg.cho_factor(Kt[np.ix_(keep, keep)], lower=True)
        kv = Kt[keep, i]
        r[i] = res[i] - kv.dot(scipy.linalg.cho_solve(cf, res[keep]))
        s[i] = np.sqrt(Kt[i, i] - kv.dot(scipy.linalg.cho_solve(cf, kv)))
    return r, s, np.sum(-0.5 * np.log(2 * np.pi * s ** 2) - 0.5 * (r / s) ** 2)


def loo_gradient_weights(Kt, res, route="inv"):
    """alpha, u and G = 1/2 (u alpha^T + alpha u^T) - 1/2 V of the gradient, d L_LOO / d theta = sum_ab G_ab dK_ab."""
    W = inverse(Kt, route)
    alpha, d = W.dot(res), np.diag(W).copy()
    r, e = alpha / d, (1.0 + alpha ** 2 / d) / d
    u = W.dot(r)
    V = (W * e).dot(W)
    return alpha, u, 0.5 * (np.outer(u, alpha) + np.outer(alpha, u)) - 0.5 * V


def three_figures(got, ref, y):
    """(means relative to max|y|, standard deviations relative to their largest, value relative to its size); got / ref = (r, s, L)."""
    return max(np.abs(got[0] - ref[0]).max() / np.abs(y).max(), np.abs(got[1] - ref[1]).max() / ref[1].max(),
               abs(got[2] - ref[2]) / abs(ref[2]))


def host_of(gp):
    """K_tot and y - T mu of a GP at its current hyperparameters: K from the K-builder."""
    K = gp.compute_Kij(gp.X, None, gp.n, None)
    res = gp.y.copy()
    if gp.mu is not None:
        m = gp.mu(gp.X, gp.n)
        res = res - (gp.T.dot(m) if gp.T is not None else m)
    return k_tot(K, gp.noise_k.params[0] ** 2.0, gp.err_y, gp.diag_factor, gp.T), res


def device_loo(gp):
    m, s = gp.loo_predict()
    assert m.shape == s.shape == gp.y.shape
    return gp.y - m, s, gp.loo_log_likelihood()


def se2(g, **kw):
    return g.SquaredExponentialKernel(num_dim=2, initial_params=[1.1, 0.4, 0.6], param_bounds=[(0.0, 1e3)] * 3, **kw)


# ---- value -------------------------------------------------------------------------------------------------------------------
def test_brute_force(g):
    """SE, d = 2, N = 40 with 8 derivative rows: loo_predict and loo_log_likelihood against 40 host refits.
    Measured: host closed form - brute force HOST_BRUTE_ERR; the device's figure is printed."""
    X, n, y = inputs(40, 2, nder=8)
    gp = g.GaussianProcess(se2(g), noise_k=noise(g, 2), X=X, y=y, err_y=0.02, n=n)
    Kt, res = host_of(gp)
    err = three_figures(device_loo(gp), loo_brute(Kt, res), y)
    print("brute force N = 40: device - host = %.3g (host's own %.3g)" % (err, HOST_BRUTE_ERR))
    assert err <= 10 * HOST_BRUTE_ERR


@pytest.mark.parametrize("N", [33, 127, 128, 257, 1100])
def test_closed_form_at_the_edges_of_the_tiles_and_of_the_inverse(g, N):
    """33: one ragged tile; 127: the augmented row last in the only leaf; 128: it opens a second leaf; 257: one column into the second
    tile; 1100: the GEMM-only inverse with a ragged last block."""
    X, n, y = inputs(N, 2, nder=min(60, N // 4))
    gp = g.GaussianProcess(se2(g), noise_k=noise(g, 2), X=X, y=y, err_y=0.02, n=n)
    Kt, res = host_of(gp)
    err = three_figures(device_loo(gp), loo_closed(Kt, res), y)
    print("closed form N = %d: device - host = %.3g (host's own %.3g)" % (N, err, HOST_CLOSED_ERR))
    assert gp._fit_mode == "kernel"
    assert err <= 10 * HOST_CLOSED_ERR


def _warped(g):
    X, n, y = inputs(257, 2, nder=60)
    return g.GaussianProcess(g.LinearWarpedKernel(se2(g), [-0.5, -0.25], [1.5, 2.0]), noise_k=noise(g, 2), X=X, y=y, err_y=0.02, n=n), "kernel"


def _python_kernel(g):
    class Mine(g.SquaredExponentialKernel):                    # a Python-defined __call__: K_tot is assembled on the host
        def __call__(self, Xi, Xj, ni, nj, hyper_deriv=None, symmetric=False):
            r2 = (((Xi - Xj) / self.params[1:]) ** 2).sum(1)
            return self.params[0] ** 2 * np.exp(-0.5 * r2)
    X, n, y = inputs(128, 2, nder=0)
    k = Mine(num_dim=2, initial_params=[1.1, 0.4, 0.6], param_bounds=[(0.0, 1e3)] * 3)
    return g.GaussianProcess(k, noise_k=noise(g, 2), X=X, y=y, err_y=0.02, n=n), "matrix"


def _transform(g):
    rs = np.random.RandomState(12)
    Nx, Ny = 260, 100
    X = np.sort(rs.rand(Nx))[:, None]
    n = np.zeros((Nx, 1), dtype=int)
    n[-20:, 0] = 1
    T = rs.rand(Ny, Nx) / Nx
    y = T.dot(np.sin(5 * X[:, 0])) + 1e-3 * rs.randn(Ny)
    gp = g.GaussianProcess(g.Matern52Kernel(num_dim=1, initial_params=[1.1, 0.35], param_bounds=[(0.0, 1e3)] * 2),
                           noise_k=g.DiagonalNoiseKernel(num_dim=1, initial_noise=0.02, noise_bound=(0.0, 1.0), fixed_noise=True))
    gp.add_data(X, y, err_y=1e-3, n=n, T=T)
    return gp, None


_transform.bound = HOST_T_ERR


@pytest.mark.parametrize("make", [_warped, _python_kernel, _transform])
def test_closed_form_on_the_other_fit_routes(g, make):
    """A warped model at N = 257, a Python-defined kernel on the matrix route at N = 128, 260 latent points transformed to 100
    observations: gpt_loo needs a resident factor and nothing else."""
    gp, mode = make(g)
    Kt, res = host_of(gp)
    assert Kt.shape[0] == len(gp.y)
    err = three_figures(device_loo(gp), loo_closed(Kt, res), gp.y)
    bound = getattr(make, "bound", HOST_CLOSED_ERR)
    print("%s: device - host = %.3g (host's own %.3g)" % (make.__name__, err, bound))
    assert mode is None or gp._fit_mode == mode
    assert err <= 10 * bound


# ---- gradient ----------------------------------------------------------------------------------------------------------------
def loo_objective(gp, theta):
    assert np.isfinite(gp.update_hyperparameters(theta))
    return gp.loo_log_likelihood() + gp.hyperprior(gp.params)


def fd_gradient(gp, theta):
    """Central differences of the device L_LOO + log prior, the rule of tests/test_gpu_grad_diff.py."""
    fd = np.zeros_like(theta)
    for i in range(len(theta)):
        h = 1e-5 * max(1.0, abs(theta[i]))
        tp, tm = theta.copy(), theta.copy()
        tp[i] += h
        tm[i] -= h
        fd[i] = (loo_objective(gp, tp) - loo_objective(gp, tm)) / (2 * h)
    return fd


def check_against_fd(make, label):
    gp = make()
    theta = np.array(gp.free_params[:], dtype=float)
    assert np.isfinite(gp.update_hyperparameters(theta))
    grad = gp.loo_gradient()
    assert gp._fit_mode == "kernel"
    assert np.array_equal(np.array(gp.free_params[:], dtype=float), theta) and gp.K_up_to_date
    fd = fd_gradient(make(), theta)
    err = np.abs(grad - fd)
    print("%s: p = %d, max|fd| = %.4g, max|grad - fd| / max|fd| = %.3g" % (label, len(theta), np.abs(fd).max(), err.max() / np.abs(fd).max()))
    np.testing.assert_allclose(grad, fd, rtol=2e-5, atol=1e-4 * np.abs(fd).max(), err_msg=label)
    return gp, grad


def test_gradient_m52_3d_with_derivative_rows(g):
    X, n, y = inputs(700, 3)
    check_against_fd(lambda: g.GaussianProcess(
        g.Matern52Kernel(num_dim=3, initial_params=[1.1, 0.4, 0.6, 0.9], param_bounds=[(0.0, 1e3)] * 4), noise_k=noise(g, 3), X=X, y=y,
        err_y=0.02, n=n), "m52 d=3")


def test_gradient_rq_plus_se(g):
    X, n, y = inputs(700, 2)
    check_against_fd(lambda: g.GaussianProcess(
        g.RationalQuadraticKernel(num_dim=2, initial_params=[1.0, 1.7, 0.4, 0.6], param_bounds=[(0.0, 1e3)] * 4) +
        g.SquaredExponentialKernel(num_dim=2, initial_params=[0.3, 1.5, 2.5], param_bounds=[(0.0, 1e3)] * 3), noise_k=noise(g, 2),
        X=X, y=y, err_y=0.02, n=n), "rq + se")


def test_gradient_se_times_m52(g):
    X, n, y = inputs(700, 2)
    check_against_fd(lambda: g.GaussianProcess(
        g.SquaredExponentialKernel(num_dim=2, initial_params=[1.1, 0.8, 1.2], param_bounds=[(0.0, 1e3)] * 3) *
        g.Matern52Kernel(num_dim=2, initial_params=[0.9, 0.7, 0.9], param_bounds=[(0.0, 1e3)] * 3), noise_k=noise(g, 2), X=X, y=y,
        err_y=0.02, n=n), "se * m52")


def test_gradient_gibbs_exp_gauss_eleven_parameters_take_two_launch_groups(g):
    X, n, y = inputs(300, 1, nder=30)
    p = [1.1, 0.35, 0.2, 0.5, 0.8, 0.15, 0.2, 0.1, 0.4, -0.5, 0.3]
    gp, grad = check_against_fd(lambda: g.GaussianProcess(
        g.GibbsKernel1dExpGauss(3, initial_params=p, param_bounds=[(-10.0, 10.0)] * 11), noise_k=noise(g, 1, free=False), X=X, y=y,
        err_y=0.05, n=n), "gibbs exp-gauss")
    assert len(grad) == 11 and np.all(grad != 0.0)


def test_gradient_constant_mean_with_a_free_parameter(g):
    X, n, y = inputs(400, 2, nder=0)
    gp, grad = check_against_fd(lambda: g.GaussianProcess(
        g.Matern52Kernel(num_dim=2, initial_params=[1.1, 0.4, 0.6], param_bounds=[(0.0, 1e3)] * 3), noise_k=noise(g, 2),
        mu=g.ConstantMeanFunction(initial_params=[0.3]), X=X, y=y + 0.5, err_y=0.02, n=n), "m52 + constant mean")
    assert len(grad) == 5


def test_gradient_masked_gibbs_tanh_times_se(g):
    X, n, y = inputs(500, 2)

    def make():
        gib = g.GibbsKernel1dTanh(initial_params=[1.2, 0.3, 0.8, 0.2, 0.5], param_bounds=[(1e-3, 10.0)] * 5)
        se = g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 0.6], fixed_params=[True, False], param_bounds=[(0.0, 10.0)] * 2)
        return g.GaussianProcess(g.MaskedKernel(gib, 2, [0]) * g.MaskedKernel(se, 2, [1]), noise_k=noise(g, 2), X=X, y=y, err_y=0.02, n=n)
    check_against_fd(make, "masked gibbs-tanh * se")


@pytest.mark.parametrize("N", [33, 257, 1100])
def test_gradient_at_the_tile_and_inverse_edges(g, N):
    X, n, y = inputs(N, 2, nder=min(60, N // 4))
    check_against_fd(lambda: g.GaussianProcess(
        g.Matern52Kernel(num_dim=2, initial_params=[1.1, 0.4, 0.6], param_bounds=[(0.0, 1e3)] * 3), noise_k=noise(g, 2), X=X, y=y,
        err_y=0.02, n=n), "m52 N=%d" % N)


def se_sum(g):
    return se2(g) + g.SquaredExponentialKernel(num_dim=2, initial_params=[0.3, 1.5, 2.5], param_bounds=[(0.0, 1e3)] * 3)


def host_gradient(Kt, res, dKs, sigma_n, route="inv"):
    """The host formula: sum_ab G_ab dK_ab per kernel parameter, then the noise entry 2 sigma_n tr G."""
    _, _, G = loo_gradient_weights(Kt, res, route)
    return np.array([np.sum(G * dK) for dK in dKs] + [2.0 * sigma_n * np.trace(G)])


def test_gradient_against_the_host_formula(g):
    """SE sum, N = 257: G = 1/2 (u alpha^T + alpha u^T) - 1/2 V by LAPACK, dK the per-pair central difference of compute_Kij at the
    stencil points of loo_gradient.  Kernel-parameter entries within ten times the host's own differencing error, the noise entry
    (no dK in it) within ten times the difference of the host's two routes to G; the device's figures are printed (measured: 7.9e-9
    and 2.0e-13)."""
    X, n, y = inputs(257, 2)
    gp = g.GaussianProcess(se_sum(g), noise_k=noise(g, 2), X=X, y=y, err_y=0.02, n=n)
    theta = np.array(gp.free_params[:], dtype=float)
    got = gp.loo_gradient()
    Kt, res = host_of(gp)
    dKs = []
    for i in range(len(theta) - 1):
        eps = 6e-6 * max(1.0, abs(theta[i]))
        ta, tb = theta.copy(), theta.copy()
        ta[i], tb[i] = theta[i] - eps, theta[i] + eps
        gp._assign_free(ta)
        Ka = gp.compute_Kij(gp.X, None, gp.n, None)
        gp._assign_free(tb)
        Kb = gp.compute_Kij(gp.X, None, gp.n, None)
        dKs.append((Kb - Ka) / (tb[i] - ta[i]))
    gp._assign_free(theta)
    ref = host_gradient(Kt, res, dKs, theta[-1])
    nk = len(theta) - 1
    err = np.abs(got[:nk] - ref[:nk]).max() / np.abs(ref[:nk]).max()
    err_noise = abs(got[nk] - ref[nk]) / abs(ref[nk])
    print("host formula N = 257: device - host = %.3g of max|grad_k| = %.4g (host's own %.3g); noise entry %.3g of itself (host's own %.3g)"
          % (err, np.abs(ref[:nk]).max(), HOST_GRAD_DIFF_ERR, err_noise, HOST_GRAD_NOISE_ERR))
    assert err <= 10 * HOST_GRAD_DIFF_ERR
    assert err_noise <= 10 * HOST_GRAD_NOISE_ERR


# ---- bits --------------------------------------------------------------------------------------------------------------------
def test_repeat_calls_are_bit_stable_and_leave_the_lml_gradient_alone(g):
    X, n, y = inputs(700, 2)
    k = se2(g) + g.Matern52Kernel(num_dim=2, initial_params=[0.5, 1.5, 2.5], fixed_params=[True, True, True], param_bounds=[(0.0, 1e3)] * 3)
    gp = g.GaussianProcess(k, noise_k=noise(g, 2), X=X, y=y, err_y=0.02, n=n)
    theta = np.array(gp.free_params[:], dtype=float)
    gp.update_hyperparameters(theta)
    ctx = gp._ctx
    ll_before, raw_before = gp.ll_gradient(), ctx.ll_grad([0, 0, 0], [0, 1, 2])
    m0, s0 = gp.loo_predict()
    v0 = gp.loo_log_likelihood()
    g1 = gp.loo_gradient()
    g2 = gp.loo_gradient()
    assert np.array_equal(g1, g2)
    assert np.array_equal(gp.ll_gradient(), ll_before) and np.array_equal(ctx.ll_grad([0, 0, 0], [0, 1, 2]), raw_before)
    m1, s1 = gp.loo_predict()
    assert np.array_equal(m0, m1) and np.array_equal(s0, s1) and gp.loo_log_likelihood() == v0
    ll1, r1, var1 = ctx.loo(len(y))                              # gpt_loo itself, behind the gradient: the same bits
    assert ll1 == v0 and np.array_equal(y - r1, m0) and np.array_equal(np.sqrt(var1), s0)
    gp.update_hyperparameters(theta + 0.01)
    gp.update_hyperparameters(theta)
    assert np.array_equal(gp.loo_gradient(), g1)
    assert gp.loo_log_likelihood() == v0


@pytest.mark.parametrize("N", [257, 1100])
def test_debug_poison(g, N):
    """Every scratch matrix filled with NaN first: value, residuals and gradient are finite and the bits of the unpoisoned run."""
    X, n, y = inputs(N, 2, nder=min(60, N // 4))
    out = {}
    for poison in (0, 1):
        gp = g.GaussianProcess(se_sum(g), noise_k=noise(g, 2), X=X, y=y, err_y=0.02, n=n)
        gp._ctx.set_option("debug_poison", poison)
        m, s = gp.loo_predict()
        out[poison] = (m, s, np.array([gp.loo_log_likelihood()]), gp.loo_gradient(), np.array(gp._ctx.loo(N)[1]))
        gp._ctx.set_option("debug_poison", 0)
    for a, b in zip(out[0], out[1]):
        assert np.all(np.isfinite(b)) and np.array_equal(a, b)


def test_a_stencil_point_the_fit_would_refuse_is_refused_before_any_launch(g):
    X, n, y = inputs(300, 2, nder=0)
    k = g.SquaredExponentialKernel(num_dim=2, initial_params=[0.6, 0.8, 1.1], param_bounds=[(0.0, 1e3)] * 3) + \
        g.MaternKernel(num_dim=2, initial_params=[1.0, 1.3, 0.35, 0.3], param_bounds=[(0.0, 1e3)] * 4)
    gp = g.GaussianProcess(k, noise_k=noise(g, 2), X=X, y=y, err_y=0.02, n=n)
    gp.update_hyperparameters(np.array(gp.free_params[:], dtype=float))
    ctx = gp._ctx
    g1 = gp.loo_gradient()
    slot, tix, pa, pb, denom = gp._ll_gradient_stencil(6e-6)
    for nu in (70.0, 0.0, np.nan):
        bad = [p.copy() for p in pb]
        bad[4][1] = nu
        with pytest.raises(ValueError, match="nu"):
            ctx.loo_grad_diff(tix, pa, bad, denom, len(y))
    with pytest.raises(ValueError):
        ctx.loo_grad_diff(tix, pa, pb, np.zeros(len(denom)), len(y))
    assert np.array_equal(gp.loo_gradient(), g1)


# ---- optimiser and outliers --------------------------------------------------------------------------------------------------
def test_optimiser_on_the_leave_one_out_objective(g):
    """Matern-5/2, N = 300, SLSQP from the same start: gradient="device" and gradient=None (scipy differences the objective, with
    the step that suits a device objective, see tests/test_gpu_grad_diff.py) agree in -fun within SLSQP's ftol; objective="ll"
    is the call without the argument."""
    X, n, y = inputs(300, 2, nder=0)
    ftol = 1e-6

    def make():
        return g.GaussianProcess(g.Matern52Kernel(num_dim=2, initial_params=[1.0, 0.5, 0.5], param_bounds=[(1e-2, 10.0)] * 3),
                                 noise_k=g.DiagonalNoiseKernel(num_dim=2, initial_noise=0.1, noise_bound=(1e-3, 5.0)), X=X, y=y, err_y=0.02, n=n)
    kw = {"options": {"ftol": ftol, "eps": 1e-6}}
    res = {}
    for gradient in (None, "device"):
        gp = make()
        best, _ = gp.optimize_hyperparameters(random_starts=0, opt_kwargs=kw, gradient=gradient, objective="loo")
        assert best.success, best
        assert abs(gp.loo_log_likelihood() + gp.hyperprior(gp.params) + best.fun) <= 1e-9 * abs(best.fun)
        res[gradient] = best
    print("loo: default %.12g (%d evaluations), device %.12g (%d evaluations, %d gradients)"
          % (res[None].fun, res[None].nfev, res["device"].fun, res["device"].nfev, res["device"].njev))
    assert abs(res[None].fun - res["device"].fun) <= ftol
    a, _ = make().optimize_hyperparameters(random_starts=0, opt_kwargs=kw)
    b, _ = make().optimize_hyperparameters(random_starts=0, opt_kwargs=kw, objective="ll")
    assert a.fun == b.fun and np.array_equal(a.x, b.x) and a.nfev == b.nfev


def outlier_data(seed=11):
    """N = 200, d = 1, noise 0.05 known as err_y, five points moved by 8 sigma.  Seed 11: on the host (CPU oracle's K, LAPACK) both
    rules flag exactly the five -- smallest planted / largest other score 5.99 / 2.39 by the predict rule, 6.09 / 2.43 by LOO."""
    rs = np.random.RandomState(seed)
    X = np.sort(rs.rand(200))[:, None]
    y = np.sin(6 * X[:, 0]) + 0.05 * rs.randn(200)
    planted = np.array([17, 61, 99, 140, 183])
    y[planted] += 8 * 0.05 * np.array([1, -1, 1, -1, 1])
    return X, y, np.full(200, 0.05), planted


@pytest.mark.parametrize("method", ["predict", "loo"])
def test_remove_outliers(g, method):
    X, y, err_y, planted = outlier_data()
    gp = g.GaussianProcess(g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 0.3], param_bounds=[(0.0, 10.0)] * 2), X=X, y=y, err_y=err_y)
    by_hand = np.abs(gp.predict(X, n=0, noise=False, return_std=False) - y) / err_y >= 3
    out = gp.remove_outliers(thresh=3, method=method)
    assert len(out) == 5
    X_bad, y_bad, err_bad, n_bad, bad = out
    assert list(np.nonzero(bad)[0]) == list(planted)
    assert X_bad.shape == (5, 1) and y_bad.shape == (5,) and err_bad.shape == (5,) and n_bad.shape == (5, 1) and bad.shape == (200,)
    assert np.array_equal(y_bad, y[planted]) and np.array_equal(X_bad, X[planted])
    if method == "predict":
        assert np.array_equal(bad, by_hand)
    assert not gp.K_up_to_date and len(gp.y) == 195
    gp.compute_K_L_alpha_ll()
    assert gp._ctx.get_alpha(195).shape == (195,) and gp.loo_predict()[0].shape == (195,)
