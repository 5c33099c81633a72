"""GPU suite (-m gpu): the device LML gradient by per-pair differencing -- gpt_ll_grad_diff (kgrad.hip) through
GaussianProcess.ll_gradient and optimize_hyperparameters(gradient="device") -- against
  (1) the exact gradient of squared-exponential models (gpt_ll_grad), within ten times the CPU oracle's own differencing error,
  (2) central differences of the device log-posterior for every kernel family, with the yardstick of
      test_device_ll_gradient_against_host_path_and_finite_differences: h = 1e-5 max(1, |theta|), rtol 2e-5, atol 1e-4 max|fd|,
  (3) sizes at the edges of the tile grid and of the inverse's two routes, repeat calls, and the optimiser."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

#: the CPU oracle's error of the per-pair differenced SE gradient at the inputs of the exact test below (oracle K at theta -+ eps,
#: LAPACK for alpha alpha^T - K_tot^-1, eps = 6e-6 max(1, |theta|)), relative to the largest kernel-parameter entry of the exact
#: gradient: 1.005e-7 for the single kernel and for the sum
ORACLE_DIFF_ERR = 1.005e-7


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


def inputs(N, d, nder=60, seed=31):
    """The inputs of the existing gradient test (seed 31, N = 700, d = 2, 60 derivative rows), at any size."""
    rs = np.random.RandomState(seed)
    X = rs.rand(N, d)
    n = np.zeros((N, d), dtype=int)
    if nder:
        n[-nder:, 0] = 1
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(N)
    return X, n, y


def noise(g, d, free=True):
    return g.DiagonalNoiseKernel(num_dim=d, initial_noise=0.1, noise_bound=(0.0, 5.0), fixed_noise=not free)


def fd_gradient(gp, theta):
    """Central differences of the device log-posterior, the existing test's rule."""
    fd = np.zeros_like(theta)
    for i in range(len(theta)):
        h = 1e-5 * max(1.0, abs(theta[i]))
        tp, tm = theta.copy(), theta.copy()
        tp[i] += h
        tm[i] -= h
        fd[i] = (-gp.update_hyperparameters(tp) + gp.update_hyperparameters(tm)) / (2 * h)
    return fd


def check_against_fd(make, label):
    gp = make()
    theta = np.array(gp.free_params[:], dtype=float)
    assert np.isfinite(gp.update_hyperparameters(theta))
    assert gp._fit_mode == "kernel"
    grad = gp.ll_gradient()
    assert np.array_equal(np.array(gp.free_params[:], dtype=float), theta) and gp.K_up_to_date
    fd = fd_gradient(make(), theta)
    err = np.abs(grad - fd)
    print("%s: p = %d, max|fd| = %.4g, max|grad - fd| / max|fd| = %.3g" % (label, len(theta), np.abs(fd).max(), err.max() / np.abs(fd).max()))
    np.testing.assert_allclose(grad, fd, rtol=2e-5, atol=1e-4 * np.abs(fd).max(), err_msg=label)
    return gp, grad


def test_se_against_the_exact_gradient(g):
    """SE and a sum of two, free noise, N = 700 with 60 derivative rows: ll_gradient against the analytic gpt_ll_grad route.  Bound
    on the kernel-parameter entries: ten times the CPU oracle's differencing error at these inputs and this step rule, measured as
    1.005e-7 of the largest exact kernel-parameter entry (the ten covers the device's other summation order; the device's own figure: 6.4e-9, single and sum); the noise entry comes
    from the same trace kernel arithmetic and must be the same bits."""
    X, n, y = inputs(700, 2)
    for build in ("single", "sum"):
        def make(deriv):
            k = g.SquaredExponentialKernel(num_dim=2, initial_params=[1.1, 0.4, 0.6], param_bounds=[(0.0, 1e3)] * 3)
            if build == "sum":
                k = k + g.SquaredExponentialKernel(num_dim=2, initial_params=[0.3, 1.5, 2.5], param_bounds=[(0.0, 1e3)] * 3)
            return g.GaussianProcess(k, noise_k=noise(g, 2), X=X, y=y, err_y=0.02, n=n, use_hyper_deriv=deriv)
        gp = make(True)
        theta = np.array(gp.free_params[:], dtype=float)
        _, negexact = gp.update_hyperparameters(theta)
        exact = -negexact
        got = make(False).ll_gradient()
        nk = len(theta) - 1
        scale = np.abs(exact[:nk]).max()
        err = np.abs(got[:nk] - exact[:nk]).max() / scale
        print("%s: max|grad_k| = %.6g, differenced - exact = %.3g of it (oracle: %.3g)" % (build, scale, err, ORACLE_DIFF_ERR))
        assert err <= 10 * ORACLE_DIFF_ERR, (build, err)
        assert got[nk] == exact[nk]


def test_m52_3d_with_derivative_rows_and_free_noise(g):
    X, n, y = inputs(700, 3)
    check_against_fd(lambda: g.GaussianProcess(
        g.Matern52Kernel(num_dim=3, initial_params=[1.1, 0.4, 0.6, 0.9], param_bounds=[(0.0, 1e3)] * 4), noise_k=noise(g, 3), X=X, y=y,
        err_y=0.02, n=n), "m52 d=3")


def test_rq_plus_se_sum(g):
    X, n, y = inputs(700, 2)
    check_against_fd(lambda: g.GaussianProcess(
        g.RationalQuadraticKernel(num_dim=2, initial_params=[1.0, 1.7, 0.4, 0.6], param_bounds=[(0.0, 1e3)] * 4) +
        g.SquaredExponentialKernel(num_dim=2, initial_params=[0.3, 1.5, 2.5], param_bounds=[(0.0, 1e3)] * 3), noise_k=noise(g, 2),
        X=X, y=y, err_y=0.02, n=n), "rq + se")


def test_general_matern_with_nu_free(g):
    X, n, y = inputs(300, 2, nder=0)
    check_against_fd(lambda: g.GaussianProcess(
        g.MaternKernel(num_dim=2, initial_params=[1.0, 1.3, 0.35, 0.3], param_bounds=[(0.0, 1e3)] * 4), noise_k=noise(g, 2), X=X, y=y,
        err_y=0.02, n=n), "matern, nu free")


def test_se_times_m52_product(g):
    X, n, y = inputs(700, 2)
    check_against_fd(lambda: g.GaussianProcess(
        g.SquaredExponentialKernel(num_dim=2, initial_params=[1.1, 0.8, 1.2], param_bounds=[(0.0, 1e3)] * 3) *
        g.Matern52Kernel(num_dim=2, initial_params=[0.9, 0.7, 0.9], param_bounds=[(0.0, 1e3)] * 3), noise_k=noise(g, 2), X=X, y=y,
        err_y=0.02, n=n), "se * m52")


def test_gibbs_exp_gauss_eleven_parameters_cross_the_launch_group(g):
    """11 free parameters of one term: two launches (8 + 3)."""
    X, n, y = inputs(300, 1, nder=30)
    p = [1.1, 0.35, 0.2, 0.5, 0.8, 0.15, 0.2, 0.1, 0.4, -0.5, 0.3]          # sigma_f, l_0, mu_1..3, sigma_1..3, beta_1..3
    gp, grad = check_against_fd(lambda: g.GaussianProcess(
        g.GibbsKernel1dExpGauss(3, initial_params=p, param_bounds=[(-10.0, 10.0)] * 11), noise_k=noise(g, 1, free=False), X=X, y=y,
        err_y=0.05, n=n), "gibbs exp-gauss")
    assert len(grad) == 11 and np.all(grad != 0.0)


def test_gibbs_nested_gp_four_points(g):
    X, n, y = inputs(300, 1, nder=30)
    m = 4
    p = [1.1, 0.5] + list(np.linspace(-0.1, 1.1, m)) + [0.3, 0.5, 0.25, 0.4]
    check_against_fd(lambda: g.GaussianProcess(
        g.GibbsKernel1dGP(m, initial_params=p, param_bounds=[(-10.0, 10.0)] * (2 * m + 2)), noise_k=noise(g, 1, free=False), X=X, y=y,
        err_y=0.05, n=n), "gibbs nested gp")


def test_masked_gibbs_tanh_times_se(g):
    X, n, y = inputs(500, 2)

    def make():
        gib = g.GibbsKernel1dTanh(initial_params=[1.2, 0.3, 0.8, 0.2, 0.5], param_bounds=[(1e-3, 10.0)] * 5)
        se = g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 0.6], fixed_params=[True, False], param_bounds=[(0.0, 10.0)] * 2)
        return g.GaussianProcess(g.MaskedKernel(gib, 2, [0]) * g.MaskedKernel(se, 2, [1]), noise_k=noise(g, 2), X=X, y=y, err_y=0.02, n=n)
    check_against_fd(make, "masked gibbs-tanh * se")


def test_linear_transform_260_latent_points_to_100_observations(g):
    """The pair pass over the latent points against T^T K_tot^-1 T.  The noise parameter is fixed: with a transform the noise entry
    is the reference's 2 sigma_n I over the OBSERVATIONS (as gpt_ll_grad and the host path return it), while the fit transforms
    the noise term with T -- that entry is no derivative of the fitted log-posterior and central differences cannot check it; it
    is compared with gpt_ll_grad's, bit for bit, on an SE model over the same points and transform."""
    rs = np.random.RandomState(12)
    Nx, Ny = 260, 100
    X = np.sort(rs.rand(Nx))[:, None]
    n = np.zeros((Nx, 1), dtype=int)
    n[-20:, 0] = 1
    T = rs.rand(Ny, Nx) / Nx
    y = T.dot(np.sin(5 * X[:, 0])) + 1e-3 * rs.randn(Ny)

    def make():
        gp = g.GaussianProcess(g.Matern52Kernel(num_dim=1, initial_params=[1.1, 0.35], param_bounds=[(0.0, 1e3)] * 2),
                               noise_k=g.DiagonalNoiseKernel(num_dim=1, initial_noise=0.02, noise_bound=(0.0, 1.0), fixed_noise=True))
        gp.add_data(X, y, err_y=1e-3, n=n, T=T)
        return gp
    gp, grad = check_against_fd(make, "m52 with T")
    # the noise trace of a transformed model: gpt_ll_grad's bits (an SE model over the same points and transform)
    se = g.GaussianProcess(g.SquaredExponentialKernel(num_dim=1, initial_params=[1.1, 0.35], param_bounds=[(0.0, 1e3)] * 2),
                           noise_k=g.DiagonalNoiseKernel(num_dim=1, initial_noise=0.02, noise_bound=(0.0, 1.0)))
    se.add_data(X, y, err_y=1e-3, n=n, T=T)
    se.update_hyperparameters(np.array(se.free_params[:], dtype=float))
    exact = se._ctx.ll_grad([0, 0], [0, 1])
    slot, tix, pa, pb, denom = se._ll_gradient_stencil(6e-6)
    got = se._ctx.ll_grad_diff(tix, pa, pb, denom)
    assert got[-1] == exact[-1]


def test_constant_mean_with_a_free_parameter(g):
    X, n, y = inputs(400, 2, nder=0)

    def make():
        return g.GaussianProcess(g.Matern52Kernel(num_dim=2, initial_params=[1.1, 0.4, 0.6], param_bounds=[(0.0, 1e3)] * 3),
                                 noise_k=noise(g, 2), mu=g.ConstantMeanFunction(initial_params=[0.3]), X=X, y=y + 0.5, err_y=0.02, n=n)
    gp, grad = check_against_fd(make, "m52 + constant mean")
    assert len(grad) == 5


@pytest.mark.parametrize("N", [33, 257, 1100])
def test_tile_and_inverse_edges(g, N):
    """N = 33: one ragged tile; 257: one column into the second 256-column tile; 1100: the GEMM-only inverse with a ragged last
    block."""
    X, n, y = inputs(N, 2, nder=min(60, N // 4))
    check_against_fd(lambda: g.GaussianProcess(
        g.Matern52Kernel(num_dim=2, initial_params=[1.1, 0.4, 0.6], param_bounds=[(0.0, 1e3)] * 3), noise_k=noise(g, 2), X=X, y=y,
        err_y=0.02, n=n), "m52 N=%d" % N)


def test_repeat_calls_and_the_analytic_gradient_are_bit_stable(g):
    """ll_gradient twice, and after a refit at the same point: the same bits.  gpt_ll_grad before and after a gpt_ll_grad_diff call:
    the same bits, and both calls' noise trace the same number."""
    X, n, y = inputs(700, 2)
    k = g.SquaredExponentialKernel(num_dim=2, initial_params=[1.1, 0.4, 0.6], param_bounds=[(0.0, 1e3)] * 3) + \
        g.Matern52Kernel(num_dim=2, initial_params=[0.5, 1.5, 2.5], fixed_params=[True, True, True], param_bounds=[(0.0, 1e3)] * 3)
    gp = g.GaussianProcess(k, noise_k=noise(g, 2), X=X, y=y, err_y=0.02, n=n)
    theta = np.array(gp.free_params[:], dtype=float)
    gp.update_hyperparameters(theta)
    ctx = gp._ctx
    before = ctx.ll_grad([0, 0, 0], [0, 1, 2])
    g1 = gp.ll_gradient()
    g2 = gp.ll_gradient()
    after = ctx.ll_grad([0, 0, 0], [0, 1, 2])
    assert np.array_equal(g1, g2)
    assert np.array_equal(before, after)
    slot, tix, pa, pb, denom = gp._ll_gradient_stencil(6e-6)
    raw = ctx.ll_grad_diff(tix, pa, pb, denom)
    assert raw[-1] == before[-1]
    assert np.array_equal(ctx.ll_grad_diff([], [], [], []), before[-1:])          # no parameters: the trace alone
    gp.update_hyperparameters(theta + 0.01)
    gp.update_hyperparameters(theta)
    assert np.array_equal(gp.ll_gradient(), g1)
    # a zero step, a term the model does not have, a vector that is not as long as its term's parameters: refused
    with pytest.raises(ValueError):
        ctx.ll_grad_diff(tix, pa, pb, np.zeros(len(denom)))
    with pytest.raises(ValueError):
        ctx.ll_grad_diff([5], pa[:1], pb[:1], denom[:1])
    with pytest.raises(ValueError, match="parameters"):
        ctx.ll_grad_diff(tix, [p[:-1] for p in pa], [p[:-1] for p in pb], denom)
    with pytest.raises(ValueError, match="parameters"):
        ctx.ll_grad_diff(tix, pa, [np.concatenate((p, [1.0])) for p in pb], denom)
    assert np.array_equal(gp.ll_gradient(), g1)


def test_a_stencil_point_the_fit_would_refuse_is_refused_before_any_launch(g):
    """SE + general Matern: a stencil point with the Matern order nu outside (0, 60) -- make_kparams' own refusal of a fit, a
    ValueError that names nu -- and one with a non-positive step; afterwards gpt_ll_grad and ll_gradient return the bits they
    returned before (nothing was launched, the resident factorisation and its weights are untouched)."""
    X, n, y = inputs(300, 2, nder=0)
    k = g.SquaredExponentialKernel(num_dim=2, initial_params=[0.6, 0.8, 1.1], param_bounds=[(0.0, 1e3)] * 3) + \
        g.MaternKernel(num_dim=2, initial_params=[1.0, 1.3, 0.35, 0.3], param_bounds=[(0.0, 1e3)] * 4)
    gp = g.GaussianProcess(k, noise_k=noise(g, 2), X=X, y=y, err_y=0.02, n=n)
    theta = np.array(gp.free_params[:], dtype=float)
    gp.update_hyperparameters(theta)
    ctx = gp._ctx
    exact = ctx.ll_grad([0, 0, 0], [0, 1, 2])
    g1 = gp.ll_gradient()
    slot, tix, pa, pb, denom = gp._ll_gradient_stencil(6e-6)
    assert tix == [0, 0, 0, 1, 1, 1, 1]
    for nu in (70.0, 0.0, -1.0, np.nan):
        bad = [p.copy() for p in pb]
        bad[4][1] = nu                                         # entry 4: the Matern term's nu, its upper stencil point
        with pytest.raises(ValueError, match="nu"):
            ctx.ll_grad_diff(tix, pa, bad, denom)
        bad = [p.copy() for p in pa]
        bad[6][1] = nu                                         # ... and as the LAST entry's lower point, whichever parameter it differences
        with pytest.raises(ValueError, match="nu"):
            ctx.ll_grad_diff(tix, bad, pb, denom)
    assert np.array_equal(ctx.ll_grad([0, 0, 0], [0, 1, 2]), exact)
    assert np.array_equal(gp.ll_gradient(), g1)


def test_a_bad_stencil_is_refused_alike_by_the_four_differenced_gradients():
    """The same bad stencil to gpt_ll_grad_diff, gpt_loo_grad_diff, gpt_ll_grad_diff_batch (a batch of one) and gpt_sparse_grad_diff,
    each called on the library itself (the wrappers of _lib.Context refuse some of these before the library sees them): a term the
    model does not have, a step of 0, a step of inf, and a stencil point the fit refuses.  N = 40, M = 5; SE + general Matern, because
    no parameter value of a squared-exponential term is refused by the fit: the Matern term's nu = 70 is, as in the test above.
    The status is the same from all four.  Where the library names the caller -- the two bad steps -- each message starts with its own
    entry point's name; the fit's refusal of nu is the fit's own text, the same from all four; a term out of range sets no text."""
    import ctypes as C
    from gptools_amd import _lib
    lib = _lib.load()
    N, M, d = 40, 5, 2
    X, n, y = inputs(N, d, nder=0)
    err_y = np.full(N, 0.02)
    Z = np.random.RandomState(5).rand(M, d)
    p_se, p_mat = [1.1, 0.4, 0.6], [1.0, 1.3, 0.35, 0.3]
    ids, terms = [_lib.KERNEL_SE, _lib.KERNEL_MATERN], [(_lib.KERNEL_SE, p_se), (_lib.KERNEL_MATERN, p_mat)]
    dense, batch = _lib.Context(), _lib.Context()
    dense.set_data(X, n)
    dense.fit_sum(ids, [p_se, p_mat], 0.01, y, err_y, 1e-12)
    dense.sparse_set_inducing(Z)
    dense.sparse_fit(_lib.SPARSE_METHODS["fitc"], terms, 0.01, y, err_y, 1e-8)
    batch.set_data(X, n)
    _, _, info = batch.fit_batch_sum(ids, [p_se + p_mat], [3, 4], [0.01], [y], err_y, 1e-12)
    assert info[0] == 0
    keep = _lib.i32([1])
    ll = C.c_double()
    v = [np.empty(N) for _ in range(3)]

    def calls(ti, pa, pb, dn):
        ti, pa, pb, dn = _lib.i32(ti), _lib.f64(pa), _lib.f64(pb), _lib.f64(dn)
        nh, out = len(ti), np.empty(len(ti) + 1)
        head = (nh, _lib.iptr(ti), _lib.dptr(pa), _lib.dptr(pb), _lib.dptr(dn))
        return [("gpt_ll_grad_diff", lambda: lib.gpt_ll_grad_diff(dense.handle, *head, _lib.dptr(out))),
                ("gpt_loo_grad_diff", lambda: lib.gpt_loo_grad_diff(dense.handle, *head, _lib.dptr(out), C.byref(ll), _lib.dptr(v[0]),
                                                                   _lib.dptr(v[1]), _lib.dptr(v[2]))),
                ("gpt_ll_grad_diff_batch", lambda: lib.gpt_ll_grad_diff_batch(batch.handle, *head, _lib.iptr(keep), _lib.dptr(out), None)),
                ("gpt_sparse_grad_diff", lambda: lib.gpt_sparse_grad_diff(dense.handle, *head, _lib.dptr(y), _lib.dptr(err_y),
                                                                         _lib.dptr(out), None))]

    def answers(ti, pa, pb, dn):
        got = []
        for name, call in calls(ti, pa, pb, dn):
            rc = call()
            got.append((name, rc, _lib.last_error()))
            print("%s: status %d, %r" % got[-1])
        return got

    a, b = [1.1, 0.4, 0.6 - 1e-5], [1.1, 0.4, 0.6 + 1e-5]
    # a good stencil first: every entry point answers GPT_OK (the bad ones below differ from it in one place each)
    assert [rc for _, rc, _ in answers([0], a, b, [2e-5])] == [_lib.GPT_OK] * 4
    # a term the model does not have
    assert [rc for _, rc, _ in answers([2], a, b, [2e-5])] == [_lib.GPT_E_ARG] * 4
    assert [rc for _, rc, _ in answers([-1], a, b, [2e-5])] == [_lib.GPT_E_ARG] * 4
    # a step of 0, a step of inf
    for step in (0.0, np.inf):
        got = answers([0], a, b, [step])
        assert [rc for _, rc, _ in got] == [_lib.GPT_E_ARG] * 4
        for name, _, msg in got:
            assert msg.startswith(name + ": denom["), (name, msg)
    # a stencil point the fit refuses: the Matern term's nu
    a, b = [1.0, 70.0, 0.35, 0.3], [1.0, 1.3, 0.35, 0.3]
    got = answers([1], a, b, [-68.7])
    assert [rc for _, rc, _ in got] == [got[0][1]] * 4 and got[0][1] in (_lib.GPT_E_ARG, _lib.GPT_E_VALUE)
    assert len({msg for _, _, msg in got}) == 1 and "nu" in got[0][2]
    # ... and the good stencil still goes through
    assert [rc for _, rc, _ in answers([0], [1.1, 0.4, 0.6 - 1e-5], [1.1, 0.4, 0.6 + 1e-5], [2e-5])] == [_lib.GPT_OK] * 4


def test_optimiser_with_the_device_gradient_reaches_the_default_routes_optimum(g):
    """Matern-5/2, N = 300, SLSQP from the same start: the log-posteriors of gradient="device" and of the default route (finite
    differences of the objective) agree within the optimiser's ftol, SLSQP's own 1e-6, absolute as SLSQP applies it.

    The default route is given a forward-difference step that suits the objective, `eps` = 1e-6 in the optimiser's options (it
    means nothing to the device route).  scipy's own step, 1.5e-8 = sqrt(machine epsilon), is the one for an objective known to
    machine precision; the device log-posterior carries a rounding of some 1e-10 (central differences at h = 1e-5 reproduce its
    gradient to 1e-8 of 2e3), so at 1.5e-8 the gradients are noisy at 1e-2 and that noise, not ftol, decides where the route
    stops: -403.4583168 against the device route's -403.4583436, 2.7e-5 apart, and still -403.4583193 with ftol = 1e-12.  At 1e-6
    the noise is 1e-4 and the truncation (eps f'' / 2) of the same order.  Measured with it: default -403.458343569, device
    -403.458343555 (25 evaluations each), 1.4e-8 apart; the optimum itself (device route, ftol = 1e-12): -403.458343836."""
    X, n, y = inputs(300, 2, nder=0)
    ftol = 1e-6
    res = {}
    for gradient in (None, "device"):
        gp = g.GaussianProcess(g.Matern52Kernel(num_dim=2, initial_params=[1.0, 0.5, 0.5], param_bounds=[(1e-2, 10.0)] * 3),
                               noise_k=g.DiagonalNoiseKernel(num_dim=2, initial_noise=0.1, noise_bound=(1e-3, 5.0)), X=X, y=y, err_y=0.02, n=n)
        best, _ = gp.optimize_hyperparameters(random_starts=0, opt_kwargs={"options": {"ftol": ftol, "eps": 1e-6}}, gradient=gradient)
        assert best.success, best
        res[gradient] = best
    print("default %.12g (%d evaluations), device %.12g (%d evaluations, %d gradients)"
          % (res[None].fun, res[None].nfev, res["device"].fun, res["device"].nfev, res["device"].njev))
    assert res["device"].fun <= res[None].fun + ftol
    assert abs(res[None].fun - res["device"].fun) <= ftol
