"""CPU suite: gptools_amd.multistart.lockstep_minimize -- the starts of a multi-start optimisation served together -- against
sequential scipy.optimize.minimize runs, and the refusals of optimize_hyperparameters(batch_starts=True) and of
GaussianProcess.ll_gradient_batch, which are decided before any device is touched."""
import threading
import warnings

import numpy as np
import pytest
import scipy.optimize

from gptools_amd.multistart import lockstep_minimize

METHODS = ("SLSQP", "L-BFGS-B", "TNC")
BOUNDS = [(-2.0, 2.0), (-1.5, 2.5), (-2.0, 1.0), (-3.0, 3.0)]
A = np.array([1.0, 2.5, 0.7, 4.0])
C = np.array([0.3, -0.4, 0.9, 1.7])


def value_and_gradient(x):
    """A smooth function of 4 variables with several local minima inside BOUNDS, and its gradient."""
    x = np.asarray(x, dtype=float)
    r = x - C
    f = 0.5 * np.sum(A * r * r) + np.sum(np.sin(3.0 * x)) + 0.1 * np.prod(np.cos(x))
    cosx = np.cos(x)
    dprod = np.array([-np.sin(x[i]) * np.prod(np.delete(cosx, i)) for i in range(len(x))])
    return float(f), A * r + 3.0 * np.cos(3.0 * x) + 0.1 * dprod


def batch(points):
    vals = [value_and_gradient(p) for p in points]
    return [v[0] for v in vals], [v[1] for v in vals]


def starts(count=24, seed=5):
    rs = np.random.RandomState(seed)
    lo, hi = np.array(BOUNDS).T
    return [lo + (hi - lo) * rs.rand(4) for _ in range(count)]


def test_the_test_functions_gradient_is_its_gradient():
    for x in starts(3):
        assert scipy.optimize.check_grad(lambda z: value_and_gradient(z)[0], lambda z: value_and_gradient(z)[1], x) < 1e-5


@pytest.mark.parametrize("method", METHODS)
def test_lockstep_runs_are_the_sequential_runs_bit_for_bit(method):
    x0s = starts()
    seq = [scipy.optimize.minimize(value_and_gradient, x0, jac=True, method=method, bounds=BOUNDS) for x0 in x0s]
    before = threading.active_count()
    got, rounds = lockstep_minimize(x0s, batch, method=method, bounds=BOUNDS)
    assert threading.active_count() == before
    assert len(got) == len(seq)
    for a, b in zip(got, seq):
        assert a is not None
        assert np.array_equal(a.x, b.x) and a.fun == b.fun and a.nfev == b.nfev
    print("%s: %d rounds against %d sequential evaluations" % (method, rounds, sum(r.nfev for r in seq)))
    assert rounds == max(r.nfev for r in seq)
    assert len({r.nfev for r in seq}) > 1                     # (the starts do not all take equally long: lockstep is not trivial)


@pytest.mark.parametrize("method", METHODS)
def test_a_start_whose_function_raises_comes_back_none_and_the_others_are_unchanged(method):
    x0s = starts(6)
    seq = [scipy.optimize.minimize(value_and_gradient, x0, jac=True, method=method, bounds=BOUNDS) for x0 in x0s]
    victim, calls = 2, [0]
    first = x0s[victim].copy()

    def evaluate(points):
        f, g = batch(points)
        # the victim's points: round r holds its r-th call as long as it runs, in the order of the starts
        if calls[0] < 3 and len(points) == len(x0s):
            calls[0] += 1
            if calls[0] == 3:
                f[victim] = RuntimeError("this start's function raises on its third call")
        return f, g

    assert seq[victim].nfev >= 3 and np.array_equal(first, x0s[victim])
    before = threading.active_count()
    got, _ = lockstep_minimize(x0s, evaluate, method=method, bounds=BOUNDS)
    assert threading.active_count() == before
    assert got[victim] is None
    for i, (a, b) in enumerate(zip(got, seq)):
        if i != victim:
            assert np.array_equal(a.x, b.x) and a.fun == b.fun and a.nfev == b.nfev


def test_an_evaluator_that_raises_ends_every_thread_and_the_exception_leaves_the_driver():
    class Boom(Exception):
        pass
    rounds = [0]

    def evaluate(points):
        rounds[0] += 1
        if rounds[0] == 2:
            raise Boom("round 2")
        return batch(points)

    before = threading.active_count()
    with pytest.raises(Boom, match="round 2"):
        lockstep_minimize(starts(8), evaluate, method="SLSQP", bounds=BOUNDS)
    assert rounds[0] == 2
    assert threading.active_count() == before


def test_a_wrong_number_of_results_is_an_error_and_leaves_no_thread():
    before = threading.active_count()
    with pytest.raises(ValueError, match="evaluate returned"):
        lockstep_minimize(starts(4), lambda pts: ([0.0], [np.zeros(4)]), method="L-BFGS-B", bounds=BOUNDS)
    assert threading.active_count() == before
    with pytest.raises(ValueError, match="jac"):
        lockstep_minimize(starts(2), batch, method="SLSQP", jac=True)
    assert threading.active_count() == before


def test_a_value_that_is_not_finite_reaches_scipy_with_a_zero_gradient(monkeypatch):
    """+inf from the evaluator with a NaN gradient beside it: the optimiser's objective sees (inf, zeros)."""
    seen = []
    real = scipy.optimize.minimize

    def spy(fun, x0, **kw):
        for x in (x0, np.asarray(x0) + 0.25):
            seen.append(fun(np.array(x, dtype=float)))
        return real(lambda z: value_and_gradient(z), x0, **kw)

    monkeypatch.setattr(scipy.optimize, "minimize", spy)

    def evaluate(points):
        return [np.inf if p[0] > 0.1 else 1.5 for p in points], [np.full(4, np.nan) if p[0] > 0.1 else np.arange(4.0) for p in points]

    got, rounds = lockstep_minimize([np.zeros(4)], evaluate, method="SLSQP", bounds=BOUNDS)
    assert rounds == 2 and got[0] is not None
    (f0, g0), (f1, g1) = seen
    assert f0 == 1.5 and np.array_equal(g0, np.arange(4.0))
    assert f1 == np.inf and np.array_equal(g1, np.zeros(4))


# ---- refusals, decided on the host -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


def data(d=2, N=40, seed=3):
    rs = np.random.RandomState(seed)
    X = rs.rand(N, d)
    return X, np.sin(3 * X.sum(1)) + 0.05 * rs.randn(N)


def m52_gp(g, **kw):
    X, y = data()
    return g.GaussianProcess(g.Matern52Kernel(num_dim=2, initial_params=[1.0, 0.5, 0.5], param_bounds=[(1e-2, 10.0)] * 3),
                             noise_k=g.DiagonalNoiseKernel(num_dim=2, initial_noise=0.1, noise_bound=(1e-3, 5.0)), X=X, y=y, err_y=0.02, **kw)


def test_batch_starts_refuses_what_it_cannot_run_before_any_device_is_touched(g, monkeypatch):
    from gptools_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(_lib, "Context", no_device)
    gp = m52_gp(g)
    with pytest.raises(ValueError, match="gradient='device'"):
        gp.optimize_hyperparameters(random_starts=4, batch_starts=True)
    with pytest.raises(ValueError, match="more than one start"):
        gp.optimize_hyperparameters(random_starts=1, gradient="device", batch_starts=True)
    with pytest.raises(ValueError, match="more than one start"):
        gp.optimize_hyperparameters(random_starts=0, gradient="device", batch_starts=True)
    with pytest.raises(ValueError, match="more than one start"):
        gp.optimize_hyperparameters(gradient="device", batch_starts=True)
    for kw in (dict(method="Nelder-Mead"), dict(opt_kwargs={"method": "BFGS"})):
        with pytest.raises(ValueError, match="SLSQP, L-BFGS-B and TNC"):
            gp.optimize_hyperparameters(random_starts=4, gradient="device", batch_starts=True, **kw)
    assert gp._batch_gradient_refusal() is None


def test_ll_gradient_batch_and_batch_starts_refuse_warped_matrix_route_and_transformed_models(g, monkeypatch):
    from gptools_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(_lib, "Context", no_device)
    X, y = data()
    p = [np.array([1.0, 0.5, 0.5, 0.1])] * 2

    def noise():
        return g.DiagonalNoiseKernel(num_dim=2, initial_noise=0.1, noise_bound=(1e-3, 5.0))

    base = g.Matern52Kernel(num_dim=2, initial_params=[1.0, 0.5, 0.5], param_bounds=[(1e-2, 10.0)] * 3)
    from gptools_amd.kernel.warping import LinearWarpedKernel
    warped = g.GaussianProcess(LinearWarpedKernel(base, [0.0, 0.0], [1.5, 1.5]), noise_k=noise(), X=X, y=y, err_y=0.02)

    class HostKernel(g.Matern52Kernel):
        def __call__(self, *a, **k):                           # a Python-defined kernel: K_tot is assembled on the host
            return super(HostKernel, self).__call__(*a, **k)
    matrix = g.GaussianProcess(HostKernel(num_dim=2, initial_params=[1.0, 0.5, 0.5], param_bounds=[(1e-2, 10.0)] * 3), noise_k=noise(),
                               X=X, y=y, err_y=0.02)
    T = np.random.RandomState(0).rand(10, len(y)) / len(y)
    transformed = g.GaussianProcess(g.Matern52Kernel(num_dim=2, initial_params=[1.0, 0.5, 0.5], param_bounds=[(1e-2, 10.0)] * 3), noise_k=noise())
    transformed.add_data(X, T.dot(y), err_y=0.02, T=T)
    large = m52_gp(g)
    large.batch_grid_max_n = 16
    for gp, text in ((warped, "warped model"), (matrix, "matrix route"), (transformed, "linear transform"), (large, "batch_grid_max_n")):
        assert text in gp._batch_gradient_refusal()
        with pytest.raises(NotImplementedError, match=text):
            gp.ll_gradient_batch(p)
        if gp is transformed or gp is large:                  # (what gradient='device' alone accepts: the keyword's own refusal)
            with pytest.raises(NotImplementedError, match=text):
                gp.optimize_hyperparameters(random_starts=3, gradient="device", batch_starts=True)
