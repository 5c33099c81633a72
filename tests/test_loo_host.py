"""CPU suite: the host half of leave-one-out cross-validation (GaussianProcess.loo_predict / loo_log_likelihood / loo_gradient,
optimize_hyperparameters(objective="loo"), remove_outliers, gpt_loo / gpt_loo_grad_diff) -- the refusals, the assembly of the
gradient, remove_outliers' bookkeeping and the binding.  The numbers are the GPU suite's (tests/test_gpu_loo.py)."""
import os
import re
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


def _data(d, N=12, seed=3):
    rs = np.random.RandomState(seed)
    X = rs.rand(N, d)
    return X, np.sin(3 * X.sum(1))


def _se(g, d=1):
    return g.SquaredExponentialKernel(num_dim=d, initial_params=[1.0] + [0.3] * d, param_bounds=[(0.0, 10.0)] * (d + 1))


@pytest.fixture()
def no_device(g, monkeypatch):
    """Any attempt to create a context, hence any device call, fails the test."""
    from gptools_amd import _lib

    def boom(*a, **kw):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_lib, "Context", boom)
    monkeypatch.setattr(_lib, "default_context", boom)


def test_refusals_are_raised_before_any_device_call(g, no_device, monkeypatch):
    X, y = _data(1)
    # a transform T
    gp = g.GaussianProcess(_se(g))
    gp.add_data(X, y[:5], err_y=0.1, T=np.random.RandomState(0).rand(5, 12))
    with pytest.raises(NotImplementedError, match="transform"):
        gp.loo_gradient()
    with pytest.raises(NotImplementedError, match="transform"):
        gp.optimize_hyperparameters(random_starts=0, gradient="device", objective="loo")
    with pytest.raises(NotImplementedError, match="transform"):
        gp.remove_outliers()
    with pytest.raises(NotImplementedError, match="transform"):
        gp.remove_outliers(method="loo")
    # a warped model
    warped = g.GaussianProcess(g.BetaWarpedKernel(_se(g)), X=X, y=y, err_y=0.1)
    with pytest.raises(NotImplementedError, match="warped"):
        warped.loo_gradient()
    with pytest.raises(NotImplementedError, match="warped"):
        warped.optimize_hyperparameters(random_starts=0, gradient="device", objective="loo")

    # the matrix route
    class Mine(g.SquaredExponentialKernel):
        def __call__(self, Xi, Xj, ni, nj, hyper_deriv=None, symmetric=False):
            return np.ones(np.atleast_2d(Xi).shape[0])
    python_kernel = g.GaussianProcess(Mine(num_dim=1, initial_params=[1.0, 0.3], param_bounds=[(0.0, 10.0)] * 2), X=X, y=y, err_y=0.1)
    with pytest.raises(NotImplementedError, match="matrix route"):
        python_kernel.loo_gradient()
    # a partitioned fit
    part = g.GaussianProcess(_se(g), X=X, y=y, err_y=0.1)
    monkeypatch.setattr(part, "_partitioned_possible", lambda model=None: True)
    with pytest.raises(NotImplementedError, match="partitioned"):
        part.loo_gradient()
    # the objective and what it cannot be combined with
    gp = g.GaussianProcess(_se(g), X=X, y=y, err_y=0.1)
    with pytest.raises(ValueError, match="objective"):
        gp.optimize_hyperparameters(random_starts=0, objective="cv")
    with pytest.raises(ValueError, match="batch_starts"):
        gp.optimize_hyperparameters(random_starts=4, gradient="device", batch_starts=True, objective="loo")
    with pytest.raises(ValueError, match="jac"):
        gp.optimize_hyperparameters(random_starts=0, objective="loo", opt_kwargs={"jac": lambda x: x})
    gp.use_hyper_deriv = True
    with pytest.raises(ValueError, match="use_hyper_deriv"):
        gp.optimize_hyperparameters(random_starts=0, objective="loo")
    gp.use_hyper_deriv = False
    with pytest.raises(ValueError, match="method"):
        gp.remove_outliers(method="mcmc")
    with pytest.raises(TypeError, match="predict arguments"):
        gp.remove_outliers(method="loo", use_MCMC=True)


@pytest.mark.parametrize("with_T", [False, True])
def test_gradient_assembly_against_numpy(g, with_T, no_device):
    """Synthetic g_dev and u: the kernel entries land in their slots (two stencil entries of one parameter add up), the noise entry
    is 2 sigma_n times the trace term, a mean parameter's entry is u^T (T) d mu / d theta, and the hyperprior's derivative is added."""
    rs = np.random.RandomState(7)
    d, N = 2, 9
    X = rs.rand(N, d)
    k = g.Matern52Kernel(num_dim=d, initial_params=[1.3, 0.4, 2.5], fixed_params=[False, True, False], param_bounds=[(0.0, 1e3)] * 3)
    nk = g.DiagonalNoiseKernel(num_dim=d, initial_noise=0.3, noise_bound=(0.0, 5.0))
    mu = g.LinearMeanFunction(num_dim=d, initial_params=[0.5, -1.0, 0.2])
    gp = g.GaussianProcess(k, noise_k=nk, mu=mu)
    T = rs.rand(4, N) if with_T else None
    Ny = 4 if with_T else N
    gp.add_data(X, rs.rand(Ny), err_y=0.1, T=T)
    prior_grad = np.arange(1.0, 7.0)
    gp._hyperprior_gradient = lambda: prior_grad
    u = rs.randn(Ny)
    g_dev = np.array([2.0, 3.0, 5.0, 7.0])                   # three stencil entries and the trace term
    got = gp._loo_gradient_assemble([0, 1, 1], g_dev, u)
    want = np.zeros(6)
    want[0], want[1] = 2.0, 3.0 + 5.0
    want[2] = 2.0 * 0.3 * 7.0
    for i in range(3):
        dmu = mu(X, np.zeros((N, d), dtype=int), hyper_deriv=i)
        want[3 + i] = (T.dot(dmu) if with_T else dmu).dot(u)
    assert np.allclose(got, want + prior_grad, rtol=1e-14, atol=0)
    assert np.all(want[3:] != 0.0)
    # fixed noise: no entry for it, the mean's entries move up
    gp.noise_k = g.DiagonalNoiseKernel(num_dim=d, initial_noise=0.3, noise_bound=(0.0, 5.0), fixed_noise=True)
    gp._hyperprior_gradient = lambda: np.zeros(5)
    got = gp._loo_gradient_assemble([0, 1, 1], g_dev, u)
    assert np.allclose(got, np.concatenate((want[:2], want[3:])), rtol=1e-14, atol=0)


@pytest.mark.parametrize("method", ["predict", "loo"])
def test_remove_outliers_bookkeeping(g, method, no_device, monkeypatch):
    rs = np.random.RandomState(1)
    N = 10
    X, y = rs.rand(N, 2), rs.rand(N)
    n = np.zeros((N, 2), dtype=int)
    n[7, 1] = 1
    err_y = np.full(N, 0.1)
    err_y[4] = 0.0                                            # an exact observation is never bad by the predict rule
    gp = g.GaussianProcess(_se(g, 2), X=X, y=y, err_y=err_y, n=n)
    gp.K_up_to_date = True
    gp._data_on_device = True
    version = getattr(gp, "_data_version", 0)
    off = np.zeros(N)
    off[[2, 4, 7]] = [0.3, 5.0, -0.31]                        # 3 sigma exactly at point 2 (>= thresh counts), far off at 4, beyond at 7
    off[5] = 0.29
    seen = {}

    def predict(Xs, n=0, noise=False, return_std=True, **kw):
        seen.update(kw, noise=noise, return_std=return_std, n=n, X=Xs)
        return y + off

    def loo_predict(return_std=True):
        assert return_std
        return y - off, np.full(N, 0.1)
    monkeypatch.setattr(gp, "predict", predict)
    monkeypatch.setattr(gp, "loo_predict", loo_predict)
    kw = {"use_MCMC": False} if method == "predict" else {}
    X_bad, y_bad, err_bad, n_bad, bad = gp.remove_outliers(thresh=3, method=method, **kw)
    # (0.3 / 0.1 rounds below 3 in floating point for one sign and not the other: leave point 2 out of the exact comparison)
    expect = np.zeros(N, dtype=bool)
    expect[7] = True
    if method == "loo":
        expect[4] = True
    rest = np.arange(N) != 2
    assert bad.dtype == bool and bad.shape == (N,) and np.array_equal(bad[rest], expect[rest])
    assert np.array_equal(X_bad, X[bad]) and np.array_equal(y_bad, y[bad]) and np.array_equal(err_bad, err_y[bad]) and np.array_equal(n_bad, n[bad])
    assert np.array_equal(gp.X, X[~bad]) and np.array_equal(gp.y, y[~bad]) and np.array_equal(gp.err_y, err_y[~bad]) and np.array_equal(gp.n, n[~bad])
    assert gp.K_up_to_date is False and gp._data_on_device is False and gp._data_version == version + 1
    if method == "predict":
        assert seen["noise"] is False and seen["return_std"] is False and seen["use_MCMC"] is False
        assert np.array_equal(seen["X"], X) and np.array_equal(seen["n"], n)


def test_exports_and_bindings():
    """The ctypes argument lists of the two exports match the header's."""
    from gptools_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpt_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("gpt_loo", "gpt_loo_grad_diff"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, hdr)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and len(args) == len(params), (name, params)
        for p, a in zip(params, args):
            if "gpt_ctx" in p:
                assert a is _lib.C.c_void_p, p
            elif "double *" in p:
                assert a is _lib._dp, p
            elif "int *" in p:
                assert a is _lib._ip, p
            else:
                assert p.startswith("int ") and a is _lib.C.c_int, p
        assert hasattr(_lib.load(), name)
    assert callable(_lib.Context.loo) and callable(_lib.Context.loo_grad_diff)
    with pytest.raises(ValueError, match="loo_grad_diff"):
        class Fake(object):
            _term_nparams = [3]
        _lib.Context._pack_stencil(Fake(), "loo_grad_diff", [0], [[1.0, 0.3]], [[1.0, 0.3, 0.4]], [1e-5])
