"""CPU suite: the host half of the device LML gradient by per-pair differencing (GaussianProcess.ll_gradient,
optimize_hyperparameters(gradient="device"), gpt_ll_grad_diff) -- the stencils, the refusals and the binding.  The numbers are the
GPU suite's (tests/test_gpu_grad_diff.py)."""
import os
import re
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


def _data(d, N=12, seed=3):
    rs = np.random.RandomState(seed)
    X = rs.rand(N, d)
    return X, np.sin(3 * X.sum(1))


def test_stencil_steps_denominators_and_restored_parameters(g):
    """A sum of Matern-5/2 (one length scale fixed) and RQ: one entry per free kernel parameter, in the term that holds it, with the
    term's complete parameters at theta -+ eps, eps = rel_step max(1, |theta|), and denom the floating-point theta_b - theta_a;
    the noise parameter gets no stencil; afterwards the hyperparameters are the bits they were and the fit still counts."""
    d = 2
    k = g.Matern52Kernel(num_dim=d, initial_params=[1.3, 0.4, 2.5], fixed_params=[False, True, False], param_bounds=[(0.0, 1e3)] * 3) + \
        g.RationalQuadraticKernel(num_dim=d, initial_params=[0.7, 1.5, 0.5, 30.0], param_bounds=[(0.0, 1e3)] * 4)
    nk = g.DiagonalNoiseKernel(num_dim=d, initial_noise=0.1, noise_bound=(0.0, 5.0))
    X, y = _data(d)
    gp = g.GaussianProcess(k, noise_k=nk, X=X, y=y, err_y=0.02)
    gp.K_up_to_date = True                                   # (pretend: the stencil must leave the flag as it found it)
    before = np.array(gp.params[:], dtype=float)
    rel = 6e-6
    slot, tix, pa, pb, denom = gp._ll_gradient_stencil(rel)
    assert np.array_equal(np.array(gp.params[:], dtype=float), before)
    assert gp.K_up_to_date is True
    theta = np.array(gp.k.free_params[:], dtype=float)        # 1.3, 2.5 | 0.7, 1.5, 0.5, 30.0
    assert slot == list(range(6)) and tix == [0, 0, 1, 1, 1, 1]
    full = [np.array([1.3, 0.4, 2.5]), np.array([0.7, 1.5, 0.5, 30.0])]
    where = [(0, 0), (0, 2), (1, 0), (1, 1), (1, 2), (1, 3)]       # (term, index in the term's parameters)
    for h, (t, j) in enumerate(where):
        eps = rel * max(1.0, abs(theta[h]))
        a, b = full[t].copy(), full[t].copy()
        a[j], b[j] = theta[h] - eps, theta[h] + eps
        assert np.array_equal(pa[h], a) and np.array_equal(pb[h], b), h
        assert denom[h] == b[j] - a[j]                                # the difference as formed in floating point, not 2 eps
    assert denom[5] == (30.0 + rel * 30.0) - (30.0 - rel * 30.0) and abs(denom[5] - 2 * rel * 30.0) < 1e-12
    # another step rule
    assert np.allclose(gp._ll_gradient_stencil(1e-3)[4], 2e-3 * np.maximum(1.0, theta), rtol=1e-9)


def test_stencil_stays_inside_the_parameter_bounds(g):
    """An optimiser puts parameters exactly on their bounds, and beyond one the library may refuse the point (Matern's nu): a
    stencil point that would leave the bounds stays on the bound -- the difference is then one-sided and denom the floating-point
    distance actually taken; bounds that pin a parameter leave no entry; a value already outside its bounds keeps the plain stencil."""
    rel = 6e-6
    k = g.MaternKernel(num_dim=2, initial_params=[2.0, 0.5, 0.4, 3.0],
                       param_bounds=[(0.0, 2.0), (0.5, 59.0), (0.4, 0.4), (0.0, 2.5)])      # upper, lower, pinned, outside
    X, y = _data(2)
    gp = g.GaussianProcess(k, X=X, y=y, err_y=0.02)
    before = np.array(gp.params[:], dtype=float)
    slot, tix, pa, pb, denom = gp._ll_gradient_stencil(rel)
    assert np.array_equal(np.array(gp.params[:], dtype=float), before)
    assert slot == [0, 1, 3] and tix == [0, 0, 0]
    assert pb[0][0] == 2.0 and pa[0][0] == 2.0 - rel * 2.0 and denom[0] == 2.0 - (2.0 - rel * 2.0)
    assert pa[1][1] == 0.5 and pb[1][1] == 0.5 + rel and denom[1] == (0.5 + rel) - 0.5
    assert pa[2][3] == 3.0 - rel * 3.0 and pb[2][3] == 3.0 + rel * 3.0 and denom[2] == pb[2][3] - pa[2][3]
    for a, b in zip(pa, pb):
        assert a[2] == 0.4 and b[2] == 0.4


def test_stencil_of_a_masked_product_carries_the_device_encoding(g):
    """MaskedKernel(Gibbs-tanh on dimension 0) * MaskedKernel(SE on dimension 1): ONE product term whose stencil points hold both
    factors' device parameters -- the SE factor's expanded array with its infinite length scale."""
    from gptools_amd import _lib
    gib = g.GibbsKernel1dTanh(initial_params=[1.2, 0.3, 0.8, 0.2, 0.5], param_bounds=[(1e-3, 10.0)] * 5)
    se = g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 0.6], fixed_params=[True, False], param_bounds=[(0.0, 10.0)] * 2)
    k = g.MaskedKernel(gib, 2, [0]) * g.MaskedKernel(se, 2, [1])
    X, y = _data(2)
    gp = g.GaussianProcess(k, X=X, y=y, err_y=0.02)
    slot, tix, pa, pb, denom = gp._ll_gradient_stencil(6e-6)
    assert slot == list(range(6)) and tix == [0] * 6
    terms = gp._native_terms()
    assert len(terms) == 1 and terms[0][0] == _lib.kernel_on_dim(_lib.KERNEL_GIBBS_TANH, 0) and terms[0][2] == _lib.KERNEL_SE
    base = np.concatenate([terms[0][1], terms[0][3]])          # 5 Gibbs parameters, then [1, inf, l]
    assert base.size == 8 and np.isinf(base[6])
    for h in range(6):
        j = h if h < 5 else 7
        changed = np.nonzero(pa[h] != pb[h])[0]
        assert list(changed) == [j]
        assert pb[h][j] - pa[h][j] == denom[h]
        rest = np.arange(8) != j
        assert np.array_equal(pa[h][rest], base[rest]) and np.array_equal(pb[h][rest], base[rest])


def test_refusals_name_the_model_and_gradient_keyword_is_checked(g):
    """Warped models and the matrix route are refused with a message that says which, before any device call; an unknown value of
    `gradient` and a combination with use_hyper_deriv are ValueErrors."""
    X, y = _data(1)
    se = g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 0.3], param_bounds=[(0.0, 10.0)] * 2)
    warped = g.GaussianProcess(g.BetaWarpedKernel(se), X=X, y=y, err_y=0.1)
    with pytest.raises(NotImplementedError, match="warped"):
        warped.ll_gradient()
    with pytest.raises(NotImplementedError, match="warped"):
        warped.optimize_hyperparameters(random_starts=0, gradient="device")

    class Mine(g.SquaredExponentialKernel):
        def __call__(self, Xi, Xj, ni, nj, hyper_deriv=None, symmetric=False):
            return np.ones(np.atleast_2d(Xi).shape[0])
    python_kernel = g.GaussianProcess(Mine(num_dim=1, initial_params=[1.0, 0.3], param_bounds=[(0.0, 10.0)] * 2), X=X, y=y, err_y=0.1)
    with pytest.raises(NotImplementedError, match="matrix route"):
        python_kernel.ll_gradient()
    with pytest.raises(NotImplementedError, match="matrix route"):
        python_kernel.optimize_hyperparameters(random_starts=0, gradient="device")
    gp = g.GaussianProcess(se, X=X, y=y, err_y=0.1)
    with pytest.raises(ValueError, match="gradient"):
        gp.optimize_hyperparameters(random_starts=0, gradient="host")
    gp.use_hyper_deriv = True
    with pytest.raises(ValueError, match="use_hyper_deriv"):
        gp.optimize_hyperparameters(random_starts=0, gradient="device")


@pytest.mark.skipif(_have_gpu(), reason="checks the no-GPU failure mode")
def test_device_gradient_fails_loudly_without_gpu(g):
    from gptools_amd import _lib
    X, y = _data(2)
    k = g.Matern52Kernel(num_dim=2, initial_params=[1.0, 0.3, 0.4], param_bounds=[(1e-3, 10.0)] * 3)
    gp = g.GaussianProcess(k, X=X, y=y, err_y=0.1)
    with pytest.raises(_lib.GPTBackendError):
        gp.ll_gradient()
    # (not a +inf objective at every start and "no start ended at a finite log-posterior")
    with pytest.raises(_lib.GPTBackendError):
        gp.optimize_hyperparameters(random_starts=0, gradient="device")
    with pytest.raises(_lib.GPTBackendError):
        _lib.Context(0).ll_grad_diff([0], [[1.0, 0.3, 0.4]], [[1.0, 0.3, 0.4]], [1e-5])


def test_export_and_binding_of_ll_grad_diff():
    from gptools_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpt_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+gpt_ll_grad_diff\s*\(", hdr)
    res, args = _lib.SIGNATURES["gpt_ll_grad_diff"]
    assert len(args) == 7
    assert hasattr(_lib.load(), "gpt_ll_grad_diff")
    assert callable(_lib.Context.ll_grad_diff)
