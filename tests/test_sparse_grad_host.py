"""Host suite (no GPU) of the sparse gradient: the yardstick of tests/test_gpu_sparse_grad.py and what needs no device.

test_differencing_error is the measurement behind sparse_grad_cases.DIFF_ERR; test_host_routes_agree holds the restated adjoint form
against the dense 1/2 tr((alpha alpha^T - Sigma^-1) dSigma); test_against_central_differences holds it against central differences of
the dense N(r; 0, Q_ff + Lambda) log-density, the definition of the objective."""
import warnings

import numpy as np
import pytest

import sparse_cases as S
import sparse_grad_cases as SG


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


@pytest.mark.parametrize("name", sorted(SG.SE_CASES))
def test_differencing_error(oracle, name):
    """Adjoint form with the oracle's blocks differenced per pair against the same with its exact dK: the figure DIFF_ERR records
    (the largest over the three methods and the kernel parameters), printed in the form the table holds it."""
    worst = 0.0
    for method in SG.METHODS:
        exact, diff, _, _, _ = SG.se_gradients(oracle, name, method)
        worst = max(worst, np.abs(diff - exact).max() / np.abs(exact).max())
    print('    "%s": %.3g,' % (name, worst))
    assert SG.DIFF_ERR[name] <= 1e-6                     # eps^2 f''' / 6 at eps = 6e-6 and rounding 1e-16 / eps: far below
    assert worst <= SG.bound(name), (worst, SG.bound(name))      # the host holds the bound the device is held to


# The two routes share the covariance blocks and nothing else: Cholesky factors and triangular solves against an LU solve and an
# N x N inverse.  Both carry cond(K_uu + jitter I) u = 1e8 * 1e-16 = 1e-8 of their largest intermediate; measured here 6e-14 ... 8e-13
# of the largest entry over the cases below (1.4e-11 at se_m127).  The bound is the estimate with a margin of ten.
ROUTES_TOL = 1e-7


@pytest.mark.parametrize("name", ["se_300", "se_m63", "se3_130", "se1_64"])
def test_host_routes_agree(oracle, name):
    for method in SG.METHODS:
        exact, _, dens, noise, _ = SG.se_gradients(oracle, name, method)
        scale = max(np.abs(dens).max(), abs(noise[1]))
        err = max(np.abs(exact - dens).max(), abs(noise[0] - noise[1])) / scale
        print("%s %s: adjoint - dense = %.3g of the largest entry %.4g" % (name, method, err, scale))
        assert err <= ROUTES_TOL, (name, method, err)


def small_case():
    """SE, d = 2, N = 120, M = 17, heteroscedastic err_y, 20 derivative rows."""
    rs = np.random.RandomState(7)
    X, n, y = S.inputs(120, 2, nder=20)
    Z = rs.rand(17, 2)
    nZ = np.zeros((17, 2), dtype=int)
    err = 0.02 + 0.05 * rs.rand(120)
    return X, n, y, Z, nZ, err


#: |adjoint form - central differences of the dense density| relative to the largest entry, measured on the CPU at small_case() with
#: h = 1e-5 max(1, |theta|) (kernel parameters and the noise VARIANCE): the figure printed below.  The bound is ten times it: the
#: differences carry the truncation h^2 f''' / 6 and a rounding of 1e-16 cond |ll| / h, neither of which the adjoint form shares.
FD_ERR = {"fitc": 1.32e-8, "vfe": 8.89e-9, "dtc": 1.12e-8}


@pytest.mark.parametrize("method", SG.METHODS)
def test_against_central_differences(oracle, method):
    X, n, y, Z, nZ, err = small_case()
    theta, nv = list(S.SE2), S.NOISE ** 2.0

    def blocks(p):
        t = [("se", p)]
        return dict(Kuu=S.gram(oracle, t, Z, nZ, Z, nZ), Kuf=S.gram(oracle, t, Z, nZ, X, n), kd=S.kdiag(oracle, t, X, n),
                    Kus=np.zeros((17, 1)), Kss=np.zeros((1, 1)))

    def ll(p, v):
        return S.dense(blocks(p), y, v + err ** 2.0, method)["ll"]
    b = blocks(theta)
    adj = SG.adjoints(b, y, nv + err ** 2.0, method)
    got, fd = [], []
    for h in range(3):
        dk = [oracle.kbuild("se", theta, A, na, B, nb, hyper_deriv=h) for A, na, B, nb in ((Z, nZ, Z, nZ), (Z, nZ, X, n))]
        dkd = np.array([oracle.kbuild("se", theta, X[i:i + 1], n[i:i + 1], X[i:i + 1], n[i:i + 1], hyper_deriv=h)[0, 0] for i in range(120)])
        got.append(SG.contract(adj, dk[0], dk[1], dkd))
        step = 1e-5 * max(1.0, abs(theta[h]))
        tp, tm = list(theta), list(theta)
        tp[h] += step
        tm[h] -= step
        fd.append((ll(tp, nv) - ll(tm, nv)) / (tp[h] - tm[h]))
    got.append(adj["g"].sum())
    step = 1e-5 * nv
    fd.append((ll(theta, nv + step) - ll(theta, nv - step)) / ((nv + step) - (nv - step)))
    got, fd = np.array(got), np.array(fd)
    rel = np.abs(got - fd).max() / np.abs(fd).max()
    print('"%s": %.3g   (gradient %s)' % (method, rel, got))
    assert rel <= 10.0 * FD_ERR[method], (method, rel)


def test_new_names_and_old_refusals(g):
    d = S.case_data("se_300")
    k = g.SquaredExponentialKernel(num_dim=2, initial_params=S.SE2, param_bounds=[(0.0, 1e3)] * 3)
    gp = g.SparseGaussianProcess(k, d["Z"], noise_k=g.DiagonalNoiseKernel(num_dim=2, initial_noise=S.NOISE, noise_bound=(0.0, 5.0)),
                                 X=d["X"], y=d["y"], err_y=0.02, n=d["n"])
    assert callable(gp.sparse_gradient) and hasattr(g._lib.Context, "sparse_grad_diff")
    assert "gpt_sparse_grad_diff" in g._lib.SIGNATURES and "gpt_dev_sparse_grad_pairs" in g._lib.SIGNATURES
    x0 = np.array(gp.free_params[:], dtype=float)
    for call in (gp.ll_gradient, lambda: gp.ll_gradient_batch([x0]), lambda: gp.optimize_hyperparameters(gradient="device"),
                 lambda: gp.optimize_hyperparameters(gradient="sparse", batch_starts=True, random_starts=2),
                 lambda: gp.optimize_hyperparameters(gradient="sparse", objective="loo")):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError):
        gp.optimize_hyperparameters(gradient="sparse", opt_kwargs={"jac": lambda x: x})
    # the stencil is the base class's and leaves the hyperparameters as they were
    slot, tix, pa, pb, denom = gp._ll_gradient_stencil(6e-6)
    assert slot == [0, 1, 2] and tix == [0, 0, 0] and np.all(denom > 0.0)
    assert np.array_equal(np.array(gp.free_params[:], dtype=float), x0)
