"""Host suite (no GPU): the yardstick of the sparse-GP tests and what SparseGaussianProcess decides without a device.

test_host_routes is the measurement behind sparse_cases.HOST_ERR: the Woodbury form in numpy against the dense N(0, Q_ff + Lambda)
evaluation, on the CPU oracle's covariance blocks, at every input set tests/test_gpu_sparse.py uses.  It prints the table, asserts
every figure and every recorded constant <= 1e-10 (the ceiling of HOST_T_ERR in tests/test_gpu_loo.py) and holds the host itself to
the bound the device is held to."""
import os
import pickle
import re
import warnings

import numpy as np
import pytest

import sparse_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_METHODS = [(name, m) for name, c in S.CASES.items() for m in c["methods"]]


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


@pytest.mark.parametrize("name,method", CASE_METHODS)
def test_host_routes(oracle, name, method):
    """Woodbury against dense for one case and method; the measured figures are printed in the form HOST_ERR holds them."""
    w, d = S.host_routes(oracle, name, method)
    N = S.CASES[name]["N"]
    fig = S.figures(w, d, S.case_data(name)["y"])
    print('("%s", "%s"): cond(K_uu + jitter I) = %.1e, cond(B) = %.1e' % (name, method, w["cond_uu"], w["cond_B"]))
    print("    " + ", ".join('"%s": %.3g' % (k, fig[k]) for k in S.FIGURES))
    assert np.all(w["lam"] > 0.0)
    for k in S.FIGURES:
        assert S.HOST_ERR[(name, method)][k] <= 1e-10, k
        assert fig[k] <= 1e-10, (k, fig[k])
        assert fig[k] <= S.bound(name, method, k, N), (k, fig[k], S.bound(name, method, k, N))


def test_leibniz_product_blocks(oracle):
    """The yardstick's product blocks: (m52 * se) with derivative rows against central differences of the order-0 product."""
    rs = np.random.RandomState(5)
    X, Y = rs.rand(6, 2), rs.rand(5, 2)
    pm, ps = [0.7, 0.9, 1.3], [1.0, 1.5, 0.8]
    z6, z5 = np.zeros((6, 2), dtype=int), np.zeros((5, 2), dtype=int)

    def k0(A, B):
        return oracle.kbuild("m52", pm, A, np.zeros_like(A, dtype=int), B, np.zeros_like(B, dtype=int)) * \
            oracle.kbuild("se", ps, A, np.zeros_like(A, dtype=int), B, np.zeros_like(B, dtype=int))
    h = 1e-5
    e = np.array([h, 0.0])
    n6, n5 = z6.copy(), z5.copy()
    n6[:, 0] = 1
    n5[:, 0] = 1
    got = S._leibniz_product(oracle, "m52", pm, "se", ps, X, n6, Y, z5)
    np.testing.assert_allclose(got, (k0(X + e, Y) - k0(X - e, Y)) / (2 * h), rtol=0, atol=1e-8)
    got = S._leibniz_product(oracle, "m52", pm, "se", ps, X, n6, Y, n5)
    ref = (k0(X + e, Y + e) - k0(X + e, Y - e) - k0(X - e, Y + e) + k0(X - e, Y - e)) / (4 * h * h)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-5)


# ---- SparseGaussianProcess without a device ----------------------------------------------------------------------------------
def se2(g):
    return g.SquaredExponentialKernel(num_dim=2, initial_params=S.SE2, param_bounds=[(0.0, 1e3)] * 3)


def noise(g, d=2):
    return g.DiagonalNoiseKernel(num_dim=d, initial_noise=S.NOISE, noise_bound=(0.0, 5.0))


def make(g, **kw):
    d = S.case_data("se_300")
    args = dict(noise_k=noise(g), X=d["X"], y=d["y"], err_y=0.02, n=d["n"])
    args.update(kw)
    return g.SparseGaussianProcess(args.pop("k", se2(g)), args.pop("Z", d["Z"]), **args)


def test_exported_and_a_subclass(g):
    assert "SparseGaussianProcess" in g.sparse.__all__ and issubclass(g.SparseGaussianProcess, g.GaussianProcess)
    gp = make(g, method="vfe", jitter=1e-8, chunk_rows=128)
    assert (gp.method, gp.jitter, gp.chunk_rows) == ("vfe", 1e-8, 128)
    assert gp.Z.shape == (40, 2) and gp.n_Z.shape == (40, 2) and not gp.n_Z.any()
    assert len(gp.free_params) == 4 and gp.X.shape == (300, 2) and not gp.K_up_to_date


def test_argument_checks(g):
    d = S.case_data("se_300")
    with pytest.raises(ValueError):
        make(g, Z=np.zeros((5, 3)))
    with pytest.raises(ValueError):
        make(g, Z=np.zeros((0, 2)))
    with pytest.raises(ValueError):
        make(g, Z=np.full((5, 2), np.nan))
    with pytest.raises(ValueError):
        make(g, n_Z=np.zeros((7, 2), dtype=int))
    with pytest.raises(ValueError):
        make(g, method="sor")
    with pytest.raises(ValueError):
        make(g, jitter=-1.0)
    with pytest.raises(ValueError):
        make(g, chunk_rows=100)
    with pytest.raises(g.GPArgumentError):
        g.SparseGaussianProcess(se2(g), d["Z"], X=d["X"])
    gp = make(g)
    with pytest.raises(ValueError):
        gp.set_inducing(np.zeros((4, 1)))
    gp.K_up_to_date = True
    gp.set_inducing(d["Z"][:7], n_Z=0)
    assert gp.Z.shape == (7, 2) and not gp.K_up_to_date and not gp._data_on_device


def test_refusals_that_need_no_device(g):
    d = S.case_data("se_300")
    with pytest.raises(NotImplementedError):
        make(g, T=np.eye(300))
    with pytest.raises(NotImplementedError):
        make(g, use_hyper_deriv=True)
    gp = make(g)
    with pytest.raises(NotImplementedError):
        gp.add_data(d["X"][:3], d["y"][:3], T=np.eye(3))

    class Mine(g.SquaredExponentialKernel):                    # a Python-defined __call__: no device model
        def __call__(self, Xi, Xj, ni, nj, hyper_deriv=None, symmetric=False):
            return np.zeros(len(Xi))
    with pytest.raises(NotImplementedError):
        make(g, k=Mine(num_dim=2, initial_params=S.SE2, param_bounds=[(0.0, 1e3)] * 3))
    with pytest.raises(NotImplementedError):
        make(g, k=g.LinearWarpedKernel(se2(g), [-0.5, -0.25], [1.5, 2.0]))
    with pytest.raises(NotImplementedError):
        make(g, noise_k=se2(g))
    # refused at the call, not mapped to +inf by update_hyperparameters' error handling
    x0 = np.array(gp.free_params[:], dtype=float)
    gp.use_hyper_deriv = True
    with pytest.raises(NotImplementedError):
        gp.update_hyperparameters(x0)
    gp.use_hyper_deriv = False
    with pytest.raises(NotImplementedError):
        gp.update_hyperparameters(x0, hyper_deriv_handling="deriv")
    gp.partitioned = True
    with pytest.raises(NotImplementedError):
        gp.update_hyperparameters(x0)
    gp.partitioned = False
    for call in (gp.ll_gradient, gp.loo_predict, gp.loo_log_likelihood, gp.loo_gradient, lambda: gp.ll_batch([x0]),
                 lambda: gp.ll_gradient_batch([x0]), lambda: gp.L, lambda: gp.alpha,
                 lambda: gp.optimize_hyperparameters(gradient="device"), lambda: gp.optimize_hyperparameters(objective="loo"),
                 lambda: gp.optimize_hyperparameters(batch_starts=True, random_starts=2),
                 lambda: gp.predict(d["Xs"], use_MCMC=True), lambda: gp.predict_MCMC(d["Xs"]),
                 lambda: gp.compute_from_MCMC(d["Xs"])):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError):
        gp.sample_hyperparameter_posterior(nwalkers=8, nsamp=1, stepping="library")


def test_pickle_drops_the_device_state(g):
    gp = make(g, method="dtc")
    gp._data_on_device = True
    gp2 = pickle.loads(pickle.dumps(gp))
    assert isinstance(gp2, g.SparseGaussianProcess) and gp2.method == "dtc" and np.array_equal(gp2.Z, gp.Z)
    assert gp2._ctx_obj is None and not gp2._data_on_device and not gp2.K_up_to_date


def test_exports_and_bindings():
    """The ctypes argument lists of the new exports match the header's."""
    from gptools_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpt_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("gpt_sparse_set_inducing", "gpt_sparse_fit", "gpt_sparse_predict", "gpt_sparse_get_c", "gpt_dev_sparse_gram",
                 "gpt_dev_sparse_lambda", "gpt_dev_sparse_rowsum", "gpt_dev_sparse_var", "gpt_dev_sparse_assemble_b"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, hdr)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and len(args) == len(params), (name, params)
        for p, a in zip(params, args):
            if "gpt_ctx" in p:
                assert a is _lib.C.c_void_p, p
            elif "double *" in p:
                assert a in ((_lib._dp, _lib.C.c_void_p) if name.startswith("gpt_dev_") else (_lib._dp,)), p
            elif "int32_t *" in p or "int *" in p:
                assert a is _lib._ip, p
            elif p.startswith("int64_t "):
                assert a is _lib.C.c_int64, p
            elif p.startswith("double "):
                assert a is _lib.C.c_double, p
            else:
                assert p.startswith("int ") and a is _lib.C.c_int, p
        assert hasattr(_lib.load(), name)
    assert _lib.SPARSE_METHODS == {"fitc": 0, "vfe": 1, "dtc": 2}
    for mname, code in (("FITC", 0), ("VFE", 1), ("DTC", 2)):
        assert re.search(r"#define\s+GPT_SPARSE_%s\s+%d\b" % (mname, code), hdr)
