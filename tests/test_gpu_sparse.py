"""GPU suite (-m gpu): the inducing-point path -- gpt_sparse_fit / gpt_sparse_predict (api_sparse.inc, ksparse.hip) through
SparseGaussianProcess.

The yardstick is the host's (tests/sparse_cases.py): the dense N(0, Q_ff + Lambda) log-density and the dense predictive formulas in
numpy / LAPACK on covariance blocks from the CPU oracle's builder -- never an output of the sparse code under test, except where a
test is about bits.  Every bound is ten times the host's own discrepancy between its two routes (Woodbury, dense) to the same
figure at the same inputs, measured on the CPU by tests/test_sparse_host.py and recorded in sparse_cases.HOST_ERR with the
condition numbers beside it, never below the format floor that module states.  Each figure is printed before it is asserted."""
import functools
import warnings

import numpy as np
import pytest

import sparse_cases as S

pytestmark = pytest.mark.gpu

PARAMS = [(name, m, ch) for name, c in S.CASES.items() for m in c["methods"] for ch in c["chunks"]]


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


@functools.lru_cache(maxsize=None)
def host_ref(name, method):
    """The dense route of a case: computed once, shared, never modified."""
    from oracle import oracle as O
    O.build()
    return S.host_routes(O, name, method)[1]


def kernel_of(g, terms, d):
    cls = {"se": g.SquaredExponentialKernel, "m52": g.Matern52Kernel, "rq": g.RationalQuadraticKernel}

    def one(name, p):
        return cls[name](num_dim=d, initial_params=list(p), param_bounds=[(0.0, 1e3)] * len(p))
    out = None
    for t in terms:
        k = one(t[0], t[1]) * one(t[2], t[3]) if len(t) == 4 else one(t[0], t[1])
        out = k if out is None else out + k
    return out


def noise(g, d):
    return g.DiagonalNoiseKernel(num_dim=d, initial_noise=S.NOISE, noise_bound=(0.0, 5.0))


def make(g, name, method, chunk, **kw):
    c, d = S.CASES[name], S.case_data(name)
    args = dict(noise_k=noise(g, c["d"]), n_Z=d["nZ"], method=method, jitter=S.JITTER, chunk_rows=chunk, X=d["X"], y=d["y"],
                err_y=d["err_y"], n=d["n"])
    args.update(kw)
    return g.SparseGaussianProcess(args.pop("k", None) or kernel_of(g, c["terms"], c["d"]), args.pop("Z", d["Z"]), **args)


def device_figures(gp, d):
    """ll, parts and the predictions of a fitted GP in the layout sparse_cases.figures compares; std from the want = 1 route, cov from
    the want = 2 route, each without and with the noise term."""
    gp.compute_K_L_alpha_ll()
    out = dict(ll=gp.ll - gp.hyperprior(gp.params), parts=gp.ll_parts.copy())
    for suffix, flag in (("", False), ("_noise", True)):
        mean, std = gp.predict(d["Xs"], n=d["ns"], noise=flag)
        mean2, cov = gp.predict(d["Xs"], n=d["ns"], noise=flag, return_cov=True)
        mean0 = gp.predict(d["Xs"], n=d["ns"], noise=flag, return_std=False)
        assert mean.shape == std.shape == (S.NSTAR,) and cov.shape == (S.NSTAR, S.NSTAR)
        assert np.array_equal(mean, mean2) and np.array_equal(mean, mean0)
        assert np.array_equal(cov, cov.T)
        out["mean" + suffix], out["std" + suffix], out["cov" + suffix] = mean, std, cov
    return out


@pytest.mark.parametrize("name,method,chunk", PARAMS)
def test_fit_and_predict_against_the_dense_form(g, name, method, chunk):
    """ll, the five sums of the fit and the predictions at 50 test points (four derivative rows), noise False and True, against the
    host's dense form; then the same fit again: identical bits in ll and c."""
    c, d = S.CASES[name], S.case_data(name)
    gp = make(g, name, method, chunk)
    got = device_figures(gp, d)
    assert gp._fit_mode == "sparse"
    fig = S.figures(got, host_ref(name, method), d["y"])
    for k in S.FIGURES:
        print("%s %s chunk %s: %s device - host = %.3g (bound %.3g)" % (name, method, chunk, k, fig[k], S.bound(name, method, k, c["N"])))
    # the std of the want = 2 route is the covariance's diagonal
    for k in S.FIGURES:
        assert fig[k] <= S.bound(name, method, k, c["N"]), (k, fig[k])
    ll, cvec = gp.ll, gp._ctx.sparse_get_c()
    assert cvec.shape == (c["M"],) and np.all(np.isfinite(cvec))
    gp.K_up_to_date = False
    gp.compute_K_L_alpha_ll()
    assert gp.ll == ll and np.array_equal(gp._ctx.sparse_get_c(), cvec)


@pytest.mark.parametrize("method", ["fitc", "vfe", "dtc"])
def test_chunked_and_one_chunk_agree(g, method):
    """chunk_rows 128 (three chunks, the last with 44 rows) against the default (one chunk): within the bound of either against the
    host (the bits need not match: the Gram's slices differ)."""
    d = S.case_data("se_300")
    a = device_figures(make(g, "se_300", method, None), d)
    b = device_figures(make(g, "se_300", method, 128), d)
    fig = S.figures(a, b, d["y"])
    for k in S.FIGURES:
        print("se_300 %s: %s chunked - one chunk = %.3g" % (method, k, fig[k]))
        assert fig[k] <= S.bound("se_300", method, k, 300), (k, fig[k])


def test_update_hyperparameters_with_a_gamma_prior_and_bounds(g):
    d = S.case_data("se_300")
    hp = g.GammaJointPriorAlt([1.0, 0.4, 0.5], [0.5, 0.2, 0.3])
    k = g.SquaredExponentialKernel(num_dim=2, initial_params=S.SE2, hyperprior=hp)
    gp = make(g, "se_300", "vfe", None, k=k)
    x = np.array([1.2, 0.45, 0.55, 0.12])
    val = gp.update_hyperparameters(x)
    ll_data = gp.ll_parts
    prior = gp.hyperprior(gp.params)
    assert np.isfinite(prior) and prior != 0.0 and np.array_equal(gp.free_params[:], x)
    N = 300
    want = -0.5 * (ll_data[0] + 2.0 * ll_data[1] + ll_data[2] - ll_data[3] + N * np.log(2.0 * np.pi)) - 0.5 * ll_data[4]
    assert abs(-val - (want + prior)) <= 2e-15 * (abs(want) + abs(prior)) and val == -gp.ll
    # outside the noise kernel's bounds / the prior's support: +inf, no evaluation
    assert gp.update_hyperparameters([1.2, 0.45, 0.55, 7.0]) == np.inf
    assert gp.update_hyperparameters([-1.0, 0.45, 0.55, 0.12]) == np.inf
    assert gp.update_hyperparameters(x) == val


def test_duplicated_inducing_row_without_jitter_is_a_status(g):
    """Z[1] = Z[0], sigma_f = 1, jitter = 0: the second pivot of K_uu is 1 - 1 * 1 = 0 exactly, so the factorisation reports its
    second leading minor -- a status, as tests/test_gpu_parity.py::test_g5_not_positive_definite pins for the dense path: +inf from
    update_hyperparameters, LinAlgError when called directly."""
    d = S.case_data("se_300")
    Z = d["Z"].copy()
    Z[1] = Z[0]
    k = g.SquaredExponentialKernel(num_dim=2, initial_params=[1.0, 0.4, 0.6], param_bounds=[(0.0, 1e3)] * 3)
    gp = make(g, "se_300", "fitc", None, k=k, Z=Z, jitter=0.0)
    assert gp.update_hyperparameters([1.0, 0.4, 0.6, 0.1]) == np.inf
    gp.K_up_to_date = False
    with pytest.raises(np.linalg.LinAlgError) as ei:
        gp.compute_K_L_alpha_ll()
    assert "K_uu" in str(ei.value) and "2-th leading minor" in str(ei.value)
    # the context is usable afterwards: distinct inducing inputs fit
    gp.set_inducing(d["Z"])
    assert np.isfinite(gp.update_hyperparameters([1.0, 0.4, 0.6, 0.1]))


def test_optimize_hyperparameters_does_not_end_below_its_start(g):
    gp = make(g, "se_300", "vfe", None)
    gp.compute_K_L_alpha_ll()
    start = gp.ll
    res, nstarts = gp.optimize_hyperparameters(random_starts=0, opt_kwargs={"options": {"maxiter": 15}})
    print("optimize_hyperparameters: ll %.6f -> %.6f in %d evaluations" % (start, gp.ll, res.nfev))
    assert nstarts == 1 and np.isfinite(gp.ll) and gp.ll >= start and gp.ll == -res.fun


def test_compute_ll_matrix_walks_the_grid_one_vector_at_a_time(g):
    gp = make(g, "se1_64", "fitc", None)
    here = np.array(gp.free_params[:], dtype=float)
    ll_vals, axes = gp.compute_ll_matrix([(0.8, 1.2), (0.3, 0.4), (0.05, 0.15)], 2)
    assert ll_vals.shape == (2, 2, 2) and np.all(np.isfinite(ll_vals)) and np.array_equal(gp.free_params[:], here)
    assert ll_vals[1, 0, 1] == -gp.update_hyperparameters([axes[0][1], axes[1][0], axes[2][1]])


def test_draw_sample_goes_through_the_returned_covariance(g):
    d = S.case_data("se_300")
    gp = make(g, "se_300", "fitc", None)
    mean, cov = gp.predict(d["Xs"][:12], n=d["ns"][:12], return_cov=True)
    u = np.random.RandomState(3).randn(12, 5)
    samp = gp.draw_sample(d["Xs"][:12], n=d["ns"][:12], rand_vars=u)
    L = np.linalg.cholesky(cov + 1e3 * np.finfo(float).eps * np.eye(12))
    np.testing.assert_allclose(samp, mean[:, None] + L.dot(u), rtol=0, atol=1e-9)


def test_dense_fit_survives_a_sparse_fit_on_its_context(g):
    """gpt_fit, gpt_sparse_fit, gpt_predict on ONE context: the dense predictions' bits are those without the sparse fit between."""
    from gptools_amd import _lib
    d = S.case_data("se_300")
    nk = noise(g, 2)
    ctx = _lib.Context()
    ctx.set_data(d["X"], d["n"])
    ll0, _ = ctx.fit(_lib.KERNEL_SE, S.SE2, S.NOISE ** 2, d["y"], d["err_y"], 1e2 * np.finfo(float).eps)
    before = ctx.predict(d["Xs"], d["ns"], 2, nk.params, nk.n)
    ll1, _ = ctx.fit(_lib.KERNEL_SE, S.SE2, S.NOISE ** 2, d["y"], d["err_y"], 1e2 * np.finfo(float).eps)
    ctx.sparse_set_inducing(d["Z"], d["nZ"])
    lls, parts = ctx.sparse_fit(_lib.SPARSE_METHODS["fitc"], [(_lib.KERNEL_SE, S.SE2)], S.NOISE ** 2, d["y"], d["err_y"], S.JITTER, 128)
    sp = ctx.sparse_predict(d["Xs"], d["ns"], 2, nk.params, nk.n)
    after = ctx.predict(d["Xs"], d["ns"], 2, nk.params, nk.n)
    assert ll0 == ll1 and np.isfinite(lls)
    for a, b in zip(before, after):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    # ... and the other way round: the sparse predictions after the dense ones
    sp2 = ctx.sparse_predict(d["Xs"], d["ns"], 2, nk.params, nk.n)
    for a, b in zip(sp, sp2):
        assert np.array_equal(a, b)


def test_calls_out_of_order_and_refusals_of_the_library(g):
    from gptools_amd import _lib
    d = S.case_data("se_300")
    terms = [(_lib.KERNEL_SE, S.SE2)]
    ctx = _lib.Context()
    with pytest.raises(_lib.GPTBackendError):                     # GPT_E_STATE: no data
        ctx.sparse_set_inducing(d["Z"], d["nZ"])
    ctx.set_data(d["X"], d["n"])
    with pytest.raises(_lib.GPTBackendError):                     # no inducing points
        ctx.sparse_fit(0, terms, 0.01, d["y"], d["err_y"], S.JITTER)
    ctx.sparse_set_inducing(d["Z"], d["nZ"])
    with pytest.raises(_lib.GPTBackendError):                     # no sparse fit
        ctx.sparse_predict(d["Xs"], d["ns"], 1)
    with pytest.raises(ValueError):
        ctx.sparse_fit(3, terms, 0.01, d["y"], d["err_y"], S.JITTER)
    with pytest.raises(ValueError):
        ctx.sparse_fit(0, terms, 0.01, d["y"], d["err_y"], S.JITTER, chunk_rows=100)
    with pytest.raises(ValueError):                               # a Lambda_i that is not positive: GPT_E_VALUE
        ctx.sparse_fit(1, terms, 0.0, d["y"], np.zeros(300), S.JITTER)
    ctx.set_T(np.eye(300))
    with pytest.raises(NotImplementedError):
        ctx.sparse_fit(0, terms, 0.01, d["y"], d["err_y"], S.JITTER)
    ctx.set_T(None)
    ctx.set_warp([(_lib.WARP_LINEAR, [-0.5, -0.25, 1.5, 2.0])])
    with pytest.raises(NotImplementedError):
        ctx.sparse_fit(0, terms, 0.01, d["y"], d["err_y"], S.JITTER)
    ctx.set_warp(None)
    ll, _ = ctx.sparse_fit(0, terms, 0.01, d["y"], d["err_y"], S.JITTER)
    assert np.isfinite(ll)
    ctx.set_data(d["X"], d["n"])                                  # new data drop the inducing points and the fit
    with pytest.raises(_lib.GPTBackendError):
        ctx.sparse_predict(d["Xs"], d["ns"], 1)


@pytest.mark.parametrize("rows,mg,nslices", [(1, 64, 1), (3, 64, 2), (5, 192, 0), (130, 128, 7), (1000, 320, 1), (257, 64, 0)])
def test_gram_kernel_alone(rows, mg, nslices):
    """gpt_dev_sparse_gram on integer data, where every order of summation gives the same bits: G += V^T V against numpy, exactly;
    a last slice shorter than four rows, one slice, several tiles, and the accumulation onto what G held."""
    import torch
    from gptools_amd import _lib
    rs = np.random.RandomState(rows + mg)
    ldv = mg + 64
    V = rs.randint(-4, 5, size=(rows, ldv)).astype(float)
    G0 = rs.randint(-3, 4, size=(mg, mg)).astype(float)
    ctx = _lib.Context()
    dV = torch.tensor(V, device="cuda")
    dG = torch.tensor(G0, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.load().gpt_dev_sparse_gram(ctx.handle, dV.data_ptr(), ldv, rows, mg, nslices, dG.data_ptr(), mg))
    ctx.synchronize()
    got = dG.cpu().numpy()
    want = G0 + V[:, :mg].T.dot(V[:, :mg])
    low = np.tril(np.ones((mg // 64, mg // 64))).repeat(64, 0).repeat(64, 1) > 0      # the 64 x 64 tiles on and below the diagonal
    assert np.array_equal(got[low], want[low])
    assert np.array_equal(got[~low], G0[~low])                                        # the tiles above it are not touched
