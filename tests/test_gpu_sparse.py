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
        assert mean.shape == std.shape == (len(d["Xs"]),) and cov.shape == (len(d["Xs"]), len(d["Xs"]))
        assert np.array_equal(mean, mean2) and np.array_equal(mean, mean0)
        assert np.array_equal(cov, cov.T)
        out["mean" + suffix], out["std" + suffix], out["cov" + suffix] = mean, std, cov
    return out


@pytest.mark.parametrize("name,method,chunk", PARAMS)
def test_fit_and_predict_against_the_dense_form(g, name, method, chunk):
    """ll, the five sums of the fit and the predictions at the case's test points (50, or its nstar; four derivative rows), noise False
    and True, against the host's dense form; then the same fit again: identical bits in ll and c.  The want <= 1 predictions run in
    the fit's chunks: se_m127 (chunk_rows 64, 150 test points) sends them through chunks of 64, 64 and 22 rows."""
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


@pytest.mark.parametrize("method", S.CASES["m52_m300"]["methods"])
def test_chunked_and_one_chunk_agree_m52_m300(g, method):
    """M = 300: chunk_rows 256 (three chunks, the last with 188 rows) against the default (one chunk), as above."""
    d = S.case_data("m52_m300")
    a = device_figures(make(g, "m52_m300", method, None), d)
    b = device_figures(make(g, "m52_m300", method, 256), d)
    fig = S.figures(a, b, d["y"])
    for k in S.FIGURES:
        print("m52_m300 %s: %s chunked - one chunk = %.3g (bound %.3g)" % (method, k, fig[k], S.bound("m52_m300", method, k, 700)))
    for k in S.FIGURES:
        assert fig[k] <= S.bound("m52_m300", method, k, 700), (k, fig[k])


@pytest.mark.parametrize("method", S.CASES["se_m127"]["methods"])
def test_predictions_in_chunks_and_in_one_chunk_agree(g, method):
    """gpt_sparse_predict runs want <= 1 in the fit's chunks: 150 test points after a fit with chunk_rows 64 (chunks of 64, 64 and
    22 rows: r0 > 0, the offsets into mean_out / std_out, the buffers' reuse) against the same after a fit with the default chunk
    (one chunk), within the case's bound (not bit for bit: trsm_rlt may take its few-rows route, which sums in another order, at one
    chunk height and not at the other)."""
    d = S.case_data("se_m127")
    assert len(d["Xs"]) == 150
    a = device_figures(make(g, "se_m127", method, None), d)
    b = device_figures(make(g, "se_m127", method, 64), d)
    fig = S.figures(a, b, d["y"])
    for k in S.GROUPS["pred"]:
        print("se_m127 %s: %s chunked - one chunk = %.3g (bound %.3g)" % (method, k, fig[k], S.bound("se_m127", method, k, 200)))
    for k in S.GROUPS["pred"]:
        assert fig[k] <= S.bound("se_m127", method, k, 200), (k, fig[k])


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


#: the cases of test_gram_kernel_alone whose G has a row stride of mg + 64 (every other: ldg == mg)
GRAM_WIDE_LDG = {(70, 192, 3)}


@pytest.mark.parametrize("rows,mg,nslices", [(1, 64, 1), (3, 64, 2), (5, 192, 0), (130, 128, 7), (1000, 320, 1), (257, 64, 0),
                                             (8, 1088, 1), (8, 4160, 1), (70, 192, 3)])
def test_gram_kernel_alone(rows, mg, nslices):
    """gpt_dev_sparse_gram on integer data, where every order of summation gives the same bits: G += V^T V against numpy, exactly;
    a last slice shorter than four rows, one slice, several tiles, and the accumulation onto what G held.  153 and 2145 tiles (the
    Gram orders of M = 1024 and M = 4096) check the tile index recovered from sqrt(8 t + 1); one case has a G wider than its order,
    whose extra columns keep their bits."""
    import torch
    from gptools_amd import _lib
    rs = np.random.RandomState(rows + mg)
    ldv = mg + 64
    V = rs.randint(-4, 5, size=(rows, ldv)).astype(float)
    ldg = mg + 64 if (rows, mg, nslices) in GRAM_WIDE_LDG else mg
    Gwide = rs.randint(-3, 4, size=(mg, ldg)).astype(float)
    G0 = Gwide[:, :mg]
    ctx = _lib.Context()
    dV = torch.tensor(V, device="cuda")
    dG = torch.tensor(Gwide, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.load().gpt_dev_sparse_gram(ctx.handle, dV.data_ptr(), ldv, rows, mg, nslices, dG.data_ptr(), ldg))
    ctx.synchronize()
    got = dG.cpu().numpy()
    assert np.array_equal(got[:, mg:], Gwide[:, mg:])                                 # the columns behind the order keep their bits
    got = got[:, :mg]
    want = G0 + V[:, :mg].T.dot(V[:, :mg])
    low = np.tril(np.ones((mg // 64, mg // 64))).repeat(64, 0).repeat(64, 1) > 0      # the 64 x 64 tiles on and below the diagonal
    assert np.array_equal(got[low], want[low])
    assert np.array_equal(got[~low], G0[~low])                                        # the tiles above it are not touched


# ---- the four other kernels of ksparse.hip, each alone (gpt_dev_sparse_lambda / _rowsum / _var / _assemble_b) -------------------------
# Integer data wherever a sum is formed: every order of summation then gives the same bits and the comparison is exact.
M_LIST = [1, 2, 255, 256, 257, 511, 512, 513, 768, 769, 1025]      # around the 256-thread stride and the two-wide loop's 512
ULP4 = 4.0 * 2.0 ** -52


def _up(x, m):
    return (x + m - 1) // m * m


def _ip(t):
    from gptools_amd import _lib
    return _lib.C.cast(t.data_ptr(), _lib._ip)


def _within_4ulp(got, ref):
    return np.all(np.abs(got - ref) <= ULP4 * np.abs(ref))


@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("M", M_LIST)
def test_lambda_kernel_alone(M, method):
    """gpt_dev_sparse_lambda on six rows of integers: q_i exactly (through (k_i - q_i) / s_i for vfe: a dropped or doubled column
    changes an integer), log Lambda_i and the scaled row within 4 ulp of float64 (a 1-2 ulp device log; sqrt, divide, multiply),
    the columns behind M untouched; then bad rows among good ones: flag word, zeros, the good rows' bits unchanged."""
    import math
    import torch
    from gptools_amd import _lib
    lib = _lib.load()
    rows, ldv, ldr, FILL = 6, _up(M + 1, 128), 8, 777.0
    rs = np.random.RandomState(1000 * method + M)
    V = np.full((rows, ldv), FILL)
    V[:, :M] = rs.randint(-3, 4, size=(rows, M))
    q = (V[:, :M] ** 2).sum(1)
    k = rs.randint(1, 6, size=rows).astype(float)
    r = rs.randint(1, 6, size=rows) * rs.choice([-1.0, 1.0], size=rows)
    lam = k + 4.0 if method == 0 else np.full(rows, 4.0)
    ctx = _lib.Context()

    def run(kdiag, err, noise_var):
        dV = torch.tensor(V, device="cuda")
        dk, dr, de = (torch.tensor(np.asarray(a, dtype=float), device="cuda") for a in (kdiag, r, err))
        drow = torch.full((2 * ldr,), -7.0, dtype=torch.float64, device="cuda")
        dbad = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        _lib.check(lib.gpt_dev_sparse_lambda(ctx.handle, dV.data_ptr(), ldv, rows, M, method, dk.data_ptr(), dr.data_ptr(), de.data_ptr(),
                                             noise_var, drow.data_ptr(), ldr, _ip(dbad)))
        ctx.synchronize()
        return dV.cpu().numpy(), drow.cpu().numpy(), int(dbad.cpu()[0])

    # ---- every row good: noise_var 3, err 1 -> s = 4
    gV, grow, gbad = run(q + k, np.ones(rows), 3.0)
    assert gbad == 0
    assert np.array_equal(grow[ldr:ldr + rows], k / 4.0 if method == 1 else np.zeros(rows))
    assert np.array_equal(gV[:, M + 1:], V[:, M + 1:])
    assert np.array_equal(grow[rows:ldr], np.full(ldr - rows, -7.0)) and np.array_equal(grow[ldr + rows:], np.full(ldr - rows, -7.0))
    ref_log = np.array([math.log(x) for x in lam])
    ref_row = np.hstack([V[:, :M], r[:, None]]) / np.sqrt(lam)[:, None]                  # the scaled columns [0, M) and r~ in column M
    print("M %d method %d: log Lambda off by %.3g, the scaled row by %.3g (in units of 2^-52 of the reference)" % (
        M, method, (np.abs(grow[:rows] - ref_log) / np.abs(ref_log)).max() * 2.0 ** 52,
        (np.abs(gV[:, :M + 1] - ref_row) / np.maximum(np.abs(ref_row), 1e-300)).max() * 2.0 ** 52))
    assert _within_4ulp(grow[:rows], ref_log)
    assert _within_4ulp(gV[:, :M], ref_row[:, :M])
    assert _within_4ulp(gV[:, M], ref_row[:, M])

    # ---- rows 1 and 4 bad.  fitc: k_i = q_i - 10 (Lambda = -6) and k_i = nan; vfe / dtc: noise_var = 0 with err = 0 (Lambda = 0) and
    # err = inf; the good rows keep s = 4 (err = 2 where noise_var = 0)
    kd = q + k
    if method == 0:
        kd[1], kd[4] = q[1] - 10.0, np.nan
        bV, brow, bbad = run(kd, np.ones(rows), 3.0)
    else:
        err = np.full(rows, 2.0)
        err[1], err[4] = 0.0, np.inf
        bV, brow, bbad = run(kd, err, 0.0)
    good = np.array([0, 2, 3, 5])
    assert bbad == 1
    for i in (1, 4):
        assert brow[i] == 0.0 and brow[ldr + i] == 0.0 and np.array_equal(bV[i, :M + 1], np.zeros(M + 1))
    assert np.array_equal(bV[:, M + 1:], V[:, M + 1:])
    assert np.array_equal(bV[good], gV[good]) and np.array_equal(brow[good], grow[good])
    assert np.array_equal(brow[ldr + good], grow[ldr + good])

    # ---- the launcher's refusals: no column for r~, more rows than the row values hold -- GPT_E_ARG, nothing launched
    dV = torch.tensor(V, device="cuda")
    dv = torch.ones(2 * ldr, dtype=torch.float64, device="cuda")
    dbad = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for bad_M, bad_ldr in ((ldv, ldr), (M, rows - 1)):
        rc = lib.gpt_dev_sparse_lambda(ctx.handle, dV.data_ptr(), ldv, rows, bad_M, method, dv.data_ptr(), dv.data_ptr(), dv.data_ptr(), 3.0,
                                       dv.data_ptr(), bad_ldr, _ip(dbad))
        assert rc == _lib.GPT_E_ARG
    ctx.synchronize()
    assert np.array_equal(dV.cpu().numpy(), V) and np.array_equal(dv.cpu().numpy(), np.ones(2 * ldr)) and int(dbad.cpu()[0]) == 0


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1000])
def test_rowsum_kernel_alone(rows):
    """gpt_dev_sparse_rowsum on integers: both sums added, exactly, onto what acc held; the entries between rows and ldr stay out."""
    import torch
    from gptools_amd import _lib
    ldr = rows + 3
    rs = np.random.RandomState(rows)
    rowval = rs.randint(-50, 51, size=2 * ldr).astype(float)
    rowval[rows:ldr], rowval[ldr + rows:] = 1e6, 1e6
    ctx = _lib.Context()
    drow = torch.tensor(rowval, device="cuda")
    dacc = torch.tensor([5.0, -11.0], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.load().gpt_dev_sparse_rowsum(ctx.handle, drow.data_ptr(), ldr, rows, dacc.data_ptr()))
    ctx.synchronize()
    got = dacc.cpu().numpy()
    assert got[0] == 5.0 + rowval[:rows].sum() and got[1] == -11.0 + rowval[ldr:ldr + rows].sum()
    assert np.array_equal(drow.cpu().numpy(), rowval)


@pytest.mark.parametrize("M", M_LIST)
def test_var_kernel_alone(M):
    """gpt_dev_sparse_var on integers: var = kdiag - sum V^2 + sum W^2 over the columns < M against numpy, exactly; the columns at
    and behind M hold non-zero values that must not enter."""
    import torch
    from gptools_amd import _lib
    rows, ld = 5, M + 5
    rs = np.random.RandomState(M)
    V = rs.randint(-3, 4, size=(rows, ld)).astype(float)
    W = rs.randint(-3, 4, size=(rows, ld)).astype(float)
    V[:, M:], W[:, M:] = 9.0, -8.0
    kd = rs.randint(-20, 21, size=rows).astype(float)
    ctx = _lib.Context()
    dV, dW, dk = (torch.tensor(a, device="cuda") for a in (V, W, kd))
    dvar = torch.full((rows + 2,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.load().gpt_dev_sparse_var(ctx.handle, dV.data_ptr(), dW.data_ptr(), ld, rows, M, dk.data_ptr(), dvar.data_ptr()))
    ctx.synchronize()
    got = dvar.cpu().numpy()
    assert np.array_equal(got[:rows], kd - (V[:, :M] ** 2).sum(1) + (W[:, :M] ** 2).sum(1))
    assert np.array_equal(got[rows:], [-7.0, -7.0])


@pytest.mark.parametrize("M,extra", [(1, 0), (63, 0), (127, 0), (128, 0), (129, 0), (129, 64)])
def test_assemble_b_kernel_alone(M, extra):
    """gpt_dev_sparse_assemble_b: B, pre-filled with NaN, against the construction of the comment above the kernel, exactly --
    rows < M: I + G on and below the diagonal, zero above it (G's upper triangle holds integers that must not be read); row M:
    G[M][0..M), big on the diagonal, zero behind; rows > M: a unit diagonal.  ldg = M + 1 rounded up to 64, once 64 more."""
    import torch
    from gptools_amd import _lib
    bp, mg, big = _up(M + 1, 128), _up(M + 1, 64), 1e300
    ldg = mg + extra
    rs = np.random.RandomState(M + extra)
    G = rs.randint(-9, 10, size=(mg, ldg)).astype(float)
    G[G == 0.0] = 4.0                                      # (a zero would hide a wrongly read element of the upper triangle)
    ctx = _lib.Context()
    dG = torch.tensor(G, device="cuda")
    dB = torch.full((bp, bp), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.load().gpt_dev_sparse_assemble_b(ctx.handle, dG.data_ptr(), ldg, M, dB.data_ptr(), bp, big))
    ctx.synchronize()
    want = np.eye(bp)
    want[:M, :M] += np.tril(G[:M, :M])
    want[M, :M] = G[M, :M]
    want[M, M] = big
    assert np.array_equal(dB.cpu().numpy(), want)
    assert np.array_equal(dG.cpu().numpy(), G)
