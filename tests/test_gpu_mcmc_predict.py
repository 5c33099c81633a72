"""GPU suite: predictions marginalised over a trace of hyperparameters -- GaussianProcess.compute_from_MCMC / predict_MCMC /
predict(use_MCMC=True) against the reference's (tests/golden/g14_mcmc.npz), the batched device route (gpt_fit_batch_terms +
gpt_predict_batch) against the loop route and against gpt_fit_terms + gpt_predict per element."""
import sys

import numpy as np
import pytest
import scipy.linalg

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import gen_g14_mcmc as G14      # noqa: E402

pytestmark = pytest.mark.gpu
SF2 = 3.0                        # bound on sigma_f^2 over the fixture traces: the tolerances are absolute, relative to it


def _case(golden, name):
    g = golden("g14_mcmc")
    d = {k.split("__", 1)[1]: v for k, v in g.items() if k.startswith(name + "__") and k.count("__") == 1}
    res = {}
    for k, v in g.items():
        parts = k.split("__")
        if parts[0] == name and len(parts) == 3:
            res.setdefault(parts[1], {})[parts[2]] = v
    return d, res


def _cmp(got, want, tol, msg):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (msg, got.shape, want.shape)
    np.testing.assert_allclose(got, want, rtol=0, atol=tol, err_msg=msg)


def _cmp_result(got, want, tol, msg):
    if isinstance(got, tuple):
        got = dict(zip(("mean", "second"), got))
    assert set(want) <= set(got), (msg, sorted(got), sorted(want))
    for key, w in want.items():
        g = np.asarray(got[key], dtype=float)
        if key.startswith("std") or key == "second":         # (compare variances: sqrt amplifies rounding where std is small)
            _cmp(g ** 2, w ** 2, tol, "%s %s" % (msg, key))
        else:
            _cmp(g, w, tol, "%s %s" % (msg, key))


@pytest.mark.parametrize("name", G14.CASES)
def test_fixture_cases_match_reference(golden, name):
    import gptools_amd as g
    d, res = _case(golden, name)
    for call, meth, kw in G14.CALLS[name]:
        gp = G14.make_gp(g, name, d)
        before = np.array(gp.free_params[:], dtype=float)
        got = getattr(gp, meth)(d["Xs"], **G14.call_kwargs(d, kw))
        _cmp_result(got, res[call], 1e-9 * SF2, "%s/%s" % (name, call))
        if meth == "compute_from_MCMC" and "cov_func" in got:
            # (the fixture stores only the independent keys: per row the reference's cov_func is zero, cov_without_func = cov)
            assert not np.any(np.array(got["cov_func"]))
            np.testing.assert_array_equal(np.array(got["cov_without_func"]), np.array(got["cov"]))
        np.testing.assert_array_equal(np.array(gp.free_params[:], dtype=float), before)      # (8) unchanged afterwards


@pytest.mark.parametrize("name,call", [("se1", "pm_cov0_noise"), ("se1", "cfm"), ("mu", "cfm"), ("sum", "pm_cov1"),
                                       ("m52d", "cfm"), ("ot", "pm_std")])
def test_batched_route_matches_loop_route(golden, name, call):
    import gptools_amd as g
    d, _ = _case(golden, name)
    meth, kw = next((c[1], c[2]) for c in G14.CALLS[name] if c[0] == call)
    gp = G14.make_gp(g, name, d)
    batched = getattr(gp, meth)(d["Xs"], **G14.call_kwargs(d, kw))
    gp.batch_grid_max_n = 0                                    # forces the loop route
    loop = getattr(gp, meth)(d["Xs"], **G14.call_kwargs(d, kw))
    for key in loop:
        _cmp(batched[key], loop[key], 1e-10 * SF2, "%s/%s %s" % (name, call, key))


def test_chunking_gives_the_same_results(golden):
    import gptools_amd as g
    d, _ = _case(golden, "se1")
    kw = G14.call_kwargs(d, dict(return_cov=True))
    kw["flat_trace"] = d["trace"][:23]
    gp = G14.make_gp(g, "se1", d)
    one = gp.predict_MCMC(d["Xs"], **kw)
    rows_one = gp.compute_from_MCMC(d["Xs"], return_cov=True, **{k: v for k, v in kw.items() if k != "return_cov"})
    gp.batch_grid = 5
    five = gp.predict_MCMC(d["Xs"], **kw)
    rows_five = gp.compute_from_MCMC(d["Xs"], return_cov=True, **{k: v for k, v in kw.items() if k != "return_cov"})
    for key in one:
        _cmp(five[key], one[key], 1e-12 * SF2, "chunked " + key)
    for key in rows_one:
        _cmp(np.array(rows_five[key]), np.array(rows_one[key]), 1e-12 * SF2, "chunked rows " + key)


def _abi_setup(terms_of, rows, D=1, N=60, M=33, seed=11):
    from gptools_amd import _lib
    rs = np.random.RandomState(seed)
    X = rs.uniform(0.0, 5.0, (N, D))
    n = np.zeros((N, D), dtype=np.int32)
    n[-5:, 0] = 1
    Xs = rs.uniform(-0.5, 5.5, (M, D))
    ns = np.zeros((M, D), dtype=np.int32)
    ns[:4, 0] = 1
    y = np.sin(X.sum(axis=1)) + 0.05 * rs.randn(N)
    err_y = np.full(N, 0.03)
    ctx = _lib.Context()
    ctx.set_data(X, n)
    terms = [terms_of(p) for p in rows]
    nv = np.array([p[-1] ** 2 for p in rows])
    Y = np.array([y - 0.1 * b for b in range(len(rows))])
    return ctx, X, n, Xs, ns, Y, err_y, terms, nv


@pytest.mark.parametrize("model", ["se", "sum", "product"])
def test_cabi_predict_batch_matches_fit_and_predict_per_element(model):
    from gptools_amd import _lib
    SE, M52 = _lib.KERNEL_SE, _lib.KERNEL_M52
    if model == "se":
        terms_of = lambda p: [(SE, np.array(p[:2]))]                                   # noqa: E731
        rows = [[1.0, 0.8, 0.1], [1.4, 1.2, 0.05], [0.6, 400.0, 0.0], [1.1, 0.5, 0.2], [0.9, 1.0, 0.1], [1.2, 0.7, 0.02]]
    elif model == "sum":
        terms_of = lambda p: [(SE, np.array(p[:2])), (M52, np.array(p[2:4]))]          # noqa: E731
        rows = [[1.0, 0.8, 0.3, 2.0, 0.1], [1.3, 1.1, 0.5, 1.5, 0.05], [0.8, 0.6, 0.2, 3.0, 0.03]]
    else:
        terms_of = lambda p: [(SE, np.array(p[:2]), SE, np.array(p[2:4]))]            # noqa: E731
        rows = [[1.0, 0.8, 1.0, 3.0, 0.1], [1.3, 1.1, 0.7, 2.0, 0.05]]
    ctx, X, n, Xs, ns, Y, err_y, terms, nv = _abi_setup(terms_of, rows)
    diag_add = 0.0
    err_y = np.zeros_like(err_y)              # (no loading: the noise-free element with l = 400 is singular, skipped)
    _, _, info = ctx.fit_batch_terms(terms, nv, Y, err_y, diag_add)
    keep = info == 0
    assert keep.sum() >= 2
    if model == "se":
        assert not keep[2]
    noise_n = np.zeros(1, dtype=np.int32)
    mean, var, cov, cov_sum = ctx.predict_batch(Xs, ns, keep, noise_n, True, True, True)
    single = _lib.Context()
    single.set_data(X, n)
    total = np.zeros_like(cov_sum)
    for b, p in enumerate(rows):
        try:
            single.fit_terms(terms[b], nv[b], Y[b], err_y, diag_add)
            fitted = True
        except np.linalg.LinAlgError:
            fitted = False
        assert fitted == bool(keep[b]), "element %d: gpt_fit says %s, info %d" % (b, fitted, info[b])
        if not fitted:
            assert np.isnan(mean[b]).all()                     # (skipped: not written)
            continue
        m1, s1, c1 = single.predict(Xs, ns, 2, noise_params=[p[-1]], noise_n=noise_n)
        tol = 1e-10 * max(1.0, p[0] ** 2)
        _cmp(mean[b], m1, tol, "mean %d" % b)
        _cmp(var[b], s1 ** 2, tol, "var %d" % b)
        _cmp(cov[b], c1, tol, "cov %d" % b)
        total += cov[b]
    _cmp(cov_sum, total, 1e-10 * SF2 * len(rows), "cov_sum")


def test_cabi_predict_batch_state_and_transform_errors():
    from gptools_amd import _lib
    SE = _lib.KERNEL_SE
    rows = [[1.0, 0.8, 0.1], [1.2, 1.0, 0.1]]
    ctx, X, n, Xs, ns, Y, err_y, terms, nv = _abi_setup(lambda p: [(SE, np.array(p[:2]))], rows)
    diag_add = 1e2 * np.finfo(float).eps
    keep = np.ones(2, dtype=np.int32)
    with pytest.raises(_lib.GPTBackendError):                  # no batch resident yet
        ctx.predict_batch(Xs, ns, keep)
    ctx.fit_batch_terms(terms, nv, Y, err_y, diag_add)
    ctx.predict_batch(Xs, ns, keep)                            # resident
    ctx.fit(SE, np.array(rows[0][:2]), nv[0], Y[0], err_y, diag_add)
    ctx.predict(Xs, ns, 2, device_cov=True)
    ctx.cov_sample(1e-10, np.random.RandomState(0).randn(Xs.shape[0], 2))
    with pytest.raises(_lib.GPTBackendError):                  # gpt_cov_sample reused the batch's workspace
        ctx.predict_batch(Xs, ns, keep)
    ctx.fit_batch_terms(terms, nv, Y, err_y, diag_add)
    ctx.predict_batch(Xs, ns, keep)
    ctx.release_batch_scratch()
    with pytest.raises(_lib.GPTBackendError):
        ctx.predict_batch(Xs, ns, keep)
    ctx.set_T(np.eye(X.shape[0])[::2])
    ctx.fit_batch_terms(terms, nv, Y[:, ::2], err_y[::2], diag_add)
    with pytest.raises(NotImplementedError):
        ctx.predict_batch(Xs, ns, keep)


def test_mid_size_against_oracle_composition(oracle):
    import gptools_amd as g
    rs = np.random.RandomState(5)
    N, M, S = 2048, 512, 16
    X = rs.uniform(-3.0, 3.0, (N, 2))
    n = np.zeros((N, 2), dtype=int)
    n[1800:1900, 0] = 1
    n[1900:, 1] = 1
    y = np.sin(X[:, 0]) * np.cos(0.5 * X[:, 1]) + 0.02 * rs.randn(N)
    Xs = rs.uniform(-3.0, 3.0, (M, 2))
    ns = np.zeros((M, 2), dtype=int)
    ns[400:450, 0] = 1
    trace = np.column_stack([rs.uniform(0.8, 1.4, S), rs.uniform(0.9, 1.5, S), rs.uniform(0.9, 1.5, S)])
    gp = g.GaussianProcess(g.SquaredExponentialKernel(num_dim=2, initial_params=[1.0, 1.0, 1.0], param_bounds=[(1e-3, 10.0)] * 3))
    gp.add_data(X, y, err_y=0.05, n=n)
    got = gp.predict_MCMC(Xs, n=ns, flat_trace=trace, return_cov=True)
    means, covs = [], []
    for p in trace:
        f = oracle.fit("se", p, X, n, y, np.full(N, 0.05), chol="scipy")
        Ks = oracle.kbuild("se", p, Xs, ns, X, n)                      # (M, N)
        v = scipy.linalg.solve_triangular(f["L"], Ks.T, lower=True)
        means.append(Ks.dot(f["alpha"]))
        covs.append(oracle.kbuild("se", p, Xs, ns) - v.T.dot(v))
    means, covs = np.array(means), np.array(covs)
    cov = np.mean(covs, axis=0) + np.cov(means, rowvar=0, ddof=1)
    _cmp(got["mean"], np.mean(means, axis=0), 1e-8 * SF2, "mean")
    _cmp(got["cov"], cov, 1e-8 * SF2, "cov")


def test_full_mc_rejection_and_samples(golden):
    import gptools_amd as g
    d, _ = _case(golden, "se1")
    gp = G14.make_gp(g, "se1", d)
    before = np.array(gp.free_params[:], dtype=float)
    kw = dict(n=d["ns"], flat_trace=d["trace"])
    rows = gp.compute_from_MCMC(d["Xs"], return_cov=True, **kw)
    K, M = len(rows["mean"]), d["Xs"].shape[0]
    np.random.seed(7)
    res = gp.predict_MCMC(d["Xs"], full_MC=True, num_samples=3, return_cov=True, **kw)
    np.random.seed(7)
    host = np.hstack([np.random.multivariate_normal(m, c, 3).T for m, c in zip(rows["mean"], rows["cov"])])
    assert res["samp"].shape == (M, 3 * K)
    _cmp(res["samp"], host, 1e-9, "samples")
    _cmp(res["mean"], np.mean(host, axis=1), 1e-9, "full_MC mean")
    _cmp(res["cov"], np.cov(host, rowvar=1, ddof=1), 1e-9, "full_MC cov")
    rule = lambda s: s[0] > np.median(host[0])                 # noqa: E731
    np.random.seed(7)
    rej = gp.predict_MCMC(d["Xs"], full_MC=True, num_samples=3, rejection_func=rule, **kw)
    assert rej["samp"].shape == (M, sum(rule(s) for s in host.T))
    np.random.seed(3)
    out = gp.compute_from_MCMC(d["Xs"], return_samples=True, num_samples=2, **kw)
    assert len(out["samp"]) == K and all(s.shape == (M, 2) for s in out["samp"])
    np.random.seed(3)
    pr = gp.predict(d["Xs"], n=d["ns"], use_MCMC=True, full_output=True, return_samples=True, num_samples=2,
                    flat_trace=d["trace"])
    assert pr["samp"].shape == (M, 2 * K)
    np.testing.assert_array_equal(pr["samp"], np.hstack(out["samp"]))
    np.testing.assert_array_equal(np.array(gp.free_params[:], dtype=float), before)


def test_without_trace_or_sampler_names_flat_trace():
    import gptools_amd as g
    gp = g.GaussianProcess(g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 1.0]))
    gp.add_data(np.linspace(0, 1, 10), np.sin(np.linspace(0, 1, 10)))
    with pytest.raises(NotImplementedError, match="flat_trace"):
        gp.predict_MCMC(np.linspace(0, 1, 5))


def test_sampler_chain_is_burned_thinned_and_flattened(golden):
    import gptools_amd as g
    d, _ = _case(golden, "se1")
    gp = G14.make_gp(g, "se1", d)

    class Chain(object):
        chain = d["trace"].reshape(2, 12, 3)
    a = gp.compute_from_MCMC(d["Xs"], n=d["ns"], sampler=Chain(), burn=2, thin=2)
    flat = d["trace"].reshape(2, 12, 3)[:, 2::2, :].reshape(-1, 3)
    b = gp.compute_from_MCMC(d["Xs"], n=d["ns"], flat_trace=flat)
    _cmp(np.array(a["mean"]), np.array(b["mean"]), 0.0, "sampler chain")
