"""Which calls GaussianProcess hands the library's context on each device route, and what it makes of the answers (no GPU,
no library): single fits, ll_batch (batched chunks, halving on MemoryError, a chunk the library rejects, the thread route),
compute_from_MCMC (batched chunks and the loop route), compute_Kij and the matrix route.

A recording stand-in replaces the contexts.  It appends every call to one shared log and answers with a simple function of what it
was handed -- ll = the sum of the element's kernel parameters + its noise variance, predictive mean = the element's sigma_f,
standard deviation = sigma_f too -- so an element that ends up in another element's place shows."""
import contextlib

import numpy as np
import pytest

import gptools_amd as g
from gptools_amd import _lib

import test_gibbs_gp_host as GH

SE, M52 = _lib.KERNEL_SE, _lib.KERNEL_M52
SIGMAS = [1.0, 1.25, 1.5, 1.75, 2.0, 2.25, 2.5]
EXCLUDED = 2                     # the vector with sigma_f = 1.5 has a length scale outside its bounds
N, M = 12, 5


def _norm_terms(terms):
    return tuple(tuple(tuple(float(v) for v in np.ravel(e)) if i % 2 else int(e) for i, e in enumerate(t)) for t in terms)


def _norm_layers(layers):
    return tuple((int(t), tuple(float(v) for v in np.ravel(p))) for t, p in (layers or []))


def _ll(terms, noise_var):
    return float(sum(sum(p) for t in _norm_terms(terms) for p in t[1::2]) + noise_var)


class _Recorder(object):
    """Stands in for ``_lib.Context``.  ``log`` is shared between the contexts of one test; entries are ``(op, context name,
    payload ...)``.  ``fit`` / ``fit_sum`` / ``fit_terms`` are the same event, carrying the model.  Told to fail by:
    ``mem_limit`` (fit_batch_terms raises MemoryError above that many elements), ``reject`` (a sigma_f at which the library raises
    ValueError, alone or anywhere in a chunk) and ``not_pd`` (a sigma_f whose batch element reports info = 1)."""

    def __init__(self, log, name="main", mem_limit=None, reject=None, not_pd=None):
        self.log, self.name, self.mem_limit, self.reject, self.not_pd = log, name, mem_limit, reject, not_pd
        self._warp_key = None
        self.batch = self.single = None

    # ---- state ------------------------------------------------------------------------------------------------------------
    def set_data(self, X, n):
        self._warp_key = None
        self.log.append(("set_data", self.name, np.shape(X)))

    def set_T(self, T):
        self.log.append(("set_T", self.name))

    def set_warp(self, layers):
        self._warp_key = _norm_layers(layers) or None
        self.log.append(("set_warp", self.name, _norm_layers(layers)))

    def set_warp_batch(self, layers_list):
        self.log.append(("set_warp_batch", self.name, tuple(_norm_layers(l) for l in layers_list)))

    def set_option(self, key, value):
        pass

    def mem_info(self):
        return (1 << 40, 1 << 40)

    def release_batch_scratch(self):
        self.log.append(("release", self.name))

    # ---- fits -------------------------------------------------------------------------------------------------------------
    def _fit(self, terms, noise_var, y):
        terms = _norm_terms(terms)
        self.log.append(("fit", self.name, terms, float(noise_var)))
        assert np.shape(y) == (N,)
        if terms[0][1][0] == self.reject:
            raise ValueError("the library rejects sigma_f = %r" % self.reject)
        self.single = terms[0][1][0]
        return _ll(terms, noise_var), 0.0

    def fit(self, kernel_id, params, noise_var, y, err_y, diag_add):
        return self._fit([(kernel_id, params)], noise_var, y)

    def fit_sum(self, kernel_ids, params_list, noise_var, y, err_y, diag_add):
        return self._fit(list(zip(kernel_ids, params_list)), noise_var, y)

    def fit_terms(self, terms, noise_var, y, err_y, diag_add):
        return self._fit(terms, noise_var, y)

    def fit_batch_terms(self, terms_list, noise_var, y, err_y, diag_add):
        sig = tuple(float(t[0][1][0]) for t in terms_list)
        self.log.append(("fit_batch", self.name, sig))
        assert np.shape(noise_var) == (len(sig),) and np.shape(y) == (len(sig), N)
        if self.mem_limit is not None and len(sig) > self.mem_limit:
            raise MemoryError("no room for %d elements" % len(sig))
        if self.reject in sig:
            raise ValueError("the library rejects sigma_f = %r" % self.reject)
        self.batch = np.array(sig)
        ll = np.array([_ll(t, v) for t, v in zip(terms_list, noise_var)])
        return ll, np.zeros(len(sig)), np.array([int(s == self.not_pd) for s in sig], dtype=np.int32)

    def fit_matrix(self, K_tot, y):
        self.log.append(("fit_matrix", self.name, np.shape(K_tot)))
        return float(np.trace(K_tot)), 0.0

    def get_alpha(self, Ny):
        return np.zeros(Ny)

    def cov_sample(self, diag_add, rand_vars):
        self.log.append(("cov_sample", self.name))
        return np.zeros(np.shape(rand_vars))

    # ---- predictions --------------------------------------------------------------------------------------------------------
    def predict_batch(self, Xs, ns, keep, noise_n=None, want_var=True, want_cov=False, want_cov_sum=False):
        keep = np.asarray(keep) != 0
        self.log.append(("predict_batch", self.name, tuple(int(v) for v in keep), None if noise_n is None else tuple(int(v) for v in noise_n)))
        assert len(keep) == len(self.batch)
        m = len(Xs)
        s = np.where(keep, self.batch, np.nan)
        cov = s[:, None, None] ** 2.0 * np.eye(m)[None]
        return (s[:, None] * np.ones((1, m)), s[:, None] ** 2.0 * np.ones((1, m)) if want_var else None,
                cov if want_cov else None, np.nansum(cov, axis=0) if want_cov_sum else None)

    def predict(self, Xs, ns, want, noise_params=None, noise_n=None, device_cov=False):
        noise = None if noise_params is None else (tuple(float(v) for v in noise_params), tuple(int(v) for v in noise_n))
        self.log.append(("predict", self.name, self.single, noise))
        m = len(Xs)
        return (self.single * np.ones(m), self.single * np.ones(m) if want >= 1 else None,
                self.single ** 2.0 * np.eye(m) if want == 2 else None)

    # ---- Gram blocks --------------------------------------------------------------------------------------------------------
    def _block(self, Xi, Xj, value):
        return np.full((len(Xi), len(Xi) if Xj is None else len(Xj)), value)

    def kbuild(self, kernel_id, params, Xi, ni, Xj=None, nj=None, hyper_deriv=None, noise_n=None):
        self.log.append(("kbuild", self.name, _norm_terms([(kernel_id, params)])[0], Xj is None))
        assert np.ndim(Xi) == 2 and np.shape(ni) == np.shape(Xi) and (Xj is None or (np.ndim(Xj) == 2 and np.shape(nj) == np.shape(Xj)))
        return self._block(Xi, Xj, float(np.sum(params)))

    def kbuild2(self, kid1, params1, kid2, params2, Xi, ni, Xj=None, nj=None):
        self.log.append(("kbuild2", self.name, _norm_terms([(kid1, params1, kid2, params2)])[0], Xj is None))
        assert np.ndim(Xi) == 2 and np.shape(ni) == np.shape(Xi) and (Xj is None or (np.ndim(Xj) == 2 and np.shape(nj) == np.shape(Xj)))
        return self._block(Xi, Xj, float(np.sum(params1) * np.sum(params2)))


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    """The thread route without the shared library; and nothing here may reach for the library's default context."""
    def refuse(*a, **kw):
        raise AssertionError("the library's default context was asked for")
    monkeypatch.setattr(_lib, "concurrent_evaluations", contextlib.nullcontext)
    monkeypatch.setattr(_lib, "default_context", refuse)


def _data(num_dim=1):
    rs = np.random.RandomState(5)
    X = np.sort(rs.uniform(0.05, 0.95, (N, num_dim)), axis=0)
    return X, np.sin(3.0 * X.sum(axis=1)), np.linspace(0.1, 0.9, M)


def _se(num_dim=1, p=(1.0, 0.5)):
    p = list(p) + [0.5] * (num_dim + 1 - len(p))
    return g.SquaredExponentialKernel(num_dim=num_dim, initial_params=p, param_bounds=[(0.01, 10.0)] * (num_dim + 1))


def _noise(num_dim=1):
    return g.DiagonalNoiseKernel(num_dim, initial_noise=0.1, noise_bound=(1e-3, 1.0))


def _gp(k=None, mu=None, **failures):
    """The fixture: N = 12 points in 1-D, squared exponential + diagonal noise, a main and one pooled recording context."""
    k = _se() if k is None else k
    X, y, Xs = _data(k.num_dim)
    gp = g.GaussianProcess(k, noise_k=_noise(k.num_dim), X=X, y=y, err_y=0.05, mu=mu)
    log = []
    gp._ctx_obj = _Recorder(log, "main", **failures)
    gp._ctx_pool = [[_Recorder(log, "pool", **failures), -1]]
    return gp, log, Xs


def _vectors(extra=()):
    """Seven vectors of free parameters (sigma_f, l_1, sigma_n, extra ...), all entries different; one outside the bounds."""
    vs = [np.array([s, 0.5 + 0.01 * i, 0.1 + 0.01 * i] + [e + 0.1 * i for e in extra]) for i, s in enumerate(SIGMAS)]
    vs[EXCLUDED][1] = 20.0
    return vs


def _want_ll(gp, vs):
    """Every entry its own element's answer plus its own log-prior; -inf where the prior excludes the vector."""
    want = np.array([v[0] + v[1] + v[2] ** 2.0 + gp.hyperprior(v) for v in vs])
    assert np.isinf(want[EXCLUDED]) and np.isfinite(np.delete(want, EXCLUDED)).all()
    return want


def _model(v):
    return (((SE, (float(v[0]), float(v[1]))),), float(v[2] ** 2.0))


NO_WARP = ("set_warp", "main", ())


# ---- ll_batch -----------------------------------------------------------------------------------------------------------------------
def test_ll_batch_chunks_of_three():
    gp, log, _ = _gp()
    vs, here = _vectors(), np.array(gp.free_params[:], dtype=float)
    gp.batch_grid = 3
    out = gp.ll_batch(vs)
    assert log == [("set_data", "main", (N, 1)),
                   NO_WARP, ("fit_batch", "main", (1.0, 1.25, 1.75)),
                   NO_WARP, ("fit_batch", "main", (2.0, 2.25, 2.5))]          # (the excluded vector is never sent)
    np.testing.assert_array_equal(out, _want_ll(gp, vs))
    np.testing.assert_array_equal(gp.free_params[:], here)
    assert gp._data_on_device is True


def test_ll_batch_halves_on_memory_error():
    gp, log, _ = _gp(mem_limit=2)
    vs = _vectors()
    gp.batch_grid = 8
    out = gp.ll_batch(vs)
    attempt = lambda *s: [NO_WARP, ("fit_batch", "main", s)]          # noqa: E731
    rel = [("release", "main")]
    assert log == ([("set_data", "main", (N, 1))] + attempt(1.0, 1.25, 1.75, 2.0, 2.25, 2.5) + rel + attempt(1.0, 1.25, 1.75, 2.0) + rel
                   + attempt(1.0, 1.25) + attempt(1.75, 2.0) + attempt(2.25, 2.5))
    np.testing.assert_array_equal(out, _want_ll(gp, vs))


def test_ll_batch_no_chunk_fits_thread_route():
    gp, log, _ = _gp(mem_limit=0)
    vs = _vectors()
    gp.batch_grid = 4
    out = gp.ll_batch(vs)
    head = [("set_data", "main", (N, 1))]
    for s in ((1.0, 1.25, 1.75, 2.0), (1.0, 1.25), (1.0,)):
        head += [NO_WARP, ("fit_batch", "main", s), ("release", "main")]
    assert log[:len(head)] == head
    assert log[len(head)] == ("set_data", "pool", (N, 1))
    tail = log[len(head) + 1:]
    # which context ran which vector is a race between two host threads: per context set_warp + one fit each, together all six
    for name in ("main", "pool"):
        mine = [e for e in tail if e[1] == name]
        assert [e[0] for e in mine] == ["set_warp", "fit"] * (len(mine) // 2) and all(e[2] == () for e in mine[0::2])
    assert sorted(e[2:] for e in tail if e[0] == "fit") == sorted(_model(v) for i, v in enumerate(vs) if i != EXCLUDED)
    assert len(tail) == 12
    np.testing.assert_array_equal(out, _want_ll(gp, vs))


def test_ll_batch_rejected_chunk_one_by_one():
    gp, log, _ = _gp(reject=1.75)
    vs = _vectors()
    gp.batch_grid = 3
    out = gp.ll_batch(vs)
    want = [("set_data", "main", (N, 1)), NO_WARP, ("fit_batch", "main", (1.0, 1.25, 1.75))]
    for i in (0, 1, 3):
        want += [NO_WARP, ("fit", "main") + _model(vs[i])]
    want += [NO_WARP, ("fit_batch", "main", (2.0, 2.25, 2.5))]
    assert log == want
    ll = _want_ll(gp, vs)
    ll[3] = -np.inf
    np.testing.assert_array_equal(out, ll)


def test_ll_batch_warped_model_gets_layers_per_element():
    gp, log, _ = _gp(k=g.BetaWarpedKernel(_se()))
    vs = [np.array([s, 0.5, 1.0 + 0.1 * i, 2.0 + 0.1 * i, 0.1]) for i, s in enumerate(SIGMAS[:4])]
    gp.batch_grid = 3
    out = gp.ll_batch(vs)
    lay = lambda i: ((_lib.WARP_BETA, (1.0 + 0.1 * i, 2.0 + 0.1 * i)),)          # noqa: E731
    assert log == [("set_data", "main", (N, 1)),
                   ("set_warp_batch", "main", (lay(0), lay(1), lay(2))), ("fit_batch", "main", (1.0, 1.25, 1.5)),
                   ("set_warp_batch", "main", (lay(3),)), ("fit_batch", "main", (1.75,))]
    np.testing.assert_array_equal(out, [v[0] + v[1] + v[4] ** 2.0 + gp.hyperprior(v) for v in vs])


# ---- compute_from_MCMC --------------------------------------------------------------------------------------------------------------
def _mcmc(gp, Xs, vs, **kw):
    gp.batch_grid = 3
    here = np.array(gp.free_params[:], dtype=float)
    out = gp.compute_from_MCMC(Xs, flat_trace=np.array(vs), return_std=True, **kw)
    np.testing.assert_array_equal(gp.free_params[:], here)
    return out


def _assert_rows(out, sigmas, shift=None):
    """Mean = the row's sigma_f (+ its mean function), std = sigma_f, for exactly these rows in this order."""
    assert len(out["mean"]) == len(out["std"]) == len(sigmas)
    for q, s in enumerate(sigmas):
        np.testing.assert_array_equal(out["mean"][q], np.full(M, s if shift is None else s + shift[q]))
        np.testing.assert_array_equal(out["std"][q], np.full(M, s))


def _batched(sig, keep=None, noise_n=None):
    return [("fit_batch", "main", tuple(sig)), ("predict_batch", "main", tuple(keep or [1] * len(sig)), noise_n)]


def _looped(v, predicted=True):
    return [("set_warp", "main", ()), ("fit", "main") + _model(v)] + ([("predict", "main", float(v[0]), None)] if predicted else [])


def _no_unwarp(log):
    """The log without the calls that clear the warp in front of an unwarped batch (``Context.set_warp`` returns before the
    library when the layers are the ones it holds: such a call changes nothing)."""
    return [e for i, e in enumerate(log) if not (e == NO_WARP and i + 1 < len(log) and log[i + 1][0] == "fit_batch")]


def test_mcmc_element_not_positive_definite_is_dropped():
    gp, log, Xs = _gp(not_pd=1.25)
    vs = _vectors()
    out = _mcmc(gp, Xs, vs)
    # (the MCMC route evaluates the vector the prior excludes, unlike ll_batch)
    assert _no_unwarp(log) == ([("set_data", "main", (N, 1))] + _batched(SIGMAS[0:3], (1, 0, 1)) + _batched(SIGMAS[3:6])
                               + _batched(SIGMAS[6:]))
    _assert_rows(out, [s for s in SIGMAS if s != 1.25])


def test_mcmc_rejected_chunk_goes_to_the_loop_route():
    gp, log, Xs = _gp(reject=1.75)
    vs = _vectors()
    out = _mcmc(gp, Xs, vs)
    # the row the library rejects: update_hyperparameters counts it as +inf, predict refits and raises, the row is dropped
    assert _no_unwarp(log) == ([("set_data", "main", (N, 1))] + _batched(SIGMAS[0:3]) + [("fit_batch", "main", tuple(SIGMAS[3:6]))]
                               + _batched(SIGMAS[6:]) + _looped(vs[3], False) + _looped(vs[3], False) + _looped(vs[4]) + _looped(vs[5]))
    _assert_rows(out, [s for s in SIGMAS if s != 1.75])


def test_mcmc_halves_on_memory_error():
    gp, log, Xs = _gp(mem_limit=1)
    vs = _vectors()
    out = _mcmc(gp, Xs, vs)
    want = [("set_data", "main", (N, 1)), ("fit_batch", "main", tuple(SIGMAS[0:3])), ("release", "main")]
    for s in SIGMAS:
        want += _batched([s])
    assert _no_unwarp(log) == want
    _assert_rows(out, SIGMAS)


def test_mcmc_no_chunk_fits_loop_route():
    gp, log, Xs = _gp(mem_limit=0)
    vs = _vectors()
    out = _mcmc(gp, Xs, vs)
    want = [("set_data", "main", (N, 1)), ("fit_batch", "main", tuple(SIGMAS[0:3])), ("release", "main"),
            ("fit_batch", "main", (1.0,)), ("release", "main")]
    for v in vs:
        want += _looped(v)
    assert _no_unwarp(log) == want
    _assert_rows(out, SIGMAS)


def test_mcmc_mean_function_per_row():
    mu = g.ConstantMeanFunction(initial_params=[0.3], param_bounds=[(-5.0, 5.0)])
    gp, log, Xs = _gp(mu=mu)
    vs = _vectors(extra=(0.3,))
    out = _mcmc(gp, Xs, vs, return_mean_func=True)
    assert _no_unwarp(log) == ([("set_data", "main", (N, 1))] + _batched(SIGMAS[0:3]) + _batched(SIGMAS[3:6]) + _batched(SIGMAS[6:]))
    shift = [v[3] for v in vs]
    _assert_rows(out, SIGMAS, shift)
    for q, s in enumerate(SIGMAS):
        np.testing.assert_array_equal(out["mean_func"][q], np.full(M, shift[q]))
        np.testing.assert_array_equal(out["mean_without_func"][q], np.full(M, s + shift[q]) - shift[q])
        np.testing.assert_array_equal(out["cov_without_func"][q], s ** 2.0 * np.eye(M))


def test_mcmc_every_row_fails_to_solve():
    """Every row has x_2 = x_3: no row's device parameters solve, so there is no job at all -- the documented ValueError."""
    gp, base, rows = GH._gp_and_rows()
    for r in rows:
        r[3] = r[4]
    with pytest.raises(ValueError, match="every row of the hyperparameter trace failed"):
        gp.compute_from_MCMC(np.linspace(0.1, 1.9, 7), flat_trace=np.array(rows), return_std=True)
    assert gp._ctx.batches == []
    np.testing.assert_array_equal(gp.free_params[:], base)


# ---- single fits ----------------------------------------------------------------------------------------------------------------------
def _m52():
    return g.Matern52Kernel(num_dim=1, initial_params=[0.7, 0.3], param_bounds=[(0.01, 10.0)] * 2)


@pytest.mark.parametrize("model", ["se", "sum", "product"])
def test_update_hyperparameters_uploads_once_and_fits_the_model(model):
    k = {"se": _se, "sum": lambda: _se() + _m52(), "product": lambda: _se() * _m52()}[model]()
    gp, log, _ = _gp(k=k)
    tail = [] if model == "se" else [0.7, 0.3]
    want = [("set_data", "main", (N, 1))]
    for s in (1.25, 1.5):
        p = [s, 0.4] + tail + [0.2]
        val = gp.update_hyperparameters(p)
        terms = {"se": ((SE, (s, 0.4)),), "sum": ((SE, (s, 0.4)), (M52, (0.7, 0.3))), "product": ((SE, (s, 0.4), M52, (0.7, 0.3)),)}[model]
        want += [NO_WARP, ("fit", "main", terms, 0.2 ** 2.0)]
        assert val == -(_ll(terms, 0.2 ** 2.0) + gp.hyperprior(np.array(p)))
        assert gp._fit_mode == "kernel" and gp._data_on_device is True
    assert log == want


def test_python_defined_kernel_takes_the_matrix_route():
    class PySE(g.SquaredExponentialKernel):
        def __call__(self, Xi, Xj, ni, nj, hyper_deriv=None, symmetric=False):
            d = np.asarray(Xi, dtype=float)[:, 0] - np.asarray(Xj, dtype=float)[:, 0]
            return self.params[0] ** 2.0 * np.exp(-d ** 2.0 / (2.0 * self.params[1] ** 2.0))
    gp, log, _ = _gp(k=PySE(num_dim=1, initial_params=[1.0, 0.5], param_bounds=[(0.01, 10.0)] * 2))
    assert gp._device_model() is None and not gp._fast_fit_possible()
    val = gp.update_hyperparameters([1.5, 0.4, 0.2])
    assert log == [("fit_matrix", "main", (N, N))]
    assert gp._fit_mode == "matrix" and gp._data_on_device is False
    d = gp.X[:, 0][:, None] - gp.X[:, 0][None, :]
    K_tot = 1.5 ** 2.0 * np.exp(-d ** 2.0 / (2.0 * 0.4 ** 2.0)) + (0.2 ** 2.0 + 0.05 ** 2.0 + gp.diag_factor * np.finfo(float).eps) * np.eye(N)
    np.testing.assert_allclose(-val, np.trace(K_tot) + gp.hyperprior(gp.params), rtol=1e-14)


def test_noisy_predictions_carry_the_noise_kernel():
    """predict, draw_sample's device route and the batched MCMC route hand over the noise kernel's parameter and orders when asked
    for a noisy prediction -- and nothing otherwise."""
    gp, log, Xs = _gp()
    gp.update_hyperparameters([1.5, 0.4, 0.2])
    del log[:]
    gp.predict(Xs, noise=True)
    gp.predict(Xs)
    gp.draw_sample(Xs, rand_vars=np.zeros((M, 2)), noise=True)
    gp.draw_sample(Xs, rand_vars=np.zeros((M, 2)))
    noisy = ((0.2,), (0,))
    assert log == [("predict", "main", 1.5, noisy), ("predict", "main", 1.5, None),
                   ("predict", "main", 1.5, noisy), ("cov_sample", "main"), ("predict", "main", 1.5, None), ("cov_sample", "main")]
    del log[:]
    _mcmc(gp, Xs, _vectors()[:3], noise=True)
    assert _no_unwarp(log) == _batched(SIGMAS[:3], noise_n=(0,))


# ---- compute_Kij ----------------------------------------------------------------------------------------------------------------------
def test_compute_kij_own_warped_model():
    gp, log, Xs = _gp(k=g.BetaWarpedKernel(_se() + _m52(), initial_params=[1.5, 2.5]))
    lay = ((_lib.WARP_BETA, (1.5, 2.5)),)
    K = gp.compute_Kij(Xs[:, None], None, np.zeros((M, 1), dtype=int), None)
    assert log == [("set_data", "main", (N, 1)), ("set_warp", "main", lay),
                   ("kbuild", "main", (SE, (1.0, 0.5)), True), ("kbuild", "main", (M52, (0.7, 0.3)), True)]
    np.testing.assert_array_equal(K, np.full((M, M), 1.5 + 1.0))          # one block per term, summed
    del log[:]
    K = gp.compute_Kij(Xs[:, None], gp.X, np.zeros((M, 1), dtype=int), gp.n)
    assert log == [("set_warp", "main", lay), ("kbuild", "main", (SE, (1.0, 0.5)), False), ("kbuild", "main", (M52, (0.7, 0.3)), False)]
    np.testing.assert_array_equal(K, np.full((M, N), 1.5 + 1.0))


def test_compute_kij_product_and_masked_kernels():
    gp, log, _ = _gp(k=_se(2))
    Xi, ni = np.random.RandomState(1).rand(M, 2), np.zeros((M, 2), dtype=int)
    prod = _se(2, (1.0, 0.5, 0.25)) * g.Matern52Kernel(num_dim=2, initial_params=[0.7, 0.3, 0.2], param_bounds=[(0.01, 10.0)] * 3)
    K = gp.compute_Kij(Xi, None, ni, None, k=prod)
    assert log == [("kbuild2", "main", (SE, (1.0, 0.5, 0.25), M52, (0.7, 0.3, 0.2)), True)]
    np.testing.assert_array_equal(K, np.full((M, M), 1.75 * (0.7 + 0.3 + 0.2)))
    # a masked stationary kernel is one native term (infinite length scales outside its mask) ...
    del log[:]
    K = gp.compute_Kij(Xi, gp.X, ni, gp.n, k=g.MaskedKernel(_se(), total_dim=2, mask=[1]))
    assert log == [("kbuild", "main", (SE, (1.0, np.inf, 0.5)), False)]
    assert K.shape == (M, N) and np.isinf(K).all()
    # ... a masked Gibbs kernel a product with the unit factor
    del log[:]
    tanh = g.GibbsKernel1dTanh(initial_params=[1.0, 0.5, 0.25, 0.125, 0.5], param_bounds=[(0.01, 10.0)] * 5)
    K = gp.compute_Kij(Xi, None, ni, None, k=g.MaskedKernel(tanh, total_dim=2, mask=[1]))
    kid = _lib.kernel_on_dim(_lib.KERNEL_GIBBS_TANH, 1)
    assert log == [("kbuild2", "main", (kid, (1.0, 0.5, 0.25, 0.125, 0.5), SE, (1.0, np.inf, np.inf)), True)]
    assert K.shape == (M, M)
