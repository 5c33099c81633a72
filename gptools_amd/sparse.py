"""SparseGaussianProcess: inducing-point approximations (FITC, VFE, DTC) of the GP on the GPU.

The same kernel, hyperparameters, priors and ``predict`` as :class:`GaussianProcess`, with ``M`` inducing inputs ``Z`` in place of
the ``N x N`` covariance: ``O(N M^2)`` time and ``O(M^2 + chunk M)`` device memory (``gpt_sparse_fit`` / ``gpt_sparse_predict``,
include/gpt_hip.h).  With ``s_i = sigma_noise^2 + err_y_i^2`` and ``jitter`` on the diagonal of ``K_uu``::

    L_u = chol(k(Z,Z) + jitter I)      V = L_u^-1 k(Z,X)      q_i = sum_m V_mi^2      k_i = k(x_i,x_i)
    Lambda_i = k_i - q_i + s_i (fitc)  Lambda_i = s_i (vfe, dtc)
    B = I + V Lambda^-1 V^T            L_B = chol(B)          c = L_B^-1 V Lambda^-1 r         r = y - mu(X)
    ll = -1/2 [sum log Lambda_i + 2 sum log (L_B)_mm + r^T Lambda^-1 r - c.c + N log 2 pi]  - 1/2 sum (k_i - q_i)/s_i (vfe only)

What the dense class offers beyond value, optimisation over the value and prediction is refused here, never routed to the dense
path: see the class docstring.
"""
import traceback
import warnings

import numpy as np

from . import _lib, _ingest
from .error_handling import GPArgumentError
from .gaussian_process import GaussianProcess, _BatchJob, _terms_shape
from .kernel import ZeroKernel, DiagonalNoiseKernel

__all__ = ["SparseGaussianProcess", "greedy_inducing"]


def _device_terms(gp):
    """The terms of ``gp``'s covariance kernel as the library takes them (:meth:`GaussianProcess._device_model`); raises for a
    kernel the sparse path does not take: the class and :func:`greedy_inducing` resolve, and refuse, through this."""
    model = gp._device_model()
    if model is None:
        raise NotImplementedError("the covariance kernel is not one the library evaluates itself (a Python-defined kernel, or "
                                  "a tree of kernels it does not take): SparseGaussianProcess has no host route")
    terms, layers = model
    if layers:
        raise NotImplementedError("SparseGaussianProcess does not take warped kernels (WarpedKernel)")
    return terms


def _greedy_select(ctx, terms, X, n, M, candidates, max_candidates, seed, tol):
    """Greedy conditional-variance selection on a context that holds ``X`` and ``n`` (``gpt_sparse_select_inducing``): resolves the
    candidate rows, returns ``(Z, info)`` and warns if the stop rule ended the selection early."""
    M = int(M)
    cand = None
    if candidates is not None:
        if max_candidates is not None:
            raise ValueError("pass candidates or max_candidates, not both")
        cand = np.asarray(candidates)
        if cand.ndim != 1 or cand.size < 1 or not np.issubdtype(cand.dtype, np.integer):
            raise ValueError("candidates must be a non-empty vector of row indices")
        cand = np.sort(cand.astype(np.int64))
        if np.any(cand[1:] == cand[:-1]):
            raise ValueError("candidates holds a row more than once")
        if cand[0] < 0 or cand[-1] >= X.shape[0]:
            raise ValueError("candidates must lie within [0, %d)" % X.shape[0])
    elif max_candidates is not None:
        if int(max_candidates) != max_candidates or max_candidates < 1:
            raise ValueError("max_candidates must be a positive integer, got %r" % (max_candidates,))
        pool = np.flatnonzero(np.all(np.asarray(n) == 0, axis=1))
        if int(max_candidates) < pool.size:
            cand = np.sort(np.random.RandomState(seed).choice(pool, int(max_candidates), replace=False))
    indices, dmax, trace = ctx.sparse_select_inducing(terms, M, cand, tol)
    if len(indices) < M:
        warnings.warn("greedy selection stopped after %d of %d inducing inputs: the largest remaining conditional variance is not "
                      "above tol = %g times the first (%.3g), or not a positive finite number; the remaining trace is %.3g"
                      % (len(indices), M, tol, dmax[0], trace[-1]), RuntimeWarning)
    return np.array(X[indices], dtype=float), {"indices": indices, "dmax": dmax, "trace": trace}


def greedy_inducing(k, X, M, n=0, candidates=None, max_candidates=None, seed=0, tol=0.0, device=0):
    """Choose ``M`` inducing inputs among the rows of ``X`` by greedy conditional-variance selection (the partial pivoted Cholesky of
    ``K_ff``) on the GPU: each step adds the row whose variance, conditioned on the rows chosen so far, is
    largest (ties: the lowest row; for a stationary kernel the first pivot is therefore the lowest candidate).  It needs no ``y``, no
    noise level and no optimiser, costs ``O(N M^2)`` and holds an ``N x M`` factor on the device.

    ``k``: a covariance kernel :class:`SparseGaussianProcess` takes (resolved and refused as there), at its current parameters.
    ``n``: the derivative orders of ``X``; only rows whose orders are all zero are candidates.  ``candidates``: row indices to choose
    among (sorted here; duplicates are refused).  ``max_candidates``: choose among a seeded (``seed``) subsample without replacement
    of that many order-zero rows -- for data whose ``N x M`` factor would not fit.  ``tol``: stop once the largest remaining
    conditional variance is at most ``tol`` times the first (a warning; fewer than ``M`` rows come back).

    Returns ``(Z, info)``: ``Z = X[info["indices"]]``; ``info["dmax"][j]`` the conditional variance of pivot ``j`` when it was chosen;
    ``info["trace"][j]`` the sum of the candidates' conditional variances after ``j`` pivots (length ``count + 1``) -- the quantity
    the VFE objective penalises, ``tr(K_ff - K_fu K_uu^-1 K_uf)``: it tells how large ``M`` must be."""
    probe = GaussianProcess(k, device=device)
    terms = _device_terms(probe)
    X = _ingest.points(X, probe.num_dim)
    n = _ingest.derivative_orders(n, X, probe.num_dim, column_rule="not-column")
    ctx = _lib.Context(device)
    try:
        ctx.set_data(X, n)
        return _greedy_select(ctx, terms, X, n, M, candidates, max_candidates, seed, tol)
    finally:
        ctx.close()


class SparseGaussianProcess(GaussianProcess):
    """Gaussian process regression through ``M`` inducing inputs.

    ``k``, ``noise_k``, ``X``, ``y``, ``err_y``, ``n``, ``mu``, ``diag_factor``, ``verbose``, ``device`` as
    :class:`GaussianProcess`.  ``Z`` (M, D): the inducing inputs, ``n_Z`` their derivative orders (scalar or (M, D)); they are
    not hyperparameters: :meth:`set_inducing` replaces them, :meth:`select_inducing` (or :func:`greedy_inducing`, before there is
    an instance) chooses them among the rows of ``X`` by greedy conditional-variance selection, :meth:`inducing_gradient`
    differentiates the objective with respect to ``Z`` and :meth:`optimize_inducing` moves ``Z`` to maximise it (``n_Z`` stays what it is).  ``method``: ``"fitc"``, ``"vfe"`` or ``"dtc"``.
    ``jitter``: added to the diagonal of ``k(Z, Z)`` (absolute).  ``chunk_rows``: training rows per pass over the data, a
    multiple of 64 (``None``: chosen by the library from a byte budget); predictions of the mean and the standard deviation send
    their test points through chunks of the same size.

    Supported: ``update_hyperparameters`` (value only), ``compute_K_L_alpha_ll`` (sets ``ll`` and ``ll_parts``),
    :meth:`sparse_gradient` (the gradient of the objective, ``gpt_sparse_grad_diff``), :meth:`inducing_gradient` and
    :meth:`optimize_inducing` (``gpt_sparse_grad_z``: ``n_Z = 0`` for every kernel; derivative rows among ``Z`` are refused for a
    Matern52 factor and, in its coordinate, for a Gibbs factor), ``optimize_hyperparameters`` (scipy on the
    value, or with ``gradient="sparse"`` on the value and that gradient; ``random_starts`` one after another),
    :meth:`sparse_ll_batch` (many hyperparameter vectors per launch sequence, ``gpt_sparse_fit_batch``), ``compute_ll_matrix`` and the
    host-stepped sampler (through it), ``predict`` and ``draw_sample`` (through the returned covariance).

    Refused (``NotImplementedError`` / ``ValueError``): a covariance kernel the library does not evaluate itself, warped
    kernels, a noise kernel that is not a ``DiagonalNoiseKernel``; ``T``, ``use_hyper_deriv``, ``partitioned``;
    ``ll_gradient*`` (see :meth:`sparse_gradient`), ``loo_*``, ``objective="loo"``, ``gradient="device"``, ``batch_starts``, ``ll_batch`` (see :meth:`sparse_ll_batch`); the
    library-stepped sampler, ``use_MCMC`` predictions; ``L`` and ``alpha`` (there is no ``N x N`` factor)."""

    def __init__(self, k, Z, noise_k=None, n_Z=0, method="fitc", jitter=1e-6, chunk_rows=None, X=None, y=None, err_y=0, n=0,
                 mu=None, diag_factor=1e2, verbose=False, device=0, T=None, use_hyper_deriv=False):
        if T is not None:
            raise NotImplementedError("SparseGaussianProcess does not take a linear transform T")
        if use_hyper_deriv:
            raise NotImplementedError("SparseGaussianProcess has no hyperparameter derivatives (use_hyper_deriv)")
        if method not in _lib.SPARSE_METHODS:
            raise ValueError("method must be one of %s, got %r" % (sorted(_lib.SPARSE_METHODS), method))
        jitter = float(jitter)
        if not jitter >= 0.0:
            raise ValueError("jitter must be non-negative, got %r" % (jitter,))
        if chunk_rows is not None and (int(chunk_rows) != chunk_rows or chunk_rows <= 0 or chunk_rows % 64):
            raise ValueError("chunk_rows must be None or a positive multiple of 64, got %r" % (chunk_rows,))
        self.method = method
        self.jitter = jitter
        self.chunk_rows = None if chunk_rows is None else int(chunk_rows)
        self.ll_parts = None
        super(SparseGaussianProcess, self).__init__(k, noise_k=noise_k, mu=mu, diag_factor=diag_factor, verbose=verbose,
                                                    device=device)
        self.set_inducing(Z, n_Z)
        self._sparse_refusal()
        if X is not None:
            if y is None:
                raise GPArgumentError("Must pass both X and y when constructing SparseGaussianProcess!")
            self.add_data(X, y, err_y=err_y, n=n)
        elif y is not None:
            raise GPArgumentError("Must pass both X and y when constructing SparseGaussianProcess!")

    # ---- inducing inputs, data -------------------------------------------------------------------
    def set_inducing(self, Z, n_Z=0):
        """Replace the inducing inputs ``Z`` (M, D) and their derivative orders ``n_Z`` (scalar or (M, D)).  On a context that
        holds the data only ``Z`` is sent again (the library drops its sparse fit with it); ``X`` stays where it is."""
        Z = _ingest.points(Z, self.num_dim, "Z")
        if Z.shape[0] < 1 or not np.all(np.isfinite(Z)):
            raise ValueError("Z must hold at least one point and finite entries only")
        self.Z = Z
        self.n_Z = _ingest.derivative_orders(n_Z, Z, self.num_dim, "n_Z", column_rule="row")
        self.K_up_to_date = False
        self._inducing_on_device = False

    def add_data(self, X, y, err_y=0, n=0, T=None):
        if T is not None:
            raise NotImplementedError("SparseGaussianProcess does not take a linear transform T")
        super(SparseGaussianProcess, self).add_data(X, y, err_y=err_y, n=n)

    def select_inducing(self, M, candidates=None, max_candidates=None, seed=0, tol=0.0, set=True):
        """Choose ``M`` inducing inputs among the rows of the instance's data by greedy conditional-variance selection at the
        current hyperparameters (``gpt_sparse_select_inducing`` on the resident data; arguments and ``(Z, info)`` as
        :func:`greedy_inducing`).  ``set=True``: ``set_inducing(Z, 0)`` with the result.  If the stop rule ends the selection early
        it warns and ``Z`` has ``count`` rows.  A resident fit is not disturbed by the selection itself."""
        if self.X is None:
            raise GPArgumentError("No data have been added to the SparseGaussianProcess!")
        terms = self._sparse_refusal()
        ctx = self._resident_ctx()
        ctx.set_warp(None)
        Z, info = _greedy_select(ctx, terms, self.X, self.n, M, candidates, max_candidates, seed, tol)
        if set:
            self.set_inducing(Z, 0)
        return Z, info

    def _upload_data(self, ctx):
        ctx.set_data(self.X, self.n)
        ctx.sparse_set_inducing(self.Z, self.n_Z)

    def _resident_ctx(self):
        """The instance's context with the data and the inducing inputs on it: each uploaded unless resident (an upload of the data
        sends ``Z`` after it)."""
        fresh = not self._data_on_device
        ctx = super(SparseGaussianProcess, self)._resident_ctx()
        if not fresh and not getattr(self, "_inducing_on_device", False):
            ctx.sparse_set_inducing(self.Z, self.n_Z)
        self._inducing_on_device = True
        return ctx

    # ---- what this class does not do ---------------------------------------------------------------
    def _sparse_refusal(self):
        """Raise for a configuration the sparse path does not take; returns the device model's terms otherwise."""
        if self.T is not None:
            raise NotImplementedError("SparseGaussianProcess does not take a linear transform T")
        if self.use_hyper_deriv:
            raise NotImplementedError("SparseGaussianProcess has no hyperparameter derivatives (use_hyper_deriv)")
        if self.partitioned:
            raise NotImplementedError("SparseGaussianProcess has no partitioned evaluation (partitioned)")
        if not isinstance(self.noise_k, (ZeroKernel, DiagonalNoiseKernel)):
            raise NotImplementedError("SparseGaussianProcess takes a ZeroKernel or DiagonalNoiseKernel as noise_k, not %s"
                                      % type(self.noise_k).__name__)
        return _device_terms(self)

    def _refuse(what):
        def method(self, *args, **kwargs):
            raise NotImplementedError("SparseGaussianProcess has no %s" % what)
        method.__doc__ = "Refused: the sparse path has no %s." % what
        return method

    ll_gradient = _refuse("dense-path gradient (ll_gradient): the gradient of the sparse objective is sparse_gradient")
    ll_gradient_batch = _refuse("batched gradient of the sparse objective (ll_gradient_batch): sparse_gradient takes one point at a time")
    loo_predict = _refuse("leave-one-out cross-validation (loo_predict)")
    loo_log_likelihood = _refuse("leave-one-out cross-validation (loo_log_likelihood)")
    loo_gradient = _refuse("leave-one-out cross-validation (loo_gradient)")
    ll_batch = _refuse("dense-path batched evaluator (ll_batch): the batched evaluator of the sparse objective is sparse_ll_batch")
    predict_MCMC = _refuse("predictions marginalised over hyperparameter samples (predict_MCMC)")
    compute_from_MCMC = _refuse("predictions marginalised over hyperparameter samples (compute_from_MCMC)")
    L = property(_refuse("N x N Cholesky factor (L)"))
    alpha = property(_refuse("N-vector alpha: the predictive mean is a dot product with the M-vector c"))
    del _refuse

    def _library_stepping(self):
        return "SparseGaussianProcess has no batched evaluator for the library to step", None

    # ---- the fit -------------------------------------------------------------------------------------
    def compute_K_L_alpha_ll(self, need_factor=True):
        """Evaluate the sparse objective on the GPU and set ``ll`` (log-posterior: objective + log hyperprior) and
        ``ll_parts`` (the five sums ``gpt_sparse_fit`` returns); no-op while ``K_up_to_date``.  Raises
        ``numpy.linalg.LinAlgError`` if ``K_uu + jitter I`` or ``B`` is not positive definite."""
        if self.K_up_to_date:
            return
        if self.X is None:
            raise GPArgumentError("No data have been added to the SparseGaussianProcess!")
        terms = self._sparse_refusal()
        self._cache = {}
        ctx = self._resident_ctx()
        ctx.set_warp(None)
        ll_data, parts = ctx.sparse_fit(_lib.SPARSE_METHODS[self.method], terms, self._noise_var(), self._y_alph(), self.err_y,
                                        self.jitter, self.chunk_rows or 0)
        self._fit_mode = "sparse"
        self.ll_parts = parts
        self.ll = ll_data + self.hyperprior(self.params)
        self.K_up_to_date = True

    def update_hyperparameters(self, new_params, hyper_deriv_handling="default", exit_on_bounds=True, inf_on_error=True):
        """``-(ll + log prior)`` at the free hyperparameters ``new_params``; ``+inf`` where the prior excludes them or a matrix
        is not positive definite (``inf_on_error``), as in the base class.  Value only."""
        if hyper_deriv_handling not in ("default", "value"):
            raise NotImplementedError("SparseGaussianProcess has no hyperparameter derivatives (hyper_deriv_handling=%r)"
                                      % (hyper_deriv_handling,))
        self._sparse_refusal()
        return super(SparseGaussianProcess, self).update_hyperparameters(new_params, hyper_deriv_handling="value",
                                                                         exit_on_bounds=exit_on_bounds,
                                                                         inf_on_error=inf_on_error)

    # ---- the gradient (gpt_sparse_grad_diff) ---------------------------------------------
    def sparse_gradient(self, rel_step=6e-6, inducing=False):
        """Gradient of the sparse objective plus the log hyperprior with respect to the free hyperparameters at their current
        values (``gpt_sparse_grad_diff``): one more pass over the data in chunks, whatever the number of parameters -- per free
        kernel parameter the term's central difference, eps = ``rel_step`` max(1, abs(theta)), is taken per pair (x_i, z_m),
        (z_m, z_m') and (x_i, x_i) before it meets its weight.  The noise parameter, the mean function's parameters and the
        hyperprior's derivative as in :meth:`GaussianProcess.ll_gradient`.  Fits first if the hyperparameters changed; they and
        ``K_up_to_date`` are afterwards what they were.  The result has no entry for ``Z``; with ``inducing=True`` the return value is
        ``(gradient, dZ)``, ``dZ`` as :meth:`inducing_gradient` returns it, both from ONE library call (``gpt_sparse_grad_z``)."""
        self._sparse_refusal()
        self.compute_K_L_alpha_ll()
        slot, tix, pa, pb, denom = self._ll_gradient_stencil(rel_step)
        if not inducing:
            g_dev, alpha = self._ctx.sparse_grad_diff(tix, pa, pb, denom, self._y_alph(), self.err_y, want_alpha=self.mu is not None)
            return self._ll_gradient_assemble(slot, g_dev, lambda: alpha)
        g_dev, alpha, dZ = self._ctx.sparse_grad_z(tix, pa, pb, denom, self._y_alph(), self.err_y, want_alpha=self.mu is not None)
        return self._ll_gradient_assemble(slot, g_dev, lambda: alpha), self._finite_dz(dZ)

    # ---- the inducing inputs (gpt_sparse_grad_z) ------------------------------------------
    @staticmethod
    def _finite_dz(dZ):
        if not np.all(np.isfinite(dZ)):
            raise FloatingPointError("d ll / d Z holds %d non-finite entries: the kernel's derivative does not exist at a pair the "
                                     "pass meets (a Matern kernel of small order where a training point coincides with an inducing "
                                     "input)" % int((~np.isfinite(dZ)).sum()))
        return dZ

    def inducing_gradient(self):
        """``d ll / d Z`` as an (M, D) array (``gpt_sparse_grad_z``): the gradient of the sparse objective with respect to every
        coordinate of the inducing inputs from one more pass over the data -- the derivative of a covariance entry with respect to
        a coordinate of ``z_m`` is the kernel with that point's derivative order raised by one, so nothing is differenced.  The log
        hyperprior does not depend on ``Z``.  Fits first if needed; hyperparameters and ``K_up_to_date`` are afterwards what they
        were.  ``FloatingPointError`` if an entry is not finite."""
        self._sparse_refusal()
        self.compute_K_L_alpha_ll()
        _, _, dZ = self._ctx.sparse_grad_z([], [], [], [], self._y_alph(), self.err_y)
        return self._finite_dz(dZ)

    def _inducing_box(self, bounds):
        """(M D, 2): the box of every coordinate of ``Z``, row-major as ``Z.ravel()``.  ``None``: the bounding box of ``X`` in the
        coordinate's dimension; a (D, 2) array: one box per dimension; (M, D, 2): one per coordinate."""
        M, D = self.Z.shape
        if bounds is None:
            if self.X is None:
                raise GPArgumentError("No data have been added to the SparseGaussianProcess!")
            bounds = np.stack([np.asarray(self.X, dtype=float).min(0), np.asarray(self.X, dtype=float).max(0)], axis=1)
        box = np.asarray(bounds, dtype=float)
        if box.shape == (D, 2):
            box = np.broadcast_to(box, (M, D, 2))
        if box.shape != (M, D, 2) or not np.all(box[..., 0] <= box[..., 1]):
            raise ValueError("bounds must be None, a (D, 2) or an (M, D, 2) array of (low, high) pairs with low <= high")
        return box.reshape(M * D, 2).copy()

    def optimize_inducing(self, method="L-BFGS-B", joint=False, bounds=None, opt_kwargs={}):
        """Move the inducing inputs to maximise the sparse objective: ``scipy.optimize.minimize`` on minus the log-posterior over
        ``vec(Z)`` -- with ``joint=True`` over ``[free hyperparameters, vec(Z)]``, the hyperparameters within their own bounds --
        with the gradient of :meth:`inducing_gradient` / :meth:`sparse_gradient` as ``jac``: one fit and one gradient pass per
        step.  ``bounds``: the box of ``Z`` (``None``: every coordinate within the bounding box of ``X`` in its dimension; a (D, 2)
        or (M, D, 2) array overrides it).  A fit that fails counts as ``+inf`` with a zero gradient.  On return ``Z`` (and, with
        ``joint``, the hyperparameters) are the optimum found; ``n_Z`` is not changed.  If the optimiser raises, ``Z`` and the
        hyperparameters are put back.  Returns scipy's result."""
        import scipy.optimize
        self._sparse_refusal()
        if "jac" in (opt_kwargs or {}) or "bounds" in (opt_kwargs or {}):
            raise ValueError("optimize_inducing supplies jac and bounds itself")
        M, D = self.Z.shape
        Z0, theta0 = self.Z.copy(), np.array(self.free_params[:], dtype=float)
        nfree = len(theta0) if joint else 0
        zbox = self._inducing_box(bounds)
        box = np.vstack([np.array(self.free_param_bounds[:], dtype=float).reshape(-1, 2), zbox]) if joint else zbox
        box[:, 0], box[:, 1] = np.where(np.isnan(box[:, 0]), -np.inf, box[:, 0]), np.where(np.isnan(box[:, 1]), np.inf, box[:, 1])
        x0 = np.concatenate([theta0[:nfree], np.clip(Z0.ravel(), zbox[:, 0], zbox[:, 1])])
        self._ctx                              # (no device: GPTBackendError here, not a +inf objective at every step)

        def assign(x):
            self.set_inducing(x[nfree:].reshape(M, D), self.n_Z)
            return self.update_hyperparameters(x[:nfree] if joint else theta0)

        def fun(x):
            x = np.array(x, dtype=float)
            f0 = assign(x)
            if not np.isfinite(f0):
                return np.inf, np.zeros(len(x))
            if joint:
                g, dZ = self.sparse_gradient(inducing=True)
            else:
                g, dZ = np.zeros(0), self.inducing_gradient()
            return f0, -1.0 * np.concatenate([g, dZ.ravel()])
        try:
            res = scipy.optimize.minimize(fun, x0, method=method, jac=True, bounds=[tuple(b) for b in box], **dict(opt_kwargs or {}))
            assign(np.array(res.x, dtype=float))
        except Exception:
            self.set_inducing(Z0, self.n_Z)
            self._assign_free(theta0)
            raise
        return res

    def _sparse_grad_jac(self):
        """``jac`` for scipy beside ``update_hyperparameters`` as ``fun``: minus :meth:`sparse_gradient`, zeros where the value is
        ``+inf`` -- the objective of ``GaussianProcess._device_grad_objective``.  The value at the point is the fit's if scipy has
        just evaluated it there (the hyperparameters are still its), one more evaluation otherwise."""
        def jac(x):
            x = np.array(x, dtype=float)
            if self.K_up_to_date and np.array_equal(np.asarray(self.free_params[:], dtype=float), x):
                f0 = -1.0 * self.ll
            else:
                f0 = self.update_hyperparameters(x)
            if not np.isfinite(f0):
                return np.zeros(len(x))
            try:
                return -1.0 * self.sparse_gradient()
            except Exception:
                warnings.warn("the gradient of the sparse objective failed at free hyperparameters %s, where the log-posterior is "
                              "%.6g:\n%s" % (x, -f0, traceback.format_exc()), RuntimeWarning)
                raise
        return jac

    # ---- many hyperparameter vectors per launch sequence (gpt_sparse_fit_batch) ------------
    #: most elements of one launch sequence of :meth:`sparse_ll_batch`; 1: one ``gpt_sparse_fit`` per vector, the loop.  :meth:`_ll_rows`
    #: (``compute_ll_matrix``, the host-stepped sampler) batches at EVERY shape: measured on MI355X with 32 vectors (DESIGN.md 18.11,
    #: SE, d = 2, fitc, N = 4096 ... 262144 x M = 64 ... 4096) the batch is faster than the loop at all sixteen shapes -- 6.6x at N =
    #: 4096 / M = 64, 1.2x to 1.6x at M = 4096, the least 1.07x at N = 262144 / M = 64 -- so no shape stays on the loop.
    sparse_batch_grid = 32

    def _sparse_batch_element_bytes(self):
        """``(chunk, bytes)``: the rows per pass of a fit of this shape and the device memory ONE element of ``gpt_sparse_fit_batch``
        takes.  With MPU = M to 128, BP = LDV = M + 1 to 128, MG = M + 1 to 64 and T = (MG / 64)(MG / 64 + 1) / 2 lower tiles::

            bytes = 8 [ chunk LDV                       the chunk buffer
                      + MPU^2 + 9216 (MPU / 128)        L_u and its leaves' workspaces
                      + BP^2 + 9216 (BP / 128)          B and its leaves' workspaces
                      + MG^2                            G
                      + 4096 S T                        the Gram partials, S slices
                      + 3 chunk + N ]                   k_i, the two per-row values; y

        ``chunk`` is ``chunk_rows``, or 512 MiB / (2 LDV 8) rounded down to 64, at most N rounded up to 64.  S T is about six times the
        compute units; the library knows their number, this bound takes 256 of them: S = min((1536 + T / 2) / T, rows / 4 rounded up,
        1024), at least 1."""
        M, N = int(self.Z.shape[0]), int(self.X.shape[0])
        MPU, BP, MG = -(-M // 128) * 128, -(-(M + 1) // 128) * 128, -(-(M + 1) // 64) * 64
        chunk = self.chunk_rows or max(64, (512 << 20) // (2 * BP * 8) // 64 * 64)
        chunk = min(chunk, -(-N // 64) * 64)
        T = (MG // 64) * (MG // 64 + 1) // 2
        S = max(1, min((1536 + T // 2) // T, -(-min(chunk, N) // 4), 1024))
        per = 8 * (chunk * BP + MPU * MPU + 9216 * (MPU // 128) + BP * BP + 9216 * (BP // 128) + MG * MG + 4096 * S * T + 3 * chunk + N)
        return chunk, per

    def sparse_ll_batch(self, param_list, exit_on_bounds=True):
        """Log-posterior at each free-parameter vector of ``param_list`` -- what ``-update_hyperparameters(p)`` returns for every
        ``p``, bit for bit -- from ONE launch sequence per chunk of the list (``gpt_sparse_fit_batch``): ``-inf`` where the prior
        excludes the vector (``exit_on_bounds``), where ``K_uu + jitter I`` or ``B`` is not positive definite and where a Lambda_i is
        not a positive finite number.  The host part runs per vector in order (prior, device terms, noise variance, ``y - mu(X)``);
        the list then goes through chunks of at most ``sparse_batch_grid`` elements, or as many as fit ``batch_grid_bytes`` and half
        of the free device memory at :meth:`_sparse_batch_element_bytes` an element.  A chunk that answers ``MemoryError`` is
        halved, a chunk the library rejects and a list whose elements are not one model shape are evaluated row by row.  An
        element's bits do not depend on how the list was cut.  The batch's device scratch (at most ``batch_grid_bytes``) stays allocated
        for the next call; ``self._ctx.release_batch_scratch()`` frees it.  Hyperparameters and ``K_up_to_date`` are afterwards what they were
        (``K_up_to_date`` is dropped if a row-by-row evaluation replaced the resident fit)."""
        param_list = [np.asarray(p, dtype=float) for p in param_list]
        out = np.full(len(param_list), -np.inf)
        if not param_list:
            return out
        if self.X is None:
            raise GPArgumentError("No data have been added to the SparseGaussianProcess!")
        self._sparse_refusal()
        keep, fitted = np.array(self.free_params[:], dtype=float), self.K_up_to_date
        try:
            jobs = []
            for i, p in enumerate(param_list):
                self._assign_free(p)
                prior = self.hyperprior(self.params)
                if exit_on_bounds and np.isinf(prior):
                    continue                                        # impossible parameters: stays -inf
                try:
                    terms = _device_terms(self)
                except np.linalg.LinAlgError:
                    continue                                        # (device parameters that need a solve that failed)
                jobs.append(_BatchJob(i, terms, [], self._noise_var(), np.array(self._y_alph(), dtype=float), prior))
            if jobs and not self._sparse_fit_jobs(jobs, param_list, exit_on_bounds, out):
                fitted = False
        finally:
            self._assign_free(keep)
            self.K_up_to_date = fitted
        return out

    def _sparse_fit_jobs(self, jobs, param_list, exit_on_bounds, out):
        """The chunk loop of :meth:`sparse_ll_batch`; returns whether the resident single fit is still the one it was (no row went
        through ``update_hyperparameters``)."""
        def rows_one_by_one(chunk):
            for j in chunk:
                out[j.row] = -1.0 * self.update_hyperparameters(param_list[j.row], exit_on_bounds=exit_on_bounds)

        G = int(self.sparse_batch_grid)
        if G <= 1 or any(_terms_shape(j.terms) != _terms_shape(jobs[0].terms) for j in jobs):
            rows_one_by_one(jobs)
            return False
        ctx = self._resident_ctx()
        ctx.set_warp(None)
        _, per = self._sparse_batch_element_bytes()
        G = max(1, min(G, min(int(self.batch_grid_bytes), ctx.mem_info()[0] // 2) // per))
        method, err_y, intact, s0 = _lib.SPARSE_METHODS[self.method], np.asarray(self.err_y, dtype=float), True, 0
        while s0 < len(jobs):
            chunk = jobs[s0:s0 + G]
            try:
                ll, _, _, which = ctx.sparse_fit_batch(method, [j.terms for j in chunk], np.array([j.noise_var for j in chunk]),
                                                       np.array([j.y_alph for j in chunk]), err_y, self.jitter, self.chunk_rows or 0)
                for j, l, w in zip(chunk, ll, which):
                    if w == 0:
                        out[j.row] = l + j.extra
            except MemoryError:
                ctx.release_batch_scratch()
                if G > 1:
                    G //= 2
                    continue
                rows_one_by_one(chunk)                              # (not even one element fits beside what is resident)
                intact = False
            except (ValueError, ArithmeticError):
                rows_one_by_one(chunk)                              # an argument of ONE element fails the whole call
                intact = False
            s0 += len(chunk)
        # (the batch's scratch stays on the device -- at most batch_grid_bytes: a sampler comes back thousands of times, and freeing and
        #  allocating gigabytes per call costs more than the fits; release_batch_scratch() of the context gives it back)
        return intact

    def _ll_rows(self, param_list):
        """The log-posterior at every row of ``param_list`` (``compute_ll_matrix``, the host-stepped sampler): through
        :meth:`sparse_ll_batch` (see ``sparse_batch_grid`` for the measurement behind it), one ``update_hyperparameters`` per row
        with ``sparse_batch_grid = 1``; the same bits either way."""
        if int(self.sparse_batch_grid) > 1:
            return self.sparse_ll_batch(param_list)
        keep = np.array(self.free_params[:], dtype=float)
        try:
            return np.array([-1.0 * self.update_hyperparameters(np.asarray(p, dtype=float)) for p in param_list])
        finally:
            self._assign_free(keep)

    def optimize_hyperparameters(self, method="SLSQP", opt_kwargs={}, verbose=False, random_starts=None, num_proc=None,
                                 max_tries=1, batch_fd=None, gradient=None, batch_starts=False, objective="ll"):
        """``scipy.optimize.minimize`` on the sparse objective, the starts one after another; arguments and return value as the base
        class.  ``gradient=None``: scipy differences the value itself, one fit per free parameter and step;
        ``gradient="sparse"``: scipy is given ``jac`` = minus :meth:`sparse_gradient`, one fit and one gradient pass per step
        (``+inf`` with a zero gradient where the value fails).  ``gradient="device"`` (the dense path's), ``batch_starts`` and
        ``objective="loo"`` are refused."""
        if gradient not in (None, "sparse"):
            raise NotImplementedError("SparseGaussianProcess has no dense-path gradient (gradient=%r): the gradient of the sparse "
                                      "objective is gradient='sparse'" % (gradient,))
        if batch_starts:
            raise NotImplementedError("SparseGaussianProcess has no batched evaluator (batch_starts)")
        if objective != "ll":
            raise NotImplementedError("SparseGaussianProcess has no leave-one-out objective (objective=%r)" % (objective,))
        self._sparse_refusal()
        if gradient == "sparse":
            if "jac" in (opt_kwargs or {}):
                raise ValueError("gradient='sparse' cannot be combined with a jac of the caller's")
            self._ctx                          # (no device: GPTBackendError here, not a +inf objective at every start)
            opt_kwargs = dict(opt_kwargs or {}, jac=self._sparse_grad_jac())
        return super(SparseGaussianProcess, self).optimize_hyperparameters(
            method=method, opt_kwargs=opt_kwargs, verbose=verbose, random_starts=random_starts, num_proc=num_proc,
            max_tries=max_tries, batch_fd=False)

    # ---- prediction ------------------------------------------------------------------------------------
    def predict(self, Xstar, n=0, noise=False, return_std=True, return_cov=False, full_output=False, use_MCMC=False, **kwargs):
        """Predictive mean (and std / covariance) of the sparse fit at ``Xstar``; arguments and return values as
        :meth:`GaussianProcess.predict`.  For ``"fitc"`` the covariance is the standard FITC predictive.  ``use_MCMC`` is
        refused."""
        if use_MCMC:
            raise NotImplementedError("SparseGaussianProcess has no predictions marginalised over hyperparameter samples (use_MCMC)")
        return super(SparseGaussianProcess, self).predict(Xstar, n=n, noise=noise, return_std=return_std, return_cov=return_cov,
                                                          full_output=full_output, **kwargs)

    def _predict_general(self, Xstar, n, noise, need_std, need_cov=True):
        want = 2 if need_cov else (1 if need_std else 0)
        return self._ctx.sparse_predict(Xstar, n, want, *self._prediction_noise(noise))
