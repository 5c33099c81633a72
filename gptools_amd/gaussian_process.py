"""GaussianProcess: the reference's GP API with the covariance build + Cholesky + LML + predict
hot path running on an MI355X through the C ABI of ``libgpt_hip.so``.

ref: gptools/gaussian_process.py:56-503 (class, add_data), :623-783 (optimize_hyperparameters),
:785-1034 (predict), :1332-1416 (update_hyperparameters), :1418-1522 (compute_K_L_alpha_ll),
:1535-1605 (compute_Kij), :2443-2486 (_OptimizeHyperparametersEval).

What runs where
  * GPU (include/gpt_hip.h): ``K(X, X', n, n')`` (fused, never tiled), ``K_tot`` assembly, blocked
    Cholesky, ``z = L^-1 y`` (as an extra row of the factorisation), log-determinant, ``alpha``,
    and predict's ``K*^T alpha``, ``K*^T L^-T`` and ``K** - v^T v``.
  * Host Python: argument checking, hyperparameter bookkeeping, the O(num_params) log-prior, the
    mean function, ``T`` / ``output_transform`` products and scipy.optimize driving the MAP loop.
There is no CPU fallback for the hot path: without the HIP library every computation raises.

State attributes follow the reference: ``X n y err_y T K noise_K L alpha ll ll_deriv
K_up_to_date``.  ``K``, ``noise_K``, ``L`` and ``alpha`` are fetched lazily from the device the
first time they are read after a fit, so the MAP loop moves only ``params`` and a scalar.
"""
import collections
import sys
import traceback
import warnings

import numpy as np
import scipy.linalg
import scipy.optimize

from . import _lib, _ingest
from . import replicas
from .error_handling import GPArgumentError, GPImpossibleParamsError
from .kernel import Kernel, ZeroKernel, DiagonalNoiseKernel, BinaryKernel, SumKernel, ProductKernel
from .kernel.masked import MaskedKernel
from .kernel.warping import WarpedKernel, beta_cdf_warp, linear_warp
from .utils import CombinedBounds, ProductJointPrior, UniformJointPrior

__all__ = ["GaussianProcess"]

_GIBBS = (_lib.KERNEL_GIBBS_TANH, _lib.KERNEL_GIBBS_DTANH, _lib.KERNEL_GIBBS_CUBIC, _lib.KERNEL_GIBBS_QUINTIC,
          _lib.KERNEL_GIBBS_EXPGAUSS, _lib.KERNEL_GIBBS_BSPLINE, _lib.KERNEL_GIBBS_GP)
_NATIVE_FIT = (_lib.KERNEL_SE, _lib.KERNEL_M52, _lib.KERNEL_RQ, _lib.KERNEL_MATERN, _lib.KERNEL_PERIODIC, _lib.KERNEL_SPECTRAL) + _GIBBS
_DEVICE_WARPS = {linear_warp: _lib.WARP_LINEAR, beta_cdf_warp: _lib.WARP_BETA}


def _uniform_to_normal(u):
    from scipy.stats import norm
    return norm.ppf(u)


# draw_sample: how the given variates are distributed -> what turns them into standard normals
_VARIATE_KINDS = {"standard normal": lambda u: u, "uniform": _uniform_to_normal}
# draw_sample(modify_sign=...): e = the three entries of every eigenvector at the chosen end, in index order
_SIGN_FEATURES = {
    "value": lambda e, where: e[0] if where == "left" else e[-1],
    "slope": lambda e, where: (e[1] - e[0]) if where == "left" else (e[-1] - e[-2]),
    "concavity": lambda e, where: e[2] - 2.0 * e[1] + e[0],
}


def _combine(a, b, c=None):
    out = CombinedBounds(a, b)
    return CombinedBounds(out, c) if c is not None else out


_UNRESOLVED = object()          # "resolve the device model yourself" (None is a resolved model: the library does not evaluate it)

#: one element of a batched fit: the row of the caller's list it answers, its device model (``_device_model``), noise variance and
#: ``y - mu``, and what the route carries along -- the log-prior (ll_batch) or the mean function at the test points (MCMC)
_BatchJob = collections.namedtuple("_BatchJob", "row terms layers noise_var y_alph extra")


def _terms_shape(terms):
    """What a batch needs equal in all its elements: the kernel id(s) of every term."""
    return [(t[0], t[2] if len(t) == 4 else -1) for t in terms]


def _gram(ctx, terms, Xi, ni, Xj, nj):
    """Gram block of a list of terms on a context: one builder call per term (a product term: ``kbuild2``), summed."""
    out = None
    for t in terms:
        Kt = ctx.kbuild2(t[0], t[1], t[2], t[3], Xi, ni, Xj, nj) if len(t) == 4 else ctx.kbuild(t[0], t[1], Xi, ni, Xj, nj)
        out = Kt if out is None else out + Kt
    return out


class GaussianProcess(object):
    """Gaussian process regression with derivative observations and predictions.

    Parameters are those of ref: gptools/gaussian_process.py:196-238: ``k``, ``noise_k``, ``X``,
    ``y``, ``err_y``, ``n``, ``T``, ``diag_factor``, ``mu``, ``use_hyper_deriv``, ``verbose``;
    ``device`` (extra) selects the GPU.

    ``partitioned`` (extra attribute, default False): in a ``torch.distributed`` job with one rank per GPU,
    ``update_hyperparameters`` evaluates the log-posterior with the factorisation partitioned over the ranks
    (``gptools_amd.dist.DistributedLML``: block-cyclic block columns, panels over RCCL) instead of on this rank's GPU
    alone -- for one native kernel without ``T`` and without hyperparameter derivatives.  Every rank must then make
    the same calls with the same hyperparameters (an optimiser run identically on every rank does: all ranks see the
    same ``ll``).  ``L``, ``alpha``, ``predict`` ... need the factor on this GPU and refit locally on first use.
    """

    def __init__(self, k, noise_k=None, X=None, y=None, err_y=0, n=0, T=None, diag_factor=1e2, mu=None,
                 use_hyper_deriv=False, verbose=False, device=0, eager_alpha=False):
        if not isinstance(k, Kernel):
            raise TypeError("Argument k must be an instance of Kernel when constructing GaussianProcess!")
        if noise_k is None:
            noise_k = ZeroKernel(k.num_dim)
        elif not isinstance(noise_k, Kernel):
            raise TypeError("Keyword noise_k must be an instance of Kernel when constructing GaussianProcess!")
        self.mu = mu
        self.diag_factor = diag_factor
        self.k = k
        self.noise_k = noise_k
        self.use_hyper_deriv = use_hyper_deriv
        self.verbose = verbose
        self.device = device
        if eager_alpha:
            self.eager_alpha = True
        self.y = np.array([], dtype=float)
        self.X = None
        self.err_y = np.array([], dtype=float)
        self.n = None
        self.T = None
        self.ll = None
        self.ll_deriv = None
        self._reset_device_state()
        if X is not None:
            if y is None:
                raise GPArgumentError("Must pass both X and y when constructing GaussianProcess!")
            self.add_data(X, y, err_y=err_y, n=n, T=T)
        elif y is not None:
            raise GPArgumentError("Must pass both X and y when constructing GaussianProcess!")
        else:
            self.K_up_to_date = False

    # ---- device plumbing -------------------------------------------------------------------
    def _reset_device_state(self, state=None):
        """Device handles and what depends on them, as before the first use (``state``: in that dict instead of the instance)."""
        (self.__dict__ if state is None else state).update(_ctx_obj=None, _scratch_ctx=None, _ctx_pool=None, _data_on_device=False,
                                                           _cache={}, _fit_mode=None, _dist_plan=None)

    partitioned = False
    partition_block = 512
    #: ``eager_alpha = True``: every fit also computes ``alpha`` and brings it to the host, like the reference's
    #: ``compute_K_L_alpha_ll`` (gaussian_process.py:1462) -- for drop-in users who read ``gp.alpha`` after every
    #: ``update_hyperparameters``.  Default False: ``alpha`` is computed on first use (``gp.alpha``, ``predict``, the analytic
    #: gradient); the MAP loop never reads it.  Cost at N = 8192: ~0.3 ms per evaluation (bench.py ``with_alpha``).
    eager_alpha = False

    def _partitioned_possible(self, model=_UNRESOLVED):
        if not self.partitioned or self.use_hyper_deriv or self.T is not None:
            return False
        model = self._device_model() if model is _UNRESOLVED else model
        # (one native term without warp layers; the multi-GPU engines have no Gibbs builder and know nothing of the masked encoding)
        if (not self._fast_fit_possible(model) or model[1] or len(model[0]) != 1 or model[0][0][0] in _GIBBS
                or self._has_masked()):
            return False
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized()

    @property
    def _ctx(self):
        """Per-instance context (owns the resident factorisation); created on first use."""
        if self._ctx_obj is None:
            self._ctx_obj = _lib.Context(self.device)
            # The contexts of ll_batch are created NOW, before any of them has run: measured on MI355X / ROCm 7,
            # streams created after another context's streams have been busy end up sharing hardware queues with
            # them (two evaluations in flight: 173 evaluations/s instead of 210 at N=8192).  An idle context costs
            # two streams and a few small buffers; its matrix is allocated on first use.
            self._ctx_pool = [[_lib.Context(self.device), -1] for _ in range(max(0, int(self.batch_concurrency) - 1))]
        return self._ctx_obj

    def __getstate__(self):
        # The reference keeps the GP picklable for its process pools (gaussian_process.py:1701-1703);
        # device handles never cross a pickle: they are re-created lazily in the new process.
        st = dict(self.__dict__)
        self._reset_device_state(st)
        st["K_up_to_date"] = False
        return st

    # ---- hyperparameter views (ref: gptools/gaussian_process.py:246-374) ---------------------
    @property
    def hyperprior(self):
        hp = self.k.hyperprior * self.noise_k.hyperprior
        if self.mu is not None:
            hp = hp * self.mu.hyperprior
        return hp

    @property
    def num_dim(self):
        return self.k.num_dim

    def _parts(self):
        return [self.k, self.noise_k] + ([self.mu] if self.mu is not None else [])

    def _view(self, attr):
        return _combine(*[getattr(p, attr) for p in self._parts()])

    def _scatter(self, attr, value, count_attr):
        pos = 0
        for p in self._parts():
            cnt = getattr(p, count_attr)
            setattr(p, attr, value[pos:pos + cnt])
            pos += cnt

    @property
    def fixed_params(self):
        return self._view("fixed_params")

    @fixed_params.setter
    def fixed_params(self, value):
        self._scatter("fixed_params", np.asarray(value, dtype=bool), "num_params")

    @property
    def params(self):
        return self._view("params")

    @params.setter
    def params(self, value):
        self.K_up_to_date = False
        self._scatter("params", np.asarray(value, dtype=float), "num_params")

    @property
    def param_bounds(self):
        return self.hyperprior.bounds

    @param_bounds.setter
    def param_bounds(self, value):
        self.hyperprior.bounds = value

    @property
    def param_names(self):
        return self._view("param_names")

    @param_names.setter
    def param_names(self, value):
        self._scatter("param_names", value, "num_params")

    @property
    def free_params(self):
        return self._view("free_params")

    @free_params.setter
    def free_params(self, value):
        self.K_up_to_date = False
        self._scatter("free_params", np.asarray(value, dtype=float), "num_free_params")

    @property
    def free_param_bounds(self):
        return self._view("free_param_bounds")

    @free_param_bounds.setter
    def free_param_bounds(self, value):
        self._scatter("free_param_bounds", np.asarray(value, dtype=float), "num_free_params")

    @property
    def free_param_names(self):
        return self._view("free_param_names")

    @free_param_names.setter
    def free_param_names(self, value):
        self.K_up_to_date = False
        self._scatter("free_param_names", np.asarray(value, dtype=str), "num_free_params")

    # ---- data ingest (ref: gptools/gaussian_process.py:376-503) ------------------------------
    def add_data(self, X, y, err_y=0, n=0, T=None):
        """Append observations: ``y`` (M,) observed at ``X`` (M, D) with standard deviations ``err_y`` (scalar or (M,))
        and derivative orders ``n`` (scalar or (M, D)).  With ``T`` (M, N') the observations are linear combinations
        ``T f(X)`` of the process at N' points ``X`` (line integrals); once any block has a transform, blocks without one
        get the identity and the blocks sit on the diagonal of ``self.T``.  Forms accepted: ``gptools_amd._ingest``."""
        y = _ingest.targets(y)
        err_y = _ingest.noise_levels(err_y, y)
        X = _ingest.points(X, self.num_dim)
        if T is None and X.shape[0] != y.size:
            raise ValueError("%d points for %d observations (without a transform T there is one point per observation)"
                             % (X.shape[0], y.size))
        n = _ingest.derivative_orders(n, X, self.num_dim, column_rule="not-column")
        if T is not None or self.T is not None:
            block = np.eye(y.size) if T is None else _ingest.linear_map(T, y.size, X.shape[0])
            if self.T is None and self.X is not None:
                self.T = np.eye(self.y.size)               # what was there so far was observed directly
            self.T = block if self.T is None else scipy.linalg.block_diag(self.T, block)
        self.X = X if self.X is None else np.concatenate((self.X, X), axis=0)
        self.n = n if self.n is None else np.concatenate((self.n, n), axis=0)
        self.y = np.concatenate((self.y, y))
        self.err_y = np.concatenate((self.err_y, err_y))
        self.K_up_to_date = False
        self._data_on_device = False
        self._dist_plan = None
        self._data_version = getattr(self, "_data_version", 0) + 1

    # ---- covariance matrices (ref: gptools/gaussian_process.py:1535-1605) --------------------
    def compute_Kij(self, Xi, Xj, ni, nj, noise=False, hyper_deriv=None, k=None):
        """Covariance matrix between ``Xi`` (M, D) and ``Xj`` (P, D) -> (M, P); ``Xj=None`` gives the
        symmetric ``K(Xi, Xi)``.  Native kernels use the fused GPU builder (``gpt_kbuild``); other
        ``Kernel`` subclasses receive the row-major pair list like the reference."""
        if k is None:
            k = self.noise_k if noise else self.k
        Xi = np.atleast_2d(np.asarray(Xi, dtype=float))
        ni = np.atleast_2d(np.asarray(ni, dtype=int))
        symmetric = Xj is None
        Xj = None if symmetric else np.atleast_2d(np.asarray(Xj, dtype=float))
        nj = None if symmetric else np.atleast_2d(np.asarray(nj, dtype=int))
        if k is self.k and isinstance(k, WarpedKernel) and hyper_deriv is None and self.X is not None:
            model = self._device_model()
            if model is not None:
                # the GP's own warped model: the builder on the warped points (gpt_set_warp needs the resident data for num_dim)
                ctx = self._resident_ctx()
                ctx.set_warp(model[1])
                return _gram(ctx, model[0], Xi, ni, Xj, nj)
        kid = getattr(k, "_gpt_kernel_id", None)
        if kid is not None and type(k).__call__ in (Kernel.__call__, _M52_CALL, _ZERO_CALL):
            if kid == _lib.KERNEL_M52 and hyper_deriv is not None:
                raise NotImplementedError("Hyperparameter derivatives have not been implemented!")
            return self._plain_ctx().kbuild(kid, k._native_params(), Xi, ni, Xj, nj, hyper_deriv=hyper_deriv,
                                            noise_n=getattr(k, "n", None))
        # a product of native kernels, or a masked kernel on its device route (kernel/masked.py): the builder, as one term
        nat = None
        if hyper_deriv is None and type(k) in (ProductKernel, MaskedKernel):
            nat = k._native_factors() if type(k) is ProductKernel else k._native_term()
        if nat is not None:
            return _gram(self._plain_ctx(), [nat], Xi, ni, Xj, nj)
        if symmetric:
            Xj, nj = Xi, ni
        M, P = Xi.shape[0], Xj.shape[0]
        Kij = k(np.repeat(Xi, P, axis=0), np.tile(Xj, (M, 1)), np.repeat(ni, P, axis=0), np.tile(nj, (M, 1)),
                hyper_deriv=hyper_deriv, symmetric=symmetric)
        return np.reshape(Kij, (M, -1))

    # ---- lazily materialised state ------------------------------------------------------------
    def _cached(self, key, fn):
        if key not in self._cache:
            self._cache[key] = fn()
        return self._cache[key]

    @property
    def K(self):
        """Noise-free training covariance (ref attribute ``K``, gaussian_process.py:1431)."""
        self.compute_K_L_alpha_ll()
        return self._cached("K", lambda: self.compute_Kij(self.X, None, self.n, None))

    @property
    def noise_K(self):
        """Noise part of the training covariance (ref: gaussian_process.py:1434-1439)."""
        self.compute_K_L_alpha_ll()
        return self._cached("noise_K", self._noise_K)

    def _noise_K(self):
        N = self.X.shape[0]
        if isinstance(self.noise_k, DiagonalNoiseKernel):
            return self._noise_var() * np.eye(N)
        return self.compute_Kij(self.X, None, self.n, None, noise=True)

    @property
    def L(self):
        """Lower Cholesky factor of ``K_tot`` (ref: gaussian_process.py:1452)."""
        self.compute_K_L_alpha_ll()
        return self._cached("L", lambda: self._ctx.get_L(len(self.y)))

    @property
    def alpha(self):
        """``K_tot^-1 (y - T mu)`` as an (N_y, 1) column (ref: gaussian_process.py:1462)."""
        self.compute_K_L_alpha_ll()
        return self._cached("alpha", lambda: self._ctx.get_alpha(len(self.y)).reshape(-1, 1))

    # ---- the fit (ref: gptools/gaussian_process.py:1418-1522) --------------------------------
    def _y_alph(self):
        if self.mu is None:
            return self.y
        mu_alph = self.mu(self.X, self.n)
        if self.T is not None:
            mu_alph = self.T.dot(mu_alph)
        return self.y - mu_alph

    def _upload_data(self, ctx):
        """X, n and -- when the observations are linear transforms of the latent values -- T (ref :376-503)."""
        ctx.set_data(self.X, self.n)
        if self.T is not None:
            ctx.set_T(self.T)

    def _resident_ctx(self):
        """The instance's context with the data on it: uploaded unless resident."""
        ctx = self._ctx
        if not self._data_on_device:
            self._upload_data(ctx)
            self._data_on_device = True
        return ctx

    # ---- the noise kernel as the device takes it: a variance in the fit, (parameters, orders) in a noisy prediction -------------
    def _noise_var(self):
        return 0.0 if isinstance(self.noise_k, ZeroKernel) else self.noise_k.params[0] ** 2.0

    def _diagonal_noise(self):
        return isinstance(self.noise_k, DiagonalNoiseKernel) and not isinstance(self.noise_k, ZeroKernel)

    def _noise_is_free(self):
        return self._diagonal_noise() and not self.noise_k.fixed_params[0]

    def _prediction_noise(self, noise):
        """``(noise_params, noise_n)`` of a prediction on the kernel route, ``(None, None)`` for a noise-free one."""
        return (self.noise_k.params, self.noise_k.n) if noise and self._diagonal_noise() else (None, None)

    def _native_terms(self, k=None):
        """The covariance kernel as a list of ``(kernel_id, params)`` terms the HIP library evaluates itself -- a native
        kernel, or a SumKernel tree of them (ref: gptools/kernel/core.py:549-584) -- else ``None``."""
        k = self.k if k is None else k
        if type(k) is SumKernel:
            a, b = self._native_terms(k.k1), self._native_terms(k.k2)
            return None if a is None or b is None or len(a) + len(b) > 8 else a + b
        if (getattr(k, "_gpt_kernel_id", None) in _NATIVE_FIT and type(k).__call__ in (Kernel.__call__, _M52_CALL)):
            return [(k._gpt_kernel_id, k._native_params())]
        if type(k) is ProductKernel:
            # k1 * k2 of two native kernels: one PRODUCT term of the fused builder (ref: gptools/kernel/core.py:587-671)
            nat = k._native_factors()
            return None if nat is None else [nat]
        if type(k) is MaskedKernel:
            # (by type, never through a forwarded attribute) a stationary kernel with infinite length scales outside its mask, or
            # a Gibbs kernel on one dimension times the unit factor (kernel/masked.py); None: the host route
            nat = k._native_term()
            return None if nat is None else [nat]
        return None

    def _has_masked(self, k=None):
        """A ``MaskedKernel`` anywhere in the covariance kernel's tree."""
        k = self.k if k is None else k
        if isinstance(k, MaskedKernel):
            return True
        if isinstance(k, BinaryKernel):
            return self._has_masked(k.k1) or self._has_masked(k.k2)
        return isinstance(k, WarpedKernel) and self._has_masked(k.k)

    def _device_model(self):
        """``(terms, layers)`` when the library evaluates the whole covariance kernel itself, else ``None``: ``terms`` as
        :meth:`_native_terms` gives them for the kernel under the outer ``WarpedKernel`` layers, ``layers`` those layers as
        ``gpt_set_warp`` takes them -- ``(type, params)``, the outermost (applied first) first; empty without a warp.  Only
        layers whose warp function is exactly ``beta_cdf_warp`` or ``linear_warp`` (and whose ``__call__`` is the class's own)
        peel off, at most ``GPT_WARP_MAX_LAYERS``; a warped kernel anywhere else in the tree keeps the host class."""
        k, layers = self.k, []
        while isinstance(k, WarpedKernel):
            kind = _DEVICE_WARPS.get(getattr(k.w, "fun", None))
            if kind is None or type(k).__call__ is not WarpedKernel.__call__ or len(k.w.params) != 2 * k.num_dim:
                return None
            layers.append((kind, np.array(k.w.params, dtype=float)))
            k = k.k
        if len(layers) > _lib.WARP_MAX_LAYERS:
            return None
        terms = self._native_terms(k)
        return None if terms is None else (terms, layers)

    def _plain_ctx(self):
        """The context for a kernel that is not the GP's model (``compute_Kij(k=...)``): the instance's own, unless that
        holds the model's warp layers -- they would warp this kernel's points too."""
        ctx = self._ctx
        return ctx if ctx._warp_key is None else _lib.default_context(self.device)

    def _fast_fit_possible(self, model=_UNRESOLVED):
        """The kernel route: the library evaluates the covariance kernel (``model``: what :meth:`_device_model` gave, where the
        caller has resolved it already) and the noise is a variance on the diagonal."""
        model = self._device_model() if model is _UNRESOLVED else model
        return model is not None and isinstance(self.noise_k, (ZeroKernel, DiagonalNoiseKernel))

    def _device_fit(self, ctx, terms, noise_var, y_alph, diag_add):
        if any(len(t) == 4 for t in terms):
            return ctx.fit_terms(terms, noise_var, y_alph, self.err_y, diag_add)
        if len(terms) == 1:
            return ctx.fit(terms[0][0], terms[0][1], noise_var, y_alph, self.err_y, diag_add)
        return ctx.fit_sum([t[0] for t in terms], [t[1] for t in terms], noise_var, y_alph, self.err_y, diag_add)

    def compute_K_L_alpha_ll(self, need_factor=True):
        """Build ``K_tot``, factor it and evaluate the log-posterior ``ll`` on the GPU (no-op while
        ``K_up_to_date``).  Raises ``numpy.linalg.LinAlgError`` if ``K_tot`` is not positive
        definite, like ``scipy.linalg.cholesky`` in the reference.

        ``need_factor=False`` (``update_hyperparameters``): only ``ll`` is wanted, which lets a ``partitioned`` GP
        evaluate it with the factorisation spread over the ranks of the job; the factor then is not on this GPU and
        the next call that needs it refits locally."""
        if self.K_up_to_date and (self._fit_mode != "partitioned" or not need_factor):
            return
        if self.X is None:
            raise GPArgumentError("No data have been added to the GaussianProcess!")
        self._cache = {}
        y_alph = self._y_alph()
        diag_add = self.diag_factor * sys.float_info.epsilon
        model = self._device_model()                 # resolved once per evaluation: for GibbsKernel1dGP a host solve
        if not need_factor and self._partitioned_possible(model):
            from .dist import DistributedLML
            if self._dist_plan is None:
                self._dist_plan = DistributedLML(self.X, self.n, nb=self.partition_block, device=self.device)
            kid, kparams = model[0][0]
            ll_data, _ = self._dist_plan.fit(kid, kparams, y_alph, self.err_y, noise_var=self._noise_var(),
                                             diag_factor=self.diag_factor)
            self._fit_mode = "partitioned"
            self.ll = ll_data + self.hyperprior(self.params)
            self.K_up_to_date = True
            return
        ctx = self._ctx
        # (eager: the device enqueues alpha behind the factorisation of the same call; get_alpha below is then a copy)
        ctx.set_option("eager_alpha", 1 if self.eager_alpha else 0)
        if self._fast_fit_possible(model):
            self._resident_ctx()
            terms, layers = model
            ctx.set_warp(layers)                 # (no-op unless the layers or their parameters changed)
            ll_data, _ = self._device_fit(ctx, terms, self._noise_var(), y_alph, diag_add)
            self._fit_mode = "kernel"
        else:
            # T (linear transform) or a Python-defined kernel: K is still built by the GPU builder
            # where the kernel is native, the small T products are host GEMMs, the factorisation and
            # solves run on the GPU (gpt_fit_matrix).
            K = self.compute_Kij(self.X, None, self.n, None)
            self._cache["K"] = K
            noise_K = self._noise_K()
            self._cache["noise_K"] = noise_K
            KnK = K + noise_K
            if self.T is not None:
                KnK = self.T.dot(KnK).dot(self.T.T)
            K_tot = KnK + np.diag(self.err_y ** 2.0) + diag_add * np.eye(len(self.y))
            ll_data, _ = ctx.fit_matrix(K_tot, y_alph)
            self._data_on_device = False
            self._fit_mode = "matrix"
        self.ll = ll_data + self.hyperprior(self.params)          # log-posterior (ref :1469)
        if self.eager_alpha:
            self._cache["alpha"] = ctx.get_alpha(len(self.y)).reshape(-1, 1)      # (ref :1462)
        if self.use_hyper_deriv:
            self._compute_ll_deriv()
        self.K_up_to_date = True

    def _compute_ll_deriv(self):
        """Gradient of the log-posterior with respect to the free hyperparameters
        (ref: gptools/gaussian_process.py:1471-1520): 1/2 (alpha^T dK alpha - tr(K_tot^-1 dK))."""
        warnings.warn("Use of hyperparameter derivatives is experimental!")
        ctx = self._ctx
        Ny = len(self.y)
        alpha = ctx.get_alpha(Ny)
        self._cache["alpha"] = alpha.reshape(-1, 1)

        def term(dK, transform=True):
            if self.T is not None and transform:
                dK = self.T.dot(dK).dot(self.T.T)
            W = ctx.solve_L(dK)                     # L^-1 dK
            W2 = ctx.solve_L(np.ascontiguousarray(W.T))    # L^-1 (L^-1 dK)^T -> trace equals tr(K^-1 dK)
            return 0.5 * (alpha.dot(dK.dot(alpha)) - np.trace(W2))

        ll_deriv = np.zeros(len(self.free_params))
        # (a masked term: gpt_ll_grad indexes the DEVICE parameter arrays, which the masked encoding expands -- the
        # per-parameter host branch below, every dK through compute_Kij)
        terms = self._native_terms() if self._fit_mode == "kernel" and not self._has_masked() else None
        knk = self.k
        free_idx = np.arange(0, len(knk.params), dtype=int)[~np.asarray(knk.fixed_params, dtype=bool)]
        tix = lix = None
        if terms is not None:
            # which kernel term each free parameter belongs to; the device path needs every FREE parameter in a
            # squared-exponential term (terms of other kernels may take part in the sum with all their parameters fixed:
            # they have no hyperparameter derivatives in the reference either, kernel/core.py:723-726)
            bounds = np.cumsum([0] + [len(t[1]) + (len(t[3]) if len(t) == 4 else 0) for t in terms])
            tix = [int(np.searchsorted(bounds, pi, side="right") - 1) for pi in free_idx]
            lix = [int(pi - bounds[t]) for pi, t in zip(free_idx, tix)]
        if terms is not None and all(len(terms[t]) == 2 and terms[t][0] == _lib.KERNEL_SE for t in tix):
            # device path (gpt_ll_grad): K_tot^-1 once (2 N^3 / 3 flop on the MFMA GEMM, whatever the number of
            # parameters), then one fused pass over the pairs per group of parameters; dK never exists.  With a linear
            # transform T the pass runs over the latent points against T^T K_tot^-1 T (two more GEMMs on the device).
            g_dev = ctx.ll_grad(tix, lix)
            ll_deriv[:len(free_idx)] = g_dev[:-1]
            if self._noise_is_free():
                ll_deriv[len(self.k.free_params)] = 2.0 * self.noise_k.params[0] * g_dev[-1]
        else:
            if not isinstance(self.noise_k, DiagonalNoiseKernel):
                knk = self.k + self.noise_k
            elif self._noise_is_free():
                # (the reference does not transform this term: 2 sigma_n eye(len(y)), ref :1482-1488)
                ll_deriv[len(self.k.free_params)] = term(2.0 * self.noise_k.params[0] * np.eye(Ny), transform=False)
            free_idx = np.arange(0, len(knk.params), dtype=int)[~np.asarray(knk.fixed_params, dtype=bool)]
            for i, pi in enumerate(free_idx):
                ll_deriv[i] = term(self.compute_Kij(self.X, None, self.n, None, k=knk, hyper_deriv=int(pi)))
        if self.mu is not None:
            free_idx = np.arange(0, len(self.mu.params), dtype=int)[~self.mu.fixed_params]
            for i, pi in enumerate(free_idx):
                dmu = self.mu(self.X, self.n, hyper_deriv=int(pi))
                if self.T is not None:
                    dmu = self.T.dot(dmu)
                ll_deriv[i + len(knk.free_params)] = dmu.dot(alpha)
        self.ll_deriv = ll_deriv + self._hyperprior_gradient()

    def _hyperprior_gradient(self):
        """The log-prior's derivative with respect to every free hyperparameter (ref :1517-1520)."""
        free_idx = np.arange(0, len(self.params), dtype=int)[~np.asarray(self.fixed_params[:], dtype=bool)]
        grad = np.zeros(len(free_idx))
        for i, pi in enumerate(free_idx):
            grad[i] = self.hyperprior(self.params[:], hyper_deriv=int(pi))
        return grad

    # ---- device gradient for every native kernel (gpt_ll_grad_diff) ------------
    def _ll_gradient_refusal(self):
        """Why ``gpt_ll_grad_diff`` cannot serve this model, or ``None``."""
        model = self._device_model()
        if model is not None and model[1]:
            return "a warped model (WarpedKernel layers evaluated on the device)"
        if not self._fast_fit_possible(model):
            return ("the matrix route (a covariance or noise kernel the library does not evaluate itself: K_tot is assembled "
                    "on the host)")
        if self._partitioned_possible(model):
            return "a partitioned fit (the factor is spread over the ranks of the job)"
        return None

    def _ll_gradient_stencil(self, rel_step):
        """The central stencils of the free KERNEL parameters at the current hyperparameters, as ``Context.ll_grad_diff``
        takes them: ``(slot, term_idx, params_a, params_b, denom)``, entry ``h`` a term of the device model whose parameters
        change along free parameter ``slot[h]``, with that term's complete device parameters at theta - eps and theta + eps
        (eps = ``rel_step`` max(1, abs(theta)); a point that would leave the parameter's bounds stays on the bound) and ``denom[h]``
        the floating-point difference of the two values of the parameter.
        The device parameters are :meth:`_native_terms` after :meth:`_assign_free` at each point -- a masked term's expanded
        array and the nested GP's weights are what a fit there would send.  The hyperparameters are restored; host only."""
        theta = np.array(self.free_params[:], dtype=float)
        box = np.array(self.free_param_bounds[:], dtype=float).reshape(-1, 2)
        up_to_date = self.K_up_to_date
        slot, tix, pa, pb, denom = [], [], [], [], []

        def flat(t):
            return np.concatenate([np.asarray(p, dtype=float).ravel() for p in t[1::2]])
        try:
            for i in range(len(self.k.free_params)):
                eps = rel_step * max(1.0, abs(theta[i]))
                ta, tb = theta.copy(), theta.copy()
                # (an optimiser puts parameters ON their bounds, and beyond one the library may refuse the point -- Matern's nu,
                # a B-spline's knot order: a stencil point that would leave the bounds stays on the bound, the difference then
                # one-sided, first order in eps)
                ta[i] = theta[i] - eps
                tb[i] = theta[i] + eps
                if box[i, 0] <= theta[i] <= box[i, 1]:      # (NaN bounds, or a value already outside them: the plain stencil)
                    ta[i] = max(ta[i], box[i, 0])
                    tb[i] = min(tb[i], box[i, 1])
                if not tb[i] > ta[i]:
                    continue                                # (bounds that pin the parameter: no derivative to take)
                self._assign_free(ta)
                terms_a = self._native_terms()
                self._assign_free(tb)
                terms_b = self._native_terms()
                if terms_a is None or terms_b is None or len(terms_a) != len(terms_b):
                    raise NotImplementedError("ll_gradient: the covariance kernel is not a model the library evaluates itself")
                for t, (a, b) in enumerate(zip(terms_a, terms_b)):
                    if a[0::2] != b[0::2]:
                        raise NotImplementedError("ll_gradient: term %d changes its kernel along free parameter %d" % (t, i))
                    fa, fb = flat(a), flat(b)
                    if fa.shape != fb.shape or not np.array_equal(fa, fb):
                        slot.append(i)
                        tix.append(t)
                        pa.append(fa)
                        pb.append(fb)
                        denom.append(tb[i] - ta[i])
        finally:
            self._assign_free(theta)
            self.K_up_to_date = up_to_date          # (the very values the fit was made at)
        return slot, tix, pa, pb, np.asarray(denom, dtype=float)

    def ll_gradient(self, rel_step=6e-6):
        """Gradient of the log-posterior with respect to the free hyperparameters at their current values, for every model of
        native kernels (``gpt_ll_grad_diff``): ``K_tot^-1`` once on the device, then per free kernel parameter two passes over
        the pairs with the term's central difference taken per pair -- eps = ``rel_step`` max(1, abs(theta)) -- instead of a
        factorisation per parameter.  Fits first if the hyperparameters changed.  The noise parameter, the mean function's
        parameters and the hyperprior's derivative as in the analytic gradient (``use_hyper_deriv``), which this leaves as it
        is -- with a transform ``T`` that includes the reference's form of the noise entry, 2 sigma_n I over the observations (ref
        :1482-1488), which is not the derivative of the fitted likelihood (the fit transforms the noise term): fix the noise
        parameter when optimising such a model with this gradient.  ``NotImplementedError`` for a warped model, the matrix route and a partitioned fit."""
        why = self._ll_gradient_refusal()
        if why is not None:
            raise NotImplementedError("ll_gradient is not available for %s" % why)
        self.compute_K_L_alpha_ll()
        if self._fit_mode != "kernel":
            raise NotImplementedError("ll_gradient is not available for a fit by the %s route" % self._fit_mode)
        ctx = self._ctx
        slot, tix, pa, pb, denom = self._ll_gradient_stencil(rel_step)
        g_dev = ctx.ll_grad_diff(tix, pa, pb, denom)
        return self._ll_gradient_assemble(slot, g_dev, lambda: ctx.get_alpha(len(self.y)))

    def _ll_gradient_assemble(self, slot, g_dev, get_alpha):
        """The gradient at the CURRENT hyperparameters from the device's entries ``g_dev`` (one per stencil entry, kernel parameter
        ``slot[h]``; the noise trace last): the noise entry 2 sigma_n times the trace, the mean function's entries against
        ``get_alpha()`` and the hyperprior's derivative.  Host only; shared by :meth:`ll_gradient` and :meth:`ll_gradient_batch`."""
        grad = np.zeros(len(self.free_params))
        for s, v in zip(slot, g_dev[:-1]):
            grad[s] += v
        nk = len(self.k.free_params)
        if self._noise_is_free():
            grad[nk] = 2.0 * self.noise_k.params[0] * g_dev[-1]
        if self.mu is not None:
            alpha = get_alpha()
            free_idx = np.arange(0, len(self.mu.params), dtype=int)[~self.mu.fixed_params]
            for i, pi in enumerate(free_idx):
                dmu = self.mu(self.X, self.n, hyper_deriv=int(pi))
                if self.T is not None:
                    dmu = self.T.dot(dmu)
                grad[i + nk + len(self.noise_k.free_params)] = dmu.dot(alpha)
        return grad + self._hyperprior_gradient()

    # ---- leave-one-out cross-validation (gpt_loo, gpt_loo_grad_diff) ------------
    def _loo(self):
        """``(L_LOO, resid, var)`` of the current fit (``Context.loo``), cached with it."""
        self.compute_K_L_alpha_ll()
        return self._cached("loo", lambda: self._ctx.loo(len(self.y)))

    def loo_predict(self, return_std=True):
        """Leave-one-out predictions at the training observations (Rasmussen & Williams 5.4.2): ``m[i]`` is the mean at observation
        i of the model fitted to all the others at the current hyperparameters and ``s[i]`` its standard deviation, the noise
        of observation i included -- ``(y[i] - m[i]) / s[i]`` is standard normal if the model is right.  From the resident factor
        (``gpt_loo``), no refits.  Returns ``m``, or ``(m, s)`` with ``return_std``, of length ``len(y)``.  Fits first if the
        hyperparameters changed; every fit route serves, a transform ``T`` and a warped model included."""
        _, resid, var = self._loo()
        m = self.y - resid
        return (m, np.sqrt(var)) if return_std else m

    def loo_log_likelihood(self):
        """The leave-one-out log predictive probability ``sum_i log N(y_i; m_i, s_i^2)`` at the current hyperparameters, without
        the hyperprior (see :meth:`loo_predict`)."""
        return self._loo()[0]

    def _loo_gradient_refusal(self):
        """Why ``gpt_loo_grad_diff`` cannot serve this model, or ``None``: a reason of :meth:`_ll_gradient_refusal`, or a linear
        transform."""
        why = self._ll_gradient_refusal()
        if why is None and self.T is not None:
            why = "a linear transform T (the leave-one-out weights would have to be carried to the latent points)"
        return why

    def _loo_value_and_gradient(self, rel_step):
        """``(L_LOO, gradient of L_LOO + log hyperprior)`` at the current hyperparameters from ONE ``gpt_loo_grad_diff`` call."""
        why = self._loo_gradient_refusal()
        if why is not None:
            raise NotImplementedError("loo_gradient is not available for %s" % why)
        self.compute_K_L_alpha_ll()
        if self._fit_mode != "kernel":
            raise NotImplementedError("loo_gradient is not available for a fit by the %s route" % self._fit_mode)
        slot, tix, pa, pb, denom = self._ll_gradient_stencil(rel_step)
        g_dev, ll, resid, var, u = self._ctx.loo_grad_diff(tix, pa, pb, denom, len(self.y))
        self._cache["loo"] = (ll, resid, var)
        return ll, self._loo_gradient_assemble(slot, g_dev, u)

    def loo_gradient(self, rel_step=6e-6):
        """Gradient of :meth:`loo_log_likelihood` plus the log hyperprior with respect to the free hyperparameters at their current
        values (``gpt_loo_grad_diff``): ``K_tot^-1`` and one further GEMM on the device, whatever the number of parameters, then per
        free kernel parameter the two pair passes of :meth:`ll_gradient` against the leave-one-out weights.  Fits first if the
        hyperparameters changed.  ``NotImplementedError`` where :meth:`ll_gradient` raises it, and for a transform ``T``."""
        return self._loo_value_and_gradient(rel_step)[1]

    def _loo_gradient_assemble(self, slot, g_dev, u):
        """:meth:`_ll_gradient_assemble` for the leave-one-out objective: ``g_dev`` are ``gpt_loo_grad_diff``'s entries (the noise
        trace last) and the mean function's entries are taken against ``u = K_tot^-1 resid`` where the LML has ``alpha``.  Host
        only."""
        grad = np.zeros(len(self.free_params))
        for s, v in zip(slot, g_dev[:-1]):
            grad[s] += v
        nk = len(self.k.free_params)
        if self._noise_is_free():
            grad[nk] = 2.0 * self.noise_k.params[0] * g_dev[-1]
        if self.mu is not None:
            u = np.asarray(u, dtype=float).ravel()
            free_idx = np.arange(0, len(self.mu.params), dtype=int)[~self.mu.fixed_params]
            for i, pi in enumerate(free_idx):
                dmu = self.mu(self.X, self.n, hyper_deriv=int(pi))
                if self.T is not None:
                    dmu = self.T.dot(dmu)
                grad[i + nk + len(self.noise_k.free_params)] = dmu.dot(u)
        return grad + self._hyperprior_gradient()

    def _loo_objective(self, device):
        """``(fun, jac)`` for scipy.optimize.minimize with ``objective="loo"``: ``fun`` is minus (``L_LOO`` + log hyperprior), ``+inf``
        where the hyperprior excludes the point or the evaluation fails.  ``device``: value and ``jac`` of a point come from one
        ``gpt_loo_grad_diff`` call (zeros where the value is ``+inf``); else ``jac`` is ``None`` and scipy differences ``fun``."""
        last = {}

        def evaluate(x):
            x = np.array(x, dtype=float)
            try:
                self._assign_free(x)
                prior = self.hyperprior(self.params)
                if np.isinf(prior):
                    raise GPImpossibleParamsError("the hyperprior excludes these hyperparameters")
                if device:
                    ll, grad = self._loo_value_and_gradient(6e-6)
                else:
                    ll, grad = self.loo_log_likelihood(), None
                f, g = -1.0 * (ll + prior), (None if grad is None else -1.0 * grad)
                if not np.isfinite(f) or (g is not None and not np.all(np.isfinite(g))):
                    raise FloatingPointError("the leave-one-out objective is not finite")
            except Exception as exc:
                if self.verbose and not isinstance(exc, GPImpossibleParamsError):
                    warnings.warn("evaluation failed at free hyperparameters %s and counts as +inf:\n%s"
                                  % (x, traceback.format_exc()))
                f, g = np.inf, np.zeros(len(x))
            last["x"], last["f"], last["g"] = x, f, g
            return f, g

        def fun(x):
            return evaluate(x)[0]

        def jac(x):
            if "x" in last and np.array_equal(last["x"], np.asarray(x, dtype=float)):
                return last["g"]
            return evaluate(x)[1]
        return fun, (jac if device else None)

    def remove_outliers(self, thresh=3, method="predict", **predict_kwargs):
        """Drop the observations that sit ``thresh`` standard deviations or more from what the GP says about them, and return
        them (ref: gaussian_process.py:543-621).

        ``method="predict"``, the reference's rule: observation i is bad when ``abs(predict(X, n, noise=False)[i] - y[i]) /
        err_y[i] >= thresh``; an observation with ``err_y == 0`` is never bad.  ``predict_kwargs`` go to :meth:`predict`.  The
        rule ignores the GP's own uncertainty, and the mean it tests against has seen the point it judges.
        ``method="loo"``: ``abs(y[i] - m[i]) / s[i] >= thresh`` with :meth:`loo_predict`'s leave-one-out mean and standard
        deviation -- every point is judged by the model that has not seen it, the GP's uncertainty and the noise included.

        Returns ``(X_bad, y_bad, err_y_bad, n_bad, bad_idxs)``; ``bad_idxs`` is a boolean array over the observations as they
        were before the call.  The next evaluation refits on what is left.  With a transform ``T``: ``NotImplementedError``."""
        if method not in ("predict", "loo"):
            raise ValueError("method must be 'predict' or 'loo', got %r" % (method,))
        if self.T is not None:
            raise NotImplementedError("remove_outliers is not available with a linear transform T")
        if method == "loo":
            if predict_kwargs:
                raise TypeError("method='loo' takes no predict arguments, got %s" % sorted(predict_kwargs))
            m, s = self.loo_predict(return_std=True)
            deltas = np.abs(self.y - m) / s
        else:
            mean = self.predict(self.X, n=self.n, noise=False, return_std=False, **predict_kwargs)
            exact = self.err_y == 0
            deltas = np.abs(np.asarray(mean, dtype=float).ravel() - self.y) / np.where(exact, 1.0, self.err_y)
            deltas[exact] = 0.0
        bad = deltas >= thresh
        removed = (self.X[bad, :], self.y[bad], self.err_y[bad], self.n[bad, :], bad)
        self.X, self.n, self.y, self.err_y = self.X[~bad, :], self.n[~bad, :], self.y[~bad], self.err_y[~bad]
        self.K_up_to_date = False
        self._data_on_device = False
        self._dist_plan = None
        self._data_version = getattr(self, "_data_version", 0) + 1
        return removed

    def _batch_gradient_refusal(self):
        """Why :meth:`ll_gradient_batch` (``gpt_ll_grad_diff_batch``) cannot serve this model, or ``None``: a reason of
        :meth:`_ll_gradient_refusal`, a linear transform, or more points than the batched evaluator takes."""
        why = self._ll_gradient_refusal()
        if why is not None:
            return why
        if self.T is not None:
            return "a linear transform T (the batched gradient has no transformed pair pass)"
        if self.X is not None and max(len(self.y), self.X.shape[0]) > self.batch_grid_max_n:
            return "N = %d above batch_grid_max_n = %d (one evaluation fills the GPU there)" % (len(self.y), self.batch_grid_max_n)
        return None

    def ll_gradient_batch(self, param_list, rel_step=6e-6, exit_on_bounds=True):
        """Log-posterior and its gradient at each free-parameter vector of ``param_list``: ``(ll (B,), grad (B, nfree))`` with
        ``ll[i]`` what :meth:`ll_batch` gives -- ``-update_hyperparameters(p_i)`` bit for bit -- and ``grad[i]`` what
        :meth:`ll_gradient` gives at ``p_i``, from ONE launch sequence per chunk of ``batch_grid`` points: the batched fit and,
        while its factors are resident, ``gpt_ll_grad_diff_batch`` (``U = L^-T``, ``U U^T``, alpha and the pair passes with the
        batch in a grid dimension, one host synchronisation).  The round of a multi-start optimiser in lockstep
        (``optimize_hyperparameters(batch_starts=True)``).

        A row the prior excludes (``exit_on_bounds``) or whose fit fails has ``ll = -inf`` and a NaN gradient.  A row whose
        stencil differs in shape from the first one's (a parameter pinned between its bounds) and a chunk the library rejects go
        through :meth:`update_hyperparameters` and :meth:`ll_gradient` one by one.  The GP's own hyperparameters are left as
        they were.  ``NotImplementedError`` for what :meth:`ll_gradient` refuses, for a transform ``T`` and above
        ``batch_grid_max_n`` points."""
        why = self._batch_gradient_refusal()
        if why is not None:
            raise NotImplementedError("ll_gradient_batch is not available for %s" % why)
        if self.X is None:
            raise GPArgumentError("No data have been added to the GaussianProcess!")
        param_list = [np.array(p, dtype=float) for p in param_list]
        ll = np.full(len(param_list), -np.inf)
        grad = np.full((len(param_list), len(self.free_params)), np.nan)
        if not param_list:
            return ll, grad
        own, up_to_date = np.array(self.free_params[:], dtype=float), self.K_up_to_date
        disturbed = [False]                                   # the single route ran: the GP's own factor is gone

        def single(row):
            disturbed[0] = True
            v = self.update_hyperparameters(param_list[row], hyper_deriv_handling="value", exit_on_bounds=exit_on_bounds)
            ll[row] = -1.0 * v
            if np.isfinite(v):
                try:
                    grad[row] = self.ll_gradient(rel_step)
                except Exception:
                    warnings.warn("the device gradient failed at free hyperparameters %s, where the log-posterior is %.6g:\n%s"
                                  % (param_list[row], -v, traceback.format_exc()), RuntimeWarning)

        try:
            # host part, in order (the kernel / mean objects are shared): every point's device model and stencil
            jobs = []
            for i, p in enumerate(param_list):
                self._assign_free(p)
                prior = self.hyperprior(self.params)
                if exit_on_bounds and np.isinf(prior):
                    continue
                try:
                    stencil = self._ll_gradient_stencil(rel_step)
                except (np.linalg.LinAlgError, ValueError, ArithmeticError):
                    stencil = None                              # (a stencil point whose device parameters need a solve that failed)
                job = self._batch_job(i, (prior, stencil))
                if job is not None:
                    jobs.append(job)
            ref = next(((j.extra[1][0], j.extra[1][1]) for j in jobs if j.extra[1] is not None), None)
            ctx = self._resident_ctx()
            NP, per = self._batch_element_bytes(False)

            def done(chunk, llv, info):
                same = np.array([j.extra[1] is not None and (j.extra[1][0], j.extra[1][1]) == ref for j in chunk])
                keep = (np.asarray(info) == 0) & same
                for j, l, bad in zip(chunk, llv, info):
                    if bad == 0:
                        ll[j.row] = l + j.extra[0]
                out = alpha = None
                if keep.any():
                    # (rows that are not kept are not read by the library: they carry a kept row's stencil for the length checks)
                    fill = chunk[int(np.argmax(keep))].extra[1]
                    st = [j.extra[1] if k else fill for j, k in zip(chunk, keep)]
                    try:
                        out, alpha = ctx.ll_grad_diff_batch(ref[1], [s[2] for s in st], [s[3] for s in st], [s[4] for s in st], keep,
                                                            want_alpha=self.mu is not None)
                    except (ValueError, ArithmeticError, NotImplementedError):
                        keep[:] = False                         # the library rejects the chunk: its rows one by one
                for e, j in enumerate(chunk):
                    if keep[e]:
                        self._assign_free(param_list[j.row])
                        grad[j.row] = self._ll_gradient_assemble(ref[0], out[e], lambda: alpha[e])
                    elif info[e] == 0:
                        single(j.row)

            # (a lockstep optimisation holds the scratch over its rounds: returning and allocating gigabytes every round cost five
            # times the rounds' own work at N = 4096 x 32 starts)
            left = self._fit_batched(jobs, per + 16 * NP * NP, 0 if self._hold_batch_scratch else 24 * NP * NP, done,
                                     lambda chunk: [single(j.row) for j in chunk])
            for j in left:
                single(j.row)
        finally:
            self._assign_free(own)
            self.K_up_to_date = up_to_date and not disturbed[0]
        return ll, grad

    def _device_grad_objective(self):
        """``(fun, jac)`` for scipy.optimize.minimize: ``fun`` is ``update_hyperparameters``, ``jac`` minus :meth:`ll_gradient`
        at the same point (zeros where the value is ``+inf``)."""
        last = {}

        def fun(x):
            x = np.array(x, dtype=float)
            v = self.update_hyperparameters(x, hyper_deriv_handling="value")
            last["x"], last["f"] = x, v
            return v

        def jac(x):
            x = np.array(x, dtype=float)
            f0 = last["f"] if ("x" in last and np.array_equal(last["x"], x)) else fun(x)
            if not np.isfinite(f0):
                return np.zeros(len(x))
            try:
                return -1.0 * self.ll_gradient()
            except Exception:
                # (the optimiser's caller drops a start whose run raised and says so only when verbose: a gradient that fails at a
                # point whose VALUE was finite is reported whatever the setting)
                warnings.warn("the device gradient failed at free hyperparameters %s, where the log-posterior is %.6g:\n%s"
                              % (x, -f0, traceback.format_exc()), RuntimeWarning)
                raise
        return fun, jac

    _hold_batch_scratch = False       # True while a lockstep optimisation runs: ll_gradient_batch keeps its device scratch between rounds

    def _lockstep_starts(self, starts, opt_kwargs):
        """The starts of ``optimize_hyperparameters(batch_starts=True)`` in lockstep (``gptools_amd.multistart``): every round's
        pending points are one :meth:`ll_gradient_batch`.  Returns one result per start, ``None`` for a start whose run raised --
        what the sequential loop's ``run`` returns.  The objective is :meth:`_device_grad_objective`'s: minus the log-posterior,
        ``+inf`` with a zero gradient where the evaluation fails; a gradient that fails where the value is finite ends its start."""
        from .multistart import lockstep_minimize

        def evaluate(points):
            ll, grad = self.ll_gradient_batch(points)
            f = [-1.0 * v for v in ll]
            for i, p in enumerate(points):
                if np.isfinite(f[i]) and not np.all(np.isfinite(grad[i])):
                    f[i] = RuntimeError("the device gradient failed at free hyperparameters %s, where the log-posterior is %.6g"
                                        % (p, ll[i]))
            return f, -1.0 * grad

        self._hold_batch_scratch = True
        try:
            results, _ = lockstep_minimize(list(starts), evaluate, **opt_kwargs)
        finally:
            self._hold_batch_scratch = False
            if 24 * self._batch_element_bytes(False)[0] ** 2 * min(len(starts), int(self.batch_grid)) > (2 << 30):
                self._ctx.release_batch_scratch()            # a large scratch goes back to the device once the starts are done
        if self.verbose:
            for samp, r in zip(starts, results):
                if r is None:
                    warnings.warn("start %s dropped, the optimiser raised" % (samp,), RuntimeWarning)
        return results

    # ---- hyperparameter update (ref: gptools/gaussian_process.py:1332-1416) -------------------
    def _assign_free(self, values):
        """Distribute a vector of FREE hyperparameters over the kernel, the noise kernel and the mean function, in the
        order ``free_params`` lists them (ref: gaussian_process.py:1377-1384)."""
        values = np.asarray(values, dtype=float)
        at = 0
        for part in self._parts():
            cnt = len(part.free_params)
            part.set_hyperparams(values[at:at + cnt])
            at += cnt
        self.K_up_to_date = False

    def update_hyperparameters(self, new_params, hyper_deriv_handling="default", exit_on_bounds=True,
                               inf_on_error=True):
        """Set the free hyperparameters and evaluate the negative log-posterior there -- the objective an optimiser
        minimises (ref: gptools/gaussian_process.py:1332-1416).

        Returns ``-ll``; ``(-ll, -ll_deriv)`` when the GP uses hyperparameter derivatives; ``hyper_deriv_handling`` =
        ``'value'`` / ``'deriv'`` asks for one of the two alone whatever the GP's setting.  Hyperparameters the prior
        rules out (``exit_on_bounds``) and any failure of the evaluation -- a covariance matrix that is not positive
        definite above all -- count as ``+inf`` (gradient: zeros) while ``inf_on_error`` is set; otherwise they raise."""
        want_value = hyper_deriv_handling != "deriv"
        want_deriv = hyper_deriv_handling == "deriv" or (hyper_deriv_handling == "default" and self.use_hyper_deriv)
        configured = self.use_hyper_deriv
        self.use_hyper_deriv = want_deriv
        try:
            self._assign_free(new_params)
            if exit_on_bounds and np.isinf(self.hyperprior(self.params)):
                raise GPImpossibleParamsError("the hyperprior excludes these hyperparameters")
            self.compute_K_L_alpha_ll(need_factor=False)
            value, deriv = -1.0 * self.ll, (-1.0 * self.ll_deriv if want_deriv else None)
        except Exception as exc:
            if not inf_on_error:
                raise
            if self.verbose and not isinstance(exc, GPImpossibleParamsError):
                warnings.warn("evaluation failed at free hyperparameters %s and counts as +inf:\n%s"
                              % (self.free_params[:], traceback.format_exc()))
            value, deriv = np.inf, np.zeros(len(self.free_params))
        finally:
            self.use_hyper_deriv = configured
        if want_value and want_deriv:
            return (value, deriv)
        return value if want_value else deriv

    # ---- independent evaluations (ref: gptools/gaussian_process.py:1607-1692) ----
    #: independent LML evaluations kept in flight on one GPU.  While one factorisation is in its latency-bound tail
    #: (panel chain, most CUs idle) another is in its update-bound head: measured on MI355X, 2 in flight give
    #: 211 evaluations/s against 164 at N=8192 and 811 against 476 at N=4096; more than 2 lose again (the
    #: diagonal-block kernels compete for the CUs reserved for them).
    batch_concurrency = 2
    #: at most this many points: ll_batch (hence compute_ll_matrix, the finite-difference gradients of
    #: optimize_hyperparameters) evaluates ``batch_grid`` hyperparameter vectors per launch sequence (gpt_fit_batch) instead
    #: of one per context and host thread; measured on MI355X at N = 1024: see DESIGN.md section 7.2
    batch_grid_max_n = 4096
    #: device memory the batch's matrices may take (bytes): the chunk size is batch_grid or what fits, whichever is smaller
    batch_grid_bytes = 16 << 30
    batch_grid = 256                                          # (measured: N = 256 262 k / 569 k / 699 k evaluations/s at 64 / 256 / 1024
                                                              #  per launch sequence, N = 1024 45 k / 62 k / 64 k at 64 / 256 / 512)

    def _batch_contexts(self, count):
        self._ctx                                            # creates the pool together with the main context
        pool = self._ctx_pool
        while len(pool) < count - 1:                         # batch_concurrency raised later: late contexts (slower)
            pool.append([_lib.Context(self.device), -1])
        return pool

    def ll_batch(self, param_list, exit_on_bounds=True):
        """Log-posterior at each free-parameter vector of ``param_list`` -- what ``-update_hyperparameters(p)``
        returns for every ``p`` (``-inf`` where that gives ``+inf``) -- with ``batch_concurrency`` evaluations in
        flight on this GPU and, under a ``torch.distributed`` job, the list spread over the ranks
        (``gptools_amd.replicas``).  The GP's own hyperparameters are left unchanged."""
        param_list = [np.asarray(p, dtype=float) for p in param_list]
        keep = np.array(self.free_params[:], dtype=float)
        world = replicas.world_size()
        # Independent evaluations are never partitioned: the ranks evaluate DIFFERENT hyperparameters here (their slices
        # of the list), and a partitioned evaluation is a collective that every rank must enter with the same ones.
        keep_partitioned = self.partitioned
        self.partitioned = False
        try:
            if world > 1 and len(param_list) > 1:
                import torch.distributed as dist
                rank = dist.get_rank()
                mine = self._ll_batch_local(param_list[rank::world], exit_on_bounds)
                parts = replicas.distributed_map(lambda r: mine if r == rank else None, range(world))
                out = np.empty(len(param_list))
                for r in range(world):
                    out[r::world] = parts[r]
                return out
            return self._ll_batch_local(param_list, exit_on_bounds)
        finally:
            self._assign_free(keep)
            self.partitioned = keep_partitioned

    def _ll_rows(self, param_list):
        """The log-posterior at every row of ``param_list`` for the callers that walk many points (``compute_ll_matrix``, the
        host-stepped sampler): :meth:`ll_batch`; a subclass without a batched evaluator answers row by row."""
        return self.ll_batch(param_list)

    def _batch_job(self, row, extra):
        """The current hyperparameters as one element of a batched fit; ``None`` for a kernel whose device parameters need a solve
        that failed (the evaluation fails: the caller drops the row)."""
        try:
            terms, layers = self._device_model()
        except np.linalg.LinAlgError:
            return None
        return _BatchJob(row, terms, layers, self._noise_var(), np.array(self._y_alph(), dtype=float), extra)

    def _batch_element_bytes(self, warped):
        """``(NP, bytes)``: the padded order of one element of a batched fit and the device memory it takes."""
        NP = -(-(len(self.y) + 1) // 128) * 128
        per = 8 * NP * NP + 8 * 9216 * (NP // 128) + (8 * self.X.shape[0] * (self.num_dim + 1) if warped else 0)
        if self.T is not None:                               # + every element's K over the latent points and T K
            NxP = -(-self.X.shape[0] // 16) * 16
            per += 8 * NxP * NxP + 8 * (-(-len(self.y) // 64) * 64) * NxP
        return NP, per

    def _batch_chunk(self, ctx, per):
        """Elements of one launch sequence: ``batch_grid``, or as many as fit ``batch_grid_bytes`` and half of the free memory."""
        return max(1, min(int(self.batch_grid), min(int(self.batch_grid_bytes), ctx.mem_info()[0] // 2) // per))

    def _fit_batched(self, jobs, per, release_per, done, rejected):
        """The chunk loop of the batched routes (ll_batch, compute_from_MCMC): ``jobs`` through ``gpt_fit_batch_terms``,
        ``batch_grid`` per launch sequence or as many as fit ``batch_grid_bytes`` and HALF of the device memory free right now (other
        ranks / processes may share the GPU) at ``per`` bytes an element -- and should the allocation still fail, half as many.
        ``done(chunk, ll, info)`` takes a fitted chunk while it is resident; ``rejected(chunk)`` one the library refused (an argument
        of ONE element, e.g. a kernel parameter out of its domain, fails the whole call).  A scratch above 2 GiB (``release_per`` bytes
        an element) goes back at the end.  Returns the jobs NOT evaluated: all when they are not one model shape, the remainder
        when not even one element fits."""
        if not jobs:
            return []
        ctx, first = self._resident_ctx(), jobs[0]
        if any(_terms_shape(j.terms) != _terms_shape(first.terms) or [t for t, _ in j.layers] != [t for t, _ in first.layers]
               for j in jobs):
            return jobs
        self._cache = {}
        err_y = np.asarray(self.err_y, dtype=float)
        diag_add = self.diag_factor * sys.float_info.epsilon
        G = self._batch_chunk(ctx, per)
        s0 = 0
        while s0 < len(jobs) and G >= 1:
            chunk = jobs[s0:s0 + G]
            try:
                if first.layers:
                    ctx.set_warp_batch([j.layers for j in chunk])
                else:
                    ctx.set_warp(None)                       # (layers an earlier warped model left on the context)
                ll, _, info = ctx.fit_batch_terms([j.terms for j in chunk], np.array([j.noise_var for j in chunk]),
                                                  np.array([j.y_alph for j in chunk]), err_y, diag_add)
                done(chunk, ll, info)
            except MemoryError:
                ctx.release_batch_scratch()
                G //= 2
                continue
            except (ValueError, ArithmeticError):
                rejected(chunk)
            s0 += len(chunk)
        if release_per * min(G, len(jobs)) > (2 << 30):
            ctx.release_batch_scratch()                      # a large scratch goes back to the device once the list is done
        return jobs[s0:]

    def _ll_batch_local(self, param_list, exit_on_bounds):
        out = np.full(len(param_list), -np.inf)
        if not param_list:
            return out
        if self.X is None:
            raise GPArgumentError("No data have been added to the GaussianProcess!")
        B = max(1, int(self.batch_concurrency))
        if B == 1 or len(param_list) == 1 or not self._fast_fit_possible():
            for i, p in enumerate(param_list):
                out[i] = -1.0 * self.update_hyperparameters(p, hyper_deriv_handling="value",
                                                            exit_on_bounds=exit_on_bounds)
            return out
        # host part, in order: the kernel / mean objects are shared, so the numeric inputs of every evaluation are
        # extracted one after another; only the GPU work overlaps
        diag_add = self.diag_factor * sys.float_info.epsilon
        jobs = []
        for i, p in enumerate(param_list):
            self._assign_free(p)
            prior = self.hyperprior(self.params)
            if exit_on_bounds and np.isinf(prior):
                continue                                            # impossible parameters: stays -inf
            job = self._batch_job(i, prior)
            if job is not None:
                jobs.append(job)
        if not jobs:
            return out

        def fit_one(ctx, j):
            try:
                ctx.set_warp(j.layers)
                out[j.row] = self._device_fit(ctx, j.terms, j.noise_var, j.y_alph, diag_add)[0] + j.extra
            except (np.linalg.LinAlgError, ValueError, ArithmeticError):
                pass                                                # the +inf policy of update_hyperparameters

        if max(len(self.y), self.X.shape[0]) <= self.batch_grid_max_n and int(self.batch_grid) > 1:
            # small N: the whole batch in ONE launch sequence (gpt_fit_batch_terms: every kernel of the factorisation carries the
            # batch in a grid dimension), batch_grid evaluations at a time; bit-identical to one gpt_fit_terms per vector.  Any
            # model of native kernels -- sums, products, with or without the linear transform T (the reference's
            # grids take any model: ref gaussian_process.py:1607-1692).  A warped model: the elements' warp parameters differ,
            # set_warp_batch gives every element its own warped points
            NP, per = self._batch_element_bytes(bool(jobs[0].layers))

            def store(chunk, ll, info):
                for j, l, bad in zip(chunk, ll, info):
                    if bad == 0:
                        out[j.row] = l + j.extra

            # (a chunk the library rejects: one vector at a time)
            jobs = self._fit_batched(jobs, per, 8 * NP * NP, store, lambda chunk: [fit_one(self._ctx, j) for j in chunk])
            if not jobs:
                return out                                       # (else no chunk size fits: the rest one context per thread)
        version = getattr(self, "_data_version", 0)
        ctxs = [[self._resident_ctx(), version]] + self._batch_contexts(B)
        for c in ctxs[1:]:
            if c[1] != version:                                      # data added since this context last saw it
                self._upload_data(c[0])
                c[1] = version
        self._cache = {}
        import threading
        lock = threading.Lock()
        it = iter(jobs)

        def worker(ctx):
            while True:
                with lock:
                    job = next(it, None)
                if job is None:
                    return
                fit_one(ctx, job)
        threads = [threading.Thread(target=worker, args=(c[0],)) for c in ctxs[:B]]
        with _lib.concurrent_evaluations():          # several chains at once: event edges (include/gpt_hip.h)
            for t in threads:
                t.start()
            for t in threads:
                t.join()
        return out

    def _batched_fd(self, eps, bounds):
        """``(fun, jac)`` for scipy.optimize.minimize: ``fun`` is ``update_hyperparameters``; ``jac`` is the
        forward-difference gradient scipy would form itself (``approx_derivative(..., '2-point', abs_step=eps,
        bounds=...)``), with the perturbed points evaluated through the batched evaluator.  scipy's routine is run
        twice -- once to record the points it asks for, once on the cached values -- so step signs near bounds and
        the rounding of ``(x + h) - x`` are exactly its own."""
        from scipy.optimize._numdiff import approx_derivative
        last = {}

        def fun(x):
            x = np.array(x, dtype=float)
            v = self.update_hyperparameters(x)
            last["x"], last["f"] = x, v
            return v

        def jac(x):
            x = np.array(x, dtype=float)
            f0 = last["f"] if ("x" in last and np.array_equal(last["x"], x)) else fun(x)
            kw = dict(method="2-point", abs_step=eps, f0=f0, bounds=(bounds[:, 0], bounds[:, 1]))
            pts = []
            approx_derivative(lambda z: (pts.append(np.array(z, dtype=float)), 0.0)[1], x, **kw)
            vals = -1.0 * self._ll_batch_local(pts, True)
            self._assign_free(x)                                 # back to the expansion point
            table = {p.tobytes(): v for p, v in zip(pts, vals)}
            return approx_derivative(lambda z: table[np.array(z, dtype=float).tobytes()], x, **kw)
        return fun, jac

    def compute_ll_matrix(self, bounds, num_pts):
        """Log-posterior on a regular grid over the free hyperparameters (ref: gptools/gaussian_process.py:1607-1692).

        ``bounds``: one ``(low, high)`` pair for all free hyperparameters or one pair each; ``num_pts``: one count or
        one per hyperparameter.  Returns ``(ll_vals, param_vals)``: the grid axes ``param_vals[i] = linspace(low_i,
        high_i, num_pts[i])`` and ``ll_vals`` of shape ``num_pts`` (axis i = free hyperparameter i; ``-inf`` where the
        prior excludes the point or the evaluation fails).  The reference walks the grid recursively, one evaluation
        at a time; here all points go through :meth:`ll_batch`.  The GP is left at its present hyperparameters."""
        here = np.array(self.free_params[:], dtype=float)
        nfree = here.size
        box = np.asarray(bounds, dtype=float)
        if box.ndim == 1:
            box = box[None, :]
        if box.ndim != 2 or box.shape[1] != 2:
            raise ValueError("bounds must be a (low, high) pair or one pair per free hyperparameter")
        if box.shape[0] == 1:
            box = np.repeat(box, nfree, axis=0)
        counts = np.asarray(num_pts, dtype=int)
        if counts.ndim == 0:
            counts = np.full(box.shape[0], int(counts))
        elif counts.size != nfree:
            raise ValueError("num_pts lists %d counts for %d free hyperparameters" % (counts.size, nfree))
        axes = [np.linspace(lo, hi, c) for (lo, hi), c in zip(box[:nfree], counts)]
        mesh = np.meshgrid(*axes, indexing="ij")
        points = np.column_stack([m.ravel() for m in mesh])
        ll_vals = self._ll_rows(list(points)).reshape([int(c) for c in counts[:nfree]])
        self.update_hyperparameters(here)
        return (ll_vals, axes)

    # ---- samples of the hyperparameter posterior (ref: gptools/gaussian_process.py:1694-1838) --
    def _library_stepping(self):
        """What ``gpt_ensemble_run`` needs to step an ensemble over this GP's free hyperparameters: ``(None, plan)`` with the
        plan a dict of :meth:`_lib.Context.ensemble_run`'s model arguments -- or ``(refusal, None)``, the refusal a sentence
        that names what keeps the model on the host route.  No device call."""
        try:
            model = self._device_model()
        except np.linalg.LinAlgError:
            return "the kernel's device parameters need a host solve, which failed at the current hyperparameters", None
        if model is None:
            return ("the covariance kernel is not one the library evaluates itself (a Python-defined kernel, or a tree of kernels "
                    "it does not take)"), None
        terms, layers = model
        if layers:
            return "the kernel has input-warp layers (WarpedKernel): the library route steps plain models only", None
        if not isinstance(self.noise_k, (ZeroKernel, DiagonalNoiseKernel)) or len(self.noise_k.params) != 1:
            return "the noise kernel is neither ZeroKernel nor DiagonalNoiseKernel", None
        if self.mu is not None:
            return "the GP has a mean function (mu): its parameters change the targets of every walker", None
        if self.X is None:
            return "no data have been added to the GaussianProcess", None
        if max(len(self.y), self.X.shape[0]) > self.batch_grid_max_n:
            return "more than batch_grid_max_n = %d points: the batched evaluator does not take them" % self.batch_grid_max_n, None
        flat, own = _lib.Context._flat_params(terms), np.array(self.k.params, dtype=float)
        if flat.shape != own.shape or not np.array_equal(flat, own):
            return ("the parameters the library takes for this kernel are not the kernel's hyperparameters element for element (a "
                    "MaskedKernel's expansion, a nested GP's weights): only the host can form them"), None

        def leaves(p):
            return leaves(p.p1) + leaves(p.p2) if type(p) is ProductJointPrior else [p]
        others = sorted(set(type(p).__name__ for p in leaves(self.hyperprior) if type(p) is not UniformJointPrior))
        if others:
            return "the hyperprior is not a product of UniformJointPrior boxes (it holds %s)" % ", ".join(others), None
        fixed = np.asarray(self.fixed_params[:], dtype=bool)
        box = np.array([tuple(b) for b in self.hyperprior.bounds[:]], dtype=float).reshape(-1, 2)[~fixed]
        inside = np.array(self.params[:], dtype=float)
        inside[~fixed] = box[:, 0]
        log_prior = self.hyperprior(inside)                  # (the same sum at every point of the box: one term per bound)
        if not np.isfinite(log_prior):
            return "the box prior has no finite density (an unbounded side, or a fixed hyperparameter outside its bounds)", None
        free_idx = np.flatnonzero(~fixed)                    # (the noise sigma follows the kernel's parameters: index len(flat))
        return None, dict(terms=terms, free_idx=free_idx, lo=box[:, 0], hi=box[:, 1], log_prior=log_prior)

    def _library_stepping_refusal(self):
        """``None`` when ``sample_hyperparameter_posterior(stepping="library")`` can run this model, else the reason."""
        return self._library_stepping()[0]

    #: what ``stepping="auto"`` selects for a model the library route can run (DESIGN.md section 13 has the measurements)
    sampler_auto_route = "library"

    def sample_hyperparameter_posterior(self, nwalkers=200, nsamp=500, burn=0, thin=1, num_proc=None, sampler=None,
                                        plot_posterior=False, plot_chains=False, sampler_type='ensemble', ntemps=20,
                                        sampler_a=2.0, theta0=None, random_state=None, stepping="auto"):
        """Samples of the free hyperparameters from their posterior by an affine-invariant ensemble sampler
        (:class:`gptools_amd.sampler.EnsembleSampler`; ref: gptools/gaussian_process.py:1694-1838, which drives emcee).  Returns
        the sampler: pass it to ``predict_MCMC`` / ``compute_from_MCMC`` (``sampler=``), or back in here to add ``nsamp`` steps.

        ``nwalkers`` walkers take ``nsamp`` steps from ``theta0`` (nwalkers, free parameters) -- default: draws of the hyperprior
        -- or from where ``sampler``'s chain ends.  The log-probability of a row is what :meth:`ll_batch` returns for it.
        ``sampler``: an ``EnsembleSampler`` of this package, or any object with ``run_mcmc`` and ``chain`` (then
        ``run_mcmc(theta0, nsamp)`` is all that is called).  ``random_state``: a ``numpy.random.RandomState`` or a seed for the
        sampler's moves.  ``burn`` only enters the summary printed when the GP is ``verbose``; ``thin``, ``num_proc`` and
        ``ntemps`` are accepted for compatibility.  Plots and ``sampler_type='pt'`` are not implemented.

        ``stepping``: ``"host"`` -- the loop runs in Python, every half-ensemble through :meth:`ll_batch` (any model);
        ``"library"`` -- the whole loop runs inside the HIP library (``gpt_ensemble_run``) for a plain model: native kernels
        without warp, ``ZeroKernel`` / ``DiagonalNoiseKernel`` noise, no mean function, a prior that is a product of
        ``UniformJointPrior`` boxes (``ValueError`` names what is in the way otherwise); ``"auto"``: ``sampler_auto_route`` where
        the model allows it, else the host loop.  Both give the same chain bit for bit.  Unlike the reference, the GP keeps its
        own hyperparameters."""
        from .sampler import EnsembleSampler
        from .utils import summarize_sampler
        if sampler_type != 'ensemble':
            raise NotImplementedError("Sampler type {} not supported!".format(sampler_type))
        if plot_posterior or plot_chains:
            raise NotImplementedError("plots are not part of this package: plot sampler.chain yourself")
        if stepping not in ("auto", "host", "library"):
            raise ValueError("stepping must be 'auto', 'host' or 'library'")
        ours = sampler is None or isinstance(sampler, EnsembleSampler)
        plan = None
        if ours and stepping != "host":
            refusal, plan = self._library_stepping()
            if stepping == "library" and refusal is not None:
                raise ValueError("stepping='library': " + refusal)
            if stepping == "auto" and self.sampler_auto_route != "library":
                plan = None
        elif stepping == "library":
            raise ValueError("stepping='library' needs this package's EnsembleSampler, not a foreign sampler")
        if self.X is None:
            raise GPArgumentError("No data have been added to the GaussianProcess!")
        ctx = self._resident_ctx()                           # (no device: GPTBackendError here, not a chain of -inf)
        ndim = len(self.free_params)

        def lnprob(P):
            return self._ll_rows(list(np.atleast_2d(P)))
        if sampler is None:
            sampler = EnsembleSampler(nwalkers, ndim, lnprob, a=sampler_a, random_state=random_state)
        else:
            sampler.a = sampler_a
            if ours:
                sampler.lnprob_batch = lnprob
                if random_state is not None:
                    sampler.random_state = (random_state if isinstance(random_state, np.random.RandomState)
                                            else np.random.RandomState(random_state))
        lnprob0 = None
        if np.asarray(sampler.chain).size == 0:
            if theta0 is None:
                fixed = np.asarray(self.fixed_params[:], dtype=bool)
                theta0 = self.hyperprior.random_draw(size=sampler.k if ours else nwalkers).T[:, ~fixed]
        else:
            theta0 = sampler.chain[:, -1, :]                 # from where the chain ends (ref :1784-1785)
            lnprob0 = sampler._last_lnprob if ours else None
        saved = np.array(self.free_params[:], dtype=float)
        was_current, fit_mode = self.K_up_to_date, self._fit_mode
        try:
            if not ours:
                sampler.run_mcmc(theta0, nsamp)
            else:
                if plan is not None:
                    _, per = self._batch_element_bytes(False)
                    diag_add = self.diag_factor * sys.float_info.epsilon

                    def stepper(pos, lnp, a, u_stretch, partner, u_accept):
                        ctx.set_warp(None)                   # (layers an earlier warped model left on the context)
                        self._cache = {}
                        return ctx.ensemble_run(plan["terms"], plan["free_idx"], plan["lo"], plan["hi"], plan["log_prior"],
                                                self._noise_var(), self.y, self.err_y, diag_add, a, u_stretch, partner, u_accept,
                                                pos, lnp, self._batch_chunk(ctx, per))
                    stepper.route = "library"
                    sampler.stepper = stepper
                try:
                    sampler.run_mcmc(theta0, nsamp, lnprob0=lnprob0)
                finally:
                    sampler.stepper = None
        finally:
            # the GP as it was: its hyperparameters, and the factor of K_tot at them where it had one
            self._assign_free(saved)
            if was_current:
                self.compute_K_L_alpha_ll(need_factor=fit_mode != "partitioned")
        if self.verbose:
            print("MCMC parameter summary:")
            print("param\tmean\t95% posterior interval")
            for name, m, lo, hi in zip(self.free_param_names[:], *summarize_sampler(sampler, burn=burn)):
                print("{:s}\t{:4.4g}\t[{:4.4g}, {:4.4g}]".format(str(name), m, lo, hi))
        return sampler

    # ---- MAP estimate (ref: gptools/gaussian_process.py:623-783, :2443-2486) ------------------
    def optimize_hyperparameters(self, method="SLSQP", opt_kwargs={}, verbose=False, random_starts=None,
                                 num_proc=None, max_tries=1, batch_fd=None, gradient=None, batch_starts=False, objective="ll"):
        """Maximise the log-posterior with ``scipy.optimize.minimize`` from ``random_starts`` draws
        of the hyperprior (0: start from the current values).  Every objective evaluation is one GPU
        fit.  ``num_proc`` is accepted for compatibility: a HIP context must not be shared across forked
        workers, so inside one process the starts run one after another; under a ``torch.distributed`` job
        (one process per GPU) they are spread over the ranks instead (``gptools_amd.replicas``) and every
        rank returns the same best result.

        ``gradient="device"``: the optimiser is given ``jac`` = minus :meth:`ll_gradient` -- one fit, ``K_tot^-1`` and two passes
        over the pairs per free kernel parameter, for every model of native kernels -- instead of finite differences of the
        objective at one fit per free parameter (``None``, the default).  Independent of ``use_hyper_deriv`` (the analytic
        gradient of squared-exponential models), with which it cannot be combined.

        ``batch_starts=True`` (with ``gradient="device"``, more than one start and SLSQP, L-BFGS-B or TNC): the starts run in
        lockstep (``gptools_amd.multistart``) -- one thread per start, and every round's pending points of ALL starts are one
        :meth:`ll_gradient_batch`, a single launch sequence, instead of one fit and one gradient per start and evaluation.  The
        starts, ``max_tries``, the choice of the best result, the warnings and the return value are those of the sequential loop.
        ``NotImplementedError`` for a model :meth:`ll_gradient_batch` refuses; ``ValueError`` under a ``torch.distributed`` job
        of more than one rank.

        ``objective="loo"``: maximise the leave-one-out log predictive probability plus the log hyperprior
        (:meth:`loo_log_likelihood`) instead of the log-posterior (``"ll"``, the default).  With ``gradient="device"`` the value
        and ``jac`` of a point come from one ``gpt_loo_grad_diff`` call (:meth:`loo_gradient`); with ``gradient=None`` scipy
        differences the objective itself, one fit per evaluation.  ``ValueError`` together with ``batch_starts=True``,
        ``use_hyper_deriv`` or a ``jac`` of the caller's; the hyperparameters the optimiser ends at are kept, ``ll`` is the
        log-posterior there."""
        if gradient not in (None, "device"):
            raise ValueError("gradient must be None or 'device', got %r" % (gradient,))
        if objective not in ("ll", "loo"):
            raise ValueError("objective must be 'll' or 'loo', got %r" % (objective,))
        loo = objective == "loo"
        if loo:
            if batch_starts:
                raise ValueError("objective='loo' cannot be combined with batch_starts=True: there is no batched leave-one-out")
            if self.use_hyper_deriv or "jac" in (opt_kwargs or {}):
                raise ValueError("objective='loo' cannot be combined with use_hyper_deriv or a jac of the caller's")
            if gradient == "device":
                why = self._loo_gradient_refusal()
                if why is not None:
                    raise NotImplementedError("objective='loo' with gradient='device' is not available for %s" % why)
        if batch_starts:
            nstarts = 1 if random_starts == 0 else (max(num_proc or 1, 1) if random_starts is None else int(random_starts))
            chosen = (opt_kwargs or {}).get("method", method)
            if gradient != "device":
                raise ValueError("batch_starts=True needs gradient='device': the starts share one batched gradient per round")
            if nstarts < 2:
                raise ValueError("batch_starts=True needs more than one start (random_starts >= 2)")
            if chosen not in ("SLSQP", "L-BFGS-B", "TNC"):
                raise ValueError("batch_starts=True takes the methods SLSQP, L-BFGS-B and TNC, got %r" % (chosen,))
            if self.use_hyper_deriv or "jac" in (opt_kwargs or {}):
                raise ValueError("gradient='device' cannot be combined with use_hyper_deriv or a jac of the caller's")
            if replicas.world_size() > 1:
                raise ValueError("batch_starts=True is not available under a torch.distributed job of more than one rank")
            why = self._batch_gradient_refusal()
            if why is not None:
                raise NotImplementedError("batch_starts=True is not available for %s" % why)
        if gradient == "device":
            if self.use_hyper_deriv or "jac" in (opt_kwargs or {}):
                raise ValueError("gradient='device' cannot be combined with use_hyper_deriv or a jac of the caller's")
            why = self._ll_gradient_refusal()
            if why is not None:
                raise NotImplementedError("gradient='device' is not available for %s" % why)
            self._ctx                          # (no device: GPTBackendError here, not a +inf objective at every start)
        opt_kwargs = dict(opt_kwargs or {})
        if "method" in opt_kwargs:
            method = opt_kwargs["method"]
        else:
            opt_kwargs["method"] = method
        if num_proc is None:
            num_proc = 1
        param_ranges = np.array(self.free_param_bounds[:], dtype=float)
        lo, hi = param_ranges[:, 0], param_ranges[:, 1]
        lo[np.isnan(lo) | np.isinf(lo)] = -1e16
        hi[np.isnan(hi) | np.isinf(hi)] = 1e16
        free_mask = ~np.asarray(self.fixed_params[:], dtype=bool)

        def draw():
            return np.atleast_2d(self.hyperprior.random_draw(size=random_starts).T)[:, free_mask]

        if random_starts == 0:
            param_samples = [np.array(self.free_params[:], dtype=float)]
        else:
            if random_starts is None:
                random_starts = max(num_proc, 1)
            param_samples = draw()
        opt_kwargs.setdefault("bounds", param_ranges)
        if self.use_hyper_deriv:
            opt_kwargs["jac"] = True

        target = self.update_hyperparameters
        # Finite-difference gradients (what scipy does itself when no `jac` is given) through ll_batch: the p
        # perturbed points of one gradient are independent evaluations, kept two in flight on the GPU.  The points
        # and the difference formula are scipy's own (approx_derivative is replayed), so the iterates are the same.
        fd_eps = {"L-BFGS-B": 1e-8, "TNC": 1e-8, "SLSQP": 1.4901161193847656e-08}
        partitioned = self._partitioned_possible()       # every evaluation is a collective: no local batching,
        if loo:
            target, loo_jac = self._loo_objective(gradient == "device")
            if loo_jac is not None:
                opt_kwargs["jac"] = loo_jac
        elif gradient == "device" and not batch_starts:
            target, opt_kwargs["jac"] = self._device_grad_objective()
        elif (not batch_starts and batch_fd is not False and int(self.batch_concurrency) > 1 and not self.use_hyper_deriv and not partitioned
                and "jac" not in opt_kwargs and method in fd_eps and self._fast_fit_possible()):
            eps = (opt_kwargs.get("options") or {}).get("eps", fd_eps[method])
            target, opt_kwargs["jac"] = self._batched_fd(eps, np.asarray(opt_kwargs["bounds"], dtype=float))

        def run(samp):
            try:
                return scipy.optimize.minimize(target, samp, **opt_kwargs)
            except Exception:
                if self.verbose:
                    warnings.warn("start %s dropped, the optimiser raised (free hyperparameters now %s):\n%s"
                                  % (samp, self.free_params[:], traceback.format_exc()), RuntimeWarning)
                return None

        best, finished = None, []
        for attempt in range(max(int(max_tries), 0)):
            if attempt > 0 and random_starts != 0:
                param_samples = draw()                        # nothing usable last time: fresh draws
            if partitioned and replicas.world_size() > 1:
                # ... and every rank walks all the starts (rank 0's draws), in the same order
                param_samples = list(replicas.shared(np.asarray(param_samples)))
                outcomes = [run(s) for s in param_samples]
            elif replicas.world_size() > 1 and len(param_samples) > 1:
                # one start per GPU: the ranks of the torch.distributed job replace the reference's process pool
                param_samples = replicas.shared(np.asarray(param_samples))
                outcomes = replicas.distributed_map(run, list(param_samples))
            elif batch_starts:
                outcomes = self._lockstep_starts(param_samples, opt_kwargs)
            else:
                outcomes = [run(s) for s in param_samples]
            finished = [r for r in outcomes if r is not None]
            usable = [r for r in finished if np.isfinite(r.fun)]
            if usable:
                best = min(usable, key=lambda r: r.fun)
                break
        if best is None:
            raise ValueError("no start of the optimiser ended at a finite log-posterior; widen or shift the parameter "
                             "bounds, start elsewhere or use more random starts")
        self.update_hyperparameters(best.x)
        if verbose:
            print("%d starts completed; the best one:" % len(finished))
            print(best)
            print("%s %.6g" % ("leave-one-out log probability + log prior" if loo else "log-posterior", -best.fun))
            for name, v in zip(self.free_param_names[:], best.x):
                print("  %s = %.6g" % (str(name).replace("\\", ""), v))
        if not best.success:
            warnings.warn("%s stopped without converging (status %s: %s); the hyperparameters it ended at are kept but "
                          "are probably not the optimum -- other bounds, starting points or more random starts may help"
                          % (method, best.status, best.message), RuntimeWarning)
        box = np.asarray(self.free_param_bounds[:], dtype=float)
        # (within 0.1 % of an edge counts as on it, as in the reference)
        if np.any(best.x <= 1.001 * box[:, 0]) or np.any(best.x >= 0.999 * box[:, 1]):
            warnings.warn("the optimum sits on the edge of the parameter bounds\n%s\nat %s: the bounds, not the data, "
                          "decided it" % (box, best.x))
        return (best, len(finished))

    # ---- prediction (ref: gptools/gaussian_process.py:785-1034) ------------------------------
    def _check_predict_args(self, Xstar, n, output_transform=None):
        """Test points, their derivative orders and the optional output transform in the layout ``gpt_predict`` takes
        (forms accepted: ``gptools_amd._ingest``; ref: gaussian_process.py:913-963)."""
        Xstar = _ingest.points(Xstar, self.num_dim, "Xstar")
        n = _ingest.derivative_orders(n, Xstar, self.num_dim, column_rule="row")
        if output_transform is not None:
            output_transform = _ingest.linear_map(output_transform, None, Xstar.shape[0], "output_transform")
        return Xstar, n, output_transform

    def predict(self, Xstar, n=0, noise=False, return_std=True, return_cov=False, full_output=False,
                return_samples=False, num_samples=1, samp_kwargs={}, return_mean_func=False, use_MCMC=False,
                full_MC=False, rejection_func=None, ddof=1, output_transform=None, **kwargs):
        """Predictive mean (and std / covariance) at ``Xstar`` (M, D) for derivative orders ``n``.

        Returns ``mean``, ``(mean, std)``, ``(mean, cov)`` or the ``full_output`` dict exactly like the
        reference's non-MCMC branch (``return_samples`` / ``full_MC`` draw through :meth:`draw_sample`).  ``use_MCMC``:
        the prediction marginalised over a trace of the hyperparameters -- :meth:`predict_MCMC` with ``flat_trace`` (or
        ``sampler``), ``burn``, ``thin`` among the keyword arguments, as the reference forwards it (ref :888-912)."""
        if use_MCMC:
            res = self.predict_MCMC(Xstar, n=n, noise=noise, return_std=return_std or full_output,
                                    return_cov=return_cov or full_output,
                                    return_samples=full_output and bool(return_samples or rejection_func),
                                    return_mean_func=full_output and return_mean_func, num_samples=num_samples,
                                    samp_kwargs=samp_kwargs, full_MC=full_MC, rejection_func=rejection_func, ddof=ddof,
                                    output_transform=output_transform, **kwargs)
            if full_output:
                return res
            if return_cov:
                return (res["mean"], res["cov"])
            if return_std:
                return (res["mean"], res["std"])
            return res["mean"]
        Xstar, n, output_transform = self._check_predict_args(Xstar, n, output_transform)
        self.compute_K_L_alpha_ll()
        need_cov = (return_cov or full_output or return_samples or full_MC or
                    (output_transform is not None and (return_std or return_cov)))
        need_std = return_std or need_cov
        if self._fit_mode == "kernel":
            want = 2 if need_cov else (1 if need_std else 0)
            mean, std, covariance = self._ctx.predict(Xstar, n, want, *self._prediction_noise(noise))
        else:
            mean, std, covariance = self._predict_general(Xstar, n, noise, need_std, need_cov)
        mean_func = None
        if self.mu is not None:
            mean_func = self.mu(Xstar, n)
            mean = mean + mean_func
        if output_transform is not None:
            mean = output_transform.dot(mean)
            if mean_func is not None:
                mean_func = output_transform.dot(mean_func)
            if covariance is not None:
                covariance = output_transform.dot(covariance.dot(output_transform.T))
                std = np.sqrt(np.diagonal(covariance))
        if not need_std:
            return mean
        samps = None
        if return_samples or full_MC:                                    # ref :990-1005
            samps = self.draw_sample(Xstar, n=n, num_samp=num_samples, mean=mean, cov=covariance, **samp_kwargs)
            if rejection_func:
                good = [samp for samp in samps.T if rejection_func(samp)]
                if len(good) == 0:
                    raise ValueError("Did not get any good samples!")
                samps = np.asarray(good, dtype=float).T
            if full_MC:
                mean = np.mean(samps, axis=1)
                covariance = np.cov(samps, rowvar=1, ddof=ddof)
                std = np.sqrt(np.diagonal(covariance))
        if full_output:
            out = {"mean": mean, "std": std, "cov": covariance}
            if samps is not None:
                out["samp"] = samps
            if return_mean_func and mean_func is not None:
                out["mean_func"] = mean_func
                out["cov_func"] = np.zeros((len(mean_func), len(mean_func)), dtype=float)
                out["std_func"] = np.zeros_like(mean_func)
                out["mean_without_func"] = mean - mean_func
                out["cov_without_func"] = covariance
                out["std_without_func"] = std
            return out
        if return_cov:
            return (mean, covariance)
        return (mean, std)

    # ---- prediction marginalised over hyperparameter samples (ref: gptools/gaussian_process.py:888-912, :1840-1987,
    # :2144-2330) -----------------------------------------------------------------------------------------------------
    #: traces with fewer usable rows than this take the loop route (one update_hyperparameters + predict per row) even where
    #: the batched route (gpt_fit_batch_terms + gpt_predict_batch) could run: see DESIGN.md section 9 for the measurements
    mcmc_batch_min_rows = 2

    @staticmethod
    def _mcmc_trace(sampler, flat_trace, burn, thin):
        """The rows of free hyperparameters to marginalise over, burned and thinned as the reference does (:1935-1940)."""
        if flat_trace is None:
            if sampler is None:
                raise NotImplementedError("no sampling run is started here: pass flat_trace (samples of the free hyperparameters, "
                                          "one per row) or a sampler that has already been run -- "
                                          "sample_hyperparameter_posterior returns one")
            chain = np.asarray(sampler.chain, dtype=float)[:, burn::thin, :]
            return chain.reshape((-1, chain.shape[2]))
        return np.atleast_2d(np.asarray(flat_trace, dtype=float))[burn::thin, :]

    def _mcmc_evaluate(self, X, n, trace, noise, output_transform, want_var, want_cov, want_cov_sum):
        """Predictive moments at every row of ``trace``.  Returns a dict over the rows that were evaluated (``rows``: their
        indices, in order): ``mean`` (K, M) with the mean function added, ``mean_func`` (K, M) or None, ``var`` (K, M),
        ``cov`` (K, M, M), ``cov_sum`` (M, M) = the sum of the rows' covariances -- each None unless asked for -- all
        after ``output_transform``.  A row is dropped only when its evaluation fails (a NaN parameter, a factor that is not
        positive definite, parameters the library rejects); rows the hyperprior excludes are evaluated as the reference's
        ``update_hyperparameters`` + ``predict`` evaluate them.  The GP's own hyperparameters are unchanged afterwards."""
        if self.X is None:
            raise GPArgumentError("No data have been added to the GaussianProcess!")
        Xs, ns, A = self._check_predict_args(X, n, output_transform)
        if A is not None and want_var:
            want_cov = True                             # (the transformed variances are the diagonals of A cov A^T)
        S, M = trace.shape[0], Xs.shape[0]
        res = {"mean": np.full((S, M), np.nan), "mean_func": None if self.mu is None else np.full((S, M), np.nan),
               "var": np.full((S, M), np.nan) if want_var and A is None else None,
               "cov": np.full((S, M, M), np.nan) if want_cov else None,
               "cov_sum": np.zeros((M, M)) if want_cov_sum else None}
        ok = np.zeros(S, dtype=bool)
        noise_n = self._prediction_noise(noise)[1]      # (the batch's noise variances are those of its fits)
        if noise_n is not None:
            noise_n = np.broadcast_to(np.asarray(noise_n, dtype=np.int32), (self.num_dim,))
        saved = np.array(self.free_params[:], dtype=float)
        keep_partitioned = self.partitioned
        self.partitioned = False
        try:
            rows = [i for i in range(S) if not np.isnan(trace[i]).any()]      # (a NaN parameter: the evaluation fails)
            rest = self._mcmc_batched(Xs, ns, trace, rows, noise_n, res, ok)
            for i in rest:                                   # the loop route (_ComputeGPWrapper, ref :2256-2330)
                try:
                    self.update_hyperparameters(list(trace[i]))      # (+inf where the prior excludes p: predict runs there anyway)
                    if want_cov or want_cov_sum:
                        mean, cov = self.predict(Xs, n=ns, noise=noise, return_cov=True)
                        var = np.diagonal(cov)
                    else:
                        mean, std = self.predict(Xs, n=ns, noise=noise, return_std=True)
                        cov, var = None, std ** 2.0
                except Exception:
                    if self.verbose:
                        warnings.warn("evaluation at trace row %d failed and is dropped:\n%s" % (i, traceback.format_exc()))
                    continue
                res["mean"][i] = mean
                if self.mu is not None:
                    res["mean_func"][i] = self.mu(Xs, ns)
                if res["var"] is not None:
                    res["var"][i] = var
                if want_cov:
                    res["cov"][i] = cov
                if want_cov_sum:
                    res["cov_sum"] += cov
                ok[i] = True
        finally:
            self._assign_free(saved)
            self.partitioned = keep_partitioned
        if not ok.any():
            raise ValueError("every row of the hyperparameter trace failed to evaluate")
        out = {"rows": np.flatnonzero(ok)}
        for key in ("mean", "mean_func", "var", "cov"):
            out[key] = None if res[key] is None else res[key][ok]
        out["cov_sum"] = res["cov_sum"]
        if A is not None:
            # linear in the prediction: transforming the marginal moments equals transforming each row's first
            out["mean"] = out["mean"].dot(A.T)
            if out["mean_func"] is not None:
                out["mean_func"] = out["mean_func"].dot(A.T)
            if out["cov"] is not None:
                out["cov"] = np.matmul(np.matmul(A, out["cov"]), A.T)
                if want_var:
                    out["var"] = np.array([np.diagonal(c) for c in out["cov"]])
            if out["cov_sum"] is not None:
                out["cov_sum"] = A.dot(out["cov_sum"]).dot(A.T)
        return out

    def _mcmc_batched(self, Xs, ns, trace, rows, noise_n, res, ok):
        """The batched route: chunks of rows through gpt_fit_batch_terms + gpt_predict_batch.  Fills ``res`` / ``ok`` for the
        rows it evaluates and returns the rows left to the loop route."""
        N = len(self.y)
        if not rows or len(rows) < int(self.mcmc_batch_min_rows):
            return rows
        model = self._device_model()
        if (not self._fast_fit_possible(model) or self.T is not None or max(N, self.X.shape[0]) > self.batch_grid_max_n
                or int(self.batch_grid) < 1 or model[1]):    # (a warped model: the loop route, each row a device fit + predict)
            return rows
        jobs = []
        for i in rows:
            self._assign_free(trace[i])
            job = self._batch_job(i, None if self.mu is None else np.asarray(self.mu(Xs, ns), dtype=float))
            if job is not None:                              # (else as a fit that fails: the row is dropped)
                jobs.append(job)
        want_var, want_cov, want_sum = res["var"] is not None, res["cov"] is not None, res["cov_sum"] is not None
        M = Xs.shape[0]
        NP, MP = -(-(N + 1) // 128) * 128, -(-M // 64) * 64
        per = 8 * (NP * NP + 9216 * (NP // 128) + MP * NP + (MP * MP if want_cov else 0))
        rest = []

        def predict(chunk, _, info):
            keep = info == 0
            if not keep.any():
                return
            mean, var, cov, cov_sum = self._ctx.predict_batch(Xs, ns, keep, noise_n, want_var, want_cov, want_sum)
            for q, j in enumerate(chunk):
                if not keep[q]:
                    continue                                 # not positive definite: the evaluation fails, the row is dropped
                res["mean"][j.row] = mean[q] if j.extra is None else mean[q] + j.extra
                if j.extra is not None:
                    res["mean_func"][j.row] = j.extra
                if want_var:
                    res["var"][j.row] = var[q]
                if want_cov:
                    res["cov"][j.row] = cov[q]
                ok[j.row] = True
            if want_sum:
                res["cov_sum"] += cov_sum

        # (a parameter the library rejects fails the whole chunk: its rows, like the rows left when not even one element fits, one
        # at a time on the loop route)
        left = self._fit_batched(jobs, per, 8 * (NP * NP + MP * NP), predict, lambda chunk: rest.extend(j.row for j in chunk))
        return sorted(rest + [j.row for j in left])

    def compute_from_MCMC(self, X, n=0, return_mean=True, return_std=True, return_cov=False, return_samples=False,
                          return_mean_func=False, num_samples=1, noise=False, samp_kwargs={}, sampler=None, flat_trace=None,
                          burn=0, thin=1, **kwargs):
        """Predictive quantities at each row of a trace of the free hyperparameters (ref: gaussian_process.py:1840-1987):
        a dict of per-row lists -- ``mean`` (M,), ``std`` (M,), ``cov`` (M, M), ``samp`` (M, num_samples) and, with
        ``return_mean_func`` and a mean function, the ``*_func`` / ``*_without_func`` entries -- over the rows whose
        evaluation succeeded, in trace order.  ``flat_trace[burn::thin]`` or, duck-typed, ``sampler.chain[:, burn::thin, :]``
        flattened (:meth:`sample_hyperparameter_posterior` draws one; no run is started here).  ``num_proc`` is accepted and ignored:
        the rows are evaluated in batches on the GPU (gpt_fit_batch_terms + gpt_predict_batch) where the model allows it,
        else one after another.  Samples are drawn on the host per row, in row order (numpy.random.multivariate_normal).
        The GP's hyperparameters are unchanged afterwards."""
        output_transform = kwargs.pop("output_transform", None)
        trace = self._mcmc_trace(sampler, flat_trace, burn, thin)
        want_func = bool(return_mean_func) and self.mu is not None
        need_cov = bool(return_cov or return_samples or want_func)
        ev = self._mcmc_evaluate(X, n, trace, noise, output_transform, bool(return_std), need_cov, False)
        K = len(ev["rows"])
        std = None
        if return_std or want_func:
            var = ev["var"] if ev["var"] is not None else np.array([np.diagonal(c) for c in ev["cov"]])
            std = np.sqrt(var)
        out = {}
        if return_mean:
            out["mean"] = list(ev["mean"])
        if return_std:
            out["std"] = list(std)
        if return_cov:
            out["cov"] = list(ev["cov"])
        if return_samples:
            out["samp"] = [self.draw_sample(X, n=n, num_samp=num_samples, mean=ev["mean"][q], cov=ev["cov"][q], **samp_kwargs)
                           for q in range(K)]
        if want_func:
            mf = ev["mean_func"]
            out["mean_func"] = list(mf)
            out["cov_func"] = [np.zeros((mf.shape[1], mf.shape[1])) for _ in range(K)]
            out["std_func"] = [np.zeros(mf.shape[1]) for _ in range(K)]
            out["mean_without_func"] = list(ev["mean"] - mf)
            out["cov_without_func"] = list(ev["cov"])
            out["std_without_func"] = list(std)
        return out

    def compute_l_from_MCMC(self, X, n=0, sampler=None, flat_trace=None, burn=0, thin=1, **kwargs):
        """The covariance length-scale function ``k.l_func`` of a Gibbs kernel (its derivative for ``n = 1``) at ``X`` for each
        row of a trace of the free hyperparameters (ref: gaussian_process.py:1989-2065, _ComputeLWrapper :2341-2377): an
        ``(S, M)`` array, one row per trace row, where the reference returns a list (or a lazy ``map``).  A row whose
        evaluation fails is NaN.  ``flat_trace[burn::thin]`` or, duck-typed, ``sampler.chain[:, burn::thin, :]`` flattened;
        :meth:`sample_hyperparameter_posterior` draws one (no run is started here).  ``X`` and ``n`` go to ``l_func`` unchanged.
        Host numpy (O(M S)); ``num_proc`` is accepted and ignored."""
        trace = self._mcmc_trace(sampler, flat_trace, burn, thin)
        X = np.asarray(X, dtype=float)
        p = np.array(self.k.params, dtype=float)
        free = ~np.asarray(self.k.fixed_params, dtype=bool)
        nk = len(self.k.free_params)
        rows = []
        for t in trace:
            try:
                q = p.copy()
                q[free] = t[:nk]
                rows.append(np.asarray(self.k.l_func(X, n, *q[1:]), dtype=float))
            except Exception:
                if self.verbose:
                    warnings.warn("Encountered exception during evaluation of MCMC samples. Exception is:\n%s\nParams are:\n%s"
                                  % (traceback.format_exc(), str(list(t))))
                rows.append(None)
        shape = next((np.shape(r) for r in rows if r is not None), np.shape(X))
        return np.array([np.full(shape, np.nan) if r is None else np.broadcast_to(r, shape) for r in rows], dtype=float)

    def compute_w_from_MCMC(self, X, n=0, sampler=None, flat_trace=None, burn=0, thin=1, **kwargs):
        """The warping function ``k.w_func`` of dimension 0 of a :class:`WarpedKernel` (its slope for ``n = 1``) at ``X`` for
        each row of a trace of the free hyperparameters (ref: gaussian_process.py:2067-2142, _ComputeWWrapper :2379-2420): an
        ``(S, M)`` array where the reference returns a list (or a lazy ``map``).  A row whose evaluation fails, or that holds
        a NaN parameter, is NaN.  Trace handling as :meth:`compute_l_from_MCMC`; the kernel's hyperparameters are unchanged
        afterwards.  Host numpy (O(M S)); ``num_proc`` is accepted and ignored."""
        trace = self._mcmc_trace(sampler, flat_trace, burn, thin)
        X = np.asarray(X, dtype=float)
        p = np.array(self.k.params, dtype=float)
        free = ~np.asarray(self.k.fixed_params, dtype=bool)
        nk = len(self.k.free_params)
        rows = []
        try:
            for t in trace:
                try:
                    q = p.copy()
                    q[free] = t[:nk]
                    self.k.params = q
                    rows.append(np.asarray(self.k.w_func(X, 0, n), dtype=float))
                except Exception:
                    if self.verbose:
                        warnings.warn("Encountered exception during evaluation of MCMC samples. Exception is:\n%s\nParams "
                                      "are:\n%s" % (traceback.format_exc(), str(list(t))))
                    rows.append(None)
        finally:
            self.k.params = p
        shape = next((np.shape(r) for r in rows if r is not None), np.shape(X))
        return np.array([np.full(shape, np.nan) if r is None else np.broadcast_to(r, shape) for r in rows], dtype=float)

    def predict_MCMC(self, X, ddof=1, full_MC=False, rejection_func=None, **kwargs):
        """Prediction marginalised over a trace of the hyperparameters (ref: gaussian_process.py:2144-2254): the mean of the
        rows' means, and by the laws of total variance / covariance ``mean(var) + var(means, ddof)`` /
        ``mean(cov) + cov(means, ddof)`` (numpy's estimators: NaN when no more rows than ``ddof`` survive); ``full_MC``: the
        sample mean and covariance of draws from every row (filtered by ``rejection_func``).  The keyword arguments are
        those of :meth:`compute_from_MCMC` (``flat_trace`` or ``sampler``, ``burn``, ``thin``, ``n``, ``noise``,
        ``return_std``, ``return_cov``, ``return_samples``, ``num_samples``, ``return_mean_func``, ``output_transform``).
        Only the summed covariance of the rows is formed (on the GPU where the batched route runs), not one per row."""
        return_std = kwargs.get("return_std", True)
        return_cov = kwargs.get("return_cov", False)
        return_samples = bool(full_MC or kwargs.get("return_samples", False))
        trace = self._mcmc_trace(kwargs.get("sampler"), kwargs.get("flat_trace"), kwargs.get("burn", 0), kwargs.get("thin", 1))
        X_, n, noise = X, kwargs.get("n", 0), kwargs.get("noise", False)
        output_transform = kwargs.get("output_transform")
        want_func = bool(kwargs.get("return_mean_func", False)) and self.mu is not None and not full_MC
        if full_MC or return_samples:
            ev = self._mcmc_evaluate(X_, n, trace, noise, output_transform, False, True, False)
            samps = np.hstack([self.draw_sample(X_, n=n, num_samp=kwargs.get("num_samples", 1), mean=m, cov=c)
                               for m, c in zip(ev["mean"], ev["cov"])])
            if not full_MC:
                ev["cov_sum"] = np.sum(ev["cov"], axis=0)
        else:
            use_sum = bool(return_cov or want_func or (return_std and output_transform is not None))
            ev = self._mcmc_evaluate(X_, n, trace, noise, output_transform, bool(return_std) and not use_sum, False, use_sum)
        out = {}
        K = len(ev["rows"])
        if full_MC:
            if rejection_func:
                good = [samp for samp in samps.T if rejection_func(samp)]
                if len(good) == 0:
                    raise ValueError("Did not get any good samples!")
                samps = np.asarray(good, dtype=float).T
            mean = np.mean(samps, axis=1)
            cov = np.cov(samps, rowvar=1, ddof=ddof)
            std = np.sqrt(np.diagonal(cov))
        else:
            means = ev["mean"]
            mean = np.mean(means, axis=0)
            if return_cov:
                cov = ev["cov_sum"] / K + np.cov(means, rowvar=0, ddof=ddof)
                std = np.sqrt(np.diagonal(cov))
            elif return_std:
                if ev["var"] is not None:
                    mvar = np.mean(np.sqrt(ev["var"]) ** 2, axis=0)
                else:
                    mvar = np.diagonal(ev["cov_sum"]) / K
                std = np.sqrt(mvar + np.var(means, axis=0, ddof=ddof))
            if want_func:
                mean_funcs = ev["mean_func"]
                mean_func = np.mean(mean_funcs, axis=0)
                cov_func = np.cov(mean_funcs, rowvar=0, ddof=ddof)
                without = means - mean_funcs
                cov_without_func = ev["cov_sum"] / K + np.cov(without, rowvar=0, ddof=ddof)
                out["mean_func"] = mean_func
                out["cov_func"] = cov_func
                out["std_func"] = np.sqrt(np.diagonal(cov_func))
                out["mean_without_func"] = np.mean(without, axis=0)
                out["cov_without_func"] = cov_without_func
                out["std_without_func"] = np.sqrt(np.diagonal(cov_without_func))
        out["mean"] = mean
        if return_samples:
            out["samp"] = samps
        if return_std or return_cov:
            out["std"] = std
        if return_cov:
            out["cov"] = cov
        return out

    # ---- posterior samples (ref: gptools/gaussian_process.py:1155-1330) --------------------------------------
    def draw_sample(self, Xstar, n=0, num_samp=1, rand_vars=None, rand_type="standard normal", diag_factor=1e3,
                    method="cholesky", num_eig=None, mean=None, cov=None, modify_sign=None, **kwargs):
        """Samples ``y* = mean + L u`` of the GP at ``Xstar`` -> (M, num_samp), like the reference: without
        ``rand_vars`` and with ``method='cholesky'`` the draw goes through ``numpy.random.multivariate_normal``
        (falling back on ``'eig'`` if that fails); with ``rand_vars`` (standard normal, or uniform mapped through
        the normal quantile function) the square root ``L`` of ``cov + diag_factor * eps * I`` is the lower Cholesky
        factor -- computed on the GPU -- or ``Q sqrt(Lambda)`` from ``scipy.linalg.eigh``.  The predictive mean and
        covariance come from :meth:`predict` (device path) unless given."""
        if (mean is None and cov is None and rand_vars is not None and method == "cholesky"
                and set(kwargs) <= {"noise"} and rand_type in ("standard normal", "uniform")):
            # Device route (gpt_cov_sample): the predictive covariance stays in HBM, its Cholesky factor is formed there and only
            # L u (M x num_samp) comes back -- nothing of size M^2 crosses PCIe.  Same arithmetic as below (ref :1295-1300, :1330).
            self.compute_K_L_alpha_ll()
            if self._fit_mode == "kernel":
                Xs, ns, _ = self._check_predict_args(Xstar, n)
                noise_params, noise_n = self._prediction_noise(kwargs.get("noise", False))
                M = Xs.shape[0]
                ne = M if (num_eig is None or num_eig > M) else max(int(num_eig), 1)
                rv = np.atleast_2d(np.asarray(rand_vars, dtype=float))[:ne, :]
                if rv.shape[0] == M:              # (anything else is the reference's shape error: raised by the host route)
                    mean_d, _, _ = self._ctx.predict(Xs, ns, 2, noise_params, noise_n, device_cov=True)
                    if self.mu is not None:
                        mean_d = mean_d + self.mu(Xs, ns)
                    if rand_type == "uniform":
                        from scipy.stats import norm as _norm
                        rv = _norm.ppf(rv)
                    return np.atleast_2d(mean_d).T + self._ctx.cov_sample(diag_factor * sys.float_info.epsilon, rv)
        if mean is None or cov is None:
            both = self.predict(Xstar, n=n, full_output=True, **kwargs)
            mean, cov = both["mean"], both["cov"]
        mean, cov = np.asarray(mean, dtype=float), np.asarray(cov, dtype=float)
        M = mean.size
        if rand_vars is None and method != "eig":
            # no variates given: numpy's own multivariate normal (global random state), the eigen route as its fallback
            try:
                return np.random.multivariate_normal(mean, cov, num_samp).T
            except np.linalg.LinAlgError as exc:
                if self.verbose:
                    warnings.warn("multivariate_normal failed (%s); using the eigendecomposition instead" % exc, RuntimeWarning)
                method = "eig"
        if rand_type not in _VARIATE_KINDS:
            raise ValueError("rand_type %r is not one of %s" % (rand_type, sorted(_VARIATE_KINDS)))
        modes = M if (num_eig is None or num_eig > M) else max(int(num_eig), 1)
        u = np.random.standard_normal((modes, num_samp)) if rand_vars is None else np.asarray(rand_vars, dtype=float)
        u = _VARIATE_KINDS[rand_type](u)
        root = self._covariance_root(cov + diag_factor * sys.float_info.epsilon * np.eye(M), method, modes, modify_sign)
        return mean[:, None] + root.dot(u[:modes, :])

    def _covariance_root(self, loaded, method, modes, modify_sign):
        """A matrix ``R`` with ``R R^T`` = the (jittered) predictive covariance: its lower Cholesky factor (computed on the
        GPU), or ``Q sqrt(Lambda)`` over the ``modes`` largest eigenpairs, eigenvalues ascending like ``eigh`` returns them
        (ref: gaussian_process.py:1295-1329)."""
        if method == "cholesky":
            # a context of its own: factoring here must not disturb the resident factor of the fit
            if getattr(self, "_scratch_ctx", None) is None:
                self._scratch_ctx = _lib.Context(self.device)
            return np.tril(self._scratch_ctx.potrf_host(loaded))
        if method != "eig":
            raise ValueError("method %r is neither 'cholesky' nor 'eig'" % (method,))
        M = loaded.shape[0]
        lam, Q = scipy.linalg.eigh(loaded, subset_by_index=(M - modes, M - 1))
        if modify_sign is not None:
            # the sign of an eigenvector is arbitrary; these rules pin it by a feature of the vector's first / last entries
            where, feature = (str(modify_sign).split(" ") + [""])[:2]
            if where not in ("left", "right") or feature not in _SIGN_FEATURES:
                raise ValueError("modify_sign %r is not '<left|right> <value|slope|concavity>'" % (modify_sign,))
            ends = Q[:3, :] if where == "left" else Q[-3:, :]
            Q[:, _SIGN_FEATURES[feature](ends, where) < 0.0] *= -1.0
        return Q * np.sqrt(lam)[None, :]

    def _predict_general(self, Xstar, n, noise, need_std, need_cov=True):
        """predict for fits that went through ``gpt_fit_matrix`` (``T`` present or a Python kernel):
        covariance blocks from ``compute_Kij``, triangular solves on the GPU (the covariance comes with the std whether or not
        ``need_cov`` asks for it)."""
        Kstar = self.compute_Kij(self.X, Xstar, self.n, n)
        if noise:
            Kstar = Kstar + self.compute_Kij(self.X, Xstar, self.n, n, noise=True)
        if self.T is not None:
            Kstar = self.T.dot(Kstar)
        mean = Kstar.T.dot(self.alpha).ravel()
        if not need_std:
            return mean, None, None
        v = self._ctx.solve_L(Kstar)
        Kss = self.compute_Kij(Xstar, None, n, None)
        if noise:
            Kss = Kss + self.compute_Kij(Xstar, None, n, None, noise=True)
        covariance = Kss - v.T.dot(v)
        return mean, np.sqrt(np.diagonal(covariance)), covariance


from .kernel.matern import Matern52Kernel as _M52       # noqa: E402
_M52_CALL = _M52.__call__
_ZERO_CALL = ZeroKernel.__call__
