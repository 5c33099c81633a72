r"""Input-warped kernels: ``k(w(x), w(x'))`` with an elementwise, per-dimension warp ``w``.

ref: gptools/kernel/warping.py:63-313 (WarpingFunction), :315-402 (beta_cdf_warp, linear_warp), :404-462 (ISplineWarp),
:464-631 (WarpedKernel), :633-758 (BetaWarpedKernel, LinearWarpedKernel, ISplineWarpedKernel); Snoek et al., "Input Warping for Bayesian Optimization of Non-stationary
Functions", ICML 2014.  With ``w_d`` acting on dimension ``d`` alone,

.. math::  \tilde k(x, x') = k(w(x), w(x')), \qquad
           \partial_{x_d} \tilde k = w_d'(x_d)\, (\partial_d k)(w(x), w(x')),

so a pair with first-derivative orders is the inner kernel at the warped points with the same orders, times ``w_d'`` of
every dimension in which the row point carries order 1, and likewise for the column point.  Orders above 1 would need
``w''`` (Faa di Bruno) and raise ``ValueError`` like the reference.

* beta warp: ``w = I_x(alpha, beta)`` (regularised incomplete beta function), ``w' = x^(alpha-1) (1-x)^(beta-1) / B(alpha, beta)``;
  inputs must lie in [0, 1] (NaN outside, exactly 0 / 1 at the ends).
* linear warp: ``w = (x - a)/(b - a)``, ``w' = 1/(b - a)``: maps data onto the unit cube in front of a beta warp.
* I-spline warp: ``w = sum_i C_i I_{i,k}(x | t)`` on a knot grid per dimension (``splines.spev``), monotone for positive
  coefficients, ``w(t_1) = 0``; ``w'`` is the M-spline of degree ``k - 1``.

``WarpedKernel.__call__`` runs on the host (numpy / scipy) around the inner kernel's pair-list route and works for any
inner kernel, any placement (a warped term of a sum) and any user warp function.  ``GaussianProcess`` peels beta / linear
layers off the *outside* of a native model and evaluates that on the GPU instead (``gpt_set_warp``).
The I-spline warp is not among those layers: a kernel warped by it is a Python kernel (pair list on the host, the matrix fit on
the GPU).
"""
import inspect

import numpy as np
import scipy.special

from .core import Kernel
from .._hyper import HyperparameterSet
from ..splines import spev
from ..utils import CombinedBounds, LogNormalJointPrior

__all__ = ["WarpingFunction", "beta_cdf_warp", "linear_warp", "ISplineWarp", "WarpedKernel", "BetaWarpedKernel",
           "LinearWarpedKernel", "ISplineWarpedKernel"]


class WarpingFunction(HyperparameterSet):
    """A function ``fun(X, d, n, p1, p2, ...)`` -- ``X`` the (M,) coordinates of dimension ``d``, ``n`` the derivative
    order, ``p1 ...`` hyperparameters -- with the hyperparameter bookkeeping ``WarpedKernel`` needs (ref: warping.py:63-313).

    ``num_params`` is counted from ``fun``'s signature when not given; for a ``*args`` signature it is the length of
    ``hyperprior.bounds``, ``param_names`` or ``param_bounds``, whichever is given first in that order.  The other keywords are
    those of :class:`Kernel`; the default prior is uniform over (0, 1e16)."""

    def __init__(self, fun, num_dim=1, num_params=None, initial_params=None, fixed_params=None, param_bounds=None,
                 param_names=None, enforce_bounds=False, hyperprior=None):
        self.fun = fun
        if num_params is None:
            sig = inspect.signature(fun)              # (a bound method's or callable object's signature omits self already)
            kinds = [p.kind for p in sig.parameters.values()]
            if inspect.Parameter.VAR_POSITIONAL in kinds:
                if hyperprior is not None:
                    num_params = len(hyperprior.bounds) if hasattr(hyperprior, "bounds") else len(hyperprior)
                elif param_names is not None:
                    num_params = len(param_names)
                elif param_bounds is not None:
                    num_params = len(param_bounds)
                else:
                    raise ValueError("If warping function w uses a variable number of arguments, you must also specify an "
                                     "explicit hyperprior, list of param_names and/or list of param_bounds.")
            else:
                num_params = sum(k in (inspect.Parameter.POSITIONAL_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD)
                                 for k in kinds) - 3
        if isinstance(num_dim, bool) or not isinstance(num_dim, (int, np.integer)) or num_dim < 1:
            raise ValueError("num_dim must be an integer > 0!")
        self.num_dim = int(num_dim)
        self._init_hyperparameters(num_params, values=initial_params, fixed=fixed_params, bounds=param_bounds,
                                   names=param_names, prior=hyperprior, clamp=enforce_bounds)

    def __call__(self, X, d, n):
        """``w`` (``n = 0``) or its ``n``-th derivative on the coordinates ``X`` of dimension ``d``."""
        return self.fun(X, d, n, *self.params)


def beta_cdf_warp(X, d, n, *args):
    r"""Beta-CDF warp of dimension ``d``: ``I_x(alpha_d, beta_d)`` with ``alpha_d, beta_d = args[2d], args[2d+1]``
    (``n = 0``), its slope (``n = 1``) or a higher derivative (ref: warping.py:315-365).  Inputs in [0, 1]."""
    X = np.asarray(X, dtype=float)
    a, b = args[2 * d], args[2 * d + 1]
    with np.errstate(all="ignore"):
        if n == 0:
            return scipy.special.betainc(a, b, X)
        if n == 1:
            return (1 - X) ** (b - 1) * X ** (a - 1) / scipy.special.beta(a, b)
        # d^n/dx^n I_x(a, b), functions.wolfram.com/GammaBetaErf/BetaRegularized/20/02/01/; (.)_k is the Pochhammer symbol
        def poch(z, k):
            return float(np.prod([z + i for i in range(int(k))]))
        out = np.zeros_like(X)
        for k in range(0, n):
            out += ((-1.0) ** (n - k) * scipy.special.binom(n - 1, k) * poch(1.0 - b, k) * poch(1.0 - a, n - k - 1) *
                    (X / (1.0 - X)) ** k)
        return -(1.0 - X) ** (b - 1.0) * X ** (a - n) * out / scipy.special.beta(a, b)


def linear_warp(X, d, n, *args):
    r"""Linear warp of dimension ``d``: ``(x - a_d)/(b_d - a_d)`` with ``a_d, b_d = args[2d], args[2d+1]`` (``n = 0``),
    ``1/(b_d - a_d)`` (``n = 1``), zero above (ref: warping.py:367-402)."""
    X = np.asarray(X, dtype=float)
    a, b = args[2 * d], args[2 * d + 1]
    if n == 0:
        return (X - a) / (b - a)
    if n == 1:
        return 1.0 / (b - a) * np.ones_like(X)
    return np.zeros_like(X)


class ISplineWarp(object):
    r"""I-spline warp ``w(x) = \sum_{i=1}^{nt+k-2} C_i I_{i,k}(x | t)`` per dimension (ref: warping.py:404-462).

    ``nt``: the number of knots, one int for every dimension or one per dimension; ``k``: the degree, the same in every
    dimension.  Called as ``warp(X, d, n, *args)`` with ALL dimensions' parameters in ``args``: per dimension the ``nt_d`` knots,
    then the ``nt_d + k - 2`` coefficients.  The constant I-spline gets the coefficient 0, so ``w(t_1) = 0``."""

    def __init__(self, nt, k=3):
        self.nt = nt
        self.k = k

    def __call__(self, X, d, n, *args):
        X = np.asarray(X, dtype=float)
        args = np.asarray(args, dtype=float)
        nt = np.asarray(self.nt, dtype=int)
        if nt.ndim == 0:
            nt = np.full(d + 1, int(nt), dtype=int)
        i = int(sum(2 * nt[j] + self.k - 2 for j in range(d)))
        ntd = int(nt[d])
        t = args[i:i + ntd]
        C = np.concatenate(([0.0], args[i + ntd:i + 2 * ntd + self.k - 2]))
        return spev(t, C, self.k, X, n=n, I_spline=True)


class WarpedKernel(Kernel):
    """``k`` with its inputs passed through the warp ``w`` (a :class:`WarpingFunction`, or a bare function that is
    wrapped in one).  Parameters: those of ``k``, then those of ``w``; nesting ``WarpedKernel(WarpedKernel(k, w_in), w_out)``
    applies ``w_out`` first and orders the parameters ``[k, w_in, w_out]`` (ref: warping.py:464-631)."""

    def __init__(self, k, w):
        if not isinstance(k, Kernel):
            raise TypeError("Argument k of WarpedKernel must be an instance of Kernel!")
        if not isinstance(w, WarpingFunction):
            w = WarpingFunction(w)
        if k.num_dim != w.num_dim:
            raise ValueError("k and w must have the same number of dimensions!")
        self.k = k
        self.w = w
        self.num_dim = k.num_dim
        self.num_params = k.num_params + w.num_params
        self._enforce_bounds = k.enforce_bounds or w.enforce_bounds
        self.hyperprior = k.hyperprior * w.hyperprior

    def __call__(self, Xi, Xj, ni, nj, hyper_deriv=None, symmetric=False):
        Xi, Xj = np.atleast_2d(np.asarray(Xi, dtype=float)), np.atleast_2d(np.asarray(Xj, dtype=float))
        ni, nj = np.atleast_2d(np.asarray(ni, dtype=int)), np.atleast_2d(np.asarray(nj, dtype=int))
        if (ni > 1).any() or (nj > 1).any():
            raise ValueError("Derivative orders greater than one are not supported!")
        wXi, wXj = np.empty_like(Xi), np.empty_like(Xj)
        for d in range(self.num_dim):
            wXi[:, d] = self.w(Xi[:, d], d, 0)
            wXj[:, d] = self.w(Xj[:, d], d, 0)
        out = np.array(self.k(wXi, wXj, ni, nj, hyper_deriv=hyper_deriv, symmetric=symmetric), dtype=float)
        for d in range(self.num_dim):
            mi, mj = ni[:, d] == 1, nj[:, d] == 1
            if mi.any():
                out[mi] *= self.w(Xi[mi, d], d, 1)
            if mj.any():
                out[mj] *= self.w(Xj[mj, d], d, 1)
        return out

    def w_func(self, X, d, n):
        """The whole (possibly nested) warp of dimension ``d`` at ``X`` (``n = 0``), or its slope (``n = 1``: the product of
        the layers' slopes, each at its own layer's input)."""
        X = np.asarray(X, dtype=float)
        if n == 0:
            wX = self.w(X, d, 0)
            return self.k.w_func(wX, d, 0) if isinstance(self.k, WarpedKernel) else wX
        if n == 1:
            s = self.w(X, d, 1)
            return s * self.k.w_func(self.w(X, d, 0), d, 1) if isinstance(self.k, WarpedKernel) else s
        raise ValueError("Derivative orders greater than one are not supported!")

    # ---- hyperparameter views: k's, then w's (CombinedBounds writes through) ----
    @property
    def enforce_bounds(self):
        return self._enforce_bounds

    @enforce_bounds.setter
    def enforce_bounds(self, v):
        self._enforce_bounds = v
        self.k.enforce_bounds = v
        self.w.enforce_bounds = v

    def _split(self, attr, value, count_attr):
        nk = getattr(self.k, count_attr)
        setattr(self.k, attr, value[:nk])
        setattr(self.w, attr, value[nk:nk + getattr(self.w, count_attr)])

    @property
    def fixed_params(self):
        return CombinedBounds(self.k.fixed_params, self.w.fixed_params)

    @fixed_params.setter
    def fixed_params(self, value):
        self._split("fixed_params", np.asarray(value, dtype=bool), "num_params")

    @property
    def params(self):
        return CombinedBounds(self.k.params, self.w.params)

    @params.setter
    def params(self, value):
        self._split("params", np.asarray(value, dtype=float), "num_params")

    @property
    def param_names(self):
        return CombinedBounds(self.k.param_names, self.w.param_names)

    @param_names.setter
    def param_names(self, value):
        self._split("param_names", np.asarray(value, dtype=str), "num_params")

    @property
    def free_params(self):
        return CombinedBounds(self.k.free_params, self.w.free_params)

    @free_params.setter
    def free_params(self, value):
        self._split("free_params", np.asarray(value, dtype=float), "num_free_params")

    @property
    def free_param_bounds(self):
        return CombinedBounds(self.k.free_param_bounds, self.w.free_param_bounds)

    @free_param_bounds.setter
    def free_param_bounds(self, value):
        self._split("free_param_bounds", np.asarray(value, dtype=float), "num_free_params")

    @property
    def free_param_names(self):
        return CombinedBounds(self.k.free_param_names, self.w.free_param_names)

    @free_param_names.setter
    def free_param_names(self, value):
        self._split("free_param_names", np.asarray(value, dtype=str), "num_free_params")

    @property
    def num_free_params(self):
        return self.k.num_free_params + self.w.num_free_params

    @property
    def free_param_idxs(self):
        return np.flatnonzero(~np.asarray(self.fixed_params[:], dtype=bool))

    def set_hyperparams(self, new_params):
        new_params = np.asarray(new_params, dtype=float)
        if len(new_params) != len(self.free_params):
            raise ValueError("Length of new_params must be {:d}!".format(len(self.free_params)))
        nk = self.k.num_free_params
        self.k.set_hyperparams(new_params[:nk])
        self.w.set_hyperparams(new_params[nk:])


class BetaWarpedKernel(WarpedKernel):
    r"""``k`` warped by the beta CDF in every dimension; inputs must lie in the unit cube.  Parameters of the warp:
    ``\alpha_0, \beta_0, \alpha_1, ...``; without ``hyperprior`` / ``param_bounds`` each follows a log-normal prior
    (``mu = 0``, ``sigma = 0.5``).  Other keywords go to :class:`WarpingFunction` (ref: warping.py:633-673)."""

    def __init__(self, k, **w_kwargs):
        names = []
        for d in range(k.num_dim):
            names += ["\\alpha_{:d}".format(d), "\\beta_{:d}".format(d)]
        if "hyperprior" not in w_kwargs and "param_bounds" not in w_kwargs:
            w_kwargs["hyperprior"] = LogNormalJointPrior([0, 0] * k.num_dim, [0.5, 0.5] * k.num_dim)
        super(BetaWarpedKernel, self).__init__(
            k, WarpingFunction(beta_cdf_warp, num_dim=k.num_dim, param_names=names, **w_kwargs))


class LinearWarpedKernel(WarpedKernel):
    """``k`` behind ``(x - a_d)/(b_d - a_d)`` per dimension (``a``, ``b`` of length ``k.num_dim``); the parameters
    ``a_0, b_0, a_1, ...`` are fixed, with bounds +-1e-3 around their values (ref: warping.py:675-716)."""

    def __init__(self, k, a, b):
        a = np.atleast_1d(np.asarray(a, dtype=float))
        b = np.atleast_1d(np.asarray(b, dtype=float))
        if len(a) != k.num_dim:
            raise ValueError("a must have length equal to k.num_dim!")
        if len(b) != k.num_dim:
            raise ValueError("b must have length equal to k.num_dim!")
        names, values, bounds = [], [], []
        for d in range(k.num_dim):
            names += ["a_{:d}".format(d), "b_{:d}".format(d)]
            values += [a[d], b[d]]
            bounds += [(a[d] - 1e-3, a[d] + 1e-3), (b[d] - 1e-3, b[d] + 1e-3)]
        super(LinearWarpedKernel, self).__init__(
            k, WarpingFunction(linear_warp, num_dim=k.num_dim, initial_params=values, param_bounds=bounds,
                               fixed_params=np.ones(len(values), dtype=bool), param_names=names))


class ISplineWarpedKernel(WarpedKernel):
    """``k`` warped by an I-spline of degree ``k_deg`` per dimension (:class:`ISplineWarp`); ``nt`` is the number of knots, an int
    or one per dimension.  Parameters of the warp: per dimension ``t_{d,1} ..`` then ``C_{d,1} .. C_{d,nt+k_deg-2}``.  Other
    keywords go to :class:`WarpingFunction` (ref: warping.py:718-758).  Evaluated on the host around the inner kernel."""

    def __init__(self, k, nt, k_deg=3, **w_kwargs):
        try:
            iter(nt)
        except TypeError:
            nt = nt * np.ones(k.num_dim, dtype=int)
        else:
            nt = np.asarray(nt, dtype=int)
            if len(nt) != k.num_dim:
                raise ValueError("nt must have length equal to k.num_dim!")
        names = []
        for d, ntv in enumerate(nt):
            names += ["t_{{{:d},{:d}}}".format(d, i + 1) for i in range(ntv)]
            names += ["C_{{{:d},{:d}}}".format(d, i + 1) for i in range(ntv + k_deg - 2)]
        super(ISplineWarpedKernel, self).__init__(
            k, WarpingFunction(ISplineWarp(nt, k=k_deg), num_dim=k.num_dim, param_names=names, num_params=len(names),
                               **w_kwargs))
