"""MaskedKernel: a kernel that acts on a subset of the dimensions (ref: gptools/kernel/core.py:1011-1149).

``MaskedKernel(base, total_dim, mask, scale)`` has ``num_dim = total_dim``; it hands the columns ``mask`` of the points (times
``scale``) and of the derivative orders to ``base`` and is exactly 0 for a pair with a derivative order in any other dimension.
That is how different covariance families are given to different dimensions, e.g.
``MaskedKernel(GibbsKernel1dTanh(...), 2, [0]) * MaskedKernel(SquaredExponentialKernel(...), 2, [1])``.

The hyperparameters ARE the base kernel's: every view of them (``params``, ``free_params``, bounds, names, ``fixed_params``,
``hyperprior``, ``enforce_bounds``, ``set_hyperparams``) reads and writes ``base``.  The reference gets there by overriding
``__getattribute__`` / ``__setattr__``; here each view is forwarded by name.

Two routes of evaluation:

* **device** (:meth:`MaskedKernel._native_factor` is not ``None``): the base is a kernel the HIP library evaluates itself, ``scale``
  was left at its default and ``__call__`` is this class's own.

  - SE, Matern52, RationalQuadratic, Matern: the masked kernel is the same kernel at ``total_dim`` whose masked-out dimensions have
    an infinite length scale -- ``1/l = 1/l^2 = 0``, so the distance ignores them and a derivative order there multiplies the
    pair by zero (include/gpt_hip.h).
  - Periodic: likewise, with the period 1 beside the infinite length scale in the masked-out dimensions.
  - Spectral: likewise, with the frequency 0 beside the infinite length scale in the masked-out dimensions.
  - a 1-D Gibbs kernel at ``total_dim <= 3``: the kernel id carries the dimension it acts on (``GPT_KERNEL_ON_DIM``); such a
    kernel is a product factor on the device, and on its own it is its product with the constant unit factor
    ``SE [1, inf .. inf]`` (:func:`unit_factor`).

  The library's derivative-order rules for the stationary kernels look at WHOLE rows of orders (Matern52: a point's orders sum to
  <= 1; the caps of RationalQuadratic / Matern / products on the sum over a pair), masked-out dimensions included.  That is
  conservative: the reference would answer 0 for some pairs this route refuses.  The Gibbs rule (orders <= 1) looks at the
  kernel's own dimension only: the orders of the other dimensions belong to the other factor.

* **host** (everything else: a non-default ``scale``, a base that is a sum, a product, a warped, a masked or a Python-defined
  kernel, Gibbs at ``total_dim > 3``): the reference's own steps -- the pairs without an outside order go to ``base`` on the sliced
  columns, the rest stay 0.
"""
import numpy as np

from .core import Kernel
from .matern import Matern52Kernel
from .. import _lib

__all__ = ["MaskedKernel"]

_STATIONARY = (_lib.KERNEL_SE, _lib.KERNEL_M52, _lib.KERNEL_RQ, _lib.KERNEL_MATERN)
_GIBBS = (_lib.KERNEL_GIBBS_TANH, _lib.KERNEL_GIBBS_DTANH, _lib.KERNEL_GIBBS_CUBIC, _lib.KERNEL_GIBBS_QUINTIC,
          _lib.KERNEL_GIBBS_EXPGAUSS, _lib.KERNEL_GIBBS_BSPLINE, _lib.KERNEL_GIBBS_GP)


def unit_factor(num_dim):
    """``(kernel_id, params)`` of the constant 1 as a native product factor: SE with ``sigma_f = 1`` and every length scale
    infinite (value exactly 1.0, every derivative exactly 0)."""
    return _lib.KERNEL_SE, np.concatenate(([1.0], np.full(num_dim, np.inf)))


def _to_base(name):
    return property(lambda self: getattr(self.base, name), lambda self, value: setattr(self.base, name, value),
                    doc="``base.%s``" % name)


class MaskedKernel(Kernel):
    """``base`` applied to the dimensions ``mask`` of ``total_dim``-dimensional points (ref: gptools/kernel/core.py:1011-1149).

    ``mask``: ``base.num_dim`` distinct indices below ``total_dim`` (default ``[0]``); ``scale``: ``2 * base.num_dim`` factors, the
    first half for the columns of ``Xi``, the second for those of ``Xj`` (default: ones).  A first-order derivative with respect
    to a scaled column picks up that column's factor, per order, as in the reference (core.py:1143-1147)."""

    def __init__(self, base, total_dim=2, mask=[0], scale=None):
        if not isinstance(base, Kernel):
            raise TypeError("base must be an instance of type Kernel!")
        if len(mask) != base.num_dim:
            raise ValueError("Length of mask must be equal to the number of dimensions of the base kernel!")
        self._default_scale = scale is None
        if scale is None:
            scale = [1] * 2 * base.num_dim
        elif len(scale) != 2 * base.num_dim:
            raise ValueError("Length of scale must be equal to twice the number of dimensions of the base kernel!")
        if isinstance(total_dim, bool) or not isinstance(total_dim, (int, np.integer)) or total_dim < 1:
            raise ValueError("num_dim must be an integer > 0!")
        self.base = base
        self.num_dim = int(total_dim)
        self.mask = [int(v) for v in mask]
        # the complement of the mask (the reference removes the entries one by one from range(total_dim): an index that is not
        # there, or not there any more, is its ValueError)
        self.maskC = list(range(self.num_dim))
        for v in self.mask:
            if v not in self.maskC:
                raise ValueError("mask must hold distinct dimensions below total_dim = %d, got %r" % (self.num_dim, list(mask)))
            self.maskC.remove(v)
        self.scale = np.array(scale, dtype=float)

    # ---- the hyperparameters are the base kernel's ----------------------------------------------------------------------
    num_params = _to_base("num_params")
    params = property(lambda self: self.base.params,
                      lambda self, value: setattr(self.base, "params", np.asarray(value, dtype=float)), doc="``base.params``")
    fixed_params = property(lambda self: self.base.fixed_params,
                            lambda self, value: setattr(self.base, "fixed_params", np.asarray(value, dtype=bool)),
                            doc="``base.fixed_params``")
    param_names = _to_base("param_names")
    param_bounds = _to_base("param_bounds")
    hyperprior = _to_base("hyperprior")
    enforce_bounds = _to_base("enforce_bounds")
    free_params = _to_base("free_params")
    free_param_bounds = _to_base("free_param_bounds")
    free_param_names = _to_base("free_param_names")
    free_param_idxs = property(lambda self: self.base.free_param_idxs)
    num_free_params = property(lambda self: self.base.num_free_params)

    def set_hyperparams(self, new_params):
        self.base.set_hyperparams(new_params)

    # ---- routing ---------------------------------------------------------------------------------------------------------
    def _native_factor(self):
        """``(kernel_id, params)`` as the HIP library takes this kernel -- a stationary kernel with infinite length scales in the
        masked-out dimensions, or a Gibbs id that carries its dimension -- else ``None`` (the host route).  The class is
        recognised by type: a subclass that overrides ``__call__`` is a Python-defined kernel."""
        base = self.base
        if (type(self).__call__ is not MaskedKernel.__call__ or not self._default_scale
                or type(base).__call__ not in (Kernel.__call__, Matern52Kernel.__call__)):
            return None
        kid = type(base)._gpt_kernel_id
        if kid in _STATIONARY:
            lead = base.num_params - base.num_dim
            p = np.array(base.params, dtype=float)
            ls = np.full(self.num_dim, np.inf)
            ls[self.mask] = p[lead:]
            return kid, np.concatenate((p[:lead], ls))
        if kid == _lib.KERNEL_PERIODIC:
            # [sigma_f, l .., p ..]: outside the mask l = inf (1 / l^2 = 0: the factor is exactly 1, its derivatives exactly 0) and
            # p = 1, any legal period
            d = base.num_dim
            p = np.array(base.params, dtype=float)
            ls, ps = np.full(self.num_dim, np.inf), np.ones(self.num_dim)
            ls[self.mask] = p[1:1 + d]
            ps[self.mask] = p[1 + d:]
            return kid, np.concatenate((p[:1], ls, ps))
        if kid == _lib.KERNEL_SPECTRAL:
            # [sigma_f, mu .., l ..]: outside the mask mu = 0 and l = inf (no phase, no envelope: the dimension contributes exactly 1,
            # its derivatives exactly 0)
            d = base.num_dim
            p = np.array(base.params, dtype=float)
            mus, ls = np.zeros(self.num_dim), np.full(self.num_dim, np.inf)
            mus[self.mask] = p[1:1 + d]
            ls[self.mask] = p[1 + d:]
            return kid, np.concatenate((p[:1], mus, ls))
        if kid in _GIBBS and self.num_dim <= _lib.GIBBS_ON_DIM_MAX_D:
            return _lib.kernel_on_dim(kid, self.mask[0]), base._native_params()
        return None

    def _native_term(self):
        """The kernel as ONE term of a device model (``GaussianProcess._native_terms``): ``(kernel_id, params)``, or for a Gibbs
        base the product ``(kernel_id, params, SE, [1, inf ..])``; ``None`` on the host route."""
        f = self._native_factor()
        if f is None or f[0] < _lib.KERNEL_ON_DIM_STRIDE:
            return f
        return f + unit_factor(self.num_dim)

    def _device_hyper_deriv(self, hyper_deriv):
        """Index of base parameter ``hyper_deriv`` in the expanded parameter array of a stationary base."""
        lead = self.base.num_params - self.base.num_dim
        return hyper_deriv if hyper_deriv < lead else lead + self.mask[hyper_deriv - lead]

    # ---- evaluation --------------------------------------------------------------------------------------------------------
    def __call__(self, Xi, Xj, ni, nj, hyper_deriv=None, symmetric=False):
        Xi, Xj = np.atleast_2d(np.asarray(Xi, dtype=float)), np.atleast_2d(np.asarray(Xj, dtype=float))
        ni, nj = np.atleast_2d(np.asarray(ni, dtype=int)), np.atleast_2d(np.asarray(nj, dtype=int))
        term = self._native_term()
        if term is not None and (hyper_deriv is None or len(term) == 2):
            if hyper_deriv is not None:
                if not 0 <= int(hyper_deriv) < self.base.num_params:
                    raise ValueError("hyper_deriv %d out of range" % hyper_deriv)
                if term[0] != _lib.KERNEL_SE:
                    raise NotImplementedError("Hyperparameter derivatives have not been implemented!")
                hyper_deriv = self._device_hyper_deriv(int(hyper_deriv))
            ctx = _lib.default_context()
            if len(term) == 4:
                return ctx.kpairs2(term[0], term[1], term[2], term[3], Xi, Xj, ni, nj)
            return ctx.kpairs(term[0], term[1], Xi, Xj, ni, nj, hyper_deriv=hyper_deriv, symmetric=symmetric)
        return self._host_call(Xi, Xj, ni, nj, hyper_deriv=hyper_deriv, symmetric=symmetric)

    def _host_call(self, Xi, Xj, ni, nj, hyper_deriv=None, symmetric=False):
        """The reference's steps (core.py:1128-1149): ``base`` on the sliced, scaled columns of the pairs without an order outside
        the mask, times ``scale ** order`` over the masked columns; every other pair stays 0."""
        Xi, Xj = np.atleast_2d(np.asarray(Xi, dtype=float)), np.atleast_2d(np.asarray(Xj, dtype=float))
        ni, nj = np.atleast_2d(np.asarray(ni, dtype=int)), np.atleast_2d(np.asarray(nj, dtype=int))
        good = (ni[:, self.maskC] == 0).all(axis=1) & (nj[:, self.maskC] == 0).all(axis=1)
        result = np.zeros(Xi.shape[0])
        if good.any():
            d = self.base.num_dim
            scale = np.asarray(self.scale, dtype=float)
            nig, njg = ni[good][:, self.mask], nj[good][:, self.mask]
            result[good] = self.base(Xi[good][:, self.mask] * scale[:d], Xj[good][:, self.mask] * scale[d:], nig, njg,
                                     hyper_deriv=hyper_deriv, symmetric=symmetric) * \
                (scale[None, :] ** np.hstack((nig, njg))).prod(axis=1)
        return result
