r"""Gibbs non-stationary squared-exponential kernels in one dimension.

ref: gptools/kernel/gibbs.py:229-424 (GibbsKernel1d), :426-466 (tanh_warp, GibbsKernel1dTanh), :508-558 (double_tanh_warp,
GibbsKernel1dDoubleTanh).  With a point-dependent length scale ``l(x)``, ``a = l(x_i)``, ``b = l(x_j)``, ``s = a^2 + b^2``
and ``d = x_i - x_j``:

.. math::  k = \sigma_f^2 \sqrt{2ab/s}\, \exp(-d^2/s).

The reference hard-codes the derivative classes as expanded polynomials (terms up to ``l^8``); here they are written as
``k`` times a short factor (``a' = dl/dx`` at ``x_i``, ``b'`` at ``x_j``)::

    P = a'/(2a) - a a'/s - 2d/s + 2d^2 a a'/s^2            d k / d x_i        = k P
    Q = b'/(2b) - b b'/s + 2d/s + 2d^2 b b'/s^2            d k / d x_j        = k Q
    R = 2 a a' b b'/s^2 + 2/s + 4d b b'/s^2 - 4d a a'/s^2 - 8d^2 a a' b b'/s^3
                                                           d2 k / dx_i dx_j   = k (P Q + R)

``GibbsKernel1d(l_func)`` evaluates that on the host in numpy for any warp (the Python-kernel route of
``GaussianProcess``: pair list, then ``fit_matrix`` on the GPU).  ``GibbsKernel1dTanh`` and ``GibbsKernel1dDoubleTanh`` are
native: the HIP library evaluates them (``GPT_KERNEL_GIBBS_TANH`` / ``GPT_KERNEL_GIBBS_DTANH``, gptools_amd/csrc/kpair.hpp)
with the warps hoisted out of the builder's pair loop.  A subclass that overrides ``__call__`` is a Python kernel again.
Derivative orders above ``[1, 1]`` and hyperparameter derivatives raise ``NotImplementedError`` like the reference.
"""
import inspect

import numpy as np

from .core import Kernel
from .. import _lib

__all__ = ["GibbsKernel1d", "GibbsKernel1dTanh", "GibbsKernel1dDoubleTanh", "tanh_warp", "double_tanh_warp"]


def gibbs_1d(x, y, ni, nj, lx, ly, lx1, ly1):
    """``k / sigma_f^2`` of the pairs ``(x[m], y[m])`` with orders ``ni[m], nj[m]`` in {0, 1}, from the warp values ``l``
    and slopes ``l'`` at both points."""
    with np.errstate(all="ignore"):
        d = x - y
        s = lx * lx + ly * ly
        u = 1.0 / s
        k = np.sqrt(2.0 * lx * ly / s) * np.exp(-d * d / s)
        A = lx * lx1
        B = ly * ly1
        P = lx1 / (2.0 * lx) - A * u - 2.0 * d * u + 2.0 * d * d * A * u * u
        Q = ly1 / (2.0 * ly) - B * u + 2.0 * d * u + 2.0 * d * d * B * u * u
        R = 2.0 * A * B * u * u + 2.0 * u + 4.0 * d * B * u * u - 4.0 * d * A * u * u - 8.0 * d * d * A * B * u * u * u
        out = np.where(ni == 1, np.where(nj == 1, k * (P * Q + R), k * P), np.where(nj == 1, k * Q, k))
    return out


class GibbsKernel1d(Kernel):
    r"""Gibbs warped squared-exponential kernel in 1d with an arbitrary length-scale function (ref: gibbs.py:229-424).

    ``l_func(x, n, p1, p2, ...)`` returns ``l`` for ``n == 0`` and ``dl/dx`` for ``n == 1``; ``p1 ...`` are the kernel's
    parameters after ``sigma_f``.  ``num_params`` (``sigma_f`` included) is counted from ``l_func``'s signature when not
    given.  Evaluated on the host (numpy).
    """

    def __init__(self, l_func, num_params=None, **kwargs):
        self.l_func = l_func
        if kwargs.get("num_dim", 1) != 1:
            raise ValueError("Gibbs kernel only supports 1d data.")
        kwargs.pop("num_dim", None)
        if num_params is None:
            # (x, n, p1 .. pk) -> k parameters of the warp, plus sigma_f; a bound method's signature omits self already
            sig = inspect.signature(l_func)
            pos = [p for p in sig.parameters.values()
                   if p.kind in (inspect.Parameter.POSITIONAL_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD)]
            num_params = len(pos) - 2 + 1
        super(GibbsKernel1d, self).__init__(num_dim=1, num_params=num_params, **kwargs)

    def __call__(self, Xi, Xj, ni, nj, hyper_deriv=None, symmetric=False):
        if hyper_deriv is not None:
            raise NotImplementedError("Hyperparameter derivatives have not been implemented!")
        ni = np.atleast_2d(np.asarray(ni, dtype=int))
        nj = np.atleast_2d(np.asarray(nj, dtype=int))
        if (ni > 1).any() or (nj > 1).any() or (ni < 0).any() or (nj < 0).any():
            raise NotImplementedError("Derivatives greater than [1, 1] are not supported!")
        x = np.atleast_2d(np.asarray(Xi, dtype=float))[:, 0]
        y = np.atleast_2d(np.asarray(Xj, dtype=float))[:, 0]
        p = self.params[1:]
        with np.errstate(all="ignore"):
            lx, ly = self.l_func(x, 0, *p), self.l_func(y, 0, *p)
            lx1, ly1 = self.l_func(x, 1, *p), self.l_func(y, 1, *p)
        return self.params[0] ** 2 * gibbs_1d(x, y, ni[:, 0], nj[:, 0], lx, ly, lx1, ly1)


def tanh_warp(x, n, l1, l2, lw, x0):
    r"""``l = (l_1 + l_2)/2 - (l_1 - l_2)/2 tanh((x - x_0)/l_w)`` (``n = 0``) or its slope (``n = 1``) (ref: gibbs.py:426-466)."""
    if n == 0:
        return (l1 + l2) / 2.0 - (l1 - l2) / 2.0 * np.tanh((x - x0) / lw)
    elif n == 1:
        return -(l1 - l2) / (2.0 * lw) * (np.cosh((x - x0) / lw)) ** (-2.0)
    else:
        raise NotImplementedError("Only derivatives up to order 1 are supported!")


def double_tanh_warp(x, n, lcore, lmid, ledge, la, lb, xa, xb):
    r"""``l = a tanh((x - x_a)/l_a) + b tanh((x - x_b)/l_b) + c`` with ``a = (l_mid - l_core)/2``, ``b = (l_edge - l_mid)/2``,
    ``c = (l_core + l_edge)/2`` (``n = 0``) or its slope (``n = 1``) (ref: gibbs.py:508-558)."""
    a, b, c = double_tanh_abc(lcore, lmid, ledge)
    if n == 0:
        return a * np.tanh((x - xa) / la) + b * np.tanh((x - xb) / lb) + c
    elif n == 1:
        return a / la * (np.cosh((x - xa) / la)) ** (-2.0) + b / lb * (np.cosh((x - xb) / lb)) ** (-2.0)
    else:
        raise NotImplementedError("Only derivatives up to order 1 are supported!")


def double_tanh_abc(lcore, lmid, ledge):
    """The reference's ``a, b, c`` of the double-tanh warp (a matrix product with rows (-1/2, 0, 1/2), (0, 1/2, -1/2),
    (1/2, 1/2, 0) against (l_core, l_edge, l_mid)); the device receives the same three numbers from make_kparams."""
    return (-0.5 * lcore + 0.0 * ledge + 0.5 * lmid,
            0.0 * lcore + 0.5 * ledge - 0.5 * lmid,
            0.5 * lcore + 0.5 * ledge + 0.0 * lmid)


class GibbsKernel1dTanh(GibbsKernel1d):
    r"""Gibbs kernel with the tanh warp, evaluated on the GPU.  Parameters ``[sigma_f, l_1, l_2, l_w, x_0]``."""
    _gpt_kernel_id = _lib.KERNEL_GIBBS_TANH
    __call__ = Kernel.__call__

    def __init__(self, **kwargs):
        super(GibbsKernel1dTanh, self).__init__(tanh_warp, param_names=[r"\sigma_f", "l_1", "l_2", "l_w", "x_0"], **kwargs)


class GibbsKernel1dDoubleTanh(GibbsKernel1d):
    r"""Gibbs kernel with the double-tanh warp, evaluated on the GPU.  Parameters
    ``[sigma_f, l_c, l_m, l_e, l_a, l_b, x_a, x_b]``."""
    _gpt_kernel_id = _lib.KERNEL_GIBBS_DTANH
    __call__ = Kernel.__call__

    def __init__(self, **kwargs):
        super(GibbsKernel1dDoubleTanh, self).__init__(
            double_tanh_warp, param_names=[r"\sigma_f", "l_c", "l_m", "l_e", "l_a", "l_b", "x_a", "x_b"], **kwargs)
