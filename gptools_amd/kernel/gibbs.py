r"""Gibbs non-stationary squared-exponential kernels in one dimension.

ref: gptools/kernel/gibbs.py:229-424 (GibbsKernel1d), :426-466 (tanh_warp, GibbsKernel1dTanh), :508-558 (double_tanh_warp,
GibbsKernel1dDoubleTanh), :603-801 (cubic_bucket_warp, quintic_bucket_warp and their kernels), :804-902 (exp_gauss_warp,
GibbsKernel1dExpGauss), :905-992 (BSplineWarp, GibbsKernel1dBSpline), :995-1095 (GPWarp, GibbsKernel1dGP).  With a point-dependent length scale ``l(x)``, ``a = l(x_i)``, ``b = l(x_j)``, ``s = a^2 + b^2``
and ``d = x_i - x_j``:

.. math::  k = \sigma_f^2 \sqrt{2ab/s}\, \exp(-d^2/s).

The reference hard-codes the derivative classes as expanded polynomials (terms up to ``l^8``); here they are written as
``k`` times a short factor (``a' = dl/dx`` at ``x_i``, ``b'`` at ``x_j``)::

    P = a'/(2a) - a a'/s - 2d/s + 2d^2 a a'/s^2            d k / d x_i        = k P
    Q = b'/(2b) - b b'/s + 2d/s + 2d^2 b b'/s^2            d k / d x_j        = k Q
    R = 2 a a' b b'/s^2 + 2/s + 4d b b'/s^2 - 4d a a'/s^2 - 8d^2 a a' b b'/s^3
                                                           d2 k / dx_i dx_j   = k (P Q + R)

``GibbsKernel1d(l_func)`` evaluates that on the host in numpy for any warp (the Python-kernel route of
``GaussianProcess``: pair list, then ``fit_matrix`` on the GPU).  ``GibbsKernel1dTanh``, ``GibbsKernel1dDoubleTanh``,
``GibbsKernel1dCubicBucket``, ``GibbsKernel1dQuinticBucket``, ``GibbsKernel1dExpGauss``, the cubic ``GibbsKernel1dBSpline`` and
``GibbsKernel1dGP`` with a nested 1-D squared-exponential kernel are native: the HIP library evaluates them (``GPT_KERNEL_GIBBS_*``, gptools_amd/csrc/kpair.hpp and gibbs_lfunc.hpp) with the
length-scale functions hoisted out of the builder's pair loop.  A subclass that overrides ``__call__`` is a Python kernel again;
so is a ``GibbsKernel1dExpGauss`` with more Gaussians than the device kernel carries (``_lib.GIBBS_MAX_GAUSS``) and a
``GibbsKernel1dBSpline`` of another degree than 3 or with more knots than ``_lib.GIBBS_MAX_KNOTS`` and a ``GibbsKernel1dGP`` with
another nested kernel, a free nested amplitude or more points than ``_lib.GIBBS_MAX_GP_POINTS``.
Derivative orders above ``[1, 1]`` and hyperparameter derivatives raise ``NotImplementedError`` like the reference.
"""
import inspect
import sys

import numpy as np
import scipy.linalg

from .core import Kernel
from .. import _lib
from ..splines import spev

__all__ = ["GibbsKernel1d", "GibbsKernel1dTanh", "GibbsKernel1dDoubleTanh", "GibbsKernel1dCubicBucket",
           "GibbsKernel1dQuinticBucket", "GibbsKernel1dExpGauss", "BSplineWarp", "GibbsKernel1dBSpline", "GPWarp", "GibbsKernel1dGP", "tanh_warp",
           "double_tanh_warp", "cubic_bucket_warp", "quintic_bucket_warp", "exp_gauss_warp"]


def gibbs_1d(x, y, ni, nj, lx, ly, lx1, ly1, zero_nan=False):
    """``k / sigma_f^2`` of the pairs ``(x[m], y[m])`` with orders ``ni[m], nj[m]`` in {0, 1}, from the warp values ``l``
    and slopes ``l'`` at both points.  ``zero_nan``: a length scale of exactly zero at either point makes every derivative
    class NaN (the B-spline warp, which is zero over whole intervals)."""
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
        if zero_nan:
            # a length scale of exactly zero at either point: the reference divides its derivative classes by sqrt(2 l l') -> 0/0
            # (gibbs.py:358, :371, :415); k Q above is 0 * finite where only the OTHER point's l is zero.  Applied for the
            # B-spline warp alone, as on the device (kpair.hpp, gibbs_h_other): the other warps keep the numbers they had
            out = np.where(((ni == 1) | (nj == 1)) & ((lx == 0.0) | (ly == 0.0)), np.nan, out)
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
        return self.params[0] ** 2 * gibbs_1d(x, y, ni[:, 0], nj[:, 0], lx, ly, lx1, ly1,
                                              zero_nan=isinstance(self.l_func, BSplineWarp))


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


def _bucket_sections(x, x0, w1, w2, w3):
    """Centres of the two joins and the five 0/1 masks of a bucket, in the reference's order of operations (gibbs.py:627-639)."""
    x1 = x0 - w2 / 2.0 - w1 / 2.0
    x2 = x0 + w2 / 2.0 + w3 / 2.0
    masks = (x <= (x1 - w1 / 2.0),
             (x > (x1 - w1 / 2.0)) & (x < (x1 + w1 / 2.0)),
             (x >= (x1 + w1 / 2.0)) & (x <= x2 - w3 / 2.0),
             (x > (x2 - w3 / 2.0)) & (x < (x2 + w3 / 2.0)),
             x >= (x2 + w3 / 2.0))
    return x1, x2, masks


def cubic_bucket_warp(x, n, l1, l2, l3, x0, w1, w2, w3):
    r"""Piecewise cubic "bucket": ``l_1`` left of the bucket, ``l_2`` inside it (centre ``x_0``, width ``w_2``), ``l_3`` right of
    it, joined by cubic sections of widths ``w_1`` and ``w_3``; its slope for ``n = 1`` (ref: gibbs.py:603-651).

    Written as the reference writes it -- every section's value times its 0/1 mask, summed -- because that sum defines the
    function: a non-finite section value times a zero mask is NaN (``w_1 = 0``: NaN everywhere), negative widths make the masks
    overlap or leave gaps."""
    x = np.asarray(x, dtype=float)
    x1, x2, (m0, m1, m2, m3, m4) = _bucket_sections(x, x0, w1, w2, w3)
    with np.errstate(all="ignore"):
        s1 = (x - x1 + w1 / 2.0) / w1
        s2 = (x - x2 + w3 / 2.0) / w3
        if n == 0:
            return (l1 * m0 + (-2.0 * (l2 - l1) * (s1 ** 3 - 3.0 / 2.0 * s1 ** 2) + l1) * m1 + l2 * m2 +
                    (-2.0 * (l3 - l2) * (s2 ** 3 - 3.0 / 2.0 * s2 ** 2) + l2) * m3 + l3 * m4)
        elif n == 1:
            return ((-2.0 * (l2 - l1) * (3 * s1 ** 2 - 3.0 * s1) / w1) * m1 +
                    (-2.0 * (l3 - l2) * (3 * s2 ** 2 - 3.0 * s2) / w3) * m3)
    raise NotImplementedError("Only up to first derivatives are supported!")


def quintic_bucket_warp(x, n, l1, l2, l3, x0, w1, w2, w3):
    r"""The bucket of :func:`cubic_bucket_warp` with quintic joins (continuous second derivative) (ref: gibbs.py:695-760); the
    same masked-sum form."""
    x = np.asarray(x, dtype=float)
    x1, x2, (m0, m1, m2, m3, m4) = _bucket_sections(x, x0, w1, w2, w3)
    with np.errstate(all="ignore"):
        s1 = 2.0 * (x - x1) / w1
        s3 = 2.0 * (x - x2) / w3
        if n == 0:
            return (l1 * m0 +
                    (0.5 * (l2 - l1) * (3.0 / 8.0 * s1 ** 5 - 5.0 / 4.0 * s1 ** 3 + 15.0 / 8.0 * s1) + (l1 + l2) / 2.0) * m1 +
                    l2 * m2 +
                    (0.5 * (l3 - l2) * (3.0 / 8.0 * s3 ** 5 - 5.0 / 4.0 * s3 ** 3 + 15.0 / 8.0 * s3) + (l2 + l3) / 2.0) * m3 +
                    l3 * m4)
        elif n == 1:
            return ((0.5 * (l2 - l1) * (5.0 * 3.0 / 8.0 * s1 ** 4 - 3.0 * 5.0 / 4.0 * s1 ** 2 + 15.0 / 8.0) / w1) * m1 +
                    (0.5 * (l3 - l2) * (5.0 * 3.0 / 8.0 * s3 ** 4 - 3.0 * 5.0 / 4.0 * s3 ** 2 + 15.0 / 8.0) / w3) * m3)
    raise NotImplementedError("Only up to first derivatives are supported!")


def exp_gauss_warp(X, n, l0, *msb):
    r"""``l = l_0 \exp(\sum_i \beta_i \exp(-(x - \mu_i)^2 / (2 \sigma_i^2)))`` (``n = 0``) or its slope (``n = 1``); ``msb``: the
    means, then the standard deviations, then the weights (ref: gibbs.py:804-855).  The thirds of ``msb`` are split with integer
    division (the reference's ``len(msb) / 3`` is a float under Python 3 and cannot index)."""
    X = np.asarray(X, dtype=float)
    msb = np.asarray(msb, dtype=float)
    G = len(msb) // 3
    mm, ss, bb = msb[:G], msb[G:2 * G], msb[2 * G:]
    with np.errstate(all="ignore"):
        if n == 0:
            l = np.zeros_like(X)
            for m, s, b in zip(mm, ss, bb):
                l += b * np.exp(-(X - m) ** 2.0 / (2.0 * s ** 2.0))
            return l0 * np.exp(l)
        elif n == 1:
            l1 = np.zeros_like(X)
            l2 = np.zeros_like(X)
            for m, s, b in zip(mm, ss, bb):
                term = b * np.exp(-(X - m) ** 2.0 / (2.0 * s ** 2.0))
                l1 += term
                l2 += term * (X - m) / s ** 2.0
            return -l0 * np.exp(l1) * l2
    raise NotImplementedError("Only n <= 1 is supported!")


_BUCKET_NAMES = [r"\sigma_f", "l_1", "l_2", "l_3", "x_0", "w_1", "w_2", "w_3"]


class GibbsKernel1dCubicBucket(GibbsKernel1d):
    r"""Gibbs kernel with the cubic bucket, evaluated on the GPU.  Parameters ``[sigma_f, l_1, l_2, l_3, x_0, w_1, w_2, w_3]``."""
    _gpt_kernel_id = _lib.KERNEL_GIBBS_CUBIC
    __call__ = Kernel.__call__

    def __init__(self, **kwargs):
        super(GibbsKernel1dCubicBucket, self).__init__(cubic_bucket_warp, param_names=list(_BUCKET_NAMES), **kwargs)


class GibbsKernel1dQuinticBucket(GibbsKernel1d):
    r"""Gibbs kernel with the quintic bucket, evaluated on the GPU.  Parameters as :class:`GibbsKernel1dCubicBucket`."""
    _gpt_kernel_id = _lib.KERNEL_GIBBS_QUINTIC
    __call__ = Kernel.__call__

    def __init__(self, **kwargs):
        super(GibbsKernel1dQuinticBucket, self).__init__(quintic_bucket_warp, param_names=list(_BUCKET_NAMES), **kwargs)


class GibbsKernel1dExpGauss(GibbsKernel1d):
    r"""Gibbs kernel whose length scale is an exponential of ``n_gaussians`` Gaussians, evaluated on the GPU.  Parameters
    ``[sigma_f, l_0, mu_1 .., sigma_1 .., beta_1 ..]`` (ref: gibbs.py:858-902).

    The device kernel carries up to ``_lib.GIBBS_MAX_GAUSS`` Gaussians.  With more, the constructor returns an instance of a
    subclass whose ``__call__`` is the host ``GibbsKernel1d``'s -- a Python kernel by the rule above, with the same numbers.
    That switch is made for this class only: a user subclass that keeps the native ``__call__`` and asks for more Gaussians
    than the cap stays a native kernel and gets the library's ``ValueError`` (``GPT_GIBBS_MAX_GAUSS``) at its first evaluation;
    it takes the host route by overriding ``__call__`` (``__call__ = GibbsKernel1d.__call__``), like any Python kernel."""
    _gpt_kernel_id = _lib.KERNEL_GIBBS_EXPGAUSS
    __call__ = Kernel.__call__

    def __new__(cls, n_gaussians=None, **kwargs):
        if cls is GibbsKernel1dExpGauss and n_gaussians is not None and n_gaussians > _lib.GIBBS_MAX_GAUSS:
            cls = _GibbsKernel1dExpGaussHost
        return super(GibbsKernel1dExpGauss, cls).__new__(cls)

    def __init__(self, n_gaussians, **kwargs):
        super(GibbsKernel1dExpGauss, self).__init__(
            exp_gauss_warp, num_params=3 * n_gaussians + 2,
            param_names=([r"\sigma_f", "l_0"] + [r"\mu_{{{:d}}}".format(i + 1) for i in range(n_gaussians)] +
                         [r"\sigma_{{{:d}}}".format(i + 1) for i in range(n_gaussians)] +
                         [r"\beta_{{{:d}}}".format(i + 1) for i in range(n_gaussians)]),
            **kwargs)


class _GibbsKernel1dExpGaussHost(GibbsKernel1dExpGauss):
    """``GibbsKernel1dExpGauss`` beyond the device kernel's cap: evaluated on the host."""
    __call__ = GibbsKernel1d.__call__


class BSplineWarp(object):
    r"""Length-scale function that is a B-spline of fixed degree ``k`` (default 3) with free knots and coefficients
    (ref: gibbs.py:905-941).  ``warp(X, n, t_1 .. t_nt, C_1 .. C_{nt+k-1})`` is the spline (``n = 0``) or its ``n``-th
    derivative at ``X`` (the first column of a 2-D ``X``), in the shape of ``X``; ``nt = (len(tC) - k + 1) // 2``.  Outside
    ``[t_1, t_nt]`` the spline, and with it the length scale, is zero: keep the boundary knots at or beyond the data."""

    def __init__(self, k=3):
        self.k = k

    def __call__(self, X, n, *tC):
        X = np.asarray(X, dtype=float)
        shape = X.shape
        if X.ndim == 2:
            X = X[:, 0]
        tC = np.asarray(tC, dtype=float)
        nt = (len(tC) - self.k + 1) // 2
        return np.reshape(spev(tC[:nt], tC[nt:], self.k, X, n=n), shape)


class GibbsKernel1dBSpline(GibbsKernel1d):
    r"""Gibbs kernel whose length scale is a B-spline of degree ``k`` on ``nt`` free knots.  Parameters
    ``[sigma_f, t_1 .. t_nt, C_1 .. C_{nt+k-1}]`` (ref: gibbs.py:944-992).  Put the two outer knots at or beyond the edges of
    the data (the length scale is zero outside them) and keep the coefficients positive (the spline lies in their hull).
    Knots out of increasing order raise ``ValueError("Knots must be in increasing order!")`` at evaluation.

    The cubic kernel with ``2 <= nt <= _lib.GIBBS_MAX_KNOTS`` is evaluated on the GPU.  For another degree or knot count the
    constructor returns an instance of a subclass whose ``__call__`` is the host ``GibbsKernel1d``'s -- a Python kernel, with
    the same numbers.  As for :class:`GibbsKernel1dExpGauss` that switch is made for this class only: a user subclass that keeps
    the native ``__call__`` stays native and gets the library's ``ValueError`` beyond the cap."""
    _gpt_kernel_id = _lib.KERNEL_GIBBS_BSPLINE
    __call__ = Kernel.__call__

    def __new__(cls, nt=None, k=3, **kwargs):
        if cls is GibbsKernel1dBSpline and nt is not None and (k != 3 or not 2 <= nt <= _lib.GIBBS_MAX_KNOTS):
            cls = _GibbsKernel1dBSplineHost
        return super(GibbsKernel1dBSpline, cls).__new__(cls)

    def __init__(self, nt, k=3, **kwargs):
        super(GibbsKernel1dBSpline, self).__init__(
            BSplineWarp(k=k), num_params=2 * nt + k,
            param_names=([r"\sigma_f"] + [r"t_{{{:d}}}".format(i + 1) for i in range(nt)] +
                         [r"C_{{{:d}}}".format(i + 1) for i in range(nt + k - 1)]),
            **kwargs)


class _GibbsKernel1dBSplineHost(GibbsKernel1dBSpline):
    """``GibbsKernel1dBSpline`` of a degree or knot count the device kernel does not carry: evaluated on the host."""
    __call__ = GibbsKernel1d.__call__


class GPWarp(object):
    r"""Length-scale function that is the mean of a small noiseless Gaussian process through ``npts`` free values at free
    locations (ref: gibbs.py:995-1036).  ``warp(X, n, *hpXy)`` is that mean (``n = 0``) or its slope (``n = 1``) at ``X``, in the
    shape of ``X``; ``hpXy`` holds the free hyperparameters of the nested kernel ``k``, then ``x_1 .. x_npts``, then
    ``y_1 .. y_npts``.  With ``K`` the nested kernel over the ``x_j``, ``K_tot = K + 1e2 eps I`` (the reference's nested
    ``GaussianProcess``: no noise, ``diag_factor = 1e2``) and ``alpha = K_tot^-1 y`` (``cho_factor(lower=True)`` /
    ``cho_solve``), the mean is ``K_*(X) alpha``.

    For a nested kernel whose type is exactly ``SquaredExponentialKernel`` with ``num_dim == 1``, parameters ``[sigma_n, l]``,
    that is a closed form evaluated here in numpy, and the statement the device kernel ``GPT_KERNEL_GIBBS_GP`` is compared with::

        l(x)  =  sum_j c_j exp(-(x - x_j)^2 / (2 l^2))
        l'(x) = -sum_j c_j exp(-(x - x_j)^2 / (2 l^2)) (x - x_j) / l^2
        c     = sigma_n^2 (sigma_n^2 E + 1e2 eps I)^-1 y,       E_ij = exp(-(x_i - x_j)^2 / (2 l^2))

    (terms added in index order).  Any other nested kernel is evaluated through its own ``__call__``, with the same solve.

    Deliberate differences from the reference:

    * ``k=None`` builds the default the reference documents -- a squared-exponential kernel with ``sigma_f = 1`` fixed and
      ``l_1 = 1`` free, the class's default bounds.  The reference cannot construct it: its ``GPWarp(npts)`` raises
      ``GPArgumentError("Must pass explicit parameter values if fixing parameters!")`` and only works with a kernel passed in.
    * The warp is a pure function of its arguments: the weights are recomputed at every call and the nested kernel's own
      hyperparameters are left as they were.  The reference routes through a nested ``GaussianProcess`` whose
      ``update_hyperparameters`` can decline to refit (bounds, a swallowed ``LinAlgError``) and then predicts from stale state.
    * A nested matrix that does not factor raises ``numpy.linalg.LinAlgError`` -- and so does one that factors only by the
      ``1e2 eps`` on its diagonal: a squared pivot of the Cholesky factor at or below ``pivot_factor`` (10) times that jitter.  Two
      ``x_j`` that coincide (to about ``1e-6 l``) with values that differ are the case: the reference's nested fit succeeds
      there, with weights of the order ``1e12`` whose sum leaves a length scale of two digits; here the evaluation fails and
      ``update_hyperparameters`` counts it as ``+inf``.  The condition numbers an optimiser meets otherwise (the fixture's: up to
      344) are ten orders of magnitude away from that threshold."""

    diag_factor = 1e2
    pivot_factor = 10.0

    def __init__(self, npts, k=None):
        if isinstance(npts, bool) or not isinstance(npts, (int, np.integer)) or npts < 1:
            raise ValueError("npts must be an integer > 0!")
        self.npts = int(npts)
        if k is None:
            from .squared_exponential import SquaredExponentialKernel
            k = SquaredExponentialKernel(initial_params=[1.0, 1.0], fixed_params=[True, False],
                                         param_bounds=[(0.0, 1e16), (0.0, 1e16)])
        if not isinstance(k, Kernel):
            raise TypeError("k must be an instance of type Kernel!")
        if k.num_dim != 1:
            raise ValueError("Gibbs kernel only supports 1d data.")
        self.k = k

    def _closed_form(self):
        """The nested kernel is exactly a 1-D ``SquaredExponentialKernel``: the closed form applies."""
        from .squared_exponential import SquaredExponentialKernel
        return type(self.k) is SquaredExponentialKernel and self.k.num_dim == 1

    def split(self, hpXy):
        """``(p, x, y)``: the nested kernel's full parameter array with its free entries taken from ``hpXy``, the points, the
        values."""
        hpXy = np.asarray(hpXy, dtype=float).ravel()
        nf = self.k.num_free_params
        if len(hpXy) != nf + 2 * self.npts:
            raise ValueError("%d values given for %d nested hyperparameters and 2 x %d points" % (len(hpXy), nf, self.npts))
        p = np.array(self.k.params, dtype=float)
        p[self.k.free_param_idxs] = hpXy[:nf]
        return p, hpXy[nf:nf + self.npts], hpXy[nf + self.npts:]

    def _solve(self, K, y):
        K_tot = K + self.diag_factor * sys.float_info.epsilon * np.eye(self.npts)
        if not np.isfinite(K_tot).all():
            raise np.linalg.LinAlgError("the nested covariance matrix of GPWarp is not finite")
        c, low = scipy.linalg.cho_factor(K_tot, lower=True)
        if (np.diagonal(c) ** 2.0).min() <= self.pivot_factor * self.diag_factor * sys.float_info.epsilon:
            raise np.linalg.LinAlgError("the nested covariance matrix of GPWarp factors only by the jitter on its diagonal "
                                        "(coincident points?)")
        return scipy.linalg.cho_solve((c, low), y)

    def weights(self, *hpXy):
        """``(l, x, c)`` of the closed form above: what the device kernel takes.  ``ValueError`` for a nested kernel that is not
        exactly a 1-D ``SquaredExponentialKernel`` (its parameters are not ``[sigma_n, l]``)."""
        if not self._closed_form():
            raise ValueError("GPWarp.weights: the closed form needs a nested 1-D SquaredExponentialKernel, got %s"
                             % type(self.k).__name__)
        p, x, y = self.split(hpXy)
        with np.errstate(all="ignore"):
            d = x[:, None] - x[None, :]
            E = np.exp(-d ** 2.0 / (2.0 * p[1] ** 2.0))
            s2 = p[0] ** 2.0
            return p[1], x, s2 * self._solve(s2 * E, y)

    def __call__(self, X, n, *hpXy):
        if n not in (0, 1):
            raise NotImplementedError("Only derivatives up to order 1 are supported!")
        X = np.asarray(X, dtype=float)
        shape = X.shape
        xs = X[:, 0] if X.ndim == 2 else X.ravel()
        if self._closed_form():
            l, x, c = self.weights(*hpXy)
            out = np.zeros_like(xs)
            with np.errstate(all="ignore"):
                for xj, cj in zip(x, c):
                    term = cj * np.exp(-(xs - xj) ** 2.0 / (2.0 * l ** 2.0))
                    out += term if n == 0 else term * (xs - xj) / l ** 2.0
            return np.reshape(out if n == 0 else -out, shape)
        p, x, y = self.split(hpXy)
        k, keep = self.k, np.array(self.k.params, dtype=float)
        m, M = self.npts, len(xs)
        zm = np.zeros((m * m, 1), dtype=int)
        try:
            k.params = p
            K = np.reshape(k(np.repeat(x, m)[:, None], np.tile(x, m)[:, None], zm, zm, symmetric=True), (m, m))
            alpha = self._solve(np.asarray(K, dtype=float), y)
            Ks = np.reshape(k(np.repeat(xs, m)[:, None], np.tile(x, M)[:, None], np.full((M * m, 1), n, dtype=int),
                              np.zeros((M * m, 1), dtype=int)), (M, m))
        finally:
            k.params = keep
        return np.reshape(np.asarray(Ks, dtype=float).dot(alpha), shape)


class GibbsKernel1dGP(GibbsKernel1d):
    r"""Gibbs kernel whose length scale interpolates ``npts`` free values ``y_j`` at free locations ``x_j`` with a small nested
    Gaussian process (:class:`GPWarp`; ref: gibbs.py:1039-1095).  Parameters ``[sigma_f, (free nested hyperparameters), x_1 ..
    x_npts, y_1 .. y_npts]``.  Keep the outer points near the edges of the data (the nested GP goes to zero away from its points)
    and the values positive.  ``k=None``: see :class:`GPWarp` (the reference fails there).

    With a nested kernel that is exactly a 1-D ``SquaredExponentialKernel`` whose ``l_1`` is free and ``sigma_f`` fixed and with
    ``npts <= _lib.GIBBS_MAX_GP_POINTS`` the kernel is evaluated on the GPU: the library gets ``[sigma_f, l, x_1 .., c_1 ..]``
    with the nested GP's weights ``c`` (:meth:`_native_params`; an ``npts x npts`` solve on the host per hyperparameter vector).
    For another nested kernel, a free nested ``sigma_f`` or more points the constructor returns an instance of a subclass whose
    ``__call__`` is the host ``GibbsKernel1d``'s -- a Python kernel, with the same numbers.  As for :class:`GibbsKernel1dBSpline`
    that switch is made for this class only: a user subclass that keeps the native ``__call__`` with such a nested kernel or point
    count stays native and gets a ``ValueError`` at its first evaluation (from :meth:`_native_params`, or the library's beyond the
    cap); it takes the host route by overriding ``__call__``, like any Python kernel.  Coincident ``x_j``: see :class:`GPWarp`."""
    _gpt_kernel_id = _lib.KERNEL_GIBBS_GP
    __call__ = Kernel.__call__

    @staticmethod
    def _device_form(npts, k):
        from .squared_exponential import SquaredExponentialKernel
        if npts is None or not 1 <= npts <= _lib.GIBBS_MAX_GP_POINTS:
            return False
        if k is None or not isinstance(k, Kernel):
            return True                                     # (not a Kernel: GPWarp's constructor raises the TypeError)
        fixed = np.asarray(k.fixed_params, dtype=bool)
        return type(k) is SquaredExponentialKernel and k.num_dim == 1 and bool(fixed[0]) and not bool(fixed[1])

    def __new__(cls, npts=None, k=None, **kwargs):
        if cls is GibbsKernel1dGP and npts is not None and not cls._device_form(npts, k):
            cls = _GibbsKernel1dGPHost
        return super(GibbsKernel1dGP, cls).__new__(cls)

    def __init__(self, npts, k=None, **kwargs):
        w = GPWarp(npts, k=k)
        super(GibbsKernel1dGP, self).__init__(
            w, num_params=w.k.num_free_params + 2 * npts + 1,
            param_names=([r"\sigma_f"] + [str(s) for s in w.k.free_param_names[:]] +
                         [r"x_{{{:d}}}".format(i + 1) for i in range(npts)] +
                         [r"y_{{{:d}}}".format(i + 1) for i in range(npts)]),
            **kwargs)

    def _native_params(self):
        """``[sigma_f, l, x_1 .. x_m, c_1 .. c_m]``: what ``GPT_KERNEL_GIBBS_GP`` takes (the weights, not the values)."""
        w = self.l_func
        if not w._closed_form() or w.k.num_free_params != 1 or bool(np.asarray(w.k.fixed_params, dtype=bool)[1]):
            raise ValueError("GibbsKernel1dGP: the device kernel takes a nested 1-D SquaredExponentialKernel with sigma_f fixed and "
                             "l_1 free; override __call__ (GibbsKernel1d.__call__) for the host route")
        p = np.array(self.params, dtype=float)
        l, x, c = w.weights(*p[1:])
        return np.concatenate(([p[0], l], x, c))


class _GibbsKernel1dGPHost(GibbsKernel1dGP):
    """``GibbsKernel1dGP`` with a nested kernel or a number of points the device kernel does not carry: evaluated on the host."""
    __call__ = GibbsKernel1d.__call__
