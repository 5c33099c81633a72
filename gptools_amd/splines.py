r"""B-, M- and I-splines on a free knot grid, with derivatives (ref: gptools/splines.py:5-146).

With the internal knots ``t_1 <= ... <= t_M`` and ``deg`` copies of the two boundary knots appended on either side (the padded
vector ``t`` below), the basis functions of degree ``d`` follow the Cox--de Boor recursion

.. math::  B_{i,0} = [t_i \le x < t_{i+1}], \qquad
           B_{i,d} = \frac{x - t_i}{t_{i+d} - t_i} B_{i,d-1} + \frac{t_{i+d+1} - x}{t_{i+d+1} - t_{i+1}} B_{i+1,d-1},

a term with a zero knot difference left out; the last span also holds ``x = t_M`` (continuity at the right-hand end).  The
M-splines are the same functions normalised to unit integral, ``M_{i,d} = (d + 1) B_{i,d} / (t_{i+d+1} - t_i)``, built level by
level with the factor ``(d + 1) / (d (t_{i+d+1} - t_i))``, and the I-splines their running integrals,
``I_i = \sum_{m \ge i} (t_{m+deg+1} - t_m) M_m / (deg + 1)``, ``i = 0`` (a constant) included.  A derivative differences the
coefficients and drops one degree: ``C_{i+1} - C_i`` for a B-spline, ``(deg + 1) (C_{i+1} / (t_{i+deg+2} - t_{i+1}) - C_i /
(t_{i+deg+1} - t_i))`` for an M-spline, both onto the M-splines of degree ``deg - 1``; an I-spline's derivative is the M-spline
of degree ``deg - 1`` without the constant.

The Gibbs kernel with a B-spline length scale (``kernel/gibbs.py``: ``BSplineWarp``, and on the device ``gpt_gibbs_bspline`` in
``csrc/gibbs_lfunc.hpp``) and the I-spline input warp (``kernel/warping.py``) evaluate their splines through :func:`spev`.
"""
import numpy as np

__all__ = ["spev"]


def _padded(t_int, deg):
    return np.concatenate((np.full(deg, t_int[0]), t_int, np.full(deg, t_int[-1])))


def _basis(t_int, deg, x, m_spline):
    """The ``M + deg - 1`` basis functions of degree ``deg`` at ``x``: an array ``(len(x), M + deg - 1)``."""
    nt = len(t_int)
    t = _padded(t_int, deg)
    nb = len(t) - 1                     # functions of degree 0 (one per knot interval; only the internal ones are non-zero)
    last = deg + nt - 2                 # the last internal interval
    prev = np.zeros((nb, len(x)))
    for i in range(deg, last + 1):
        inside = (t[i] <= x) & ((x < t[i + 1]) | ((i == last) & (x == t[-1])))
        if inside.any():
            prev[i, inside] = 1.0 / (t[i + 1] - t[i]) if m_spline else 1.0
    for d in range(1, deg + 1):
        cur = np.zeros((nb, len(x)))
        for i in range(deg - d, last + 1):
            left, right = t[i + d] != t[i], t[i + d + 1] != t[i + 1]
            if left:
                term = (x - t[i]) * prev[i]
                cur[i] += term if m_spline else term / (t[i + d] - t[i])
            if right:
                term = (t[i + d + 1] - x) * prev[i + 1]
                cur[i] += term if m_spline else term / (t[i + d + 1] - t[i + 1])
            if m_spline and (left or right):
                cur[i] *= (d + 1) / (d * (t[i + d + 1] - t[i]))
        prev = cur
    return prev[:nt + deg - 1].T


def spev(t_int, C, deg, x, cov_C=None, M_spline=False, I_spline=False, n=0):
    """Evaluate a B-, M- or I-spline, or its ``n``-th derivative, at ``x``.

    Parameters
    ----------
    t_int : array of float, (`M`,)
        The internal knots, in increasing order (repeats allowed).  ``deg`` boundary knots are appended on both sides.
    C : array of float, (`M + deg - 1`,)
        The coefficients of the basis functions.
    deg : nonnegative int
        The polynomial degree.
    x : array of float, (`N`,)
        Where to evaluate.  Outside ``[t_1, t_M]`` every basis function is zero.
    cov_C : array of float, (`M + deg - 1`,) or (`M + deg - 1`, `M + deg - 1`), optional
        Variances or the covariance matrix of the coefficients; with it the result is ``(y, cov_y)``.  For a derivative of an
        I-spline the constant's entries are dropped with its coefficient.  (Derivatives of B- and M-splines difference the
        coefficients and, like the reference, hand ``cov_C`` on unchanged: give the covariance of the differenced ones.)
    M_spline : bool, optional
        M-splines (unit integral) instead of B-splines (partition of unity).
    I_spline : bool, optional
        I-splines of degree ``deg``: the integrals of the M-splines of that degree, the first (``i = 0``) a constant offset --
        set ``C[0] = 0`` to start at zero.  Overrides `M_spline`.  Monotone when the coefficients share a sign.
    n : int, optional
        Derivative order.  ``n > deg`` gives zeros (the jumps are not represented).
    """
    C = np.asarray(C, dtype=float)
    t_int = np.asarray(t_int, dtype=float)
    if (t_int != np.sort(t_int)).any():
        raise ValueError("Knots must be in increasing order!")
    x = np.asarray(x, dtype=float)
    if n > deg:
        return np.zeros_like(x, dtype=float)
    if I_spline:
        if n > 0:
            # d/dx of the integral: the M-spline itself, one degree down; the constant goes, its variance and covariances with it
            if cov_C is not None:
                cov_C = np.asarray(cov_C)
                cov_C = cov_C[1:] if cov_C.ndim == 1 else cov_C[1:, 1:]
            return spev(t_int, C[1:], deg - 1, x, cov_C=cov_C, M_spline=True, n=n - 1)
        # (n = 0 keeps the whole covariance: the reference drops the constant's row and column here too, while it keeps the
        # coefficient, and fails on the shapes)
        M_spline = True
    if n > 0:
        nt = len(t_int)
        if M_spline:
            t = _padded(t_int, deg)
            nc = nt + deg - 1
            C = (deg + 1.0) * (C[1:] / (t[deg + 2:nc + deg + 1] - t[1:nc]) - C[:-1] / (t[deg + 1:nc + deg] - t[:nc - 1]))
        else:
            C = C[1:] - C[:-1]
        return spev(t_int, C, deg - 1, x, cov_C=cov_C, M_spline=True, n=n - 1)
    if len(C) != len(t_int) + deg - 1:
        raise ValueError("Length of C must be equal to M + deg - 1!")
    B = _basis(t_int, deg, x, M_spline)
    if I_spline:
        t = _padded(t_int, deg)
        I = np.zeros_like(B)
        for i in range(len(C)):
            for m in range(i, len(C)):
                I[:, i] += (t[m + deg + 1] - t[m]) * B[:, m] / (deg + 1.0)
        B = I
    # the basis functions summed in their order, one product at a time: the device's B-spline length scale (gpt_gibbs_bspline,
    # csrc/gibbs_lfunc.hpp) adds the four that are non-zero in the same order, and the zeros in between change nothing -- a
    # matrix product would leave the order, and with it the last bits where the spline crosses zero, to the BLAS at hand
    y = np.zeros(B.shape[0])
    for i in range(len(C)):
        y = y + B[:, i] * C[i]
    if cov_C is not None:
        cov_C = np.asarray(cov_C)
        if cov_C.ndim == 1:
            cov_C = np.diag(cov_C)
        return y, B.dot(cov_C).dot(B.T)
    return y
