#!/usr/bin/env python
"""g18_gibbs_bspline.npz: the spline module and the two kernels built on it, from the imported reference (ref: splines.py:5-146,
kernel/gibbs.py:905-992, kernel/warping.py:404-462, :718-758).  Seeded; needs the reference tree (``ref_harness``).  The reference's ``WarpingFunction`` names Python 2's
``long``: ``builtins.long = int`` is set before the import.

Layout:
  * ``spev__x``, ``spev__t_<grid>``, ``spev__C_<grid>_d<deg>``, ``spev_<grid>_<form>_d<deg>_n<n>``: ``spev`` tables at 60 points
    that hold every knot, both boundary knots and two points outside; forms ``B``, ``M``, ``I``; degrees 1 to 3; derivative orders
    0 .. deg + 1; grids ``u`` (6 distinct knots) and ``r`` (a repeated internal knot).  ``spev_cov1__{var, y, cov}`` (B-spline,
    variances) and ``spev_cov2__{cov_C, y, cov}`` (the first derivative of an I-spline, a full covariance matrix: the constant's row
    and column go with its coefficient; at n = 0 the reference drops them but keeps the coefficient, and fails).
  * ``pairs_<case>__{xi, xj, ni, nj, params, k}``: GibbsKernel1dBSpline pair lists, 1200 pairs per case over all four derivative
    classes with coincident points: a single span (``nt2``), six non-uniform knots (``nt6``), the device kernel's cap (``nt11``), a
    repeated internal knot (``rep``), points at every knot and at both boundaries (``knots``), points outside the knot range where
    the length scale is zero (``out``: both outside NaN; one outside 0 in the value class, NaN in the others), a negative
    coefficient (``neg``: the length scale changes sign, mixed-sign pairs are NaN).
  * ``kij__*``: compute_Kij of the ``nt6`` kernel, symmetric and a 30-row rectangle, mixed orders.
  * ``terms__*`` / ``terms_<case>__*``: the kernel alone, + SE, x SE and with T: ll, alpha, predict at n = 0 / 1.
  * ``isw__*``: an ISplineWarpedKernel pair list around a 2-D squared exponential, 4 knots in one dimension and 3 in the other,
    orders 0 and 1; ``isw__w<d>_n<n>``: the warp of dimension d and its first two derivatives at the row points;
    ``isw__order2_error``: the message of the ValueError the reference raises for an order of 2.
``bspline`` / ``make_terms_gp`` / ``isw_kernel`` build the models from either package.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_g17_gibbs_more as G17      # noqa: E402  (terms_data: the data of its terms block)

MAX_KNOTS = 11     # the device kernel's cap (GPT_GIBBS_MAX_KNOTS)
M_PAIRS = 1200
T6 = [0.0, 0.3, 0.7, 1.1, 1.6, 2.0]
T6_REP = [0.0, 0.4, 0.9, 0.9, 1.5, 2.0]
C6 = [0.9, 0.5, 0.3, 0.6, 1.1, 0.4, 0.7, 1.0]
_rs11 = np.random.RandomState(1811)
T11 = [0.0] + list(np.sort(_rs11.uniform(0.1, 1.9, 9))) + [2.0]
C11 = list(_rs11.uniform(0.2, 1.2, 13))
PAIR_CASES = {
    "nt2": [1.0] + [0.0, 2.0] + [0.8, 0.3, 1.1, 0.5],
    "nt6": [1.3] + T6 + C6,
    "nt11": [0.8] + T11 + C11,
    "rep": [1.0] + T6_REP + C6,
    "knots": [1.1] + T6 + C6,
    "out": [1.0] + T6 + C6,
    "neg": [1.0] + T6 + [0.9, 0.5, 0.3, -0.8, 1.1, 0.4, 0.7, 1.0],
}
KIJ_CASE = "nt6"
TERM_CASES = ("alone", "sum_se", "prod_se", "T")
TERM_PARAMS = [1.1] + [-0.2, 0.3, 0.8, 1.2, 1.7, 2.2] + [0.8, 0.6, 0.3, 0.35, 0.5, 0.7, 0.6, 0.9]
SPEV_GRIDS = {"u": T6, "r": T6_REP}
ISW_NT = [4, 3]
ISW_K_PARAMS = [1.2, 0.4, 0.7]
ISW_W_PARAMS = [0.0, 0.3, 0.6, 1.0, 0.5, 1.0, 0.8, 1.5, 0.7] + [0.0, 0.5, 1.0, 1.0, 0.6, 1.2, 0.9]


def nt_of(params):
    return (len(params) - 3) // 2


def bspline(g, params, k=3, bounds=(-10.0, 10.0)):
    nt = (len(params) - k) // 2
    return g.GibbsKernel1dBSpline(nt, k=k, initial_params=list(params), param_bounds=[bounds] * len(params))


def spev_x(t):
    """60 points: every knot (the boundary knots among them), two points outside, the rest spread over and beyond the range."""
    t = np.asarray(t, dtype=float)
    rest = np.linspace(t[0] - 0.05, t[-1] + 0.05, 60 - len(t) - 2)
    return np.concatenate((t, [t[0] - 0.1, t[-1] + 0.1], rest))


def spev_coeffs(grid, deg):
    rs = np.random.RandomState(1800 + 10 * sorted(SPEV_GRIDS).index(grid) + deg)
    return rs.uniform(-0.5, 1.5, len(SPEV_GRIDS[grid]) + deg - 1)


def spev_cov_inputs():
    rs = np.random.RandomState(1850)
    var = rs.uniform(0.01, 0.1, len(T6) + 2)
    A = rs.randn(len(T6) + 2, len(T6) + 2)
    return var, A.dot(A.T) / 10.0


def pair_data(case):
    rs = np.random.RandomState(1800 + sorted(PAIR_CASES).index(case))
    params = PAIR_CASES[case]
    nt = nt_of(params)
    t = np.asarray(params[1:1 + nt])
    M = M_PAIRS
    lo, hi = (-0.3, 2.3) if case == "out" else (0.0, 2.0)
    xi = rs.uniform(lo, hi, M)
    xj = rs.uniform(lo, hi, M)
    xj[:40] = xi[:40]                            # coincident points
    if case == "knots":
        xi[40:40 + 3 * nt] = np.tile(t, 3)       # at the knots: against random points, ...
        xj[40 + 2 * nt:40 + 6 * nt] = np.repeat(t, 4)      # ... against each other, random points against them
    ni = rs.randint(0, 2, M)
    nj = rs.randint(0, 2, M)
    return xi, xj, ni, nj


def kij_data():
    rs = np.random.RandomState(1801)
    X = np.sort(rs.uniform(0.0, 2.0, 40))
    n = (rs.rand(40) < 0.3).astype(int)
    Xj = rs.uniform(0.0, 2.0, 25)
    nj = (rs.rand(25) < 0.5).astype(int)
    return X, n, Xj, nj


def make_terms_gp(g, case, d):
    k = bspline(g, TERM_PARAMS)
    if case == "sum_se":
        k = k + g.SquaredExponentialKernel(num_dim=1, initial_params=[0.5, 0.7], param_bounds=[(1e-3, 10.0)] * 2)
    elif case == "prod_se":
        k = k * g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 1.5], param_bounds=[(1e-3, 10.0)] * 2)
    gp = g.GaussianProcess(k)
    if case == "T":
        gp.add_data(d["X"], d["yT"], err_y=0.01, T=d["T"])
    else:
        gp.add_data(d["X"], d["y"], err_y=0.05, n=d["n"])
    return gp


def isw_kernel(g):
    se = g.SquaredExponentialKernel(num_dim=2, initial_params=ISW_K_PARAMS, param_bounds=[(1e-3, 10.0)] * 3)
    return g.ISplineWarpedKernel(se, ISW_NT, initial_params=ISW_W_PARAMS, param_bounds=[(-10.0, 10.0)] * len(ISW_W_PARAMS))


def isw_data():
    rs = np.random.RandomState(1860)
    M = 300
    Xi, Xj = rs.uniform(0.0, 1.0, (M, 2)), rs.uniform(0.0, 1.0, (M, 2))
    Xj[:20] = Xi[:20]
    Xi[20:24, 0] = ISW_W_PARAMS[0:4]             # at the knots of dimension 0
    ni, nj = rs.randint(0, 2, (M, 2)), rs.randint(0, 2, (M, 2))
    return Xi, Xj, ni, nj


def main():
    import builtins
    builtins.long = int      # the reference's WarpingFunction tests isinstance(., (int, long)), a NameError under Python 3
    from ref_harness import import_reference
    g = import_reference()
    from gptools.splines import spev
    out = {}
    # --- spev tables
    for grid, t in sorted(SPEV_GRIDS.items()):
        x = spev_x(t)
        out["spev__t_" + grid], out["spev__x_" + grid] = np.asarray(t), x
        for deg in (1, 2, 3):
            C = spev_coeffs(grid, deg)
            out["spev__C_%s_d%d" % (grid, deg)] = C
            for form, kw in (("B", {}), ("M", dict(M_spline=True)), ("I", dict(I_spline=True))):
                for n in range(deg + 2):
                    with np.errstate(all="ignore"):
                        out["spev_%s_%s_d%d_n%d" % (grid, form, deg, n)] = np.asarray(spev(t, C, deg, x, n=n, **kw), dtype=float)
    var, cov = spev_cov_inputs()
    x = spev_x(T6)
    C = spev_coeffs("u", 3)
    out["spev_cov1__var"], out["spev_cov2__cov_C"] = var, cov
    out["spev_cov1__y"], out["spev_cov1__cov"] = spev(T6, C, 3, x, cov_C=var)
    out["spev_cov2__y"], out["spev_cov2__cov"] = spev(T6, C, 3, x, cov_C=cov, I_spline=True, n=1)
    # --- pair lists
    for case, params in sorted(PAIR_CASES.items()):
        xi, xj, ni, nj = pair_data(case)
        k = bspline(g, params)
        with np.errstate(all="ignore"):
            val = k(xi[:, None], xj[:, None], ni[:, None], nj[:, None])
        for key, v in dict(xi=xi, xj=xj, ni=ni, nj=nj, params=np.asarray(params, dtype=float), k=val).items():
            out["pairs_%s__%s" % (case, key)] = np.asarray(v)
        print(case, "nan", int(np.isnan(val).sum()), "zero", int((val == 0).sum()), "max", np.nanmax(np.abs(val)))
    # --- compute_Kij
    X, n, Xj, nj = kij_data()
    gp = g.GaussianProcess(bspline(g, PAIR_CASES[KIJ_CASE]))
    out["kij__X"], out["kij__n"], out["kij__Xj"], out["kij__nj"] = X, n, Xj, nj
    out["kij__sym"] = np.asarray(gp.compute_Kij(X[:, None], None, n[:, None], None))
    out["kij__rect"] = np.asarray(gp.compute_Kij(X[:30, None], Xj[:, None], n[:30, None], nj[:, None]))
    # --- alone, in a sum, in a product, with T
    td = G17.terms_data()
    for key, v in td.items():
        out["terms__" + key] = v
    for case in TERM_CASES:
        gp = make_terms_gp(g, case, td)
        gp.compute_K_L_alpha_ll()
        out["terms_%s__ll" % case] = np.float64(gp.ll)
        out["terms_%s__alpha" % case] = np.asarray(gp.alpha).ravel()
        out["terms_%s__mean0" % case], out["terms_%s__std0" % case] = gp.predict(td["Xs"])
        out["terms_%s__mean1" % case], out["terms_%s__std1" % case] = gp.predict(td["Xs"], n=1)
        print(case, out["terms_%s__ll" % case])
    # --- the I-spline warp around a 2-D squared exponential
    k = isw_kernel(g)
    Xi, Xj, ni, nj = isw_data()
    out["isw__Xi"], out["isw__Xj"], out["isw__ni"], out["isw__nj"] = Xi, Xj, ni, nj
    out["isw__k"] = np.asarray(k(Xi, Xj, ni, nj), dtype=float)
    for d in (0, 1):
        for n in (0, 1, 2):
            out["isw__w%d_n%d" % (d, n)] = np.asarray(k.w(Xi[:, d], d, n), dtype=float)
    try:
        k(Xi[:2], Xj[:2], 2 * np.ones((2, 2), dtype=int), nj[:2])
        raise RuntimeError("the reference accepted a derivative order of 2")
    except ValueError as e:
        out["isw__order2_error"] = np.array(str(e))
    np.savez_compressed(os.path.join(HERE, "g18_gibbs_bspline.npz"), **out)
    print("bytes", os.path.getsize(os.path.join(HERE, "g18_gibbs_bspline.npz")))


if __name__ == "__main__":
    main()
