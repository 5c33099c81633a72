#!/usr/bin/env python
"""g20_gibbs_gp.npz: ``GibbsKernel1dGP`` (ref: kernel/gibbs.py:995-1095) from the imported reference, the nested kernel given
explicitly (the reference's default ``k=None`` cannot be constructed).  Seeded; needs the reference tree (``ref_harness``).  The
reference's ``MaskedKernel`` removes entries from ``range(...)``: ``gptools.kernel.core`` gets a list-returning ``range``, as in
``gen_g19_masked.py``.  Nothing of the reference is copied: only the inputs and its results are stored.

Layout:
  * ``pairs_<case>__{xi, xj, ni, nj, params, sigma_n, k, l, dl}`` for the four length-scale cases ``CASES``: 300 pairs on [0, 2] with
    orders 0 or 1 on each side; rows 0-9 coincident, the next rows at the ``x_j`` themselves (at most 12), the last four rows
    outside the hull of the points (-0.4, 2.3, -1.0, 3.5); ``l`` / ``dl``: the reference's ``l_func`` and its slope at ``xi``.
    ``params``: the outer kernel's ``[sigma_f, l, x_1 .., y_1 ..]``; ``sigma_n``: the nested kernel's fixed amplitude.  ``m12`` shows
    that the nested amplitude cancels; in ``m5wide`` the length scale goes negative between the points (the NaN classes).
  * ``fit__{X, n, y, Xs, ns}`` and ``fit__{K, ll, alpha, mean, cov, std}``: case ``m5`` at N = 60 sorted points (the last 12 with
    order 1), M = 30 test points (the last 6 slopes), ``err_y = 0.05``.
  * ``m2d__{X, n, y, Xi, Xj, ni, nj}`` and ``m2d__{k, ll}``: ``Masked(GibbsKernel1dGP m5, [0]) * Masked(SE [1.0, 0.8], [1])`` on
    60 points in 2-D with a few orders in each coordinate (two rows ``n = [0, 2]``): a 300-row pair list and the fit's ``ll``.

What makes the project's pair bound (rtol 1e-12 plus 1e-13 of the scale) fair for the reference alone is asserted here: every case's
nested ``K_tot`` has a condition number below 1e3, and at every row inside [0, 2] the cancellation ``sum_j |c_j e_j| / |l|`` of the
nested mean is at most 200.  Rows outside the hull are compared with the absolute part of a tolerance only (``inside``).
``nested_se`` / ``gp_kernel`` / ``make_fit_gp`` / ``make_2d_kernel`` build the models from either package.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

SIGMA_F = 1.2
M_PAIRS = 300
OUTSIDE = [-0.4, 2.3, -1.0, 3.5]
Y5 = [0.5, 0.7, 0.4, 0.9, 0.6]
# case: (x, l, y, sigma_n)
CASES = {
    "m2": ([0.3, 1.6], 0.8, [0.4, 0.9], 1.0),
    "m5": (list(np.linspace(0.0, 2.0, 5)), 0.45, Y5, 1.0),
    "m12": (list(np.linspace(0.0, 2.0, 12)), 0.16, list(np.random.RandomState(20).uniform(0.3, 1.0, 12)), 2.5),
    "m5wide": (list(np.linspace(0.0, 2.0, 5)), 0.75, Y5, 1.0),
}
FIT_CASE = "m5"
N_FIT, N_FIT_DERIV, M_FIT, M_FIT_DERIV, ERR_Y = 60, 12, 30, 6, 0.05
SE2_P = [1.0, 0.8]
COND_MAX, CANCEL_MAX = 1e3, 200.0


def case_params(case):
    x, l, y, _ = CASES[case]
    return [SIGMA_F, l] + list(x) + list(y)


def nested_se(g, sigma_n=1.0, l=0.45):
    """The nested kernel: SE ``[sigma_n, l]``, ``sigma_n`` fixed, ``l`` free."""
    return g.SquaredExponentialKernel(initial_params=[sigma_n, l], fixed_params=[True, False], param_bounds=[(0.0, 10.0)] * 2)


def gp_kernel(g, case, bounds=(-10.0, 10.0)):
    x, l, y, sigma_n = CASES[case]
    p = case_params(case)
    return g.GibbsKernel1dGP(len(x), k=nested_se(g, sigma_n, l), initial_params=p, param_bounds=[bounds] * len(p))


def inside(x):
    """Rows whose point lies in the hull [0, 2] of every case's data range: compared relatively; the rest absolutely."""
    x = np.asarray(x, dtype=float)
    return (x >= 0.0) & (x <= 2.0)


def pair_data(case):
    rs = np.random.RandomState(2000 + sorted(CASES).index(case))
    xg = np.asarray(CASES[case][0], dtype=float)
    M = M_PAIRS
    xi, xj = rs.uniform(0.0, 2.0, M), rs.uniform(0.0, 2.0, M)
    xj[:10] = xi[:10]                                # coincident points
    xi[10:10 + len(xg)] = xg                         # rows at the x_j themselves
    xi[M - 4:] = OUTSIDE                             # outside the hull
    ni, nj = rs.randint(0, 2, M), rs.randint(0, 2, M)
    return xi, xj, ni, nj


def fit_data():
    rs = np.random.RandomState(2010)
    X = np.sort(rs.uniform(0.0, 2.0, N_FIT))
    n = np.zeros(N_FIT, dtype=int)
    n[N_FIT - N_FIT_DERIV:] = 1
    y = np.where(n == 0, np.sin(3.0 * X), 3.0 * np.cos(3.0 * X)) + ERR_Y * rs.randn(N_FIT)
    Xs = np.sort(rs.uniform(0.0, 2.0, M_FIT))
    ns = np.zeros(M_FIT, dtype=int)
    ns[M_FIT - M_FIT_DERIV:] = 1
    return dict(X=X, n=n, y=y, Xs=Xs, ns=ns)


def make_fit_gp(g, d):
    gp = g.GaussianProcess(gp_kernel(g, FIT_CASE))
    gp.add_data(d["X"], d["y"], err_y=ERR_Y, n=d["n"])
    return gp


def make_2d_kernel(g):
    se = g.SquaredExponentialKernel(num_dim=1, initial_params=SE2_P, param_bounds=[(1e-3, 10.0)] * 2)
    return g.MaskedKernel(gp_kernel(g, FIT_CASE), total_dim=2, mask=[0]) * g.MaskedKernel(se, total_dim=2, mask=[1])


def m2d_data():
    rs = np.random.RandomState(2020)
    N = 60
    X = rs.uniform(0.0, 2.0, (N, 2))
    n = np.zeros((N, 2), dtype=int)
    n[40:48, 0] = 1
    n[48:56, 1] = 1
    n[56:58] = [1, 1]
    n[58:60] = [0, 2]
    y = np.sin(2.0 * X[:, 0]) * np.cos(X[:, 1]) + 0.05 * rs.randn(N)
    M = M_PAIRS
    a, b = rs.randint(0, N, M), rs.randint(0, N, M)
    b[:10] = a[:10]
    return dict(X=X, n=n, y=y, Xi=X[a], Xj=X[b], ni=n[a], nj=n[b])


def nested_numbers(case):
    """Condition number of the nested ``K_tot`` and the weights ``c`` of the closed form (numpy, for the assertions only)."""
    x, l, y, sigma_n = CASES[case]
    x = np.asarray(x, dtype=float)
    E = np.exp(-(x[:, None] - x[None, :]) ** 2 / (2.0 * l ** 2))
    K_tot = sigma_n ** 2 * E + 1e2 * np.finfo(float).eps * np.eye(len(x))
    return np.linalg.cond(K_tot), sigma_n ** 2 * np.linalg.solve(K_tot, np.asarray(y, dtype=float))


def main():
    import builtins
    sys.path.insert(0, HERE)
    from ref_harness import import_reference
    g = import_reference()
    import gptools.kernel.core as core
    core.range = lambda *a: list(builtins.range(*a))
    out = {}
    for case in sorted(CASES):
        xg, l, y, sigma_n = CASES[case]
        xi, xj, ni, nj = pair_data(case)
        k = gp_kernel(g, case)
        p = case_params(case)
        with np.errstate(all="ignore"):
            val = np.asarray(k(xi[:, None], xj[:, None], ni[:, None], nj[:, None]), dtype=float)
            lv = np.asarray(k.l_func(xi, 0, *p[1:]), dtype=float).ravel()
            dlv = np.asarray(k.l_func(xi, 1, *p[1:]), dtype=float).ravel()
        cond, c = nested_numbers(case)
        e = np.exp(-(xi[:, None] - np.asarray(xg)[None, :]) ** 2 / (2.0 * l ** 2))
        ins = inside(xi)
        cancel = (np.abs(c[None, :] * e).sum(axis=1) / np.abs(lv))[ins].max()
        print(case, "cond", cond, "cancellation", cancel, "min l", lv[ins].min(), "nan", int(np.isnan(val).sum()))
        assert cond < COND_MAX, (case, cond)
        assert cancel <= CANCEL_MAX, (case, cancel)
        for key, v in dict(xi=xi, xj=xj, ni=ni, nj=nj, params=np.asarray(p, dtype=float), sigma_n=np.float64(sigma_n), k=val,
                           l=lv, dl=dlv).items():
            out["pairs_%s__%s" % (case, key)] = np.asarray(v)
    d = fit_data()
    for key, v in d.items():
        out["fit__" + key] = v
    gp = make_fit_gp(g, d)
    gp.compute_K_L_alpha_ll()
    out["fit__K"], out["fit__ll"], out["fit__alpha"] = np.asarray(gp.K), np.float64(gp.ll), np.asarray(gp.alpha).ravel()
    mean, cov = gp.predict(d["Xs"], n=d["ns"], return_cov=True, return_std=False)
    out["fit__mean"], out["fit__cov"] = np.asarray(mean).ravel(), np.asarray(cov)
    out["fit__std"] = np.asarray(gp.predict(d["Xs"], n=d["ns"])[1]).ravel()
    print("fit ll", out["fit__ll"])
    d2 = m2d_data()
    for key, v in d2.items():
        out["m2d__" + key] = v
    k2 = make_2d_kernel(g)
    out["m2d__k"] = np.asarray(k2(d2["Xi"], d2["Xj"], d2["ni"], d2["nj"]), dtype=float)
    gp2 = g.GaussianProcess(k2)
    gp2.add_data(d2["X"], d2["y"], err_y=0.05, n=d2["n"])
    gp2.compute_K_L_alpha_ll()
    out["m2d__ll"] = np.float64(gp2.ll)
    print("2-D ll", out["m2d__ll"])
    path = os.path.join(HERE, "g20_gibbs_gp.npz")
    np.savez_compressed(path, **out)
    print("bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
