#!/usr/bin/env python
"""g16_warp.npz: input-warped kernels (beta-CDF and linear warps), from the imported reference (ref: kernel/warping.py:315-716,
gaussian_process.py:2067-2142).  Seeded; needs the reference tree (``ref_harness``).  The reference's warping.py still says
``long``: ``builtins.long = int`` is set before the import.

Layout (``<inner>`` in INNERS, ``<warp>`` in WARPS, ``<D>`` in 1, 2, 3):
  * ``pairs_<inner>_<warp>_d<D>__{xi, xj, ni, nj, k}``: pair lists; orders 0 / 1 on either side, a point's derivative in one
    dimension (squared-exponential cases: in any set of dimensions); alpha, beta on both sides of 1.
  * ``edge_d<D>__{xi, xj, k}``: beta warp around SE at x = 0, x = 1 and outside [0, 1] (NaN), values only.
  * ``wfun_<warp>_d<D>__{x, w, w1}``: the whole warp of dimension 0 and its slope (``w_func``; the slope recorded for single
    layers only: the reference evaluates a nested inner slope at the wrong point).
  * ``fit_<case>_d<D>__*`` (FIT_CASES): Gram matrix, ll, alpha, predictive mean / std / cov at n = 0 and with derivative
    predictions, with value and derivative observations; a DiagonalNoiseKernel case and a case with T.
  * ``grid__*``: compute_ll_matrix over (alpha_0, beta_0); ``wmcmc__*``: compute_w_from_MCMC on a short trace.
``make_kernel`` / ``make_fit_gp`` build the models from either package (their APIs are the same); ``inner`` may be replaced
by a factory of stand-in kernels (the CPU tests use the oracle).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

INNERS = ("se", "m52", "rq", "sum", "prod")
WARPS = ("beta", "lin", "lin_beta", "beta_lin")          # "lin_beta": the linear layer outside (applied first), beta inside
DIMS = (1, 2, 3)
FIT_CASES = ("se_lin_beta", "m52_beta", "sum_lin_beta", "prod_beta", "noise", "T")
LIN_A, LIN_B = [-1.0, 2.0, 0.5], [3.0, 2.5, 10.0]         # per dimension
BETA_P = [0.4, 2.2, 3.0, 0.7, 1.6, 1.3]                   # alpha_0, beta_0, alpha_1, ...
B = (1e-3, 1e3)


def native(g, name, D):
    """One of the package's kernels with fixed, case-independent parameters."""
    ls = [0.35, 0.5, 0.8][:D]
    if name == "se":
        return g.SquaredExponentialKernel(num_dim=D, initial_params=[1.3] + ls, param_bounds=[B] * (D + 1))
    if name == "m52":
        return g.Matern52Kernel(num_dim=D, initial_params=[0.9] + ls, param_bounds=[B] * (D + 1))
    if name == "rq":
        return g.RationalQuadraticKernel(num_dim=D, initial_params=[1.1, 1.7] + ls, param_bounds=[B] * (D + 2))
    raise ValueError(name)


def inner_kernel(g, inner, D, factory=native):
    if inner == "sum":
        return factory(g, "se", D) + factory(g, "m52", D)
    if inner == "prod":
        return factory(g, "se", D) * factory(g, "rq", D)
    return factory(g, inner, D)


def make_kernel(g, inner, warp, D, factory=native, beta=None):
    k = inner_kernel(g, inner, D, factory)
    bp = list(BETA_P[:2 * D] if beta is None else beta)
    bb = [(1e-3, 1e2)] * (2 * D)
    if warp == "beta":
        return g.BetaWarpedKernel(k, initial_params=bp, param_bounds=bb)
    if warp == "lin":
        return g.LinearWarpedKernel(k, LIN_A[:D], LIN_B[:D])
    if warp == "lin_beta":
        return g.LinearWarpedKernel(g.BetaWarpedKernel(k, initial_params=bp, param_bounds=bb), LIN_A[:D], LIN_B[:D])
    if warp == "beta_lin":
        return g.BetaWarpedKernel(g.LinearWarpedKernel(k, LIN_A[:D], LIN_B[:D]), initial_params=bp, param_bounds=bb)
    raise ValueError(warp)


def raw_points(rs, warp, M, D):
    """Points whose coordinates lie in [0.02, 0.98] where they enter a beta layer."""
    u = rs.uniform(0.02, 0.98, (M, D))
    if warp in ("lin", "lin_beta"):
        return np.asarray(LIN_A[:D]) + u * (np.asarray(LIN_B[:D]) - np.asarray(LIN_A[:D]))
    return u


def orders(rs, M, D, multi):
    n = np.zeros((M, D), dtype=int)
    if multi:
        return (rs.rand(M, D) < 0.4).astype(int)
    hit = rs.rand(M) < 0.6
    n[np.flatnonzero(hit), rs.randint(0, D, int(hit.sum()))] = 1
    return n


def pair_data(inner, warp, D):
    rs = np.random.RandomState(1600 + 100 * INNERS.index(inner) + 10 * WARPS.index(warp) + D)
    M = 36
    xi, xj = raw_points(rs, warp, M, D), raw_points(rs, warp, M, D)
    xj[:4] = xi[:4]
    return xi, xj, orders(rs, M, D, inner == "se"), orders(rs, M, D, inner == "se")


def fit_data(D):
    rs = np.random.RandomState(1650 + D)
    N = 48
    U = rs.uniform(0.02, 0.98, (N, D))
    n = np.zeros((N, D), dtype=int)
    for r, d in zip(range(N - 10, N), rs.randint(0, D, 10)):
        n[r, d] = 1
    f = np.sin(4.0 * U.sum(axis=1))
    y = f + 0.05 * rs.randn(N)
    y[-10:] = 4.0 * np.cos(4.0 * U[-10:].sum(axis=1))
    T = rs.uniform(0.0, 1.0, (12, N)) / N
    yT = T.dot(f) + 0.01 * rs.randn(12)
    Us = rs.uniform(0.02, 0.98, (14, D))
    ns = np.zeros((14, D), dtype=int)
    for r, d in zip(range(8, 14), rs.randint(0, D, 6)):
        ns[r, d] = 1
    return dict(U=U, n=n, y=y, T=T, yT=yT, Us=Us, ns=ns)


def fit_points(case, d, D):
    """The unit-cube points of ``fit_data`` in the coordinates the case's outermost layer takes."""
    if "lin" in case or case == "T":
        a, b = np.asarray(LIN_A[:D]), np.asarray(LIN_B[:D])
        return a + d["U"] * (b - a), a + d["Us"] * (b - a)
    return d["U"], d["Us"]


def make_fit_gp(g, case, D, d, factory=native, beta=None, fixed=None):
    noise_k = None
    if case == "noise":
        k = make_kernel(g, "se", "beta", D, factory, beta)
        noise_k = g.DiagonalNoiseKernel(num_dim=D, initial_noise=0.1, noise_bound=(1e-4, 1.0))
    elif case == "T":
        k = make_kernel(g, "se", "lin_beta", D, factory, beta)
    else:
        inner, warp = case.split("_", 1)
        k = make_kernel(g, inner, warp, D, factory, beta)
    if fixed is not None:
        k.fixed_params = fixed
    gp = g.GaussianProcess(k, noise_k=noise_k)
    X, _ = fit_points(case, d, D)
    if case == "T":
        gp.add_data(X, d["yT"], err_y=0.01, T=d["T"])
    else:
        gp.add_data(X, d["y"], err_y=0.05, n=d["n"])
    return gp


def main():
    import builtins
    builtins.long = int
    sys.path.insert(0, HERE)
    from ref_harness import import_reference
    g = import_reference()
    out = {}
    for D in DIMS:
        for inner in INNERS:
            for warp in WARPS:
                xi, xj, ni, nj = pair_data(inner, warp, D)
                k = make_kernel(g, inner, warp, D)
                val = np.asarray(k(xi, xj, ni, nj), dtype=float)
                assert np.isfinite(val).all(), (inner, warp, D)
                for key, v in dict(xi=xi, xj=xj, ni=ni.astype(np.int8), nj=nj.astype(np.int8), k=val).items():
                    out["pairs_%s_%s_d%d__%s" % (inner, warp, D, key)] = v
        # edges of the beta warp: values only
        rs = np.random.RandomState(1690 + D)
        xi = rs.uniform(0.0, 1.0, (12, D))
        xj = rs.uniform(0.0, 1.0, (12, D))
        xi[0:3, 0], xj[2:5, D - 1] = 0.0, 1.0
        xi[5, 0], xi[6, D - 1], xj[7, 0], xj[8, 0] = 1.0, 0.0, -0.25, 1.5
        xi[9, D - 1] = -1e-9
        z = np.zeros((12, D), dtype=int)
        val = np.asarray(make_kernel(g, "se", "beta", D)(xi, xj, z, z), dtype=float)
        assert np.isnan(val).sum() == 3, val
        out["edge_d%d__xi" % D], out["edge_d%d__xj" % D], out["edge_d%d__k" % D] = xi, xj, val
        # the warp functions alone
        for warp in WARPS:
            k = make_kernel(g, "se", warp, D)
            x = raw_points(np.random.RandomState(1695), warp, 25, D)[:, 0]
            out["wfun_%s_d%d__x" % (warp, D)] = x
            out["wfun_%s_d%d__w" % (warp, D)] = np.asarray(k.w_func(x, 0, 0), dtype=float)
            if warp in ("beta", "lin"):
                out["wfun_%s_d%d__w1" % (warp, D)] = np.asarray(k.w_func(x, 0, 1), dtype=float)
        # fits
        d = fit_data(D)
        for key, v in d.items():
            out["fit_d%d__%s" % (D, key)] = v
        for case in FIT_CASES:
            gp = make_fit_gp(g, case, D, d)
            gp.compute_K_L_alpha_ll()
            key = "fit_%s_d%d__" % (case, D)
            _, Xs = fit_points(case, d, D)
            out[key + "K"] = np.asarray(gp.K, dtype=float)
            out[key + "ll"] = np.float64(gp.ll)
            out[key + "alpha"] = np.asarray(gp.alpha, dtype=float).ravel()
            m, c = gp.predict(Xs, n=d["ns"], return_std=False, return_cov=True)
            out[key + "mean"], out[key + "cov"] = np.asarray(m, dtype=float), np.asarray(c, dtype=float)
            m0, s0 = gp.predict(Xs, n=0)
            out[key + "mean0"], out[key + "std0"] = np.asarray(m0, dtype=float), np.asarray(s0, dtype=float)
            if case == "noise":
                _, sn = gp.predict(Xs, n=0, noise=True)
                out[key + "std0_noise"] = np.asarray(sn, dtype=float)
            print(case, D, out[key + "ll"])
    # likelihood grid over (alpha_0, beta_0), everything else fixed
    D = 2
    d = fit_data(D)
    gp = make_fit_gp(g, "se_lin_beta", D, d)
    fixed = np.ones(len(gp.k.params), dtype=bool)
    fixed[D + 1], fixed[D + 2] = False, False
    gp = make_fit_gp(g, "se_lin_beta", D, d, fixed=fixed)
    ll, pv = gp.compute_ll_matrix([(0.5, 2.5), (0.6, 3.0)], [4, 3])
    out["grid__ll"] = np.asarray(ll, dtype=float)
    out["grid__p0"], out["grid__p1"] = np.asarray(pv[0]), np.asarray(pv[1])
    out["grid__fixed"] = fixed
    # compute_w_from_MCMC
    gp = make_fit_gp(g, "se_beta", 1, fit_data(1))
    rsw = np.random.RandomState(1699)
    trace = np.column_stack([rsw.uniform(0.5, 2.0, 12), rsw.uniform(0.2, 0.6, 12), rsw.uniform(0.4, 3.0, 12),
                             rsw.uniform(0.4, 3.0, 12)])
    Xw = np.linspace(0.02, 0.98, 20)
    out["wmcmc__trace"], out["wmcmc__X"] = trace, Xw
    out["wmcmc__w0"] = np.asarray(list(gp.compute_w_from_MCMC(Xw, n=0, flat_trace=trace, num_proc=0)), dtype=float)
    out["wmcmc__w1"] = np.asarray(list(gp.compute_w_from_MCMC(Xw, n=1, flat_trace=trace, num_proc=0)), dtype=float)
    out["wmcmc__w0_bt"] = np.asarray(list(gp.compute_w_from_MCMC(Xw, n=0, flat_trace=trace, burn=2, thin=3, num_proc=0)),
                                     dtype=float)
    np.savez_compressed(os.path.join(HERE, "g16_warp.npz"), **out)
    print("size", os.path.getsize(os.path.join(HERE, "g16_warp.npz")))


if __name__ == "__main__":
    main()
