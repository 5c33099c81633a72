#!/usr/bin/env python
"""g17_gibbs_more.npz: the Gibbs kernels with the cubic / quintic bucket and the exponential-of-Gaussians length scales, from the
imported reference (ref: kernel/gibbs.py:603-902, gaussian_process.py:1989-2065).  Seeded; needs the reference tree
(``ref_harness``).

The bucket kernels are the reference's own ``GibbsKernel1dCubicBucket`` / ``GibbsKernel1dQuinticBucket``.  The reference's
``exp_gauss_warp`` cannot run under Python 3 (it slices with ``len(msb) / 3``, a float, and raises ``TypeError``), and with it
``GibbsKernel1dExpGauss``.  For that kernel the generator therefore builds the reference's ``GibbsKernel1d(l_func, num_params=
3 G + 2)`` -- the reference's own Mathematica derivative classes -- around ``ref_exp_gauss`` below, which is written here from the
formula and the loop the reference documents (gibbs.py:804-855) with the thirds of ``msb`` split by integer division.

Layout:
  * ``pairs_<case>__{xi, xj, ni, nj, params, k}``: 400 pairs per case over all four derivative classes, with coincident points
    and, for the buckets, points exactly at the four section ends (``bucket_ends``).  Buckets (``c_*`` cubic, ``q_*`` quintic):
    a base case, another sigma_f, a negative length scale in one region (mixed-sign pairs are NaN), w_1 = 0 (NaN everywhere), a
    negative width (overlapping masks), a width so small that the quintic's fifth power overflows outside the section (NaN there;
    the cubic stays finite).  Exp-Gauss (``e_*``): G = 1, 2 and the device cap 8, a negative beta, a sigma so small that every
    Gaussian underflows at most points.
  * ``kij_<case>__*``: compute_Kij, symmetric and rectangular, mixed orders, one case per kernel.
  * ``terms__*`` / ``terms_<case>__*``: each kernel alone, + SE, x SE, with a DiagonalNoiseKernel, and one case with T: ll, alpha,
    predict at n = 0 / 1.
  * ``lmcmc__*``: compute_l_from_MCMC of the cubic bucket on a 12-row trace at n = 0 and n = 1.
``gibbs`` / ``make_terms_gp`` build the models from either package.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

MAX_GAUSS = 8      # the device kernel's cap (GPT_GIBBS_MAX_GAUSS)
BASE = [1.3, 1.0, 0.3, 0.7, 1.0, 0.2, 0.4, 0.3]
_rs8 = np.random.RandomState(1708)
E_G8 = ([0.9, 0.5] + list(np.linspace(0.1, 1.9, 8)) + list(_rs8.uniform(0.1, 0.4, 8)) + list(_rs8.uniform(-0.8, 0.8, 8)))
PAIR_CASES = {}
for _k, _kind in (("c", "cubic"), ("q", "quintic")):
    PAIR_CASES[_k + "_base"] = (_kind, BASE)
    PAIR_CASES[_k + "_sig"] = (_kind, [2.5, 0.6, 1.1, 0.4, 0.9, 0.3, 0.2, 0.5])
    PAIR_CASES[_k + "_neg"] = (_kind, [1.0, 1.0, -0.3, 0.7, 1.0, 0.2, 0.4, 0.3])
    PAIR_CASES[_k + "_w10"] = (_kind, [1.0, 1.0, 0.3, 0.7, 1.0, 0.0, 0.4, 0.3])
    PAIR_CASES[_k + "_wneg"] = (_kind, [1.0, 1.0, 0.3, 0.7, 1.0, 0.2, 0.4, -0.3])
    PAIR_CASES[_k + "_tiny"] = (_kind, [1.0, 1.0, 0.3, 0.7, 1.0, 1e-65, 0.4, 0.3])
PAIR_CASES["e_g1"] = ("expgauss", [1.3, 0.5, 1.0, 0.3, 0.8])
PAIR_CASES["e_g2"] = ("expgauss", [1.0, 0.4, 0.6, 1.4, 0.2, 0.3, 0.9, -0.7])
PAIR_CASES["e_g8"] = ("expgauss", E_G8)
PAIR_CASES["e_negb"] = ("expgauss", [1.1, 0.6, 1.0, 0.25, -1.2])
PAIR_CASES["e_under"] = ("expgauss", [1.0, 0.5, 0.7, 1.2, 1e-3, 2e-3, 0.8, -0.6])
KIJ_CASES = ("c_base", "q_base", "e_g2")
KINDS = ("cubic", "quintic", "expgauss")
TERM_CASES = tuple("%s_%s" % (k, m) for k in KINDS for m in ("alone", "sum_se", "prod_se", "noise")) + ("cubic_T",)
TERM_PARAMS = {"cubic": [1.1, 0.8, 0.3, 0.6, 1.0, 0.3, 0.5, 0.3], "quintic": [1.1, 0.8, 0.3, 0.6, 1.0, 0.3, 0.5, 0.3],
               "expgauss": [1.1, 0.8, 0.7, 1.3, 0.2, 0.3, -0.8, -0.5]}
M_PAIRS = 400


def ref_exp_gauss(X, n, l0, *msb):
    """l = l_0 exp(sum_i beta_i exp(-(x - mu_i)^2 / (2 sigma_i^2))) and its slope, as gibbs.py:804-855 documents and loops."""
    X = np.asarray(X, dtype=float)
    msb = np.asarray(msb, dtype=float)
    G = len(msb) // 3
    mm, ss, bb = msb[:G], msb[G:2 * G], msb[2 * G:]
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


def is_reference(g):
    return g.__name__ == "gptools"


def gibbs(g, kind, params, bounds=(-10.0, 10.0), **kw):
    kw = dict(initial_params=list(params), param_bounds=[bounds] * len(params), **kw)
    if kind == "cubic":
        return g.GibbsKernel1dCubicBucket(**kw)
    if kind == "quintic":
        return g.GibbsKernel1dQuinticBucket(**kw)
    if is_reference(g):
        return g.GibbsKernel1d(ref_exp_gauss, num_params=len(params), **kw)
    return g.GibbsKernel1dExpGauss((len(params) - 2) // 3, **kw)


def bucket_ends(params):
    """The four section ends in the reference's order of operations (gibbs.py:627-639)."""
    x0, w1, w2, w3 = params[4:8]
    x1 = x0 - w2 / 2.0 - w1 / 2.0
    x2 = x0 + w2 / 2.0 + w3 / 2.0
    return np.array([x1 - w1 / 2.0, x1 + w1 / 2.0, x2 - w3 / 2.0, x2 + w3 / 2.0])


def pair_data(case):
    rs = np.random.RandomState(1700 + sorted(PAIR_CASES).index(case))
    kind, params = PAIR_CASES[case]
    M = M_PAIRS
    xi = rs.uniform(-0.2, 2.2, M)
    xj = rs.uniform(-0.2, 2.2, M)
    xj[:40] = xi[:40]                       # coincident points
    if kind != "expgauss":
        # the section ends as the reference computes them, and their decimal values (for BASE 0.6, 0.8, 1.2, 1.5; the
        # computed ones differ from some of those by an ulp, so a point at either lies exactly at or just beside an end)
        ends = bucket_ends(params)
        ends = np.concatenate((ends, np.round(ends, 10)))
        xi[40:64] = np.tile(ends, 3)        # at the section ends: against random points (40:56), ...
        xj[56:88] = np.repeat(ends, 4)      # ... against each other (56:64), random points against them (64:88)
    ni = rs.randint(0, 2, M)
    nj = rs.randint(0, 2, M)
    return xi, xj, ni, nj


def terms_data():
    rs = np.random.RandomState(1717)
    N = 40
    X = np.sort(rs.uniform(0.0, 2.0, N))
    n = np.zeros(N, dtype=int)
    n[-8:] = 1
    y = np.tanh(3.0 * (X - 1.0)) + 0.05 * rs.randn(N)
    y[n == 1] = 3.0 / np.cosh(3.0 * (X[n == 1] - 1.0)) ** 2
    T = rs.uniform(0.0, 1.0, (10, N)) / N
    yT = T.dot(np.tanh(3.0 * (X - 1.0))) + 0.01 * rs.randn(10)
    Xs = np.linspace(-0.1, 2.1, 30)
    return dict(X=X, n=n, y=y, T=T, yT=yT, Xs=Xs)


def make_terms_gp(g, case, d):
    kind = case.split("_")[0]
    mode = case[len(kind) + 1:]
    b = (-10.0, 10.0)
    k = gibbs(g, kind, TERM_PARAMS[kind], bounds=b)
    noise_k = None
    if mode == "noise":
        noise_k = g.DiagonalNoiseKernel(num_dim=1, initial_noise=0.1, noise_bound=(1e-4, 1.0))
    elif mode == "sum_se":
        k = k + g.SquaredExponentialKernel(num_dim=1, initial_params=[0.5, 0.7], param_bounds=[(1e-3, 10.0)] * 2)
    elif mode == "prod_se":
        k = k * g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 1.5], param_bounds=[(1e-3, 10.0)] * 2)
    gp = g.GaussianProcess(k, noise_k=noise_k)
    if mode == "T":
        gp.add_data(d["X"], d["yT"], err_y=0.01, T=d["T"])
    else:
        gp.add_data(d["X"], d["y"], err_y=0.05, n=d["n"])
    return gp


def lmcmc_trace():
    rs = np.random.RandomState(1720)
    lo = np.array([1.0, 0.6, 0.2, 0.4, 0.9, 0.1, 0.3, 0.1])
    hi = np.array([2.0, 1.2, 0.5, 0.9, 1.1, 0.4, 0.6, 0.4])
    return rs.uniform(lo, hi, (12, 8)), np.linspace(0.0, 2.0, 50)


def main():
    sys.path.insert(0, HERE)
    from ref_harness import import_reference
    g = import_reference()
    out = {}
    # --- pair lists
    for case, (kind, params) in sorted(PAIR_CASES.items()):
        xi, xj, ni, nj = pair_data(case)
        k = gibbs(g, kind, params)
        with np.errstate(all="ignore"):
            val = k(xi[:, None], xj[:, None], ni[:, None], nj[:, None])
        for key, v in dict(xi=xi, xj=xj, ni=ni, nj=nj, params=np.asarray(params, dtype=float), k=val).items():
            out["pairs_%s__%s" % (case, key)] = np.asarray(v)
        print(case, "nan", int(np.isnan(val).sum()), "inf", int(np.isinf(val).sum()), "max", np.nanmax(np.abs(val)) if
              np.isfinite(val).any() else None)
    # --- compute_Kij
    rs = np.random.RandomState(1701)
    for case in KIJ_CASES:
        kind, params = PAIR_CASES[case]
        gp = g.GaussianProcess(gibbs(g, kind, params))
        X = np.sort(rs.uniform(0.0, 2.0, 40))
        n = (rs.rand(40) < 0.3).astype(int)
        Xj = rs.uniform(0.0, 2.0, 25)
        nj = (rs.rand(25) < 0.5).astype(int)
        out["kij_%s__X" % case], out["kij_%s__n" % case] = X, n
        out["kij_%s__Xj" % case], out["kij_%s__nj" % case] = Xj, nj
        out["kij_%s__sym" % case] = np.asarray(gp.compute_Kij(X[:, None], None, n[:, None], None))
        out["kij_%s__rect" % case] = np.asarray(gp.compute_Kij(X[:30, None], Xj[:, None], n[:30, None], nj[:, None]))
    # --- each kernel alone, in a sum, in a product, with a noise kernel; T
    td = terms_data()
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
    # --- compute_l_from_MCMC
    gp = make_terms_gp(g, "cubic_alone", td)
    trace, Xl = lmcmc_trace()
    out["lmcmc__trace"], out["lmcmc__X"] = trace, Xl
    out["lmcmc__l0"] = np.asarray(list(gp.compute_l_from_MCMC(Xl, n=0, flat_trace=trace, num_proc=0)), dtype=float)
    out["lmcmc__l1"] = np.asarray(list(gp.compute_l_from_MCMC(Xl, n=1, flat_trace=trace, num_proc=0)), dtype=float)
    np.savez_compressed(os.path.join(HERE, "g17_gibbs_more.npz"), **out)


if __name__ == "__main__":
    main()
