#!/usr/bin/env python
"""g15_gibbs.npz: the Gibbs kernels with tanh length-scale warps, from the imported reference (ref: kernel/gibbs.py:229-590,
gaussian_process.py:1989-2065, demo/demo.py:370-406).  Seeded; needs the reference tree (``ref_harness``).

Layout:
  * ``pairs_<case>__{xi, xj, ni, nj, params, k}``: pair lists of GibbsKernel1dTanh (``t_*``) / GibbsKernel1dDoubleTanh (``d_*``)
    over all four derivative classes, with coincident points, points exactly at the transition, both length scales
    negative, mixed signs (NaN), a transition so sharp that cosh overflows, l_w = 0 (NaN derivative classes), sigma_f != 1.
  * ``kij_<case>__*``: compute_Kij, symmetric and rectangular, mixed orders.
  * ``demo__*``: the demo's Gibbs section -- core + edge data and a slope constraint at 0 -- at fixed parameters (ll, alpha, L,
    predict at n = 0 / 1 with covariances, draw_sample with explicit variates), the MAP from a fixed start, a
    compute_ll_matrix grid and seeded random starts (g12's scheme: the draws of the hyperprior under np.random.seed(4242)).
  * ``terms_<case>__*``: Gibbs + noise, Gibbs + SE, Gibbs x SE, the double-tanh kernel, a case with T: ll and predict.
  * ``lmcmc__*``: compute_l_from_MCMC on a 20-row trace at n = 0 and n = 1.
``make_demo_gp`` / ``make_terms_gp`` build the models from either package (their APIs are the same).
"""
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

PAIR_CASES = {
    "t_base": ("tanh", [1.3, 1.0, 0.5, 0.1, 1.0]),
    "t_neg": ("tanh", [1.0, -1.0, -0.5, 0.1, 1.0]),
    "t_mixed": ("tanh", [1.0, 1.0, -0.5, 0.3, 1.0]),
    "t_sharp": ("tanh", [0.8, 1.0, 0.5, 1e-3, 1.0]),
    "t_lw0": ("tanh", [1.0, 1.0, 0.5, 0.0, 1.0]),
    "d_base": ("dtanh", [1.2, 1.0, 0.5, 0.2, 0.1, 0.05, 0.6, 0.9]),
    "d_neg": ("dtanh", [1.0, -1.0, -0.5, -0.2, 0.1, 0.05, 0.6, 0.9]),
    "d_mixed": ("dtanh", [1.0, 1.0, -0.5, 0.3, 0.2, 0.1, 0.6, 0.9]),
    "d_sharp": ("dtanh", [1.0, 1.0, 0.5, 0.2, 1e-3, 1e-3, 0.6, 0.9]),
}
DEMO_PARAMS = [1.53, 1.13, 0.52, 0.0136, 1.005]
TERM_CASES = ("noise", "sum_se", "prod_se", "dtanh", "T")


def gibbs(g, warp, params, **kw):
    cls = g.GibbsKernel1dTanh if warp == "tanh" else g.GibbsKernel1dDoubleTanh
    return cls(initial_params=list(params), param_bounds=[(-10.0, 10.0)] * len(params), **kw)


def pair_data(case):
    rs = np.random.RandomState(1500 + sorted(PAIR_CASES).index(case))
    warp, params = PAIR_CASES[case]
    x0 = params[4] if warp == "tanh" else params[6]
    M = 240
    xi = rs.uniform(x0 - 1.5, x0 + 1.5, M)
    xj = rs.uniform(x0 - 1.5, x0 + 1.5, M)
    xj[:30] = xi[:30]                       # coincident points
    xi[30:45] = x0                          # exactly at the transition
    xj[40:55] = x0
    ni = rs.randint(0, 2, M)
    nj = rs.randint(0, 2, M)
    return xi, xj, ni, nj


def load_demo_data():
    from ref_harness import REF_ROOT
    out = {}
    for nm in ("core", "edge"):
        with open(os.path.join(REF_ROOT, "demo", "sample_data_%s.pkl" % nm), "rb") as f:
            dat = pickle.load(f, encoding="latin1")
        for kk in ("X", "y", "err_y"):
            out["%s_%s" % (nm, kk)] = np.asarray(dat[kk], dtype=float)
    return out


def make_demo_gp(g, d, fixed=None):
    """demo/demo.py:381-391 (the hyperprior as there)."""
    hp = g.UniformJointPrior([[0.0, 20.0]]) * g.GammaJointPriorAlt([1.0, 0.5, 0.0, 1.0], [0.3, 0.25, 0.1, 0.1])
    kw = {} if fixed is None else dict(fixed_params=fixed, initial_params=DEMO_PARAMS)
    gp = g.GaussianProcess(g.GibbsKernel1dTanh(hyperprior=hp, **kw))
    gp.add_data(d["core_X"], d["core_y"], err_y=d["core_err_y"])
    gp.add_data(d["edge_X"], d["edge_y"], err_y=d["edge_err_y"])
    gp.add_data(0, 0, n=1)
    return gp


def terms_data():
    rs = np.random.RandomState(1515)
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
    b = [(1e-3, 10.0)]
    kt = g.GibbsKernel1dTanh(initial_params=[1.1, 0.8, 0.3, 0.2, 1.0], param_bounds=b * 5)
    noise_k = None
    if case == "noise":
        k = kt
        noise_k = g.DiagonalNoiseKernel(num_dim=1, initial_noise=0.1, noise_bound=(1e-4, 1.0))
    elif case == "sum_se":
        k = kt + g.SquaredExponentialKernel(num_dim=1, initial_params=[0.5, 0.7], param_bounds=b * 2)
    elif case == "prod_se":
        k = kt * g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 1.5], param_bounds=b * 2)
    elif case == "dtanh":
        k = g.GibbsKernel1dDoubleTanh(initial_params=[1.1, 0.8, 0.5, 0.2, 0.2, 0.1, 0.7, 1.3], param_bounds=b * 8)
    else:
        k = kt
    gp = g.GaussianProcess(k, noise_k=noise_k)
    if case == "T":
        gp.add_data(d["X"], d["yT"], err_y=0.01, T=d["T"])
    else:
        gp.add_data(d["X"], d["y"], err_y=0.05, n=d["n"])
    return gp


def main():
    sys.path.insert(0, HERE)
    from ref_harness import import_reference
    g = import_reference()
    out = {}
    # --- pair lists
    for case, (warp, params) in sorted(PAIR_CASES.items()):
        xi, xj, ni, nj = pair_data(case)
        k = gibbs(g, warp, params)
        val = k(xi[:, None], xj[:, None], ni[:, None], nj[:, None])
        for key, v in dict(xi=xi, xj=xj, ni=ni, nj=nj, params=np.asarray(params), k=val).items():
            out["pairs_%s__%s" % (case, key)] = np.asarray(v)
        print(case, "nan", int(np.isnan(val).sum()), "inf", int(np.isinf(val).sum()))
    # --- compute_Kij
    rs = np.random.RandomState(1501)
    for case in ("t_base", "d_base", "t_neg"):
        warp, params = PAIR_CASES[case]
        gp = g.GaussianProcess(gibbs(g, warp, params))
        X = np.sort(rs.uniform(0.0, 2.0, 40))
        n = (rs.rand(40) < 0.3).astype(int)
        Xj = rs.uniform(0.0, 2.0, 25)
        nj = (rs.rand(25) < 0.5).astype(int)
        out["kij_%s__X" % case], out["kij_%s__n" % case] = X, n
        out["kij_%s__Xj" % case], out["kij_%s__nj" % case] = Xj, nj
        out["kij_%s__sym" % case] = np.asarray(gp.compute_Kij(X[:, None], None, n[:, None], None))
        out["kij_%s__rect" % case] = np.asarray(gp.compute_Kij(X[:30, None], Xj[:, None], n[:30, None], nj[:, None]))
    # --- the demo's Gibbs section
    d = load_demo_data()
    for key, v in d.items():
        out["demo__" + key] = v
    gp = make_demo_gp(g, d)
    p = np.asarray(DEMO_PARAMS)
    out["demo__params"] = p
    out["demo__negll"] = np.float64(gp.update_hyperparameters(p))
    out["demo__ll"] = np.float64(gp.ll)
    out["demo__alpha"] = np.asarray(gp.alpha).ravel()
    out["demo__L"] = np.asarray(gp.L)
    Xs = np.linspace(0.0, 1.2, 200)
    out["demo__Xs"] = Xs
    out["demo__mean0"], out["demo__std0"] = gp.predict(Xs)
    out["demo__mean1"], out["demo__std1"] = gp.predict(Xs, n=1)
    Xc = np.linspace(0.0, 1.2, 48)
    out["demo__Xc"] = Xc
    for nn in (0, 1):
        m, c = gp.predict(Xc, n=nn, return_std=False, return_cov=True)
        out["demo__cmean%d" % nn], out["demo__cov%d" % nn] = m, c
    # samples at a few points whose predictive covariance is well conditioned (on the 48-point grid above it is singular to
    # working precision: a 1e-10 relative change of the covariance moves a sample by percents there, or breaks the Cholesky)
    Xd = np.array([0.0, 0.6, 0.95, 1.02, 1.1, 1.2])
    u = rs.randn(len(Xd), 3)
    out["demo__Xd"], out["demo__u"] = Xd, u
    out["demo__samp0"] = np.asarray(gp.draw_sample(Xd, rand_vars=u))
    out["demo__samp1"] = np.asarray(gp.draw_sample(Xd, n=1, rand_vars=u))
    # MAP from a fixed start (no random starts)
    gp = make_demo_gp(g, d)
    gp.update_hyperparameters(np.array([1.0, 1.0, 0.5, 0.05, 1.0]))
    res, _ = gp.optimize_hyperparameters(method="SLSQP", random_starts=0, num_proc=0)
    out["demo__map_x"], out["demo__map_fun"] = np.asarray(res.x, dtype=float), np.float64(res.fun)
    # compute_ll_matrix over l_1, l_2 (the others fixed)
    gp = make_demo_gp(g, d, fixed=[True, False, False, True, True])
    ll, pv = gp.compute_ll_matrix([(0.8, 1.6), (0.3, 0.8)], [4, 3])
    out["demo__grid_ll"] = np.asarray(ll, dtype=float)
    out["demo__grid_p0"], out["demo__grid_p1"] = np.asarray(pv[0]), np.asarray(pv[1])
    # seeded random starts (g12's scheme)
    gp = make_demo_gp(g, d)
    gp.update_hyperparameters(np.array([1.0, 1.0, 0.5, 0.05, 1.0]))
    np.random.seed(4242)
    out["demo__rs_draws"] = np.asarray(gp.hyperprior.random_draw(size=3).T, dtype=float)
    np.random.seed(4242)
    res, count = gp.optimize_hyperparameters(method="SLSQP", random_starts=3, num_proc=0)
    out["demo__rs_x"], out["demo__rs_fun"] = np.asarray(res.x, dtype=float), np.float64(res.fun)
    out["demo__rs_count"] = np.int64(count)
    print("demo", out["demo__ll"], out["demo__map_x"], out["demo__rs_x"], count)
    # --- sums, products, the double-tanh warp, T
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
    gp = make_demo_gp(g, d)
    rsl = np.random.RandomState(1520)
    trace = np.column_stack([rsl.uniform(1.0, 2.0, 20), rsl.uniform(0.8, 1.4, 20), rsl.uniform(0.3, 0.7, 20),
                             rsl.uniform(0.005, 0.05, 20), rsl.uniform(0.95, 1.05, 20)])
    Xl = np.linspace(0.0, 1.2, 50)
    out["lmcmc__trace"], out["lmcmc__X"] = trace, Xl
    out["lmcmc__l0"] = np.asarray(list(gp.compute_l_from_MCMC(Xl, n=0, flat_trace=trace, num_proc=0)), dtype=float)
    out["lmcmc__l1"] = np.asarray(list(gp.compute_l_from_MCMC(Xl, n=1, flat_trace=trace, num_proc=0)), dtype=float)
    out["lmcmc__l0_bt"] = np.asarray(list(gp.compute_l_from_MCMC(Xl, n=0, flat_trace=trace, burn=2, thin=3, num_proc=0)),
                                     dtype=float)
    np.savez_compressed(os.path.join(HERE, "g15_gibbs.npz"), **out)


if __name__ == "__main__":
    main()
