#!/usr/bin/env python
"""g19_masked.npz: ``MaskedKernel`` (ref: kernel/core.py:1011-1149) from the imported reference -- pair lists and whole models.
Seeded; needs the reference tree (``ref_harness``).  Two shims for Python 3, set on the imported modules: the reference's constructor
removes entries from ``range(...)``, so ``gptools.kernel.core`` gets a list-returning ``range``; ``compute_from_MCMC`` walks the result
of ``map`` more than once, so ``gptools.gaussian_process`` gets a list-returning ``map`` (the calls run with ``num_proc=0``).  Nothing
of the reference is copied: only the inputs and its results are stored.

Layout:
  * ``pairs_<case>__{Xi, Xj, ni, nj, k}``: about 200 pairs per case (``PAIR_CASES``: base kernel, its parameters, total_dim, mask,
    scale).  Rows 0-39 are coincident points; rows 40-99 carry a derivative order in a dimension outside the mask (the reference
    answers exactly 0 there), a third of the coincident rows too; the rest have orders inside the mask or none.  Orders are <= 1
    per entry -- and at most one per point, over all dimensions -- where Matern52 or a Gibbs kernel is the base, <= 1 per entry for
    the general Matern kernel, up to 3 per entry for SE / RationalQuadratic (the sum over a pair capped at 5 for the latter: the
    reference walks every set partition); the Matern52 lists hold the ``(e_a, e_a)`` pairs for ``a`` inside and outside the mask,
    coincident and not.  ``se_scale_d2`` has a non-default ``scale``.  ``pairs_se_d3__k_hd<i>``: the same list with
    ``hyper_deriv = i`` for every parameter of the base.
  * ``model_<m>__{X, n, y, Xs, ns}`` and ``model_<m>__{ll, alpha, mean, std, K, Ks}`` for the models ``MODELS`` at N = 300 training and
    M = 70 test points (the last 40 training and the last 20 test rows carry first derivatives, split over the dimensions);
    ``K``: the last 60 rows and columns of the training covariance (20 value rows, 40 derivative rows), ``Ks``: the last 30 test
    rows against the same 60 training points.  ``model_b__{trace, mc_mean, mc_std, mc_cov}``: a 12-row trace of the free
    parameters and the reference's ``predict_MCMC`` over it.
  * No ``ll_deriv`` is stored for model (a): the reference's ``ProductKernel`` refuses ``hyper_deriv`` (core.py:618-619), so
    ``use_hyper_deriv`` fails there for every product.
``base_kernel`` / ``masked`` / ``make_model`` build the kernels from either package.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

N_TRAIN, N_DERIV, M_TEST, M_DERIV = 300, 40, 70, 20
CORNER, CORNER_S = 60, 30
M_PAIRS = 200
TANH_P = [1.1, 0.8, 0.3, 0.2, 1.0]
CUBIC_P = [1.0, 0.9, 0.3, 0.7, 1.0, 0.4, 0.5, 0.3]

# case: (base kind, base parameters, total_dim, mask, scale)
PAIR_CASES = {
    "se_d2": ("se", [1.2, 0.6], 2, [1], None),
    "se_d3": ("se", [0.9, 0.7, 1.1], 3, [0, 2], None),
    "se_scale_d2": ("se", [1.2, 0.6], 2, [0], [2.0, 0.5]),
    "m52_d2": ("m52", [1.0, 0.9], 2, [0], None),
    "m52_d3": ("m52", [1.3, 0.5], 3, [2], None),      # (1-D base: the reference's own Matern52 extension refuses the non-contiguous
                                                      #  order columns a wider mask slices out)
    "rq_d2": ("rq", [0.8, 1.5, 0.7], 2, [1], None),
    "rq_d3": ("rq", [1.1, 0.6, 0.9, 0.5], 3, [1, 2], None),
    "mat15_d2": ("matern", [1.0, 1.5, 0.8], 2, [0], None),
    "mat25_d3": ("matern", [1.2, 2.5, 0.6], 3, [1], None),
    "tanh_d2": ("tanh", TANH_P, 2, [1], None),
    "tanh_d3": ("tanh", TANH_P, 3, [2], None),
}
HD_CASE = "se_d3"
MODELS = ("a", "b", "c", "d", "e")
MODEL_DIM = {"a": 2, "b": 2, "c": 3, "d": 3, "e": 2}


def base_kernel(g, kind, params):
    params = list(params)
    kw = dict(initial_params=params, param_bounds=[(-10.0, 20.0) if kind in ("tanh", "cubic") else (1e-3, 20.0)] * len(params))
    if kind == "se":
        return g.SquaredExponentialKernel(num_dim=len(params) - 1, **kw)
    if kind == "m52":
        return g.Matern52Kernel(num_dim=len(params) - 1, **kw)
    if kind == "rq":
        return g.RationalQuadraticKernel(num_dim=len(params) - 2, **kw)
    if kind == "matern":
        return g.MaternKernel(num_dim=len(params) - 2, **kw)
    if kind == "tanh":
        return g.GibbsKernel1dTanh(**kw)
    if kind == "cubic":
        return g.GibbsKernel1dCubicBucket(**kw)
    raise ValueError(kind)


def masked(g, kind, params, total_dim, mask, scale=None):
    return g.MaskedKernel(base_kernel(g, kind, params), total_dim=total_dim, mask=list(mask), scale=scale)


def pair_kernel(g, case):
    return masked(g, *PAIR_CASES[case])


def make_kernel(g, m):
    if m == "a":
        return masked(g, "se", [1.2, 0.6], 2, [0]) * masked(g, "m52", [1.0, 0.9], 2, [1])
    if m == "b":
        return masked(g, "tanh", TANH_P, 2, [0]) * masked(g, "se", [1.0, 0.8], 2, [1])
    if m == "c":
        return masked(g, "se", [1.0, 0.7, 0.9], 3, [0, 2]) + masked(g, "rq", [0.6, 1.5, 0.8], 3, [1])
    if m == "d":
        return masked(g, "cubic", CUBIC_P, 3, [1]) * masked(g, "se", [1.0, 0.8, 1.1], 3, [0, 2])
    if m == "e":
        return masked(g, "se", [1.2, 0.6], 2, [0], scale=[2, 2]) * masked(g, "m52", [1.0, 0.9], 2, [1])
    raise ValueError(m)


def model_data(m):
    rs = np.random.RandomState(1900 + MODELS.index(m))
    D = MODEL_DIM[m]

    def points(count, nder):
        X = rs.uniform(0.0, 2.0, (count, D))
        n = np.zeros((count, D), dtype=int)
        for q in range(nder):
            n[count - nder + q, q % D] = 1
        return X, n
    X, n = points(N_TRAIN, N_DERIV)
    f = np.tanh(3.0 * (X[:, 0] - 1.0)) * np.cos(X[:, 1]) + (0.3 * X[:, 2] if D == 3 else 0.0)
    y = np.where(n.sum(axis=1) > 0, 0.5 * rs.randn(N_TRAIN), f) + 0.05 * rs.randn(N_TRAIN)
    Xs, ns = points(M_TEST, M_DERIV)
    return dict(X=X, n=n, y=y, Xs=Xs, ns=ns)


def make_model(g, m, d):
    gp = g.GaussianProcess(make_kernel(g, m))
    gp.add_data(d["X"], d["y"], err_y=0.05, n=d["n"])
    return gp


def model_trace(m="b"):
    rs = np.random.RandomState(1950)
    p0 = np.array(TANH_P + [1.0, 0.8])
    return p0 * rs.uniform(0.9, 1.1, (12, len(p0)))


def pair_data(case):
    kind, _, D, mask, _ = PAIR_CASES[case]
    rs = np.random.RandomState(1900 + 10 * sorted(PAIR_CASES).index(case) + 50)
    M = M_PAIRS
    out_dims = [d for d in range(D) if d not in mask]
    Xi, Xj = rs.uniform(0.0, 2.0, (M, D)), rs.uniform(0.0, 2.0, (M, D))
    Xj[:40] = Xi[:40]
    Xj[100:110, mask] = Xi[100:110][:, mask]              # coincident in the masked dimensions only
    one_per_point = kind in ("m52", "tanh")
    top = 3 if kind in ("se", "rq") else 1
    ni, nj = np.zeros((M, D), dtype=int), np.zeros((M, D), dtype=int)
    for r in range(M):
        outside = 40 <= r < 100 or (r < 40 and r % 3 == 0)
        for side in (ni, nj):
            if one_per_point:
                if rs.rand() < 0.5:
                    side[r, rs.choice(mask)] = 1
            else:
                side[r, mask] = rs.randint(0, top + 1, len(mask)) * (rs.rand(len(mask)) < 0.5)
        if outside:
            side = ni if rs.rand() < 0.5 else nj
            if one_per_point:
                side[r, :] = 0
            side[r, rs.choice(out_dims)] = rs.randint(1, top + 1)
        if kind in ("rq", "matern"):
            while ni[r].sum() + nj[r].sum() > 5:          # the reference walks every set partition of the pair's derivatives
                side = ni if ni[r].sum() >= nj[r].sum() else nj
                side[r, int(np.argmax(side[r]))] -= 1
    if kind == "m52":
        # the (e_a, e_a) class: a inside the mask (coincident and not), a outside it (likewise)
        for r, a in ((1, mask[0]), (2, out_dims[0]), (110, mask[0]), (111, out_dims[0]), (112, mask[-1]), (41, out_dims[-1])):
            ni[r], nj[r] = 0, 0
            ni[r, a] = nj[r, a] = 1
    return Xi, Xj, ni, nj


def main():
    import builtins
    sys.path.insert(0, HERE)
    from ref_harness import import_reference
    g = import_reference()
    import gptools.kernel.core as core
    import gptools.gaussian_process as gpmod
    core.range = lambda *a: list(builtins.range(*a))
    gpmod.map = lambda f, *a: list(builtins.map(f, *a))
    out = {}
    for case in sorted(PAIR_CASES):
        Xi, Xj, ni, nj = pair_data(case)
        k = pair_kernel(g, case)
        with np.errstate(all="ignore"):
            val = np.asarray(k(Xi, Xj, ni, nj), dtype=float)
        for key, v in dict(Xi=Xi, Xj=Xj, ni=ni, nj=nj, k=val).items():
            out["pairs_%s__%s" % (case, key)] = np.asarray(v)
        outside = (ni[:, k.maskC] != 0).any(axis=1) | (nj[:, k.maskC] != 0).any(axis=1)
        assert np.all(val[outside] == 0.0) and outside.sum() >= 60
        print(case, "outside", int(outside.sum()), "nonfinite", int((~np.isfinite(val)).sum()), "max", np.nanmax(np.abs(val)))
        if case == HD_CASE:
            for hd in range(len(PAIR_CASES[case][1])):
                out["pairs_%s__k_hd%d" % (case, hd)] = np.asarray(k(Xi, Xj, ni, nj, hyper_deriv=hd), dtype=float)
    for m in MODELS:
        d = model_data(m)
        for key, v in d.items():
            out["model_%s__%s" % (m, key)] = v
        gp = make_model(g, m, d)
        gp.compute_K_L_alpha_ll()
        out["model_%s__ll" % m] = np.float64(gp.ll)
        out["model_%s__alpha" % m] = np.asarray(gp.alpha).ravel()
        mean, std = gp.predict(d["Xs"], n=d["ns"])
        out["model_%s__mean" % m], out["model_%s__std" % m] = np.asarray(mean), np.asarray(std)
        c = slice(N_TRAIN - CORNER, N_TRAIN)
        out["model_%s__K" % m] = np.asarray(gp.compute_Kij(d["X"][c], None, d["n"][c], None))
        cs = slice(M_TEST - CORNER_S, M_TEST)
        out["model_%s__Ks" % m] = np.asarray(gp.compute_Kij(d["Xs"][cs], d["X"][c], d["ns"][cs], d["n"][c]))
        print(m, "ll", gp.ll)
        if m == "a":
            try:
                gp.k(d["X"][:2], d["X"][:2], d["n"][:2], d["n"][:2], hyper_deriv=0)
                raise RuntimeError("the reference's product took hyper_deriv")
            except NotImplementedError:
                pass
        if m == "b":
            trace = model_trace()
            res = gp.predict_MCMC(d["Xs"], n=d["ns"], flat_trace=trace, return_cov=True, return_samples=False, ddof=1, num_proc=0)
            out["model_b__trace"] = trace
            out["model_b__mc_mean"], out["model_b__mc_cov"] = np.asarray(res["mean"]), np.asarray(res["cov"])
            out["model_b__mc_std"] = np.asarray(res["std"]) if "std" in res else np.sqrt(np.diag(np.asarray(res["cov"])))
    path = os.path.join(HERE, "g19_masked.npz")
    np.savez_compressed(path, **out)
    print("bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
