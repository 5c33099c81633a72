#!/usr/bin/env python
"""g14_mcmc.npz: predictions marginalised over a trace of hyperparameters, from the imported reference's
``predict(use_MCMC=True)``, ``predict_MCMC`` and ``compute_from_MCMC`` with ``flat_trace`` (ref: gaussian_process.py:888-912,
:1840-1987, :2144-2330).  The reference is run with ``num_proc=2`` (its process pool: ``pool.map`` returns a list, so every
key of compute_from_MCMC comes back complete -- with ``num_proc <= 1`` a one-shot ``map`` iterator leaves all keys after
``'mean'`` empty under Python 3).

Size: the per-row covariances are most of the file, so the calls that return them walk every other (fourth) row, and of the
mean-function keys only the independent ones are stored -- the reference's per-row ``cov_func`` is all zeros and its
``cov_without_func`` equals ``cov`` (both asserted here; the tests check the same relations on this package's results).

Layout: per case ``<case>__X``, ``__y``, ``__n``, ``__err_y``, ``__Xs``, ``__ns``, ``__trace`` (and ``__A``, the output transform);
per call ``<case>__<call>__<key>`` with the per-row lists of compute_from_MCMC stacked along a first axis.  ``make_gp`` builds
the case's GaussianProcess from either package (the reference's API and this package's are the same), so the tests build the
very same models without the reference.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = ("se1", "m52d", "sum", "mu", "ot", "drop")


def _data(name):
    rs = np.random.RandomState({"se1": 1, "m52d": 2, "sum": 3, "mu": 4, "ot": 5, "drop": 6}[name])
    if name == "m52d":
        N, M = 48, 20
        X = rs.uniform(-2.0, 2.0, (N, 2))
        n = np.zeros((N, 2), dtype=int)
        n[36:42, 0] = 1                                # derivative observations
        n[42:, 1] = 1
        y = np.sin(X[:, 0]) * np.cos(X[:, 1]) + 0.05 * rs.randn(N)
        Xs = rs.uniform(-2.0, 2.0, (M, 2))
        ns = np.zeros((M, 2), dtype=int)
        ns[12:16, 0] = 1                               # derivative predictions
        ns[16:, 1] = 1
        trace = np.column_stack([rs.uniform(0.8, 1.5, 24), rs.uniform(0.8, 1.6, 24), rs.uniform(0.8, 1.6, 24)])
        return dict(X=X, y=y, n=n, err_y=np.full(N, 0.05), Xs=Xs, ns=ns, trace=trace)
    N, M = (60, 40) if name == "ot" else (60, 20) if name != "drop" else (40, 20)
    X = np.sort(rs.uniform(0.0, 5.0, N))[:, None]
    y = np.sin(1.3 * X[:, 0]) + 0.3 * X[:, 0] + 0.1 * rs.randn(N)
    Xs = np.linspace(-0.5, 5.5, M)[:, None]
    ns = np.zeros((M, 1), dtype=int)
    if name == "se1":
        ns[-6:] = 1                                    # a few slopes
    S = 12 if name == "drop" else 24
    sf, ls = rs.uniform(0.7, 1.6, S), rs.uniform(0.6, 1.4, S)
    if name == "se1":
        trace = np.column_stack([sf, ls, rs.uniform(0.05, 0.2, S)])          # + sigma_n of the DiagonalNoiseKernel
    elif name == "sum":
        trace = np.column_stack([sf, ls, rs.uniform(0.2, 0.6, S), rs.uniform(1.0, 3.0, S)])
    elif name == "mu":
        trace = np.column_stack([sf, ls, rs.uniform(-0.5, 1.5, S)])          # + the constant of the mean function
    else:
        trace = np.column_stack([sf, ls])
    if name == "drop":
        trace[3, 1] = np.nan                           # evaluation fails: dropped
        trace[7, 1] = 12.0                             # outside the length scale's bounds: the prior excludes it, still evaluated
    out = dict(X=X, y=y, n=np.zeros((N, 1), dtype=int), err_y=np.full(N, 0.1), Xs=Xs, ns=ns, trace=trace)
    if name == "ot":
        out["A"] = rs.randn(5, M) / M
    return out


def make_gp(g, name, d):
    """The case's GaussianProcess from package ``g`` (the reference's gptools or gptools_amd), data added."""
    b = [(1e-3, 10.0)]
    if name == "m52d":
        k = g.Matern52Kernel(num_dim=2, initial_params=[1.0, 1.0, 1.0], param_bounds=b * 3)
    elif name == "sum":
        k = (g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 1.0], param_bounds=b * 2) +
             g.Matern52Kernel(num_dim=1, initial_params=[0.4, 2.0], param_bounds=b * 2))
    else:
        k = g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 1.0], param_bounds=b * 2)
    kw = {}
    if name == "se1":
        kw["noise_k"] = g.DiagonalNoiseKernel(num_dim=1, initial_noise=0.1, noise_bound=(1e-4, 1.0))
    if name == "mu":
        kw["mu"] = g.ConstantMeanFunction(initial_params=[0.5], param_bounds=[(-5.0, 5.0)])
    gp = g.GaussianProcess(k, **kw)
    gp.add_data(d["X"], d["y"], err_y=d["err_y"], n=d["n"])
    return gp


# (call name, method, keyword arguments); every call gets flat_trace and num_proc=2
CALLS = {
    "se1": [("cfm", "compute_from_MCMC", dict(return_std=True, return_cov=True, thin=2)),
            ("cfm_noise", "compute_from_MCMC", dict(return_std=True, noise=True)),
            ("pm_cov1", "predict_MCMC", dict(return_cov=True, return_samples=False, ddof=1)),
            ("pm_cov0_noise", "predict_MCMC", dict(return_cov=True, return_samples=False, ddof=0, noise=True)),
            ("pm_std", "predict_MCMC", dict(return_std=True, return_samples=False, ddof=1)),
            ("pr_std_bt", "predict", dict(use_MCMC=True, return_std=True, burn=2, thin=3))],
    "m52d": [("cfm", "compute_from_MCMC", dict(return_std=True, return_cov=True, thin=2)),
             ("pm_cov1", "predict_MCMC", dict(return_cov=True, return_samples=False, ddof=1)),
             ("pm_std0", "predict_MCMC", dict(return_std=True, return_samples=False, ddof=0))],
    "sum": [("cfm", "compute_from_MCMC", dict(return_std=True)),
            ("pm_cov1", "predict_MCMC", dict(return_cov=True, return_samples=False, ddof=1))],
    "mu": [("cfm", "compute_from_MCMC", dict(return_std=True, return_cov=True, return_mean_func=True, thin=4)),
           ("pr_full", "predict", dict(use_MCMC=True, full_output=True, return_mean_func=True))],
    "ot": [("cfm", "compute_from_MCMC", dict(return_std=True, return_cov=True, output_transform="A")),
           ("pm_std", "predict_MCMC", dict(return_std=True, return_samples=False, output_transform="A")),
           ("pm_cov", "predict_MCMC", dict(return_cov=True, return_samples=False, output_transform="A"))],
    "drop": [("cfm", "compute_from_MCMC", dict(return_std=True, return_cov=True)),
             ("pm_cov1", "predict_MCMC", dict(return_cov=True, return_samples=False, ddof=1))],
}


def call_kwargs(d, kw):
    """The keyword arguments of a call, with the case's arrays in (shared by the generator and the tests)."""
    kw = dict(kw)
    if kw.get("output_transform") == "A":
        kw["output_transform"] = d["A"]
    kw["n"] = d["ns"]
    kw["flat_trace"] = d["trace"]
    return kw


def main():
    sys.path.insert(0, HERE)
    from ref_harness import import_reference
    gptools = import_reference()
    out = {}
    for name in CASES:
        d = _data(name)
        for key, v in d.items():
            out["%s__%s" % (name, key)] = np.asarray(v)
        for call, meth, kw in CALLS[name]:
            gp = make_gp(gptools, name, d)
            kw = call_kwargs(d, kw)
            kw["num_proc"] = 2
            res = getattr(gp, meth)(d["Xs"], **kw)
            if isinstance(res, tuple):
                res = dict(zip(("mean", "second"), res))
            if meth == "compute_from_MCMC" and "cov_func" in res:
                assert not np.any(np.asarray(res.pop("cov_func")))
                assert np.array_equal(np.asarray(res.pop("cov_without_func")), np.asarray(res["cov"]))
            for key, v in res.items():
                out["%s__%s__%s" % (name, call, key)] = np.asarray(v, dtype=float)
            print(name, call, {k: np.shape(v) for k, v in res.items()})
    np.savez_compressed(os.path.join(HERE, "g14_mcmc.npz"), **out)


if __name__ == "__main__":
    main()
