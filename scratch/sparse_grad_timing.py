"""Timing of gpt_sparse_grad_diff on one MI355X.  Not bench.py: a report, nothing is asserted.

  1. One gpt_sparse_fit and one gpt_sparse_grad_diff (three free kernel parameters of an SE model, d = 2) from the same process, wall time
     of the synchronous calls, warmed up, median of 3: N = 65536 and 262144 at M = 256 and 1024, fitc and vfe.  (The call has no phase
     marks of its own yet: the whole call against the whole fit.)
  2. One SLSQP run of SparseGaussianProcess.optimize_hyperparameters at N = 65536, M = 256 by each route: gradient=None (scipy
     differences the value) and gradient="sparse".

One JSON line per measurement on stdout.

    python scratch/sparse_grad_timing.py [--quick]
"""
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (first: the HIP runtime of the process)
import gptools_amd as g  # noqa: E402
from gptools_amd import _lib  # noqa: E402

QUICK = "--quick" in sys.argv
SE = [1.1, 0.4, 0.6]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def data(N, M):
    rs = np.random.RandomState(7)
    X = rs.rand(N, 2)
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(N)
    return X, y, rs.rand(M, 2)


def fit_and_gradient(N, M, method):
    X, y, Z = data(N, M)
    err = np.full(N, 0.02)
    ctx = _lib.Context()
    ctx.set_data(X, np.zeros((N, 2), dtype=int))
    ctx.sparse_set_inducing(Z)
    fit_args = (_lib.SPARSE_METHODS[method], [(_lib.KERNEL_SE, SE)], 0.01, y, err, 1e-6, 0)
    pa, pb, dn = [], [], []
    for h in range(3):
        eps = 6e-6 * max(1.0, abs(SE[h]))
        a, b = list(SE), list(SE)
        a[h] -= eps
        b[h] += eps
        pa.append(a)
        pb.append(b)
        dn.append(b[h] - a[h])
    ll, _ = ctx.sparse_fit(*fit_args)
    out, _ = ctx.sparse_grad_diff([0, 0, 0], pa, pb, dn, y, err)                 # warm-up: code objects, workspaces
    tf, tg = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.sparse_fit(*fit_args)
        tf.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        out, _ = ctx.sparse_grad_diff([0, 0, 0], pa, pb, dn, y, err)
        tg.append((time.perf_counter() - t0) * 1e3)
    emit(what="fit_and_gradient", N=N, M=M, method=method, ll=ll, grad=[float(v) for v in out], fit_ms=float(np.median(tf)),
         grad_ms=float(np.median(tg)), grad_over_fit=float(np.median(tg) / np.median(tf)))
    ctx.close()


def slsqp(N, M):
    X, y, Z = data(N, M)
    for gradient in (None, "sparse"):
        gp = g.SparseGaussianProcess(g.SquaredExponentialKernel(num_dim=2, initial_params=[1.0, 0.5, 0.5], param_bounds=[(1e-2, 10.0)] * 3), Z,
                                     noise_k=g.DiagonalNoiseKernel(num_dim=2, initial_noise=0.1, noise_bound=(1e-3, 5.0)), method="vfe", X=X,
                                     y=y, err_y=0.02)
        gp.update_hyperparameters(np.array(gp.free_params[:], dtype=float))       # warm-up
        t0 = time.perf_counter()
        best, _ = gp.optimize_hyperparameters(random_starts=0, opt_kwargs={"options": {"ftol": 1e-6, "maxiter": 60}}, gradient=gradient)
        emit(what="slsqp", N=N, M=M, gradient=gradient, wall_s=time.perf_counter() - t0, fun=float(best.fun), nfev=int(best.nfev),
             njev=int(best.njev), success=bool(best.success))


if __name__ == "__main__":
    warnings.simplefilter("ignore")
    shapes = [(65536, 256)] if QUICK else [(65536, 256), (65536, 1024), (262144, 256), (262144, 1024)]
    for N, M in shapes:
        for method in ("fitc", "vfe"):
            fit_and_gradient(N, M, method)
    slsqp(65536, 256)
