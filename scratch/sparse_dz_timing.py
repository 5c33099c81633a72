"""Timing of gpt_sparse_grad_z on one MI355X.  Not bench.py: a report, nothing is asserted.

  1. gpt_sparse_grad_diff of this library against the same call of another build of the library (--prev PATH, e.g. the parent commit's
     libgpt_hip.so), and gpt_sparse_grad_z beside them: one process, the three calls in alternated windows after a warm-up, wall time of
     the synchronous calls, median of 3.  SE, d = 2, three free kernel parameters, vfe; N = 65536 and 262144 at M = 256 and 1024.
  2. The pair pass alone (gpt_dev_sparse_grad_dz_pairs) on 32768 rows at the same M.
  3. One optimize_inducing run at N = 65536, M = 256, vfe: steps, wall time, objective before and after.

Host wall time (time.perf_counter) around the synchronous calls, not device events: the calls run on the context's own stream and
copy their arguments and results inside the call, so every figure includes the host's launch and copy overhead.

One JSON line per measurement on stdout.

    python scratch/sparse_dz_timing.py [--prev PATH] [--quick]
"""
import importlib.util
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
PREV = sys.argv[sys.argv.index("--prev") + 1] if "--prev" in sys.argv else None
SE = [1.1, 0.4, 0.6]
NEW_EXPORTS = ("gpt_sparse_grad_z", "gpt_dev_sparse_grad_dz_pairs")


def emit(**kw):
    print(json.dumps(kw), flush=True)


def previous_build(path):
    """The bindings of gptools_amd/_lib.py a second time, over another build of the library (without the exports it does not have)."""
    spec = importlib.util.spec_from_file_location("gptools_amd._lib_prev", _lib.__file__)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    mod.LIB_PATH = os.path.abspath(path)
    for name in NEW_EXPORTS:
        mod.SIGNATURES.pop(name, None)
    return mod


def data(N, M):
    rs = np.random.RandomState(7)
    X = rs.rand(N, 2)
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(N)
    return X, y, rs.rand(M, 2)


def stencil():
    pa, pb, dn = [], [], []
    for h in range(3):
        eps = 6e-6 * max(1.0, abs(SE[h]))
        a, b = list(SE), list(SE)
        a[h] -= eps
        b[h] += eps
        pa.append(a)
        pb.append(b)
        dn.append(b[h] - a[h])
    return [0, 0, 0], pa, pb, dn


def gradients(N, M, prev, method="vfe"):
    X, y, Z = data(N, M)
    err = np.full(N, 0.02)
    tix, pa, pb, dn = stencil()
    ctxs = {"new": _lib.Context()}
    if prev is not None:
        ctxs["prev"] = prev.Context()
    for c in ctxs.values():
        c.set_data(X, np.zeros((N, 2), dtype=int))
        c.sparse_set_inducing(Z)
        c.sparse_fit(_lib.SPARSE_METHODS[method], [(_lib.KERNEL_SE, SE)], 0.01, y, err, 1e-6, 0)
        c.sparse_grad_diff(tix, pa, pb, dn, y, err)                              # warm-up: code objects, workspaces
    ctxs["new"].sparse_grad_z(tix, pa, pb, dn, y, err)
    ctxs["new"].sparse_grad_z([], [], [], [], y, err)
    t = {"prev_diff": [], "new_diff": [], "new_z": [], "new_z_alone": []}
    outs = {}
    for _ in range(3):
        for name, c in sorted(ctxs.items(), reverse=True):                       # prev, then new
            t0 = time.perf_counter()
            outs[name] = c.sparse_grad_diff(tix, pa, pb, dn, y, err)[0]
            t[name + "_diff"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        outz, _, dz = ctxs["new"].sparse_grad_z(tix, pa, pb, dn, y, err)
        t["new_z"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ctxs["new"].sparse_grad_z([], [], [], [], y, err)
        t["new_z_alone"].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in t.items() if v}
    emit(what="gradients", N=N, M=M, method=method, same_bits_as_prev=(bool(np.array_equal(outs["new"], outs["prev"])) if prev else None),
         same_bits_diff_and_z=bool(np.array_equal(outs["new"], outz)), max_abs_dz=float(np.abs(dz).max()), **{k + "_ms": v for k, v in med.items()})
    for c in ctxs.values():
        c.close()


def pair_pass(M, rows=32768):
    rs = np.random.RandomState(3)
    lda = (M + 1 + 127) // 128 * 128
    dX, dZ = torch.tensor(rs.rand(rows, 2), device="cuda"), torch.tensor(rs.rand(M, 2), device="cuda")
    dA = torch.randn(rows, lda, dtype=torch.float64, device="cuda")
    dnx, dnz = torch.zeros(rows, 2, dtype=torch.int32, device="cuda"), torch.zeros(M, 2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx = _lib.Context()
    out = np.zeros((M, 2))
    p = np.array(SE)

    def call():
        _lib.check(_lib.load().gpt_dev_sparse_grad_dz_pairs(ctx.handle, _lib.KERNEL_SE, -1, 2, 1, _lib.dptr(p), 3, 3, dX.data_ptr(), dnx.data_ptr(),
                                                            rows, dZ.data_ptr(), dnz.data_ptr(), M, dA.data_ptr(), lda, 0, _lib.dptr(out)))
    call()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    emit(what="pair_pass_alone", rows=rows, M=M, D=2, ms=float(np.median(ts)), ns_per_pair_and_dim=float(np.median(ts)) * 1e6 / (rows * M * 2))
    ctx.close()


def optimise(N, M):
    X, y, _ = data(N, M)
    Z0 = np.random.RandomState(11).rand(M, 2)
    gp = g.SparseGaussianProcess(g.SquaredExponentialKernel(num_dim=2, initial_params=[1.0, 0.5, 0.5], param_bounds=[(1e-2, 10.0)] * 3), Z0,
                                 noise_k=g.DiagonalNoiseKernel(num_dim=2, initial_noise=0.1, noise_bound=(1e-3, 5.0)), method="vfe", X=X, y=y,
                                 err_y=0.02)
    theta = np.array(gp.free_params[:], dtype=float)
    before = -gp.update_hyperparameters(theta)
    gp.inducing_gradient()                                                       # warm-up
    t0 = time.perf_counter()
    res = gp.optimize_inducing(opt_kwargs={"options": {"maxiter": 30}})
    emit(what="optimize_inducing", N=N, M=M, wall_s=time.perf_counter() - t0, nit=int(res.nit), nfev=int(res.nfev), before=float(before),
         after=float(-res.fun), success=bool(res.success))


if __name__ == "__main__":
    warnings.simplefilter("ignore")
    prev = previous_build(PREV) if PREV else None
    shapes = [(65536, 256)] if QUICK else [(65536, 256), (65536, 1024), (262144, 256), (262144, 1024)]
    for N, M in shapes:
        gradients(N, M, prev)
    for M in ([256] if QUICK else [256, 1024]):
        pair_pass(M)
    optimise(65536, 256)
