"""Timing of the greedy inducing-input selection on one MI355X.  Not bench.py: a report, nothing is asserted.

Per shape (N = 65536, 262144, 1048576; M = 256, 1024; the SE d = 2 model of section 18.6), from ONE process, device events on the
context's stream, every shape warmed up once:
  1. the whole selection, gpt_sparse_select_inducing (events around the synchronous call: the 3 M + 3 launches and the gaps between them);
  2. the update kernel alone: M launches of gpt_dev_greedy_update, j = 0 .. M - 1, back to back on a factor of the same shape -- its
     effective rate is 4 N M^2 bytes over that time, beside the ~6.3 TB/s a streaming read achieves on this chip;
  3. one gpt_sparse_fit (vfe) at the same N with the M selected rows as inducing inputs (where the SE selection stops before M --
     its residuals reach rounding -- the whole call and the fit are timed with a Matern52 model that runs all M steps).
One JSON line per measurement on stdout.

    python scratch/greedy_timing.py [--quick]
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: the HIP runtime of the process)
from gptools_amd import _lib  # noqa: E402

QUICK = "--quick" in sys.argv
SE = [1.1, 0.4, 0.6]
TERMS = [(_lib.KERNEL_SE, SE)]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, reps):
    """Median and spread of the device time of fn() over reps windows (events on the current stream)."""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), [float(min(out)), float(max(out))]


def shape(N, M, reps):
    rs = np.random.RandomState(7)
    X = rs.rand(N, 2)
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(N)
    ctx = _lib.Context(stream=torch.cuda.current_stream().cuda_stream)
    ctx.set_data(X, np.zeros((N, 2), dtype=int))
    res = {}

    def select():
        res["sel"] = ctx.sparse_select_inducing(TERMS, M)
    select()                                                         # warm-up: code objects, the slots
    sel_ms, sel_spread = timed(select, reps)
    idx, dmax, trace = res["sel"]

    # the update kernel alone on a factor of the same shape (values do not matter to its time; zeros keep everything finite)
    ld = (N + 63) // 64 * 64
    nparts = ctx.dev_greedy_parts(N)
    L = torch.zeros(M, ld, dtype=torch.float64, device="cuda")
    resid, prow = torch.ones(ld, dtype=torch.float64, device="cuda"), torch.zeros(M, dtype=torch.float64, device="cuda")
    mark, words = torch.zeros(ld, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    scal = torch.ones(2, dtype=torch.float64, device="cuda")
    part, pidx = torch.zeros(2 * nparts, dtype=torch.float64, device="cuda"), torch.zeros(nparts, dtype=torch.int32, device="cuda")

    def updates():
        for j in range(M):
            ctx.dev_greedy_update(L.data_ptr(), ld, N, j, L.data_ptr() + 8 * j * ld, resid.data_ptr(), mark.data_ptr(), prow.data_ptr(),
                                  scal.data_ptr(), words.data_ptr(), part.data_ptr(), pidx.data_ptr())
    updates()
    torch.cuda.synchronize()
    upd_ms, upd_spread = timed(updates, reps)
    del L

    emit(what="greedy_select", N=N, M=M, count=len(idx), trace0=float(trace[0]), traceM=float(trace[-1]), select_ms=sel_ms, select_spread_ms=sel_spread,
         update_sum_ms=upd_ms, update_spread_ms=upd_spread, update_TBps=4.0 * N * M * M / (upd_ms * 1e-3) / 1e12)
    terms = TERMS
    if len(idx) < M:
        # the stop rule ended the SE selection early (its residuals reach rounding first): the steps behind `count` are no-ops, so the
        # whole call is timed again with a Matern52 model that runs all M steps, and the fit beside it has that model and its M rows
        terms = [(_lib.KERNEL_M52, [1.0, 0.1, 0.1])]
        res["sel"] = ctx.sparse_select_inducing(terms, M)
        sel_ms, sel_spread = timed(lambda: res.update(sel=ctx.sparse_select_inducing(terms, M)), reps)
        idx = res["sel"][0]
    ctx.sparse_set_inducing(X[idx])
    fit_args = (_lib.SPARSE_METHODS["vfe"], terms, 0.01, y, np.full(N, 0.02), 1e-6, 0)
    ctx.sparse_fit(*fit_args)
    fit_ms, fit_spread = timed(lambda: ctx.sparse_fit(*fit_args), reps)
    emit(what="greedy_select_all_steps", N=N, M=M, model="se" if terms is TERMS else "m52", count=len(idx), select_ms=sel_ms,
         select_spread_ms=sel_spread, update_share_of_select=upd_ms / sel_ms, us_per_step_outside_update=(sel_ms - upd_ms) * 1e3 / M,
         sparse_fit_vfe_ms=fit_ms, sparse_fit_spread_ms=fit_spread, select_over_fit=sel_ms / fit_ms)
    ctx.close()


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("greedy_timing.py needs the GPU: nothing is measured without it")
    for N in ((8192,) if QUICK else (65536, 262144, 1048576)):
        for M in ((64,) if QUICK else (256, 1024)):
            shape(N, M, 3)
