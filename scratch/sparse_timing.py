"""Timing of the inducing-point path on one MI355X.  Not bench.py: a report, nothing is asserted.

  1. gpt_sparse_fit per phase (option "timing": device events at the phase boundaries of every chunk, summed by the library):
     K_fu build, right-side solve, row pass, Gram, the two factorisations -- N = 65536 and 262144, M = 256, 1024, 4096, SE d = 2, fitc.
  2. The Gram kernel alone (gpt_dev_sparse_gram) against gpt_dev_gemm_nt(..., tri=1) on a transposed copy of the same chunk, alternating
     in the same run, device events around REPS launches each; the two results are compared first.
  3. The dense gpt_fit at N = 16384 from the same process, for scale.

Every shape is warmed up once before it is timed.  One JSON line per measurement on stdout.

    python scratch/sparse_timing.py [--quick] [--slices] [--gram-only]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: the HIP runtime of the process)
from gptools_amd import _lib  # noqa: E402

QUICK = "--quick" in sys.argv
SE = [1.1, 0.4, 0.6]
REPS = 3 if QUICK else 10


def emit(**kw):
    print(json.dumps(kw), flush=True)


def fit_phases(N, M):
    rs = np.random.RandomState(7)
    X = rs.rand(N, 2)
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(N)
    ctx = _lib.Context()
    ctx.set_data(X, np.zeros((N, 2), dtype=int))
    ctx.sparse_set_inducing(rs.rand(M, 2))
    ctx.set_option("timing", 1)
    args = (_lib.SPARSE_METHODS["fitc"], [(_lib.KERNEL_SE, SE)], 0.01, y, np.full(N, 0.02), 1e-6, 0)
    ll, _ = ctx.sparse_fit(*args)                                    # warm-up: code objects, workspaces
    phases, wall = [], []
    for _ in range(2 if QUICK else 3):
        t0 = time.perf_counter()
        ll, _ = ctx.sparse_fit(*args)                                # (synchronous: ends in a stream synchronise)
        wall.append((time.perf_counter() - t0) * 1e3)
        phases.append(list(ctx.last_timings().values()))      # (after a sparse fit the five slots are the five phases)
    ph = np.median(np.array(phases), axis=0)
    emit(what="sparse_fit", N=N, M=M, ll=ll, wall_ms=float(np.median(wall)), kfu_build_ms=float(ph[0]), solve_ms=float(ph[1]), row_pass_ms=float(ph[2]),
         gram_ms=float(ph[3]), factorisations_ms=float(ph[4]), gram_tflops=float(N * (M + 1.0) ** 2 / (ph[3] * 1e-3) / 1e12))
    ctx.close()


def gram_against_gemm(M, rows, nslices=0):
    """Device events around REPS launches of each kernel, alternating A / B five times.  nslices: 0 = the fit's choice."""
    mg = (M + 1 + 63) // 64 * 64
    ldv = (M + 1 + 127) // 128 * 128
    ctx = _lib.Context(stream=torch.cuda.current_stream().cuda_stream)
    lib = _lib.load()
    V = torch.randn(rows, ldv, dtype=torch.float64, device="cuda")
    Vt = V[:, :mg].t().contiguous()                                  # mg x rows: the layout gemm_nt wants (long dimension contiguous)
    G1 = torch.zeros(mg, mg, dtype=torch.float64, device="cuda")
    G2 = torch.zeros(mg, mg, dtype=torch.float64, device="cuda")

    def gram():
        _lib.check(lib.gpt_dev_sparse_gram(ctx.handle, V.data_ptr(), ldv, rows, mg, nslices, G1.data_ptr(), mg))

    def gemm():
        _lib.check(lib.gpt_dev_gemm_nt(ctx.handle, mg, mg, rows, 1.0, Vt.data_ptr(), rows, Vt.data_ptr(), rows, 1.0, G2.data_ptr(), mg, 1))
    gram()
    gemm()
    torch.cuda.synchronize()
    low = torch.tril(torch.ones(mg, mg, device="cuda")) > 0          # (gemm_nt cuts small launches into 32 x 32 tiles: compare i >= j only)
    diff = float(((G1 - G2).abs() * low).max() / G2.abs().max())
    times = {"gram": [], "gemm": []}
    for _ in range(5):
        for name, fn in (("gram", gram), ("gemm", gemm)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / REPS)
    flop = rows * mg * (mg + 64.0)                                   # 2 * rows per element of the lower 64 x 64 tiles
    g, m = float(np.median(times["gram"])), float(np.median(times["gemm"]))
    emit(what="gram_vs_gemm_nt", M=M, rows=rows, mg=mg, nslices=nslices, rel_diff=diff, gram_ms=g, gemm_nt_ms=m, gram_spread_ms=[min(times["gram"]), max(times["gram"])],
         gemm_spread_ms=[min(times["gemm"]), max(times["gemm"])], gram_tflops=flop / (g * 1e-3) / 1e12, gemm_tflops=flop / (m * 1e-3) / 1e12,
         gemm_over_gram=m / g)
    ctx.close()


def dense_fit(N):
    rs = np.random.RandomState(7)
    X = rs.rand(N, 2)
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(N)
    ctx = _lib.Context()
    ctx.set_data(X, np.zeros((N, 2), dtype=int))
    args = (_lib.KERNEL_SE, SE, 0.01, y, np.full(N, 0.02), 1e2 * np.finfo(float).eps)
    ctx.fit(*args)
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        ll, _ = ctx.fit(*args)
        wall.append((time.perf_counter() - t0) * 1e3)
    emit(what="dense_fit", N=N, ll=ll, wall_ms=float(np.median(wall)))
    ctx.close()


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("sparse_timing.py needs the GPU: nothing is measured without it")
    Ns = (8192,) if QUICK else (65536, 262144)
    Ms = (256, 1024) if QUICK else (256, 1024, 4096)
    for M in Ms:
        rows = min(max(64, (512 << 20) // (2 * ((M + 128) // 128 * 128) * 8) // 64 * 64), 65536)      # the fit's default chunk
        gram_against_gemm(M, 8192 if QUICK else rows)
        if "--slices" in sys.argv:                                   # the slice count against the fit's choice (0)
            ntiles = ((M + 64) // 64) * ((M + 64) // 64 + 1) // 2
            for mult in (3, 4, 6, 8):
                if mult * 256 // ntiles >= 1:
                    gram_against_gemm(M, rows, max(1, mult * 256 // ntiles))
    if "--gram-only" in sys.argv:
        raise SystemExit(0)
    for N in Ns:
        for M in Ms:
            fit_phases(N, M)
    dense_fit(4096 if QUICK else 16384)
