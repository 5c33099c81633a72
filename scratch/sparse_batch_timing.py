"""Timing of SparseGaussianProcess.sparse_ll_batch against the loop it replaces, on one MI355X.  Not bench.py:
a report, nothing is asserted.

Model: SE, d = 2, fitc, the default chunk.  Shapes: N in {4096, 16384, 65536, 262144} x M in {64, 256, 1024, 4096} (M <= N), 32
hyperparameter vectors.  Measured: the wall time of sparse_ll_batch(vectors) of THIS tree, and of the same vectors through
SparseGaussianProcess._ll_rows of the PARENT commit (one gpt_sparse_fit per vector), the parent's package and library imported from a
checkout of it built in a second directory:

    git archive HEAD^ | tar -x -C /some/dir && make -C /some/dir/gptools_amd/csrc
    python scratch/sparse_batch_timing.py --parent /some/dir [--quick]

Each side runs in a process of its own (two packages of one name cannot share an interpreter); the driver alternates the two, five
windows each after a warm-up call, one window = REPS calls.  The two results are compared first (the same bits).  One JSON line per
shape on stdout."""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NVEC, WINDOWS = 32, 5


def worker(root, side):
    sys.path.insert(0, root)
    import warnings
    warnings.simplefilter("ignore")
    import numpy as np
    import gptools_amd as g
    gp, vecs = None, None
    for line in sys.stdin:
        cmd = json.loads(line)
        if cmd["op"] == "setup":
            N, M = cmd["N"], cmd["M"]
            rs = np.random.RandomState(7)
            X = rs.rand(N, 2)
            y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(N)
            k = g.SquaredExponentialKernel(num_dim=2, initial_params=[1.1, 0.4, 0.6], param_bounds=[(0.0, 1e3)] * 3)
            gp = g.SparseGaussianProcess(k, rs.rand(M, 2), noise_k=g.DiagonalNoiseKernel(num_dim=2, initial_noise=0.1, noise_bound=(0.0, 5.0)),
                                         method="fitc", X=X, y=y, err_y=0.02)
            x0 = np.array(gp.free_params[:], dtype=float)
            vecs = [x0 * rs.uniform(0.9, 1.1, size=x0.size) for _ in range(NVEC)]
            out = {"ok": True}
        elif cmd["op"] == "call":
            fn = gp.sparse_ll_batch if side == "new" else gp._ll_rows
            t0 = time.perf_counter()
            for _ in range(cmd["reps"]):
                ll = fn(vecs)
            out = {"ms": (time.perf_counter() - t0) * 1e3 / cmd["reps"], "ll": [float(v).hex() for v in ll]}
        else:
            break
        print(json.dumps(out), flush=True)


def ask(proc, **cmd):
    proc.stdin.write(json.dumps(cmd) + "\n")
    proc.stdin.flush()
    return json.loads(proc.stdout.readline())


def main():
    if "--worker" in sys.argv:
        return worker(sys.argv[sys.argv.index("--worker") + 1], sys.argv[sys.argv.index("--side") + 1])
    parent = os.path.abspath(sys.argv[sys.argv.index("--parent") + 1])
    quick = "--quick" in sys.argv
    procs = {side: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root, "--side", side], stdin=subprocess.PIPE,
                                    stdout=subprocess.PIPE, universal_newlines=True)
             for side, root in (("new", HERE), ("parent", parent))}
    Ns = (4096, 16384) if quick else (4096, 16384, 65536, 262144)
    Ms = (64, 1024) if quick else (64, 256, 1024, 4096)
    try:
        for N in Ns:
            for M in Ms:
                if M > N:
                    continue
                first = {}
                for side, p in procs.items():
                    ask(p, op="setup", N=N, M=M)
                    first[side] = ask(p, op="call", reps=1)                         # warm-up: code objects, workspaces
                    first[side] = ask(p, op="call", reps=1)
                reps = {s: max(1, min(10, int(200.0 / first[s]["ms"]))) for s in procs}    # a window of about 0.2 s, at least one call
                ms = {s: [] for s in procs}
                for _ in range(WINDOWS):
                    for side, p in procs.items():
                        ms[side].append(ask(p, op="call", reps=reps[side])["ms"])
                med = {s: sorted(v)[len(v) // 2] for s, v in ms.items()}
                print(json.dumps(dict(what="sparse_ll_batch_vs_loop", N=N, M=M, vectors=NVEC, same_bits=first["new"]["ll"] == first["parent"]["ll"],
                                      batch_ms=med["new"], loop_ms=med["parent"], batch_spread_ms=[min(ms["new"]), max(ms["new"])],
                                      loop_spread_ms=[min(ms["parent"]), max(ms["parent"])], loop_over_batch=med["parent"] / med["new"])),
                      flush=True)
    finally:
        for p in procs.values():
            try:
                ask(p, op="quit")
            except Exception:
                pass
            p.stdin.close()
            p.wait(timeout=60)


if __name__ == "__main__":
    main()
