#!/usr/bin/env python
"""bench.py -- throughput of the covariance-build + Cholesky log-marginal-likelihood hot path on MI355X.

Metric (BASELINE.json): "K-build+Cholesky GFLOP/s (% fp64 MFMA peak) and LML evals/sec, N=8192".
A *step* is one FULL LML evaluation on a fixed synthetic data set: fused K-build (with the diagonal
loading) + blocked Cholesky + z = L^-1 y + log-determinant + the ll scalar + alpha = K_tot^-1 y returned to the
host -- compute_K_L_alpha_ll as the reference performs it (ref: gptools/gaussian_process.py:1418-1469).
X, n are resident in HBM before the timed region; per step only the hyperparameters (and the 2 x 64 KB
y / err_y vectors) cross the boundary.

  python bench.py --gpus 1 --steps K --warmup W          # 1 GPU: config C3 (Matern52, N=8192, d=3, derivative rows)
  python bench.py --gpus N ...                            # N>1: config C4 (SE, N=32768, d=4) block-cyclic panel
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...
                                                          # Cholesky partitioned over the N ranks, RCCL broadcasts; without a
                                                          # launcher (no RANK in the environment) bench.py starts its N ranks
                                                          # itself as child processes (self_launch)
value  = algorithmic flops of the steps / wall time, in GFLOP/s, with the LAPACK potrf+potrs count
         (N^3/3 + N^2/2 + N/6 + 2 N^2) -- K-build time is in the denominator but adds no flops.

A plain run does only what `value` needs: set-up, --warmup steps, the --steps timed steps, --dump-outputs, the line.
(With N > 1 that includes the tuning pass over the other schedules, since the fastest one becomes the line, and
`roofline`, which HIP events take inside the timed steps.)  Everything else the bench measures or checks runs with --full,
whose --no-* switches leave single legs out:
roofline  : N = 1: the trailing-update SYRK/GEMM kernel (fp64 MFMA bound), achieved = sum of algorithmic flops of the
            large GEMM launches / sum of their HIP-event durations, in instrumented steps after the timed region.
cpu_baseline : the oracle's fused K-build (OpenMP) + scipy.linalg.cholesky / cho_solve on the host cores
            (rank 0), a reported baseline and the reference of the parity gate, which fails the run (exit 4).
other legs : N = 1: two evaluations in flight (`batched`), the step without alpha (`lazy_alpha`), the plugin API
            (`via_gp_api`, `with_alpha`), predict, the K build alone.  N > 1: C5 partitioned, C3 replicas, step trace and
            link probes, the single-GPU run of the same workload.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP64_MFMA_PEAK_TFLOPS = 78.6      # MI355X fp64 matrix peak (256 CU x 4 SIMD x 32 flop/clk x 2.4 GHz); measured 77.8
METRIC = "K-build+Cholesky GFLOP/s (% fp64 MFMA peak) and LML evals/sec, N=8192"

WORKLOADS = {
    # name: (kernel, N, d, derivative rows)                        BASELINE.json configs[i]
    "c2": ("se", 4096, 2, False),      # configs[1]
    "c3": ("m52", 8192, 3, True),      # configs[2]  <- the metric's N=8192 configuration
    "c5": ("se", 16384, 2, False),     # configs[4] (one objective evaluation of the MAP loop)
    "c4": ("se", 32768, 4, False),     # configs[3]
}
KID = {"se": 0, "m52": 1}


def synth(kernel, N, d, deriv):
    """Deterministic inputs of SURVEY.md section 8(d)."""
    rs = np.random.RandomState(1234)
    X = rs.rand(N, d)
    s = X.sum(axis=1)
    y = np.sin(s)
    n = np.zeros((N, d), dtype=np.int32)
    if deriv:
        for i in range(3 * N // 4, N):
            n[i, i % d] = 1
            y[i] = np.cos(s[i])
    y = y + 0.05 * rs.randn(N)
    params = np.concatenate(([1.0], 0.3 * np.ones(d)))
    return X, n, y, 0.05 * np.ones(N), params


def flops_fit(N, alpha=True):
    """LAPACK counts: potrf N^3/3 + N^2/2 + N/6, potrs 2 N^2.  ``alpha=False``: what a GPU step EXECUTES when
    alpha is not asked for -- the forward half of potrs (z = L^-1 y rides along as the augmented row), N^2."""
    return N ** 3 / 3.0 + N ** 2 / 2.0 + N / 6.0 + (2.0 if alpha else 1.0) * N ** 2


_CPU_CHILD = r"""
import json, os, sys, time
th, cpus, root, kernel, N, d, deriv = int(sys.argv[1]), [int(v) for v in sys.argv[2].split(",")], sys.argv[3], sys.argv[4], int(sys.argv[5]), int(sys.argv[6]), int(sys.argv[7])
os.sched_setaffinity(0, cpus)              # BEFORE any BLAS / OpenMP thread exists: the workers inherit this mask
for k in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[k] = str(th)
sys.path.insert(0, root)
import numpy as np, scipy.linalg
import bench
from oracle import oracle as O
X, n, y, err, params = bench.synth(kernel, N, d, bool(deriv))
tm = {}
best = None
for rep in range(2):
    tm = {}
    t0 = time.perf_counter()
    res = O.fit(kernel, params, X, n, y, err, chol="scipy", timings=tm)
    t = time.perf_counter() - t0
    if best is None or t < best[0]:
        best = (t, dict(tm), res["ll_data"], res["logdet_half"])
print("CPUCHILD " + json.dumps({"threads": th, "t_eval_s": best[0], "t_kbuild_s": best[1]["kbuild_s"], "t_potrf_s": best[1]["potrf_s"],
                                "t_solve_ll_s": best[1]["solve_ll_s"], "ll_data": best[2], "logdet_half": best[3]}))
"""


def _numa_node0_cpus():
    """CPUs of NUMA node 0 this process may use, physical cores first (the first half of a node's cpulist on SMT hosts)."""
    allowed = sorted(os.sched_getaffinity(0))
    try:
        txt = open("/sys/devices/system/node/node0/cpulist").read().strip()
        cpus = []
        for part in txt.split(","):
            lo, _, hi = part.partition("-")
            cpus.extend(range(int(lo), int(hi or lo) + 1))
        cpus = [c for c in cpus if c in set(allowed)]
        return cpus or allowed, txt
    except (OSError, ValueError):
        return allowed, "unknown"


def cpu_baseline(kernel, X, n, y, err, params, sweep=True, workload=None):
    """The reference-equivalent CPU path on the GPU box's host cores: the oracle's fused K-build (C, OpenMP) +
    scipy.linalg.cholesky / cho_solve, like the reference's gaussian_process.py:1452,1462; K-build and factorisation timed
    separately.  One evaluation runs in this process (it also provides L and alpha for the parity gate); the
    quoted baseline is the best of a sweep over {8, 16, 32, 64} threads, each in a CHILD process whose CPU affinity is set to
    that many cores of NUMA node 0 before any BLAS / OpenMP thread exists (with the default of one thread per
    visible core -- 256 on this pool's hosts -- OpenBLAS' dpotrf crawls at N = 8192; BASELINE.md measured 81.7 GFLOP/s on 8
    vCPUs).  A bounded sample: ~5 evaluations of the workload."""
    from oracle import oracle as O
    import subprocess
    cores = len(os.sched_getaffinity(0))
    N = X.shape[0]
    tm = {}
    t0 = time.perf_counter()
    res = O.fit(kernel, params, X, n, y, err, chol="scipy", timings=tm)
    t_default = time.perf_counter() - t0
    try:
        from threadpoolctl import threadpool_info
        blas_threads = max([i.get("num_threads", 0) for i in threadpool_info() if i.get("user_api") == "blas"] or [0])
    except Exception:
        blas_threads = 0
    potrf_flops = N ** 3 / 3.0 + N ** 2 / 2.0 + N / 6.0
    runs = {"default": {"threads": blas_threads, "placement": "all visible cores, no pinning", "t_eval_s": t_default,
                        "t_kbuild_s": tm["kbuild_s"], "t_potrf_s": tm["potrf_s"], "t_solve_ll_s": tm["solve_ll_s"]}}
    node_cpus, node_txt = _numa_node0_cpus()
    if sweep and workload is not None:
        kern_, N_, d_, deriv_ = workload
        for th in (8, 16, 32, 64):
            if th > len(node_cpus):
                continue
            cpus = node_cpus[:th]
            try:
                out = subprocess.run([sys.executable, "-c", _CPU_CHILD, str(th), ",".join(str(c) for c in cpus), ROOT, kern_, str(N_),
                                      str(d_), str(int(deriv_))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
                line = [l for l in out.stdout.splitlines() if l.startswith("CPUCHILD ")]
                if out.returncode == 0 and line:
                    r_ = json.loads(line[-1][9:])
                    r_["placement"] = "%d threads pinned to CPUs %d..%d of NUMA node 0 (cpulist %s)" % (th, cpus[0], cpus[-1], node_txt)
                    runs[str(th)] = r_
            except (subprocess.TimeoutExpired, OSError, ValueError):
                pass
    best = min(runs, key=lambda k_: runs[k_]["t_eval_s"])
    rb = runs[best]
    return res, {
        "value": flops_fit(N) / rb["t_eval_s"] * 1e-9, "unit": "GFLOP/s", "cores": int(rb["threads"]) or cores, "host_cores_visible": cores,
        "kind": "port", "best_run": best, "placement": rb["placement"],
        "sample": "one full LML evaluation of the same workload (N=%d) per configuration -- oracle fused K-build (C, OpenMP) + "
                  "scipy.linalg.cholesky + cho_solve (OpenBLAS) -- default threads in this process, then {8,16,32,64} threads pinned "
                  "to one NUMA node in child processes (best of 2 each); quoted: the fastest (%s), %.2f s per evaluation"
                  % (N, best, rb["t_eval_s"]),
        "lml_evals_per_s": 1.0 / rb["t_eval_s"],
        "t_kbuild_cpu_s": rb["t_kbuild_s"], "t_potrf_cpu_s": rb["t_potrf_s"], "t_solve_ll_cpu_s": rb["t_solve_ll_s"],
        "kbuild_GBps_written_cpu": 8.0 * N * N / rb["t_kbuild_s"] * 1e-9,
        "potrf_GFLOPs_cpu": potrf_flops / rb["t_potrf_s"] * 1e-9,
        "runs": {k_: {"threads": v_["threads"], "t_eval_s": v_["t_eval_s"], "t_potrf_s": v_["t_potrf_s"],
                      "potrf_GFLOPs": potrf_flops / v_["t_potrf_s"] * 1e-9, "placement": v_["placement"]} for k_, v_ in runs.items()},
        "note": "a reported baseline, not the optimisation target; `cores` = the threads of the quoted run",
    }


def parity_report(ll, ld, ref, pred_gpu=None, pred_cpu=None):
    """The parity gate of SURVEY.md section 8(d): ll (data term) and sum(log L_ii) within 1e-8 relative of the CPU path,
    predictive mean / std at 64 random points within 1e-6 (sigma_f = 1).  Returns (report, ok)."""
    rep = {"ll_rel_err_vs_cpu": abs(ll - ref["ll_data"]) / abs(ref["ll_data"]),
           "logdet_rel_err_vs_cpu": abs(ld - ref["logdet_half"]) / abs(ref["logdet_half"]),
           "tolerance": 1e-8}
    ok = rep["ll_rel_err_vs_cpu"] <= 1e-8 and rep["logdet_rel_err_vs_cpu"] <= 1e-8
    if pred_gpu is not None:
        (gm, gs), (cm, cs) = pred_gpu, pred_cpu
        rep.update({"predict_mean_max_abs_err": float(np.abs(gm - cm).max()),
                    "predict_std_max_abs_err": float(np.abs(gs - cs).max()),
                    "predict_var_max_abs_err": float(np.abs(gs ** 2 - cs ** 2).max()),
                    "predict_tolerance": 1e-6})
        # (std is gated through the variance: where the data pin the curve the variance is a cancellation residue)
        ok = ok and rep["predict_mean_max_abs_err"] <= 1e-6 and rep["predict_var_max_abs_err"] <= 1e-6
    rep["ok"] = bool(ok)
    return rep, ok


def dist_trace(plan, step):
    """One traced evaluation (device-timeline stamps of gptools_amd.dist): per panel k, when it had arrived on this
    rank's main queue and when its trailing update was done, in ms from the start of the K build; summarised as the
    time spent waiting for panels against the time spent updating."""
    plan.trace = True
    step()
    plan.trace = False
    st = plan.timings.get("steps_ms", [])
    arr = {k: t for k, tag, t in st if tag == "arrived"}
    app = {k: t for k, tag, t in st if tag == "applied"}
    ks = sorted(arr)
    wait = sum(arr[k] - (app[k - 1] if k - 1 in app else arr[k]) for k in ks)
    upd = sum(app[k] - arr[k] for k in ks if k in app)
    return {"first_panel_ms": arr[ks[0]] if ks else None, "waiting_for_panels_ms": wait, "updating_ms": upd,
            "end_ms": app[ks[-1]] if ks else None,
            "arrived_ms": [round(arr[k], 3) for k in ks], "applied_ms": [round(app[k], 3) for k in ks if k in app]}


def comm_probe(torch, dist, world, rank):
    """What the interconnect delivers for the message sizes of the panel exchange (device time per call, averaged over
    5 calls after 2 warm-up calls, max over ranks): broadcast from rank 0, scatter + in-place all-gather, and a
    point-to-point send rank 0 -> rank 1."""
    out = {}
    dev = torch.device("cuda", torch.cuda.current_device())

    def run(fn, reps=5):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        dist.barrier()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        t = torch.tensor([e0.elapsed_time(e1) / reps], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    for mb in (2, 16, 128):
        rows = mb * 256                      # rows of a 512-column fp64 panel chunk: 4 KB per row
        buf = torch.zeros((rows, 512), dtype=torch.float64, device=dev)
        ms = run(lambda: dist.broadcast(buf, src=0))
        out["bcast_%dMB" % mb] = {"ms": ms, "GBps": mb * 1.048576e-3 / (ms * 1e-3)}
        c = rows // world
        pieces = [buf[r * c:(r + 1) * c] for r in range(world)]

        def sag():
            dist.scatter(pieces[rank], scatter_list=pieces if rank == 0 else None, src=0)
            dist.all_gather_into_tensor(buf, pieces[rank])
        ms = run(sag)
        out["scatter_allgather_%dMB" % mb] = {"ms": ms, "GBps": mb * 1.048576e-3 / (ms * 1e-3)}

        def p2p():
            if rank == 0:
                dist.send(buf, dst=1)
            elif rank == 1:
                dist.recv(buf, src=0)
        if world > 1:
            ms = run(p2p)
            out["send_0_to_1_%dMB" % mb] = {"ms": ms, "GBps": mb * 1.048576e-3 / (ms * 1e-3)}
        del buf
    small = torch.zeros((3,), dtype=torch.float64, device=dev)
    out["allreduce_24B_ms"] = run(lambda: dist.all_reduce(small))
    return out


class Watchdog(object):
    """The partitioned path first measures the whole-panel schedule, then tries the newer schedules and runs the
    diagnostics.  None of those later legs has ever run on more than one real GPU: should one of them hang, this timer
    prints the line that is already complete (flagged) and ends the process, on every rank, instead of losing the run."""

    def __init__(self, rank):
        import threading
        self.rank, self.lock, self.done, self.timer = rank, threading.Lock(), False, None
        self.line, self.phase, self._threading = None, "", threading

    def arm(self, seconds):
        self.timer = self._threading.Timer(seconds, self._fire)
        self.timer.daemon = True
        self.timer.start()

    def _fire(self):
        with self.lock:
            if self.done:
                return
            self.done = True
            if self.rank == 0 and self.line is not None:
                self.line["watchdog"] = "timed out during: %s; this is the line that was complete by then" % self.phase
                print(json.dumps(self.line), flush=True)
            # non-zero: a hung leg must be visible to the launcher (torchrun / CI); the complete line is on stdout
            os._exit(3)

    def finish(self):
        """True if the caller may print the final line (the timer has not fired and no longer will)."""
        with self.lock:
            if self.done:
                return False
            self.done = True
        if self.timer is not None:
            self.timer.cancel()
        return True


def self_launch(ngpus):
    """`python bench.py --gpus N` without a launcher: this process starts the N ranks itself -- fresh child processes of
    this same script, one per GPU, with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their environment (what
    torch.distributed.run would set) -- relays rank 0's JSON line and exits with the worst child status.  The parent
    never imports torch or touches HIP (a process that has initialised the GPU must not be the one that forks / execs the
    ranks), and nothing is re-exec'ed: the children are ordinary subprocesses."""
    import signal
    import socket
    import subprocess
    import threading
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    base = dict(os.environ, WORLD_SIZE=str(ngpus), LOCAL_WORLD_SIZE=str(ngpus), MASTER_ADDR="127.0.0.1",
                MASTER_PORT=os.environ.get("MASTER_PORT", str(port)), HSA_ENABLE_IPC_MODE_LEGACY="0")
    one_gpu = bool(os.environ.get("GPT_BENCH_ONE_GPU"))        # (test hook: every rank on cuda:0, with GPT_BENCH_BACKEND=gloo)
    cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]
    procs = []
    for r in range(ngpus):
        env = dict(base, RANK=str(r), LOCAL_RANK="0" if one_gpu else str(r), GROUP_RANK="0")
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=None, text=True, bufsize=1))

    def relay(p, r):
        for line in p.stdout:
            # rank 0's stdout is the bench line; whatever another rank prints goes to stderr, tagged
            if r == 0:
                sys.stdout.write(line)
                sys.stdout.flush()
            else:
                sys.stderr.write("[rank %d] %s" % (r, line))
    threads = [threading.Thread(target=relay, args=(p, r), daemon=True) for r, p in enumerate(procs)]
    for t in threads:
        t.start()
    # a rank that dies leaves the others waiting in a collective: give them a grace period, then end them (exact PIDs)
    grace, first_bad = float(os.environ.get("GPT_BENCH_GRACE_S", "60")), None
    while True:
        codes = [p.poll() for p in procs]
        if all(c is not None for c in codes):
            break
        if first_bad is None and any(c not in (None, 0) for c in codes):
            first_bad = time.time()
        if first_bad is not None and time.time() - first_bad > grace:
            for p in procs:
                if p.poll() is None:
                    p.send_signal(signal.SIGTERM)
            time.sleep(5)
            for p in procs:
                if p.poll() is None:
                    p.kill()
        time.sleep(0.2)
    for t in threads:
        t.join(timeout=5)
    worst = 0
    for c in codes:
        c = 128 - c if c < 0 else c
        worst = max(worst, c)
    sys.exit(worst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default=None, choices=sorted(WORKLOADS))
    ap.add_argument("--nb", type=int, default=0, help="outer block width (0 = default)")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beside the headline: CPU baseline + parity gate, roofline of instrumented steps, "
                         "throughput, plugin API, predict and K-build legs (N=1), C5 / replica / probe / single-GPU legs (N>1)")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the cpu_baseline leg")
    ap.add_argument("--dist", action="store_true", help="use the block-cyclic DistributedLML path even with one rank")
    ap.add_argument("--no-batched", action="store_true", help="with --full, N=1: skip the two-evaluations-in-flight throughput leg")
    ap.add_argument("--no-predict", action="store_true", help="with --full, N=1: skip the predict leg")
    ap.add_argument("--no-gp-api", action="store_true", help="with --full, N=1: skip the GaussianProcess.update_hyperparameters leg")
    ap.add_argument("--no-ref", action="store_true", help="with --full, N>1: skip the single-GPU run of the same workload on rank 0")
    ap.add_argument("--schedule", default=None, help="N>1: fix the layout (1d+bcast, 1d+scatter_gather, grid2x4, ...) instead of tuning")
    ap.add_argument("--no-probe", action="store_true", help="with --full, N>1: skip the step trace and the link probes after the timed region")
    ap.add_argument("--ctx-opt", action="append", default=[], metavar="KEY=VALUE",
                    help="N=1: a gpt_ctx_set_option pair for the timed context (scratch/prof_r06.sh traces with tail_wait=0)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step returned (ll_data, logdet_half and, N=1, alpha) as DIR/<name>.npy, float64")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "RANK" not in os.environ and int(os.environ.get("WORLD_SIZE", "1")) == 1:
        self_launch(args.gpus)          # plain `python bench.py --gpus N`: start the N ranks (never returns)

    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("--gpus %d does not match WORLD_SIZE %d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("GPT_BENCH_BACKEND", "nccl")       # (test hook: gloo ranks sharing one GPU)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)

    from gptools_amd import _lib
    wl = args.workload or ("c3" if world == 1 else "c4")
    kernel, N, d, deriv = WORKLOADS[wl]
    X, n, y, err, params = synth(kernel, N, d, deriv)
    diag_add = 1e2 * sys.float_info.epsilon

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    roof = None
    extra = {}
    elapsed, ll, ld, parallelism = None, None, None, None
    full_eval = (world == 1 and not args.dist)      # the single-GPU step computes and returns alpha (compute_K_L_alpha_ll in full)
    wd = Watchdog(rank)

    def build_out():
        per_step = elapsed / args.steps
        # N = 1: a step is the FULL evaluation incl. alpha (VERDICT r5 #2a), full LAPACK potrf + potrs count.  The partitioned
        # engines (N > 1 / --dist) compute ll only: executed flops (the forward half of potrs), as before.
        value = flops_fit(N, alpha=full_eval) / per_step * 1e-9
        out_ = {
            # (BASELINE.json quotes the metric on N=8192 = the default workload; other workloads carry their own N in the name)
            "metric": METRIC if N == 8192 else METRIC.replace("N=8192", "N=%d" % N), "value": value, "unit": "GFLOP/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": per_step * 1e3, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": "%s: %s kernel, N=%d, d=%d%s, err_y=0.05, sigma_f=1, l=0.3 (BASELINE.json configs)"
                                   % (wl.upper(), {"se": "SquaredExponential", "m52": "Matern52"}[kernel], N, d,
                                      ", last quarter of rows first-derivative observations" if deriv else ""),
                       "N": N, "d": d, "parallelism": parallelism},
            "lml_evals_per_s": 1.0 / per_step,
            "pct_fp64_mfma_peak": 100.0 * value * 1e-3 / (FP64_MFMA_PEAK_TFLOPS * world),
            "ll_data": ll, "logdet_half": ld,
        }
        out_.update(extra)
        if roof is not None:
            out_["roofline"] = roof
        return out_
    if world == 1 and not args.dist:
        ctx = _lib.Context(local_rank)
        # (the second context of the throughput leg is created before the first one runs: streams created after
        # another context has been busy share hardware queues with it on ROCm 7 -- 173 instead of 210 evaluations/s)
        ctx2 = _lib.Context(local_rank) if (args.full and not args.no_batched) else None
        if args.nb:
            ctx.set_option("nb_outer", args.nb)
        for kv_ in args.ctx_opt:
            ctx.set_option(kv_.split("=")[0], int(kv_.split("=")[1]))
        if args.ctx_opt:
            extra["ctx_opt"] = list(args.ctx_opt)
        ctx.set_option("timing", 1)
        ctx.set_data(X, n)

        def step():
            return ctx.fit(KID[kernel], params, 0.0, y, err, diag_add)
        for _ in range(args.warmup):
            ll, ld = step()
        # With --full, the throughput leg (two contexts, two host threads) runs first, inside _lib.concurrent_evaluations():
        # while several chains are in flight the library keeps every look-ahead on event edges (a kernel spinning on a flag word must not
        # share the hardware queues with a second chain: gptools_amd/csrc/api.hip, EvalScope).  The second context then
        # STAYS ALIVE through the timed loop -- as GaussianProcess's pooled context does -- because what decides the schedule
        # is the number of evaluations in flight, not of contexts alive; `flag_schedule` / `live_contexts` below say what ran.
        if ctx2 is not None:
            # Throughput mode (reported beside `value`, never in it): two INDEPENDENT evaluations (different theta, same
            # data) in flight on the GPU, one context + host thread each -- how GaussianProcess.ll_batch /
            # compute_ll_matrix / multi-start MAP run.  One factorisation's latency-bound tail overlaps the other's
            # update-bound head.
            import threading
            ctx2.set_data(X, n)
            ctx.set_option("profile_gemm", 0)
            ctx.set_option("timing", 0)
            pair = [(ctx, params), (ctx2, params * 1.01)]
            for c_, p_ in pair:
                c_.fit(KID[kernel], p_, 0.0, y, err, diag_add)

            def run(c_, p_):
                for _ in range(args.steps):
                    c_.fit(KID[kernel], p_, 0.0, y, err, diag_add)
            th = [threading.Thread(target=run, args=cp) for cp in pair]
            with _lib.concurrent_evaluations():
                barrier()
                tb = time.perf_counter()
                for t_ in th:
                    t_.start()
                for t_ in th:
                    t_.join()
                barrier()
                tb = time.perf_counter() - tb
            extra["batched"] = {"in_flight": 2, "lml_evals_per_s": 2 * args.steps / tb,
                                "value": 2 * args.steps * flops_fit(N) / tb * 1e-9, "unit": "GFLOP/s",
                                "note": "two independent LML evaluations (different hyperparameters) concurrently on one "
                                        "GPU; throughput of multi-start MAP / likelihood grids, not of one MAP chain"}
            del pair, th, c_, p_, t_
            ctx.set_option("timing", 1)
            for _ in range(2):   # (untimed: the first evaluations after the mode change)
                ll, ld = step()
        # ---- the timed region.  A step = ONE FULL evaluation as the reference's compute_K_L_alpha_ll performs it (ref
        # gaussian_process.py:1418-1469; SURVEY 8d "t_fit = kbuild + load + potrf + potrs + ll"): K build with the diagonal loading,
        # blocked Cholesky, z = L^-1 y (the augmented row), log-determinant, the ll scalar AND alpha = L^-T z, computed on the
        # device behind the factorisation (context option eager_alpha) and handed to the host with the call.  `value` counts the
        # full LAPACK potrf + potrs flops.  (Rounds 1-5 timed the evaluation WITHOUT alpha -- what the MAP loop needs -- as the
        # headline; that figure is now the sibling `lazy_alpha`.)
        # The timed region is exactly --steps evaluations, bracketed by barrier + synchronize on both sides; ms_per_step = its
        # time / --steps.
        # The bench's own instrumentation -- HIP events on every >= 1-GFLOP GEMM launch of the main stream (`roofline`) and around
        # the K-build / factorisation phases -- costs 0.13 ms per C3 step (3 %; scratch/instr_ab.py) and is not part of the
        # product: with --full it runs on INSTR_STEPS further evaluations right after the timed region (100-180 timed launches),
        # `roofline.sampled_steps` says how many.
        INSTR_STEPS = 8
        alpha_box = [None]

        def step_full():
            r_ = ctx.fit(KID[kernel], params, 0.0, y, err, diag_add)
            alpha_box[0] = ctx.get_alpha(N)                     # (a host copy: the fit's own synchronisation covered the transfer)
            return r_

        def timed_steps(step_fn):
            """Exactly --steps evaluations; returns (seconds, result of the last one)."""
            barrier()
            t0_ = time.perf_counter()
            for _ in range(args.steps):
                res_ = step_fn()
            barrier()
            return time.perf_counter() - t0_, res_

        ctx.set_option("profile_gemm", 0)
        ctx.set_option("timing", 0)
        ctx.set_option("eager_alpha", 1)
        for _ in range(2):
            ll, ld = step_full()
        edges0_ = ctx.edge_count
        elapsed, (ll, ld) = timed_steps(step_full)
        alpha_eager = alpha_box[0].copy()
        outputs = {"ll_data": ll, "logdet_half": ld, "alpha": alpha_eager}
        extra["flag_edges_per_step"] = (ctx.edge_count - edges0_) / float(args.steps)   # 0: the look-ahead ran on events
        extra["flag_schedule"] = extra["flag_edges_per_step"] > 0
        extra["timed_region"] = {"steps": args.steps, "seconds": elapsed,
                                 "note": "exactly --steps full evaluations between barrier + synchronize, none of them instrumented; "
                                         "ms_per_step and value are their mean"}
        if args.full:
            # instrumented steps (`roofline`, `kbuild_ms`, `potrf_ms`), then the step without alpha (`lazy_alpha`)
            ctx.gemm_profile_read()
            t_instr, tk, tp, n_instr = [], 0.0, 0.0, 0
            for _ in range(INSTR_STEPS):
                ctx.set_option("profile_gemm", 1)
                ctx.set_option("timing", 1)
                ts_ = time.perf_counter()
                step_full()
                t_instr.append(time.perf_counter() - ts_)
                tm_ = ctx.last_timings()
                tk += tm_["kbuild"]
                tp += tm_["potrf"]
                n_instr += 1
                ctx.set_option("profile_gemm", 0)
                ctx.set_option("timing", 0)
            gflops_alg, gms, gcount, gbytes = ctx.gemm_profile_read(with_bytes=True)
            # sibling: the evaluation without alpha (what update_hyperparameters costs in the MAP loop, which never reads alpha);
            # executed flops = potrf + the forward half of potrs
            ctx.set_option("eager_alpha", 0)
            for _ in range(2):
                step()
            per_l = timed_steps(step)[0] / args.steps
            extra["lazy_alpha"] = {"ms_per_step": per_l * 1e3, "value": flops_fit(N, alpha=False) / per_l * 1e-9, "unit": "GFLOP/s",
                                   "pct_fp64_mfma_peak": 100.0 * flops_fit(N, alpha=False) / per_l * 1e-12 / FP64_MFMA_PEAK_TFLOPS,
                                   "lml_evals_per_s": 1.0 / per_l,
                                   "alpha_extra_ms": (elapsed / args.steps - per_l) * 1e3,
                                   "note": "the same step with alpha left to first use (gp.alpha, predict, the analytic gradient): z = L^-1 y "
                                           "and ll only -- the headline of rounds 1-5; flops counted: potrf + the forward half of potrs"}
            ctx.set_option("timing", 1)
            if gcount:
                ach = gflops_alg / (gms * 1e-3) * 1e-12
                import glob
                roof = {"bound": "mfma", "kernel": "gemm_nt_kernel<64,64> (trailing SYRK/GEMM updates >= 1 GFLOP on the main stream)",
                        "achieved": ach, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": ach / FP64_MFMA_PEAK_TFLOPS,
                        "frac_events": ach / FP64_MFMA_PEAK_TFLOPS,
                        "launch_population": "the >= 1 GFLOP launches of the timed steps' own schedule (flag edges: urgent + rest merged, one "
                                             "launch per panel), HIP events on the dispatch packets of the main stream; in the instrumented "
                                             "steps (after the timed region) the main stream's wait for the next panel is a kernel of its own -- "
                                             "the other steps let the update's last workgroup wait (option tail_wait), which a timed launch "
                                             "would report as its own duration (the library drops it while profile_gemm is on; the committed "
                                             "kernel trace is taken with --ctx-opt tail_wait=0 for the same reason)",
                        "launches_per_step": gcount / max(n_instr, 1), "sampled_steps": n_instr,
                        "avg_launch_us": gms * 1e3 / gcount, "flops_per_launch": gflops_alg / gcount,
                        "algorithmic_bytes": gbytes / gcount, "traffic_unit": "bytes/launch"}
                # frac_trace: the same launches' average duration in the committed rocprofv3 --kernel-trace --stats run of this command
                # (scratch/pmc_summary.py writes profiles/rNN_gemm_trace.json beside the summary); traffic: HBM bytes per launch from the
                # committed PMC passes over a REPLAY of the same launch shapes (scratch/gemm_replay.py: a counter pass runs one kernel at a
                # time, so the library cannot keep its flag edges there -- the shapes of a flag-schedule evaluation are logged and replayed
                # one by one): one launch population throughout (VERDICT r5 #2b).
                tr_ = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_gemm_trace.json")))
                if wl == "c3" and tr_:
                    tj_ = json.load(open(tr_[-1]))
                    roof["frac_trace"] = tj_["flops_per_launch"] / (tj_["avg_launch_us"] * 1e-6) * 1e-12 / FP64_MFMA_PEAK_TFLOPS
                    roof["trace_avg_launch_us"] = tj_["avg_launch_us"]
                    roof["trace_flops_per_launch"] = tj_["flops_per_launch"]
                    roof["trace_file"] = tj_.get("trace_file")
                else:
                    roof["frac_trace"] = None
                tf_ = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_gemm_traffic.json")))
                roof["traffic"] = None
                if wl == "c3" and tf_:
                    tj_ = json.load(open(tf_[-1]))
                    if tj_.get("population") == "replay of the flag schedule's launches":
                        roof["traffic"] = tj_["hbm_bytes_per_launch"]
                        roof["traffic_ratio"] = tj_["hbm_bytes_per_launch"] / tj_["algorithmic_bytes_per_launch"]
                        roof["traffic_flops_per_launch"] = tj_["flops_per_launch"]
                        roof["traffic_algorithmic_bytes"] = tj_["algorithmic_bytes_per_launch"]
                        roof["traffic_file"] = os.path.relpath(tf_[-1], ROOT)
                        roof["traffic_note"] = tj_.get("note")
        extra["methodology"] = {"version": 7,
                                "instrumented": ("%d steps after the timed region" % INSTR_STEPS) if args.full else "none (--full only)",
                                "ms_per_step_plain": 1e3 * elapsed / args.steps,
                                "note": "version 7: exactly --steps timed steps, none instrumented; version 6: rounds of --steps repeated to "
                                        "1 s, median round, one instrumented step per two rounds; versions >= 6: a step computes and returns "
                                        "alpha (full compute_K_L_alpha_ll, full LAPACK flop count); versions <= 5: no alpha in the step, "
                                        "executed flops -- compare those with `lazy_alpha`"}
        if args.full:
            extra["methodology"]["ms_per_step_instrumented"] = 1e3 * sum(t_instr) / max(len(t_instr), 1)
        extra["live_contexts"] = 1 if ctx2 is None else 2
        # The same step through the plugin API (north_star's unit: GaussianProcess.update_hyperparameters, ref
        # gaussian_process.py:1332-1416): a GaussianProcess over the same data whose main / pooled contexts ARE the two of this
        # bench -- the same streams and hardware queues as the timed loop above, so the difference is what the Python layer
        # costs (parameter bookkeeping, the log-prior, ctypes) and which schedule the library picks for it.
        if args.full and not args.no_gp_api:
            import warnings
            import gptools_amd as g
            kcls_ = {"se": g.SquaredExponentialKernel, "m52": g.Matern52Kernel}[kernel]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                gp_ = g.GaussianProcess(kcls_(num_dim=d, initial_params=params, param_bounds=[(1e-3, 10.0)] * (d + 1)),
                                        X=X, y=y, err_y=err, n=n)
            gp_._ctx_obj, gp_._ctx_pool, gp_._data_on_device = ctx, ([[ctx2, -1]] if ctx2 is not None else []), True
            ctx.set_option("profile_gemm", 0)      # (what a user of the plugin API runs: no bench events at all, like the timed
            ctx.set_option("timing", 0)            #  steps above)
            for _ in range(2):
                v_ = gp_.update_hyperparameters(params)
            eg_ = ctx.edge_count
            barrier()
            tg_ = time.perf_counter()
            for _ in range(args.steps):
                v_ = gp_.update_hyperparameters(params)
            barrier()
            tg_ = (time.perf_counter() - tg_) / args.steps
            extra["via_gp_api"] = {"call": "GaussianProcess.update_hyperparameters (alpha on first use)", "ms_per_step": tg_ * 1e3,
                                   "ratio_to_lazy_alpha_step": tg_ / per_l,
                                   "flag_edges_per_step": (ctx.edge_count - eg_) / float(args.steps),
                                   "ll_identical_to_c_abi": bool(-v_ - gp_.hyperprior(gp_.params) == ll
                                                                 or abs((-v_ - gp_.hyperprior(gp_.params)) - ll) <= 1e-12 * abs(ll))}
            # ... and with GaussianProcess(eager_alpha=True): the drop-in for users who read gp.alpha after every evaluation -- the
            # headline's step through the plugin API
            gp_.eager_alpha = True
            for _ in range(2):
                v_ = gp_.update_hyperparameters(params)
            barrier()
            ta_ = time.perf_counter()
            for _ in range(args.steps):
                v_ = gp_.update_hyperparameters(params)
            barrier()
            ta_ = (time.perf_counter() - ta_) / args.steps
            a_gpu_ = np.array(gp_.alpha).ravel()
            # alpha alone, device side, on the resident factor: block inverses cached (what predict / gp.alpha pay after a
            # fit) and rebuilt (what every eager evaluation pays)
            ctx.set_option("eager_alpha", 0)

            def alpha_ms(rebuild):
                ts = []
                for _ in range(5):
                    if rebuild:
                        ctx.fit(KID[kernel], params, 0.0, y, err, diag_add)      # a new factor: nothing cached
                    else:
                        ctx.set_option("alpha_invalidate", 1)                    # the substitution again, inverses cached
                    t_ = time.perf_counter()
                    ctx.get_alpha(N)
                    ts.append(time.perf_counter() - t_)
                return 1e3 * min(ts)
            extra["with_alpha"] = {"call": "GaussianProcess(eager_alpha=True).update_hyperparameters + gp.alpha",
                                   "ms_per_step": ta_ * 1e3, "value": flops_fit(N) / ta_ * 1e-9, "unit": "GFLOP/s",
                                   "pct_fp64_mfma_peak": 100.0 * flops_fit(N) / ta_ * 1e-12 / FP64_MFMA_PEAK_TFLOPS,
                                   "ratio_to_ms_per_step": ta_ / (elapsed / args.steps),
                                   "alpha_alone_ms": alpha_ms(True), "alpha_alone_cached_inverses_ms": alpha_ms(False),
                                   "alpha_max_abs_diff_vs_lazy": float(np.abs(a_gpu_ - ctx.get_alpha(N)).max()),
                                   "alpha_max_abs_diff_headline_vs_lazy": float(np.abs(alpha_eager - ctx.get_alpha(N)).max()),
                                   "note": "the headline's step (`value`) through the plugin API; alpha = L^-T z in 2 N / 512 steps against "
                                           "the 512-wide block inverses (one launch, trinv512_kernel), enqueued by the fit itself behind the "
                                           "factorisation (context option eager_alpha), the N doubles landing in pinned memory under the "
                                           "fit's own sync; alpha_alone_*: a separate gpt_get_alpha call after a plain fit"}
            gp_._ctx_obj = gp_._ctx_pool = None
            del gp_
            ctx.set_option("timing", 1)
        # predict leg (SURVEY 8d "Predict (if timed): N^2 M + N M^2"; ref gaussian_process.py:965-1006) on the factor of
        # the last timed step: K* build, mean = K*^T alpha, v = L^-1 K*, then the row norms (std) or the SYRK (cov).
        # Host buffers in and out (Xstar up, mean / std / cov down) are inside the wall time.
        if args.full and not args.no_predict:
            rsp = np.random.RandomState(4096)
            pl = {}
            lib_ = _lib.load()
            for M_, want_, tag in ((64, 1, "M64_std"), (4096, 1, "M4096_std"), (4096, 2, "M4096_cov"),
                                   (4096, 3, "M4096_cov_device_resident"), (4096, 4, "M4096_draw_16_samples")):
                Xs_ = rsp.rand(M_, d)
                ns_ = np.zeros((M_, d), dtype=np.int32)
                if want_ == 3:
                    # cov_out == NULL: the covariance stays in HBM (C ABI directly; mean and std still come back)
                    m_, s_ = np.empty(M_), np.empty(M_)

                    def call_():
                        _lib.check(lib_.gpt_predict(ctx.handle, _lib.dptr(Xs_), _lib.iptr(ns_), M_, 2, None, None,
                                                    _lib.dptr(m_), _lib.dptr(s_), None))
                elif want_ == 4:
                    # draw_sample's device route: the covariance stays in HBM, is factored there (+ 1e3 eps I) and 16 samples
                    # mean + L u come back (gpt_predict with cov_out NULL + gpt_cov_sample)
                    u_ = rsp.randn(M_, 16)

                    def call_():
                        m2_, _, _ = ctx.predict(Xs_, ns_, 2, device_cov=True)
                        return m2_[:, None] + ctx.cov_sample(1e3 * np.finfo(float).eps, u_)
                else:
                    def call_():
                        return ctx.predict(Xs_, ns_, want_)
                call_()
                call_()                      # (the second call finds the pooled pinned result buffer of the first)
                reps_ = 5
                barrier()
                tp0 = time.perf_counter()
                for _ in range(reps_):
                    r_ = call_()
                barrier()
                tp_ = (time.perf_counter() - tp0) / reps_
                fl_ = float(N) * N * M_ + (float(N) * M_ * M_ if want_ >= 2 else 2.0 * N * M_)
                if want_ == 4:
                    fl_ += float(M_) ** 3 / 3.0 + 2.0 * float(M_) * M_ * 16
                pl[tag] = {"M": M_, "ms": tp_ * 1e3, "flops": fl_, "TFLOPs": fl_ / tp_ * 1e-12,
                           "frac_fp64_mfma_peak": fl_ / tp_ * 1e-12 / FP64_MFMA_PEAK_TFLOPS}
            del r_
            pl["note"] = ("wall time of gpt_predict incl. host->device Xstar and device->host results (cov: M^2 doubles = "
                          "134 MB over PCIe at M=4096, written by DMA into a pooled pinned buffer while the SYRK runs; "
                          "device_resident: cov_out = NULL, nothing of size M^2 moves; draw: + M^3/3 Cholesky of that covariance on the device and "
                          "2 M^2 S for 16 samples, only M x 16 doubles come back); flops = N^2 M (triangular solve) + "
                          "N M^2 (cov) or 2 N M (std)")
            extra["predict"] = pl
        if args.full:
            extra["kbuild_ms"] = tk / max(n_instr, 1)
            extra["potrf_ms"] = tp / max(n_instr, 1)
            extra["kbuild_GBps_written"] = (8.0 * N * (N + 1) / 2.0) / (tk / max(n_instr, 1) * 1e-3) * 1e-9
            # the same K build ALONE on the chip (inside a fit the panel stream starts its first diagonal block under it, so
            # the in-fit figure above is the time to the K build's end, not the builder's rate): gpt_dev_kbuild on device
            # buffers, HIP events on the context's stream
            try:
                st_ = torch.cuda.ExternalStream(int(ctx.stream))
                with torch.cuda.stream(st_):
                    dX_ = torch.from_numpy(np.ascontiguousarray(X)).cuda()
                    dn_ = torch.from_numpy(np.ascontiguousarray(n, dtype=np.int32)).cuda()
                    de_ = torch.from_numpy(np.ascontiguousarray(err)).cuda()
                    dK_ = torch.empty((N, N), dtype=torch.float64, device="cuda")
                    lib_ = _lib.load()
                    best_ = 1e9
                    for _ in range(6):
                        e0_, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0_.record(st_)
                        _lib.check(lib_.gpt_dev_kbuild(ctx.handle, KID[kernel], _lib.dptr(params), len(params), dX_.data_ptr(),
                                                       dn_.data_ptr(), N, dX_.data_ptr(), dn_.data_ptr(), N, d, -1, 1, None, 1, 0, 0,
                                                       de_.data_ptr(), 0.0, float(diag_add), dK_.data_ptr(), N))
                        e1_.record(st_)
                        st_.synchronize()
                        best_ = min(best_, e0_.elapsed_time(e1_))
                extra["kbuild_standalone"] = {"ms": best_, "GBps_written": (8.0 * N * (N + 1) / 2.0) / (best_ * 1e-3) * 1e-9,
                                              "frac_hbm": (8.0 * N * (N + 1) / 2.0) / (best_ * 1e-3) * 1e-12 / 6.3,
                                              "note": "lower triangle + fused diagonal, best of 6, alone on the GPU; frac_hbm against 6.3 TB/s "
                                                      "achievable write bandwidth (the same store pattern without arithmetic reaches 5.6 TB/s at this "
                                                      "N; the builder is bound by its arithmetic: DESIGN.md section 7.7)"}
                del dK_
            except Exception as e_:       # (reported, never fatal: the headline line does not depend on it)
                extra["kbuild_standalone"] = {"error": repr(e_)}
        parallelism = "1 GPU, look-ahead on a second HIP stream"
    else:
        from gptools_amd.dist import DistributedLML, GridLML, HipPanelOps
        ops = HipPanelOps(local_rank)
        plans = {}
        plan = None

        # A leg of the partitioned bench is named "<layout>@<nb>": layout = "1d+bcast" / "1d+scatter_gather" (1-D block-cyclic
        # block columns, whole panels, moved by one broadcast or by scatter + all-gather) or "grid<Pr>x<Pc>" (2-D block-cyclic
        # over a process grid, gptools_amd.dist.GridLML: the per-panel column update and solve split over a process column).
        def get_plan(name):
            layout, nb_ = name.split("@")
            nb_ = int(nb_)
            if layout.startswith("grid"):
                # "grid<Pr>x<Pc>[+native]": as below -- "+native" = gpt_plan_run with the plan's own five RCCL communicators
                if name not in plans:
                    gparts_ = layout[4:].split("+")
                    g_ = tuple(int(v) for v in gparts_[0].split("x"))
                    plans[name] = GridLML(X, n, g_, nb=nb_, ops=ops, compiled="native" if (len(gparts_) > 1 or world == 1) else "python")
                return plans[name]
            # "1d+<exchange>[+native]": with "+native" the rank's step loop is replayed by gpt_plan_run (compiled schedule, RCCL
            # called from the library on the plan's own communicator); without it the same op list goes through the Python
            # interpreter and torch.distributed.  World size 1 always takes the native replay (no communicator involved).
            parts_ = layout.split("+")
            native_ = (len(parts_) > 2 and parts_[2] == "native") or world == 1
            key = "1d%s@%d" % ("+native" if native_ else "", nb_)
            if key not in plans:
                plans[key] = DistributedLML(X, n, nb=nb_, ops=ops, compiled="native" if native_ else "python")
            plans[key].exchange = parts_[1]
            return plans[key]

        def step():
            return plan.fit(KID[kernel], params, y, err)

        def timed(nsteps, profile=False):
            if profile:
                ops.ctx_main.set_option("profile_gemm", 1)
                ops.ctx_main.gemm_profile_read()
            barrier()
            t_ = time.perf_counter()
            for _ in range(nsteps):
                r_ = step()
            barrier()
            t_ = time.perf_counter() - t_
            if world > 1:
                tt = torch.tensor([t_], dtype=torch.float64, device="cuda")
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                t_ = float(tt.item())
            if profile:
                # the dominant kernel of the partitioned path: this rank's trailing updates (staircase SYRK/GEMM launches of
                # >= 1 GFLOP on the main queue), HIP events on that queue inside the timed steps -- rank 0's GPU, per-GPU peak
                gfl, gms, gcnt = ops.ctx_main.gemm_profile_read()
                ops.ctx_main.set_option("profile_gemm", 0)
                if gcnt:
                    ach_ = gfl / (gms * 1e-3) * 1e-12
                    roof_box[0] = {"bound": "mfma", "kernel": "gemm_nt_kernel<64,64> (rank 0's staircase trailing updates "
                                   ">= 1 GFLOP, one launch per panel and rank)", "achieved": ach_,
                                   "peak": FP64_MFMA_PEAK_TFLOPS, "peak_note": "per GPU (the job's peak is %d x this)" % world,
                                   "unit": "TFLOP/s", "frac": ach_ / FP64_MFMA_PEAK_TFLOPS, "traffic": None,
                                   "launches_per_step": gcnt / nsteps, "avg_launch_us": gms * 1e3 / gcnt,
                                   "flops_per_launch": gfl / gcnt}
            return t_ / nsteps, r_
        roof_box = [None]

        # (1) The 1-D whole-panel schedule at nb = 512, panels moved by one broadcast -- the one this code base has run longest:
        # W warm-up steps, K timed steps, a complete line.  (2) Only then the other legs -- scatter + all-gather, the process
        # grids of this world size, other block widths -- each run once (communicator set-up) and timed over two evaluations;
        # if the fastest of them beats (1) by more than 3 % it gets its own W warm-up + K timed steps and becomes the line.
        # Everything after (1) runs under the watchdog above (none of it has run on more than one real GPU).  All timings are
        # reported (`schedules_ms`).
        nb0 = args.nb or 512
        base_name = "1d+bcast@%d" % nb0
        if args.schedule:
            base_name = "%s@%d" % (args.schedule, nb0)
        plan = get_plan(base_name)

        def describe(name):
            layout, nb_ = name.split("@")
            if layout.startswith("grid"):
                return "2-D block-cyclic (nb=%s) over a %s process grid: diagonal block -> inverse down the process column -> row " \
                       "slices by GEMM -> row broadcast + column exchange over RCCL" % (nb_, layout[4:])
            return "1-D block-cyclic block columns (nb=%s) over %d ranks, whole panels over RCCL (%s)%s" % (
                nb_, world, layout.split("+")[1], ", compiled schedule replayed by gpt_plan_run" if (layout.endswith("+native") or world == 1) else "")
        for _ in range(args.warmup):
            ll, ld = step()
        per, (ll, ld) = timed(args.steps, profile=True)
        outputs = {"ll_data": ll, "logdet_half": ld}
        roof = roof_box[0]
        elapsed = per * args.steps
        parallelism = describe(base_name)
        tune, failed = {base_name: per * 1e3}, {}
        extra["schedules_ms"] = tune
        extra["schedule"] = base_name
        cpu_ref = None
        if args.full and not args.no_cpu:
            # The CPU path once on the SAME workload, now (before the legs that run under the watchdog), so that the
            # line kept for the watchdog already carries cpu_baseline and parity: rank 0's host cores work, the other
            # ranks wait at the barrier.
            if rank == 0:
                ref_, extra["cpu_baseline"] = cpu_baseline(kernel, X, n, y, err, params, sweep=False)
                cpu_ref = {"ll_data": ref_["ll_data"], "logdet_half": ref_["logdet_half"]}
                del ref_
                extra["parity"] = parity_report(ll, ld, cpu_ref)[0]
            barrier()
        wd.line = build_out()
        wd.phase = "tuning pass over the other schedules"
        wd.arm(float(os.environ.get("GPT_BENCH_WATCHDOG_S", 0)) or 120.0 + 30.0 * per * (args.steps + args.warmup + 20))
        if os.environ.get("GPT_BENCH_FAKE_HANG"):        # (test hook for the watchdog: scratch/README.md)
            time.sleep(3600)
        grids_ = {1: [(1, 1)], 2: [(2, 1), (1, 2)], 4: [(2, 2), (4, 1)], 8: [(2, 4), (4, 2)]}.get(world, [])
        # (the native replay with its own RCCL communicator has run at world size 1 only: on more ranks it is a LEG -- under the
        # watchdog like everything after the first timed region -- and becomes the line only if it completes and is faster)
        # They are OPT-IN (GPT_BENCH_NATIVE_LEGS=1, or --schedule 1d+bcast+native): a hang of an untried path the watchdog can end, a
        # crash it cannot -- and at 8 ranks an evaluation is GPU-bound (45 ms against 2-6 ms of host enqueue either way), so the native
        # replay has nothing to add to THIS number on a first run on hardware.
        native_legs = (world > 1 and os.environ.get("GPT_BENCH_BACKEND", "nccl") == "nccl" and bool(os.environ.get("GPT_BENCH_NATIVE_LEGS")))
        combos = ["1d+scatter_gather@%d" % nb0] + (["1d+bcast+native@%d" % nb0, "1d+scatter_gather+native@%d" % nb0] if native_legs else []) \
            + ["grid%dx%d@%d" % (g_[0], g_[1], nb0) for g_ in grids_] \
            + (["grid%dx%d+native@%d" % (g_[0], g_[1], nb0) for g_ in grids_[:1]] if native_legs else [])
        if not args.nb:
            combos += ["1d+bcast@384", "1d+bcast@256"] + ["grid%dx%d@256" % g_ for g_ in grids_[:1]]
        if args.schedule:
            combos = []
        if world == 1:
            combos = [c_ for c_ in combos if "scatter_gather" not in c_]
        combos.append(base_name)

        def select(name):
            return get_plan(name)
        for name in [k_ for k_ in combos if k_ != base_name]:
            wd.phase = "tuning pass, " + name
            try:
                plan = select(name)
                step()
                tune[name] = timed(2)[0] * 1e3
            except (RuntimeError, ValueError, NotImplementedError) as e:
                # (an error every rank raises alike, e.g. an operation the backend does not offer: skip the combination)
                failed[name] = repr(e)[:200]
        if failed:
            extra["schedules_failed"] = failed
        best = min(tune, key=tune.get)
        plan = select(base_name)
        if best != base_name and tune[best] < 0.97 * tune[base_name]:
            wd.phase = "timed steps of " + best
            plan = select(best)
            for _ in range(args.warmup):
                ll2, ld2 = step()
            roof_keep = roof_box[0]
            per2, (ll2, ld2) = timed(args.steps, profile=True)
            tune[best + " (K timed steps)"] = per2 * 1e3
            if per2 >= per:
                roof_box[0] = roof_keep
            roof = roof_box[0]
            if per2 < per:
                per, ll, ld = per2, ll2, ld2
                outputs = {"ll_data": ll, "logdet_half": ld}
                elapsed = per * args.steps
                parallelism = describe(best)
                extra["schedule"] = best
                wd.line = build_out()
            else:
                plan = select(base_name)
        for k_ in [k_ for k_ in plans if plans[k_] is not plan]:
            del plans[k_]                       # (frees the other block width's matrix and panel buffers)
        torch.cuda.empty_cache()
        wd.phase = "diagnostics after the timed region"
        extra["host_enqueue_ms"] = plan.timings.get("host_enqueue_s", 0.0) * 1e3
        if args.full and (world > 1 or os.environ.get("GPT_BENCH_C5_TOO")) and wl == "c4" and not args.no_probe:
            # SURVEY 8e also asks for the partitioned factorisation at C5's size (N = 16384): same schedule, reported
            # beside the headline (a few evaluations after the timed region; never in `value`)
            try:
                k5, N5, d5, der5 = WORKLOADS["c5"]
                X5, n5, y5, err5, params5 = synth(k5, N5, d5, der5)
                main_plan = plan
                plan5 = (GridLML(X5, n5, (main_plan.Pr, main_plan.Pc), nb=main_plan.nb, ops=ops) if isinstance(main_plan, GridLML)
                         else DistributedLML(X5, n5, nb=main_plan.nb, ops=ops, exchange=main_plan.exchange))
                plan = plan5
                step5 = lambda: plan5.fit(KID[k5], params5, y5, err5)
                step5()
                barrier()
                t5 = time.perf_counter()
                for _ in range(5):
                    ll5, ld5 = step5()
                barrier()
                t5 = (time.perf_counter() - t5) / 5
                if world > 1:
                    tt = torch.tensor([t5], dtype=torch.float64, device="cuda")
                    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                    t5 = float(tt.item())
                extra["c5_partitioned"] = {"N": N5, "ms_per_step": t5 * 1e3, "value": flops_fit(N5) / t5 * 1e-9,
                                           "unit": "GFLOP/s", "pct_fp64_mfma_peak": 100.0 * flops_fit(N5) / t5 * 1e-12
                                           / (FP64_MFMA_PEAK_TFLOPS * world), "ll_data": ll5}
                plan = main_plan
                del plan5
            except (RuntimeError, ValueError) as e:
                plan = main_plan
                extra["c5_partitioned"] = {"error": repr(e)[:200]}
        if args.full and (world > 1 or os.environ.get("GPT_BENCH_C5_TOO")) and not args.no_probe:
            # The other way to use N GPUs (below N ~ 10k a partitioned factorisation cannot beat one
            # GPU): independent evaluations of the metric's own configuration (C3, N = 8192), two in flight per GPU, every
            # rank its own hyperparameters -- aggregate LML evaluations/s of the job (weak scaling; never in `value`).
            try:
                import threading
                k3, N3, d3, der3 = WORKLOADS["c3"]
                X3, n3, y3, err3, p3 = synth(k3, N3, d3, der3)
                pair = [_lib.Context(local_rank), _lib.Context(local_rank)]
                for c_ in pair:
                    c_.set_data(X3, n3)
                    c_.fit(KID[k3], p3, 0.0, y3, err3, diag_add)
                reps = max(10, args.steps)

                def run3(c_, p_):
                    for _ in range(reps):
                        c_.fit(KID[k3], p_, 0.0, y3, err3, diag_add)
                th = [threading.Thread(target=run3, args=(c_, p3 * (1.0 + 0.01 * (2 * rank + i_))))
                      for i_, c_ in enumerate(pair)]
                barrier()
                t3 = time.perf_counter()
                for t_ in th:
                    t_.start()
                for t_ in th:
                    t_.join()
                barrier()
                t3 = time.perf_counter() - t3
                if world > 1:
                    tt = torch.tensor([t3], dtype=torch.float64, device="cuda")
                    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                    t3 = float(tt.item())
                extra["replicas_c3"] = {"N": N3, "in_flight_per_gpu": 2, "lml_evals_per_s": 2 * reps * world / t3,
                                        "value": 2 * reps * world * flops_fit(N3) / t3 * 1e-9, "unit": "GFLOP/s",
                                        "pct_fp64_mfma_peak": 100.0 * 2 * reps * world * flops_fit(N3) / t3 * 1e-12
                                        / (FP64_MFMA_PEAK_TFLOPS * world), "scaling": "weak",
                                        "note": "contexts created after the partitioned run has used the GPU: their streams "
                                                "share hardware queues (about 20 % below the N=1 line's `batched` figure "
                                                "per GPU, DESIGN section 6)"}
                del pair
            except (RuntimeError, ValueError) as e:
                extra["replicas_c3"] = {"error": repr(e)[:200]}
        if args.full and not args.no_probe:
            # after the timed region: where the time of one evaluation goes on rank 0, and what the links deliver
            try:
                extra["trace"] = dist_trace(plan, step)
                if world > 1:
                    extra["comm_probe"] = comm_probe(torch, dist, world, rank)
            except Exception as e:          # diagnostics must never cost the measurement
                extra["probe_error"] = repr(e)[:300]
        # Same workload on ONE GPU (rank 0, single-context path), measured in the same run, so that the speed-up of
        # the partitioned factorisation can be read off this line (the N=1 bench line is a different workload, C3).
        if args.full and (world > 1 or args.dist) and not args.no_ref:
            if rank == 0:
                ctx = _lib.Context(local_rank)
                ctx.set_data(X, n)
                ctx.set_option("timing", 1)
                tref = []
                for _ in range(3):
                    ll1, ld1 = ctx.fit(KID[kernel], params, 0.0, y, err, diag_add)
                    tref.append(ctx.last_timings()["total"])
                extra["single_gpu_same_workload"] = {
                    "ms_per_step": min(tref), "value": flops_fit(N) / min(tref) * 1e-6, "unit": "GFLOP/s",
                    "ll_rel_diff_vs_partitioned": abs(ll1 - ll) / abs(ll1),
                    "note": "context created after the partitioned run has used the GPU (shared hardware queues): a few % "
                            "slower than the same workload in a fresh process (DESIGN section 6: 206-213 ms for C4)"}
                del ctx
            barrier()

    parity_ok = True
    if rank == 0:
        out = build_out()
        out["flops_note"] = (("full LAPACK count, N^3/3 + N^2/2 + N/6 (potrf) + 2 N^2 (potrs): the step computes alpha = K_tot^-1 y and "
                              "hands it to the host, like the reference's compute_K_L_alpha_ll; `lazy_alpha` is the step without alpha "
                              "(executed flops)") if full_eval else
                             ("executed flops: LAPACK potrf count + the forward half of potrs (z = L^-1 y rides along as the augmented "
                              "row); the partitioned engines evaluate ll only"))
        if args.full and not args.no_cpu:
            from oracle import oracle as O
            if world == 1 and not args.dist:
                ref, cb = cpu_baseline(kernel, X, n, y, err, params, workload=WORKLOADS[wl])
                out["cpu_baseline"] = cb
                # parity gate of SURVEY.md section 8(d): ll, sum(log L_ii), predictive mean / std at 64 random points
                rs = np.random.RandomState(64)
                Xs, ns = rs.rand(64, d), np.zeros((64, d), dtype=np.int32)
                ctx.fit(KID[kernel], params, 0.0, y, err, diag_add)
                gm, gs, _ = ctx.predict(Xs, ns, 1)
                cm, cs, _ = O.predict(kernel, params, X, n, ref["L"], ref["alpha"], Xs, ns, want_cov=False)
                out["parity"], parity_ok = parity_report(ll, ld, ref, (gm, gs), (cm, cs))
            else:
                # partitioned line: cpu_baseline was measured right after the first timed leg (same workload, rank 0's
                # host cores); the gate is re-evaluated on the ll / log|K| of the schedule that became the line
                out["parity"], parity_ok = parity_report(ll, ld, cpu_ref)
    if rank == 0 and args.dump_outputs:
        # (the inputs are seeded, so two builds run with the same arguments can be compared output for output)
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name_, v_ in outputs.items():
            np.save(os.path.join(args.dump_outputs, name_ + ".npy"), np.asarray(v_, dtype=np.float64))
    if wd.finish():
        if rank == 0:
            print(json.dumps(out), flush=True)
    if world > 1:
        flag = torch.tensor([0 if parity_ok else 1], dtype=torch.int32, device="cuda")
        dist.broadcast(flag, src=0)                  # (also the barrier the other ranks wait at during rank 0's CPU leg)
        parity_ok = int(flag.item()) == 0
        dist.destroy_process_group()
    if not parity_ok:
        # the gate gates: a line whose numbers differ from the CPU path's is printed (with parity.ok = false) and the
        # run fails
        sys.exit(4)


if __name__ == "__main__":
    main()
