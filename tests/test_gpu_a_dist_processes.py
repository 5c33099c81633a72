"""GPU suite, multi-process part: gptools_amd.dist on real process groups (a 1-rank RCCL group with the collectives
forced on; two gloo ranks sharing cuda:0).  Kept in a file of its own that sorts before test_gpu_parity.py and creates no
HIP context in the pytest process: a parent that holds many CU-masked queues while a child runs the row-chunked schedule
plus RCCL oversubscribes the GPU's hardware queues, and the child then crawls (seconds per evaluation instead of
milliseconds; seen on some boxes only) -- not a situation of the product (one process per GPU), so not one to test in."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


def c3_inputs(N, d):
    from test_gpu_parity import c3_inputs as f
    return f(N, d)


def test_distributed_plan_rccl_single_rank(oracle):
    """The RCCL call pattern of gptools_amd.dist (async panel broadcasts on the ops stream, scalar all-reduces)
    on the one GPU that is available: a 1-rank nccl process group with the collectives forced on."""
    import os
    import subprocess
    import sys
    code = (
        "import faulthandler; faulthandler.dump_traceback_later(150, exit=True)      # a hang reports where\n"
        "import os, sys, numpy as np, torch, torch.distributed as dist\n"
        "sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
        "os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='29517', GPT_DIST_FORCE_COLLECTIVES='1')\n"
        "torch.cuda.set_device(0)\n"
        "dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))\n"
        "from gptools_amd.dist import DistributedLML, GridLML\n"
        "from test_gpu_parity import c3_inputs\n"
        "X, n, y = c3_inputs(1500, 3)\n"
        "plan = DistributedLML(X, n, nb=128, device=0, sag_min_bytes=0)\n"
        "assert plan.force_collectives and plan.lookahead and plan.schedule == 'bcast'\n"
        "grid = GridLML(X, n, (1, 1), nb=128, ops=plan.ops)       # row / column / grid communicators of one rank each\n"
        "assert grid.force_collectives and grid.g_row is not None and grid.g_colx is not None\n"
        "for pl, exch in ((plan, 'bcast'), (plan, 'scatter_gather'), (grid, None), (grid, 'no_lookahead')):\n"
        "    if pl is plan: plan.exchange = exch\n"
        "    else: grid.lookahead = exch is None\n"
        "    print('RESULT', *pl.fit(1, np.array([1.0, 0.3, 0.3, 0.3]), y, 0.05 * np.ones(1500)))\n"
        "    print('RESULT2', *pl.fit(1, np.array([1.0, 0.3, 0.3, 0.3]), y, 0.05 * np.ones(1500)))\n"
        "dist.destroy_process_group()\n" % ((os.path.dirname(os.path.dirname(os.path.abspath(__file__))),) * 2))
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    vals = [l.split()[1:] for l in out.stdout.splitlines() if l.startswith("RESULT")]
    X, n, y = c3_inputs(1500, 3)
    ref = oracle.fit("m52", np.array([1.0, 0.3, 0.3, 0.3]), X, n, y, 0.05 * np.ones(1500), chol="scipy")
    for v in vals:
        assert abs(float(v[0]) - ref["ll_data"]) <= 1e-9 * abs(ref["ll_data"])
        assert abs(float(v[1]) - ref["logdet_half"]) <= 1e-10 * abs(ref["logdet_half"])
    assert len(vals) == 8


@pytest.mark.parametrize("case", ["m52_d3_nb128", "c4_shape_se_d4_nb512"])
def test_distributed_plan_two_ranks_sharing_the_gpu(oracle, case):
    """The product ops under a real two-rank data flow: two gloo ranks, both on cuda:0 (gloo moves CUDA tensors through
    the host): the 1-D whole-panel schedule and the process grids 1 x 2 and 2 x 1 of GridLML.  Exercises what
    a single rank cannot: receiving into panel buffers, waiting for foreign rows / columns from the panel, "recv" and main
    queues, the column exchange, buffer reuse.
    Second case: BASELINE configs[3]'s shape (SquaredExponential, d=4, no derivative rows) at the product block width
    nb=512, N=4100 -- the C4 workload scaled to what two ranks on one GPU finish in seconds."""
    kern, kid, N, d, nb, deriv = {"m52_d3_nb128": ("m52", 1, 2500, 3, 128, True),
                                  "c4_shape_se_d4_nb512": ("se", 0, 4100, 4, 512, False)}[case]
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import faulthandler; faulthandler.dump_traceback_later(150, exit=True)      # a hang reports where\n"
        "import os, sys, numpy as np, torch, torch.distributed as dist\n"
        "sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
        "rank = int(sys.argv[1])\n"
        "os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='29523')\n"
        "torch.cuda.set_device(0)\n"
        "dist.init_process_group('gloo', rank=rank, world_size=2)\n"
        "from gptools_amd.dist import DistributedLML, GridLML\n"
        "from test_gpu_parity import c3_inputs\n"
        "kid, N, d, nb, deriv = %d, %d, %d, %d, %d\n"
        "X, n, y = c3_inputs(N, d)\n"
        "if not deriv: n[:] = 0\n"
        "p = np.concatenate(([1.0], 0.3 * np.ones(d)))\n"
        "plan = DistributedLML(X, n, nb=nb, device=0)\n"
        "for pl in (plan, GridLML(X, n, (1, 2), nb=nb, ops=plan.ops), GridLML(X, n, (2, 1), nb=nb, ops=plan.ops)):\n"
        "    for rep in range(3):\n"
        "        print('RESULT', *pl.fit(kid, p, y, 0.05 * np.ones(N)))\n"
        "dist.destroy_process_group()\n" % (root, root, kid, N, d, nb, int(deriv)))
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=600) for p in procs]
    X, n, y = c3_inputs(N, d)
    if not deriv:
        n[:] = 0
    ref = oracle.fit(kern, np.concatenate(([1.0], 0.3 * np.ones(d))), X, n, y, 0.05 * np.ones(N), chol="scipy")
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]
        vals = [l.split()[1:] for l in so.splitlines() if l.startswith("RESULT")]
        assert len(vals) == 9
        for v in vals:
            assert abs(float(v[0]) - ref["ll_data"]) <= 1e-9 * abs(ref["ll_data"])
            assert abs(float(v[1]) - ref["logdet_half"]) <= 1e-10 * abs(ref["logdet_half"])


def test_grid_four_ranks_sharing_the_gpu(oracle):
    """GridLML on a 2 x 2 process grid through the product ops: four gloo ranks on cuda:0 -- row broadcasts, the inverse of the
    diagonal block down a process column, the head block to everybody and the column exchange all cross rank boundaries, with
    and without look-ahead (what can run of the 2-D layout on a one-GPU box)."""
    root = ROOT
    N, d, nb = 2300, 3, 128
    code = (
        "import faulthandler; faulthandler.dump_traceback_later(400, exit=True)\n"
        "import os, sys, numpy as np, torch, torch.distributed as dist\n"
        "sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
        "rank = int(sys.argv[1])\n"
        "os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='29531')\n"
        "torch.cuda.set_device(0)\n"
        "dist.init_process_group('gloo', rank=rank, world_size=4)\n"
        "from gptools_amd.dist import GridLML\n"
        "from test_gpu_parity import c3_inputs\n"
        "X, n, y = c3_inputs(%d, %d)\n"
        "p = np.concatenate(([1.0], 0.3 * np.ones(%d)))\n"
        "plan = GridLML(X, n, (2, 2), nb=%d, device=0)\n"
        "for la in (True, False, True):\n"
        "    plan.lookahead = la\n"
        "    print('RESULT', *plan.fit(1, p, y, 0.05 * np.ones(%d)))\n"
        "dist.destroy_process_group()\n" % (root, root, N, d, d, nb, N))
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(4)]
    outs = [p.communicate(timeout=900) for p in procs]
    X, n, y = c3_inputs(N, d)
    ref = oracle.fit("m52", np.concatenate(([1.0], 0.3 * np.ones(d))), X, n, y, 0.05 * np.ones(N), chol="scipy")
    allvals = []
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]
        vals = [l.split()[1:] for l in so.splitlines() if l.startswith("RESULT")]
        assert len(vals) == 3
        for v in vals:
            assert abs(float(v[0]) - ref["ll_data"]) <= 1e-9 * abs(ref["ll_data"])
            assert abs(float(v[1]) - ref["logdet_half"]) <= 1e-10 * abs(ref["logdet_half"])
        allvals.append(vals)
    assert all(v == allvals[0] for v in allvals)          # every rank: the same bits


@pytest.mark.parametrize("world", [1, 2, 3])
def test_distributed_schedules_under_queue_jitter(world):
    """Missing-edge detector (tests/dist_jitter_worker.py): the schedules of gptools_amd.dist with random delay kernels
    on every queue must return the same numbers every time -- on 2 and on 3 gloo ranks sharing the GPU, and on one rank
    with the RCCL collectives (both exchanges) forced on."""
    worker = os.path.join(ROOT, "tests", "dist_jitter_worker.py")
    out = subprocess.run([sys.executable, worker, str(world)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=900)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    assert out.stdout.count(": 0 bad of ") == world, out.stdout[-1500:]


def test_gaussian_process_partitioned_update_and_map_two_ranks(oracle):
    """``GaussianProcess.partitioned``: update_hyperparameters / optimize_hyperparameters with the factorisation spread
    over the ranks of the job (two gloo ranks sharing cuda:0) give what one process gives, on every rank; the factor is
    rebuilt locally when predict needs it."""
    root = ROOT
    code = (
        "import faulthandler; faulthandler.dump_traceback_later(200, exit=True)\n"
        "import os, sys, json, warnings, numpy as np\n"
        "warnings.simplefilter('ignore')\n"
        "sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
        "rank, world = int(sys.argv[1]), int(sys.argv[2])\n"
        "if world > 1:\n"
        "    import torch, torch.distributed as dist\n"
        "    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='29527')\n"
        "    torch.cuda.set_device(0)\n"
        "    dist.init_process_group('gloo', rank=rank, world_size=world)\n"
        "import gptools_amd as g\n"
        "from test_gpu_parity import c3_inputs\n"
        "X, n, y = c3_inputs(1200, 2)\n"
        "k = g.Matern52Kernel(num_dim=2, initial_params=[1.0, 0.4, 0.4], param_bounds=[(0.05, 10.0)] * 3)\n"
        "gp = g.GaussianProcess(k, X=X, y=y, err_y=0.05, n=n)\n"
        "gp.partitioned = world > 1\n"
        "gp.partition_block = 128\n"
        "v1 = gp.update_hyperparameters([1.1, 0.35, 0.45])\n"
        "mode1 = gp._fit_mode\n"
        "m1, s1 = gp.predict(X[:5], n=0)\n"
        "mode2 = gp._fit_mode\n"
        "# independent evaluations on a partitioned GP (ADVICE r1): the ranks evaluate DIFFERENT points, so these must\n"
        "# stay local -- one point per rank (len == world) used to enter the collective with mixed hyperparameters\n"
        "grid2, _ = gp.compute_ll_matrix([(0.8, 1.2), (0.4, 0.4), (0.4, 0.4)], [2, 1, 1])\n"
        "b4 = gp.ll_batch([[1.0, 0.3, 0.4], [1.1, 0.35, 0.45], [0.9, 0.4, 0.4], [1.2, 0.3, 0.5]])\n"
        "assert gp.partitioned == (world > 1)\n"
        "res, nres = gp.optimize_hyperparameters(method='L-BFGS-B', random_starts=0, opt_kwargs={'options': {'maxiter': 6}})\n"
        "print('RESULT', json.dumps({'v1': float(v1), 'mode1': mode1, 'mode2': mode2, 'm1': [float(v) for v in m1],\n"
        "                            'grid2': [float(v) for v in grid2.ravel()], 'b4': [float(v) for v in b4],\n"
        "                            'fun': float(res.fun), 'x': [float(v) for v in res.x]}))\n"
        "if world > 1: dist.destroy_process_group()\n") % (root, root)

    def launch(rank, world):
        return subprocess.Popen([sys.executable, "-c", code, str(rank), str(world)], stdout=subprocess.PIPE,
                                stderr=subprocess.PIPE, text=True)

    def result(p):
        so, se = p.communicate(timeout=600)
        assert p.returncode == 0, se[-2000:]
        import json
        return json.loads([l for l in so.splitlines() if l.startswith("RESULT")][0][7:])

    single = result(launch(0, 1))
    procs = [launch(r, 2) for r in range(2)]
    both = [result(p) for p in procs]
    assert single["mode1"] == "kernel"
    for r in both:
        assert r["mode1"] == "partitioned" and r["mode2"] == "kernel"
        assert abs(r["v1"] - single["v1"]) <= 1e-9 * abs(single["v1"])
        np.testing.assert_allclose(r["m1"], single["m1"], rtol=0, atol=1e-8)
        np.testing.assert_allclose(r["grid2"], single["grid2"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(r["b4"], single["b4"], rtol=1e-12, atol=0)
        # The objective VALUES agree to 1e-9 and better (above); the optimiser's path does not: scipy's finite-difference
        # gradients amplify the 1e-13 summation-order difference between the two engines (after the 6 iterations run here:
        # 1.6e-6 in -ll, 1.3e-3 in the parameters; run to convergence the two stop at different points of a flat valley).
        assert abs(r["fun"] - single["fun"]) <= 5e-5 * abs(single["fun"])
        np.testing.assert_allclose(r["x"], single["x"], rtol=5e-2)
    # the two ranks see the SAME collective values at every step: identical trajectories
    assert abs(both[0]["fun"] - both[1]["fun"]) <= 1e-12 * abs(both[0]["fun"])
    np.testing.assert_allclose(both[0]["x"], both[1]["x"], rtol=1e-12)
    assert both[0]["fun"] == both[1]["fun"] and both[0]["x"] == both[1]["x"]      # the ranks walked the same iterates



def test_bench_partitioned_line_is_complete_two_ranks():
    """bench.py --full's N>1 branch end to end -- two gloo ranks sharing cuda:0 (test hook GPT_BENCH_BACKEND), the C2 workload:
    rank 0 prints ONE JSON line that carries `roofline` (HIP-event timing of the staircase updates), `cpu_baseline`
    (with the K-build / potrf split) and a passing `parity` gate; both ranks exit 0."""
    import json
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29531", WORLD_SIZE="2", LOCAL_RANK="0",
               GPT_BENCH_BACKEND="gloo", GPT_BENCH_WATCHDOG_S="500")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "c2", "--steps", "3", "--warmup", "1",
           "--schedule", "bcast+bcast", "--full", "--no-probe", "--no-ref"]
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]
    lines = [l for l in outs[0][0].splitlines() if l.startswith("{")]
    assert len(lines) == 1 and not [l for l in outs[1][0].splitlines() if l.startswith("{")]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["config"]["N"] == 4096 and "watchdog" not in line
    roof = line["roofline"]
    assert roof["bound"] == "mfma" and roof["achieved"] > 0 and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-12
    cb = line["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["t_kbuild_cpu_s"] > 0 and cb["t_potrf_cpu_s"] > 0
    par = line["parity"]
    assert par["ok"] and par["ll_rel_err_vs_cpu"] <= 1e-8 and par["logdet_rel_err_vs_cpu"] <= 1e-8


def test_flag_edges_single_context_bitwise_and_under_jitter():
    """The look-ahead's per-panel dependencies as flag words (EdgeSig: last-workgroup flag + hipStreamWaitValue32 / in-kernel
    wait, api.hip potrf_enqueue) give bit-identical results to the event edges, also with random delays in front of every
    dense launch.  Fresh process: the flags are used only while the context is the only one alive."""
    code = (
        "import faulthandler; faulthandler.dump_traceback_later(300, exit=True)\n"
        "import os, sys, json, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
        "from gptools_amd import _lib\n"
        "from test_gpu_parity import c3_inputs\n"
        "out = {}\n"
        "for N, kid, d in ((2900, _lib.KERNEL_M52, 3), (8192, _lib.KERNEL_M52, 3), (5000, _lib.KERNEL_SE, 2)):\n"
        "    X, n, y = c3_inputs(N, d)\n"
        "    err = np.full(N, 0.05)\n"
        "    p = np.array([1.0] + [0.3] * d)\n"
        "    ctx = _lib.Context(0)\n"
        "    ctx.set_data(X, n)\n"
        "    res = []\n"
        "    for flags in (1, 0, 1, 1):\n"
        "        ctx.set_option('edge_flags', flags)\n"
        "        e0 = ctx.edge_count\n"
        "        ll, ld = ctx.fit(kid, p, 0.0, y, err, 2.2e-14)\n"
        "        L = ctx.get_L(N)\n"
        "        res.append((ll, ld, float(np.abs(L).sum()), ctx.edge_count - e0))\n"
        "    # a factorisation that fails (not positive definite) with the flag edges in use: error, no hang, and the next\n"
        "    # evaluation on the same context is unaffected\n"
        "    ctx.set_option('edge_flags', 1)\n"
        "    try:\n"
        "        ctx.fit(kid, p, 0.0, y, 0.0 * err, -5.0)\n"
        "        failed = False\n"
        "    except np.linalg.LinAlgError:\n"
        "        failed = True\n"
        "    again = ctx.fit(kid, p, 0.0, y, err, 2.2e-14)\n"
        "    res.append((again[0], again[1], res[0][2], 1 if failed else -1))\n"
        "    # the plain factorisation entry (gpt_potrf on a host matrix) through the same look-ahead, flags in use\n"
        "    rs = np.random.RandomState(N)\n"
        "    Ad = rs.randn(1700, 1700); Ad = Ad.dot(Ad.T) + 1700 * np.eye(1700)\n"
        "    e1 = ctx.edge_count\n"
        "    Ld = np.tril(ctx.potrf_host(Ad))\n"
        "    assert ctx.edge_count > e1, 'potrf_host did not use the flag edges'\n"
        "    np.testing.assert_allclose(Ld, np.linalg.cholesky(Ad), rtol=1e-11, atol=1e-11)\n"
        "    out[str(N)] = res\n"
        "    del ctx\n"
        "print('RESULT', json.dumps(out))\n") % (ROOT, ROOT)
    for jitter in (None, "40"):
        env = dict(os.environ)
        env.pop("GPT_EDGE_FLAGS", None)
        if jitter:
            env["GPT_JITTER"] = jitter
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        import json
        out = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT")][0][7:])
        for N, res in out.items():
            assert res[0][3] > 0 and res[2][3] > 0, "flag edges were not in use at N=%s: %r" % (N, res)
            assert res[1][3] == 0
            assert res[-1][3] == 1, "the indefinite matrix did not raise LinAlgError"
            for r in res[1:]:
                assert r[:3] == res[0][:3], (N, jitter, res)


def test_bench_plain_python_gpus_2_self_launches():
    """`python bench.py --gpus 2` with NO launcher (no RANK / WORLD_SIZE in the environment): bench.py starts the two ranks
    itself (bench.self_launch), relays rank 0's one JSON line and exits 0.  Both ranks on cuda:0 over gloo (test hooks
    GPT_BENCH_ONE_GPU / GPT_BENCH_BACKEND), the C2 workload."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(GPT_BENCH_BACKEND="gloo", GPT_BENCH_ONE_GPU="1", GPT_BENCH_WATCHDOG_S="500")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "c2", "--steps", "3", "--warmup", "1",
           "--schedule", "bcast+bcast", "--full", "--no-probe", "--no-ref"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["config"]["N"] == 4096 and line["parity"]["ok"] and line["roofline"]["achieved"] > 0


def _bench_line(args, timeout=900):
    """One single-GPU bench.py run in a fresh process; returns its one JSON line."""
    import json
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, capture_output=True, text=True,
                         timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_single_gpu_line_is_the_headline_only(tmp_path):
    """A plain `bench.py --gpus 1` run times the steps and nothing else: the headline fields, the timed region and the
    dumped outputs of its last timed step -- no CPU baseline, no parity gate, no second context, no instrumented or
    extra legs (those are --full's)."""
    line = _bench_line(["--workload", "c2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert line["metric"].endswith("N=4096") and line["unit"] == "GFLOP/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["value"] > 0 and abs(line["ms_per_step"] - 1e3 * line["timed_region"]["seconds"] / 3) < 1e-9
    assert line["live_contexts"] == 1 and line["methodology"]["version"] == 7
    for key in ("cpu_baseline", "parity", "roofline", "batched", "lazy_alpha", "via_gp_api", "with_alpha", "predict",
                "kbuild_ms", "kbuild_standalone"):
        assert key not in line, key
    assert float(np.load(str(tmp_path / "ll_data.npy"))) == line["ll_data"]
    assert float(np.load(str(tmp_path / "logdet_half.npy"))) == line["logdet_half"]
    alpha = np.load(str(tmp_path / "alpha.npy"))
    assert alpha.shape == (4096,) and np.isfinite(alpha).all()


def test_bench_full_single_gpu_line_is_complete():
    """`bench.py --gpus 1 --full` still runs every leg beside the headline: CPU baseline with a passing parity gate,
    the roofline of the instrumented steps, the throughput, plugin-API, predict and K-build legs."""
    line = _bench_line(["--workload", "c2", "--steps", "3", "--warmup", "1", "--full"])
    assert line["parity"]["ok"] and line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["t_potrf_cpu_s"] > 0
    assert line["roofline"]["achieved"] > 0 and line["roofline"]["sampled_steps"] == 8
    assert line["live_contexts"] == 2 and line["batched"]["lml_evals_per_s"] > 0
    assert line["lazy_alpha"]["ms_per_step"] > 0 and line["via_gp_api"]["ms_per_step"] > 0 and line["with_alpha"]["ms_per_step"] > 0
    assert set(line["predict"]) >= {"M64_std", "M4096_std", "M4096_cov"} and line["kbuild_standalone"]["ms"] > 0
    assert line["methodology"]["ms_per_step_instrumented"] > 0


def _run_fresh(code, env_extra=None, timeout=900):
    env = dict(os.environ)
    env.pop("GPT_EDGE_FLAGS", None)
    env.update(env_extra or {})
    head = ("import faulthandler; faulthandler.dump_traceback_later(%d, exit=True)\n"
            "import os, sys, json, warnings, numpy as np\n"
            "warnings.simplefilter('ignore')\n"
            "sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n" % (timeout - 30, ROOT, ROOT))
    p = subprocess.run([sys.executable, "-c", head + code], capture_output=True, text=True, timeout=timeout, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    import json
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT")][0][7:]), p.stderr


def test_gaussian_process_reaches_the_flag_schedule_by_default():
    """north_star's unit is GaussianProcess.update_hyperparameters: with default settings -- the pooled second context of
    ll_batch alive, the process-wide context of Kernel.__call__ alive -- the evaluation must run the flag-edge schedule the
    bench times (idle contexts do not count, api.hip EvalScope), at the metric's N = 8192; ll_batch (two chains in flight)
    must run on events and leave the flag schedule usable afterwards."""
    code = (
        "import gptools_amd as g\n"
        "from gptools_amd import _lib\n"
        "from test_gpu_parity import c3_inputs\n"
        "X, n, y = c3_inputs(8192, 3)\n"
        "k = g.Matern52Kernel(num_dim=3, initial_params=[1.0, 0.3, 0.3, 0.3], param_bounds=[(1e-3, 10.0)] * 4)\n"
        "k(X[:4], X[:4], n[:4], n[:4])                      # Kernel.__call__: creates the process-wide default context\n"
        "gp = g.GaussianProcess(k, X=X, y=y, err_y=0.05, n=n)\n"
        "v0 = gp.update_hyperparameters([1.0, 0.3, 0.3, 0.3])\n"
        "assert gp._ctx_pool and len(gp._ctx_pool) == 1     # the pooled context exists (batch_concurrency = 2)\n"
        "e0 = gp._ctx.edge_count\n"
        "v1 = gp.update_hyperparameters([1.0, 0.3, 0.3, 0.3])\n"
        "e1 = gp._ctx.edge_count\n"
        "b = gp.ll_batch([[1.0, 0.3, 0.3, 0.3], [1.1, 0.3, 0.3, 0.3], [1.0, 0.33, 0.3, 0.3], [1.0, 0.3, 0.3, 0.27]])\n"
        "e2 = gp._ctx.edge_count\n"
        "v2 = gp.update_hyperparameters([1.0, 0.3, 0.3, 0.3])\n"
        "e3 = gp._ctx.edge_count\n"
        "gp._ctx.set_option('edge_flags', 0)\n"
        "v3 = gp.update_hyperparameters([1.0, 0.3, 0.3, 0.3])\n"
        "print('RESULT', json.dumps({'v': [v0, v1, v2, v3], 'b0': float(b[0]), 'e': [e0, e1, e2, e3, gp._ctx.edge_count]}))\n")
    out, _ = _run_fresh(code)
    e = out["e"]
    assert e[1] - e[0] >= 20, "update_hyperparameters did not run on flag edges: %r" % (e,)
    assert e[2] == e[1], "ll_batch (two chains in flight) must stay on event edges: %r" % (e,)
    assert e[3] - e[2] >= 20 and e[4] == e[3], e
    assert out["v"][0] == out["v"][1] == out["v"][2] == out["v"][3]          # flag and event schedules: bit-identical
    assert -out["b0"] == out["v"][0]


def test_flag_wait_times_out_and_the_evaluation_is_repeated_on_events():
    """Every flag wait is bounded (common.hpp edge_poll): with the head flag withheld once (context option `edge_test_stall`) the
    first leaf times out after 250 ms instead of hanging, the evaluation is repeated on event edges and returns the right
    numbers, and the process stays on events from then on."""
    code = (
        "import time\n"
        "from gptools_amd import _lib\n"
        "from test_gpu_parity import c3_inputs\n"
        "X, n, y = c3_inputs(3000, 3)\n"
        "err, p = np.full(3000, 0.05), np.array([1.0, 0.3, 0.3, 0.3])\n"
        "ctx = _lib.Context(0); ctx.set_data(X, n); ctx.set_option('edge_test_stall', 1)\n"
        "t0 = time.time(); r0 = ctx.fit(1, p, 0.0, y, err, 2.2e-14); t0 = time.time() - t0\n"
        "e0 = ctx.edge_count\n"
        "t1 = time.time(); r1 = ctx.fit(1, p, 0.0, y, err, 2.2e-14); t1 = time.time() - t1\n"
        "e1 = ctx.edge_count\n"
        "ctx.set_option('edge_flags', 0); r2 = ctx.fit(1, p, 0.0, y, err, 2.2e-14)\n"
        "print('RESULT', json.dumps({'r': [r0, r1, r2], 't': [t0, t1], 'e': [e0, e1]}))\n")
    out, err = _run_fresh(code)
    assert out["r"][0] == out["r"][1] == out["r"][2], out
    assert 0.2 < out["t"][0] < 20.0 and out["t"][1] < 0.2, out["t"]
    assert out["e"][1] == out["e"][0], "after a timeout the process must stay on event edges"
    assert "flag-edge wait timed out" in err


def test_fit_with_every_gemm_tile_option_in_a_single_context_process():
    """`tile` = 64 / 32 (one GEMM macro-tile forced for every launch) in a single-context process: with 64 the look-ahead stays on
    flag edges and gives the default's bits; with 32 everywhere (no order tables, no merged launches) the factorisation still
    completes and agrees.  The tile options that went with their kernels in round 6 (65 / 128 / 129) are refused."""
    code = (
        "from gptools_amd import _lib\n"
        "from test_gpu_parity import c3_inputs\n"
        "X, n, y = c3_inputs(2900, 3)\n"
        "err, p = np.full(2900, 0.05), np.array([1.0, 0.3, 0.3, 0.3])\n"
        "ctx = _lib.Context(0); ctx.set_data(X, n)\n"
        "res = {}\n"
        "for tile in (0, 64, 32, 0):\n"
        "    ctx.set_option('tile', tile)\n"
        "    e0 = ctx.edge_count\n"
        "    ll, ld = ctx.fit(1, p, 0.0, y, err, 2.2e-14)\n"
        "    res[str(tile)] = (ll, ld, ctx.edge_count - e0)\n"
        "for tile in (65, 128, 129):\n"
        "    try:\n"
        "        ctx.set_option('tile', tile); res['refused%d' % tile] = False\n"
        "    except Exception:\n"
        "        res['refused%d' % tile] = True\n"
        "print('RESULT', json.dumps(res))\n")
    out, _ = _run_fresh(code)
    ref = out["0"]
    assert ref[2] > 0 and out["64"][2] > 0
    assert out["64"][:2] == ref[:2]
    assert abs(out["32"][0] - ref[0]) <= 1e-10 * abs(ref[0]) and abs(out["32"][1] - ref[1]) <= 1e-11 * abs(ref[1]), out
    assert out["refused65"] and out["refused128"] and out["refused129"]


def test_two_threads_without_the_concurrency_hint_do_not_crawl():
    """Two contexts evaluated from two host threads WITHOUT gpt_concurrency_hint: the library notices the overlap itself (an
    evaluation that starts while a flag-mode one is in flight waits for it, then both run on events): right numbers, and
    nothing near the 0.8 s per evaluation of the queue-oversubscription crawl."""
    code = (
        "import threading, time\n"
        "from gptools_amd import _lib\n"
        "from test_gpu_parity import c3_inputs\n"
        "X, n, y = c3_inputs(4096, 2)\n"
        "n[:] = 0\n"
        "err, p = np.full(4096, 0.05), np.array([1.0, 0.3, 0.3])\n"
        "cs = [_lib.Context(0), _lib.Context(0)]\n"
        "for c in cs: c.set_data(X, n)\n"
        "ref = cs[0].fit(0, p, 0.0, y, err, 2.2e-14)\n"
        "cs[1].fit(0, p, 0.0, y, err, 2.2e-14)\n"
        "res = [[], []]\n"
        "def run(i):\n"
        "    for _ in range(60): res[i].append(cs[i].fit(0, p, 0.0, y, err, 2.2e-14))\n"
        "th = [threading.Thread(target=run, args=(i,)) for i in range(2)]\n"
        "t = time.time()\n"
        "for x in th: x.start()\n"
        "for x in th: x.join()\n"
        "t = time.time() - t\n"
        "ok = all(r == ref for rr in res for r in rr)\n"
        "e_thr = [c.edge_count for c in cs]\n"
        "time.sleep(0.25)\n"
        "cs[0].fit(0, p, 0.0, y, err, 2.2e-14)\n"
        "e_after = cs[0].edge_count - e_thr[0]\n"
        "t1 = time.time()\n"
        "for _ in range(60): cs[0].fit(0, p, 0.0, y, err, 2.2e-14)\n"
        "t1 = time.time() - t1\n"
        "print('RESULT', json.dumps({'ok': ok, 't': t, 'edges_threads': e_thr, 'edges_after': e_after, 't_one': t1}))\n")
    out, _ = _run_fresh(code)
    assert out["ok"]
    assert out["t"] < 3.0, "120 evaluations at N=4096 took %.2f s" % out["t"]
    # the overlap is noticed: after the first hand-over the two threads run side by side on event edges (a flag-mode evaluation
    # raises ~31 edges at this size: 60 of them would be ~1900 per context) instead of taking turns on flags ...
    assert max(out["edges_threads"]) < 600, out
    assert out["t"] < 1.8 * out["t_one"], out          # ... i.e. 2 x 60 evaluations in under twice the time of 60 (measured 1.3 x)
    # ... and a lone evaluation a moment later is back on the flag schedule
    assert out["edges_after"] > 0, out


def test_flag_edges_across_xcds_with_stale_l2_lines():
    """The flag-edge protocol of common.hpp ("memory model") under the conditions it is built for: producer
    and waiter on DIFFERENT XCDs (both launches are large; only workgroups that find themselves on XCD 0 / XCD 1 take part; the
    XCC ids of the working workgroups are checked), the waiter's L2 pre-warmed with stale lines of the payload before
    the flag goes up, 10^4 hand-overs per form, every word checked (gptools_amd/csrc/test_aids/edge_stress.hip, which uses the
    product's edge_signal / edge_poll and the product's store / load forms).  The three forms the library uses must never see a
    stale word; with the write-through stores or the acquire compiled out the same harness must SHOW stale words -- otherwise
    it would not be testing anything."""
    import ctypes
    so = os.path.join(ROOT, "gptools_amd", "csrc", "build", "libedge_stress.so")
    assert os.path.exists(so), "run __graft_entry__.build() (make -C gptools_amd/csrc edge_stress)"
    code = (
        "import ctypes, json, sys\n"
        "lib = ctypes.CDLL(%r)\n"
        "lib.edge_stress_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)]\n"
        "res = {}\n"
        "for mode, iters in ((0, 10000), (1, 10000), (4, 10000), (2, 2000), (3, 2000)):\n"
        "    out = (ctypes.c_longlong * 8)()\n"
        "    rc = lib.edge_stress_run(mode, iters, 1 << 16, 8, out)\n"
        "    res[str(mode)] = [rc] + list(out)[:5]\n"
        "print('RESULT', json.dumps(res))\n" % so)
    out, _ = _run_fresh(code, timeout=900)
    for mode in ("0", "1", "4", "2", "3"):
        rc, xp, xc, bad_iters, bad_words, timed_out = out[mode]
        assert rc == 0 and timed_out == 0, (mode, out[mode])
        # placement: the working workgroups of the producer all on ONE XCD, those of the consumer all on ANOTHER one
        assert xp and xc and xp & (xp - 1) == 0 and xc & (xc - 1) == 0 and xp != xc, "XCC id masks %#x / %#x" % (xp, xc)
    for mode in ("0", "1", "4"):            # the library's three consumer forms: never a stale word
        assert out[mode][3] == 0 and out[mode][4] == 0, (mode, out[mode])
    # negative controls.  (3) the producer's write-through stores compiled out (plain stores, flag raised all the same): the
    # harness MUST show stale words -- round 4: all 2000 hand-overs, 2.5 million words -- or it is not testing anything.  (2) the
    # consumer's acquire compiled out (plain loads behind the poll): reported, not asserted -- on this MI355X no stale word was
    # seen in 2000 hand-overs (a clean line pre-warmed in the waiter's L2 was not served stale); the acquire stays, argued
    # from the memory model
    assert out["3"][3] > 0 and out["3"][4] > 0, "plain (write-back) stores were visible across XCDs without a release: %r" % (out["3"],)
    print("negative controls: no-acquire plain loads: %d stale words in 2000 hand-overs; plain stores: %d stale words in %d of 2000"
          % (out["2"][4], out["3"][4], out["3"][3]))
    sys.stderr.write("edge stress result: %r\n" % (out,))
