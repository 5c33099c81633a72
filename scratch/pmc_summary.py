"""Summarise the rocprofv3 CSV outputs of scratch/prof_all.sh into profiles/ (per round)."""
import csv, collections, re, sys, json
src, out = sys.argv[1], sys.argv[2]
def short(n): return re.sub(r'\(.*', '', n).replace('void ', '')
lines = []
# kernel stats
rows = list(csv.DictReader(open(src + '/trace/t_kernel_stats.csv')))
lines.append("# rocprofv3 --kernel-trace --stats --output-format csv -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu --no-batched   (C3: Matern52, N=8192, d=3)")
lines.append("%-44s %7s %14s %12s %10s %10s %7s" % ("kernel", "calls", "total_ns", "avg_ns", "min_ns", "max_ns", "%"))
for r in rows:
    lines.append("%-44s %7s %14s %12.0f %10s %10s %7s" % (short(r['Name'])[:44], r['Calls'], r['TotalDurationNs'], float(r['AverageNs']), r['MinNs'], r['MaxNs'], r['Percentage']))
bench = [l for l in open(src + '/trace.log') if l.startswith('{')]
if bench: lines.append("\n# bench.py line of the traced run:\n" + bench[-1].strip())
# cross-check of bench.py's roofline.avg_launch_us (HIP events around the >= 1 GFLOP trailing updates) with the trace:
# the same launches are the gemm_nt_kernel dispatches of the main queue with >= 1 GFLOP worth of 64x64 tiles
try:
    K_OUTER_ = 384
    MIN_GRID_ = -(-10**9 // (2 * K_OUTER_ * 64 * 64)) * 256
    kt = list(csv.DictReader(open(src + '/trace/t_kernel_trace.csv')))
    mq = [r['Queue_Id'] for r in kt if 'kbuild_kernel' in r['Kernel_Name']][0]
    bigd = [int(r['End_Timestamp']) - int(r['Start_Timestamp']) for r in kt
            if 'gemm_nt_kernel' in r['Kernel_Name'] and '64, 64' in r['Kernel_Name'] and r['Queue_Id'] == mq
            and int(r['Grid_Size_X']) >= MIN_GRID_]
    bl = json.loads(bench[-1])
    lines.append("\n# dominant kernel, the launches bench.py's roofline times (gemm_nt_kernel on the main queue, Grid_Size >= %d): "
                 "%d dispatches in the trace (all %d evaluations of the run), average %.1f us;  bench.py (HIP events, the %d timed "
                 "evaluations): roofline.avg_launch_us = %.1f" % (MIN_GRID_, len(bigd), round(len(bigd) / bl['roofline']['launches_per_step']), sum(bigd) / len(bigd) * 1e-3,
                                                                 bl['steps'], bl['roofline']['avg_launch_us']))
except Exception as e:
    lines.append("# (cross-check skipped: %r)" % (e,))
def agg(path):
    rows = list(csv.DictReader(open(path)))
    acc = collections.defaultdict(lambda: collections.defaultdict(float)); cnt = collections.Counter(); seen = set()
    for r in rows:
        k = short(r['Kernel_Name']); acc[k][r['Counter_Name']] += float(r['Counter_Value'])
        if (r['Dispatch_Id'], k) not in seen:
            seen.add((r['Dispatch_Id'], k)); cnt[k] += 1
            acc[k]['_dur_ns_' + path.split('/')[-2]] += float(r['End_Timestamp']) - float(r['Start_Timestamp'])
    return acc, cnt
lines.append("\n# PMC passes (separate runs, rocprofv3 --kernel-trace --pmc <...> -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu --no-batched; 3 LML evaluations each)")
res = {}
for name in ('pmc_fetch', 'pmc_write', 'pmc_sq'):
    acc, cnt = agg(src + '/' + name + '/t_counter_collection.csv')
    for k in acc:
        res.setdefault(k, {'dispatches': cnt[k]}).update(acc[k])
for k, v in sorted(res.items(), key=lambda kv: -kv[1].get('SQ_BUSY_CYCLES', 0)):
    d = v['dispatches']
    s = "%-28s disp %4d" % (k[:28], d)
    if 'FETCH_SIZE' in v: s += "  FETCH_SIZE %.4g KB (x2 gfx950 correction -> %.4g GB)" % (v['FETCH_SIZE'], 2 * v['FETCH_SIZE'] * 1024 / 1e9)
    if 'WRITE_SIZE' in v: s += "  WRITE_SIZE %.4g KB (%.4g GB)" % (v['WRITE_SIZE'], v['WRITE_SIZE'] * 1024 / 1e9)
    if v.get('_dur_ns_pmc_sq') and 'SQ_VALU_MFMA_BUSY_CYCLES' in v:
        s += "  MFMA-busy %.1f%% (SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x 2.4 GHz x kernel time in that pass))" % (
            100 * v['SQ_VALU_MFMA_BUSY_CYCLES'] / (1024 * 2.4 * v['_dur_ns_pmc_sq']))
    if v.get('SQ_LDS_IDX_ACTIVE'): s += "  LDS conflict cycles %.1f%%" % (100 * v.get('SQ_LDS_BANK_CONFLICT', 0) / v['SQ_LDS_IDX_ACTIVE'])
    if 'SQ_INSTS_VALU_MFMA_MOPS_F64' in v: s += "  MFMA f64 flops %.4g" % (v['SQ_INSTS_VALU_MFMA_MOPS_F64'] * 512)
    lines.append(s)
open(out, 'w').write("\n".join(lines) + "\n")
print("\n".join(lines))

# ---- HBM traffic per large trailing-update launch (the launches bench.py's roofline line times: >= 1 GFLOP, i.e. the
# rank-512 updates on the main stream's queue with >= 240 workgroups) ----
K_OUTER = 384            # outer block width the library picks at N=8192
MIN_GRID = -(-10**9 // (2 * K_OUTER * 64 * 64)) * 256     # threads of a launch with >= 1 GFLOP (64x64 tiles, 256 threads)
def big_launch_bytes(path, counter):
    rows = list(csv.DictReader(open(path)))
    mainq = [r['Queue_Id'] for r in rows if 'kbuild_kernel' in r['Kernel_Name']][0]
    per = collections.defaultdict(float)
    for r in rows:
        # (the 64x64-tile kernel only: the 32x32 variant of the small launches has four times the threads per tile)
        if r['Counter_Name'] == counter and 'gemm_nt_kernel' in r['Kernel_Name'] and '64, 64' in r['Kernel_Name'] \
                and r['Queue_Id'] == mainq and int(r['Grid_Size']) >= MIN_GRID:
            per[r['Dispatch_Id']] += float(r['Counter_Value'])
    return len(per), sum(per.values()) * 1024.0
# algorithmic flops / bytes of THE SAME launches: the library logged their shapes (GPT_GEMM_LOG, api.hip gemm_nt) during the
# FETCH_SIZE pass, in launch order -- C read + written once (16 B per computed element) + the operand panel once (the B rows of a
# trailing update are a subset of its A rows: 8 k max(m, n) bytes)
ALG = {}
try:
    shapes = [l.split() for l in open(src + '/pmc_fetch_gemm_shapes.txt') if l.strip()]
    shapes = [x for x in shapes if len(x) < 6 or int(x[5]) == 1]       # (those that ran the 64x64 kernel the counter filter selects)
    fl = [float(x[4]) for x in shapes]
    by = [16.0 * float(x[4]) / (2.0 * float(x[2])) + 8.0 * float(x[2]) * max(float(x[0]), float(x[1])) for x in shapes]
    ALG = {"logged_launches": len(shapes), "flops_per_launch": sum(fl) / len(fl), "algorithmic_bytes_per_launch": sum(by) / len(by),
           "algorithmic_note": "shapes of the measured launches themselves (GPT_GEMM_LOG during the FETCH_SIZE pass): 16 B per computed "
                               "element of C + the operand panel once"}
except Exception as e:
    ALG = {"algorithmic_note": "no shape log: %r" % (e,)}
nf, fb = big_launch_bytes(src + '/pmc_fetch/t_counter_collection.csv', 'FETCH_SIZE')
nw, wb = big_launch_bytes(src + '/pmc_write/t_counter_collection.csv', 'WRITE_SIZE')
tj = {"round": int(sys.argv[4]) if len(sys.argv) > 4 else 2, "kernel": "gemm_nt_kernel<64,64>",
      "launch_filter": "main-stream queue, Grid_Size >= %d threads (the >= 1 GFLOP rank-%d trailing updates)" % (MIN_GRID, K_OUTER),
      "launches": nf, "launches_per_evaluation": round(nf / 3.0, 1),
      "note": "counter collection runs one kernel at a time, so the library falls back to event edges there (api.hip, EvalScope): these are the launches of the EVENT schedule (urgent and rest separate); the timed bench line runs the flag schedule with urgent + rest merged: bytes per launch scale with the flops per launch, the ratio to the algorithmic bytes is what carries over", "fetch_bytes_per_launch_x2_corrected": 2 * fb / nf, "write_bytes_per_launch": wb / nw,
      "hbm_bytes_per_launch": 2 * fb / nf + wb / nw,
      **ALG, "ratio": ((2 * fb / nf + wb / nw) / ALG["algorithmic_bytes_per_launch"]) if "algorithmic_bytes_per_launch" in ALG else None,
      "launch_count_matches_log": (ALG.get("logged_launches") == nf),
      "source": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes, scratch/prof_all.sh); FETCH_SIZE doubled per the gfx950 note of MI355X_MICROARCH.md"}
if len(sys.argv) > 3:
    json.dump(tj, open(sys.argv[3], 'w'), indent=1)
print(json.dumps(tj, indent=1))
