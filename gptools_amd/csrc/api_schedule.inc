// api_schedule.inc -- part of api.hip (ONE translation unit: included from there, in this order; the parts share struct gpt_ctx and
// static helpers).  The factorisation: GEMM driver, flag-edge policy (EvalScope), panels, the look-ahead schedule potrf_enqueue / potrf_run.
// ------------------------------------------------------------------------------------------------
// Dense drivers on device data
// ------------------------------------------------------------------------------------------------
#define GPT_PANEL_PRIO 2           // wave priority (0..3) of the panel stream's GEMM main loops
static int gemm_nt(gpt_ctx *c, hipStream_t st, int64_t m, int64_t n, int64_t k, double alpha, const double *A,
                   int64_t lda, const double *B, int64_t ldb, double beta, double *C, int64_t ldc, int tri,
                   hipEvent_t done = nullptr, EdgeSig edge = EdgeSig(), EdgeSig wait = EdgeSig(), int64_t edge_cols = 0,
                   EdgeSig tail = EdgeSig(), int64_t m_live = -1)
{
    // algorithmic flop count: 2k per computed element of C (lower trapezoid when tri)
    // (m_live, launch_gemm_nt: the rows the result needs -- the padding rows of a fit's factor are not computed and not counted;
    // with fewer live rows than columns the trapezoid ends inside its triangle)
    const int64_t ml = (tri && m_live >= 0 && m_live < m) ? m_live : m;
    const double elems = !tri ? (double)m * (double)n
                         : ml >= n ? 0.5 * (double)n * (double)(n + 1) + (double)(ml - n) * (double)n
                                   : 0.5 * (double)ml * (double)(ml + 1);
    const double flops = 2.0 * (double)k * elems;
    // (the roofline line of bench.py: the trailing updates on the MAIN stream only -- at large N the panel and helper
    // streams also launch >= 1 GFLOP updates, on the few CUs reserved for them and concurrently with these; summing their
    // durations with the main stream's would count the same wall time twice)
    const bool on_main = st == c->stream;
    const bool prof = c->prof_gemm && flops >= 1.0e9 && on_main;
    gpt_ctx::GemmProf *gp = nullptr;
    if (prof) {
        if (c->gprof_used == c->gprof.size()) {
            gpt_ctx::GemmProf g;
            GPT_HIP_CHECK(hipEventCreate(&g.e0));
            GPT_HIP_CHECK(hipEventCreate(&g.e1));
            g.flops = 0;
            g.stop = g.e1;
            c->gprof.push_back(g);
        }
        gp = &c->gprof[c->gprof_used++];
        gp->flops = flops;
        // algorithmic bytes of the launch: C read and written once (16 B per computed element) + the operand panel once (the B rows
        // of a trailing update are a subset of its A rows: 8 k max(m, n) bytes) -- SURVEY 8d's per-unit figure for this kernel
        gp->bytes = 16.0 * elems + 8.0 * (double)k * (double)(tri ? ml : (m > n ? m : n));
    }
    // trailing updates on the main stream leave room on every CU for the panel stream (see gemm.hip)
    const int lds_pad = on_main ? (c->lookahead ? c->gemm_pad : (int)c->dev_gemm_pad) : 0;
    // `done` (a cross-stream edge) and the timing events ride on the dispatch packet itself where possible
    // (hipExtLaunchKernelGGL): a separate hipEventRecord is a barrier packet, ~6 us of command-processor time
    const bool ext = !c->use_graph && (c->tile == 0 || c->tile == 64);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ext) {
        e0 = prof ? gp->e0 : nullptr;
        e1 = done ? done : (prof ? gp->e1 : nullptr);
        if (prof) gp->stop = e1;
    } else if (prof) {
        gp->stop = gp->e1;
        GPT_HIP_CHECK(hipEventRecord(gp->e0, st));
    }
    // GPT_GEMM_LOG=<file> (evidence aid, scratch/collect_r04.sh): the shape of every >= 1 GFLOP main-stream launch, in launch order, and
    // whether it runs the 64x64 kernel (launch_gemm_nt cuts launches under gemm_small_threshold() tiles into 32x32 tiles unless a
    // start event or a partial edge rides on them), so that a profiler's per-dispatch counters of that kernel can be set against
    // the algorithmic flops / bytes of THE SAME launches
    {
        static FILE *glog = getenv("GPT_GEMM_LOG") ? fopen(getenv("GPT_GEMM_LOG"), "a") : nullptr;
        if (glog && flops >= 1.0e9 && on_main) {
            const int64_t nt64 = ((m + 63) / 64) * ((n + 63) / 64);
            const int k64 = (c->tile == 64) || !(c->tile == 0 && nt64 < gemm_small_threshold() && !e0 && edge_cols == 0);
            fprintf(glog, "%lld %lld %lld %d %.6e %d\n", (long long)ml, (long long)n, (long long)k, tri, flops, k64);
            fflush(glog);
        }
    }
    // the panel stream's updates keep a raised wave priority (0..3) in their main loop (see gemm.hip)
    // (option gemm_prio >= 0: every GEMM of this context -- the panel-side context of the block-cyclic engine, whose
    // launches all sit on the chain)
    const int prio = (c->gemm_prio >= 0) ? (int)c->gemm_prio : (!on_main && c->lookahead) ? GPT_PANEL_PRIO : 0;
    int rc = launch_gemm_nt(st, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, tri, c->tile, lds_pad, e0, e1, prio, edge, wait, edge_cols, 1, 0, tail,
                            -1, -1, ml < m ? ml : -1);
    if (!ext) {
        if (prof) GPT_HIP_CHECK(hipEventRecord(gp->e1, st));
        if (done) GPT_HIP_CHECK(hipEventRecord(done, st));
    }
    return rc;
}

// Outer block width of the factorisation.  Measured on MI355X (scratch/nb_sweep.py, with the fused diagonal-block + TRSM
// kernel): 256 below N ~ 5k (N=4096: 1.82 ms against 1.86 at 384, 1.90 at 512), 384 while the panel chain dominates
// (N=8192: 5.61 ms against 5.84 at 256 and 5.82 at 512), 512 once the trailing updates do (N=16384: 30.2 ms against
// 30.9 at 384 and 31.2 at 640).
static inline int64_t outer_width(const gpt_ctx *c, int64_t n)
{
    if (c->nb_outer > 0) return c->nb_outer;
    // (round 2, with the helper stream at its measured rate: 640 against 512 gains 1 % at N = 16384, 0.5 % at 32768)
    return (n <= 5120) ? 256 : (n <= 12288) ? 384 : 640;
}

// ------------------------------------------------------------------------------------------------
// When may an evaluation run its look-ahead on flag edges (EdgeSig, common.hpp)?
// ------------------------------------------------------------------------------------------------
// A kernel that waits for a flag holds its hardware queue's slot.  With two evaluations in flight in one process (two
// contexts in two host threads: GaussianProcess.ll_batch, the `batched` leg of bench.py) the streams of both plus the
// runtime's own can exceed the hardware queues the firmware keeps resident; the queue of the kernel that would raise the
// flag is then scheduled out behind the waiter and every hand-over costs a scheduling quantum: measured 0.8 s per evaluation
// instead of 1.3 ms at N = 4096, intermittently (scratch/stress_flags.py).  Event edges do not spin and are immune.
// What decides is therefore not how many contexts EXIST (an idle context's streams cost nothing: GaussianProcess keeps a
// pooled second context for ll_batch, Kernel.__call__ a process-wide one) but how many evaluations are IN FLIGHT:
//   * an evaluation (EvalScope, below) takes the flag edges only if it is the only one in flight in the process when it
//     starts, nobody has announced concurrent evaluations (gpt_concurrency_hint: ll_batch and bench.py bracket their
//     threaded sections with it), the context owns its streams, and the process has not tripped a flag timeout;
//   * an evaluation that starts while a flag-mode evaluation is in flight first waits for that one to end, and the process
//     then stays on event edges while un-announced evaluations keep overlapping (every overlapping start re-arms a 100 ms
//     window; without it two un-hinted threads would take turns, each alone at its start and on flags, the other waiting:
//     one at a time).  Measured, two contexts in two threads at N = 4096: 990-1176 evaluations/s un-hinted, 1147-1168 hinted,
//     765 from one thread (scratch/two_thread_modes.py); a lone evaluation 100 ms later is back on flags;
//   * every wait is bounded (common.hpp); a timeout -- queues oversubscribed by ANOTHER process on the same GPU, a tool that
//     serialises kernels and is not recognised below -- ends the evaluation with an internal status, the process goes to
//     event edges for good (g_flags_tripped) and the evaluation is repeated (fit_terms / gpt_fit_matrix).
// Not usable at all: under rocprofv3 counter collection (ROCPROF_COUNTER_COLLECTION: one kernel at a time -- a --pmc pass
// once hung until the box's limit; with bounded waits it would crawl instead), with GPT_EDGE_FLAGS=0 (the documented switch
// for jobs that share a GPU between processes), under graph capture, on a caller-supplied stream (its other work is
// invisible to the accounting above).
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
static std::mutex g_eval_mu;
static std::condition_variable g_eval_cv;
static int g_evals = 0;                 // evaluations in flight in this process
static int g_flag_evals = 0;            // ... of which on flag edges (0 or 1)
static int g_announced = 0;             // gpt_concurrency_hint depth
static std::atomic<bool> g_flags_tripped{false};
static std::chrono::steady_clock::time_point g_contention_until;   // (under g_eval_mu) overlapping evaluations seen recently: no flags before
#define GPT_I_EDGE_TIMEOUT (-100)       // internal status of an evaluation whose flag wait timed out (never leaves the library)

static bool edge_flags_env_ok()
{
    static int flags_ok = -1;
    if (flags_ok < 0) {
        const char *e = getenv("GPT_EDGE_FLAGS"), *r = getenv("ROCPROF_COUNTER_COLLECTION");
        flags_ok = !((e && atoi(e) == 0) || (r && r[0] && r[0] != '0' && r[0] != 'F' && r[0] != 'f'));
    }
    return flags_ok != 0;
}

// One synchronous evaluation (K build + factorisation + reduction, ends with the streams drained): decides c->flags_now.
// never_flags: work that is in flight like an evaluation but has no flag edges of its own (gpt_fit_batch, gpt_cov_sample): it
// is COUNTED (a flag-mode evaluation started meanwhile sees it and stays on events) but never takes the flag-mode slot itself
// -- holding it would make every other thread's evaluation wait out the whole batch in the constructor below (ADVICE r3).
struct EvalScope {
    gpt_ctx *c;
    bool flags;
    explicit EvalScope(gpt_ctx *c_, bool never_flags = false) : c(c_), flags(false)
    {
        std::unique_lock<std::mutex> lk(g_eval_mu);
        const auto now = std::chrono::steady_clock::now();
        if (never_flags) {
            // (a flag-mode evaluation must be alone: this work fills all 256 CUs from the unmasked panel stream, and kernels that
            // spin on flags beside it would run into their bounded waits, repeat the evaluation and put the process on event edges
            // for good -- so it WAITS for one in flight like any other evaluation; it only never takes the flag-mode slot.  ADVICE r4)
            if (g_flag_evals != 0) {
                g_contention_until = now + std::chrono::milliseconds(100);
                g_eval_cv.wait(lk, [] { return g_flag_evals == 0; });
            }
            if (g_evals != 0 && g_announced == 0) g_contention_until = now + std::chrono::milliseconds(100);
            g_evals++;
            c->flags_now = false;
            return;
        }
        if (g_flag_evals != 0) {
            // Somebody else's flag-mode evaluation is in flight: this process runs evaluations from several threads without
            // having said so (gpt_concurrency_hint).  Wait for that one -- a flag-mode evaluation must be alone -- and keep the
            // process on event edges for a while: otherwise two un-hinted threads take turns, each alone at its start, each on
            // flags, the other one waiting -- serialised (measured: 2 x 600 evaluations at N = 4096 in 1.6 s against 0.8 s for
            // 600).  On events they overlap (1.5 x one at a time).
            g_contention_until = now + std::chrono::milliseconds(100);
            g_eval_cv.wait(lk, [] { return g_flag_evals == 0; });
        }
        flags = edge_flags_env_ok() && !g_flags_tripped.load() && g_evals == 0 && g_announced == 0 && c->edge_flags &&
                c->own_stream && c->d_edge && !c->use_graph && now >= g_contention_until;
        // (un-announced overlap seen: stay on events for the next 100 ms; announced sections -- ll_batch, bench.py -- end with
        // their bracket and the next lone evaluation is back on flags at once)
        if (g_evals != 0 && g_announced == 0) g_contention_until = now + std::chrono::milliseconds(100);
        g_evals++;
        if (flags) g_flag_evals++;
        c->flags_now = flags;
    }
    ~EvalScope()
    {
        std::lock_guard<std::mutex> lk(g_eval_mu);
        g_evals--;
        if (flags) g_flag_evals--;
        c->flags_now = false;
        g_eval_cv.notify_all();
    }
};

extern "C" int gpt_concurrency_hint(int delta)
{
    std::lock_guard<std::mutex> lk(g_eval_mu);
    g_announced += delta;
    if (g_announced < 0) g_announced = 0;
    return g_announced;
}

// May a rank-k update of an m x n block wait for its flag INSIDE the kernel?  Its workgroups spin until the word is up, so
// the launch must not be able to fill the chip in front of the update it waits for: only launches that launch_gemm_nt cuts
// into 32x32 tiles (fewer than gemm_small_threshold() 64x64 tiles: 8 KB of LDS and 256 threads per workgroup, many fit
// beside a trailing update) and only up to 1024 of those workgroups (half the chip's wave slots).  A launch of 64x64 tiles
// never does: measured at N = 8192 with 750 such workgroups waiting in the kernel, 4.84 against 4.45 ms per evaluation.
// Everything else waits on the stream, in front of the launch (launch_wait_flag).
static bool gemm_may_wait_in_kernel(const gpt_ctx *c, int64_t m, int64_t n)
{
    if (!(c->tile == 0 || c->tile == 64)) return false;
    const int64_t nt64 = ((m + 63) / 64) * ((n + 63) / 64);
    return nt64 < gemm_small_threshold() && ((m + 31) / 32) * ((n + 31) / 32) <= 1024;
}
// the next edge of the context on word d_edge[word]: the words are only ever raised, and every wait for one is bounded
// (its error word is d_edge[60], see EdgeSig)
static inline EdgeSig new_edge(gpt_ctx *c, int word)
{
    EdgeSig e;
    e.word = c->d_edge + word;
    e.value = ++c->edge_seq;
    e.err = c->d_edge + 60;
    return e;
}

// ------------------------------------------------------------------------------------------------
// Leaves (128-column diagonal block + the TRSM of the rows below it) and panels
// ------------------------------------------------------------------------------------------------
// short panel (the head chunk of the row-chunked multi-GPU schedule, the last panels of a factorisation): diagonal block
// and TRSM in one launch, the substitution trailing the pivots (potf2_trsm_kernel, potrf.hip)
static bool leaf_is_fused(const gpt_ctx *c, int64_t m) { return c->fuse_trsm > 0 && m >= 128 && m <= c->fuse_trsm && !c->use_graph; }
// workgroups of the launch that factors a leaf with m rows below it (the pivot block's, plus the fused kernel's consumers)
static int64_t leaf_workgroups(const gpt_ctx *c, int64_t m)
{
    if (!leaf_is_fused(c, m)) return 1;
    const int code = strip_rows_code(c, m);
    return code > 0 ? 1 + m / (128 >> code) : 1 + (m + 127) / 128;
}

// One leaf: the pivot block at Ad (global column `base`, packed workspace ws) and the m rows below it.  done_ev / done_edge
// are recorded / raised when L of the leaf is final; `wait` is polled by the leaf's first kernel before it reads anything.
static int leaf_factor(gpt_ctx *c, hipStream_t st, double *Ad, int64_t lda, double *ws, int32_t *info, int64_t base, int64_t m,
                       hipEvent_t done_ev = nullptr, EdgeSig done_edge = EdgeSig(), EdgeSig wait = EdgeSig())
{
    if (leaf_is_fused(c, m)) {
        if (c->flag_epoch > 0x3fffff00u) {      // (the progress word is only ever raised: start over long before a wrap)
            GPT_HIP_CHECK(hipMemsetAsync(c->d_flag, 0, 256, st));
            c->flag_epoch = 0;
        }
        c->flag_epoch += 32;           // (a launch raises the word by 8: one per 16-column step)
        return launch_potf2_trsm(st, Ad, lda, ws, info, base, m, c->d_flag, c->flag_epoch, done_ev, done_edge, wait, strip_rows_code(c, m));
    }
    GPT_TRY(launch_potf2_diag(st, Ad, lda, ws, info, base, wait));
    // (a stop event on the launch is not recorded by stream capture: under a graph use a plain record)
    GPT_TRY(launch_trsm_panel(st, m, Ad, lda, ws, Ad + 128 * lda, lda, c->use_graph ? nullptr : done_ev, done_edge));
    if (done_ev && c->use_graph) GPT_HIP_CHECK(hipEventRecord(done_ev, st));
    return GPT_OK;
}

static int panel_rec(gpt_ctx *c, hipStream_t st, double *Ap, int64_t lda, int64_t m, int64_t w, double *invd,
                     int32_t *info, int64_t base)
{
    if (w == 128) return leaf_factor(c, st, Ap, lda, invd, info, base, m - 128);
    const int64_t h = (w / 256) * 128 > 0 ? (w / 256) * 128 : 128;
    GPT_TRY(panel_rec(c, st, Ap, lda, m, h, invd, info, base));
    GPT_TRY(gemm_nt(c, st, m - h, w - h, h, -1.0, Ap + h * lda, lda, Ap + h * lda, lda, 1.0, Ap + h * lda + h, lda, 1));
    return panel_rec(c, st, Ap + h * lda + h, lda, m - h, w - h, invd + (h / 128) * GPT_WS_BLOCK, info, base + h);
}

// What the caller of one factorisation asks of it beyond the matrix (potrf_run / potrf_enqueue), and what it is told.
// The defaults are what every caller but factor_and_ll gets: the factorisation starts behind everything on the main stream
// and ends joined on it.
struct PotrfRequest {
    hipEvent_t head_event = nullptr;   // the columns panel 0 touches (nb_outer + 128) are built: the panel stream may start behind it
    EdgeSig head_wait;                 // ... the same as a flag word: the first leaf's kernel waits for it (fit_terms_once)
    bool defer_join = false;           // leave the final panel -> main join to the caller; the result names the stream the work ended on
    bool want_early_binv = false;      // eager alpha: build the 512-wide block inverses left of the last panel under that panel
    // Eager alpha with N a multiple of 512: the factor's last 128 columns hold only the augmented row and the padding.  alpha needs
    // nothing of that leaf, so its pivot block (and the rank-128 updates that reach it) leave the panel stream: the substitution
    // follows the last REAL leaf at once, the pad leaf and the reduction run beside it on the main stream (potrf_enqueue).
    bool defer_pad_leaf = false;
    // The matrix is a fit's augmented factor: only its first live_rows rows (the data rows and the augmented one) carry anything, the
    // rest is padding -- zero left of a unit diagonal, and stays so.  The trailing updates then leave those rows out (potrf_enqueue's
    // `update`; option "skip_pad_rows").  0: every row is live.
    int64_t live_rows = 0;
};
struct PotrfResult {
    hipStream_t tail_stream = nullptr;   // defer_join: the stream the factorisation ended on (nullptr: the main stream, joined)
    bool pad_leaf_deferred = false;      // the pad leaf went to the main stream (the reduction must follow it there)
};
// What the panels of ONE factorisation share (potrf_enqueue -> panel_ext)
struct PanelShared {
    EdgeSig first_wait;                // the first leaf of the factorisation waits for this word (the K build's head), once
    bool defer_pad = false;            // the pad leaf and what updates it go to the main stream (PotrfRequest::defer_pad_leaf)
    bool pad_leaf_deferred = false;    // ... and the pad leaf has been met and left out
    std::vector<int64_t> pad_upd_lc;   // leaves whose update of the pad block was held back, by first column
};

#define GPT_PANEL_EXT 128          // columns past its block column that a look-ahead panel's updates reach (panel_ext)
// The look-ahead panel of panel_ext (below), LEFT-looking inside the block column (option "inner" = 1): leaf j first receives the
// update of the leaves 0..j-1 of this block column in ONE launch (k = 128 j, 128 columns wide), then is factored; after
// the last leaf the 128 columns that follow the block column (the next panel's first leaf) get the whole block column's
// update (k = w).  Same flops as the right-looking form, but every update launch on the chain is 128 columns wide --
// the right-looking form's first leaf carries a (w + 128 - 128)-column update that shares the chip with the main stream's
// trailing update and measured 60 us against 13-16 us for the narrow ones (profiles/r01_timeline_c3_N8192.txt).
static int panel_ext_ll(gpt_ctx *c, hipStream_t st, double *A, int64_t lda, int64_t n, int64_t c0, int64_t w,
                        double *invd, int32_t *info, hipEvent_t wait_ev, hipEvent_t done_ev)
{
    bool waited = (wait_ev == nullptr);
    for (int64_t lc = c0; lc < c0 + w; lc += 128) {
        const int64_t kk = lc - c0;
        if (kk > 0) {
            if (!waited) {
                GPT_HIP_CHECK(hipStreamWaitEvent(st, wait_ev, 0));
                waited = true;
            }
            GPT_TRY(gemm_nt(c, st, n - lc, 128, kk, -1.0, A + lc * lda + c0, lda, A + lc * lda + c0, lda, 1.0,
                            A + lc * lda + lc, lda, 1));
        }
        const bool last = (lc + 128 == c0 + w);
        GPT_TRY(leaf_factor(c, st, A + lc * lda + lc, lda, invd + (lc / 128) * GPT_WS_BLOCK, info, lc, n - (lc + 128),
                            last ? done_ev : nullptr));
    }
    const int64_t e0 = c0 + w;
    if (e0 < n) {
        if (!waited) GPT_HIP_CHECK(hipStreamWaitEvent(st, wait_ev, 0));
        const int64_t ew = (n - e0 < GPT_PANEL_EXT) ? n - e0 : GPT_PANEL_EXT;
        GPT_TRY(gemm_nt(c, st, n - e0, ew, w, -1.0, A + e0 * lda + c0, lda, A + e0 * lda + c0, lda, 1.0,
                        A + e0 * lda + e0, lda, 1));
    }
    return GPT_OK;
}

// Look-ahead panel: block column [c0, c0+w) of the n x n matrix, right-looking in 128-column leaves.  Every leaf's
// rank-128 update also reaches the GPT_PANEL_EXT columns that follow the block column, so when the panel is done the
// first leaf of the NEXT block column is already up to date with respect to this one and its pivot chain can start
// without waiting for anybody.  `wait_ev` (the other stream's update of the columns this panel reads beyond its first
// leaf) is waited for before the first update; `done_ev` is recorded once L of the block column is final.
#define GPT_INNER_ROWS 4608        // "inner" = 2: left-looking once at most this many rows remain (the chain-bound end)
#define GPT_HEAD_WAIT_WGS 33       // first leaf: in-kernel wait for the K build's head while its launch has at most this many workgroups
// wait_edge / done_edge: the same two dependencies as wait_ev / done_ev carried by flag words (EdgeSig, common.hpp)
// first_ev: recorded by the panel's FIRST update launch (see "deferred rest" in potrf_enqueue)
static int panel_ext(gpt_ctx *c, PanelShared &ps, hipStream_t st, double *A, int64_t lda, int64_t n, int64_t c0, int64_t w,
                     double *invd, int32_t *info, hipEvent_t wait_ev, hipEvent_t done_ev, hipEvent_t first_ev,
                     EdgeSig wait_edge, EdgeSig done_edge)
{
    if (c->inner == 1 || (c->inner == 2 && n - c0 <= GPT_INNER_ROWS))
        return panel_ext_ll(c, st, A, lda, n, c0, w, invd, info, wait_ev, done_ev);
    const int64_t cend = (c0 + w + GPT_PANEL_EXT < n) ? c0 + w + GPT_PANEL_EXT : n;
    for (int64_t lc = c0; lc < c0 + w; lc += 128) {
        const int64_t r1 = lc + 128;
        const bool last = (r1 == c0 + w);
        const int64_t m = n - r1;
        if (ps.defer_pad && m == 0) {
            // the pad leaf itself: enqueued by potrf_enqueue on the main stream (nothing on this stream depends on it)
            ps.pad_leaf_deferred = true;
            if (last && done_ev) GPT_HIP_CHECK(hipEventRecord(done_ev, st));
            if (lc == c0 && wait_ev) GPT_HIP_CHECK(hipStreamWaitEvent(st, wait_ev, 0));
            continue;
        }
        EdgeSig fw;                                   // the first leaf of a factorisation may have to wait for the K build's head
        if (lc == 0 && ps.first_wait.word) {
            fw = ps.first_wait;
            ps.first_wait = EdgeSig();
            // Inside the leaf's kernel only while that launch fits the CUs reserved for the panel stream: every workgroup of
            // the fused kernel holds a whole CU (135 KB of LDS) while it spins, and beyond the reserved CUs they would be
            // taken from the K build the launch is waiting for.  Otherwise a one-wave wait kernel in front of it.
            if (leaf_workgroups(c, m) > GPT_HEAD_WAIT_WGS) {
                GPT_TRY(launch_wait_flag(st, fw));
                fw = EdgeSig();
            }
        }
        GPT_TRY(leaf_factor(c, st, A + lc * lda + lc, lda, invd + (lc / 128) * GPT_WS_BLOCK, info, lc, m, last ? done_ev : nullptr,
                            last ? done_edge : EdgeSig(), fw));
        if (lc == c0 && wait_ev) GPT_HIP_CHECK(hipStreamWaitEvent(st, wait_ev, 0));
        int64_t cend_p = cend;                       // this stream's share of the leaf's update: columns [r1, cend_p)
        if (ps.defer_pad && cend == n) {
            // the leaf's update of the pad block (the last 128 columns) is held back for the main stream (all of them: a leaf
            // that applied its own here would run ahead of the held-back ones -- another order than defer_pad = 0)
            ps.pad_upd_lc.push_back(lc);
            cend_p = n - 128;
            if (cend_p <= r1 && first_ev) {
                GPT_HIP_CHECK(hipEventRecord(first_ev, st));
                first_ev = nullptr;
            }
        }
        if (cend_p > r1) {
            // (the first update of the panel is the first kernel of the chain that touches what the main stream's urgent
            // update wrote: it waits for that edge itself, see gemm.hip)
            // Its workgroups SPIN until the word is up, so the launch must not be able to fill the chip (the update they
            // wait for needs room to run): in the kernel only while the launch stays under 1024 workgroups = half the wave
            // slots, otherwise as a stream operation in front of it (a one-wave wait kernel, ~5 us).
            EdgeSig inwait;
            if (lc == c0 && wait_edge.word) {
                if (gemm_may_wait_in_kernel(c, n - r1, cend_p - r1)) inwait = wait_edge;
                else GPT_TRY(launch_wait_flag(st, wait_edge));
            }
            GPT_TRY(gemm_nt(c, st, n - r1, cend_p - r1, 128, -1.0, A + r1 * lda + lc, lda, A + r1 * lda + lc, lda, 1.0,
                            A + r1 * lda + r1, lda, 1, first_ev, EdgeSig(), inwait));
            first_ev = nullptr;
        }
    }
    return GPT_OK;
}

static int enqueue_early_block_inverses(gpt_ctx *c, hipStream_t S, int64_t cols, int64_t cols_final);      // api_solve.inc
#define GPT_MERGE_MIN_TILES 512    // urgent + rest are one launch while it has at least this many 64x64 tiles (it needs an order table)
static int potrf_enqueue(gpt_ctx *c, int64_t n, double *A, int64_t lda, double *invd, int32_t *info, const PotrfRequest &req,
                         PotrfResult *res)
{
    if (n % 128) {
        gpt_set_error("potrf: n must be a multiple of 128 (n=%lld)", (long long)n);
        return GPT_E_ARG;
    }
    const int64_t nbo = outer_width(c, n);
    const int64_t nblk = (n + nbo - 1) / nbo;
    const hipStream_t S = c->stream, P = c->panel_stream;
    const bool la = c->lookahead && nblk > 1;
    // the rank-pw update by the block column [pc0, pc0 + pw): the lower trapezoid of the columns [a, b), rows [a, n) -- of which the
    // rows [a, live) are computed (PotrfRequest::live_rows: for a padding row r every L[r, k] is 0 and stays 0, its update is
    // C[r, :] -= 0 * B^T and nothing reads it; a < live always, the last block column holds the augmented row).  On every stream
    // the look-ahead uses it on, and in the one-stream loop below.
    // (not under option graph: a captured factorisation is replayed for every N of the same padded order)
    const int64_t live = (req.live_rows > 0 && req.live_rows < n && c->skip_pad_rows && !c->use_graph) ? req.live_rows : n;
    auto update = [&](hipStream_t st, int64_t pc0, int64_t pw, int64_t a, int64_t b, hipEvent_t done = nullptr, EdgeSig edge = EdgeSig(),
                      EdgeSig wait = EdgeSig(), int64_t edge_cols = 0, EdgeSig tail = EdgeSig()) -> int {
        return gemm_nt(c, st, n - a, b - a, pw, -1.0, A + a * lda + pc0, lda, A + a * lda + pc0, lda, 1.0, A + a * lda + a, lda, 1,
                       done, edge, wait, edge_cols, tail, live > a ? live - a : -1);
    };
    if (!la) {
        for (int64_t k = 0; k < nblk; k++) {
            const int64_t c0 = k * nbo, w = (n - c0 < nbo) ? n - c0 : nbo, m = n - c0;
            GPT_TRY(panel_rec(c, S, A + c0 * lda + c0, lda, m, w, invd + (c0 / 128) * GPT_WS_BLOCK, info, c0));
            if (c0 + w < n) GPT_TRY(update(S, c0, w, c0 + w, n));
        }
        return GPT_OK;
    }
    // ---- look-ahead.  P (high priority, reserved CUs) runs the latency-bound chain: the panels, each extended by
    // GPT_PANEL_EXT columns (panel_ext).  S applies panel k (rank nbo) to everything right of column
    // u0 = c0 + nbo + EXT in two launches: the nbo columns panel k+1 is going to touch first ("urgent", event e_cu),
    // then the rest.  P never waits for a large update: its only dependency is e_cu(k) before the first update of
    // panel k+1, and S has the whole first pivot block + TRSM of that panel to get there.
    //
    // What holds for the whole factorisation:
    const bool graph = c->use_graph != 0;
    const bool tile64 = (c->tile == 0 || c->tile == 64);      // (the edge flags and the tail wait live in the 64x64 / 32x32 GEMM kernels only)
    // Helper: while the trailing updates dominate, the panel stream leaves its reserved CUs idle most of the time.
    // The bottom-right triangle [s, n)^2 of the rank-w update of panel k therefore runs on H, a stream masked to
    // those CUs (minus 8 that stay free for the diagonal-block kernel), concurrently with S's share; the split is
    // sized by the two streams' rates so that they finish together.  The split column only moves right: a helper
    // region lies inside the previous one, so H needs nothing but "panel k is final"; S waits for helper k before
    // it next touches columns >= s.
    // (only where the updates dominate: at n = 8192 the helper costs 0.5-1 %, at 16384 / 32768 it gains 2 / 3 %)
    const hipStream_t H = (c->helper_stream && !graph && c->helper_tf > 0 && n > c->helper_min_n) ? c->helper_stream : nullptr;
    const double rate_s = 46e12, rate_h = 1e11 * (double)c->helper_tf * (double)c->helper_cus / 24.0;
    // Flag edges (EdgeSig): "panel k is final" (panel stream -> main stream) and "the urgent update of panel k is done"
    // (main -> panel stream) are raised by the last workgroup of the kernel that completes them and waited for by a
    // kernel -- 1.5 us per edge against 8-9 for an event, and no stop event on the chain's kernels (4.5 us
    // each).  In the chain-bound end both edges are on the critical path of every panel.
    // (not with the helper stream: flags + helper -- the helper waiting behind a wait kernel, the merged launch cut at the
    // split column, code below -- measured the same as events + helper at N = 16384 (27.65 against 27.49 ms), and the helper
    // in the head of an N = 8192 factorisation still loses, 4.64 against 4.45 ms: round 3)
    const bool use_flags = c->flags_now && !H && c->inner == 0 && c->defer_rows == 0 && tile64;
    // Update-bound head (option purg_rows): while more rows than this remain, the PANEL stream applies panel k to the columns
    // panel k+1 touches ("urgent") itself, right behind the panel -- no event round trip panel -> main -> panel on the chain and
    // one launch less on the main stream, which sets the pace there.
    // (with flag edges and merged launches the main stream has one launch per panel anyway and the urgent tiles run at
    // the large launch's rate: the panel stream's own urgent update no longer pays -- 4.444 against 4.492 ms at N = 8192)
    const int64_t purg_eff = (H || graph || (use_flags && c->merge_urgent)) ? 0 : c->purg_rows;
    // (edge_flags >= 2: "the rest of panel k-1 is done" as a flag edge as well -- no stop event on the main
    // stream's large launches, which set the pace there; the whole C of that launch is then written through)
    const bool rest_flag = use_flags && c->edge_flags >= 2;
    // Tail wait: the last launch of a panel on the main stream ends only when the NEXT panel's flag is up, so the next
    // panel's launch follows it without a wait kernel in between.
    // NOT while the launches are being timed (option profile_gemm: bench.py's roofline events): a launch that waits at its
    // end reports its wait as its own duration -- in the transition from the update-bound head to the chain-bound end,
    // where the main stream does wait for the panel stream, 20-50 us of a 60-110-us launch.  A timed evaluation keeps the
    // wait in a kernel of its own, like tail_wait = 0, and its launches' durations are the GEMM's.
    const bool tail_here = use_flags && c->tail_wait != 0 && !c->prof_gemm;
    // Deferred rest (chain-bound end of the factorisation, option defer_rows).  There the panel stream sets the pace and the
    // main stream has slack, yet its large "rest" update of panel k used to start right after the urgent one and shared
    // the chip with the panel stream's first leaf update of panel k+1 -- which is ON the chain and ran 60 us instead of
    // ~17 (profiles/r01_timeline_c3_N8192.txt).  The rest of panel k is therefore held back until that leaf update is
    // done (one event), and is enqueued one loop iteration late so that the event is recorded before it is waited for.
    const int64_t defer_rows = (!H && !graph) ? c->defer_rows : 0;
    // Panel widths: nbo; optionally ("ramp") 128, 256, ... at the start so that the main stream gets its first update
    // after one leaf instead of after a whole panel -- measured slightly slower (N=8192: 5.95 against 5.90 ms,
    // N=16384: 31.4 against 31.2: the rank-128/256 updates it adds are inefficient), so it is off by default.
    std::vector<int64_t> widths;
    {
        int64_t c0 = 0, w = c->ramp ? 128 : nbo;
        while (c0 < n) {
            // (option nb_early: wider panels while more than nb_switch_rows rows remain -- the update-bound head of the
            // factorisation -- and nbo in the chain-bound rest)
            const int64_t cap = (c->nb_early > 0 && n - c0 > c->nb_switch_rows) ? c->nb_early : nbo;
            if (w > cap || (!c->ramp)) w = cap;
            if (w > n - c0) w = n - c0;
            widths.push_back(w);
            c0 += w;
            w += 128;
        }
    }
    const size_t np = widths.size();

    PanelShared ps;
    ps.defer_pad = req.defer_pad_leaf && c->inner == 0 && !graph;      // (the right-looking look-ahead panels only)
    if (req.head_wait.word && c->inner == 0) {
        // the first leaf's kernel waits for the word itself (potrf.hip: edge_wait): no event edge in front of the chain
        ps.first_wait = req.head_wait;
    } else {
        hipEvent_t head = req.head_event;
        if (!head) {
            head = get_event(c, 0);
            if (!head) return GPT_E_HIP;
            GPT_HIP_CHECK(hipEventRecord(head, S));
        }
        GPT_HIP_CHECK(hipStreamWaitEvent(P, head, 0));
    }
    if (use_flags && c->edge_seq > 0xf0000000u && !req.head_wait.word) {       // (the words are only ever raised: start over long before a wrap)
        GPT_HIP_CHECK(hipStreamSynchronize(S));
        GPT_HIP_CHECK(hipStreamSynchronize(P));
        GPT_HIP_CHECK(hipMemsetAsync(c->d_edge, 0, 256, S));
        GPT_HIP_CHECK(hipStreamSynchronize(S));
        c->edge_seq = 0;
        c->alpha_counter = 0;                  // (the step counter of the wide back-substitution lives in the same words)
    }
    hipEvent_t e_cu_prev = nullptr, e_help_prev = nullptr, e_rest_prev = nullptr;
    EdgeSig cu_edge_prev, rest_edge_prev;
    EdgeSig next_panel_edge;      // the NEXT panel's edge, allocated early: the main stream's last launch of this panel awaits it at its end
    int64_t c0 = 0, s_prev = 0;
    int64_t awaited = 0;          // end column of the last panel the main stream has waited for (eager alpha's early block inverses)
    struct PendingRest { bool on; int64_t c0, w, u1, split; } pend = {false, 0, 0, 0, 0};
    for (size_t k = 0; k < np; c0 += widths[k], k++) {
        const int64_t w = widths[k];
        const int64_t wn = (k + 1 < np) ? widths[k + 1] : 0;      // width of the next panel
        hipEvent_t e_panel = get_event(c, 2 + 4 * k), e_cu = get_event(c, 3 + 4 * k), e_help = get_event(c, 4 + 4 * k);
        hipEvent_t e_sdone = get_event(c, 5 + 4 * k);
        if (!e_panel || !e_cu || !e_help || !e_sdone) return GPT_E_HIP;
        hipEvent_t e_first = pend.on ? get_event(c, 8 + 4 * np + k) : nullptr;
        if (pend.on && !e_first) return GPT_E_HIP;
        const int64_t u0 = c0 + w + GPT_PANEL_EXT;      // the first column panel k's own leaf updates did not reach
        EdgeSig panel_edge;
        bool panel_awaited = false;      // (by the tail wait of the previous panel's last main-stream launch)
        if (use_flags && u0 < n) {
            panel_awaited = next_panel_edge.word != nullptr;
            panel_edge = panel_awaited ? next_panel_edge : new_edge(c, 0);
        }
        next_panel_edge = EdgeSig();
        GPT_TRY(panel_ext(c, ps, P, A, lda, n, c0, w, invd, info, e_cu_prev, use_flags ? nullptr : e_panel, e_first, cu_edge_prev,
                          panel_edge));
        e_cu_prev = nullptr;
        cu_edge_prev = EdgeSig();
        if (pend.on) {
            GPT_HIP_CHECK(hipStreamWaitEvent(S, e_first, 0));
            GPT_TRY(update(S, pend.c0, pend.w, pend.u1, pend.split));
            pend.on = false;
        }
        if (u0 >= n) continue;      // nothing right of what the panel itself updated
        // urgent: the columns panel k+1 touches beyond what panel k's own leaf updates reached, [u0, u1)
        const int64_t u1 = (u0 + wn < n) ? u0 + wn : n;
        int64_t split = n;                                        // S takes columns [u1, split), H [split, n)
        if (H && u1 < n) {
            const double side0 = (double)(n - u1);
            int64_t side = (int64_t)(sqrt(rate_h / (rate_s + rate_h)) * side0) / 64 * 64;
            if (n - side < s_prev) side = n - s_prev;
            // worth a launch only while the update is large (>= ~10 GFLOP) and the slice a real triangle
            if (side >= 1024 && n - side > u1 && (double)w * side0 * side0 >= 1e10) split = n - side;
        }
        if (split < n && !e_help_prev) {
            // first helper (or first after a gap): its region was last written by S (K build / a whole update)
            GPT_HIP_CHECK(hipEventRecord(e_sdone, S));
            GPT_HIP_CHECK(hipStreamWaitEvent(H, e_sdone, 0));
        }
        if (!use_flags) GPT_HIP_CHECK(hipStreamWaitEvent(S, e_panel, 0));
        else if (!panel_awaited) GPT_TRY(launch_wait_flag(S, panel_edge));
        awaited = c0 + w;        // (panel_awaited: the previous panel's last launch on S waited for it at its end)
        // (the tail wait's flag is the next panel's: its value is fixed here, one panel early)
        EdgeSig tail;
        if (tail_here && split == n && k + 1 < np && u0 + wn < n) tail = new_edge(c, 0);
        if (split < n) {
            if (use_flags) GPT_TRY(launch_wait_flag(H, panel_edge));
            else GPT_HIP_CHECK(hipStreamWaitEvent(H, e_panel, 0));
            GPT_TRY(update(H, c0, w, split, n, e_help));
        }
        bool help_waited = false;      // S waits for the previous helper slice before it touches that slice's columns
        if (e_help_prev && u1 > s_prev) {
            GPT_HIP_CHECK(hipStreamWaitEvent(S, e_help_prev, 0));
            help_waited = true;
        }
        auto wait_help_prev = [&]() -> int {
            if (e_help_prev && !help_waited) GPT_HIP_CHECK(hipStreamWaitEvent(S, e_help_prev, 0));
            e_help_prev = nullptr;
            return GPT_OK;
        };
        // A panel ends in one of three ways:
        if (purg_eff > 0 && n - c0 > purg_eff && u1 < n) {
            // (1) urgent update on the PANEL stream, rest on the main stream (no helper here: split == n).  Both streams
            // read-modify-write the urgent columns (the main stream's rest of panel k-1 covers them too), so the panel stream
            // waits for that rest.
            if (e_rest_prev) GPT_HIP_CHECK(hipStreamWaitEvent(P, e_rest_prev, 0));
            if (!e_rest_prev && !rest_edge_prev.word) {
                // First update the PANEL stream applies beyond the head columns: whatever the main stream still has in
                // flight on those columns -- the rest of the K build of this evaluation -- must be through.  (Found with the
                // `ramp` option, whose 128-wide first panel is done before the K build is: "8064-th leading minor not
                // positive definite"; with 384-wide panels the build happened to finish first.)
                hipEvent_t e_k = get_event(c, 9 + 5 * np);
                if (!e_k) return GPT_E_HIP;
                GPT_HIP_CHECK(hipEventRecord(e_k, S));
                GPT_HIP_CHECK(hipStreamWaitEvent(P, e_k, 0));
            }
            EdgeSig rwait;
            if (rest_edge_prev.word) {
                if (gemm_may_wait_in_kernel(c, n - u0, u1 - u0)) rwait = rest_edge_prev;
                else GPT_TRY(launch_wait_flag(P, rest_edge_prev));
            }
            GPT_TRY(update(P, c0, w, u0, u1, nullptr, EdgeSig(), rwait));
            e_rest_prev = nullptr;
            rest_edge_prev = EdgeSig();
            if (rest_flag) {
                rest_edge_prev = new_edge(c, 32);
                GPT_TRY(update(S, c0, w, u1, n, nullptr, rest_edge_prev));
            } else {
                e_rest_prev = get_event(c, 10 + 5 * np + k);
                if (!e_rest_prev) return GPT_E_HIP;
                GPT_TRY(update(S, c0, w, u1, n, e_rest_prev));
            }
            continue;
        }
        e_rest_prev = nullptr;
        rest_edge_prev = EdgeSig();
        if (use_flags) {
            cu_edge_prev = new_edge(c, 16);
            // (2) urgent + rest as ONE launch (option merge_urgent) while the update is large enough for an order table: the
            // tiles of the urgent columns come first on every XCD, write through and raise the flag when THEY are done;
            // the rest follows in the same launch -- one drain and one ramp-up less per panel on the main stream, and
            // the small urgent launch (30 TFLOP/s on its own) runs at the large launch's rate.
            // (with a helper slice the merged launch is the lower trapezoid of the columns [u0, split))
            const int64_t mtn = (split - u0 + 63) / 64, mtm = (n - u0 + 63) / 64;
            const int64_t nt64m = mtn * (mtn + 1) / 2 + (mtm - mtn) * mtn;
            if (c->merge_urgent && u1 < split && nt64m >= GPT_MERGE_MIN_TILES && (u1 - u0) % 64 == 0) {
                GPT_TRY(wait_help_prev());
                GPT_TRY(update(S, c0, w, u0, split, nullptr, cu_edge_prev, EdgeSig(), u1 - u0, tail));
                next_panel_edge = tail;
                if (split < n) {
                    s_prev = split;
                    e_help_prev = e_help;
                }
                continue;
            }
            GPT_TRY(update(S, c0, w, u0, u1, nullptr, cu_edge_prev));
        } else {
            GPT_TRY(update(S, c0, w, u0, u1, e_cu));
            e_cu_prev = e_cu;
        }
        // (3) urgent, then the rest -- at once, or (defer_rows) behind the next panel's first update
        if (u1 < n) {
            GPT_TRY(wait_help_prev());
            if (defer_rows > 0 && n - c0 <= defer_rows && k + 1 < np) {
                pend = PendingRest{true, c0, w, u1, split};
            } else {
                // (an event may not ride on the launch that carries the tail wait)
                GPT_TRY(update(S, c0, w, u1, split, nullptr, EdgeSig(), EdgeSig(), 0, tail));
                next_panel_edge = tail;
            }
            if (split < n) {
                s_prev = split;
                e_help_prev = e_help;
            }
        }
    }
    if (pend.on) GPT_TRY(update(S, pend.c0, pend.w, pend.u1, pend.split));
    // Eager alpha: the inverses of the 512 x 512 diagonal blocks left of the last panel are built now, on the main stream, which has
    // nothing else to do while the panel stream factors the last panel (api_solve.inc; the blocks right of them follow behind the
    // factorisation) -- as far as they are FINAL on S, i.e. left of the last panel S has WAITED for.  That is usually the
    // panel in front of the last one, but a panel whose update reaches no column (c0 + w + EXT >= n: the one in front of a
    // 128-wide last panel) is never waited for, and reading its columns would race the panel stream (ADVICE r6).
    // The last helper slice (e_help_prev, joined below) writes nothing left of `awaited` by then: every column there belongs to
    // a panel S has waited for, and a panel is factored only behind every update of its columns, the helper's included (S waits
    // for a helper slice before its next urgent update touches the slice's columns, and the panel stream waits for that update).
    if (req.want_early_binv && A == c->dA && invd == c->d_invd && np >= 2)
        GPT_TRY(enqueue_early_block_inverses(c, S, n - widths.back(), awaited));
    if (ps.pad_leaf_deferred) {
        // The pad leaf (PotrfRequest::defer_pad_leaf): behind the last real leaf, on the main stream -- the held-back rank-128 updates
        // of the pad block in leaf order (the order the panel stream would have applied them in: same bits), then its pivot block.
        hipEvent_t e_real = get_event(c, 12 + 6 * np);
        if (!e_real) return GPT_E_HIP;
        GPT_HIP_CHECK(hipEventRecord(e_real, P));
        GPT_HIP_CHECK(hipStreamWaitEvent(S, e_real, 0));
        const int64_t pc = n - 128;
        for (const int64_t lc : ps.pad_upd_lc)
            GPT_TRY(gemm_nt(c, S, 128, 128, 128, -1.0, A + pc * lda + lc, lda, A + pc * lda + lc, lda, 1.0, A + pc * lda + pc, lda, 1));
        GPT_TRY(launch_potf2_diag(S, A + pc * lda + pc, lda, invd + (pc / 128) * GPT_WS_BLOCK, info, pc));
        res->pad_leaf_deferred = true;
    }
    if (e_help_prev) GPT_HIP_CHECK(hipStreamWaitEvent(S, e_help_prev, 0));
    if (req.defer_join && !graph) {
        // (the caller continues on the panel stream -- the last leaf runs there -- and joins the streams itself)
        res->tail_stream = P;
        return GPT_OK;
    }
    hipEvent_t e_end = get_event(c, 1);
    if (!e_end) return GPT_E_HIP;
    GPT_HIP_CHECK(hipEventRecord(e_end, P));
    GPT_HIP_CHECK(hipStreamWaitEvent(S, e_end, 0));
    return GPT_OK;
}

static int potrf_run(gpt_ctx *c, int64_t n, double *A, int64_t lda, double *invd, int32_t *info,
                     const PotrfRequest &req = PotrfRequest(), PotrfResult *res = nullptr)
{
    PotrfResult unused;
    if (!res) res = &unused;
    *res = PotrfResult();
    if (!c->use_graph) return potrf_enqueue(c, n, A, lda, invd, info, req, res);
    if (c->gexec && (c->g_n != n || c->g_nb != c->nb_outer || c->g_la != c->lookahead || c->g_A != A)) {
        hipGraphExecDestroy(c->gexec);
        c->gexec = nullptr;
    }
    if (!c->gexec) {
        hipGraph_t graph = nullptr;
        GPT_HIP_CHECK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
        int rc = potrf_enqueue(c, n, A, lda, invd, info, req, res);
        hipError_t e = hipStreamEndCapture(c->stream, &graph);
        if (rc != GPT_OK) {
            if (graph) hipGraphDestroy(graph);
            return rc;
        }
        GPT_HIP_CHECK(e);
        GPT_HIP_CHECK(hipGraphInstantiate(&c->gexec, graph, nullptr, nullptr, 0));
        hipGraphDestroy(graph);
        c->g_n = n;
        c->g_nb = c->nb_outer;
        c->g_la = c->lookahead;
        c->g_A = A;
    }
    GPT_HIP_CHECK(hipGraphLaunch(c->gexec, c->stream));
    return GPT_OK;
}

// B (m x n) <- B L^-T, n a multiple of 128
static int trsm_rlt(gpt_ctx *c, hipStream_t st, int64_t m, int64_t n, const double *L, int64_t ldl, const double *invd,
                    double *B, int64_t ldb)
{
    if (n == 128) return launch_trsm_panel(st, m, L, ldl, invd, B, ldb);
    const int64_t h = (n / 256) * 128 > 0 ? (n / 256) * 128 : 128;
    GPT_TRY(trsm_rlt(c, st, m, h, L, ldl, invd, B, ldb));
    GPT_TRY(gemm_nt(c, st, m, n - h, h, -1.0, B, ldb, L + h * ldl, ldl, 1.0, B + h, ldb, 0));
    return trsm_rlt(c, st, m, n - h, L + h * ldl + h, ldl, invd + (h / 128) * GPT_WS_BLOCK, B + h, ldb);
}
