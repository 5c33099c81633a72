// api.hip -- C ABI (include/gpt_hip.h) and host-side orchestration for libgpt_hip.so.
// One translation unit, kept in parts by entry-point family (api_*.inc, included at the end of this file in dependency order):
// this file holds the error channel and struct gpt_ctx.  What belongs to ONE factorisation (not to the context) travels as
// arguments: PotrfRequest / PotrfResult / PanelShared, api_schedule.inc.  The model kernel is ONE value (ModelKernel,
// api_kparams.inc): parse_model is the only place that reads the ABI's id / parameter-count arrays, and the derivative-order
// rules live there too, one function per family (training points, test points, free-standing pair lists / Gram blocks).
//
// Host logic restated here (not kernels): the blocked right-looking Cholesky with a recursive
// panel and one-panel look-ahead on a second, high-priority HIP stream; the padded / augmented
// matrix layout; GaussianProcess.compute_K_L_alpha_ll (ref: gptools/gaussian_process.py:1418-1469)
// and GaussianProcess.predict (ref: gptools/gaussian_process.py:965-1006) sequencing.
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <chrono>
#include <mutex>
#include <vector>
#include "common.hpp"
#include "warp.hpp"

// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void gpt_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *gpt_last_error(void) { return g_err; }
extern "C" int gpt_version(void) { return 100; }

#define GPT_TRY(expr)          \
    do {                       \
        int rc_ = (expr);      \
        if (rc_ != GPT_OK) return rc_; \
    } while (0)

static inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

#include "api_kparams.inc"      // the model kernel (KParams marshalling, ModelKernel, parse_model) and the derivative-order checks of every entry point

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

enum { SLOT_XI = 0, SLOT_XJ, SLOT_NI, SLOT_NJ, SLOT_OUT, SLOT_KST, SLOT_KSS, SLOT_XS, SLOT_NS, SLOT_VEC, SLOT_VEC2,
       SLOT_RHS, SLOT_LOW, SLOT_KFULL, SLOT_TK, SLOT_ZERO, SLOT_UINV, SLOT_WINV, SLOT_GPART, SLOT_BINV, SLOT_BTMP,
       SLOT_BINV2, SLOT_BINV3, SLOT_BINV3U, SLOT_BINVU, SLOT_BATCH_A, SLOT_BATCH_WS, SLOT_BATCH_MISC, SLOT_SPLITK,
       SLOT_PB_V, SLOT_PB_COV, SLOT_PB_MISC, SLOT_XSW, SLOT_SS, SLOT_SI, SLOT_SJ, SLOT_WB_X, SLOT_WB_S, SLOT_WB_P, SLOT_GKP, SLOT_GB_U, SLOT_GB_W, SLOT_GB_MISC,
       SLOT_LOO_V, SLOT_LOO_VEC,
       SLOT_SP_Z, SLOT_SP_LU, SLOT_SP_LB, SLOT_SP_V, SLOT_SP_W, SLOT_SP_G, SLOT_SP_PART, SLOT_SP_MISC, SLOT_SP_Y,
       SLOT_SP_S1, SLOT_SP_S2, SLOT_SP_GM, SLOT_SP_GVEC, SLOT_SP_GPART, SLOT_SP_DZPART, SLOT_SP_DZ,
       SLOT_SP_SEL_L, SLOT_SP_SEL_X, SLOT_SP_SEL_MISC,
       SLOT_SPB_LU, SLOT_SPB_LB, SLOT_SPB_V, SLOT_SPB_G, SLOT_SPB_PART, SLOT_SPB_MISC, SLOT_COUNT };

struct gpt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t panel_stream = nullptr;
    hipStream_t helper_stream = nullptr;   // CU-masked to part of the reserved CUs (own streams only)
    int64_t nb_early = 0, nb_switch_rows = 4608;   // see potrf_enqueue (panel widths)
    unsigned *d_edge = nullptr;            // edge-flag words (EdgeSig, common.hpp): [0,1] "panel k final", [16,17] "urgent update k done"
    unsigned edge_seq = 0;                 // value of the last edge raised (monotonic over the context's life)
    int64_t tail_wait = 1;                 // 1: the main stream's last launch of a panel awaits the NEXT panel's flag at its end (gemm.hip "tail wait"): no
                                           //    wait kernel between two trailing updates.  Round 4 measured it the same as 0 (4.459 / 4.471 ms at N = 8192); at
                                           //    round 6's schedule: C3 -2 ... -47 us in six same-process A/Bs (mean 19), C2 -11 ... -18 us -- on.  The gain sits in
                                           //    the launches that DO wait (1-6 GFLOP: only-large or only-small launches gain nothing); not while launches are timed.
    int64_t merge_urgent = 1;              // 1: with flag edges, urgent + rest of a panel are ONE launch (urgent tiles first, partial flag)
                                           //    while the merged launch has at least GPT_MERGE_MIN_TILES 64x64 tiles
    int64_t skip_pad_rows = 1;             // 1: the trailing updates of a fit leave out the padding rows of the augmented factor (PotrfRequest::live_rows);
                                           //    0: they cover all NP rows, as they did before (same bits in every row <= N; A/B and the tests' reference)
    int64_t edge_flags = 1;                // 1: those two edges of the look-ahead may be flag words instead of events (see EvalScope)
    bool flags_now = false;                // ... and ARE, in the evaluation in progress (set by EvalScope)
    int reserve_cus = 0;                   // CUs the main stream's mask leaves to the panel stream (0: unmasked)
    int64_t gemm_prio = -1;                // >= 0: wave priority of ALL GEMM main loops of this context
    int64_t purg_rows = 6144;              // > 0: while more rows than this remain, the panel stream does the "urgent" update itself
                                           // (N=8192: 5.36 against 5.44 ms, bit-identical; no effect below ~7k rows or with the helper stream)
    int64_t defer_rows = 0;             // chain-bound end: with at most this many rows left, the main stream's "rest" update of
                                           // panel k starts only after the panel stream's first update of panel k+1 (0 = off)
    int helper_cus = 0;
    std::vector<hipEvent_t> events;       // sync-only events (look-ahead fork/join)
    hipEvent_t tev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // options
    int64_t nb_outer = 0;              // outer block width; 0 = by size (outer_width())
    int lookahead = 1;
    int use_graph = 0;
    long n_maxsum = 0;                 // largest row sum of the training derivative orders (gpt_set_data)
    long n_colmax[GPT_MAX_DIM] = {};   // largest training order of each coordinate (gpt_set_data): a Gibbs factor's own rule
    long n_maxord = 0;                 // largest single derivative order of the training points (gpt_set_data)
    int timing = 0;
    int tile = 0;
    int gemm_pad = 1024;
    int64_t fuse_trsm = 8192;          // panels with at most this many rows below the leaf use potf2_trsm_kernel (0 = never)
    unsigned *d_flag = nullptr;        // progress word of potf2_trsm_kernel (only ever raised)
    unsigned flag_epoch = 0;
    int64_t binv_launches = 0;             // 1: the 512-wide block inverses by the recursion over 15 launches of rounds 2-4 instead of trinv512_kernel
    int64_t splitk = 512;                  // few-rows solves: GEMMs with k >= 1024 of fewer 32x32 tiles than this are split along k until they reach it (0: never)
    int64_t fuse_rows32 = 2048, fuse_rows16 = 0;   // ... 32 / 16 rows per consumer workgroup: two / one strip waves per CU (same-box A/B, bit-identical: N = 4096
                                                   // 1.158 -> 1.152 ms, N = 8192 4.346 -> 4.31 ms with 32 rows below 2048; 16 rows: no further gain)
    int64_t fuse_rows64 = 2048;        // fused leaves with at most this many rows below them: 64 rows per consumer workgroup (one strip
                                       // wave per SIMD, potf2_trsm_kernel<.., true>); 0 = always 128
    int64_t helper_min_n = 12288;      // the helper stream takes part only above this matrix size
    int helper_tf = 45;                // assumed rate of the helper stream, in 0.1 TFLOP/s per 24 CUs (0 = no helper);
                                       // measured: 0 / 25 / 35 / 50 -> 212 / 209 / 206 / 214 ms at N=32768, 30.8 / 30.6 / 30.2 / 32.0 at N=16384
    int ramp = 0;                      // first panels 128, 256, ... wide (see potrf_enqueue); measured slower, off
    int inner = 0;                     // look-ahead panel: 0 right-looking leaves, 1 left-looking (panel_ext_ll), 2 left-looking
                                       //   once at most GPT_INNER_ROWS rows remain (the chain-bound end of the factorisation)
    // resident training inputs
    int64_t N = 0;             // order of the factorised matrix (= Nx without T, = Ny with T)
    int64_t Nx = 0;            // resident points
    int D = 0;
    double *dT = nullptr;      // linear transform T (Ny x Nx), zero-padded to (round_up(Ny,64) x round_up(Nx,16))
    int64_t Ny = 0, NxP = 0;
    double *dX = nullptr;
    int32_t *dn = nullptr;
    // input warp (gpt_set_warp): while warp.nlayers > 0 the builders read dXw (Nx x D warped points) in place of dX and take
    // the slope factors dS (Nx) on tiles with derivative orders
    WarpLayers warp = WarpLayers();
    double *dXw = nullptr, *dS = nullptr;
    // a batch's warps (gpt_set_warp_batch): SLOT_WB_X / SLOT_WB_S hold warpb_nbatch x Nx x D warped points / warpb_nbatch x Nx slope
    // factors for the next gpt_fit_batch* of that many elements, which consumes them (warpb_nbatch back to 0)
    int warpb_nbatch = 0;
    bool rb_warped = false;            // the resident batch was fitted with warps (gpt_predict_batch refuses it)
    // factorisation state
    int64_t NP = 0;            // padded order (multiple of 128, > N)
    double *dA = nullptr;      // NP x NP, row-major, lower triangle meaningful
    double *d_invd = nullptr;  // (NP/128) x GPT_WS_BLOCK packed workspace (see common.hpp)
    int32_t *d_info = nullptr;
    double *d_y = nullptr, *d_erry = nullptr, *d_scal = nullptr, *d_alpha = nullptr;
    double *h_scal = nullptr;  // pinned
    double *h_yerr = nullptr;  // pinned staging for y | err_y (a pageable source would make the upload synchronous)
    double *h_alpha = nullptr; // pinned landing place of alpha (a pageable destination costs a staged, synchronous copy: ~70 us for 64 KB)
    bool h_alpha_valid = false;
    int32_t *h_info = nullptr; // pinned
    bool factored = false, alpha_valid = false, have_kernel = false;
    bool binv_valid = false;           // SLOT_BINV holds the inverses of the 512x512 diagonal blocks of the resident factor
    bool binv2_valid = false;          // SLOT_BINV2 those of its 1024x1024 diagonal blocks (solves with very few rows)
    bool binv3_valid = false;          // SLOT_BINV3 those of its 2048x2048 diagonal blocks (the same, large factors)
    int64_t dev_gemm_pad = 0;          // dummy LDS (bytes) per workgroup of the device API's GEMM launches on this context (gpt_dev_gemm_nt*):
                                       // a residency cap for the partitioned engines' trailing updates, see "dev_gemm_pad" in gpt_hip.h
    int64_t eager_alpha = 0;           // 1: every evaluation also enqueues alpha = L^-T z behind the factorisation (no second host round trip)
    int64_t binv_early = 0;            // this factorisation: the 512-wide inverses of the diagonal blocks [0, binv_early) were enqueued on the
                                       // main stream under the last panel (enqueue_early_block_inverses); e_binv_early follows them there
    hipEvent_t e_binv_early = nullptr;
    int64_t defer_pad = 1;             // option "defer_pad": 0 keeps the pad leaf of an eager evaluation on the panel stream (A/B; see PotrfRequest)
    // (all three are always built for the whole padded order, floor(NP / width) blocks, whatever extent the caller needs:
    // gpt_ll_grad and the solves ask for different extents at N = 512 k - 128, and a valid flag says nothing about how far)
    unsigned alpha_counter = 0;        // value of the step counter of the wide back-substitution (d_edge[40], only ever raised)
    int64_t debug_poison = 0;          // option "debug_poison": the gradients and gpt_loo* fill their scratch matrices with NaN first (test aid)
    int64_t edge_test_stall = 0;       // option "edge_test_stall": the next head flag is withheld once (test aid, see fit_terms_once)
    double *h_stage = nullptr;         // pinned staging ring for results that go to pageable host memory (2 x GPT_STAGE_BYTES)
    hipStream_t copy_stream = nullptr; // device-to-host copies that overlap the next block's compute (created on first use)
    hipEvent_t cev[4] = {nullptr, nullptr, nullptr, nullptr};
    double *h_batch = nullptr;         // pinned staging of gpt_fit_batch (y, KParams, noise variances, err_y in; results out)
    size_t h_batch_cap = 0;
    // The RESIDENT BATCH: what the last successful gpt_fit_batch* left in SLOT_BATCH_A (factors, augmented row z_b) and
    // SLOT_BATCH_WS (the leaves' packed workspaces), for gpt_predict_batch.  Valid while rb_nbatch > 0 and rb_gen == batch_gen:
    // everything that frees, reuses or outdates those slots (gpt_set_data, gpt_set_T, gpt_release_batch_scratch, gpt_cov_sample,
    // the next gpt_fit_batch* until it succeeds) advances batch_gen.
    uint64_t batch_gen = 1, rb_gen = 0;
    int rb_nbatch = 0;
    int64_t rb_N = 0;
    ModelKernel rb_model;                 // the first element's model: ids, nterms and the product pattern are every element's
    std::vector<KParams> rb_kp, rb_kp2;   // term-major [t][b], the device layout; rb_kp2 (kernel_id -1 where term t is no product) only with rb_model.any_prod
    std::vector<double> rb_nv;            // element noise variances
    int64_t cov_M = 0;                 // > 0: SLOT_KSS holds the lower triangle of the predictive covariance of the last gpt_predict(want = 2, cov_out = NULL)
    ModelKernel model;               // the model kernel of the resident factorisation (gpt_fit, gpt_fit_sum, gpt_fit_terms)
    // The INDUCING-POINT state (api_sparse.inc), beside the dense factor and independent of it: the inducing
    // inputs (SLOT_SP_Z) and, after a gpt_sparse_fit that succeeded, L_u (SLOT_SP_LU), the augmented L_B with c in its row M
    // (SLOT_SP_LB), each with its packed workspace behind the matrix.  gpt_set_data and gpt_sparse_set_inducing drop all of it.
    // The greedy selection of inducing inputs (api_sparse_select.inc) keeps no state here: it works in SLOT_SP_SEL_* and reads the data only.
    int64_t sp_M = 0;                  // inducing points resident (0: none)
    long sp_zmaxsum = 0, sp_zcolmax[GPT_MAX_DIM] = {};      // their largest order row sum / order per coordinate
    bool sp_fitted = false;
    int64_t sp_chunk_rows = 0;         // the chunk_rows argument of the resident sparse fit: its predictions run in the same chunks
    ModelKernel sp_model;              // the model kernel of the resident sparse fit
    int sp_method = 0;                 // ... its method, noise variance and jitter: what gpt_sparse_grad_diff needs beyond the model
    double sp_noise_var = 0.0, sp_jitter = 0.0;
    int sp_ncu = 0;                    // compute units of the device (the Gram kernel's slice count), read on first use
    std::vector<hipEvent_t> sp_events; // phase marks of a timed gpt_sparse_fit (option "timing")
    double timings[5] = {0, 0, 0, 0, 0};
    // per-launch HIP-event timing of the dominant (large) GEMM/SYRK launches, for the roofline line
    int prof_gemm = 0;
    struct GemmProf { hipEvent_t e0, e1, stop; double flops, bytes; };
    std::vector<GemmProf> gprof;
    size_t gprof_used = 0;
    double prof_flops = 0, prof_ms = 0, prof_count = 0, prof_bytes = 0;
    // graph cache for the factorisation
    hipGraphExec_t gexec = nullptr;
    int64_t g_n = 0, g_nb = 0;
    int g_la = 0;
    double *g_A = nullptr;
    DevBuf slots[SLOT_COUNT];
};

// rows per consumer workgroup of a fused leaf with m rows below it, as launch_potf2_trsm's code: 0 = 128, 1 = 64, 2 = 32, 3 = 16
static int strip_rows_code(const gpt_ctx *c, int64_t m) { return m <= c->fuse_rows16 ? 3 : m <= c->fuse_rows32 ? 2 : m <= c->fuse_rows64 ? 1 : 0; }

static int ensure(gpt_ctx *c, int slot, size_t bytes, void **out)
{
    DevBuf &b = c->slots[slot];
    if (b.cap < bytes) {
        if (b.p) GPT_HIP_CHECK(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
        const size_t want = bytes + bytes / 8 + 256;
        GPT_HIP_CHECK(hipMalloc(&b.p, want));
        b.cap = want;
    }
    *out = b.p;
    return GPT_OK;
}

static hipEvent_t get_event(gpt_ctx *c, size_t idx)
{
    while (c->events.size() <= idx) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;      // (timing-capable: an edge can double as a GEMM stop event)
        c->events.push_back(e);
    }
    return c->events[idx];
}

// what the resident factor was good for is gone: alpha (device and host copy) and the three sets of block inverses
static void invalidate_factor(gpt_ctx *c)
{
    c->factored = false;
    c->h_alpha_valid = c->alpha_valid = c->binv_valid = c->binv2_valid = c->binv3_valid = false;
}

// stream `to` continues behind everything enqueued on `from` so far (one record / wait pair on the context's event `idx`)
static int stream_follows(gpt_ctx *c, hipStream_t from, hipStream_t to, size_t idx)
{
    hipEvent_t e = get_event(c, idx);
    if (!e) return GPT_E_HIP;
    GPT_HIP_CHECK(hipEventRecord(e, from));
    GPT_HIP_CHECK(hipStreamWaitEvent(to, e, 0));
    return GPT_OK;
}

#include "api_schedule.inc"      // the factorisation: GEMM driver, flag-edge policy (EvalScope), panels, the look-ahead schedule potrf_enqueue / potrf_run
#include "api_context.inc"      // gpt_ctx_create / destroy / set_option / synchronize, workspace slots
#include "api_kernels.inc"      // Kernel.__call__ and compute_Kij: gpt_kpairs, gpt_kbuild, gpt_kpairs2, gpt_kbuild2
#include "api_fit.inc"      // data residency and the fit: gpt_set_data, gpt_set_T, gpt_fit, gpt_fit_sum, gpt_fit_terms, gpt_fit_matrix
#include "api_batch.inc"      // batched small fits (gpt_fit_batch*), timings / GEMM profile read-out, gpt_get_L, alpha (gpt_get_alpha)
#include "grad_stencil.inc"      // the stencil of the differenced gradients: one parser of its points, one walk of the launch groups
#include "api_grad.inc"      // triangular inverses (gpt_dev_trinv) and the analytic LML gradient gpt_ll_grad
#include "api_loo.inc"      // leave-one-out cross-validation: gpt_loo, gpt_loo_grad_diff
#include "api_grad_batch.inc"      // gpt_ll_grad_diff_batch: the gradient half of a resident batch
#include "api_solve.inc"      // many-right-hand-side solves against the resident factor: block inverses, right-TRSM by GEMMs, split-k; pinned host buffers
#include "api_predict.inc"      // gpt_predict, gpt_cov_sample, gpt_solve_L / gpt_cho_solve, gpt_potrf_host / gpt_gemm_nt_host
#include "api_dev.inc"      // device API (gpt_dev_*): raw device pointers on the context's streams, for the one-process-per-GPU engines
#include "api_sparse.inc"      // inducing-point approximations (FITC / VFE / DTC): gpt_sparse_set_inducing, gpt_sparse_fit, gpt_sparse_predict
#include "api_sparse_batch.inc"      // gpt_sparse_fit_batch: a batch of sparse fits in one launch sequence, gpt_dev_sparse_*_batch
#include "api_sparse_select.inc"      // greedy conditional-variance choice of the inducing inputs: gpt_sparse_select_inducing, gpt_dev_greedy_*
#include "api_sparse_grad.inc"      // the gradient of the sparse objective: gpt_sparse_grad_diff and the device API of its kernels
#include "api_plan.inc"      // compiled schedules of the partitioned engines: gpt_plan_* (op list replay, RCCL called directly)
#include "api_ensemble.inc"      // gpt_ensemble_run: the ensemble sampler's loop (ensemble.hpp) around the batched fit
