// common.hpp -- shared declarations for libgpt_hip.so (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/gpt_hip.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

#define GPT_WAVE 64
// Per 128-column diagonal block the factorisation leaves a packed workspace ("ws") of GPT_WS_BLOCK doubles:
//   [0, 2048)     inverses of the eight 16x16 diagonal blocks of L_kk,
//   [2048, 9216)  the 28 strictly-lower 16x16 blocks of L_kk (block (j, c), c < j, at index j(j-1)/2 + c),
// every 16x16 block stored in MFMA B-operand lane order: element (r, c) at [c / 4][r + 16 * (c % 4)], so that a
// fragment is 512 contiguous bytes for the panel TRSM.
#define GPT_WS_BLOCK 9216
#define GPT_WS_LOFF 2048

void gpt_set_error(const char *fmt, ...);

#define GPT_HIP_CHECK(expr)                                                              \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            gpt_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return (e_ == hipErrorOutOfMemory) ? GPT_E_NOMEM : GPT_E_HIP;                \
        }                                                                                \
    } while (0)

#define GPT_LAUNCH_CHECK()                                                               \
    do {                                                                                 \
        hipError_t e_ = hipGetLastError();                                               \
        if (e_ != hipSuccess) {                                                          \
            gpt_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
            return GPT_E_HIP;                                                            \
        }                                                                                \
    } while (0)

// Kernel hyperparameters as passed by value to the device kernels.
struct KParams {
    int kernel_id;
    int D;
    int hyper_deriv;      // -1 = None
    int symmetric;        // DiagonalNoiseKernel only fires for symmetric calls
    double sigma;         // params[0]
    double alpha;         // RationalQuadraticKernel: params[1]
    union {
        struct {
            double l[GPT_MAX_DIM];      // length scales (SE / M52)
            double inv_l[GPT_MAX_DIM];  // 1 / l
            double inv_var[GPT_MAX_DIM];// 1 / l^2
        };
        // bucket, exp-Gauss, B-spline and nested-GP Gibbs kernels (1-D, no length scales of the kind above): the parameters after sigma_f as the ABI
        // hands them over (gibbs_lfunc.hpp reads them raw).  In the place of the three arrays, so that sizeof(KParams) is what it
        // was: the product kernels keep both factors' KParams on the stack and pay for every byte in scratch
        double g_raw[3 * GPT_GIBBS_MAX_GAUSS + 1];
    };
    int noise_n[GPT_MAX_DIM];   // DiagonalNoiseKernel.n
    // MaternKernel (general nu): nu = alpha; constants of make_kparams (api.hip)
    double m_cnu;             // 2^(1-nu) / Gamma(nu)
    double m_mu;              // nu - round(nu), |mu| <= 1/2
    int m_nint;               // round(nu)
    int m_isint;              // nu is an integer (the reference then averages nu -+ 0.001 near the origin)
    int zero_l;               // some length scale is exactly 0 (1 / l = inf): the squared-exponential pair function then applies the
    int inf_l;                //   reference's 0/0 -> 0 rule per dimension (core.py:416); otherwise it is one multiply
                              // inf_l (MaternKernel only: set and read for no other kernel): some length scale is +inf (1 / l = 0: a
                              //   masked-out dimension, gpt_hip.h) -- the Matern pair function then returns 0.0 for an order in such a dimension in front of its r = 0 classes
    double m_gampl, m_gammi, m_gam1, m_gam2;      // Temme's 1/Gamma(1 +- mu) and their combinations
    double m_g[2], m_gm[2], m_nus[2];             // Gamma(nu_s), Gamma(-nu_s), nu_s for the small-y series (nu_s = nu, or nu -+ 0.001)
    // Gibbs kernels (1-D): l(x) = g_c + sum_q g_amp[q] tanh((x - g_x0[q]) / g_w[q]) over g_nt terms (1: tanh warp, 2: double tanh)
    double g_amp[2], g_w[2], g_x0[2], g_c;
    int g_nt, g_dim;       // (exp-Gauss: g_nt = the number of Gaussians; B-spline: the number of knots; nested GP: of points); g_dim: the coordinate the
                           // kernel acts on (GPT_KERNEL_ON_DIM, num_dim 2 .. GPT_GIBBS_ON_DIM_MAX_D; 0 for a plain id)
};

static_assert(3 * GPT_GIBBS_MAX_GAUSS + 1 <= 3 * GPT_MAX_DIM, "g_raw must fit the arrays it shares its place with");
static_assert(2 * GPT_GIBBS_MAX_KNOTS + 2 <= 3 * GPT_GIBBS_MAX_GAUSS + 1, "the B-spline's knots and coefficients must fit g_raw");
static_assert(2 * GPT_GIBBS_MAX_GP_POINTS + 1 <= 3 * GPT_GIBBS_MAX_GAUSS + 1, "the nested GP's length scale, points and weights must fit g_raw");
static_assert(sizeof(KParams) == 656, "KParams travels by value in the kernel arguments (two per product term)");

// the Gibbs kernels (1-D, derivative orders <= 1): the tanh warps, the buckets, the exponential of Gaussians, the B-spline, the nested GP
__host__ __device__ constexpr bool gibbs_kid(int kid)
{
    return kid == GPT_KERNEL_GIBBS_TANH || kid == GPT_KERNEL_GIBBS_DTANH || kid == GPT_KERNEL_GIBBS_CUBIC ||
           kid == GPT_KERNEL_GIBBS_QUINTIC || kid == GPT_KERNEL_GIBBS_EXPGAUSS || kid == GPT_KERNEL_GIBBS_BSPLINE ||
           kid == GPT_KERNEL_GIBBS_GP;
}

// ... those of them added after the tanh warps (kernel ids 9-11), and the builder's INTERNAL id of a product with such a factor
// (never in the ABI): the single-matrix product kernels at num_dim 1 were already out of registers, and carrying the three
// extra length-scale branches cost them ~350 bytes more scratch per lane whatever the model.  So a product kernel
// compiles those branches only as GPT_KID_PRODUCT_GM, which the launchers choose when a factor needs them (kbuild_prod.hip);
// GPT_KERNEL_PRODUCT is the code it was.  The batched kernels (kbuild_batch.hip), whose registers had room, take
// GPT_KID_PRODUCT_GM for every 1-D product: same registers, same scratch as before.
__host__ __device__ constexpr bool gibbs_more_kid(int kid)
{
    return kid == GPT_KERNEL_GIBBS_CUBIC || kid == GPT_KERNEL_GIBBS_QUINTIC || kid == GPT_KERNEL_GIBBS_EXPGAUSS;
}
#define GPT_KID_PRODUCT_GM 106
// ... and a product with a B-spline factor (id 12): the spline costs registers again, in the batched kernels too, so it has an
// instantiation of its own everywhere -- the builders' GPT_KID_PRODUCT_GB, the B-spline forms of kdiag_batch / kss_sum
// (kbuild_batch.hip) -- which the launchers take only for a model that holds a kernel of these forms (ModelKernel::has_gb, gibbs_gb_kid below); GPT_KERNEL_PRODUCT,
// GPT_KID_PRODUCT_GM and the batched kernels of every other model are the code they were
#define GPT_KID_PRODUCT_GB 107
// The nested-GP kernel (id 13) rides with the B-spline: compiled into GPT_KID_PRODUCT_GM and kss_sum / kdiag_batch<1> it took their
// scratch from 736 to 1488 bytes and the single-matrix GM product from 512 to 256 VGPRs at 2080 bytes (profiles/gibbs_gp_resource_usage.txt),
// in kernels every 1-D model runs; as a second out-of-line call in front of the GB forms' switch every kernel keeps its record.
// GPT_GFORM_GB says "a kernel of the GB forms among them".
__host__ __device__ constexpr bool gibbs_gb_kid(int kid)
{
    return kid == GPT_KERNEL_GIBBS_BSPLINE || kid == GPT_KERNEL_GIBBS_GP;
}
// what the launchers are told about the Gibbs kernels of a model or a product (their `gform` argument; ModelKernel::gibbs_form(),
// gibbs_form_of): GPT_GFORM_GB, a kernel of the GB forms -- a B-spline or a nested GP, gibbs_gb_kid -- among them; GPT_GFORM_ON_DIM, a Gibbs factor on one coordinate of num_dim > 1
// (GPT_KERNEL_ON_DIM, gpt_hip.h)
#define GPT_GFORM_GB 1
#define GPT_GFORM_ON_DIM 2
// The periodic kernel (id 14) as a product factor or as a term whose id only the device sees (kdiag_batch / kss_sum) likewise has forms
// of its own: the builders' GPT_KID_PRODUCT_PER and the PER forms of those two kernels, taken only for a product / a model that holds
// a Periodic kernel (GPT_GFORM_PER; ModelKernel::has_per) -- every other instantiation is the code it was.  ONE form per num_dim: it
// carries every branch of factor_pair (the GM and GB ones too), so a model may hold Periodic terms beside Gibbs terms.
// The spectral kernel (id 15) shares these forms: a second test beside the periodic one, an out-of-line call, no instantiation of its own
// (profiles/spectral_resource_usage.txt: what that changed for the PER forms, and that every other kernel is the code it was).
#define GPT_KID_PRODUCT_PER 108
#define GPT_GFORM_PER 4

// A cross-stream edge without an event: the kernel that completes a piece of work raises a 32-bit word in device
// memory when its LAST workgroup is through (its results written with write-through stores and drained first) and the
// consumer polls that word -- inside its first kernel, or in a one-wave wait kernel in front of it (launch_wait_flag).
// Measured (scratch/waitvalue_probe.hip): producer end -> consumer start 1.5 us and nothing added to the producer's own
// stream, against 7.6-9.1 us and 1.7-4.5 us for a stop event on the dispatch packet + hipStreamWaitEvent.
// word[0] = the flag (only ever raised), word[1] = workgroup counter.
//
// Memory ordering.  Producer: the payload is written with agent-scope (write-through, sc1) stores, every wave drains its
// own (s_waitcnt vmcnt(0)) before the barrier, then ONE thread raises the word -- no release fence: on gfx950 that is
// buffer_wbl2, a write-back of every dirty line of the XCD's L2 (1.7-6 us per hand-over, measured) for data that is
// already in memory.  Consumer: whatever it reads of the payload BEHIND the flag inside the same kernel must not come from
// a line cached before the producer wrote it.  Two forms: (a) the payload is read with agent-scope (sc1, cache-bypassing)
// loads -- the GEMM waiter's C tile, the TRSM consumers' packed blocks -- and nothing else is needed; (b) the payload is read
// with plain loads (the first diagonal-block kernel of a factorisation: its 128 x 128 block and rows) and the polling
// thread issues an agent-scope ACQUIRE fence (buffer_inv sc1) after it has seen the value and before the workgroup
// barrier (edge_poll<.., true>).  The fence is NOT free for the rest of the chip -- it drops the non-coherent lines of the
// whole XCD's L2, i.e. the operand panels of a trailing update running there: issued by every workgroup of the panel
// stream's waiting GEMM launches it cost 10 % of an evaluation at N = 8192 (4.96 against 4.50 ms, same-box A/B) -- so it is
// used only in form (b), once per evaluation and workgroup.  A stream-side wait (wait_flag_kernel) needs neither: the
// kernel behind it starts with the dispatch packet's own acquire.
//
// Every wait is BOUNDED: a kernel that waits for another kernel never ends if the other one cannot run -- a tool that runs
// one kernel at a time, queues oversubscribed by other processes on the GPU, a lost launch.  After GPT_EDGE_TIMEOUT_TICKS of
// the 100 MHz wall clock the waiter raises `*err`, stops waiting and carries on (on data that may be incomplete); the host
// finds the error word at the end of the evaluation, switches the process to event edges for good and runs the
// evaluation again (api.hip: EvalScope / fit_terms).
struct EdgeSig {
    unsigned *word = nullptr;
    unsigned value = 0;
    unsigned *err = nullptr;      // waits only: raised when the wait timed out
};
#define GPT_EDGE_TIMEOUT_TICKS 25000000ll      // 250 ms
// device side: called by every workgroup that takes part, after its results are stored (all threads of the workgroup)
#ifdef __HIPCC__
__device__ __forceinline__ void edge_signal(unsigned *word, unsigned value, unsigned total)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's (write-through) stores have been acknowledged
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned done = __hip_atomic_fetch_add(word + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
        if (done == total) {
            __hip_atomic_store(word + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(word, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
// Consumer side, ONE thread of the workgroup (the caller follows with __syncthreads()): poll until *word >= value (signed
// difference: the words only ever go up), SLEEP = s_sleep argument between polls; bounded; ACQUIRE: see above.
template <int SLEEP, bool ACQUIRE>
__device__ __forceinline__ void edge_poll(const unsigned *word, unsigned value, unsigned *err)
{
    if ((int)(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - value) < 0) {
        const long long t0 = wall_clock64();
        while ((int)(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - value) < 0) {
            __builtin_amdgcn_s_sleep(SLEEP);
            if (err && wall_clock64() - t0 > GPT_EDGE_TIMEOUT_TICKS) {
                __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
            }
        }
    }
    if (ACQUIRE) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}
#endif

// ---- launchers implemented in the .hip files (all asynchronous on `st`) -------------------
int launch_kpairs(hipStream_t st, const KParams &kp, const double *dXi, const double *dXj,
                  const int32_t *dni, const int32_t *dnj, int64_t M, double *dout, int accumulate = 0,
                  const KParams *kp2 = nullptr);      // kp2 (kernel_id >= 0): the pair list of the product kp * kp2
// One block of the covariance builder: rows Xi / ni (M points), columns Xj / nj (P points), written to K (row stride ldk).
// lower_only: skip the tiles strictly above the diagonal of the whole matrix, in which this block starts at (i0, j0); err_y != NULL:
// the diagonal epilogue ((K + noise_var) + err_y^2) + diag_add; accumulate: add to what K holds (a later term of a sum).
// Si / Sj (both or neither): Xi / Xj are WARPED points, these their slope factors (warp.hpp; the fit kernels only).
struct KBuildArgs {
    const double *Xi;
    const int32_t *ni;
    int64_t M;
    const double *Xj;
    const int32_t *nj;
    int64_t P;
    int lower_only;
    int64_t i0, j0;
    const double *err_y;
    double noise_var, diag_add;
    double *K;
    int64_t ldk;
    int accumulate = 0;
    const double *Si = nullptr, *Sj = nullptr;
};
int launch_kbuild(hipStream_t st, const KParams &kp, const KParams *kp2, const KBuildArgs &a);      // kp2 (kernel_id >= 0): kp * kp2
int launch_check_orders(hipStream_t st, const int32_t *dn, int64_t M, int D, int32_t *d_flag);
int launch_gemm_nt(hipStream_t st, int64_t m, int64_t n, int64_t k, double alpha, const double *A, int64_t lda,
                   const double *B, int64_t ldb, double beta, double *C, int64_t ldc, int tri, int force_tile, int lds_pad,
                   hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, int prio = 0, EdgeSig edge = EdgeSig(),
                   EdgeSig wait = EdgeSig(), int64_t edge_cols = 0, int64_t nbatch = 1, int64_t bstride = 0,
                   EdgeSig tail = EdgeSig(), int64_t bstride_b = -1, int64_t bstride_c = -1,       // batch strides of B / C (< 0: bstride)
                   int64_t m_live = -1);      // tri launches: only the first m_live rows are computed (< 0: all m), see gemm.hip
int launch_potf2_diag(hipStream_t st, double *A, int64_t lda, double *invd, int32_t *info, int64_t info_base,
                      EdgeSig wait = EdgeSig(), int64_t nbatch = 1, int64_t bstride_a = 0, int64_t bstride_ws = 0);
int launch_gemm_nt_stair(hipStream_t st, int64_t m, int64_t nseg, int64_t seg_cols, int64_t k, double alpha,
                         const double *A, int64_t lda, const double *B, int64_t ldb, int64_t b_stride, int64_t row_step,
                         double beta, double *C, int64_t ldc, int lds_pad, hipEvent_t ev0 = nullptr,
                         hipEvent_t ev1 = nullptr);
int launch_gemm_nt_gridstair(hipStream_t st, int64_t m, int64_t nseg, int64_t seg_cols, int64_t k, double alpha, const double *A,
                             int64_t lda, const double *B, int64_t ldb, int64_t off, int64_t num, int64_t den, int64_t base,
                             double beta, double *C, int64_t ldc, int lds_pad, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
int launch_potf2_trsm(hipStream_t st, double *A, int64_t lda, double *invd, int32_t *info, int64_t info_base, int64_t m,
                      unsigned *flag, unsigned flag_base, hipEvent_t done = nullptr, EdgeSig edge = EdgeSig(),
                      EdgeSig wait = EdgeSig(), int rows64 = 0);
// (batched: element y of the grid works on B + y * bstride_b with the workspace invd + y * bstride_ws; L itself is never read --
// the packed workspace carries the block -- so B's stride is the only matrix stride: inside the factor for the batched fit,
// the element's columns of V for gpt_predict_batch)
int launch_trsm_panel(hipStream_t st, int64_t m, const double *L, int64_t ldl, const double *invd,
                      double *B, int64_t ldb, hipEvent_t done = nullptr, EdgeSig edge = EdgeSig(), int64_t nbatch = 1,
                      int64_t bstride_b = 0, int64_t bstride_ws = 0);
// batched small fits (gpt_fit_batch)
int launch_kbuild_batch(hipStream_t st, int kernel_id, int D, const KParams *d_kps, const double *d_noise_var, int64_t nbatch,
                        const double *dX, const int32_t *dn, int64_t N, const double *d_err_y, double diag_add, double *dK,
                        int64_t ldk, int64_t bstride, int accumulate = 0, int full = 0, const KParams *d_kps2 = nullptr,
                        int64_t xstride = 0, const double *dS = nullptr, int64_t sstride = 0, int gform = 0);
                        // dS != NULL: a warped batch -- element z's (warped) points at dX + z * xstride, its slopes at dS + z * sstride
int launch_batch_pad(hipStream_t st, const double *h_y, int64_t nbatch, double *A, int64_t lda, int64_t bstride, int64_t n_valid,
                     int64_t n_pad, double big, int32_t *info);
// the predictive half of a resident batch (gpt_predict_batch)
int launch_kbuild_batch_cross(hipStream_t st, int kernel_id, int D, const KParams *d_kps, const double *d_nv, int64_t nbatch,
                              const double *dXi, const int32_t *dni, int64_t M, const double *dXj, const int32_t *dnj, int64_t P, double *dK,
                              int64_t ldk, int64_t bstride, int accumulate = 0, const KParams *d_kps2 = nullptr, int gform = 0);
                              // gform (here and below): ModelKernel::gibbs_form(), GPT_GFORM_* bits -- the kernels with those branches
int launch_kdiag_batch(hipStream_t st, int D, int nterms, const KParams *d_kps, const KParams *d_kps2, int64_t nbatch, const double *dX,
                       const int32_t *dn, int64_t M, double *dout, int64_t ldo, int gform = 0);
int launch_kss_sum(hipStream_t st, int D, int nterms, const KParams *d_kps, const KParams *d_kps2, int64_t nbatch, const int32_t *d_keep,
                   const double *dX, const int32_t *dn, int64_t M, int64_t MP, const int32_t *d_hit, double noise_sum, double *dC,
                   int64_t ldc, int gform = 0);
int launch_batch_meanvar(hipStream_t st, int64_t M, int64_t MP, int64_t N, int64_t NP, int64_t nbatch, double *V, int64_t ldv,
                         const double *A, int64_t bs, const int32_t *keep, double *mean, double *var, int64_t ld);
int launch_batch_logdet_dot(hipStream_t st, const double *A, int64_t lda, int64_t bstride, int64_t n, int64_t nbatch,
                            const int32_t *d_info, double *out3);
#define GPT_GRAD_MAXH 8
int grad_reduce_blocks(int64_t N);
int launch_grad_reduce(hipStream_t st, const KParams &kp, int nh, const int *hl, const double *dX, const int32_t *dn,
                       int64_t N, const double *dalpha, const double *dW, int64_t ldw, double *dpartial);
// the pair pass of gpt_ll_grad_diff (kgrad.hip): nh <= GPT_GRAD_MAXH parameters of one term id1 (* id2 where id2 >= 0), 2 nh KParams in
// device memory per factor (the term at the stencil points a, b of every parameter); dpartial as launch_grad_reduce
int launch_kgrad_diff(hipStream_t st, int id1, int id2, int D, const KParams *d_kps, const KParams *d_kps2, int nh, const double *dX,
                      const int32_t *dn, int64_t N, const double *dalpha, const double *dW, int64_t ldw, double *dpartial, int64_t nbatch = 1,
                      const double *du = nullptr);      // du: the leave-one-out weights (gpt_loo_grad_diff), see kgrad.hip kgrad_weight
// ... of a resident batch (gpt_ll_grad_diff_batch; kgrad.hip): launch_kgrad_diff with nbatch elements in the grid's second dimension
// (element e: d_kps + 2 nh e, dalpha + e ldw, dW + e ldw^2, dpartial + e grad_reduce_blocks(N) (GPT_GRAD_MAXH + 1)), alpha_b = U_b z_b
// and the sum of the partial rows in index order on the device
int launch_kgrad_batch_alpha(hipStream_t st, const double *dU, int64_t ldu, int64_t su, const double *dA, int64_t lda, int64_t sa,
                             int64_t N, int64_t nbatch, double *dalpha, int64_t sal);
int launch_kgrad_batch_finish(hipStream_t st, const double *dpartial, const int32_t *dsrc, int nout, int64_t nblk, int64_t nbatch,
                              double *dout);
// the leave-one-out entry points (kloo.hip): d_i = sum_{i <= k < N} U_ik^2, r = alpha / d, se = sqrt((1 + alpha^2 / d) / d) and the rows'
// terms of L_LOO over the NP rows of U = L^-T (rows >= N: 1, 0, 0, 0), out1[0] the first N terms added in index order; A = W diag(se)
int launch_loo_terms(hipStream_t st, const double *dU, int64_t ldu, const double *dalpha, int64_t N, int64_t NP, double *d, double *r,
                     double *se, double *term, double *out1);
int launch_loo_scale_cols(hipStream_t st, const double *dW, int64_t ldw, const double *se, int64_t n, double *dA, int64_t lda);
int launch_add_diag(hipStream_t st, double *A, int64_t lda, int64_t n, const double *err, double diag_add, int64_t nbatch = 1,
                    int64_t bstride = 0);
// Test aid (GPT_JITTER=<max microseconds> in the environment): a delay kernel of random length on `st`, called in front of
// every dense launch.  The schedules express every dependency as an event, so results must not move with the relative
// timing of the streams; a missing edge shows up as a wrong number (tests/test_gpu_parity.py).  Off: one branch.
void gpt_jitter(hipStream_t st);
int launch_set_flag(hipStream_t st, unsigned *word, unsigned value);
// One-wave kernel on `st` that waits (bounded, see EdgeSig) until *w.word >= w.value: the stream-side end of a flag edge.
int launch_wait_flag(hipStream_t st, EdgeSig w);
int gemm_small_threshold();      // 64x64-tile count under which launch_gemm_nt cuts a launch into 32x32 tiles (gemm.hip)
int launch_upload_pad(hipStream_t st, const double *h_src, double *d_dst, int64_t ncopy, int32_t *info, double *A,
                      int64_t lda, int64_t n_valid, int64_t n_pad, double big);
int launch_fill_pad(hipStream_t st, double *A, int64_t lda, int64_t n_valid, int64_t n_pad, const double *dy,
                    double big);
int launch_logdet_dot(hipStream_t st, const double *A, int64_t lda, int64_t n, const int32_t *d_info, double *d_part,
                      double *out4, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, unsigned *edge_err = nullptr);
int launch_extract_lower(hipStream_t st, const double *A, int64_t lda, int64_t n, double *out, int64_t ldo);
int launch_trsv_lt(hipStream_t st, int64_t n, const double *L, int64_t ldl, const double *invd, double *x, int64_t b_lo = 0);
int launch_trsv_lt_wide(hipStream_t st, int64_t nwide, const double *L, int64_t ldl, const double *U, double *w, double *x,
                        const double *w0 = nullptr);
int launch_alpha_init(hipStream_t st, int64_t n, int64_t np, const double *z, double *w, double *x);
int launch_gemv_n(hipStream_t st, int64_t m, int64_t n, const double *A, int64_t lda, const double *x, double *y);
int launch_trinv512(hipStream_t st, int64_t nblk, const double *L, int64_t ldl, const double *invd, double *U, double *W);
int launch_rowsumsq_sub(hipStream_t st, int64_t m, int64_t n, const double *V, int64_t ldv, const double *kdiag,
                        double *var_out);
int launch_add_noise_sym(hipStream_t st, const KParams &kp, const double *dX, const int32_t *dn, int64_t M,
                         double *C, int64_t ldc);
int launch_mirror_rows(hipStream_t st, double *A, int64_t lda, int64_t c0, int64_t w, int64_t n);
int launch_alpha_trace(hipStream_t st, const double *alpha, const double *W, int64_t ldw, int64_t n, double *out);
int launch_diag_gather(hipStream_t st, const double *A, int64_t lda, int64_t n, double *out);
int launch_copy2d(hipStream_t st, int64_t rows, int64_t cols, const double *src, int64_t lds, double *dst, int64_t ldd);
int launch_zero2d(hipStream_t st, int64_t rows, int64_t cols, double *dst, int64_t ldd);
int launch_pad_block(hipStream_t st, double *A, int64_t lda, int64_t c0, int64_t nb, int64_t n_valid, int64_t n_pad,
                     const double *dy, double big);
int launch_row_sumsq(hipStream_t st, const double *row, int64_t w, double *acc);
// the inducing-point path (ksparse.hip)
int launch_sparse_lambda(hipStream_t st, double *V, int64_t ldv, int64_t rows, int64_t M, int method, const double *kdiag,
                         const double *r, const double *err, double noise_var, double *rowval, int64_t ldr, int32_t *bad);
int launch_sparse_rowsum(hipStream_t st, const double *rowval, int64_t ldr, int64_t rows, double *acc);
// (A == NULL: G += V^T V, the fit's instantiation; else G += A^T V, the gradient's signed-weight Gram)
int launch_sparse_gram(hipStream_t st, const double *A, const double *V, int64_t ldv, int64_t rows, int64_t mg, int nslices, double *part,
                       double *G, int64_t ldg);
// the lower 64 x 64 tiles of a Gram of order mg
inline int64_t sparse_gram_tiles(int64_t mg) { return (mg / 64) * (mg / 64 + 1) / 2; }
// how a Gram over `rows` rows asked for in nslices slices is cut: whole k-steps of four rows per slice and no slice empty, so ns <=
// nslices slices of slice_rows rows.  The bits of G depend on it (the partials are added in slice order): the one statement of the rule
struct SparseSlicing {
    int64_t slice_rows;
    int ns;
};
inline SparseSlicing sparse_gram_slicing(int64_t rows, int nslices)
{
    const int64_t slice_rows = ((rows + nslices - 1) / nslices + 3) / 4 * 4;
    return SparseSlicing{slice_rows, (int)((rows + slice_rows - 1) / slice_rows)};
}
// ... and the doubles of its workspace `part`: one 64 x 64 partial tile per (slice, lower tile), sized for nslices
inline int64_t sparse_gram_part_doubles(int64_t mg, int nslices) { return (int64_t)nslices * sparse_gram_tiles(mg) * 4096; }
int launch_sparse_assemble_b(hipStream_t st, const double *G, int64_t ldg, int64_t M, double *B, int64_t bp, double big);
int launch_sparse_var(hipStream_t st, const double *V, const double *W, int64_t ld, int64_t rows, int64_t M, const double *kdiag,
                      double *var);
// ... for a batch of fits (gpt_sparse_fit_batch): the element in a grid dimension, element b on V + b vstride, kdiag + b
// kstride, r + b rstride, rowval + b rvstride, bad[b], acc + b astride, part + b pstride, G + b gstride, B + b bstride.  Each pair of
// launchers goes through one helper and one kernel source (ksparse.hip), so an element's bits are those of the launchers above
int launch_sparse_lambda_batch(hipStream_t st, int64_t nbatch, double *V, int64_t ldv, int64_t vstride, int64_t rows, int64_t M, int method,
                               const double *kdiag, int64_t kstride, const double *r, int64_t rstride, const double *err,
                               const double *noise_var, double *rowval, int64_t ldr, int64_t rvstride, int32_t *bad);
int launch_sparse_rowsum_batch(hipStream_t st, int64_t nbatch, const double *rowval, int64_t ldr, int64_t rvstride, int64_t rows, double *acc,
                               int64_t astride);
int launch_sparse_gram_batch(hipStream_t st, int64_t nbatch, const double *V, int64_t ldv, int64_t vstride, int64_t rows, int64_t mg, int nslices,
                             double *part, int64_t pstride, double *G, int64_t ldg, int64_t gstride);
int launch_sparse_assemble_b_batch(hipStream_t st, int64_t nbatch, const double *G, int64_t ldg, int64_t gstride, int64_t M, double *B, int64_t bp,
                                   int64_t bstride, double big);
int launch_sparse_unit_pad_batch(hipStream_t st, int64_t nbatch, double *A, int64_t lda, int64_t bstride, int64_t n_valid, int64_t n_pad);
// ... and the gradient of its objective (gpt_sparse_grad_diff): the per-row pass, the rank-one part of A_fu,
// L_B without its augmented rows, the middle factor of A_uu (ksparse.hip) and the rectangular pair
// pass with its running sums (kgrad_rect.hip)
int launch_sparse_grad_rows(hipStream_t st, const double *V, const double *W, int64_t ld, int64_t rows, int64_t M, int method,
                            const double *kdiag, const double *r, const double *err, double noise_var, const double *t, double *alpha,
                            double *e_out, double *gval, int64_t ldr, double *S1, double *S2, int32_t *bad);
int launch_sparse_rank1(hipStream_t st, double *A, int64_t lda, int64_t rows, int64_t M, const double *alpha, const double *beta);
int launch_sparse_tril(hipStream_t st, const double *src, int64_t lds, int64_t n, double *dst, int64_t ldd, int64_t np);
int launch_sparse_grad_mid(hipStream_t st, const double *Binv, int64_t ldb, const double *E, int64_t lde, int64_t M, int mode, double *Mid,
                           int64_t np);
int64_t kgrad_rect_blocks(int64_t rows, int64_t M);
int launch_kgrad_rect_diff(hipStream_t st, int id1, int id2, int D, const KParams *d_kps, const KParams *d_kps2, int nh, const double *dX,
                           const int32_t *dnx, int64_t rows, const double *dZ, const int32_t *dnz, int64_t M, const double *dA, int64_t lda,
                           const double *de, double *dpartial, double *dacc);
// the pair pass of gpt_sparse_grad_z (kgrad_dz.hip): ddz[m][d] += sum_i dA[i][m] k(x_i, z_m; n_i, n_m + e_d) for ONE term id1
// (* id2 where id2 >= 0) at its parameters k1 (k2); skip_diag: without the pairs i == m (the Z-Z pass, X := Z).  dpartial:
// kgrad_dz_tiles(rows) x M x D doubles
int64_t kgrad_dz_tiles(int64_t rows);
int launch_kgrad_dz(hipStream_t st, int id1, int id2, int D, const KParams &k1, const KParams *k2, const double *dX, const int32_t *dnx,
                    int64_t rows, const double *dZ, const int32_t *dnz, int64_t M, const double *dA, int64_t lda, int skip_diag,
                    double *dpartial, double *ddz);
// 2 A_uu = S - beta beta^T whole (ksparse.hip): S read in its lower triangle
int launch_sparse_auu2(hipStream_t st, const double *S, int64_t lds, int64_t M, const double *beta, double *dst, int64_t ldd);
// greedy conditional-variance selection of inducing inputs (kgreedy.hip): a column-major factor (column stride ld >= rows),
// one partial per GREEDY_WG rows -- part[b] the largest residual, pidx[b] the lowest row at it, part[nparts + b] the sum of max(., 0) --
// scal / words as GPT_GREEDY_S_* / GPT_GREEDY_W_* (gpt_hip.h) index them
#define GREEDY_WG GPT_GREEDY_ROWS_PER_PART
#define GREEDY_UNROLL 16
int64_t greedy_blocks(int64_t rows);
int launch_greedy_init(hipStream_t st, int64_t rows, const double *resid, int32_t *mark, double *part, int32_t *pidx);
int launch_greedy_update(hipStream_t st, const double *L, int64_t ld, int64_t rows, int64_t j, double *col, double *resid, const int32_t *mark,
                         const double *prow, const double *scal, const int32_t *words, double *part, int32_t *pidx);
int launch_greedy_pick(hipStream_t st, int64_t j, int64_t M, double tol, const double *part, const int32_t *pidx, int64_t nparts,
                       const int32_t *cand, const double *X, int D, const double *L, int64_t ld, int32_t *mark, double *scal, int32_t *words,
                       int32_t *idx, double *dmax, double *trace, double *xp, double *prow);
int launch_greedy_gather(hipStream_t st, const double *X, const int32_t *cand, int64_t ncand, int D, double *Xc, int32_t *nc);
int launch_panel_scalars(hipStream_t st, const double *P, int64_t ldp, int64_t w, int64_t zrow, double *acc);
