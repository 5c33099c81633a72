// api_plan.inc -- part of api.hip (ONE translation unit).  Compiled schedules of the partitioned engines: gpt_plan_* (VERDICT r5 #4).
// ------------------------------------------------------------------------------------------------
// The one-process-per-GPU block-cyclic Cholesky (gptools_amd/dist.py) issues ~1000 operations per rank and evaluation -- kernels
// of this library on two or three in-order queues, events between them, one panel exchange per step.  Which operations, on which
// buffers, in which order is STATIC per (N, nb, world, rank, options): the Python layer walks its step loop ONCE against a
// recorder, which yields an op list of fixed-size integer records (addresses, sizes, bit patterns of doubles), and every
// evaluation afterwards is one call of gpt_plan_run: a C loop over that list -- no interpreter, no framework dispatch, no
// per-op ctypes marshalling between the launches (host enqueue per N = 32768 evaluation: profiles/r06_plan_host.txt).
//
// The panel exchange is RCCL, called DIRECTLY from here (librccl is dlopen'ed: the library has no link-time dependency on it
// and single-GPU users never load it).  A plan has up to GPT_PLAN_CHANNELS communication CHANNELS, each one communicator
// (ncclCommInitRank with an id the Python layer distributes over its own process groups) with a dedicated high-priority stream:
// the 1-D engine uses one (all ranks), the 2-D engine five (process row: bulk rows / early block; process column: inverse of the
// diagonal block / column exchange; the whole grid: head blocks) -- transfers of different kinds never queue behind each other.
// A collective op waits (event) for the queue it was issued from, runs on its channel's stream and records an event the
// consumers wait for -- the dependency structure torch.distributed's asynchronous collectives give the Python-driven schedule,
// without the framework.
//
// Record layout: GPT_PLAN_W int64 per op: [opcode, queue, a0 .. a17]; doubles travel as their bit patterns.  Queues: 0 main,
// 1 panel, 2 recv (the contexts handed to gpt_plan_create, in this order), 3 + c = the stream of communication channel c.
// The per-evaluation inputs (kernel id, hyperparameters, noise variance, diagonal loading) are arguments of gpt_plan_run and
// reach the K-builder ops at replay time; X, n, err_y are device arrays fixed at plan creation.
// ------------------------------------------------------------------------------------------------
#include <dlfcn.h>

#define GPT_PLAN_W 20
#define GPT_PLAN_CHANNELS 8
enum { GPT_OP_RECORD = 0, GPT_OP_WAIT, GPT_OP_KBUILD, GPT_OP_PAD, GPT_OP_COPY2D, GPT_OP_POTRF_PANEL, GPT_OP_TRINV, GPT_OP_GEMM,
       GPT_OP_STAIR, GPT_OP_SCALARS, GPT_OP_BCAST, GPT_OP_SCATTER, GPT_OP_ALLGATHER, GPT_OP_KRECT, GPT_OP_ROWSUMSQ, GPT_OP_GRIDSTAIR,
       GPT_OP_COUNT };

// ---- RCCL through dlopen ----------------------------------------------------------------------
typedef struct { char internal[128]; } gpt_nccl_id;
typedef void *gpt_nccl_comm;
struct RcclApi {
    void *handle = nullptr;
    int (*GetUniqueId)(gpt_nccl_id *) = nullptr;
    int (*CommInitRank)(gpt_nccl_comm *, int, gpt_nccl_id, int) = nullptr;
    int (*CommDestroy)(gpt_nccl_comm) = nullptr;
    int (*Broadcast)(const void *, void *, size_t, int, int, gpt_nccl_comm, hipStream_t) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, gpt_nccl_comm, hipStream_t) = nullptr;
    int (*Send)(const void *, size_t, int, int, gpt_nccl_comm, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, gpt_nccl_comm, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
#define GPT_NCCL_DOUBLE 8      // ncclFloat64 (nccl.h: ncclDouble = 8)

static RcclApi *rccl_api()
{
    static RcclApi api;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (api.handle) return &api;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void *h = nullptr;
    for (const char *n : names)
        if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL)) != nullptr) break;
    if (!h) {
        gpt_set_error("gpt_plan: librccl.so not found (%s)", dlerror());
        return nullptr;
    }
#define GPT_RCCL_SYM(field, name)                                                   \
    *(void **)(&api.field) = dlsym(h, name);                                        \
    if (!api.field) {                                                               \
        gpt_set_error("gpt_plan: symbol %s missing from librccl", name);            \
        dlclose(h);                                                                 \
        return nullptr;                                                             \
    }
    GPT_RCCL_SYM(GetUniqueId, "ncclGetUniqueId")
    GPT_RCCL_SYM(CommInitRank, "ncclCommInitRank")
    GPT_RCCL_SYM(CommDestroy, "ncclCommDestroy")
    GPT_RCCL_SYM(Broadcast, "ncclBroadcast")
    GPT_RCCL_SYM(AllGather, "ncclAllGather")
    GPT_RCCL_SYM(Send, "ncclSend")
    GPT_RCCL_SYM(Recv, "ncclRecv")
    GPT_RCCL_SYM(GroupStart, "ncclGroupStart")
    GPT_RCCL_SYM(GroupEnd, "ncclGroupEnd")
    GPT_RCCL_SYM(GetErrorString, "ncclGetErrorString")
#undef GPT_RCCL_SYM
    api.handle = h;
    return &api;
}

struct PlanChannel {
    hipStream_t stream = nullptr;
    gpt_nccl_comm comm = nullptr;
    int nranks = 1, rank = 0;
};

struct gpt_plan {
    std::vector<gpt_ctx *> ctxs;            // queue q < ctxs.size() runs on ctxs[q]->stream through ctxs[q]
    std::vector<int64_t> ops;
    int64_t nops = 0;
    std::vector<hipEvent_t> events;
    PlanChannel ch[GPT_PLAN_CHANNELS];      // queue 3 + c
    int device = 0;
    const double *dX = nullptr;
    const int32_t *dn = nullptr;
    const double *d_err = nullptr;
    int D = 0;
    double last_enqueue_ms = 0.0;
};

#define GPT_NCCL_CHECK(api, expr)                                                                   \
    do {                                                                                            \
        int rc_ = (expr);                                                                           \
        if (rc_ != 0) {                                                                             \
            gpt_set_error("RCCL: %s (%s)", (api)->GetErrorString ? (api)->GetErrorString(rc_) : "?", #expr); \
            return GPT_E_HIP;                                                                       \
        }                                                                                           \
    } while (0)

extern "C" int gpt_plan_unique_id(void *out128)
{
    if (!out128) return GPT_E_ARG;
    RcclApi *api = rccl_api();
    if (!api) return GPT_E_STATE;
    gpt_nccl_id id;
    GPT_NCCL_CHECK(api, api->GetUniqueId(&id));
    memcpy(out128, &id, sizeof(id));
    return GPT_OK;
}

extern "C" int gpt_plan_create(int nctx, gpt_ctx **ctxs, const int64_t *ops, int64_t nops, int nevents, const void *dX, const void *dn,
                               int D, const void *d_err, gpt_plan **out)
{
    if (nctx < 1 || nctx > 3 || !ctxs || !ops || nops < 0 || nevents < 0 || !out) return GPT_E_ARG;
    for (int i = 0; i < nctx; i++) {
        if (!ctxs[i]) return GPT_E_ARG;
        GPT_TRY(refuse_warp(ctxs[i], "gpt_plan_create"));      // (a plan builds from its own points: it would ignore the layers)
    }
    for (int64_t i = 0; i < nops; i++) {
        const int64_t *o = ops + i * GPT_PLAN_W;
        const bool coll = o[0] == GPT_OP_BCAST || o[0] == GPT_OP_SCATTER || o[0] == GPT_OP_ALLGATHER;
        const bool evt = o[0] == GPT_OP_RECORD || o[0] == GPT_OP_WAIT;
        // (collectives run on a channel's stream, kernels on a context's; events on either)
        if (o[0] < 0 || o[0] >= GPT_OP_COUNT || o[1] < 0 || o[1] >= 3 + GPT_PLAN_CHANNELS || (o[1] < 3 && o[1] >= nctx) ||
            (coll && o[1] < 3) || (!coll && !evt && o[1] >= 3) || (evt && (o[2] < 0 || o[2] >= nevents))) {
            gpt_set_error("gpt_plan_create: malformed op %lld (opcode %lld, queue %lld)", (long long)i, (long long)o[0], (long long)o[1]);
            return GPT_E_ARG;
        }
    }
    gpt_plan *p = new (std::nothrow) gpt_plan;
    if (!p) return GPT_E_NOMEM;
    p->ctxs.assign(ctxs, ctxs + nctx);
    p->ops.assign(ops, ops + nops * GPT_PLAN_W);
    p->nops = nops;
    p->device = ctxs[0]->device;
    p->dX = (const double *)dX;
    p->dn = (const int32_t *)dn;
    p->d_err = (const double *)d_err;
    p->D = D;
    if (hipSetDevice(p->device) != hipSuccess) { delete p; return GPT_E_HIP; }
    for (int i = 0; i < nevents; i++) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            for (hipEvent_t q : p->events) hipEventDestroy(q);
            delete p;
            gpt_set_error("gpt_plan_create: hipEventCreate failed");
            return GPT_E_HIP;
        }
        p->events.push_back(e);
    }
    *out = p;
    return GPT_OK;
}

// One communication channel of the plan: ncclCommInitRank (collective over the nranks processes of THAT channel; id from
// gpt_plan_unique_id of the channel's rank 0) and its stream.  Every rank sets its channels in the same order.
extern "C" int gpt_plan_set_channel(gpt_plan *p, int channel, int nranks, int rank, const void *unique_id128)
{
    if (!p || channel < 0 || channel >= GPT_PLAN_CHANNELS || nranks < 1 || rank < 0 || rank >= nranks || !unique_id128) return GPT_E_ARG;
    PlanChannel &c = p->ch[channel];
    if (c.comm) {
        gpt_set_error("gpt_plan_set_channel: channel %d already has a communicator", channel);
        return GPT_E_STATE;
    }
    RcclApi *api = rccl_api();
    if (!api) return GPT_E_STATE;
    GPT_HIP_CHECK(hipSetDevice(p->device));
    if (!c.stream) {
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        GPT_HIP_CHECK(hipStreamCreateWithPriority(&c.stream, hipStreamNonBlocking, hi));
    }
    gpt_nccl_id id;
    memcpy(&id, unique_id128, sizeof(id));
    GPT_NCCL_CHECK(api, api->CommInitRank(&c.comm, nranks, id, rank));
    c.nranks = nranks;
    c.rank = rank;
    return GPT_OK;
}

// (the 1-D engine's one channel)
extern "C" int gpt_plan_set_comm(gpt_plan *p, int nranks, int rank, const void *unique_id128)
{
    return gpt_plan_set_channel(p, 0, nranks, rank, unique_id128);
}

static inline double plan_f64(int64_t bits)
{
    double v;
    memcpy(&v, &bits, sizeof(v));
    return v;
}

extern "C" int gpt_plan_run(gpt_plan *p, int kernel_id, const double *params, int nparams, double noise_var, double diag_add)
{
    if (!p || !params) return GPT_E_ARG;
    for (const gpt_ctx *pc : p->ctxs) GPT_TRY(refuse_warp(pc, "gpt_plan_run"));
    GPT_HIP_CHECK(hipSetDevice(p->device));
    const auto t0 = std::chrono::steady_clock::now();
    RcclApi *api = nullptr;
    for (const PlanChannel &c : p->ch)
        if (c.comm) api = rccl_api();
    auto stream_of = [&](int64_t q) -> hipStream_t { return q >= 3 ? p->ch[q - 3].stream : p->ctxs[(size_t)q]->stream; };
    // GPT_PLAN_PROFILE=1: host time per opcode of this call on stderr (where an evaluation's enqueue time goes)
    static const bool prof = getenv("GPT_PLAN_PROFILE") != nullptr;
    double prof_ms[GPT_OP_COUNT] = {0};
    int64_t prof_n[GPT_OP_COUNT] = {0};
    auto tp = t0;
    for (int64_t i = 0; i < p->nops; i++) {
        const int64_t *o = p->ops.data() + i * GPT_PLAN_W;
        const int64_t q = o[1], *a = o + 2;
        if (prof && i > 0) {
            const auto tn = std::chrono::steady_clock::now();
            const int64_t prev = o[-GPT_PLAN_W];
            prof_ms[prev] += std::chrono::duration<double, std::milli>(tn - tp).count();
            prof_n[prev]++;
            tp = tn;
        }
        gpt_ctx *c = q < 3 ? p->ctxs[(size_t)q] : nullptr;
        const PlanChannel *ch = q >= 3 ? &p->ch[q - 3] : nullptr;
        int rc = GPT_OK;
        switch ((int)o[0]) {
        case GPT_OP_RECORD:
            if (ch && !ch->stream) break;
            GPT_HIP_CHECK(hipEventRecord(p->events[(size_t)a[0]], stream_of(q)));
            break;
        case GPT_OP_WAIT:
            if (ch && !ch->stream) break;
            GPT_HIP_CHECK(hipStreamWaitEvent(stream_of(q), p->events[(size_t)a[0]], 0));
            break;
        case GPT_OP_KBUILD:          // a: r0, r1, c0, c1, out, ld
            rc = gpt_dev_kbuild(c, kernel_id, params, nparams, p->dX + a[0] * p->D, p->dn + a[0] * p->D, a[1] - a[0],
                                p->dX + a[2] * p->D, p->dn + a[2] * p->D, a[3] - a[2], p->D, -1, 1, nullptr, 1, a[0], a[2], p->d_err,
                                noise_var, diag_add, (double *)a[4], a[5]);
            break;
        case GPT_OP_PAD:             // a: ptr, lda, c0, nb, N, NP, y, big
            rc = gpt_dev_pad_block(c, (double *)a[0], a[1], a[2], a[3], a[4], a[5], (const double *)a[6], plan_f64(a[7]));
            break;
        case GPT_OP_COPY2D:          // a: rows, cols, src, lds, dst, ldd
            rc = gpt_dev_copy2d(c, a[0], a[1], (const double *)a[2], a[3], (double *)a[4], a[5]);
            break;
        case GPT_OP_POTRF_PANEL:     // a: m, nb, A, lda, invd, info, info_base
            rc = gpt_dev_potrf_panel(c, a[0], a[1], (double *)a[2], a[3], (double *)a[4], (int32_t *)a[5], a[6]);
            break;
        case GPT_OP_TRINV:           // a: nb, L, ldl, invd, W, ldw
            rc = gpt_dev_trinv(c, a[0], (const double *)a[1], a[2], (const double *)a[3], (double *)a[4], a[5]);
            break;
        case GPT_OP_GEMM:            // a: m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, tri
            rc = gpt_dev_gemm_nt(c, a[0], a[1], a[2], plan_f64(a[3]), (const double *)a[4], a[5], (const double *)a[6], a[7], plan_f64(a[8]),
                                 (double *)a[9], a[10], (int)a[11]);
            break;
        case GPT_OP_STAIR:           // a: m, nseg, seg_cols, k, alpha, A, lda, B, ldb, b_stride, row_step, beta, C, ldc
            rc = gpt_dev_gemm_nt_stair(c, a[0], a[1], a[2], a[3], plan_f64(a[4]), (const double *)a[5], a[6], (const double *)a[7], a[8],
                                       a[9], a[10], plan_f64(a[11]), (double *)a[12], a[13]);
            break;
        case GPT_OP_SCALARS:         // a: buf, ld, w, zrow, red
            rc = gpt_dev_panel_scalars(c, (const double *)a[0], a[1], a[2], a[3], (double *)a[4]);
            break;
        case GPT_OP_KRECT:           // a: Xi, ni, r0, r1, c0, c1, out, ld: a plain rectangle, rows from the rank's own gathered rows
            rc = gpt_dev_kbuild(c, kernel_id, params, nparams, (const double *)a[0] + a[2] * p->D, (const int32_t *)a[1] + a[2] * p->D,
                                a[3] - a[2], p->dX + a[4] * p->D, p->dn + a[4] * p->D, a[5] - a[4], p->D, -1, 1, nullptr, 0, 0, 0, nullptr,
                                0.0, 0.0, (double *)a[6], a[7]);
            break;
        case GPT_OP_ROWSUMSQ:        // a: row, count, out
            rc = gpt_dev_row_sumsq(c, (const double *)a[0], a[1], (double *)a[2]);
            break;
        case GPT_OP_GRIDSTAIR:       // a: m, nseg, seg_cols, k, alpha, A, lda, B, ldb, off, num, den, base, beta, C, ldc
            rc = gpt_dev_gemm_nt_gridstair(c, a[0], a[1], a[2], a[3], plan_f64(a[4]), (const double *)a[5], a[6], (const double *)a[7], a[8],
                                           a[9], a[10], a[11], a[12], plan_f64(a[13]), (double *)a[14], a[15]);
            break;
        case GPT_OP_BCAST:           // a: buf, count, root (rank inside the channel's communicator)
            if (!ch->comm) break;
            GPT_NCCL_CHECK(api, api->Broadcast((const void *)a[0], (void *)a[0], (size_t)a[1], GPT_NCCL_DOUBLE, (int)a[2], ch->comm,
                                               ch->stream));
            break;
        case GPT_OP_SCATTER: {       // a: buf, count per rank, root: piece r of buf goes to rank r (in place on the root)
            if (!ch->comm) break;
            double *buf = (double *)a[0];
            const size_t cnt = (size_t)a[1];
            const int root = (int)a[2];
            GPT_NCCL_CHECK(api, api->GroupStart());
            if (ch->rank == root)
                for (int r = 0; r < ch->nranks; r++)
                    if (r != root) GPT_NCCL_CHECK(api, api->Send(buf + (size_t)r * cnt, cnt, GPT_NCCL_DOUBLE, r, ch->comm, ch->stream));
            if (ch->rank != root)
                GPT_NCCL_CHECK(api, api->Recv(buf + (size_t)ch->rank * cnt, cnt, GPT_NCCL_DOUBLE, root, ch->comm, ch->stream));
            GPT_NCCL_CHECK(api, api->GroupEnd());
            break;
        }
        case GPT_OP_ALLGATHER:       // a: buf, count per rank: in place, rank r's piece at buf + r * count
            if (!ch->comm) break;
            GPT_NCCL_CHECK(api, api->AllGather((const void *)((double *)a[0] + (size_t)ch->rank * (size_t)a[1]), (void *)a[0], (size_t)a[1],
                                               GPT_NCCL_DOUBLE, ch->comm, ch->stream));
            break;
        default:
            gpt_set_error("gpt_plan_run: unknown opcode %lld", (long long)o[0]);
            return GPT_E_ARG;
        }
        if (rc != GPT_OK) return rc;
    }
    p->last_enqueue_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (prof) {
        fprintf(stderr, "gpt_plan_run: %.3f ms;", p->last_enqueue_ms);
        for (int k = 0; k < GPT_OP_COUNT; k++)
            if (prof_n[k]) fprintf(stderr, " op%d x%lld %.3f ms (%.2f us)", k, (long long)prof_n[k], prof_ms[k], 1e3 * prof_ms[k] / (double)prof_n[k]);
        fprintf(stderr, "\n");
    }
    return GPT_OK;
}

extern "C" double gpt_plan_last_enqueue_ms(gpt_plan *p) { return p ? p->last_enqueue_ms : -1.0; }

extern "C" int gpt_plan_destroy(gpt_plan *p)
{
    if (!p) return GPT_OK;
    (void)hipSetDevice(p->device);
    // (the contexts may already be gone -- interpreter teardown destroys objects in no particular order -- so their streams are
    // not touched here: the caller synchronises them while it still holds them; only what the plan owns is released)
    for (PlanChannel &c : p->ch)
        if (c.stream) (void)hipStreamSynchronize(c.stream);
    for (PlanChannel &c : p->ch)
        if (c.comm) {
            RcclApi *api = rccl_api();
            if (api) (void)api->CommDestroy(c.comm);
        }
    for (hipEvent_t e : p->events) hipEventDestroy(e);
    for (PlanChannel &c : p->ch)
        if (c.stream) hipStreamDestroy(c.stream);
    delete p;
    return GPT_OK;
}
