// api_context.inc -- part of api.hip (ONE translation unit: included from there, in this order; the parts share struct gpt_ctx and
// static helpers).  Gpt_ctx_create / destroy / set_option / synchronize, workspace slots.
// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
extern "C" int gpt_ctx_create(int device_id, void *stream, gpt_ctx **out)
{
    if (!out) return GPT_E_ARG;
    int ndev = 0;
    GPT_HIP_CHECK(hipGetDeviceCount(&ndev));
    if (ndev <= 0 || device_id < 0 || device_id >= ndev) {
        gpt_set_error("no such HIP device %d (count %d)", device_id, ndev);
        return GPT_E_HIP;
    }
    GPT_HIP_CHECK(hipSetDevice(device_id));
    gpt_ctx *c = new (std::nothrow) gpt_ctx();
    if (!c) return GPT_E_NOMEM;
    c->device = device_id;
    int lo = 0, hi = 0;
    GPT_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    if (stream) {
        c->stream = (hipStream_t)stream;
    } else {
        // The context's own main stream is created with a CU mask that leaves a few CUs to the (unmasked,
        // high-priority) panel stream: the 128x128 diagonal-block kernel needs ~133 KB of LDS and would otherwise
        // never find a CU while a trailing update occupies the chip, which defeats the look-ahead.
        int reserve = 32;
        if (const char *e = getenv("GPT_RESERVE_CUS")) reserve = atoi(e);
        hipDeviceProp_t prop;
        GPT_HIP_CHECK(hipGetDeviceProperties(&prop, device_id));
        const int ncu = prop.multiProcessorCount;
        bool masked = false;
        if (reserve > 0 && reserve < ncu) {
            std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
            for (int i = reserve; i < ncu; i++) mask[i / 32] |= (1u << (i % 32));
            masked = hipExtStreamCreateWithCUMask(&c->stream, (uint32_t)mask.size(), mask.data()) == hipSuccess;
            if (!masked) (void)hipGetLastError();
            else c->reserve_cus = reserve;
            // helper stream: the reserved CUs except the first 8 (those stay free for the diagonal-block kernel, which
            // needs a whole CU's LDS).  While the trailing updates dominate, the panel stream leaves the reserved CUs
            // idle most of the time; a slice of every update runs there (potrf_enqueue).
            // NOTE: every extra stream of a context costs: with a FIFTH stream (main, panel, helper + two more) the
            // runtime maps two of them to one hardware queue and the whole factorisation ran 2x slower (5.5 -> 10.7 ms at
            // N=8192) even with the extra streams unused: no further stream may be added to a context.
            if (masked && reserve >= 16) {
                std::vector<uint32_t> hm((ncu + 31) / 32, 0u);
                for (int i = 8; i < reserve; i++) hm[i / 32] |= (1u << (i % 32));
                if (hipExtStreamCreateWithCUMask(&c->helper_stream, (uint32_t)hm.size(), hm.data()) != hipSuccess) {
                    (void)hipGetLastError();
                    c->helper_stream = nullptr;
                }
                c->helper_cus = reserve - 8;
            }
        }
        if (!masked) GPT_HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    GPT_HIP_CHECK(hipStreamCreateWithPriority(&c->panel_stream, hipStreamNonBlocking, hi));
    for (int i = 0; i < 5; i++) GPT_HIP_CHECK(hipEventCreate(&c->tev[i]));
    GPT_HIP_CHECK(hipMalloc(&c->d_info, sizeof(int32_t)));
    GPT_HIP_CHECK(hipMalloc((void **)&c->d_flag, 256));
    GPT_HIP_CHECK(hipMalloc((void **)&c->d_edge, 256));
    // (hipMemsetAsync on the context's stream, never hipMemset: one call on the legacy null stream and from then on
    // every kernel of this process starts ~40 us late on every stream -- measured on the block-cyclic engine,
    // 31 -> 41 ms per rank at N=32768 over 8 ranks, potf2 26 -> 45..90 us in the trace)
    GPT_HIP_CHECK(hipMemsetAsync(c->d_flag, 0, 256, c->stream));
    GPT_HIP_CHECK(hipMemsetAsync(c->d_edge, 0, 256, c->stream));
    GPT_HIP_CHECK(hipMalloc(&c->d_scal, 80 * sizeof(double)));     // logdet_dot's partial sums (64) + its counter
    GPT_HIP_CHECK(hipMemsetAsync(c->d_scal, 0, 80 * sizeof(double), c->stream));
    GPT_HIP_CHECK(hipHostMalloc((void **)&c->h_scal, 4 * sizeof(double), hipHostMallocDefault));
    GPT_HIP_CHECK(hipHostMalloc((void **)&c->h_info, sizeof(int32_t), hipHostMallocDefault));
    *out = c;
    return GPT_OK;
}

static void free_factor(gpt_ctx *c)
{
    if (c->gexec) { hipGraphExecDestroy(c->gexec); c->gexec = nullptr; }
    if (c->dA) hipFree(c->dA);
    if (c->d_invd) hipFree(c->d_invd);
    if (c->d_y) hipFree(c->d_y);
    if (c->h_yerr) hipHostFree(c->h_yerr);
    c->h_yerr = nullptr;
    if (c->h_alpha) hipHostFree(c->h_alpha);
    c->h_alpha = nullptr;
    c->h_alpha_valid = false;
    if (c->d_alpha) hipFree(c->d_alpha);
    c->dA = c->d_invd = c->d_y = c->d_erry = c->d_alpha = nullptr;
    c->NP = 0;
    invalidate_factor(c);
}

extern "C" int gpt_ctx_destroy(gpt_ctx *c)
{
    if (!c) return GPT_OK;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    hipStreamSynchronize(c->panel_stream);
    free_factor(c);
    if (c->dX) hipFree(c->dX);
    if (c->dn) hipFree(c->dn);
    if (c->dXw) hipFree(c->dXw);
    if (c->dS) hipFree(c->dS);
    if (c->dT) hipFree(c->dT);
    for (auto &b : c->slots)
        if (b.p) hipFree(b.p);
    for (auto e : c->events) hipEventDestroy(e);
    for (auto e : c->sp_events) hipEventDestroy(e);
    for (auto &g : c->gprof) { hipEventDestroy(g.e0); hipEventDestroy(g.e1); }
    for (int i = 0; i < 5; i++)
        if (c->tev[i]) hipEventDestroy(c->tev[i]);
    if (c->d_info) hipFree(c->d_info);
    if (c->d_flag) hipFree(c->d_flag);
    if (c->d_edge) hipFree(c->d_edge);
    if (c->d_scal) hipFree(c->d_scal);
    if (c->h_scal) hipHostFree(c->h_scal);
    if (c->h_stage) hipHostFree(c->h_stage);
    if (c->h_batch) hipHostFree(c->h_batch);
    if (c->copy_stream) hipStreamDestroy(c->copy_stream);
    for (auto &e : c->cev)
        if (e) hipEventDestroy(e);
    if (c->h_info) hipHostFree(c->h_info);
    hipStreamDestroy(c->panel_stream);
    if (c->e_binv_early) hipEventDestroy(c->e_binv_early);
    if (c->helper_stream) hipStreamDestroy(c->helper_stream);
    if (c->own_stream) hipStreamDestroy(c->stream);
    delete c;
    return GPT_OK;
}

extern "C" int gpt_ctx_set_option(gpt_ctx *c, const char *key, int64_t value)
{
    if (!c || !key) return GPT_E_ARG;
    if (!strcmp(key, "nb_outer")) {
        if (value < 0 || value % 128) {
            gpt_set_error("nb_outer must be 0 (chosen by size) or a positive multiple of 128");
            return GPT_E_ARG;
        }
        c->nb_outer = value;
    } else if (!strcmp(key, "lookahead")) c->lookahead = value ? 1 : 0;
    else if (!strcmp(key, "graph")) c->use_graph = value ? 1 : 0;
    else if (!strcmp(key, "timing")) c->timing = value ? 1 : 0;
    else if (!strcmp(key, "profile_gemm")) c->prof_gemm = value ? 1 : 0;
    else if (!strcmp(key, "gemm_pad")) c->gemm_pad = (int)value;
    else if (!strcmp(key, "dev_gemm_pad")) c->dev_gemm_pad = value;
    else if (!strcmp(key, "ramp")) c->ramp = value ? 1 : 0;
    else if (!strcmp(key, "defer_rows")) c->defer_rows = value;
    else if (!strcmp(key, "purg_rows")) c->purg_rows = value;
    else if (!strcmp(key, "edge_flags")) c->edge_flags = value;
    else if (!strcmp(key, "merge_urgent")) c->merge_urgent = value;
    else if (!strcmp(key, "tail_wait")) c->tail_wait = value;
    else if (!strcmp(key, "skip_pad_rows")) c->skip_pad_rows = value ? 1 : 0;
    else if (!strcmp(key, "gemm_prio")) c->gemm_prio = value;
    else if (!strcmp(key, "nb_early")) c->nb_early = value;
    else if (!strcmp(key, "nb_switch_rows")) c->nb_switch_rows = value;
    else if (!strcmp(key, "inner")) c->inner = (int)value;
    else if (!strcmp(key, "helper_tf")) c->helper_tf = (int)value;
    else if (!strcmp(key, "helper_min_n")) c->helper_min_n = value;
    else if (!strcmp(key, "fuse_trsm")) c->fuse_trsm = value;
    else if (!strcmp(key, "fuse_rows64")) c->fuse_rows64 = value;
    else if (!strcmp(key, "fuse_rows32")) c->fuse_rows32 = value;
    else if (!strcmp(key, "fuse_rows16")) c->fuse_rows16 = value;
    else if (!strcmp(key, "splitk")) c->splitk = value;
    else if (!strcmp(key, "eager_alpha")) c->eager_alpha = value;
    else if (!strcmp(key, "defer_pad")) c->defer_pad = value;
    else if (!strcmp(key, "binv_launches")) { c->binv_launches = value; c->binv_valid = c->binv2_valid = c->binv3_valid = false; c->h_alpha_valid = c->alpha_valid = false; }
    else if (!strcmp(key, "debug_poison")) c->debug_poison = value;
    else if (!strcmp(key, "alpha_invalidate")) c->h_alpha_valid = c->alpha_valid = false;          // (measurement aid: the next gpt_get_alpha recomputes)
    else if (!strcmp(key, "edge_test_stall")) c->edge_test_stall = value;
    else if (!strcmp(key, "tile")) {
        if (value != 0 && value != 32 && value != 64) {
            gpt_set_error("tile must be 0 (by launch size), 32 or 64");
            return GPT_E_ARG;
        }
        c->tile = (int)value;
    } else {
        gpt_set_error("unknown option '%s'", key);
        return GPT_E_ARG;
    }
    return GPT_OK;
}

extern "C" int gpt_ctx_synchronize(gpt_ctx *c)
{
    if (!c) return GPT_E_ARG;
    GPT_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GPT_OK;
}

extern "C" void *gpt_ctx_stream(gpt_ctx *c) { return c ? (void *)c->stream : nullptr; }
extern "C" int64_t gpt_ctx_edge_count(gpt_ctx *c) { return c ? (int64_t)c->edge_seq : -1; }

#define CTX_ENTER(c)                          \
    do {                                      \
        if (!(c)) {                           \
            gpt_set_error("null context");    \
            return GPT_E_ARG;                 \
        }                                     \
        GPT_HIP_CHECK(hipSetDevice((c)->device)); \
    } while (0)
