// dh_api.h -- the C-ABI entry points of the pricing and loss requests (include/dhcos.h): context
// and surface objects, dh_surface_price* / _loss*, dh_price_pairs, the CF / truncation range /
// coefficient probes, the one-shot batch calls and the host driver's function + gradient requests
// (dh_surface_fg*).  Host code only.  Included by dh_kernels.hip after dh_launch.h; it needs
// launch_price, loss_stage and the uncontracted device code at the end of dh_kernels.hip.
#pragma once

extern "C" {

int dh_version(void) { return 1; }

const char* dh_last_error(void) { return g_err.c_str(); }

int dh_device_count(int* count) {
    if (!count) return fail(DH_E_ARG, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(DH_E_NODEV, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = n;
    return DH_OK;
}

int dh_ctx_create(int device, dh_ctx** out) {
    if (!out) return fail(DH_E_ARG, "out is null");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(DH_E_NODEV, std::string("no HIP device: ") + hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(DH_E_ARG, "device index out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(DH_E_NODEV, std::string("libdhcos is built for gfx950, device is ") +
                                    prop.gcnArchName);
    dh_ctx* c = new (std::nothrow) dh_ctx();
    if (!c) return fail(DH_E_ALLOC, "ctx alloc");
    c->device = device;
    DeviceScope dev_scope(device);
    if (dev_scope.rc) {
        delete c;
        return dev_scope.rc;
    }
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(DH_E_HIP, std::string("stream create: ") + hipGetErrorString(e));
    }
    *out = c;
    return DH_OK;
}

int dh_ctx_destroy(dh_ctx* ctx) {
    if (!ctx) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (hipEvent_t e : ctx->lb_ev)
        if (e) (void)hipEventDestroy(e);
    gen_bufs_release(ctx);
    if (ctx->vr_surf) (void)dh_surface_destroy(ctx->vr_surf);
    for (auto& F : ctx->fg)
        if (F.done) (void)hipEventDestroy(F.done);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;             // with the device current: every DevBuf / HostBuf member frees itself
    return DH_OK;
}

int dh_ctx_synchronize(dh_ctx* ctx) {
    if (!ctx) return fail(DH_E_ARG, "ctx is null");
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DH_OK;
}

void* dh_ctx_stream(dh_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int dh_ctx_debug_stamps(dh_ctx* ctx, int on) {
    if (!ctx) return fail(DH_E_ARG, "ctx is null");
#ifdef DH_STAMPS
    ctx->stamps_on = on ? 1 : 0;
    return DH_OK;
#else
    (void)on;
    return fail(DH_E_ARG, "library built without DH_STAMPS (use `make stamps`)");
#endif
}

int dh_ctx_read_stamps(dh_ctx* ctx, unsigned long long* out, int64_t cap, int64_t* n) {
    if (!ctx || !n) return fail(DH_E_ARG, "null argument");
    *n = ctx->stamps_n;
    if (!out || ctx->stamps_n == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, ctx->stamps.ptr, (size_t)std::min<int64_t>(cap, ctx->stamps_n) * 8,
                      hipMemcpyDeviceToHost));
    return DH_OK;
}

int dh_ctx_set_path(dh_ctx* ctx, int path) {
    if (!ctx) return fail(DH_E_ARG, "ctx is null");
    if (path != DH_PATH_AUTO && path != DH_PATH_SPLIT && path != DH_PATH_FUSED)
        return fail(DH_E_ARG, "bad path");
    ctx->path = path;
    return DH_OK;
}

int dh_ctx_last_path(dh_ctx* ctx) { return ctx ? ctx->last_path : DH_E_ARG; }

int dh_ctx_set_exact(dh_ctx* ctx, int on) {
    if (!ctx) return fail(DH_E_ARG, "ctx is null");
    ctx->exact = on ? 1 : 0;
    return DH_OK;
}

int dh_ctx_set_tail_cut(dh_ctx* ctx, int on) {
    if (!ctx) return fail(DH_E_ARG, "ctx is null");
    ctx->tail_cut = on ? 1 : 0;
    return DH_OK;
}

int dh_surface_create(dh_ctx* ctx, const double* K, const double* T, const int8_t* is_call,
                      const double* mkt, int M, int strike_mode, dh_surface** out) {
    if (!ctx || !out) return fail(DH_E_ARG, "ctx/out is null");
    *out = nullptr;
    if (M < 0) return fail(DH_E_ARG, "M < 0");
    if (M > 0 && (!K || !T || !is_call)) return fail(DH_E_ARG, "K/T/is_call is null");
    if (strike_mode != DH_STRIKE_ABSOLUTE && strike_mode != DH_STRIKE_PCT_SPOT)
        return fail(DH_E_ARG, "bad strike_mode");
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    // group by exact maturity (stable), cut groups into tiles of <= kTileMax options
    std::vector<int> perm(M);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int i, int j) { return T[i] < T[j]; });
    std::vector<double> sK(M), sT(M), sm(M, 0.0);
    std::vector<int8_t> sc(M);
    for (int i = 0; i < M; ++i) {
        sK[i] = K[perm[i]];
        sT[i] = T[perm[i]];
        sc[i] = is_call[perm[i]] ? 1 : 0;
        if (mkt) sm[i] = mkt[perm[i]];
    }
    std::vector<int2> tiles;
    std::vector<int> tile_group;
    std::vector<double> group_T;
    std::vector<int2> groups;
    int max_nopt = 0, max_group = 0;
    for (int i = 0; i < M;) {
        int j = i;
        while (j < M && sT[j] == sT[i]) ++j;
        groups.push_back(make_int2(i, j - i));
        max_group = std::max(max_group, j - i);
        for (int s = i; s < j; s += kTileMax) {
            tiles.push_back(make_int2(s, std::min(kTileMax, j - s)));
            tile_group.push_back((int)group_T.size());
            max_nopt = std::max(max_nopt, std::min(kTileMax, j - s));
        }
        group_T.push_back(sT[i]);
        i = j;
    }
    dh_surface* s = new (std::nothrow) dh_surface();
    if (!s) return fail(DH_E_ALLOC, "surface alloc");
    s->ctx = ctx;
    s->M = M;
    s->n_tiles = (int)tiles.size();
    s->n_groups = (int)group_T.size();
    s->max_nopt = max_nopt;
    s->max_group = max_group;
    s->strike_mode = strike_mode;
    s->has_mkt = mkt != nullptr;
    s->h_group_T = group_T;
    s->h_groups = groups;
    // every array in one device allocation, staged on the host and uploaded by one copy (one
    // hipMalloc and one synchronous copy instead of nine of each: ~0.5 ms of a C3 calibration)
    struct Part {
        void** dst;
        const void* src;
        size_t bytes;
    };
    const size_t m = (size_t)M;
    const Part parts[] = {{(void**)&s->K, sK.data(), m * 8},
                          {(void**)&s->T, sT.data(), m * 8},
                          {(void**)&s->mkt, sm.data(), m * 8},
                          {(void**)&s->call, sc.data(), m},
                          {(void**)&s->perm, perm.data(), m * 4},
                          {(void**)&s->tiles, tiles.data(), tiles.size() * sizeof(int2)},
                          {(void**)&s->tile_group, tile_group.data(), tile_group.size() * sizeof(int)},
                          {(void**)&s->group_T, group_T.data(), group_T.size() * sizeof(double)},
                          {(void**)&s->groups, groups.data(), groups.size() * sizeof(int2)}};
    size_t off[9], total = 0;
    for (int i = 0; i < 9; ++i) {          // 256-byte aligned, >= 16 bytes each (empty surfaces)
        off[i] = total;
        total += (std::max<size_t>(parts[i].bytes, 16) + 255) & ~(size_t)255;
    }
    hipError_t e = hipMalloc(&s->block, total);
    if (e == hipSuccess) {
        for (int i = 0; i < 9; ++i) *parts[i].dst = (char*)s->block + off[i];
        if (M > 0) {
            std::vector<char> stage(total, 0);
            for (int i = 0; i < 9; ++i)
                if (parts[i].bytes) std::memcpy(stage.data() + off[i], parts[i].src, parts[i].bytes);
            e = hipMemcpy(s->block, stage.data(), total, hipMemcpyHostToDevice);
        }
    }
    if (e != hipSuccess) {
        dh_surface_destroy(s);
        return fail(DH_E_HIP, std::string("surface upload: ") + hipGetErrorString(e));
    }
    *out = s;
    return DH_OK;
}

int dh_surface_destroy(dh_surface* s) {
    if (!s) return DH_OK;
    DeviceScope dev_scope(s->ctx ? s->ctx->device : 0);
    if (s->block) (void)hipFree(s->block);
    if (s->iv_block) (void)hipFree(s->iv_block);
    if (s->spot_block) (void)hipFree(s->spot_block);
    delete s;
    return DH_OK;
}

int dh_surface_stage_spot(dh_surface* s, double S0) {
    if (!s || !s->ctx) return fail(DH_E_ARG, "surface is null");
    if (!(S0 > 0.0) || std::isinf(S0)) return fail(DH_E_ARG, "S0 must be finite and > 0");
    if (s->M == 0) return DH_OK;
    dh_ctx* ctx = s->ctx;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t m = (size_t)s->M;
    if (!s->spot_block) {
        HIP_TRY(hipMalloc(&s->spot_block, 3 * m * sizeof(double)));
    }
    double* base = (double*)s->spot_block;
    // off while the arrays are rewritten, and for good should the launch fail
    s->spot_staged = kSpotNone;
    s->xk_s = s->exk_s = s->k_s = nullptr;
    PriceArgs A{};
    A.K = s->K;
    A.strike_mode = s->strike_mode;
    A.M = s->M;
    hipLaunchKernelGGL(stage_spot_kernel, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock),
                       0, ctx->stream, A, S0, base + 2 * m, base, base + m);
    HIP_TRY(hipGetLastError());
    // once per surface: requests on any stream (the SciPy loop's slots) then need no ordering
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    s->xk_s = base;
    s->exk_s = base + m;
    s->k_s = base + 2 * m;
    std::memcpy(&s->spot_staged, &S0, sizeof(S0));
    return DH_OK;
}

int dh_surface_size(const dh_surface* s, int* M, int* n_tiles) {
    if (!s) return fail(DH_E_ARG, "surface is null");
    if (M) *M = s->M;
    if (n_tiles) *n_tiles = s->n_tiles;
    return DH_OK;
}

static PriceArgs surface_args(const dh_ctx* ctx, const dh_surface* s, const double* d_params,
                              int64_t P, int N, double L) {
    PriceArgs A{};
    A.exact = per_term(ctx, N);
    A.prm = d_params;
    A.P = P;
    A.K = s->K;
    A.T = s->T;
    A.call = s->call;
    A.mkt = s->mkt;
    A.perm = s->perm;
    A.tiles = s->tiles;
    A.tile_group = s->tile_group;
    A.group_T = s->group_T;
    A.groups = s->groups;
    A.max_group = s->max_group;
    A.n_tiles = s->n_tiles;
    A.n_groups = s->n_groups;
    A.opt_cap = ((s->max_nopt + 1) / 2) * 2;
    A.M = s->M;
    A.paired = 0;
    A.strike_mode = s->strike_mode;
    A.N = N;
    A.L = L;
    A.out_stride = s->M;
    A.xk_s = s->xk_s;                      // null until dh_surface_stage_spot
    A.exk_s = s->exk_s;
    A.k_s = s->k_s;
    A.spot_staged = s->spot_staged;
    return A;
}

int dh_surface_price_dev(dh_ctx* ctx, const dh_surface* s, const double* d_params, int64_t P,
                         int N, double L, double* d_out, void* stream) {
    if (!ctx || !s || (P > 0 && (!d_params || !d_out))) return fail(DH_E_ARG, "null argument");
    int rc = check_N(N);
    if (rc) return rc;
    if (P < 0) return fail(DH_E_ARG, "P < 0");
    if (P == 0 || s->M == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    PriceArgs A = surface_args(ctx, s, d_params, P, N, L);
    A.out = d_out;
    return launch_price(ctx, A, stream ? (hipStream_t)stream : ctx->stream);
}

}  // extern "C"

// dh_surface_price_dev for the batch driver's requests (dh_calibrate_lbfgs_batch): a no-op once
// *live_count is 0, and the kernel choice does not follow the request's size -- under
// DH_PATH_AUTO the fused kernels wherever they apply, so a start's prices have the same bits
// whatever shares its launch (the generator kernel of large calls rounds differently, 3.3)
static int surface_price_launch_lb(dh_ctx* ctx, const dh_surface* s, const double* d_params,
                                   int64_t P, int N, double L, double* d_out, hipStream_t st,
                                   const int* live_count) {
    if (P == 0 || s->M == 0) return DH_OK;
    PriceArgs A = surface_args(ctx, s, d_params, P, N, L);
    A.out = d_out;
    A.live_count = live_count;
    const int path = ctx->path;
    if (path == DH_PATH_AUTO) ctx->path = DH_PATH_FUSED;
    const int rc = launch_price(ctx, A, st);
    ctx->path = path;
    return rc;
}

static int surface_loss_launch(dh_ctx* ctx, const dh_surface* s, const double* d_params, int S,
                               int N, double L, double* d_sse, int32_t* d_n_bad,
                               double* d_prices, void* stream, const int* live_count,
                               bool partials_only = false) {
    if (!ctx || !s || (S > 0 && (!d_params || !d_sse || !d_n_bad)))
        return fail(DH_E_ARG, "null argument");
    if (!s->has_mkt) return fail(DH_E_ARG, "surface has no market prices");
    int rc = check_N(N);
    if (rc) return rc;
    return loss_stage(ctx, s, S, d_sse, d_n_bad, stream, [&](hipStream_t st) -> int {
        const size_t nparts = (size_t)S * s->n_tiles;
        HIP_TRY(ctx->part_sse.reserve(nparts * 8));
        HIP_TRY(ctx->part_bad.reserve(nparts * 4));
        const size_t cap0 = ctx->counter.cap;
        HIP_TRY(ctx->counter.reserve((size_t)S * kCounterStride * 4));
        if (ctx->counter.cap != cap0) {       // fresh counters start at zero; kernels self-reset
            HIP_TRY(hipMemsetAsync(ctx->counter.ptr, 0, ctx->counter.cap, st));
        }
        PriceArgs A = surface_args(ctx, s, d_params, S, N, L);
        A.out = d_prices;
        A.part_sse = (double*)ctx->part_sse.ptr;
        A.part_bad = (int*)ctx->part_bad.ptr;
        A.counter = (unsigned*)ctx->counter.ptr;
        A.sse = d_sse;
        A.n_bad = (int*)d_n_bad;
        A.live_count = live_count;
        A.partials_only = partials_only && !A.exact ? 1 : 0;
        A.host_out = ctx->kp_src != nullptr;     // the host API's zero-copy requests (kp_src set)
        return launch_price(ctx, A, st);
    });
}

extern "C" {

int dh_surface_loss_dev(dh_ctx* ctx, const dh_surface* s, const double* d_params, int S, int N,
                        double L, double* d_sse, int32_t* d_n_bad, double* d_prices,
                        void* stream) {
    return surface_loss_launch(ctx, s, d_params, S, N, L, d_sse, d_n_bad, d_prices, stream,
                               nullptr);
}

int dh_surface_price(dh_ctx* ctx, const dh_surface* s, const double* params, int64_t P, int N,
                     double L, double* out) {
    if (!ctx || !s || (P > 0 && (!params || !out))) return fail(DH_E_ARG, "null argument");
    int rc = check_N(N);
    if (rc) return rc;
    if (P < 0) return fail(DH_E_ARG, "P < 0");
    if (P == 0 || s->M == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t pb = (size_t)P * DH_PARAM_STRIDE * 8, ob = (size_t)P * s->M * 8;
    HIP_TRY(ctx->params.reserve(pb));
    HIP_TRY(ctx->out.reserve(ob));
    HIP_TRY(hipMemcpyAsync(ctx->params.ptr, params, pb, hipMemcpyHostToDevice, ctx->stream));
    rc = dh_surface_price_dev(ctx, s, (const double*)ctx->params.ptr, P, N, L,
                              (double*)ctx->out.ptr, ctx->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, ctx->out.ptr, ob, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DH_OK;
}

int dh_surface_price_cols(dh_ctx* ctx, const dh_surface* s, const double* params,
                          const double* spots, double r, int64_t P, int N, double L, double* out) {
    if (!ctx || !s || (P > 0 && (!params || !spots || !out))) return fail(DH_E_ARG, "null argument");
    int rc = check_N(N);
    if (rc) return rc;
    if (P < 0) return fail(DH_E_ARG, "P < 0");
    if (P == 0 || s->M == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    hipStream_t st = ctx->stream;
    const size_t ob = (size_t)P * s->M * 8;
    HIP_TRY(ctx->params.reserve((size_t)P * DH_PARAM_STRIDE * 8));
    HIP_TRY(ctx->aux0.reserve((size_t)P * 13 * 8));
    HIP_TRY(ctx->aux1.reserve((size_t)P * 8));
    HIP_TRY(ctx->out.reserve(ob));
    HIP_TRY(hipMemcpyAsync(ctx->aux0.ptr, params, (size_t)P * 13 * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->aux1.ptr, spots, (size_t)P * 8, hipMemcpyHostToDevice, st));
    const int64_t n_el = P * DH_PARAM_STRIDE;
    const int64_t nb = (n_el + 255) / 256;
    if (nb > 0x7fffffffLL) return fail(DH_E_ARG, "launch too large");
    hipLaunchKernelGGL(gen_records_kernel, dim3((unsigned)nb), dim3(256), 0, st,
                       (const double*)ctx->aux0.ptr, (const double*)ctx->aux1.ptr, r, P,
                       (double*)ctx->params.ptr);
    HIP_TRY(hipGetLastError());
    rc = dh_surface_price_dev(ctx, s, (const double*)ctx->params.ptr, P, N, L,
                              (double*)ctx->out.ptr, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, ctx->out.ptr, ob, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}

// A failed (un)registration is reported here and nowhere else: HIP's per-thread last error is
// read back (cleared), so the next call's hipGetLastError check after a launch does not report it
// (a caller that leaves an array pageable after a failed registration, _native.pinned, goes on)
int dh_host_register(void* ptr, size_t bytes) {
    if (!ptr || !bytes) return fail(DH_E_ARG, "null or empty range");
    const hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(DH_E_HIP, std::string("hipHostRegister: ") + hipGetErrorString(e));
    }
    return DH_OK;
}

int dh_host_unregister(void* ptr) {
    if (!ptr) return fail(DH_E_ARG, "null argument");
    const hipError_t e = hipHostUnregister(ptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(DH_E_HIP, std::string("hipHostUnregister: ") + hipGetErrorString(e));
    }
    return DH_OK;
}

int dh_surface_loss(dh_ctx* ctx, const dh_surface* s, const double* params, int S, int N,
                    double L, double* sse, int32_t* n_bad, double* prices) {
    if (!ctx || !s || (S > 0 && (!params || !sse || !n_bad))) return fail(DH_E_ARG, "null argument");
    int rc = check_N(N);
    if (rc) return rc;
    if (S < 0) return fail(DH_E_ARG, "S < 0");
    if (S == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t pb = (size_t)S * DH_PARAM_STRIDE * 8;
    double* d_prices = nullptr;
    const size_t ob = (size_t)S * s->M * 8;
    if (prices) {
        HIP_TRY(ctx->out.reserve(ob));
        d_prices = (double*)ctx->out.ptr;
    }
    if (S <= kZeroCopyMaxSets) {
        // calibration-sized request: the kernels read the params and write sse / n_bad through
        // pinned, mapped host memory -- one launch and one sync, no staging copies
        HIP_TRY(ctx->h_params.reserve(pb));
        HIP_TRY(ctx->h_loss.reserve((size_t)S * 12));
        std::memcpy(ctx->h_params.ptr, params, pb);
        double* h_sse = (double*)ctx->h_loss.ptr;
        int32_t* h_bad = (int32_t*)(h_sse + S);
        ctx->kp_src = (const double*)ctx->h_params.ptr;     // <= 14 records: in the arguments
        ctx->kp_surf = s;
        ctx->kp_n = S;
        rc = dh_surface_loss_dev(ctx, s, (const double*)ctx->h_params.dptr, S, N, L,
                                 (double*)ctx->h_loss.dptr, (int32_t*)((double*)ctx->h_loss.dptr + S),
                                 d_prices, ctx->stream);
        ctx->kp_src = nullptr;
        ctx->kp_surf = nullptr;
        ctx->kp_n = 0;
        if (rc) return rc;
        if (prices && s->M > 0)
            HIP_TRY(hipMemcpyAsync(prices, d_prices, ob, hipMemcpyDeviceToHost, ctx->stream));
        rc = spin_sync(ctx->stream);
        if (rc) return rc;
        std::memcpy(sse, h_sse, (size_t)S * 8);
        std::memcpy(n_bad, h_bad, (size_t)S * 4);
        return check_loss_counts(n_bad, S);
    }
    HIP_TRY(ctx->params.reserve(pb));
    HIP_TRY(ctx->sse.reserve((size_t)S * 8));
    HIP_TRY(ctx->bad.reserve((size_t)S * 4));
    HIP_TRY(hipMemcpyAsync(ctx->params.ptr, params, pb, hipMemcpyHostToDevice, ctx->stream));
    rc = dh_surface_loss_dev(ctx, s, (const double*)ctx->params.ptr, S, N, L,
                             (double*)ctx->sse.ptr, (int32_t*)ctx->bad.ptr, d_prices, ctx->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(sse, ctx->sse.ptr, (size_t)S * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(n_bad, ctx->bad.ptr, (size_t)S * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (prices && s->M > 0)
        HIP_TRY(hipMemcpyAsync(prices, d_prices, ob, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return check_loss_counts(n_bad, S);
}

int dh_price_pairs(dh_ctx* ctx, const double* params, const double* K, const double* T,
                   const int8_t* is_call, int64_t P, int N, double L, double* out) {
    if (!ctx || (P > 0 && (!params || !K || !T || !is_call || !out)))
        return fail(DH_E_ARG, "null argument");
    int rc = check_N(N);
    if (rc) return rc;
    if (P < 0) return fail(DH_E_ARG, "P < 0");
    if (P == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t pb = (size_t)P * DH_PARAM_STRIDE * 8, vb = (size_t)P * 8;
    hipStream_t st = ctx->stream;
    PriceArgs A{};
    A.P = P;
    double* d_out = nullptr;
    const bool zc = P <= kZeroCopyMaxSets;
    if (zc) {
        // single options and small batches (DoubleHeston.pricing() calls): the kernel reads the
        // inputs and writes the prices through pinned, mapped host memory -- one launch and one
        // spin-wait instead of five staging copies, a read-back and a stream sync
        const size_t need = pb + 3 * vb + (size_t)P * 4 + (size_t)P;
        HIP_TRY(ctx->h_pairs.reserve(need));
        char* h = (char*)ctx->h_pairs.ptr;
        char* d = (char*)ctx->h_pairs.dptr;
        std::memcpy(h, params, pb);
        std::memcpy(h + pb, K, vb);
        std::memcpy(h + pb + vb, T, vb);
        int* perm = (int*)(h + pb + 3 * vb);
        for (int64_t i = 0; i < P; ++i) perm[i] = (int)i;
        std::memcpy(h + pb + 3 * vb + (size_t)P * 4, is_call, (size_t)P);
        A.prm = (const double*)d;
        A.K = (const double*)(d + pb);
        A.T = (const double*)(d + pb + vb);
        d_out = (double*)(d + pb + 2 * vb);
        A.perm = (const int*)(d + pb + 3 * vb);
        A.call = (const int8_t*)(d + pb + 3 * vb + (size_t)P * 4);
    } else {
        HIP_TRY(ctx->params.reserve(pb));
        HIP_TRY(ctx->out.reserve(vb));
        HIP_TRY(ctx->aux0.reserve(vb));
        HIP_TRY(ctx->aux1.reserve(vb));
        HIP_TRY(ctx->aux2.reserve((size_t)P));
        HIP_TRY(ctx->aux3.reserve((size_t)P * 4));
        std::vector<int> ident((size_t)P);
        std::iota(ident.begin(), ident.end(), 0);
        HIP_TRY(hipMemcpyAsync(ctx->params.ptr, params, pb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->aux0.ptr, K, vb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->aux1.ptr, T, vb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->aux2.ptr, is_call, (size_t)P, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->aux3.ptr, ident.data(), (size_t)P * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));        // `ident` is pageable and leaves scope
        A.prm = (const double*)ctx->params.ptr;
        A.K = (const double*)ctx->aux0.ptr;
        A.T = (const double*)ctx->aux1.ptr;
        A.call = (const int8_t*)ctx->aux2.ptr;
        A.perm = (const int*)ctx->aux3.ptr;
        d_out = (double*)ctx->out.ptr;
    }
    A.paired = 1;
    A.opt_cap = 2;
    A.max_group = 1;
    A.M = (int)P;
    A.exact = per_term(ctx, N);
    A.strike_mode = DH_STRIKE_ABSOLUTE;
    A.N = N;
    A.L = L;
    A.out = d_out;
    A.out_stride = 0;
    rc = launch_price(ctx, A, st);
    if (rc) return rc;
    if (zc) {
        rc = spin_sync(st);
        if (rc) return rc;
        std::memcpy(out, (char*)ctx->h_pairs.ptr + pb + 2 * vb, vb);
        return DH_OK;
    }
    HIP_TRY(hipMemcpyAsync(out, ctx->out.ptr, vb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}

int dh_cf(dh_ctx* ctx, const double* params, const double* u, int n, double tau, double* re,
          double* im) {
    if (!ctx || !params || (n > 0 && (!u || !re || !im))) return fail(DH_E_ARG, "null argument");
    if (n < 0) return fail(DH_E_ARG, "n < 0");
    if (n == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t vb = (size_t)n * 8;
    HIP_TRY(ctx->params.reserve(DH_PARAM_STRIDE * 8));
    HIP_TRY(ctx->aux0.reserve(vb));
    HIP_TRY(ctx->aux1.reserve(vb));
    HIP_TRY(ctx->aux2.reserve(vb));
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(ctx->params.ptr, params, DH_PARAM_STRIDE * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->aux0.ptr, u, vb, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(cf_kernel, dim3((n + 255) / 256), dim3(256), 0, st,
                       (const double*)ctx->params.ptr, (const double*)ctx->aux0.ptr, n, tau,
                       (double*)ctx->aux1.ptr, (double*)ctx->aux2.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(re, ctx->aux1.ptr, vb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(im, ctx->aux2.ptr, vb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}

int dh_cf_complex(dh_ctx* ctx, const double* params, const double* u_re, const double* u_im,
                  int n, double tau, double* re, double* im) {
    if (!ctx || !params || (n > 0 && (!u_re || !u_im || !re || !im)))
        return fail(DH_E_ARG, "null argument");
    if (n < 0) return fail(DH_E_ARG, "n < 0");
    if (n == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t vb = (size_t)n * 8;
    HIP_TRY(ctx->params.reserve(DH_PARAM_STRIDE * 8));
    HIP_TRY(ctx->aux0.reserve(vb));
    HIP_TRY(ctx->aux1.reserve(vb));
    HIP_TRY(ctx->aux2.reserve(vb));
    HIP_TRY(ctx->aux3.reserve(vb));
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(ctx->params.ptr, params, DH_PARAM_STRIDE * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->aux0.ptr, u_re, vb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->aux1.ptr, u_im, vb, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(cf_kernel_z, dim3((n + 255) / 256), dim3(256), 0, st,
                       (const double*)ctx->params.ptr, (const double*)ctx->aux0.ptr,
                       (const double*)ctx->aux1.ptr, n, tau, (double*)ctx->aux2.ptr,
                       (double*)ctx->aux3.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(re, ctx->aux2.ptr, vb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(im, ctx->aux3.ptr, vb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}

int dh_trunc_range(dh_ctx* ctx, const double* params, const double* K, const double* T,
                   int64_t P, double L, double* a, double* b) {
    if (!ctx || (P > 0 && (!params || !K || !T || !a || !b))) return fail(DH_E_ARG, "null argument");
    if (P < 0) return fail(DH_E_ARG, "P < 0");
    if (P == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t pb = (size_t)P * DH_PARAM_STRIDE * 8, vb = (size_t)P * 8;
    HIP_TRY(ctx->params.reserve(pb));
    HIP_TRY(ctx->aux0.reserve(vb));
    HIP_TRY(ctx->aux1.reserve(vb));
    HIP_TRY(ctx->aux2.reserve(vb));
    HIP_TRY(ctx->aux3.reserve(vb));
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(ctx->params.ptr, params, pb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->aux0.ptr, K, vb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->aux1.ptr, T, vb, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(trunc_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st,
                       (const double*)ctx->params.ptr, (const double*)ctx->aux0.ptr,
                       (const double*)ctx->aux1.ptr, P, L, (double*)ctx->aux2.ptr,
                       (double*)ctx->aux3.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(a, ctx->aux2.ptr, vb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(b, ctx->aux3.ptr, vb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}

int dh_cos_coeffs(dh_ctx* ctx, const int32_t* k, int n, double c, double d, double a, double b,
                  double* chi, double* psi) {
    if (!ctx || (n > 0 && (!k || !chi || !psi))) return fail(DH_E_ARG, "null argument");
    if (n < 0) return fail(DH_E_ARG, "n < 0");
    if (n == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t vb = (size_t)n * 8;
    HIP_TRY(ctx->aux0.reserve((size_t)n * 4));
    HIP_TRY(ctx->aux1.reserve(vb));
    HIP_TRY(ctx->aux2.reserve(vb));
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(ctx->aux0.ptr, k, (size_t)n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(coeff_kernel, dim3((n + 255) / 256), dim3(256), 0, st,
                       (const int32_t*)ctx->aux0.ptr, n, c, d, a, b, (double*)ctx->aux1.ptr,
                       (double*)ctx->aux2.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(chi, ctx->aux1.ptr, vb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(psi, ctx->aux2.ptr, vb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// one-shot entry points in the shape SURVEY.md 8(b) proposes (a surface per call)
// ----------------------------------------------------------------------------------------------
extern "C" int dh_price_batch(dh_ctx* ctx, const double* params, int64_t P, const double* K,
                              const double* T, const int8_t* is_call, int M, int N, double L,
                              double* out) {
    if (!ctx || (P > 0 && M > 0 && (!params || !out))) return fail(DH_E_ARG, "null argument");
    if (P < 0) return fail(DH_E_ARG, "P < 0");
    dh_surface* s = nullptr;
    int rc = dh_surface_create(ctx, K, T, is_call, nullptr, M, DH_STRIKE_ABSOLUTE, &s);
    if (rc) return rc;
    rc = dh_surface_price(ctx, s, params, P, N, L, out);
    dh_surface_destroy(s);
    return rc;
}

extern "C" int dh_loss_batch(dh_ctx* ctx, const double* x, int S, const double* K, const double* T,
                             const int8_t* is_call, const double* mkt, int M, double S0, double r,
                             int N, double L, double* loss, int32_t* n_invalid) {
    if (!ctx || (S > 0 && (!x || !loss || !n_invalid))) return fail(DH_E_ARG, "null argument");
    if (S < 0) return fail(DH_E_ARG, "S < 0");
    if (M > 0 && !mkt) return fail(DH_E_ARG, "mkt is null");
    int rc = check_N(N);
    if (rc) return rc;
    if (S == 0) return DH_OK;
    if (M == 0) {                                   // np.mean([]) -> nan (lbfgs_calibrator.py:163)
        for (int i = 0; i < S; ++i) {
            loss[i] = __builtin_nan("");
            n_invalid[i] = 0;
        }
        return DH_OK;
    }
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    dh_surface* s = nullptr;
    rc = dh_surface_create(ctx, K, T, is_call, mkt, M, DH_STRIKE_ABSOLUTE, &s);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    const size_t xb = (size_t)S * dhlb::kN * 8;
    auto run = [&]() -> int {
        HIP_TRY(ctx->aux0.reserve(xb));
        HIP_TRY(ctx->aux1.reserve((size_t)S * DH_PARAM_STRIDE * 8));
        HIP_TRY(ctx->aux2.reserve((size_t)S * 8 * 3));     // pen | sse | loss
        HIP_TRY(ctx->aux3.reserve((size_t)S * 4));
        double* d_x = (double*)ctx->aux0.ptr;
        double* d_rec = (double*)ctx->aux1.ptr;
        double* d_pen = (double*)ctx->aux2.ptr;
        double* d_sse = d_pen + S;
        double* d_loss = d_sse + S;
        int* d_bad = (int*)ctx->aux3.ptr;
        HIP_TRY(hipMemcpyAsync(d_x, x, xb, hipMemcpyHostToDevice, st));
        const unsigned b = (unsigned)((S + 255) / 256);
        hipLaunchKernelGGL(x_records_kernel, dim3(b), dim3(256), 0, st, d_x, S, S0, r, d_rec, d_pen);
        HIP_TRY(hipGetLastError());
        int e = surface_loss_launch(ctx, s, d_rec, S, N, L, d_sse, (int32_t*)d_bad, nullptr, st,
                                    nullptr);
        if (e) return e;
        hipLaunchKernelGGL(loss_finalize_kernel, dim3(b), dim3(256), 0, st, d_sse, d_bad, d_pen, S,
                           s->M, d_loss);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(loss, d_loss, (size_t)S * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(n_invalid, d_bad, (size_t)S * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return DH_OK;
    };
    rc = run();
    dh_surface_destroy(s);
    return rc;
}

// ----------------------------------------------------------------------------------------------
// function + FD-gradient requests for the host (SciPy) driver
// ----------------------------------------------------------------------------------------------
namespace {

// The request's points (scipy/optimize/_numdiff.py:498-511: x0, then x0 + h_i e_i with h = 1e-8,
// or sqrt(eps) sign(x) max(1, |x|) where the absolute step vanishes), their model params (exp /
// tanh / identity, lbfgs_calibrator.py:62-87) and Feller penalties (:113-116): rec [S * 14][16],
// pen [S * 14], dx [S][13].  The caller passes the model params of x0 and x0 + h (model:
// [2][S][13]) when they must be the bits of its own exp / tanh (NumPy's, as the reference's
// transform_params); otherwise they come from libm here.
void fg_points(const double* x0, const double* model, int S, double S0, double r, double* rec,
               double* pen, double* dx) {
    constexpr int kP = dhlb::kPts, kN = dhlb::kN;
    for (int st = 0; st < S; ++st) {
        const double* x = x0 + (size_t)st * kN;
        double pb[kN], pp[kN];
        for (int i = 0; i < kN; ++i) {
            double h = kFdStep;
            if ((x[i] + h) - x[i] == 0.0)
                h = kSqrtEps * (x[i] >= 0.0 ? 1.0 : -1.0) * std::max(1.0, std::fabs(x[i]));
            const double xh = x[i] + h;
            dx[(size_t)st * kN + i] = xh - x[i];
            if (model) {
                pb[i] = model[(size_t)st * kN + i];
                pp[i] = model[((size_t)S + st) * kN + i];
            } else {
                pb[i] = lb_transform(i, x[i]);
                pp[i] = lb_transform(i, xh);
            }
        }
        for (int t = 0; t < kP; ++t) {
            double* o = rec + ((size_t)st * kP + t) * DH_PARAM_STRIDE;
            for (int i = 0; i < kN; ++i) o[i] = (i == t - 1) ? pp[i] : pb[i];
            pen[(size_t)st * kP + t] = feller_penalty(o);
            o[13] = S0;
            o[14] = r;
            o[15] = 0.0;
        }
    }
}

// loss = n_bad ? 1e10 : sse / M + Feller (lbfgs_calibrator.py:152-166); f, the FD gradient
// (f_i - f_0) / dx_i as SciPy forms it, and the smallest valid loss of the request
void fg_finish(int S, int M, const double* sse, const int32_t* bad, const double* pen,
               const double* dx, double* f, double* g, double* low) {
    constexpr int kP = dhlb::kPts, kN = dhlb::kN;
    for (int st = 0; st < S; ++st) {
        double lo = __builtin_huge_val(), fl[kP];
        for (int t = 0; t < kP; ++t) {
            const size_t i = (size_t)st * kP + t;
            fl[t] = bad[i] > 0 ? kInvalidLoss : sse[i] / (double)M + pen[i];
            if (fl[t] == fl[t] && fl[t] != kInvalidLoss && fl[t] < lo) lo = fl[t];
        }
        f[st] = fl[0];
        low[st] = lo;
        for (int i = 0; i < kN; ++i)
            g[(size_t)st * kN + i] = (fl[i + 1] - fl[0]) / dx[(size_t)st * kN + i];
    }
}

int fg_check(const dh_surface* s, int S) {
    if (!s->has_mkt) return fail(DH_E_ARG, "surface has no market prices");
    if (s->M == 0) return fail(DH_E_ARG, "empty market (the loss is NaN)");
    if (S < 0) return fail(DH_E_ARG, "S < 0");
    return DH_OK;
}

}  // namespace

extern "C" int dh_surface_fg(dh_ctx* ctx, const dh_surface* s, const double* x0,
                             const double* model, int S, double S0, double r, int N, double L,
                             double* f, double* g, double* low) {
    if (!ctx || !s || (S > 0 && (!x0 || !f || !g || !low))) return fail(DH_E_ARG, "null argument");
    int rc = fg_check(s, S);
    if (rc) return rc;
    if (S == 0) return DH_OK;
    const size_t P = (size_t)S * dhlb::kPts;
    std::vector<double> rec(P * DH_PARAM_STRIDE), pen(P), dx((size_t)S * dhlb::kN), sse(P);
    std::vector<int32_t> bad(P);
    fg_points(x0, model, S, S0, r, rec.data(), pen.data(), dx.data());
    rc = dh_surface_loss(ctx, s, rec.data(), (int)P, N, L, sse.data(), bad.data(), nullptr);
    if (rc) return rc;
    fg_finish(S, s->M, sse.data(), bad.data(), pen.data(), dx.data(), f, g, low);
    return DH_OK;
}

extern "C" int dh_surface_fg_begin(dh_ctx* ctx, const dh_surface* s, const double* x0,
                                   const double* model, int S, double S0, double r, int N,
                                   double L, int slot) {
    if (!ctx || !s || (S > 0 && !x0)) return fail(DH_E_ARG, "null argument");
    if (slot < 0 || slot >= DH_FG_SLOTS) return fail(DH_E_ARG, "slot out of range");
    int rc = fg_check(s, S);
    if (rc) return rc;
    rc = check_N(N);
    if (rc) return rc;
    if (s->ctx && s->ctx->device != ctx->device)
        return fail(DH_E_ARG, "surface and context are on different devices");
    auto& F = ctx->fg[slot];
    if (F.pending) return fail(DH_E_ARG, "slot has a request in flight (call dh_surface_fg_end)");
    const size_t P = (size_t)S * dhlb::kPts;
    if (P > (size_t)kZeroCopyMaxSets)
        return fail(DH_E_ARG, "too many starts for one asynchronous request (use dh_surface_fg)");
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    // The loss launch may grow the context's device scratch (partials, counters, the prologue
    // buffer, table / clamp workspaces), whose sizes follow from the surface, N and the param-set
    // count only.  A grow frees buffers the other slot's enqueued launch still reads.  hipFree
    // happens to synchronise the device first, but nothing here relies on that: wait for the
    // other slots (their requests share the stream) whenever this request is not covered by an
    // earlier one on the same surface and N (the pipelined SciPy driver's requests always are,
    // after its first round).
    const size_t units = P * (size_t)std::max(s->n_tiles, s->n_groups);
    const bool covered = s == ctx->fg_surf && N == ctx->fg_N && units <= ctx->fg_max_units;
    bool others = false;
    for (int o = 0; o < DH_FG_SLOTS; ++o) others = others || (o != slot && ctx->fg[o].pending);
    if (others && !covered) HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (s != ctx->fg_surf || N != ctx->fg_N) {
        ctx->fg_surf = s;
        ctx->fg_N = N;
        ctx->fg_max_units = 0;
    }
    ctx->fg_max_units = std::max(ctx->fg_max_units, units);
    HIP_TRY(F.h_params.reserve(P * DH_PARAM_STRIDE * 8));
    HIP_TRY(F.h_loss.reserve(P * 12));
    F.pen.resize(P);
    F.dx.resize((size_t)S * dhlb::kN);
    if (!F.done) HIP_TRY(hipEventCreateWithFlags(&F.done, hipEventDisableTiming));
    F.S = S;
    F.M = s->M;
    F.surf = s;
    if (S == 0) {
        HIP_TRY(hipEventRecord(F.done, ctx->stream));
        F.pending = true;
        return DH_OK;
    }
    fg_points(x0, model, S, S0, r, (double*)F.h_params.ptr, F.pen.data(), F.dx.data());
    // the records also travel in the fused launch's kernel arguments when they fit (KargParams)
    ctx->kp_src = (const double*)F.h_params.ptr;
    ctx->kp_surf = s;
    ctx->kp_n = (int64_t)P;
    ctx->kp_done = F.done;
    ctx->kp_done_set = false;
    rc = dh_surface_loss_dev(ctx, s, (const double*)F.h_params.dptr, (int)P, N, L,
                             (double*)F.h_loss.dptr, (int32_t*)((double*)F.h_loss.dptr + P),
                             nullptr, ctx->stream);
    ctx->kp_src = nullptr;
    ctx->kp_surf = nullptr;
    ctx->kp_n = 0;
    ctx->kp_done = nullptr;
    if (rc) return rc;
    if (!ctx->kp_done_set) HIP_TRY(hipEventRecord(F.done, ctx->stream));
    ctx->kp_done_set = false;
    F.pending = true;
    return DH_OK;
}

extern "C" int dh_surface_fg_end(dh_ctx* ctx, const dh_surface* s, int slot, int S, double* f,
                                 double* g, double* low) {
    if (!ctx || !s) return fail(DH_E_ARG, "null argument");
    if (slot < 0 || slot >= DH_FG_SLOTS) return fail(DH_E_ARG, "slot out of range");
    auto& F = ctx->fg[slot];
    if (!F.pending) return fail(DH_E_ARG, "no request in flight in this slot");
    // the slot belongs to the context: the caller must name the request it enqueued (its surface
    // and start count, which size f / g / low), else its buffers may be smaller than F.S rows
    if (s != F.surf) return fail(DH_E_ARG, "slot's request was enqueued on another surface");
    if (S != F.S)
        return fail(DH_E_ARG, "slot's request has " + std::to_string(F.S) + " starts, caller passed " +
                                  std::to_string(S));
    if (F.S > 0 && (!f || !g || !low)) return fail(DH_E_ARG, "null argument");
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t P = (size_t)F.S * dhlb::kPts;
    for (;;) {                          // busy-wait: an optimizer iteration waits on it
        const hipError_t e = hipEventQuery(F.done);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) {
            F.pending = false;
            return fail(DH_E_HIP, std::string("hipEventQuery: ") + hipGetErrorString(e));
        }
    }
    F.pending = false;
    const int32_t* nb = (const int32_t*)((double*)F.h_loss.ptr + P);
    const int crc = check_loss_counts(nb, (int64_t)P);
    if (crc) return crc;
    fg_finish(F.S, F.M, (const double*)F.h_loss.ptr, nb, F.pen.data(), F.dx.data(), f, g, low);
    return DH_OK;
}

extern "C" int dh_surface_fg_cancel(dh_ctx* ctx, int slot) {
    if (!ctx) return fail(DH_E_ARG, "null argument");
    if (slot < 0 || slot >= DH_FG_SLOTS) return fail(DH_E_ARG, "slot out of range");
    auto& F = ctx->fg[slot];
    if (!F.pending) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    F.pending = false;                  // cleared even if the wait fails: the slot is usable again
    HIP_TRY(hipEventSynchronize(F.done));
    return DH_OK;
}
