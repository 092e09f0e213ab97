// dh_launch.h -- the launch planner of the pricing requests: which kernels a request runs
// (launch_price: per-term, fused, generator or table + option kernels), at what
// shapes, and the one table of kernel builds those choices index.  Host code only.  Included by
// dh_kernels.hip after dh_host.h; it needs the request kernels, their shape helpers and dh_ctx.
#pragma once

namespace {

// Threads per table.  The fused kernel takes one entry per thread up to N = 256 (latency).  The
// split path's table kernel takes the slot width (64, 128 or 256 threads; 64 = one wave per table
// defines the canonical order of the k-sums, which the others re-form from LDS) that minimises
// rounds of resident slots x entries per thread; 64 unless a wider slot saves >= 10% (requests
// with few tables per slot, e.g. C3: 4,200 tables on 3,072 one-wave slots).
int fused_tpt(int N) { return N <= 64 ? 64 : (N <= 128 ? 128 : 256); }

// cos_gen_kernel<TB>: TB tables' (T2, T6) in LDS, <= 32 KB per block (three blocks per CU)
constexpr int gen_max_n(int TB) { return 2048 / TB; }
int gen_tb(int N) { return N <= gen_max_n(16) ? 16 : (N <= gen_max_n(8) ? 8 : (N <= gen_max_n(4) ? 4 : 0)); }

int table_tpt(const dh_ctx_view& v, int64_t n_q, int N) {
    auto cost = [&](int i) {
        const int tpt = 64 << i;
        const int64_t slots = (int64_t)std::max(1, v.resident[i]) * (kBlock / tpt);
        return (double)((n_q + slots - 1) / slots) * (double)((N + tpt - 1) / tpt);
    };
    const double c64 = cost(0);
    int best = 0;
    double bc = c64;
    for (int i = 1; i < 3; ++i) {
        if ((64 << i) > N) break;
        const double c = cost(i);
        if (c < bc && c <= 0.9 * c64) {
            best = i;
            bc = c;
        }
    }
    return 64 << best;
}

// option-kernel threads per task: enough lanes for ceil(nopt/kR) groups, LDS permitting
#ifndef DH_BIG_TILE_TPT
#define DH_BIG_TILE_TPT 256   // option threads of tiles of more than 64 options (128: G <= 4 lanes
#endif                        // per 4-option group on C3's 100-option tiles)
int option_tpt(int max_nopt, int N, int cap) {
    int tpt = max_nopt <= kR ? 64 : (max_nopt <= 4 * kR ? 128 : (max_nopt > 64 ? DH_BIG_TILE_TPT : 256));
    while (tpt < kBlock &&
           ((size_t)(kBlock / tpt) * option_lds_doubles(N, cap) + (tpt == kBlock ? kRedDoubles : 0)) *
                   sizeof(double) > (size_t)kLdsDyn)
        tpt *= 2;
    return tpt;
}

size_t fused_lds_bytes(int N, int cap) {
    return ((size_t)option_lds_doubles(N, cap) + (size_t)cap + kRedDoubles) * sizeof(double);
}

#ifndef DH_FUSED_WIDE_MIN_BLOCKS
#define DH_FUSED_WIDE_MIN_BLOCKS 4096
#endif
constexpr int64_t kFusedWideMinBlocks = DH_FUSED_WIDE_MIN_BLOCKS;
// fused grids from this size take their prologue constants from table_prologue_kernel (C4's
// 28,672 blocks: 297 -> 285 us; C3's 4,200 lose 3% to the extra launch, C2's 448 its latency)
#ifndef DH_PROLOGUE_KERNEL_MIN_BLOCKS
#define DH_PROLOGUE_KERNEL_MIN_BLOCKS 8192
#endif
constexpr int64_t kPrologueKernelMinBlocks = DH_PROLOGUE_KERNEL_MIN_BLOCKS;

// A one-digit environment switch, read once per context: `cache` is its int in dh_ctx (-1: not
// read yet).  A first character in '0' .. '0' + max is the value; anything else, or no variable,
// gives `dflt`.
int env_digit(int& cache, const char* name, int max, int dflt) {
    if (cache < 0) {
        const char* e = std::getenv(name);
        cache = (e && e[0] >= '0' && e[0] <= '0' + max) ? e[0] - '0' : dflt;
    }
    return cache;
}

// The kernel builds: the instantiations of the table, generator, option and fused kernels are
// named here and nowhere else.  ensure_attrs walks these tables, the launches index them.
using PriceKernel = void (*)(PriceArgs);
using GenKernel = void (*)(PriceArgs, int);

PriceKernel table_kernel(int tpt) {
    return tpt == 64 ? cos_table_kernel<64> : (tpt == 128 ? cos_table_kernel<128> : cos_table_kernel<256>);
}

GenKernel gen_kernel(int TB) {
    return TB == 16 ? cos_gen_kernel<16> : (TB == 8 ? cos_gen_kernel<8> : cos_gen_kernel<4>);
}

PriceKernel option_kernel(int tpt, bool r1) {
    if (r1) return tpt == 64 ? cos_option_kernel<64, 1> : (tpt == 128 ? cos_option_kernel<128, 1> : cos_option_kernel<256, 1>);
    return tpt == 64 ? cos_option_kernel<64, kR> : (tpt == 128 ? cos_option_kernel<128, kR> : cos_option_kernel<256, kR>);
}

// One build of cos_fused_kernel as a type.  Its argument lists differ (FusedKargs, FusedKargsKP),
// so a build is handed to a generic callable (for_fused_build) instead of returned as a pointer.
template <int T1, int RT, int WV = DH_FUSED_WAVES, bool KP = false>
struct FusedBuild {
    static const void* fn() { return (const void*)cos_fused_kernel<T1, RT, WV, KP>; }
    // The typed launch of args..., then the records `pb` (KP) or the placeholder.  The KP build
    // (a host request's last launch) may record the request's completion event `stop` itself.
    template <typename... Args>
    static void launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, hipEvent_t stop,
                       const KargParams& pb, const Args&... args) {
        if constexpr (KP)
            hipExtLaunchKernelGGL((cos_fused_kernel<T1, RT, WV, KP>), grid, block, lds, st, nullptr,
                                  stop, 0, args..., pb);
        else
            hipLaunchKernelGGL((cos_fused_kernel<T1, RT, WV, KP>), grid, block, lds, st, args...,
                               NoKargParams{});
    }
};

// The four builds of one t1: both option-lane layouts at the default waves, and for r1 alone the
// wide (5-wave) build and the one with the records in its arguments.
template <int T1, typename F>
int fused_row(bool r1, bool wide, bool kp, F&& f) {
    if (!r1) return f(FusedBuild<T1, kR>{});
    if (kp) return f(FusedBuild<T1, 1, DH_FUSED_WAVES, true>{});
    return wide ? f(FusedBuild<T1, 1, DH_FUSED_WAVES_WIDE>{}) : f(FusedBuild<T1, 1>{});
}

// f(FusedBuild<...>{}) for the build of (t1 in {64, 128, 256}, r1, wide, kp); returns f's code
template <typename F>
int for_fused_build(int t1, bool r1, bool wide, bool kp, F&& f) {
    if ((wide || kp) && (!r1 || (wide && kp))) return fail(DH_E_ARG, "no such fused kernel build");
    if (t1 == 64) return fused_row<64>(r1, wide, kp, f);
    return t1 == 128 ? fused_row<128>(r1, wide, kp, f) : fused_row<256>(r1, wide, kp, f);
}

const void* fused_fn(int t1, bool r1, bool wide, bool kp) {
    const void* f = nullptr;
    (void)for_fused_build(t1, r1, wide, kp, [&](auto b) -> int { f = b.fn(); return DH_OK; });
    return f;
}

int ensure_attrs(dh_ctx* ctx) {
    if (ctx->attr_set) return DH_OK;
    for (int t = 64; t <= 256; t *= 2) {
        for (const bool r1 : {true, false}) {
            const void* f = (const void*)option_kernel(t, r1);
            HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsDyn));
        }
        for (int i = 0; i < 4; ++i) {           // fused_row's builds: kR, 1, 1 wide, 1 kp
            const void* f = fused_fn(t, i > 0, i == 2, i == 3);
            HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsDyn));
        }
    }
    // table-kernel grid = resident capacity (each block then owns a contiguous table range)
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    for (int i = 0; i < 3; ++i) {
        // dynamic LDS at DH_MAX_N (T2 of each wider slot) so the count never overstates
        const size_t lds = i == 0 ? 0 : (size_t)(kBlock / (64 << i)) * DH_MAX_N * sizeof(double);
        const void* fns[3] = {(const void*)table_kernel(64), (const void*)table_kernel(128),
                              (const void*)table_kernel(256)};
        int per_cu = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fns[i], kBlock, lds));
        ctx->view.resident[i] = std::max(1, per_cu) * std::max(1, cus);
    }
    for (int i = 0; i < 3; ++i) {               // LDS of the largest N each build takes
        const size_t lds = (size_t)gen_max_n(16 >> i) * (16 >> i) * sizeof(double2);
        const void* gens[3] = {(const void*)gen_kernel(16), (const void*)gen_kernel(8),
                               (const void*)gen_kernel(4)};
        int per_cu = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, gens[i], kBlock, lds));
        ctx->view.resident_gen[i] = std::max(1, per_cu) * std::max(1, cus);
    }
    ctx->attr_set = true;
    return DH_OK;
}

int launch_exact(dh_ctx* ctx, const PriceArgs& A, hipStream_t st) {
    const int64_t n_items = A.paired ? A.P : A.P * (int64_t)A.M;
    double* prices = nullptr;
    if (A.part_sse) {
        HIP_TRY(ctx->exact_prices.reserve((size_t)n_items * 8));
        prices = (double*)ctx->exact_prices.ptr;
    }
    const int64_t blocks = (n_items * 64 + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffLL) return fail(DH_E_ARG, "too many items for one launch");
    hipLaunchKernelGGL(cos_exact_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, A, prices);
    HIP_TRY(hipGetLastError());
    if (A.part_sse) {
        const int64_t S = A.P;
        hipLaunchKernelGGL(loss_from_prices_kernel, dim3((unsigned)((S * 64 + kBlock - 1) / kBlock)),
                           dim3(kBlock), 0, st, (const double*)prices, A.mkt, A.M, S, A.sse,
                           A.n_bad);
        HIP_TRY(hipGetLastError());
    }
    return DH_OK;
}

// One fused launch for the whole request (every group is one tile).
int launch_fused(dh_ctx* ctx, const PriceArgs& A0, hipStream_t st) {
    const int N = A0.N;
    const int tpp = A0.paired ? 1 : A0.n_groups;
    const int t1 = fused_tpt(N);
    const int max_nopt = A0.paired ? 1 : A0.opt_cap;
    const int t2 = option_tpt(max_nopt, N, A0.opt_cap);
    const size_t lds = fused_lds_bytes(N, A0.opt_cap);
    const int64_t blocks = A0.P * tpp;
    if (blocks > 0x7fffffffLL) return fail(DH_E_ARG, "launch too large");
    PriceArgs A = A0;
    A.p0 = 0;
    A.np = A0.P;
    if (ctx->stamps_on) {
        HIP_TRY(ctx->stamps.reserve((size_t)blocks * kStamps * 8));
        HIP_TRY(hipMemsetAsync(ctx->stamps.ptr, 0, (size_t)blocks * kStamps * 8, st));
        ctx->stamps_n = blocks * kStamps;
        A.stamps = (unsigned long long*)ctx->stamps.ptr;
    }
    const dim3 grid((unsigned)blocks), block((unsigned)std::max(t1, t2));
    const double* tsrc = A.paired ? A.T : A.group_T;       // FusedHead: preloaded arguments
    const bool r1 = tile_r(max_nopt, t2) == 1;
    A.ahead = nullptr;
    A.ahead_flag = nullptr;
    A.ahead_stride = 0;
    A.gran = nullptr;
    // by XCD: one-round grids of more than one maturity group (below); multi-round grids (C3)
    // measured slower with it (57.7 vs 56.5 us per request), one-round C2 0.15 us faster
    const int remap_on = env_digit(ctx->remap_on, "DHCOS_XCD_REMAP", 2, 1);
    A.remap = 0;
    const bool remap_ok = remap_on && !A.paired && tpp > 1;
    // grids of many small blocks (C4: 28,672) gain from a fifth wave per SIMD to overlap the
    // blocks' latency-bound phases; small grids keep the 4-wave build, whose blocks are shorter
    // (same arithmetic: only the register allocation differs, so the same bits)
    const bool wide = r1 && blocks >= kFusedWideMinBlocks;
    // prologues ahead: the 4-wave build of >= 3-wave blocks, more blocks than one round of
    // resident ones, in-block prologues (no prologue kernel)
    if (env_digit(ctx->ahead_on, "DHCOS_AHEAD", 0, 1) && !wide && block.x >= 192 &&
        blocks < kPrologueKernelMinBlocks) {
        const std::array<int64_t, 3> key{t1, r1 ? 1 : 0, (int64_t)lds};
        int res = -1;
        for (const auto& kv : ctx->resident_fused)
            if (kv.first == key) res = kv.second;
        if (res < 0) {
            const void* f = fused_fn(t1, r1, false, false);
            int per_cu = 0, cus = 0;
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, (int)block.x, lds));
            HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
            res = std::max(1, per_cu) * std::max(1, cus);
            ctx->resident_fused.push_back({key, res});
        }
        const int defer = env_digit(ctx->defer_on, "DHCOS_DEFER", 2, 2);
        if (blocks > res) {
            const size_t slots = (size_t)blocks;
            HIP_TRY(ctx->ahead.reserve(slots * kAheadRec * sizeof(double)));
            if (slots > ctx->ahead_flag_cap) {
                HIP_TRY(ctx->ahead_flag.reserve(slots * sizeof(unsigned long long)));
                HIP_TRY(hipMemsetAsync(ctx->ahead_flag.ptr, 0, ctx->ahead_flag.cap, st));
                ctx->ahead_flag_cap = ctx->ahead_flag.cap / sizeof(unsigned long long);
            }
            if (++ctx->ahead_epoch == 0) ++ctx->ahead_epoch;     // 0: the cleared flags' value
            A.ahead = (double*)ctx->ahead.ptr;
            A.ahead_flag = (unsigned long long*)ctx->ahead_flag.ptr;
            A.ahead_stride = res;
            A.ahead_epoch = ctx->ahead_epoch;
            if (remap_on == 2 && remap_ok) A.remap = 1;   // C3 +1.1 us: off by default
            // and the loss sums deferred (below), or in loss_partials_kernel ($DHCOS_DEFER=1)
            if (defer == 1 && A.part_sse && !A.partials_only && !A.paired) {
                // (partial, invalid count) pairs: 16 bytes per task
                HIP_TRY(ctx->part_sse.reserve((size_t)A.P * A.n_tiles * 2 * sizeof(double)));
                A.part_sse = (double*)ctx->part_sse.ptr;
                A.partials_only = 2;
            }
        } else if (remap_ok) {
            A.remap = 1;                         // one round of resident blocks
        }
        // loss sums in the launch's tail ($DHCOS_DEFER=2, the default; 0: the hand-off's ticket in
        // every block): C3 -1.1 us against loss_partials_kernel, C2 (one round) -0.5 us against
        // the ticket.  At most a quarter of the resident blocks wait (tail_sums)
        if (defer == 2 && A.part_sse && !A.partials_only && !A.paired && A.P <= res / 4 &&
            A.max_group < (1 << kGranCountBits)) {
            if (A.ahead_stride == 0 && ++ctx->ahead_epoch == 0) ++ctx->ahead_epoch;
            A.ahead_epoch = ctx->ahead_epoch;
            const int64_t tasks = A.P * A.n_tiles;
            if ((size_t)tasks > ctx->gran_cap) {    // two granules per task, zeroed (no epoch is 0)
                HIP_TRY(ctx->gran.reserve((size_t)tasks * 2 * sizeof(unsigned long long)));
                HIP_TRY(hipMemsetAsync(ctx->gran.ptr, 0, ctx->gran.cap, st));
                ctx->gran_cap = ctx->gran.cap / (2 * sizeof(unsigned long long));
            }
            A.gran = (unsigned long long*)ctx->gran.ptr;
            A.partials_only = 3;
        }
    }
    if (blocks >= kPrologueKernelMinBlocks && !ctx->stamps_on) {
        HIP_TRY(ctx->pre.reserve((size_t)blocks * kTabC * sizeof(double)));
        A.pre = (const double*)ctx->pre.ptr;
        hipLaunchKernelGGL(table_prologue_kernel,
                           dim3((unsigned)((blocks * kPreLanes + kBlock - 1) / kBlock)),
                           dim3(kBlock), 0, st, A, blocks, (double*)ctx->pre.ptr);
        HIP_TRY(hipGetLastError());
    }
    // small requests whose records were handed over from the host (dh_surface_fg_begin): the
    // records in the kernel arguments (in-block-prologue launches of the 4-wave build), and the
    // request's completion event recorded by the launch when it is the request's last
    const bool kp = env_digit(ctx->kp_on, "DHCOS_KARG_PARAMS", 0, 1) && ctx->kp_src &&
                    ctx->kp_surf && !A.paired && (int)ctx->kp_surf->h_group_T.size() == tpp &&
                    tpp <= kKargGroups && A.P == ctx->kp_n && A.P <= kKargSets && r1 && !wide &&
                    blocks < kPrologueKernelMinBlocks && !ctx->stamps_on && !A.exact;
    KargParams pb;                           // filled for the kp build alone
    hipEvent_t stop = nullptr;
    if (kp) {
        pb = KargParams{};
        std::memcpy(pb.v, ctx->kp_src, (size_t)A.P * DH_PARAM_STRIDE * sizeof(double));
        std::memcpy(pb.T, ctx->kp_surf->h_group_T.data(), (size_t)tpp * sizeof(double));
        std::memcpy(pb.groups, ctx->kp_surf->h_groups.data(), (size_t)tpp * sizeof(int2));
        if (env_digit(ctx->ext_on, "DHCOS_EXT_EVENT", 0, 1) && A.partials_only != 2)
            stop = ctx->kp_done;
    }
    const int rc = for_fused_build(t1, r1, wide, kp, [&](auto b) -> int {
        b.launch(grid, block, lds, st, stop, pb, A.prm, tsrc, A.groups, A.live_count, A.pre, tpp,
                 A.paired, A, t2);
        HIP_TRY(hipGetLastError());
        return DH_OK;
    });
    if (rc) return rc;
    if (kp) ctx->kp_done_set = stop != nullptr;
    if (A.partials_only == 2) {
        hipLaunchKernelGGL(loss_partials_kernel, dim3((unsigned)A.P), dim3(64), 0, st,
                           (const double2*)A.part_sse, A.n_tiles, A.sse, A.n_bad);
        HIP_TRY(hipGetLastError());
    }
    return DH_OK;
}

// The generator batch path: every maturity group one tile of <= kSmallTile options, a large call
// (DESIGN.md 3.3): one persistent cos_gen_kernel launch for the whole request.
int launch_gen(dh_ctx* ctx, const PriceArgs& A0, hipStream_t st, int TB) {
    const int tpp = A0.paired ? 1 : A0.n_groups;
    const int max_nopt = A0.paired ? 1 : A0.opt_cap;
    int OP = 1;
    while (OP < max_nopt) OP *= 2;
    PriceArgs A = A0;
    A.p0 = 0;
    A.np = A0.P;
    A.partials_only = 0;
    const int64_t n_q = A.np * tpp;
    const int gi = TB == 16 ? 0 : (TB == 8 ? 1 : 2);
    const int64_t blocks = std::min<int64_t>((n_q + TB - 1) / TB, ctx->view.resident_gen[gi]);
    const size_t lds = (size_t)TB * A.N * sizeof(double2);
    if (blocks <= 0 || OP > kBlock / TB) return fail(DH_E_ARG, "generator kernel shape");
    const GenKernel kernel = gen_kernel(TB);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), lds, st, A, OP);
    HIP_TRY(hipGetLastError());
    return DH_OK;
}

// Table kernel then option kernel per chunk of param sets; the chunk keeps the table workspace
// within kTableBudget (L2/MALL-resident between the two launches).  Requests whose maturity
// groups are single tiles may instead run as one fused launch (ctx->path).
int launch_price(dh_ctx* ctx, const PriceArgs& A_in, hipStream_t st) {
    PriceArgs A0 = A_in;
    A0.tail = ctx->tail_cut ? kTailScale : -1.0;
    const int64_t tasks_per_p = A0.paired ? 1 : A0.n_tiles;
    if (A0.P * tasks_per_p == 0) return DH_OK;
    if (A0.exact) return launch_exact(ctx, A0, st);
    int rc = ensure_attrs(ctx);
    if (rc) return rc;
    const int N = A0.N;
    const int max_nopt = A0.paired ? 1 : A0.opt_cap;
    // small tiles in a large call (decided once per call, so every chunk of it runs the same
    // arithmetic)
    const bool small = max_nopt <= kSmallTile && A0.P * tasks_per_p >= kSmallMinTasks;
    const bool fusable = (A0.paired || A0.max_group <= kTileMax) &&
                         fused_lds_bytes(N, A0.opt_cap) <= (size_t)kLdsDyn;
    // auto: fused wherever it applies except small tiles in large calls (generator grids,
    // whose lane-per-option-group kernel is 1.7x faster); measured on the current kernels:
    // C3 113 vs 133 us, C4 393 vs 407 us per request
    const bool fused = fusable && (ctx->path == DH_PATH_FUSED ||
                                   (ctx->path == DH_PATH_AUTO && !small));
    ctx->last_path = fused ? DH_PATH_FUSED : DH_PATH_SPLIT;
    if (fused) return launch_fused(ctx, A0, st);
    // generator grids: one fused small-tile launch (PATH_SPLIT keeps the table + option
    // kernels, for A/B)
    const int tb = gen_tb(N);
    if (small && ctx->path == DH_PATH_AUTO && tb && (A0.paired || A0.n_tiles == A0.n_groups)) {
        ctx->last_path = DH_PATH_GEN;
        return launch_gen(ctx, A0, st, tb);
    }
    const int tpp = A0.paired ? 1 : A0.n_groups;
    const int words = cl_words(A0);
    const size_t per_p =
        (size_t)tpp * ((size_t)N + kConsts + words + (size_t)A0.max_group) * sizeof(double);
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(A0.P, kTableBudget / per_p));
    // rounded up to whole kTabTile-table tiles (the small-tile kernel's layout)
    HIP_TRY(ctx->table.reserve((size_t)((chunk * tpp + kTabTile - 1) / kTabTile) * kTabTile * N *
                               sizeof(double)));
    HIP_TRY(ctx->consts.reserve((size_t)chunk * tpp * kConsts * sizeof(double)));
    HIP_TRY(ctx->cl_mask.reserve((size_t)chunk * tpp * words * 8));
    HIP_TRY(ctx->cl_price.reserve((size_t)chunk * tpp * A0.max_group * sizeof(double)));
    // Few tables per resident slot (< 2, e.g. C3's 4,200 tables on 3,072 one-wave slots): one
    // block per kTabs tables, not persistent, so the dispatcher backfills CUs as blocks finish
    // instead of fixing each block's share up front (a 5-vs-6-table tail cost C3 ~30% of the
    // table kernel).  Otherwise a resident grid of persistent blocks and the slot width of
    // table_tpt.
    const int64_t nq_max = std::min<int64_t>(A0.P, chunk) * tpp;
    const bool backfill = nq_max < 2 * (int64_t)ctx->view.resident[0] * (kBlock / 64);
    const int t1 = backfill ? 64 : table_tpt(ctx->view, nq_max, N);
    const size_t lds1 = t1 == 64 ? 0 : (size_t)(kBlock / t1) * N * sizeof(double);
    // small tiles in a large call take the lane-per-option-group kernel
    const int rs = small_rs(max_nopt);
    int L = 1;
    while (L * rs < max_nopt) L *= 2;
    const int t2 = small ? kBlock : option_tpt(max_nopt, N, A0.opt_cap);
    const size_t lds2 =
        small ? 0 : ((size_t)(kBlock / t2) * option_lds_doubles(N, A0.opt_cap) +
                     (t2 == kBlock ? kRedDoubles : 0)) * sizeof(double);
    if (lds2 > (size_t)kLdsDyn) return fail(DH_E_ARG, "COS table does not fit in LDS");
    if (ctx->stamps_on) {
        const int64_t nb = std::max((chunk * tasks_per_p + kBlock / t2 - 1) / (kBlock / t2),
                                    (chunk * tpp + kBlock / t1 - 1) / (kBlock / t1));
        HIP_TRY(ctx->stamps.reserve((size_t)nb * kStamps * 8));
        HIP_TRY(hipMemsetAsync(ctx->stamps.ptr, 0, (size_t)nb * kStamps * 8, st));
        ctx->stamps_n = nb * kStamps;
    }
    const PriceKernel table = table_kernel(t1);
    const PriceKernel option = option_kernel(t2, tile_r(max_nopt, t2) == 1);
    for (int64_t p0 = 0; p0 < A0.P; p0 += chunk) {
        PriceArgs A = A0;
        A.partials_only = 0;        // the split kernels always finish the loss hand-off
        A.p0 = p0;
        A.np = std::min<int64_t>(chunk, A0.P - p0);
        A.table = (double*)ctx->table.ptr;
        A.table_tiled = small ? 1 : 0;
        A.consts = (double*)ctx->consts.ptr;
        A.cl_mask = (unsigned long long*)ctx->cl_mask.ptr;
        A.cl_price = (double*)ctx->cl_price.ptr;
        A.stamps = ctx->stamps_on ? (unsigned long long*)ctx->stamps.ptr : nullptr;
        const int64_t n_q = A.np * tpp;
        const int res = ctx->view.resident[t1 == 64 ? 0 : (t1 == 128 ? 1 : 2)];
        const int64_t b1 = backfill ? (n_q + kBlock / t1 - 1) / (kBlock / t1)
                                    : std::min<int64_t>((n_q + kBlock / t1 - 1) / (kBlock / t1), res);
        const int64_t n_t = A.np * tasks_per_p;
        const int64_t b2 = small ? (n_t * L + kBlock - 1) / kBlock
                                 : (n_t + kBlock / t2 - 1) / (kBlock / t2);
        if (b1 > 0x7fffffffLL || b2 > 0x7fffffffLL) return fail(DH_E_ARG, "launch too large");
        hipLaunchKernelGGL(table, dim3((unsigned)b1), dim3(kBlock), lds1, st, A);
        HIP_TRY(hipGetLastError());
        if (!small)
            hipLaunchKernelGGL(option, dim3((unsigned)b2), dim3(kBlock), lds2, st, A);
        else if (rs == 8)
            hipLaunchKernelGGL((cos_option_small_kernel<8>), dim3((unsigned)b2), dim3(kBlock), 0, st, A, L);
        else
            hipLaunchKernelGGL((cos_option_small_kernel<4>), dim3((unsigned)b2), dim3(kBlock), 0, st, A, L);
        HIP_TRY(hipGetLastError());
    }
    return DH_OK;
}

}  // namespace
