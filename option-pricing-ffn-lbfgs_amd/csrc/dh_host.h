// dh_host.h -- what every host-side part of the request library shares: the error plumbing
// (g_err / fail, HIP_TRY), the grow-only device and mapped-host buffers, the context and surface
// objects of the C ABI (include/dhcos.h), DeviceScope, and the small argument checks.  Host code
// only.  Included by dh_kernels.hip after the kernels; it needs none of them.
#pragma once

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return fail(DH_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));      \
    } while (0)

// Device memory (grow-only).  A buffer frees itself with its owner (dh_ctx, dh_comm: deleted with
// their device current), so a feature's scratch is one member and nothing to release by hand.
struct DevBuf {
    void* ptr = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(bytes, 4096);
        hipError_t e = hipMalloc(&ptr, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

// Pinned, device-mapped host memory (grow-only): small request inputs and outputs the kernels
// read and write directly over PCIe, so a host-API request is one launch and one sync.
struct HostBuf {
    void* ptr = nullptr;       // host address
    void* dptr = nullptr;      // device address of the same bytes
    size_t cap = 0;
    HostBuf() = default;
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
    ~HostBuf() { release(); }
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        const size_t want = std::max<size_t>(bytes, 4096);
        hipError_t e = hipHostMalloc(&ptr, want, hipHostMallocMapped | hipHostMallocCoherent);
        if (e != hipSuccess) {
            ptr = nullptr;
            return e;
        }
        e = hipHostGetDevicePointer(&dptr, ptr, 0);
        if (e != hipSuccess) {
            release();
            return e;
        }
        cap = want;
        return hipSuccess;
    }
    void release() {
        if (ptr) (void)hipHostFree(ptr);
        ptr = dptr = nullptr;
        cap = 0;
    }
};

// resident blocks of the persistent kernels, whole chip (ensure_attrs, dh_launch.h)
struct dh_ctx_view {
    int resident[3] = {0, 0, 0};       // cos_table_kernel<64 / 128 / 256>
    int resident_gen[3] = {0, 0, 0};   // cos_gen_kernel<16 / 8 / 4> at its N's LDS
};

}  // namespace

struct GenBufs;                         // dh_gen_device.h
void gen_bufs_release(dh_ctx* ctx);

struct dh_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    DevBuf params, out, sse, bad, part_sse, part_bad, counter, exact_prices, table, consts, cl_mask,
        cl_price, aux0, aux1, aux2, aux3, pre;
    HostBuf h_params, h_loss;  // zero-copy inputs / outputs of small host-API loss requests
    HostBuf h_pairs;           // zero-copy inputs / outputs of small dh_price_pairs calls
    DevBuf lb_state, lb_rec, lb_sse, lb_bad, lb_live, lb_done, lb_x0;   // dh_calibrate_lbfgs
    HostBuf h_lb;              // finished flags / live list of dh_calibrate_lbfgs
    // the two in-flight slots of dh_surface_fg_begin / _end: zero-copy records in, sse / n_bad
    // out, the host-side Feller terms and FD steps, and the request's completion event
    // largest (param sets x tasks) of any dh_surface_fg_begin request on (fg_surf, fg_N): the
    // scratch reservations are a function of the surface, N and the param-set count only
    size_t fg_max_units = 0;
    const dh_surface* fg_surf = nullptr;
    int fg_N = 0;
    struct FgSlot {
        HostBuf h_params, h_loss;
        std::vector<double> pen, dx;
        int S = 0, M = 0;
        const dh_surface* surf = nullptr;   // the surface the request was enqueued on
        bool pending = false;
        hipEvent_t done = nullptr;
    } fg[DH_FG_SLOTS];
    DevBuf lb_trace, lb_trace_n;   // diagnostic request trace of dh_calibrate_lbfgs
    hipEvent_t lb_ev[2] = {nullptr, nullptr};   // chunk-completion events of dh_calibrate_lbfgs
    int64_t lb_trace_cap = 0;
    bool attr_set = false;
    dh_ctx_view view;
    int exact = 0;          // validation mode: every option through the per-term exact path
    int tail_cut = 1;       // adaptive tail of the angle sums (tail_delta; dh_ctx_set_tail_cut)
    int path = DH_PATH_AUTO;   // fused / split request kernels (dh_ctx_set_path)
    int last_path = 0;         // kernels of the last fast-path request (dh_ctx_last_path)
    int stamps_on = 0;      // diagnostic builds: record per-block phase stamps
    DevBuf stamps;
    int64_t stamps_n = 0;
    // prologues ahead (launch_fused): constants and flags of the later-round tables, the launch
    // epoch, and the resident-block counts of the fused kernel builds it applies to, by (t1, r1,
    // LDS bytes)
    DevBuf ahead, ahead_flag;
    size_t ahead_flag_cap = 0;
    DevBuf gran;               // tail_sums' granules (partials_only == 3), zeroed on allocation
    size_t gran_cap = 0;
    unsigned ahead_epoch = 0;
    std::vector<std::pair<std::array<int64_t, 3>, int>> resident_fused;
    // launch_fused's one-digit environment switches (env_digit, dh_launch.h; -1: not read yet)
    int remap_on = -1;         // $DHCOS_XCD_REMAP: one-round fused grids map blocks to tables by XCD
                               // (xcd_table; 0 off, 2 multi-round grids too)
    int ahead_on = -1;         // $DHCOS_AHEAD: 0 turns the prologues ahead off
    int kp_on = -1;            // $DHCOS_KARG_PARAMS: 0 keeps the records out of the arguments
    int ext_on = -1;           // $DHCOS_EXT_EVENT: 0 records kp_done by a separate hipEventRecord
    int defer_on = -1;         // $DHCOS_DEFER: multi-round fused loss requests sum their partials
                               // in the launch's tail (2), in loss_partials_kernel (1) or through
                               // the ticket hand-off (0)
    // the host copy of the next fused launch's param records (dh_surface_fg_begin sets it
    // around its launch): fused launches of <= kKargSets records pass them in their kernel
    // arguments
    const double* kp_src = nullptr;
    const dh_surface* kp_surf = nullptr;   // and its surface (host copies of the groups)
    int64_t kp_n = 0;
    // and its completion event: recorded by the launch itself (hipExtLaunchKernel's stop event)
    // when the fused kernel is the request's last launch; kp_done_set tells the caller
    hipEvent_t kp_done = nullptr;
    bool kp_done_set = false;
    GenBufs* gen = nullptr;    // the generator's device draw (dh_gen_device)
    DevBuf iv;                 // quote columns / vols of dh_implied_vol, dh_surface_implied_vol
    DevBuf iv_part_sse, iv_part_bad;   // tile partials of dh_surface_iv_sse_dev (dh_iv_loss.h)
    DevBuf rows_mkt, rows_row;         // market rows / row of each set (dh_loss_rows.h)
    // dh_calibrate_lbfgs_batch: the requests' prices, and each start's spot, rate and market
    DevBuf lb_prices, lb_spot, lb_rate, lb_mof;
    // the vol-space rows (dh_loss_rows.h): weight rows [B][M], each start's weight sum; each
    // market's [B] (dh_calibrate_lbfgs_batch_iv_grad)
    DevBuf rows_wgt, lb_div, lb_wsum;
    // the Monte Carlo pricer (dh_mc.h): staged records, sorted options / observation steps, the
    // blocks' partial sums (two per option, five under a control), staged outputs
    DevBuf mc_params, mc_opts, mc_part, mc_out;
    // its control variate (dh_mc_vr.h): the records with q zeroed, the twins' COS prices; the
    // twins' surface, the (strike, maturity, type) list it was built from and the stream of the
    // last call that read it
    DevBuf mc_vr_rec, mc_vr_cos;
    dh_surface* vr_surf = nullptr;
    std::vector<double> vr_key;
    hipStream_t vr_stream = nullptr;
    // the least-squares Monte Carlo pricer (dh_lsm.h): the states at the exercise dates, each
    // option's cashflow and exercise date per path, the blocks' normal-equation and price
    // partials, options, per-set discounts, coefficients, staged outputs
    DevBuf lsm_state, lsm_cash, lsm_tau, lsm_part, lsm_fin, lsm_opts, lsm_disc, lsm_coef, lsm_out;    // the Greeks kernel (dh_greeks.h): the dynamic-LDS cap raised for it on this context's device
    // (bytes; 0: not yet)
    int greeks_lds = 0;
    // the full Greeks kernel (dh_greeks_full.h): its dynamic-LDS cap likewise
    int greeks_full_lds = 0;
    // the parameter-gradient kernel (dh_param_grad.h): its dynamic-LDS cap likewise; the records,
    // penalties and [14][S][M] planes of a loss_grad request; the host form's x, f, g and bad
    int param_grad_lds = 0;
    DevBuf pg_scratch, pg_io;
};

// dh_surface::spot_staged before any staging: a NaN's bits, which dh_surface_stage_spot refuses
constexpr uint64_t kSpotNone = ~uint64_t(0);

struct dh_surface {
    dh_ctx* ctx = nullptr;
    int M = 0;
    int n_tiles = 0;
    int n_groups = 0;       // distinct maturities
    int max_nopt = 0;       // largest tile
    int max_group = 0;      // largest maturity group
    int strike_mode = 0;
    bool has_mkt = false;
    double* K = nullptr;
    double* T = nullptr;
    double* mkt = nullptr;
    int8_t* call = nullptr;
    int* perm = nullptr;
    int2* tiles = nullptr;
    int* tile_group = nullptr;
    double* group_T = nullptr;
    int2* groups = nullptr;
    void* block = nullptr;  // the one device allocation every array above points into
    // dh_surface_set_iv_market (dh_iv_loss.h): market vols and weights [M] in the caller's option
    // order, in an allocation of their own
    bool has_iv = false;
    double* iv_mkt = nullptr;
    double* iv_wgt = nullptr;
    void* iv_block = nullptr;
    // dh_surface_stage_spot (dh_api.h): log(K / S0), K / S0 and the strike (K itself unless
    // DH_STRIKE_PCT_SPOT) [M] in the sorted option order, formed for the S0 whose 64 bits
    // spot_staged holds, in an allocation of their own
    uint64_t spot_staged = kSpotNone;
    double* xk_s = nullptr;
    double* exk_s = nullptr;
    double* k_s = nullptr;
    void* spot_block = nullptr;
    std::vector<double> h_group_T;  // host copies of group_T / groups (the fused launch's
    std::vector<int2> h_groups;      // kernel arguments, KargParams)
};

// Makes the context's device current for one C-ABI call and restores the caller's device on
// return.  The HIP runtime is shared with torch (one libamdhip64 per process), so leaving another
// device current would move torch's current device under the caller (a rank's RCCL tensors would
// land on the wrong GPU).
struct DeviceScope {
    int prev = -1;
    int rc = DH_OK;
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev == device) return;
        const hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) {
            rc = fail(DH_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
            prev = -1;
        }
    }
    ~DeviceScope() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

namespace {

constexpr int kZeroCopyMaxSets = 1024;       // host-API loss requests up to this many param sets
                                             // read / write through mapped host memory

// Requests run the per-term path (cos_exact_kernel) in validation mode, and for series longer
// than the fast path's LDS-resident table holds (N > DH_MAX_N).
bool per_term(const dh_ctx* ctx, int N) { return ctx->exact || N > DH_MAX_N; }

int check_N(int N) {
    if (N < 1 || N > DH_MAX_N_PER_TERM)
        return fail(DH_E_ARG, "N must be in [1, " + std::to_string(DH_MAX_N_PER_TERM) + "], got " +
                                  std::to_string(N));
    return DH_OK;
}

// A negative invalid count is tail_sums' timeout marker (a loss hand-off that never completed):
// an error, not a loss
int check_loss_counts(const int32_t* n_bad, int64_t S) {
    for (int64_t i = 0; i < S; ++i)
        if (n_bad[i] < 0)
            return fail(DH_E_HIP, "loss hand-off timed out in the fused kernel (param set " +
                                      std::to_string(i) + ")");
    return DH_OK;
}

// Busy-wait for a short request (a calibration iteration waits on it): polling hipStreamQuery
// returns as soon as the stream drains, where hipStreamSynchronize may yield the thread.
int spin_sync(hipStream_t st) {
    for (;;) {
        const hipError_t e = hipStreamQuery(st);
        if (e == hipSuccess) return DH_OK;
        if (e != hipErrorNotReady)
            return fail(DH_E_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(e));
    }
}

// A loss request or reduction stage between its argument checks and its launches: S < 0 is an
// error and S == 0 nothing; a surface with no option gets sse and n_bad zeroed, no launch;
// otherwise launch(st) runs with the context's device current.
template <typename Launch>
int loss_stage(dh_ctx* ctx, const dh_surface* s, int S, double* d_sse, int32_t* d_n_bad,
               void* stream, Launch&& launch) {
    if (S < 0) return fail(DH_E_ARG, "S < 0");
    if (S == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    if (s->M == 0) {
        HIP_TRY(hipMemsetAsync(d_sse, 0, (size_t)S * 8, st));
        HIP_TRY(hipMemsetAsync(d_n_bad, 0, (size_t)S * 4, st));
        return DH_OK;
    }
    return launch(st);
}

}  // namespace
