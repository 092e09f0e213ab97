// dh_lb_driver.h -- the device-resident multi-start L-BFGS-B driver (dh_calibrate_lbfgs,
// dh_calibrate_lbfgs_batch, dh_calibrate_lbfgs_batch_iv, dh_calibrate_lbfgs_batch_grad,
// dh_calibrate_lbfgs_batch_iv_grad, dh_ctx_set_lb_trace, dh_ctx_read_lb_trace): the step kernel,
// its launch and the host loop; and the Levenberg-Marquardt driver on the same host loop
// (dh_calibrate_lm_batch: lm_step_kernel around dh_lm.h's state machine).  Included by dh_kernels.hip after the loss stages (dh_iv_loss.h,
// dh_loss_rows.h, dh_param_grad.h, dh_iv_grad.h), whose launches the host loop calls;
// kInvalidLoss, kFdStep, kSqrtEps and the record arithmetic (lb_transform, feller_penalty), which
// the one-shot entry points share, stay in dh_kernels.hip.  The analytic iterations are one
// dhpg::GradRows (dh_param_grad.h) built once per run over carve_grad_scratch's layout, and one of
// the three rows launches picked once.  DESIGN.md 3.8, 3.12-3.14, 3.19-3.21, 3.23.
//
// Nothing here is contracted into FMAs: the step kernel must compute the bits of the CPU build
// of dh_lbfgs.h (tests/native/lb_host.cpp).
#pragma once
#pragma clang fp contract(off)

namespace {

// A 13-vector held one component per lane of each 16-lane row (lane l holds component l & 15;
// components 13..15 are 0): the four rows are copies, so every lane computes the same scalars
// and the state machine's branches are uniform across the wave.  Reductions are DPP
// butterflies inside each 16-lane row -- quad_perm [1,0,3,2], quad_perm [2,3,0,1],
// row_half_mirror, row_mirror -- in which both partners add the same two operands, so every lane
// of the row ends with the same bits: the pairwise tree ((p0+p1)+(p2+p3)) + ... that
// tests/native/lb_host.cpp reproduces.
struct WaveVec {
    double v;
};
__device__ __forceinline__ WaveVec operator+(WaveVec a, WaveVec b) { return {a.v + b.v}; }
__device__ __forceinline__ WaveVec operator-(WaveVec a, WaveVec b) { return {a.v - b.v}; }
__device__ __forceinline__ WaveVec operator-(WaveVec a) { return {-a.v}; }
__device__ __forceinline__ WaveVec operator*(double s, WaveVec a) { return {s * a.v}; }


__device__ __forceinline__ double row_sum(double p) {
    p = p + dpp_f64<kDppXor1>(p);
    p = p + dpp_f64<kDppXor2>(p);
    p = p + dpp_f64<kDppHalfMirror>(p);
    return p + dpp_f64<kDppMirror>(p);
}
__device__ __forceinline__ double row_max(double m) {
    m = fmax(m, dpp_f64<kDppXor1>(m));
    m = fmax(m, dpp_f64<kDppXor2>(m));
    m = fmax(m, dpp_f64<kDppHalfMirror>(m));
    return fmax(m, dpp_f64<kDppMirror>(m));
}
__device__ __forceinline__ double row_min(double m) {
    m = fmin(m, dpp_f64<kDppXor1>(m));
    m = fmin(m, dpp_f64<kDppXor2>(m));
    m = fmin(m, dpp_f64<kDppHalfMirror>(m));
    return fmin(m, dpp_f64<kDppMirror>(m));
}
__device__ __forceinline__ double dot(WaveVec a, WaveVec b) { return row_sum(a.v * b.v); }
// max |a_i|; a NaN component makes it NaN (SciPy's projected-gradient norm: any NaN gradient
// component fails the pgtol test)
__device__ __forceinline__ double amax(WaveVec a) {
    const double m = fmax(0.0, row_max(fabs(a.v)));
    return __any(a.v != a.v) ? __builtin_nan("") : m;
}
__device__ __forceinline__ bool equal(WaveVec a, WaveVec b) { return __all(a.v == b.v); }

// The pair memory in LDS: s_j, y_j as 16-double rows (lane i reads column i), rho_j and the
// two-loop's alpha_j.  Every lane computes the same scalars, so the scalar writes are uniform.
struct WaveRing {
    double* rs;                // [kM][16]
    double* ry;                // [kM][16]
    double* rdr;               // [kM] rho_j = 1 / dr_j
    double* ra;                // [kM]
    int lane;
    __device__ WaveVec s(int j) const { return {rs[j * dhlb::kLanes + (lane & 15)]}; }
    __device__ WaveVec y(int j) const { return {ry[j * dhlb::kLanes + (lane & 15)]}; }
    __device__ double rho(int j) const { return rdr[j]; }
    __device__ double& a(int j) { return ra[j]; }
    __device__ void put(int j, WaveVec sj, WaveVec yj, double d) {
        if (lane < dhlb::kLanes) {
            rs[j * dhlb::kLanes + lane] = sj.v;
            ry[j * dhlb::kLanes + lane] = yj.v;
        }
        rdr[j] = d;
    }
    __device__ void shift() {
        for (int j = 0; j + 1 < dhlb::kM; ++j) {
            if (lane < dhlb::kLanes) {
                rs[j * dhlb::kLanes + lane] = rs[(j + 1) * dhlb::kLanes + lane];
                ry[j * dhlb::kLanes + lane] = ry[(j + 1) * dhlb::kLanes + lane];
            }
            rdr[j] = rdr[j + 1];
        }
    }
};

using WaveCore = dhlb::LbCore<WaveVec, WaveRing>;

// diagnostic trace record of one consumed request: start, request number, f, x[13], g[13], 3 spare,
// then (DH_STAMPS build only) s_memtime at the step kernel's phase boundaries: start, state
// loaded, request consumed, state machine done, request emitted, end
constexpr int kLbTrace = 40;
[[maybe_unused]] constexpr int kLbStamp0 = 32;

__device__ __forceinline__ unsigned long long lb_clock() {
#ifdef DH_STAMPS
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
#else
    return 0;
#endif
}

// Global state of one start: the vectors as 16-double rows (lane i holds column i), the pair
// memory (staged in LDS by the step kernel), then the scalars.
constexpr int kLbVecs = 10;                           // x g z d t r xe ge dx pen
constexpr int kLbRing = 2 * dhlb::kM * dhlb::kLanes + dhlb::kM;   // s rows, y rows, rho
struct LbSlot {
    double vec[kLbVecs][dhlb::kLanes];
    double ring[kLbRing];
    dhlb::LbScalars s;
};

constexpr int kLbInline = 64;   // live lists up to this size travel in the kernel arguments

struct LbArgs {
    LbSlot* states;            // [S]
    const int* live;           // [n_live] start index of each slot
    const double* x0;          // [S][13] (mode 0)
    const double* sse;         // [n_live * 14] loss partial sums of the last request, slot-major
    const int* bad;            // [n_live * 14]
    double* rec;               // [n_live * 14][16] param records of the next request
    int* done;                 // [S] finished flags (pinned host memory, read between chunks)
    int* live_count;           // starts not finished yet (the loss launches halt at 0)
    double* trace;             // diagnostic: [trace_cap][kLbTrace] consumed requests, or null
    unsigned long long* trace_n;
    int64_t trace_cap;
    dhlb::LbConfig cfg;
    double S0, r;
    int M;
    int mode;                  // 0 begin at x0, 1 consume the request and advance, 2 re-emit
    int part_mode;             // 1: the request ran fused with partials_only -- sum its tile
                               // partials here (the hand-off's order); 0: read sse / bad
    const double* part_sse;    // [n_live * 14][n_tiles] (part_mode 1; sign bit: invalid price)
    int n_tiles;
    int n_inline;              // live list passed by value below (saves a dependent load), or 0
    int live_inline[kLbInline];
    // dh_calibrate_lbfgs_batch only (lb_step_kernel<., true>), appended so that nothing above
    // moves: each start's spot, rate and market, and the market row of every set of the next
    // request (what dh_loss_rows.h's reduction reads)
    const double* spot_of;     // [S]
    const double* rate_of;     // [S]
    const int* market_of;      // [S]
    int* row;                  // [n_live * 14]
    // dh_calibrate_lbfgs_batch_iv only (lb_step_kernel<., true, true>), appended again: each
    // start's loss divisor, its market's weight sum (dh_loss_rows.h)
    const double* div_of;      // [S]
    // dh_calibrate_lbfgs_batch_grad only (lb_step_kernel<., true, false, true>), appended again:
    // the analytic gradient of the last request [n_live][13] (its loss, Feller included, is sse
    // [n_live]) and the Feller penalty of each next record [n_live] (dh_param_grad.h's rows
    // reduction writes the one and reads the other)
    const double* grad;
    double* pen_out;
};
static_assert(std::is_standard_layout<LbArgs>::value, "lb_live_inline reads LbArgs by offset");

// The step kernel's leading arguments (LbHead), ahead of LbArgs: plain scalars, preloaded into
// SGPRs at wave launch (Makefile PRELOAD), so the state and partial loads of the load phase issue
// at once instead of behind a kernel-argument load.  With at most kLbPre live starts their slots'
// start indices travel here as well (lb_step_kernel<true>).
constexpr int kLbPre = 4;
// byte offset of LbArgs in the kernel-argument segment: the leading arguments in declaration order
// at their natural alignment (2 pointers, 3 + kLbPre ints = 44 bytes), then LbArgs 8-aligned
constexpr int kLbArgsKernargOff = 48;
struct LbKargs {            // lb_step_kernel's argument list as a struct (its kernarg layout)
    void* states;
    const double* part;
    int ntiles, mode, part_mode, l[kLbPre];
    LbArgs A;
};
static_assert(offsetof(LbKargs, A) == kLbArgsKernargOff, "LbArgs kernarg offset");
// karg_prefetch_lines reads up to byte 0x1b4: inside the explicit arguments and the 256 bytes of
// implicit ones every HIP kernel's segment carries after them
static_assert(sizeof(LbKargs) + 256 >= 0x1b4, "kernel-argument prefetch past the segment");

// live_inline[slot] as a scalar load straight from the kernel-argument segment; indexing the
// by-value argument compiled to a flat load
__device__ __forceinline__ int lb_live_inline(int slot) {
    typedef const __attribute__((address_space(4))) char* KargPtr;
    const KargPtr k = (KargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    return ((const __attribute__((address_space(4))) int*)(k + kLbArgsKernargOff +
                                                            offsetof(LbArgs, live_inline)))
        [slot < kLbInline ? slot : 0];
}

__device__ __forceinline__ WaveVec lb_ld(const LbSlot* g, int v, int lane) {
    return {g->vec[v][lane & 15]};
}

__device__ __forceinline__ void lb_st(LbSlot* g, int v, int lane, WaveVec x) {
    if (lane < dhlb::kLanes) g->vec[v][lane] = x.v;
}

// Emit the pending request at xe.  Lanes i and 16 + i (i < 13) form x_i + h_i (SciPy's step rule,
// scipy/optimize/_numdiff.py:498-511); lane i maps x_i and lane 16 + i maps x_i + h_i to a model
// param (one transform per lane), lane i keeps dx_i = (x_i + h_i) - x_i; lane t < 14 assembles
// point t (x, or x + h_{t-1} e_{t-1}), writes its record and keeps its Feller penalty
// (lbfgs_calibrator.py:113-116) in pen.  kB (the multi-market driver): the record carries start
// sidx's own spot and rate, and the set's market row is written beside it.
template <bool kB>
__device__ void lb_emit(const WaveCore& c, WaveVec& dx, WaveVec& pen, double* pb, double* pp,
                        const LbArgs& A, int slot, int lane, [[maybe_unused]] int sidx) {
    const int i = lane & 15;
    const double xi = c.xe.v;                       // every row holds xe
    double h = kFdStep;
    if ((xi + h) - xi == 0.0) h = kSqrtEps * (xi >= 0.0 ? 1.0 : -1.0) * fmax(1.0, fabs(xi));
    const double xh = xi + h;
    dx.v = i < dhlb::kN ? xh - xi : 0.0;
    if (lane < 32 && i < dhlb::kN) {
        const double v = lb_transform(i, lane < 16 ? xi : xh);
        if (lane < 16) pb[i] = v;
        else pp[i] = v;
    }
    __syncthreads();
    pen.v = 0.0;
    if (lane < dhlb::kPts) {
        double p[dhlb::kN];
#pragma unroll
        for (int i = 0; i < dhlb::kN; ++i) p[i] = (i == lane - 1) ? pp[i] : pb[i];
        pen.v = feller_penalty(p);
        double* out = A.rec + ((size_t)slot * dhlb::kPts + lane) * DH_PARAM_STRIDE;
#pragma unroll
        for (int i = 0; i < dhlb::kN; ++i) out[i] = p[i];
        if constexpr (kB) {
            out[13] = A.spot_of[sidx];
            out[14] = A.rate_of[sidx];
            A.row[(size_t)slot * dhlb::kPts + lane] = A.market_of[sidx];
        } else {
            out[13] = A.S0;
            out[14] = A.r;
        }
        out[15] = 0.0;
    }
}

// The analytic-gradient driver's request (dh_calibrate_lbfgs_batch_grad, and dh_calibrate_lm_batch's):
// the one record of xe, no bumps and no dx.  Lane i < 13 maps x_i = xi to its model param and writes it; lanes 13..15 write the
// start's spot, its rate and q = 0; lane 0 writes the set's market row and the record's Feller
// penalty (feller_penalty, as the record kernels'), which the rows reduction adds to the loss.
__device__ void lb_emit_grad(double xi, WaveVec& dx, WaveVec& pen, double* pb, const LbArgs& A,
                             int slot, int lane, int sidx) {
    dx.v = 0.0;
    if (lane < dhlb::kN) pb[lane] = lb_transform(lane, xi);
    __syncthreads();
    pen.v = feller_penalty(pb);
    double* out = A.rec + (size_t)slot * DH_PARAM_STRIDE;
    if (lane < dhlb::kN) out[lane] = pb[lane];
    else if (lane == 13) out[13] = A.spot_of[sidx];
    else if (lane == 14) out[14] = A.rate_of[sidx];
    else if (lane == 15) out[15] = 0.0;
    if (lane == 0) {
        A.row[slot] = A.market_of[sidx];
        A.pen_out[slot] = pen.v;
    }
}

// The loss hand-off's sum of one param set's nt tile partials (task_loss: lane l adds tiles l,
// l + 64, ... in order, then an xor butterfly), formed by one lane: leaf l as that lane's sum,
// then the butterfly's tree (level w adds leaves w apart).  Leaves past nt are +0.0 and adding
// +0.0 to a partial (a sum of squares) changes no bit, so W = 16 or 32 leaves give the 64-leaf
// tree's bits.  Loads are clamped in-bounds and issued before any add.  A tile with an invalid
// price stored its partial with the sign bit set (task_loss), so the magnitudes give the sum --
// a NaN sum (a NaN or infinite market price) stays the NaN loss the reference gives -- and any
// sign bit gives 1e10 whatever the sum.
template <int W>
__device__ __forceinline__ void lb_tile_tree(const double* ps, int nt, double& sse, int& bad) {
    double x[W];
    unsigned hi = 0;        // OR of the high words: loads past nt repeat tile nt - 1 (clamped), so
                            // the OR over all of them is the OR of the first nt sign bits (a
                            // short-circuit || compiled to an exec-mask branch per tile)
#pragma unroll
    for (int u = 0; u < W; ++u) {
        const double v = ps[min(u, nt - 1)];
        x[u] = 0.0 + (u < nt ? fabs(v) : 0.0);
        hi |= (unsigned)__double2hiint(v);
    }
    for (int j0 = W; j0 < nt; j0 += W) {          // W = 64 only
#pragma unroll
        for (int u = 0; u < W; ++u) {
            const double v = ps[min(j0 + u, nt - 1)];
            x[u] += j0 + u < nt ? fabs(v) : 0.0;
            hi |= (unsigned)__double2hiint(v);
        }
    }
#pragma unroll
    for (int w = 1; w < W; w <<= 1) {
#pragma unroll
        for (int u = 0; u < W; u += 2 * w) x[u] = x[u] + x[u + w];
    }
    sse = x[0];
    bad = (int)(hi >> 31);
}

// One wave per live start: load the state (vectors into registers, lane i = component i; the
// pair memory into LDS), consume the finished request (lane t forms loss t, lane i gradient
// component i), run the L-BFGS-B state machine until it needs a new point, emit that request,
// store the state.  kB: dh_calibrate_lbfgs_batch's build -- the emitted records carry the start's
// own spot and rate (lb_emit<true>) and the trace's first spare double the start's market; the
// two kB = false builds are dh_calibrate_lbfgs's, unchanged.  kIv (with kB):
// dh_calibrate_lbfgs_batch_iv's builds -- the request's sse is dh_loss_rows.h's vol reduction and
// the loss divides it by the start's weight sum (div_of) where the price objective divides by M.
// kG (with kB): dh_calibrate_lbfgs_batch_grad's builds -- the request is one point, its loss (sse)
// and gradient (grad) come finished from dh_param_grad.h's rows reduction, and the next request
// is the one record of lb_emit_grad.  dh_calibrate_lbfgs_batch_iv_grad runs the kG builds as they
// are: dh_iv_grad.h's reduction hands them a finished f and g as dh_param_grad.h's does.
template <bool kPre, bool kB = false, bool kIv = false, bool kG = false>
__global__ __launch_bounds__(64) void lb_step_kernel(
    LbSlot* __restrict__ h_states, const double* __restrict__ h_part, int h_ntiles, int h_mode,
    int h_part_mode, int h_l0, int h_l1, int h_l2, int h_l3, LbArgs A_) {
    const LbArgs& A = karg_ref<LbArgs, kLbArgsKernargOff>();   // read in place (karg_ref)
    karg_prefetch_lines();                             // LbArgs spans the same lines
    __shared__ double ring[kLbRing + dhlb::kM];
    __shared__ double fl[dhlb::kLanes];
    __shared__ double pb[dhlb::kLanes], pp[dhlb::kLanes];
    [[maybe_unused]] const unsigned long long t_start = lb_clock();
    const int slot = blockIdx.x;
    const int lane = threadIdx.x;
    int sidx;
    if constexpr (kPre)                                // slot < kLbPre (the host's choice)
        sidx = slot == 0 ? h_l0 : (slot == 1 ? h_l1 : (slot == 2 ? h_l2 : h_l3));
    else
        sidx = A.n_inline ? lb_live_inline(slot) : A.live[slot];
    LbSlot* G = h_states + sidx;
    WaveCore c;
    [[maybe_unused]] unsigned long long t_load = 0, t_req = 0, t_sm = 0;
    c.pairs = WaveRing{ring, ring + dhlb::kM * dhlb::kLanes, ring + 2 * dhlb::kM * dhlb::kLanes,
                       ring + kLbRing, lane};
    WaveVec dx, pen;
    double req_sse = 0.0;
    int req_bad = 0;
    [[maybe_unused]] double req_g = 0.0;
    if (h_mode == 0) {
        c.s = dhlb::LbScalars{};
        const WaveVec z{0.0};
        c.x = c.g = c.z = c.d = c.t = c.r = c.ge = z;
        for (int i = lane; i < kLbRing + dhlb::kM; i += 64) ring[i] = 0.0;
        const int li = lane & 15;
        const WaveVec x0{li < dhlb::kN ? A.x0[(size_t)sidx * dhlb::kN + li] : 0.0};
        dhlb::lb_begin(c, x0);
        c.s.best_loss = __builtin_huge_val();
        c.s.n_calls = 0;
    } else {
        // every load is issued before any is used (one memory round trip): the finished request's
        // loss terms, the pair memory, the vectors and the scalars
        if constexpr (kG) {
            if (h_mode == 1) {
                req_sse = A.sse[slot];
                req_g = (lane & 15) < dhlb::kN ? A.grad[(size_t)slot * dhlb::kN + (lane & 15)] : 0.0;
            }
        } else if (h_mode == 1 && h_part_mode) {
            // the loss hand-off's sum (task_loss), formed by lane t of every row for point t
            // (lb_tile_tree: the same additions, so the same bits).  Measured alternatives, all
            // slower: staging the request's contiguous partials through LDS with coalesced loads
            // (C2 step load phase 4.4k -> 5.5k cycles); issuing these loads together with the
            // state's (5.6k)
            const int li = lane & 15;
            if (li < dhlb::kPts) {
                const int nt = h_ntiles;
                const double* ps = h_part + ((size_t)slot * dhlb::kPts + li) * nt;
                if (nt <= 16) lb_tile_tree<16>(ps, nt, req_sse, req_bad);
                else if (nt <= 32) lb_tile_tree<32>(ps, nt, req_sse, req_bad);
                else lb_tile_tree<64>(ps, nt, req_sse, req_bad);
            }
        } else if (h_mode == 1 && (lane & 15) < dhlb::kPts) {
            const size_t i = (size_t)slot * dhlb::kPts + (lane & 15);
            req_sse = A.sse[i];
            req_bad = A.bad[i];
        }
        double rg[(kLbRing + 63) / 64];
#pragma unroll
        for (int j = 0; j < (kLbRing + 63) / 64; ++j) {
            const int i = lane + 64 * j;
            rg[j] = i < kLbRing ? G->ring[i] : 0.0;
        }
        c.s = G->s;
#pragma unroll
        for (int j = 0; j < (kLbRing + 63) / 64; ++j) {
            const int i = lane + 64 * j;
            if (i < kLbRing) ring[i] = rg[j];
        }
        c.x = lb_ld(G, 0, lane);
        c.g = lb_ld(G, 1, lane);
        c.z = lb_ld(G, 2, lane);
        c.d = lb_ld(G, 3, lane);
        c.t = lb_ld(G, 4, lane);
        c.r = lb_ld(G, 5, lane);
        c.xe = lb_ld(G, 6, lane);
        c.ge = lb_ld(G, 7, lane);
        dx = lb_ld(G, 8, lane);
        pen = lb_ld(G, 9, lane);
        if (c.s.done) return;                          // uniform across the wave
    }
    int need = 1;
    double* tr = nullptr;                              // this request's trace record, if any
    if (h_mode == 1) {
        t_load = lb_clock();
        double f = __builtin_huge_val();
        if constexpr (kG) {
            // the reduction's loss: Feller included, 1e10 (and a zero gradient) at an invalid price
            f = req_sse;
            c.s.n_calls += 1;
            if (f == f && f != kInvalidLoss && f < c.s.best_loss) c.s.best_loss = f;
            c.s.fe = f;
            c.ge.v = req_g;
        } else if constexpr (kIv) {
            if ((lane & 15) < dhlb::kPts)
                f = req_bad > 0 ? kInvalidLoss : req_sse / A.div_of[sidx] + pen.v;
        } else {
            if ((lane & 15) < dhlb::kPts) f = req_bad > 0 ? kInvalidLoss : req_sse / (double)A.M + pen.v;
        }
        if constexpr (!kG) {
            if (lane < dhlb::kLanes) fl[lane] = f;
            __syncthreads();
            const double lo = row_min((f == f && f != kInvalidLoss) ? f : __builtin_huge_val());
            c.s.n_calls += dhlb::kPts;
            if (lo < c.s.best_loss) c.s.best_loss = lo;
            c.s.fe = fl[0];
            c.ge.v = (lane & 15) < dhlb::kN ? (fl[(lane & 15) + 1] - fl[0]) / dx.v : 0.0;
        }
        if (A.trace) {
            unsigned long long k = 0;
            if (lane == 0) k = atomicAdd(A.trace_n, 1ull);
            k = __shfl(k, 0, 64);
            if ((int64_t)k < A.trace_cap) {
                tr = A.trace + k * kLbTrace;
                if (lane == 0) {
                    tr[0] = sidx;
                    tr[1] = c.s.n_calls / (kG ? 1 : dhlb::kPts) - 1;
                    tr[2] = c.s.fe;
                    if constexpr (kB) tr[3 + 2 * dhlb::kN] = A.market_of[sidx];
                }
                if (lane < dhlb::kN) {
                    tr[3 + lane] = c.xe.v;
                    tr[3 + dhlb::kN + lane] = c.ge.v;
                }
            }
        }
    }
    __syncthreads();
    if (h_mode == 1) {
        t_req = lb_clock();
        need = dhlb::lb_resume(c, A.cfg);
        t_sm = lb_clock();
        if (!need && lane == 0) {
            __hip_atomic_store(&A.done[sidx], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            atomicSub(A.live_count, 1);
        }
    }
    if constexpr (kG) {
        if (need) lb_emit_grad(c.xe.v, dx, pen, pb, A, slot, lane, sidx);
    } else {
        if (need) lb_emit<kB>(c, dx, pen, pb, pp, A, slot, lane, sidx);
    }
    __syncthreads();
    [[maybe_unused]] const unsigned long long t_emit = lb_clock();
    {   // every LDS read before the first store (one LDS round trip, not one per store)
        double rg[(kLbRing + 63) / 64];
#pragma unroll
        for (int j = 0; j < (kLbRing + 63) / 64; ++j) rg[j] = ring[min(lane + 64 * j, kLbRing - 1)];
#pragma unroll
        for (int j = 0; j < (kLbRing + 63) / 64; ++j)
            if (lane + 64 * j < kLbRing) G->ring[lane + 64 * j] = rg[j];
    }
    lb_st(G, 0, lane, c.x);
    lb_st(G, 1, lane, c.g);
    lb_st(G, 2, lane, c.z);
    lb_st(G, 3, lane, c.d);
    lb_st(G, 4, lane, c.t);
    lb_st(G, 5, lane, c.r);
    lb_st(G, 6, lane, c.xe);
    lb_st(G, 7, lane, c.ge);
    lb_st(G, 8, lane, dx);
    lb_st(G, 9, lane, pen);
    if (lane == 0) G->s = c.s;
#ifdef DH_STAMPS
    if (tr && lane == 0) {
        const unsigned long long t_end = lb_clock();
        const unsigned long long ts[6] = {t_start, t_load, t_req, t_sm, t_emit, t_end};
        for (int i = 0; i < 6; ++i) tr[kLbStamp0 + i] = (double)ts[i];
    }
#endif
}

// One objective's step launch: the kPre build where the (inline) live list fits the leading
// arguments, the in-argument / in-memory list's build otherwise.
template <bool kB, bool kIv, bool kG = false>
int launch_lb_step_as(hipStream_t st, const LbArgs& A, int n_live) {
    static_assert(kB || !(kIv || kG), "the vol objective and the analytic gradient are the batch "
                                      "driver's only");
    const bool pre = A.n_inline && n_live <= kLbPre;
    int l[kLbPre] = {0, 0, 0, 0};
    for (int i = 0; pre && i < n_live; ++i) l[i] = A.live_inline[i];
    const auto step =
        pre ? lb_step_kernel<true, kB, kIv, kG> : lb_step_kernel<false, kB, kIv, kG>;
    hipLaunchKernelGGL(step, dim3((unsigned)n_live), dim3(64), 0, st, A.states, A.part_sse,
                       A.n_tiles, A.mode, A.part_mode, l[0], l[1], l[2], l[3], A);
    HIP_TRY(hipGetLastError());
    return DH_OK;
}

int launch_lb_step(hipStream_t st, const LbArgs& A, int n_live, bool batch = false,
                   bool iv = false, bool grad = false) {
    if (batch && grad) return launch_lb_step_as<true, false, true>(st, A, n_live);
    if (batch && iv) return launch_lb_step_as<true, true>(st, A, n_live);
    if (batch) return launch_lb_step_as<true, false>(st, A, n_live);
    return launch_lb_step_as<false, false>(st, A, n_live);
}


// ---- Levenberg-Marquardt (dh_calibrate_lm_batch; dh_lm.h) -------------------------
// Global state of one start: the LmCore as it is (all doubles, then the scalars).
using LmSlot = dhlm::LmCore;
static_assert(sizeof(LmSlot) % 8 == 0 && std::is_trivially_copyable<LmSlot>::value,
              "lm_step_kernel copies the state as 8-byte words");
constexpr int kLmWords = (int)(sizeof(LmSlot) / 8);

// One wave per live start, as lb_step_kernel's kG build: stage the state in LDS (coalesced), consume
// the finished request -- f (A.sse), g (A.grad) and the Gauss-Newton Hessian (hess) of the slot,
// from dh_gauss_newton.h's reduction -- run the state machine in lane 0 (plain scalar code, the CPU
// build's: tests/native/lm_host.cpp), emit the next record with lb_emit_grad (the same transform,
// penalty, spot, rate and row as the analytic L-BFGS-B driver's), store the state.  The live list
// is read from memory (the host uploads it at every compaction).  The trace rows are lb_step_kernel's.
__global__ __launch_bounds__(64) void lm_step_kernel(LbArgs A, LmSlot* __restrict__ states,
                                                     const double* __restrict__ hess) {
    __shared__ LmSlot c;
    __shared__ double pb[dhlb::kLanes];
    __shared__ int need_s;
    const int slot = blockIdx.x;
    const int lane = threadIdx.x;
    const int sidx = A.live[slot];
    unsigned long long* const G = (unsigned long long*)(states + sidx);
    unsigned long long* const cw = (unsigned long long*)&c;
    if (A.mode == 0) {
        if (lane == 0) dhlm::lm_begin(c, A.x0 + (size_t)sidx * dhlm::kN);
    } else {
        for (int i = lane; i < kLmWords; i += 64) cw[i] = G[i];
    }
    __syncthreads();
    if (A.mode != 0 && c.s.done) return;               // uniform across the wave
    int need = 1;
    if (A.mode == 1) {
        const double f = A.sse[slot];
        const double* ge = A.grad + (size_t)slot * dhlm::kN;
        if (A.trace) {
            unsigned long long k = 0;
            if (lane == 0) k = atomicAdd(A.trace_n, 1ull);
            k = __shfl(k, 0, 64);
            if ((int64_t)k < A.trace_cap) {
                double* tr = A.trace + k * kLbTrace;
                if (lane == 0) {
                    tr[0] = sidx;
                    tr[1] = c.s.n_calls;
                    tr[2] = f;
                    tr[3 + 2 * dhlm::kN] = A.market_of[sidx];
                }
                if (lane < dhlm::kN) {
                    tr[3 + lane] = c.xe[lane];
                    tr[3 + dhlm::kN + lane] = ge[lane];
                }
            }
        }
        if (lane == 0) {
            const dhlm::LmConfig cf{A.cfg.maxiter, A.cfg.maxfun, A.cfg.factr_epsmch, A.cfg.pgtol};
            need_s = dhlm::lm_resume(c, cf, f, ge, hess + (size_t)slot * (dhlm::kN * dhlm::kN));
            if (!need_s) {
                __hip_atomic_store(&A.done[sidx], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                atomicSub(A.live_count, 1);
            }
        }
        __syncthreads();
        need = need_s;
    }
    if (need) {
        WaveVec dx, pen;
        lb_emit_grad(lane < dhlm::kN ? c.xe[lane] : 0.0, dx, pen, pb, A, slot, lane, sidx);
    }
    __syncthreads();
    for (int i = lane; i < kLmWords; i += 64) G[i] = cw[i];
}

int launch_lm_step(hipStream_t st, const LbArgs& A, int n_live, LmSlot* states, const double* hess) {
    hipLaunchKernelGGL(lm_step_kernel, dim3((unsigned)n_live), dim3(64), 0, st, A, states, hess);
    HIP_TRY(hipGetLastError());
    return DH_OK;
}

// the markets of dh_calibrate_lbfgs_batch (host arrays): mkt [B][M], spot [B], rate [B] and the
// market of each start
struct LbBatch {
    const double* mkt;
    const double* spot;
    const double* rate;
    int B;
    const int32_t* market_of;
    // dh_calibrate_lbfgs_batch_iv: mkt holds the market vols; the weight rows [B][M] and each
    // market's weight sum [B] (null: the price objective)
    const double* iv_wgt = nullptr;
    const double* iv_wsum = nullptr;
    // dh_calibrate_lbfgs_batch_grad: one analytic loss + gradient request per iteration; with
    // the weights, dh_calibrate_lbfgs_batch_iv_grad: the vol objective's (dh_iv_grad.h)
    bool grad = false;
    // dh_calibrate_lm_batch (with grad): the same request through dh_gauss_newton.h's reduction,
    // which adds the Gauss-Newton Hessian, and lm_step_kernel in place of lb_step_kernel
    bool lm = false;
};

}  // namespace

// dh_calibrate_lbfgs (bt null: one market, the surface's, through the fused loss launches) and
// dh_calibrate_lbfgs_batch (bt: a market per start, through price + dh_loss_rows.h's reduction)
// and dh_calibrate_lbfgs_batch_iv (bt with weights: through price + dh_loss_rows.h's vol one)
// and dh_calibrate_lbfgs_batch_grad (bt with grad: one record per start through dh_param_grad.h's
// planes and rows reduction) and dh_calibrate_lbfgs_batch_iv_grad (bt with weights and grad: the
// same planes through dh_iv_grad.h's reduction)
static int lb_run(dh_ctx* ctx, const dh_surface* s, const double* x0, int S, double S0, double r,
                  int N, double L, const dh_lb_options* opt, dh_lb_result* out,
                  int32_t* n_launches, const LbBatch* bt) {
    if (!ctx || !s || !opt || (S > 0 && (!x0 || !out))) return fail(DH_E_ARG, "null argument");
    if (!bt && !s->has_mkt) return fail(DH_E_ARG, "surface has no market prices");
    if (s->M == 0) return fail(DH_E_ARG, "empty market (the loss is NaN; no optimisation)");
    int rc = check_N(N);
    if (rc) return rc;
    const bool grad = bt && bt->grad;
    const bool lm = grad && bt->lm;
    if (grad && N > DH_PARAM_GRAD_MAX_N)
        return fail(DH_E_ARG, "N must be in [1, " + std::to_string(DH_PARAM_GRAD_MAX_N) +
                                  "] under the analytic gradient, got " + std::to_string(N));
    if (grad && (!std::isfinite(L) || !(L > 0.0)))
        return fail(DH_E_ARG, "L must be finite and > 0");
    if (S < 0) return fail(DH_E_ARG, "S < 0");
    if (opt->maxiter < 0 || opt->maxfun < 0 || opt->maxls < 1)   // SciPy: maxls must be > 0
        return fail(DH_E_ARG, "maxiter and maxfun must be >= 0, maxls >= 1");
    if (n_launches) *n_launches = 0;
    if (bt) {
        if (S > 0 && bt->B <= 0) return fail(DH_E_ARG, "B <= 0");
        if (bt->B > 0 && (!bt->mkt || !bt->spot || !bt->rate))
            return fail(DH_E_ARG, "null argument");
        if (S > 0 && !bt->market_of) return fail(DH_E_ARG, "null argument");
        rc = check_spot_rate(bt->spot, bt->rate, bt->B);
        if (rc) return rc;
        for (int i = 0; i < S; ++i)
            if (bt->market_of[i] < 0 || bt->market_of[i] >= bt->B)
                return fail(DH_E_ARG, "market_of " + std::to_string(i) + " is outside [0, B)");
    }
    if (S == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t st = ctx->stream;
    const size_t npts = (size_t)S * dhlb::kPts;
    const size_t slot_bytes = lm ? sizeof(LmSlot) : sizeof(LbSlot);
    HIP_TRY(ctx->lb_state.reserve((size_t)S * slot_bytes));
    HIP_TRY(ctx->lb_rec.reserve(npts * DH_PARAM_STRIDE * 8));
    HIP_TRY(ctx->lb_sse.reserve(npts * 8));
    HIP_TRY(ctx->lb_bad.reserve(npts * 4));
    HIP_TRY(ctx->lb_live.reserve((size_t)S * 4));
    HIP_TRY(ctx->lb_done.reserve(4));                  // live-start count (halts launches at 0)
    HIP_TRY(ctx->lb_x0.reserve((size_t)S * dhlb::kN * 8));
    // pinned, device-mapped: finished flags (written by the step kernel) | 2 live-list buffers
    HIP_TRY(ctx->h_lb.reserve((size_t)S * 3 * 4));
    int* h_done = (int*)ctx->h_lb.ptr;
    int* h_live[2] = {h_done + S, h_done + 2 * S};
    std::memset(h_done, 0, (size_t)S * 4);
    std::vector<int> live(S);
    for (int i = 0; i < S; ++i) live[i] = h_live[0][i] = i;
    HIP_TRY(hipMemcpyAsync(ctx->lb_x0.ptr, x0, (size_t)S * dhlb::kN * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->lb_live.ptr, h_live[0], (size_t)S * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)ctx->lb_done.ptr, S, 1, st));
    const int M = s->M;
    if (bt) {
        // each start's spot and rate gathered on the host: one load per emitted record
        const size_t mb = (size_t)bt->B * M * 8;
        HIP_TRY(ctx->rows_mkt.reserve(mb));
        HIP_TRY(ctx->rows_row.reserve(npts * 4));
        if (grad)   // once, for all S starts: a rows request's scratch, with the vol objective's
                    // c_m plane or Levenberg-Marquardt's Hessians after the planes
            HIP_TRY(ctx->pg_scratch.reserve(dhpg::grad_scratch_bytes(
                S, M,
                bt->iv_wgt ? dhpg::Scratch::kVol
                           : (lm ? dhpg::Scratch::kHess : dhpg::Scratch::kPrice))));
        else
            HIP_TRY(ctx->lb_prices.reserve(npts * M * 8));
        HIP_TRY(ctx->lb_spot.reserve((size_t)S * 8));
        HIP_TRY(ctx->lb_rate.reserve((size_t)S * 8));
        HIP_TRY(ctx->lb_mof.reserve((size_t)S * 4));
        std::vector<double> sr((size_t)2 * S);
        for (int i = 0; i < S; ++i) {
            sr[i] = bt->spot[bt->market_of[i]];
            sr[(size_t)S + i] = bt->rate[bt->market_of[i]];
        }
        HIP_TRY(hipMemcpyAsync(ctx->rows_mkt.ptr, bt->mkt, mb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->lb_spot.ptr, sr.data(), (size_t)S * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->lb_rate.ptr, sr.data() + S, (size_t)S * 8,
                               hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->lb_mof.ptr, bt->market_of, (size_t)S * 4, hipMemcpyHostToDevice,
                               st));
        std::vector<double> dv;
        if (bt->iv_wgt) {                             // each start's weight sum, gathered as well
            HIP_TRY(ctx->rows_wgt.reserve(mb));
            HIP_TRY(ctx->lb_div.reserve((size_t)S * 8));
            dv.resize(S);
            for (int i = 0; i < S; ++i) dv[i] = bt->iv_wsum[bt->market_of[i]];
            HIP_TRY(hipMemcpyAsync(ctx->rows_wgt.ptr, bt->iv_wgt, mb, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ctx->lb_div.ptr, dv.data(), (size_t)S * 8,
                                   hipMemcpyHostToDevice, st));
            if (grad) {
                // dh_iv_grad.h's reduction works per slot, and a start changes slot at a
                // compaction: it reads the divisor at the set's market row, so the sums go up
                // per market as well
                HIP_TRY(ctx->lb_wsum.reserve((size_t)bt->B * 8));
                HIP_TRY(hipMemcpyAsync(ctx->lb_wsum.ptr, bt->iv_wsum, (size_t)bt->B * 8,
                                       hipMemcpyHostToDevice, st));
            }
        }
        HIP_TRY(hipStreamSynchronize(st));            // `sr`, `dv` are pageable and leave scope
    }
    if (!ctx->lb_ev[0]) {
        for (hipEvent_t& e : ctx->lb_ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }

    LbArgs A;
    A.states = (LbSlot*)ctx->lb_state.ptr;
    A.live = (const int*)ctx->lb_live.ptr;
    A.x0 = (const double*)ctx->lb_x0.ptr;
    A.sse = (const double*)ctx->lb_sse.ptr;
    A.bad = (const int*)ctx->lb_bad.ptr;
    A.rec = (double*)ctx->lb_rec.ptr;
    A.done = (int*)ctx->h_lb.dptr;
    A.live_count = (int*)ctx->lb_done.ptr;
    A.trace = nullptr;
    A.trace_n = nullptr;
    A.trace_cap = 0;
    if (ctx->lb_trace_cap > 0) {
        HIP_TRY(ctx->lb_trace.reserve((size_t)ctx->lb_trace_cap * kLbTrace * 8));
        HIP_TRY(ctx->lb_trace_n.reserve(8));
        HIP_TRY(hipMemsetAsync(ctx->lb_trace_n.ptr, 0, 8, st));
        A.trace = (double*)ctx->lb_trace.ptr;
        A.trace_n = (unsigned long long*)ctx->lb_trace_n.ptr;
        A.trace_cap = ctx->lb_trace_cap;
    }
    A.cfg.maxiter = opt->maxiter;
    A.cfg.maxfun = opt->maxfun;
    A.cfg.maxls = opt->maxls;
    A.cfg.pad = 0;
    A.cfg.factr_epsmch = (opt->ftol / dhlb::kEpsMch) * dhlb::kEpsMch;   // factr * epsmch
    A.cfg.pgtol = opt->gtol;
    A.S0 = S0;
    A.r = r;
    A.M = s->M;
    A.mode = 0;
    A.part_mode = 0;
    A.part_sse = nullptr;
    A.n_tiles = s->n_tiles;
    A.spot_of = bt ? (const double*)ctx->lb_spot.ptr : nullptr;
    A.rate_of = bt ? (const double*)ctx->lb_rate.ptr : nullptr;
    A.market_of = bt ? (const int*)ctx->lb_mof.ptr : nullptr;
    A.row = bt ? (int*)ctx->rows_row.ptr : nullptr;
    const bool batch = bt != nullptr;
    const bool iv = batch && bt->iv_wgt != nullptr;
    A.div_of = iv ? (const double*)ctx->lb_div.ptr : nullptr;
    // The analytic request of an iteration, over all S starts' scratch: the one-shot calls' carve
    // with the gradients [S][16] where they keep their records (the driver's records are lb_rec,
    // one per live start).  The step kernel writes the records, rows and penalties and reads f
    // (sse) and g (grad) finished; under the vol objective rows_mkt holds vols.
    dhpg::GradRows R{};
    dhpg::GradScratch c{};
    dhpg::RowsLaunch rows_launch = nullptr;
    if (grad) {
        c = dhpg::carve_grad_scratch(ctx->pg_scratch.ptr, S, M);
        R.rec = A.rec, R.pen = c.pen, R.planes = c.planes, R.extra = c.extra;
        R.mkt = (const double*)ctx->rows_mkt.ptr;
        R.wgt = iv ? (const double*)ctx->rows_wgt.ptr : nullptr;
        R.row = A.row;
        R.div = iv ? (const double*)ctx->lb_wsum.ptr : nullptr;
        R.div_by_row = true;
        R.f = (double*)A.sse;
        R.g = c.rec;
        R.bad = (int*)A.bad;
        R.live_count = A.live_count;
        rows_launch = lm   ? dhgn::gauss_newton_rows_launch
                      : iv ? dhivg::loss_iv_grad_rows_launch
                           : dhpg::loss_grad_rows_launch;
    }
    A.grad = c.rec;
    A.pen_out = c.pen;
    double* const d_hess = lm ? R.extra : nullptr;
    auto set_inline = [&](const int* lst, int n) {
        A.n_inline = !lm && n <= kLbInline ? 1 : 0;   // lm_step_kernel reads the list from memory
        for (int i = 0; i < kLbInline; ++i) A.live_inline[i] = i < n && A.n_inline ? lst[i] : 0;
    };
    // the seam between the two optimisers: which step kernel advances the live starts
    auto launch_step = [&](int n) -> int {
        return lm ? launch_lm_step(st, A, n, (LmSlot*)ctx->lb_state.ptr, d_hess)
                  : launch_lb_step(st, A, n, batch, iv, grad);
    };
    set_inline(h_live[0], S);
    rc = launch_step(S);
    if (rc) return rc;

    // Chunks of `chunk` iterations (loss launch(es) + step launch) are enqueued two ahead of the
    // host: while the GPU runs chunk k + 1, the host reads the finished flags as of the end of
    // chunk k, compacts the live starts (their requests are re-emitted at the new slots, in
    // stream order after chunk k + 1) and enqueues chunk k + 2.  Launches enqueued after the
    // last start finished return at once (live count 0).
    DrainOnError drain{st};    // an early error return leaves no launch writing our buffers
    const int chunk = opt->chunk > 0 ? opt->chunk : 8;
    const int64_t max_iters = (int64_t)opt->maxfun + 2LL * opt->maxls + 8;   // nfev bound per start
    std::vector<double> t_done(S, 0.0);
    int n_live = S;
    int64_t iters = 0, launches = 0;
    auto enqueue_chunk = [&](int k) -> int {
        A.mode = 1;
        R.S = n_live;
        for (int c = 0; c < chunk; ++c) {
            int e;
            if (grad) {
                // the planes of the live starts' records, then each set's loss and gradient
                // against its start's market row; the step reads them finished
                e = rows_launch(ctx, s, R, N, L, st);
                if (e) return e;
                e = launch_step(n_live);
                if (e) return e;
                ++launches;
                continue;
            }
            if (batch) {
                // prices of the 14 x live records, then each set against its start's market row
                // (the rows the step kernel wrote beside the records)
                e = surface_price_launch_lb(ctx, s, A.rec, (int64_t)n_live * dhlb::kPts, N, L,
                                            (double*)ctx->lb_prices.ptr, st, A.live_count);
                if (e) return e;
                if (iv)                                // the vol-space reduction: rows_mkt holds vols
                    e = iv_rows_launch(ctx, s, A.rec, (const double*)ctx->lb_prices.ptr,
                                       (const double*)ctx->rows_mkt.ptr,
                                       (const double*)ctx->rows_wgt.ptr, (const int32_t*)A.row,
                                       n_live * dhlb::kPts, (double*)A.sse, (int32_t*)A.bad,
                                       nullptr, st, A.live_count);
                else
                    e = loss_rows_launch(ctx, s, (const double*)ctx->lb_prices.ptr,
                                         (const double*)ctx->rows_mkt.ptr, (const int32_t*)A.row,
                                         n_live * dhlb::kPts, (double*)A.sse, (int32_t*)A.bad, st,
                                         A.live_count);
                if (e) return e;
                e = launch_lb_step(st, A, n_live, true, iv);   // part_mode 0: reads sse / bad
                if (e) return e;
                ++launches;
                continue;
            }
            e = surface_loss_launch(ctx, s, A.rec, n_live * dhlb::kPts, N, L, (double*)A.sse,
                                    (int32_t*)A.bad, nullptr, st, A.live_count, true);
            if (e) return e;
            // a fused request stored its tile partials only (no hand-off): the step sums them
            A.part_mode = !per_term(ctx, N) && ctx->last_path == DH_PATH_FUSED ? 1 : 0;
            A.part_sse = (const double*)ctx->part_sse.ptr;
            e = launch_lb_step(st, A, n_live);
            if (e) return e;
            ++launches;
        }
        iters += chunk;
        HIP_TRY(hipEventRecord(ctx->lb_ev[k & 1], st));
        return DH_OK;
    };
    rc = enqueue_chunk(0);
    if (rc) return rc;
    rc = enqueue_chunk(1);
    if (rc) return rc;
    for (int k = 0;; ++k) {
        for (;;) {                                     // spin: a chunk is ~0.1-1 ms
            const hipError_t e = hipEventQuery(ctx->lb_ev[k & 1]);
            if (e == hipSuccess) break;
            if (e != hipErrorNotReady)
                return fail(DH_E_HIP, std::string("hipEventQuery: ") + hipGetErrorString(e));
        }
        const double now =
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::vector<int> next;
        next.reserve(live.size());
        for (int sidx : live) {
            if (__atomic_load_n(&h_done[sidx], __ATOMIC_ACQUIRE)) {
                if (t_done[sidx] == 0.0) t_done[sidx] = now;
            } else {
                next.push_back(sidx);
            }
        }
        if (next.empty()) break;
        if (iters > max_iters) {
            (void)hipStreamSynchronize(st);
            return fail(DH_E_ARG, "L-BFGS-B starts did not terminate");
        }
        if (next.size() != live.size()) {              // compact; re-emit their requests
            live.swap(next);
            n_live = (int)live.size();
            set_inline(live.data(), n_live);
            if (!A.n_inline) {
                int* hl = h_live[(k + 1) & 1];         // the other buffer's upload has run
                std::memcpy(hl, live.data(), (size_t)n_live * 4);
                HIP_TRY(hipMemcpyAsync(ctx->lb_live.ptr, hl, (size_t)n_live * 4,
                                       hipMemcpyHostToDevice, st));
            }
            A.mode = 2;
            rc = launch_step(n_live);
            if (rc) return rc;
        }
        rc = enqueue_chunk(k + 2);
        if (rc) return rc;
    }
    std::vector<unsigned char> hbytes((size_t)S * slot_bytes);
    HIP_TRY(hipMemcpyAsync(hbytes.data(), ctx->lb_state.ptr, hbytes.size(), hipMemcpyDeviceToHost,
                           st));
    HIP_TRY(hipStreamSynchronize(st));
    drain.armed = false;
    if (n_launches) *n_launches = (int32_t)launches;
    if (lm) {
        const LmSlot* hl = (const LmSlot*)hbytes.data();
        for (int i = 0; i < S; ++i) {
            const dhlm::LmScalars& q = hl[i].s;
            dh_lb_result& o = out[i];
            for (int j = 0; j < dhlm::kN; ++j) o.x[j] = hl[i].x[j];
            o.fun = q.f;
            o.best_loss = q.best_loss;
            o.t_done = t_done[i];
            o.nit = q.nit;
            o.nfev = q.nfev;
            o.task = q.task;
            o.warnflag = q.warnflag;
            o.n_calls = q.n_calls;
            o.pad = 0;
        }
        return DH_OK;
    }
    const LbSlot* hs = (const LbSlot*)hbytes.data();
    for (int i = 0; i < S; ++i) {
        const LbSlot& q = hs[i];
        dh_lb_result& o = out[i];
        for (int j = 0; j < dhlb::kN; ++j) o.x[j] = q.vec[0][j];   // row 0 = x
        o.fun = q.s.fe;
        o.best_loss = q.s.best_loss;
        o.t_done = t_done[i];
        o.nit = q.s.nit;
        o.nfev = q.s.nfev;
        o.task = q.s.task;
        o.warnflag = q.s.warnflag;
        o.n_calls = q.s.n_calls;
        o.pad = 0;
    }
    return DH_OK;
}

extern "C" int dh_calibrate_lbfgs(dh_ctx* ctx, const dh_surface* s, const double* x0, int S,
                                  double S0, double r, int N, double L, const dh_lb_options* opt,
                                  dh_lb_result* out, int32_t* n_launches) {
    return lb_run(ctx, s, x0, S, S0, r, N, L, opt, out, n_launches, nullptr);
}

extern "C" int dh_calibrate_lbfgs_batch(dh_ctx* ctx, const dh_surface* s, const double* mkt,
                                        const double* spot, const double* rate, int B,
                                        const double* x0, const int32_t* market_of, int S, int N,
                                        double L, const dh_lb_options* opt, dh_lb_result* out,
                                        int32_t* n_launches) {
    const LbBatch bt{mkt, spot, rate, B, market_of};
    return lb_run(ctx, s, x0, S, 0.0, 0.0, N, L, opt, out, n_launches, &bt);
}

// The vol objective's loss is sse / sum_m w[b][m] + Feller (loss_batch's): each market's weight
// sum is formed on the host (iv_check_weights: option order, sequential, from 0.0) and gathered
// per start as spot and rate are; the step kernel's kIv builds divide by it.
extern "C" int dh_calibrate_lbfgs_batch_iv(dh_ctx* ctx, const dh_surface* s, const double* mkt_iv,
                                           const double* wgt, const double* spot,
                                           const double* rate, int B, const double* x0,
                                           const int32_t* market_of, int S, int N, double L,
                                           const dh_lb_options* opt, dh_lb_result* out,
                                           int32_t* n_launches) {
    if (!ctx || !s || !opt || (S > 0 && (!x0 || !out)) || (B > 0 && !mkt_iv))
        return fail(DH_E_ARG, "null argument");
    // the weights as the reduction reads them ([B][M], null: all 1) and each market's weight sum
    std::vector<double> w((size_t)std::max(B, 0) * s->M), wsum((size_t)std::max(B, 0), 0.0);
    const int rc = iv_check_weights(mkt_iv, wgt, B, s->M, true, w.data(), wsum.data());
    if (rc) return rc;
    LbBatch bt{mkt_iv, spot, rate, B, market_of};
    bt.iv_wgt = w.data();
    bt.iv_wsum = wsum.data();
    return lb_run(ctx, s, x0, S, 0.0, 0.0, N, L, opt, out, n_launches, &bt);
}

// The price objective with its analytic gradient: one request per start and iteration
// (dh_param_grad.h's planes and rows reduction) where dh_calibrate_lbfgs_batch prices fourteen.
extern "C" int dh_calibrate_lbfgs_batch_grad(dh_ctx* ctx, const dh_surface* s, const double* mkt,
                                             const double* spot, const double* rate, int B,
                                             const double* x0, const int32_t* market_of, int S,
                                             int N, double L, const dh_lb_options* opt,
                                             dh_lb_result* out, int32_t* n_launches) {
    LbBatch bt{mkt, spot, rate, B, market_of};
    bt.grad = true;
    return lb_run(ctx, s, x0, S, 0.0, 0.0, N, L, opt, out, n_launches, &bt);
}

// The vol objective with its exact gradient: dh_calibrate_lbfgs_batch_iv's arguments and checks,
// dh_calibrate_lbfgs_batch_grad's iteration with dh_iv_grad.h's reduction in place of the price
// one.  The step kernel's kG builds run unchanged.
extern "C" int dh_calibrate_lbfgs_batch_iv_grad(dh_ctx* ctx, const dh_surface* s,
                                                const double* mkt_iv, const double* wgt,
                                                const double* spot, const double* rate, int B,
                                                const double* x0, const int32_t* market_of, int S,
                                                int N, double L, const dh_lb_options* opt,
                                                dh_lb_result* out, int32_t* n_launches) {
    if (!ctx || !s || !opt || (S > 0 && (!x0 || !out)) || (B > 0 && !mkt_iv))
        return fail(DH_E_ARG, "null argument");
    std::vector<double> w((size_t)std::max(B, 0) * s->M), wsum((size_t)std::max(B, 0), 0.0);
    const int rc = iv_check_weights(mkt_iv, wgt, B, s->M, true, w.data(), wsum.data());
    if (rc) return rc;
    LbBatch bt{mkt_iv, spot, rate, B, market_of};
    bt.iv_wgt = w.data();
    bt.iv_wsum = wsum.data();
    bt.grad = true;
    return lb_run(ctx, s, x0, S, 0.0, 0.0, N, L, opt, out, n_launches, &bt);
}

// Levenberg-Marquardt on the Gauss-Newton Hessian: dh_calibrate_lbfgs_batch_grad's arguments, checks
// and host loop; the iteration is the planes launch, dh_gauss_newton.h's reduction and
// lm_step_kernel (dh_lm.h).
extern "C" int dh_calibrate_lm_batch(dh_ctx* ctx, const dh_surface* s, const double* mkt,
                                     const double* spot, const double* rate, int B,
                                     const double* x0, const int32_t* market_of, int S, int N,
                                     double L, const dh_lb_options* opt, dh_lb_result* out,
                                     int32_t* n_launches) {
    LbBatch bt{mkt, spot, rate, B, market_of};
    bt.grad = true;
    bt.lm = true;
    return lb_run(ctx, s, x0, S, 0.0, 0.0, N, L, opt, out, n_launches, &bt);
}

extern "C" int dh_ctx_set_lb_trace(dh_ctx* ctx, int64_t cap) {
    if (!ctx) return fail(DH_E_ARG, "null argument");
    if (cap < 0) return fail(DH_E_ARG, "cap < 0");
    ctx->lb_trace_cap = cap;
    return DH_OK;
}

extern "C" int dh_ctx_read_lb_trace(dh_ctx* ctx, double* out, int64_t cap, int64_t* n) {
    if (!ctx || !n || (cap > 0 && !out)) return fail(DH_E_ARG, "null argument");
    *n = 0;
    if (ctx->lb_trace_cap == 0 || !ctx->lb_trace_n.ptr) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    unsigned long long cnt = 0;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(&cnt, ctx->lb_trace_n.ptr, 8, hipMemcpyDeviceToHost));
    const int64_t m = std::min<int64_t>({(int64_t)cnt, ctx->lb_trace_cap, cap});
    if (m > 0) HIP_TRY(hipMemcpy(out, ctx->lb_trace.ptr, (size_t)m * kLbTrace * 8, hipMemcpyDeviceToHost));
    *n = (int64_t)cnt;
    return DH_OK;
}
