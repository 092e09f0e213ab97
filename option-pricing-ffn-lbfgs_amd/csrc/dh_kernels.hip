// dh_kernels.hip -- gfx950 kernels of the COS pricing / calibration-objective hot path, and the
// library's one translation unit: the host side (launch planner, C ABI) and the features are the
// headers included at the end.
//
// Two kernels per request (DESIGN.md "Kernels"), each with its own small register footprint:
//
//   cos_table_kernel<TPT>  one table per (param set p, maturity group g):  for k < N
//     (blocks = resident capacity, each a contiguous range of tables; prologues of up to 64
//     tables computed lane-parallel by one wave)
//       w_k = Re(phi(u_k) e^{-i u_k a}) 2/(b-a)            (double_heston.py:48-97,163-168,187)
//     (8 bytes per term) plus per-(p, g) constants c0/c1 (call), c5 (put), w0 (k = 0 weight),
//     a, b, e^b, e^a reduced in a fixed order.  CF-bound; the table lands in an L2/MALL-resident
//     workspace.
//
//   cos_option_kernel<TPT> one task per (p, tile), a tile = <= 256 options of one maturity:
//     stage the (p, g) table into LDS, expanded to the strike-independent parts of chi_k/psi_k
//     (k >= 1, double_heston.py:141-158):  u_k = k pi/(b-a),  T2_k = w_k S0/(1+u_k^2),
//     T6_k = -T2_k/u_k;  per option one angle sum remains
//       S = sum_k T2_k cos(k th) + T6_k sin(k th),   th = pi (log(K/S0) - a)/(b - a),
//       price = e^{-rT} (const + w0 V_0 - e^{xK} S)
//     (the chi and psi parts at the log-strike, -e^{xK}(T2 cos + T2 u sin) + K (w/u) sin, with
//     K = S0 e^{xK}), computed by G lanes per group of kR options (lane j: k = 1 + j, 1 + j + G,
//     ...), cos/sin(k th) advanced by the Chebyshev recurrence x_{k+G} = 2 cos(G th) x_k -
//     x_{k-G} with an exact sincos re-anchor every kAnchor steps, then DPP butterflies.
//
//   Options whose [a, b] is widened by the log-strike clamp (double_heston.py:135-137) are
//   found and priced by the TABLE kernel (it already carries the CF code): per (p, group) it
//   writes a 64-bit mask word per 64 options and the clamped options' prices (per-term path on
//   the option's own range).  The option kernel only reads them, so it carries no CF code and
//   runs at ~100 VGPRs (4-5 waves per SIMD) instead of ~200.
//     Loss mode: fixed-order per-task partial of sum rel^2 and #invalid; the last task of p to
//     finish (agent-scope counter, sc1 hand-off) sums the partials in tile order.  No float
//     atomics: bitwise reproducible, independent of how many param sets share the launch.
//
//   Validation ("exact") mode runs cos_exact_kernel instead: per-term CF + sincos in the
//   reference's operation order, one wave per option.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <array>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "dh_device.h"
#include "dh_index.h"
#include "dh_lbfgs.h"
#include "dh_lm.h"
#include "dhcos.h"

using dh::cplx;
using dh::Params;

namespace {

constexpr int kBlock = 256;
constexpr int kTileMax = 256;
constexpr int kAnchor = 64;       // exact sincos re-anchor period of the angle recurrence
constexpr int kR = 4;             // options carried per lane in the option kernel
constexpr int kConsts = 8;        // c0, c1, c5, w0, a, b, e^b, e^a per table
constexpr size_t kTableBudget = size_t(256) << 20;   // table workspace per chunk (MALL-sized)
constexpr int kLdsMax = 160 * 1024;
constexpr int kLdsDyn = kLdsMax - 8192;   // dynamic LDS cap: the kernels keep <= 8 KB static

// Arrival counters of the loss hand-off, one per 128-byte line: every tile of a param set bumps
// its set's counter with an agent-scope atomic, and packed counters put all the sets of a
// request on one line, serialising every block's atomic (C2: 3.7k cycles per ticket).
constexpr int kCounterStride = 32;

struct PriceArgs {
    const double* prm;      // [P][16]
    int64_t P;              // param sets of the whole request
    int64_t p0, np;         // this launch covers param sets p0 .. p0 + np - 1
    const double* K;        // [M] sorted by T (absolute strike or K_relative)
    const double* T;        // [M]
    const int8_t* call;     // [M]
    const double* mkt;      // [M] or null
    const int* perm;        // [M] sorted -> caller index
    const int2* tiles;      // [n_tiles] (opt0, nopt)
    const int2* groups;     // [n_groups] (opt0, nopt) of each maturity group (null if paired)
    int max_group;          // largest group (clamp price slots per table)
    const int* tile_group;  // [n_tiles] maturity group of each tile
    const double* group_T;  // [n_groups]
    int n_tiles, n_groups;
    int opt_cap;            // >= largest tile (LDS option arrays)
    int paired;             // option i under param set i, one option per task
    int strike_mode;
    int exact;              // validation mode (host routes to cos_exact_kernel)
    int partials_only;      // 1: loss requests of the device L-BFGS-B: every task stores its partial
                            // (invalid flag in the sign bit) and ends (no hand-off); the step
                            // kernel forms the sums.  2: multi-round fused requests: every task
                            // stores its (partial, invalid count) pair and ends; loss_partials_kernel
                            // then forms the sums as the hand-off's last task would.  3: the same
                            // pairs as epoch-tagged granules (gran), summed by the grid's last
                            // P blocks in the same launch (tail_sums)
    int M;                  // options in the (sorted) option arrays
    int N;
    double L;
    double* out;            // prices [P*out_stride] or null
    int64_t out_stride;     // M (surface) or 0 (paired)
    double* part_sse;       // loss mode: [P*n_tiles] partials, else null
    int* part_bad;          // [P*n_tiles]
    unsigned* counter;      // [P * kCounterStride] arrival counters (zero between launches)
    double* sse;            // [P] final sums (loss mode)
    int* n_bad;             // [P]
    double* table;          // workspace: w_k, [np*tabs_per_p][N], or tiled (table_tiled) as
                            // [np*tabs_per_p / kTabTile][N][kTabTile]
    int table_tiled;        // set when cos_option_small_kernel reads the tables (table_w)
    double* consts;         // workspace: [np*tabs_per_p][kConsts]
    unsigned long long* cl_mask;   // workspace: [np*tabs_per_p][cl_words] clamp bits per option
    double* cl_price;       // workspace: [np*tabs_per_p][max_group] prices of clamped options
    unsigned long long* stamps;   // diagnostic builds (DH_STAMPS) only: [blocks][kStamps]
    const int* live_count;  // device-resident calibration: the launch is a no-op once every start
                            // has finished (*live_count == 0), else null
    const double* pre;      // fused kernel on large grids: [tables][kTabC] prologue constants
                            // formed by table_prologue_kernel ahead of it, else null
    double tail;            // tail_delta's scale: kTailScale, or -1 (dh_ctx_set_tail_cut(0): every
                            // term summed); set by launch_price
    // prologues ahead (fused kernel, requests of more than one round of resident blocks): block
    // q < ahead_stride (dispatch index) forms the truncation ranges and K_cf of the blocks
    // q + j ahead_stride (j = 1 .. kAheadMax) into ahead[.][kAheadRec] and then sets ahead_flag[.]
    // = ahead_epoch << 32 | K_cf; a later block whose flag holds this launch's epoch re-forms its
    // constants from the record instead of running the cumulant chain and the CF-cut test
    double* ahead;
    unsigned long long* ahead_flag;   // epoch << 32 | K_cf of the table's record
    int ahead_stride;       // 0: off
    unsigned ahead_epoch;
    // partials_only == 3: [P * n_tiles][2] granules (epoch-tagged halves of each task's pair)
    unsigned long long* gran;
    int remap;              // fused kernel: dispatch index -> table by XCD (xcd_table), else 0
    int host_out;           // sse / n_bad in mapped host memory (the host API's zero-copy
                            // requests): written by system-scope stores, drained (loss_out)
    // the surface's spot cache (dh_surface_stage_spot; xk_s null: off): [M] log(K / S0), K / S0
    // and the strike option_strike gives, formed for the S0 whose bits are spot_staged.  The
    // fused kernel's blocks whose record carries those bits load them instead of computing them
    const double* xk_s;
    const double* exk_s;
    const double* k_s;
    unsigned long long spot_staged;
};

// w_k of table q sits at table_w(A, q)[k * table_step(A)].  The small-tile option kernel has one
// lane per table, so a row-major table puts every lane of a load on its own line (64 lines per
// wave-load, ~30% VALU issue in round 2); tiled, kTabTile consecutive tables share each line and
// a wave-load touches 4 lines.  The table kernel's writes then scatter over kTabTile-table lines
// that its 64-table batches fill within L2.
constexpr int kTabTile = 16;
__device__ __forceinline__ int table_step(const PriceArgs& A) { return A.table_tiled ? kTabTile : 1; }
__device__ __forceinline__ double* table_w(const PriceArgs& A, int64_t q) {
    return A.table_tiled ? A.table + (q / kTabTile) * kTabTile * (int64_t)A.N + (q % kTabTile)
                         : A.table + q * (int64_t)A.N;
}

// A launch enqueued ahead by dh_calibrate_lbfgs after its starts have all finished returns at
// once.  The count only changes between launches (the step kernel writes it), so every block of
// a launch takes the same branch and the loss hand-off counters stay consistent.
__device__ __forceinline__ bool halted(const PriceArgs& A) {
    return A.live_count && __builtin_amdgcn_readfirstlane(*A.live_count) <= 0;
}

// In-kernel phase stamps, compiled only into the diagnostic build (make stamps): lane 0 of each
// block of the option kernel writes s_memtime at its phase boundaries.
constexpr int kStamps = 32;     // [24, 28): HW_ID of waves 0..3 (SIMD placement)
#ifdef DH_STAMPS
#define DH_STAMP_T(A, i, thr)                                                              \
    do {                                                                                   \
        if ((A).stamps && threadIdx.x == (thr)) {                                          \
            unsigned long long _t;                                                         \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");     \
            (A).stamps[(size_t)blockIdx.x * kStamps + (i)] = _t;                          \
        }                                                                                  \
    } while (0)
// the block's residency in the chip-wide 100 MHz clock (s_memrealtime): slot 23 = start << 32 |
// end, low 32 bits of each (tools/stamps.py --timeline)
#define DH_RT_BEGIN(A)                                                                     \
    unsigned long long _rt0 = 0;                                                           \
    if ((A).stamps && threadIdx.x == 0)                                                    \
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_rt0)::"memory");    \
    if ((A).stamps && (threadIdx.x & 63) == 0 && threadIdx.x < 256) {                      \
        unsigned _hw;                                                                      \
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(_hw));                  \
        (A).stamps[(size_t)blockIdx.x * kStamps + 24 + (threadIdx.x >> 6)] = _hw;          \
    }
#define DH_RT_END(A)                                                                       \
    do {                                                                                   \
        if ((A).stamps && threadIdx.x == 0) {                                              \
            unsigned long long _rt1;                                                       \
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_rt1)::"memory"); \
            (A).stamps[(size_t)blockIdx.x * kStamps + 23] = (_rt0 << 32) | (_rt1 & 0xffffffffull); \
        }                                                                                  \
    } while (0)
#else
#define DH_STAMP_T(A, i, thr) do {} while (0)
#define DH_RT_BEGIN(A) do {} while (0)
#define DH_RT_END(A) do {} while (0)
#endif
#define DH_STAMP(A, i) DH_STAMP_T(A, i, 0)

__host__ __device__ inline int tabs_per_p(const PriceArgs& A) { return A.paired ? 1 : A.n_groups; }
__host__ __device__ inline int cl_words(const PriceArgs& A) { return (A.max_group + 63) / 64; }

// log(K / S0) and K / S0 (= e^{xK} to an ulp) of sorted option m under spot S0
__device__ __forceinline__ double option_logk(double K, double S0, double& ratio) {
    ratio = K / S0;
    return dh::dlog(ratio);                                          // double_heston.py:162
}

__device__ __forceinline__ double option_strike(const PriceArgs& A, int m, double S0) {
    const double Kin = A.K[m];
    return (A.strike_mode == DH_STRIKE_PCT_SPOT) ? Kin * S0 / 100.0 : Kin;
}

// dh_surface_stage_spot: the two functions above for every option of the surface under one spot,
// once (A: K, strike_mode and M).  The fused kernel's staging loop forms the same values by the
// same functions, so a block may load these instead.
__global__ __launch_bounds__(kBlock) void stage_spot_kernel(PriceArgs A, double S0,
                                                            double* __restrict__ k_s,
                                                            double* __restrict__ xk_s,
                                                            double* __restrict__ exk_s) {
    const int m = blockIdx.x * kBlock + threadIdx.x;
    if (m >= A.M) return;
    const double K = option_strike(A, m, S0);
    double ratio;
    const double xK = option_logk(K, S0, ratio);
    k_s[m] = K;
    xk_s[m] = xK;
    exk_s[m] = ratio;
}

// ----------------------------------------------------------------------------------------------
// table kernel
// ----------------------------------------------------------------------------------------------
// Per-term path for a clamp-widened option: own range [a, b], own u grid, CF per term (fast
// exponent form) and the generic chi/psi (double_heston.py:141-158,160-192).  Lane share of
// the sum' over k = k_first, k_first + k_step, ...
__device__ __forceinline__ double clamped_term_sum(const Params& P, double T, double K, double xK,
                                                   double a, double b, bool is_call, int k_first,
                                                   int k_step, int N, const double2* sct) {
    const dh::CfConsts CC = dh::cf_consts(P, T);
    const double ba = b - a;
    const double scale = 2.0 / ba;
    double acc = 0.0;
    for (int k = k_first; k < N; k += k_step) {
        const double u = k * dh::kPi / ba;
        const double w = dh::cf_phase_re(CC, u, T, a, sct) * scale;
        double chi, psi;
        if (is_call) dh::cos_coeffs(k, xK, b, a, b, chi, psi);
        else dh::cos_coeffs(k, a, xK, a, b, chi, psi);
        const double V = is_call ? (P.S0 * chi - K * psi) : (K * psi - P.S0 * chi);
        acc += (k == 0 ? 0.5 : 1.0) * w * V;
    }
    return acc;
}

constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141, kDppMirror = 0x140;
template <int Ctrl>
__device__ __forceinline__ double dpp_f64(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, Ctrl, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), Ctrl, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// the value of lane ^ 16 (or lane ^ 32): v_permlane16_swap / v_permlane32_swap of v with itself
// swap the odd rows (upper half) of the first copy with the even rows (lower half) of the second,
// so the second copy holds the partner's value in the even rows (lower half) and the first in the
// odd rows (upper half)
template <bool k32>
__device__ __forceinline__ double xor_partner(double v) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
    const bool upper = (__lane_id() & (k32 ? 32 : 16)) != 0;
    unsigned plo, phi;
    if constexpr (k32) {
        const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        plo = upper ? l[0] : l[1];
        phi = upper ? h[0] : h[1];
    } else {
        const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        plo = upper ? l[0] : l[1];
        phi = upper ? h[0] : h[1];
    }
    return __longlong_as_double(((long long)phi << 32) | plo);
}

// s summed over its aligned group of `width` lanes (a power of two <= 64) exactly as the xor
// butterfly s += __shfl_xor(s, off), off = 1, 2, 4, ... < width, sums it, without an LDS round
// trip per level: levels 1 and 2 are DPP quad permutes, levels 4 and 8 DPP half-row / row mirrors
// (after the lower levels every lane of a quad (half-row) holds the same value, so the mirror
// partner's operand is the xor partner's and every sum is the same bits), levels 16 and 32
// v_permlane16/32_swap.  Every lane of the wave must be active.
__device__ __forceinline__ double xor_sum(double s, int width) {
    if (width > 1) s += dpp_f64<kDppXor1>(s);
    if (width > 2) s += dpp_f64<kDppXor2>(s);
    if (width > 4) s += dpp_f64<kDppHalfMirror>(s);
    if (width > 8) s += dpp_f64<kDppMirror>(s);
    if (width > 16) s += xor_partner<false>(s);
    if (width > 32) s += xor_partner<true>(s);
    return s;
}

// Adaptive tail of the angle sums.  A table's terms k >= n_eff are not summed, n_eff - 1 being
// the last k >= 1 with |T2_k| > tail_delta.  Past it |T6_k| = |T2_k| / u_k <= |T2_k| (b - a)/pi,
// so the dropped part of S is at most (1 + (b - a)/pi) N delta = 2^-72 S0/(b - a), and a price
// moves by at most e^{-rT} e^{xK} 2^-72 S0/(b - a) = e^{-rT} 2^-72 K/(b - a): below 2^-64 of its
// own k = 0 term e^{-rT} w0 V0 (w0 = 1/(b - a); V0 >= 0.0048 K because the log-strike lies at
// least 0.1 inside [a, b] -- clamp-widened options take the per-term path), i.e. far inside the
// price's rounding.  The characteristic function decays like exp(-c u): at N = 512 (C3) a table
// keeps ~26% of its terms, at N = 256 ~46%, at N = 128 ~97%.  Every path forms n_eff from the
// same T2_k values with the same expressions, so fused and split keep their identical bits.
// NaN / inf entries (and a NaN delta) always count as kept: a NaN still reaches the price.
constexpr double kTailScale = 0x1.0p-72;
__device__ __forceinline__ double tail_delta(double scale, double S0, double ba, int N) {
    return scale * S0 / (ba * (1.0 + ba * (1.0 / dh::kPi)) * (double)N);
}
__device__ __forceinline__ int tail_keep(int k, double T2, double delta) {
    return fabs(T2) <= delta ? 0 : k + 1;
}
__device__ __forceinline__ int xor_max_i(int v, int width) {
    for (int off = 1; off < width; off <<= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// Certified end of a table's CF entries.  For one Heston factor, conditioning on its variance
// path leaves a Gaussian part with variance (1 - rho^2) I (I = the integrated variance), so
// |phi_factor(u)| <= E[exp(-s I)] with s = u^2 (1 - rho^2) / 2: the CIR Laplace transform
// exp(A(s) - B(s) v0), which decreases in u; the jump factor's modulus is <= 1 (lambda >= 0) and
// the drift's is 1.  So |T2_k| <= 2 S0 M(u_k) / ((b - a)(1 + u_k^2)) =: bound(k), decreasing in
// k, and from the first k with bound(k) <= delta / 2 (tail_delta) on every entry would be dropped
// by the tail cut anyway: the CF is not evaluated there (K_cf, prologue slot 30).  The bound
// follows |phi| closely: at N = 512 (C3) K_cf is ~7 terms past n_eff, ~28% of N
// (tests/test_cf_cut_bound.py checks the bound against the oracle's CF).
// The test runs in fp32 at the native rate (v_exp / v_log / v_sqrt / v_rcp, ~1 ulp each; the
// errors, ~1e-6 relative on log values of magnitude < 1e3 near the threshold, sit far inside the
// 0.01 log-margin it keeps) on the
// candidates k_j = (j + 1) ceil(N / 64), j < 64: K_cf is the first that passes (else N).  The
// one-lane scan (table_prologue) and the wave's ballot (table_prologue_wave) test the same
// candidates with the same bits, so they pick the same one.  Series of N < 256 terms are not
// cut: at N = 128 (C1, C5) almost every term lies inside the bound.  At N = 256 (C2, C4) the cut
// costs C2 nothing now that the test runs on its own wave at the native fp32 rate, and C4 gains
// 2.5% (with the first, libm-rate test on wave 0 it had cost C2 12.1 -> 12.9 us).  Parameters
// outside the model's domain (kappa, sigma, T <= 0, theta, v0, lambda < 0, |rho| > 1, NaN) and a
// disabled tail cut (delta < 0) are not cut either.
constexpr int kCfCutMinN = 256;

// fp32 at the native rate: v_sqrt_f32, v_exp_f32 / v_log_f32 (base 2, ~1 ulp) and v_rcp_f32
__device__ __forceinline__ float f_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504f); }
__device__ __forceinline__ float f_log(float x) { return __builtin_amdgcn_logf(x) * 0.693147181f; }
__device__ __forceinline__ float f_div(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }

// log E[exp(-s I)] of one CIR factor, A(s) - B(s) v0, in a cancellation-free form.  The textbook
// A = (2 kappa theta / sigma^2) [log(2g) + (kappa - g) tau / 2 - log(den)] takes a difference of
// O(1) logs and scales it by 2 kappa theta / sigma^2: at small sigma the fp32 rounding of the logs
// is amplified past the test's margin.  With x = g tau, om = 1 - e^-x,
// h(x) = x - om >= 0, g - kappa = 2 sigma^2 s / (g + kappa) and den = 2g - (g - kappa) om:
//   A = -(2 kappa theta s / (g + kappa)) (h - om (R - 1)) / g,
//   R = -log(1 - y) / y,  y = sigma^2 s om / ((g + kappa) g) <= 1/2,
// where h and om come from one series for x < 1 (no 1 - e^-x cancellation) and R - 1 from its
// series for small y.  Each piece is within a few fp32 ulps, h - om (R - 1) cancels by at most a
// factor of 2 (om (R - 1) <= h / 2), and A, -B v0 are both <= 0: the log-bound is within ~1e-5
// relative of the exact one for every sigma > 0 (tests/test_cf_cut_bound.py, sigma down to 1e-6,
// kappa theta / sigma^2 up to 1e9).
__device__ __forceinline__ float cir_log_laplace(float s, float tau, float v0, float kap,
                                                 float th, float sig) {
#pragma clang fp contract(off)
    const float s2 = sig * sig;
    const float g = __builtin_amdgcn_sqrtf(kap * kap + 2.0f * s2 * s);
    const float gk = g + kap;
    const float x = g * tau;
    float h, om, e;
    if (x < 1.0f) {          // h = x^2/2 - x^3/6 + ... (Horner through x^11 / 11!: < 1e-8 rel.)
        float p = 1.0f / 39916800.0f;
        p = p * -x + 1.0f / 3628800.0f;
        p = p * -x + 1.0f / 362880.0f;
        p = p * -x + 1.0f / 40320.0f;
        p = p * -x + 1.0f / 5040.0f;
        p = p * -x + 1.0f / 720.0f;
        p = p * -x + 1.0f / 120.0f;
        p = p * -x + 1.0f / 24.0f;
        p = p * -x + 1.0f / 6.0f;
        p = p * -x + 0.5f;
        h = p * (x * x);
        om = x - h;
        e = 1.0f - om;
    } else {
        e = f_exp(-x);
        om = 1.0f - e;
        h = x - om;
    }
    const float y = f_div(s2 * s * om, gk * g);
    float rm1;               // R - 1 = y/2 + y^2/3 + y^3/4 + ...
    if (y < 0.125f) {
        float q = 1.0f / 9.0f;
        q = q * y + 1.0f / 8.0f;
        q = q * y + 1.0f / 7.0f;
        q = q * y + 1.0f / 6.0f;
        q = q * y + 1.0f / 5.0f;
        q = q * y + 0.25f;
        q = q * y + 1.0f / 3.0f;
        q = q * y + 0.5f;
        rm1 = q * y;
    } else {
        rm1 = f_div(-f_log(1.0f - y) - y, y);
    }
    const float D = f_div(h - om * rm1, g);
    const float A = -f_div(2.0f * kap * th * s, gk) * D;
    const float den = gk * om + 2.0f * g * e;
    const float B = f_div(2.0f * s * om, den);
    return A - B * v0;
}

__device__ __forceinline__ bool cf_cut_domain(const dh::Params& P, double T, double delta, int N) {
    return N >= kCfCutMinN && delta > 0.0 &&
           P.k1 > 0.0 && P.t1 >= 0.0 && P.s1 > 0.0 && P.v01 >= 0.0 && fabs(P.r1) <= 1.0 &&
           P.k2 > 0.0 && P.t2 >= 0.0 && P.s2 > 0.0 && P.v02 >= 0.0 && fabs(P.r2) <= 1.0 &&
           P.lam >= 0.0 && T > 0.0 && P.S0 > 0.0;
}

// log(delta / 2) less the margin: the candidates' threshold (fp32, native rate; delta > 0 and
// far above fp32's normal range: ~2^-80 S0)
__device__ __forceinline__ float cf_cut_threshold(double delta) {
    return f_log(0.5f * (float)delta) - 0.01f;
}

// bound(k) <= delta / 2 with the margin, in logs, fp32
__device__ __forceinline__ bool cf_cut_passes(const dh::Params& P, float T, float ba, float thr,
                                              int k) {
#pragma clang fp contract(off)
    const float u = (float)k * f_div(3.14159265f, ba);
    const float u2 = u * u;
    const float lm =
        cir_log_laplace(0.5f * u2 * (1.0f - (float)P.r1 * (float)P.r1), T, (float)P.v01,
                        (float)P.k1, (float)P.t1, (float)P.s1) +
        cir_log_laplace(0.5f * u2 * (1.0f - (float)P.r2 * (float)P.r2), T, (float)P.v02,
                        (float)P.k2, (float)P.t2, (float)P.s2);
    return f_log(f_div(2.0f * (float)P.S0, ba * (1.0f + u2))) + lm <= thr;
}

__host__ __device__ constexpr int cf_cut_step(int N) { return (N + 63) / 64; }

__device__ __forceinline__ int cf_cut_scan(const dh::Params& P, double T, double a, double b,
                                           double delta, int N) {
    if (!cf_cut_domain(P, T, delta, N)) return N;
    const float thr = cf_cut_threshold(delta), ba = (float)(b - a);
    const int st = cf_cut_step(N);
    for (int j = 0; j < 64; ++j) {
        const int k = (j + 1) * st;
        if (k >= N) break;
        if (cf_cut_passes(P, (float)T, ba, thr, k)) return k;
    }
    return N;
}

__device__ __forceinline__ int cf_cut_wave(const dh::Params& P, double T, double a, double b,
                                           double delta, int N, int lane) {
    if (!cf_cut_domain(P, T, delta, N)) return N;           // uniform
    const int st = cf_cut_step(N);
    const int k = (lane + 1) * st;
    const bool ok = k < N && cf_cut_passes(P, (float)T, (float)(b - a), cf_cut_threshold(delta), k);
    const unsigned long long m = __ballot(ok);
    return m ? (__ffsll((long long)m)) * st : N;      // lowest passing lane j: (j + 1) st
}

// per-table values staged in LDS by the prologue lane of the table:
//   [0..5] a, b, e^b, e^a, 2/(b-a), pi/(b-a) | [6..21] CfConsts | [22] S0, [23] r, [24] T,
//   [25] K/S0 below which the clamp test must be evaluated, [26] above which (prefilter),
//   [27] group's first option, [28] group size (as doubles), [29] the discount e^{-rT},
//   [30] K_cf: the CF entries k < K_cf are evaluated (cf_cut_scan), as a double
constexpr int kTabC = 31;
constexpr double kClampMargin = 1e-9;   // relative safety margin of the K-space prefilter
static_assert(sizeof(dh::CfConsts) == 16 * sizeof(double), "CfConsts layout");

// Prologue of table q = (p, g) of a launch: truncation range, CF constants and the staged values
// above, written to c[0 .. kTabC).
__device__ __forceinline__ void table_prologue(const PriceArgs& A, int64_t q, double* c,
                                               bool with_cut = true) {
#pragma clang fp contract(off)   // table_prologue and table_prologue_wave: same bits
    const int tpp = tabs_per_p(A);
    const int64_t p = A.p0 + q / tpp;
    const int g = (int)(q % tpp);
    const Params P = dh::load_params(A.prm + p * DH_PARAM_STRIDE);
    const double T = A.paired ? A.T[p] : A.group_T[g];
    int2 gr = make_int2((int)p, 1);
    if (!A.paired) gr = A.groups[g];
    double a, b;
    dh::trunc_unclamped(P, T, A.L, a, b);            // double_heston.py:100-132
    const dh::CfConsts CC = dh::cf_consts(P, T);
    c[0] = a;
    c[1] = b;
    c[2] = exp(b);
    c[3] = exp(a);
    c[4] = 2.0 / (b - a);
    c[5] = dh::kPi / (b - a);
    const double* cc = (const double*)&CC;
    for (int i = 0; i < 16; ++i) c[6 + i] = cc[i];
    c[22] = P.S0;
    c[23] = P.r;
    c[24] = T;
    // unclamped iff a + 0.1 <= log(K/S0) <= b - 0.1: strikes whose K/S0 is inside these
    // bounds by a 1e-9 relative margin cannot be clamped (exp/log errors are ~1e-16)
    c[25] = exp(a + 0.1) * (1.0 + kClampMargin);
    c[26] = exp(b - 0.1) * (1.0 - kClampMargin);
    c[27] = gr.x;
    c[28] = gr.y;
    c[29] = exp(-P.r * T);
    if (with_cut) c[30] = cf_cut_scan(P, T, a, b, tail_delta(A.tail, P.S0, b - a, A.N), A.N);
}

// table_prologue run by one wave in lockstep (the fused kernel's wave 0): the two variance
// factors' cumulants and CF constants on alternate lanes, the five exponentials (e^b, e^a, the
// clamp bounds' e^(a+0.1) and e^(b-0.1), and the jump compensator's e^(mu + sj^2/2)) one per lane,
// broadcast with readlane.  Every value is the same expression on the same inputs as in
// table_prologue and cf_consts, so the staged constants are the same bits.
__device__ __forceinline__ double lane_bcast(double v, int l) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, l);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// The fused kernel's leading arguments: what its prologue reads first.  As plain scalar kernel
// arguments ahead of PriceArgs they are preloaded into SGPRs at wave launch (gfx950 kernarg
// preloading, -mllvm -amdgpu-kernarg-preload-count, Makefile), so the parameter, maturity and
// group loads issue at once instead of behind a kernel-argument load (one memory round trip
// less on the request's critical path).  The fused launch has p0 = 0.
struct FusedHead {
    const double* prm;      // PriceArgs::prm
    const double* tsrc;     // PriceArgs::T (paired) or ::group_T
    const int2* groups;     // PriceArgs::groups
    const int* live;        // PriceArgs::live_count, or kLiveOne when null
    const double* pre;      // PriceArgs::pre
    int tpp;                // tabs_per_p
    int paired;
};

// A by-value kernel argument read in place: its fields load from the kernel-argument segment at
// their uses.  (Every use of a by-value argument is lowered to a load in the kernel's entry block;
// with the SGPR file full the compiler then spills them to VGPR lanes at once, which waits for the
// whole load before the prologue's first memory access can issue.)  off = the argument's byte
// offset in the segment: the preceding arguments at their natural alignment.
template <typename T, int off>
__device__ __forceinline__ const T& karg_ref() {
    typedef const __attribute__((address_space(4))) char* KargPtr;
    const KargPtr k = (KargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    return *(const T*)(const char*)(k + off);
}
// FusedHead's arguments: 5 pointers and 2 ints, so PriceArgs starts at byte 48 (kernel arguments
// are laid out in declaration order at their natural alignment, as the members of this struct)
constexpr int kFusedArgsKernargOff = 48;
struct FusedKargs {         // cos_fused_kernel's argument list as a struct (its kernarg layout)
    const double* prm;
    const double* tsrc;
    const int2* groups;
    const int* live;
    const double* pre;
    int tpp, paired;
    PriceArgs A;
};
static_assert(offsetof(FusedKargs, A) == kFusedArgsKernargOff, "PriceArgs kernarg offset");
// karg_prefetch_lines (below) reads up to byte 0x1b4: inside the explicit arguments and the 256
// bytes of implicit ones every HIP kernel's segment carries after them
static_assert(sizeof(FusedKargs) + 256 >= 0x1b4, "kernel-argument prefetch past the segment");

// Small requests' param records in the kernel arguments (cos_fused_kernel<..., KP = true>): the
// host driver's function+gradient requests of one start (14 records) travel in the
// launch's kernel-argument segment, which the runtime writes to device memory ahead of the
// dispatch, instead of being read by the blocks from mapped host memory across PCIe at the start
// of the request's critical path (C1: 11.9 -> 10.1 us per kernel with the records in HBM).  One
// start's 14 records: 1,792 bytes, 2,720 with the rest of the arguments (the groups below among
// them) and 2,976 with the runtime's hidden ones (28 records would pass the 4 KiB segment).
constexpr int kKargSets = 14;
// and, for surfaces of at most kKargGroups maturity groups (C1's 3, C2's 32), the groups' maturities
// and option ranges: the prologue's first dependent load (the table's T) then comes from the
// kernel-argument segment too instead of device memory (C2 prologue chain: one memory round trip)
constexpr int kKargGroups = 32;
struct KargParams {
    double v[kKargSets * DH_PARAM_STRIDE];
    double T[kKargGroups];
    int2 groups[kKargGroups];
};
struct NoKargParams {
    int unused;
};
struct FusedKargsKP {       // cos_fused_kernel<..., true>'s argument list
    FusedKargs head;
    int tpt2;
    KargParams pb;
};
constexpr int kFusedParamsKernargOff = 416;
static_assert(offsetof(FusedKargsKP, pb) == kFusedParamsKernargOff, "param block kernarg offset");
static_assert(sizeof(FusedKargsKP) + 256 <= 4096, "kernel arguments over 4 KiB");

#ifndef DH_PRE_GROUP8
#define DH_PRE_GROUP8 1
#endif
#ifndef DH_KARG_PREFETCH
#define DH_KARG_PREFETCH 1
#endif
// The kernel-argument lines the fused kernel reads PriceArgs from (in place, karg_ref; the step
// kernel's LbArgs lie in the same byte range), pulled
// into the scalar cache in ONE round trip at entry: one s_load_dword per 64-byte line brings the
// whole line, and the wave waits once.  Without it the prologue's path met each line as its own
// dependent round trip (xcd_table's switch, the ahead stride, the tail-cut and table fields: five
// serial ~550-cycle misses before the table record could be loaded, tools/ubench/kernarg_latency).
// The lines are 64 bytes apart from byte 0x30 through 0x1b0 (PriceArgs and the arguments after
// it), so every line is touched whatever the segment's alignment.
__device__ __forceinline__ void karg_prefetch_lines() {
#if DH_KARG_PREFETCH
    const char* ka = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
    unsigned d0, d1, d2, d3, d4, d5, d6;
    asm volatile(
        "s_load_dword %0, %7, 0x30\n\t"
        "s_load_dword %1, %7, 0x70\n\t"
        "s_load_dword %2, %7, 0xb0\n\t"
        "s_load_dword %3, %7, 0xf0\n\t"
        "s_load_dword %4, %7, 0x130\n\t"
        "s_load_dword %5, %7, 0x170\n\t"
        "s_load_dword %6, %7, 0x1b0\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=s"(d0), "=s"(d1), "=s"(d2), "=s"(d3), "=s"(d4), "=s"(d5), "=s"(d6)
        : "s"(ka)
        : "memory");
#endif
}

// the live count read by launches without one (FusedHead::live): the halt test is then a load
// like any other, with no branch on the pointer (a branch made the compiler wait for it at the
// kernel's entry)
__device__ const int kLiveOne = 1;

// The table (p * tpp + g) the fused grid's block of dispatch index b prices.  With A.remap the
// blocks that share an XCD (b and b + 8: MI355X_MICROARCH.md, round-robin dispatch, observed, for
// speed only) take, in dispatch order, one contiguous run of the tables in maturity-major order
// (g * P + p): each XCD's L2 then holds ~1/8 of the option arrays, and the blocks running together
// on an XCD stage the same maturity group's options.  A bijection onto the grid's tables for any
// grid size, so any placement gives the same bits.
__device__ __forceinline__ int64_t xcd_table(const PriceArgs& A, int tpp, int64_t b) {
    if (!A.remap) return b;
    const unsigned nb = gridDim.x;
    const unsigned x = (unsigned)b & 7u, pos = (unsigned)b >> 3;
    const unsigned per = nb >> 3, extra = nb & 7u;
    const unsigned t = x * per + min(x, extra) + pos;        // maturity-major rank
    const unsigned np = nb / (unsigned)tpp;
    const unsigned g = t / np, p = t - g * np;
    return (int64_t)p * tpp + g;
}

// The truncation range of table q (trunc_unclamped's bits) with the two variance factors'
// cumulants on alternate lanes: table_prologue_wave's first step, and the whole of what
// prologue_cut_wave needs.
__device__ __forceinline__ void prologue_range_wave(const PriceArgs& A, const FusedHead& H,
                                                    int64_t q, int lane, Params& P, double& T,
                                                    double& a, double& b) {
#pragma clang fp contract(off)   // table_prologue and table_prologue_wave: same bits
    const int64_t p = (int64_t)((unsigned)q / (unsigned)H.tpp);
    const int g = (int)((unsigned)q % (unsigned)H.tpp);
    P = dh::load_params(H.prm + p * DH_PARAM_STRIDE);
    T = H.tsrc[H.paired ? p : g];
#ifdef DH_STAMPS
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the record and T (scalar loads) are in
#endif
    DH_STAMP_T(A, 31, 0);
    const bool two = lane & 1;                     // factor 2 on odd lanes
    const double v0 = two ? P.v02 : P.v01, k = two ? P.k2 : P.k1, th = two ? P.t2 : P.t1;
    const double sg = two ? P.s2 : P.s1, rh = two ? P.r2 : P.r1;
    double c1j, c2j;
    dh::factor_cumulants(T, P.r, v0, k, th, sg, rh, c1j, c2j);   // double_heston.py:101-118
    const double c1 = lane_bcast(c1j, 0) + lane_bcast(c1j, 1) + P.lam * T * P.muj;
    const double c2 = lane_bcast(c2j, 0) + lane_bcast(c2j, 1) +
                      P.lam * T * (P.sj * P.sj + P.muj * P.muj);
    const double h = A.L * sqrt(fabs(c2));
    a = c1 - h;                                    // trunc_unclamped (double_heston.py:120-132)
    b = c1 + h;
}

// K_cf of table q by one wave (cf_cut_wave on prologue_range_wave's range): in the fused kernel
// a wave other than the prologue's runs it, so the bound's fp32 chain overlaps the prologue's
// instead of following it.
__device__ __forceinline__ int prologue_cut_wave(const PriceArgs& A, const FusedHead& H,
                                                 int64_t q, int lane) {
    Params P;
    double T, a, b;
    prologue_range_wave(A, H, q, lane, P, T, a, b);
    return cf_cut_wave(P, T, a, b, tail_delta(A.tail, P.S0, b - a, A.N), A.N, lane);
}

// with_cut: also K_cf (slot 30); else the caller's other wave stores it
__device__ __forceinline__ void table_prologue_wave(const PriceArgs& A, const FusedHead& H,
                                                    int64_t q, double* c, int lane,
                                                    bool with_cut) {
#pragma clang fp contract(off)   // table_prologue and table_prologue_wave: same bits
    Params P;
    double T, a, b;
    prologue_range_wave(A, H, q, lane, P, T, a, b);
    DH_STAMP_T(A, 28, 0);
    const int64_t p = (int64_t)((unsigned)q / (unsigned)H.tpp);
    const int g = (int)((unsigned)q % (unsigned)H.tpp);
    int2 gr = make_int2((int)p, 1);
    if (!H.paired) gr = H.groups[g];
    const bool two = lane & 1;                     // factor 2 on odd lanes
    const double v0 = two ? P.v02 : P.v01, k = two ? P.k2 : P.k1, th = two ? P.t2 : P.t1;
    const double sg = two ? P.s2 : P.s1, rh = two ? P.r2 : P.r1;
    const dh::FactorC Fj = dh::factor_consts(v0, k, th, sg, rh);
    const int e_lane = lane < 6 ? lane : 0;
    const double arg = e_lane == 0 ? b : e_lane == 1 ? a : e_lane == 2 ? a + 0.1
                     : e_lane == 3 ? b - 0.1 : e_lane == 4 ? P.muj + 0.5 * (P.sj * P.sj)
                     : -P.r * T;
    const double e = exp(arg);
    dh::CfConsts CC;
    double* f1 = (double*)&CC.f1;
    double* f2 = (double*)&CC.f2;
    const double* fj = (const double*)&Fj;
    for (int i = 0; i < (int)(sizeof(dh::FactorC) / 8); ++i) {
        f1[i] = lane_bcast(fj[i], 0);
        f2[i] = lane_bcast(fj[i], 1);
    }
    const double comp = lane_bcast(e, 4) - 1.0;    // cf_consts
    CC.drift = (P.r - P.q - P.lam * comp) * T;
    CC.half_sj2 = 0.5 * (P.sj * P.sj);
    CC.muj = P.muj;
    CC.lt = P.lam * T;
    DH_STAMP_T(A, 30, 0);
    const int kcf =
        with_cut ? cf_cut_wave(P, T, a, b, tail_delta(A.tail, P.S0, b - a, A.N), A.N, lane) : 0;
    if (lane == 0) {
        c[0] = a;
        c[1] = b;
        c[2] = e;
        c[3] = lane_bcast(e, 1);
        c[4] = 2.0 / (b - a);
        c[5] = dh::kPi / (b - a);
        const double* cc = (const double*)&CC;
        for (int i = 0; i < 16; ++i) c[6 + i] = cc[i];
        c[22] = P.S0;
        c[23] = P.r;
        c[24] = T;
        c[25] = lane_bcast(e, 2) * (1.0 + kClampMargin);
        c[26] = lane_bcast(e, 3) * (1.0 - kClampMargin);
        c[27] = gr.x;
        c[28] = gr.y;
        c[29] = lane_bcast(e, 5);
        if (with_cut) c[30] = kcf;
    }
}

// cf_cut_scan by a group of 8 lanes (sub = 0..7; the group's lanes are active together): the
// candidates in chunks of 8 in increasing j, each chunk's first passing lane from the wave's
// ballot, so the same first passing candidate -- the same K_cf -- as the one-lane scan.
constexpr int kPreLanes = 8;
__device__ __forceinline__ int cf_cut_group8(const dh::Params& P, double T, double a, double b,
                                             double delta, int N, int sub) {
    if (!cf_cut_domain(P, T, delta, N)) return N;              // uniform in the group
    const float thr = cf_cut_threshold(delta), ba = (float)(b - a);
    const int st = cf_cut_step(N);
    const int sh = (int)(__lane_id() & ~(kPreLanes - 1));      // the group's bits in the ballot
    for (int j0 = 0; j0 < 64; j0 += kPreLanes) {
        if ((j0 + 1) * st >= N) break;                         // every candidate left is >= N
        const int k = (j0 + sub + 1) * st;
        const bool ok = k < N && cf_cut_passes(P, (float)T, ba, thr, k);
        const unsigned m = (unsigned)(__ballot(ok) >> sh) & ((1u << kPreLanes) - 1u);
        if (m) return (j0 + __ffs((int)m)) * st;               // j = j0 + ffs - 1, k = (j + 1) st
    }
    return N;
}

// ----------------------------------------------------------------------------------------------
// Prologues ahead (round 5).  A fused request of more than one round of resident blocks (C3:
// 4,200 tables on 1,024 slots) spends ~18% of every block's chain, and ~1,000 wave-instructions
// per table, on the serial prologue (table_prologue_wave + the CF-cut test).  Its first-round
// blocks form the later-round tables' prologues on the cut wave during the CF loop, which leaves
// that wave idle on C3's tables: 8 lanes per table (the two variance factors on sub-lanes 0 and 1,
// the six exponentials on sub-lanes 0 .. 5: table_prologue_wave's expressions on the same
// operands, uncontracted, so the same bits), the CF-cut candidates 8 at a time (cf_cut_group8:
// the same first passing candidate as the wave's ballot).  The constants go out with agent-scope
// stores; once drained (s_waitcnt vmcnt(0)), after the block's CF barrier a flag per table takes
// the launch's epoch -- MI355X_MICROARCH.md's "valid forms" row 1, as the loss hand-off.  A later
// block reads its flag: set, it loads the record (wave 0) and K_cf (the cut wave); not set (its
// writer has not got there: never seen, dispatch runs in block order and a later block starts only
// after a whole block lifetime), it forms them itself.  Either way the same values, so the same
// bits.
// ----------------------------------------------------------------------------------------------
constexpr int kAheadMax = 8;       // later tables per first-round block: 8-lane groups of a wave
// What travels per later table: the prologue's values that cost a transcendental or a cumulant
// chain -- a, b, e^b, e^a, the clamp bounds' slots 25 and 26, e^{-rT} and the CF drift -- at
// ahead[q * kAheadRec + i] (one 64-byte record per table, the writer group's 8 lanes storing it in
// one coalesced store), and K_cf in the low half of the table's 64-bit flag (its high half the
// launch's epoch); the reader re-forms the cheap slots (2/(b - a), pi/(b - a), the factors'
// constants, S0, r, T, the group) from the parameters by the same expressions.  (Round 5 sent K_cf
// in the record, one 128-byte line per table: 541 KB written per C3 request.  Sending (a, b) alone
// and re-forming the six exponentials in the reader halved the writes again but cost C3 1.3 us.)
constexpr int kAheadRec = 8;
// v of lane (lane & ~7) | l: the 8-lane group's broadcast
__device__ __forceinline__ double grp8_bcast(double v, int l) {
    const int src = ((int)__lane_id() & ~7) | l;
    const long long b = __double_as_longlong(v);
    const int lo = __shfl((int)b, src, 64);
    const int hi = __shfl((int)(b >> 32), src, 64);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ void agent_store(double* p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ double agent_load(const double* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The later table of 8-lane group lane / 8 of first-round block q0: q0 + (j + 1) R (act: it
// exists; an inactive group runs in step on q0's own table and stores nothing).  Dispatch indices:
// the table each one prices is xcd_table's
__device__ __forceinline__ int64_t ahead_table(const PriceArgs& A, int64_t q0, int64_t nblocks,
                                               int lane, bool& act) {
    const int64_t qa = q0 + (int64_t)((lane >> 3) + 1) * A.ahead_stride;
    act = qa < nblocks;
    return act ? qa : q0;
}
// The writer (a first-round block's cut wave, during the CF loop, which leaves it idle on C3's
// tables): for the tables of dispatch indices q0 + (j + 1) R, j = lane / 8, the record's 8 values
// into ahead[], then its stores drained (the flags, which carry K_cf -- returned on sub-lane 0 --
// follow the block's CF barrier)
__device__ __forceinline__ int ahead_write(const PriceArgs& A, const FusedHead& H, int64_t q0,
                                           int64_t nblocks, int lane) {
#pragma clang fp contract(off)   // table_prologue and table_prologue_wave: same bits
    const int sub = lane & 7;
    bool act;
    const int64_t qa = ahead_table(A, q0, nblocks, lane, act);
    const int64_t q = xcd_table(A, H.tpp, qa);
    const int64_t p = (int64_t)((unsigned)q / (unsigned)H.tpp);
    const int g = (int)((unsigned)q % (unsigned)H.tpp);
    const Params P = dh::load_params(H.prm + p * DH_PARAM_STRIDE);
    const double T = H.tsrc[H.paired ? p : g];
    const bool two = sub & 1;                      // factor 2 on odd sub-lanes
    const double v0 = two ? P.v02 : P.v01, k = two ? P.k2 : P.k1, th = two ? P.t2 : P.t1;
    const double sg = two ? P.s2 : P.s1, rh = two ? P.r2 : P.r1;
    double c1j, c2j;
    dh::factor_cumulants(T, P.r, v0, k, th, sg, rh, c1j, c2j);   // double_heston.py:101-118
    const double c1 = grp8_bcast(c1j, 0) + grp8_bcast(c1j, 1) + P.lam * T * P.muj;
    const double c2 = grp8_bcast(c2j, 0) + grp8_bcast(c2j, 1) +
                      P.lam * T * (P.sj * P.sj + P.muj * P.muj);
    const double h = A.L * sqrt(fabs(c2));
    const double a = c1 - h;                       // trunc_unclamped (double_heston.py:120-132)
    const double b = c1 + h;
    const int e_lane = sub < 6 ? sub : 0;
    const double arg = e_lane == 0 ? b : e_lane == 1 ? a : e_lane == 2 ? a + 0.1
                     : e_lane == 3 ? b - 0.1 : e_lane == 4 ? P.muj + 0.5 * (P.sj * P.sj)
                     : -P.r * T;
    const double e = exp(arg);
    const double comp = grp8_bcast(e, 4) - 1.0;    // cf_consts
    const double drift = (P.r - P.q - P.lam * comp) * T;
    // record value sub of the group's table: a, b, e^b, e^a, slot 25, slot 26, e^{-rT}, drift.
    // The shuffles run on every lane, outside the selection: a lane shuffle inside a branch would
    // read the branch's inactive lanes (sub-lanes 0 and 1 hold e^b and e^a)
    const double e2 = grp8_bcast(e, 2), e3 = grp8_bcast(e, 3);
    const double es = grp8_bcast(e, sub == 2 ? 0 : sub == 3 ? 1 : 5);
    double v = sub == 0 ? a : sub == 1 ? b : es;
    v = sub == 4 ? e2 * (1.0 + kClampMargin) : v;
    v = sub == 5 ? e3 * (1.0 - kClampMargin) : v;
    v = sub == 7 ? drift : v;
    if (act) agent_store(A.ahead + qa * kAheadRec + sub, v);
    // K_cf of the group's table by cf_cut_group8 on the same operands (the same first passing
    // candidate as the wave's ballot), then every store of the wave drained
    const int kcf = A.N < kCfCutMinN
                        ? A.N
                        : cf_cut_group8(P, T, a, b, tail_delta(A.tail, P.S0, b - a, A.N), A.N, sub);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return kcf;
}

// The reader (wave 0 of a later block whose flag holds this launch's epoch): the record of dispatch
// index q and table qt's cheap slots re-formed from the parameters, into c[0 .. 30) --
// table_prologue_wave's expressions on the same operands, uncontracted, so the same bits
__device__ __forceinline__ void ahead_read(const PriceArgs& A, const FusedHead& H, int64_t q,
                                           int64_t qt, double* c, int lane) {
#pragma clang fp contract(off)   // table_prologue and table_prologue_wave: same bits
    const double v = agent_load(A.ahead + q * kAheadRec + (lane & 7));
    const int64_t p = (int64_t)((unsigned)qt / (unsigned)H.tpp);
    const int g = (int)((unsigned)qt % (unsigned)H.tpp);
    const Params P = dh::load_params(H.prm + p * DH_PARAM_STRIDE);
    const double T = H.tsrc[H.paired ? p : g];
    int2 gr = make_int2((int)p, 1);
    if (!H.paired) gr = H.groups[g];
    const double a = lane_bcast(v, 0), b = lane_bcast(v, 1);
    const bool two = lane & 1;                     // factor 2 on odd lanes (table_prologue_wave)
    const dh::FactorC Fj = two ? dh::factor_consts(P.v02, P.k2, P.t2, P.s2, P.r2)
                               : dh::factor_consts(P.v01, P.k1, P.t1, P.s1, P.r1);
    const double* fj = (const double*)&Fj;
    double f1[6], f2[6];
    for (int i = 0; i < 6; ++i) {
        f1[i] = lane_bcast(fj[i], 0);
        f2[i] = lane_bcast(fj[i], 1);
    }
    if (lane == 0) {
        c[0] = a;
        c[1] = b;
        c[2] = lane_bcast(v, 2);
        c[3] = lane_bcast(v, 3);
        c[4] = 2.0 / (b - a);
        c[5] = dh::kPi / (b - a);
        for (int i = 0; i < 6; ++i) {
            c[6 + i] = f1[i];
            c[12 + i] = f2[i];
        }
        c[18] = lane_bcast(v, 7);                  // drift
        c[19] = 0.5 * (P.sj * P.sj);               // half_sj2
        c[20] = P.muj;
        c[21] = P.lam * T;                         // lt
        c[22] = P.S0;
        c[23] = P.r;
        c[24] = T;
        c[25] = lane_bcast(v, 4);
        c[26] = lane_bcast(v, 5);
        c[27] = gr.x;
        c[28] = gr.y;
        c[29] = lane_bcast(v, 6);
    }
}

// The flags, after the writer's stores drained and a barrier (every lane of a wave calls this;
// kcf: ahead_write's value, read on sub-lane 0)
__device__ __forceinline__ void ahead_publish(const PriceArgs& A, int64_t q0, int64_t nblocks,
                                              int lane, int kcf) {
    bool act;
    const int64_t qa = ahead_table(A, q0, nblocks, lane, act);
    if ((lane & 7) == 0 && act)
        __hip_atomic_store(&A.ahead_flag[qa],
                           ((unsigned long long)A.ahead_epoch << 32) | (unsigned)kcf,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The reader: this launch's record of dispatch index q is in ahead[] (a wave-uniform answer), with
// its K_cf
__device__ __forceinline__ bool ahead_ready(const PriceArgs& A, int64_t q, int& kcf) {
    const unsigned long long f = __hip_atomic_load(&A.ahead_flag[q], __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(f >> 32));
    kcf = (int)__builtin_amdgcn_readfirstlane((unsigned)f);
    return hi == A.ahead_epoch;
}


// Every table's prologue of a large fused request ahead of the fused launch (launch_fused): the
// fused blocks then load their constants instead of running the one-wave prologue chain while
// their other waves wait at the barrier.  A group of kPreLanes lanes per table: each runs
// table_prologue's chain (the bits of every other path), then the CF-cut candidates are tested
// 8 at a time (cf_cut_group8) instead of one after another (C4 at N = 256: ~30 candidates).
__global__ __launch_bounds__(kBlock) void table_prologue_kernel(PriceArgs A, int64_t n_q,
                                                                double* out) {
    if (halted(A)) return;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t q = gid / kPreLanes;
    const int sub = (int)(gid % kPreLanes);
    if (q >= n_q) return;                                      // whole groups (kBlock % 8 == 0)
#if DH_PRE_GROUP8
    // the chain spread over the group as in ahead_write: the two factors' cumulants on sub-lanes 0
    // and 1, the six exponentials one per sub-lane, shuffled to the group -- table_prologue's
    // expressions on the same operands, uncontracted, so the same bits
  {
#pragma clang fp contract(off)
    const int tpp = tabs_per_p(A);
    const int64_t p = A.p0 + q / tpp;
    const int g = (int)(q % tpp);
    const Params P = dh::load_params(A.prm + p * DH_PARAM_STRIDE);
    const double T = A.paired ? A.T[p] : A.group_T[g];
    int2 gr = make_int2((int)p, 1);
    if (!A.paired) gr = A.groups[g];
    const bool two = sub & 1;
    const double v0 = two ? P.v02 : P.v01, k = two ? P.k2 : P.k1, th = two ? P.t2 : P.t1;
    const double sg = two ? P.s2 : P.s1, rh = two ? P.r2 : P.r1;
    double c1j, c2j;
    dh::factor_cumulants(T, P.r, v0, k, th, sg, rh, c1j, c2j);   // double_heston.py:101-118
    const double c1 = grp8_bcast(c1j, 0) + grp8_bcast(c1j, 1) + P.lam * T * P.muj;
    const double c2 = grp8_bcast(c2j, 0) + grp8_bcast(c2j, 1) +
                      P.lam * T * (P.sj * P.sj + P.muj * P.muj);
    const double h = A.L * sqrt(fabs(c2));
    const double a = c1 - h;                       // trunc_unclamped (double_heston.py:120-132)
    const double b = c1 + h;
    const int e_lane = sub < 6 ? sub : 0;
    const double arg = e_lane == 0 ? b : e_lane == 1 ? a : e_lane == 2 ? a + 0.1
                     : e_lane == 3 ? b - 0.1 : e_lane == 4 ? P.muj + 0.5 * (P.sj * P.sj)
                     : -P.r * T;
    const double e = exp(arg);
    const double eb = grp8_bcast(e, 0), ea = grp8_bcast(e, 1), e2 = grp8_bcast(e, 2);
    const double e3 = grp8_bcast(e, 3), e4 = grp8_bcast(e, 4), e5 = grp8_bcast(e, 5);
    const int kcf = cf_cut_group8(P, T, a, b, tail_delta(A.tail, P.S0, b - a, A.N), A.N, sub);
    if (sub == 0) {
        const dh::FactorC F1 = dh::factor_consts(P.v01, P.k1, P.t1, P.s1, P.r1);
        const dh::FactorC F2 = dh::factor_consts(P.v02, P.k2, P.t2, P.s2, P.r2);
        const double comp = e4 - 1.0;              // cf_consts
        double* o = out + q * kTabC;
        o[0] = a;
        o[1] = b;
        o[2] = eb;
        o[3] = ea;
        o[4] = 2.0 / (b - a);
        o[5] = dh::kPi / (b - a);
        const double* f1 = (const double*)&F1;
        const double* f2 = (const double*)&F2;
        for (int i = 0; i < 6; ++i) {
            o[6 + i] = f1[i];
            o[12 + i] = f2[i];
        }
        o[18] = (P.r - P.q - P.lam * comp) * T;    // drift
        o[19] = 0.5 * (P.sj * P.sj);               // half_sj2
        o[20] = P.muj;
        o[21] = P.lam * T;                         // lt
        o[22] = P.S0;
        o[23] = P.r;
        o[24] = T;
        o[25] = e2 * (1.0 + kClampMargin);
        o[26] = e3 * (1.0 - kClampMargin);
        o[27] = gr.x;
        o[28] = gr.y;
        o[29] = e5;
        o[30] = kcf;
    }
  }
#else
    double c[kTabC];
    table_prologue(A, q, c, false);
    const int tpp = tabs_per_p(A);
    const int64_t p = A.p0 + q / tpp;
    const Params P = dh::load_params(A.prm + p * DH_PARAM_STRIDE);
    c[30] = cf_cut_group8(P, c[24], c[0], c[1], tail_delta(A.tail, c[22], c[1] - c[0], A.N), A.N,
                          sub);
    if (sub == 0) {
        double* o = out + q * kTabC;
        for (int i = 0; i < kTabC; ++i) o[i] = c[i];
    }
#endif
}

#ifndef DH_TABLE_WAVES
#define DH_TABLE_WAVES 3    // min waves per SIMD: caps VGPR+AGPR at 168 (3 waves per SIMD)
#endif
#ifndef DH_OPTION_WAVES
#define DH_OPTION_WAVES 1
#endif
#ifndef DH_FUSED_WAVES
#define DH_FUSED_WAVES 4    // caps VGPR+AGPR at 128 (4 waves per SIMD)
#endif
#ifndef DH_FUSED_WAVES_WIDE
#define DH_FUSED_WAVES_WIDE 5   // the one-option-per-lane-group variant for large grids (<= 96 VGPRs)
#endif
#ifndef DH_PRIO
#define DH_PRIO 1
#endif
// Wave priority on a block's serial phases (the prologue, the k-sums, the loss hand-off): the
// waves the rest of the block waits for at a barrier issue ahead of the other resident blocks'
// waves on their SIMD, whose CF and option sums fill the slots they leave.  Scheduling only:
// the same instructions, so the same bits.
__device__ __forceinline__ void serial_prio(bool on) {
    if constexpr (DH_PRIO > 0) {
        if (on) __builtin_amdgcn_s_setprio(DH_PRIO);
        else __builtin_amdgcn_s_setprio(0);
    }
}


// CF entries of one table slot (thread t of TPT): k = t, t + TPT, ..., emitted in increasing k
// (the k-sums' order) as emit(k, u_k, w_k).
template <int TPT, typename F>
__device__ __forceinline__ void table_entries(const dh::CfConsts& CC, int t, int N, double piba,
                                              double T, double a, double scale,
                                              const double2* sct, F&& emit) {
    for (int k = t; k < N; k += TPT) {
        const double u = k * piba;                                   // k pi / (b - a)
        emit(k, u, dh::cf_phase_re(CC, u, T, a, sct) * scale);
    }
}

// Grid: a fixed number of blocks (resident capacity), each owning a contiguous range of tables.
// Tables are taken in batches of up to kBatch: lane i of wave 0 computes the truncation range and
// CF constants of table i of the batch (one prologue latency for up to 64 tables), then every
// table slot (TPT threads) runs the CF loops of its tables back to back; per-table sums are
// finished in a fixed order at the end of the batch (bitwise independent of the grid).
constexpr int kBatch = 64;

// Slots of TPT = 64 form the per-table k-sums in registers, in the canonical order (lane l of the
// slot accumulates k = l, l + 64, ... then an xor butterfly); wider slots (fewer, fatter work
// units when a request has few tables per slot) store T2_k in LDS and let the slot's first wave
// re-form the same sums in the same order, so every slot width gives the same bits.
template <int TPT>
__global__ __launch_bounds__(kBlock, DH_TABLE_WAVES) void cos_table_kernel(PriceArgs A_) {
    const PriceArgs& A = karg_ref<PriceArgs, 0>();   // read in place (karg_ref)
    if (halted(A)) return;
    constexpr int kTabs = kBlock / TPT;      // table slots per block
    extern __shared__ __attribute__((aligned(16))) double t2s[];   // TPT > 64: [kTabs][N] T2_k
    __shared__ double shc[kBatch][kTabC];
    __shared__ double red[kBatch][4];
    __shared__ double w0s[kTabs];
    __shared__ double2 sct[dh::kMathTab];
    dh::load_sincos_table(sct);           // synchronised by the first batch's barrier
    const int slot = __builtin_amdgcn_readfirstlane(threadIdx.x / TPT);
    const int t = threadIdx.x % TPT;
    const int lane = threadIdx.x & 63;
    const int wv = t >> 6;
    const int N = A.N;
    const int tpp = tabs_per_p(A);
    const int64_t n_q = A.np * tpp;
    const int64_t q_begin = n_q * blockIdx.x / gridDim.x;
    const int64_t q_end = n_q * (blockIdx.x + 1) / gridDim.x;
    DH_STAMP(A, 4);

    for (int64_t b0 = q_begin; b0 < q_end; b0 += kBatch) {
        const int nb = (int)min<int64_t>(kBatch, q_end - b0);
        // ---- prologue, one lane per table: truncation range and CF constants ----
        if (threadIdx.x < nb) table_prologue(A, b0 + threadIdx.x, shc[threadIdx.x]);
        __syncthreads();
        if (b0 == q_begin) DH_STAMP(A, 5);

        for (int i0 = 0; i0 < nb; i0 += kTabs) {        // every thread runs every pass (barriers)
            const int i = i0 + slot;
            const bool has = i < nb;
            const int64_t q = b0 + i;
            const double* c = shc[has ? i : 0];
            const double a = c[0], b = c[1], eb = c[2], ea = c[3], scale = c[4], piba = c[5];
            const double S0 = c[22], T = c[24], lo = c[25], hi = c[26];
            const int g0 = (int)c[27], gn = has ? (int)c[28] : 0;
            const int kcf = (int)c[30];                  // CF entries k < K_cf (cf_cut_scan)
            double* t2 = t2s + (TPT > 64 ? slot * N : 0);
            double c0 = 0.0, c5 = 0.0, w0 = 0.0;
            const double delta = tail_delta(A.tail, S0, b - a, N);
            int ne = 0;
            if (has) {
                dh::CfConsts CC;
                {
                    double* cc = (double*)&CC;
                    for (int j = 0; j < 16; ++j) cc[j] = c[6 + j];
                }
                double* tw = table_w(A, q);
                const int ts = table_step(A);
                table_entries<TPT>(CC, t, kcf, piba, T, a, scale, sct, [&](int k, double u, double w) {
                    tw[k * ts] = w;
                    if (k == 0) {
                        w0 = 0.5 * w;
                        return;
                    }
                    // chi_k / psi_k at d = b: u (b - a) = k pi, so cos = (-1)^k and sin = 0
                    // exactly (the reference evaluates them with ~1e-16 rounding noise; c1 =
                    // sum T4 sin(.) is therefore 0 and kept only for the consts layout)
                    const double cb = (k & 1) ? -1.0 : 1.0;
                    const double T2 = w * S0 * dh::drcp(1.0 + u * u);
                    if (TPT == 64) {
                        c0 += T2 * eb * cb;
                        c5 += T2 * ea;
                        ne = max(ne, tail_keep(k, T2, delta));
                    } else {
                        t2[k] = T2;
                    }
                });
            }
            if (TPT > 64) {
                if (has && t == 0) w0s[slot] = w0;
                __syncthreads();
                if (has && wv == 0) {                          // the canonical 64-lane order
                    w0 = lane == 0 ? w0s[slot] : 0.0;
                    for (int k = lane; k < kcf; k += 64) {
                        if (k == 0) continue;
                        const double T2 = t2[k];
                        const double cb = (k & 1) ? -1.0 : 1.0;
                        c0 += T2 * eb * cb;
                        c5 += T2 * ea;
                        ne = max(ne, tail_keep(k, T2, delta));
                    }
                }
            }
            if (has && wv == 0) {
                // w0 has one nonzero term (lane 0's): its butterfly would change no bit.  The
                // consts' second slot (c1, a sum of zeros) carries n_eff
                c0 = xor_sum(c0, 64);
                c5 = xor_sum(c5, 64);
                ne = xor_max_i(ne, 64);
                if (lane == 0) {
                    red[i][0] = c0;
                    red[i][1] = (double)ne;
                    red[i][2] = c5;
                    red[i][3] = w0;
                }
            }

            // ---- clamp-widened options of this table's group (double_heston.py:135-137) ----
            // 64 options per wave step: a ballot of the clamp test, then the wave prices each
            // clamped option on its own range [min(a, xK - 0.1), max(b, xK + 0.1)] (lanes over
            // k).  Mask words are written for every option, prices only for clamped ones; the
            // option kernel trusts these bits, so the two kernels never disagree on a decision.
            const int64_t slot0 = q * (int64_t)A.max_group;
            for (int base = wv * 64; base < gn; base += TPT) {
                const int o = base + lane;
                bool cl = false;
                double xK = 0.0, K = 0.0;
                if (o < gn) {
                    K = option_strike(A, g0 + o, S0);
                    const double rq = K / S0;
                    if (!(rq >= lo && rq <= hi)) {                   // near or past an edge
                        double ratio;
                        xK = option_logk(K, S0, ratio);
                        cl = xK - 0.1 < a || xK + 0.1 > b;
                    }
                }
                unsigned long long mask = __ballot(cl);
                if (lane == 0) A.cl_mask[q * cl_words(A) + base / 64] = mask;
                if (mask == 0) continue;
                const int64_t p = A.p0 + q / tpp;
                const Params P = dh::load_params(A.prm + p * DH_PARAM_STRIDE);
                const double disc = exp(-P.r * T);
                while (mask) {
                    const int l = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const double x = __shfl(xK, l, 64);
                    const double Kl = __shfl(K, l, 64);
                    const int m = g0 + base + l;
                    const double ac = (x - 0.1 < a) ? x - 0.1 : a;      // Python min/max
                    const double bc = (x + 0.1 > b) ? x + 0.1 : b;
                    double v = clamped_term_sum(P, T, Kl, x, ac, bc, A.call[m] != 0, lane, 64, N,
                                                sct);
                    v = xor_sum(v, 64);
                    if (lane == 0) A.cl_price[slot0 + base + l] = disc * v;
                }
            }
            if (TPT > 64) __syncthreads();                     // t2s / w0s are reused
        }
        __syncthreads();
        if (b0 == q_begin) DH_STAMP(A, 6);
        // ---- fixed-order per-table sums of the batch ----
        if (threadIdx.x < nb) {
            const int i = threadIdx.x;
            double sm[4] = {0.0, 0.0, 0.0, 0.0};
            for (int j = 0; j < 4; ++j) sm[j] += red[i][j];
            const double* c = shc[i];
            double* cs = A.consts + (b0 + i) * kConsts;
            cs[0] = sm[0];
            cs[1] = sm[1];
            cs[2] = sm[2];
            cs[3] = sm[3];
            cs[4] = c[0];
            cs[5] = c[1];
            cs[6] = c[2];
            cs[7] = c[3];
        }
        __syncthreads();
    }
    DH_STAMP(A, 7);
}

// ----------------------------------------------------------------------------------------------
// option kernel helpers
// ----------------------------------------------------------------------------------------------
struct Consts {
    double c0, ne, c5, w0, a, b, eb, ea;   // ne: the table's n_eff (tail_keep), as a double
};


// sum' of one option from the table constants and its angle sum (k = 0 term:
// chi_0 = e^d - e^c, psi_0 = d - c, double_heston.py:142-143,154-155).
__device__ __forceinline__ double option_sum(const Consts& C, bool is_call, double S0, double K,
                                             double xK, double exK, double sum) {
    const double v0 = is_call ? (S0 * (C.eb - exK) - K * (C.b - xK))
                              : (K * (xK - C.a) - S0 * (exK - C.ea));
    const double cst = is_call ? C.c0 : C.c5;      // (the call's - K c1 term: c1 == 0 exactly)
    return cst + C.w0 * v0 - exK * sum;
}

// Angle sums of up to kR options on lanes k = k1, k1 + G, ...:
//   s_j = sum_k T2_k cos(k th_j) + T6_k sin(k th_j)
// cos/sin(k th_j) follow the Chebyshev recurrence x_{k+G} = 2 cos(G th_j) x_k - x_{k-G} (two FMAs
// per option-term; cg, sg = cos/sin(G th_j) staged once per option), re-anchored by an exact sincos
// every kAnchor steps: a rounding error introduced n steps before an anchor is amplified by at
// most n, so every cos/sin is within ~kAnchor^2 eps / 2 ~ 2e-13 of exact.  One (T2, T6)
// ds_read_b128 serves all kR options.
// Table reads run ahead of the arithmetic through a per-lane pointer and are not clamped to the
// table: an entry read past the end is never used, and an LDS read cannot fault (past the
// workgroup's allocation it returns 0), so each read is one ds_read_b128 at an immediate or
// uniform offset with no index arithmetic.
//
// One option per lane group (tile_r == 1): a lane's steps carry only this option's FMAs, so the
// cos and sin halves accumulate apart (two independent chains, summed at the end) and the table
// entries are read four steps ahead: each step's chain is one FMA deep and no LDS latency sits
// between steps.
__device__ __forceinline__ double angle_sum_1(int k1, int G, int N, double dx, double cg,
                                              double sg, double piba, const double2* t26,
                                              const double2* sct) {
    double sc = 0.0, ss = 0.0;
    const double c2 = 2.0 * cg;
    for (int k0 = k1; k0 < N; k0 += kAnchor * G) {
        double cx, sx;
        dh::dsincos_t(k0 * piba * dx, sct, &sx, &cx);          // u_k0 as the table's u
        double cp = cx * cg + sx * sg;                  // cos((k - G) th)
        double sp = sx * cg - cx * sg;                  // sin((k - G) th)
        const int kend = min(N, k0 + kAnchor * G);
        int k = k0;
        const double2* tq = t26 + k;
        double2 t0 = tq[0], t1 = tq[G], t2 = tq[2 * G], t3 = tq[3 * G];
        for (; k + 3 * G < kend; k += 4 * G) {
            tq += 4 * G;
            const double2 n0 = tq[0], n1 = tq[G], n2 = tq[2 * G], n3 = tq[3 * G];
            sc = fma(t0.x, cx, sc);                     // step k: x_{k+G} into (cp, sp)
            ss = fma(t0.y, sx, ss);
            cp = fma(c2, cx, -cp);
            sp = fma(c2, sx, -sp);
            sc = fma(t1.x, cp, sc);                     // step k + G: x_{k+2G} into (cx, sx)
            ss = fma(t1.y, sp, ss);
            cx = fma(c2, cp, -cx);
            sx = fma(c2, sp, -sx);
            sc = fma(t2.x, cx, sc);                     // step k + 2G
            ss = fma(t2.y, sx, ss);
            cp = fma(c2, cx, -cp);
            sp = fma(c2, sx, -sp);
            sc = fma(t3.x, cp, sc);                     // step k + 3G
            ss = fma(t3.y, sp, ss);
            cx = fma(c2, cp, -cx);
            sx = fma(c2, sp, -sx);
            t0 = n0;
            t1 = n1;
            t2 = n2;
            t3 = n3;
        }
        for (; k < kend; k += G) {                      // the last < 4 steps
            sc = fma(t0.x, cx, sc);
            ss = fma(t0.y, sx, ss);
            const double nc = fma(c2, cx, -cp), ns = fma(c2, sx, -sp);
            cp = cx;
            sp = sx;
            cx = nc;
            sx = ns;
            t0 = t1;
            t1 = t2;
            t2 = t3;
        }
    }
    return sc + ss;
}

template <int RR>
__device__ __forceinline__ void angle_sums_r(int k1, int G, int N, const double (&dx)[RR],
                                             const double (&cg)[RR], const double (&sg)[RR],
                                             double piba, const double2* t26,
                                             const double2* sct, double (&sum)[RR]) {
    if constexpr (RR == 1) {
        sum[0] = angle_sum_1(k1, G, N, dx[0], cg[0], sg[0], piba, t26, sct);
        return;
    }
#pragma unroll
    for (int j = 0; j < RR; ++j) sum[j] = 0.0;
    double c2[RR];
#pragma unroll
    for (int j = 0; j < RR; ++j) c2[j] = 2.0 * cg[j];
    // segments of kAnchor steps, each opened by an exact (k, k - G) pair; inside a segment four
    // steps per iteration (then at most one pair and one single step), so x_k and x_{k-G} swap
    // registers instead of being copied, with the table entries read ahead of the arithmetic
    for (int k0 = k1; k0 < N; k0 += kAnchor * G) {
        double cx[RR], sx[RR], cp[RR], sp[RR];
        const double uk = k0 * piba;                 // u_k0, the table's expression
#pragma unroll
        for (int j = 0; j < RR; ++j) {
            dh::dsincos_t(uk * dx[j], sct, &sx[j], &cx[j]);
            cp[j] = cx[j] * cg[j] + sx[j] * sg[j];              // cos((k - G) th)
            sp[j] = sx[j] * cg[j] - cx[j] * sg[j];              // sin((k - G) th)
        }
        const int kend = min(N, k0 + kAnchor * G);
        int k = k0;
        const double2* tq = t26 + k;
        double2 ta = tq[0], tb = tq[G];
        auto step = [&](const double2& t, double (&x)[RR], double (&y)[RR], double (&xp)[RR],
                        double (&yp)[RR]) {         // x_{k+G} into (xp, yp)
#pragma unroll
            for (int j = 0; j < RR; ++j) {
                sum[j] = fma(t.x, x[j], sum[j]);
                sum[j] = fma(t.y, y[j], sum[j]);
                xp[j] = fma(c2[j], x[j], -xp[j]);
                yp[j] = fma(c2[j], y[j], -yp[j]);
            }
        };
        for (; k + 3 * G < kend; k += 4 * G) {
            const double2 tc = tq[2 * G], td = tq[3 * G];
            tq += 4 * G;
            step(ta, cx, sx, cp, sp);
            step(tb, cp, sp, cx, sx);
            ta = tq[0];
            tb = tq[G];
            step(tc, cx, sx, cp, sp);
            step(td, cp, sp, cx, sx);
        }
        if (k + G < kend) {
            step(ta, cx, sx, cp, sp);
            step(tb, cp, sp, cx, sx);
            k += 2 * G;
            ta = tq[2 * G];
        }
        if (k < kend) {
#pragma unroll
            for (int j = 0; j < RR; ++j) {
                sum[j] = fma(ta.x, cx[j], sum[j]);
                sum[j] = fma(ta.y, sx[j], sum[j]);
            }
        }
    }
}

__device__ __forceinline__ void record_price(const PriceArgs& A, int64_t p, int col, double mk,
                                             int oi, double price, double* lsse, double* lbad) {
    if (A.out) A.out[p * A.out_stride + col] = price;
    if (A.part_sse) {
        const double rel = (price - mk) / mk;
        lsse[oi] = rel * rel;
        // lbfgs_calibrator.py:152: NaN, inf or <= 0 is invalid
        lbad[oi] = (isnan(price) || isinf(price) || price <= 0.0) ? 1.0 : 0.0;
    }
}

// Loss pairs handed over inside a fused launch (partials_only == 3): the guide's data-tagged
// granule form (cdna_hip_programming.md, Guideline 16 R2; MI355X_MICROARCH.md "valid forms"):
// every byte of a granule goes out in one aligned write-through (sc1) store that carries the
// launch's epoch, and every read of it is an sc1 load, re-read until the tag matches -- no flag,
// no fence, no drain.  Granule 0 of a task: epoch << 32 | low word of the
// partial; granule 1: (epoch << 9 | invalid count) << 32 | high word.  The epoch is never 0 and
// the buffer is zeroed when allocated, so a granule from another launch never matches.
constexpr int kGranCountBits = 9;           // invalid count of a tile: <= kTileMax = 256
__device__ __forceinline__ unsigned long long gran_load(const unsigned long long* g) {
    return __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// A task's two granules in ONE 16-byte write-through store (buffer_store_dwordx4 with sc1: aux 16,
// cdna_hip_programming.md Guideline 16 R1's store form), one fabric write instead of two; each
// 8-byte half still carries its own tag, so a torn pair is seen as not yet written.  g: uniform.
typedef unsigned int dh_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void gran_store2(unsigned long long* g, unsigned long long v0,
                                            unsigned long long v1) {
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(g, 0, 16, 0x00020000);
    const dh_u32x4 d = {(unsigned)v0, (unsigned)(v0 >> 32), (unsigned)v1, (unsigned)(v1 >> 32)};
    __builtin_amdgcn_raw_buffer_store_b128(d, rsrc, 0, 0, 16);
}

// The final sse / n_bad of param set p (lane 0 of the summing wave).  Into mapped host memory
// (host_out) they go as system-scope stores and the wave waits for their acknowledgement before it
// ends, so they are complete before the kernel's end-of-dispatch signal, whichever release scope
// the runtime gives that signal (the slot's event may be the launch's own stop event,
// hipExtLaunchKernel, whose release scope HIP does not document).
#ifndef DH_HOST_OUT_DRAIN
#define DH_HOST_OUT_DRAIN 1
#endif
__device__ __forceinline__ void loss_out(const PriceArgs& A, int64_t p, double sse, int nb) {
    if (DH_HOST_OUT_DRAIN && A.host_out) {
        __hip_atomic_store(&A.sse[p], sse, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&A.n_bad[p], nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        A.sse[p] = sse;
        A.n_bad[p] = nb;
    }
}

// The loss sums of param set pc by one wave of one of the grid's last P blocks (dispatch order),
// after its own task's granules went out: every lane sweeps its tiles' granules until all carry
// this launch's epoch (the producers are earlier-dispatched blocks, or blocks of the last round
// running beside it; at most P waiting blocks of a grid larger than one round of resident ones,
// so every producer still gets a slot), then the partials are summed in loss_partials_kernel's
// order and butterfly (same bits as the hand-off's last task).  The sweep is bounded: a timeout
// (never seen; some 10^8 cycles) leaves n_bad[pc] = -1.
__device__ __forceinline__ void tail_sums(const PriceArgs& A, int64_t pc, int t) {
    const int64_t base = pc * A.n_tiles;
    const unsigned ep = A.ahead_epoch;
    const unsigned ep_hi = ep << kGranCountBits;
    const unsigned cmask = (1u << kGranCountBits) - 1u;
    double acc = 0.0, bad = 0.0;
    bool timed_out = false;
    for (int j0 = 0; j0 < A.n_tiles; j0 += 64) {
        const int j = j0 + t;
        unsigned long long g0 = 0, g1 = 0;
        bool ok = j >= A.n_tiles;
        for (unsigned spins = 0;; ++spins) {
            if (!ok) {
                g0 = gran_load(A.gran + 2 * (base + j));
                g1 = gran_load(A.gran + 2 * (base + j) + 1);
                ok = (unsigned)(g0 >> 32) == ep && ((unsigned)(g1 >> 32) & ~cmask) == (ep_hi & ~cmask);
            }
            if (__all(ok)) break;
            if (spins > (1u << 20)) {
                timed_out = true;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
        if (j < A.n_tiles) {
            acc += __longlong_as_double((long long)((g1 << 32) | (g0 & 0xffffffffull)));
            bad += (double)((unsigned)(g1 >> 32) & cmask);
        }
    }
    acc = xor_sum(acc, 64);
    bad = xor_sum(bad, 64);
    if (t == 0) loss_out(A, pc, acc, timed_out ? -1 : (int)bad);
}

// Fixed-order loss partial of one task (wave 0 of the task).  Hand-off to the last task of param
// set p without fences (MI355X_MICROARCH.md, "Valid forms", first table row): one lane writes
// the partial with agent-scope (sc1, write-through) stores, drains them with s_waitcnt vmcnt(0),
// then adds to p's counter; in the wave whose add returns n_tiles - 1 every lane reads partials
// of p with sc1 loads, the wave sums them in a fixed order and resets the counter.
__device__ __forceinline__ void task_loss(const PriceArgs& A, int64_t p, int64_t task, int nopt,
                                          int t, const double* lsse, const double* lbad) {
    DH_STAMP(A, 13);
    double s = 0.0;
    int nb = 0;                     // invalid prices: a count (0/1 flags), so a ballot suffices
    for (int i0 = 0; i0 < nopt; i0 += 64) {
        const int i = i0 + t;
        if (i < nopt) s += lsse[i];
        nb += __popcll(__ballot(i < nopt && lbad[i] != 0.0));
    }
    // lanes >= nopt hold +0.0 and only lane 0's sum is used, so levels with off >= nopt would add
    // +0.0 to it (an exact no-op on a sum of squares): skip them (C2's 32 options: 5 levels)
    const int lvl = nopt < 64 ? nopt : 64;
    int width = 1;
    while (width < lvl) width <<= 1;
    s = xor_sum(s, width);
    const double f = nb;
    DH_STAMP(A, 14);
    const int64_t base_i = p * A.n_tiles;
    if (A.partials_only == 3) {     // the pair as two epoch-tagged 8-byte granules, write-through
        // (agent-scope) stores with no drain: each granule is its own flag (tail_sums)
        if (t == 0) {
            const unsigned long long sb = (unsigned long long)__double_as_longlong(s);
            const unsigned ep = A.ahead_epoch;
            const unsigned long long g0 = ((unsigned long long)ep << 32) | (unsigned)sb;
            const unsigned long long g1 =
                ((unsigned long long)((ep << kGranCountBits) | (unsigned)nb) << 32) | (unsigned)(sb >> 32);
            gran_store2(A.gran + 2 * task, g0, g1);
        }
        return;
    }
    if (A.partials_only == 2) {     // one plain 16-byte store (one line write per block):
        // loss_partials_kernel reads the (partial, invalid count) pairs next
        if (t == 0) reinterpret_cast<double2*>(A.part_sse)[task] = make_double2(s, f);
        return;
    }
    if (A.partials_only) {          // plain stores: the next launch (the step kernel) reads them;
        // the tile's invalid flag rides in the sign bit (a valid partial is a sum of squares: +0,
        // positive, +inf or NaN, canonicalised to + here), so the step kernel reads one array
        if (t == 0) A.part_sse[task] = f > 0.0 ? -fabs(s) : fabs(s);
        return;
    }
    unsigned old = 0;
    if (t == 0) {
        __hip_atomic_store(&A.part_sse[task], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.part_bad[task], (int)f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        DH_STAMP(A, 15);
        old = __hip_atomic_fetch_add(&A.counter[p * kCounterStride], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    old = __builtin_amdgcn_readlane(old, 0);       // lane 0's ticket (no LDS round trip)
    DH_STAMP(A, 12);
    if (old != (unsigned)A.n_tiles - 1u) return;
    double acc = 0.0, bad = 0.0;
    for (int j = t; j < A.n_tiles; j += 64) {
        acc += __hip_atomic_load(&A.part_sse[base_i + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bad += __hip_atomic_load(&A.part_bad[base_i + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    acc = xor_sum(acc, 64);
    bad = xor_sum(bad, 64);
    if (t == 0) {
        loss_out(A, p, acc, (int)bad);
        __hip_atomic_store(&A.counter[p * kCounterStride], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The hand-off's last task, as its own launch after a partials_only == 2 request (one 64-lane
// block per param set): the same reads in the same order and the same butterfly, so the same bits
// as task_loss.  A multi-round fused grid's blocks then end with plain stores instead of the
// agent-scope store drain and the ticket atomic (~1.8k cycles of every block's chain).
__global__ __launch_bounds__(64) void loss_partials_kernel(const double2* __restrict__ part,
                                                           int n_tiles, double* sse, int* n_bad) {
    const int64_t p = blockIdx.x;
    const int t = threadIdx.x;
    const int64_t base_i = p * n_tiles;
    double acc = 0.0, bad = 0.0;
    for (int j = t; j < n_tiles; j += 64) {
        const double2 v = part[base_i + j];
        acc += v.x;
        bad += v.y;
    }
    acc = xor_sum(acc, 64);
    bad = xor_sum(bad, 64);
    if (t == 0) {
        sse[p] = acc;
        n_bad[p] = (int)bad;
    }
}

__host__ __device__ constexpr int option_lds_doubles(int N, int opt_cap) {
    // (T2,T6)[N] | K, mkt, sse, bad, xK, e^xK, cos/sin step [opt_cap] | call, perm [opt_cap]
    // ints, rounded to whole 16-byte pairs (u_k = k pi/(b - a) is re-formed where needed)
    return 2 * N + 8 * opt_cap + ((2 * opt_cap + 3) / 4) * 2;
}

// LDS view of one staged tile: the expanded (p, g) table and the per-option arrays
struct TileLds {
    double2* t26;     // (T2_k, T6_k)
    double* K;
    double* mkt;
    double* sse;
    double* bad;
    double* xK;       // log(K / S0)
    double* exK;      // e^{log(K / S0)}
    double* cs;       // cos / sin of the G-step rotation (sin = NaN marks a clamped option)
    double* ss;
    int* call;
    int* perm;
};

__device__ __forceinline__ TileLds tile_lds(double* base, int N, int cap) {
    TileLds L;
    L.t26 = (double2*)base;
    L.K = base + 2 * N;
    L.mkt = L.K + cap;
    L.sse = L.mkt + cap;
    L.bad = L.sse + cap;
    L.xK = L.bad + cap;
    L.exK = L.xK + cap;
    L.cs = L.exK + cap;
    L.ss = L.cs + cap;
    L.call = (int*)(L.ss + cap);
    L.perm = L.call + cap;
    return L;
}

// Options per lane group of a launch whose largest tile has max_nopt options priced by tpt
// threads: kR (one table read serves kR options) unless that tile leaves >= 8 lanes per option,
// where one option per group gives each lane one anchor sincos instead of kR and a butterfly over
// one sum instead of kR (the latency path of small calibration tiles: C2's 32-option tiles, C1's
// 5).  A property of the surface and N, never of the batch: every path and batch composition
// prices a tile with the same lanes.  The request kernels are instantiated per value.
inline int tile_r(int max_nopt, int tpt) { return tpt >= 8 * std::max(max_nopt, 1) ? 1 : kR; }

// lanes per group of RT options for a tile of nopt options priced by tpt threads
// A block-wide tile (tpt == kBlock) with kR options per group takes any G (its partials are
// reduced through LDS, e.g. G = 10 for 100-option tiles: 250 of 256 lanes busy instead of 200 with
// G = 8); other tiles keep a power of two <= 64 for the in-wave butterfly.
// IDX: the index arithmetic of dh_index.h in place of `/` and `%` (the same values; the 4-wave
// fused builds, where it pays: DESIGN 3.4).
template <int RT, bool IDX = false>
__device__ __forceinline__ int group_lanes(int nopt, int N, int tpt) {
    const int R = min(RT, max(nopt, 1));
    const int ngroups = IDX ? dh_idx::n_groups<RT>(nopt) : (nopt + R - 1) / R;
#ifndef DH_GMAX
#define DH_GMAX 1024
#endif
    if (tpt == kBlock && RT == kR) return max(1, min(min(tpt / ngroups, DH_GMAX), N - 1));
    int G = 1;
    while (G * 2 <= tpt / max(ngroups, 1) && G < 64) G *= 2;
    while (G > 1 && G / 2 >= N - 1) G /= 2;                 // no more lanes than terms k >= 1
    return G;
}

// Angle sums, finalisation and price / loss-term recording of one staged tile (thread t of the
// tile's tpt).  Shared by cos_option_kernel and cos_fused_kernel, so both give the same bits.
// A block-wide tile (tpt == kBlock; every thread of the block must call this) whose G is not a
// power of two <= 64 reduces each group's G lane partials through LDS (red: kR x kBlock doubles)
// in lane order; otherwise xor butterflies inside the wave.
template <int RT, bool IDX = false>
__device__ __forceinline__ void tile_sums_r(const PriceArgs& A, int64_t p, const Consts& C,
                                            double S0, double disc, int nopt, int G, int tpt,
                                            int t, bool active, const TileLds& L, double* red,
                                            const double2* sct) {
    const int Ne = (int)C.ne;                     // the table's kept terms: k < n_eff
    const int R = IDX ? dh_idx::group_r<RT>(nopt) : min(RT, max(nopt, 1));
    const int ngroups = IDX ? dh_idx::n_groups<RT>(nopt) : (nopt + R - 1) / R;
    // IDX: t / G and t % G as a 24-bit multiply by gm and a shift (t < tpt <= 256, G <= 256)
    const unsigned gm = IDX ? dh_idx::div256_magic(G) : 0u;
    const int groups_per_pass = max(1, IDX ? (int)dh_idx::div256(tpt, gm) : tpt / G);
    const bool lds_red = tpt == kBlock && (G > 64 || (G & (G - 1)) != 0);   // else butterflies
    for (int pass = 0; pass < ngroups; pass += groups_per_pass) {
        const int tg = IDX ? (int)dh_idx::div256(t, gm) : t / G;
        const int gi = pass + tg;
        const int gl = IDX ? (int)dh_idx::mod256(t, tg, G) : t % G;
        const bool gvalid = active && t < groups_per_pass * G && gi < ngroups;
        double dx[RT], cs[RT], ss[RT];
        bool use[RT];
#pragma unroll
        for (int j = 0; j < RT; ++j) {
            const int oi = gi * R + j;
            const bool in = gvalid && j < R && oi < nopt;
            const double sj = in ? L.ss[oi] : 0.0;
            use[j] = in && !isnan(sj);                               // clamped: recorded
            dx[j] = use[j] ? L.xK[oi] - C.a : 0.0;
            cs[j] = use[j] ? L.cs[oi] : 1.0;
            ss[j] = use[j] ? sj : 0.0;
        }
        double sm[RT];
        if (pass == 0) DH_STAMP(A, 9);
        angle_sums_r<RT>(1 + gl, G, Ne, dx, cs, ss, dh::kPi / (C.b - C.a), L.t26, sct, sm);
        if (pass == 0) DH_STAMP(A, 10);
        if (lds_red) {
            if (gvalid) {
                // the slot address formed here, not kept across the angle loop (held there, it was
                // the C3 build's one hot-path register spill: a scratch store and a reload per
                // thread, ~1.3 MB of scratch written back per request)
                int tr = t;
                asm volatile("" : "+v"(tr));
#pragma unroll
                for (int j = 0; j < RT; ++j) red[j * kBlock + tr] = sm[j];
            }
            __syncthreads();
            if (pass == 0) DH_STAMP(A, 11);
            // thread t finalises option pass R + t of the pass (one option per thread: the
            // pass's options on its first lanes, not on lanes gl < R of every group, so fewer
            // waves issue the finalisation): its group's G lane partials in lane order
            const int o_end = min(nopt, min(pass + groups_per_pass, ngroups) * R);
            for (int oi = pass * R + t; active && oi < o_end; oi += tpt) {
                if (!isnan(L.ss[oi])) {
                    const int j = IDX ? dh_idx::opt_slot<RT>(oi, nopt) : oi % R;
                    const int og = IDX ? dh_idx::opt_group<RT>(oi, nopt) : oi / R;
                    const double* rj = red + j * kBlock + (og - pass) * G;
                    double sum = 0.0;
                    for (int l = 0; l < G; ++l) sum += rj[l];
                    const double v = option_sum(C, L.call[oi] != 0, S0, L.K[oi], L.xK[oi],
                                                L.exK[oi], sum);
                    record_price(A, p, L.perm[oi], L.mkt[oi], oi, disc * v, L.sse, L.bad);
                }
            }
            __syncthreads();
            continue;
        }
#pragma unroll
        for (int j = 0; j < RT; ++j) sm[j] = xor_sum(sm[j], G);
        if (pass == 0) DH_STAMP(A, 11);
        // every lane of the group holds the (bitwise identical) sums: lane j finalises option j
        if (G >= R) {
            double m = sm[0];
            bool mu = use[0];
#pragma unroll
            for (int j = 1; j < RT; ++j) {
                m = gl == j ? sm[j] : m;
                mu = gl == j ? use[j] : mu;
            }
            if (gl < R && mu) {
                const int oi = gi * R + gl;
                const double sum = option_sum(C, L.call[oi] != 0, S0, L.K[oi], L.xK[oi],
                                              L.exK[oi], m);
                record_price(A, p, L.perm[oi], L.mkt[oi], oi, disc * sum, L.sse, L.bad);
            }
        } else if (gl == 0) {
#pragma unroll
            for (int j = 0; j < RT; ++j) {
                if (!use[j]) continue;
                const int oi = gi * R + j;
                const double sum = option_sum(C, L.call[oi] != 0, S0, L.K[oi], L.xK[oi],
                                              L.exK[oi], sm[j]);
                record_price(A, p, L.perm[oi], L.mkt[oi], oi, disc * sum, L.sse, L.bad);
            }
        }
    }
}

// LDS doubles of the lane partials of a block-wide tile (tile_sums' red)
constexpr int kRedDoubles = kR * kBlock;

// ----------------------------------------------------------------------------------------------
// option kernel
// ----------------------------------------------------------------------------------------------
template <int TPT, int RT>
__global__ __launch_bounds__(kBlock, DH_OPTION_WAVES) void cos_option_kernel(PriceArgs A_) {
    const PriceArgs& A = karg_ref<PriceArgs, 0>();   // read in place (karg_ref)
    if (halted(A)) return;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int kTasks = kBlock / TPT;
    const int slot = threadIdx.x / TPT;
    const int t = threadIdx.x % TPT;
    const int N = A.N;
    const int64_t n_tasks = A.paired ? A.np : A.np * (int64_t)A.n_tiles;
    // the task index is wave-uniform: make that visible so per-task values live in SGPRs
    const int64_t task_l = (int64_t)blockIdx.x * kTasks + __builtin_amdgcn_readfirstlane(slot);
    const bool active = task_l < n_tasks;
    const int64_t p = A.p0 + (active ? (A.paired ? task_l : task_l / A.n_tiles) : 0);
    const int tile = (active && !A.paired) ? (int)(task_l % A.n_tiles) : 0;
    const int64_t task = A.paired ? p : p * A.n_tiles + tile;       // global task id
    DH_STAMP(A, 0);

    const int cap = A.opt_cap;
    const TileLds L = tile_lds(smem + (size_t)slot * option_lds_doubles(N, cap), N, cap);
    double* red = smem + (size_t)kTasks * option_lds_doubles(N, cap);   // TPT == kBlock only
    __shared__ double2 sct[dh::kMathTab];
    dh::load_sincos_table(sct);                                // synchronised by the staging barrier
    double2* t26 = L.t26;
    double* lK = L.K;
    double* lmkt = L.mkt;
    double* lsse = L.sse;
    double* lbad = L.bad;
    double* lxK = L.xK;
    double* lexK = L.exK;
    double* lcs = L.cs;
    double* lss = L.ss;
    int* lcall = L.call;
    int* lperm = L.perm;

    int opt0 = 0, nopt = 0, g = 0;
    if (active) {
        if (A.paired) {
            opt0 = (int)p;
            nopt = 1;
        } else {
            const int2 tl = A.tiles[tile];
            opt0 = tl.x;
            nopt = tl.y;
            g = A.tile_group[tile];
        }
    }
    // lanes: groups of kR options on G lanes each
    const int G = group_lanes<RT>(nopt, N, TPT);

    const int64_t q = (p - A.p0) * tabs_per_p(A) + g;
    const Params P = dh::load_params(A.prm + p * DH_PARAM_STRIDE);
    Consts C{0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0};
    if (active) {
        const double* cs = A.consts + q * kConsts;
        C = Consts{cs[0], cs[1], cs[2], cs[3], cs[4], cs[5], cs[6], cs[7]};
    }
    const double ba = C.b - C.a;
    const double T = active ? A.T[opt0] : 1.0;
    const double disc = exp(-P.r * T);
    // stage the (p, g) table, expanded to u, (T2, T6) (same expressions as the table
    // kernel's k-sums), and per-option data: log(K/S0), e^{xK} and the G-step rotation of each
    // option; clamp-widened options (bit set by the table kernel) are recorded right here
    if (active) {
        const double* tw = A.table + q * (int64_t)N;     // row-major (never tiled here)
        const double piba = dh::kPi / ba;
        const int ne = (int)C.ne;                        // terms past n_eff are never read
        for (int k = t; k < ne; k += TPT) {
            const double w = tw[k];
            const double u = k * piba;
            const double T2 = k == 0 ? 0.0 : w * P.S0 * dh::drcp(1.0 + u * u);
            t26[k] = make_double2(T2, k == 0 ? 0.0 : -(T2 * dh::drcp(u)));
        }
        const double ustep = G * dh::kPi / ba;
        const int g0 = A.paired ? (int)p : A.groups[g].x;
        const unsigned long long* msk = A.cl_mask + q * cl_words(A);
        const double* clp = A.cl_price + q * (int64_t)A.max_group;
        for (int i = t; i < nopt; i += TPT) {
            const double K = option_strike(A, opt0 + i, P.S0);
            double ratio;
            const double xK = option_logk(K, P.S0, ratio);
            lK[i] = K;
            lmkt[i] = A.mkt ? A.mkt[opt0 + i] : 0.0;
            lcall[i] = A.call[opt0 + i];
            lperm[i] = A.perm[opt0 + i];
            lxK[i] = xK;
            lexK[i] = ratio;                                         // e^{xK} to an ulp
            const int gpos = opt0 + i - g0;
            const bool cl = (msk[gpos >> 6] >> (gpos & 63)) & 1ull;
            double ss, cs;
            dh::dsincos(ustep * (cl ? 0.0 : xK - C.a), &ss, &cs);
            lcs[i] = cs;
            // NaN marks clamped; a NaN sine of an unclamped option (NaN params, strike or
            // range) is stored as 0: its NaN cosine and offset still make the price NaN
            lss[i] = cl ? NAN : (ss == ss ? ss : 0.0);
            if (cl) record_price(A, p, lperm[i], lmkt[i], i, clp[gpos], lsse, lbad);
        }
    }
    __syncthreads();
    DH_STAMP(A, 1);

    tile_sums_r<RT>(A, p, C, P.S0, disc, nopt, G, TPT, t, active, L, red, sct);
    DH_STAMP(A, 2);

    // ---- loss: fixed-order per-task partial, last arriver finalises the param set ----
    if (A.part_sse) {
        __syncthreads();
        if (active && t < 64) task_loss(A, p, task, nopt, t, lsse, lbad);
    }
    DH_STAMP(A, 3);
}

// ----------------------------------------------------------------------------------------------
// option kernel, small tiles (<= kSmallTile options per tile): one lane carries RS options of a
// tile through every term k = 1 .. N-1.  Its step rotation e^{i th} is also its start angle, the
// 8-byte table w_k is read straight from L2/MALL and expanded to (T2, T6) on the fly
// (amortised over RS options), and a task's partial is reduced over its L lanes (L = lanes per
// task, a power of two <= 4) before the same fence-free hand-off.  Per lane this is ~9 VALU
// instructions per option-term with no LDS, no per-lane anchors and no butterflies -- the
// large-tile kernel's fixed costs dominate when a tile has 5-16 options (generator grids).
// ----------------------------------------------------------------------------------------------
constexpr int kSmallTile = 16;
// options per lane: 4, or 8 for tiles of more than 4 options (C5's 8-option tiles: one lane per
// tile, so the per-term expansion of w_k is not repeated on a second lane: -24% VALU per tile-term)
constexpr int small_rs(int max_nopt) { return max_nopt > 4 ? 8 : 4; }
// ...and only when a call has enough tasks to fill the chip with one lane group per task
// (below this the large-tile kernel's many lanes per option win on latency).  Calibration
// launches (14 x starts param sets) stay far below it, so lockstep == sequential bit for bit.
constexpr int64_t kSmallMinTasks = 65536;

template <int RS>
__global__ __launch_bounds__(kBlock) void cos_option_small_kernel(PriceArgs A_, int L) {
    const PriceArgs& A = karg_ref<PriceArgs, 0>();   // read in place (karg_ref)
    if (halted(A)) return;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t n_tasks = A.paired ? A.np : A.np * (int64_t)A.n_tiles;
    const int64_t task_l = gid / L;
    const int sub = (int)(gid % L);
    const bool active = task_l < n_tasks;
    const int64_t p = A.p0 + (active ? (A.paired ? task_l : task_l / A.n_tiles) : 0);
    const int tile = (active && !A.paired) ? (int)(task_l % A.n_tiles) : 0;
    const int64_t task = A.paired ? p : p * A.n_tiles + tile;
    int opt0 = 0, nopt = 0, g = 0;
    if (active) {
        if (A.paired) {
            opt0 = (int)p;
            nopt = 1;
        } else {
            const int2 tl = A.tiles[tile];
            opt0 = tl.x;
            nopt = tl.y;
            g = A.tile_group[tile];
        }
    }
    const int64_t q = (p - A.p0) * tabs_per_p(A) + g;
    const double* prm = A.prm + p * DH_PARAM_STRIDE;
    const double S0 = prm[13], r = prm[14];
    Consts C{0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0};
    if (active) {
        const double* cs = A.consts + q * kConsts;
        C = Consts{cs[0], cs[1], cs[2], cs[3], cs[4], cs[5], cs[6], cs[7]};
    }
    const double ba = C.b - C.a;
    const double piba = dh::kPi / ba;
    const double T = active ? A.T[opt0] : 1.0;
    const double disc = exp(-r * T);
    const int g0 = A.paired ? (int)p : (active ? A.groups[g].x : 0);
    const unsigned long long* msk = A.cl_mask + q * cl_words(A);
    const double* clp = A.cl_price + q * (int64_t)A.max_group;

    // per option: log-strike, clamp bit; cos/sin(k th) by the Chebyshev recurrence from
    // (k = 0, k = 1) = (1 + 0i, e^{i th})
    double dx[RS], c[RS], sn[RS], cp[RS], sp[RS], cs[RS], ss[RS], sm[RS];
    bool use[RS];
    double lsum = 0.0, lbad = 0.0;
#pragma unroll
    for (int j = 0; j < RS; ++j) {
        const int oi = sub * RS + j;
        const bool in = active && oi < nopt;
        bool cl = false;
        double xK = 0.0;
        if (in) {
            const int m = opt0 + oi;
            const double K = option_strike(A, m, S0);
            double ratio;
            xK = option_logk(K, S0, ratio);
            const int gpos = m - g0;
            cl = (msk[gpos >> 6] >> (gpos & 63)) & 1ull;
            if (cl) {                      // priced by the table kernel
                const double price = clp[gpos];
                if (A.out) A.out[p * A.out_stride + A.perm[m]] = price;
                if (A.part_sse) {
                    const double mk = A.mkt[m];
                    const double rel = (price - mk) / mk;
                    lsum += rel * rel;
                    lbad += (isnan(price) || isinf(price) || price <= 0.0) ? 1.0 : 0.0;
                }
            }
        }
        use[j] = in && !cl;
        dx[j] = use[j] ? xK - C.a : 0.0;
        double s1, c1;
        dh::dsincos(piba * dx[j], &s1, &c1);
        cs[j] = c1;
        ss[j] = s1;
        c[j] = c1;
        sn[j] = s1;
        cp[j] = 1.0;
        sp[j] = 0.0;
        sm[j] = 0.0;
    }
    // the host always tiles the tables this kernel reads: entry k at tw[k * kTabTile]
    const double* tw = A.table + (q / kTabTile) * kTabTile * (int64_t)A.N + (q % kTabTile);
    double c2[RS];
#pragma unroll
    for (int j = 0; j < RS; ++j) c2[j] = 2.0 * cs[j];
    // segments of kAnchor terms (the first starts exact at k = 1; later ones re-anchor on an
    // exact (k, k - 1) pair), two terms per iteration with x_k / x_{k-1} swapping registers
    const int N = A.N;
    const int ne = (int)C.ne;                        // the table's kept terms: k < n_eff
    for (int k0 = 1; k0 < ne; k0 += kAnchor) {
        if (k0 > 1) {
            const double uk = k0 * piba;
#pragma unroll
            for (int j = 0; j < RS; ++j) {
                dh::dsincos(uk * dx[j], &sn[j], &c[j]);
                cp[j] = c[j] * cs[j] + sn[j] * ss[j];
                sp[j] = sn[j] * cs[j] - c[j] * ss[j];
            }
        }
        const int kend = min(ne, k0 + kAnchor);
        int k = k0;
        double wa = active ? tw[k * kTabTile] : 0.0;
        for (; k + 1 < kend; k += 2) {
            const double wb = active ? tw[(k + 1) * kTabTile] : 0.0;
            const double ua = k * piba, ub = (k + 1) * piba;
            const double T2a = wa * S0 * dh::drcp(1.0 + ua * ua);
            const double T6a = -(T2a * dh::drcp(ua));
            const double T2b = wb * S0 * dh::drcp(1.0 + ub * ub);
            const double T6b = -(T2b * dh::drcp(ub));
            wa = active ? tw[min(k + 2, N - 1) * kTabTile] : 0.0;
#pragma unroll
            for (int j = 0; j < RS; ++j) {
                sm[j] = fma(T2a, c[j], sm[j]);
                sm[j] = fma(T6a, sn[j], sm[j]);
                cp[j] = fma(c2[j], c[j], -cp[j]);               // x_{k+1}
                sp[j] = fma(c2[j], sn[j], -sp[j]);
                sm[j] = fma(T2b, cp[j], sm[j]);
                sm[j] = fma(T6b, sp[j], sm[j]);
                c[j] = fma(c2[j], cp[j], -c[j]);                // x_{k+2}
                sn[j] = fma(c2[j], sp[j], -sn[j]);
            }
        }
        if (k < kend) {
            const double u = k * piba;
            const double T2 = wa * S0 * dh::drcp(1.0 + u * u);
            const double T6 = -(T2 * dh::drcp(u));
#pragma unroll
            for (int j = 0; j < RS; ++j) {
                sm[j] = fma(T2, c[j], sm[j]);
                sm[j] = fma(T6, sn[j], sm[j]);
            }
        }
    }
    // finalise this lane's options, then the task partial over its L lanes (fixed tree)
#pragma unroll
    for (int j = 0; j < RS; ++j) {
        if (!use[j]) continue;
        const int m = opt0 + sub * RS + j;
        const double K = option_strike(A, m, S0);
        double ratio;
        const double xK = option_logk(K, S0, ratio);
        const double sum = option_sum(C, A.call[m] != 0, S0, K, xK, ratio, sm[j]);
        const double price = disc * sum;
        if (A.out) A.out[p * A.out_stride + A.perm[m]] = price;
        if (A.part_sse) {
            const double mk = A.mkt[m];
            const double rel = (price - mk) / mk;
            lsum += rel * rel;
            lbad += (isnan(price) || isinf(price) || price <= 0.0) ? 1.0 : 0.0;
        }
    }
    if (!A.part_sse) return;
    lsum = xor_sum(lsum, L);
    lbad = xor_sum(lbad, L);
    if (!active || sub != 0) return;
    // fence-free hand-off (as task_loss): sc1 stores, drain, agent-scope ticket
    __hip_atomic_store(&A.part_sse[task], lsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&A.part_bad[task], (int)lbad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned old =
        __hip_atomic_fetch_add(&A.counter[p * kCounterStride], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old != (unsigned)A.n_tiles - 1u) return;
    const int64_t base_i = p * A.n_tiles;
    double acc = 0.0;
    int bad = 0;
    for (int j = 0; j < A.n_tiles; ++j) {           // tile order
        acc += __hip_atomic_load(&A.part_sse[base_i + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bad += __hip_atomic_load(&A.part_bad[base_i + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    loss_out(A, p, acc, bad);
    __hip_atomic_store(&A.counter[p * kCounterStride], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ----------------------------------------------------------------------------------------------
// fused small-tile kernel (generator grids: every maturity group one tile of <= kSmallTile
// options, >= kSmallMinTasks tasks): a persistent block takes TB tables at a time, forms their
// expanded tables (T2_k, T6_k) in LDS -- no table round trip through L2/MALL and no second
// launch -- then prices their options on lanes (table, option, k-block):
//   * prologue: one lane per table (table_prologue, the split path's constants);
//   * CF: TPT = 256 / TB threads per table, entries k = t, t + TPT, ... (cf_phase_re), each
//     stored as (T2, T6) with the table kernel's expressions; c0 / c5 / w0 summed per thread in
//     increasing k, then a TPT-lane butterfly;
//   * options: OP (a power of two >= the largest tile) option slots per table x S = TPT / OP
//     k-blocks per option: lane j of an option sums k in [1 + j L, 1 + (j + 1) L), L = ceil((N - 1)
//     / S), cos/sin(k th) by the step-th Chebyshev recurrence re-anchored by an exact sincos every
//     kAnchor terms, then an S-lane butterfly; clamp-widened options (double_heston.py:135-137)
//     are priced afterwards by the whole wave (clamped_term_sum, lanes over k);
//   * loss: per table the options' rel^2 / invalid flags summed in option order, then the
//     fence-free hand-off of the other request kernels (one task = one (p, tile)).
// Prices agree with the split / fused paths to ~1e-15 relative (another summation order), as the
// lane-per-option-group small-tile kernel's did.
// ----------------------------------------------------------------------------------------------
template <int TB>
__global__ __launch_bounds__(kBlock, 3) void cos_gen_kernel(PriceArgs A_, int OP) {
    const PriceArgs& A = karg_ref<PriceArgs, 0>();   // read in place (karg_ref)
    if (halted(A)) return;
    constexpr int TPT = kBlock / TB;                 // threads per table (CF), <= 64
    static_assert(TPT <= 64 && TPT >= kSmallTile, "one table's lanes inside one wave");
    extern __shared__ __attribute__((aligned(16))) double2 gtab[];   // [TB][N] (T2, T6)
    __shared__ double shc[TB][kTabC];
    __shared__ double ks[TB][3];                     // c0, c5, w0
    __shared__ int kne[TB];                          // n_eff (tail_keep)
    __shared__ double osse[TB][kSmallTile], obad[TB][kSmallTile];
    __shared__ double2 sct[dh::kMathTab];
    dh::load_math_tables(sct, 0);                    // synchronised by the first barrier
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int N = A.N;
    const int tpp = tabs_per_p(A);
    const int64_t n_q = A.np * tpp;
    const int S = TPT / OP;                          // k-blocks per option
    const int it = t / TPT, sub = t % TPT;           // CF phase: table slot, thread in table
    const int io = t / TPT, oo = (t % TPT) / S, jj = t % S;   // option phase: table, option, k-block
    for (int64_t b0 = (int64_t)blockIdx.x * TB; b0 < n_q; b0 += (int64_t)gridDim.x * TB) {
        const int nb = (int)min<int64_t>(TB, n_q - b0);
        if (t < 64) serial_prio(true);               // the prologue lanes' wave
        if (t < nb) table_prologue(A, b0 + t, shc[t]);
        __syncthreads();
        serial_prio(false);
        // ---- CF entries of table slot `it` into LDS ----
        if (it < nb) {
            const double* c = shc[it];
            const double a = c[0], eb = c[2], ea = c[3], scale = c[4], piba = c[5];
            const double S0 = c[22], T = c[24];
            const int kcf = (int)c[30];                  // CF entries k < K_cf (cf_cut_scan)
            dh::CfConsts CC;
            {
                double* cc = (double*)&CC;
                for (int j = 0; j < 16; ++j) cc[j] = c[6 + j];
            }
            double2* tb = gtab + (size_t)it * N;
            const double delta = tail_delta(A.tail, S0, c[1] - a, N);
            double c0 = 0.0, c5 = 0.0, w0 = 0.0;
            int ne = 0;
            table_entries<TPT>(CC, sub, kcf, piba, T, a, scale, sct, [&](int k, double u, double w) {
                if (k == 0) {
                    w0 = 0.5 * w;
                    tb[0] = make_double2(0.0, 0.0);
                    return;
                }
                const double T2 = w * S0 * dh::drcp(1.0 + u * u);
                tb[k] = make_double2(T2, -(T2 * dh::drcp(u)));
                const double cb = (k & 1) ? -1.0 : 1.0;
                c0 += T2 * eb * cb;
                c5 += T2 * ea;
                ne = max(ne, tail_keep(k, T2, delta));
            });
            c0 = xor_sum(c0, TPT);
            c5 = xor_sum(c5, TPT);
            w0 = xor_sum(w0, TPT);                   // one nonzero term (thread 0's)
            ne = xor_max_i(ne, TPT);
            if (sub == 0) {
                ks[it][0] = c0;
                ks[it][1] = c5;
                ks[it][2] = w0;
                kne[it] = ne;
            }
        }
        __syncthreads();
        // ---- options of table slot `io`: option oo, k-block jj ----
        const int64_t q = b0 + io;
        const bool tab_ok = io < nb;
        const double* c = shc[tab_ok ? io : 0];
        const double a = c[0], b = c[1], piba = c[5], S0 = c[22];
        const int g0 = (int)c[27], gn = tab_ok ? (int)c[28] : 0;
        const bool in = tab_ok && oo < gn;
        const int m = g0 + (in ? oo : 0);
        double K = 0.0, xK = 0.0, ratio = 1.0;
        if (in) {
            K = option_strike(A, m, S0);
            xK = option_logk(K, S0, ratio);
        }
        const bool cl = in && (xK - 0.1 < a || xK + 0.1 > b);
        const bool use = in && !cl;
        double sum = 0.0;
        {
            const double th = use ? piba * (xK - a) : 0.0;
            double st, ct;
            dh::dsincos_t(th, sct, &st, &ct);
            const double c2 = 2.0 * ct;
            const double2* tb = gtab + (size_t)(tab_ok ? io : 0) * N;
            // the kept terms k < n_eff in S k-blocks of Lk
            const int ne = tab_ok ? kne[io] : 0;
            const int Lk = (max(ne, 1) - 1 + S - 1) / S;
            const int k_lo = 1 + jj * Lk, k_hi = min(ne, k_lo + Lk);
            double sc = 0.0, ss = 0.0;
            for (int k0 = k_lo; k0 < k_hi; k0 += kAnchor) {
                double cx, sx;                                     // cos / sin (k0 th)
                if (k0 == 1) {
                    cx = ct;
                    sx = st;
                } else {
                    dh::dsincos_t((double)k0 * piba * (xK - a), sct, &sx, &cx);
                }
                double cp = cx * ct + sx * st;                     // cos / sin ((k0 - 1) th)
                double sp = sx * ct - cx * st;
                // four steps per iteration with the entries read four ahead (immediate LDS
                // offsets), x_k / x_{k-1} swapping registers (angle_sum_1 with G = 1)
                const int kend = min(k_hi, k0 + kAnchor);
                int k = k0;
                const double2* tq = tb + k;
                double2 t0 = tq[0], t1 = tq[1], t2 = tq[2], t3 = tq[3];
                for (; k + 3 < kend; k += 4) {
                    tq += 4;
                    const double2 n0 = tq[0], n1 = tq[1], n2 = tq[2], n3 = tq[3];
                    sc = fma(t0.x, cx, sc);
                    ss = fma(t0.y, sx, ss);
                    cp = fma(c2, cx, -cp);                         // x_{k+1} into (cp, sp)
                    sp = fma(c2, sx, -sp);
                    sc = fma(t1.x, cp, sc);
                    ss = fma(t1.y, sp, ss);
                    cx = fma(c2, cp, -cx);                         // x_{k+2} into (cx, sx)
                    sx = fma(c2, sp, -sx);
                    sc = fma(t2.x, cx, sc);
                    ss = fma(t2.y, sx, ss);
                    cp = fma(c2, cx, -cp);
                    sp = fma(c2, sx, -sp);
                    sc = fma(t3.x, cp, sc);
                    ss = fma(t3.y, sp, ss);
                    cx = fma(c2, cp, -cx);
                    sx = fma(c2, sp, -sx);
                    t0 = n0;
                    t1 = n1;
                    t2 = n2;
                    t3 = n3;
                }
                for (; k < kend; ++k) {                            // the last < 4 steps
                    sc = fma(t0.x, cx, sc);
                    ss = fma(t0.y, sx, ss);
                    const double nc = fma(c2, cx, -cp), ns = fma(c2, sx, -sp);
                    cp = cx;
                    sp = sx;
                    cx = nc;
                    sx = ns;
                    t0 = t1;
                    t1 = t2;
                    t2 = t3;
                }
            }
            sum = use ? sc + ss : 0.0;
        }
        sum = xor_sum(sum, S);
        const int64_t p = A.p0 + (tab_ok ? q / tpp : 0);
        if (use && jj == 0) {
            const Consts C{ks[io][0], 0.0, ks[io][1], ks[io][2], a, b, c[2], c[3]};   // ne unused
            const double price = c[29] * option_sum(C, A.call[m] != 0, S0, K, xK, ratio, sum);
            if (A.out) A.out[p * A.out_stride + A.perm[m]] = price;
            if (A.part_sse) {
                const double mk = A.mkt[m];
                const double rel = (price - mk) / mk;
                osse[io][oo] = rel * rel;
                obad[io][oo] = (isnan(price) || isinf(price) || price <= 0.0) ? 1.0 : 0.0;
            }
        }
        // ---- clamp-widened options: the whole wave prices each (lanes over k) ----
        unsigned long long mask = __ballot(cl && jj == 0);
        while (mask) {
            const int l = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const int src = (t & ~63) + l;                         // the clamped option's lane
            const int li = src / TPT, lo_ = (src % TPT) / S;
            const double* cl_c = shc[li];
            const double x = __shfl(xK, l, 64), Kl = __shfl(K, l, 64);
            const int ml = (int)cl_c[27] + lo_;
            const int64_t pl = A.p0 + (b0 + li) / tpp;
            const Params P = dh::load_params(A.prm + pl * DH_PARAM_STRIDE);
            const double ac = (x - 0.1 < cl_c[0]) ? x - 0.1 : cl_c[0];      // Python min/max
            const double bc = (x + 0.1 > cl_c[1]) ? x + 0.1 : cl_c[1];
            double v = clamped_term_sum(P, cl_c[24], Kl, x, ac, bc, A.call[ml] != 0, lane, 64, N,
                                        sct);
            v = xor_sum(v, 64);
            if (lane == 0) {
                const double price = cl_c[29] * v;
                if (A.out) A.out[pl * A.out_stride + A.perm[ml]] = price;
                if (A.part_sse) {
                    const double mk = A.mkt[ml];
                    const double rel = (price - mk) / mk;
                    osse[li][lo_] = rel * rel;
                    obad[li][lo_] = (isnan(price) || isinf(price) || price <= 0.0) ? 1.0 : 0.0;
                }
            }
        }
        if (A.part_sse) {
            __syncthreads();
            // one lane per table: the options' terms in option order, then the hand-off
            if (t < 64) serial_prio(true);
            if (t < nb) {
                const double* cc = shc[t];
                const int ng = (int)cc[28];
                double acc = 0.0;
                int nbad = 0;
                for (int o = 0; o < ng; ++o) {
                    acc += osse[t][o];
                    nbad += obad[t][o] != 0.0 ? 1 : 0;
                }
                const int64_t qq = b0 + t;
                const int64_t pp = A.p0 + qq / tpp;
                const int tile = A.paired ? 0 : (int)(qq % tpp);
                const int64_t task = A.paired ? pp : pp * A.n_tiles + tile;
                __hip_atomic_store(&A.part_sse[task], acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&A.part_bad[task], nbad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const unsigned old = __hip_atomic_fetch_add(&A.counter[pp * kCounterStride], 1u,
                                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int ntask = A.paired ? 1 : A.n_tiles;
                if (old == (unsigned)ntask - 1u) {
                    const int64_t base_i = A.paired ? pp : pp * A.n_tiles;
                    double s2 = 0.0;
                    int bad = 0;
                    for (int j = 0; j < ntask; ++j) {                // tile order
                        s2 += __hip_atomic_load(&A.part_sse[base_i + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        bad += __hip_atomic_load(&A.part_bad[base_i + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    loss_out(A, pp, s2, bad);
                    __hip_atomic_store(&A.counter[pp * kCounterStride], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        __syncthreads();                                 // gtab / shc / osse reused
    }
}

// ----------------------------------------------------------------------------------------------
// fused request kernel: one block per table (p, g) whose maturity group is one tile.
//   prologue (thread 0) || option staging (other waves first) -> CF loop writing the expanded
//   table straight into LDS + k-sums -> clamp scan -> fixed-order constants || rotations ->
//   tile sums -> fence-free loss hand-off.
// One launch and no table round trip through L2/MALL: the latency path of small requests
// (calibration function+gradient requests).  Every value is computed by the same expression, in
// the same order and with the same lane partition as cos_table_kernel<TPT1> followed by
// cos_option_kernel<tpt2>, so the two paths give the same bits.
// ----------------------------------------------------------------------------------------------
template <int TPT1, int RT, int WV = DH_FUSED_WAVES, bool KP = false>
__global__ __launch_bounds__(kBlock, WV) void cos_fused_kernel(
    const double* __restrict__ h_prm, const double* __restrict__ h_tsrc,
    const int2* __restrict__ h_groups, const int* __restrict__ h_live,
    const double* __restrict__ h_pre, int h_tpp, int h_paired, PriceArgs A_, int tpt2,
    typename std::conditional<KP, KargParams, NoKargParams>::type pb_) {
    // KP: the records are the param block at the end of the kernel arguments (read in place)
    const double* prm0 = KP ? karg_ref<KargParams, kFusedParamsKernargOff>().v : h_prm;
    const double* tsrc0 = KP ? karg_ref<KargParams, kFusedParamsKernargOff>().T : h_tsrc;
    const int2* groups0 = KP ? karg_ref<KargParams, kFusedParamsKernargOff>().groups : h_groups;
    const FusedHead H{prm0, tsrc0, groups0, h_live ? h_live : &kLiveOne, h_pre, h_tpp, h_paired};
    const PriceArgs& A = karg_ref<PriceArgs, kFusedArgsKernargOff>();
    // the halt test's load is issued here (a global load: a flat one would also hold up every
    // scalar load's wait) and its value used after the staging barrier, so it overlaps the
    // prologue instead of delaying it (a halted launch wastes the prologue only)
    const int live_v = *(const __attribute__((address_space(1))) int*)H.live;
    karg_prefetch_lines();
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double shc[kTabC];
    __shared__ double red[4][1];
    __shared__ double2 sct[dh::kMathTab];
    __shared__ unsigned long long cmask[kTileMax / 64];
    const int nthr = blockDim.x;
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wv = t >> 6;
    const int64_t q = blockIdx.x;                       // dispatch index
    // index arithmetic without per-lane divisions (dh_index.h) in the 4-wave builds; the 5-wave
    // build keeps `/` and `%`: with them replaced its register allocation cost C4 2%
    constexpr bool kIdx = WV <= DH_FUSED_WAVES;
    // the table it prices (block-uniform: said so, its decomposition runs on the scalar unit)
    const int64_t qt = kIdx ? (int64_t)(unsigned)__builtin_amdgcn_readfirstlane(
                                  (int)xcd_table(A, H.tpp, q))
                            : xcd_table(A, H.tpp, q);
    int64_t p;                                          // 32-bit: grids < 2^31 blocks
    int g;
    dh_idx::table_split(qt, H.tpp, p, g);
    DH_RT_BEGIN(A);
    DH_STAMP(A, 0);

    // ---- prologue (wave 0, lane-parallel) || per-option staging (wave 0 takes the last
    //      indices).  The prologue comes first in program order and reads the preloaded
    //      arguments only, so its loads issue before any kernel-argument wait ----
    // K_cf on the block's last wave (its CF-cut test overlaps wave 0's prologue; the staging loop
    // below gives that wave option indices nthr - 128 .. nthr - 65, none on C3's 100-option tiles)
    // (the <= 96-VGPR wide build runs it on wave 0 after the prologue: one range computation
    // less, and the build's register allocation gains: C4 -2.6%)
    const int wcut = (nthr > 64 && WV <= DH_FUSED_WAVES) ? nthr / 64 - 1 : 0;
    // prologues ahead (4-wave build, >= 3 waves): the first-round block's writer wave, and
    // whether this block's constants may have been formed ahead
    const int64_t R = (WV <= DH_FUSED_WAVES && nthr >= 192) ? A.ahead_stride : 0;
    const bool ahead_w = R > 0 && q < R;
    const bool ahead_r = R > 0 && q >= R && q < (kAheadMax + 1) * R;
    const int64_t nblocks = gridDim.x;
    if (!H.pre && (wv == 0 || wv == wcut)) serial_prio(true);
    if (H.pre) {
        if (t < kTabC) shc[t] = H.pre[qt * kTabC + t];
    } else if (wv == 0) {
        // (each of the two waves decides on its own flag load and fills its own slots: loaded or
        // formed, the same values, so a flag set between the two loads changes nothing)
        int kcf_f = 0;
        if (ahead_r && ahead_ready(A, q, kcf_f)) {
            ahead_read(A, H, q, qt, shc, lane);
            if (wcut == 0 && lane == 0) shc[30] = kcf_f;
        } else {
            table_prologue_wave(A, H, qt, shc, lane, wcut == 0);
        }
    } else if (wv == wcut) {
        int kcf_f = 0;
        if (ahead_r && ahead_ready(A, q, kcf_f)) {
            if (lane == 0) shc[30] = kcf_f;
        } else {
            const int kcf = A.N < kCfCutMinN ? A.N : prologue_cut_wave(A, H, qt, lane);
            if (lane == 0) shc[30] = kcf;
        }
    }
    DH_STAMP(A, 8);
    const int N = A.N;
    const int cap = A.opt_cap;
    const TileLds L = tile_lds(smem, N, cap);
    double* lclp = smem + option_lds_doubles(N, cap);     // prices of clamp-widened options
    int g0, gn;
    if (H.paired) {
        g0 = (int)p;
        gn = 1;
    } else {
        const int2 gr = H.groups[g];
        g0 = gr.x;
        gn = gr.y;
    }
    const double* prm = H.prm + p * DH_PARAM_STRIDE;
    const double S0 = prm[13];
    dh::load_math_tables(sct, nthr > 64 ? 64 : 0);      // the waves after the prologue's
    // the surface's spot cache (dh_surface_stage_spot) holds this record's spot, bit for bit: the
    // strike, its log-moneyness and K / S0 are loaded, not formed (an fp64 division and a log per
    // option and table less).  Block-uniform, decided on the scalar unit; the 4-wave builds only
    // (the 5-wave build's register allocation is left alone, as with kIdx).  Whether the surface
    // has a cache is known from the kernel arguments alone, so its loads issue beside the
    // record's (S0) and not behind it; the compare then keeps them or forms the values
    // (measured with the loads inside the branch on the compare: C2 +0.09 us)
    constexpr bool kSpot = WV <= DH_FUSED_WAVES;
    const bool cached = kSpot && A.xk_s != nullptr;
    // staging order: waves 1, 2, .., then 0 (its prologue first)
    for (int i = kIdx ? dh_idx::rot64(t, nthr) : (t + nthr - 64) % nthr; i < gn; i += nthr) {
        const int m = g0 + i;
        double K = 0.0, xK = 0.0, ratio = 0.0;
        if (cached) {
            K = A.k_s[m];
            xK = A.xk_s[m];
            ratio = A.exk_s[m];
        }
        const bool staged = cached && __builtin_amdgcn_readfirstlane((int)(
            (unsigned long long)__double_as_longlong(S0) == A.spot_staged));
        if (!staged) {
            K = option_strike(A, m, S0);
            xK = option_logk(K, S0, ratio);
        }
        L.K[i] = K;
        L.mkt[i] = A.mkt ? A.mkt[m] : 0.0;
        L.call[i] = A.call[m];
        if (A.out) L.perm[i] = A.perm[m];                 // loss requests: no price columns
        L.xK[i] = xK;
        L.exK[i] = ratio;
    }
    __syncthreads();
    serial_prio(false);
    if (__builtin_amdgcn_readfirstlane(live_v) <= 0) return;   // every block reads the same count
    DH_STAMP(A, 1);

    const double a = shc[0], b = shc[1], eb = shc[2], ea = shc[3], scale = shc[4], piba = shc[5];
    const double T = shc[24];
    const int kcf = (int)shc[30];                    // CF entries k < K_cf (cf_cut_wave)
    // ---- clamp-widened options (double_heston.py:135-137), decided and priced per wave: the
    //      masks first (a short loop), the pricing loop only where a mask is set (rare: its
    //      register traffic stays off the common path).  The masks and prices are read after the
    //      CF barrier, so the scan may run before or after the CF loop with the same bits: before
    //      it in the 4-wave build (after it, the scan's LDS reads queue behind the table's stores
    //      on the request's critical path: C2 -1.7%), after it in the 5-wave build (before it,
    //      the register allocation of the <= 96-VGPR build costs C4 3%) ----
    auto clamp_scan = [&](int first, int step) {
        bool any_cl = false;
        for (int base = first; base < gn; base += step) {
            const int o = base + lane;
            bool cl = false;
            if (o < gn) {
                const double xK = L.xK[o];
                cl = xK - 0.1 < a || xK + 0.1 > b;
            }
            const unsigned long long mask = __ballot(cl);
            if (lane == 0) cmask[base / 64] = mask;
            any_cl = any_cl || mask != 0;
        }
        if (__builtin_expect(any_cl, 0))
        for (int base = first; base < gn; base += step) {
            const int o = base + lane;
            bool cl = false;
            if (o < gn) {
                const double xK = L.xK[o];
                cl = xK - 0.1 < a || xK + 0.1 > b;
            }
            unsigned long long mask = __ballot(cl);
            if (mask == 0) continue;
            const Params P = dh::load_params(prm);
            const double disc = exp(-P.r * T);
            while (mask) {
                const int l = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const double x = L.xK[base + l];
                const double ac = (x - 0.1 < a) ? x - 0.1 : a;      // Python min/max
                const double bc = (x + 0.1 > b) ? x + 0.1 : b;
                double v = clamped_term_sum(P, T, L.K[base + l], x, ac, bc, L.call[base + l] != 0,
                                            lane, 64, N, sct);
                v = xor_sum(v, 64);
                if (lane == 0) lclp[base + l] = disc * v;
            }
        }
    };
    // (measured and not kept: the scan after the CF loop in multi-round requests, C3 +0.8 us)
    constexpr bool kEarlyClamp = WV <= DH_FUSED_WAVES;
    // (measured and not kept: the scan by the block's last wave when the CF loop leaves it idle,
    // so that the CF waves start their entries at once: C2 -0.1 us, C3 +0.2 us)
    if constexpr (kEarlyClamp) clamp_scan(wv * 64, nthr);
    DH_STAMP(A, 29);
    // ---- CF loop (threads < TPT1, one entry each up to N = 256): expanded table into LDS.
    //      (A lane pair per entry, one Heston factor each, cut C1 by 5% but cost C2 2%: the CF
    //      phase of a C2 request is issue-bound on the CUs that host two blocks.) ----
    __shared__ double w0s;
    if (t < TPT1) {
        dh::CfConsts CC;
        {
            double* cc = (double*)&CC;
            for (int j = 0; j < 16; ++j) cc[j] = shc[6 + j];
        }
        DH_STAMP(A, 6);
        DH_STAMP_T(A, 19, 64);
        DH_STAMP_T(A, 20, 192);
        table_entries<TPT1>(CC, t, kcf, piba, T, a, scale, sct, [&](int k, double u, double w) {
            if (k == 0) {
                w0s = 0.5 * w;
                L.t26[0] = make_double2(0.0, 0.0);
                return;
            }
            const double T2 = w * S0 * dh::drcp(1.0 + u * u);
            L.t26[k] = make_double2(T2, -(T2 * dh::drcp(u)));
        });
        DH_STAMP(A, 7);
        DH_STAMP_T(A, 16, 64);
        DH_STAMP_T(A, 17, 128);
        DH_STAMP_T(A, 18, 192);
    }
    // prologues ahead: the later tables' K_cf on the cut wave; both writer waves' stores drained
    // before the barrier, the flags after it
    int kcf_ahead = 0;
    if (ahead_w && wv == wcut) kcf_ahead = ahead_write(A, H, q, nblocks, lane);
    if constexpr (!kEarlyClamp) clamp_scan(wv * 64, nthr);
    DH_STAMP(A, 21);
    DH_STAMP_T(A, 22, 64);
    __syncthreads();
    DH_STAMP(A, 2);
    if (ahead_w && wv == wcut) ahead_publish(A, q, nblocks, lane, kcf_ahead);

    // ---- k-sums in the canonical order of a 64-thread table slot (from the LDS table; the same
    //      bits as cos_table_kernel).  c1 is a sum of zeros (+0.0) and w0 has one nonzero term
    //      (lane 0's), so their butterflies change no bit and are skipped || per-option
    //      rotations ----
    // c0 on wave 0 and c5 on the block's last wave (wave 1 stages the rotations): each wave runs
    // one sum's chain, in the same lane order and butterfly, so the same bits (4-wave build; the
    // 5-wave build keeps both on wave 0: its register allocation cost C4 2%)
    const int w5 = (WV <= DH_FUSED_WAVES && nthr >= 192) ? nthr / 64 - 1 : 0;
    if (wv == 0 || wv == w5) {
        serial_prio(true);
        const bool f0 = wv == 0, f5 = wv == w5;
        const double delta = tail_delta(A.tail, S0, b - a, N);
        double c0 = 0.0, c5 = 0.0;
        int ne = 0;                                  // n_eff (tail_keep), on wave 0 with c0
        for (int k = lane; k < kcf; k += 64) {
            if (k == 0) continue;
            const double T2 = L.t26[k].x;
            const double cb = (k & 1) ? -1.0 : 1.0;
            if (f0) {
                c0 += T2 * eb * cb;
                ne = max(ne, tail_keep(k, T2, delta));
            }
            if (f5) c5 += T2 * ea;
        }
        if (f0) {
            c0 = xor_sum(c0, 64);
            ne = xor_max_i(ne, 64);
        }
        if (f5) c5 = xor_sum(c5, 64);
        if (lane == 0) {
            if (f0) {
                red[0][0] = c0;
                red[1][0] = (double)ne;
                red[3][0] = w0s;
            }
            if (f5) red[2][0] = c5;
        }
    }
    const double disc = shc[29];                    // e^{-rT}, staged by the prologue
    const int G = group_lanes<RT, kIdx>(gn, N, tpt2);
    {
        const double ustep = G * dh::kPi / (b - a);
        // (wave 0 does the sums)
        for (int i = kIdx ? dh_idx::rot64(t, nthr) : (t + nthr - 64) % nthr; i < gn; i += nthr) {
            const bool cl = (cmask[i >> 6] >> (i & 63)) & 1ull;
            double ss, cs;
            dh::dsincos(ustep * (cl ? 0.0 : L.xK[i] - a), &ss, &cs);
            L.cs[i] = cs;
            L.ss[i] = cl ? NAN : (ss == ss ? ss : 0.0);   // as cos_option_kernel
            if (cl) record_price(A, p, L.perm[i], L.mkt[i], i, lclp[i], L.sse, L.bad);
        }
    }
    __syncthreads();
    serial_prio(false);
    DH_STAMP(A, 3);

    const Consts C{0.0 + red[0][0], 0.0 + red[1][0], 0.0 + red[2][0], 0.0 + red[3][0], a, b, eb, ea};
    if (t < tpt2)
        tile_sums_r<RT, kIdx>(A, p, C, S0, disc, gn, G, tpt2, t, true, L, lclp + cap, sct);
    DH_STAMP(A, 4);
    // (a block-wide tile reduced through LDS has just passed tile_sums' closing barrier, after
    // its last loss terms were written, so a second one is not needed; measured, dropping it was
    // slower on C3: 57.8 vs 57.45 us per request)
#ifndef DH_SKIP_HANDOFF_BARRIER
#define DH_SKIP_HANDOFF_BARRIER 0
#endif
    const bool lds_red = DH_SKIP_HANDOFF_BARRIER && tpt2 == kBlock && nthr == kBlock &&
                         (G > 64 || (G & (G - 1)) != 0);
    if (A.part_sse) {
        if (!lds_red) __syncthreads();
        if (t < 64) {
            serial_prio(true);
            task_loss(A, p, A.paired ? p : p * A.n_tiles + g, gn, t, L.sse, L.bad);
            // the grid's last P blocks (dispatch order) then sum one param set each
            if (A.partials_only == 3 && q >= nblocks - A.P) tail_sums(A, q - (nblocks - A.P), t);
        }
    }
    DH_STAMP(A, 5);
    DH_RT_END(A);
}

// ----------------------------------------------------------------------------------------------
// validation path: reference operation order (double_heston.py:160-192), one wave per option
// ----------------------------------------------------------------------------------------------
__device__ __forceinline__ double exact_term_sum(const Params& P, double T, double K, double xK,
                                                 double a, double b, bool is_call, int k_first,
                                                 int k_step, int N) {
    const double ba = b - a;
    const double scale = 2.0 / ba;
    double acc = 0.0;
    for (int k = k_first; k < N; k += k_step) {
        const double u = k * dh::kPi / ba;
        const cplx phi = dh::cf_eval(P, u, T);
        double sa, ca;
        dh::dsincos(u * a, &sa, &ca);
        const double re = phi.re * ca + phi.im * sa;       // Re(phi exp(-i u a))
        double chi, psi;
        if (is_call) dh::cos_coeffs(k, xK, b, a, b, chi, psi);
        else dh::cos_coeffs(k, a, xK, a, b, chi, psi);
        const double V = is_call ? scale * (P.S0 * chi - K * psi) : scale * (K * psi - P.S0 * chi);
        double term = re * V;
        if (k == 0) term *= 0.5;
        acc += term;
    }
    return acc;
}

__global__ __launch_bounds__(kBlock) void cos_exact_kernel(PriceArgs A, double* prices) {
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const int M = A.M;
    const int64_t n_items = A.paired ? A.P : A.P * (int64_t)M;
    if (item >= n_items) return;                       // whole wave exits together
    const int64_t p = A.paired ? item : item / M;
    const int m = A.paired ? (int)p : (int)(item % M);
    const Params P = dh::load_params(A.prm + p * DH_PARAM_STRIDE);
    const double T = A.T[m];
    const double K = option_strike(A, m, P.S0);
    const bool is_call = A.call[m] != 0;
    const double xK = log(K / P.S0);
    double a0, b0;
    dh::trunc_unclamped(P, T, A.L, a0, b0);
    const double a = (xK - 0.1 < a0) ? xK - 0.1 : a0;   // Python min/max semantics (:136-137)
    const double b = (xK + 0.1 > b0) ? xK + 0.1 : b0;
    double acc = exact_term_sum(P, T, K, xK, a, b, is_call, lane, 64, A.N);
    acc = xor_sum(acc, 64);
    if (lane == 0) {
        const double price = exp(-P.r * T) * acc;
        if (A.out) A.out[p * A.out_stride + A.perm[m]] = price;
        if (prices) prices[A.paired ? p : p * M + m] = price;
    }
}

// Loss sums from a [P][M] price buffer (validation mode): one wave per param set, fixed order.
// The generator's param records from its sampler's columns (dh_surface_price_cols): rec[i][c] =
// params[i][c] (c < 13), spots[i], r, 0 -- one thread per record field, coalesced stores.
__global__ void gen_records_kernel(const double* __restrict__ params,
                                   const double* __restrict__ spots, double r, int64_t P,
                                   double* __restrict__ rec) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P * DH_PARAM_STRIDE) return;
    const int64_t row = i / DH_PARAM_STRIDE;
    const int c = (int)(i % DH_PARAM_STRIDE);
    rec[i] = c < 13 ? params[row * 13 + c] : (c == 13 ? spots[row] : (c == 14 ? r : 0.0));
}

__global__ void loss_from_prices_kernel(const double* __restrict__ prices,
                                        const double* __restrict__ mkt, int M, int64_t S,
                                        double* __restrict__ sse, int* __restrict__ n_bad) {
    const int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (s >= S) return;
    double acc = 0.0, bad = 0.0;
    for (int m = lane; m < M; m += 64) {
        const double pr = prices[s * M + m];
        const double rel = (pr - mkt[m]) / mkt[m];
        acc += rel * rel;
        bad += (isnan(pr) || isinf(pr) || pr <= 0.0) ? 1.0 : 0.0;
    }
    acc = xor_sum(acc, 64);
    bad = xor_sum(bad, 64);
    if (lane == 0) {
        sse[s] = acc;
        n_bad[s] = (int)bad;
    }
}

// ----------------------------------------------------------------------------------------------
// building blocks behind the reference's public methods
// ----------------------------------------------------------------------------------------------
__global__ void cf_kernel(const double* __restrict__ prm, const double* __restrict__ u, int n,
                          double tau, double* __restrict__ re, double* __restrict__ im) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Params P = dh::load_params(prm);
    const cplx c = dh::cf_eval(P, u[i], tau);
    re[i] = c.re;
    im[i] = c.im;
}

__global__ void cf_kernel_z(const double* __restrict__ prm, const double* __restrict__ ure,
                            const double* __restrict__ uim, int n, double tau,
                            double* __restrict__ re, double* __restrict__ im) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Params P = dh::load_params(prm);
    const cplx c = dh::cf_eval_z(P, {ure[i], uim[i]}, tau);
    re[i] = c.re;
    im[i] = c.im;
}

__global__ void trunc_kernel(const double* __restrict__ prm, const double* __restrict__ K,
                             const double* __restrict__ T, int64_t P, double L,
                             double* __restrict__ a, double* __restrict__ b) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const Params Q = dh::load_params(prm + i * DH_PARAM_STRIDE);
    double a0, b0;
    dh::trunc_unclamped(Q, T[i], L, a0, b0);
    const double xK = log(K[i] / Q.S0);
    a[i] = (xK - 0.1 < a0) ? xK - 0.1 : a0;
    b[i] = (xK + 0.1 > b0) ? xK + 0.1 : b0;
}

__global__ void coeff_kernel(const int32_t* __restrict__ k, int n, double c, double d, double a,
                             double b, double* __restrict__ chi, double* __restrict__ psi) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x, y;
    dh::cos_coeffs(k[i], c, d, a, b, x, y);
    chi[i] = x;
    psi[i] = y;
}

}  // namespace

// Nothing below, the headers included, is contracted into FMAs: the device L-BFGS-B (dh_lbfgs.h,
// dh_lb_driver.h) must compute the bits of its CPU build (tests/native/lb_host.cpp), and the
// feature headers the bits their tests pin.  Device code above this line is contracted.
#pragma clang fp contract(off)

namespace {

constexpr double kInvalidLoss = 1e10;                 // lbfgs_calibrator.py:152-158,176-177
constexpr double kFdStep = 1e-8;                      // SciPy L-BFGS-B eps
constexpr double kSqrtEps = 1.4901161193847656e-08;   // sqrt(DBL_EPSILON), _numdiff fallback

// ---- the record arithmetic, defined once for every optimiser path, device and host ---------------
// model parameter i from unconstrained x_i (lbfgs_calibrator.py:62-87): tanh for the two
// correlations, identity for mu_j, exp otherwise
__host__ __device__ __forceinline__ double lb_transform(int i, double x) {
    if (i == 4 || i == 9) return tanh(x);
    if (i == 11) return x;
    return exp(x);
}

// d lb_transform(i, x_i) / d x_i from the model parameters q
__device__ __forceinline__ double transform_dt(int i, const double* q) {
    return (i == 4 || i == 9) ? 1.0 - q[i] * q[i] : (i == 11 ? 1.0 : q[i]);
}

// the Feller penalty (lbfgs_calibrator.py:113-116): 1000 max(0, sigma^2 - 2 kappa theta) per factor
__host__ __device__ __forceinline__ double feller_penalty(const double* p) {
    const double v1 = p[3] * p[3] - 2.0 * p[1] * p[2];
    const double v2 = p[8] * p[8] - 2.0 * p[6] * p[7];
    return 1000.0 * ((v1 > 0.0 ? v1 : 0.0) + (v2 > 0.0 ? v2 : 0.0));
}

// adds d feller_penalty / d x to go [13], per factor where its slack is strictly positive
__device__ __forceinline__ void feller_kink_grad(const double* q, double* go) {
#pragma unroll
    for (int fct = 0; fct < 2; ++fct) {
        const int o = 5 * fct;
        const double kap = q[o + 1], th = q[o + 2], sig = q[o + 3];
        if (sig * sig - 2.0 * kap * th > 0.0) {
            go[o + 3] = go[o + 3] + 2000.0 * (sig * sig);
            go[o + 1] = go[o + 1] - 2000.0 * (kap * th);
            go[o + 2] = go[o + 2] - 2000.0 * (kap * th);
        }
    }
}

// unconstrained x [S][13] -> param records (exp / tanh / identity, lbfgs_calibrator.py:62-87)
// and Feller penalties (:113-116); one thread per set
__global__ void x_records_kernel(const double* __restrict__ x, int S, double S0, double r,
                                 double* __restrict__ rec, double* __restrict__ pen) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    double p[dhlb::kN];
#pragma unroll
    for (int i = 0; i < dhlb::kN; ++i) p[i] = lb_transform(i, x[(size_t)s * dhlb::kN + i]);
    pen[s] = feller_penalty(p);
    double* out = rec + (size_t)s * DH_PARAM_STRIDE;
#pragma unroll
    for (int i = 0; i < dhlb::kN; ++i) out[i] = p[i];
    out[13] = S0;
    out[14] = r;
    out[15] = 0.0;
}

// loss = n_bad ? 1e10 : sse / M + penalty (lbfgs_calibrator.py:152-166)
__global__ void loss_finalize_kernel(const double* __restrict__ sse, const int* __restrict__ bad,
                                     const double* __restrict__ pen, int S, int M,
                                     double* __restrict__ loss) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    loss[s] = bad[s] > 0 ? kInvalidLoss : sse[s] / (double)M + pen[s];
}

}  // namespace

// The host side and the features, in this one translation unit.  Each header needs the kernels
// above and the headers named after it here.
#include "dh_host.h"         // errors, buffers, dh_ctx / dh_surface, DeviceScope, checks: none
#include "dh_launch.h"       // the table of kernel builds, the launch planner: dh_host.h
#include "dh_api.h"          // context, surface, price, loss, function+gradient calls: dh_launch.h
#include "dh_comm.h"         // the RCCL communicator: dh_host.h
#include "dh_gen_device.h"   // the generator's device draw (defines GenBufs): dh_api.h
#include "dh_iv.h"           // implied vols: dh_api.h
#include "dh_iv_loss.h"      // the vol-space loss stages: dh_iv.h, dh_api.h
#include "dh_loss_rows.h"    // per-set market rows: dh_iv_loss.h
#include "dh_math_probe.h"   // the device math primitives one by one: dh_host.h
#include "dh_mc.h"           // the Monte Carlo path pricer (includes dh_mc_vr.h, its control
                             // variates): dh_host.h, dh_api.h
#include "dh_mc_greeks.h"    // its delta, gamma and v0 vegas from coupled paths: dh_mc.h
#include "dh_lsm.h"          // American / Bermudan options by least-squares Monte Carlo: dh_mc.h
#include "dh_greeks.h"       // analytic Greeks of the COS price: dh_host.h
#include "dh_greeks_full.h"  // their full build (maturity, rate, dual gamma, local variance):
                             // dh_greeks.h
#include "dh_param_grad.h"   // analytic parameter sensitivities, loss + gradient, and the analytic
                             // rows request (GradRows, its scratch, epilogue and host path):
                             // dh_greeks.h, dh_loss_rows.h, dh_api.h
#include "dh_iv_grad.h"      // the vol objective's exact gradient: dh_iv_loss.h, dh_param_grad.h
#include "dh_gauss_newton.h" // the Gauss-Newton rows reduction: dh_param_grad.h
#include "dh_lb_driver.h"    // the device-resident L-BFGS-B and Levenberg-Marquardt: dh_api.h,
                             // dh_iv_loss.h, dh_loss_rows.h, dh_param_grad.h, dh_iv_grad.h,
                             // dh_gauss_newton.h
#include "dh_ffn.h"          // the warm-start network's inference: dh_host.h
