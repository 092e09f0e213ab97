// dh_loss_rows.h -- the losses against per-set market rows, the reductions of the batched
// multi-market calibrations: in relative price (dh_surface_loss_rows_dev, dh_surface_loss_rows;
// dh_calibrate_lbfgs_batch) and in implied vol (dh_surface_iv_sse_rows_dev,
// dh_surface_loss_iv_rows; dh_calibrate_lbfgs_batch_iv).  Included by dh_kernels.hip after
// dh_iv_loss.h and ahead of the L-BFGS-B driver (dh_lb_driver.h).  DESIGN.md 3.12, 3.13.
//
// Stages beside the request kernels, as dh_iv_loss.h's: each reads the [S][M] prices a pricing
// request wrote (the caller's option order) and reduces each set against the market row its start
// belongs to, one wave per set.  No atomics, no hand-off between waves.
#pragma once
#pragma clang fp contract(off)

namespace {

constexpr int kBlockRows = 256;     // four waves, four sets per block

// the grid of a one-wave-per-set launch
unsigned rows_grid(int S) {
    return (unsigned)(((int64_t)S * 64 + kBlockRows - 1) / kBlockRows);
}

// the row checks of the two host entry points
int check_rows(const int32_t* row, int S, int B) {
    if (B <= 0) return fail(DH_E_ARG, "B <= 0");
    for (int i = 0; i < S; ++i)
        if (row[i] < 0 || row[i] >= B)
            return fail(DH_E_ARG, "row " + std::to_string(i) + " is outside [0, B)");
    return DH_OK;
}

// the spot and rate of every market of a rows request or a batch calibration
int check_spot_rate(const double* spot, const double* rate, int B) {
    for (int b = 0; b < B; ++b) {
        if (!std::isfinite(spot[b]) || !(spot[b] > 0.0))
            return fail(DH_E_ARG, "spot " + std::to_string(b) + " is not finite or not > 0");
        if (!std::isfinite(rate[b]))
            return fail(DH_E_ARG, "rate " + std::to_string(b) + " is not finite");
    }
    return DH_OK;
}

}  // namespace

// ---- relative price ---------------------------------------------------------------------------
//     sse[s] = sum_m ((p_sm - mkt[row[s]][m]) / mkt[row[s]][m])^2,
//     n_bad[s] = #{m : p_sm NaN, +-inf or <= 0}
// -- dh_surface_loss's rules: a zero market price gives inf (NaN where the price is 0 too), a NaN
// one NaN.
//
// Summation order.  One wave per set.  Lane l starts from 0.0 and adds the terms of options l,
// l + 64, l + 128, ... in that order (a lane with no option keeps 0.0); then the xor butterfly over
// the 64 lanes, offsets 1, 2, 4, 8, 16, 32 (xor_sum: both partners add the same two operands).
// Nothing is contracted into an FMA.  The order is a function of M alone: not of S, of the set's
// place in the request, of its row or of the stream.
namespace dhrows {

// live_count: the device-resident driver's count of unfinished starts (the launch is a no-op at
// 0), or null
__global__ __launch_bounds__(kBlockRows) void loss_rows_kernel(
    const double* __restrict__ prices, const double* __restrict__ mkt,
    const int* __restrict__ row, int M, int64_t S, const int* __restrict__ live_count,
    double* __restrict__ sse, int* __restrict__ n_bad) {
    if (live_count && __builtin_amdgcn_readfirstlane(*live_count) <= 0) return;
    const int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (s >= S) return;                              // whole waves: s is uniform across a wave
    const double* p = prices + s * M;
    const double* mk = mkt + (int64_t)row[s] * M;
    double acc = 0.0;
    int bad = 0;
    for (int m0 = 0; m0 < M; m0 += 64) {             // every lane makes every pass
        const int m = m0 + lane;
        if (m < M) {
            const double pr = p[m], mm = mk[m];
            const double rel = (pr - mm) / mm;
            acc = acc + rel * rel;
            bad += (pr != pr || isinf(pr) || pr <= 0.0) ? 1 : 0;
        }
    }
    acc = xor_sum(acc, 64);
    for (int off = 1; off < 64; off <<= 1) bad += __shfl_xor(bad, off, 64);
    if (lane == 0) {
        sse[s] = acc;
        n_bad[s] = bad;
    }
}

}  // namespace dhrows

// the launch behind dh_surface_loss_rows_dev and the batch driver's iterations
static int loss_rows_launch(dh_ctx* ctx, const dh_surface* s, const double* d_prices,
                            const double* d_mkt, const int32_t* d_row, int S, double* d_sse,
                            int32_t* d_n_bad, void* stream, const int* live_count) {
    if (!ctx || !s || (S > 0 && (!d_prices || !d_mkt || !d_row || !d_sse || !d_n_bad)))
        return fail(DH_E_ARG, "null argument");
    return loss_stage(ctx, s, S, d_sse, d_n_bad, stream, [&](hipStream_t st) -> int {
        hipLaunchKernelGGL(dhrows::loss_rows_kernel, dim3(rows_grid(S)), dim3(kBlockRows), 0, st,
                           d_prices, d_mkt, (const int*)d_row, s->M, (int64_t)S, live_count,
                           d_sse, (int*)d_n_bad);
        HIP_TRY(hipGetLastError());
        return DH_OK;
    });
}

extern "C" int dh_surface_loss_rows_dev(dh_ctx* ctx, const dh_surface* s, const double* d_prices,
                                        const double* d_mkt, const int32_t* d_row, int S,
                                        double* d_sse, int32_t* d_n_bad, void* stream) {
    return loss_rows_launch(ctx, s, d_prices, d_mkt, d_row, S, d_sse, d_n_bad, stream, nullptr);
}

extern "C" int dh_surface_loss_rows(dh_ctx* ctx, const dh_surface* s, const double* params,
                                    const double* mkt, const int32_t* row, int S, int B, int N,
                                    double L, double* sse, int32_t* n_bad, double* prices) {
    if (!ctx || !s || (S > 0 && (!params || !mkt || !row || !sse || !n_bad)))
        return fail(DH_E_ARG, "null argument");
    int rc = check_N(N);
    if (rc) return rc;
    if (S < 0) return fail(DH_E_ARG, "S < 0");
    if (S == 0) return DH_OK;
    rc = check_rows(row, S, B);
    if (rc) return rc;
    const HostRows rows{mkt, nullptr, row, B, false};
    return loss_round_trip(ctx, s, params, &rows, S, N, L, sse, n_bad, prices, nullptr,
                           [&](const StageIn& d) {
                               return loss_rows_launch(ctx, s, d.prices, d.mkt, d.row, S, d.sse,
                                                       d.n_bad, d.st, nullptr);
                           });
}

// ---- implied vol ------------------------------------------------------------------------------
// dh_iv_loss.h's semantics: each price is inverted with dhiv::implied_vol under the set's own
// record (spot, rate, q from rec[13..15]),
//     sse[s]   = sum_m w[row[s]][m] (v_sm - mkt_iv[row[s]][m])^2,
//     n_bad[s] = #{m : w[row[s]][m] > 0, option m has no vol}
// -- surface_iv_sse_kernel's rules, by its own text (dhivl::vol_term): a price that is NaN, +-inf
// or <= 0 is passed as inactive and is bad; a NaN vol of a price a rounding below its lower bound
// becomes 0.0 (below_lower); a zero weight contributes to neither sum.
//
// Summation order.  One wave per set.  Lane l starts from 0.0 and takes the surface's *sorted*
// options l, l + 64, l + 128, ... in that order (the index surface_iv_sse_kernel walks: K[m], T[m],
// c = perm[m] the option's place in the caller's order), adding each term w (d d) uncontracted (a
// lane with no option, a zero weight or a bad option adds nothing); then the xor butterfly over
// the 64 lanes, offsets 1, 2, 4, 8, 16, 32 (xor_sum).  Every lane of a live wave makes every pass
// -- implied_vol leaves its loop on a wave-wide __all, so a lane past M calls it as inactive --
// and only whole waves with s >= S return early.  The order is a function of M and the surface's
// option sort alone.
//
// Consequence: for M <= 64 a set's sse and n_bad have the bits dh_surface_iv_sse_dev gives the
// same vols and weights -- that kernel's wave 0 holds the same lanes (0.0 + term is term), and its
// other three wave sums are +0.0.
namespace dhivr {

// live_count: the device-resident driver's count of unfinished starts (the launch is a no-op at
// 0), or null
__global__ __launch_bounds__(kBlockRows, DH_IV_WAVES) void iv_sse_rows_kernel(
    const double* __restrict__ prices, const double* __restrict__ prm,
    const double* __restrict__ K, const double* __restrict__ T, const int8_t* __restrict__ call,
    const int* __restrict__ perm, const double* __restrict__ mkt_iv,
    const double* __restrict__ wgt, const int* __restrict__ row, int strike_mode, int M, int64_t S,
    const int* __restrict__ live_count, double* __restrict__ iv, double* __restrict__ sse,
    int* __restrict__ n_bad) {
    if (live_count && __builtin_amdgcn_readfirstlane(*live_count) <= 0) return;
    const int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (s >= S) return;                              // whole waves: s is uniform across a wave
    const double* rec = prm + s * DH_PARAM_STRIDE;
    const double S0 = rec[13], r = rec[14], q = rec[15];
    const int64_t b = row[s];
    const double* mk = mkt_iv + b * M;
    const double* wg = wgt + b * M;
    double acc = 0.0;
    int bad = 0;
    for (int m0 = 0; m0 < M; m0 += 64) {             // every lane makes every pass
        const int i = m0 + lane;
        const dhivl::VolTerm t = dhivl::vol_term(S0, r, q, s, i, i < M, prices, K, T, call, perm,
                                                 mk, wg, strike_mode, M, iv);
        if (t.bad) bad += 1;
        else if (t.w > 0.0) acc = acc + t.term;
    }
    acc = xor_sum(acc, 64);
    for (int off = 1; off < 64; off <<= 1) bad += __shfl_xor(bad, off, 64);
    if (lane == 0) {
        sse[s] = acc;
        n_bad[s] = bad;
    }
}

}  // namespace dhivr

// the launch behind dh_surface_iv_sse_rows_dev and the vol-space batch driver's iterations
static int iv_rows_launch(dh_ctx* ctx, const dh_surface* s, const double* d_params,
                          const double* d_prices, const double* d_mkt_iv, const double* d_wgt,
                          const int32_t* d_row, int S, double* d_sse, int32_t* d_n_bad,
                          double* d_iv, void* stream, const int* live_count) {
    if (!ctx || !s ||
        (S > 0 && (!d_params || !d_prices || !d_mkt_iv || !d_wgt || !d_row || !d_sse || !d_n_bad)))
        return fail(DH_E_ARG, "null argument");
    return loss_stage(ctx, s, S, d_sse, d_n_bad, stream, [&](hipStream_t st) -> int {
        hipLaunchKernelGGL(dhivr::iv_sse_rows_kernel, dim3(rows_grid(S)), dim3(kBlockRows), 0, st,
                           d_prices, d_params, s->K, s->T, s->call, s->perm, d_mkt_iv, d_wgt,
                           (const int*)d_row, s->strike_mode, s->M, (int64_t)S, live_count, d_iv,
                           d_sse, (int*)d_n_bad);
        HIP_TRY(hipGetLastError());
        return DH_OK;
    });
}

extern "C" int dh_surface_iv_sse_rows_dev(dh_ctx* ctx, const dh_surface* s, const double* d_params,
                                          const double* d_prices, const double* d_mkt_iv,
                                          const double* d_wgt, const int32_t* d_row, int S,
                                          double* d_sse, int32_t* d_n_bad, double* d_iv,
                                          void* stream) {
    return iv_rows_launch(ctx, s, d_params, d_prices, d_mkt_iv, d_wgt, d_row, S, d_sse, d_n_bad,
                          d_iv, stream, nullptr);
}

extern "C" int dh_surface_loss_iv_rows(dh_ctx* ctx, const dh_surface* s, const double* params,
                                       const double* mkt_iv, const double* wgt, const int32_t* row,
                                       int S, int B, int N, double L, double* sse, int32_t* n_bad,
                                       double* prices, double* iv) {
    if (!ctx || !s || (S > 0 && (!params || !mkt_iv || !row || !sse || !n_bad)))
        return fail(DH_E_ARG, "null argument");
    int rc = check_N(N);
    if (rc) return rc;
    if (S < 0) return fail(DH_E_ARG, "S < 0");
    if (S == 0) return DH_OK;
    rc = check_rows(row, S, B);
    if (rc) return rc;
    const HostRows rows{mkt_iv, wgt, row, B, true};
    return loss_round_trip(ctx, s, params, &rows, S, N, L, sse, n_bad, prices, iv,
                           [&](const StageIn& d) {
                               return iv_rows_launch(ctx, s, d.params, d.prices, d.mkt, d.wgt,
                                                     d.row, S, d.sse, d.n_bad, d.iv, d.st,
                                                     nullptr);
                           });
}
