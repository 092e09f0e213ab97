// dh_iv_loss_rows.h -- the implied-vol loss against per-set market rows
// (dh_surface_iv_sse_rows_dev, dh_surface_loss_iv_rows) and the batched multi-market calibration
// in vol space (dh_calibrate_lbfgs_batch_iv).  Included by dh_kernels.hip after dh_iv_loss.h; the
// L-BFGS-B driver (lb_run, ahead of dh_iv.h) reaches the launch through a forward declaration.
// DESIGN.md 3.13.
//
// A stage beside the request kernels, shaped like dh_loss_rows.h's, with dh_iv_loss.h's semantics:
// it reads the [S][M] prices a pricing request wrote (the caller's option order), inverts each with
// dhiv::implied_vol under the set's own record (spot, rate, q from rec[13..15]) and reduces each
// set against the market row its start belongs to,
//     sse[s]   = sum_m w[row[s]][m] (v_sm - mkt_iv[row[s]][m])^2,
//     n_bad[s] = #{m : w[row[s]][m] > 0, option m has no vol}
// -- surface_iv_sse_kernel's rules: a price that is NaN, +-inf or <= 0 is passed as inactive and is
// bad; a NaN vol of a price a rounding below its lower bound becomes 0.0 (below_lower); a zero
// weight contributes to neither sum.
//
// Summation order.  One wave per set.  Lane l starts from 0.0 and takes the surface's *sorted*
// options l, l + 64, l + 128, ... in that order (the index surface_iv_sse_kernel walks: K[m], T[m],
// c = perm[m] the option's place in the caller's order), adding each term w (d d) uncontracted (a
// lane with no option, a zero weight or a bad option adds nothing); then the xor butterfly over
// the 64 lanes, offsets 1, 2, 4, 8, 16, 32 (xor_sum).  Every lane of a live wave makes every pass
// -- implied_vol leaves its loop on a wave-wide __all, so a lane past M calls it as inactive --
// and only whole waves with s >= S return early.  No atomics, no hand-off between waves.  The
// order is a function of M and the surface's option sort alone.
//
// Consequence: for M <= 64 a set's sse and n_bad have the bits dh_surface_iv_sse_dev gives the
// same vols and weights -- that kernel's wave 0 holds the same lanes (0.0 + term is term), and its
// other three wave sums are +0.0.
//
// The divisor.  The vol objective's loss is sse / sum_m w[b][m] + Feller (loss_batch's).  A
// market's weight sum is formed on the host, in option order, sequentially (wsum += w[b][m], m =
// 0 .. M - 1, from 0.0), and gathered per start as spot and rate are; the step kernel's kIv builds
// divide by it where the price objective divides by M.
#pragma once
#pragma clang fp contract(off)

namespace dhivr {

constexpr int kBlockRows = 256;     // four waves, four sets per block

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
        const bool active = i < M;
        const int m = active ? i : 0;
        const double Kin = K[m], Tm = T[m];
        const bool is_call = call[m] != 0;
        const double strike = strike_mode == DH_STRIKE_PCT_SPOT ? Kin * S0 / 100.0 : Kin;
        const int c = perm[m];                       // the option's place in the caller's order
        const int64_t o = s * M + c;
        const double price = prices[o];
        // dh_surface_loss's rule: NaN, +-inf and <= 0 are bad prices (a > 0 also rejects NaN)
        const bool priced = active && price > 0.0 && isfinite(price);
        double v = dhiv::implied_vol(priced, price, S0, strike, Tm, r, q, is_call);
        // a model price a rounding below its lower bound: the vol's continuous extension
        if (priced && v != v && dhivl::below_lower(price, S0, strike, Tm, r, q, is_call)) v = 0.0;
        if (active && iv) iv[o] = v;
        const double w = active ? wg[c] : 0.0;
        if (w > 0.0) {                               // a zero weight: nothing enters the sums
            if (v != v) {
                bad += 1;
            } else {
                const double d = v - mk[c];
                acc = acc + w * (d * d);
            }
        }
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
    const int64_t nb = ((int64_t)S * 64 + dhivr::kBlockRows - 1) / dhivr::kBlockRows;
    hipLaunchKernelGGL(dhivr::iv_sse_rows_kernel, dim3((unsigned)nb), dim3(dhivr::kBlockRows), 0,
                       st, d_prices, d_params, s->K, s->T, s->call, s->perm, d_mkt_iv, d_wgt,
                       (const int*)d_row, s->strike_mode, s->M, (int64_t)S, live_count, d_iv,
                       d_sse, (int*)d_n_bad);
    HIP_TRY(hipGetLastError());
    return DH_OK;
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
    if (B <= 0) return fail(DH_E_ARG, "B <= 0");
    for (int i = 0; i < S; ++i)
        if (row[i] < 0 || row[i] >= B)
            return fail(DH_E_ARG, "row " + std::to_string(i) + " is outside [0, B)");
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const int M = s->M;
    const size_t pb = (size_t)S * DH_PARAM_STRIDE * 8, ob = (size_t)S * M * 8;
    const size_t mb = (size_t)B * M * 8;
    HIP_TRY(ctx->params.reserve(pb));
    HIP_TRY(ctx->sse.reserve((size_t)S * 8));
    HIP_TRY(ctx->bad.reserve((size_t)S * 4));
    HIP_TRY(ctx->out.reserve(ob));
    HIP_TRY(ctx->rows_mkt.reserve(mb));
    HIP_TRY(ctx->rows_wgt.reserve(mb));
    HIP_TRY(ctx->rows_row.reserve((size_t)S * 4));
    if (iv) HIP_TRY(ctx->iv.reserve(ob));
    hipStream_t st = ctx->stream;
    std::vector<double> ones;                        // wgt null: every weight 1
    if (!wgt && M > 0) {
        ones.assign((size_t)B * M, 1.0);
        wgt = ones.data();
    }
    HIP_TRY(hipMemcpyAsync(ctx->params.ptr, params, pb, hipMemcpyHostToDevice, st));
    if (M > 0) {
        HIP_TRY(hipMemcpyAsync(ctx->rows_mkt.ptr, mkt_iv, mb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->rows_wgt.ptr, wgt, mb, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(ctx->rows_row.ptr, row, (size_t)S * 4, hipMemcpyHostToDevice, st));
    if (M > 0) {
        rc = dh_surface_price_dev(ctx, s, (const double*)ctx->params.ptr, S, N, L,
                                  (double*)ctx->out.ptr, st);
        if (rc) {
            (void)hipStreamSynchronize(st);          // `ones` is pageable and leaves scope
            return rc;
        }
    }
    // M == 0: nothing is priced and the stage reads neither prices nor market rows
    const double* any = (const double*)ctx->params.ptr;
    rc = iv_rows_launch(ctx, s, (const double*)ctx->params.ptr,
                        M > 0 ? (const double*)ctx->out.ptr : any,
                        M > 0 ? (const double*)ctx->rows_mkt.ptr : any,
                        M > 0 ? (const double*)ctx->rows_wgt.ptr : any,
                        (const int32_t*)ctx->rows_row.ptr, S, (double*)ctx->sse.ptr,
                        (int32_t*)ctx->bad.ptr, iv && M > 0 ? (double*)ctx->iv.ptr : nullptr, st,
                        nullptr);
    if (rc) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    HIP_TRY(hipMemcpyAsync(sse, ctx->sse.ptr, (size_t)S * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(n_bad, ctx->bad.ptr, (size_t)S * 4, hipMemcpyDeviceToHost, st));
    if (M > 0) {
        if (prices) HIP_TRY(hipMemcpyAsync(prices, ctx->out.ptr, ob, hipMemcpyDeviceToHost, st));
        if (iv) HIP_TRY(hipMemcpyAsync(iv, ctx->iv.ptr, ob, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}

extern "C" int dh_calibrate_lbfgs_batch_iv(dh_ctx* ctx, const dh_surface* s, const double* mkt_iv,
                                           const double* wgt, const double* spot,
                                           const double* rate, int B, const double* x0,
                                           const int32_t* market_of, int S, int N, double L,
                                           const dh_lb_options* opt, dh_lb_result* out,
                                           int32_t* n_launches) {
    if (!ctx || !s || !opt || (S > 0 && (!x0 || !out)) || (B > 0 && !mkt_iv))
        return fail(DH_E_ARG, "null argument");
    const int M = s->M;
    // the weights as the reduction reads them ([B][M], null: all 1) and each market's weight sum:
    // option order, sequential, from 0.0
    std::vector<double> w((size_t)std::max(B, 0) * M), wsum((size_t)std::max(B, 0), 0.0);
    for (int b = 0; b < B; ++b) {
        double acc = 0.0;
        for (int m = 0; m < M; ++m) {
            const size_t k = (size_t)b * M + m;
            const double wm = wgt ? wgt[k] : 1.0;
            if (!(wm >= 0.0) || !std::isfinite(wm))
                return fail(DH_E_ARG, "weight of market " + std::to_string(b) + " option " +
                                          std::to_string(m) + " is negative or not finite");
            if (wm > 0.0 && (!(mkt_iv[k] >= 0.0) || !std::isfinite(mkt_iv[k])))
                return fail(DH_E_ARG, "mkt_iv of market " + std::to_string(b) + " option " +
                                          std::to_string(m) +
                                          " is negative or not finite at a positive weight");
            w[k] = wm;
            acc += wm;
        }
        if (M > 0 && (!(acc > 0.0) || !std::isfinite(acc)))
            return fail(DH_E_ARG, "the weights of market " + std::to_string(b) +
                                      " sum to zero (or overflow)");
        wsum[b] = acc;
    }
    LbBatch bt{mkt_iv, spot, rate, B, market_of};
    bt.iv_wgt = w.data();
    bt.iv_wsum = wsum.data();
    return lb_run(ctx, s, x0, S, 0.0, 0.0, N, L, opt, out, n_launches, &bt);
}
