// dh_loss_rows.h -- the relative-price loss against per-set market rows (dh_surface_loss_rows_dev,
// dh_surface_loss_rows): the reduction of the batched multi-market calibration
// (dh_calibrate_lbfgs_batch).  Included by dh_kernels.hip ahead of the L-BFGS-B driver.
// DESIGN.md 3.12.
//
// A stage beside the request kernels, as dh_iv_loss.h's: it reads the [S][M] prices a pricing
// request wrote (the caller's option order) and reduces each set against the market row its start
// belongs to,
//     sse[s] = sum_m ((p_sm - mkt[row[s]][m]) / mkt[row[s]][m])^2,
//     n_bad[s] = #{m : p_sm NaN, +-inf or <= 0}
// -- dh_surface_loss's rules: a zero market price gives inf (NaN where the price is 0 too), a NaN
// one NaN.
//
// Summation order.  One wave per set.  Lane l starts from 0.0 and adds the terms of options l,
// l + 64, l + 128, ... in that order (a lane with no option keeps 0.0); then the xor butterfly over
// the 64 lanes, offsets 1, 2, 4, 8, 16, 32 (xor_sum: both partners add the same two operands).
// Nothing is contracted into an FMA.  The order is a function of M alone: not of S, of the set's
// place in the request, of its row or of the stream.  No atomics, no hand-off between waves.
#pragma once
#pragma clang fp contract(off)

namespace dhrows {

constexpr int kBlockRows = 256;     // four waves, four sets per block

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
    const int64_t nb = ((int64_t)S * 64 + dhrows::kBlockRows - 1) / dhrows::kBlockRows;
    hipLaunchKernelGGL(dhrows::loss_rows_kernel, dim3((unsigned)nb), dim3(dhrows::kBlockRows), 0,
                       st, d_prices, d_mkt, (const int*)d_row, s->M, (int64_t)S, live_count, d_sse,
                       (int*)d_n_bad);
    HIP_TRY(hipGetLastError());
    return DH_OK;
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
    HIP_TRY(ctx->rows_row.reserve((size_t)S * 4));
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(ctx->params.ptr, params, pb, hipMemcpyHostToDevice, st));
    if (M > 0) HIP_TRY(hipMemcpyAsync(ctx->rows_mkt.ptr, mkt, mb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->rows_row.ptr, row, (size_t)S * 4, hipMemcpyHostToDevice, st));
    if (M > 0) {
        rc = dh_surface_price_dev(ctx, s, (const double*)ctx->params.ptr, S, N, L,
                                  (double*)ctx->out.ptr, st);
        if (rc) return rc;
    }
    // M == 0: nothing is priced and the stage reads neither prices nor market rows
    rc = loss_rows_launch(ctx, s, (const double*)(M > 0 ? ctx->out.ptr : ctx->params.ptr),
                          (const double*)(M > 0 ? ctx->rows_mkt.ptr : ctx->params.ptr),
                          (const int32_t*)ctx->rows_row.ptr, S, (double*)ctx->sse.ptr,
                          (int32_t*)ctx->bad.ptr, st, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(sse, ctx->sse.ptr, (size_t)S * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(n_bad, ctx->bad.ptr, (size_t)S * 4, hipMemcpyDeviceToHost, st));
    if (prices && M > 0)
        HIP_TRY(hipMemcpyAsync(prices, ctx->out.ptr, ob, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}
