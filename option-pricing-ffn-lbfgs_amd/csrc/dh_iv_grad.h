// dh_iv_grad.h -- the implied-vol objective with its exact gradient against a market row per set
// (dh_surface_iv_grad_rows_dev, dh_surface_loss_iv_grad_rows*; the reduction of
// dh_calibrate_lbfgs_batch_iv_grad).  Included by dh_kernels.hip after
// dh_param_grad.h and ahead of the L-BFGS-B driver (dh_lb_driver.h); needs dh_iv.h, dh_iv_loss.h
// (vol_term), dh_loss_rows.h (rows_grid) and dh_param_grad.h (the planes, x_records_rows_kernel).
//
// Definition.  The vol objective of dh_loss_rows.h, f = sum_m w_m (v_m - mkt_iv_m)^2 / sum(w) +
// Feller, v_m the Black-Scholes vol of the model price P_m.  v_m is defined by BS(v_m) = P_m, so
//     d v_m / d theta_i = (d P_m / d theta_i) / vega_BS(v_m),
// one chain-rule step from the planes param_grad_kernel writes, and
//     g_i = (2 / sum(w)) sum_m (w_m (v_m - mkt_iv_m) / vega_m) d P_m / d theta_i  d theta_i / d x_i
//           + d Feller / d x_i.
// The vega is closed-form in the inverter's own variables (dhiv::vega below).  A request inverts M
// prices where the forward quotient inverts 14 M, and no inverter noise is divided by a step.
//
// One-sided rule.  An option whose vol as used is 0.0 -- its price is at its lower bound, or a
// rounding below it (dhivl::below_lower's clamp) -- or whose vega is not > 0 (underflow) adds its
// residual to the loss and NOTHING to the gradient: on the clamp the vol does not move with the
// price to the one side, and its slope to the other is unbounded.  Like the Feller kink this is
// the derivative of the side on which the loss is flat.
#pragma once
#pragma clang fp contract(off)

namespace dhiv {

// Black-Scholes vega d price / d sigma at vol v, in implied_vol's variables: A = S0 e^{-qT}, B =
// K e^{-rT}, s = v sqrt(T), h = |x| / s with x from log1p as implied_vol forms it, t = s / 2:
//     vega = sqrt(A) sqrt(B) sqrt(T) phi(h) e^{-t^2/2}
// (b' = phi(h) e^{-t^2/2} of dh_iv.h, times the normalisation and ds / dsigma).  The same for a
// call and a put.  v = 0 gives h = inf (NaN at the money) and a vega that is not > 0; so does a
// NaN v.  Out of line, as mills and implied_vol: the body forms exp's and log1p's constants where
// it uses them and the calling loop holds none of them.
__device__ __noinline__ double vega(double v, double S0, double K, double T, double r, double q) {
    const double A = S0 * exp(-q * T), B = K * exp(-r * T);
    const double rT = sqrt(T);
    const double s = v * rT;
    const double h = fabs(log1p((S0 - K) / K) + (r - q) * T) / s;
    const double t = 0.5 * s;
    return sqrt(A) * sqrt(B) * rT * exp(-0.5 * (h * h + t * t) - kLnSqrt2Pi);
}

}  // namespace dhiv

// ---- the reduction ---------------------------------------------------------------------------------
// One wave per set, dhivr::iv_sse_rows_kernel's layout and rules (by its own text, dhivl::vol_term:
// bad prices, the clamp at the lower bound, a zero weight enters nothing, iv as used) and
// dhpg::loss_grad_wave's gradient sums and lane-0 expressions.
//
// Pass 1, every lane every pass (implied_vol's loop is wave-wide): lane l takes the surface's sorted
// options l, l + 64, ... from 0.0; a used option adds w (d d) to sse, uncontracted, and writes
//     c_m = w_m (v_m - mkt_iv_m) / vega_m      (0.0 under the one-sided rule, a zero weight, a bad
//                                               option)
// to the scratch plane cm [S][M] at its place in the caller's order.  Pass 2: the same lane reads
// its c_m back and adds c_m plane_i[m] to each of thirteen sums, again from 0.0 in the order l,
// l + 64, ...; a c_m of 0.0 is skipped by a branch, so nothing of an option that enters no
// gradient is read.  Then the xor butterfly (xor_sum) over sse and the thirteen sums.  The thirteen
// accumulators do not live across the out-of-line implied_vol: that is what the two passes are for.
//
// sse, n_bad and iv are dhivr::iv_sse_rows_kernel's terms in its order: fed plane 0 as its prices
// that kernel gives the same bits.  A set's outputs read nothing but its own record, planes,
// penalty and market row.
namespace dhivg {

constexpr int kN = dhpg::kPlanes - 1;

// div: the loss divisor, the weight sum of the set's market -- [S] per set, or with div_by_row
// [B] per market, read at row[s] (the driver's form: its sets move between slots).  live_count:
// the device-resident driver's count of unfinished starts (the launch is a no-op at 0), or null.
__global__ __launch_bounds__(kBlockRows, DH_IV_WAVES) void iv_grad_rows_kernel(
    const double* __restrict__ planes, const double* __restrict__ prm,
    const double* __restrict__ pen, const double* __restrict__ K, const double* __restrict__ T,
    const int8_t* __restrict__ call, const int* __restrict__ perm,
    const double* __restrict__ mkt_iv, const double* __restrict__ wgt,
    const int* __restrict__ row, const double* __restrict__ div, int div_by_row, int strike_mode,
    int M, int64_t S, const int* __restrict__ live_count, double* __restrict__ cm,
    double* __restrict__ iv, double* __restrict__ f, double* __restrict__ g,
    double* __restrict__ sse, int* __restrict__ n_bad) {
    if (live_count && __builtin_amdgcn_readfirstlane(*live_count) <= 0) return;
    const int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (s >= S) return;                              // whole waves: s is uniform across a wave
    const double* rec = prm + s * DH_PARAM_STRIDE;
    const double S0 = rec[13], r = rec[14], q = rec[15];
    const int64_t b = row[s];
    const double* mk = mkt_iv + b * M;
    const double* wg = wgt + b * M;
    double* cs = cm + s * M;
    double acc = 0.0;
    int bad = 0;
    for (int m0 = 0; m0 < M; m0 += 64) {             // every lane makes every pass
        const int i = m0 + lane;
        const dhivl::VolTerm t = dhivl::vol_term(S0, r, q, s, i, i < M, planes, K, T, call, perm,
                                                 mk, wg, strike_mode, M, iv);
        const int m = i < M ? i : 0;
        const double Kin = K[m];
        const double strike = strike_mode == DH_STRIKE_PCT_SPOT ? Kin * S0 / 100.0 : Kin;
        const double vg = dhiv::vega(t.v, S0, strike, T[m], r, q);
        const int c = perm[m];
        double cv = 0.0;
        if (t.bad) {
            bad += 1;
        } else if (t.w > 0.0) {
            acc = acc + t.term;
            if (t.v != 0.0 && vg > 0.0) cv = (t.w * (t.v - mk[c])) / vg;
        }
        if (i < M) cs[c] = cv;
    }
    const int64_t plane = S * (int64_t)M;
    const double* p = planes + s * M;
    double gs[kN];
#pragma unroll
    for (int k = 0; k < kN; ++k) gs[k] = 0.0;
    for (int m0 = 0; m0 < M; m0 += 64) {
        const int m = m0 + lane;
        if (m < M) {
            const int c = perm[m];
            const double cv = cs[c];                 // this lane's own store of pass 1
            if (cv != 0.0) {
#pragma unroll
                for (int k = 0; k < kN; ++k) gs[k] = gs[k] + cv * p[(k + 1) * plane + c];
            }
        }
    }
    acc = xor_sum(acc, 64);
#pragma unroll
    for (int k = 0; k < kN; ++k) gs[k] = xor_sum(gs[k], 64);
    for (int off = 1; off < 64; off <<= 1) bad += __shfl_xor(bad, off, 64);
    if (lane != 0) return;
    if (sse) sse[s] = acc;
    n_bad[s] = bad;
    double* go = g + s * kN;
    if (bad > 0) {                                   // the FD quotient of a constant 1e10
        f[s] = kInvalidLoss;
#pragma unroll
        for (int k = 0; k < kN; ++k) go[k] = 0.0;
        return;
    }
    const double dv = div[div_by_row ? b : s];
    f[s] = acc / dv + pen[s];
    const double c2 = 2.0 / dv;
    // dhpg::loss_grad_wave's transform and Feller expressions
#pragma unroll
    for (int k = 0; k < kN; ++k) {
        const double dt = (k == 4 || k == 9) ? 1.0 - rec[k] * rec[k] : (k == 11 ? 1.0 : rec[k]);
        go[k] = c2 * gs[k] * dt;
    }
#pragma unroll
    for (int fct = 0; fct < 2; ++fct) {
        const int o = 5 * fct;
        const double kap = rec[o + 1], th = rec[o + 2], sig = rec[o + 3];
        if (sig * sig - 2.0 * kap * th > 0.0) {
            go[o + 3] = go[o + 3] + 2000.0 * (sig * sig);
            go[o + 1] = go[o + 1] - 2000.0 * (kap * th);
            go[o + 2] = go[o + 2] - 2000.0 * (kap * th);
        }
    }
}

// the reduction's launch: behind dh_surface_iv_grad_rows_dev, stage 3 of a rows request and the
// vol-space analytic driver's iterations.  d_cm: [S][M] scratch.
int iv_grad_rows_launch(const dh_surface* s, const double* d_planes, const double* d_rec,
                        const double* d_pen, const double* d_mkt_iv, const double* d_wgt,
                        const int* d_row, const double* d_div, bool div_by_row, int S,
                        double* d_cm, double* d_f, double* d_g, double* d_sse, int* d_bad,
                        double* d_iv, hipStream_t st, const int* live_count) {
    hipLaunchKernelGGL(iv_grad_rows_kernel, dim3(rows_grid(S)), dim3(kBlockRows), 0, st, d_planes,
                       d_rec, d_pen, (const double*)s->K, (const double*)s->T,
                       (const int8_t*)s->call, (const int*)s->perm, d_mkt_iv, d_wgt, d_row, d_div,
                       div_by_row ? 1 : 0, s->strike_mode, s->M, (int64_t)S, live_count, d_cm,
                       d_iv, d_f, d_g, d_sse, d_bad);
    HIP_TRY(hipGetLastError());
    return DH_OK;
}

// Stages 2 and 3 of a rows request over records already on the device: param_grad_kernel,
// unchanged, into d_planes [14][S][M], then the reduction.  The vol-space analytic driver's
// iteration.
int loss_iv_grad_rows_launch(dh_ctx* ctx, const dh_surface* s, const double* d_rec,
                             const double* d_pen, const double* d_mkt_iv, const double* d_wgt,
                             const int* d_row, const double* d_div, bool div_by_row, int S, int N,
                             double L, double* d_planes, double* d_cm, double* d_f, double* d_g,
                             int* d_bad, double* d_iv, hipStream_t st, const int* live_count) {
    const int rc =
        dhpg::launch_param_grad(ctx, dhpg::surface_args(s, d_rec, S, N, L, d_planes), S, st);
    if (rc) return rc;
    return iv_grad_rows_launch(s, d_planes, d_rec, d_pen, d_mkt_iv, d_wgt, d_row, d_div,
                               div_by_row, S, d_cm, d_f, d_g, nullptr, d_bad, d_iv, st,
                               live_count);
}

// scratch of a request in the context's buffer: dhpg::loss_grad_scratch's records, penalties and
// planes, then the c_m plane [S][M]
size_t scratch_bytes(int S, int M) {
    return dhpg::loss_grad_scratch(S, M) + (size_t)S * M * 8;
}

}  // namespace dhivg

extern "C" int dh_surface_iv_grad_rows_dev(dh_ctx* ctx, const dh_surface* s,
                                           const double* d_planes, const double* d_params,
                                           const double* d_pen, const double* d_mkt_iv,
                                           const double* d_wgt, const int32_t* d_row,
                                           const double* d_div, int S, double* d_f, double* d_g,
                                           double* d_sse, int32_t* d_n_bad, double* d_iv,
                                           void* stream) {
    if (!ctx) return fail(DH_E_ARG, "ctx is null");
    if (!s) return fail(DH_E_ARG, "surface is null");
    if (S < 1) return fail(DH_E_ARG, "S must be >= 1, got " + std::to_string(S));
    if (s->M == 0) return fail(DH_E_ARG, "surface is empty (the loss is NaN)");
    if (!d_planes || !d_params || !d_pen || !d_mkt_iv || !d_wgt || !d_row || !d_div || !d_f ||
        !d_g || !d_n_bad)
        return fail(DH_E_ARG, "null argument");
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    // the c_m plane alone (the planes are the caller's); grow-only
    HIP_TRY(ctx->pg_scratch.reserve((size_t)S * s->M * 8));
    return dhivg::iv_grad_rows_launch(s, d_planes, d_params, d_pen, d_mkt_iv, d_wgt,
                                      (const int*)d_row, d_div, false, S,
                                      (double*)ctx->pg_scratch.ptr, d_f, d_g, d_sse,
                                      (int*)d_n_bad, d_iv, st, nullptr);
}

extern "C" int dh_surface_loss_iv_grad_rows_dev(dh_ctx* ctx, const dh_surface* s,
                                                const double* d_x, const double* d_mkt_iv,
                                                const double* d_wgt, const double* d_div,
                                                const double* d_spot, const double* d_rate,
                                                const int32_t* d_row, int S, int N, double L,
                                                double* d_f, double* d_g, int32_t* d_bad,
                                                double* d_iv, void* stream) {
    int rc = dhpg::check_loss_grad_rows(ctx, s, S, N, L);
    if (rc) return rc;
    if (!d_x) return fail(DH_E_ARG, "x is null");
    if (!d_mkt_iv) return fail(DH_E_ARG, "mkt_iv is null");
    if (!d_wgt) return fail(DH_E_ARG, "wgt is null");
    if (!d_div) return fail(DH_E_ARG, "div is null");
    if (!d_spot) return fail(DH_E_ARG, "spot is null");
    if (!d_rate) return fail(DH_E_ARG, "rate is null");
    if (!d_row) return fail(DH_E_ARG, "row is null");
    if (!d_f) return fail(DH_E_ARG, "f is null");
    if (!d_g) return fail(DH_E_ARG, "g is null");
    if (!d_bad) return fail(DH_E_ARG, "bad is null");
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    // dh_surface_loss_grad_rows_dev's scratch and layout, then the c_m plane
    HIP_TRY(ctx->pg_scratch.reserve(dhivg::scratch_bytes(S, s->M)));
    double* d_rec = (double*)ctx->pg_scratch.ptr;
    double* d_pen = d_rec + (size_t)S * DH_PARAM_STRIDE;
    double* d_planes = d_pen + S;
    double* d_cm = d_planes + (size_t)dhpg::kPlanes * S * s->M;
    hipLaunchKernelGGL(dhpg::x_records_rows_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256),
                       0, st, d_x, S, d_spot, d_rate, (const int*)d_row, d_rec, d_pen);
    HIP_TRY(hipGetLastError());
    return dhivg::loss_iv_grad_rows_launch(ctx, s, d_rec, d_pen, d_mkt_iv, d_wgt,
                                           (const int*)d_row, d_div, false, S, N, L, d_planes,
                                           d_cm, d_f, d_g, (int*)d_bad, d_iv, st, nullptr);
}

extern "C" int dh_surface_loss_iv_grad_rows(dh_ctx* ctx, const dh_surface* s, const double* x,
                                            const double* mkt_iv, const double* wgt,
                                            const double* spot, const double* rate,
                                            const int32_t* row, int S, int B, int N, double L,
                                            double* f, double* g, int32_t* bad, double* iv) {
    int rc = dhpg::check_loss_grad_rows(ctx, s, S, N, L);
    if (rc) return rc;
    if (!x) return fail(DH_E_ARG, "x is null");
    if (!mkt_iv) return fail(DH_E_ARG, "mkt_iv is null");
    if (!spot) return fail(DH_E_ARG, "spot is null");
    if (!rate) return fail(DH_E_ARG, "rate is null");
    if (!row) return fail(DH_E_ARG, "row is null");
    if (!f) return fail(DH_E_ARG, "f is null");
    if (!g) return fail(DH_E_ARG, "g is null");
    if (!bad) return fail(DH_E_ARG, "bad is null");
    rc = check_rows(row, S, B);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) {
        if (!std::isfinite(spot[b]) || !(spot[b] > 0.0))
            return fail(DH_E_ARG, "spot " + std::to_string(b) + " is not finite or not > 0");
        if (!std::isfinite(rate[b]))
            return fail(DH_E_ARG, "rate " + std::to_string(b) + " is not finite");
    }
    const int M = s->M;
    // the weights as the reduction reads them ([B][M], null: all 1), each market's weight sum
    // (dh_calibrate_lbfgs_batch_iv's checks and order) and each set's divisor
    std::vector<double> w((size_t)B * M), wsum((size_t)B, 0.0), dv((size_t)S);
    rc = iv_check_weights(mkt_iv, wgt, B, M, true, w.data(), wsum.data());
    if (rc) return rc;
    for (int i = 0; i < S; ++i) dv[i] = wsum[row[i]];
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    constexpr int kN = dhivg::kN;
    const size_t xb = (size_t)S * kN * 8, mb = (size_t)B * M * 8, ob = (size_t)S * M * 8;
    hipStream_t st = ctx->stream;
    DrainOnError drain{st};                          // w, dv are pageable: drained before they go
    // x [S][13], then f [S], g [S][13], div [S], spot [B], rate [B], bad [S]
    HIP_TRY(ctx->pg_io.reserve(2 * xb + (size_t)S * 24 + (size_t)B * 16));
    HIP_TRY(ctx->rows_mkt.reserve(mb));
    HIP_TRY(ctx->rows_wgt.reserve(mb));
    HIP_TRY(ctx->rows_row.reserve((size_t)S * 4));
    if (iv) HIP_TRY(ctx->iv.reserve(ob));
    double* d_x = (double*)ctx->pg_io.ptr;
    double* d_f = d_x + (size_t)S * kN;
    double* d_g = d_f + S;
    double* d_div = d_g + (size_t)S * kN;
    double* d_spot = d_div + S;
    double* d_rate = d_spot + B;
    int32_t* d_bad = (int32_t*)(d_rate + B);
    HIP_TRY(hipMemcpyAsync(d_x, x, xb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_div, dv.data(), (size_t)S * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_spot, spot, (size_t)B * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_rate, rate, (size_t)B * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->rows_mkt.ptr, mkt_iv, mb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->rows_wgt.ptr, w.data(), mb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->rows_row.ptr, row, (size_t)S * 4, hipMemcpyHostToDevice, st));
    rc = dh_surface_loss_iv_grad_rows_dev(ctx, s, d_x, (const double*)ctx->rows_mkt.ptr,
                                          (const double*)ctx->rows_wgt.ptr, d_div, d_spot, d_rate,
                                          (const int32_t*)ctx->rows_row.ptr, S, N, L, d_f, d_g,
                                          d_bad, iv ? (double*)ctx->iv.ptr : nullptr, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(f, d_f, (size_t)S * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(g, d_g, xb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(bad, d_bad, (size_t)S * 4, hipMemcpyDeviceToHost, st));
    if (iv) HIP_TRY(hipMemcpyAsync(iv, ctx->iv.ptr, ob, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    drain.armed = false;
    return DH_OK;
}
