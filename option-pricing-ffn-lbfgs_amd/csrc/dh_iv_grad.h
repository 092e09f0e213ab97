// dh_iv_grad.h -- the implied-vol objective with its exact gradient against a market row per set
// (dh_surface_iv_grad_rows_dev, dh_surface_loss_iv_grad_rows*; the reduction of
// dh_calibrate_lbfgs_batch_iv_grad).  Included by dh_kernels.hip after
// dh_param_grad.h and ahead of the L-BFGS-B driver (dh_lb_driver.h); needs dh_iv.h, dh_iv_loss.h
// (vol_term, iv_check_weights), dh_loss_rows.h (rows_grid) and dh_param_grad.h: the planes and the
// analytic rows request (GradRows, rows_request_dev, rows_round_trip).  What is the vol objective's
// own stays here: the vega, the reduction kernel, its launches and the host form's weights and
// divisors.
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
// dhpg::loss_grad_wave's gradient sums and lane-0 end (transform_dt, feller_kink_grad).
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
#pragma unroll
    for (int k = 0; k < kN; ++k) {
        const double dt = transform_dt(k, rec);
        go[k] = c2 * gs[k] * dt;
    }
    feller_kink_grad(rec, go);
}

// the reduction's launch: behind dh_surface_iv_grad_rows_dev, stage 3 of a rows request and the
// vol-space analytic driver's iterations.  R.extra: the c_m plane [S][M].
int iv_grad_rows_launch(const dh_surface* s, const dhpg::GradRows& R, hipStream_t st) {
    hipLaunchKernelGGL(iv_grad_rows_kernel, dim3(rows_grid(R.S)), dim3(kBlockRows), 0, st,
                       (const double*)R.planes, R.rec, R.pen, (const double*)s->K,
                       (const double*)s->T, (const int8_t*)s->call, (const int*)s->perm, R.mkt, R.wgt, R.row, R.div, R.div_by_row ? 1 : 0,
                       s->strike_mode, s->M, (int64_t)R.S, R.live_count, R.extra, R.iv, R.f, R.g,
                       R.sse, R.bad);
    HIP_TRY(hipGetLastError());
    return DH_OK;
}

// Stages 2 and 3 of a rows request over records already on the device: param_grad_kernel,
// unchanged, into the planes, then the reduction.  The vol-space analytic driver's iteration.
int loss_iv_grad_rows_launch(dh_ctx* ctx, const dh_surface* s, const dhpg::GradRows& R, int N,
                             double L, hipStream_t st) {
    const int rc =
        dhpg::launch_param_grad(ctx, dhpg::surface_args(s, R.rec, R.S, N, L, R.planes), R.S, st);
    if (rc) return rc;
    return iv_grad_rows_launch(s, R, st);
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
    dhpg::GradRows R{};
    R.rec = d_params;
    R.pen = d_pen;
    R.planes = const_cast<double*>(d_planes);        // the caller's: this launch only reads them
    R.extra = (double*)ctx->pg_scratch.ptr;
    R.mkt = d_mkt_iv;
    R.wgt = d_wgt;
    R.row = (const int*)d_row;
    R.div = d_div;
    R.f = d_f;
    R.g = d_g;
    R.sse = d_sse;
    R.bad = (int*)d_n_bad;
    R.iv = d_iv;
    R.S = S;
    return dhivg::iv_grad_rows_launch(s, R, st);
}

extern "C" int dh_surface_loss_iv_grad_rows_dev(dh_ctx* ctx, const dh_surface* s,
                                                const double* d_x, const double* d_mkt_iv,
                                                const double* d_wgt, const double* d_div,
                                                const double* d_spot, const double* d_rate,
                                                const int32_t* d_row, int S, int N, double L,
                                                double* d_f, double* d_g, int32_t* d_bad,
                                                double* d_iv, void* stream) {
    dhpg::GradRows R{};
    R.mkt = d_mkt_iv;
    R.wgt = d_wgt;
    R.row = (const int*)d_row;
    R.div = d_div;
    R.f = d_f;
    R.g = d_g;
    R.bad = (int*)d_bad;
    R.iv = d_iv;
    R.S = S;
    return dhpg::rows_request_dev(
        ctx, s,
        {{d_x, "x"}, {d_mkt_iv, "mkt_iv"}, {d_wgt, "wgt"}, {d_div, "div"}, {d_spot, "spot"},
         {d_rate, "rate"}, {d_row, "row"}, {d_f, "f"}, {d_g, "g"}, {d_bad, "bad"}},
        d_x, d_spot, d_rate, R, dhpg::Scratch::kVol, dhivg::loss_iv_grad_rows_launch, N, L, stream);
}

extern "C" int dh_surface_loss_iv_grad_rows(dh_ctx* ctx, const dh_surface* s, const double* x,
                                            const double* mkt_iv, const double* wgt,
                                            const double* spot, const double* rate,
                                            const int32_t* row, int S, int B, int N, double L,
                                            double* f, double* g, int32_t* bad, double* iv) {
    // the weights as the reduction reads them ([B][M], null: all 1), each market's weight sum
    // (dh_calibrate_lbfgs_batch_iv's checks and order) and each set's divisor
    auto prep = [&](std::vector<double>& w, std::vector<double>& dv) -> int {
        std::vector<double> wsum((size_t)B, 0.0);
        w.resize((size_t)B * s->M);
        dv.resize((size_t)S);
        const int rc = iv_check_weights(mkt_iv, wgt, B, s->M, true, w.data(), wsum.data());
        if (rc) return rc;
        for (int i = 0; i < S; ++i) dv[i] = wsum[row[i]];
        return DH_OK;
    };
    return dhpg::rows_round_trip(
        ctx, s,
        {{x, "x"}, {mkt_iv, "mkt_iv"}, {spot, "spot"}, {rate, "rate"}, {row, "row"}, {f, "f"},
         {g, "g"}, {bad, "bad"}},
        dhpg::RowsIo{x, mkt_iv, nullptr, nullptr, spot, rate, row, f, g, bad, iv}, S, B,
        s ? (size_t)S * s->M : 0, N, L, prep, [&](const dhpg::RowsIo& d, hipStream_t st) {
            return dh_surface_loss_iv_grad_rows_dev(ctx, s, d.x, d.mkt, d.wgt, d.div, d.spot,
                                                    d.rate, d.row, S, N, L, d.f, d.g, d.bad,
                                                    d.extra, st);
        });
}
