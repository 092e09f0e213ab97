// dh_iv_loss.h -- the calibration objective in implied-vol space (dh_surface_set_iv_market,
// dh_surface_iv_sse_dev, dh_surface_loss_iv_dev, dh_surface_loss_iv), and what the loss stages
// share: one option's vol term (vol_term), the weight checks (iv_check_weights) and the host
// scaffolding of a stage (loss_round_trip, on dh_host.h's loss_stage; dh_loss_rows.h too).  Included by
// dh_kernels.hip after dh_iv.h.  DESIGN.md 3.11, 3.14.
//
// A stage beside the request kernels: it reads the [S][M] prices a pricing request wrote
// (dh_surface_price_dev, untouched), inverts each with dhiv::implied_vol -- the device function of
// dh_surface_implied_vol, so a finite vol here has that call's bits -- and reduces
//     sse[s] = sum_m w_m (v_sm - mkt_iv_m)^2,   n_bad[s] = #{m : w_m > 0, option m has no vol}.
// One lane per (set, option), blocks of 256 lanes over a 1-D grid of (tiles of 256 sorted options)
// x S, whole blocks inside implied_vol's loop (a lane past M is passed as inactive).
//
// Summation order.  Within a wave the xor butterfly (xor_sum), the block's four wave sums left to
// right, then the set's tile partials left to right (iv_sse_sum_kernel, one lane per set; a
// one-tile surface writes sse / n_bad from the first launch).  The order is a function of M and
// the surface's option sort alone: not of S, of the set's place in the request, of the stream or
// of the run.  No atomics, no hand-off between blocks.
#pragma once
#pragma clang fp contract(off)

namespace dhivl {

constexpr int kBlockIv = 256;

// true where implied_vol's NaN for this (valid, finite, positive) price means price < lower: the
// bound formed exactly as dh_iv.h forms it, behind the same validity tests
__device__ __forceinline__ bool below_lower(double price, double S0, double K, double T, double r,
                                            double q, bool is_call) {
    const bool valid = S0 > 0.0 && K > 0.0 && T > 0.0 && isfinite(S0) && isfinite(K) &&
                       isfinite(T) && isfinite(r) && isfinite(q);
    if (!valid) return false;
    const double A = S0 * exp(-q * T), B = K * exp(-r * T);
    const double lower = is_call ? fmax(A - B, 0.0) : fmax(B - A, 0.0);
    const double norm = sqrt(A) * sqrt(B);
    if (!(A > 0.0) || !(B > 0.0) || !isfinite(A) || !isfinite(B) || !(norm > 0.0)) return false;
    return price < lower;
}

struct VolTerm {
    double v;       // the option's vol (NaN: none)
    double w;       // its weight (0.0 for a lane past M)
    double term;    // w (v - mkt_iv)^2, where it enters the sum (w > 0, a vol); else 0.0
    bool bad;       // w > 0 and no vol
};

// One option's part of set p's vol loss, for both reductions (surface_iv_sse_kernel and
// dhivr::iv_sse_rows_kernel, which differ in how they accumulate it): sorted option i under the
// set's spot, rate and q (rec[13..15]); active: i < M (an inactive lane still makes implied_vol's
// wave-wide loop).  mk / wg: the market vols and weights the set is held against, in the caller's
// option order; iv: [S][M] for the vols, or null.
__device__ __forceinline__ VolTerm vol_term(double S0, double r, double q, int64_t p, int i,
                                            bool active, const double* __restrict__ prices,
                                            const double* __restrict__ K,
                                            const double* __restrict__ T,
                                            const int8_t* __restrict__ call,
                                            const int* __restrict__ perm,
                                            const double* __restrict__ mk,
                                            const double* __restrict__ wg, int strike_mode, int M,
                                            double* __restrict__ iv) {
    const int m = active ? i : 0;
    const double Kin = K[m], Tm = T[m];
    const bool is_call = call[m] != 0;
    const double strike = strike_mode == DH_STRIKE_PCT_SPOT ? Kin * S0 / 100.0 : Kin;
    const int c = perm[m];                          // the option's place in the caller's order
    const int64_t o = p * M + c;
    const double price = prices[o];
    // dh_surface_loss's rule: NaN, +-inf and <= 0 are bad prices (a > 0 also rejects NaN)
    const bool priced = active && price > 0.0 && isfinite(price);
    double v = dhiv::implied_vol(priced, price, S0, strike, Tm, r, q, is_call);
    // a model price a rounding below its lower bound: the vol's continuous extension
    if (priced && v != v && below_lower(price, S0, strike, Tm, r, q, is_call)) v = 0.0;
    if (active && iv) iv[o] = v;
    double term = 0.0;
    bool bad = false;
    const double w = active ? wg[c] : 0.0;
    if (w > 0.0) {                                  // a zero weight: nothing enters the sums
        if (v != v) {
            bad = true;
        } else {
            const double d = v - mk[c];
            term = w * (d * d);
        }
    }
    return {v, w, term, bad};
}

// block b: tile b % tiles of param set b / tiles.  part_sse / part_bad: [S][tiles].
__global__ __launch_bounds__(kBlockIv, DH_IV_WAVES) void surface_iv_sse_kernel(
    const double* __restrict__ prices, const double* __restrict__ prm,
    const double* __restrict__ K, const double* __restrict__ T, const int8_t* __restrict__ call,
    const int* __restrict__ perm, const double* __restrict__ mkt_iv,
    const double* __restrict__ wgt, int strike_mode, int M, int tiles, double* __restrict__ iv,
    double* __restrict__ part_sse, int* __restrict__ part_bad) {
    __shared__ double s_sse[kBlockIv / 64];
    __shared__ int s_bad[kBlockIv / 64];
    const int64_t p = blockIdx.x / (unsigned)tiles;
    const int tile = (int)(blockIdx.x - (unsigned)(p * tiles));
    const int i = tile * kBlockIv + (int)threadIdx.x;
    const double* rec = prm + p * DH_PARAM_STRIDE;
    const double S0 = rec[13], r = rec[14], q = rec[15];
    const VolTerm t = vol_term(S0, r, q, p, i, i < M, prices, K, T, call, perm, mkt_iv, wgt,
                               strike_mode, M, iv);
    const double wave_sse = xor_sum(t.term, 64);
    const int wave_bad = (int)__popcll(__ballot(t.bad));
    if ((threadIdx.x & 63) == 0) {
        s_sse[threadIdx.x >> 6] = wave_sse;
        s_bad[threadIdx.x >> 6] = wave_bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = s_sse[0];
        int nb = s_bad[0];
        for (int k = 1; k < kBlockIv / 64; ++k) acc += s_sse[k], nb += s_bad[k];
        part_sse[blockIdx.x] = acc;
        part_bad[blockIdx.x] = nb;
    }
}

// one lane per param set: its tile partials, left to right
__global__ __launch_bounds__(64) void iv_sse_sum_kernel(const double* __restrict__ part_sse,
                                                        const int* __restrict__ part_bad,
                                                        int tiles, int S, double* __restrict__ sse,
                                                        int* __restrict__ n_bad) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= S) return;
    const double* ps = part_sse + (int64_t)s * tiles;
    const int* pb = part_bad + (int64_t)s * tiles;
    double acc = ps[0];
    int nb = pb[0];
    for (int t = 1; t < tiles; ++t) acc += ps[t], nb += pb[t];
    sse[s] = acc;
    n_bad[s] = nb;
}

}  // namespace dhivl

namespace {     // host scaffolding of the loss stages

// Checks a [B][M] block of weights (null: all 1) against its market vols, writes the weights to
// w [B][M] and each row's sum to wsum [B]: option order, sequential, from 0.0 (the vol
// objective's divisor, so part of the result's bits).  per_market: the messages name the market
// as well as the option.
int iv_check_weights(const double* mkt_iv, const double* wgt, int B, int M, bool per_market,
                     double* w, double* wsum) {
    for (int b = 0; b < B; ++b) {
        auto of_b = [&] { return per_market ? " of market " + std::to_string(b) : ""; };
        auto at = [&](int m) {
            return of_b() + (per_market ? " option " : " ") + std::to_string(m);
        };
        double acc = 0.0;
        for (int m = 0; m < M; ++m) {
            const size_t k = (size_t)b * M + m;
            const double wm = wgt ? wgt[k] : 1.0;
            if (!(wm >= 0.0) || !std::isfinite(wm))
                return fail(DH_E_ARG, "weight" + at(m) + " is negative or not finite");
            if (wm > 0.0 && (!(mkt_iv[k] >= 0.0) || !std::isfinite(mkt_iv[k])))
                return fail(DH_E_ARG,
                            "mkt_iv" + at(m) + " is negative or not finite at a positive weight");
            w[k] = wm;
            acc += wm;
        }
        if (M > 0 && (!(acc > 0.0) || !std::isfinite(acc)))
            return fail(DH_E_ARG, "the weights" + of_b() + " sum to zero (or overflow)");
        wsum[b] = acc;
    }
    return DH_OK;
}

// an early error return leaves no launch or copy of ours on the stream
struct DrainOnError {
    hipStream_t st;
    bool armed = true;
    ~DrainOnError() {
        if (armed) (void)hipStreamSynchronize(st);
    }
};

// the per-set market rows of the *_rows host entry points (host arrays): mkt [B][M], the row of
// each set [S], and where `weighted` wgt [B][M] (null: every weight 1)
struct HostRows {
    const double* mkt;
    const double* wgt;
    const int32_t* row;
    int B;
    bool weighted;
};

// what loss_round_trip hands its stage, all device memory (mkt / wgt / row: null without rows)
struct StageIn {
    const double *params, *prices, *mkt, *wgt;
    const int32_t* row;
    double* sse;
    int32_t* n_bad;
    double* iv;
    hipStream_t st;
};

// The host entry points' round trip (S > 0): upload the records and the rows, price the records,
// run the device stage on the prices, download sse / n_bad and the optional prices / vols,
// synchronise.  Every error return drains the stream before `ones`, which it may still be
// copying from, is freed: `ones` is declared ahead of the guard, so it is destroyed after it.
template <typename Stage>
int loss_round_trip(dh_ctx* ctx, const dh_surface* s, const double* params, const HostRows* rows,
                    int S, int N, double L, double* sse, int32_t* n_bad, double* prices,
                    double* iv, Stage&& stage) {
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const int M = s->M;
    const bool weighted = rows && rows->weighted;
    const size_t pb = (size_t)S * DH_PARAM_STRIDE * 8, ob = (size_t)S * M * 8;
    const size_t mb = rows ? (size_t)rows->B * M * 8 : 0;
    hipStream_t st = ctx->stream;
    std::vector<double> ones;                        // wgt null: every weight 1 (pageable)
    DrainOnError drain{st};                          // after `ones`: unwinding drains first
    HIP_TRY(ctx->params.reserve(pb));
    HIP_TRY(ctx->sse.reserve((size_t)S * 8));
    HIP_TRY(ctx->bad.reserve((size_t)S * 4));
    HIP_TRY(ctx->out.reserve(ob));
    if (rows) {
        HIP_TRY(ctx->rows_mkt.reserve(mb));
        HIP_TRY(ctx->rows_row.reserve((size_t)S * 4));
    }
    if (weighted) HIP_TRY(ctx->rows_wgt.reserve(mb));
    if (iv) HIP_TRY(ctx->iv.reserve(ob));
    const double* wgt = weighted ? rows->wgt : nullptr;
    if (weighted && !wgt && M > 0) {
        ones.assign((size_t)rows->B * M, 1.0);
        wgt = ones.data();
    }
    HIP_TRY(hipMemcpyAsync(ctx->params.ptr, params, pb, hipMemcpyHostToDevice, st));
    if (rows && M > 0)
        HIP_TRY(hipMemcpyAsync(ctx->rows_mkt.ptr, rows->mkt, mb, hipMemcpyHostToDevice, st));
    if (weighted && M > 0)
        HIP_TRY(hipMemcpyAsync(ctx->rows_wgt.ptr, wgt, mb, hipMemcpyHostToDevice, st));
    if (rows)
        HIP_TRY(hipMemcpyAsync(ctx->rows_row.ptr, rows->row, (size_t)S * 4, hipMemcpyHostToDevice,
                               st));
    const double* d_params = (const double*)ctx->params.ptr;
    int rc = M > 0 ? dh_surface_price_dev(ctx, s, d_params, S, N, L, (double*)ctx->out.ptr, st)
                   : DH_OK;
    if (rc) return rc;
    // M == 0: nothing is priced and the stage reads neither prices nor market rows; the records
    // stand in for the arrays it only checks against null
    auto dev = [&](bool used, const DevBuf& b) {
        return !used ? nullptr : M > 0 ? (const double*)b.ptr : d_params;
    };
    rc = stage(StageIn{d_params, dev(true, ctx->out), dev(rows, ctx->rows_mkt),
                       dev(weighted, ctx->rows_wgt),
                       rows ? (const int32_t*)ctx->rows_row.ptr : nullptr, (double*)ctx->sse.ptr,
                       (int32_t*)ctx->bad.ptr, iv && M > 0 ? (double*)ctx->iv.ptr : nullptr, st});
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(sse, ctx->sse.ptr, (size_t)S * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(n_bad, ctx->bad.ptr, (size_t)S * 4, hipMemcpyDeviceToHost, st));
    if (M > 0) {
        if (prices) HIP_TRY(hipMemcpyAsync(prices, ctx->out.ptr, ob, hipMemcpyDeviceToHost, st));
        if (iv) HIP_TRY(hipMemcpyAsync(iv, ctx->iv.ptr, ob, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    drain.armed = false;
    return DH_OK;
}

}  // namespace

extern "C" int dh_surface_set_iv_market(dh_surface* s, const double* mkt_iv,
                                        const double* weight) {
    if (!s || !s->ctx) return fail(DH_E_ARG, "surface is null");
    const int M = s->M;
    if (M > 0 && !mkt_iv) return fail(DH_E_ARG, "mkt_iv is null");
    // [0, M): vols, [M, 2M): weights, both in the caller's option order
    std::vector<double> stage((size_t)2 * M);
    double wsum = 0.0;
    const int rc = iv_check_weights(mkt_iv, weight, 1, M, false, stage.data() + M, &wsum);
    if (rc) return rc;
    std::copy(mkt_iv, mkt_iv + M, stage.begin());
    DeviceScope dev_scope(s->ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    if (!s->iv_block) HIP_TRY(hipMalloc(&s->iv_block, std::max<size_t>((size_t)2 * M * 8, 16)));
    if (M > 0) {
        // a request that still reads the previous vols ends first
        HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        HIP_TRY(hipMemcpy(s->iv_block, stage.data(), (size_t)2 * M * 8, hipMemcpyHostToDevice));
    }
    s->iv_mkt = (double*)s->iv_block;
    s->iv_wgt = (double*)s->iv_block + M;
    s->has_iv = true;
    return DH_OK;
}

extern "C" int dh_surface_iv_sse_dev(dh_ctx* ctx, const dh_surface* s, const double* d_params,
                                     const double* d_prices, int S, double* d_sse,
                                     int32_t* d_n_bad, double* d_iv, void* stream) {
    if (!ctx || !s || (S > 0 && (!d_params || !d_prices || !d_sse || !d_n_bad)))
        return fail(DH_E_ARG, "null argument");
    if (!s->has_iv) return fail(DH_E_ARG, "surface has no market vols (dh_surface_set_iv_market)");
    return loss_stage(ctx, s, S, d_sse, d_n_bad, stream, [&](hipStream_t st) -> int {
        const int tiles = (s->M + dhivl::kBlockIv - 1) / dhivl::kBlockIv;
        const int64_t nb = (int64_t)tiles * S;
        if (nb > 0x7fffffffLL) return fail(DH_E_ARG, "launch too large");
        double* part_sse = d_sse;
        int* part_bad = (int*)d_n_bad;
        if (tiles > 1) {
            HIP_TRY(ctx->iv_part_sse.reserve((size_t)nb * 8));
            HIP_TRY(ctx->iv_part_bad.reserve((size_t)nb * 4));
            part_sse = (double*)ctx->iv_part_sse.ptr;
            part_bad = (int*)ctx->iv_part_bad.ptr;
        }
        hipLaunchKernelGGL(dhivl::surface_iv_sse_kernel, dim3((unsigned)nb),
                           dim3(dhivl::kBlockIv), 0, st, d_prices, d_params, s->K, s->T, s->call,
                           s->perm, s->iv_mkt, s->iv_wgt, s->strike_mode, s->M, tiles, d_iv,
                           part_sse, part_bad);
        HIP_TRY(hipGetLastError());
        if (tiles > 1) {
            hipLaunchKernelGGL(dhivl::iv_sse_sum_kernel, dim3((unsigned)((S + 63) / 64)),
                               dim3(64), 0, st, (const double*)part_sse, (const int*)part_bad,
                               tiles, S, d_sse, (int*)d_n_bad);
            HIP_TRY(hipGetLastError());
        }
        return DH_OK;
    });
}

extern "C" int dh_surface_loss_iv_dev(dh_ctx* ctx, const dh_surface* s, const double* d_params,
                                      int S, int N, double L, double* d_sse, int32_t* d_n_bad,
                                      double* d_prices, double* d_iv, void* stream) {
    if (!ctx || !s || (S > 0 && (!d_params || !d_sse || !d_n_bad)))
        return fail(DH_E_ARG, "null argument");
    if (!s->has_iv) return fail(DH_E_ARG, "surface has no market vols (dh_surface_set_iv_market)");
    int rc = check_N(N);
    if (rc) return rc;
    if (S < 0) return fail(DH_E_ARG, "S < 0");
    if (S == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    if (!d_prices && s->M > 0) {
        HIP_TRY(ctx->out.reserve((size_t)S * s->M * 8));
        d_prices = (double*)ctx->out.ptr;
    }
    if (s->M > 0) {
        rc = dh_surface_price_dev(ctx, s, d_params, S, N, L, d_prices, stream);
        if (rc) return rc;
    }
    // M == 0: nothing is priced and the stage reads no price
    return dh_surface_iv_sse_dev(ctx, s, d_params, s->M > 0 ? d_prices : d_params, S, d_sse,
                                 d_n_bad, d_iv, stream);
}

extern "C" int dh_surface_loss_iv(dh_ctx* ctx, const dh_surface* s, const double* params, int S,
                                  int N, double L, double* sse, int32_t* n_bad, double* prices,
                                  double* iv) {
    if (!ctx || !s || (S > 0 && (!params || !sse || !n_bad))) return fail(DH_E_ARG, "null argument");
    if (!s->has_iv) return fail(DH_E_ARG, "surface has no market vols (dh_surface_set_iv_market)");
    int rc = check_N(N);
    if (rc) return rc;
    if (S < 0) return fail(DH_E_ARG, "S < 0");
    if (S == 0) return DH_OK;
    return loss_round_trip(ctx, s, params, nullptr, S, N, L, sse, n_bad, prices, iv,
                           [&](const StageIn& d) {
                               return dh_surface_iv_sse_dev(ctx, s, d.params, d.prices, S, d.sse,
                                                            d.n_bad, d.iv, d.st);
                           });
}
