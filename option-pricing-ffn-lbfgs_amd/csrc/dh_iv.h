// dh_iv.h -- Black-Scholes implied volatility on the device (dh_implied_vol, dh_implied_vol_dev,
// dh_surface_implied_vol).  Included by dh_kernels.hip after its host helpers.  DESIGN.md 3.10.
//
// One lane per quote (price, S0, K, T, r, q, is_call) -> sigma, structure of arrays, grid-stride,
// no LDS, no tables: HIP's own erfcx / exp / log for double (nothing here is bit-compared to
// NumPy).  The reference has no implied-vol code; this replaces the host root-finder a user of
// the price outputs runs per option.
//
// Formulation.  With A = S0 e^{-qT}, B = K e^{-rT} (the discounted legs), x = ln(A / B) = ln(F / K)
// and s = sigma sqrt(T), an in-the-money quote is replaced by its out-of-the-money twin by parity
// (time value = price - lower), and the twin's value is normalised by sqrt(A B):
//     beta = b(s) = e^{y/2} Phi(h + t) - e^{-y/2} Phi(h - t),   y = -|x|, h = y / s, t = s / 2.
// The two tail probabilities are never subtracted as such: with Mills' ratio R(z) = Phi(-z) / phi(z)
// = sqrt(pi / 2) erfcx(z / sqrt 2) the powers of e cancel exactly,
//     b = phi(h) e^{-t^2/2} I,    I = R(|h| - t) - R(|h| + t) = int_{|h|-t}^{|h|+t} (1 - z R(z)) dz,
// so ln b = -(h^2 + t^2) / 2 - ln sqrt(2 pi) + ln I holds its relative accuracy however deep out of
// the money the quote is, and b' = db/ds = phi(h) e^{-t^2/2}, i.e. I = b / b'.  For s >= kIvQuad the
// difference of the two R is formed directly (it cancels by ~|h| / s ulps at most); below, where
// the two arguments nearly coincide, the integral form is taken by 4-point Gauss-Legendre (its
// integrand 1 - z R(z) = -R'(z) is smooth; the rule's error is < 1e-15 of I at s = kIvQuad).
// x comes from log1p((S0 - K) / K) + (r - q) T: its absolute error scales with |x| and not with 1,
// which is what a deep out-of-the-money quote at a small s needs (d ln b / dx = |h| / s).
//
// Iteration.  Two closed-form starting points, one exact at the money / for large s, one the deep
// out-of-the-money asymptote; the better one starts a Halley iteration on ln b where h^2 > 2 and
// on b itself otherwise (the same root; each objective is close to linear on its side), inside a
// bracket [lo, hi] that every evaluation tightens; a step that leaves the bracket is replaced by
// its midpoint.  The loop is uniform: every lane runs it under a done mask and leaves after at
// most kIvCap evaluations whatever its input (no input can make the kernel spin); the wave leaves
// early when all its lanes are done.
#pragma once
#pragma clang fp contract(off)

namespace dhiv {

#ifndef DH_IV_WAVES
#define DH_IV_WAVES 4                   // min waves per SIMD: caps the kernels at 128 VGPRs
#endif
constexpr int kIvCap = 24;              // evaluations per quote after the two starting points
constexpr double kIvQuad = 0.1;         // s below which I is the Gauss-Legendre integral
constexpr double kEps = 2.220446049250313e-16;
constexpr double kRsqrt2 = 0.7071067811865476;
constexpr double kSqrtHalfPi = 1.2533141373155003;
constexpr double kLnSqrt2Pi = 0.9189385332046728;
constexpr double k2Sqrt2 = 2.8284271247461903;

// Mills' ratio.  Out of line, as implied_vol below: inlined, the compiler hoists the fp64 polynomial
// constants of erfcx, erfinv, log, exp ... (two VGPRs each, no inline form) out of the grid-stride
// and iteration loops and the kernels need > 256 VGPRs plus scratch; as calls, each body forms its
// constants where it uses them (120 VGPRs; the only scratch is the call frame's 16 bytes per lane).
__device__ __noinline__ double mills(double z) { return kSqrtHalfPi * erfcx(z * kRsqrt2); }

// I(s) = b / b' and ln b at s, for ay = |x|; h = ay / s is returned.  One loop over the nodes, not
// unrolled: the kernel carries a single copy of erfcx.
__device__ __forceinline__ double iv_eval(double ay, double s, double& lnb, double& h) {
    constexpr double x0 = 0.3399810435848563, x1 = 0.8611363115940526;   // 4-point Gauss-Legendre
    constexpr double w0 = 0.6521451548625461, w1 = 0.3478548451374538;
    h = ay / s;
    const double t = 0.5 * s;
    const bool quad = s < kIvQuad;
    double acc = 0.0;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        if (!quad && k >= 2) break;
        // quad: nodes -x1, -x0, x0, x1 of [|h| - t, |h| + t]; direct: the two ends
        const double xi = quad ? (k == 0 ? -x1 : (k == 1 ? -x0 : (k == 2 ? x0 : x1)))
                               : (k == 0 ? -1.0 : 1.0);
        const double z = h + xi * t;
        const double R = mills(z);
        acc += quad ? ((k == 0 || k == 3) ? w1 : w0) * (1.0 - z * R) : (k == 0 ? R : -R);
    }
    const double I = quad ? t * acc : acc;
    lnb = -0.5 * (h * h + t * t) - kLnSqrt2Pi + log(I);
    return I;
}

// sigma of one quote (include/dhcos.h, dh_implied_vol, has the table of results).  `active` is
// false for a lane past the end of the arrays: it takes no step and its result is unused, but it
// stays in the wave so the loop's exit test sees every lane.
__device__ __noinline__ double implied_vol(bool active, double price, double S0, double K,
                                              double T, double r, double q, bool is_call) {
    double result = __builtin_nan("");
    bool done = true;
    double ay = 0.0, lnbeta = 0.0, s = 1.0, s2 = 1.0, lo = 0.0, hi = 1.0, rsT = 1.0;
    // a > 0 also rejects NaN; isfinite rejects +-inf
    const bool valid = active && isfinite(price) && S0 > 0.0 && K > 0.0 && T > 0.0 &&
                       isfinite(S0) && isfinite(K) && isfinite(T) && isfinite(r) && isfinite(q);
    if (valid) {
        const double A = S0 * exp(-q * T), B = K * exp(-r * T);
        const double lower = is_call ? fmax(A - B, 0.0) : fmax(B - A, 0.0);
        const double upper = is_call ? A : B;
        const double norm = sqrt(A) * sqrt(B);
        if (!(A > 0.0) || !(B > 0.0) || !isfinite(A) || !isfinite(B) || !(norm > 0.0)) {
            // the discounted legs left fp64's range: no bounds to compare with
        } else if (price == lower) {
            result = 0.0;
        } else if (price > lower && price < upper) {
            const double beta = (price - lower) / norm;
            ay = fabs(log1p((S0 - K) / K) + (r - q) * T);
            lnbeta = log(beta);
            rsT = 1.0 / sqrt(T);
            // beyond hi the value is its s -> inf limit e^{-ay/2} to the last bit (t - |h| = 9)
            hi = 9.0 + sqrt(81.0 + 2.0 * ay);
            // start 1: exact at the money (b = erf(s / (2 sqrt 2))) and for large s
            const double a2 = 0.5 * ay;
            const double arg = fmin(beta / cosh(a2) + tanh(a2), 1.0 - 0.5 * kEps);
            s = fmin(fmax(k2Sqrt2 * erfinv(arg), 1e-300), hi);
            // start 2: ln b ~ -x^2 / (2 s^2) + 3 ln s - 2 ln|x| - ln sqrt(2 pi) deep out of the money
            s2 = s;
            if (ay > 0.0 && lnbeta < 0.0) {
                const double sa = ay / sqrt(-2.0 * lnbeta);
                const double d = -lnbeta + 3.0 * log(sa) - 2.0 * log(ay) - kLnSqrt2Pi;
                const double sb = d > 0.0 ? ay / sqrt(2.0 * d) : sa;
                if (sb > 0.0 && isfinite(sb)) s2 = fmin(fmax(sb, 1e-300), hi);
            }
            result = s * rsT;
            done = false;
        }
    }
    // evaluations 0 and 1 are the two starting points: each tightens the bracket and forms its
    // own step; the one nearer the root (smaller |ln beta - ln b|) goes on
    double d1 = 0.0, s1 = 0.0, sn1 = 0.0;
    bool conv1 = false;
#pragma unroll 1
    for (int it = 0; it < kIvCap + 2; ++it) {
        if (__all(done)) break;
        if (!done) {
            double lnb, h;
            const double I = iv_eval(ay, s, lnb, h);
            double dl = lnbeta - lnb;                 // > 0: s is below the root
            if (dl > 0.0) lo = fmax(lo, s);
            if (dl < 0.0) hi = fmin(hi, s);
            const double c = h * h / s - 0.25 * s;    // b'' / b'
            // Newton steps n = F / F' of F = ln b - ln beta and of F = b - beta, and Halley's
            // denominators 1 - n F'' / (2 F')
            const bool use_log = h * h > 2.0;
            const double n = use_log ? -dl * I : -I * expm1(dl);
            double den = use_log ? 1.0 + 0.5 * n * (1.0 - I * c) / I : 1.0 - 0.5 * n * c;
            den = fmin(fmax(den, 0.5), 2.0);
            const double ds = -n / den;
            // converged: the step or the residual is at the evaluation's own noise (ln b carries
            // ~eps (1 + (h^2 + t^2) / 2)); the negated tests also end a lane whose values went NaN
            bool conv = !(fabs(ds) > 2.0 * kEps * s) ||
                        !(fabs(dl) > 4.0 * kEps * (1.0 + 0.5 * (h * h + 0.25 * s * s)));
            double sn = s + ds;
            if (it == 0) {
                d1 = dl, s1 = s, sn1 = sn, conv1 = conv;
                s = s2;
            } else {
                if (it == 1 && !(fabs(dl) < fabs(d1))) s = s1, sn = sn1, conv = conv1;
                if (conv || !(hi - lo > 2.0 * kEps * s)) {
                    done = true;
                } else {
                    if (!(sn > lo) || !(sn < hi)) sn = 0.5 * (lo + hi);
                    s = sn;
                }
                result = s * rsT;
            }
        }
    }
    return result;
}

// structure-of-arrays form: quote i of n
__global__ __launch_bounds__(256, DH_IV_WAVES) void implied_vol_kernel(
    const double* __restrict__ price, const double* __restrict__ S0, const double* __restrict__ K,
    const double* __restrict__ T, const double* __restrict__ r, const double* __restrict__ q,
    const int8_t* __restrict__ is_call, int64_t n, double* __restrict__ sigma) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // whole waves stay in the loop (implied_vol's exit test is over the wave)
    const int64_t n_up = (n + 63) / 64 * 64;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_up; i += stride) {
        const bool active = i < n;
        const int64_t j = active ? i : 0;
        const double v = implied_vol(active, price[j], S0[j], K[j], T[j], r[j], q[j],
                                     is_call[j] != 0);
        if (active) sigma[i] = v;
    }
}

// surface form: the price of sorted option i under param set p sits at prices[p * M + perm[i]];
// S0, r, q from the record's slots 13..15, the strike formed as the pricing kernels form it
__global__ __launch_bounds__(256, DH_IV_WAVES) void surface_implied_vol_kernel(
    const double* __restrict__ prices, const double* __restrict__ prm,
    const double* __restrict__ K, const double* __restrict__ T, const int8_t* __restrict__ call,
    const int* __restrict__ perm, int strike_mode, int M, int64_t n, double* __restrict__ iv) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t n_up = (n + 63) / 64 * 64;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_up; i += stride) {
        const bool active = i < n;
        const int64_t j = active ? i : 0;
        const int64_t p = j / M;
        const int m = (int)(j - p * M);
        const double* rec = prm + p * DH_PARAM_STRIDE;
        const double S0 = rec[13];
        const double Kin = K[m];
        const double strike = strike_mode == DH_STRIKE_PCT_SPOT ? Kin * S0 / 100.0 : Kin;
        const int64_t o = p * M + perm[m];
        const double v = implied_vol(active, prices[o], S0, strike, T[m], rec[14], rec[15],
                                     call[m] != 0);
        if (active) iv[o] = v;
    }
}

// <= 2048 blocks of 256 lanes (8 per CU), grid-stride past that
inline unsigned iv_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 2048); }

}  // namespace dhiv

extern "C" int dh_implied_vol_dev(dh_ctx* ctx, const double* d_price, const double* d_S0,
                                  const double* d_K, const double* d_T, const double* d_r,
                                  const double* d_q, const int8_t* d_is_call, int64_t n,
                                  double* d_sigma, void* stream) {
    if (!ctx) return fail(DH_E_ARG, "ctx is null");
    if (n < 0) return fail(DH_E_ARG, "n < 0");
    if (n > 0 && (!d_price || !d_S0 || !d_K || !d_T || !d_r || !d_q || !d_is_call || !d_sigma))
        return fail(DH_E_ARG, "null argument");
    if (n == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    hipLaunchKernelGGL(dhiv::implied_vol_kernel, dim3(dhiv::iv_blocks(n)), dim3(256), 0, st,
                       d_price, d_S0, d_K, d_T, d_r, d_q, d_is_call, n, d_sigma);
    HIP_TRY(hipGetLastError());
    return DH_OK;
}

extern "C" int dh_implied_vol(dh_ctx* ctx, const double* price, const double* S0, const double* K,
                              const double* T, const double* r, const double* q,
                              const int8_t* is_call, int64_t n, double* sigma) {
    if (!ctx) return fail(DH_E_ARG, "ctx is null");
    if (n < 0) return fail(DH_E_ARG, "n < 0");
    if (n > 0 && (!price || !S0 || !K || !T || !r || !q || !is_call || !sigma))
        return fail(DH_E_ARG, "null argument");
    if (n == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    // chunks of <= 4M quotes bound the device scratch (7 double columns and the flags per chunk)
    constexpr int64_t kChunk = int64_t(1) << 22;
    const int64_t cap = std::min(n, kChunk);
    const size_t col = ((size_t)cap * 8 + 255) & ~(size_t)255;
    HIP_TRY(ctx->iv.reserve(8 * col));
    char* base = (char*)ctx->iv.ptr;
    double* d[7];
    for (int k = 0; k < 7; ++k) d[k] = (double*)(base + k * col);
    int8_t* d_call = (int8_t*)(base + 7 * col);
    hipStream_t st = ctx->stream;
    const double* src[6] = {price, S0, K, T, r, q};
    for (int64_t i0 = 0; i0 < n; i0 += kChunk) {
        const int64_t m = std::min(kChunk, n - i0);
        for (int k = 0; k < 6; ++k)
            HIP_TRY(hipMemcpyAsync(d[k], src[k] + i0, (size_t)m * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_call, is_call + i0, (size_t)m, hipMemcpyHostToDevice, st));
        const int rc = dh_implied_vol_dev(ctx, d[0], d[1], d[2], d[3], d[4], d[5], d_call, m, d[6],
                                          st);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(sigma + i0, d[6], (size_t)m * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}

extern "C" int dh_surface_implied_vol(dh_ctx* ctx, const dh_surface* s, const double* params,
                                      int64_t P, int N, double L, double* iv, double* prices) {
    if (!ctx || !s || (P > 0 && (!params || !iv))) return fail(DH_E_ARG, "null argument");
    int rc = check_N(N);
    if (rc) return rc;
    if (P < 0) return fail(DH_E_ARG, "P < 0");
    if (P == 0 || s->M == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const int64_t n = P * s->M;
    const size_t pb = (size_t)P * DH_PARAM_STRIDE * 8, ob = (size_t)n * 8;
    HIP_TRY(ctx->params.reserve(pb));
    HIP_TRY(ctx->out.reserve(ob));
    HIP_TRY(ctx->iv.reserve(ob));
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(ctx->params.ptr, params, pb, hipMemcpyHostToDevice, st));
    // the prices of dh_surface_price: the same request, the same kernels
    rc = dh_surface_price_dev(ctx, s, (const double*)ctx->params.ptr, P, N, L,
                              (double*)ctx->out.ptr, st);
    if (rc) return rc;
    hipLaunchKernelGGL(dhiv::surface_implied_vol_kernel, dim3(dhiv::iv_blocks(n)), dim3(256), 0,
                       st, (const double*)ctx->out.ptr, (const double*)ctx->params.ptr, s->K, s->T,
                       s->call, s->perm, s->strike_mode, s->M, n, (double*)ctx->iv.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(iv, ctx->iv.ptr, ob, hipMemcpyDeviceToHost, st));
    if (prices) HIP_TRY(hipMemcpyAsync(prices, ctx->out.ptr, ob, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}
