// dh_mc.h -- Monte Carlo path pricer of the Double-Heston + Merton-jump model: the walk and every
// kernel that prices from it (dh_mc_price*, dh_mc_price_vr*, dh_mc_paths, dh_mc_paths_vr).  Included
// by dh_kernels.hip after its host helpers; includes dh_mc_vr.h, the control variate's own parts.
// DESIGN.md 3.15 is the contract of the scheme and 3.15.2 of the variance reduction;
// tests/mc_reference.py and tests/mc_vr_reference.py restate them in NumPy.
//
// One path per lane on the uniform grid dt = 1 / steps_per_year.  Per step and path, in this
// order: each variance factor by Andersen's quadratic-exponential scheme and its log-spot
// increment with central weights, then the compound-Poisson jump, then the running maximum,
// minimum and sum of S.  The random numbers of (seed, path, step) are five Philox4x32-10 blocks
// (counter: path low, path high, step, block), so a path does not depend on the launch, on the
// number of paths or on the other parameter sets of the call, which all see the same draws.
//
// Arithmetic is uncontracted fp64 in the document's operation order: the NumPy restatement then
// differs only by the last bits of exp / log / sincos.  exp, log, sqrt and the divisions are the
// compiler's (correctly rounded sqrt and division; exp and log within 1 ulp and with no table to
// stage); sincos is dh::dsincos -- the compiler's inlines its large-argument reduction at every
// call site (~100 VGPRs, dh_device.h) for arguments that here never leave [0, 2 pi).
//
// Under the antithetic flag a lane walks path i and its mirror side by side: one set of Philox
// blocks and one Box-Muller per step, applied as (U, Z) to the path and as (1 - U, -Z) to the
// mirror (1 - U is exact: U is an odd multiple of 2^-53).  The sample of the pair is the average of
// the two payoffs.  The step, the price kernel and the paths kernel are templates over that flag,
// so the plain pricer is the instantiation without it and there is one walk to change.
#pragma once
#pragma clang fp contract(off)

namespace dhmc {

constexpr int kThreads = 256;            // one chunk: 256 consecutive path indices
constexpr int kWaves = kThreads / 64;
constexpr int kMaxSlots = 1024;          // blocks per parameter set; a block walks chunks
                                         // slot, slot + slots, ... and sums them in that order
constexpr int kCap = DH_MC_POISSON_CAP;  // terms of the Poisson CDF walked (lambda dt <= 1)
constexpr double kPsiC = 1.5;            // QE branch switch
constexpr double kTwoPi = 6.283185307179586;
constexpr int kVrSums = 5;               // sum y, sum y^2 of the samples; with a control c also
                                         // sum c, sum c^2, sum y c
constexpr int live_sums(bool ctrl) { return ctrl ? kVrSums : 2; }

// one option as the kernels read it (sorted by maturity step; orig = the caller's index)
struct Opt {
    double strike, barrier, T;
    int32_t step, kind, is_call, orig;
};

// ---- Philox4x32-10 (Salmon et al., SC'11) ---------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(M0, c0), l0 = M0 * c0;
        const uint32_t h1 = __umulhi(M1, c2), l1 = M1 * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += W0;                        // the bump after the last round is dead code
        k1 += W1;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// two words -> the odd 53-bit integer 2 k + 1, k = (hi >> 6) 2^26 + (lo >> 6), times 2^-53: exact,
// strictly inside (0, 1), symmetric about 1/2
__device__ __forceinline__ double uniform53(uint32_t hi, uint32_t lo) {
    const uint64_t k = ((uint64_t)(hi >> 6) << 26) | (uint64_t)(lo >> 6);
    return (double)((k << 1) | 1u) * 0x1p-53;
}

__device__ __forceinline__ void box_muller(const uint32_t (&w)[4], double& z0, double& z1) {
    const double rad = sqrt(-2.0 * log(uniform53(w[0], w[1])));
    double s, c;
    dh::dsincos(kTwoPi * uniform53(w[2], w[3]), &s, &c);
    z0 = rad * c;
    z1 = rad * s;
}

// ---- per-set constants: formed by one thread of the block, read back into scalar registers ----
enum {
    kTheta = 0, kKappa, kE, kK1, kK2, kRs, kKtdt, kOmr2, kV0, kFactor,   // per factor: 9 doubles
    kDrift = 2 * kFactor, kMuJ, kSigJ, kS0, kCdf, kNConst = kCdf + kCap
};

struct Factor {
    double theta, kappa, e, k1, k2, rs, ktdt, omr2;
};
struct SetK {
    Factor f[2];
    double drift, mu_j, sig_j, S0;
};

__device__ inline void form_constants(const double* __restrict__ rec, double dt, double* sc) {
    for (int i = 0; i < 2; ++i) {
        const double v0 = rec[5 * i], kappa = rec[5 * i + 1], theta = rec[5 * i + 2],
                     sigma = rec[5 * i + 3], rho = rec[5 * i + 4];
        const double e = exp(-kappa * dt), ome = 1.0 - e;
        double* f = sc + i * kFactor;
        f[kTheta] = theta;
        f[kKappa] = kappa;
        f[kE] = e;
        f[kK1] = sigma * sigma * e * ome / kappa;
        f[kK2] = theta * sigma * sigma * ome * ome / (2.0 * kappa);
        f[kRs] = rho / sigma;
        f[kKtdt] = kappa * theta * dt;
        f[kOmr2] = 1.0 - rho * rho;
        f[kV0] = v0;
    }
    const double lam = rec[10], mu_j = rec[11], sig_j = rec[12];
    const double kbar = exp(mu_j + 0.5 * sig_j * sig_j) - 1.0;
    sc[kDrift] = (rec[14] - lam * kbar) * dt;
    sc[kMuJ] = mu_j;
    sc[kSigJ] = sig_j;
    sc[kS0] = rec[13];
    const double lam_dt = lam * dt;
    double pk = exp(-lam_dt), acc = pk;
    sc[kCdf] = acc;
    for (int k = 1; k < kCap; ++k) {     // cdf[k] = P(N <= k)
        pk = pk * lam_dt / (double)k;
        acc = acc + pk;
        sc[kCdf + k] = acc;
    }
}

// a wave-uniform double into a scalar register pair
__device__ __forceinline__ double to_sgpr(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readfirstlane((int)b);
    const int hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ SetK load_constants(const double* sc) {
    SetK k;
    for (int i = 0; i < 2; ++i) {
        const double* f = sc + i * kFactor;
        k.f[i] = {to_sgpr(f[kTheta]), to_sgpr(f[kKappa]), to_sgpr(f[kE]), to_sgpr(f[kK1]),
                  to_sgpr(f[kK2]), to_sgpr(f[kRs]), to_sgpr(f[kKtdt]), to_sgpr(f[kOmr2])};
    }
    k.drift = to_sgpr(sc[kDrift]);
    k.mu_j = to_sgpr(sc[kMuJ]);
    k.sig_j = to_sgpr(sc[kSigJ]);
    k.S0 = to_sgpr(sc[kS0]);
    return k;
}

// The prologue of every kernel that walks paths: thread 0 forms the constants of the block's set
// in sc [kNConst] (shared), every wave reads them back.
__device__ __forceinline__ SetK block_constants(const double* __restrict__ rec, double dt,
                                                double* sc) {
    if (threadIdx.x == 0) form_constants(rec, dt, sc);
    __syncthreads();
    return load_constants(sc);
}

struct State {
    double x, v1, v2, S, mx, mn, sm;
};

__device__ __forceinline__ State initial_state(const double* sc) {
    return {0.0, sc[kV0], sc[kFactor + kV0], sc[kS0], -INFINITY, INFINITY, 0.0};
}

// one factor: v -> v' by QE, and the factor's log-spot increment added to x
__device__ __forceinline__ void factor_step(const Factor& F, double dt, double u_v, double z_v,
                                            double z_s, double& v, double& x) {
    const double m = F.theta + (v - F.theta) * F.e;
    const double s2 = v * F.k1 + F.k2;
    const double psi = s2 / (m * m);
    double vn;
    if (psi <= kPsiC) {
        const double t = 2.0 / psi;
        const double b2 = t - 1.0 + sqrt(t) * sqrt(t - 1.0);
        const double a = m / (1.0 + b2);
        const double bz = sqrt(b2) + z_v;
        vn = a * (bz * bz);
    } else {
        const double p = (psi - 1.0) / (psi + 1.0);
        const double beta = (1.0 - p) / m;
        vn = u_v <= p ? 0.0 : log((1.0 - p) / (1.0 - u_v)) / beta;
    }
    const double iv = 0.5 * (v + vn) * dt;
    x = x + (-0.5 * iv + F.rs * (vn - v - F.ktdt + F.kappa * iv) + sqrt(F.omr2 * iv) * z_s);
    v = vn;
}

// The jump count, the jump and the running statistics: the tail of the step.
__device__ __forceinline__ void jump_and_track(const SetK& K, int nj, double z_j, State& s) {
    const double n = (double)nj;
    s.x = s.x + ((K.drift + n * K.mu_j) + (sqrt(n) * K.sig_j) * z_j);
    s.S = K.S0 * exp(s.x);
    s.mx = fmax(s.mx, s.S);
    s.mn = fmin(s.mn, s.S);
    s.sm = s.sm + s.S;
}

// The step of path (plo, phi) arriving at date `step` (1-based), in `s`; under ANTI also of its
// mirror in `m` (else `m` is not touched), each draw applied to the path and, mirrored, to the
// mirror.  Every lane of the wave must be active (the Poisson walk and the jump draw end by votes
// of the wave).  Block 0: U_v1 (words 0, 1), U_v2 (2, 3); block 1: Box-Muller of its two uniforms
// -> Z_v1 (cos), Z_s1 (sin); block 2: Z_v2, Z_s2; block 3: U_N (words 0, 1; 2, 3 unused); block 4:
// Z_J (cos; the sin partner is unused).
template <bool ANTI>
__device__ __forceinline__ void mc_step(const SetK& K, const double* cdf, double dt, uint32_t plo,
                                        uint32_t phi, uint32_t step, uint32_t k0, uint32_t k1,
                                        State& s, State& m) {
    uint32_t w[4];
    philox4x32_10(plo, phi, step, 0u, k0, k1, w);
    const double u_v1 = uniform53(w[0], w[1]), u_v2 = uniform53(w[2], w[3]);
    double z_v, z_s;
    philox4x32_10(plo, phi, step, 1u, k0, k1, w);
    box_muller(w, z_v, z_s);
    factor_step(K.f[0], dt, u_v1, z_v, z_s, s.v1, s.x);
    if constexpr (ANTI) factor_step(K.f[0], dt, 1.0 - u_v1, -z_v, -z_s, m.v1, m.x);
    philox4x32_10(plo, phi, step, 2u, k0, k1, w);
    box_muller(w, z_v, z_s);
    factor_step(K.f[1], dt, u_v2, z_v, z_s, s.v2, s.x);
    if constexpr (ANTI) factor_step(K.f[1], dt, 1.0 - u_v2, -z_v, -z_s, m.v2, m.x);
    philox4x32_10(plo, phi, step, 3u, k0, k1, w);
    const double u_n = uniform53(w[0], w[1]), u_m = 1.0 - u_n;
    int nj = 0, njm = 0;
    for (int k = 0; k < kCap; ++k) {     // N = #{k : U_N > cdf[k]}; the CDF only grows, so the
        const bool above = u_n > cdf[k]; // counts are complete once no lane is above on any path
        const bool above_m = ANTI && u_m > cdf[k];
        if (__ballot(above || above_m) == 0) break;
        nj += above ? 1 : 0;
        njm += above_m ? 1 : 0;
    }
    // sqrt(0) sigma_j Z_J = +-0 adds nothing: the draw is made only where some lane jumped
    double z_j = 0.0, spare;
    if (__ballot(nj > 0 || njm > 0) != 0) {
        philox4x32_10(plo, phi, step, 4u, k0, k1, w);
        box_muller(w, z_j, spare);
    }
    jump_and_track(K, nj, z_j, s);
    if constexpr (ANTI) jump_and_track(K, njm, -z_j, m);
}

__device__ __forceinline__ double payoff(int kind, int is_call, double strike, double barrier,
                                         int step, const State& s) {
    const double under = kind == DH_MC_ASIAN ? s.sm / (double)step : s.S;
    double pay = is_call ? fmax(under - strike, 0.0) : fmax(strike - under, 0.0);
    if (kind == DH_MC_UP_AND_OUT) pay = s.mx < barrier ? pay : 0.0;
    if (kind == DH_MC_DOWN_AND_OUT) pay = s.mn > barrier ? pay : 0.0;
    return pay;
}

}  // namespace dhmc

#include "dh_mc_vr.h"        // the control variate: control(), control_estimate(), the twins

namespace dhmc {

// Path kernel: grid (slots, P), over n_samples samples: paths, or under ANTI pairs whose sample is
// the average of the two payoffs.  part[((set * slots + slot) * n_opt + j) * kLive + t] = the
// block's sums of sorted option j -- sum y and sum y^2, under CTRL also sum c, sum c^2 and sum y c
// of its control -- over the block's chunks: per chunk the 64 lanes of a wave by the xor
// butterfly, the four waves as (w0 + w1) + (w2 + w3), then the chunks in increasing order.
template <bool ANTI, bool CTRL>
__global__ __launch_bounds__(kThreads) void mc_price_kernel(
    const double* __restrict__ prm, const Opt* __restrict__ opts, int n_opt, int64_t n_samples,
    int64_t n_chunks, int max_step, double dt, uint32_t k0, uint32_t k1,
    double* __restrict__ part) {
    constexpr int kLive = live_sums(CTRL);
    __shared__ double sc[kNConst];
    __shared__ double red[kWaves][DH_MC_MAX_OPTIONS][kLive];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int set = blockIdx.y, slot = blockIdx.x, slots = gridDim.x;
    const SetK K = block_constants(prm + (size_t)set * DH_PARAM_STRIDE, dt, sc);
    double acc[kLive] = {};              // thread j < n_opt owns sorted option j
    for (int64_t chunk = slot; chunk < n_chunks; chunk += slots) {
        const int64_t path = chunk * kThreads + tid;
        const bool active = path < n_samples;  // a lane past the end walks its path, pays 0
        const uint32_t plo = (uint32_t)path, phi = (uint32_t)((uint64_t)path >> 32);
        State s = initial_state(sc), m = s;
        int next = 0;
        int next_step = opts[0].step;
        for (int step = 1; step <= max_step; ++step) {
            mc_step<ANTI>(K, sc + kCdf, dt, plo, phi, (uint32_t)step, k0, k1, s, m);
            while (next_step == step) {
                const Opt o = opts[next];
                double y = payoff(o.kind, o.is_call, o.strike, o.barrier, step, s);
                double c = CTRL ? control(o, step, s) : 0.0;
                if constexpr (ANTI) {
                    y = 0.5 * (y + payoff(o.kind, o.is_call, o.strike, o.barrier, step, m));
                    if (CTRL) c = 0.5 * (c + control(o, step, m));
                }
                y = active ? y : 0.0;
                c = active ? c : 0.0;
                const double v[kVrSums] = {y, y * y, c, c * c, y * c};
#pragma unroll
                for (int t = 0; t < kLive; ++t) {
                    const double w = xor_sum(v[t], 64);
                    if (lane == 0) red[wave][next][t] = w;
                }
                ++next;
                next_step = next < n_opt ? opts[next].step : -1;
            }
        }
        __syncthreads();
        if (tid < n_opt) {
#pragma unroll
            for (int t = 0; t < kLive; ++t)
                acc[t] += (red[0][tid][t] + red[1][tid][t]) + (red[2][tid][t] + red[3][tid][t]);
        }
        __syncthreads();
    }
    if (tid < n_opt) {
        double* p = part + (((size_t)set * slots + slot) * n_opt + tid) * kLive;
#pragma unroll
        for (int t = 0; t < kLive; ++t) p[t] = acc[t];
    }
}

// what the finishing kernel writes, each [P][n_options] in the caller's option order; the last
// four may be null
struct PriceOut {
    double *price, *err, *base_price, *base_err, *beta, *mean;
};

// The slots' partials of one (set, option), LIVE sums each, added in slot order.  LIVE is a
// compile-time count so that the loads of a slot are independent and the loop unrolls: with a
// run-time count the walk over 1,024 slots is one chain of load latencies.
template <int LIVE>
__device__ __forceinline__ void add_slots(const double* __restrict__ part, size_t first,
                                          int n_opt, int slots, double (&sum)[kVrSums]) {
    for (int k = 0; k < slots; ++k) {
        const double* p = part + (first + (size_t)k * n_opt) * LIVE;
#pragma unroll
        for (int t = 0; t < LIVE; ++t) sum[t] += p[t];
    }
}

// Finishing kernel: one thread per (set, sorted option); the slots' partials in slot order, then
// the plain mean and its error and, under `ctrl`, the control's estimator (dh_mc_vr.h).  twin[j] =
// the option's column of cos [P][n_twins], or -1 where the control's mean is S0; without `ctrl`
// beta = 0 and the mean is NaN.
__global__ __launch_bounds__(kThreads) void mc_finish_kernel(
    const double* __restrict__ prm, const Opt* __restrict__ opts, const int32_t* __restrict__ twin,
    const double* __restrict__ cos, int n_twins, int n_opt, int P, int slots, int64_t n_samples,
    int ctrl, const double* __restrict__ part, PriceOut out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= P * n_opt) return;
    const int set = i / n_opt, j = i - set * n_opt;
    double sum[kVrSums] = {};            // sum y, sum y^2, sum c, sum c^2, sum y c
    const size_t first = (size_t)set * slots * n_opt + j;
    if (ctrl) add_slots<live_sums(true)>(part, first, n_opt, slots, sum);
    else add_slots<live_sums(false)>(part, first, n_opt, slots, sum);
    const double* rec = prm + (size_t)set * DH_PARAM_STRIDE;
    const double n = (double)n_samples;
    const double disc = exp(-rec[14] * opts[j].T);
    const double cyy = sum[1] - sum[0] * sum[0] / n;
    const double base_price = disc * sum[0] / n;
    const double base_err = disc * sqrt(fmax(cyy, 0.0) / (n * (n - 1.0)));
    double beta = 0.0, mean = __builtin_nan(""), price = base_price, err = base_err;
    if (ctrl) {
        mean = twin[j] < 0 ? rec[13] : cos[(size_t)set * n_twins + twin[j]];
        control_estimate(sum, n, disc, cyy, base_price, mean, beta, price, err);
    }
    const size_t o = (size_t)set * n_opt + opts[j].orig;
    out.price[o] = price;
    out.err[o] = err;
    if (out.base_price) out.base_price[o] = base_price;
    if (out.base_err) out.base_err[o] = base_err;
    if (out.beta) out.beta[o] = beta;
    if (out.mean) out.mean[o] = mean;
}

// Validation kernel: grid (ceil(n_paths / 256), P); the statistics of paths path0 + i -- under
// MIRROR of their mirrors, walked as the antithetic price kernel walks them -- at the listed
// steps, by the pricing kernel's own step function.
template <bool MIRROR>
__global__ __launch_bounds__(kThreads) void mc_paths_kernel(
    const double* __restrict__ prm, const int32_t* __restrict__ obs, int n_obs, int64_t path0,
    int64_t n_paths, double dt, uint32_t k0, uint32_t k1, double* __restrict__ out) {
    __shared__ double sc[kNConst];
    const int tid = threadIdx.x;
    const int set = blockIdx.y;
    const SetK K = block_constants(prm + (size_t)set * DH_PARAM_STRIDE, dt, sc);
    const int64_t i = (int64_t)blockIdx.x * kThreads + tid;
    const bool active = i < n_paths;     // whole waves walk (mc_step votes over the wave)
    const int64_t path = path0 + (active ? i : 0);
    const uint32_t plo = (uint32_t)path, phi = (uint32_t)((uint64_t)path >> 32);
    State s = initial_state(sc), m = s;
    int next = 0;
    int next_step = obs[0];
    const int max_step = obs[n_obs - 1];
    for (int step = 1; step <= max_step; ++step) {
        mc_step<MIRROR>(K, sc + kCdf, dt, plo, phi, (uint32_t)step, k0, k1, s, m);
        if (next_step == step) {
            if (active) {
                const State& w = MIRROR ? m : s;
                double* o = out + (((size_t)set * n_paths + i) * n_obs + next) * 6;
                o[0] = w.S, o[1] = w.v1, o[2] = w.v2, o[3] = w.mx, o[4] = w.mn, o[5] = w.sm;
            }
            ++next;
            next_step = next < n_obs ? obs[next] : -1;
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------
constexpr int kMaxSets = 65535;          // grid y
constexpr double kStepTol = 1e-9;        // |T steps_per_year - n| <= kStepTol n

int check_common(const dh_ctx* ctx, int64_t P, int steps_per_year) {
    if (!ctx) return fail(DH_E_ARG, "ctx is null");
    if (P < 1 || P > kMaxSets)
        return fail(DH_E_ARG, "P must be in [1, " + std::to_string(kMaxSets) + "], got " +
                                  std::to_string(P));
    if (steps_per_year < 1)
        return fail(DH_E_ARG, "steps_per_year must be >= 1, got " + std::to_string(steps_per_year));
    return DH_OK;
}

int check_params(const double* params, int64_t P, int steps_per_year) {
    static const char* names[16] = {"v01", "kappa1", "theta1", "sigma1", "rho1", "v02", "kappa2",
                                    "theta2", "sigma2", "rho2", "lambda_j", "mu_j", "sigma_j",
                                    "spot", "rate", "q"};
    for (int64_t p = 0; p < P; ++p) {
        const double* r = params + p * DH_PARAM_STRIDE;
        auto bad = [&](int k, const char* why) {
            return fail(DH_E_ARG, std::string("params: ") + names[k] + " of set " +
                                      std::to_string(p) + " " + why);
        };
        for (int k = 0; k < 15; ++k)
            if (!std::isfinite(r[k])) return bad(k, "is not finite");
        for (int f = 0; f < 2; ++f) {
            if (r[5 * f] < 0.0) return bad(5 * f, "must be >= 0");
            for (int k = 1; k <= 3; ++k)
                if (!(r[5 * f + k] > 0.0)) return bad(5 * f + k, "must be > 0");
            if (!(std::fabs(r[5 * f + 4]) < 1.0)) return bad(5 * f + 4, "must lie inside (-1, 1)");
        }
        if (r[10] < 0.0) return bad(10, "must be >= 0");
        if (r[10] / (double)steps_per_year > 1.0)
            return bad(10, "gives lambda dt > 1 (the Poisson walk's cap): raise steps_per_year");
        if (r[12] < 0.0) return bad(12, "must be >= 0");
        if (!(r[13] > 0.0)) return bad(13, "must be > 0");
    }
    return DH_OK;
}

// the step of a maturity: `at` names the option in the refusal
int maturity_step(double maturity, int steps_per_year, const std::string& at, int32_t& step) {
    const double ns = maturity * (double)steps_per_year, n = std::rint(ns);
    if (!std::isfinite(ns) || n < 1.0 || n > 2147483647.0 || std::fabs(ns - n) > kStepTol * n)
        return fail(DH_E_ARG, "options: maturity" + at + " is not a whole number (>= 1) of " +
                                  "steps of 1 / steps_per_year");
    step = (int32_t)n;
    return DH_OK;
}

// the options sorted by maturity step (stable: the caller's order within a step)
int check_options(const dh_mc_option* options, int n_options, int steps_per_year,
                  std::vector<Opt>& sorted) {
    if (n_options < 1 || n_options > DH_MC_MAX_OPTIONS)
        return fail(DH_E_ARG, "n_options must be in [1, " + std::to_string(DH_MC_MAX_OPTIONS) +
                                  "], got " + std::to_string(n_options));
    if (!options) return fail(DH_E_ARG, "options is null");
    sorted.resize(n_options);
    for (int j = 0; j < n_options; ++j) {
        const dh_mc_option& o = options[j];
        const std::string at = " of option " + std::to_string(j);
        if (o.kind < DH_MC_EUROPEAN || o.kind > DH_MC_DOWN_AND_OUT)
            return fail(DH_E_ARG, "options: unknown kind " + std::to_string(o.kind) + at);
        if (!std::isfinite(o.strike) || o.strike < 0.0)
            return fail(DH_E_ARG, "options: strike" + at + " must be finite and >= 0");
        int32_t step;
        const int rc = maturity_step(o.maturity, steps_per_year, at, step);
        if (rc) return rc;
        const bool barrier = o.kind == DH_MC_UP_AND_OUT || o.kind == DH_MC_DOWN_AND_OUT;
        if (barrier && !(o.barrier > 0.0))
            return fail(DH_E_ARG, "options: barrier" + at + " must be > 0");
        sorted[j] = {o.strike, barrier ? o.barrier : 0.0, o.maturity, step, o.kind,
                     o.is_call != 0, j};
    }
    std::stable_sort(sorted.begin(), sorted.end(),
                     [](const Opt& a, const Opt& b) { return a.step < b.step; });
    return DH_OK;
}

// n_paths and the flags of a pricing call; `vr`: an entry that refuses flags == 0
int check_walks(int64_t n_paths, int flags, bool vr) {
    if (n_paths < 2) return fail(DH_E_ARG, "n_paths must be >= 2, got " + std::to_string(n_paths));
    if (vr && flags == 0)
        return fail(DH_E_ARG, "flags is 0: neither antithetic nor control (that is dh_mc_price)");
    if (flags & ~(DH_MC_VR_ANTITHETIC | DH_MC_VR_CONTROL))
        return fail(DH_E_ARG, "flags has unknown bits: " + std::to_string(flags));
    if ((flags & DH_MC_VR_ANTITHETIC) && (n_paths % 2 != 0 || n_paths < 4))
        return fail(DH_E_ARG, "n_paths counts walks: under the antithetic flag it must be even "
                              "and >= 4, got " + std::to_string(n_paths));
    return DH_OK;
}

// dh_mc_price_dev (flags 0; base_price, base_err, beta and mean of `out` null) and
// dh_mc_price_vr_dev (`vr`)
int price_dev(dh_ctx* ctx, const double* d_params, int64_t P, const dh_mc_option* options,
              int n_options, int64_t n_paths, int steps_per_year, uint64_t seed, int flags, bool vr,
              const PriceOut& out, void* stream) {
    int rc = check_common(ctx, P, steps_per_year);
    if (rc) return rc;
    rc = check_walks(n_paths, flags, vr);
    if (rc) return rc;
    std::vector<Opt> sorted;
    rc = check_options(options, n_options, steps_per_year, sorted);
    if (rc) return rc;
    if (!d_params || !out.price || !out.err) return fail(DH_E_ARG, "null argument");
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    const bool anti = flags & DH_MC_VR_ANTITHETIC, ctrl = flags & DH_MC_VR_CONTROL;
    const int64_t n_samples = anti ? n_paths / 2 : n_paths;
    const int64_t n_chunks = (n_samples + kThreads - 1) / kThreads;
    const int slots = (int)std::min<int64_t>(n_chunks, kMaxSlots);
    // the sorted options, then under `ctrl` each one's column among the twins
    const size_t ob = (size_t)n_options * sizeof(Opt), tb = ctrl ? (size_t)n_options * 4 : 0;
    HIP_TRY(ctx->mc_opts.reserve(ob + tb));
    HIP_TRY(ctx->mc_part.reserve((size_t)P * slots * n_options * live_sums(ctrl) * 8));
    // pageable source: the copy has read `sorted` when the call returns
    HIP_TRY(hipMemcpyAsync(ctx->mc_opts.ptr, sorted.data(), ob, hipMemcpyHostToDevice, st));
    const Opt* d_opts = (const Opt*)ctx->mc_opts.ptr;
    const int32_t* d_twin = (const int32_t*)((const char*)ctx->mc_opts.ptr + ob);
    const double* d_cos = nullptr;
    int n_twins = 0;
    if (ctrl) {
        rc = control_means(ctx, d_params, P, sorted, (int32_t*)d_twin, st, n_twins, d_cos);
        if (rc) return rc;
    }
    double* part = (double*)ctx->mc_part.ptr;
    const auto kernel = anti ? (ctrl ? mc_price_kernel<true, true> : mc_price_kernel<true, false>)
                             : (ctrl ? mc_price_kernel<false, true> : mc_price_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(slots, (unsigned)P), dim3(kThreads), 0, st, d_params, d_opts,
                       n_options, n_samples, n_chunks, sorted.back().step,
                       1.0 / (double)steps_per_year, (uint32_t)seed, (uint32_t)(seed >> 32), part);
    HIP_TRY(hipGetLastError());
    const int64_t n_out = P * n_options;
    hipLaunchKernelGGL(mc_finish_kernel, dim3((unsigned)((n_out + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, st, d_params, d_opts, d_twin, d_cos, n_twins, n_options,
                       (int)P, slots, n_samples, ctrl ? 1 : 0, (const double*)part, out);
    HIP_TRY(hipGetLastError());
    return DH_OK;
}

// dh_mc_price (flags 0, two results) and dh_mc_price_vr (`vr`, six; the last four may be null)
int price_host(dh_ctx* ctx, const double* params, int64_t P, const dh_mc_option* options,
               int n_options, int64_t n_paths, int steps_per_year, uint64_t seed, int flags,
               bool vr, double* const (&host)[6]) {
    int rc = check_common(ctx, P, steps_per_year);
    if (rc) return rc;
    if (!params || !host[0] || !host[1]) return fail(DH_E_ARG, "null argument");
    rc = check_params(params, P, steps_per_year);
    if (rc) return rc;
    rc = check_walks(n_paths, flags, vr);
    if (rc) return rc;
    std::vector<Opt> sorted;
    rc = check_options(options, n_options, steps_per_year, sorted);
    if (rc) return rc;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t n = (size_t)P * n_options, pb = (size_t)P * DH_PARAM_STRIDE * 8, ob = n * 8;
    const size_t n_res = vr ? 6 : 2;
    HIP_TRY(ctx->mc_params.reserve(pb));
    HIP_TRY(ctx->mc_out.reserve(n_res * ob));
    hipStream_t st = ctx->stream;
    double* d = (double*)ctx->mc_out.ptr;
    HIP_TRY(hipMemcpyAsync(ctx->mc_params.ptr, params, pb, hipMemcpyHostToDevice, st));
    const PriceOut out = vr ? PriceOut{d, d + n, d + 2 * n, d + 3 * n, d + 4 * n, d + 5 * n}
                            : PriceOut{d, d + n, nullptr, nullptr, nullptr, nullptr};
    rc = price_dev(ctx, (const double*)ctx->mc_params.ptr, P, options, n_options, n_paths,
                   steps_per_year, seed, flags, vr, out, st);
    if (rc) return rc;
    for (size_t k = 0; k < n_res; ++k)
        if (host[k]) HIP_TRY(hipMemcpyAsync(host[k], d + k * n, ob, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}

// dh_mc_paths and, with a mirror switch, dh_mc_paths_vr
int paths(dh_ctx* ctx, const double* params, int64_t P, int n_obs, const int32_t* obs_steps,
          int64_t path0, int64_t n_paths, int steps_per_year, uint64_t seed, bool mirror,
          double* out) {
    int rc = check_common(ctx, P, steps_per_year);
    if (rc) return rc;
    if (!params || !out) return fail(DH_E_ARG, "null argument");
    rc = check_params(params, P, steps_per_year);
    if (rc) return rc;
    if (n_obs < 1 || !obs_steps) return fail(DH_E_ARG, "n_obs must be >= 1 and obs_steps given");
    for (int j = 0; j < n_obs; ++j)
        if (obs_steps[j] < 1 || (j > 0 && obs_steps[j] <= obs_steps[j - 1]))
            return fail(DH_E_ARG, "obs_steps must be >= 1 and strictly increasing (entry " +
                                      std::to_string(j) + ")");
    if (path0 < 0) return fail(DH_E_ARG, "path0 must be >= 0");
    if (n_paths < 1 || n_paths > (int64_t(1) << 31) * kThreads || path0 > INT64_MAX - n_paths)
        return fail(DH_E_ARG, "n_paths must be >= 1 and path0 + n_paths fit 63 bits, got " +
                                  std::to_string(n_paths));
    const double words = (double)P * (double)n_paths * (double)n_obs * 6.0;   // exact below 2^53
    if (words > 0x1p31)
        return fail(DH_E_ARG, "out [P, n_paths, n_obs, 6] is larger than 2^31 doubles: ask for "
                              "fewer paths per call (path0 selects the range)");
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t pb = (size_t)P * DH_PARAM_STRIDE * 8, sb = (size_t)n_obs * 4;
    const size_t ob = (size_t)words * 8;
    HIP_TRY(ctx->mc_params.reserve(pb));
    HIP_TRY(ctx->mc_opts.reserve(sb));
    HIP_TRY(ctx->mc_out.reserve(ob));
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(ctx->mc_params.ptr, params, pb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->mc_opts.ptr, obs_steps, sb, hipMemcpyHostToDevice, st));
    const unsigned blocks = (unsigned)((n_paths + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(mirror ? mc_paths_kernel<true> : mc_paths_kernel<false>,
                       dim3(blocks, (unsigned)P), dim3(kThreads), 0, st,
                       (const double*)ctx->mc_params.ptr, (const int32_t*)ctx->mc_opts.ptr, n_obs,
                       path0, n_paths, 1.0 / (double)steps_per_year, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (double*)ctx->mc_out.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, ctx->mc_out.ptr, ob, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}

}  // namespace dhmc

extern "C" int dh_mc_price_dev(dh_ctx* ctx, const double* d_params, int64_t P,
                               const dh_mc_option* options, int n_options, int64_t n_paths,
                               int steps_per_year, uint64_t seed, double* d_price,
                               double* d_stderr, void* stream) {
    return dhmc::price_dev(ctx, d_params, P, options, n_options, n_paths, steps_per_year, seed, 0,
                           false, {d_price, d_stderr, nullptr, nullptr, nullptr, nullptr}, stream);
}

extern "C" int dh_mc_price(dh_ctx* ctx, const double* params, int64_t P,
                           const dh_mc_option* options, int n_options, int64_t n_paths,
                           int steps_per_year, uint64_t seed, double* price, double* stderr_out) {
    return dhmc::price_host(ctx, params, P, options, n_options, n_paths, steps_per_year, seed, 0,
                            false, {price, stderr_out, nullptr, nullptr, nullptr, nullptr});
}

extern "C" int dh_mc_price_vr_dev(dh_ctx* ctx, const double* d_params, int64_t P,
                                  const dh_mc_option* options, int n_options, int64_t n_paths,
                                  int steps_per_year, uint64_t seed, int flags, double* d_price,
                                  double* d_stderr, double* d_base_price, double* d_base_stderr,
                                  double* d_beta, double* d_control_mean, void* stream) {
    return dhmc::price_dev(
        ctx, d_params, P, options, n_options, n_paths, steps_per_year, seed, flags, true,
        {d_price, d_stderr, d_base_price, d_base_stderr, d_beta, d_control_mean}, stream);
}

extern "C" int dh_mc_price_vr(dh_ctx* ctx, const double* params, int64_t P,
                              const dh_mc_option* options, int n_options, int64_t n_paths,
                              int steps_per_year, uint64_t seed, int flags, double* price,
                              double* stderr_out, double* base_price, double* base_stderr,
                              double* beta, double* control_mean) {
    return dhmc::price_host(ctx, params, P, options, n_options, n_paths, steps_per_year, seed,
                            flags, true,
                            {price, stderr_out, base_price, base_stderr, beta, control_mean});
}

extern "C" int dh_mc_paths(dh_ctx* ctx, const double* params, int64_t P, int n_obs,
                           const int32_t* obs_steps, int64_t path0, int64_t n_paths,
                           int steps_per_year, uint64_t seed, double* out) {
    return dhmc::paths(ctx, params, P, n_obs, obs_steps, path0, n_paths, steps_per_year, seed,
                       false, out);
}

extern "C" int dh_mc_paths_vr(dh_ctx* ctx, const double* params, int64_t P, int n_obs,
                              const int32_t* obs_steps, int64_t path0, int64_t n_paths,
                              int steps_per_year, uint64_t seed, int mirror, double* out) {
    return dhmc::paths(ctx, params, P, n_obs, obs_steps, path0, n_paths, steps_per_year, seed,
                       mirror != 0, out);
}
