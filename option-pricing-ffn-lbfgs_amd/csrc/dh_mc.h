// dh_mc.h -- Monte Carlo path pricer of the Double-Heston + Merton-jump model (dh_mc_price,
// dh_mc_price_dev, dh_mc_paths).  Included by dh_kernels.hip after its host helpers.
// DESIGN.md 3.15 is the contract of the scheme; tests/mc_reference.py restates it in NumPy.
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

// The step of path (plo, phi) arriving at date `step` (1-based).  Every lane of the wave must be
// active (the jump draw is skipped by a vote of the wave).  Block 0: U_v1 (words 0, 1), U_v2 (2,
// 3); block 1: Box-Muller of its two uniforms -> Z_v1 (cos), Z_s1 (sin); block 2: Z_v2, Z_s2;
// block 3: U_N (words 0, 1; 2, 3 unused); block 4: Z_J (cos; the sin partner is unused).
__device__ __forceinline__ void mc_step(const SetK& K, const double* cdf, double dt, uint32_t plo,
                                        uint32_t phi, uint32_t step, uint32_t k0, uint32_t k1,
                                        State& s) {
    uint32_t w[4];
    philox4x32_10(plo, phi, step, 0u, k0, k1, w);
    const double u_v1 = uniform53(w[0], w[1]), u_v2 = uniform53(w[2], w[3]);
    double z_v, z_s;
    philox4x32_10(plo, phi, step, 1u, k0, k1, w);
    box_muller(w, z_v, z_s);
    factor_step(K.f[0], dt, u_v1, z_v, z_s, s.v1, s.x);
    philox4x32_10(plo, phi, step, 2u, k0, k1, w);
    box_muller(w, z_v, z_s);
    factor_step(K.f[1], dt, u_v2, z_v, z_s, s.v2, s.x);
    philox4x32_10(plo, phi, step, 3u, k0, k1, w);
    const double u_n = uniform53(w[0], w[1]);
    int nj = 0;
    for (int k = 0; k < kCap; ++k) {     // N = #{k : U_N > cdf[k]}; the CDF only grows, so the
        const bool above = u_n > cdf[k]; // count is complete once no lane is above
        if (__ballot(above) == 0) break;
        nj += above ? 1 : 0;
    }
    // sqrt(0) sigma_j Z_J = +-0 adds nothing: the draw is made only where some lane jumped
    double z_j = 0.0, spare;
    if (__ballot(nj > 0) != 0) {
        philox4x32_10(plo, phi, step, 4u, k0, k1, w);
        box_muller(w, z_j, spare);
    }
    const double n = (double)nj;
    s.x = s.x + ((K.drift + n * K.mu_j) + (sqrt(n) * K.sig_j) * z_j);
    s.S = K.S0 * exp(s.x);
    s.mx = fmax(s.mx, s.S);
    s.mn = fmin(s.mn, s.S);
    s.sm = s.sm + s.S;
}

__device__ __forceinline__ double payoff(int kind, int is_call, double strike, double barrier,
                                         int step, const State& s) {
    const double under = kind == DH_MC_ASIAN ? s.sm / (double)step : s.S;
    double pay = is_call ? fmax(under - strike, 0.0) : fmax(strike - under, 0.0);
    if (kind == DH_MC_UP_AND_OUT) pay = s.mx < barrier ? pay : 0.0;
    if (kind == DH_MC_DOWN_AND_OUT) pay = s.mn > barrier ? pay : 0.0;
    return pay;
}

// Path kernel: grid (slots, P).  part[(set * slots + slot) * n_opt + j] = (sum of payoffs, sum of
// squared payoffs) of sorted option j over the block's chunks: per chunk the 64 lanes of a wave by
// the xor butterfly, the four waves as (w0 + w1) + (w2 + w3), then the chunks in increasing order.
__global__ __launch_bounds__(kThreads) void mc_price_kernel(
    const double* __restrict__ prm, const Opt* __restrict__ opts, int n_opt, int64_t n_paths,
    int64_t n_chunks, int max_step, double dt, uint32_t k0, uint32_t k1,
    double2* __restrict__ part) {
    __shared__ double sc[kNConst];
    __shared__ double red[kWaves][DH_MC_MAX_OPTIONS][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int set = blockIdx.y, slot = blockIdx.x, slots = gridDim.x;
    if (tid == 0) form_constants(prm + (size_t)set * DH_PARAM_STRIDE, dt, sc);
    __syncthreads();
    const SetK K = load_constants(sc);
    double acc1 = 0.0, acc2 = 0.0;       // thread j < n_opt owns sorted option j
    for (int64_t chunk = slot; chunk < n_chunks; chunk += slots) {
        const int64_t path = chunk * kThreads + tid;
        const bool active = path < n_paths;   // a lane past the end walks its path, pays 0
        const uint32_t plo = (uint32_t)path, phi = (uint32_t)((uint64_t)path >> 32);
        State s = initial_state(sc);
        int next = 0;
        int next_step = opts[0].step;
        for (int step = 1; step <= max_step; ++step) {
            mc_step(K, sc + kCdf, dt, plo, phi, (uint32_t)step, k0, k1, s);
            while (next_step == step) {
                const Opt o = opts[next];
                const double pay =
                    active ? payoff(o.kind, o.is_call, o.strike, o.barrier, step, s) : 0.0;
                const double s1 = xor_sum(pay, 64), s2 = xor_sum(pay * pay, 64);
                if (lane == 0) {
                    red[wave][next][0] = s1;
                    red[wave][next][1] = s2;
                }
                ++next;
                next_step = next < n_opt ? opts[next].step : -1;
            }
        }
        __syncthreads();
        if (tid < n_opt) {
            acc1 += (red[0][tid][0] + red[1][tid][0]) + (red[2][tid][0] + red[3][tid][0]);
            acc2 += (red[0][tid][1] + red[1][tid][1]) + (red[2][tid][1] + red[3][tid][1]);
        }
        __syncthreads();
    }
    if (tid < n_opt) part[((size_t)set * slots + slot) * n_opt + tid] = make_double2(acc1, acc2);
}

// Finishing kernel: one thread per (set, sorted option); the slots' partials in slot order.
__global__ __launch_bounds__(kThreads) void mc_finish_kernel(
    const double* __restrict__ prm, const Opt* __restrict__ opts, int n_opt, int P, int slots,
    int64_t n_paths, const double2* __restrict__ part, double* __restrict__ price,
    double* __restrict__ err) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= P * n_opt) return;
    const int set = i / n_opt, j = i - set * n_opt;
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < slots; ++k) {
        const double2 p = part[((size_t)set * slots + k) * n_opt + j];
        s1 += p.x;
        s2 += p.y;
    }
    const double n = (double)n_paths;
    const double disc = exp(-prm[(size_t)set * DH_PARAM_STRIDE + 14] * opts[j].T);
    const size_t o = (size_t)set * n_opt + opts[j].orig;
    price[o] = disc * s1 / n;
    err[o] = disc * sqrt(fmax(s2 - s1 * s1 / n, 0.0) / (n * (n - 1.0)));
}

// Validation kernel: grid (ceil(n_paths / 256), P); the statistics of paths path0 + i at the
// listed steps, by the pricing kernel's own step function.
__global__ __launch_bounds__(kThreads) void mc_paths_kernel(
    const double* __restrict__ prm, const int32_t* __restrict__ obs, int n_obs, int64_t path0,
    int64_t n_paths, double dt, uint32_t k0, uint32_t k1, double* __restrict__ out) {
    __shared__ double sc[kNConst];
    const int tid = threadIdx.x;
    const int set = blockIdx.y;
    if (tid == 0) form_constants(prm + (size_t)set * DH_PARAM_STRIDE, dt, sc);
    __syncthreads();
    const SetK K = load_constants(sc);
    const int64_t i = (int64_t)blockIdx.x * kThreads + tid;
    const bool active = i < n_paths;     // whole waves walk (mc_step votes over the wave)
    const int64_t path = path0 + (active ? i : 0);
    const uint32_t plo = (uint32_t)path, phi = (uint32_t)((uint64_t)path >> 32);
    State s = initial_state(sc);
    int next = 0;
    int next_step = obs[0];
    const int max_step = obs[n_obs - 1];
    for (int step = 1; step <= max_step; ++step) {
        mc_step(K, sc + kCdf, dt, plo, phi, (uint32_t)step, k0, k1, s);
        if (next_step == step) {
            if (active) {
                double* o = out + (((size_t)set * n_paths + i) * n_obs + next) * 6;
                o[0] = s.S, o[1] = s.v1, o[2] = s.v2, o[3] = s.mx, o[4] = s.mn, o[5] = s.sm;
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
        const double ns = o.maturity * (double)steps_per_year, n = std::rint(ns);
        if (!std::isfinite(ns) || n < 1.0 || n > 2147483647.0 || std::fabs(ns - n) > kStepTol * n)
            return fail(DH_E_ARG, "options: maturity" + at + " is not a whole number (>= 1) of " +
                                      "steps of 1 / steps_per_year");
        const bool barrier = o.kind == DH_MC_UP_AND_OUT || o.kind == DH_MC_DOWN_AND_OUT;
        if (barrier && !(o.barrier > 0.0))
            return fail(DH_E_ARG, "options: barrier" + at + " must be > 0");
        sorted[j] = {o.strike, barrier ? o.barrier : 0.0, o.maturity, (int32_t)n, o.kind,
                     o.is_call != 0, j};
    }
    std::stable_sort(sorted.begin(), sorted.end(),
                     [](const Opt& a, const Opt& b) { return a.step < b.step; });
    return DH_OK;
}

// the arguments of dh_mc_paths (and of dh_mc_paths_vr, dh_mc_vr.h)
int check_paths(const dh_ctx* ctx, const double* params, int64_t P, int n_obs,
                const int32_t* obs_steps, int64_t path0, int64_t n_paths, int steps_per_year,
                const double* out) {
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
    if ((double)P * (double)n_paths * (double)n_obs * 6.0 > 0x1p31)
        return fail(DH_E_ARG, "out [P, n_paths, n_obs, 6] is larger than 2^31 doubles: ask for "
                              "fewer paths per call (path0 selects the range)");
    return DH_OK;
}

}  // namespace dhmc

extern "C" int dh_mc_price_dev(dh_ctx* ctx, const double* d_params, int64_t P,
                               const dh_mc_option* options, int n_options, int64_t n_paths,
                               int steps_per_year, uint64_t seed, double* d_price,
                               double* d_stderr, void* stream) {
    int rc = dhmc::check_common(ctx, P, steps_per_year);
    if (rc) return rc;
    if (n_paths < 2) return fail(DH_E_ARG, "n_paths must be >= 2, got " + std::to_string(n_paths));
    std::vector<dhmc::Opt> sorted;
    rc = dhmc::check_options(options, n_options, steps_per_year, sorted);
    if (rc) return rc;
    if (!d_params || !d_price || !d_stderr) return fail(DH_E_ARG, "null argument");
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    const int64_t n_chunks = (n_paths + dhmc::kThreads - 1) / dhmc::kThreads;
    const int slots = (int)std::min<int64_t>(n_chunks, dhmc::kMaxSlots);
    const size_t ob = (size_t)n_options * sizeof(dhmc::Opt);
    HIP_TRY(ctx->mc_opts.reserve(ob));
    HIP_TRY(ctx->mc_part.reserve((size_t)P * slots * n_options * sizeof(double2)));
    // pageable source: the copy has read `sorted` when the call returns
    HIP_TRY(hipMemcpyAsync(ctx->mc_opts.ptr, sorted.data(), ob, hipMemcpyHostToDevice, st));
    const dhmc::Opt* d_opts = (const dhmc::Opt*)ctx->mc_opts.ptr;
    double2* part = (double2*)ctx->mc_part.ptr;
    const double dt = 1.0 / (double)steps_per_year;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    hipLaunchKernelGGL(dhmc::mc_price_kernel, dim3(slots, (unsigned)P), dim3(dhmc::kThreads), 0,
                       st, d_params, d_opts, n_options, n_paths, n_chunks, sorted.back().step, dt,
                       k0, k1, part);
    HIP_TRY(hipGetLastError());
    const int64_t n_out = P * n_options;
    hipLaunchKernelGGL(dhmc::mc_finish_kernel,
                       dim3((unsigned)((n_out + dhmc::kThreads - 1) / dhmc::kThreads)),
                       dim3(dhmc::kThreads), 0, st, d_params, d_opts, n_options, (int)P, slots,
                       n_paths, (const double2*)part, d_price, d_stderr);
    HIP_TRY(hipGetLastError());
    return DH_OK;
}

extern "C" int dh_mc_price(dh_ctx* ctx, const double* params, int64_t P,
                           const dh_mc_option* options, int n_options, int64_t n_paths,
                           int steps_per_year, uint64_t seed, double* price, double* stderr_out) {
    int rc = dhmc::check_common(ctx, P, steps_per_year);
    if (rc) return rc;
    if (!params || !price || !stderr_out) return fail(DH_E_ARG, "null argument");
    rc = dhmc::check_params(params, P, steps_per_year);
    if (rc) return rc;
    if (n_paths < 2) return fail(DH_E_ARG, "n_paths must be >= 2, got " + std::to_string(n_paths));
    std::vector<dhmc::Opt> sorted;
    rc = dhmc::check_options(options, n_options, steps_per_year, sorted);
    if (rc) return rc;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t pb = (size_t)P * DH_PARAM_STRIDE * 8, ob = (size_t)P * n_options * 8;
    HIP_TRY(ctx->mc_params.reserve(pb));
    HIP_TRY(ctx->mc_out.reserve(2 * ob));
    hipStream_t st = ctx->stream;
    double* d_out = (double*)ctx->mc_out.ptr;
    HIP_TRY(hipMemcpyAsync(ctx->mc_params.ptr, params, pb, hipMemcpyHostToDevice, st));
    rc = dh_mc_price_dev(ctx, (const double*)ctx->mc_params.ptr, P, options, n_options, n_paths,
                         steps_per_year, seed, d_out, d_out + P * n_options, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(price, d_out, ob, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(stderr_out, d_out + P * n_options, ob, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}

extern "C" int dh_mc_paths(dh_ctx* ctx, const double* params, int64_t P, int n_obs,
                           const int32_t* obs_steps, int64_t path0, int64_t n_paths,
                           int steps_per_year, uint64_t seed, double* out) {
    const int rc = dhmc::check_paths(ctx, params, P, n_obs, obs_steps, path0, n_paths,
                                     steps_per_year, out);
    if (rc) return rc;
    const double words = (double)P * (double)n_paths * (double)n_obs * 6.0;
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
    const unsigned blocks = (unsigned)((n_paths + dhmc::kThreads - 1) / dhmc::kThreads);
    hipLaunchKernelGGL(dhmc::mc_paths_kernel, dim3(blocks, (unsigned)P), dim3(dhmc::kThreads), 0,
                       st, (const double*)ctx->mc_params.ptr, (const int32_t*)ctx->mc_opts.ptr,
                       n_obs, path0, n_paths, 1.0 / (double)steps_per_year, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (double*)ctx->mc_out.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, ctx->mc_out.ptr, ob, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}
