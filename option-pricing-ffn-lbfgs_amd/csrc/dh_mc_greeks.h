// dh_mc_greeks.h -- delta, gamma and the two v0 vegas of the Monte Carlo path pricer from coupled
// paths in one walk (dh_mc_greeks*).  Included by dh_kernels.hip after dh_mc.h, whose Philox,
// uniform, Box-Muller, constants, payoff and host checks it uses.  DESIGN.md 3.15.3 is the
// contract; tests/mc_greeks_reference.py restates it in NumPy.
//
// Two facts of dhmc::mc_step carry the estimator.  Spot enters a path only as S = S0 exp(x), so
// S and its running maximum, minimum and sum are linear in S0: the path at spot S0 u is the base
// path with those four statistics times u, and the spot bumps need no walk.  And x is a sum of
// per-factor increments plus the jump and drift term, factor j's increment a function of v_j's
// path alone: bumping v0_j changes factor j's variance path and its increment and nothing else.
// A lane therefore walks the base path and the four paths from v0_1 +- d_1, v0_2 +- d_2 off one
// set of Philox blocks, Box-Muller pairs, Poisson count and jump draw: six factor steps per step
// where the plain walk has two, five exp, one of everything else.  The base state goes through the
// expressions of mc_step<false>, so the price plane is dh_mc_price's bits.
#pragma once
#pragma clang fp contract(off)

namespace dhmc {

constexpr int kGreeks = DH_MC_N_GREEKS;  // samples per (path, option): price, delta, gamma, vegas
constexpr int kGreekSums = 2 * kGreeks;  // sum and sum of squares of each

// what a path from a bumped v0_j carries of its own: the bumped factor's variance, the log-spot
// and the statistics of S (the other factor's variance is the base path's)
struct Bumped {
    double x, v, S, mx, mn, sm;
};

// factor_step's arithmetic with the increment returned, not added: v -> v' by QE and the
// parenthesised term that factor_step adds to x.  A copy of dh_mc.h's factor_step, expression for
// expression (dh_mc.h stays as it is so that the pricer's kernels stay instruction-identical): a
// change to either must be made to both, or the price plane stops being dh_mc_price's bits --
// tests/test_gpu_mc_greeks.py::test_price_plane_is_the_pricers_bits is what notices.  The same
// holds for track() / mc_greeks_step() against jump_and_track() / mc_step<false>().
__device__ __forceinline__ double factor_increment(const Factor& F, double dt, double u_v,
                                                   double z_v, double z_s, double& v) {
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
    const double inc = -0.5 * iv + F.rs * (vn - v - F.ktdt + F.kappa * iv) + sqrt(F.omr2 * iv) * z_s;
    v = vn;
    return inc;
}

// jump_and_track's arithmetic on a bumped path: `jump` is the base path's jump and drift term
__device__ __forceinline__ void track(const SetK& K, double jump, Bumped& b) {
    b.x = b.x + jump;
    b.S = K.S0 * exp(b.x);
    b.mx = fmax(b.mx, b.S);
    b.mn = fmin(b.mn, b.S);
    b.sm = b.sm + b.S;
}

// The step of mc_step<false> on the base path `s` and, off the same draws, on the four bumped
// paths: b[0], b[1] from v0_1 + d_1, v0_1 - d_1 (factor 1 walked anew, factor 2's increment the base
// path's), b[2], b[3] from v0_2 +- d_2 (the other way round).  Every lane of the wave must be
// active (the Poisson walk and the jump draw end by votes of the wave).
__device__ __forceinline__ void mc_greeks_step(const SetK& K, const double* cdf, double dt,
                                               uint32_t plo, uint32_t phi, uint32_t step,
                                               uint32_t k0, uint32_t k1, State& s, Bumped (&b)[4]) {
    uint32_t w[4];
    philox4x32_10(plo, phi, step, 0u, k0, k1, w);
    const double u_v1 = uniform53(w[0], w[1]), u_v2 = uniform53(w[2], w[3]);
    double z_v, z_s;
    philox4x32_10(plo, phi, step, 1u, k0, k1, w);
    box_muller(w, z_v, z_s);
    const double inc1 = factor_increment(K.f[0], dt, u_v1, z_v, z_s, s.v1);
    s.x = s.x + inc1;
    b[0].x = b[0].x + factor_increment(K.f[0], dt, u_v1, z_v, z_s, b[0].v);
    b[1].x = b[1].x + factor_increment(K.f[0], dt, u_v1, z_v, z_s, b[1].v);
    b[2].x = b[2].x + inc1;
    b[3].x = b[3].x + inc1;
    philox4x32_10(plo, phi, step, 2u, k0, k1, w);
    box_muller(w, z_v, z_s);
    const double inc2 = factor_increment(K.f[1], dt, u_v2, z_v, z_s, s.v2);
    s.x = s.x + inc2;
    b[0].x = b[0].x + inc2;
    b[1].x = b[1].x + inc2;
    b[2].x = b[2].x + factor_increment(K.f[1], dt, u_v2, z_v, z_s, b[2].v);
    b[3].x = b[3].x + factor_increment(K.f[1], dt, u_v2, z_v, z_s, b[3].v);
    philox4x32_10(plo, phi, step, 3u, k0, k1, w);
    const double u_n = uniform53(w[0], w[1]);
    int nj = 0;
    for (int k = 0; k < kCap; ++k) {     // N = #{k : U_N > cdf[k]}, ended by the wave's vote
        const bool above = u_n > cdf[k];
        if (__ballot(above) == 0) break;
        nj += above ? 1 : 0;
    }
    double z_j = 0.0, spare;
    if (__ballot(nj > 0) != 0) {
        philox4x32_10(plo, phi, step, 4u, k0, k1, w);
        box_muller(w, z_j, spare);
    }
    const double n = (double)nj;
    const double jump = (K.drift + n * K.mu_j) + (sqrt(n) * K.sig_j) * z_j;
    s.x = s.x + jump;
    s.S = K.S0 * exp(s.x);
    s.mx = fmax(s.mx, s.S);
    s.mn = fmin(s.mn, s.S);
    s.sm = s.sm + s.S;
#pragma unroll
    for (int k = 0; k < 4; ++k) track(K, jump, b[k]);
}

// dhmc::payoff on the state with S, max, min and sum each times u: the payoff at spot S0 u
__device__ __forceinline__ double payoff_scaled(const Opt& o, int step, const State& s, double u) {
    const State t = {s.x, s.v1, s.v2, u * s.S, u * s.mx, u * s.mn, u * s.sm};
    return payoff(o.kind, o.is_call, o.strike, o.barrier, step, t);
}

__device__ __forceinline__ double payoff_bumped(const Opt& o, int step, const Bumped& b) {
    const State t = {b.x, 0.0, 0.0, b.S, b.mx, b.mn, b.sm};
    return payoff(o.kind, o.is_call, o.strike, o.barrier, step, t);
}

// Path kernel: mc_price_kernel's grid (slots, P), block, chunk loop and walk over `opts`, ten sums
// per option.  part[((set * slots + slot) * n_opt + j) * 10 + 2 g + t] = the block's sum (t = 0) and
// sum of squares (t = 1) of sample g (DH_MC_GREEK_*) of sorted option j, in mc_price_kernel's order.
__global__ __launch_bounds__(kThreads) void mc_greeks_kernel(
    const double* __restrict__ prm, const Opt* __restrict__ opts, int n_opt, int64_t n_samples,
    int64_t n_chunks, int max_step, double dt, uint32_t k0, uint32_t k1, double eps, double bump,
    double* __restrict__ part) {
    __shared__ double sc[kNConst];
    __shared__ double red[kWaves][DH_MC_MAX_OPTIONS][kGreekSums];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int set = blockIdx.y, slot = blockIdx.x, slots = gridDim.x;
    const SetK K = block_constants(prm + (size_t)set * DH_PARAM_STRIDE, dt, sc);
    const double h = to_sgpr(eps * sc[kS0]), up = 1.0 + eps, um = 1.0 - eps;
    const double d1 = to_sgpr(bump * sc[kV0]), d2 = to_sgpr(bump * sc[kFactor + kV0]);
    double acc[kGreekSums] = {};         // thread j < n_opt owns sorted option j
    for (int64_t chunk = slot; chunk < n_chunks; chunk += slots) {
        const int64_t path = chunk * kThreads + tid;
        const bool active = path < n_samples;  // a lane past the end walks its path, pays 0
        const uint32_t plo = (uint32_t)path, phi = (uint32_t)((uint64_t)path >> 32);
        State s = initial_state(sc);
        Bumped b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double v0 = k < 2 ? s.v1 : s.v2, d = k < 2 ? d1 : d2;
            b[k] = {0.0, (k & 1) ? v0 - d : v0 + d, s.S, -INFINITY, INFINITY, 0.0};
        }
        int next = 0;
        int next_step = opts[0].step;
        for (int step = 1; step <= max_step; ++step) {
            mc_greeks_step(K, sc + kCdf, dt, plo, phi, (uint32_t)step, k0, k1, s, b);
            while (next_step == step) {
                const Opt o = opts[next];
                const double y = payoff(o.kind, o.is_call, o.strike, o.barrier, step, s);
                const double ysp = payoff_scaled(o, step, s, up);
                const double ysm = payoff_scaled(o, step, s, um);
                double g[kGreeks];
                g[DH_MC_GREEK_PRICE] = y;
                g[DH_MC_GREEK_DELTA] = (ysp - ysm) / (2.0 * h);
                g[DH_MC_GREEK_GAMMA] = ((ysp - y) + (ysm - y)) / (h * h);
                g[DH_MC_GREEK_VEGA1] =
                    (payoff_bumped(o, step, b[0]) - payoff_bumped(o, step, b[1])) / (2.0 * d1);
                g[DH_MC_GREEK_VEGA2] =
                    (payoff_bumped(o, step, b[2]) - payoff_bumped(o, step, b[3])) / (2.0 * d2);
#pragma unroll
                for (int q = 0; q < kGreeks; ++q) {
                    const double v = active ? g[q] : 0.0;
                    const double w1 = xor_sum(v, 64), w2 = xor_sum(v * v, 64);
                    if (lane == 0) red[wave][next][2 * q] = w1, red[wave][next][2 * q + 1] = w2;
                }
                ++next;
                next_step = next < n_opt ? opts[next].step : -1;
            }
        }
        __syncthreads();
        if (tid < n_opt) {
#pragma unroll
            for (int t = 0; t < kGreekSums; ++t)
                acc[t] += (red[0][tid][t] + red[1][tid][t]) + (red[2][tid][t] + red[3][tid][t]);
        }
        __syncthreads();
    }
    if (tid < n_opt) {
        double* p = part + (((size_t)set * slots + slot) * n_opt + tid) * kGreekSums;
#pragma unroll
        for (int t = 0; t < kGreekSums; ++t) p[t] = acc[t];
    }
}

// Finishing kernel: one thread per (set, sorted option); the slots' partials in slot order, then
// value and stderr [P][n_options][DH_MC_N_GREEKS] in the caller's option order, each by
// mc_finish_kernel's expressions for the plain mean and its error.
__global__ __launch_bounds__(kThreads) void mc_greeks_finish_kernel(
    const double* __restrict__ prm, const Opt* __restrict__ opts, int n_opt, int P, int slots,
    int64_t n_samples, const double* __restrict__ part, double* __restrict__ value,
    double* __restrict__ err) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= P * n_opt) return;
    const int set = i / n_opt, j = i - set * n_opt;
    double sum[kGreekSums] = {};
    const size_t first = (size_t)set * slots * n_opt + j;
    for (int k = 0; k < slots; ++k) {
        const double* p = part + (first + (size_t)k * n_opt) * kGreekSums;
#pragma unroll
        for (int t = 0; t < kGreekSums; ++t) sum[t] += p[t];
    }
    const double* rec = prm + (size_t)set * DH_PARAM_STRIDE;
    const double n = (double)n_samples;
    const double disc = exp(-rec[14] * opts[j].T);
    const size_t o = ((size_t)set * n_opt + opts[j].orig) * kGreeks;
#pragma unroll
    for (int g = 0; g < kGreeks; ++g) {
        const double cyy = sum[2 * g + 1] - sum[2 * g] * sum[2 * g] / n;
        value[o + g] = disc * sum[2 * g] / n;
        err[o + g] = disc * sqrt(fmax(cyy, 0.0) / (n * (n - 1.0)));
    }
}

// ---- host side ---------------------------------------------------------------------------------
int check_bumps(double spot_bump, double v0_bump) {
    if (!(spot_bump > 0.0 && spot_bump < 1.0))
        return fail(DH_E_ARG, "spot_bump must lie inside (0, 1), got " + std::to_string(spot_bump));
    if (!(v0_bump > 0.0 && v0_bump < 1.0))
        return fail(DH_E_ARG, "v0_bump must lie inside (0, 1), got " + std::to_string(v0_bump));
    return DH_OK;
}

// a relative bump of a v0 that is 0 would be empty
int check_v0(const double* params, int64_t P) {
    for (int64_t p = 0; p < P; ++p)
        for (int f = 0; f < 2; ++f)
            if (params[p * DH_PARAM_STRIDE + 5 * f] == 0.0)
                return fail(DH_E_ARG, std::string("params: v0") + (f ? "2" : "1") + " of set " +
                                          std::to_string(p) + " is 0: its relative bump v0_bump "
                                          "would be empty");
    return DH_OK;
}

int greeks_dev(dh_ctx* ctx, const double* d_params, int64_t P, const dh_mc_option* options,
               int n_options, int64_t n_paths, int steps_per_year, uint64_t seed, double spot_bump,
               double v0_bump, double* d_value, double* d_stderr, void* stream) {
    int rc = check_common(ctx, P, steps_per_year);
    if (rc) return rc;
    rc = check_walks(n_paths, 0, false);
    if (rc) return rc;
    std::vector<Opt> sorted;
    rc = check_options(options, n_options, steps_per_year, sorted);
    if (rc) return rc;
    rc = check_bumps(spot_bump, v0_bump);
    if (rc) return rc;
    if (!d_params || !d_value || !d_stderr) return fail(DH_E_ARG, "null argument");
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    const int64_t n_chunks = (n_paths + kThreads - 1) / kThreads;
    const int slots = (int)std::min<int64_t>(n_chunks, kMaxSlots);
    const size_t ob = (size_t)n_options * sizeof(Opt);
    HIP_TRY(ctx->mc_opts.reserve(ob));
    HIP_TRY(ctx->mc_part.reserve((size_t)P * slots * n_options * kGreekSums * 8));
    // pageable source: the copy has read `sorted` when the call returns
    HIP_TRY(hipMemcpyAsync(ctx->mc_opts.ptr, sorted.data(), ob, hipMemcpyHostToDevice, st));
    const Opt* d_opts = (const Opt*)ctx->mc_opts.ptr;
    double* part = (double*)ctx->mc_part.ptr;
    hipLaunchKernelGGL(mc_greeks_kernel, dim3(slots, (unsigned)P), dim3(kThreads), 0, st, d_params,
                       d_opts, n_options, n_paths, n_chunks, sorted.back().step,
                       1.0 / (double)steps_per_year, (uint32_t)seed, (uint32_t)(seed >> 32),
                       spot_bump, v0_bump, part);
    HIP_TRY(hipGetLastError());
    const int64_t n_out = P * n_options;
    hipLaunchKernelGGL(mc_greeks_finish_kernel,
                       dim3((unsigned)((n_out + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                       d_params, d_opts, n_options, (int)P, slots, n_paths, (const double*)part,
                       d_value, d_stderr);
    HIP_TRY(hipGetLastError());
    return DH_OK;
}

int greeks_host(dh_ctx* ctx, const double* params, int64_t P, const dh_mc_option* options,
                int n_options, int64_t n_paths, int steps_per_year, uint64_t seed,
                double spot_bump, double v0_bump, double* value, double* stderr_out) {
    int rc = check_common(ctx, P, steps_per_year);
    if (rc) return rc;
    if (!params || !value || !stderr_out) return fail(DH_E_ARG, "null argument");
    rc = check_params(params, P, steps_per_year);
    if (rc) return rc;
    rc = check_walks(n_paths, 0, false);
    if (rc) return rc;
    std::vector<Opt> sorted;
    rc = check_options(options, n_options, steps_per_year, sorted);
    if (rc) return rc;
    rc = check_bumps(spot_bump, v0_bump);
    if (rc) return rc;
    rc = check_v0(params, P);
    if (rc) return rc;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t n = (size_t)P * n_options * kGreeks, pb = (size_t)P * DH_PARAM_STRIDE * 8;
    HIP_TRY(ctx->mc_params.reserve(pb));
    HIP_TRY(ctx->mc_out.reserve(2 * n * 8));
    hipStream_t st = ctx->stream;
    double* d = (double*)ctx->mc_out.ptr;
    HIP_TRY(hipMemcpyAsync(ctx->mc_params.ptr, params, pb, hipMemcpyHostToDevice, st));
    rc = greeks_dev(ctx, (const double*)ctx->mc_params.ptr, P, options, n_options, n_paths,
                    steps_per_year, seed, spot_bump, v0_bump, d, d + n, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(value, d, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(stderr_out, d + n, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}

}  // namespace dhmc

extern "C" int dh_mc_greeks(dh_ctx* ctx, const double* params, int64_t P,
                            const dh_mc_option* options, int n_options, int64_t n_paths,
                            int steps_per_year, uint64_t seed, double spot_bump, double v0_bump,
                            double* value, double* stderr_out) {
    return dhmc::greeks_host(ctx, params, P, options, n_options, n_paths, steps_per_year, seed,
                             spot_bump, v0_bump, value, stderr_out);
}

extern "C" int dh_mc_greeks_dev(dh_ctx* ctx, const double* d_params, int64_t P,
                                const dh_mc_option* options, int n_options, int64_t n_paths,
                                int steps_per_year, uint64_t seed, double spot_bump,
                                double v0_bump, double* d_value, double* d_stderr, void* stream) {
    return dhmc::greeks_dev(ctx, d_params, P, options, n_options, n_paths, steps_per_year, seed,
                            spot_bump, v0_bump, d_value, d_stderr, stream);
}
