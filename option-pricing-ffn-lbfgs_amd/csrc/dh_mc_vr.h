// dh_mc_vr.h -- variance reduction for the Monte Carlo path pricer: antithetic pairs and control
// variates whose means the library knows exactly (dh_mc_price_vr, dh_mc_price_vr_dev,
// dh_mc_paths_vr).  Included by dh_kernels.hip after dh_mc.h, whose step, payoff and reduction it
// reuses.  DESIGN.md 3.15.2 is the contract; tests/mc_vr_reference.py restates it in NumPy.
//
// A lane of the antithetic kernel walks path i and its mirror side by side: one set of Philox
// blocks and one Box-Muller per step, applied as (U, Z) to the path and as (1 - U, -Z) to the
// mirror (1 - U is exact: U is an odd multiple of 2^-53).  The sample of the pair is the average of
// the two payoffs.  The control of an option is the terminal spot (mean S0 after discounting) for
// Europeans and strike-0 options, else the European payoff of the same strike, type and maturity,
// whose mean is the COS price dh_surface_price_dev puts on the device.  dh_mc.h's kernels are not
// touched: without the antithetic flag the walk is mc_step itself, so sum y and sum y^2 are
// dh_mc_price's bits.
#pragma once
#pragma clang fp contract(off)

namespace dhmc {

constexpr int kVrSums = 5;               // sum y, sum y^2, sum c, sum c^2, sum y c

// The jump count, the jump and the running statistics: the tail of mc_step, in its order.
__device__ __forceinline__ void jump_and_track(const SetK& K, int nj, double z_j, State& s) {
    const double n = (double)nj;
    s.x = s.x + ((K.drift + n * K.mu_j) + (sqrt(n) * K.sig_j) * z_j);
    s.S = K.S0 * exp(s.x);
    s.mx = fmax(s.mx, s.S);
    s.mn = fmin(s.mn, s.S);
    s.sm = s.sm + s.S;
}

// mc_step for path (plo, phi) in `s` and its mirror in `m`: the blocks and their order are
// mc_step's, each draw applied to the path and, mirrored, to the mirror.  Z_J is drawn where some
// lane of the wave jumped on either of its two paths (where it is not drawn it multiplies 0).
__device__ __forceinline__ void mc_step_pair(const SetK& K, const double* cdf, double dt,
                                             uint32_t plo, uint32_t phi, uint32_t step,
                                             uint32_t k0, uint32_t k1, State& s, State& m) {
    uint32_t w[4];
    philox4x32_10(plo, phi, step, 0u, k0, k1, w);
    const double u_v1 = uniform53(w[0], w[1]), u_v2 = uniform53(w[2], w[3]);
    double z_v, z_s;
    philox4x32_10(plo, phi, step, 1u, k0, k1, w);
    box_muller(w, z_v, z_s);
    factor_step(K.f[0], dt, u_v1, z_v, z_s, s.v1, s.x);
    factor_step(K.f[0], dt, 1.0 - u_v1, -z_v, -z_s, m.v1, m.x);
    philox4x32_10(plo, phi, step, 2u, k0, k1, w);
    box_muller(w, z_v, z_s);
    factor_step(K.f[1], dt, u_v2, z_v, z_s, s.v2, s.x);
    factor_step(K.f[1], dt, 1.0 - u_v2, -z_v, -z_s, m.v2, m.x);
    philox4x32_10(plo, phi, step, 3u, k0, k1, w);
    const double u_n = uniform53(w[0], w[1]), u_m = 1.0 - u_n;
    int nj = 0, njm = 0;
    for (int k = 0; k < kCap; ++k) {     // both counts are complete once no lane is above on
        const bool above = u_n > cdf[k], above_m = u_m > cdf[k];   // either path
        if (__ballot(above || above_m) == 0) break;
        nj += above ? 1 : 0;
        njm += above_m ? 1 : 0;
    }
    double z_j = 0.0, spare;
    if (__ballot(nj > 0 || njm > 0) != 0) {
        philox4x32_10(plo, phi, step, 4u, k0, k1, w);
        box_muller(w, z_j, spare);
    }
    jump_and_track(K, nj, z_j, s);
    jump_and_track(K, njm, -z_j, m);
}

// the control of one option on one path: S at the maturity step where the known mean is S0, else
// the European twin's payoff
__device__ __forceinline__ double control(const Opt& o, int step, const State& s) {
    const bool spot = o.kind == DH_MC_EUROPEAN || o.strike == 0.0;
    return spot ? s.S : payoff(DH_MC_EUROPEAN, o.is_call, o.strike, 0.0, step, s);
}

// Path kernel: grid (slots, P), mc_price_kernel's walk and reduction over n_samples samples
// (paths, or pairs under ANTI).  part[((set * slots + slot) * n_opt + j) * 5 + t] = the block's
// five sums of sorted option j; the three control sums are 0 without CTRL.
template <bool ANTI, bool CTRL>
__global__ __launch_bounds__(kThreads) void mc_vr_price_kernel(
    const double* __restrict__ prm, const Opt* __restrict__ opts, int n_opt, int64_t n_samples,
    int64_t n_chunks, int max_step, double dt, uint32_t k0, uint32_t k1,
    double* __restrict__ part) {
    __shared__ double sc[kNConst];
    __shared__ double red[kWaves][DH_MC_MAX_OPTIONS][kVrSums];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int set = blockIdx.y, slot = blockIdx.x, slots = gridDim.x;
    if (tid == 0) form_constants(prm + (size_t)set * DH_PARAM_STRIDE, dt, sc);
    __syncthreads();
    const SetK K = load_constants(sc);
    constexpr int kLive = CTRL ? kVrSums : 2;
    double acc[kVrSums] = {0.0, 0.0, 0.0, 0.0, 0.0};   // thread j < n_opt owns sorted option j
    for (int64_t chunk = slot; chunk < n_chunks; chunk += slots) {
        const int64_t path = chunk * kThreads + tid;
        const bool active = path < n_samples;  // a lane past the end walks its path, pays 0
        const uint32_t plo = (uint32_t)path, phi = (uint32_t)((uint64_t)path >> 32);
        State s = initial_state(sc), m = s;
        int next = 0;
        int next_step = opts[0].step;
        for (int step = 1; step <= max_step; ++step) {
            if (ANTI) mc_step_pair(K, sc + kCdf, dt, plo, phi, (uint32_t)step, k0, k1, s, m);
            else mc_step(K, sc + kCdf, dt, plo, phi, (uint32_t)step, k0, k1, s);
            while (next_step == step) {
                const Opt o = opts[next];
                double y = payoff(o.kind, o.is_call, o.strike, o.barrier, step, s);
                double c = CTRL ? control(o, step, s) : 0.0;
                if (ANTI) {
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
        double* p = part + (((size_t)set * slots + slot) * n_opt + tid) * kVrSums;
#pragma unroll
        for (int t = 0; t < kVrSums; ++t) p[t] = acc[t];
    }
}

// what the finishing kernel writes, each [P][n_options] in the caller's option order; the last
// four may be null
struct VrOut {
    double *price, *err, *base_price, *base_err, *beta, *mean;
};

// Finishing kernel: one thread per (set, sorted option); the slots' partials in slot order, then
// the estimator of DESIGN.md 3.15.2.  twin[j] = the option's column of cos [P][n_twins], or -1
// where the control's mean is S0; without `ctrl` beta = 0 and the mean is NaN.
__global__ __launch_bounds__(kThreads) void mc_vr_finish_kernel(
    const double* __restrict__ prm, const Opt* __restrict__ opts, const int32_t* __restrict__ twin,
    const double* __restrict__ cos, int n_twins, int n_opt, int P, int slots, int64_t n_samples,
    int ctrl, const double* __restrict__ part, VrOut out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= P * n_opt) return;
    const int set = i / n_opt, j = i - set * n_opt;
    double sy = 0.0, syy = 0.0, sc = 0.0, scc = 0.0, syc = 0.0;
    for (int k = 0; k < slots; ++k) {
        const double* p = part + (((size_t)set * slots + k) * n_opt + j) * kVrSums;
        sy += p[0];
        syy += p[1];
        sc += p[2];
        scc += p[3];
        syc += p[4];
    }
    const double* rec = prm + (size_t)set * DH_PARAM_STRIDE;
    const double n = (double)n_samples;
    const double disc = exp(-rec[14] * opts[j].T);
    const double cyy = syy - sy * sy / n;
    const double base_price = disc * sy / n;
    const double base_err = disc * sqrt(fmax(cyy, 0.0) / (n * (n - 1.0)));
    double beta = 0.0, mean = __builtin_nan(""), price = base_price, err = base_err;
    if (ctrl) {
        const double ccc = scc - sc * sc / n;
        const double cyc = syc - sy * sc / n;
        beta = ccc > 0.0 ? cyc / ccc : 0.0;
        mean = twin[j] < 0 ? rec[13] : cos[(size_t)set * n_twins + twin[j]];
        price = base_price - beta * (disc * sc / n - mean);
        err = disc * sqrt(fmax(cyy - beta * cyc, 0.0) / (n * (n - 1.0)));
    }
    const size_t o = (size_t)set * n_opt + opts[j].orig;
    out.price[o] = price;
    out.err[o] = err;
    if (out.base_price) out.base_price[o] = base_price;
    if (out.base_err) out.base_err[o] = base_err;
    if (out.beta) out.beta[o] = beta;
    if (out.mean) out.mean[o] = mean;
}

// the records with q (slot 15) zeroed: the path pricer does not read q, the COS pricer does
__global__ __launch_bounds__(kThreads) void mc_vr_records_kernel(const double* __restrict__ prm,
                                                                 int64_t n,
                                                                 double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = (i % DH_PARAM_STRIDE) == 15 ? 0.0 : prm[i];
}

// mc_paths_kernel for the mirrors: the pair is walked by the pricing kernel's own pair step and
// the mirror's statistics are written
__global__ __launch_bounds__(kThreads) void mc_vr_mirror_paths_kernel(
    const double* __restrict__ prm, const int32_t* __restrict__ obs, int n_obs, int64_t path0,
    int64_t n_paths, double dt, uint32_t k0, uint32_t k1, double* __restrict__ out) {
    __shared__ double sc[kNConst];
    const int tid = threadIdx.x;
    const int set = blockIdx.y;
    if (tid == 0) form_constants(prm + (size_t)set * DH_PARAM_STRIDE, dt, sc);
    __syncthreads();
    const SetK K = load_constants(sc);
    const int64_t i = (int64_t)blockIdx.x * kThreads + tid;
    const bool active = i < n_paths;     // whole waves walk (the pair step votes over the wave)
    const int64_t path = path0 + (active ? i : 0);
    const uint32_t plo = (uint32_t)path, phi = (uint32_t)((uint64_t)path >> 32);
    State s = initial_state(sc), m = s;
    int next = 0;
    int next_step = obs[0];
    const int max_step = obs[n_obs - 1];
    for (int step = 1; step <= max_step; ++step) {
        mc_step_pair(K, sc + kCdf, dt, plo, phi, (uint32_t)step, k0, k1, s, m);
        if (next_step == step) {
            if (active) {
                double* o = out + (((size_t)set * n_paths + i) * n_obs + next) * 6;
                o[0] = m.S, o[1] = m.v1, o[2] = m.v2, o[3] = m.mx, o[4] = m.mn, o[5] = m.sm;
            }
            ++next;
            next_step = next < n_obs ? obs[next] : -1;
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------
int check_vr(int64_t n_paths, int flags) {
    if (n_paths < 2) return fail(DH_E_ARG, "n_paths must be >= 2, got " + std::to_string(n_paths));
    if (flags == 0)
        return fail(DH_E_ARG, "flags is 0: neither antithetic nor control (that is dh_mc_price)");
    if (flags & ~(DH_MC_VR_ANTITHETIC | DH_MC_VR_CONTROL))
        return fail(DH_E_ARG, "flags has unknown bits: " + std::to_string(flags));
    if ((flags & DH_MC_VR_ANTITHETIC) && (n_paths % 2 != 0 || n_paths < 4))
        return fail(DH_E_ARG, "n_paths counts walks: under the antithetic flag it must be even "
                              "and >= 4, got " + std::to_string(n_paths));
    return DH_OK;
}

// The surface of the European twins of `sorted`, cached in the context by its (strike, maturity,
// type) list; twin[j] = sorted option j's column, -1 where its control is S.  A list that differs
// from the cached one waits for the stream that last read the old surface before replacing it.
int twins_surface(dh_ctx* ctx, const std::vector<Opt>& sorted, hipStream_t st,
                  std::vector<int32_t>& twin) {
    std::vector<double> key;
    std::vector<double> K, T;
    std::vector<int8_t> call;
    twin.assign(sorted.size(), -1);
    for (size_t j = 0; j < sorted.size(); ++j) {
        const Opt& o = sorted[j];
        if (o.kind == DH_MC_EUROPEAN || o.strike == 0.0) continue;
        twin[j] = (int32_t)K.size();
        K.push_back(o.strike);
        T.push_back(o.T);
        call.push_back(o.is_call ? 1 : 0);
        key.insert(key.end(), {o.strike, o.T, o.is_call ? 1.0 : 0.0});
    }
    const bool hit = ctx->vr_surf && key.size() == ctx->vr_key.size() &&
                     (key.empty() ||
                      std::memcmp(key.data(), ctx->vr_key.data(), key.size() * 8) == 0);
    if (!hit) {
        if (ctx->vr_surf) {
            HIP_TRY(hipStreamSynchronize(ctx->vr_stream));
            dh_surface_destroy(ctx->vr_surf);
            ctx->vr_surf = nullptr;
        }
        const int rc = dh_surface_create(ctx, K.data(), T.data(), call.data(), nullptr,
                                         (int)K.size(), DH_STRIKE_ABSOLUTE, &ctx->vr_surf);
        if (rc) return rc;
        ctx->vr_key = key;
    }
    ctx->vr_stream = st;
    return DH_OK;
}

template <bool ANTI, bool CTRL>
void launch_vr_price(dim3 grid, hipStream_t st, const double* d_params, const Opt* d_opts,
                     int n_opt, int64_t n_samples, int64_t n_chunks, int max_step, double dt,
                     uint32_t k0, uint32_t k1, double* part) {
    hipLaunchKernelGGL((mc_vr_price_kernel<ANTI, CTRL>), grid, dim3(kThreads), 0, st, d_params,
                       d_opts, n_opt, n_samples, n_chunks, max_step, dt, k0, k1, part);
}

}  // namespace dhmc

extern "C" int dh_mc_price_vr_dev(dh_ctx* ctx, const double* d_params, int64_t P,
                                  const dh_mc_option* options, int n_options, int64_t n_paths,
                                  int steps_per_year, uint64_t seed, int flags, double* d_price,
                                  double* d_stderr, double* d_base_price, double* d_base_stderr,
                                  double* d_beta, double* d_control_mean, void* stream) {
    int rc = dhmc::check_common(ctx, P, steps_per_year);
    if (rc) return rc;
    rc = dhmc::check_vr(n_paths, flags);
    if (rc) return rc;
    std::vector<dhmc::Opt> sorted;
    rc = dhmc::check_options(options, n_options, steps_per_year, sorted);
    if (rc) return rc;
    if (!d_params || !d_price || !d_stderr) return fail(DH_E_ARG, "null argument");
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    const bool anti = flags & DH_MC_VR_ANTITHETIC, ctrl = flags & DH_MC_VR_CONTROL;
    const int64_t n_samples = anti ? n_paths / 2 : n_paths;
    const int64_t n_chunks = (n_samples + dhmc::kThreads - 1) / dhmc::kThreads;
    const int slots = (int)std::min<int64_t>(n_chunks, dhmc::kMaxSlots);
    // the sorted options, then each one's column among the twins
    const size_t ob = (size_t)n_options * sizeof(dhmc::Opt), tb = (size_t)n_options * 4;
    std::vector<int32_t> twin(n_options, -1);
    int n_twins = 0;
    const double* d_cos = nullptr;
    if (ctrl) {
        rc = dhmc::twins_surface(ctx, sorted, st, twin);
        if (rc) return rc;
        n_twins = ctx->vr_surf->M;
    }
    HIP_TRY(ctx->mc_opts.reserve(ob + tb));
    HIP_TRY(ctx->mc_vr_part.reserve((size_t)P * slots * n_options * dhmc::kVrSums * 8));
    // pageable sources: the copies have read them when the calls return
    HIP_TRY(hipMemcpyAsync(ctx->mc_opts.ptr, sorted.data(), ob, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync((char*)ctx->mc_opts.ptr + ob, twin.data(), tb, hipMemcpyHostToDevice,
                           st));
    const dhmc::Opt* d_opts = (const dhmc::Opt*)ctx->mc_opts.ptr;
    const int32_t* d_twin = (const int32_t*)((const char*)ctx->mc_opts.ptr + ob);
    if (n_twins > 0) {
        // the twins' COS prices under the records with q = 0, on the device
        const int64_t n_el = P * DH_PARAM_STRIDE;
        HIP_TRY(ctx->mc_vr_rec.reserve((size_t)n_el * 8));
        HIP_TRY(ctx->mc_vr_cos.reserve((size_t)P * n_twins * 8));
        hipLaunchKernelGGL(dhmc::mc_vr_records_kernel,
                           dim3((unsigned)((n_el + dhmc::kThreads - 1) / dhmc::kThreads)),
                           dim3(dhmc::kThreads), 0, st, d_params, n_el,
                           (double*)ctx->mc_vr_rec.ptr);
        HIP_TRY(hipGetLastError());
        const int last_path = ctx->last_path;
        rc = dh_surface_price_dev(ctx, ctx->vr_surf, (const double*)ctx->mc_vr_rec.ptr, P,
                                  DH_MC_VR_COS_N, DH_MC_VR_COS_L, (double*)ctx->mc_vr_cos.ptr, st);
        ctx->last_path = last_path;
        if (rc) return rc;
        d_cos = (const double*)ctx->mc_vr_cos.ptr;
    }
    double* part = (double*)ctx->mc_vr_part.ptr;
    const double dt = 1.0 / (double)steps_per_year;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const dim3 grid(slots, (unsigned)P);
    auto launch = anti ? (ctrl ? dhmc::launch_vr_price<true, true>
                               : dhmc::launch_vr_price<true, false>)
                       : dhmc::launch_vr_price<false, true>;
    launch(grid, st, d_params, d_opts, n_options, n_samples, n_chunks, sorted.back().step, dt, k0,
           k1, part);
    HIP_TRY(hipGetLastError());
    const int64_t n_out = P * n_options;
    const dhmc::VrOut out{d_price, d_stderr, d_base_price, d_base_stderr, d_beta, d_control_mean};
    hipLaunchKernelGGL(dhmc::mc_vr_finish_kernel,
                       dim3((unsigned)((n_out + dhmc::kThreads - 1) / dhmc::kThreads)),
                       dim3(dhmc::kThreads), 0, st, d_params, d_opts, d_twin, d_cos, n_twins,
                       n_options, (int)P, slots, n_samples, ctrl ? 1 : 0, (const double*)part, out);
    HIP_TRY(hipGetLastError());
    return DH_OK;
}

extern "C" int dh_mc_price_vr(dh_ctx* ctx, const double* params, int64_t P,
                              const dh_mc_option* options, int n_options, int64_t n_paths,
                              int steps_per_year, uint64_t seed, int flags, double* price,
                              double* stderr_out, double* base_price, double* base_stderr,
                              double* beta, double* control_mean) {
    int rc = dhmc::check_common(ctx, P, steps_per_year);
    if (rc) return rc;
    if (!params || !price || !stderr_out) return fail(DH_E_ARG, "null argument");
    rc = dhmc::check_params(params, P, steps_per_year);
    if (rc) return rc;
    rc = dhmc::check_vr(n_paths, flags);
    if (rc) return rc;
    std::vector<dhmc::Opt> sorted;
    rc = dhmc::check_options(options, n_options, steps_per_year, sorted);
    if (rc) return rc;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t pb = (size_t)P * DH_PARAM_STRIDE * 8, ob = (size_t)P * n_options * 8;
    HIP_TRY(ctx->mc_params.reserve(pb));
    HIP_TRY(ctx->mc_out.reserve(6 * ob));
    hipStream_t st = ctx->stream;
    double* d_out = (double*)ctx->mc_out.ptr;
    const size_t n = (size_t)P * n_options;
    HIP_TRY(hipMemcpyAsync(ctx->mc_params.ptr, params, pb, hipMemcpyHostToDevice, st));
    rc = dh_mc_price_vr_dev(ctx, (const double*)ctx->mc_params.ptr, P, options, n_options, n_paths,
                            steps_per_year, seed, flags, d_out, d_out + n, d_out + 2 * n,
                            d_out + 3 * n, d_out + 4 * n, d_out + 5 * n, st);
    if (rc) return rc;
    double* const host[6] = {price, stderr_out, base_price, base_stderr, beta, control_mean};
    for (int k = 0; k < 6; ++k)
        if (host[k]) HIP_TRY(hipMemcpyAsync(host[k], d_out + k * n, ob, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}

extern "C" int dh_mc_paths_vr(dh_ctx* ctx, const double* params, int64_t P, int n_obs,
                              const int32_t* obs_steps, int64_t path0, int64_t n_paths,
                              int steps_per_year, uint64_t seed, int mirror, double* out) {
    if (!mirror)
        return dh_mc_paths(ctx, params, P, n_obs, obs_steps, path0, n_paths, steps_per_year, seed,
                           out);
    int rc = dhmc::check_paths(ctx, params, P, n_obs, obs_steps, path0, n_paths, steps_per_year,
                               out);
    if (rc) return rc;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t pb = (size_t)P * DH_PARAM_STRIDE * 8, sb = (size_t)n_obs * 4;
    const size_t ob = (size_t)P * (size_t)n_paths * (size_t)n_obs * 6 * 8;
    HIP_TRY(ctx->mc_params.reserve(pb));
    HIP_TRY(ctx->mc_opts.reserve(sb));
    HIP_TRY(ctx->mc_out.reserve(ob));
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(ctx->mc_params.ptr, params, pb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->mc_opts.ptr, obs_steps, sb, hipMemcpyHostToDevice, st));
    const unsigned blocks = (unsigned)((n_paths + dhmc::kThreads - 1) / dhmc::kThreads);
    hipLaunchKernelGGL(dhmc::mc_vr_mirror_paths_kernel, dim3(blocks, (unsigned)P),
                       dim3(dhmc::kThreads), 0, st, (const double*)ctx->mc_params.ptr,
                       (const int32_t*)ctx->mc_opts.ptr, n_obs, path0, n_paths,
                       1.0 / (double)steps_per_year, (uint32_t)seed, (uint32_t)(seed >> 32),
                       (double*)ctx->mc_out.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, ctx->mc_out.ptr, ob, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}
