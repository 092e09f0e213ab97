// dh_lsm.h -- American and Bermudan vanilla options by the least-squares Monte Carlo method of
// Longstaff and Schwartz (2001) on the paths of dh_mc.h (dh_lsm_price, dh_lsm_price_dev).  Included
// by dh_kernels.hip after dh_mc.h, whose step function, block prologue and checks it reuses.
// DESIGN.md 3.15.1 is the contract; tests/lsm_reference.py restates the backward pass in NumPy.
//
// Exercise dates are the steps e, 2 e, 3 e, ... (e = exercise_every; the start value is not a
// date), spaced Delta = e / steps_per_year; option j has D_j = step_j / e of them, the last its
// maturity.  Three kinds of launch, all on one stream:
//   lsm_paths_kernel   walks the paths of (seed, path, step) -- dh_mc_paths' paths, bit for bit --
//                      and stores S, v1, v2 at every date as [set][date][field][path];
//   lsm_back_kernel    one launch per date d = Dmax .. 1, grid (slots, n_options, P): fits the
//                      continuation value of date d from the sums the launch of date d + 1 left,
//                      exercises where the intrinsic value beats it, and leaves the sums of date
//                      d - 1;
//   lsm_finish_kernel  one thread per (set, option): prices and standard errors.
//
// Order of every sum (the 55 + 10 + 1 normal-equation sums, the cashflow sums, the maturity payoff
// sums): each thread adds the terms of its paths in chunk order from 0.0 (a block walks chunks
// slot, slot + slots, ...; thread t owns path chunk * 256 + t); then the 64 lanes of a wave by the
// xor butterfly, offsets 1 .. 32; then the four waves as (w0 + w1) + (w2 + w3); then the slots in
// slot order.  No atomics; arithmetic is uncontracted fp64.  The fitted value of a path is
// beta_0 + beta_1 phi_1 + ... + beta_9 phi_9 added in that order.
#pragma once
#pragma clang fp contract(off)

namespace dhlsm {

constexpr int kThreads = dhmc::kThreads;     // one chunk: 256 consecutive path indices
constexpr int kWaves = dhmc::kWaves;
constexpr int kSlots = DH_LSM_SLOTS;         // blocks per (set, option) of a backward launch
constexpr int kB = DH_LSM_BASIS;
constexpr int kTri = kB * (kB + 1) / 2;      // upper triangle of sum phi phi^T, row by row
constexpr int kRec = kTri + kB + 1;          // + sum phi Y + the in-the-money count
constexpr int kHalf = kRec / 2;              // sums a thread holds at once (lsm_back_kernel)
constexpr int kFin = 4;                      // sum cash, sum cash^2, sum payoff, sum payoff^2
constexpr double kMaxBytes = (double)DH_LSM_MAX_GIB * 1073741824.0;

struct Opt {
    double strike;
    int32_t is_call, dates;
};

// Forward kernel: grid (slots, P), chunks as mc_price_kernel.  Every lane walks its path (mc_step
// votes over the wave); lanes past n_paths are masked only at the stores.
__global__ __launch_bounds__(kThreads) void lsm_paths_kernel(
    const double* __restrict__ prm, int64_t n_paths, int64_t n_chunks, int every, int n_dates,
    double dt, double delta, uint32_t k0, uint32_t k1, double* __restrict__ state,
    double* __restrict__ disc) {
    __shared__ double sc[dhmc::kNConst];
    const int tid = threadIdx.x;
    const int set = blockIdx.y, slot = blockIdx.x, slots = gridDim.x;
    const double* rec = prm + (size_t)set * DH_PARAM_STRIDE;
    if (tid == 0 && slot == 0) disc[set] = exp(-rec[14] * delta);   // formed once per set
    const dhmc::SetK K = dhmc::block_constants(rec, dt, sc);
    double* base = state + (size_t)set * n_dates * 3 * n_paths;
    for (int64_t chunk = slot; chunk < n_chunks; chunk += slots) {
        const int64_t path = chunk * kThreads + tid;
        const bool active = path < n_paths;
        const uint32_t plo = (uint32_t)path, phi = (uint32_t)((uint64_t)path >> 32);
        dhmc::State s = dhmc::initial_state(sc);
        int step = 0;
        for (int date = 0; date < n_dates; ++date) {
            for (int k = 0; k < every; ++k) {
                ++step;
                dhmc::mc_step<false>(K, sc + dhmc::kCdf, dt, plo, phi, (uint32_t)step, k0, k1, s,
                                     s);         // no mirror: the last argument is not touched
            }
            if (active) {
                double* o = base + (size_t)date * 3 * n_paths + path;
                o[0] = s.S;
                o[n_paths] = s.v1;
                o[2 * n_paths] = s.v2;
            }
        }
    }
}

// the basis at (S, v1, v2): 1, x, y1, y2, x^2, y1^2, y2^2, x y1, x y2, y1 y2 with x = S / K - 1,
// y_i = v_i / theta_i - 1
__device__ __forceinline__ void basis(double S, double v1, double v2, double strike, double th1,
                                      double th2, double (&p)[kB]) {
    const double x = S / strike - 1.0, y1 = v1 / th1 - 1.0, y2 = v2 / th2 - 1.0;
    p[0] = 1.0, p[1] = x, p[2] = y1, p[3] = y2;
    p[4] = x * x, p[5] = y1 * y1, p[6] = y2 * y2;
    p[7] = x * y1, p[8] = x * y2, p[9] = y1 * y2;
}

// Entries [T0, T0 + kHalf) of a path's record -- the upper triangle of phi phi^T row by row, phi Y,
// the count -- added to acc; the entry numbers are compile-time after unrolling.
template <int T0>
__device__ __forceinline__ void add_terms(const double (&p)[kB], double Y, double (&acc)[kHalf]) {
    int t = 0;
#pragma unroll
    for (int a = 0; a < kB; ++a)
#pragma unroll
        for (int bb = a; bb < kB; ++bb, ++t)
            if (t >= T0 && t < T0 + kHalf) acc[t - T0] += p[a] * p[bb];
#pragma unroll
    for (int a = 0; a < kB; ++a, ++t)
        if (t >= T0 && t < T0 + kHalf) acc[t - T0] += p[a] * Y;
    if (t >= T0 && t < T0 + kHalf) acc[t - T0] += 1.0;
}

// The 10 x 10 normal equations G beta = rhs by Cholesky without pivoting, rows in basis order; one
// lane.  g holds G (full, symmetric) and is overwritten by the factor.  False where fewer than
// DH_LSM_MIN_ITM paths are in the money or a pivot is not > 0 (NaN included): beta is ten NaNs.
__device__ inline bool solve(double count, double (*g)[kB], const double* rhs, double* beta) {
    bool ok = count >= (double)DH_LSM_MIN_ITM;
    for (int j = 0; ok && j < kB; ++j) {
        double s = g[j][j];
        for (int k = 0; k < j; ++k) s = s - g[j][k] * g[j][k];
        if (!(s > 0.0)) {
            ok = false;
            break;
        }
        const double l = sqrt(s);
        g[j][j] = l;
        for (int i = j + 1; i < kB; ++i) {
            double t = g[i][j];
            for (int k = 0; k < j; ++k) t = t - g[i][k] * g[j][k];
            g[i][j] = t / l;
        }
    }
    if (ok) {
        for (int i = 0; i < kB; ++i) {       // L z = rhs
            double t = rhs[i];
            for (int k = 0; k < i; ++k) t = t - g[i][k] * beta[k];
            beta[i] = t / g[i][i];
        }
        for (int i = kB - 1; i >= 0; --i) {  // L^T beta = z
            double t = beta[i];
            for (int k = i + 1; k < kB; ++k) t = t - g[k][i] * beta[k];
            beta[i] = t / g[i][i];
        }
    } else {
        for (int i = 0; i < kB; ++i) beta[i] = __longlong_as_double(0x7FF8000000000000LL);
    }
    return ok;
}

// Backward kernel, date d: grid (slots, n_options, P).  part holds two sets of records
// [P][n_options][slots][kRec], the sums of date d in set d & 1: this launch reads set d & 1 (left
// by the launch of date d + 1) and writes set (d - 1) & 1.  fin [P][n_options][slots][kFin]: the
// maturity payoff sums at d == D_j, the cashflow sums at d == 1.
__global__ __launch_bounds__(kThreads) void lsm_back_kernel(
    const double* __restrict__ prm, const Opt* __restrict__ opts, const double* __restrict__ disc_of,
    int d, int n_dates, int64_t n_paths, int64_t n_chunks, const double* __restrict__ state,
    double* __restrict__ cash, int32_t* __restrict__ tau, double* part, double* __restrict__ fin,
    double* __restrict__ coef) {
    __shared__ double red[kWaves][kRec + kFin];
    __shared__ double g[kB][kB], rhs[kB], beta[kB];
    __shared__ int fit_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = blockIdx.x, slots = gridDim.x, j = blockIdx.y, n_opt = gridDim.y;
    const int set = blockIdx.z, P = gridDim.z;
    const Opt o = opts[j];
    if (o.dates < d) return;                 // the whole block: this option has no date d
    const size_t so = (size_t)set * n_opt + j;
    const bool regress = d < o.dates;
    if (regress) {
        const double* rd = part + (((size_t)(d & 1) * P * n_opt + so) * slots) * kRec;
        if (tid < kRec) {
            double s = 0.0;
            for (int k = 0; k < slots; ++k) s += rd[(size_t)k * kRec + tid];
            red[0][tid] = s;
        }
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int a = 0; a < kB; ++a)
                for (int b = a; b < kB; ++b, ++t) g[a][b] = g[b][a] = red[0][t];
            for (int a = 0; a < kB; ++a) rhs[a] = red[0][kTri + a];
            fit_s = solve(red[0][kTri + kB], g, rhs, beta) ? 1 : 0;
            if (slot == 0)
                for (int a = 0; a < kB; ++a) coef[(so * n_dates + (d - 1)) * kB + a] = beta[a];
        }
        __syncthreads();
    }
    const bool fit = regress && fit_s != 0;
    const double disc = disc_of[set];
    const double th1 = prm[(size_t)set * DH_PARAM_STRIDE + 2];
    const double th2 = prm[(size_t)set * DH_PARAM_STRIDE + 7];
    const double strike = o.strike;
    const bool is_call = o.is_call != 0;
    double b[kB];
#pragma unroll
    for (int a = 0; a < kB; ++a) b[a] = fit ? beta[a] : 0.0;
    const double* st_d = state + ((size_t)set * n_dates + (d - 1)) * 3 * n_paths;
    const double* st_p = d > 1 ? st_d - 3 * n_paths : st_d;   // date d - 1: read only where d > 1
    double* cs = cash + so * n_paths;
    int32_t* tu = tau + so * n_paths;
    // the record's sums in two passes over the block's paths, entries [0, kHalf) then
    // [kHalf, kRec), so that a thread holds at most kHalf running sums (all 66 at once spill)
    double acc[kHalf];
#pragma unroll
    for (int t = 0; t < kHalf; ++t) acc[t] = 0.0;
    double c1 = 0.0, c2 = 0.0, e1 = 0.0, e2 = 0.0;
    for (int64_t chunk = slot; chunk < n_chunks; chunk += slots) {
        const int64_t path = chunk * kThreads + tid;
        if (path < n_paths) {                // a lane past the end enters no sum
            const double S = st_d[path];
            const double h = is_call ? fmax(S - strike, 0.0) : fmax(strike - S, 0.0);
            double c;
            if (!regress) {
                c = h;
                tu[path] = d;
                e1 += h;
                e2 += h * h;
            } else {
                c = disc * cs[path];
                if (fit && h > 0.0) {
                    double p[kB];
                    basis(S, st_d[n_paths + path], st_d[2 * n_paths + path], strike, th1, th2, p);
                    double cont = b[0];
#pragma unroll
                    for (int a = 1; a < kB; ++a) cont = cont + b[a] * p[a];
                    if (h > cont) {
                        c = h;
                        tu[path] = d;
                    }
                }
            }
            cs[path] = c;
            if (d == 1) {
                c1 += c;
                c2 += c * c;
            } else {
                const double Sp = st_p[path];
                const double hp = is_call ? fmax(Sp - strike, 0.0) : fmax(strike - Sp, 0.0);
                if (hp > 0.0) {
                    double p[kB];
                    basis(Sp, st_p[n_paths + path], st_p[2 * n_paths + path], strike, th1, th2, p);
                    add_terms<0>(p, disc * c, acc);
                }
            }
        }
    }
    // every lane of the block is here: the butterfly needs whole waves
    if (d > 1) {
#pragma unroll
        for (int t = 0; t < kHalf; ++t) {
            const double s = xor_sum(acc[t], 64);
            if (lane == 0) red[wave][t] = s;
            acc[t] = 0.0;
        }
        for (int64_t chunk = slot; chunk < n_chunks; chunk += slots) {
            const int64_t path = chunk * kThreads + tid;
            if (path < n_paths) {
                const double Sp = st_p[path];
                const double hp = is_call ? fmax(Sp - strike, 0.0) : fmax(strike - Sp, 0.0);
                if (hp > 0.0) {
                    double p[kB];
                    basis(Sp, st_p[n_paths + path], st_p[2 * n_paths + path], strike, th1, th2, p);
                    add_terms<kHalf>(p, disc * cs[path], acc);   // cs: this thread's own store
                }
            }
        }
#pragma unroll
        for (int t = 0; t < kRec - kHalf; ++t) {
            const double s = xor_sum(acc[t], 64);
            if (lane == 0) red[wave][kHalf + t] = s;
        }
    }
    c1 = xor_sum(c1, 64), c2 = xor_sum(c2, 64), e1 = xor_sum(e1, 64), e2 = xor_sum(e2, 64);
    if (lane == 0) {
        red[wave][kRec] = c1, red[wave][kRec + 1] = c2;
        red[wave][kRec + 2] = e1, red[wave][kRec + 3] = e2;
    }
    __syncthreads();
    if (tid < kRec + kFin) {
        const double s = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        if (tid < kRec) {
            if (d > 1)
                part[((((size_t)((d - 1) & 1) * P * n_opt + so) * slots) + slot) * kRec + tid] = s;
        } else {
            const int f = tid - kRec;
            if (f < 2 ? d == 1 : !regress) fin[(so * slots + slot) * kFin + f] = s;
        }
    }
}

// Finishing kernel: one thread per (set, option); the slots' partials in slot order.  The European
// value of the same paths is discounted over the maturity on the date grid, D_j Delta.
__global__ __launch_bounds__(kThreads) void lsm_finish_kernel(
    const double* __restrict__ prm, const Opt* __restrict__ opts, const double* __restrict__ disc_of,
    int n_opt, int P, int slots, int64_t n_paths, double delta, const double* __restrict__ fin,
    double* __restrict__ price, double* __restrict__ err, double* __restrict__ euro,
    double* __restrict__ euro_err) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= P * n_opt) return;
    const int set = i / n_opt, j = i - set * n_opt;
    double s[kFin] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < slots; ++k)
        for (int f = 0; f < kFin; ++f) s[f] += fin[((size_t)i * slots + k) * kFin + f];
    const double n = (double)n_paths;
    const double disc = disc_of[set];
    const double disc_T =
        exp(-prm[(size_t)set * DH_PARAM_STRIDE + 14] * ((double)opts[j].dates * delta));
    price[i] = disc * s[0] / n;
    err[i] = disc * sqrt(fmax(s[1] - s[0] * s[0] / n, 0.0) / (n * (n - 1.0)));
    euro[i] = disc_T * s[2] / n;
    euro_err[i] = disc_T * sqrt(fmax(s[3] - s[2] * s[2] / n, 0.0) / (n * (n - 1.0)));
}

// ---- host side ---------------------------------------------------------------------------------
struct Plan {
    std::vector<Opt> opts;
    int n_dates = 0;                         // the longest D_j
};

// every check of the call that needs no parameter value, in the order the header lists them
int check_call(const dh_lsm_option* options, int n_options, int64_t P, int64_t n_paths,
               int steps_per_year, int exercise_every, Plan& plan) {
    if (n_paths < 2) return fail(DH_E_ARG, "n_paths must be >= 2, got " + std::to_string(n_paths));
    if (exercise_every < 1)
        return fail(DH_E_ARG, "exercise_every must be >= 1, got " + std::to_string(exercise_every));
    if (n_options < 1 || n_options > DH_LSM_MAX_OPTIONS)
        return fail(DH_E_ARG, "n_options must be in [1, " + std::to_string(DH_LSM_MAX_OPTIONS) +
                                  "], got " + std::to_string(n_options));
    if (!options) return fail(DH_E_ARG, "options is null");
    plan.opts.resize(n_options);
    for (int j = 0; j < n_options; ++j) {
        const dh_lsm_option& o = options[j];
        const std::string at = " of option " + std::to_string(j);
        if (!std::isfinite(o.strike) || o.strike < 0.0)
            return fail(DH_E_ARG, "options: strike" + at + " must be finite and >= 0");
        int32_t step;
        const int rc = dhmc::maturity_step(o.maturity, steps_per_year, at, step);
        if (rc) return rc;
        if (step % exercise_every != 0)
            return fail(DH_E_ARG, "options: maturity" + at + " (step " + std::to_string(step) +
                                      ") is not a whole multiple of exercise_every = " +
                                      std::to_string(exercise_every));
        const int dates = (int)(step / exercise_every);
        plan.opts[j] = {o.strike, o.is_call != 0, dates};
        plan.n_dates = std::max(plan.n_dates, dates);
    }
    // the state store [P][dates][3][n_paths] doubles plus each option's cashflow (double) and
    // exercise date (int32) per path
    const double bytes =
        (double)P * (double)n_paths * (24.0 * plan.n_dates + 12.0 * (double)n_options);
    if (bytes > kMaxBytes)
        return fail(DH_E_ARG, "n_paths: the path store of P x n_paths x (24 dates + 12 n_options) "
                              "bytes exceeds the cap of " + std::to_string(DH_LSM_MAX_GIB) +
                                  " GiB: fewer paths or parameter sets per call");
    return DH_OK;
}

// the launches; d_coef / d_tau null: the context's own scratch (read back by dh_lsm_price)
int run(dh_ctx* ctx, const double* d_params, int64_t P, const Plan& plan, int64_t n_paths,
        int steps_per_year, int exercise_every, uint64_t seed, double* d_price, double* d_err,
        double* d_euro, double* d_euro_err, double* d_coef, int32_t* d_tau, hipStream_t st) {
    const int n_opt = (int)plan.opts.size(), D = plan.n_dates;
    const int64_t n_chunks = (n_paths + kThreads - 1) / kThreads;
    const int fslots = (int)std::min<int64_t>(n_chunks, dhmc::kMaxSlots);
    const int slots = (int)std::min<int64_t>(n_chunks, kSlots);
    const size_t so = (size_t)P * n_opt, ob = (size_t)n_opt * sizeof(Opt);
    HIP_TRY(ctx->lsm_state.reserve((size_t)P * D * 3 * n_paths * 8));
    HIP_TRY(ctx->lsm_cash.reserve(so * n_paths * 8));
    HIP_TRY(ctx->lsm_part.reserve(2 * so * slots * kRec * 8));
    HIP_TRY(ctx->lsm_fin.reserve(so * slots * kFin * 8));
    HIP_TRY(ctx->lsm_opts.reserve(ob));
    HIP_TRY(ctx->lsm_disc.reserve((size_t)P * 8));
    if (!d_coef) {
        HIP_TRY(ctx->lsm_coef.reserve(so * D * kB * 8));
        d_coef = (double*)ctx->lsm_coef.ptr;
    }
    if (!d_tau) {
        HIP_TRY(ctx->lsm_tau.reserve(so * n_paths * 4));
        d_tau = (int32_t*)ctx->lsm_tau.ptr;
    }
    // pageable source: the copy has read plan.opts when the call returns
    HIP_TRY(hipMemcpyAsync(ctx->lsm_opts.ptr, plan.opts.data(), ob, hipMemcpyHostToDevice, st));
    // all-ones bytes are a NaN: rows no launch writes (the maturity date and past it) stay NaN
    HIP_TRY(hipMemsetAsync(d_coef, 0xFF, so * D * kB * 8, st));
    const Opt* d_opts = (const Opt*)ctx->lsm_opts.ptr;
    double* state = (double*)ctx->lsm_state.ptr;
    double* disc = (double*)ctx->lsm_disc.ptr;
    const double dt = 1.0 / (double)steps_per_year;
    const double delta = (double)exercise_every / (double)steps_per_year;
    hipLaunchKernelGGL(lsm_paths_kernel, dim3(fslots, (unsigned)P), dim3(kThreads), 0, st,
                       d_params, n_paths, n_chunks, exercise_every, D, dt, delta, (uint32_t)seed,
                       (uint32_t)(seed >> 32), state, disc);
    HIP_TRY(hipGetLastError());
    for (int d = D; d >= 1; --d) {
        hipLaunchKernelGGL(lsm_back_kernel, dim3(slots, n_opt, (unsigned)P), dim3(kThreads), 0, st,
                           d_params, d_opts, (const double*)disc, d, D, n_paths, n_chunks,
                           (const double*)state, (double*)ctx->lsm_cash.ptr, d_tau,
                           (double*)ctx->lsm_part.ptr, (double*)ctx->lsm_fin.ptr, d_coef);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(lsm_finish_kernel, dim3((unsigned)((so + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, st, d_params, d_opts, (const double*)disc, n_opt, (int)P,
                       slots, n_paths, delta, (const double*)ctx->lsm_fin.ptr, d_price, d_err,
                       d_euro, d_euro_err);
    HIP_TRY(hipGetLastError());
    return DH_OK;
}

}  // namespace dhlsm

extern "C" int dh_lsm_price_dev(dh_ctx* ctx, const double* d_params, int64_t P,
                                const dh_lsm_option* options, int n_options, int64_t n_paths,
                                int steps_per_year, int exercise_every, uint64_t seed,
                                double* d_price, double* d_stderr, double* d_european,
                                double* d_european_stderr, double* d_coef,
                                int32_t* d_exercise_date, void* stream) {
    int rc = dhmc::check_common(ctx, P, steps_per_year);
    if (rc) return rc;
    dhlsm::Plan plan;
    rc = dhlsm::check_call(options, n_options, P, n_paths, steps_per_year, exercise_every, plan);
    if (rc) return rc;
    if (!d_params || !d_price || !d_stderr || !d_european || !d_european_stderr)
        return fail(DH_E_ARG, "null argument");
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    return dhlsm::run(ctx, d_params, P, plan, n_paths, steps_per_year, exercise_every, seed,
                      d_price, d_stderr, d_european, d_european_stderr, d_coef, d_exercise_date,
                      stream ? (hipStream_t)stream : ctx->stream);
}

extern "C" int dh_lsm_price(dh_ctx* ctx, const double* params, int64_t P,
                            const dh_lsm_option* options, int n_options, int64_t n_paths,
                            int steps_per_year, int exercise_every, uint64_t seed, double* price,
                            double* stderr_out, double* european, double* european_stderr,
                            double* coef, int32_t* exercise_date) {
    int rc = dhmc::check_common(ctx, P, steps_per_year);
    if (rc) return rc;
    if (!params || !price || !stderr_out || !european || !european_stderr)
        return fail(DH_E_ARG, "null argument");
    rc = dhmc::check_params(params, P, steps_per_year);
    if (rc) return rc;
    dhlsm::Plan plan;
    rc = dhlsm::check_call(options, n_options, P, n_paths, steps_per_year, exercise_every, plan);
    if (rc) return rc;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t pb = (size_t)P * DH_PARAM_STRIDE * 8, so = (size_t)P * n_options, ob = so * 8;
    HIP_TRY(ctx->mc_params.reserve(pb));
    HIP_TRY(ctx->lsm_out.reserve(4 * ob));
    hipStream_t st = ctx->stream;
    double* d_out = (double*)ctx->lsm_out.ptr;
    HIP_TRY(hipMemcpyAsync(ctx->mc_params.ptr, params, pb, hipMemcpyHostToDevice, st));
    rc = dhlsm::run(ctx, (const double*)ctx->mc_params.ptr, P, plan, n_paths, steps_per_year,
                    exercise_every, seed, d_out, d_out + so, d_out + 2 * so, d_out + 3 * so,
                    nullptr, nullptr, st);
    if (rc) return rc;
    double* outs[4] = {price, stderr_out, european, european_stderr};
    for (int k = 0; k < 4; ++k)
        HIP_TRY(hipMemcpyAsync(outs[k], d_out + k * so, ob, hipMemcpyDeviceToHost, st));
    if (coef)
        HIP_TRY(hipMemcpyAsync(coef, ctx->lsm_coef.ptr, so * plan.n_dates * dhlsm::kB * 8,
                               hipMemcpyDeviceToHost, st));
    if (exercise_date)
        HIP_TRY(hipMemcpyAsync(exercise_date, ctx->lsm_tau.ptr, so * (size_t)n_paths * 4,
                               hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}
