// dh_greeks.h -- analytic sensitivities of the COS price: delta, gamma, dual delta and the two v0
// vegas, with the price itself, in one pass (dh_surface_greeks*, dh_greeks_pairs).
// Included by dh_kernels.hip after dh_api.h; needs the kernels' helpers (xor_sum, option_logk) and
// dh_host.h.
//
// Definition.  With y = log(S_T / S0), xK = log(K / S0), [a, b] = truncationRange(L), u_k =
// k pi / (b - a) and w_k = phi(u_k) e^{-i u_k a}, the reference's price is (double_heston.py:160-192)
//     price = e^{-rT} sum'_{k < N} Re(w_k) V_k,   V_k = +-(2 / (b - a)) (S0 chi_k - K psi_k),
// chi_k, psi_k over [xK, b] with + for a call and over [a, xK] with - for a put, sum' halving k = 0.
// The Greeks are the partial derivatives of THIS series at fixed [a, b] and fixed absolute strike (a
// DH_STRIKE_PCT_SPOT strike is resolved to K = K_rel S0 / 100 first, then held):
//     delta      d/dS0     V_k -> +-(2 / (b - a)) chi_k
//     gamma      d2/dS0^2  V_k -> (2 / (b - a)) cos(u_k (xK - a)) K / S0^2     (call and put alike)
//     dual_delta d/dK      V_k -> -+(2 / (b - a)) psi_k
//     vega1      d/dv01    w_k -> w_k B1(u_k)
//     vega2      d/dv02    w_k -> w_k B2(u_k)
// (the boundary terms of d chi / dS0 and d psi / dS0 cancel because S0 e^{xK} = K; B_j is the factor
// heston_factor returns; the vegas are with respect to the variances v01, v02, not a volatility).
// They do NOT differentiate through the cumulant range or through the log(K / S0) -+ 0.1 clamp:
// that is the difference from a total derivative, of the size of the truncation error where the
// clamp is inactive and not small where it is active (DESIGN.md 3.17 has a measured example).
// Consequently price = S0 delta + K dual_delta holds to rounding, clamp or not.
//
// No tail cut: every term k < N is summed (gamma's coefficients cos(u_k (xK - a)) do not decay, so
// the price path's bound on the dropped terms does not carry over).  1 <= N <= DH_MAX_N.
//
// One block per (param set, tile of <= 256 options of one maturity):
//   1. the block fills LDS with Re(w_k), Re(w_k B1_k), Re(w_k B2_k) (halved at k = 0), k < N, on
//      the tile's unclamped range [a0, b0], and with the two reciprocals every option of the tile
//      needs per term, 1 / (1 + u_k^2) and 1 / u_k, one lane per term: five doubles per term, 80 KB
//      at N = 2048.  (With the three weights alone and the reciprocals formed per (option, term)
//      the C3 request took 9.2 pricing requests' time)
//   2. after a barrier every option whose own range is [a0, b0] runs one pass over k on kLanes
//      lanes (lane j: k = j, j + kLanes, ...), one sincos(u_k (xK - a0)) per (option, term) --
//      u_k (b0 - a0) = k pi gives +-1 and 0 without a call -- into six sums, then the xor butterfly
//      over the kLanes lanes;
//   3. an option whose range the clamp widens (xK - 0.1 < a0 or xK + 0.1 > b0, cos_exact_kernel's
//      rule) takes the per-term way on its own [a, b]: one wave per option, lane l the terms l,
//      l + 64, ... with their own CF, then the butterfly over 64 lanes.
// Every sum is in an order fixed by (N, the option's path) alone: no atomics, the same bits in any
// call, for any tile size, any P, on any stream, surface or pairs.
#pragma once

namespace dhgreeks {

using dh::cplx;

constexpr int kLanes = 16;                                 // lanes per option in the table pass
constexpr int kTabBytes = dh::kMathTab * (int)sizeof(double2);   // 5,648: a multiple of 16
static_assert(kTabBytes % 16 == 0, "LDS carve alignment");
static_assert(kLanes % 2 == 0 && kBlock % kLanes == 0, "a lane's terms share one parity");

struct GreekArgs {
    const double* prm;      // [P][16]
    int64_t p0;             // first param set (paired: first pair) of this launch
    const double* K;        // [M] sorted by T (surface) or [P] (paired)
    const double* T;
    const int8_t* call;
    const int* perm;        // surface: sorted -> caller index
    const int2* tiles;      // surface: (opt0, nopt)
    const int* tile_group;
    const double* group_T;
    int n_tiles;
    int paired;             // option i under param set i: one block per pair
    int strike_mode;
    int M;
    int N;
    double L;
    double* out;            // [DH_N_GREEKS][plane] ([DH_N_GREEKS_FULL][plane] for the full build)
    int64_t plane;          // P * M (surface) or P (paired)
};

// factor_x (dh_device.h) with the factor's B handed out: the same expressions, nothing added.
__device__ __forceinline__ cplx factor_x_b(const dh::FactorC& F, double u, double tau,
                                           const double2* __restrict__ sct, cplx& Bout) {
    const cplx beta = {F.kap, -(F.rs * u)};
    const double s2u = F.s2 * u;
    const cplx dd = {fma(beta.re, beta.re, -beta.im * beta.im) + s2u * u,
                     2.0 * beta.re * beta.im + s2u};
    double h, rh, sq, rs;
    dh::dsqrt_rsqrt_pos(fma(dd.re, dd.re, dd.im * dd.im), h, rh);
    dh::dsqrt_rsqrt_pos(0.5 * (h + fabs(dd.re)), sq, rs);
    const double other = 0.5 * dd.im * rs;
    const double dre = dd.re > 0.0 ? sq : fabs(other);
    const double dim = dd.re > 0.0 ? other : copysign(sq, dd.im);
    const cplx bm = {beta.re - dre, beta.im - dim};
    const cplx bp = {beta.re + dre, beta.im + dim};
    double es, ec;
    dh::dsincos_t(-dim * tau, sct, &es, &ec);
    const double em = dh::dexp_t_nonpos(-dre * tau, sct);
    const cplx e = {em * ec, em * es};
    const cplx D = {bp.re - (bm.re * e.re - bm.im * e.im), bp.im - (bm.re * e.im + bm.im * e.re)};
    const cplx ome = {1.0 - e.re, -e.im};
    const cplx num = dh::cmul(dh::cscale(bm, F.inv_s2), dh::cmul(ome, bp));
    const cplx B = dh::cdiv_rcp(num, D);
    const double lq2 = dh::dlog_t(fma(D.re, D.re, D.im * D.im) * (0.25 * rh), sct);
    const double aq = dh::datan2_t(fma(D.im, dre, -(D.re * dim)), fma(D.re, dre, D.im * dim), sct);
    Bout = B;
    return {F.coef * (bm.re * tau - lq2) + B.re * F.v0,
            F.coef * (bm.im * tau - 2.0 * aq) + B.im * F.v0};
}

// cf_phase_re (dh_device.h) with the vega weights: w = phi(u) e^{-i u a} = e^{Re E} e^{i (Im E -
// u a)} from the exponent's parts in cf_phase_from's order -> Re w, Re(w B1), Re(w B2).
__device__ __forceinline__ void cf_eval_b(const dh::CfConsts& C, double u, double tau, double a,
                                          const double2* __restrict__ sct, double& rw,
                                          double& rb1, double& rb2) {
    cplx B1, B2;
    const cplx X1 = factor_x_b(C.f1, u, tau, sct, B1);
    const cplx X2 = factor_x_b(C.f2, u, tau, sct, B2);
    cplx E = {0.0, C.drift * u};
    E = dh::cadd(E, X1);
    E = dh::cadd(E, X2);
    E = dh::cadd(E, dh::jump_x(C, u, sct));
    double ps, pc;
    dh::dsincos_t(E.im - u * a, sct, &ps, &pc);
    const double m = dh::dexp_t(E.re, sct);
    const double wr = m * pc, wi = m * ps;
    rw = wr;
    rb1 = wr * B1.re - wi * B1.im;
    rb2 = wr * B2.re - wi * B2.im;
}

struct Sums {
    double price, delta, gamma, dual, v1, v2;
};

// what a pass needs of its option and range
struct OptC {
    double S0, K, exk;      // exk = K / S0 = e^{xK}
    double c_even, c_odd;   // chi's constant term at even / odd k: +-e^b (call), -e^a (put)
    double sgn;             // sign of e^{xK}(cos + u sin) in chi and of sin / u in psi: -1 (call),
                            // +1 (put)
    double psi0;            // psi_0: b - xK (call), xK - a (put)
    bool call;
};

__device__ __forceinline__ void set_range(OptC& o, double xK, double a, double b, double ea,
                                          double eb) {
    o.c_even = o.call ? eb : -ea;
    o.c_odd = o.call ? -eb : -ea;
    o.sgn = o.call ? -1.0 : 1.0;
    o.psi0 = o.call ? b - xK : xK - a;
}

// Term k of the six sums.  chi_k, psi_k (double_heston.py:141-158) over [xK, b] (call) or [a, xK]
// (put), with sin and cos of u_k (b - a) = k pi and of u_k (a - a) = 0 written out; sn, cs = sin,
// cos(u_k (xK - a)); r1u2 = 1 / (1 + u^2), ru = 1 / u (not read at k = 0); cst = c_even or c_odd by
// k's parity.  At k = 0 (u = 0, sn = 0, cs = 1) chi's expression is e^d - e^c as it stands and psi
// is psi0.  rw, rb1, rb2 come weighted: halved at k = 0.
__device__ __forceinline__ void add_term(Sums& s, const OptC& o, int k, double u, double r1u2,
                                         double ru, double cst, double sn, double cs, double rw,
                                         double rb1, double rb2) {
    const double ex = o.exk * fma(u, sn, cs);
    const double chi = fma(o.sgn, ex, cst) * r1u2;
    const double psi = k == 0 ? o.psi0 : (o.sgn * sn) * ru;
    const double v = fma(o.S0, chi, -(o.K * psi));
    s.price = fma(rw, v, s.price);
    s.delta = fma(rw, chi, s.delta);
    s.gamma = fma(rw, cs, s.gamma);
    s.dual = fma(rw, psi, s.dual);
    s.v1 = fma(rb1, v, s.v1);
    s.v2 = fma(rb2, v, s.v2);
}

__device__ __forceinline__ void write_planes(const GreekArgs& A, int64_t at, const Sums& s,
                                             const OptC& o, double scale, double disc) {
    const double c = disc * (o.call ? scale : -scale);       // e^{-rT} (+-) 2 / (b - a)
    A.out[DH_GREEK_PRICE * A.plane + at] = c * s.price;
    A.out[DH_GREEK_DELTA * A.plane + at] = c * s.delta;
    A.out[DH_GREEK_GAMMA * A.plane + at] = (disc * scale) * (o.K / (o.S0 * o.S0)) * s.gamma;
    A.out[DH_GREEK_DUAL_DELTA * A.plane + at] = -c * s.dual;
    A.out[DH_GREEK_VEGA1 * A.plane + at] = c * s.v1;
    A.out[DH_GREEK_VEGA2 * A.plane + at] = c * s.v2;
}

__device__ __forceinline__ Sums butterfly(Sums s, int width) {
    s.price = xor_sum(s.price, width);
    s.delta = xor_sum(s.delta, width);
    s.gamma = xor_sum(s.gamma, width);
    s.dual = xor_sum(s.dual, width);
    s.v1 = xor_sum(s.v1, width);
    s.v2 = xor_sum(s.v2, width);
    return s;
}

// dynamic LDS: the CF's math tables, then the five per-term arrays [N rounded up to even] each,
// then one clamp flag per option of the tile
constexpr int kTermArrays = 5;     // Re w, Re(w B1), Re(w B2), 1 / (1 + u^2), 1 / u
inline size_t greeks_lds_bytes(int N) {
    return (size_t)kTabBytes + kTermArrays * (size_t)((N + 1) & ~1) * sizeof(double) + kTileMax;
}

// 3 waves per SIMD (<= 168 VGPRs): three blocks share a CU while their LDS fits
__global__ __launch_bounds__(kBlock, 3) void greeks_kernel(GreekArgs A) {
    extern __shared__ __attribute__((aligned(16))) char greeks_smem[];
    double2* sct = (double2*)greeks_smem;
    const int N = A.N, Np = (N + 1) & ~1;
    double* t_rw = (double*)(greeks_smem + kTabBytes);
    double* t_rb1 = t_rw + Np;
    double* t_rb2 = t_rb1 + Np;
    double* t_r1u2 = t_rb2 + Np;
    double* t_ru = t_r1u2 + Np;
    unsigned char* clamped = (unsigned char*)(t_ru + Np);
    const int tid = threadIdx.x;

    int64_t p, opt0;
    int nopt;
    double T;
    if (A.paired) {
        p = A.p0 + blockIdx.x;
        opt0 = p;
        nopt = 1;
        T = A.T[p];
    } else {
        p = A.p0 + blockIdx.x / A.n_tiles;
        const int tile = blockIdx.x % A.n_tiles;
        const int2 t = A.tiles[tile];
        opt0 = t.x;
        nopt = t.y;
        T = A.group_T[A.tile_group[tile]];
    }
    const Params P = dh::load_params(A.prm + p * DH_PARAM_STRIDE);
    dh::load_math_tables(sct, 0);
    double a0, b0;
    dh::trunc_unclamped(P, T, A.L, a0, b0);
    const dh::CfConsts CC = dh::cf_consts(P, T);
    const double disc = exp(-P.r * T);
    __syncthreads();

    // 1. the tile's table on [a0, b0]
    const double ba0 = b0 - a0;
    const double piba0 = dh::kPi / ba0;
    for (int k = tid; k < N; k += kBlock) {
        const double u = (double)k * piba0;
        double rw, rb1, rb2;
        cf_eval_b(CC, u, T, a0, sct, rw, rb1, rb2);
        const double wt = k == 0 ? 0.5 : 1.0;
        t_rw[k] = wt * rw;
        t_rb1[k] = wt * rb1;
        t_rb2[k] = wt * rb2;
        t_r1u2[k] = dh::drcp(fma(u, u, 1.0));
        t_ru[k] = dh::drcp(k == 0 ? 1.0 : u);
    }
    __syncthreads();

    // 2. options on the tile's range: kLanes lanes each, kBlock / kLanes options per round
    const double ea0 = exp(a0), eb0 = exp(b0);
    const int grp = tid / kLanes, j = tid % kLanes;
    for (int base = 0; base < nopt; base += kBlock / kLanes) {     // the same trips for every lane
        const int t = base + grp;
        const bool live = t < nopt;
        const int64_t m = opt0 + (live ? t : 0);
        OptC o;
        o.S0 = P.S0;
        o.K = A.strike_mode == DH_STRIKE_PCT_SPOT ? A.K[m] * P.S0 / 100.0 : A.K[m];
        o.call = A.call[m] != 0;
        const double xK = option_logk(o.K, P.S0, o.exk);
        const bool cl = (xK - 0.1 < a0) || (xK + 0.1 > b0);
        if (live && j == 0) clamped[t] = cl ? 1 : 0;
        set_range(o, xK, a0, b0, ea0, eb0);
        Sums s = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (live && !cl) {
            const double dx = xK - a0;
            const double cst = (j & 1) ? o.c_odd : o.c_even;      // kLanes is even: k's parity is j's
            for (int k = j; k < N; k += kLanes) {
                const double u = (double)k * piba0;
                double sn, cs;
                dh::dsincos_t(u * dx, sct, &sn, &cs);
                add_term(s, o, k, u, t_r1u2[k], t_ru[k], cst, sn, cs, t_rw[k], t_rb1[k],
                         t_rb2[k]);
            }
        }
        s = butterfly(s, kLanes);                                  // every lane of the wave
        if (live && !cl && j == 0)
            write_planes(A, A.paired ? p : p * A.M + A.perm[m], s, o, 2.0 / ba0, disc);
    }
    __syncthreads();

    // 3. clamp-widened options: the per-term way on their own range, one wave each
    const int wave = tid >> 6, lane = tid & 63;
    for (int t = wave; t < nopt; t += kBlock / 64) {
        if (!clamped[t]) continue;                                 // the same for the whole wave
        const int64_t m = opt0 + t;
        OptC o;
        o.S0 = P.S0;
        o.K = A.strike_mode == DH_STRIKE_PCT_SPOT ? A.K[m] * P.S0 / 100.0 : A.K[m];
        o.call = A.call[m] != 0;
        const double xK = option_logk(o.K, P.S0, o.exk);
        const double a = (xK - 0.1 < a0) ? xK - 0.1 : a0;          // double_heston.py:136-137
        const double b = (xK + 0.1 > b0) ? xK + 0.1 : b0;
        set_range(o, xK, a, b, exp(a), exp(b));
        const double ba = b - a;
        const double piba = dh::kPi / ba;
        const double dx = xK - a;
        Sums s = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const double cst = (lane & 1) ? o.c_odd : o.c_even;
        for (int k = lane; k < N; k += 64) {
            const double u = (double)k * piba;
            double rw, rb1, rb2, sn, cs;
            cf_eval_b(CC, u, T, a, sct, rw, rb1, rb2);
            dh::dsincos_t(u * dx, sct, &sn, &cs);
            const double wt = k == 0 ? 0.5 : 1.0;
            add_term(s, o, k, u, dh::drcp(fma(u, u, 1.0)), dh::drcp(k == 0 ? 1.0 : u), cst, sn, cs,
                     wt * rw, wt * rb1, wt * rb2);
        }
        s = butterfly(s, 64);
        if (lane == 0)
            write_planes(A, A.paired ? p : p * A.M + A.perm[m], s, o, 2.0 / ba, disc);
    }
}

// blocks of one launch at most (the grid's x extent is 2^31 - 1)
constexpr int64_t kMaxBlocks = int64_t(1) << 30;

int launch_greeks(dh_ctx* ctx, GreekArgs A, int64_t P, hipStream_t st) {
    const size_t lds = greeks_lds_bytes(A.N);
    // past the default cap of a launch's dynamic LDS (N > ~1000): raised once per context, to the
    // largest N's size, so that later requests make no runtime call but their launch
    if (lds > 48 * 1024 && ctx->greeks_lds == 0) {
        const size_t most = greeks_lds_bytes(DH_MAX_N);
        HIP_TRY(hipFuncSetAttribute((const void*)greeks_kernel,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
        ctx->greeks_lds = (int)most;
    }
    const int64_t per = A.paired ? 1 : A.n_tiles;                  // blocks per param set
    const int64_t sets = std::max<int64_t>(1, kMaxBlocks / per);   // param sets per launch
    for (int64_t p0 = 0; p0 < P; p0 += sets) {
        A.p0 = p0;
        const int64_t np = std::min(sets, P - p0);
        hipLaunchKernelGGL(greeks_kernel, dim3((unsigned)(np * per)), dim3(kBlock), lds, st, A);
        HIP_TRY(hipGetLastError());
    }
    return DH_OK;
}

// the checks every entry point makes before any device work; `count` names P or n
int check_greeks(const dh_ctx* ctx, int64_t count, const char* count_name, int N, double L) {
    if (!ctx) return fail(DH_E_ARG, "ctx is null");
    if (N < 1 || N > DH_MAX_N)
        return fail(DH_E_ARG, "N must be in [1, " + std::to_string(DH_MAX_N) + "], got " +
                                  std::to_string(N));
    if (count < 1)
        return fail(DH_E_ARG, std::string(count_name) + " must be >= 1, got " +
                                  std::to_string(count));
    if (!std::isfinite(L) || !(L > 0.0)) return fail(DH_E_ARG, "L must be finite and > 0");
    return DH_OK;
}

// The three entry points' bodies, over the build that answers them: `launch` is launch_greeks or
// the full build's (dh_greeks_full.h), `planes` the planes it writes.
using LaunchFn = int (*)(dh_ctx*, GreekArgs, int64_t, hipStream_t);

int surface_dev(dh_ctx* ctx, const dh_surface* s, const double* d_params, int64_t P, int N,
                double L, double* d_out, void* stream, LaunchFn launch) {
    int rc = check_greeks(ctx, P, "P", N, L);
    if (rc) return rc;
    if (!s) return fail(DH_E_ARG, "surface is null");
    if (!d_params) return fail(DH_E_ARG, "params is null");
    if (!d_out) return fail(DH_E_ARG, "out is null");
    if (s->M == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    GreekArgs A{};
    A.prm = d_params;
    A.K = s->K;
    A.T = s->T;
    A.call = s->call;
    A.perm = s->perm;
    A.tiles = s->tiles;
    A.tile_group = s->tile_group;
    A.group_T = s->group_T;
    A.n_tiles = s->n_tiles;
    A.strike_mode = s->strike_mode;
    A.M = s->M;
    A.N = N;
    A.L = L;
    A.out = d_out;
    A.plane = P * (int64_t)s->M;
    return launch(ctx, A, P, stream ? (hipStream_t)stream : ctx->stream);
}

int surface_host(dh_ctx* ctx, const dh_surface* s, const double* params, int64_t P, int N,
                 double L, double* out, LaunchFn launch, int planes) {
    int rc = check_greeks(ctx, P, "P", N, L);
    if (rc) return rc;
    if (!s) return fail(DH_E_ARG, "surface is null");
    if (!params) return fail(DH_E_ARG, "params is null");
    if (!out) return fail(DH_E_ARG, "out is null");
    if (s->M == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t pb = (size_t)P * DH_PARAM_STRIDE * 8, ob = (size_t)planes * P * s->M * 8;
    HIP_TRY(ctx->params.reserve(pb));
    HIP_TRY(ctx->out.reserve(ob));
    HIP_TRY(hipMemcpyAsync(ctx->params.ptr, params, pb, hipMemcpyHostToDevice, ctx->stream));
    rc = surface_dev(ctx, s, (const double*)ctx->params.ptr, P, N, L, (double*)ctx->out.ptr,
                     ctx->stream, launch);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, ctx->out.ptr, ob, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DH_OK;
}

int pairs_host(dh_ctx* ctx, const double* params, const double* K, const double* T,
               const int8_t* is_call, int64_t n, int N, double L, double* out, LaunchFn launch,
               int planes) {
    int rc = check_greeks(ctx, n, "n", N, L);
    if (rc) return rc;
    if (!params) return fail(DH_E_ARG, "params is null");
    if (!K) return fail(DH_E_ARG, "K is null");
    if (!T) return fail(DH_E_ARG, "T is null");
    if (!is_call) return fail(DH_E_ARG, "is_call is null");
    if (!out) return fail(DH_E_ARG, "out is null");
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t pb = (size_t)n * DH_PARAM_STRIDE * 8, vb = (size_t)n * 8;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx->params.reserve(pb));
    HIP_TRY(ctx->out.reserve(planes * vb));
    HIP_TRY(ctx->aux0.reserve(vb));
    HIP_TRY(ctx->aux1.reserve(vb));
    HIP_TRY(ctx->aux2.reserve((size_t)n));
    HIP_TRY(hipMemcpyAsync(ctx->params.ptr, params, pb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->aux0.ptr, K, vb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->aux1.ptr, T, vb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->aux2.ptr, is_call, (size_t)n, hipMemcpyHostToDevice, st));
    GreekArgs A{};
    A.prm = (const double*)ctx->params.ptr;
    A.K = (const double*)ctx->aux0.ptr;
    A.T = (const double*)ctx->aux1.ptr;
    A.call = (const int8_t*)ctx->aux2.ptr;
    A.paired = 1;
    A.strike_mode = DH_STRIKE_ABSOLUTE;
    A.N = N;
    A.L = L;
    A.out = (double*)ctx->out.ptr;
    A.plane = n;
    rc = launch(ctx, A, n, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, ctx->out.ptr, planes * vb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}

}  // namespace dhgreeks

extern "C" int dh_surface_greeks_dev(dh_ctx* ctx, const dh_surface* s, const double* d_params,
                                     int64_t P, int N, double L, double* d_out, void* stream) {
    return dhgreeks::surface_dev(ctx, s, d_params, P, N, L, d_out, stream,
                                 dhgreeks::launch_greeks);
}

extern "C" int dh_surface_greeks(dh_ctx* ctx, const dh_surface* s, const double* params,
                                 int64_t P, int N, double L, double* out) {
    return dhgreeks::surface_host(ctx, s, params, P, N, L, out, dhgreeks::launch_greeks,
                                  DH_N_GREEKS);
}

extern "C" int dh_greeks_pairs(dh_ctx* ctx, const double* params, const double* K, const double* T,
                               const int8_t* is_call, int64_t n, int N, double L, double* out) {
    return dhgreeks::pairs_host(ctx, params, K, T, is_call, n, N, L, out, dhgreeks::launch_greeks,
                                DH_N_GREEKS);
}
