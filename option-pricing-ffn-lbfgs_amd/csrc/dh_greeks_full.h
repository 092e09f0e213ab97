// dh_greeks_full.h -- the "full" build of the Greeks pass: dh_greeks.h's six planes, bit for bit,
// and with them the maturity and rate sensitivities, the dual gamma and Dupire's local variance
// (dh_surface_greeks_full*, dh_greeks_full_pairs).  Included by dh_kernels.hip
// after dh_greeks.h, whose option pass (OptC, set_range, add_term, write_planes), arguments and
// host bodies it uses; greeks_kernel itself is not touched.
//
// Definition.  In dh_greeks.h's notation (price = e^{-rT} sum'_k Re(w_k) V_k, w_k = phi(u_k)
// e^{-i u_k a}), the four further planes are, like the six, partial derivatives of the series at a
// FIXED range [a, b] (so at fixed u_k) and a fixed absolute strike:
//     dprice_dT   d/dT     = -r price + e^{-rT} sum'_k Re(w_k G_k) V_k,   G = d log phi / d tau
//     rho         d/dr     = -T price + e^{-rT} sum'_k (-u_k T Im w_k) V_k
//     dual_gamma  d2/dK^2  : V_k -> (2 / (b - a)) cos(u_k (xK - a)) / K     (call and put alike)
//     local_var   Dupire's quotient of the planes (below)
// G.  phi = exp(i drift u + X1 + X2 + J) with the drift and the jump exponent J linear in tau and
// X_j = (kappa_j theta_j / sigma_j^2)((beta_j - d_j) tau - 2 log Q_j) + B_j v0_j, whose tau-derivative
// is kappa_j theta_j B_j + v0_j B_j' (A_j' = kappa_j theta_j B_j), so
//     G = (i drift u + J) / tau + sum_j (kappa_j theta_j B_j + v0_j B_j').
// B_j' is the Riccati right side 1/2 sigma^2 B^2 - (kappa - i rho sigma u) B - 1/2 (u^2 + i u); its
// three terms are O(u^2) each and cancel to O(e^{-d tau}) at large u, so it is evaluated in the
// equal closed form, from d/d tau of B = ((beta - d) / sigma^2)(1 - e) / (1 - g e),
//     B' = -2 u (u + i) d^2 e / D^2,     e = e^{-d tau},  D = (beta + d) - (beta - d) e,
// which has no cancellation (d^2, e and D are factor_x_b's dd, e and D).
// rho: r enters the discount and the drift's i (r - q) T u only, so d w / d r = i u T w.
// d price / d q = -(rho + T price) needs no plane.
// dual_gamma: at a fixed range the series is homogeneous of degree one in (S0, K) -- price = S0
// delta + K dual_delta -- hence K^2 dual_gamma = S0^2 gamma: gamma's sum with 1 / K where gamma has
// K / S0^2.  e^{rT} dual_gamma is the risk-neutral density of S_T at K.
//
// local_var.  Dupire's formula with rates and dividends, the same for calls and puts (the parity
// terms cancel); with jumps it is the model's Markovian projection.  Formed from the planes just
// written, in plain fp64, every operation rounded on its own (no contraction), in this order:
//     num = (dprice_dT + ((r - q) * K) * dual_delta) + q * price
//     den = (0.5 * (K * K)) * dual_gamma
//     local_var = num / den
// where dprice_dT, price, dual_delta and dual_gamma are finite and den > 0, NaN otherwise; a
// negative quotient is not clipped.  A host that repeats the order gets the same bits.
//
// The pass is greeks_kernel's: one block per (param set, tile of <= 256 options of one maturity),
// the table on [a0, b0] in LDS -- seven doubles per term, the two new ones Re(w_k G_k) and -u_k T
// Im(w_k), halved at k = 0: 120,592 B at N = 2048 -- then kLanes lanes per option with one sincos
// per (option, term) into eight sums (dual gamma shares gamma's), the xor butterfly, and the
// clamp-widened options the per-term way on their own range, one wave each.  The six sums of
// dh_greeks.h are formed by its own add_term from the same table values, so the six planes are
// greeks_kernel's bits.  No atomics: every sum's order is fixed by (N, the option's path) alone.
#pragma once

namespace dhgfull {

using dh::cplx;
using dhgreeks::GreekArgs;
using dhgreeks::kLanes;
using dhgreeks::kTabBytes;
using dhgreeks::OptC;

// what G needs beside CfConsts, per (param set, T)
struct TauC {
    double inv_tau, kt1, kt2, T;      // 1 / tau, kappa_j theta_j, tau
};

// factor_x_b (dh_greeks.h) with B' handed out: the same expressions for X and B, and
// B' = -2 u (u + i) dd e / D^2 from its dd, e and D.
__device__ __forceinline__ cplx factor_x_bt(const dh::FactorC& F, double u, double tau,
                                            const double2* __restrict__ sct, cplx& Bout,
                                            cplx& dBout) {
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
    const cplx q = dh::cdiv_rcp(dh::cmul(dd, e), dh::cmul(D, D));
    const cplx uq = dh::cmul({u * u, u}, q);
    dBout = {-2.0 * uq.re, -2.0 * uq.im};
    return {F.coef * (bm.re * tau - lq2) + B.re * F.v0,
            F.coef * (bm.im * tau - 2.0 * aq) + B.im * F.v0};
}

// cf_eval_b (dh_greeks.h) with the maturity and rate weights: Re w, Re(w B1), Re(w B2) as there,
// and Re(w G), -u T Im w.
__device__ __forceinline__ void cf_eval_bt(const dh::CfConsts& C, const TauC& Q, double u,
                                           double tau, double a, const double2* __restrict__ sct,
                                           double& rw, double& rb1, double& rb2, double& rg,
                                           double& rr) {
    cplx B1, B2, dB1, dB2;
    const cplx X1 = factor_x_bt(C.f1, u, tau, sct, B1, dB1);
    const cplx X2 = factor_x_bt(C.f2, u, tau, sct, B2, dB2);
    const cplx J = dh::jump_x(C, u, sct);
    cplx E = {0.0, C.drift * u};
    E = dh::cadd(E, X1);
    E = dh::cadd(E, X2);
    E = dh::cadd(E, J);
    double ps, pc;
    dh::dsincos_t(E.im - u * a, sct, &ps, &pc);
    const double m = dh::dexp_t(E.re, sct);
    const double wr = m * pc, wi = m * ps;
    rw = wr;
    rb1 = wr * B1.re - wi * B1.im;
    rb2 = wr * B2.re - wi * B2.im;
    const double gre = J.re * Q.inv_tau +
                       ((Q.kt1 * B1.re + C.f1.v0 * dB1.re) + (Q.kt2 * B2.re + C.f2.v0 * dB2.re));
    const double gim = (C.drift * u + J.im) * Q.inv_tau +
                       ((Q.kt1 * B1.im + C.f1.v0 * dB1.im) + (Q.kt2 * B2.im + C.f2.v0 * dB2.im));
    rg = wr * gre - wi * gim;
    rr = -((u * Q.T) * wi);
}

struct SumsF {
    dhgreeks::Sums s;       // dh_greeks.h's six, formed by its add_term
    double dT, rho;
};

// term k of the eight sums: rg, rr come weighted like rw (halved at k = 0)
__device__ __forceinline__ void add_term_full(SumsF& f, const OptC& o, int k, double u, double r1u2,
                                              double ru, double cst, double sn, double cs,
                                              double rw, double rb1, double rb2, double rg,
                                              double rr) {
    dhgreeks::add_term(f.s, o, k, u, r1u2, ru, cst, sn, cs, rw, rb1, rb2);
    // V_k without its +-(2 / (b - a)), add_term's expressions
    const double ex = o.exk * fma(u, sn, cs);
    const double chi = fma(o.sgn, ex, cst) * r1u2;
    const double psi = k == 0 ? o.psi0 : (o.sgn * sn) * ru;
    const double v = fma(o.S0, chi, -(o.K * psi));
    f.dT = fma(rg, v, f.dT);
    f.rho = fma(rr, v, f.rho);
}

__device__ __forceinline__ SumsF butterfly_full(SumsF f, int width) {
    f.s = dhgreeks::butterfly(f.s, width);
    f.dT = xor_sum(f.dT, width);
    f.rho = xor_sum(f.rho, width);
    return f;
}

// Dupire's quotient of the planes, in the header comment's order; every operation rounded on its
// own, so that a host repeats it
__device__ __forceinline__ double local_var_of(double dT, double price, double dual, double dgam,
                                               double K, double r, double q) {
#pragma clang fp contract(off)
    const double num = (dT + ((r - q) * K) * dual) + q * price;
    const double den = (0.5 * (K * K)) * dgam;
    const bool ok = isfinite(dT) && isfinite(price) && isfinite(dual) && isfinite(dgam) &&
                    den > 0.0;
    return ok ? num / den : __builtin_nan("");
}

__device__ __forceinline__ void write_planes_full(const GreekArgs& A, int64_t at, const SumsF& f,
                                                  const OptC& o, double scale, double disc,
                                                  double r, double q, double T) {
    dhgreeks::write_planes(A, at, f.s, o, scale, disc);
    const double c = disc * (o.call ? scale : -scale);       // write_planes' factor
    const double price = c * f.s.price;
    const double dual = -c * f.s.dual;
    const double dT = fma(c, f.dT, -(r * price));
    const double rho = fma(c, f.rho, -(T * price));
    const double dgam = (disc * scale) * (f.s.gamma / o.K);
    A.out[DH_GREEK_DPRICE_DT * A.plane + at] = dT;
    A.out[DH_GREEK_RHO * A.plane + at] = rho;
    A.out[DH_GREEK_DUAL_GAMMA * A.plane + at] = dgam;
    A.out[DH_GREEK_LOCAL_VAR * A.plane + at] = local_var_of(dT, price, dual, dgam, o.K, r, q);
}

// dynamic LDS: the CF's math tables, then the seven per-term arrays [N rounded up to even] each,
// then one clamp flag per option of the tile: 49,136 B at N = 772, 49,248 B at N = 773
constexpr int kTermArrays = 7;     // dh_greeks.h's five, Re(w G), -u T Im w
inline size_t greeks_full_lds_bytes(int N) {
    return (size_t)kTabBytes + kTermArrays * (size_t)((N + 1) & ~1) * sizeof(double) + kTileMax;
}
static_assert(kTabBytes + kTermArrays * DH_MAX_N * 8 + kTileMax <= kLdsMax, "LDS of a workgroup");

__global__ __launch_bounds__(kBlock, 3) void greeks_full_kernel(GreekArgs A) {
    extern __shared__ __attribute__((aligned(16))) char greeks_full_smem[];
    double2* sct = (double2*)greeks_full_smem;
    const int N = A.N, Np = (N + 1) & ~1;
    double* t_rw = (double*)(greeks_full_smem + kTabBytes);
    double* t_rb1 = t_rw + Np;
    double* t_rb2 = t_rb1 + Np;
    double* t_r1u2 = t_rb2 + Np;
    double* t_ru = t_r1u2 + Np;
    double* t_rg = t_ru + Np;
    double* t_rr = t_rg + Np;
    unsigned char* clamped = (unsigned char*)(t_rr + Np);
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
    const TauC TC = {1.0 / T, P.k1 * P.t1, P.k2 * P.t2, T};
    const double disc = exp(-P.r * T);
    __syncthreads();

    // 1. the tile's table on [a0, b0]
    const double ba0 = b0 - a0;
    const double piba0 = dh::kPi / ba0;
    for (int k = tid; k < N; k += kBlock) {
        const double u = (double)k * piba0;
        double rw, rb1, rb2, rg, rr;
        cf_eval_bt(CC, TC, u, T, a0, sct, rw, rb1, rb2, rg, rr);
        const double wt = k == 0 ? 0.5 : 1.0;
        t_rw[k] = wt * rw;
        t_rb1[k] = wt * rb1;
        t_rb2[k] = wt * rb2;
        t_r1u2[k] = dh::drcp(fma(u, u, 1.0));
        t_ru[k] = dh::drcp(k == 0 ? 1.0 : u);
        t_rg[k] = wt * rg;
        t_rr[k] = wt * rr;
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
        dhgreeks::set_range(o, xK, a0, b0, ea0, eb0);
        SumsF f = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, 0.0, 0.0};
        if (live && !cl) {
            const double dx = xK - a0;
            const double cst = (j & 1) ? o.c_odd : o.c_even;      // kLanes is even: k's parity is j's
            for (int k = j; k < N; k += kLanes) {
                const double u = (double)k * piba0;
                double sn, cs;
                dh::dsincos_t(u * dx, sct, &sn, &cs);
                add_term_full(f, o, k, u, t_r1u2[k], t_ru[k], cst, sn, cs, t_rw[k], t_rb1[k],
                              t_rb2[k], t_rg[k], t_rr[k]);
            }
        }
        f = butterfly_full(f, kLanes);                             // every lane of the wave
        if (live && !cl && j == 0)
            write_planes_full(A, A.paired ? p : p * A.M + A.perm[m], f, o, 2.0 / ba0, disc, P.r,
                              P.q, T);
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
        dhgreeks::set_range(o, xK, a, b, exp(a), exp(b));
        const double ba = b - a;
        const double piba = dh::kPi / ba;
        const double dx = xK - a;
        SumsF f = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, 0.0, 0.0};
        const double cst = (lane & 1) ? o.c_odd : o.c_even;
        for (int k = lane; k < N; k += 64) {
            const double u = (double)k * piba;
            double rw, rb1, rb2, rg, rr, sn, cs;
            cf_eval_bt(CC, TC, u, T, a, sct, rw, rb1, rb2, rg, rr);
            dh::dsincos_t(u * dx, sct, &sn, &cs);
            const double wt = k == 0 ? 0.5 : 1.0;
            add_term_full(f, o, k, u, dh::drcp(fma(u, u, 1.0)), dh::drcp(k == 0 ? 1.0 : u), cst,
                          sn, cs, wt * rw, wt * rb1, wt * rb2, wt * rg, wt * rr);
        }
        f = butterfly_full(f, 64);
        if (lane == 0)
            write_planes_full(A, A.paired ? p : p * A.M + A.perm[m], f, o, 2.0 / ba, disc, P.r,
                              P.q, T);
    }
}

int launch_greeks_full(dh_ctx* ctx, GreekArgs A, int64_t P, hipStream_t st) {
    const size_t lds = greeks_full_lds_bytes(A.N);
    // past the default cap of a launch's dynamic LDS (N > 772): raised once per context, to the
    // largest N's size, as launch_greeks does for its kernel
    if (lds > 48 * 1024 && ctx->greeks_full_lds == 0) {
        const size_t most = greeks_full_lds_bytes(DH_MAX_N);
        HIP_TRY(hipFuncSetAttribute((const void*)greeks_full_kernel,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
        ctx->greeks_full_lds = (int)most;
    }
    const int64_t per = A.paired ? 1 : A.n_tiles;                  // blocks per param set
    const int64_t sets = std::max<int64_t>(1, dhgreeks::kMaxBlocks / per);
    for (int64_t p0 = 0; p0 < P; p0 += sets) {
        A.p0 = p0;
        const int64_t np = std::min(sets, P - p0);
        hipLaunchKernelGGL(greeks_full_kernel, dim3((unsigned)(np * per)), dim3(kBlock), lds, st,
                           A);
        HIP_TRY(hipGetLastError());
    }
    return DH_OK;
}

}  // namespace dhgfull

extern "C" int dh_surface_greeks_full_dev(dh_ctx* ctx, const dh_surface* s, const double* d_params,
                                          int64_t P, int N, double L, double* d_out,
                                          void* stream) {
    return dhgreeks::surface_dev(ctx, s, d_params, P, N, L, d_out, stream,
                                 dhgfull::launch_greeks_full);
}

extern "C" int dh_surface_greeks_full(dh_ctx* ctx, const dh_surface* s, const double* params,
                                      int64_t P, int N, double L, double* out) {
    return dhgreeks::surface_host(ctx, s, params, P, N, L, out, dhgfull::launch_greeks_full,
                                  DH_N_GREEKS_FULL);
}

extern "C" int dh_greeks_full_pairs(dh_ctx* ctx, const double* params, const double* K,
                                    const double* T, const int8_t* is_call, int64_t n, int N,
                                    double L, double* out) {
    return dhgreeks::pairs_host(ctx, params, K, T, is_call, n, N, L, out,
                                dhgfull::launch_greeks_full, DH_N_GREEKS_FULL);
}
