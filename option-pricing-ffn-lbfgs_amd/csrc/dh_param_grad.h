// dh_param_grad.h -- analytic sensitivities of the COS price to the thirteen model parameters, and
// the calibration loss with its exact gradient (dh_surface_param_sens*, dh_param_sens_pairs,
// dh_surface_loss_grad*, and against a market row per set dh_surface_loss_grad_rows*; DESIGN.md
// 3.18, 3.19).  Included by dh_kernels.hip after dh_greeks.h and ahead of the L-BFGS-B driver
// (dh_lb_driver.h); needs the kernels' helpers (xor_sum, option_logk), dh_kernels.hip's record
// arithmetic (x_records_kernel, feller_penalty, transform_dt, feller_kink_grad), dh_host.h,
// dh_iv_loss.h (DrainOnError) and dh_loss_rows.h (rows_grid, check_rows, check_spot_rate).
//
// The analytic rows request lives here too, once, for the three objectives that share it (the
// price objective below, dh_iv_grad.h's vol one, dh_gauss_newton.h's Gauss-Newton reduction):
// GradRows names a request's buffers, carve_grad_scratch alone knows the scratch layout,
// rows_request_dev is the _dev entry points' body and rows_round_trip the host entry points'.
//
// Definition.  In dh_greeks.h's notation (xK = log(K / S0), [a, b] = truncationRange(L), u_k =
// k pi / (b - a), w_k = phi(u_k) e^{-i u_k a}, price = e^{-rT} sum'_{k < N} Re(w_k) V_k), for a
// model parameter p at FIXED [a, b]
//     d price / d p = e^{-rT} sum'_{k < N} Re(w_k D_p(u_k)) V_k,   D_p = d log phi / d p,
// V_k and the halving of k = 0 unchanged.  Per factor (v0, kappa, theta, sigma, rho), with beta =
// kappa - i rho sigma u, uu = u (u + i), d = sqrt(beta^2 + sigma^2 uu), bm = beta - d, bp = beta + d,
// e = e^{-d tau}, D = bp - bm e, c = kappa theta / sigma^2, B = -uu (1 - e) / D, A = c (bm tau -
// 2 log(D / (2 d))) -- the quantities factor_x forms --
//     d/dv0 = B,    d/dtheta = (kappa / sigma^2) (bm tau - 2 log(D / (2 d)))
//     p in {kappa, sigma, rho}, from (beta', (d^2)', c'):
//         kappa (1, 2 beta, theta / sigma^2)
//         sigma (-i rho u, 2 beta (-i rho u) + 2 sigma uu, -2 kappa theta / sigma^3)
//         rho   (-i sigma u, 2 beta (-i sigma u), 0)
//       d' = (d^2)' / (2 d), bm' = beta' - d', bp' = beta' + d', e' = -tau d' e,
//       D' = bp' - bm' e - bm e', B' = -uu (-e' D - (1 - e) D') / D^2,
//       A' = c' (bm tau - 2 log(D / (2 d))) + c (bm' tau - 2 (D' / D - d' / d)),  d/dp = A' + B' v0
// and for the jumps, with J = e^{i u mu_j - sigma_j^2 u^2 / 2} and m = e^{mu_j + sigma_j^2 / 2},
//     d/dlambda = tau (J - 1) - i u tau (m - 1),   d/dmu_j = lambda tau i u J - i u tau lambda m,
//     d/dsigma_j = -lambda tau sigma_j u^2 J - i u tau lambda sigma_j m.
// Like the Greeks these do NOT differentiate through the cumulant range or its log-strike clamp.
// Planes: 0 the price, 1..13 the parameters in the record's order (v1_0 kappa1 theta1 sigma1 rho1
// v2_0 kappa2 theta2 sigma2 rho2 lambda_j mu_j sigma_j).
//
// No tail cut: every term k < N is summed.  1 <= N <= DH_PARAM_GRAD_MAX_N.
//
// param_grad_kernel, one block per (param set, tile of <= 256 options of one maturity), is the
// Greeks kernel's shape:
//   1. the block fills LDS with Re(w_k) and the thirteen Re(w_k D_p(u_k)) (halved at k = 0, where
//      the thirteen are exactly 0: phi(0) = 1) on the
//      tile's unclamped range [a0, b0], and with 1 / (1 + u_k^2) and 1 / u_k, one lane per term:
//      sixteen doubles per term, 128 KB at N = 1024;
//   2. every option whose own range is [a0, b0] runs one pass over k on kLanes lanes into fourteen
//      sums, then the xor butterfly over the kLanes lanes;
//   3. an option whose range the clamp widens takes the per-term way on its own [a, b], one wave per
//      option, lane l the terms l, l + 64, ... with their own CF and derivatives.
// Every sum is in an order fixed by (N, the option's path) alone: no atomics, the same bits in any
// call, for any tile size, any P, on any stream, surface or pairs.
//
// loss_grad_kernel reads the [14][S][M] planes a param_grad launch wrote (they are materialised in
// HBM: the reduction is a stage of its own, as dh_loss_rows.h's) and reduces, one wave per set,
//     f = sse / M + Feller,   g_i = (2 / M) sum_m ((p_m - mkt_m) / mkt_m^2) dp_m/dtheta_i
//                                   dtheta_i/dx_i + dFeller/dx_i
// in the optimiser's unconstrained x (dtheta/dx: theta for the exp-mapped parameters, 1 - rho^2 for
// the correlations, 1 for mu_j; the Feller term's derivative where its slack is strictly positive).
// A set with an invalid price (NaN, +-inf or <= 0) gets f = 1e10 and g = 0.
#pragma once

#include <initializer_list>

namespace dhpg {

using dh::cplx;

constexpr int kLanes = dhgreeks::kLanes;                   // lanes per option in the table pass
constexpr int kTabBytes = dhgreeks::kTabBytes;
constexpr int kPlanes = DH_N_PARAM_SENS;                   // the price and the thirteen parameters
constexpr int kTermArrays = kPlanes + 2;                   // and 1 / (1 + u^2), 1 / u
static_assert(kPlanes == 14, "record order: 13 model parameters");
static_assert(kLanes % 2 == 0 && kBlock % kLanes == 0, "a lane's terms share one parity");

// One factor's constants: factor_x's, and what the derivatives add.
struct GFactor {
    dh::FactorC F;
    double sig, rho;
    double kos;        // kappa / sigma^2: d/dtheta's coefficient
    double tos;        // theta / sigma^2: c' of kappa
    double csig;       // -2 kappa theta / sigma^3: c' of sigma
};

struct GConsts {
    dh::CfConsts C;
    GFactor g1, g2;
    double tau, lam_m;   // lam_m: lambda tau e^{mu_j + sigma_j^2 / 2}
    double tau_m1;       // tau (e^{mu_j + sigma_j^2 / 2} - 1)
    double sj;
};

__device__ __forceinline__ GFactor gfactor(const dh::FactorC& F, double th, double sig,
                                           double rho) {
    GFactor G;
    G.F = F;
    G.sig = sig;
    G.rho = rho;
    G.kos = F.kap * F.inv_s2;
    G.tos = th * F.inv_s2;
    G.csig = -2.0 * F.coef / sig;
    return G;
}

__device__ __forceinline__ GConsts gconsts(const Params& P, double tau) {
    GConsts G;
    G.C = dh::cf_consts(P, tau);
    G.g1 = gfactor(G.C.f1, P.t1, P.s1, P.r1);
    G.g2 = gfactor(G.C.f2, P.t2, P.s2, P.r2);
    const double m = exp(P.muj + 0.5 * (P.sj * P.sj));
    G.tau = tau;
    G.lam_m = G.C.lt * m;
    G.tau_m1 = tau * (m - 1.0);
    G.sj = P.sj;
    return G;
}

// the four derivatives of one factor's exponent that are not B itself
struct FactorD {
    cplx B, kap, th, sig, rho;
};

// factor_x_b (dh_greeks.h) with the derivatives handed out: the same expressions for X and B (the
// price and v0 planes agree with the Greeks kernel's to rounding; not bit for bit, the compiler
// contracts dh_device.h's functions per kernel), then the chain above from the quantities it has
// already formed.  1 / d = conj(d) / |d|^2 and 1 / D = conj(D) / |D|^2, each with one drcp.
__device__ __forceinline__ cplx factor_x_g(const GFactor& G, double u, double tau,
                                           const double2* __restrict__ sct, FactorD& out) {
    const dh::FactorC& F = G.F;
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
    const cplx inner = {bm.re * tau - lq2, bm.im * tau - 2.0 * aq};   // bm tau - 2 log(D / (2 d))

    out.B = B;
    out.th = dh::cscale(inner, G.kos);
    const double rD2 = dh::drcp(fma(D.re, D.re, D.im * D.im));
    const cplx invD = {D.re * rD2, -(D.im * rD2)};
    // 1 / (2 d) from a reciprocal of its own: rh, good enough inside factor_x's logarithm, is a
    // one-step rsqrt product (up to 193 ulp, DESIGN.md "The characteristic function"), and d' =
    // (d^2)' / (2 d) would carry that error into every kappa, sigma and rho plane
    const double rd2 = dh::drcp(fma(dre, dre, dim * dim));
    const cplx hinvd = {0.5 * dre * rd2, -(0.5 * dim * rd2)};
    const cplx invd = {2.0 * hinvd.re, 2.0 * hinvd.im};
    const cplx uu = {u * u, u};
    const cplx uD2 = dh::cmul(uu, dh::cmul(invD, invD));              // uu / D^2

    // d/dp from (beta', (d^2)', c'): beta' = (br, bi)
    auto chain = [&](double br, double bi, cplx d2q, double cq) -> cplx {
        const cplx dq = dh::cmul(d2q, hinvd);
        const cplx bmq = {br - dq.re, bi - dq.im};
        const cplx bpq = {br + dq.re, bi + dq.im};
        const cplx eq = dh::cscale(dh::cmul(dq, e), -tau);
        const cplx t1 = dh::cmul(bmq, e), t2 = dh::cmul(bm, eq);
        const cplx Dq = {bpq.re - t1.re - t2.re, bpq.im - t1.im - t2.im};
        const cplx n1 = dh::cmul(eq, D), n2 = dh::cmul(ome, Dq);
        const cplx Bq = dh::cmul(uD2, {n1.re + n2.re, n1.im + n2.im});
        const cplx r1 = dh::cmul(Dq, invD), r2 = dh::cmul(dq, invd);
        const cplx Aq = {cq * inner.re + F.coef * (bmq.re * tau - 2.0 * (r1.re - r2.re)),
                         cq * inner.im + F.coef * (bmq.im * tau - 2.0 * (r1.im - r2.im))};
        return {Aq.re + Bq.re * F.v0, Aq.im + Bq.im * F.v0};
    };
    out.kap = chain(1.0, 0.0, {2.0 * beta.re, 2.0 * beta.im}, G.tos);
    {
        const double bi = -(G.rho * u);                               // beta' = -i rho u
        const double ts = 2.0 * G.sig;
        out.sig = chain(0.0, bi, {-(2.0 * beta.im * bi) + ts * uu.re, 2.0 * beta.re * bi + ts * uu.im},
                        G.csig);
    }
    {
        const double bi = -(G.sig * u);                               // beta' = -i sigma u
        out.rho = chain(0.0, bi, {-(2.0 * beta.im * bi), 2.0 * beta.re * bi}, 0.0);
    }
    return {F.coef * (bm.re * tau - lq2) + B.re * F.v0,
            F.coef * (bm.im * tau - 2.0 * aq) + B.im * F.v0};
}

// cf_eval_b (dh_greeks.h) with all thirteen derivatives: t[0] = Re w, t[1 + i] = Re(w D_i) in the
// record's parameter order, w = phi(u) e^{-i u a} from the exponent's parts in cf_phase_from's
// order.
__device__ __forceinline__ void cf_eval_g(const GConsts& G, double u, double a,
                                          const double2* __restrict__ sct, double (&t)[kPlanes]) {
    FactorD d1, d2;
    const cplx X1 = factor_x_g(G.g1, u, G.tau, sct, d1);
    const cplx X2 = factor_x_g(G.g2, u, G.tau, sct, d2);
    // The exponent's jump part is dh::jump_x itself, as in cf_eval_b: that function is compiled
    // with FMA contraction (dh_device.h stands above dh_kernels.hip's contract(off) line), so its
    // expressions restated here, uncontracted, would round differently.  J is formed again for the
    // derivatives only.
    const cplx JX = dh::jump_x(G.C, u, sct);
    double js, jc;
    dh::dsincos_t(u * G.C.muj, sct, &js, &jc);
    const double jm = dh::dexp_t_nonpos(-(G.C.half_sj2 * (u * u)), sct);
    const cplx J = {jm * jc, jm * js};
    cplx E = {0.0, G.C.drift * u};
    E = dh::cadd(E, X1);
    E = dh::cadd(E, X2);
    E = dh::cadd(E, JX);
    double ps, pc;
    dh::dsincos_t(E.im - u * a, sct, &ps, &pc);
    const double m = dh::dexp_t(E.re, sct);
    const double wr = m * pc, wi = m * ps;
    const double ltu = G.C.lt * u;
    const double su = G.sj * u;
    const cplx dlam = {G.tau * (J.re - 1.0), G.tau * J.im - u * G.tau_m1};
    const cplx dmu = {-(ltu * J.im), ltu * J.re - u * G.lam_m};
    const cplx dsj = {-(ltu * su * J.re), -(ltu * su * J.im) - su * G.lam_m};
    const cplx Dv[kPlanes - 1] = {d1.B, d1.kap, d1.th, d1.sig, d1.rho, d2.B, d2.kap, d2.th, d2.sig,
                                  d2.rho, dlam, dmu, dsj};
    t[0] = wr;
    // phi(0) = 1 whatever the parameters, so every D_p(0) is exactly 0.  Formed in fp64 it is a
    // residue of the primitives' roundings instead (bm = kappa - sqrt(kappa^2), log(|D|^2 / 4 |d|^2)
    // at 1: up to 1e-15 times c' on the sigma plane), which at N = 1 is the whole plane.  Term 0
    // (u == 0 only there) carries the exact value.
    const bool k0 = u == 0.0;
#pragma unroll
    for (int i = 0; i < kPlanes - 1; ++i) t[1 + i] = k0 ? 0.0 : wr * Dv[i].re - wi * Dv[i].im;
}

struct GradArgs {
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
    double* out;            // [kPlanes][plane]
    int64_t plane;          // P * M (surface) or P (paired)
};

// what a pass needs of its option and range (dh_greeks.h's OptC without the spot Greeks' parts)
struct OptC {
    double S0, K, exk;
    double c_even, c_odd, sgn, psi0;
    bool call;
};

__device__ __forceinline__ void set_range(OptC& o, double xK, double a, double b, double ea,
                                          double eb) {
    o.c_even = o.call ? eb : -ea;
    o.c_odd = o.call ? -eb : -ea;
    o.sgn = o.call ? -1.0 : 1.0;
    o.psi0 = o.call ? b - xK : xK - a;
}

// V_k without its +-(2 / (b - a)): dh_greeks.h's add_term expressions
__device__ __forceinline__ double term_v(const OptC& o, int k, double u, double r1u2, double ru,
                                         double cst, double sn, double cs) {
    const double ex = o.exk * fma(u, sn, cs);
    const double chi = fma(o.sgn, ex, cst) * r1u2;
    const double psi = k == 0 ? o.psi0 : (o.sgn * sn) * ru;
    return fma(o.S0, chi, -(o.K * psi));
}

__device__ __forceinline__ void write_planes(const GradArgs& A, int64_t at, const double (&s)[kPlanes],
                                             const OptC& o, double scale, double disc) {
    const double c = disc * (o.call ? scale : -scale);       // e^{-rT} (+-) 2 / (b - a)
#pragma unroll
    for (int i = 0; i < kPlanes; ++i) A.out[i * A.plane + at] = c * s[i];
}

// dynamic LDS: the CF's math tables, then the sixteen per-term arrays [N rounded up to even] each,
// then one clamp flag per option of the tile
inline size_t lds_bytes(int N) {
    return (size_t)kTabBytes + kTermArrays * (size_t)((N + 1) & ~1) * sizeof(double) + kTileMax;
}
static_assert(kTabBytes + kTermArrays * DH_PARAM_GRAD_MAX_N * 8 + kTileMax <= 160 * 1024,
              "the table of the longest series fits one CU's LDS");

// 2 waves per SIMD (<= 256 VGPRs): the term lane holds thirteen complex derivatives at once
__global__ __launch_bounds__(kBlock, 2) void param_grad_kernel(GradArgs A) {
    extern __shared__ __attribute__((aligned(16))) char pg_smem[];
    double2* sct = (double2*)pg_smem;
    const int N = A.N, Np = (N + 1) & ~1;
    double* tab = (double*)(pg_smem + kTabBytes);            // tab[i * Np + k], i < kPlanes
    double* t_r1u2 = tab + kPlanes * Np;
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
    const GConsts G = gconsts(P, T);
    const double disc = exp(-P.r * T);
    __syncthreads();

    // 1. the tile's table on [a0, b0]
    const double ba0 = b0 - a0;
    const double piba0 = dh::kPi / ba0;
    for (int k = tid; k < N; k += kBlock) {
        const double u = (double)k * piba0;
        double t[kPlanes];
        cf_eval_g(G, u, a0, sct, t);
        const double wt = k == 0 ? 0.5 : 1.0;
#pragma unroll
        for (int i = 0; i < kPlanes; ++i) tab[i * Np + k] = wt * t[i];
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
        double s[kPlanes];
#pragma unroll
        for (int i = 0; i < kPlanes; ++i) s[i] = 0.0;
        if (live && !cl) {
            const double dx = xK - a0;
            const double cst = (j & 1) ? o.c_odd : o.c_even;      // kLanes is even: k's parity is j's
            for (int k = j; k < N; k += kLanes) {
                const double u = (double)k * piba0;
                double sn, cs;
                dh::dsincos_t(u * dx, sct, &sn, &cs);
                const double v = term_v(o, k, u, t_r1u2[k], t_ru[k], cst, sn, cs);
#pragma unroll
                for (int i = 0; i < kPlanes; ++i) s[i] = fma(tab[i * Np + k], v, s[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < kPlanes; ++i) s[i] = xor_sum(s[i], kLanes);   // every lane of the wave
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
        double s[kPlanes];
#pragma unroll
        for (int i = 0; i < kPlanes; ++i) s[i] = 0.0;
        const double cst = (lane & 1) ? o.c_odd : o.c_even;
        for (int k = lane; k < N; k += 64) {
            const double u = (double)k * piba;
            double tt[kPlanes], sn, cs;
            cf_eval_g(G, u, a, sct, tt);
            dh::dsincos_t(u * dx, sct, &sn, &cs);
            const double wt = k == 0 ? 0.5 : 1.0;
            const double v = wt * term_v(o, k, u, dh::drcp(fma(u, u, 1.0)),
                                         dh::drcp(k == 0 ? 1.0 : u), cst, sn, cs);
#pragma unroll
            for (int i = 0; i < kPlanes; ++i) s[i] = fma(tt[i], v, s[i]);
        }
#pragma unroll
        for (int i = 0; i < kPlanes; ++i) s[i] = xor_sum(s[i], 64);
        if (lane == 0)
            write_planes(A, A.paired ? p : p * A.M + A.perm[m], s, o, 2.0 / ba, disc);
    }
}

constexpr int64_t kMaxBlocks = int64_t(1) << 30;

int launch_param_grad(dh_ctx* ctx, GradArgs A, int64_t P, hipStream_t st) {
    const size_t lds = lds_bytes(A.N);
    // past the default cap of a launch's dynamic LDS: raised once per context, to the largest N's
    // size, so that later requests make no runtime call but their launch
    if (lds > 48 * 1024 && ctx->param_grad_lds == 0) {
        const size_t most = lds_bytes(DH_PARAM_GRAD_MAX_N);
        HIP_TRY(hipFuncSetAttribute((const void*)param_grad_kernel,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
        ctx->param_grad_lds = (int)most;
    }
    const int64_t per = A.paired ? 1 : A.n_tiles;                  // blocks per param set
    const int64_t sets = std::max<int64_t>(1, kMaxBlocks / per);   // param sets per launch
    for (int64_t p0 = 0; p0 < P; p0 += sets) {
        A.p0 = p0;
        const int64_t np = std::min(sets, P - p0);
        hipLaunchKernelGGL(param_grad_kernel, dim3((unsigned)(np * per)), dim3(kBlock), lds, st, A);
        HIP_TRY(hipGetLastError());
    }
    return DH_OK;
}

GradArgs surface_args(const dh_surface* s, const double* d_params, int64_t P, int N, double L,
                      double* d_out) {
    GradArgs A{};
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
    return A;
}

// the checks every entry point makes before any device work; `count` names P, n or S
int check_args(const dh_ctx* ctx, int64_t count, const char* count_name, int N, double L) {
    if (!ctx) return fail(DH_E_ARG, "ctx is null");
    if (N < 1 || N > DH_PARAM_GRAD_MAX_N)
        return fail(DH_E_ARG, "N must be in [1, " + std::to_string(DH_PARAM_GRAD_MAX_N) +
                                  "], got " + std::to_string(N));
    if (count < 1)
        return fail(DH_E_ARG, std::string(count_name) + " must be >= 1, got " +
                                  std::to_string(count));
    if (!std::isfinite(L) || !(L > 0.0)) return fail(DH_E_ARG, "L must be finite and > 0");
    return DH_OK;
}

// ---- the loss and its gradient from the planes --------------------------------------------------
// Summation order.  One wave per set.  Lane l starts its fourteen sums from 0.0 and adds the terms
// of the surface's *sorted* options l, l + 64, ... in that order (planes read at the option's place
// in the caller's order, perm[m]); then the xor butterfly over the 64 lanes.  Nothing is contracted.
// The order is a function of M and the surface's option sort alone.

// mkt: the set's market prices, in the surface's sorted order (kCaller false: the surface's own)
// or in the caller's option order (kCaller true: a market row, read at perm[m]).
template <bool kCaller>
__device__ __forceinline__ void loss_grad_wave(
    const double* __restrict__ planes, const double* __restrict__ rec,
    const double* __restrict__ pen, const double* __restrict__ mkt, const int* __restrict__ perm,
    int M, int64_t S, int64_t s, int lane, double* __restrict__ f, double* __restrict__ g,
    int* __restrict__ n_bad) {
    const int64_t plane = S * (int64_t)M;
    const double* p = planes + s * M;
    double acc = 0.0, gs[kPlanes - 1];
#pragma unroll
    for (int i = 0; i < kPlanes - 1; ++i) gs[i] = 0.0;
    int bad = 0;
    for (int m0 = 0; m0 < M; m0 += 64) {             // every lane makes every pass
        const int m = m0 + lane;
        if (m < M) {
            const int c = perm[m];
            const double pr = p[c], mm = mkt[kCaller ? c : m];
            const double rel = (pr - mm) / mm;
            acc = acc + rel * rel;
            bad += (pr != pr || isinf(pr) || pr <= 0.0) ? 1 : 0;
            const double w = rel / mm;               // (p - mkt) / mkt^2
#pragma unroll
            for (int i = 0; i < kPlanes - 1; ++i) gs[i] = gs[i] + w * p[(i + 1) * plane + c];
        }
    }
    acc = xor_sum(acc, 64);
#pragma unroll
    for (int i = 0; i < kPlanes - 1; ++i) gs[i] = xor_sum(gs[i], 64);
    for (int off = 1; off < 64; off <<= 1) bad += __shfl_xor(bad, off, 64);
    if (lane != 0) return;
    n_bad[s] = bad;
    double* go = g + s * (kPlanes - 1);
    if (bad > 0) {                                   // the FD quotient of a constant 1e10
        f[s] = kInvalidLoss;
#pragma unroll
        for (int i = 0; i < kPlanes - 1; ++i) go[i] = 0.0;
        return;
    }
    const double* q = rec + s * DH_PARAM_STRIDE;
    f[s] = acc / (double)M + pen[s];
    const double c2 = 2.0 / (double)M;
#pragma unroll
    for (int i = 0; i < kPlanes - 1; ++i) {
        const double dt = transform_dt(i, q);
        go[i] = c2 * gs[i] * dt;
    }
    feller_kink_grad(q, go);
}

__global__ __launch_bounds__(kBlockRows) void loss_grad_kernel(
    const double* __restrict__ planes, const double* __restrict__ rec,
    const double* __restrict__ pen, const double* __restrict__ mkt, const int* __restrict__ perm,
    int M, int64_t S, double* __restrict__ f, double* __restrict__ g, int* __restrict__ n_bad) {
    const int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (s >= S) return;                              // whole waves: s is uniform across a wave
    loss_grad_wave<false>(planes, rec, pen, mkt, perm, M, S, s, lane, f, g, n_bad);
}

// ---- the same against a market row per set (dh_surface_loss_grad_rows*, the analytic batch
// driver's reduction) ---------------------------------------------------------------
// x_records_kernel (dh_kernels.hip) with each set's spot and rate taken from its market row: the
// same x_record, so the same records and penalties for the same inputs.
__global__ void x_records_rows_kernel(const double* __restrict__ x, int S,
                                      const double* __restrict__ spot,
                                      const double* __restrict__ rate, const int* __restrict__ row,
                                      double* __restrict__ rec, double* __restrict__ pen) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    double p[dhlb::kN];
#pragma unroll
    for (int i = 0; i < dhlb::kN; ++i) p[i] = lb_transform(i, x[(size_t)s * dhlb::kN + i]);
    pen[s] = feller_penalty(p);
    double* out = rec + (size_t)s * DH_PARAM_STRIDE;
#pragma unroll
    for (int i = 0; i < dhlb::kN; ++i) out[i] = p[i];
    const int b = row[s];
    out[13] = spot[b];
    out[14] = rate[b];
    out[15] = 0.0;
}

// loss_grad_kernel's wave against row[s] of mkt [B][M] (the caller's option order): the same sums
// in the same order, so with B = 1 and the surface's own market prices the same bits.  live_count:
// the device-resident driver's count of unfinished starts (the launch is a no-op at 0), or null.
__global__ __launch_bounds__(kBlockRows) void loss_grad_rows_kernel(
    const double* __restrict__ planes, const double* __restrict__ rec,
    const double* __restrict__ pen, const double* __restrict__ mkt, const int* __restrict__ row,
    const int* __restrict__ perm, int M, int64_t S, const int* __restrict__ live_count,
    double* __restrict__ f, double* __restrict__ g, int* __restrict__ n_bad) {
    if (live_count && __builtin_amdgcn_readfirstlane(*live_count) <= 0) return;
    const int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (s >= S) return;                              // whole waves: s is uniform across a wave
    loss_grad_wave<true>(planes, rec, pen, mkt + (int64_t)row[s] * M, perm, M, S, s, lane, f, g,
                         n_bad);
}

// ---- one analytic rows request: its buffers ---------------------------------------------------------
// All device memory.  The three objectives' launches (loss_grad_rows_launch here,
// dhivg::loss_iv_grad_rows_launch, dhgn::gauss_newton_rows_launch) read what they need of it.
struct GradRows {
    const double *rec, *pen; // scratch (carve_grad_scratch): records [S][16], Feller penalties [S],
    double *planes, *extra;  // planes [14][S][M], then the vol c_m plane [S][M] or H [S][13][13]
    const double *mkt, *wgt; // the markets [B][M]: prices or vols, and the vol objective's weights
    const int* row;          // [S] each set's market
    const double* div;       // the vol objective's loss divisor: [S], or with div_by_row [B] read
    bool div_by_row;         // at row[s] (the driver's form: its sets move between slots)
    double *f, *g, *sse;     // results: [S], [S][13], and [S] or null (the vol reduction alone)
    int* bad;                // [S]
    double* iv;              // [S][M] the vols as used, or null
    int S;
    const int* live_count;   // the device-resident driver's count of unfinished starts, or null
};

enum class Scratch { kPrice, kVol, kHess };     // what follows the planes: nothing, c_m, Hessians

// scratch of a request in the context's buffer: records [S][16], penalties [S], planes [14][S][M],
// then the kind's extra
size_t grad_scratch_bytes(int S, int M, Scratch kind) {
    const size_t extra = kind == Scratch::kVol    ? (size_t)S * M
                         : kind == Scratch::kHess ? (size_t)S * (kPlanes - 1) * (kPlanes - 1)
                                                  : 0;
    return ((size_t)S * (DH_PARAM_STRIDE + 1) + (size_t)kPlanes * S * M + extra) * 8;
}

// the one place that knows that layout (extra: valid where grad_scratch_bytes counted one)
struct GradScratch {
    double *rec, *pen, *planes, *extra;
};
GradScratch carve_grad_scratch(void* ptr, int S, int M) {
    GradScratch c;
    c.rec = (double*)ptr;
    c.pen = c.rec + (size_t)S * DH_PARAM_STRIDE;
    c.planes = c.pen + S;
    c.extra = c.planes + (size_t)kPlanes * S * M;
    return c;
}

// stages 2 and 3 of a request over records already on the device
using RowsLaunch = int (*)(dh_ctx*, const dh_surface*, const GradRows&, int N, double L,
                           hipStream_t);

// param_grad_kernel into the planes, then the rows reduction.  The analytic batch driver's
// iteration.
int loss_grad_rows_launch(dh_ctx* ctx, const dh_surface* s, const GradRows& R, int N, double L,
                          hipStream_t st) {
    const int rc = launch_param_grad(ctx, surface_args(s, R.rec, R.S, N, L, R.planes), R.S, st);
    if (rc) return rc;
    hipLaunchKernelGGL(loss_grad_rows_kernel, dim3(rows_grid(R.S)), dim3(kBlockRows), 0, st,
                       (const double*)R.planes, R.rec, R.pen, R.mkt, R.row, (const int*)s->perm,
                       s->M, (int64_t)R.S, R.live_count, R.f, R.g, R.bad);
    HIP_TRY(hipGetLastError());
    return DH_OK;
}

int check_loss_grad(const dh_ctx* ctx, const dh_surface* s, int S, double S0, double r, int N,
                    double L) {
    int rc = check_args(ctx, S, "S", N, L);
    if (rc) return rc;
    if (!s) return fail(DH_E_ARG, "surface is null");
    if (s->M == 0) return fail(DH_E_ARG, "surface is empty (the loss is NaN)");
    if (!s->has_mkt) return fail(DH_E_ARG, "surface has no market prices");
    if (!std::isfinite(S0) || !(S0 > 0.0)) return fail(DH_E_ARG, "S0 must be finite and > 0");
    if (!std::isfinite(r)) return fail(DH_E_ARG, "r must be finite");
    return DH_OK;
}

// the rows forms: the surface needs no market prices of its own
int check_loss_grad_rows(const dh_ctx* ctx, const dh_surface* s, int S, int N, double L) {
    int rc = check_args(ctx, S, "S", N, L);
    if (rc) return rc;
    if (!s) return fail(DH_E_ARG, "surface is null");
    if (s->M == 0) return fail(DH_E_ARG, "surface is empty (the loss is NaN)");
    return DH_OK;
}

// ---- one analytic rows request: its entry points ----------------------------------------------------
// the pointers an entry point needs, in its order: the first null one fails with "<name> is null"
struct NamedPtr {
    const void* p;
    const char* name;
};
int check_not_null(std::initializer_list<NamedPtr> need) {
    for (const NamedPtr& a : need)
        if (!a.p) return fail(DH_E_ARG, std::string(a.name) + " is null");
    return DH_OK;
}

// The _dev entry points' body: the checks, then x [S][13] -> records and penalties in the
// context's scratch (each set's spot and rate from its market row), then `launch`.  R brings the
// markets and results; its scratch pointers are set here (extra only where the caller gave none).
int rows_request_dev(dh_ctx* ctx, const dh_surface* s, std::initializer_list<NamedPtr> need,
                     const double* d_x, const double* d_spot, const double* d_rate, GradRows R,
                     Scratch kind, RowsLaunch launch, int N, double L, void* stream) {
    int rc = check_loss_grad_rows(ctx, s, R.S, N, L);
    if (rc) return rc;
    rc = check_not_null(need);
    if (rc) return rc;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    // grow-only: a request no larger than an earlier one on this context allocates nothing
    HIP_TRY(ctx->pg_scratch.reserve(grad_scratch_bytes(R.S, s->M, kind)));
    const GradScratch c = carve_grad_scratch(ctx->pg_scratch.ptr, R.S, s->M);
    R.rec = c.rec, R.pen = c.pen, R.planes = c.planes;
    if (!R.extra) R.extra = c.extra;
    hipLaunchKernelGGL(x_records_rows_kernel, dim3((unsigned)((R.S + 255) / 256)), dim3(256), 0, st,
                       d_x, R.S, d_spot, d_rate, R.row, c.rec, c.pen);
    HIP_TRY(hipGetLastError());
    return launch(ctx, s, R, N, L, st);
}

// An entry point's arrays, the host's or as rows_round_trip staged them on the device: x [S][13],
// mkt [B][M] (prices, or vols), spot [B], rate [B], row [S] in; f [S], g [S][13], bad [S] and the
// objective's extra (the vols as used [S][M] or null, or H [S][13][13]) out.  wgt [B][M] and div
// [S] are what `prep` made, on the device only (null without).
struct RowsIo {
    const double *x, *mkt, *wgt, *div, *spot, *rate;
    const int32_t* row;
    double *f, *g;
    int32_t* bad;
    double* extra;
};

// The host entry points' round trip: the checks in the order below, the objective's own host
// preparation (`prep(w, dv)` fills the weights [B][M] and divisors [S] it wants uploaded, or leaves
// them empty), the uploads, the _dev form (`dev`), the downloads, synchronise.  w and dv are
// pageable and declared ahead of the guard: every error return drains the stream before they go.
template <typename Prep, typename Dev>
int rows_round_trip(dh_ctx* ctx, const dh_surface* s, std::initializer_list<NamedPtr> need,
                    const RowsIo& h, int S, int B, size_t n_extra, int N, double L, Prep&& prep,
                    Dev&& dev) {
    int rc = check_loss_grad_rows(ctx, s, S, N, L);
    if (rc) return rc;
    rc = check_not_null(need);
    if (rc) return rc;
    rc = check_rows(h.row, S, B);
    if (rc) return rc;
    rc = check_spot_rate(h.spot, h.rate, B);
    if (rc) return rc;
    std::vector<double> w, dv;
    rc = prep(w, dv);
    if (rc) return rc;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    constexpr int kN = kPlanes - 1;
    const size_t xb = (size_t)S * kN * 8, mb = (size_t)B * s->M * 8, ne = h.extra ? n_extra : 0;
    hipStream_t st = ctx->stream;
    DrainOnError drain{st};
    // x [S][13], then f [S], g [S][13], div [S], spot [B], rate [B], extra [ne], bad [S] (int32)
    HIP_TRY(ctx->pg_io.reserve(2 * xb + (size_t)S * 20 + (size_t)B * 16 + ne * 8));
    HIP_TRY(ctx->rows_mkt.reserve(mb));
    if (!w.empty()) HIP_TRY(ctx->rows_wgt.reserve(mb));
    HIP_TRY(ctx->rows_row.reserve((size_t)S * 4));
    double* d_x = (double*)ctx->pg_io.ptr;
    double* d_f = d_x + (size_t)S * kN;
    double* d_g = d_f + S;
    double* d_div = d_g + (size_t)S * kN;
    double* d_spot = d_div + S;
    double* d_rate = d_spot + B;
    double* d_extra = d_rate + B;
    int32_t* d_bad = (int32_t*)(d_extra + ne);
    HIP_TRY(hipMemcpyAsync(d_x, h.x, xb, hipMemcpyHostToDevice, st));
    if (!dv.empty())
        HIP_TRY(hipMemcpyAsync(d_div, dv.data(), (size_t)S * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_spot, h.spot, (size_t)B * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_rate, h.rate, (size_t)B * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->rows_mkt.ptr, h.mkt, mb, hipMemcpyHostToDevice, st));
    if (!w.empty())
        HIP_TRY(hipMemcpyAsync(ctx->rows_wgt.ptr, w.data(), mb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->rows_row.ptr, h.row, (size_t)S * 4, hipMemcpyHostToDevice, st));
    rc = dev(RowsIo{d_x, (const double*)ctx->rows_mkt.ptr,
                    w.empty() ? nullptr : (const double*)ctx->rows_wgt.ptr,
                    dv.empty() ? nullptr : d_div, d_spot, d_rate, (const int32_t*)ctx->rows_row.ptr,
                    d_f, d_g, d_bad, ne ? d_extra : nullptr},
             st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(h.f, d_f, (size_t)S * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h.g, d_g, xb, hipMemcpyDeviceToHost, st));
    if (ne) HIP_TRY(hipMemcpyAsync(h.extra, d_extra, ne * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h.bad, d_bad, (size_t)S * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    drain.armed = false;
    return DH_OK;
}

// the price and Gauss-Newton objectives prepare nothing on the host
inline int no_prep(std::vector<double>&, std::vector<double>&) { return DH_OK; }

}  // namespace dhpg

extern "C" int dh_surface_param_sens_dev(dh_ctx* ctx, const dh_surface* s, const double* d_params,
                                         int64_t P, int N, double L, double* d_out, void* stream) {
    int rc = dhpg::check_args(ctx, P, "P", N, L);
    if (rc) return rc;
    if (!s) return fail(DH_E_ARG, "surface is null");
    if (!d_params) return fail(DH_E_ARG, "params is null");
    if (!d_out) return fail(DH_E_ARG, "out is null");
    if (s->M == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    return dhpg::launch_param_grad(ctx, dhpg::surface_args(s, d_params, P, N, L, d_out), P,
                                   stream ? (hipStream_t)stream : ctx->stream);
}

extern "C" int dh_surface_param_sens(dh_ctx* ctx, const dh_surface* s, const double* params,
                                     int64_t P, int N, double L, double* out) {
    int rc = dhpg::check_args(ctx, P, "P", N, L);
    if (rc) return rc;
    if (!s) return fail(DH_E_ARG, "surface is null");
    if (!params) return fail(DH_E_ARG, "params is null");
    if (!out) return fail(DH_E_ARG, "out is null");
    if (s->M == 0) return DH_OK;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const size_t pb = (size_t)P * DH_PARAM_STRIDE * 8, ob = (size_t)dhpg::kPlanes * P * s->M * 8;
    HIP_TRY(ctx->params.reserve(pb));
    HIP_TRY(ctx->out.reserve(ob));
    HIP_TRY(hipMemcpyAsync(ctx->params.ptr, params, pb, hipMemcpyHostToDevice, ctx->stream));
    rc = dh_surface_param_sens_dev(ctx, s, (const double*)ctx->params.ptr, P, N, L,
                                   (double*)ctx->out.ptr, ctx->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, ctx->out.ptr, ob, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DH_OK;
}

extern "C" int dh_param_sens_pairs(dh_ctx* ctx, const double* params, const double* K,
                                   const double* T, const int8_t* is_call, int64_t n, int N,
                                   double L, double* out) {
    int rc = dhpg::check_args(ctx, n, "n", N, L);
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
    HIP_TRY(ctx->out.reserve(dhpg::kPlanes * vb));
    HIP_TRY(ctx->aux0.reserve(vb));
    HIP_TRY(ctx->aux1.reserve(vb));
    HIP_TRY(ctx->aux2.reserve((size_t)n));
    HIP_TRY(hipMemcpyAsync(ctx->params.ptr, params, pb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->aux0.ptr, K, vb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->aux1.ptr, T, vb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->aux2.ptr, is_call, (size_t)n, hipMemcpyHostToDevice, st));
    dhpg::GradArgs A{};
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
    rc = dhpg::launch_param_grad(ctx, A, n, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, ctx->out.ptr, dhpg::kPlanes * vb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}

extern "C" int dh_surface_loss_grad_dev(dh_ctx* ctx, const dh_surface* s, const double* d_x, int S,
                                        double S0, double r, int N, double L, double* d_f,
                                        double* d_g, int32_t* d_bad, void* stream) {
    int rc = dhpg::check_loss_grad(ctx, s, S, S0, r, N, L);
    if (rc) return rc;
    if (!d_x) return fail(DH_E_ARG, "x is null");
    if (!d_f) return fail(DH_E_ARG, "f is null");
    if (!d_g) return fail(DH_E_ARG, "g is null");
    if (!d_bad) return fail(DH_E_ARG, "bad is null");
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    // grow-only: a request no larger than an earlier one on this context allocates nothing
    HIP_TRY(ctx->pg_scratch.reserve(dhpg::grad_scratch_bytes(S, s->M, dhpg::Scratch::kPrice)));
    const dhpg::GradScratch R = dhpg::carve_grad_scratch(ctx->pg_scratch.ptr, S, s->M);
    hipLaunchKernelGGL(x_records_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, d_x,
                       S, S0, r, R.rec, R.pen);
    HIP_TRY(hipGetLastError());
    rc = dhpg::launch_param_grad(ctx, dhpg::surface_args(s, R.rec, S, N, L, R.planes), S, st);
    if (rc) return rc;
    hipLaunchKernelGGL(dhpg::loss_grad_kernel, dim3(rows_grid(S)), dim3(kBlockRows), 0, st,
                       (const double*)R.planes, (const double*)R.rec, (const double*)R.pen,
                       (const double*)s->mkt, (const int*)s->perm, s->M, (int64_t)S, d_f, d_g,
                       (int*)d_bad);
    HIP_TRY(hipGetLastError());
    return DH_OK;
}

extern "C" int dh_surface_loss_grad(dh_ctx* ctx, const dh_surface* s, const double* x, int S,
                                    double S0, double r, int N, double L, double* f, double* g,
                                    int32_t* bad) {
    int rc = dhpg::check_loss_grad(ctx, s, S, S0, r, N, L);
    if (rc) return rc;
    if (!x) return fail(DH_E_ARG, "x is null");
    if (!f) return fail(DH_E_ARG, "f is null");
    if (!g) return fail(DH_E_ARG, "g is null");
    if (!bad) return fail(DH_E_ARG, "bad is null");
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    constexpr int kN = dhpg::kPlanes - 1;
    const size_t xb = (size_t)S * kN * 8;
    hipStream_t st = ctx->stream;
    // x [S][13], then f [S], g [S][13], bad [S]
    HIP_TRY(ctx->pg_io.reserve(2 * xb + (size_t)S * 16));
    double* d_x = (double*)ctx->pg_io.ptr;
    double* d_f = d_x + (size_t)S * kN;
    double* d_g = d_f + S;
    int32_t* d_bad = (int32_t*)(d_g + (size_t)S * kN);
    HIP_TRY(hipMemcpyAsync(d_x, x, xb, hipMemcpyHostToDevice, st));
    rc = dh_surface_loss_grad_dev(ctx, s, d_x, S, S0, r, N, L, d_f, d_g, d_bad, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(f, d_f, (size_t)S * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(g, d_g, xb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(bad, d_bad, (size_t)S * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}

extern "C" int dh_surface_loss_grad_rows_dev(dh_ctx* ctx, const dh_surface* s, const double* d_x,
                                             const double* d_mkt, const double* d_spot,
                                             const double* d_rate, const int32_t* d_row, int S,
                                             int N, double L, double* d_f, double* d_g,
                                             int32_t* d_bad, void* stream) {
    dhpg::GradRows R{};
    R.mkt = d_mkt;
    R.row = (const int*)d_row;
    R.f = d_f;
    R.g = d_g;
    R.bad = (int*)d_bad;
    R.S = S;
    return dhpg::rows_request_dev(ctx, s,
                                  {{d_x, "x"}, {d_mkt, "mkt"}, {d_spot, "spot"}, {d_rate, "rate"},
                                   {d_row, "row"}, {d_f, "f"}, {d_g, "g"}, {d_bad, "bad"}},
                                  d_x, d_spot, d_rate, R, dhpg::Scratch::kPrice,
                                  dhpg::loss_grad_rows_launch, N, L, stream);
}

extern "C" int dh_surface_loss_grad_rows(dh_ctx* ctx, const dh_surface* s, const double* x,
                                         const double* mkt, const double* spot,
                                         const double* rate, const int32_t* row, int S, int B,
                                         int N, double L, double* f, double* g, int32_t* bad) {
    return dhpg::rows_round_trip(
        ctx, s,
        {{x, "x"}, {mkt, "mkt"}, {spot, "spot"}, {rate, "rate"}, {row, "row"}, {f, "f"}, {g, "g"},
         {bad, "bad"}},
        dhpg::RowsIo{x, mkt, nullptr, nullptr, spot, rate, row, f, g, bad, nullptr}, S, B, 0, N, L,
        dhpg::no_prep, [&](const dhpg::RowsIo& d, hipStream_t st) {
            return dh_surface_loss_grad_rows_dev(ctx, s, d.x, d.mkt, d.spot, d.rate, d.row, S, N,
                                                 L, d.f, d.g, d.bad, st);
        });
}
