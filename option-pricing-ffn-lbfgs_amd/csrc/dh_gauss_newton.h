// dh_gauss_newton.h -- the Gauss-Newton rows reduction (dh_surface_gauss_newton_rows*; DESIGN.md
// 3.21): from the [14][S][M] planes of param_grad_kernel and the records and penalties of
// x_records_rows_kernel, per set s against its market row,
//     f, g, n_bad   dh_surface_loss_grad_rows's, bit for bit, and
//     H_ij = (2 / M) dt_i dt_j sum_m a_im a_jm,   a_im = plane_i[m] / mkt_m,
// the Gauss-Newton Hessian of the price part of the loss in the optimiser's x (dt: the transform's
// derivative, dh_kernels.hip's transform_dt).  The Feller penalty enters g only.  Included by
// dh_kernels.hip after dh_param_grad.h and ahead of dh_lb_driver.h, whose Levenberg-Marquardt
// iteration launches it; needs dh_param_grad.h: loss_grad_wave, launch_param_grad and the analytic
// rows request (GradRows, rows_request_dev, rows_round_trip), which carry everything here but the
// kernel and its launch.
//
// Shape.  One block of five waves per set.  Wave 0 IS loss_grad_wave<true>: the same function, so
// the same f, g and n_bad.  Waves 1..4 own entries 23 (w - 1) .. 23 w - 1 of the 91 upper entries
// (row-major over i <= j; the last wave owns 22), 23 accumulators a lane, and each counts the set's
// invalid prices for itself, so no wave waits for another: there is no barrier and no LDS.  Every
// wave reads the same thirteen plane values of an option, from L2 after the first.  105 sums in one
// wave would be 210 accumulator registers a lane.
//
// Order.  Every entry's sum is loss_grad_wave's: lane l starts from 0.0 and adds the surface's
// sorted options l, l + 64, ... in that order, then the xor butterfly over the 64 lanes.  Nothing
// is contracted, there are no atomics, and the order is a function of M and the option sort alone:
// a set's bits depend neither on S nor on the set's place in the call.  The 91 upper entries are
// computed and mirrored, so H is exactly symmetric.
#pragma once

#include <utility>

namespace dhgn {

constexpr int kN = dhpg::kPlanes - 1;                 // 13 parameters
constexpr int kUpper = kN * (kN + 1) / 2;             // 91 entries i <= j
constexpr int kHWaves = 4;                            // waves that own entries
constexpr int kPerWave = (kUpper + kHWaves - 1) / kHWaves;   // 23
constexpr int kBlock = 64 * (1 + kHWaves);

// entry e of the upper triangle, row-major: (0,0) (0,1) .. (0,12) (1,1) ..
constexpr int entry_row(int e) {
    int i = 0;
    while (e >= kN - i) {
        e -= kN - i;
        ++i;
    }
    return i;
}
constexpr int entry_col(int e) {
    int i = 0;
    while (e >= kN - i) {
        e -= kN - i;
        ++i;
    }
    return i + e;
}
template <int E>
inline constexpr int kRow = entry_row(E);      // constants at every use: the arrays stay in registers
template <int E>
inline constexpr int kCol = entry_col(E);
static_assert(entry_row(0) == 0 && entry_col(12) == 12 && entry_row(13) == 1 && entry_col(13) == 1 &&
                  entry_row(kUpper - 1) == kN - 1 && entry_col(kUpper - 1) == kN - 1,
              "upper-triangle numbering");

template <int E0, int... K>
__device__ __forceinline__ void add_products(double (&acc)[sizeof...(K)], const double (&a)[kN],
                                             std::integer_sequence<int, K...>) {
    ((acc[K] = acc[K] + a[kRow<E0 + K>] * a[kCol<E0 + K>]), ...);
}

template <int E0, int... K>
__device__ __forceinline__ void store_entries(double* __restrict__ H, const double (&acc)[sizeof...(K)],
                                              const double (&dt)[kN], double c2, bool bad,
                                              std::integer_sequence<int, K...>) {
    ((H[kRow<E0 + K> * kN + kCol<E0 + K>] = H[kCol<E0 + K> * kN + kRow<E0 + K>] =
          bad ? 0.0 : c2 * dt[kRow<E0 + K>] * dt[kCol<E0 + K>] * acc[K]),
     ...);
}

// entries E0 .. E0 + kCnt - 1 of set s, one wave
template <int E0, int kCnt>
__device__ __forceinline__ void hess_wave(const double* __restrict__ planes,
                                          const double* __restrict__ rec,
                                          const double* __restrict__ mkt,
                                          const int* __restrict__ perm, int M, int64_t S, int64_t s,
                                          int lane, double* __restrict__ H) {
    const int64_t plane = S * (int64_t)M;
    const double* p = planes + s * M;
    const auto seq = std::make_integer_sequence<int, kCnt>{};
    double acc[kCnt];
#pragma unroll
    for (int k = 0; k < kCnt; ++k) acc[k] = 0.0;
    int bad = 0;
    for (int m0 = 0; m0 < M; m0 += 64) {             // every lane makes every pass
        const int m = m0 + lane;
        if (m < M) {
            const int c = perm[m];
            const double pr = p[c], mm = mkt[c];
            bad += (pr != pr || isinf(pr) || pr <= 0.0) ? 1 : 0;
            double a[kN];
#pragma unroll
            for (int i = 0; i < kN; ++i) a[i] = p[(i + 1) * plane + c] / mm;
            add_products<E0>(acc, a, seq);
        }
    }
#pragma unroll
    for (int k = 0; k < kCnt; ++k) acc[k] = xor_sum(acc[k], 64);
    for (int off = 1; off < 64; off <<= 1) bad += __shfl_xor(bad, off, 64);
    if (lane != 0) return;
    const double* q = rec + s * DH_PARAM_STRIDE;
    double dt[kN];
#pragma unroll
    for (int i = 0; i < kN; ++i) dt[i] = transform_dt(i, q);
    store_entries<E0>(H + s * (kN * kN), acc, dt, 2.0 / (double)M, bad > 0, seq);
}

// live_count: the device-resident driver's count of unfinished starts (a no-op at 0), or null
__global__ __launch_bounds__(kBlock) void gauss_newton_rows_kernel(
    const double* __restrict__ planes, const double* __restrict__ rec,
    const double* __restrict__ pen, const double* __restrict__ mkt, const int* __restrict__ row,
    const int* __restrict__ perm, int M, int64_t S, const int* __restrict__ live_count,
    double* __restrict__ f, double* __restrict__ g, int* __restrict__ n_bad,
    double* __restrict__ H) {
    if (live_count && __builtin_amdgcn_readfirstlane(*live_count) <= 0) return;
    const int64_t s = blockIdx.x;                    // grid = S blocks
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const double* mk = mkt + (int64_t)row[s] * M;
    switch (wave) {
        case 0:
            dhpg::loss_grad_wave<true>(planes, rec, pen, mk, perm, M, S, s, lane, f, g, n_bad);
            break;
        case 1: hess_wave<0, kPerWave>(planes, rec, mk, perm, M, S, s, lane, H); break;
        case 2: hess_wave<kPerWave, kPerWave>(planes, rec, mk, perm, M, S, s, lane, H); break;
        case 3: hess_wave<2 * kPerWave, kPerWave>(planes, rec, mk, perm, M, S, s, lane, H); break;
        default:
            hess_wave<3 * kPerWave, kUpper - 3 * kPerWave>(planes, rec, mk, perm, M, S, s, lane, H);
    }
}

// Stages 2 and 3 of a request over records already on the device: param_grad_kernel into the
// planes, then the reduction (R.extra: the Hessians).  The Levenberg-Marquardt driver's iteration.
int gauss_newton_rows_launch(dh_ctx* ctx, const dh_surface* s, const dhpg::GradRows& R, int N,
                             double L, hipStream_t st) {
    const int rc =
        dhpg::launch_param_grad(ctx, dhpg::surface_args(s, R.rec, R.S, N, L, R.planes), R.S, st);
    if (rc) return rc;
    hipLaunchKernelGGL(gauss_newton_rows_kernel, dim3((unsigned)R.S), dim3(kBlock), 0, st,
                       (const double*)R.planes, R.rec, R.pen, R.mkt, R.row, (const int*)s->perm,
                       s->M, (int64_t)R.S, R.live_count, R.f, R.g, R.bad, R.extra);
    HIP_TRY(hipGetLastError());
    return DH_OK;
}

}  // namespace dhgn

extern "C" int dh_surface_gauss_newton_rows_dev(dh_ctx* ctx, const dh_surface* s, const double* d_x,
                                                const double* d_mkt, const double* d_spot,
                                                const double* d_rate, const int32_t* d_row, int S,
                                                int N, double L, double* d_f, double* d_g,
                                                int32_t* d_bad, double* d_H, void* stream) {
    dhpg::GradRows R{};
    R.extra = d_H;                                   // the caller's: the scratch holds none
    R.mkt = d_mkt;
    R.row = (const int*)d_row;
    R.f = d_f;
    R.g = d_g;
    R.bad = (int*)d_bad;
    R.S = S;
    return dhpg::rows_request_dev(ctx, s,
                                  {{d_x, "x"}, {d_mkt, "mkt"}, {d_spot, "spot"}, {d_rate, "rate"},
                                   {d_row, "row"}, {d_f, "f"}, {d_g, "g"}, {d_bad, "bad"},
                                   {d_H, "H"}},
                                  d_x, d_spot, d_rate, R, dhpg::Scratch::kPrice,
                                  dhgn::gauss_newton_rows_launch, N, L, stream);
}

extern "C" int dh_surface_gauss_newton_rows(dh_ctx* ctx, const dh_surface* s, const double* x,
                                            const double* mkt, const double* spot,
                                            const double* rate, const int32_t* row, int S, int B,
                                            int N, double L, double* f, double* g, int32_t* bad,
                                            double* H) {
    return dhpg::rows_round_trip(
        ctx, s,
        {{x, "x"}, {mkt, "mkt"}, {spot, "spot"}, {rate, "rate"}, {row, "row"}, {f, "f"}, {g, "g"},
         {bad, "bad"}, {H, "H"}},
        dhpg::RowsIo{x, mkt, nullptr, nullptr, spot, rate, row, f, g, bad, H}, S, B,
        (size_t)S * dhgn::kN * dhgn::kN, N, L, dhpg::no_prep,
        [&](const dhpg::RowsIo& d, hipStream_t st) {
            return dh_surface_gauss_newton_rows_dev(ctx, s, d.x, d.mkt, d.spot, d.rate, d.row, S,
                                                    N, L, d.f, d.g, d.bad, d.extra, st);
        });
}

