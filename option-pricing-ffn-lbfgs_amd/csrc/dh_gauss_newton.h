// dh_gauss_newton.h -- the Gauss-Newton rows reduction (dh_surface_gauss_newton_rows*; DESIGN.md
// 3.21): from the [14][S][M] planes of param_grad_kernel and the records and penalties of
// x_records_rows_kernel, per set s against its market row,
//     f, g, n_bad   dh_surface_loss_grad_rows's, bit for bit, and
//     H_ij = (2 / M) dt_i dt_j sum_m a_im a_jm,   a_im = plane_i[m] / mkt_m,
// the Gauss-Newton Hessian of the price part of the loss in the optimiser's x (dt: the transform's
// derivative, loss_grad_wave's).  The Feller penalty enters g only.  Included by dh_kernels.hip
// after dh_param_grad.h and ahead of dh_lb_driver.h, whose Levenberg-Marquardt iteration launches
// it; needs dh_param_grad.h (loss_grad_wave, launch_param_grad, x_records_rows_kernel) and
// dh_loss_rows.h (check_rows).
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
    for (int i = 0; i < kN; ++i)
        dt[i] = (i == 4 || i == 9) ? 1.0 - q[i] * q[i] : (i == 11 ? 1.0 : q[i]);
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

// Stages 2 and 3 of a request over records already on the device: param_grad_kernel into d_planes
// [14][S][M], then the reduction.  The Levenberg-Marquardt driver's iteration.
int gauss_newton_rows_launch(dh_ctx* ctx, const dh_surface* s, const double* d_rec,
                             const double* d_pen, const double* d_mkt, const int* d_row, int S,
                             int N, double L, double* d_planes, double* d_f, double* d_g,
                             int* d_bad, double* d_H, hipStream_t st, const int* live_count) {
    const int rc = dhpg::launch_param_grad(ctx, dhpg::surface_args(s, d_rec, S, N, L, d_planes), S, st);
    if (rc) return rc;
    hipLaunchKernelGGL(gauss_newton_rows_kernel, dim3((unsigned)S), dim3(kBlock), 0, st,
                       (const double*)d_planes, d_rec, d_pen, d_mkt, d_row, (const int*)s->perm,
                       s->M, (int64_t)S, live_count, d_f, d_g, d_bad, d_H);
    HIP_TRY(hipGetLastError());
    return DH_OK;
}

// dh_surface_loss_grad_rows_dev's pointer checks, and H
int check_pointers(const void* x, const void* mkt, const void* spot, const void* rate,
                   const void* row, const void* f, const void* g, const void* bad, const void* H) {
    if (!x) return fail(DH_E_ARG, "x is null");
    if (!mkt) return fail(DH_E_ARG, "mkt is null");
    if (!spot) return fail(DH_E_ARG, "spot is null");
    if (!rate) return fail(DH_E_ARG, "rate is null");
    if (!row) return fail(DH_E_ARG, "row is null");
    if (!f) return fail(DH_E_ARG, "f is null");
    if (!g) return fail(DH_E_ARG, "g is null");
    if (!bad) return fail(DH_E_ARG, "bad is null");
    if (!H) return fail(DH_E_ARG, "H is null");
    return DH_OK;
}

}  // namespace dhgn

extern "C" int dh_surface_gauss_newton_rows_dev(dh_ctx* ctx, const dh_surface* s, const double* d_x,
                                                const double* d_mkt, const double* d_spot,
                                                const double* d_rate, const int32_t* d_row, int S,
                                                int N, double L, double* d_f, double* d_g,
                                                int32_t* d_bad, double* d_H, void* stream) {
    int rc = dhpg::check_loss_grad_rows(ctx, s, S, N, L);
    if (rc) return rc;
    rc = dhgn::check_pointers(d_x, d_mkt, d_spot, d_rate, d_row, d_f, d_g, d_bad, d_H);
    if (rc) return rc;
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    // dh_surface_loss_grad_rows_dev's scratch and layout: records, penalties, planes
    HIP_TRY(ctx->pg_scratch.reserve(dhpg::loss_grad_scratch(S, s->M)));
    double* d_rec = (double*)ctx->pg_scratch.ptr;
    double* d_pen = d_rec + (size_t)S * DH_PARAM_STRIDE;
    double* d_planes = d_pen + S;
    hipLaunchKernelGGL(dhpg::x_records_rows_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256),
                       0, st, d_x, S, d_spot, d_rate, (const int*)d_row, d_rec, d_pen);
    HIP_TRY(hipGetLastError());
    return dhgn::gauss_newton_rows_launch(ctx, s, d_rec, d_pen, d_mkt, (const int*)d_row, S, N, L,
                                          d_planes, d_f, d_g, (int*)d_bad, d_H, st, nullptr);
}

extern "C" int dh_surface_gauss_newton_rows(dh_ctx* ctx, const dh_surface* s, const double* x,
                                            const double* mkt, const double* spot,
                                            const double* rate, const int32_t* row, int S, int B,
                                            int N, double L, double* f, double* g, int32_t* bad,
                                            double* H) {
    int rc = dhpg::check_loss_grad_rows(ctx, s, S, N, L);
    if (rc) return rc;
    rc = dhgn::check_pointers(x, mkt, spot, rate, row, f, g, bad, H);
    if (rc) return rc;
    rc = check_rows(row, S, B);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) {
        if (!std::isfinite(spot[b]) || !(spot[b] > 0.0))
            return fail(DH_E_ARG, "spot " + std::to_string(b) + " is not finite or not > 0");
        if (!std::isfinite(rate[b]))
            return fail(DH_E_ARG, "rate " + std::to_string(b) + " is not finite");
    }
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    constexpr int kN = dhgn::kN;
    const size_t xb = (size_t)S * kN * 8, hb = (size_t)S * kN * kN * 8, mb = (size_t)B * s->M * 8;
    hipStream_t st = ctx->stream;
    // x [S][13], then f [S], g [S][13], H [S][13][13], spot [B], rate [B], bad [S]
    HIP_TRY(ctx->pg_io.reserve(2 * xb + hb + (size_t)S * 16 + (size_t)B * 16));
    HIP_TRY(ctx->rows_mkt.reserve(mb));
    HIP_TRY(ctx->rows_row.reserve((size_t)S * 4));
    double* d_x = (double*)ctx->pg_io.ptr;
    double* d_f = d_x + (size_t)S * kN;
    double* d_g = d_f + S;
    double* d_H = d_g + (size_t)S * kN;
    double* d_spot = d_H + (size_t)S * kN * kN;
    double* d_rate = d_spot + B;
    int32_t* d_bad = (int32_t*)(d_rate + B);
    HIP_TRY(hipMemcpyAsync(d_x, x, xb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_spot, spot, (size_t)B * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_rate, rate, (size_t)B * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->rows_mkt.ptr, mkt, mb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->rows_row.ptr, row, (size_t)S * 4, hipMemcpyHostToDevice, st));
    rc = dh_surface_gauss_newton_rows_dev(ctx, s, d_x, (const double*)ctx->rows_mkt.ptr, d_spot,
                                          d_rate, (const int32_t*)ctx->rows_row.ptr, S, N, L, d_f,
                                          d_g, d_bad, d_H, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(f, d_f, (size_t)S * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(g, d_g, xb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(H, d_H, hb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(bad, d_bad, (size_t)S * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}
