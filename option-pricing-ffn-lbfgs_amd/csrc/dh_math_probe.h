// dh_math_probe.h -- test support: the fp64 elementary functions of dh_device.h over arrays
// (dh_math_probe), one lane per element, so that each can be compared alone with a high-precision
// truth (tests/test_gpu_math.py, tests/golden/math_truth.npz, tools/math_accuracy.py).  Included
// at the end of dh_kernels.hip; no production path calls it.
//
// The kernel calls the inline functions of dh_device.h themselves, after filling the LDS math
// tables with load_math_tables and a __syncthreads() as the production kernels do.  Device code is
// built with the compiler's default contraction, so an inlined call site in a production kernel
// may fuse a multiply-add differently from the probe's: the probe tests each function as written,
// and the bounds of its test leave room for that.  It is not a bit-for-bit statement about any one
// call site.
//
// Layout (n = number of results; out0 and out1 always hold n doubles each):
//   one real argument  (dsincos*, dexp*, dlog*, drcp, dsqrt_rsqrt*): x[n]; y is not read.
//       out0 / out1 = sin / cos, sqrt / rsqrt; the single-result functions write out0, out1 = 0.
//   atan2 (datan2, datan2_t): x[n] is atan2's first argument (the "y" of atan2(y, x)), y[n] its
//       second; out0 = the angle, out1 = 0.
//   csqrt_p: z = x[n] + i y[n]; out0 + i out1 = the root.
//   cdiv, cdiv_rcp: two operands as two calls' worth of arrays, x[2n] and y[2n]: the numerator is
//       x[i] + i y[i], the divisor x[n + i] + i y[n + i]; out0 + i out1 = the quotient.
#pragma once

namespace dhprobe {

enum Fn : int {
    kSincos = 0, kSincosT, kExp, kExpNonpos, kExpT, kExpTNonpos, kLog, kLogT, kAtan2, kAtan2T,
    kRcp, kSqrtRsqrt, kSqrtRsqrtPos, kCsqrt, kCdiv, kCdivRcp, kFnCount
};

inline bool two_args(int fn) { return fn == kAtan2 || fn == kAtan2T || fn >= kCsqrt; }
inline bool two_operands(int fn) { return fn == kCdiv || fn == kCdivRcp; }

__global__ __launch_bounds__(256) void math_probe_kernel(int fn, const double* __restrict__ x,
                                                         const double* __restrict__ y, int64_t n,
                                                         double* __restrict__ out0,
                                                         double* __restrict__ out1) {
    __shared__ double2 tab[dh::kMathTab];
    dh::load_math_tables(tab, 0);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double a = x[i];
    double r0 = 0.0, r1 = 0.0;
    switch (fn) {
        case kSincos: dh::dsincos(a, &r0, &r1); break;
        case kSincosT: dh::dsincos_t(a, tab, &r0, &r1); break;
        case kExp: r0 = dh::dexp(a); break;
        case kExpNonpos: r0 = dh::dexp_nonpos(a); break;
        case kExpT: r0 = dh::dexp_t(a, tab); break;
        case kExpTNonpos: r0 = dh::dexp_t_nonpos(a, tab); break;
        case kLog: r0 = dh::dlog(a); break;
        case kLogT: r0 = dh::dlog_t(a, tab); break;
        case kAtan2: r0 = dh::datan2(a, y[i]); break;
        case kAtan2T: r0 = dh::datan2_t(a, y[i], tab); break;
        case kRcp: r0 = dh::drcp(a); break;
        case kSqrtRsqrt: dh::dsqrt_rsqrt(a, r0, r1); break;
        case kSqrtRsqrtPos: dh::dsqrt_rsqrt_pos(a, r0, r1); break;
        case kCsqrt: {
            const dh::cplx r = dh::csqrt_p({a, y[i]});
            r0 = r.re, r1 = r.im;
            break;
        }
        case kCdiv: {
            const dh::cplx r = dh::cdiv({a, y[i]}, {x[n + i], y[n + i]});
            r0 = r.re, r1 = r.im;
            break;
        }
        case kCdivRcp: {
            const dh::cplx r = dh::cdiv_rcp({a, y[i]}, {x[n + i], y[n + i]});
            r0 = r.re, r1 = r.im;
            break;
        }
        default: break;
    }
    out0[i] = r0;
    out1[i] = r1;
}

}  // namespace dhprobe

extern "C" int dh_math_probe(dh_ctx* ctx, int fn, const double* x, const double* y, int64_t n,
                             double* out0, double* out1) {
    if (!ctx) return fail(DH_E_ARG, "ctx is null");
    if (fn < 0 || fn >= dhprobe::kFnCount) return fail(DH_E_ARG, "dh_math_probe: unknown fn");
    if (n < 0) return fail(DH_E_ARG, "n < 0");
    if (n > 0 && (!x || !out0 || !out1 || (dhprobe::two_args(fn) && !y)))
        return fail(DH_E_ARG, "null argument");
    if (n == 0) return DH_OK;
    if ((n + 255) / 256 > 0x7fffffffLL) return fail(DH_E_ARG, "launch too large");
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.rc) return dev_scope.rc;
    const int64_t n_in = dhprobe::two_operands(fn) ? 2 * n : n;
    const size_t ib = (size_t)n_in * 8, ob = (size_t)n * 8;
    HIP_TRY(ctx->aux0.reserve(ib));
    HIP_TRY(ctx->aux1.reserve(ib));
    HIP_TRY(ctx->aux2.reserve(ob));
    HIP_TRY(ctx->aux3.reserve(ob));
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(ctx->aux0.ptr, x, ib, hipMemcpyHostToDevice, st));
    if (dhprobe::two_args(fn))
        HIP_TRY(hipMemcpyAsync(ctx->aux1.ptr, y, ib, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(dhprobe::math_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       st, fn, (const double*)ctx->aux0.ptr, (const double*)ctx->aux1.ptr, n,
                       (double*)ctx->aux2.ptr, (double*)ctx->aux3.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out0, ctx->aux2.ptr, ob, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out1, ctx->aux3.ptr, ob, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
}
