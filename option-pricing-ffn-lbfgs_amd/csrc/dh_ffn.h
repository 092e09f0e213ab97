// dh_ffn.h -- the warm-start network's inference on the device (dh_ffn_create, dh_ffn_destroy,
// dh_ffn_forward, dh_ffn_forward_dev).  Included by dh_kernels.hip after its host helpers, and by
// tests/native/ffn_host.cpp (DH_FFN_HOST_ONLY: the shared scalar functions alone).  DESIGN.md 3.22.
//
// One launch, ffn_forward_kernel: a block of 8 waves owns a tile of kTM = 32 markets and walks the
// whole network on it.
//   prologue  fp64: feature i = (sum_j C[i][j] p[j]) / S0, j ascending by explicit fma, then
//             (f - x_mean) / x_std, one rounding to float (ffn_feature, shared with the host twin)
//   layers    v_mfma_f32_32x32x2_f32: D[market][neuron] += act[market][k] Wt[k][neuron].  A wave
//             owns the neuron tiles wave, wave + 8 (<= 16 tiles of 32 at 512 wide), one
//             accumulator tile each, started from the bias; k ascends two at a time, and the
//             instruction sums its two k in order, so every output element is ONE fmaf chain
//             bias -> k = 0 -> ... -> k = K - 1 whatever B and whatever the market's row in the
//             tile.  No split-K, no atomics.  ReLU is fmaxf(0, .) on the hidden layers.
//   epilogue  fp64: x0 = fma(y_std, (double)raw, y_mean) (ffn_output, shared)
// The tile's activations live in LDS as float, transposed: act[k][market] with a row stride of
// kStride = 33 floats, in two buffers that the layers alternate between.  A lane's A operand is
// act[k + (lane >> 5)][lane & 31] (consecutive banks); its results are column lane & 31 of the
// next layer's act, rows (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) -- the standard C/D map.  The
// weights are stored transposed and padded, Wt[k][n] (k up to a multiple of 8, n of 32, zeros),
// so a lane's B operand Wt[k + (lane >> 5)][n0 + (lane & 31)] is a coalesced 128-byte row piece;
// they are streamed from global memory (712 KB at the default widths: L2-resident).
// Rows of the last tile past B hold zeros, run the same arithmetic and are not stored.
#pragma once
#pragma clang fp contract(off)

#include <math.h>
#include <stdint.h>

#ifndef DH_HD
#define DH_HD __host__ __device__
#endif

namespace dhffn {

constexpr int kOut = 13;            // the optimiser's x
constexpr int kTM = 32;             // markets per block (DH_FFN_TM)
constexpr int kMaxHidden = 6;       // hidden layers at most (DH_FFN_MAX_HIDDEN)
constexpr int kMaxLayers = kMaxHidden + 1;   // weight layers: the hidden ones and the output
constexpr int kMaxWidth = 512;      // widest hidden layer (DH_FFN_MAX_WIDTH)
constexpr int kMaxIn = 64;          // features F and prices M per market at most (DH_FFN_MAX_IN)
constexpr int kStride = kTM + 1;    // floats per activation row in LDS
constexpr int kWaves = 8;           // waves per block: 2 neuron tiles each at 512 wide
constexpr int kUnroll = 8;          // k per trip of a layer's loop; F is padded up to a multiple

// Standardised feature of one market, rounded once to float: C_row [M] the feature's row of the
// matrix, p [M] the market's prices.  No a * b + c is left to the compiler: the sum is explicit
// fma, the rest a division, a subtraction and a division.
DH_HD inline float ffn_feature(const double* C_row, const double* p, int M, double S0, double mean,
                               double std) {
    double s = 0.0;
    for (int j = 0; j < M; ++j) s = fma(C_row[j], p[j], s);
    const double f = s / S0;
    return (float)((f - mean) / std);
}

DH_HD inline float ffn_relu(float v) { return fmaxf(0.0f, v); }

// The optimiser-space output of the network's standardised output raw
DH_HD inline double ffn_output(double y_std, float raw, double y_mean) {
    return fma(y_std, (double)raw, y_mean);
}

}  // namespace dhffn

#ifndef DH_FFN_HOST_ONLY

namespace dhffn {

// The padded network as the kernel walks it (a kernel argument, by value)
struct Layers {
    int n;                      // weight layers
    int kpad[kMaxLayers];       // input width of layer l, padded to a multiple of kUnroll
    int npad[kMaxLayers];       // output width of layer l, padded to a multiple of 32
    int w_off[kMaxLayers];      // float offset of Wt_l [kpad][npad] in the weight block
    int b_off[kMaxLayers];      // float offset of its bias [npad]
    int buf_off[2];             // float offsets of the two activation buffers in LDS
};

using f32x16 = __attribute__((ext_vector_type(16))) float;

__global__ __launch_bounds__(kWaves * 64) void ffn_forward_kernel(
    const float* __restrict__ wts, const double* __restrict__ C, const double* __restrict__ stats,
    const double* __restrict__ market, const double* __restrict__ spots, int64_t B, int F, int M,
    double* __restrict__ x0, float* __restrict__ raw_out, Layers L) {
    extern __shared__ float ffn_act[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * kTM;
    float* cur = ffn_act + L.buf_off[0];
    float* nxt = ffn_act + L.buf_off[1];

    // prologue: act[k][m], k < kpad[0]; the pad row and the rows past B are zeros
    for (int e = tid; e < L.kpad[0] * kTM; e += kWaves * 64) {
        const int k = e / kTM, m = e - k * kTM;
        const int64_t row = row0 + m;
        float v = 0.0f;
        if (k < F && row < B)
            v = ffn_feature(C + (size_t)k * M, market + row * M, M, spots[row], stats[k],
                            stats[F + k]);
        cur[k * kStride + m] = v;
    }
    __syncthreads();

    for (int l = 0; l < L.n; ++l) {
        const float* __restrict__ W = wts + L.w_off[l];
        const float* __restrict__ bias = wts + L.b_off[l];
        const int K = L.kpad[l], N = L.npad[l], NT = N >> 5;
        const bool hidden = l + 1 < L.n;
        // this wave's neuron tiles: wave and wave + kWaves (NT <= 2 kWaves)
        const bool on0 = wave < NT, on1 = wave + kWaves < NT;
        const int n0 = wave * 32 + j, n1 = (wave + kWaves) * 32 + j;
        f32x16 acc0, acc1;
        {
            const float b0 = on0 ? bias[n0] : 0.0f, b1 = on1 ? bias[n1] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc0[r] = b0, acc1[r] = b1;
        }
        // K is a multiple of kUnroll: four MFMA steps' operands are loaded ahead of their use
        if (on1) {
            for (int k0 = 0; k0 < K; k0 += kUnroll) {
                float a[kUnroll / 2], w0[kUnroll / 2], w1[kUnroll / 2];
#pragma unroll
                for (int u = 0; u < kUnroll / 2; ++u) {
                    const int k = k0 + 2 * u + h;
                    a[u] = cur[k * kStride + j];
                    w0[u] = W[(size_t)k * N + n0];
                    w1[u] = W[(size_t)k * N + n1];
                }
#pragma unroll
                for (int u = 0; u < kUnroll / 2; ++u) {
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], w0[u], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], w1[u], acc1, 0, 0, 0);
                }
            }
        } else if (on0) {
            for (int k0 = 0; k0 < K; k0 += kUnroll) {
                float a[kUnroll / 2], w0[kUnroll / 2];
#pragma unroll
                for (int u = 0; u < kUnroll / 2; ++u) {
                    const int k = k0 + 2 * u + h;
                    a[u] = cur[k * kStride + j];
                    w0[u] = W[(size_t)k * N + n0];
                }
#pragma unroll
                for (int u = 0; u < kUnroll / 2; ++u)
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], w0[u], acc0, 0, 0, 0);
            }
        }
        // results: column (neuron) on the lane, the 16 registers its market rows
        if (on0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = (r & 3) + 8 * (r >> 2) + 4 * h;
                nxt[n0 * kStride + m] = hidden ? ffn_relu(acc0[r]) : acc0[r];
            }
        }
        if (on1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = (r & 3) + 8 * (r >> 2) + 4 * h;
                nxt[n1 * kStride + m] = hidden ? ffn_relu(acc1[r]) : acc1[r];
            }
        }
        __syncthreads();
        float* t = cur;
        cur = nxt;
        nxt = t;
    }

    // epilogue: the first kOut neurons of the output layer, row-major [market][kOut]
    const double* y_mean = stats + 2 * F;
    const double* y_std = y_mean + kOut;
    for (int e = tid; e < kTM * kOut; e += kWaves * 64) {
        const int m = e / kOut, o = e - m * kOut;
        const int64_t row = row0 + m;
        if (row < B) {
            const float raw = cur[o * kStride + m];
            if (raw_out) raw_out[row * kOut + o] = raw;
            x0[row * kOut + o] = ffn_output(y_std[o], raw, y_mean[o]);
        }
    }
}

}  // namespace dhffn

struct dh_ffn {
    dh_ctx* ctx = nullptr;
    int device = 0;                // the context's, kept here: destroying needs no live context
    int F = 0, M = 0;
    dhffn::Layers L{};
    size_t lds_bytes = 0;
    float* d_w = nullptr;          // every layer's Wt and bias
    double* d_C = nullptr;         // [F][M]
    double* d_stats = nullptr;     // x_mean [F], x_std [F], y_mean [13], y_std [13]
    void* block = nullptr;         // the one device allocation the three point into
    DevBuf io;                     // staging of dh_ffn_forward's host arrays
};

extern "C" int dh_ffn_destroy(dh_ffn* f) {
    if (!f) return DH_OK;
    {
        DeviceScope dev_scope(f->device);
        if (f->block) (void)hipFree(f->block);
        f->io.release();
    }
    delete f;
    return DH_OK;
}

extern "C" int dh_ffn_create(dh_ctx* ctx, int n_layers, const int* widths, const float* weights,
                             const float* biases, const double* C, int M, const double* x_mean,
                             const double* x_std, const double* y_mean, const double* y_std,
                             dh_ffn** out) {
    using namespace dhffn;
    if (!ctx || !widths || !weights || !biases || !C || !x_mean || !x_std || !y_mean || !y_std ||
        !out)
        return fail(DH_E_ARG, "null argument");
    *out = nullptr;
    if (n_layers < 2 || n_layers > kMaxLayers)
        return fail(DH_E_ARG, "n_layers (hidden layers + 1) must be in [2, " +
                                  std::to_string(kMaxLayers) + "], got " +
                                  std::to_string(n_layers));
    const int F = widths[0];
    if (F < 1 || F > kMaxIn || M < 1 || M > kMaxIn)
        return fail(DH_E_ARG, "F and M must be in [1, " + std::to_string(kMaxIn) + "]");
    if (widths[n_layers] != kOut)
        return fail(DH_E_ARG, "the output width must be " + std::to_string(kOut));
    for (int l = 1; l < n_layers; ++l)
        if (widths[l] < 32 || widths[l] > kMaxWidth || widths[l] % 32)
            return fail(DH_E_ARG, "hidden width " + std::to_string(widths[l]) +
                                      ": a multiple of 32 in [32, " + std::to_string(kMaxWidth) +
                                      "]");
    for (int i = 0; i < F; ++i)
        if (!(x_std[i] > 0.0) || !std::isfinite(x_std[i]) || !std::isfinite(x_mean[i]))
            return fail(DH_E_ARG, "x_std must be finite and > 0, x_mean finite");
    for (int i = 0; i < kOut; ++i)
        if (!std::isfinite(y_std[i]) || !std::isfinite(y_mean[i]))
            return fail(DH_E_ARG, "y_mean and y_std must be finite");

    dh_ffn* f = new (std::nothrow) dh_ffn;
    if (!f) return fail(DH_E_ALLOC, "dh_ffn");
    f->ctx = ctx;
    f->device = ctx->device;
    f->F = F;
    f->M = M;
    Layers& L = f->L;
    L.n = n_layers;
    int total = 0, widest[2] = {0, 0};
    for (int l = 0; l < n_layers; ++l) {
        L.kpad[l] = (widths[l] + kUnroll - 1) & ~(kUnroll - 1);
        L.npad[l] = (widths[l + 1] + 31) & ~31;
        L.w_off[l] = total;
        total += L.kpad[l] * L.npad[l];
        L.b_off[l] = total;
        total += L.npad[l];
        // activation a (the input of layer a; a = n: the output) lives in buffer a & 1
        widest[l & 1] = std::max(widest[l & 1], L.kpad[l]);
        widest[(l + 1) & 1] = std::max(widest[(l + 1) & 1], L.npad[l]);
    }
    L.buf_off[0] = 0;
    L.buf_off[1] = widest[0] * kStride;
    f->lds_bytes = (size_t)(widest[0] + widest[1]) * kStride * sizeof(float);

    // transposed, zero-padded weights
    std::vector<float> host((size_t)total, 0.0f);
    size_t w_at = 0, b_at = 0;
    for (int l = 0; l < n_layers; ++l) {
        const int in = widths[l], on = widths[l + 1];
        for (int n = 0; n < on; ++n) {
            for (int k = 0; k < in; ++k)
                host[(size_t)L.w_off[l] + (size_t)k * L.npad[l] + n] = weights[w_at + (size_t)n * in + k];
            host[(size_t)L.b_off[l] + n] = biases[b_at + n];
        }
        w_at += (size_t)in * on;
        b_at += on;
    }
    std::vector<double> stats((size_t)2 * F + 2 * kOut);
    for (int i = 0; i < F; ++i) stats[i] = x_mean[i], stats[F + i] = x_std[i];
    for (int i = 0; i < kOut; ++i) stats[2 * F + i] = y_mean[i], stats[2 * F + kOut + i] = y_std[i];

    DeviceScope dev_scope(ctx->device);
    int rc = dev_scope.rc;
    auto done = [&](int code) {
        if (code) (void)dh_ffn_destroy(f);
        return code;
    };
    if (rc) return done(rc);
    hipError_t e = hipSuccess;
    // past the default cap of a launch's dynamic LDS: raised for the kernel on this device, to the
    // widest network's size (two buffers of kMaxWidth rows: 132 KiB of CDNA4's 160), so that a
    // later, narrower network never lowers it
    if (f->lds_bytes > 48 * 1024) {
        constexpr int most = 2 * kMaxWidth * kStride * (int)sizeof(float);
        e = hipFuncSetAttribute((const void*)ffn_forward_kernel,
                                hipFuncAttributeMaxDynamicSharedMemorySize, most);
        if (e != hipSuccess)
            return done(fail(DH_E_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e)));
    }
    const size_t wb = ((size_t)total * 4 + 255) & ~(size_t)255;
    const size_t cb = ((size_t)F * M * 8 + 255) & ~(size_t)255;
    const size_t sb = stats.size() * 8;
    e = hipMalloc(&f->block, wb + cb + sb);
    if (e != hipSuccess) {
        f->block = nullptr;
        return done(fail(DH_E_ALLOC, hipGetErrorString(e)));
    }
    f->d_w = (float*)f->block;
    f->d_C = (double*)((char*)f->block + wb);
    f->d_stats = (double*)((char*)f->block + wb + cb);
    // synchronous copies from the vectors above
    if ((e = hipMemcpy(f->d_w, host.data(), (size_t)total * 4, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(f->d_C, C, (size_t)F * M * 8, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(f->d_stats, stats.data(), sb, hipMemcpyHostToDevice)) != hipSuccess)
        return done(fail(DH_E_HIP, hipGetErrorString(e)));
    *out = f;
    return DH_OK;
}

extern "C" int dh_ffn_forward_dev(dh_ffn* f, const double* d_market, const double* d_spots,
                                  int64_t B, double* d_x0, float* d_raw, void* stream) {
    if (!f) return fail(DH_E_ARG, "ffn is null");
    if (B < 0) return fail(DH_E_ARG, "B < 0");
    if (B > 0 && (!d_market || !d_spots || !d_x0)) return fail(DH_E_ARG, "null argument");
    if (B == 0) return DH_OK;
    const int64_t blocks = (B + dhffn::kTM - 1) / dhffn::kTM;
    if (blocks > 0x7fffffff) return fail(DH_E_ARG, "B too large for one launch");
    DeviceScope dev_scope(f->device);
    if (dev_scope.rc) return dev_scope.rc;
    hipStream_t st = stream ? (hipStream_t)stream : f->ctx->stream;
    hipLaunchKernelGGL(dhffn::ffn_forward_kernel, dim3((unsigned)blocks), dim3(dhffn::kWaves * 64),
                       f->lds_bytes, st, (const float*)f->d_w, (const double*)f->d_C,
                       (const double*)f->d_stats, d_market, d_spots, B, f->F, f->M, d_x0, d_raw,
                       f->L);
    HIP_TRY(hipGetLastError());
    return DH_OK;
}

extern "C" int dh_ffn_forward(dh_ffn* f, const double* market, const double* spots, int64_t B,
                              double* x0, float* raw) {
    if (!f) return fail(DH_E_ARG, "ffn is null");
    if (B < 0) return fail(DH_E_ARG, "B < 0");
    if (B > 0 && (!market || !spots || !x0)) return fail(DH_E_ARG, "null argument");
    if (B == 0) return DH_OK;
    DeviceScope dev_scope(f->device);
    if (dev_scope.rc) return dev_scope.rc;
    // chunks of <= 1M markets bound the staging (the prices, the spot and both outputs per market)
    constexpr int64_t kChunk = int64_t(1) << 20;
    const int64_t cap = std::min(B, kChunk);
    const int M = f->M;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t mb = up((size_t)cap * M * 8), sb = up((size_t)cap * 8);
    const size_t xb = up((size_t)cap * dhffn::kOut * 8), rb = up((size_t)cap * dhffn::kOut * 4);
    HIP_TRY(f->io.reserve(mb + sb + xb + rb));
    char* base = (char*)f->io.ptr;
    double* d_m = (double*)base;
    double* d_s = (double*)(base + mb);
    double* d_x = (double*)(base + mb + sb);
    float* d_r = (float*)(base + mb + sb + xb);
    hipStream_t st = f->ctx->stream;
    for (int64_t i0 = 0; i0 < B; i0 += kChunk) {
        const int64_t n = std::min(kChunk, B - i0);
        HIP_TRY(hipMemcpyAsync(d_m, market + i0 * M, (size_t)n * M * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_s, spots + i0, (size_t)n * 8, hipMemcpyHostToDevice, st));
        const int rc = dh_ffn_forward_dev(f, d_m, d_s, n, d_x, raw ? d_r : nullptr, st);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(x0 + i0 * dhffn::kOut, d_x, (size_t)n * dhffn::kOut * 8,
                               hipMemcpyDeviceToHost, st));
        if (raw)
            HIP_TRY(hipMemcpyAsync(raw + i0 * dhffn::kOut, d_r, (size_t)n * dhffn::kOut * 4,
                                   hipMemcpyDeviceToHost, st));
        // the staging is reused by the next chunk
        HIP_TRY(hipStreamSynchronize(st));
    }
    return DH_OK;
}

#endif  // DH_FFN_HOST_ONLY
