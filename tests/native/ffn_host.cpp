// CPU twin of the warm-start network's inference kernel
// (option-pricing-ffn-lbfgs_amd/csrc/dh_ffn.h), for tests only: tests/test_ffn.py holds it to the
// float64 truth within a derived bound, and the GPU tests hold the device to it bit for bit.  The
// prologue, ReLU and epilogue are the header's own functions; a neuron is a plain fmaf chain from
// its bias over k ascending, the chain the f32 MFMA is documented to be.  The kernel pads F up to
// a multiple of kUnroll with zero features under zero weights: the twin takes those steps too (they
// change nothing but the sign of a chain that sits at -0).  Built by the csrc Makefile (target
// ffnhost) with contraction off.
#include <math.h>
#include <stdint.h>

#include <vector>

#define DH_HD
#define DH_FFN_HOST_ONLY
#include "dh_ffn.h"

extern "C" {

// dh_ffn_create's description of the network, dh_ffn_forward's arrays -> x0 [B][13], raw [B][13]
int ffnh_forward(int n_layers, const int* widths, const float* weights, const float* biases,
                 const double* C, int M, const double* x_mean, const double* x_std,
                 const double* y_mean, const double* y_std, const double* market,
                 const double* spots, int64_t B, double* x0, float* raw) {
    using namespace dhffn;
    if (n_layers < 1 || widths[n_layers] != kOut) return -1;
    const int F = widths[0];
    int widest = 0;
    for (int l = 0; l <= n_layers; ++l) widest = widths[l] > widest ? widths[l] : widest;
    std::vector<float> a(widest), b(widest);
    for (int64_t i = 0; i < B; ++i) {
        for (int k = 0; k < F; ++k)
            a[k] = ffn_feature(C + (size_t)k * M, market + i * M, M, spots[i], x_mean[k], x_std[k]);
        const float* W = weights;
        const float* bias = biases;
        for (int l = 0; l < n_layers; ++l) {
            const int in = widths[l], on = widths[l + 1];
            for (int n = 0; n < on; ++n) {
                float acc = bias[n];
                for (int k = 0; k < in; ++k) acc = fmaf(a[k], W[(size_t)n * in + k], acc);
                for (int k = in; k % kUnroll; ++k) acc = fmaf(0.0f, 0.0f, acc);   // the pad steps
                b[n] = l + 1 < n_layers ? ffn_relu(acc) : acc;
            }
            a.swap(b);
            W += (size_t)in * on;
            bias += on;
        }
        for (int o = 0; o < kOut; ++o) {
            raw[i * kOut + o] = a[o];
            x0[i * kOut + o] = ffn_output(y_std[o], a[o], y_mean[o]);
        }
    }
    return 0;
}

}  // extern "C"
