// dh_mc_vr.h -- the control variate of the Monte Carlo path pricer (DH_MC_VR_CONTROL of
// dh_mc_price_vr*): a control whose mean the library knows exactly.  Included by dh_mc.h between its
// walk and its kernels, which call control() per sample and control_estimate() per option; the
// antithetic pairs are the walk's own (mc_step<true>, dh_mc.h).  DESIGN.md 3.15.2 is the contract;
// tests/mc_vr_reference.py restates it in NumPy.
//
// The control of an option is the terminal spot (mean S0 after discounting) for Europeans and
// strike-0 options, else the European payoff of the same strike, type and maturity, whose mean is
// the COS price dh_surface_price_dev puts on the device.
#pragma once
#pragma clang fp contract(off)

namespace dhmc {

// the control of one option on one path: S at the maturity step where the known mean is S0, else
// the European twin's payoff
__device__ __forceinline__ double control(const Opt& o, int step, const State& s) {
    const bool spot = o.kind == DH_MC_EUROPEAN || o.strike == 0.0;
    return spot ? s.S : payoff(DH_MC_EUROPEAN, o.is_call, o.strike, 0.0, step, s);
}

// The estimator of DESIGN.md 3.15.2 from an option's five sums over n samples (sum y, sum y^2,
// sum c, sum c^2, sum y c), cyy = sum y^2 - (sum y)^2 / n and the control's known mean.
__device__ __forceinline__ void control_estimate(const double (&sum)[kVrSums], double n,
                                                 double disc, double cyy, double base_price,
                                                 double mean, double& beta, double& price,
                                                 double& err) {
    const double sy = sum[0], sc = sum[2], scc = sum[3], syc = sum[4];
    const double ccc = scc - sc * sc / n;
    const double cyc = syc - sy * sc / n;
    beta = ccc > 0.0 ? cyc / ccc : 0.0;
    price = base_price - beta * (disc * sc / n - mean);
    err = disc * sqrt(fmax(cyy - beta * cyc, 0.0) / (n * (n - 1.0)));
}

// the records with q (slot 15) zeroed: the path pricer does not read q, the COS pricer does
__global__ __launch_bounds__(kThreads) void mc_vr_records_kernel(const double* __restrict__ prm,
                                                                 int64_t n,
                                                                 double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = (i % DH_PARAM_STRIDE) == 15 ? 0.0 : prm[i];
}

// ---- host side ---------------------------------------------------------------------------------
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

// The controls' known means on the device, enqueued on `st`: d_twin [n_options] = each sorted
// option's column among the n_twins twins (-1: the mean is S0), d_cos [P][n_twins] = the twins' COS
// prices under the records with q = 0 (null without twins).
int control_means(dh_ctx* ctx, const double* d_params, int64_t P, const std::vector<Opt>& sorted,
                  int32_t* d_twin, hipStream_t st, int& n_twins, const double*& d_cos) {
    std::vector<int32_t> twin;
    int rc = twins_surface(ctx, sorted, st, twin);
    if (rc) return rc;
    n_twins = ctx->vr_surf->M;
    // pageable source: the copy has read `twin` when the call returns
    HIP_TRY(hipMemcpyAsync(d_twin, twin.data(), twin.size() * 4, hipMemcpyHostToDevice, st));
    d_cos = nullptr;
    if (n_twins == 0) return DH_OK;
    const int64_t n_el = P * DH_PARAM_STRIDE;
    HIP_TRY(ctx->mc_vr_rec.reserve((size_t)n_el * 8));
    HIP_TRY(ctx->mc_vr_cos.reserve((size_t)P * n_twins * 8));
    hipLaunchKernelGGL(mc_vr_records_kernel, dim3((unsigned)((n_el + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, st, d_params, n_el, (double*)ctx->mc_vr_rec.ptr);
    HIP_TRY(hipGetLastError());
    const int last_path = ctx->last_path;
    rc = dh_surface_price_dev(ctx, ctx->vr_surf, (const double*)ctx->mc_vr_rec.ptr, P,
                              DH_MC_VR_COS_N, DH_MC_VR_COS_L, (double*)ctx->mc_vr_cos.ptr, st);
    ctx->last_path = last_path;
    if (rc) return rc;
    d_cos = (const double*)ctx->mc_vr_cos.ptr;
    return DH_OK;
}

}  // namespace dhmc
