/*
 * dhcos.h -- C-ABI of the MI355X-native Double-Heston + Merton-jump COS pricer and calibration
 * objective (libdhcos.so, gfx950).
 *
 * The reference (zenthepen/Option-Pricing-FFN-LBFGS) is pure Python; it has no FFI of its own.
 * Each entry point below replaces one reference call site on the hot path, named per function
 * (file:line in the reference).  The Python host layer (option-pricing-ffn-lbfgs_amd/dhcos) binds
 * these through ctypes; INTEGRATION.md shows the binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - Every function returns 0 on success and a negative DH_E* code on failure; the message of
 *     the last failure on the calling thread is returned by dh_last_error().
 *   - Numeric failures (NaN / inf / non-positive prices) are NOT errors: they are reported in the
 *     outputs exactly as the reference produces them (see dh_surface_loss).
 *   - "host" entry points take host pointers, copy synchronously and return when results are on
 *     the host (the caller may free its buffers on return).  "_dev" entry points take device
 *     pointers and enqueue on the given HIP stream (NULL = the context's own stream) without
 *     synchronising.
 *   - Param-set record: DH_PARAM_STRIDE (16) doubles per set:
 *       [0..12] v01 kappa1 theta1 sigma1 rho1 v02 kappa2 theta2 sigma2 rho2 lambda_j mu_j sigma_j
 *       [13] S0   [14] r   [15] q
 *     (double_heston.py:26-46 constructor arguments, same meaning).
 *   - All arithmetic is IEEE fp64.
 */
#ifndef DHCOS_H
#define DHCOS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DH_PARAM_STRIDE 16
#define DH_MAX_N 2048            /* longest COS series of the table (fast) path: LDS-resident */
#define DH_MAX_N_PER_TERM 65536  /* longest accepted: N > DH_MAX_N runs the per-term path (the
                                    reference's operation order, one wave per option), slower
                                    but any length the reference's pricing(N) takes up to here  */

enum {
    DH_OK = 0,
    DH_E_ARG = -1,               /* invalid argument (null pointer, bad size, N out of range) */
    DH_E_HIP = -2,               /* HIP runtime error (message has the HIP error string) */
    DH_E_NODEV = -3,             /* no usable gfx950 device */
    DH_E_ALLOC = -4,             /* host/device allocation failure */
    DH_E_COMM = -5               /* RCCL failure or librccl not loadable (message has the detail) */
};

/* strike_mode for surfaces */
enum {
    DH_STRIKE_ABSOLUTE = 0,      /* K[m] is the strike */
    DH_STRIKE_PCT_SPOT = 1       /* K[m] is K_relative; strike = K_relative * S0 / 100.0 per param
                                    set (synthetic_generator.py:125) */
};

typedef struct dh_ctx dh_ctx;
typedef struct dh_surface dh_surface;

/* ---- context ------------------------------------------------------------------------------ */
int dh_version(void);
const char* dh_last_error(void);
int dh_device_count(int* count);
/* One context per (device, host thread).  Owns a HIP stream and grow-only device scratch. */
int dh_ctx_create(int device, dh_ctx** out);
int dh_ctx_destroy(dh_ctx* ctx);
int dh_ctx_synchronize(dh_ctx* ctx);
/* The HIP stream the context launches on (hipStream_t as void*). */
void* dh_ctx_stream(dh_ctx* ctx);
/* Validation mode: when on, every option is priced by the per-term path in the reference's
 * operation order (own CF and sincos per COS term) instead of the shared-table fast path.   */
int dh_ctx_set_exact(dh_ctx* ctx, int on);
/* Adaptive tail of the fast path's angle sums (on by default): a table's COS terms past the last
 * one with |T2_k| > 2^-72 S0 / ((b - a)(1 + (b - a)/pi) N) are not summed, which moves no price by
 * more than 2^-64 of its k = 0 term.  Off: every term k < N is summed (A/B, tests). */
int dh_ctx_set_tail_cut(dh_ctx* ctx, int on);
/* Request kernels of the fast path.  AUTO (default): one fused launch per request when every
 * maturity group fits one tile (<= 256 options), except small tiles in large calls (generator
 * grids: a COS-table launch then the lane-per-option-group kernel); otherwise the table launch
 * then an option launch.  FUSED / SPLIT force one of the two where it applies.  Both produce
 * the same bits; the choice only changes speed.                                              */
enum { DH_PATH_AUTO = 0, DH_PATH_SPLIT = 1, DH_PATH_FUSED = 2, DH_PATH_GEN = 3 };
int dh_ctx_set_path(dh_ctx* ctx, int path);
/* DH_PATH_FUSED, DH_PATH_SPLIT or DH_PATH_GEN (AUTO only: generator grids -- every maturity group
 * one tile of <= 16 options in a call of >= 65,536 tasks -- priced by one fused small-tile
 * launch, agreeing with the other paths to ~1e-15): the kernels the last fast-path request ran
 * (0 before any).                                                                              */
int dh_ctx_last_path(dh_ctx* ctx);
/* Diagnostics (only in the DH_STAMPS build, `make stamps`; the production library returns
 * DH_E_ARG): record per-block s_memtime phase stamps of the COS kernels, read the last request's. */
int dh_ctx_debug_stamps(dh_ctx* ctx, int on);
int dh_ctx_read_stamps(dh_ctx* ctx, unsigned long long* out, int64_t cap, int64_t* n);

/* ---- option surfaces ---------------------------------------------------------------------- */
/* Upload an option set once.  Options are grouped by exact maturity on the host; groups are cut
 * into tiles of at most 256 options; every tile shares one COS/CF table per param set.
 *   K, T, is_call: [M]   (is_call resolved by the caller as option_type.upper()[0]=='C',
 *                         double_heston.py:172)
 *   mkt:           [M] market prices, may be NULL (needed only by dh_surface_loss*)
 * Replaces the per-option DoubleHeston construction in lbfgs_calibrator.py:128-150 and
 * synthetic_generator.py:123-138.                                                           */
int dh_surface_create(dh_ctx* ctx, const double* K, const double* T, const int8_t* is_call,
                      const double* mkt, int M, int strike_mode, dh_surface** out);
int dh_surface_destroy(dh_surface* s);
int dh_surface_size(const dh_surface* s, int* M, int* n_tiles);
/* Form, once, what the request kernels otherwise form per table from the spot and the surface
 * alone: log(K / S0) and K / S0 of every option (DH_STRIKE_PCT_SPOT: the strike K_relative * S0 /
 * 100.0 too), by the kernels' own device functions, so the same bits.  A fused request block whose
 * record carries exactly this S0 (the same 64 bits) loads the values; any other record, and every
 * request on a surface never staged, computes them as before.  S0 finite and > 0; calling it again
 * restages.  Runs on the context's stream and waits for it: requests on any stream may follow.
 * Not to be called while a request on the surface is in flight.                                 */
int dh_surface_stage_spot(dh_surface* s, double S0);

/* Price every option of the surface under every param set: out[p*M + m], m in the caller's
 * original option order.  Replaces DoubleHeston.pricing(N) (double_heston.py:160-192) called
 * P*M times.  L is the truncation width (truncationRange(L=10), double_heston.py:100).        */
int dh_surface_price(dh_ctx* ctx, const dh_surface* s, const double* params, int64_t P, int N,
                     double L, double* out);

/* The generator's pricing from its sampler's columns (synthetic_generator.py:123-138): params
 * [P][13] model params, spots [P] (each record's S0), one rate r and q = 0 -- the records of
 * dh_surface_price, formed on the device (no host packing pass), then priced into out[P][M].
 * Host buffers; registered ones (dh_host_register) move by DMA without staging copies.         */
int dh_surface_price_cols(dh_ctx* ctx, const dh_surface* s, const double* params,
                          const double* spots, double r, int64_t P, int N, double L, double* out);
/* Page-lock a host range for the copies of the calls above (hipHostRegister) and release it.
 * A range must be unregistered before its memory is freed.                                     */
int dh_host_register(void* ptr, size_t bytes);
int dh_host_unregister(void* ptr);

/* Calibration objective over the surface for S param sets (one FD request = 14 sets):
 *   sse[s]   = sum_m ((price_sm - mkt_m) / mkt_m)^2      (lbfgs_calibrator.py:163, un-normalised)
 *   n_bad[s] = #{m : price_sm is NaN, +-inf or <= 0}      (lbfgs_calibrator.py:152)
 *   prices   = optional [S][M] output (NULL to skip)
 * The host forms loss = n_bad ? 1e10 : sse / M + feller (lbfgs_calibrator.py:118-177).
 * A fused request sums each set's tile partials in its own tail; a sum whose
 * hand-off never completed (bounded wait, never observed) leaves n_bad[s] = -1 and the call
 * returns DH_E_HIP.                                                                            */
int dh_surface_loss(dh_ctx* ctx, const dh_surface* s, const double* params, int S, int N,
                    double L, double* sse, int32_t* n_bad, double* prices);

/* Device-pointer variants: params/out/sse/n_bad are device pointers; enqueue on `stream`
 * (hipStream_t; NULL = context stream).  No synchronisation, no allocation after warm-up.
 * A request is one fused launch or two launches (COS table, then options), dh_ctx_set_path;
 * in loss mode each param set's sum is finalised in a fixed order (n_bad[s] = -1: a hand-off
 * timeout, see dh_surface_loss).
 * Launches through one context share its scratch: issue them on one stream at a time.       */
int dh_surface_price_dev(dh_ctx* ctx, const dh_surface* s, const double* d_params, int64_t P,
                         int N, double L, double* d_out, void* stream);
int dh_surface_loss_dev(dh_ctx* ctx, const dh_surface* s, const double* d_params, int S, int N,
                        double L, double* d_sse, int32_t* d_n_bad, double* d_prices,
                        void* stream);

/* One function+gradient request per start for a host-driven optimizer (the SciPy driver):
 * x0[S][13] unconstrained -> f[S] = compute_loss(x0) (lbfgs_calibrator.py:118-177), g[S][13] =
 * SciPy's 2-point forward difference (loss(x0 + h_i e_i) - f) / ((x0_i + h_i) - x0_i) with
 * h = 1e-8 (scipy/optimize/_numdiff.py:498-511,592-596), low[S] = the smallest valid loss of the
 * 14 points (best_loss, :171-172).  The 14 x S records are formed on the host and priced in one
 * request (dh_surface_loss).
 * model: [2][S][13] model params (transform_params, lbfgs_calibrator.py:62-87) of x0 (block 0)
 * and of x0 + h (block 1, h as above), formed by the caller with the same exp / tanh the
 * reference's NumPy uses, so f equals compute_loss(x0) bit for bit; NULL = libm exp / tanh here. */
int dh_surface_fg(dh_ctx* ctx, const dh_surface* s, const double* x0, const double* model, int S,
                  double S0, double r, int N, double L, double* f, double* g, double* low);
/* The same request in two halves, so a host driver can run one group of starts' optimizer steps
 * while other groups' requests are on the device: begin forms the records into slot (0 ..
 * DH_FG_SLOTS - 1; each slot owns its pinned buffers) and enqueues the request on the context's
 * stream, then returns;
 * end waits for that slot's request and writes f, g, low as dh_surface_fg would (the same bits:
 * a start's values depend only on its own x0).  A slot holds one request at a time; requests
 * run in enqueue order; 14 S <= 1024 (larger: dh_surface_fg).                                   */
#define DH_FG_SLOTS 4
int dh_surface_fg_begin(dh_ctx* ctx, const dh_surface* s, const double* x0, const double* model,
                        int S, double S0, double r, int N, double L, int slot);
/* end: S must be the start count the slot's request was enqueued with, and s its surface
 * (DH_E_ARG otherwise, the request stays in flight): f[S], g[S][13], low[S] are written.
 * cancel: wait for the slot's request (if any) and discard it, so the slot is free again (a
 * driver unwinding from an error); no-op on an idle slot.                                      */
int dh_surface_fg_end(dh_ctx* ctx, const dh_surface* s, int slot, int S, double* f, double* g,
                      double* low);
int dh_surface_fg_cancel(dh_ctx* ctx, int slot);

/* ---- device-resident multi-start L-BFGS-B ------------------------------------------------- */
/* Runs S independent L-BFGS-B starts (no bounds) on the surface's calibration loss without a
 * host round trip per iteration.  Replaces the per-start
 *   minimize(compute_loss, x0, method='L-BFGS-B', options={maxiter, ftol, gtol})
 * of DoubleHestonJumpCalibrator.calibrate (lbfgs_calibrator.py:259-269, SciPy's 2-point
 * forward-difference gradient at h = 1e-8, scipy/optimize/_numdiff.py:498-511,592-596).
 * Each iteration is one loss launch over the 14 x (live starts) points of every live start's
 * pending function+gradient request, then one step launch (one wave per start) that forms
 * loss = n_bad ? 1e10 : sse / M + Feller penalty and the FD gradient, advances the start's
 * L-BFGS-B state (csrc/dh_lbfgs.h) to its next request and writes that request's 14 param
 * records.  The host only checks for finished starts every `chunk` iterations.
 * x0: [S][13] unconstrained start points (lbfgs_calibrator.py:62-87 transform), S0 / r the
 * spot and rate of every record.  Results per start in out[S].                                */
typedef struct {
    int32_t maxiter;             /* NEW_X iterations (minimize's maxiter) */
    int32_t maxfun;              /* stop when requests (x0 included) > maxfun at a NEW_X */
    int32_t maxls;               /* line-search trial points (SciPy default 20) */
    int32_t chunk;               /* iterations enqueued between host checks (<= 0: 8) */
    double ftol;                 /* relative-reduction test: factr = ftol / eps */
    double gtol;                 /* projected-gradient test */
} dh_lb_options;

typedef struct {
    double x[13];                /* final x (restored start of the last line search if ABNORMAL) */
    double fun;                  /* f of the LAST evaluated point, as SciPy's OptimizeResult.fun */
    double best_loss;            /* smallest valid loss this start evaluated (:171-172) */
    double t_done;               /* seconds from the call until the host saw the start finish */
    int32_t nit;                 /* NEW_X iterations */
    int32_t nfev;                /* function+gradient requests, x0 included */
    int32_t task;                /* SciPy status*1000 + message: 4401/4402 CONVERGENCE,
                                    5502/5504 STOP, 8000 ABNORMAL, 7000 ERROR (line search) */
    int32_t warnflag;            /* 0 converged, 1 maxfun/maxiter, 2 other */
    int32_t n_calls;             /* loss evaluations (14 per request) */
    int32_t pad;
} dh_lb_result;

int dh_calibrate_lbfgs(dh_ctx* ctx, const dh_surface* s, const double* x0, int S, double S0,
                       double r, int N, double L, const dh_lb_options* opt, dh_lb_result* out,
                       int32_t* n_launches);
/* Diagnostics (tests): with cap > 0, dh_calibrate_lbfgs records every consumed request as 40
 * doubles [start, request number, f, x[13], g[13], 3 spare (dh_calibrate_lbfgs_batch: the
 * start's market, then 2 spare), 6 phase stamps of the step kernel
 * (DH_STAMPS build only, else 0) 0 0] (order across starts arbitrary); dh_ctx_read_lb_trace
 * copies up to cap records of the last call and sets *n to the count.                         */
int dh_ctx_set_lb_trace(dh_ctx* ctx, int64_t cap);
int dh_ctx_read_lb_trace(dh_ctx* ctx, double* out, int64_t cap, int64_t* n);

/* ---- one-shot forms (SURVEY.md 8(b)'s proposed exports; a surface is built per call) ------- */
/* out[p*M + m] = price of option m (K, T, is_call) under params[p] (13 model params, S0, r, q):
 * dh_surface_create + dh_surface_price + dh_surface_destroy.  Replaces P x M calls of
 * DoubleHeston(...).pricing(N) (double_heston.py:160-192).                                      */
int dh_price_batch(dh_ctx* ctx, const double* params, int64_t P, const double* K, const double* T,
                   const int8_t* is_call, int M, int N, double L, double* out);
/* compute_loss (lbfgs_calibrator.py:118-177) of S unconstrained points x[S][13], all on the
 * device: transform (exp / tanh / identity, :62-87), Feller penalty (:113-116), the surface's
 * loss terms, then loss[s] = n_invalid[s] ? 1e10 : sse / M + penalty (:152-166).  M == 0 gives
 * NaN (np.mean([]), :163); a zero market price gives inf.  One FD request = the 14 points
 * x, x + h_i e_i.                                                                               */
int dh_loss_batch(dh_ctx* ctx, const double* x, int S, const double* K, const double* T,
                  const int8_t* is_call, const double* mkt, int M, double S0, double r, int N,
                  double L, double* loss, int32_t* n_invalid);

/* ---- generator batch path: host RNG ------------------------------------------------------ */
/* Draws n_samples samples of generate_synthetic_calibrations (synthetic_generator.py:98-141)
 * from NumPy's legacy RandomState stream, bit for bit, on the host (no device work): per sample
 * 13 uniform(lo[j], hi[j]) (:100-102), the AR(1) blend alpha * prev + (1 - alpha) * draw for
 * i > 0 (:105-109), spot *= 1 + normal(ret_mu, ret_sigma) for i > 0 (:112-116, spot0 at i = 0),
 * then n_opt normal(0, noise_sigma) (:141).  The state is NumPy's get_state() tuple: mt_key[624],
 * mt_pos, has_gauss, cached_gauss -- read and advanced in place (set it back with set_state).
 * Outputs: params [n][13], spots [n], noise [n][n_opt].  The draws replace the reference's
 * per-sample Python loop; pricing then runs on the GPU (dh_surface_price, STRIKE_PCT_SPOT).      */
int dh_gen_draw(uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss, double* cached_gauss,
                int64_t n_samples, const double* lo, const double* hi, int n_opt, double alpha,
                double spot0, double ret_mu, double ret_sigma, double noise_sigma, double* params,
                double* spots, double* noise);
/* dh_gen_draw that also publishes its progress: *done (required) is stored, with release order,
 * as the count of leading samples whose params, spot and noise rows are complete (after every
 * chunk of 65,536 samples, and n_samples at the end), so a caller thread can price finished rows
 * while the draw runs.  Same draws, same bits, same final RNG state as dh_gen_draw.           */
int dh_gen_draw_progress(uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss,
                         double* cached_gauss, int64_t n_samples, const double* lo,
                         const double* hi, int n_opt, double alpha, double spot0, double ret_mu,
                         double ret_sigma, double noise_sigma, double* params, double* spots,
                         double* noise, int64_t* done);
/* ---- sharded draw (generate_sharded): one rank locates, every rank draws its own samples -- */
/* The serial part of the draw only (the MT19937 twister, the polar method's acceptance bitmaps
 * and the walk over them; no sample is drawn): for each of n_starts sample indices starts[]
 * (non-decreasing, <= n_samples) the generator's state at that sample's first draw, as
 * DH_GEN_LOC_WORDS doubles at loc[j * DH_GEN_LOC_WORDS]: key[624], pos, has_gauss, cached gauss
 * (np.random.get_state()'s fields).  The state arguments are advanced in place to where
 * dh_gen_draw of n_samples would leave them.  Replaces the stream positions the reference's
 * per-sample loop reaches (synthetic_generator.py:98-141).                                      */
#define DH_GEN_LOC_WORDS 627
int dh_gen_locate(uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss, double* cached_gauss,
                  int64_t n_samples, int n_opt, const int64_t* starts, int64_t n_starts,
                  double* loc);
/* Draw samples [starts[0], i_end) from located states: chunk j = [starts[j], starts[j + 1]) (the
 * last ends at i_end) from loc[j], chunks in parallel on the host's threads.  Rows relative to
 * starts[0]: params [n][13] the raw uniforms (:100-102, before the AR(1) blend), rets [n] the spot
 * return's normal(0.0003, 0.01) draw (:112-116; sample 0 has none), noise [n][n_opt] (:141).   */
int dh_gen_draw_located(const double* loc, const int64_t* starts, int64_t n_starts,
                        int64_t i_end, const double* lo, const double* hi, int n_opt,
                        double ret_mu, double ret_sigma, double noise_sigma, double* params,
                        double* rets, double* noise);
/* The values that carry across samples, over rows [0, n) = samples [i0, i0 + n): the AR(1) blend
 * params[i] = alpha params[i - 1] + (1 - alpha) raw[i] (:105-109) and the spot walk spot[i] =
 * spot[i - 1] (1 + ret[i]) (:112-116), in place (spots: rets in, spots out).  carry [14] holds
 * the previous sample's blended params and spot (ignored when i0 = 0: spot0 starts the walk)
 * and receives this block's last row: the 14 doubles one rank passes to the next.            */
int dh_gen_sweep(double* params, double* spots, int64_t i0, int64_t n, double alpha, double spot0,
                 double* carry);
/* Samples drawn by this process's draw calls so far (instrumentation of the sharded draw).    */
int dh_gen_drawn_samples(int64_t* count);
/* The generator's trading dates (synthetic_generator.py:59-67: weekdays from a Monday, here
 * 2022-01-03 = day 18995 since 1970-01-01, as 'YYYY-MM-DD'): sample i's date as 10 UCS-4 code
 * points at out[10 i] (a NumPy '<U10' array's buffer).  DH_E_ARG past year 9999.             */
int dh_gen_dates(int64_t first_day, int64_t n, uint32_t* out);

/* The generator's host arithmetic after pricing (synthetic_generator.py:141-157), per sample i
 * and option j of [n_samples][n_opt] row-major arrays: market = model + noise * model, loss[i] =
 * mean_j ((model - market) / market)^2 formed as np.mean forms it (bit for bit), strikes =
 * (k_rel[j] * spots[i]) / 100.  Host code (threads), no device work.                      */
int dh_gen_assemble(const double* model, const double* noise, const double* spots,
                    const double* k_rel, int64_t n_samples, int n_opt, double* market,
                    double* loss, double* strikes);

/* The generator's whole batch path on the device (replaces synthetic_generator.py:98-157's
 * per-sample loop).  The host keeps only the serial part of NumPy's legacy stream
 * -- the MT19937 twister and the walk over the polar acceptances, which give each sample its
 * first double -- on a team of threads; per 65,536-sample chunk the device re-creates the
 * stream's words, draws each sample's uniforms and normals (glibc's log restated), runs the AR(1)
 * blend (alpha; 1 - alpha as the reference forms it) and the spot walk from spot0 (returns
 * normal(ret_mu, ret_sigma)), prices the grid's options (`grid`: strikes in percent of each
 * sample's spot, DH_STRIKE_PCT_SPOT; rate r, COS N, L) and forms market = model + normal(0,
 * noise_sigma) * model, the per-sample loss (np.mean's bits) and strikes = k_rel[j] spot / 100.
 * Every value is the reference loop's bit for bit; the RNG state arguments (np.random.get_state()
 * fields) are advanced in place to where that loop leaves them.  Host outputs (page-locked ones,
 * dh_host_alloc, move by DMA): params [n][13], spots [n], market, model, strikes [n][M], loss [n],
 * and dates [n][10] UCS-4 ('YYYY-MM-DD' weekdays from day first_day, dh_gen_dates) unless null.
 * stats [8] (optional): seconds from the call's start at which the twister and the walk ended,
 * the first chunk was issued and the call returned; AR(1) segments re-run serially; key blocks
 * bounded / used; chunks.  1 <= M <= 128.                                                        */
int dh_gen_device(dh_ctx* ctx, const dh_surface* grid, uint32_t* mt_key, int32_t* mt_pos,
                  int32_t* has_gauss, double* cached_gauss, int64_t n_samples, const double* lo,
                  const double* hi, double alpha, double spot0, double ret_mu, double ret_sigma,
                  double noise_sigma, double r, int N, double L, const double* k_rel,
                  int64_t first_day, double* params, double* spots, double* market,
                  double* model, double* loss, double* strikes, uint32_t* dates, double* stats);
/* The device's restatement of glibc's log (the legacy gauss's, dh_gen_device) over x[n]: its
 * GPU test against libm.                                                                         */
int dh_gen_log(dh_ctx* ctx, const double* x, int64_t n, double* out);
/* Test support: one of the fp64 elementary functions of csrc/dh_device.h over arrays, one GPU lane
 * per element, for its test against a high-precision truth (csrc/dh_math_probe.h, which also fixes
 * the layout; tests/test_gpu_math.py).  fn: 0 dsincos, 1 dsincos_t, 2 dexp, 3 dexp_nonpos,
 * 4 dexp_t, 5 dexp_t_nonpos, 6 dlog, 7 dlog_t, 8 datan2, 9 datan2_t, 10 drcp, 11 dsqrt_rsqrt,
 * 12 dsqrt_rsqrt_pos, 13 csqrt_p, 14 cdiv, 15 cdiv_rcp; any other value gives DH_E_ARG.
 * x[n]: the argument, the first argument of atan2(y, x) (its "y"), or the real part; y[n]: the
 * second argument or the imaginary part (not read by the one-argument functions, may be NULL).
 * cdiv and cdiv_rcp read x[2n], y[2n]: the numerator x[i] + i y[i], the divisor x[n+i] + i y[n+i].
 * out0[n], out1[n]: sin / cos, sqrt / rsqrt, re / im; a single result in out0 (out1 = 0).
 * Host pointers, synchronous; n == 0 is a no-op.                                                  */
int dh_math_probe(dh_ctx* ctx, int fn, const double* x, const double* y, int64_t n, double* out0,
                  double* out1);
/* Page-locked host memory from a process-wide cache (hipHostMalloc; a freed block serves the next
 * request of up to 1.25x its size): the generator's output arrays.  dh_host_cache_trim releases
 * the cached blocks.                                                                             */
int dh_host_alloc(size_t bytes, void** out);
int dh_host_free(void* p);
int dh_host_cache_trim(void);

/* ---- paired pricing: option i under param set i ------------------------------------------- */
/* out[i] = price of (K[i], T[i], is_call[i]) under params[i]; replaces a loop of single
 * DoubleHeston(...).pricing(N) calls (double_heston.py:160-192).                              */
int dh_price_pairs(dh_ctx* ctx, const double* params, const double* K, const double* T,
                   const int8_t* is_call, int64_t P, int N, double L, double* out);

/* ---- analytic Greeks of the COS price (csrc/dh_greeks.h) --------------------- */
/* Replaces nothing in the reference (it has no sensitivities): it replaces bumping and repricing,
 * nine pricings for the five sensitivities below by central differences.  With xK = log(K / S0),
 * [a, b] = truncationRange(L), u_k = k pi / (b - a), w_k = phi(u_k) e^{-i u_k a}, the price is
 *     e^{-rT} sum'_{k < N} Re(w_k) V_k,  V_k = +-(2 / (b - a)) (S0 chi_k - K psi_k)
 * (double_heston.py:160-192; chi_k, psi_k over [xK, b] and + for a call, over [a, xK] and - for a
 * put), and the planes are the partial derivatives of this series at FIXED [a, b] and fixed
 * absolute strike (a DH_STRIKE_PCT_SPOT strike is first resolved to K_relative * S0 / 100.0):
 *     DH_GREEK_PRICE       the series itself
 *     DH_GREEK_DELTA       d / dS0:     V_k -> +-(2 / (b - a)) chi_k
 *     DH_GREEK_GAMMA       d2 / dS0^2:  V_k -> (2 / (b - a)) cos(u_k (xK - a)) K / S0^2
 *     DH_GREEK_DUAL_DELTA  d / dK:      V_k -> -+(2 / (b - a)) psi_k
 *     DH_GREEK_VEGA1       d / dv01:    w_k -> w_k B1(u_k)   (B_j: the CF's variance-factor
 *     DH_GREEK_VEGA2       d / dv02:    w_k -> w_k B2(u_k)    coefficients; per unit of variance)
 * They do NOT differentiate through the cumulant range or through the log(K / S0) -+ 0.1 clamp
 * (double_heston.py:131-137): the difference from a total derivative is of the size of the series'
 * truncation error where the clamp is inactive and is not small where it is active.
 * price = S0 delta + K dual_delta holds to rounding.  Every term k < N is summed (the price path's
 * adaptive tail cut is not applied: gamma's coefficients do not decay), every sum in a fixed order:
 * the same call gives the same bits, and an option's values do not depend on what shares its call.
 * q is supported as for prices.  Non-finite parameters give NaN in every plane, as prices do.
 * DH_E_ARG, before any device work and naming the argument in dh_last_error(): N outside
 * [1, DH_MAX_N]; P (n) < 1; L not finite or <= 0; a NULL pointer.                               */
enum { DH_GREEK_PRICE, DH_GREEK_DELTA, DH_GREEK_GAMMA, DH_GREEK_DUAL_DELTA, DH_GREEK_VEGA1,
       DH_GREEK_VEGA2, DH_N_GREEKS };
/* out[(g * P + p) * M + m], g a DH_GREEK_* plane, m in the caller's option order as in
 * dh_surface_price.  Host arrays, synchronous.                                                  */
int dh_surface_greeks(dh_ctx* ctx, const dh_surface* s, const double* params, int64_t P, int N,
                      double L, double* out);
/* The same over device pointers: enqueued on `stream` (hipStream_t; NULL = the context's) without
 * synchronisation, no allocation; the same bits as dh_surface_greeks.                           */
int dh_surface_greeks_dev(dh_ctx* ctx, const dh_surface* s, const double* d_params, int64_t P,
                          int N, double L, double* d_out, void* stream);
/* Option i under param set i, the counterpart of dh_price_pairs: out[g * n + i].  Host arrays,
 * synchronous; the bits dh_surface_greeks gives the same (set, option) pair.                    */
int dh_greeks_pairs(dh_ctx* ctx, const double* params, const double* K, const double* T,
                    const int8_t* is_call, int64_t n, int N, double L, double* out);

/* ---- the full Greeks: maturity, rate, dual gamma, local variance (csrc/dh_greeks_full.h,
 *      DESIGN.md 3.24) ------------------------------------------------------------------------- */
/* The six planes above, bit for bit, and four more from the same pass, again partial derivatives of
 * the series at FIXED [a, b] (fixed u_k) and fixed absolute strike:
 *     DH_GREEK_DPRICE_DT   d / dT = -r price + e^{-rT} sum'_k Re(w_k G_k) V_k, G = d log phi / d tau
 *                          (theta, the calendar decay per year, is its negative)
 *     DH_GREEK_RHO         d / dr = -T price + e^{-rT} sum'_k (-u_k T Im w_k) V_k
 *                          (d / dq = -(rho + T price))
 *     DH_GREEK_DUAL_GAMMA  d2 / dK^2: V_k -> (2 / (b - a)) cos(u_k (xK - a)) / K; K^2 dual_gamma =
 *                          S0^2 gamma; e^{rT} dual_gamma is the risk-neutral density of S_T at K
 *     DH_GREEK_LOCAL_VAR   Dupire's local variance (with jumps: the model's Markovian projection),
 *                          formed in fp64 without contraction from the planes of the same option as
 *                              num = (dprice_dT + ((r - q) * K) * dual_delta) + q * price
 *                              den = (0.5 * (K * K)) * dual_gamma
 *                              local_var = num / den
 *                          where those four planes are finite and den > 0, NaN otherwise; not
 *                          clipped where negative.  The same for a call and a put.
 * dprice_dT is not the total derivative in T: [a, b] moves with T and is held here, a difference
 * of the size of the series' truncation error where the clamp is inactive.
 * Arguments, refusals, layout (out[(g * P + p) * M + m], g < DH_N_GREEKS_FULL; pairs: out[g * n +
 * i]) and reproducibility are those of the three calls above.                                    */
enum { DH_GREEK_DPRICE_DT = 6, DH_GREEK_RHO = 7, DH_GREEK_DUAL_GAMMA = 8, DH_GREEK_LOCAL_VAR = 9,
       DH_N_GREEKS_FULL = 10 };
int dh_surface_greeks_full(dh_ctx* ctx, const dh_surface* s, const double* params, int64_t P,
                           int N, double L, double* out);
int dh_surface_greeks_full_dev(dh_ctx* ctx, const dh_surface* s, const double* d_params, int64_t P,
                               int N, double L, double* d_out, void* stream);
int dh_greeks_full_pairs(dh_ctx* ctx, const double* params, const double* K, const double* T,
                         const int8_t* is_call, int64_t n, int N, double L, double* out);

/* ---- analytic parameter sensitivities and the calibration gradient (csrc/dh_param_grad.h,
 * DESIGN.md 3.18) --------------------------------------------------------------------------- */
/* Replaces nothing in the reference (it has no sensitivities and hands SciPy no gradient): it
 * replaces bumping and repricing, the fourteen pricings of a forward-difference request
 * (dh_surface_fg).  In the Greeks' notation, for a model parameter p at FIXED [a, b]
 *     d price / d p = e^{-rT} sum'_{k < N} Re(w_k D_p(u_k)) V_k,   D_p = d log phi / d p
 * (the closed forms of the thirteen D_p: csrc/dh_param_grad.h).  Like the Greeks the planes do NOT
 * differentiate through the cumulant range or its log(K / S0) -+ 0.1 clamp.  Plane 0 is the price,
 * planes 1..13 the parameters in the record's order: v1_0 kappa1 theta1 sigma1 rho1 v2_0 kappa2
 * theta2 sigma2 rho2 lambda_j mu_j sigma_j.  Planes 0, 1 and 6 are the same series as
 * dh_surface_greeks' price and vegas and agree with them to rounding (1e-13 at S0 = 100), not bit
 * for bit.  Every term k < N is summed in a fixed order: the same call
 * gives the same bits, and a set's values do not depend on what shares its call.  Non-finite
 * parameters give NaN in every plane.
 * DH_E_ARG, before any device work and naming the argument in dh_last_error(): N outside
 * [1, DH_PARAM_GRAD_MAX_N] (sixteen doubles per term in one CU's LDS); P (n, S) < 1; L not finite
 * or <= 0; a NULL pointer.                                                                       */
enum { DH_PARAM_GRAD_MAX_N = 1024, DH_N_PARAM_SENS = 14 };
/* out[(i * P + p) * M + m], i = 0 the price and 1..13 the parameters, m in the caller's option
 * order as in dh_surface_price.  Host arrays, synchronous.                                       */
int dh_surface_param_sens(dh_ctx* ctx, const dh_surface* s, const double* params, int64_t P, int N,
                          double L, double* out);
/* The same over device pointers: enqueued on `stream` (hipStream_t; NULL = the context's) without
 * synchronisation, no allocation; the same bits as dh_surface_param_sens.                        */
int dh_surface_param_sens_dev(dh_ctx* ctx, const dh_surface* s, const double* d_params, int64_t P,
                              int N, double L, double* d_out, void* stream);
/* Option i under param set i: out[i_plane * n + i].  Host arrays, synchronous; the bits
 * dh_surface_param_sens gives the same (set, option) pair.                                       */
int dh_param_sens_pairs(dh_ctx* ctx, const double* params, const double* K, const double* T,
                        const int8_t* is_call, int64_t n, int N, double L, double* out);
/* The price objective (compute_loss, lbfgs_calibrator.py:118-177) of S unconstrained points
 * x[S][13] against the surface's market prices, with its exact gradient in x, reduced on the
 * device in a fixed order (one wave per set):
 *     f[s] = sse / M + Feller,
 *     g[s][i] = (2 / M) sum_m ((p_m - mkt_m) / mkt_m^2) dp_m/dtheta_i dtheta_i/dx_i + dFeller/dx_i
 * with dtheta/dx = theta (exp-mapped parameters), 1 - rho^2 (the two correlations), 1 (mu_j), and
 * the Feller term 1000 max(0, sigma^2 - 2 kappa theta) per factor differentiated where its slack
 * is strictly positive (+2000 sigma^2 for sigma, -2000 kappa theta for each of kappa and theta),
 * zero otherwise: on the kink itself this differs from dh_surface_fg's forward quotient.  A set
 * with an invalid price (bad[s] > 0: NaN, +-inf or <= 0) gets f = 1e10 and g = 0, what the
 * quotient of the constant 1e10 gives.  S0, r, N, L as in dh_surface_fg (q = 0).  Host arrays,
 * synchronous.  DH_E_ARG also for a surface without market prices or options, and S0 or r not
 * finite.                                                                                        */
int dh_surface_loss_grad(dh_ctx* ctx, const dh_surface* s, const double* x, int S, double S0,
                         double r, int N, double L, double* f, double* g, int32_t* bad);
/* The same over device pointers, enqueued on `stream`; the same bits.  Its records and the
 * [14][S][M] planes live in the context's one grow-only scratch buffer, so:
 *   - ONE request in flight per context: a second dh_surface_loss_grad_dev (or the host form) on
 *     the same context may be issued only on the same stream, or after the first has completed;
 *     requests that are to overlap take a context each (dh_ctx_create on the same device);
 *   - a request larger (S x M) than any earlier one on this context grows the buffer with hipFree
 *     / hipMalloc, which synchronises the device and cannot be captured into a graph.  A request
 *     no larger than an earlier one allocates nothing and does not synchronise: issue the largest
 *     request once before capturing or timing.                                                   */
int dh_surface_loss_grad_dev(dh_ctx* ctx, const dh_surface* s, const double* d_x, int S, double S0,
                             double r, int N, double L, double* d_f, double* d_g, int32_t* d_bad,
                             void* stream);
/* The same against a market row per set: set s of x[S][13] is priced under
 * spot[row[s]] and rate[row[s]] (q = 0) and held to the market prices mkt[row[s]][M], the caller's
 * option order, of mkt [B][M].  Three stages: records and Feller penalties from x (dh_surface_fg's
 * transform, each set's spot and rate from its row), the parameter planes, and a reduction of one
 * wave per set -- lane l adds the surface's sorted options l, l + 64, ... uncontracted from 0.0,
 * then the xor butterfly over the 64 lanes -- with dh_surface_loss_grad's f, g and bad, its invalid
 * sets (f = 1e10, g = 0) and its one-sided Feller derivative.  A set's f and g depend on nothing
 * but its own x and market row: not on S, B or the set's place in the call; with B = 1 and the
 * surface's own market prices, spot and rate they are dh_surface_loss_grad's bits.  The surface
 * needs no market prices of its own.  Host arrays, synchronous.  DH_E_ARG as dh_surface_loss_grad
 * (N outside [1, DH_PARAM_GRAD_MAX_N], S < 1, L, an empty surface, a NULL pointer) and as
 * dh_surface_loss_rows: B <= 0, a row outside [0, B), a spot that is not finite or not > 0, a rate
 * that is not finite.                                                                            */
int dh_surface_loss_grad_rows(dh_ctx* ctx, const dh_surface* s, const double* x, const double* mkt,
                              const double* spot, const double* rate, const int32_t* row, int S,
                              int B, int N, double L, double* f, double* g, int32_t* bad);
/* The same over device pointers, enqueued on `stream`; the same bits.  d_mkt [B][M], d_spot [B],
 * d_rate [B], d_row [S] with every row in [0, B) and every spot and rate valid (the caller's
 * promise).  Scratch, the one request in flight per context and the growth rule are
 * dh_surface_loss_grad_dev's.                                                                    */
int dh_surface_loss_grad_rows_dev(dh_ctx* ctx, const dh_surface* s, const double* d_x,
                                  const double* d_mkt, const double* d_spot, const double* d_rate,
                                  const int32_t* d_row, int S, int N, double L, double* d_f,
                                  double* d_g, int32_t* d_bad, void* stream);

/* ---- Black-Scholes implied volatility ----------------------------------------------------- */
/* sigma[i] = the volatility whose Black-Scholes price of (S0[i], K[i], T[i], r[i], q[i],
 * is_call[i]) is price[i]; every array has n entries (structure of arrays), one GPU lane per quote.
 * Replaces nothing in the reference (it has no implied-vol code; its only trace is the
 * implied_var start guess, lbfgs_calibrator.py:220-222): it replaces the per-option host
 * root-finder a user of the price outputs runs.  With the bounds formed in fp64 as written,
 *   call: lower = max(S0 e^{-qT} - K e^{-rT}, 0), upper = S0 e^{-qT}
 *   put:  lower = max(K e^{-rT} - S0 e^{-qT}, 0), upper = K e^{-rT}
 * the result is 0.0 where price == lower, and NaN where price < lower, price >= upper, price is
 * not finite, S0 <= 0, K <= 0, T <= 0 or any input is NaN or infinite.  NaN is the only failure
 * signal (a numeric failure is not an error).  Every quote is solved within a fixed number of
 * steps whatever its value (csrc/dh_iv.h).
 * Host pointers, synchronous; n == 0 is a no-op.                                               */
int dh_implied_vol(dh_ctx* ctx, const double* price, const double* S0, const double* K,
                   const double* T, const double* r, const double* q, const int8_t* is_call,
                   int64_t n, double* sigma);
/* The same over device pointers: one launch enqueued on `stream` (hipStream_t; NULL = the
 * context's stream).  No synchronisation, no allocation.                                       */
int dh_implied_vol_dev(dh_ctx* ctx, const double* d_price, const double* d_S0, const double* d_K,
                       const double* d_T, const double* d_r, const double* d_q,
                       const int8_t* d_is_call, int64_t n, double* d_sigma, void* stream);
/* Model vols of a surface: prices it as dh_surface_price does (the same kernels, the same bits),
 * then inverts every price on the device, without a host round trip: iv[p*M + m], m in the
 * caller's original option order, from S0, r, q of param record p (slots 13..15) and K, T,
 * is_call of option m (DH_STRIKE_PCT_SPOT: the strike K_relative * S0 / 100.0 the pricing forms).
 * prices: optional [P][M] output of what dh_surface_price returns (NULL to skip).               */
int dh_surface_implied_vol(dh_ctx* ctx, const dh_surface* s, const double* params, int64_t P,
                           int N, double L, double* iv, double* prices);

/* ---- calibration objective in implied-vol space (csrc/dh_iv_loss.h) --------- */
/* Replaces nothing in the reference (its only objective is the relative price error of
 * dh_surface_loss); it replaces pulling dh_surface_implied_vol's [S][M] vols to the host and
 * summing them there on every request of a vol-space fit.
 * Market vols of the surface: mkt_iv[M] and weight[M] (host arrays, the caller's option order;
 * weight NULL = every weight 1), copied to the device; a second call replaces the first's data.
 * DH_E_ARG if a weight is negative or not finite, if the weights sum to zero, or if mkt_iv[m] is
 * negative or not finite where weight[m] > 0 (where the weight is 0 it may hold anything).      */
int dh_surface_set_iv_market(dh_surface* s, const double* mkt_iv, const double* weight);
/* The reduction stage alone, over prices already on the device: d_prices [S][M] as
 * dh_surface_price_dev writes them (the caller's option order), d_params the records they were
 * priced under.  Per param set s and option m, with S0, r, q from the record, K, T, is_call of the
 * option (DH_STRIKE_PCT_SPOT: the strike dh_surface_implied_vol forms):
 *   bad      price NaN, +-inf or <= 0 (dh_surface_loss's rule), or a vol that does not exist
 *            (price >= upper, T <= 0, legs out of range: dh_implied_vol's NaN)
 *   v        dh_implied_vol's sigma of the price (the same device function, the same bits); 0.0
 *            where price < lower -- the vol's continuous extension, so that a deep in-the-money
 *            model price a rounding below intrinsic does not turn the loss into 1e10
 *   iv[s*M + m] = v as used: 0.0 where clamped, NaN where bad; every option, whatever its weight
 *                 (d_iv NULL to skip)
 *   sse[s]   = sum of weight[m] (v - mkt_iv[m])^2 over options with weight[m] > 0 that are not bad
 *   n_bad[s] = #{m : weight[m] > 0 and option m is bad}
 * The host forms loss = n_bad ? 1e10 : sse / sum(weight) + feller.  sse[s] is summed in an order
 * fixed by the surface alone and depends on nothing but record s: the same bits in any request,
 * at any place in it, on any stream.  Enqueues on `stream` (NULL = the context's); no
 * synchronisation, no allocation after warm-up.  DH_E_ARG on a surface without market vols.    */
int dh_surface_iv_sse_dev(dh_ctx* ctx, const dh_surface* s, const double* d_params,
                          const double* d_prices, int S, double* d_sse, int32_t* d_n_bad,
                          double* d_iv, void* stream);
/* Price, then reduce, on one stream: dh_surface_price_dev into d_prices (NULL: context scratch),
 * then the stage above (d_iv NULL to skip the vols).                                            */
int dh_surface_loss_iv_dev(dh_ctx* ctx, const dh_surface* s, const double* d_params, int S, int N,
                           double L, double* d_sse, int32_t* d_n_bad, double* d_prices,
                           double* d_iv, void* stream);
/* The host-pointer form, synchronous as dh_surface_loss: params [S][16] in, sse [S], n_bad [S] and
 * the optional prices [S][M], iv [S][M] out (NULL to skip either).                              */
int dh_surface_loss_iv(dh_ctx* ctx, const dh_surface* s, const double* params, int S, int N,
                       double L, double* sse, int32_t* n_bad, double* prices, double* iv);

/* ---- many markets on one option grid (csrc/dh_loss_rows.h) ------------------- */
/* Replaces the Python loop DoubleHestonJumpCalibrator(spot_b, r_b, options_b).calibrate() over the
 * rows of the generator's (market [n][15], spots [n]) arrays (lbfgs_calibrator.py:179-299 once
 * per row).  B markets share the surface's options (its strike mode forms each record's strikes
 * from the record's own spot, or keeps the listed ones); the surface needs no market prices.
 * The reduction stage alone, over prices already on the device: d_prices [S][M] as
 * dh_surface_price_dev writes them, d_mkt [B][M] market prices in the caller's option order,
 * d_row [S] the market row of each param set (in [0, B); the caller's promise).  Per set s, with
 * m = d_mkt[d_row[s]*M + .]:
 *   sse[s]   = sum of ((p - m) / m)^2 over the M options
 *   n_bad[s] = #{p NaN, +-inf or <= 0}
 * dh_surface_loss's rules (a zero market price gives inf, a NaN one NaN).  One wave per set: lane
 * l adds options l, l + 64, ... in order from 0.0, then the xor butterfly over the 64 lanes
 * (offsets 1, 2, 4, 8, 16, 32); nothing is contracted.  sse[s] depends on nothing but set s's
 * prices and its market row: the same bits in any request, at any place in it.  Enqueues on
 * `stream` (NULL = the context's); no synchronisation, no allocation.                           */
int dh_surface_loss_rows_dev(dh_ctx* ctx, const dh_surface* s, const double* d_prices,
                             const double* d_mkt, const int32_t* d_row, int S, double* d_sse,
                             int32_t* d_n_bad, void* stream);
/* The host-pointer form, synchronous: params [S][16] are priced as dh_surface_price prices them
 * (the same kernels), then reduced against mkt [B][M] by row [S]; sse [S], n_bad [S] and the
 * optional prices [S][M] out.  DH_E_ARG for a row outside [0, B).                                */
int dh_surface_loss_rows(dh_ctx* ctx, const dh_surface* s, const double* params, const double* mkt,
                         const int32_t* row, int S, int B, int N, double L, double* sse,
                         int32_t* n_bad, double* prices);
/* dh_calibrate_lbfgs over many markets at once: start i fits market market_of[i], whose market
 * prices are mkt[market_of[i]][M], spot spot[market_of[i]] and rate rate[market_of[i]].  Every
 * iteration is one price launch over the 14 x (live starts) records, the reduction above (each
 * slot's row taken from its start's market) and one step launch, which writes each next request's
 * records with that start's spot and rate.  Options, results, chunked enqueue, compaction and the
 * trace (whose first spare double holds the market index) are dh_calibrate_lbfgs's.  A start's
 * requests and results depend on nothing but its own x0 and market: not on B, S, the order of the
 * markets or the chunk size.  DH_E_ARG for M == 0, B <= 0 with S > 0, a market_of entry outside
 * [0, B), a spot that is not finite or not > 0, a rate that is not finite.                      */
int dh_calibrate_lbfgs_batch(dh_ctx* ctx, const dh_surface* s, const double* mkt,
                             const double* spot, const double* rate, int B, const double* x0,
                             const int32_t* market_of, int S, int N, double L,
                             const dh_lb_options* opt, dh_lb_result* out, int32_t* n_launches);

/* ---- many markets on one grid, in implied-vol space (csrc/dh_loss_rows.h) ----- */
/* Replaces the loop DoubleHestonJumpCalibrator(spot_b, r_b, options_b, objective="iv").calibrate(
 * driver="scipy") over the markets: the vol-space objective of dh_surface_loss_iv, against a
 * market row per param set as dh_surface_loss_rows has it.
 * The reduction stage alone, over prices already on the device: d_prices [S][M] as
 * dh_surface_price_dev writes them, d_params the records they were priced under (S0, r, q of set
 * s from its record, so each set inverts with its own market's spot), d_mkt_iv [B][M] market vols
 * and d_wgt [B][M] weights in the caller's option order, d_row [S] the market row of each set (in
 * [0, B); the caller's promise).  Per set s, with b = d_row[s], by dh_surface_iv_sse_dev's rules
 * (bad prices, the clamp at the lower bound, iv as used):
 *   sse[s]   = sum of w[b][m] (v - mkt_iv[b][m])^2 over options with w[b][m] > 0 that are not bad
 *   n_bad[s] = #{m : w[b][m] > 0 and option m is bad}
 *   iv[s*M + m] = v as used (d_iv NULL to skip)
 * One wave per set: lane l adds the surface's sorted options l, l + 64, ... in order from 0.0,
 * then the xor butterfly over the 64 lanes (offsets 1, 2, 4, 8, 16, 32); nothing is contracted.
 * For M <= 64 these are dh_surface_iv_sse_dev's bits for the same vols and weights.  sse[s]
 * depends on nothing but set s's record, prices and market row.  Enqueues on `stream` (NULL = the
 * context's); no synchronisation, no allocation.                                                */
int dh_surface_iv_sse_rows_dev(dh_ctx* ctx, const dh_surface* s, const double* d_params,
                               const double* d_prices, const double* d_mkt_iv, const double* d_wgt,
                               const int32_t* d_row, int S, double* d_sse, int32_t* d_n_bad,
                               double* d_iv, void* stream);
/* The host-pointer form, synchronous: params [S][16] are priced as dh_surface_price prices them,
 * then reduced against mkt_iv [B][M] and wgt [B][M] (NULL: every weight 1) by row [S]; sse [S],
 * n_bad [S] and the optional prices [S][M], iv [S][M] out.  DH_E_ARG for a row outside [0, B). */
int dh_surface_loss_iv_rows(dh_ctx* ctx, const dh_surface* s, const double* params,
                            const double* mkt_iv, const double* wgt, const int32_t* row, int S,
                            int B, int N, double L, double* sse, int32_t* n_bad, double* prices,
                            double* iv);
/* dh_calibrate_lbfgs_batch in vol space: start i fits the vols mkt_iv[market_of[i]][M] under the
 * weights wgt[market_of[i]][M] (NULL: every weight 1), loss = n_bad ? 1e10 : sse / wsum + Feller,
 * wsum the market's weight sum (formed on the host: option order, sequential, from 0.0).  Every
 * iteration is three launches: price, the reduction above, step.  Everything else is
 * dh_calibrate_lbfgs_batch's, its DH_E_ARG cases included; DH_E_ARG also for a weight that is
 * negative or not finite, a market whose weights sum to 0, and a market vol that is negative or
 * not finite at a positive weight (the message names the market and the option).               */
int dh_calibrate_lbfgs_batch_iv(dh_ctx* ctx, const dh_surface* s, const double* mkt_iv,
                                const double* wgt, const double* spot, const double* rate, int B,
                                const double* x0, const int32_t* market_of, int S, int N, double L,
                                const dh_lb_options* opt, dh_lb_result* out, int32_t* n_launches);

/* ---- many markets on one grid, with the analytic gradient (csrc/dh_lb_driver.h) */
/* dh_calibrate_lbfgs_batch with the exact gradient of dh_surface_loss_grad_rows where that driver
 * forms SciPy's forward quotient: a request is ONE point per start.  Every iteration is the
 * parameter-plane launch over one record per live start, the rows reduction into f [live] and
 * g [live][13], and one step launch, which hands (f, g) to the same L-BFGS-B state machine and
 * writes each next record with its start's spot, rate, market row and Feller penalty.  The
 * arguments, options, results, chunked enqueue, compaction and trace are
 * dh_calibrate_lbfgs_batch's; n_calls counts one loss evaluation per request (n_calls == nfev),
 * best_loss is the smallest valid f.  On the Feller kink the gradient is the one-sided rule of
 * dh_surface_loss_grad, not the forward quotient's slope, so a start on it may move where the FD
 * driver's stalls.  The planes' scratch is reserved once for all S starts before the first
 * iteration.  A start's requests and results depend on nothing but its own x0 and market: not on
 * B, S, the order of the markets or the chunk size.  DH_E_ARG as dh_calibrate_lbfgs_batch, and for
 * N outside [1, DH_PARAM_GRAD_MAX_N] or L not finite or <= 0.                                    */
int dh_calibrate_lbfgs_batch_grad(dh_ctx* ctx, const dh_surface* s, const double* mkt,
                                  const double* spot, const double* rate, int B, const double* x0,
                                  const int32_t* market_of, int S, int N, double L,
                                  const dh_lb_options* opt, dh_lb_result* out, int32_t* n_launches);

/* ---- the vol objective with its exact gradient (csrc/dh_iv_grad.h) ------------- */
/* The vol-space loss of dh_surface_loss_iv_rows and its exact gradient in the optimiser's x: the
 * model vol v_m solves BS(v_m) = P_m, so dv_m/dtheta_i = (dP_m/dtheta_i) / vega_BS(v_m), with
 * dP_m/dtheta_i the planes of dh_surface_param_sens and the vega closed-form in dh_implied_vol's
 * variables (A = S0 e^{-qT}, B = K e^{-rT}, s = v sqrt T, h = |log1p((S0-K)/K) + (r-q)T| / s, t =
 * s / 2: vega = sqrt A sqrt B sqrt T exp(-(h^2 + t^2)/2 - ln sqrt(2 pi))).
 * The reduction stage alone, the vol-space sibling of dh_surface_iv_sse_rows_dev: d_planes
 * [14][S][M] as dh_surface_param_sens_dev writes them (plane 0 the price; the caller's option
 * order), d_params [S][16] the records they were formed under, d_pen [S] each record's Feller
 * penalty, d_mkt_iv / d_wgt [B][M], d_row [S] (in [0, B); the caller's promise), d_div [S] the
 * loss divisor of each set (its market's weight sum).  Per set s, by dh_surface_iv_sse_rows_dev's
 * rules line for line (bad prices, the clamp at the lower bound, a zero weight enters nothing):
 *   sse[s], n_bad[s], iv[s*M + m]: dh_surface_iv_sse_rows_dev's, bit for bit, for d_planes' plane
 *                                  0 as its prices (d_sse, d_iv NULL to skip)
 *   f[s]    = n_bad ? 1e10 : sse / div + pen
 *   g[s][i] = n_bad ? 0 : (2 / div) sum_m c_m plane_i[m] dtheta_i/dx_i + dFeller/dx_i,
 *             c_m = w_m (v_m - mkt_iv_m) / vega_m
 * with dh_surface_loss_grad's transform and Feller expressions.  One-sided rule: an option whose
 * vol as used is 0.0 (its price at, or a rounding below, its lower bound) or whose vega is not
 * > 0 adds its residual to sse and nothing to g, as the Feller kink's flat side.  One wave per
 * set: lane l takes the surface's sorted options l, l + 64, ... from 0.0, then the xor butterfly;
 * nothing is contracted.  A set's outputs depend on nothing but its own record, planes, penalty
 * and market row.  Enqueues on `stream` (NULL = the context's); no synchronisation; may grow the
 * context's scratch by [S][M] doubles.                                                          */
int dh_surface_iv_grad_rows_dev(dh_ctx* ctx, const dh_surface* s, const double* d_planes,
                                const double* d_params, const double* d_pen,
                                const double* d_mkt_iv, const double* d_wgt, const int32_t* d_row,
                                const double* d_div, int S, double* d_f, double* d_g,
                                double* d_sse, int32_t* d_n_bad, double* d_iv, void* stream);
/* The request from x [S][13]: the records and penalties of dh_surface_loss_grad_rows_dev (set s
 * under d_spot / d_rate [d_row[s]]), dh_surface_param_sens_dev's planes, the reduction above; d_f
 * [S], d_g [S][13], d_bad [S] and the optional d_iv [S][M] out.  DH_E_ARG as
 * dh_surface_loss_grad_rows_dev.                                                                */
int dh_surface_loss_iv_grad_rows_dev(dh_ctx* ctx, const dh_surface* s, const double* d_x,
                                     const double* d_mkt_iv, const double* d_wgt,
                                     const double* d_div, const double* d_spot,
                                     const double* d_rate, const int32_t* d_row, int S, int N,
                                     double L, double* d_f, double* d_g, int32_t* d_bad,
                                     double* d_iv, void* stream);
/* The host-pointer form, synchronous: mkt_iv [B][M], wgt [B][M] (NULL: every weight 1), spot [B],
 * rate [B], row [S]; each market's weight sum is formed as dh_calibrate_lbfgs_batch_iv forms it.
 * DH_E_ARG as dh_surface_loss_grad_rows, and for that call's vol and weight cases.              */
int dh_surface_loss_iv_grad_rows(dh_ctx* ctx, const dh_surface* s, const double* x,
                                 const double* mkt_iv, const double* wgt, const double* spot,
                                 const double* rate, const int32_t* row, int S, int B, int N,
                                 double L, double* f, double* g, int32_t* bad, double* iv);
/* dh_calibrate_lbfgs_batch_iv with that gradient where it forms SciPy's forward quotient: a
 * request is ONE point per start, and every iteration is the parameter-plane launch, the
 * reduction above and dh_calibrate_lbfgs_batch_grad's step launch, unchanged.  n_calls == nfev.
 * The arguments and DH_E_ARG cases are dh_calibrate_lbfgs_batch_iv's, and
 * dh_calibrate_lbfgs_batch_grad's for N and L; isolation, the trace and the scratch as there.  */
int dh_calibrate_lbfgs_batch_iv_grad(dh_ctx* ctx, const dh_surface* s, const double* mkt_iv,
                                     const double* wgt, const double* spot, const double* rate,
                                     int B, const double* x0, const int32_t* market_of, int S,
                                     int N, double L, const dh_lb_options* opt, dh_lb_result* out,
                                     int32_t* n_launches);

/* ---- Gauss-Newton Hessian and Levenberg-Marquardt (csrc/dh_gauss_newton.h, csrc/dh_lm.h,
 *      DESIGN.md 3.21) -------------------------------------------------------------------------- */
/* dh_surface_loss_grad_rows with the Gauss-Newton Hessian of the price part of the loss in the
 * optimiser's x: the same arguments, stages, f [S], g [S][13] and bad [S] -- bit for bit -- and
 *   H[s][i][j] = (2 / M) dt_i dt_j sum_m a_im a_jm,   a_im = plane_i[m] / mkt[row[s]][m]
 * with plane_i dh_surface_param_sens's plane of parameter i and dt_i the transform's derivative
 * dtheta_i/dx_i that g uses (1 - rho^2 for the two correlations, 1 for mu_j, the parameter itself
 * otherwise), formed as ((2 / M) dt_i) dt_j times the sum.  The Feller penalty, piecewise linear in
 * its slack, enters g only.  Every sum runs in dh_surface_loss_grad_rows's order (lane l adds the
 * sorted options l, l + 64, ... from 0.0, then the xor butterfly); the 91 entries i <= j are
 * computed and mirrored, so H is exactly symmetric; a set's bits depend on nothing but its own x
 * and market row.  An invalid set (bad > 0) has f = 1e10, g = 0 and H = 0; a NaN market price gives
 * NaN.  Host arrays, synchronous.  DH_E_ARG as dh_surface_loss_grad_rows, and for a NULL H.      */
int dh_surface_gauss_newton_rows(dh_ctx* ctx, const dh_surface* s, const double* x,
                                 const double* mkt, const double* spot, const double* rate,
                                 const int32_t* row, int S, int B, int N, double L, double* f,
                                 double* g, int32_t* bad, double* H);
/* The same over device pointers, enqueued on `stream`; the same bits.  d_H [S][13][13]; the other
 * arguments, the caller's promises, the scratch and the one request in flight per context are
 * dh_surface_loss_grad_rows_dev's.                                                              */
int dh_surface_gauss_newton_rows_dev(dh_ctx* ctx, const dh_surface* s, const double* d_x,
                                     const double* d_mkt, const double* d_spot,
                                     const double* d_rate, const int32_t* d_row, int S, int N,
                                     double L, double* d_f, double* d_g, int32_t* d_bad,
                                     double* d_H, void* stream);
/* dh_lb_result.task of a dh_calibrate_lm_batch start: the two gradient and loss tolerances of
 * dh_lb_options, the step tolerance, the two budgets, a damping past its ceiling (or a NaN gradient),
 * and an invalid or NaN loss at x0.  warnflag is 0 for the first three, 1 for the budgets, 2 else. */
enum { DH_LM_GTOL = 1, DH_LM_FTOL = 2, DH_LM_XTOL = 3, DH_LM_MAXITER = 4, DH_LM_MAXFUN = 5, DH_LM_STALLED = 6, DH_LM_INVALID_X0 = 7 };
/* dh_calibrate_lbfgs_batch_grad's markets, starts, options and results under Levenberg-Marquardt
 * on that Hessian (Nielsen's damping with Marquardt scaling; csrc/dh_lm.h states the algorithm and
 * its constants).  Every iteration is the parameter-plane launch over one record per live start,
 * the reduction above into f, g and H, and one step launch that accepts or rejects each start's
 * trial point, solves (H + lambda diag(D)) delta = -g by Cholesky and writes the record of x +
 * delta with the start's spot, rate, market row and Feller penalty.  One iteration is one request:
 * nfev == n_calls counts requests (x0 included), nit accepted steps (opt->maxiter bounds nit,
 * opt->maxfun nfev; opt->gtol and opt->ftol are the gradient and loss tolerances; maxls is checked
 * and not used).  x is the last accepted point and fun its loss, so fun <= f(x0) and best_loss ==
 * fun whenever f(x0) is valid; a start whose f(x0) is 1e10 or NaN ends at once with x = x0.  task
 * is a DH_LM_* code.  The chunked enqueue, compaction and trace are dh_calibrate_lbfgs_batch's; a
 * start's requests and results depend on nothing but its own x0 and market.  DH_E_ARG as
 * dh_calibrate_lbfgs_batch_grad.                                                                */
int dh_calibrate_lm_batch(dh_ctx* ctx, const dh_surface* s, const double* mkt, const double* spot,
                          const double* rate, int B, const double* x0, const int32_t* market_of,
                          int S, int N, double L, const dh_lb_options* opt, dh_lb_result* out,
                          int32_t* n_launches);

/* ---- warm-start network: a feed-forward net from a market's prices to an optimiser start ------
 * x0 [13] = y_mean + y_std * net(((C p) / S0 - x_mean) / x_std): p [M] the market's prices, C
 * [F][M] the (linear) feature matrix, net a stack of n_layers - 1 hidden layers (ReLU) and a linear
 * output of DH_FFN_OUT values, BatchNorm already folded into its float weights.  The output is the
 * optimiser's unconstrained x (log / arctanh / identity of the 13 model parameters): it goes into
 * dh_calibrate_lbfgs_batch* and dh_calibrate_lm_batch as x0s, unchanged.
 * Arithmetic (one launch): each feature is an fp64 fma chain over j ascending,
 * divided by S0, standardised and rounded once to float; every neuron is one float fmaf chain from
 * its bias over k ascending (v_mfma_f32_32x32x2_f32, exact f32), ReLU = fmaxf(0, .); the output is
 * fma(y_std, (double)raw, y_mean) in fp64.  A market's result depends on nothing but its own row:
 * not on B, not on its place in the batch.                                                     */
enum {
    DH_FFN_OUT = 13,             /* outputs: the optimiser's x */
    DH_FFN_TM = 32,              /* markets per block */
    DH_FFN_MAX_HIDDEN = 6,       /* hidden layers at most (at least 1) */
    DH_FFN_MAX_WIDTH = 512,      /* hidden widths: multiples of 32 in [32, DH_FFN_MAX_WIDTH] */
    DH_FFN_MAX_IN = 64           /* F and M at most */
};
typedef struct dh_ffn dh_ffn;
/* widths [n_layers + 1] = F, the hidden widths, DH_FFN_OUT; weights the layers' W_l [out][in]
 * row-major one after the other, biases likewise; C [F][M]; x_mean, x_std [F]; y_mean, y_std
 * [DH_FFN_OUT].  Everything is copied to the device once (layers transposed and zero-padded: F up
 * to a multiple of 8, the outputs up to 32).  DH_E_ARG for n_layers outside [2, DH_FFN_MAX_HIDDEN + 1], F or
 * M outside [1, DH_FFN_MAX_IN], a hidden width that is no multiple of 32 in [32,
 * DH_FFN_MAX_WIDTH], a last width other than DH_FFN_OUT, x_std not finite and > 0, or any other
 * statistic not finite.  The object belongs to ctx: no forward call after the context is gone (dh_ffn_destroy alone needs no live context). */
int dh_ffn_create(dh_ctx* ctx, int n_layers, const int* widths, const float* weights,
                  const float* biases, const double* C, int M, const double* x_mean,
                  const double* x_std, const double* y_mean, const double* y_std, dh_ffn** out);
int dh_ffn_destroy(dh_ffn* ffn);
/* market [B][M], spots [B] -> x0 [B][DH_FFN_OUT] and, unless NULL, raw [B][DH_FFN_OUT] (the
 * network's standardised float output).  Host arrays, synchronous.  The values are the caller's
 * promise: finite prices and spots > 0 (the Python layer checks them).                          */
int dh_ffn_forward(dh_ffn* ffn, const double* market, const double* spots, int64_t B, double* x0,
                   float* raw);
/* The same over device pointers (d_raw may be NULL): one launch enqueued on `stream` (hipStream_t;
 * NULL = the context's), no synchronisation, no allocation, no host round trip; the same bits.  */
int dh_ffn_forward_dev(dh_ffn* ffn, const double* d_market, const double* d_spots, int64_t B,
                       double* d_x0, float* d_raw, void* stream);

/* ---- building blocks (exposed for API parity with the reference's public methods) -------- */
/* phi(u_j; tau) for one param set: DoubleHeston.characteristic_function (double_heston.py:48-97) */
int dh_cf(dh_ctx* ctx, const double* params, const double* u, int n, double tau, double* re,
          double* im);
/* The same at complex frequencies phi_j = u_re[j] + i u_im[j] (the reference documents
 * phi : complex, double_heston.py:48-61, and evaluates it with complex arithmetic throughout)  */
int dh_cf_complex(dh_ctx* ctx, const double* params, const double* u_re, const double* u_im,
                  int n, double tau, double* re, double* im);
/* [a_i, b_i] for param set i and option i: DoubleHeston.truncationRange (double_heston.py:100-139) */
int dh_trunc_range(dh_ctx* ctx, const double* params, const double* K, const double* T,
                   int64_t P, double L, double* a, double* b);
/* chi_k / psi_k for integer k_j on [c,d] within [a,b]: double_heston.py:141-158 */
int dh_cos_coeffs(dh_ctx* ctx, const int32_t* k, int n, double c, double d, double a, double b,
                  double* chi, double* psi);

/* ---- multi-GPU: RCCL communicator (SURVEY 8(b) dh_allgather_best, 8(e)) --------------------- */
/* For callers without torch.distributed (the Python layer's dhcos.distributed uses either).  One
 * communicator per rank, on its context's device and stream; RCCL (librccl.so.1, resolved at run
 * time) over xGMI.  Rank 0 makes the id and ships its bytes to the other ranks by any means.
 * Replaces nothing in the reference (single process); it carries the multi-start sharding of
 * lbfgs_calibrator.py:251-299 across GPUs.                                                      */
#define DH_COMM_ID_BYTES 128
typedef struct dh_comm dh_comm;
int dh_comm_id(unsigned char* id /* [DH_COMM_ID_BYTES] */);
/* Collective: every rank of `world` calls it with the same id. */
int dh_comm_create(dh_ctx* ctx, const unsigned char* id, int world, int rank, dh_comm** out);
int dh_comm_destroy(dh_comm* comm);
/* buf[n] (host): root's values on every rank (the start x0s and the RNG state after the draws). */
int dh_comm_broadcast(dh_comm* comm, double* buf, int64_t n, int root);
/* send[n] (host) of every rank -> recv[world][n] in rank order (the generator's price blocks). */
int dh_comm_allgather(dh_comm* comm, const double* send, int64_t n, double* recv);
/* All-gather of fixed-size per-start records: each rank passes rows x width doubles (its starts;
 * rows must be equal on every rank, padding rows carry a negative start index), all receives
 * [world * rows][width] in rank order, and best the winning start index (or -1): the first start,
 * in start order (column col_start), whose col_fun value is strictly below every earlier one's --
 * lbfgs_calibrator.py:271-275's rule (NaN never wins), without its re-pricing step.            */
int dh_allgather_best(dh_comm* comm, const double* rec, int rows, int width, int col_start,
                      int col_fun, double* all, int* best);
/* The same selection over records already on the host (no device work). */
int dh_best_start(const double* all, int64_t rows, int width, int col_start, int col_fun,
                  int* best);

/* ---- Monte Carlo path pricer (csrc/dh_mc.h) --------------------------------- */
/* Replaces nothing in the reference (it prices European vanillas by COS only): it is where the
 * calibrated parameters go to price what vanillas cannot, and the one check of the COS prices
 * that does not pass through the characteristic function.  The model's SDE (q = 0) is simulated
 * on the uniform grid dt = 1 / steps_per_year, one path per GPU lane: Andersen's QE scheme for
 * each variance factor, central weights for the log-spot, Poisson jumps by inversion, the running
 * maximum / minimum / sum of S over the step dates 1..n (discrete monitoring; the start value is
 * not a date).  Path i's random numbers are Philox4x32-10 blocks keyed by `seed` and counted by
 * (i, step), so they depend on (seed, i, step) only, and all P parameter sets of a call see the
 * same draws (common random numbers).  Results are a function of (params, options, n_paths,
 * steps_per_year, seed) alone: no atomics, every sum in a fixed order.                          */
enum { DH_MC_EUROPEAN = 0, DH_MC_ASIAN = 1, DH_MC_UP_AND_OUT = 2, DH_MC_DOWN_AND_OUT = 3 };
#define DH_MC_MAX_OPTIONS 64     /* options of one call (all priced from the same paths) */
#define DH_MC_POISSON_CAP 16     /* jumps per step at most; lambda / steps_per_year <= 1 */
typedef struct {
    int32_t kind;                /* DH_MC_*: european (S_T - K)^+ / (K - S_T)^+; asian: the
                                    arithmetic mean of S over dates 1..n against K; up_and_out /
                                    down_and_out: european if the running max stayed < barrier /
                                    the running min stayed > barrier, else 0 */
    int32_t is_call;             /* 0 put, else call */
    double strike;               /* finite, >= 0 */
    double maturity;             /* years: a whole number n >= 1 of steps (to 1e-9 relative) */
    double barrier;              /* > 0 for the two barrier kinds; not read otherwise */
} dh_mc_option;
/* price[p * n_options + j] = e^{-rT} mean payoff of option j under params[p] (records of
 * DH_PARAM_STRIDE doubles: 13 model params, S0 at 13, r at 14; q is not read) over paths
 * 0 .. n_paths - 1, stderr[...] = e^{-rT} sqrt((sum p^2 - (sum p)^2 / n) / (n (n - 1))).  Host
 * arrays, synchronous.  DH_E_ARG, before any device work, names the argument in dh_last_error():
 * a parameter that is not finite, v0 < 0, kappa / theta / sigma <= 0, |rho| >= 1, lambda < 0,
 * lambda / steps_per_year > 1, sigma_j < 0, spot <= 0; n_paths < 2; steps_per_year < 1; P outside
 * [1, 65535]; n_options outside [1, DH_MC_MAX_OPTIONS]; an unknown kind; a maturity that is not a
 * whole number of steps; a barrier <= 0 on a barrier option; a strike < 0 or not finite.         */
int dh_mc_price(dh_ctx* ctx, const double* params, int64_t P, const dh_mc_option* options,
                int n_options, int64_t n_paths, int steps_per_year, uint64_t seed, double* price,
                double* stderr_out);
/* The same over device pointers (d_params [P][16] in, d_price / d_stderr [P][n_options] out;
 * `options` stays a host array, copied when the call returns): two launches enqueued on `stream`
 * (hipStream_t; NULL = the context's), no synchronisation, no allocation after warm-up.  The
 * parameter values are the caller's promise (not readable here); the same bits as dh_mc_price.  */
int dh_mc_price_dev(dh_ctx* ctx, const double* d_params, int64_t P, const dh_mc_option* options,
                    int n_options, int64_t n_paths, int steps_per_year, uint64_t seed,
                    double* d_price, double* d_stderr, void* stream);
/* Validation export, in the spirit of dh_cf / dh_cos_coeffs: out[((p * n_paths + i) * n_obs + j) *
 * 6 ..] = S, v1, v2, running max, running min, running sum of path path0 + i under params[p] at
 * step obs_steps[j] (>= 1, strictly increasing), by the very step function the pricing kernel
 * runs.  Host arrays, synchronous; n_paths >= 1; at most 2^31 doubles of output per call.       */
int dh_mc_paths(dh_ctx* ctx, const double* params, int64_t P, int n_obs, const int32_t* obs_steps,
                int64_t path0, int64_t n_paths, int steps_per_year, uint64_t seed, double* out);

/* ---- Variance reduction for the path pricer (csrc/dh_mc_vr.h) ------------- */
/* Antithetic pairs and one control variate per option, by flag.
 * Mirror: the mirror of path i uses path i's Philox words, the uniforms 1 - U (exact: U is an odd
 * multiple of 2^-53) and the normals -Z; everything else is the step of 3.15.  Under
 * DH_MC_VR_ANTITHETIC n_paths counts walks (even, >= 4), there are n = n_paths / 2 pairs and the
 * sample y_i is the average of the payoffs of path i and its mirror; else n = n_paths, y_i the
 * payoff of path i.  Under DH_MC_VR_CONTROL the control c_i of a european option, and of any
 * option with strike 0, is S at its maturity step (known discounted mean m = S0); of an asian,
 * up_and_out or down_and_out option it is the European payoff of the same type and strike at the
 * same step, whose mean m is its COS price (dh_surface_price_dev, N = DH_MC_VR_COS_N, L =
 * DH_MC_VR_COS_L, the set's spot and rate, q = 0); under both flags c_i is the pair's average.
 * With the five sums over the n samples, every one in dh_mc_price's order, and disc = e^{-rT}:
 *     Cyy = Syy - Sy Sy / n,  Ccc = Scc - Sc Sc / n,  Cyc = Syc - Sy Sc / n,
 *     beta = Ccc > 0 ? Cyc / Ccc : 0,
 *     base_price = disc Sy / n,  base_stderr = disc sqrt(max(Cyy, 0) / (n (n - 1))),
 *     price = base_price - beta (disc Sc / n - m),
 *     stderr = disc sqrt(max(Cyy - beta Cyc, 0) / (n (n - 1))).
 * Without the control flag beta = 0, m = NaN, price = base_price, stderr = base_stderr; without
 * the antithetic flag base_price / base_stderr are dh_mc_price's bits.  beta is fitted on the
 * priced sample: the estimator carries the usual O(1 / n) bias, which is not corrected.         */
enum dh_mc_vr_flag { DH_MC_VR_ANTITHETIC = 1, DH_MC_VR_CONTROL = 2 };
enum dh_mc_vr_cos { DH_MC_VR_COS_N = 256 };   /* series length of the control means */
#define DH_MC_VR_COS_L (10.0)                 /* and their truncation width */
/* Host arrays [P][n_options], synchronous; base_price, base_stderr, beta and control_mean may be
 * NULL.  DH_E_ARG before any device work: everything dh_mc_price refuses; flags == 0 (that is
 * dh_mc_price) or with unknown bits; under the antithetic flag an odd n_paths or n_paths < 4.   */
int dh_mc_price_vr(dh_ctx* ctx, const double* params, int64_t P, const dh_mc_option* options,
                   int n_options, int64_t n_paths, int steps_per_year, uint64_t seed, int flags,
                   double* price, double* stderr_out, double* base_price, double* base_stderr,
                   double* beta, double* control_mean);
/* The same over device pointers (as dh_mc_price_dev; the last four may be NULL): enqueued on
 * `stream` without synchronisation, the same bits as dh_mc_price_vr.  The twins' option surface is
 * kept in the context: a call whose twins (strike, maturity, type, in maturity order) are those of
 * the call before rebuilds nothing; one whose twins differ waits for the earlier call's stream,
 * then builds its surface (one allocation, one blocking copy).                                  */
int dh_mc_price_vr_dev(dh_ctx* ctx, const double* d_params, int64_t P, const dh_mc_option* options,
                       int n_options, int64_t n_paths, int steps_per_year, uint64_t seed, int flags,
                       double* d_price, double* d_stderr, double* d_base_price,
                       double* d_base_stderr, double* d_beta, double* d_control_mean, void* stream);
/* dh_mc_paths with a mirror switch: mirror != 0 gives the statistics of the mirrors of the paths,
 * by the pair step the antithetic kernel runs; mirror == 0 is dh_mc_paths, bit for bit.         */
int dh_mc_paths_vr(dh_ctx* ctx, const double* params, int64_t P, int n_obs,
                   const int32_t* obs_steps, int64_t path0, int64_t n_paths, int steps_per_year,
                   uint64_t seed, int mirror, double* out);

/* ---- Greeks of the path pricer from coupled paths (csrc/dh_mc_greeks.h) --- */
/* Delta, gamma and the two v0 vegas of every option of dh_mc_price, with standard errors, from one
 * walk.  Inputs are those of dh_mc_price, plus spot_bump = eps (relative, 0 < eps < 1) and
 * v0_bump = b (relative, 0 < b < 1).  For a parameter record with spot S0:
 *     h = eps S0,   u+- = 1 +- eps,   d_j = b v0_j.
 * For path i and option o at its maturity step, the five payoffs are
 *     y      the payoff of dh_mc_price on the base path's state;
 *     y_S+-  the same payoff function on the base state with S, the running maximum, minimum and
 *            sum each multiplied by u+- (barrier tests use u max < barrier and u min > barrier, the
 *            Asian underlier is u sum / step): spot enters a path only as S = S0 exp(x), so this is
 *            the path at spot S0 u+-;
 *     y_j+-  the payoff on the path walked from v0_j +- d_j, with the same draws; the other factor
 *            and the jumps are the base path's.
 * The samples are
 *     delta_i  = (y_S+ - y_S-) / (2 h),
 *     gamma_i  = ((y_S+ - y) + (y_S- - y)) / (h h),
 *     vega_j,i = (y_j+ - y_j-) / (2 d_j),  j = 1, 2   (per unit of variance, as dh_surface_greeks).
 * For each of the five samples (price first), with disc = e^{-rT} and the sums over the n paths,
 *     value = disc Sum / n,   stderr = disc sqrt(max(Sum2 - Sum Sum / n, 0) / (n (n - 1))),
 * every sum in dh_mc_price's order (a xor butterfly per wave, the four waves as (w0 + w1) + (w2 +
 * w3), chunks in increasing order, slots in slot order): no atomics, the same call gives the same
 * bits, and the price plane and its stderr are dh_mc_price's bits.  A barrier's delta and gamma
 * carry the paths that u+- moves across the barrier: they estimate the difference quotients at eps,
 * not the derivatives.  Antithetic pairs and the control variate are not composed with these.   */
enum dh_mc_greek {
    DH_MC_GREEK_PRICE = 0, DH_MC_GREEK_DELTA, DH_MC_GREEK_GAMMA, DH_MC_GREEK_VEGA1,
    DH_MC_GREEK_VEGA2, DH_MC_N_GREEKS
};
/* value[(p * n_options + j) * DH_MC_N_GREEKS + g], stderr_out laid out the same way.  Host arrays,
 * synchronous.  DH_E_ARG, before any device work and naming the argument in dh_last_error():
 * everything dh_mc_price refuses; spot_bump or v0_bump outside (0, 1) or not finite; a record with
 * a v0 of 0, whose relative bump would be empty (v0_j - d_j > 0 always holds for b < 1).         */
int dh_mc_greeks(dh_ctx* ctx, const double* params, int64_t P, const dh_mc_option* options,
                 int n_options, int64_t n_paths, int steps_per_year, uint64_t seed,
                 double spot_bump, double v0_bump, double* value, double* stderr_out);
/* The same over device pointers (d_params [P][16] in, d_value / d_stderr [P][n_options][
 * DH_MC_N_GREEKS] out; `options` stays a host array, copied when the call returns): two launches
 * enqueued on `stream` (hipStream_t; NULL = the context's), no synchronisation, no allocation
 * after warm-up.  The parameter values are the caller's promise (not readable here: a v0 of 0
 * gives NaN vegas); the same bits as dh_mc_greeks.                                              */
int dh_mc_greeks_dev(dh_ctx* ctx, const double* d_params, int64_t P, const dh_mc_option* options,
                     int n_options, int64_t n_paths, int steps_per_year, uint64_t seed,
                     double spot_bump, double v0_bump, double* d_value, double* d_stderr,
                     void* stream);

/* ---- American and Bermudan options by least-squares Monte Carlo (csrc/dh_lsm.h) */
/* Early exercise on the paths of the pricer above, by the method of Longstaff and Schwartz (2001).
 * The exercise dates are the steps e, 2 e, 3 e, ... (e = exercise_every >= 1; the start value is
 * not a date), Delta = e / steps_per_year apart; every option's maturity step must be a whole
 * multiple of e, option j has D_j = step_j / e dates and date D_j is its maturity.  The state
 * (S, v1, v2) of every path is stored at every date; the dates are then walked backwards, one
 * launch each: at date d < D_j the discounted realised cashflow Y = e^{-r Delta} cash of the paths
 * in the money (intrinsic value h > 0) is regressed on the DH_LSM_BASIS terms
 *     1, x, y1, y2, x^2, y1^2, y2^2, x y1, x y2, y1 y2,   x = S / K - 1, y_i = v_i / theta_i - 1,
 * by the normal equations (Cholesky without pivoting), and a path exercises (cash = h, its
 * exercise date = d) where h > 0 and h > the fitted value, else cash = Y.  Nobody exercises at a
 * date with fewer than DH_LSM_MIN_ITM paths in the money or a Cholesky pivot that is not > 0: its
 * coefficient row is ten NaNs.  The same paths fit and value the policy (in-sample).  No atomics,
 * every sum in a fixed order: results are a function of the arguments alone.                     */
enum {
    DH_LSM_MAX_OPTIONS = 16,     /* options of one call (all priced from the same paths) */
    DH_LSM_BASIS = 10,           /* regression terms */
    DH_LSM_MIN_ITM = 64,         /* in-the-money paths a date needs to be fitted */
    DH_LSM_SLOTS = 128,          /* blocks per (set, option) of a backward launch at most; a block
                                    walks the chunks of 256 paths slot, slot + slots, ... */
    DH_LSM_MAX_GIB = 16          /* cap of the path store, P n_paths (24 Dmax + 12 n_options) bytes */
};
typedef struct {
    int32_t is_call;             /* 0 put, else call */
    int32_t pad;                 /* not read */
    double strike;               /* finite, >= 0 */
    double maturity;             /* years: a whole number n >= 1 of steps (to 1e-9 relative), n a
                                    multiple of exercise_every */
} dh_lsm_option;
/* price[p * n_options + j] = e^{-r Delta} mean of the cashflows of option j under params[p] after
 * date 1, stderr their sample standard error (dh_mc_price's formula); european / european_stderr
 * the same of the maturity payoffs of the same paths, discounted by e^{-r T} with T = D_j Delta
 * (price - european is the early-exercise premium; european is dh_mc_price's European value of the
 * same seed, paths and steps up to the order of its sum).  coef (may be NULL) is
 * [P][n_options][Dmax][DH_LSM_BASIS], Dmax the largest D_j: row d - 1 holds the coefficients used
 * at date d, NaN where the date was skipped, at the option's maturity date and past it.
 * exercise_date (may be NULL) is [P][n_options][n_paths]: the date 1 .. D_j at which each path's
 * cashflow falls (D_j where it never exercised early).  Host arrays, synchronous.  DH_E_ARG,
 * before any device work and naming the argument in dh_last_error(): the parameter, n_paths,
 * steps_per_year, P, strike and maturity cases of dh_mc_price; exercise_every < 1; a maturity step
 * that is not a multiple of exercise_every; n_options outside [1, DH_LSM_MAX_OPTIONS]; a path
 * store above DH_LSM_MAX_GIB GiB (ask for fewer paths or parameter sets per call).              */
int dh_lsm_price(dh_ctx* ctx, const double* params, int64_t P, const dh_lsm_option* options,
                 int n_options, int64_t n_paths, int steps_per_year, int exercise_every,
                 uint64_t seed, double* price, double* stderr_out, double* european,
                 double* european_stderr, double* coef, int32_t* exercise_date);
/* The same over device pointers (`options` stays a host array, copied when the call returns; d_coef
 * and d_exercise_date may be NULL): 2 + Dmax launches enqueued on `stream` (hipStream_t; NULL = the
 * context's), no synchronisation, no allocation after warm-up.  The parameter values are the
 * caller's promise (not readable here); the same bits as dh_lsm_price.                          */
int dh_lsm_price_dev(dh_ctx* ctx, const double* d_params, int64_t P, const dh_lsm_option* options,
                     int n_options, int64_t n_paths, int steps_per_year, int exercise_every,
                     uint64_t seed, double* d_price, double* d_stderr, double* d_european,
                     double* d_european_stderr, double* d_coef, int32_t* d_exercise_date,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DHCOS_H */
