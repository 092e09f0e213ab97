// dh_lm.h -- Levenberg-Marquardt as a resumable state machine, for the device-resident batch
// driver (dh_calibrate_lm_batch).  One calibration start = one LmCore.  The code is
// plain scalar C++ over the start's own arrays: the step kernel (dh_lb_driver.h lm_step_kernel)
// runs it in one lane on the start's state in LDS, the CPU check build (tests/native/lm_host.cpp)
// as it stands -- nothing is contracted into FMAs, every sum runs in index order, and sqrt and
// the divisions are correctly rounded on both, so both give the same bits.
//
// The algorithm is Nielsen's damping (K. Madsen, H. B. Nielsen, O. Tingleff, Methods for Non-Linear
// Least Squares Problems, 2nd ed. 2004, algorithm 3.16) with Marquardt's scaling of the damping
// term.  The caller supplies, at each requested point, the loss f, its gradient g and the
// Gauss-Newton Hessian H of its least-squares part (dh_gauss_newton.h):
//   1. at the current x hold f, g, H;
//   2. D_i = max(D_i, H_ii, kDFloor): a running maximum over the accepted points;
//   3. solve (H + lambda diag(D)) delta = -g by Cholesky; on a pivot that is not > 0 (NaN
//      included) lambda <- lambda nu, nu <- 2 nu and re-factor, at most kCholRetries times -- this
//      costs no request;
//   4. request f, g, H at x + delta;
//   5. rho = (f - f_trial) / pred,  pred = -g'delta - delta'H delta / 2;
//   6. accept if the trial is valid (not NaN, not the 1e10 marker), pred > 0 and rho > 0:
//      lambda <- lambda max(1/3, 1 - (2 rho - 1)^3), nu = 2, and the trial's f, g, H become the
//      current ones; otherwise lambda <- lambda nu, nu <- 2 nu.
// One iteration is one request; nfev == n_calls counts requests (x0 included), nit accepted steps.
//
// Stops, each with its own code (include/dhcos.h DH_LM_*), tested in this order:
//   at x0         f invalid or NaN                                    kInvalidX0  (x = x0)
//   after accept  max |g_i| <= pgtol                                  kGtol       (also at x0)
//                 (f_old - f) <= ftol max(|f_old|, |f|, 1)            kFtol
//                 nit >= maxiter                                      kMaxiter
//   before a step nfev >= maxfun                                      kMaxfun
//                 lambda > kLambdaMax, or the retries ran out         kStalled
//   after solve   a NaN step (a NaN gradient or Hessian)              kStalled
//                 |delta| <= kXtol (|x| + kXtol)                      kXtolStop
// x is always the last accepted point and s.f its loss, so fun <= f(x0).
//
// Constants: kLambda0 = 1e-3 (Marquardt's; with the scaling it is relative to H's diagonal),
// kDFloor = 1e-12, kLambdaMax = 1e16, kXtol = 1e-10, kCholRetries = 16 (lambda grows by
// 2^(k (k + 1) / 2) over k retries: past kLambdaMax from kLambda0 at k = 11).
#ifndef DH_LM_H
#define DH_LM_H

#include <math.h>

#ifndef DH_HD
#define DH_HD __host__ __device__
#endif

namespace dhlm {

constexpr int kN = 13;
constexpr double kLambda0 = 1.0e-3;
constexpr double kDFloor = 1.0e-12;
constexpr double kLambdaMax = 1.0e16;
constexpr double kXtol = 1.0e-10;
constexpr int kCholRetries = 16;
constexpr double kInvalid = 1.0e10;     // the loss of a set with an invalid price

// task codes: 0 before the first request is consumed, -1 running, > 0 final (DH_LM_*)
enum : int {
    kStart = 0, kRun = -1,
    kGtol = 1, kFtol = 2, kXtolStop = 3, kMaxiter = 4, kMaxfun = 5, kStalled = 6, kInvalidX0 = 7
};

struct LmConfig {
    int maxiter;                // accepted steps
    int maxfun;                 // requests, x0 included
    double ftol;
    double pgtol;
};

struct LmScalars {
    double f;                   // loss at x
    double lambda, nu;
    double pred;                // predicted reduction of the pending step
    double best_loss;           // smallest valid loss evaluated (== f once x0 is valid)
    int task, nit, nfev, warnflag, done, n_calls;
};

struct LmCore {
    double x[kN], g[kN], H[kN * kN], D[kN];
    double xe[kN];              // the requested point x + delta
    double delta[kN];
    double w[kN * kN];          // the Cholesky factor (work)
    LmScalars s;
};

DH_HD inline int lm_finish(LmScalars& s, int task) {
    s.task = task;
    s.warnflag = task <= kXtolStop ? 0 : (task == kMaxiter || task == kMaxfun ? 1 : 2);
    s.done = 1;
    return 0;
}

// lower Cholesky factor of H + lambda diag(D) into w; false at a pivot that is not > 0
DH_HD inline bool lm_factor(LmCore& c) {
#pragma clang fp contract(off)
    for (int j = 0; j < kN; ++j) {
        double d = c.H[j * kN + j] + c.s.lambda * c.D[j];
        for (int k = 0; k < j; ++k) d = d - c.w[j * kN + k] * c.w[j * kN + k];
        if (!(d > 0.0)) return false;
        const double l = sqrt(d);
        c.w[j * kN + j] = l;
        for (int i = j + 1; i < kN; ++i) {
            double t = c.H[i * kN + j];
            for (int k = 0; k < j; ++k) t = t - c.w[i * kN + k] * c.w[j * kN + k];
            c.w[i * kN + j] = t / l;
        }
    }
    return true;
}

// delta = -(L L')^-1 g and the predicted reduction
DH_HD inline void lm_solve(LmCore& c) {
#pragma clang fp contract(off)
    for (int i = 0; i < kN; ++i) {                     // L y = -g
        double t = -c.g[i];
        for (int k = 0; k < i; ++k) t = t - c.w[i * kN + k] * c.delta[k];
        c.delta[i] = t / c.w[i * kN + i];
    }
    for (int i = kN - 1; i >= 0; --i) {                // L' delta = y
        double t = c.delta[i];
        for (int k = i + 1; k < kN; ++k) t = t - c.w[k * kN + i] * c.delta[k];
        c.delta[i] = t / c.w[i * kN + i];
    }
    double gd = 0.0, dHd = 0.0;
    for (int i = 0; i < kN; ++i) {
        gd = gd + c.g[i] * c.delta[i];
        double r = 0.0;
        for (int k = 0; k < kN; ++k) r = r + c.H[i * kN + k] * c.delta[k];
        dHd = dHd + c.delta[i] * r;
    }
    c.s.pred = -gd - 0.5 * dHd;
}

DH_HD inline double lm_amax(const double* v) {         // NaN if any component is
    double m = 0.0;
    bool nan = false;
    for (int i = 0; i < kN; ++i) {
        m = fmax(m, fabs(v[i]));
        nan = nan || v[i] != v[i];
    }
    return nan ? __builtin_nan("") : m;
}

// lm_begin starts a run at x0.  Whenever it or lm_resume returns 1, evaluate f, g and H at xe and
// call lm_resume with them; 0 means the start is finished (s.task, s.warnflag, s.nit, s.nfev, x and
// s.f are final).
DH_HD inline int lm_begin(LmCore& c, const double* x0) {
    for (int i = 0; i < kN; ++i) {
        c.x[i] = c.xe[i] = x0[i];
        c.g[i] = c.D[i] = c.delta[i] = 0.0;
    }
    for (int i = 0; i < kN * kN; ++i) c.H[i] = c.w[i] = 0.0;
    c.s = LmScalars{};
    c.s.lambda = kLambda0;
    c.s.nu = 2.0;
    c.s.best_loss = __builtin_huge_val();
    c.s.task = kStart;
    c.s.nfev = 1;
    return 1;
}

DH_HD inline int lm_resume(LmCore& c, const LmConfig& cf, double fe, const double* ge,
                           const double* He) {
#pragma clang fp contract(off)
    LmScalars& s = c.s;
    if (s.done) return 0;
    s.n_calls += 1;
    const bool valid = fe == fe && fe != kInvalid;
    bool accept;
    double fold = 0.0;
    if (s.task == kStart) {
        if (!valid) {
            s.f = fe;
            return lm_finish(s, kInvalidX0);
        }
        accept = true;
        s.task = kRun;
    } else {
        const double rho = (valid && s.pred > 0.0) ? (s.f - fe) / s.pred : -1.0;
        accept = valid && rho > 0.0;
        if (accept) {
            const double t = 2.0 * rho - 1.0;
            s.lambda = s.lambda * fmax(1.0 / 3.0, 1.0 - t * t * t);
            s.nu = 2.0;
            s.nit += 1;
            fold = s.f;
        } else {
            s.lambda = s.lambda * s.nu;
            s.nu = 2.0 * s.nu;
        }
    }
    if (accept) {
        const bool first = s.nit == 0;
        s.f = fe;
        s.best_loss = fe;
        for (int i = 0; i < kN; ++i) {
            c.x[i] = c.xe[i];
            c.g[i] = ge[i];
        }
        for (int i = 0; i < kN * kN; ++i) c.H[i] = He[i];
        for (int i = 0; i < kN; ++i) c.D[i] = fmax(fmax(c.D[i], c.H[i * kN + i]), kDFloor);
        if (lm_amax(c.g) <= cf.pgtol) return lm_finish(s, kGtol);
        if (!first && (fold - s.f) <= cf.ftol * fmax(fmax(fabs(fold), fabs(s.f)), 1.0))
            return lm_finish(s, kFtol);
    }
    if (s.nit >= cf.maxiter) return lm_finish(s, kMaxiter);
    if (s.nfev >= cf.maxfun) return lm_finish(s, kMaxfun);
    for (int retry = 0;; ++retry) {
        if (!(s.lambda <= kLambdaMax) || retry > kCholRetries) return lm_finish(s, kStalled);
        if (lm_factor(c)) break;
        s.lambda = s.lambda * s.nu;
        s.nu = 2.0 * s.nu;
    }
    lm_solve(c);
    double dd = 0.0, xx = 0.0;
    for (int i = 0; i < kN; ++i) {
        dd = dd + c.delta[i] * c.delta[i];
        xx = xx + c.x[i] * c.x[i];
    }
    if (dd != dd) return lm_finish(s, kStalled);        // a NaN gradient or Hessian
    if (sqrt(dd) <= kXtol * (sqrt(xx) + kXtol)) return lm_finish(s, kXtolStop);
    for (int i = 0; i < kN; ++i) c.xe[i] = c.x[i] + c.delta[i];
    s.nfev += 1;
    return 1;
}

}  // namespace dhlm

#endif  // DH_LM_H
