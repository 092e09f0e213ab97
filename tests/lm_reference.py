"""NumPy restatement of the device Levenberg-Marquardt state machine
(option-pricing-ffn-lbfgs_amd/csrc/dh_lm.h), in the same operation order: every sum is a Python
loop in index order over float64 scalars, nothing is fused, sqrt and / are correctly rounded, so
the CPU build of dh_lm.h (tests/native/liblmhost.so) must give the same bits.

    lm = Lm(x0, maxiter, maxfun, ftol, pgtol)
    while lm.more: lm.resume(f(lm.xe), g(lm.xe), H(lm.xe))
"""
import math

import numpy as np

N = 13
LAMBDA0, D_FLOOR, LAMBDA_MAX, XTOL, CHOL_RETRIES, INVALID = 1e-3, 1e-12, 1e16, 1e-10, 16, 1e10
GTOL, FTOL, XTOL_STOP, MAXITER, MAXFUN, STALLED, INVALID_X0 = 1, 2, 3, 4, 5, 6, 7


class Lm:
    def __init__(self, x0, maxiter, maxfun, ftol, pgtol):
        self.cfg = (int(maxiter), int(maxfun), float(ftol), float(pgtol))
        self.x = [float(v) for v in x0]
        self.xe = list(self.x)
        self.g = [0.0] * N
        self.H = [[0.0] * N for _ in range(N)]
        self.D = [0.0] * N
        self.delta = [0.0] * N
        self.w = [[0.0] * N for _ in range(N)]
        self.f = 0.0
        self.lam, self.nu, self.pred = LAMBDA0, 2.0, 0.0
        self.best_loss = math.inf
        self.started = False
        self.task = 0
        self.nit, self.nfev, self.n_calls, self.warnflag = 0, 1, 0, 0
        self.more = True

    def finish(self, task):
        self.task = task
        self.warnflag = 0 if task <= XTOL_STOP else (1 if task in (MAXITER, MAXFUN) else 2)
        self.more = False

    def factor(self):
        H, w = self.H, self.w
        for j in range(N):
            d = H[j][j] + self.lam * self.D[j]
            for k in range(j):
                d = d - w[j][k] * w[j][k]
            if not d > 0.0:
                return False
            piv = math.sqrt(d)
            w[j][j] = piv
            for i in range(j + 1, N):
                t = H[i][j]
                for k in range(j):
                    t = t - w[i][k] * w[j][k]
                w[i][j] = t / piv
        return True

    def solve(self):
        w, dl = self.w, self.delta
        for i in range(N):
            t = -self.g[i]
            for k in range(i):
                t = t - w[i][k] * dl[k]
            dl[i] = t / w[i][i]
        for i in range(N - 1, -1, -1):
            t = dl[i]
            for k in range(i + 1, N):
                t = t - w[k][i] * dl[k]
            dl[i] = t / w[i][i]
        gd = dHd = 0.0
        for i in range(N):
            gd = gd + self.g[i] * dl[i]
            r = 0.0
            for k in range(N):
                r = r + self.H[i][k] * dl[k]
            dHd = dHd + dl[i] * r
        self.pred = -gd - 0.5 * dHd

    def resume(self, fe, ge, He):
        maxiter, maxfun, ftol, pgtol = self.cfg
        if not self.more:
            return
        fe = float(fe)
        self.n_calls += 1
        valid = fe == fe and fe != INVALID
        fold = 0.0
        if not self.started:
            if not valid:
                self.f = fe
                return self.finish(INVALID_X0)
            accept = True
            self.started = True
        else:
            rho = (self.f - fe) / self.pred if valid and self.pred > 0.0 else -1.0
            accept = valid and rho > 0.0
            if accept:
                t = 2.0 * rho - 1.0
                self.lam = self.lam * max(1.0 / 3.0, 1.0 - t * t * t)
                self.nu = 2.0
                self.nit += 1
                fold = self.f
            else:
                self.lam = self.lam * self.nu
                self.nu = 2.0 * self.nu
        if accept:
            first = self.nit == 0
            self.f = fe
            self.best_loss = fe
            self.x = list(self.xe)
            self.g = [float(v) for v in ge]
            self.H = [[float(v) for v in row] for row in np.asarray(He).reshape(N, N)]
            self.D = [max(max(self.D[i], self.H[i][i]), D_FLOOR) for i in range(N)]
            gm = max(abs(v) for v in self.g)
            if not any(v != v for v in self.g) and gm <= pgtol:
                return self.finish(GTOL)
            if not first and (fold - self.f) <= ftol * max(max(abs(fold), abs(self.f)), 1.0):
                return self.finish(FTOL)
        if self.nit >= maxiter:
            return self.finish(MAXITER)
        if self.nfev >= maxfun:
            return self.finish(MAXFUN)
        retry = 0
        while True:
            if not self.lam <= LAMBDA_MAX or retry > CHOL_RETRIES:
                return self.finish(STALLED)
            if self.factor():
                break
            self.lam = self.lam * self.nu
            self.nu = 2.0 * self.nu
            retry += 1
        self.solve()
        dd = xx = 0.0
        for i in range(N):
            dd = dd + self.delta[i] * self.delta[i]
            xx = xx + self.x[i] * self.x[i]
        if dd != dd:
            return self.finish(STALLED)
        if math.sqrt(dd) <= XTOL * (math.sqrt(xx) + XTOL):
            return self.finish(XTOL_STOP)
        self.xe = [self.x[i] + self.delta[i] for i in range(N)]
        self.nfev += 1
