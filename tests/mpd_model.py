"""Model of the memory-polynomial predistorter (mcrx_hip_mpd_*; the definition is in include/mcrx_hip.h): the apply in float64 with a
bound for what the fp32 arithmetic of the definition may differ from it (dpd_model.apply's per branch plus the M - 1 additions); the
regressors in fp32 exactly as defined; the sums as exact integers; the update written operation for operation in IEEE doubles (Python
floats; math.sqrt and / are correctly rounded), so that coefficients, res and tables are the device's to the last bit."""
import math

import numpy as np

import dpd_model

EPS = dpd_model.EPS
QB = 17
GUARD_LOG2 = 26
TWO_QB = np.float32(2.0 ** QB)


def constants(table_log2, full_scale, target_gain):
    """(K, inv_step as fp32, step as double, e, inv_g0 as fp32): the host's values"""
    K, inv_step, step, e = dpd_model.constants(table_log2, full_scale)
    return K, inv_step, step, e, np.float32(1.0 / float(np.float32(target_gain)))


def regressors(z, inv_g0, e, P):
    """(Z, good): Z int64 [n, P, 2], the integers of phi_0 .. phi_{P-1} of every sample (zeros where it is not good); good bool [n]"""
    z = np.asarray(z, np.complex64)
    with np.errstate(all="ignore"):
        wr, wi = z.real * np.float32(inv_g0), z.imag * np.float32(inv_g0)
        pr, pi = np.ldexp(wr, -e).astype(np.float32), np.ldexp(wi, -e).astype(np.float32)
        t = dpd_model.fmaf(pr, pr, pi * pi)
        a = np.sqrt(t)
        good = t <= np.float32(1.0)
        Z = np.zeros((len(z), P, 2), np.int64)
        for k in range(P):
            Z[:, k, 0] = np.where(good, np.rint(pr * TWO_QB), 0.0).astype(np.int64)
            Z[:, k, 1] = np.where(good, np.rint(pi * TWO_QB), 0.0).astype(np.int64)
            pr, pi = pr * a, pi * a
    return Z, good


def targets(u, e):
    """(U, good): U int64 [n, 2]; good where |u / E|^2 <= 4"""
    u = np.asarray(u, np.complex64)
    with np.errstate(all="ignore"):
        pr, pi = np.ldexp(u.real, -e).astype(np.float32), np.ldexp(u.imag, -e).astype(np.float32)
        t = dpd_model.fmaf(pr, pr, pi * pi)
        good = t <= np.float32(4.0)
        U = np.stack([np.where(good, np.rint(pr * TWO_QB), 0.0), np.where(good, np.rint(pi * TWO_QB), 0.0)], axis=-1).astype(np.int64)
    return U, good


def rows_of(u, z, delays, P, inv_g0, e):
    """(Vr, Vi, skipped): the integer rows V = (B_0 .. B_{L-1}, U) of the eligible rows lead .. n - 1 as int64 [rows, L + 1] each"""
    Z, zg = regressors(z, inv_g0, e, P)
    U, ug = targets(u, e)
    lead, n = delays[-1], len(Z)
    ok = ug[lead:].copy()
    for d in delays:
        ok &= zg[lead - d:n - d]
    cols_r = [Z[lead - d:n - d, k, 0] for d in delays for k in range(P)] + [U[lead:, 0]]
    cols_i = [Z[lead - d:n - d, k, 1] for d in delays for k in range(P)] + [U[lead:, 1]]
    return np.stack(cols_r, axis=1)[ok], np.stack(cols_i, axis=1)[ok], int((~ok).sum())


def gram(Vr, Vi):
    """(Sre, Sim) int64 [L + 1, L + 1]: S_pq = sum conj(V_p) V_q, exactly.  Entries are below 2^18.01, so the two-product sums of 2^14
    rows stay below 2^52: every partial sum of a float64 matrix product is an integer it holds exactly, in any order."""
    W = Vr.shape[1]
    Sre, Sim = np.zeros((W, W), np.int64), np.zeros((W, W), np.int64)
    for at in range(0, len(Vr), 1 << 14):
        a, b = Vr[at:at + (1 << 14)].astype(np.float64), Vi[at:at + (1 << 14)].astype(np.float64)
        Sre += (a.T @ a + b.T @ b).astype(np.int64)
        Sim += (a.T @ b - b.T @ a).astype(np.int64)
    return Sre, Sim


def solve(S, L, rows, min_rows, ridge_log2):
    """The update's linear algebra, operation for operation: (c as a list of L (re, im) doubles, res), or None where it is degenerate.
    S: (Sre, Sim) [L + 1, L + 1] integers, the upper triangle used."""
    Sre, Sim = S
    if rows < min_rows:
        return None
    Ar = [[float(int(Sre[p][q])) for q in range(L)] for p in range(L)]
    Ai = [[float(int(Sim[p][q])) for q in range(L)] for p in range(L)]
    br, bi = [float(int(Sre[p][L])) for p in range(L)], [float(int(Sim[p][L])) for p in range(L)]
    suu = float(int(Sre[L][L]))
    tr = 0.0
    for l in range(L):
        tr = tr + Ar[l][l]
    lam = (tr / float(L)) * math.ldexp(1.0, -ridge_log2)
    for l in range(L):
        Ar[l][l] = Ar[l][l] + lam
    for j in range(L):
        for i in range(j + 1):
            sr, si = Ar[i][j], Ai[i][j]
            for p in range(i):
                ar, ai, cr, ci = Ar[p][i], Ai[p][i], Ar[p][j], Ai[p][j]
                sr = sr - (ar * cr + ai * ci)
                si = si - (ar * ci - ai * cr)
            if i < j:
                d = Ar[i][i]
                Ar[i][j], Ai[i][j] = sr / d, si / d
            else:
                if not sr > 0.0:
                    return None
                Ar[j][j], Ai[j][j] = math.sqrt(sr), 0.0
    yr, yi = [0.0] * L, [0.0] * L
    for i in range(L):
        sr, si = br[i], bi[i]
        for p in range(i):
            ar, ai = Ar[p][i], Ai[p][i]
            sr = sr - (ar * yr[p] + ai * yi[p])
            si = si - (ar * yi[p] - ai * yr[p])
        d = Ar[i][i]
        yr[i], yi[i] = sr / d, si / d
    cr, ci = [0.0] * L, [0.0] * L
    for i in range(L - 1, -1, -1):
        sr, si = yr[i], yi[i]
        for p in range(i + 1, L):
            ar, ai = Ar[i][p], Ai[i][p]
            sr = sr - (ar * cr[p] - ai * ci[p])
            si = si - (ar * ci[p] + ai * cr[p])
        d = Ar[i][i]
        cr[i], ci[i] = sr / d, si / d
    q = 0.0
    for l in range(L):
        q = q + (cr[l] * br[l] + ci[l] * bi[l])
    res = suu - q
    if not all(math.isfinite(v) for v in cr + ci + [res]):
        return None
    return list(zip(cr, ci)), res


def tabulate(c, M, P, K, step, e):
    """F [M, K + 1] complex64 of the coefficients, or None where an entry is not finite"""
    F = np.zeros((M, K + 1), np.complex64)
    inv_E = math.ldexp(1.0, -e)
    with np.errstate(all="ignore"):
        for m in range(M):
            for j in range(K + 1):
                rho = (float(j) * step) * inv_E
                gr, gi = c[m * P + P - 1]
                for k in range(P - 2, -1, -1):
                    gr = gr * rho + c[m * P + k][0]
                    gi = gi * rho + c[m * P + k][1]
                fr, fi = np.float32(gr), np.float32(gi)
                if not (np.isfinite(fr) and np.isfinite(fi)):
                    return None
                F[m, j] = complex(fr, fi)
    return F


def apply(F, x, delays, table_log2, full_scale, gain=1.0):
    """(y, bound): float64 apply of the fp32 tables F [M, K + 1] to lead + n complex64 samples x (the history in front), and per component
    what the fp32 arithmetic of the definition may differ from it: dpd_model.apply's bound per branch, and for each of the M - 1 fp32
    additions eps times the magnitude of the sum it rounds (the exact partial sum plus the bound so far); the gain adds eps |y|.
    Second-order terms are covered by dpd_model.apply's factor 1.01 and one more here."""
    x = np.asarray(x, np.complex64)
    lead = delays[-1]
    n = len(x) - lead
    yr = yi = br = bi = None
    for m, d in enumerate(delays):
        p, b = dpd_model.apply(F[m], x[lead - d:lead - d + n], table_log2, full_scale)
        if m == 0:
            yr, yi, br, bi = p.real.copy(), p.imag.copy(), b[:, 0].copy(), b[:, 1].copy()
        else:
            yr, yi, br, bi = yr + p.real, yi + p.imag, br + b[:, 0], bi + b[:, 1]
            br, bi = br + EPS * (np.abs(yr) + br), bi + EPS * (np.abs(yi) + bi)
    g = float(np.float32(gain))
    if g != 1.0:
        yr, yi = g * yr, g * yi
        br, bi = abs(g) * br + EPS * (np.abs(yr) + abs(g) * br), abs(g) * bi + EPS * (np.abs(yi) + abs(g) * bi)
    return yr + 1j * yi, 1.01 * np.stack([br, bi], axis=-1)


class Model(object):
    """the handle: tables (complex64), sums (int64: the guard keeps them inside), counters, the host's count of the guard"""

    def __init__(self, branches, delays, order=5, table_log2=7, full_scale=None, target_gain=None, min_rows=None, ridge_log2=30,
                 forget_shift=0, gain=1.0):
        self.M, self.delays, self.P = int(branches), [int(d) for d in delays], int(order)
        assert len(self.delays) == self.M
        self.L, self.lead = self.M * self.P, self.delays[-1]
        self.table_log2, self.full_scale = int(table_log2), float(np.float32(full_scale))
        self.K, self.inv_step, self.step, self.e, self.inv_g0 = constants(table_log2, full_scale, target_gain)
        self.min_rows = 64 * self.L if min_rows is None else int(min_rows)
        self.ridge_log2, self.forget_shift, self.gain = int(ridge_log2), int(forget_shift), float(np.float32(gain))
        self.reset()

    def reset(self):
        self.F = np.zeros((self.M, self.K + 1), np.complex64)
        self.F[0] = 1.0
        self.Sre, self.Sim = np.zeros((self.L + 1, self.L + 1), np.int64), np.zeros((self.L + 1, self.L + 1), np.int64)
        self.c = [(1.0, 0.0)] + [(0.0, 0.0)] * (self.L - 1)
        self.res = 0.0
        self.rows = self.updates = self.skipped = self.degenerate = self.since = 0
        self.trained = False

    def set_tables(self, F):
        self.F = np.asarray(F, np.complex64).reshape(self.M, self.K + 1).copy()
        self.trained = True

    def execute(self, x):
        """float64, of lead + n samples; an untrained handle copies (times the gain)"""
        x = np.asarray(x, np.complex64)
        if not self.trained:
            return x[self.lead:].astype(np.complex128) * (self.gain if self.gain != 1.0 else 1.0)
        return apply(self.F, x, self.delays, self.table_log2, self.full_scale, self.gain)[0]

    def measure(self, u, z):
        """False, nothing measured, where the guard refuses"""
        u, z = np.asarray(u, np.complex64), np.asarray(z, np.complex64)
        offered = max(len(u) - self.lead, 0)
        if self.since + offered > (1 << GUARD_LOG2):
            return False
        if offered == 0:
            return True
        self.since += offered
        Vr, Vi, skipped = rows_of(u, z, self.delays, self.P, self.inv_g0, self.e)
        Sre, Sim = gram(Vr, Vi)
        self.Sre += np.triu(Sre)
        self.Sim += np.triu(Sim)
        self.rows += len(Vr)
        self.skipped += skipped
        return True

    def update(self):
        got = solve((self.Sre, self.Sim), self.L, self.rows, self.min_rows, self.ridge_log2)
        F = None if got is None else tabulate(got[0], self.M, self.P, self.K, self.step, self.e)
        if F is None:
            self.degenerate += 1
        else:
            self.F, self.c, self.res = F, got[0], got[1]
        s = self.forget_shift
        self.Sre >>= s                                          # (numpy's >> of a negative int64 is the arithmetic shift)
        self.Sim >>= s
        self.rows >>= s
        self.since = (self.since + (1 << s) - 1) >> s
        self.updates += 1
        self.trained = True

    def sums(self):
        """int64 [(L + 1)(L + 2) / 2, 2]: the upper triangle row by row, as mcrx_hip_mpd_read gives it"""
        iu = np.triu_indices(self.L + 1)
        return np.stack([self.Sre[iu], self.Sim[iu]], axis=-1)

    def coefficients(self):
        return np.array([complex(re, im) for re, im in self.c], np.complex128).reshape(self.M, self.P)


def memory_amplifier(configs, weights, u):
    """the three-branch amplifier of the end-to-end case on the host: sum_b weights[b] * rfchain_model.amplifier(configs[b], u[i - b]),
    zeros in front of the stream; float64"""
    import rfchain_model
    u = np.asarray(u, np.complex128)
    y = np.zeros(len(u), np.complex128)
    for b, (cfg, w) in enumerate(zip(configs, weights)):
        a = rfchain_model.amplifier(cfg, u)
        y[b:] += complex(w) * a[:len(u) - b]
    return y


nmse_db = dpd_model.nmse_db

# The end-to-end case (tests/test_mpd.py finds it on the oracle alone; tests/test_gpu_mpd.py runs exactly this): cfr_model.SEVERITY's
# transmitter and its stage, then the predistorter (three branches on delays 0, 1, 2, five powers each, 128 intervals up to twice the
# stream's peak), then a three-branch amplifier: Rapp p = 2 at 10 / 7 / 12 dB input back-off with +5 / -8 / +3 degrees of AM/PM on
# u[i], u[i-1], u[i-2], weighted 1, 0.08 e^{0.7j}, -0.032 e^{-0.4j}.  Three rounds of mpd and three of dpd on the same amplifier.
# model_nmse_db: what the exact models reach on the oracle's stream after three rounds (dpd, mpd), as tests/test_mpd.py measured and
# asserts; nmse_gain_db = their difference less the 6 dB that cover the device transmitter's different payload stream.
SEVERITY = dict(branches=3, delays=(0, 1, 2), order=5, table_log2=7, full_scale_over_peak=2.0, rounds=3, edge=0.32,
                amp_ibo_db=(10.0, 7.0, 12.0), amp_ampm_deg=(5.0, -8.0, 3.0), amp_smooth=2, amp_gain=1.0,
                amp_weights=(1.0, 0.08 * np.exp(0.7j), -0.032 * np.exp(-0.4j)),
                model_nmse_db=(-25.52, -52.75), nmse_gain_db=(-25.52 - -52.75) - 6.0, oob_slack_db=1.0)
# (measured there: no predistorter -22.35 dB NMSE and -39.50 dB at |f| > 0.32; dpd -25.52 and -53.89; mpd -52.75 and -61.10)
