"""Model of the feedback aligner (mcrx_hip_fbalign_*; the definition is in include/mcrx_hip.h): the quantiser in fp32 exactly as defined;
the sums as exact integers; the update written operation for operation in IEEE doubles (Python floats; / is correctly rounded), so that
tau_fp, s and res are the device's to the last bit; the coefficients as an exact fp32 restatement (userclock_model.coefs_f32); and
apply in float64 with a bound for what the fp32 arithmetic of the definition may differ from it."""
import math

import numpy as np

import dpd_model
import userclock_model

EPS = dpd_model.EPS
H, TAPS, GUARD_LOG2, MIN_LAG, MAX_LAG = 8, 32, 31, 8, 64


def taps_f32():
    """h_1 .. h_8: made in double, rounded to fp32"""
    return np.array([((-1.0) ** k) / k * (0.54 + 0.46 * math.cos(math.pi * k / 9.0)) for k in range(1, H + 1)], np.float64).astype(np.float32)


def constants(max_lag, full_scale):
    """(e, R, halo)"""
    return dpd_model.constants(5, full_scale)[3], int(max_lag) + H, int(max_lag) + 17


def q15(v, e):
    """(Q15 of the fp32 components v as int64, bad): clamp(rint(ldexpf(v, 15 - e))), a NaN gives 0; bad where it clamps or is not finite"""
    v = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        s = np.ldexp(v, 15 - e).astype(np.float32)
        r = np.rint(s)
        nan = np.isnan(s)
        bad = nan | (r > 32767.0) | (r < -32768.0)
        q = np.clip(np.where(nan, 0.0, r), -32768.0, 32767.0).astype(np.int64)
    return q, bad


def quantise(x, e):
    """(re, im as int64, bad per sample) of complex64 samples"""
    x = np.asarray(x, np.complex64)
    qr, br = q15(x.real, e)
    qi, bi = q15(x.imag, e)
    return qr, qi, br | bi


def sums(u, zh, R, e):
    """(C int64 [2 R + 1, 2], A int64 [2 H + 1, 2], Szz, rows, clamped) of one measure call, exactly.  A component is below 2^15, so a
    sum over fewer than 2^31 rows stays inside int64: numpy's integer dot products are exact."""
    n = len(u)
    rows = max(n - 2 * R, 0)
    C, A = np.zeros((2 * R + 1, 2), np.int64), np.zeros((2 * H + 1, 2), np.int64)
    if rows == 0:
        return C, A, 0, 0, 0
    ur, ui, ub = quantise(u, e)
    zr, zi, zb = quantise(zh, e)
    a, b = ur[R:n - R], ui[R:n - R]
    for l in range(-R, R + 1):
        c, d = zr[R + l:n - R + l], zi[R + l:n - R + l]
        C[l + R] = (a @ c + b @ d, a @ d - b @ c)
    for l in range(2 * H + 1):
        c, d = ur[R + l:n - R + l], ui[R + l:n - R + l]
        A[l] = (a @ c + b @ d, a @ d - b @ c)
    zc, zd = zr[R:n - R], zi[R:n - R]
    return C, A, int(zc @ zc + zd @ zd), rows, int(ub[R:n - R].sum() + zb[R:n - R].sum())


def split(tau_fp):
    """(nd, mu) of a delay: d = -tau_fp, nd = d >> 32 (floor), mu the low word"""
    d = -int(tau_fp)
    return d >> 32, d & 0xFFFFFFFF


def tau_ok(tau_fp, max_lag):
    return abs(int(tau_fp)) <= (int(max_lag) + 1) << 32


def coefs(W32, tau_fp):
    """(c as float32 [32], nd): the library's coefficients, exactly"""
    nd, mu = split(tau_fp)
    return userclock_model.coefs_f32(np.asarray(W32, np.float32), mu), nd


def solve(C, A, Szz, rows, R, max_lag, min_rows, h, g0, tau_fp, s):
    """The update's arithmetic, operation for operation: (tau_fp, (s.re, s.im), res, D, delta), or None where it is degenerate.
    C [2 R + 1, 2], A [17, 2]: integers; h: the eight taps; s: (re, im) doubles."""
    if rows < min_rows:
        return None
    hd = [float(v) for v in h]

    def c(l):
        return float(int(C[l + R][0])), float(int(C[l + R][1]))

    best, D = -1.0, -max_lag
    for l in range(-max_lag, max_lag + 1):
        cr, ci = c(l)
        p = cr * cr + ci * ci
        if p > best:
            best, D = p, l
    if not best > 0.0:
        return None
    bur, bui = c(D)
    bdr = bdi = g = 0.0
    for k in range(1, H + 1):
        (pr, pi), (mr, mi) = c(D + k), c(D - k)
        tr, ti = pr - mr, pi - mi
        bdr = bdr + hd[k - 1] * tr
        bdi = bdi + hd[k - 1] * ti
    Guu = float(int(A[0][0]))
    for k in range(1, H + 1):
        g = g + hd[k - 1] * float(int(A[k][1]))
    gud = -2.0 * g
    Gdd = 0.0
    for k in range(-H, H + 1):
        if k == 0:
            continue
        hk = hd[k - 1] if k > 0 else -hd[-k - 1]
        for m in range(-H, H + 1):
            if m == 0:
                continue
            hm = hd[m - 1] if m > 0 else -hd[-m - 1]
            Gdd = Gdd + (hk * hm) * float(int(A[abs(k - m)][0]))
    det = Guu * Gdd - gud * gud
    if not det > 0.0:
        return None
    alr, ali = (Gdd * bur + gud * bdi) / det, (Gdd * bui - gud * bdr) / det
    ber, bei = (Guu * bdr - gud * bui) / det, (Guu * bdi + gud * bur) / det
    m2 = alr * alr + ali * ali
    try:
        delta = -((ber * alr + bei * ali) / m2)
        xr, xi = s[0] * g0, s[1] * g0
        nsr, nsi = (xr * alr + xi * ali) / m2, (xi * alr - xr * ali) / m2
    except ZeroDivisionError:                                   # (the device divides by zero into an infinity or a NaN: not finite)
        return None
    res = float(int(Szz)) - (alr * bur + ali * bui)
    with np.errstate(all="ignore"):
        f32 = np.isfinite(np.float32(nsr)) and np.isfinite(np.float32(nsi))
    if not (all(math.isfinite(v) for v in (delta, nsr, nsi, res)) and f32 and -1.0 <= delta <= 1.0):
        return None
    tau = int(tau_fp) + round((float(D) + delta) * 4294967296.0)            # (Python's round of a float: ties to even, an exact int)
    if not tau_ok(tau, max_lag):
        return None
    return tau, (nsr, nsi), res, D, delta


def apply(W32, tau_fp, s, x, halo):
    """(y, bound): float64 apply to n + 2 halo complex64 samples with the library's fp32 coefficients and fp32 scale, and per component
    what the fp32 arithmetic of the definition may differ from it.  The coefficients and the scale are the library's own values, so
    only the arithmetic on the samples rounds: each of the 32 fused multiply-adds rounds a partial sum that is at most P = sum_j |c_j|
    |x_j| (plus the error so far) in magnitude: 32 eps P; the product s.im acc rounds once and the closing fused multiply-add once:
    eps (|s.im acc| + |out|).  Second-order terms are covered by the factor 1.01."""
    x = np.asarray(x, np.complex64).astype(np.complex128)
    n = len(x) - 2 * halo
    c, nd = coefs(W32, tau_fp)
    c = c.astype(np.float64)
    idx = (halo + np.arange(n) - nd + 15)[:, None] - np.arange(TAPS)[None, :]
    assert n == 0 or (idx.min() >= 0 and idx.max() < len(x)), (idx.min(), idx.max(), len(x))
    xs = x[idx]
    acc = (c * xs).sum(axis=1)
    pr, pi = (np.abs(c) * np.abs(xs.real)).sum(axis=1), (np.abs(c) * np.abs(xs.imag)).sum(axis=1)
    with np.errstate(all="ignore"):
        sr, si = float(np.float32(s[0])), float(np.float32(s[1]))
    y = complex(sr, si) * acc
    er, ei = TAPS * EPS * pr, TAPS * EPS * pi
    br = abs(sr) * er + abs(si) * ei + EPS * (np.abs(si * acc.imag) + np.abs(y.real))
    bi = abs(sr) * ei + abs(si) * er + EPS * (np.abs(si * acc.real) + np.abs(y.imag))
    return y, 1.01 * np.stack([br, bi], axis=-1)


class Model(object):
    """the handle: tau_fp, s, res, sums (Python-exact int64), counters, the host's count of the guard"""

    def __init__(self, max_lag=32, full_scale=None, target_gain=None, min_rows=1024, W32=None):
        self.Lm, self.g0, self.min_rows = int(max_lag), float(np.float32(target_gain)), int(min_rows)
        self.e, self.R, self.halo = constants(max_lag, full_scale)
        self.h = taps_f32()
        self.W32 = np.asarray(userclock_model.table_f64() if W32 is None else W32).astype(np.float32)
        self.reset()

    def reset(self):
        self.tau_fp, self.s, self.res = 0, (1.0, 0.0), 0.0
        self.C, self.A = np.zeros((2 * self.R + 1, 2), np.int64), np.zeros((2 * H + 1, 2), np.int64)
        self.Szz = self.rows = self.clamped = self.updates = self.degenerate = self.since = 0
        self.trained, self.last = False, None

    def set(self, tau_fp, s=1.0):
        s = complex(s)
        assert tau_ok(tau_fp, self.Lm)
        self.tau_fp, self.s, self.trained = int(tau_fp), (s.real, s.imag), True

    @property
    def tau(self):
        return self.tau_fp * 2.0 ** -32

    def execute(self, x):
        """float64, of n + 2 halo samples; an untrained handle copies"""
        x = np.asarray(x, np.complex64)
        if not self.trained:
            return x[self.halo:len(x) - self.halo].astype(np.complex128)
        return apply(self.W32, self.tau_fp, self.s, x, self.halo)[0]

    def measure(self, u, zh):
        """False, nothing measured, where the guard refuses"""
        u, zh = np.asarray(u, np.complex64), np.asarray(zh, np.complex64)
        offered = max(len(u) - 2 * self.R, 0)
        if self.since + offered > (1 << GUARD_LOG2):
            return False
        if offered == 0:
            return True
        C, A, Szz, rows, clamped = sums(u, zh, self.R, self.e)
        self.C += C
        self.A += A
        self.Szz, self.rows, self.clamped, self.since = self.Szz + Szz, self.rows + rows, self.clamped + clamped, self.since + offered
        return True

    def update(self):
        got = solve(self.C, self.A, self.Szz, self.rows, self.R, self.Lm, self.min_rows, self.h, self.g0, self.tau_fp, self.s)
        if got is None:
            self.degenerate += 1
        else:
            self.tau_fp, self.s, self.res, self.last = got[0], got[1], got[2], got[3:]
        self.C[:], self.A[:] = 0, 0
        self.Szz = self.rows = self.since = 0
        self.updates += 1
        self.trained = True

    def coefs(self):
        return coefs(self.W32, self.tau_fp)

    def align(self, u, z, rounds=3):
        """liquid_usrp_amd.fbalign.align on the model: (u[halo : n - halo], the aligned capture in float64)"""
        u, z = np.asarray(u, np.complex64), np.asarray(z, np.complex64)
        ut = u[self.halo:len(u) - self.halo]
        for _ in range(int(rounds)):
            assert self.measure(ut, self.execute(z).astype(np.complex64))
            self.update()
        return ut, self.execute(z)


def path(x, tau, gain=1.0, noise_std=0.0, seed=0):
    """What an observation receiver returns of the stream x, in float64: x late by tau samples (a fractional delay in the frequency domain
    of the stream extended circularly), times the complex gain, plus white noise of noise_std per component."""
    x = np.asarray(x, np.complex128)
    f = np.fft.fftfreq(len(x))
    y = complex(gain) * np.fft.ifft(np.fft.fft(x) * np.exp(-2j * np.pi * f * float(tau)))
    if noise_std:
        rng = np.random.RandomState(seed)
        y = y + noise_std * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))
    return y


def to_sc16(x):
    """int16 [n, 2] of a float stream through the shared codec's quantiser: rint(v 32768) clamped, round half to even"""
    x = np.asarray(x, np.complex64)
    v = np.stack([x.real, x.imag], axis=-1).astype(np.float32) * np.float32(32768.0)
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def remove_delay_and_gain(y, ref):
    """y with the least-squares complex gain and delay against ref taken out: (y', tau) where tau is the slope of the cross spectrum's
    phase over the occupied band, found by a fine search around the correlation peak; float64, circular"""
    y, ref = np.asarray(y, np.complex128), np.asarray(ref, np.complex128)
    n = len(y)
    Y, Rf = np.fft.fft(y), np.fft.fft(ref)
    X = Y * np.conj(Rf)
    f = np.fft.fftfreq(n)

    def score(t):
        return abs(np.sum(X * np.exp(2j * np.pi * f * t)))

    t0 = float(np.argmax(np.abs(np.fft.ifft(X))))
    t0 = t0 - n if t0 > n / 2 else t0
    lo, hi = t0 - 1.0, t0 + 1.0
    for _ in range(60):                                          # golden-section search on a unimodal peak
        a, b = lo + 0.381966 * (hi - lo), lo + 0.618034 * (hi - lo)
        if score(a) < score(b):
            lo = a
        else:
            hi = b
    tau = 0.5 * (lo + hi)
    yd = np.fft.ifft(Y * np.exp(2j * np.pi * f * tau))
    g = np.vdot(ref, yd) / np.vdot(ref, ref)
    return yd / g, tau


def nmse_aligned_db(y, ref):
    """NMSE of y against ref after delay and gain removal, in dB"""
    return dpd_model.nmse_db(remove_delay_and_gain(y, ref)[0], ref)


# The end-to-end cases (tests/test_fbalign.py finds them on the oracle alone with the exact models; tests/test_gpu_fbalign.py runs
# exactly these): cfr_model.SEVERITY's transmitter and stage, dpd on dpd_model.SEVERITY's amplifier and mpd on mpd_model.SEVERITY's
# three-branch amplifier, the amplifier's output through a path of 7.37 samples, 0.6 e^{1.1j} and 50 dB SNR, three rounds each of which
# aligns three times.  Recorded by tests/test_fbalign.py (power at |f| > 0.32 in dB; NMSE after delay and gain removal in dB; tau):
# `direct` = feedback without a path, `aligned` = through path and aligner, `whole` = the path removed to the whole sample and in gain.
# oob_margin_db = what the aligner costs against direct feedback there (0 where it costs nothing) plus 1 dB.  tau is what the aligner
# holds after the last round: behind the three-branch amplifier it includes that amplifier's own group delay (0.028 samples here).
# tau_tol: the noise of the path alone moves a delay estimate over these 86 400 samples at 50 dB SNR by about 1 / (2 pi B sqrt(N SNR))
# = 1e-5 samples rms (B = 0.16, the stream's rms bandwidth); ten times that.  (Measured on the memoryless amplifier: 2.5e-6.)
SEVERITY = dict(max_lag=16, tau=7.37, gain=0.6 * np.exp(1.1j), snr_db=50.0, rounds=3, align_rounds=3, min_rows=1024, edge=0.32,
                tau_tol=1e-4, oob_gain_db=15.0, device_slack_db=6.0,
                dpd=dict(oob_db=dict(direct=-73.25, aligned=-70.09, whole=-47.26), nmse_db=dict(direct=-68.89, aligned=-66.12, whole=-41.91),
                         tau=7.3700025, oob_margin_db=(-70.09 - -73.25) + 1.0),
                mpd=dict(oob_db=dict(direct=-61.10, aligned=-61.24, whole=-38.99), nmse_db=dict(direct=-52.79, aligned=-46.18, whole=-19.92),
                         tau=7.3978965, oob_margin_db=1.0))
