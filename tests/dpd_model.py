"""Model of the digital predistorter (mcrx_hip_dpd_*; the definition is in include/mcrx_hip.h): the apply in float64 with a bound for
what the fp32 arithmetic of the definition may differ from it; the bins in fp32 exactly as defined; the accumulators as Python
integers; the update written operation for operation in IEEE doubles (Python floats; math.sqrt and / are correctly rounded), so that the
table it makes is the device's to the last bit."""
import math

import numpy as np

EPS = 2.0 ** -24          # half an ulp of fp32, relative
GUARD_LOG2 = 28


def constants(table_log2, full_scale):
    """(K, inv_step as fp32, step as double, e): the host's values"""
    K = 1 << int(table_log2)
    fs = float(np.float32(full_scale))
    m, ex = math.frexp(fs)
    return K, np.float32(K / fs), fs / K, (ex - 1 if m == 0.5 else ex)


def fmaf(a, b, c):
    """fp32 fma of fp32 arrays, correctly rounded: the exact product in float64, one float64 addition whose error TwoSum recovers, and
    the rounding to fp32 decided by that error where the float64 sum lies exactly between two fp32 values"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        r = p + c
        bb = r - p
        err = (p - (r - bb)) + (c - bb)
        r32 = r.astype(np.float32)
        up, dn = np.nextafter(r32, np.float32(np.inf)), np.nextafter(r32, np.float32(-np.inf))
        tie_up = np.isfinite(r) & (r == (r32.astype(np.float64) + up.astype(np.float64)) / 2.0) & (err > 0.0)
        tie_dn = np.isfinite(r) & (r == (r32.astype(np.float64) + dn.astype(np.float64)) / 2.0) & (err < 0.0)
    return np.where(tie_up, up, np.where(tie_dn, dn, r32))


def norm2_f32(x):
    """fmaf(x.re, x.re, x.im * x.im) of complex64 samples"""
    x = np.asarray(x, np.complex64)
    with np.errstate(all="ignore"):
        return fmaf(x.real, x.real, x.imag * x.imag)


def bins(u, z, table_log2, full_scale):
    """the bin of every pair, -1 where it is not eligible (int64)"""
    K, inv_step, _, e = constants(table_log2, full_scale)
    tu, tz = norm2_f32(u), norm2_f32(z)
    with np.errstate(all="ignore"):
        jf = np.rint(np.sqrt(tu) * inv_step)                # fp32 throughout
        zmax2 = np.float32(math.ldexp(1.0, 2 * e + 4)) if 2 * e + 4 <= 127 else np.float32(np.inf)
        ok = (tu < np.inf) & (tz < np.inf) & (tz <= zmax2) & (jf <= np.float32(K))
    return np.where(ok, np.where(ok, jf, 0).astype(np.int64), -1)


def terms(u, z, e):
    """(sre, sim, suu) as int64: fp64 products of fp32 components are exact, so the float64 sum of two IS the fma's single rounding"""
    u, z = np.asarray(u, np.complex64), np.asarray(z, np.complex64)
    a, b, c, d = (v.astype(np.float64) for v in (u.real, u.imag, z.real, z.imag))
    scale = math.ldexp(1.0, 32 - 2 * e)
    return tuple(np.rint(v * scale).astype(np.int64) for v in (c * a + d * b, d * a + (-(c * b)), a * a + b * b))


def apply(F, x, table_log2, full_scale, gain=1.0):
    """(y, bound): float64 apply of the fp32 table F to the complex64 samples x, and per component (re, im) what the fp32 arithmetic
    of the definition may differ from it.  The bound, with eps = 2^-24:
      s     t carries 2 eps (the product and the fma), the root halves that and adds its own eps, the product with inv_step one more:
            |ds| <= 3.1 eps s.  The interpolant is continuous and min() is 1-Lipschitz, so a step across an interval edge or across K
            costs no more than the steeper neighbour's slope.
      G_c   |dG_c| <= |ds| max(|dF_c| of intervals k - 1, k, k + 1) + eps f |dF_c| (the fp32 difference) + eps |G_c| (the fma)
      y.re  |dG.re| |x.re| + |dG.im| |x.im| + eps (|G.im x.im| + |G.re x.re| + |G.im x.im|), likewise y.im; the gain adds eps |y_c|.
    Second-order terms are covered by the factor 1.01 the bound is returned with."""
    K, inv_step, _, _ = constants(table_log2, full_scale)
    F = np.asarray(F, np.complex64)
    Fr, Fi = F.real.astype(np.float64), F.imag.astype(np.float64)
    dFr, dFi = (F.real[1:] - F.real[:-1]).astype(np.float64), (F.imag[1:] - F.imag[:-1]).astype(np.float64)      # fp32 differences
    x = np.asarray(x, np.complex64)
    xr, xi = x.real.astype(np.float64), x.imag.astype(np.float64)
    with np.errstate(all="ignore"):
        a = np.sqrt(xr * xr + xi * xi)
        s = np.fmin(a * float(inv_step), float(K))
        k = np.minimum(np.floor(s), K - 1).astype(np.int64)
        f = s - k
        gr, gi = Fr[k] + f * dFr[k], Fi[k] + f * dFi[k]
        yr, yi = gr * xr - gi * xi, gr * xi + gi * xr
        lo, hi = np.maximum(k - 1, 0), np.minimum(k + 1, K - 1)
        slope_r = np.maximum(np.abs(dFr[k]), np.maximum(np.abs(dFr[lo]), np.abs(dFr[hi])))
        slope_i = np.maximum(np.abs(dFi[k]), np.maximum(np.abs(dFi[lo]), np.abs(dFi[hi])))
        ds = 3.1 * EPS * s
        dgr = ds * slope_r + EPS * (f * np.abs(dFr[k]) + np.abs(gr))
        dgi = ds * slope_i + EPS * (f * np.abs(dFi[k]) + np.abs(gi))
        br = dgr * np.abs(xr) + dgi * np.abs(xi) + EPS * (np.abs(gr * xr) + 2.0 * np.abs(gi * xi))
        bi = dgr * np.abs(xi) + dgi * np.abs(xr) + EPS * (np.abs(gr * xi) + 2.0 * np.abs(gi * xr))
        g = float(np.float32(gain))
        if g != 1.0:
            yr, yi, br, bi = g * yr, g * yi, abs(g) * br + EPS * np.abs(g * yr), abs(g) * bi + EPS * np.abs(g * yi)
    return yr + 1j * yi, 1.01 * np.stack([br, bi], axis=-1) + 1e-44


def update_table(cnt, Sre, Sim, Suu, K, step, g0, min_count):
    """The update, operation for operation: the new table as a list of K + 1 (re, im) doubles before the rounding to fp32, or None
    where no bin is valid."""
    Ar, Ai = [0.0] * (K + 1), [0.0] * (K + 1)
    first = -1
    for j in range(K + 1):
        if int(cnt[j]) >= min_count and int(Suu[j]) > 0:
            Ar[j], Ai[j] = float(int(Sre[j])) / float(int(Suu[j])), float(int(Sim[j])) / float(int(Suu[j]))
            if first < 0:
                first = j
        elif first >= 0:
            Ar[j], Ai[j] = Ar[j - 1], Ai[j - 1]
    if first < 0:
        return None
    for j in range(first):
        Ar[j], Ai[j] = Ar[first], Ai[first]
    o, prev = [0.0] * (K + 1), 0.0
    for j in range(K + 1):
        v = math.sqrt(Ar[j] * Ar[j] + Ai[j] * Ai[j]) * (float(j) * step)
        prev = v if j == 0 else (v if v > prev else prev)
        o[j] = prev
    F = [None] * (K + 1)
    j = 1
    for i in range(1, K + 1):
        ri = float(i) * step
        d = g0 * ri
        while j <= K and o[j] < d:
            j += 1
        if j > K:
            rin, ar, ai = float(K) * step, Ar[K], Ai[K]
        else:
            den = o[j] - o[j - 1]
            fr = (d - o[j - 1]) / den if den > 0.0 else 0.0
            rin = float(j - 1) * step + fr * step
            ar, ai = Ar[j - 1] + fr * (Ar[j] - Ar[j - 1]), Ai[j - 1] + fr * (Ai[j] - Ai[j - 1])
        mag, q = math.sqrt(ar * ar + ai * ai), rin / ri
        F[i] = ((q * ar) / mag, -((q * ai) / mag)) if mag > 0.0 else (q, 0.0)
    F[0] = F[1]
    return F


class Model(object):
    """the handle: table (complex64), accumulators (lists of Python integers), counters, the host's count of the guard"""

    def __init__(self, table_log2, full_scale, target_gain, min_count=8, forget_shift=0, gain=1.0):
        self.table_log2, self.full_scale = int(table_log2), float(np.float32(full_scale))
        self.K, self.inv_step, self.step, self.e = constants(table_log2, full_scale)
        self.g0, self.min_count, self.forget_shift, self.gain = float(np.float32(target_gain)), int(min_count), int(forget_shift), float(np.float32(gain))
        self.reset()

    def reset(self):
        K = self.K
        self.F = np.ones(K + 1, np.complex64)
        self.cnt, self.Sre, self.Sim, self.Suu = [0] * (K + 1), [0] * (K + 1), [0] * (K + 1), [0] * (K + 1)
        self.updates = self.skipped = self.degenerate = self.since = 0
        self.trained = False

    def set_table(self, F):
        self.F = np.asarray(F, np.complex64).copy()
        self.trained = True

    def execute(self, x):
        """float64; an untrained handle copies (times the gain)"""
        if not self.trained:
            return np.asarray(x, np.complex64).astype(np.complex128) * (self.gain if self.gain != 1.0 else 1.0)
        return apply(self.F, x, self.table_log2, self.full_scale, self.gain)[0]

    def measure(self, u, z):
        """False, nothing measured, where the guard refuses"""
        u, z = np.asarray(u, np.complex64), np.asarray(z, np.complex64)
        if self.since + len(u) > (1 << GUARD_LOG2):
            return False
        self.since += len(u)
        j = bins(u, z, self.table_log2, self.full_scale)
        ok = j >= 0
        self.skipped += int(len(u) - ok.sum())
        sre, sim, suu = terms(u[ok], z[ok], self.e)
        jj = j[ok]
        for acc, add in ((self.cnt, np.ones(len(jj), np.int64)), (self.Sre, sre), (self.Sim, sim), (self.Suu, suu)):
            part = np.zeros(self.K + 1, np.int64)               # (2^28 terms below 2^34.1 fit an int64)
            np.add.at(part, jj, add)
            for b in np.nonzero(part)[0]:
                acc[b] += int(part[b])
        return True

    def update(self):
        F = update_table(self.cnt, self.Sre, self.Sim, self.Suu, self.K, self.step, self.g0, self.min_count)
        if F is None:
            self.degenerate += 1
        else:
            self.F = np.array([complex(np.float32(re), np.float32(im)) for re, im in F], np.complex64)
        s = self.forget_shift
        for acc in (self.cnt, self.Sre, self.Sim, self.Suu):
            acc[:] = [v >> s for v in acc]                      # Python's >> of a negative integer is the arithmetic shift
        self.since = (self.since + (1 << s) - 1) >> s
        self.updates += 1
        self.trained = True

    def accumulators(self):
        return tuple(np.array(v, np.int64) for v in (self.cnt, self.Sre, self.Sim, self.Suu))


def nmse_db(y, ref):
    y, ref = np.asarray(y, np.complex128), np.asarray(ref, np.complex128)
    return float(10.0 * np.log10(np.sum(np.abs(y - ref) ** 2) / np.sum(np.abs(ref) ** 2)))


# The end-to-end case (tests/test_dpd.py finds it on the oracle alone; tests/test_gpu_dpd.py runs exactly this): cfr_model.SEVERITY's
# transmitter and its stage (7 dB over the rms, two passes), then the predistorter with 128 bins whose full scale is twice the
# stream's peak, then a Rapp amplifier (p = 2) at 10 dB input back-off with 5 degrees of AM/PM and gain 1; three updates.
SEVERITY = dict(table_log2=7, full_scale_over_peak=2.0, amp_ibo_db=10.0, amp_smooth=2, amp_ampm_deg=5.0, amp_gain=1.0, rounds=3,
                edge=0.32, oob_gain_db=25.0, nmse_gain_db=30.0)
# The two-carrier case: channels 3 and 4 of 8 carry frames, no cfr; the back-off is the least whole number of dB that puts the stream's
# peak at or below 0.85 of the saturation amplitude (13 dB).
TWO_CARRIER = dict(first=3, count=2, peak_over_sat=0.85, table_log2=7, full_scale_over_peak=2.0, amp_smooth=2, amp_ampm_deg=5.0, rounds=3,
                   recorded_db={2: 2.25, 5: 2.12})      # what three updates take off channels 2 and 5 on this model (tests/test_dpd.py)
