"""The receiver calibration (include/mcrx_hip.h, mcrx_hip_rfcal_*) as a float64 model with the bounds the tests hold the library to.

    moments   cnt, S1 = sum u, S2 = sum u^2, P = sum |u|^2 as [S1.re, S1.im, S2.re, S2.im, P]
              sc16: exact integers of the int16 components; cf32: exactly rounded sums (math.fsum) of the exact fp64 products
    update    b = acc / cnt;  R = b, then R += mu_j (b - R), mu_j = max(1 / (j + 1), 2^-forget_log2);  m = R.s1, c2 = R.s2 - m^2,
              pc = R.p - |m|^2, w = c2 / (pc + sqrt(pc^2 - |c2|^2)) -- scalar Python floats, operation for operation the device's lane
    apply     t = u - m, y = t - w conj(t), v = gain y: in float64 from the fp32 coefficients (apply), and in emulated fp32 with the
              header's fmaf order (apply_fp32)

Bounds, each from the arithmetic:
  moment_bound   a cf32 block moment is a sum of n exact terms (2 n for S2.re and P, which add re^2 and im^2) taken in a fixed order
                 of depth at most d = terms + 6 (wave tree) + 3 (waves) + 96 (the fold: a thread's rows, its tree and waves, with
                 room) additions, and one more rounding where a row forms A - B, A + B: |error| <= (d + 1) u sum |term| (1 + d u), u = 2^-53 (Higham, recursive summation in any order).
  coef_bound     the update is some twenty fp64 operations, then one rounding to fp32.  With a relative perturbation delta of every
                 running mean, |d c2| <= delta (|s2| + 2 |m|^2), |d pc| <= delta (p + 2 |m|^2), and through den = pc + sqrt(D):
                 |d w| <= (|d c2| + |w| |d den|) / den, |d den| <= |d pc| + (pc |d pc| + |c2| |d c2|) / sqrt(D); delta = (8 + 4 j) u
                 after j updates (three roundings per recursion step, the weights sum to at most j); plus 2^-23 |w| for the fp32 store.
  apply_bound    fp32: t, the inner and the outer fmaf and the gain round once each, and the first three errors pass through
                 factors of at most (1 + |w.re| + |w.im|): |error| <= 5 * 2^-24 |gain| (1 + |w.re| + |w.im|) (|t.re| + |t.im|)
                 per component, plus the smallest normal for the flush of denormals."""
import math

import numpy as np

DC, IQ = 1, 2
U = 2.0 ** -53


def from_sc16(i):
    i = np.asarray(i, np.float64).reshape(-1, 2)
    return (i[:, 0] + 1j * i[:, 1]) * 2.0 ** -15


def moments_sc16(ints):
    """[S1.re, S1.im, S2.re, S2.im, P] as Python ints, in units of 2^-15 (S1) and 2^-30 (S2, P)"""
    a = np.asarray(ints).reshape(-1, 2).astype(np.int64)
    if len(a) > 4096:      # int64 numpy sums are exact here: |term| <= 2^31, fewer than 2^31 terms
        re_, im_ = a[:, 0], a[:, 1]
        return [int(re_.sum()), int(im_.sum()), int((re_ * re_).sum() - (im_ * im_).sum()), int(2 * (re_ * im_).sum()),
                int((re_ * re_).sum() + (im_ * im_).sum())]
    re, im = [int(v) for v in a[:, 0]], [int(v) for v in a[:, 1]]
    return [sum(re), sum(im), sum(r * r - i * i for r, i in zip(re, im)), sum(2 * r * i for r, i in zip(re, im)),
            sum(r * r + i * i for r, i in zip(re, im))]


def moments_cf32(x):
    """the exactly rounded sums, and sum |term| of each for moment_bound"""
    x = np.asarray(x, np.complex64)
    re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
    rr, ii, ri = re * re, im * im, re * im                  # exact: 24-bit factors
    mom = [math.fsum(re), math.fsum(im), math.fsum(np.concatenate([rr, -ii])), 2.0 * math.fsum(ri), math.fsum(np.concatenate([rr, ii]))]
    mag = [math.fsum(np.abs(re)), math.fsum(np.abs(im)), math.fsum(rr) + math.fsum(ii), 2.0 * math.fsum(np.abs(ri)), math.fsum(rr) + math.fsum(ii)]
    return mom, mag


def moment_bound(n, mag):
    out = []
    for k, s in enumerate(mag):
        d = (2 * n if k in (2, 4) else n) + 6 + 3 + 96
        out.append((d + 1) * U * s * (1.0 + d * U))
    return out


def mu(j, forget_log2):
    return max(1.0 / (float(j) + 1.0), 1.0 / float(1 << int(forget_log2)))


def closed_form(R):
    """(m, w) of the running means R, or None where the update keeps the previous coefficients"""
    mr, mi = R[0], R[1]
    c2r, c2i, pc = R[2] - (mr * mr - mi * mi), R[3] - 2.0 * (mr * mi), R[4] - (mr * mr + mi * mi)
    D = pc * pc - (c2r * c2r + c2i * c2i)
    if not pc > 0.0 or not D > 0.0 or not math.isfinite(D):
        return None
    den = pc + math.sqrt(D)
    return complex(mr, mi), complex(c2r / den, c2i / den)


class State(object):
    """what mcrx_hip_rfcal_read returns, kept by the model"""

    def __init__(self, stages=DC | IQ, forget_log2=30, sc16=False):
        self.stages, self.forget_log2, self.sc16 = int(stages), int(forget_log2), bool(sc16)
        self.m, self.w, self.mean = 0j, 0j, [0.0] * 5
        self.acc, self.count = [0] * 5 if sc16 else [0.0] * 5, 0
        self.updates = self.measured = self.degenerate = 0

    def measure(self, x):
        if self.sc16:
            mom, n = moments_sc16(x), len(np.asarray(x).reshape(-1, 2))
        else:
            mom, n = moments_cf32(x)[0], len(x)
        self.acc = [a + b for a, b in zip(self.acc, mom)]
        self.count += n
        self.measured += n

    def update(self, acc=None, count=None):
        """one update, of the model's own accumulators or of the ones given (the library's)"""
        acc, cnt = (self.acc if acc is None else acc), (self.count if count is None else count)
        if cnt == 0:
            return
        if self.sc16:
            b = [float(int(a)) * (2.0 ** -15 if k < 2 else 2.0 ** -30) / float(cnt) for k, a in enumerate(acc)]
        else:
            b = [float(a) / float(cnt) for a in acc]
        self.acc, self.count = [0] * 5 if self.sc16 else [0.0] * 5, 0
        if not all(math.isfinite(v) for v in b):
            self.degenerate += 1
            return
        w8 = mu(self.updates, self.forget_log2)
        self.mean = list(b) if self.updates == 0 else [r + w8 * (v - r) for r, v in zip(self.mean, b)]
        self.updates += 1
        mw = closed_form(self.mean)
        if mw is None:
            self.degenerate += 1
            return
        f32 = lambda z: complex(np.float32(z.real), np.float32(z.imag))
        self.m = f32(mw[0]) if self.stages & DC else 0j
        self.w = f32(mw[1]) if self.stages & IQ else 0j


def coef_bound(R, updates, summed=0):
    """(bound on |m - model m|, bound on |w - model w|) for coefficients made of the running means R.  summed = n: the means come from
    cf32 moments of n samples summed in another order as well: every mean then carries moment_bound's ds = (2 n + 106) u times the
    mean of |term| -- at most ds sqrt(p) for s1 (Cauchy-Schwarz) and ds p for s2 and p -- so c2 and pc move by at most 3 ds p more
    (their own sums, and 2 |m| ds sqrt(p) <= 2 ds p through m^2)."""
    delta = (8.0 + 4.0 * updates) * U
    ds = (2.0 * summed + 106.0) * U if summed else 0.0
    mw = closed_form(R)
    m2 = R[0] * R[0] + R[1] * R[1]
    bm = delta * math.hypot(R[0], R[1]) + 2.0 ** -23 * math.hypot(R[0], R[1]) + ds * math.sqrt(max(R[4], 0.0))
    if mw is None:
        return bm, 0.0
    w = mw[1]
    c2 = math.hypot(R[2] - (R[0] * R[0] - R[1] * R[1]), R[3] - 2.0 * R[0] * R[1])
    pc = R[4] - m2
    D = pc * pc - c2 * c2
    dc2, dpc = delta * (math.hypot(R[2], R[3]) + 2.0 * m2) + 3.0 * ds * R[4], delta * (R[4] + 2.0 * m2) + 3.0 * ds * R[4]
    dden = dpc + (pc * dpc + c2 * dc2) / math.sqrt(D)
    return bm, (dc2 + abs(w) * dden) / (pc + math.sqrt(D)) + 2.0 ** -23 * abs(w)


def apply(u, m, w, gain=1.0):
    """the corrected samples in float64: u complex (the fp32 or sc16 values), m, w the fp32 coefficients"""
    t = np.asarray(u, np.complex128) - complex(m)
    return float(gain) * (t - complex(w) * np.conj(t))


def apply_bound(u, m, w, gain=1.0):
    t = np.asarray(u, np.complex128) - complex(m)
    return 5.0 * 2.0 ** -24 * abs(float(gain)) * (1.0 + abs(w.real) + abs(w.imag)) * (np.abs(t.real) + np.abs(t.imag)) + 2.0 ** -126


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)      # the product is exact in float64


def apply_fp32(u, m, w, gain=1.0):
    """the header's fp32 sequence (each fmaf through float64: exact product, one sum, rounded to fp32 -- double rounding can differ from a
    true fmaf in the last bit, which apply_bound covers)"""
    u = np.asarray(u, np.complex64)
    f = np.float32
    tr, ti = u.real - f(m.real), u.imag - f(m.imag)
    wr, wi = np.full(len(u), f(w.real)), np.full(len(u), f(w.imag))
    yr = _fma32(-wr, tr, _fma32(-wi, ti, tr))
    yi = _fma32(wr, ti, _fma32(-wi, tr, ti))
    if float(gain) != 1.0:
        yr, yi = f(gain) * yr, f(gain) * yi
    return (yr + 1j * yi).astype(np.complex64)


def segments(pos, n, period_log2):
    """(lengths, ends_block) of the call (pos, n): cut at the multiples of 2^period_log2 of the absolute index (mod 2^64)"""
    if period_log2 == 0:
        return ([n], [False]) if n else ([], [])
    B, lens, ends, p = 1 << period_log2, [], [], pos % (1 << 64)
    while n:
        m = min(n, B - p % B)
        lens.append(m)
        ends.append((p + m) % B == 0)
        p, n = (p + m) % (1 << 64), n - m
    return lens, ends


def proper_noise(n, seed, rms=0.3):
    """circular complex Gaussian noise whose SAMPLE moments are exactly proper: mean 0, sum z^2 = 0 (float64)"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    if n < 4:                                               # (too few samples to constrain: plain noise)
        return z * (rms / math.sqrt(2.0))
    z -= z.mean()
    c = np.mean(z * z) / np.mean(np.abs(z) ** 2)            # z' = z - k conj(z) with k = c / (1 + sqrt(1 - |c|^2)) has mean z'^2 = 0
    z = z - c / (1.0 + math.sqrt(1.0 - abs(c) ** 2)) * np.conj(z)
    return z * (rms / math.sqrt(np.mean(np.abs(z) ** 2)))
