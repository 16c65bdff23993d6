"""Each user's own sample clock and fractional timing in the per-user channel emulator (include/mcrx_hip.h, mcrx_hip_userclock_*;
DESIGN.md section 4.17): the integers as Python integers, the coefficients as an exact fp32 restatement, and the stage in float64.

    tau_fp(b) = delay_fp + floor(sco (b - origin) / 2^16)       Q32 samples; n = tau_fp >> 32, mu = tau_fp & 0xffffffff
    z[b]      = sum_{j<32} h_j(mu) x[b - n + 15 - j]
    h_j(mu)   = fmaf(f, W[r+1][j] - W[r][j], W[r][j])           r = mu >> 26, f = ((mu >> 2) & 0xffffff) 2^-24
    W[p][j]   = sinc(t) I0(6 sqrt(1 - (t / 16)^2)) / I0(6)      t = j - 15 - p / 64; rows 0 and 64 the unit vectors of taps 15 and 16
and what follows z (rays, fading gains, rotation, level) is userchan_model's / userchan_fading_model's, on z in place of x.

A user is None (no clock: z = x) or a dict(delay_fp, sco, origin) of integers.  The GPU tests feed the model with the table the library
reports (mcrx_hip_userclock_table), so the model's h is the library's up to its fp32 roundings, which bound() counts."""
from fractions import Fraction

import numpy as np

TAPS, PHASES, MIN_DELAY = 32, 64, 15


def table_f64():
    """W[65][32] from the formula in double (numpy's I0), the two end rows exact"""
    p, j = np.arange(PHASES + 1, dtype=np.float64)[:, None], np.arange(TAPS, dtype=np.float64)[None, :]
    t = j - 15.0 - p / PHASES
    w = np.sinc(t) * np.i0(6.0 * np.sqrt(np.maximum(1.0 - (t / 16.0) ** 2, 0.0))) / np.i0(6.0)
    w[0], w[PHASES] = np.eye(TAPS)[15], np.eye(TAPS)[16]
    return w


def user_of(delay, ppm=0.0, origin=0):
    """the integers liquid_usrp_amd.userclock_user makes of a delay in samples and a clock error in ppm"""
    return dict(delay_fp=int(np.rint(float(delay) * 2.0 ** 32)), sco=int(np.rint(float(ppm) * 1e-6 * 2.0 ** 48)), origin=int(origin))


def tau_fp(user, b):
    """Python integers: >> is floor"""
    return int(user["delay_fp"]) + ((int(user["sco"]) * (int(b) - int(user["origin"]))) >> 16)


def split(tau):
    """(n, mu, r, the 24 bits of f)"""
    mu = tau & 0xFFFFFFFF
    return tau >> 32, mu, mu >> 26, (mu >> 2) & 0xFFFFFF


def f32_round(q):
    """the fp32 value nearest to the Fraction q, ties to even (normal and subnormal range; no overflow here)"""
    if q == 0:
        return 0.0
    s, q = (-1.0 if q < 0 else 1.0), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length() - 24
    while q >= Fraction(2) ** (e + 24):
        e += 1
    while q < Fraction(2) ** (e + 23):
        e -= 1
    e = max(e, -149)
    m = q / Fraction(2) ** e
    k = m.numerator // m.denominator
    rem = m - k
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (k & 1)):
        k += 1
    return s * float(k) * 2.0 ** e


def coefs_f32(W32, mu):
    """h_j(mu) as the library computes it, exactly: the difference of the rows rounded to fp32, then ONE rounding of f d + w0"""
    r, f = mu >> 26, Fraction((mu >> 2) & 0xFFFFFF, 1 << 24)
    out = []
    for j in range(TAPS):
        w0, w1 = float(W32[r, j]), float(W32[r + 1, j])
        d = float(np.float32(w1) - np.float32(w0))
        out.append(f32_round(f * Fraction(d) + Fraction(w0)))
    return np.array(out, dtype=np.float32)


def coefs_f64(W32, mu):
    """h(mu)[..., 32] in float64 for an array of fractions: the rows' difference as fp32 (the library's), the rest unrounded"""
    mu = np.asarray(mu, dtype=np.int64)
    r, f = mu >> 26, ((mu >> 2) & 0xFFFFFF).astype(np.float64) * 2.0 ** -24
    w0, d = W32[r].astype(np.float64), (W32[r + 1] - W32[r]).astype(np.float64)
    return w0 + f[..., None] * d


def z_channel(x, user, W32, first_block, lead, zlead):
    """x: the channel's samples of blocks [first_block - lead, first_block + n) -> (z of blocks [first_block - zlead, first_block + n) as
    complex128, the largest sum_j |h_j| used, the smallest and largest n used)"""
    x = np.asarray(x, np.complex128)
    nb = len(x) - lead + zlead
    if user is None:
        return x[lead - zlead:].copy(), 1.0, 0, 0
    taus = [tau_fp(user, int(first_block) - zlead + m) for m in range(nb)]
    n = np.array([t >> 32 for t in taus], dtype=np.int64)
    h = coefs_f64(np.asarray(W32, np.float32), np.array([t & 0xFFFFFFFF for t in taus], dtype=np.int64))
    idx = (lead - zlead + np.arange(nb) - n + 15)[:, None] - np.arange(TAPS)[None, :]
    assert idx.min() >= 0 and idx.max() < len(x), (idx.min(), idx.max(), len(x))
    return (h * x[idx]).sum(axis=1), float(np.abs(h).sum(axis=1).max()), int(n.min()), int(n.max())


def z_bound(W32, hsum, x):
    """Per component, |fp32 z - model z| for one channel.  With X = max |x| (each component is at most that), H = the largest sum_j |h_j|
    of the blocks computed and Dw = the largest sum_j |W[r+1][j] - W[r][j]| over the rows: the 32 fused multiply-adds round 32 partial
    sums, each at most H X in magnitude: 32 2^-24 H X; the coefficient's own fused multiply-add rounds h_j once, 2^-24 |h_j| each:
    2^-24 H X; and the rows' difference is rounded to fp32 before it is scaled by f < 1: 2^-24 Dw X."""
    W32 = np.asarray(W32, np.float32).astype(np.float64)
    dw = float(np.abs(W32[1:] - W32[:-1]).sum(axis=1).max())
    return (33.0 * hsum + dw) * 2.0 ** -24 * float(np.abs(x).max())


def frequency_error_db(W32, fmax, nmu, nf):
    """the worst |sum_j h_j e^{-2 pi i f (j - 15)} - e^{-2 pi i f mu}| over mu = k / nmu and nf frequencies of |f| <= fmax, in dB"""
    mu = (np.arange(nmu, dtype=np.int64) << 32) // nmu
    h = coefs_f64(np.asarray(W32, np.float32), mu)
    f = np.linspace(-fmax, fmax, nf)
    E = np.exp(-2j * np.pi * f[:, None] * (np.arange(TAPS) - 15.0)[None, :])                 # [nf, 32]
    want = np.exp(-2j * np.pi * f[None, :] * (mu.astype(np.float64) * 2.0 ** -32)[:, None])  # [nmu, nf]
    return 20.0 * np.log10(float(np.abs(h @ E.T - want).max()))
