"""The multi-stage resampler (csrc/msresamp.hip) in float64, with a rounding bound beside every output
component.  Plain numpy, vectorised; fed with the plan's own integers and its fp32 taps widened to float64
(liquid_usrp_amd.msresamp_plan), so that it shares no arithmetic with the library but the design of the taps -- and those are held
against an independent design in tests/test_resamp_model.py.

The chain, from the closed forms at the top of msresamp.hip (samples before sample 0 are zeros):
  half-band decimator     y[k] = 0.5 (x[2k-13] + sum_{i<14} h1[i] x[2(k-13+i)]),  k < floor(nin / 2)
  arbitrary stage         n_j = (j step) >> 24,  b_j = ((j step) mod 2^24) >> 16,  y[j] = sum_{k<14} H[b_j][k] x[n_j-13+k],  every j with n_j < nin
  half-band interpolator  v[2k] = u[k-7],  v[2k+1] = sum_{i<14} h1[i] u[k-13+i]
rate <= 1: num_stages decimators, then the arbitrary stage; rate > 1: the arbitrary stage, then num_stages interpolators.  The last stage's
store multiplies by the output gain; an sc16 handle stores Q of that fp32 value (tx_sc16_model.py), and an sc16 input sample (re, im)
means (re, im) 2^-15 exactly.

The bound.  u = 2^-24 is one fp32 rounding, relative.  Every stage's input component x carries a bound d >= |computed - model|.
  * a 14-tap sum s = sum h x, accumulated in any order with or without fused multiply-adds, is off by at most gamma_14 sum |h| |x|,
    gamma_14 = 14 u / (1 - 14 u), for its own roundings (the first product is added to zero, so each term passes through at most 14
    roundings), and passes the bounds of its inputs on as sum |h| d;
  * the half-band decimator adds the delayed sample (bound d) and rounds once more, u |x[2k-13] + s|; the halving is exact;
  * the interpolator's even outputs are copies: the bound of u[k-7] unchanged;
  * a gain other than 1 multiplies the bound by |gain| and rounds once more, u |gain y|; a gain of 1 is exact and costs nothing.
Underflow: a result below 2^-126 is rounded absolutely, not relatively (to a multiple of 2^-149, or to zero where denormals are flushed),
so every rounding above also costs up to T = 2^-126: 14 T a sum, T for the decimator's add and halving, T for the gain.  It matters only
where a deep chain's first outputs are made of a few samples times the products of small taps (1e-45 at fifteen stages).
The magnitudes on the right are the model's, not the computed ones: they differ by the bound itself, a term of second order, for which
0.1 % is added.  Nothing in the bound is fitted; every comparison that uses it also holds the max-norm error to 1e-5 of the model's peak
(REL), because sum |h1| = 1.995 doubles the bound per half-band interpolator and it becomes pessimistic for deep chains."""
import numpy as np

import tx_sc16_model as q16

U = 2.0 ** -24
G14 = 14.0 * U / (1.0 - 14.0 * U)
TINY = 2.0 ** -126      # the least normal fp32
SECOND_ORDER = 1.001
REL = 1e-5              # tests/test_gpu_parity.py's bar: max-norm error over the reference's peak
TAPS, M, PHASE_BITS, NPFB_BITS = 14, 7, 24, 8


def as_pairs(x):
    """complex samples -> float64 [n, 2]"""
    x = np.ascontiguousarray(x, np.complex128)
    return x.view(np.float64).reshape(-1, 2).copy()


def as_complex(v):
    return np.ascontiguousarray(v, np.float64).view(np.complex128).reshape(-1)


def from_sc16(w):
    """int16 [n, 2] -> the complex samples they mean"""
    return as_complex(np.asarray(w, np.int16).reshape(-1, 2).astype(np.float64) * 2.0 ** -15)


def _front(a, n):
    return np.concatenate([np.zeros((n, 2)), a])


def halfband_decim(v, d, h1):
    n = len(v) // 2
    vp, dp = _front(v, 26), _front(d, 26)               # vp[t + 26] = x[t]
    s, sa, sd = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2))
    for i in range(TAPS):
        sl = slice(2 * i, 2 * i + 2 * n, 2)             # x[2 (k - 13 + i)]
        s += h1[i] * vp[sl]
        sa += abs(h1[i]) * np.abs(vp[sl])
        sd += abs(h1[i]) * dp[sl]
    od = slice(13, 13 + 2 * n, 2)                       # x[2 k - 13]
    y = 0.5 * (vp[od] + s)
    return y, 0.5 * (dp[od] + sd + G14 * sa + TAPS * TINY) + U * np.abs(y) + TINY


def arbitrary_indices(step, nin):
    """(n_j, b_j) of every output j of the arbitrary stage on nin input samples"""
    nout = -((-nin << PHASE_BITS) // step)              # the first j with j step >= nin 2^24
    ph = np.arange(nout, dtype=np.uint64) * np.uint64(step)
    return (ph >> np.uint64(PHASE_BITS)).astype(np.int64), ((ph & np.uint64((1 << PHASE_BITS) - 1)) >> np.uint64(PHASE_BITS - NPFB_BITS)).astype(np.int64)


def arbitrary(v, d, step, H):
    nj, bj = arbitrary_indices(step, len(v))
    vp, dp = _front(v, TAPS - 1), _front(d, TAPS - 1)   # vp[t + 13] = x[t]
    s, sa, sd = np.zeros((len(nj), 2)), np.zeros((len(nj), 2)), np.zeros((len(nj), 2))
    for k in range(TAPS):
        h = H[bj, k][:, None]
        s += h * vp[nj + k]
        sa += np.abs(h) * np.abs(vp[nj + k])
        sd += np.abs(h) * dp[nj + k]
    return s, sd + G14 * sa + TAPS * TINY


def halfband_interp(v, d, h1):
    n = len(v)
    vp, dp = _front(v, TAPS - 1), _front(d, TAPS - 1)   # vp[t + 13] = u[t]
    s, sa, sd = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2))
    for i in range(TAPS):
        s += h1[i] * vp[i:i + n]
        sa += abs(h1[i]) * np.abs(vp[i:i + n])
        sd += abs(h1[i]) * dp[i:i + n]
    y, e = np.empty((2 * n, 2)), np.empty((2 * n, 2))
    y[0::2], e[0::2] = vp[TAPS - 1 - M:TAPS - 1 - M + n], dp[TAPS - 1 - M:TAPS - 1 - M + n]
    y[1::2], e[1::2] = s, sd + G14 * sa + TAPS * TINY
    return y, e


def count_out(plan, nin):
    """outputs of a fresh handle on nin input samples"""
    if plan.interp:
        return -((-nin << PHASE_BITS) // plan.step) << plan.num_stages
    return -((-(nin >> plan.num_stages) << PHASE_BITS) // plan.step)


def nin_for(plan, nout):
    """the fewest input samples on which a fresh handle makes at least nout outputs (interpolators make them in runs)"""
    lo, hi = 0, 1
    while count_out(plan, hi) < nout:
        hi *= 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if count_out(plan, mid) >= nout else (mid, hi)
    return hi


def run(plan, x, gain=1.0):
    """(y, bound): the outputs of a fresh handle on the complex samples x as complex128, and the bound of every component as float64
    [nout, 2].  x are the samples the handle means: fp32 values (or from_sc16's) widened."""
    h1, H = plan.h1.astype(np.float64), plan.hpfb.astype(np.float64)
    v = as_pairs(x)
    d = np.zeros_like(v)
    if plan.interp:
        v, d = arbitrary(v, d, plan.step, H)
        for _ in range(plan.num_stages):
            v, d = halfband_interp(v, d, h1)
    else:
        for _ in range(plan.num_stages):
            v, d = halfband_decim(v, d, h1)
        v, d = arbitrary(v, d, plan.step, H)
    g = float(np.float32(gain))
    if g != 1.0:
        v = v * g
        d = abs(g) * d + U * np.abs(v) + TINY
    assert len(v) == count_out(plan, len(x))
    return as_complex(v), d * SECOND_ORDER


def compare(got, y, bound):
    """(worst fraction of the bound, max-norm error over the model's peak) of complex64 outputs against run()'s; components whose bound is
    zero must be equal and count as 0 (or inf)"""
    err = np.abs(as_pairs(got) - as_pairs(y))
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return (float(frac.max()) if len(frac) else 0.0), (float(err.max() / np.abs(as_pairs(y)).max()) if len(err) else 0.0)


def quantised(y, gain=1.0):
    """what an sc16-output handle stores for fp32 outputs y of a cf32 handle of the same gain (that handle has multiplied already):
    (int16 [n, 2], clipped samples)"""
    y = np.ascontiguousarray(y, np.complex64)
    return q16.quantise_iq(y), q16.clipped_samples(y)


def true_rate(plan):
    """output samples per input sample, exactly as the integers make it"""
    r = float(1 << PHASE_BITS) / plan.step
    return r * 2.0 ** plan.num_stages if plan.interp else r / 2.0 ** plan.num_stages


def delay_tone(plan, nslow=600):
    """(x, f_in): a tone of 0.01 cycles per sample of the slower side, long enough for nslow samples of that side behind the transient"""
    r = true_rate(plan)
    f_in = 0.01 * min(r, 1.0)
    nin = int(3 * plan.delay + 64 + nslow / min(r, 1.0))
    return np.exp(2j * np.pi * f_in * np.arange(nin)).astype(np.complex64), f_in


def fit_delay(plan, y, f_in):
    """The delay D in input samples that the outputs y of delay_tone show: y[m] = A exp(j 2 pi f_in (m / rate - D)) behind the
    transient, from the phase of the mean of y[m] exp(-j 2 pi f_in m / rate) there."""
    r = true_rate(plan)
    m = np.arange(len(y))
    skip = int(2 * plan.delay * r) + 32
    assert len(y) > skip + 100
    z = np.asarray(y, np.complex128)[skip:] * np.exp(-2j * np.pi * f_in * m[skip:] / r)
    return float(-np.angle(z.mean()) / (2.0 * np.pi * f_in))


def delay_tolerance(plan):
    """Input samples.  The phase is quantised to 1/256 of an arbitrary-stage input sample (0.0039); the branch table drops the last tap
    of the 3585-tap prototype, measured on the model as at most 0.0061 at rate 0.5: 0.010, and half as much again.  An arbitrary-stage
    input sample of a decimating handle is 2^num_stages input samples."""
    return 0.015 * (1.0 if plan.interp else 2.0 ** plan.num_stages)
