"""Model of the amplifier with memory (mcrx_hip_pamem_*; the definition is in include/mcrx_hip.h): the parallel Hammerstein sum in
float64 numpy from the closed forms, each branch rfchain_model.amplifier on that branch's configuration; beside it a bound for what the
fp32 arithmetic of the definition may differ from it; the sc16 codec and the clip count through the shared model (tx_sc16_model).

A configuration is the product's PamemConfig (product.pamem_config(...)): its fields are the fp32 values the handle holds.

The bound, per component, eps = 2^-24 (one fp32 rounding, relative), SC = 3e-7 (sincos_u32's error), term by term:
  amplifier   a_b[s] = A_b(u[s]) differs from the model's by at most e_b[s] = g_b |u[s]| (6 eps + [ampm_b != 0] (2 pi (6 eps |ampm_b| +
              2^-33) + sqrt2 (SC + 2 eps))): tests/test_gpu_rfchain.py's amplifier bound with nothing carried in (the input is exact).
  a term      h a moves a component by at most c e, c = |h.re| + |h.im|, for the error carried in by a, and is itself at most
              m = c (|a| + sqrt2 e) in magnitude (a component of a is at most |a|).
  the chain   the first term is a product and an fmaf: eps |h.im a.y| for the product, eps |result| for the fmaf, together at most
              2 eps m_1.  A later term is two nested fmaf onto the accumulator: each rounds a partial sum that is at most
              P_j = m_1 + ... + m_j in magnitude: 2 eps P_j.  With P_1 = m_1 the chain adds 2 eps sum_j P_j.
  gain        one multiply: e' = |gain| (e + eps |y|); skipped at gain 1.
Second-order terms (a rounding of a rounding error) are covered by the factor 1.01 at the end, as in mpd_model.apply."""
import math

import numpy as np

import rfchain_model
import tx_sc16_model as q16

EPS, SC, SQ2 = 2.0 ** -24, 3e-7, math.sqrt(2.0)
MAX_BRANCHES, MAX_TAPS, MAX_DELAY = 4, 8, 16


class BranchAmp(object):
    """branch b of a PamemConfig with the field names rfchain_model.amplifier reads"""

    def __init__(self, br):
        self.amp_sat, self.amp_gain, self.amp_ampm, self.amp_smooth = float(br.sat), float(br.amp_gain), float(br.ampm), int(br.smooth)


def branches_of(cfg):
    """[(BranchAmp, [(delay, complex weight), ...]), ...] of a PamemConfig"""
    out = []
    for b in range(int(cfg.branches)):
        br = cfg.branch[b]
        out.append((BranchAmp(br), [(int(br.delay[k]), complex(float(br.h_re[k]), float(br.h_im[k]))) for k in range(int(br.taps))]))
    return out


def lead_of(cfg):
    return max(d for _, taps in branches_of(cfg) for d, _ in taps)


def inv_sat2(cfg):
    """r_b as fp32 values: the host's"""
    return [np.float32(rfchain_model.inv_sat2(amp)) for amp, _ in branches_of(cfg)]


def flat_taps(cfg):
    """[(branch, delay, weight), ...] in the order the sum runs: branch ascending, then tap ascending"""
    return [(b, d, h) for b, (_, taps) in enumerate(branches_of(cfg)) for d, h in taps]


def to_float(cfg, x):
    """the input as complex128: complex samples, or int16 [n, 2] on an sc16-in configuration"""
    return rfchain_model.from_sc16(x) if int(cfg.input_format) == 1 else np.asarray(x, np.complex128)


def amp_bound(amp, u):
    """e_b[s]: per component, what the device's A_b(u[s]) may differ from rfchain_model.amplifier's"""
    g, am = abs(amp.amp_gain), abs(amp.amp_ampm)
    own = 6 * EPS + ((2 * np.pi * (6 * EPS * am + 2.0 ** -33) + SQ2 * (SC + 2 * EPS)) if am else 0.0)
    return g * np.abs(u) * own


def apply(cfg, x, shift=None):
    """(y, bound): the cf32 output for lead + n input samples x (the history in front) in float64, n complex128; bound [n] per
    component, the module docstring's.  shift = (flat tap index, samples): that tap's delay moved, a model broken on purpose."""
    u = to_float(cfg, x)
    lead = lead_of(cfg)
    n = len(u) - lead
    assert n >= 0
    y, e, P, S = np.zeros(n, np.complex128), np.zeros(n), np.zeros(n), np.zeros(n)
    at = 0
    for amp, taps in branches_of(cfg):
        a, ea = rfchain_model.amplifier(amp, u), amp_bound(amp, u)
        for d, h in taps:
            if shift is not None and shift[0] == at:
                d = min(max(d + shift[1], 0), lead)
            c = abs(h.real) + abs(h.imag)
            seg, es = a[lead - d:lead - d + n], ea[lead - d:lead - d + n]
            y = y + h * seg
            e = e + c * es
            P = P + c * (np.abs(seg) + SQ2 * es)
            S = S + P
            at += 1
    e = e + 2 * EPS * S
    g = float(cfg.gain)
    if g != 1.0:
        y, e = g * y, abs(g) * (e + EPS * np.abs(y))
    return y, 1.01 * e


def quantise(y):
    """(int16 [n, 2], clipped samples) of the fp32 values a cf32 handle stored"""
    return q16.quantise_iq(y), q16.clipped_samples(y)


def small_signal(cfg):
    """H[0 .. lead] complex128: H[d] = sum over the taps at delay d of gain_b h -- the linear regime's FIR, from the definition"""
    H = np.zeros(lead_of(cfg) + 1, np.complex128)
    for amp, taps in branches_of(cfg):
        for d, h in taps:
            H[d] += amp.amp_gain * h
    return H
