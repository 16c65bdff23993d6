"""The RF front end (include/mcrx_hip.h, mcrx_hip_rfchain_*) as numpy in float64 -- except the oscillator's integers, which are exact.

A configuration is the product's RfchainConfig (product.rfchain_config(...)): its fields are the fp32 values the handle holds.  The
oscillator's integers (steps N_k, phases Phi_k, coefficient c) come from the library's selftest (product.rfchain_integers) or from
integers() below, the model's own derivation from the seed.

    mixer       u = alpha z + beta conj(z) + d
    oscillator  u = z exp(2 pi j theta(n)),  theta(n) = Theta[b] + f (Theta[b+1] - Theta[b]),  b = n >> L, f = (n & (B-1)) / B
                Theta[b] = c sum_k cos 2 pi ((((Phi_k << 32) + N_k n_b) mod 2^64) >> 32) / 2^32,  n_b = (b << L) mod 2^64   [turns]
    amplifier   u = G z exp(2 pi j phi),  t = |z|^2 r,  G = amp_gain (1 + t^p)^(-1/(2p)),  phi = ampm t / (1 + t)           [turns]
    order 0: mixer, oscillator, amplifier; order 1: amplifier, oscillator, mixer; v = gain u."""
import math

import numpy as np

from chanemu_model import philox4x32_10, positions

MIXER, OSCILLATOR, AMPLIFIER = 1, 2, 4
U64 = np.uint64


def integers(seed, sinusoids, log2_block, bandwidth, rms):
    """(steps, phases, c): the Philox words of counter (k, 0, 3, 0) under key `seed` -> a stratified draw from a Lorentzian line.
    Scalar double arithmetic with the C library's tan, operation for operation what the header writes down."""
    S, fmax = int(sinusoids), 0.125 / float(1 << int(log2_block))
    w = philox4x32_10((np.arange(S), 0, 3, 0), (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    steps = []
    for k in range(S):
        u = (float(k) + (float(int(w[0][k])) + 0.5) * 2.0 ** -32) / float(S)
        f = min(max(float(bandwidth) * math.tan(math.pi * (u - 0.5)), -fmax), fmax)
        steps.append(int(np.rint(f * 2.0 ** 64)))
    c = float(np.float32(float(np.float32(rms)) * math.sqrt(2.0 / S) / (2.0 * math.pi)))
    return steps, [int(v) for v in w[1]], c


def theta_rows(ints, log2_block, rows):
    """Theta[b] in turns (float64) for the grid rows `rows` (any 64-bit values)"""
    steps, phases, c = ints
    b = np.atleast_1d(np.asarray(rows, U64))
    nb = np.left_shift(b, U64(int(log2_block)))                         # mod 2^64
    acc = np.zeros(len(b), np.float64)
    for N, P in zip(steps, phases):
        ph = (U64(int(P)) << U64(32)) + U64(int(N) % (1 << 64)) * nb    # uint64 arrays wrap
        acc += np.cos(2.0 * np.pi * (ph >> U64(32)).astype(np.float64) / 4294967296.0)
    return c * acc


def theta(ints, log2_block, idx):
    """theta(n) in turns for the absolute indices idx (uint64)"""
    L = U64(int(log2_block))
    idx = np.asarray(idx, U64)
    b = idx >> L
    f = (idx & ((U64(1) << L) - U64(1))).astype(np.float64) / float(1 << int(log2_block))
    rows, inv = np.unique(np.concatenate([b, b + U64(1)]), return_inverse=True)
    T = theta_rows(ints, log2_block, rows)
    T0, T1 = T[inv[:len(b)]], T[inv[len(b):]]
    return T0 + f * (T1 - T0)


def mixer(cfg, z):
    al, be, d = complex(cfg.alpha_re, cfg.alpha_im), complex(cfg.beta_re, cfg.beta_im), complex(cfg.dc_re, cfg.dc_im)
    return al * z + be * np.conj(z) + d


def oscillator(z, th):
    return z * np.exp(2j * np.pi * th)


def inv_sat2(cfg):
    return float(np.float32(1.0 / (float(cfg.amp_sat) * float(cfg.amp_sat))))


def amplifier(cfg, z):
    p = int(cfg.amp_smooth)
    t = np.abs(z) ** 2 * inv_sat2(cfg)
    G = float(cfg.amp_gain) * (1.0 + t ** p) ** (-1.0 / (2.0 * p))
    return G * z * np.exp(2j * np.pi * float(cfg.amp_ampm) * t / (1.0 + t))


def sequence(cfg):
    """the stages that are on, in the order they run"""
    on = [s for s in (MIXER, OSCILLATOR, AMPLIFIER) if int(cfg.stages) & s]
    return on if int(cfg.order) == 0 else on[::-1]


def from_sc16(i):
    """int16 [n, 2] -> complex128, a word meaning (re, im) * 2^-15"""
    i = np.asarray(i, np.float64)
    return (i[:, 0] + 1j * i[:, 1]) * 2.0 ** -15


def apply(cfg, x, first_sample=0, ints=None):
    """the front end's cf32 output for the samples x (complex, or int16 [n, 2] on an sc16-in configuration) that begin at absolute
    index first_sample, in float64 (complex128)"""
    z = from_sc16(x) if int(cfg.input_format) == 1 else np.asarray(x, np.complex128)
    for s in sequence(cfg):
        if s == MIXER:
            z = mixer(cfg, z)
        elif s == OSCILLATOR:
            z = oscillator(z, theta(ints, int(cfg.pn_log2_block), positions(first_sample, len(z))))
        else:
            z = amplifier(cfg, z)
    return float(cfg.gain) * z


# The end-to-end case (tests/test_rfchain.py finds these on the oracle alone; tests/test_gpu_rfchain.py runs exactly these):
# N = 8, M = 64, three frames per channel, QPSK / Hamming(12,8); IQ imbalance and phase noise at each end, the amplifier in the
# transmitter, white noise between, sc16 out of the receive chain with the peak at half of full scale.
SEVERITY = dict(N=8, M=64, cp=8, taper=4, frames=3, payload_len=96,
                iq_gain_db=0.5, iq_phase_deg=3.0, pn_rms_deg=1.0, pn_bandwidth=1e-5, pn_seed_tx=11, pn_seed_rx=12,
                amp_smooth=2, amp_ibo_db=8.0, amp_ampm_deg=5.0, snr_db=25.0, noise_seed=2024, peak=0.5)


def severity_chains(product, rms):
    """the two keyword sets of the end-to-end case: (transmit chain, receive chain without its gain) for a signal of amplitude rms"""
    s = SEVERITY
    pn = dict(rms_deg=s["pn_rms_deg"], bandwidth=s["pn_bandwidth"])
    tx = dict(order="tx", mixer=product.rfchain_iq(s["iq_gain_db"], s["iq_phase_deg"], "tx"), phase_noise=dict(pn, seed=s["pn_seed_tx"]),
              amplifier=dict(sat=product.rfchain_backoff(s["amp_ibo_db"], rms), smooth=s["amp_smooth"], ampm_deg=s["amp_ampm_deg"]))
    rx = dict(order="rx", mixer=product.rfchain_iq(s["iq_gain_db"], s["iq_phase_deg"], "rx"), phase_noise=dict(pn, seed=s["pn_seed_rx"]))
    return tx, rx
