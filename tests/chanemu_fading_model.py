"""The channel emulator's fading rays (include/mcrx_hip.h, mcrx_hip_chanfade_*) as numpy in float64 -- except
the phases, which are exact 64-bit integers.

    B = 2^L, b = n >> L, n_b = (b << L) mod 2^64, e(p) = exp(2 pi j (p >> 32) / 2^32) for a 64-bit phase p
    G_i[b] = c_los_i e((psi_i << 32) + Lambda_i n_b) + c_sc_i sum_{k<S} e((Phi_ik << 32) + N_ik n_b)
    g_i(n) = G_i[b] + f (G_i[b+1] - G_i[b]),  f = (n & (B - 1)) 2^-L
    s[n]   = sum_i (g_i(n) a_i) x[n - d_i]
and what follows s[n] (rotation, gain, noise) is chanemu_model.apply with the one tap (0, 1).

A ray's table is (steps, phases, coef): steps[0], phases[0] the line-of-sight term, then the S scattered sinusoids; steps are signed
Python integers (2^64 * cycles per sample), phases 32-bit, coef = (c_los, c_sc) as the fp32 values the handle holds.  tables() makes them
from the fading seed as the library does; the GPU tests feed the model with the integers the library itself reports."""
import numpy as np

import chanemu_model as base

U64 = (1 << 64) - 1


def tables(seed, doppler, los_doppler, rice_k, los_phase, S):
    """one table per ray from the fading seed: Philox words of counter (k, i, 1, 0), alpha = 2 pi (k + w0 2^-32) / S, N = rint(f_d cos(alpha) 2^64)"""
    out = []
    for i in range(len(doppler)):
        k = np.arange(S, dtype=np.uint64)
        w = base.philox4x32_10((k, i, 1, 0), (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
        alpha = 2.0 * np.pi * (k.astype(np.float64) + w[0].astype(np.float64) * 2.0 ** -32) / float(S)
        steps = [int(np.rint(float(los_doppler[i]) * 2.0 ** 64))] + [int(v) for v in np.rint(float(doppler[i]) * np.cos(alpha) * 2.0 ** 64)]
        phases = [int(los_phase[i]) & 0xFFFFFFFF] + [int(v) for v in w[1]]
        K = float(np.float32(rice_k[i]))
        coef = (float(np.float32(np.sqrt(K / (K + 1.0)))), float(np.float32(np.sqrt(1.0 / ((K + 1.0) * S)))))
        out.append((steps, phases, coef, [int(v) for v in w[0]]))
    return out


def grid(table, rows, L):
    """G[b] for the grid rows b (uint64 array, each < 2^(64 - L)) as complex128"""
    steps, phases, coef = table[0], table[1], table[2]
    nb = np.asarray(rows, np.uint64) << np.uint64(L)                       # mod 2^64
    G = np.zeros(len(nb), np.complex128)
    with np.errstate(over="ignore"):
        for j, (st, ph) in enumerate(zip(steps, phases)):
            p = np.uint64((int(ph) << 32) & U64) + np.uint64(int(st) & U64) * nb          # wraps mod 2^64
            G += (coef[0] if j == 0 else coef[1]) * np.exp(2j * np.pi * (p >> np.uint64(32)).astype(np.float64) / 4294967296.0)
    return G


def gain(table, start, count, L):
    """g(n) for n = start .. start + count - 1 (mod 2^64) as complex128"""
    n = base.positions(start, count)
    mask = np.uint64(U64 >> L)
    b = n >> np.uint64(L)
    rel = ((b - b[0]) & mask).astype(np.int64)                            # rows relative to the first: the row index wraps with n
    rows = (b[0] + np.arange(int(rel.max()) + 2, dtype=np.uint64)) & mask
    G = grid(table, rows, L)
    f = (n & np.uint64((1 << L) - 1)).astype(np.float64) * 2.0 ** -L
    return G[rel] + f * (G[rel + 1] - G[rel])


def faded(x, taps, tabs, L, start=0):
    """s[n] for the stream x that begins at absolute index `start` behind a reset (complex128)"""
    x = np.asarray(x, np.complex128)
    n = len(x)
    s = np.zeros(n, np.complex128)
    for (d, a), t in zip(taps, tabs):
        if d < n:
            g = gain(t, start, n, L)
            s[d:] += (g[d:] * complex(np.complex64(a))) * x[:n - d]
    return s


def apply(x, taps, tabs, L, cfo_step=0, phase0=0, gain=1.0, noise_std=0.0, seed=0, start=0):
    """the fading emulator's cf32 output in float64"""
    return base.apply(faded(x, taps, tabs, L, start), [(0, 1.0)], cfo_step, phase0, gain, noise_std, seed, start)
