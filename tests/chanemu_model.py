"""The channel emulator (include/mcrx_hip.h, mcrx_hip_chanemu_*) as numpy in float64 -- except the random integers, which are exact.

    s[n] = sum_i a_i x[n - d_i]          x[m] = 0 in front of the last reset
    r[n] = s[n] exp(+j 2 pi th_n / 2^32)  th_n = phase0 + cfo_step n mod 2^32
    v[n] = gain r[n] + noise_std w[n]
w[n]: Philox4x32-10, counter (lo32(n >> 1), hi32(n >> 1), 0, 0), key (lo32(seed), hi32(seed)); sample n takes the words w[j], w[j + 1],
j = 2 (n & 1); u1 = ((w[j] >> 9) + 0.5) 2^-23, u2 = (w[j + 1] >> 8) 2^-24, w[n] = sqrt(-2 ln u1) (cos 2 pi u2, sin 2 pi u2)."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four arrays (or ints) of 32-bit words, key: two -> the four output words as uint64 arrays holding 32-bit values"""
    c = [np.atleast_1d(np.asarray(v, np.uint64)) & MASK for v in ctr]
    k = [int(v) & 0xFFFFFFFF for v in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]             # 32 x 32 bits: fits 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k[0]), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k[1]), p0 & MASK]
        k = [(k[0] + W0) & 0xFFFFFFFF, (k[1] + W1) & 0xFFFFFFFF]
    return c


def words(seed, positions):
    """the two words every sample of `positions` (absolute indices, any 64-bit values) draws: uint32 [n, 2]"""
    pos = np.atleast_1d(np.asarray(positions, np.uint64))
    pair = pos >> np.uint64(1)
    w = philox4x32_10((pair & MASK, pair >> np.uint64(32), 0, 0), (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    odd = (pos & np.uint64(1)).astype(bool)
    return np.stack([np.where(odd, w[2], w[0]), np.where(odd, w[3], w[1])], axis=1).astype(np.uint32)


def positions(start, count):
    """absolute indices start .. start + count - 1 modulo 2^64, as uint64"""
    return (np.arange(count, dtype=np.uint64) + np.uint64(int(start) % (1 << 64)))


def noise(seed, start, count):
    """w[start .. start + count) as complex128"""
    w = words(seed, positions(start, count)).astype(np.float64)
    u1 = (np.floor(w[:, 0] / 512.0) + 0.5) * 2.0 ** -23
    u2 = np.floor(w[:, 1] / 256.0) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.exp(2j * np.pi * u2)


def apply(x, taps, cfo_step=0, phase0=0, gain=1.0, noise_std=0.0, seed=0, start=0):
    """the emulator's cf32 output for the stream x that begins at absolute index `start` behind a reset, in float64 (complex128).
    gain, noise_std and the taps are taken as the fp32 values the handle holds."""
    x = np.asarray(x, np.complex128)
    n = len(x)
    s = np.zeros(n, np.complex128)
    for d, a in taps:
        a = complex(np.complex64(a))
        if d < n:
            s[d:] += a * x[:n - d]
    idx = positions(start, n)
    if cfo_step or phase0:
        th = (np.uint64(int(phase0)) + np.uint64(int(cfo_step)) * (idx & MASK)) & MASK
        s = s * np.exp(2j * np.pi * th.astype(np.float64) / 4294967296.0)
    v = float(np.float32(gain)) * s
    if noise_std:
        v = v + float(np.float32(noise_std)) * noise(seed, start, n)
    return v
