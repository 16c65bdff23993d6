"""The per-user channel emulator (include/mcrx_hip.h, mcrx_hip_userchan_*) as numpy in float64, fed with the library's own integers.

    s_c[b] = sum_i a_ci x_c[b - d_ci]                table order
    r_c[b] = s_c[b] exp(+j 2 pi th / 2^32)           th = phase0_c + cfo_step_c (b mod 2^32) mod 2^32, the exact phase th / 2^32
    y_c[b] = gain_c r_c[b]
A channel is a dict(taps=[(delay, a), ...], gain_db=0.0, cfo_step=0, phase0=0, delay=0), as liquid_usrp_amd.userchan takes it; taps and gain
are taken as the fp32 values the handle holds.  When no channel of the table has a step or a start phase nothing is rotated, otherwise
every channel is (a zero phase rotates by exactly 1: the two are the same numbers here)."""
import numpy as np

MASK = (1 << 32) - 1


def gain_of(ch):
    return float(np.float32(10.0 ** (float(ch.get("gain_db", 0.0)) / 20.0)))


def rays_of(ch):
    """[(delay with the timing offset, the fp32 tap as a Python complex)]"""
    return [(int(d) + int(ch.get("delay", 0)), complex(np.complex64(complex(a)))) for d, a in ch["taps"]]


def lead_of(channels):
    """the handle's lead: the largest delay rounded up to 8"""
    return (max(d for ch in channels for d, _ in rays_of(ch)) + 7) // 8 * 8


def apply_channel(x, ch, first_block, lead):
    """x: the channel's samples of blocks [first_block - lead, first_block + n) -> y of blocks [first_block, first_block + n), complex128"""
    x = np.asarray(x, np.complex128)
    n = len(x) - lead
    s = np.zeros(n, np.complex128)
    for d, a in rays_of(ch):
        assert 0 <= d <= lead
        s += a * x[lead - d:lead - d + n]
    b = (np.arange(n, dtype=np.int64) + (int(first_block) & MASK)) & MASK           # b mod 2^32 (first_block may be negative or large)
    th = (int(ch.get("phase0", 0)) + int(ch.get("cfo_step", 0)) * b.astype(object)) % (1 << 32)
    s = s * np.exp(2j * np.pi * th.astype(np.float64) / 4294967296.0)
    return gain_of(ch) * s


def apply(x, channels, first_block, lead):
    """x[C, lead + n] (channel-major) -> y[C, n]"""
    return np.stack([apply_channel(x[c], ch, first_block, lead) for c, ch in enumerate(channels)])


def to_tiles(x):
    """x[C, nb] channel-major, nb % 8 == 0 -> the granules [nb / 8][C][8], flat"""
    C, nb = x.shape
    return np.ascontiguousarray(x.reshape(C, nb // 8, 8).transpose(1, 0, 2)).reshape(-1)


def from_tiles(t, C):
    """the inverse of to_tiles"""
    t = np.asarray(t).reshape(-1, C, 8)
    return np.ascontiguousarray(t.transpose(1, 0, 2)).reshape(C, -1)


def bound(ch, x):
    """per component, tests/test_gpu_chanemu.py's tap_bound for one channel: the fp32 rounding of 2T fused multiply-adds plus rotation
    and gain, and sincos_u32's stated error, against gain * sum|a_i| * max|x|"""
    rays = rays_of(ch)
    return ((2 * len(rays) + 8) * 2.0 ** -24 + 3e-7) * gain_of(ch) * sum(abs(a) for _, a in rays) * float(np.abs(x).max())
