"""Crest-factor reduction (include/mcrx_hip.h, mcrx_hip_cfr_*) as numpy in float64.

The model takes the handle's own fp32 numbers: the threshold A (float(cfg.threshold)), A2 = fp32(A * A) and the taps h[0 .. H].

    t    = |x|^2
    e[n] = (1 - A / sqrt(t)) x[n]  where t > A2, else 0
    c[n] = h[0] e[n] + sum_{k=1..H} h[k] (e[n-k] + e[n+k])
    y[n] = x[n] - c[n]

One pass maps m + 2 H samples to m; P passes map n + 2 P H samples to n; v = gain y.  Beside it: the measures the tests quote (PAPR,
the share of the power beyond a band edge) and the committed values of the end-to-end cases."""
import numpy as np


def threshold2(A):
    """A2 = fp32(A * A), the product in double"""
    return float(np.float32(float(A) * float(A)))


def lowpass(half_len, cutoff, beta):
    """the design formula in float64, before the rounding to fp32: h[k] = 2 fc sinc(2 fc k) w(k), k = 0 .. H, with the Kaiser window
    w(k) = I0(beta sqrt(1 - (2 k / (2 H + 1))^2)) / I0(beta), scaled so that h[0] + 2 sum h[k] = 1"""
    k = np.arange(int(half_len) + 1, dtype=np.float64)
    r = 2.0 * k / (2.0 * half_len + 1.0)
    h = 2.0 * cutoff * np.sinc(2.0 * cutoff * k) * np.i0(beta * np.sqrt(1.0 - r * r)) / np.i0(beta)
    return h / (h[0] + 2.0 * h[1:].sum())


def response(h, f):
    """the (real) frequency response of the symmetric filter h[0 .. H] at the frequencies f, cycles per sample"""
    h = np.asarray(h, np.float64)
    k = np.arange(1, len(h))
    return h[0] + 2.0 * np.cos(2.0 * np.pi * np.outer(np.atleast_1d(f), k)) @ h[1:]


def excess(x, A):
    """e of every sample, and which samples exceed the threshold"""
    x = np.asarray(x, np.complex128)
    t = x.real * x.real + x.imag * x.imag
    with np.errstate(invalid="ignore"):
        over = t > threshold2(A)
    s = np.zeros(len(x))
    s[over] = 1.0 - float(A) / np.sqrt(t[over])
    return s * np.where(over, x, 0.0), over


def full_taps(h):
    h = np.asarray(h, np.float64)
    return np.concatenate([h[:0:-1], h])


def one_pass(x, A, h):
    """m + 2 H samples -> (y, e, over): y the m samples in the middle corrected, e and over of all the input samples"""
    x = np.asarray(x, np.complex128)
    H = len(h) - 1
    e, over = excess(x, A)
    c = np.convolve(e, full_taps(h), mode="valid")
    return x[H:len(x) - H] - c, e, over


def apply(x, A, h, passes=1, gain=1.0):
    """n + 2 P H samples -> the n output samples, float64 (complex128)"""
    y = np.asarray(x, np.complex128)
    for _ in range(int(passes)):
        y = one_pass(y, A, h)[0]
    return float(gain) * y


def apply_stream(x, A, h, passes=1, gain=1.0):
    """a whole stream: zeros for lead and tail"""
    halo = int(passes) * (len(h) - 1)
    return apply(np.concatenate([np.zeros(halo), np.asarray(x, np.complex128), np.zeros(halo)]), A, h, passes, gain)


def hard_clip(x, A):
    x = np.asarray(x, np.complex128)
    return x - excess(x, A)[0]


def rms(x):
    x = np.asarray(x, np.complex128)
    return float(np.sqrt(np.mean(x.real ** 2 + x.imag ** 2)))


def papr_db(x):
    """peak-to-average power ratio of the stream"""
    x = np.asarray(x, np.complex128)
    p = x.real ** 2 + x.imag ** 2
    return float(10.0 * np.log10(p.max() / p.mean()))


SPECTRUM_NFFT = 4096


def spectrum(x, nfft=SPECTRUM_NFFT):
    """(f, P): the power spectrum as the mean of |FFT|^2 over Hann-windowed segments of nfft samples that overlap by half"""
    x = np.asarray(x, np.complex128)
    nseg = (len(x) - nfft) // (nfft // 2) + 1
    w = np.hanning(nfft + 1)[:nfft]
    P = np.zeros(nfft)
    for i in range(nseg):
        P += np.abs(np.fft.fft(w * x[i * (nfft // 2):i * (nfft // 2) + nfft])) ** 2
    return np.fft.fftfreq(nfft), P / nseg


def oob_db(x, edge=0.32):
    """the share of the power that lies at |f| > edge cycles per sample, in dB"""
    f, P = spectrum(x)
    return float(10.0 * np.log10(P[np.abs(f) > edge].sum() / P.sum()))


# The end-to-end cases (tests/test_cfr.py finds these on the oracle alone; tests/test_gpu_cfr.py runs exactly these):
# N = 8, M = 64, three frames of 96 bytes per channel, QPSK / Hamming(12,8), the transmitter's gain 1 / N.  The stage at 7 dB over the
# rms, 63 taps with the edge at 0.28, two passes; before an amplifier (Rapp, p = 2, 6 dB input back-off) at 5 dB over the rms.
# `peak`: where the largest component of the sc16 output is put, as a share of full scale.
SEVERITY = dict(N=8, M=64, cp=8, taper=4, frames=3, payload_len=96,
                papr_db=7.0, half_len=31, cutoff=0.28, beta=5.65, passes=2, edge=0.32, peak=0.9,
                amp_papr_db=5.0, amp_ibo_db=6.0, amp_smooth=2,
                papr_gain_db=5.0, oob_margin_db=40.0, amp_oob_gain_db=4.0)
