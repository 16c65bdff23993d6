"""Float64 model of the channel monitor (include/mcrx_hip.h, "channel monitor"): what tests/test_monitor.py and
tests/test_gpu_monitor.py hold the GPU kernel to.  chan[n, c] = channel-rate samples of channel c, counted from the monitor's origin."""
import numpy as np

WINDOWS = {0: "rect", 1: "hann", 2: "hamming", "rect": 0, "rectangular": 0, "hann": 1, "hamming": 2}


def window(kind, nfft):
    kind = WINDOWS[kind] if isinstance(kind, str) else int(kind)
    n = np.arange(nfft, dtype=np.float64)
    if kind == 0:
        return np.ones(nfft)
    c = np.cos(2.0 * np.pi * n / nfft)
    return 0.5 - 0.5 * c if kind == 1 else 0.54 - 0.46 * c


def monitor(chan, nfft=64, win=0):
    """(level[nch], peak[nch], psd[nch, nfft], nseg, nsamp) of chan[nsamp, nch]: segments aligned to sample 0, a trailing partial
    segment is not counted in psd but is in level / peak."""
    x = np.asarray(chan, np.complex128)
    nsamp, nch = x.shape
    w = window(win, nfft)
    nseg = nsamp // nfft
    p = np.abs(x) ** 2
    level = p.mean(axis=0) if nsamp else np.zeros(nch)
    peak = p.max(axis=0) if nsamp else np.zeros(nch)
    if nseg:
        seg = x[:nseg * nfft].reshape(nseg, nfft, nch) * w[None, :, None]
        psd = (np.abs(np.fft.fft(seg, axis=1)) ** 2).mean(axis=0).T / np.sum(w * w)
    else:
        psd = np.zeros((nch, nfft))
    return level, peak, np.ascontiguousarray(psd), nseg, nsamp


def omega(N, nfft, c, kp):
    """wideband frequency [radians per wideband sample] of signed bin kp in (-nfft/2, nfft/2] of channel c (front_end 0 and 1)"""
    return np.pi * (c - (N - 1) / 2.0) / N + 2.0 * np.pi * kp / (nfft * 2.0 * N)


def signed_bin(k, nfft):
    return k if k <= nfft // 2 else k - nfft
