"""Channel monitor, the parts that need no GPU: the C-ABI's boundary (symbols, argument checks on a null handle), the float64 model
(tests/monitor_model.py) on the oracle's channelizer output -- Parseval, and where a wideband tone lands: that pins the (channel, bin)
-> frequency formula of DESIGN.md --, the pure-numpy helpers of a reading, and the scan tool's build."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import monitor_model as mm                      # noqa: E402
from test_boundary import declared_symbols      # noqa: E402

NAMES = ["mcrx_hip_monitor_enable", "mcrx_hip_monitor_disable", "mcrx_hip_monitor_read", "mcrx_hip_monitor_nfft"]


def test_monitor_symbols_declared_bound_and_exported(product):
    path = product.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    exported = set(re.findall(r" T ((?:mcrx|msresamp|mctx)_hip_[a-z_0-9]+)", out))
    for n in NAMES:
        assert n in declared_symbols(), n
        assert n in product.exported_symbols(), n
        assert n in exported, n
    for m in ("monitor_enable", "monitor_disable", "monitor_read"):
        assert callable(getattr(product.multichannelrx, m)) and callable(getattr(product.ofdmflexframesync, m))


def test_monitor_argument_checks_without_a_gpu(product):
    product.build()
    L = product.lib()
    EINVAL = -1

    def enable(h, nfft, window):
        c = product.MonitorConfig()
        c.struct_size, c.nfft, c.window = ctypes.sizeof(c), nfft, window
        return L.mcrx_hip_monitor_enable(h, ctypes.addressof(c)), L.mcrx_hip_last_error().decode()

    # a bad configuration is named before the handle is looked at
    rc, msg = enable(None, 48, 0)
    assert rc == EINVAL and "nfft" in msg
    rc, msg = enable(None, 64, 3)
    assert rc == EINVAL and "window" in msg
    for nfft in (16, 32, 64, 128, 256, 0):
        for w in (0, 1, 2):
            rc, msg = enable(None, nfft, w)
            assert rc == EINVAL and "null handle" in msg
    assert L.mcrx_hip_monitor_enable(None, None) == EINVAL
    assert L.mcrx_hip_monitor_disable(None) == EINVAL
    lv, n = (ctypes.c_double * 4)(), ctypes.c_uint64(7)
    assert L.mcrx_hip_monitor_read(None, lv, None, None, ctypes.byref(n), None, 1) == EINVAL and n.value == 7
    assert L.mcrx_hip_monitor_nfft(None) == 0


def _tone(N, nfft, c, kp, nblocks):
    n = np.arange(nblocks * 2 * N, dtype=np.float64)
    return np.exp(1j * mm.omega(N, nfft, c, kp) * n).astype(np.complex64)


def test_model_parseval_on_the_oracles_channelizer(oracle):
    N, M, cp, tp = 8, 64, 16, 4
    iq, _ = oracle.synth_traffic(N, M, cp, tp, 2, payload_len=200)
    chan = oracle.MultiChannelRx(N, M, cp, tp).channelize(iq[:len(iq) // (2 * N) * (2 * N)])
    for nfft in (16, 64, 256):
        n = chan.shape[0] // nfft * nfft
        level, peak, psd, nseg, nsamp = mm.monitor(chan[:n], nfft, 0)
        assert nseg == n // nfft and nsamp == n
        assert np.max(np.abs(psd.mean(axis=1) - level) / level) < 1e-12
        assert np.all(peak >= level)
    # a trailing partial segment counts for level and peak only
    l2, p2, psd2, nseg2, nsamp2 = mm.monitor(chan[:64 * 5 + 16], 64, 1)
    assert nseg2 == 5 and nsamp2 == 64 * 5 + 16
    assert np.array_equal(psd2, mm.monitor(chan[:64 * 5], 64, 1)[2])


@pytest.mark.parametrize("front_end", [0, 1])
def test_tones_land_in_the_predicted_channel_and_bin(oracle, front_end):
    N, M, cp, tp, nfft = 8, 64, 16, 4, 64
    skip = 64                                    # blocks of filter transient
    cases = [(3, 5), (7, 0), (0, -7), (5, 32), (1, -4)]
    for c, kp in cases:
        rx = oracle.MultiChannelRx(N, M, cp, tp, front_end=front_end)
        x = _tone(N, nfft, c, kp, skip + 8 * nfft)
        chan = (rx.channelize_oversampled if front_end else rx.channelize)(x)
        level, peak, psd, nseg, _ = mm.monitor(chan[skip:], nfft, 1)
        got = np.unravel_index(np.argmax(psd), psd.shape)
        assert (int(got[0]), mm.signed_bin(int(got[1]), nfft)) == (c, kp), (front_end, c, kp, got)
    if front_end == 0:
        # 60 bins above channel 0's centre = 4 bins below channel 1's: the fft-shifted rows tile the band
        rx = oracle.MultiChannelRx(N, M, cp, tp)
        n = np.arange((skip + 8 * nfft) * 2 * N, dtype=np.float64)
        x = np.exp(1j * (mm.omega(N, nfft, 0, 0) + 2 * np.pi * 60 / (nfft * 2.0 * N)) * n).astype(np.complex64)
        psd = mm.monitor(rx.channelize(x)[skip:], nfft, 1)[2]
        assert np.unravel_index(np.argmax(psd), psd.shape) == (1, 60)


def test_reading_helpers_order_and_axis(product):
    N, nfft = 4, 16
    psd = np.arange(N * nfft, dtype=np.float64).reshape(N, nfft) + 1.0
    level = np.array([1.0, 1e-4, 10.0, 1e-3])
    r = product.MonitorReading(level, level * 2, psd, 3, 48, N)
    assert np.allclose(r.level_db(), [0.0, -40.0, 10.0, -30.0])
    assert r.occupied(-20.0).tolist() == [True, False, True, False]
    row, om = r.wideband()
    assert row.shape == om.shape == (N * nfft,)
    assert np.all(np.diff(om) > 0) and np.allclose(np.diff(om), 2 * np.pi / (nfft * 2 * N))       # no gap, no overlap
    for c in range(N):
        for k in range(nfft):
            i = np.argmin(np.abs(om - mm.omega(N, nfft, c, mm.signed_bin(k, nfft))))
            assert row[i] == psd[c, k], (c, k)
    assert np.allclose(product.monitor_omega(N, nfft, 2, -3), mm.omega(N, nfft, 2, -3))
    # a shard's reading carries its first channel
    r2 = product.MonitorReading(level[:2], level[:2], psd[:2], 3, 48, N, channel_first=2)
    assert np.allclose(r2.wideband()[1], om[2 * nfft:])


def test_scan_tool_builds_beside_the_host_programs():
    host = os.path.join(ROOT, "liquid-usrp_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s"])
    subprocess.check_call(["make", "-C", host, "-s", "mcrx_scan"])
    assert os.access(os.path.join(host, "mcrx_scan"), os.X_OK)
