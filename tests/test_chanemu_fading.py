"""Fading rays of the channel emulator (mcrx_hip_chanfade_*), what needs no GPU: the integer tables the library
makes on the host against the model's own, every configuration error, the statistics of the model's gains against Jakes' spectrum, and
the end-to-end scenario of tests/test_gpu_chanemu_fading.py through the float64 model and the oracle's receiver."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import chanemu_fading_model as fmodel
import chanemu_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mcrx_hip_chanfade_gains", "mcrx_hip_chanfade_on", "mcrx_hip_chanfade_selftest", "mcrx_hip_chanfade_set"]


def selftest(product, f, ray):
    S = int(f.num_sinusoids)
    steps, phases, coef = (C.c_int64 * 17)(), (C.c_uint32 * 17)(), (C.c_float * 2)()
    rc = product.lib().mcrx_hip_chanfade_selftest(C.addressof(f), ray, steps, phases, coef)
    assert rc == product.MCRX_OK, product.lib().mcrx_hip_chanemu_last_error()
    return [int(v) for v in steps[:S + 1]], [int(v) for v in phases[:S + 1]], (float(coef[0]), float(coef[1]))


# ---------------------------------------------------------------------------------------------- the boundary
def test_symbols_are_declared_exported_and_bound(product):
    text = open(os.path.join(ROOT, "include", "mcrx_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(mcrx_hip_chanfade_[a-z_0-9]+)\s*\(", text))) == NEW
    assert [s for s in product.exported_symbols() if s.startswith("mcrx_hip_chanfade_")] == NEW
    for s in NEW:
        assert getattr(product.lib(), s).argtypes is not None
    assert "MCRX_CHANEMU_MAX_SINUSOIDS 16" in text and product.CHANEMU_MAX_SINUSOIDS == 16
    assert C.sizeof(product.ChanemuFading) == 16 + 8 * (8 + 8 + 4 + 4) + 8
    for m in ("set_fading", "fading_on"):
        assert callable(getattr(product.chanemu, m))


def test_null_handles_are_answered(product):
    L = product.lib()
    f = product.chanemu_fading(1, doppler=1e-5)
    assert L.mcrx_hip_chanfade_on(None) == 0
    assert L.mcrx_hip_chanfade_set(None, C.addressof(f)) == product.MCRX_EINVAL
    assert L.mcrx_hip_chanfade_set(None, None) == product.MCRX_EINVAL
    assert L.mcrx_hip_chanfade_gains(None, 0, 1, None, None) == product.MCRX_EINVAL
    assert L.mcrx_hip_chanemu_last_error()
    steps, phases, coef = (C.c_int64 * 17)(), (C.c_uint32 * 17)(), (C.c_float * 2)()
    assert L.mcrx_hip_chanfade_selftest(None, 0, steps, phases, coef) == product.MCRX_EINVAL
    assert L.mcrx_hip_chanfade_selftest(C.addressof(f), 0, None, phases, coef) == product.MCRX_EINVAL
    assert L.mcrx_hip_chanfade_selftest(C.addressof(f), 8, steps, phases, coef) == product.MCRX_EINVAL


# ---------------------------------------------------------------------------------------------- the integers
CASES = [dict(doppler=3e-6, rice_k=[8.0, 0.0, 0.5], los_doppler=[0.9e-6, 0.0, -2e-6], los_phase=[0x12345678, 0, 0xFFFFFFFF], sinusoids=8,
              log2_block=10, seed=4),
         dict(doppler=[2.0 ** -12, 0.0, 1e-3], rice_k=0.0, sinusoids=16, log2_block=6, seed=0xC0FFEE0123456789),
         dict(doppler=[0.0625, 0.01, 0.0], rice_k=[1e6, 3.0, 0.0], los_doppler=[-0.0625, 0.0625, 0.0], sinusoids=1, log2_block=1, seed=1)]


@pytest.mark.parametrize("kw", CASES, ids=["rician", "rayleigh", "edges"])
def test_selftest_tables_equal_the_model(product, kw):
    """phases (Philox words) exact; steps within 2^-50 |step| + 1 (libm and numpy may differ in cos by an ulp); coefficients exact as fp32"""
    f = product.chanemu_fading(3, **kw)
    assert (f.log2_block, f.num_sinusoids, f.seed) == (kw["log2_block"], kw["sinusoids"], kw["seed"])
    want = fmodel.tables(f.seed, list(f.doppler)[:3], list(f.los_doppler)[:3], list(f.rice_k)[:3], list(f.los_phase)[:3], f.num_sinusoids)
    for i in range(3):
        steps, phases, coef = selftest(product, f, i)
        assert phases == want[i][1], i
        assert len(steps) == f.num_sinusoids + 1
        for a, b in zip(steps, want[i][0]):
            assert abs(a - b) <= 2.0 ** -50 * abs(b) + 1, (i, a, b)
        assert coef == want[i][2], (i, coef, want[i][2])
        assert abs(coef[0] ** 2 + f.num_sinusoids * coef[1] ** 2 - 1.0) < 1e-6               # E |g|^2 = 1
        # the scattered steps lie inside the Doppler spread, one per stratum of the arrival angle
        fd = f.doppler[i] * 2.0 ** 64
        for k, (st, w0) in enumerate(zip(steps[1:], want[i][3])):
            assert abs(st) <= fd + 1
            alpha = 2.0 * np.pi * (k + w0 * 2.0 ** -32) / f.num_sinusoids
            assert 2.0 * np.pi * k / f.num_sinusoids <= alpha < 2.0 * np.pi * (k + 1) / f.num_sinusoids
    # the words are those of counter (k, ray, 1, 0): apart from the noise words (c2 = 0), and another seed gives other tables
    w = model.philox4x32_10((0, 1, 1, 0), (f.seed & 0xFFFFFFFF, f.seed >> 32))
    assert selftest(product, f, 1)[1][1] == int(w[1][0])
    g = product.chanemu_fading(3, **dict(kw, seed=kw["seed"] + 1))
    assert selftest(product, g, 0)[1][1:] != selftest(product, f, 0)[1][1:]


def test_doppler_helper(product):
    assert product.chanemu_doppler(0, 64, 8, 2) == 0.0
    assert product.chanemu_doppler(0.25, 64, 8, 2) == 0.25 / (72 * 4)
    assert product.chanemu_doppler(1.0, 1024, 16, 512) == 1.0 / (1040 * 1024)


# ---------------------------------------------------------------------------------------------- configuration errors
def good_fading(product):
    return product.chanemu_fading(8, doppler=1e-5, rice_k=1.0, los_doppler=-1e-5, sinusoids=8, log2_block=10)


BAD = [("struct_size", lambda f: setattr(f, "struct_size", f.struct_size - 4)),
       ("L zero", lambda f: setattr(f, "log2_block", 0)),
       ("L 25", lambda f: setattr(f, "log2_block", 25)),
       ("S zero", lambda f: setattr(f, "num_sinusoids", 0)),
       ("S 17", lambda f: setattr(f, "num_sinusoids", 17)),
       ("one row", lambda f: setattr(f, "table_rows", 1)),
       ("doppler nan", lambda f: f.doppler.__setitem__(2, float("nan"))),
       ("doppler inf", lambda f: f.doppler.__setitem__(2, float("inf"))),
       ("los doppler nan", lambda f: f.los_doppler.__setitem__(2, float("nan"))),
       ("doppler negative", lambda f: f.doppler.__setitem__(2, -1e-6)),
       ("doppler too fast", lambda f: f.doppler.__setitem__(2, 0.126 / 1024)),
       ("los doppler too fast", lambda f: f.los_doppler.__setitem__(2, -0.126 / 1024)),
       ("rice negative", lambda f: f.rice_k.__setitem__(2, -0.5)),
       ("rice nan", lambda f: f.rice_k.__setitem__(2, float("nan"))),
       ("rice inf", lambda f: f.rice_k.__setitem__(2, float("inf")))]


@pytest.mark.parametrize("what,spoil", BAD, ids=[b[0] for b in BAD])
def test_configuration_errors_need_no_device(product, what, spoil):
    """the check mcrx_hip_chanfade_set makes, reached here through the host self-test (a handle needs a device: the same cases on a
    handle are in tests/test_gpu_chanemu_fading.py)"""
    L = product.lib()
    f = good_fading(product)
    steps, phases, coef = (C.c_int64 * 17)(), (C.c_uint32 * 17)(), (C.c_float * 2)()
    assert L.mcrx_hip_chanfade_selftest(C.addressof(f), 2, steps, phases, coef) == product.MCRX_OK
    spoil(f)
    coef[0] = -7.0
    assert L.mcrx_hip_chanfade_selftest(C.addressof(f), 2, steps, phases, coef) == product.MCRX_EINVAL, what
    assert L.mcrx_hip_chanemu_last_error() and coef[0] == -7.0                              # nothing written
    if "doppler" in what or "rice" in what:                                                 # another ray's entry is not looked at
        assert L.mcrx_hip_chanfade_selftest(C.addressof(f), 1, steps, phases, coef) == product.MCRX_OK


def test_the_limit_itself_is_accepted(product):
    f = product.chanemu_fading(1, doppler=0.125 / 1024, los_doppler=-0.125 / 1024, log2_block=10, table_rows=2)
    selftest(product, f, 0)


PY_BAD = [dict(log2_block=0), dict(log2_block=25), dict(log2_block=1.5), dict(sinusoids=0), dict(sinusoids=17), dict(table_rows=1),
          dict(table_rows=-1), dict(doppler=float("nan")), dict(doppler=-1e-6), dict(doppler=0.126 / 1024), dict(los_doppler=float("inf")),
          dict(los_doppler=0.126 / 1024), dict(rice_k=-1.0), dict(rice_k=float("nan")), dict(rice_k=1e39), dict(doppler=[1e-6, 1e-6]),
          dict(los_phase=[0, 0, 0]), dict(dopler=1e-6), "rayleigh"]


@pytest.mark.parametrize("kw", PY_BAD, ids=[str(i) for i in range(len(PY_BAD))])
def test_python_class_raises_value_error_without_a_device(product, kw):
    with pytest.raises(ValueError):
        product.chanemu(taps=[(0, 1.0)], fading=kw)


# ---------------------------------------------------------------------------------------------- statistics
def bessel_j0(x):
    th = (np.arange(4096) + 0.5) * (2.0 * np.pi / 4096)                                    # (a periodic integrand: exact to rounding)
    return float(np.mean(np.cos(x * np.sin(th))))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_statistics(seed):
    """K = 0, S = 16, f_d = 2^-12, L = 6 over 40 000 grid rows: mean |G|^2 within 2 % of 1, and the real part of the normalised
    autocorrelation at lags 4, 8, 16 rows within 0.05 of Jakes' J0(2 pi f_d lag B)"""
    fd, L, rows = 2.0 ** -12, 6, 40000
    t = fmodel.tables(seed, [fd], [0.0], [0.0], [0], 16)[0]
    G = fmodel.grid(t, np.arange(rows, dtype=np.uint64), L)
    p = float(np.mean(np.abs(G) ** 2))
    print("fading seed %d: mean |G|^2 %.4f" % (seed, p))
    assert abs(p - 1.0) < 0.02
    for lag in (4, 8, 16):
        r = complex(np.mean(G[lag:] * np.conj(G[:-lag]))) / p
        want = bessel_j0(2.0 * np.pi * fd * lag * (1 << L))
        print("  lag %2d rows: R = %.4f %+.4fj, J0 = %.4f" % (lag, r.real, r.imag, want))
        assert abs(r.real - want) < 0.05, (lag, r, want)
    # the interpolated gain passes through the grid and is linear between its rows
    g = fmodel.gain(t, 5 << L, (2 << L) + 1, L)
    assert np.array_equal(g[::1 << L], G[5:8])
    assert abs(g[(1 << L) // 2] - 0.5 * (G[5] + G[6])) < 1e-15


# ---------------------------------------------------------------------------------------------- end to end on the CPU
def scenario(oracle, fading_seed, snr_db=25.0, doppler=3e-6):
    """oracle.synth_traffic(2, 64, 8, 4, 12, 96, seed=79) plus 64 K zeros through the float64 model (three fading rays inside every
    channel, noise at snr_db) and the oracle's receiver: (frames, sent)"""
    N, M, cp, taper, nf, plen = 2, 64, 8, 4, 12, 96
    K = 2 * N
    iq, sent = oracle.synth_traffic(N, M, cp, taper, nf, plen, seed=79)
    iq = np.concatenate([iq, np.zeros(64 * K, np.complex64)])
    taps = [(0, 1.0), (K + 3, 0.35 - 0.2j), (3 * K, -0.15 + 0.2j)]
    tabs = fmodel.tables(fading_seed, [doppler] * 3, [0.9e-6, 0.0, 0.0], [8.0, 0.0, 0.0], [0x12345678, 0, 0], 8)
    s = fmodel.faded(iq, taps, tabs, 10)
    nstd = float(np.sqrt(np.mean(np.abs(s) ** 2) / 10.0 ** (snr_db / 10.0) / 2.0))
    v = (s + nstd * model.noise(2024, 0, len(s))).astype(np.complex64)
    rx = oracle.MultiChannelRx(N, M, cp, taper)
    rx.execute(np.ascontiguousarray(v))
    return rx.frames, sent


def valid_frames(frames, sent):
    seen = set()
    for f in frames:
        if f.header_valid and f.payload_valid:
            pid = (f.header[0] << 8) | f.header[1]
            assert sent[f.channel][pid] == (bytes(f.header), bytes(f.payload)), (f.channel, pid)      # valid means the sent bytes
            seen.add((f.channel, pid))
    return len(seen)


@pytest.mark.parametrize("seed", [4, 5])
def test_end_to_end_on_the_cpu(oracle, seed):
    frames, sent = scenario(oracle, seed)
    assert len(frames) == 24 and all(f.header_valid and f.payload_valid for f in frames)
    assert valid_frames(frames, sent) == 24


def test_deep_fade_scenario_is_a_mixed_one(oracle):
    """fading seed 3: the input of the contract case of tests/test_gpu_chanemu_fading.py.  Some frames fade out, most do not."""
    frames, sent = scenario(oracle, 3)
    n = valid_frames(frames, sent)
    print("fading seed 3: %d of 24 valid" % n)
    assert 8 <= n <= 23
