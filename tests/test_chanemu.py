"""Channel emulator (mcrx_hip_chanemu_*), what needs no GPU: the random numbers' integers against published-style known answers and
against the library's own host build of the kernel's generator, the statistics of the noise construction, and the boundary -- symbols,
null handles, and every configuration error reported before a device is looked for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import chanemu_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mcrx_hip_chanemu_clipped", "mcrx_hip_chanemu_create", "mcrx_hip_chanemu_destroy", "mcrx_hip_chanemu_execute_device",
           "mcrx_hip_chanemu_last_error", "mcrx_hip_chanemu_output_format", "mcrx_hip_chanemu_position", "mcrx_hip_chanemu_reset",
           "mcrx_hip_chanemu_reset_at", "mcrx_hip_chanemu_selftest_words"]


# ---------------------------------------------------------------------------------------------- the integers
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = tuple(int(w[0]) for w in model.philox4x32_10(ctr, key))
    assert got == want, [hex(g) for g in got]


SEEDS = [0x1234567, 0xC0FFEE0123456789]                   # one above 2^32: the key's second word
POSITIONS = [0, 1, 2, 3, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 1]


@pytest.mark.parametrize("seed", SEEDS)
def test_selftest_words_equal_the_model(product, seed):
    L = product.lib()
    want = model.words(seed, np.array(POSITIONS, np.uint64))
    for p, w in zip(POSITIONS, want):
        out = (C.c_uint32 * 2)()
        assert L.mcrx_hip_chanemu_selftest_words(seed, p, out) == product.MCRX_OK
        assert (int(out[0]), int(out[1])) == (int(w[0]), int(w[1])), p
    # a pair shares one evaluation: the counter is n >> 1, the odd sample takes the upper two words
    full = model.philox4x32_10((1, 0, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    assert [int(v) for v in model.words(seed, [2, 3]).reshape(-1)] == [int(v[0]) for v in full]
    assert L.mcrx_hip_chanemu_selftest_words(seed, 0, None) == product.MCRX_EINVAL


def test_words_differ_between_seeds_and_positions():
    a, b = model.words(SEEDS[0], np.arange(64, dtype=np.uint64)), model.words(SEEDS[1], np.arange(64, dtype=np.uint64))
    assert len(set(map(tuple, a.tolist()))) == 64 and not np.array_equal(a, b)


def test_noise_model_statistics():
    n = 1 << 20
    w = model.noise(2024, 0, n)
    print("mean %.3e  var %.5f %.5f" % (abs(w.mean()), w.real.var(), w.imag.var()))
    assert abs(w.real.mean()) < 3e-3 and abs(w.imag.mean()) < 3e-3
    for c in (w.real, w.imag):
        var = float(np.mean(c * c))
        kurt = float(np.mean(c ** 4)) / var ** 2
        print("var %.5f kurtosis %.4f" % (var, kurt))
        assert abs(var - 1.0) < 0.01
        assert abs(kurt - 3.0) < 0.05
    assert np.all(np.isfinite(w.view(np.float64))) and float(np.abs(w).max()) <= 5.8      # u1 >= 2^-24


def test_cfo_step_helper(product):
    M, N = 64, 2
    assert product.chanemu_cfo_step(0, M, N) == 0
    assert product.chanemu_cfo_step(0.3, M, N) == int(round(0.3 / (M * 2 * N) * 2 ** 32))
    assert product.chanemu_cfo_step(-0.45, M, N) == (1 << 32) - int(round(0.45 / (M * 2 * N) * 2 ** 32))
    assert product.chanemu_cfo_step(M * 2 * N, M, N) == 0                                  # a whole cycle per sample


# ---------------------------------------------------------------------------------------------- the boundary
def test_symbols_are_declared_exported_and_bound(product):
    text = open(os.path.join(ROOT, "include", "mcrx_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mcrx_hip_chanemu_[a-z_0-9]+)\s*\(", text)))
    assert declared == SYMBOLS
    assert [s for s in product.exported_symbols() if s.startswith("mcrx_hip_chanemu_")] == SYMBOLS
    L = product.lib()
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None
    assert C.sizeof(product.ChanemuConfig) == 4 * (2 + 3 * 8 + 4) + 8 + 8                  # (seed is 8-byte aligned, the tail padded)
    assert "MCRX_CHANEMU_MAX_TAPS  8" in text and "MCRX_CHANEMU_MAX_DELAY 65535" in text
    assert (product.CHANEMU_MAX_TAPS, product.CHANEMU_MAX_DELAY) == (8, 65535)


def test_null_handles_are_answered(product):
    L = product.lib()
    assert L.mcrx_hip_chanemu_position(None) == 0
    assert L.mcrx_hip_chanemu_output_format(None) == 0
    assert L.mcrx_hip_chanemu_destroy(None) == product.MCRX_OK
    n = C.c_uint64(7)
    for rc in (L.mcrx_hip_chanemu_reset(None), L.mcrx_hip_chanemu_reset_at(None, 5), L.mcrx_hip_chanemu_clipped(None, C.byref(n), 0),
               L.mcrx_hip_chanemu_execute_device(None, None, 0, None, None), L.mcrx_hip_chanemu_create(None, None)):
        assert rc == product.MCRX_EINVAL
    assert L.mcrx_hip_chanemu_last_error()


def good_config(product):
    c = product.ChanemuConfig()
    c.struct_size, c.num_taps = C.sizeof(product.ChanemuConfig), 2
    c.delay[0], c.delay[1] = 0, 65535
    c.tap_re[0], c.tap_im[1] = 1.0, -0.5
    c.gain, c.noise_std, c.output_format = 1.0, 0.1, 1
    return c


BAD = [("struct_size", lambda c: setattr(c, "struct_size", c.struct_size - 4)),
       ("no taps", lambda c: setattr(c, "num_taps", 0)),
       ("nine taps", lambda c: setattr(c, "num_taps", 9)),
       ("delay", lambda c: c.delay.__setitem__(1, 65536)),
       ("tap nan", lambda c: c.tap_re.__setitem__(0, float("nan"))),
       ("tap inf", lambda c: c.tap_im.__setitem__(1, float("inf"))),
       ("gain", lambda c: setattr(c, "gain", float("inf"))),
       ("noise nan", lambda c: setattr(c, "noise_std", float("nan"))),
       ("noise negative", lambda c: setattr(c, "noise_std", -0.25)),
       ("format", lambda c: setattr(c, "output_format", 2))]


@pytest.mark.parametrize("what,spoil", BAD, ids=[b[0] for b in BAD])
def test_configuration_errors_come_before_the_device(product, what, spoil):
    L = product.lib()
    c = good_config(product)
    spoil(c)
    h = C.c_void_p(0x1234)
    assert L.mcrx_hip_chanemu_create(C.byref(h), C.addressof(c)) == product.MCRX_EINVAL, what
    assert not h.value                                                                     # *out is cleared
    assert L.mcrx_hip_chanemu_last_error()


def test_null_configuration(product):
    h = C.c_void_p()
    assert product.lib().mcrx_hip_chanemu_create(C.byref(h), None) == product.MCRX_EINVAL
    # a delay beyond the unused part of the table is not looked at
    c = good_config(product)
    c.delay[5] = 1 << 20
    rc = product.lib().mcrx_hip_chanemu_create(C.byref(h), C.addressof(c))
    assert rc in (product.MCRX_OK, product.MCRX_EHIP)                                      # (MCRX_EHIP: no device here)
    if rc == product.MCRX_OK:
        assert product.lib().mcrx_hip_chanemu_output_format(h) == 1
        product.lib().mcrx_hip_chanemu_destroy(h)


PY_BAD = [dict(taps=[]), dict(taps=[(0, 1.0)] * 9), dict(taps=[(65536, 1.0)]), dict(taps=[(-1, 1.0)]), dict(taps=[(1.5, 1.0)]),
          dict(taps=[(0, complex(float("nan"), 0))]), dict(taps=[(3, complex(0, float("inf")))]), dict(gain=float("inf")),
          dict(noise_std=-1.0), dict(noise_std=float("nan")), dict(output_format="sc8"), dict(output_format=2)]


@pytest.mark.parametrize("kw", PY_BAD, ids=[str(i) for i in range(len(PY_BAD))])
def test_python_class_raises_value_error_without_a_device(product, kw):
    with pytest.raises(ValueError):
        product.chanemu(**kw)
