"""Per-user channel emulator (mcrx_hip_userchan_*), what needs no GPU: the boundary -- symbols, null handles, every configuration error
reported before a device is looked for -- the oscillator helper, and the float64 model against a direct shift-and-add."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import userchan_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mcrx_hip_userchan_apply_tiles", "mcrx_hip_userchan_create", "mcrx_hip_userchan_destroy", "mcrx_hip_userchan_last_error",
           "mcrx_hip_userchan_lead_blocks", "mcrx_hip_userchan_num_channels"]


def test_symbols_are_declared_exported_and_bound(product):
    import subprocess
    text = open(os.path.join(ROOT, "include", "mcrx_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mcrx_hip_userchan_[a-z_0-9]+)\s*\(", text)))
    assert declared == SYMBOLS
    assert [s for s in product.exported_symbols() if s.startswith("mcrx_hip_userchan_")] == SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only", product.build()]).decode()
    assert sorted(set(re.findall(r" T (mcrx_hip_userchan_[a-z_0-9]+)", out))) == SYMBOLS
    L = product.lib()
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None
    assert C.sizeof(product.UserchanChannel) == 4 * (1 + 3 * 4 + 3)
    assert "MCRX_USERCHAN_MAX_RAYS     4" in text and "MCRX_USERCHAN_MAX_DELAY    255" in text
    assert (product.USERCHAN_MAX_RAYS, product.USERCHAN_MAX_DELAY, product.USERCHAN_MAX_CHANNELS) == (4, 255, 1024)
    assert product.USERCHAN_SYNTH_LEAD >= 25 and product.USERCHAN_SYNTH_LEAD % 8 == 0


def test_null_handles_are_answered(product):
    L = product.lib()
    assert L.mcrx_hip_userchan_num_channels(None) == 0
    assert L.mcrx_hip_userchan_lead_blocks(None) == 0
    assert L.mcrx_hip_userchan_destroy(None) == product.MCRX_OK
    assert L.mcrx_hip_userchan_apply_tiles(None, None, 0, 0, 0, None, None) == product.MCRX_EINVAL
    assert L.mcrx_hip_userchan_last_error()


def good_table(product, n=3):
    t = (product.UserchanChannel * n)()
    for c in range(n):
        t[c].num_rays = 2
        t[c].delay[0], t[c].delay[1] = 0, 255
        t[c].tap_re[0], t[c].tap_im[1] = 1.0, -0.5
        t[c].gain, t[c].cfo_step = 0.5, 12345 * c
    return t


def create(product, table, n=None, size=None, out=True):
    h = C.c_void_p(0x1234)
    rc = product.lib().mcrx_hip_userchan_create(C.byref(h) if out else None, len(table) if n is None else n,
                                                C.addressof(table) if table is not None else None,
                                                C.sizeof(product.UserchanChannel) if size is None else size)
    return rc, h


BAD = [("no rays", lambda t: setattr(t[1], "num_rays", 0)),
       ("five rays", lambda t: setattr(t[2], "num_rays", 5)),
       ("delay", lambda t: t[1].delay.__setitem__(1, 256)),
       ("tap nan", lambda t: t[0].tap_re.__setitem__(0, float("nan"))),
       ("tap inf", lambda t: t[2].tap_im.__setitem__(1, float("inf"))),
       ("gain inf", lambda t: setattr(t[1], "gain", float("inf"))),
       ("gain nan", lambda t: setattr(t[2], "gain", float("nan")))]


@pytest.mark.parametrize("what,spoil", BAD, ids=[b[0] for b in BAD])
def test_channel_errors_come_before_the_device(product, what, spoil):
    t = good_table(product)
    spoil(t)
    rc, h = create(product, t)
    assert rc == product.MCRX_EINVAL, what
    assert not h.value                                                                     # *out is cleared
    assert product.lib().mcrx_hip_userchan_last_error()


def test_argument_errors_come_before_the_device(product):
    t = good_table(product)
    EINVAL = product.MCRX_EINVAL
    assert create(product, t, out=False)[0] == EINVAL                                      # null out
    rc, h = create(product, t, n=0)
    assert rc == EINVAL and not h.value
    big = good_table(product, 1025)
    assert create(product, big)[0] == EINVAL
    assert create(product, t, size=C.sizeof(product.UserchanChannel) - 4)[0] == EINVAL
    h = C.c_void_p(0x1234)
    assert product.lib().mcrx_hip_userchan_create(C.byref(h), 3, None, C.sizeof(product.UserchanChannel)) == EINVAL and not h.value
    # what lies beyond a channel's num_rays is not looked at; 1024 channels are allowed
    t[0].delay[3], t[0].tap_re[2] = 1 << 20, float("nan")
    rc, h = create(product, t)
    assert rc in (product.MCRX_OK, product.MCRX_EHIP)                                      # (MCRX_EHIP: no device here)
    if rc == product.MCRX_OK:
        assert product.lib().mcrx_hip_userchan_num_channels(h) == 3 and product.lib().mcrx_hip_userchan_lead_blocks(h) == 256
        product.lib().mcrx_hip_userchan_destroy(h)
    rc, h = create(product, good_table(product, 1024))
    assert rc in (product.MCRX_OK, product.MCRX_EHIP)
    if rc == product.MCRX_OK:
        product.lib().mcrx_hip_userchan_destroy(h)


PY_BAD = [[], [dict(taps=[])], [dict(taps=[(0, 1.0)] * 5)], [dict(taps=[(256, 1.0)])], [dict(taps=[(250, 1.0)], delay=6)],
          [dict(taps=[(-1, 1.0)])], [dict(taps=[(1.5, 1.0)])], [dict(taps=[(0, 1.0)], delay=-1)],
          [dict(taps=[(0, complex(float("nan"), 0))])], [dict(taps=[(3, complex(0, float("inf")))])],
          [dict(taps=[(0, 1.0)], gain_db=float("inf"))], [dict(taps=[(0, 1.0)], gain_db=float("nan"))], [dict(taps=[(0, 1.0)], gain_db=1e4)],
          [dict(taps=[(0, 1.0)], level=3.0)], [dict(taps=[(0, 1.0)])] * 1025]


@pytest.mark.parametrize("channels", PY_BAD, ids=[str(i) for i in range(len(PY_BAD))])
def test_python_class_raises_value_error_without_a_device(product, channels):
    with pytest.raises(ValueError):
        product.userchan(channels=channels)


def test_channel_structure_of_a_description(product):
    u = product.userchan_channel(taps=[(0, 1.0), (3, 0.25 - 0.15j)], gain_db=-30.0, cfo_step=-5, phase0=1 << 32, delay=7)
    assert u.num_rays == 2 and list(u.delay)[:2] == [7, 10]
    assert u.gain == float(np.float32(10.0 ** -1.5)) and u.cfo_step == (1 << 32) - 5 and u.phase0 == 0
    assert (u.tap_re[1], u.tap_im[1]) == (0.25, float(np.float32(-0.15)))


def test_cfo_step_helper(product):
    for M in (64, 48):
        assert product.userchan_cfo_step(0, M) == 0
        assert product.userchan_cfo_step(0.45, M) == int(round(0.45 / M * 2 ** 32))
        assert product.userchan_cfo_step(-0.45, M) == (1 << 32) - int(round(0.45 / M * 2 ** 32))
        assert product.userchan_cfo_step(1.0, M) == int(round(2 ** 32 / M))
    assert product.userchan_cfo_step(1.0, 64) == 1 << 26 and product.userchan_cfo_step(1.0, 48) == 89478485
    assert product.userchan_cfo_step(64.0, 64) == 0                                        # a whole cycle per sample


def test_model_is_a_shift_and_add():
    rng = np.random.RandomState(3)
    lead, n, first = 16, 64, 40
    x = rng.randn(lead + n) + 1j * rng.randn(lead + n)
    ch = dict(taps=[(0, 1.0), (2, 0.5 - 0.25j), (9, -0.125j)], gain_db=-6.0, cfo_step=1 << 29, phase0=1 << 30, delay=3)
    want = np.zeros(n, np.complex128)
    for b in range(n):
        s = x[lead + b - 3] + (0.5 - 0.25j) * x[lead + b - 5] - 0.125j * x[lead + b - 12]
        want[b] = float(np.float32(10.0 ** -0.3)) * s * np.exp(2j * np.pi * (0.25 + (first + b) / 8.0))
    got = model.apply_channel(x, ch, first, lead)
    assert np.abs(got - want).max() < 1e-12
    assert model.lead_of([ch]) == 16 and model.bound(ch, x) > 0
    # the phase depends on b mod 2^32 only, negative block indices included
    assert np.abs(model.apply_channel(x, ch, first - (1 << 32), lead) - want).max() < 1e-12
    assert np.abs(model.apply_channel(x, ch, first + (1 << 40), lead) - want).max() < 1e-12
    # granules: [tile][channel][8]
    X = np.arange(3 * 16).reshape(3, 16)
    t = model.to_tiles(X)
    assert list(t[:8]) == list(range(8)) and list(t[8:16]) == list(range(16, 24)) and list(t[24:32]) == list(range(8, 16))
    assert np.array_equal(model.from_tiles(t, 3), X)
