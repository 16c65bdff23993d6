"""Each user's own sample clock and fractional timing in the per-user channel emulator (mcrx_hip_userclock_*),
what needs no GPU: the boundary, every configuration error through the host self-test, the integers and coefficients the library makes
against the model's Python integers and exact fp32 restatement, the table against the formula in double, the interpolator's quality
computed from the library's own table, and the Python argument handling."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import userclock_model as kmodel
from test_chanemu_fading import NEW as CHANFADE_SYMBOLS
from test_userchan import SYMBOLS as USERCHAN_SYMBOLS
from test_userchan_fading import NEW as USERFADE_SYMBOLS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mcrx_hip_userclock_apply_tiles", "mcrx_hip_userclock_lead_blocks", "mcrx_hip_userclock_on", "mcrx_hip_userclock_selftest",
       "mcrx_hip_userclock_set", "mcrx_hip_userclock_table"]
PPM = 281474977                                   # 1 ppm in units of 2^-48 samples per sample


def library_table(product):
    """W[65][32] as the library reports it (fp32)"""
    W = (C.c_float * (65 * 32))()
    assert product.lib().mcrx_hip_userclock_table(W) == product.MCRX_OK
    return np.array(W, dtype=np.float32).reshape(65, 32)


def selftest(product, f, u, block):
    """(rc, tau_fp, h[32] as fp32) of one user at one block; tau_fp and h are None when the library refuses"""
    tau, h = C.c_int64(-7), (C.c_float * 32)(*([-7.0] * 32))
    rc = product.lib().mcrx_hip_userclock_selftest(C.addressof(f), C.addressof(u), int(block), C.byref(tau), h)
    if rc != product.MCRX_OK:
        assert tau.value == -7 and all(v == -7.0 for v in h), "nothing is written on an error"
        return rc, None, None
    return rc, int(tau.value), np.array(h, dtype=np.float32)


def structs(product, max_delay=64, **user):
    f, users = product.userchan_clock(1, max_delay=max_delay, users=[user])
    return f, users[0]


def integers(u):
    return dict(delay_fp=int(u.delay_fp), sco=int(u.sco), origin=int(u.origin))


# ---------------------------------------------------------------------------------------------- the boundary
def test_symbols_are_declared_exported_and_bound(product):
    text = open(os.path.join(ROOT, "include", "mcrx_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", product.build()]).decode()
    for prefix, want in (("mcrx_hip_userclock_", NEW), ("mcrx_hip_userchan_", USERCHAN_SYMBOLS), ("mcrx_hip_userfade_", USERFADE_SYMBOLS),
                         ("mcrx_hip_chanfade_", CHANFADE_SYMBOLS)):
        assert sorted(set(re.findall(r"\b(%s[a-z_0-9]+)\s*\(" % prefix, text))) == want
        assert [s for s in product.exported_symbols() if s.startswith(prefix)] == want
        assert sorted(set(re.findall(r" T (%s[a-z_0-9]+)" % prefix, out))) == want
    for s in NEW:
        assert getattr(product.lib(), s).argtypes is not None
    assert C.sizeof(product.UserclockUser) == 32 and C.sizeof(product.UserclockConfig) == 16
    assert C.sizeof(product.UserchanChannel) == 64                                         # the channel structure is the parent's
    for name, val in (("TAPS", 32), ("PHASES", 64), ("MIN_DELAY", 15), ("MAX_DELAY", 255)):
        assert re.search(r"#define MCRX_USERCLOCK_%s\s+%d\b" % (name, val), text), name
        assert getattr(product, "USERCLOCK_" + name) == val
    for m in ("set_clock", "clock_on", "resample"):
        assert callable(getattr(product.userchan, m))


def test_null_handles_are_answered(product):
    L, EINVAL = product.lib(), product.MCRX_EINVAL
    f, u = structs(product, delay=16.25, ppm=20.0)
    assert L.mcrx_hip_userclock_on(None) == 0 and L.mcrx_hip_userclock_lead_blocks(None) == 0
    assert L.mcrx_hip_userclock_set(None, C.addressof(f), C.addressof(u)) == EINVAL
    assert L.mcrx_hip_userclock_set(None, None, None) == EINVAL
    assert L.mcrx_hip_userclock_apply_tiles(None, None, 0, 0, 0, None, None) == EINVAL
    assert L.mcrx_hip_userchan_last_error()
    tau, h = C.c_int64(0), (C.c_float * 32)()
    assert L.mcrx_hip_userclock_selftest(None, C.addressof(u), 0, C.byref(tau), h) == EINVAL
    assert L.mcrx_hip_userclock_selftest(C.addressof(f), None, 0, C.byref(tau), h) == EINVAL
    assert L.mcrx_hip_userclock_selftest(C.addressof(f), C.addressof(u), 0, None, h) == EINVAL
    assert L.mcrx_hip_userclock_selftest(C.addressof(f), C.addressof(u), 0, C.byref(tau), None) == EINVAL
    assert L.mcrx_hip_userclock_table(None) == EINVAL


# ---------------------------------------------------------------------------------------------- configuration errors
# (what, spoil(f, u), the block asked for)
BAD = [("struct_size", lambda f, u: setattr(f, "struct_size", f.struct_size - 4), 0),
       ("user_struct_size", lambda f, u: setattr(f, "user_struct_size", f.user_struct_size + 8), 0),
       ("max_delay 14", lambda f, u: setattr(f, "max_delay", 14), 0),
       ("max_delay 256", lambda f, u: setattr(f, "max_delay", 256), 0),
       ("span not in granules", lambda f, u: setattr(f, "span_blocks", 12), 0),
       ("sco above", lambda f, u: setattr(u, "sco", (1 << 38) + 1), 0),
       ("sco below", lambda f, u: setattr(u, "sco", -(1 << 38) - 1), 0),
       ("delay_fp n 14", lambda f, u: setattr(u, "delay_fp", (15 << 32) - 1), 0),
       ("delay_fp n above max_delay", lambda f, u: setattr(u, "delay_fp", 65 << 32), 0),
       ("delay_fp huge", lambda f, u: setattr(u, "delay_fp", 1 << 63), 0),
       ("a block whose n falls below 15", lambda f, u: (setattr(u, "delay_fp", 15 << 32), setattr(u, "sco", -20 * PPM)), 1),
       ("a block whose n rises above max_delay", lambda f, u: (setattr(u, "delay_fp", (65 << 32) - 1), setattr(u, "sco", 20 * PPM)), 1 << 20),
       ("a product beyond int64", lambda f, u: setattr(u, "sco", 1 << 38), 1 << 26),
       ("block - origin beyond int64", lambda f, u: setattr(u, "origin", -(1 << 63)), 1 << 40)]
SET_BAD = [b for b in BAD if "block" not in b[0] and "product" not in b[0]]      # those mcrx_hip_userclock_set refuses on a handle


@pytest.mark.parametrize("what,spoil,block", BAD, ids=[b[0] for b in BAD])
def test_configuration_errors_need_no_device(product, what, spoil, block):
    """the checks mcrx_hip_userclock_set and a call make, reached through the host self-test (the same cases on a handle are in
    tests/test_gpu_userclock.py)"""
    f, u = structs(product, delay=16.25)                                                    # (no drift: good at every block)
    assert selftest(product, f, u, block)[0] == product.MCRX_OK
    spoil(f, u)
    assert selftest(product, f, u, block)[0] == product.MCRX_EINVAL, what
    assert product.lib().mcrx_hip_userchan_last_error()
    if what.startswith(("sco", "delay_fp", "a block", "a product", "block")):
        u.enabled = 0                                                                       # a user without a clock is not looked at
        rc, tau, h = selftest(product, f, u, block)
        assert rc == product.MCRX_OK and tau == 0 and np.array_equal(h, np.eye(32, dtype=np.float32)[15])


def test_the_limits_themselves_are_accepted(product):
    for md, dfp, sco in ((15, 15 << 32, 0), (15, (16 << 32) - 1, 0), (255, (256 << 32) - 1, 1 << 38), (255, 15 << 32, -(1 << 38))):
        f, u = structs(product, max_delay=md, delay=15.0)
        u.delay_fp, u.sco = dfp, sco
        f.span_blocks = 8
        assert selftest(product, f, u, 0)[0] == product.MCRX_OK, (md, dfp, sco)
    # the steepest clock, 2^16 blocks from its origin: a product of -2^54, 64 samples down, still in range
    f, u = structs(product, max_delay=255, delay=100.0)
    u.sco, u.origin = -(1 << 38), 7
    assert selftest(product, f, u, 7 + (1 << 16))[0] == product.MCRX_OK


# ---------------------------------------------------------------------------------------------- integers and coefficients
# origin and b near 2^40, negative blocks, across 2^32, negative sco (floor is not truncate), both signs of b - origin
INTS = [dict(delay=16.25, ppm=20.0, origin=0, blocks=[0, 1, 7, 1000, 123457, (1 << 20) + 3]),
        dict(delay=40.5, ppm=-20.0, origin=0, blocks=[1, 3, 5, 11, 99999, 1 << 19]),
        dict(delay=30.0, ppm=-900.0, origin=(1 << 40) + 5, blocks=[(1 << 40) + 5, (1 << 40) + 6, (1 << 40) + 12345, (1 << 40) - 3, (1 << 40) - 9999]),
        dict(delay=33.987654321, ppm=137.5, origin=-(1 << 40), blocks=[-(1 << 40) - 1, -(1 << 40) + 1, -(1 << 40) + 54321, -(1 << 40) - 54321]),
        dict(delay=20.75, ppm=3.0, origin=(1 << 32) - 100, blocks=[(1 << 32) - 101, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 32) + 777]),
        dict(delay=17.0, ppm=-0.001, origin=0, blocks=[-1, -2, -65536, -65537, 1, 65536])]


@pytest.mark.parametrize("case", INTS, ids=["plus20", "minus20", "near_2^40", "near_minus_2^40", "across_2^32", "one_unit_of_sco"])
def test_selftest_equals_the_model(product, case):
    """tau_fp is the model's Python integer, exactly; h is the model's exact fp32 restatement from the library's own table, exactly"""
    W32 = library_table(product)
    f, u = structs(product, max_delay=64, delay=case["delay"], ppm=case["ppm"], origin=case["origin"])
    assert integers(u) == kmodel.user_of(case["delay"], case["ppm"], case["origin"]) and u.enabled == 1
    seen = set()
    for b in case["blocks"]:
        rc, tau, h = selftest(product, f, u, b)
        assert rc == product.MCRX_OK, (b, product.lib().mcrx_hip_userchan_last_error())
        want = kmodel.tau_fp(integers(u), b)
        assert tau == want, (b, tau, want)
        assert np.array_equal(h, kmodel.coefs_f32(W32, want & 0xFFFFFFFF)), b
        assert abs(float(h.astype(np.float64).sum()) - 1.0) < 1e-3                           # (an interpolator: unit gain at 0 Hz)
        seen.add(want)
    assert len(seen) > 1 or u.sco == 0
    if u.sco < 0:                  # floor, not truncate: a negative product that is no multiple of 2^16 rounds down
        b = next(b for b in case["blocks"] if (u.sco * (b - u.origin)) < 0 and (u.sco * (b - u.origin)) % (1 << 16))
        p = u.sco * (b - u.origin)
        assert kmodel.tau_fp(integers(u), b) - u.delay_fp == -((-p) >> 16) - 1


def test_the_fraction_picks_rows_and_weights(product):
    """mu = 0 is row 0 (the unit vector of tap 15) exactly; the last fraction is all but row 64; between two rows the weights are linear"""
    W32 = library_table(product)
    f, u = structs(product, delay=16.0)
    assert np.array_equal(selftest(product, f, u, 0)[2], np.eye(32, dtype=np.float32)[15])
    u.delay_fp = (17 << 32) - 1
    h = selftest(product, f, u, 0)[2]
    assert np.argmax(h) == 16 and abs(float(h[16]) - 1.0) < 1e-6 and not np.array_equal(h, W32[64])
    u.delay_fp = (16 << 32) + (5 << 26) + (1 << 25)                                          # half way between rows 5 and 6
    h = selftest(product, f, u, 0)[2]
    assert np.allclose(h, 0.5 * (W32[5].astype(np.float64) + W32[6]), rtol=0, atol=2.0 ** -24)
    u.delay_fp = (16 << 32) + (5 << 26) + 3                                                  # the low two bits are not used
    assert np.array_equal(selftest(product, f, u, 0)[2], W32[5])


def test_table_against_the_formula(product):
    """within 1 fp32 ulp of each entry's magnitude or 1e-9, whichever is larger (the Bessel series differ in the last bits); rows 0 and 64
    are exactly the unit vectors"""
    W32 = library_table(product)
    W64 = kmodel.table_f64()
    tol = np.maximum(np.spacing(np.abs(W64).astype(np.float32)).astype(np.float64), 1e-9)
    dev = np.abs(W32.astype(np.float64) - W64)
    assert np.all(dev <= tol), float((dev / tol).max())
    assert np.array_equal(W32[0], np.eye(32, dtype=np.float32)[15]) and np.array_equal(W32[64], np.eye(32, dtype=np.float32)[16])
    assert 0.9 < W32[32, 15] / W32[32, 16] < 1.1 and W32[32, 15] > 0.6                       # the half-sample row is symmetric about it


# ---------------------------------------------------------------------------------------------- the interpolator's quality
def test_quality_of_the_interpolator(product):
    """A condition on the defined table, computed here from the library's own: the worst |sum_j h_j e^{-2 pi i f (j - 15)} -
    e^{-2 pi i f mu}|.  On a 1/256 grid of mu it is -58.9 dB for |f| <= 0.41 and -56.0 dB for |f| <= 0.44 cycles per sample (the default
    allocations occupy |f| <= 0.406, 0.417 and 0.402 at M = 64, 48 and 256).  Asserted: <= -54 dB on |f| <= 0.44 over a 1/1024 grid and
    331 frequencies -- 2 dB over the figure found, for the denser grid."""
    W32 = library_table(product)
    a, b = kmodel.frequency_error_db(W32, 0.41, 256, 165), kmodel.frequency_error_db(W32, 0.44, 256, 165)
    dense = kmodel.frequency_error_db(W32, 0.44, 1024, 331)
    print("userclock interpolator: %.2f dB on |f| <= 0.41, %.2f dB on |f| <= 0.44 (mu / 256); %.2f dB on the 1/1024 grid" % (a, b, dense))
    assert dense <= -54.0, dense
    assert a <= -58.0 and b <= -55.0, (a, b)


# ---------------------------------------------------------------------------------------------- the model
def test_model_rounding_and_shift():
    from fractions import Fraction
    for v in (1.0, -0.3, 1e-3, 2.0 ** -130, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 16777217.0):
        assert kmodel.f32_round(Fraction(v)) == float(np.float32(v)), v
    assert kmodel.f32_round(Fraction(1) + Fraction(1, 1 << 24) + Fraction(1, 1 << 60)) == float(np.float32(1.0) + np.float32(2.0 ** -23))
    u = kmodel.user_of(20.0, -1.0)
    assert u["sco"] == -281474977 and kmodel.tau_fp(u, 1) == (20 << 32) - 4295                # floor(-281474977 / 65536) = -4295
    # an integer delay moves the samples, nothing else
    x = np.arange(200, dtype=np.float64) * (1 + 0.5j)
    z, hsum, n0, n1 = kmodel.z_channel(x, kmodel.user_of(23.0), kmodel.table_f64().astype(np.float32), 0, 72, 0)
    assert np.array_equal(z, x[72 - 23:72 - 23 + 128]) and (hsum, n0, n1) == (1.0, 23, 23)


# ---------------------------------------------------------------------------------------------- Python arguments
def test_helper_and_structures(product):
    f, users = product.userchan_clock(3, max_delay=40, span_blocks=64, users=[dict(delay=16.25, ppm=20.0, origin=-5), None, dict(delay=15)])
    assert (f.struct_size, f.user_struct_size, f.max_delay, f.span_blocks) == (16, 32, 40, 64)
    assert [u.enabled for u in users] == [1, 0, 1]
    assert (users[0].delay_fp, users[0].sco, users[0].origin) == (int(16.25 * 2 ** 32), 5629499534, -5)      # rint(20e-6 * 2^48)
    assert (users[2].delay_fp, users[2].sco, users[2].origin) == (15 << 32, 0, 0)
    assert product.userclock_user(64, 16.0, ppm=1.0).sco == PPM
    # what shard() does: the structures of the users it keeps
    g, part = product.userchan_clock(2, max_delay=40, span_blocks=64, users=[users[1], users[0]])
    assert [u.enabled for u in part] == [0, 1] and part[1].delay_fp == users[0].delay_fp and part[1].origin == -5


CH = [dict(taps=[(0, 1.0), (3, 0.5j)])]
USER = dict(delay=16.5, ppm=20.0)
PY_BAD = [dict(max_delay=14, users=[USER]), dict(max_delay=256, users=[USER]), dict(max_delay=20.5, users=[USER]),
          dict(span_blocks=12, users=[USER]), dict(span_blocks=-8, users=[USER]), dict(users=[]), dict(users=[USER, USER]), dict(),
          dict(users=[dict(ppm=1.0)]), dict(users=[dict(delay=float("nan"))]), dict(users=[dict(delay=16.0, ppm=float("inf"))]),
          dict(users=[dict(delay=14.99)]), dict(users=[dict(delay=65.0)]), dict(max_delay=15, users=[dict(delay=16.0)]),
          dict(users=[dict(delay=16.0, ppm=977.0)]), dict(users=[dict(delay=16.0, ppm=-977.0)]),
          dict(users=[dict(delay=16.0, origin=0.5)]), dict(users=[dict(delay=16.0, origin=1 << 63)]),
          dict(users=[dict(dely=16.0)]), dict(users=["late"]), dict(user=[USER]), "late"]


@pytest.mark.parametrize("kw", PY_BAD, ids=[str(i) for i in range(len(PY_BAD))])
def test_python_class_raises_value_error_without_a_device(product, kw):
    with pytest.raises(ValueError):
        product.userchan(channels=CH, clock=kw)
