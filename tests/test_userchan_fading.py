"""Fading rays per user of the per-user channel emulator (mcrx_hip_userfade_*), what needs no GPU: the
boundary, every configuration error through the host self-test, the integers the library makes against the model's own Philox
restatement, the model's mean power, and the Python argument handling."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import chanemu_fading_model as cmodel
import userchan_fading_model as fmodel
from test_chanemu_fading import NEW as CHANFADE_SYMBOLS
from test_chanemu_fading import selftest as chanfade_selftest
from test_userchan import SYMBOLS as USERCHAN_SYMBOLS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mcrx_hip_userfade_gains", "mcrx_hip_userfade_on", "mcrx_hip_userfade_selftest", "mcrx_hip_userfade_set"]


def selftest(product, f, u, ray):
    """the library's integers of one ray: (steps, phases, (c_los, c_sc)), a table of tests/userchan_fading_model.py"""
    S = int(f.num_sinusoids)
    steps, phases, coef = (C.c_int64 * 17)(), (C.c_uint32 * 17)(), (C.c_float * 2)()
    rc = product.lib().mcrx_hip_userfade_selftest(C.addressof(f), C.addressof(u), ray, steps, phases, coef)
    assert rc == product.MCRX_OK, product.lib().mcrx_hip_userchan_last_error()
    return [int(v) for v in steps[:S + 1]], [int(v) for v in phases[:S + 1]], (float(coef[0]), float(coef[1]))


def library_tables(product, structs, rays):
    """per channel: None for a user who does not fade, else one table per ray"""
    f, users = structs
    return [[selftest(product, f, users[c], i) for i in range(T)] if users[c].enabled else None for c, T in enumerate(rays)]


# ---------------------------------------------------------------------------------------------- the boundary
def test_symbols_are_declared_exported_and_bound(product):
    text = open(os.path.join(ROOT, "include", "mcrx_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", product.build()]).decode()
    for prefix, want in (("mcrx_hip_userfade_", NEW), ("mcrx_hip_userchan_", USERCHAN_SYMBOLS), ("mcrx_hip_chanfade_", CHANFADE_SYMBOLS)):
        assert sorted(set(re.findall(r"\b(%s[a-z_0-9]+)\s*\(" % prefix, text))) == want
        assert [s for s in product.exported_symbols() if s.startswith(prefix)] == want
        assert sorted(set(re.findall(r" T (%s[a-z_0-9]+)" % prefix, out))) == want
    for s in NEW:
        assert getattr(product.lib(), s).argtypes is not None
    assert C.sizeof(product.UserfadeUser) == 8 + 4 * (8 + 8 + 4 + 4) and C.sizeof(product.UserfadeConfig) == 32
    assert C.sizeof(product.UserchanChannel) == 4 * (1 + 3 * 4 + 3)                          # the channel structure is the parent's
    assert "MCRX_USERFADE_MIN_LOG2_BLOCK 3" in text and "MCRX_USERFADE_MAX_LOG2_BLOCK 20" in text
    assert (product.USERFADE_MIN_LOG2_BLOCK, product.USERFADE_MAX_LOG2_BLOCK) == (3, 20)
    for m in ("set_fading", "fading_on", "gains"):
        assert callable(getattr(product.userchan, m))


def good(product, **kw):
    args = dict(log2_block=10, sinusoids=8, seed=5, users=[dict(doppler=1e-5, rice_k=1.0, los_doppler=-1e-5)])
    args.update(kw)
    f, users = product.userchan_fading([4], **args)
    return f, users[0]


def test_null_handles_are_answered(product):
    L, EINVAL = product.lib(), product.MCRX_EINVAL
    f, u = good(product)
    assert L.mcrx_hip_userfade_on(None) == 0
    assert L.mcrx_hip_userfade_set(None, C.addressof(f), C.addressof(u)) == EINVAL
    assert L.mcrx_hip_userfade_set(None, None, None) == EINVAL
    assert L.mcrx_hip_userfade_gains(None, 0, 1, None, None) == EINVAL
    assert L.mcrx_hip_userchan_last_error()
    steps, phases, coef = (C.c_int64 * 17)(), (C.c_uint32 * 17)(), (C.c_float * 2)()
    assert L.mcrx_hip_userfade_selftest(None, C.addressof(u), 0, steps, phases, coef) == EINVAL
    assert L.mcrx_hip_userfade_selftest(C.addressof(f), None, 0, steps, phases, coef) == EINVAL
    assert L.mcrx_hip_userfade_selftest(C.addressof(f), C.addressof(u), 0, None, phases, coef) == EINVAL
    assert L.mcrx_hip_userfade_selftest(C.addressof(f), C.addressof(u), 4, steps, phases, coef) == EINVAL


# ---------------------------------------------------------------------------------------------- configuration errors
BAD = [("struct_size", lambda f, u: setattr(f, "struct_size", f.struct_size - 4)),
       ("user_struct_size", lambda f, u: setattr(f, "user_struct_size", f.user_struct_size + 8)),
       ("L 2", lambda f, u: setattr(f, "log2_block", 2)),
       ("L 21", lambda f, u: setattr(f, "log2_block", 21)),
       ("S zero", lambda f, u: setattr(f, "num_sinusoids", 0)),
       ("S 17", lambda f, u: setattr(f, "num_sinusoids", 17)),
       ("one row", lambda f, u: setattr(f, "table_rows", 1)),
       ("doppler nan", lambda f, u: u.doppler.__setitem__(2, float("nan"))),
       ("doppler inf", lambda f, u: u.doppler.__setitem__(2, float("inf"))),
       ("los doppler nan", lambda f, u: u.los_doppler.__setitem__(2, float("nan"))),
       ("doppler negative", lambda f, u: u.doppler.__setitem__(2, -1e-6)),
       ("doppler too fast", lambda f, u: u.doppler.__setitem__(2, 0.126 / 1024)),
       ("los doppler too fast", lambda f, u: u.los_doppler.__setitem__(2, -0.126 / 1024)),
       ("rice negative", lambda f, u: u.rice_k.__setitem__(2, -0.5)),
       ("rice nan", lambda f, u: u.rice_k.__setitem__(2, float("nan"))),
       ("rice inf", lambda f, u: u.rice_k.__setitem__(2, float("inf")))]


@pytest.mark.parametrize("what,spoil", BAD, ids=[b[0] for b in BAD])
def test_configuration_errors_need_no_device(product, what, spoil):
    """the check mcrx_hip_userfade_set makes, reached through the host self-test (the same cases on a handle are in
    tests/test_gpu_userchan_fading.py)"""
    L = product.lib()
    f, u = good(product)
    steps, phases, coef = (C.c_int64 * 17)(), (C.c_uint32 * 17)(), (C.c_float * 2)()
    assert L.mcrx_hip_userfade_selftest(C.addressof(f), C.addressof(u), 2, steps, phases, coef) == product.MCRX_OK
    spoil(f, u)
    coef[0] = -7.0
    assert L.mcrx_hip_userfade_selftest(C.addressof(f), C.addressof(u), 2, steps, phases, coef) == product.MCRX_EINVAL, what
    assert L.mcrx_hip_userchan_last_error() and coef[0] == -7.0                             # nothing written
    if "doppler" in what or "rice" in what:
        assert L.mcrx_hip_userfade_selftest(C.addressof(f), C.addressof(u), 1, steps, phases, coef) == product.MCRX_OK      # another ray
        u.enabled = 0                                                                       # a user who does not fade is not looked at
        assert L.mcrx_hip_userfade_selftest(C.addressof(f), C.addressof(u), 2, steps, phases, coef) == product.MCRX_OK


def test_the_limits_themselves_are_accepted(product):
    for Lb in (3, 20):
        B = float(1 << Lb)
        f, u = good(product, log2_block=Lb, table_rows=2, users=[dict(doppler=0.125 / B, los_doppler=-0.125 / B)])
        selftest(product, f, u, 3)


# ---------------------------------------------------------------------------------------------- the integers
CASES = [dict(seed=4, id=0, S=8, L=10, doppler=3e-6, rice_k=[8.0, 0.0, 0.5, 2.0], los_doppler=[0.9e-6, 0.0, -2e-6, 1e-6],
              los_phase=[0x12345678, 0, 0xFFFFFFFF, 7]),
         dict(seed=0xC0FFEE0123456789, id=1023, S=16, L=6, doppler=[2.0 ** -12, 0.0, 1e-3, 1e-4], rice_k=0.0, los_doppler=0.0, los_phase=0),
         dict(seed=1, id=0xFFFFFFFF, S=1, L=3, doppler=[0.015625, 0.01, 0.0, 0.002], rice_k=[1e6, 3.0, 0.0, 1.0],
              los_doppler=[-0.015625, 0.015625, 0.0, 0.0], los_phase=0x9E3779B9)]


def case_structs(product, kw, **over):
    kw = dict(kw, **over)
    user = dict(doppler=kw["doppler"], rice_k=kw["rice_k"], los_doppler=kw["los_doppler"], los_phase=kw["los_phase"], id=kw["id"])
    f, users = product.userchan_fading([4], log2_block=kw["L"], sinusoids=kw["S"], seed=kw["seed"], users=[user])
    return f, users[0]


@pytest.mark.parametrize("kw", CASES, ids=["rician", "rayleigh", "edges"])
def test_selftest_tables_equal_the_model(product, kw):
    """phases (Philox words of counter (k, ray, 2, id)) exact; steps within 2^-50 |step| + 1 (libm and numpy may differ in cos by an
    ulp); coefficients exact as fp32"""
    f, u = case_structs(product, kw)
    assert (f.log2_block, f.num_sinusoids, f.seed, u.id, u.enabled) == (kw["L"], kw["S"], kw["seed"], kw["id"], 1)
    want = fmodel.tables(f.seed, u.id, list(u.doppler), list(u.los_doppler), list(u.rice_k), list(u.los_phase), f.num_sinusoids)
    for i in range(4):
        steps, phases, coef = selftest(product, f, u, i)
        assert phases == want[i][1], i
        assert len(steps) == f.num_sinusoids + 1
        for a, b in zip(steps, want[i][0]):
            assert abs(a - b) <= 2.0 ** -50 * abs(b) + 1, (i, a, b)
        assert coef == want[i][2], (i, coef, want[i][2])
        assert abs(coef[0] ** 2 + f.num_sinusoids * coef[1] ** 2 - 1.0) < 1e-6              # E |g|^2 = 1
    # another id, another seed: other integers
    base = selftest(product, f, u, 1)[1][1:]
    assert selftest(product, *case_structs(product, kw, id=(kw["id"] + 1) % (1 << 32)), 1)[1][1:] != base
    assert selftest(product, *case_structs(product, kw, seed=kw["seed"] ^ 1), 1)[1][1:] != base
    # the third counter word: not the wideband emulator's integers for the same seed and ray, whatever the id -- they are the words
    # of counter (k, ray, 2, id), which the model's Philox gives directly
    cf = product.chanemu_fading(4, doppler=list(u.doppler), rice_k=list(u.rice_k), los_doppler=list(u.los_doppler),
                                los_phase=list(u.los_phase), sinusoids=kw["S"], log2_block=kw["L"], seed=kw["seed"])
    zero = selftest(product, *case_structs(product, kw, id=0), 3)                            # (ray 3 has a Doppler in every case)
    wide = chanfade_selftest(product, cf, 3)
    assert wide[1][0] == zero[1][0] and wide[1][1:] != zero[1][1:] and wide[0][1:] != zero[0][1:]
    w = fmodel.philox4x32_10((0, 1, 2, kw["id"]), (f.seed & 0xFFFFFFFF, f.seed >> 32))
    assert selftest(product, f, u, 1)[1][1] == int(w[1][0])


def test_a_user_who_does_not_fade_has_unit_gain(product):
    f, users = product.userchan_fading([2, 3], log2_block=4, sinusoids=8, seed=3, users=[None, dict(doppler=1e-3)])
    assert (users[0].enabled, users[0].id, users[1].enabled, users[1].id) == (0, 0, 1, 1)
    for i in range(4):
        assert selftest(product, f, users[0], i) == ([0] * 9, [0] * 9, (1.0, 0.0))
    G = cmodel.grid(fmodel.static_table(8), np.arange(5, dtype=np.uint64), 4)
    assert np.array_equal(G, np.ones(5, np.complex128))


# ---------------------------------------------------------------------------------------------- the model
def test_model_mean_power():
    """E|G|^2 = 1: the mean of |G|^2 over 1024 (id, ray) pairs at one row lies within 0.125 of 1 -- var |g|^2 <= 1 for any K >= 0,
    so this is four standard errors"""
    S, L, row = 8, 4, 12345
    p = []
    for uid in range(256):
        K = [0.0, 1.0, 4.0, 10.0][uid % 4]
        for t in fmodel.tables(77, uid, [1e-3] * 4, [2e-4] * 4, [K] * 4, [uid] * 4, S):
            p.append(abs(fmodel.grid_rows(t, row, 1, L)[0]) ** 2)
    assert len(p) == 1024
    m = float(np.mean(p))
    print("userchan fading: mean |G|^2 over 1024 (id, ray) pairs %.4f" % m)
    assert abs(m - 1.0) <= 0.125


def test_model_gain_is_linear_between_rows_and_signed():
    t = fmodel.tables(9, 3, [2e-3], [1e-3], [1.0], [5], 8)[0]
    L = 4
    for first in (-64, 0, (1 << 40) - 32):
        g, pk = fmodel.gain(t, first, 49, L)
        G = fmodel.grid_rows(t, first >> L, 5, L)                                           # blocks of four rows, and the row behind
        assert np.array_equal(g[::16], G[:4]) and abs(g[8] - 0.5 * (G[0] + G[1])) < 1e-15 and pk == float(np.abs(G).max())
    # a negative row is the row of the 64-bit position: n_r = (row << L) mod 2^64
    assert np.array_equal(fmodel.grid_rows(t, -4, 1, L), cmodel.grid(t, np.array([(1 << 60) - 4], np.uint64), L))


# ---------------------------------------------------------------------------------------------- Python arguments
def test_doppler_helper(product):
    assert product.userchan_doppler(0, 64, 8) == 0.0
    assert product.userchan_doppler(0.25, 64, 8) == 0.25 / 72
    assert product.userchan_doppler(1.0, 1024, 16) == 1.0 / 1040


def test_scalars_lists_and_ids(product):
    f, users = product.userchan_fading([3, 1, 4], log2_block=5, sinusoids=4, seed=-1, table_rows=2,
                                       users=[dict(doppler=1e-3, rice_k=[0.0, 2.0, 4.0], los_phase=-1), None,
                                              dict(doppler=[1e-3, 2e-3, 0.0, 3e-3], los_doppler=-1e-3, id=77)])
    assert (f.struct_size, f.user_struct_size) == (C.sizeof(product.UserfadeConfig), C.sizeof(product.UserfadeUser))
    assert (f.log2_block, f.num_sinusoids, f.table_rows, f.reserved, f.seed) == (5, 4, 2, 0, 2 ** 64 - 1)
    assert [u.enabled for u in users] == [1, 0, 1] and [u.id for u in users] == [0, 1, 77]
    assert list(users[0].doppler)[:3] == [1e-3] * 3 and list(users[0].rice_k)[:3] == [0.0, 2.0, 4.0]
    assert list(users[0].los_phase)[:3] == [0xFFFFFFFF] * 3 and list(users[0].los_doppler) == [0.0] * 4
    assert list(users[2].doppler) == [1e-3, 2e-3, 0.0, 3e-3] and list(users[2].los_doppler) == [-1e-3] * 4
    # what shard() does: the structures of the users it keeps, ids included, whatever their place in the new table
    g, part = product.userchan_fading([1, 4], log2_block=5, sinusoids=4, seed=f.seed, table_rows=2, users=[users[1], users[2]])
    assert [u.enabled for u in part] == [0, 1] and [u.id for u in part] == [1, 77]
    assert selftest(product, g, part[1], 3) == selftest(product, f, users[2], 3)


CH = [dict(taps=[(0, 1.0), (3, 0.5j)])]
USER = dict(doppler=1e-3)
PY_BAD = [dict(log2_block=2, users=[USER]), dict(log2_block=21, users=[USER]), dict(log2_block=4.5, users=[USER]),
          dict(sinusoids=0, users=[USER]), dict(sinusoids=17, users=[USER]), dict(table_rows=1, users=[USER]),
          dict(table_rows=-1, users=[USER]), dict(users=[]), dict(users=[USER, USER]), dict(), dict(users=[dict(rice_k=1.0)]),
          dict(users=[dict(doppler=float("nan"))]), dict(users=[dict(doppler=-1e-6)]), dict(users=[dict(doppler=0.126 / 16)]),
          dict(users=[dict(doppler=0.0, los_doppler=float("inf"))]), dict(users=[dict(doppler=0.0, los_doppler=-0.126 / 16)]),
          dict(users=[dict(doppler=0.0, rice_k=-1.0)]), dict(users=[dict(doppler=0.0, rice_k=float("nan"))]),
          dict(users=[dict(doppler=0.0, rice_k=1e39)]), dict(users=[dict(doppler=[1e-6] * 3)]), dict(users=[dict(doppler=0.0, los_phase=[0])]),
          dict(users=[dict(doppler=0.0, id=-1)]), dict(users=[dict(doppler=0.0, id=1 << 32)]), dict(users=[dict(dopler=1e-6)]),
          dict(users=["rayleigh"]), dict(user=[USER]), "rayleigh"]


@pytest.mark.parametrize("kw", PY_BAD, ids=[str(i) for i in range(len(PY_BAD))])
def test_python_class_raises_value_error_without_a_device(product, kw):
    with pytest.raises(ValueError):
        product.userchan(channels=CH, fading=kw)
