"""Amplifier with memory (mcrx_hip_pamem_*), what needs no GPU: the boundary -- symbols, null handles, every configuration error reported
before a device is looked for --, the library's host arithmetic (lead, r_b, the flattened taps) against tests/pamem_model.py, the model
against mpd_model.memory_amplifier on mpd_model.SEVERITY's branches, pamem_small_signal against the definition, and the host program of
the plan plain and under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mpd_model
import pamem_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mcrx_hip_pamem_clipped", "mcrx_hip_pamem_create", "mcrx_hip_pamem_destroy", "mcrx_hip_pamem_execute_device",
           "mcrx_hip_pamem_input_format", "mcrx_hip_pamem_last_error", "mcrx_hip_pamem_lead", "mcrx_hip_pamem_output_format",
           "mcrx_hip_pamem_selftest"]
NAN, INF = float("nan"), float("inf")
BRANCHES = [dict(sat=0.5, smooth=1, gain=1.1, ampm_deg=4.0, taps=[(0, 1.0)]),
            dict(sat=0.75, smooth=2, gain=0.9, ampm_deg=-7.0, taps=[(1, 0.1 - 0.2j), (4, 0.0)]),
            dict(sat=1.5, smooth=4, taps=[(0, 0.02j), (2, -0.01), (16, 0.03 + 0.01j)])]


# ---------------------------------------------------------------------------------------------- the boundary
def test_symbols_are_declared_exported_and_bound(product):
    text = open(os.path.join(ROOT, "include", "mcrx_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(mcrx_hip_pamem_[a-z_0-9]+)\s*\(", text))) == SYMBOLS
    assert [s for s in product.exported_symbols() if s.startswith("mcrx_hip_pamem_")] == SYMBOLS
    L = product.lib()
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", product.build()]).decode()
    assert sorted(set(re.findall(r" T (mcrx_hip_pamem_[a-z_0-9]+)", out))) == SYMBOLS
    assert C.sizeof(product.PamemBranch) == 29 * 4 and C.sizeof(product.PamemConfig) == 5 * 4 + 4 * 29 * 4
    assert (product.PAMEM_MAX_BRANCHES, product.PAMEM_MAX_TAPS, product.PAMEM_MAX_DELAY) == (4, 8, 16)
    assert (model.MAX_BRANCHES, model.MAX_TAPS, model.MAX_DELAY) == (4, 8, 16)


def good_config(product):
    return product.pamem_config(BRANCHES, gain=0.9, input_format="cf32", output_format="sc16")


def selftest(L, c):
    return L.mcrx_hip_pamem_selftest(C.addressof(c), None, None, None, None, None, None)


def test_null_handles_are_answered(product):
    L = product.lib()
    assert L.mcrx_hip_pamem_output_format(None) == 0 and L.mcrx_hip_pamem_input_format(None) == 0 and L.mcrx_hip_pamem_lead(None) == 0
    assert L.mcrx_hip_pamem_destroy(None) == product.MCRX_OK
    n = C.c_uint64(7)
    for rc in (L.mcrx_hip_pamem_clipped(None, C.byref(n), 0), L.mcrx_hip_pamem_execute_device(None, None, 0, None, None),
               L.mcrx_hip_pamem_create(None, None), L.mcrx_hip_pamem_selftest(None, None, None, None, None, None, None)):
        assert rc == product.MCRX_EINVAL
    assert L.mcrx_hip_pamem_last_error()
    h = C.c_void_p(0x1234)
    assert L.mcrx_hip_pamem_create(C.byref(h), None) == product.MCRX_EINVAL and not h.value


def edit(c, field, value):
    if isinstance(field, tuple):
        br = c.branch[field[0]]
        if len(field) == 3:
            getattr(br, field[1])[field[2]] = value
        else:
            setattr(br, field[1], value)
    else:
        setattr(c, field, value)


BAD = [("struct_size", "struct_size", 480, b"struct_size"), ("branches 0", "branches", 0, b"branches"), ("branches 5", "branches", 5, b"branches"),
       ("input format", "input_format", 2, b"input format"), ("output format", "output_format", 2, b"output format"),
       ("gain nan", "gain", NAN, b"gain must be finite"), ("gain inf", "gain", INF, b"gain must be finite"),
       ("taps 0", (1, "taps"), 0, b"taps must be 1 .. 8"), ("taps 9", (1, "taps"), 9, b"taps must be 1 .. 8"),
       ("delay 17", (2, "delay", 2), 17, b"at most 16"), ("delay equal", (2, "delay", 2), 2, b"increase strictly"),
       ("delay falling", (1, "delay", 0), 5, b"increase strictly"), ("weight nan", (0, "h_re", 0), NAN, b"weights must be finite"),
       ("weight inf", (2, "h_im", 1), INF, b"weights must be finite"), ("smooth 3", (0, "smooth"), 3, b"amp_smooth"),
       ("sat 0", (1, "sat"), 0.0, b"amp_sat"), ("sat negative", (1, "sat"), -1.0, b"amp_sat"), ("sat nan", (1, "sat"), NAN, b"amp_sat"),
       ("sat inf", (1, "sat"), INF, b"amp_sat"), ("sat too small for r", (1, "sat"), 1e-30, b"1 / amp_sat^2"),
       ("sat too large for r", (1, "sat"), 3e30, b"1 / amp_sat^2"), ("amp_gain nan", (2, "amp_gain"), NAN, b"amp_gain"),
       ("amp_gain inf", (2, "amp_gain"), INF, b"amp_gain"), ("ampm beyond a quarter turn", (0, "ampm"), 0.26, b"amp_ampm"),
       ("ampm nan", (0, "ampm"), NAN, b"amp_ampm")]


@pytest.mark.parametrize("what,field,value,message", BAD, ids=[b[0] for b in BAD])
def test_configuration_errors_come_before_the_device(product, what, field, value, message):
    L = product.lib()
    c = good_config(product)
    edit(c, field, value)
    h = C.c_void_p(0x1234)
    assert L.mcrx_hip_pamem_create(C.byref(h), C.addressof(c)) == product.MCRX_EINVAL, what
    assert not h.value                                                                     # *out is cleared
    assert message in L.mcrx_hip_pamem_last_error(), L.mcrx_hip_pamem_last_error()
    assert selftest(L, c) == product.MCRX_EINVAL and message in L.mcrx_hip_pamem_last_error(), what


def test_the_amplifier_fields_are_judged_as_rfchain_judges_them(product):
    """the same value in the same field of an amplifier-only rfchain configuration and of a branch: the same verdict, the same words"""
    L = product.lib()
    for field, rf_field, values in (("sat", "amp_sat", (0.0, -1.0, NAN, INF, 1e-30, 3e30, 1e-18, 1e18)), ("smooth", "amp_smooth", (0, 1, 2, 3, 4, 5)),
                                    ("amp_gain", "amp_gain", (NAN, INF, 0.0, -2.0)), ("ampm", "amp_ampm", (0.25, -0.25, 0.26, NAN))):
        for v in values:
            c = good_config(product)
            setattr(c.branch[1], field, v)
            r = product.rfchain_config(amplifier=dict(sat=0.5))
            setattr(r, rf_field, v)
            h, g = C.c_void_p(), C.c_void_p()
            rc, rr = L.mcrx_hip_pamem_create(C.byref(h), C.addressof(c)), L.mcrx_hip_rfchain_create(C.byref(g), C.addressof(r))
            assert (rc == product.MCRX_EINVAL) == (rr == product.MCRX_EINVAL), (field, v)
            if rc == product.MCRX_EINVAL:
                assert L.mcrx_hip_pamem_last_error() == L.mcrx_hip_rfchain_last_error(), (field, v)
            if rc == product.MCRX_OK:
                L.mcrx_hip_pamem_destroy(h)
            if rr == product.MCRX_OK:
                L.mcrx_hip_rfchain_destroy(g)


def test_the_limits_themselves_are_accepted(product):
    """on the allowed side of every bound the answer is a handle, or 'no device' here -- never MCRX_EINVAL; branches at index >=
    `branches` and taps at index >= `taps` are not looked at"""
    L = product.lib()
    edits = [[("branches", 1)], [("branches", 2), ((2, "taps"), 99), ((2, "sat"), NAN), ((2, "smooth"), 7)], [((3, "taps"), 0)], [("input_format", 1)],
             [("output_format", 0)], [("gain", 0.0)], [("gain", -3.0)], [((0, "h_re", 0), 0.0)], [((0, "delay", 0), 16)],
             [((1, "delay", 5), 99), ((1, "h_re", 7), NAN)], [((0, "ampm"), 0.25)], [((0, "ampm"), -0.25)], [((1, "amp_gain"), -2.0)],
             [((1, "sat"), 1e-18)], [((1, "sat"), 1e18)]]
    for es in edits:
        c = good_config(product)
        for field, value in es:
            edit(c, field, value)
        assert selftest(L, c) == product.MCRX_OK, (es, L.mcrx_hip_pamem_last_error())
        h = C.c_void_p()
        rc = L.mcrx_hip_pamem_create(C.byref(h), C.addressof(c))
        assert rc in (product.MCRX_OK, product.MCRX_EHIP), (es, L.mcrx_hip_pamem_last_error())
        if rc == product.MCRX_OK:
            assert L.mcrx_hip_pamem_output_format(h) == c.output_format and L.mcrx_hip_pamem_input_format(h) == c.input_format
            L.mcrx_hip_pamem_destroy(h)
    product.pamem_config([dict(sat=1.0, taps=[(2 * k, 0.1 * k) for k in range(8)])] * 4)


OK_BRANCH = dict(sat=1.0, taps=[(0, 1.0), (3, 0.1j)])
PY_BAD = [dict(branches=None), dict(branches=[]), dict(branches=[OK_BRANCH] * 5), dict(branches=[dict(taps=[(0, 1.0)])]), dict(branches=[dict(OK_BRANCH, knee=1)]),
          dict(branches=[dict(OK_BRANCH, taps=[])]), dict(branches=[dict(OK_BRANCH, taps=[(k, 1.0) for k in range(9)])]),
          dict(branches=[dict(OK_BRANCH, taps=[(0, 1.0), (0, 1.0)])]), dict(branches=[dict(OK_BRANCH, taps=[(3, 1.0), (1, 1.0)])]),
          dict(branches=[dict(OK_BRANCH, taps=[(17, 1.0)])]), dict(branches=[dict(OK_BRANCH, taps=[(1.5, 1.0)])]), dict(branches=[dict(OK_BRANCH, taps=[(-1, 1.0)])]),
          dict(branches=[dict(OK_BRANCH, taps=[(0, NAN)])]), dict(branches=[dict(OK_BRANCH, taps=[(0, complex(0, INF))])]), dict(branches=[dict(OK_BRANCH, taps=[0, 1.0])]),
          dict(branches=[dict(OK_BRANCH, sat=0.0)]), dict(branches=[dict(OK_BRANCH, sat=NAN)]), dict(branches=[dict(OK_BRANCH, smooth=3)]),
          dict(branches=[dict(OK_BRANCH, smooth=2.5)]), dict(branches=[dict(OK_BRANCH, gain=INF)]), dict(branches=[dict(OK_BRANCH, ampm_deg=91.0)]),
          dict(branches=[OK_BRANCH], gain=NAN), dict(branches=[OK_BRANCH], input_format="sc8"), dict(branches=[OK_BRANCH], output_format=2),
          dict(branches=[OK_BRANCH, "second"])]


@pytest.mark.parametrize("kw", PY_BAD, ids=[str(i) for i in range(len(PY_BAD))])
def test_python_class_raises_value_error_without_a_device(product, kw):
    with pytest.raises(ValueError):
        product.pamem(**kw)
    with pytest.raises(ValueError):
        product.pamem_config(**kw)


# ---------------------------------------------------------------------------------------------- the host arithmetic
def test_selftest_returns_what_the_model_computes(product):
    for branches in (BRANCHES, BRANCHES[:1], BRANCHES[1:2], [dict(sat=0.3, taps=[(k, 0.5 ** k * np.exp(0.3j * k)) for k in range(0, 16, 2)])] * 4):
        c = product.pamem_config(branches)
        lead, r, taps = product.pamem_constants(c)
        assert lead == model.lead_of(c) == max(d for b in branches for d, _ in b["taps"])
        assert np.array_equal(np.array(r, np.float32).view(np.uint32), np.array(model.inv_sat2(c), np.float32).view(np.uint32))
        want = model.flat_taps(c)
        assert len(taps) == len(want) == sum(len(b["taps"]) for b in branches)
        for (b, d, h), (wb, wd, wh) in zip(taps, want):
            assert (b, d) == (wb, wd) and h == wh
        assert [(b, d) for b, d, _ in taps] == [(b, d) for b, br in enumerate(branches) for d, _ in br["taps"]]
        assert all(h == complex(np.complex64(w)) for (_, _, h), w in zip(taps, [w for br in branches for _, w in br["taps"]]))
    assert product.pamem_constants(product.pamem_config([dict(sat=0.5)])) == (0, [4.0], [(0, 0, 1 + 0j)])


def severity_branches(product, rms):
    """mpd_model.SEVERITY's amplifier as pamem branches: three single-tap branches on delays 0, 1, 2"""
    v = mpd_model.SEVERITY
    return [dict(sat=product.rfchain_backoff(ibo, rms), smooth=v["amp_smooth"], gain=v["amp_gain"], ampm_deg=deg, taps=[(b, w)])
            for b, (ibo, deg, w) in enumerate(zip(v["amp_ibo_db"], v["amp_ampm_deg"], v["amp_weights"]))]


def test_model_equals_the_memory_amplifier_of_the_mpd_case(product):
    """on mpd_model.SEVERITY's branches the model is mpd_model.memory_amplifier within 1e-12 of the peak: both float64, they differ in
    the order of the sum and in the weights, which a configuration holds as fp32 -- so the comparison is on the weights it holds"""
    v, rms = mpd_model.SEVERITY, 0.11
    rng = np.random.RandomState(5)
    u = (rms * (rng.standard_normal(5000) + 1j * rng.standard_normal(5000)) / np.sqrt(2.0)).astype(np.complex64)
    c = product.pamem_config(severity_branches(product, rms))
    assert model.lead_of(c) == 2
    y, bound = model.apply(c, np.concatenate([np.zeros(2, np.complex64), u]))
    cfgs = [product.rfchain_config(amplifier=dict(sat=product.rfchain_backoff(ibo, rms), smooth=v["amp_smooth"], gain=v["amp_gain"], ampm_deg=deg))
            for ibo, deg in zip(v["amp_ibo_db"], v["amp_ampm_deg"])]
    held = [h for _, _, h in model.flat_taps(c)]
    want = mpd_model.memory_amplifier(cfgs, held, u)
    peak = np.abs(want).max()
    assert y.shape == want.shape and np.abs(y - want).max() <= 1e-12 * peak
    assert np.abs(want - mpd_model.memory_amplifier(cfgs, v["amp_weights"], u)).max() <= 2.0 ** -24 * 1.2 * peak      # the fp32 weights
    assert bound.shape == (5000,) and np.all(bound > 0) and bound.max() < 1e-5 * peak


def test_small_signal_is_the_definition(product):
    H = product.pamem_small_signal(BRANCHES)
    c = product.pamem_config(BRANCHES)
    assert H.dtype == np.complex128 and H.shape == (17,)
    want = np.zeros(17, np.complex128)
    for br in BRANCHES:
        for d, w in br["taps"]:
            want[d] += float(np.float32(br.get("gain", 1.0))) * complex(np.complex64(w))
    assert np.array_equal(H, want) and np.array_equal(H, model.small_signal(c))
    assert H[0] == float(np.float32(1.1)) + complex(np.complex64(0.02j)) and H[3] == 0 and H[16] == complex(np.complex64(0.03 + 0.01j))
    # the linear regime of the model is that FIR: a drive 1e-5 of the smallest saturation amplitude (t < 1e-8), AM/PM off
    lin = [dict(b, ampm_deg=0.0) for b in BRANCHES]
    cl = product.pamem_config(lin)
    rng = np.random.RandomState(1)
    u = (5e-6 * (rng.standard_normal(400) + 1j * rng.standard_normal(400))).astype(np.complex64)
    y, _ = model.apply(cl, u)
    fir = np.convolve(u.astype(np.complex128), product.pamem_small_signal(lin))[16:400]
    assert np.abs(y - fir).max() <= 1e-7 * np.abs(fir).max()
    with pytest.raises(ValueError):
        product.pamem_small_signal([dict(sat=1.0, taps=[(17, 1.0)])])


@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitizers"])
def test_host_program_of_the_plan(product, san):
    """host/pamem_plan_test.cc: csrc/pamem_plan.hpp with a main of its own (no GPU, no Python), plain and under the address and
    undefined-behaviour sanitizers"""
    host = os.path.join(ROOT, "liquid-usrp_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "pamem_plan_test"] + (["SAN=1"] if san else []))
    out = subprocess.run([os.path.join(ROOT, "liquid-usrp_amd", "lib", "pamem_plan_test" + ("_san" if san else ""))], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT)
    assert out.returncode == 0 and b"pamem_plan_test ok" in out.stdout, out.stdout.decode()
