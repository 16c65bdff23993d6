"""Predistortion with memory (mcrx_hip_mpd_*), what needs no GPU: the boundary -- symbols, null handles, every configuration error
reported before a device is looked for --, the library's host arithmetic (constants, the integers of feedback and target samples)
against tests/mpd_model.py, the model against exact rational arithmetic where it claims exactness, the host program of the plan plain
and under the sanitizers, and the end-to-end case of tests/test_gpu_mpd.py found on the oracle alone with the exact models."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cfr_model
import dpd_model
import mpd_model as model
from test_dpd import decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mcrx_hip_mpd_clipped", "mcrx_hip_mpd_create", "mcrx_hip_mpd_destroy", "mcrx_hip_mpd_execute_device", "mcrx_hip_mpd_last_error",
           "mcrx_hip_mpd_lead", "mcrx_hip_mpd_measure_device", "mcrx_hip_mpd_output_format", "mcrx_hip_mpd_read", "mcrx_hip_mpd_reset",
           "mcrx_hip_mpd_selftest", "mcrx_hip_mpd_set_tables", "mcrx_hip_mpd_update"]
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------- the boundary
def test_symbols_are_declared_exported_and_bound(product):
    text = open(os.path.join(ROOT, "include", "mcrx_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(mcrx_hip_mpd_[a-z_0-9]+)\s*\(", text))) == SYMBOLS
    assert [s for s in product.exported_symbols() if s.startswith("mcrx_hip_mpd_")] == SYMBOLS
    L = product.lib()
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", product.build()]).decode()
    assert sorted(set(re.findall(r" T (mcrx_hip_mpd_[a-z_0-9]+)", out))) == SYMBOLS
    assert C.sizeof(product.MpdConfig) == 15 * 4 and C.sizeof(product.MpdState) == 5 * 8
    assert (product.MPD_MAX_BRANCHES, product.MPD_MAX_DELAY, product.MPD_MAX_ORDER, product.MPD_QB, product.MPD_GUARD_LOG2) == (4, 16, 5, 17, 26)
    assert (model.QB, model.GUARD_LOG2) == (product.MPD_QB, product.MPD_GUARD_LOG2)


def good_config(product):
    return product.mpd_config(3, (0, 1, 5), 5, 7, 0.75, 2.0, min_rows=15, ridge_log2=30, forget_shift=2, gain=0.9, output_format="sc16")


def test_null_handles_are_answered(product):
    L = product.lib()
    assert L.mcrx_hip_mpd_output_format(None) == 0 and L.mcrx_hip_mpd_lead(None) == 0
    assert L.mcrx_hip_mpd_destroy(None) == product.MCRX_OK
    n, st = C.c_uint64(7), product.MpdState()
    for rc in (L.mcrx_hip_mpd_clipped(None, C.byref(n), 0), L.mcrx_hip_mpd_execute_device(None, None, 0, None, None),
               L.mcrx_hip_mpd_measure_device(None, None, None, 0, None), L.mcrx_hip_mpd_update(None, None),
               L.mcrx_hip_mpd_set_tables(None, None, None), L.mcrx_hip_mpd_read(None, C.addressof(st), None, None, None, None),
               L.mcrx_hip_mpd_reset(None), L.mcrx_hip_mpd_create(None, None),
               L.mcrx_hip_mpd_selftest(None, None, None, None, None, None, None, 0, None, None, None)):
        assert rc == product.MCRX_EINVAL
    assert L.mcrx_hip_mpd_last_error()
    h = C.c_void_p(0x1234)
    assert L.mcrx_hip_mpd_create(C.byref(h), None) == product.MCRX_EINVAL and not h.value
    c = good_config(product)
    assert L.mcrx_hip_mpd_selftest(C.addressof(c), None, None, None, None, None, None, 3, None, None, None) == product.MCRX_EINVAL


def edit(c, field, value):
    if isinstance(field, tuple):
        c.delay[field[1]] = value
    else:
        setattr(c, field, value)


BAD = [("struct_size", "struct_size", 56), ("branches 0", "branches", 0), ("branches 5", "branches", 5), ("delay[0] 1", ("delay", 0), 1),
       ("delay[1] 0", ("delay", 1), 0), ("delay[2] equal", ("delay", 2), 1), ("delay[2] 17", ("delay", 2), 17), ("order 0", "order", 0),
       ("order 6", "order", 6), ("table_log2 4", "table_log2", 4), ("table_log2 11", "table_log2", 11), ("3 tables of 1024", "table_log2", 10),
       ("full_scale 0", "full_scale", 0.0), ("full_scale negative", "full_scale", -0.5), ("full_scale nan", "full_scale", NAN),
       ("full_scale inf", "full_scale", INF), ("full_scale too small for inv_step", "full_scale", 1e-42), ("target_gain 0", "target_gain", 0.0),
       ("target_gain negative", "target_gain", -1.0), ("target_gain nan", "target_gain", NAN), ("target_gain inf", "target_gain", INF),
       ("min_rows below L", "min_rows", 14), ("ridge_log2 9", "ridge_log2", 9), ("ridge_log2 41", "ridge_log2", 41),
       ("forget_shift 9", "forget_shift", 9), ("gain nan", "gain", NAN), ("gain inf", "gain", INF), ("output format", "output_format", 2)]


@pytest.mark.parametrize("what,field,value", BAD, ids=[b[0] for b in BAD])
def test_configuration_errors_come_before_the_device(product, what, field, value):
    L = product.lib()
    c = good_config(product)
    edit(c, field, value)
    h = C.c_void_p(0x1234)
    assert L.mcrx_hip_mpd_create(C.byref(h), C.addressof(c)) == product.MCRX_EINVAL, what
    assert not h.value                                                                     # *out is cleared
    assert L.mcrx_hip_mpd_last_error()
    assert L.mcrx_hip_mpd_selftest(C.addressof(c), None, None, None, None, None, None, 0, None, None, None) == product.MCRX_EINVAL, what


def test_the_limits_themselves_are_accepted(product):
    """on the allowed side of every bound the answer is a handle, or 'no device' here -- never MCRX_EINVAL"""
    L = product.lib()
    edits = [("table_log2", 5), ("table_log2", 9), (("delay", 2), 16), (("delay", 2), 2), ("order", 1), ("full_scale", 1e-30), ("full_scale", 3e38),
             ("target_gain", 1e-30), ("target_gain", 3e38), ("min_rows", 15), ("min_rows", 0xffffffff), ("ridge_log2", 10), ("ridge_log2", 40),
             ("forget_shift", 0), ("forget_shift", 8), ("gain", 0.0), ("gain", -3.0), ("output_format", 0), ("output_format", 1)]
    for field, value in edits:
        c = good_config(product)
        edit(c, field, value)
        h = C.c_void_p()
        rc = L.mcrx_hip_mpd_create(C.byref(h), C.addressof(c))
        assert rc in (product.MCRX_OK, product.MCRX_EHIP), (field, L.mcrx_hip_mpd_last_error())
        if rc == product.MCRX_OK:
            assert L.mcrx_hip_mpd_output_format(h) == c.output_format and L.mcrx_hip_mpd_lead(h) == c.delay[2]
            L.mcrx_hip_mpd_destroy(h)
    for kw in (dict(branches=1, delays=(0,), table_log2=10), dict(branches=2, delays=(0, 16), table_log2=10),
               dict(branches=4, delays=(0, 1, 2, 3), table_log2=9, order=5, min_rows=20)):
        product.mpd_config(full_scale=1.0, target_gain=1.0, **kw)


OK_KW = dict(branches=2, delays=(0, 1), full_scale=1.0, target_gain=1.0)
PY_BAD = [dict(), dict(branches=2, delays=(0, 1), full_scale=1.0), dict(branches=2, delays=(0, 1), target_gain=1.0), dict(OK_KW, delays=None),
          dict(OK_KW, branches=None), dict(OK_KW, delays=(0,)), dict(OK_KW, delays=(0, 1, 2)), dict(OK_KW, delays=(1, 2)), dict(OK_KW, delays=(0, 0)),
          dict(OK_KW, delays=(0, 17)), dict(OK_KW, delays=(0, 1.5)), dict(OK_KW, delays=(0, -1)), dict(OK_KW, branches=0, delays=()),
          dict(OK_KW, branches=5, delays=(0, 1, 2, 3, 4)), dict(OK_KW, order=0), dict(OK_KW, order=6), dict(OK_KW, order=2.5), dict(OK_KW, table_log2=4),
          dict(OK_KW, table_log2=11), dict(OK_KW, branches=3, delays=(0, 1, 2), table_log2=10), dict(OK_KW, full_scale=0.0), dict(OK_KW, full_scale=NAN),
          dict(OK_KW, full_scale=INF), dict(OK_KW, target_gain=0.0), dict(OK_KW, target_gain=NAN), dict(OK_KW, min_rows=9), dict(OK_KW, min_rows=-1),
          dict(OK_KW, ridge_log2=9), dict(OK_KW, ridge_log2=41), dict(OK_KW, forget_shift=9), dict(OK_KW, forget_shift=True), dict(OK_KW, gain=INF),
          dict(OK_KW, output_format="sc8"), dict(OK_KW, output_format=2)]


@pytest.mark.parametrize("kw", PY_BAD, ids=[str(i) for i in range(len(PY_BAD))])
def test_python_class_raises_value_error_without_a_device(product, kw):
    with pytest.raises(ValueError):
        product.mpd(**kw)
    with pytest.raises(ValueError):
        product.mpd_config(**kw)


@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitizers"])
def test_host_program_of_the_plan(product, san):
    """host/mpd_plan_test.cc: csrc/mpd_plan.hpp with a main of its own (no GPU, no Python), plain and under the address and
    undefined-behaviour sanitizers"""
    host = os.path.join(ROOT, "liquid-usrp_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "mpd_plan_test"] + (["SAN=1"] if san else []))
    out = subprocess.run([os.path.join(ROOT, "liquid-usrp_amd", "lib", "mpd_plan_test" + ("_san" if san else ""))], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT)
    assert out.returncode == 0 and b"mpd_plan_test ok" in out.stdout, out.stdout.decode()


# ---------------------------------------------------------------------------------------------- the host arithmetic against the model
@pytest.mark.parametrize("log2,fs,g0", [(5, 1.0, 1.0), (7, 0.75, 2.0), (9, 0.3, 3.0), (7, 0.5, 0.7), (7, 0.50000006, 1e-3), (6, 2.0000002, 1e3),
                                        (7, 1e-3, 1.0), (5, 3e38, 3e38), (9, 1e-30, 1e-30)])
def test_constants_equal_the_model(product, log2, fs, g0):
    c = product.mpd_config(3, (0, 1, 2), 5, log2, fs, g0)
    inv_step, step, e, inv_g0 = product.mpd_constants(c)
    K, m_inv, m_step, m_e, m_g = model.constants(log2, fs, g0)
    assert (inv_step, step, e, inv_g0) == (float(m_inv), m_step, m_e, float(m_g))
    d = product.dpd_constants(product.dpd_config(log2, fs, g0))
    assert (inv_step, step, e) == d                                                        # made exactly as dpd's
    assert inv_g0 == float(np.float32(1.0 / float(np.float32(g0))))


def edge_samples(fs, g0, seed):
    """(u, z): feedback amplitudes at, one ulp below and one ulp above g0 E (the edge of `good`), targets likewise around 2 E, values
    whose integers sit on ties, random samples around both edges, and one sample of every bad kind"""
    rng = np.random.RandomState(seed)
    e = model.constants(7, fs, g0)[3]
    E = 2.0 ** e
    up, dn = np.float32(np.inf), np.float32(0)
    zedge, uedge = np.float32(float(np.float32(g0)) * E), np.float32(2.0 * E)
    za = np.array([0.0, zedge, np.nextafter(zedge, dn), np.nextafter(zedge, up), 0.5 * zedge], np.float32)
    ua = np.array([0.0, uedge, np.nextafter(uedge, dn), np.nextafter(uedge, up), 0.5 * uedge], np.float32)
    ties = (np.arange(1, 40) + 0.5) * 2.0 ** -17 * E
    n = 4000
    z = np.concatenate([za, -za, 1j * za, ties * float(np.float32(g0)), rng.uniform(0, 1.2, n) * zedge * np.exp(2j * np.pi * rng.uniform(0, 1, n))])
    u = np.concatenate([ua, -ua, 1j * ua, ties, rng.uniform(0, 1.2, n) * uedge * np.exp(2j * np.pi * rng.uniform(0, 1, n))])
    odd = np.array([NAN, complex(0, NAN), INF, complex(0, -INF), 3e38, complex(3e38, 3e38), complex(-0.0, 0.0)], np.complex64)
    return np.concatenate([u, odd]).astype(np.complex64), np.concatenate([z, odd]).astype(np.complex64)


@pytest.mark.parametrize("P,fs,g0", [(5, 1.0, 1.0), (3, 0.75, 2.0), (1, 0.3, 0.7), (5, 0.0123, 3.0), (4, 7.5, 1.0)])
def test_selftest_integers_equal_the_model(product, P, fs, g0):
    c = product.mpd_config(2, (0, 3), P, 7, fs, g0)
    u, z = edge_samples(fs, g0, seed=P)
    Z, U, good = product.mpd_integers(c, u, z)
    _, _, _, e, inv_g0 = model.constants(7, fs, g0)
    Zm, zg = model.regressors(z, inv_g0, e, P)
    Um, ug = model.targets(u, e)
    assert np.array_equal(Z, Zm), np.nonzero((Z != Zm).any(axis=(1, 2)))[0][:10]
    assert np.array_equal(U, Um), np.nonzero((U != Um).any(axis=1))[0][:10]
    assert np.array_equal(good, zg.astype(np.int32) + 2 * ug.astype(np.int32))
    assert list(good[-7:]) == [0, 0, 0, 0, 0, 0, 3]                                        # NaN, infinity, overflow; -0.0 is good
    assert 0.5 < zg.mean() < 1 and 0.5 < ug.mean() < 1 and np.abs(Z).max() <= 2 ** 17 + 1 and np.abs(U).max() <= 2 ** 18 + 1
    assert not Z[~zg].any() and not U[~ug].any()
    if g0 == 1.0 and fs == 1.0:                                                            # every product exact: the edges as written
        assert list(good[:5] & 1) == [1, 1, 1, 0, 1] and list(good[:5] >> 1) == [1, 1, 1, 0, 1]
        assert Z[1, :, 0].tolist() == [2 ** 17] * P and Z[4, :, 0].tolist() == [2 ** 16 >> k for k in range(P)]
        assert U[1].tolist() == [2 ** 18, 0] and U[11].tolist() == [0, 2 ** 18]
        ties = slice(15, 15 + 39)
        assert U[ties, 0].tolist() == [k + 1 if k % 2 else k for k in range(1, 40)]         # k + 1/2 goes to the even neighbour
    for k in range(1, P):                                                                  # no power is larger than the one before it
        assert (np.abs(Z[:, k]) <= np.abs(Z[:, k - 1])).all()


def test_the_model_sums_are_exact():
    """model.gram against Python integers; model.rows_of drops a row for each bad sample it touches; the layout of model.sums"""
    rng = np.random.RandomState(9)
    n, delays, P = 3000, (0, 2, 5), 3
    z = (0.4 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    u = (0.8 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    z[100], u[200] = NAN, INF
    Vr, Vi, skipped = model.rows_of(u, z, delays, P, np.float32(1.0), 0)
    _, zg = model.regressors(z, np.float32(1.0), 0, P)
    _, ug = model.targets(u, 0)
    bad = set(np.nonzero(~ug)[0])
    for j in np.nonzero(~zg)[0]:
        bad |= {j + d for d in delays}
    bad = {i for i in bad if 5 <= i < n}
    assert {100, 102, 105, 200} <= bad and skipped == len(bad) and len(Vr) == n - 5 - skipped
    Sre, Sim = model.gram(Vr, Vi)
    W = Vr.shape[1]
    for p, q in ((0, 0), (0, W - 1), (3, 7), (W - 1, W - 1), (8, 2)):
        re = sum(int(a) * int(c) + int(b) * int(d) for a, b, c, d in zip(Vr[:, p], Vi[:, p], Vr[:, q], Vi[:, q]))
        im = sum(int(a) * int(d) - int(b) * int(c) for a, b, c, d in zip(Vr[:, p], Vi[:, p], Vr[:, q], Vi[:, q]))
        assert (int(Sre[p, q]), int(Sim[p, q])) == (re, im)
    assert not np.diag(Sim).any()
    m = model.Model(3, delays, P, 7, 1.0, 1.0)
    assert m.measure(u, z) and m.rows == len(Vr) and m.skipped == skipped and m.since == n - 5
    s = m.sums()
    assert s.shape == ((W + 1) * W // 2, 2) and tuple(s[0]) == (Sre[0, 0], 0) and tuple(s[W - 1]) == (Sre[0, W - 1], Sim[0, W - 1])
    assert tuple(s[W]) == (Sre[1, 1], 0) and tuple(s[-1]) == (Sre[W - 1, W - 1], 0)
    assert m.measure(u[:5], z[:5]) and m.measure(u[:3], z[:3]) and m.since == n - 5        # n <= lead: nothing measured


def test_the_guard_and_degenerate_updates():
    m = model.Model(2, (0, 1), 2, 5, 1.0, 1.0, min_rows=4, forget_shift=2)
    u = np.full(6, 0.5, np.complex64)
    assert m.measure(u, u) and m.since == 5 and m.rows == 5
    before = m.Sre.copy()
    m.update()                                                  # z = u in every row: the Gram matrix is singular but for the ridge
    assert m.since == 2 and m.rows == 1 and m.updates == 1 and np.array_equal(m.Sre, before >> 2)
    m.since = (1 << 26) - 4
    assert not m.measure(u, u) and m.since == (1 << 26) - 4 and m.rows == 1
    assert m.measure(u[:5], u[:5]) and m.since == 1 << 26
    empty = model.Model(2, (0, 1), 2, 5, 1.0, 1.0, min_rows=4)
    empty.update()
    assert empty.degenerate == 1 and empty.updates == 1 and np.all(empty.F[0] == 1) and not empty.F[1].any() and empty.trained
    zero = model.Model(2, (0, 1), 2, 5, 1.0, 1.0, min_rows=4)
    zero.measure(np.zeros(100, np.complex64), np.zeros(100, np.complex64))
    zero.update()                                               # an all-zero record: the first pivot is not positive
    assert zero.rows == 99 and zero.degenerate == 1 and np.all(zero.F[0] == 1)


def test_the_update_of_a_linear_filter_is_its_inverse():
    """u = h0 z + h1 z[i-1] exactly: the least squares solution is c = (h0, 0 ..., h1, 0 ...), the tables are constant, res is rounding"""
    rng = np.random.RandomState(3)
    n = 6000
    z = (0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    h0, h1 = 0.9 * np.exp(0.2j), 0.1 * np.exp(-1.0j)
    u = (h0 * z.astype(np.complex128) + h1 * np.concatenate([[0], z[:-1]]).astype(np.complex128)).astype(np.complex64)
    m = model.Model(2, (0, 1), 3, 6, 1.0, 1.0)
    assert m.measure(u, z)
    m.update()
    assert m.degenerate == 0 and m.updates == 1
    c = m.coefficients()
    assert abs(c[0, 0] - h0) < 1e-3 and abs(c[1, 0] - h1) < 1e-3 and np.abs(m.F[0] - h0).max() < 2e-3 and np.abs(m.F[1] - h1).max() < 2e-3
    assert 0 <= m.res < 1e-4 * int(m.Sre[-1, -1]) * 4                                      # (before the shift of 0)
    x = np.concatenate([[0], z[:500]]).astype(np.complex64)
    y, bound = model.apply(m.F, x, m.delays, 6, 1.0)
    assert np.abs(y - u[:500]).max() < 2e-3 and bound.max() < 1e-6


# ---------------------------------------------------------------------------------------------- the end-to-end case on the oracle alone
@functools.lru_cache(maxsize=None)
def severity_case(product, oracle):
    """(x, sent, configs, full_scale, papr0): cfr_model.SEVERITY's stream behind its stage, the three amplifier configurations, the
    tables' end"""
    s, d = cfr_model.SEVERITY, model.SEVERITY
    iq, sent = oracle.synth_traffic(s["N"], s["M"], s["cp"], s["taper"], s["frames"], payload_len=s["payload_len"])
    rms = cfr_model.rms(iq)
    h = product.cfr_lowpass(s["half_len"], s["cutoff"], s["beta"])
    A = float(np.float32(product.cfr_threshold(s["papr_db"], rms)))
    x = cfr_model.apply_stream(iq, A, h, s["passes"]).astype(np.complex64)
    cfgs = [product.rfchain_config(amplifier=dict(sat=product.rfchain_backoff(ibo, rms), smooth=d["amp_smooth"], gain=d["amp_gain"], ampm_deg=deg))
            for ibo, deg in zip(d["amp_ibo_db"], d["amp_ampm_deg"])]
    return x, sent, cfgs, float(np.float32(d["full_scale_over_peak"] * np.abs(x).max())), cfr_model.papr_db(iq)


def test_severity_on_the_oracle_alone(product, oracle):
    """The oracle's transmitter, cfr's model, then the three-branch amplifier of mpd_model.SEVERITY made of rfchain's amplifier model:
    three rounds of the exact dpd model and three of the exact mpd model on it.  Asserted: the two NMSE figures are the ones recorded
    in mpd_model.SEVERITY (which is what tests/test_gpu_mpd.py's threshold is made of), their difference is at least 15 dB, the power
    at |f| > 0.32 behind mpd is not worse than behind dpd by more than 1 dB, every frame valid with its bytes as sent behind mpd."""
    s, d = cfr_model.SEVERITY, model.SEVERITY
    x, sent, cfgs, full_scale, papr0 = severity_case(product, oracle)
    g0 = d["amp_gain"]
    ref = g0 * x.astype(np.complex128)

    def amp(u):
        return model.memory_amplifier(cfgs, d["amp_weights"], np.asarray(u).astype(np.complex64))

    y0 = amp(x)
    md = dpd_model.Model(d["table_log2"], full_scale, g0)
    for _ in range(d["rounds"]):
        u = md.execute(x).astype(np.complex64)
        assert md.measure(u, amp(u).astype(np.complex64))
        md.update()
    yd = amp(md.execute(x))
    mm = model.Model(d["branches"], d["delays"], d["order"], d["table_log2"], full_scale, g0)
    xp = np.concatenate([np.zeros(mm.lead, np.complex64), x])
    for _ in range(d["rounds"]):
        u = mm.execute(xp).astype(np.complex64)
        assert mm.measure(u, amp(u).astype(np.complex64))
        mm.update()
    ym = amp(mm.execute(xp))
    evm = decode(oracle, s, sent, ym)
    rows = [(name, cfr_model.oob_db(y, d["edge"]), model.nmse_db(y, ref)) for name, y in (("none", y0), ("dpd", yd), ("mpd", ym))]
    print("mpd severity: %d samples, PAPR %.1f -> %.1f dB, full_scale %.4f; rows %d, skipped %d, res / Suu %.3e"
          % (len(x), papr0, cfr_model.papr_db(x), full_scale, mm.rows, mm.skipped, mm.res / float(mm.Sre[-1, -1])))
    for name, oob, nmse in rows:
        print("mpd severity, predistorter %-4s: power at |f| > %.2f %.2f dB, NMSE %.2f dB" % (name, d["edge"], oob, nmse))
    print("mpd severity: oracle EVM behind mpd %.1f .. %.1f dB; NMSE gain of mpd over dpd %.2f dB" % (min(evm), max(evm), rows[1][2] - rows[2][2]))
    assert mm.degenerate == 0 and mm.updates == d["rounds"] and mm.skipped == 0 and md.degenerate == 0
    assert abs(rows[1][2] - d["model_nmse_db"][0]) <= 0.05 and abs(rows[2][2] - d["model_nmse_db"][1]) <= 0.05
    assert d["model_nmse_db"][0] - d["model_nmse_db"][1] >= 15.0
    assert abs(d["nmse_gain_db"] - (d["model_nmse_db"][0] - d["model_nmse_db"][1] - 6.0)) < 1e-9
    assert rows[2][1] <= rows[1][1] + d["oob_slack_db"]
