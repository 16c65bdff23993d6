"""Feedback alignment for the predistorters (mcrx_hip_fbalign_*), what needs no GPU: the boundary -- symbols, null handles, every
configuration error reported before a device is looked for --, the library's host arithmetic (constants, the quantiser, the
coefficients of a delay) against tests/fbalign_model.py, the guard and the degenerate updates on the model, the host program of the plan
plain and under the sanitizers, linear paths found by the model, and the severity study of tests/test_gpu_fbalign.py's closed loops on
the oracle alone with the exact models."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cfr_model
import dpd_model
import fbalign_model as model
import mpd_model
import rfchain_model
import userclock_model
from test_dpd import decode
from test_mpd import severity_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mcrx_hip_fbalign_create", "mcrx_hip_fbalign_destroy", "mcrx_hip_fbalign_execute_device", "mcrx_hip_fbalign_halo",
           "mcrx_hip_fbalign_input_format", "mcrx_hip_fbalign_last_error", "mcrx_hip_fbalign_measure_device", "mcrx_hip_fbalign_read",
           "mcrx_hip_fbalign_reset", "mcrx_hip_fbalign_selftest", "mcrx_hip_fbalign_set", "mcrx_hip_fbalign_update"]
NAN, INF = float("nan"), float("inf")


def library_table(product):
    W = np.zeros((userclock_model.PHASES + 1, userclock_model.TAPS), np.float32)
    assert product.lib().mcrx_hip_userclock_table(W.ctypes.data_as(C.POINTER(C.c_float))) == product.MCRX_OK
    return W


# ---------------------------------------------------------------------------------------------- the boundary
def test_symbols_are_declared_exported_and_bound(product):
    text = open(os.path.join(ROOT, "include", "mcrx_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(mcrx_hip_fbalign_[a-z_0-9]+)\s*\(", text))) == SYMBOLS
    assert [s for s in product.exported_symbols() if s.startswith("mcrx_hip_fbalign_")] == SYMBOLS
    L = product.lib()
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", product.build()]).decode()
    assert sorted(set(re.findall(r" T (mcrx_hip_fbalign_[a-z_0-9]+)", out))) == SYMBOLS
    assert C.sizeof(product.FbalignConfig) == 6 * 4 and C.sizeof(product.FbalignState) == 9 * 8
    assert (product.FBALIGN_MIN_LAG, product.FBALIGN_MAX_LAG, product.FBALIGN_H, product.FBALIGN_TAPS, product.FBALIGN_GUARD_LOG2) == \
        (model.MIN_LAG, model.MAX_LAG, model.H, model.TAPS, model.GUARD_LOG2)
    for name in ("execute", "measure", "update", "set", "read", "reset", "align"):
        assert callable(getattr(product.fbalign, name))
    import inspect
    assert inspect.signature(product._Predistorter.learn).parameters["aligner"].default is None


def good_config(product):
    return product.fbalign_config(16, 0.75, 2.0, min_rows=64, input_format="sc16")


def test_null_handles_are_answered(product):
    L = product.lib()
    assert L.mcrx_hip_fbalign_halo(None) == 0 and L.mcrx_hip_fbalign_input_format(None) == 0
    assert L.mcrx_hip_fbalign_destroy(None) == product.MCRX_OK
    st = product.FbalignState()
    for rc in (L.mcrx_hip_fbalign_execute_device(None, None, 0, None, None), L.mcrx_hip_fbalign_measure_device(None, None, None, 0, None),
               L.mcrx_hip_fbalign_update(None, None), L.mcrx_hip_fbalign_set(None, 0, 1.0, 0.0, None),
               L.mcrx_hip_fbalign_read(None, C.addressof(st), None, None, None), L.mcrx_hip_fbalign_reset(None), L.mcrx_hip_fbalign_create(None, None),
               L.mcrx_hip_fbalign_selftest(None, None, None, None, 0, None, None, 0, None, None)):
        assert rc == product.MCRX_EINVAL
    assert L.mcrx_hip_fbalign_last_error()
    h = C.c_void_p(0x1234)
    assert L.mcrx_hip_fbalign_create(C.byref(h), None) == product.MCRX_EINVAL and not h.value
    c = good_config(product)
    assert L.mcrx_hip_fbalign_selftest(C.addressof(c), None, None, None, 3, None, None, 0, None, None) == product.MCRX_EINVAL


BAD = [("struct_size", "struct_size", 20), ("max_lag 7", "max_lag", 7), ("max_lag 65", "max_lag", 65), ("full_scale 0", "full_scale", 0.0),
       ("full_scale negative", "full_scale", -0.5), ("full_scale nan", "full_scale", NAN), ("full_scale inf", "full_scale", INF),
       ("target_gain 0", "target_gain", 0.0), ("target_gain negative", "target_gain", -1.0), ("target_gain nan", "target_gain", NAN),
       ("target_gain inf", "target_gain", INF), ("min_rows 0", "min_rows", 0), ("input format", "input_format", 2)]


@pytest.mark.parametrize("what,field,value", BAD, ids=[b[0] for b in BAD])
def test_configuration_errors_come_before_the_device(product, what, field, value):
    L = product.lib()
    c = good_config(product)
    setattr(c, field, value)
    h = C.c_void_p(0x1234)
    assert L.mcrx_hip_fbalign_create(C.byref(h), C.addressof(c)) == product.MCRX_EINVAL, what
    assert not h.value                                                                     # *out is cleared
    assert L.mcrx_hip_fbalign_last_error()
    assert L.mcrx_hip_fbalign_selftest(C.addressof(c), None, None, None, 0, None, None, 0, None, None) == product.MCRX_EINVAL, what


def test_the_limits_themselves_are_accepted(product):
    """on the allowed side of every bound the answer is a handle, or 'no device' here -- never MCRX_EINVAL"""
    L = product.lib()
    for field, value in [("max_lag", 8), ("max_lag", 64), ("full_scale", 1e-30), ("full_scale", 3e38), ("target_gain", 1e-30), ("target_gain", 3e38),
                         ("min_rows", 1), ("min_rows", 0xffffffff), ("input_format", 0), ("input_format", 1)]:
        c = good_config(product)
        setattr(c, field, value)
        h = C.c_void_p()
        rc = L.mcrx_hip_fbalign_create(C.byref(h), C.addressof(c))
        assert rc in (product.MCRX_OK, product.MCRX_EHIP), (field, L.mcrx_hip_fbalign_last_error())
        if rc == product.MCRX_OK:
            assert L.mcrx_hip_fbalign_input_format(h) == c.input_format and L.mcrx_hip_fbalign_halo(h) == c.max_lag + 17
            L.mcrx_hip_fbalign_destroy(h)


OK_KW = dict(max_lag=16, full_scale=1.0, target_gain=1.0)
PY_BAD = [dict(), dict(max_lag=16, full_scale=1.0), dict(max_lag=16, target_gain=1.0), dict(OK_KW, max_lag=7), dict(OK_KW, max_lag=65),
          dict(OK_KW, max_lag=16.5), dict(OK_KW, max_lag=-8), dict(OK_KW, full_scale=0.0), dict(OK_KW, full_scale=NAN), dict(OK_KW, full_scale=INF),
          dict(OK_KW, target_gain=0.0), dict(OK_KW, target_gain=NAN), dict(OK_KW, min_rows=0), dict(OK_KW, min_rows=-1), dict(OK_KW, min_rows=True),
          dict(OK_KW, input_format="sc8"), dict(OK_KW, input_format=2)]


@pytest.mark.parametrize("kw", PY_BAD, ids=[str(i) for i in range(len(PY_BAD))])
def test_python_class_raises_value_error_without_a_device(product, kw):
    with pytest.raises(ValueError):
        product.fbalign(**kw)
    with pytest.raises(ValueError):
        product.fbalign_config(**kw)


@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitizers"])
def test_host_program_of_the_plan(product, san):
    """host/fbalign_plan_test.cc: csrc/fbalign_plan.hpp with a main of its own (no GPU, no Python), plain and under the address and
    undefined-behaviour sanitizers"""
    host = os.path.join(ROOT, "liquid-usrp_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "fbalign_plan_test"] + (["SAN=1"] if san else []))
    out = subprocess.run([os.path.join(ROOT, "liquid-usrp_amd", "lib", "fbalign_plan_test" + ("_san" if san else ""))], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT)
    assert out.returncode == 0 and b"fbalign_plan_test ok" in out.stdout, out.stdout.decode()


# ---------------------------------------------------------------------------------------------- the host arithmetic against the model
@pytest.mark.parametrize("fs", [1.0, 0.75, 0.3, 0.50000006, 2.0000002, 1e-3, 3e38, 1e-30])
def test_constants_equal_the_model(product, fs):
    c = product.fbalign_config(64, fs, 1.0)
    e, taps = product.fbalign_constants(c)
    assert e == model.constants(64, fs)[0] == product.dpd_constants(product.dpd_config(7, fs, 1.0))[2]      # made exactly as dpd's
    assert np.array_equal(taps, model.taps_f32()) and taps.dtype == np.float32
    assert taps[0] < 0 < taps[1] and abs(float(taps[0]) + 0.54 + 0.46 * np.cos(np.pi / 9)) < 1e-7


@pytest.mark.parametrize("fs", [1.0, 0.75, 0.0123, 7.5])
def test_selftest_integers_equal_the_model(product, fs):
    """the quantiser at its clamps, one ulp to either side of them, on ties, on random values and on every bad kind"""
    rng = np.random.RandomState(5)
    c = product.fbalign_config(16, fs, 1.0)
    e = model.constants(16, fs)[0]
    E = np.float32(2.0 ** e)
    up, dn = np.float32(np.inf), np.float32(-np.inf)
    edges = [E * np.float32(v) for v in (32767.0 / 32768.0, 32767.5 / 32768.0, 32767.49 / 32768.0, -1.0, -32768.5 / 32768.0, -32768.51 / 32768.0, 1.0)]
    edges = np.array([f(v) for v in edges for f in (lambda t: t, lambda t: np.nextafter(t, up), lambda t: np.nextafter(t, dn))], np.float32)
    ties = ((np.arange(-40, 40) + 0.5) * 2.0 ** -15 * float(E)).astype(np.float32)
    odd = np.array([NAN, INF, -INF, 3e38, -3e38, -0.0, 0.0, 1e-45], np.float32)
    v = np.concatenate([edges, ties, (rng.uniform(-1.2, 1.2, 4000) * float(E)).astype(np.float32), odd])
    q, bad = product.fbalign_q15(c, v)
    qm, bm = model.q15(v, e)
    assert np.array_equal(q, qm) and np.array_equal(bad.astype(bool), bm)
    assert list(q[-8:]) == [0, 32767, -32768, 32767, -32768, 0, 0, 0] and list(bad[-8:]) == [1, 1, 1, 1, 1, 0, 0, 0]
    assert q.min() == -32768 and q.max() == 32767 and 0.05 < bad.mean() < 0.3
    k = len(edges)
    assert q[k:k + 80].tolist() == [2 * int(np.floor((t + 1) / 2.0)) for t in range(-40, 40)]      # t + 1/2 goes to the even neighbour
    assert (q[0], bad[0]) == (32767, 0) and (q[3], bad[3]) == (32767, 1) and (q[9], bad[9]) == (-32768, 0) and (q[18], bad[18]) == (32767, 1)


def test_coefficients_equal_the_model(product):
    """every table row, fractions between them, both ends of the range and the whole samples: coefficients and nd, bit for bit"""
    W = library_table(product)
    assert np.array_equal(W, userclock_model.table_f64().astype(np.float32)) or np.abs(W - userclock_model.table_f64()).max() < 1e-7
    rng = np.random.RandomState(2)
    for Lm in (8, 64):
        c = product.fbalign_config(Lm, 1.0, 1.0)
        most = (Lm + 1) << 32
        taus = [0, 1, -1, 3, -3, 4, -4, most, -most, most - 1, -most + 1, (7 << 32) + (1 << 31), -(5 << 32)] + [r << 26 for r in range(0, 64, 7)] \
            + [int(t) for t in rng.randint(-most, most, 40)]
        for tau in taus:
            co, nd = product.fbalign_coefficients(c, tau)
            cm, ndm = model.coefs(W, tau)
            assert nd == ndm and np.array_equal(co, cm), tau
            d = -tau
            assert nd == d >> 32 and -(Lm + 1) <= nd <= Lm + 1
            if d & 0xFFFFFFFF == 0:
                assert co.tolist() == [1.0 if j == 15 else 0.0 for j in range(32)]
        for tau in (most + 1, -most - 1, 1 << 62):
            with pytest.raises(ValueError):
                product.fbalign_coefficients(c, tau)


# ---------------------------------------------------------------------------------------------- the model on its own
def band_limited(n, occupied, seed, rms=0.1):
    rng = np.random.RandomState(seed)
    X = np.zeros(n, np.complex128)
    k = int(0.5 * occupied * n)
    idx = np.r_[0:k, n - k:n]
    X[idx] = rng.standard_normal(len(idx)) + 1j * rng.standard_normal(len(idx))
    x = np.fft.ifft(X)
    return (rms * x / cfr_model.rms(x)).astype(np.complex64)


def test_the_model_sums_are_exact():
    """model.sums against Python integers on a few lags; the rows; clamped counts row samples only"""
    rng = np.random.RandomState(9)
    n, R = 700, 16
    u = (0.4 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    z = (0.4 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    u[3], z[5], u[100], z[200], z[n - 2] = 7.0, NAN, NAN, complex(INF, 0), -9.0
    Cm, Am, Szz, rows, clamped = model.sums(u, z, R, 0)
    ur, ui, ub = model.quantise(u, 0)
    zr, zi, zb = model.quantise(z, 0)
    assert rows == n - 2 * R and clamped == int(ub[R:n - R].sum() + zb[R:n - R].sum()) and ub[3] and zb[5] and ub[100] and zb[200]
    assert (ur[100], ui[100]) == (0, 0) and zr[200] == 32767 and clamped >= 2
    for l in (-R, -1, 0, 5, R):
        re = sum(int(ur[i]) * int(zr[i + l]) + int(ui[i]) * int(zi[i + l]) for i in range(R, n - R))
        im = sum(int(ur[i]) * int(zi[i + l]) - int(ui[i]) * int(zr[i + l]) for i in range(R, n - R))
        assert (int(Cm[l + R, 0]), int(Cm[l + R, 1])) == (re, im)
    for l in (0, 1, 16):
        re = sum(int(ur[i]) * int(ur[i + l]) + int(ui[i]) * int(ui[i + l]) for i in range(R, n - R))
        im = sum(int(ur[i]) * int(ui[i + l]) - int(ui[i]) * int(ur[i + l]) for i in range(R, n - R))
        assert (int(Am[l, 0]), int(Am[l, 1])) == (re, im)
    assert Am[0, 1] == 0 and Szz == sum(int(zr[i]) ** 2 + int(zi[i]) ** 2 for i in range(R, n - R))
    assert model.sums(u[:2 * R], z[:2 * R], R, 0)[3] == 0 and model.sums(u[:2 * R + 1], z[:2 * R + 1], R, 0)[3] == 1


def test_the_guard_and_degenerate_updates():
    x = band_limited(400, 0.5, 1)
    m = model.Model(8, 1.0, 1.0, min_rows=100)
    assert (m.R, m.halo, m.tau_fp, m.s) == (16, 25, 0, (1.0, 0.0)) and not m.trained
    assert m.measure(x, x) and m.since == m.rows == 400 - 32
    m.since = (1 << 31) - 367
    assert not m.measure(x, x) and m.rows == 368 and m.since == (1 << 31) - 367           # refused: nothing measured
    assert m.measure(x[:399], x[:399]) and m.since == 1 << 31
    m.update()                                                  # u = zh: D = 0, delta = 0, alpha = 1
    assert m.degenerate == 0 and m.updates == 1 and m.since == 0 and m.rows == 0 and not m.C.any() and not m.A.any() and m.Szz == 0
    assert abs(m.tau) < 0.05 and abs(complex(*m.s) - 1.0) < 0.05 and m.trained         # (368 rows: the ends of the record weigh 1 %)
    few = model.Model(8, 1.0, 1.0, min_rows=369)
    few.measure(x, x)
    few.update()                                                # rows < min_rows
    assert (few.degenerate, few.updates, few.tau_fp, few.s, few.rows) == (1, 1, 0, (1.0, 0.0), 0) and few.trained
    empty = model.Model(8, 1.0, 1.0, min_rows=1)
    empty.update()
    assert empty.degenerate == 1
    zero = model.Model(8, 1.0, 1.0, min_rows=1)
    zero.measure(x, np.zeros(400, np.complex64))
    zero.update()                                               # every C[l] = 0: the greatest value is 0
    assert zero.degenerate == 1 and zero.tau_fp == 0
    const = model.Model(8, 1.0, 1.0, min_rows=1)
    one = np.full(400, 0.25, np.complex64)
    const.measure(one, one)
    const.update()                                              # a constant has no derivative: det = 0
    assert const.degenerate == 1 and const.s == (1.0, 0.0)
    far = model.Model(8, 1.0, 1.0, min_rows=1)
    far.set(-(8 << 32) - (1 << 31))
    far.measure(x[:-8], x[8:])                                  # eight more samples early: the new delay would leave +-(Lm + 1)
    far.update()
    assert far.degenerate == 1 and far.tau_fp == -(8 << 32) - (1 << 31)
    far.measure(x[8:], x[:-8])
    far.update()
    assert far.degenerate == 1 and far.updates == 2 and abs(far.tau + 0.5) < 0.05


LINEAR_TAU_TOL = 5e-5       # measured below: the worst |tau - true| after three updates is 1.9e-5 samples (Lm = 64); the tolerance is 2.6 times that


@pytest.mark.parametrize("Lm", [16, 64])
def test_a_linear_path_is_found(product, Lm):
    """no amplifier, no noise: delays 0, 0.5, 7.37, -12.5 and +-(Lm - 0.51) at gains of any phase are found within LINEAR_TAU_TOL samples
    in three updates from tau = 0, the scale within 1e-4 of g0 / gain"""
    W = library_table(product)
    n = 20000
    x = band_limited(n, 0.56, 1)
    worst = 0.0
    for k, tau in enumerate((0.0, 0.5, 7.37, -12.5, Lm - 0.51, -(Lm - 0.51))):
        gain = (0.3 + 0.5 * k) * np.exp(1.1j * (k + 1))
        z = model.path(x, tau, gain).astype(np.complex64)
        m = model.Model(Lm, 0.75, 2.0, W32=W)
        ut, zh = m.align(x, z, 3)
        err = abs(m.tau - tau)
        worst = max(worst, err)
        print("fbalign linear path: Lm %d tau %+.2f gain %.2f e^{%.1fj}: found %+.7f (error %.2e), s %s, D and delta of the last step %s"
              % (Lm, tau, abs(gain), np.angle(gain), m.tau, err, complex(*m.s), m.last))
        assert m.degenerate == 0 and m.updates == 3 and err <= LINEAR_TAU_TOL
        assert abs(complex(*m.s) * gain / 2.0 - 1.0) < 1e-4
        assert dpd_model.nmse_db(zh, 2.0 * ut.astype(np.complex128)) < -60.0
    print("fbalign linear path: worst error %.2e samples at Lm = %d" % (worst, Lm))


# ---------------------------------------------------------------------------------------------- the severity study on the oracle alone
def feedback(z, mode, v, aligner, u, seed):
    """(u', z') for a predistorter's measure: the amplifier's output z as it is (`direct`), through the path and the aligner
    (`aligned`), or through the path, moved back by the whole samples and divided by the gain (`whole`)"""
    if mode == "direct":
        return u, z.astype(np.complex64)
    nstd = cfr_model.rms(z) * abs(v["gain"]) * 10.0 ** (-v["snr_db"] / 20.0) / np.sqrt(2.0)
    cap = model.path(z, v["tau"], v["gain"], nstd, seed=seed).astype(np.complex64)
    if mode == "whole":
        return u, (np.roll(cap, -int(round(v["tau"]))) / v["gain"]).astype(np.complex64)
    ut, zh = aligner.align(u, cap, v["align_rounds"])
    return ut, zh.astype(np.complex64)


def severity_study(product, oracle):
    """{(predistorter, feedback): (power at |f| > edge in dB, NMSE after delay and gain removal in dB, tau, EVMs)}"""
    s, d, dd, v = cfr_model.SEVERITY, mpd_model.SEVERITY, dpd_model.SEVERITY, model.SEVERITY
    x, sent, cfgs, full_scale, _ = severity_case(product, oracle)
    iq, _ = oracle.synth_traffic(s["N"], s["M"], s["cp"], s["taper"], s["frames"], payload_len=s["payload_len"])
    one = product.rfchain_config(amplifier=dict(sat=product.rfchain_backoff(dd["amp_ibo_db"], cfr_model.rms(iq)), smooth=dd["amp_smooth"],
                                                gain=dd["amp_gain"], ampm_deg=dd["amp_ampm_deg"]))
    g0 = d["amp_gain"]
    ref = g0 * x.astype(np.complex128)
    W = library_table(product)
    amps = dict(dpd=lambda u: rfchain_model.amplifier(one, np.asarray(u).astype(np.complex64).astype(np.complex128)),
                mpd=lambda u: mpd_model.memory_amplifier(cfgs, d["amp_weights"], np.asarray(u).astype(np.complex64)))
    out = {}
    for kind in ("dpd", "mpd"):
        for mode in ("direct", "aligned", "whole"):
            if kind == "dpd":
                pd, xp = dpd_model.Model(dd["table_log2"], full_scale, g0), x
            else:
                pd = mpd_model.Model(d["branches"], d["delays"], d["order"], d["table_log2"], full_scale, g0)
                xp = np.concatenate([np.zeros(pd.lead, np.complex64), x])
            al = model.Model(v["max_lag"], full_scale * g0, g0, v["min_rows"], W32=W)
            for r in range(v["rounds"]):
                u = pd.execute(xp).astype(np.complex64)
                assert pd.measure(*feedback(amps[kind](u), mode, v, al, u, r))
                pd.update()
            y = amps[kind](pd.execute(xp))
            evm = decode(oracle, s, sent, y)                    # every frame valid with its bytes as sent
            assert pd.degenerate == 0 and al.degenerate == 0
            out[kind, mode] = (cfr_model.oob_db(y, v["edge"]), model.nmse_aligned_db(y, ref), al.tau, (min(evm), max(evm)))
            print("fbalign severity: %s, %-7s feedback: power at |f| > %.2f %.2f dB, NMSE after delay and gain removal %.2f dB, tau %.7f, oracle EVM %.1f .. %.1f dB"
                  % ((kind, mode, v["edge"]) + out[kind, mode][:3] + out[kind, mode][3]))
    return out


def test_severity_on_the_oracle_alone(product, oracle):
    """The oracle's transmitter, cfr's model, dpd's model on dpd_model.SEVERITY's amplifier and mpd's model on mpd_model.SEVERITY's
    three-branch amplifier, three rounds each; the feedback direct, through a path of 7.37 samples, 0.6 e^{1.1j} and 50 dB SNR with the
    aligner's model (three alignments a round), and with whole-sample alignment and exact gain removal only.  Asserted: the figures are
    the ones recorded in fbalign_model.SEVERITY (which is what tests/test_gpu_fbalign.py's thresholds are made of); the power at
    |f| > 0.32 through the aligner is at least 15 dB better than with whole-sample alignment; it is within the recorded margin (the
    measured difference plus 1 dB) of direct feedback; on the memoryless amplifier tau is within tau_tol of the true delay; every
    frame of every case is valid with its bytes as sent (severity_study)."""
    v = model.SEVERITY
    got = severity_study(product, oracle)
    for kind in ("dpd", "mpd"):
        rec = v[kind]
        for mode in ("direct", "aligned", "whole"):
            oob, nmse, tau, _ = got[kind, mode]
            assert abs(oob - rec["oob_db"][mode]) <= 0.05 and abs(nmse - rec["nmse_db"][mode]) <= 0.05, (kind, mode, oob, nmse)
        assert abs(got[kind, "aligned"][2] - rec["tau"]) <= 1e-5
        assert rec["oob_db"]["whole"] - rec["oob_db"]["aligned"] >= v["oob_gain_db"]
        assert got[kind, "whole"][0] - got[kind, "aligned"][0] >= v["oob_gain_db"]
        assert abs(rec["oob_margin_db"] - (max(rec["oob_db"]["aligned"] - rec["oob_db"]["direct"], 0.0) + 1.0)) < 1e-9
        assert got[kind, "aligned"][0] <= got[kind, "direct"][0] + rec["oob_margin_db"]
    assert abs(got["dpd", "aligned"][2] - v["tau"]) <= v["tau_tol"]
