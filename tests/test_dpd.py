"""Digital predistortion (mcrx_hip_dpd_*), what needs no GPU: the boundary -- symbols, null handles, every configuration error reported
before a device is looked for --, the library's host arithmetic (constants, bins, eligibility) against tests/dpd_model.py, the guard's
bound, the host program of the plan, and the severity of the end-to-end cases of tests/test_gpu_dpd.py found on the oracle alone with
the exact model."""
import ctypes as C
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cfr_model
import dpd_model as model
import rfchain_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mcrx_hip_dpd_clipped", "mcrx_hip_dpd_create", "mcrx_hip_dpd_destroy", "mcrx_hip_dpd_execute_device", "mcrx_hip_dpd_last_error",
           "mcrx_hip_dpd_measure_device", "mcrx_hip_dpd_output_format", "mcrx_hip_dpd_read", "mcrx_hip_dpd_reset", "mcrx_hip_dpd_selftest",
           "mcrx_hip_dpd_set_table", "mcrx_hip_dpd_update"]
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------- the boundary
def test_symbols_are_declared_exported_and_bound(product):
    text = open(os.path.join(ROOT, "include", "mcrx_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(mcrx_hip_dpd_[a-z_0-9]+)\s*\(", text))) == SYMBOLS
    assert [s for s in product.exported_symbols() if s.startswith("mcrx_hip_dpd_")] == SYMBOLS
    L = product.lib()
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", product.build()]).decode()
    assert sorted(set(re.findall(r" T (mcrx_hip_dpd_[a-z_0-9]+)", out))) == SYMBOLS
    assert C.sizeof(product.DpdConfig) == 8 * 4 and C.sizeof(product.DpdState) == 3 * 8
    assert (product.DPD_MIN_LOG2, product.DPD_MAX_LOG2, product.DPD_MAX_FORGET, product.DPD_GUARD_LOG2) == (5, 10, 8, 28)


def test_null_handles_are_answered(product):
    L = product.lib()
    assert L.mcrx_hip_dpd_output_format(None) == 0
    assert L.mcrx_hip_dpd_destroy(None) == product.MCRX_OK
    n, st = C.c_uint64(7), product.DpdState()
    for rc in (L.mcrx_hip_dpd_clipped(None, C.byref(n), 0), L.mcrx_hip_dpd_execute_device(None, None, 0, None, None),
               L.mcrx_hip_dpd_measure_device(None, None, None, 0, None), L.mcrx_hip_dpd_update(None, None),
               L.mcrx_hip_dpd_set_table(None, None, None), L.mcrx_hip_dpd_read(None, C.addressof(st), None, None, None),
               L.mcrx_hip_dpd_reset(None), L.mcrx_hip_dpd_create(None, None),
               L.mcrx_hip_dpd_selftest(None, None, None, None, None, None, 0, None)):
        assert rc == product.MCRX_EINVAL
    assert L.mcrx_hip_dpd_last_error()
    h = C.c_void_p(0x1234)
    assert L.mcrx_hip_dpd_create(C.byref(h), None) == product.MCRX_EINVAL and not h.value
    c = good_config(product)
    assert L.mcrx_hip_dpd_selftest(C.addressof(c), None, None, None, None, None, 3, None) == product.MCRX_EINVAL      # pairs without buffers


def good_config(product):
    return product.dpd_config(7, 0.75, 2.0, min_count=8, forget_shift=2, gain=0.9, output_format="sc16")


BAD = [("struct_size", "struct_size", 28), ("table_log2 4", "table_log2", 4), ("table_log2 11", "table_log2", 11), ("full_scale 0", "full_scale", 0.0),
       ("full_scale negative", "full_scale", -0.5), ("full_scale nan", "full_scale", NAN), ("full_scale inf", "full_scale", INF),
       ("full_scale too small for inv_step", "full_scale", 1e-42), ("target_gain 0", "target_gain", 0.0), ("target_gain negative", "target_gain", -1.0),
       ("target_gain nan", "target_gain", NAN), ("target_gain inf", "target_gain", INF), ("min_count 0", "min_count", 0),
       ("forget_shift 9", "forget_shift", 9), ("gain nan", "gain", NAN), ("gain inf", "gain", INF), ("output format", "output_format", 2)]


@pytest.mark.parametrize("what,field,value", BAD, ids=[b[0] for b in BAD])
def test_configuration_errors_come_before_the_device(product, what, field, value):
    L = product.lib()
    c = good_config(product)
    setattr(c, field, value)
    h = C.c_void_p(0x1234)
    assert L.mcrx_hip_dpd_create(C.byref(h), C.addressof(c)) == product.MCRX_EINVAL, what
    assert not h.value                                                                     # *out is cleared
    assert L.mcrx_hip_dpd_last_error()
    assert L.mcrx_hip_dpd_selftest(C.addressof(c), None, None, None, None, None, 0, None) == product.MCRX_EINVAL, what


def test_the_limits_themselves_are_accepted(product):
    """on the allowed side of every bound the answer is a handle, or 'no device' here -- never MCRX_EINVAL"""
    L = product.lib()
    edits = [("table_log2", 5), ("table_log2", 10), ("full_scale", 1e-30), ("full_scale", 3e38), ("target_gain", 1e-30), ("target_gain", 3e38),
             ("min_count", 1), ("min_count", 0xffffffff), ("forget_shift", 0), ("forget_shift", 8), ("gain", 0.0), ("gain", -3.0),
             ("output_format", 0), ("output_format", 1)]
    for field, value in edits:
        c = good_config(product)
        setattr(c, field, value)
        h = C.c_void_p()
        rc = L.mcrx_hip_dpd_create(C.byref(h), C.addressof(c))
        assert rc in (product.MCRX_OK, product.MCRX_EHIP), (field, L.mcrx_hip_dpd_last_error())
        if rc == product.MCRX_OK:
            assert L.mcrx_hip_dpd_output_format(h) == c.output_format
            L.mcrx_hip_dpd_destroy(h)


PY_BAD = [dict(), dict(full_scale=1.0), dict(target_gain=1.0), dict(full_scale=0.0, target_gain=1.0), dict(full_scale=-1.0, target_gain=1.0),
          dict(full_scale=NAN, target_gain=1.0), dict(full_scale=INF, target_gain=1.0), dict(full_scale=1.0, target_gain=0.0),
          dict(full_scale=1.0, target_gain=NAN), dict(full_scale=1.0, target_gain=1.0, table_log2=4), dict(full_scale=1.0, target_gain=1.0, table_log2=11),
          dict(full_scale=1.0, target_gain=1.0, table_log2=7.5), dict(full_scale=1.0, target_gain=1.0, min_count=0),
          dict(full_scale=1.0, target_gain=1.0, min_count=-1), dict(full_scale=1.0, target_gain=1.0, forget_shift=9),
          dict(full_scale=1.0, target_gain=1.0, forget_shift=True), dict(full_scale=1.0, target_gain=1.0, gain=INF),
          dict(full_scale=1.0, target_gain=1.0, output_format="sc8"), dict(full_scale=1.0, target_gain=1.0, output_format=2)]


@pytest.mark.parametrize("kw", PY_BAD, ids=[str(i) for i in range(len(PY_BAD))])
def test_python_class_raises_value_error_without_a_device(product, kw):
    with pytest.raises(ValueError):
        product.dpd(**kw)
    with pytest.raises(ValueError):
        product.dpd_config(**kw)


def test_host_program_of_the_plan(product):
    """host/dpd_plan_test.cc: csrc/dpd_plan.hpp with a main of its own (no GPU, no Python)"""
    host = os.path.join(ROOT, "liquid-usrp_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "dpd_plan_test"])
    out = subprocess.run([os.path.join(ROOT, "liquid-usrp_amd", "lib", "dpd_plan_test")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0 and b"dpd_plan_test ok" in out.stdout, out.stdout.decode()


# ---------------------------------------------------------------------------------------------- the host arithmetic against the model
@pytest.mark.parametrize("log2,fs", [(5, 1.0), (7, 0.75), (10, 0.3), (7, 0.5), (7, 0.50000006), (6, 2.0), (8, 2.0000002), (7, 1e-3), (5, 3e38), (10, 1e-30)])
def test_constants_equal_the_model(product, log2, fs):
    c = product.dpd_config(log2, fs, 1.0)
    inv_step, step, e = product.dpd_constants(c)
    K, m_inv, m_step, m_e = model.constants(log2, fs)
    assert (inv_step, step, e) == (float(m_inv), m_step, m_e)
    assert 2.0 ** e >= float(np.float32(fs)) > 2.0 ** (e - 1)
    assert inv_step == float(np.float32(K / float(np.float32(fs)))) and step == float(np.float32(fs)) / K


def edge_cases(K, fs, seed):
    """(u, z): amplitudes on every bin edge, on every tie between two bins and one ulp either side of both, at random phases; the end
    of the table and beyond it; random amplitudes; and one pair of every ineligible kind"""
    rng = np.random.RandomState(seed)
    fs = float(np.float32(fs))
    edges = np.arange(0, K + 2, dtype=np.float64) * fs / K
    ties = (np.arange(0, K + 1, dtype=np.float64) + 0.5) * fs / K
    amp = np.concatenate([edges, ties]).astype(np.float32)
    amp = np.concatenate([amp, np.nextafter(amp, np.float32(0)), np.nextafter(amp, np.float32(np.inf)), rng.uniform(0, 1.2 * fs, 4000).astype(np.float32)])
    ph = rng.uniform(0, 2 * np.pi, len(amp))
    ph[:len(edges) + len(ties)] = 0.0                                                      # (on the real axis the amplitude survives the fp32 norm)
    u = (amp * np.exp(1j * ph)).astype(np.complex64)
    z = (0.9 * u * np.exp(0.1j)).astype(np.complex64)
    E = 2.0 ** model.constants(int(math.log2(K)), fs)[3]
    odd_u = np.array([NAN, complex(0, NAN), INF, complex(0, -INF), 0.5 * fs, 0.5 * fs, 0.5 * fs, 0.5 * fs, 0.5 * fs, 3e30, 10 * fs], np.complex64)
    odd_z = np.array([0.1, 0.1, 0.1, 0.1, NAN, complex(0, NAN), INF, 4.0 * E, np.nextafter(np.float32(4.0 * E), np.float32(np.inf)), 0.1, 0.1], np.complex64)
    return np.concatenate([u, odd_u]), np.concatenate([z, odd_z])


@pytest.mark.parametrize("log2,fs", [(5, 1.0), (7, 0.75), (10, 0.3), (10, 1.0), (7, 0.0123)])
def test_selftest_bins_equal_the_model(product, log2, fs):
    K = 1 << log2
    c = product.dpd_config(log2, fs, 1.0)
    u, z = edge_cases(K, fs, seed=log2)
    got, want = product.dpd_bins(c, u, z), model.bins(u, z, log2, fs)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    assert list(got[-11:]) == [-1, -1, -1, -1, -1, -1, -1, K // 2, -1, -1, -1]             # (|z| = 4 E is the last eligible one)
    assert got.max() == K and (got == 0).any()
    if fs == 1.0:                                                                          # every product exact: edges and ties as written
        edges, ties = got[:K + 2], got[K + 2:2 * K + 3]
        assert list(edges) == list(range(K + 1)) + [-1]
        assert list(ties) == [j if j % 2 == 0 else j + 1 for j in range(K)] + [K]           # ties go to the even bin; K + 1/2 down to K


def test_the_model_fma_rounds_once():
    """model.fmaf against exact rational arithmetic on inputs chosen to sit on and beside fp32 ties"""
    import fractions
    rng = np.random.RandomState(5)
    a = rng.standard_normal(2000).astype(np.float32)
    b = rng.standard_normal(2000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32) * np.float32(2.0) ** rng.randint(-30, 2, 2000).astype(np.float32)
    a[:3], b[:3], c[:3] = [1.0 + 2.0 ** -12] * 3, [1.0 + 2.0 ** -12] * 3, [0.0, 2.0 ** -60, -2.0 ** -60]      # 1 + 2^-11 + 2^-24: a tie
    got = model.fmaf(a, b, c)
    for i in range(len(a)):
        exact = fractions.Fraction(float(a[i])) * fractions.Fraction(float(b[i])) + fractions.Fraction(float(c[i]))
        lo = np.float32(float(exact))                                                      # (Fraction -> float is correctly rounded; then
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]      # pick the nearest fp32 exactly)
        err = [abs(fractions.Fraction(float(v)) - exact) for v in cands]
        best = min(err)
        near = [v for v, e in zip(cands, err) if e == best]
        want = near[0] if len(near) == 1 else [v for v in near if (np.float32(v).view(np.uint32) & 1) == 0][0]
        assert got[i] == want, (i, a[i], b[i], c[i], got[i], want)


def test_the_guard_bound(product):
    """2^28 samples of the largest term stay inside an int64, and the model's count follows an update as the library's does"""
    for log2 in (5, 7, 10):
        for fs in (1.0, 0.50000006, 0.75):
            K, inv_step, _, e = model.constants(log2, fs)
            E = 2.0 ** e
            top = np.float32(float(np.float32(fs)) * (1.0 + 0.5 / K))
            while model.bins([np.nextafter(top, np.float32(np.inf))], [0], log2, fs)[0] >= 0:
                top = np.nextafter(top, np.float32(np.inf))
            while model.bins([top], [0], log2, fs)[0] < 0:
                top = np.nextafter(top, np.float32(0))
            c = product.dpd_config(log2, fs, 1.0)
            assert product.dpd_bins(c, [top, np.nextafter(top, np.float32(np.inf))], [4.0 * E, 4.0 * E]).tolist() == [K, -1]
            sre, sim, suu = model.terms(np.array([top], np.complex64), np.array([4.0 * E], np.complex64), e)
            assert 2 ** 33 < int(sre[0]) < 2 ** 34.1 and int(suu[0]) < 2 ** 34.1 and int(sim[0]) == 0
            assert int(sre[0]) * 2 ** model.GUARD_LOG2 < 2 ** 63
    m = model.Model(7, 1.0, 1.0, forget_shift=2)
    u = np.full(5, 0.5, np.complex64)
    assert m.measure(u, u) and m.since == 5
    m.update()
    assert m.since == 2 and m.cnt[64] == 1                                                 # ceil(5 / 4); 5 >> 2
    m.since = (1 << 28) - 4
    assert not m.measure(u, u) and m.since == (1 << 28) - 4 and m.cnt[64] == 1             # refused: nothing measured
    assert m.measure(u[:4], u[:4]) and m.since == 1 << 28


def test_the_update_of_a_linear_amplifier_is_its_inverse():
    """z = A u with one complex A: every valid bin measures A, and the table becomes g0 / A wherever the drive was -- below the first
    valid bin and in the gaps too"""
    A = 0.8 * np.exp(0.3j)
    m = model.Model(6, 1.0, 1.0, min_count=2)
    rng = np.random.RandomState(3)
    u = (rng.uniform(0.2, 0.7, 4000) * np.exp(2j * np.pi * rng.uniform(0, 1, 4000))).astype(np.complex64)
    z = (A * u.astype(np.complex128)).astype(np.complex64)
    assert m.measure(u, z)
    m.update()
    assert m.updates == 1 and m.degenerate == 0
    # 1 / A up to the table's end: beyond g0 r = |A| full_scale the drive would leave the table, and the entry holds r_K / r_i
    i = np.arange(1, 65)
    inside = i * (1.0 / 64) <= abs(A) * 1.0
    assert np.abs(m.F[1:][inside] - 1.0 / A).max() < 1e-6
    assert np.allclose(np.abs(m.F[1:][~inside]), 64.0 / i[~inside], rtol=1e-6)
    assert m.F[0] == m.F[1]
    empty = model.Model(6, 1.0, 1.0, min_count=2)
    empty.update()
    assert empty.degenerate == 1 and empty.updates == 1 and np.all(empty.F == 1)


# ---------------------------------------------------------------------------------------------- severity of the end-to-end cases
def decode(oracle, s, sent, y, channels=None):
    """the oracle's receiver on the stream y: the EVMs, with every frame asserted valid and its bytes the ones sent"""
    channels = list(range(s["N"])) if channels is None else channels
    ora = oracle.MultiChannelRx(s["N"], s["M"], s["cp"], s["taper"])
    ora.execute(np.ascontiguousarray(np.asarray(y).astype(np.complex64)))
    frames = [f for f in ora.frames if f.channel in channels]
    assert len(frames) == len(channels) * s["frames"], len(frames)
    seen = set()
    for f in frames:
        assert f.header_valid and f.payload_valid, f
        pid = (f.header[0] << 8) | f.header[1]
        assert sent[f.channel][pid] == (bytes(f.header), bytes(f.payload)), (f.channel, pid)
        seen.add((f.channel, pid))
    assert len(seen) == len(channels) * s["frames"]
    return [f.evm for f in frames]


def learn(m, x, amp, rounds):
    """`rounds` times execute -> amplifier -> measure -> update on the model; u and z are what a cf32 handle and a cf32 amplifier store"""
    for _ in range(rounds):
        u = m.execute(x).astype(np.complex64)
        z = rfchain_model.amplifier(amp, u.astype(np.complex128)).astype(np.complex64)
        assert m.measure(u, z)
        m.update()


@functools.lru_cache(maxsize=None)
def severity_case(product, oracle):
    """(x, sent, amp, full_scale): cfr_model.SEVERITY's stream behind its stage, the amplifier's configuration, the table's end"""
    s, d = cfr_model.SEVERITY, model.SEVERITY
    iq, sent = oracle.synth_traffic(s["N"], s["M"], s["cp"], s["taper"], s["frames"], payload_len=s["payload_len"])
    rms = cfr_model.rms(iq)
    h = product.cfr_lowpass(s["half_len"], s["cutoff"], s["beta"])
    A = float(np.float32(product.cfr_threshold(s["papr_db"], rms)))
    x = cfr_model.apply_stream(iq, A, h, s["passes"]).astype(np.complex64)
    amp = product.rfchain_config(amplifier=dict(sat=product.rfchain_backoff(d["amp_ibo_db"], rms), smooth=d["amp_smooth"], gain=d["amp_gain"],
                                                ampm_deg=d["amp_ampm_deg"]))
    return x, sent, amp, float(np.float32(d["full_scale_over_peak"] * np.abs(x).max())), cfr_model.papr_db(iq)


def test_severity_on_the_oracle_alone(product, oracle):
    """The oracle's transmitter, cfr's model, the exact model of the predistorter and rfchain's amplifier model at dpd_model.SEVERITY:
    after three updates the power at |f| > 0.32 lies at least 25 dB below the uncorrected amplifier's and the NMSE against
    amp_gain * x is at least 30 dB better, every frame valid with its bytes as sent throughout."""
    s, d = cfr_model.SEVERITY, model.SEVERITY
    x, sent, amp, full_scale, papr0 = severity_case(product, oracle)
    ref = float(amp.amp_gain) * x.astype(np.complex128)
    m = model.Model(d["table_log2"], full_scale, d["amp_gain"])
    rows = []
    for r in range(d["rounds"] + 1):
        y = rfchain_model.amplifier(amp, m.execute(x).astype(np.complex64).astype(np.complex128))
        evm = decode(oracle, s, sent, y)
        rows.append((cfr_model.oob_db(y, d["edge"]), model.nmse_db(y, ref), min(evm), max(evm)))
        if r < d["rounds"]:
            learn(m, x, amp, 1)
    print("dpd severity: %d samples, PAPR %.1f -> %.1f dB, peak / amp_sat %.3f, full_scale %.4f; %d bins valid of %d"
          % (len(x), papr0, cfr_model.papr_db(x), float(np.abs(x).max()) / float(amp.amp_sat), full_scale,
             sum(1 for c, v in zip(m.cnt, m.Suu) if c >= m.min_count and v > 0), m.K + 1))
    for r, (oob, nmse, e0, e1) in enumerate(rows):
        print("dpd severity after %d updates: power at |f| > %.2f %.1f dB, NMSE %.1f dB, oracle EVM %.1f .. %.1f dB" % (r, d["edge"], oob, nmse, e0, e1))
    assert m.degenerate == 0 and m.updates == d["rounds"] and m.skipped == 0
    assert rows[0][0] - rows[-1][0] >= d["oob_gain_db"]
    assert rows[0][1] - rows[-1][1] >= d["nmse_gain_db"]


@functools.lru_cache(maxsize=None)
def two_carrier_case(oracle):
    """(x, sent): channels 3 and 4 of 8 carry three frames each, the rest are silent; the oracle's transmitter at gain 1 / N"""
    s, t = cfr_model.SEVERITY, model.TWO_CARRIER
    tx = oracle.MultiChannelTx(s["N"], s["M"], s["cp"], s["taper"])
    chans = range(t["first"], t["first"] + t["count"])
    rngs = {c: np.random.RandomState(977 + c) for c in chans}
    sent, pid, chunks, idle = [[] for _ in range(s["N"])], {c: 0 for c in chans}, [], 0
    L = s["M"] + s["cp"]
    while idle < 64:
        for c in chans:
            if pid[c] < s["frames"] and tx.ready(c):
                hdr = bytes([0, pid[c], c]) + bytes(rngs[c].randint(0, 256, 5).astype(np.uint8))
                pl = bytes(rngs[c].randint(0, 256, s["payload_len"]).astype(np.uint8))
                tx.update(c, hdr, pl)
                sent[c].append((hdr, pl))
                pid[c] += 1
        chunks.append(tx.generate(L))
        if all(pid[c] >= s["frames"] and tx.ready(c) for c in chans):
            idle += L
    return (np.concatenate(chunks) * np.float32(1.0 / s["N"])).astype(np.complex64), sent


def two_carrier_backoff(x):
    """the least whole number of dB of input back-off at which the stream's peak is at most 0.85 of the saturation amplitude"""
    rms, peak = cfr_model.rms(x), float(np.abs(x).max())
    ibo = 0
    while peak > model.TWO_CARRIER["peak_over_sat"] * rms * 10.0 ** (ibo / 20.0):
        ibo += 1
    return float(ibo)


def channel_levels_db(oracle, y):
    s = cfr_model.SEVERITY
    ch = oracle.MultiChannelRx(s["N"], s["M"], s["cp"], s["taper"]).channelize(np.asarray(y).astype(np.complex64))
    return 10.0 * np.log10(np.maximum(np.mean(np.abs(ch.astype(np.complex128)) ** 2, axis=0), 1e-300))


def test_two_carriers_on_the_oracle_alone(product, oracle):
    """Channels 3 and 4 carry frames, no cfr: the amplifier's third-order products land in channels 2 and 5 (tests/test_gpu_rfchain.py);
    three updates bring them down.  Recorded (dpd_model.TWO_CARRIER["recorded_db"]): at 13 dB back-off (peak 0.78 of amp_sat) channel 2
    falls by 2.25 dB and channel 5 by 2.12 dB -- to within 0.05 dB of what the bank's own skirt of the two carriers leaves there with no
    amplifier at all (-39.2 and -38.8 dB), which is as far as they can fall.  The fifth-order products in channels 1 and 6, which no
    skirt hides, fall by 14.7 dB."""
    s, t = cfr_model.SEVERITY, model.TWO_CARRIER
    x, sent = two_carrier_case(oracle)
    ibo = two_carrier_backoff(x)
    rms, peak = cfr_model.rms(x), float(np.abs(x).max())
    amp = product.rfchain_config(amplifier=dict(sat=product.rfchain_backoff(ibo, rms), smooth=t["amp_smooth"], ampm_deg=t["amp_ampm_deg"]))
    assert peak <= t["peak_over_sat"] * float(amp.amp_sat) * (1 + 1e-6)
    m = model.Model(t["table_log2"], float(np.float32(t["full_scale_over_peak"] * peak)), 1.0)
    before = channel_levels_db(oracle, rfchain_model.amplifier(amp, x.astype(np.complex128)))
    clean = channel_levels_db(oracle, x)
    learn(m, x, amp, t["rounds"])
    y = rfchain_model.amplifier(amp, m.execute(x).astype(np.complex64).astype(np.complex128))
    after = channel_levels_db(oracle, y)
    decode(oracle, s, sent, y, channels=[3, 4])
    print("dpd two carriers: back-off %.0f dB, PAPR %.1f dB, peak / amp_sat %.3f" % (ibo, cfr_model.papr_db(x), peak / float(amp.amp_sat)))
    for name, lv in (("no amplifier", clean), ("amplifier", before), ("dpd + amplifier", after)):
        print("dpd two carriers, %-16s levels [dB] " % (name + ":") + " ".join("%.1f" % v for v in lv))
    print("dpd two carriers: channel 2 falls by %.2f dB, channel 5 by %.2f dB" % (before[2] - after[2], before[5] - after[5]))
    for c in (2, 5):
        assert before[c] - after[c] >= t["recorded_db"][c] - 0.05, (c, before[c] - after[c])
        assert abs(after[c] - clean[c]) <= 0.1                                             # down to the bank's own skirt, which is the floor
    assert before[1] - after[1] >= 14.0 and before[6] - after[6] >= 14.0
