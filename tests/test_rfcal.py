"""Receiver calibration (mcrx_hip_rfcal_*), what needs no GPU: the boundary -- symbols, struct sizes, null handles, every configuration
error reported before a device is looked for -- the split of a call against the model, the host program of the plan, the closed form on
synthetic proper noise, the mixer helper against rfchain_model, and the severity of the case worth correcting, found on the oracle
alone."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import rfcal_model as model
import rfchain_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mcrx_hip_rfcal_clipped", "mcrx_hip_rfcal_create", "mcrx_hip_rfcal_destroy", "mcrx_hip_rfcal_execute_device",
           "mcrx_hip_rfcal_hold", "mcrx_hip_rfcal_last_error", "mcrx_hip_rfcal_position", "mcrx_hip_rfcal_read", "mcrx_hip_rfcal_reset_at",
           "mcrx_hip_rfcal_selftest", "mcrx_hip_rfcal_set", "mcrx_hip_rfcal_update"]


# ---------------------------------------------------------------------------------------------- the boundary
def test_symbols_are_declared_exported_and_bound(product):
    text = open(os.path.join(ROOT, "include", "mcrx_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(mcrx_hip_rfcal_[a-z_0-9]+)\s*\(", text))) == SYMBOLS
    assert [s for s in product.exported_symbols() if s.startswith("mcrx_hip_rfcal_")] == SYMBOLS
    L = product.lib()
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None
    assert C.sizeof(product.RfcalConfig) == 7 * 4 == 28
    assert C.sizeof(product.RfcalState) == 4 * 4 + 5 * 8 * 3 + 4 * 8 == 168
    assert re.search(r"uint32_t struct_size, stages;.*\n\s*uint32_t input_format, output_format;.*\n\s*uint32_t period_log2, forget_log2;.*\n\s*float\s+gain;\s*\n\} mcrx_hip_rfcal_config;", text)
    assert (product.RFCAL_DC, product.RFCAL_IQ) == (1, 2)
    for name, val in (("DC", "1u"), ("IQ", "2u")):
        assert re.search(r"#define MCRX_RFCAL_%s\s+%s" % (name, val), text)


def test_null_handles_are_answered(product):
    L = product.lib()
    assert L.mcrx_hip_rfcal_position(None) == 0
    assert L.mcrx_hip_rfcal_destroy(None) == product.MCRX_OK
    n, st, k = C.c_uint64(7), product.RfcalState(), C.c_uint64(0)
    for rc in (L.mcrx_hip_rfcal_clipped(None, C.byref(n), 0), L.mcrx_hip_rfcal_execute_device(None, None, 0, None, None),
               L.mcrx_hip_rfcal_create(None, None), L.mcrx_hip_rfcal_reset_at(None, 0), L.mcrx_hip_rfcal_update(None, None),
               L.mcrx_hip_rfcal_hold(None, 1), L.mcrx_hip_rfcal_set(None, 0.0, 0.0, 0.0, 0.0, None),
               L.mcrx_hip_rfcal_read(None, C.addressof(st), None), L.mcrx_hip_rfcal_selftest(None, 0, 1, None, None, 0, C.byref(k))):
        assert rc == product.MCRX_EINVAL
    assert L.mcrx_hip_rfcal_last_error()
    h = C.c_void_p(0x1234)
    assert L.mcrx_hip_rfcal_create(C.byref(h), None) == product.MCRX_EINVAL and not h.value


GOOD = dict(dc=True, iq=True, period_log2=14, forget_log2=3, gain=0.9, input_format="sc16", output_format="sc16")
NAN, INF = float("nan"), float("inf")
BAD = [("struct_size", "struct_size", 24), ("stage bits", "stages", 4), ("input format", "input_format", 2), ("output format", "output_format", 2),
       ("period 1", "period_log2", 1), ("period 5", "period_log2", 5), ("period 31", "period_log2", 31), ("forget 31", "forget_log2", 31),
       ("gain inf", "gain", INF), ("gain nan", "gain", NAN)]


@pytest.mark.parametrize("what,field,value", BAD, ids=[b[0] for b in BAD])
def test_configuration_errors_come_before_the_device(product, what, field, value):
    L = product.lib()
    c = product.rfcal_config(**GOOD)
    setattr(c, field, value)
    h = C.c_void_p(0x1234)
    assert L.mcrx_hip_rfcal_create(C.byref(h), C.addressof(c)) == product.MCRX_EINVAL, what
    assert not h.value                                                                     # *out is cleared
    assert L.mcrx_hip_rfcal_last_error()
    k = C.c_uint64(0)                                                                      # the selftest checks as create does
    assert L.mcrx_hip_rfcal_selftest(C.addressof(c), 0, 1, None, None, 0, C.byref(k)) == product.MCRX_EINVAL


def test_the_limits_themselves_are_accepted(product):
    """on the allowed side of every bound the answer is a handle, or 'no device' here -- never MCRX_EINVAL"""
    L = product.lib()
    for field, value in [("period_log2", 0), ("period_log2", 6), ("period_log2", 30), ("forget_log2", 0), ("forget_log2", 30), ("stages", 0),
                         ("stages", 3), ("gain", 0.0), ("gain", -3.0e38)]:
        c = product.rfcal_config(**GOOD)
        setattr(c, field, value)
        h = C.c_void_p()
        rc = L.mcrx_hip_rfcal_create(C.byref(h), C.addressof(c))
        assert rc in (product.MCRX_OK, product.MCRX_EHIP), (field, L.mcrx_hip_rfcal_last_error())
        if rc == product.MCRX_OK:
            L.mcrx_hip_rfcal_destroy(h)


PY_BAD = [dict(period_log2=5), dict(period_log2=31), dict(period_log2=-1), dict(period_log2=6.5), dict(forget_log2=31), dict(forget_log2=-1),
          dict(gain=INF), dict(gain=NAN), dict(input_format="sc8"), dict(output_format=2), dict(dc=1), dict(iq="yes")]


@pytest.mark.parametrize("kw", PY_BAD, ids=[str(i) for i in range(len(PY_BAD))])
def test_python_class_raises_value_error_without_a_device(product, kw):
    with pytest.raises(ValueError):
        product.rfcal(**kw)


# ---------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("k", [6, 10, 30])
def test_selftest_segments_equal_the_model(product, k):
    cfg = product.rfcal_config(period_log2=k, input_format="sc16")
    for pos in (0, 1, 12345, 2 ** 40, 2 ** 40 + 777, 2 ** 64 - 1000, 2 ** 64 - 1):
        for n in (1, 63, 64, 65, 1000, 4097, 70000):
            assert product.rfcal_segments(cfg, pos, n) == model.segments(pos, n, k), (pos, n, k)
    # a long call: the count without the list, and the first segments of it
    lens, ends = product.rfcal_segments(cfg, 5, 2 ** 32, cap=3)
    B = 1 << k
    assert lens == [B - 5, B, B][:len(lens)] and all(ends[:-1])
    nseg = C.c_uint64(0)
    assert product.lib().mcrx_hip_rfcal_selftest(C.addressof(cfg), 5, 2 ** 32, None, None, 0, C.byref(nseg)) == product.MCRX_OK
    assert nseg.value == 1 + -(-(2 ** 32 - (B - 5)) // B)
    manual = product.rfcal_config()
    assert product.rfcal_segments(manual, 2 ** 64 - 3, 1000) == ([1000], [False])
    assert product.rfcal_segments(manual, 0, 0) == ([], [])


def test_selftest_refuses_what_execute_refuses(product):
    with pytest.raises(ValueError):
        product.rfcal_segments(product.rfcal_config(), 0, 2 ** 32 + 1)                     # 2^32 samples a call
    assert product.rfcal_segments(product.rfcal_config(), 0, 2 ** 32) == ([2 ** 32], [False])
    sc = product.rfcal_config(input_format="sc16")                                         # manual updates: the whole call is one block
    assert product.rfcal_segments(sc, 7, 2 ** 31) == ([2 ** 31], [False])
    with pytest.raises(ValueError):
        product.rfcal_segments(sc, 7, 2 ** 31 + 1)
    assert len(product.rfcal_segments(product.rfcal_config(input_format="sc16", period_log2=30), 7, 2 ** 32)[0]) == 5


def test_host_program_of_the_plan(product):
    """host/rfcal_plan_test.cc: csrc/rfcal_plan.hpp with a main of its own (no GPU, no Python)"""
    host = os.path.join(ROOT, "liquid-usrp_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "rfcal_plan_test"])
    out = subprocess.run([os.path.join(ROOT, "liquid-usrp_amd", "lib", "rfcal_plan_test")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0 and b"rfcal_plan_test ok" in out.stdout, out.stdout.decode()


# ---------------------------------------------------------------------------------------------- the closed form
@pytest.mark.parametrize("gain_db,phase_deg,dc", [(1.0, 5.0, 0.0), (3.0, 15.0, 0.02 + 0.01j), (6.0, 30.0, 0.05 + 0.025j), (-2.0, -40.0, -0.3j)])
def test_closed_form_is_exact_on_proper_noise(product, gain_db, phase_deg, dc):
    """u = alpha z + beta conj(z) + d with z of sample mean 0 and sample mean z^2 = 0: the estimator returns beta / conj(alpha) and d to
    float64 rounding, and the corrected stream is alpha (1 - |w|^2) z."""
    mix = product.rfchain_iq(gain_db, phase_deg, "rx")
    al, be = mix["alpha"], mix["beta"]
    z = model.proper_noise(20000, 5, rms=0.1)                           # (no component reaches full scale)
    u = al * z + be * np.conj(z) + dc
    R = [u.real.mean(), u.imag.mean(), (u * u).real.mean(), (u * u).imag.mean(), (np.abs(u) ** 2).mean()]
    m, w = model.closed_form(R)
    assert abs(m - dc) <= 1e-15
    assert abs(w - be / al.conjugate()) <= 1e-12, (w, be / al.conjugate())
    y = model.apply(u, m, w)
    assert np.max(np.abs(y - al * (1.0 - abs(w) ** 2) * z)) <= 1e-12
    # through the model's state, an exact sc16 stream: the same, to the quantisation of the integers
    ints = np.stack([np.rint(u.real * 32768.0), np.rint(u.imag * 32768.0)], axis=1).astype(np.int16)
    st = model.State(sc16=True)
    st.measure(ints)
    st.update()
    assert st.updates == 1 and st.degenerate == 0 and st.count == 0
    assert abs(st.m - dc) <= 2e-5 and abs(st.w - be / al.conjugate()) <= 2e-4


def test_degenerate_blocks_keep_the_coefficients():
    for x in (np.zeros(64, np.complex64), np.full(64, 0.25 - 0.5j, np.complex64), np.linspace(-1, 1, 64).astype(np.complex64)):
        st = model.State()
        st.m, st.w = 0.1j, 0.2 + 0j
        st.measure(x)
        st.update()
        assert (st.m, st.w, st.updates, st.degenerate) == (0.1j, 0.2 + 0j, 1, 1)


def test_forgetting_rule():
    assert [model.mu(j, 3) for j in (0, 1, 6, 7, 8, 1000)] == [1.0, 0.5, 1.0 / 7.0, 0.125, 0.125, 0.125]
    st = model.State(forget_log2=0)                                     # every block replaces the means
    for seed in (1, 2):
        x = model.proper_noise(256, seed).astype(np.complex64)
        st.measure(x)
        st.update()
    assert np.allclose(st.mean[4], np.mean(np.abs(x.astype(np.complex128)) ** 2), rtol=1e-12)


# ---------------------------------------------------------------------------------------------- the mixer helper
def test_rfcal_as_mixer_is_the_correction(product):
    m, w = 0.03 - 0.01j, 0.12 + 0.2j
    mix = product.rfcal_as_mixer(m, w)
    assert set(mix) == {"alpha", "beta", "dc"} and mix["alpha"] == 1.0
    cfg = product.rfchain_config(order="rx", mixer=mix)
    u = model.proper_noise(1000, 9) + 0.1
    f32 = lambda z: complex(np.float32(z.real), np.float32(z.imag))
    got = rfchain_model.apply(cfg, u)
    assert np.max(np.abs(got - model.apply(u, m, w))) <= 4e-7            # (the configuration holds fp32 coefficients)
    assert abs(complex(cfg.beta_re, cfg.beta_im) - f32(-w)) == 0 and abs(complex(cfg.dc_re, cfg.dc_im) - f32(-m + w * m.conjugate())) == 0
    # it undoes a receive mixer: estimate, freeze, apply
    rx = product.rfchain_iq(1.0, 5.0, "rx")
    v = rx["alpha"] * u + rx["beta"] * np.conj(u)
    back = rfchain_model.apply(product.rfchain_config(order="rx", mixer=product.rfcal_as_mixer(0.0, rx["beta"] / rx["alpha"].conjugate())), v)
    k = rx["alpha"] * (1.0 - abs(rx["beta"] / rx["alpha"].conjugate()) ** 2)
    assert np.max(np.abs(back - k * u)) <= 1e-6


# ---------------------------------------------------------------------------------------------- severity of the case worth correcting
SEVERITY = dict(N=8, M=64, cp=16, taper=4, frames=3, payload_len=256, iq_gain_db=6.0, iq_phase_deg=30.0, dc=0.05 * (1 + 0.5j), snr_db=30.0,
                noise_seed=2025)


def severity_stream(product, oracle):
    """(u, sent, mixer): the oracle's transmitter, white noise 30 dB below its rms, through the receive mixer of rfchain_model"""
    s = SEVERITY
    iq, sent = oracle.synth_traffic(s["N"], s["M"], s["cp"], s["taper"], s["frames"], payload_len=s["payload_len"])
    rms = float(np.sqrt(np.mean(np.abs(iq.astype(np.complex128)) ** 2)))
    rng = np.random.default_rng(s["noise_seed"])
    sd = rms * 10.0 ** (-s["snr_db"] / 20.0) / math.sqrt(2.0)
    z = (iq.astype(np.complex128) + sd * (rng.standard_normal(len(iq)) + 1j * rng.standard_normal(len(iq)))).astype(np.complex64)
    mix = dict(product.rfchain_iq(s["iq_gain_db"], s["iq_phase_deg"], "rx"), dc=s["dc"])
    u = rfchain_model.apply(product.rfchain_config(order="rx", mixer=mix), z).astype(np.complex64)
    return u, sent, mix


def decode(oracle, y, sent):
    s = SEVERITY
    ora = oracle.MultiChannelRx(s["N"], s["M"], s["cp"], s["taper"])
    ora.execute(np.ascontiguousarray(np.asarray(y, np.complex64)))
    good = [f for f in ora.frames if f.header_valid and f.payload_valid and ((f.header[0] << 8) | f.header[1]) < len(sent[f.channel])
            and sent[f.channel][(f.header[0] << 8) | f.header[1]] == (bytes(f.header), bytes(f.payload))]
    return ora.frames, good


def test_severity_on_the_oracle_alone(product, oracle):
    """6 dB / 30 degrees / DC 0.05 (1 + 0.5j) at 30 dB SNR.  Uncorrected the oracle loses frames; corrected by the model's estimate over
    the whole stream every frame is valid with identical bytes, at an EVM at least 20 dB better than the worst uncorrected frame.
    (The issue's own alpha, beta gave 26 dB better; the figure with rfchain_iq's receive convention is printed here.)"""
    s = SEVERITY
    u, sent, mix = severity_stream(product, oracle)
    total = s["N"] * s["frames"]
    st = model.State()
    st.measure(u)
    st.update()
    truth = mix["beta"] / mix["alpha"].conjugate()
    before, after = -20 * math.log10(abs(truth)), -20 * math.log10(abs((truth - st.w) / (1 - truth.conjugate() * st.w) if st.w != truth else 1e-30))
    frames0, good0 = decode(oracle, u, sent)
    frames1, good1 = decode(oracle, model.apply_fp32(u, st.m, st.w), sent)
    evm0, evm1 = [f.evm for f in frames0], [f.evm for f in frames1]
    print("rfcal severity: image rejection %.1f -> %.1f dB, |m - d| %.2e; uncorrected %d/%d valid, EVM %.1f .. %.1f dB; corrected %d/%d valid, EVM %.1f .. %.1f dB; margin %.1f dB"
          % (before, after, abs(st.m - s["dc"]), len(good0), total, min(evm0), max(evm0), len(good1), total, min(evm1), max(evm1), max(evm0) - max(evm1)))
    assert len(frames1) == len(good1) == total and len({(f.channel, f.header[1]) for f in good1}) == total
    assert len(good0) < total                                           # the case is worth correcting
    assert max(evm1) <= max(evm0) - 20.0
