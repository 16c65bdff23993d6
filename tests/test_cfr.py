"""Crest-factor reduction (mcrx_hip_cfr_*), what needs no GPU: the boundary -- symbols, null handles, every configuration error
reported before a device is looked for -- the low-pass design against the model's own formula and its response, the host program of
the plan, and the severity of the end-to-end cases of tests/test_gpu_cfr.py found on the oracle alone with the float64 model."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cfr_model as model
import rfchain_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mcrx_hip_cfr_clipped", "mcrx_hip_cfr_create", "mcrx_hip_cfr_design", "mcrx_hip_cfr_destroy", "mcrx_hip_cfr_execute_device",
           "mcrx_hip_cfr_halo", "mcrx_hip_cfr_last_error", "mcrx_hip_cfr_output_format", "mcrx_hip_cfr_stats"]
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------- the boundary
def test_symbols_are_declared_exported_and_bound(product):
    text = open(os.path.join(ROOT, "include", "mcrx_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(mcrx_hip_cfr_[a-z_0-9]+)\s*\(", text))) == SYMBOLS
    assert [s for s in product.exported_symbols() if s.startswith("mcrx_hip_cfr_")] == SYMBOLS
    L = product.lib()
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", product.build()]).decode()
    assert sorted(set(re.findall(r" T (mcrx_hip_cfr_[a-z_0-9]+)", out))) == SYMBOLS
    # 4 words, 2 floats, 65 taps
    assert C.sizeof(product.CfrConfig) == 4 * 4 + 2 * 4 + 65 * 4 == 284
    assert (product.CFR_MAX_HALF_LEN, product.CFR_MAX_PASSES) == (64, 4)
    for name, val in (("MAX_HALF_LEN", "64"), ("MAX_PASSES", "4")):
        assert re.search(r"#define MCRX_CFR_%s\s+%s\b" % (name, val), text)


def test_null_handles_are_answered(product):
    L = product.lib()
    assert L.mcrx_hip_cfr_halo(None) == 0 and L.mcrx_hip_cfr_output_format(None) == 0
    assert L.mcrx_hip_cfr_destroy(None) == product.MCRX_OK
    n, over, peak = C.c_uint64(7), (C.c_uint64 * 4)(), C.c_float(0.0)
    for rc in (L.mcrx_hip_cfr_clipped(None, C.byref(n), 0), L.mcrx_hip_cfr_execute_device(None, None, 0, None, None),
               L.mcrx_hip_cfr_create(None, None), L.mcrx_hip_cfr_stats(None, over, C.byref(peak), 0),
               L.mcrx_hip_cfr_design(31, 0.28, 5.65, None)):
        assert rc == product.MCRX_EINVAL
    assert L.mcrx_hip_cfr_last_error()
    h = C.c_void_p(0x1234)
    assert L.mcrx_hip_cfr_create(C.byref(h), None) == product.MCRX_EINVAL and not h.value


def good_config(product):
    return product.cfr_config(0.5, half_len=31, passes=2, gain=0.9, output_format="sc16")


def set_field(c, field, value):
    if isinstance(field, tuple):
        c.taps[field[1]] = value
    else:
        setattr(c, field, value)


BAD = [("struct_size", "struct_size", 280), ("half_len 0", "half_len", 0), ("half_len 65", "half_len", 65), ("passes 0", "passes", 0),
       ("passes 5", "passes", 5), ("output format", "output_format", 2), ("threshold 0", "threshold", 0.0),
       ("threshold negative", "threshold", -0.5), ("threshold nan", "threshold", NAN), ("threshold inf", "threshold", INF),
       ("threshold^2 overflows", "threshold", 1e30), ("threshold^2 underflows", "threshold", 1e-30), ("gain inf", "gain", INF),
       ("gain nan", "gain", NAN), ("h[0] nan", ("taps", 0), NAN), ("h[H] inf", ("taps", 31), INF), ("h[5] -inf", ("taps", 5), -INF)]


@pytest.mark.parametrize("what,field,value", BAD, ids=[b[0] for b in BAD])
def test_configuration_errors_come_before_the_device(product, what, field, value):
    L = product.lib()
    c = good_config(product)
    set_field(c, field, value)
    h = C.c_void_p(0x1234)
    assert L.mcrx_hip_cfr_create(C.byref(h), C.addressof(c)) == product.MCRX_EINVAL, what
    assert not h.value                                                                     # *out is cleared
    assert L.mcrx_hip_cfr_last_error()


def test_the_limits_themselves_are_accepted(product):
    """on the allowed side of every bound the answer is a handle, or 'no device' here -- never MCRX_EINVAL"""
    L = product.lib()
    edits = [("half_len", 1), ("half_len", 64), ("passes", 1), ("passes", 4), ("output_format", 0), ("output_format", 1),
             ("threshold", 1e-18), ("threshold", 1e18), ("gain", 0.0), ("gain", -3.0), (("taps", 32), NAN), (("taps", 64), INF)]
    for field, value in edits:
        c = good_config(product)
        set_field(c, field, value)                                                         # (taps behind h[H] are not looked at)
        h = C.c_void_p()
        rc = L.mcrx_hip_cfr_create(C.byref(h), C.addressof(c))
        assert rc in (product.MCRX_OK, product.MCRX_EHIP), (field, L.mcrx_hip_cfr_last_error())
        if rc == product.MCRX_OK:
            assert L.mcrx_hip_cfr_halo(h) == c.passes * c.half_len and L.mcrx_hip_cfr_output_format(h) == c.output_format
            L.mcrx_hip_cfr_destroy(h)


PY_BAD = [dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=NAN), dict(threshold=INF), dict(threshold=0.5, passes=0),
          dict(threshold=0.5, passes=5), dict(threshold=0.5, passes=1.5), dict(threshold=0.5, gain=INF), dict(threshold=0.5, output_format="sc8"),
          dict(threshold=0.5, output_format=2), dict(threshold=0.5, half_len=0), dict(threshold=0.5, half_len=65), dict(threshold=0.5, half_len=2.5),
          dict(threshold=0.5, cutoff=0.0), dict(threshold=0.5, cutoff=0.5), dict(threshold=0.5, cutoff=NAN), dict(threshold=0.5, beta=-1.0),
          dict(threshold=0.5, beta=INF), dict(threshold=0.5, taps=[1.0]), dict(threshold=0.5, taps=np.ones(66)), dict(threshold=0.5, taps=np.ones((2, 3))),
          dict(threshold=0.5, taps=[0.5, NAN]), dict(threshold=0.5, taps=np.array([1 + 0j, 0.1]))]


@pytest.mark.parametrize("kw", PY_BAD, ids=[str(i) for i in range(len(PY_BAD))])
def test_python_class_raises_value_error_without_a_device(product, kw):
    with pytest.raises(ValueError):
        product.cfr(**kw)


def test_python_helpers(product):
    assert product.cfr_threshold(7.0, 0.25) == 0.25 * 10.0 ** 0.35
    c = product.cfr_config(0.5, taps=[0.5, 0.25], passes=3, gain=2.0, output_format="sc16")
    assert (c.half_len, c.passes, c.output_format, c.threshold, c.gain) == (1, 3, 1, 0.5, 2.0) and list(c.taps[:3]) == [0.5, 0.25, 0.0]
    c = product.cfr_config(0.5)
    assert c.half_len == 31 and c.passes == 1 and np.array_equal(np.array(c.taps[:32], np.float32), product.cfr_lowpass(31, 0.28, 5.65))
    for bad in (dict(half_len=0, cutoff=0.28, beta=5.65), dict(half_len=31, cutoff=0.6, beta=5.65), dict(half_len=31, cutoff=0.28, beta=-0.1),
                dict(half_len=31, cutoff=INF, beta=5.65), dict(half_len=31, cutoff=0.28, beta=NAN)):
        with pytest.raises(ValueError):
            product.cfr_lowpass(**bad)


def test_host_program_of_the_plan(product):
    """host/cfr_plan_test.cc: csrc/cfr_plan.hpp with a main of its own (no GPU, no Python)"""
    host = os.path.join(ROOT, "liquid-usrp_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "cfr_plan_test"])
    out = subprocess.run([os.path.join(ROOT, "liquid-usrp_amd", "lib", "cfr_plan_test")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0 and b"cfr_plan_test ok" in out.stdout, out.stdout.decode()


# ---------------------------------------------------------------------------------------------- the low-pass
@pytest.mark.parametrize("H,fc,beta", [(31, 0.28, 5.65), (1, 0.25, 0.0), (7, 0.3, 3.0), (63, 0.28, 5.65), (64, 0.1, 9.0), (40, 0.49, 12.0)])
def test_design_equals_the_formula(product, H, fc, beta):
    h = product.cfr_lowpass(H, fc, beta)
    want = model.lowpass(H, fc, beta)
    assert h.dtype == np.float32 and h.shape == (H + 1,)
    assert float(np.abs(h.astype(np.float64) - want).max()) <= 1e-6
    assert abs(float(h[0]) + 2.0 * float(h[1:].astype(np.float64).sum()) - 1.0) <= 1e-6


def test_response_of_the_default_low_pass(product):
    """the taps the library returns for the defaults: flat within 0.1 dB where the channels are, and in the stop band at least what
    the float64 formula itself gives, less 1 dB"""
    h = product.cfr_lowpass(31, 0.28, 5.65)
    inband, stop = np.linspace(0.0, 0.25, 501), np.linspace(0.32, 0.5, 721)
    g = 20.0 * np.log10(np.abs(model.response(h, inband)))
    ripple = float(g.max() - g.min())
    att = -20.0 * np.log10(float(np.abs(model.response(h, stop)).max()))
    att64 = -20.0 * np.log10(float(np.abs(model.response(model.lowpass(31, 0.28, 5.65), stop)).max()))
    print("cfr low-pass (H = 31, 0.28, 5.65): ripple %.4f dB on |f| <= 0.25; attenuation %.2f dB on |f| >= 0.32 (the formula: %.2f dB)"
          % (ripple, att, att64))
    assert ripple <= 0.1
    assert att >= att64 - 1.0 and att64 > 40.0


# ---------------------------------------------------------------------------------------------- severity of the end-to-end cases
def decode(oracle, s, sent, y):
    """the oracle's receiver on the stream y: (frames, EVMs) with every frame asserted valid and its bytes the ones sent"""
    ora = oracle.MultiChannelRx(s["N"], s["M"], s["cp"], s["taper"])
    ora.execute(np.ascontiguousarray(np.asarray(y).astype(np.complex64)))
    assert len(ora.frames) == s["N"] * s["frames"], len(ora.frames)
    seen = set()
    for f in ora.frames:
        assert f.header_valid and f.payload_valid, f
        pid = (f.header[0] << 8) | f.header[1]
        assert sent[f.channel][pid] == (bytes(f.header), bytes(f.payload)), (f.channel, pid)
        seen.add((f.channel, pid))
    assert len(seen) == s["N"] * s["frames"]
    return [f.evm for f in ora.frames]


def test_severity_on_the_oracle_alone(product, oracle):
    """The oracle's own transmitter through the float64 model at cfr_model.SEVERITY into the oracle's receiver.  Out of band: the
    share of the power at |f| > 0.32, the mean of |FFT|^2 over Hann-windowed segments of 4096 samples overlapping by half
    (cfr_model.spectrum).  With that spectrum the corrected stream holds 3.6 dB MORE there than the clean one (-90.7 against -94.4 dB:
    fp32 taps and 63 of them), so "at most 1 dB above the clean stream's" does not hold and the statement asserted is the other one:
    at least 40 dB below what a hard clip at the same threshold leaves (measured: 65.9 dB below)."""
    s = model.SEVERITY
    iq, sent = oracle.synth_traffic(s["N"], s["M"], s["cp"], s["taper"], s["frames"], payload_len=s["payload_len"])
    rms = model.rms(iq)
    h = product.cfr_lowpass(s["half_len"], s["cutoff"], s["beta"])
    A = float(np.float32(product.cfr_threshold(s["papr_db"], rms)))
    y = model.apply_stream(iq, A, h, s["passes"])
    evm = decode(oracle, s, sent, y)
    papr0, papr1 = model.papr_db(iq), model.papr_db(y)
    oob0, oob1, oobc = model.oob_db(iq, s["edge"]), model.oob_db(y, s["edge"]), model.oob_db(model.hard_clip(iq, A), s["edge"])
    print("cfr severity: %d samples, rms %.4f, A %.4f; PAPR %.2f -> %.2f dB; peak / A %.3f; power at |f| > %.2f: clean %.1f dB, "
          "corrected %.1f dB, hard clip %.1f dB; oracle EVM %.1f .. %.1f dB over %d frames"
          % (len(iq), rms, A, papr0, papr1, float(np.abs(y).max()) / A, s["edge"], oob0, oob1, oobc, min(evm), max(evm), len(evm)))
    assert papr0 - papr1 >= s["papr_gain_db"]
    assert oob1 <= oobc - s["oob_margin_db"]


def test_severity_with_an_amplifier(product, oracle):
    """... and in front of a Rapp amplifier (p = 2) at 6 dB input back-off, the stage at 5 dB over the rms: what the amplifier puts
    at |f| > 0.32 falls by at least 4 dB (measured: 7.2), every frame valid with and without the stage -- at a worse EVM with it."""
    s = model.SEVERITY
    iq, sent = oracle.synth_traffic(s["N"], s["M"], s["cp"], s["taper"], s["frames"], payload_len=s["payload_len"])
    rms = model.rms(iq)
    h = product.cfr_lowpass(s["half_len"], s["cutoff"], s["beta"])
    A = float(np.float32(product.cfr_threshold(s["amp_papr_db"], rms)))
    amp = product.rfchain_config(amplifier=dict(sat=product.rfchain_backoff(s["amp_ibo_db"], rms), smooth=s["amp_smooth"]))
    without = rfchain_model.amplifier(amp, iq.astype(np.complex128))
    with_ = rfchain_model.amplifier(amp, model.apply_stream(iq, A, h, s["passes"]))
    evm0, evm1 = decode(oracle, s, sent, without), decode(oracle, s, sent, with_)
    oob0, oob1 = model.oob_db(without, s["edge"]), model.oob_db(with_, s["edge"])
    print("cfr severity behind the amplifier at %.0f dB back-off: power at |f| > %.2f %.1f dB without the stage, %.1f dB with it; oracle "
          "EVM %.1f .. %.1f dB without, %.1f .. %.1f dB with" % (s["amp_ibo_db"], s["edge"], oob0, oob1, min(evm0), max(evm0), min(evm1), max(evm1)))
    assert oob0 - oob1 >= s["amp_oob_gain_db"]
