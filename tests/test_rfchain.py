"""RF front end (mcrx_hip_rfchain_*), what needs no GPU: the boundary -- symbols, null handles, every configuration error reported
before a device is looked for -- the oscillator's integers against the model's own derivation, the statistics of the phase the model
makes of them, the amplifier's and the mixer's textbook figures, the host program of the configuration check, and the severity of the
end-to-end case of tests/test_gpu_rfchain.py found on the oracle alone."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import chanemu_model
import rfchain_model as model
import tx_sc16_model as q16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mcrx_hip_rfchain_clipped", "mcrx_hip_rfchain_create", "mcrx_hip_rfchain_destroy", "mcrx_hip_rfchain_execute_device",
           "mcrx_hip_rfchain_input_format", "mcrx_hip_rfchain_last_error", "mcrx_hip_rfchain_output_format",
           "mcrx_hip_rfchain_phase_rows", "mcrx_hip_rfchain_selftest"]


# ---------------------------------------------------------------------------------------------- the boundary
def test_symbols_are_declared_exported_and_bound(product):
    text = open(os.path.join(ROOT, "include", "mcrx_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(mcrx_hip_rfchain_[a-z_0-9]+)\s*\(", text))) == SYMBOLS
    assert [s for s in product.exported_symbols() if s.startswith("mcrx_hip_rfchain_")] == SYMBOLS
    L = product.lib()
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None
    # 5 + 6 + 3 + 1 words, padding to the double, double, uint64, 5 words, tail padded to 8
    assert C.sizeof(product.RfchainConfig) == 4 * 15 + 4 + 8 + 8 + 4 * 5 + 4 == 104
    assert (product.RFCHAIN_MIXER, product.RFCHAIN_OSCILLATOR, product.RFCHAIN_AMPLIFIER) == (1, 2, 4)
    for name, val in (("MIXER", "1u"), ("OSCILLATOR", "2u"), ("AMPLIFIER", "4u")):
        assert re.search(r"#define MCRX_RFCHAIN_%s\s+%s" % (name, val), text)


def test_null_handles_are_answered(product):
    L = product.lib()
    assert L.mcrx_hip_rfchain_input_format(None) == 0 and L.mcrx_hip_rfchain_output_format(None) == 0
    assert L.mcrx_hip_rfchain_destroy(None) == product.MCRX_OK
    n = C.c_uint64(7)
    for rc in (L.mcrx_hip_rfchain_clipped(None, C.byref(n), 0), L.mcrx_hip_rfchain_execute_device(None, None, 0, 0, None, None),
               L.mcrx_hip_rfchain_create(None, None), L.mcrx_hip_rfchain_phase_rows(None, 0, 1, None, None),
               L.mcrx_hip_rfchain_selftest(None, None, None, None)):
        assert rc == product.MCRX_EINVAL
    assert L.mcrx_hip_rfchain_last_error()
    h = C.c_void_p(0x1234)
    assert L.mcrx_hip_rfchain_create(C.byref(h), None) == product.MCRX_EINVAL and not h.value


GOOD = dict(order="rx", mixer=dict(alpha=1.0, beta=0.05j, dc=0.01), phase_noise=dict(rms_deg=1.0, bandwidth=1e-5, seed=5),
            amplifier=dict(sat=0.5, smooth=2, gain=1.0, ampm_deg=5.0), gain=0.9, input_format="sc16", output_format="sc16")


def good_config(product):
    return product.rfchain_config(**GOOD)


NAN, INF = float("nan"), float("inf")
BAD = [("struct_size", "struct_size", 100), ("order", "order", 2), ("stage bits", "stages", 8), ("input format", "input_format", 2),
       ("output format", "output_format", 2), ("gain", "gain", INF), ("alpha nan", "alpha_im", NAN), ("dc inf", "dc_re", INF),
       ("no sinusoids", "pn_sinusoids", 0), ("17 sinusoids", "pn_sinusoids", 17), ("L 0", "pn_log2_block", 0), ("L 25", "pn_log2_block", 25),
       ("one row", "pn_table_rows", 1), ("rms negative", "pn_rms", -0.01), ("rms nan", "pn_rms", NAN), ("rms inf", "pn_rms", INF),
       ("bandwidth negative", "pn_bandwidth", -1e-6), ("bandwidth nan", "pn_bandwidth", NAN), ("bandwidth inf", "pn_bandwidth", INF),
       ("bandwidth * B > 1/8", "pn_bandwidth", 0.1251 / 1024), ("rms sqrt(2S) >= pi/2", "pn_rms", math.pi / 2 / math.sqrt(32.0) * 1.0001),
       ("smooth 3", "amp_smooth", 3), ("smooth 0", "amp_smooth", 0), ("sat 0", "amp_sat", 0.0), ("sat negative", "amp_sat", -1.0),
       ("sat nan", "amp_sat", NAN), ("amp gain", "amp_gain", INF), ("ampm nan", "amp_ampm", NAN), ("ampm large", "amp_ampm", 0.3)]


@pytest.mark.parametrize("what,field,value", BAD, ids=[b[0] for b in BAD])
def test_configuration_errors_come_before_the_device(product, what, field, value):
    L = product.lib()
    c = good_config(product)
    setattr(c, field, value)
    h = C.c_void_p(0x1234)
    assert L.mcrx_hip_rfchain_create(C.byref(h), C.addressof(c)) == product.MCRX_EINVAL, what
    assert not h.value                                                                     # *out is cleared
    assert L.mcrx_hip_rfchain_last_error()
    if field.startswith("pn_") or field == "struct_size":                                  # the selftest checks as create does
        steps, phases, coef = (C.c_int64 * 16)(), (C.c_uint32 * 16)(), C.c_float()
        assert L.mcrx_hip_rfchain_selftest(C.addressof(c), steps, phases, C.byref(coef)) == product.MCRX_EINVAL


def test_the_limits_themselves_are_accepted(product):
    """on the allowed side of every bound the answer is a handle, or 'no device' here -- never MCRX_EINVAL"""
    L = product.lib()
    edits = [("pn_bandwidth", 0.125 / 1024), ("pn_rms", math.pi / 2 / math.sqrt(32.0) * 0.999), ("pn_sinusoids", 1), ("pn_log2_block", 24),
             ("pn_table_rows", 2), ("amp_ampm", -0.25), ("amp_smooth", 4), ("pn_rms", 0.0), ("pn_bandwidth", 0.0)]
    for field, value in edits:
        c = good_config(product)
        if field == "pn_log2_block":
            c.pn_bandwidth = 0.0
        setattr(c, field, value)
        h = C.c_void_p()
        rc = L.mcrx_hip_rfchain_create(C.byref(h), C.addressof(c))
        assert rc in (product.MCRX_OK, product.MCRX_EHIP), (field, L.mcrx_hip_rfchain_last_error())
        if rc == product.MCRX_OK:
            assert L.mcrx_hip_rfchain_input_format(h) == 1 and L.mcrx_hip_rfchain_output_format(h) == 1
            L.mcrx_hip_rfchain_destroy(h)
    # a stage that is off is not looked at
    c = product.rfchain_config()
    c.pn_sinusoids, c.amp_smooth, c.alpha_re = 99, 3, NAN
    h = C.c_void_p()
    assert L.mcrx_hip_rfchain_create(C.byref(h), C.addressof(c)) in (product.MCRX_OK, product.MCRX_EHIP)
    if h.value:
        L.mcrx_hip_rfchain_destroy(h)


PY_BAD = [dict(order="up"), dict(order=0), dict(input_format="sc8"), dict(output_format=2), dict(gain=INF), dict(mixer=dict(alpha=1.0)),
          dict(mixer=dict(alpha=1.0, beta=0.0, lo=0.1)), dict(mixer=(1.0, 0.0)), dict(mixer=dict(alpha=complex(NAN, 0), beta=0.0)),
          dict(phase_noise=dict(rms_deg=1.0)), dict(phase_noise=dict(rms_deg=1.0, bandwidth=1e-5, sinusoids=17)),
          dict(phase_noise=dict(rms_deg=1.0, bandwidth=1e-5, sinusoids=2.5)), dict(phase_noise=dict(rms_deg=1.0, bandwidth=1e-5, log2_block=0)),
          dict(phase_noise=dict(rms_deg=1.0, bandwidth=1e-5, log2_block=-1)), dict(phase_noise=dict(rms_deg=1.0, bandwidth=1e-5, table_rows=1)),
          dict(phase_noise=dict(rms_deg=-1.0, bandwidth=1e-5)), dict(phase_noise=dict(rms_deg=1.0, bandwidth=-1e-5)),
          dict(phase_noise=dict(rms_deg=1.0, bandwidth=1e-3)), dict(phase_noise=dict(rms_deg=20.0, bandwidth=1e-5)),
          dict(amplifier=dict(smooth=2)), dict(amplifier=dict(sat=0.0)), dict(amplifier=dict(sat=1.0, smooth=3)),
          dict(amplifier=dict(sat=1.0, gain=INF)), dict(amplifier=dict(sat=1.0, ampm_deg=120.0)), dict(amplifier=dict(sat=1.0, p=2))]


@pytest.mark.parametrize("kw", PY_BAD, ids=[str(i) for i in range(len(PY_BAD))])
def test_python_class_raises_value_error_without_a_device(product, kw):
    with pytest.raises(ValueError):
        product.rfchain(**kw)
    with pytest.raises(ValueError):
        product.rfchain_iq(1.0, 5.0, side="both")


def test_host_program_of_the_configuration_check(product):
    """host/rfchain_plan_test.cc: csrc/rfchain_plan.hpp with a main of its own (no GPU, no Python)"""
    host = os.path.join(ROOT, "liquid-usrp_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "rfchain_plan_test"])
    out = subprocess.run([os.path.join(ROOT, "liquid-usrp_amd", "lib", "rfchain_plan_test")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0 and b"rfchain_plan_test ok" in out.stdout, out.stdout.decode()


# ---------------------------------------------------------------------------------------------- the oscillator's integers
SEEDS = [0, 0x1234567, 0xC0FFEE0123456789]                # one above 2^32: the key's second word


@pytest.mark.parametrize("seed", SEEDS)
def test_selftest_integers_equal_the_model(product, seed):
    for S, L, bw, rms_deg in ((16, 10, 1e-5, 1.0), (1, 1, 0.0625, 3.0), (7, 24, 7e-9, 0.25), (16, 6, 0.125 / 64, 2.0)):
        c = product.rfchain_config(phase_noise=dict(rms_deg=rms_deg, bandwidth=bw, sinusoids=S, log2_block=L, seed=seed))
        steps, phases, coef = product.rfchain_integers(c)
        want = model.integers(seed, S, L, bw, math.radians(rms_deg))
        assert (steps, phases) == (want[0], want[1]), (S, L)
        assert coef == want[2]
        B = 1 << L
        assert all(abs(n) * B <= 2 ** 61 for n in steps)                                   # every |f_k| B <= 1/8
        if bw * B == 0.125:
            assert sum(abs(n) * B == 2 ** 61 for n in steps) >= S // 4                     # ... and the widest line reaches the clamp
    # the stratum of sinusoid k: u_k in [k / S, (k + 1) / S), so the steps ascend with k
    steps = product.rfchain_integers(product.rfchain_config(phase_noise=dict(rms_deg=1.0, bandwidth=1e-6, seed=seed)))[0]
    assert steps == sorted(steps) and steps[0] < 0 < steps[-1]


def test_seeds_differ(product):
    a, b = (product.rfchain_integers(product.rfchain_config(phase_noise=dict(rms_deg=1.0, bandwidth=1e-5, seed=s))) for s in (1, 2))
    assert a[0] != b[0] and a[1] != b[1] and a[2] == b[2]


def test_theta_rms():
    """E theta^2 = c^2 S / 2 = (pn_rms / 2 pi)^2 turns^2 on the grid rows (phases uniform and independent).  Sampling error: over R seeds
    theta^2 at one row is R independent draws with E theta^4 = c^4 (3 S^2 / 4 - 3 S / 8), so the mean of theta^2 has the relative
    standard deviation sqrt(2 - 3 / (2 S)) / sqrt(R), and the rms half of it.  J rows per seed only lower the variance (they are
    correlated draws of the same law), so the bound from R alone holds; four standard deviations are asserted."""
    S, L, R, J, rms = 16, 10, 400, 32, math.radians(1.0)
    rows = (np.arange(J, dtype=np.uint64) * np.uint64(2 ** 37 + 12345)) + np.uint64(3)
    acc = 0.0
    for seed in range(R):
        th = model.theta_rows(model.integers(1000 + seed, S, L, 1e-5, rms), L, rows)
        acc += float(np.mean(th * th))
    got = 2.0 * math.pi * math.sqrt(acc / R)
    sigma = 0.5 * math.sqrt(2.0 - 1.5 / S) / math.sqrt(R)
    print("theta rms %.5f rad, configured %.5f: off by %.2f %% (one sigma %.2f %%)" % (got, rms, 100 * (got / rms - 1), 100 * sigma))
    assert abs(got / rms - 1.0) <= 4.0 * sigma
    # between the rows the angle is the straight line of the definition
    ints = model.integers(5, S, 4, 1e-3, rms)
    th = model.theta(ints, 4, np.arange(64, dtype=np.uint64) + np.uint64(2 ** 40))
    T = model.theta_rows(ints, 4, (np.arange(5, dtype=np.uint64) + np.uint64(2 ** 36)))
    assert np.allclose(th[::16], T[:4], rtol=0, atol=1e-15) and np.allclose(th[8::16], 0.5 * (T[:4] + T[1:5]), rtol=0, atol=1e-15)
    assert float(np.abs(th).max()) < 0.25


# ---------------------------------------------------------------------------------------------- amplifier and mixer
@pytest.mark.parametrize("p", [1, 2, 4])
def test_rapp_curve(product, p):
    A, g = 0.37, 1.3
    c = product.rfchain_config(amplifier=dict(sat=A, smooth=p, gain=g))
    z = float(c.amp_sat) * np.exp(1j * np.array([0.0, 1.0, 2.5]))
    u = model.amplifier(c, z)
    assert np.allclose(np.abs(u) / np.abs(z), float(c.amp_gain) * 2.0 ** (-1.0 / (2 * p)), rtol=2e-7, atol=0)      # (fp32(1 / A^2): 6e-8)
    assert np.allclose(np.angle(u / z), 0.0, atol=1e-15)                                                             # no AM/PM
    small, large = model.amplifier(c, np.array([1e-3 * A + 0j])), model.amplifier(c, np.array([1e3 * A + 0j]))
    assert abs(abs(small[0]) / (1e-3 * A) / float(c.amp_gain) - 1.0) < 1e-6                                           # linear below ...
    assert abs(abs(large[0]) / (float(c.amp_gain) * float(c.amp_sat)) - 1.0) < 1e-5                                   # ... saturated above
    # AM/PM: half of ampm at |z| = A, all of it far above
    c = product.rfchain_config(amplifier=dict(sat=A, smooth=p, gain=g, ampm_deg=10.0))
    u = model.amplifier(c, np.array([float(c.amp_sat) + 0j, 1e4 * A + 0j]))
    assert np.allclose(np.degrees(np.angle(u)), [5.0, 10.0], rtol=1e-6)
    assert product.rfchain_backoff(6.0, 0.25) == 0.25 * 10.0 ** 0.3


def test_iq_helper(product):
    for gain_db, phase_deg in ((0.5, 3.0), (1.0, 5.0), (-0.3, -2.0)):
        g, phi = 10.0 ** (gain_db / 20.0), math.radians(phase_deg)
        irr = (1 + 2 * g * math.cos(phi) + g * g) / (1 - 2 * g * math.cos(phi) + g * g)    # the textbook image rejection
        for side in ("tx", "rx"):
            m = product.rfchain_iq(gain_db, phase_deg, side)
            assert abs(abs(m["alpha"]) ** 2 / abs(m["beta"]) ** 2 / irr - 1.0) < 1e-12, side
        tx, rx = product.rfchain_iq(gain_db, phase_deg, "tx"), product.rfchain_iq(gain_db, phase_deg, "rx")
        assert tx["beta"] == rx["beta"] and tx["alpha"] == rx["alpha"].conjugate()
        # a modulator: I arm cos, Q arm g sin(. + phi) -> the baseband equivalent of re + j g e^{j phi} im
        z = 0.3 - 0.8j
        assert abs(tx["alpha"] * z + tx["beta"] * z.conjugate() - (z.real + 1j * g * complex(math.cos(phi), math.sin(phi)) * z.imag)) < 1e-15
    m = product.rfchain_iq(0.0, 0.0)
    assert m["alpha"] == 1.0 and m["beta"] == 0.0
    # the image of channel c lies in channel N - 1 - c: the centres are symmetric
    N = 8
    om = product.monitor_omega(N, 64, np.arange(N), 0)
    assert np.allclose(om, -om[::-1])


# ---------------------------------------------------------------------------------------------- severity of the end-to-end case
def test_severity_on_the_oracle_alone(product, oracle):
    """The oracle's own transmitter through the float64 model of both chains, noise from chanemu_model between them, sc16 out of the
    receive chain, into oracle.MultiChannelRx: all 24 frames valid at rfchain_model.SEVERITY, the values the GPU end-to-end test uses."""
    s = model.SEVERITY
    N, M, cp, taper, nf, plen = s["N"], s["M"], s["cp"], s["taper"], s["frames"], s["payload_len"]
    iq, sent = oracle.synth_traffic(N, M, cp, taper, nf, payload_len=plen)
    rms = float(np.sqrt(np.mean(np.abs(iq.astype(np.complex128)) ** 2)))
    txk, rxk = model.severity_chains(product, rms)
    ctx = product.rfchain_config(**txk)
    y = model.apply(ctx, iq, 0, product.rfchain_integers(ctx)).astype(np.complex64)
    power = float(np.mean(np.abs(y.astype(np.complex128)) ** 2))
    nstd = float(np.float32(math.sqrt(power / 10.0 ** (s["snr_db"] / 10.0) / 2.0)))
    y = chanemu_model.apply(y, [(0, 1.0)], noise_std=nstd, seed=s["noise_seed"]).astype(np.complex64)
    crx = product.rfchain_config(**rxk)
    v = model.apply(crx, y, 0, product.rfchain_integers(crx))
    g = float(np.float32(s["peak"] / max(np.abs(v.real).max(), np.abs(v.imag).max())))
    crx = product.rfchain_config(gain=g, output_format="sc16", **rxk)
    v = model.apply(crx, y, 0, product.rfchain_integers(crx)).astype(np.complex64)
    assert q16.clipped_samples(v) == 0
    ints = q16.quantise_iq(v)
    y_host = (ints.astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64).reshape(-1)
    ora = oracle.MultiChannelRx(N, M, cp, taper)
    ora.execute(np.ascontiguousarray(y_host))
    assert len(ora.frames) == N * nf, len(ora.frames)
    seen = set()
    for f in ora.frames:
        assert f.header_valid and f.payload_valid, f
        pid = (f.header[0] << 8) | f.header[1]
        assert sent[f.channel][pid] == (bytes(f.header), bytes(f.payload)), (f.channel, pid)
        seen.add((f.channel, pid))
    assert len(seen) == N * nf
    evm = [f.evm for f in ora.frames]
    print("severity: rms %.4f, A %.4f, noise_std %.5f, rx gain %.3f; oracle EVM %.1f .. %.1f dB over %d frames"
          % (rms, float(ctx.amp_sat), nstd, g, min(evm), max(evm), len(evm)))
