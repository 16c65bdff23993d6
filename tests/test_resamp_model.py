"""The resampler without a GPU: the plan msresamp_hip_selftest returns (csrc/resamp_plan.hpp) at the rate edges
and its refusals, the taps against an independent float64 Kaiser design, the float64 model of tests/resamp_model.py against the
oracle, and the delay the plan states against the delay a tone shows.  host/resamp_plan_test.cc runs the same plan as a program of its
own, plain and under the address and undefined-behaviour sanitizers."""
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.special

import resamp_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "liquid-usrp_amd", "host")
LIB = os.path.join(ROOT, "liquid-usrp_amd", "lib")

PARITY_RATES = [0.5, 0.37, 0.8, 0.2, 0.11, 2.0, 1.5, 4.0, 6.3, 0.25, 0.45, 0.06]       # tests/test_gpu_parity.py's twelve
F32 = np.float32
LEAST = 2.0 ** -38                                                                      # 37 half-band decimators: resamp_plan.hpp
EDGES = {
    "0.5": (0.5, dict(interp=False, num_stages=0, step=1 << 25, per_in=2, per_out=1)),
    "0.5-": (float(np.nextafter(F32(0.5), F32(0))), dict(interp=False, num_stages=1, step=(1 << 24) + 1, per_in=(1 << 24) + 1, per_out=1 << 24)),
    "1": (1.0, dict(interp=False, num_stages=0, step=1 << 24, per_in=1, per_out=1)),
    "1+": (float(np.nextafter(F32(1), F32(2))), dict(interp=True, num_stages=0, step=(1 << 24) - 2, per_in=(1 << 23) - 1, per_out=1 << 23)),
    "2": (2.0, dict(interp=True, num_stages=0, step=1 << 23, per_in=1, per_out=2)),
    "2+": (float(np.nextafter(F32(2), F32(3))), dict(interp=True, num_stages=1, step=(1 << 24) - 2, per_in=(1 << 23) - 1, per_out=1 << 23)),
    "1024": (1024.0, dict(interp=True, num_stages=9, step=1 << 23, per_in=1, per_out=2)),
    "least": (LEAST, dict(interp=False, num_stages=37, step=1 << 25, per_in=2, per_out=1)),
    "0.8": (0.8, dict(interp=False, num_stages=0, step=5 << 22, per_in=5, per_out=4)),
    # 16/25 is no float: the float nearest 0.64 is 0.63999998569..., 2^24 over it 26214400.59
    "0.64": (0.64, dict(interp=False, num_stages=0, step=26214401, per_in=26214401, per_out=1 << 24)),
}
ORACLE_FIGURES = {}


def kaiser64(n, fc, As=60.0):
    """liquid's Kaiser design in float64 (the window over n, not n - 1, as tests/test_oracle_dsp.py states it)"""
    beta = 0.1102 * (As - 8.7)
    t = np.arange(n) - (n - 1) / 2.0
    w = scipy.special.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (2.0 * t / n) ** 2))) / scipy.special.i0(beta)
    return np.sinc(2.0 * fc * t) * w


@pytest.mark.parametrize("name", sorted(EDGES))
def test_plan_at_the_rate_edges(product, name):
    rate, want = EDGES[name]
    p = product.msresamp_plan(rate)
    assert {k: getattr(p, k) for k in want} == want
    rate = float(F32(rate))                         # the library's rate is a float
    assert p.rate_arb == (rate / 2.0 ** p.num_stages if p.interp else rate * 2.0 ** p.num_stages)
    assert p.per_in << 24 == p.per_out * p.step
    assert p.step == int(np.rint(2.0 ** 24 / p.rate_arb))
    assert p.h1.shape == (14,) and p.hpfb.shape == (256, 14) and p.h1.dtype == np.float32 and p.hpfb.dtype == np.float32
    if not p.interp:
        d = 7.0
        for _ in range(p.num_stages):
            d = 2.0 * d + 13.0
        assert p.delay == float(F32(d))
    else:
        assert p.delay == float(F32(7.0 + 7.0 / p.rate_arb * (2.0 - 2.0 ** (1 - p.num_stages))))


def test_plan_period_at_every_rate(product):
    for rate in PARITY_RATES + [0.001, 1.0 / 65536, 16.0, 100.0, 0.7, 0.999, 1.25]:
        p = product.msresamp_plan(rate)
        assert p.per_in << 24 == p.per_out * p.step and (p.per_in | p.per_out) & 1, rate
        assert (0.5 <= p.rate_arb <= 1.0) if not p.interp else (1.0 < p.rate_arb <= 2.0), rate


@pytest.mark.parametrize("rate", [0.0, -1.0, float("nan"), float(np.nextafter(F32(1024), F32(2048))), 2000.0, float("inf"),
                                  float(np.nextafter(F32(LEAST), F32(0))), 1e-20])
def test_refused_rates(product, rate):
    """before any HIP call: a ValueError on a machine without a device too, from the plan and from create alike"""
    for make in (product.msresamp_plan, product.msresamp):
        with pytest.raises(ValueError) as ei:
            make(rate)
        assert "2^-38" in str(ei.value) and "1024" in str(ei.value)
    if 0 < rate < LEAST:
        with pytest.raises(ValueError) as ei:
            product.msresamp_plan(rate)
        assert "37" in str(ei.value)


def test_least_rate_is_accepted(product):
    assert product.msresamp_plan(LEAST).num_stages == 37
    assert product.msresamp_plan(float(np.nextafter(F32(LEAST), F32(1)))).num_stages == 37


@pytest.mark.parametrize("rate", [0.5, 0.37, 0.8, 1.0, 1.5, 2.0, 6.3, 0.06, 1024.0])
def test_taps_against_an_independent_design(product, rate):
    p = product.msresamp_plan(rate)
    fc = F32(0.515) * F32(p.rate_arb)
    fc = min(fc, F32(0.49))
    proto = kaiser64(2 * 7 * 256 + 1, float(F32(fc) / F32(256)))
    proto *= 256.0 / proto.sum()
    want = proto[:14 * 256].reshape(14, 256).T[:, ::-1]                 # H[b][13 - k] = proto[b + 256 k]
    assert np.max(np.abs(p.hpfb - want)) < 2e-6
    dc = p.hpfb.astype(np.float64).sum(axis=1)
    assert np.all(np.abs(dc - 1.0) <= 1e-3), (dc.min(), dc.max())
    hb = kaiser64(29, 0.25)
    assert np.max(np.abs(p.h1 - hb[27::-2])) < 2e-6                      # the odd taps, reversed
    assert np.array_equal(p.h1, p.h1[::-1])
    assert abs(float(p.h1.astype(np.float64).sum()) - 1.0) <= 2e-3


def noise_len(rate):
    return max(16384, int(300 / rate)) if rate <= 1 else max(200, int(16384 / rate))


@pytest.mark.parametrize("rate", PARITY_RATES + [0.001, 100.0, 1024.0])
def test_model_against_oracle(oracle, product, rate):
    """The oracle computes in fp32, sequentially and without fused multiply-adds: within the derived bound of the model, component by
    component (a), and within REL of its peak in max-norm (b)."""
    p = product.msresamp_plan(rate)
    rng = np.random.RandomState(int(rate * 1000) + 7)
    n = noise_len(rate)
    x = (rng.randn(n) + 1j * rng.randn(n)).astype(np.complex64)
    got = oracle.MsResamp(rate).execute(x)
    y, bound = model.run(p, x)
    assert len(got) == len(y) == model.count_out(p, n) and len(y) >= 64
    frac, rel = model.compare(got, y, bound)
    ORACLE_FIGURES["%g" % rate] = {"bound_fraction": frac, "max_norm": rel}
    print("model against oracle, rate %g: %.3f of the bound, max-norm %.2e of the peak" % (rate, frac, rel))
    assert frac <= 1.0
    assert rel <= model.REL


@pytest.mark.parametrize("rate", PARITY_RATES + [16.0, 100.0])
def test_true_delay(product, rate):
    """The delay the plan states (get_delay(), input samples) is the delay a slow tone shows."""
    p = product.msresamp_plan(rate)
    x, f_in = model.delay_tone(p)
    y, _ = model.run(p, x)
    D = model.fit_delay(p, y, f_in)
    print("rate %g: delay %.4f input samples (%.2f output samples), the plan says %.4f" % (rate, D, D * model.true_rate(p), p.delay))
    assert abs(p.delay - D) <= model.delay_tolerance(p)


@pytest.mark.parametrize("rate", PARITY_RATES + [16.0, 100.0, 0.001, 1024.0])
def test_oracle_delay_is_the_plans(oracle, product, rate):
    assert oracle.MsResamp(rate).get_delay() == product.msresamp_plan(rate).delay


def test_model_is_causal_and_counts_its_outputs(product):
    """what the GPU tests rely on when they compare a shorter call with the head of a longer one's model"""
    rng = np.random.RandomState(5)
    x = (rng.randn(3000) + 1j * rng.randn(3000)).astype(np.complex64)
    for rate in (0.37, 0.11, 1.5, 6.3):
        p = product.msresamp_plan(rate)
        y, b = model.run(p, x)
        for n in (0, 1, 7, 999, 2048):
            yn, bn = model.run(p, x[:n])
            assert np.array_equal(yn, y[:len(yn)]) and np.array_equal(bn, b[:len(bn)])
        for nout in (1, 255, 1024, 1025):
            n = model.nin_for(p, nout)
            assert model.count_out(p, n) >= nout and (n == 0 or model.count_out(p, n - 1) < nout)


def test_host_program_plain_and_sanitized():
    """host/resamp_plan_test.cc, with its own main: plain, and under the address and undefined-behaviour sanitizers"""
    for args, exe in (([], "resamp_plan_test"), (["SAN=1"], "resamp_plan_test_san")):
        subprocess.check_call(["make", "-C", HOST, "-s", "resamp_plan_test"] + args)
        out = subprocess.run([os.path.join(LIB, exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert out.returncode == 0 and b"resamp_plan_test ok" in out.stdout, out.stdout.decode(errors="replace")


def test_zz_print_oracle_figures():
    """(last of this file: the figures measured above as one JSON line -- profiles/resamp_model_oracle.json is such a record;
    RESAMP_ORACLE_OUT names a file to write it to as well)"""
    line = json.dumps(ORACLE_FIGURES, sort_keys=True)
    print("resamp_model_oracle " + line)
    path = os.environ.get("RESAMP_ORACLE_OUT")
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")
