"""Amplifier with memory on the MI355X (mcrx_hip_pamem_*) against tests/pamem_model.py: one branch with a unit tap is rfchain's amplifier;
the float64 model within the rounding bound it derives, at the kernel's own edges; cuts that carry their leads and the four format
pairs bit for bit; the shared quantiser and clip count; the refusals; the linear regime as the FIR of pamem_small_signal; the torch
stand-in of tests/test_gpu_mpd.py beside it; and that test's closed loop with this operator as the amplifier."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cfr_model
import mpd_model
import pamem_model as model
import tx_sc16_model as q16
from test_gpu_dpd import SENTINEL_WORD, _torch, bits, dev, host, nmse_of, oob_of, placed, rms_of, words

pytestmark = pytest.mark.gpu

RATIOS, PARITY = {}, {}
EPS, SQ2 = model.EPS, model.SQ2
SPAN = 2048                                                 # outputs of one workgroup: pamem_rounds() rounds of 512 (csrc/pamem_plan.hpp)
FORMATS = [("cf32", "cf32"), ("cf32", "sc16"), ("sc16", "cf32"), ("sc16", "sc16")]


def worst(got, want, bound):
    """the largest error of a component as a fraction of the sample's bound [n] (a sample whose bound is zero must be exact: 0 <= 0)"""
    d = np.asarray(got, np.complex128) - want
    tiny = np.finfo(np.float32).tiny
    return float(np.max(np.maximum(np.abs(d.real), np.abs(d.imag)) / np.maximum(bound, tiny)))


def to_sc16(x):
    """complex samples as int16 [n, 2] through the shared quantiser: an sc16 stream"""
    return q16.quantise_iq(np.asarray(x, np.complex64))


def from_sc16(i):
    """the cf32 samples an sc16 stream means: (re, im) * 2^-15, exact"""
    return (i.astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64).reshape(-1)


def placed16(i, shift):
    """the sc16 samples i [n, 2] on the device, beginning `shift` samples (4 bytes each) behind a 16-byte boundary"""
    torch = _torch()
    buf = torch.zeros((len(i) + 4, 2), dtype=torch.int16, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[shift:shift + len(i)].copy_(torch.from_numpy(np.ascontiguousarray(i)).cuda())
    return buf[shift:shift + len(i)]


def put(x, shift, in16):
    return placed16(x, shift) if in16 else placed(x, shift)


def drive(n, sat, seed, top=30.0):
    """amplitudes from 1e-3 sat to `top` sat (log-uniform), the four corners first, any phase: complex64"""
    rng = np.random.RandomState(seed)
    amp = sat * 10.0 ** rng.uniform(-3.0, np.log10(top), n)
    k = min(n, 4)
    amp[:k] = (sat * np.array([1e-3, top, 1.0, 0.0]))[:k]
    return (amp * np.exp(2j * np.pi * rng.uniform(size=n))).astype(np.complex64)


# ---------------------------------------------------------------------------------------------- 1. one branch is rfchain's amplifier
@pytest.mark.parametrize("ampm_deg", [0.0, 5.0])
@pytest.mark.parametrize("smooth", [1, 2, 4])
def test_one_branch_is_the_amplifier_of_rfchain(product, smooth, ampm_deg):
    """B = 1 with the tap (0, 1): the numbers of the amplifier-only rfchain handle on the same input, amplitudes 1e-3 A .. 30 A, for
    the four format pairs (np.array_equal: the sign of a zero may differ); A = 0.03 keeps 30 A inside an sc16 input"""
    sat, n = 0.03, 4099
    x = drive(n, sat, seed=smooth)
    amp = dict(sat=sat, smooth=smooth, gain=1.25, ampm_deg=ampm_deg)
    for fin, fout in FORMATS:
        a = product.rfchain(amplifier=amp, input_format=fin, output_format=fout)
        b = product.pamem([dict(amp, taps=[(0, 1.0)])], input_format=fin, output_format=fout)
        assert b.lead == 0
        src = to_sc16(x) if fin == "sc16" else x
        for shift in (0, 1):
            xd = put(src, shift, fin == "sc16")
            ya, yb = host(a.execute(xd)), host(b.execute(xd))
            assert ya.shape == yb.shape and ya.dtype == yb.dtype and len(ya) == n
            assert np.array_equal(ya, yb), (fin, fout, shift, np.nonzero(ya != yb)[0][:8])
            assert np.all(np.isfinite(ya.astype(np.float64) if fout == "sc16" else ya.view(np.float32)))
        assert a.clipped() == b.clipped()
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 2. the float64 model
def shape(product, name):
    """branch lists around the kernel's edges: every B, tap counts 1, 3 and 8, delays 0, 1, 15, 16, lead 0, an odd lead"""
    rng = np.random.RandomState(len(name))

    def w(k):
        return complex(np.round(0.3 * (rng.standard_normal() + 1j * rng.standard_normal()), 3)) * 0.5 ** (k > 0)
    A = dict(sat=0.5, smooth=2, gain=1.1, ampm_deg=5.0)
    Bb = dict(sat=0.35, smooth=1, gain=0.9, ampm_deg=-8.0)
    Cc = dict(sat=0.7, smooth=4, gain=1.0, ampm_deg=0.0)
    Dd = dict(sat=0.4, smooth=2, gain=-0.8, ampm_deg=3.0)
    return {"B1_T1_lead0": [dict(A, taps=[(0, 1.0)])],
            "B1_T1_lead16": [dict(A, taps=[(16, 1.0)])],
            "B2_T3_T1_lead16": [dict(A, taps=[(0, 1.0), (1, w(1)), (16, w(2))]), dict(Bb, taps=[(15, w(3))])],
            "B2_T1_T1_lead15": [dict(A, taps=[(0, 1.0)]), dict(Bb, taps=[(15, w(1))])],
            "B3_T1_T3_T8_lead16": [dict(A, taps=[(1, 1.0)]), dict(Bb, taps=[(0, w(1)), (2, w(2)), (15, 0.0)]),
                                   dict(Cc, taps=[(d, w(d)) for d in (0, 1, 2, 3, 5, 8, 13, 16)])],
            "B4_T8_lead16": [dict(A, taps=[(d, w(d)) for d in range(8)]), dict(Bb, taps=[(d, w(d)) for d in range(1, 16, 2)]),
                             dict(Cc, taps=[(d, w(d)) for d in range(0, 16, 2)]), dict(Dd, taps=[(d, w(d)) for d in range(9, 17)])],
            "B4_T1_lead3": [dict(A, taps=[(0, 1.0)]), dict(Bb, taps=[(1, w(1))]), dict(Cc, taps=[(2, w(2))]), dict(Dd, taps=[(3, w(3))])]}[name]


SHAPES = ["B1_T1_lead0", "B1_T1_lead16", "B2_T3_T1_lead16", "B2_T1_T1_lead15", "B3_T1_T3_T8_lead16", "B4_T8_lead16", "B4_T1_lead3"]


def sizes(lead):
    return sorted(set(n for n in (1, 2, lead, lead + 1, 255, 256, 257, 511, 512, 513, 1025, SPAN - 1, SPAN, SPAN + 1) if n > 0))


@pytest.mark.parametrize("gain", [1.0, 0.37])
@pytest.mark.parametrize("name", SHAPES)
def test_apply_against_the_model(product, name, gain):
    """every n at which the kernel takes another path -- one lane, one pair, the history alone, a wave, a round of 512 and one more, one
    workgroup's span of 2048 outputs less one, exactly, and one more -- from input buffers that are 16-byte aligned and 8-byte but not
    16-byte aligned: (a) every component within the model's bound, (b) the max-norm within 1e-5 of the peak.  The operator is
    time-invariant, so the model of the longest input serves every n: the outputs of a prefix are a prefix of the outputs."""
    branches = shape(product, name)
    d = product.pamem(branches, gain=gain)
    lead = d.lead
    assert lead == model.lead_of(d.config)
    x = drive(lead + SPAN + 1, 0.5, seed=lead + len(branches), top=10.0)
    want, bound = model.apply(d.config, x)
    peak = np.abs(want).max()
    for n in sizes(lead):
        for shift in (0, 1):
            xd = placed(x[:lead + n], shift)
            assert (xd.data_ptr() % 16 == 0) == (shift == 0)
            got = host(d.execute(xd, pad=False))
            assert got.shape == (n,)
            w = worst(got, want[:n], bound[:n])
            RATIOS[name] = max(RATIOS.get(name, 0.0), w)
            assert w <= 1.0, (n, shift, w)
            assert np.abs(got - want[:n]).max() <= 1e-5 * peak, (n, shift)
    print("pamem apply %s, gain %.2f: worst error is %.3f of the rounding bound" % (name, gain, RATIOS[name]))
    d.close()


def test_a_model_broken_on_purpose_is_caught(product):
    """one tap's delay off by one in the model: the bound of (a) is exceeded, so (a) is a test of where the taps lie"""
    branches = shape(product, "B3_T1_T3_T8_lead16")
    d = product.pamem(branches)
    x = drive(d.lead + 513, 0.5, seed=9, top=10.0)
    got = host(d.execute(dev(x), pad=False))
    want, bound = model.apply(d.config, x)
    assert worst(got, want, bound) <= 1.0
    for tap in (0, 2, 11):
        broken, _ = model.apply(d.config, x, shift=(tap, -1 if tap == 11 else 1))
        assert worst(got, broken, bound) > 100.0, tap
    d.close()


# ---------------------------------------------------------------------------------------------- 3. cuts
@pytest.mark.parametrize("fin,fout", FORMATS, ids=["%s_%s" % f for f in FORMATS])
def test_cuts_are_the_bits_of_one_call(product, fin, fout):
    """pieces of 1 .. 257 samples, each handed its lead samples of history, are the bits of one call; pad=True on a whole stream is
    pad=False on the stream behind lead explicit zeros"""
    torch = _torch()
    in16, out16 = fin == "sc16", fout == "sc16"
    d = product.pamem(shape(product, "B3_T1_T3_T8_lead16"), gain=1.3, input_format=fin, output_format=fout)
    lead, n = d.lead, 33153                                                                # 33153 = 1 + 2 + ... + 257
    x = drive(lead + n, 0.25, seed=21, top=4.0)
    src = to_sc16(x) if in16 else x
    xd = put(src, 1, in16)
    one = d.execute(xd, pad=False)
    assert int(one.shape[0]) == n
    pieces = torch.zeros((n, 2), dtype=torch.int16, device="cuda") if out16 else torch.zeros(n, dtype=torch.complex64, device="cuda")
    at = 0
    for k in range(1, 258):
        y = d.execute(xd[at:at + lead + k], out=pieces[at:], pad=False)
        assert int(y.shape[0]) == k
        at += k
    assert at == n
    same = (lambda a, b: np.array_equal(host(a), host(b))) if out16 else (lambda a, b: np.array_equal(words(a), words(b)))
    assert same(pieces, one)
    zeros = np.zeros((lead, 2), np.int16) if in16 else np.zeros(lead, np.complex64)
    body = src[lead:]
    assert same(d.execute(put(body, 0, in16)), d.execute(put(np.concatenate([zeros, body]), 0, in16), pad=False))
    assert same(d.execute(put(body, 0, in16), 12345), d.execute(put(body, 1, in16), first_sample=1 << 40, pad=True))     # position is ignored
    d.close()


# ---------------------------------------------------------------------------------------------- 4. formats
def test_sc16_out_is_q_of_cf32_out_and_the_clip_count_is_the_models(product):
    branches = shape(product, "B4_T8_lead16")
    n = 5000
    for gain, clips_expected in ((2.5, True), (0.2, False)):
        f32, s16 = product.pamem(branches, gain=gain), product.pamem(branches, gain=gain, output_format="sc16")
        x = drive(f32.lead + n, 0.5, seed=31, top=10.0)
        xd = placed(x, 1)
        yf = host(f32.execute(xd, pad=False))
        ys = host(s16.execute(xd, pad=False))
        want, clips = model.quantise(yf)
        assert ys.dtype == np.int16 and np.array_equal(ys, want)
        assert s16.clipped() == clips and f32.clipped() == 0 and (0 < clips < n if clips_expected else clips == 0)
        s16.execute(xd, pad=False)
        assert s16.clipped(reset=True) == 2 * clips and s16.clipped() == 0
        f32.close(); s16.close()


def test_sc16_in_is_cf32_in_on_the_converted_floats(product):
    branches = shape(product, "B3_T1_T3_T8_lead16")
    n = 5000
    a, b = product.pamem(branches, gain=0.9), product.pamem(branches, gain=0.9, input_format="sc16")
    i16 = to_sc16(drive(a.lead + n, 0.25, seed=41, top=3.9))
    i16[:6] = [[-32768, 32767], [32767, -32768], [0, 0], [1, -1], [-32768, -32768], [-1, 0]]
    for shift in (0, 1):
        ya, yb = a.execute(placed(from_sc16(i16), shift), pad=False), b.execute(placed16(i16, shift), pad=False)
        assert np.array_equal(words(ya), words(yb)), shift
    a.close(); b.close()


def test_all_65536_values_of_a_component_pass(product):
    """B = 1, unit gain, far below saturation (A = 1e4: t <= 2e-8 rounds 1 + t to 1, so G = 1): every int16 value of re, and of im,
    comes out as it went in, sc16 to sc16; sc16 to cf32 it is the value times 2^-15"""
    d = product.pamem([dict(sat=1e4, smooth=1, taps=[(0, 1.0)])], input_format="sc16", output_format="sc16")
    f = product.pamem([dict(sat=1e4, smooth=1, taps=[(0, 1.0)])], input_format="sc16")
    v = np.arange(-32768, 32768, dtype=np.int32)
    i16 = np.stack([v, v[::-1]], axis=-1).astype(np.int16)
    for shift in (0, 1):
        assert np.array_equal(host(d.execute(placed16(i16, shift))), i16)
        assert np.array_equal(bits(host(f.execute(placed16(i16, shift)))), bits(from_sc16(i16)))
    assert d.clipped() == 0
    d.close(); f.close()


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_write_nothing(product):
    torch = _torch()
    L, EINVAL, OK = product.lib(), product.MCRX_EINVAL, product.MCRX_OK
    n, lead = 4096, 16
    buf = torch.zeros(4 * n, dtype=torch.complex64, device="cuda")
    torch.view_as_real(buf).view(torch.int32).fill_(SENTINEL_WORD)
    keep = buf.clone()
    p = buf.data_ptr()
    for fin, fout in FORMATS:
        d = product.pamem(shape(product, "B2_T3_T1_lead16"), input_format=fin, output_format=fout)
        assert d.lead == lead
        si, so = (4 if fin == "sc16" else 8), (4 if fout == "sc16" else 8)

        def call(a, b, count=n):
            return L.mcrx_hip_pamem_execute_device(d._h, C.c_void_p(a) if a else None, count, C.c_void_p(b) if b else None, None)
        far = p + 16 * n
        assert call(None, far) == EINVAL and call(p, None) == EINVAL                        # a null buffer
        assert call(p + si // 2, far) == EINVAL and call(p, far + so // 2) == EINVAL        # half a sample
        assert call(p, p) == EINVAL                                                         # in place: never
        assert call(p, p + so) == EINVAL and call(p + si, p) == EINVAL                      # out inside x, x inside out
        assert call(p, p + si * (n + lead) - so) == EINVAL                                  # the output's first sample on the input's last
        assert call(p + so * n - si, p) == EINVAL                                           # the input's first sample on the output's last
        assert call(p, far, (1 << 32) - lead + 1) == EINVAL and b"lead" in L.mcrx_hip_pamem_last_error()
        view16 = torch.view_as_real(buf).view(torch.int16).view(-1, 2)
        x = view16[:2 * n] if fin == "sc16" else buf[:n]
        with pytest.raises(ValueError):
            d.execute(x, out=(view16[2:] if fout == "sc16" else buf[1:]), pad=False)        # out inside x
        with pytest.raises(ValueError):
            d.execute(x[:lead - 1], pad=False)
        with pytest.raises(TypeError):
            d.execute(buf.real)
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(buf).view(torch.int32), torch.view_as_real(keep).view(torch.int32)), (fin, fout)
        assert d.clipped() == 0
        # what is allowed: adjacent ranges, nothing to do, an empty output
        assert call(p, p + si * (n + lead)) == OK and call(p + so * n, p) == OK and call(p, p, 0) == OK
        y = d.execute(x[:lead], pad=False)
        assert int(y.shape[0]) == 0 and int(d.execute(x[:0]).shape[0]) == 0
        torch.cuda.synchronize()
        buf.copy_(keep)
        d.close()


# ---------------------------------------------------------------------------------------------- 6. the linear regime
@pytest.mark.parametrize("f", [0.11, -0.37])
def test_the_linear_regime_is_the_fir(product, f):
    """sat = 1e4 times the drive's amplitude, AM/PM off: a complex tone at f cycles per sample comes out as H(f) times the tone, H from
    pamem_small_signal.  The tolerance is the model's rounding bound plus the compression term: for x >= 0,
    1 - x / (2p) <= (1 + x)^(-1 / (2p)) <= 1, so |A_b(u) - g_b u| <= g_b |u| t^p / (2p) with t = |u|^2 r_b -- 5e-9 |u| at p = 1 and
    t = 1e-8 --, through a tap at most |h| times that per component, through the gain |gain| times the sum.  The tone is fed as the
    nearest complex64 samples u; H(f) times THOSE samples is not a closed form (their rounding is no tone), so the device is held to
    sum_d H[d] u[i - d] in float64, and on the host that sum is H(f) times the exact tone to within the input's rounding."""
    amp, n, gain = 0.25, 4099, 0.8
    branches = [dict(b, sat=1e4 * amp, ampm_deg=0.0) for b in shape(product, "B3_T1_T3_T8_lead16")]
    d = product.pamem(branches, gain=gain)
    lead = d.lead
    H = product.pamem_small_signal(branches)
    assert len(H) == lead + 1
    tone = amp * np.exp(2j * np.pi * f * np.arange(-lead, n))
    u = tone.astype(np.complex64)
    fir = gain * np.convolve(u.astype(np.complex128), H)[lead:lead + n]
    Hf = np.sum(H * np.exp(-2j * np.pi * f * np.arange(lead + 1)))
    assert np.abs(fir - gain * Hf * tone[lead:]).max() <= abs(gain) * np.abs(H).sum() * SQ2 * EPS * amp
    _, bound = model.apply(d.config, u)
    comp = np.zeros(n)
    for b, (cfg, taps) in enumerate(model.branches_of(d.config)):
        p = cfg.amp_smooth
        t = np.abs(u.astype(np.complex128)) ** 2 * float(model.inv_sat2(d.config)[b])
        lack = abs(cfg.amp_gain) * np.abs(u) * t ** p / (2 * p)
        for dl, h in taps:
            comp += abs(h) * lack[lead - dl:lead - dl + n]
    comp *= abs(gain)
    got = host(d.execute(dev(u), pad=False))
    w = worst(got, fir, bound + comp)
    RATIOS["linear_f%+.2f" % f] = w
    print("pamem linear regime at f = %+.2f: worst error is %.3f of the tolerance; |H(f)| = %.4f" % (f, w, abs(Hf)))
    assert w <= 1.0
    d.close()


# ---------------------------------------------------------------------------------------------- 7. the stand-in
class MemoryAmplifier(object):
    """tests/test_gpu_mpd.py's stand-in, declared again: the three-branch amplifier of mpd_model.SEVERITY as three rfchain amplifier
    handles on u[i], u[i-1], u[i-2], shifted and summed with torch; zeros in front of the stream"""

    def __init__(self, product, rms):
        v = mpd_model.SEVERITY
        self.amps = [product.rfchain(amplifier=dict(sat=product.rfchain_backoff(ibo, rms), smooth=v["amp_smooth"], gain=v["amp_gain"], ampm_deg=deg))
                     for ibo, deg in zip(v["amp_ibo_db"], v["amp_ampm_deg"])]
        self.weights = [complex(w) for w in v["amp_weights"]]

    def execute(self, u, first_sample=0, stream=None):
        n = int(u.numel())
        z = self.amps[0].execute(u, first_sample, stream=stream) * self.weights[0]
        for b in (1, 2):
            z[b:] += self.amps[b].execute(u, first_sample, stream=stream)[:n - b] * self.weights[b]
        return z

    def close(self):
        for a in self.amps:
            a.close()


def severity_branches(product, rms):
    """mpd_model.SEVERITY's amplifier as pamem branches: three single-tap branches on delays 0, 1, 2"""
    v = mpd_model.SEVERITY
    return [dict(sat=product.rfchain_backoff(ibo, rms), smooth=v["amp_smooth"], gain=v["amp_gain"], ampm_deg=deg, taps=[(b, w)])
            for b, (ibo, deg, w) in enumerate(zip(v["amp_ibo_db"], v["amp_ampm_deg"], v["amp_weights"]))]


_STREAM = {}


def severity_stream(product):
    """(x, rms, sent): cfr_model.SEVERITY's transmitter behind its crest-factor reduction, as tests/test_gpu_mpd.py's closed loop makes
    it; made once and left alone"""
    if not _STREAM:
        torch = _torch()
        s = cfr_model.SEVERITY
        tx = product.multichanneltx(s["N"], s["M"], s["cp"], s["taper"])
        iq, sent = tx.generate(s["frames"], s["payload_len"], seed=77 + s["N"])
        tx.close()
        rms = rms_of(torch, iq)
        h = product.cfr_lowpass(s["half_len"], s["cutoff"], s["beta"])
        cf = product.cfr(float(np.float32(product.cfr_threshold(s["papr_db"], rms))), taps=h, passes=s["passes"])
        x = cf.execute(iq, pad=True)
        cf.close()
        _STREAM.update(x=x, rms=rms, sent=sent)
    return _STREAM["x"], _STREAM["rms"], _STREAM["sent"]


def standin_bound(cfgs, weights, u):
    """per component, what MemoryAmplifier may differ from the float64 sum of the weights it holds (complex128 Python numbers, applied
    by torch to complex64 tensors): the amplifier's bound e_b a branch (pamem_model.amp_bound); a complex product by the weight rounded
    to complex64 (eps |w| on the weight) is at most four products and two additions, six roundings of values <= c (|a| + sqrt2 e);
    the addition onto the sum one rounding of the partial sum.  Factor 1.01 for the second order, as the model's."""
    n = len(u)
    e, P = np.zeros(n), np.zeros(n)
    for b, (cfg, w) in enumerate(zip(cfgs, weights)):
        a, ea = np.abs(model.rfchain_model.amplifier(cfg, u.astype(np.complex128))), model.amp_bound(cfg, u)
        c = abs(w.real) + abs(w.imag)
        m = np.zeros(n)
        m[b:] = (c * (a + SQ2 * ea))[:n - b]
        e[b:] += (c * ea)[:n - b]
        P += m
        e += 7 * EPS * m + (EPS * P if b else 0.0)
    return 1.01 * e


def test_the_stand_in_agrees(product):
    """on mpd_model.SEVERITY's configuration and the cfr-shaped stream both this operator and the torch stand-in lie within their own
    bounds of the float64 model; their difference is printed and recorded, not asserted beyond the two bounds"""
    x, rms, _ = severity_stream(product)
    d = product.pamem(severity_branches(product, rms))
    st = MemoryAmplifier(product, rms)
    u = host(x)
    got, alt = host(d.execute(x)), host(st.execute(x))
    want, bound = model.apply(d.config, np.concatenate([np.zeros(d.lead, np.complex64), u]))
    w = worst(got, want, bound)
    cfgs = [a.config for a in st.amps]
    ref = mpd_model.memory_amplifier(cfgs, st.weights, u)
    ws = worst(alt, ref, standin_bound(cfgs, st.weights, u))
    peak = float(np.abs(want).max())
    diff = float(np.abs(got.astype(np.complex128) - alt).max())
    RATIOS["severity"], RATIOS["severity_stand_in"], RATIOS["severity_difference_over_peak"] = w, ws, diff / peak
    print("pamem on the SEVERITY stream (%d samples): %.3f of its bound; the stand-in %.3f of its own; they differ by %.3e of the peak"
          % (len(u), w, ws, diff / peak))
    assert w <= 1.0 and np.abs(got - want).max() <= 1e-5 * peak
    assert ws <= 1.0
    d.close(); st.close()


# ---------------------------------------------------------------------------------------------- 8. the closed loop
def learn_both(product, x, amp, torch):
    """three rounds of dpd and of mpd on `amp` at mpd_model.SEVERITY: (y0, yd, y, oob, nmse, mpd state, dpd state)"""
    v = mpd_model.SEVERITY
    peak = float(x.abs().max())
    fs, g0 = v["full_scale_over_peak"] * peak, v["amp_gain"]
    ref = x * g0
    y0 = amp.execute(x)
    dp = product.dpd(v["table_log2"], fs, g0)
    dp.learn(x, amp, v["rounds"])
    yd = amp.execute(dp.execute(x))
    mp = product.mpd(v["branches"], v["delays"], v["order"], v["table_log2"], fs, g0)
    mp.learn(x, amp, v["rounds"])
    y = amp.execute(mp.execute(x, pad=True))
    oob = [oob_of(torch, t, v["edge"]) for t in (y0, yd, y)]
    nmse = [nmse_of(torch, t, ref) for t in (y0, yd, y)]
    st, sd = mp.read(), dp.read()
    dp.close(); mp.close()
    return y0, yd, y, oob, nmse, st, sd


def test_closed_loop_on_the_device(product, oracle):
    """tests/test_gpu_mpd.py::test_closed_loop_on_the_device with this operator as the amplifier and nothing else changed:
    multichanneltx -> cfr -> predistorter -> pamem, three rounds of mpd(M = 3, P = 5, K = 128) and three of dpd on the same amplifier, at
    mpd_model.SEVERITY.  Asserted: mpd's NMSE is better than dpd's by SEVERITY's nmse_gain_db; mpd's power at |f| > 0.32 is not worse
    than dpd's by more than oob_slack_db; behind mpd all 24 frames are valid on the GPU receiver and on the oracle, the bytes identical,
    the equalised symbols within 1e-3.  The same figures of a run on the torch stand-in are recorded beside them (PARITY), not asserted."""
    from test_gpu_parity import match_frames, relerr, relerr_elem
    torch = _torch()
    s, v = cfr_model.SEVERITY, mpd_model.SEVERITY
    N, nf = s["N"], s["frames"]
    x, rms, sent = severity_stream(product)
    amp = product.pamem(severity_branches(product, rms))
    y0, yd, y, oob, nmse, st, sd = learn_both(product, x, amp, torch)
    assert (st["updates"], st["degenerate"], st["skipped"]) == (v["rounds"], 0, 0) and sd["degenerate"] == 0
    print("pamem closed loop: %d samples; none / dpd / mpd: power at |f| > %.2f %.2f / %.2f / %.2f dB, NMSE %.2f / %.2f / %.2f dB; gain of mpd over dpd %.2f dB"
          % ((int(x.numel()), v["edge"]) + tuple(oob) + tuple(nmse) + (nmse[1] - nmse[2],)))
    assert nmse[1] - nmse[2] >= v["nmse_gain_db"]
    assert oob[2] <= oob[1] + v["oob_slack_db"]
    n = int(y.numel()) // (product.TILE * 2 * N) * (product.TILE * 2 * N)
    y = y[:n].contiguous()
    rx = product.multichannelrx(N, s["M"], s["cp"], s["taper"], max_payload_len=s["payload_len"])
    rx.Execute(y); rx.Flush()
    ora = oracle.MultiChannelRx(N, s["M"], s["cp"], s["taper"])
    ora.execute(np.ascontiguousarray(host(y)))
    for side, frames in (("gpu", rx.frames), ("oracle", ora.frames)):
        assert len(frames) == N * nf, (side, len(frames))
        seen = set()
        for f in frames:
            assert f.header_valid and f.payload_valid, (side, f)
            pid = (f.header[0] << 8) | f.header[1]
            assert sent[f.channel][pid] == (bytes(f.header), bytes(f.payload)), (side, f.channel, pid)
            seen.add((f.channel, pid))
        assert len(seen) == N * nf
    w = we = 0.0
    for fg, fo in match_frames(rx.frames, ora.frames):
        assert bytes(fg.header) == bytes(fo.header) and bytes(fg.payload) == bytes(fo.payload)
        assert len(fg.framesyms) == len(fo.framesyms) > 0
        w, we = max(w, relerr(fg.framesyms, fo.framesyms)), max(we, relerr_elem(fg.framesyms, fo.framesyms))
    evm = [f.evm for f in rx.frames]
    rx.close(); amp.close()
    stand = MemoryAmplifier(product, rms)
    _, _, _, oob_s, nmse_s, st_s, _ = learn_both(product, x, stand, torch)
    stand.close()
    PARITY["severity"] = {"max_norm": w, "element_wise": we, "oob_db": oob, "nmse_db": nmse, "nmse_gain_over_dpd_db": nmse[1] - nmse[2],
                          "evm_db": [min(evm), max(evm)], "rows": st["rows"], "res_over_suu": st["res"] / st["Suu"],
                          "memory_amplifier": {"oob_db": oob_s, "nmse_db": nmse_s, "nmse_gain_over_dpd_db": nmse_s[1] - nmse_s[2],
                                               "rows": st_s["rows"], "res_over_suu": st_s["res"] / st_s["Suu"]}}
    print("pamem_parity: framesyms max-norm %.3e element-wise %.3e; EVM %.1f .. %.1f dB; on the stand-in NMSE %.2f / %.2f / %.2f dB"
          % ((w, we, min(evm), max(evm)) + tuple(nmse_s)))
    assert w <= 1e-3, w


def test_zz_print_pamem_figures():
    """(last of this file: the figures measured above as one JSON line each -- profiles/pamem_model.json and profiles/pamem_parity.json
    are such records; PAMEM_OUT / PAMEM_PARITY_OUT name files to write them to as well)"""
    for tag, rec, env in (("pamem_model", RATIOS, "PAMEM_OUT"), ("pamem_parity", PARITY, "PAMEM_PARITY_OUT")):
        line = json.dumps(rec, sort_keys=True)
        print(tag + " " + line)
        path = os.environ.get(env)
        if path:
            with open(path, "w") as f:
                f.write(line + "\n")
