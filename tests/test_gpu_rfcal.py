"""Receiver calibration on the GPU (mcrx_hip_rfcal_*): a handle before its first update against the codecs, the
moments against the model's integers (sc16) and within the summation bound (cf32), the update against the model fed with the library's
own accumulators, apply against the model fed with the library's own coefficients, the stream cut into pieces, the handle's operations
and refusals, where the image goes in a multichannelrx, and end to end against the oracle.  The bounds are derived in
tests/rfcal_model.py; the worst fraction of each that was met is recorded (RATIOS, printed by the last test)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import rfcal_model as model
import tx_sc16_model as q16

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5B
RATIOS, PARITY = {}, {}
GRID_MAX_N = 2048 * 512 + 513       # more pairs than RFCAL_MAX_ROWS workgroups of 256 lanes: the capped grid, lanes loop


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def host(t):
    return t.cpu().numpy()


def bits(t):
    torch = _torch()
    return torch.view_as_real(t).contiguous().view(torch.int32) if t.dtype == torch.complex64 else t


def dev(x):
    return _torch().from_numpy(np.ascontiguousarray(x)).cuda()


def ratio(tag, value):
    RATIOS[tag] = max(RATIOS.get(tag, 0.0), float(value))


_S = {}


def stream_cf32(n, seed=11):
    """an impaired stream: proper noise through a 3 dB / 15 degree receive mixer with DC, cf32; made once and left alone"""
    if (n, seed) not in _S:
        z = model.proper_noise(n, seed, rms=0.15)                      # (no component reaches full scale)
        g, phi = 10.0 ** (3.0 / 20.0), math.radians(15.0)
        al, be = (1.0 + g * np.exp(-1j * phi)) / 2.0, (1.0 - g * np.exp(1j * phi)) / 2.0
        _S[(n, seed)] = (al * z + be * np.conj(z) + STREAM_DC).astype(np.complex64)
    return _S[(n, seed)]


STREAM_DC = 0.02 - 0.01j
STREAM_W = ((1.0 - 10.0 ** 0.15 * np.exp(1j * math.radians(15.0))) / 2.0) / np.conj((1.0 + 10.0 ** 0.15 * np.exp(-1j * math.radians(15.0))) / 2.0)


def within(y, u, m, w, gain=1.0):
    """the worst fraction of apply_bound that the cf32 output y is from the model's"""
    d = np.asarray(y, np.complex128) - model.apply(u, m, w, gain)
    return float(np.max(np.maximum(np.abs(d.real), np.abs(d.imag)) / model.apply_bound(u, m, w, gain)))


def stream_sc16(n, seed=11):
    u = stream_cf32(n, seed)
    return q16.quantise_iq(u)


# ---------------------------------------------------------------------------------------------- 1. pass-through
def special_floats(n, seed):
    rng = np.random.RandomState(seed)
    w = rng.randint(0, 2 ** 32, size=2 * n, dtype=np.uint64).astype(np.uint32)
    fixed = np.array([0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0x7F800001, 0xFFC12345, 0x00000001, 0x807FFFFF], np.uint32)
    w[:min(len(fixed), 2 * n)] = fixed[:2 * n]
    return w.view(np.complex64)


@pytest.mark.parametrize("fin,fout", [("cf32", "cf32"), ("sc16", "cf32"), ("cf32", "sc16"), ("sc16", "sc16")])
def test_passthrough(product, fin, fout):
    """before the first update, gain 1: load, convert, store -- n = 1 .. 257, buffers offset by one sample, even and odd positions, the
    measuring builds and (held) the ones that do not measure"""
    torch = _torch()
    cal = product.rfcal(input_format=fin, output_format=fout)
    for n in range(1, 258):
        shift, first, held = n & 1, 7 * ((n >> 1) & 1), bool((n >> 2) & 1)
        if fin == "sc16":
            xi = np.random.RandomState(n).randint(-32768, 32768, size=(n, 2)).astype(np.int16)
            want = (xi.astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64).reshape(-1) if fout == "cf32" else xi
            src = torch.zeros((n + 2, 2), dtype=torch.int16, device="cuda")
            src[shift:shift + n].copy_(dev(xi))
        else:
            xi = special_floats(n, n)
            if fout == "sc16":
                with np.errstate(invalid="ignore"):
                    v = (xi.view(np.float32) % np.float32(3.0) - np.float32(1.5)).copy()
                v[:6] = [np.nan, np.inf, -np.inf, -0.0, 1.0, -1.0][:len(v)]
                xi = v.view(np.complex64)
            want = xi if fout == "cf32" else q16.quantise_iq(xi)
            src = torch.zeros((n + 2,), dtype=torch.complex64, device="cuda")
            torch.view_as_real(src).view(torch.int32)[shift:shift + n].copy_(dev(xi.view(np.int32).reshape(-1, 2)))
        if fout == "sc16":
            dst = torch.full((n + 3, 2), SENTINEL, dtype=torch.int16, device="cuda")
            fill = SENTINEL
        else:
            dst = torch.zeros((n + 3,), dtype=torch.complex64, device="cuda")
            torch.view_as_real(dst).view(torch.int32).fill_(0x7FC05A5B)
            fill = 0x7FC05A5B
        cal.reset_at(first)
        cal.hold(held)
        y = cal.execute(src[shift:shift + n], out=dst[shift:])
        assert int(y.shape[0]) == n and cal.position() == first + n
        got = host(bits(dst))
        want_bits = np.ascontiguousarray(want).view(np.int32).reshape(-1, 2) if fout == "cf32" else want
        assert np.array_equal(got[shift:shift + n], want_bits), (fin, fout, n)
        assert np.all(np.concatenate([got[:shift], got[shift + n:]]) == fill), (fin, fout, n)
    if fin == "sc16":
        assert cal.clipped() == 0
    cal.close()
    cal.close()                                                         # twice is harmless


# ---------------------------------------------------------------------------------------------- 2. moments
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, GRID_MAX_N])
def test_sc16_moments_are_the_models_integers(product, n):
    cal = product.rfcal(input_format="sc16")
    rng = np.random.RandomState(n)
    for tag, xi, first in (("all -32768", np.full((n, 2), -32768, np.int16), 0), ("random", rng.randint(-32768, 32768, size=(n, 2)).astype(np.int16), 5),
                           ("extremes", rng.choice(np.array([-32768, 32767], np.int16), size=(n, 2)), 2 ** 40 + 1)):
        cal.reset_at(first)
        assert cal.measure(dev(xi)) == n
        st = cal.read()
        assert st["acc"] == model.moments_sc16(xi), (tag, n)
        assert (st["count"], st["measured"], st["updates"]) == (n, n, 0) and cal.position() == first + n
    # in two calls, the second from an odd position and an unaligned buffer: the same integers
    if n > 1:
        cal.reset_at(0)
        buf = dev(np.concatenate([xi, xi[:1]]))
        k = n // 2 | 1
        cal.measure(buf[:k]); cal.measure(buf[k:n])
        assert cal.read()["acc"] == model.moments_sc16(xi)
    cal.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, GRID_MAX_N])
def test_cf32_moments_within_the_summation_bound(product, n):
    cal = product.rfcal()
    rng = np.random.RandomState(n + 1)
    amp = 10.0 ** rng.uniform(-3.0, math.log10(30.0), n)
    cases = [("log-uniform", (amp * np.exp(2j * np.pi * rng.uniform(size=n))).astype(np.complex64), 3)]
    if n < GRID_MAX_N:
        cases.append(("stream", stream_cf32(n, 4), 0))
    for tag, x, first in cases:
        cal.reset_at(first)
        cal.measure(dev(x))
        st = cal.read()
        mom, mag = model.moments_cf32(x)
        bound = model.moment_bound(n, mag)
        for k in range(5):
            assert abs(st["acc"][k] - mom[k]) <= bound[k], (tag, n, k, st["acc"][k], mom[k], bound[k])
            if bound[k] > 0:
                ratio("cf32_moment", abs(st["acc"][k] - mom[k]) / bound[k])
        assert st["count"] == n
    cal.close()


# ---------------------------------------------------------------------------------------------- 3. coefficients
def check_coefficients(st, ref, updates, tag, summed=0):
    bm, bw = model.coef_bound(ref.mean, updates, summed)
    assert abs(st["m"] - ref.m) <= bm * math.sqrt(2.0) + 1e-300, (tag, st["m"], ref.m, bm)
    assert abs(st["w"] - ref.w) <= bw * math.sqrt(2.0) + 1e-300, (tag, st["w"], ref.w, bw)
    ratio("coefficient_w", abs(st["w"] - ref.w) / (bw * math.sqrt(2.0)) if bw else 0.0)
    ratio("coefficient_m", abs(st["m"] - ref.m) / (bm * math.sqrt(2.0)) if bm else 0.0)


@pytest.mark.parametrize("fin", ["cf32", "sc16"])
def test_one_update_against_the_model(product, fin):
    n = 20001
    x = stream_cf32(n) if fin == "cf32" else stream_sc16(n)
    for stages in (3, 1, 2, 0):
        cal = product.rfcal(dc=bool(stages & 1), iq=bool(stages & 2), input_format=fin)
        cal.measure(dev(x))
        before = cal.read()
        ref = model.State(stages=stages, sc16=fin == "sc16")
        ref.update(before["acc"], before["count"])                      # the library's own accumulators
        cal.update()
        st = cal.read()
        assert (st["updates"], st["degenerate"], st["count"], st["measured"]) == (1, 0, 0, n)
        assert st["acc"] == ([0] * 5 if fin == "sc16" else [0.0] * 5)
        assert np.allclose(st["mean"], ref.mean, rtol=8 * model.U, atol=0)
        check_coefficients(st, ref, 1, (fin, stages))
        if stages == 3:                                                 # the stream's own mixer and DC: its noise is proper in its sample moments,
            assert abs(st["w"] - STREAM_W) <= 1e-3 and abs(st["m"] - STREAM_DC) <= 1e-4     # up to the rounding of the samples to cf32 / sc16
        if not stages & 1:
            assert st["m"] == 0
        if not stages & 2:
            assert st["w"] == 0 and st["irr_db"] == math.inf
        cal.close()


@pytest.mark.parametrize("forget_log2", [0, 3, 30])
def test_300_updates_against_the_model(product, forget_log2):
    """sc16 in, blocks of 64: the library's accumulators are the model's integers (test above), so the model runs on its own"""
    n = 300 * 64 + 17
    xi = stream_sc16(n, 21)
    cal = product.rfcal(period_log2=6, forget_log2=forget_log2, input_format="sc16")
    cal.measure(dev(xi))
    st = cal.read()
    ref = model.State(forget_log2=forget_log2, sc16=True)
    for j in range(300):
        ref.measure(xi[64 * j:64 * j + 64])
        ref.update()
    ref.measure(xi[300 * 64:])
    assert (st["updates"], st["count"], st["measured"], st["degenerate"]) == (300, 17, n, ref.degenerate)
    assert st["acc"] == ref.acc
    assert np.allclose(st["mean"], ref.mean, rtol=(8 + 4 * 300) * model.U, atol=(8 + 4 * 300) * model.U * ref.mean[4])
    check_coefficients(st, ref, 300, forget_log2)
    cal.close()


def test_degenerate_blocks_keep_the_coefficients(product):
    for fin in ("cf32", "sc16"):
        for tag, x in (("zeros", np.zeros(64, np.complex64)), ("constant", np.full(64, 0.25 - 0.5j, np.complex64)),
                       ("real", (np.linspace(-1, 1, 64) * 0.9).astype(np.complex64))):
            cal = product.rfcal(input_format=fin)
            cal.set(0.125j, 0.25)
            cal.measure(dev(x if fin == "cf32" else q16.quantise_iq(x)))
            cal.update()
            st = cal.read()
            assert (st["m"], st["w"], st["updates"], st["degenerate"], st["count"]) == (0.125j, 0.25, 1, 1, 0), (fin, tag, st)
            cal.close()
    cal = product.rfcal()                                               # a block that is not finite is dropped whole
    cal.measure(dev(stream_cf32(1000))); cal.update()
    good = cal.read()
    cal.measure(dev(np.array([1.0, np.nan, 2.0], np.complex64))); cal.update()
    st = cal.read()
    assert (st["m"], st["w"], st["mean"], st["updates"]) == (good["m"], good["w"], good["mean"], 1) and st["degenerate"] == 1 and st["count"] == 0
    cal.close()


# ---------------------------------------------------------------------------------------------- 4. apply
@pytest.mark.parametrize("fin", ["cf32", "sc16"])
def test_apply_against_the_model(product, fin):
    torch = _torch()
    n = 4099
    rng = np.random.RandomState(5)
    amp = 10.0 ** rng.uniform(-3.0, math.log10(30.0), n) * (1.0 if fin == "cf32" else 1.0 / 30.0)
    x = (amp * np.exp(2j * np.pi * rng.uniform(size=n))).astype(np.complex64)
    xin = x if fin == "cf32" else q16.quantise_iq(x)
    u = x.astype(np.complex128) if fin == "cf32" else model.from_sc16(xin)
    for gain in (1.0, 0.75, 2.5):
        outs = {}
        for fout in ("cf32", "sc16"):
            cal = product.rfcal(gain=gain, input_format=fin, output_format=fout)
            cal.set(0.03 - 0.02j, -0.17 + 0.13j)
            cal.hold(True)
            st = cal.read()
            outs[fout] = host(cal.execute(dev(xin)))
            if fout == "sc16":
                assert cal.clipped() == q16.clipped_samples(outs["cf32"]), (fin, gain)
            assert cal.read()["measured"] == 0
            cal.close()
        g32 = float(np.float32(gain))
        want, bound = model.apply(u, st["m"], st["w"], g32), model.apply_bound(u, st["m"], st["w"], g32)
        d = outs["cf32"].astype(np.complex128) - want
        worst = float(np.max(np.maximum(np.abs(d.real), np.abs(d.imag)) / bound))
        ratio("apply", worst)
        assert worst <= 1.0, (fin, gain, worst)
        assert np.array_equal(outs["sc16"], q16.quantise_iq(outs["cf32"])), (fin, gain)      # the integers are Q of the floats
        d = outs["cf32"].astype(np.complex128) - model.apply_fp32(u.astype(np.complex64), st["m"], st["w"], g32).astype(np.complex128)
        assert float(np.max(np.maximum(np.abs(d.real), np.abs(d.imag)) / bound)) <= 1.0


# ---------------------------------------------------------------------------------------------- 5. cuts
def pieces(n, seed):
    rng, cuts, at = np.random.RandomState(seed), [], 0
    while at < n:
        m = min(int(rng.randint(1, 258)), n - at)
        cuts.append((at, m))
        at += m
    return cuts


@pytest.mark.parametrize("first", [0, 2 ** 40 + 1, 2 ** 64 - 1501], ids=["0", "2^40", "across_2^64"])
@pytest.mark.parametrize("fout", ["sc16", "cf32"])
def test_sc16_cuts_give_the_same_bits(product, first, fout):
    torch = _torch()
    n, k = 3001, 6
    xi = stream_sc16(n, 31)
    x = dev(xi)
    kw = dict(period_log2=k, forget_log2=2, input_format="sc16", output_format=fout, gain=0.9)
    one = product.rfcal(**kw)
    one.reset_at(first)
    want = one.execute(x)
    ref = one.read()
    assert ref["updates"] == len([e for e in model.segments(first, n, k)[1] if e]) >= 46
    for seed, inplace in ((1, False), (2, fout == "sc16")):
        cal = product.rfcal(**kw)
        cal.reset_at(first)
        buf = x.clone()
        out = buf if inplace else torch.empty_like(want)
        for at, m in pieces(n, seed):
            cal.execute(buf[at:at + m], out=out[at:at + m])
        assert torch.equal(bits(out), bits(want)), (first, fout, seed)
        assert cal.read() == ref and cal.position() == (first + n) % 2 ** 64
        assert cal.clipped() == one.clipped()
        cal.close()
    # manual updates at the same absolute positions
    man = product.rfcal(**dict(kw, period_log2=0))
    man.reset_at(first)
    out, at = torch.empty_like(want), 0
    for m, ends in zip(*model.segments(first, n, k)):
        man.execute(x[at:at + m], out=out[at:at + m])
        if ends:
            man.update()
        at += m
    assert torch.equal(bits(out), bits(want)) and man.read() == ref
    man.close(); one.close()


def test_cf32_cuts(product):
    """the same calls twice: the same bits.  Differently cut: the accumulators within twice the summation bound of each other, the
    coefficients within the bound that follows from it."""
    torch = _torch()
    n = 30001
    xh = stream_cf32(n, 41)
    x = dev(xh)
    runs = []
    for seed in (1, 1, 2, None):
        cal = product.rfcal()
        cuts = pieces(n, seed) if seed else [(0, n)]
        for at, m in cuts:
            cal.measure(x[at:at + m])
        acc = cal.read()
        cal.update()
        y = cal.execute(x)
        runs.append((acc, cal.read(), y))
        cal.close()
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1] and torch.equal(bits(runs[0][2]), bits(runs[1][2]))
    mom, mag = model.moments_cf32(xh)
    bound = model.moment_bound(n, mag)
    ref = model.State()
    ref.update(mom, n)
    for acc, st, _ in runs:
        for k in range(5):
            assert abs(acc["acc"][k] - mom[k]) <= bound[k]
            ratio("cf32_cut_moment", abs(acc["acc"][k] - mom[k]) / bound[k])
        check_coefficients(st, ref, 1, "cuts", summed=n)
    for k in range(5):
        assert abs(runs[0][0]["acc"][k] - runs[3][0]["acc"][k]) <= 2.0 * bound[k]


# ---------------------------------------------------------------------------------------------- 6. the handle's operations
def test_hold_set_and_reset(product):
    torch = _torch()
    x = dev(stream_cf32(5000))
    cal = product.rfcal(period_log2=10)
    cal.execute(x[:2048])
    a = cal.read()
    assert a["updates"] == 2 and a["measured"] == 2048
    cal.hold(True)
    y = cal.execute(x[2048:4096])
    assert cal.read() == a and cal.position() == 4096                   # frozen: nothing measured, no update, the coefficients apply
    assert within(host(y), stream_cf32(5000)[2048:4096], a["m"], a["w"]) <= 1.0
    cal.hold(False)
    cal.set(0.5, 0.25j)                                                 # set takes effect ...
    b = cal.read()
    assert (b["m"], b["w"], b["updates"]) == (0.5, 0.25j, 2) and b["irr_db"] == pytest.approx(-20 * math.log10(0.25))
    y = cal.execute(x[4096:4100])
    assert within(host(y), stream_cf32(5000)[4096:4100], 0.5, 0.25j) <= 1.0
    cal.reset_at(2 ** 40)                                               # ... and reset_at clears
    c = cal.read()
    assert (c["m"], c["w"], c["mean"], c["acc"], c["count"], c["updates"], c["measured"], c["degenerate"]) == (0, 0, [0.0] * 5, [0.0] * 5, 0, 0, 0, 0)
    assert cal.position() == 2 ** 40
    y = cal.execute(x[:100])                                            # the first block after a reset passes uncorrected
    assert torch.equal(bits(y), bits(x[:100]))
    cal.reset_at(0)                                                     # a reset carried by the next fold: nothing of the 100 samples stays
    cal.measure(x[:64])
    d = cal.read()
    assert (d["count"], d["measured"], d["updates"]) == (64, 64, 0)
    with pytest.raises(ValueError):
        cal.update()                                                    # the handle updates by itself
    with pytest.raises(ValueError):
        cal.set(float("nan"), 0.0)
    cal.close()


def test_refusals_write_nothing_and_consume_nothing(product):
    torch = _torch()
    L = product.lib()
    n = 1000
    xi = dev(stream_sc16(n + 8))
    cal = product.rfcal(input_format="sc16", output_format="sc16")
    cal.reset_at(5)
    cal.measure(xi[:100])
    before = cal.read()
    out = torch.full((n + 8, 2), SENTINEL, dtype=torch.int16, device="cuda")

    def refused(d_in, count, d_out):
        assert L.mcrx_hip_rfcal_execute_device(cal._h, C.c_void_p(d_in), count, C.c_void_p(d_out) if d_out else None, None) == product.MCRX_EINVAL
        assert L.mcrx_hip_rfcal_last_error()
        assert cal.position() == 105 and cal.read() == before
        assert bool((out == SENTINEL).all())
    pi, po = xi.data_ptr(), out.data_ptr()
    refused(pi + 2, n, po)                                              # misaligned input
    refused(pi, n, po + 2)                                              # misaligned output
    refused(pi, n, pi + 4)                                              # overlap that is not in place
    refused(pi + 4, n, pi)
    refused(0, n, po)                                                   # null input
    refused(pi, 2 ** 32 + 1, po)                                        # too many samples
    refused(pi, 2 ** 31 - 99, None)                                     # the guard: 100 + 2^31 - 99 > 2^31 measured since the last update
    assert L.mcrx_hip_rfcal_execute_device(cal._h, C.c_void_p(pi), 0, C.c_void_p(po), None) == product.MCRX_OK
    cal.update()                                                        # an update clears the count the guard looks at
    assert cal.execute(xi[:n], out=out).shape[0] == n and cal.position() == 105 + n
    assert cal.execute(xi[:n], out=xi[:n]).shape[0] == n                # in place is allowed
    cal.close()
    cf = product.rfcal()
    xc = dev(stream_cf32(16))
    assert L.mcrx_hip_rfcal_execute_device(cf._h, C.c_void_p(xc.data_ptr() + 4), 8, None, None) == product.MCRX_EINVAL and cf.position() == 0
    cf.close()


# ---------------------------------------------------------------------------------------------- 7. where the image goes
def test_the_image_goes_where_it_must(product):
    """test_gpu_rfchain.py's lone carrier (8 channels, channel 2 sending) through a 1 dB / 5 degree receive mixer: measure, update,
    execute, then the receiver's monitor."""
    from test_gpu_rfchain import carriers, levels_db
    torch = _torch()
    mix = product.rfchain_iq(1.0, 5.0, "rx")
    truth = mix["beta"] / mix["alpha"].conjugate()
    iq = carriers(product, 2, 1)
    rf = product.rfchain(order="rx", mixer=mix)
    cfg = rf.config
    want = 10.0 * math.log10((cfg.beta_re ** 2 + cfg.beta_im ** 2) / (cfg.alpha_re ** 2 + cfg.alpha_im ** 2))
    u = rf.execute(iq)
    cal = product.rfcal()
    cal.measure(u); cal.update()
    y = cal.execute(u)
    st = cal.read()
    off, frames_off = levels_db(product, iq)
    raw, _ = levels_db(product, u)
    fixed, frames = levels_db(product, y)
    print("rfcal image: level[5] - level[2]: mixer off %.2f dB, uncorrected %.2f dB (|beta|^2 / |alpha|^2 = %.2f dB), corrected %.2f dB; irr %.1f dB"
          % (off[5] - off[2], raw[5] - raw[2], want, fixed[5] - fixed[2], st["irr_db"]))
    assert frames == frames_off == 3
    assert abs((raw[5] - raw[2]) - want) <= 0.5
    assert abs((fixed[5] - fixed[2]) - (off[5] - off[2])) <= 1.0
    RATIOS["image_uncorrected_db"], RATIOS["image_corrected_db"], RATIOS["image_off_db"] = raw[5] - raw[2], fixed[5] - fixed[2], off[5] - off[2]
    cal.close()
    # channels 2 and 5 both sending: mirror channels carry the same preamble, the estimate is biased -- judged against the float64
    # model on the same samples, not against a fixed figure
    iq2 = carriers(product, 2, 1) + carriers(product, 5, 1)
    u2 = rf.execute(iq2)
    rf.close()
    cal = product.rfcal()
    cal.measure(u2); cal.update()
    st = cal.read()
    ref = model.State()
    ref.measure(host(u2)); ref.update()
    resid = lambda w: -20.0 * math.log10(abs((truth - w) / (1.0 - truth.conjugate() * w)))
    print("rfcal image, mirror channels 2 and 5: residual image %.1f dB, the model on the same samples %.1f dB (uncorrected %.1f dB)"
          % (resid(st["w"]), resid(ref.w), -20.0 * math.log10(abs(truth))))
    assert abs(resid(st["w"]) - resid(ref.w)) <= 1.0
    RATIOS["mirror_residual_db"] = resid(st["w"])
    cal.close()


# ---------------------------------------------------------------------------------------------- 8. end to end
@pytest.mark.parametrize("period_log2", [0, 14])
def test_end_to_end(product, oracle, period_log2):
    """multichanneltx -> rfchain (rx order, the severity case's mixer and DC) -> chanemu (noise at 30 dB) -> rfcal (sc16 out) ->
    multichannelrx(sc16), and the oracle's receiver on the same corrected integers.  period_log2 = 0: measured over the whole stream,
    one update, every frame valid on both sides with the bytes sent.  14: tracking from a cold start; the frames that begin after the
    second block are all valid."""
    from test_gpu_parity import relerr
    from test_rfcal import SEVERITY as s
    torch = _torch()
    N, M, cp, taper, nf, plen = s["N"], s["M"], s["cp"], s["taper"], s["frames"], s["payload_len"]
    tx = product.multichanneltx(N, M, cp, taper)
    iq, sent = tx.generate(nf, plen, seed=77 + N)
    tx.close()
    rf = product.rfchain(order="rx", mixer=dict(product.rfchain_iq(s["iq_gain_db"], s["iq_phase_deg"], "rx"), dc=s["dc"]))
    a = rf.execute(iq)
    rf.close()
    rms = float(torch.view_as_real(iq).pow(2).sum().div(int(iq.numel())).sqrt())
    nstd = float(np.float32(rms * 10.0 ** (-s["snr_db"] / 20.0) / math.sqrt(2.0)))
    ce = product.chanemu(taps=[(0, 1.0)], noise_std=nstd, seed=s["noise_seed"])
    b = ce.execute(a)
    ce.close()
    peak = float(torch.view_as_real(b).abs().max())
    cal = product.rfcal(period_log2=period_log2, forget_log2=3, gain=float(np.float32(0.5 / peak)), output_format="sc16")
    if period_log2 == 0:
        cal.measure(b); cal.update()
    y = cal.execute(b)
    st = cal.read()
    assert cal.clipped() == 0
    cal.close()
    n = int(y.shape[0]) // (product.TILE * 2 * N) * (product.TILE * 2 * N)
    y = y[:n].contiguous()
    y_host = (host(y).astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64).reshape(-1)
    rx = product.multichannelrx(N, M, cp, taper, max_payload_len=plen, input_format="sc16")
    rx.Execute(y); rx.Flush()
    ora = oracle.MultiChannelRx(N, M, cp, taper)
    ora.execute(np.ascontiguousarray(y_host))
    frame_len = int(n // nf)                                            # frames go back to back: frame p of a channel begins near p n / nf
    late = [p for p in range(nf) if p * frame_len >= 2 << 14]
    must = {(c, p) for c in range(N) for p in (range(nf) if period_log2 == 0 else late)}
    assert period_log2 == 0 or late, "the stream must outlast two blocks"
    for side, frames in (("gpu", rx.frames), ("oracle", ora.frames)):
        seen = set()
        for f in frames:
            pid = (f.header[0] << 8) | f.header[1]
            if f.header_valid and f.payload_valid and pid < nf and sent[f.channel][pid] == (bytes(f.header), bytes(f.payload)):
                seen.add((f.channel, pid))
        assert must <= seen, (side, sorted(must - seen))
        if period_log2 == 0:
            assert len(frames) == N * nf, (side, len(frames))
    w = 0.0
    key = lambda f: (f.channel, (f.header[0] << 8) | f.header[1])
    by_key = {key(f): f for f in ora.frames if f.header_valid and f.payload_valid}
    for fg in rx.frames:
        if fg.header_valid and fg.payload_valid and key(fg) in must:
            fo = by_key[key(fg)]
            assert bytes(fg.header) == bytes(fo.header) and bytes(fg.payload) == bytes(fo.payload)
            assert len(fg.framesyms) == len(fo.framesyms) > 0
            w = max(w, relerr(fg.framesyms, fo.framesyms))
    evm = [f.evm for f in rx.frames if f.payload_valid]
    rx.close()
    PARITY["period_%d" % period_log2] = {"max_norm": w, "irr_db": st["irr_db"], "updates": st["updates"], "evm_db": [min(evm), max(evm)], "noise_std": nstd}
    print("rfcal_parity period_log2 %d: framesyms max-norm %.3e; irr %.1f dB after %d updates; EVM %.1f .. %.1f dB" % (period_log2, w, st["irr_db"], st["updates"], min(evm), max(evm)))
    assert w <= 1e-3, w


def test_zz_print_rfcal_figures():
    """(last of this file: the figures measured above as one JSON line each -- profiles/rfcal_model.json and profiles/rfcal_parity.json
    are such records; RFCAL_OUT / RFCAL_PARITY_OUT name files to write them to as well)"""
    for tag, rec, env in (("rfcal_model", RATIOS, "RFCAL_OUT"), ("rfcal_parity", PARITY, "RFCAL_PARITY_OUT")):
        line = json.dumps(rec, sort_keys=True)
        print(tag + " " + line)
        path = os.environ.get(env)
        if path:
            with open(path, "w") as f:
                f.write(line + "\n")
