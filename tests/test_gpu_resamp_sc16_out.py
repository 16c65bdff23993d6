"""16-bit integer IQ (sc16) straight out of the resampler, and its output gain.  Let y be the fp32 value a cf32 resampler stores for a
component: a handle with output gain g stores v = y * g (one fp32 multiply), and an sc16-output handle stores Q(v), the transmitter's
quantiser (tests/tx_sc16_model.py) -- so everything here is raw-word equality against Q of a cf32 handle's output, no tolerance.  (The
cf32 path is held to the oracle by test_gpu_parity.test_msresamp_front_end_matches_oracle, the sc16 input to the cf32 one by
test_gpu_resamp_sc16.py.)"""
import ctypes as C
import struct

import numpy as np
import pytest

import position_model as pm
import tx_sc16_model as model

pytestmark = pytest.mark.gpu

# every last-stage build: the arbitrary stage with a table (0.37, 0.45 folded half-band; 0.7, 1.5 plain) or with one branch per thread
# (0.25 folded; 0.5, 0.8, 1.0, 2.0 plain), behind halfband_kernel (0.2, 0.11, 0.06), and the half-band interpolator last (4.0, 6.3)
ONE_SHOT_RATES = [0.5, 0.37, 0.8, 0.2, 0.11, 2.0, 1.5, 4.0, 6.3, 0.25, 0.45, 0.06, 0.7, 1.0]
BOTH_RATES = [0.5, 0.37, 2.0, 4.0]
STREAM_RATES = [0.5, 0.37, 0.06, 1.5, 4.0]
CLIP_RATES = [2.0, 0.37, 4.0]
GAIN = float(np.float32(0.7310585))        # not a power of two: the multiply rounds
SENTINEL = 0x5A5B                          # planted where nothing may be stored


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def dequantise(q):
    """interleaved int16 -> complex64, the definition of an sc16 sample: exact"""
    return (q.astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64)


def words(t):
    """a complex64 device tensor as its raw 32-bit words"""
    import torch
    return torch.view_as_real(t).contiguous().view(torch.int32)


def same_words(a, b):
    import torch
    return a.numel() == b.numel() and torch.equal(words(a), words(b))


def Q(y):
    """the model's integers for a complex64 device tensor, as an int16 device tensor of shape (n, 2)"""
    import torch
    return torch.from_numpy(model.quantise_iq(y.cpu().numpy())).to(y.device)


def stream_len(rate):
    """test_gpu_resamp_sc16.py's: inputs for which the arbitrary stage makes two full workgroups and a partial chunk (2 * 8192 + 1000
    outputs, and a bit) -- a workgroup's last partial chunk, the prefetch of a following chunk, and a wave whose lanes leave the output
    loop at different points before the clip commit.  Odd."""
    plan = pm.ResampPlan(rate)
    return (int(17400 / plan.rate_arb) + 1) * plan.raw_per_arb() + 3


def samples(rate):
    """Seeded noise of moderate level (a quarter of full scale rms) on the int16 grid, so that the same values exist as int16"""
    n = stream_len(rate)
    rng = np.random.RandomState(int(rate * 1000) + 11)
    return np.clip(np.rint(rng.randn(2 * n) * 8192.0), -32768, 32767).astype(np.int16)


_REF = {}


class Ref(object):
    """Computed once per rate, on the device, and left alone: d_q / d_x the input as int16 and as the same floats; y[g] the output of
    a cf32 handle with gain g; i[g] the output of an sc16-output handle with gain g (both on d_x); plain: a handle made without the
    new keywords."""


def ref(product, rate):
    if rate not in _REF:
        torch = _torch()
        r = Ref()
        q = samples(rate)
        r.d_q, r.d_x = torch.from_numpy(q).cuda(), torch.from_numpy(dequantise(q)).cuda()
        r.n = int(r.d_x.numel())
        rs = product.msresamp(rate)
        r.plain = rs.execute(r.d_x)
        rs.close()
        r.y, r.i = {}, {}
        for g in (1.0, GAIN):
            rs_f, rs_i = product.msresamp(rate, output_format="cf32", gain=g), product.msresamp(rate, output_format="sc16", gain=g)
            assert (rs_f.output_format, rs_i.output_format) == (0, 1) and rs_f.gain == g and rs_i.gain == g
            r.y[g], r.i[g] = rs_f.execute(r.d_x), rs_i.execute(r.d_x)
            torch.cuda.synchronize()
            rs_f.close(); rs_i.close()
        _REF[rate] = r
    return _REF[rate]


# ---------------------------------------------------------------------------------------------- 1. one-shot identity
@pytest.mark.parametrize("rate", ONE_SHOT_RATES)
def test_one_shot_identity(product, rate):
    torch = _torch()
    r = ref(product, rate)
    assert r.plain.numel() > 0.9 * rate * r.n
    peak = float(torch.view_as_real(r.plain).abs().max())
    assert np.isfinite(peak) and peak > 1e-3                                   # (the comparisons below are not of zeros)
    # gain 1 with the new keywords is the handle without them, word for word
    assert r.y[1.0].dtype == torch.complex64 and same_words(r.y[1.0], r.plain)
    # the gain is one fp32 multiply behind the value stored today
    by_torch = torch.view_as_complex(torch.view_as_real(r.plain) * torch.tensor(GAIN, dtype=torch.float32, device="cuda"))
    assert same_words(r.y[GAIN], by_torch)
    assert not same_words(r.y[GAIN], r.plain)
    for g in (1.0, GAIN):
        got = r.i[g]
        assert got.dtype == torch.int16 and got.dim() == 2 and got.shape[1] == 2 and got.is_contiguous()
        assert got.shape[0] == r.y[g].numel()
        assert int(torch.unique(got).numel()) > 64
        assert torch.equal(got, Q(r.y[g])), g


# ---------------------------------------------------------------------------------------------- 2. both formats at once
@pytest.mark.parametrize("rate", BOTH_RATES)
def test_sc16_in_and_sc16_out(product, rate):
    """int16 in, int16 out = Q of (cf32 in on the dequantised floats, cf32 out)"""
    torch = _torch()
    r = ref(product, rate)
    for g in (1.0, GAIN):
        rs = product.msresamp(rate, input_format="sc16", output_format="sc16", gain=g)
        assert (rs.input_format, rs.output_format) == (1, 1)
        got = rs.execute(r.d_q)
        rs.close()
        assert got.dtype == torch.int16 and got.shape == (r.y[g].numel(), 2)
        assert torch.equal(got, Q(r.y[g])), g


# ---------------------------------------------------------------------------------------------- 3. streamed identity
def ragged_pieces(n, seed):
    """test_gpu_resamp_sc16.py's cuts of [0, n): pieces shorter than the retained history first (0, 1, 7, 63), odd sizes, one large
    piece, then seeded odds and ends."""
    rng = np.random.RandomState(seed)
    sizes = [1, 7, 0, 63, 1, 2, 777, (n // 3) | 1, 64, 4096, 0, 333]
    cuts, pos = [], 0
    for s in sizes:
        cuts.append((pos, min(pos + s, n))); pos = min(pos + s, n)
    while pos < n:
        s = int(rng.randint(1, 3000))
        cuts.append((pos, min(pos + s, n))); pos = min(pos + s, n)
    assert all(any(b - a == s for a, b in cuts) for s in (0, 1, 7, 63))
    return cuts


def execute_c(product, h, src, n, dst_ptr, cap, sc16_in=False):
    """(return code, *nout) of one call of the C-ABI: src a device tensor, dst_ptr a device address"""
    L = product.lib()
    fn = L.msresamp_hip_execute_device_sc16 if sc16_in else L.msresamp_hip_execute_device
    nout = C.c_size_t(0)
    rc = fn(h, C.c_void_p(src.data_ptr()), n, C.c_void_p(dst_ptr), cap, C.byref(nout), None)
    return rc, int(nout.value)


@pytest.mark.parametrize("rate", STREAM_RATES)
def test_streamed_identity(product, rate):
    """Every call writes behind the previous one in ONE buffer, which begins on an odd sample (lead = 1) or an even one: output
    pointers that are 4- but not 8-byte aligned, at 4.0 -- where a call's outputs come in fours -- for every call of the first pass."""
    torch = _torch()
    r = ref(product, rate)
    want = r.i[GAIN]
    total = int(want.shape[0])
    rs = product.msresamp(rate, output_format="sc16", gain=GAIN)
    for lead in (1, 2):
        buf = torch.full((lead + total + 64, 2), SENTINEL, dtype=torch.int16, device="cuda")
        assert buf.data_ptr() % 8 == 0
        rs.reset()
        pos, odd_calls = lead, []
        for a, b in ragged_pieces(r.n, int(rate * 100)):
            ptr = buf.data_ptr() + 4 * pos
            rc, nout = execute_c(product, rs._h, r.d_x[a:b], b - a, ptr, buf.shape[0] - pos)
            assert rc == product.MCRX_OK, (a, b, product.lib().msresamp_hip_last_error())
            if ptr % 8 == 4:
                odd_calls.append(nout)
            pos += nout
            assert pos <= lead + total
            assert bool((buf[pos:pos + 8] == SENTINEL).all()), (a, b)         # no store past *nout
        assert pos == lead + total
        assert torch.equal(buf[lead:pos], want)                                # the stream cut in pieces is the stream
        assert bool((buf[:lead] == SENTINEL).all()) and bool((buf[pos:] == SENTINEL).all())
        if lead == 1:
            assert any(k > 0 for k in odd_calls)
            if rate == 4.0:
                assert any(k > 2048 for k in odd_calls)
    rs.close()


# ---------------------------------------------------------------------------------------------- 4. format and gain in mid-stream
@pytest.mark.parametrize("rate", [0.37, 2.0, 4.0])
def test_format_and_gain_in_mid_stream(product, rate):
    torch = _torch()
    L = product.lib()
    r = ref(product, rate)
    rs = product.msresamp(rate)
    h = rs._h
    cap = int(L.msresamp_hip_max_output(h, r.n)) + 8
    out_f = torch.zeros(cap, dtype=torch.complex64, device="cuda")
    out_i = torch.zeros((cap, 2), dtype=torch.int16, device="cuda")
    settings = [(1, GAIN), (0, 1.0), (1, 1.0), (0, GAIN), (1, GAIN), (0, GAIN), (1, 1.0)]
    step = r.n // len(settings) | 1
    cuts = [(k * step, r.n if k + 1 == len(settings) else (k + 1) * step) for k in range(len(settings))]
    pos = 0
    for k, ((fmt, g), (a, b)) in enumerate(zip(settings, cuts)):
        rc_f, rc_g = L.msresamp_hip_set_output_format(h, fmt), L.msresamp_hip_set_output_gain(h, g)
        assert rc_f != product.MCRX_EBUSY and rc_g != product.MCRX_EBUSY
        assert rc_f == product.MCRX_OK and rc_g == product.MCRX_OK
        assert (rs.output_format, rs.gain) == (fmt, g)
        dst = out_i if fmt else out_f
        if k in (2, 3):         # an output buffer too small: refused, and the next correct call continues the stream
            rc, nout = execute_c(product, h, r.d_x[a:b], b - a, dst.data_ptr(), 16)
            assert rc == product.MCRX_EINVAL and nout == 0
        rc, nout = execute_c(product, h, r.d_x[a:b], b - a, dst.data_ptr(), cap)
        assert rc == product.MCRX_OK and nout > 0.9 * rate * (b - a) - 64
        if fmt:
            assert torch.equal(out_i[:nout], r.i[g][pos:pos + nout]), k
        else:
            assert same_words(out_f[:nout], r.y[g][pos:pos + nout]), k
        pos += nout
    assert pos == r.plain.numel()
    # bad values are refused and change nothing
    assert L.msresamp_hip_set_output_format(h, 2) == product.MCRX_EINVAL
    assert L.msresamp_hip_set_output_gain(h, float("nan")) == product.MCRX_EINVAL
    assert L.msresamp_hip_set_output_gain(h, float("inf")) == product.MCRX_EINVAL
    assert (rs.output_format, rs.gain) == settings[-1]
    with pytest.raises(ValueError):
        rs.gain = float("inf")
    rs.close()


# ---------------------------------------------------------------------------------------------- 5. clipping
@pytest.mark.parametrize("rate", CLIP_RATES)
def test_clipping(product, rate):
    torch = _torch()
    r = ref(product, rate)
    n = int(r.plain.numel())
    mag = torch.view_as_real(r.plain).abs().max(dim=1).values.cpu().numpy()
    g_clip = float(np.float32(1.0 / np.quantile(mag, 0.8)))                     # a fifth of the samples reach full scale
    g_safe = float(np.float32(0.5 / mag.max()))
    rs_f = product.msresamp(rate, gain=g_clip)
    y = rs_f.execute(r.d_x)
    want = model.clipped_samples(y.cpu().numpy())
    assert 0.01 * n < want < 0.5 * n, (want, n)                                # (the model first)
    rs_f.gain = g_safe
    rs_f.reset()
    y_safe = rs_f.execute(r.d_x)
    assert model.clipped_samples(y_safe.cpu().numpy()) == 0
    assert rs_f.clipped() == 0                                                 # a cf32 handle counts nothing
    rs_f.close()

    rs = product.msresamp(rate, output_format="sc16", gain=g_clip)
    assert rs.clipped() == 0
    got = rs.execute(r.d_x)
    assert rs.clipped() == want
    assert torch.equal(got, Q(y))
    assert int(got.min()) == -32768 and int(got.max()) == 32767                # saturated, not wrapped
    rs.reset()
    rs.execute(r.d_x)
    assert rs.clipped() == 2 * want                                            # it accumulates
    assert rs.clipped(reset=True) == 2 * want
    assert rs.clipped() == 0                                                   # ... and starts again
    rs.reset()
    rs.execute(r.d_x)
    assert rs.clipped(reset=True) == want
    rs.gain = g_safe
    rs.reset()
    got = rs.execute(r.d_x)
    assert rs.clipped() == 0
    assert torch.equal(got, Q(y_safe))
    rs.close()


def test_clip_count_across_a_format_switch(product):
    """The resampler's read-out rule: clipped() reports the count whatever the handle's format is now (the transmitter's reports 0
    while it is cf32: tests/test_gpu_tx_sc16.py), and only sc16 calls add to it."""
    rate = CLIP_RATES[0]
    x = ref(product, rate).d_x[:3001]
    rs_f = product.msresamp(rate)
    mag = np.abs(rs_f.execute(x).cpu().numpy().view(np.float32))
    g_clip = float(np.float32(1.0 / np.quantile(mag, 0.9)))
    rs_f.gain = g_clip
    rs_f.reset()
    want = model.clipped_samples(rs_f.execute(x).cpu().numpy())
    rs_f.close()
    assert want > 0
    rs = product.msresamp(rate, output_format="sc16", gain=g_clip)
    rs.execute(x)
    assert rs.clipped() == want
    rs.output_format = "cf32"
    assert rs.output_format == 0 and rs.clipped() == want
    rs.reset()
    rs.execute(x)                                                              # a cf32 call adds nothing
    assert rs.clipped() == want
    rs.output_format = "sc16"
    rs.reset()
    rs.execute(x)
    assert rs.clipped() == 2 * want
    rs.close()


# ---------------------------------------------------------------------------------------------- 6. NaN and infinities
def test_nan_and_infinities(product):
    torch = _torch()
    rate = 2.0
    r = ref(product, rate)
    x = r.d_x.clone()
    x[1000] = complex(float("inf"), 0.25)
    x[3000] = complex(-0.125, float("nan"))
    rs_f, rs_i = product.msresamp(rate, gain=GAIN), product.msresamp(rate, output_format="sc16", gain=GAIN)
    y, got = rs_f.execute(x), rs_i.execute(x)
    yr = torch.view_as_real(y)
    assert bool(torch.isinf(yr).any()) and bool(torch.isnan(yr).any())
    assert torch.equal(got, Q(y))
    assert bool((got[torch.isnan(yr)] == 0).all())                             # NaN stores 0
    want = model.clipped_samples(y.cpu().numpy())
    assert want > 0 and rs_i.clipped() == want                                 # the infinities count, NaN does not
    rs_f.close(); rs_i.close()


# ---------------------------------------------------------------------------------------------- 7. end to end
def frame_words(f):
    """every field of a delivered frame, floats as their bits"""
    return (f.channel, f.header, f.header_valid, f.payload, f.payload_valid, struct.pack("<3f", f.evm, f.rssi, f.cfo),
            f.mod_scheme, f.mod_bps, f.check, f.fec0, f.fec1, f.end_sample, f.framesyms.view(np.uint32).tobytes())


def test_end_to_end_radio_chain(product):
    """multichanneltx -> msresamp(2.0, sc16 out, gain g) -> sc16 msresamp(0.5) -> multichannelrx: the int16 stream is the one the torch
    quantisation pass makes from the cf32 interpolator's output at the same gain, and the frames are that chain's and what was sent."""
    torch = _torch()
    N, M, cp, taper, nf, plen = 4, 64, 8, 4, 3, 64
    tile = product.TILE * 2 * N
    tx = product.multichanneltx(N, M, cp, taper)
    iq, sent = tx.generate(nf, plen, gain=1.0 / N, seed=2024)                   # QPSK / h128
    iq = torch.cat([iq, torch.zeros(4 * tile, dtype=torch.complex64, device="cuda")])          # (the resamplers' delay)
    tx.close()
    up = product.msresamp(2.0)
    peak = float(torch.view_as_real(up.execute(iq)).abs().max())
    up.close()
    assert peak > 0
    g = float(np.float32(0.5 / peak))                                           # the peak at half of full scale: nothing clips
    up_f, up_i = product.msresamp(2.0, gain=g), product.msresamp(2.0, output_format="sc16", gain=g)
    v = torch.view_as_real(up_f.execute(iq)).contiguous()
    rnd = torch.round(v * 32768.0)
    d_ref = torch.clamp(rnd, -32768.0, 32767.0).to(torch.int16)                 # the pass sc16 output replaces
    assert torch.equal(d_ref.to(torch.float32), rnd) and 8000 < int(d_ref.abs().max()) < 32767
    d_q = up_i.execute(iq)
    assert d_q.dtype == torch.int16 and torch.equal(d_q, d_ref)
    assert up_i.clipped() == 0
    up_f.close(); up_i.close()
    frames = []
    for src in (d_q, d_ref):
        rs = product.msresamp(0.5, input_format="sc16")
        y = rs.execute(src)
        rs.close()
        rx = product.multichannelrx(N, M, cp, taper, max_payload_len=plen)
        n = int(y.numel()) // tile * tile
        rx.Execute(y[:n].contiguous()); rx.Flush()
        frames.append(list(rx.frames))
        rx.close()
    got, want = frames
    assert len(got) == N * nf and all(f.header_valid and f.payload_valid for f in got)
    assert len(got) == len(want)
    for fa, fb in zip(got, want):
        assert frame_words(fa) == frame_words(fb), (fa, fb)
    for f in got:
        assert sent[f.channel][(f.header[0] << 8) | f.header[1]] == (f.header, f.payload)
