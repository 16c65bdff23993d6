"""16-bit integer IQ (sc16) straight into the resampler: an sc16 sample (re, im) means (re * 2^-15, im * 2^-15), both steps exact in
fp32, and only the first stage's staging differs between the formats -- so everything an sc16 handle returns must equal, as raw
32-bit words, what a second cf32 handle returns on the dequantised floats pushed in the same pieces.  (The cf32 path is held to the
oracle by test_gpu_parity.test_msresamp_front_end_matches_oracle.)"""
import ctypes as C
import struct

import numpy as np
import pytest

import position_model as pm

pytestmark = pytest.mark.gpu

RATES = [0.5, 0.37, 0.8, 0.2, 0.11, 2.0, 1.5, 4.0, 6.3, 0.25, 0.45, 0.06]      # test_msresamp_front_end_matches_oracle's
ONE_SHOT_RATES = RATES + [0.7, 1.0]
STREAM_RATES = [0.5, 0.37, 0.2, 0.06, 1.5]
KEEP = 64           # RS_KEEP (csrc/msresamp.hip): samples of input history a handle retains


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def dequantise(q):
    """interleaved int16 -> complex64, the definition: exact"""
    return (q.astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64)


def words(t):
    """a complex64 device tensor as its raw 32-bit words"""
    import torch
    return torch.view_as_real(t).contiguous().view(torch.int32)


def same_words(a, b):
    import torch
    return a.numel() == b.numel() and torch.equal(words(a), words(b))


def stream_len(rate):
    """Inputs for which the arbitrary stage makes two full workgroups and a partial chunk (2 * 8192 + 1000 outputs, and a bit): it
    reads the caller's samples itself when interpolating, and sits behind num_stages halvings when decimating.  Odd."""
    plan = pm.ResampPlan(rate)
    return (int(17400 / plan.rate_arb) + 1) * plan.raw_per_arb() + 3


def samples(rate):
    """Seeded full-range int16 pairs, the four corners of the range planted at the start and at 64 random places, in both halves of
    the word."""
    n = stream_len(rate)
    rng = np.random.RandomState(int(rate * 1000) + 5)
    q = rng.randint(-32768, 32768, size=2 * n).astype(np.int16)
    q[:6] = [32767, -32768, -32768, 32767, -32767, -32768]
    at = rng.randint(0, n, size=64) * 2
    q[at] = np.where(rng.rand(64) < 0.5, 32767, -32768); q[at + 1] = np.where(rng.rand(64) < 0.5, -32768, 32767)
    return q


_ONE_SHOT = {}


def one_shot(product, rate):
    """(int16 samples, their floats, the output of one execute on an sc16 handle and on a cf32 handle) -- computed once per rate, on
    the device, and left alone"""
    if rate not in _ONE_SHOT:
        torch = _torch()
        q = samples(rate)
        d_q, d_x = torch.from_numpy(q).cuda(), torch.from_numpy(dequantise(q)).cuda()
        rs_i, rs_f = product.msresamp(rate, input_format="sc16"), product.msresamp(rate)
        assert (rs_i.input_format, rs_f.input_format) == (1, 0)
        y_i, y_f = rs_i.execute(d_q), rs_f.execute(d_x)
        torch.cuda.synchronize()
        rs_i.close(); rs_f.close()
        _ONE_SHOT[rate] = (d_q, d_x, y_i, y_f)
    return _ONE_SHOT[rate]


# ---------------------------------------------------------------------------------------------- 1. one-shot identity
@pytest.mark.parametrize("rate", ONE_SHOT_RATES)
def test_one_shot_identity(product, rate):
    """Every first-stage build: the arbitrary stage with a table (0.37, 0.45 with the half-band stage folded in, 0.7 plain) and with
    one branch per thread (0.25 folded, 0.5 / 0.8 / 1.0 plain), halfband_kernel in front (0.2, 0.11, 0.06), and the interpolating
    direction (the arbitrary stage first: 2.0 and 4.0 one branch per thread, 1.5 and 6.3 with a table)."""
    d_q, d_x, y_i, y_f = one_shot(product, rate)
    n = int(d_x.numel())
    assert d_q.numel() == 2 * n and y_f.numel() > 0.9 * rate * n
    peak = float(y_f.abs().max())
    assert np.isfinite(peak) and peak > 1e-3                                   # (the comparison below is not one of zeros)
    assert y_i.numel() == y_f.numel()
    assert same_words(y_i, y_f)
    # (n, 2) is the same buffer
    rs = product.msresamp(rate, input_format=1)
    assert same_words(rs.execute(d_q.view(-1, 2)), y_f)
    rs.close()


# ---------------------------------------------------------------------------------------------- 2. streamed identity
def ragged_pieces(n, seed):
    """Cuts of [0, n): pieces shorter than the retained history first (0, 1, 7, 63: the tail is built from tail + new samples over
    several calls), odd sizes (which break the parity of the folded half-band stage's vector loads), one large piece that starts
    at an odd sample -- a device pointer that is only 4-byte aligned in sc16 --, then seeded odds and ends."""
    rng = np.random.RandomState(seed)
    sizes = [1, 7, 0, 63, 1, 2, 777, (n // 3) | 1, 64, 4096, 0, 333]
    cuts, pos = [], 0
    for s in sizes:
        cuts.append((pos, min(pos + s, n))); pos = min(pos + s, n)
    while pos < n:
        s = int(rng.randint(1, 3000))
        cuts.append((pos, min(pos + s, n))); pos = min(pos + s, n)
    assert any(a % 2 == 1 and b - a > 2048 for a, b in cuts) and any(a % 2 == 0 and b - a >= 4096 for a, b in cuts)
    assert all(any(b - a == s for a, b in cuts) for s in (0, 1, 7, 63))
    return cuts


@pytest.mark.parametrize("rate", STREAM_RATES)
def test_streamed_identity(product, rate):
    torch = _torch()
    d_q, d_x, y_i, y_f = one_shot(product, rate)
    n = int(d_x.numel())
    rs_i, rs_f = product.msresamp(rate, input_format="sc16"), product.msresamp(rate)
    got_i, got_f = [], []
    for a, b in ragged_pieces(n, int(rate * 100)):
        piece = d_q[2 * a:2 * b]
        assert piece.data_ptr() % 4 == 0 and (a % 2 == 0 or piece.data_ptr() % 8 == 4)
        got_i.append(rs_i.execute(piece))
        got_f.append(rs_f.execute(d_x[a:b]))
        assert got_i[-1].numel() == got_f[-1].numel(), (a, b)
    z_i, z_f = torch.cat(got_i), torch.cat(got_f)
    assert same_words(z_i, y_i)                                                # the stream cut in pieces is the stream
    assert same_words(z_f, z_i)                                                # ... and the cf32 handle's, piece by piece
    # the same stream from a buffer that starts on an odd sample: every piece lies the other way round against 8 bytes
    shifted = torch.zeros(2 * n + 2, dtype=torch.int16, device="cuda")
    shifted[2:] = d_q
    rs_i.reset()
    got = []
    for a, b in ragged_pieces(n, int(rate * 100)):
        got.append(rs_i.execute(shifted[2 + 2 * a:2 + 2 * b]))
    assert shifted[2:].data_ptr() % 8 == 4
    assert same_words(torch.cat(got), y_i)
    rs_i.close(); rs_f.close()


# ---------------------------------------------------------------------------------------------- 3. positions
@pytest.mark.parametrize("rate", [0.37, 0.06])
def test_positions(product, rate):
    """After reset(at=p) the two formats agree, p a multiple of 2^num_stages up to beyond 2^40, 2^48 and 2^56 -- aligned with the
    period of the phase (where the output is the origin's) and not."""
    torch = _torch()
    d_q, d_x, y_i, y_f = one_shot(product, rate)
    plan = pm.ResampPlan(rate)
    n = int(d_x.numel())
    unit = 1 << plan.num_stages
    rs_i, rs_f = product.msresamp(rate, input_format="sc16"), product.msresamp(rate)
    cuts = [(0, 1001), (1001, 1008), (1008, n)]
    for p in (unit * 12345, (1 << 40) + unit * 777, plan.aligned_raw_at_or_above(1 << 40), (1 << 48) + unit * 3, (1 << 56) + unit * 100001):
        assert p % unit == 0
        rs_i.reset(at=p); rs_f.reset(at=p)
        z_i = torch.cat([rs_i.execute(d_q[2 * a:2 * b]) for a, b in cuts])
        z_f = torch.cat([rs_f.execute(d_x[a:b]) for a, b in cuts])
        assert z_f.numel() > 0.9 * rate * n and float(z_f.abs().max()) > 1e-3
        assert same_words(z_i, z_f), p
        if p == plan.aligned_raw_at_or_above(1 << 40):
            assert same_words(z_i, y_i)
    rs_i.close(); rs_f.close()


# ---------------------------------------------------------------------------------------------- 4. format rules
def test_format_rules(product):
    torch = _torch()
    L = product.lib()
    rate = 0.37
    d_q, d_x, y_i, y_f = one_shot(product, rate)
    n = 5000
    cap = n
    rs = product.msresamp(rate)
    h = rs._h
    assert L.msresamp_hip_input_format(h) == 0
    assert L.msresamp_hip_set_input_format(h, 2) == product.MCRX_EINVAL
    assert L.msresamp_hip_set_input_format(h, 1) == product.MCRX_OK and L.msresamp_hip_input_format(h) == 1     # a fresh handle
    assert L.msresamp_hip_set_input_format(h, 0) == product.MCRX_OK and L.msresamp_hip_input_format(h) == 0
    assert L.msresamp_hip_set_input_format(h, 1) == product.MCRX_OK
    out = torch.zeros(cap, dtype=torch.complex64, device="cuda")
    nout = C.c_size_t(77)

    def call(fn, src, count):
        return fn(h, C.c_void_p(src.data_ptr()), count, C.c_void_p(out.data_ptr()), cap, C.byref(nout), None)

    # a call of the other format's kind: MCRX_EINVAL, nothing consumed
    assert call(L.msresamp_hip_execute_device, d_x, n) == product.MCRX_EINVAL
    assert b"format" in L.msresamp_hip_last_error()
    assert L.msresamp_hip_set_input_format(h, 1) == product.MCRX_OK                # (still no history)
    assert call(L.msresamp_hip_execute_device_sc16, d_q, n) == product.MCRX_OK
    torch.cuda.synchronize()
    n1 = int(nout.value)
    assert n1 > 0.9 * rate * n - 64 and same_words(out[:n1], y_i[:n1])
    # the handle holds input history now
    assert L.msresamp_hip_set_input_format(h, 0) == product.MCRX_EBUSY
    assert L.msresamp_hip_set_input_format(h, 1) == product.MCRX_EBUSY
    assert L.msresamp_hip_input_format(h) == 1
    # in mid-stream: the refused call leaves the state alone, the next correct one continues the stream
    assert call(L.msresamp_hip_execute_device, d_x[n:], n) == product.MCRX_EINVAL
    assert call(L.msresamp_hip_execute_device_sc16, d_q[2 * n:], n) == product.MCRX_OK
    torch.cuda.synchronize()
    n2 = int(nout.value)
    assert n2 > 0 and same_words(out[:n2], y_i[n1:n1 + n2])
    # the Python face raises on the other format's dtype
    with pytest.raises(TypeError):
        rs.execute(d_x[:64])
    rs.reset()
    assert L.msresamp_hip_set_input_format(h, 0) == product.MCRX_OK and rs.input_format == 0     # after a reset it may change again
    assert call(L.msresamp_hip_execute_device_sc16, d_q, n) == product.MCRX_EINVAL
    with pytest.raises(TypeError):
        rs.execute(d_q[:128])
    y = rs.execute(d_x[:n])                                                      # an undisturbed cf32 handle's output
    assert y.numel() == n1 and same_words(y, y_f[:n1])
    assert L.msresamp_hip_set_input_format(h, 1) == product.MCRX_EBUSY
    rs.reset(at=1 << 20)
    assert L.msresamp_hip_set_input_format(h, 1) == product.MCRX_OK
    rs.close()


# ---------------------------------------------------------------------------------------------- 5. end to end
def frame_words(f):
    """every field of a delivered frame, floats as their bits"""
    return (f.channel, f.header, f.header_valid, f.payload, f.payload_valid, struct.pack("<3f", f.evm, f.rssi, f.cfo),
            f.mod_scheme, f.mod_bps, f.check, f.fec0, f.fec1, f.end_sample, f.framesyms.view(np.uint32).tobytes())


def same_frames(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for fa, fb in zip(a, b):
        assert frame_words(fa) == frame_words(fb), (fa, fb)


def test_end_to_end_radio_chain(product):
    """multichanneltx -> msresamp(2.0) -> a radio's int16 -> sc16 msresamp(0.5) -> multichannelrx: the frames are, field for field
    and symbol bit for symbol bit, those of the chain with a cf32 resampler on the dequantised floats, and what was sent."""
    torch = _torch()
    N, M, cp, taper, nf, plen = 4, 64, 8, 4, 3, 64
    tile = product.TILE * 2 * N
    tx = product.multichanneltx(N, M, cp, taper)

    def antenna(gain):
        iq, sent = tx.generate(nf, plen, gain=gain, seed=2024)                  # QPSK / h128
        iq = torch.cat([iq, torch.zeros(4 * tile, dtype=torch.complex64, device="cuda")])      # (the resamplers' delay)
        up = product.msresamp(2.0)
        v = up.execute(iq)
        up.close()
        return torch.view_as_real(v).contiguous().view(-1), sent

    v0, _ = antenna(1.0 / N)
    peak0 = float(v0.abs().max())
    assert peak0 > 0
    v, sent = antenna(0.5 / (N * peak0))                                        # half of full scale: nothing clips
    r = torch.round(v * 32768.0)
    d_q = torch.clamp(r, -32768.0, 32767.0).to(torch.int16)
    assert torch.equal(d_q.to(torch.float32), r) and 8000 < int(d_q.abs().max()) < 32767
    tx.close()
    d_x = torch.view_as_complex((d_q.to(torch.float32) * 2.0 ** -15).view(-1, 2))
    frames = []
    for sc16 in (True, False):
        rs = product.msresamp(0.5, input_format="sc16" if sc16 else "cf32")
        y = rs.execute(d_q if sc16 else d_x)
        rs.close()
        rx = product.multichannelrx(N, M, cp, taper, max_payload_len=plen)
        n = int(y.numel()) // tile * tile
        rx.Execute(y[:n].contiguous()); rx.Flush()
        frames.append(list(rx.frames))
        rx.close()
    got_i, got_f = frames
    assert len(got_i) == N * nf and all(f.header_valid and f.payload_valid for f in got_i)
    same_frames(got_i, got_f)
    for f in got_i:
        assert sent[f.channel][(f.header[0] << 8) | f.header[1]] == (f.header, f.payload)
