"""16-bit integer IQ (sc16) straight into the channelizer: an sc16 sample (re, im) means (re * 2^-15, im * 2^-15), both steps exact in
fp32, so everything an sc16 handle produces must equal, bit for bit, what a cf32 handle produces on the dequantised floats pushed in
the same pieces -- channel tiles, frames, equalised symbols, the monitor's sums.  The cf32 handle in turn is held to the oracle on those
floats at the project's bar (payloads exact, symbols <= 1e-5: test_gpu_parity.check_frames)."""
import ctypes as C
import struct

import numpy as np
import pytest

from test_gpu_parity import check_frames

pytestmark = pytest.mark.gpu


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


# ---------------------------------------------------------------------------------------------- 1. stage identity
def slabs_per_workgroup(K, front_end):
    """csrc/channelizer.hip: threads per workgroup / threads per slab"""
    T = 512 if (K >= 1024 or (front_end and K >= 512)) else 256
    Cc = 2 if K >= 4 else 1
    return T // (K // Cc)


@pytest.mark.parametrize("N,front_end", [(1, 0), (2, 0), (8, 0), (64, 0), (512, 0), (3, 0), (8, 1), (512, 1)])
def test_stage_identity(product, N, front_end):
    """mcrx_hip_channelize on the sc16 handle == the cf32 handle fed float(v) * 2^-15, as raw words: cold and with a halo.  Slabs of 32
    blocks and three workgroups and a bit, so that the first one (history in front of the stream), an interior one (the build without
    clamps and masks) and the last ones (past the end) all run; N = 3 goes through the generic kernel."""
    torch = _torch()
    K = 2 * N
    pow2 = K & (K - 1) == 0
    nblocks = 32 * (3 * slabs_per_workgroup(K, front_end) + 1) if pow2 else 96
    rng = np.random.RandomState(1000 * front_end + N)
    q = rng.randint(-32768, 32768, size=2 * nblocks * K).astype(np.int16)
    q[:6] = [32767, -32768, -32768, 32767, -32767, -32768]                  # the corners of the range, in both halves of the word
    at = rng.randint(0, nblocks * K, size=64) * 2
    q[at] = np.where(rng.rand(64) < 0.5, 32767, -32768); q[at + 1] = np.where(rng.rand(64) < 0.5, -32768, 32767)
    x = dequantise(q)
    d_q, d_x = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda()
    cfg = dict(slab_blocks=32, front_end=front_end)
    rx_f = product.multichannelrx(N, 64, 8, 4, **cfg)
    rx_i = product.multichannelrx(N, 64, 8, 4, input_format="sc16", **cfg)
    H = rx_i.history_blocks()
    assert H == rx_f.history_blocks() == (27 if front_end else 13)
    out_f = torch.zeros(nblocks * N, dtype=torch.complex64, device="cuda"); out_i = torch.full_like(out_f, 7.0)
    rx_f.channelize(d_x, nblocks, 0, out_f)
    rx_i.channelize(d_q, nblocks, 0, out_i)
    torch.cuda.synchronize()
    peak = float(out_f.abs().max())
    assert np.isfinite(peak) and peak > 1e-3                                   # (the comparison below is not one of zeros)
    assert torch.equal(words(out_i), words(out_f))
    # with a halo, from a tile boundary that is no slab boundary of the first call, at a non-zero oscillator phase
    h = 48
    nb = nblocks - h
    o_f = torch.zeros(nb * N, dtype=torch.complex64, device="cuda"); o_i = torch.full_like(o_f, 7.0)
    rx_f.channelize(d_x[h * K:], nb, h * K, o_f, d_halo=d_x[(h - H) * K:h * K])
    rx_i.channelize(d_q[2 * h * K:], nb, h * K, o_i, d_halo=d_q[2 * (h - H) * K:2 * h * K])
    torch.cuda.synchronize()
    assert torch.equal(words(o_i), words(o_f))
    assert torch.equal(words(o_f), words(out_f[h * N:]))                       # (and the halo made it the same stream)
    rx_f.close(); rx_i.close()


# ---------------------------------------------------------------------------------------------- 2., 3. receiver identity, monitor
def frame_words(f):
    """every field of a delivered frame, floats as their bits"""
    return (f.channel, f.header, f.header_valid, f.payload, f.payload_valid, struct.pack("<3f", f.evm, f.rssi, f.cfo),
            f.mod_scheme, f.mod_bps, f.check, f.fec0, f.fec1, f.end_sample, f.framesyms.view(np.uint32).tobytes())


def same_frames(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for fa, fb in zip(a, b):
        assert frame_words(fa) == frame_words(fb), (fa, fb)


class Case(object):
    pass


CASES = {
    "qpsk_h128": dict(N=8, M=64, cp=8, mod=40, fec1=6, plen=200, nf=4, front_end=0),
    "qam16_g2412_ovs": dict(N=64, M=256, cp=32, mod=27, fec1=7, plen=120, nf=2, front_end=1),
}


def device_pieces(n, tile, seed):
    """uneven pushes of whole tiles"""
    rng = np.random.RandomState(seed)
    cuts, i = [], 0
    while i < n:
        step = tile * int(rng.randint(1, max(2, n // tile // 5)))
        cuts.append((i, min(i + step, n))); i += step
    return cuts


def host_pieces(n, K, seed):
    """odd pushes that respect neither blocks nor tiles"""
    rng = np.random.RandomState(seed)
    cuts, i = [], 0
    while i < n:
        step = 2 * int(rng.randint(K, 40 * K)) + 1
        cuts.append((i, min(i + step, n))); i += step
    return cuts


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request, product):
    """The traffic of one configuration, quantised, and what a cf32 and an sc16 receiver make of it, pushed in the same pieces:
    once from device memory (monitor on), once from host memory through small stagings."""
    torch = _torch()
    p = CASES[request.param]
    c = Case()
    c.p, c.N, c.K = p, p["N"], 2 * p["N"]
    tx = product.multichanneltx(c.N, p["M"], p["cp"], 4)
    iq, c.sent = tx.generate(p["nf"], p["plen"], mod=p["mod"], fec1=p["fec1"], seed=77 + c.N)
    tx.close()
    tile = product.TILE * c.K
    c.n = int(iq.numel()) // tile * tile
    x = iq[:c.n].cpu().numpy()
    peak = float(max(np.abs(x.real).max(), np.abs(x.imag).max()))
    c.q = np.round(x.view(np.float32) * np.float32(0.45 / peak * 32768.0)).astype(np.int16)        # peak 0.45 of full scale
    assert np.abs(c.q).max() < 16384
    c.x = dequantise(c.q)
    c.cfg = dict(max_payload_len=max(p["plen"], 64), front_end=p["front_end"])
    d_q, d_x = torch.from_numpy(c.q).cuda(), torch.from_numpy(c.x).cuda()

    def run_device(sc16):
        rx = product.multichannelrx(c.N, p["M"], p["cp"], 4, input_format="sc16" if sc16 else "cf32", **c.cfg)
        rx.monitor_enable(64, "hann")
        for a, b in device_pieces(c.n, tile, 5):
            rx.Execute(d_q[2 * a:2 * b] if sc16 else d_x[a:b])
        rx.Flush()
        mon = rx.monitor_read()
        return rx, mon

    def run_host(sc16):
        rx = product.multichannelrx(c.N, p["M"], p["cp"], 4, input_format="sc16" if sc16 else "cf32", batch_samples=8 * tile, **c.cfg)
        for a, b in host_pieces(c.n, c.K, 6):
            rx.Execute(c.q[2 * a:2 * b] if sc16 else c.x[a:b])
        rx.Flush()
        return rx

    def run_bulk(sc16):
        """one large host push (>= 64 tiles with nothing staged: whole tiles go from the caller's memory to the device in chunks, past
        the staging buffer), cut so that a partial tile is left for the staging path, then the rest"""
        rx = product.multichannelrx(c.N, p["M"], p["cp"], 4, input_format="sc16" if sc16 else "cf32", **c.cfg)
        cut = c.n - tile // 2 - 37
        assert cut >= 64 * tile
        for a, b in ((0, cut), (cut, c.n)):
            rx.Execute(c.q[2 * a:2 * b] if sc16 else c.x[a:b])
        rx.Flush()
        return rx

    c.dev_f, c.mon_f = run_device(False)
    c.dev_i, c.mon_i = run_device(True)
    c.host_f, c.host_i = run_host(False), run_host(True)
    c.bulk_f, c.bulk_i = run_bulk(False), run_bulk(True)
    c.d_q, c.d_x, c.tile = d_q, d_x, tile
    yield c
    for rx in (c.dev_f, c.dev_i, c.host_f, c.host_i, c.bulk_f, c.bulk_i):
        rx.close()


def test_receiver_identity_device_pushes(case):
    c = case
    assert len(c.dev_f.frames) == c.N * c.p["nf"] and all(f.header_valid and f.payload_valid for f in c.dev_f.frames)
    same_frames(c.dev_i.frames, c.dev_f.frames)
    for f in c.dev_i.frames:
        assert c.sent[f.channel][(f.header[0] << 8) | f.header[1]] == (f.header, f.payload)


def test_receiver_identity_host_pushes(case):
    c = case
    assert len(c.host_f.frames) == c.N * c.p["nf"] and all(f.header_valid and f.payload_valid for f in c.host_f.frames)
    same_frames(c.host_i.frames, c.host_f.frames)


def test_receiver_identity_bulk_host_push(case):
    c = case
    assert len(c.bulk_f.frames) == c.N * c.p["nf"] and all(f.header_valid and f.payload_valid for f in c.bulk_f.frames)
    same_frames(c.bulk_i.frames, c.bulk_f.frames)
    for f in c.bulk_i.frames:
        assert c.sent[f.channel][(f.header[0] << 8) | f.header[1]] == (f.header, f.payload)


def test_cf32_result_on_the_dequantised_floats_matches_the_oracle(case, oracle):
    c = case
    ora = oracle.MultiChannelRx(c.N, c.p["M"], c.p["cp"], 4, **({"front_end": 1} if c.p["front_end"] else {}))
    ora.execute(c.x)
    assert len(ora.frames) == c.N * c.p["nf"] and all(f.payload_valid for f in ora.frames)
    check_frames(c.dev_f.frames, ora.frames)
    check_frames(c.host_f.frames, ora.frames)


def test_monitor_is_bit_equal(case):
    a, b = case.mon_i, case.mon_f
    assert (a.nseg, a.nsamp) == (b.nseg, b.nsamp) and a.nseg > 0
    assert a.level.tobytes() == b.level.tobytes() and a.peak.tobytes() == b.peak.tobytes() and a.psd.tobytes() == b.psd.tobytes()
    assert float(b.level.max()) > 0


# ---------------------------------------------------------------------------------------------- 4. guards and refusals
def test_format_guards_and_refusals(product):
    torch = _torch()
    L = product.lib()
    N, tile = 2, 16 * 4
    rx_f = product.multichannelrx(N, 64, 8, 4)
    rx_i = product.multichannelrx(N, 64, 8, 4, input_format=1)
    assert L.mcrx_hip_input_format(rx_f._h) == 0 and L.mcrx_hip_input_format(rx_i._h) == 1
    d = torch.zeros(2 * tile, dtype=torch.int16, device="cuda")
    z = np.zeros(2 * tile, np.int16)
    # a typed call on a handle of the other format: MCRX_EINVAL, both directions, nothing consumed
    assert L.mcrx_hip_execute_device(rx_i._h, d.data_ptr(), tile, None) == product.MCRX_EINVAL
    assert b"format" in L.mcrx_hip_last_error()
    assert L.mcrx_hip_execute_host(rx_i._h, z.ctypes.data, tile) == product.MCRX_EINVAL
    assert L.mcrx_hip_execute_device_sc16(rx_f._h, d.data_ptr(), tile, None) == product.MCRX_EINVAL
    assert L.mcrx_hip_execute_host_sc16(rx_f._h, z.ctypes.data, tile) == product.MCRX_EINVAL
    assert L.mcrx_hip_launches(rx_i._h) == 0 and L.mcrx_hip_launches(rx_f._h) == 0
    # ... and the Python face raises on the wrong dtype for the handle
    with pytest.raises(TypeError):
        rx_i.Execute(np.zeros(tile, np.complex64))
    with pytest.raises(TypeError):
        rx_i.Execute(torch.zeros(tile, dtype=torch.complex64, device="cuda"))
    with pytest.raises(TypeError):
        rx_f.Execute(z)
    with pytest.raises(TypeError):
        rx_f.Execute(d)
    rx_i.Execute(d); rx_i.Execute(z); rx_i.Flush()                           # (the right ones go through)
    assert L.mcrx_hip_launches(rx_i._h) == 2

    def create(**kw):
        c = product.Config()
        c.struct_size, c.payload_soft = C.sizeof(product.Config), 1
        for k, v in kw.items():
            setattr(c, k, v)
        h = C.c_void_p()
        rc = L.mcrx_hip_create(C.byref(h), 1 if kw.get("single_channel") else 4, 64, 8, 4, None, C.addressof(c))
        msg = L.mcrx_hip_last_error()
        if h.value:
            L.mcrx_hip_destroy(h)
        return rc, msg

    rc, msg = create(input_format=1, single_channel=1)
    assert rc == product.MCRX_EUNSUPP and b"single_channel" in msg
    rc, msg = create(input_format=1, front_end=2)
    assert rc == product.MCRX_EUNSUPP and b"front_end" in msg
    assert create(input_format=0, front_end=2)[0] == product.MCRX_OK
    assert create(input_format=2)[0] == product.MCRX_EINVAL
    # the multi-GPU pipeline moves cf32 sub-slabs
    ph = C.c_void_p()
    assert L.mcrx_hip_pipeline_create(C.byref(ph), rx_i._h, 0, 1, None, 64, 3) == product.MCRX_EUNSUPP
    assert b"sc16" in L.mcrx_hip_pipeline_last_error() and not ph.value
    rx_f.close(); rx_i.close()


# ---------------------------------------------------------------------------------------------- 5. reset
def test_reset_and_restart(case, product):
    """mcrx_hip_restart returns an sc16 handle to its first sample: the same stream gives the same frames, word for word.  After
    mcrx_hip_reset the oscillator keeps counting (the reference's Reset), so the frames are the cf32 handle's after the same calls --
    and, as bytes, the first pass's."""
    c = case
    first = list(c.dev_i.frames)
    rx = c.dev_i
    rx.restart()
    del rx.frames[:]
    for a, b in device_pieces(c.n, c.tile, 5):
        rx.Execute(c.d_q[2 * a:2 * b])
    rx.Flush()
    same_frames(rx.frames, first)
    # Reset in mid-stream, a partial tile staged: host pushes
    got = []
    for rxh, data, m in ((c.host_i, c.q, 2), (c.host_f, c.x, 1)):
        seen = len(rxh.frames)
        rxh.Execute(data[:m * (c.n // 3 + 5)])
        rxh.Reset()
        dropped = len(rxh.frames)
        for a, b in host_pieces(c.n, c.K, 9):
            rxh.Execute(data[m * a:m * b])
        rxh.Flush()
        got.append((rxh.frames[seen:dropped], rxh.frames[dropped:]))
    same_frames(got[0][0], got[1][0])
    same_frames(got[0][1], got[1][1])
    again = sorted((f.channel, f.header, f.payload, f.payload_valid) for f in got[0][1])
    assert again == sorted((f.channel, f.header, f.payload, f.payload_valid) for f in first)
