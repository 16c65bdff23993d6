"""16-bit integer IQ (sc16) straight out of the transmitter (mctx_hip_set_output_format(q, 1)).  An sc16 transmitter stores
Q(v) = clamp(rint(v * 32768), -32768, 32767) of the fp32 value v a cf32 transmitter stores, so its output is a function of the cf32
output alone: the reference everywhere below is a cf32 transmitter of the same process with the same arguments and seed (which the
existing tests hold to the oracle), put through the numpy quantiser of tests/tx_sc16_model.py -- exact equality, no tolerance.

(The shape (6, 64, 8, 4) -- K = 12, no power of two -- is not among the identity cases: mctx_hip_create refuses it with MCRX_EUNSUPP,
for either format.)

The clip count at gain 1 / N.  The traffic does not stay inside full scale at the default gain: the preamble symbols of all channels
start together and their peaks add up (CPU oracle, same recipe and gain: largest component 2.70 of full scale at N = 1, 2.04 at N = 8
and N = 16; 2137 of 7488, 403 of 59904 and 361 of 119808 samples outside the range).  A count of 0 is therefore not what a correct
transmitter reports there; the identity tests hold clipped() to the numpy count of the cf32 stream instead -- which is 0 exactly where
the stream stays in range, and is the contract the clipping test states."""
import ctypes as C
import struct

import numpy as np
import pytest

import tx_sc16_model as model

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def pair(product, N, M, cp, taper):
    return product.multichanneltx(N, M, cp, taper), product.multichanneltx(N, M, cp, taper, output_format="sc16")


def check_identity(iq_f, iq_i):
    """the int16 tensor is the model of the cf32 one; returns the cf32 samples (host)"""
    torch = _torch()
    assert iq_i.dtype == torch.int16 and iq_i.is_contiguous() and tuple(iq_i.shape) == (int(iq_f.numel()), 2)
    x = iq_f.cpu().numpy()
    peak = float(np.abs(x.view(np.float32)).max())
    assert np.isfinite(peak) and peak > 1e-3                        # (not a comparison of zeros)
    got, want = iq_i.cpu().numpy(), model.quantise_iq(x)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], want[bad[:8]])
    return x


# ---------------------------------------------------------------------------------------------- 1. identity, path by path
SHAPES = [(1, 64, 8, 4),        # K = 2
          (8, 64, 8, 4),        # K = 16: the two-kernel path (txifft + txfir)
          (64, 64, 8, 4),       # K = 128: the smallest fused kernel, block walk
          (256, 64, 8, 2),      # K = 512, aligned loader
          (256, 64, 8, 8),      # K = 512, block walk (taper > 4)
          (256, 48, 6, 4),      # K = 512, M = 48 / cp = 6: block walk
          (512, 64, 8, 3)]      # K = 1024


@pytest.mark.parametrize("N,M,cp,taper", SHAPES)
def test_identity_per_synthesis_path(product, N, M, cp, taper):
    tx_f, tx_i = pair(product, N, M, cp, taper)
    assert (tx_f.output_format, tx_i.output_format) == (0, 1)
    iq_f, sent_f = tx_f.generate(2, 100, seed=1234 + N)             # QPSK / h128, gain 1 / N
    iq_i, sent_i = tx_i.generate(2, 100, seed=1234 + N)
    x = check_identity(iq_f, iq_i)
    print("N=%d M=%d cp=%d taper=%d: peak component %.4f of full scale" % (N, M, cp, taper, np.abs(x.view(np.float32)).max()))
    assert sent_i == sent_f
    assert tx_i.clipped() == model.clipped_samples(x) and tx_f.clipped() == 0
    tx_f.close(); tx_i.close()


@pytest.mark.parametrize("N,M,cp", [(4, 64, 8), (256, 64, 8)])
def test_identity_ragged(product, N, M, cp):
    """1024 blocks are 14 OFDM symbols: room for one short frame per channel (12 or 13 symbols at payloads of 0 .. 8 bytes, no gap in
    front: with one the longer ones would not fit)."""
    tx_f, tx_i = pair(product, N, M, cp, 4)
    kw = dict(len_lo=0, len_hi=8, gap_max=0, long_every=0, long_max=0, seed=99)
    iq_f, sent_f, starts_f = tx_f.generate_ragged(1024, **kw)
    iq_i, sent_i, starts_i = tx_i.generate_ragged(1024, **kw)
    assert sum(len(s) for s in sent_f) >= N // 2                    # (there is traffic)
    x = check_identity(iq_f, iq_i)
    assert sent_i == sent_f and starts_i == starts_f
    assert tx_i.clipped() == model.clipped_samples(x)
    tx_f.close(); tx_i.close()


@pytest.mark.parametrize("keep", [16, 13])
def test_identity_synthesize_from_exchanged_tiles(product, keep):
    """N = 256 from the granules of two channel shards, as tests/test_gpu_txshard.py builds them: lead - keep = 32 takes the fused
    kernel's granule loader, 35 (no multiple of 8) the two-kernel path.  Both handles read the same tiles."""
    torch = _torch()
    from liquid_usrp_amd import sharding
    N, M, cp, world, Tc, lead, nf, plen = 256, 64, 8, 2, 256, 48, 2, 100
    K, cg = 2 * N, N // world
    tx_f, tx_i = pair(product, N, M, cp, 4)
    trs = []
    for r in range(world):
        c0, cnt = sharding.shard_of(r, world, N)
        trs.append(tx_f.traffic(c0, cnt, nf, plen, seed=4242))
    per = (lead + Tc) * cg
    nclip = 0
    for u in (0, 3):                                                # the stream's first sub-slab (zeros in front) and an interior one
        recv = torch.empty(world * per, dtype=torch.complex64, device="cuda")
        for s in range(world):
            trs[s].tiles(u * Tc - lead, lead + Tc, recv[s * per:(s + 1) * per])
        torch.cuda.synchronize()
        iq_f = tx_f.synthesize(recv, world, u * Tc, Tc, lead, keep)
        iq_i = tx_i.synthesize(recv, world, u * Tc, Tc, lead, keep)
        torch.cuda.synchronize()
        assert int(iq_f.numel()) == (keep + Tc) * K
        nclip += 2 * model.clipped_samples(check_identity(iq_f, iq_i))      # (two sc16 calls per sub-slab: the one below too)
        out = torch.zeros(((keep + Tc) * K, 2), dtype=torch.int16, device="cuda")       # ... and into a caller's buffer
        assert tx_i.synthesize(recv, world, u * Tc, Tc, lead, keep, out=out) is out
        torch.cuda.synchronize()
        assert torch.equal(out, iq_i)
    assert tx_i.clipped() == nclip
    for t in trs:
        t.close()
    tx_f.close(); tx_i.close()


# ---------------------------------------------------------------------------------------------- 2. clipping
@pytest.mark.parametrize("N", [8, 256])
def test_clipping_is_the_clamp_and_is_counted(product, N):
    """Gain set so that the 99th percentile of |re|, |im| sits at full scale: about 2 % of the samples clip.  The integers are the
    clamp of the model and clipped() is the model's count, on the two-kernel path (N = 8) and the fused kernel (N = 256)."""
    tx_f, tx_i = pair(product, N, 64, 8, 4)
    gain0 = 1.0 / N
    x0 = tx_f.generate(2, 100, gain=gain0, seed=31)[0].cpu().numpy()
    p = float(np.percentile(np.abs(x0.view(np.float32)), 99.0))
    assert p > 0
    gain = gain0 / p
    iq_f, _ = tx_f.generate(2, 100, gain=gain, seed=31)
    iq_i, _ = tx_i.generate(2, 100, gain=gain, seed=31)
    x = check_identity(iq_f, iq_i)
    want = model.clipped_samples(x)
    print("N=%d: gain %.4g, %d of %d samples clipped" % (N, gain, want, x.size))
    assert 0 < want < x.size // 2
    got = iq_i.cpu().numpy()
    assert got.max() == 32767 and got.min() == -32768
    assert tx_i.clipped() == want
    assert tx_i.clipped() == want                                   # (reading does not reset)
    iq_i2, _ = tx_i.generate(2, 100, gain=gain, seed=31)            # every sample-producing call adds
    assert tx_i.clipped(reset=True) == 2 * want
    assert tx_i.clipped() == 0
    assert tx_f.clipped() == 0 and tx_f.clipped(reset=True) == 0    # a cf32 handle reports 0 throughout
    tx_f.close(); tx_i.close()


def test_clip_count_across_a_format_switch(product):
    """The transmitter's read-out rule: clipped() is 0 while the handle's format is cf32, and what the sc16 calls counted is still
    there when the handle is sc16 again (the resampler's rule differs: tests/test_gpu_resamp_sc16_out.py)."""
    L = product.lib()
    tx_f, tx_i = pair(product, 8, 64, 8, 4)
    gain0 = 1.0 / 8
    x0 = tx_f.generate(1, 20, gain=gain0, seed=31)[0].cpu().numpy()
    p = float(np.percentile(np.abs(x0.view(np.float32)), 99.0))
    assert p > 0
    gain = gain0 / p
    want = model.clipped_samples(tx_f.generate(1, 20, gain=gain, seed=31)[0].cpu().numpy())
    assert want > 0
    tx_i.generate(1, 20, gain=gain, seed=31)
    assert tx_i.clipped() == want
    assert L.mctx_hip_set_output_format(tx_i._h, 0) == product.MCRX_OK and tx_i.output_format == 0
    assert tx_i.clipped() == 0
    assert L.mctx_hip_set_output_format(tx_i._h, 1) == product.MCRX_OK and tx_i.output_format == 1
    assert tx_i.clipped() == want
    assert tx_i.clipped(reset=True) == want
    assert tx_i.clipped() == 0
    tx_f.close(); tx_i.close()


# ---------------------------------------------------------------------------------------------- 3. the quantiser itself
def test_selftest_quantise_reaches_ties_and_edges(product):
    _torch()
    lsb = []
    for k in (0, 1, 2, 3, 4, 5, 100, 101, 4094, 4095, 32765, 32766):
        lsb += [k + 0.5, -(k + 0.5)]                                # even and odd k, both signs
    lsb += [32767.4, -32767.4, 32767.5, -32767.5, -32768.5, -32768.6, 1e9, -1e9]
    v = (np.array(lsb, np.float64) / 32768.0).astype(np.float32)
    v = np.concatenate([v, np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-45, -1e-45], np.float32),
                        np.random.RandomState(5).uniform(-1.2, 1.2, 4096).astype(np.float32)])
    out = np.full(v.size, 12345, np.int16)
    assert product.lib().mctx_hip_selftest_quantise(v.ctypes.data, out.ctypes.data, v.size) == product.MCRX_OK
    want = model.quantise(v)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, (v[bad[:8]], out[bad[:8]], want[bad[:8]])
    assert out[:4].tolist() == [0, 0, 2, -2]                        # (0.5 -> 0, 1.5 -> 2: the model itself is pinned in test_tx_sc16.py)


# ---------------------------------------------------------------------------------------------- 4. loopback
def frame_words(f):
    return (f.channel, f.header, f.header_valid, f.payload, f.payload_valid, struct.pack("<3f", f.evm, f.rssi, f.cfo),
            f.mod_scheme, f.mod_bps, f.check, f.fec0, f.fec1, f.end_sample, f.framesyms.view(np.uint32).tobytes())


def test_loopback_into_an_sc16_receiver(product):
    torch = _torch()
    N, M, cp, nf, plen = 16, 64, 8, 3, 400
    tx = product.multichanneltx(N, M, cp, 4, output_format="sc16")
    iq, sent = tx.generate(nf, plen, seed=2024)
    rx_i = product.multichannelrx(N, M, cp, 4, max_payload_len=plen, input_format="sc16")
    rx_i.Execute(iq)                                                # the tensor as it stands
    rx_i.Flush()
    assert len(rx_i.frames) == N * nf
    for f in rx_i.frames:
        assert f.header_valid and f.payload_valid
        assert sent[f.channel][(f.header[0] << 8) | f.header[1]] == (f.header, f.payload)
    rx_f = product.multichannelrx(N, M, cp, 4, max_payload_len=plen)
    rx_f.Execute(torch.view_as_complex((iq.float() * 2.0 ** -15).contiguous()))
    rx_f.Flush()
    assert len(rx_f.frames) == len(rx_i.frames)
    for a, b in zip(rx_i.frames, rx_f.frames):
        assert frame_words(a) == frame_words(b)
    rx_i.close(); rx_f.close(); tx.close()


# ---------------------------------------------------------------------------------------------- 5. interface
def test_interface_refusals(product):
    torch = _torch()
    L = product.lib()
    tx_f, tx_i = pair(product, 4, 64, 8, 4)
    assert L.mctx_hip_set_output_format(tx_f._h, 2) == product.MCRX_EINVAL
    assert L.mctx_hip_output_format(tx_f._h) == 0
    assert L.mctx_hip_set_output_format(tx_f._h, 1) == product.MCRX_OK and tx_f.output_format == 1       # (before streaming: free to change)
    assert L.mctx_hip_set_output_format(tx_f._h, 0) == product.MCRX_OK and tx_f.output_format == 0
    tx_f.GenerateSamples()
    assert L.mctx_hip_set_output_format(tx_f._h, 1) == product.MCRX_EBUSY
    assert tx_f.output_format == 0
    # the host paths are cf32 only
    for call in (lambda: tx_i.GenerateSamples(), lambda: tx_i.UpdateData(0, b"\0" * 8, b"abc"), lambda: tx_i.frame(b"\0" * 8, b"abc")):
        with pytest.raises(product.McrxError) as ei:
            call()
        assert "sc16" in str(ei.value)
    assert L.mctx_hip_stream_begin(tx_i._h, 64) == product.MCRX_EUNSUPP
    # synthesize(out=...) of the wrong dtype for the handle, both ways
    tiles = torch.zeros((48 + 64) * 4, dtype=torch.complex64, device="cuda")
    with pytest.raises(TypeError):
        tx_i.synthesize(tiles, 1, 0, 64, 48, 16, out=torch.zeros((16 + 64) * 8, dtype=torch.complex64, device="cuda"))
    with pytest.raises(TypeError):
        tx_f.synthesize(tiles, 1, 0, 64, 48, 16, out=torch.zeros(((16 + 64) * 8, 2), dtype=torch.int16, device="cuda"))
    out = tx_i.synthesize(tiles, 1, 0, 64, 48, 16)                  # (the right one goes through: silence in, zeros out)
    torch.cuda.synchronize()
    assert out.dtype == torch.int16 and tuple(out.shape) == ((16 + 64) * 8, 2) and int(out.abs().max()) == 0
    n = C.c_uint64(9)
    assert L.mctx_hip_clipped(tx_i._h, C.byref(n), 0) == product.MCRX_OK and n.value == 0
    tx_f.close(); tx_i.close()


def test_tx_pipeline_allocates_in_the_transmitters_format(product):
    torch = _torch()
    from liquid_usrp_amd import sharding
    N, M, cp, Tc = 32, 64, 8, 256
    dev = torch.device("cuda", 0)
    slabs = {}
    for fmt in ("cf32", "sc16"):
        tx = product.multichanneltx(N, M, cp, 4, output_format=fmt)
        tr = tx.traffic(0, N, 1, 60, seed=7)
        txp = sharding.TxPipeline(tx, tr, 0, 1, None, N, Tc, device=dev)
        assert txp.recv[0].dtype == torch.complex64
        got = []
        for c in range(2):
            iq, ev = txp.push()
            ev.synchronize()
            got.append(iq.clone())
        slabs[fmt] = got
        torch.cuda.synchronize()
        tr.close(); tx.close()
    for f, i in zip(slabs["cf32"], slabs["sc16"]):
        check_identity(f, i)
