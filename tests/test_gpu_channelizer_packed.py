"""The channelizer's complex products as packed instructions, and its two carries for the next push (the bank's last blocks, the
synchronizers' history tiles) written by the kernel itself: neither may move a bit.  Everything here is compared as BYTES with
fixtures recorded from the library of the commit before that change (tests/golden/channelizer_packed_*.npz, written by
tests/golden/make_channelizer_packed.py: SHA-256 digests of the outputs, and of the inputs so that a drifting input is told from a
drifting kernel), and pushes cut differently are compared with each other.

Shapes: slabs of 16 blocks (two rounds of 8: both halves of a granule) and as few blocks as still hold an INTERIOR workgroup -- the
kernel's build without clamps and masks, which is the one that runs on all but two workgroups of a real push.  interior_workgroups()
below repeats the kernel's own dispatch test (channelizer_kernel: first >= 0 && last <= nblocks) and every stage case asserts that it
finds one: K = 1024 (one slab per workgroup) has them from 48 blocks on (64 with the 28-tap bank's 27 blocks of history); K = 128 runs
four slabs per workgroup, so its first interior workgroup needs 144 blocks.  The streaming cases are long enough by themselves and
say so the same way.

A frame's evm / rssi / cfo words and equalised symbols depend in their last bits on how a stream is cut into pushes (the acquisition takes
another route; so it was before this change), so differently cut streams are compared with each other on what they decode and where, and
word for word with the parent's frames for the SAME cuts."""
import hashlib
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SLAB = 16


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def dequantise(q):
    return (q.astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64)


def slabs_per_workgroup(K, front_end):
    """csrc/channelizer.hip (launch_format): threads per workgroup / threads per slab"""
    T = 512 if (K >= 1024 or (front_end and K >= 512)) else 256
    return T // (K // (2 if K >= 4 else 1))


def interior_workgroups(K, front_end, nblocks, slab):
    """workgroups whose every block -- history, slabs, the prefetch of one round past them -- lies inside the launch's x"""
    ns, H = slabs_per_workgroup(K, front_end), 27 if front_end else 13
    grid = ((nblocks + slab - 1) // slab + ns - 1) // ns
    return [w for w in range(grid) if w * ns * slab - H >= 0 and (w + 1) * ns * slab + 8 <= nblocks]


def auto_slab(K, nblocks, ncu):
    """csrc/channelizer.hip: channelizer_auto_slab, the slab of a launch whose handle names none"""
    threads, C = (512 if K >= 1024 else 256), (2 if K >= 4 else 1)
    ns = max(1, threads // (K // C))
    cap = ncu * (1 if K >= 1024 else 2) * ns
    k = (nblocks + cap * 512 - 1) // (cap * 512)
    slab = (nblocks + cap * k - 1) // (cap * k)
    return max(32, (slab + 15) // 16 * 16)


# ---------------------------------------------------------------------------------------------- stage level
STAGE_CASES = [(N, fe, fmt) for N in (64, 512) for fe in (0, 1) for fmt in ("cf32", "sc16")]
STAGE_IDS = ["K%d_%s_%s" % (2 * N, "p28" if fe else "p14", fmt) for N, fe, fmt in STAGE_CASES]
FIRST = 48 * 1024 + 37          # where x[0] sits in the stream: no multiple of anything, so the oscillator starts at a phase of its own


def stage_blocks(N):
    return 144 if N == 64 else 64


def stage_pieces(nblocks):
    """three uneven pieces of whole tiles, the middle one a single tile (16 blocks < history + 8)"""
    return [(0, 48), (48, 64), (64, nblocks)] if nblocks > 64 else [(0, 16), (16, 32), (32, nblocks)]


def run_stage(product, N, fe, fmt):
    """-> (digest of the input, the tiles of one call as bytes, the tiles of three calls as bytes)"""
    torch = _torch()
    K, nblocks = 2 * N, stage_blocks(N)
    assert interior_workgroups(K, fe, nblocks, SLAB), "no interior workgroup at this shape"
    rx = product.multichannelrx(N, 64, 8, 4, slab_blocks=SLAB, front_end=fe, input_format=fmt)
    H = rx.history_blocks()
    rng = np.random.RandomState(7000 + 10 * N + fe)
    q = rng.randint(-20000, 20001, size=2 * (H + nblocks) * K).astype(np.int16)
    m = 1 if fmt == "cf32" else 2           # array elements per sample
    data = torch.from_numpy(dequantise(q) if fmt == "cf32" else q).cuda()
    x0 = H * K                              # the stream's first H blocks are the first call's halo
    out = torch.zeros(nblocks * N, dtype=torch.complex64, device="cuda")
    rx.channelize(data[m * x0:], nblocks, FIRST, out, d_halo=data[:m * x0])
    parts = []
    for a, b in stage_pieces(nblocks):
        o = torch.full(((b - a) * N,), 7.0, dtype=torch.complex64, device="cuda")
        rx.channelize(data[m * (x0 + a * K):m * (x0 + b * K)], b - a, FIRST + a * K, o, d_halo=data[m * (x0 + (a - H) * K):m * (x0 + a * K)])
        parts.append(o)
    torch.cuda.synchronize()
    one, cut = out.cpu().numpy(), torch.cat(parts).cpu().numpy()
    rx.close()
    assert np.isfinite(one.view(np.float32)).all() and float(np.abs(one).max()) > 1e-3
    return sha(q.tobytes()), one.tobytes(), cut.tobytes()


# ---------------------------------------------------------------------------------------------- a streaming receiver
STREAM_CASES = {
    "K16_p14_cf32": dict(N=8, M=64, cp=8, mod=40, fec1=6, plen=200, nf=3, front_end=0, fmt="cf32"),
    "K16_p14_sc16": dict(N=8, M=64, cp=8, mod=40, fec1=6, plen=200, nf=3, front_end=0, fmt="sc16"),
    "K128_p28_cf32": dict(N=64, M=64, cp=8, mod=40, fec1=6, plen=96, nf=2, front_end=1, fmt="cf32"),
    "K1024_p14_cf32": dict(N=512, M=64, cp=8, mod=40, fec1=6, plen=64, nf=1, front_end=0, fmt="cf32"),
}


def frame_words(f):
    """every field of a delivered frame, floats as their bits"""
    return (f.channel, f.header, f.header_valid, f.payload, f.payload_valid, struct.pack("<3f", f.evm, f.rssi, f.cfo),
            f.mod_scheme, f.mod_bps, f.check, f.fec0, f.fec1, f.end_sample, f.framesyms.view(np.uint32).tobytes())


def decoded(f):
    """what a frame says and where it ended"""
    return (f.channel, f.header, f.header_valid, f.payload, f.payload_valid, f.mod_scheme, f.mod_bps, f.check, f.fec0, f.fec1, f.end_sample)


CUTS = ("pieces", "restart_growth")


def frames_digest(frames):
    h = hashlib.sha256()
    for f in frames:
        h.update(repr(frame_words(f)).encode())
    return h.hexdigest()


def run_stream(product, p):
    """-> dict: the input's digest and the frames of the stream pushed once, in three uneven pieces, and again after a restart in
    two pieces that make the tile buffers grow"""
    torch = _torch()
    N, K = p["N"], 2 * p["N"]
    tx = product.multichanneltx(N, p["M"], p["cp"], 4)
    iq, sent = tx.generate(p["nf"], p["plen"], mod=p["mod"], fec1=p["fec1"], seed=4242 + N)
    tx.close()
    tile = product.TILE * K
    n = int(iq.numel()) // tile * tile
    x = iq[:n].cpu().numpy()
    peak = float(max(np.abs(x.real).max(), np.abs(x.imag).max()))
    q = np.round(x.view(np.float32) * np.float32(0.45 / peak * 32768.0)).astype(np.int16)
    sc16 = p["fmt"] == "sc16"
    m = 2 if sc16 else 1
    data = torch.from_numpy(q if sc16 else dequantise(q)).cuda()
    ntiles = n // tile

    def receiver():
        return product.multichannelrx(N, p["M"], p["cp"], 4, input_format=p["fmt"], front_end=p["front_end"], max_payload_len=max(p["plen"], 64))

    def push(rx, cuts):
        for a, b in cuts:
            rx.Execute(data[m * a * tile:m * b * tile])
        rx.Flush()
        return sorted(rx.frames, key=lambda f: (f.end_sample, f.channel))

    rx = receiver()
    hist_tiles, H = rx.hist_tiles, rx.history_blocks()
    # every push of the long kind holds the history tiles itself and an interior workgroup (slabs are sized per launch: >= 32 blocks,
    # so three workgroups' worth of them is enough)
    t1 = ntiles // 3 + 1
    assert t1 >= hist_tiles and ntiles - t1 - 1 >= hist_tiles and product.TILE < H + 8
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    for nt in (ntiles, t1, ntiles - t1 - 1):
        nb = nt * product.TILE
        assert interior_workgroups(K, p["front_end"], nb, auto_slab(K, nb, ncu)), "no interior workgroup in a push of %d blocks" % nb
    res = {"input": sha(q.tobytes()), "ntiles": ntiles}
    res["once"] = push(rx, [(0, ntiles)])
    rx.close()
    rx = receiver()
    res["pieces"] = push(rx, [(0, t1), (t1, t1 + 1), (t1 + 1, ntiles)])       # carried tiles into the one-tile push, the copy behind it
    rx.close()
    rx = receiver()
    rx.Execute(data[:m * 2 * tile])                                             # a push the restart throws away
    rx.Flush()
    rx.restart()
    del rx.frames[:]
    t2 = max(hist_tiles, ntiles // 4)
    res["restart_growth"] = push(rx, [(0, t2), (t2, ntiles)])                  # no history after the restart; then a larger push: new buffers
    rx.close()
    res["sent"] = sent
    return res


# ---------------------------------------------------------------------------------------------- the tests
def golden(name):
    path = os.path.join(GOLDEN, name)
    assert os.path.exists(path), "fixture missing: tests/golden/make_channelizer_packed.py records it from the parent commit's library"
    z = np.load(path)
    return {k: str(z[k]) for k in z.files}


@pytest.mark.parametrize("N,fe,fmt", STAGE_CASES, ids=STAGE_IDS)
def test_stage_bytes(product, N, fe, fmt):
    """one call == the parent commit's bytes; three calls with halos == one call"""
    g = golden("channelizer_packed_stage.npz")
    key = STAGE_IDS[STAGE_CASES.index((N, fe, fmt))]
    inp, one, cut = run_stage(product, N, fe, fmt)
    assert inp == g[key + "/input"]
    assert sha(one) == g[key + "/tiles"]
    assert cut == one


@pytest.mark.parametrize("name", sorted(STREAM_CASES))
def test_stream_bytes(product, name):
    """a streaming receiver: frames of one push == the parent commit's, every word; cut in three (a one-tile push in the middle), and
    after a restart with growing buffers: the same decoded frames at the same positions as the one push, and every word (evm, rssi, cfo
    and the equalised symbols included) equal to what the parent commit delivers for the same cuts"""
    g = golden("channelizer_packed_stream.npz")
    p = STREAM_CASES[name]
    r = run_stream(product, p)
    assert r["input"] == g[name + "/input"]
    once = r["once"]
    assert len(once) == p["N"] * p["nf"] and all(f.header_valid and f.payload_valid for f in once)
    for f in once:
        assert r["sent"][f.channel][(f.header[0] << 8) | f.header[1]] == (f.header, f.payload)
    assert frames_digest(once) == g[name + "/frames"]
    for other in CUTS:
        assert len(r[other]) == len(once), (other, len(r[other]), len(once))
        for fa, fb in zip(r[other], once):
            assert decoded(fa) == decoded(fb), (other, fa.channel, fa.end_sample, fb.channel, fb.end_sample)
        assert frames_digest(r[other]) == g[name + "/frames_" + other], other
