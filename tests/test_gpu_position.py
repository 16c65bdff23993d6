"""The receiver, the transmitter and the resampler far into a stream: channel-rate positions across 2^31, 2^32, 2^40 and up to
the 48-bit limit of the speculation keys; the 32-bit oscillator across its wrap; the resampler's phase past 2^40 inputs.

One method throughout.  A run at origin 0 is held to the CPU oracle by the standing bars of tests/test_gpu_parity.py
(check_frames, REL) -- so the reference is never merely the code under test -- and the same input at a far position must then
reproduce that run: bit for bit where the arithmetic is position-free (no tolerance), through an exact identity
(tests/position_model.py, checked on the CPU by tests/test_position.py) where it is not."""
import ctypes as C

import numpy as np
import pytest

import position_model as pm
from test_gpu_parity import REL, check_frames, relerr

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


# ============================================================ 1. channel-rate position
SHAPES = {
    # default acquisition + lean M = 64 workers
    "lean64": dict(N=8, M=64, cp=8, mod=40, fec1=6, plen=120, nf=6),
    # the 3 x 16 transform
    "dft48": dict(N=2, M=48, cp=6, mod=40, fec1=6, plen=120, nf=6),
    # wide workers
    "wide256": dict(N=4, M=256, cp=32, mod=27, fec1=7, plen=300, nf=4),
    # K = 7 decoder: the exact path, and the default block path
    "v27_exact": dict(N=2, M=64, cp=8, mod=40, fec1=11, plen=200, nf=4, cfg=dict(conv_scratch=1)),
    "v27_block": dict(N=2, M=64, cp=8, mod=40, fec1=11, plen=200, nf=4, cfg=dict(conv_scratch=0)),
    # scouts that walk: ragged traffic
    "ragged": dict(N=4, M=64, cp=8, mod=40, fec1=6, ragged=True),
    # folded front end, in-line execution
    "folded": dict(N=8, M=64, cp=8, mod=40, fec1=6, plen=120, nf=6, cfg=dict(front_end=1)),
    "serial": dict(N=8, M=64, cp=8, mod=40, fec1=6, plen=120, nf=6, cfg=dict(serial=1)),
    # deferral across pushes: a frame straddles a push boundary and the position boundary
    "defer": dict(N=4, M=64, cp=8, mod=40, fec1=6, plen=120, nf=6, cfg=dict(defer_samples=4096), push=32 * 4 * 9 + 5),
}
BOUNDARIES = [1 << 31, 1 << 32, 1 << 40]        # P = boundary - 4096: a multiple of 4096, so tile, row and segment alignment stay
_STREAMS, _ORIGIN, _FLEN = {}, {}, {}


def _stream(oracle, product, name):
    """(wideband samples, oracle frames) of a shape, made once."""
    if name not in _STREAMS:
        s = SHAPES[name]
        N = s["N"]
        if s.get("ragged"):
            _torch()
            tx = product.multichanneltx(N, s["M"], s["cp"], 4)
            iq, _, _ = tx.generate_ragged(12288, len_lo=64, len_hi=200, seed=99)
            x = iq.cpu().numpy()
            tx.close()
        else:
            x, _ = oracle.synth_traffic(N, s["M"], s["cp"], 4, s["nf"], payload_len=s["plen"], mod=s["mod"], fec1=s["fec1"], seed=31)
        x = np.ascontiguousarray(x[:len(x) // (32 * N) * (32 * N)])
        ora = oracle.MultiChannelRx(N, s["M"], s["cp"], 4, front_end=s.get("cfg", {}).get("front_end", 0))
        ora.execute(x)
        # (ragged traffic: a channel that starts with a silence may first lock onto its neighbour's leakage -- a frame without a
        #  valid header, in the oracle and on the GPU alike)
        assert sum(1 for f in ora.frames if f.payload_valid) >= 3 * N and (s.get("ragged") or all(f.payload_valid for f in ora.frames))
        _STREAMS[name] = (x, ora.frames)
    return _STREAMS[name]


def _pieces(name, x):
    push = SHAPES[name].get("push")
    if push:
        return [x[i:i + push] for i in range(0, len(x), push)]
    a, b = int(len(x) * 0.37) | 1, int(len(x) * 0.71) | 1          # three uneven pieces, like a radio's packets
    return [x[:a], x[a:b], x[b:]]


def _receive(product, name, x, P, extra_cfg=None, monitor=False, twice=False):
    """Frames (and the monitor's reading) of stream x on a fresh handle moved to channel-rate position P (None: never moved)."""
    s = SHAPES[name]
    cfg = dict(s.get("cfg", {}))
    cfg.update(extra_cfg or {})
    rx = product.multichannelrx(s["N"], s["M"], s["cp"], 4, max_payload_len=256 if s.get("ragged") else max(s["plen"], 64), **cfg)
    if P is not None:
        rx.reset_at(P)
    if monitor:
        rx.monitor_enable(64, "hann")
    for rep in range(2 if twice else 1):
        if rep:
            rx.Reset()                  # positions continue from where the stream stood
        for p in _pieces(name, x):
            rx.Execute(p)
        rx.Flush()
    reading = rx.monitor_read() if monitor else None
    frames = list(rx.frames)
    rx.close()
    return frames, reading


def _origin(oracle, product, name, key=(), **kw):
    """The origin-0 run of a shape, held to the oracle by the standing bars; made once per variant."""
    if (name, key) not in _ORIGIN:
        x, ora_frames = _stream(oracle, product, name)
        frames, reading = _receive(product, name, x, None, **kw)
        n = len(ora_frames)
        if kw.get("twice"):
            assert len(frames) == 2 * n
            check_frames(frames[n:], ora_frames)
        check_frames(frames[:n], ora_frames)
        _ORIGIN[(name, key)] = (frames, reading)
    return _ORIGIN[(name, key)]


FIELDS = ("channel", "header", "payload", "header_valid", "payload_valid", "mod_scheme", "mod_bps", "check", "fec0", "fec1")


def _same_frames(far, org, P):
    """Field for field, in delivery order; floats as their bits; end_sample relative to P."""
    assert len(far) == len(org), (len(far), len(org))
    for i, (a, b) in enumerate(zip(far, org)):
        for k in FIELDS:
            assert getattr(a, k) == getattr(b, k), (i, k, getattr(a, k), getattr(b, k))
        for k in ("evm", "rssi", "cfo"):
            assert np.float32(getattr(a, k)).tobytes() == np.float32(getattr(b, k)).tobytes(), (i, k, getattr(a, k), getattr(b, k))
        assert a.framesyms.tobytes() == b.framesyms.tobytes(), (i, "framesyms", relerr(a.framesyms, b.framesyms) if len(a.framesyms) == len(b.framesyms) else None)
        assert a.end_sample - P == b.end_sample, (i, "end_sample", a.end_sample - P, b.end_sample)


def _frame_len(oracle, name, f):
    s = SHAPES[name]
    key = (s["M"], s["cp"], s["mod"], s["fec1"], len(f.payload))
    if key not in _FLEN:
        g = oracle.FlexFrameGen(s["M"], s["cp"], 4, fec1=s["fec1"], mod=s["mod"])
        _FLEN[key] = len(g.frame(bytes(8), bytes(len(f.payload))))
    return _FLEN[key]


def _boundary_inside_the_traffic(oracle, name, frames, boundary):
    ends = [(f.end_sample, f.end_sample - _frame_len(oracle, name, f)) for f in frames if f.payload_valid]
    assert any(e < boundary for e, _ in ends), "no frame ends below the boundary"
    assert any(s < boundary <= e for e, s in ends), "no frame starts below the boundary and ends above it"
    assert any(s >= boundary for _, s in ends), "no frame lies wholly above the boundary"


@pytest.mark.parametrize("boundary", BOUNDARIES, ids=["2^31", "2^32", "2^40"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_frames_do_not_depend_on_where_the_stream_stands(oracle, product, name, boundary):
    """reset_at(P) on a fresh handle, then the stream in pieces: every frame equals the origin run's, bit for bit, with end_sample
    moved by P.  The wideband oscillator runs on total_samples, which reset_at leaves alone, so the channelizer's bits are the
    same; the synchronizers work on positions relative to the buffer, their CFO oscillator on positions relative to nco_t_ref."""
    _torch()
    P = boundary - 4096
    org, _ = _origin(oracle, product, name)
    x, _ = _stream(oracle, product, name)
    far, _ = _receive(product, name, x, P)
    _same_frames(far, org, P)
    _boundary_inside_the_traffic(oracle, name, far, boundary)


@pytest.mark.parametrize("build", ["default", "lean_segments", "one_kernel_scout"])
def test_segment_wave_and_scout_builds_across_2_31(oracle, product, build):
    """The build switches tests/test_gpu_alloc.py parametrises, at P = 2^31 - 4096 on the first shape."""
    _torch()
    cfg = {"default": {}, "lean_segments": {"scout_build": 2}, "one_kernel_scout": {"acquisition": 4}}[build]
    P = (1 << 31) - 4096
    org, _ = _origin(oracle, product, "lean64", key=build, extra_cfg=cfg)
    x, _ = _stream(oracle, product, "lean64")
    far, _ = _receive(product, "lean64", x, P, extra_cfg=cfg)
    _same_frames(far, org, P)
    _boundary_inside_the_traffic(oracle, "lean64", far, 1 << 31)


def test_reset_after_the_boundary_then_a_second_burst(oracle, product):
    """Reset() behind 2^31 and the stream again: positions continue from where the stream stood (the second burst's end_sample
    values lie one stream length further on, in both runs), and the frames again equal the origin run's."""
    _torch()
    P = (1 << 31) - 4096
    org, _ = _origin(oracle, product, "lean64", key="twice", twice=True)
    x, _ = _stream(oracle, product, "lean64")
    far, _ = _receive(product, "lean64", x, P, twice=True)
    _same_frames(far, org, P)
    n = len(org) // 2
    assert min(f.end_sample for f in far[n:]) > max(f.end_sample for f in far[:n]) > 1 << 31


def test_channel_monitor_across_2_31(oracle, product):
    _torch()
    P = (1 << 31) - 4096
    org, r0 = _origin(oracle, product, "lean64", key="monitor", monitor=True)
    x, _ = _stream(oracle, product, "lean64")
    far, r1 = _receive(product, "lean64", x, P, monitor=True)
    _same_frames(far, org, P)
    assert (r1.nseg, r1.nsamp) == (r0.nseg, r0.nsamp) and r0.nseg > 0
    for k in ("level", "peak", "psd"):
        assert getattr(r1, k).tobytes() == getattr(r0, k).tobytes(), k


def test_just_below_the_position_limit_and_refusal_above_it(oracle, product):
    """spec_key / sp_start (csrc/ofdmsync.hip) pack a position into 48 bits: every position a launch handles, the one behind its
    last sample included, must stay below MCRX_POSITION_MAX = 2^48.  A stream that ends a few thousand samples below it is
    received like the origin run; mcrx_hip_reset_at and mcrx_hip_sync refuse what would reach it with MCRX_EINVAL."""
    torch = _torch()
    name = "lean64"
    s = SHAPES[name]
    LIMIT = product.POSITION_MAX
    assert LIMIT == 1 << 48
    org, _ = _origin(oracle, product, name)
    x, _ = _stream(oracle, product, name)
    nchan = len(x) // (2 * s["N"])
    P = LIMIT - 4096 * (nchan // 4096 + 2)               # the last multiple of 4096 that leaves the stream (and a tile) room below the limit
    far, _ = _receive(product, name, x, P)
    _same_frames(far, org, P)
    assert LIMIT - 2 * 4096 < max(f.end_sample for f in far) + 4096 and max(f.end_sample for f in far) < LIMIT
    rx = product.multichannelrx(s["N"], s["M"], s["cp"], 4)
    L = product.lib()
    for bad in (LIMIT, LIMIT + 4096, 1 << 52, (1 << 64) - 4096):
        with pytest.raises(ValueError):
            rx.reset_at(bad)
        assert L.mcrx_hip_reset_at(rx._h, bad) == product.MCRX_EINVAL
    rx.reset_at(LIMIT - 4096)
    ntile = rx.hist_tiles + 4
    d = torch.zeros(ntile * s["N"] * 16, dtype=torch.complex64, device="cuda")
    first = LIMIT - 4096 - rx.hist_tiles * 16
    assert L.mcrx_hip_sync(rx._h, C.c_void_p(d.data_ptr()), first, ntile * 16, None) == product.MCRX_OK       # ends at LIMIT - 4096 + 64
    assert L.mcrx_hip_sync(rx._h, C.c_void_p(d.data_ptr()), LIMIT - ntile * 16, ntile * 16, None) == product.MCRX_EINVAL     # would end at LIMIT
    assert L.mcrx_hip_sync(rx._h, C.c_void_p(d.data_ptr()), LIMIT + 4096, ntile * 16, None) == product.MCRX_EINVAL
    # the push path stops at the limit too, instead of wrapping the keys
    rx.reset_at(LIMIT - 16)
    with pytest.raises(product.McrxError):
        rx.Execute(x[:32 * s["N"] * 4]); rx.Flush()
    rx.reset_at(0)
    rx.close()


# ============================================================ 2. wideband position: the oscillator across 2^32
PARITY = {}         # measured deviations (printed; recorded in profiles/position_parity.json)


class _Bank(object):
    """Stage-level channelizer calls over one seeded input: x = [history_blocks() blocks passed as the halo | nblocks]."""

    def __init__(self, oracle, product, N, front_end):
        torch = _torch()
        self.torch, self.product = torch, product
        self.N, self.K = N, 2 * N
        self.nblocks = 96 if (N & (N - 1)) == 0 else 64
        self.rx = product.multichannelrx(N, 64, 8, 4, front_end=front_end)
        self.H = self.rx.history_blocks()
        assert self.H == (27 if front_end else 13)
        rng = np.random.RandomState(1000 * front_end + N)
        n = (self.H + self.nblocks) * self.K
        self.x = (rng.randn(n) + 1j * rng.randn(n)).astype(np.complex64)
        self.d_x = torch.from_numpy(self.x).cuda()
        ora = oracle.MultiChannelRx(N, 64, 8, 4)
        # the oracle runs from origin 0 over halo and body alike: its oscillator stands at H*K where the body begins
        self.ref = (ora.channelize_oversampled(self.x) if front_end else ora.channelize(self.x))[self.H:]
        self.dth = self.rx.nco_step()

    def run(self, first_sample, b0=0, nb=None):
        """Blocks [b0, b0 + nb) of the body, with the H blocks in front of them as the halo -> [block][N]"""
        nb = self.nblocks - b0 if nb is None else nb
        K, H = self.K, self.H
        d_out = self.torch.zeros(nb * self.N, dtype=self.torch.complex64, device="cuda")
        self.rx.channelize(self.d_x[(H + b0) * K:(H + b0 + nb) * K], nb, first_sample, d_out, d_halo=self.d_x[b0 * K:(H + b0) * K])
        self.torch.cuda.synchronize()
        return self.product.tiles_to_channels(d_out, self.N).T

    def expected(self, first_sample):
        """The oracle's body blocks turned to the origin `first_sample` of the body's first sample (exact identity, float64)."""
        return pm.origin_rotation(first_sample - self.H * self.K, self.dth) * self.ref.astype(np.complex128)


BANKS = [(1, 0), (8, 0), (64, 0), (3, 0), (40, 0), (8, 1), (64, 1)]      # power-of-two fast path, generic kernel, folded front end


@pytest.mark.parametrize("N,front_end", BANKS)
def test_oscillator_across_2_32(oracle, product, N, front_end):
    """The phase word is (t * dtheta) mod 2^32, so the bank's output at origin s0 is the output at origin 0 times one constant.
    s0 = 2^32 - 32 K: the sample count wraps a third (N = 3, 40: half) of the way into the call.  Value: within REL of the oracle
    turned by that constant.  Bits: the wrap inside a call equals a cut at the wrap, whichever of 2^32 and 0 the second call is
    given; first_sample + k 2^32 equals first_sample.  (For N = 3 and 40, 2^32 is no multiple of 16 K, so s0 is none either;
    first_sample only enters the phase, the call pattern is the same at every origin.)
    front_end = 2 and the push path (nco_mix_kernel) have no stage-level entry -- mcrx_hip_channelize refuses such a handle -- and
    reaching 2^32 wideband samples through Execute means pushing 32 GB: not covered here.  That kernel takes (uint32_t)first_abs and
    forms (first_lo + i) * dtheta in 32 bits, the same closed form."""
    b = _Bank(oracle, product, N, front_end)
    K = b.K
    s0 = (1 << 32) - 32 * K
    g0, gs = b.run(0), b.run(s0)
    e0 = relerr(g0, b.expected(0))
    assert e0 <= REL, e0                                    # the origin run is the oracle's
    es = relerr(gs, b.expected(s0))
    assert es <= REL, es
    c = pm.origin_rotation(s0, b.dth)
    self_dev = relerr(gs, c * g0.astype(np.complex128))
    PARITY["N=%d front_end=%d" % (N, front_end)] = {"gpu_s0_vs_c_times_oracle": es, "gpu_s0_vs_c_times_gpu_0": self_dev, "gpu_0_vs_oracle": e0}
    print("position_parity N=%d front_end=%d: gpu(s0) vs c*oracle %.3g, gpu(s0) vs c*gpu(0) %.3g, gpu(0) vs oracle %.3g" % (N, front_end, es, self_dev, e0))
    assert self_dev <= REL, self_dev
    # the wrap inside a call equals a cut at the wrap
    head = b.run(s0, 0, 32)
    for second in (1 << 32, 0):
        cut = np.concatenate([head, b.run(second, 32)])
        assert np.array_equal(cut, gs), second
    # only the low 32 bits of first_sample count
    s = 5 * 16 * K
    gsm = b.run(s)
    assert relerr(gsm, b.expected(s)) <= REL
    for k in (1, 1 << 20):
        assert np.array_equal(b.run(s + (k << 32)), gsm), k
    b.rx.close()


# ============================================================ 3. transmit side across 2^32
def test_transmitter_across_2_32(oracle, product):
    """synthesize() with first_block * K wrapping inside the call: the waveform is the origin-0 waveform times the conjugate of the
    receiver's constant (the transmitter mixes up), within REL; fed to the receiver's bank at the same first_sample, the synchronizers
    decode the same headers and payloads as from the origin-0 pair.
    The tiles are channel rate and have no oscillator, but a TxTraffic's frames are anchored at block 0 and end after a few thousand
    blocks: at block 2^32 / K the traffic is silent, and tiles() must say so -- zeros, like the tiles behind the traffic's end at the
    origin.  The tiles synthesized here are therefore the traffic's own (blocks from 0 on), handed to synthesize() at either origin."""
    torch = _torch()
    N, M, cp, nf, plen = 8, 64, 8, 2, 120
    K, lead = 2 * N, 48
    tx = product.multichanneltx(N, M, cp, 4)
    tr = tx.traffic(0, N, nf, plen, seed=5)
    nb = (tr.blocks + 15) // 16 * 16
    assert nb > 64
    fb = (1 << 32) // K - 32
    tiles = tr.tiles(-lead, lead + nb, torch.empty((lead + nb) * N, dtype=torch.complex64, device="cuda"))
    far_tiles = tr.tiles(fb - lead, lead + nb, torch.full(((lead + nb) * N,), 1.0, dtype=torch.complex64, device="cuda"))
    past_tiles = tr.tiles(nb + 4096 - lead, lead + nb, torch.full(((lead + nb) * N,), 1.0, dtype=torch.complex64, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(far_tiles, past_tiles) and not bool(far_tiles.abs().max() > 0) and bool(tiles.abs().max() > 0)
    w0 = tx.synthesize(tiles, 1, 0, nb, lead).clone()
    ws = tx.synthesize(tiles, 1, fb, nb, lead).clone()
    torch.cuda.synchronize()
    rx = product.multichannelrx(N, M, cp, 4)
    c = pm.origin_rotation(fb * K, rx.nco_step())
    a0, a1 = w0.cpu().numpy(), ws.cpu().numpy()
    assert np.max(np.abs(a0)) > 0
    e = relerr(a1, np.conj(c) * a0.astype(np.complex128))
    PARITY["tx N=8"] = {"synth_fb_vs_conj_c_times_synth_0": e}
    print("position_parity tx N=8: synthesize(first_block) vs conj(c)*synthesize(0) %.3g" % e)
    assert e <= REL, e
    rx.close()
    got = []
    for w, first in ((w0, 0), (ws, fb * K)):
        rx = product.multichannelrx(N, M, cp, 4)
        ht = rx.hist_tiles
        d_chan = torch.zeros((ht * 16 + nb) * N, dtype=torch.complex64, device="cuda")
        rx.channelize(w, nb, first, d_chan[ht * 16 * N:])
        rx.sync(d_chan, -ht * 16, ht * 16 + nb)
        rx.Flush()
        got.append(sorted((f.channel, f.header, f.payload, f.header_valid, f.payload_valid) for f in rx.frames))
        rx.close()
    assert got[0] == got[1] and len(got[0]) == nf * N
    for ch, h, p, hv, pv in got[1]:
        assert hv and pv and (h, p) in tr.sent[ch]
    tr.close(); tx.close()


# ============================================================ 4. the resampler past 2^40
RATES = [0.5, 0.37, 0.8, 0.2, 0.11, 2.0, 1.5, 4.0, 6.3, 0.25, 0.45, 0.06]      # test_msresamp_front_end_matches_oracle's


def _randn(torch, n, gen):
    return torch.view_as_complex(torch.randn(n, 2, generator=gen, device="cuda", dtype=torch.float32))


@pytest.mark.parametrize("rate", RATES)
def test_resampler_beyond_2_40(product, rate):
    """From the first aligned position at or above 2^40, 2^41, 2^48 and 2^56 the output equals a fresh handle's on the same samples,
    bit for bit (test_msresamp_front_end_matches_oracle ties that run to the oracle).  Positions that are no multiple of
    2^num_stages are refused."""
    torch = _torch()
    plan = pm.ResampPlan(rate)
    n = 64 * 1024
    rng = np.random.RandomState(int(rate * 1000))
    d_x = torch.from_numpy((rng.randn(n) + 1j * rng.randn(n)).astype(np.complex64)).cuda()

    def feed(q):
        parts, pos = [], 0
        for step in (1000, 7, 8192, 333, n):
            parts.append(q.execute(d_x[pos:pos + step]))
            pos += step
            if pos >= n:
                break
        return torch.cat(parts)

    q0 = product.msresamp(rate)
    y0 = feed(q0)
    assert y0.numel() > 0.9 * rate * n
    q = product.msresamp(rate)
    for target in (1 << 40, 1 << 41, 1 << 48, 1 << 56):
        pos = plan.aligned_raw_at_or_above(target)
        q.reset(at=pos)
        y = feed(q)
        assert y.numel() == y0.numel() and torch.equal(y, y0), (target, pos, y.numel(), y0.numel())
    if plan.num_stages:
        with pytest.raises(ValueError):
            q.reset(at=(1 << 40) + 1)
    q.reset()
    assert torch.equal(feed(q), y0)
    q.close(); q0.close()


@pytest.mark.parametrize("rate", [0.5, 0.8, 2.0, 1.5, 0.37, 6.3])
def test_resampler_crossing_2_40(product, rate):
    """Seek to the largest aligned position at least 4096 arbitrary-stage inputs below 2^40 and push random samples until 64 K past
    the point where that stage's input index reaches 2^40 -- one push ends just before it, one straddles it, one starts after it --
    against an origin-0 handle fed the same pushes, bit for bit, push by push.
    Before the fix (phase products wrapping at 2^64) every push from the straddling one on returned no samples, with MCRX_OK."""
    torch = _torch()
    plan = pm.ResampPlan(rate)
    seek, sizes, straddle = pm.crossing_plan(plan)
    assert sum(sizes) <= 1 << 27 and straddle == len(sizes) - 2
    gen = torch.Generator(device="cuda")
    gen.manual_seed(int(rate * 1000))
    q0, q1 = product.msresamp(rate), product.msresamp(rate)
    q1.reset(at=seek)
    total = 0
    for i, n in enumerate(sizes):
        x = _randn(torch, n, gen)
        y0 = q0.execute(x)
        y1 = q1.execute(x)
        same = y1.numel() == y0.numel() and torch.equal(y1, y0)
        assert same, (i, len(sizes), n, int(y1.numel()), int(y0.numel()))
        total += int(y0.numel())
        if n >= 1024:
            assert y0.numel() > 0.9 * plan.rate * n - 64 * plan.rate, (i, n, int(y0.numel()))
        del x, y0, y1
    assert abs(total - plan.rate * sum(sizes)) <= 64 * max(plan.rate, 1.0) + 1e-4 * plan.rate * sum(sizes)
    q0.close(); q1.close()


@pytest.mark.parametrize("rate,push", [(0.37, 4 << 20), (6.3, 1 << 20), (0.8, 1 << 16)])
def test_resampler_rebase_point_does_not_show(product, rate, push):
    """The host takes whole periods of the phase off its counters between calls (csrc/msresamp.hip, rs_rebase), when the stage
    buffers allow it -- so WHEN depends on how the stream is cut.  One handle is fed pushes of `push` samples, another the same
    samples with every push cut in four uneven pieces, through more than one period: the outputs are the same bits, although in
    between one handle works on rebased counters and the other does not."""
    torch = _torch()
    plan = pm.ResampPlan(rate)
    total = plan.per_in * plan.raw_per_arb() + 2 * push
    assert total <= 1 << 26
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    q0, q1 = product.msresamp(rate), product.msresamp(rate)
    pos = 0
    while pos < total:
        x = _randn(torch, push, gen)
        y0 = q0.execute(x)
        a, b, c = push // 4 + 3, push // 2 - 1, 3 * (push // 4)
        y1 = torch.cat([q1.execute(x[:a]), q1.execute(x[a:b]), q1.execute(x[b:c]), q1.execute(x[c:])])
        assert y1.numel() == y0.numel() and torch.equal(y1, y0), (pos, int(y1.numel()), int(y0.numel()))
        pos += push
        del x, y0, y1
    q0.close(); q1.close()


def test_zz_print_position_parity():
    """(last of this file: the deviations measured above, one JSON line, for profiles/position_parity.json)"""
    import json
    print("POSITION_PARITY " + json.dumps(PARITY, sort_keys=True))
