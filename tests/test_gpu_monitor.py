"""Channel monitor on the GPU (csrc/monitor.hip, mcrx_hip_monitor_*) against the float64 model of tests/monitor_model.py.

Two comparisons per shape, with bars taken from the project's standing ones (not from what the kernel gives):
  (a) the kernel alone -- the model fed with the GPU's own channel tiles (mcrx_hip_channelize of the same IQ; the pushed stream for a
      single-channel handle): per channel psd within 1e-5 of that channel's largest bin, level and peak within 1e-5 relative;
  (b) end to end -- the model fed with the oracle's channelizer output: psd within 3e-5 of the largest bin of any channel, level / peak
      within 3e-5 of the largest channel's (the channelizer's 1e-5 amplitude bar doubled for the square, plus the kernel's 1e-5).
Every figure is printed before it is asserted; with MCRX_MONITOR_PARITY=<path> the largest deviations per shape are written there as
JSON (profiles/monitor_parity.json is such a record)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import monitor_model as mm          # noqa: E402

M, CP, TP = 64, 16, 4
RECORD = {}


def _record(key, **figs):
    RECORD[key] = {k: float(v) for k, v in figs.items()}
    print("monitor parity", key, " ".join("%s=%.3g" % kv for kv in sorted(figs.items())))
    path = os.environ.get("MCRX_MONITOR_PARITY")
    if path:
        with open(path, "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)


def tx_stream(oracle, N, active, nframes, plen, seed=7, extra_blocks=64):
    """The oracle transmitter's stream (gain 1) with frames back to back on the `active` channels only (per-channel UpdateData)."""
    tx = oracle.MultiChannelTx(N, M, CP, TP)
    rngs = {c: np.random.RandomState((seed + c) & 0x7FFFFFFF) for c in active}
    pid = {c: 0 for c in active}
    chunks, idle, L = [], 0, M + CP
    while idle < extra_blocks:
        for c in active:
            if pid[c] < nframes and tx.ready(c):
                hdr = bytes([(pid[c] >> 8) & 0xff, pid[c] & 0xff, c & 0xff]) + bytes(rngs[c].randint(0, 256, 5).astype(np.uint8))
                tx.update(c, hdr, bytes(rngs[c].randint(0, 256, plen).astype(np.uint8)))
                pid[c] += 1
        chunks.append(tx.generate(L))
        if all(pid[c] >= nframes and tx.ready(c) for c in active):
            idle += L
    return np.concatenate(chunks)


def whole_tiles(x, N):
    return np.ascontiguousarray(x[:len(x) // (32 * N) * (32 * N)], np.complex64)


def awgn(x, snr_db, seed=3):
    rng = np.random.RandomState(seed)
    nstd = np.sqrt(np.mean(np.abs(x) ** 2)) * 10.0 ** (-snr_db / 20.0) / np.sqrt(2.0)
    return (x + nstd * (rng.randn(len(x)) + 1j * rng.randn(len(x)))).astype(np.complex64)


def make_input(oracle, N, traffic):
    if N == 1:                                   # a single synchronizer's own stream: frames of one generator, idle gaps, noise
        gen = oracle.FlexFrameGen(M, CP, TP)
        rng = np.random.RandomState(11)
        parts = []
        for i in range(4):
            parts += [gen.frame(bytes([0, i, 0, 1, 2, 3, 4, 5]), bytes(rng.randint(0, 256, 200).astype(np.uint8))), np.zeros(40 + 16 * i, np.complex64)]
        x = np.concatenate(parts)
        return awgn(np.ascontiguousarray(x[:len(x) // 16 * 16], np.complex64), 30.0)
    nframes = 2 if N <= 64 else 1
    if traffic == "frames":
        iq, _ = oracle.synth_traffic(N, M, CP, TP, nframes, payload_len=200)
    else:                                        # near-far: per-channel gains spread over 30 dB
        gains = 10.0 ** (-30.0 * np.arange(N) / (N - 1.0) / 20.0)
        rng = np.random.RandomState(5)
        rng.shuffle(gains)
        parts = [tx_stream(oracle, N, [c], nframes, 200) * gains[c] for c in range(N)]
        n = min(len(p) for p in parts)
        iq = sum(p[:n] for p in parts) / N
    return awgn(whole_tiles(iq, N), 30.0 if traffic == "frames" else 50.0)


def gpu_tiles(product, x, N, fe, first_sample=0):
    """channel-rate samples [n, N] as the GPU's own channelizer produces them from a fresh history"""
    import torch
    h = product.multichannelrx(N, M, CP, TP, front_end=fe)
    d = torch.from_numpy(x).cuda()
    nb = len(x) // (2 * N)
    out = torch.empty(nb * N, dtype=torch.complex64, device="cuda")
    h.channelize(d, nb, first_sample, out)
    torch.cuda.synchronize()
    chan = product.tiles_to_channels(out, N).T
    h.close()
    return chan


def make_rx(product, N, **cfg):
    if N == 1:
        return product.ofdmflexframesync(M, CP, TP, **cfg)
    return product.multichannelrx(N, M, CP, TP, max_payload_len=300, **cfg)


def push(rx, x, cuts=None):
    """x in pushes of cuts[i % len] blocks (tiles of 16), device resident"""
    import torch
    d = torch.from_numpy(x).cuda()
    K = rx.K
    if cuts is None:
        rx.Execute(d)
        return
    b, i, nb = 0, 0, len(x) // K
    while b < nb:
        n = min(cuts[i % len(cuts)], nb - b)
        rx.Execute(d[b * K:(b + n) * K])
        b += n; i += 1


def dev_kernel(r, model):
    level, peak, psd = model[:3]
    return dict(psd=np.max(np.abs(r.psd - psd).max(axis=1) / psd.max(axis=1)), level=np.max(np.abs(r.level - level) / level),
                peak=np.max(np.abs(r.peak - peak) / peak))


def dev_end_to_end(r, model):
    level, peak, psd = model[:3]
    return dict(psd=np.max(np.abs(r.psd - psd)) / psd.max(), level=np.max(np.abs(r.level - level)) / level.max(),
                peak=np.max(np.abs(r.peak - peak)) / peak.max())


SHAPES = [(1, 64, 1, 0, "frames"), (8, 16, 1, 0, "frames"), (8, 32, 1, 0, "frames"), (8, 64, 0, 0, "frames"), (8, 64, 1, 0, "frames"),
          (8, 64, 2, 0, "frames"), (8, 128, 1, 0, "frames"), (8, 256, 1, 0, "frames"), (8, 64, 1, 1, "frames"), (64, 64, 1, 0, "frames"),
          (64, 64, 1, 1, "frames"), (512, 64, 1, 0, "frames"), (8, 64, 1, 0, "nearfar"), (8, 256, 2, 0, "nearfar"), (8, 64, 1, 1, "nearfar")]


@pytest.mark.parametrize("N,nfft,win,fe,traffic", SHAPES)
def test_monitor_against_model(oracle, product, N, nfft, win, fe, traffic):
    x = make_input(oracle, N, traffic)
    rx = make_rx(product, N, **({"front_end": fe} if N > 1 else {}))
    rx.monitor_enable(nfft, win)
    assert rx.monitor_nfft() == nfft
    push(rx, x)
    r = rx.monitor_read()
    rx.close()
    if N == 1:
        own = x.reshape(-1, 1)
        ora = own
    else:
        own = gpu_tiles(product, x, N, fe)
        o = oracle.MultiChannelRx(N, M, CP, TP, front_end=fe)
        ora = (o.channelize_oversampled if fe else o.channelize)(x)
    ma, mb = mm.monitor(own, nfft, win), mm.monitor(ora, nfft, win)
    assert (r.nseg, r.nsamp) == (ma[3], ma[4]) == (mb[3], mb[4]) and r.nseg > 0
    assert r.psd.shape == (N, nfft) and r.level.shape == (N,) and r.peak.shape == (N,)
    a, b = dev_kernel(r, ma), dev_end_to_end(r, mb)
    key = "N%d_nfft%d_win%d_fe%d_%s" % (N, nfft, win, fe, traffic)
    _record(key, kernel_psd=a["psd"], kernel_level=a["level"], kernel_peak=a["peak"], e2e_psd=b["psd"], e2e_level=b["level"], e2e_peak=b["peak"])
    if traffic == "nearfar":
        db = 10 * np.log10(mb[0])
        assert db.max() - db.min() > 25.0, db           # the input really is near-far
    assert a["psd"] < 1e-5 and a["level"] < 1e-5 and a["peak"] < 1e-5, a
    assert b["psd"] < 3e-5 and b["level"] < 3e-5 and b["peak"] < 3e-5, b
    if win == 0 and r.nsamp == r.nseg * nfft:              # Parseval on the device's own sums (fp32 transform: the kernel's bar)
        assert np.max(np.abs(r.psd.mean(axis=1) - r.level) / r.level) < 1e-5


@pytest.mark.parametrize("N,active", [(8, [1, 2, 5]), (64, list(range(0, 64, 5)))])
def test_occupancy_mask(oracle, product, N, active):
    skip = 64
    x = whole_tiles(tx_stream(oracle, N, active, 3 if N == 8 else 2, 200) / N, N)
    chan = oracle.MultiChannelRx(N, M, CP, TP).channelize(x)
    level = mm.monitor(chan[skip:], 64, 1)[0]
    db = 10 * np.log10(np.maximum(level, 1e-300))
    act = np.zeros(N, bool); act[active] = True
    gap = db[act].min() - db[~act].max()
    print("occupancy N=%d: weakest active %.1f dB, strongest idle %.1f dB, gap %.1f dB" % (N, db[act].min(), db[~act].max(), gap))
    if gap < 30.0:
        raise RuntimeError("the input does not separate active from idle channels by 30 dB (%.1f dB): the test would pass vacuously" % gap)
    t = 0.5 * (db[act].min() + db[~act].max())
    rx = make_rx(product, N)
    K = 2 * N
    push(rx, x[:skip * K])
    rx.monitor_enable(64, "hann")                          # mid-stream: counted from here
    push(rx, x[skip * K:])
    r = rx.monitor_read()
    rx.close()
    assert r.nsamp == chan.shape[0] - skip
    assert r.occupied(t).tolist() == act.tolist() == (db > t).tolist()


def _read_cut(product, x, N, nfft, cuts):
    rx = make_rx(product, N)
    rx.monitor_enable(nfft, "hann")
    push(rx, x, cuts)
    r = rx.monitor_read()
    rx.close()
    return r


@pytest.mark.parametrize("nfft", [32, 64, 256])
def test_cuts_do_not_change_the_result(oracle, product, nfft):
    N = 8
    x = make_input(oracle, N, "frames")
    whole = _read_cut(product, x, N, nfft, None)
    for cuts in ([16], [16, 48, 80, 208]):
        r = _read_cut(product, x, N, nfft, cuts)
        assert (r.nseg, r.nsamp) == (whole.nseg, whole.nsamp)
        assert np.array_equal(r.peak, whole.peak)
        dl, dp = np.max(np.abs(r.level - whole.level) / whole.level), np.max(np.abs(r.psd - whole.psd) / whole.psd)
        print("cuts", nfft, cuts, "level %.3g psd %.3g" % (dl, dp))
        assert dl < 1e-12 and dp < 1e-12
        again = _read_cut(product, x, N, nfft, cuts)
        assert np.array_equal(again.psd, r.psd) and np.array_equal(again.level, r.level) and np.array_equal(again.peak, r.peak)


def test_intervals_tile_the_stream(oracle, product):
    import torch
    N, nfft = 8, 128
    x = make_input(oracle, N, "frames")
    one = _read_cut(product, x, N, nfft, [16, 48, 80, 208])
    rx = make_rx(product, N)
    rx.monitor_enable(nfft, "hann")
    d = torch.from_numpy(x).cuda()
    K, cuts, b, i, rows = 2 * N, [16, 48, 80, 208], 0, 0, []
    while b < len(x) // K:
        n = min(cuts[i % 4], len(x) // K - b)
        rx.Execute(d[b * K:(b + n) * K])
        rows.append(rx.monitor_read(reset=True))
        b += n; i += 1
    rx.close()
    assert sum(r.nseg for r in rows) == one.nseg and sum(r.nsamp for r in rows) == one.nsamp
    assert any(r.nseg == 0 for r in rows) and any(r.nseg > 1 for r in rows)
    psd = sum(r.psd * r.nseg for r in rows) / one.nseg
    level = sum(r.level * r.nsamp for r in rows) / one.nsamp
    assert np.max(np.abs(psd - one.psd) / one.psd) < 1e-12 and np.max(np.abs(level - one.level) / one.level) < 1e-12
    assert np.array_equal(np.max([r.peak for r in rows], axis=0), one.peak)


def test_reset_drops_carry_and_sums(oracle, product):
    N, nfft = 8, 64
    x = make_input(oracle, N, "frames")
    K = 2 * N
    na = 48 * K                                            # 48 samples per channel: three quarters of a segment are carried
    rx = make_rx(product, N)
    rx.monitor_enable(nfft, "rect")
    push(rx, x[:na])
    assert rx.monitor_read().nseg == 0 and rx.monitor_read().nsamp == 48
    rx.Reset()
    r0 = rx.monitor_read()
    assert (r0.nseg, r0.nsamp) == (0, 0) and not r0.level.any() and not r0.psd.any() and not r0.peak.any()
    push(rx, x[na:])
    r = rx.monitor_read()
    rx.close()
    own = gpu_tiles(product, x[na:], N, 0, first_sample=na)     # the oscillator runs on, the filter starts from zeros again
    m = mm.monitor(own, nfft, 0)
    assert (r.nseg, r.nsamp) == (m[3], m[4])
    a = dev_kernel(r, m)
    print("after Reset", a)
    assert a["psd"] < 1e-5 and a["level"] < 1e-5 and a["peak"] < 1e-5


def test_shards_concatenate_to_the_whole(oracle, product):
    """the multi-GPU code path on one GPU: two handles with channel_first / channel_count fed through mcrx_hip_sync, and the C pipeline
    at world = 1, against the unsharded handle"""
    import torch
    from liquid_usrp_amd import sharding
    N, nfft, world = 16, 64, 2
    K, cg = 2 * N, N // world
    x = make_input(oracle, N, "frames")
    whole = _read_cut(product, x, N, nfft, None)
    d = torch.from_numpy(x).cuda()
    T = len(x) // K
    full = product.multichannelrx(N, M, CP, TP)
    out = torch.empty(T * N, dtype=torch.complex64, device="cuda")
    full.channelize(d, T, 0, out, groups=world)
    torch.cuda.synchronize()
    full.close()
    chunk = (T // product.TILE) * cg * product.TILE
    parts = []
    for r in range(world):
        c0, cnt = sharding.shard_of(r, world, N)
        h = product.multichannelrx(N, M, CP, TP, max_payload_len=300, channel_first=c0, channel_count=cnt)
        h.monitor_enable(nfft, "hann")
        h.sync(out[r * chunk:(r + 1) * chunk], 0, T)
        parts.append(h.monitor_read())
        assert parts[-1].channel_first == c0 and parts[-1].psd.shape == (cnt, nfft)
        h.close()
    assert all((p.nseg, p.nsamp) == (whole.nseg, whole.nsamp) for p in parts)
    psd, level = np.concatenate([p.psd for p in parts]), np.concatenate([p.level for p in parts])
    assert np.max(np.abs(psd - whole.psd) / whole.psd) < 1e-12 and np.max(np.abs(level - whole.level) / whole.level) < 1e-12
    assert np.array_equal(np.concatenate([p.peak for p in parts]), whole.peak)
    # the pipeline's rounds (history tiles in front of every round: counted once)
    Tc = 256
    rounds = T // Tc
    ref = _read_cut(product, x[:rounds * Tc * K], N, nfft, None)
    rx = product.multichannelrx(N, M, CP, TP, max_payload_len=300, defer_samples=2048)
    rx.monitor_enable(nfft, "hann")
    pipe = product.pipeline(rx, 0, 1, Tc)
    for c in range(rounds):
        pipe.push(d[c * Tc * K:(c + 1) * Tc * K], None if c == 0 else d[(c * Tc - 13) * K:c * Tc * K])
    pipe.wait()
    p = rx.monitor_read()
    pipe.close(); rx.close()
    assert (p.nseg, p.nsamp) == (ref.nseg, ref.nsamp)
    assert np.max(np.abs(p.psd - ref.psd) / ref.psd) < 1e-12 and np.max(np.abs(p.level - ref.level) / ref.level) < 1e-12
    assert np.array_equal(p.peak, ref.peak)


def _frames(product, N, iq, mode, pushes, **cfg):
    rx = product.multichannelrx(N, M, 8, TP, max_payload_len=400, **cfg)
    if mode != "never":
        rx.monitor_enable(64, "hann")
    if mode == "off_again":
        rx.monitor_disable()
    K = 2 * N
    nb = int(iq.numel()) // K // product.TILE * product.TILE
    step = max(product.TILE, nb // pushes // product.TILE * product.TILE)
    for b in range(0, nb, step):
        rx.Execute(iq[b * K:min(b + step, nb) * K])
    if mode == "on":
        assert rx.monitor_read().nsamp == nb
    rx.Flush()
    out = [(f.channel, f.header_valid, f.payload_valid, f.header, f.payload, f.end_sample, f.framesyms.tobytes()) for f in rx.frames]
    rx.close()
    return out


@pytest.mark.parametrize("shape", ["headline", "conv8", "chunked"])
def test_monitor_reads_and_never_perturbs(product, shape):
    N, nf, plen, fec1, pushes, cfg = {"headline": (512, 3, 300, product.LIQUID_FEC_HAMMING128, 3, {}),
                                      "conv8": (8, 24, 300, product.LIQUID_FEC_CONV_V27, 12, {}),
                                      "chunked": (64, 6, 300, product.LIQUID_FEC_HAMMING128, 2, {"chunk_blocks": 512})}[shape]
    tx = product.multichanneltx(N, M, 8, TP)
    iq, sent = tx.generate(nf, plen, fec1=fec1, seed=31)
    tx.close()
    never = _frames(product, N, iq, "never", pushes, **cfg)
    assert len(never) >= N * (nf - 1) and all(f[2] == 1 for f in never)
    assert _frames(product, N, iq, "on", pushes, **cfg) == never
    assert _frames(product, N, iq, "off_again", pushes, **cfg) == never


REFAPP = os.path.join(ROOT, "oracle", "_ref", "multichannel_rx_ref")


def _monitor_lines(path):
    rows = []
    for line in open(path).read().splitlines():
        v = line.split()
        rows.append((int(v[0]), float(v[1]), float(v[2]), np.array([float(t) for t in v[3:]])))
    return rows


@pytest.mark.skipif(not os.path.exists(REFAPP), reason="reference app binary not built")
def test_class_switches_on_the_unchanged_receiver_application(oracle, tmp_path):
    N, cp = 4, 8
    tx = oracle.MultiChannelTx(N, M, cp, TP)
    iq, _ = oracle.synth_traffic(N, M, cp, TP, 3, payload_len=120)
    f, mon = tmp_path / "iq.bin", tmp_path / "monitor.txt"
    iq.astype(np.complex64).tofile(f)
    del tx
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "liquid-usrp_amd", "host"), "-s"])
    base = dict(os.environ, MCRX_IQ_FILE=str(f), MCRX_IQ_PACKET="4096")
    args = [REFAPP, "-n", str(N), "-M", str(M), "-C", str(cp), "-T", str(TP), "-t", "0.5", "-v"]
    plain = subprocess.run(args, env=base, capture_output=True, text=True, timeout=120)
    out = subprocess.run(args, env=dict(base, MCRX_MONITOR="64", MCRX_MONITOR_FILE=str(mon)), capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and out.returncode == 0, out.stderr[-2000:]
    pk = r"channel: (\d+) rx packet id:\s+(\d+)\n"
    # (the application stops after 0.5 s of WALL time and the stand-in radio replays the file unpaced: how many passes a run
    #  gets through depends on the machine's load, so the two runs print the same sequence to different lengths -- on a busy
    #  machine they differed by four passes either way.  What the monitor must not change is the sequence.)
    got_mon, got_plain = re.findall(pk, out.stdout), re.findall(pk, plain.stdout)
    both = min(len(got_mon), len(got_plain))
    assert got_mon[:both] == got_plain[:both] and both >= 3 * N
    rows = _monitor_lines(mon)
    assert len(rows) % N == 0 and len(rows) >= N and [r[0] for r in rows[:N]] == list(range(N))
    assert all(len(r[3]) == 64 for r in rows)
    # the last report covers the stream since the last Reset (none here: everything that was pushed in whole tiles)
    chan = oracle.MultiChannelRx(N, M, cp, TP).channelize(iq[:len(iq) // (32 * N) * (32 * N)])
    level = 10 * np.log10(mm.monitor(chan, 64, 0)[0])
    got = np.array([r[1] for r in rows[-N:]])
    print("refapp monitor levels", got, "model", level)
    assert np.max(np.abs(got - level)) < 0.05
    bad = subprocess.run(args, env=dict(base, MCRX_MONITOR="48"), capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "MCRX_MONITOR" in bad.stderr


def test_scan_tool_marks_the_active_channels(oracle, tmp_path):
    N, active = 8, [1, 2, 5]
    x = whole_tiles(tx_stream(oracle, N, active, 3, 200) / N, N)
    f = tmp_path / "iq.bin"
    x.tofile(f)
    host = os.path.join(ROOT, "liquid-usrp_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s"])
    subprocess.check_call(["make", "-C", host, "-s", "mcrx_scan"])
    env = dict(os.environ, MCRX_IQ_FILE=str(f), MCRX_IQ_PACKET="4096")
    out = subprocess.run([os.path.join(host, "mcrx_scan"), "-n", str(N), "-M", str(M), "-C", str(CP), "-T", str(TP), "-i", "1", "-w", "64"],
                         env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = re.findall(r"^\s*(\d+)\s+(-?[\d.]+)\s+(-?[\d.]+)\s+(yes|no)\s*$", out.stdout, flags=re.M)
    assert len(rows) == N, out.stdout[-2000:]
    assert [int(c) for c, _, _, occ in rows if occ == "yes"] == active
    assert re.search(r"^\|.{64}\|$", out.stdout, flags=re.M), out.stdout[-2000:]
