"""The payload workers' integer diet (csrc/payload_lean.hpp, payload_wide.hpp: the frame oscillator's phase carried per lane instead of
three 32-bit multiplies per symbol, loop-invariant branches hoisted into instantiations) may not move a bit: no floating-point
instruction changed its operands or its place.  Every delivered frame -- record words (flags, evm / rssi / cfo as their bits, where it
ended), payload bytes and equalised symbols -- is compared as BYTES with fixtures recorded from the library of the commit before that
change (tests/golden/payload_diet_*.npz, written by tests/golden/make_payload_diet.py: SHA-256 digests per frame, and of the input so
that a drifting input is told from a drifting kernel), and against the oracle at the usual bar (flags, headers, payloads equal,
framesyms within 1e-5).

Shapes are the smallest that reach every changed path: 8 channels of 64 subcarriers (payload_lean_kernel<63,64>), QPSK / Hamming(12,8)
and BPSK, 1200-byte (165 QPSK symbols: the steady loop) and 64-byte payloads, three frames per channel; once with a carrier offset of
1.6e-3 rad per channel sample (the upper end of tests/test_gpu_parity.py) under 20 dB AWGN -- every symbol's oscillator trim is then
non-zero and of either sign, which is what the signed 24-bit lane step has to get right -- and once clean; hard decisions and
skip_framesyms = 2 (the other instantiations); 48 subcarriers (payload_lean_kernel<63,48>); worker_build = 1 (the XB = 0 build);
two channels of 256 subcarriers with 16-QAM / Golay (payload_wide_kernel, lane indices up to 255 times the trim); and one stream
pushed in pieces that cut frames, so that first and last windows of a push take load_win's clamped path and a frame resumes from the
oscillator step its worker wrote back."""
import hashlib
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL = 1e-5                      # framesyms against the oracle: max |gpu - oracle| over the largest |oracle| of the frame

QPSK, BPSK, QAM16 = 40, 39, 27
NONE, H128, GOLAY = 1, 6, 7

# a stream: what is sent and what the channel does to it.  w = carrier offset in rad per WIDEBAND sample (x 2N per channel sample)
STREAMS = {
    "m64_qpsk_1200_cfo":   dict(N=8, M=64, cp=8, mod=QPSK, fec1=H128, plen=1200, nf=3, w=+1.0e-4, snr_db=20.0),
    "m64_qpsk_1200_clean": dict(N=8, M=64, cp=8, mod=QPSK, fec1=H128, plen=1200, nf=3, w=0.0, snr_db=None),
    "m64_qpsk_64_cfo":     dict(N=8, M=64, cp=8, mod=QPSK, fec1=H128, plen=64, nf=3, w=-1.0e-4, snr_db=20.0),
    "m64_qpsk_64_clean":   dict(N=8, M=64, cp=8, mod=QPSK, fec1=H128, plen=64, nf=3, w=0.0, snr_db=None),
    "m64_bpsk_1200_cfo":   dict(N=8, M=64, cp=8, mod=BPSK, fec1=NONE, plen=1200, nf=3, w=-1.0e-4, snr_db=20.0),
    "m64_bpsk_1200_clean": dict(N=8, M=64, cp=8, mod=BPSK, fec1=NONE, plen=1200, nf=3, w=0.0, snr_db=None),
    "m64_bpsk_64_cfo":     dict(N=8, M=64, cp=8, mod=BPSK, fec1=NONE, plen=64, nf=3, w=+1.0e-4, snr_db=20.0),
    "m64_bpsk_64_clean":   dict(N=8, M=64, cp=8, mod=BPSK, fec1=NONE, plen=64, nf=3, w=0.0, snr_db=None),
    "m48_qpsk_1200_cfo":   dict(N=8, M=48, cp=6, mod=QPSK, fec1=H128, plen=1200, nf=3, w=+1.0e-4, snr_db=20.0),
    "m48_bpsk_64_clean":   dict(N=8, M=48, cp=6, mod=BPSK, fec1=NONE, plen=64, nf=3, w=0.0, snr_db=None),
    # 288-sample symbols: the same phase advance per symbol as above (0.115 rad), 25 dB as the parity tests use for 16-QAM
    "m256_qam16_cfo":      dict(N=2, M=256, cp=32, mod=QAM16, fec1=GOLAY, plen=600, nf=2, w=+1.0e-4, snr_db=25.0),
}
# a case: (stream, receiver configuration, how the stream is pushed)
CASES = {name: (name, {}, "once") for name in STREAMS}
CASES.update({
    "m64_qpsk_1200_cfo_hard":   ("m64_qpsk_1200_cfo", dict(payload_soft=0), "once"),
    "m64_qpsk_1200_cfo_nosyms": ("m64_qpsk_1200_cfo", dict(skip_framesyms=2), "once"),
    "m64_bpsk_64_clean_hard":   ("m64_bpsk_64_clean", dict(payload_soft=0), "once"),
    "m64_bpsk_64_clean_nosyms": ("m64_bpsk_64_clean", dict(skip_framesyms=2), "once"),
    "m64_qpsk_1200_cfo_valu":   ("m64_qpsk_1200_cfo", dict(worker_build=1), "once"),
    "m64_qpsk_1200_cfo_pieces": ("m64_qpsk_1200_cfo", {}, "pieces"),
    "m64_bpsk_1200_cfo_pieces": ("m64_bpsk_1200_cfo", {}, "pieces"),
    "m256_qam16_cfo_pieces":    ("m256_qam16_cfo", {}, "pieces"),
})
CASE_IDS = sorted(CASES)


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def sha_rows(items):
    """SHA-256 of every item, a row of 32 bytes each"""
    return np.frombuffer(b"".join(hashlib.sha256(bytes(b)).digest() for b in items), np.uint8).reshape(-1, 32)


_STREAM = {}


def stream(oracle, name):
    """the wideband samples of a stream (whole tiles), computed once and never written to"""
    if name not in _STREAM:
        p = STREAMS[name]
        N = p["N"]
        iq, sent = oracle.synth_traffic(N, p["M"], p["cp"], 4, p["nf"], payload_len=p["plen"], mod=p["mod"], fec1=p["fec1"], seed=1000 + p["M"] + p["mod"])
        x = iq.astype(np.complex128)
        if p["w"]:
            x = 0.73 * x * np.exp(1j * (p["w"] * np.arange(len(x)) + 0.4))
        if p["snr_db"] is not None:
            rng = np.random.RandomState(p["M"] + p["plen"])
            nstd = np.sqrt(np.mean(np.abs(iq) ** 2)) * 10.0 ** (-p["snr_db"] / 20.0) / np.sqrt(2.0)
            x = x + nstd * (rng.randn(len(x)) + 1j * rng.randn(len(x)))
        x = np.ascontiguousarray(x.astype(np.complex64))
        x.setflags(write=False)
        _STREAM[name] = (x, sent)
    return _STREAM[name]


def cuts(ntiles, how):
    if how == "once":
        return [(0, ntiles)]
    t1 = ntiles // 3 + 1                  # three uneven pieces, the middle one a single tile
    return [(0, t1), (t1, t1 + 1), (t1 + 1, ntiles)]


def run_case(product, oracle, case):
    """-> (digest of the input, the delivered frames in the reference's order)"""
    torch = _torch()
    sname, cfg, how = CASES[case]
    p = STREAMS[sname]
    x, _ = stream(oracle, sname)
    tile = product.TILE * 2 * p["N"]
    ntiles = len(x) // tile
    data = torch.from_numpy(np.array(x[:ntiles * tile])).cuda()            # (a copy: the shared stream is read-only)
    rx = product.multichannelrx(p["N"], p["M"], p["cp"], 4, max_payload_len=max(p["plen"], 64), **cfg)
    for a, b in cuts(ntiles, how):
        rx.Execute(data[a * tile:b * tile])
    rx.Flush()
    frames = sorted(rx.frames, key=lambda f: (f.end_sample, f.channel))
    rx.close()
    return sha(x[:ntiles * tile].tobytes()), frames


def record_words(f):
    """a frame's record, floats as their bits"""
    return repr((f.channel, f.header, f.header_valid, f.payload_valid, len(f.payload), struct.pack("<3f", f.evm, f.rssi, f.cfo),
                 f.mod_scheme, f.mod_bps, f.check, f.fec0, f.fec1, f.end_sample, len(f.framesyms))).encode()


def digests(frames):
    """per frame: (record words, payload bytes, equalised symbols)"""
    return {"records": sha_rows(record_words(f) for f in frames),
            "payloads": sha_rows(f.payload for f in frames),
            "syms": sha_rows(np.ascontiguousarray(f.framesyms).view(np.uint32).tobytes() for f in frames)}


_ORACLE = {}


def oracle_frames(oracle, sname, soft):
    if (sname, soft) not in _ORACLE:
        p = STREAMS[sname]
        x, _ = stream(oracle, sname)
        tile = 16 * 2 * p["N"]
        ora = oracle.MultiChannelRx(p["N"], p["M"], p["cp"], 4, soft=soft)
        ora.execute(x[:len(x) // tile * tile])
        _ORACLE[(sname, soft)] = ora.frames
    return _ORACLE[(sname, soft)]


def golden():
    path = os.path.join(GOLDEN, "payload_diet_frames.npz")
    assert os.path.exists(path), "fixture missing: tests/golden/make_payload_diet.py records it from the parent commit's library"
    return np.load(path)


@pytest.mark.parametrize("case", CASE_IDS)
def test_frames_equal_the_parent_commits_bytes(oracle, product, case):
    sname, cfg, how = CASES[case]
    p = STREAMS[sname]
    assert product.TILE == 16
    g = golden()
    inp, frames = run_case(product, oracle, case)
    assert inp == str(g[case + "/input"]), "the input drifted, not the kernel"
    # ---- the oracle's bar
    ora = oracle_frames(oracle, sname, cfg.get("payload_soft", 1) != 0)
    assert len(ora) >= p["N"] * p["nf"] - 1 and len(frames) == len(ora)
    if p["snr_db"] is None:
        assert len(frames) == p["N"] * p["nf"] and all(f.header_valid and f.payload_valid for f in frames)
    by_ch = {}
    for fo in ora:
        by_ch.setdefault(fo.channel, []).append(fo)
    seen, worst = {}, 0.0
    for f in frames:
        k = seen.get(f.channel, 0)
        seen[f.channel] = k + 1
        fo = by_ch[f.channel][k]
        assert (f.header_valid, f.payload_valid) == (fo.header_valid, fo.payload_valid), (f.channel, k)
        assert f.header == fo.header and f.payload == fo.payload, (f.channel, k)
        if cfg.get("skip_framesyms", 0) == 2:
            continue                                    # (the caller said it never reads stats.framesyms)
        assert len(f.framesyms) == len(fo.framesyms)
        if len(fo.framesyms):
            worst = max(worst, float(np.max(np.abs(f.framesyms - fo.framesyms)) / max(float(np.max(np.abs(fo.framesyms))), 1e-30)))
    print(case, len(frames), "frames, worst framesyms rel err %.3g" % worst)
    assert worst <= REL, worst
    # ---- the parent commit's bytes, frame by frame
    d = digests(frames)
    for what in ("records", "payloads", "syms"):
        want, got = g[case + "/" + what], d[what]
        assert got.shape == want.shape, (what, got.shape, want.shape)
        bad = [i for i in range(len(got)) if not np.array_equal(got[i], want[i])]
        assert not bad, "%s of %d frames differ from the parent's, first: frame %d (channel %d)" % (what, len(bad), bad[0], frames[bad[0]].channel)
