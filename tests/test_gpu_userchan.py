"""Per-user channel emulator on the GPU (mcrx_hip_userchan_*) against the float64 model of tests/userchan_model.py,
against itself cut into pieces and into channel shards, and end to end: multichanneltx tiles -> userchan -> synthesize -> chanemu (noise)
-> multichannelrx, with the oracle's receiver on the same samples.

Bound, per component and per channel: |got - model| <= ((2T + 8) 2^-24 + 3e-7) * gain_c * sum|a_ci| * max|x_c| -- tap_bound of
tests/test_gpu_chanemu.py (the fp32 rounding of 2T fused multiply-adds plus rotation and gain, and sincos_u32's stated error): the
arithmetic has the same shapes."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import userchan_model as model

pytestmark = pytest.mark.gpu

DELAYS = [0, 1, 7, 8, 9, 16, 255]
NB = 128
RATIOS, PARITY = {}, {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def table(C_):
    """a seeded table of C_ channels: T cycles through 1 .. 4, delays from DELAYS (255 among them), gains over 30 dB, every channel with
    its own step and start phase"""
    rng = np.random.RandomState(100 + C_)
    chans = []
    for c in range(C_):
        T = (c + C_) % 4 + 1
        d = [int(v) for v in rng.choice(DELAYS, T)]
        if c == 0:
            d[-1] = 255
        taps = [(d[i], complex(rng.uniform(-1, 1), rng.uniform(-1, 1))) for i in range(T)]
        chans.append(dict(taps=taps, gain_db=-30.0 * c / max(C_ - 1, 1), cfo_step=int(rng.randint(1, 1 << 31)) * 2 + 1,
                          phase0=int(rng.randint(0, 1 << 31)) * 2 + (c & 1)))
    return chans


_X = {}


def samples(C_, nb, seed=7):
    """seeded unit-normal channel samples x[C_, nb] (complex64), made once per shape and left alone"""
    if (C_, nb, seed) not in _X:
        rng = np.random.RandomState(seed + 1000 * C_)
        _X[(C_, nb, seed)] = (rng.randn(C_, nb) + 1j * rng.randn(C_, nb)).astype(np.complex64)
    return _X[(C_, nb, seed)]


def device_tiles(x):
    torch = _torch()
    return torch.from_numpy(model.to_tiles(x)).cuda()


def host_channels(t, C_):
    return model.from_tiles(t.cpu().numpy(), C_)


def worst_ratio(got, want, chans, x):
    """the largest |got - want| per component over its channel's bound, asserted channel by channel"""
    w = 0.0
    for c, ch in enumerate(chans):
        d = got[c].astype(np.complex128) - want[c]
        dev, b = float(max(np.abs(d.real).max(), np.abs(d.imag).max())), model.bound(ch, x[c])
        assert dev <= b, (c, dev, b)
        w = max(w, dev / b)
    return w


def run(product, chans, x, first_block, lead):
    uc = product.userchan(channels=chans)
    assert uc.num_channels == len(chans) and uc.lead_blocks == model.lead_of(chans) <= lead
    got = host_channels(uc.apply(device_tiles(x), first_block, x.shape[1] - lead, lead), len(chans))
    uc.close()
    return got


# ---------------------------------------------------------------------------------------------- 1. identity
def test_identity(product):
    torch = _torch()
    C_ = 3
    x = samples(C_, 8 + NB)
    d_x = device_tiles(x)
    uc = product.userchan(channels=[dict(taps=[(0, 1.0)])] * C_)
    assert uc.num_channels == C_ and uc.lead_blocks == 0
    y = uc.apply(d_x, 0, 8 + NB)
    assert y.dtype == torch.complex64 and int(y.numel()) == (8 + NB) * C_ and torch.equal(y, d_x)
    y = uc.apply(d_x, 4096, NB, lead_blocks=8)
    assert int(y.numel()) == NB * C_ and torch.equal(y, d_x[8 * C_:])
    uc.close()
    N, M, cp, taper, nf, plen = 2, 64, 8, 4, 2, 96
    tx = product.multichanneltx(N, M, cp, taper)
    want, sent_want = tx.generate(nf, plen, seed=4242)
    uc = product.userchan(channels=[dict(taps=[(0, 1.0)])] * N)
    got, sent = uc.generate(tx, nf, plen, seed=4242)
    assert sent == sent_want and float(want.abs().max()) > 0
    assert got.shape == want.shape and torch.equal(got, want)
    uc.close(); tx.close()


# ---------------------------------------------------------------------------------------------- 2. the model
@pytest.mark.parametrize("C_", [1, 3, 8, 64])
def test_against_the_model(product, C_):
    chans = table(C_)
    lead = model.lead_of(chans)
    assert lead == 256
    x = samples(C_, lead + NB)
    first = 8 * 1234
    want = model.apply(x, chans, first, lead)
    assert float(np.abs(want).max()) > 1.0
    w = worst_ratio(run(product, chans, x, first, lead), want, chans, x)
    RATIOS["model_C%d" % C_] = w
    print("userchan C = %d: worst |got - model| over its channel's bound %.3f" % (C_, w))


# ---------------------------------------------------------------------------------------------- 3. indexing
def test_reversed_ray_tables_meet_the_same_bound(product):
    chans = table(8)
    lead = model.lead_of(chans)
    x = samples(8, lead + NB)
    want = model.apply(x, chans, 8 * 1234, lead)
    rev = [dict(ch, taps=ch["taps"][::-1]) for ch in chans]            # another sum of the same channel
    RATIOS["reversed_C8"] = worst_ratio(run(product, rev, x, 8 * 1234, lead), want, chans, x)


@pytest.mark.parametrize("odd", [0, 3, 7])
def test_a_channel_of_its_own_wherever_it_sits(product, odd):
    common = dict(taps=[(0, 0.5 + 0.5j), (9, 0.25j)], gain_db=-3.0, cfo_step=0x01234567, phase0=0x10000000)
    other = dict(taps=[(1, -0.75 + 0.1j), (8, 0.3 - 0.3j), (16, 0.2 + 0.1j)], gain_db=-20.0, cfo_step=0xF0F0F0F1, phase0=0xC0000000, delay=5)
    chans = [other if c == odd else common for c in range(8)]
    lead = model.lead_of(chans)
    assert lead == 24
    x = samples(8, lead + NB)
    want = model.apply(x, chans, 8 * 77, lead)
    got = run(product, chans, x, 8 * 77, lead)
    worst_ratio(got, want, chans, x)
    # ... and it is that channel's output, not a neighbour's parameters on its samples
    wrong = model.apply_channel(x[odd], common, 8 * 77, lead)
    assert float(np.abs(got[odd] - wrong).max()) > 100 * model.bound(other, x[odd])


# ---------------------------------------------------------------------------------------------- 4. cut anywhere
def test_cut_anywhere(product):
    torch = _torch()
    C_, total, extra = 3, 256, 16
    chans = table(C_)
    uc = product.userchan(channels=chans)
    lead = uc.lead_blocks
    L = lead + extra
    d_x = device_tiles(samples(C_, L + total))
    first = 8 * 999
    one = uc.apply(d_x[extra * C_:], first, total).clone()
    assert float(one.abs().max()) > 1.0
    for l in (lead, lead + extra):
        out = torch.full((total * C_ + 8,), float("nan"), dtype=torch.complex64, device="cuda")
        pos = 0
        for n in (8, 64, 8, 176):
            y = uc.apply(d_x[(L + pos - l) * C_:], first + pos, n, lead_blocks=l, out=out[pos * C_:])
            assert int(y.numel()) == n * C_
            pos += n
        assert pos == total
        assert torch.equal(torch.view_as_real(out[:total * C_]).view(torch.int32), torch.view_as_real(one).view(torch.int32)), l
        assert bool(torch.isnan(out[total * C_:].real).all())          # nothing stored behind it
    uc.close()


# ---------------------------------------------------------------------------------------------- 5. shards
def test_shards(product):
    C_ = 8
    chans = table(C_)
    uc = product.userchan(channels=chans)
    lead = uc.lead_blocks
    x = samples(C_, lead + NB)
    first = 8 * 55
    full = host_channels(uc.apply(device_tiles(x), first, NB), C_)
    for c0, cnt in ((0, 3), (3, 5)):
        sh = uc.shard(c0, cnt)
        assert sh.num_channels == cnt
        part = host_channels(sh.apply(device_tiles(x[c0:c0 + cnt]), first, NB, lead_blocks=lead), cnt)
        assert part.tobytes() == full[c0:c0 + cnt].tobytes(), (c0, cnt)
        sh.close()
    with pytest.raises(ValueError):
        uc.shard(5, 4)
    uc.close()


# ---------------------------------------------------------------------------------------------- 6. far positions
@pytest.mark.parametrize("name,first", [("2^40", 2 ** 40), ("minus_64", -64), ("across_2^32", 2 ** 32 - 64)])
def test_far_positions(product, name, first):
    C_ = 3
    chans = table(C_)
    lead = model.lead_of(chans)
    x = samples(C_, lead + NB).copy()
    if first < 0:
        x[:, :lead - first] = 0                                         # zeros in front of block 0
    want = model.apply(x, chans, first, lead)
    got = run(product, chans, x, first, lead)
    RATIOS["far_" + name] = worst_ratio(got, want, chans, x)
    # ... and it is not the stream at another position
    assert float(np.abs(got - model.apply(x, chans, first + 8, lead)).max()) > 0.01


# ---------------------------------------------------------------------------------------------- 7. errors on the device
def test_errors_on_the_device(product):
    torch = _torch()
    L, EINVAL, OK = product.lib(), product.MCRX_EINVAL, product.MCRX_OK
    C_, n = 3, 64
    chans = [dict(taps=[(0, 1.0), (9, 0.5j)], cfo_step=77)] * C_          # lead 16
    uc = product.userchan(channels=chans)
    lead = uc.lead_blocks
    assert lead == 16
    d_x = torch.zeros(4 * (lead + n) * C_, dtype=torch.complex64, device="cuda")
    d_y = torch.zeros(4 * n * C_, dtype=torch.complex64, device="cuda")
    px, py = d_x.data_ptr(), d_y.data_ptr()
    bi, bo = 8 * (lead + n) * C_, 8 * n * C_

    def call(a, b, first=0, count=n, ld=lead, h=uc._h):
        return L.mcrx_hip_userchan_apply_tiles(h, C.c_void_p(a) if a else None, first, count, ld, C.c_void_p(b) if b else None, None)
    assert call(px, py, h=None) == EINVAL
    assert call(None, py) == EINVAL and call(px, None) == EINVAL
    assert call(px + 8, py) == EINVAL and call(px, py + 8) == EINVAL      # 16 bytes
    assert call(px, py, count=n + 4) == EINVAL and call(px, py, first=4) == EINVAL and call(px, py, first=-12) == EINVAL
    assert call(px, py, ld=lead + 4) == EINVAL                            # the lead comes in granules too
    assert call(px, py, ld=lead - 8) == EINVAL                            # below the handle's
    assert call(px, px) == EINVAL                                         # in place
    assert call(px, px + bi - 16) == EINVAL                               # the output's first pair on the input's last
    assert call(px + bo, px + 16) == EINVAL                               # the output's last pair on the input's first
    assert L.mcrx_hip_userchan_last_error()
    assert call(px, px + bi) == OK and call(px + bo, px) == OK            # adjacent is not overlapping
    assert call(px, py, first=-64) == OK and call(px, py, count=0) == OK
    with pytest.raises(ValueError):
        uc.apply(d_x, 0, n, out=d_x)                                      # in place
    with pytest.raises(ValueError):
        uc.apply(d_x[:8], 0, n)
    with pytest.raises(TypeError):
        uc.apply(d_x.real, 0, n)
    torch.cuda.synchronize()
    # the handle stays usable, belongs to its device, and calls put the caller's device back
    x = samples(C_, lead + n)
    other = 1 if torch.cuda.device_count() > 1 else 0
    torch.cuda.set_device(other)
    try:
        y = uc.apply(device_tiles(x).to("cuda:0"), 8, n)
        torch.cuda.synchronize(0)
        assert torch.cuda.current_device() == other
    finally:
        torch.cuda.set_device(0)
    worst_ratio(host_channels(y, C_), model.apply(x, chans, 8, lead), chans, x)
    uc.close()
    uc.close()                                                            # twice is harmless


# ---------------------------------------------------------------------------------------------- 8. end to end
LEVELS_DB = [0, -30, -10, -20, -3, -27, -15, -6]
CFO = [0.45, -0.45, 0.3, -0.2, 0.0, 0.4, -0.35, 0.1]
TIMING = [0, 3, 7, 1, 12, 5, 9, 2]
TRAFFIC_SEED = 85


@pytest.mark.parametrize("name,noise_ratio", [("clean", 0.0), ("noise_0.006rms", 0.006)])
def test_end_to_end(product, oracle, name, noise_ratio):
    """Eight users, each with their own three rays, oscillator, timing and level (30 dB between the strongest and the weakest, side by
    side in the bank): multichanneltx tiles -> userchan -> synthesize -> chanemu (noise only) -> multichannelrx, and the oracle's
    receiver on the same samples.  framesyms: the deviation is recorded (PARITY, printed by the last test) and held to the loosest
    bar check_frames uses, 1e-3, as tests/test_gpu_chanemu.py does."""
    from test_gpu_parity import match_frames, relerr, relerr_elem
    torch = _torch()
    N, M, cp, taper, nf, plen = 8, 64, 8, 4, 3, 96
    K = 2 * N
    chans = [dict(taps=[(0, 1.0), (1 + c % 3, (0.25 - 0.15j) * np.exp(1j * c)), (4, (-0.10 + 0.15j) * np.exp(-2j * c))],
                  gain_db=float(LEVELS_DB[c]), cfo_step=product.userchan_cfo_step(CFO[c], M), delay=TIMING[c]) for c in range(N)]
    uc = product.userchan(channels=chans)
    tx = product.multichanneltx(N, M, cp, taper)
    iq, sent = uc.generate(tx, nf, plen, seed=TRAFFIC_SEED)          # QPSK / Hamming(12,8), gain 1 / N
    uc.close(); tx.close()
    iq = torch.cat([iq, torch.zeros(64 * K, dtype=torch.complex64, device="cuda")])           # (room behind the delayed users' last frames)
    rms = float(torch.view_as_real(iq).pow(2).sum().div(int(iq.numel())).sqrt())
    assert rms > 0
    ce = product.chanemu(taps=[(0, 1.0)], noise_std=noise_ratio * rms, seed=2024)
    y = ce.execute(iq)
    ce.close()
    assert int(y.numel()) % (product.TILE * K) == 0
    y_host = y.cpu().numpy()
    rx = product.multichannelrx(N, M, cp, taper, max_payload_len=plen)
    if not noise_ratio:
        rx.monitor_enable()
    rx.Execute(y); rx.Flush()
    if not noise_ratio:
        level = rx.monitor_read().level_db()
        print("userchan monitor levels [dB]: " + " ".join("%.1f" % v for v in level))
        assert list(np.argsort(level)) == list(np.argsort(LEVELS_DB)), level
    ora = oracle.MultiChannelRx(N, M, cp, taper)
    ora.execute(np.ascontiguousarray(y_host))
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
        assert (fg.header_valid, fg.payload_valid) == (fo.header_valid, fo.payload_valid)
        assert bytes(fg.header) == bytes(fo.header) and bytes(fg.payload) == bytes(fo.payload)
        assert len(fg.framesyms) == len(fo.framesyms) > 0
        w, we = max(w, relerr(fg.framesyms, fo.framesyms)), max(we, relerr_elem(fg.framesyms, fo.framesyms))
    rx.close()
    PARITY[name] = {"max_norm": w, "element_wise": we, "noise_std": noise_ratio * rms, "rms": rms}
    print("userchan_parity %s: framesyms max-norm %.3e element-wise %.3e" % (name, w, we))
    assert w <= 1e-3, w


def test_zz_print_userchan_deviations():
    """(last of this file: the figures measured above as one JSON line each -- profiles/userchan_model.json and
    profiles/userchan_parity.json are such records; USERCHAN_OUT / USERCHAN_PARITY_OUT name files to write them to as well)"""
    for tag, rec, env in (("userchan_model", RATIOS, "USERCHAN_OUT"), ("userchan_parity", PARITY, "USERCHAN_PARITY_OUT")):
        line = json.dumps(rec, sort_keys=True)
        print(tag + " " + line)
        path = os.environ.get(env)
        if path:
            with open(path, "w") as f:
                f.write(line + "\n")
