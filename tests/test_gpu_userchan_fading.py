"""Fading rays per user of the per-user channel emulator on the GPU (mcrx_hip_userfade_*) against the float64
model of tests/userchan_fading_model.py fed with the integers the library reports (so integer parity is exact), against a handle
without fading, against itself cut into pieces, into spans of the gain table and into channel shards, and far out on the block axis.

Bounds, per component.  The gain kernel, with Gs = c_los + S c_sc: |got - G| <= Gs (3e-7 + (S + 2) 2^-24), the gain-kernel bound of
tests/test_gpu_chanemu_fading.py (sincos_u32 on every term, the line-of-sight product, S + 1 roundings of the sum).  apply():
userchan_fading_model.bound -- userchan_model.bound with every |a_i| scaled by that ray's largest |G|, plus the roundings of the table
entry, the interpolation and the product g a, derived there."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import test_gpu_userchan as base
import userchan_fading_model as fmodel
import userchan_model as model
from test_userchan_fading import BAD, library_tables

pytestmark = pytest.mark.gpu

NB = 128
RATIOS = {}
_torch, samples, device_tiles, host_channels = base._torch, base.samples, base.device_tiles, base.host_channels


def table(C_, rot=True):
    """tests/test_gpu_userchan.py's seeded table (T cycles through 1 .. 4, delays of both parities from [0, 1, 7, 8, 9, 16, 255], gains
    over 30 dB, every channel its own oscillator), or the same without oscillators"""
    chans = base.table(C_)
    return chans if rot else [dict(ch, cfo_step=0, phase0=0) for ch in chans]


def fading(chans, L, S, seed=21, table_rows=0, mix=True):
    """every user their own Dopplers (up to 0.12 / B), Rice factors and line-of-sight terms; with `mix` every third user (c % 3 == 1)
    does not fade"""
    rng = np.random.RandomState(500 + len(chans) + L)
    B = float(1 << L)
    users = []
    for c, ch in enumerate(chans):
        T = len(ch["taps"])
        if mix and c % 3 == 1:
            users.append(None)
            continue
        users.append(dict(doppler=[float(v) for v in rng.uniform(0.02, 0.12, T) / B], rice_k=[float(v) for v in rng.choice([0.0, 1.0, 8.0], T)],
                          los_doppler=[float(v) for v in rng.uniform(-0.1, 0.1, T) / B], los_phase=[int(v) for v in rng.randint(0, 1 << 31, T)]))
    return dict(log2_block=L, sinusoids=S, seed=seed, table_rows=table_rows, users=users)


def tables_of(product, uc, chans):
    return library_tables(product, uc._fading, [len(ch["taps"]) for ch in chans])


def bits(t):
    torch = _torch()
    return torch.view_as_real(t).view(torch.int32)


def check(product, chans, fade, x, first, lead, tag):
    """apply() of a fading handle against the model, channel by channel; returns (worst over bound, the output as channels)"""
    uc = product.userchan(channels=chans, fading=fade)
    assert uc.fading_on() and uc.lead_blocks == model.lead_of(chans) <= lead
    tabs = tables_of(product, uc, chans)
    got = host_channels(uc.apply(device_tiles(x), first, x.shape[1] - lead, lead), len(chans))
    uc.close()
    w = 0.0
    for c, ch in enumerate(chans):
        want, peaks = fmodel.apply_channel(x[c], ch, tabs[c], fade["log2_block"], first, lead)
        d = got[c].astype(np.complex128) - want
        dev, b = float(max(np.abs(d.real).max(), np.abs(d.imag).max())), fmodel.bound(ch, tabs[c], peaks, fade["sinusoids"], x[c])
        assert dev <= b, (tag, c, dev, b)
        w = max(w, dev / b)
        if tabs[c] is not None and c < 3:            # ... and it is not the static channel
            assert float(np.abs(got[c] - model.apply_channel(x[c], ch, first, lead)).max()) > 1e-3 * model.gain_of(ch), (tag, c)
    RATIOS[tag] = w
    print("userchan fading %s: worst |got - model| over its channel's bound %.3f" % (tag, w))
    return w, got


# ---------------------------------------------------------------------------------------------- 1. the gain kernel
@pytest.mark.parametrize("C_,S,L", [(1, 1, 3), (3, 8, 4), (64, 16, 10)])
def test_gains_against_the_model(product, C_, S, L):
    torch = _torch()
    chans = table(C_)
    uc = product.userchan(channels=chans, fading=fading(chans, L, S))
    tabs = tables_of(product, uc, chans)
    rows = 20                                                    # three chunks of the kernel's eight rows, the last one short
    for first in (0, -2, 2 ** 37):
        got = uc.gains(first, rows)
        assert got.dtype == torch.complex64 and tuple(got.shape) == (rows, C_, 4)
        got = got.cpu().numpy()
        for c, ch in enumerate(chans):
            T = len(ch["taps"])
            assert np.all(got[:, c, T:] == 1.0)                  # rays the channel does not have
            if tabs[c] is None:
                assert np.all(got[:, c, :] == 1.0)               # a user who does not fade: G = (1, 0) exactly
                continue
            for i, t in enumerate(tabs[c]):
                want = fmodel.grid_rows(t, first, rows, L)
                d = got[:, c, i].astype(np.complex128) - want
                dev, b = float(max(np.abs(d.real).max(), np.abs(d.imag).max())), (t[2][0] + S * t[2][1]) * (3e-7 + (S + 2) * 2.0 ** -24)
                assert dev <= b, (first, c, i, dev, b)
    assert float(np.abs(got - 1.0).max()) > 0.1
    uc.set_fading(None)
    d = torch.zeros(64 * C_, dtype=torch.complex64, device="cuda")
    L_ = product.lib()
    assert L_.mcrx_hip_userfade_gains(uc._h, 0, 8, C.c_void_p(d.data_ptr()), None) == product.MCRX_EINVAL       # fading off
    uc.close()


# ---------------------------------------------------------------------------------------------- 2. the model
@pytest.mark.parametrize("rot", [True, False], ids=["rot", "norot"])
@pytest.mark.parametrize("C_", [1, 3, 8, 64])
def test_apply_against_the_model(product, C_, rot):
    chans = table(C_, rot)
    lead = model.lead_of(chans)
    assert lead == 256
    x = samples(C_, lead + NB)
    check(product, chans, fading(chans, 4, 8), x, 8 * 1234, lead, "model_C%d_%s" % (C_, "rot" if rot else "norot"))


# ---------------------------------------------------------------------------------------------- 3. off is the parent
def test_fading_off_is_the_parent(product):
    torch = _torch()
    C_ = 8
    for rot in (True, False):
        chans = table(C_, rot)
        fade = fading(chans, 4, 8)
        lead = model.lead_of(chans)
        d_x = device_tiles(samples(C_, lead + NB))
        plain = product.userchan(channels=chans)
        assert not plain.fading_on()
        ref = plain.apply(d_x, 8 * 77, NB).clone()
        plain.close()
        uc = product.userchan(channels=chans, fading=fade)
        y = uc.apply(d_x, 8 * 77, NB).clone()
        yc, rc = y.view(-1, C_, 8), ref.view(-1, C_, 8)
        for c in range(C_):
            if fade["users"][c] is None:                                   # a user who does not fade, inside a fading handle
                assert torch.equal(yc[:, c], rc[:, c]), (rot, c)
            else:
                assert not torch.equal(yc[:, c], rc[:, c]), (rot, c)
        uc.set_fading(None)
        assert not uc.fading_on()
        assert torch.equal(bits(uc.apply(d_x, 8 * 77, NB)), bits(ref)), rot   # the handle that never faded, bit for bit
        uc.set_fading(fade)
        assert uc.fading_on() and torch.equal(bits(uc.apply(d_x, 8 * 77, NB)), bits(y))
        uc.close()
        late = product.userchan(channels=chans)                            # a handle made static and switched on later
        late.set_fading(fade)
        assert torch.equal(bits(late.apply(d_x, 8 * 77, NB)), bits(y))
        late.close()


# ---------------------------------------------------------------------------------------------- 4. cut anywhere
@pytest.mark.parametrize("L,cuts", [(4, (8, 64, 8, 176)), (3, (8, 8, 16, 224))], ids=["L4", "L3"])
def test_cut_anywhere(product, L, cuts):
    """L = 4, first = 8 * 999 (half a gain interval in): the cuts behind 8 and 72 blocks fall on row boundaries, the one behind 80 inside
    an interval; L = 3: one granule per row, every cut on a row boundary.  Two sufficient leads each."""
    torch = _torch()
    C_, total, extra = 3, 256, 16
    chans = table(C_)
    uc = product.userchan(channels=chans, fading=fading(chans, L, 8, mix=False))
    lead = uc.lead_blocks
    LL = lead + extra
    d_x = device_tiles(samples(C_, LL + total))
    first = 8 * 999
    ends = np.cumsum(cuts) + first
    assert sum(cuts) == total and any(e % (1 << L) == 0 for e in ends[:-1]) and (L == 3 or any(e % (1 << L) for e in ends[:-1]))
    one = uc.apply(d_x[extra * C_:], first, total).clone()
    assert float(one.abs().max()) > 1.0
    for l in (lead, lead + extra):
        out = torch.full((total * C_ + 8,), float("nan"), dtype=torch.complex64, device="cuda")
        pos = 0
        for n in cuts:
            y = uc.apply(d_x[(LL + pos - l) * C_:], first + pos, n, lead_blocks=l, out=out[pos * C_:])
            assert int(y.numel()) == n * C_
            pos += n
        assert torch.equal(bits(out[:total * C_]), bits(one)), l
        assert bool(torch.isnan(out[total * C_:].real).all())          # nothing stored behind it
    uc.close()


# ---------------------------------------------------------------------------------------------- 5. spans
def test_spans_of_the_gain_table(product):
    """table_rows = 2 at L = 3: a span is one grid interval, 512 blocks are 64 spans -- and the same bits as one span"""
    torch = _torch()
    C_, total = 3, 512
    chans = table(C_)
    lead = model.lead_of(chans)
    d_x = device_tiles(samples(C_, lead + total))
    outs = []
    for rows in (2, 0, 5):
        uc = product.userchan(channels=chans, fading=fading(chans, 3, 8, table_rows=rows))
        outs.append(uc.apply(d_x, -8 * 3, total).clone())
        uc.close()
    assert float(outs[0].abs().max()) > 1.0
    assert torch.equal(bits(outs[0]), bits(outs[1])) and torch.equal(bits(outs[2]), bits(outs[1]))


def test_the_gain_table_grows_and_is_reused(product):
    """L = 3, 8 channels, the default table: 64 blocks in the first allocation (10 rows), 1 024 that force the table to grow, 64 again in
    the grown one -- each call the bits of a fresh handle's"""
    torch = _torch()
    C_, total = 8, 1024
    chans = table(C_)
    fade = fading(chans, 3, 8)
    lead = model.lead_of(chans)
    d_x = device_tiles(samples(C_, lead + total))
    uc = product.userchan(channels=chans, fading=fade)
    for n in (64, 1024, 64):
        fresh = product.userchan(channels=chans, fading=fade)
        got, want = uc.apply(d_x, 8 * 999, n), fresh.apply(d_x, 8 * 999, n)
        assert int(got.numel()) == n * C_ and float(got.abs().max()) > 1.0
        assert torch.equal(bits(got), bits(want)), n
        fresh.close()
    uc.close()


# ---------------------------------------------------------------------------------------------- 6. shards
def test_shards_keep_their_users(product):
    C_ = 8
    chans = table(C_)
    fade = fading(chans, 4, 8)
    uc = product.userchan(channels=chans, fading=fade)
    lead = uc.lead_blocks
    x = samples(C_, lead + NB)
    first = 8 * 55
    full = host_channels(uc.apply(device_tiles(x), first, NB), C_)
    for c0, cnt in ((0, 3), (3, 5)):
        sh = uc.shard(c0, cnt)
        assert sh.num_channels == cnt and sh.fading_on()
        assert [u.id for u in sh._fading[1]] == list(range(c0, c0 + cnt))
        assert [u.enabled for u in sh._fading[1]] == [0 if fade["users"][c] is None else 1 for c in range(c0, c0 + cnt)]
        part = host_channels(sh.apply(device_tiles(x[c0:c0 + cnt]), first, NB, lead_blocks=lead), cnt)
        assert part.tobytes() == full[c0:c0 + cnt].tobytes(), (c0, cnt)
        sh.close()
    # ... and a table of the same users with ids of its own is another channel
    other = product.userchan(channels=chans[3:], fading=dict(fade, users=fade["users"][3:]))
    part = host_channels(other.apply(device_tiles(x[3:]), first, NB, lead_blocks=lead), 5)
    assert part[0].tobytes() != full[3].tobytes() and part[1].tobytes() == full[4].tobytes()      # (user 4 does not fade)
    other.close(); uc.close()


# ---------------------------------------------------------------------------------------------- 7. far positions
FAR = [("2^40", 2 ** 40, 4), ("minus_64", -64, 4), ("across_2^32_L10", 2 ** 32 - 64, 10)]


@pytest.mark.parametrize("name,first,L", FAR, ids=[f[0] for f in FAR])
def test_far_positions(product, name, first, L):
    C_ = 3
    chans = table(C_)
    lead = model.lead_of(chans)
    x = samples(C_, lead + NB).copy()
    if first < 0:
        x[:, :lead - first] = 0                                         # zeros in front of block 0
    fade = fading(chans, L, 8, mix=False)
    _, got = check(product, chans, fade, x, first, lead, "far_" + name)
    # ... and it is not the stream one grid interval further on
    uc = product.userchan(channels=chans, fading=fade)
    tabs = tables_of(product, uc, chans)
    uc.close()
    assert float(np.abs(got[0] - fmodel.apply_channel(x[0], chans[0], tabs[0], L, first + (1 << L), lead)[0]).max()) > 1e-3


# ---------------------------------------------------------------------------------------------- 8. errors on the device
@pytest.mark.parametrize("what,spoil", BAD, ids=[b[0] for b in BAD])
def test_set_errors_leave_the_handle_as_it_was(product, what, spoil):
    torch = _torch()
    L_ = product.lib()
    chans = [dict(taps=[(0, 1.0), (9, 0.5j), (3, 0.25)], cfo_step=77)] * 2
    good = dict(log2_block=10, sinusoids=8, seed=5, users=[dict(doppler=1e-5, rice_k=1.0, los_doppler=-1e-5)] * 2)
    d_x = device_tiles(samples(2, 16 + 64))
    plain = product.userchan(channels=chans)
    faded = product.userchan(channels=chans, fading=dict(good, log2_block=4, users=[dict(doppler=5e-3)] * 2))
    before = faded.apply(d_x, 0, 64).clone()
    f, users = product.userchan_fading([3, 3], **good)
    spoil(f, users[1])
    for uc in (plain, faded):
        assert L_.mcrx_hip_userfade_set(uc._h, C.addressof(f), C.addressof(users)) == product.MCRX_EINVAL, what
        assert L_.mcrx_hip_userchan_last_error()
    assert L_.mcrx_hip_userfade_set(faded._h, C.addressof(f), None) == product.MCRX_EINVAL
    assert not plain.fading_on() and faded.fading_on()
    assert torch.equal(bits(faded.apply(d_x, 0, 64)), bits(before))
    d = torch.zeros(64, dtype=torch.complex64, device="cuda")
    assert L_.mcrx_hip_userfade_gains(faded._h, 0, 2, C.c_void_p(d.data_ptr() + 8), None) == product.MCRX_EINVAL      # 16 bytes
    assert L_.mcrx_hip_userfade_gains(faded._h, 0, 2, None, None) == product.MCRX_EINVAL
    assert L_.mcrx_hip_userfade_gains(faded._h, 0, 0, C.c_void_p(d.data_ptr()), None) == product.MCRX_OK
    if "doppler" in what or "rice" in what:          # entries beyond a channel's rays, and those of a user who does not fade, are ignored
        two = product.userchan(channels=[dict(taps=[(0, 1.0), (9, 0.5j)])] * 2)
        assert L_.mcrx_hip_userfade_set(two._h, C.addressof(f), C.addressof(users)) == product.MCRX_OK and two.fading_on()
        two.close()
        users[1].enabled = 0
        assert L_.mcrx_hip_userfade_set(plain._h, C.addressof(f), C.addressof(users)) == product.MCRX_OK and plain.fading_on()
    plain.close(); faded.close()


# ---------------------------------------------------------------------------------------------- 9. end to end
PARITY = {}
E2E_N, E2E_M, E2E_CP, E2E_TAPER, E2E_NF, E2E_PLEN = 8, 64, 8, 4, 3, 96
SEED_A, SEED_B = 1, 4


def e2e_fading(product, case):
    """case A: Rician, K = 10, every user their own Doppler of 0.002 .. 0.005 cycles per OFDM symbol and a line-of-sight shift of up to
    0.001; case B: Rayleigh, every user their own Doppler of 0.012 .. 0.02 cycles per symbol.  Gains updated every 16 blocks."""
    N, M, cp = E2E_N, E2E_M, E2E_CP
    if case == "A":
        users = [dict(doppler=product.userchan_doppler(0.002 + 0.003 * c / (N - 1), M, cp), rice_k=10.0,
                      los_doppler=product.userchan_doppler(0.001 * (c - 3.5) / 3.5, M, cp), los_phase=c * 0x1F3D5B79) for c in range(N)]
        return dict(log2_block=4, sinusoids=8, seed=SEED_A, users=users)
    users = [dict(doppler=product.userchan_doppler(0.02, M, cp) * (0.6 + 0.4 * c / (N - 1)), rice_k=0.0) for c in range(N)]
    return dict(log2_block=4, sinusoids=8, seed=SEED_B, users=users)


def through_the_channels(product, oracle, case):
    """tests/test_gpu_userchan.py::test_end_to_end's eight users (three rays, oscillator, timing, 30 dB of levels) with every user
    fading: multichanneltx tiles -> userchan -> synthesize -> chanemu (noise only) -> multichannelrx, and the oracle's receiver on the
    same samples.  Noise: 25 dB on the weakest user -- w = that user's nominal share of the power (levels; E|g|^2 = 1), a user channel
    is 1 / K of the band, so noise_std = rms sqrt(K w / 10^2.5 / 2) per component = 0.00365 rms."""
    torch = _torch()
    N, M, cp, taper, nf, plen = E2E_N, E2E_M, E2E_CP, E2E_TAPER, E2E_NF, E2E_PLEN
    K = 2 * N
    chans = [dict(taps=[(0, 1.0), (1 + c % 3, (0.25 - 0.15j) * np.exp(1j * c)), (4, (-0.10 + 0.15j) * np.exp(-2j * c))],
                  gain_db=float(base.LEVELS_DB[c]), cfo_step=product.userchan_cfo_step(base.CFO[c], M), delay=base.TIMING[c]) for c in range(N)]
    uc = product.userchan(channels=chans, fading=e2e_fading(product, case))
    tx = product.multichanneltx(N, M, cp, taper)
    iq, sent = uc.generate(tx, nf, plen, seed=base.TRAFFIC_SEED)      # QPSK / Hamming(12,8), gain 1 / N
    uc.close(); tx.close()
    iq = torch.cat([iq, torch.zeros(64 * K, dtype=torch.complex64, device="cuda")])
    rms = float(torch.view_as_real(iq).pow(2).sum().div(int(iq.numel())).sqrt())
    assert rms > 0
    weak = 10.0 ** (min(base.LEVELS_DB) / 10.0) / sum(10.0 ** (v / 10.0) for v in base.LEVELS_DB)
    nstd = rms * float(np.sqrt(K * weak / 10.0 ** 2.5 / 2.0))
    ce = product.chanemu(taps=[(0, 1.0)], noise_std=nstd, seed=2024)
    y = ce.execute(iq)
    ce.close()
    assert int(y.numel()) % (product.TILE * K) == 0
    rx = product.multichannelrx(N, M, cp, taper, max_payload_len=plen)
    rx.Execute(y); rx.Flush()
    gpu = list(rx.frames)
    rx.close()
    ora = oracle.MultiChannelRx(N, M, cp, taper)
    ora.execute(np.ascontiguousarray(y.cpu().numpy()))
    return gpu, list(ora.frames), sent, nstd, rms


def test_end_to_end_rician(product, oracle):
    """Case A, fading seed 1.  Chosen on the CPU: the oracle's FlexFrameGen (three frames of 96 bytes a user) -> the float64 model with
    the integers the library's self-test reports -> Channelizer.synthesize and the bank's oscillator -> the same noise ->
    MultiChannelRx, for the fading seeds 1 .. 8: every frame was found for every seed, and all 24 were valid for every seed but 6
    (21: user 5 lost all three).  All 24 frames valid on both sides with the bytes sent; framesyms held to the 1e-3 bar of
    tests/test_gpu_userchan.py and recorded (profiles/userchan_fading_parity.json)."""
    from test_gpu_parity import match_frames, relerr, relerr_elem
    gpu, ora, sent, nstd, rms = through_the_channels(product, oracle, "A")
    n = E2E_N * E2E_NF
    for side, frames in (("gpu", gpu), ("oracle", ora)):
        assert len(frames) == n, (side, len(frames))
        seen = set()
        for f in frames:
            assert f.header_valid and f.payload_valid, (side, f)
            pid = (f.header[0] << 8) | f.header[1]
            assert sent[f.channel][pid] == (bytes(f.header), bytes(f.payload)), (side, f.channel, pid)
            seen.add((f.channel, pid))
        assert len(seen) == n
    w = we = 0.0
    for fg, fo in match_frames(gpu, ora):
        assert bytes(fg.header) == bytes(fo.header) and bytes(fg.payload) == bytes(fo.payload)
        assert len(fg.framesyms) == len(fo.framesyms) > 0
        w, we = max(w, relerr(fg.framesyms, fo.framesyms)), max(we, relerr_elem(fg.framesyms, fo.framesyms))
    PARITY["rician_seed%d" % SEED_A] = {"max_norm": w, "element_wise": we, "noise_std": nstd, "rms": rms}
    print("userchan_fading_parity rician: framesyms max-norm %.3e element-wise %.3e" % (w, we))
    assert w <= 1e-3, w


def test_end_to_end_rayleigh_contract(product, oracle):
    """Case B, fading seed 4.  The same rehearsal for seeds 1 .. 8 at K = 0 and 0.012 .. 0.02 cycles per symbol: every frame found for
    every seed; valid of 24: 11, 14, 13, 15, 15, 8, 11, 11 -- seed 4 leaves the case a mixed one with room on both sides.  Both
    receivers find all 24 frames, agree on every frame's flags and on the bytes where valid; the oracle flags at least one frame invalid
    and at least 12 valid."""
    from test_gpu_parity import match_frames
    gpu, ora, sent, _, _ = through_the_channels(product, oracle, "B")
    n = E2E_N * E2E_NF
    assert len(gpu) == n and len(ora) == n, (len(gpu), len(ora))
    both = 0
    for fg, fo in match_frames(gpu, ora):
        assert (fg.header_valid, fg.payload_valid) == (fo.header_valid, fo.payload_valid), (fg.channel, fg.header, fo.header)
        if fo.header_valid:
            assert bytes(fg.header) == bytes(fo.header)
        if fo.header_valid and fo.payload_valid:
            assert bytes(fg.payload) == bytes(fo.payload)
            pid = (fg.header[0] << 8) | fg.header[1]
            assert sent[fg.channel][pid] == (bytes(fg.header), bytes(fg.payload))
            both += 1
    n_ora = sum(1 for f in ora if f.header_valid and f.payload_valid)
    print("userchan fading contract case: %d valid on both sides, %d on the oracle's, %d / %d frames reported" % (both, n_ora, len(gpu), len(ora)))
    PARITY["rayleigh_seed%d_contract" % SEED_B] = {"valid_on_both": both, "oracle_valid": n_ora, "reported": len(ora)}
    assert 12 <= n_ora <= n - 1, n_ora
    assert both == n_ora


def test_zz_print_userchan_fading_deviations():
    """(last of this file: the figures measured above as one JSON line each -- profiles/userchan_fading_model.json and
    profiles/userchan_fading_parity.json are such records; USERCHAN_FADING_OUT / USERCHAN_FADING_PARITY_OUT name files to write them
    to as well)"""
    for tag, rec, env in (("userchan_fading_model", RATIOS, "USERCHAN_FADING_OUT"), ("userchan_fading_parity", PARITY, "USERCHAN_FADING_PARITY_OUT")):
        line = json.dumps(rec, sort_keys=True)
        print(tag + " " + line)
        path = os.environ.get(env)
        if path:
            with open(path, "w") as f:
                f.write(line + "\n")
