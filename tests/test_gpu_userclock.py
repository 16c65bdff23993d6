"""Each user's own sample clock and fractional timing on the GPU (mcrx_hip_userclock_*) against the float64 model
of tests/userclock_model.py fed with the library's own table and integers -- the stage alone (resample) and the whole operator (apply)
-- against handles without a clock, against itself cut into pieces, spans and channel shards, far out on the block axis, on a tone,
and end to end: multichanneltx tiles -> userchan with eight users' own clocks -> synthesize -> chanemu (noise) -> multichannelrx, with
the oracle's receiver on the same samples.

Bounds, per component and per channel.  The stage, userclock_model.z_bound: with X = max |x|, H = the largest sum_j |h_j| of the blocks
computed and Dw = the largest sum_j |W[r+1][j] - W[r][j]| of the table, |got - z| <= (33 H + Dw) 2^-24 X -- the 32 fused multiply-adds
round 32 partial sums of at most H X, the coefficient's fused multiply-add rounds each h_j once (H X 2^-24 in the sum), and the rows'
difference is rounded to fp32 before it is scaled by f < 1.  apply(): the operator's own bound on z in place of x (userchan_model.bound
or userchan_fading_model.bound, with max |z| <= H X) plus that error of z through the rays: gain sum_i |a_i| max|G_i| (33 H + Dw) 2^-24 X."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import test_gpu_userchan as base
import test_gpu_userchan_fading as fbase
import userchan_fading_model as fmodel
import userchan_model as model
import userclock_model as kmodel
from test_userclock import SET_BAD, library_table

pytestmark = pytest.mark.gpu

RATIOS, PARITY = {}, {}
_torch, samples, device_tiles, host_channels, bits = base._torch, base.samples, base.device_tiles, base.host_channels, fbase.bits
KINDS = [dict(delay=16.37, ppm=0.0), dict(delay=20.0, ppm=20.0), None, dict(delay=33.5, ppm=-20.0), dict(delay=17.999, ppm=900.0),
         dict(delay=40.001, ppm=-900.0), dict(delay=15.0, ppm=0.0), dict(delay=63.75, ppm=0.0)]


def clocks(C_, origin=0, max_delay=64, span_blocks=0, shift=0):
    """every channel its own kind of clock, cycling through KINDS (static fractions, +-20 ppm, +-900 ppm, the two ends of the range, and a
    user without a clock), all with the same origin"""
    users = [KINDS[(c + shift) % len(KINDS)] for c in range(C_)]
    return dict(max_delay=max_delay, span_blocks=span_blocks, users=[None if u is None else dict(u, origin=origin) for u in users])


def integers_of(uc):
    """per channel None or the integers the handle was given"""
    return [dict(delay_fp=int(u.delay_fp), sco=int(u.sco), origin=int(u.origin)) if u.enabled else None for u in uc._clock[1]]


def check_stage(product, C_, clock, x, first, lead, tag):
    """resample() against the model, channel by channel; returns the output as channels"""
    W32 = library_table(product)
    uc = product.userchan(channels=[dict(taps=[(0, 1.0)])] * C_, clock=clock)
    assert uc.clock_on() and uc.clock_lead_blocks == (clock["max_delay"] + 16 + 7) // 8 * 8 <= lead
    users = integers_of(uc)
    got = host_channels(uc.resample(device_tiles(x), first, x.shape[1] - lead, lead), C_)
    uc.close()
    w = 0.0
    for c in range(C_):
        want, hsum, _, _ = kmodel.z_channel(x[c], users[c], W32, first, lead, 0)
        if users[c] is None:
            assert got[c].tobytes() == x[c, lead:].tobytes(), (tag, c)             # z = x, bit for bit
            continue
        d = got[c].astype(np.complex128) - want
        dev, b = float(max(np.abs(d.real).max(), np.abs(d.imag).max())), kmodel.z_bound(W32, hsum, x[c])
        assert dev <= b, (tag, c, dev, b)
        w = max(w, dev / b)
    RATIOS[tag] = w
    print("userclock %s: worst |got - model| over its channel's bound %.3f" % (tag, w))
    return got


def check_apply(product, chans, fade, clock, x, first, lead, tag):
    """apply() of a clocked handle against the model: z in float64, then the operator's model on z"""
    W32 = library_table(product)
    uc = product.userchan(channels=chans, fading=fade, clock=clock)
    lz = model.lead_of(chans)
    D = max(d for ch in chans for d, _ in model.rays_of(ch))
    assert uc.clock_on() and uc.lead_blocks == (D + clock["max_delay"] + 16 + 7) // 8 * 8 <= lead
    users = integers_of(uc)
    tabs = fbase.tables_of(product, uc, chans) if fade else [None] * len(chans)
    got = host_channels(uc.apply(device_tiles(x), first, x.shape[1] - lead, lead), len(chans))
    uc.close()
    w = 0.0
    for c, ch in enumerate(chans):
        Dc = max(d for d, _ in model.rays_of(ch))
        z, hsum, _, _ = kmodel.z_channel(x[c], users[c], W32, first, lead, Dc)     # z of the blocks this channel's rays read ...
        z = np.concatenate([np.zeros(lz - Dc, np.complex128), z])                   # ... with the handle's lead in front
        rays = model.rays_of(ch)
        if fade:
            want, peaks = fmodel.apply_channel(z, ch, tabs[c], fade["log2_block"], first, lz)
            b = fmodel.bound(ch, tabs[c], peaks, fade["sinusoids"], z)
        else:
            want, peaks, b = model.apply_channel(z, ch, first, lz), [1.0] * len(rays), model.bound(ch, z)
        if users[c] is not None:
            b += model.gain_of(ch) * sum(abs(a) * pk for (_, a), pk in zip(rays, peaks)) * kmodel.z_bound(W32, hsum, x[c])
        d = got[c].astype(np.complex128) - want
        dev = float(max(np.abs(d.real).max(), np.abs(d.imag).max()))
        assert dev <= b, (tag, c, dev, b)
        w = max(w, dev / b)
    RATIOS[tag] = w
    print("userclock %s: worst |got - model| over its channel's bound %.3f" % (tag, w))
    return got


# ---------------------------------------------------------------------------------------------- 1. the stage alone
@pytest.mark.parametrize("C_", [1, 3, 8, 64])
def test_stage_against_the_model(product, C_):
    """256 blocks: two workgroup columns; 64 channels: four workgroup rows of 16 channels; 3: a ragged wave"""
    lead, nb = 80, 256
    x = samples(C_, lead + nb)
    got = check_stage(product, C_, clocks(C_, origin=8 * 4321 + 3, shift=C_ % 3), x, 8 * 4321, lead, "stage_C%d" % C_)
    assert float(np.abs(got).max()) > 1.0
    # ... and it is not the stream a sample further on
    assert float(np.abs(got[0, 1:] - got[0, :-1]).max()) > 0.1


# ---------------------------------------------------------------------------------------------- 2. the whole operator
@pytest.mark.parametrize("fade", [False, True], ids=["static", "fading"])
@pytest.mark.parametrize("rot", [True, False], ids=["rot", "norot"])
@pytest.mark.parametrize("C_", [1, 3, 8, 64])
def test_apply_against_the_model(product, C_, rot, fade):
    """tests/test_gpu_userchan.py's seeded table (1 .. 4 rays, delays up to 255, 30 dB of levels) behind every user's own clock"""
    chans = fbase.table(C_, rot)
    lead, nb = 256 + 80, 128
    x = samples(C_, lead + nb)
    f = fbase.fading(chans, 4, 8) if fade else None
    check_apply(product, chans, f, clocks(C_, origin=8 * 1234 - 5), x, 8 * 1234, lead,
                "apply_C%d_%s_%s" % (C_, "rot" if rot else "norot", "fading" if fade else "static"))


# ---------------------------------------------------------------------------------------------- 3. a crossing
@pytest.mark.parametrize("name,delay,ppm", [("up", 16.9, 900.0), ("down", 17.1, -900.0)])
def test_a_crossing(product, name, delay, ppm):
    """tau passes 17 samples 111.1 blocks behind the origin (block 3): mu wraps and n steps at block 115, inside the granule of blocks
    112 .. 119 and inside one call; within the bound, and the same bits whether or not a call begins or ends at that granule"""
    torch = _torch()
    C_, lead, nb = 3, 40, 256
    clock = dict(max_delay=17, users=[dict(delay=delay, ppm=ppm, origin=3)] * C_)
    x = samples(C_, lead + nb)
    W32 = library_table(product)
    user = kmodel.user_of(delay, ppm, 3)
    ns = [kmodel.tau_fp(user, b) >> 32 for b in range(nb)]
    assert set(ns) == {16, 17} and ns[114] != ns[115] and ns[0] == ns[114] and ns[115] == ns[255]
    got = check_stage(product, C_, clock, x, 0, lead, "crossing_" + name)
    uc = product.userchan(channels=[dict(taps=[(0, 1.0), (5, 0.5j)], cfo_step=12345)] * C_, clock=clock)
    assert uc.clock_lead_blocks == 40 and uc.lead_blocks == 40
    d_x = device_tiles(x)
    for fn, ld in ((uc.resample, 40), (uc.apply, 40)):
        one = fn(d_x, 0, nb, ld).clone()
        for cuts in ((112, 144), (120, 136), (64, 192), (112, 8, 136)):
            out = torch.full((nb * C_,), float("nan"), dtype=torch.complex64, device="cuda")
            pos = 0
            for n in cuts:
                fn(d_x[pos * C_:], pos, n, ld, out=out[pos * C_:])
                pos += n
            assert pos == nb and torch.equal(bits(out), bits(one)), cuts
    uc.close()
    assert float(np.abs(got).max()) > 1.0


# ---------------------------------------------------------------------------------------------- 4. identity
def test_users_without_a_clock_equal_a_handle_without_one(product):
    torch = _torch()
    C_, nb = 8, 128
    for rot in (True, False):
        chans = fbase.table(C_, rot)
        clock = clocks(C_)
        plain = product.userchan(channels=chans)
        lead0 = plain.lead_blocks
        uc = product.userchan(channels=chans, clock=clock)
        lead = uc.lead_blocks
        assert not plain.clock_on() and plain.clock_lead_blocks == 0 and lead == (255 + 64 + 16 + 7) // 8 * 8 and lead0 == 256
        d_x = device_tiles(samples(C_, lead + nb))
        ref = plain.apply(d_x[(lead - lead0) * C_:], 8 * 77, nb).clone()
        y = uc.apply(d_x, 8 * 77, nb).clone()
        yc, rc = y.view(-1, C_, 8), ref.view(-1, C_, 8)
        for c in range(C_):
            same = torch.equal(bits(yc[:, c].contiguous()), bits(rc[:, c].contiguous()))
            assert same == (clock["users"][c] is None), (rot, c)
        # the clock off after it was on: the parent's lead and the parent's bits; on again: the clocked bits
        uc.set_clock(None)
        assert not uc.clock_on() and uc.lead_blocks == lead0 and uc.clock_lead_blocks == 0
        assert torch.equal(bits(uc.apply(d_x[(lead - lead0) * C_:], 8 * 77, nb)), bits(ref)), rot
        with pytest.raises(ValueError):
            uc.resample(d_x, 8 * 77, nb, lead)
        uc.set_clock(clock)
        assert uc.clock_on() and torch.equal(bits(uc.apply(d_x, 8 * 77, nb)), bits(y))
        uc.close()
        late = product.userchan(channels=chans)                               # a handle made without a clock and given one later
        late.set_clock(clock)
        assert torch.equal(bits(late.apply(d_x, 8 * 77, nb)), bits(y))
        late.close(); plain.close()


def test_a_whole_sample_delay_is_the_parents_delay(product):
    """delay = n and sco = 0: W's row 0 is the unit vector of tap 15, so z[b] = x[b - n] on finite input, the sign of a zero aside -- the
    parent handle with n added to the user's rays (torch.equal compares values: -0 == +0)"""
    torch = _torch()
    C_, nb = 3, 128
    ns = [15, 22, 64]
    chans = [dict(taps=[(0, 1.0), (1 + c, 0.5j), (9, -0.25)], gain_db=-3.0 * c, cfo_step=1000 + c) for c in range(C_)]
    moved = [dict(ch, delay=n) for ch, n in zip(chans, ns)]
    uc = product.userchan(channels=chans, clock=dict(max_delay=64, users=[dict(delay=float(n), origin=99) for n in ns]))
    plain = product.userchan(channels=moved)
    lead = uc.lead_blocks
    assert lead == 96 and plain.lead_blocks == 80
    d_x = device_tiles(samples(C_, lead + nb))
    y, ref = uc.apply(d_x, 8 * 5, nb), plain.apply(d_x[(lead - 80) * C_:], 8 * 5, nb)
    assert torch.equal(y, ref) and float(y.abs().max()) > 1.0
    z = host_channels(uc.resample(d_x, 8 * 5, nb, lead), C_)
    x = host_channels(d_x, C_)
    for c, n in enumerate(ns):
        assert np.array_equal(z[c], x[c, lead - n:lead - n + nb]), c
    uc.close(); plain.close()


# ---------------------------------------------------------------------------------------------- 5. cut anywhere
@pytest.mark.parametrize("fade", [False, True], ids=["static", "fading"])
def test_cut_anywhere(product, fade):
    """pieces of 8, 64, 8 and 176 blocks with two sufficient leads, spans of 8 and of 64 blocks, and the default span: the one-call bits"""
    torch = _torch()
    C_, total, extra = 3, 256, 16
    chans = fbase.table(C_)
    f = fbase.fading(chans, 4, 8, mix=False) if fade else None
    first = 8 * 999
    outs = []
    for span in (0, 8, 64):
        uc = product.userchan(channels=chans, fading=f, clock=clocks(C_, origin=first + 100, span_blocks=span, shift=3))
        lead = uc.lead_blocks
        LL = lead + extra
        d_x = device_tiles(samples(C_, LL + total))
        one = uc.apply(d_x[extra * C_:], first, total).clone()
        outs.append(one)
        assert float(one.abs().max()) > 1.0
        for fn, ld in ((uc.apply, lead), (uc.resample, uc.clock_lead_blocks)):
            whole = fn(d_x[(LL - ld) * C_:], first, total, ld).clone()
            for l in (ld, ld + extra):
                out = torch.full((total * C_ + 8,), float("nan"), dtype=torch.complex64, device="cuda")
                pos = 0
                for n in (8, 64, 8, 176):
                    y = fn(d_x[(LL + pos - l) * C_:], first + pos, n, lead_blocks=l, out=out[pos * C_:])
                    assert int(y.numel()) == n * C_
                    pos += n
                assert pos == total and torch.equal(bits(out[:total * C_]), bits(whole)), (span, l)
                assert bool(torch.isnan(out[total * C_:].real).all())              # nothing stored behind it
        uc.close()
    assert torch.equal(bits(outs[1]), bits(outs[0])) and torch.equal(bits(outs[2]), bits(outs[0]))


def test_shards_keep_their_users_clocks(product):
    C_, nb = 8, 128
    chans = fbase.table(C_)
    fade = fbase.fading(chans, 4, 8)
    clock = clocks(C_, origin=8 * 55 - 1000)
    uc = product.userchan(channels=chans, fading=fade, clock=clock)
    lead = uc.lead_blocks
    x = samples(C_, lead + nb)
    first = 8 * 55
    full = host_channels(uc.apply(device_tiles(x), first, nb), C_)
    for c0, cnt in ((0, 3), (3, 5)):
        sh = uc.shard(c0, cnt)
        assert sh.num_channels == cnt and sh.fading_on() and sh.clock_on() and sh._clock[0].max_delay == 64
        assert integers_of(sh) == integers_of(uc)[c0:c0 + cnt]
        part = host_channels(sh.apply(device_tiles(x[c0:c0 + cnt]), first, nb, lead_blocks=lead), cnt)
        assert part.tobytes() == full[c0:c0 + cnt].tobytes(), (c0, cnt)
        sh.close()
    uc.close()


# ---------------------------------------------------------------------------------------------- 6. far positions
FAR = [("2^40", 2 ** 40, 2 ** 40 - 7), ("minus_256", -256, -131), ("across_2^32", 2 ** 32 - 64, 2 ** 32 + 5)]


@pytest.mark.parametrize("name,first,origin", FAR, ids=[f[0] for f in FAR])
def test_far_positions(product, name, first, origin):
    C_, nb = 3, 128
    chans = fbase.table(C_)
    lead = 256 + 80
    x = samples(C_, lead + nb)
    clock = clocks(C_, origin=origin, shift=3)                       # -20 ppm, +900 ppm and -900 ppm
    got = check_apply(product, chans, fbase.fading(chans, 4, 8, mix=False), clock, x, first, lead, "far_" + name)
    z = check_stage(product, C_, clock, x[:, 256:], first, 80, "far_stage_" + name)
    # ... and it is not the stream with its origin 1024 blocks further on (0.92 samples at 900 ppm)
    uc = product.userchan(channels=[dict(taps=[(0, 1.0)])] * C_, clock=clocks(C_, origin=origin + 1024, shift=3))
    other = host_channels(uc.resample(device_tiles(x[:, 256:]), first, nb, 80), C_)
    uc.close()
    assert float(np.abs(other[1] - z[1]).max()) > 0.1 and float(np.abs(got).max()) > 0.5


# ---------------------------------------------------------------------------------------------- 7. a tone
@pytest.mark.parametrize("ppm", [0.0, 20.0, -900.0])
def test_a_tone_is_delayed_by_tau(product, ppm):
    """the physical meaning of the definition, once on the device: e^{2 pi i 0.3 b} comes out as e^{2 pi i 0.3 (b - tau(b))} within
    10^(-54 / 20), the interpolator's figure on |f| <= 0.44"""
    C_, lead, nb, first = 3, 80, 256, 8 * 100
    b = np.arange(first - lead, first + nb, dtype=np.float64)
    x = np.tile(np.exp(2j * np.pi * 0.3 * b).astype(np.complex64), (C_, 1))
    delays = [16.37, 33.5, 47.83]
    uc = product.userchan(channels=[dict(taps=[(0, 1.0)])] * C_, clock=dict(max_delay=64, users=[dict(delay=d, ppm=ppm, origin=first - 50) for d in delays]))
    users = integers_of(uc)
    got = host_channels(uc.resample(device_tiles(x), first, nb, lead), C_)
    uc.close()
    w = 0.0
    for c in range(C_):
        tau = np.array([kmodel.tau_fp(users[c], first + m) for m in range(nb)], dtype=np.float64) * 2.0 ** -32
        want = np.exp(2j * np.pi * 0.3 * (np.arange(first, first + nb) - tau))
        w = max(w, float(np.abs(got[c] - want).max()))
    RATIOS["tone_%g_ppm_db" % ppm] = 20.0 * np.log10(w)
    print("userclock tone at %g ppm: worst error %.2f dB" % (ppm, 20.0 * np.log10(w)))
    assert w <= 10.0 ** (-54.0 / 20.0), w


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_a_call_that_leaves_the_range_is_refused(product):
    torch = _torch()
    L, EINVAL, OK = product.lib(), product.MCRX_EINVAL, product.MCRX_OK
    C_, nb = 3, 1024
    chans = [dict(taps=[(0, 1.0), (9, 0.5j)])] * C_
    # user 1 drifts 0.92 samples in 1024 blocks: from 16.5 through 17, beyond max_delay = 16, at block 556 (and below 16 never)
    uc = product.userchan(channels=chans, clock=dict(max_delay=16, users=[None, dict(delay=16.5, ppm=900.0), dict(delay=16.5)]))
    lead = uc.lead_blocks
    assert lead == 48 and uc.clock_lead_blocks == 32
    d_x = device_tiles(samples(C_, lead + nb))
    out = torch.full((nb * C_,), float("nan"), dtype=torch.complex64, device="cuda")

    def call(fn, first, count, ld):
        return fn(uc._h, C.c_void_p(d_x.data_ptr()), first, count, ld, C.c_void_p(out.data_ptr()), None)
    for fn, ld in ((L.mcrx_hip_userchan_apply_tiles, lead), (L.mcrx_hip_userclock_apply_tiles, 32)):
        assert call(fn, 0, 552, ld) == OK
        torch.cuda.synchronize()
        assert not bool(torch.isnan(out[:552 * C_].real).any())
        out.fill_(float("nan"))
        assert call(fn, 0, 560, ld) == EINVAL                                  # block 556 has n = 17
        assert b"channel 1" in L.mcrx_hip_userchan_last_error()
        assert call(fn, 560, 8, ld) == EINVAL and call(fn, 8 * 10 ** 9, 8, ld) == EINVAL
        assert call(fn, -(1 << 62), 8, ld) == EINVAL                           # 2^38 * 2^62 leaves int64 ... and says so
        assert call(fn, 0, 64, ld - 8) == EINVAL                               # a lead below the handle's
        torch.cuda.synchronize()
        assert bool(torch.isnan(out.real).all())                               # nothing written
    # the lower end of the range: this user's delay falls below 15 samples at block 1
    low = product.userchan(channels=chans, clock=dict(max_delay=16, users=[None, dict(delay=15.004, ppm=-900.0, origin=-4), None]))
    assert L.mcrx_hip_userclock_apply_tiles(low._h, C.c_void_p(d_x.data_ptr()), 0, 8, 32, C.c_void_p(out.data_ptr()), None) == EINVAL     # block 1: 14.9995
    assert L.mcrx_hip_userclock_apply_tiles(low._h, C.c_void_p(d_x.data_ptr()), -8, 8, 32, C.c_void_p(out.data_ptr()), None) == OK
    assert L.mcrx_hip_userchan_apply_tiles(low._h, C.c_void_p(d_x.data_ptr()), -8, 8, 48, C.c_void_p(out.data_ptr()), None) == OK
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        low.apply(d_x, 0, 8)
    low.close(); uc.close()


@pytest.mark.parametrize("what,spoil,block", SET_BAD, ids=[b[0] for b in SET_BAD])
def test_set_errors_leave_the_handle_as_it_was(product, what, spoil, block):
    torch = _torch()
    L_ = product.lib()
    chans = [dict(taps=[(0, 1.0), (9, 0.5j), (3, 0.25)], cfo_step=77)] * 2
    good = dict(max_delay=64, users=[dict(delay=16.25, ppm=20.0)] * 2)
    plain = product.userchan(channels=chans)
    clocked = product.userchan(channels=chans, clock=dict(max_delay=32, users=[dict(delay=20.5, ppm=-20.0)] * 2))
    lead = clocked.lead_blocks
    assert lead == 64
    d_x = device_tiles(samples(2, lead + 64))
    before = clocked.apply(d_x, 0, 64).clone()
    f, users = product.userchan_clock(2, **good)
    spoil(f, users[1])
    for uc in (plain, clocked):
        assert L_.mcrx_hip_userclock_set(uc._h, C.addressof(f), C.addressof(users)) == product.MCRX_EINVAL, what
        assert L_.mcrx_hip_userchan_last_error()
    assert L_.mcrx_hip_userclock_set(clocked._h, C.addressof(f), None) == product.MCRX_EINVAL
    assert not plain.clock_on() and clocked.clock_on() and plain.lead_blocks == 16 and clocked.lead_blocks == lead
    assert torch.equal(bits(clocked.apply(d_x, 0, 64)), bits(before))
    if what.startswith(("sco", "delay_fp")):         # a user without a clock is not looked at
        users[1].enabled = 0
        assert L_.mcrx_hip_userclock_set(plain._h, C.addressof(f), C.addressof(users)) == product.MCRX_OK and plain.clock_on()
    plain.close(); clocked.close()


# ---------------------------------------------------------------------------------------------- 9. end to end
E2E_N, E2E_M, E2E_CP, E2E_TAPER, E2E_NF, E2E_PLEN = 8, 64, 8, 4, 3, 96
E2E_DELAY = [20.0, 20.13, 20.5, 20.87, 21.25, 21.63, 22.37, 20.75]
E2E_PPM = [200.0, -200.0, 50.0, -100.0, 20.0, 150.0, -20.0, 35.0]
E2E_CFO = [0.45, -0.45, 0.3, -0.2, 0.05, 0.4, -0.35, 0.1]          # subcarrier spacings, each of its user's clock's sign


@pytest.mark.parametrize("name,snr_db", [("clean", None), ("weakest_at_20dB", 20.0)])
def test_end_to_end(product, oracle, name, snr_db):
    """tests/test_gpu_userchan.py::test_end_to_end's eight users (three rays, 30 dB of levels, an integer timing each) with every user on
    a clock of their own: a fraction of a sample each (20.5 among them: two integer timings equally good), +-20 .. +-200 ppm and an
    oscillator offset of the matching sign.  multichanneltx tiles -> userchan -> synthesize -> chanemu (noise only) -> multichannelrx, and
    the oracle's receiver on the same samples.  Noise: w = the weakest user's nominal share of the power, a user channel is 1 / K of the
    band, so noise_std = rms sqrt(K w / 10^(snr / 10) / 2) per component.  All 24 frames valid on both sides with the bytes sent;
    framesyms held to the 1e-3 bar of tests/test_gpu_userchan.py and recorded (profiles/userclock_parity.json)."""
    from test_gpu_parity import match_frames, relerr, relerr_elem
    torch = _torch()
    N, M, cp, taper, nf, plen = E2E_N, E2E_M, E2E_CP, E2E_TAPER, E2E_NF, E2E_PLEN
    K = 2 * N
    assert all((p > 0) == (f > 0) for p, f in zip(E2E_PPM, E2E_CFO))
    chans = [dict(taps=[(0, 1.0), (1 + c % 3, (0.25 - 0.15j) * np.exp(1j * c)), (4, (-0.10 + 0.15j) * np.exp(-2j * c))],
                  gain_db=float(base.LEVELS_DB[c]), cfo_step=product.userchan_cfo_step(E2E_CFO[c], M), delay=base.TIMING[c]) for c in range(N)]
    clock = dict(max_delay=64, users=[dict(delay=E2E_DELAY[c], ppm=E2E_PPM[c], origin=0) for c in range(N)])
    uc = product.userchan(channels=chans, clock=clock)
    tx = product.multichanneltx(N, M, cp, taper)
    iq, sent = uc.generate(tx, nf, plen, seed=base.TRAFFIC_SEED)      # QPSK / Hamming(12,8), gain 1 / N
    uc.close(); tx.close()
    iq = torch.cat([iq, torch.zeros(64 * K, dtype=torch.complex64, device="cuda")])           # (room behind the delayed users' last frames)
    rms = float(torch.view_as_real(iq).pow(2).sum().div(int(iq.numel())).sqrt())
    assert rms > 0
    nstd = 0.0
    if snr_db is not None:
        weak = 10.0 ** (min(base.LEVELS_DB) / 10.0) / sum(10.0 ** (v / 10.0) for v in base.LEVELS_DB)
        nstd = rms * float(np.sqrt(K * weak / 10.0 ** (snr_db / 10.0) / 2.0))
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
    n = N * nf
    for side, frames in (("gpu", gpu), ("oracle", list(ora.frames))):
        assert len(frames) == n, (side, len(frames))
        seen = set()
        for f in frames:
            assert f.header_valid and f.payload_valid, (side, f.channel)
            pid = (f.header[0] << 8) | f.header[1]
            assert sent[f.channel][pid] == (bytes(f.header), bytes(f.payload)), (side, f.channel, pid)
            seen.add((f.channel, pid))
        assert len(seen) == n
    w = we = 0.0
    for fg, fo in match_frames(gpu, list(ora.frames)):
        assert bytes(fg.header) == bytes(fo.header) and bytes(fg.payload) == bytes(fo.payload)
        assert len(fg.framesyms) == len(fo.framesyms) > 0
        w, we = max(w, relerr(fg.framesyms, fo.framesyms)), max(we, relerr_elem(fg.framesyms, fo.framesyms))
    PARITY[name] = {"max_norm": w, "element_wise": we, "noise_std": nstd, "rms": rms}
    print("userclock_parity %s: framesyms max-norm %.3e element-wise %.3e" % (name, w, we))
    assert w <= 1e-3, w


def test_zz_print_userclock_deviations():
    """(last of this file: the figures measured above as one JSON line each -- profiles/userclock_model.json and
    profiles/userclock_parity.json are such records; USERCLOCK_OUT / USERCLOCK_PARITY_OUT name files to write them to as well)"""
    for tag, rec, env in (("userclock_model", RATIOS, "USERCLOCK_OUT"), ("userclock_parity", PARITY, "USERCLOCK_PARITY_OUT")):
        line = json.dumps(rec, sort_keys=True)
        print(tag + " " + line)
        path = os.environ.get(env)
        if path:
            with open(path, "w") as f:
                f.write(line + "\n")
