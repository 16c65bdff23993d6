"""Fading rays of the channel emulator on the GPU (mcrx_hip_chanfade_*) against the float64 model of
tests/chanemu_fading_model.py fed with the integers the library reports (so integer parity is exact), against itself cut into pieces and
into spans of the gain table, with fading switched off and on in mid-stream, and end to end between multichanneltx and multichannelrx /
the oracle.

Bound, per component, with S sinusoids, Gmax = max_i (c_los_i + S c_sc_i) >= |g_i(n)|:

    |got - model| <= { [(2T + 8) 2^-24 + 3e-7] Gmax + E_g } * gain * sum|a_i| * max|x|,   E_g = Gmax (3e-7 + 2^-24) + (S + 5) 2^-24 Gmax

The first term is tap_bound of tests/test_gpu_chanemu.py with every a_i scaled by a gain of at most Gmax.  E_g is the error of the fp32
g_i(n) a_i relative to |a_i|: sincos_u32's stated error on every term of G (their coefficients sum to Gmax) and the rounding of the
line-of-sight product; S + 1 roundings of the sum (one product, S fused multiply-adds), 2 of the interpolation (the difference of
the rows and one fused multiply-add), 2 of the product g a (cmul_fx: a product and a fused multiply-add per component), each at most
2^-24 of a value bounded by Gmax.  The implementation's count of roundings is this one.  Noise adds 1e-5 * noise_std as in the static tests."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import chanemu_fading_model as fmodel
import test_gpu_chanemu as base
import tx_sc16_model as q16
from test_chanemu_fading import BAD, good_fading, selftest

pytestmark = pytest.mark.gpu

TAPS_A, TAPS_B, N_LONG = base.TAPS_A, base.TAPS_B, base.N_LONG
CFO_STEP, PHASE0, GAIN, NOISE_STD, SEED, SENTINEL = base.CFO_STEP, base.PHASE0, base.GAIN, base.NOISE_STD, base.SEED, base.SENTINEL
FADE_A = dict(doppler=[1e-4, 3e-5, 1e-5], rice_k=[8.0, 0.0, 1.0], los_doppler=[5e-5, 0.0, -1e-5], los_phase=[0x12345678, 0, 0x80000001],
              sinusoids=8, log2_block=10, seed=11)
FADE_B = dict(doppler=[5e-3, 1e-3, 7e-3, 0.0, 2e-3, 5e-3, 1e-4, 3e-3], rice_k=[0.0, 2.0, 0.0, 5.0, 0.0, 1.0, 0.0, 0.5],
              los_doppler=[0.0, -4e-3, 0.0, 7e-3, 0.0, 1e-3, 0.0, -1e-4], los_phase=0x9E3779B9, sinusoids=16, log2_block=4, seed=12)
FADE_C = dict(doppler=0.05, rice_k=0.0, sinusoids=16, log2_block=1, seed=13)
FADE_4 = dict(doppler=[5e-3, 1e-3, 7e-3], rice_k=[0.0, 2.0, 0.5], los_doppler=[0.0, -4e-3, 1e-3], sinusoids=8, log2_block=4, seed=14)


def tables(product, num_taps, fading):
    f = product.chanemu_fading(num_taps, **fading)
    return [selftest(product, f, i) for i in range(num_taps)]


def fade_bound(taps, tabs, S, gain, x):
    T = len(taps)
    gmax = max(c[0] + S * c[1] for _, _, c in tabs)
    e_g = gmax * (3e-7 + 2.0 ** -24) + (S + 5) * 2.0 ** -24 * gmax
    return (((2 * T + 8) * 2.0 ** -24 + 3e-7) * gmax + e_g) * gain * sum(abs(complex(np.complex64(a))) for _, a in taps) * float(np.abs(x).max())


def bits(t):
    import torch
    return torch.view_as_real(t).view(torch.int32) if t.dtype == torch.complex64 else t


# ---------------------------------------------------------------------------------------------- 1. against the model
CASES = [("T3_L10", TAPS_A, FADE_A), ("T8_L4", TAPS_B, FADE_B), ("T1_L1", [(0, 1.0)], FADE_C)]


@pytest.mark.parametrize("name,taps,fading", CASES, ids=[c[0] for c in CASES])
def test_fading_against_the_model(product, name, taps, fading):
    x, d_x = base.samples(N_LONG)
    ce = product.chanemu(taps=taps, cfo_step=CFO_STEP, phase0=PHASE0, gain=GAIN, fading=fading)
    assert ce.fading_on()
    got = base.host(ce.execute(d_x))
    assert ce.position() == N_LONG
    ce.close()
    tabs = tables(product, len(taps), fading)
    want = fmodel.apply(x, taps, tabs, fading["log2_block"], CFO_STEP, PHASE0, GAIN)
    bound, w = fade_bound(taps, tabs, fading["sinusoids"], GAIN, x), base.worst(got, want)
    print("chanemu fading case %s: worst |got - model| %.3e, bound %.3e (%.2f of it)" % (name, w, bound, w / bound))
    assert float(np.abs(want).max()) > 1.0
    assert w <= bound, (w, bound)
    # ... and it is not the static channel
    assert base.worst(got, base.model.apply(x, taps, CFO_STEP, PHASE0, GAIN)) > 0.1


def test_gain_table_against_the_model(product):
    """the gain kernel on its own, at the start, far out and across the wrap of the row index.  Per component
    |got - G| <= Gmax (3e-7 + 2^-24) + (S + 1) 2^-24 Gmax: sincos_u32 on every term, the line-of-sight product, S + 1 roundings of the sum"""
    L = product.lib()
    ce = product.chanemu(taps=TAPS_B, fading=FADE_B)
    tabs = tables(product, 8, FADE_B)
    S, Lb = FADE_B["sinusoids"], FADE_B["log2_block"]
    for first in (0, 2 ** 30 + 5, 2 ** (64 - Lb) - 300):
        got = base.host(ce.gains(first, 1000))
        rows = (np.uint64(first) + np.arange(1000, dtype=np.uint64)) & np.uint64((1 << (64 - Lb)) - 1)
        for i, t in enumerate(tabs):
            bound = (t[2][0] + S * t[2][1]) * (3e-7 + (S + 2) * 2.0 ** -24)
            w = base.worst(got[:, i], fmodel.grid(t, rows, Lb))
            assert w <= bound, (first, i, w, bound)
    ce.set_fading(None)
    d = base._torch().zeros(64, dtype=base._torch().complex64, device="cuda")
    assert L.mcrx_hip_chanfade_gains(ce._h, 0, 8, C.c_void_p(d.data_ptr()), None) == product.MCRX_EINVAL       # fading off
    ce.close()


# ---------------------------------------------------------------------------------------------- 2. cut anywhere, spans anywhere
@pytest.mark.parametrize("fmt", ["cf32", "sc16"])
def test_cut_anywhere(product, fmt):
    """one shot with a table of 4 rows at L = 4 (spans of at most 48 samples) == one shot with the default table == either cut in pieces"""
    torch = base._torch()
    x, d_x = base.samples(N_LONG)
    sc16 = fmt == "sc16"
    ones = []
    for rows in (4, 0):
        cfg = dict(taps=TAPS_A, cfo_step=CFO_STEP, phase0=PHASE0, gain=GAIN, noise_std=NOISE_STD, seed=SEED, output_format=fmt,
                   fading=dict(FADE_4, table_rows=rows))
        ce = product.chanemu(**cfg)
        one = ce.execute(d_x).clone()
        clips = ce.clipped(reset=True)
        assert (clips > 100) if sc16 else (clips == 0)
        ones.append((one, clips))
        ce.reset()
        if sc16:
            buf = torch.full((N_LONG + 64, 2), SENTINEL, dtype=torch.int16, device="cuda")
        else:
            buf = torch.full((N_LONG + 64,), float("nan"), dtype=torch.complex64, device="cuda")
        for a, b in base.pieces(N_LONG):
            y = ce.execute(d_x[a:b], out=buf[a:])
            assert int(y.shape[0]) == b - a and ce.position() == b
        torch.cuda.synchronize()
        assert torch.equal(bits(buf[:N_LONG]), bits(one))               # the stream cut in pieces is the stream, word for word
        if sc16:
            assert bool((buf[N_LONG:] == SENTINEL).all())               # nothing stored behind it
        else:
            assert bool(torch.isnan(buf[N_LONG:].real).all())
        assert ce.clipped() == clips
        ce.close()
    assert torch.equal(bits(ones[0][0]), bits(ones[1][0])) and ones[0][1] == ones[1][1]       # spans are invisible


def test_the_gain_table_grows_and_is_reused(product):
    """L = 1, the default table, from an odd position: 130 samples in the first allocation (67 rows), 5 000 that force the table to grow,
    130 again in the grown one -- each call the bits of a fresh handle's"""
    torch = base._torch()
    x, d_x = base.samples(5000)
    cfg = dict(taps=[(0, 1.0), (3, 0.5j)], cfo_step=CFO_STEP, phase0=PHASE0, gain=GAIN, noise_std=NOISE_STD, seed=SEED, fading=dict(FADE_C, table_rows=0))
    ce = product.chanemu(**cfg)
    for n in (130, 5000, 130):
        fresh = product.chanemu(**cfg)
        ce.reset(at=1001); fresh.reset(at=1001)
        got, want = ce.execute(d_x[:n]), fresh.execute(d_x[:n])
        assert int(got.shape[0]) == n and ce.position() == 1001 + n
        assert torch.equal(bits(got), bits(want)), n
        fresh.close()
    assert float(got.abs().max()) > 0.0
    ce.close()


# ---------------------------------------------------------------------------------------------- 3. far positions
FAR =[("2^40 + 3", 2 ** 40 + 3), ("across 2^33", 2 ** 33 - 1000), ("across 2^64", 2 ** 64 - 5000)]


@pytest.mark.parametrize("name,p", FAR, ids=["2p40", "2p33", "wrap"])
def test_far_positions(product, name, p):
    torch = base._torch()
    x, d_x = base.samples(8000, seed=9)
    cfg = dict(taps=TAPS_A, cfo_step=CFO_STEP, phase0=PHASE0, gain=GAIN, noise_std=NOISE_STD, seed=SEED, fading=FADE_A)
    tabs = tables(product, 3, FADE_A)
    bound = fade_bound(TAPS_A, tabs, FADE_A["sinusoids"], GAIN, x) + 1e-5 * NOISE_STD
    ce = product.chanemu(**cfg)
    ce.execute(d_x[:1000])                                        # (history that the reset must drop)
    ce.reset(at=p)
    one = ce.execute(d_x).clone()
    assert ce.position() == (p + 8000) % 2 ** 64
    want = fmodel.apply(x, TAPS_A, tabs, 10, CFO_STEP, PHASE0, GAIN, NOISE_STD, SEED, start=p)
    w = base.worst(base.host(one), want)
    print("chanemu fading at %s: worst %.3e, bound %.3e" % (name, w, bound))
    assert w <= bound
    assert base.worst(base.host(one), fmodel.apply(x, TAPS_A, tabs, 10, CFO_STEP, PHASE0, GAIN, NOISE_STD, SEED, start=0)) > 0.1
    # cut there, with a table of two rows (a span never crosses a grid row): the same bits
    ce.set_fading(dict(FADE_A, table_rows=2))
    ce.reset(at=p)
    cut = torch.cat([ce.execute(d_x[:777]).clone(), ce.execute(d_x[777:4999]).clone(), ce.execute(d_x[4999:]).clone()])
    assert torch.equal(bits(cut), bits(one))
    ce.close()


# ---------------------------------------------------------------------------------------------- 4. sc16 is Q of cf32
def test_sc16_is_q_of_cf32(product):
    x, d_x = base.samples(N_LONG)
    cfg = dict(taps=TAPS_A, cfo_step=CFO_STEP, phase0=PHASE0, gain=0.4, noise_std=0.05, seed=SEED, fading=FADE_A)
    cf, sc = product.chanemu(**cfg), product.chanemu(output_format="sc16", **cfg)
    y, i = base.host(cf.execute(d_x)), base.host(sc.execute(d_x))
    want = q16.clipped_samples(y)
    assert 0 < want < 0.2 * len(y), want                          # some samples clip, most do not
    assert np.array_equal(i, q16.quantise_iq(y))
    assert cf.clipped() == 0 and sc.clipped() == want
    cf.close(); sc.close()


# ---------------------------------------------------------------------------------------------- 5. off means off
def test_off_means_off_and_set_in_mid_stream(product):
    torch = base._torch()
    x, d_x = base.samples(N_LONG)
    cfg = dict(taps=TAPS_A, cfo_step=CFO_STEP, phase0=PHASE0, gain=GAIN)
    a, b, c = 70001, 140001, N_LONG
    plain = product.chanemu(**cfg)
    assert not plain.fading_on()
    ref = plain.execute(d_x).clone()
    plain.close()
    ce = product.chanemu(fading=FADE_A, **cfg)
    on1 = ce.execute(d_x[:a]).clone()
    ce.set_fading(None)
    assert not ce.fading_on()
    off = ce.execute(d_x[a:b]).clone()
    assert torch.equal(bits(off), bits(ref[a:b]))                 # a handle that never had fading, on the same stream positions
    ce.set_fading(FADE_A)
    assert ce.fading_on()
    on2 = ce.execute(d_x[b:]).clone()
    ce.close()
    tabs = tables(product, 3, FADE_A)
    want = fmodel.apply(x, TAPS_A, tabs, 10, CFO_STEP, PHASE0, GAIN)
    bound = fade_bound(TAPS_A, tabs, FADE_A["sinusoids"], GAIN, x)
    assert base.worst(base.host(on1), want[:a]) <= bound and base.worst(base.host(on2), want[b:]) <= bound
    assert base.worst(base.host(off), want[a:b]) > 0.1
    # a handle made static and switched on later is the handle made with fading
    late = product.chanemu(**cfg)
    late.set_fading(FADE_A)
    assert torch.equal(bits(late.execute(d_x[:a])), bits(on1))
    late.close()


@pytest.mark.parametrize("what,spoil", BAD, ids=[b[0] for b in BAD])
def test_configuration_errors_on_a_handle(product, what, spoil):
    L = product.lib()
    ce = product.chanemu(taps=TAPS_A)
    f = good_fading(product)
    spoil(f)
    assert L.mcrx_hip_chanfade_set(ce._h, C.addressof(f)) == product.MCRX_EINVAL, what
    assert L.mcrx_hip_chanemu_last_error() and not ce.fading_on()
    ce.close()


def test_entries_beyond_num_taps_are_ignored(product):
    L = product.lib()
    ce = product.chanemu(taps=TAPS_A)
    f = good_fading(product)
    f.doppler[3], f.rice_k[7], f.los_doppler[5] = -1.0, float("nan"), float("inf")
    assert L.mcrx_hip_chanfade_set(ce._h, C.addressof(f)) == product.MCRX_OK and ce.fading_on()
    ce.close()


# ---------------------------------------------------------------------------------------------- 6. determinism
def test_determinism_and_independent_seeds(product):
    torch = base._torch()
    n = 2 ** 16 + 3
    x, d_x = base.samples(N_LONG)
    d_x = d_x[:n]
    zeros = torch.zeros(n, dtype=torch.complex64, device="cuda")
    cfg = dict(taps=TAPS_A, cfo_step=CFO_STEP, phase0=PHASE0, gain=GAIN)

    def run(inp, fseed, nstd, nseed):
        ce = product.chanemu(noise_std=nstd, seed=nseed, fading=dict(FADE_A, seed=fseed), **cfg)
        y = ce.execute(inp).clone()
        ce.close()
        return y
    a = run(d_x, 21, 0.0, 1)
    assert torch.equal(bits(a), bits(run(d_x, 21, 0.0, 1)))                        # the same fading seed: the same bits
    other = run(d_x, 22, 0.0, 1)
    assert int((a != other).sum()) > 0.99 * n                                      # another: another channel
    assert torch.equal(bits(a), bits(run(d_x, 21, 0.0, 2)))                        # noise off: the noise seed does not matter
    w = run(zeros, 21, NOISE_STD, 1)
    assert torch.equal(bits(w), bits(run(zeros, 22, NOISE_STD, 1)))                # no signal: the fading seed does not matter
    assert int((w != run(zeros, 21, NOISE_STD, 2)).sum()) > 0.99 * n
    plain = product.chanemu(noise_std=NOISE_STD, seed=1, **cfg)
    assert torch.equal(bits(w), bits(plain.execute(zeros)))                        # ... and the noise is the static emulator's
    plain.close()


# ---------------------------------------------------------------------------------------------- 7. end to end
PARITY = {}
N_CH, M, CP, TAPER, NF, PLEN = 2, 64, 8, 4, 12, 96


def through_the_channel(product, oracle, fading_seed, fmt, snr_db=25.0):
    """multichanneltx -> fading emulator (the scenario of tests/test_chanemu_fading.py) -> multichannelrx, and the oracle's receiver on
    the same emulated samples: (gpu frames, oracle frames, sent, noise_std)"""
    torch = base._torch()
    K = 2 * N_CH
    taps = [(0, 1.0), (K + 3, 0.35 - 0.2j), (3 * K, -0.15 + 0.2j)]
    fading = dict(doppler=3e-6, rice_k=(8.0, 0.0, 0.0), los_doppler=(0.9e-6, 0.0, 0.0), los_phase=(0x12345678, 0, 0), sinusoids=8,
                  log2_block=10, seed=fading_seed)
    tx = product.multichanneltx(N_CH, M, CP, TAPER)
    iq, sent = tx.generate(NF, PLEN, seed=79)
    tx.close()
    iq = torch.cat([iq, torch.zeros(64 * K, dtype=torch.complex64, device="cuda")])
    clean = product.chanemu(taps=taps, fading=fading)
    v = torch.view_as_real(clean.execute(iq))
    power = float(v.pow(2).sum()) / int(iq.numel())
    g = float(np.float32(0.5 / float(v.abs().max()))) if fmt == "sc16" else 1.0
    clean.close()
    nstd = float(np.sqrt(g * g * power / 10.0 ** (snr_db / 10.0) / 2.0))
    ce = product.chanemu(taps=taps, gain=g, noise_std=nstd, seed=2024, output_format=fmt, fading=fading)
    y = ce.execute(iq)
    n = int(iq.numel()) // (product.TILE * K) * (product.TILE * K)
    y = y[:n].contiguous()
    if fmt == "sc16":
        assert ce.clipped() == 0
        y_host = (base.host(y).astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64).reshape(-1)
    else:
        y_host = base.host(y)
    ce.close()
    rx = product.multichannelrx(N_CH, M, CP, TAPER, max_payload_len=PLEN, input_format=fmt)
    rx.Execute(y); rx.Flush()
    frames = list(rx.frames)
    rx.close()
    ora = oracle.MultiChannelRx(N_CH, M, CP, TAPER)
    ora.execute(np.ascontiguousarray(y_host))
    return frames, list(ora.frames), sent, nstd


E2E = [("seed4", 4, "cf32"), ("seed5", 5, "cf32"), ("seed4_sc16", 4, "sc16")]


@pytest.mark.parametrize("name,fseed,fmt", E2E, ids=[e[0] for e in E2E])
def test_end_to_end(product, oracle, name, fseed, fmt):
    from test_gpu_parity import match_frames, relerr, relerr_elem
    gpu, ora, sent, nstd = through_the_channel(product, oracle, fseed, fmt)
    for side, frames in (("gpu", gpu), ("oracle", ora)):
        assert len(frames) == N_CH * NF, (side, len(frames))
        seen = set()
        for f in frames:
            assert f.header_valid and f.payload_valid, (side, f)
            pid = (f.header[0] << 8) | f.header[1]
            assert sent[f.channel][pid] == (bytes(f.header), bytes(f.payload)), (side, f.channel, pid)
            seen.add((f.channel, pid))
        assert len(seen) == N_CH * NF
    w = we = 0.0
    for fg, fo in match_frames(gpu, ora):
        assert (fg.header_valid, fg.payload_valid) == (fo.header_valid, fo.payload_valid)
        assert bytes(fg.header) == bytes(fo.header) and bytes(fg.payload) == bytes(fo.payload)
        assert len(fg.framesyms) == len(fo.framesyms) > 0
        w, we = max(w, relerr(fg.framesyms, fo.framesyms)), max(we, relerr_elem(fg.framesyms, fo.framesyms))
    PARITY[name] = {"max_norm": w, "element_wise": we, "noise_std": nstd}
    print("chanemu_fading_parity %s: framesyms max-norm %.3e element-wise %.3e" % (name, w, we))
    assert w <= 1e-3, w


def test_contract_in_deep_fades(product, oracle):
    """fading seed 3: frames fade in and out (tests/test_chanemu_fading.py: the oracle delivers 15 of 24 from its own transmitter).  Both
    receivers agree on every frame's flags, every valid frame has the same bytes on the other side, and at least 8 are valid on both."""
    from test_gpu_parity import match_frames
    gpu, ora, sent, _ = through_the_channel(product, oracle, 3, "cf32")
    both = 0
    for fg, fo in match_frames(gpu, ora):
        assert (fg.header_valid, fg.payload_valid) == (fo.header_valid, fo.payload_valid), (fg.channel, fg.header, fo.header)
        if fg.header_valid or fo.header_valid:
            assert bytes(fg.header) == bytes(fo.header)
        if (fg.header_valid and fg.payload_valid) or (fo.header_valid and fo.payload_valid):
            assert bytes(fg.header) == bytes(fo.header) and bytes(fg.payload) == bytes(fo.payload)
            pid = (fg.header[0] << 8) | fg.header[1]
            assert sent[fg.channel][pid] == (bytes(fg.header), bytes(fg.payload))
            both += 1
    n_ora = sum(1 for f in ora if f.header_valid and f.payload_valid)
    print("chanemu fading contract case: %d valid on both sides, %d on the oracle's, %d / %d frames reported" % (both, n_ora, len(gpu), len(ora)))
    assert 8 <= n_ora <= 23, n_ora                                # the case stays a mixed one
    assert both >= 8
    PARITY["seed3_contract"] = {"valid_on_both": both, "oracle_valid": n_ora, "reported": len(ora)}


def test_zz_print_chanemu_fading_parity():
    """(last of this file: the deviations measured above as one JSON line -- profiles/chanemu_fading_parity.json is such a record;
    CHANEMU_FADING_PARITY_OUT names a file to write it to as well)"""
    line = json.dumps(PARITY, sort_keys=True)
    print("chanemu_fading_parity " + line)
    path = os.environ.get("CHANEMU_FADING_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")
