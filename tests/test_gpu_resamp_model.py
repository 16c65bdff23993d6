"""The resampler on the GPU (csrc/msresamp.hip) against the float64 model of tests/resamp_model.py, whose docstring
derives the bound: at the kernels' tile edges, tap by tap and branch by branch, through deep chains of half-band stages fed in awkward
pieces, at the neighbours of the rates where the chain changes shape, its delay, and its two integer formats.  Every comparison with
the model asserts (a) every component within its derived bound and (b) the max-norm error within REL = 1e-5 of the model's peak; every
call asserts nout <= max_output(nin).  All integers and taps come from msresamp_plan.  Neither the oracle nor the reference is needed.

Tile sizes: the half-band kernels make 1024 outputs a workgroup; the arbitrary kernel 8 chunks of 1024, with a half-band decimator
folded in (rates below 1/2) 8 chunks of 512.  An interpolating handle makes its outputs in runs (2 per input at rate 2, 2^num_stages per
output of the arbitrary stage), so where a count cannot be met the fewest inputs that make at least as many are fed."""
import json
import os

import numpy as np
import pytest

import resamp_model as model

pytestmark = pytest.mark.gpu

F32 = np.float32
COUNTS = [1, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 16385]
FIGURES = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def noise(seed, n):
    rng = np.random.RandomState(seed)
    return (rng.randn(n) + 1j * rng.randn(n)).astype(np.complex64)


def execute(product, q, d_x):
    """one call on a device tensor -> the outputs on the host; nout <= max_output(nin)"""
    n = int(d_x.numel()) if d_x.dtype != _torch().int16 else int(d_x.numel()) // 2
    y = q.execute(d_x)
    assert int(y.shape[0]) <= int(product.lib().msresamp_hip_max_output(q._h, n))
    return y.cpu().numpy()


def hold(tag, got, y, bound):
    """bars (a) and (b); the worst figures of a tag are kept for the record"""
    assert len(got) == len(y)
    frac, rel = model.compare(got, y, bound)
    rec = FIGURES.setdefault(tag, {"bound_fraction": 0.0, "max_norm": 0.0})
    rec["bound_fraction"], rec["max_norm"] = max(rec["bound_fraction"], frac), max(rec["max_norm"], rel)
    print("%s: n = %d, %.3f of the bound, max-norm %.2e of the peak" % (tag, len(y), frac, rel))
    assert frac <= 1.0, (tag, len(y), frac)
    assert rel <= model.REL, (tag, len(y), rel)


@pytest.mark.parametrize("rate", [0.8, 0.7, 0.37, 0.25, 0.11, 1.5, 2.0, 4.0, 6.3])
def test_model_at_the_tile_edges(product, rate):
    """0.8 the fixed-tap build, 0.7 the table build, 0.37 a folded half-band stage and the table, 0.25 folded and fixed, 0.11 two
    stand-alone half-band kernels in front, 1.5 / 2.0 the arbitrary stage alone, 4.0 / 6.3 with one and two interpolators behind it.
    Noise of unit variance at every count; a tone of 0.45 cycles per input sample once (decimating: 60 - 100 dB down at the output, where
    only the bound can see an error)."""
    torch = _torch()
    p = product.msresamp_plan(rate)
    nmax = model.nin_for(p, COUNTS[-1])
    x = noise(int(rate * 1000) + 11, nmax)
    y, bound = model.run(p, x)
    d_x = torch.from_numpy(x).cuda()
    q = product.msresamp(rate)
    for count in COUNTS:
        nin = model.nin_for(p, count)
        nout = model.count_out(p, nin)
        assert nout >= count and (nout == count or p.interp)
        q.reset()
        got = execute(product, q, d_x[:nin])
        assert len(got) == nout
        hold("edges_%g" % rate, got, y[:nout], bound[:nout])
    tone = np.exp(2j * np.pi * 0.45 * np.arange(nmax)).astype(np.complex64)
    yt, bt = model.run(p, tone)
    q.reset()
    hold("tone_%g" % rate, execute(product, q, torch.from_numpy(tone).cuda()), yt, bt)
    q.close()


@pytest.mark.parametrize("rate", [1.0, 0.5, 0.8, 0.64, 1.25, 2.0, 0.7, 0.999, 1.5])
def test_taps_and_branches_bit_for_bit(product, rate):
    """The arbitrary stage alone.  1.0 - 0.5j on every 32nd sample of zeros: at most one product of a 14-tap sum is not zero, and it is
    exact, so output j is H[b_j][k] (1 - 0.5j) for the k that puts the impulse into its window and 0 where none is in it -- over a
    second workgroup and all of its chunks.  Twice, the impulses on samples 32 m and on 32 m + 1: at rate 1/2 every n_j is even and one
    train meets the odd taps only; together they meet all fourteen.  (1, 1/2, 0.8, 1.25, 2 keep a thread's taps in registers; 0.7,
    0.999, 1.5 and -- its step is odd as a float -- 0.64 read the staged table.)"""
    torch = _torch()
    p = product.msresamp_plan(rate)
    assert p.num_stages == 0
    nin = model.nin_for(p, 8193)
    nj, bj = model.arbitrary_indices(p.step, nin)
    q = product.msresamp(rate)
    taps_met = set()
    for first in (0, 1):
        x = np.zeros(nin, np.complex64)
        x[first::32] = 1.0 - 0.5j
        k = (13 + first - nj) % 32                      # window sample k is input sample n_j - 13 + k
        hit = (k < 14) & (nj - 13 + k >= 0)
        h = np.where(hit, p.hpfb[bj, np.minimum(k, 13)], F32(0)).astype(np.float32)
        want = (h + 1j * (h * F32(-0.5))).astype(np.complex64)
        taps_met |= set(k[hit].tolist())
        q.reset()
        got = execute(product, q, torch.from_numpy(x).cuda())
        assert len(got) == len(want) and len(got) >= 8193
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (first, len(bad), bad[:8], got[bad[:8]], want[bad[:8]])
        y, bound = model.run(p, x)                      # the model says the same, with a bound of rounding size
        assert np.array_equal(y.astype(np.complex64), want)
    q.close()
    assert taps_met == set(range(14))


def pieces(n, stride):
    """call sizes that add up to n: single samples, an empty call, sizes below, at and above `stride`, then the rest"""
    out, pos = [], 0
    for s in [1, 0, 1, 3, stride - 1, 7, stride + 1, 0, 2, stride, 1, n]:
        s = min(s, n - pos)
        out.append(s)
        pos += s
    assert pos == n
    return out


@pytest.mark.parametrize("rate,nin", [(0.001, None), (1.0 / 65536, None), (1024.0, 200)], ids=["0.001", "2^-16", "1024"])
def test_deep_chains(product, rate, nin):
    """Nine decimators (0.001), fifteen and an arbitrary stage that halves once more (2^-16), nine interpolators (1024): an input just
    long enough for 64 outputs (1024: 200 samples) against the model; the same input in pieces after many of which some stages have
    nothing new, and from a buffer one sample off its alignment, bit for bit the single call."""
    torch = _torch()
    p = product.msresamp_plan(rate)
    assert p.num_stages == {0.001: 9, 1.0 / 65536: 15, 1024.0: 9}[rate]
    nin = nin or model.nin_for(p, 64)
    x = noise(p.num_stages, nin)
    y, bound = model.run(p, x)
    d_x = torch.from_numpy(x).cuda()
    q = product.msresamp(rate)
    got = execute(product, q, d_x)
    assert len(got) == model.count_out(p, nin) and len(got) >= 64
    hold("deep_%g" % rate, got, y, bound)
    q.reset()
    parts, pos = [], 0
    for s in pieces(nin, 8 if p.interp else 1 << p.num_stages):
        parts.append(execute(product, q, d_x[pos:pos + s]))
        pos += s
    assert np.array_equal(np.concatenate(parts).view(np.uint32), got.view(np.uint32))
    off = torch.zeros(nin + 1, dtype=torch.complex64, device="cuda")
    off[1:].copy_(d_x)
    q.reset()
    assert np.array_equal(execute(product, q, off[1:]).view(np.uint32), got.view(np.uint32))
    q.close()


@pytest.mark.parametrize("rate", [0.5, float(np.nextafter(F32(0.5), F32(0))), 1.0, float(np.nextafter(F32(1), F32(2))), 2.0,
                                  float(np.nextafter(F32(2), F32(3)))], ids=["0.5", "0.5-", "1", "1+", "2", "2+"])
def test_rate_edges(product, rate):
    """the neighbours of 1/2, 1 and 2, where a stage appears or the chain turns round: 4097 outputs"""
    torch = _torch()
    p = product.msresamp_plan(rate)
    nin = model.nin_for(p, 4097)
    x = noise(int(rate * 64), nin)
    y, bound = model.run(p, x)
    q = product.msresamp(rate)
    got = execute(product, q, torch.from_numpy(x).cuda())
    q.close()
    hold("rate_edge_%.9g" % rate, got, y, bound)


@pytest.mark.parametrize("rate", [0.37, 2.0, 4.0, 16.0])
def test_delay_on_the_device(product, rate):
    """get_delay() is the plan's, and the delay the GPU's own output shows for the slow tone lies within the tolerance of it"""
    torch = _torch()
    p = product.msresamp_plan(rate)
    x, f_in = model.delay_tone(p)
    q = product.msresamp(rate)
    assert q.get_delay() == p.delay
    got = execute(product, q, torch.from_numpy(x).cuda())
    q.close()
    D = model.fit_delay(p, got, f_in)
    FIGURES["delay_%g" % rate] = {"fitted": D, "get_delay": p.delay}
    print("rate %g: the GPU's output shows %.4f input samples, get_delay() %.4f" % (rate, D, p.delay))
    assert abs(p.delay - D) <= model.delay_tolerance(p)


@pytest.mark.parametrize("rate", [0.001, 0.06, 0.5, 1.0, 1.5, 6.3, 100.0, 1024.0])
def test_get_delay_is_the_plans(product, rate):
    q = product.msresamp(rate)
    assert q.get_delay() == product.msresamp_plan(rate).delay
    q.close()


@pytest.mark.parametrize("rate", [0.37, 4.0])
def test_formats_against_the_model(product, rate):
    """An sc16-input handle: the samples mean (re, im) 2^-15, the model on those holds its outputs to (a) and (b), and a cf32 handle on
    those floats gives the same bits.  An sc16-output handle with gain 0.5: with v the fp32 values a cf32 handle of that gain stores --
    held to the model by (a) and (b) -- it stores exactly the model's Q(v) and counts exactly the samples Q clips.  Q of the float64
    model itself cannot be asked bit for bit (v sits within the bound of it, and a rounding boundary may lie between): every stored
    component is within 1/2 + 32768 bound of the model's clamped 32768 y, and the count lies between the samples that clip for every
    value within the bound and those that clip for some."""
    torch = _torch()
    p = product.msresamp_plan(rate)
    nin = model.nin_for(p, 4097)
    rng = np.random.RandomState(int(rate * 100))
    w = np.clip(np.rint(rng.randn(nin, 2) * 8000.0), -32768, 32767).astype(np.int16)
    w[:4] = [[-32768, 32767], [32767, -32768], [0, -1], [1, 0]]
    xs = model.from_sc16(w)
    y, bound = model.run(p, xs)
    qi = product.msresamp(rate, input_format="sc16")
    got = execute(product, qi, torch.from_numpy(w).cuda())
    qi.close()
    hold("sc16_in_%g" % rate, got, y, bound)
    qf = product.msresamp(rate)
    same = execute(product, qf, torch.from_numpy(xs.astype(np.complex64)).cuda())
    qf.close()
    assert np.array_equal(same.view(np.uint32), got.view(np.uint32))
    # sc16 out, gain 0.5: noise of three times the full scale's rms, so that a good share of the samples clips at either rate
    x = noise(int(rate * 100) + 1, nin) * F32(3)
    y, bound = model.run(p, x, gain=0.5)
    d_x = torch.from_numpy(x).cuda()
    qg = product.msresamp(rate, gain=0.5)
    v = execute(product, qg, d_x)
    qg.close()
    hold("gain_%g" % rate, v, y, bound)
    qo = product.msresamp(rate, output_format="sc16", gain=0.5)
    out = execute(product, qo, d_x)
    clipped = qo.clipped()
    qo.close()
    want, nclip = model.quantised(v)
    assert out.dtype == np.int16 and np.array_equal(out, want)
    assert clipped == nclip and nclip > 0.01 * len(v)
    r, e = 32768.0 * model.as_pairs(y), 32768.0 * bound
    assert np.all(np.abs(out.astype(np.float64) - np.clip(r, -32768.0, 32767.0)) <= 0.5 + e)
    surely = ((r - e > 32767.5) | (r + e < -32768.5)).any(axis=1)
    maybe = ((r + e >= 32767.5) | (r - e <= -32768.5)).any(axis=1)
    assert int(surely.sum()) <= clipped <= int(maybe.sum())


def test_zz_print_resamp_figures():
    """(last of this file: the figures measured above as one JSON line -- profiles/resamp_model.json is such a record; RESAMP_OUT names a
    file to write it to as well)"""
    line = json.dumps(FIGURES, sort_keys=True)
    print("resamp_model " + line)
    path = os.environ.get("RESAMP_OUT")
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")
