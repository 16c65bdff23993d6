"""Crest-factor reduction on the GPU (mcrx_hip_cfr_*): the copy where nothing exceeds the threshold, every
pass against the float64 model of tests/cfr_model.py, the statistics against integers, the operator against itself cut into pieces,
against the shared quantiser, the refusals, and end to end against the oracle and in front of the amplifier.

The bound of the model test (model_with_bound below), per component, eps = 2^-24 (one fp32 rounding, relative).  d is the bound
carried in from the pass before (0 in front of the first), |x| the model's input of the pass:
  e     the map x -> e = x - (x projected onto the disc of radius A) is 1-Lipschitz and continuous at |x| = A, so an input error (a
        component of it <= d, the vector <= sqrt2 d) moves e by at most sqrt2 d whichever side of the threshold either precision
        puts the sample on.  Its own arithmetic: t carries 2 roundings, sqrtf(t) half of that and 1, A / . one more (3 eps on a
        quotient <= 1), s = 1 - . one more on s <= 1, s x one more: 5 eps |x|.  A sample the two sides decide differently has
        |s| <= 3 eps beyond what its input error explains: covered by the same term, which is therefore charged to every sample
        the kernel can find above the threshold, |x| + sqrt2 d + 8 eps |x| > A (its input error, and t and A2 against A^2: 3 eps on
        the squares), and to no other:                   E = sqrt2 d + 5 eps |x|   there, 0 elsewhere
  c     errors of e pass through the taps: sum |h[k]| E.  Its own arithmetic: with S = sum |h[k]| |e[n +- k]| (every partial sum is
        at most S) the first product, the H additions e[n-k] + e[n+k] together and the H fmaf cost (H + 2) eps S; H + 3 is charged
  y     x - c: d' = d + sum |h| E + (H + 3) eps S + eps |y|
  gain  d' = |gain| (d + eps |y|)
and 0.1 % on top for the terms of second order."""
import ctypes as C
import fractions
import json
import math
import os

import numpy as np
import pytest

import cfr_model as model
import rfchain_model
import tx_sc16_model as q16

pytestmark = pytest.mark.gpu

EPS, SQ2 = 2.0 ** -24, math.sqrt(2.0)
SENTINEL, SENTINEL_WORD = 0x5A5B, 0x7FC05A5B
GUARD = 3                                                   # sentinel samples on either side of an output
RATIOS, PARITY = {}, {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def host(t):
    return t.cpu().numpy()


def taps_for(product, H):
    return product.cfr_lowpass(H, 0.28, 5.65)


def execute(cf, x, shift=0):
    """cf.execute on the host samples x (n + 2 halo of them) from a device buffer that begins `shift` samples behind a 16-byte
    boundary, into an output placed likewise between sentinels, which are checked: -> the n outputs on the host"""
    torch = _torch()
    out16 = cf.output_format == 1
    n = len(x) - 2 * cf.halo
    src = torch.zeros(len(x) + 2, dtype=torch.complex64, device="cuda")
    torch.view_as_real(src).view(torch.int32)[shift:shift + len(x)].copy_(torch.from_numpy(np.ascontiguousarray(x, np.complex64).view(np.int32).reshape(-1, 2)).cuda())
    if out16:
        dst = torch.full((n + 2 * GUARD + 2, 2), SENTINEL, dtype=torch.int16, device="cuda")
    else:
        dst = torch.zeros(n + 2 * GUARD + 2, dtype=torch.complex64, device="cuda")
        torch.view_as_real(dst).view(torch.int32).fill_(SENTINEL_WORD)
    lo = GUARD + shift
    y = cf.execute(src[shift:shift + len(x)], out=dst[lo:])
    assert int(y.shape[0]) == n
    got = host(dst if out16 else torch.view_as_real(dst).view(torch.int32))
    rest = np.concatenate([got[:lo], got[lo + n:]])
    assert np.all(rest == (SENTINEL if out16 else SENTINEL_WORD)), "written outside the output"
    return got[lo:lo + n].copy() if out16 else got[lo:lo + n].copy().view(np.float32).view(np.complex64).reshape(-1)


def round_f32(q):
    """the fp32 nearest to the non-negative rational q, ties to even"""
    if q == 0:
        return 0.0
    e = max(q.numerator.bit_length() - q.denominator.bit_length() - 24, -149)
    while q >= fractions.Fraction(2) ** (e + 24):
        e += 1
    while e > -149 and q < fractions.Fraction(2) ** (e + 23):
        e -= 1
    m = q / fractions.Fraction(2) ** e
    f = m.numerator // m.denominator
    r = m - f
    f += 1 if (r > fractions.Fraction(1, 2) or (r == fractions.Fraction(1, 2) and f % 2)) else 0
    return float(fractions.Fraction(f) * fractions.Fraction(2) ** e)


def power_f32(x, near=None):
    """t = fmaf(re, re, im * im) in fp32 for the complex64 samples x (NaN where a component is): float64 arithmetic, and exact rational
    arithmetic where its two roundings could differ from the one of the fmaf -- the samples within 1e-6 of `near` (default: of the maximum)"""
    x = np.ascontiguousarray(x, np.complex64)
    with np.errstate(invalid="ignore", over="ignore"):
        re, im = x.real.astype(np.float64), x.imag.astype(np.float64)   # (a signalling NaN is "invalid" in a cast)
        im2 = (x.imag * x.imag).astype(np.float64)                      # the fp32 product
        t = (re * re + im2).astype(np.float32).astype(np.float64)
        ref = np.nanmax(t) if near is None else float(near)
        close = np.flatnonzero(np.abs(t - ref) <= 1e-6 * ref)
    for i in close:
        t[i] = round_f32(fractions.Fraction(float(re[i])) ** 2 + fractions.Fraction(float(im2[i])))
    return t


def count_over(x, A):
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero(power_f32(x, near=model.threshold2(A)) > model.threshold2(A)))


# ---------------------------------------------------------------------------------------------- 1. nothing exceeds the threshold
def quiet_input(n, halo, seed):
    """n + 2 halo samples of every kind below A = 4: random values in (-1, 1); denormals, both zeros and NaNs with payloads among the n
    in the middle (as many of the eight as 2 n words hold) and scattered over the halos"""
    rng = np.random.RandomState(seed)
    w = rng.uniform(-1.0, 1.0, 2 * (n + 2 * halo)).astype(np.float32).view(np.uint32)
    special = np.array([0x80000000, 0x00000000, 0x7FC00001, 0x00000001, 0xFFC12345, 0x807FFFFF, 0x7F800001, 0x00400000], np.uint32)
    for i in range(min(2 * n, len(special))):
        w[2 * halo + (7 * i) % (2 * n)] = special[i]
    for side in (0, 2 * (halo + n)):
        at = rng.permutation(2 * halo)[:len(special)]
        w[side + at] = special[:len(at)]
    return w.view(np.float32).view(np.complex64)


@pytest.mark.parametrize("P", [1, 3])
def test_no_clipping_is_a_copy(product, P):
    H = 31
    cf = product.cfr(4.0, taps=taps_for(product, H), passes=P)
    assert cf.halo == P * H and cf.half_len == H and cf.passes == P
    want_peak = 0.0
    for n in (1, 2, 63, 2049, 4099):
        for shift in (0, 1):
            x = quiet_input(n, cf.halo, 100 * n + shift)
            if n > 2:
                x[cf.halo + n // 2] = 1.5 + 0.5j
            got = execute(cf, x, shift)
            mid = x[cf.halo:cf.halo + n]
            gw, mw = got.view(np.uint32), mid.view(np.uint32)
            nan = np.isnan(mid.view(np.float32))
            assert np.array_equal(gw[~nan], mw[~nan]), (P, n, shift)    # bit for bit: denormals and -0.0 among them
            assert np.all(np.isnan(got.view(np.float32)[nan])), (P, n, shift)
            assert nan.any() or n < 2
            want_peak = max(want_peak, float(np.nanmax(np.concatenate([power_f32(mid), [0.0]]))))
    over, peak2 = cf.stats()
    assert over == [0] * P
    assert peak2 == want_peak == 2.5
    assert cf.clipped() == 0
    assert cf.stats(reset=True)[1] == 2.5 and cf.stats() == ([0] * P, 0.0)
    cf.close()
    cf.close()                                                          # twice is harmless


def test_negative_taps_follow_the_definition(product):
    """every tap negative: c = -0 where nothing is within reach, so -0.0 comes out as +0.0 and every other word as it is -- in one call
    and in pieces alike, because such a handle skips nothing"""
    torch = _torch()
    taps, n = np.array([-0.5, -0.25, -0.0], np.float32), 1500
    cf = product.cfr(4.0, taps=taps)
    x = quiet_input(n, cf.halo, 9)
    x[cf.halo + 700] = 5.0 - 1.0j                                       # one sample above the threshold, far from most of the stream
    got = execute(cf, x, 1).view(np.uint32)
    mid = x[cf.halo:cf.halo + n].view(np.uint32)
    far = np.ones(2 * n, bool)
    far[2 * (700 - cf.halo):2 * (700 + cf.halo + 1)] = False
    nan = np.isnan(mid.view(np.float32))
    want = np.where(mid == 0x80000000, 0, mid)
    assert np.count_nonzero(mid[far] == 0x80000000) > 0
    assert np.array_equal(got[far & ~nan], want[far & ~nan])
    d_x = torch.from_numpy(x).cuda()
    pieces = torch.cat([cf.execute(d_x[a:b + 2 * cf.halo]) for a, b in ((0, 1), (1, 600), (600, 601), (601, n))])
    assert np.array_equal(host(torch.view_as_real(pieces).contiguous().view(torch.int32)).reshape(-1).view(np.uint32)[~nan], got[~nan])
    assert cf.stats()[0] == [2]
    cf.close()


# ---------------------------------------------------------------------------------------------- 2. against the model
A_MODEL = 0.75
KINDS = {"1%": 0.01, "10%": 0.10, "60%": 0.60, "all": None}
LENGTHS = [1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 4099]
_X = {}


def noise(n, kind, seed):
    """n samples, made once and left alone: Gaussian with the share KINDS[kind] of them above A_MODEL (P(|x| > A) = exp(-A^2 / 2 sigma^2)),
    or every sample at 1.2 .. 3 A"""
    if (n, kind, seed) not in _X:
        rng = np.random.RandomState(seed)
        if KINDS[kind] is None:
            x = A_MODEL * rng.uniform(1.2, 3.0, n) * np.exp(2j * np.pi * rng.uniform(size=n))
        else:
            sigma = A_MODEL / math.sqrt(-2.0 * math.log(KINDS[kind]))
            x = sigma * (rng.randn(n) + 1j * rng.randn(n))
        _X[(n, kind, seed)] = x.astype(np.complex64)
    return _X[(n, kind, seed)]


def model_with_bound(x, A, h, passes, gain):
    """(model output, bound on each component of got - model): the module docstring's recursion along the model's passes"""
    H = len(h) - 1
    habs, hfull = np.abs(model.full_taps(h)), model.full_taps(h)
    y = np.asarray(x, np.complex128)
    d = np.zeros(len(y))
    for _ in range(passes):
        e, _ = model.excess(y, A)
        mag = np.abs(y)
        E = np.where(mag + SQ2 * d + 8.0 * EPS * mag > A, SQ2 * d + 5.0 * EPS * mag, 0.0)
        S = np.convolve(np.abs(e), habs, mode="valid")
        new = y[H:len(y) - H] - np.convolve(e, hfull, mode="valid")
        d = d[H:len(d) - H] + np.convolve(E, habs, mode="valid") + (H + 3) * EPS * S + EPS * np.abs(new)
        y = new
    if gain != 1.0:
        d = abs(gain) * (d + EPS * np.abs(y))
    return gain * y, d * 1.001


def worst_ratio(got, want, bound):
    diff = np.asarray(got, np.complex128) - want
    tiny = np.finfo(np.float32).tiny                                    # (a zero sample has a zero bound: 0 <= 0)
    return float(np.max(np.maximum(np.abs(diff.real), np.abs(diff.imag)) / np.maximum(bound, tiny)))


@pytest.mark.parametrize("H", [1, 7, 31, 64])
@pytest.mark.parametrize("P", [1, 2, 3])
def test_against_the_model(product, H, P):
    """every length, from buffers on a 16-byte boundary and one sample behind it; the four kinds of input take turns over the lengths
    and all four are run at the longest"""
    gain = 0.8
    cf = product.cfr(A_MODEL, taps=taps_for(product, H), passes=P, gain=gain)
    A, h = float(cf.config.threshold), cf.taps
    worst, names = 0.0, list(KINDS)
    runs = [(n, names[(i + H + P) % 4]) for i, n in enumerate(LENGTHS)] + [(LENGTHS[-1], k) for k in names]
    for i, (n, kind) in enumerate(runs):
        x = noise(n + 2 * cf.halo, kind, 1000 * H + 10 * P + (i % 3))
        want, bound = model_with_bound(x, A, h, P, gain)
        if KINDS[kind] is not None and n == LENGTHS[-1]:                # the input is what its name says
            share = np.count_nonzero(model.excess(x, A)[1]) / float(len(x))
            assert 0.6 * KINDS[kind] < share < 1.4 * KINDS[kind], (kind, share)
        assert np.allclose(want, model.apply(x, A, h, P, gain), rtol=0, atol=0)    # (the recursion walks the model itself)
        for shift in (0, 1):
            r = worst_ratio(execute(cf, x, shift), want, bound)
            assert r <= 1.0, (H, P, n, kind, shift, r)
            worst = max(worst, r)
    RATIOS["H%d_P%d" % (H, P)] = worst
    print("cfr_model H=%d P=%d: worst fraction of the bound %.3f" % (H, P, worst))
    cf.close()


# ---------------------------------------------------------------------------------------------- 3. the statistics are integers
@pytest.mark.parametrize("P", [1, 3])
def test_counts(product, P):
    """components on the grid k 2^-10, |k| <= 4096, and A = 1.5: t = (k1^2 + k2^2) 2^-20 is exact up to 4 and rounds monotonically
    above, A2 = 2.25 is exact, so numpy's integers decide as the kernel does"""
    H, n, A = 7, 4099, 1.5
    rng = np.random.RandomState(5 + P)
    k = np.clip(np.rint(rng.randn(n + 2 * P * H, 2) * 1100.0), -4096, 4096).astype(np.int64)
    k[17], k[n // 2] = (4096, -4096), (1536, 0)                         # the corner of the grid; |x| = A exactly: not above
    x = (k[:, 0] * 2.0 ** -10 + 1j * k[:, 1] * 2.0 ** -10).astype(np.complex64)
    cf = product.cfr(A, taps=taps_for(product, H), passes=P)
    y = execute(cf, x, 1)
    over, peak2 = cf.stats()
    mid = k[P * H:P * H + n]
    want0 = int(np.count_nonzero(mid[:, 0] ** 2 + mid[:, 1] ** 2 > 2359296))      # 2.25 * 2^20
    print("cfr counts P=%d: over %s of %d, peak2 %.6f" % (P, over, n, peak2))
    assert 0.1 * n < want0 < 0.6 * n and over[0] == want0
    assert peak2 == float(np.nanmax(power_f32(y)))
    # over[p]: the count taken from the operator's own output of p passes around the same n samples
    for p in range(1, P):
        part = product.cfr(A, taps=taps_for(product, H), passes=p)
        yp = execute(part, x[(P - p) * H:(P - p) * H + n + 2 * p * H], 0)
        part.close()
        assert over[p] == count_over(yp, A), p
        assert 0 < over[p] < n
    cf.close()


# ---------------------------------------------------------------------------------------------- 4. cuts
N_CUT = 3001


@pytest.mark.parametrize("fout", ["cf32", "sc16"])
@pytest.mark.parametrize("P", [1, 3])
def test_cuts(product, fout, P):
    """one call against pieces of 1, 2, 3, 255, 256, 257 samples and the rest, each with its halos"""
    torch = _torch()
    H = 31
    halo = P * H
    x = noise(N_CUT + 2 * halo, "10%", 77 + P)
    d_x = torch.from_numpy(x).cuda()
    gain = 1.6 if fout == "sc16" else 1.0                               # sc16: |y| reaches about A = 0.75, times 1.6: some samples clip
    kw = dict(taps=taps_for(product, H), passes=P, gain=gain, output_format=fout)
    one, pieces = product.cfr(A_MODEL, **kw), product.cfr(A_MODEL, **kw)
    want = one.execute(d_x).clone()
    if fout == "sc16":
        buf = torch.full((N_CUT + 8, 2), SENTINEL, dtype=torch.int16, device="cuda")
    else:
        buf = torch.full((N_CUT + 8,), float("nan"), dtype=torch.complex64, device="cuda")
    pos, starts = 0, set()
    for size in (1, 2, 3, 255, 256, 257, N_CUT):
        end = min(pos + size, N_CUT)
        starts.add(pos & 1)
        y = pieces.execute(d_x[pos:end + 2 * halo], out=buf[pos:])
        assert int(y.shape[0]) == end - pos
        pos = end
    assert pos == N_CUT and starts == {0, 1}
    bits = (lambda t: t) if fout == "sc16" else (lambda t: torch.view_as_real(t).contiguous().view(torch.int32))
    assert torch.equal(bits(buf[:N_CUT]), bits(want))
    tail = buf[N_CUT:]
    assert bool((tail == SENTINEL).all()) if fout == "sc16" else bool(torch.isnan(tail.real).all())
    (over1, peak1), (overp, peakp) = one.stats(), pieces.stats()
    print("cfr cuts %s P=%d: over %s, peak2 %.6f, clipped %d" % (fout, P, over1, peak1, one.clipped()))
    assert over1 == overp and over1[0] > 100 and peak1 == peakp > 0.0
    assert one.clipped() == pieces.clipped()
    assert (one.clipped() > 20) if fout == "sc16" else (one.clipped() == 0)
    one.close(); pieces.close()


def test_the_scratch_buffers_grow_and_are_reused(product):
    """passes = 3 (both scratch buffers), half_len = 8: 300 samples in the first allocation, 20 000 that force both to grow, 300 again in
    the grown ones -- each call the bits of a fresh handle's"""
    torch = _torch()
    H, P = 8, 3
    d_x = torch.from_numpy(noise(20000 + 2 * P * H, "10%", 91)).cuda()
    kw = dict(taps=taps_for(product, H), passes=P)
    cf = product.cfr(A_MODEL, **kw)
    for n in (300, 20000, 300):
        fresh = product.cfr(A_MODEL, **kw)
        got, want = cf.execute(d_x[:n + 2 * P * H]), fresh.execute(d_x[:n + 2 * P * H])
        assert int(got.shape[0]) == n and fresh.stats()[0][0] > 0
        assert torch.equal(torch.view_as_real(got).view(torch.int32), torch.view_as_real(want).view(torch.int32)), n
        fresh.close()
    cf.close()


# ---------------------------------------------------------------------------------------------- 5. sc16 is Q of cf32
@pytest.mark.parametrize("P", [1, 2])
def test_sc16_is_q_of_cf32(product, P):
    H, n, gain = 31, 4099, 1.45
    x = noise(n + 2 * P * H, "10%", 31 + P).copy()
    x[[P * H + 5, P * H + 900]] = [complex(np.nan, 0.1), complex(0.2, np.nan)]
    kw = dict(taps=taps_for(product, H), passes=P, gain=gain)
    cf, sc = product.cfr(A_MODEL, **kw), product.cfr(A_MODEL, output_format="sc16", **kw)
    y, i = execute(cf, x, 1), execute(sc, x, 1)
    want = q16.clipped_samples(y)
    mclip = q16.clipped_samples(model.apply(np.nan_to_num(x), A_MODEL, cf.taps, P, gain).astype(np.complex64))
    print("cfr sc16 P=%d: %d of %d samples clip (the float64 model without the NaNs: %d)" % (P, want, n, mclip))
    assert 100 <= want <= n // 4, want                                  # some hundred clip, most do not
    assert np.array_equal(i, q16.quantise_iq(y))
    assert np.isnan(y.view(np.float32)).any()                           # NaN went through and is not counted
    assert cf.clipped() == 0 and cf.stats() == sc.stats()
    assert sc.clipped() == want and sc.clipped(reset=True) == want and sc.clipped() == 0
    cf.close(); sc.close()


# ---------------------------------------------------------------------------------------------- 6. refusals on the device
def test_refusals_on_the_device(product):
    torch = _torch()
    L, EINVAL, OK = product.lib(), product.MCRX_EINVAL, product.MCRX_OK
    n = 4096
    buf = torch.zeros(4 * n, dtype=torch.complex64, device="cuda")
    torch.view_as_real(buf).view(torch.int32).fill_(SENTINEL_WORD)
    keep = buf.clone()
    p = buf.data_ptr()
    for fout in ("cf32", "sc16"):
        cf = product.cfr(0.5, passes=2, output_format=fout)             # halo 62: a call of n reads n + 124 samples
        so, nin = (4 if fout == "sc16" else 8), n + 2 * cf.halo

        def call(a, b, count=n):
            return L.mcrx_hip_cfr_execute_device(cf._h, C.c_void_p(a) if a else None, count, C.c_void_p(b) if b else None, None)
        assert call(None, p) == EINVAL and call(p, None) == EINVAL
        assert call(p + 4, p + 16 * n) == EINVAL                        # d_in: half a sample
        assert call(p, p + 16 * n + so // 2) == EINVAL                  # d_out likewise
        assert call(p, p) == EINVAL                                     # in place
        assert call(p, p + 8 * cf.halo) == EINVAL                       # the output on the samples it belongs to
        assert call(p, p + 8 * nin - so) == EINVAL                      # the output's first sample on the input's last
        assert call(p + so * n - 8, p) == EINVAL                        # the input's first sample on the output's last
        assert call(p, p + 16 * n, 1 << 32) == EINVAL                   # 2^32 samples and their halos
        assert call(p, p + 16 * n, (1 << 32) - 2 * cf.halo + 1) == EINVAL
        assert L.mcrx_hip_cfr_last_error()
        with pytest.raises(ValueError):
            cf.execute(buf[:nin], out=torch.view_as_real(buf).view(torch.int16).view(-1, 2) if fout == "sc16" else buf)
        with pytest.raises(ValueError):
            cf.execute(buf[:2 * cf.halo - 1])                           # shorter than the halos
        with pytest.raises(TypeError):
            cf.execute(buf.real)
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(buf).view(torch.int32), torch.view_as_real(keep).view(torch.int32)), fout
        assert cf.clipped() == 0 and cf.stats() == ([0, 0], 0.0)
        # what is allowed: adjacent ranges, nothing to do, and an empty tensor
        assert call(p, p + 8 * nin) == OK and call(p + so * n, p) == OK and call(p, p, 0) == OK
        assert int(cf.execute(buf[:2 * cf.halo]).shape[0]) == 0
        torch.cuda.synchronize()
        buf.copy_(keep)
        cf.close()


# ---------------------------------------------------------------------------------------------- 7. end to end
def rms_of(torch, t):
    return float(torch.view_as_real(t).double().pow(2).sum().div(int(t.numel())).sqrt())


def papr_of(torch, t):
    p = torch.view_as_real(t).double().pow(2).sum(dim=1)
    return float(10.0 * torch.log10(p.max() / p.mean()))


def oob_of(torch, t, edge):
    """cfr_model.oob_db with torch.fft on the device"""
    nfft = model.SPECTRUM_NFFT
    seg = t.to(torch.complex128).unfold(0, nfft, nfft // 2) * torch.hann_window(nfft, periodic=True, dtype=torch.float64, device=t.device)
    P = torch.fft.fft(seg, dim=1).abs().pow(2).mean(dim=0)
    f = torch.fft.fftfreq(nfft, device=t.device, dtype=torch.float64)
    return float(10.0 * torch.log10(P[f.abs() > edge].sum() / P.sum()))


def severity_stream(product):
    torch = _torch()
    s = model.SEVERITY
    tx = product.multichanneltx(s["N"], s["M"], s["cp"], s["taper"])
    iq, sent = tx.generate(s["frames"], s["payload_len"], seed=77 + s["N"])      # QPSK / Hamming(12,8), gain 1 / N
    tx.close()
    return iq, sent, rms_of(torch, iq)


def test_end_to_end(product, oracle):
    """multichanneltx -> cfr (cfr_model.SEVERITY, sc16 out) -> multichannelrx(sc16), and the oracle's receiver on the same integers
    times 2^-15.  The gain puts the largest component of the MODEL's output at 0.9 of full scale, so the model clips nothing; the same
    stream at the same gain without the stage clips.  framesyms: held to the 1e-3 the sibling end-to-end tests assert, the deviation
    recorded (PARITY, printed by the last test)."""
    from test_gpu_parity import match_frames, relerr, relerr_elem
    torch = _torch()
    s = model.SEVERITY
    N, nf = s["N"], s["frames"]
    iq, sent, rms = severity_stream(product)
    x = host(iq)
    h = product.cfr_lowpass(s["half_len"], s["cutoff"], s["beta"])
    A = float(np.float32(product.cfr_threshold(s["papr_db"], rms)))
    ym = model.apply_stream(x, A, h, s["passes"])
    g = float(np.float32(s["peak"] / max(np.abs(ym.real).max(), np.abs(ym.imag).max())))
    assert q16.clipped_samples((g * ym).astype(np.complex64)) == 0
    bare = int(q16.clipped_samples(np.float32(g) * x))                  # the stream as it is, at the same gain (one fp32 multiply)
    plain = product.rfchain(gain=g, output_format="sc16")
    plain.execute(iq)
    assert plain.clipped() == bare > 0
    plain.close()
    cf = product.cfr(A, taps=h, passes=s["passes"], gain=g, output_format="sc16")
    y = cf.execute(iq, pad=True)
    assert int(y.shape[0]) == int(iq.numel()) and cf.clipped() == 0
    over, peak2 = cf.stats()
    cf.close()
    # the floats of the same operator: PAPR and the power beyond the band edge against the model on the same input
    cf32 = product.cfr(A, taps=h, passes=s["passes"])
    yf = cf32.execute(iq, pad=True)
    assert cf32.stats() == (over, peak2)
    cf32.close()
    papr, papr_m = papr_of(torch, yf), model.papr_db(ym)
    oob, oob_m, oob_in = oob_of(torch, yf, s["edge"]), model.oob_db(ym, s["edge"]), oob_of(torch, iq, s["edge"])
    assert abs(10.0 * math.log10(peak2 / (model.rms(ym) ** 2)) - papr_m) <= 0.05
    n = int(y.shape[0]) // (product.TILE * 2 * N) * (product.TILE * 2 * N)
    y = y[:n].contiguous()
    y_host = (host(y).astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64).reshape(-1)
    rx = product.multichannelrx(N, s["M"], s["cp"], s["taper"], max_payload_len=s["payload_len"], input_format="sc16")
    rx.Execute(y); rx.Flush()
    ora = oracle.MultiChannelRx(N, s["M"], s["cp"], s["taper"])
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
    evm = [f.evm for f in rx.frames]
    rx.close()
    PARITY["severity"] = {"max_norm": w, "element_wise": we, "rms": rms, "threshold": A, "gain": g, "over": over, "clipped_without": bare,
                          "papr_db": [papr_of(torch, iq), papr, papr_m], "oob_db": [oob_in, oob, oob_m], "evm_db": [min(evm), max(evm)]}
    print("cfr_parity: framesyms max-norm %.3e element-wise %.3e; EVM %.1f .. %.1f dB; PAPR %.2f dB (model %.2f); power at |f| > %.2f "
          "%.1f dB (model %.1f, input %.1f); over %s; %d samples clip without the stage"
          % (w, we, min(evm), max(evm), papr, papr_m, s["edge"], oob, oob_m, oob_in, over, bare))
    assert abs(papr - papr_m) <= 0.05
    assert abs(oob - oob_m) <= 0.5 or (oob < -80.0 and oob_m < -80.0)
    assert w <= 1e-3, w


def test_behind_the_amplifier(product):
    """cfr -> rfchain (the amplifier alone at 6 dB input back-off) against the float64 model of both, and against the amplifier
    without the stage in front of it"""
    torch = _torch()
    s = model.SEVERITY
    iq, _, rms = severity_stream(product)
    h = product.cfr_lowpass(s["half_len"], s["cutoff"], s["beta"])
    A = float(np.float32(product.cfr_threshold(s["amp_papr_db"], rms)))
    ampk = dict(amplifier=dict(sat=product.rfchain_backoff(s["amp_ibo_db"], rms), smooth=s["amp_smooth"]))
    cf, amp = product.cfr(A, taps=h, passes=s["passes"]), product.rfchain(**ampk)
    with_, without = amp.execute(cf.execute(iq, pad=True)), amp.execute(iq)
    oob1, oob0 = oob_of(torch, with_, s["edge"]), oob_of(torch, without, s["edge"])
    cf.close(); amp.close()
    cfg = product.rfchain_config(**ampk)
    x = host(iq)
    m1 = model.oob_db(rfchain_model.amplifier(cfg, model.apply_stream(x, A, h, s["passes"])), s["edge"])
    m0 = model.oob_db(rfchain_model.amplifier(cfg, x.astype(np.complex128)), s["edge"])
    PARITY["amplifier"] = {"oob_db_with": [oob1, m1], "oob_db_without": [oob0, m0]}
    print("cfr behind the amplifier: power at |f| > %.2f %.2f dB with the stage (model %.2f), %.2f dB without (model %.2f)"
          % (s["edge"], oob1, m1, oob0, m0))
    assert abs(oob1 - m1) <= 0.5 and abs(oob0 - m0) <= 0.5
    assert oob0 - oob1 >= s["amp_oob_gain_db"]


def test_zz_print_cfr_figures():
    """(last of this file: the figures measured above as one JSON line each -- profiles/cfr_model.json and profiles/cfr_parity.json are
    such records; CFR_OUT / CFR_PARITY_OUT name files to write them to as well)"""
    for tag, rec, env in (("cfr_model", RATIOS, "CFR_OUT"), ("cfr_parity", PARITY, "CFR_PARITY_OUT")):
        line = json.dumps(rec, sort_keys=True)
        print(tag + " " + line)
        path = os.environ.get(env)
        if path:
            with open(path, "w") as f:
                f.write(line + "\n")
