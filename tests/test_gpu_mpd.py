"""Predistortion with memory on the MI355X (mcrx_hip_mpd_*) against tests/mpd_model.py: the untouched handle is a copy bit for bit; one
branch is dpd bit for bit; the apply within the rounding bound the model derives; cuts that carry their leads, sc16 as Q of cf32; the
sums are the model's integers and coefficients, res and tables after updates the model's to the last bit; the refusals; the closed loop
on a three-branch amplifier at mpd_model.SEVERITY against dpd on the same amplifier, with the receiver and the oracle behind it."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cfr_model
import mpd_model as model
import tx_sc16_model as q16
from test_gpu_dpd import (SENTINEL, SENTINEL_WORD, _torch, amplitudes, bits, dev, host, nmse_of, odd_words, oob_of, placed, random_table, rms_of, words,
                          worst)

pytestmark = pytest.mark.gpu

RATIOS, PARITY = {}, {}
NAN, INF = float("nan"), float("inf")
DELAYS = [(0, 1), (0, 1, 2), (0, 3, 16), (0, 1, 2, 3)]


def tables(M, K, seed):
    """M random tables; the side branches a tenth of the main one"""
    F = np.stack([random_table(K, seed + 17 * m) for m in range(M)])
    F[1:] *= np.float32(0.1)
    return F.astype(np.complex64)


# ---------------------------------------------------------------------------------------------- 1. the untouched handle
@pytest.mark.parametrize("fout", ["cf32", "sc16"])
def test_untouched_handle_is_a_copy(product, fout):
    """n = 1 .. 257 behind a history of 16 samples, from and to even and odd sample offsets: load in[lead + i], convert, store, nothing
    else written; NaN payloads and -0.0 kept"""
    torch = _torch()
    out16 = fout == "sc16"
    d = product.mpd(3, (0, 3, 16), 5, 7, 1.0, 1.0, output_format=fout)
    lead = d.lead
    assert lead == 16
    src = odd_words(lead + 257, seed=11)
    clips = 0
    for shift_in in (0, 1):
        for shift_out in (0, 1):
            x = placed(src, shift_in)
            total = sum(n + 4 for n in range(1, 258)) + 4
            if out16:
                dst = torch.full((total, 2), SENTINEL, dtype=torch.int16, device="cuda")
            else:
                dst = torch.zeros(total, dtype=torch.complex64, device="cuda")
                torch.view_as_real(dst).view(torch.int32).fill_(SENTINEL_WORD)
            at, cur = [], 2
            for n in range(1, 258):
                cur += (cur + shift_out) % 2
                y = d.execute(x[:lead + n], out=dst[cur:])
                assert int(y.shape[0]) == n
                at.append(cur)
                cur += n + 2
            got = host(dst) if out16 else words(dst)
            mask = np.ones(len(got), bool)
            for n, a in zip(range(1, 258), at):
                mask[a:a + n] = False
                want = src[lead:lead + n]
                if out16:
                    assert np.array_equal(got[a:a + n], q16.quantise_iq(want)), (n, shift_in, shift_out)
                    clips += q16.clipped_samples(want)
                else:
                    assert np.array_equal(got[a:a + n].view(np.uint32), bits(want)), (n, shift_in, shift_out)
            assert np.all(got[mask] == (SENTINEL if out16 else SENTINEL_WORD)), "written outside the output"
    assert d.clipped() == clips and (clips > 0) == out16
    st = d.read()
    assert st["updates"] == 0 and np.all(st["F"][0] == 1) and not st["F"][1:].any() and not st["sums"].any() and st["rows"] == 0
    assert st["c"][0, 0] == 1 and np.count_nonzero(st["c"]) == 1
    d.close()


@pytest.mark.parametrize("gain", [1.0, 0.5])
@pytest.mark.parametrize("delays", [(0, 3), (0, 16)], ids=["lead3", "lead16"])
@pytest.mark.parametrize("fout", ["cf32", "sc16"])
def test_untouched_copy_from_either_parity(product, fout, delays, gain):
    """The untouched handle with branches copies from in + lead, the pair parity taken from that address: an odd lead flips it, so odd
    and even leads meet x at even and odd elements of a larger tensor, around one workgroup's 512 samples, to even and odd offsets.
    cf32: gain * x[lead:] exactly (gain 1: bit for bit, NaN payloads and -0.0 kept; 0.5 on finite normal values is exact);
    sc16: the quantiser's model of the same, the clip count with it; nothing written in front of or behind the output."""
    torch = _torch()
    out16 = fout == "sc16"
    d = product.mpd(2, delays, 5, 7, 1.0, 1.0, gain=gain, output_format=fout)
    lead, sizes = d.lead, (1, 2, 511, 512, 513)
    assert lead == delays[-1]
    if gain == 1.0:
        src = odd_words(lead + 513, seed=23)
    else:
        rng = np.random.RandomState(29)
        src = (1.5 * (rng.standard_normal(lead + 513) + 1j * rng.standard_normal(lead + 513))).astype(np.complex64)
    scaled = src if gain == 1.0 else (np.float32(gain) * src).astype(np.complex64)
    clips = 0
    for shift_in in (0, 1):
        x = placed(src, shift_in)
        for shift_out in (0, 1):
            total = sum(n + 4 for n in sizes) + 4
            if out16:
                dst = torch.full((total, 2), SENTINEL, dtype=torch.int16, device="cuda")
            else:
                dst = torch.zeros(total, dtype=torch.complex64, device="cuda")
                torch.view_as_real(dst).view(torch.int32).fill_(SENTINEL_WORD)
            at, cur = [], 2
            for n in sizes:
                cur += (cur + shift_out) % 2
                assert int(d.execute(x[:lead + n], out=dst[cur:]).shape[0]) == n
                at.append(cur)
                cur += n + 2
            got = host(dst) if out16 else words(dst)
            mask = np.ones(len(got), bool)
            for n, a in zip(sizes, at):
                mask[a:a + n] = False
                want = scaled[lead:lead + n]
                if out16:
                    assert np.array_equal(got[a:a + n], q16.quantise_iq(want)), (n, shift_in, shift_out)
                    clips += q16.clipped_samples(want)
                else:
                    assert np.array_equal(got[a:a + n].view(np.uint32), bits(want)), (n, shift_in, shift_out)
            assert np.all(got[mask] == (SENTINEL if out16 else SENTINEL_WORD)), "written outside the output"
    assert d.clipped() == clips and (clips > 0) == out16
    d.close()


# ---------------------------------------------------------------------------------------------- 2. one branch is dpd
@pytest.mark.parametrize("fout", ["cf32", "sc16"])
@pytest.mark.parametrize("log2", [5, 10])
def test_one_branch_equals_dpd(product, log2, fout):
    K, fs = 1 << log2, 0.75
    F, x = random_table(K, seed=log2), amplitudes(K, fs, 20000, seed=7)
    for gain in (1.0, 1.6):
        a = product.dpd(log2, fs, 1.0, gain=gain, output_format=fout)
        b = product.mpd(1, (0,), 5, log2, fs, 1.0, gain=gain, output_format=fout)
        assert b.lead == 0
        a.set_table(F); b.set_tables(F[None])
        for shift in (0, 1):
            ya, yb = host(a.execute(placed(x, shift))), host(b.execute(placed(x, shift)))
            assert np.array_equal(ya, yb) if fout == "sc16" else np.array_equal(bits(ya), bits(yb)), (gain, shift)
        assert a.clipped() == b.clipped() and (b.clipped() > 0) == (fout == "sc16")                # (ten times full scale clips at either gain)
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 3. apply against the model
@pytest.mark.parametrize("n", [1, 255, 4099])
@pytest.mark.parametrize("delays", DELAYS, ids=[str(len(d)) + "_" + str(d[-1]) for d in DELAYS])
def test_apply_against_the_model(product, delays, n):
    M, log2, fs = len(delays), 7, 0.75
    K, lead = 1 << log2, delays[-1]
    F = tables(M, K, seed=M + lead)
    rng = np.random.RandomState(n + lead)
    amp = fs * 10.0 ** rng.uniform(-3.0, 0.1, lead + n)                                    # 1e-3 of full scale to beyond it
    amp[:min(len(amp), K + 3)] = (np.arange(K + 3) * (fs / K))[:min(len(amp), K + 3)]      # every interval edge, and beyond the table
    rng.shuffle(amp)
    x = (amp * np.exp(2j * np.pi * rng.uniform(0, 1, len(amp)))).astype(np.complex64)
    tag = "apply_worst_fraction_M%d_lead%d" % (M, lead)
    for gain in (1.0, 0.37):
        d = product.mpd(M, delays, 5, log2, fs, 1.0, gain=gain)
        d.set_tables(F)
        assert np.array_equal(bits(d.read()["F"].reshape(-1)), bits(F.reshape(-1)))
        want, bound = model.apply(F, x, delays, log2, fs, gain)
        for shift in (0, 1):
            got = host(d.execute(placed(x, shift)))
            assert got.shape == (n,)
            w = worst(got, want, bound)
            RATIOS[tag] = max(RATIOS.get(tag, 0.0), w)
            print("mpd apply, M = %d, lead %d, n = %d, gain %.2f: worst error is %.3f of the rounding bound" % (M, lead, n, gain, w))
            assert w <= 1.0
        d.close()


# ---------------------------------------------------------------------------------------------- 4. cuts and formats
@pytest.mark.parametrize("delays", [(0, 1, 2), (0, 3, 16)], ids=["lead2", "lead16"])
def test_cuts_and_formats(product, delays):
    """pieces of 1 .. 257 samples that carry their leads are the bits of one call; sc16 is Q of cf32; the clip count is the model's;
    NaN and infinity come out not finite in the lead + 1 outputs they reach and disturb nothing else"""
    torch = _torch()
    M, log2, fs, lead = len(delays), 7, 0.75, delays[-1]
    F = tables(M, 1 << log2, seed=3)
    x = amplitudes(1 << log2, fs, lead + 33153 - (128 + 4), seed=100 + lead)               # 33153 = 1 + 2 + ... + 257
    n = len(x) - lead
    assert n == 33153
    kw = dict(branches=M, delays=delays, order=5, table_log2=log2, full_scale=fs, target_gain=1.0, gain=1.6)      # the largest leave the int16 range
    f32, s16 = product.mpd(**kw), product.mpd(output_format="sc16", **kw)
    f32.set_tables(F); s16.set_tables(F)
    xd = placed(x, 1)
    one = f32.execute(xd)
    yf = host(one)
    ys = host(s16.execute(xd))
    assert ys.dtype == np.int16 and np.array_equal(ys, q16.quantise_iq(yf))
    clips = q16.clipped_samples(yf)
    assert s16.clipped() == clips and 0 < clips < n and f32.clipped() == 0
    want, bound = model.apply(F, x, delays, log2, fs, 1.6)
    assert worst(yf, want, bound) <= 1.0
    pieces = torch.zeros(n, dtype=torch.complex64, device="cuda")
    pieces16 = torch.zeros((n, 2), dtype=torch.int16, device="cuda")
    at = 0
    for k in range(1, 258):
        f32.execute(xd[at:at + lead + k], out=pieces[at:])
        s16.execute(xd[at:at + lead + k], out=pieces16[at:])
        at += k
    assert at == n and np.array_equal(words(pieces), words(one)) and np.array_equal(host(pieces16), ys)
    assert s16.clipped(reset=True) == 2 * clips and s16.clipped() == 0
    xs = x.copy()
    bad = np.array([lead, lead + 77, lead + 1000, len(x) - 1 - lead])
    xs[bad] = np.array([NAN, complex(0, INF), complex(NAN, -INF), -INF], np.complex64)
    gs = host(f32.execute(dev(xs)))
    touched = np.zeros(n, bool)
    for b in bad:
        for dl in delays:
            touched[b - lead + dl] = True
        assert not (np.isfinite(gs[b - lead].real) and np.isfinite(gs[b - lead].imag))
    assert np.array_equal(bits(gs[~touched]), bits(yf[~touched]))
    f32.close(); s16.close()


# ---------------------------------------------------------------------------------------------- 5. the sums
def memory_feedback(n, fs, seed, spoil=True):
    """(u, z): a drive up to 1.1 full_scale, a compressing three-tap amplifier with AM/PM and a little noise; with `spoil`, one sample of
    every bad kind in u and in z (NaN, infinity, over range)"""
    rng = np.random.RandomState(seed)
    u = (rng.uniform(0, 1.1 * fs, n) * np.exp(2j * np.pi * rng.uniform(0, 1, n))).astype(np.complex64)
    v = u.astype(np.complex128)
    t = (np.abs(v) / fs) ** 2
    a = v * (1.0 + t) ** -0.5 * np.exp(-0.4j * t)
    z = a.copy()
    z[1:] += 0.08 * np.exp(0.7j) * a[:-1]
    z[2:] -= 0.03 * a[:-2]
    z = (z + 1e-3 * fs * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    if spoil and n > 40:
        at = rng.choice(np.arange(20, n), 12, replace=False)
        u[at[0]], u[at[1]], u[at[2]], u[at[3]], u[at[4]] = NAN, complex(0, NAN), INF, 3e30, 2.5 * 2.0 ** model.constants(7, fs, 1.0)[3]
        z[at[5]], z[at[6]], z[at[7]], z[at[8]], z[at[9]] = NAN, complex(0, INF), complex(-INF, 1), 1.2 * 2.0 ** model.constants(7, fs, 1.0)[3], 3e30
    return u, z


def same_sums(d, m):
    st = d.read()
    want = m.sums()
    assert np.array_equal(st["sums"], want), np.nonzero((st["sums"] != want).any(axis=1))[0][:8]
    assert (st["rows"], st["skipped"], st["updates"], st["degenerate"]) == (m.rows, m.skipped, m.updates, m.degenerate)
    return st


SHAPES = [((0, 3, 16), 5), ((0, 1, 2, 3), 5), ((0,), 1)]


@pytest.mark.parametrize("size", ["lead+1", "257", "70001", "beyond the grid"])
@pytest.mark.parametrize("delays,P", SHAPES, ids=["L15_lead16", "L20_lead3", "L1"])
def test_sums_equal_the_model(product, delays, P, size):
    """('beyond the grid': one tile more than the capped grid has workgroups, so the first workgroup takes a second tile)"""
    M, fs, lead = len(delays), 0.75, delays[-1]
    n = {"lead+1": lead + 1, "257": 257, "70001": 70001, "beyond the grid": lead + 256 * product.MPD_MAX_WGS + 77}[size]
    kw = dict(branches=M, delays=delays, order=P, table_log2=7, full_scale=fs, target_gain=1.0)
    d, m = product.mpd(**kw), model.Model(**kw)
    u, z = memory_feedback(n, fs, seed=n + P)
    assert d.measure(placed(u, 1), placed(z, 0)) == n - lead and m.measure(u, z)
    st = same_sums(d, m)
    assert st["rows"] + st["skipped"] == n - lead and not st["sums"][np.cumsum([0] + list(range(M * P + 1, 1, -1))), 1].any()      # the diagonal is real
    if n > 1000:
        assert st["skipped"] >= 10 and st["rows"] > 0.8 * n and st["Suu"] > 0
        # a bad z[i] drops the rows i + delay[m]; the same calls in another order give the same integers
        ud, zd = dev(u), dev(z)
        cuts = [(0, 1000), (1000 - lead, 40000 + 1), (40001 - lead, n)]
        mc = model.Model(**kw)
        for order in ([0, 1, 2], [2, 0, 1]):
            d.reset()
            for i in order:
                a, b = cuts[i]
                d.measure(ud[a:b], zd[a:b])
                if order[0] == 0:
                    mc.measure(u[a:b], z[a:b])
            same_sums(d, mc)
        same_sums(d, m)                                                                     # cuts that keep the same rows: the bits of one call
    d.close()


# ---------------------------------------------------------------------------------------------- 6. the update
def host_amplifier(u, fs):
    """a made-up amplifier with memory, float64 on the host: compression and AM/PM on three taps"""
    v = u.astype(np.complex128)
    t = (np.abs(v) / (0.8 * fs)) ** 2
    a = 0.9 * v * (1.0 + t * t) ** -0.25 * np.exp(0.3j * t / (1.0 + t))
    z = a.copy()
    z[1:] += 0.1 * np.exp(0.5j) * a[:-1]
    z[3:] -= 0.04 * np.exp(-0.3j) * a[:-3]
    return z.astype(np.complex64)


def same_solution(d, m):
    st = same_sums(d, m)
    assert np.array_equal(st["c"].view(np.uint64), m.coefficients().view(np.uint64)), (st["c"], m.coefficients())
    assert np.float64(st["res"]).view(np.uint64) == np.float64(m.res).view(np.uint64), (st["res"], m.res)
    assert np.array_equal(bits(st["F"].reshape(-1)), bits(m.F.reshape(-1))), np.nonzero(bits(st["F"].reshape(-1)) != bits(m.F.reshape(-1)))[0][:8]
    return st


@pytest.mark.parametrize("delays,P,log2,forget", [((0, 1, 3), 5, 7, 0), ((0, 1, 3), 5, 7, 2), ((0, 1, 2, 3), 5, 9, 2), ((0, 16), 3, 10, 0), ((0,), 1, 5, 0)],
                         ids=["L15", "L15_forget2", "L20_K512_forget2", "L6_K1024", "L1_K32"])
def test_solution_after_updates_equals_the_model(product, delays, P, log2, forget):
    fs, g0, M, lead = 0.75, 0.8, len(delays), delays[-1]
    kw = dict(branches=M, delays=delays, order=P, table_log2=log2, full_scale=fs, target_gain=g0, min_rows=500, forget_shift=forget)
    d, m = product.mpd(**kw), model.Model(**kw)
    # too few rows, then an all-zero record: degenerate, the tables stay
    rng = np.random.RandomState(log2 + forget)
    few = (0.2 * (rng.standard_normal(lead + 499) + 1j * rng.standard_normal(lead + 499))).astype(np.complex64)
    d.measure(dev(few), dev(few)); m.measure(few, few)
    d.update(); m.update()
    st = same_solution(d, m)
    assert st["degenerate"] == 1 and st["updates"] == 1 and np.all(st["F"][0] == 1) and not st["F"][1:].any()
    d.reset(); m.reset()
    zeros = np.zeros(lead + 600, np.complex64)
    d.measure(dev(zeros), dev(zeros)); m.measure(zeros, zeros)
    d.update(); m.update()
    st = same_solution(d, m)
    assert st["degenerate"] == 1 and st["rows"] == 600 >> forget and np.all(st["F"][0] == 1)
    d.reset(); m.reset()
    n = 20000
    x = (rng.uniform(0.02, 0.7, lead + n) * fs * np.exp(2j * np.pi * rng.uniform(0, 1, lead + n))).astype(np.complex64)
    xd = dev(x)
    for r in range(3):
        u = host(d.execute(xd))
        if r == 0:
            assert np.array_equal(bits(u), bits(x[lead:]))
        z = host_amplifier(u, fs)
        d.measure(dev(u), dev(z)); assert m.measure(u, z)
        d.update(); m.update()
        st = same_solution(d, m)                                                            # (behind the shift)
        assert st["updates"] == r + 1 and st["degenerate"] == 0 and st["skipped"] == 0
        if r in (0, 2):                                                                     # what execute now does is the model's tables applied
            want, bound = model.apply(m.F, x, delays, log2, fs)
            assert worst(host(d.execute(xd)), want, bound) <= 1.0
    if {1, 3} <= set(delays):                                                               # the branches cover the amplifier's taps
        y = host_amplifier(host(d.execute(xd)), fs)[lead:]
        y0 = host_amplifier(x[lead:], fs)[lead:]
        ref = g0 * x[2 * lead:].astype(np.complex128)
        print("mpd update, L = %d: NMSE %.1f -> %.1f dB; res / Suu %.2e" % (M * P, model.nmse_db(y0, ref), model.nmse_db(y, ref), st["res"] / max(st["Suu"], 1)))
        assert model.nmse_db(y, ref) < model.nmse_db(y0, ref) - 10.0
    d.reset(); m.reset()
    st = same_solution(d, m)
    assert np.all(st["F"][0] == 1) and np.array_equal(bits(host(d.execute(xd))), bits(x[lead:]))
    d.close()


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_on_the_device(product):
    torch = _torch()
    L, EINVAL, OK = product.lib(), product.MCRX_EINVAL, product.MCRX_OK
    n, lead = 4096, 16
    buf = torch.zeros(4 * n, dtype=torch.complex64, device="cuda")
    torch.view_as_real(buf).view(torch.int32).fill_(SENTINEL_WORD)
    keep = buf.clone()
    p = buf.data_ptr()
    for fout in ("cf32", "sc16"):
        d = product.mpd(3, (0, 3, lead), 5, 7, 1.0, 1.0, output_format=fout)
        d.set_tables(tables(3, 128, seed=1))
        so = 4 if fout == "sc16" else 8

        def call(a, b, count=n):
            return L.mcrx_hip_mpd_execute_device(d._h, C.c_void_p(a) if a else None, count, C.c_void_p(b) if b else None, None)

        def measure(a, b, count=n):
            return L.mcrx_hip_mpd_measure_device(d._h, C.c_void_p(a) if a else None, C.c_void_p(b) if b else None, count, None)
        far = p + 16 * n
        assert call(None, far) == EINVAL and call(p, None) == EINVAL
        assert call(p + 4, far) == EINVAL and call(p, far + so // 2) == EINVAL             # half a sample
        assert call(p, p) == EINVAL                                                         # in place: never
        assert call(p, p + so) == EINVAL and call(p + 8, p) == EINVAL
        assert call(p, p + 8 * (n + lead) - so) == EINVAL                                   # the output's first sample on the input's last
        assert call(p + so * n - 8, p) == EINVAL                                            # the input's first sample on the output's last
        assert call(p, far, (1 << 32) - lead + 1) == EINVAL and b"lead" in L.mcrx_hip_mpd_last_error()
        assert measure(None, p) == EINVAL and measure(p, None) == EINVAL and measure(p + 4, p) == EINVAL and measure(p, p + 4) == EINVAL
        most = 1 << product.MPD_GUARD_LOG2
        assert measure(p, p, most + lead + 1) == EINVAL and b"2^26" in L.mcrx_hip_mpd_last_error()
        assert measure(p, p, (1 << 32) + 1) == EINVAL
        assert L.mcrx_hip_mpd_set_tables(d._h, None, None) == EINVAL
        bad = tables(3, 128, seed=2)
        bad[2, 5] = complex(1.0, NAN)
        with pytest.raises(ValueError):
            d.set_tables(bad)
        with pytest.raises(ValueError):
            d.set_tables(bad[:2])
        with pytest.raises(ValueError):
            d.execute(buf[:lead - 1])
        with pytest.raises(ValueError):
            d.execute(buf[:n], out=torch.view_as_real(buf).view(torch.int16).view(-1, 2)[2:] if fout == "sc16" else buf[1:])
        with pytest.raises(ValueError):
            d.measure(buf[:n], buf[:n - 1])
        with pytest.raises(TypeError):
            d.execute(buf.real)
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(buf).view(torch.int32), torch.view_as_real(keep).view(torch.int32)), fout
        st = d.read()
        assert d.clipped() == 0 and not st["sums"].any() and st["skipped"] == 0 and st["rows"] == 0
        # the guard counts rows: 5 offered, then a call that would pass 2^26 measures nothing and leaves the count as it was
        good = torch.full((lead + 9,), 0.25, dtype=torch.complex64, device="cuda")
        assert d.measure(good[:lead + 5], good[:lead + 5]) == 5
        assert measure(p, p, most - 4 + lead) == EINVAL
        assert d.read()["rows"] == 5
        assert d.measure(good[5:], good[5:]) == 4 and d.read()["rows"] == 9
        # what is allowed: adjacent ranges, nothing to do, an empty output, u and z the same buffer, n <= lead measures nothing
        assert call(p, p + 8 * (n + lead)) == OK and call(p + so * n, p) == OK and call(p, p, 0) == OK and measure(p, p, 0) == OK
        assert measure(p, p, lead) == OK and d.read()["rows"] == 9
        assert int(d.execute(buf[:lead]).shape[0]) == 0
        torch.cuda.synchronize()
        buf.copy_(keep)
        d.close()
    with pytest.raises(ValueError):
        product.mpd(2, (0, 1), full_scale=1.0, target_gain=1.0, output_format="sc16").learn(buf[:n], None)


# ---------------------------------------------------------------------------------------------- 8. the closed loop
class MemoryAmplifier(object):
    """the three-branch amplifier of mpd_model.SEVERITY: three rfchain amplifier handles on u[i], u[i-1], u[i-2], shifted and summed with
    torch; zeros in front of the stream"""

    def __init__(self, product, rms):
        v = model.SEVERITY
        self.amps = [product.rfchain(amplifier=dict(sat=product.rfchain_backoff(ibo, rms), smooth=v["amp_smooth"], gain=v["amp_gain"], ampm_deg=deg))
                     for ibo, deg in zip(v["amp_ibo_db"], v["amp_ampm_deg"])]
        self.weights = [complex(w) for w in v["amp_weights"]]

    def execute(self, u, first_sample=0, stream=None):
        n = int(u.numel())
        z = self.amps[0].execute(u, first_sample, stream=stream) * self.weights[0]
        for b in (1, 2):
            z[b:] += self.amps[b].execute(u, first_sample, stream=stream)[:n - b] * self.weights[b]
        return z

    def close(self):
        for a in self.amps:
            a.close()


def test_closed_loop_on_the_device(product, oracle):
    """multichanneltx -> cfr -> predistorter -> the three-branch amplifier, three rounds of mpd(M = 3, P = 5, K = 128) and three of dpd on
    the same amplifier, at mpd_model.SEVERITY.  Asserted: mpd's NMSE is better than dpd's by what tests/test_mpd.py measured with the
    exact models on the oracle's stream less 6 dB (27.23 - 6 = 21.23 dB); mpd's power at |f| > 0.32 is not worse than dpd's by more
    than 1 dB; behind mpd all 24 frames are valid on the GPU receiver and on the oracle, the bytes identical, the equalised symbols
    within 1e-3 (the measured figure: PARITY, printed by the last test)."""
    from test_gpu_parity import match_frames, relerr, relerr_elem
    torch = _torch()
    s, v = cfr_model.SEVERITY, model.SEVERITY
    N, nf = s["N"], s["frames"]
    tx = product.multichanneltx(N, s["M"], s["cp"], s["taper"])
    iq, sent = tx.generate(nf, s["payload_len"], seed=77 + N)
    tx.close()
    rms = rms_of(torch, iq)
    h = product.cfr_lowpass(s["half_len"], s["cutoff"], s["beta"])
    cf = product.cfr(float(np.float32(product.cfr_threshold(s["papr_db"], rms))), taps=h, passes=s["passes"])
    x = cf.execute(iq, pad=True)
    cf.close()
    peak = float(x.abs().max())
    amp = MemoryAmplifier(product, rms)
    fs, g0 = v["full_scale_over_peak"] * peak, v["amp_gain"]
    ref = x * g0
    y0 = amp.execute(x)
    dp = product.dpd(v["table_log2"], fs, g0)
    dp.learn(x, amp, v["rounds"])
    yd = amp.execute(dp.execute(x))
    mp = product.mpd(v["branches"], v["delays"], v["order"], v["table_log2"], fs, g0)
    mp.learn(x, amp, v["rounds"])
    y = amp.execute(mp.execute(x, pad=True))
    oob = [oob_of(torch, t, v["edge"]) for t in (y0, yd, y)]
    nmse = [nmse_of(torch, t, ref) for t in (y0, yd, y)]
    st, sd = mp.read(), dp.read()
    assert (st["updates"], st["degenerate"], st["skipped"]) == (v["rounds"], 0, 0) and sd["degenerate"] == 0
    print("mpd closed loop: %d samples; none / dpd / mpd: power at |f| > %.2f %.2f / %.2f / %.2f dB, NMSE %.2f / %.2f / %.2f dB; gain of mpd over dpd %.2f dB"
          % ((int(x.numel()), v["edge"]) + tuple(oob) + tuple(nmse) + (nmse[1] - nmse[2],)))
    assert nmse[1] - nmse[2] >= v["nmse_gain_db"]
    assert oob[2] <= oob[1] + v["oob_slack_db"]
    n = int(y.numel()) // (product.TILE * 2 * N) * (product.TILE * 2 * N)
    y = y[:n].contiguous()
    rx = product.multichannelrx(N, s["M"], s["cp"], s["taper"], max_payload_len=s["payload_len"])
    rx.Execute(y); rx.Flush()
    ora = oracle.MultiChannelRx(N, s["M"], s["cp"], s["taper"])
    ora.execute(np.ascontiguousarray(host(y)))
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
        assert bytes(fg.header) == bytes(fo.header) and bytes(fg.payload) == bytes(fo.payload)
        assert len(fg.framesyms) == len(fo.framesyms) > 0
        w, we = max(w, relerr(fg.framesyms, fo.framesyms)), max(we, relerr_elem(fg.framesyms, fo.framesyms))
    evm = [f.evm for f in rx.frames]
    rx.close(); amp.close(); dp.close(); mp.close()
    PARITY["severity"] = {"max_norm": w, "element_wise": we, "oob_db": oob, "nmse_db": nmse, "nmse_gain_over_dpd_db": nmse[1] - nmse[2],
                          "evm_db": [min(evm), max(evm)], "rows": st["rows"], "res_over_suu": st["res"] / st["Suu"]}
    print("mpd_parity: framesyms max-norm %.3e element-wise %.3e; EVM %.1f .. %.1f dB" % (w, we, min(evm), max(evm)))
    assert w <= 1e-3, w


def test_zz_print_mpd_figures():
    """(last of this file: the figures measured above as one JSON line each -- profiles/mpd_model.json and profiles/mpd_parity.json are
    such records; MPD_OUT / MPD_PARITY_OUT name files to write them to as well)"""
    for tag, rec, env in (("mpd_model", RATIOS, "MPD_OUT"), ("mpd_parity", PARITY, "MPD_PARITY_OUT")):
        line = json.dumps(rec, sort_keys=True)
        print(tag + " " + line)
        path = os.environ.get(env)
        if path:
            with open(path, "w") as f:
                f.write(line + "\n")
