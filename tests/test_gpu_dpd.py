"""Digital predistortion on the MI355X (mcrx_hip_dpd_*) against tests/dpd_model.py: the untouched handle is a copy bit for bit; the
apply within the rounding bound the model derives; sc16 is Q of cf32; the accumulators are the model's integers and the table after
updates the model's to the last bit; the closed loop at dpd_model.SEVERITY with the receiver and the oracle behind it; the two-carrier
case on the receiver's channel monitor; the refusals."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cfr_model
import dpd_model as model
import tx_sc16_model as q16

pytestmark = pytest.mark.gpu

SENTINEL, SENTINEL_WORD = 0x5A5B, 0x7FC05A5B
RATIOS, PARITY = {}, {}
NAN, INF = float("nan"), float("inf")


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def host(t):
    return t.cpu().numpy()


def dev(x):
    """complex64 host samples on the device, bit for bit (NaN payloads survive: the copy is of int32 words)"""
    torch = _torch()
    w = torch.from_numpy(np.ascontiguousarray(x, np.complex64).view(np.int32).copy()).cuda()
    return torch.view_as_complex(w.view(torch.float32).view(-1, 2))


def words(t):
    """the int32 words of a complex64 device tensor, on the host, as [n, 2]"""
    torch = _torch()
    return host(torch.view_as_real(t).view(torch.int32))


def bits(x):
    return np.ascontiguousarray(x, np.complex64).view(np.uint32).reshape(-1, 2)


def placed(x, shift):
    """the samples x on the device, beginning `shift` samples behind a 16-byte boundary"""
    torch = _torch()
    buf = torch.zeros(len(x) + 2, dtype=torch.complex64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[shift:shift + len(x)].copy_(dev(x))
    return buf[shift:shift + len(x)]


def odd_words(n, seed):
    """n samples of everything a copy must keep: normal values, NaNs with payloads (quiet, signalling, negative), -0.0, infinities,
    denormals"""
    rng = np.random.RandomState(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    w = x.view(np.uint32).reshape(-1, 2)
    special = np.array([0x7FC05A5B, 0xFFC00001, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x00000000], np.uint32)
    where = rng.rand(n, 2) < 0.15
    w[where] = special[rng.randint(0, len(special), int(where.sum()))]
    return w.reshape(-1).view(np.complex64).copy()


# ---------------------------------------------------------------------------------------------- 1. the untouched handle
@pytest.mark.parametrize("fout", ["cf32", "sc16"])
def test_untouched_handle_is_a_copy(product, fout):
    """n = 1 .. 257 from and to even and odd sample offsets (8-byte but not 16-byte aligned): load, convert, store, nothing else written"""
    torch = _torch()
    out16 = fout == "sc16"
    d = product.dpd(7, 1.0, 1.0, output_format=fout)
    src = odd_words(257 + 2, seed=11)
    clips = 0
    for shift_in in (0, 1):
        for shift_out in (0, 1):
            x = placed(src[:257], shift_in)
            total = sum(n + 4 for n in range(1, 258)) + 4
            if out16:
                dst = torch.full((total, 2), SENTINEL, dtype=torch.int16, device="cuda")
            else:
                dst = torch.zeros(total, dtype=torch.complex64, device="cuda")
                torch.view_as_real(dst).view(torch.int32).fill_(SENTINEL_WORD)
            at, cur = [], 2
            for n in range(1, 258):
                cur += (cur + shift_out) % 2                                # even or odd sample offset, as asked
                y = d.execute(x[:n], out=dst[cur:])
                assert int(y.shape[0]) == n
                at.append(cur)
                cur += n + 2
            got = host(dst) if out16 else words(dst)
            mask = np.ones(len(got), bool)
            for n, a in zip(range(1, 258), at):
                mask[a:a + n] = False
                if out16:
                    assert np.array_equal(got[a:a + n], q16.quantise_iq(src[:n])), (n, shift_in, shift_out)
                    clips += q16.clipped_samples(src[:n])
                else:
                    assert np.array_equal(got[a:a + n].view(np.uint32), bits(src[:n])), (n, shift_in, shift_out)
            assert np.all(got[mask] == (SENTINEL if out16 else SENTINEL_WORD)), "written outside the output"
    assert d.clipped() == clips and (clips > 0) == out16
    st = d.read()
    assert st["updates"] == 0 and np.all(st["F"] == 1) and not st["cnt"].any()
    d.close()


# ---------------------------------------------------------------------------------------------- 2. apply against the model
def random_table(K, seed):
    rng = np.random.RandomState(seed)
    return (1.0 + 0.3 * rng.standard_normal(K + 1) + 0.3j * rng.standard_normal(K + 1)).astype(np.complex64)


def amplitudes(K, fs, n, seed):
    """0, every bin edge, full_scale, ten times full_scale, and random ones up to 1.2 full_scale, at random phases"""
    rng = np.random.RandomState(seed)
    amp = np.concatenate([[0.0], np.arange(K + 1) * (fs / K), [fs, 10.0 * fs], rng.uniform(0, 1.2 * fs, n)])
    return (amp * np.exp(2j * np.pi * rng.uniform(0, 1, len(amp)))).astype(np.complex64)


def worst(got, want, bound):
    err = np.stack([np.abs(got.real.astype(np.float64) - want.real), np.abs(got.imag.astype(np.float64) - want.imag)], axis=-1)
    return float((err / bound).max())


@pytest.mark.parametrize("log2", [5, 10])
def test_apply_against_the_model(product, log2):
    torch = _torch()
    K, fs = 1 << log2, 0.75
    F = random_table(K, seed=log2)
    d = product.dpd(log2, fs, 1.0)
    d.set_table(F)
    assert np.array_equal(bits(d.read()["F"]), bits(F))
    x = amplitudes(K, fs, 33153 - (K + 4), seed=100 + log2)                 # 33153 = 1 + 2 + ... + 257
    assert len(x) == 33153
    want, bound = model.apply(F, x, log2, fs)
    one = d.execute(placed(x, 1))
    got = host(one)
    w = worst(got, want, bound)
    RATIOS["apply_worst_fraction_K%d" % K] = w
    print("dpd apply, K = %d: worst error is %.3f of the rounding bound; largest bound %.3e, largest |y| %.3f" % (K, w, float(bound.max()), float(np.abs(want).max())))
    assert w <= 1.0
    # with a gain
    dg = product.dpd(log2, fs, 1.0, gain=0.37)
    dg.set_table(F)
    wantg, boundg = model.apply(F, x, log2, fs, gain=0.37)
    assert worst(host(dg.execute(dev(x))), wantg, boundg) <= 1.0
    dg.close()
    # NaN and infinity in place: they come out not finite where they went in and disturb nothing else
    xs = x.copy()
    bad = np.array([0, 1, 77, 1000, 1001, len(x) - 1])
    xs[bad] = np.array([NAN, complex(0, NAN), INF, complex(1, -INF), complex(NAN, INF), -INF], np.complex64)
    gs = host(d.execute(dev(xs)))
    assert all(not (np.isfinite(v.real) and np.isfinite(v.imag)) for v in gs[bad])
    keep = np.ones(len(x), bool)
    keep[bad] = False
    assert np.array_equal(bits(gs[keep]), bits(got[keep]))
    # in place, and in pieces of 1 .. 257 samples: the bits of the one call
    work = dev(x).clone()
    assert d.execute(work, out=work).data_ptr() == work.data_ptr()
    assert np.array_equal(words(work), words(one))
    pieces = torch.zeros(len(x), dtype=torch.complex64, device="cuda")
    xd, at = dev(x), 0
    for n in range(1, 258):
        d.execute(xd[at:at + n], out=pieces[at:])
        at += n
    assert at == len(x) and np.array_equal(words(pieces), words(one))
    d.close()


# ---------------------------------------------------------------------------------------------- 3. sc16 is Q of cf32
@pytest.mark.parametrize("log2", [5, 10])
def test_sc16_is_q_of_cf32(product, log2):
    K, fs = 1 << log2, 0.75
    F, x = random_table(K, seed=log2), amplitudes(K, fs, 20000, seed=7)
    kw = dict(table_log2=log2, full_scale=fs, target_gain=1.0, gain=1.6)                    # the largest outputs leave the int16 range
    f32, s16 = product.dpd(**kw), product.dpd(output_format="sc16", **kw)
    f32.set_table(F); s16.set_table(F)
    yf = host(f32.execute(placed(x, 1)))
    ys = host(s16.execute(placed(x, 1)))
    assert ys.dtype == np.int16 and np.array_equal(ys, q16.quantise_iq(yf))
    clips = q16.clipped_samples(yf)
    assert s16.clipped() == clips and 0 < clips < len(x) and f32.clipped() == 0
    assert s16.clipped(reset=True) == clips and s16.clipped() == 0
    f32.close(); s16.close()


# ---------------------------------------------------------------------------------------------- 4. the accumulators
def feedback(n, fs, seed, one_bin=False):
    """(u, z): amplitudes up to 1.15 full_scale (so some leave the table), a compressing gain with AM/PM and a little noise"""
    rng = np.random.RandomState(seed)
    r = np.full(n, 0.4 * fs) if one_bin else rng.uniform(0, 1.15 * fs, n)
    u = (r * np.exp(2j * np.pi * rng.uniform(0, 1, n))).astype(np.complex64)
    t = (np.abs(u.astype(np.complex128)) / fs) ** 2
    z = u * (1.0 + t) ** -0.5 * np.exp(-0.4j * t) + 1e-3 * fs * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return u, z.astype(np.complex64)


def same_accumulators(d, m):
    st = d.read()
    cnt, sre, sim, suu = m.accumulators()
    for name, want in (("cnt", cnt), ("Sre", sre), ("Sim", sim), ("Suu", suu)):
        assert np.array_equal(st[name], want), (name, np.nonzero(st[name] != want)[0][:8])
    assert (st["skipped"], st["updates"], st["degenerate"]) == (m.skipped, m.updates, m.degenerate)
    return st


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097, 1049089])
def test_accumulators_equal_the_model(product, n):
    """(1 049 089 samples are 2049 workgroups' worth of pairs: one more than the capped grid, so lanes take a second pass)"""
    fs = 0.75
    d, m = product.dpd(7, fs, 1.0), model.Model(7, fs, 1.0)
    u, z = feedback(n, fs, seed=n)
    assert d.measure(placed(u, 1), placed(z, 0)) == n and m.measure(u, z)
    st = same_accumulators(d, m)
    assert int(st["cnt"].sum()) + st["skipped"] == n
    d.close()


def test_accumulators_edge_cases(product):
    """every sample in one bin; ineligible samples of each kind; pieces of 1 .. 257; the guard's refusal measures nothing"""
    torch = _torch()
    L, fs = product.lib(), 0.75
    for log2 in (5, 10):
        K = 1 << log2
        d, m = product.dpd(log2, fs, 1.0), model.Model(log2, fs, 1.0)
        u, z = feedback(5000, fs, seed=3, one_bin=True)
        d.measure(dev(u), dev(z)); m.measure(u, z)
        st = same_accumulators(d, m)
        assert np.count_nonzero(st["cnt"]) == 1 and st["cnt"].max() == 5000 and st["Suu"].max() > 0
        d.reset(); m.reset()
        assert not same_accumulators(d, m)["cnt"].any()
        # one of each kind among good ones: NaN and infinite u, u beyond the table, NaN and infinite z, |z| above 4 E
        u, z = feedback(999, fs, seed=4)
        u[10], u[11], u[12], u[13], u[14] = NAN, complex(0, NAN), INF, 3e30, 2.0 * fs
        z[20], z[21], z[22], z[23], z[24] = NAN, complex(0, INF), complex(-INF, 1), 4.0000005, complex(0, 3e30)
        d.measure(placed(u, 1), placed(z, 1)); m.measure(u, z)
        st = same_accumulators(d, m)
        assert st["skipped"] >= 10 and m.skipped == st["skipped"]
        d.reset(); m.reset()
        # pieces of 1 .. 257, u and z on different 16-byte phases: the integers of one call
        u, z = feedback(33153, fs, seed=5)
        ud, zd, at = placed(u, 0), placed(z, 1), 0
        for n in range(1, 258):
            d.measure(ud[at:at + n], zd[at:at + n])
            at += n
        m.measure(u, z)
        cut = same_accumulators(d, m)
        d.reset()
        d.measure(ud, zd)
        whole = d.read()
        assert all(np.array_equal(cut[k], whole[k]) for k in ("cnt", "Sre", "Sim", "Suu")) and cut["skipped"] == whole["skipped"]
        # the guard: 33153 samples offered; a call that would pass 2^28 is refused before a buffer is looked at, and measures nothing
        p = ud.data_ptr()
        most = 1 << product.DPD_GUARD_LOG2
        for count in (most - 33153 + 1, most, most + 1, 1 << 32):
            assert L.mcrx_hip_dpd_measure_device(d._h, C.c_void_p(p), C.c_void_p(p), count, None) == product.MCRX_EINVAL
        assert b"2^28" in L.mcrx_hip_dpd_last_error()
        d.reset()
        d.measure(ud[:5], zd[:5])
        assert L.mcrx_hip_dpd_measure_device(d._h, C.c_void_p(p), C.c_void_p(p), most - 4, None) == product.MCRX_EINVAL      # 5 + 2^28 - 4
        m.reset(); m.measure(u[:5], z[:5])
        same_accumulators(d, m)                                                             # the five samples, nothing of the refused call
        d.measure(ud[5:9], zd[5:9]); m.measure(u[5:9], z[5:9])                              # and the count is as before: this fits
        same_accumulators(d, m)
        d.close()


# ---------------------------------------------------------------------------------------------- 5. the table after updates
def odd_amplifier(u, fs):
    """a made-up amplifier with everything the update must get through: compression, a phase that turns past 90 degrees above 0.72 of full scale (so
    Sre goes negative there) and negative Sim throughout"""
    a = np.abs(u.astype(np.complex128)) / fs
    return (u * (0.9 / (1.0 + a * a)) * np.exp(-3.0j * a * a)).astype(np.complex64)


def gappy_drive(n, fs, seed):
    """amplitudes in 0.05 .. 0.35 and 0.5 .. 0.8 of full scale -- a gap between, nothing below, nothing above -- and a handful of lone
    samples in between so that min_count has bins to refuse"""
    rng = np.random.RandomState(seed)
    r = np.where(rng.rand(n) < 0.5, rng.uniform(0.05, 0.35, n), rng.uniform(0.5, 0.8, n))
    r[:12] = np.linspace(0.37, 0.48, 12)
    return (fs * r * np.exp(2j * np.pi * rng.uniform(0, 1, n))).astype(np.complex64)


@pytest.mark.parametrize("log2,forget", [(6, 0), (6, 2), (10, 2)])
def test_table_after_updates_equals_the_model(product, log2, forget):
    fs, g0, K = 0.75, 0.8, 1 << log2
    kw = dict(table_log2=log2, full_scale=fs, target_gain=g0, min_count=3, forget_shift=forget)
    d, m = product.dpd(**kw), model.Model(**kw)
    # no valid bin: degenerate, the table stays 1
    d.update(); m.update()
    st = same_accumulators(d, m)
    assert st["degenerate"] == 1 and np.all(st["F"] == 1)
    d.reset(); m.reset()
    x = gappy_drive(6000, fs, seed=log2 + forget)
    xd = dev(x)
    worst_ulp = 0
    for r in range(3):
        u = host(d.execute(xd))                                                             # (round 0: the copy)
        if r == 0:
            assert np.array_equal(bits(u), bits(x))
        z = odd_amplifier(u, fs)
        d.measure(dev(u), dev(z)); assert m.measure(u, z)
        if r == 0:
            pre = same_accumulators(d, m)
            valid = (pre["cnt"] >= 3) & (pre["Suu"] > 0)
            assert 0 < np.count_nonzero((pre["cnt"] > 0) & ~valid), "min_count refuses nothing"
            assert (pre["Sre"] < 0).any() and (pre["Sim"] < 0).any() and not valid[0] and not valid[K]
            gaps = np.nonzero(~valid)[0]
            assert ((gaps > np.nonzero(valid)[0].min()) & (gaps < np.nonzero(valid)[0].max())).any(), "no gap between valid bins"
        d.update(); m.update()
        st = same_accumulators(d, m)                                                        # (behind the shift)
        assert st["updates"] == r + 1 and st["degenerate"] == 0
        assert np.isfinite(st["F"].real).all() and np.isfinite(st["F"].imag).all()
        diff = np.abs(bits(st["F"]).astype(np.int64) - bits(m.F).astype(np.int64)).max()
        worst_ulp = max(worst_ulp, int(diff))
        assert np.array_equal(bits(st["F"]), bits(m.F)), (r, int(diff), np.nonzero(bits(st["F"]) != bits(m.F))[0][:8])
        if r in (0, 2):                                                                     # what execute now does is the model's table applied
            want, bound = model.apply(m.F, x, log2, fs)
            assert worst(host(d.execute(xd)), want, bound) <= 1.0
    RATIOS["table_worst_ulp_K%d_forget%d" % (K, forget)] = worst_ulp
    # reset between: an untouched handle again
    d.reset(); m.reset()
    st = same_accumulators(d, m)
    assert np.all(st["F"] == 1) and np.array_equal(bits(host(d.execute(xd))), bits(x))
    d.close()


# ---------------------------------------------------------------------------------------------- 6. the closed loop
def rms_of(torch, t):
    return float(torch.view_as_real(t).double().pow(2).sum().div(int(t.numel())).sqrt())


def oob_of(torch, t, edge):
    """cfr_model.oob_db with torch.fft on the device"""
    nfft = cfr_model.SPECTRUM_NFFT
    seg = t.to(torch.complex128).unfold(0, nfft, nfft // 2) * torch.hann_window(nfft, periodic=True, dtype=torch.float64, device=t.device)
    P = torch.fft.fft(seg, dim=1).abs().pow(2).mean(dim=0)
    f = torch.fft.fftfreq(nfft, device=t.device, dtype=torch.float64)
    return float(10.0 * torch.log10(P[f.abs() > edge].sum() / P.sum()))


def nmse_of(torch, y, ref):
    y, ref = y.to(torch.complex128), ref.to(torch.complex128)
    return float(10.0 * torch.log10((y - ref).abs().pow(2).sum() / ref.abs().pow(2).sum()))


def test_closed_loop_on_the_device(product, oracle):
    """multichanneltx -> cfr -> dpd -> rfchain (amplifier), measure, update, three rounds at dpd_model.SEVERITY: the two thresholds
    tests/test_dpd.py found on the oracle hold; then -> multichannelrx and the oracle's receiver on the same samples.  framesyms: held
    to the 1e-3 the sibling end-to-end tests assert, the deviation recorded (PARITY, printed by the last test)."""
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
    ampk = dict(sat=product.rfchain_backoff(v["amp_ibo_db"], rms), smooth=v["amp_smooth"], gain=v["amp_gain"], ampm_deg=v["amp_ampm_deg"])
    amp = product.rfchain(amplifier=ampk)
    assert peak < float(amp.config.amp_sat)                                                # cfr comes first: the peaks lie below saturation
    d = product.dpd(v["table_log2"], v["full_scale_over_peak"] * peak, v["amp_gain"])
    ref = x * v["amp_gain"]
    y0 = amp.execute(x)
    oob0, nmse0 = oob_of(torch, y0, v["edge"]), nmse_of(torch, y0, ref)
    d.learn(x, amp, v["rounds"])
    y = amp.execute(d.execute(x))
    oob1, nmse1 = oob_of(torch, y, v["edge"]), nmse_of(torch, y, ref)
    st = d.read()
    assert (st["updates"], st["degenerate"], st["skipped"]) == (v["rounds"], 0, 0)
    cfg = amp.config
    print("dpd closed loop: %d samples, peak / amp_sat %.3f; power at |f| > %.2f %.1f -> %.1f dB, NMSE %.1f -> %.1f dB"
          % (int(x.numel()), peak / float(cfg.amp_sat), v["edge"], oob0, oob1, nmse0, nmse1))
    assert oob0 - oob1 >= v["oob_gain_db"]
    assert nmse0 - nmse1 >= v["nmse_gain_db"]
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
    rx.close(); amp.close(); d.close()
    PARITY["severity"] = {"max_norm": w, "element_wise": we, "oob_db": [oob0, oob1], "nmse_db": [nmse0, nmse1], "evm_db": [min(evm), max(evm)],
                          "peak_over_sat": peak / float(cfg.amp_sat), "valid_bins": int(np.count_nonzero((st["cnt"] >= 8) & (st["Suu"] > 0)))}
    print("dpd_parity: framesyms max-norm %.3e element-wise %.3e; EVM %.1f .. %.1f dB" % (w, we, min(evm), max(evm)))
    assert w <= 1e-3, w


# ---------------------------------------------------------------------------------------------- 7. two carriers on the channel monitor
def test_two_carriers_on_the_monitor(product):
    """Channels 3 and 4 carry frames, no cfr, the back-off of tests/test_dpd.py's rule: three updates take off channels 2 and 5 at
    least what the exact model recorded on the oracle (dpd_model.TWO_CARRIER: 2.25 and 2.12 dB -- the bank's own skirt is the floor
    there), less the 3 dB the monitor's averaging and the fp32 path account for; the fifth-order products in channels 1 and 6, which no
    skirt hides, fall by 14.7 dB on the model and are held to the same margin."""
    from test_gpu_rfchain import carriers, levels_db
    torch = _torch()
    t = model.TWO_CARRIER
    x = carriers(product, t["first"], t["count"])
    rms, peak = rms_of(torch, x), float(x.abs().max())
    ibo = 0
    while peak > t["peak_over_sat"] * rms * 10.0 ** (ibo / 20.0):
        ibo += 1
    amp = product.rfchain(amplifier=dict(sat=product.rfchain_backoff(float(ibo), rms), smooth=t["amp_smooth"], ampm_deg=t["amp_ampm_deg"]))
    d = product.dpd(t["table_log2"], t["full_scale_over_peak"] * peak, 1.0)
    before, _ = levels_db(product, amp.execute(x))
    d.learn(x, amp, t["rounds"])
    after, frames = levels_db(product, amp.execute(d.execute(x)))
    clean, _ = levels_db(product, x)
    amp.close(); d.close()
    print("dpd two carriers on the monitor: back-off %d dB, peak / amp_sat %.3f" % (ibo, peak / (rms * 10.0 ** (ibo / 20.0))))
    for name, lv in (("no amplifier", clean), ("amplifier", before), ("dpd + amplifier", after)):
        print("dpd two carriers on the monitor, %-16s levels [dB] " % (name + ":") + " ".join("%.1f" % v for v in lv))
    fall = {c: float(before[c] - after[c]) for c in (1, 2, 5, 6)}
    print("dpd two carriers on the monitor: falls [dB] " + " ".join("ch %d %.2f" % (c, v) for c, v in sorted(fall.items())))
    RATIOS["two_carrier_fall_db"] = fall
    RATIOS["two_carrier_backoff_db"] = ibo
    assert frames == 2 * cfr_model.SEVERITY["frames"]
    for c in (2, 5):
        assert fall[c] >= t["recorded_db"][c] - 3.0, fall
    for c in (1, 6):
        assert fall[c] >= 14.7 - 3.0, fall


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_on_the_device(product):
    torch = _torch()
    L, EINVAL, OK = product.lib(), product.MCRX_EINVAL, product.MCRX_OK
    n = 4096
    buf = torch.zeros(4 * n, dtype=torch.complex64, device="cuda")
    torch.view_as_real(buf).view(torch.int32).fill_(SENTINEL_WORD)
    keep = buf.clone()
    p = buf.data_ptr()
    for fout in ("cf32", "sc16"):
        d = product.dpd(7, 1.0, 1.0, output_format=fout)
        d.set_table(random_table(128, seed=1))
        so = 4 if fout == "sc16" else 8

        def call(a, b, count=n):
            return L.mcrx_hip_dpd_execute_device(d._h, C.c_void_p(a) if a else None, count, C.c_void_p(b) if b else None, None)

        def measure(a, b, count=n):
            return L.mcrx_hip_dpd_measure_device(d._h, C.c_void_p(a) if a else None, C.c_void_p(b) if b else None, count, None)
        assert call(None, p) == EINVAL and call(p, None) == EINVAL
        assert call(p + 4, p + 16 * n) == EINVAL                        # d_in: half a sample
        assert call(p, p + 16 * n + so // 2) == EINVAL                  # d_out likewise
        assert call(p, p + so) == EINVAL and call(p + 8, p) == EINVAL   # overlapping, one sample apart either way
        assert call(p, p + 8 * n - so) == EINVAL                        # the output's first sample on the input's last
        assert call(p + so * n - 8, p) == EINVAL                        # the input's first sample on the output's last
        assert call(p, p + 16 * n, (1 << 32) + 1) == EINVAL
        if fout == "sc16":
            assert call(p, p) == EINVAL                                 # in place with unequal formats
        assert measure(None, p) == EINVAL and measure(p, None) == EINVAL and measure(p + 4, p) == EINVAL and measure(p, p + 4) == EINVAL
        assert L.mcrx_hip_dpd_set_table(d._h, None, None) == EINVAL
        bad = random_table(128, seed=2)
        bad[5] = complex(1.0, NAN)
        with pytest.raises(ValueError):
            d.set_table(bad)
        with pytest.raises(ValueError):
            d.set_table(bad[:100])
        assert L.mcrx_hip_dpd_last_error()
        with pytest.raises(ValueError):
            d.execute(buf[:n], out=torch.view_as_real(buf).view(torch.int16).view(-1, 2)[2:] if fout == "sc16" else buf[1:])
        with pytest.raises(ValueError):
            d.measure(buf[:n], buf[:n - 1])
        with pytest.raises(TypeError):
            d.execute(buf.real)
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(buf).view(torch.int32), torch.view_as_real(keep).view(torch.int32)), fout
        st = d.read()
        assert d.clipped() == 0 and not st["cnt"].any() and st["skipped"] == 0
        # what is allowed: adjacent ranges, nothing to do, an empty tensor, u and z the same buffer, in place with equal formats
        assert call(p, p + 8 * n) == OK and call(p + so * n, p) == OK and call(p, p, 0) == OK and measure(p, p, 0) == OK
        assert int(d.execute(buf[:0]).shape[0]) == 0
        if fout == "cf32":
            assert call(p, p) == OK
        torch.cuda.synchronize()
        buf.copy_(keep)
        d.close()
    with pytest.raises(ValueError):
        product.dpd(7, 1.0, 1.0, output_format="sc16").learn(buf[:n], None)


def test_zz_print_dpd_figures():
    """(last of this file: the figures measured above as one JSON line each -- profiles/dpd_model.json and profiles/dpd_parity.json are
    such records; DPD_OUT / DPD_PARITY_OUT name files to write them to as well)"""
    for tag, rec, env in (("dpd_model", RATIOS, "DPD_OUT"), ("dpd_parity", PARITY, "DPD_PARITY_OUT")):
        line = json.dumps(rec, sort_keys=True)
        print(tag + " " + line)
        path = os.environ.get(env)
        if path:
            with open(path, "w") as f:
                f.write(line + "\n")
