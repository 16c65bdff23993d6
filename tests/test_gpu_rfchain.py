"""RF front end on the GPU (mcrx_hip_rfchain_*): the stage-less builds against the codecs, every stage against
the float64 model of tests/rfchain_model.py, against itself cut into pieces, spans and in place, against the shared quantiser, the
refusals, where the image and the intermodulation land in a multichannelrx, and end to end against the oracle.

Bounds (stage_bounds below), per component, eps = 2^-24 (one fp32 rounding, relative), SC = 3e-7 (sincos_u32's error, the figure
tests/test_gpu_chanemu.py uses), |z| the model's input of the stage, e the bound carried in:
  mixer       four nested fmaf a component, every partial sum <= P = (|ar| + |ai| + |br| + |bi|) (|z| + sqrt2 e) + max|d|:
              e' = (|ar| + |ai| + |br| + |bi|) e + 4 eps P
  oscillator  a table row: S cosines (SC each) and S fmaf whose results are <= c S:  dTheta = c S (SC + S eps) turns; the line between
              two rows adds three roundings of values <= c S, the phase word 2^-33 turn:  dtheta = dTheta + 3 eps c S + 2^-33;
              the rotation turns the incoming error (a component of it <= sqrt2 e), its sine and cosine carry SC each and its
              product and fmaf one rounding each:  e' = sqrt2 e + |z| (2 pi dtheta + sqrt2 (SC + 2 eps))
  amplifier   t carries 3 roundings, q at most t's + 2.25 (p = 4), sqrtf(q) half of that + 1, the division + 1, G z + 1: 6 eps on
              |G z| <= g |z|; phi = ampm (t / (1 + t)) carries t's 3 + 2 + 1 = 6 eps of |ampm| turns and the phase word 2^-33; then the
              rotation's terms as above.  The stage is compressive (d|u| / d|z| <= g) and its phase moves by at most pi |ampm| g per
              unit of input error, so the incoming error grows by at most g (1 + pi |ampm|):
              e' = sqrt2 g (1 + pi |ampm|) e + g |z| (6 eps + [ampm != 0] (2 pi (6 eps |ampm| + 2^-33) + sqrt2 (SC + 2 eps)))
  gain        e' = |gain| (e + eps |u|)"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import chanemu_model
import rfchain_model as model
import tx_sc16_model as q16

pytestmark = pytest.mark.gpu

EPS, SC, SQ2 = 2.0 ** -24, 3e-7, math.sqrt(2.0)
SENTINEL = 0x5A5B
A_SAT = 0.4
MIXER = dict(alpha=None, beta=None, dc=0.01 - 0.02j)      # alpha, beta: rfchain_iq(1 dB, 5 degrees), filled in by mixer_kw
PN = dict(rms_deg=2.0, bandwidth=1e-3, log2_block=4, seed=0xC0FFEE0123456789)
N_MODEL = 4099
RATIOS, PARITY = {}, {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def mixer_kw(product, side="tx"):
    return dict(product.rfchain_iq(1.0, 5.0, side), dc=MIXER["dc"])


def chain_kw(product, mask, order="tx", p=2, ampm_deg=7.0, amp_gain=1.25, **more):
    kw = dict(order=order, **more)
    if mask & 1:
        kw["mixer"] = mixer_kw(product, order)
    if mask & 2:
        kw["phase_noise"] = dict(PN)
    if mask & 4:
        kw["amplifier"] = dict(sat=A_SAT, smooth=p, gain=amp_gain, ampm_deg=ampm_deg)
    return kw


_X = {}


def samples(n, seed=7):
    """amplitudes from 1e-3 A to 30 A (log-uniform), any phase: host complex64 and device; made once and left alone"""
    if (n, seed) not in _X:
        torch = _torch()
        rng = np.random.RandomState(seed)
        amp = A_SAT * 10.0 ** rng.uniform(-3.0, math.log10(30.0), n)
        amp[:4] = A_SAT * np.array([1e-3, 30.0, 1.0, 0.0])
        x = (amp * np.exp(2j * np.pi * rng.uniform(size=n))).astype(np.complex64)
        _X[(n, seed)] = (x, torch.from_numpy(x).cuda())
    return _X[(n, seed)]


def host(t):
    return t.cpu().numpy()


def bits(t):
    """the words of a cf32 or sc16 tensor, for bit-for-bit comparisons"""
    torch = _torch()
    return torch.view_as_real(t).contiguous().view(torch.int32) if t.dtype == torch.complex64 else t


def stage_bounds(cfg, ints, x, first_sample):
    """(model output, per-sample bound on each component of got - model): the module docstring's recursion along the model's stages"""
    z = np.asarray(x, np.complex128)
    e = np.zeros(len(z))
    for s in model.sequence(cfg):
        mag = np.abs(z)
        if s == model.MIXER:
            co = abs(cfg.alpha_re) + abs(cfg.alpha_im) + abs(cfg.beta_re) + abs(cfg.beta_im)
            P = co * (mag + SQ2 * e) + max(abs(cfg.dc_re), abs(cfg.dc_im))
            z, e = model.mixer(cfg, z), co * e + 4 * EPS * P
        elif s == model.OSCILLATOR:
            S, c = int(cfg.pn_sinusoids), ints[2]
            dth = c * S * (SC + S * EPS) + 3 * EPS * c * S + 2.0 ** -33
            th = model.theta(ints, int(cfg.pn_log2_block), chanemu_model.positions(first_sample, len(z)))
            z, e = model.oscillator(z, th), SQ2 * e + mag * (2 * np.pi * dth + SQ2 * (SC + 2 * EPS))
        else:
            g, am = abs(float(cfg.amp_gain)), abs(float(cfg.amp_ampm))
            own = 6 * EPS + ((2 * np.pi * (6 * EPS * am + 2.0 ** -33) + SQ2 * (SC + 2 * EPS)) if am else 0.0)
            z, e = model.amplifier(cfg, z), SQ2 * g * (1 + np.pi * am) * e + g * mag * own
    gain = abs(float(cfg.gain))
    return float(cfg.gain) * z, gain * (e + EPS * np.abs(z))


def worst_ratio(got, want, bound):
    d = np.asarray(got, np.complex128) - want
    tiny = np.finfo(np.float32).tiny                                    # (a zero sample has a zero bound: 0 <= 0)
    return float(np.max(np.maximum(np.abs(d.real), np.abs(d.imag)) / np.maximum(bound, tiny)))


# ---------------------------------------------------------------------------------------------- 1. passthrough
LENGTHS = [1, 2, 3, 511, 512, 513, 4099]


def special_floats(n, seed):
    """cf32 bit patterns of every kind: random words (NaN payloads, denormals, infinities among them), -0.0, +-inf, quiet and signalling NaN"""
    rng = np.random.RandomState(seed)
    w = rng.randint(0, 2 ** 32, size=2 * n, dtype=np.uint64).astype(np.uint32)
    fixed = np.array([0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0x7F800001, 0xFFC12345, 0x00000001, 0x807FFFFF], np.uint32)
    w[:min(len(fixed), 2 * n)] = fixed[:2 * n]
    return w.view(np.complex64)


@pytest.mark.parametrize("fin,fout", [("cf32", "cf32"), ("sc16", "cf32"), ("cf32", "sc16"), ("sc16", "sc16")])
def test_passthrough(product, fin, fout):
    """no stage on, gain 1: load, convert, store -- from aligned buffers and from buffers offset by one sample, at even and odd positions"""
    torch = _torch()
    rf = product.rfchain(input_format=fin, output_format=fout)
    assert rf.stages == 0 and (rf.input_format, rf.output_format) == (int(fin == "sc16"), int(fout == "sc16"))
    rng = np.random.RandomState(3)
    for n in LENGTHS + ([65536] if (fin, fout) == ("sc16", "sc16") else []):
        if fin == "sc16":
            xi = rng.randint(-32768, 32768, size=(n, 2)).astype(np.int16)
            if n == 65536:                                              # all 65536 values of each component
                xi[:, 0] = np.arange(-32768, 32768).astype(np.int16)
                xi[:, 1] = np.roll(xi[:, 0], 12345)
            want = (xi.astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64).reshape(-1) if fout == "cf32" else xi
        else:
            xi = special_floats(n, n)
            if fout == "sc16":
                with np.errstate(invalid="ignore"):
                    xi = (xi.view(np.float32) % np.float32(3.0) - np.float32(1.5)).view(np.complex64)
            if fout == "sc16":                                          # values around the range, NaN and infinities kept
                v = xi.view(np.float32).copy()
                v[:6] = [np.nan, np.inf, -np.inf, -0.0, 1.0, -1.0][:len(v)]
                xi = v.view(np.complex64)
            want = xi if fout == "cf32" else q16.quantise_iq(xi)
        for shift in (0, 1):
            for first in (0, 7):
                src = torch.zeros((n + 2, 2) if fin == "sc16" else (n + 2,), dtype=torch.int16 if fin == "sc16" else torch.complex64, device="cuda")
                if fin == "cf32":
                    torch.view_as_real(src).view(torch.int32)[shift:shift + n].copy_(torch.from_numpy(xi.view(np.int32).reshape(-1, 2)).cuda())
                else:
                    src[shift:shift + n].copy_(torch.from_numpy(xi).cuda())
                if fout == "sc16":
                    dst = torch.full((n + 3, 2), SENTINEL, dtype=torch.int16, device="cuda")
                else:
                    dst = torch.full((n + 3,), float("nan"), dtype=torch.complex64, device="cuda")
                    torch.view_as_real(dst).view(torch.int32).fill_(0x7FC05A5B)
                y = rf.execute(src[shift:shift + n], first_sample=first, out=dst[shift:])
                assert int(y.shape[0]) == n
                got = host(bits(dst))
                where = (fin, fout, n, shift, first)
                if fout == "cf32":
                    assert np.array_equal(got[shift:shift + n], np.ascontiguousarray(want).view(np.int32).reshape(-1, 2)), where
                    rest = np.concatenate([got[:shift], got[shift + n:]])
                    assert np.all(rest == 0x7FC05A5B), where
                else:
                    assert np.array_equal(got[shift:shift + n], want), where
                    assert np.all(np.concatenate([got[:shift], got[shift + n:]]) == SENTINEL), where
    if fin == "sc16":
        assert rf.clipped() == 0                                        # Q of an int16 times 2^-15 is that int16
    rf.close()
    rf.close()                                                          # twice is harmless


# ---------------------------------------------------------------------------------------------- 2. against the model
def model_cases():
    cases = []
    for order in ("tx", "rx"):
        cases.append(("mixer_%s" % order, 1, order, 2, 0.0))
        cases.append(("oscillator_%s" % order, 2, order, 2, 0.0))
        for mask in (4, 7):
            for p in (1, 2, 4):
                for ampm in (0.0, 7.0):
                    cases.append(("%s_%s_p%d_%s" % ("amplifier" if mask == 4 else "all", order, p, "ampm" if ampm else "noampm"), mask, order, p, ampm))
    return cases


@pytest.mark.parametrize("name,mask,order,p,ampm", model_cases(), ids=[c[0] for c in model_cases()])
def test_against_the_model(product, name, mask, order, p, ampm):
    x, d_x = samples(N_MODEL)
    first = 12345
    kw = chain_kw(product, mask, order, p, ampm, gain=0.8)
    rf = product.rfchain(**kw)
    got = host(rf.execute(d_x, first_sample=first))
    rf.close()
    cfg = product.rfchain_config(**kw)
    ints = product.rfchain_integers(cfg) if mask & 2 else None
    want, bound = stage_bounds(cfg, ints, x, first)
    assert np.allclose(want, model.apply(cfg, x, first, ints), rtol=0, atol=0)     # (the recursion walks the model itself)
    r = worst_ratio(got, want, bound)
    RATIOS[name] = r
    print("rfchain_model %s: worst fraction of the bound %.3f" % (name, r))
    assert float(np.abs(x).max()) >= 29.9 * A_SAT and 0 < float(np.abs(x[x != 0]).min()) <= 1.01e-3 * A_SAT
    assert r <= 1.0, r


@pytest.mark.parametrize("L", [1, 4, 10])
def test_phase_rows_against_the_model(product, L):
    kw = dict(phase_noise=dict(PN, log2_block=L, bandwidth=0.1 / (1 << L)))
    rf = product.rfchain(**kw)
    cfg = product.rfchain_config(**kw)
    ints = product.rfchain_integers(cfg)
    S, c = int(cfg.pn_sinusoids), ints[2]
    bound = c * S * (SC + S * EPS)
    worst = 0.0
    for first_row in (0, 2 ** 30 + 7, 2 ** (64 - L) - 300):             # the last: across the wrap of the 64-bit position
        got = host(rf.phase_rows(first_row, 1000)).astype(np.float64)
        rows = (np.arange(1000, dtype=np.uint64) + np.uint64(first_row)) & np.uint64(2 ** (64 - L) - 1)
        want = model.theta_rows(ints, L, rows)
        worst = max(worst, float(np.abs(got - want).max()))
        assert float(np.abs(want).max()) > 0.3 * c * math.sqrt(S)
    RATIOS["phase_rows_L%d" % L] = worst / bound
    print("rfchain_model phase_rows L=%d: worst |got - model| %.3e turns, bound %.3e" % (L, worst, bound))
    assert worst <= bound
    rf.close()


# ---------------------------------------------------------------------------------------------- 3. positions
@pytest.mark.parametrize("name,first", [("2^40", 2 ** 40 + 3), ("across_2^32", 2 ** 32 - 1001), ("across_2^64", 2 ** 64 - 1000)])
def test_far_positions(product, name, first):
    x, d_x = samples(2500, seed=9)
    kw = chain_kw(product, 7, "tx")
    rf = product.rfchain(**kw)
    cfg = product.rfchain_config(**kw)
    ints = product.rfchain_integers(cfg)
    got = host(rf.execute(d_x, first_sample=first))
    want, bound = stage_bounds(cfg, ints, x, first)
    r = worst_ratio(got, want, bound)
    RATIOS["position_" + name] = r
    print("rfchain_model at %s: worst fraction of the bound %.3f" % (name, r))
    assert r <= 1.0
    # ... and it is not the stream at position 0
    assert worst_ratio(got, model.apply(cfg, x, 0, ints), bound) > 100.0
    rf.close()


# ---------------------------------------------------------------------------------------------- 4. cuts, spans, in place
N_CUT = 5003


def cut_input(product, fin):
    torch = _torch()
    x, d_x = samples(N_CUT, seed=11)
    if fin == "sc16":
        pre = product.rfchain(gain=0.05, output_format="sc16")          # 30 A * 0.05 = 0.6 of full scale
        d_x = pre.execute(d_x).clone()
        pre.close()
    return d_x


@pytest.mark.parametrize("fin,fout", [("cf32", "cf32"), ("cf32", "sc16"), ("sc16", "sc16"), ("sc16", "cf32")])
def test_cuts_spans_and_in_place(product, fin, fout):
    torch = _torch()
    d_x = cut_input(product, fin)
    amp_gain = 4.0 if fout == "sc16" else 1.25                          # sc16 out: some samples clip (|u| <= 4 A = 1.6)
    first = 2 ** 40 + 1
    kw = chain_kw(product, 7, "rx", amp_gain=amp_gain, input_format=fin, output_format=fout)
    rf = product.rfchain(**kw)
    one = rf.execute(d_x, first_sample=first).clone()
    clips = rf.clipped(reset=True)
    assert (clips > 50) if fout == "sc16" else (clips == 0)
    # pieces of 1, 2, 3, 255, 256, 257 and the rest, the stream starting at an odd and at an even index
    for base in (first, first + 1):
        want = rf.execute(d_x, first_sample=base).clone()
        want_clips = rf.clipped(reset=True)
        if fout == "sc16":
            buf = torch.full((N_CUT + 8, 2), SENTINEL, dtype=torch.int16, device="cuda")
        else:
            buf = torch.full((N_CUT + 8,), float("nan"), dtype=torch.complex64, device="cuda")
        pos, starts = 0, []
        for size in (1, 2, 3, 255, 256, 257, N_CUT):
            end = min(pos + size, N_CUT)
            starts.append((base + pos) & 1)
            y = rf.execute(d_x[pos:end], first_sample=base + pos, out=buf[pos:])
            assert int(y.shape[0]) == end - pos
            pos = end
        assert pos == N_CUT and 0 in starts and 1 in starts
        assert torch.equal(bits(buf[:N_CUT]), bits(want))
        tail = buf[N_CUT:]
        assert bool((tail == SENTINEL).all()) if fout == "sc16" else bool(torch.isnan(tail.real).all())
        assert rf.clipped(reset=True) == want_clips                     # the pieces count what the one call counted
    # many spans: a table of 2 and of 4 rows (L = 4: spans of 16 and 48 samples)
    for rows in (2, 4):
        kw_s = dict(kw, phase_noise=dict(PN, table_rows=rows))
        rs = product.rfchain(**kw_s)
        assert torch.equal(bits(rs.execute(d_x, first_sample=first)), bits(one)), rows
        assert rs.clipped() == clips
        rs.close()
    # in place (equal formats); with unequal formats the class refuses it as the library does
    if fin == fout:
        work = d_x.clone()
        y = rf.execute(work, first_sample=first, out=work)
        assert y.data_ptr() == work.data_ptr() and torch.equal(bits(work), bits(one))
    rf.close()


def test_the_phase_table_grows_and_is_reused(product):
    """L = 1, the default table, from an odd position: 130 samples in the first allocation (67 rows), 5 000 that force the table to grow,
    130 again in the grown one -- each call the bits of a fresh handle's"""
    torch = _torch()
    x, d_x = samples(5000, seed=17)
    kw = dict(chain_kw(product, 7), phase_noise=dict(PN, log2_block=1, table_rows=0))
    rf = product.rfchain(**kw)
    for n in (130, 5000, 130):
        fresh = product.rfchain(**kw)
        got, want = rf.execute(d_x[:n], first_sample=1001), fresh.execute(d_x[:n], first_sample=1001)
        assert int(got.shape[0]) == n and torch.equal(bits(got), bits(want)), n
        fresh.close()
    assert not torch.equal(bits(got), bits(d_x[:130]))
    rf.close()


# ---------------------------------------------------------------------------------------------- 5. sc16 is Q of cf32
@pytest.mark.parametrize("mask", range(8))
def test_sc16_is_q_of_cf32(product, mask):
    torch = _torch()
    n = 4099
    rng = np.random.RandomState(21 + mask)
    x = (0.45 * (rng.randn(n) + 1j * rng.randn(n))).astype(np.complex64)
    x[[5, 100, 4000]] = [complex(np.nan, 0.1), complex(0.2, np.nan), complex(np.nan, np.nan)]
    x[[6, 7]] = [complex(np.inf, 0.0), complex(0.0, -np.inf)]
    d_x = torch.from_numpy(x).cuda()
    for order in ("tx", "rx"):
        kw = chain_kw(product, mask, order, amp_gain=2.7)               # amplifier on: |u| <= 2.7 A = 1.08
        cf, sc = product.rfchain(**kw), product.rfchain(output_format="sc16", **kw)
        y, i = host(cf.execute(d_x, first_sample=77)), host(sc.execute(d_x, first_sample=77))
        want = q16.clipped_samples(y)
        print("rfchain sc16 mask %d %s: %d of %d samples clip" % (mask, order, want, n))
        assert 100 <= want <= n // 2, want                              # some hundreds clip, most do not
        assert np.array_equal(i, q16.quantise_iq(y)), (mask, order)
        assert np.isnan(y.view(np.float32)).any()                       # NaN went through and is not counted
        assert cf.clipped() == 0
        assert sc.clipped() == want and sc.clipped(reset=True) == want and sc.clipped() == 0
        sc.execute(d_x, first_sample=77); sc.execute(d_x, first_sample=77)
        assert sc.clipped() == 2 * want                                 # it accumulates over calls
        cf.close(); sc.close()


# ---------------------------------------------------------------------------------------------- 6. refusals on the device
def test_refusals_on_the_device(product):
    torch = _torch()
    L, EINVAL, OK = product.lib(), product.MCRX_EINVAL, product.MCRX_OK
    n = 4096
    buf = torch.full((4 * n,), float("nan"), dtype=torch.complex64, device="cuda")
    torch.view_as_real(buf).view(torch.int32).fill_(0x7FC05A5B)
    keep = buf.clone()
    p = buf.data_ptr()
    for fin, fout in (("cf32", "cf32"), ("cf32", "sc16"), ("sc16", "cf32"), ("sc16", "sc16")):
        rf = product.rfchain(input_format=fin, output_format=fout, **chain_kw(product, 7))
        si, so = (4 if fin == "sc16" else 8), (4 if fout == "sc16" else 8)

        def call(a, b, count=n):
            return L.mcrx_hip_rfchain_execute_device(rf._h, C.c_void_p(a) if a else None, 5, count, C.c_void_p(b) if b else None, None)
        assert call(None, p) == EINVAL and call(p, None) == EINVAL
        assert call(p + si // 2, p + 16 * n) == EINVAL                  # d_in: one sample of its format
        assert call(p, p + 16 * n + so // 2) == EINVAL                  # d_out likewise
        assert call(p, p + si * n - so) == EINVAL                       # the output's first sample on the input's last
        assert call(p + so * n - si, p) == EINVAL                       # the input's first sample on the output's last
        assert call(p + si, p) == EINVAL and call(p, p + so) == EINVAL  # shifted by one sample: overlapping, not in place
        assert call(p, p, (1 << 32) + 1) == EINVAL                      # too long
        if fin != fout:
            assert call(p, p) == EINVAL                                 # in place with unequal formats
            with pytest.raises(ValueError):
                x = torch.view_as_real(buf).view(torch.int16).view(-1, 2)[:n] if fin == "sc16" else buf[:n]
                o = torch.view_as_real(buf).view(torch.int16).view(-1, 2) if fout == "sc16" else buf
                rf.execute(x, first_sample=5, out=o)
        assert L.mcrx_hip_rfchain_last_error()
        torch.cuda.synchronize()
        assert torch.equal(bits(buf), bits(keep)), (fin, fout)          # refused calls wrote nothing
        assert rf.clipped() == 0
        with pytest.raises(TypeError):
            rf.execute(buf.real if fin == "cf32" else buf)
        rf.close()
    # what is allowed: adjacent ranges, one sample's alignment, in place with equal formats; and the handle belongs to its device
    rf = product.rfchain(**chain_kw(product, 7))
    x, d_x = samples(2 * n + 1, seed=13)
    work = d_x.clone()
    pw = work.data_ptr()

    def call(a, b, count=n):
        return L.mcrx_hip_rfchain_execute_device(rf._h, C.c_void_p(a), 5, count, C.c_void_p(b), None)
    assert call(pw, pw + 8 * n) == OK and call(pw + 16 * n, pw + 16 * n, 1) == OK and call(pw, pw, 0) == OK
    other = 1 if torch.cuda.device_count() > 1 else 0
    torch.cuda.set_device(other)
    try:
        y = rf.execute(d_x[:n], first_sample=5)
        torch.cuda.synchronize(0)
        assert torch.cuda.current_device() == other and int(y.numel()) == n
    finally:
        torch.cuda.set_device(0)
    assert torch.equal(bits(work[n:2 * n]), bits(y))                    # the adjacent call computed the same samples
    with pytest.raises(ValueError):
        product.rfchain().phase_rows(0, 4)                              # the oscillator is off
    rf.close()


# ---------------------------------------------------------------------------------------------- 7. where the products land
NCH, M_, CP, TAPER, NF, PLEN = 8, 64, 8, 4, 3, 96


def carriers(product, first, count, seed=31):
    """the wideband stream of a multichanneltx of which only channels first .. first + count - 1 carry frames: tx.traffic on those
    channels, their granules placed into tiles that are zero elsewhere, tx.synthesize"""
    torch = _torch()
    tx = product.multichanneltx(NCH, M_, CP, TAPER)
    tr = tx.traffic(first, count, NF, PLEN, seed=seed)
    ls, nb = product.USERCHAN_SYNTH_LEAD, tr.blocks
    part = torch.empty((ls + nb) * count, dtype=torch.complex64, device="cuda")
    tr.tiles(-ls, ls + nb, part)
    tiles = torch.zeros(((ls + nb) // 8, NCH, 8), dtype=torch.complex64, device="cuda")
    tiles[:, first:first + count, :] = part.view((ls + nb) // 8, count, 8)
    iq = tx.synthesize(tiles.view(-1), 1, 0, nb, ls, 0)
    tr.close(); tx.close()
    return iq


def levels_db(product, y):
    rx = product.multichannelrx(NCH, M_, CP, TAPER, max_payload_len=PLEN)
    rx.monitor_enable()
    n = int(y.numel()) // (product.TILE * 2 * NCH) * (product.TILE * 2 * NCH)
    rx.Execute(y[:n].contiguous()); rx.Flush()
    level = rx.monitor_read().level_db()
    frames = len([f for f in rx.frames if f.payload_valid])
    rx.close()
    return level, frames


def test_the_image_lands_in_the_mirror_channel(product):
    iq = carriers(product, 2, 1)
    m = product.rfchain_iq(1.0, 5.0, "tx")
    rf = product.rfchain(mixer=m)
    cfg = rf.config
    want = 10.0 * math.log10((cfg.beta_re ** 2 + cfg.beta_im ** 2) / (cfg.alpha_re ** 2 + cfg.alpha_im ** 2))
    level, frames = levels_db(product, rf.execute(iq))
    rf.close()
    off, frames_off = levels_db(product, iq)
    print("rfchain image: levels [dB] " + " ".join("%.1f" % v for v in level) + "; mixer off " + " ".join("%.1f" % v for v in off))
    print("rfchain image: level[5] - level[2] = %.2f dB, |beta|^2 / |alpha|^2 = %.2f dB" % (level[5] - level[2], want))
    assert frames == frames_off == NF
    assert abs((level[5] - level[2]) - want) <= 0.5
    others = [c for c in range(NCH) if c not in (2, 5)]
    assert all(level[c] <= level[5] - 20.0 for c in others), level
    # mixer off: as silent as the rest -- no louder than the loudest of them, and in the bank's stop band (60 dB down; 50 asked)
    assert off[5] <= max(off[c] for c in others) and off[5] <= off[2] - 50.0, off
    RATIOS["image_db_error"] = (level[5] - level[2]) - want


def test_intermodulation_lands_beside_the_carriers(product):
    """Channels 3 and 4 carry frames; the amplifier alone at 12, 6 and 2 dB back-off puts their third-order products into channels
    2 = 2 * 3 - 4 and 5 = 2 * 4 - 3.  No absolute level is asserted.
    "With the amplifier off they are as silent as the rest": channels 2 and 5 are the carriers' neighbours, and the bank's transition
    band leaves a neighbour of a carrier 44.5 dB below it with no front end in the chain at all (measured on the MI355X: -38.7 and
    -39.8 dB beside carriers at +5.7 dB, the channels further out at -81 .. -88 dB; the lone carrier of the image test shows the same
    -44.5 dB in channels 1 and 3).  So the sentence cannot hold against channels 0, 1, 6 and 7, and is asserted against its like: with
    the amplifier off channel 2 (5) holds what the neighbour of a LONE carrier in channel 3 (4) holds, within 1 dB -- the other
    carrier's skirt two channels away adds under 0.01 dB -- and the channels further out hold at least 20 dB less than that."""
    torch = _torch()
    iq = carriers(product, 3, 2)
    rms = float(torch.view_as_real(iq).pow(2).sum().div(int(iq.numel())).sqrt())
    silent = [0, 1, 2, 5, 6, 7]
    off, _ = levels_db(product, iq)
    rows = []
    for ibo in (12.0, 6.0, 2.0):
        rf = product.rfchain(amplifier=dict(sat=product.rfchain_backoff(ibo, rms), smooth=2))
        level, _ = levels_db(product, rf.execute(iq))
        rf.close()
        print("rfchain imd at %4.1f dB back-off: levels [dB] " % ibo + " ".join("%.1f" % v for v in level))
        assert sorted(sorted(silent, key=lambda c: level[c])[-2:]) == [2, 5], (ibo, level)
        rows.append(level)
    print("rfchain imd amplifier off:        levels [dB] " + " ".join("%.1f" % v for v in off))
    lone = {2: levels_db(product, carriers(product, 3, 1))[0], 5: levels_db(product, carriers(product, 4, 1))[0]}
    for c in (2, 5):
        print("rfchain imd lone carrier beside channel %d: levels [dB] " % c + " ".join("%.1f" % v for v in lone[c]))
        assert rows[0][c] < rows[1][c] < rows[2][c], [r[c] for r in rows]         # rises as the back-off falls
        assert off[c] < rows[0][c]                                                # ... from the level of the amplifier off,
        assert abs(off[c] - lone[c][c]) <= 1.0, (off, lone[c])                    # which is the bank's skirt of one carrier alone
    assert all(off[c] <= min(off[2], off[5]) - 20.0 for c in (0, 1, 6, 7)), off


# ---------------------------------------------------------------------------------------------- 8. end to end
def test_end_to_end(product, oracle):
    """multichanneltx -> rfchain (tx) -> chanemu (noise) -> rfchain (rx, sc16 out) -> multichannelrx(sc16), and the oracle's receiver on
    the same integers times 2^-15, at rfchain_model.SEVERITY (found on the oracle alone by tests/test_rfchain.py).  framesyms: held to
    the 1e-3 the sibling end-to-end tests assert, the deviation recorded (PARITY, printed by the last test)."""
    from test_gpu_parity import match_frames, relerr, relerr_elem
    torch = _torch()
    s = model.SEVERITY
    N, M, cp, taper, nf, plen = s["N"], s["M"], s["cp"], s["taper"], s["frames"], s["payload_len"]
    tx = product.multichanneltx(N, M, cp, taper)
    iq, sent = tx.generate(nf, plen, seed=77 + N)                    # QPSK / Hamming(12,8), gain 1 / N
    tx.close()
    rms = float(torch.view_as_real(iq).pow(2).sum().div(int(iq.numel())).sqrt())
    txk, rxk = model.severity_chains(product, rms)
    rtx = product.rfchain(**txk)
    a = rtx.execute(iq)
    rtx.close()
    power = float(torch.view_as_real(a).pow(2).sum()) / int(a.numel())
    nstd = float(np.float32(math.sqrt(power / 10.0 ** (s["snr_db"] / 10.0) / 2.0)))
    ce = product.chanemu(taps=[(0, 1.0)], noise_std=nstd, seed=s["noise_seed"])
    b = ce.execute(a)
    ce.close()
    probe = product.rfchain(**rxk)
    g = float(np.float32(s["peak"] / float(torch.view_as_real(probe.execute(b)).abs().max())))
    probe.close()
    rrx = product.rfchain(gain=g, output_format="sc16", **rxk)
    y = rrx.execute(b)
    assert rrx.clipped() == 0
    rrx.close()
    n = int(y.shape[0]) // (product.TILE * 2 * N) * (product.TILE * 2 * N)
    y = y[:n].contiguous()
    y_host = (host(y).astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64).reshape(-1)
    rx = product.multichannelrx(N, M, cp, taper, max_payload_len=plen, input_format="sc16")
    rx.Execute(y); rx.Flush()
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
    evm = [f.evm for f in rx.frames]
    rx.close()
    PARITY["severity"] = {"max_norm": w, "element_wise": we, "noise_std": nstd, "rms": rms, "rx_gain": g, "evm_db": [min(evm), max(evm)]}
    print("rfchain_parity: framesyms max-norm %.3e element-wise %.3e; EVM %.1f .. %.1f dB" % (w, we, min(evm), max(evm)))
    assert w <= 1e-3, w


def test_zz_print_rfchain_figures():
    """(last of this file: the figures measured above as one JSON line each -- profiles/rfchain_model.json and
    profiles/rfchain_parity.json are such records; RFCHAIN_OUT / RFCHAIN_PARITY_OUT name files to write them to as well)"""
    for tag, rec, env in (("rfchain_model", RATIOS, "RFCHAIN_OUT"), ("rfchain_parity", PARITY, "RFCHAIN_PARITY_OUT")):
        line = json.dumps(rec, sort_keys=True)
        print(tag + " " + line)
        path = os.environ.get(env)
        if path:
            with open(path, "w") as f:
                f.write(line + "\n")
