"""Channel emulator on the GPU (mcrx_hip_chanemu_*) against the float64 model of tests/chanemu_model.py, against
itself cut into pieces, against the transmitter's quantiser, and end to end between multichanneltx and multichannelrx / the oracle.

Bounds.  Taps, rotation and gain, per component:  |got - model| <= ((2T + 8) 2^-24 + 3e-7) * gain * sum|a_i| * max|x|  -- the fp32
rounding of 2T fused multiply-adds plus rotation and gain, and sincos_u32's stated error.  Noise, per component: 1e-5 * noise_std (the
project's relative bar; a few ulp of logf, sqrtf and the sine at rho <= 5.8 is about 1e-6).  Where both act, the sum of the two."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import chanemu_model as model
import tx_sc16_model as q16

pytestmark = pytest.mark.gpu

TAPS_A = [(0, 1.0 + 0.0j), (37, 0.35 - 0.2j), (4099, -0.15 + 0.2j)]
TAPS_B = [(5, 0.5 + 0.1j), (1, -0.3 + 0.25j), (65535, 0.2 - 0.2j), (37, 0.1 + 0.3j), (37, -0.25 - 0.05j), (0, 1.0 - 0.1j),
          (4099, 0.15 + 0.15j), (1000, -0.1 + 0.2j)]                       # table order is not delay order; 37 twice
CFO_STEP, PHASE0, GAIN = 0x00A3D70B, 0x9E3779B9, 0.7
N_LONG = 3 * 65536 + 1235
NOISE_STD, SEED = 0.25, 0xC0FFEE0123456789
SENTINEL = 0x5A5B


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_X = {}


def samples(n, seed=7):
    """seeded complex normal samples, host (complex64) and device; made once per length and left alone"""
    if (n, seed) not in _X:
        torch = _torch()
        rng = np.random.RandomState(seed)
        x = (rng.randn(n) + 1j * rng.randn(n)).astype(np.complex64)
        _X[(n, seed)] = (x, torch.from_numpy(x).cuda())
    return _X[(n, seed)]


def tap_bound(taps, gain, x):
    T = len(taps)
    return ((2 * T + 8) * 2.0 ** -24 + 3e-7) * gain * sum(abs(complex(np.complex64(a))) for _, a in taps) * float(np.abs(x).max())


def worst(got, want):
    d = np.asarray(got, np.complex128) - want
    return float(max(np.abs(d.real).max(), np.abs(d.imag).max()))


def host(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. identity
def test_identity(product):
    torch = _torch()
    x, d_x = samples(10007)
    ce = product.chanemu(taps=[(0, 1.0)])
    y = ce.execute(d_x)
    assert y.dtype == torch.complex64 and ce.position() == 10007 and ce.clipped() == 0
    assert np.array_equal(host(y), x)
    ce.close()
    ce = product.chanemu(taps=[(0, 1.0)], output_format="sc16")
    assert ce.output_format == 1 and product.lib().mcrx_hip_chanemu_output_format(ce._h) == 1
    y = ce.execute(d_x)
    assert y.dtype == torch.int16 and tuple(y.shape) == (10007, 2) and y.is_contiguous()
    assert np.array_equal(host(y), q16.quantise_iq(x))
    want = q16.clipped_samples(x)
    assert want > 100 and ce.clipped() == want                   # (unit normal components: a third of the samples pass full scale)
    ce.close()


# ---------------------------------------------------------------------------------------------- 2. taps, rotation, gain
@pytest.mark.parametrize("name,taps", [("A", TAPS_A), ("B", TAPS_B)])
def test_taps_rotation_gain_against_the_model(product, name, taps):
    x, d_x = samples(N_LONG)
    ce = product.chanemu(taps=taps, cfo_step=CFO_STEP, phase0=PHASE0, gain=GAIN)
    got = host(ce.execute(d_x))
    ce.close()
    want = model.apply(x, taps, CFO_STEP, PHASE0, GAIN)
    bound, w = tap_bound(taps, GAIN, x), worst(got, want)
    print("chanemu case %s: worst |got - model| %.3e, bound %.3e (%.2f of it)" % (name, w, bound, w / bound))
    assert float(np.abs(want).max()) > 1.0
    assert w <= bound, (w, bound)
    # a tap table in another order is another sum of the same channel: the same bound
    ce = product.chanemu(taps=taps[::-1], cfo_step=CFO_STEP, phase0=PHASE0, gain=GAIN)
    assert worst(host(ce.execute(d_x)), want) <= bound
    ce.close()


# ---------------------------------------------------------------------------------------------- 3. noise
def test_noise_against_the_model(product):
    torch = _torch()
    n = 2 ** 16 + 3
    zeros = torch.zeros(n, dtype=torch.complex64, device="cuda")
    ce = product.chanemu(taps=[(0, 1.0)], noise_std=NOISE_STD, seed=SEED)
    a = host(ce.execute(zeros))
    ce.reset()
    b = host(ce.execute(zeros))
    ce.close()
    want = np.float64(np.float32(NOISE_STD)) * model.noise(SEED, 0, n)
    w = worst(a, want)
    print("chanemu noise: worst |got - model| %.3e = %.3e of noise_std (bar 1e-5)" % (w, w / NOISE_STD))
    assert w <= 1e-5 * NOISE_STD, w
    assert abs(float(np.mean(np.abs(a) ** 2)) / (2 * NOISE_STD ** 2) - 1.0) < 0.02
    assert a.tobytes() == b.tobytes()                             # the same seed: the same bits
    ce = product.chanemu(taps=[(0, 1.0)], noise_std=NOISE_STD, seed=SEED + 1)
    c = host(ce.execute(zeros))
    ce.close()
    assert np.count_nonzero(c != a) > 0.99 * n


# ---------------------------------------------------------------------------------------------- 4. cut anywhere
def pieces(n):
    """odd and even, empty, shorter and longer than D = 4099, one of MAX_DELAY, then seeded odds and ends"""
    sizes = [1, 0, 2, 4098, 65535, 7, 4099, 4100, 3, 1, 30001, 0, 8192]
    rng = np.random.RandomState(5)
    cuts, pos = [], 0
    for s in sizes:
        cuts.append((pos, min(pos + s, n))); pos = min(pos + s, n)
    while pos < n:
        s = int(rng.randint(1, 40000))
        cuts.append((pos, min(pos + s, n))); pos = min(pos + s, n)
    return cuts


@pytest.mark.parametrize("fmt", ["cf32", "sc16"])
def test_cut_anywhere(product, fmt):
    torch = _torch()
    x, d_x = samples(N_LONG)
    cfg = dict(taps=TAPS_A, cfo_step=CFO_STEP, phase0=PHASE0, gain=GAIN, noise_std=NOISE_STD, seed=SEED, output_format=fmt)
    ce = product.chanemu(**cfg)
    one = ce.execute(d_x).clone()
    clips = ce.clipped(reset=True)
    ce.reset()
    sc16 = fmt == "sc16"
    if sc16:
        buf = torch.full((N_LONG + 64, 2), SENTINEL, dtype=torch.int16, device="cuda")
        assert clips > 100
    else:
        buf = torch.full((N_LONG + 64,), float("nan"), dtype=torch.complex64, device="cuda")
        assert clips == 0
    odd_calls = 0
    for a, b in pieces(N_LONG):
        out = buf[a:]
        odd_calls += int(b > a and out.data_ptr() % (8 if sc16 else 16) != 0)
        y = ce.execute(d_x[a:b], out=out)
        assert int(y.shape[0]) == b - a and ce.position() == b
    assert odd_calls > 3                                          # pieces that begin on an odd sample: 4- (8-) byte-only alignment
    torch.cuda.synchronize()
    if sc16:
        assert torch.equal(buf[:N_LONG], one)                     # the stream cut in pieces is the stream, word for word
        assert bool((buf[N_LONG:] == SENTINEL).all())             # nothing stored behind it
    else:
        assert torch.equal(torch.view_as_real(buf[:N_LONG]).view(torch.int32), torch.view_as_real(one).view(torch.int32))
        assert bool(torch.isnan(buf[N_LONG:].real).all())
    assert ce.clipped() == clips
    ce.close()


# ---------------------------------------------------------------------------------------------- 5. far positions
def test_far_positions(product):
    x, d_x = samples(5000, seed=9)
    cfg = dict(taps=TAPS_A, cfo_step=CFO_STEP, phase0=PHASE0, gain=GAIN, noise_std=NOISE_STD, seed=SEED)
    bound = tap_bound(TAPS_A, GAIN, x) + 1e-5 * NOISE_STD
    ce = product.chanemu(**cfg)
    ce.execute(d_x[:1000])                                        # (history that the reset must drop)
    p = 2 ** 40 + 3
    ce.reset(at=p)
    assert ce.position() == p
    got = host(ce.execute(d_x))
    assert ce.position() == p + 5000
    w = worst(got, model.apply(x, TAPS_A, CFO_STEP, PHASE0, GAIN, NOISE_STD, SEED, start=p))
    print("chanemu at 2^40 + 3: worst %.3e, bound %.3e" % (w, bound))
    assert w <= bound
    p = 2 ** 33 - 1000                                            # the counter's low word wraps at sample 2^33
    ce.reset(at=p)
    got = np.concatenate([host(ce.execute(d_x[:777])), host(ce.execute(d_x[777:2500]))])
    assert ce.position() == p + 2500
    want = model.apply(x[:2500], TAPS_A, CFO_STEP, PHASE0, GAIN, NOISE_STD, SEED, start=p)
    w = worst(got, want)
    print("chanemu across 2^33: worst %.3e, bound %.3e" % (w, bound))
    assert w <= bound
    # ... and it is not the stream at position 0
    assert worst(got, model.apply(x[:2500], TAPS_A, CFO_STEP, PHASE0, GAIN, NOISE_STD, SEED, start=0)) > 0.1
    ce.close()


# ---------------------------------------------------------------------------------------------- 6. sc16 is Q of cf32
@pytest.mark.parametrize("name", ["taps", "noise"])
def test_sc16_is_q_of_cf32(product, name):
    torch = _torch()
    if name == "taps":
        x, d_x = samples(N_LONG)
        cfg = dict(taps=TAPS_A, cfo_step=CFO_STEP, phase0=PHASE0, gain=0.4)
    else:
        d_x = torch.zeros(2 ** 16 + 3, dtype=torch.complex64, device="cuda")
        cfg = dict(taps=[(0, 1.0)], noise_std=NOISE_STD, seed=SEED)
    cf, sc = product.chanemu(**cfg), product.chanemu(output_format="sc16", **cfg)
    y, i = host(cf.execute(d_x)), host(sc.execute(d_x))
    want = q16.clipped_samples(y)
    assert 0 < want < 0.2 * len(y), want                          # some samples clip, most do not
    assert np.array_equal(i, q16.quantise_iq(y))
    if name == "taps":
        assert i.min() == -32768 and i.max() == 32767             # saturated, not wrapped
    assert cf.clipped() == 0
    assert sc.clipped() == want and sc.clipped(reset=True) == want and sc.clipped() == 0
    for _ in range(2):
        sc.reset()
        sc.execute(d_x)
    assert sc.clipped() == 2 * want                               # it accumulates over calls
    cf.close(); sc.close()


# ---------------------------------------------------------------------------------------------- 7. errors on the device
def test_errors_on_the_device(product):
    torch = _torch()
    L, EINVAL = product.lib(), product.MCRX_EINVAL
    n = 4096
    d_x = torch.zeros(2 * n, dtype=torch.complex64, device="cuda")
    d_y = torch.zeros(2 * n, dtype=torch.complex64, device="cuda")
    cf, sc = product.chanemu(taps=TAPS_A), product.chanemu(taps=TAPS_A, output_format="sc16")
    px, py = d_x.data_ptr(), d_y.data_ptr()

    def call(ce, a, b, count=n):
        return L.mcrx_hip_chanemu_execute_device(ce._h, C.c_void_p(a) if a else None, count, C.c_void_p(b) if b else None, None)
    for ce in (cf, sc):
        size = 4 if ce is sc else 8
        assert call(ce, None, py) == EINVAL and call(ce, px, None) == EINVAL
        assert call(ce, px + 4, py) == EINVAL                     # d_in: 8 bytes
        assert call(ce, px, py + size // 2) == EINVAL             # d_out: one sample of its format
        assert call(ce, px, px) == EINVAL                         # in place
        assert call(ce, px, px + 8 * n - size) == EINVAL          # the output's first sample on the input's last
        assert call(ce, px + 8 * n, px + 8 * n - size * n + size) == EINVAL        # the output's last sample on the input's first
        assert L.mcrx_hip_chanemu_last_error()
        assert ce.position() == 0                                 # refused calls consumed nothing
        assert call(ce, px, px + 8 * n) == product.MCRX_OK        # adjacent is not overlapping
        assert call(ce, px + 8 * n, px + 8 * n - size * n) == product.MCRX_OK
        assert call(ce, px + 8, py + size) == product.MCRX_OK     # one sample's alignment is enough
        assert ce.position() == 3 * n
        with pytest.raises(ValueError):
            ce.execute(d_x[:n], out=(torch.view_as_real(d_x).view(torch.int16).view(-1, 2) if ce is sc else d_x))     # in place
        with pytest.raises(TypeError):
            ce.execute(d_x.real)
    with pytest.raises(TypeError):
        sc.execute(d_x[:n], out=d_y)
    torch.cuda.synchronize()
    # the handle belongs to its device: calls run there and put the caller's device back
    other = 1 if torch.cuda.device_count() > 1 else 0
    torch.cuda.set_device(other)
    try:
        y = cf.execute(d_x[:n], out=d_y)
        torch.cuda.synchronize(0)
        assert torch.cuda.current_device() == other and int(y.numel()) == n and cf.clipped() == 0 and sc.clipped() == 0
    finally:
        torch.cuda.set_device(0)
    cf.close(); sc.close()
    cf.close()                                                    # twice is harmless


# ---------------------------------------------------------------------------------------------- 8. end to end
PARITY = {}
E2E = [("N2_p0.30_25dB", 2, 0.3, 25.0, "cf32"), ("N2_m0.45_25dB", 2, -0.45, 25.0, "cf32"), ("N8_p0.45_20dB", 8, 0.45, 20.0, "cf32"),
       ("N2_p0.30_25dB_sc16", 2, 0.3, 25.0, "sc16")]


@pytest.mark.parametrize("name,N,spacings,snr_db,fmt", E2E, ids=[e[0] for e in E2E])
def test_end_to_end(product, oracle, name, N, spacings, snr_db, fmt):
    """multichanneltx -> chanemu (three rays inside every channel, carrier offset, noise) -> multichannelrx, and the oracle's receiver
    on the same emulated samples.  The 1e-5 framesyms bar has only been evidenced on flat channels: here the deviation is recorded
    (PARITY, printed by the last test) and held to the loosest bar check_frames uses, 1e-3."""
    from test_gpu_parity import match_frames, relerr, relerr_elem
    torch = _torch()
    M, cp, taper, nf, plen = 64, 8, 4, 3, 96
    K = 2 * N
    taps = [(0, 1.0), (K + 3, 0.35 - 0.2j), (3 * K, -0.15 + 0.2j)]
    tx = product.multichanneltx(N, M, cp, taper)
    iq, sent = tx.generate(nf, plen, seed=77 + N)                  # QPSK / Hamming(12,8), gain 1 / N
    tx.close()
    iq = torch.cat([iq, torch.zeros(64 * K, dtype=torch.complex64, device="cuda")])           # (the delayed rays' tail)
    step = product.chanemu_cfo_step(spacings, M, N)
    clean = product.chanemu(taps=taps, cfo_step=step)
    v = torch.view_as_real(clean.execute(iq))
    power = float(v.pow(2).sum()) / int(iq.numel())
    g = float(np.float32(0.5 / float(v.abs().max()))) if fmt == "sc16" else 1.0      # sc16: the noise-free peak at half of full scale
    clean.close()
    nstd = float(np.sqrt(g * g * power / 10.0 ** (snr_db / 10.0) / 2.0))
    ce = product.chanemu(taps=taps, cfo_step=step, gain=g, noise_std=nstd, seed=2024, output_format=fmt)
    y = ce.execute(iq)
    n = int(iq.numel()) // (product.TILE * K) * (product.TILE * K)
    rx = product.multichannelrx(N, M, cp, taper, max_payload_len=plen, input_format=fmt)
    if fmt == "sc16":
        assert ce.clipped() == 0
        y = y[:n].contiguous()
        y_host = (host(y).astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64).reshape(-1)
    else:
        y = y[:n].contiguous()
        y_host = host(y)
    ce.close()
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
    rx.close()
    PARITY[name] = {"max_norm": w, "element_wise": we, "noise_std": nstd, "cfo_step": step}
    print("chanemu_parity %s: framesyms max-norm %.3e element-wise %.3e" % (name, w, we))
    assert w <= 1e-3, w


def test_zz_print_chanemu_parity():
    """(last of this file: the deviations measured above as one JSON line -- profiles/chanemu_parity.json is such a record;
    CHANEMU_PARITY_OUT names a file to write it to as well)"""
    line = json.dumps(PARITY, sort_keys=True)
    print("chanemu_parity " + line)
    path = os.environ.get("CHANEMU_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")
