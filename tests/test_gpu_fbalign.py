"""Feedback alignment for the predistorters on the MI355X (mcrx_hip_fbalign_*): the copy build bit for bit, apply
against tests/fbalign_model.py within its derived bound, cuts and input formats bit for bit, the sums, tau_fp, s, res and coefficients
against the model to the last bit, set, reset and the refusals, and the two closed loops -- dpd on rfchain's amplifier and mpd on
mpd_model.SEVERITY's three-branch amplifier, the amplifier's output through a host-made path and sc16 -- at fbalign_model.SEVERITY."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cfr_model
import dpd_model
import fbalign_model as model
import mpd_model
from test_fbalign import band_limited, library_table
from test_gpu_dpd import _torch, bits, dev, host, odd_words, oob_of, placed, rms_of, words, worst
from test_gpu_mpd import MemoryAmplifier

pytestmark = pytest.mark.gpu

PARITY = {}
NAN, INF = float("nan"), float("inf")


def dev16(q, shift=0):
    """int16 [n, 2] host samples on the device, beginning `shift` samples (4 bytes each) behind a 16-byte boundary"""
    torch = _torch()
    buf = torch.zeros((len(q) + 4, 2), dtype=torch.int16, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[shift:shift + len(q)].copy_(torch.from_numpy(np.ascontiguousarray(q, np.int16)))
    return buf[shift:shift + len(q)]


def same_state(r, m, W):
    c, nd = m.coefs()
    with np.errstate(all="ignore"):
        sc = complex(np.float32(m.s[0]), np.float32(m.s[1]))
    assert (r["tau_fp"], r["s"], r["res"]) == (m.tau_fp, complex(*m.s), m.res), (r["tau_fp"], m.tau_fp, r["s"], m.s, r["res"], m.res)
    assert (r["updates"], r["degenerate"], r["rows"], r["clamped"]) == (m.updates, m.degenerate, m.rows, m.clamped)
    assert np.array_equal(r["coef"].view(np.uint32), c.view(np.uint32)) and r["nd"] == nd and r["scale"] == sc


def same_sums(r, m):
    assert np.array_equal(r["C"], m.C), np.nonzero((r["C"] != m.C).any(axis=1))[0][:10]
    assert np.array_equal(r["A"], m.A) and r["Szz"] == m.Szz and r["rows"] == m.rows and r["clamped"] == m.clamped


# ---------------------------------------------------------------------------------------------- 1. the untouched handle
@pytest.mark.parametrize("fin", ["cf32", "sc16"])
def test_untouched_handle_is_a_copy(product, fin):
    """n = 1 .. 257 from both parities of the output and (sc16) from capture buffers that are 4-byte but not 8-byte aligned: out[i] is
    in[halo + i], bit for bit -- NaN payloads and -0.0 included on cf32, every int16 times 2^-15 on sc16 --, nothing else is written"""
    torch = _torch()
    d = product.fbalign(8, 1.0, 1.0, input_format=fin)
    halo = d.halo
    assert halo == 25
    rng = np.random.RandomState(3)
    total = 257 + 2 * halo
    if fin == "cf32":
        x = odd_words(total, 11)
        want = bits(x)
    else:
        q = rng.randint(-32768, 32768, (total, 2)).astype(np.int16)
        q[:4] = [[-32768, 32767], [0, -1], [1, 0], [-32768, -32768]]
        want = bits((q.astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64).reshape(-1))
    for n in range(1, 258):
        shift = n % 4 if fin == "sc16" else n % 2
        src = dev16(q[:n + 2 * halo], shift) if fin == "sc16" else placed(x[:n + 2 * halo], shift)
        out = torch.full((n + 3,), complex(7.0, -7.0), dtype=torch.complex64, device="cuda")
        oshift = (n // 2) % 2
        got = d.execute(src, out=out[oshift:oshift + n])
        assert got.data_ptr() == out.data_ptr() + 8 * oshift
        o = words(out).view(np.uint32)
        assert np.array_equal(o[oshift:oshift + n], want[halo:halo + n]), n
        guard = np.array([np.float32(7.0), np.float32(-7.0)]).view(np.uint32)
        assert (o[:oshift] == guard).all() and (o[oshift + n:] == guard).all(), n
    assert d.read()["updates"] == 0 and d.read()["tau_fp"] == 0 and d.read()["s"] == 1.0
    d.close()


# ---------------------------------------------------------------------------------------------- 2. apply against the model
@pytest.mark.parametrize("n", [1, 255, 4099])
@pytest.mark.parametrize("Lm", [8, 64])
def test_apply_against_the_model(product, Lm, n):
    """tau = 0, all 64 table rows (fractions 1/64 apart) and fractions between them at whole parts across the range, +-(Lm + 1); a
    scale of any phase: every output component within the model's derived bound of the float64 result"""
    W = library_table(product)
    d = product.fbalign(Lm, 1.0, 1.0)
    rng = np.random.RandomState(n + Lm)
    x = (rng.standard_normal(n + 2 * d.halo) + 1j * rng.standard_normal(n + 2 * d.halo)).astype(np.complex64)
    xd = placed(x, n % 2)
    obuf = _torch().zeros(n + 2, dtype=_torch().complex64, device="cuda")
    assert obuf.data_ptr() % 16 == 0
    most = (Lm + 1) << 32
    taus = [0, most, -most, most - 1, -most + 1] + [(int(rng.randint(-Lm, Lm + 1)) << 32) + (r << 26) for r in range(64)] \
        + [int(t) for t in rng.randint(-most, most, 16)]
    ratio = 0.0
    for k, tau in enumerate(taus):
        s = complex(1.0) if k == 0 else (0.2 + 1.5 * rng.rand()) * np.exp(2j * np.pi * rng.rand())
        d.set(tau, s)
        oshift = k % 2                                                                     # the output begins at an even / odd multiple of 8 bytes
        got = d.execute(xd, out=obuf[oshift:oshift + n])
        assert got.data_ptr() == obuf.data_ptr() + 8 * oshift
        got = host(got)
        want, bound = model.apply(W, tau, (s.real, s.imag), x, d.halo)
        assert got.shape == want.shape == (n,)
        ratio = max(ratio, worst(got, want, np.maximum(bound, 1e-30)))
        if tau % (1 << 32) == 0 and k == 0:
            assert np.array_equal(bits(got), bits(x[d.halo:d.halo + n]))                       # a whole-sample delay at s = 1 is exact
    print("fbalign apply: Lm %d n %d: worst error / bound %.3f over %d delays" % (Lm, n, ratio, len(taus)))
    assert ratio <= 1.0
    d.close()


# ---------------------------------------------------------------------------------------------- 3. cuts and formats
def test_pieces_with_their_halos_are_one_call(product):
    """a stream cut into pieces of 1 .. 257 samples, each with its halos, gives the bits of one call; sc16 in gives the bits of cf32 in
    on the same floats"""
    torch = _torch()
    rng = np.random.RandomState(8)
    n = sum(range(1, 258))
    d, d16 = product.fbalign(16, 1.0, 1.0), product.fbalign(16, 1.0, 1.0, input_format="sc16")
    halo = d.halo
    q = rng.randint(-32768, 32768, (n + 2 * halo, 2)).astype(np.int16)
    x = (q.astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64).reshape(-1)
    tau, s = -(3 << 32) - 0x5A5A5A5A, 0.7 * np.exp(2.1j)
    d.set(tau, s); d16.set(tau, s)
    xd, qd = placed(x, 1), dev16(q, 1)
    whole = words(d.execute(xd))
    assert np.array_equal(whole, words(d16.execute(qd)))
    assert np.array_equal(whole, words(d16.execute(dev16(q, 2))))
    obuf, obuf16 = torch.zeros(260, dtype=torch.complex64, device="cuda"), torch.zeros(260, dtype=torch.complex64, device="cuda")
    assert obuf.data_ptr() % 16 == 0 and obuf16.data_ptr() % 16 == 0
    odd = torch.zeros(n + 2, dtype=torch.complex64, device="cuda")
    assert np.array_equal(whole, words(d.execute(xd, out=odd[1:1 + n])))                   # the whole stream into an odd multiple of 8 bytes
    at = 0
    for k in range(1, 258):
        o = (k // 3) % 2                                                                   # either parity of the output
        piece = words(d.execute(xd[at:at + k + 2 * halo], out=obuf[o:o + k]))
        piece16 = words(d16.execute(qd[at:at + k + 2 * halo], out=obuf16[1 - o:1 - o + k]))
        assert np.array_equal(piece, whole[at:at + k]) and np.array_equal(piece16, whole[at:at + k]), k
        at += k
    assert at == n
    d.close(); d16.close()


# ---------------------------------------------------------------------------------------------- 4. the sums
def spoiled(n, seed):
    """(u, zh): two correlated streams around a full scale of 1 with NaN, infinite and over-range samples in both"""
    rng = np.random.RandomState(seed)
    u = (0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    z = (np.roll(u, 3) * np.complex64(0.8 - 0.3j) + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    for k, bad in enumerate([NAN, complex(0, NAN), INF, complex(0, -INF), 3e38, complex(-1.5, 0.2), complex(1.0, -1.0), complex(-1.0, 0.99997)]):
        u[(17 * k + 5) % n], z[(29 * k + 11) % n] = bad, bad
    u[n // 2], z[n // 2] = complex(-1.0, -1.0), complex(-1.0, -1.0)                                # the worst term: 2^31
    return u, z


@pytest.mark.parametrize("size", ["2R+1", "257", "70001", "beyond the grid"])
@pytest.mark.parametrize("Lm", [8, 32, 64])
def test_sums_equal_the_model(product, Lm, size):
    """C, A, Szz, rows and clamped equal the model's integers; two calls add up; a call of n <= 2 R measures nothing"""
    R = Lm + 8
    n = {"2R+1": 2 * R + 1, "257": 257, "70001": 70001, "beyond the grid": 2 * R + (product.FBALIGN_MAX_WGS + 1) * 256 - 3}[size]
    u, z = spoiled(n, n + Lm)
    d, m = product.fbalign(Lm, 1.0, 1.0), model.Model(Lm, 1.0, 1.0)
    ud, zd = placed(u, 1), placed(z, 0)
    assert d.measure(ud, zd) == n - 2 * R and m.measure(u, z)
    r = d.read()
    same_sums(r, m)
    assert r["rows"] == n - 2 * R and (r["clamped"] > 0 or n < 300) and r["A"][0, 1] == 0
    assert d.measure(ud[:2 * R], zd[:2 * R]) == 0
    k = min(n, 1000)
    assert d.measure(ud[:k], zd[:k]) == k - 2 * R and m.measure(u[:k], z[:k])
    same_sums(d.read(), m)
    d.close()


# ---------------------------------------------------------------------------------------------- 5. the update
@pytest.mark.parametrize("fin", ["cf32", "sc16"])
@pytest.mark.parametrize("Lm,tau", [(8, 0.5), (16, 7.37), (64, -12.5), (64, 63.49), (8, -7.49)])
def test_state_after_updates_equals_the_model(product, Lm, tau, fin):
    """execute -> measure -> update three times on a linear path: after every update tau_fp, s, res, the coefficients, nd and the fp32
    scale equal the model's to the last bit (the model measures the very samples the device's apply wrote), and the path is found"""
    W = library_table(product)
    n = 12000
    u = band_limited(n, 0.56, Lm)
    gain = 0.6 * np.exp(1.1j)
    z = model.path(u, tau, gain).astype(np.complex64)
    if fin == "sc16":
        zq = model.to_sc16(z)
        zd = dev16(zq, 1)
    else:
        zd = placed(z, 1)
    d, m = product.fbalign(Lm, 0.75, 2.0, min_rows=100, input_format=fin), model.Model(Lm, 0.75, 2.0, min_rows=100, W32=W)
    ud = dev(u)[d.halo:n - d.halo]
    for k in range(3):
        zh = d.execute(zd)
        assert d.measure(ud, zh) == n - 2 * d.halo - 2 * d.R
        assert m.measure(host(ud), host(zh))
        same_sums(d.read(), m)
        d.update(); m.update()
        same_state(d.read(), m, W)
    r = d.read()
    print("fbalign update: Lm %d tau %+.2f %s: found %+.7f, s %s, res %.4g" % (Lm, tau, fin, r["tau"], r["s"], r["res"]))
    # the rows within R of the record's ends pair samples the circular path took from its other end: they weigh 2 R / rows of every
    # sum, and what they add is bounded by the signal's own correlation, so they move tau and s by less than that share
    ends = 2.0 * d.R / (n - 2 * d.halo - 2 * d.R)
    assert r["degenerate"] == 0 and abs(r["tau"] - tau) < ends and abs(r["s"] * gain / 2.0 - 1.0) < ends
    ut, za = d.align(dev(u), zd, rounds=1)
    assert int(ut.numel()) == int(za.numel()) == n - 2 * d.halo
    assert dpd_model.nmse_db(host(za), 2.0 * host(ut).astype(np.complex128)) < -55.0
    assert d.read()["updates"] == 4
    d.close()


def test_degenerate_updates_on_the_device(product):
    W = library_table(product)
    x = band_limited(400, 0.5, 1)
    for what, u, z, rows in (("too few rows", x, x, 369), ("nothing measured", None, None, 1), ("zero capture", x, np.zeros(400, np.complex64), 1),
                             ("a constant", np.full(400, 0.25, np.complex64), np.full(400, 0.25, np.complex64), 1)):
        d, m = product.fbalign(8, 1.0, 1.0, min_rows=rows), model.Model(8, 1.0, 1.0, min_rows=rows, W32=W)
        d.set(5 << 30, 2.0 - 1.0j); m.set(5 << 30, 2.0 - 1.0j)
        if u is not None:
            d.measure(dev(u), dev(z)); m.measure(u, z)
        d.update(); m.update()
        r = d.read()
        assert r["degenerate"] == 1 and r["updates"] == 1 and r["rows"] == 0 and not r["sums"].any(), what
        same_state(r, m, W)
        assert r["tau_fp"] == 5 << 30 and r["s"] == 2.0 - 1.0j
        d.close()


# ---------------------------------------------------------------------------------------------- 6. set, reset, refusals
def test_set_and_reset(product):
    torch = _torch()
    W = library_table(product)
    d = product.fbalign(8, 1.0, 1.0)
    x = odd_words(300 + 2 * d.halo, 4)
    xd = dev(x)
    u = band_limited(300, 0.5, 2)
    r = d.read()
    assert (r["tau_fp"], r["s"], r["res"], r["rows"], r["updates"], r["nd"], r["scale"]) == (0, 1.0, 0.0, 0, 0, 0, 1.0) and not r["sums"].any()
    assert r["coef"].tolist() == [1.0 if j == 15 else 0.0 for j in range(32)]
    d.measure(dev(u), dev(u))
    d.set((2 << 32) + 12345678, 0.5j)
    r = d.read()
    c, nd = model.coefs(W, (2 << 32) + 12345678)
    assert (r["tau_fp"], r["s"], r["nd"], r["scale"]) == ((2 << 32) + 12345678, 0.5j, nd, 0.5j) and np.array_equal(r["coef"], c)
    assert r["rows"] == 300 - 32 and r["sums"].any()                                       # a set keeps sums and counters
    assert not np.array_equal(words(d.execute(xd)).view(np.uint32), bits(x[d.halo:d.halo + 300]))
    d.reset()                                                                              # no synchronisation: the next launches see it
    assert np.array_equal(words(d.execute(xd)).view(np.uint32), bits(x[d.halo:d.halo + 300]))  # the copy build again
    r = d.read()
    assert (r["tau_fp"], r["s"], r["res"], r["rows"], r["updates"], r["degenerate"], r["clamped"], r["nd"]) == (0, 1.0, 0.0, 0, 0, 0, 0, 0) and not r["sums"].any()
    assert r["coef"].tolist() == [1.0 if j == 15 else 0.0 for j in range(32)]
    d.set(1 << 31)
    d.reset()
    d.measure(dev(u), dev(u))                                                              # the pending reset is served first
    r = d.read()
    assert r["tau_fp"] == 0 and r["rows"] == 300 - 32
    torch.cuda.synchronize()
    d.close()


def test_refusals_on_the_device(product):
    """every refused call writes nothing and measures nothing"""
    torch = _torch()
    L, OK, EINVAL = product.lib(), product.MCRX_OK, product.MCRX_EINVAL
    d = product.fbalign(8, 1.0, 1.0)
    d16 = product.fbalign(8, 1.0, 1.0, input_format="sc16")
    halo, n = d.halo, 200
    buf = torch.zeros(n + 2 * halo + 8, dtype=torch.complex64, device="cuda")
    out = torch.full((n + 8,), complex(3.0, 4.0), dtype=torch.complex64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def execute(h, src, k, dst):
        return L.mcrx_hip_fbalign_execute_device(h._h, C.c_void_p(src), k, C.c_void_p(dst), st)

    def measure(a, b, k):
        return L.mcrx_hip_fbalign_measure_device(d._h, C.c_void_p(a), C.c_void_p(b), k, st)

    p, o = buf.data_ptr(), out.data_ptr()
    for rc in (execute(d, 0, n, o), execute(d, p, n, 0), execute(d, p + 4, n, o), execute(d, p, n, o + 4), execute(d16, p + 2, n, o),
               execute(d, p, (1 << 32) - 2 * halo + 1, o), execute(d, p, n, p), execute(d, p, n, p + 8 * (n + 2 * halo - 1)),
               execute(d, p + 8, 8, p), execute(d16, p, n, p + 4 * (n + 2 * halo) - 8)):
        assert rc == EINVAL and L.mcrx_hip_fbalign_last_error()
    assert execute(d, p, 0, o) == OK
    for rc in (measure(0, p, n), measure(p, 0, n), measure(p + 4, p, n), measure(p, p + 4, n), measure(p, p, (1 << 32) + 1)):
        assert rc == EINVAL
    for tau, s in ((10 << 32, 1.0), (-(9 << 32) - 1, 1.0), (0, complex(NAN, 0)), (0, complex(0, INF)), (0, 1e300)):
        with pytest.raises(ValueError):
            d.set(tau, s)
    with pytest.raises(ValueError):
        d.set(0.5)
    torch.cuda.synchronize()
    assert (host(out) == complex(3.0, 4.0)).all() and not host(buf).any()
    r = d.read()
    assert r["rows"] == 0 and not r["sums"].any() and r["tau_fp"] == 0 and r["updates"] == 0
    with pytest.raises(ValueError):
        d.execute(buf[:2 * halo - 1])
    with pytest.raises(ValueError):
        d.measure(buf[:10], buf[:11])
    with pytest.raises(TypeError):
        d16.execute(buf)
    with pytest.raises(ValueError):
        d.align(buf[:100], buf[:99])
    assert int(d.execute(buf[:2 * halo]).shape[0]) == 0
    d.close(); d16.close()


def test_the_guard_on_the_device(product):
    """the handle's own count of the rows offered: a call that would take it above 2^31 is refused before a buffer is looked at, measures
    nothing and leaves the count as it was; update and reset clear it"""
    torch = _torch()
    L, OK, EINVAL = product.lib(), product.MCRX_OK, product.MCRX_EINVAL
    most = 1 << product.FBALIGN_GUARD_LOG2
    d, m = product.fbalign(8, 1.0, 1.0, min_rows=1), model.Model(8, 1.0, 1.0, min_rows=1, W32=library_table(product))
    R = d.R
    x = band_limited(300, 0.5, 6)
    xd = dev(x)
    p = xd.data_ptr()

    def measure(k):
        return L.mcrx_hip_fbalign_measure_device(d._h, C.c_void_p(p), C.c_void_p(p), k, None)

    assert measure(most + 2 * R + 1) == EINVAL and b"2^31" in L.mcrx_hip_fbalign_last_error()
    assert d.read()["offered"] == 0
    assert d.measure(xd[:2 * R + 40], xd[:2 * R + 40]) == 40 and m.measure(x[:2 * R + 40], x[:2 * R + 40])
    assert measure(most - 40 + 1 + 2 * R) == EINVAL and b"2^31" in L.mcrx_hip_fbalign_last_error()      # 40 + (2^31 - 39) rows
    r = d.read()
    assert (r["offered"], r["rows"]) == (40, 40) == (m.since, m.rows)
    same_sums(r, m)
    assert d.measure(xd, xd) == 300 - 2 * R and m.measure(x, x)                             # the next call that fits is accepted
    r = d.read()
    assert r["offered"] == r["rows"] == 340 - 2 * R == m.since
    same_sums(r, m)
    assert measure(2 * R) == OK and measure(0) == OK and d.read()["offered"] == 340 - 2 * R    # no rows: nothing counted
    d.update(); m.update()
    r = d.read()
    assert (r["offered"], r["rows"], r["updates"]) == (0, 0, 1) == (m.since, m.rows, m.updates)   # an update clears the count with the sums
    assert measure(most + 2 * R + 1) == EINVAL and d.read()["offered"] == 0
    assert d.measure(xd, xd) == 300 - 2 * R and d.read()["offered"] == 300 - 2 * R
    assert measure(most - (300 - 2 * R) + 1 + 2 * R) == EINVAL
    d.reset()                                                                              # (a refusal comes before the pending reset is served)
    assert measure(most + 2 * R + 1) == EINVAL
    r = d.read()
    assert (r["offered"], r["rows"], r["updates"]) == (0, 0, 0) and not r["sums"].any()
    assert d.measure(xd[:2 * R + 7], xd[:2 * R + 7]) == 7 and d.read()["offered"] == 7 and d.read()["rows"] == 7
    torch.cuda.synchronize()
    d.close()


# ---------------------------------------------------------------------------------------------- 7. the closed loops
class Observed(object):
    """an amplifier seen through an observation receiver: its output late by tau samples (a float64 fractional delay in the frequency
    domain of the circularly extended stream, on the host), times the gain, plus noise at snr_db, quantised to sc16 -- or, with
    whole=True, that capture moved back by the whole samples and divided by the gain, as cf32"""

    def __init__(self, amp, v, whole=False):
        self.amp, self.v, self.whole, self.calls = amp, v, whole, 0

    def execute(self, u, first_sample=0, stream=None):
        torch, v = _torch(), self.v
        z = host(self.amp.execute(u, first_sample, stream=stream)).astype(np.complex128)
        nstd = cfr_model.rms(z) * abs(v["gain"]) * 10.0 ** (-v["snr_db"] / 20.0) / np.sqrt(2.0)
        cap = model.path(z, v["tau"], v["gain"], nstd, seed=self.calls)
        self.calls += 1
        q = model.to_sc16(cap)
        assert np.abs(q).max() < 32767
        if not self.whole:
            return torch.from_numpy(q).cuda()
        back = q.astype(np.float32).view(np.complex64).reshape(-1) * np.float32(2.0 ** -15)
        return dev((np.roll(back, -int(round(v["tau"]))) / v["gain"]).astype(np.complex64))


def receive(product, oracle, s, sent, y):
    """the GPU receiver and the oracle on y: every frame valid on both sides with its bytes as sent; (max-norm, element-wise) of the symbols"""
    from test_gpu_parity import match_frames, relerr, relerr_elem
    N, nf = s["N"], s["frames"]
    n = int(y.numel()) // (product.TILE * 2 * N) * (product.TILE * 2 * N)
    y = y[:n].contiguous()
    rx = product.multichannelrx(N, s["M"], s["cp"], s["taper"], max_payload_len=s["payload_len"])
    rx.Execute(y); rx.Flush()
    ora = oracle.MultiChannelRx(N, s["M"], s["cp"], s["taper"])
    ora.execute(np.ascontiguousarray(host(y)))
    for side, frames in (("gpu", rx.frames), ("oracle", ora.frames)):
        assert len(frames) == N * nf == 24, (side, len(frames))
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
    rx.close()
    return w, we


@pytest.mark.parametrize("kind", ["dpd", "mpd"])
def test_closed_loop_on_the_device(product, oracle, kind):
    """multichanneltx -> cfr -> predistorter -> amplifier -> the host-made path (7.37 samples, 0.6 e^{1.1j}, 50 dB SNR, sc16) -> fbalign
    -> measure, three rounds through _Predistorter.learn(aligner=); the same with direct feedback and with whole-sample alignment only.
    dpd on rfchain's amplifier, mpd on mpd_model.SEVERITY's three-branch amplifier.  Asserted, at what tests/test_fbalign.py recorded
    on the oracle's stream less 6 dB (the slack the mpd test grants the device transmitter's different payload stream): the power at
    |f| > 0.32 through the aligner is better than with whole-sample alignment by the recorded gain less 6 dB, and within the recorded
    margin plus 6 dB of direct feedback; the power through the aligner and the NMSE after delay and gain removal are each within 6 dB
    of the recorded figure; on the memoryless amplifier tau is within tau_tol of 7.37; all 24 frames valid on the GPU
    receiver and on the oracle with identical bytes, the symbols within 1e-3."""
    torch = _torch()
    s, v, dd, dm = cfr_model.SEVERITY, model.SEVERITY, dpd_model.SEVERITY, mpd_model.SEVERITY
    rec = v[kind]
    N = s["N"]
    tx = product.multichanneltx(N, s["M"], s["cp"], s["taper"])
    iq, sent = tx.generate(s["frames"], s["payload_len"], seed=77 + N)
    tx.close()
    rms = rms_of(torch, iq)
    h = product.cfr_lowpass(s["half_len"], s["cutoff"], s["beta"])
    cf = product.cfr(float(np.float32(product.cfr_threshold(s["papr_db"], rms))), taps=h, passes=s["passes"])
    x = cf.execute(iq, pad=True)
    cf.close()
    peak = float(x.abs().max())
    if kind == "dpd":
        amp = product.rfchain(amplifier=dict(sat=product.rfchain_backoff(dd["amp_ibo_db"], rms), smooth=dd["amp_smooth"], gain=dd["amp_gain"],
                                             ampm_deg=dd["amp_ampm_deg"]))
        fs, g0, pad = dd["full_scale_over_peak"] * peak, dd["amp_gain"], {}
    else:
        amp = MemoryAmplifier(product, rms)
        fs, g0, pad = dm["full_scale_over_peak"] * peak, dm["amp_gain"], dict(pad=True)
    oob, tau, y, al_state = {}, None, None, None
    for mode in ("direct", "whole", "aligned"):
        pd = product.dpd(dd["table_log2"], fs, g0) if kind == "dpd" else product.mpd(dm["branches"], dm["delays"], dm["order"], dm["table_log2"], fs, g0)
        if mode == "direct":
            pd.learn(x, amp, v["rounds"])
        elif mode == "whole":
            pd.learn(x, Observed(amp, v, whole=True), v["rounds"])
        else:
            al = product.fbalign(v["max_lag"], fs * g0, g0, v["min_rows"], input_format="sc16")
            pd.learn(x, Observed(amp, v), v["rounds"], aligner=al)
            al_state = al.read()
            al.close()
        y = amp.execute(pd.execute(x, **pad))
        oob[mode] = oob_of(torch, y, v["edge"])
        assert pd.read()["degenerate"] == 0 and pd.read()["updates"] == v["rounds"]
        pd.close()
    tau = al_state["tau"]
    nmse = model.nmse_aligned_db(host(y), g0 * host(x).astype(np.complex128))
    gain_db, margin_db = rec["oob_db"]["whole"] - rec["oob_db"]["aligned"] - v["device_slack_db"], rec["oob_margin_db"] + v["device_slack_db"]
    print("fbalign closed loop, %s: %d samples; power at |f| > %.2f direct / aligned / whole %.2f / %.2f / %.2f dB (asserted: %.2f dB better than whole, within "
          "%.2f dB of direct); NMSE after delay and gain removal %.2f dB; tau %.7f, s %s, clamped %d"
          % (kind, int(x.numel()), v["edge"], oob["direct"], oob["aligned"], oob["whole"], gain_db, margin_db, nmse, tau, al_state["s"], al_state["clamped"]))
    assert al_state["degenerate"] == 0 and al_state["updates"] == v["rounds"] * v["align_rounds"] and al_state["clamped"] == 0
    assert oob["whole"] - oob["aligned"] >= gain_db
    assert oob["aligned"] <= oob["direct"] + margin_db
    assert oob["aligned"] <= rec["oob_db"]["aligned"] + v["device_slack_db"]
    assert nmse <= rec["nmse_db"]["aligned"] + v["device_slack_db"]
    if kind == "dpd":
        assert abs(tau - v["tau"]) <= v["tau_tol"], tau
    w, we = receive(product, oracle, s, sent, y)
    amp.close()
    PARITY[kind] = {"max_norm": w, "element_wise": we, "oob_db": oob, "nmse_aligned_db": nmse, "tau": tau, "s": [al_state["s"].real, al_state["s"].imag]}
    print("fbalign_parity %s: framesyms max-norm %.3e element-wise %.3e" % (kind, w, we))
    assert w <= 1e-3, w


def test_zz_print_fbalign_figures():
    """(last of this file: the figures measured above as one JSON line -- profiles/fbalign_parity.json is such a record; FBALIGN_PARITY_OUT
    names a file to write it to as well)"""
    line = json.dumps(PARITY, sort_keys=True)
    print("fbalign_parity " + line)
    path = os.environ.get("FBALIGN_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")
