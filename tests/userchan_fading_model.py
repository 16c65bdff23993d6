"""The per-user channel emulator's fading rays (include/mcrx_hip.h, mcrx_hip_userfade_*) as numpy in float64 --
except the phases, which are exact 64-bit integers (tests/chanemu_fading_model.py's grid()).

    B = 2^L, row = b >> L (arithmetic: b is signed), n_r = (row << L) mod 2^64, f = (b & (B - 1)) 2^-L
    G_ci[row] = c_los e((psi << 32) + Lambda n_r) + c_sc sum_{k<S} e((Phi_k << 32) + N_k n_r)
    g_ci(b)   = G_ci[row] + f (G_ci[row + 1] - G_ci[row])
    s_c[b]    = sum_i (g_ci(b) a_ci) x_c[b - d_ci]
and what follows s_c[b] (rotation, gain) is userchan_model's.

A ray's table is (steps, phases, coef) as in chanemu_fading_model; tables() makes them from the fading seed and the user's id the way
the library does -- Philox counter (k, ray, 2, id) -- and the GPU tests feed the model with the integers the library itself reports.
A user without fading inside a fading handle has STATIC rays: G = 1."""
import numpy as np

import chanemu_fading_model as fmodel
import userchan_model as model

philox4x32_10 = fmodel.base.philox4x32_10


def static_table(S):
    return ([0] * (S + 1), [0] * (S + 1), (1.0, 0.0))


def tables(seed, uid, doppler, los_doppler, rice_k, los_phase, S):
    """one table per ray of the user with id `uid`: the words of counter (k, i, 2, uid), alpha = 2 pi (k + w0 2^-32) / S"""
    out = []
    for i in range(len(doppler)):
        k = np.arange(S, dtype=np.uint64)
        w = philox4x32_10((k, i, 2, int(uid)), (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
        alpha = 2.0 * np.pi * (k.astype(np.float64) + w[0].astype(np.float64) * 2.0 ** -32) / float(S)
        steps = [int(np.rint(float(los_doppler[i]) * 2.0 ** 64))] + [int(v) for v in np.rint(float(doppler[i]) * np.cos(alpha) * 2.0 ** 64)]
        phases = [int(los_phase[i]) & 0xFFFFFFFF] + [int(v) for v in w[1]]
        K = float(np.float32(rice_k[i]))
        coef = (float(np.float32(np.sqrt(K / (K + 1.0)))), float(np.float32(np.sqrt(1.0 / ((K + 1.0) * S)))))
        out.append((steps, phases, coef))
    return out


def grid_rows(table, first_row, rows, L):
    """G[first_row .. first_row + rows) for a signed first row, complex128"""
    r = [(int(first_row) + j) & ((1 << (64 - L)) - 1) for j in range(int(rows))]
    return fmodel.grid(table, np.array(r, dtype=np.uint64), L)


def gain(table, first_block, count, L):
    """g(b) for b = first_block .. first_block + count - 1 (signed), complex128; also the largest |G| of the rows it used"""
    b = np.arange(count, dtype=np.int64) + np.int64(first_block)
    row = b >> np.int64(L)
    rel = row - row[0]
    G = grid_rows(table, int(row[0]), int(rel.max()) + 2, L)
    f = (b & np.int64((1 << L) - 1)).astype(np.float64) * 2.0 ** -L
    return G[rel] + f * (G[rel + 1] - G[rel]), float(np.abs(G).max())


def apply_channel(x, ch, tabs, L, first_block, lead):
    """x: the channel's samples of blocks [first_block - lead, first_block + n) -> (y of blocks [first_block, first_block + n) as
    complex128, [the largest |G| per ray]); tabs: one table per ray, or None for a user without fading"""
    x = np.asarray(x, np.complex128)
    n = len(x) - lead
    rays = model.rays_of(ch)
    if tabs is None:
        return model.apply_channel(x, ch, first_block, lead), [1.0] * len(rays)
    s = np.zeros(n, np.complex128)
    peaks = []
    for (d, a), t in zip(rays, tabs):
        assert 0 <= d <= lead
        g, pk = gain(t, first_block, n, L)
        peaks.append(pk)
        s += (g * a) * x[lead - d:lead - d + n]
    return model.apply_channel(s, dict(ch, taps=[(0, 1.0)], delay=0), first_block, 0), peaks


def bound(ch, tabs, peaks, S, x):
    """Per component, for one channel.  userchan_model.bound with every |a_i| scaled by that ray's largest |G| (peaks), plus E_g, the
    error of the fp32 g_i(b) a_i relative to |a_i|, derived as fade_bound of tests/test_gpu_chanemu_fading.py derives it: with
    Gs = c_los + S c_sc >= every partial sum of G and |g|: sincos_u32's stated error on every term and the rounding of the line-of-sight
    product, Gs (3e-7 + 2^-24); S roundings of the sum's fused multiply-adds, 2 of the interpolation (the difference of the rows and one
    fused multiply-add) and 2 of the product g a (cmul_fx), each at most 2^-24 Gs, and one more for the table entry: (S + 5) 2^-24 Gs."""
    rays = model.rays_of(ch)
    T = len(rays)
    if tabs is None:
        return model.bound(ch, x)
    total = 0.0
    for (_, a), t, pk in zip(rays, tabs, peaks):
        gs = t[2][0] + S * t[2][1]
        e_g = gs * (3e-7 + 2.0 ** -24) + (S + 5) * 2.0 ** -24 * gs
        total += abs(a) * (((2 * T + 8) * 2.0 ** -24 + 3e-7) * pk + e_g)
    return total * model.gain_of(ch) * float(np.abs(x).max())
