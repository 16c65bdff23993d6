// fbalign.hip -- feedback alignment for the predistorters on gfx950: the observation receiver's capture of the amplifier's output
// brought back onto the amplifier's input in delay (whole samples and a fraction), gain and phase, all learned on the device; cf32 or
// sc16 in, cf32 out (mcrx_hip_fbalign_*; the definition with every operation is in include/mcrx_hip.h).
//
// The handle owns one device block: the state (tau_fp, s, res, counters, and what apply reads: the 32 coefficients, nd, the fp32
// scale), the interpolator's table W[65][32] (interp_table.hpp: userclock's) and the 2 R + 19 complex int64 sums.  Nothing of it is
// read back by a launch's host side.
// fbalign_apply_kernel<FIN>: the coefficients are the same for every sample of a call, so this is a 32-tap real-by-complex FIR whose
// coefficients, offset and scale are uniform loads from the state: they live in scalar registers.  A workgroup stages the 546 samples
// its 512 outputs need in LDS as floats (an sc16 capture is converted on the way in), then a lane owns an index-aligned pair of
// outputs -- iqpair.hpp's layout, one 16-byte store -- and reads its 34 samples as 17 16-byte LDS words.
// fbalign_copy_kernel<FIN>: the handle that has learned nothing: load in[halo + i], convert, store.
// fbalign_measure_kernel: a workgroup stages a tile of 256 rows -- U with 16 samples behind it, Z with R on either side -- in LDS as
// int16 pairs; lane t < 2 R + 19 owns one sum (a lag of C, a lag of A, or Szz) and walks the tile's rows: the U[i] read is a
// broadcast, the Z[i + l] reads of neighbouring lanes are neighbouring banks.  The lane keeps its sum in int64 registers over all the
// workgroup's tiles and flushes it with one pair of atomics.
// fbalign_update_kernel: one lane, fp64.  fbalign_state_kernel: the reset, or a set.
//
// Contraction is switched off for this file, as in mpd.hip: the update is the + - * / sequence a float64 model reproduces.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>
#include <string>
#include "../../include/mcrx_hip.h"
#include "fbalign_plan.hpp"
#include "iqpair.hpp"
#include "ophost.hpp"
#include "stream_call.hpp"

namespace mcrx {

struct FbState {                                            // device; W and the sums lie behind it
    long long tau_fp;
    double s_re, s_im, res;
    unsigned long long updates, degenerate, clamped;
    long long rows;
    float coef[FBA_TAPS];                                   // what apply reads: c_0 .. c_31, the scale as fp32, nd
    float sc_re, sc_im;
    int nd, pad_;
};

struct FbApply {
    const void *in; float2 *out;                            // in: the call's d_in (output 0's sample is in[halo])
    uint64_t parity, n;                                     // (address of out[0] / 8) & 1; outputs of this launch
    uint32_t halo, Lm;
};

template <int FIN> __device__ __forceinline__ float2 fbalign_load(const void *in, long long j)
{
    if (FIN == IQ_SC16) return sc16_unpack(reinterpret_cast<const uint32_t *>(in)[j]);
    return reinterpret_cast<const float2 *>(in)[j];
}

template <int FIN>
__global__ __launch_bounds__(FBA_WG) void fbalign_apply_kernel(FbApply a, const FbState *__restrict__ st)
{
    __shared__ __attribute__((aligned(16))) float2 win[FBA_WIN];
    const int most = (int)a.Lm + 1;
    int nd = st->nd;
    nd = nd < -most ? -most : (nd > most ? most : nd);                  // (held there whatever the state is: no tap leaves the input)
    const long long total = (long long)a.n + 2ll * a.halo;
    // slot k of the window is the input sample first + k; output m's tap j is in[halo + m - nd + 15 - j] = slot (m - mb) + 31 - j
    const long long mb = 2ll * ((long long)blockIdx.x * FBA_WG) - (long long)(a.parity & 1u);       // the workgroup's first output (-1: masked)
    const long long first = mb + (long long)a.halo - nd - 16;
    for (uint32_t k = threadIdx.x; k < (uint32_t)FBA_WIN; k += FBA_WG) {
        const long long j = first + k;
        float2 v = make_float2(0.f, 0.f);
        if (j >= 0 && j < total) v = fbalign_load<FIN>(a.in, j);
        win[k] = v;
    }
    __syncthreads();
    const IqPair p = iq_pair(a.parity, a.n, (uint64_t)blockIdx.x * FBA_WG + threadIdx.x);
    float2 x[FBA_TAPS + 2];                                             // slots 2 t .. 2 t + 33
    const float4 *w4 = reinterpret_cast<const float4 *>(win + 2u * threadIdx.x);
#pragma unroll
    for (int q = 0; q < (FBA_TAPS + 2) / 2; q++) {
        const float4 v = w4[q];
        x[2 * q] = make_float2(v.x, v.y); x[2 * q + 1] = make_float2(v.z, v.w);
    }
    float2 a0 = make_float2(0.f, 0.f), a1 = a0;
#pragma unroll
    for (int j = 0; j < FBA_TAPS; j++) {
        const float c = st->coef[j];
        a0.x = fmaf(c, x[31 - j].x, a0.x); a0.y = fmaf(c, x[31 - j].y, a0.y);
        a1.x = fmaf(c, x[32 - j].x, a1.x); a1.y = fmaf(c, x[32 - j].y, a1.y);
    }
    const float sr = st->sc_re, si = st->sc_im;
    const float2 v0 = make_float2(fmaf(sr, a0.x, -(si * a0.y)), fmaf(sr, a0.y, si * a0.x));
    const float2 v1 = make_float2(fmaf(sr, a1.x, -(si * a1.y)), fmaf(sr, a1.y, si * a1.x));
    (void)store_pair<IQ_CF32>(a.out, p, v0, v1);
}

template <int FIN>
__global__ __launch_bounds__(FBA_WG) void fbalign_copy_kernel(FbApply a)
{
    const IqPair p = iq_pair(a.parity, a.n, (uint64_t)blockIdx.x * FBA_WG + threadIdx.x);
    float2 v0, v1;
    if (FIN == IQ_SC16) load_pair<IQ_SC16>(reinterpret_cast<const uint32_t *>(a.in) + a.halo, p, v0, v1);
    else                load_pair<IQ_CF32>(reinterpret_cast<const float2 *>(a.in) + a.halo, p, v0, v1);
    (void)store_pair<IQ_CF32>(a.out, p, v0, v1);
}

struct FbMeasure {
    const float2 *u, *z;
    unsigned long long *sums;                               // 2 (2 R + 19): (re, im) of C[-R .. R], A[0 .. 16], (Szz, 0)
    FbState *state;
    uint64_t n, rows, tiles;
    uint32_t R; int e;
};

#define FBA_USPAN (FBA_TILE + 2 * FBA_H)                    // U of a tile: its rows and 16 samples behind them
#define FBA_ZSPAN (FBA_TILE + 2 * FBA_MAX_R)                // Z of a tile: its rows and R samples on either side (the most)

__global__ __launch_bounds__(FBA_WG) void fbalign_measure_kernel(FbMeasure a)
{
    __shared__ uint32_t tile[FBA_USPAN + FBA_ZSPAN];
    const uint32_t t = threadIdx.x, R = a.R, nl = 2u * R + 1u, zspan = (uint32_t)FBA_TILE + 2u * R;
    uint32_t *U = tile, *Z = tile + FBA_USPAN;
    // this lane's sum of conj(tile[ia + r]) tile[ib + r] over the rows r: a lag of C, a lag of A, or Szz
    const bool own = t < nl + 2u * (uint32_t)FBA_H + 2u;
    uint32_t ia = 0u, ib = 0u;
    if (t < nl) ib = (uint32_t)FBA_USPAN + t;                           // U[i], Z[i + (t - R)]
    else if (t < nl + 2u * (uint32_t)FBA_H + 1u) ib = t - nl;           // U[i], U[i + (t - nl)]
    else ia = ib = (uint32_t)FBA_USPAN + R;                             // Z[i], Z[i]
    long long sre = 0, sim = 0;
    uint32_t nbad = 0;
    unsigned long long nrows = 0;
    for (uint64_t tl = blockIdx.x; tl < a.tiles; tl += gridDim.x) {
        const uint64_t i0 = (uint64_t)R + tl * FBA_TILE, left = a.rows - tl * FBA_TILE;     // the tile's first row; (tl < tiles: at least one row)
        const uint32_t nr = left < (uint64_t)FBA_TILE ? (uint32_t)left : (uint32_t)FBA_TILE;
        for (uint32_t s = t; s < (uint32_t)FBA_USPAN; s += FBA_WG) {
            const uint64_t j = i0 + s;
            uint32_t w = 0u;
            bool bad = false;
            if (j < a.n) { const float2 v = a.u[j]; w = fbalign_word(v.x, v.y, a.e, &bad); }
            U[s] = w;
            nbad += (bad && s < nr) ? 1u : 0u;
        }
        for (uint32_t s = t; s < zspan; s += FBA_WG) {
            const uint64_t j = i0 - R + s;
            uint32_t w = 0u;
            bool bad = false;
            if (j < a.n) { const float2 v = a.z[j]; w = fbalign_word(v.x, v.y, a.e, &bad); }
            Z[s] = w;
            nbad += (bad && s >= R && s < R + nr) ? 1u : 0u;
        }
        __syncthreads();
        if (own) {
#pragma unroll 4
            for (uint32_t r = 0; r < nr; r++) {
                const uint32_t wa = tile[ia + r], wb = tile[ib + r];
                const int ar = (int)(int16_t)(wa & 0xffffu), ai = (int)wa >> 16, br = (int)(int16_t)(wb & 0xffffu), bi = (int)wb >> 16;
                sre += (long long)(ar * br) + (long long)(ai * bi);     // (a product is at most 2^30)
                sim += (long long)(ar * bi) - (long long)(ai * br);
            }
        }
        if (t == 0u) nrows += nr;
        __syncthreads();                                                // the tile is restaged
    }
    sc16_clip_commit(&a.state->clamped, nbad);                          // (the wave's sum, one atomic from its first lane, none for 0)
    if (t == 0u && nrows) atomicAdd(reinterpret_cast<unsigned long long *>(&a.state->rows), nrows);
    if (own) {
        if (sre) atomicAdd(&a.sums[2u * t], (unsigned long long)sre);   // (two's complement: the unsigned add is the signed one)
        if (sim) atomicAdd(&a.sums[2u * t + 1u], (unsigned long long)sim);
    }
}

__device__ __forceinline__ bool fba_finite(double v) { return v - v == 0.0; }

// tau_fp and s into the state, with what apply reads of them
__device__ __forceinline__ void fbalign_commit(FbState *st, const float *W, long long tau_fp, double s_re, double s_im)
{
    st->tau_fp = tau_fp; st->s_re = s_re; st->s_im = s_im;
    fbalign_coefs(W, tau_fp, st->coef);
    st->sc_re = (float)s_re; st->sc_im = (float)s_im;
    st->nd = fbalign_split(tau_fp).nd;
}

struct FbUpdate {
    FbState *state; const float *W; long long *sums;
    uint32_t Lm, R, nsums, min_rows;
    double g0, h[FBA_H];
};

// The update (include/mcrx_hip.h), lane 0 of one workgroup; the other lanes clear the sums behind it.
__global__ __launch_bounds__(FBA_WG) void fbalign_update_kernel(FbUpdate u)
{
    if (threadIdx.x == 0) {
        FbState *st = u.state;
        const long long *C = u.sums + 2ll * u.R, *A = u.sums + 2ll * (2u * u.R + 1u);      // C[2 l], C[2 l + 1]: lag l; A likewise
        const int Lm = (int)u.Lm;
        bool ok = st->rows >= (long long)u.min_rows;
        int D = -Lm;
        if (ok) {
            double best = -1.0;
            for (int l = -Lm; l <= Lm; l++) {
                const double cr = (double)C[2 * l], ci = (double)C[2 * l + 1];
                const double p = cr * cr + ci * ci;
                if (p > best) { best = p; D = l; }
            }
            ok = best > 0.0;
        }
        if (ok) {
            const double bur = (double)C[2 * D], bui = (double)C[2 * D + 1];
            double bdr = 0.0, bdi = 0.0, g = 0.0;
            for (int k = 1; k <= FBA_H; k++) {
                const double tr = (double)C[2 * (D + k)] - (double)C[2 * (D - k)], ti = (double)C[2 * (D + k) + 1] - (double)C[2 * (D - k) + 1];
                bdr = bdr + u.h[k - 1] * tr;
                bdi = bdi + u.h[k - 1] * ti;
            }
            const double Guu = (double)A[0];
            for (int k = 1; k <= FBA_H; k++) g = g + u.h[k - 1] * (double)A[2 * k + 1];
            const double gud = -2.0 * g;
            double Gdd = 0.0;
            for (int k = -FBA_H; k <= FBA_H; k++) {
                if (k == 0) continue;
                const double hk = k > 0 ? u.h[k - 1] : -u.h[-k - 1];
                for (int m = -FBA_H; m <= FBA_H; m++) {
                    if (m == 0) continue;
                    const double hm = m > 0 ? u.h[m - 1] : -u.h[-m - 1];
                    const int l = k > m ? k - m : m - k;
                    Gdd = Gdd + (hk * hm) * (double)A[2 * l];
                }
            }
            const double det = Guu * Gdd - gud * gud;
            ok = det > 0.0;
            if (ok) {
                const double alr = (Gdd * bur + gud * bdi) / det, ali = (Gdd * bui - gud * bdr) / det;
                const double ber = (Guu * bdr - gud * bui) / det, bei = (Guu * bdi + gud * bur) / det;
                const double m2 = alr * alr + ali * ali;
                const double delta = -((ber * alr + bei * ali) / m2);
                const double xr = st->s_re * u.g0, xi = st->s_im * u.g0;
                const double nsr = (xr * alr + xi * ali) / m2, nsi = (xi * alr - xr * ali) / m2;
                const double res = (double)u.sums[2u * (u.nsums - 1u)] - (alr * bur + ali * bui);
                const float fr = (float)nsr, fi = (float)nsi;
                ok = fba_finite(delta) && fba_finite(nsr) && fba_finite(nsi) && fba_finite(res) && fr - fr == 0.f && fi - fi == 0.f
                     && delta <= 1.0 && delta >= -1.0;
                if (ok) {
                    const long long tau = st->tau_fp + (long long)rint(((double)D + delta) * 4294967296.0);
                    ok = fbalign_tau_ok(tau, u.Lm);
                    if (ok) { fbalign_commit(st, u.W, tau, nsr, nsi); st->res = res; }
                }
            }
        }
        if (!ok) st->degenerate += 1;
        st->updates += 1;
        st->rows = 0;
    }
    __syncthreads();                                                    // lane 0 has read the sums
    for (uint32_t b = threadIdx.x; b < 2u * u.nsums; b += FBA_WG) u.sums[b] = 0;
}

// reset != 0: tau_fp := 0, s := 1, res, sums and counters := 0; else a set: tau_fp and s as given, the rest stays
__global__ __launch_bounds__(FBA_WG) void fbalign_state_kernel(FbState *st, const float *W, long long *sums, uint32_t nsums, uint32_t reset, long long tau_fp,
                                                               double s_re, double s_im)
{
    if (reset)
        for (uint32_t b = threadIdx.x; b < 2u * nsums; b += FBA_WG) sums[b] = 0;
    if (threadIdx.x == 0) {
        if (reset) { st->res = 0.0; st->updates = 0; st->degenerate = 0; st->clamped = 0; st->rows = 0; tau_fp = 0; s_re = 1.0; s_im = 0.0; }
        fbalign_commit(st, W, tau_fp, s_re, s_im);
    }
}

}  // namespace mcrx

using namespace mcrx;

static thread_local std::string g_fba_err;

struct mcrx_hip_fbalign_s {
    int device = -1;            // the HIP device the handle was created on: every entry point runs with it current (devscope.hpp)
    mcrx_hip_fbalign_config cfg;
    FbalignConsts k;
    char *mem = nullptr;        // one device block: FbState | W[65][32] | the sums
    FbState *state = nullptr; float *W = nullptr; long long *sums = nullptr;
    uint64_t since = 0;         // rows offered since the last update or reset (the guard)
    bool trained = false;       // an update or a set has been enqueued since the reset: launches carry the filter
    bool reset_pending = false; // the next kernel that touches the state clears it first
};

// the state cleared if a reset is pending: in front of every kernel that reads or writes it
static hipError_t fbalign_serve_reset(mcrx_hip_fbalign_t q, hipStream_t st)
{
    if (!q->reset_pending) return hipSuccess;
    hipLaunchKernelGGL(fbalign_state_kernel, dim3(1), dim3(FBA_WG), 0, st, q->state, q->W, q->sums, q->k.sums, 1u, 0ll, 1.0, 0.0);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) q->reset_pending = false;
    return e;
}

extern "C" const char *mcrx_hip_fbalign_last_error(void) { return g_fba_err.c_str(); }

extern "C" int mcrx_hip_fbalign_selftest(const mcrx_hip_fbalign_config *cfg, int *e, float *taps, const float *v, size_t n, int32_t *q15, int32_t *bad,
                                         int64_t tau_fp, float *coef, int *nd)
{
    if (!cfg || (n && (!v || !q15 || !bad))) { g_fba_err = "null pointer"; return MCRX_EINVAL; }
    if (const char *why = fbalign_check(cfg)) { g_fba_err = why; return MCRX_EINVAL; }
    const FbalignConsts k = fbalign_consts(cfg);
    if (e) *e = k.e;
    if (taps) for (int i = 0; i < FBA_H; i++) taps[i] = k.h[i];
    for (size_t i = 0; i < n; i++) {
        bool b = false;
        q15[i] = fbalign_q15(v[i], k.e, &b);
        bad[i] = b ? 1 : 0;
    }
    if (coef) {
        if (!fbalign_tau_ok(tau_fp, k.Lm)) { g_fba_err = "tau_fp lies outside (max_lag + 1) samples"; return MCRX_EINVAL; }
        fbalign_coefs(userclock_table(), tau_fp, coef);
        if (nd) *nd = fbalign_split(tau_fp).nd;
    }
    return MCRX_OK;
}

extern "C" int mcrx_hip_fbalign_create(mcrx_hip_fbalign_t *out, const mcrx_hip_fbalign_config *cfg)
{
    if (!out) { g_fba_err = "null pointer"; return MCRX_EINVAL; }
    *out = nullptr;
    if (!cfg) { g_fba_err = "null configuration"; return MCRX_EINVAL; }
    if (const char *bad = fbalign_check(cfg)) { g_fba_err = bad; return MCRX_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { g_fba_err = "no HIP device (no CPU fallback)"; return MCRX_EHIP; }
    mcrx_hip_fbalign_t q = new mcrx_hip_fbalign_s();
    q->cfg = *cfg;
    q->k = fbalign_consts(cfg);
    q->device = current_device();
    const size_t wn = (size_t)(MCRX_USERCLOCK_PHASES + 1) * MCRX_USERCLOCK_TAPS;
    const size_t o_W = (sizeof(FbState) + 15u) & ~(size_t)15u, o_sums = o_W + wn * sizeof(float), bytes = o_sums + 2 * (size_t)q->k.sums * sizeof(long long);
    hipError_t e = hipMalloc((void **)&q->mem, bytes);
    if (e == hipSuccess) e = hipMemset(q->mem, 0, bytes);
    if (e == hipSuccess) e = hipMemcpy(q->mem + o_W, userclock_table(), wn * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        g_fba_err = std::string("device state: ") + hipGetErrorString(e);
        (void)hipDeviceSynchronize();
        if (q->mem) (void)hipFree(q->mem);
        delete q;
        return MCRX_EHIP;
    }
    q->state = reinterpret_cast<FbState *>(q->mem);
    q->W = reinterpret_cast<float *>(q->mem + o_W);
    q->sums = reinterpret_cast<long long *>(q->mem + o_sums);
    q->reset_pending = true;                                            // s = 1 and the unit coefficients before anything reads them
    *out = q;
    return MCRX_OK;
}

extern "C" int mcrx_hip_fbalign_destroy(mcrx_hip_fbalign_t q)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) return MCRX_OK;
    (void)hipDeviceSynchronize();
    if (q->mem) (void)hipFree(q->mem);
    delete q;
    return MCRX_OK;
}

extern "C" unsigned mcrx_hip_fbalign_halo(mcrx_hip_fbalign_t q) { return q ? q->k.halo : 0u; }
extern "C" unsigned mcrx_hip_fbalign_input_format(mcrx_hip_fbalign_t q) { return q ? q->cfg.input_format : 0u; }

extern "C" int mcrx_hip_fbalign_reset(mcrx_hip_fbalign_t q)
{
    if (!q) { g_fba_err = "null handle"; return MCRX_EINVAL; }
    q->since = 0; q->trained = false; q->reset_pending = true;
    return MCRX_OK;
}

extern "C" int mcrx_hip_fbalign_execute_device(mcrx_hip_fbalign_t q, const void *d_in, size_t n, void *d_out, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_fba_err = "null handle"; return MCRX_EINVAL; }
    const bool in16 = q->cfg.input_format == IQ_SC16;
    const char *bad = stream_call_check(reinterpret_cast<uintptr_t>(d_in), reinterpret_cast<uintptr_t>(d_out), n, in16 ? 4u : 8u, 8u, 2ull * q->k.halo, false,
                                        false, "d_in and d_out overlap: a lane reads its neighbours' samples, so no overlap is allowed");
    if (bad) { g_fba_err = bad; return MCRX_EINVAL; }
    if (n == 0) return MCRX_OK;
    hipStream_t st = (hipStream_t)stream;
    FbApply a = {};
    a.in = d_in; a.out = reinterpret_cast<float2 *>(d_out);
    a.parity = (reinterpret_cast<uintptr_t>(d_out) >> 3) & 1u; a.n = n;
    a.halo = q->k.halo; a.Lm = q->k.Lm;
    const dim3 grid(fbalign_apply_grid(a.parity, n)), wg(FBA_WG);
    if (q->trained) {                                                   // (a reset still pending means not trained: the stale state is not read)
        if (in16) hipLaunchKernelGGL((fbalign_apply_kernel<IQ_SC16>), grid, wg, 0, st, a, (const FbState *)q->state);
        else      hipLaunchKernelGGL((fbalign_apply_kernel<IQ_CF32>), grid, wg, 0, st, a, (const FbState *)q->state);
    } else {
        if (in16) hipLaunchKernelGGL((fbalign_copy_kernel<IQ_SC16>), grid, wg, 0, st, a);
        else      hipLaunchKernelGGL((fbalign_copy_kernel<IQ_CF32>), grid, wg, 0, st, a);
    }
    MCRX_OP_CHK(g_fba_err, hipGetLastError());
    return MCRX_OK;
}

extern "C" int mcrx_hip_fbalign_measure_device(mcrx_hip_fbalign_t q, const void *d_u, const void *d_zh, size_t n, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_fba_err = "null handle"; return MCRX_EINVAL; }
    const uint64_t rows = fbalign_rows(n, q->k.R);
    const char *bad = stream_call_check(reinterpret_cast<uintptr_t>(d_u), 0, n, 8u, 8u, 0, false, true, "");
    if (!bad) bad = stream_call_check(reinterpret_cast<uintptr_t>(d_zh), 0, n, 8u, 8u, 0, false, true, "");
    if (!bad && !fbalign_guard_ok(q->since, rows)) bad = "more than 2^31 rows offered since the last update or reset: the int64 sums could overflow";
    if (bad) { g_fba_err = bad; return MCRX_EINVAL; }
    if (rows == 0) return MCRX_OK;
    hipStream_t st = (hipStream_t)stream;
    MCRX_OP_CHK(g_fba_err, fbalign_serve_reset(q, st));
    FbMeasure m = {};
    m.u = reinterpret_cast<const float2 *>(d_u); m.z = reinterpret_cast<const float2 *>(d_zh);
    m.sums = reinterpret_cast<unsigned long long *>(q->sums); m.state = q->state;
    m.n = n; m.rows = rows; m.tiles = fbalign_tiles(rows); m.R = q->k.R; m.e = q->k.e;
    hipLaunchKernelGGL(fbalign_measure_kernel, dim3(fbalign_measure_grid(rows)), dim3(FBA_WG), 0, st, m);
    MCRX_OP_CHK(g_fba_err, hipGetLastError());
    q->since += rows;
    return MCRX_OK;
}

extern "C" int mcrx_hip_fbalign_update(mcrx_hip_fbalign_t q, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_fba_err = "null handle"; return MCRX_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    MCRX_OP_CHK(g_fba_err, fbalign_serve_reset(q, st));
    FbUpdate p = {};
    p.state = q->state; p.W = q->W; p.sums = q->sums;
    p.Lm = q->k.Lm; p.R = q->k.R; p.nsums = q->k.sums; p.min_rows = q->cfg.min_rows; p.g0 = (double)q->cfg.target_gain;
    for (int i = 0; i < FBA_H; i++) p.h[i] = (double)q->k.h[i];
    hipLaunchKernelGGL(fbalign_update_kernel, dim3(1), dim3(FBA_WG), 0, st, p);
    MCRX_OP_CHK(g_fba_err, hipGetLastError());
    q->since = 0;
    q->trained = true;
    return MCRX_OK;
}

extern "C" int mcrx_hip_fbalign_set(mcrx_hip_fbalign_t q, int64_t tau_fp, double s_re, double s_im, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_fba_err = "null handle"; return MCRX_EINVAL; }
    if (!fbalign_tau_ok(tau_fp, q->k.Lm)) { g_fba_err = "tau_fp lies outside (max_lag + 1) samples"; return MCRX_EINVAL; }
    if (!std::isfinite(s_re) || !std::isfinite(s_im) || !std::isfinite((float)s_re) || !std::isfinite((float)s_im)) { g_fba_err = "s must be finite as fp32"; return MCRX_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    MCRX_OP_CHK(g_fba_err, fbalign_serve_reset(q, st));
    hipLaunchKernelGGL(fbalign_state_kernel, dim3(1), dim3(FBA_WG), 0, st, q->state, q->W, q->sums, q->k.sums, 0u, (long long)tau_fp, s_re, s_im);
    MCRX_OP_CHK(g_fba_err, hipGetLastError());
    q->trained = true;
    return MCRX_OK;
}

extern "C" int mcrx_hip_fbalign_read(mcrx_hip_fbalign_t q, mcrx_hip_fbalign_state *state, float *coef, int64_t *sums, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_fba_err = "null handle"; return MCRX_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    MCRX_OP_CHK(g_fba_err, fbalign_serve_reset(q, st));
    FbState s = {};
    if (state || coef) MCRX_OP_CHK(g_fba_err, hipMemcpyAsync(&s, q->state, sizeof(s), hipMemcpyDeviceToHost, st));
    if (sums) MCRX_OP_CHK(g_fba_err, hipMemcpyAsync(sums, q->sums, 2 * (size_t)q->k.sums * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    MCRX_OP_CHK(g_fba_err, hipStreamSynchronize(st));
    if (state) {
        state->tau_fp = s.tau_fp; state->s_re = s.s_re; state->s_im = s.s_im; state->res = s.res;
        state->updates = s.updates; state->degenerate = s.degenerate; state->clamped = s.clamped; state->rows = s.rows; state->offered = q->since;
    }
    if (coef) { for (int j = 0; j < FBA_TAPS; j++) coef[j] = s.coef[j]; coef[FBA_TAPS] = s.sc_re; coef[FBA_TAPS + 1] = s.sc_im; coef[FBA_TAPS + 2] = (float)s.nd; }
    return MCRX_OK;
}
