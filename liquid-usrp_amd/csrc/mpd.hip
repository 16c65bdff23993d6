// mpd.hip -- predistortion with memory on the wideband stream for gfx950: M branch tables looked up by the amplitudes of delayed
// samples, their coefficients learned on the device by least squares from the amplifier's input and output; cf32 in, cf32 or sc16 out
// (mcrx_hip_mpd_*; the definition with every operation is in include/mcrx_hip.h).
//
// The handle owns, in device memory, the state (counters, rows, res, c), the M tables F_m[0 .. K], the same tables as M K quadruples
// (F[k], F[k+1] - F[k]) and the (L + 1)(L + 2) / 2 complex int64 sums.  Nothing of it is read back by a launch's host side.
//
// A trained handle of one branch runs pdtable.hpp's pd_stream_kernel as dpd does.  The handle's fields and the bodies of create,
// destroy, reset and set_tables are pdtable.hpp's too.
// mpd_apply_kernel<M, FOUT>, M = 2 .. 4: pd_stream_kernel's lane layout -- a lane owns an index-aligned pair of outputs.  A workgroup
// stages the quadruples of all M tables in LDS once and takes mpd_rounds() rounds of 256 pairs.  A round stages its 512 + lead samples
// in LDS as (x.re, x.im, f, k): amplitude, index and fraction are computed once a sample (pd_stage), and a branch is two 16-byte LDS
// reads (the staged sample, the quadruple), two fmaf and the product (pd_branch).
// mpd_copy_kernel<FOUT>: the handle that has learned nothing: load in[lead + i], [gain,] convert, store.  It is pd_stream_kernel's copy
// build without the loop, and stays because it is the faster of the two (0.540 against 0.558 ms on 207.7 M samples:
// profiles/pd_bench_ab.jsonl).
// mpd_measure_kernel: a workgroup stages a tile of 256 rows -- the 256 + lead feedback samples' regressors and the 256 targets as
// int32 pairs, one flag a row -- then lane t < (L + 1)(L + 2) / 2 owns the sum S_pq and loops over the tile's eligible rows: two
// 8-byte LDS reads and four 32 x 32 -> 64-bit multiply-adds a row.  The lane keeps its sum in registers over all the workgroup's tiles
// and flushes it with one pair of int64 atomics.  (The regressors of a sample do not depend on the branch that uses it, so the tile is
// (256 + lead) P pairs, not 256 L.)
// mpd_update_kernel: one workgroup; lane 0 factors and solves in fp64 with its arrays in LDS, all lanes tabulate and shift.
// mpd_table_kernel: the quadruples of tables that set_tables copied in, or the reset.
//
// Contraction is switched off for this file, as in dpd.hip: the update is the + - * / sqrt sequence a float64 model reproduces.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>
#include <string>
#include "../../include/mcrx_hip.h"
#include "mpd_plan.hpp"
#include "pdtable.hpp"

namespace mcrx {

struct MpdArgs {                                             // a launch of the window kernel (M > 1) or of the copy kernel
    const void *in; void *out;                              // in: the sample of output 0 (lead samples behind the call's d_in)
    const float4 *quads;                                    // M K quadruples (F[k].re, F[k].im, dF.re, dF.im), table after table
    unsigned long long *clip;                               // sc16-out builds: the handle's count of clipped samples
    uint64_t parity, n;                                     // (address of in[0] / 8) & 1; outputs of this launch
    uint32_t K, rounds, lead, delay[MPD_MAX_BRANCHES]; float inv_step, gain;
};

template <int M, int FOUT>
__global__ __launch_bounds__(MPD_WG) void mpd_apply_kernel(MpdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float4 mpd_lds[];
    float4 *tab = mpd_lds;                                              // M K quadruples
    for (uint32_t k = threadIdx.x; k < (uint32_t)M * a.K; k += MPD_WG) tab[k] = a.quads[k];
    __syncthreads();
    const float Kf = (float)a.K;
    const int Km1 = (int)a.K - 1;
    uint32_t nclip = 0;
    const uint64_t base = (uint64_t)blockIdx.x * a.rounds * MPD_WG + threadIdx.x;
    // win[s] is the staged sample wbase + s of the launch, wbase = (the round's first pair's m0) - lead; a sample outside
    // -lead .. n - 1 is staged as a zero and used by masked outputs only
    float4 *win = mpd_lds + (uint32_t)M * a.K;
    const float2 *cur = reinterpret_cast<const float2 *>(a.in);
    const long long lead = (long long)a.lead, n = (long long)a.n;
    for (uint32_t r = 0; r < a.rounds; r++) {
        const IqPair p = iq_pair(a.parity, a.n, base + (uint64_t)r * MPD_WG);
        // the lane's pair as the window needs it: a half in front of the launch's first output is history, not masked
        float2 x0 = make_float2(0.f, 0.f), x1 = x0;
        const bool in0 = p.m0 >= -lead && p.m0 < n, in1 = p.m0 + 1 >= -lead && p.m0 + 1 < n;
        if (in0 && in1 && (reinterpret_cast<uintptr_t>(cur + p.m0) & 15u) == 0) {
            const float4 v = *reinterpret_cast<const float4 *>(cur + p.m0);
            x0 = make_float2(v.x, v.y); x1 = make_float2(v.z, v.w);
        } else { if (in0) x0 = cur[p.m0]; if (in1) x1 = cur[p.m0 + 1]; }
        float2 h = make_float2(0.f, 0.f);
        const long long j = p.m0 - 2ll * threadIdx.x - lead + (long long)threadIdx.x;      // lane t < lead: history sample wbase + t
        if ((long long)threadIdx.x < lead && j >= -lead && j < n) h = cur[j];
        const uint32_t mine = a.lead + 2u * threadIdx.x;
        win[mine] = pd_stage(x0, a.inv_step, Kf, Km1);
        win[mine + 1u] = pd_stage(x1, a.inv_step, Kf, Km1);
        if ((long long)threadIdx.x < lead) win[threadIdx.x] = pd_stage(h, a.inv_step, Kf, Km1);
        __syncthreads();
        float2 v0 = pd_branch(tab, win[mine]), v1 = pd_branch(tab, win[mine + 1u]);
#pragma unroll
        for (int m = 1; m < M; m++) {
            const float2 p0 = pd_branch(tab + (uint32_t)m * a.K, win[mine - a.delay[m]]);
            const float2 p1 = pd_branch(tab + (uint32_t)m * a.K, win[mine + 1u - a.delay[m]]);
            v0 = make_float2(v0.x + p0.x, v0.y + p0.y); v1 = make_float2(v1.x + p1.x, v1.y + p1.y);
        }
        if (a.gain != 1.0f) { v0 = make_float2(a.gain * v0.x, a.gain * v0.y); v1 = make_float2(a.gain * v1.x, a.gain * v1.y); }
        nclip += store_pair<FOUT>(a.out, p, v0, v1);
        __syncthreads();                                            // the window is restaged by the next round
    }
    if (FOUT == IQ_SC16) sc16_clip_commit(a.clip, nclip);               // every lane of every wave gets here
}

template <int FOUT>
__global__ __launch_bounds__(MPD_WG) void mpd_copy_kernel(MpdArgs a)
{
    const IqPair p = iq_pair(a.parity, a.n, (uint64_t)blockIdx.x * MPD_WG + threadIdx.x);
    float2 v0, v1;
    load_pair<IQ_CF32>(a.in, p, v0, v1);
    if (a.gain != 1.0f) { v0 = make_float2(a.gain * v0.x, a.gain * v0.y); v1 = make_float2(a.gain * v1.x, a.gain * v1.y); }
    const uint32_t nclip = store_pair<FOUT>(a.out, p, v0, v1);
    if (FOUT == IQ_SC16) sc16_clip_commit(a.clip, nclip);
}

struct MpdState {                                           // device; the arrays lie behind it
    unsigned long long updates, skipped, degenerate;
    long long rows;
    double res, c[2 * MPD_MAX_COEFFS];
};

struct MpdMeasure {
    const float2 *u, *z;
    unsigned long long *sums;                               // 2 (L + 1)(L + 2) / 2: S_pq.re, S_pq.im, the upper triangle row by row
    MpdState *state;
    uint64_t n, tiles;
    uint32_t M, P, L, lead, delay[MPD_MAX_BRANCHES]; float inv_g0; int e;
};

__global__ __launch_bounds__(MPD_WG) void mpd_measure_kernel(MpdMeasure a)
{
    extern __shared__ __attribute__((aligned(16))) int2 mpd_tile[];
    const uint32_t t = threadIdx.x, L = a.L, P = a.P, lead = a.lead, span = (uint32_t)MPD_TILE + lead;
    int2 *Z = mpd_tile;                                                 // span samples' P regressors
    int2 *U = Z + span * P;                                             // 256 targets
    int *zgood = reinterpret_cast<int *>(U + MPD_TILE);                 // span
    int *rowok = zgood + span;                                          // 256
    // this lane's sum: t enumerates p <= q <= L row by row; V_p of row r lies at mpd_tile[ip + r * sp]
    const bool own = t < (L + 1u) * (L + 2u) / 2u;
    uint32_t p = 0, q = 0;
    if (own) { uint32_t rem = t; while (rem >= L + 1u - p) { rem -= L + 1u - p; p++; } q = p + rem; }
    const uint32_t mp = p < L ? p / P : 0u, mq = q < L ? q / P : 0u;
    const uint32_t ip = p < L ? (lead - a.delay[mp]) * P + (p - mp * P) : span * P, sp = p < L ? P : 1u;
    const uint32_t iq = q < L ? (lead - a.delay[mq]) * P + (q - mq * P) : span * P, sq = q < L ? P : 1u;
    long long sre = 0, sim = 0;
    uint32_t nrows = 0, nskip = 0;
    for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const uint64_t r0 = (uint64_t)lead + tile * MPD_TILE;           // the sample of the tile's first row
        for (uint32_t s = t; s < span; s += MPD_WG) {
            const uint64_t j = r0 - lead + s;
            int32_t bre[MPD_MAX_ORDER] = {0, 0, 0, 0, 0}, bim[MPD_MAX_ORDER] = {0, 0, 0, 0, 0};
            bool good = false;
            if (j < a.n) { const float2 z = a.z[j]; good = mpd_basis(z.x, z.y, a.inv_g0, a.e, P, bre, bim); }
#pragma unroll
            for (uint32_t k = 0; k < (uint32_t)MPD_MAX_ORDER; k++)
                if (k < P) Z[s * P + k] = make_int2(bre[k], bim[k]);
            zgood[s] = good ? 1 : 0;
        }
        const uint64_t i = r0 + t;
        int32_t ure = 0, uim = 0;
        bool ok = false;
        if (i < a.n) { const float2 u = a.u[i]; ok = mpd_target(u.x, u.y, a.e, &ure, &uim); }
        U[t] = make_int2(ure, uim);
        __syncthreads();
        for (uint32_t m = 0; m < a.M; m++) ok = ok && zgood[t + lead - a.delay[m]] != 0;
        rowok[t] = ok ? 1 : 0;
        if (i < a.n) { if (ok) nrows += 1u; else nskip += 1u; }
        __syncthreads();
        if (own) {
            const uint64_t left = a.n - r0;                             // (tile < tiles: at least one row)
            const uint32_t nr = left < (uint64_t)MPD_TILE ? (uint32_t)left : (uint32_t)MPD_TILE;
            for (uint32_t r = 0; r < nr; r++) {
                if (!rowok[r]) continue;
                const int2 vp = mpd_tile[ip + r * sp], vq = mpd_tile[iq + r * sq];
                sre += (long long)vp.x * vq.x + (long long)vp.y * vq.y;
                sim += (long long)vp.x * vq.y - (long long)vp.y * vq.x;
            }
        }
        __syncthreads();                                                // the tile is restaged
    }
    sc16_clip_commit(&a.state->skipped, nskip);                         // (the wave's sum, one atomic from its first lane, none for 0)
    sc16_clip_commit(reinterpret_cast<unsigned long long *>(&a.state->rows), nrows);
    if (own) {
        if (sre) atomicAdd(&a.sums[2u * t], (unsigned long long)sre);   // (two's complement: the unsigned add is the signed one)
        if (sim) atomicAdd(&a.sums[2u * t + 1u], (unsigned long long)sim);
    }
}

struct MpdUpdate {
    MpdState *state; float2 *F; float4 *quads; long long *sums;
    uint32_t M, P, L, K, min_rows, forget_shift;
    double step, ridge, inv_E;                              // 2^-ridge_log2, 2^-e
};

__device__ __forceinline__ bool mpd_finite(double v) { return v - v == 0.0; }

// The update's linear algebra (include/mcrx_hip.h), lane 0 of one workgroup.  Ar, Ai: L x L (the upper triangle is used; R overwrites
// A); the vectors: L doubles each.  True, with c in (cr, ci) and *res, unless the update is degenerate.
__device__ bool mpd_solve_lane(const MpdUpdate &u, double *Ar, double *Ai, double *br, double *bi, double *yr, double *yi, double *cr, double *ci,
                               double *res)
{
    const uint32_t L = u.L;
    if (u.state->rows < (long long)u.min_rows) return false;
    uint32_t ent = 0;
    double suu = 0.0;
    for (uint32_t p = 0; p <= L; p++)
        for (uint32_t q = p; q <= L; q++, ent++) {
            const double re = (double)u.sums[2u * ent], im = (double)u.sums[2u * ent + 1u];
            if (q < L) { Ar[p * L + q] = re; Ai[p * L + q] = im; }
            else if (p < L) { br[p] = re; bi[p] = im; }
            else suu = re;
        }
    double tr = 0.0;
    for (uint32_t l = 0; l < L; l++) tr = tr + Ar[l * L + l];
    const double lambda = (tr / (double)L) * u.ridge;
    for (uint32_t l = 0; l < L; l++) Ar[l * L + l] = Ar[l * L + l] + lambda;
    for (uint32_t j = 0; j < L; j++)
        for (uint32_t i = 0; i <= j; i++) {
            double sr = Ar[i * L + j], si = Ai[i * L + j];
            for (uint32_t p = 0; p < i; p++) {
                const double ar = Ar[p * L + i], ai = Ai[p * L + i], cr_ = Ar[p * L + j], ci_ = Ai[p * L + j];
                sr = sr - (ar * cr_ + ai * ci_);
                si = si - (ar * ci_ - ai * cr_);
            }
            if (i < j) { const double d = Ar[i * L + i]; Ar[i * L + j] = sr / d; Ai[i * L + j] = si / d; }
            else { if (!(sr > 0.0)) return false; Ar[j * L + j] = sqrt(sr); Ai[j * L + j] = 0.0; }
        }
    for (uint32_t i = 0; i < L; i++) {
        double sr = br[i], si = bi[i];
        for (uint32_t p = 0; p < i; p++) {
            const double ar = Ar[p * L + i], ai = Ai[p * L + i];
            sr = sr - (ar * yr[p] + ai * yi[p]);
            si = si - (ar * yi[p] - ai * yr[p]);
        }
        const double d = Ar[i * L + i];
        yr[i] = sr / d; yi[i] = si / d;
    }
    for (uint32_t ii = L; ii > 0; ii--) {
        const uint32_t i = ii - 1u;
        double sr = yr[i], si = yi[i];
        for (uint32_t p = i + 1u; p < L; p++) {
            const double ar = Ar[i * L + p], ai = Ai[i * L + p];
            sr = sr - (ar * cr[p] - ai * ci[p]);
            si = si - (ar * ci[p] + ai * cr[p]);
        }
        const double d = Ar[i * L + i];
        cr[i] = sr / d; ci[i] = si / d;
    }
    double qq = 0.0;
    for (uint32_t l = 0; l < L; l++) qq = qq + (cr[l] * br[l] + ci[l] * bi[l]);
    *res = suu - qq;
    bool fin = mpd_finite(*res);
    for (uint32_t l = 0; l < L; l++) fin = fin && mpd_finite(cr[l]) && mpd_finite(ci[l]);
    return fin;
}

// entry j of table m from the coefficients: Horner with a multiplication and an addition a step, rounded to fp32
__device__ __forceinline__ float2 mpd_entry(const MpdUpdate &u, const double *cr, const double *ci, uint32_t m, uint32_t j)
{
    const double rho = ((double)j * u.step) * u.inv_E;
    double gr = cr[m * u.P + u.P - 1u], gi = ci[m * u.P + u.P - 1u];
    for (uint32_t k = u.P - 1u; k > 0; k--) {
        gr = gr * rho + cr[m * u.P + k - 1u];
        gi = gi * rho + ci[m * u.P + k - 1u];
    }
    return make_float2((float)gr, (float)gi);
}

__global__ __launch_bounds__(MPD_WG) void mpd_update_kernel(MpdUpdate u)
{
    __shared__ double Ar[MPD_MAX_COEFFS * MPD_MAX_COEFFS], Ai[MPD_MAX_COEFFS * MPD_MAX_COEFFS], vec[6 * MPD_MAX_COEFFS], res;
    __shared__ int solved, bad;
    double *cr = vec + 4 * MPD_MAX_COEFFS, *ci = vec + 5 * MPD_MAX_COEFFS;
    if (threadIdx.x == 0) {
        solved = mpd_solve_lane(u, Ar, Ai, vec, vec + MPD_MAX_COEFFS, vec + 2 * MPD_MAX_COEFFS, vec + 3 * MPD_MAX_COEFFS, cr, ci, &res) ? 1 : 0;
        bad = 0;
    }
    __syncthreads();
    const uint32_t entries = u.M * (u.K + 1u);
    if (solved)
        for (uint32_t i = threadIdx.x; i < entries; i += MPD_WG) {
            const float2 f = mpd_entry(u, cr, ci, i / (u.K + 1u), i % (u.K + 1u));
            if (!(f.x - f.x == 0.f) || !(f.y - f.y == 0.f)) bad = 1;
        }
    __syncthreads();
    const bool keep = solved && !bad;
    if (keep)
        for (uint32_t i = threadIdx.x; i < entries; i += MPD_WG) u.F[i] = mpd_entry(u, cr, ci, i / (u.K + 1u), i % (u.K + 1u));
    if (threadIdx.x == 0) {
        if (keep) { u.state->res = res; for (uint32_t l = 0; l < u.L; l++) { u.state->c[2u * l] = cr[l]; u.state->c[2u * l + 1u] = ci[l]; } }
        else u.state->degenerate += 1;
        u.state->updates += 1;
        u.state->rows >>= u.forget_shift;                               // arithmetic
    }
    __threadfence();
    __syncthreads();
    pd_write_quads(u.F, u.quads, u.M, u.K);
    if (u.forget_shift)
        for (uint32_t b = threadIdx.x; b < (u.L + 1u) * (u.L + 2u); b += MPD_WG) u.sums[b] >>= u.forget_shift;
}

// reset != 0: F_0 := 1, the other tables := 0, c := (1, 0, 0 ...), sums and counters := 0; then (either way) the quadruples
__global__ __launch_bounds__(MPD_WG) void mpd_table_kernel(MpdState *state, float2 *F, float4 *quads, long long *sums, uint32_t M, uint32_t K, uint32_t L,
                                                           uint32_t reset)
{
    if (reset) {
        for (uint32_t i = threadIdx.x; i < M * (K + 1u); i += MPD_WG) F[i] = make_float2(i <= K ? 1.f : 0.f, 0.f);
        for (uint32_t b = threadIdx.x; b < (L + 1u) * (L + 2u); b += MPD_WG) sums[b] = 0;
        if (threadIdx.x == 0) {
            state->updates = 0; state->skipped = 0; state->degenerate = 0; state->rows = 0; state->res = 0.0;
            for (uint32_t l = 0; l < 2u * MPD_MAX_COEFFS; l++) state->c[l] = l == 0 ? 1.0 : 0.0;
        }
        __threadfence();
        __syncthreads();
    }
    pd_write_quads(F, quads, M, K);
}

}  // namespace mcrx

using namespace mcrx;

static thread_local std::string g_mpd_err;

struct mcrx_hip_mpd_s : PdHandle {
    mcrx_hip_mpd_config cfg;
    MpdConsts k;
    MpdState *state = nullptr; long long *sums = nullptr;   // in mem, with F and quads
};

static void mpd_launch_table(mcrx_hip_mpd_t q, hipStream_t st, uint32_t reset)
{
    hipLaunchKernelGGL(mpd_table_kernel, dim3(1), dim3(MPD_WG), 0, st, q->state, q->F, q->quads, q->sums, q->k.M, q->k.K, q->k.L, reset);
}

extern "C" const char *mcrx_hip_mpd_last_error(void) { return g_mpd_err.c_str(); }

extern "C" int mcrx_hip_mpd_selftest(const mcrx_hip_mpd_config *cfg, float *inv_step, double *step, int *e, float *inv_g0, const float *u,
                                     const float *z, size_t n, int32_t *Z, int32_t *U, int32_t *good)
{
    if (!cfg || (n && (!u || !z || !Z || !U || !good))) { g_mpd_err = "null pointer"; return MCRX_EINVAL; }
    if (const char *bad = mpd_check(cfg)) { g_mpd_err = bad; return MCRX_EINVAL; }
    const MpdConsts k = mpd_consts(cfg);
    if (inv_step) *inv_step = k.inv_step;
    if (step) *step = k.step;
    if (e) *e = k.e;
    if (inv_g0) *inv_g0 = k.inv_g0;
    for (size_t i = 0; i < n; i++) {
        int32_t bre[MPD_MAX_ORDER], bim[MPD_MAX_ORDER];
        const bool zg = mpd_basis(z[2 * i], z[2 * i + 1], k.inv_g0, k.e, k.P, bre, bim);
        for (uint32_t p = 0; p < k.P; p++) { Z[(i * k.P + p) * 2] = bre[p]; Z[(i * k.P + p) * 2 + 1] = bim[p]; }
        const bool ug = mpd_target(u[2 * i], u[2 * i + 1], k.e, &U[2 * i], &U[2 * i + 1]);
        good[i] = (zg ? 1 : 0) + (ug ? 2 : 0);
    }
    return MCRX_OK;
}

extern "C" int mcrx_hip_mpd_create(mcrx_hip_mpd_t *out, const mcrx_hip_mpd_config *cfg)
{
    if (!out) { g_mpd_err = "null pointer"; return MCRX_EINVAL; }
    *out = nullptr;
    if (!cfg) { g_mpd_err = "null configuration"; return MCRX_EINVAL; }
    if (const char *bad = mpd_check(cfg)) { g_mpd_err = bad; return MCRX_EINVAL; }
    mcrx_hip_mpd_t q = new mcrx_hip_mpd_s();
    q->cfg = *cfg;
    q->k = mpd_consts(cfg);
    const size_t K = q->k.K, M = q->k.M;
    const int rc = pd_alloc(q, g_mpd_err, cfg->output_format == IQ_SC16, M, K, sizeof(MpdState), 2 * (size_t)q->k.sums * sizeof(long long));
    if (rc != MCRX_OK) { delete q; return rc; }
    q->state = reinterpret_cast<MpdState *>(q->mem);
    q->sums = reinterpret_cast<long long *>(q->quads + M * K);
    *out = q;
    return MCRX_OK;
}

extern "C" int mcrx_hip_mpd_destroy(mcrx_hip_mpd_t q) { return pd_destroy(q); }

extern "C" unsigned mcrx_hip_mpd_output_format(mcrx_hip_mpd_t q) { return q ? q->cfg.output_format : 0u; }
extern "C" unsigned mcrx_hip_mpd_lead(mcrx_hip_mpd_t q) { return q ? q->k.lead : 0u; }

extern "C" int mcrx_hip_mpd_reset(mcrx_hip_mpd_t q) { return pd_reset(q, g_mpd_err); }

template <int FOUT> static void mpd_launch_apply(uint32_t M, dim3 grid, uint32_t lds, hipStream_t st, const MpdArgs &a)
{
    const dim3 wg(MPD_WG);
    switch (M) {
    case 2: hipLaunchKernelGGL((mpd_apply_kernel<2, FOUT>), grid, wg, lds, st, a); break;
    case 3: hipLaunchKernelGGL((mpd_apply_kernel<3, FOUT>), grid, wg, lds, st, a); break;
    default: hipLaunchKernelGGL((mpd_apply_kernel<4, FOUT>), grid, wg, lds, st, a); break;
    }
}

extern "C" int mcrx_hip_mpd_execute_device(mcrx_hip_mpd_t q, const void *d_in, size_t n, void *d_out, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_mpd_err = "null handle"; return MCRX_EINVAL; }
    const bool out16 = q->cfg.output_format == IQ_SC16;
    const uint32_t lead = q->k.lead;
    const char *bad = (uint64_t)n > ((uint64_t)1 << 32) - lead ? "n + lead must not exceed 2^32 samples" : nullptr;
    if (!bad) bad = stream_call_check(reinterpret_cast<uintptr_t>(d_in), reinterpret_cast<uintptr_t>(d_out), n, 8u, out16 ? 4u : 8u, lead, false, false,
                                      "d_in and d_out overlap: a lane reads its neighbours' samples, so no overlap is allowed");
    if (bad) { g_mpd_err = bad; return MCRX_EINVAL; }
    if (n == 0) return MCRX_OK;
    hipStream_t st = (hipStream_t)stream;
    const float2 *in = reinterpret_cast<const float2 *>(d_in) + lead;  // the sample of output 0
    const bool apply = q->trained;                                      // (a reset still pending means not trained: the stale tables are not read)
    if (apply && q->k.M == 1u) {
        MCRX_OP_CHK(g_mpd_err, pd_stream_launch(out16, true, in, d_out, n, q->quads, q->clip.device(), q->k.K, q->k.inv_step, q->cfg.gain, st));
    } else {
        MpdArgs a = {};
        a.in = in; a.out = d_out; a.quads = q->quads; a.clip = q->clip.device();
        a.parity = (reinterpret_cast<uintptr_t>(a.in) >> 3) & 1u; a.n = n;
        a.K = q->k.K; a.lead = lead; a.inv_step = q->k.inv_step; a.gain = q->cfg.gain;
        for (uint32_t m = 0; m < q->k.M; m++) a.delay[m] = q->k.delay[m];
        a.rounds = apply ? mpd_rounds(q->k.M, a.K) : 1u;
        const dim3 grid(pd_stream_grid(a.parity, n, a.rounds));
        if (apply) {
            const uint32_t lds = mpd_apply_lds(q->k.M, a.K, lead);
            if (out16) mpd_launch_apply<IQ_SC16>(q->k.M, grid, lds, st, a); else mpd_launch_apply<IQ_CF32>(q->k.M, grid, lds, st, a);
        } else {
            if (out16) hipLaunchKernelGGL((mpd_copy_kernel<IQ_SC16>), grid, dim3(MPD_WG), 0, st, a);
            else       hipLaunchKernelGGL((mpd_copy_kernel<IQ_CF32>), grid, dim3(MPD_WG), 0, st, a);
        }
        MCRX_OP_CHK(g_mpd_err, hipGetLastError());
    }
    if (out16) MCRX_OP_CHK(g_mpd_err, q->clip.mark(st));
    return MCRX_OK;
}

extern "C" int mcrx_hip_mpd_measure_device(mcrx_hip_mpd_t q, const void *d_u, const void *d_z, size_t n, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_mpd_err = "null handle"; return MCRX_EINVAL; }
    const uint64_t rows = mpd_rows(n, q->k.lead);
    const char *bad = pd_measure_check(q, d_u, d_z, n, rows, MPD_GUARD_LOG2, "more than 2^26 rows offered since the last reset: the int64 sums could overflow");
    if (bad) { g_mpd_err = bad; return MCRX_EINVAL; }
    if (rows == 0) return MCRX_OK;
    hipStream_t st = (hipStream_t)stream;
    MCRX_OP_CHK(g_mpd_err, pd_serve_reset(q, st, mpd_launch_table));
    MpdMeasure m = {};
    m.u = reinterpret_cast<const float2 *>(d_u); m.z = reinterpret_cast<const float2 *>(d_z);
    m.sums = reinterpret_cast<unsigned long long *>(q->sums); m.state = q->state;
    m.n = n; m.tiles = mpd_tiles(rows);
    m.M = q->k.M; m.P = q->k.P; m.L = q->k.L; m.lead = q->k.lead; m.inv_g0 = q->k.inv_g0; m.e = q->k.e;
    for (uint32_t b = 0; b < q->k.M; b++) m.delay[b] = q->k.delay[b];
    hipLaunchKernelGGL(mpd_measure_kernel, dim3(mpd_measure_grid(rows)), dim3(MPD_WG), mpd_measure_lds(m.P, m.lead), st, m);
    MCRX_OP_CHK(g_mpd_err, hipGetLastError());
    q->since += rows;
    return MCRX_OK;
}

extern "C" int mcrx_hip_mpd_update(mcrx_hip_mpd_t q, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_mpd_err = "null handle"; return MCRX_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    MCRX_OP_CHK(g_mpd_err, pd_serve_reset(q, st, mpd_launch_table));
    MpdUpdate p = {};
    p.state = q->state; p.F = q->F; p.quads = q->quads; p.sums = q->sums;
    p.M = q->k.M; p.P = q->k.P; p.L = q->k.L; p.K = q->k.K; p.min_rows = q->cfg.min_rows; p.forget_shift = q->cfg.forget_shift;
    p.step = q->k.step; p.ridge = std::ldexp(1.0, -(int)q->cfg.ridge_log2); p.inv_E = std::ldexp(1.0, -q->k.e);
    hipLaunchKernelGGL(mpd_update_kernel, dim3(1), dim3(MPD_WG), 0, st, p);
    MCRX_OP_CHK(g_mpd_err, hipGetLastError());
    q->since = pd_guard_after_update(q->since, q->cfg.forget_shift);
    q->trained = true;
    return MCRX_OK;
}

extern "C" int mcrx_hip_mpd_set_tables(mcrx_hip_mpd_t q, const float *F, void *stream)
{
    return pd_set_tables(q, g_mpd_err, "the tables must be finite", F, q ? q->k.M : 0, q ? q->k.K : 0, stream, mpd_launch_table);
}

extern "C" int mcrx_hip_mpd_read(mcrx_hip_mpd_t q, mcrx_hip_mpd_state *state, float *F, double *c, int64_t *sums, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_mpd_err = "null handle"; return MCRX_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    MCRX_OP_CHK(g_mpd_err, pd_serve_reset(q, st, mpd_launch_table));
    MpdState s = {};
    if (state || c) MCRX_OP_CHK(g_mpd_err, hipMemcpyAsync(&s, q->state, sizeof(s), hipMemcpyDeviceToHost, st));
    if (F) MCRX_OP_CHK(g_mpd_err, hipMemcpyAsync(F, q->F, 2 * (size_t)q->k.M * (q->k.K + 1) * sizeof(float), hipMemcpyDeviceToHost, st));
    if (sums) MCRX_OP_CHK(g_mpd_err, hipMemcpyAsync(sums, q->sums, 2 * (size_t)q->k.sums * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    MCRX_OP_CHK(g_mpd_err, hipStreamSynchronize(st));
    if (state) { state->updates = s.updates; state->skipped = s.skipped; state->degenerate = s.degenerate; state->rows = s.rows; state->res = s.res; }
    if (c) for (uint32_t l = 0; l < 2u * q->k.L; l++) c[l] = s.c[l];
    return MCRX_OK;
}

extern "C" int mcrx_hip_mpd_clipped(mcrx_hip_mpd_t q, uint64_t *samples, int reset)
{
    return op_clipped(q, g_mpd_err, samples, reset);
}
