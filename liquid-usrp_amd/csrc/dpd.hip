// dpd.hip -- digital predistortion on the wideband stream for gfx950: a complex gain table looked up by amplitude, learned on the
// device from the amplifier's input and output; cf32 in, cf32 or sc16 out (mcrx_hip_dpd_*; the definition
// with every fmaf is in include/mcrx_hip.h).
//
// The handle owns, in device memory, the table F[0 .. K], the same table as K quadruples (F[k], F[k+1] - F[k]), the accumulators
// (four int64 a bin) and the counters.  Nothing of it is read back by a launch's host side: whether there has been an update or a
// set_table, and how many samples have been offered, the host knows itself.
//
// execute is pdtable.hpp's pd_stream_kernel<FOUT, APPLY>, the parity taken from d_in's address: a workgroup of an APPLY build takes
// K / 32 (at least 4) rounds of 256 consecutive pairs, four rounds' loads in flight at a time, so that staging the table is 1/16 of
// the bytes it streams; the build without APPLY takes one (a lane a pair, rfchain_kernel's grid).  The handle's fields and the bodies
// of create, destroy, reset and set_table are pdtable.hpp's too.
// dpd_measure_kernel: the streaming lanes over (u, z); a histogram in the workgroup's LDS -- three 64-bit sums and a 32-bit count per bin,
// integer LDS atomics -- flushed bin by bin, the non-zero ones only, with 64-bit integer atomics on the handle's accumulators.  The
// ineligible samples are counted per lane, summed across the wave and added once per wave.
// dpd_update_kernel: one workgroup; lane 0 runs the update in fp64 with its work arrays (A, o) in LDS, then all lanes write the
// quadruples and shift the accumulators.  dpd_table_kernel: the quadruples of a table that set_table copied in, or the reset.
//
// Contraction is switched off for this file, as in rfchain.hip: every build rounds the same way, and the update is the + - * / sqrt
// sequence a float64 model reproduces to the last bit.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>
#include <string>
#include "../../include/mcrx_hip.h"
#include "dpd_plan.hpp"
#include "pdtable.hpp"

namespace mcrx {

struct DpdMeasure {
    const void *u, *z;
    unsigned long long *acc;                                // 4 (K + 1): cnt, Sre, Sim, Suu of bin j at acc[4 j ..]
    unsigned long long *skipped;
    uint64_t parity, n;
    uint32_t K; float inv_step, zmax2; double scale;
};

__device__ __forceinline__ void dpd_measure_one(const DpdMeasure &m, unsigned long long *sums, uint32_t *cnt, float2 u, float2 z, uint32_t &skip)
{
    int j;
    if (!dpd_bin(u.x, u.y, z.x, z.y, m.inv_step, (float)m.K, m.zmax2, &j)) { skip += 1u; return; }
    long long sre, sim, suu;
    dpd_terms(u.x, u.y, z.x, z.y, m.scale, &sre, &sim, &suu);
    atomicAdd(&cnt[j], 1u);
    atomicAdd(&sums[3 * j + 0], (unsigned long long)sre);               // (two's complement: the unsigned add is the signed one)
    atomicAdd(&sums[3 * j + 1], (unsigned long long)sim);
    atomicAdd(&sums[3 * j + 2], (unsigned long long)suu);
}

__global__ __launch_bounds__(DPD_WG) void dpd_measure_kernel(DpdMeasure m)
{
    extern __shared__ unsigned long long dpd_hist[];                    // 3 (K + 1) sums, then K + 1 counts
    unsigned long long *sums = dpd_hist;
    uint32_t *cnt = reinterpret_cast<uint32_t *>(dpd_hist + 3 * (m.K + 1u));
    for (uint32_t b = threadIdx.x; b <= m.K; b += DPD_WG) { sums[3 * b] = 0; sums[3 * b + 1] = 0; sums[3 * b + 2] = 0; cnt[b] = 0; }
    __syncthreads();
    const uint64_t pairs = iq_pairs(m.parity, m.n), stride = (uint64_t)gridDim.x * DPD_WG;
    uint32_t skip = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * DPD_WG + threadIdx.x; g < pairs; g += stride) {
        const IqPair p = iq_pair(m.parity, m.n, g);
        float2 u0, u1, z0, z1;
        load_pair<IQ_CF32>(m.u, p, u0, u1);
        load_pair<IQ_CF32>(m.z, p, z0, z1);
        if (p.ok0) dpd_measure_one(m, sums, cnt, u0, z0, skip);
        if (p.ok1) dpd_measure_one(m, sums, cnt, u1, z1, skip);
    }
    sc16_clip_commit(m.skipped, skip);                                  // (the wave's sum, one atomic from its first lane, none for 0)
    __syncthreads();
    for (uint32_t b = threadIdx.x; b <= m.K; b += DPD_WG) {
        const uint32_t c = cnt[b];
        if (c == 0u) continue;
        atomicAdd(&m.acc[4 * b + 0], (unsigned long long)c);
        atomicAdd(&m.acc[4 * b + 1], sums[3 * b + 0]);
        atomicAdd(&m.acc[4 * b + 2], sums[3 * b + 1]);
        atomicAdd(&m.acc[4 * b + 3], sums[3 * b + 2]);
    }
}

struct DpdState {                                           // device; the arrays lie behind it (dpd_layout)
    unsigned long long updates, skipped, degenerate, pad_;
};

struct DpdUpdate {
    DpdState *state; float2 *F; float4 *quads; long long *acc;
    uint32_t K, min_count, forget_shift;
    double step, g0;
};

// the update (include/mcrx_hip.h), lane 0 of one workgroup; Ar, Ai, o: K + 1 doubles each, in LDS
__device__ void dpd_update_lane(const DpdUpdate &p, double *Ar, double *Ai, double *o)
{
    const uint32_t K = p.K;
    int first = -1;
    for (uint32_t j = 0; j <= K; j++) {
        const long long cnt = p.acc[4 * j], sre = p.acc[4 * j + 1], sim = p.acc[4 * j + 2], suu = p.acc[4 * j + 3];
        if (cnt >= (long long)p.min_count && suu > 0) {
            Ar[j] = (double)sre / (double)suu; Ai[j] = (double)sim / (double)suu;
            if (first < 0) first = (int)j;
        } else if (first >= 0) { Ar[j] = Ar[j - 1]; Ai[j] = Ai[j - 1]; }
    }
    if (first < 0) { p.state->degenerate += 1; return; }
    for (int j = 0; j < first; j++) { Ar[j] = Ar[first]; Ai[j] = Ai[first]; }
    double prev = 0.0;
    for (uint32_t j = 0; j <= K; j++) {
        const double mag = sqrt(Ar[j] * Ar[j] + Ai[j] * Ai[j]), v = mag * ((double)j * p.step);
        prev = j == 0 ? v : (v > prev ? v : prev);
        o[j] = prev;
    }
    uint32_t j = 1;
    for (uint32_t i = 1; i <= K; i++) {
        const double ri = (double)i * p.step, d = p.g0 * ri;
        while (j <= K && o[j] < d) j++;
        double rin, ar, ai;
        if (j > K) { rin = (double)K * p.step; ar = Ar[K]; ai = Ai[K]; }
        else {
            const double den = o[j] - o[j - 1];
            const double fr = den > 0.0 ? (d - o[j - 1]) / den : 0.0;
            rin = (double)(j - 1) * p.step + fr * p.step;
            ar = Ar[j - 1] + fr * (Ar[j] - Ar[j - 1]); ai = Ai[j - 1] + fr * (Ai[j] - Ai[j - 1]);
        }
        const double mag = sqrt(ar * ar + ai * ai), q = rin / ri;
        p.F[i] = mag > 0.0 ? make_float2((float)((q * ar) / mag), (float)(-((q * ai) / mag))) : make_float2((float)q, 0.f);
    }
    p.F[0] = p.F[1];
}

__global__ __launch_bounds__(DPD_WG) void dpd_update_kernel(DpdUpdate p)
{
    __shared__ double work[3 * ((1 << DPD_MAX_LOG2) + 1)];
    if (threadIdx.x == 0) {
        dpd_update_lane(p, work, work + (p.K + 1u), work + 2 * (p.K + 1u));
        p.state->updates += 1;
        __threadfence();
    }
    __syncthreads();
    pd_write_quads(p.F, p.quads, 1u, p.K);
    if (p.forget_shift)
        for (uint32_t b = threadIdx.x; b < 4u * (p.K + 1u); b += DPD_WG) p.acc[b] >>= p.forget_shift;      // arithmetic
}

// reset != 0: table := 1, accumulators and counters := 0; then (either way) the quadruples of the table that is there
__global__ __launch_bounds__(DPD_WG) void dpd_table_kernel(DpdState *state, float2 *F, float4 *quads, long long *acc, uint32_t K, uint32_t reset)
{
    if (reset) {
        for (uint32_t k = threadIdx.x; k <= K; k += DPD_WG) F[k] = make_float2(1.f, 0.f);
        for (uint32_t b = threadIdx.x; b < 4u * (K + 1u); b += DPD_WG) acc[b] = 0;
        if (threadIdx.x == 0) { state->updates = 0; state->skipped = 0; state->degenerate = 0; }
        __threadfence();
        __syncthreads();
    }
    pd_write_quads(F, quads, 1u, K);
}

}  // namespace mcrx

using namespace mcrx;

static thread_local std::string g_dpd_err;

struct mcrx_hip_dpd_s : PdHandle {
    mcrx_hip_dpd_config cfg;
    DpdConsts k;
    DpdState *state = nullptr; long long *acc = nullptr;    // in mem, with F and quads
};

static void dpd_launch_table(mcrx_hip_dpd_t q, hipStream_t st, uint32_t reset)
{
    hipLaunchKernelGGL(dpd_table_kernel, dim3(1), dim3(DPD_WG), 0, st, q->state, q->F, q->quads, q->acc, q->k.K, reset);
}

extern "C" const char *mcrx_hip_dpd_last_error(void) { return g_dpd_err.c_str(); }

extern "C" int mcrx_hip_dpd_selftest(const mcrx_hip_dpd_config *cfg, float *inv_step, double *step, int *e, const float *u, const float *z,
                                     size_t n, int32_t *bin)
{
    if (!cfg || (n && (!u || !z || !bin))) { g_dpd_err = "null pointer"; return MCRX_EINVAL; }
    if (const char *bad = dpd_check(cfg)) { g_dpd_err = bad; return MCRX_EINVAL; }
    const DpdConsts k = dpd_consts(cfg);
    if (inv_step) *inv_step = k.inv_step;
    if (step) *step = k.step;
    if (e) *e = k.e;
    for (size_t i = 0; i < n; i++) {
        int j;
        dpd_bin(u[2 * i], u[2 * i + 1], z[2 * i], z[2 * i + 1], k.inv_step, k.Kf, k.zmax2, &j);
        bin[i] = j;
    }
    return MCRX_OK;
}

extern "C" int mcrx_hip_dpd_create(mcrx_hip_dpd_t *out, const mcrx_hip_dpd_config *cfg)
{
    if (!out) { g_dpd_err = "null pointer"; return MCRX_EINVAL; }
    *out = nullptr;
    if (!cfg) { g_dpd_err = "null configuration"; return MCRX_EINVAL; }
    if (const char *bad = dpd_check(cfg)) { g_dpd_err = bad; return MCRX_EINVAL; }
    mcrx_hip_dpd_t q = new mcrx_hip_dpd_s();
    q->cfg = *cfg;
    q->k = dpd_consts(cfg);
    const size_t K = q->k.K;
    const int rc = pd_alloc(q, g_dpd_err, cfg->output_format == IQ_SC16, 1, K, sizeof(DpdState), 4 * (K + 1) * sizeof(long long));
    if (rc != MCRX_OK) { delete q; return rc; }
    q->state = reinterpret_cast<DpdState *>(q->mem);
    q->acc = reinterpret_cast<long long *>(q->quads + K);
    *out = q;
    return MCRX_OK;
}

extern "C" int mcrx_hip_dpd_destroy(mcrx_hip_dpd_t q) { return pd_destroy(q); }

extern "C" unsigned mcrx_hip_dpd_output_format(mcrx_hip_dpd_t q) { return q ? q->cfg.output_format : 0u; }

extern "C" int mcrx_hip_dpd_reset(mcrx_hip_dpd_t q) { return pd_reset(q, g_dpd_err); }

extern "C" int mcrx_hip_dpd_execute_device(mcrx_hip_dpd_t q, const void *d_in, size_t n, void *d_out, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_dpd_err = "null handle"; return MCRX_EINVAL; }
    const bool out16 = q->cfg.output_format == IQ_SC16;
    const char *bad = stream_call_check(reinterpret_cast<uintptr_t>(d_in), reinterpret_cast<uintptr_t>(d_out), n, 8u, out16 ? 4u : 8u, 0, true, false,
                                        "d_in and d_out overlap: in-place use takes d_in == d_out and equal formats");
    if (bad) { g_dpd_err = bad; return MCRX_EINVAL; }
    if (n == 0) return MCRX_OK;
    hipStream_t st = (hipStream_t)stream;
    // (a reset still pending means not trained: the stale table is not read)
    MCRX_OP_CHK(g_dpd_err, pd_stream_launch(out16, q->trained, d_in, d_out, n, q->quads, q->clip.device(), q->k.K, q->k.inv_step, q->cfg.gain, st));
    if (out16) MCRX_OP_CHK(g_dpd_err, q->clip.mark(st));
    return MCRX_OK;
}

extern "C" int mcrx_hip_dpd_measure_device(mcrx_hip_dpd_t q, const void *d_u, const void *d_z, size_t n, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_dpd_err = "null handle"; return MCRX_EINVAL; }
    const char *bad = pd_measure_check(q, d_u, d_z, n, n, DPD_GUARD_LOG2, "more than 2^28 samples offered since the last reset: the int64 sums could overflow");
    if (bad) { g_dpd_err = bad; return MCRX_EINVAL; }
    if (n == 0) return MCRX_OK;
    hipStream_t st = (hipStream_t)stream;
    MCRX_OP_CHK(g_dpd_err, pd_serve_reset(q, st, dpd_launch_table));
    DpdMeasure m = {};
    m.u = d_u; m.z = d_z; m.acc = reinterpret_cast<unsigned long long *>(q->acc); m.skipped = &q->state->skipped;
    m.parity = (reinterpret_cast<uintptr_t>(d_u) >> 3) & 1u; m.n = n;
    m.K = q->k.K; m.inv_step = q->k.inv_step; m.zmax2 = q->k.zmax2; m.scale = q->k.scale;
    hipLaunchKernelGGL(dpd_measure_kernel, dim3(dpd_measure_grid(m.parity, n)), dim3(DPD_WG), dpd_measure_lds(m.K), st, m);
    MCRX_OP_CHK(g_dpd_err, hipGetLastError());
    q->since += n;
    return MCRX_OK;
}

extern "C" int mcrx_hip_dpd_update(mcrx_hip_dpd_t q, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_dpd_err = "null handle"; return MCRX_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    MCRX_OP_CHK(g_dpd_err, pd_serve_reset(q, st, dpd_launch_table));
    DpdUpdate p = {};
    p.state = q->state; p.F = q->F; p.quads = q->quads; p.acc = q->acc;
    p.K = q->k.K; p.min_count = q->cfg.min_count; p.forget_shift = q->cfg.forget_shift;
    p.step = q->k.step; p.g0 = (double)q->cfg.target_gain;
    hipLaunchKernelGGL(dpd_update_kernel, dim3(1), dim3(DPD_WG), 0, st, p);
    MCRX_OP_CHK(g_dpd_err, hipGetLastError());
    q->since = pd_guard_after_update(q->since, q->cfg.forget_shift);
    q->trained = true;
    return MCRX_OK;
}

extern "C" int mcrx_hip_dpd_set_table(mcrx_hip_dpd_t q, const float *F, void *stream)
{
    return pd_set_tables(q, g_dpd_err, "the table must be finite", F, 1, q ? q->k.K : 0, stream, dpd_launch_table);
}

extern "C" int mcrx_hip_dpd_read(mcrx_hip_dpd_t q, mcrx_hip_dpd_state *state, float *F, int64_t *acc, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_dpd_err = "null handle"; return MCRX_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    MCRX_OP_CHK(g_dpd_err, pd_serve_reset(q, st, dpd_launch_table));
    const size_t K = q->k.K;
    DpdState s = {};
    if (state) MCRX_OP_CHK(g_dpd_err, hipMemcpyAsync(&s, q->state, sizeof(s), hipMemcpyDeviceToHost, st));
    if (F) MCRX_OP_CHK(g_dpd_err, hipMemcpyAsync(F, q->F, 2 * (K + 1) * sizeof(float), hipMemcpyDeviceToHost, st));
    if (acc) MCRX_OP_CHK(g_dpd_err, hipMemcpyAsync(acc, q->acc, 4 * (K + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    MCRX_OP_CHK(g_dpd_err, hipStreamSynchronize(st));
    if (state) { state->updates = s.updates; state->skipped = s.skipped; state->degenerate = s.degenerate; }
    return MCRX_OK;
}

extern "C" int mcrx_hip_dpd_clipped(mcrx_hip_dpd_t q, uint64_t *samples, int reset)
{
    return op_clipped(q, g_dpd_err, samples, reset);
}
