// dpd.hip -- digital predistortion on the wideband stream for gfx950: a complex gain table looked up by amplitude, learned on the
// device from the amplifier's input and output; cf32 in, cf32 or sc16 out (mcrx_hip_dpd_*; the definition
// with every fmaf is in include/mcrx_hip.h).
//
// The handle owns, in device memory, the table F[0 .. K], the same table as K quadruples (F[k], F[k+1] - F[k]), the accumulators
// (four int64 a bin) and the counters.  Nothing of it is read back by a launch's host side: whether there has been an update or a
// set_table, and how many samples have been offered, the host knows itself.
//
// dpd_kernel<FOUT, APPLY>: streaming, rfchain_kernel's lane layout -- a lane owns an index-aligned pair, 16-byte accesses where the
// address allows, the parity taken from d_in's address.  A workgroup of an APPLY build stages the table's quadruples in LDS once
// (16 bytes * K), so that a sample's gather is one 16-byte LDS read, and takes K / 32 (at least 4) rounds of 256 consecutive pairs,
// four rounds' loads in flight at a time: the staging is 1/16 of the bytes it streams.  The build without APPLY has no LDS, no table
// and no loop (a lane a pair, rfchain_kernel's grid): load, [gain,] convert, store.
// dpd_measure_kernel: the same lanes over (u, z); a histogram in the workgroup's LDS -- three 64-bit sums and a 32-bit count per bin,
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
#include "iqpair.hpp"
#include "ophost.hpp"
#include "stream_call.hpp"

namespace mcrx {

struct DpdArgs {
    const void *in; void *out;
    const float4 *quads;                                    // APPLY builds: K quadruples (F[k].re, F[k].im, dF.re, dF.im)
    unsigned long long *clip;                               // sc16-out builds: the handle's count of clipped samples
    uint64_t parity, n;                                     // (address of in[0] / 8) & 1; samples of this launch
    uint32_t K, rounds; float inv_step, gain;               // rounds: of 256 pairs a workgroup takes (dpd_rounds)
};

__device__ __forceinline__ float2 dpd_sample(const float4 *tab, float2 x, float inv_step, float Kf, int Km1)
{
    const float t = fmaf(x.x, x.x, x.y * x.y), a = sqrtf(t);
    const float s = fminf(a * inv_step, Kf);
    const int k = min((int)s, Km1);
    const float f = s - (float)k;
    const float4 q = tab[k];
    const float gr = fmaf(f, q.z, q.x), gi = fmaf(f, q.w, q.y);
    return make_float2(fmaf(gr, x.x, -(gi * x.y)), fmaf(gr, x.y, gi * x.x));
}

template <int FOUT, bool APPLY>
__global__ __launch_bounds__(DPD_WG) void dpd_kernel(DpdArgs a)
{
    extern __shared__ float4 dpd_tab[];
    if (APPLY) {
        for (uint32_t k = threadIdx.x; k < a.K; k += DPD_WG) dpd_tab[k] = a.quads[k];
        __syncthreads();
    }
    const float Kf = (float)a.K;
    const int Km1 = (int)a.K - 1;
    uint32_t nclip = 0;
    // A workgroup owns a.rounds * 256 consecutive pairs and takes them 256 at a time; an APPLY build has the loads of DPD_UNROLL rounds
    // in flight before it computes on the first (a pair beyond the launch is masked on both halves: it loads and stores nothing).
    // The copy build has one round: a lane a pair.
    constexpr int U = APPLY ? (int)DPD_UNROLL : 1;
    const uint64_t base = (uint64_t)blockIdx.x * a.rounds * DPD_WG + threadIdx.x;
    for (uint32_t r = 0; r < a.rounds; r += U) {
        IqPair p[U];
        float2 x0[U], x1[U];                                            // (the masked half of an edge pair computes on a zero)
#pragma unroll
        for (int u = 0; u < U; u++) {
            p[u] = iq_pair(a.parity, a.n, base + (uint64_t)(r + u) * DPD_WG);
            load_pair<IQ_CF32>(a.in, p[u], x0[u], x1[u]);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            float2 v0 = x0[u], v1 = x1[u];
            if (APPLY) { v0 = dpd_sample(dpd_tab, v0, a.inv_step, Kf, Km1); v1 = dpd_sample(dpd_tab, v1, a.inv_step, Kf, Km1); }
            if (a.gain != 1.0f) { v0 = make_float2(a.gain * v0.x, a.gain * v0.y); v1 = make_float2(a.gain * v1.x, a.gain * v1.y); }
            nclip += store_pair<FOUT>(a.out, p[u], v0, v1);
        }
    }
    if (FOUT == IQ_SC16) sc16_clip_commit(a.clip, nclip);               // every lane of every wave gets here
}

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

// quads[k] = (F[k], F[k+1] - F[k]): the same fp32 subtraction the definition writes
__device__ __forceinline__ void dpd_write_quads(const float2 *F, float4 *quads, uint32_t K)
{
    for (uint32_t k = threadIdx.x; k < K; k += DPD_WG) {
        const float2 f0 = F[k], f1 = F[k + 1];
        quads[k] = make_float4(f0.x, f0.y, f1.x - f0.x, f1.y - f0.y);
    }
}

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
    dpd_write_quads(p.F, p.quads, p.K);
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
    dpd_write_quads(F, quads, K);
}

}  // namespace mcrx

using namespace mcrx;

static thread_local std::string g_dpd_err;

struct mcrx_hip_dpd_s {
    int device = -1;            // the HIP device the handle was created on: every entry point runs with it current (devscope.hpp)
    mcrx_hip_dpd_config cfg;
    DpdConsts k;
    Sc16ClipCount clip;         // sc16-out handles only
    char *mem = nullptr;        // device: DpdState, F, quads, acc
    DpdState *state = nullptr; float2 *F = nullptr; float4 *quads = nullptr; long long *acc = nullptr;
    uint64_t since = 0;         // samples offered since the last reset, following the updates' shifts (the 2^28 guard)
    bool trained = false;       // an update or a set_table has been enqueued since the reset: launches carry the apply code
    bool reset_pending = false; // the next kernel that touches the state clears it first
};

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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { g_dpd_err = "no HIP device (no CPU fallback)"; return MCRX_EHIP; }
    mcrx_hip_dpd_t q = new mcrx_hip_dpd_s();
    q->device = current_device();
    q->cfg = *cfg;
    q->k = dpd_consts(cfg);
    const size_t K = q->k.K;
    const size_t o_quads = sizeof(DpdState), o_acc = o_quads + K * sizeof(float4), o_F = o_acc + 4 * (K + 1) * sizeof(long long);
    const size_t bytes = o_F + (K + 1) * sizeof(float2);
    hipError_t e = hipMalloc((void **)&q->mem, bytes);
    if (e == hipSuccess) {
        q->state = reinterpret_cast<DpdState *>(q->mem);
        q->quads = reinterpret_cast<float4 *>(q->mem + o_quads);
        q->acc = reinterpret_cast<long long *>(q->mem + o_acc);
        q->F = reinterpret_cast<float2 *>(q->mem + o_F);
        e = hipMemset(q->mem, 0, bytes);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && cfg->output_format == IQ_SC16) e = q->clip.ensure();
    if (e != hipSuccess) { g_dpd_err = std::string("device state: ") + hipGetErrorString(e); mcrx_hip_dpd_destroy(q); return MCRX_EHIP; }
    q->reset_pending = true;                                            // the table is 1 before anything reads it
    *out = q;
    return MCRX_OK;
}

extern "C" int mcrx_hip_dpd_destroy(mcrx_hip_dpd_t q)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) return MCRX_OK;
    (void)hipDeviceSynchronize();
    if (q->mem) (void)hipFree(q->mem);
    q->clip.release();
    delete q;
    return MCRX_OK;
}

extern "C" unsigned mcrx_hip_dpd_output_format(mcrx_hip_dpd_t q) { return q ? q->cfg.output_format : 0u; }

extern "C" int mcrx_hip_dpd_reset(mcrx_hip_dpd_t q)
{
    if (!q) { g_dpd_err = "null handle"; return MCRX_EINVAL; }
    q->since = 0; q->trained = false; q->reset_pending = true;
    return MCRX_OK;
}

// the state cleared if a reset is pending: in front of every kernel that reads or writes table, accumulators or counters
static hipError_t dpd_serve_reset(mcrx_hip_dpd_t q, hipStream_t st)
{
    if (!q->reset_pending) return hipSuccess;
    hipLaunchKernelGGL(dpd_table_kernel, dim3(1), dim3(DPD_WG), 0, st, q->state, q->F, q->quads, q->acc, q->k.K, 1u);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) q->reset_pending = false;
    return e;
}

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
    const bool apply = q->trained;                                      // (a reset still pending means not trained: the stale table is not read)
    DpdArgs a = {};
    a.in = d_in; a.out = d_out; a.quads = q->quads; a.clip = q->clip.device();
    a.parity = (reinterpret_cast<uintptr_t>(d_in) >> 3) & 1u; a.n = n;
    a.K = q->k.K; a.inv_step = q->k.inv_step; a.gain = q->cfg.gain;
    a.rounds = apply ? dpd_rounds(a.K) : 1u;
    const dim3 grid(dpd_apply_grid(a.parity, n, a.rounds)), wg(DPD_WG);
    const uint32_t lds = apply ? dpd_apply_lds(a.K) : 0u;
    if (apply) { if (out16) hipLaunchKernelGGL((dpd_kernel<IQ_SC16, true>), grid, wg, lds, st, a);
                 else       hipLaunchKernelGGL((dpd_kernel<IQ_CF32, true>), grid, wg, lds, st, a); }
    else       { if (out16) hipLaunchKernelGGL((dpd_kernel<IQ_SC16, false>), grid, wg, lds, st, a);
                 else       hipLaunchKernelGGL((dpd_kernel<IQ_CF32, false>), grid, wg, lds, st, a); }
    MCRX_OP_CHK(g_dpd_err, hipGetLastError());
    if (out16) MCRX_OP_CHK(g_dpd_err, q->clip.mark(st));
    return MCRX_OK;
}

extern "C" int mcrx_hip_dpd_measure_device(mcrx_hip_dpd_t q, const void *d_u, const void *d_z, size_t n, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_dpd_err = "null handle"; return MCRX_EINVAL; }
    // two inputs, nothing written: the call check once per buffer (an overlap of u and z harms nothing)
    const char *bad = stream_call_check(reinterpret_cast<uintptr_t>(d_u), 0, n, 8u, 8u, 0, false, true, "");
    if (!bad) bad = stream_call_check(reinterpret_cast<uintptr_t>(d_z), 0, n, 8u, 8u, 0, false, true, "");
    if (!bad && !dpd_guard_ok(q->since, n)) bad = "more than 2^28 samples offered since the last reset: the int64 sums could overflow";
    if (bad) { g_dpd_err = bad; return MCRX_EINVAL; }
    if (n == 0) return MCRX_OK;
    hipStream_t st = (hipStream_t)stream;
    MCRX_OP_CHK(g_dpd_err, dpd_serve_reset(q, st));
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
    MCRX_OP_CHK(g_dpd_err, dpd_serve_reset(q, st));
    DpdUpdate p = {};
    p.state = q->state; p.F = q->F; p.quads = q->quads; p.acc = q->acc;
    p.K = q->k.K; p.min_count = q->cfg.min_count; p.forget_shift = q->cfg.forget_shift;
    p.step = q->k.step; p.g0 = (double)q->cfg.target_gain;
    hipLaunchKernelGGL(dpd_update_kernel, dim3(1), dim3(DPD_WG), 0, st, p);
    MCRX_OP_CHK(g_dpd_err, hipGetLastError());
    q->since = dpd_guard_after_update(q->since, q->cfg.forget_shift);
    q->trained = true;
    return MCRX_OK;
}

extern "C" int mcrx_hip_dpd_set_table(mcrx_hip_dpd_t q, const float *F, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_dpd_err = "null handle"; return MCRX_EINVAL; }
    if (!F) { g_dpd_err = "null pointer"; return MCRX_EINVAL; }
    const size_t nf = 2 * ((size_t)q->k.K + 1);
    for (size_t i = 0; i < nf; i++)
        if (!std::isfinite(F[i])) { g_dpd_err = "the table must be finite"; return MCRX_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    MCRX_OP_CHK(g_dpd_err, dpd_serve_reset(q, st));
    MCRX_OP_CHK(g_dpd_err, hipMemcpyAsync(q->F, F, nf * sizeof(float), hipMemcpyHostToDevice, st));
    MCRX_OP_CHK(g_dpd_err, hipStreamSynchronize(st));                    // F is the caller's: it has been read when this returns
    hipLaunchKernelGGL(dpd_table_kernel, dim3(1), dim3(DPD_WG), 0, st, q->state, q->F, q->quads, q->acc, q->k.K, 0u);
    MCRX_OP_CHK(g_dpd_err, hipGetLastError());
    q->trained = true;
    return MCRX_OK;
}

extern "C" int mcrx_hip_dpd_read(mcrx_hip_dpd_t q, mcrx_hip_dpd_state *state, float *F, int64_t *acc, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_dpd_err = "null handle"; return MCRX_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    MCRX_OP_CHK(g_dpd_err, dpd_serve_reset(q, st));
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
