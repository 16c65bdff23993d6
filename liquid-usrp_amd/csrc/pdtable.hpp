// pdtable.hpp -- what a gain-table predistorter is, once, for dpd.hip (one table) and mpd.hip (1 to 4 branch tables): a complex gain
// looked up by amplitude in a table of K intervals and interpolated, times the sample (DESIGN.md sections 4.21 / 4.22; the definition
// with every fmaf is in include/mcrx_hip.h).  Three parts:
//   the plan (pd_plan.hpp): the constants of a table, the guard of int64 sums and the sizes of a streaming launch; no device, any host compiler
//             (dpd_plan.hpp and mpd_plan.hpp build on it, host/dpd_plan_test.cc and host/mpd_plan_test.cc compile it);
//   the device part (hipcc only): the two halves of the lookup, the single-table streaming kernel with its launcher, the quadruples;
//   the host handle (hipcc only): the fields and the entry-point bodies the operators share, in the style of ophost.hpp's op_clipped:
//             each takes the operator's error string and, where a kernel of the operator's is needed, the function that launches it.
#pragma once
#include <cmath>
#include <stdint.h>
#include "pd_plan.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include <string>
#include "../../include/mcrx_hip.h"
#include "iqpair.hpp"
#include "ophost.hpp"
#include "stream_call.hpp"

namespace mcrx {

// The lookup in its two halves: what depends on the sample alone -- (x.re, x.im, fraction, index) --, and one table's gain and product
__device__ __forceinline__ float4 pd_stage(float2 x, float inv_step, float Kf, int Km1)
{
    const float t = fmaf(x.x, x.x, x.y * x.y), a = sqrtf(t);
    const float s = fminf(a * inv_step, Kf);
    const int k = min((int)s, Km1);
    return make_float4(x.x, x.y, s - (float)k, __int_as_float(k));
}
__device__ __forceinline__ float2 pd_branch(const float4 *tab, float4 w)
{
    const float4 q = tab[__float_as_int(w.w)];
    const float gr = fmaf(w.z, q.z, q.x), gi = fmaf(w.z, q.w, q.y);
    return make_float2(fmaf(gr, w.x, -(gi * w.y)), fmaf(gr, w.y, gi * w.x));
}

struct PdArgs {                                             // a single-table streaming launch
    const void *in; void *out;
    const float4 *quads;                                    // APPLY builds: K quadruples (F[k].re, F[k].im, dF.re, dF.im)
    unsigned long long *clip;                               // sc16-out builds: the handle's count of clipped samples
    uint64_t parity, n;                                     // (address of in[0] / 8) & 1; samples of this launch
    uint32_t K, rounds; float inv_step, gain;               // rounds: of 256 pairs a workgroup takes (pd_rounds; the copy build: 1)
};

// Streaming, rfchain_kernel's lane layout: a lane owns an index-aligned pair, 16-byte accesses where the address allows.  A workgroup
// of an APPLY build stages the table's quadruples in LDS once (16 bytes * K), so that a sample's gather is one 16-byte LDS read.  The
// build without APPLY has no LDS and no table: load, [gain,] convert, store.
template <int FOUT, bool APPLY>
__global__ __launch_bounds__(PD_WG) void pd_stream_kernel(PdArgs a)
{
    extern __shared__ float4 pd_tab[];
    if (APPLY) {
        for (uint32_t k = threadIdx.x; k < a.K; k += PD_WG) pd_tab[k] = a.quads[k];
        __syncthreads();
    }
    const float Kf = (float)a.K;
    const int Km1 = (int)a.K - 1;
    uint32_t nclip = 0;
    // A workgroup owns a.rounds * 256 consecutive pairs and takes them 256 at a time; an APPLY build has the loads of PD_UNROLL rounds
    // in flight before it computes on the first (a pair beyond the launch is masked on both halves: it loads and stores nothing).
    // The copy build has one round: a lane a pair.
    constexpr int U = APPLY ? (int)PD_UNROLL : 1;
    const uint64_t base = (uint64_t)blockIdx.x * a.rounds * PD_WG + threadIdx.x;
    for (uint32_t r = 0; r < a.rounds; r += U) {
        IqPair p[U];
        float2 x0[U], x1[U];                                            // (the masked half of an edge pair computes on a zero)
#pragma unroll
        for (int u = 0; u < U; u++) {
            p[u] = iq_pair(a.parity, a.n, base + (uint64_t)(r + u) * PD_WG);
            load_pair<IQ_CF32>(a.in, p[u], x0[u], x1[u]);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            float2 v0 = x0[u], v1 = x1[u];
            if (APPLY) { v0 = pd_branch(pd_tab, pd_stage(v0, a.inv_step, Kf, Km1)); v1 = pd_branch(pd_tab, pd_stage(v1, a.inv_step, Kf, Km1)); }
            if (a.gain != 1.0f) { v0 = make_float2(a.gain * v0.x, a.gain * v0.y); v1 = make_float2(a.gain * v1.x, a.gain * v1.y); }
            nclip += store_pair<FOUT>(a.out, p[u], v0, v1);
        }
    }
    if (FOUT == IQ_SC16) sc16_clip_commit(a.clip, nclip);               // every lane of every wave gets here
}

// quads[m K + k] = (F_m[k], F_m[k+1] - F_m[k]): the same fp32 subtraction the definition writes
__device__ __forceinline__ void pd_write_quads(const float2 *F, float4 *quads, uint32_t M, uint32_t K)
{
    for (uint32_t i = threadIdx.x; i < M * K; i += PD_WG) {
        const uint32_t m = i / K, k = i - m * K;
        const float2 f0 = F[m * (K + 1u) + k], f1 = F[m * (K + 1u) + k + 1u];
        quads[i] = make_float4(f0.x, f0.y, f1.x - f0.x, f1.y - f0.y);
    }
}

// What dpd's and mpd's handles share.  mem is one device block: the operator's state, the quadruples, its sums, the tables.
struct PdHandle {
    int device = -1;            // the HIP device the handle was created on: every entry point runs with it current (devscope.hpp)
    Sc16ClipCount clip;         // sc16-out handles only
    char *mem = nullptr;
    float2 *F = nullptr; float4 *quads = nullptr;
    uint64_t since = 0;         // terms offered since the last reset, following the updates' shifts (the guard)
    bool trained = false;       // an update or a set_table(s) has been enqueued since the reset: launches carry the apply code
    bool reset_pending = false; // the next kernel that touches the state clears it first
};

// n samples from `in` to `out` through one table (apply) or none: the one place that picks among pd_stream_kernel's four builds
static inline hipError_t pd_stream_launch(bool out16, bool apply, const void *in, void *out, uint64_t n, const float4 *quads, unsigned long long *clip,
                                          uint32_t K, float inv_step, float gain, hipStream_t st)
{
    PdArgs a = {};
    a.in = in; a.out = out; a.quads = quads; a.clip = clip;
    a.parity = (reinterpret_cast<uintptr_t>(in) >> 3) & 1u; a.n = n;
    a.K = K; a.inv_step = inv_step; a.gain = gain;
    a.rounds = apply ? pd_rounds(K) : 1u;
    const dim3 grid(pd_stream_grid(a.parity, n, a.rounds)), wg(PD_WG);
    const uint32_t lds = apply ? pd_stream_lds(K) : 0u;
    if (apply) { if (out16) hipLaunchKernelGGL((pd_stream_kernel<IQ_SC16, true>), grid, wg, lds, st, a);
                 else       hipLaunchKernelGGL((pd_stream_kernel<IQ_CF32, true>), grid, wg, lds, st, a); }
    else       { if (out16) hipLaunchKernelGGL((pd_stream_kernel<IQ_SC16, false>), grid, wg, lds, st, a);
                 else       hipLaunchKernelGGL((pd_stream_kernel<IQ_CF32, false>), grid, wg, lds, st, a); }
    return hipGetLastError();
}

// create, behind the configuration check: the device, the block of state_bytes | M K quadruples | sums_bytes | M tables of K + 1, zeroed,
// and the clip counter of an sc16-out handle: the state lies at mem, the sums behind the quadruples.  On failure nothing is held and
// the caller deletes q.
static inline int pd_alloc(PdHandle *q, std::string &err, bool out16, size_t M, size_t K, size_t state_bytes, size_t sums_bytes)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { err = "no HIP device (no CPU fallback)"; return MCRX_EHIP; }
    q->device = current_device();
    const size_t o_quads = (state_bytes + 15u) & ~(size_t)15u, o_sums = o_quads + M * K * sizeof(float4);
    const size_t o_F = o_sums + sums_bytes, bytes = o_F + M * (K + 1) * sizeof(float2);
    hipError_t e = hipMalloc((void **)&q->mem, bytes);
    if (e == hipSuccess) {
        q->quads = reinterpret_cast<float4 *>(q->mem + o_quads);
        q->F = reinterpret_cast<float2 *>(q->mem + o_F);
        e = hipMemset(q->mem, 0, bytes);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && out16) e = q->clip.ensure();
    if (e != hipSuccess) {
        err = std::string("device state: ") + hipGetErrorString(e);
        (void)hipDeviceSynchronize();
        if (q->mem) (void)hipFree(q->mem);
        q->clip.release();
        return MCRX_EHIP;
    }
    q->reset_pending = true;                                            // the tables are (1, 0 ...) before anything reads them
    return MCRX_OK;
}

template <typename Handle> static int pd_destroy(Handle *q)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) return MCRX_OK;
    (void)hipDeviceSynchronize();
    if (q->mem) (void)hipFree(q->mem);
    q->clip.release();
    delete q;
    return MCRX_OK;
}

static inline int pd_reset(PdHandle *q, std::string &err)
{
    if (!q) { err = "null handle"; return MCRX_EINVAL; }
    q->since = 0; q->trained = false; q->reset_pending = true;
    return MCRX_OK;
}

// The state cleared if a reset is pending: in front of every kernel that reads or writes tables, sums or counters.
// table(q, st, reset) launches the operator's table kernel: with reset != 0 it clears first, either way it writes the quadruples.
template <typename Handle> static hipError_t pd_serve_reset(Handle *q, hipStream_t st, void (*table)(Handle *, hipStream_t, uint32_t))
{
    if (!q->reset_pending) return hipSuccess;
    table(q, st, 1u);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) q->reset_pending = false;
    return e;
}

// set_table(s): M tables of K + 1 finite complex gains from the caller's F
template <typename Handle>
static int pd_set_tables(Handle *q, std::string &err, const char *not_finite, const float *F, size_t M, size_t K, void *stream,
                         void (*table)(Handle *, hipStream_t, uint32_t))
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { err = "null handle"; return MCRX_EINVAL; }
    if (!F) { err = "null pointer"; return MCRX_EINVAL; }
    const size_t nf = 2 * M * (K + 1);
    for (size_t i = 0; i < nf; i++)
        if (!std::isfinite(F[i])) { err = not_finite; return MCRX_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    MCRX_OP_CHK(err, pd_serve_reset(q, st, table));
    MCRX_OP_CHK(err, hipMemcpyAsync(q->F, F, nf * sizeof(float), hipMemcpyHostToDevice, st));
    MCRX_OP_CHK(err, hipStreamSynchronize(st));                          // F is the caller's: it has been read when this returns
    table(q, st, 0u);
    MCRX_OP_CHK(err, hipGetLastError());
    q->trained = true;
    return MCRX_OK;
}

// What measure_device checks of a call: two inputs, nothing written -- the call check once per buffer (an overlap of u and z harms
// nothing) --, then the guard on the `terms` the call would add.  nullptr or what is wrong.
static inline const char *pd_measure_check(const PdHandle *q, const void *d_u, const void *d_z, size_t n, uint64_t terms, uint32_t guard_log2,
                                           const char *guard_msg)
{
    const char *bad = stream_call_check(reinterpret_cast<uintptr_t>(d_u), 0, n, 8u, 8u, 0, false, true, "");
    if (!bad) bad = stream_call_check(reinterpret_cast<uintptr_t>(d_z), 0, n, 8u, 8u, 0, false, true, "");
    if (!bad && !pd_guard_ok(q->since, terms, guard_log2)) bad = guard_msg;
    return bad;
}

}  // namespace mcrx
#endif
