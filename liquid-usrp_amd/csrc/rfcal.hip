// rfcal.hip -- receiver calibration on the wideband stream for gfx950: blind DC offset and IQ correction; cf32 or sc16 in, cf32 or sc16
// (or nothing) out (mcrx_hip_rfcal_*; the definition with every fmaf is in include/mcrx_hip.h).
//
// Stateful: the handle owns, in device memory, the coefficients (m, w), the running means R, the block accumulators and the counters
// (one mcrx_hip_rfcal_state) and a buffer of partial rows.  Nothing of it is read back by execute: what the host needs to choose a
// build (has there been an update or a set? is the handle held?) it knows itself.
//
// rfcal_kernel<FIN, FOUT, APPLY, MEASURE>: streaming, rfchain_kernel's lane layout -- a lane owns the index-aligned pair (2k, 2k + 1),
// 16-byte accesses (sc16: 8) where the address allows, a uniform choice.  A measuring build loops over pairs grid * 256 apart (the
// grid is capped at RFCAL_MAX_ROWS workgroups), sums its own samples' moments in registers -- int64 for sc16, fp64 for cf32 -- then
// the wave's tree, then LDS across the four waves, and writes ONE partial row of five sums; FOUT = RFCAL_NONE has no store at all.
// The coefficients are read once through a wave-uniform address.  LDS is used for the cross-wave sums only.
// rfcal_fold_kernel<FIN>: one workgroup.  Adds the rows in a fixed order (thread t the rows t, t + 256, ... ascending, the wave's tree, the
// four waves in order) to the block accumulators and, asked to, runs the update in thread 0 -- a block boundary costs two launches.
// rfcal_set_kernel: one lane; writes coefficients (mcrx_hip_rfcal_set) and serves a reset nothing else has carried yet.
//
// Contraction is switched off for this file, as in rfchain.hip: every build rounds the same way, so the integers of an sc16-out handle
// are Q of a cf32-out handle's floats, and pc^2 - |c2|^2 of a pure real signal is exactly 0.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>
#include <string>
#include "../../include/mcrx_hip.h"
#include "iqpair.hpp"
#include "ophost.hpp"
#include "rfcal_plan.hpp"
#include "stream_call.hpp"

namespace mcrx {

enum { RFCAL_NONE = 2 };                                    // FOUT of the measure-only builds

struct RfcalArgs {
    const void *in; void *out;
    const mcrx_hip_rfcal_state *state;                      // APPLY builds: the coefficients in its first 16 bytes
    void *rows;                                             // MEASURE builds: five 8-byte sums a workgroup, row = blockIdx.x
    unsigned long long *clip;                               // sc16-out builds: the handle's count of clipped samples
    uint64_t pos, n;                                        // absolute index of in[0]; samples of this launch
    float gain;
};

template <typename T> __device__ __forceinline__ T rfcal_wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int FIN> struct RfcalSum { typedef double type; };
template <> struct RfcalSum<IQ_SC16> { typedef long long type; };

template <int FIN, int FOUT, bool APPLY, bool MEASURE>
__global__ __launch_bounds__(RFCAL_WG) void rfcal_kernel(RfcalArgs a)
{
    typedef typename RfcalSum<FIN>::type sum_t;
    const uint64_t pairs = iq_pairs(a.pos, a.n), stride = (uint64_t)gridDim.x * RFCAL_WG;      // the index-aligned pairs (iqpair.hpp)
    float mr = 0.f, mi = 0.f, wr = 0.f, wi = 0.f;
    if (APPLY) {
        const float4 cf = *reinterpret_cast<const float4 *>(a.state);      // the same address in every lane
        mr = cf.x; mi = cf.y; wr = cf.z; wi = cf.w;
    }
    sum_t s1r = 0, s1i = 0, srr = 0, sii = 0, sri = 0;                  // sum re, im, re^2, im^2, re im of this lane's samples
    uint32_t nclip = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * RFCAL_WG + threadIdx.x; g < pairs; g += stride) {
        const IqPair p = iq_pair(a.pos, a.n, g);
        float2 x0 = make_float2(0.f, 0.f), x1 = x0;                     // (the masked half of an edge pair is a zero: it adds nothing)
        if (FIN == IQ_SC16) {
            uint32_t w0, w1;
            load_pair_words(a.in, p, w0, w1);
            if (MEASURE) {
                const int r0 = (int16_t)(w0 & 0xffffu), i0 = (int32_t)w0 >> 16, r1 = (int16_t)(w1 & 0xffffu), i1 = (int32_t)w1 >> 16;
                s1r += (sum_t)(r0 + r1); s1i += (sum_t)(i0 + i1);
                srr += (sum_t)((long long)(r0 * r0) + (long long)(r1 * r1)); sii += (sum_t)((long long)(i0 * i0) + (long long)(i1 * i1));
                sri += (sum_t)((long long)(r0 * i0) + (long long)(r1 * i1));
            }
            if (FOUT != RFCAL_NONE) { x0 = sc16_unpack(w0); x1 = sc16_unpack(w1); }
        } else {
            load_pair<IQ_CF32>(a.in, p, x0, x1);
            if (MEASURE) {          // fp64 products of fp32 values are exact, so fma(a, b, s) IS s + a * b: one instruction instead of two
                const double r0 = x0.x, i0 = x0.y, r1 = x1.x, i1 = x1.y;
                s1r += (sum_t)r0; s1r += (sum_t)r1; s1i += (sum_t)i0; s1i += (sum_t)i1;
                srr = (sum_t)__builtin_fma(r1, r1, __builtin_fma(r0, r0, (double)srr)); sii = (sum_t)__builtin_fma(i1, i1, __builtin_fma(i0, i0, (double)sii));
                sri = (sum_t)__builtin_fma(r1, i1, __builtin_fma(r0, i0, (double)sri));
            }
        }
        if (FOUT != RFCAL_NONE) {
            float2 v0 = x0, v1 = x1;
            if (APPLY) {
                const float t0r = x0.x - mr, t0i = x0.y - mi, t1r = x1.x - mr, t1i = x1.y - mi;
                v0 = make_float2(fmaf(-wr, t0r, fmaf(-wi, t0i, t0r)), fmaf(wr, t0i, fmaf(-wi, t0r, t0i)));
                v1 = make_float2(fmaf(-wr, t1r, fmaf(-wi, t1i, t1r)), fmaf(wr, t1i, fmaf(-wi, t1r, t1i)));
            }
            if (a.gain != 1.0f) { v0 = make_float2(a.gain * v0.x, a.gain * v0.y); v1 = make_float2(a.gain * v1.x, a.gain * v1.y); }
            nclip += store_pair<FOUT>(a.out, p, v0, v1);
        }
    }
    if (FOUT == IQ_SC16) sc16_clip_commit(a.clip, nclip);               // every lane of every wave gets here
    if (MEASURE) {
        __shared__ sum_t part[RFCAL_WG / 64][5];
        const sum_t t[5] = { rfcal_wave_sum(s1r), rfcal_wave_sum(s1i), rfcal_wave_sum(srr), rfcal_wave_sum(sii), rfcal_wave_sum(sri) };
        if ((threadIdx.x & 63u) == 0u)
            for (int k = 0; k < 5; k++) part[threadIdx.x >> 6][k] = t[k];
        __syncthreads();
        if (threadIdx.x == 0) {
            sum_t s[5];
            for (int k = 0; k < 5; k++) { s[k] = part[0][k]; for (int w = 1; w < RFCAL_WG / 64; w++) s[k] += part[w][k]; }
            sum_t *row = reinterpret_cast<sum_t *>(a.rows) + (size_t)blockIdx.x * 5;
            row[0] = s[0]; row[1] = s[1]; row[2] = s[2] - s[3]; row[3] = s[4] + s[4]; row[4] = s[2] + s[3];       // S1, S2, P
        }
    }
}

struct RfcalFold {
    mcrx_hip_rfcal_state *state;
    const void *rows; uint32_t nrows;                       // rows of the launch in front (0: none)
    uint64_t n;                                             // samples those rows hold
    uint32_t reset, update, stages, forget_log2;            // reset: clear the state first (mcrx_hip_rfcal_reset_at)
};

__device__ __forceinline__ void rfcal_clear(mcrx_hip_rfcal_state *s)
{
    s->m_re = s->m_im = s->w_re = s->w_im = 0.f;
    for (int k = 0; k < 5; k++) { s->mean[k] = 0.0; s->acc[k] = 0.0; s->acc_int[k] = 0; }
    s->count = s->updates = s->measured = s->degenerate = 0;
}

// the update (include/mcrx_hip.h), one lane
template <int FIN>
__device__ __forceinline__ void rfcal_update(mcrx_hip_rfcal_state *s, uint32_t stages, uint32_t forget_log2)
{
    if (s->count == 0) return;
    const double cnt = (double)s->count;
    double b[5];
    for (int k = 0; k < 5; k++) {
        if (FIN == IQ_SC16) b[k] = (double)s->acc_int[k] * (k < 2 ? 0x1p-15 : 0x1p-30) / cnt;
        else b[k] = s->acc[k] / cnt;
        s->acc[k] = 0.0; s->acc_int[k] = 0;
    }
    s->count = 0;
    bool finite = true;
    for (int k = 0; k < 5; k++) finite = finite && std::isfinite(b[k]);
    if (!finite) { s->degenerate += 1; return; }
    double R[5];
    const double mu = rfcal_mu(s->updates, forget_log2);
    for (int k = 0; k < 5; k++) { R[k] = s->updates == 0 ? b[k] : s->mean[k] + mu * (b[k] - s->mean[k]); s->mean[k] = R[k]; }
    s->updates += 1;
    const double mr = R[0], mi = R[1];
    const double c2r = R[2] - (mr * mr - mi * mi), c2i = R[3] - 2.0 * (mr * mi), pc = R[4] - (mr * mr + mi * mi);
    const double D = pc * pc - (c2r * c2r + c2i * c2i);
    if (!(pc > 0.0) || !(D > 0.0) || !std::isfinite(D)) { s->degenerate += 1; return; }
    const double den = pc + sqrt(D);
    const bool dc = (stages & MCRX_RFCAL_DC) != 0, iq = (stages & MCRX_RFCAL_IQ) != 0;
    s->m_re = dc ? (float)mr : 0.f; s->m_im = dc ? (float)mi : 0.f;
    s->w_re = iq ? (float)(c2r / den) : 0.f; s->w_im = iq ? (float)(c2i / den) : 0.f;
}

template <int FIN>
__global__ __launch_bounds__(RFCAL_WG) void rfcal_fold_kernel(RfcalFold f)
{
    typedef typename RfcalSum<FIN>::type sum_t;
    __shared__ sum_t part[RFCAL_WG / 64][5];
    const sum_t *rows = reinterpret_cast<const sum_t *>(f.rows);
    sum_t s[5] = { 0, 0, 0, 0, 0 };
    for (uint32_t r = threadIdx.x; r < f.nrows; r += RFCAL_WG)          // thread t: rows t, t + 256, ... ascending
        for (int k = 0; k < 5; k++) s[k] += rows[(size_t)r * 5 + k];
    for (int k = 0; k < 5; k++) s[k] = rfcal_wave_sum(s[k]);            // the wave's tree, then the four waves in order
    if ((threadIdx.x & 63u) == 0u)
        for (int k = 0; k < 5; k++) part[threadIdx.x >> 6][k] = s[k];
    __syncthreads();
    if (threadIdx.x != 0) return;
    sum_t tot[5];
    for (int k = 0; k < 5; k++) { tot[k] = part[0][k]; for (int w = 1; w < RFCAL_WG / 64; w++) tot[k] += part[w][k]; }
    mcrx_hip_rfcal_state *st = f.state;
    if (f.reset) rfcal_clear(st);
    if (f.nrows) {
        for (int k = 0; k < 5; k++) { if (FIN == IQ_SC16) st->acc_int[k] += (long long)tot[k]; else st->acc[k] += (double)tot[k]; }
        st->count += f.n; st->measured += f.n;
    }
    if (f.update) rfcal_update<FIN>(st, f.stages, f.forget_log2);
}

__global__ __launch_bounds__(64) void rfcal_set_kernel(mcrx_hip_rfcal_state *st, uint32_t reset, uint32_t set, float mr, float mi, float wr, float wi)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (reset) rfcal_clear(st);
    if (set) { st->m_re = mr; st->m_im = mi; st->w_re = wr; st->w_im = wi; }
}

}  // namespace mcrx

using namespace mcrx;

static thread_local std::string g_cal_err;

struct mcrx_hip_rfcal_s {
    int device = -1;            // the HIP device the handle was created on: every entry point runs with it current (devscope.hpp)
    mcrx_hip_rfcal_config cfg;
    Sc16ClipCount clip;         // sc16-out handles only
    mcrx_hip_rfcal_state *state = nullptr;      // device
    void *rows = nullptr;       // device: RFCAL_MAX_ROWS partial rows of five 8-byte sums
    uint64_t pos = 0;           // absolute index of the next sample
    uint64_t since = 0;         // samples measured since the last update (the 2^31 guard)
    bool calibrated = false;    // an update or a set has been enqueued since the reset: launches carry the apply code
    bool held = false;
    bool reset_pending = false; // the next fold / set kernel clears the state first
};

extern "C" const char *mcrx_hip_rfcal_last_error(void) { return g_cal_err.c_str(); }

// the call (pos, n) as execute judges it before it touches a buffer: nullptr or what is wrong
static const char *rfcal_call_check(const mcrx_hip_rfcal_config *c, uint64_t pos, uint64_t n, uint64_t since, bool measures)
{
    if (n > ((uint64_t)1 << 32)) return "at most 2^32 samples a call";
    if (measures && c->input_format == IQ_SC16 && n) {
        bool ends;
        if (!rfcal_guard_ok(since, rfcal_segment(pos, n, c->period_log2, &ends)))
            return "more than 2^31 sc16 samples between two updates: the int64 moments could overflow";
    }
    return nullptr;
}

extern "C" int mcrx_hip_rfcal_selftest(const mcrx_hip_rfcal_config *cfg, uint64_t pos, uint64_t n, uint64_t *seg_len, uint32_t *seg_updates,
                                       size_t cap, uint64_t *nseg)
{
    if (!cfg || !nseg || (cap && (!seg_len || !seg_updates))) { g_cal_err = "null pointer"; return MCRX_EINVAL; }
    const char *bad = rfcal_check(cfg);
    if (!bad) bad = rfcal_call_check(cfg, pos, n, 0, true);
    if (bad) { g_cal_err = bad; return MCRX_EINVAL; }
    *nseg = rfcal_segments(pos, n, cfg->period_log2);
    uint64_t p = pos, left = n;
    for (size_t i = 0; i < cap && left; i++) {
        bool ends;
        const uint64_t m = rfcal_segment(p, left, cfg->period_log2, &ends);
        seg_len[i] = m; seg_updates[i] = ends ? 1u : 0u;
        p += m; left -= m;
    }
    return MCRX_OK;
}

extern "C" int mcrx_hip_rfcal_create(mcrx_hip_rfcal_t *out, const mcrx_hip_rfcal_config *cfg)
{
    if (!out) { g_cal_err = "null pointer"; return MCRX_EINVAL; }
    *out = nullptr;
    if (!cfg) { g_cal_err = "null configuration"; return MCRX_EINVAL; }
    if (const char *bad = rfcal_check(cfg)) { g_cal_err = bad; return MCRX_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { g_cal_err = "no HIP device (no CPU fallback)"; return MCRX_EHIP; }
    mcrx_hip_rfcal_t q = new mcrx_hip_rfcal_s();
    q->device = current_device();
    q->cfg = *cfg;
    hipError_t e = hipMalloc((void **)&q->state, sizeof(mcrx_hip_rfcal_state));
    if (e == hipSuccess) e = hipMemset(q->state, 0, sizeof(mcrx_hip_rfcal_state));
    if (e == hipSuccess) e = hipMalloc(&q->rows, (size_t)RFCAL_MAX_ROWS * 5 * 8);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && cfg->output_format == IQ_SC16) e = q->clip.ensure();
    if (e != hipSuccess) { g_cal_err = std::string("device state: ") + hipGetErrorString(e); mcrx_hip_rfcal_destroy(q); return MCRX_EHIP; }
    *out = q;
    return MCRX_OK;
}

extern "C" int mcrx_hip_rfcal_destroy(mcrx_hip_rfcal_t q)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) return MCRX_OK;
    (void)hipDeviceSynchronize();
    if (q->state) (void)hipFree(q->state);
    if (q->rows) (void)hipFree(q->rows);
    q->clip.release();
    delete q;
    return MCRX_OK;
}

extern "C" int mcrx_hip_rfcal_reset_at(mcrx_hip_rfcal_t q, uint64_t pos)
{
    if (!q) { g_cal_err = "null handle"; return MCRX_EINVAL; }
    q->pos = pos; q->since = 0; q->calibrated = false; q->reset_pending = true;
    return MCRX_OK;
}

extern "C" uint64_t mcrx_hip_rfcal_position(mcrx_hip_rfcal_t q) { return q ? q->pos : 0u; }

extern "C" int mcrx_hip_rfcal_hold(mcrx_hip_rfcal_t q, int on)
{
    if (!q) { g_cal_err = "null handle"; return MCRX_EINVAL; }
    q->held = on != 0;
    return MCRX_OK;
}

template <int FIN, int FOUT>
static void rfcal_launch(bool apply, bool measure, const RfcalArgs &a, dim3 grid, hipStream_t st)
{
    if (apply) { if (measure) hipLaunchKernelGGL((rfcal_kernel<FIN, FOUT, true, true>), grid, dim3(RFCAL_WG), 0, st, a);
                 else         hipLaunchKernelGGL((rfcal_kernel<FIN, FOUT, true, false>), grid, dim3(RFCAL_WG), 0, st, a); }
    else       { if (measure) hipLaunchKernelGGL((rfcal_kernel<FIN, FOUT, false, true>), grid, dim3(RFCAL_WG), 0, st, a);
                 else         hipLaunchKernelGGL((rfcal_kernel<FIN, FOUT, false, false>), grid, dim3(RFCAL_WG), 0, st, a); }
}

// fold (rows of the launch in front, if any) and, asked to, update; carries a pending reset
static hipError_t rfcal_fold(mcrx_hip_rfcal_t q, uint32_t nrows, uint64_t n, bool update, hipStream_t st)
{
    RfcalFold f = {};
    f.state = q->state; f.rows = q->rows; f.nrows = nrows; f.n = n;
    f.reset = q->reset_pending ? 1u : 0u; f.update = update ? 1u : 0u; f.stages = q->cfg.stages; f.forget_log2 = q->cfg.forget_log2;
    if (q->cfg.input_format == IQ_SC16) hipLaunchKernelGGL(rfcal_fold_kernel<IQ_SC16>, dim3(1), dim3(RFCAL_WG), 0, st, f);
    else hipLaunchKernelGGL(rfcal_fold_kernel<IQ_CF32>, dim3(1), dim3(RFCAL_WG), 0, st, f);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        q->reset_pending = false;
        if (update) { q->since = 0; q->calibrated = true; }
    }
    return e;
}

extern "C" int mcrx_hip_rfcal_execute_device(mcrx_hip_rfcal_t q, const void *d_in, size_t n, void *d_out, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_cal_err = "null handle"; return MCRX_EINVAL; }
    const mcrx_hip_rfcal_config &c = q->cfg;
    const bool in16 = c.input_format == IQ_SC16, out16 = c.output_format == IQ_SC16;
    const uint32_t si = in16 ? 4u : 8u, so = out16 ? 4u : 8u;
    const bool measure = !q->held;
    static const char *const overlap = "d_in and d_out overlap: in-place use takes d_in == d_out and equal formats";
    const char *bad = stream_call_check(reinterpret_cast<uintptr_t>(d_in), reinterpret_cast<uintptr_t>(d_out), n, si, so, 0, true, true, overlap);
    if (!bad || bad == overlap)                                         // the guard of the sc16 moments is judged in front of the overlap
        if (const char *guard = rfcal_call_check(&c, q->pos, n, q->since, measure)) bad = guard;
    if (bad) { g_cal_err = bad; return MCRX_EINVAL; }
    if (n == 0) return MCRX_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!measure && !d_out) { q->pos += n; return MCRX_OK; }            // held and nothing to write
    if (q->reset_pending && !measure) {                                 // no fold in this call to carry the reset
        hipLaunchKernelGGL(rfcal_set_kernel, dim3(1), dim3(64), 0, st, q->state, 1u, 0u, 0.f, 0.f, 0.f, 0.f);
        MCRX_OP_CHK(g_cal_err, hipGetLastError());
        q->reset_pending = false;
    }
    RfcalArgs a = {};
    a.state = q->state; a.rows = q->rows; a.clip = q->clip.device(); a.gain = c.gain;
    // a measuring call is split at the block boundaries of the absolute index: samples' kernel -> fold (+ update) each; one that does
    // not measure is one launch
    for (size_t off = 0; off < n; ) {
        bool ends = false;
        const uint64_t m = measure ? rfcal_segment(q->pos, n - off, c.period_log2, &ends) : (uint64_t)(n - off);
        const bool apply = q->calibrated && d_out;          // (a reset still pending means not calibrated: the stale state is not read)
        a.in = static_cast<const char *>(d_in) + off * si;
        a.out = d_out ? static_cast<char *>(d_out) + off * so : nullptr;
        a.pos = q->pos; a.n = m;
        const dim3 grid(rfcal_grid(q->pos, m, measure));
        if (!d_out) {
            if (in16) hipLaunchKernelGGL((rfcal_kernel<IQ_SC16, RFCAL_NONE, false, true>), grid, dim3(RFCAL_WG), 0, st, a);
            else      hipLaunchKernelGGL((rfcal_kernel<IQ_CF32, RFCAL_NONE, false, true>), grid, dim3(RFCAL_WG), 0, st, a);
        } else if (in16) { if (out16) rfcal_launch<IQ_SC16, IQ_SC16>(apply, measure, a, grid, st); else rfcal_launch<IQ_SC16, IQ_CF32>(apply, measure, a, grid, st); }
        else             { if (out16) rfcal_launch<IQ_CF32, IQ_SC16>(apply, measure, a, grid, st); else rfcal_launch<IQ_CF32, IQ_CF32>(apply, measure, a, grid, st); }
        MCRX_OP_CHK(g_cal_err, hipGetLastError());
        q->pos += m;
        off += (size_t)m;
        if (measure) {
            q->since += m;
            MCRX_OP_CHK(g_cal_err, rfcal_fold(q, grid.x, m, ends, st));
        }
    }
    if (d_out && out16) MCRX_OP_CHK(g_cal_err, q->clip.mark(st));
    return MCRX_OK;
}

extern "C" int mcrx_hip_rfcal_update(mcrx_hip_rfcal_t q, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_cal_err = "null handle"; return MCRX_EINVAL; }
    if (q->cfg.period_log2 != 0u) { g_cal_err = "the handle updates by itself (period_log2 != 0)"; return MCRX_EINVAL; }
    if (q->held) return MCRX_OK;                                        // while held the update changes nothing
    MCRX_OP_CHK(g_cal_err, rfcal_fold(q, 0u, 0u, true, (hipStream_t)stream));
    return MCRX_OK;
}

extern "C" int mcrx_hip_rfcal_set(mcrx_hip_rfcal_t q, float m_re, float m_im, float w_re, float w_im, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_cal_err = "null handle"; return MCRX_EINVAL; }
    if (!std::isfinite(m_re) || !std::isfinite(m_im) || !std::isfinite(w_re) || !std::isfinite(w_im)) { g_cal_err = "the coefficients must be finite"; return MCRX_EINVAL; }
    hipLaunchKernelGGL(rfcal_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, q->state, q->reset_pending ? 1u : 0u, 1u, m_re, m_im, w_re, w_im);
    MCRX_OP_CHK(g_cal_err, hipGetLastError());
    q->reset_pending = false; q->calibrated = true;
    return MCRX_OK;
}

extern "C" int mcrx_hip_rfcal_read(mcrx_hip_rfcal_t q, mcrx_hip_rfcal_state *out, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_cal_err = "null handle"; return MCRX_EINVAL; }
    if (!out) { g_cal_err = "null pointer"; return MCRX_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    if (q->reset_pending) {
        hipLaunchKernelGGL(rfcal_set_kernel, dim3(1), dim3(64), 0, st, q->state, 1u, 0u, 0.f, 0.f, 0.f, 0.f);
        MCRX_OP_CHK(g_cal_err, hipGetLastError());
        q->reset_pending = false;
    }
    MCRX_OP_CHK(g_cal_err, hipMemcpyAsync(out, q->state, sizeof(*out), hipMemcpyDeviceToHost, st));
    MCRX_OP_CHK(g_cal_err, hipStreamSynchronize(st));
    return MCRX_OK;
}

extern "C" int mcrx_hip_rfcal_clipped(mcrx_hip_rfcal_t q, uint64_t *samples, int reset)
{
    return op_clipped(q, g_cal_err, samples, reset);
}
