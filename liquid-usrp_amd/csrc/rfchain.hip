// rfchain.hip -- RF front end on the wideband stream for gfx950: IQ imbalance and LO leakage, oscillator phase noise, amplifier
// compression; cf32 or sc16 in, cf32 or sc16 out (mcrx_hip_rfchain_*; the definition with every fmaf is in
// include/mcrx_hip.h).
//
// Memoryless in the samples and stateless: everything is a function of the sample's value and its ABSOLUTE index n, which the caller
// passes -- never of how the stream is cut into calls, of the GPU a time shard runs on or of the launch geometry.
//   mixer       u = alpha z + beta conj(z) + d              four nested fmaf per component
//   oscillator  u = z e(theta(n))                           theta(n) = fmaf(f, Theta[b+1] - Theta[b], Theta[b]), b = n >> L; sincos_u32,
//                                                           chanemu_sample's rotation
//   amplifier   u = (G z) e(phi)                            G = amp_gain / sqrtf(q(t)), t = |z|^2 / A^2; phi = ampm t / (1 + t) turns
//   order 0: mixer, oscillator, amplifier; order 1: amplifier, oscillator, mixer; then v = gain u, out = v or Q(v) (sc16.hpp)
// rfchain_phase_kernel writes the rows of Theta a span of samples needs into the handle's table (one float a row), a lane per row;
// the integers of its sinusoids are made on the host from pn_seed (rfchain_plan.hpp) and travel as kernel arguments.
//
// rfchain_kernel<STAGES, FIN, FOUT>: streaming, no LDS.  A lane owns the index-aligned pair (2k, 2k + 1): 2^L is even, so a pair never
// straddles a grid row and the two table rows serve both samples; its accesses are 16 bytes (sc16: 8) where the address allows -- a
// uniform choice, all lanes' pairs have the same parity.  The stage mask and the formats are template parameters: a build carries
// only its stages' code, and the build with none is load, convert, store.  `order`, the amplifier's smoothness and "AM/PM on" are
// wave-uniform branches on kernel arguments.  A lane writes only the samples it read: in-place use is allowed with equal formats.
//
// Contraction is switched off for this file: every build rounds the same way, so the integers of an sc16 handle are Q of a cf32
// handle's floats, and the products that matter are written as fmaf.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>
#include <string>
#include "../../include/mcrx_hip.h"
#include "devmath.h"
#include "fadegen.hpp"
#include "iqpair.hpp"
#include "ophost.hpp"
#include "rapp.hpp"
#include "rfchain_plan.hpp"
#include "span_plan.hpp"
#include "stream_call.hpp"

namespace mcrx {

enum { RF_MIX = MCRX_RFCHAIN_MIXER, RF_OSC = MCRX_RFCHAIN_OSCILLATOR, RF_AMP = MCRX_RFCHAIN_AMPLIFIER };

struct RfchainArgs {
    const void *in; void *out;
    unsigned long long *clip;                               // sc16-out builds: the handle's count of clipped samples
    uint64_t pos, n;                                        // absolute index of in[0]; samples of this launch
    uint32_t order;
    float ar, ai, br, bi, dr, di;                           // mixer
    // oscillator builds only: the table of this span, its row 0 = grid row row0 = pos >> L; rows = rows it holds; finv = 2^-L
    const float *tab; uint64_t row0; uint32_t L, rows; float finv;
    float inv_a2, amp_gain, ampm; uint32_t smooth;          // amplifier
    float gain;
};

// the oscillator's sinusoids
struct RfchainPhase {
    int64_t step[MCRX_RFCHAIN_MAX_SINUSOIDS];               // 2^64 * cycles per wideband sample
    uint32_t phase[MCRX_RFCHAIN_MAX_SINUSOIDS];             // 2^32 * cycles
    float c; uint32_t S;
};

// table[row] = Theta[row0 + row], row < rows: a lane per row, the integers are scalar loads
__global__ __launch_bounds__(256) void rfchain_phase_kernel(RfchainPhase t, float *table, uint64_t row0, uint32_t rows, uint32_t L)
{
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= rows) return;
    const uint64_t nb = (row0 + row) << L;                              // the grid index wraps with the 64-bit position
    float acc = 0.f;
    for (uint32_t k = 0; k < t.S; k++) {
        float sn, cs;
        sincos_u32((uint32_t)((((uint64_t)t.phase[k] << 32) + (uint64_t)t.step[k] * nb) >> 32), sn, cs);
        acc = fmaf(t.c, cs, acc);
    }
    table[row] = acc;
}

__device__ __forceinline__ float2 rfchain_mixer(const RfchainArgs &a, float2 z)
{
    return make_float2(fmaf(a.ar, z.x, fmaf(-a.ai, z.y, fmaf(a.br, z.x, fmaf(a.bi, z.y, a.dr)))),
                       fmaf(a.ar, z.y, fmaf(a.ai, z.x, fmaf(a.bi, z.x, fmaf(-a.br, z.y, a.di)))));
}
// the amplifier is rapp.hpp's, which pamem.hip's branches share
__device__ __forceinline__ float2 rfchain_amplifier(const RfchainArgs &a, float2 z)
{
    return rapp_amplifier(a.inv_a2, a.smooth, a.amp_gain, a.ampm, z);
}

template <int STAGES>
__device__ __forceinline__ float2 rfchain_sample(const RfchainArgs &a, float2 z, float theta)
{
    constexpr bool several = (STAGES & (STAGES - 1)) != 0;             // one stage alone has no sequence
    if (!several || a.order == 0u) {
        if (STAGES & RF_MIX) z = rfchain_mixer(a, z);
        if (STAGES & RF_OSC) z = rfchain_rotate(z, rfchain_phase_word(theta));
        if (STAGES & RF_AMP) z = rfchain_amplifier(a, z);
    } else {
        if (STAGES & RF_AMP) z = rfchain_amplifier(a, z);
        if (STAGES & RF_OSC) z = rfchain_rotate(z, rfchain_phase_word(theta));
        if (STAGES & RF_MIX) z = rfchain_mixer(a, z);
    }
    if (a.gain != 1.0f) z = make_float2(a.gain * z.x, a.gain * z.y);
    return z;
}

template <int STAGES, int FIN, int FOUT>
__global__ __launch_bounds__(256) void rfchain_kernel(RfchainArgs a)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const IqPair p = iq_pair(a.pos, a.n, g);                            // lane g owns the index-aligned pair g (iqpair.hpp)
    uint32_t nclip = 0;
    if (p.ok0 || p.ok1) {
        float2 x0, x1;                                                  // (the masked half of an edge pair computes on a zero)
        load_pair<FIN>(a.in, p, x0, x1);
        float th0 = 0.f, th1 = 0.f;
        if (STAGES & RF_OSC) {
            const uint64_t nabs = iq_pair_index(a.pos, g);
            const uint64_t row = ((nabs >> a.L) - a.row0) & (~(uint64_t)0 >> a.L);
            const float *trow = a.tab + (size_t)(row < a.rows - 1u ? row : a.rows - 2u);      // (row + 1 < rows for every pair of the span)
            const float T0 = trow[0], dT = trow[1] - T0;
            const uint32_t frac = (uint32_t)nabs & ((1u << a.L) - 1u);
            th0 = fmaf((float)frac * a.finv, dT, T0); th1 = fmaf((float)(frac + 1u) * a.finv, dT, T0);
        }
        const float2 v0 = rfchain_sample<STAGES>(a, x0, th0);
        const float2 v1 = rfchain_sample<STAGES>(a, x1, th1);
        nclip = store_pair<FOUT>(a.out, p, v0, v1);
    }
    if (FOUT == IQ_SC16) sc16_clip_commit(a.clip, nclip);               // every lane of every wave gets here
}

}  // namespace mcrx

using namespace mcrx;

static thread_local std::string g_rf_err;

struct mcrx_hip_rfchain_s {
    int device = -1;            // the HIP device the handle was created on: every entry point runs with it current (devscope.hpp)
    mcrx_hip_rfchain_config cfg;
    Sc16ClipCount clip;         // sc16-out handles only (allocated at creation): clipped samples since the handle was made
    RfchainPhase pt = {};       // oscillator on: its sinusoids
    uint32_t cap = 0;           // the most rows of the table a span may use
    DevBuffer tab;              // Theta's table, one float a row
};

// 2^18 rows = 1 MB at most (chanemu's row count): at L = 10 one span for 2.7e8 samples, at L = 6 spans of 1.7e7 samples
static const uint32_t RFCHAIN_DEFAULT_ROWS = 1u << 18;

extern "C" const char *mcrx_hip_rfchain_last_error(void) { return g_rf_err.c_str(); }

extern "C" int mcrx_hip_rfchain_selftest(const mcrx_hip_rfchain_config *cfg, int64_t *steps, uint32_t *phases, float *coef)
{
    if (!cfg || !steps || !phases || !coef) { g_rf_err = "null pointer"; return MCRX_EINVAL; }
    const char *bad = rfchain_check(cfg);
    if (!bad) bad = rfchain_osc_check(cfg);
    if (bad) { g_rf_err = bad; return MCRX_EINVAL; }
    rfchain_phase_integers(cfg, steps, phases, coef);
    return MCRX_OK;
}

extern "C" int mcrx_hip_rfchain_create(mcrx_hip_rfchain_t *out, const mcrx_hip_rfchain_config *cfg)
{
    if (!out) { g_rf_err = "null pointer"; return MCRX_EINVAL; }
    *out = nullptr;
    if (!cfg) { g_rf_err = "null configuration"; return MCRX_EINVAL; }
    if (const char *bad = rfchain_check(cfg)) { g_rf_err = bad; return MCRX_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { g_rf_err = "no HIP device (no CPU fallback)"; return MCRX_EHIP; }
    mcrx_hip_rfchain_t q = new mcrx_hip_rfchain_s();
    q->device = current_device();
    q->cfg = *cfg;
    if (cfg->stages & MCRX_RFCHAIN_OSCILLATOR) {
        q->pt.S = cfg->pn_sinusoids;
        rfchain_phase_integers(cfg, q->pt.step, q->pt.phase, &q->pt.c);
        q->cap = cfg->pn_table_rows ? cfg->pn_table_rows : RFCHAIN_DEFAULT_ROWS;
    }
    if (cfg->output_format == IQ_SC16) {
        const hipError_t e = q->clip.ensure();
        if (e != hipSuccess) { g_rf_err = std::string("clip counter: ") + hipGetErrorString(e); mcrx_hip_rfchain_destroy(q); return MCRX_EHIP; }
    }
    *out = q;
    return MCRX_OK;
}

extern "C" int mcrx_hip_rfchain_destroy(mcrx_hip_rfchain_t q)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) return MCRX_OK;
    (void)hipDeviceSynchronize();
    q->tab.release();
    q->clip.release();
    delete q;
    return MCRX_OK;
}

extern "C" unsigned mcrx_hip_rfchain_input_format(mcrx_hip_rfchain_t q) { return q ? q->cfg.input_format : 0u; }
extern "C" unsigned mcrx_hip_rfchain_output_format(mcrx_hip_rfchain_t q) { return q ? q->cfg.output_format : 0u; }

template <int FIN, int FOUT>
static void rfchain_launch(uint32_t stages, const RfchainArgs &a, dim3 grid, hipStream_t st)
{
    switch (stages) {
#define RFCHAIN_CASE(S) case S: hipLaunchKernelGGL((rfchain_kernel<S, FIN, FOUT>), grid, dim3(256), 0, st, a); break;
    RFCHAIN_CASE(0) RFCHAIN_CASE(1) RFCHAIN_CASE(2) RFCHAIN_CASE(3) RFCHAIN_CASE(4) RFCHAIN_CASE(5) RFCHAIN_CASE(6) RFCHAIN_CASE(7)
#undef RFCHAIN_CASE
    }
}

extern "C" int mcrx_hip_rfchain_execute_device(mcrx_hip_rfchain_t q, const void *d_in, uint64_t first_sample, size_t n, void *d_out, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_rf_err = "null handle"; return MCRX_EINVAL; }
    const mcrx_hip_rfchain_config &c = q->cfg;
    const bool in16 = c.input_format == IQ_SC16, out16 = c.output_format == IQ_SC16;
    const uint32_t si = in16 ? 4u : 8u, so = out16 ? 4u : 8u;
    if (const char *bad = stream_call_check(reinterpret_cast<uintptr_t>(d_in), reinterpret_cast<uintptr_t>(d_out), n, si, so, 0, true, false,
                                            "d_in and d_out overlap: in-place use takes d_in == d_out and equal formats")) { g_rf_err = bad; return MCRX_EINVAL; }
    if (n == 0) return MCRX_OK;
    hipStream_t st = (hipStream_t)stream;
    const bool osc = (c.stages & MCRX_RFCHAIN_OSCILLATOR) != 0;
    const uint32_t L = c.pn_log2_block;
    uint64_t cap = 0;                                                   // oscillator: the rows of the table a span may use (span_plan.hpp)
    if (osc) {
        cap = span_cap(span_rows(span_frac(first_sample, L), n, L), q->cap);
        const uint64_t have = q->tab.bytes / sizeof(float);
        if (cap > have) MCRX_OP_CHK(g_rf_err, q->tab.ensure((size_t)span_grow(have, q->cap, cap) * sizeof(float)));
    }
    RfchainArgs a = {};
    a.clip = q->clip.device(); a.order = c.order;
    a.ar = c.alpha_re; a.ai = c.alpha_im; a.br = c.beta_re; a.bi = c.beta_im; a.dr = c.dc_re; a.di = c.dc_im;
    if (c.stages & MCRX_RFCHAIN_AMPLIFIER) { a.inv_a2 = rfchain_inv_sat2(c.amp_sat); a.amp_gain = c.amp_gain; a.ampm = c.amp_ampm; a.smooth = c.amp_smooth; }
    a.gain = c.gain;
    // without the oscillator one span; with it, spans of at most cap - 1 grid intervals: table kernel -> samples' kernel each.
    // The operator is a function of the absolute index, so the spans are invisible in the output.
    uint64_t pos = first_sample;
    for (size_t off = 0; off < n; ) {
        size_t m = n - off;
        if (osc) {
            const Span<uint64_t> s = span_next(pos, m, L, cap);
            m = (size_t)s.m;
            a.L = L; a.row0 = s.row0; a.rows = (uint32_t)s.rows; a.tab = q->tab.as<float>();
            a.finv = std::ldexp(1.0f, -(int)L);
            hipLaunchKernelGGL(rfchain_phase_kernel, dim3((a.rows + 255) / 256), dim3(256), 0, st, q->pt, q->tab.as<float>(), a.row0, a.rows, L);
            MCRX_OP_CHK(g_rf_err, hipGetLastError());
        }
        a.in = static_cast<const char *>(d_in) + off * si;
        a.out = static_cast<char *>(d_out) + off * so;
        a.pos = pos; a.n = m;
        const dim3 grid((unsigned)((iq_pairs(pos, m) + 255) / 256));
        if (in16) { if (out16) rfchain_launch<IQ_SC16, IQ_SC16>(c.stages, a, grid, st); else rfchain_launch<IQ_SC16, IQ_CF32>(c.stages, a, grid, st); }
        else      { if (out16) rfchain_launch<IQ_CF32, IQ_SC16>(c.stages, a, grid, st); else rfchain_launch<IQ_CF32, IQ_CF32>(c.stages, a, grid, st); }
        MCRX_OP_CHK(g_rf_err, hipGetLastError());
        pos += m;
        off += m;
    }
    if (out16) MCRX_OP_CHK(g_rf_err, q->clip.mark(st));
    return MCRX_OK;
}

// the table kernel on its own, into the caller's buffer: what execute_device computes for itself, for tests and measurements
extern "C" int mcrx_hip_rfchain_phase_rows(mcrx_hip_rfchain_t q, uint64_t first_row, uint32_t rows, void *d_table, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_rf_err = "null handle"; return MCRX_EINVAL; }
    if (!(q->cfg.stages & MCRX_RFCHAIN_OSCILLATOR)) { g_rf_err = "the oscillator is off"; return MCRX_EINVAL; }
    if (!d_table || (reinterpret_cast<uintptr_t>(d_table) & 3u)) { g_rf_err = "d_table must be a 4-byte aligned device buffer"; return MCRX_EINVAL; }
    if (rows == 0) return MCRX_OK;
    hipLaunchKernelGGL(rfchain_phase_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, q->pt,
                       static_cast<float *>(d_table), first_row, rows, q->cfg.pn_log2_block);
    MCRX_OP_CHK(g_rf_err, hipGetLastError());
    return MCRX_OK;
}

extern "C" int mcrx_hip_rfchain_clipped(mcrx_hip_rfchain_t q, uint64_t *samples, int reset)
{
    return op_clipped(q, g_rf_err, samples, reset);
}
