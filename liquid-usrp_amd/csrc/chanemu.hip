// chanemu.hip -- channel emulator on the wideband stream for gfx950: sparse multipath, carrier offset, white noise, cf32 or sc16 out
// (mcrx_hip_chanemu_*).
//
// Everything is a function of the ABSOLUTE sample index n, never of how the stream is cut into calls or of the launch geometry:
//   s[n] = sum_{i<T} a_i x[n - d_i]                    table order, two explicit fused multiply-adds per tap and component
//   r[n] = s[n] e^{+j 2 pi th_n / 2^32}                 th_n = phase0 + cfo_step n mod 2^32 (closed form), sincos_u32, cmul_fx's shape
//   v[n] = gain r[n] + noise_std w[n]                   one multiply, one fused multiply-add per component
//   out  = v[n] (cf32)  or  Q(v[n]) (sc16: sc16.hpp, the shared quantiser as it stands)
// w[n]: Box-Muller on the words Philox4x32-10 gives for counter (n >> 1, 0, 0) and key seed; sample n takes words 2 (n & 1), 2 (n & 1) + 1.
//
// With fading on (mcrx_hip_chanfade_*) the constant a_i becomes g_i(n) a_i, where g_i is a sum of sinusoids sampled
// on the grid n = b 2^L and interpolated linearly between its rows -- a function of n again:
//   G_i[b] = c_los_i e((psi_i << 32) + Lambda_i n_b) + c_sc_i sum_{k<S} e((Phi_ik << 32) + N_ik n_b)      n_b = b << L, phases mod 2^64,
//                                                       e(p) = sincos_u32(p >> 32); LOS first, then k ascending, one fmaf per term
//   g_i(n) = fmaf(f, G_i[b+1] - G_i[b], G_i[b])          b = n >> L, f = (n & (2^L - 1)) 2^-L (exact), per component
//   s[n]   = sum_i (g_i(n) a_i) x[n - d_i]               the product in cmul_fx's shape, then the two fmaf per component as above
// chanemu_gain_kernel writes the rows a span of samples needs into the handle's table (float2 [row][MCRX_CHANEMU_MAX_TAPS]), a lane per
// (row, ray); chanemu_kernel<..., FADE = true> reads two rows per ray.  The integers (steps, phases) are made on the host from the
// fading seed (fading_ray) and travel as kernel arguments.
//
// chanemu_kernel<ROT, NOISE, FMT, FADE>: streaming, no LDS.  A lane owns the index-aligned pair (2k, 2k + 1): one Philox evaluation serves
// it, and its accesses are 16 bytes where the address allows (a uniform choice per tap: all lanes' pairs have the same parity).  A tap's
// reads are the input shifted by d_i -- coalesced, re-reading lines the neighbouring lanes and workgroups fetch anyway.  Reads in
// front of the call's first sample come from the handle's history (the last D = max d_i inputs), of which hist_len are valid; the rest
// are the zeros in front of the last reset.  Builds without rotation / noise carry none of that code (template parameters).
// chanemu_history_kernel brings the history up to date behind it, from the old history and the call's input into the OTHER of two
// buffers (a call shorter than D shifts the history, which cannot be done in place).
//
// Contraction is switched off for this file: sincos_u32's polynomials and everything else round the same way in every build, so the
// integers of an sc16 handle are Q of a cf32 handle's floats, and the products that matter are written as fmaf.
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
#include "span_plan.hpp"
#include "stream_call.hpp"

namespace mcrx {

// (Philox4x32-10 comes from fadegen.hpp: the same code on host -- mcrx_hip_chanemu_selftest_words -- and device)
// the words of the pair that holds absolute sample n
__host__ __device__ inline Philox4 chanemu_pair_words(uint64_t seed, uint64_t n)
{
    const uint64_t c = n >> 1;
    return philox4x32_10((uint32_t)c, (uint32_t)(c >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

struct ChanemuArgs {
    const float2 *in; void *out; const float2 *hist;        // hist[D]: x[pos - D .. pos), its last hist_len entries valid
    unsigned long long *clip;                               // sc16 builds: the handle's count of clipped samples
    uint64_t pos, n;                                        // absolute index of in[0]; samples of this call
    uint32_t D, hist_len, T;
    uint32_t delay[MCRX_CHANEMU_MAX_TAPS];
    float are[MCRX_CHANEMU_MAX_TAPS], aim[MCRX_CHANEMU_MAX_TAPS];
    uint32_t cfo_step, phase0;
    float gain, nstd;
    uint64_t seed;
    // FADE builds only: the gain table of this span, its row 0 = grid row row0 = pos >> L; rows = rows it holds; finv = 2^-L
    const float2 *gtab; uint64_t row0; uint32_t L, rows; float finv;
};

// The sinusoids of the fading gains: per ray the line-of-sight term [0] and S scattered ones [1 .. S]
struct FadeTables {
    int64_t step[MCRX_CHANEMU_MAX_TAPS][MCRX_CHANEMU_MAX_SINUSOIDS + 1];      // 2^64 * cycles per wideband sample
    uint32_t phase[MCRX_CHANEMU_MAX_TAPS][MCRX_CHANEMU_MAX_SINUSOIDS + 1];    // 2^32 * cycles
    float c_los[MCRX_CHANEMU_MAX_TAPS], c_sc[MCRX_CHANEMU_MAX_TAPS];
    uint32_t S;
};

// table[row][ray] = G_ray[row0 + row], row < rows: blockIdx.y is the ray (its integers are scalar loads), a lane per row
__global__ __launch_bounds__(256) void chanemu_gain_kernel(FadeTables t, float2 *table, uint64_t row0, uint32_t rows, uint32_t L)
{
    const uint32_t row = blockIdx.x * 256u + threadIdx.x, ray = blockIdx.y;
    if (row >= rows) return;
    const uint64_t nb = (row0 + row) << L;                              // the grid index wraps with the 64-bit position
    float sn, cs;
    sincos_u32((uint32_t)((((uint64_t)t.phase[ray][0] << 32) + (uint64_t)t.step[ray][0] * nb) >> 32), sn, cs);
    float2 G = make_float2(t.c_los[ray] * cs, t.c_los[ray] * sn);
    const float c = t.c_sc[ray];
    for (uint32_t k = 1; k <= t.S; k++) {
        sincos_u32((uint32_t)((((uint64_t)t.phase[ray][k] << 32) + (uint64_t)t.step[ray][k] * nb) >> 32), sn, cs);
        G.x = fmaf(c, cs, G.x); G.y = fmaf(c, sn, G.y);
    }
    table[(size_t)row * MCRX_CHANEMU_MAX_TAPS + ray] = G;
}

// x[pos + r] for one sample: the input, the history, or a zero in front of the last reset (and for the masked half of an edge pair)
__device__ __forceinline__ float2 chanemu_fetch(const ChanemuArgs &a, long long r)
{
    if (r >= 0) return r < (long long)a.n ? a.in[r] : make_float2(0.f, 0.f);
    return -r <= (long long)a.hist_len ? a.hist[(long long)a.D + r] : make_float2(0.f, 0.f);
}
// the pair x[pos + r], x[pos + r + 1]
__device__ __forceinline__ void chanemu_fetch_pair(const ChanemuArgs &a, long long r, float2 &x0, float2 &x1)
{
    if (r >= 0 && r + 1 < (long long)a.n) {
        const float2 *p = a.in + r;
        if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0) {          // (uniform: r = 2 lane + a constant)
            const float4 v = *reinterpret_cast<const float4 *>(p);
            x0 = make_float2(v.x, v.y); x1 = make_float2(v.z, v.w);
        } else { x0 = p[0]; x1 = p[1]; }
    } else { x0 = chanemu_fetch(a, r); x1 = chanemu_fetch(a, r + 1); }
}

template <bool ROT, bool NOISE>
__device__ __forceinline__ float2 chanemu_sample(const ChanemuArgs &a, float2 s, uint64_t nabs, uint32_t w0, uint32_t w1)
{
    float2 r = s;
    if (ROT) {
        float sn, cs;
        sincos_u32(a.phase0 + a.cfo_step * (uint32_t)nabs, sn, cs);
        r = make_float2(fmaf(s.x, cs, -(s.y * sn)), fmaf(s.x, sn, s.y * cs));
    }
    float2 v = make_float2(a.gain * r.x, a.gain * r.y);
    if (NOISE) {
        const float u1 = ((float)(w0 >> 9) + 0.5f) * 1.1920928955078125e-07f;      // 2^-23: exact, in (0, 1)
        const float rho = sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincos_u32((w1 >> 8) << 8, sn, cs);                                       // 2 pi u2, u2 = (w1 >> 8) 2^-24
        const float wr = rho * cs, wi = rho * sn;
        v = make_float2(fmaf(a.nstd, wr, v.x), fmaf(a.nstd, wi, v.y));
    }
    return v;
}

template <bool ROT, bool NOISE, int FMT, bool FADE>
__global__ __launch_bounds__(256) void chanemu_kernel(ChanemuArgs a)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const IqPair p = iq_pair(a.pos, a.n, g);                            // lane g owns the index-aligned pair g (iqpair.hpp)
    uint32_t nclip = 0;
    if (p.ok0 || p.ok1) {
        float2 x0[MCRX_CHANEMU_MAX_TAPS], x1[MCRX_CHANEMU_MAX_TAPS];
#pragma unroll
        for (int i = 0; i < MCRX_CHANEMU_MAX_TAPS; i++)                 // every tap's loads first: T pairs in flight
            if (i < (int)a.T) chanemu_fetch_pair(a, p.m0 - (long long)a.delay[i], x0[i], x1[i]);
        const uint64_t nabs = iq_pair_index(a.pos, g);
        float2 s0 = make_float2(0.f, 0.f), s1 = s0;
        // FADE: the pair's grid row (2^L is even: a pair never straddles one) relative to the table's first, and its two fractions
        const float2 *grow = nullptr;
        float f0 = 0.f, f1 = 0.f;
        if (FADE) {
            const uint64_t row = ((nabs >> a.L) - a.row0) & (~(uint64_t)0 >> a.L);
            grow = a.gtab + (size_t)(row < a.rows - 1u ? row : a.rows - 2u) * MCRX_CHANEMU_MAX_TAPS;     // (row + 1 < rows for every pair of the span)
            const uint32_t frac = (uint32_t)nabs & ((1u << a.L) - 1u);
            f0 = (float)frac * a.finv; f1 = (float)(frac + 1u) * a.finv;
        }
#pragma unroll
        for (int i = 0; i < MCRX_CHANEMU_MAX_TAPS; i++)
            if (i < (int)a.T && FADE) {
                const float2 G0 = grow[i], G1 = grow[MCRX_CHANEMU_MAX_TAPS + i];
                const float dx = G1.x - G0.x, dy = G1.y - G0.y;
                const float2 av = make_float2(a.are[i], a.aim[i]);
                const float2 h0 = cmul_fx(make_float2(fmaf(f0, dx, G0.x), fmaf(f0, dy, G0.y)), av);
                const float2 h1 = cmul_fx(make_float2(fmaf(f1, dx, G0.x), fmaf(f1, dy, G0.y)), av);
                s0.x = fmaf(h0.x, x0[i].x, fmaf(-h0.y, x0[i].y, s0.x)); s0.y = fmaf(h0.x, x0[i].y, fmaf(h0.y, x0[i].x, s0.y));
                s1.x = fmaf(h1.x, x1[i].x, fmaf(-h1.y, x1[i].y, s1.x)); s1.y = fmaf(h1.x, x1[i].y, fmaf(h1.y, x1[i].x, s1.y));
            } else if (i < (int)a.T) {
                const float ar = a.are[i], ai = a.aim[i];
                s0.x = fmaf(ar, x0[i].x, fmaf(-ai, x0[i].y, s0.x)); s0.y = fmaf(ar, x0[i].y, fmaf(ai, x0[i].x, s0.y));
                s1.x = fmaf(ar, x1[i].x, fmaf(-ai, x1[i].y, s1.x)); s1.y = fmaf(ar, x1[i].y, fmaf(ai, x1[i].x, s1.y));
            }
        Philox4 w = {};
        if (NOISE) w = chanemu_pair_words(a.seed, nabs);
        const float2 v0 = chanemu_sample<ROT, NOISE>(a, s0, nabs, w.w[0], w.w[1]);
        const float2 v1 = chanemu_sample<ROT, NOISE>(a, s1, nabs + 1, w.w[2], w.w[3]);
        nclip = store_pair<FMT>(a.out, p, v0, v1);
    }
    if (FMT == IQ_SC16) sc16_clip_commit(a.clip, nclip);               // every lane of every wave gets here
}

// next[j] = x[pos + n - D + j], j < D: from the old history while j + n < D, from the input behind it
__global__ __launch_bounds__(256) void chanemu_history_kernel(ChanemuArgs a, float2 *next)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= a.D) return;
    next[j] = chanemu_fetch(a, (long long)a.n - (long long)a.D + (long long)j);
}

}  // namespace mcrx

using namespace mcrx;

static thread_local std::string g_ce_err;

struct mcrx_hip_chanemu_s {
    int device = -1;            // the HIP device the handle was created on: every entry point runs with it current (devscope.hpp)
    mcrx_hip_chanemu_config cfg;
    uint32_t D = 0;             // max d_i
    uint64_t pos = 0;           // absolute index of the next input sample
    uint32_t hist_len = 0;      // valid samples at the end of hist[cur] (the rest: zeros in front of the last reset)
    float2 *hist[2] = { nullptr, nullptr }; int cur = 0;
    Sc16ClipCount clip;         // sc16 handles only (allocated at creation): clipped samples since the handle was made
    bool fade = false;          // fading on: ft holds the sinusoids of rays 0 .. num_taps - 1
    FadeTables ft = {};
    uint32_t fade_L = 0, fade_cap = 0;              // log2 of the update interval; the most rows of the table a span may use
    DevBuffer gtab;             // the gain table, float2 [row][MCRX_CHANEMU_MAX_TAPS]
};

// 2^18 rows = 16 MB at most, and only what a call needs: at L = 10 that is one span for 2.7e8 samples (the 512-channel slab is 2.1e8),
// at L = 6 a span of 1.7e7 samples = 0.27 GB of traffic, against which three launches are nothing; a larger table buys no speed
static const uint32_t FADE_DEFAULT_ROWS = 1u << 18;

static const char *fading_check(const mcrx_hip_chanemu_fading *f, unsigned ray0, unsigned ray1)
{
    if (f->struct_size != sizeof(mcrx_hip_chanemu_fading)) return "mcrx_hip_chanemu_fading: wrong struct_size";
    if (f->log2_block < 1 || f->log2_block > 24) return "log2_block must be 1 .. 24";
    if (f->num_sinusoids < 1 || f->num_sinusoids > MCRX_CHANEMU_MAX_SINUSOIDS) return "num_sinusoids must be 1 .. 16";
    if (f->table_rows == 1) return "table_rows must be 0 (default) or at least 2";
    const double B = (double)(1u << f->log2_block);
    for (unsigned i = ray0; i < ray1; i++)
        if (const char *bad = fade_ray_check(B, f->doppler[i], f->los_doppler[i], f->rice_k[i])) return bad;
    return nullptr;
}

// the integers and coefficients of one ray (a checked configuration): entry 0 the line-of-sight term, then the S scattered sinusoids
static void fading_ray(const mcrx_hip_chanemu_fading *f, unsigned i, int64_t *steps, uint32_t *phases, float coef[2])
{
    fade_ray_integers(f->seed, i, 1u, 0u, f->num_sinusoids, f->doppler[i], f->los_doppler[i], f->rice_k[i], f->los_phase[i], steps, phases, coef);
}

extern "C" int mcrx_hip_chanfade_selftest(const mcrx_hip_chanemu_fading *f, unsigned ray, int64_t *steps, uint32_t *phases, float coef[2])
{
    if (!f || !steps || !phases || !coef) { g_ce_err = "null pointer"; return MCRX_EINVAL; }
    if (ray >= MCRX_CHANEMU_MAX_TAPS) { g_ce_err = "ray must be 0 .. 7"; return MCRX_EINVAL; }
    if (const char *bad = fading_check(f, ray, ray + 1)) { g_ce_err = bad; return MCRX_EINVAL; }
    fading_ray(f, ray, steps, phases, coef);
    return MCRX_OK;
}

extern "C" int mcrx_hip_chanfade_set(mcrx_hip_chanemu_t q, const mcrx_hip_chanemu_fading *f)
{
    if (!q) { g_ce_err = "null handle"; return MCRX_EINVAL; }
    if (!f) { q->fade = false; return MCRX_OK; }
    if (const char *bad = fading_check(f, 0, q->cfg.num_taps)) { g_ce_err = bad; return MCRX_EINVAL; }
    FadeTables &t = q->ft;
    t = FadeTables();
    t.S = f->num_sinusoids;
    for (uint32_t i = 0; i < q->cfg.num_taps; i++) {
        float coef[2];
        fading_ray(f, i, t.step[i], t.phase[i], coef);
        t.c_los[i] = coef[0]; t.c_sc[i] = coef[1];
    }
    q->fade_L = f->log2_block;
    q->fade_cap = f->table_rows ? f->table_rows : FADE_DEFAULT_ROWS;
    q->fade = true;
    return MCRX_OK;
}
extern "C" int mcrx_hip_chanfade_on(mcrx_hip_chanemu_t q) { return q && q->fade ? 1 : 0; }

extern "C" const char *mcrx_hip_chanemu_last_error(void) { return g_ce_err.c_str(); }

extern "C" int mcrx_hip_chanemu_selftest_words(uint64_t seed, uint64_t position, uint32_t out[2])
{
    if (!out) { g_ce_err = "null pointer"; return MCRX_EINVAL; }
    const Philox4 w = chanemu_pair_words(seed, position);
    const unsigned j = 2u * (unsigned)(position & 1u);
    out[0] = w.w[j]; out[1] = w.w[j + 1];
    return MCRX_OK;
}

extern "C" int mcrx_hip_chanemu_create(mcrx_hip_chanemu_t *out, const mcrx_hip_chanemu_config *cfg)
{
    if (!out) { g_ce_err = "null pointer"; return MCRX_EINVAL; }
    *out = nullptr;
    if (!cfg) { g_ce_err = "null configuration"; return MCRX_EINVAL; }
    if (cfg->struct_size != sizeof(mcrx_hip_chanemu_config)) { g_ce_err = "mcrx_hip_chanemu_config: wrong struct_size"; return MCRX_EINVAL; }
    if (cfg->num_taps < 1 || cfg->num_taps > MCRX_CHANEMU_MAX_TAPS) { g_ce_err = "num_taps must be 1 .. 8"; return MCRX_EINVAL; }
    uint32_t D = 0;
    for (uint32_t i = 0; i < cfg->num_taps; i++) {
        if (cfg->delay[i] > MCRX_CHANEMU_MAX_DELAY) { g_ce_err = "a delay exceeds MCRX_CHANEMU_MAX_DELAY"; return MCRX_EINVAL; }
        if (!std::isfinite(cfg->tap_re[i]) || !std::isfinite(cfg->tap_im[i])) { g_ce_err = "taps must be finite"; return MCRX_EINVAL; }
        D = cfg->delay[i] > D ? cfg->delay[i] : D;
    }
    if (!std::isfinite(cfg->gain)) { g_ce_err = "gain must be finite"; return MCRX_EINVAL; }
    if (!std::isfinite(cfg->noise_std) || cfg->noise_std < 0.f) { g_ce_err = "noise_std must be finite and not negative"; return MCRX_EINVAL; }
    if (cfg->output_format != IQ_CF32 && cfg->output_format != IQ_SC16) { g_ce_err = "output format must be 0 (cf32) or 1 (sc16)"; return MCRX_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { g_ce_err = "no HIP device (no CPU fallback)"; return MCRX_EHIP; }
    mcrx_hip_chanemu_t q = new mcrx_hip_chanemu_s();
    q->device = current_device();
    q->cfg = *cfg; q->D = D;
    auto fail = [&](hipError_t e, const char *what) { g_ce_err = std::string(what) + ": " + hipGetErrorString(e); mcrx_hip_chanemu_destroy(q); return MCRX_EHIP; };
    hipError_t e;
    for (int b = 0; b < 2 && D; b++)
        if ((e = hipMalloc((void **)&q->hist[b], (size_t)D * sizeof(float2))) != hipSuccess) return fail(e, "hipMalloc(history)");
    if (cfg->output_format == IQ_SC16) {
        if ((e = q->clip.ensure()) != hipSuccess) return fail(e, "clip counter");
    }
    *out = q;
    return MCRX_OK;
}

extern "C" int mcrx_hip_chanemu_destroy(mcrx_hip_chanemu_t q)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) return MCRX_OK;
    (void)hipDeviceSynchronize();
    for (float2 *p : q->hist) if (p) (void)hipFree(p);
    q->gtab.release();
    q->clip.release();
    delete q;
    return MCRX_OK;
}

// no device work: the history is marked empty, and what the kernels read in front of it are zeros
extern "C" int mcrx_hip_chanemu_reset_at(mcrx_hip_chanemu_t q, uint64_t position)
{
    if (!q) { g_ce_err = "null handle"; return MCRX_EINVAL; }
    q->pos = position; q->hist_len = 0;
    return MCRX_OK;
}
extern "C" int mcrx_hip_chanemu_reset(mcrx_hip_chanemu_t q) { return mcrx_hip_chanemu_reset_at(q, 0); }
extern "C" uint64_t mcrx_hip_chanemu_position(mcrx_hip_chanemu_t q) { return q ? q->pos : 0; }
extern "C" unsigned mcrx_hip_chanemu_output_format(mcrx_hip_chanemu_t q) { return q ? q->cfg.output_format : 0u; }

template <int FMT, bool FADE>
static void chanemu_launch(const ChanemuArgs &a, bool rot, bool noise, dim3 grid, hipStream_t st)
{
    if (rot) { if (noise) hipLaunchKernelGGL((chanemu_kernel<true, true, FMT, FADE>), grid, dim3(256), 0, st, a);
               else       hipLaunchKernelGGL((chanemu_kernel<true, false, FMT, FADE>), grid, dim3(256), 0, st, a); }
    else     { if (noise) hipLaunchKernelGGL((chanemu_kernel<false, true, FMT, FADE>), grid, dim3(256), 0, st, a);
               else       hipLaunchKernelGGL((chanemu_kernel<false, false, FMT, FADE>), grid, dim3(256), 0, st, a); }
}

extern "C" int mcrx_hip_chanemu_execute_device(mcrx_hip_chanemu_t q, const void *d_in, size_t n, void *d_out, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_ce_err = "null handle"; return MCRX_EINVAL; }
    const bool sc16 = q->cfg.output_format == IQ_SC16;
    if (const char *bad = stream_call_check(reinterpret_cast<uintptr_t>(d_in), reinterpret_cast<uintptr_t>(d_out), n, 8u, sc16 ? 4u : 8u, 0, false, false,
                                            "d_in and d_out overlap: the taps read behind the write front, in-place use is not possible")) { g_ce_err = bad; return MCRX_EINVAL; }
    if (n == 0) return MCRX_OK;
    hipStream_t st = (hipStream_t)stream;
    const mcrx_hip_chanemu_config &c = q->cfg;
    const bool fade = q->fade;
    const uint32_t L = q->fade_L;
    const size_t row_bytes = MCRX_CHANEMU_MAX_TAPS * sizeof(float2);
    uint64_t cap = 0;                                                   // fading: the rows of the table a span may use (span_plan.hpp)
    if (fade) {
        cap = span_cap(span_rows(span_frac(q->pos, L), n, L), q->fade_cap);
        const uint64_t have = q->gtab.bytes / row_bytes;
        if (cap > have) MCRX_OP_CHK(g_ce_err, q->gtab.ensure((size_t)span_grow(have, q->fade_cap, cap) * row_bytes));
    }
    ChanemuArgs a = {};
    a.clip = q->clip.device(); a.D = q->D; a.T = c.num_taps;
    for (uint32_t i = 0; i < c.num_taps; i++) { a.delay[i] = c.delay[i]; a.are[i] = c.tap_re[i]; a.aim[i] = c.tap_im[i]; }
    a.cfo_step = c.cfo_step; a.phase0 = c.phase0; a.gain = c.gain; a.nstd = c.noise_std; a.seed = c.seed;
    const bool rot = c.cfo_step != 0 || c.phase0 != 0, noise = c.noise_std != 0.f;
    // without fading one span; with it, spans of at most cap - 1 grid intervals: gain kernel -> main kernel -> history kernel each.
    // The operator is cut-invariant, so the spans are invisible in the output.
    for (size_t off = 0; off < n; ) {
        size_t m = n - off;
        if (fade) {
            const Span<uint64_t> s = span_next(q->pos, m, L, cap);
            m = (size_t)s.m;
            a.L = L; a.row0 = s.row0; a.rows = (uint32_t)s.rows; a.gtab = q->gtab.as<float2>();
            a.finv = std::ldexp(1.0f, -(int)L);
            hipLaunchKernelGGL(chanemu_gain_kernel, dim3((a.rows + 255) / 256, c.num_taps), dim3(256), 0, st, q->ft, q->gtab.as<float2>(), a.row0, a.rows, L);
            MCRX_OP_CHK(g_ce_err, hipGetLastError());
        }
        a.in = static_cast<const float2 *>(d_in) + off;
        a.out = sc16 ? static_cast<void *>(static_cast<uint32_t *>(d_out) + off) : static_cast<void *>(static_cast<float2 *>(d_out) + off);
        a.hist = q->hist[q->cur]; a.pos = q->pos; a.n = m; a.hist_len = q->hist_len;
        const dim3 grid((unsigned)((iq_pairs(q->pos, m) + 255) / 256));
        if (fade) { if (sc16) chanemu_launch<IQ_SC16, true>(a, rot, noise, grid, st); else chanemu_launch<IQ_CF32, true>(a, rot, noise, grid, st); }
        else      { if (sc16) chanemu_launch<IQ_SC16, false>(a, rot, noise, grid, st); else chanemu_launch<IQ_CF32, false>(a, rot, noise, grid, st); }
        MCRX_OP_CHK(g_ce_err, hipGetLastError());
        if (q->D) {
            hipLaunchKernelGGL(chanemu_history_kernel, dim3((q->D + 255) / 256), dim3(256), 0, st, a, q->hist[q->cur ^ 1]);
            MCRX_OP_CHK(g_ce_err, hipGetLastError());
            q->cur ^= 1;
            q->hist_len = (uint32_t)((uint64_t)q->hist_len + m < q->D ? q->hist_len + m : q->D);
        }
        q->pos += m;
        off += m;
    }
    if (sc16) MCRX_OP_CHK(g_ce_err, q->clip.mark(st));
    return MCRX_OK;
}

// the gain kernel on its own, into the caller's buffer: what execute_device computes for itself, for tests and measurements
extern "C" int mcrx_hip_chanfade_gains(mcrx_hip_chanemu_t q, uint64_t first_row, uint32_t rows, void *d_table, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_ce_err = "null handle"; return MCRX_EINVAL; }
    if (!q->fade) { g_ce_err = "fading is off"; return MCRX_EINVAL; }
    if (!d_table || (reinterpret_cast<uintptr_t>(d_table) & 7u)) { g_ce_err = "d_table must be an 8-byte aligned device buffer"; return MCRX_EINVAL; }
    if (rows == 0) return MCRX_OK;
    hipLaunchKernelGGL(chanemu_gain_kernel, dim3((rows + 255) / 256, q->cfg.num_taps), dim3(256), 0, (hipStream_t)stream, q->ft,
                       static_cast<float2 *>(d_table), first_row, rows, q->fade_L);
    MCRX_OP_CHK(g_ce_err, hipGetLastError());
    return MCRX_OK;
}

extern "C" int mcrx_hip_chanemu_clipped(mcrx_hip_chanemu_t q, uint64_t *samples, int reset)
{
    return op_clipped(q, g_ce_err, samples, reset);
}
