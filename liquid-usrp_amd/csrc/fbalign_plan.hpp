// fbalign_plan.hpp -- the arithmetic of the feedback aligner (fbalign.hip: mcrx_hip_fbalign_*) that needs no
// device: the configuration check, the constants made of a configuration (e, R, halo, the differentiator's taps), the quantiser of one
// component -- the very function the measuring kernel calls --, the split of a delay into whole samples, table row and fraction and the
// 32 coefficients that follow, the bound of the int64 sums' guard, the grids and the layout of the sums.  selftest, create, set and
// measure all call it; host/fbalign_plan_test.cc compiles it with a main of its own.
#pragma once
#include <cmath>
#include <stdint.h>
#include "../../include/mcrx_hip.h"
#include "interp_table.hpp"
#include "pd_plan.hpp"

#if defined(__HIPCC__)
#define FBA_HD __host__ __device__
#else
#define FBA_HD
#endif

namespace mcrx {

enum { FBA_WG = 256,                // lanes of a workgroup
       FBA_TILE = 256,              // rows a measuring workgroup stages at a time
       FBA_MAX_WGS = 256,           // the most workgroups of a measure launch (1 per CU): a workgroup loops over tiles grid apart
       FBA_MIN_LAG = 8, FBA_MAX_LAG = 64,
       FBA_H = 8,                   // half length of the differentiator
       FBA_MAX_R = FBA_MAX_LAG + FBA_H,
       FBA_TAPS = MCRX_USERCLOCK_TAPS,
       FBA_WIN = 2 * FBA_WG + FBA_TAPS + 2,     // samples an applying workgroup stages: 512 outputs' windows, rounded up to a pair
       FBA_GUARD_LOG2 = 31 };       // at most 2^31 rows offered between two updates or resets (derived below)
static_assert((int)FBA_WG == (int)PD_WG, "fbalign_apply_grid counts pd_plan.hpp's workgroups of 256 pairs");

// the whole configuration, as create sees it: nullptr or what is wrong
static inline const char *fbalign_check(const mcrx_hip_fbalign_config *c)
{
    if (c->struct_size != sizeof(mcrx_hip_fbalign_config)) return "mcrx_hip_fbalign_config: wrong struct_size";
    if (c->max_lag < (uint32_t)FBA_MIN_LAG || c->max_lag > (uint32_t)FBA_MAX_LAG) return "max_lag must be 8 .. 64";
    if (!std::isfinite(c->full_scale) || !(c->full_scale > 0.f)) return "full_scale must be finite and positive";
    if (!std::isfinite(c->target_gain) || !(c->target_gain > 0.f)) return "target_gain must be finite and positive";
    if (c->min_rows < 1u) return "min_rows must be at least 1";
    if (c->input_format > 1u) return "input format must be 0 (cf32) or 1 (sc16)";
    return nullptr;
}

// What apply, measure and update use of a (checked) configuration: Lm, R = Lm + H, halo = Lm + 17, sums = 2 R + 1 + 2 H + 1 + 1 complex
// entries (C, A, Szz); e as dpd makes it (pd_table_consts); the taps h_1 .. h_8 of the differentiator, made in double, rounded to fp32.
struct FbalignConsts { uint32_t Lm, R, halo, sums; int e; float h[FBA_H]; };

static inline FbalignConsts fbalign_consts(const mcrx_hip_fbalign_config *c)
{
    FbalignConsts k = {};
    k.Lm = c->max_lag; k.R = k.Lm + (uint32_t)FBA_H; k.halo = k.Lm + 17u; k.sums = 2u * k.R + 1u + 2u * (uint32_t)FBA_H + 1u + 1u;
    k.e = pd_table_consts(5u, c->full_scale).e;
    for (int i = 1; i <= FBA_H; i++)
        k.h[i - 1] = (float)(((i & 1) ? -1.0 : 1.0) / (double)i * (0.54 + 0.46 * std::cos(M_PI * (double)i / 9.0)));
    return k;
}

// Q15 of one component: clamp(llrint(ldexpf(v, 15 - e)), -32768, 32767), ties to even; a NaN gives 0.  *bad is set where the value
// clamps or is not finite (and left alone otherwise).  rintf of an fp32 is the integer llrint would give.  Host and device.
FBA_HD static inline int32_t fbalign_q15(float v, int e, bool *bad)
{
    const float s = ldexpf(v, 15 - e);
    if (s != s) { *bad = true; return 0; }
    const float r = __builtin_rintf(s);
    if (r > 32767.0f) { *bad = true; return 32767; }
    if (r < -32768.0f) { *bad = true; return -32768; }
    return (int32_t)r;
}
// a sample as the measuring kernel keeps it in LDS: int16 re in the low half, im in the high half
FBA_HD static inline uint32_t fbalign_word(float re, float im, int e, bool *bad)
{
    const int32_t a = fbalign_q15(re, e, bad), b = fbalign_q15(im, e, bad);
    return ((uint32_t)a & 0xffffu) | ((uint32_t)b << 16);
}

// The delay as apply uses it: d = -tau_fp; nd = d >> 32 (floor); mu = the low word; r = mu >> 26; f = ((mu >> 2) & 0xffffff) 2^-24
struct FbalignSplit { int32_t nd; uint32_t r; float f; };
FBA_HD static inline FbalignSplit fbalign_split(int64_t tau_fp)
{
    const int64_t d = -tau_fp;
    const uint32_t mu = (uint32_t)(uint64_t)d;
    FbalignSplit s;
    s.nd = (int32_t)(d >> 32); s.r = mu >> 26; s.f = (float)((mu >> 2) & 0xffffffu) * 0x1p-24f;
    return s;
}
// |tau_fp| <= (Lm + 1) 2^32: every tap of every output lies inside the n + 2 halo samples of a call
FBA_HD static inline bool fbalign_tau_ok(int64_t tau_fp, uint32_t Lm)
{
    const int64_t most = (int64_t)(Lm + 1u) << 32;
    return tau_fp >= -most && tau_fp <= most;
}
// the 32 coefficients of a delay from the table W[65][32]
FBA_HD static inline void fbalign_coefs(const float *W, int64_t tau_fp, float *c)
{
    const FbalignSplit s = fbalign_split(tau_fp);
    const float *w0 = W + s.r * (uint32_t)FBA_TAPS, *w1 = w0 + FBA_TAPS;
    for (int j = 0; j < FBA_TAPS; j++) c[j] = userclock_coef(w0[j], w1[j], s.f);
}

// The guard.  A quantised component lies in -32768 .. 32767, so the real and the imaginary part of conj(X) Y are two products of at
// most 2^30 each: a term is at most 2^31 in magnitude.  N rows move a sum by at most N 2^31: N <= 2^31 keeps every sum within 2^62 <
// 2^63, in a lane's register, in a workgroup's flush and on the handle.  An update clears the sums, and the host's count with them.
static inline double fbalign_term_bound() { return 2.0 * 32768.0 * 32768.0; }
static inline bool fbalign_guard_ok(uint64_t since, uint64_t rows) { return pd_guard_ok(since, rows, FBA_GUARD_LOG2); }

// rows of a measure call on n samples: i = R .. n - R - 1; its tiles of 256 rows; its workgroups (capped: a workgroup takes tiles grid apart)
static inline uint64_t fbalign_rows(uint64_t n, uint32_t R) { return n > 2ull * R ? n - 2ull * R : 0; }
static inline uint64_t fbalign_tiles(uint64_t rows) { return (rows + FBA_TILE - 1) / FBA_TILE; }
static inline uint32_t fbalign_measure_grid(uint64_t rows)
{
    const uint64_t t = fbalign_tiles(rows);
    return (uint32_t)(t > (uint64_t)FBA_MAX_WGS ? (uint64_t)FBA_MAX_WGS : t);
}
// the workgroups of an apply launch: 256 index-aligned pairs each
static inline uint32_t fbalign_apply_grid(uint64_t parity, uint64_t n) { return pd_stream_grid(parity, n, 1u); }

}  // namespace mcrx
