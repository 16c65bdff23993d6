// mpd_plan.hpp -- the arithmetic of the memory-polynomial predistorter (mpd.hip: mcrx_hip_mpd_*) that needs no
// device: the configuration check, the constants made of a configuration, the integers one feedback sample and one amplifier-input
// sample turn into -- the very functions the measuring kernel calls --, the bound of the int64 sums' guard, the grids and the LDS sizes.
// What a table and a streaming launch are it takes from pdtable.hpp.  selftest, create and measure all call it; host/mpd_plan_test.cc compiles it with a main of its own.
#pragma once
#include <cmath>
#include <stdint.h>
#include "../../include/mcrx_hip.h"
#include "dpd_plan.hpp"

#if defined(__HIPCC__)
#define MPD_HD __host__ __device__
#else
#define MPD_HD
#endif

namespace mcrx {

enum { MPD_WG = PD_WG,               // lanes of a workgroup
       MPD_TILE = 256,              // rows a measuring workgroup stages at a time
       MPD_MAX_WGS = 1024,          // the most workgroups of a measure launch (4 per CU): a workgroup loops over tiles grid apart
       MPD_MAX_BRANCHES = 4, MPD_MAX_DELAY = 16, MPD_MAX_ORDER = 5, MPD_MAX_COEFFS = 20,
       MPD_MAX_ENTRIES = 2048,      // M * 2^table_log2 at most: 32 KB of quadruples in LDS
       MPD_MAX_SUMS = 231,          // (L + 1)(L + 2) / 2 at L = 20: at most one Gram entry a lane
       MPD_QB = 17,                 // fractional bits of the regressors' integers
       MPD_MIN_RIDGE = 10, MPD_MAX_RIDGE = 40, MPD_MAX_FORGET = 8,
       MPD_GUARD_LOG2 = 26 };       // at most 2^26 rows offered between two resets (derived below)

// the whole configuration, as create sees it: nullptr or what is wrong
static inline const char *mpd_check(const mcrx_hip_mpd_config *c)
{
    if (c->struct_size != sizeof(mcrx_hip_mpd_config)) return "mcrx_hip_mpd_config: wrong struct_size";
    if (c->branches < 1u || c->branches > (uint32_t)MPD_MAX_BRANCHES) return "branches must be 1 .. 4";
    if (c->delay[0] != 0u) return "delay[0] must be 0";
    for (uint32_t m = 1; m < c->branches; m++)
        if (c->delay[m] <= c->delay[m - 1] || c->delay[m] > (uint32_t)MPD_MAX_DELAY) return "delays must increase strictly and be at most 16";
    if (c->order < 1u || c->order > (uint32_t)MPD_MAX_ORDER) return "order must be 1 .. 5";
    if (c->table_log2 < (uint32_t)DPD_MIN_LOG2 || c->table_log2 > (uint32_t)DPD_MAX_LOG2) return "table_log2 must be 5 .. 10";
    if ((c->branches << c->table_log2) > (uint32_t)MPD_MAX_ENTRIES) return "branches * 2^table_log2 must be at most 2048";
    if (!std::isfinite(c->full_scale) || !(c->full_scale > 0.f)) return "full_scale must be finite and positive";
    const float inv_step = (float)((double)(1u << c->table_log2) / (double)c->full_scale);
    if (!std::isfinite(inv_step) || !(inv_step > 0.f)) return "full_scale: 2^table_log2 / full_scale must be a finite positive fp32";
    if (!std::isfinite(c->target_gain) || !(c->target_gain > 0.f)) return "target_gain must be finite and positive";
    const float inv_g0 = (float)(1.0 / (double)c->target_gain);
    if (!std::isfinite(inv_g0) || !(inv_g0 > 0.f)) return "target_gain: 1 / target_gain must be a finite positive fp32";
    if (c->min_rows < c->branches * c->order) return "min_rows must be at least branches * order";
    if (c->ridge_log2 < (uint32_t)MPD_MIN_RIDGE || c->ridge_log2 > (uint32_t)MPD_MAX_RIDGE) return "ridge_log2 must be 10 .. 40";
    if (c->forget_shift > (uint32_t)MPD_MAX_FORGET) return "forget_shift must be 0 .. 8";
    if (!std::isfinite(c->gain)) return "gain must be finite";
    if (c->output_format > 1u) return "output format must be 0 (cf32) or 1 (sc16)";
    return nullptr;
}

// What apply, measure and update use of a (checked) configuration: the table's constants (pd_table_consts);
// inv_g0 = fp32(1 / g0), the quotient made in double; M, P, L = M P, the delays and lead = delay[M - 1]; sums = (L + 1)(L + 2) / 2.
struct MpdConsts : PdTableConsts { uint32_t M, P, L, lead, sums, delay[MPD_MAX_BRANCHES]; float inv_g0; };

static inline MpdConsts mpd_consts(const mcrx_hip_mpd_config *c)
{
    MpdConsts k = {};
    static_cast<PdTableConsts &>(k) = pd_table_consts(c->table_log2, c->full_scale);
    k.inv_g0 = (float)(1.0 / (double)c->target_gain);
    k.M = c->branches; k.P = c->order; k.L = k.M * k.P; k.sums = (k.L + 1u) * (k.L + 2u) / 2u;
    for (uint32_t m = 0; m < k.M; m++) k.delay[m] = c->delay[m];
    k.lead = k.delay[k.M - 1u];
    return k;
}

// One feedback sample z, in fp32 as the definition writes it (include/mcrx_hip.h): its P regressors as integer pairs, and whether it
// is eligible (t finite and <= 1: every comparison is false for a NaN).  An ineligible sample gives zeros.  Host and device; the loop is
// over all five powers so that a kernel keeps them in registers.
MPD_HD static inline bool mpd_basis(float zr, float zi, float inv_g0, int e, uint32_t P, int32_t *bre, int32_t *bim)
{
    const float wr = zr * inv_g0, wi = zi * inv_g0;
    float pr = ldexpf(wr, -e), pi = ldexpf(wi, -e);                     // zeta = w / E
    const float t = fmaf(pr, pr, pi * pi), a = sqrtf(t);
    const bool ok = t <= 1.0f;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < (uint32_t)MPD_MAX_ORDER; k++) {
        const bool use = ok && k < P;
        bre[k] = use ? (int32_t)__builtin_rintf(pr * 131072.0f) : 0;    // (|phi| <= 1: the product is exact, the integer below 2^17.001)
        bim[k] = use ? (int32_t)__builtin_rintf(pi * 131072.0f) : 0;
        pr = pr * a; pi = pi * a;
    }
    return ok;
}

// One amplifier-input sample u: U = llrint(u / E * 2^17) per component, eligible when |u / E|^2 (formed the same way) is <= 4
MPD_HD static inline bool mpd_target(float ur, float ui, int e, int32_t *Ure, int32_t *Uim)
{
    const float pr = ldexpf(ur, -e), pi = ldexpf(ui, -e);
    const float t = fmaf(pr, pr, pi * pi);
    const bool ok = t <= 4.0f;
    *Ure = ok ? (int32_t)__builtin_rintf(pr * 131072.0f) : 0;
    *Uim = ok ? (int32_t)__builtin_rintf(pi * 131072.0f) : 0;
    return ok;
}

// The guard.  An eligible feedback sample has t = fl(zeta.re^2 + zeta.im^2) <= 1 with two roundings, so |zeta| <= 1 + 2^-23; a =
// fl(sqrt(t)) <= 1, so no power is larger than the one before it: |phi_k| <= |zeta|.  B = rint(2^17 phi) moves a component by at most
// 1/2: |B_l| <= 2^17 (1 + 2^-23) + 0.71 < 2^17.001.  Likewise |u / E| <= 2 (1 + 2^-23) and |U| < 2^18.001.  By Cauchy-Schwarz the real
// and the imaginary part of conj(V_p) V_q are at most |V_p| |V_q| in magnitude:
//     A_pq: 2^34.01        b_l: 2^35.01        Suu: 2^36.01
// Each is one or two products of int32 values summed in an int64, exactly.  R rows move a sum by less than R 2^36.01: R <= 2^26 keeps
// every sum below 2^62.01 < 2^63, in a lane's register, in a workgroup's flush and on the handle.  Across an update the host's count
// follows the shift (pd_guard_after_update) and stays an upper bound of |a| / 2^36.01.
static inline double mpd_term_bound() { const double U = 262144.0 * (1.0 + 1.2e-7) + 0.71; return U * U; }

// rows of a measure call on n samples; its tiles of 256 rows; its workgroups (capped: a workgroup takes tiles grid apart)
static inline uint64_t mpd_rows(uint64_t n, uint32_t lead) { return n > lead ? n - lead : 0; }
static inline uint64_t mpd_tiles(uint64_t rows) { return (rows + MPD_TILE - 1) / MPD_TILE; }
static inline uint32_t mpd_measure_grid(uint64_t rows)
{
    const uint64_t t = mpd_tiles(rows);
    return (uint32_t)(t > (uint64_t)MPD_MAX_WGS ? (uint64_t)MPD_MAX_WGS : t);
}
// rounds of 256 pairs an apply workgroup takes: pd_rounds' rule on all M tables (their 16 M K bytes are 1/16 of what the rounds stream)
static inline uint32_t mpd_rounds(uint32_t M, uint32_t K) { return pd_rounds(M * K); }
// LDS of an apply launch: M K quadruples, and with M > 1 the round's window of 512 + lead staged samples, 16 bytes each
static inline uint32_t mpd_apply_lds(uint32_t M, uint32_t K, uint32_t lead) { return pd_stream_lds(M * K) + (M > 1u ? (2u * MPD_WG + lead) * 16u : 0u); }
// LDS of a measure launch: (256 + lead) samples' P regressors and 256 targets, 8 bytes each; (256 + lead) + 256 flags
static inline uint32_t mpd_measure_lds(uint32_t P, uint32_t lead) { return ((MPD_TILE + lead) * P + MPD_TILE) * 8u + (2u * MPD_TILE + lead) * 4u; }

}  // namespace mcrx
