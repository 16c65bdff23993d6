// dpd_plan.hpp -- the host arithmetic of the digital predistorter (dpd.hip: mcrx_hip_dpd_*) that needs no
// device: the configuration check, the constants made of a configuration (inv_step, step, e and what follows from e), the bin and the
// eligibility of one (u, z) pair -- the very function the measuring kernel calls --, the bound of the int64 accumulators' guard and the
// measuring launch's grid.  What a table and a streaming launch are it takes from pdtable.hpp.  selftest, create and measure all call it;
// host/dpd_plan_test.cc compiles it with a main of its own.
#pragma once
#include <cmath>
#include <stdint.h>
#include "../../include/mcrx_hip.h"
#include "pdtable.hpp"

#if defined(__HIPCC__)
#define DPD_HD __host__ __device__
#else
#define DPD_HD
#endif

namespace mcrx {

enum { DPD_WG = PD_WG,              // lanes of a workgroup; a lane owns index-aligned sample pairs
       DPD_MAX_WGS = 2048,          // the most workgroups of a measure launch (8 per CU): a lane loops grid * 256 pairs apart
       DPD_MIN_LOG2 = 5, DPD_MAX_LOG2 = 10, DPD_MAX_FORGET = 8,
       DPD_GUARD_LOG2 = 28 };       // at most 2^28 samples offered between two resets (derived below)

// the whole configuration, as create sees it: nullptr or what is wrong
static inline const char *dpd_check(const mcrx_hip_dpd_config *c)
{
    if (c->struct_size != sizeof(mcrx_hip_dpd_config)) return "mcrx_hip_dpd_config: wrong struct_size";
    if (c->table_log2 < (uint32_t)DPD_MIN_LOG2 || c->table_log2 > (uint32_t)DPD_MAX_LOG2) return "table_log2 must be 5 .. 10";
    if (!std::isfinite(c->full_scale) || !(c->full_scale > 0.f)) return "full_scale must be finite and positive";
    const float inv_step = (float)((double)(1u << c->table_log2) / (double)c->full_scale);
    if (!std::isfinite(inv_step) || !(inv_step > 0.f)) return "full_scale: 2^table_log2 / full_scale must be a finite positive fp32";
    if (!std::isfinite(c->target_gain) || !(c->target_gain > 0.f)) return "target_gain must be finite and positive";
    if (c->min_count < 1u) return "min_count must be at least 1";
    if (c->forget_shift > (uint32_t)DPD_MAX_FORGET) return "forget_shift must be 0 .. 8";
    if (!std::isfinite(c->gain)) return "gain must be finite";
    if (c->output_format > 1u) return "output format must be 0 (cf32) or 1 (sc16)";
    return nullptr;
}

// What apply, measure and update use of a (checked) configuration: the table's constants (pd_table_consts) and
//   scale = 2^(32 - 2e): what a product of two amplitudes is multiplied with before it is rounded to an integer (exact in double:
//           e lies in -149 .. 128, so the exponent in -224 .. 330);
//   zmax2 = fp32(16 E^2) = 2^(2e + 4): the largest |z|^2 of an eligible sample; +inf where 2e + 4 > 127 (finiteness is the bound
//           then), 0 where 2e + 4 < -149.
struct DpdConsts : PdTableConsts { float zmax2; double scale; };

static inline DpdConsts dpd_consts(const mcrx_hip_dpd_config *c)
{
    DpdConsts k;
    static_cast<PdTableConsts &>(k) = pd_table_consts(c->table_log2, c->full_scale);
    k.scale = std::ldexp(1.0, 32 - 2 * k.e);
    k.zmax2 = (float)std::ldexp(1.0, 2 * k.e + 4);
    return k;
}

// The bin of one pair and whether it is eligible, in fp32 as the definition writes it (include/mcrx_hip.h): true and *j = the bin, or
// false and *j = -1.  Every comparison is false for a NaN, so a NaN anywhere makes the sample ineligible.  Host and device.
DPD_HD static inline bool dpd_bin(float ur, float ui, float zr, float zi, float inv_step, float Kf, float zmax2, int *j)
{
    const float tu = fmaf(ur, ur, ui * ui), tz = fmaf(zr, zr, zi * zi);
    const float jf = rintf(sqrtf(tu) * inv_step);
    const bool ok = tu < INFINITY && tz < INFINITY && tz <= zmax2 && jf <= Kf;
    *j = ok ? (int)jf : -1;
    return ok;
}

// The three integers an eligible pair adds: fp64 products of fp32 values are exact, the sum of two is rounded once (fma), the scaling by
// a power of two is exact, llrint rounds to nearest even.
DPD_HD static inline void dpd_terms(float ur, float ui, float zr, float zi, double scale, long long *sre, long long *sim, long long *suu)
{
    const double a = ur, b = ui, c = zr, d = zi;
    *sre = (long long)__builtin_rint(__builtin_fma(c, a, d * b) * scale);
    *sim = (long long)__builtin_rint(__builtin_fma(d, a, -(c * b)) * scale);
    *suu = (long long)__builtin_rint(__builtin_fma(a, a, b * b) * scale);
}

// The guard.  An eligible sample has rintf(|u|_32 inv_step) <= K, hence |u|_32 inv_step < K + 1/2 up to one fp32 rounding, with
// inv_step >= (K / full_scale)(1 - 2^-24), |u|_32 >= |u| (1 - 2^-22) and K >= 32:
//     |u| <= full_scale (1 + 1 / (2 K)) (1 + 2^-21) < 1.016 E,        and |z| <= 4 E (1 + 2^-23) from |z|^2_32 <= 16 E^2
// (where 16 E^2 is not an fp32, E >= 2^62 and a finite |z|^2_32 means |z| < 2^64 <= 4 E as well).  So a term is at most
//     |z| |u| 2^32 / E^2 + 1/2 < 4.07 * 2^32 < 2^34.03         (Suu: 1.04 * 2^32)
// in magnitude, and M samples move an accumulator by less than M 2^34.03: M <= 2^28 keeps it below 2^62.03 < 2^63.  The count is a
// 32-bit word in a workgroup's LDS and an int64 on the handle; 2^28 fits both.  Across an update the host's count follows the shift
// (pd_guard_after_update) and stays an upper bound of |a| / 2^34.03.
static inline double dpd_term_bound(uint32_t K) { return 4.0 * 1.0000002 * (1.0 + 0.5 / (double)K) * 1.000001 * 4294967296.0 + 0.5; }

// the workgroups of a measure launch: a workgroup owns a histogram, so the grid is capped and a lane loops over pairs grid * 256 apart
static inline uint32_t dpd_measure_grid(uint64_t parity, uint64_t n)
{
    const uint64_t wgs = (pd_pairs(parity, n) + DPD_WG - 1) / DPD_WG;
    return (uint32_t)(wgs > (uint64_t)DPD_MAX_WGS ? (uint64_t)DPD_MAX_WGS : wgs);
}
// LDS of a measure launch: three 8-byte sums and a 4-byte count per bin
static inline uint32_t dpd_measure_lds(uint32_t K) { return (K + 1u) * 28u; }           // (the sums first: they stay 8-byte aligned)

}  // namespace mcrx
