// interp_table.hpp -- the fractional-delay interpolator, once, for userchan.hip (mcrx_hip_userclock_*: each user's own sample clock) and
// fbalign.hip (mcrx_hip_fbalign_*: the feedback's delay): the table W[65][32] of 64 phases of a Kaiser-windowed sinc plus the row of the
// next whole sample, and the one fused multiply-add that makes a coefficient of two of its rows (include/mcrx_hip.h has the definition).
// The table is made on the host in double; any host compiler (host/fbalign_plan_test.cc compiles it without HIP).
#pragma once
#include <cmath>
#include <stdint.h>
#include <vector>
#include "../../include/mcrx_hip.h"
#include "design.hpp"

#if defined(__HIPCC__)
#define INTERP_HD __host__ __device__ __forceinline__
#else
#define INTERP_HD inline
#endif

namespace mcrx {

static void userclock_make_table(float *W)
{
    const double ib = besseli0(6.0);
    for (int p = 0; p <= MCRX_USERCLOCK_PHASES; p++)
        for (int j = 0; j < MCRX_USERCLOCK_TAPS; j++) {
            const double t = (double)(j - 15) - (double)p / MCRX_USERCLOCK_PHASES;
            const double x = M_PI * t, sn = std::fabs(t) < 1e-12 ? 1.0 : std::sin(x) / x;
            const double r = t / 16.0, w = 1.0 - r * r;
            float v = (float)(sn * besseli0(6.0 * std::sqrt(w < 0.0 ? 0.0 : w)) / ib);
            if (p == 0) v = j == 15 ? 1.f : 0.f;                        // the two ends are whole-sample delays: exact unit vectors
            if (p == MCRX_USERCLOCK_PHASES) v = j == 16 ? 1.f : 0.f;
            W[p * MCRX_USERCLOCK_TAPS + j] = v;
        }
}

static const float *userclock_table()
{
    static const std::vector<float> W = [] { std::vector<float> w((MCRX_USERCLOCK_PHASES + 1) * MCRX_USERCLOCK_TAPS); userclock_make_table(w.data()); return w; }();
    return W.data();
}

// h_j(mu) from the two rows of W around the fraction: the definition's one fused multiply-add, the same on the host and on the device
INTERP_HD float userclock_coef(float w0, float w1, float f) { return fmaf(f, w1 - w0, w0); }

}  // namespace mcrx
