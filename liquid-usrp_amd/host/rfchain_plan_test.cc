// rfchain_plan_test.cc -- the RF front end's host side without a GPU (tests/test_rfchain.py): csrc/rfchain_plan.hpp's configuration
// check refuses what include/mcrx_hip.h says create refuses and nothing else of a good configuration, and the oscillator's integers
// keep |f_k| B <= 1/8 for extreme bandwidths and every block size.  Built by `make rfchain_plan_test`; `make rfchain_plan_test
// SAN=1` builds the same program under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include "../csrc/rfchain_plan.hpp"

using namespace mcrx;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_bad <= 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static mcrx_hip_rfchain_config good()
{
    mcrx_hip_rfchain_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c); c.order = 1; c.stages = 7; c.input_format = 1; c.output_format = 1;
    c.alpha_re = 1.f; c.beta_im = 0.05f; c.dc_re = 0.01f;
    c.pn_sinusoids = 16; c.pn_log2_block = 10; c.pn_table_rows = 0; c.pn_rms = 0.02f; c.pn_bandwidth = 1e-5; c.pn_seed = 0xC0FFEE0123456789ull;
    c.amp_sat = 0.5f; c.amp_gain = 1.f; c.amp_ampm = 0.01f; c.amp_smooth = 2;
    c.gain = 1.f;
    return c;
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    mcrx_hip_rfchain_config c = good();
    CHECK(rfchain_check(&c) == nullptr, "%s", rfchain_check(&c));
#define REFUSED(stmt) do { c = good(); stmt; CHECK(rfchain_check(&c) != nullptr, "accepted: %s", #stmt); } while (0)
    REFUSED(c.struct_size -= 4); REFUSED(c.order = 2); REFUSED(c.stages = 8); REFUSED(c.input_format = 2); REFUSED(c.output_format = 2);
    REFUSED(c.gain = inf); REFUSED(c.alpha_im = nan); REFUSED(c.dc_im = inf);
    REFUSED(c.pn_sinusoids = 0); REFUSED(c.pn_sinusoids = 17); REFUSED(c.pn_log2_block = 0); REFUSED(c.pn_log2_block = 25);
    REFUSED(c.pn_table_rows = 1); REFUSED(c.pn_rms = -0.1f); REFUSED(c.pn_rms = nan); REFUSED(c.pn_bandwidth = -1e-6);
    REFUSED(c.pn_bandwidth = (double)inf); REFUSED(c.pn_bandwidth = 0.126 / 1024.0); REFUSED(c.pn_rms = 0.28f);      // 0.28 sqrt(32) = 1.58 > pi / 2
    REFUSED(c.amp_smooth = 3); REFUSED(c.amp_smooth = 0); REFUSED(c.amp_sat = 0.f); REFUSED(c.amp_sat = -1.f); REFUSED(c.amp_sat = nan);
    REFUSED(c.amp_sat = 1e30f); REFUSED(c.amp_sat = 1e-30f); REFUSED(c.amp_gain = inf); REFUSED(c.amp_ampm = 0.3f); REFUSED(c.amp_ampm = nan);
#undef REFUSED
    // a stage that is off is not looked at
    c = good(); c.stages = 0; c.pn_sinusoids = 99; c.amp_smooth = 3; c.alpha_re = nan;
    CHECK(rfchain_check(&c) == nullptr, "%s", rfchain_check(&c));
    CHECK(rfchain_osc_check(&c) != nullptr, "the selftest's check looks at the oscillator anyway");
    // the integers: every |f_k| B <= 1/8, at the widest line every block size takes and at a narrow one; c = rms sqrt(2 / S) / (2 pi)
    for (uint32_t L = 1; L <= 24; L++)
        for (uint32_t S = 1; S <= 16; S++)
            for (int wide = 0; wide < 2; wide++) {
                c = good(); c.pn_log2_block = L; c.pn_sinusoids = S; c.pn_bandwidth = wide ? 0.125 / (double)(1u << L) : 1e-9; c.pn_seed = 77u * L + S;
                c.pn_rms = 0.2f / std::sqrt((float)S);
                CHECK(rfchain_check(&c) == nullptr, "L %u S %u: %s", L, S, rfchain_check(&c));
                int64_t steps[MCRX_RFCHAIN_MAX_SINUSOIDS]; uint32_t phases[MCRX_RFCHAIN_MAX_SINUSOIDS]; float coef = -1.f;
                rfchain_phase_integers(&c, steps, phases, &coef);
                const int64_t most = (int64_t)1 << (61 - L);        // 2^64 / (8 B)
                int clamped = 0;
                for (uint32_t k = 0; k < S; k++) {
                    CHECK(steps[k] >= -most && steps[k] <= most, "L %u S %u k %u: step %lld", L, S, k, (long long)steps[k]);
                    clamped += steps[k] == most || steps[k] == -most;
                }
                if (wide && S >= 8) CHECK(clamped >= 2, "L %u S %u: the widest line must reach the clamp", L, S);
                const double want = (double)c.pn_rms * std::sqrt(2.0 / S) / 6.283185307179586;
                CHECK(std::fabs((double)coef - want) <= 6e-8 * want, "L %u S %u: c %g, want %g", L, S, (double)coef, want);
            }
    if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
    printf("rfchain_plan_test ok\n");
    return 0;
}
