// cfr_plan_test.cc -- the crest-factor reduction's host side without a GPU (tests/test_cfr.py): csrc/cfr_plan.hpp's configuration check
// refuses what include/mcrx_hip.h says create refuses and nothing else of a good configuration; the passes of a call cover, count and
// launch what the header says; the low-pass design is symmetric about nothing it does not own, sums to one and refuses its bad
// arguments.  Built by `make cfr_plan_test`; `make cfr_plan_test SAN=1` builds the same program under the address and
// undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include "../csrc/cfr_plan.hpp"

using namespace mcrx;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_bad <= 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static mcrx_hip_cfr_config good()
{
    mcrx_hip_cfr_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c); c.half_len = 31; c.passes = 2; c.output_format = 1; c.threshold = 0.5f; c.gain = 0.9f;
    const char *bad = cfr_design(c.half_len, 0.28, 5.65, c.taps);
    CHECK(bad == nullptr, "%s", bad);
    return c;
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    mcrx_hip_cfr_config c = good();
    CHECK(sizeof(c) == 284, "%zu", sizeof(c));
    CHECK(cfr_check(&c) == nullptr, "%s", cfr_check(&c));
#define REFUSED(stmt) do { c = good(); stmt; CHECK(cfr_check(&c) != nullptr, "accepted: %s", #stmt); } while (0)
#define ACCEPTED(stmt) do { c = good(); stmt; CHECK(cfr_check(&c) == nullptr, "refused: %s: %s", #stmt, cfr_check(&c)); } while (0)
    REFUSED(c.struct_size -= 4); REFUSED(c.half_len = 0); REFUSED(c.half_len = 65); REFUSED(c.passes = 0); REFUSED(c.passes = 5);
    REFUSED(c.output_format = 2); REFUSED(c.threshold = 0.f); REFUSED(c.threshold = -1.f); REFUSED(c.threshold = nan); REFUSED(c.threshold = inf);
    REFUSED(c.threshold = 1e30f); REFUSED(c.threshold = 1e-30f); REFUSED(c.gain = inf); REFUSED(c.gain = nan);
    REFUSED(c.taps[0] = nan); REFUSED(c.taps[31] = inf); REFUSED(c.taps[7] = -inf);
    ACCEPTED(c.half_len = 1); ACCEPTED(c.half_len = 64); ACCEPTED(c.passes = 1); ACCEPTED(c.passes = 4); ACCEPTED(c.output_format = 0);
    ACCEPTED(c.taps[32] = nan);                                         // behind h[H]: not looked at
    ACCEPTED(c.threshold = 1e-18f); ACCEPTED(c.threshold = 1e18f); ACCEPTED(c.gain = 0.f); ACCEPTED(c.gain = -2.f);
#undef REFUSED
#undef ACCEPTED
    // the passes: pass p writes n + 2 (P - 1 - p) H samples, counts the caller's n of them, and the last pass writes exactly n
    for (uint32_t P = 1; P <= 4; P++)
        for (uint32_t H : { 1u, 7u, 31u, 64u })
            for (uint64_t n : { (uint64_t)1, (uint64_t)2047, (uint64_t)2048, (uint64_t)2049, (uint64_t)207700000 }) {
                c = good(); c.passes = P; c.half_len = H;
                CHECK(cfr_halo(&c) == P * H, "halo");
                uint64_t need = n + 2ull * cfr_halo(&c);                // what the pass reads
                for (uint32_t p = 0; p < P; p++) {
                    const CfrPass ps = cfr_pass(&c, n, p);
                    CHECK(ps.outputs + 2ull * H == need, "P %u H %u p %u: outputs %llu", P, H, p, (unsigned long long)ps.outputs);
                    CHECK(ps.count_hi - ps.count_lo == n && ps.count_lo == (ps.outputs - n) / 2, "P %u H %u p %u: count", P, H, p);
                    CHECK((uint64_t)ps.grid * CFR_RUN >= ps.outputs && (uint64_t)(ps.grid - 1) * CFR_RUN < ps.outputs, "P %u H %u p %u: grid %u", P, H, p, ps.grid);
                    need = ps.outputs;
                }
                CHECK(need == n, "the last pass writes n");
                CHECK(cfr_scratch_samples(&c, n) == (P > 1 ? n + 2ull * (P - 1) * H : 0), "scratch");
            }
    // skipping: allowed as soon as one tap h[0 .. H] is not negative; taps behind h[H] do not count
    c = good(); CHECK(cfr_may_skip(&c), "the default low-pass");
    for (uint32_t k = 0; k <= c.half_len; k++) c.taps[k] = -0.01f;
    c.taps[40] = 1.f; CHECK(!cfr_may_skip(&c), "every tap negative");
    c.taps[31] = 0.f; CHECK(cfr_may_skip(&c), "+0 counts as not negative");
    c.taps[31] = -0.f; CHECK(!cfr_may_skip(&c), "-0 is negative");
    c.taps[0] = 1e-30f; CHECK(cfr_may_skip(&c), "one positive tap");
    // the size guard: n + 2 halo <= 2^32
    c = good(); c.passes = 4; c.half_len = 64;
    const uint64_t most = (uint64_t)1 << 32;
    CHECK(cfr_fits(&c, most - 512) && !cfr_fits(&c, most - 511) && !cfr_fits(&c, most) && !cfr_fits(&c, ~(uint64_t)0), "fits");
    CHECK(cfr_pass(&c, most - 512, 0).grid == (uint32_t)((most - 128 + CFR_RUN - 1) / CFR_RUN), "grid of the largest call");
    CHECK(cfr_threshold2(1.5f) == 2.25f && cfr_threshold2(0.1f) == (float)((double)0.1f * (double)0.1f), "A2");
    // the design
    float h[MCRX_CFR_MAX_HALF_LEN + 2];
    for (uint32_t H = 1; H <= 64; H++)
        for (double fc : { 0.01, 0.25, 0.28, 0.49 })
            for (double beta : { 0.0, 5.65, 12.0 }) {
                for (float &v : h) v = 77.f;
                const char *bad = cfr_design(H, fc, beta, h);
                CHECK(bad == nullptr, "H %u fc %g beta %g: %s", H, fc, beta, bad);
                double sum = h[0];
                for (uint32_t k = 1; k <= H; k++) sum += 2.0 * h[k];
                CHECK(std::fabs(sum - 1.0) < 1e-6, "H %u fc %g beta %g: sum %.9f", H, fc, beta, sum);
                CHECK(h[H + 1] == 77.f, "H %u: wrote behind h[H]", H);
                CHECK(h[0] > 0.f && std::fabs(h[0]) >= std::fabs(h[H]), "H %u fc %g beta %g: shape", H, fc, beta);
            }
    CHECK(cfr_design(0, 0.28, 5.65, h) && cfr_design(65, 0.28, 5.65, h) && cfr_design(31, 0.0, 5.65, h) && cfr_design(31, 0.5, 5.65, h), "bounds");
    CHECK(cfr_design(31, -0.1, 5.65, h) && cfr_design(31, 0.28, -1.0, h) && cfr_design(31, (double)nan, 5.65, h) && cfr_design(31, 0.28, (double)inf, h), "values");
    CHECK(cfr_design(31, 0.28, 5.65, nullptr) != nullptr, "null");
    if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
    printf("cfr_plan_test ok\n");
    return 0;
}
