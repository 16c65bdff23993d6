// rfcal_plan_test.cc -- the receiver calibration's host arithmetic without a GPU (tests/test_rfcal.py): csrc/rfcal_plan.hpp's
// configuration check refuses what include/mcrx_hip.h says create refuses and nothing else, the split of a call covers it exactly with
// every cut on a block boundary of the absolute index (at 0, at odd positions, at 2^40 and across 2^64), the grid is a capped function
// of (pos, n), mu_j is the cumulative mean down to its floor, and the 2^31 guard holds at its edge.  Built by `make rfcal_plan_test`;
// `make rfcal_plan_test SAN=1` builds the same program under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include "../csrc/rfcal_plan.hpp"

using namespace mcrx;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_bad <= 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static mcrx_hip_rfcal_config good()
{
    mcrx_hip_rfcal_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c); c.stages = MCRX_RFCAL_DC | MCRX_RFCAL_IQ; c.input_format = 1; c.output_format = 1;
    c.period_log2 = 14; c.forget_log2 = 3; c.gain = 1.f;
    return c;
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    mcrx_hip_rfcal_config c = good();
    CHECK(rfcal_check(&c) == nullptr, "%s", rfcal_check(&c));
#define REFUSED(stmt) do { c = good(); stmt; CHECK(rfcal_check(&c) != nullptr, "accepted: %s", #stmt); } while (0)
#define ACCEPTED(stmt) do { c = good(); stmt; CHECK(rfcal_check(&c) == nullptr, "refused: %s", #stmt); } while (0)
    REFUSED(c.struct_size -= 4); REFUSED(c.stages = 4); REFUSED(c.input_format = 2); REFUSED(c.output_format = 2);
    REFUSED(c.period_log2 = 1); REFUSED(c.period_log2 = 5); REFUSED(c.period_log2 = 31); REFUSED(c.forget_log2 = 31);
    REFUSED(c.gain = inf); REFUSED(c.gain = nan);
    ACCEPTED(c.stages = 0); ACCEPTED(c.period_log2 = 0); ACCEPTED(c.period_log2 = 6); ACCEPTED(c.period_log2 = 30);
    ACCEPTED(c.forget_log2 = 0); ACCEPTED(c.forget_log2 = 30); ACCEPTED(c.gain = 0.f); ACCEPTED(c.input_format = 0);
#undef REFUSED
#undef ACCEPTED
    // the split: covers the call, cuts only at block boundaries, the count agrees with rfcal_segments
    const uint64_t positions[] = { 0, 1, 63, 64, 12345, (1ull << 40) - 3, (1ull << 40) + 1, ~0ull - 100, ~0ull, (1ull << 63) + 7 };
    const uint64_t sizes[] = { 1, 2, 63, 64, 65, 257, 4097, 100000 };
    const uint32_t periods[] = { 0, 6, 10, 30 };
    for (uint64_t pos : positions)
        for (uint64_t n : sizes)
            for (uint32_t k : periods) {
                uint64_t p = pos, left = n, segs = 0;
                while (left) {
                    bool ends = false;
                    const uint64_t m = rfcal_segment(p, left, k, &ends);
                    CHECK(m >= 1 && m <= left, "pos %llu n %llu k %u: segment %llu", (unsigned long long)pos, (unsigned long long)n, k, (unsigned long long)m);
                    if (m < 1 || m > left) break;
                    if (k) {
                        const uint64_t B = 1ull << k;
                        CHECK(ends == (((p + m) & (B - 1)) == 0), "pos %llu n %llu k %u: a segment ends a block exactly on a boundary", (unsigned long long)pos, (unsigned long long)n, k);
                        CHECK((p & ~(B - 1)) == ((p + m - 1) & ~(B - 1)), "pos %llu n %llu k %u: a segment straddles a boundary", (unsigned long long)pos, (unsigned long long)n, k);
                        CHECK(ends || m == left, "only the last segment may stop short of a boundary");
                    } else CHECK(!ends && m == n, "manual handles have one segment");
                    p += m; left -= m; segs++;
                }
                CHECK(segs == rfcal_segments(pos, n, k), "pos %llu n %llu k %u: %llu segments, rfcal_segments %llu", (unsigned long long)pos, (unsigned long long)n, k,
                      (unsigned long long)segs, (unsigned long long)rfcal_segments(pos, n, k));
            }
    CHECK(rfcal_segments(5, 0, 10) == 0, "an empty call has no segment");
    CHECK(rfcal_segments(0, 1ull << 32, 6) == 1ull << 26, "2^32 samples in blocks of 64");
    const uint64_t launch_sizes[] = { 1, 2, 511, 512, 513, 1048576, 1048577, 1ull << 32 };
    // the grid: every pair has a lane when the launch does not measure; capped when it does; a function of (pos, n)
    for (uint64_t pos : positions)
        for (uint64_t n : launch_sizes) {
            const uint64_t pairs = rfcal_pairs(pos, n);
            CHECK(pairs == (n + (pos & 1) + 1) / 2, "pairs");
            const uint32_t g0 = rfcal_grid(pos, n, false), g1 = rfcal_grid(pos, n, true);
            CHECK((uint64_t)g0 * RFCAL_WG >= pairs && (uint64_t)(g0 - 1) * RFCAL_WG < pairs, "pos %llu n %llu: grid %u", (unsigned long long)pos, (unsigned long long)n, g0);
            CHECK(g1 == (g0 < (uint32_t)RFCAL_MAX_ROWS ? g0 : (uint32_t)RFCAL_MAX_ROWS) && g1 >= 1, "pos %llu n %llu: measuring grid %u", (unsigned long long)pos, (unsigned long long)n, g1);
        }
    // mu_j
    CHECK(rfcal_mu(0, 30) == 1.0 && rfcal_mu(1, 30) == 0.5 && rfcal_mu(2, 30) == 1.0 / 3.0, "the cumulative mean");
    CHECK(rfcal_mu(6, 3) == 1.0 / 7.0 && rfcal_mu(7, 3) == 0.125 && rfcal_mu(8, 3) == 0.125 && rfcal_mu(1ull << 40, 3) == 0.125, "the floor 2^-3");
    CHECK(rfcal_mu(0, 0) == 1.0 && rfcal_mu(5, 0) == 1.0, "forget_log2 = 0: every block replaces the means");
    CHECK(rfcal_mu(~0ull, 30) == std::ldexp(1.0, -30), "the floor 2^-30");
    // the guard
    CHECK(rfcal_guard_ok(0, 1ull << 31) && !rfcal_guard_ok(0, (1ull << 31) + 1), "2^31 itself is allowed");
    CHECK(rfcal_guard_ok((1ull << 31) - 5, 5) && !rfcal_guard_ok((1ull << 31) - 5, 6) && !rfcal_guard_ok(1ull << 31, 1) && rfcal_guard_ok(1ull << 31, 0), "the count since the last update");
    CHECK(!rfcal_guard_ok(~0ull, 1) && !rfcal_guard_ok(1, ~0ull), "no wrap");
    if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
    printf("rfcal_plan_test ok\n");
    return 0;
}
