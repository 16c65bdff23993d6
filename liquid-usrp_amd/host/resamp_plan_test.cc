// resamp_plan_test.cc -- the resampler's host side without a GPU (tests/test_resamp_model.py): csrc/resamp_plan.hpp's rate check refuses
// what include/mcrx_hip.h says create refuses and nothing else; the decomposition, the step and its period at the rate edges; the
// 64-bit terms of msresamp.hip at the deepest chain the check lets through; the delay; the taps' symmetry and DC gains.  Built by
// `make resamp_plan_test`; `make resamp_plan_test SAN=1` builds the same program under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include "../csrc/resamp_plan.hpp"

using namespace mcrx;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_bad <= 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static void check_plan(float rate)
{
    CHECK(resamp_rate_check(rate) == nullptr, "rate %g refused: %s", (double)rate, resamp_rate_check(rate));
    const ResampPlan p = resamp_plan(rate, 60.0f);
    const double want = p.interp ? (double)rate / std::ldexp(1.0, (int)p.num_stages) : (double)rate * std::ldexp(1.0, (int)p.num_stages);
    CHECK(p.interp == (rate > 1.0f), "rate %g: interp", (double)rate);
    CHECK(p.rate_arb == want, "rate %g: rate_arb %.17g", (double)rate, p.rate_arb);
    if (p.interp) CHECK(p.rate_arb > 1.0 && p.rate_arb <= 2.0, "rate %g: rate_arb %.17g", (double)rate, p.rate_arb);
    else CHECK(p.rate_arb >= 0.5 && p.rate_arb <= 1.0, "rate %g: rate_arb %.17g", (double)rate, p.rate_arb);
    CHECK(p.num_stages <= (unsigned)RSP_MAX_STAGES, "rate %g: %u stages", (double)rate, p.num_stages);
    CHECK(p.step >= (1ull << 23) && p.step <= (1ull << 25), "rate %g: step %llu", (double)rate, p.step);
    CHECK(std::fabs((double)p.step * p.rate_arb - 16777216.0) <= 0.5 * p.rate_arb + 1e-6, "rate %g: step %llu", (double)rate, p.step);
    // the period: whole, coprime apart from what 2^24 and step share, and per_in / per_out = step / 2^24 exactly
    CHECK(p.per_in >= 1 && p.per_out >= 1 && p.per_out <= (1ll << 24) && p.per_in < (1ll << 25), "rate %g: period %lld %lld", (double)rate, p.per_in, p.per_out);
    CHECK((unsigned long long)p.per_in << 24 == (unsigned long long)p.per_out * p.step, "rate %g: per_in 2^24 != per_out step", (double)rate);
    CHECK((p.per_in & 1) || (p.per_out & 1), "rate %g: the period is not the smallest", (double)rate);
    // the 64-bit terms of msresamp.hip (resamp_plan.hpp, at RSP_MAX_STAGES): the first stage's period, and a reset position's r << ns
    if (!p.interp) {
        const long long period0 = p.per_in << p.num_stages;
        CHECK(period0 > 0 && period0 >> p.num_stages == p.per_in, "rate %g: per_in << ns", (double)rate);
        CHECK(period0 <= (1ll << 62), "rate %g: the first stage's period leaves no room for a call", (double)rate);
    }
    CHECK(p.h1.size() == (size_t)RSP_TAPS && p.hpfb.size() == (size_t)RSP_NPFB * RSP_TAPS, "rate %g: sizes", (double)rate);
    // the delay
    if (!p.interp) {
        double d = 7.0;
        for (unsigned i = 0; i < p.num_stages; i++) d = 2.0 * d + 13.0;
        CHECK(p.delay == (float)d, "rate %g: delay %g", (double)rate, (double)p.delay);
    } else {
        const double d = 7.0 + (7.0 / p.rate_arb) * (2.0 - std::ldexp(1.0, 1 - (int)p.num_stages));
        CHECK(std::fabs((double)p.delay - d) <= 1e-5, "rate %g: delay %g, not %g", (double)rate, (double)p.delay, d);
        CHECK(p.delay >= 7.0f && p.delay < 21.0f, "rate %g: delay %g", (double)rate, (double)p.delay);
    }
    // taps: the half-band branch is symmetric and sums to 1 within 2e-3; every branch of the table sums to 1 within 1e-3
    double s1 = 0;
    for (unsigned i = 0; i < (unsigned)RSP_TAPS; i++) { s1 += p.h1[i]; CHECK(p.h1[i] == p.h1[RSP_TAPS - 1 - i], "rate %g: h1[%u]", (double)rate, i); }
    CHECK(std::fabs(s1 - 1.0) <= 2e-3, "rate %g: sum h1 %.6f", (double)rate, s1);
    for (unsigned b = 0; b < (unsigned)RSP_NPFB; b++) {
        double s = 0;
        for (unsigned k = 0; k < (unsigned)RSP_TAPS; k++) s += p.hpfb[(size_t)b * RSP_TAPS + k];
        CHECK(std::fabs(s - 1.0) <= 1e-3, "rate %g: branch %u sums to %.6f", (double)rate, b, s);
    }
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float least = std::ldexp(1.0f, -38);
    for (float r : { 0.0f, -0.0f, -1.0f, nan, inf, -inf, 1024.5f, std::nextafter(1024.0f, 2048.0f), std::nextafter(least, 0.0f), 1e-12f, 1e-20f, 1e-38f,
                     std::numeric_limits<float>::denorm_min() })
        CHECK(resamp_rate_check(r) != nullptr, "rate %g accepted", (double)r);
    for (float r : { least, std::nextafter(least, 1.0f), 1e-11f, 1.0f / 65536.0f, 0.001f, 0.06f, 0.11f, 0.2f, 0.25f, 0.37f, 0.45f, std::nextafter(0.5f, 0.0f), 0.5f,
                     std::nextafter(0.5f, 1.0f), 0.64f, 0.7f, 0.8f, 0.999f, std::nextafter(1.0f, 0.0f), 1.0f, std::nextafter(1.0f, 2.0f), 1.25f, 1.5f,
                     std::nextafter(2.0f, 0.0f), 2.0f, std::nextafter(2.0f, 3.0f), 4.0f, 6.3f, 16.0f, 100.0f, 1024.0f })
        check_plan(r);
    // the values at the edges
    struct { float rate; bool interp; unsigned ns; unsigned long long step; long long per_in, per_out; float delay; } want[] = {
        { 0.5f, false, 0, 1ull << 25, 2, 1, 7.f },
        { std::nextafter(0.5f, 0.0f), false, 1, (1ull << 24) + 1, (1ll << 24) + 1, 1ll << 24, 27.f },
        { 1.0f, false, 0, 1ull << 24, 1, 1, 7.f },
        { std::nextafter(1.0f, 2.0f), true, 0, (1ull << 24) - 2, (1ll << 23) - 1, 1ll << 23, 7.f },
        { 2.0f, true, 0, 1ull << 23, 1, 2, 7.f },
        { std::nextafter(2.0f, 3.0f), true, 1, (1ull << 24) - 2, (1ll << 23) - 1, 1ll << 23, 0.f },
        { 1024.0f, true, 9, 1ull << 23, 1, 2, 0.f },
        { least, false, 37, 1ull << 25, 2, 1, 0.f },
        { 0.8f, false, 0, 20971520ull, 5, 4, 7.f },
        { 0.64f, false, 0, 26214401ull, 26214401, 1ll << 24, 7.f },       // 16/25 is no float: the step of (float)0.64 is odd, the table build
    };
    for (const auto &w : want) {
        const ResampPlan p = resamp_plan(w.rate, 60.0f);
        CHECK(p.interp == w.interp && p.num_stages == w.ns && p.step == w.step && p.per_in == w.per_in && p.per_out == w.per_out,
              "rate %.9g: interp %d stages %u step %llu period %lld %lld", (double)w.rate, (int)p.interp, p.num_stages, p.step, p.per_in, p.per_out);
        if (w.delay != 0.f) CHECK(p.delay == w.delay, "rate %.9g: delay %g", (double)w.rate, (double)p.delay);
    }
    CHECK(resamp_plan(4.0f, 60.f).delay == 10.5f && resamp_plan(16.0f, 60.f).delay == 13.125f, "delay at 4 and 16");
    CHECK(std::fabs(resamp_plan(6.3f, 60.f).delay - 13.66667f) < 1e-4f && std::fabs(resamp_plan(100.0f, 60.f).delay - 15.82f) < 1e-4f, "delay at 6.3 and 100");
    if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
    printf("resamp_plan_test ok\n");
    return 0;
}
