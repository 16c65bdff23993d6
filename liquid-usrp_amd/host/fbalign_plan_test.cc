// fbalign_plan_test.cc -- the feedback aligner's host arithmetic without a GPU (tests/test_fbalign.py): csrc/fbalign_plan.hpp's
// configuration check refuses what include/mcrx_hip.h says create refuses and nothing else; the constants; the quantiser on exact
// cases, on ties, at the clamps and on values that are not finite; the split of a delay and the coefficients at whole samples, at the
// table's rows and at both ends of the range, every tap index inside a call's input; the worst term against the bound the guard is
// derived from and the guard at its edge; rows, tiles and grids.  Built by `make fbalign_plan_test`; `make fbalign_plan_test SAN=1`
// builds the same program under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include "../csrc/fbalign_plan.hpp"

using namespace mcrx;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_bad <= 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static mcrx_hip_fbalign_config good()
{
    mcrx_hip_fbalign_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c); c.max_lag = 16; c.full_scale = 0.75f; c.target_gain = 2.f; c.min_rows = 64; c.input_format = 1;
    return c;
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    mcrx_hip_fbalign_config c = good();
    CHECK(fbalign_check(&c) == nullptr, "%s", fbalign_check(&c));
#define REFUSED(stmt) do { c = good(); stmt; CHECK(fbalign_check(&c) != nullptr, "accepted: %s", #stmt); } while (0)
#define ACCEPTED(stmt) do { c = good(); stmt; CHECK(fbalign_check(&c) == nullptr, "refused: %s", #stmt); } while (0)
    REFUSED(c.struct_size -= 4); REFUSED(c.max_lag = 7); REFUSED(c.max_lag = 65); REFUSED(c.full_scale = 0.f); REFUSED(c.full_scale = -1.f);
    REFUSED(c.full_scale = nan); REFUSED(c.full_scale = inf); REFUSED(c.target_gain = 0.f); REFUSED(c.target_gain = -2.f); REFUSED(c.target_gain = nan);
    REFUSED(c.target_gain = inf); REFUSED(c.min_rows = 0); REFUSED(c.input_format = 2);
    ACCEPTED(c.max_lag = 8); ACCEPTED(c.max_lag = 64); ACCEPTED(c.full_scale = 1e-30f); ACCEPTED(c.full_scale = 3e38f); ACCEPTED(c.target_gain = 1e-30f);
    ACCEPTED(c.target_gain = 3e38f); ACCEPTED(c.min_rows = 1); ACCEPTED(c.min_rows = 0xffffffffu); ACCEPTED(c.input_format = 0);
#undef REFUSED
#undef ACCEPTED
    // the constants
    c = good();
    FbalignConsts k = fbalign_consts(&c);
    CHECK(k.Lm == 16 && k.R == 24 && k.halo == 33 && k.sums == 2 * 24 + 19 && k.e == 0, "shape: %u %u %u %u %d", k.Lm, k.R, k.halo, k.sums, k.e);
    c.full_scale = 1.f; CHECK(fbalign_consts(&c).e == 0, "E = 1 for full_scale 1");
    c.full_scale = 1.0000001f; CHECK(fbalign_consts(&c).e == 1, "E = 2 just above");
    c.full_scale = 0.25f; CHECK(fbalign_consts(&c).e == -2, "E = 1/4");
    c.max_lag = 64; CHECK(fbalign_consts(&c).R == (uint32_t)FBA_MAX_R && fbalign_consts(&c).sums == 163 && fbalign_consts(&c).sums <= (uint32_t)FBA_WG, "the largest shape");
    CHECK(k.h[0] < 0.f && k.h[1] > 0.f && std::fabs(k.h[0] + 0.9722586f) < 1e-6f && std::fabs(k.h[7] - 0.01346767f) < 1e-7f, "taps %g %g", k.h[0], k.h[7]);
    for (int i = 1; i < FBA_H; i++) CHECK(std::fabs(k.h[i]) < std::fabs(k.h[i - 1]), "the taps fall off");
    // the quantiser: E = 1
    bool bad = false;
    CHECK(fbalign_q15(0.5f, 0, &bad) == 16384 && !bad, "0.5");
    CHECK(fbalign_q15(-1.f, 0, &bad) == -32768 && !bad, "-1 is the last value that does not clamp");
    CHECK(fbalign_q15(0x1.fffcp-1f, 0, &bad) == 32767 && !bad, "32767 / 32768");
    CHECK(fbalign_q15(0x1p-16f, 0, &bad) == 0 && fbalign_q15(0x3p-16f, 0, &bad) == 2 && fbalign_q15(-0x5p-16f, 0, &bad) == -2 && !bad, "ties go to even");
    CHECK(fbalign_q15(-0.0f, 0, &bad) == 0 && !bad, "-0.0");
    bad = false; CHECK(fbalign_q15(1.f, 0, &bad) == 32767 && bad, "+1 clamps");
    bad = false; CHECK(fbalign_q15(0x1.fffep-1f, 0, &bad) == 32767 && bad, "32767.5 goes to the even 32768, which clamps");
    bad = false; CHECK(fbalign_q15(-1.00002f, 0, &bad) == -32768 && bad, "-32768.66 rounds to -32769, which clamps");
    bad = false; CHECK(fbalign_q15(-1.00001f, 0, &bad) == -32768 && !bad, "-32768.33 rounds to -32768, which does not");
    bad = false; CHECK(fbalign_q15(nan, 0, &bad) == 0 && bad, "NaN");
    bad = false; CHECK(fbalign_q15(inf, 0, &bad) == 32767 && bad, "+inf");
    bad = false; CHECK(fbalign_q15(-inf, 0, &bad) == -32768 && bad, "-inf");
    bad = false; CHECK(fbalign_q15(3e38f, 0, &bad) == 32767 && bad, "overflow of the scaling");
    bad = false; CHECK(fbalign_q15(4.f, 3, &bad) == 16384 && fbalign_q15(0.125f, -2, &bad) == 16384 && !bad, "E = 8, E = 1/4");
    bad = false; CHECK(fbalign_word(-1.f, 0.5f, 0, &bad) == (0x8000u | (16384u << 16)) && !bad, "the LDS word");
    // the split and the coefficients
    const float *W = userclock_table();
    float co[FBA_TAPS];
    FbalignSplit s = fbalign_split(0);
    CHECK(s.nd == 0 && s.r == 0 && s.f == 0.f, "tau = 0");
    fbalign_coefs(W, 0, co);
    for (int j = 0; j < FBA_TAPS; j++) CHECK(co[j] == (j == 15 ? 1.f : 0.f), "the unit vector at tau = 0: tap %d = %g", j, co[j]);
    s = fbalign_split((int64_t)3 << 32);
    CHECK(s.nd == -3 && s.r == 0 && s.f == 0.f, "three whole samples late");
    s = fbalign_split(((int64_t)7 << 32) + ((int64_t)1 << 31));
    CHECK(s.nd == -8 && s.r == 32 && s.f == 0.f, "7.5 samples late: nd = -8 and half a sample forward");
    s = fbalign_split(-(((int64_t)2 << 32) + ((int64_t)1 << 26) + 4));
    CHECK(s.nd == 2 && s.r == 1 && s.f == 0x1p-24f, "2 + 1/64 + 2^-30 early: row 1 and one step of the fraction");
    s = fbalign_split(-1);
    CHECK(s.nd == 0 && s.r == 0 && s.f == 0.f, "the two lowest bits are not used");
    s = fbalign_split(1);
    CHECK(s.nd == -1 && s.r == 63 && s.f == 0x1.fffffep-1f, "just late: the last interval of the table");
    fbalign_coefs(W, 1, co);
    CHECK(co[16] > 0.999999f && std::fabs(co[15]) < 1e-6f, "... which ends at the unit vector of tap 16: %g %g", co[16], co[15]);
    float sum = 0.f;
    fbalign_coefs(W, (int64_t)1 << 31, co);
    for (int j = 0; j < FBA_TAPS; j++) sum += co[j];
    CHECK(std::fabs(sum - 1.f) < 1e-2f && co[15] == co[16], "half a sample: symmetric, DC gain within 1 %% of 1: %g", sum);
    for (uint32_t Lm = FBA_MIN_LAG; Lm <= (uint32_t)FBA_MAX_LAG; Lm += 8) {
        const int64_t most = (int64_t)(Lm + 1) << 32;
        const uint32_t halo = Lm + 17;
        CHECK(fbalign_tau_ok(most, Lm) && fbalign_tau_ok(-most, Lm) && !fbalign_tau_ok(most + 1, Lm) && !fbalign_tau_ok(-most - 1, Lm), "the range of tau at Lm = %u", Lm);
        const int64_t taus[5] = { most, -most, most - 1, -most + 1, 0 };
        for (int64_t tau : taus) {
            const int nd = fbalign_split(tau).nd;
            CHECK((int)halo - nd + 15 - 31 >= 0 && (int)halo - nd + 15 <= 2 * (int)halo, "the taps of output 0 lie in in[0 .. 2 halo] at Lm = %u, nd = %d", Lm, nd);
        }
    }
    CHECK(FBA_WIN >= 2 * FBA_WG + FBA_TAPS && FBA_WIN % 2 == 0, "the window holds 512 outputs' taps in whole pairs");
    // the guard
    bad = false;
    const double t = (double)fbalign_q15(-1.f, 0, &bad);
    CHECK(2.0 * t * t == fbalign_term_bound() && fbalign_term_bound() == 2147483648.0, "the worst term is 2^31");
    CHECK(fbalign_term_bound() * (double)(1ull << FBA_GUARD_LOG2) < 9223372036854775807.0, "2^31 terms of 2^31");
    const uint64_t most = 1ull << FBA_GUARD_LOG2;
    CHECK(fbalign_guard_ok(0, most) && !fbalign_guard_ok(0, most + 1) && fbalign_guard_ok(most - 1, 1) && !fbalign_guard_ok(most, 1) && fbalign_guard_ok(most, 0)
          && !fbalign_guard_ok(1, ~0ull) && !fbalign_guard_ok(~0ull, 1), "the guard at its edge");
    // rows, tiles, grids
    CHECK(fbalign_rows(0, 24) == 0 && fbalign_rows(48, 24) == 0 && fbalign_rows(49, 24) == 1 && fbalign_rows(1ull << 32, 72) == (1ull << 32) - 144, "rows");
    CHECK(fbalign_tiles(1) == 1 && fbalign_tiles(256) == 1 && fbalign_tiles(257) == 2, "tiles");
    CHECK(fbalign_measure_grid(1) == 1 && fbalign_measure_grid(256 * 256) == 256 && fbalign_measure_grid(256 * 256 + 1) == 256 && fbalign_measure_grid(1ull << 31) == 256, "measure grid");
    CHECK(fbalign_apply_grid(0, 1) == 1 && fbalign_apply_grid(0, 512) == 1 && fbalign_apply_grid(1, 512) == 2 && fbalign_apply_grid(0, 513) == 2, "apply grid");
    if (g_bad) { fprintf(stderr, "fbalign_plan_test: %d failures\n", g_bad); return 1; }
    printf("fbalign_plan_test ok\n");
    return 0;
}
