// mpd_plan_test.cc -- the memory-polynomial predistorter's host arithmetic without a GPU (tests/test_mpd.py): csrc/mpd_plan.hpp's
// configuration check refuses what include/mcrx_hip.h says create refuses and nothing else; the constants are dpd's plus inv_g0; the
// integers of feedback and target samples on exact cases, on ties and at the edges of eligibility; the worst term against the bound the
// guard is derived from, the guard at its edge and across updates; the grids and the LDS sizes.  Built by `make mpd_plan_test`;
// `make mpd_plan_test SAN=1` builds the same program under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include "../csrc/mpd_plan.hpp"

using namespace mcrx;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_bad <= 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static mcrx_hip_mpd_config good()
{
    mcrx_hip_mpd_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c); c.branches = 3; c.delay[0] = 0; c.delay[1] = 1; c.delay[2] = 5; c.order = 5; c.table_log2 = 7;
    c.full_scale = 0.75f; c.target_gain = 2.f; c.min_rows = 15; c.ridge_log2 = 30; c.forget_shift = 2; c.gain = 1.f; c.output_format = 1;
    return c;
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    mcrx_hip_mpd_config c = good();
    CHECK(mpd_check(&c) == nullptr, "%s", mpd_check(&c));
#define REFUSED(stmt) do { c = good(); stmt; CHECK(mpd_check(&c) != nullptr, "accepted: %s", #stmt); } while (0)
#define ACCEPTED(stmt) do { c = good(); stmt; CHECK(mpd_check(&c) == nullptr, "refused: %s", #stmt); } while (0)
    REFUSED(c.struct_size -= 4); REFUSED(c.branches = 0); REFUSED(c.branches = 5); REFUSED(c.delay[0] = 1); REFUSED(c.delay[1] = 0);
    REFUSED(c.delay[2] = 1); REFUSED(c.delay[2] = 17); REFUSED(c.order = 0); REFUSED(c.order = 6); REFUSED(c.table_log2 = 4);
    REFUSED(c.table_log2 = 11); REFUSED(c.table_log2 = 10); REFUSED(c.full_scale = 0.f); REFUSED(c.full_scale = -1.f); REFUSED(c.full_scale = nan);
    REFUSED(c.full_scale = inf); REFUSED(c.full_scale = 1e-42f); REFUSED(c.target_gain = 0.f); REFUSED(c.target_gain = -2.f);
    REFUSED(c.target_gain = nan); REFUSED(c.target_gain = inf); REFUSED(c.min_rows = 14); REFUSED(c.ridge_log2 = 9); REFUSED(c.ridge_log2 = 41);
    REFUSED(c.forget_shift = 9); REFUSED(c.gain = nan); REFUSED(c.gain = inf); REFUSED(c.output_format = 2);
    REFUSED(c.branches = 4; c.delay[3] = 5); REFUSED(c.branches = 4; c.delay[3] = 6; c.order = 5; c.min_rows = 19);
    ACCEPTED(c.branches = 1; c.table_log2 = 10); ACCEPTED(c.branches = 2; c.table_log2 = 10); ACCEPTED(c.table_log2 = 9);
    ACCEPTED(c.branches = 4; c.delay[3] = 16; c.min_rows = 20; c.table_log2 = 9); ACCEPTED(c.branches = 2; c.delay[2] = 99);
    ACCEPTED(c.delay[2] = 16); ACCEPTED(c.order = 1); ACCEPTED(c.full_scale = 1e-30f); ACCEPTED(c.full_scale = 3e38f);
    ACCEPTED(c.target_gain = 1e-30f); ACCEPTED(c.target_gain = 3e38f); ACCEPTED(c.min_rows = 0xffffffffu); ACCEPTED(c.ridge_log2 = 10);
    ACCEPTED(c.ridge_log2 = 40); ACCEPTED(c.forget_shift = 0); ACCEPTED(c.forget_shift = 8); ACCEPTED(c.gain = 0.f); ACCEPTED(c.gain = -3.f);
    ACCEPTED(c.output_format = 0);
#undef REFUSED
#undef ACCEPTED
    // the constants: dpd's, inv_g0, the shape
    c = good();
    MpdConsts k = mpd_consts(&c);
    mcrx_hip_dpd_config d;
    memset(&d, 0, sizeof(d));
    d.struct_size = sizeof(d); d.table_log2 = 7; d.full_scale = 0.75f; d.target_gain = 2.f; d.min_count = 1;
    const DpdConsts dk = dpd_consts(&d);
    CHECK(k.K == dk.K && k.inv_step == dk.inv_step && k.step == dk.step && k.e == dk.e && k.Kf == dk.Kf, "dpd's constants");
    CHECK(k.inv_g0 == 0.5f && k.M == 3 && k.P == 5 && k.L == 15 && k.lead == 5 && k.sums == 136 && k.delay[1] == 1, "shape");
    c.target_gain = 3.f;
    CHECK(mpd_consts(&c).inv_g0 == (float)(1.0 / 3.0), "inv_g0 is rounded once");
    c.branches = 4; c.delay[3] = 16; c.table_log2 = 9;
    CHECK(mpd_consts(&c).L == 20 && mpd_consts(&c).sums == (uint32_t)MPD_MAX_SUMS && mpd_consts(&c).lead == 16, "the largest shape");
    // the integers: E = 1, g0 = 2
    int32_t br[MPD_MAX_ORDER], bi[MPD_MAX_ORDER], ur, ui;
    CHECK(mpd_basis(1.f, 0.f, 0.5f, 0, 5, br, bi), "0.5 is good");
    for (int p = 0; p < 5; p++) CHECK(br[p] == (65536 >> p) && bi[p] == 0, "power %d: %d %d", p, br[p], bi[p]);
    CHECK(mpd_basis(0.f, -2.f, 0.5f, 0, 3, br, bi) && br[0] == 0 && bi[0] == -131072 && bi[2] == -131072 && bi[3] == 0 && bi[4] == 0, "amplitude 1 is good; P = 3");
    CHECK(!mpd_basis(0.f, -2.0000002f, 0.5f, 0, 5, br, bi) && bi[0] == 0 && bi[4] == 0, "beyond 1 is not, and gives zeros");
    CHECK(!mpd_basis(nan, 0.f, 0.5f, 0, 5, br, bi) && !mpd_basis(0.f, nan, 0.5f, 0, 5, br, bi) && !mpd_basis(inf, 0.f, 0.5f, 0, 5, br, bi)
          && !mpd_basis(0.f, -inf, 0.5f, 0, 5, br, bi) && !mpd_basis(3e38f, 3e38f, 0.5f, 0, 5, br, bi) && br[0] == 0, "NaN, infinity, overflow of t");
    CHECK(mpd_basis(0.f, 0.f, 0.5f, 0, 5, br, bi) && br[0] == 0 && bi[4] == 0, "zero");
    CHECK(mpd_basis(0x1p-17f, 0x3p-17f, 0.5f, 0, 1, br, bi) && br[0] == 0 && bi[0] == 2, "ties go to even: 0.5 -> 0, 1.5 -> 2");
    CHECK(mpd_basis(4.f, 0.f, 0.5f, 2, 2, br, bi) && br[0] == 65536 && br[1] == 32768, "E = 4");
    CHECK(mpd_basis(0.25f, 0.f, 0.5f, -2, 2, br, bi) && br[0] == 65536 && br[1] == 32768, "E = 1/4");
    CHECK(mpd_target(2.f, 0.f, 0, &ur, &ui) && ur == 262144 && ui == 0, "|u| = 2 E is good");
    CHECK(!mpd_target(2.0000002f, 0.f, 0, &ur, &ui) && ur == 0, "beyond it is not");
    CHECK(!mpd_target(nan, 0.f, 0, &ur, &ui) && !mpd_target(0.f, inf, 0, &ur, &ui) && !mpd_target(3e38f, 0.f, 0, &ur, &ui), "NaN, infinity, overflow");
    CHECK(mpd_target(-0.75f, 0x5p-18f, 0, &ur, &ui) && ur == -98304 && ui == 2, "-0.75; 2.5 -> 2");
    CHECK(mpd_target(8.f, -8.f, 3, &ur, &ui) && ur == 131072 && ui == -131072, "E = 8");
    // the worst terms against the bound: the largest good samples, every component, and 2^26 of them
    float top = 2.f;
    while (mpd_basis(std::nextafterf(top, inf), 0.f, 0.5f, 0, 5, br, bi)) top = std::nextafterf(top, inf);
    CHECK(mpd_basis(top, 0.f, 0.5f, 0, 5, br, bi), "top");
    float utop = 2.f;
    while (mpd_target(std::nextafterf(utop, inf), 0.f, 0, &ur, &ui)) utop = std::nextafterf(utop, inf);
    CHECK(mpd_target(utop, 0.f, 0, &ur, &ui), "utop");
    for (int p = 0; p < 5; p++) CHECK((double)br[p] * br[p] * 4.0 <= mpd_term_bound() && br[p] <= br[0], "power %d: %d", p, br[p]);
    CHECK((double)ur * ur <= mpd_term_bound() && (double)ur * br[0] <= mpd_term_bound(), "Suu %d", ur);
    const float h = std::sqrt(0.5f);
    CHECK(mpd_basis(2.f * h, 2.f * h, 0.5f, 0, 5, br, bi), "on the diagonal");
    CHECK(2.0 * (double)br[0] * br[0] <= mpd_term_bound() / 4.0 * 1.0001, "the modulus bounds the term, not the component: %d", br[0]);
    CHECK(mpd_term_bound() < 68956000000.0 && mpd_term_bound() * (double)(1ull << MPD_GUARD_LOG2) < 9223372036854775807.0 / 1.9, "2^26 terms of 2^36.01");
    const uint64_t most = 1ull << MPD_GUARD_LOG2;
    const auto guard_ok = [](uint64_t since, uint64_t n) { return pd_guard_ok(since, n, MPD_GUARD_LOG2); };
    CHECK(guard_ok(0, most) && !guard_ok(0, most + 1) && guard_ok(most - 1, 1) && !guard_ok(most, 1) && guard_ok(most, 0)
          && !guard_ok(1, ~0ull) && !guard_ok(~0ull, 1), "the guard at its edge");
    CHECK(pd_guard_after_update(most, 0) == most && pd_guard_after_update(most, 2) == most / 4 && pd_guard_after_update(5, 2) == 2
          && pd_guard_after_update(1, 8) == 1 && pd_guard_after_update(0, 8) == 0 && pd_guard_after_update(257, 8) == 2, "the guard across an update");
    // rows, tiles, grids, LDS
    CHECK(mpd_rows(0, 0) == 0 && mpd_rows(5, 5) == 0 && mpd_rows(6, 5) == 1 && mpd_rows(3, 16) == 0 && mpd_rows(1ull << 32, 16) == (1ull << 32) - 16, "rows");
    CHECK(mpd_tiles(1) == 1 && mpd_tiles(256) == 1 && mpd_tiles(257) == 2, "tiles");
    CHECK(mpd_measure_grid(1) == 1 && mpd_measure_grid(256 * 1024) == 1024 && mpd_measure_grid(256 * 1024 + 1) == 1024 && mpd_measure_grid(1ull << 26) == 1024, "measure grid");
    CHECK(mpd_rounds(1, 32) == pd_rounds(32) && mpd_rounds(1, 1024) == pd_rounds(1024) && mpd_rounds(4, 128) == 16 && mpd_rounds(2, 32) == 4, "rounds");
    CHECK(mpd_apply_lds(1, 1024, 0) == 16384 && mpd_apply_lds(4, 512, 16) == 32768 + 528 * 16 && mpd_apply_lds(2, 1024, 1) == 32768 + 513 * 16, "apply LDS");
    CHECK(mpd_measure_lds(5, 16) == (272 * 5 + 256) * 8 + (512 + 16) * 4 && mpd_measure_lds(5, 16) < 16 * 1024 && mpd_measure_lds(1, 0) == 512 * 8 + 512 * 4, "measure LDS");
    if (g_bad) { fprintf(stderr, "mpd_plan_test: %d failures\n", g_bad); return 1; }
    printf("mpd_plan_test ok\n");
    return 0;
}
