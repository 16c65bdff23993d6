// pamem_plan_test.cc -- the amplifier with memory's host arithmetic without a GPU (tests/test_pamem.py): csrc/pamem_plan.hpp's
// configuration check refuses what include/mcrx_hip.h says create refuses and nothing else, and looks at no branch beyond `branches`;
// lead, r_b and the flattened tap list of a configuration; the LDS bytes, the rounds, the grid at its edges and the size limit.
// Built by `make pamem_plan_test`; `make pamem_plan_test SAN=1` builds the same program under the address and undefined-behaviour
// sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include "../csrc/pamem_plan.hpp"

using namespace mcrx;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_bad <= 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

// three branches: taps at (0), (1, 4), (0, 2, 16)
static mcrx_hip_pamem_config good()
{
    mcrx_hip_pamem_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c); c.branches = 3; c.input_format = 0; c.output_format = 1; c.gain = 0.9f;
    for (int b = 0; b < 3; b++) {
        c.branch[b].sat = 0.5f + 0.25f * (float)b; c.branch[b].amp_gain = 1.f; c.branch[b].ampm = 0.01f * (float)b; c.branch[b].smooth = 1u << b;
        c.branch[b].taps = (uint32_t)b + 1u;
    }
    c.branch[0].delay[0] = 0; c.branch[0].h_re[0] = 1.f;
    c.branch[1].delay[0] = 1; c.branch[1].delay[1] = 4; c.branch[1].h_re[0] = 0.1f; c.branch[1].h_im[0] = -0.2f; c.branch[1].h_re[1] = 0.f;
    c.branch[2].delay[0] = 0; c.branch[2].delay[1] = 2; c.branch[2].delay[2] = 16; c.branch[2].h_im[2] = 0.03f;
    return c;
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    mcrx_hip_pamem_config c = good();
    CHECK(pamem_check(&c) == nullptr, "%s", pamem_check(&c));
    CHECK(sizeof(mcrx_hip_pamem_branch) == 29 * 4 && sizeof(mcrx_hip_pamem_config) == 5 * 4 + 4 * 29 * 4, "the structs have no padding");
#define REFUSED(stmt) do { c = good(); stmt; CHECK(pamem_check(&c) != nullptr, "accepted: %s", #stmt); } while (0)
#define ACCEPTED(stmt) do { c = good(); stmt; CHECK(pamem_check(&c) == nullptr, "refused: %s", #stmt); } while (0)
    REFUSED(c.struct_size -= 4); REFUSED(c.branches = 0); REFUSED(c.branches = 5); REFUSED(c.input_format = 2); REFUSED(c.output_format = 2);
    REFUSED(c.gain = nan); REFUSED(c.gain = inf); REFUSED(c.branch[1].taps = 0); REFUSED(c.branch[1].taps = 9);
    REFUSED(c.branch[2].delay[2] = 17); REFUSED(c.branch[2].delay[2] = 2); REFUSED(c.branch[2].delay[1] = 0); REFUSED(c.branch[1].delay[0] = 5);
    REFUSED(c.branch[0].h_re[0] = nan); REFUSED(c.branch[2].h_im[1] = inf); REFUSED(c.branch[1].h_re[1] = -inf);
    REFUSED(c.branch[0].smooth = 3); REFUSED(c.branch[2].smooth = 0); REFUSED(c.branch[1].sat = 0.f); REFUSED(c.branch[1].sat = -1.f);
    REFUSED(c.branch[1].sat = nan); REFUSED(c.branch[1].sat = inf); REFUSED(c.branch[1].sat = 1e-30f); REFUSED(c.branch[1].sat = 3e30f);
    REFUSED(c.branch[2].amp_gain = nan); REFUSED(c.branch[2].amp_gain = inf); REFUSED(c.branch[0].ampm = 0.26f); REFUSED(c.branch[0].ampm = -0.26f);
    REFUSED(c.branch[0].ampm = nan);
    ACCEPTED(c.branches = 1); ACCEPTED(c.branches = 2; c.branch[2].taps = 99; c.branch[2].sat = nan; c.branch[2].smooth = 7);   // not looked at
    ACCEPTED(c.branch[3].taps = 0); ACCEPTED(c.branches = 4; c.branch[3] = c.branch[2]); ACCEPTED(c.input_format = 1; c.output_format = 0);
    ACCEPTED(c.gain = 0.f); ACCEPTED(c.gain = -3.f); ACCEPTED(c.branch[0].h_re[0] = 0.f); ACCEPTED(c.branch[0].delay[0] = 16);
    ACCEPTED(c.branch[1].delay[5] = 99; c.branch[1].h_re[7] = nan);                                                              // beyond taps
    ACCEPTED(c.branch[0].ampm = 0.25f); ACCEPTED(c.branch[0].ampm = -0.25f); ACCEPTED(c.branch[1].amp_gain = -2.f);
    ACCEPTED(c.branch[1].sat = 1e-18f); ACCEPTED(c.branch[1].sat = 1e18f);
    ACCEPTED(c.branch[0].taps = 8; for (uint32_t k = 0; k < 8; k++) c.branch[0].delay[k] = 2 * k + 2);
#undef REFUSED
#undef ACCEPTED
    // the constants
    c = good();
    PamemConsts k = pamem_consts(&c);
    CHECK(k.B == 3 && k.lead == 16 && k.total == 6 && k.gain == 0.9f, "shape: %u %u %u", k.B, k.lead, k.total);
    CHECK(k.first[0] == 0 && k.first[1] == 1 && k.first[2] == 3 && k.taps[0] == 1 && k.taps[1] == 2 && k.taps[2] == 3, "first and taps");
    const uint32_t wb[6] = {0, 1, 1, 2, 2, 2}, wd[6] = {0, 1, 4, 0, 2, 16};
    for (int i = 0; i < 6; i++) CHECK(k.tap_branch[i] == wb[i] && k.tap_delay[i] == wd[i], "tap %d: %u %u", i, k.tap_branch[i], k.tap_delay[i]);
    CHECK(k.tap_re[0] == 1.f && k.tap_im[0] == 0.f && k.tap_re[1] == 0.1f && k.tap_im[1] == -0.2f && k.tap_im[5] == 0.03f, "weights");
    for (uint32_t b = 0; b < 3; b++) {
        CHECK(k.r[b] == (float)(1.0 / ((double)c.branch[b].sat * (double)c.branch[b].sat)), "r[%u] is rounded once", b);
        CHECK(k.smooth[b] == (1u << b) && k.ampm[b] == c.branch[b].ampm && k.amp_gain[b] == 1.f, "branch %u", b);
    }
    CHECK(rapp_inv_sat2(0.5f) == 4.f && rapp_inv_sat2(3.f) == (float)(1.0 / 9.0), "1 / A^2");
    c.branches = 1;
    CHECK(pamem_consts(&c).lead == 0 && pamem_consts(&c).total == 1, "lead 0");
    c.branches = 2;
    CHECK(pamem_consts(&c).lead == 4 && pamem_consts(&c).total == 3, "lead 4");
    // LDS, rounds, grid, size
    CHECK(pamem_plane(0) == 512 && pamem_plane(1) == 514 && pamem_plane(2) == 514 && pamem_plane(15) == 528 && pamem_plane(16) == 528, "planes are even");
    CHECK(pamem_lds(1, 0) == 4096 && pamem_lds(4, 16) == 16896 && pamem_lds(3, 2) == 3 * 514 * 8, "LDS");
    CHECK(pamem_rounds() == 4 && pamem_span() == 2048, "rounds");
    CHECK(pamem_parity(0x1000, 8) == 0 && pamem_parity(0x1008, 8) == 1 && pamem_parity(0x1008, 4) == 0 && pamem_parity(0x1004, 4) == 1, "parity");
    CHECK(pamem_grid(0, 1) == 1 && pamem_grid(0, 2048) == 1 && pamem_grid(0, 2049) == 2 && pamem_grid(1, 2047) == 1 && pamem_grid(1, 2048) == 2, "grid");
    CHECK(pamem_grid(0, 1ull << 32) == (1u << 21) && pamem_grid(1, 1ull << 32) == (1u << 21) + 1, "the largest grid");
    CHECK(!pamem_size_check(1ull << 32, 0) && pamem_size_check((1ull << 32) + 1, 0) && !pamem_size_check((1ull << 32) - 16, 16)
          && pamem_size_check((1ull << 32) - 15, 16) && !pamem_size_check(0, 16), "the size limit");
    if (g_bad) { fprintf(stderr, "pamem_plan_test: %d failures\n", g_bad); return 1; }
    printf("pamem_plan_test ok\n");
    return 0;
}
