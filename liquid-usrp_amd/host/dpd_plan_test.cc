// dpd_plan_test.cc -- the predistorter's host arithmetic without a GPU (tests/test_dpd.py): csrc/dpd_plan.hpp's configuration check
// refuses what include/mcrx_hip.h says create refuses and nothing else; inv_step, step and e are what the definition says, e at, below
// and above powers of two; bins on edges, ties and beyond the table; every kind of ineligible pair; the terms of a pair as exact
// integers; the worst term against the bound the guard is derived from, the guard at its edge and across updates; the grids and the
// LDS sizes.  Built by `make dpd_plan_test`; `make dpd_plan_test SAN=1` builds the same program under the address and
// undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include "../csrc/dpd_plan.hpp"

using namespace mcrx;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_bad <= 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static mcrx_hip_dpd_config good()
{
    mcrx_hip_dpd_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c); c.table_log2 = 7; c.full_scale = 0.75f; c.target_gain = 2.f; c.min_count = 8; c.forget_shift = 2;
    c.gain = 1.f; c.output_format = 1;
    return c;
}

static int bin_of(const DpdConsts &k, float ur, float ui, float zr, float zi)
{
    int j = 12345;
    const bool ok = dpd_bin(ur, ui, zr, zi, k.inv_step, k.Kf, k.zmax2, &j);
    CHECK(ok == (j >= 0), "ok %d, j %d", (int)ok, j);
    return j;
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    mcrx_hip_dpd_config c = good();
    CHECK(dpd_check(&c) == nullptr, "%s", dpd_check(&c));
#define REFUSED(stmt) do { c = good(); stmt; CHECK(dpd_check(&c) != nullptr, "accepted: %s", #stmt); } while (0)
#define ACCEPTED(stmt) do { c = good(); stmt; CHECK(dpd_check(&c) == nullptr, "refused: %s", #stmt); } while (0)
    REFUSED(c.struct_size -= 4); REFUSED(c.table_log2 = 4); REFUSED(c.table_log2 = 11); REFUSED(c.full_scale = 0.f);
    REFUSED(c.full_scale = -1.f); REFUSED(c.full_scale = nan); REFUSED(c.full_scale = inf); REFUSED(c.full_scale = 1e-42f);
    REFUSED(c.target_gain = 0.f); REFUSED(c.target_gain = -2.f); REFUSED(c.target_gain = nan); REFUSED(c.target_gain = inf);
    REFUSED(c.min_count = 0); REFUSED(c.forget_shift = 9); REFUSED(c.gain = nan); REFUSED(c.gain = inf); REFUSED(c.output_format = 2);
    ACCEPTED(c.table_log2 = 5); ACCEPTED(c.table_log2 = 10); ACCEPTED(c.full_scale = 1e-30f); ACCEPTED(c.full_scale = 3e38f);
    ACCEPTED(c.target_gain = 1e-30f); ACCEPTED(c.min_count = 1); ACCEPTED(c.min_count = 0xffffffffu); ACCEPTED(c.forget_shift = 0);
    ACCEPTED(c.forget_shift = 8); ACCEPTED(c.gain = 0.f); ACCEPTED(c.gain = -3.f); ACCEPTED(c.output_format = 0);
#undef REFUSED
#undef ACCEPTED
    // the constants
    struct { float fs; int e; } es[] = { { 1.f, 0 }, { 0.75f, 0 }, { 0.5f, -1 }, { 0.50000006f, 0 }, { 2.f, 1 }, { 2.0000002f, 2 }, { 1e-3f, -9 },
                                         { 3e38f, 128 }, { 1e-30f, -99 } };
    for (auto &t : es) {
        c = good(); c.full_scale = t.fs;
        const DpdConsts k = dpd_consts(&c);
        CHECK(k.e == t.e, "full_scale %g: e %d, want %d", t.fs, k.e, t.e);
        CHECK(std::ldexp(1.0, k.e) >= (double)t.fs && std::ldexp(1.0, k.e - 1) < (double)t.fs, "full_scale %g: e %d", t.fs, k.e);
        CHECK(k.K == 128u && k.Kf == 128.f && k.step == (double)t.fs / 128.0 && k.inv_step == (float)(128.0 / (double)t.fs), "full_scale %g", t.fs);
        CHECK(k.scale == std::ldexp(1.0, 32 - 2 * k.e), "full_scale %g: scale", t.fs);
    }
    // bins: K = 32 on full_scale 1 makes inv_step 32 and every product below exact
    c = good(); c.table_log2 = 5; c.full_scale = 1.f;
    const DpdConsts k = dpd_consts(&c);
    CHECK(k.inv_step == 32.f && k.e == 0 && k.zmax2 == 16.f && k.scale == 4294967296.0, "constants of the bin cases");
    CHECK(bin_of(k, 0.f, 0.f, 0.f, 0.f) == 0, "zero");
    for (int j = 0; j <= 32; j++) {
        CHECK(bin_of(k, (float)j / 32.f, 0.f, 0.1f, 0.f) == j, "edge %d", j);
        CHECK(bin_of(k, 0.f, -(float)j / 32.f, 0.1f, 0.f) == j, "edge %d on the imaginary axis", j);
    }
    for (int j = 0; j < 32; j++) {                          // ties go to the even bin
        const int want = (j & 1) ? j + 1 : j;
        CHECK(bin_of(k, ((float)j + 0.5f) / 32.f, 0.f, 0.f, 0.1f) == want, "tie above %d", j);
    }
    CHECK(bin_of(k, 32.5f / 32.f, 0.f, 0.f, 0.f) == 32, "the tie above K goes down to K");
    CHECK(bin_of(k, 32.51f / 32.f, 0.f, 0.f, 0.f) == -1, "beyond the table");
    CHECK(bin_of(k, 10.f, 0.f, 0.f, 0.f) == -1 && bin_of(k, 3e30f, 0.f, 0.f, 0.f) == -1, "far beyond the table, |u|^2 infinite");
    CHECK(bin_of(k, nan, 0.f, 0.f, 0.f) == -1 && bin_of(k, 0.f, nan, 0.f, 0.f) == -1 && bin_of(k, 0.5f, 0.f, nan, 0.f) == -1
          && bin_of(k, 0.5f, 0.f, 0.f, nan) == -1, "NaN components");
    CHECK(bin_of(k, inf, 0.f, 0.f, 0.f) == -1 && bin_of(k, 0.5f, 0.f, 0.f, -inf) == -1, "infinite components");
    CHECK(bin_of(k, 0.5f, 0.f, 4.f, 0.f) == 16 && bin_of(k, 0.5f, 0.f, 0.f, 4.0000005f) == -1 && bin_of(k, 0.5f, 0.f, 3e30f, 0.f) == -1, "|z|^2 against 16 E^2");
    // the terms: exact integers
    long long sre, sim, suu;
    dpd_terms(0.5f, 0.f, 1.f, 0.25f, k.scale, &sre, &sim, &suu);
    CHECK(sre == (1ll << 31) && sim == (1ll << 29) && suu == (1ll << 30), "%lld %lld %lld", sre, sim, suu);
    dpd_terms(0.f, -0.5f, 1.f, 0.25f, k.scale, &sre, &sim, &suu);      // z conj(u) = (1 + 0.25 i)(0.5 i) = -0.125 + 0.5 i
    CHECK(sre == -(1ll << 29) && sim == (1ll << 31) && suu == (1ll << 30), "%lld %lld %lld", sre, sim, suu);
    dpd_terms(0x1p-17f, 0.f, 0x1p-16f, -0x1p-17f, k.scale, &sre, &sim, &suu);       // 2^-33 2^32 = 1/2 ties to 0; -2^-34 2^32 = -1/4
    CHECK(sre == 0 && sim == 0 && suu == 0, "ties: %lld %lld %lld", sre, sim, suu);
    dpd_terms(0x1.8p-16f, 0.f, 0x1p-16f, 0.f, k.scale, &sre, &sim, &suu);           // 1.5 ties to 2; 2.25 to 2
    CHECK(sre == 2 && sim == 0 && suu == 2, "ties: %lld %lld %lld", sre, sim, suu);
    // the worst term of an eligible pair against the bound, for every table size and a full_scale just above a power of two (E = 2 full_scale)
    // and at one; then the guard: 2^28 such terms stay inside an int64
    for (uint32_t L = DPD_MIN_LOG2; L <= (uint32_t)DPD_MAX_LOG2; L++)
        for (float fs : { 1.f, 0.50000006f, 0.75f }) {
            c = good(); c.table_log2 = L; c.full_scale = fs;
            const DpdConsts w = dpd_consts(&c);
            const float E = (float)std::ldexp(1.0, w.e);
            float top = fs * (1.f + 0.5f / w.Kf);                       // the largest amplitude of bin K: walk up while it stays eligible
            int j;
            while (dpd_bin(std::nextafterf(top, inf), 0.f, 0.f, 0.f, w.inv_step, w.Kf, w.zmax2, &j)) top = std::nextafterf(top, inf);
            while (!dpd_bin(top, 0.f, 0.f, 0.f, w.inv_step, w.Kf, w.zmax2, &j)) top = std::nextafterf(top, 0.f);
            CHECK(j == (int)w.K, "the top of the table is bin %d", j);
            CHECK(dpd_bin(top, 0.f, 4.f * E, 0.f, w.inv_step, w.Kf, w.zmax2, &j), "4 E is eligible");
            dpd_terms(top, 0.f, 4.f * E, 0.f, w.scale, &sre, &sim, &suu);
            CHECK((double)sre <= dpd_term_bound(w.K) && (double)suu <= dpd_term_bound(w.K) && sre > (1ll << 33), "K %u, full_scale %g: %lld against %.1f",
                  w.K, fs, sre, dpd_term_bound(w.K));
            CHECK(dpd_term_bound(w.K) * (double)(1ull << DPD_GUARD_LOG2) < 9223372036854775807.0 / 1.5, "K %u: 2^28 terms overflow", w.K);
        }
    const uint64_t most = 1ull << DPD_GUARD_LOG2;
    const auto guard_ok = [](uint64_t since, uint64_t n) { return pd_guard_ok(since, n, DPD_GUARD_LOG2); };
    CHECK(guard_ok(0, most) && !guard_ok(0, most + 1) && guard_ok(most - 1, 1) && !guard_ok(most, 1) && guard_ok(most, 0)
          && !guard_ok(1, ~0ull) && !guard_ok(~0ull, 1), "the guard at its edge");
    CHECK(pd_guard_after_update(most, 0) == most && pd_guard_after_update(most, 2) == most / 4 && pd_guard_after_update(5, 2) == 2
          && pd_guard_after_update(1, 8) == 1 && pd_guard_after_update(0, 8) == 0 && pd_guard_after_update(257, 8) == 2, "the guard across an update");
    // grids and LDS
    CHECK(pd_pairs(0, 1) == 1 && pd_pairs(1, 1) == 1 && pd_pairs(0, 2) == 1 && pd_pairs(1, 2) == 2 && pd_pairs(1, 3) == 2, "pairs");
    CHECK(dpd_measure_grid(0, 1) == 1 && dpd_measure_grid(0, 512) == 1 && dpd_measure_grid(0, 513) == 2 && dpd_measure_grid(1, 512) == 2
          && dpd_measure_grid(0, 1048576) == 2048 && dpd_measure_grid(0, 1049089) == 2048 && dpd_measure_grid(1, 1ull << 32) == 2048, "measure grid");
    CHECK(pd_rounds(32) == 4 && pd_rounds(128) == 4 && pd_rounds(256) == 8 && pd_rounds(1024) == 32, "rounds");
    for (uint32_t L = DPD_MIN_LOG2; L <= (uint32_t)DPD_MAX_LOG2; L++) CHECK(pd_rounds(1u << L) % PD_UNROLL == 0, "rounds of K = 2^%u", L);
    CHECK(pd_stream_grid(0, 1, 1) == 1 && pd_stream_grid(1, 512, 1) == 2 && pd_stream_grid(0, 1049089, 1) == 2050 && pd_stream_grid(0, 1ull << 32, 1) == (1u << 23)
          && pd_stream_grid(1, 1ull << 32, 1) == (1u << 23) + 1, "copy grid");
    CHECK(pd_stream_grid(0, 1, 4) == 1 && pd_stream_grid(0, 2048, 4) == 1 && pd_stream_grid(1, 2048, 4) == 2 && pd_stream_grid(0, 2049, 4) == 2
          && pd_stream_grid(0, 1ull << 32, 32) == (1u << 18) && pd_stream_grid(1, 1ull << 32, 32) == (1u << 18) + 1, "apply grid");
    CHECK(pd_stream_lds(1024) == 16384 && dpd_measure_lds(1024) == 28700 && dpd_measure_lds(1024) < 29 * 1024 && dpd_measure_lds(32) == 924, "LDS");
    if (g_bad) { fprintf(stderr, "dpd_plan_test: %d failures\n", g_bad); return 1; }
    printf("dpd_plan_test ok\n");
    return 0;
}
