// acq_plan_test.cc -- the host-only parts of the receiver's launch path, checked without a GPU (tests/test_acq_plan.py):
//   1. csrc/acq_plan.hpp replayed over tests/golden/acq_plan_cases.txt: launch sequences (hint words that grow, reset and stall,
//      1 .. 512 channels, pushes of one tile .. 2^22 samples, every acquisition mode) with what the policy decided on each launch when
//      it still lived inside launch_sync -- recorded from that code, so every launch must match exactly -- plus the plan's invariants;
//   2. csrc/config_read.hpp against the rule of struct_size: a field that ends behind the caller's struct_size reads as 0.
//   acq_plan_test <cases file>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../csrc/acq_plan.hpp"
#include "../csrc/config_read.hpp"

using namespace mcrx;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_bad <= 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static int replay(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f) { perror(path); return 2; }
    char *rec = nullptr; size_t cap = 0;
    AcqPolicy p; AcqInputs in = {};
    unsigned nseq = 0, nlaunch = 0, lineno = 0;
    // one sequence per line, its records separated by ';': "S <the sequence's constants>" first, then one "L ..." per launch
    while (getline(&rec, &cap, f) > 0) {
        lineno++;
        if (rec[0] == '#' || rec[0] == '\n') continue;
        int have = 0, spec = 0;
        p = AcqPolicy();
        if (sscanf(rec, "S %u %u %u %d %d %d %u %u %d %d", &in.nch, &in.hist_tiles, &in.max_jobs, &in.acq_mode, &in.seg_walker, &in.lean_waves,
                   &p.nseg_fixed, &p.seg_frames, &have, &spec) != 10) { fprintf(stderr, "%s:%u: bad sequence record\n", path, lineno); return 2; }
        in.have_hints = have != 0; in.spec = spec != 0;
        nseq++;
        for (char *line = strchr(rec, ';'); line; line = strchr(line, ';')) {
            line += 2;
            unsigned long long buf = 0; uint32_t h[HINT_WORDS]; long long want[18]; int pos = 0, n = 0;
            if (sscanf(line, "L %llu%n", &buf, &pos) != 1) { fprintf(stderr, "%s:%u: bad launch record\n", path, lineno); return 2; }
            for (int i = 0; i < HINT_WORDS; i++) { if (sscanf(line + pos, "%u%n", &h[i], &n) != 1) return 2; pos += n; }
            n = -1; (void)sscanf(line + pos, " |%n", &n);
            if (n < 0) { fprintf(stderr, "%s:%u: no separator\n", path, lineno); return 2; }
            pos += n;
            for (int i = 0; i < 18; i++) { if (sscanf(line + pos, "%lld%n", &want[i], &n) != 1) { fprintf(stderr, "%s:%u: short launch line\n", path, lineno); return 2; } pos += n; }
            in.buf_samples = buf;
            const AcqPlan r = acq_plan(p, h, in);
            const long long got[18] = { r.nseg, r.spw, r.spec_cap, r.seg_jobs, r.spec_stride, r.nphase,
                                        r.nphase > 0 ? r.phase[0].seg_phase : 0, r.nphase > 0 ? (long long)r.phase[0].seg_jobs : 0,
                                        r.nphase > 1 ? r.phase[1].seg_phase : 0, r.nphase > 1 ? (long long)r.phase[1].seg_jobs : 0,
                                        r.grid_hint[0], r.grid_hint[1], r.grid_hint[2], r.frames_hint, r.enc_hint, r.want_k7, p.cadenced, p.anchor_kind };
            static const char *const name[18] = { "nseg", "spw", "spec_cap", "seg_jobs", "spec_stride", "nphase", "phase0", "jobs0", "phase1", "jobs1",
                                                  "grid_hint0", "grid_hint1", "grid_hint2", "frames_hint", "enc_hint", "want_k7", "cadenced", "anchor_kind" };
            for (int i = 0; i < 18; i++) CHECK(got[i] == want[i], "%s:%u: %s = %lld, recorded %lld", path, lineno, name[i], got[i], want[i]);
            nlaunch++;
            if (!in.spec) { CHECK(r.nseg == 0 && r.spec_cap == 0 && r.nphase == 0 && r.seg_jobs == 1, "%s:%u: a plan for segment waves without them", path, lineno); continue; }
            CHECK(r.nseg >= 1 && r.nseg <= MCRX_SEG_MAX, "%s:%u: nseg %u", path, lineno, r.nseg);
            CHECK(r.spec_cap <= r.spec_stride, "%s:%u: spec_cap %u > stride %u", path, lineno, r.spec_cap, r.spec_stride);
            CHECK(r.seg_jobs >= 1 && r.seg_jobs <= 32, "%s:%u: seg_jobs %u", path, lineno, r.seg_jobs);
            if ((uint64_t)in.nch * r.nseg <= in.max_jobs / 2)          // (room for one entry per wave at least)
                CHECK((uint64_t)in.nch * r.nseg * r.seg_jobs <= in.max_jobs / 2, "%s:%u: %u x %u x %u entries of %u", path, lineno, in.nch, r.nseg, r.seg_jobs, in.max_jobs);
            for (int i = 0; i < r.nphase; i++) CHECK(r.phase[i].seg_jobs >= 1 && r.phase[i].seg_jobs <= r.seg_jobs, "%s:%u: phase %d jobs", path, lineno, i);
        }
    }
    free(rec);
    fclose(f);
    CHECK(nseq >= 200 && nlaunch >= 1500, "%s: only %u sequences, %u launches", path, nseq, nlaunch);
    printf("acq_plan: %u sequences, %u launches replayed\n", nseq, nlaunch);
    return 0;
}

// ---- config_read.hpp
// Callers' structs with every field set, garbage behind them, and struct_size cut at every field boundary and inside every field.
// `fields` = how many leading fields (struct_size itself included) the handle may see: those that lie whole inside struct_size.
#define CUT_AT(T, field, fields_before) { offsetof(T, field), fields_before }, { offsetof(T, field) + 2, fields_before }
struct Cut { size_t struct_size; unsigned fields; };
static const unsigned NF = sizeof(mcrx_hip_config) / sizeof(uint32_t), NFM = sizeof(mcrx_hip_monitor_config) / sizeof(uint32_t);
static const Cut k_cuts[] = {
    { 4, 1 },
    CUT_AT(mcrx_hip_config, struct_size, 0), CUT_AT(mcrx_hip_config, max_payload_len, 1), CUT_AT(mcrx_hip_config, max_frames, 2),
    CUT_AT(mcrx_hip_config, payload_soft, 3), CUT_AT(mcrx_hip_config, slab_blocks, 4), CUT_AT(mcrx_hip_config, channel_first, 5),
    CUT_AT(mcrx_hip_config, channel_count, 6), CUT_AT(mcrx_hip_config, batch_samples, 7), CUT_AT(mcrx_hip_config, single_channel, 8),
    CUT_AT(mcrx_hip_config, serial, 9), CUT_AT(mcrx_hip_config, chunk_blocks, 10), CUT_AT(mcrx_hip_config, defer_samples, 11),
    CUT_AT(mcrx_hip_config, front_end, 12), CUT_AT(mcrx_hip_config, skip_framesyms, 13), CUT_AT(mcrx_hip_config, worker_build, 14),
    CUT_AT(mcrx_hip_config, acquisition, 15), CUT_AT(mcrx_hip_config, scout_build, 16), CUT_AT(mcrx_hip_config, conv_scratch, 17),
    CUT_AT(mcrx_hip_config, input_format, 18),
    { sizeof(mcrx_hip_config), 19 }, { sizeof(mcrx_hip_config) + 64, 19 },
};
static const Cut k_mon_cuts[] = {
    { 4, 1 },
    CUT_AT(mcrx_hip_monitor_config, struct_size, 0), CUT_AT(mcrx_hip_monitor_config, nfft, 1), CUT_AT(mcrx_hip_monitor_config, window, 2),
    { sizeof(mcrx_hip_monitor_config), 3 }, { sizeof(mcrx_hip_monitor_config) + 64, 3 },
};

template <class C, class F> static void check_cuts(const char *what, const Cut *cuts, size_t ncuts, unsigned nf, unsigned legacy_fields, F effective)
{
    uint32_t caller[64], got[64];
    for (size_t k = 0; k < ncuts; k++) {
        for (unsigned i = 0; i < 64; i++) caller[i] = 0xA5000000u + i;
        caller[0] = (uint32_t)cuts[k].struct_size;
        // struct_size == 0 is the one cut with a meaning of its own: the caller predates the field's use (legacy_fields of it are read)
        const unsigned fields = cuts[k].struct_size == 0 ? legacy_fields : cuts[k].fields;
        const C e = effective(reinterpret_cast<const C *>(caller));
        memcpy(got, &e, sizeof(e));
        for (unsigned i = 0; i < nf; i++)
            CHECK(got[i] == (i < fields ? caller[i] : 0u), "%s, struct_size %zu: field %u reads %#x", what, cuts[k].struct_size, i, got[i]);
    }
}

static void check_config()
{
    static_assert(sizeof(mcrx_hip_config) == 19 * sizeof(uint32_t) && sizeof(mcrx_hip_monitor_config) == 3 * sizeof(uint32_t), "a new field: add its cut to the tables");
    // struct_size == 0: the fields up to and including batch_samples (8 with struct_size itself), every later one 0
    check_cuts<mcrx_hip_config>("mcrx_hip_config", k_cuts, sizeof(k_cuts) / sizeof(k_cuts[0]), NF, 8, effective_config);
    check_cuts<mcrx_hip_monitor_config>("mcrx_hip_monitor_config", k_mon_cuts, sizeof(k_mon_cuts) / sizeof(k_mon_cuts[0]), NFM, 0, effective_monitor_config);
    // NULL: the defaults, with soft decisions
    mcrx_hip_config want{}; want.payload_soft = 1;
    const mcrx_hip_config e = effective_config(nullptr);
    CHECK(memcmp(&e, &want, sizeof(e)) == 0, "NULL config");
    const mcrx_hip_monitor_config m = effective_monitor_config(nullptr);
    CHECK(m.struct_size == 0 && m.nfft == 0 && m.window == 0, "NULL monitor config");
    printf("config_read: %zu + %zu cuts\n", sizeof(k_cuts) / sizeof(k_cuts[0]), sizeof(k_mon_cuts) / sizeof(k_mon_cuts[0]));
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s cases-file\n", argv[0]); return 2; }
    const int rc = replay(argv[1]);
    if (rc) return rc;
    check_config();
    if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
    printf("ok\n");
    return 0;
}
