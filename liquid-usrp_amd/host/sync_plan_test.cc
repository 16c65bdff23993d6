// sync_plan_test.cc -- which kernel, grid, block and LDS a synchronizer launch gets, checked without a GPU (tests/test_sync_plan.py):
//   1. csrc/sync_plan.hpp replayed over tests/golden/sync_plan_cases.txt: what the launchers at the end of csrc/ofdmsync.hip issued
//      while the decisions still lived between their hipLaunchKernelGGL calls -- recorded from that code, so every field must match;
//   2. what that code promises about grids, LDS sizes and the rewritten SyncArgs fields, for every case.
//   sync_plan_test <cases file>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "../csrc/sync_plan.hpp"

using namespace mcrx;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_bad <= 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

// the launch target's name as the recorded code wrote it (without "_kernel")
static std::string kernel_name(SyncKernel k)
{
    static const char *const width[5] = { "1", "2", "4", "8", "16" };
    static const struct { SyncKernel first; int n; const char *pre, *post; } fam[] = {
        { SK_SYNC_E1, 5, "sync<", ">" }, { SK_SPEC_E1, 5, "sync_spec<", ">" }, { SK_PAYLOAD_FAST_E1, 5, "payload<", ",true>" },
        { SK_PAYLOAD_GENERAL_E1, 5, "payload<", ",false>" }, { SK_TAIL_E1, 2, "sync_tail<", ">" }, { SK_LEAN_E1, 2, "sync_lean<", ">" }, { SK_WALK_E1, 2, "sync_walk<", ">" } };
    for (const auto &f : fam) if (sync_kernel_in(k, f.first, f.n)) return std::string(f.pre) + width[k - f.first] + f.post;
    switch (k) {
    case SK_ACQ_LEAN_M48: return "acq_lean<63,48>";
    case SK_ACQ_LEAN_M64: return "acq_lean<63,64>";
    case SK_MULTI_1: return "payload_multi<1>";
    case SK_MULTI_2: return "payload_multi<2>";
    case SK_MULTI_4: return "payload_multi<4>";
    case SK_PLEAN_XB0: return "payload_lean<0>";
    case SK_PLEAN_XB63: return "payload_lean<63>";
    case SK_PLEAN_M48: return "payload_lean<63,48>";
    case SK_PLEAN_REST_XB0: return "payload_lean_rest<0>";
    case SK_PLEAN_REST_XB63: return "payload_lean_rest<63>";
    case SK_PLEAN_REST_M48: return "payload_lean_rest<63,48>";
    case SK_WIDE_E2: return "payload_wide<63,2>";
    case SK_WIDE_E4: return "payload_wide<63,4>";
    case SK_PLACE: return "place_jobs";
    case SK_DECODE: return "decode";
    case SK_DECODE_GENERAL: return "decode_general";
    default: return "?";
    }
}
static std::string launches(const SyncLaunch *l, int n)
{
    std::string s = std::to_string(n);
    for (int i = 0; i < n; i++) s += " " + kernel_name(l[i].k) + " " + std::to_string(l[i].grid) + " " + std::to_string(l[i].block) + " " + std::to_string(l[i].lds);
    return s;
}
static int result_code(SyncStatus s) { return s == SYNC_INVALID ? 1 : 0; }        // (hipErrorInvalidValue = 1)
static unsigned g_seen[SK_COUNT];

// promises common to every launch: a grid, and the decoder's block scratch right behind the kernel's own LDS
static void check_launch(const SyncLaunch &l, uint32_t vit_off, const char *path, unsigned ln)
{
    g_seen[l.k]++;
    CHECK(l.grid >= 1 && l.block >= 1, "%s:%u: grid %u, block %u", path, ln, l.grid, l.block);
    if (sync_kernel_decodes(l.k)) CHECK(vit_off && vit_off % 16 == 0 && l.lds == vit_off + 8 * (size_t)VIT_B, "%s:%u: vit_off %u, lds %zu", path, ln, vit_off, l.lds);
    else CHECK(vit_off == 0, "%s:%u: vit_off %u for a kernel that does not decode", path, ln, vit_off);
}

static std::string replay_acq(const char *rest, const SyncDesign &d, const char *path, unsigned ln)
{
    static const char *const names[5] = { "scout", "lean", "walk", "tail", "spec" };
    char what[16]; SyncAcqInputs in = {}; in.d = d; int w = 0;
    if (sscanf(rest, "%15s %u %d %u %d %u", what, &in.nch, &in.seg_phase, &in.nseg, &in.seg_walker, &in.spec_cap) != 6) return "?";
    while (w < 5 && strcmp(what, names[w])) w++;
    if (w == 5) return "?";
    const SyncAcqPlan p = sync_acq_plan((SyncAcq)w, in);
    const int n = p.status == SYNC_LAUNCH ? 1 : 0;
    std::string got = std::to_string(result_code(p.status)) + " " + launches(&p.l, n);
    if (n) { got += " | " + std::to_string(p.vit_off); check_launch(p.l, p.vit_off, path, ln); }
    return got;
}

// what the payload stage's code promises (kernels.h: SyncArgs::live_off, split_rest; the grids' comments in sync_plan.hpp)
static void check_payload(const SyncPayloadInputs &in, SyncStage stage, const SyncPayloadPlan &p, const char *path, unsigned ln)
{
    const bool launched = p.status == SYNC_LAUNCH;
    CHECK(launched ? p.n >= 1 && p.n <= 2 : p.n == 0, "%s:%u: %d launches", path, ln, p.n);
    if (!launched) return;
    for (int i = 0; i < p.n; i++) {
        const SyncLaunch &l = p.l[i];
        check_launch(l, sync_kernel_decodes(l.k) ? p.vit_off : 0, path, ln);
        // A worker or decoder grid is at most the job list -- where the job list is not shorter than the floor of a list-driven launch
        // (SY_REST_FLOOR, SY_GEN_FLOOR: the recorded code applies them before it looks at max_jobs; a receiver's list has >= 1024 entries)
        const bool rest = sync_kernel_in(l.k, SK_PLEAN_REST_XB0, 3);
        const unsigned most = rest && in.max_jobs < SY_REST_FLOOR ? SY_REST_FLOOR : l.k == SK_DECODE_GENERAL && in.max_jobs < SY_GEN_FLOOR ? SY_GEN_FLOOR : in.max_jobs;
        if (l.k != SK_PLACE) CHECK(l.grid <= most, "%s:%u: grid %u, %u jobs", path, ln, l.grid, in.max_jobs);
        if (l.k == SK_DECODE_GENERAL && in.have_vit_scratch) CHECK(l.grid <= in.vit_waves, "%s:%u: grid %u, scratch for %u waves", path, ln, l.grid, in.vit_waves);
        if (l.k == SK_DECODE) CHECK(l.lds == 2 * (size_t)p.soft_lds + p.msg_lds + 16 && p.soft_lds >= 4096 && p.soft_lds <= 56 * 1024 && p.soft_lds == p.dec_lds_soft && l.block == DK_T,
                                    "%s:%u: decode LDS %zu, soft %u, message %u", path, ln, l.lds, p.soft_lds, p.msg_lds);
    }
    CHECK(p.vit_off == 0 || sync_kernel_decodes(p.l[0].k), "%s:%u: vit_off %u", path, ln, p.vit_off);
    CHECK(p.live_off <= in.max_jobs, "%s:%u: live_off %u, %u jobs", path, ln, p.live_off, in.max_jobs);
    CHECK((p.live_off != 0) == sync_payload_splits(in), "%s:%u: live_off %u, splits %d", path, ln, p.live_off, (int)sync_payload_splits(in));
    if (stage == SYNC_BEHIND) CHECK(p.live_off != 0, "%s:%u: a launch behind workers that do not split", path, ln);
    if (!p.live_off) CHECK(p.split_rest == 0 && p.dec_phase == 0, "%s:%u: split_rest %d, dec_phase %d without a split", path, ln, p.split_rest, p.dec_phase);
}

static std::string replay_payload(const char *rest, const SyncDesign &d, const char *path, unsigned ln)
{
    static const char *const names[5] = { "place", "workers", "decode", "general", "behind" };
    SyncPayloadInputs in = {};
    in.d = d; in.nch = 8; in.scout = 1; in.max_jobs = 4096; in.payload_fr = 1; in.payload_lean = 1; in.payload_xb = 63; in.frames_hint = in.grid_hint0 = ~0u;
    in.have_qam_list = true; in.vit_waves = 2048;
    char st[16], tok[64]; int pos = 0, n = 0, stage = 0;
    if (sscanf(rest, "%15s%n", st, &pos) != 1) return "?";
    while (stage < 5 && strcmp(st, names[stage])) stage++;
    if (stage == 5) return "?";
    while (sscanf(rest + pos, "%63s%n", tok, &n) == 1) {
        pos += n;
        char *eq = strchr(tok, '=');
        if (!eq) return "?";
        *eq = 0;
        const uint32_t v = (uint32_t)strtol(eq + 1, nullptr, 10);
        struct { const char *name; uint32_t *u; int *i; bool *b; } f[] = {
            { "nch", &in.nch }, { "scout", nullptr, &in.scout }, { "mj", &in.max_jobs }, { "nf", nullptr, &in.no_fast }, { "fr", nullptr, &in.payload_fr },
            { "lean", nullptr, &in.payload_lean }, { "xb", nullptr, &in.payload_xb }, { "fh", &in.frames_hint }, { "gh0", &in.grid_hint0 }, { "qam", nullptr, nullptr, &in.have_qam_list },
            { "gh2", &in.grid_hint2 }, { "vit", nullptr, nullptr, &in.have_vit_scratch }, { "vw", &in.vit_waves }, { "enc", &in.enc_hint }, { "pad", &in.payload_lds_pad },
            { "sr", nullptr, &in.split_rest }, { "dp", nullptr, &in.dec_phase } };
        size_t i = 0;
        for (; i < sizeof(f) / sizeof(f[0]) && strcmp(tok, f[i].name); i++) {}
        if (i == sizeof(f) / sizeof(f[0])) return "?";
        if (f[i].u) *f[i].u = v; else if (f[i].i) *f[i].i = (int)v; else *f[i].b = v != 0;
    }
    const SyncPayloadPlan p = sync_payload_plan(in, (SyncStage)stage);
    check_payload(in, (SyncStage)stage, p, path, ln);
    std::string got = std::to_string((int)sync_payload_splits(in)) + " " + std::to_string(result_code(p.status)) + " " + launches(p.l, p.n);
    if (p.n) {
        char buf[160];
        snprintf(buf, sizeof(buf), " | %u %u | %u %d %d %u %d %u", p.soft_lds, p.msg_lds, p.live_off, p.split_rest, p.dec_phase, p.dec_lds_soft, (int)p.clear_gen_list, p.vit_off);
        got += buf;
    }
    return got;
}

static int replay(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f) { perror(path); return 2; }
    char *line = nullptr; size_t cap = 0;
    unsigned ln = 0, nacq = 0, npay = 0;
    SyncDesign d = {};
    while (getline(&line, &cap, f) > 0) {
        ln++;
        if (line[0] == '#' || line[0] == '\n') continue;
        line[strcspn(line, "\n")] = 0;
        if (line[0] == 'D') {       // the design of the cases that follow
            if (sscanf(line, "D %d %d %d %d %d %u %u", &d.M, &d.E, &d.log2M, &d.M_pilot, &d.Nen, &d.max_enc_len, &d.max_payload_len) != 7) { fprintf(stderr, "%s:%u: bad design record\n", path, ln); return 2; }
            continue;
        }
        char *arrow = strstr(line, " => ");
        if (!arrow || (line[0] != 'A' && line[0] != 'P') || line[1] != ' ') { fprintf(stderr, "%s:%u: bad case record\n", path, ln); return 2; }
        *arrow = 0;
        const char *want = arrow + 4;
        const std::string got = line[0] == 'A' ? replay_acq(line + 2, d, path, ln) : replay_payload(line + 2, d, path, ln);
        if (got == "?") { fprintf(stderr, "%s:%u: bad case record\n", path, ln); return 2; }
        CHECK(got == want, "%s:%u: %s\n  plan     %s\n  recorded %s", path, ln, line, got.c_str(), want);
        if (line[0] == 'A') nacq++; else npay++;
    }
    free(line);
    fclose(f);
    for (int k = SK_NONE + 1; k < SK_COUNT; k++) CHECK(g_seen[k] >= 2, "%s: %s launched by %u cases", path, kernel_name((SyncKernel)k).c_str(), g_seen[k]);
    CHECK(nacq >= 300 && npay >= 1000, "%s: only %u + %u cases", path, nacq, npay);
    printf("sync_plan: %u acquisition and %u payload cases replayed, %d launch targets\n", nacq, npay, SK_COUNT - 1);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s cases-file\n", argv[0]); return 2; }
    const int rc = replay(argv[1]);
    if (rc) return rc;
    if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
    printf("ok\n");
    return 0;
}
