// rx_plan_test.cc -- the sizes a receiver handle is created with, checked without a GPU (tests/test_rx_plan.py):
//   1. csrc/rx_plan.hpp replayed over tests/golden/rx_plan_cases.txt: what mcrx_hip_create derived from its arguments while the
//      arithmetic still lived in its body -- recorded from that code, so every field, code and message must match exactly;
//   2. what the code's comments promise about those sizes, for every accepted case of ordinary limits.
//   rx_plan_test <cases file>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include "../csrc/design.hpp"
#include "../csrc/rx_plan.hpp"

using namespace mcrx;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_bad <= 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

// OfdmDesign::init's carrier counts, once per design (0, 0: the allocation is refused, as mcrx_hip_create refuses it in front of the plan)
static void design_counts(unsigned M, unsigned cp, unsigned taper, const char *p, unsigned *M_data, unsigned *M_pilot)
{
    static std::map<std::string, std::pair<unsigned, unsigned>> seen;
    const std::string key = std::to_string(M) + " " + std::to_string(cp) + " " + std::to_string(taper) + " " + p;
    auto it = seen.find(key);
    if (it == seen.end()) {
        std::string a(p);
        for (char &c : a) c = (char)(c - '0');
        OfdmDesign od;
        const bool ok = od.init(M, cp, taper, strcmp(p, "-") ? reinterpret_cast<const unsigned char *>(a.data()) : nullptr) == 0;
        it = seen.emplace(key, std::make_pair(ok ? od.M_data : 0u, ok ? od.M_pilot : 0u)).first;
    }
    *M_data = it->second.first; *M_pilot = it->second.second;
}

// the promises of the comments in rx_plan.hpp and kernels.h, held for max_frames <= 2^22 and max_payload_len <= 8192 (the caller filters)
static void check_promises(const RxInputs &in, const RxPlan &r, const char *path, unsigned ln)
{
    CHECK(r.max_enc >= 256 && r.max_enc % 16 == 0, "%s:%u: max_enc %u", path, ln, r.max_enc);
    CHECK(128ull * ((4ull * r.max_enc + 6 + 959) / 960) <= r.max_enc + 16ull, "%s:%u: a scratch row of %u + 16 bytes does not hold the soft decoder's checkpoints", path, ln, r.max_enc);
    CHECK(r.nch >= 1 && (uint64_t)r.ch_first + r.nch <= in.N && r.max_rec >= 1, "%s:%u: shard %u + %u of %u, %u records", path, ln, r.ch_first, r.nch, in.N, r.max_rec);
    const uint64_t pay16 = ((uint64_t)r.max_payload + 15) & ~15ull;
    CHECK(r.arena_cap / pay16 == r.max_rec && r.arena_cap % pay16 == 0, "%s:%u: arena_cap %llu for %u records of %llu bytes", path, ln, (unsigned long long)r.arena_cap, r.max_rec, (unsigned long long)pay16);
    CHECK(r.sarena_cap <= (8ull << 30), "%s:%u: sarena_cap %llu", path, ln, (unsigned long long)r.sarena_cap);
    // (without scouts -- MCRX_NO_SCOUT in a development build, e.g. N = 8, M = 64 -- there is no job list: max_jobs stays 0, as in the recorded code)
    if (r.scout) CHECK(r.max_jobs == 2ull * r.max_rec + 4ull * r.nch + 1024, "%s:%u: max_jobs %u", path, ln, r.max_jobs);
    CHECK(r.nslots >= 2 && r.nslots <= MCRX_SLOTS, "%s:%u: nslots %u", path, ln, r.nslots);
    CHECK(r.stage_cap > 0 && r.stage_cap % ((size_t)MCRX_TILE * r.K) == 0, "%s:%u: stage_cap %zu, K %u", path, ln, r.stage_cap, r.K);
    CHECK((uint64_t)r.hist_tiles * MCRX_TILE >= r.defer + in.M + in.cp + 8, "%s:%u: %u tiles of history", path, ln, r.hist_tiles);
    CHECK(!r.spec || r.lean, "%s:%u: speculation on a design that is not lean", path, ln);
}

static int replay(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f) { perror(path); return 2; }
    char *line = nullptr; size_t cap = 0;
    unsigned ln = 0, nok = 0, nerr = 0;
    std::map<std::string, unsigned> refusals;
    while (getline(&line, &cap, f) > 0) {
        ln++;
        if (line[0] == '#' || line[0] == '\n') continue;
        line[strcspn(line, "\n")] = 0;
        RxInputs in = {};
        in.ec.struct_size = sizeof(in.ec); in.ec.payload_soft = 1;
        char p[1100], tok[96], dv[11][32]; int pos = 0, n = 0; unsigned md = 0, mp = 0;
        bool ok = sscanf(line, "C %u %u %u %u %1099s |%n", &in.N, &in.M, &in.cp, &in.taper, p, &pos) == 5 && pos > 0;
        // name=value lists up to the next '|': the configuration's fields (32-bit words, in the struct's order), then the switches
        static const char *const cf[] = { "struct_size", "max_payload_len", "max_frames", "payload_soft", "slab_blocks", "channel_first", "channel_count",
                                          "batch_samples", "single_channel", "serial", "chunk_blocks", "defer_samples", "front_end", "skip_framesyms",
                                          "worker_build", "acquisition", "scout_build", "conv_scratch", "input_format" };
        static const char *const df[11] = { "serial", "slots", "no_scout", "no_spec", "payload_fr", "payload_lean", "payload_xb", "acq_mode", "lean_build",
                                            "walk_lds_pad", "payload_lds_pad" };
        static_assert(sizeof(cf) / sizeof(cf[0]) == sizeof(mcrx_hip_config) / sizeof(uint32_t), "a new field: add its name");
        const char **dst[11] = { &in.devel.serial, &in.devel.slots, &in.devel.no_scout, &in.devel.no_spec, &in.devel.payload_fr, &in.devel.payload_lean,
                                 &in.devel.payload_xb, &in.devel.acq_mode, &in.devel.lean_build, &in.devel.walk_lds_pad, &in.devel.payload_lds_pad };
        for (int list = 0; ok && list < 2; list++)
            while ((ok = sscanf(line + pos, "%95s%n", tok, &n) == 1)) {
                pos += n;
                if (!strcmp(tok, "|")) break;
                if (!strcmp(tok, "-")) continue;
                char *eq = strchr(tok, '='); size_t i = 0;
                if ((ok = eq != nullptr)) *eq = 0; else break;
                if (list == 0) {
                    for (; i < sizeof(cf) / sizeof(cf[0]) && strcmp(tok, cf[i]); i++) {}
                    if ((ok = i < sizeof(cf) / sizeof(cf[0]))) reinterpret_cast<uint32_t *>(&in.ec)[i] = (uint32_t)strtoul(eq + 1, nullptr, 10); else break;
                } else {
                    for (; i < 11 && strcmp(tok, df[i]); i++) {}
                    if ((ok = i < 11 && strlen(eq + 1) < sizeof(dv[0]))) *dst[i] = strcpy(dv[i], eq + 1); else break;
                }
            }
        if (ok) { n = -1; (void)sscanf(line + pos, " %u %u => %n", &md, &mp, &n); ok = n > 0; pos += n; }
        if (!ok) { fprintf(stderr, "%s:%u: bad case record\n", path, ln); return 2; }
        design_counts(in.M, in.cp, in.taper, p, &in.M_data, &in.M_pilot);
        CHECK(in.M_data == md && in.M_pilot == mp, "%s:%u: the design has %u data and %u pilot carriers, recorded %u and %u", path, ln, in.M_data, in.M_pilot, md, mp);
        RxPlan r; const char *why = "";
        const int rc = in.M_data ? rx_plan(in, &r, &why) : MCRX_EINVAL;
        if (!in.M_data) why = "invalid subcarrier allocation";
        const char *want = line + pos;
        char got[1024];
        if (rc != MCRX_OK) snprintf(got, sizeof(got), "ERR %d %s", rc, why);
        else {
            int k = snprintf(got, sizeof(got), "OK %u %u %u %u %u %u %u %llu %llu %llu %u %d %u %u %u %d %zu %zu %d", r.K, r.max_payload, r.max_enc, r.max_syms,
                             r.ch_first, r.nch, r.max_rec, (unsigned long long)r.min_frame, (unsigned long long)r.arena_cap, (unsigned long long)r.sarena_cap,
                             r.hist_tiles, (int)r.spec, r.max_jobs, r.vit_rows, r.vit_waves, (int)r.lean, r.stage_cap, r.hist_bytes, (int)r.side_stream);
            // ... and, by name, every other field that is not what a default-constructed plan holds
            const RxPlan d;
#define NAMED(f) if ((long long)r.f != (long long)d.f) k += snprintf(got + k, sizeof(got) - (size_t)k, " " #f "=%lld", (long long)r.f)
            NAMED(bypass); NAMED(in_fmt); NAMED(ss); NAMED(pipelined); NAMED(slab_blocks); NAMED(oversampled); NAMED(chan_P); NAMED(hist_blocks);
            NAMED(col_shift); NAMED(defer); NAMED(payload_xb); NAMED(payload_lean); NAMED(payload_fr); NAMED(acq_mode); NAMED(lean_build);
            NAMED(seg_walker); NAMED(scout); NAMED(round_lds_pad); NAMED(walk_lds_pad); NAMED(nslots); NAMED(vit_mode);
#undef NAMED
        }
        CHECK(strcmp(got, want) == 0, "%s:%u:\n  plan     %s\n  recorded %s", path, ln, got, want);
        if (rc != MCRX_OK) { nerr++; refusals[why]++; continue; }
        nok++;
        if (in.ec.max_frames <= (1u << 22) && in.ec.max_payload_len <= 8192) check_promises(in, r, path, ln);
    }
    free(line);
    fclose(f);
    // every refusal of the plan (and the allocation's in front of it), each more than once
    static const char *const all[] = { "invalid subcarrier allocation", "channel shard outside [0, N)", "front_end must be 0, 1 or 2",
                                       "the oversampled front end needs a power-of-two channel count <= 512", "worker_build / acquisition out of range",
                                       "scout_build out of range", "conv_scratch must be 0, 1 or 2" };
    for (const char *m : all) CHECK(refusals[m] >= 2, "%s: refusal \"%s\" replayed %u times", path, m, refusals[m]);
    CHECK(nok >= 300, "%s: only %u accepted cases", path, nok);
    printf("rx_plan: %u accepted and %u refused cases replayed\n", nok, nerr);
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
