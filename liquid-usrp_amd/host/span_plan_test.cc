// span_plan_test.cc -- csrc/span_plan.hpp with a main of its own (host compiler only, no HIP): replays tests/golden/span_plan_cases.txt,
// recorded from the three loops of chanemu.hip, rfchain.hip and userchan.hip while each still held this arithmetic between its launch
// calls, and holds every case to what the plan promises (tests/test_span_plan.py).
//
// A case: form L table_cap have pos n  cap alloc nspans hash listed, then `listed` spans (m row0 rows) from the first on, then the last.
// form c / r: uint64_t positions that wrap; s: userchan's long long block index (granules of 8).  alloc: the rows asked for, 0 when the
// `have` allocated suffice; hash: FNV-1a over (m, row0, rows) of every span.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../csrc/span_plan.hpp"

using namespace mcrx;

static int g_line = 0;
#define EXPECT(c) do { if (!(c)) { printf("line %d: %s fails (%s:%d)\n", g_line, #c, __FILE__, __LINE__); return false; } } while (0)

static uint64_t fnv(uint64_t h, uint64_t v) { for (int i = 0; i < 8; i++) { h ^= (v >> (8 * i)) & 0xff; h *= 0x100000001b3ull; } return h; }

struct Want { uint64_t m, row0, rows; };

// P: the position's type; the spans as an execute loop walks them
template <typename P> static bool replay(P pos, uint64_t n, uint32_t L, uint64_t table_cap, uint64_t have, bool granules, uint64_t cap_w, uint64_t alloc_w,
                                         uint64_t nspans_w, uint64_t hash_w, const Want *first, int listed, Want last)
{
    const uint64_t mask = ((uint64_t)1 << L) - 1, rowmask = ~(uint64_t)0 >> L;
    const uint64_t cap = span_cap(span_rows(span_frac(pos, L), n, L), table_cap);
    EXPECT(cap == cap_w);
    EXPECT((cap > have ? span_grow(have, table_cap, cap) : 0) == alloc_w);
    EXPECT(alloc_w == 0 || (alloc_w >= cap && alloc_w <= (table_cap > cap ? table_cap : cap) && alloc_w > have));
    EXPECT(cap >= 2);
    uint64_t nspans = 0, hash = 0xcbf29ce484222325ull, done = 0;
    Span<P> s = {};
    while (done < n) {
        const P at = (P)((uint64_t)pos + done);                         // the spans tile [pos, pos + n): each starts where the last ended
        s = span_next(at, n - done, L, cap);
        EXPECT(s.m >= 1 && s.m <= n - done);                            // progress, and never past the call
        EXPECT(s.rows >= 2 && s.rows <= cap);
        EXPECT(s.frac == ((uint64_t)at & mask));
        const uint64_t row_first = (uint64_t)at >> L, row_last = ((uint64_t)at + (s.m - 1)) >> L;
        EXPECT((((uint64_t)s.row0) & rowmask) == row_first);            // the table starts at the first sample's grid row
        EXPECT(((row_last - row_first) & rowmask) + 1 < s.rows);        // the last sample's row and the one behind it lie inside
        EXPECT(((row_last - row_first) & rowmask) + 2 == s.rows);       // and no row is computed for nothing
        if (done + s.m < n) EXPECT((((uint64_t)at + s.m) & mask) == 0);   // every span but the last ends on a grid row
        if (granules) EXPECT(s.m % 8 == 0);
        if (nspans < (uint64_t)listed) EXPECT(s.m == first[nspans].m && (uint64_t)s.row0 == first[nspans].row0 && s.rows == first[nspans].rows);
        hash = fnv(fnv(fnv(hash, s.m), (uint64_t)s.row0), s.rows);
        done += s.m; nspans++;
    }
    EXPECT(done == n && nspans == nspans_w && hash == hash_w);
    EXPECT(s.m == last.m && (uint64_t)s.row0 == last.row0 && s.rows == last.rows);
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: span_plan_test tests/golden/span_plan_cases.txt\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    // the signed form is an arithmetic shift: block -1 lies in grid row -1
    if (span_next((long long)-1, 1, 3, 2).row0 != -1 || span_next(~(uint64_t)0, 1, 3, 2).row0 != (~(uint64_t)0 >> 3)) { printf("row0 of the two forms\n"); return 1; }
    char line[1024];
    int cases[3] = { 0, 0, 0 };
    while (fgets(line, sizeof line, f)) {
        g_line++;
        if (line[0] == '#' || line[0] == '\n') continue;
        char form; unsigned L; unsigned long long tcap, have, n, cap, alloc, nspans, hash; char pos_s[32]; int listed, used = 0;
        if (sscanf(line, " %c %u %llu %llu %31s %llu %llu %llu %llu %llx %d%n", &form, &L, &tcap, &have, pos_s, &n, &cap, &alloc, &nspans, &hash, &listed, &used) != 11
            || listed < 0 || listed > 6) { printf("line %d: malformed\n", g_line); return 1; }
        Want w[7];
        const char *p = line + used;
        for (int i = 0; i <= listed; i++) {
            char r0[32]; unsigned long long m, rows; int k = 0;
            if (sscanf(p, " %llu %31s %llu%n", &m, r0, &rows, &k) != 3) { printf("line %d: malformed span\n", g_line); return 1; }
            w[i].m = m; w[i].rows = rows;
            w[i].row0 = form == 's' ? (uint64_t)strtoll(r0, nullptr, 10) : (uint64_t)strtoull(r0, nullptr, 10);
            p += k;
        }
        bool ok;
        if (form == 's') {
            const long long pos = strtoll(pos_s, nullptr, 10);
            ok = replay<long long>(pos, n, L, tcap, have, pos % 8 == 0 && n % 8 == 0 && L >= 3, cap, alloc, nspans, hash, w, listed, w[listed]);
        } else if (form == 'c' || form == 'r') {
            ok = replay<uint64_t>(strtoull(pos_s, nullptr, 10), n, L, tcap, have, false, cap, alloc, nspans, hash, w, listed, w[listed]);
        } else { printf("line %d: unknown form\n", g_line); return 1; }
        if (!ok) return 1;
        cases[form == 'c' ? 0 : form == 'r' ? 1 : 2]++;
    }
    fclose(f);
    if (!cases[0] || !cases[1] || !cases[2]) { printf("a form has no case\n"); return 1; }
    printf("%d chanemu, %d rfchain, %d userchan cases replayed\nspan_plan_test ok\n", cases[0], cases[1], cases[2]);
    return 0;
}
