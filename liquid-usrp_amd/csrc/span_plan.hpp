// span_plan.hpp -- the spans of a block-rate table, pure: which rows of a table sampled every 2^L positions a run of positions reads, how
// many rows the handle's table gets, and how a call is cut into spans that fit it.  Host code, no HIP: chanemu.hip (fading gains),
// rfchain.hip (the oscillator's phase) and userchan.hip (the users' fading gains) plan with it; host/span_plan_test.cc replays
// tests/golden/span_plan_cases.txt through it (tests/test_span_plan.py).
//
// A position p reads grid rows p >> L and (p >> L) + 1 and interpolates by frac = p & (2^L - 1).  A span's table starts at the grid row of
// the span's first position, so a table of `cap` rows serves ((cap - 1) << L) - frac positions; a span ends there (on a grid row) or with
// the call.  Positions are uint64_t sample indices that wrap (chanemu, rfchain) or long long block indices that may be negative
// (userchan): the grid row of the first is pos >> L of the unsigned value, of the second the arithmetic shift; the fraction is the
// low bits of the two's complement value for both.
#pragma once
#include <stdint.h>

namespace mcrx {

inline uint64_t span_frac(uint64_t pos, uint32_t L) { return pos & (((uint64_t)1 << L) - 1); }
inline uint64_t span_frac(long long pos, uint32_t L) { return (uint64_t)pos & (((uint64_t)1 << L) - 1); }

// rows the n >= 1 positions behind fraction `frac` of a grid interval read: their own grid rows and the one behind the last
inline uint64_t span_rows(uint64_t frac, uint64_t n, uint32_t L) { return ((frac + n - 1) >> L) + 2; }

// rows a span of this call may use: what the whole call reads, or the table's cap
inline uint64_t span_cap(uint64_t want, uint64_t table_cap) { return want < table_cap ? want : table_cap; }

// rows to allocate when `cap` exceeds the `have` allocated: twice as many, within the table's cap, and at least cap
inline uint64_t span_grow(uint64_t have, uint64_t table_cap, uint64_t cap)
{
    const uint64_t twice = 2 * have < table_cap ? 2 * have : table_cap;
    return twice > cap ? twice : cap;
}

// One span: m positions from pos on; its table holds `rows` rows from grid row row0 on; frac = the fraction of pos.  P is the
// position's own type, and row0 keeps it.
template <typename P> struct Span { uint64_t m; P row0; uint64_t rows, frac; };

// the span at pos of a call with `left` >= 1 positions to go, on a table of cap >= 2 rows (m >= 1 then)
template <typename P> inline Span<P> span_next(P pos, uint64_t left, uint32_t L, uint64_t cap)
{
    Span<P> s;
    s.frac = span_frac(pos, L);
    const uint64_t avail = ((cap - 1) << L) - s.frac;
    s.m = left < avail ? left : avail;
    s.row0 = pos >> L;
    s.rows = span_rows(s.frac, s.m, L);
    return s;
}

}  // namespace mcrx
