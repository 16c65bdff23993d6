// pd_plan.hpp -- the pure half of pdtable.hpp, in a file of its own so that a plan header can use it without the device half: the
// constants of a gain table (K, inv_step, step, e), the guard of int64 sums and the sizes of a streaming launch.  No device, any host
// compiler.  pdtable.hpp includes it; fbalign_plan.hpp takes e, the guard and the pair grid from here.
#pragma once
#include <cmath>
#include <stdint.h>

namespace mcrx {

enum { PD_WG = 256,                 // lanes of a workgroup; a lane owns index-aligned sample pairs
       PD_UNROLL = 4 };             // rounds an applying lane has in flight; pd_rounds() is a multiple of it

// What the lookup uses of a table of 2^table_log2 intervals up to full_scale:
//   K = 2^table_log2; inv_step = fp32(K / full_scale) and step = full_scale / K, both quotients made in double;
//   e: E = 2^e is the least power of two that is >= full_scale.
struct PdTableConsts { uint32_t K; float inv_step, Kf; double step; int e; };

static inline PdTableConsts pd_table_consts(uint32_t table_log2, float full_scale)
{
    PdTableConsts k;
    k.K = 1u << table_log2;
    k.Kf = (float)k.K;
    k.inv_step = (float)((double)k.K / (double)full_scale);
    k.step = (double)full_scale / (double)k.K;
    int ex = 0;
    const double m = std::frexp((double)full_scale, &ex);          // full_scale = m 2^ex, 0.5 <= m < 1
    k.e = m == 0.5 ? ex - 1 : ex;
    return k;
}

// The guard of int64 sums: at most 2^guard_log2 terms between two resets (DPD_GUARD_LOG2, MPD_GUARD_LOG2: derived where they are
// defined).  An arithmetic shift right by s maps |a| to at most ceil(|a| / 2^s), so the host's count follows an update as
// ceil(count / 2^s) and stays an upper bound.
static inline bool pd_guard_ok(uint64_t since, uint64_t n, uint32_t guard_log2)
{
    const uint64_t most = (uint64_t)1 << guard_log2;
    return since <= most && n <= most - since;
}
static inline uint64_t pd_guard_after_update(uint64_t since, uint32_t shift)
{
    return (since + (((uint64_t)1 << shift) - 1)) >> shift;
}

// lane pairs of a launch over n >= 1 samples whose first lies at an odd (1) or even (0) multiple of 8 bytes: iqpair.hpp's pairs
static inline uint64_t pd_pairs(uint64_t parity, uint64_t n) { return ((parity & 1u) + n + 1) >> 1; }
// rounds of 256 pairs a workgroup of an applying launch takes: its table (16 K bytes from L2) is 1/16 of the 2 * 8 * 512 bytes a round streams
static inline uint32_t pd_rounds(uint32_t K) { return K / 32u > (uint32_t)PD_UNROLL ? K / 32u : (uint32_t)PD_UNROLL; }
// the workgroups of a streaming launch: `rounds` * 256 pairs each (the copy build: 1 round; at most 2^31 + 1 pairs of 2^32 samples)
static inline uint32_t pd_stream_grid(uint64_t parity, uint64_t n, uint32_t rounds)
{
    const uint64_t per_wg = (uint64_t)PD_WG * rounds;
    return (uint32_t)((pd_pairs(parity, n) + per_wg - 1) / per_wg);
}
// LDS of an applying launch: the table's K quadruples
static inline uint32_t pd_stream_lds(uint32_t K) { return K * 16u; }

}  // namespace mcrx
