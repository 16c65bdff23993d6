// sync_plan.hpp -- which kernel a synchronizer launch runs, with what grid, block and dynamic LDS, and what it rewrites in SyncArgs
// on the way (ofdmsync.hip: the launchers at its end), as pure functions of a handful of integers.  No HIP, no pointer that is ever
// followed: the host compiler builds it alone (host/sync_plan_test.cc replays tests/golden/sync_plan_cases.txt through it).
//
//   design (M, pilots, enabled carriers)      switches                                              workers stage runs
//   ----------------------------------------  ----------------------------------------------------  ---------------------------------------
//   any                                       no_fast & 1, or not a fast design                     payload_kernel<E, false>
//   48 | 64 subcarriers, <= 16 pilots         payload_fr 1, payload_lean 1, lean builds allowed     payload_lean_kernel + payload_lean_rest_kernel
//                                                                                                   (<63, 48> | <payload_xb 0: 0, else 63>): "splits"
//   64 subcarriers, <= 16 pilots              payload_fr 2 | 4 (| payload_lean 0), builds allowed   payload_multi_kernel<2 | 4 (| 1)>
//   128 | 256 subcarriers, 1 .. 64 pilots     payload_fr 1, payload_lean 1, lean builds allowed     payload_wide_kernel<63, E>
//   every other fast design or switch                                                               payload_kernel<E, true>
//   fast design: M = 64 E a power of two >= 64, or M = 48, with at most 64 pilots (Walker::fast_ok() is the device's copy);
//   lean builds allowed: no_fast bits 1 and 2 clear (sync_lean_path)
//
//   acquisition        E <= 2                                  E >= 4
//   scout              sync_kernel<E>                          sync_kernel<E>
//   lean | walk | tail sync_lean | _walk | _tail_kernel<E>     sync_kernel<E>    (the compiler cannot hold the lean ones' 64-bit values there)
//   segment waves      acq_lean_kernel<63, M> where seg_walker = 0 and the design has 48 | 64 subcarriers, E = 1, 1 .. 16 pilots and at
//                      most 64 enabled carriers; else sync_spec_kernel<E>
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "acq_shared.h"

// ---- launch geometry the kernels are built for
#define SY_MAXM 1024
// a synchronizer wave's LDS scratch (ofdmsync.hip: ldsc .. ldsqn)
#define SY_LDS_BYTES(M) ((((size_t)(M) * 8 + (size_t)(M) * 12 + 256 + 3 * MCRX_HDR_SYMS + 32 + 4 * MCRX_SPEC_MAX + 256) + 15) & ~(size_t)15)
#define VIT_B 960u             /* K = 7 decoder, steps per block: a multiple of 64 (traceback chunks own whole bytes) and of 6 (the lane layout's period) */
#define DK_T 256               /* threads of a decode_kernel workgroup */
#define SY_WALK_WPB 1          /* waves per workgroup of sync_walk_kernel (ofdmsync.hip: measured with four, one it stays) */
#ifndef ACQ_LEAN_WAVES
#define ACQ_LEAN_WAVES 3        /* waves per SIMD acq_lean_kernel is built for (launch_sync sizes the segments by it: sync_lean_waves()).  Three = 168
                                   registers: the kernel's real pressure is ~165, and at four (128) the 40 spilled registers sit on every event's
                                   chain -- 136 against 110 us per launch, scratch/r5/acq_ab.sh */
#endif
#ifndef SY_REST_FLOOR
#define SY_REST_FLOOR 256u     /* least grid of the launch behind the lean workers while its list hint is small */
#endif
#ifndef SY_GEN_FLOOR
#define SY_GEN_FLOOR 128u      /* grid of the general decoder while its list has been empty */
#endif

namespace mcrx {

// the integers of SyncConsts the launchers decide by
struct SyncDesign { int M, E, log2M, M_pilot, Nen; uint32_t max_enc_len, max_payload_len; };
constexpr int SY_WAVE = 64;

// ---- design predicates, each stated once
inline int sync_width_index(int E) { return E == 1 ? 0 : E == 2 ? 1 : E == 4 ? 2 : E == 8 ? 3 : E == 16 ? 4 : -1; }      // the symbol widths that have kernels
inline bool sync_pilots_in_row(const SyncDesign &d) { return d.M_pilot <= 16; }                     // the pilots inside one DPP row
// the fast symbol path: a shuffle FFT that fills the lanes (or 48 subcarriers) and the pilots inside one wave
inline bool sync_fast_design(const SyncDesign &d) { return ((d.log2M >= 6 && d.M == SY_WAVE * d.E) || (d.M == 48 && d.E == 1)) && d.M_pilot <= SY_WAVE; }
// the lean one-frame-per-wave workers of 48 / 64 subcarriers (payload_lean.hpp)
inline bool sync_lean_workers(const SyncDesign &d) { return sync_fast_design(d) && (d.M == SY_WAVE || d.M == 48) && sync_pilots_in_row(d); }
// the lean workers of 128 / 256 subcarriers (payload_wide.hpp)
inline bool sync_wide_workers(const SyncDesign &d) { return (d.E == 2 || d.E == 4) && d.log2M >= 7 && d.M == SY_WAVE * d.E && d.M_pilot >= 1 && d.M_pilot <= SY_WAVE; }
// waves per SIMD of the lean segment-wave kernel (acq_lean.hpp) if this design takes it, else 0
inline int sync_lean_waves(const SyncDesign &d) { return ((d.M == 64 || d.M == 48) && d.E == 1 && sync_pilots_in_row(d) && d.M_pilot >= 1 && d.Nen <= 64) ? ACQ_LEAN_WAVES : 0; }

// ---- one value per launch target.  Families with a kernel per symbol width hold them in the order E = 1, 2, 4, 8, 16.
enum SyncKernel {
    SK_NONE = 0,
    SK_SYNC_E1, SK_SYNC_E2, SK_SYNC_E4, SK_SYNC_E8, SK_SYNC_E16,                                  // sync_kernel<E>
    SK_SPEC_E1, SK_SPEC_E2, SK_SPEC_E4, SK_SPEC_E8, SK_SPEC_E16,                                  // sync_spec_kernel<E>
    SK_PAYLOAD_FAST_E1, SK_PAYLOAD_FAST_E2, SK_PAYLOAD_FAST_E4, SK_PAYLOAD_FAST_E8, SK_PAYLOAD_FAST_E16,                  // payload_kernel<E, true>
    SK_PAYLOAD_GENERAL_E1, SK_PAYLOAD_GENERAL_E2, SK_PAYLOAD_GENERAL_E4, SK_PAYLOAD_GENERAL_E8, SK_PAYLOAD_GENERAL_E16,   // payload_kernel<E, false>
    SK_TAIL_E1, SK_TAIL_E2, SK_LEAN_E1, SK_LEAN_E2, SK_WALK_E1, SK_WALK_E2,                       // sync_tail_ / sync_lean_ / sync_walk_kernel<E>
    SK_ACQ_LEAN_M48, SK_ACQ_LEAN_M64,                                                             // acq_lean_kernel<63, M>
    SK_MULTI_1, SK_MULTI_2, SK_MULTI_4,                                                           // payload_multi_kernel<frames per wave>
    SK_PLEAN_XB0, SK_PLEAN_XB63, SK_PLEAN_M48,                                                    // payload_lean_kernel<0>, <63>, <63, 48>
    SK_PLEAN_REST_XB0, SK_PLEAN_REST_XB63, SK_PLEAN_REST_M48,                                     // payload_lean_rest_kernel, the same three (SK_PLEAN_* + 3)
    SK_WIDE_E2, SK_WIDE_E4,                                                                       // payload_wide_kernel<63, E>
    SK_PLACE, SK_DECODE, SK_DECODE_GENERAL,                                                       // place_jobs_kernel, decode_kernel, decode_general_kernel
    SK_COUNT
};
inline bool sync_kernel_in(SyncKernel k, SyncKernel family, int n = 5) { return k >= family && k < family + n; }
// kernels that can end up decoding a packet themselves get the Viterbi decoder's block scratch behind their LDS
inline bool sync_kernel_decodes(SyncKernel k) { return sync_kernel_in(k, SK_SYNC_E1) || sync_kernel_in(k, SK_PAYLOAD_GENERAL_E1) || sync_kernel_in(k, SK_TAIL_E1, 2); }

struct SyncLaunch { SyncKernel k = SK_NONE; unsigned grid = 0, block = SY_WAVE; size_t lds = 0; };
enum SyncStatus { SYNC_LAUNCH = 0, SYNC_NOTHING, SYNC_INVALID };      // a plan's answer: launches to issue; nothing to do (success); refused (invalid value)

// a kernel of a per-width family at its ordinary LDS; *vit_off = where the decoder's scratch begins there (0: the kernel has none)
inline SyncLaunch sync_width_launch(SyncKernel family, const SyncDesign &d, unsigned grid, uint32_t *vit_off)
{
    SyncLaunch l;
    l.k = (SyncKernel)(family + sync_width_index(d.E)); l.grid = grid; l.lds = SY_LDS_BYTES(d.M);
    *vit_off = 0;
    if (sync_kernel_decodes(l.k)) {
        *vit_off = (uint32_t)((l.lds + 15) & ~(size_t)15);
        l.lds = *vit_off + (size_t)VIT_B * 8;
    }
    return l;
}

// ---- acquisition
enum SyncAcq { SYNC_ACQ_SCOUT = 0, SYNC_ACQ_LEAN, SYNC_ACQ_WALK, SYNC_ACQ_TAIL, SYNC_ACQ_SPEC };
struct SyncAcqInputs { SyncDesign d; uint32_t nch, nseg, spec_cap; int seg_phase, seg_walker; };
struct SyncAcqPlan { SyncStatus status = SYNC_NOTHING; SyncLaunch l; uint32_t vit_off = 0; };

inline SyncAcqPlan sync_acq_plan(SyncAcq what, const SyncAcqInputs &in)
{
    SyncAcqPlan r;
    const SyncDesign &d = in.d;
    if (in.nch == 0 || (what == SYNC_ACQ_SPEC && (in.spec_cap == 0 || in.nseg == 0))) return r;
    r.status = SYNC_INVALID;
    if (what != SYNC_ACQ_TAIL && what != SYNC_ACQ_SPEC && d.M > SY_MAXM) return r;       // (those two are refused by their width alone)
    if (what == SYNC_ACQ_SPEC && sync_lean_waves(d) && !in.seg_walker) {                 // scout_build = 2: the lean segment waves; else the Walker's
        r.l.k = d.M == 48 ? SK_ACQ_LEAN_M48 : SK_ACQ_LEAN_M64;
    } else {
        if (sync_width_index(d.E) < 0) return r;
        // the acquisition kernels proper exist for E <= 2 (part 3); wider symbols keep the full kernel as their scout, tail and walker
        static const SyncKernel narrow[5] = { SK_SYNC_E1, SK_LEAN_E1, SK_WALK_E1, SK_TAIL_E1, SK_SPEC_E1 };
        r.l = sync_width_launch(d.E <= 2 || what == SYNC_ACQ_SPEC ? narrow[what] : SK_SYNC_E1, d, 0, &r.vit_off);
    }
    r.l.grid = what == SYNC_ACQ_SPEC && in.seg_phase != 1 ? in.nch * in.nseg : in.nch;       // a wave per channel, or per (channel, segment)
    if (sync_kernel_in(r.l.k, SK_WALK_E1, 2)) {                                              // SY_WALK_WPB waves, a full-width scratch each
        r.l.grid = (in.nch + SY_WALK_WPB - 1) / SY_WALK_WPB; r.l.block = SY_WAVE * SY_WALK_WPB;
        r.l.lds = SY_WALK_WPB * SY_LDS_BYTES(d.E * SY_WAVE);
    }
    r.status = SYNC_LAUNCH;
    return r;
}

// ---- payload stage
enum SyncStage { SYNC_PLACE = 0, SYNC_WORKERS = 1, SYNC_DECODE = 2, SYNC_DECODE_GENERAL = 3, SYNC_BEHIND = 4 };       // BEHIND: the launch behind the lean workers
struct SyncPayloadInputs {
    SyncDesign d;
    uint32_t nch, max_jobs, frames_hint, grid_hint0, grid_hint2, vit_waves, enc_hint, payload_lds_pad;     // SyncArgs' fields of those names
    bool have_qam_list, have_vit_scratch;
    int scout, no_fast, payload_fr, payload_lean, payload_xb, split_rest, dec_phase;
};
struct SyncPayloadPlan {
    SyncStatus status = SYNC_NOTHING;
    int n = 0; SyncLaunch l[2];                 // in the order they are issued
    uint32_t soft_lds = 0, msg_lds = 0;         // decode_kernel's parameters
    // SyncArgs as the kernels get it
    uint32_t live_off = 0, dec_lds_soft = 0, vit_off = 0; int split_rest = 0, dec_phase = 0; bool clear_gen_list = false;
};

inline bool sync_fast_path(const SyncPayloadInputs &in) { return sync_fast_design(in.d) && !(in.no_fast & 1); }
inline bool sync_lean_path(const SyncPayloadInputs &in) { return sync_fast_path(in) && !(in.no_fast & 6); }      // ... and a worker build of its own allowed
// does this design's payload stage consist of the lean one-frame-per-wave workers and a launch behind them (kernels.h, split_rest)?
inline bool sync_payload_splits(const SyncPayloadInputs &in)
{
    return in.scout && sync_lean_path(in) && sync_lean_workers(in.d) && in.payload_fr == 1 && in.payload_lean;
}

// bytes of LDS a frame's soft bits get in this push's decode launch: 8 per coded byte, at most 56 KiB (longer frames
// decode in HBM); sized from the longest frame the previous launch saw -- enc_hint, read without a sync -- so that more
// workgroups fit a CU; 0 = no history yet: size for the configured maximum
inline uint32_t sync_decode_soft_lds(const SyncPayloadInputs &in)
{
    const uint32_t enc_cap = in.enc_hint ? ((in.enc_hint + 127u) & ~127u) : in.d.max_enc_len;
    size_t soft_lds = (size_t)8 * (enc_cap < in.d.max_enc_len ? enc_cap : in.d.max_enc_len);
    if (soft_lds > 56 * 1024) soft_lds = 56 * 1024;      // (twice that is the workgroup's soft area: 112 KB + the message)
    if (soft_lds < 4096) soft_lds = 4096;
    return (uint32_t)soft_lds;
}

// the workers (SYNC_WORKERS) or the launch behind them (SYNC_BEHIND); ngrid: the live frames expected
inline void sync_worker_launches(const SyncPayloadInputs &in, SyncStage stage, unsigned ngrid, SyncPayloadPlan &r)
{
    const SyncDesign &d = in.d;
    const unsigned nj = in.max_jobs;
    const int fr = in.payload_fr;               // frames per wave of the 64-subcarrier workers (0 = the width-generic worker)
    const bool narrow = sync_lean_path(in) && sync_lean_workers(d);
    // one frame per wave: the lean build (payload_lean.hpp) unless payload_lean = 0; measured on the bench stream: 1 -> 141.7 Gsample/s,
    // 0 -> 138, 2 -> 138, 4 -> 118.  The 48-subcarrier build has no packed-frame sibling, the 64-subcarrier one takes every other count as one.
    if (narrow && in.payload_lean && (d.M == 48 ? fr == 1 : fr > 0 && fr != 2 && fr != 4)) {
        // ... and one list-driven launch for what the main one does not take: frames beyond its grid, QAM payloads; sized by the
        // QAM list's most recent length.  payload_xb picks which butterfly stages exchange through the LDS crossbar.
        unsigned nq = in.grid_hint0 == ~0u ? nj : 2u * in.grid_hint0;
        nq = nq < SY_REST_FLOOR ? SY_REST_FLOOR : (nq > nj ? nj : nq);
        const SyncKernel k = d.M == 48 ? SK_PLEAN_M48 : in.payload_xb == 0 ? SK_PLEAN_XB0 : SK_PLEAN_XB63;
        if (stage != SYNC_BEHIND) { r.l[r.n].k = k; r.l[r.n].grid = ngrid; r.n++; }
        if (stage == SYNC_BEHIND || !r.split_rest) { r.l[r.n].k = (SyncKernel)(k + 3); r.l[r.n].grid = in.have_qam_list ? nq : nj; r.n++; }
        r.l[0].lds = r.l[1].lds = in.payload_lds_pad;
    } else if (narrow && d.M == SY_WAVE && fr > 0) {         // the packed-frame workers (and the round-2 worker: payload_lean = 0)
        const unsigned f = fr == 4 ? 4 : fr == 2 ? 2 : 1;
        r.l[0].k = f == 4 ? SK_MULTI_4 : f == 2 ? SK_MULTI_2 : SK_MULTI_1; r.l[0].grid = (nj + f - 1) / f; r.l[0].lds = f == 1 ? in.payload_lds_pad : 0;
        r.n = 1;
    } else if (sync_lean_path(in) && sync_wide_workers(d) && in.payload_lean && fr == 1) {
        r.l[0].k = d.E == 2 ? SK_WIDE_E2 : SK_WIDE_E4; r.l[0].grid = ngrid; r.n = 1;
    } else if (sync_width_index(d.E) < 0) r.status = SYNC_INVALID;
    else { r.l[0] = sync_width_launch(sync_fast_path(in) ? SK_PAYLOAD_FAST_E1 : SK_PAYLOAD_GENERAL_E1, d, nj, &r.vit_off); r.n = 1; }       // the width-generic worker
}

inline SyncPayloadPlan sync_payload_plan(const SyncPayloadInputs &in, SyncStage stage)
{
    SyncPayloadPlan r;
    if (in.nch == 0 || !in.scout || in.max_jobs == 0) return r;
    const unsigned nj = in.max_jobs;
    // frames of the most recent launch + a quarter: the workers and decoders walk the live list with a grid stride, so a launch that
    // holds more than expected only takes a second turn
    unsigned ngrid = in.frames_hint == ~0u ? nj : in.frames_hint + in.frames_hint / 4 + 64;
    if (ngrid > nj) ngrid = nj;
    // the lean workers take one BPSK / QPSK frame per wave out of the first `ngrid` of the live list; the launch behind them
    // walks the rest of it (live_off tells it where the grid ended)
    const bool fast = sync_fast_path(in);
    r.live_off = sync_payload_splits(in) ? ngrid : 0;
    if (stage == SYNC_BEHIND && !r.live_off) return r;                  // (only the lean workers have a launch behind them)
    if (r.live_off) { r.split_rest = in.split_rest; r.dec_phase = in.dec_phase; }
    r.dec_lds_soft = fast ? sync_decode_soft_lds(in) : 0u;
    r.clear_gen_list = !fast;
    if ((stage == SYNC_DECODE || stage == SYNC_DECODE_GENERAL) && !fast) return r;       // (the general workers decode in place)
    r.status = SYNC_LAUNCH; r.n = 1;
    if (stage == SYNC_PLACE) { r.l[0].k = SK_PLACE; r.l[0].grid = 1; }
    else if (stage == SYNC_DECODE) {                                    // LDS: soft bits as received | de-interleaved | message
        r.soft_lds = r.dec_lds_soft; r.msg_lds = (uint32_t)(((size_t)in.d.max_payload_len + 4 + 15) & ~(size_t)15);
        r.l[0].k = SK_DECODE; r.l[0].grid = ngrid; r.l[0].block = DK_T; r.l[0].lds = 2 * (size_t)r.soft_lds + r.msg_lds + 16;
    } else if (stage == SYNC_DECODE_GENERAL) {
        // the frames on the general list (filled by decode_kernel).  Grid from the list's most recent size -- kernels.h, list_hint -- inside
        // the K = 7 decoder's scratch, a region per workgroup.  (Capping the workgroups per CU with unused dynamic LDS changed nothing or
        // cost: the decoder is bound by vector issue at any occupancy, ~0.17 us per 1200-byte frame with the chip full.)
        unsigned ggrid = in.grid_hint2 ? (nj < 4096 ? nj : 4096) : SY_GEN_FLOOR;
        if (in.have_vit_scratch && ggrid > in.vit_waves) ggrid = in.vit_waves;
        r.l[0].k = SK_DECODE_GENERAL; r.l[0].grid = ggrid; r.l[0].lds = (size_t)VIT_B * 8;
    } else { r.n = 0; sync_worker_launches(in, stage, ngrid, r); }
    return r;
}

}  // namespace mcrx
