// rx_plan.hpp -- every size and build selector a receiver handle lives by (mcrx_hip.hip: mcrx_hip_create), as a pure function of the
// call's arguments, the effective configuration, the design's carrier counts and the development switches.  No HIP, no handle: the
// host compiler builds it alone (host/rx_plan_test.cc replays tests/golden/rx_plan_cases.txt through it).  It also makes the
// configuration checks that need the design -- before anything is allocated.
#pragma once
#include "../../include/mcrx_hip.h"
#include "acq_shared.h"
#include "sync_plan.hpp"        // sync_fast_design(): which designs the lean path takes
#include "config_read.hpp"

#include <algorithm>
#include <cstdlib>

#define MCRX_SLOTS 8        /* most per-launch buffer sets (channel tiles, job list, per-job scratch); launch k uses slot k % nslots */

namespace mcrx {

// The experiment switches of development builds that change a planned value, as read_devel_env found them (devel.h: all unset =
// nullptr in a release build).  The plan applies them behind the configuration's fields and over them.
struct RxDevel {
    const char *serial = nullptr, *slots = nullptr, *no_scout = nullptr, *no_spec = nullptr;      // MCRX_SERIAL, MCRX_SLOTS, MCRX_NO_SCOUT, MCRX_NO_SPEC
    const char *payload_fr = nullptr, *payload_lean = nullptr, *payload_xb = nullptr;             // MCRX_PAYLOAD_FR / _LEAN / _XB
    const char *acq_mode = nullptr, *lean_build = nullptr;                                        // MCRX_ACQ_MODE, MCRX_LEAN_BUILD
    const char *walk_lds_pad = nullptr, *payload_lds_pad = nullptr;                               // MCRX_WALK_LDS_PAD, MCRX_PAYLOAD_LDS_PAD
};

struct RxInputs {
    unsigned N, M, cp, taper;
    mcrx_hip_config ec;             // effective_config(cfg)
    unsigned M_data, M_pilot;       // OfdmDesign::init's counts
    RxDevel devel;
};

struct RxPlan {
    unsigned K = 0;
    bool bypass = false;                    // one synchronizer fed channel-rate samples, no channelizer (ofdmtxrx)
    // the handle's wideband input format (mcrx_hip_config::input_format == sc16.hpp: IQ_*) and its bytes per sample.  The raw-sample
    // history, both stagings and the bulk path's device buffers hold samples in that format: bytes, indexed in samples * ss
    uint32_t in_fmt = 0; size_t ss = 8;
    // synchronizer bank
    uint32_t max_payload = 0, max_enc = 0, max_syms = 0;
    unsigned ch_first = 0, nch = 0;
    uint32_t max_rec = 0;
    uint64_t min_frame = 1;                 // channel-rate samples of the shortest possible frame
    uint64_t arena_cap = 0, sarena_cap = 0;
    // internal streams: channelizer | acquisition (speculative waves, scouts, placement) | payload workers + decode.
    // Launch k+1's acquisition -- a chain of dependent events per channel, a few waves per CU -- runs under launch
    // k's payload/decode kernels, and launch k+1's channelizer as soon as CUs free up.
    bool pipelined = true;
    uint32_t slab_blocks = 0;
    // oversampled front end stage by stage (cfg.front_end = 2, the form the oracle runs; kept as the cross-check of front_end = 1)
    bool oversampled = false;
    // taps per column of the bank channelizer_kernel runs and the blocks of FIR history it needs in front of every push: 14 / 13 = the
    // reference's firpfbch (m = 7), 28 / 27 = the oversampled front end folded into one bank (cfg.front_end = 1; channelizer.hip)
    unsigned chan_P = 14, hist_blocks = 13, col_shift = 0;
    uint64_t defer = 0; unsigned hist_tiles = 0;
    int payload_xb = 63, payload_lean = 1, payload_fr = 1;      // MCRX_PAYLOAD_FR / _LEAN / _XB: which build of the M = 64 payload workers (tests)
    int acq_mode = 0;
    bool spec = false;                      // segment-parallel acquisition: wanted, and the design is lean (the handle adds: the hint block exists)
    // scouts of the acquisition rounds: 1 = the lean scout's unbudgeted build (sync_walk_kernel: 256 + 40 registers, no spills), 0 = the
    // 168-register build (293 spilled) that round 2 made to fit beside four 80-register payload workers.  With eight 56-register
    // workers per SIMD neither fits beside them any more, and a scout that adopts 100 frames of a channel pays for every spill:
    // 8 channels 54.7 -> 64.8 Gsample/s, 512 channels 166.4 -> 169.9 (same box, same run; MCRX_LEAN_BUILD)
    int lean_build = 1;
    int seg_walker = 1;                     // 1: the segment waves are the general state machine's kernel (default); mcrx_hip_config::scout_build = 2: acq_lean.hpp's
    bool scout = true;
    uint32_t round_lds_pad = 0;             // the same cap outside walk mode (MCRX_PAYLOAD_LDS_PAD)
    uint32_t walk_lds_pad = 13312;          // walk mode: unused LDS per payload worker = at most three of them per SIMD, the fourth slot is the walking scouts' (95 -> 110 Gsample/s on ragged traffic)
    unsigned nslots = 5;                    // buffer sets in use: the channelizer and the acquisition chain of up to nslots - 1 pushes run ahead of the payload workers
    uint32_t max_jobs = 0;                  // job list entries per launch: the frames (max_rec) + the entries the segment waves fill for nothing (two per segment) + void reservations
    uint32_t vit_rows = 0, vit_waves = 0, vit_mode = 0;      // the K = 7 decoder's decision rows (kernels.h: vit_scratch); 0 rows: no such decoder in this handle
    bool lean = false;                      // the design runs on the lean kernels (the only ones that speculate)
    size_t stage_cap = 0;                   // host and device staging (samples): whole tiles of MCRX_TILE blocks
    size_t hist_bytes = 0;                  // the raw-sample history of one buffer, rounded up to whole 16-byte units (what sync_reset_launch clears: an even number of cf32)
    bool side_stream = false;               // the stream of the launches that normally find nothing to do is wanted (mcrx_hip.hip: create_streams_and_events)
};

static inline int devel_int(const char *v, int dflt) { return v ? atoi(v) : dflt; }

// (the plan's parts: each MCRX_OK, or the refusal's code with its text in *err)
#define MCRX_REFUSE(code, msg) do { *err = (msg); return (code); } while (0)

// the shard, the frame limits and the record pool with its arenas
static inline int plan_frames(const RxInputs &in, RxPlan &r, const char **err)
{
    const unsigned N = in.N, M = in.M, cp = in.cp;
    const mcrx_hip_config &cfg = in.ec;
    r.max_payload = cfg.max_payload_len ? cfg.max_payload_len : 2048;
    r.max_enc = 4 * (r.max_payload + 4) + 16;
    // floor: the per-frame scratch rows (max_enc + 16 bytes) also hold the soft Viterbi decoder's checkpoints, 128 bytes
    // per 960 trellis steps = 128 * ceil((8 e0 + 6) / 960) <= 0.54 max_enc + 128 bytes for a frame that fits (e0 <= max_enc / 2
    // behind the rate-1/2 code): covered from max_enc = 256 on (smaller rows were overrun by 128 bytes)
    if (r.max_enc < 256) r.max_enc = 256;
    r.max_enc = (r.max_enc + 15) & ~15u;
    r.max_syms = 8 * r.max_enc;
    r.ch_first = cfg.channel_first;
    if (r.ch_first >= N || (uint64_t)r.ch_first + cfg.channel_count > N) MCRX_REFUSE(MCRX_EINVAL, "channel shard outside [0, N)");
    r.nch = cfg.channel_count ? cfg.channel_count : N - r.ch_first;
    r.max_rec = cfg.max_frames ? cfg.max_frames : 16 * r.nch + 64;
    r.min_frame = (uint64_t)(3 + (288 + in.M_data - 1) / in.M_data + 2) * (M + cp);
    if (!cfg.max_frames) {
        // ... and never fewer than one host batch (Execute() harvests per batch) can hold: the shortest frame is
        // S0a, S0b, S1, the header symbols, one payload symbol and the tail
        const uint64_t batch = cfg.batch_samples ? cfg.batch_samples : ((uint64_t)1 << 20);
        const uint64_t per_ch = (batch / r.K + 8) / r.min_frame + 2;
        r.max_rec = (uint32_t)std::max<uint64_t>(r.max_rec, std::min<uint64_t>(per_ch * r.nch, 1u << 22));
        // ... and enough for bulk Execute() calls to run in chunks of up to 16 Mi samples between harvests, within
        // about 2 GB of per-record buffers (arena share, soft bits, scratch, equaliser)
        const uint64_t per_rec = ((((uint64_t)r.max_payload + 15) & ~15ull) + 64ull * (2ull * (r.max_payload + 4) + 8)) +
                                 10ull * r.max_enc + 32 + 8ull * M;
        const uint64_t bulk = std::min<uint64_t>((((uint64_t)16 << 20) / r.K + 8) / r.min_frame + 3, ((uint64_t)2 << 30) / per_rec / r.nch);
        r.max_rec = (uint32_t)std::max<uint64_t>(r.max_rec, bulk * r.nch);
    }
    // frame arenas (per result generation): payload bytes | equalised symbols, the latter reserved for BPSK
    // behind one rate-1/2 code (longer frames still fit while the total stays below the cap; overflow is counted)
    r.arena_cap = (uint64_t)r.max_rec * (((uint64_t)r.max_payload + 15) & ~15ull);
    r.sarena_cap = (uint64_t)r.max_rec * (8ull * 8ull * (2ull * (r.max_payload + 4) + 8));
    if (r.sarena_cap > (8ull << 30)) r.sarena_cap = 8ull << 30;
    return MCRX_OK;
}

// which builds of the stages (mcrx_hip_config::worker_build / acquisition / scout_build), then the development switches: behind the
// configuration's fields and over them
static inline int plan_builds(const mcrx_hip_config &cfg, const RxDevel &dv, RxPlan &r, const char **err)
{
    const uint32_t wb = cfg.worker_build, aq = cfg.acquisition, sb = cfg.scout_build;
    if (wb > 5 || aq > 5) MCRX_REFUSE(MCRX_EINVAL, "worker_build / acquisition out of range");
    if (wb == 1) r.payload_xb = 0;
    if (wb >= 2) { r.payload_lean = 0; r.payload_fr = wb == 2 ? 1 : wb == 3 ? 2 : wb == 4 ? 4 : 0; }
    if ((aq >= 1 && aq <= 3) || aq == 5) r.acq_mode = (int)aq;
    r.spec = aq != 4;                       // (wanted; whether the design allows it: rx_plan)
    if (sb > 2) MCRX_REFUSE(MCRX_EINVAL, "scout_build out of range");
    if (sb == 1) r.lean_build = 0;
    if (sb == 2) r.seg_walker = 0;
    if (dv.serial) r.pipelined = false;
    r.scout = dv.no_scout == nullptr;
    if (!r.scout || dv.no_spec) r.spec = false;         // (speculation hands off through the scouts' job list)
    r.payload_fr = devel_int(dv.payload_fr, r.payload_fr);
    r.payload_lean = devel_int(dv.payload_lean, r.payload_lean) != 0;
    r.payload_xb = devel_int(dv.payload_xb, r.payload_xb);
    r.acq_mode = devel_int(dv.acq_mode, r.acq_mode);
    r.lean_build = devel_int(dv.lean_build, r.lean_build);
    r.walk_lds_pad = (uint32_t)devel_int(dv.walk_lds_pad, (int)r.walk_lds_pad);
    r.round_lds_pad = (uint32_t)devel_int(dv.payload_lds_pad, (int)r.round_lds_pad);
    if (dv.slots) r.nslots = (unsigned)std::max(2, std::min(MCRX_SLOTS, atoi(dv.slots)));
    if (!r.pipelined) r.nslots = 2;
    return MCRX_OK;
}

// MCRX_OK and *out, or the refusal's code with its text in *err (and *out untouched).  The checks come in the order
// mcrx_hip_create has always made them in: the first field that is wrong is the one reported.
inline int rx_plan(const RxInputs &in, RxPlan *out, const char **err)
{
    const unsigned N = in.N, M = in.M, cp = in.cp;
    const mcrx_hip_config &cfg = in.ec;
    RxPlan r;
    r.bypass = cfg.single_channel != 0;
    r.K = r.bypass ? 1 : 2 * N;
    r.in_fmt = cfg.input_format; r.ss = r.in_fmt == 1 ? 4 : 8;       // sc16: two int16_t; cf32: a float2
    if (int rc = plan_frames(in, r, err)) return rc;
    r.pipelined = !cfg.serial;
    r.slab_blocks = cfg.slab_blocks ? ((cfg.slab_blocks + MCRX_TILE - 1) & ~(uint32_t)(MCRX_TILE - 1)) : 0;      // 0: sized per launch; slabs are whole tiles
    const uint32_t front_end = r.bypass ? 0 : cfg.front_end;
    if (front_end > 2) MCRX_REFUSE(MCRX_EINVAL, "front_end must be 0, 1 or 2");
    r.oversampled = front_end == 2;
    if (front_end && ((r.K & (r.K - 1)) || r.K > 1024 || r.K < 2)) MCRX_REFUSE(MCRX_EUNSUPP, "the oversampled front end needs a power-of-two channel count <= 512");
    if (front_end == 1) { r.chan_P = 28; r.hist_blocks = 27; r.col_shift = r.K / 2 + 1; }
    // channel-rate history in front of every push's tiles: a symbol window, plus -- if frames straddling two pushes are
    // to be deferred rather than walked serially -- the longest frame start-to-push-end distance to be covered
    r.defer = cfg.defer_samples;
    r.hist_tiles = (unsigned)((r.defer + M + cp + 8 + MCRX_TILE - 1) / MCRX_TILE + 1);
    if (int rc = plan_builds(cfg, in.devel, r, err)) return rc;
    // speculative acquisition: the lean path only (SyncConsts' E and log2M of an M-carrier design; 48 = 3 x 16: the reference
    // applications' default, round 5)
    unsigned E = 1; while (E < (M + 63) / 64) E <<= 1;
    unsigned log2M = 0;
    if ((M & (M - 1)) == 0) while ((1u << log2M) < M) log2M++;
    r.lean = sync_fast_design({ (int)M, (int)E, (int)log2M, (int)in.M_pilot, 0, 0, 0 });
    if (r.scout) {
        r.max_jobs = 2 * r.max_rec + 4 * r.nch + 1024;
        if (cfg.payload_soft) {
            // The K = 7 decoder (decode_general_kernel, viterbi_frames.hpp) takes a frame per wave and keeps 512 bytes of decisions per trellis
            // step of a block in HBM: one region per workgroup, as many workgroups as a launch can have frames (at most 2 per SIMD: it is
            // arithmetic).  Its launches follow each other on the work stream, so one set serves every slot.  ~200 KB per workgroup at 1200-byte
            // payloads = 0.4 GB: allocated when the first frame with the code has been seen (cfg.conv_scratch), launch_sync.
            r.vit_rows = vf::rows_for(4u * r.max_enc + 6u);
            r.vit_waves = (uint32_t)std::max<uint64_t>(64, std::min<uint64_t>(r.max_rec, 2048));
            r.vit_mode = cfg.conv_scratch;
            if (r.vit_mode > 2) MCRX_REFUSE(MCRX_EINVAL, "conv_scratch must be 0, 1 or 2");
        }
    }
    r.spec = r.spec && r.lean;
    r.hist_bytes = ((size_t)r.hist_blocks * r.K * r.ss + 15) & ~(size_t)15;
    const size_t tile_samples = (size_t)MCRX_TILE * r.K;
    const size_t want = cfg.batch_samples ? cfg.batch_samples : ((size_t)1 << 20);
    r.stage_cap = std::max<size_t>(1, (want + tile_samples - 1) / tile_samples) * tile_samples;
    // (Only for receivers of few channels: their pushes are chains of launch gaps.  Not a rank's shard behind a pipeline: streams enough there.)
    r.side_stream = r.pipelined && r.nch <= 32 && cfg.channel_count == 0;
    *out = r;
    return MCRX_OK;
}

#undef MCRX_REFUSE

}  // namespace mcrx
