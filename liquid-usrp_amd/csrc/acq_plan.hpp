// acq_plan.hpp -- the acquisition policy of a synchronizer launch (mcrx_hip.hip: launch_sync) as a pure function: integer and
// float arithmetic on the policy's own state, a snapshot of the hint block and the launch's sizes.  No HIP, no handle: the host
// compiler builds it alone (host/acq_plan_test.cc replays tests/golden/acq_plan_cases.txt through it).
//
// Snapshot rule.  launch_sync copies the HINT_WORDS words out of the host-mapped block ONCE per launch and every decision of the
// launch is taken from that copy.  The words are advisory (only speed depends on them) and the device updates them whenever a launch
// finishes, so reading a word twice in a launch could see two values, to no purpose; on any input where the device writes nothing
// between two reads the snapshot gives what repeated reads give.
#pragma once
#include "../../include/mcrx_hip.h"
#include "acq_shared.h"

namespace mcrx {

// what the policy remembers from launch to launch (the handle's q->acq)
struct AcqPolicy {
    float frames_per_push = 0.f; uint64_t last_nsamp = 0;        // frames per channel and push, smoothed; the samples of the push it was taken from
    bool cadenced = true; uint32_t cad_same = 0, cad_frames = 0; int cad_count = 0;      // the cadence detector: windows of 8 launches
    // cadenced traffic: 0 / 1 = the lattice carried over from the previous push (absolute / from the push's beginning), 2 = an anchor phase
    int anchor_kind = 0; uint32_t anchor_retry = 0, anc_filled = 0, anc_adopted = 0;
    uint32_t nseg_fixed = 0, seg_frames = 4;                     // experiments (MCRX_NSEG / MCRX_SEG_FRAMES): segments per channel, fixed; frames per segment aimed at
    uint32_t list_seen[3] = { 0, 0, 0 }, list_age[3] = { 64, 64, 64 };      // grids of the list-driven launches (HINT_LIST_BASE + i), sticky for 64 launches
};

struct AcqInputs {
    uint64_t buf_samples;       // channel-rate samples of the launch's buffer, history included
    uint32_t hist_tiles;        // tiles of history in front of the new samples
    uint32_t nch, max_jobs;
    int acq_mode;               // mcrx_hip_config::acquisition (0, 1, 2, 3, 5)
    int seg_walker;             // 1: the general state machine's segment waves; 0: the lean ones, lean_waves to a SIMD (0: the design has none)
    int lean_waves;
    bool have_hints;            // the hint block exists and the device can write it (else: the snapshot is zeros and says nothing)
    bool spec;                  // segment-parallel acquisition is on for this handle: without it only the hints below are planned
};

struct AcqPlan {
    // for every launch
    uint32_t frames_hint = ~0u, grid_hint[3] = { ~0u, ~0u, ~0u }, enc_hint = 0;      // SyncArgs' fields of those names
    bool want_k7 = false;       // frames with the K = 7 code arrive: its decoder wants its scratch
    // segment-parallel acquisition
    uint32_t nseg = 0;          // segment waves per channel
    uint32_t spw = 0;           // slots per wave
    uint32_t spec_stride = 0;   // slots per channel the launch needs in the slot array = nseg * spw
    uint32_t spec_cap = 0;      // SyncArgs::spec_cap (0: no segment waves)
    uint32_t seg_jobs = 1;      // SyncArgs::seg_jobs behind the segment waves' launches
    int nphase = 0;             // segment-wave launches: none, { 0 }, { 3 + anchor_kind } or { 1, 2 }
    struct { int seg_phase; uint32_t seg_jobs; } phase[2] = { { 0, 1 }, { 0, 1 } };
};

inline AcqPlan acq_plan(AcqPolicy &p, const uint32_t h[HINT_WORDS], const AcqInputs &in)
{
    AcqPlan r;
    r.want_k7 = h[HINT_K7_SEEN] != 0;
    if (in.have_hints) {
        r.frames_hint = h[HINT_LAUNCH_FRAMES];
        if (r.frames_hint == 0) r.frames_hint = ~0u;                 // (a launch without frames says nothing about the next)
        for (int i = 0; i < 3; i++) {                    // (sticky for a while: a list that was non-empty within the last 64 launches keeps its full grid)
            const uint32_t v = h[HINT_LIST_BASE + i];
            if (v) { p.list_seen[i] = v; p.list_age[i] = 0; } else if (p.list_age[i] < 64) p.list_age[i]++; else p.list_seen[i] = 0;
            r.grid_hint[i] = p.list_seen[i];
        }
        r.enc_hint = h[HINT_ENC_MAX];
    }
    if (!in.spec) return r;
    // How many segments: enough waves to fill the chip and short chains (a wave's frames are acquired one after the other),
    // but every segment costs two acquisitions that produce nothing (its first frame, taken from an arbitrary state, and the
    // frame that links it to the next segment), and its share of the channel's MCRX_SPEC_MAX slots must hold its frames.
    // F = frames per channel and push, from the hand-offs the most recent finished launch counted (host-mapped, read without
    // a sync, a launch or two late); before the first report: one segment per 16 Ki samples.  Only speed depends on it.
    const uint64_t nsamp = in.buf_samples > (uint64_t)in.hist_tiles * MCRX_TILE ? in.buf_samples - (uint64_t)in.hist_tiles * MCRX_TILE : 1;
    uint32_t nseg = p.nseg_fixed;
    if (!nseg) {
        const uint32_t nj = h[HINT_LAUNCH_FRAMES];
        if (nj) p.frames_per_push = 0.5f * p.frames_per_push + 0.5f * ((float)nj / (float)in.nch) * ((float)nsamp / (float)(p.last_nsamp ? p.last_nsamp : nsamp));
    }
    const float F = p.frames_per_push > 0.f ? p.frames_per_push : (float)nsamp / 16384.0f;
    if (!nseg) {
        float want = F / (float)p.seg_frames;                                    // chains of seg_frames (+ 2) frames ...
        const float fill = 1536.0f / (float)in.nch;                              // ... shorter while the chip is not full (1.5 waves per SIMD)
        if (want < fill) want = fill < F / 2.0f ? fill : F / 2.0f;
        // on a cadence the lattice starts make segments free (no wasted acquisitions), so chains go down to two frames while
        // all the waves still run at once (2 per SIMD): what a few-channel receiver's push is made of is this chain's latency
        // (the lean segment waves of the 64-subcarrier designs run lean_waves to a SIMD, and a frame there is a chain of ~15 us:
        //  chains of ONE frame while every wave is resident at once)
        if (p.cadenced) {
            const int lw = in.seg_walker ? 0 : in.lean_waves;
            const float conc = (lw ? 1024.0f * (float)lw : 2048.0f) / (float)in.nch, shortest = lw ? F : F / 2.0f;
            const float c2 = conc < shortest ? conc : shortest;
            if (want < c2) want = c2;
        }
        // (a wave's slots: F / nseg * 1.25 + 4, at most half a window of the scouts' slot headers -- see spw below)
        const float least = 1.25f * F / (float)(MCRX_SPEC_MAX / 2 - 4);
        if (want < least) want = least;
        const float most = in.nch * 128u <= 4096u ? 128.0f : 64.0f;               // (few channels: even 128 waves each leave the chip mostly empty)
        nseg = want < 1.0f ? 1u : (want > most ? (uint32_t)most : (uint32_t)(want + 0.999f));
    }
    if (nseg > MCRX_SEG_MAX) nseg = MCRX_SEG_MAX;
    // The anchor phase (kernels.h, SyncArgs::seg_phase) is one more launch and one frame's latency in front of everything else: worth it
    // while most frames follow their predecessor at the distance of the pair before (the scouts count both, place_jobs_kernel
    // copies the totals to host-mapped words), useless on traffic without a cadence.  Windows of 8 launches; MCRX_ACQ_MODE=3 / 1 pins it.
    if (in.have_hints && ++p.cad_count >= 8) {
        const uint32_t sm = h[HINT_CADENCE_FRAMES], fr = h[HINT_FRAMES_SEEN];
        const uint32_t ds = sm >= p.cad_same ? sm - p.cad_same : 0u, df = fr >= p.cad_frames ? fr - p.cad_frames : 0u;     // (mcrx_hip_spec_stats may have reset them)
        if (df > in.nch) p.cadenced = 2ull * ds > df;
        p.cad_same = sm; p.cad_frames = fr; p.cad_count = 0;
        // ... and which anchor.  The lattice carried over from the previous push needs no launch in front of the segment waves: as it
        // stood in the stream (a continuous stream), or as it stood from the push's beginning (pushes that are bursts of their own, a
        // replayed slab with a gap at its end).  A wrong one shows: every segment hands off two frames nobody adopts.  So: one
        // after the other while more than an eighth of the slots filled go to waste, the anchor phase (which finds the lattice inside
        // every push) when neither holds, and from the start again after 256 launches.
        const uint32_t sf = h[HINT_SLOTS_FILLED], ad = h[HINT_ADOPTED];
        const uint32_t dsf = sf >= p.anc_filled ? sf - p.anc_filled : 0u, dad = ad >= p.anc_adopted ? ad - p.anc_adopted : 0u;
        if (p.anchor_kind < 2 && dad > in.nch && dsf > dad + dad / 8) { if (++p.anchor_kind == 2) p.anchor_retry = 256; }
        p.anc_filled = sf; p.anc_adopted = ad;
    }
    if (p.anchor_kind == 2 && p.anchor_retry && --p.anchor_retry == 0) p.anchor_kind = 0;
    if (in.acq_mode == 3 || in.acq_mode == 5) p.cadenced = true;
    p.last_nsamp = nsamp;
    // Slots per wave: its share of MCRX_SPEC_MAX while the push's frames fit there (the scouts then hold every slot header in
    // registers), else what its frames need -- the channel's slots then exceed the window and the scouts move it along
    // (ofdmsync.hip: adopt_lookup), which takes two neighbouring waves' slots to fit in one window.
    uint32_t spw = MCRX_SPEC_MAX / nseg;
    { const uint32_t need = (uint32_t)(1.25f * F / (float)nseg) + 4u;
      if (need > spw) spw = need > MCRX_SPEC_MAX / 2 ? MCRX_SPEC_MAX / 2 : need; }
    r.nseg = nseg; r.spw = spw; r.spec_stride = r.spec_cap = nseg * spw;
    { const float per = F / (float)nseg + 2.0f;                      // its share of the channel's frames + the two at the segment's ends
      r.seg_jobs = per < 2.0f ? 2u : (per > 32.0f ? 32u : (uint32_t)(per + 0.999f));
      // ... and all the first blocks together leave the scouts' own hand-offs and second blocks half of the list
      const uint32_t room = in.max_jobs / 2 / (in.nch * nseg);
      if (r.seg_jobs > room) r.seg_jobs = room ? room : 1u; }
    if (in.acq_mode == 2) r.spec_cap = 0;                        // (MCRX_ACQ_MODE=2: no segment waves, the scouts walk everything)
    else if (in.acq_mode == 1 || nseg == 1 || (in.acq_mode == 0 && !p.cadenced)) { r.nphase = 1; r.phase[0] = { 0, r.seg_jobs }; }     // one launch, coarse starts
    else if (in.acq_mode != 3 && p.anchor_kind < 2) { r.nphase = 1; r.phase[0] = { 3 + p.anchor_kind, r.seg_jobs }; }       // one launch, anchored on the entry state (a channel that does not stand behind a frame: coarse starts)
    else {
        r.nphase = 2;
        r.phase[0] = { 1, 1u };                 // the first frame of every channel, from its real state: the cadence's anchor
        r.phase[1] = { 2, r.seg_jobs };         // everything behind it, segment-parallel
    }
    return r;
}

}  // namespace mcrx
