// acq_shared.h -- what the kernels and the host's planners (acq_plan.hpp, rx_plan.hpp) both read: the limits of the segment-parallel
// acquisition, the layout of the host-mapped hint block and the K = 7 decoder's row count.  No HIP types: kernels.h includes it, and
// so do programs built by the host compiler alone.
#pragma once
#include <stdint.h>

#define MCRX_SPEC_MAX 256        // slots per channel the scouts hold in registers at a time (kernels.h: SpecSlot)
#define MCRX_SEG_MAX 128         // most segment waves per channel
#define MCRX_HDR_SYMS 288        // BPSK header symbols
#ifdef __HIPCC__
#define MCRX_HD __host__ __device__
#else
#define MCRX_HD
#endif

namespace mcrx {

// The hint block: HINT_WORDS 32-bit words in pinned, device-mapped, coherent host memory.  The kernels of a launch leave there what
// sizes the NEXT launches; the host reads it without ever waiting for the device, a launch or two late.  Advisory: only speed
// depends on it.  The kernels reach the words through three pointers of SyncArgs into the one block:
//     hint      = block         hint[k]      = word k         (place_jobs_kernel: hint[0]; the packet decoder: hint[HINT_K7_SEEN])
//     walk_hint = block + 2     walk_hint[k] = word 2 + k     (place_jobs_kernel writes k = 0 .. 5: HINT_WALKED .. HINT_LAUNCH_FRAMES)
//     list_hint = block + 8     list_hint[k] = word 8 + k     (place_jobs_kernel: k = 0, HINT_LIST_QAM; k = 1, HINT_LIST_TRELLIS, has no
//                                                              writer left; the general decoder: k = 2, HINT_LIST_GENERAL)
enum HintWord {
    HINT_ENC_MAX = 0,            // longest coded frame [bytes] among a launch's jobs: sizes the next launch's decode LDS
    HINT_PRED_MAX = 1,           // widest prediction list (rounds 1-3; unused now)
    HINT_WALKED = 2,             // frames the scouts acquired themselves, so far
    HINT_ADOPTED = 3,            // frames adopted from segment waves, so far
    HINT_CADENCE_FRAMES = 4,     // frames that followed their predecessor at the distance of the pair before, so far
    HINT_FRAMES_SEEN = 5,        // frames that could have, so far
    HINT_SLOTS_FILLED = 6,       // slots the segment waves filled, so far (those nobody adopts measure a wrong anchor)
    HINT_LAUNCH_FRAMES = 7,      // frames of the most recent finished launch
    HINT_LIST_QAM = 8,           // of that launch: hand-offs with a 16- / 64-QAM payload ...
    HINT_LIST_TRELLIS = 9,       // ... trellis blocks ...
    HINT_LIST_GENERAL = 10,      // ... frames on the general decoder's list
    HINT_K7_SEEN = 11,           // a frame with the K = 7 code was decoded while its decoder had no scratch
    HINT_WORDS = 12
};
enum { HINT_WALK_BASE = HINT_WALKED, HINT_LIST_BASE = HINT_LIST_QAM };     // where walk_hint / list_hint point

// the K = 7 decoder's geometry (csrc/viterbi_frames.hpp): T trellis steps in at most 64 blocks of a multiple of 24 steps, each run W steps
// early and W steps long; a wave keeps B + 2 W decision rows of 512 bytes
namespace vf {
constexpr unsigned W = 48;
MCRX_HD constexpr unsigned block_steps(unsigned T) { return 24u * ((T + 1535u) / 1536u); }
MCRX_HD constexpr unsigned rows_for(unsigned T) { return block_steps(T) + 2u * W; }
}

}  // namespace mcrx
