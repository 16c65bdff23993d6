// stream_call.hpp -- what execute_device of a stream operator (chanemu, rfchain, rfcal, cfr) checks about a call before it touches a
// buffer, pure: a function of integers.  Host code, no HIP; host/stream_call_test.cc holds its cases (tests/test_stream_call.py).
#pragma once
#include <stdint.h>

namespace mcrx {

// nullptr, or what is wrong with the call: d_in holds n + extra_in samples of bytes_in (4: sc16, 8: cf32) each, d_out gets n samples of
// bytes_out each.  Checked in this order: null buffers (null_out: d_out may be null -- nothing is written, and nothing more is asked of
// it), alignment to one sample, the limit of 2^32 samples, overlap of the byte ranges (`overlap`: the operator's sentence for it).
// in_place: d_in == d_out with equal formats is no overlap.  A call of no samples overlaps nothing.
inline const char *stream_call_check(uint64_t d_in, uint64_t d_out, uint64_t n, uint32_t bytes_in, uint32_t bytes_out, uint64_t extra_in,
                                     bool in_place, bool null_out, const char *overlap)
{
    if (!d_in || (!d_out && !null_out)) return "null buffer";
    if (d_in & (bytes_in - 1u)) return bytes_in == 4u ? "d_in must be 4-byte aligned" : "d_in must be 8-byte aligned";
    if (d_out & (bytes_out - 1u)) return bytes_out == 4u ? "d_out must be 4-byte aligned" : "d_out must be 8-byte aligned";
    const uint64_t most = (uint64_t)1 << 32;                            // (a lane per pair, 2^31 lanes a launch)
    if (n > most || extra_in > most - n) return extra_in ? "n + 2 * halo must not exceed 2^32 samples" : "at most 2^32 samples a call";
    if (!d_out || n == 0 || (in_place && d_in == d_out && bytes_in == bytes_out)) return nullptr;
    if (d_in < d_out + n * bytes_out && d_out < d_in + (n + extra_in) * bytes_in) return overlap;
    return nullptr;
}

}  // namespace mcrx
