// stream_call_test.cc -- csrc/stream_call.hpp with a main of its own (host compiler only, no HIP, no GPU): the calls that
// tests/test_gpu_{chanemu,rfchain,rfcal,cfr}.py make with real pointers, on integers, with the message each must get (tests/test_stream_call.py).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <initializer_list>
#include "../csrc/stream_call.hpp"

using namespace mcrx;

static int g_bad = 0;
static void expect(const char *got, const char *want, const char *what, int line)
{
    const bool same = (!got && !want) || (got && want && !strcmp(got, want));
    if (!same) { printf("line %d (%s): got \"%s\", want \"%s\"\n", line, what, got ? got : "(accepted)", want ? want : "(accepted)"); g_bad++; }
}
#define EXPECT(call, want) expect(call, want, #call, __LINE__)

static const char *const TAPS = "d_in and d_out overlap: the taps read behind the write front, in-place use is not possible";
static const char *const PLACE = "d_in and d_out overlap: in-place use takes d_in == d_out and equal formats";
static const char *const NEIGH = "d_in and d_out overlap: the operator reads neighbours, in-place use is refused";
static const char *const IN4 = "d_in must be 4-byte aligned", *const IN8 = "d_in must be 8-byte aligned";
static const char *const OUT4 = "d_out must be 4-byte aligned", *const OUT8 = "d_out must be 8-byte aligned";
static const char *const MOST = "at most 2^32 samples a call", *const HALO = "n + 2 * halo must not exceed 2^32 samples";
static const char *const OK = nullptr;

int main()
{
    const uint64_t n = 4096, p = 0x7f0000100000ull, far = p + 16 * n, two32 = (uint64_t)1 << 32;
    // chanemu: cf32 in, cf32 or sc16 out, never in place
    for (uint32_t so : { 8u, 4u }) {
        auto call = [&](uint64_t a, uint64_t b, uint64_t count) { return stream_call_check(a, b, count, 8u, so, 0, false, false, TAPS); };
        EXPECT(call(0, far, n), "null buffer"); EXPECT(call(p, 0, n), "null buffer");
        EXPECT(call(p + 4, far, n), IN8);                               // d_in: 8 bytes
        EXPECT(call(p, far + so / 2, n), so == 4 ? OUT4 : OUT8);        // d_out: one sample of its format
        EXPECT(call(p, p, n), TAPS);                                    // in place
        EXPECT(call(p, p + 8 * n - so, n), TAPS);                       // the output's first sample on the input's last
        EXPECT(call(p + 8 * n, p + 8 * n - so * n + so, n), TAPS);      // the output's last sample on the input's first
        EXPECT(call(p, p + 8 * n, n), OK);                              // adjacent is not overlapping
        EXPECT(call(p + 8 * n, p + 8 * n - so * n, n), OK);
        EXPECT(call(p + 8, far + so, n), OK);                           // one sample's alignment is enough
        EXPECT(call(p, far + two32 * 8, two32), OK); EXPECT(call(p, far + two32 * 8, two32 + 1), MOST);
        EXPECT(call(p, p, 0), OK);                                      // a call of no samples overlaps nothing
    }
    // rfchain and rfcal: either format on either side, in place with equal formats
    for (uint32_t si : { 8u, 4u }) for (uint32_t so : { 8u, 4u }) {
        auto call = [&](uint64_t a, uint64_t b, uint64_t count) { return stream_call_check(a, b, count, si, so, 0, true, false, PLACE); };
        EXPECT(call(0, p, n), "null buffer"); EXPECT(call(p, 0, n), "null buffer");
        EXPECT(call(p + si / 2, far, n), si == 4 ? IN4 : IN8);          // d_in: one sample of its format
        EXPECT(call(p, far + so / 2, n), so == 4 ? OUT4 : OUT8);        // d_out likewise
        EXPECT(call(p, p + si * n - so, n), PLACE);                     // the output's first sample on the input's last
        EXPECT(call(p + so * n - si, p, n), PLACE);                     // the input's first sample on the output's last
        EXPECT(call(p + si, p, n), PLACE); EXPECT(call(p, p + so, n), PLACE);     // shifted by one sample: overlapping, not in place
        EXPECT(call(p, p, two32 + 1), MOST);                            // too long (judged before the overlap)
        EXPECT(call(p, p, n), si == so ? OK : PLACE);                   // in place: equal formats only
        EXPECT(call(p, p + si * n, n), OK);                             // adjacent, behind the input
        EXPECT(call(p + so * n, p, n), OK);                             // adjacent, behind the output
        EXPECT(call(far, far, 1), si == so ? OK : PLACE); EXPECT(call(p, p, 0), OK);
        EXPECT(call(p, p, two32), si == so ? OK : PLACE);
        // rfcal's measure-only call: d_out may be null, and then nothing more is asked of it
        auto meas = [&](uint64_t a, uint64_t b, uint64_t count) { return stream_call_check(a, b, count, si, so, 0, true, true, PLACE); };
        EXPECT(meas(p, 0, n), OK); EXPECT(meas(0, 0, n), "null buffer"); EXPECT(meas(0, p, n), "null buffer");
        EXPECT(meas(p + si / 2, 0, n), si == 4 ? IN4 : IN8);
        EXPECT(meas(p, 0, two32 + 1), MOST); EXPECT(meas(p, 0, two32), OK);
        EXPECT(meas(p, p + so / 2, n), so == 4 ? OUT4 : OUT8); EXPECT(meas(p, p + so, n), PLACE); EXPECT(meas(p + si, p, n), PLACE);
    }
    // cfr: cf32 in with 2 * halo more samples than it writes, never in place (halo 62: passes = 2, half_len = 31)
    for (uint32_t so : { 8u, 4u }) {
        const uint64_t halo = 62, nin = n + 2 * halo;
        auto call = [&](uint64_t a, uint64_t b, uint64_t count) { return stream_call_check(a, b, count, 8u, so, 2 * halo, false, false, NEIGH); };
        EXPECT(call(0, p, n), "null buffer"); EXPECT(call(p, 0, n), "null buffer");
        EXPECT(call(p + 4, far, n), IN8);                               // d_in: half a sample
        EXPECT(call(p, far + so / 2, n), so == 4 ? OUT4 : OUT8);        // d_out likewise
        EXPECT(call(p, p, n), NEIGH);                                   // in place
        EXPECT(call(p, p + 8 * halo, n), NEIGH);                        // the output on the samples it belongs to
        EXPECT(call(p, p + 8 * nin - so, n), NEIGH);                    // the output's first sample on the input's last
        EXPECT(call(p + so * n - 8, p, n), NEIGH);                      // the input's first sample on the output's last
        EXPECT(call(p, far + two32 * 8, two32), HALO);                  // 2^32 samples and their halos
        EXPECT(call(p, far + two32 * 8, two32 - 2 * halo + 1), HALO);
        EXPECT(call(p, far + two32 * 8, two32 - 2 * halo), OK);         // the limit itself
        EXPECT(call(p, far, ~(uint64_t)0), HALO);                       // (n + 2 * halo does not wrap past the limit)
        EXPECT(call(p, p + 8 * nin, n), OK); EXPECT(call(p + so * n, p, n), OK);      // adjacent ranges
        EXPECT(call(p, p, 0), OK); EXPECT(call(p, p + 8, 0), OK);       // nothing to do: the halos alone overlap nothing
    }
    if (g_bad) { printf("%d case(s) failed\n", g_bad); return 1; }
    printf("stream_call_test ok\n");
    return 0;
}
