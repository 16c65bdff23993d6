/*
 * mcrx_hip.h -- C-ABI of the MI355X-native multichannel OFDM receiver (libmcrx_hip.so).
 *
 * Drop-in boundary for liquid-usrp's `multichannelrx` hot path.  Each entry point names
 * the reference interface it replaces (paths relative to the liquid-usrp tree):
 *
 *   mcrx_hip_create          multichannelrx::multichannelrx        lib/multichannelrx.cc:45-104
 *                            (= N x ofdmflexframesync_create :82, firpfbch_crcf_create_kaiser :91,
 *                             nco_crcf_create/set_frequency :99-100)
 *   mcrx_hip_destroy         multichannelrx::~multichannelrx       lib/multichannelrx.cc:107-132
 *   mcrx_hip_reset           multichannelrx::Reset                 lib/multichannelrx.cc:135-153
 *   mcrx_hip_execute_host    multichannelrx::Execute               lib/multichannelrx.cc:155-182
 *   mcrx_hip_execute_device  same, IQ already resident in HBM (synthetic source; replaces the
 *                            UHD recv loop of src/multichannel_rx.cc:184-212)
 *   mcrx_hip_flush / _next_frame
 *                            framesync_callback delivery           include/multichannelrx.h:45,
 *                                                                  src/multichannel_rx.cc:37-66
 *   mcrx_hip_channelize      nco_crcf_mix_down + firpfbch_crcf_analyzer_execute
 *                                                                  lib/multichannelrx.cc:163-164,188
 *   mcrx_hip_sync            N x ofdmflexframesync_execute         lib/multichannelrx.cc:193-194
 *
 * Plain C: pointers and sizes only.  All functions return 0 on success or a negative
 * MCRX_E* code; nothing throws across this boundary.  One caller thread per handle
 * (the reference classes are not thread-safe either).
 */
#ifndef MCRX_HIP_H
#define MCRX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCRX_OK          0
#define MCRX_EINVAL     -1      /* bad argument (reference: fprintf + throw 0) */
#define MCRX_ENOMEM     -2
#define MCRX_EHIP       -3      /* HIP runtime error; see mcrx_hip_last_error() */
#define MCRX_EUNSUPP    -4      /* configuration outside the kernels' supported set */
#define MCRX_EOVERFLOW  -5      /* frame pool exhausted: frames were dropped */
#define MCRX_EBUSY      -6      /* multichanneltx::UpdateData on a channel whose frame is still going out */

#define MCRX_TILE 16            /* time samples per (channel, tile) granule = 128 bytes: one channel per cache line, so a
                                   synchronizer that reads one channel's time series never drags a neighbour channel's samples in */

typedef struct mcrx_hip_s *mcrx_hip_t;

typedef struct {
    uint32_t struct_size;        /* sizeof(mcrx_hip_config) */
    uint32_t max_payload_len;    /* largest decodable payload [bytes]; 0 -> 2048.  The per-frame buffers hold coded frames of up to
                                    4 (max_payload_len + 4) + 16 bytes (two rate-1/2 codes); a frame that codes to more -- rep5 expands
                                    five-fold -- or carries a longer payload is reported with payload_valid = 0 */
    uint32_t max_frames;         /* frame records kept between flushes; 0 -> auto (covers one host batch of
                                    the shortest possible frames on every channel) */
    uint32_t payload_soft;       /* 1 = soft-decision payload decoding (default), 0 = hard.  (Hard decisions of the Hamming(8,4) code: a double
                                    error -- a word at distance 2 from several codewords -- decodes to the lowest symbol at that distance; liquid-dsp's
                                    own table for that case is not visible from the reference, so such frames, which fail their CRC either way, may
                                    carry other bytes than upstream's: DESIGN.md section 2, D8) */
    uint32_t slab_blocks;        /* channelizer blocks per workgroup slab; 0 -> auto */
    uint32_t channel_first;      /* synchronizer shard: first channel ...          */
    uint32_t channel_count;      /* ... and count handled by this handle; 0 -> all  */
    uint32_t batch_samples;      /* execute_host staging size [wideband samples]; 0 -> auto */
    uint32_t single_channel;     /* 1 = no channelizer: num_channels must be 1 and the samples pushed are that
                                    channel's own stream, i.e. one ofdmflexframesync (lib/ofdmtxrx.cc:91,620-626);
                                    samples are consumed MCRX_TILE at a time */
    uint32_t serial;             /* 1 = every kernel of a push runs in order on the caller's stream (profiling, debugging).
                                    Default 0: the handle overlaps its own stages -- channelizer, acquisition and payload/decode
                                    kernels of consecutive pushes run on three internal streams with three sets of buffers */
    uint32_t chunk_blocks;       /* execute_device: split a push into sub-slabs of this many blocks (rounded up to whole tiles) so that
                                    the stages of ONE call overlap too; 0 = one launch sequence per call */
    uint32_t defer_samples;      /* > 0: every push keeps this many channel-rate samples of history (plus a symbol) in front of its
                                    channel tiles, and a frame that begins less than that before the end of a push and does not
                                    end in it is acquired again by the next push -- whole, by the parallel path -- instead of
                                    being walked symbol by symbol across the boundary by one wave.  0 = off.  Stage-level callers
                                    (mcrx_hip_sync) must supply mcrx_hip_history_tiles() tiles of history themselves */
    uint32_t front_end;          /* 0 = the reference's analysis bank: critically sampled firpfbch, 2N channels, lower N kept
                                    (lib/multichannelrx.cc:89-91).  1 = the oversampled bank BASELINE.json names: firpfbch2 with 2N
                                    channels (twice the channel rate, prototype cut off at the neighbour's centre) followed per kept
                                    channel by a half-band decimator back to the channel rate -- less aliasing at the channel edges.
                                    Oscillator, bank and decimator run as ONE kernel (the chain is a critically sampled bank with a
                                    28-tap composite prototype per column: csrc/channelizer.hip): 12 algorithmic bytes per sample like
                                    front_end = 0, 27 blocks of filter history instead of 13 (mcrx_hip_history_blocks).
                                    2 = the same chain stage by stage (oscillator pass, bank at twice the rate, adapter: three kernels,
                                    52 bytes per sample) -- the form the oracle computes, kept as the cross-check of 1; execute_host /
                                    execute_device only.  Power-of-two channel counts for 1 and 2 */
    uint32_t skip_framesyms;     /* 1 = harvests leave the equalised symbols in HBM (frames report num_framesyms = 0): 1.2 KB
                                    instead of 59 KB per frame over the host link at the benchmark's frame size; 2 = the payload workers
                                    of 64-subcarrier symbols do not even store them (a third of the bytes that stage moves): for callers
                                    whose callback never reads stats.framesyms (the reference's src/multichannel_rx.cc:37-66 does not) */
    /* Alternate builds of the same stages.  Every one decodes the same frames (the -m gpu tests hold each to the oracle); they
     * differ in speed only and exist so that a regression in the default can be told from one in the algorithm.  0 = default. */
    uint32_t worker_build;       /* M = 64 payload workers: 0 = lean workers, butterfly exchanges through the LDS crossbar;
                                    1 = lean workers with the exchanges on the VALU (DPP / permlane swaps); 2 = the round-2 worker, one
                                    frame per wave; 3 / 4 = that worker with two / four frames per wave; 5 = the width-generic kernel.
                                    M = 128 / 256: 0 = the lean one-frame-per-wave workers of csrc/payload_wide.hpp (round 6), 2 .. 5 = the
                                    width-generic kernel they replace */
    uint32_t acquisition;        /* 0 = segment-parallel acquisition, anchored on the state a push begins in while the traffic has a cadence;
                                    1 = one launch of segment waves, no anchor; 2 = no segment waves (the scouts walk every frame); 3 = an
                                    anchor phase in front of the segment waves, always (rounds 4-5: a launch that acquires every channel's first
                                    frame); 4 = no speculation at all (the round-1 scout: one kernel per push does everything); 5 = as 0 with
                                    the cadence taken for granted */
    uint32_t scout_build;        /* 0 = default: the general state machine's segment waves, the scouts' unbudgeted build; 1 = the scouts'
                                    168-register build of rounds 2-3; 2 = the lean segment waves of 48- / 64-subcarrier symbols
                                    (csrc/acq_lean.hpp: half the instructions, the same time on periodic traffic, 10 % behind on ragged) */
    uint32_t conv_scratch;       /* the K = 7 rate-1/2 decoder's scratch in HBM (512 bytes per trellis step and decoder wave: min(max_frames, 2048) waves x
                                    (32 max_payload_len + ~100) steps = 0.4 GB at 1200-byte payloads, 0.65 GB at the default 2048).  0 = allocated when
                                    the first frame with that code has been seen (the launch after the device reports it; until then such frames go
                                    through the block decoder of rounds 3-4: the same bytes on every frame that decodes, a fixed 192-step overlap
                                    instead of an exact one on frames that do not); 1 = with the handle (callers that know they will receive the code);
                                    2 = never.  An allocation that fails is not an error: the block decoder stays */
    uint32_t input_format;       /* wideband samples the handle takes: 0 = cf32 (interleaved float re, im; default), 1 = sc16 (interleaved int16 re, im,
                                    what radios deliver): half the bytes over the host link and into the channelizer, converted where its oscillator
                                    multiplies.  An sc16 sample (re, im) MEANS (re * 2^-15, im * 2^-15) -- exact in fp32 for every int16, -32768
                                    included, so an sc16 handle gives bit for bit what a cf32 handle gives on those floats.  (UHD's own sc16 -> fc32
                                    converter scales by 1 / 32767: the 3e-5 difference in gain is the caller's business.)  The format belongs to the
                                    handle: pushes go through mcrx_hip_execute_host_sc16 / _device_sc16, the plain calls return MCRX_EINVAL (and the
                                    _sc16 calls on a cf32 handle); mcrx_hip_channelize reads d_iq / d_halo in it.  Any other value: MCRX_EINVAL.
                                    Out of scope, refused with MCRX_EUNSUPP: sc16 with single_channel (no channelizer to convert in), with
                                    front_end = 2, and mcrx_hip_pipeline_create on an sc16 handle.  The C++ classes take std::complex<float> only */
} mcrx_hip_config;

/* One decoded frame = the arguments of the reference's framesync_callback
 * (include/multichannelrx.h:45) plus where it ended. */
typedef struct {
    uint32_t channel;
    int32_t  header_valid;
    int32_t  payload_valid;
    uint32_t payload_len;
    uint8_t  header[8];
    float    evm, rssi, cfo;                 /* framesyncstats_s */
    uint32_t mod_scheme, mod_bps, check, fec0, fec1;
    uint32_t num_framesyms;
    uint64_t end_sample;                     /* channel-rate sample index of the last symbol */
    const uint8_t *payload;                  /* payload_len bytes   (host memory owned by the handle, */
    const float   *framesyms;                /* 2*num_framesyms floats   valid until the next flush)  */
} mcrx_frame;

/* ---- receiver object ---------------------------------------------------------------- */
int  mcrx_hip_create(mcrx_hip_t *out, unsigned num_channels, unsigned M, unsigned cp_len,
                     unsigned taper_len, const unsigned char *p, const mcrx_hip_config *cfg);
int  mcrx_hip_destroy(mcrx_hip_t q);
int  mcrx_hip_reset(mcrx_hip_t q);
/* Channel-rate sample positions (mcrx_hip_reset_at, mcrx_hip_sync, mcrx_frame.end_sample) are 64-bit, but the synchronizers key
 * their speculation slots by a position packed into 48 bits (spec_key, csrc/ofdmsync.hip): every position a launch handles, the one
 * behind its last sample included, must stay below MCRX_POSITION_MAX.  A call that would pass it is refused with MCRX_EINVAL --
 * mcrx_hip_execute_* too, once the stream has run that far (an 8-channel receiver at 25 Msample/s: 5.7 years). */
#define MCRX_POSITION_MAX (1ll << 48)
/* the same for a handle driven through the stage-level calls (mcrx_hip_sync: it never learns the stream position by itself):
 * the synchronizers restart in SEEK at channel-rate sample `chan_position` (< MCRX_POSITION_MAX, else MCRX_EINVAL).  What
 * mcrx_hip_pipeline_reset calls. */
int  mcrx_hip_reset_at(mcrx_hip_t q, uint64_t chan_position);
unsigned mcrx_hip_num_channels(mcrx_hip_t q);

/* push wideband cf32 samples (interleaved re,im).  Any n; partial blocks are buffered.  MCRX_EOVERFLOW: the
 * samples were all processed but the frame pool filled up and frames were dropped (mcrx_hip_frames_dropped). */
int  mcrx_hip_execute_host(mcrx_hip_t q, const float *iq, size_t nsamples);
/* same with the samples already in device memory; `stream` is a hipStream_t (NULL = default).
 * nsamples must be a multiple of 2*num_channels.  Asynchronous, with a bounded lead: the call returns when the work is
 * enqueued, but waits first (once per turn of the handle's buffer sets) for the launch one turn back, so the host stays
 * within 2 * MCRX_SLOTS launches of the device and the acquisition's feedback words reach the next launches. */
int  mcrx_hip_execute_device(mcrx_hip_t q, const void *d_iq, size_t nsamples, void *stream);
/* the same two calls for a handle made with input_format = 1: nsamples sc16 samples = 2 * nsamples int16 (re, im interleaved).
 * Staging, the host-to-device copy and the channelizer's reads are half the cf32 calls'.  A call of the other format's kind
 * returns MCRX_EINVAL and processes nothing.
 * Alignment of device buffers: the channelizer fetches two samples per lane as one vector, so d_iq (and mcrx_hip_channelize's d_halo)
 * must be 16-byte aligned on a cf32 handle and 8-byte aligned on an sc16 handle (4 when num_channels = 1). */
int  mcrx_hip_execute_host_sc16(mcrx_hip_t q, const int16_t *iq, size_t nsamples);
int  mcrx_hip_execute_device_sc16(mcrx_hip_t q, const void *d_iq, size_t nsamples, void *stream);
unsigned mcrx_hip_input_format(mcrx_hip_t q);          /* the handle's mcrx_hip_config::input_format (0 for a null handle) */

/* wait for all pushed samples, gather decoded frames (ordered by end time, then channel). */
int  mcrx_hip_flush(mcrx_hip_t q);
/* Overlapped harvest for a stream that keeps coming (callbacks inside Execute, lib/multichannelrx.cc:193-194, at
 * slab granularity): gathers the frames of everything pushed before the poll BEFORE THE PREVIOUS one -- waiting only for those
 * launches -- and marks what was pushed since.  With one push + one poll per slab, slab k-2's frames cross the host link while
 * the GPU has slabs k-1 and k in flight (two, so that consecutive slabs keep overlapping on the device); flush delivers the rest. */
int  mcrx_hip_poll(mcrx_hip_t q);
/* as poll, but the frames are dropped on the device (no host wait, no copy): steady-state benchmarking.  Dropped frames are
 * never delivered by a later poll / flush. */
int  mcrx_hip_discard(mcrx_hip_t q);
/* make `stream` wait (on the device) for everything pushed so far, e.g. before a stage-level buffer is reused */
int  mcrx_hip_stream_wait(mcrx_hip_t q, void *stream);
/* ... or only for synchronizer launch number `launch` (0-based; mcrx_hip_launches() - 1 right after a
 * mcrx_hip_sync / execute_device call): what a rotating stage-level buffer needs before it is overwritten */
uint64_t mcrx_hip_launches(mcrx_hip_t q);
unsigned mcrx_hip_history_tiles(mcrx_hip_t q);      /* tiles of channel-rate history a mcrx_hip_sync buffer must start with */
int  mcrx_hip_stream_wait_launch(mcrx_hip_t q, uint64_t launch, void *stream);
/* frames the per-channel scouts acquired themselves / took over from speculative waves since the last reset of
 * the statistics (synchronises the device) */
int  mcrx_hip_spec_stats(mcrx_hip_t q, uint64_t *walked, uint64_t *adopted, int reset);
/* the K = 7 convolutional decoder (csrc/viterbi_frames.hpp: a frame per wave, a trellis block per lane, each block run from
 * an overlap and CHECKED against its neighbours): frames it decoded, forward passes and traceback passes it had to repeat because a
 * block's survivors had not merged inside the overlap (0 on any decodable signal; noise costs passes, never exactness).  Synchronises
 * the device. */
int  mcrx_hip_viterbi_stats(mcrx_hip_t q, uint64_t *frames, uint64_t *forward_repeats, uint64_t *traceback_repeats, int reset);
size_t mcrx_hip_frames_pending(mcrx_hip_t q);
int  mcrx_hip_next_frame(mcrx_hip_t q, mcrx_frame *out);      /* 1 = frame written, 0 = none */
/* a caller's delivery loop without a per-frame FFI crossing: walks every pending frame through mcrx_hip_next_frame,
 * touches its payload, and reports how many there were, how many with valid header and payload, and their payload bytes */
int  mcrx_hip_drain_count(mcrx_hip_t q, uint64_t *frames, uint64_t *valid, uint64_t *payload_bytes);
uint64_t mcrx_hip_frames_dropped(mcrx_hip_t q);

/* ---- channel monitor: "what is on the air?" ---------------------------------------------
 * Per channel of the handle's shard (channel_count, else all N): mean power, peak power and an averaged periodogram of the channel's
 * own sample stream, taken on the GPU from the channel tiles the synchronizers read -- whether or not anything decodes there.  It
 * stands in for the two small observation tools among the reference's applications: the text spectrogram that runs a 64-bin transform
 * behind the front-end resampler, and the program that logs the received signal level.  Definition ("Channel monitor"):
 * with x_c[n] the channel-rate samples counted from the last enable / reset (stage-level callers: from the first sample they pass),
 *   segment s = x_c[s nfft .. (s+1) nfft): aligned to the sample index, not to a push; one that straddles two pushes is completed by
 *   the later push, a trailing partial one is held back until its samples arrive;
 *   psd[c][k] = mean over whole segments of |sum_n w[n] x_c[s nfft + n] e^{-2 pi i k n / nfft}|^2 / sum_n w[n]^2, k in FFT order (0 = centre);
 *   level[c] = mean |x_c[n]|^2 and peak[c] = max |x_c[n]|^2 over every sample pushed.
 * Transform in fp32, sums in fp64, folded in a fixed order: the same pushes give the same bits.  Off in a new handle; while it is off
 * nothing is launched, recorded or allocated. */
typedef struct {
    uint32_t struct_size;        /* sizeof(mcrx_hip_monitor_config) */
    uint32_t nfft;               /* segment length: 16, 32, 64, 128 or 256; 0 -> 64 */
    uint32_t window;             /* 0 = rectangular, 1 = Hann 0.5 - 0.5 cos(2 pi n / nfft), 2 = Hamming 0.54 - 0.46 cos(2 pi n / nfft) */
} mcrx_hip_monitor_config;
/* switch the monitor on (NULL = defaults: 64 bins, rectangular).  MCRX_EINVAL on a bad nfft / window / handle.  Enabling a monitor
 * that is on starts it over: sums and the unfinished segment are dropped.  mcrx_hip_reset / _reset_at / _restart do the same. */
int  mcrx_hip_monitor_enable(mcrx_hip_t q, const mcrx_hip_monitor_config *cfg);
int  mcrx_hip_monitor_disable(mcrx_hip_t q);
/* level[nch], peak[nch], psd[nch][nfft] (any may be NULL), the whole segments and the samples they were taken over.  Waits for the
 * monitor's own launches only, not for the synchronizers.  MCRX_EINVAL while the monitor is off.  reset = 1 starts a new averaging
 * interval but KEEPS the unfinished segment, so that consecutive intervals tile the stream: one call per display interval is one row
 * of a waterfall. */
int  mcrx_hip_monitor_read(mcrx_hip_t q, double *level, float *peak, double *psd, uint64_t *nseg, uint64_t *nsamp, int reset);
unsigned mcrx_hip_monitor_nfft(mcrx_hip_t q);          /* segment length of the running monitor, 0 = off */

/* ---- stage level (multi-GPU split, parity tests, benchmarks) ------------------------- */
/* NCO + analysis bank on `nblocks` blocks of 2N samples.  `first_sample` is the absolute
 * index of d_iq[0] (NCO phase); d_halo holds the mcrx_hip_history_blocks() blocks preceding d_iq -- 13 = 2m - 1 for the
 * reference's bank, 27 for front_end = 1 -- (NULL = zeros).  Both are read in the handle's input format (cf32, or sc16 words).
 * Output layout: out[g][tile][c][MCRX_TILE] cf32 with channel = g*(N/groups)+c,
 * tile = block / MCRX_TILE; nblocks must be a multiple of MCRX_TILE. */
int  mcrx_hip_channelize(mcrx_hip_t q, const void *d_iq, size_t nblocks, uint64_t first_sample,
                         const void *d_halo, void *d_out, unsigned groups, void *stream);
/* run the synchronizer bank of this handle's channel shard over d_chan[tile][c][MCRX_TILE],
 * holding channel-rate samples [first_sample, first_sample + nsamples).  The buffer must
 * still contain the M+cp samples preceding the first unconsumed one.  MCRX_EINVAL unless first_sample + nsamples <
 * MCRX_POSITION_MAX. */
int  mcrx_hip_sync(mcrx_hip_t q, const void *d_chan, uint64_t first_sample, size_t nsamples, void *stream);

/* benchmark replay: discard undelivered frames and return the object to its
 * post-construction state (sample counters and NCO phase zero), asynchronously on `stream`. */
int  mcrx_hip_restart(mcrx_hip_t q, void *stream);

/* design data, for parity tests against the oracle */
int  mcrx_hip_get_taps(mcrx_hip_t q, float *h, size_t n);             /* p*K prototype taps */
uint32_t mcrx_hip_nco_step(mcrx_hip_t q);                             /* 32-bit phase increment */
unsigned mcrx_hip_history_blocks(mcrx_hip_t q);                       /* blocks of 2N samples of filter history in front of a push: 13 (27: front_end = 1) */
int  mcrx_hip_kernel_time_ms(mcrx_hip_t q, float *channelizer_ms, float *sync_ms); /* last launches */
/* summed HIP-event durations [ms] and launch counts since the last reset of the statistics, per
 * kernel: [0] channelizer_kernel, [1] sync_kernel (per-channel scout), [2] place_jobs_kernel,
 * [3] payload_kernel (per-frame symbol loop), [4] decode_kernel (per-frame packet decode).
 * Events are recorded on the launch stream; no host sync per launch -- and only while timing is switched on
 * (mcrx_hip_kernel_timing; off in a new handle: the five event pairs per push are ten more packets on the handle's
 * streams, 9 % of an 8-channel receiver's 0.25 ms push). */
#define MCRX_NKERNELS 5
int  mcrx_hip_kernel_stats(mcrx_hip_t q, double ms_total[MCRX_NKERNELS], uint64_t launches[MCRX_NKERNELS], int reset);
int  mcrx_hip_kernel_timing(mcrx_hip_t q, int on);                    /* returns the previous setting (-1: null handle) */

const char *mcrx_hip_last_error(void);

/* Devices.  A handle (receiver, resampler, bank, generator, pipeline) belongs to the HIP device that was current when it was created:
 * every entry point that touches the device makes that device current for the call and restores the caller's, and per-kernel device
 * settings (dynamic LDS limits) are made once per device, not once per process -- a host may open handles on several GPUs of one
 * process (the design and the benchmark use one process per GPU).  Device buffers and streams passed in must belong to the handle's device. */
int  mcrx_hip_device(mcrx_hip_t q);                    /* the handle's device index, -1 for a null handle */
int  mcrx_hip_selftest_device_table(void);             /* the once-per-device bookkeeping driven with made-up device ids: 0 = ok (no GPU needed) */

/* ---- multi-stage resampler: decimating front end (0 < rate <= 1) and the transmit side's interpolator
 *      (rate > 1: msresamp_crcf_create(2.0, 60), src/flexframe_tx.cc:170) -------------
 * Replaces msresamp_crcf_create(rate, As) / _execute / _destroy as the reference applications
 * call it in front of a synchronizer (src/flexframe_rx.cc:179,240,275; rate computed as in
 * src/multichannel_rx.cc:129-138).  Buffers are device pointers: input and output are cf32 or -- on a handle set to it,
 * msresamp_hip_set_input_format / msresamp_hip_set_output_format -- sc16.  `stream` is a hipStream_t; NULL = the legacy
 * default stream (so a receiver handle fed next, which orders against that stream, sees the samples written). */
typedef struct msresamp_hip_s *msresamp_hip_t;
int    msresamp_hip_create(msresamp_hip_t *out, float rate, float As);
int    msresamp_hip_destroy(msresamp_hip_t q);
int    msresamp_hip_reset(msresamp_hip_t q);
/* msresamp_hip_reset, but the stream continues from input sample `input_position` with zero history: as if that many zeros had
 * been consumed and their outputs discarded.  Any 64-bit position; MCRX_EINVAL unless it is a multiple of 2^num_stages (the
 * half-band stages in front of or behind the arbitrary one: one per halving of the rate below 1/2, per doubling above 2).
 * A running stream needs no such call: the phase arithmetic is periodic and never overflows, however long the stream. */
int    msresamp_hip_reset_at(msresamp_hip_t q, uint64_t input_position);
/* The delay of the chain IN INPUT SAMPLES OF THE HANDLE: a slow tone leaves as if the resampler had read input sample n - delay where
 * an ideal one reads sample n.  rate <= 1: d = 7 for the arbitrary stage, d = 2 d + 13 per half-band decimator in front of it.
 * rate > 1: 7 + (7 / rate_arb) * sum_{i < num_stages} 2^-i (the arbitrary stage's 7 input samples; half-band interpolator i adds 7
 * samples at rate_arb * 2^i times the input rate).  In output samples it is rate times as much.  0 for a null handle. */
float  msresamp_hip_get_delay(msresamp_hip_t q);
/* The plan of a rate, host only (no device is looked for): what msresamp_hip_create(rate, As) derives from the rate and uploads.
 * interp: rate > 1.  num_stages: the half-band stages.  rate_arb: the arbitrary stage's rate, in [1/2, 1] or (1, 2].
 * step = rint(2^24 / rate_arb): its input samples per output, 24 fractional bits.  per_in, per_out: one period of the phase,
 * per_in * 2^24 == per_out * step.  delay: msresamp_hip_get_delay.  h1: the half-band branch filter.  hpfb[b]: branch b of the
 * arbitrary stage, the tap on the OLDEST of its 14 samples first.  Set struct_size = sizeof(msresamp_hip_plan).
 * MCRX_EINVAL, with msresamp_hip_last_error set, for a null pointer, a wrong struct_size and every rate msresamp_hip_create refuses:
 * not positive, NaN, above 1024, or below 2^-38 -- more than 37 half-band stages, where the 64-bit sample counters of the first stage
 * no longer hold a period of the phase and a call (csrc/resamp_plan.hpp). */
typedef struct msresamp_hip_plan {
    uint32_t struct_size;
    uint32_t interp, num_stages, reserved;
    uint64_t step, per_in, per_out;
    double   rate_arb;
    float    delay;
    float    h1[14];
    float    hpfb[256][14];
} msresamp_hip_plan;
int    msresamp_hip_selftest(float rate, float As, msresamp_hip_plan *plan);
size_t msresamp_hip_max_output(msresamp_hip_t q, size_t nin);
int    msresamp_hip_execute_device(msresamp_hip_t q, const void *d_in, size_t nin, void *d_out,
                                   size_t out_cap, size_t *nout, void *stream);
/* Input format of the handle: 0 = cf32 (interleaved float re, im; the default), 1 = sc16 (interleaved int16 re, im, what radios
 * deliver: 4 bytes a sample, one 32-bit word with re in the low half -- the receiver's input_format = 1).  An sc16 sample (re, im) MEANS
 * (re * 2^-15, im * 2^-15) -- exact in fp32 for every int16, -32768 included -- and the first stage converts it where it stages its
 * input, so an sc16 handle gives bit for bit what a cf32 handle gives on those floats, fed in the same pieces, while the largest stream
 * the resampler reads is half the bytes.  (UHD's own sc16 -> fc32 converter scales by 1 / 32767: the 3e-5 difference in gain is the
 * caller's business.)  Everything behind the first stage stays cf32, up to the store of the output (below); reset_at, get_delay,
 * max_output and the periodic phase arithmetic do not depend on the format.
 * The format belongs to the handle: msresamp_hip_execute_device_sc16 takes nin sc16 samples = 2 * nin int16 and is otherwise
 * msresamp_hip_execute_device (*nout, out_cap, stream); a call of the other format's kind returns MCRX_EINVAL, consumes nothing and
 * leaves the state untouched.  msresamp_hip_set_input_format: MCRX_EINVAL for a null handle or any other value; MCRX_EBUSY while the
 * handle holds input history (its retained input samples are in the old format) -- allowed on a new handle and directly after
 * msresamp_hip_reset / _reset_at.
 * Alignment: d_in needs the alignment of one sample only -- 8 bytes for cf32, 4 bytes for sc16.  (Rates below 1/2 fetch an (even, odd)
 * pair of samples per lane as one vector where the pair's address allows it, 16 bytes for cf32 and 8 for sc16, and sample by sample
 * where it does not: a 16- / 8-byte aligned buffer fed in even-sized pieces stays on the vector path.)
 * Out of scope for both sc16 sides: a host-memory entry point, the C++ classes (std::complex<float> only) and the multi-GPU pipeline. */
int      msresamp_hip_set_input_format(msresamp_hip_t q, unsigned format);
unsigned msresamp_hip_input_format(msresamp_hip_t q);                               /* 0 for a null handle */
int      msresamp_hip_execute_device_sc16(msresamp_hip_t q, const void *d_in, size_t nin, void *d_out,
                                          size_t out_cap, size_t *nout, void *stream);
/* Output gain and output format of the handle (the transmit applications' msresamp(2.0) -> g * y -> radio, src/flexframe_tx.cc:170-243).
 * Let y be the fp32 value the resampler computes for one component of an output sample.  A handle has an output gain g (default 1) and
 * stores v = y * g: one fp32 multiply of its own, nothing fused into it; with g = 1 the output is y, word for word.  Output format
 * 0 = cf32 stores v (the default); 1 = sc16 stores Q(v), the transmitter's quantiser (mctx_hip_set_output_format):
 *   Q(v) = clamp(rint(v * 32768.0f), -32768, 32767)      round half to even, in fp32; NaN stores 0, infinities saturate
 * as interleaved int16 re, im -- 4 bytes a sample, the word input_format = 1 reads, with no scale factor in between.  The integers are
 * a function of the cf32 output alone.  A sample is CLIPPED when the rounded value of its re or its im lies outside the int16 range
 * (NaN does not count).
 * There are no new execute entry points: msresamp_hip_execute_device and _execute_device_sc16 (that name refers to the INPUT) write
 * *nout samples to d_out in the handle's output format; out_cap and *nout count samples in both formats, and msresamp_hip_max_output,
 * get_delay, reset_at and the periodic phase arithmetic do not change.
 * msresamp_hip_set_output_format: MCRX_EINVAL for a null handle or a value other than 0 and 1.  msresamp_hip_set_output_gain:
 * MCRX_EINVAL for a null handle or a gain that is not finite; the gain applies to both output formats.  No output state is retained
 * between calls -- every buffer between the stages is an input buffer and stays cf32, only the store to d_out knows format and gain --
 * so both may change between any two calls, in mid-stream too: there is no MCRX_EBUSY case.  The getters return 0 for a null handle.
 * msresamp_hip_clipped: *samples = the samples clipped by sc16-output calls since the count was last reset (reset = 1 starts a new
 * count; samples may be NULL) -- mctx_hip_clipped's semantics: a 64-bit device counter and an event recorded on the caller's stream
 * behind every sc16-output call, and the read waits for that event only.  Always 0 on a handle that never wrote sc16.  Counter and
 * event are allocated when sc16 output is first selected; a handle that never selects it allocates nothing.
 * Alignment of d_out: for sc16 that of one sample, 4 bytes (MCRX_EINVAL otherwise).  At rates above 2 the last stage writes an
 * (even, odd) pair of outputs per input: as one 8-byte word where d_out is 8-byte aligned and as two 4-byte stores where it is not,
 * the same choice for a whole call -- so a caller may append consecutive calls' outputs to one buffer.  cf32 output: as before. */
int      msresamp_hip_set_output_format(msresamp_hip_t q, unsigned format);
unsigned msresamp_hip_output_format(msresamp_hip_t q);                              /* 0 for a null handle */
int      msresamp_hip_set_output_gain(msresamp_hip_t q, float gain);
float    msresamp_hip_output_gain(msresamp_hip_t q);                                /* 0 for a null handle */
int      msresamp_hip_clipped(msresamp_hip_t q, uint64_t *samples, int reset);
/* Measurement aid: with `enable` set, every following execute call records HIP events around the launch of its first stage -- the
 * one kernel that reads the caller's samples -- and msresamp_hip_first_stage_ms returns the time between them for the last such call
 * (it waits for that kernel; MCRX_EINVAL when none has been timed).  Off by default: no events, no cost. */
int      msresamp_hip_time_first_stage(msresamp_hip_t q, int enable);
int      msresamp_hip_first_stage_ms(msresamp_hip_t q, float *ms);
const char *msresamp_hip_last_error(void);

/* ---- alternate front end: 2x-oversampled analysis bank --------------------------------
 * Replaces firpfbch2_crcf_create_kaiser(LIQUID_ANALYZER, M, m, As) / _execute / _destroy (liquid-dsp; the
 * channelizer BASELINE.json's north_star names -- liquid-usrp's own receiver uses the critically sampled bank,
 * lib/multichannelrx.cc:89-91).  M channels (a power of two here), every step consumes M/2 samples and
 * produces one sample on each of the M channels.  Stage-level operator on device buffers:
 * d_x[0] is absolute sample first_step * M/2 of the stream and is preceded in memory by `lead_samples`
 * valid samples of history (0 = cold start; 2*m*M covers the whole filter); d_out is [nsteps][M] cf32. */
typedef struct mcrx_hip_pfb2_s *mcrx_hip_pfb2_t;
int    mcrx_hip_pfb2_create(mcrx_hip_pfb2_t *out, unsigned num_channels, unsigned m, float As);
int    mcrx_hip_pfb2_destroy(mcrx_hip_pfb2_t q);
int    mcrx_hip_pfb2_get_taps(mcrx_hip_pfb2_t q, float *h, size_t n);        /* 2*m*M prototype taps */
int    mcrx_hip_pfb2_analyze(mcrx_hip_pfb2_t q, const void *d_x, size_t lead_samples, size_t nsteps,
                             uint64_t first_step, void *d_out, void *stream);
const char *mcrx_hip_pfb2_last_error(void);

/* ---- multi-GPU receive pipeline (one process per GPU) ----------------------------------------
 * The reference runs one multichannelrx on one host thread (lib/multichannelrx.cc:155-195).  Sharded: sub-slabs of
 * `sub_blocks` blocks of the wideband stream go round robin to the ranks (sub-slab u -> rank u % world); per round every
 * rank channelizes its sub-slab into per-destination groups, one grouped ncclSend / ncclRecv exchange over xGMI turns the
 * time shards into channel shards, and the rank's handle -- created with channel_first / channel_count = its shard of
 * N / world channels and defer_samples covering a frame -- synchronizes them; rounds overlap
 * (channelize(c+1) || exchange(c) || synchronizers(c-1)) on two streams of the pipeline's own plus the handle's, events only,
 * nothing waits on the host.  world == 1 is the same
 * code without the exchange.  RCCL is loaded at run time (librccl.so.1); the caller hands rank 0's 128-byte ncclUniqueId to
 * every rank (MPI_Bcast, a file, torch.distributed).  Frames surface through the handle (poll / flush / next_frame) on the
 * rank that owns their channel.  liquid-usrp_amd/sharding.py is the Python mirror of the same schedule. */
typedef struct mcrx_hip_pipeline_s *mcrx_hip_pipeline_t;
int      mcrx_hip_pipeline_unique_id(void *id128);                                   /* rank 0 */
int      mcrx_hip_pipeline_create(mcrx_hip_pipeline_t *out, mcrx_hip_t rx, int rank, int world, const void *unique_id128,
                                  size_t sub_blocks, unsigned nbuf /* rotating buffer sets, 0 = 3 */);
/* one round: d_iq_sub = this rank's sub-slab (sub_blocks * 2N cf32 in HBM), d_halo = the 13 blocks in front of it in the
 * stream (NULL = zeros: the stream's first sub-slab), after_stream = the hipStream_t that produced them: the round starts behind
 * what is enqueued there now.  NULL is the legacy default stream (it is waited for like any other: the pipeline's own streams are
 * non-blocking); MCRX_STREAM_READY = the buffers are complete, wait for nothing */
#define MCRX_STREAM_READY ((void *)(intptr_t)-1)
int      mcrx_hip_pipeline_push(mcrx_hip_pipeline_t p, const void *d_iq_sub, const void *d_halo, void *after_stream);
/* the same from host memory: iq_with_halo = the 13 blocks in front of this rank's sub-slab, then the sub-slab ((13 + sub_blocks) * 2N
 * cf32, contiguous; zeros in front of the stream's first sub-slab).  What the sharded multichannelrx class calls */
int      mcrx_hip_pipeline_push_host(mcrx_hip_pipeline_t p, const float *iq_with_halo);
/* Lifetime: iq_with_halo may be reused as soon as push_host returns -- it is copied to a pinned staging buffer before the call comes
 * back.  To skip that host copy, fill the buffer this call hands out ((13 + sub_blocks) * 2N cf32 = *nsamples; pinned; `nbuf` of them
 * rotate) and pass it to the next push_host.  Neither call waits for a round's kernels, only for the host-to-device copy of the push
 * `nbuf` rounds back. */
int      mcrx_hip_pipeline_host_buffer(mcrx_hip_pipeline_t p, float **buf, size_t *nsamples);
/* multichannelrx::Reset() for the sharded receiver (lib/multichannelrx.cc:135-153): called by every rank at the same point of the
 * stream.  The oscillator is not reset (:144) and runs on the samples of the stream, so the caller says how the samples it pushed
 * differ from the samples it was handed: extra_samples > 0 = handed but not pushed (a discarded partial round), < 0 = pushed but
 * never in the stream (zero padding that completed the last round so that everything before the Reset got synchronized).
 * Waits for everything pushed; decoded frames stay deliverable (poll / flush on the handle). */
int      mcrx_hip_pipeline_reset(mcrx_hip_pipeline_t p, int64_t extra_samples);
/* ranks of the RCCL communicator behind the exchange as RCCL counts them (ncclCommCount); 1 when world == 1 (no communicator);
 * -1 when the loaded RCCL does not export the call */
int      mcrx_hip_pipeline_comm_count(mcrx_hip_pipeline_t p);
int      mcrx_hip_pipeline_wait(mcrx_hip_pipeline_t p);                              /* host wait for everything pushed */
int      mcrx_hip_pipeline_time_exchange(mcrx_hip_pipeline_t p, int on);            /* HIP events around every exchange */
int      mcrx_hip_pipeline_exchange_ms(mcrx_hip_pipeline_t p, double *total_ms, uint64_t *rounds, int reset);
uint64_t mcrx_hip_pipeline_bytes_sent_per_round(mcrx_hip_pipeline_t p);             /* to OTHER ranks */
int      mcrx_hip_pipeline_destroy(mcrx_hip_pipeline_t p);
const char *mcrx_hip_pipeline_last_error(void);

/* ---- synthetic IQ source: multichanneltx on the GPU ------------------------------------
 * Replaces multichanneltx (lib/multichanneltx.cc:41-242: N x ofdmflexframegen -> 2N-channel
 * synthesis bank, m = 13 -> NCO mix-up) driven by the traffic loop of src/multichannel_tx.cc:
 * 163-213: frames back to back on every channel, header = [pid_hi, pid_lo, channel, 5 seeded
 * bytes], seeded payloads, soft gain.  The stream is written to device memory, as cf32 or as sc16
 * (mctx_hip_set_output_format). */
typedef struct mctx_hip_s *mctx_hip_t;
int    mctx_hip_create(mctx_hip_t *out, unsigned num_channels, unsigned M, unsigned cp_len,
                       unsigned taper_len, const unsigned char *p);
int    mctx_hip_destroy(mctx_hip_t q);
/* Output format of the wideband stream: 0 = cf32 (the default), 1 = sc16 -- 16-bit integer IQ, interleaved int16 re, im, 4 bytes a
 * sample in the same block order, which is the receiver's input_format = 1 as it stands (a sample means (re, im) * 2^-15; no scale
 * factor between the two).  Let v be the fp32 value a cf32 handle stores for one component, behind the oscillator and `gain`: an sc16
 * handle stores Q(v) = clamp(r, -32768, 32767), r = rint(v * 32768.0f) -- round half to even, in fp32, the multiply exact -- so the
 * integers are a function of the cf32 output alone.  NaN stores 0, infinities saturate.  `gain` therefore sets the level against the
 * full scale 1.0; a SAMPLE is clipped when r lies outside the range for its re or its im (NaN does not count).
 * On an sc16 handle mctx_hip_generate, _generate_ragged and _synthesize_tiles write nblocks * 2N samples of 4 bytes to d_iq (8-byte
 * aligned, else MCRX_EINVAL); everything else about them is unchanged.  The host paths that produce a block or a frame at a time --
 * mctx_hip_stream_begin / _update / _generate and mctx_hip_frame -- have no gain to put the full scale against and return
 * MCRX_EUNSUPP there.  Any other format value: MCRX_EINVAL, as is a null handle; MCRX_EBUSY once mctx_hip_stream_begin has run. */
int      mctx_hip_set_output_format(mctx_hip_t q, unsigned format);
unsigned mctx_hip_output_format(mctx_hip_t q);                                      /* 0 for a null handle */
/* Clipped samples of every sample-producing call on this handle since the last reset (reset = 1 starts a new count).  Waits for
 * those calls first (an event recorded on the caller's stream behind each).  Always 0 on a cf32 handle; samples may be NULL. */
int      mctx_hip_clipped(mctx_hip_t q, uint64_t *samples, int reset);
/* the quantiser Q of the kernels on n host floats (one component each): tests reach rounding ties and the saturation edges with it */
int      mctx_hip_selftest_quantise(const float *in, int16_t *out, size_t n);
/* blocks of 2N samples needed for `frames_per_channel` frames plus the filter tail (multiple of MCRX_TILE) */
size_t mctx_hip_blocks_for(mctx_hip_t q, unsigned frames_per_channel, unsigned payload_len,
                           int mod, int fec0, int fec1);
/* writes nblocks*2N samples to d_iq in the handle's output format (cf32: 8 bytes each, sc16: 4); the headers / payloads that were sent are returned in
 * hdr[ch][frame][8] and pay[ch][frame][payload_len] (host buffers, may be NULL) */
int    mctx_hip_generate(mctx_hip_t q, void *d_iq, size_t nblocks, unsigned frames_per_channel,
                         unsigned payload_len, int mod, int fec0, int fec1, float gain, uint32_t seed,
                         uint8_t *hdr, uint8_t *pay, void *stream);
/* Ragged traffic, the kind src/multichannel_txrx.cc:227-267 sends (every packet `rand() % payload_len` bytes, handed to
 * whichever channel is free): per channel, seeded, frames of len_lo .. len_hi payload bytes, 0 .. gap_max idle OFDM symbols
 * before each, with probability 1 / long_every (0: never) a silence of 16 .. 16 + long_max symbols instead; placed until the
 * stream is full.  Host outputs (may be NULL), sized for max_frames per channel: count[ch], hdr[ch][f][8], len[ch][f],
 * pay[ch][f][len_hi], start[ch][f] = block index of the frame's first sample. */
int    mctx_hip_generate_ragged(mctx_hip_t q, void *d_iq, size_t nblocks, unsigned max_frames, unsigned len_lo, unsigned len_hi,
                                unsigned gap_max, unsigned long_every, unsigned long_max, int mod, int fec0, int fec1,
                                float gain, uint32_t seed, uint32_t *count, uint8_t *hdr, uint32_t *len, uint8_t *pay,
                                uint64_t *start, void *stream);
/* Sharded form (the transmit side of src/multichannel_txrx.cc over several GPUs; mirror image of the receiver's
 * stage interface): frame generators are channel-sharded (multichanneltx.cc:230-242 steps N independent
 * ofdmflexframegen objects), the synthesis bank + oscillator (multichanneltx.cc:192-227) time-sharded.
 *   traffic_create    frames of channels [ch_first, ch_first+ch_count), the traffic recipe and seeds of
 *                     mctx_hip_generate; hdr[c][frame][8] / pay[c][frame][payload_len] may be NULL
 *   traffic_tiles     their channel-rate samples for blocks [first_block, first_block+nblocks) as granules
 *                     d_tiles[tile][c][8] (cf32; zeros before block 0 and after the last frame); nblocks % 8 == 0
 *   synthesize_tiles  d_tiles[groups][(lead+nblocks)/8][N/groups][8] (granules as received from `groups` channel
 *                     shards, covering blocks [first_block-lead, first_block+nblocks)) -> wideband samples of blocks
 *                     [first_block-keep, first_block+nblocks) into d_iq; lead >= 25 + keep blocks of filter history,
 *                     lead % 8 == 0.  Equals the same blocks of mctx_hip_generate's stream bit for bit. */
typedef struct mctx_hip_traffic_s *mctx_hip_traffic_t;
int    mctx_hip_traffic_create(mctx_hip_t q, mctx_hip_traffic_t *out, unsigned ch_first, unsigned ch_count,
                               unsigned frames_per_channel, unsigned payload_len, int mod, int fec0, int fec1,
                               uint32_t seed, uint8_t *hdr, uint8_t *pay, void *stream);
int    mctx_hip_traffic_destroy(mctx_hip_traffic_t t);
int    mctx_hip_traffic_tiles(mctx_hip_traffic_t t, long long first_block, size_t nblocks, void *d_tiles, void *stream);
int    mctx_hip_synthesize_tiles(mctx_hip_t q, const void *d_tiles, unsigned groups, long long first_block,
                                 size_t nblocks, size_t lead_blocks, size_t keep_blocks, float gain, void *d_iq,
                                 void *stream);
/* Streaming form = the class interface of lib/multichanneltx.cc, one call per reference method:
 *   stream_begin    starts streaming with frame slots for payloads up to max_payload_len (slots grow on demand)
 *   stream_ready    IsChannelReadyForData (:147-162): 1 ready, 0 frame still going out, <0 error
 *   stream_update   UpdateData (:165-189): assemble a frame for one channel (MCRX_EBUSY when not ready)
 *   stream_generate GenerateSamples (:192-227): the next 2N wideband samples into a host buffer
 *   stream_reset    Reset (:126-149): frames and filter state dropped, the oscillator keeps its phase
 * The GPU works one OFDM symbol period (M + cp calls of stream_generate) ahead, which is the
 * granularity at which the reference's own frame generators are stepped (:230-242). */
/* One frame of one frame generator at the channel rate = ofdmflexframegen_assemble + _writesymbol until the
 * last symbol, as ofdmtxrx::transmit_packet / assemble_frame + write_symbol drive it (lib/ofdmtxrx.cc:297-342,
 * 366-388): frame_len() samples (a whole number of M+cp symbols, tail symbol included), scaled by `gain`,
 * into a host buffer.  Works on any mctx handle (the channel count does not matter). */
size_t mctx_hip_frame_len(mctx_hip_t q, unsigned payload_len, int mod, int fec0, int fec1);
int    mctx_hip_frame(mctx_hip_t q, const uint8_t *header8, const uint8_t *payload, unsigned payload_len,
                      int mod, int fec0, int fec1, float gain, float *out, size_t out_cap_samples);
int    mctx_hip_stream_begin(mctx_hip_t q, unsigned max_payload_len);
int    mctx_hip_stream_ready(mctx_hip_t q, unsigned channel);
int    mctx_hip_stream_update(mctx_hip_t q, unsigned channel, const uint8_t *header8, const uint8_t *payload,
                              unsigned payload_len, int mod, int fec0, int fec1);
int    mctx_hip_stream_generate(mctx_hip_t q, float *buffer);
int    mctx_hip_stream_reset(mctx_hip_t q);
const char *mctx_hip_last_error(void);

/* ---- channel emulator: what lies between a transmitter and a receiver ---------------------
 * A stateful streaming operator on the wideband stream (the one mctx_hip_generate writes and mcrx_hip_execute_device / msresamp read):
 * sparse multipath, a carrier offset, white Gaussian noise, cf32 or sc16 out.  Everything is a function of the ABSOLUTE sample index n,
 * never of how the stream is cut into calls.  x[n] = the cf32 input, zero in front of the last reset; taps (d_i, a_i), i < T, in any order:
 *   s[n] = sum_{i<T} a_i x[n - d_i]                        in table order
 *   r[n] = s[n] exp(+j 2 pi th_n / 2^32)                   th_n = phase0 + cfo_step n mod 2^32; skipped when cfo_step == 0 && phase0 == 0
 *   v[n] = gain r[n] + noise_std w[n]                      w skipped (no random number drawn) when noise_std == 0
 *   out  = v[n] (cf32), or Q(v[n]) (sc16: mctx_hip_set_output_format's quantiser, interleaved int16 re, im)
 * Delays are wideband samples: with K = 2N channels a delay of K is one channel-rate sample, so taps at 0, K + 3, 3K put a three-ray,
 * frequency-selective channel inside every user channel.  w[n]: Philox4x32-10 with counter (lo32(n >> 1), hi32(n >> 1), 0, 0) and key
 * (lo32(seed), hi32(seed)); sample n takes the words w[j], w[j + 1], j = 2 (n & 1): u1 = ((w[j] >> 9) + 0.5) 2^-23, u2 = (w[j + 1] >> 8) 2^-24,
 * w[n] = sqrt(-2 ln u1) (cos 2 pi u2, sin 2 pi u2) -- unit variance per component.  The integers of an sc16 handle are Q of a cf32
 * handle's output exactly, and a stream cut anywhere gives the one-shot output bit for bit.
 * The handle keeps the 64-bit position of the next input sample and the last max d_i input samples (device memory); successive calls
 * must be ordered on the device (one stream, or events of the caller's).  In-place use is refused: the taps read behind the write front.
 * The rays are constants unless fading is switched on (mcrx_hip_chanfade_set, at the end of this block): then a_i becomes g_i(n) a_i. */
#define MCRX_CHANEMU_MAX_TAPS  8
#define MCRX_CHANEMU_MAX_DELAY 65535
typedef struct mcrx_hip_chanemu_s *mcrx_hip_chanemu_t;
typedef struct {
    uint32_t struct_size, num_taps;                         /* sizeof(mcrx_hip_chanemu_config); 1 .. MCRX_CHANEMU_MAX_TAPS */
    uint32_t delay[MCRX_CHANEMU_MAX_TAPS];                  /* <= MCRX_CHANEMU_MAX_DELAY wideband samples */
    float    tap_re[MCRX_CHANEMU_MAX_TAPS], tap_im[MCRX_CHANEMU_MAX_TAPS];
    uint32_t cfo_step, phase0;      /* 2^32 * cycles per wideband sample; start phase */
    float    gain, noise_std;       /* noise_std: per component (re and im each) */
    uint64_t seed;
    uint32_t output_format;         /* 0 = cf32, 1 = sc16 */
} mcrx_hip_chanemu_config;
/* MCRX_EINVAL (before a device is looked for): null pointers, a wrong struct_size, num_taps outside 1 .. 8, a delay above the maximum,
 * a tap, gain or noise_std that is not finite, a negative noise_std, another output_format. */
int      mcrx_hip_chanemu_create(mcrx_hip_chanemu_t *out, const mcrx_hip_chanemu_config *cfg);
int      mcrx_hip_chanemu_destroy(mcrx_hip_chanemu_t q);
int      mcrx_hip_chanemu_reset(mcrx_hip_chanemu_t q);                               /* zero history, position 0 */
/* zero history, the stream continues at absolute index `position` (any 64-bit value): phase and noise counter follow from it */
int      mcrx_hip_chanemu_reset_at(mcrx_hip_chanemu_t q, uint64_t position);
uint64_t mcrx_hip_chanemu_position(mcrx_hip_chanemu_t q);                            /* 0 for a null handle */
unsigned mcrx_hip_chanemu_output_format(mcrx_hip_chanemu_t q);                       /* 0 for a null handle */
/* n cf32 samples at d_in -> n samples at d_out in the handle's output format, asynchronously on `stream` (a hipStream_t, NULL = the
 * default stream); at most 2^32 samples a call.  MCRX_EINVAL: a null handle or buffer, d_in not 8-byte aligned, d_out not 8-byte (cf32) /
 * 4-byte (sc16) aligned, ranges that overlap.  (Pairs of samples go as 16-byte (sc16 out: 8-byte) words where the addresses allow.) */
int      mcrx_hip_chanemu_execute_device(mcrx_hip_chanemu_t q, const void *d_in, size_t n, void *d_out, void *stream);
/* mctx_hip_clipped's semantics: a 64-bit device counter, an event recorded on the caller's stream behind every sc16 call, and the read
 * waits for that event only.  Counter and event exist only on a handle created with sc16 output; always 0 on a cf32 handle. */
int      mcrx_hip_chanemu_clipped(mcrx_hip_chanemu_t q, uint64_t *samples, int reset);
/* host: the two Philox words sample `position` draws under `seed` (the same code the kernel compiles; needs no GPU) */
int      mcrx_hip_chanemu_selftest_words(uint64_t seed, uint64_t position, uint32_t out[2]);
const char *mcrx_hip_chanemu_last_error(void);

/* ---- channel emulator: fading rays (Rayleigh / Rician with Doppler) ----
 * With fading on, ray i of the emulator is multiplied by a complex gain g_i(n) -- still a function of the ABSOLUTE output index n alone,
 * so a stream cut anywhere stays bit-identical to one call and the sc16 integers stay Q of the cf32 output.  With fading off (the state
 * of a new handle, and after a NULL) the emulator is the one described above, word for word.
 *   B = 2^log2_block wideband samples is the update interval of the gains; b = n >> log2_block the grid row, n_b = (b << log2_block)
 *   mod 2^64; e(p) of a 64-bit phase p is (cos, sin)(2 pi (p >> 32) / 2^32).  Per ray i, with S = num_sinusoids scattered sinusoids:
 *     G_i[b] = c_los_i e((psi_i << 32) + Lambda_i n_b) + c_sc_i sum_{k<S} e((Phi_ik << 32) + N_ik n_b)        phases mod 2^64
 *     g_i(n) = G_i[b] + f (G_i[b+1] - G_i[b]),   f = (n & (B - 1)) 2^-log2_block                               linear, by definition
 *     s[n]   = sum_{i<T} (g_i(n) a_i) x[n - d_i]                                                               table order
 *   The gain is indexed by the output time n, not by n - d_i.  Rotation, gain, noise and quantiser behind s[n] are unchanged.
 * The integers are made on the host from `seed`: the Philox4x32-10 words of counter (k, i, 1, 0) and key (lo32(seed), hi32(seed)) give the
 * stratified arrival angle alpha_ik = 2 pi (k + w0 2^-32) / S and the phase Phi_ik = w1; N_ik = rint(doppler_i cos(alpha_ik) 2^64),
 * Lambda_i = rint(los_doppler_i 2^64), psi_i = los_phase_i; c_los_i = sqrt(K_i / (K_i + 1)), c_sc_i = sqrt(1 / ((K_i + 1) S)) with
 * K_i = rice_k[i] the linear Rice factor, so that E|g_i|^2 = 1: K = 0 is Rayleigh (Jakes' spectrum of width doppler_i), a large K a
 * specular ray with a Doppler shift.  Linear interpolation between grid rows is part of the definition: against the sample-exact sum of
 * sinusoids it deviates by about (pi f_d B)^2 / 2 (1.2e-3 at f_d B = 1/64), so choose log2_block for the Doppler at hand.
 * The handle keeps a table of gains in device memory (64 bytes a row), grown to what a call needs up to table_rows rows (0: 2^18 rows,
 * 16 MB); a call that needs more is processed in consecutive spans on the caller's stream, which changes no bit of the output.
 * (These three functions do not carry the emulator's prefix: its set of entry points is closed.  Errors are read with
 * the emulator's last_error function.) */
#define MCRX_CHANEMU_MAX_SINUSOIDS 16
typedef struct {
    uint32_t struct_size, log2_block, num_sinusoids, table_rows;   /* sizeof(mcrx_hip_chanemu_fading); 1 .. 24; 1 .. 16; 0 = default, else >= 2 */
    double   doppler[MCRX_CHANEMU_MAX_TAPS];       /* f_d >= 0, cycles per wideband sample */
    double   los_doppler[MCRX_CHANEMU_MAX_TAPS];   /* signed, cycles per wideband sample */
    float    rice_k[MCRX_CHANEMU_MAX_TAPS];        /* linear, >= 0, finite */
    uint32_t los_phase[MCRX_CHANEMU_MAX_TAPS];     /* 2^32 * cycles */
    uint64_t seed;
} mcrx_hip_chanemu_fading;
/* f == NULL: fading off.  Holds no stream state: it may be called between any two execute calls, needs no synchronisation with calls in
 * flight, and entries beyond the handle's num_taps are ignored.  MCRX_EINVAL, before any device work: a null handle, a wrong struct_size,
 * log2_block outside 1 .. 24, num_sinusoids outside 1 .. 16, table_rows == 1, a Doppler that is not finite, a negative doppler,
 * doppler * B > 1/8 or |los_doppler| * B > 1/8 (the grid must sample the gain), a rice_k that is negative or not finite. */
int      mcrx_hip_chanfade_set(mcrx_hip_chanemu_t q, const mcrx_hip_chanemu_fading *f);
int      mcrx_hip_chanfade_on(mcrx_hip_chanemu_t q);                                 /* 1 with fading on; 0 for a null handle */
/* host, no GPU: the integers and coefficients ray `ray` (< MCRX_CHANEMU_MAX_TAPS) gets -- steps[0] / phases[0] the line-of-sight term,
 * then the num_sinusoids scattered ones (1 + num_sinusoids entries each); coef = { c_los, c_sc }.  Checks `f` as set does, for that ray. */
int      mcrx_hip_chanfade_selftest(const mcrx_hip_chanemu_fading *f, unsigned ray, int64_t *steps, uint32_t *phases, float coef[2]);

/* The gain kernel on its own, for tests and measurements: G_i[first_row + r], r < rows, of the handle's rays as float2 [rows][MCRX_CHANEMU_MAX_TAPS]
 * (entries of rays >= num_taps are not written) into the caller's device buffer, asynchronously on `stream`.  MCRX_EINVAL with fading off. */
int      mcrx_hip_chanfade_gains(mcrx_hip_chanemu_t q, uint64_t first_row, uint32_t rows, void *d_table, void *stream);

/* ---- per-user channel emulator on the transmitter's channel tiles ----
 * Sits between mctx_hip_traffic_tiles and mctx_hip_synthesize_tiles: every channel of the bank gets its own multipath, its own
 * oscillator, its own timing and its own level, at the channel rate, before the synthesis bank -- which is what puts a strong user next
 * to a weak one through the bank's skirts.  x_c[b] is the channel-rate sample of local channel c at absolute block index b (a signed
 * 64-bit value; one block = one channel-rate sample per channel).  Channel c has T_c rays (d_ci, a_ci), a gain_c, a 32-bit phase step
 * cfo_step_c per channel-rate sample and a start phase phase0_c:
 *   s_c[b] = sum_{i<T_c} a_ci x_c[b - d_ci]                  table order, two fused multiply-adds per ray and component
 *   r_c[b] = s_c[b] exp(+j 2 pi th / 2^32)                   th = phase0_c + cfo_step_c (uint32_t)(uint64_t)b  mod 2^32
 *   y_c[b] = gain_c r_c[b]                                   one fp32 multiply per component
 * Stateless: a pure function of the absolute block index and of the input it is handed; the handle keeps no history, no position and no
 * device state beyond the parameter table.  The samples behind a call are supplied by the caller, the way synthesize_tiles takes its
 * lead: d_in holds granules [tile][channel][8] (cf32, traffic_tiles' layout for num_channels channels) of blocks
 * [first_block - lead_blocks, first_block + nblocks), d_out receives blocks [first_block, first_block + nblocks) in the same layout;
 * lead_blocks, nblocks and first_block are multiples of 8 and lead_blocks >= mcrx_hip_userchan_lead_blocks().  What the input holds in
 * front of block 0 is the caller's business (traffic_tiles writes zeros there).  A stream cut into calls anywhere, with any sufficient
 * lead, gives the one-call output bit for bit.
 * Rotation: when every channel of the handle has cfo_step == 0 && phase0 == 0 the rotation is not computed at all (s_c goes to the gain
 * as it is); otherwise EVERY channel of the handle is rotated, those with a zero step and phase by the oscillator value of phase 0.
 * A user's integer timing offset is a delay added to all of their rays; a fractional one, and a sample clock of their own, are
 * mcrx_hip_userclock_* below.
 * At most 2^28 granules (tiles * channels) a call. */
#define MCRX_USERCHAN_MAX_RAYS     4
#define MCRX_USERCHAN_MAX_DELAY    255      /* channel-rate samples */
#define MCRX_USERCHAN_MAX_CHANNELS 1024
typedef struct mcrx_hip_userchan_s *mcrx_hip_userchan_t;
typedef struct {
    uint32_t num_rays;                                      /* 1 .. MCRX_USERCHAN_MAX_RAYS */
    uint32_t delay[MCRX_USERCHAN_MAX_RAYS];                 /* <= MCRX_USERCHAN_MAX_DELAY channel-rate samples */
    float    tap_re[MCRX_USERCHAN_MAX_RAYS], tap_im[MCRX_USERCHAN_MAX_RAYS];
    float    gain;
    uint32_t cfo_step, phase0;      /* 2^32 * cycles per channel-rate sample; start phase */
} mcrx_hip_userchan_channel;
/* ch[num_channels], struct_size = sizeof(mcrx_hip_userchan_channel).  MCRX_EINVAL (before a device is looked for): null pointers, a
 * wrong struct_size, num_channels outside 1 .. 1024, num_rays outside 1 .. 4, a delay above the maximum, a tap or gain that is not
 * finite (entries beyond a channel's num_rays are not looked at).  The handle belongs to the HIP device current at creation. */
int         mcrx_hip_userchan_create(mcrx_hip_userchan_t *out, unsigned num_channels, const mcrx_hip_userchan_channel *ch,
                                     size_t struct_size);
int         mcrx_hip_userchan_destroy(mcrx_hip_userchan_t q);
unsigned    mcrx_hip_userchan_num_channels(mcrx_hip_userchan_t q);                   /* 0 for a null handle */
unsigned    mcrx_hip_userchan_lead_blocks(mcrx_hip_userchan_t q);                    /* largest delay rounded up to 8 (with a clock on: see mcrx_hip_userclock_*); 0 for a null handle */
/* Asynchronous on `stream` (a hipStream_t, NULL = the default stream).  MCRX_EINVAL: a null handle or buffer, a buffer that is not
 * 16-byte aligned, nblocks, lead_blocks or first_block not a multiple of 8, lead_blocks below mcrx_hip_userchan_lead_blocks(), input
 * and output ranges that overlap, more than 2^28 granules. */
int         mcrx_hip_userchan_apply_tiles(mcrx_hip_userchan_t q, const void *d_in, long long first_block, size_t nblocks,
                                          size_t lead_blocks, void *d_out, void *stream);
const char *mcrx_hip_userchan_last_error(void);

/* ---- per-user channel emulator: fading rays per user (Rayleigh / Rician with Doppler) ----
 * With fading on, ray i of local channel c is multiplied by a complex gain g_ci(b) -- a function of the ABSOLUTE output block index b
 * (signed 64-bit) alone, so cuts, leads and channel shards stay invisible bit for bit.  With fading off (the state of a new handle, and
 * after a NULL) the operator is the one described above, word for word, and launches the same kernels.
 *   B = 2^log2_block blocks is the update interval; row = b >> log2_block (arithmetic: negative b works), n_r = (uint64_t)(row <<
 *   log2_block) mod 2^64, f = (b & (B - 1)) 2^-log2_block; e(p) of a 64-bit phase p is (cos, sin)(2 pi (p >> 32) / 2^32).
 *     G_ci[row] = c_los_ci e((psi_ci << 32) + Lambda_ci n_r) + c_sc_ci sum_{k<S} e((Phi_cik << 32) + N_cik n_r)     phases mod 2^64
 *     g_ci(b)   = G_ci[row] + f (G_ci[row+1] - G_ci[row])                                                          linear, by definition
 *     s_c[b]    = sum_{i<T_c} (g_ci(b) a_ci) x_c[b - d_ci]                                                         table order
 *   The gain is indexed by the output time b, not by b - d_ci.  Rotation and gain behind s_c[b] are unchanged.
 * log2_block >= 3: granules are 8 blocks and first_block is a multiple of 8, so a granule never straddles a grid row.
 * The integers are made on the host as the wideband emulator's are (mcrx_hip_chanfade_*), from the Philox4x32-10 words of counter
 * (k, i, 2, id_c) and key (lo32(seed), hi32(seed)): the third word keeps them apart from the wideband emulator's (k, i, 1, 0), and id_c
 * is the user's own -- a channel shard that keeps its users' ids reproduces their channels of the whole table bit for bit.
 * Dopplers are cycles per channel-rate sample.  A user with enabled == 0 has c_los = 1, c_sc = 0, zero steps and phases: G = (1, 0),
 * and their output equals that of a handle without fading (only the sign of a zero may differ).
 * The handle keeps the sinusoids' integers and a table of gains in device memory: float2 [row][channel][4], 32 bytes a channel and
 * row, grown to the (((first_block & (B - 1)) + nblocks - 1) >> log2_block) + 2 rows a call needs, up to table_rows rows
 * (0: the most rows that fit 64 MiB for the handle's channel count); a longer call runs as consecutive spans on the caller's stream,
 * each cut at a multiple of 8 blocks, which changes no bit of the output.  Because of that table, calls of
 * mcrx_hip_userchan_apply_tiles on ONE fading handle must be ordered on the device (one stream, or events of the caller's); handles
 * without fading stay free of this.  (These functions do not carry the emulator's prefix: its set of entry points is closed.  Errors
 * are read with mcrx_hip_userchan_last_error.) */
#define MCRX_USERFADE_MIN_LOG2_BLOCK 3
#define MCRX_USERFADE_MAX_LOG2_BLOCK 20
typedef struct {
    uint32_t enabled, id;                            /* 0: this user does not fade (the rest is not looked at); the user's id_c */
    double   doppler[MCRX_USERCHAN_MAX_RAYS];        /* f_d >= 0, cycles per channel-rate sample */
    double   los_doppler[MCRX_USERCHAN_MAX_RAYS];    /* signed, cycles per channel-rate sample */
    float    rice_k[MCRX_USERCHAN_MAX_RAYS];         /* linear, >= 0, finite */
    uint32_t los_phase[MCRX_USERCHAN_MAX_RAYS];      /* 2^32 * cycles */
} mcrx_hip_userfade_user;
typedef struct {
    uint32_t struct_size, user_struct_size;          /* sizeof(mcrx_hip_userfade_config), sizeof(mcrx_hip_userfade_user) */
    uint32_t log2_block, num_sinusoids;              /* 3 .. 20; 1 .. MCRX_CHANEMU_MAX_SINUSOIDS */
    uint32_t table_rows, reserved;                   /* 0 = default, else >= 2; reserved: 0 */
    uint64_t seed;
} mcrx_hip_userfade_config;
/* users[num_channels of the handle]; f == NULL: fading off (users is not looked at).  Waits for the device before it replaces the
 * handle's tables.  MCRX_EINVAL, before any device work and with the handle left as it was: a null handle, a null users with f given,
 * wrong struct sizes, log2_block outside 3 .. 20, num_sinusoids outside 1 .. 16, table_rows == 1, and for a ray (< num_rays) of an
 * enabled user a Doppler that is not finite, a negative doppler, doppler * B > 1/8 or |los_doppler| * B > 1/8 (the grid must sample
 * the gain), a rice_k that is negative or not finite. */
int      mcrx_hip_userfade_set(mcrx_hip_userchan_t q, const mcrx_hip_userfade_config *f, const mcrx_hip_userfade_user *users);
int      mcrx_hip_userfade_on(mcrx_hip_userchan_t q);                                /* 1 with fading on; 0 for a null handle */
/* host, no GPU: the integers and coefficients ray `ray` (< MCRX_USERCHAN_MAX_RAYS) of user *u gets -- steps[0] / phases[0] the
 * line-of-sight term, then the num_sinusoids scattered ones (1 + num_sinusoids entries each); coef = { c_los, c_sc }.  Checks `f` and
 * that ray of `u` as set does. */
int      mcrx_hip_userfade_selftest(const mcrx_hip_userfade_config *f, const mcrx_hip_userfade_user *u, unsigned ray, int64_t *steps,
                                    uint32_t *phases, float coef[2]);
/* The gain kernel on its own, for tests and measurements: G_ci[first_row + r], r < rows, as float2 [rows][num_channels][4] into the
 * caller's 16-byte aligned device buffer, asynchronously on `stream` (entries of rays a channel does not have are (1, 0)).
 * MCRX_EINVAL with fading off. */
int      mcrx_hip_userfade_gains(mcrx_hip_userchan_t q, long long first_row, uint32_t rows, void *d_table, void *stream);

/* ---- per-user channel emulator: each user's own sample clock and fractional timing ----
 * A user's radio has one oscillator: the error that moves their carrier (cfo_step) also moves their sample clock.  With a clock on,
 * local channel c transmits z_c[b] = x_c(b - tau_c(b)) instead of x_c[b], IN FRONT of their multipath, and the operator above runs
 * on z unchanged (rays, fading gains, rotation, gain):  s_c[b] = sum_i (g_ci(b)) a_ci z_c[b - d_ci].
 * The delay is a straight line in the ABSOLUTE output block index b (signed 64-bit), all in integers:
 *     tau_fp_c(b) = delay_fp_c + floor( sco_c * (b - origin_c) / 2^16 )        Q32 samples, int64 (an arithmetic shift: floor)
 *     n  = tau_fp >> 32          whole samples
 *     mu = tau_fp & 0xffffffff   fraction
 *   delay_fp: the delay at b = origin in units of 2^-32 samples; sco: signed, units of 2^-48 samples per sample (1 ppm = 281 474 977),
 *   |sco| <= 2^38 (about 977 ppm); origin: a signed 64-bit block index.
 * z is interpolated by a 32-tap polyphase filter of 64 phases with linear interpolation between phases (part of the definition, as
 * the fading gains' is of theirs), in fp32, summed in the order j = 0 .. 31 from zero with one fused multiply-add per tap and component:
 *     z_c[b]  = sum_{j<32} h_j(mu) x_c[b - n + 15 - j]                          z is ROUNDED TO fp32 here
 *     h_j(mu) = fmaf(f, W[r+1][j] - W[r][j], W[r][j])                           r = mu >> 26, f = ((mu >> 2) & 0xffffff) 2^-24 (exact)
 *     W[p][j] = fp32( sinc(t) I0(6.0 sqrt(1 - (t/16)^2)) / I0(6.0) ),  t = j - 15 - p/64,  p = 0 .. 64, computed in double; rows 0 and
 *               64 are set to the exact unit vectors (tap 15, tap 16); mcrx_hip_userclock_table reports W.
 * The taps reach 15 samples ahead of b - n, so n >= MCRX_USERCLOCK_MIN_DELAY on every block of a call, and n <= the configured
 * max_delay (15 .. 255).  tau is linear over a call, so the host checks the two ends -- blocks first_block - D and first_block +
 * nblocks - 1, D the handle's largest ray delay (0 for mcrx_hip_userclock_apply_tiles) -- and refuses the call with MCRX_EINVAL,
 * before anything is launched and with a message naming the channel, when a clocked user's n leaves [15, max_delay] there or when
 * sco * (b - origin) leaves int64.  This is the documented limit: all users' traffic comes on one block grid, so a drift can use up
 * only the room max_delay gives it (at 20 ppm, 200 samples of room are 10^7 blocks); a longer run moves origin, which is a timing
 * jump, as a real user's re-synchronisation is.  A user with enabled == 0 has z = x, bit for bit.
 * Lead: with a clock on mcrx_hip_userchan_lead_blocks() is the largest ray delay + max_delay + 16 rounded up to 8, and
 * mcrx_hip_userclock_lead_blocks() is max_delay + 16 rounded up to 8 (the stage alone); with the clock off the first is as above and
 * the second 0.  Cuts, leads, spans and channel shards stay invisible bit for bit; with the clock off (a new handle, and after a
 * NULL) the operator is the one described above, word for word, and launches the same kernels.
 * The handle keeps z of a span in a scratch buffer of its own, grown on demand to span_blocks blocks (0: what fits 64 MiB for the
 * handle's channel count; else a multiple of 8) plus the rays' lead; a longer call runs as consecutive spans on the caller's stream,
 * which changes no bit.  Because of that buffer, calls of mcrx_hip_userchan_apply_tiles on ONE clocked handle must be ordered on the
 * device (one stream, or events of the caller's), as on a fading handle.  (A prefix of its own: the emulator's set of entry points
 * is closed.  Errors are read with mcrx_hip_userchan_last_error.) */
#define MCRX_USERCLOCK_TAPS      32
#define MCRX_USERCLOCK_PHASES    64
#define MCRX_USERCLOCK_MIN_DELAY 15
#define MCRX_USERCLOCK_MAX_DELAY 255
typedef struct {
    uint32_t enabled, reserved;     /* 0: this user has no clock of their own, z = x (the rest is not looked at) */
    uint64_t delay_fp;              /* 2^-32 samples, at b = origin */
    int64_t  sco, origin;           /* 2^-48 samples per sample, |sco| <= 2^38; a block index */
} mcrx_hip_userclock_user;          /* 32 bytes */
typedef struct {
    uint32_t struct_size, user_struct_size;     /* sizeof(mcrx_hip_userclock_config), sizeof(mcrx_hip_userclock_user) */
    uint32_t max_delay;                         /* 15 .. 255: the most whole samples of delay any block may have */
    uint32_t span_blocks;                       /* 0 = default, else a multiple of 8 */
} mcrx_hip_userclock_config;
/* users[num_channels of the handle]; cfg == NULL: the clock off (users is not looked at).  Waits for the device before the handle's
 * tables change.  MCRX_EINVAL, before any device work and with the handle left as it was: a null handle, a null users with cfg
 * given, wrong struct sizes, max_delay outside 15 .. 255, a span_blocks that is not a multiple of 8, and for an enabled user
 * |sco| > 2^38 or a delay_fp whose n lies outside [15, max_delay]. */
int      mcrx_hip_userclock_set(mcrx_hip_userchan_t q, const mcrx_hip_userclock_config *cfg, const mcrx_hip_userclock_user *users);
int      mcrx_hip_userclock_on(mcrx_hip_userchan_t q);                               /* 1 with a clock on; 0 for a null handle */
unsigned mcrx_hip_userclock_lead_blocks(mcrx_hip_userchan_t q);                      /* max_delay + 16 rounded up to 8; 0 with the clock off */
/* host, no GPU: the integer delay tau_fp and the 32 interpolated coefficients h_j this user's block `block` gets.  Checks cfg and user
 * as set does, and the block as a call does (n outside [15, max_delay] there, a product beyond int64: MCRX_EINVAL, nothing written).
 * A user with enabled == 0 gets tau_fp = 0 and the unit vector of tap 15. */
int      mcrx_hip_userclock_selftest(const mcrx_hip_userclock_config *cfg, const mcrx_hip_userclock_user *user, long long block,
                                     int64_t *tau_fp, float h[MCRX_USERCLOCK_TAPS]);
int      mcrx_hip_userclock_table(float W[(MCRX_USERCLOCK_PHASES + 1) * MCRX_USERCLOCK_TAPS]);      /* host: W[p][j] */
/* The clock stage on its own, for tests and measurements: z of blocks [first_block, first_block + nblocks) in the tiles' layout into
 * d_out, from d_in holding blocks [first_block - lead_blocks, first_block + nblocks); lead_blocks >= mcrx_hip_userclock_lead_blocks();
 * alignment, granules, overlap and size rules as for mcrx_hip_userchan_apply_tiles.  MCRX_EINVAL with the clock off. */
int      mcrx_hip_userclock_apply_tiles(mcrx_hip_userchan_t q, const void *d_in, long long first_block, size_t nblocks,
                                        size_t lead_blocks, void *d_out, void *stream);

/* ---- RF front end on the wideband stream: IQ imbalance and LO leakage, oscillator phase noise, amplifier ----
 * The radios at either end of the air: what couples one user's signal into another user's channel.  Memoryless in the samples and
 * STATELESS: the caller passes the absolute index of the first sample (any 64-bit value), so a stream cut anywhere, a time shard on any
 * GPU and any launch geometry give the bits of one call.  x[n] is the input, cf32 or sc16 (a word means (re, im) * 2^-15).  Three
 * stages, each switched by a bit of `stages` (a stage that is off is not computed at all), in the sequence `order` sets:
 *   order = 0 (a transmitter): mixer, oscillator, amplifier         order = 1 (a receiver): amplifier, oscillator, mixer
 * z is a stage's input and u its output, all fp32, every product that matters one fmaf:
 * Mixer (MCRX_RFCHAIN_MIXER): u = alpha z + beta conj(z) + d -- IQ imbalance (the image of channel c lands in channel N - 1 - c, its
 *   rejection is |alpha|^2 / |beta|^2) and LO leakage d:
 *     u.re = fmaf(alpha.re, z.re, fmaf(-alpha.im, z.im, fmaf(beta.re, z.re, fmaf( beta.im, z.im, d.re))))
 *     u.im = fmaf(alpha.re, z.im, fmaf( alpha.im, z.re, fmaf(beta.im, z.re, fmaf(-beta.re, z.im, d.im))))
 * Oscillator (MCRX_RFCHAIN_OSCILLATOR): u = z e(theta(n)), a stationary phase noise common to all channels, a function of the sample
 *   index: a sum of S = pn_sinusoids sinusoids sampled on the grid n = b 2^L (L = pn_log2_block, B = 2^L) and interpolated linearly
 *   between its rows -- linear interpolation of the angle is part of the definition, as it is for the fading gains.  In turns:
 *     Theta[b] = sum_{k<S} c cos 2 pi ((((Phi_k << 32) + N_k n_b) mod 2^64) >> 32) / 2^32      n_b = (b << L) mod 2^64; from 0.0f, k
 *                                                                                             ascending, acc = fmaf(c, cos_k, acc)
 *     theta(n) = fmaf(f, Theta[b+1] - Theta[b], Theta[b])                                     b = n >> L, f = (n & (B - 1)) 2^-L (exact)
 *     p        = (uint32_t)(int32_t)rintf(theta * 2^32),  (sn, cs) = sincos of the 32-bit phase p (the emulators' sincos_u32)
 *     u.re = fmaf(z.re, cs, -(z.im * sn)),  u.im = fmaf(z.re, sn, z.im * cs)                  the channel emulator's rotation
 *   c = pn_rms sqrt(2 / S) / (2 pi) rounded to fp32 on the host (pn_rms in radians: the rms of theta).  The integers are made on the
 *   host from pn_seed: the Philox4x32-10 words w0, w1 of counter (k, 0, 3, 0) and key (lo32(seed), hi32(seed)) (third counter word: 0 is
 *   noise, 1 the wideband emulator's fading, 2 the users' fading) give u_k = (k + (w0 + 0.5) 2^-32) / S, f_k = clamp(pn_bandwidth
 *   tan(pi (u_k - 1/2)), -1/(8B), +1/(8B)) -- a stratified draw from a Lorentzian line of half-width pn_bandwidth cycles per sample --
 *   N_k = rint(f_k 2^64) (int64) and Phi_k = w1.
 *   Theta lives in a table the handle owns (a row is one float), written by a kernel of its own in front of the samples' kernel and
 *   grown on demand up to pn_table_rows rows (0: 2^18); a call that needs more runs as consecutive spans on the caller's stream, which
 *   changes no bit of the output.  Because of that table, calls on ONE handle with the oscillator on must be ordered on the device
 *   (one stream, or events of the caller's); handles without it are free of this.
 * Amplifier (MCRX_RFCHAIN_AMPLIFIER): memoryless, Rapp AM/AM and a Saleh-shaped AM/PM, A = amp_sat, p = amp_smooth (1, 2 or 4):
 *     t = fmaf(z.re, z.re, z.im * z.im) * r             r = fp32(1 / A^2), made on the host (the division in double)
 *     q = 1 + t (p = 1);  sqrtf(fmaf(t, t, 1)) (p = 2);  sqrtf(sqrtf(fmaf(t2, t2, 1))), t2 = t * t (p = 4)
 *     G = amp_gain / sqrtf(q)                           = amp_gain (1 + (|z| / A)^2p)^(-1 / 2p); division and roots correctly rounded
 *     w = (G z.re, G z.im)
 *     phi = amp_ampm * (t / (1 + t)) turns; p32 = (uint32_t)(int32_t)rintf(phi * 2^32); u = w rotated by p32 as above.
 *                                                       amp_ampm == 0: skipped, no sincos, u = w
 * Behind the last stage v = gain u (one multiply per component; skipped when gain == 1, so that a handle with no stage on and gain 1
 * is a pure load-convert-store that keeps NaN payloads and the sign of zero).  out = v (cf32) or Q(v) (sc16: the shared quantiser as it
 * stands, with the shared clip count).  The integers of an sc16-out handle are Q of a cf32-out handle's floats exactly. */
#define MCRX_RFCHAIN_MIXER      1u
#define MCRX_RFCHAIN_OSCILLATOR 2u
#define MCRX_RFCHAIN_AMPLIFIER  4u
#define MCRX_RFCHAIN_MAX_SINUSOIDS 16
typedef struct mcrx_hip_rfchain_s *mcrx_hip_rfchain_t;
typedef struct {
    uint32_t struct_size, order, stages;                /* sizeof(mcrx_hip_rfchain_config); 0 = tx, 1 = rx; MCRX_RFCHAIN_* bits */
    uint32_t input_format, output_format;               /* 0 = cf32, 1 = sc16 */
    float    alpha_re, alpha_im, beta_re, beta_im, dc_re, dc_im;      /* mixer */
    uint32_t pn_sinusoids, pn_log2_block, pn_table_rows;              /* oscillator: 1 .. 16; 1 .. 24; 0 = default, else >= 2 */
    float    pn_rms;                                    /* radians rms, >= 0 */
    double   pn_bandwidth;                              /* half-width of the line, cycles per wideband sample, >= 0 */
    uint64_t pn_seed;
    float    amp_sat, amp_gain, amp_ampm;               /* amplifier: A > 0; small-signal gain; AM/PM at full compression, turns */
    uint32_t amp_smooth;                                /* 1, 2 or 4 */
    float    gain;
} mcrx_hip_rfchain_config;
/* MCRX_EINVAL, before a device is looked for: null pointers, a wrong struct_size, order above 1, unknown stage bits, a format that is not
 * 0 or 1, a gain that is not finite; with the mixer on a coefficient that is not finite; with the oscillator on pn_sinusoids outside
 * 1 .. 16, pn_log2_block outside 1 .. 24, pn_table_rows == 1, pn_rms or pn_bandwidth negative or not finite, pn_bandwidth * B > 1/8
 * (the grid must sample the angle), pn_rms * sqrt(2 S) >= pi / 2 (keeps |theta| < 1/4 turn); with the amplifier on amp_smooth other than
 * 1, 2, 4, an amp_sat that is not finite and positive or whose 1 / A^2 is not a finite positive fp32, an amp_gain that is not finite,
 * |amp_ampm| > 1/4 or not finite.  Fields of a stage that is off are not looked at. */
int      mcrx_hip_rfchain_create(mcrx_hip_rfchain_t *out, const mcrx_hip_rfchain_config *cfg);
int      mcrx_hip_rfchain_destroy(mcrx_hip_rfchain_t q);
/* n samples at d_in (the handle's input format) -> n samples at d_out (its output format), the first of them absolute sample
 * first_sample, asynchronously on `stream` (NULL = the default stream); at most 2^32 samples a call.  MCRX_EINVAL, nothing written: a
 * null handle or buffer, a cf32 buffer not 8-byte aligned, an sc16 buffer not 4-byte aligned, ranges that overlap -- EXCEPT d_in ==
 * d_out with equal formats: a lane writes only what it read, so in-place use is allowed.  (Pairs of samples go as 16-byte (sc16:
 * 8-byte) words where the addresses allow.) */
int      mcrx_hip_rfchain_execute_device(mcrx_hip_rfchain_t q, const void *d_in, uint64_t first_sample, size_t n, void *d_out, void *stream);
/* mctx_hip_clipped's semantics; counter and event exist only on a handle with sc16 output; always 0 on a cf32 one */
int      mcrx_hip_rfchain_clipped(mcrx_hip_rfchain_t q, uint64_t *samples, int reset);
unsigned mcrx_hip_rfchain_input_format(mcrx_hip_rfchain_t q);                        /* 0 for a null handle */
unsigned mcrx_hip_rfchain_output_format(mcrx_hip_rfchain_t q);                       /* 0 for a null handle */
/* host, no GPU: the oscillator's integers N_k (steps) and Phi_k (phases), pn_sinusoids entries each, and c (*coef).  Checks cfg as
 * create does, the oscillator's fields whether or not its bit is set. */
int      mcrx_hip_rfchain_selftest(const mcrx_hip_rfchain_config *cfg, int64_t *steps, uint32_t *phases, float *coef);
/* The table kernel on its own, for tests and measurements: Theta[first_row + r], r < rows, as floats into the caller's 4-byte aligned
 * device buffer, asynchronously on `stream`.  MCRX_EINVAL with the oscillator off. */
int      mcrx_hip_rfchain_phase_rows(mcrx_hip_rfchain_t q, uint64_t first_row, uint32_t rows, void *d_table, void *stream);
const char *mcrx_hip_rfchain_last_error(void);

/* ---- Receiver calibration on the wideband stream: blind DC offset and IQ correction ----
 * What a radio front end does before its samples reach the host: it removes the LO leakage d and the conjugate image that a receive
 * mixer u = alpha z + beta conj(z) + d leaves (the image of channel c lies in channel N - 1 - c), without knowing alpha, beta or d.
 * A STATEFUL operator, cf32 or sc16 in, cf32 or sc16 out (or nothing out).  For every sample u[n] one pass over the data can
 *   apply:    correct u[n] with the coefficients (m, w) the handle holds, and
 *   measure:  add u[n] to the moments the next coefficients are made of.
 * Coefficients and moments live in device memory and are updated by a kernel: a free-running stream never synchronises with the host.
 * Moments, of the RAW input (feed-forward): cnt, S1 = sum u, S2 = sum u^2 (complex), P = sum |u|^2, kept as sum re, sum im,
 *   sum re^2 - sum im^2, 2 sum re im, sum re^2 + sum im^2.  sc16 input: exact integers of the int16 components, int64 from lane to
 *   handle; a sample adds at most 2^31, so a call that would bring the samples measured since the last update above 2^31 is refused.
 *   cf32 input: every product is formed in fp64 from the fp32 components (exact) and summed in fp64 in a fixed order -- a lane over its
 *   own pairs, ascending; the wave's tree; the workgroup's waves in order; one partial row per workgroup; the fold kernel over the rows
 *   (thread t of 256 the rows t, t + 256, ... ascending, then a wave's tree and the waves in order).  No floating-point atomics.  The grid, and which samples
 *   a workgroup takes, are a function of the call's (position, n) only.
 * Update, one lane on the device in fp64, at a block boundary or on request, with cnt > 0:
 *   b = (S1, S2, P) / cnt                         (sc16: times 2^-15, 2^-30, exact); a block whose means are not finite counts as
 *                                                 degenerate and is dropped whole
 *   R = b (first update), else R += mu_j (b - R)  mu_j = max(1 / (j + 1), 2^-forget_log2), j = earlier updates: the cumulative mean
 *                                                 that turns exponential
 *   the block accumulators are cleared, j += 1
 *   m = R.s1, c2 = R.s2 - m^2, pc = R.p - |m|^2, D = pc^2 - |c2|^2
 *   w = c2 / (pc + sqrt(D))                       for u = alpha z + beta conj(z) + d with z proper (E z^2 = 0) this is exactly
 *                                                 beta / conj(alpha) and m = d: (u - m) - w conj(u - m) = alpha (1 - |w|^2) z
 *   pc <= 0, D <= 0 or D not finite: the previous coefficients stay and `degenerate` goes up.
 *   Stored: (float)m with MCRX_RFCAL_DC set, else 0; (float)w with MCRX_RFCAL_IQ set, else 0.  The central moments always use m.
 *   While the handle is held (mcrx_hip_rfcal_hold) nothing is measured and no update runs.
 * Apply, fp32, every product that matters one fmaf:
 *     t  = (u.re - m.re, u.im - m.im)
 *     y.re = fmaf(-w.re, t.re, fmaf(-w.im, t.im, t.re))
 *     y.im = fmaf( w.re, t.im, fmaf(-w.im, t.re, t.im))
 *     v = gain * y            (skipped when gain == 1)
 *     out = v (cf32) or Q(v) (sc16: the shared quantiser with the shared clip count)
 *   The integers of an sc16-out handle are Q of a cf32-out handle's floats exactly.  Until a handle has had its first update or a set,
 *   the launches carry no apply code (known on the host, no readback): such a handle with gain 1 is load, convert, store and keeps NaN
 *   payloads and -0.0.  In-place use (d_in == d_out, equal formats) is allowed: a lane writes only what it read.
 * Blocks: the handle keeps the absolute position of its next sample.  period_log2 = k in 6 .. 30: block j is the samples
 *   [j 2^k, (j + 1) 2^k) of the absolute index; a call is split there on the host and fold + update are enqueued behind each segment
 *   that ends a block, so block j is corrected with what the blocks before it measured and the first block after a reset passes
 *   uncorrected.  period_log2 = 0: nothing updates until mcrx_hip_rfcal_update.
 * Cuts.  sc16 input: output and state are a function of the stream and of the absolute positions of the updates -- any cutting into
 *   calls gives the same bits.  cf32 input: the same calls give the same bits, but DIFFERENTLY CUT CALLS GIVE COEFFICIENTS THAT DIFFER
 *   BY THE fp64 SUMMATION ERROR (each block moment within about 2 n 2^-53 sum |term| of the exact sum, n the block's samples): the one
 *   place this operator is weaker than the emulators' "cut anywhere".  Calls on one handle must be ordered on the device.
 * Limitation: the estimator assumes a proper signal.  Frames that start together in mirror channels c and N - 1 - c carry the same
 *   preamble, whose product does not average out; longer payloads dilute the bias. */
#define MCRX_RFCAL_DC 1u
#define MCRX_RFCAL_IQ 2u
typedef struct mcrx_hip_rfcal_s *mcrx_hip_rfcal_t;
typedef struct {
    uint32_t struct_size, stages;                       /* sizeof(mcrx_hip_rfcal_config); MCRX_RFCAL_* bits */
    uint32_t input_format, output_format;               /* 0 = cf32, 1 = sc16 */
    uint32_t period_log2, forget_log2;                  /* 0 (manual) or 6 .. 30; 0 .. 30 */
    float    gain;
} mcrx_hip_rfcal_config;
typedef struct {
    float    m_re, m_im, w_re, w_im;                    /* the coefficients apply uses */
    double   mean[5];                                   /* R: s1.re, s1.im, s2.re, s2.im, p */
    double   acc[5];                                    /* cf32 input: the block accumulators S1.re, S1.im, S2.re, S2.im, P */
    int64_t  acc_int[5];                                /* sc16 input: the same as exact integers of the int16 components */
    uint64_t count;                                     /* samples in the block accumulators */
    uint64_t updates, measured, degenerate;             /* j; samples measured since the reset; updates that kept the coefficients */
} mcrx_hip_rfcal_state;
/* MCRX_EINVAL before a device is looked for, *out cleared: null pointers, a wrong struct_size, unknown stage bits, a format that is not
 * 0 or 1, period_log2 other than 0 or 6 .. 30, forget_log2 above 30, a gain that is not finite. */
int      mcrx_hip_rfcal_create(mcrx_hip_rfcal_t *out, const mcrx_hip_rfcal_config *cfg);
int      mcrx_hip_rfcal_destroy(mcrx_hip_rfcal_t q);
/* position := pos, and coefficients, means, accumulators and counters cleared -- without synchronising the device: the next kernel of
 * the handle clears them.  The clip count stays. */
int      mcrx_hip_rfcal_reset_at(mcrx_hip_rfcal_t q, uint64_t pos);
uint64_t mcrx_hip_rfcal_position(mcrx_hip_rfcal_t q);                                /* 0 for a null handle */
/* The next n samples of the stream, asynchronously on `stream`; d_out == NULL: measure only.  At most 2^32 samples a call.  MCRX_EINVAL,
 * nothing written, nothing consumed, position and state as before: a null handle or d_in, a cf32 buffer not 8-byte aligned, an sc16
 * buffer not 4-byte aligned, ranges that overlap other than d_in == d_out with equal formats, and on an sc16-in handle that is not
 * held a call that would bring the samples measured since the last update above 2^31. */
int      mcrx_hip_rfcal_execute_device(mcrx_hip_rfcal_t q, const void *d_in, size_t n, void *d_out, void *stream);
int      mcrx_hip_rfcal_update(mcrx_hip_rfcal_t q, void *stream);                    /* MCRX_EINVAL when period_log2 != 0 */
int      mcrx_hip_rfcal_hold(mcrx_hip_rfcal_t q, int on);                            /* held: launches without the measuring code */
int      mcrx_hip_rfcal_set(mcrx_hip_rfcal_t q, float m_re, float m_im, float w_re, float w_im, void *stream);     /* finite values */
/* waits for the handle's work on `stream` */
int      mcrx_hip_rfcal_read(mcrx_hip_rfcal_t q, mcrx_hip_rfcal_state *out, void *stream);
int      mcrx_hip_rfcal_clipped(mcrx_hip_rfcal_t q, uint64_t *samples, int reset);   /* mctx_hip_clipped's semantics */
/* host, no GPU: the segments the call (pos, n) is split into -- seg_len[i], and seg_updates[i] = 1 where segment i ends a block -- the
 * first `cap` of them written, *nseg = how many there are.  Checks cfg as create does and the call as execute does (n above 2^32, the
 * 2^31 guard of an sc16-in handle that has measured nothing since its last update). */
int      mcrx_hip_rfcal_selftest(const mcrx_hip_rfcal_config *cfg, uint64_t pos, uint64_t n, uint64_t *seg_len, uint32_t *seg_updates,
                                 size_t cap, uint64_t *nseg);
const char *mcrx_hip_rfcal_last_error(void);

/* ---- Crest-factor reduction on the wideband stream: clip-and-filter ahead of DAC and amplifier ----
 * The transmitter's channels add coherently in their preambles and pilots: its peaks reach several times the rms.  This stage takes
 * what exceeds an amplitude A out of the stream, band-limited by a real symmetric low-pass so that the correction stays inside the
 * band the channels occupy (|f| <= 1/4 cycle per sample) and does not splatter into the outer half.  It buys headroom and containment
 * with in-band error: the EVM of every channel gets worse.  cf32 in, cf32 or sc16 out.
 * Configuration: threshold A; half_len H in 1 .. 64 and the taps h[0 .. H] of the filter h[-k] = h[k]; passes P in 1 .. 4; gain;
 * output_format.  A2 = fp32(A * A), the product made on the host in double.  ONE PASS maps a sequence x to y, all in fp32:
 *     t    = fmaf(x.re, x.re, x.im * x.im)
 *     e[n] = (0, 0)                     unless t > A2 (so a NaN gives 0)
 *            (s x.re, s x.im),          s = 1 - A / sqrtf(t), division and root correctly rounded
 *     c[n] = acc_H per component:       acc_0 = h[0] * e[n];  acc_k = fmaf(h[k], e[n-k] + e[n+k], acc_{k-1}),  k = 1 .. H
 *     y[n] = x[n] - c[n]
 * P passes run one behind the other.  Behind the last v = gain * y (one multiply per component; skipped when gain == 1), and
 * out = v (cf32) or Q(v) (sc16: the shared quantiser as it stands, with the shared clip count).
 * Nothing depends on the absolute index: the operator is STATELESS and NON-CAUSAL.  halo = P * H; a call reads n + 2 * halo input
 * samples and writes n output samples, d_out[i] belongs to d_in[i + halo]: the caller supplies lead and tail, the way
 * mctx_hip_synthesize_tiles takes its lead.  At the two ends of a stream lead and tail are zeros.  Consequences:
 *   - a stream cut anywhere, each piece with its halos, gives the bits of one call;
 *   - the integers of an sc16-out handle are Q of a cf32-out handle's floats exactly;
 *   - where no sample within reach exceeds A, c = +0 and y = x bit for bit for every word that is not a NaN, -0.0 included (a NaN
 *     stays a NaN): h[0] * (+0) is a zero, fmaf(h[k], +0, zero) keeps it a zero, and that zero is +0 as soon as one tap is not
 *     negative -- DESIGN.md section 4.20 works the signs out.  A launch therefore skips the filter for the waves whose window
 *     holds no sample above A, which changes no bit.  (With EVERY tap h[0 .. H] negative c = -0, x = -0.0 comes out as +0.0 as
 *     the definition says, and the launches of such a handle skip nothing.)
 *   - in-place use is refused: neighbours are read.
 * With P > 1 the passes run as one launch each through scratch buffers the handle owns (grown on demand); pass p covers the samples
 * [-(P - 1 - p) H, n + (P - 1 - p) H) around the output.  Because of those buffers, calls on ONE handle with P > 1 must be ordered
 * on the device (one stream, or events of the caller's), as with a userclock; handles with P = 1 are free of this.
 * Statistics, integer atomics only, none issued while nothing happens:
 *   over[p]  samples with t > A2 at the input of pass p, counted over the samples of the caller's n outputs only, never the halos;
 *   peak2    the largest |y|^2 = fmaf(y.re, y.re, y.im * y.im) of the last pass's n outputs, before the gain (a NaN does not count).
 * Both are independent of order, hence of cuts and of the launch geometry. */
#define MCRX_CFR_MAX_HALF_LEN 64
#define MCRX_CFR_MAX_PASSES   4
typedef struct mcrx_hip_cfr_s *mcrx_hip_cfr_t;
typedef struct {
    uint32_t struct_size, half_len, passes, output_format;      /* sizeof(mcrx_hip_cfr_config); H; P; 0 = cf32, 1 = sc16 */
    float    threshold, gain;                                   /* A, against the full scale 1.0; v = gain y */
    float    taps[MCRX_CFR_MAX_HALF_LEN + 1];                   /* h[0 .. H]; the entries behind h[H] are not looked at */
} mcrx_hip_cfr_config;
/* MCRX_EINVAL before a device is looked for, *out cleared: null pointers, a wrong struct_size, half_len outside 1 .. 64, passes
 * outside 1 .. 4, an output format that is not 0 or 1, a threshold that is not finite and positive or whose A2 is not a finite
 * positive fp32, a gain or one of the taps h[0 .. H] that is not finite. */
int      mcrx_hip_cfr_create(mcrx_hip_cfr_t *out, const mcrx_hip_cfr_config *cfg);
int      mcrx_hip_cfr_destroy(mcrx_hip_cfr_t q);
unsigned mcrx_hip_cfr_halo(mcrx_hip_cfr_t q);                                        /* P * H; 0 for a null handle */
unsigned mcrx_hip_cfr_output_format(mcrx_hip_cfr_t q);                               /* 0 for a null handle */
/* n + 2 * halo cf32 samples at d_in -> n samples at d_out (the handle's output format), asynchronously on `stream` (NULL = the
 * default stream).  n == 0: MCRX_OK, nothing done.  MCRX_EINVAL, nothing written: a null handle or buffer, a cf32 buffer not 8-byte
 * aligned, an sc16 output not 4-byte aligned, ranges that overlap in any way (d_in == d_out included), n + 2 * halo > 2^32. */
int      mcrx_hip_cfr_execute_device(mcrx_hip_cfr_t q, const void *d_in, size_t n, void *d_out, void *stream);
/* mctx_hip_clipped's semantics; counter and event exist only on a handle with sc16 output; always 0 on a cf32 one */
int      mcrx_hip_cfr_clipped(mcrx_hip_cfr_t q, uint64_t *samples, int reset);
/* over[p], p < 4 (0 behind the handle's last pass) and peak2 since the last reset; waits for the handle's last call only.  Either
 * pointer may be null. */
int      mcrx_hip_cfr_stats(mcrx_hip_cfr_t q, uint64_t over[MCRX_CFR_MAX_PASSES], float *peak2, int reset);
/* host, no GPU: the taps of a windowed-sinc low-pass, h[k] = 2 fc sinc(2 fc k) w(k), k = 0 .. half_len, fc = cutoff in cycles per
 * sample, w(k) = I0(beta sqrt(1 - (2 k / (2 half_len + 1))^2)) / I0(beta) (the transmitter's Kaiser window), scaled so that
 * h[0] + 2 sum_{k >= 1} h[k] = 1; all in double, then rounded to fp32.  MCRX_EINVAL: a null h, half_len outside 1 .. 64, cutoff
 * outside (0, 0.5), beta < 0, values that are not finite. */
int      mcrx_hip_cfr_design(uint32_t half_len, double cutoff, double beta, float *h);
const char *mcrx_hip_cfr_last_error(void);

/* ---- Digital predistortion on the wideband stream: learn the amplifier, invert its table ----
 * The stage between crest-factor reduction and the amplifier: a complex gain F(|x|), looked up by amplitude and interpolated, that
 * undoes the amplifier's compression (AM/AM) and phase shift (AM/PM) BELOW saturation -- it cannot undo saturation, so the peaks must
 * already lie below it: mcrx_hip_cfr_* comes first.  The table is learned on the device from what went into the amplifier (u) and
 * what came out of it (z).  cf32 in, cf32 or sc16 out; the feedback is cf32.
 * Configuration: table_log2 in 5 .. 10, K = 2^table_log2 intervals and K + 1 entries F[0 .. K]; full_scale, the amplitude of entry
 * K; target_gain g0, the linear gain the amplifier shall appear to have (as a rule its amp_gain); min_count >= 1; forget_shift in
 * 0 .. 8; gain; output_format.  The host makes, in double, inv_step = fp32(K / full_scale) and step = full_scale / K (kept double);
 * e is the least integer with 2^e >= full_scale, E = 2^e.  F = 1 + 0i in every entry until an update or a set_table.
 * APPLY, fp32, memoryless and stateless in position:
 *     t = fmaf(x.re, x.re, x.im * x.im);  a = sqrtf(t)                        correctly rounded
 *     s = fminf(a * inv_step, (float)K);  k = min((int)s, K - 1);  f = s - (float)k      (exact; a NaN amplitude gives s = K)
 *     G.re = fmaf(f, F[k+1].re - F[k].re, F[k].re)                            likewise G.im; the difference is one fp32 subtraction
 *     y.re = fmaf(G.re, x.re, -(G.im * x.im));  y.im = fmaf(G.re, x.im, G.im * x.re)
 *     v = gain * y            (skipped when gain == 1)
 *     out = v (cf32) or Q(v) (sc16: the shared quantiser with the shared clip count)
 *   Above full_scale the last entry holds.  The integers of an sc16 handle are Q of a cf32 handle's floats exactly.  Until a handle
 *   has had an update or a set_table its launches carry no apply code (known on the host, no readback): such a handle is load,
 *   [gain,] convert, store and keeps NaN payloads and -0.0.  In-place use (d_in == d_out, equal formats) is allowed: a lane writes
 *   only what it read.  A stream may be cut into calls anywhere.
 * MEASURE: two aligned cf32 streams of n samples; u is what went into the amplifier (this handle's cf32 output), z what came out of
 *   it, aligned and scaled by the caller.  Per sample, in fp32,
 *     tu = fmaf(u.re, u.re, u.im * u.im);  tz likewise of z;  j = (int)rintf(sqrtf(tu) * inv_step)         (ties to even)
 *   The sample is ELIGIBLE when tu and tz are finite, rintf(...) <= K and tz <= fp32(16 E^2) (that bound is +inf where 16 E^2 is no
 *   fp32).  An eligible sample adds to four int64 accumulators of bin j:
 *     cnt += 1
 *     Sre += llrint(fma(z.re, u.re, z.im * u.im) * 2^(32 - 2e))
 *     Sim += llrint(fma(z.im, u.re, -(z.re * u.im)) * 2^(32 - 2e))
 *     Suu += llrint(fma(u.re, u.re, u.im * u.im) * 2^(32 - 2e))
 *   the products formed in fp64 from the fp32 components (exact), the sum of two rounded once, the scaling exact, llrint to nearest
 *   even.  Every other sample adds 1 to `skipped`.  The sums are integers: order, cuts, grid and launch geometry cannot change a
 *   bit.  Integer atomics only, no floating-point atomic anywhere.  A term is below 2^34.1 in magnitude; the host keeps a count of
 *   the samples offered since the last reset (eligible or not), which follows an update as ceil(count / 2^forget_shift), and refuses
 *   a call that would take it above 2^28 -- such a call measures nothing.
 * UPDATE: one lane on the device in fp64, + - * / sqrt only, nothing contracted; no host synchronisation.  With r_j = j * step:
 *   bin j is VALID when cnt >= min_count and Suu > 0; then A_j = ((double)Sre / (double)Suu, (double)Sim / (double)Suu).
 *   An invalid bin takes the A of the nearest valid bin below it; the bins below the first valid one take the first valid one's.
 *   No valid bin: the table stays and `degenerate` goes up.  Otherwise
 *     |A| = sqrt(A.re * A.re + A.im * A.im);  o_0 = |A_0| r_0;  o_j = max(o_{j-1}, |A_j| r_j)       the AM/AM curve made monotone
 *   and the entries i = 1 .. K in this order, with one pointer j that starts at 1 and only moves up:
 *     d = g0 * r_i;  j = the least index with o_j >= d
 *     fr = (d - o_{j-1}) / (o_j - o_{j-1}), or 0 where that denominator is not positive
 *     r_in = r_{j-1} + fr * step;  A_in = A_{j-1} + fr * (A_j - A_{j-1})     per component
 *     where even o_K < d:  r_in = r_K, A_in = A_K
 *     q = r_in / r_i;  F_i = ((q * A_in.re) / |A_in|, -((q * A_in.im) / |A_in|));  F_i = (q, 0) where |A_in| is not positive
 *   F_0 = F_1; F is stored rounded to fp32.  Last -- after a degenerate update too -- every accumulator is shifted right
 *   arithmetically by forget_shift, and `updates` goes up.  What the amplifier does at amplitude r does not depend on the table, so
 *   the sums stay valid across updates: a further update adds the bins that the expanded drive reaches for the first time.
 * Calls on ONE handle must be ordered on the device (one stream, or events of the caller's): they share its table and accumulators. */
typedef struct mcrx_hip_dpd_s *mcrx_hip_dpd_t;
typedef struct {
    uint32_t struct_size, table_log2;                   /* sizeof(mcrx_hip_dpd_config); 5 .. 10 */
    float    full_scale, target_gain;                   /* the amplitude of entry K; g0 */
    uint32_t min_count, forget_shift;                   /* >= 1; 0 .. 8 */
    float    gain;
    uint32_t output_format;                             /* 0 = cf32, 1 = sc16 */
} mcrx_hip_dpd_config;
typedef struct {
    uint64_t updates, skipped, degenerate;              /* updates run; ineligible samples; updates that left the table as it was */
} mcrx_hip_dpd_state;
/* MCRX_EINVAL before a device is looked for, *out cleared: null pointers, a wrong struct_size, table_log2 outside 5 .. 10, a
 * full_scale or target_gain that is not finite and positive, a full_scale whose inv_step is not a finite positive fp32, min_count 0,
 * forget_shift above 8, a gain that is not finite, an output format that is not 0 or 1. */
int      mcrx_hip_dpd_create(mcrx_hip_dpd_t *out, const mcrx_hip_dpd_config *cfg);
int      mcrx_hip_dpd_destroy(mcrx_hip_dpd_t q);
/* n cf32 samples at d_in -> n samples at d_out (the handle's output format), asynchronously on `stream`.  n == 0: MCRX_OK, nothing
 * done.  MCRX_EINVAL, nothing written: a null handle or buffer, a cf32 buffer not 8-byte aligned, an sc16 output not 4-byte aligned,
 * more than 2^32 samples, ranges that overlap other than d_in == d_out with equal formats. */
int      mcrx_hip_dpd_execute_device(mcrx_hip_dpd_t q, const void *d_in, size_t n, void *d_out, void *stream);
/* n aligned cf32 pairs (d_u[i], d_z[i]) into the accumulators.  MCRX_EINVAL, nothing measured, the count as before: a null handle or
 * buffer, a buffer not 8-byte aligned, a call that would take the samples offered since the last reset above 2^28. */
int      mcrx_hip_dpd_measure_device(mcrx_hip_dpd_t q, const void *d_u, const void *d_z, size_t n, void *stream);
int      mcrx_hip_dpd_update(mcrx_hip_dpd_t q, void *stream);
/* F: the K + 1 entries as 2 (K + 1) floats (re, im) in host memory, all finite (MCRX_EINVAL otherwise); read before the call returns */
int      mcrx_hip_dpd_set_table(mcrx_hip_dpd_t q, const float *F, void *stream);
/* waits for the handle's work on `stream`.  F: 2 (K + 1) floats; acc: 4 (K + 1) int64, bin j at acc[4 j ..]: cnt, Sre, Sim, Suu.  Any
 * of the three pointers may be null. */
int      mcrx_hip_dpd_read(mcrx_hip_dpd_t q, mcrx_hip_dpd_state *state, float *F, int64_t *acc, void *stream);
/* table := 1, accumulators, counters and the host's count cleared -- without synchronising the device: the next kernel of the handle
 * that touches them clears them.  Launches carry no apply code again.  The clip count stays. */
int      mcrx_hip_dpd_reset(mcrx_hip_dpd_t q);
int      mcrx_hip_dpd_clipped(mcrx_hip_dpd_t q, uint64_t *samples, int reset);      /* mctx_hip_clipped's semantics */
unsigned mcrx_hip_dpd_output_format(mcrx_hip_dpd_t q);                               /* 0 for a null handle */
/* host, no GPU: checks cfg as create does; *inv_step, *step and *e of it (each may be null); and for the n pairs (u[2 i], u[2 i + 1]),
 * (z[2 i], z[2 i + 1]) bin[i] = j, or -1 where the pair is not eligible (n == 0: u, z and bin are not looked at). */
int      mcrx_hip_dpd_selftest(const mcrx_hip_dpd_config *cfg, float *inv_step, double *step, int *e, const float *u, const float *z,
                               size_t n, int32_t *bin);
const char *mcrx_hip_dpd_last_error(void);

/* ---- Predistortion with memory: branch tables learned by least squares ----
 * The stage between crest-factor reduction and an amplifier that is NOT memoryless: a diagonal memory polynomial.  M branches, branch m
 * a complex gain G_m(|x|) looked up by the amplitude of the sample delay[m] samples back and multiplied with that sample; the output is
 * the sum of the branches.  G_m is a polynomial of P coefficients in the amplitude, tabulated; the L = M P coefficients are the least
 * squares solution that maps what came out of the amplifier (z / g0) back onto what went in (u) -- indirect learning: the
 * post-inverse, used in front.  cf32 in, cf32 or sc16 out; the feedback is cf32.  With M = 1 apply is mcrx_hip_dpd_*'s, bit for bit.
 * Configuration: branches M in 1 .. 4; delay[0] = 0 < delay[1] < ... <= 16, lead = delay[M - 1] (delay[m >= M] is not looked at);
 * order P in 1 .. 5 (branch m has the powers k = 0 .. P - 1; coefficient l = m P + k); table_log2 in 5 .. 10 with
 * M 2^table_log2 <= 2048; full_scale, target_gain g0, gain, output_format, forget_shift as mcrx_hip_dpd_config's; min_rows >= L;
 * ridge_log2 in 10 .. 40.  K, inv_step, step, e and E = 2^e are made exactly as for mcrx_hip_dpd_*; inv_g0 = fp32(1 / g0), the
 * quotient made in double.  M tables F_m[0 .. K] of complex fp32; F_0 = 1 + 0i and F_m = 0 (m >= 1) until an update or a set_tables.
 * APPLY, fp32: the input is n + lead samples, the history in front; in[lead + i] is the sample of output i.  For m = 0 .. M - 1:
 *     x = in[lead + i - delay[m]]
 *     t = fmaf(x.re, x.re, x.im * x.im);  a = sqrtf(t)
 *     s = fminf(a * inv_step, (float)K);  k = min((int)s, K - 1);  f = s - (float)k
 *     G.re = fmaf(f, F_m[k+1].re - F_m[k].re, F_m[k].re)                      likewise G.im; the difference is one fp32 subtraction
 *     p_m.re = fmaf(G.re, x.re, -(G.im * x.im));  p_m.im = fmaf(G.re, x.im, G.im * x.re)
 *   y = p_0;  then for m = 1 .. M - 1 in this order:  y.re = y.re + p_m.re;  y.im = y.im + p_m.im        (fp32 additions)
 *   v = gain * y  (skipped when gain == 1);  out = v (cf32) or Q(v) (sc16: the shared quantiser with the shared clip count).
 *   Until a handle has had an update or a set_tables its launches carry no apply code: load in[lead + i], [gain,] convert, store; NaN
 *   payloads and -0.0 are kept.  Input and output must not overlap at all (a lane reads its neighbours' samples).  A stream cut into
 *   calls that each carry their lead gives the bits of one call.
 * MEASURE: two aligned cf32 streams of n samples, u what went into the amplifier, z what came out of it.  The first lead samples of
 *   a call are history only; the ROWS are i = lead .. n - 1 (n <= lead: MCRX_OK, nothing measured).  Per sample z[j], in fp32:
 *     w = z[j] * inv_g0                          per component
 *     zeta = ldexpf(w, -e)                       w / E
 *     t = fmaf(zeta.re, zeta.re, zeta.im * zeta.im);  a = sqrtf(t)
 *     phi_0 = zeta;  phi_k = phi_{k-1} * a       per component, k = 1 .. P - 1
 *     Z_k = (llrint(phi_k.re * 2^17), llrint(phi_k.im * 2^17))          ties to even; z[j] is GOOD when t <= 1 (false for a NaN)
 *   and per sample u[i]:  ups = ldexpf(u[i], -e) per component;  tu = fmaf(ups.re, ups.re, ups.im * ups.im);
 *     U = (llrint(ups.re * 2^17), llrint(ups.im * 2^17));  u[i] is GOOD when tu <= 4.
 *   Row i is ELIGIBLE when u[i] and every z[i - delay[m]] are good; any other row adds 1 to `skipped`.  Its regressors are
 *   B_l = Z_k of z[i - delay[m]], l = m P + k; with V = (B_0 .. B_{L-1}, U) an eligible row adds, to int64 sums,
 *     rows += 1;   S_pq += conj(V_p) * V_q  for 0 <= p <= q <= L:
 *         S_pq.re += V_p.re * V_q.re + V_p.im * V_q.im;   S_pq.im += V_p.re * V_q.im - V_p.im * V_q.re
 *   so A_pq = S_pq (q < L), b_p = S_pL, Suu = S_LL.re; the diagonal's imaginary part stays 0.  The sums are integers: order, cuts that
 *   keep the same rows, grid and stream position cannot change a bit.  Integer atomics only.  A term is below 2^36.01; the host counts
 *   the rows offered since the last reset (eligible or not), follows an update with ceil(count / 2^forget_shift), and refuses a call
 *   that would take the count above 2^26 -- such a call measures nothing.
 * UPDATE: on the device in fp64, + - * / sqrt only, nothing contracted, no host synchronisation.  In this order:
 *     rows < min_rows: DEGENERATE.
 *     A_pq, b_p, Suu = (double) of the sums (the conversion rounds);  tr = 0;  tr = tr + A_ll.re, l ascending
 *     lambda = (tr / (double)L) * 2^-ridge_log2;  A_ll.re = A_ll.re + lambda
 *     Cholesky A = R^H R, R upper triangular, column j = 0 .. L - 1, in it i = 0 .. j:
 *         s = A_ij;  for p = 0 .. i - 1:  s.re = s.re - (R_pi.re * R_pj.re + R_pi.im * R_pj.im)
 *                                         s.im = s.im - (R_pi.re * R_pj.im - R_pi.im * R_pj.re)
 *         i < j:  R_ij = (s.re / R_ii.re, s.im / R_ii.re)
 *         i = j:  the pivot s.re must be > 0, else DEGENERATE;  R_jj = (sqrt(s.re), 0)
 *     forward, i = 0 .. L - 1:   s = b_i;  for p = 0 .. i - 1:  s.re = s.re - (R_pi.re * y_p.re + R_pi.im * y_p.im)
 *                                                              s.im = s.im - (R_pi.re * y_p.im - R_pi.im * y_p.re);   y_i = s / R_ii.re
 *     backward, i = L - 1 .. 0:  s = y_i;  for p = i + 1 .. L - 1:  s.re = s.re - (R_ip.re * c_p.re - R_ip.im * c_p.im)
 *                                                                  s.im = s.im - (R_ip.re * c_p.im + R_ip.im * c_p.re);   c_i = s / R_ii.re
 *     q = 0;  q = q + (c_l.re * b_l.re + c_l.im * b_l.im), l ascending;  res = Suu - q
 *     a c_l component or res not finite: DEGENERATE.
 *     tables, for m and j = 0 .. K:  rho = ((double)j * step) * 2^-e;  G = c_{m,P-1};  for k = P - 2 .. 0:
 *         G.re = G.re * rho + c_{m,k}.re;  G.im = G.im * rho + c_{m,k}.im       (a multiplication, then an addition)
 *         F_m[j] = (fp32(G.re), fp32(G.im));  an entry not finite: DEGENERATE.
 *   A degenerate update keeps tables, c and res and adds 1 to `degenerate`.  Last, always: every sum and `rows` are shifted right
 *   arithmetically by forget_shift and `updates` goes up.
 * Calls on ONE handle must be ordered on the device (one stream, or events of the caller's). */
typedef struct mcrx_hip_mpd_s *mcrx_hip_mpd_t;
typedef struct {
    uint32_t struct_size, branches;                     /* sizeof(mcrx_hip_mpd_config); M: 1 .. 4 */
    uint32_t delay[4];                                  /* delay[0] = 0, strictly increasing, <= 16 */
    uint32_t order, table_log2;                         /* P: 1 .. 5; 5 .. 10, M 2^table_log2 <= 2048 */
    float    full_scale, target_gain;                   /* the amplitude of entry K; g0 */
    uint32_t min_rows, ridge_log2, forget_shift;        /* >= M P; 10 .. 40; 0 .. 8 */
    float    gain;
    uint32_t output_format;                             /* 0 = cf32, 1 = sc16 */
} mcrx_hip_mpd_config;
typedef struct {
    uint64_t updates, skipped, degenerate;              /* updates run; ineligible rows; updates that left the tables as they were */
    int64_t  rows;                                      /* eligible rows in the sums (shifted with them) */
    double   res;                                       /* Suu - Re(c^H b) of the last update that was not degenerate */
} mcrx_hip_mpd_state;
/* MCRX_EINVAL before a device is looked for, *out cleared: null pointers, a wrong struct_size, and every value outside the ranges
 * above (full_scale, target_gain, gain as mcrx_hip_dpd_create judges them; 1 / target_gain must be a finite positive fp32). */
int      mcrx_hip_mpd_create(mcrx_hip_mpd_t *out, const mcrx_hip_mpd_config *cfg);
int      mcrx_hip_mpd_destroy(mcrx_hip_mpd_t q);
unsigned mcrx_hip_mpd_lead(mcrx_hip_mpd_t q);                                        /* 0 for a null handle */
unsigned mcrx_hip_mpd_output_format(mcrx_hip_mpd_t q);                               /* 0 for a null handle */
/* n + lead cf32 samples at d_in -> n samples at d_out (the handle's output format), asynchronously on `stream`.  n == 0: MCRX_OK,
 * nothing done.  MCRX_EINVAL, nothing written: a null handle or buffer, a cf32 buffer not 8-byte aligned, an sc16 output not 4-byte
 * aligned, n + lead above 2^32, ranges that overlap in any way. */
int      mcrx_hip_mpd_execute_device(mcrx_hip_mpd_t q, const void *d_in, size_t n, void *d_out, void *stream);
/* n aligned cf32 pairs (d_u[i], d_z[i]); rows lead .. n - 1 into the sums.  MCRX_EINVAL, nothing measured, the count as before: a
 * null handle or buffer, a buffer not 8-byte aligned, more than 2^32 samples, a call that would take the rows offered since the last
 * reset above 2^26. */
int      mcrx_hip_mpd_measure_device(mcrx_hip_mpd_t q, const void *d_u, const void *d_z, size_t n, void *stream);
int      mcrx_hip_mpd_update(mcrx_hip_mpd_t q, void *stream);
/* F: the M tables one after the other, M (K + 1) entries as (re, im) floats in host memory, all finite (MCRX_EINVAL otherwise); read
 * before the call returns */
int      mcrx_hip_mpd_set_tables(mcrx_hip_mpd_t q, const float *F, void *stream);
/* waits for the handle's work on `stream`.  F: 2 M (K + 1) floats; c: 2 L doubles (re, im; (1, 0), (0, 0) ... before the first
 * update); sums: 2 (L + 1)(L + 2) / 2 int64, S_pq as (re, im) at entry p (L + 1) - p (p - 1) / 2 + (q - p), that is row by row of
 * the upper triangle.  Any of the four pointers may be null. */
int      mcrx_hip_mpd_read(mcrx_hip_mpd_t q, mcrx_hip_mpd_state *state, float *F, double *c, int64_t *sums, void *stream);
/* tables, c, res, sums, counters and the host's count as after create -- without synchronising the device: the next kernel of the
 * handle that touches them clears them.  Launches carry no apply code again.  The clip count stays. */
int      mcrx_hip_mpd_reset(mcrx_hip_mpd_t q);
int      mcrx_hip_mpd_clipped(mcrx_hip_mpd_t q, uint64_t *samples, int reset);      /* mctx_hip_clipped's semantics */
/* host, no GPU: checks cfg as create does; *inv_step, *step, *e and *inv_g0 of it (each may be null); and for the n sample pairs
 * (u[2 i], u[2 i + 1]), (z[2 i], z[2 i + 1]): Z[(i P + k) 2 ..] = Z_k of z[i] (zeros where z[i] is not good), U[2 i ..] = U of u[i]
 * (likewise), good[i] = 1 (z[i] good) + 2 (u[i] good).  n == 0: u, z, Z, U and good are not looked at. */
int      mcrx_hip_mpd_selftest(const mcrx_hip_mpd_config *cfg, float *inv_step, double *step, int *e, float *inv_g0, const float *u,
                               const float *z, size_t n, int32_t *Z, int32_t *U, int32_t *good);
const char *mcrx_hip_mpd_last_error(void);

/* ---- Amplifier with memory on the wideband stream: parallel Hammerstein branches ----
 * The amplifier that mcrx_hip_mpd_* exists to straighten: one that is NOT memoryless.  B = 1 .. 4 branches, branch b the RF front
 * end's memoryless amplifier A_b with its own saturation amplitude, smoothness, small-signal gain and AM/PM, behind it a sparse complex
 * FIR of T_b = 1 .. 8 taps (d, h): delays d in 0 .. 16, strictly increasing within a branch, weights h complex fp32 (zero allowed).
 *     y[i] = gain * sum_{b < B} sum_{k < T_b} h_{b,k} * A_b(u[i - d_{b,k}])                       lead = the largest delay, 0 .. 16
 * STATELESS and time-invariant, cf32 or sc16 in (a word means (re, im) * 2^-15), cf32 or sc16 out: the input is n + lead samples, the
 * history in front; in[lead + i] is the sample of output i.  A stream cut anywhere into calls that each carry their lead samples of
 * history gives the bits of one call; the operator does not depend on position, so no call takes one.  All fp32:
 *   a_b[s] = A_b(u[s]), once a sample and branch, the amplifier of mcrx_hip_rfchain_* line for line with A = sat, p = smooth:
 *     t = fmaf(z.re, z.re, z.im * z.im) * r_b           r_b = fp32(1 / A_b^2), made on the host (the division in double)
 *     q = 1 + t (p = 1);  sqrtf(fmaf(t, t, 1)) (p = 2);  sqrtf(sqrtf(fmaf(t2, t2, 1))), t2 = t * t (p = 4)
 *     G = amp_gain / sqrtf(q);  w = (G z.re, G z.im)
 *     phi = ampm * (t / (1 + t)) turns; p32 = (uint32_t)(int32_t)rintf(phi * 2^32); (sn, cs) = sincos of the 32-bit phase p32
 *     a.re = fmaf(w.re, cs, -(w.im * sn)),  a.im = fmaf(w.re, sn, w.im * cs)                      ampm == 0: skipped, a = w
 *   the sum, in the fixed order b ascending, then k ascending, a = a_b[lead + i - d_{b,k}], h = h_{b,k}:
 *     the first term (b = 0, k = 0), a plain complex product, not an accumulation onto zero:
 *       y.re = fmaf(h.re, a.re, -(h.im * a.im));   y.im = fmaf(h.re, a.im, h.im * a.re)
 *     every later term, two nested fmaf a component onto the accumulator:
 *       y.re = fmaf(h.re, a.re, fmaf(-h.im, a.im, y.re));   y.im = fmaf(h.re, a.im, fmaf(h.im, a.re, y.im))
 *   v = gain * y (one multiply a component; skipped when gain == 1);  out = v (cf32) or Q(v) (sc16: the shared quantiser as it stands,
 *   with the shared clip count).  The integers of an sc16-out handle are Q of a cf32-out handle's floats exactly; an sc16-in handle
 *   gives the bits of a cf32-in handle on (re, im) * 2^-15.  With B = 1 and the one tap (0, 1 + 0i) the output equals that of the
 *   mcrx_hip_rfchain_* handle with the amplifier alone as numbers for every finite input (the sign of a zero may differ).
 * Input and output must not overlap at all: a lane reads its neighbours' samples. */
#define MCRX_PAMEM_MAX_BRANCHES 4
#define MCRX_PAMEM_MAX_TAPS     8
#define MCRX_PAMEM_MAX_DELAY    16
typedef struct mcrx_hip_pamem_s *mcrx_hip_pamem_t;
typedef struct {
    float    sat, amp_gain, ampm;                       /* A > 0; small-signal gain; AM/PM at full compression, turns */
    uint32_t smooth, taps;                              /* 1, 2 or 4; T: 1 .. 8 */
    uint32_t delay[MCRX_PAMEM_MAX_TAPS];                /* 0 .. 16, strictly increasing; entries >= taps are not looked at */
    float    h_re[MCRX_PAMEM_MAX_TAPS], h_im[MCRX_PAMEM_MAX_TAPS];
} mcrx_hip_pamem_branch;
typedef struct {
    uint32_t struct_size, branches;                     /* sizeof(mcrx_hip_pamem_config); B: 1 .. 4 */
    uint32_t input_format, output_format;               /* 0 = cf32, 1 = sc16 */
    float    gain;
    mcrx_hip_pamem_branch branch[MCRX_PAMEM_MAX_BRANCHES];
} mcrx_hip_pamem_config;
/* MCRX_EINVAL before a device is looked for, *out cleared: null pointers, a wrong struct_size, branches outside 1 .. 4, a format that
 * is not 0 or 1, a gain that is not finite; in a branch taps outside 1 .. 8, a delay above 16 or not strictly increasing, a weight that
 * is not finite, and sat, smooth, amp_gain, ampm judged exactly as mcrx_hip_rfchain_create judges amp_sat, amp_smooth, amp_gain and
 * amp_ampm.  Fields of branches at index >= branches are not looked at. */
int      mcrx_hip_pamem_create(mcrx_hip_pamem_t *out, const mcrx_hip_pamem_config *cfg);
int      mcrx_hip_pamem_destroy(mcrx_hip_pamem_t q);
unsigned mcrx_hip_pamem_lead(mcrx_hip_pamem_t q);                                      /* 0 for a null handle */
unsigned mcrx_hip_pamem_input_format(mcrx_hip_pamem_t q);                              /* 0 for a null handle */
unsigned mcrx_hip_pamem_output_format(mcrx_hip_pamem_t q);                             /* 0 for a null handle */
/* n + lead samples at d_in (the handle's input format) -> n samples at d_out (its output format), asynchronously on `stream` (NULL =
 * the default stream).  n == 0: MCRX_OK, nothing done.  MCRX_EINVAL, nothing written: a null handle or buffer, a cf32 buffer not 8-byte
 * aligned, an sc16 buffer not 4-byte aligned, n + lead above 2^32, ranges that overlap in any way. */
int      mcrx_hip_pamem_execute_device(mcrx_hip_pamem_t q, const void *d_in, size_t n, void *d_out, void *stream);
/* mctx_hip_clipped's semantics; counter and event exist only on a handle with sc16 output; always 0 on a cf32 one */
int      mcrx_hip_pamem_clipped(mcrx_hip_pamem_t q, uint64_t *samples, int reset);
/* host, no GPU: checks cfg as create does; *lead; inv_a2[b] = r_b, b < branches; and the taps flattened in the order the sum runs
 * (branch ascending, then tap ascending): *num_taps of them, tap i of branch tap_branch[i] at delay tap_delay[i] with the weight
 * (tap_h[2 i], tap_h[2 i + 1]).  Room for 4 and 32 entries; each of the six pointers may be null. */
int      mcrx_hip_pamem_selftest(const mcrx_hip_pamem_config *cfg, uint32_t *lead, float *inv_a2, uint32_t *num_taps, uint32_t *tap_branch,
                                 uint32_t *tap_delay, float *tap_h);
const char *mcrx_hip_pamem_last_error(void);

/* ---- Feedback alignment for the predistorters: delay, gain and phase ----
 * The stage between an observation receiver and mcrx_hip_dpd_measure_device / mcrx_hip_mpd_measure_device.  The receiver returns the
 * amplifier's output late by some samples and a fraction of one, at its own gain and phase, as cf32 or sc16; this operator undoes the
 * three.  Stateful, with the predistorters' three parts -- apply, measure, update -- and no host synchronisation between them.
 * The handle holds, in device memory: tau_fp, an int64 in Q32 samples (how much the capture lags u); a complex fp64 scale s; the 32
 * fp32 coefficients, the whole-sample offset and the fp32 scale that follow from the two.  After create and after reset tau_fp = 0,
 * s = 1 and launches carry no filter code.
 * Configuration: max_lag Lm in 8 .. 64; full_scale finite and positive, e and E = 2^e made of it exactly as for mcrx_hip_dpd_*;
 * target_gain g0 finite and positive; min_rows >= 1; input_format 0 = cf32, 1 = sc16 (the shared codec: a word means (re, im) 2^-15).
 * Derived: H = 8; R = Lm + H; halo = Lm + 17; the differentiator h_k = fp32((-1)^k / k (0.54 + 0.46 cos(pi k / 9))), k = 1 .. 8, made
 * in double; h_-k = -h_k, h_0 = 0.
 * APPLY, fp32, stateless in the samples: the input is n + 2 halo capture samples, in[halo + i] the sample of output i; the output is
 * n cf32 samples.  With mcrx_hip_userclock_*'s table W (mcrx_hip_userclock_table):
 *     d = -tau_fp;  nd = d >> 32 (floor);  mu = d & 0xffffffff;  r = mu >> 26;  f = ((mu >> 2) & 0xffffff) 2^-24
 *     c_j = fmaf(f, W[r+1][j] - W[r][j], W[r][j])                             j = 0 .. 31, the difference one fp32 subtraction
 *     acc = 0;  acc.re = fmaf(c_j, x.re, acc.re), acc.im = fmaf(c_j, x.im, acc.im) with x = in[halo + i - nd + 15 - j], j ascending
 *     out.re = fmaf(s.re, acc.re, -(s.im * acc.im));  out.im = fmaf(s.re, acc.im, s.im * acc.re)         s rounded to fp32
 *   |tau_fp| <= (Lm + 1) 2^32 always, so every tap lies inside the call's input.  A stream cut anywhere, each piece with its halos,
 *   gives the bits of one call.  Until a handle has had an update or a set its launches carry no filter code: load in[halo + i],
 *   convert, store; NaN payloads and -0.0 are kept.  Input and output must not overlap at all.
 * MEASURE: two cf32 streams of n samples, u what went into the amplifier and zh the aligned capture that apply wrote.  Per component
 *     Q15(v) = clamp(llrint(ldexpf(v, 15 - e)), -32768, 32767)               ties to even; a NaN gives 0
 *   U[i] = Q15 of u[i], Z[i] = Q15 of zh[i].  The ROWS are i = R .. n - R - 1 (n <= 2 R: MCRX_OK, nothing measured); no row is
 *   skipped.  u[i] and zh[i] of a row each add 1 to `clamped` when a component clamps or is not finite.  To int64 sums, exactly:
 *     C[l] += conj(U[i]) Z[i + l]   l = -R .. R        A[l] += conj(U[i]) U[i + l]   l = 0 .. 2 H        Szz += |Z[i]|^2        rows += 1
 *   with conj(X) Y = (X.re Y.re + X.im Y.im, X.re Y.im - X.im Y.re).  Integer atomics only: order, grid and cuts that keep the same
 *   rows cannot change a bit.  A term is at most 2^31; the host counts the rows offered since the last update or reset and refuses a
 *   call that would take the count above 2^31 -- such a call measures nothing.
 * UPDATE: one lane on the device in fp64, + - * / and comparisons and conversions only, nothing contracted.  c(l) = (double) C[l],
 *   a(l) = (double) A[l] per component (the conversion rounds); hd_k = (double) h_k.  In this order:
 *     rows < min_rows: DEGENERATE.
 *     best = -1;  for l = -Lm .. Lm ascending:  p = c(l).re * c(l).re + c(l).im * c(l).im;  p > best:  best = p, D = l.
 *     best is not > 0: DEGENERATE.      bu = c(D)
 *     bd = 0;  for k = 1 .. 8:  t = c(D + k) - c(D - k);  bd.re = bd.re + hd_k * t.re;  bd.im = bd.im + hd_k * t.im
 *     Guu = a(0).re
 *     g = 0;  for k = 1 .. 8:  g = g + hd_k * a(k).im;      Gud = (0, -2 g)        (a(-k) = conj(a(k)): the real parts cancel)
 *     Gdd = 0;  for k = -8 .. 8 without 0, in it m = -8 .. 8 without 0:  Gdd = Gdd + (hs_k * hs_m) * a(|k - m|).re
 *                                                                       hs_k = hd_k for k > 0, -hd_-k for k < 0
 *     det = Guu * Gdd - Gud.im * Gud.im;      det is not > 0: DEGENERATE
 *     alpha = ((Gdd * bu.re + Gud.im * bd.im) / det,  (Gdd * bu.im - Gud.im * bd.re) / det)          (Gdd bu - Gud bd) / det
 *     beta  = ((Guu * bd.re - Gud.im * bu.im) / det,  (Guu * bd.im + Gud.im * bu.re) / det)          (Guu bd - conj(Gud) bu) / det
 *     m2 = alpha.re * alpha.re + alpha.im * alpha.im
 *     delta = -((beta.re * alpha.re + beta.im * alpha.im) / m2)                                      -Re(beta / alpha)
 *     x = (s.re * g0, s.im * g0);  s' = ((x.re * alpha.re + x.im * alpha.im) / m2,  (x.im * alpha.re - x.re * alpha.im) / m2)
 *     res' = Szz - (alpha.re * bu.re + alpha.im * bu.im)
 *     inc = (int64) rint(((double)D + delta) * 2^32), ties to even;  tau' = tau_fp + inc
 *     DEGENERATE if delta, s', res' or fp32(s') is not finite, if delta > 1 or delta < -1, or if |tau'| > (Lm + 1) 2^32.
 *     Otherwise tau_fp = tau', s = s', res = res', and the coefficients, nd and the fp32 scale are made anew.
 *   A degenerate update keeps tau_fp, s, res and the coefficients and adds 1 to `degenerate`.  Last, always: every sum and `rows` are
 *   cleared and `updates` goes up.  This is one Gauss-Newton step on zh ~ alpha u - alpha delta u', u' = sum_k h_k u[i - k].
 * A correlation aligner attributes the amplifier's own group delay to the path: behind an amplifier with memory the cascade keeps that
 * residual delay (a few hundredths of a sample), and an error figure against g0 x that does not remove delay first is meaningless.
 * Judge by the power outside the band, by the error after delay and gain removal and by the decoded frames.
 * Calls on ONE handle must be ordered on the device (one stream, or events of the caller's). */
typedef struct mcrx_hip_fbalign_s *mcrx_hip_fbalign_t;
typedef struct {
    uint32_t struct_size, max_lag;                      /* sizeof(mcrx_hip_fbalign_config); Lm: 8 .. 64 */
    float    full_scale, target_gain;                   /* E = 2^e is the least power of two >= full_scale; g0 */
    uint32_t min_rows, input_format;                    /* >= 1; 0 = cf32, 1 = sc16 */
} mcrx_hip_fbalign_config;
typedef struct {
    int64_t  tau_fp;                                    /* Q32 samples */
    double   s_re, s_im, res;                           /* the scale; Szz - Re(conj(alpha) bu) of the last update that was not degenerate */
    uint64_t updates, degenerate, clamped;              /* updates run; those that left the state as it was; row samples that clamped */
    int64_t  rows;                                      /* rows in the sums */
    uint64_t offered;                                   /* the host's count of the guard: rows offered since the last update or reset */
} mcrx_hip_fbalign_state;
/* MCRX_EINVAL before a device is looked for, *out cleared: null pointers, a wrong struct_size, and every value outside the ranges above */
int      mcrx_hip_fbalign_create(mcrx_hip_fbalign_t *out, const mcrx_hip_fbalign_config *cfg);
int      mcrx_hip_fbalign_destroy(mcrx_hip_fbalign_t q);
unsigned mcrx_hip_fbalign_halo(mcrx_hip_fbalign_t q);                                /* Lm + 17; 0 for a null handle */
unsigned mcrx_hip_fbalign_input_format(mcrx_hip_fbalign_t q);                        /* 0 for a null handle */
/* n + 2 halo samples at d_in (the handle's input format) -> n cf32 samples at d_out, asynchronously on `stream`.  n == 0: MCRX_OK,
 * nothing done.  MCRX_EINVAL, nothing written: a null handle or buffer, a cf32 buffer not 8-byte aligned, an sc16 input not 4-byte
 * aligned, n + 2 halo above 2^32, ranges that overlap in any way. */
int      mcrx_hip_fbalign_execute_device(mcrx_hip_fbalign_t q, const void *d_in, size_t n, void *d_out, void *stream);
/* n cf32 pairs (d_u[i], d_zh[i]); rows R .. n - R - 1 into the sums.  MCRX_EINVAL, nothing measured, the count as before: a null
 * handle or buffer, a buffer not 8-byte aligned, more than 2^32 samples, a call that would take the rows offered since the last update
 * or reset above 2^31. */
int      mcrx_hip_fbalign_measure_device(mcrx_hip_fbalign_t q, const void *d_u, const void *d_zh, size_t n, void *stream);
int      mcrx_hip_fbalign_update(mcrx_hip_fbalign_t q, void *stream);
/* a known path: tau_fp and s written, coefficients made of them; sums and counters stay.  MCRX_EINVAL, nothing written:
 * |tau_fp| > (Lm + 1) 2^32, s or fp32(s) not finite.  No synchronisation. */
int      mcrx_hip_fbalign_set(mcrx_hip_fbalign_t q, int64_t tau_fp, double s_re, double s_im, void *stream);
/* waits for the handle's work on `stream`.  coef: 35 floats -- c_0 .. c_31, fp32(s.re), fp32(s.im), (float) nd; sums: 2 (2 R + 19)
 * int64, (re, im) of C[-R] .. C[R], A[0] .. A[16], (Szz, 0).  Any of the three pointers may be null. */
int      mcrx_hip_fbalign_read(mcrx_hip_fbalign_t q, mcrx_hip_fbalign_state *state, float *coef, int64_t *sums, void *stream);
/* state, coefficients, sums, counters and the host's count as after create -- without synchronising the device: the next kernel of
 * the handle that touches them clears them.  Launches carry no filter code again. */
int      mcrx_hip_fbalign_reset(mcrx_hip_fbalign_t q);
/* host, no GPU: checks cfg as create does; *e and taps[8] = h_1 .. h_8 of it (each may be null); for the n floats v: q15[i] = Q15(v[i])
 * and bad[i] = 1 where it clamps or v[i] is not finite (n == 0: v, q15 and bad are not looked at); and, where coef is not null, the 32
 * coefficients and *nd of tau_fp (MCRX_EINVAL for |tau_fp| > (Lm + 1) 2^32; nd may be null). */
int      mcrx_hip_fbalign_selftest(const mcrx_hip_fbalign_config *cfg, int *e, float *taps, const float *v, size_t n, int32_t *q15,
                                   int32_t *bad, int64_t tau_fp, float *coef, int *nd);
const char *mcrx_hip_fbalign_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MCRX_HIP_H */
