"""liquid_usrp_amd -- MI355X-native drop-in for liquid-usrp's multichannel OFDM receive path.

This package is the Python face of ``lib/libmcrx_hip.so`` (hand-written gfx950 kernels behind
the C-ABI of ``include/mcrx_hip.h``).  :class:`multichannelrx` mirrors the reference C++ class
(``include/multichannelrx.h:29-83``): same constructor arguments, ``Execute`` / ``Reset`` /
``GetNumChannels``, per-channel callbacks with the ``framesync_callback`` argument list.

There is no CPU implementation here: if the HIP library or a GPU is missing, construction
raises.  (The CPU oracle under ``oracle/`` is test infrastructure and is never imported by
this package.)
"""
import collections
import ctypes as C
import math
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.environ.get("MCRX_LIB") or os.path.join(_HERE, "lib", "libmcrx_hip.so")      # (MCRX_LIB: A/B builds)

MCRX_OK, MCRX_EINVAL, MCRX_ENOMEM, MCRX_EHIP, MCRX_EUNSUPP, MCRX_EOVERFLOW, MCRX_EBUSY = 0, -1, -2, -3, -4, -5, -6
TILE = 16         # MCRX_TILE (include/mcrx_hip.h)
POSITION_MAX = 1 << 48      # MCRX_POSITION_MAX: channel-rate positions stay below it (mcrx_hip_reset_at, mcrx_hip_sync)
TX_TILE = 8       # granules of the transmit side (mctx_hip_traffic_tiles)

LIQUID_CRC_NONE, LIQUID_CRC_32 = 1, 6
LIQUID_FEC_NONE, LIQUID_FEC_HAMMING128, LIQUID_FEC_GOLAY2412, LIQUID_FEC_CONV_V27 = 1, 6, 7, 11
LIQUID_FEC_REP3, LIQUID_FEC_REP5, LIQUID_FEC_HAMMING74, LIQUID_FEC_HAMMING84 = 2, 3, 4, 5
LIQUID_MODEM_QAM16, LIQUID_MODEM_QAM64, LIQUID_MODEM_BPSK, LIQUID_MODEM_QPSK = 27, 29, 39, 40


def build(force=False):
    """Compile the HIP library for gfx950 with the in-tree Makefile (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    deps = [os.path.join(src, f) for f in os.listdir(src) if f.endswith((".hip", ".h", ".hpp"))]
    deps.append(os.path.join(_HERE, "..", "include", "mcrx_hip.h"))
    stale = (not os.path.exists(_LIBPATH)) or any(os.path.getmtime(d) > os.path.getmtime(_LIBPATH) for d in deps)
    if force or stale:
        subprocess.check_call(["make", "-C", src, "-s", "-j4"])
    return _LIBPATH


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_payload_len", C.c_uint32), ("max_frames", C.c_uint32),
                ("payload_soft", C.c_uint32), ("slab_blocks", C.c_uint32), ("channel_first", C.c_uint32),
                ("channel_count", C.c_uint32), ("batch_samples", C.c_uint32), ("single_channel", C.c_uint32),
                ("serial", C.c_uint32), ("chunk_blocks", C.c_uint32), ("defer_samples", C.c_uint32), ("front_end", C.c_uint32), ("skip_framesyms", C.c_uint32),
                ("worker_build", C.c_uint32), ("acquisition", C.c_uint32), ("scout_build", C.c_uint32), ("conv_scratch", C.c_uint32),
                ("input_format", C.c_uint32)]


INPUT_FORMATS = {"cf32": 0, "sc16": 1}      # mcrx_hip_config::input_format
OUTPUT_FORMATS = {"cf32": 0, "sc16": 1}     # mctx_hip_set_output_format


class FrameC(C.Structure):
    _fields_ = [("channel", C.c_uint32), ("header_valid", C.c_int32), ("payload_valid", C.c_int32),
                ("payload_len", C.c_uint32), ("header", C.c_uint8 * 8),
                ("evm", C.c_float), ("rssi", C.c_float), ("cfo", C.c_float),
                ("mod_scheme", C.c_uint32), ("mod_bps", C.c_uint32), ("check", C.c_uint32),
                ("fec0", C.c_uint32), ("fec1", C.c_uint32), ("num_framesyms", C.c_uint32),
                ("end_sample", C.c_uint64), ("payload", C.c_void_p), ("framesyms", C.c_void_p)]


_EXPORTS = {
    "mcrx_hip_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]),
    "mcrx_hip_destroy": (C.c_int, [C.c_void_p]),
    "mcrx_hip_reset": (C.c_int, [C.c_void_p]),
    "mcrx_hip_reset_at": (C.c_int, [C.c_void_p, C.c_uint64]),
    "mcrx_hip_num_channels": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_execute_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "mcrx_hip_execute_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mcrx_hip_execute_host_sc16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "mcrx_hip_execute_device_sc16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mcrx_hip_input_format": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_flush": (C.c_int, [C.c_void_p]),
    "mcrx_hip_poll": (C.c_int, [C.c_void_p]),
    "mcrx_hip_discard": (C.c_int, [C.c_void_p]),
    "mcrx_hip_stream_wait": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mcrx_hip_launches": (C.c_uint64, [C.c_void_p]),
    "mcrx_hip_history_tiles": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_stream_wait_launch": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    "mcrx_hip_spec_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]),
    "mcrx_hip_viterbi_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]),
    "mcrx_hip_frames_pending": (C.c_size_t, [C.c_void_p]),
    "mcrx_hip_next_frame": (C.c_int, [C.c_void_p, C.POINTER(FrameC)]),
    "mcrx_hip_drain_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mcrx_hip_frames_dropped": (C.c_uint64, [C.c_void_p]),
    "mcrx_hip_channelize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p]),
    "mcrx_hip_sync": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_size_t, C.c_void_p]),
    "mcrx_hip_restart": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mcrx_hip_get_taps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "mcrx_hip_nco_step": (C.c_uint32, [C.c_void_p]),
    "mcrx_hip_history_blocks": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_device": (C.c_int, [C.c_void_p]),
    "mcrx_hip_selftest_device_table": (C.c_int, []),
    "mcrx_hip_kernel_time_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "mcrx_hip_kernel_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]),
    "mcrx_hip_kernel_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "mcrx_hip_monitor_enable": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mcrx_hip_monitor_disable": (C.c_int, [C.c_void_p]),
    "mcrx_hip_monitor_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]),
    "mcrx_hip_monitor_nfft": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_last_error": (C.c_char_p, []),
    "msresamp_hip_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_float, C.c_float]),
    "msresamp_hip_destroy": (C.c_int, [C.c_void_p]),
    "msresamp_hip_reset": (C.c_int, [C.c_void_p]),
    "msresamp_hip_reset_at": (C.c_int, [C.c_void_p, C.c_uint64]),
    "msresamp_hip_get_delay": (C.c_float, [C.c_void_p]),
    "msresamp_hip_selftest": (C.c_int, [C.c_float, C.c_float, C.c_void_p]),
    "msresamp_hip_max_output": (C.c_size_t, [C.c_void_p, C.c_size_t]),
    "msresamp_hip_execute_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                              C.POINTER(C.c_size_t), C.c_void_p]),
    "msresamp_hip_set_input_format": (C.c_int, [C.c_void_p, C.c_uint]),
    "msresamp_hip_input_format": (C.c_uint, [C.c_void_p]),
    "msresamp_hip_execute_device_sc16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                   C.POINTER(C.c_size_t), C.c_void_p]),
    "msresamp_hip_set_output_format": (C.c_int, [C.c_void_p, C.c_uint]),
    "msresamp_hip_output_format": (C.c_uint, [C.c_void_p]),
    "msresamp_hip_set_output_gain": (C.c_int, [C.c_void_p, C.c_float]),
    "msresamp_hip_output_gain": (C.c_float, [C.c_void_p]),
    "msresamp_hip_clipped": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "msresamp_hip_time_first_stage": (C.c_int, [C.c_void_p, C.c_int]),
    "msresamp_hip_first_stage_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "msresamp_hip_last_error": (C.c_char_p, []),
    "mcrx_hip_pfb2_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint, C.c_uint, C.c_float]),
    "mcrx_hip_pfb2_destroy": (C.c_int, [C.c_void_p]),
    "mcrx_hip_pfb2_get_taps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "mcrx_hip_pfb2_analyze": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint64, C.c_void_p, C.c_void_p]),
    "mcrx_hip_pfb2_last_error": (C.c_char_p, []),
    "mcrx_hip_pipeline_unique_id": (C.c_int, [C.c_void_p]),
    "mcrx_hip_pipeline_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_uint]),
    "mcrx_hip_pipeline_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mcrx_hip_pipeline_push_host": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mcrx_hip_pipeline_wait": (C.c_int, [C.c_void_p]),
    "mcrx_hip_pipeline_host_buffer": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "mcrx_hip_pipeline_reset": (C.c_int, [C.c_void_p, C.c_int64]),
    "mcrx_hip_pipeline_comm_count": (C.c_int, [C.c_void_p]),
    "mcrx_hip_pipeline_time_exchange": (C.c_int, [C.c_void_p, C.c_int]),
    "mcrx_hip_pipeline_exchange_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]),
    "mcrx_hip_pipeline_bytes_sent_per_round": (C.c_uint64, [C.c_void_p]),
    "mcrx_hip_pipeline_destroy": (C.c_int, [C.c_void_p]),
    "mcrx_hip_pipeline_last_error": (C.c_char_p, []),
    "mctx_hip_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]),
    "mctx_hip_destroy": (C.c_int, [C.c_void_p]),
    "mctx_hip_set_output_format": (C.c_int, [C.c_void_p, C.c_uint]),
    "mctx_hip_output_format": (C.c_uint, [C.c_void_p]),
    "mctx_hip_clipped": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "mctx_hip_selftest_quantise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "mctx_hip_blocks_for": (C.c_size_t, [C.c_void_p, C.c_uint, C.c_uint, C.c_int, C.c_int, C.c_int]),
    "mctx_hip_generate_ragged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint,
                                           C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "mctx_hip_generate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_uint, C.c_int, C.c_int, C.c_int,
                                    C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mctx_hip_traffic_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_int,
                                          C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mctx_hip_traffic_destroy": (C.c_int, [C.c_void_p]),
    "mctx_hip_traffic_tiles": (C.c_int, [C.c_void_p, C.c_longlong, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mctx_hip_synthesize_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint, C.c_longlong, C.c_size_t, C.c_size_t, C.c_size_t,
                                            C.c_float, C.c_void_p, C.c_void_p]),
    "mctx_hip_frame_len": (C.c_size_t, [C.c_void_p, C.c_uint, C.c_int, C.c_int, C.c_int]),
    "mctx_hip_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_float,
                                 C.c_void_p, C.c_size_t]),
    "mctx_hip_stream_begin": (C.c_int, [C.c_void_p, C.c_uint]),
    "mctx_hip_stream_ready": (C.c_int, [C.c_void_p, C.c_uint]),
    "mctx_hip_stream_update": (C.c_int, [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_int, C.c_int]),
    "mctx_hip_stream_generate": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mctx_hip_stream_reset": (C.c_int, [C.c_void_p]),
    "mctx_hip_last_error": (C.c_char_p, []),
    "mcrx_hip_chanemu_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p]),
    "mcrx_hip_chanemu_destroy": (C.c_int, [C.c_void_p]),
    "mcrx_hip_chanemu_reset": (C.c_int, [C.c_void_p]),
    "mcrx_hip_chanemu_reset_at": (C.c_int, [C.c_void_p, C.c_uint64]),
    "mcrx_hip_chanemu_position": (C.c_uint64, [C.c_void_p]),
    "mcrx_hip_chanemu_output_format": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_chanemu_execute_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mcrx_hip_chanemu_clipped": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "mcrx_hip_chanemu_selftest_words": (C.c_int, [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]),
    "mcrx_hip_chanemu_last_error": (C.c_char_p, []),
    "mcrx_hip_chanfade_set": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mcrx_hip_chanfade_on": (C.c_int, [C.c_void_p]),
    "mcrx_hip_chanfade_gains": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mcrx_hip_chanfade_selftest": (C.c_int, [C.c_void_p, C.c_uint, C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    "mcrx_hip_userchan_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint, C.c_void_p, C.c_size_t]),
    "mcrx_hip_userchan_destroy": (C.c_int, [C.c_void_p]),
    "mcrx_hip_userchan_num_channels": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_userchan_lead_blocks": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_userchan_apply_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mcrx_hip_userchan_last_error": (C.c_char_p, []),
    "mcrx_hip_userfade_set": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mcrx_hip_userfade_on": (C.c_int, [C.c_void_p]),
    "mcrx_hip_userfade_selftest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint, C.POINTER(C.c_int64), C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_float)]),
    "mcrx_hip_userfade_gains": (C.c_int, [C.c_void_p, C.c_longlong, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mcrx_hip_userclock_set": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mcrx_hip_userclock_on": (C.c_int, [C.c_void_p]),
    "mcrx_hip_userclock_lead_blocks": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_userclock_selftest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.POINTER(C.c_int64), C.POINTER(C.c_float)]),
    "mcrx_hip_userclock_table": (C.c_int, [C.POINTER(C.c_float)]),
    "mcrx_hip_userclock_apply_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mcrx_hip_rfchain_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p]),
    "mcrx_hip_rfchain_destroy": (C.c_int, [C.c_void_p]),
    "mcrx_hip_rfchain_execute_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mcrx_hip_rfchain_clipped": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "mcrx_hip_rfchain_input_format": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_rfchain_output_format": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_rfchain_selftest": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    "mcrx_hip_rfchain_phase_rows": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mcrx_hip_rfchain_last_error": (C.c_char_p, []),
    "mcrx_hip_rfcal_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p]),
    "mcrx_hip_rfcal_destroy": (C.c_int, [C.c_void_p]),
    "mcrx_hip_rfcal_reset_at": (C.c_int, [C.c_void_p, C.c_uint64]),
    "mcrx_hip_rfcal_position": (C.c_uint64, [C.c_void_p]),
    "mcrx_hip_rfcal_execute_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mcrx_hip_rfcal_update": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mcrx_hip_rfcal_hold": (C.c_int, [C.c_void_p, C.c_int]),
    "mcrx_hip_rfcal_set": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "mcrx_hip_rfcal_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mcrx_hip_rfcal_clipped": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "mcrx_hip_rfcal_selftest": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_size_t,
                                          C.POINTER(C.c_uint64)]),
    "mcrx_hip_rfcal_last_error": (C.c_char_p, []),
    "mcrx_hip_cfr_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p]),
    "mcrx_hip_cfr_destroy": (C.c_int, [C.c_void_p]),
    "mcrx_hip_cfr_halo": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_cfr_output_format": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_cfr_execute_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mcrx_hip_cfr_clipped": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "mcrx_hip_cfr_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.c_int]),
    "mcrx_hip_cfr_design": (C.c_int, [C.c_uint32, C.c_double, C.c_double, C.POINTER(C.c_float)]),
    "mcrx_hip_cfr_last_error": (C.c_char_p, []),
    "mcrx_hip_dpd_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p]),
    "mcrx_hip_dpd_destroy": (C.c_int, [C.c_void_p]),
    "mcrx_hip_dpd_execute_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mcrx_hip_dpd_measure_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mcrx_hip_dpd_update": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mcrx_hip_dpd_set_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mcrx_hip_dpd_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mcrx_hip_dpd_reset": (C.c_int, [C.c_void_p]),
    "mcrx_hip_dpd_clipped": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "mcrx_hip_dpd_output_format": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_dpd_selftest": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.c_void_p]),
    "mcrx_hip_dpd_last_error": (C.c_char_p, []),
    "mcrx_hip_mpd_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p]),
    "mcrx_hip_mpd_destroy": (C.c_int, [C.c_void_p]),
    "mcrx_hip_mpd_lead": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_mpd_output_format": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_mpd_execute_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mcrx_hip_mpd_measure_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mcrx_hip_mpd_update": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mcrx_hip_mpd_set_tables": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mcrx_hip_mpd_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mcrx_hip_mpd_reset": (C.c_int, [C.c_void_p]),
    "mcrx_hip_mpd_clipped": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "mcrx_hip_mpd_selftest": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mcrx_hip_mpd_last_error": (C.c_char_p, []),
    "mcrx_hip_pamem_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p]),
    "mcrx_hip_pamem_destroy": (C.c_int, [C.c_void_p]),
    "mcrx_hip_pamem_lead": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_pamem_input_format": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_pamem_output_format": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_pamem_execute_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mcrx_hip_pamem_clipped": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "mcrx_hip_pamem_selftest": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mcrx_hip_pamem_last_error": (C.c_char_p, []),
    "mcrx_hip_fbalign_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p]),
    "mcrx_hip_fbalign_destroy": (C.c_int, [C.c_void_p]),
    "mcrx_hip_fbalign_halo": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_fbalign_input_format": (C.c_uint, [C.c_void_p]),
    "mcrx_hip_fbalign_execute_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mcrx_hip_fbalign_measure_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mcrx_hip_fbalign_update": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mcrx_hip_fbalign_set": (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_void_p]),
    "mcrx_hip_fbalign_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mcrx_hip_fbalign_reset": (C.c_int, [C.c_void_p]),
    "mcrx_hip_fbalign_selftest": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int64,
                                            C.c_void_p, C.POINTER(C.c_int)]),
    "mcrx_hip_fbalign_last_error": (C.c_char_p, []),
}

_lib = None


def exported_symbols():
    return sorted(_EXPORTS)


def lib():
    """Load libmcrx_hip.so (raises if it has not been built: there is no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIBPATH):
            raise RuntimeError("libmcrx_hip.so is not built (run __graft_entry__.build()); "
                               "liquid_usrp_amd has no CPU fallback")
        try:
            # PyTorch-ROCm bundles its own HIP runtime; load it first so this process holds a
            # single libamdhip64 (device buffers and streams are shared with torch tensors).
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(_LIBPATH)
        for name, (res, args) in _EXPORTS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


class McrxError(RuntimeError):
    pass


def _check(rc, allow=()):
    if rc != MCRX_OK and rc not in allow:
        msg = lib().mcrx_hip_last_error()
        raise McrxError("mcrx_hip error %d: %s" % (rc, msg.decode() if msg else ""))
    return rc


def _raise_rc(rc, name, last_error, einval_is_value_error=True):
    """The return code of the C call `name`: nothing on MCRX_OK, else ValueError (MCRX_EINVAL at the sites where that is an argument
    error) or McrxError, with the text of the operator's own last-error function."""
    if rc == MCRX_OK:
        return
    msg = last_error()
    msg = msg.decode() if msg else ""
    if rc == MCRX_EINVAL and einval_is_value_error:
        raise ValueError(msg)
    raise McrxError("%s failed (%d): %s" % (name, rc, msg))


def _format_code(value, table, what):
    """The code of a format given as one of `table`'s names or as a number equal to one of its codes; ValueError otherwise.  Touches
    no library: a bad format is an argument error on a machine without a device too."""
    code = table.get(value) if isinstance(value, str) else next((c for c in table.values() if c == value), None)
    if code is None:
        raise ValueError("%s must be one of %s or %s, not %r" % (what, sorted(table), sorted(table.values()), value))
    return code


def _empty_samples(n, fmt, device):
    """An uninitialised torch tensor of n samples in format `fmt` on `device`: int16 of shape (n, 2), or complex64 of shape (n,)."""
    import torch
    if fmt == OUTPUT_FORMATS["sc16"]:
        return torch.empty((n, 2), dtype=torch.int16, device=device)
    return torch.empty(n, dtype=torch.complex64, device=device)


def _sc16_device_samples(x, what):
    """The number of samples in x, an sc16 device tensor handed to a `what` ("receiver", "resampler"): int16, contiguous, whole pairs."""
    import torch
    if x.dtype != torch.int16:
        raise TypeError("this %s takes int16 device tensors (interleaved re, im), not %s" % (what, x.dtype))
    if not x.is_contiguous():
        raise ValueError("device samples must be contiguous")
    if x.numel() % 2:
        raise ValueError("an sc16 buffer holds (re, im) pairs: odd number of int16")
    return int(x.numel()) // 2


class Frame(object):
    """Arguments of one framesync_callback invocation (include/multichannelrx.h:45)."""
    __slots__ = ("channel", "header", "header_valid", "payload", "payload_valid", "evm", "rssi", "cfo",
                 "framesyms", "mod_scheme", "mod_bps", "check", "fec0", "fec1", "end_sample")

    def __repr__(self):
        return "Frame(ch=%d hv=%d pv=%d len=%d evm=%.2f end=%d)" % (
            self.channel, self.header_valid, self.payload_valid, len(self.payload), self.evm, self.end_sample)


def _dptr(t):
    """Raw device pointer of a torch tensor / int / None."""
    if t is None:
        return None
    if isinstance(t, int):
        return C.c_void_p(t)
    return C.c_void_p(t.data_ptr())


def _stream_ptr(stream):
    if stream is None:
        return None
    if isinstance(stream, int):
        return C.c_void_p(stream)
    return C.c_void_p(stream.cuda_stream)


class MonitorConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("nfft", C.c_uint32), ("window", C.c_uint32)]


MONITOR_WINDOWS = {"rect": 0, "rectangular": 0, "hann": 1, "hamming": 2}


def monitor_omega(num_channels, nfft, channel, kp):
    """Wideband frequency [radians per wideband sample] of signed bin kp, in (-nfft/2, nfft/2], of `channel`'s spectrum."""
    N = float(num_channels)
    return np.pi * (np.asarray(channel, np.float64) - (N - 1.0) / 2.0) / N + 2.0 * np.pi * np.asarray(kp, np.float64) / (nfft * 2.0 * N)


class MonitorReading(object):
    """One reading of the channel monitor: level[nch], peak[nch] (mean / largest |x|^2 per channel), psd[nch, nfft] (averaged
    periodogram, FFT order: bin 0 is the channel's centre), over nseg whole segments and nsamp samples per channel."""

    def __init__(self, level, peak, psd, nseg, nsamp, num_channels, channel_first=0):
        self.level, self.peak, self.psd = np.asarray(level, np.float64), np.asarray(peak, np.float32), np.asarray(psd, np.float64)
        self.nseg, self.nsamp, self.N, self.channel_first = int(nseg), int(nsamp), int(num_channels), int(channel_first)

    def level_db(self):
        return 10.0 * np.log10(np.maximum(self.level, 1e-300))

    def occupied(self, threshold_db):
        return self.level_db() > threshold_db

    def wideband(self):
        """(row, omega): the channels' spectra side by side in wideband frequency order -- per channel the signed bins
        -nfft/2 + 1 .. nfft/2 -- and the frequency of every bin.  The bank is critically sampled: the rows tile the band."""
        nch, nfft = self.psd.shape
        kp = np.arange(-nfft // 2 + 1, nfft // 2 + 1)
        row = self.psd[:, kp % nfft].reshape(-1)
        ch = self.channel_first + np.arange(nch)
        return row, monitor_omega(self.N, nfft, ch[:, None], kp[None, :]).reshape(-1)


class multichannelrx(object):
    """GPU multichannel OFDM receiver with the reference class's interface.

    multichannelrx(num_channels, M, cp_len, taper_len, p, userdata, callback)
      p         subcarrier allocation (bytes / uint8 array) or None for the default
      userdata  list of per-channel objects handed back to the callbacks (or None)
      callback  list of per-channel callables
                cb(header, header_valid, payload, payload_len, payload_valid, stats, userdata) -> int
                (stats is the :class:`Frame`: evm, rssi, cfo, framesyms, ...)
    Callbacks run on the calling thread at flush points (buffer full, Flush(), Reset(), close()),
    in the reference's order (frame end time, then channel).

    Keyword arguments are the fields of mcrx_hip_config.  input_format="sc16" (or 1) makes a receiver of 16-bit integer IQ:
    Execute then takes int16 arrays of interleaved (re, im) pairs, a sample meaning (re, im) * 2^-15.
    """

    def __init__(self, num_channels, M, cp_len, taper_len, p=None, userdata=None, callback=None, **cfg):
        self._h = C.c_void_p()
        self.N, self.K, self.M, self.cp = num_channels, 2 * num_channels, M, cp_len
        parr = None if p is None else np.ascontiguousarray(np.frombuffer(bytes(bytearray(p)), np.uint8))
        c = Config()
        c.struct_size = C.sizeof(Config)
        c.payload_soft = 1
        for k, v in cfg.items():
            setattr(c, k, _format_code(v, INPUT_FORMATS, "input_format") if k == "input_format" else v)
        rc = lib().mcrx_hip_create(C.byref(self._h), num_channels, M, cp_len, taper_len,
                                   None if parr is None else parr.ctypes.data, C.addressof(c))
        if rc != MCRX_OK:
            self._h = C.c_void_p()
            _raise_rc(rc, "mcrx_hip_create", lib().mcrx_hip_last_error)      # (MCRX_EINVAL: the reference prints the message and throws)
        self.userdata = list(userdata) if userdata is not None else [None] * num_channels
        self.callback = list(callback) if callback is not None else [None] * num_channels
        self.frames = []            # every frame delivered so far (also handed to the callbacks)
        self.channel_first = int(c.channel_first)
        self.nch = int(c.channel_count) if c.channel_count else num_channels - self.channel_first
        self.input_format = int(c.input_format)

    # ---- reference API -----------------------------------------------------------------
    def GetNumChannels(self):
        return self.N

    def Execute(self, x, num_samples=None, stream=None):
        """Push samples: a complex64 numpy array (host) or a torch complex64 CUDA tensor (HBM).  An sc16 receiver
        (input_format="sc16") takes an int16 numpy array or a torch int16 CUDA tensor of interleaved (re, im) pairs instead;
        num_samples counts samples (pairs).  TypeError on the wrong dtype for an sc16 receiver, and on int16 for a cf32 one (whose other
        inputs are taken as before)."""
        sc16 = self.input_format == INPUT_FORMATS["sc16"]
        if hasattr(x, "is_cuda") and x.is_cuda:
            import torch
            if sc16:
                n = _sc16_device_samples(x, "receiver")
                n = n if num_samples is None else int(num_samples)
                _check(lib().mcrx_hip_execute_device_sc16(self._h, _dptr(x), n, _stream_ptr(stream)))
                return
            if x.dtype == torch.int16:
                raise TypeError("int16 samples need a receiver made with input_format=\"sc16\"")
            n = int(x.numel()) if num_samples is None else int(num_samples)
            _check(lib().mcrx_hip_execute_device(self._h, _dptr(x), n, _stream_ptr(stream)))
            return
        if sc16:
            a = np.asarray(x)
            if a.dtype != np.int16:
                raise TypeError("this receiver takes int16 samples (interleaved re, im), not %s" % a.dtype)
            a = np.ascontiguousarray(a)
            if a.size % 2:
                raise ValueError("an sc16 buffer holds (re, im) pairs: odd number of int16")
            n = a.size // 2 if num_samples is None else int(num_samples)
            _check(lib().mcrx_hip_execute_host_sc16(self._h, a.ctypes.data, n), allow=(MCRX_EOVERFLOW,))
            self._deliver(flush=False)
            return
        if getattr(x, "dtype", None) == np.int16:
            raise TypeError("int16 samples need a receiver made with input_format=\"sc16\"")
        a = np.ascontiguousarray(x, np.complex64)
        n = a.size if num_samples is None else int(num_samples)
        _check(lib().mcrx_hip_execute_host(self._h, a.ctypes.data, n), allow=(MCRX_EOVERFLOW,))   # drops are counted
        self._deliver(flush=False)

    def Reset(self):
        _check(lib().mcrx_hip_reset(self._h))
        self._deliver(flush=False)

    def reset_at(self, pos):
        """Reset() that also moves the stream to channel-rate sample `pos` (mcrx_hip_reset_at): frames then carry end_sample from
        there.  ValueError beyond MCRX_POSITION_MAX."""
        rc = lib().mcrx_hip_reset_at(self._h, int(pos))
        if rc == MCRX_EINVAL:
            raise ValueError(lib().mcrx_hip_last_error().decode())
        _check(rc)
        self._deliver(flush=False)

    # ---- additions -----------------------------------------------------------------------
    def Flush(self):
        """Process everything pushed so far and deliver the callbacks."""
        rc = lib().mcrx_hip_flush(self._h)
        _check(rc, allow=(MCRX_EOVERFLOW,))
        self._deliver(flush=False)
        return rc

    def Poll(self, deliver=True):
        """Overlapped harvest (mcrx_hip_poll): frames of everything pushed before the previous Poll."""
        rc = lib().mcrx_hip_poll(self._h)
        _check(rc, allow=(MCRX_EOVERFLOW,))
        if deliver:
            self._deliver(flush=False)
        return rc

    def Discard(self):
        _check(lib().mcrx_hip_discard(self._h))

    def frames_pending(self):
        return int(lib().mcrx_hip_frames_pending(self._h))

    def drain_count(self):
        """Walk the harvested frames through the C-ABI (mcrx_hip_drain_count: the loop a C caller writes around
        mcrx_hip_next_frame) without building Python objects; returns (frames, valid payloads, payload bytes)."""
        n, ok, nb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().mcrx_hip_drain_count(self._h, C.byref(n), C.byref(ok), C.byref(nb)))
        return int(n.value), int(ok.value), int(nb.value)

    def stream_wait(self, stream=None, launch=None):
        if launch is None:
            _check(lib().mcrx_hip_stream_wait(self._h, _stream_ptr(stream)))
        else:
            _check(lib().mcrx_hip_stream_wait_launch(self._h, launch, _stream_ptr(stream)))

    def spec_stats(self, reset=False):
        """(frames acquired by the scouts' own walk, frames adopted from speculative waves)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _check(lib().mcrx_hip_spec_stats(self._h, C.byref(a), C.byref(b), 1 if reset else 0))
        return int(a.value), int(b.value)

    def viterbi_stats(self, reset=False):
        """(frames through the K = 7 decoder's own kernel, forward passes repeated, traceback passes repeated)"""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().mcrx_hip_viterbi_stats(self._h, C.byref(a), C.byref(b), C.byref(c), 1 if reset else 0))
        return int(a.value), int(b.value), int(c.value)

    def _deliver(self, flush):
        f = FrameC()
        while lib().mcrx_hip_next_frame(self._h, C.byref(f)) == 1:
            fr = Frame()
            fr.channel = int(f.channel)
            fr.header = bytes(bytearray(f.header))
            fr.header_valid, fr.payload_valid = int(f.header_valid), int(f.payload_valid)
            fr.payload = C.string_at(f.payload, f.payload_len) if f.payload and f.payload_len else b""
            fr.evm, fr.rssi, fr.cfo = float(f.evm), float(f.rssi), float(f.cfo)
            if f.framesyms and f.num_framesyms:
                buf = (C.c_float * (2 * f.num_framesyms)).from_address(f.framesyms)
                fr.framesyms = np.frombuffer(buf, np.float32).copy().view(np.complex64)
            else:
                fr.framesyms = np.zeros(0, np.complex64)
            fr.mod_scheme, fr.mod_bps = int(f.mod_scheme), int(f.mod_bps)
            fr.check, fr.fec0, fr.fec1 = int(f.check), int(f.fec0), int(f.fec1)
            fr.end_sample = int(f.end_sample)
            self.frames.append(fr)
            cb = self.callback[fr.channel] if fr.channel < len(self.callback) else None
            if cb is not None:
                cb(fr.header, fr.header_valid, fr.payload, len(fr.payload), fr.payload_valid, fr,
                   self.userdata[fr.channel])

    # ---- stage level (bench / multi-GPU / parity tests) ------------------------------------
    def taps(self):
        h = np.zeros(14 * self.K, np.float32)
        _check(lib().mcrx_hip_get_taps(self._h, h.ctypes.data, h.size))
        return h

    def nco_step(self):
        return int(lib().mcrx_hip_nco_step(self._h))

    def history_blocks(self):
        """Blocks of 2N samples of filter history the analysis bank needs in front of a push (13; 27 with front_end = 1)."""
        return int(lib().mcrx_hip_history_blocks(self._h))

    def channelize(self, d_iq, nblocks, first_sample, d_out, groups=1, d_halo=None, stream=None):
        """mcrx_hip_channelize: d_iq and d_halo in the receiver's input format (complex64, or int16 pairs), d_out complex64 tiles."""
        _check(lib().mcrx_hip_channelize(self._h, _dptr(d_iq), nblocks, first_sample, _dptr(d_halo),
                                         _dptr(d_out), groups, _stream_ptr(stream)))

    def sync(self, d_chan, first_sample, nsamples, stream=None):
        """Returns the launch number (for stream_wait).  first_sample may be negative (history in front of sample 0)."""
        _check(lib().mcrx_hip_sync(self._h, _dptr(d_chan), first_sample & 0xFFFFFFFFFFFFFFFF, nsamples, _stream_ptr(stream)))
        return int(lib().mcrx_hip_launches(self._h)) - 1

    @property
    def hist_tiles(self):
        """tiles of channel-rate history a stage-level sync needs in front of new samples"""
        return int(lib().mcrx_hip_history_tiles(self._h))

    def restart(self, stream=None):
        _check(lib().mcrx_hip_restart(self._h, _stream_ptr(stream)))

    def kernel_time_ms(self):
        a, b = C.c_float(0), C.c_float(0)
        _check(lib().mcrx_hip_kernel_time_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def kernel_timing(self, on=True):
        """per-kernel HIP-event timing on / off (off in a new receiver); returns the previous setting"""
        return bool(lib().mcrx_hip_kernel_timing(self._h, 1 if on else 0))

    def kernel_stats(self, reset=False):
        """{kernel: (total_ms, launches)} from HIP events recorded on the launch stream while kernel_timing() was on."""
        names = ("channelizer_kernel", "sync_kernel", "place_jobs_kernel", "payload_kernel", "decode_kernel")
        ms, cnt = (C.c_double * len(names))(), (C.c_uint64 * len(names))()
        _check(lib().mcrx_hip_kernel_stats(self._h, ms, cnt, 1 if reset else 0))
        return {n: (ms[i], cnt[i]) for i, n in enumerate(names)}

    def frames_dropped(self):
        return int(lib().mcrx_hip_frames_dropped(self._h))

    # ---- channel monitor: level, peak and power spectrum per channel, on the GPU ------------
    def monitor_enable(self, nfft=64, window="hann"):
        """Switch the monitor on (or start a running one over).  window: "rect", "hann", "hamming" or the C-ABI's number."""
        c = MonitorConfig()
        c.struct_size, c.nfft = C.sizeof(MonitorConfig), int(nfft)
        c.window = MONITOR_WINDOWS[window] if isinstance(window, str) else int(window)
        rc = lib().mcrx_hip_monitor_enable(self._h, C.addressof(c))
        if rc == MCRX_EINVAL:
            raise ValueError(lib().mcrx_hip_last_error().decode())
        _check(rc)

    def monitor_disable(self):
        _check(lib().mcrx_hip_monitor_disable(self._h))

    def monitor_nfft(self):
        return int(lib().mcrx_hip_monitor_nfft(self._h))

    def monitor_read(self, reset=False):
        """What the monitor has seen since the last reset (waits for the monitor's launches only).  reset=True starts a new averaging
        interval and keeps the unfinished segment: one call per display interval gives one waterfall row."""
        nfft = self.monitor_nfft()
        if not nfft:
            raise ValueError("the monitor is off (monitor_enable)")
        level, peak, psd = np.zeros(self.nch, np.float64), np.zeros(self.nch, np.float32), np.zeros((self.nch, nfft), np.float64)
        nseg, nsamp = C.c_uint64(0), C.c_uint64(0)
        _check(lib().mcrx_hip_monitor_read(self._h, level.ctypes.data, peak.ctypes.data, psd.ctypes.data,
                                           C.byref(nseg), C.byref(nsamp), 1 if reset else 0))
        return MonitorReading(level, peak, psd, nseg.value, nsamp.value, self.N, self.channel_first)

    def close(self):
        if self._h:
            try:
                self.Flush()
            finally:
                lib().mcrx_hip_destroy(self._h)
                self._h = C.c_void_p()

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().mcrx_hip_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass


class _MsresampPlanStruct(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("interp", C.c_uint32), ("num_stages", C.c_uint32), ("reserved", C.c_uint32),
                ("step", C.c_uint64), ("per_in", C.c_uint64), ("per_out", C.c_uint64), ("rate_arb", C.c_double),
                ("delay", C.c_float), ("h1", C.c_float * 14), ("hpfb", (C.c_float * 14) * 256)]


MsresampPlan = collections.namedtuple("MsresampPlan", "interp num_stages rate_arb step per_in per_out delay h1 hpfb")


def msresamp_plan(rate, As=60.0):
    """What a resampler of this rate derives from it and uploads (msresamp_hip_selftest; host only, no device is looked for):
    interp, num_stages, rate_arb, step, per_in, per_out as Python numbers, delay (get_delay(): in input samples), h1 as float32 [14]
    and the branch table hpfb as float32 [256, 14], the tap on the oldest sample first.  ValueError for a rate create refuses."""
    st = _MsresampPlanStruct()
    st.struct_size = C.sizeof(st)
    _raise_rc(lib().msresamp_hip_selftest(float(rate), float(As), C.addressof(st)), "msresamp_hip_selftest", lib().msresamp_hip_last_error)
    return MsresampPlan(bool(st.interp), int(st.num_stages), float(st.rate_arb), int(st.step), int(st.per_in), int(st.per_out),
                        float(st.delay), np.array(st.h1, np.float32), np.array(st.hpfb, np.float32).reshape(256, 14))


class msresamp(object):
    """GPU mirror of liquid's msresamp_crcf as the reference front ends use it
    (src/flexframe_rx.cc:179,240): msresamp(rate, As); execute(x) -> y, with x / y torch
    complex64 CUDA tensors (IQ stays in HBM).  rate <= 1 decimates (receive front ends), rate > 1 interpolates
    (the transmit applications' msresamp_crcf_create(2.0, 60), src/flexframe_tx.cc:170).
    input_format="sc16" (or 1) makes a resampler of 16-bit integer IQ: execute then takes a torch int16 CUDA tensor of interleaved
    (re, im) pairs, a sample meaning (re, im) * 2^-15, and returns complex64 as before -- bit for bit what a cf32 handle returns on
    those floats.
    gain (default 1.0) multiplies every output component, one fp32 multiply.  output_format="sc16" (or 1) makes execute return a
    contiguous torch int16 CUDA tensor of shape (nout, 2), the transmitter's quantiser applied to what a cf32 resampler of the same
    gain returns (msresamp_hip_set_output_format); clipped() counts the samples that left the int16 range."""

    def __init__(self, rate, As=60.0, input_format="cf32", output_format="cf32", gain=1.0):
        self._h = C.c_void_p()
        output_format = _format_code(output_format, OUTPUT_FORMATS, "output_format")
        gain = float(gain)
        if not math.isfinite(gain):
            raise ValueError("gain must be finite")
        input_format = _format_code(input_format, INPUT_FORMATS, "input_format")
        rc = lib().msresamp_hip_create(C.byref(self._h), rate, As)
        if rc != MCRX_OK:
            self._h = C.c_void_p()
            self._chk(rc, "msresamp_hip_create")
        self.rate = rate
        if input_format:
            self._chk(lib().msresamp_hip_set_input_format(self._h, input_format), "msresamp_hip_set_input_format", False)
        if output_format:
            self.output_format = output_format
        if gain != 1.0:
            self.gain = gain

    @staticmethod
    def _chk(rc, name, einval_is_value_error=True):
        _raise_rc(rc, name, lib().msresamp_hip_last_error, einval_is_value_error)

    @property
    def input_format(self):
        """0 (cf32) or 1 (sc16): INPUT_FORMATS"""
        return int(lib().msresamp_hip_input_format(self._h))

    @property
    def output_format(self):
        """0 (cf32) or 1 (sc16): OUTPUT_FORMATS.  May be set between any two execute calls."""
        return int(lib().msresamp_hip_output_format(self._h))

    @output_format.setter
    def output_format(self, v):
        v = _format_code(v, OUTPUT_FORMATS, "output_format")
        self._chk(lib().msresamp_hip_set_output_format(self._h, v), "msresamp_hip_set_output_format")

    @property
    def gain(self):
        """The output gain (msresamp_hip_set_output_gain): finite, applies to both output formats, may be set between any two calls."""
        return float(lib().msresamp_hip_output_gain(self._h))

    @gain.setter
    def gain(self, v):
        self._chk(lib().msresamp_hip_set_output_gain(self._h, float(v)), "msresamp_hip_set_output_gain")

    def clipped(self, reset=False):
        """Samples clipped by sc16-output calls since the count was last reset (waits for the last such call's kernels only)."""
        n = C.c_uint64(0)
        self._chk(lib().msresamp_hip_clipped(self._h, C.byref(n), 1 if reset else 0), "msresamp_hip_clipped")
        return int(n.value)

    def get_delay(self):
        """The delay of the chain in input samples of the resampler (msresamp_plan(rate).delay)."""
        return float(lib().msresamp_hip_get_delay(self._h))

    def reset(self, at=0):
        """Start over with zero history, at input sample `at` of the stream (msresamp_hip_reset_at: a multiple of 2^num_stages)."""
        self._chk(lib().msresamp_hip_reset_at(self._h, int(at)), "msresamp_hip_reset_at")

    def execute(self, x, stream=None):
        """x: the new samples, a torch CUDA tensor -- complex64, or on an sc16 resampler int16 of 2 n elements (interleaved re, im;
        shape (n, 2) is fine).  Returns complex64, or on an sc16-output resampler int16 of shape (nout, 2).  TypeError on a tensor of
        the other input format's dtype."""
        import torch
        sc16 = self.input_format == INPUT_FORMATS["sc16"]
        if sc16:
            n = _sc16_device_samples(x, "resampler")
            fn, name = lib().msresamp_hip_execute_device_sc16, "msresamp_hip_execute_device_sc16"
        else:
            if x.dtype == torch.int16:
                raise TypeError("int16 samples need a resampler made with input_format=\"sc16\"")
            n = int(x.numel())
            fn, name = lib().msresamp_hip_execute_device, "msresamp_hip_execute_device"
        cap = int(lib().msresamp_hip_max_output(self._h, n)) + 8
        y = _empty_samples(cap, self.output_format, x.device)
        nout = C.c_size_t(0)
        self._chk(fn(self._h, _dptr(x), n, _dptr(y), cap, C.byref(nout), _stream_ptr(stream)), name, False)
        return y[:nout.value]

    def time_first_stage(self, enable=True):
        """Measurement aid (msresamp_hip_time_first_stage): time the kernel that reads the caller's samples, call by call."""
        self._chk(lib().msresamp_hip_time_first_stage(self._h, int(bool(enable))), "msresamp_hip_time_first_stage", False)

    def first_stage_ms(self):
        """Milliseconds the first stage of the last timed execute took on the device (waits for it)."""
        ms = C.c_float(0)
        self._chk(lib().msresamp_hip_first_stage_ms(self._h, C.byref(ms)), "msresamp_hip_first_stage_ms", False)
        return float(ms.value)

    def close(self):
        if self._h:
            lib().msresamp_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


CHANEMU_MAX_TAPS, CHANEMU_MAX_DELAY = 8, 65535      # MCRX_CHANEMU_MAX_TAPS, MCRX_CHANEMU_MAX_DELAY


class ChanemuConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("num_taps", C.c_uint32), ("delay", C.c_uint32 * CHANEMU_MAX_TAPS),
                ("tap_re", C.c_float * CHANEMU_MAX_TAPS), ("tap_im", C.c_float * CHANEMU_MAX_TAPS),
                ("cfo_step", C.c_uint32), ("phase0", C.c_uint32), ("gain", C.c_float), ("noise_std", C.c_float),
                ("seed", C.c_uint64), ("output_format", C.c_uint32)]


CHANEMU_MAX_SINUSOIDS = 16                          # MCRX_CHANEMU_MAX_SINUSOIDS


class ChanemuFading(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("log2_block", C.c_uint32), ("num_sinusoids", C.c_uint32), ("table_rows", C.c_uint32),
                ("doppler", C.c_double * CHANEMU_MAX_TAPS), ("los_doppler", C.c_double * CHANEMU_MAX_TAPS),
                ("rice_k", C.c_float * CHANEMU_MAX_TAPS), ("los_phase", C.c_uint32 * CHANEMU_MAX_TAPS), ("seed", C.c_uint64)]


_FADING_KEYS = ("doppler", "rice_k", "los_doppler", "los_phase", "sinusoids", "log2_block", "seed", "table_rows")


def chanemu_fading(num_taps, doppler=0.0, rice_k=0.0, los_doppler=0.0, los_phase=0, sinusoids=16, log2_block=10, seed=0, table_rows=0):
    """The mcrx_hip_chanemu_fading structure of a fading description for `num_taps` rays; per-ray entries are scalars (every ray gets
    them) or sequences of num_taps values.  Raises ValueError for what the library would refuse."""
    def per_ray(v, name, conv):
        vals = [conv(x) for x in v] if hasattr(v, "__len__") else [conv(v)] * num_taps
        if len(vals) != num_taps:
            raise ValueError("fading: %s has %d entries for %d rays" % (name, len(vals), num_taps))
        return vals
    for v, name, lo, hi in ((log2_block, "log2_block", 1, 24), (sinusoids, "sinusoids", 1, CHANEMU_MAX_SINUSOIDS)):
        if int(v) != v or not lo <= int(v) <= hi:
            raise ValueError("fading: %s must be %d .. %d" % (name, lo, hi))
    if int(table_rows) != table_rows or int(table_rows) == 1 or not 0 <= int(table_rows) < (1 << 32):
        raise ValueError("fading: table_rows must be 0 (default) or 2 .. 2^32 - 1")
    f = ChanemuFading()
    f.struct_size, f.log2_block, f.num_sinusoids, f.table_rows = C.sizeof(ChanemuFading), int(log2_block), int(sinusoids), int(table_rows)
    B = float(1 << int(log2_block))
    fd, fl = per_ray(doppler, "doppler", float), per_ray(los_doppler, "los_doppler", float)
    rk, ph = per_ray(rice_k, "rice_k", float), per_ray(los_phase, "los_phase", int)
    for i in range(num_taps):
        if not (math.isfinite(fd[i]) and math.isfinite(fl[i])):
            raise ValueError("fading: a Doppler is not finite")
        if fd[i] < 0.0 or fd[i] * B > 0.125 or abs(fl[i]) * B > 0.125:
            raise ValueError("fading: 0 <= doppler and doppler * 2^log2_block <= 1/8 (|los_doppler| likewise): the grid must sample the gain")
        if not (math.isfinite(rk[i]) and rk[i] >= 0.0 and math.isfinite(C.c_float(rk[i]).value)):
            raise ValueError("fading: rice_k must be finite and not negative")
        f.doppler[i], f.los_doppler[i], f.rice_k[i], f.los_phase[i] = fd[i], fl[i], rk[i], ph[i] % (1 << 32)
    f.seed = int(seed) % (1 << 64)
    return f


def chanemu_doppler(cycles_per_ofdm_symbol, M, cp, num_channels):
    """The chanemu Doppler (cycles per wideband sample) of a gain that turns `cycles_per_ofdm_symbol` cycles in one OFDM symbol of a
    user channel: a symbol is M + cp channel-rate samples, each 2 * num_channels wideband samples."""
    return float(cycles_per_ofdm_symbol) / ((M + cp) * 2 * num_channels)


def chanemu_cfo_step(spacings, M, num_channels):
    """The chanemu cfo_step (2^32 * cycles per wideband sample, mod 2^32) of a carrier offset of `spacings` subcarrier spacings as
    every channel's synchronizer sees it: a channel-rate sample is 2 * num_channels wideband samples, a spacing 1 / M cycles of those."""
    return int(round(float(spacings) / (M * 2 * num_channels) * 4294967296.0)) % (1 << 32)


def _whole(v, name):
    """v as the uint32 field `name` of a configuration"""
    if isinstance(v, bool) or int(v) != v or not 0 <= int(v) < (1 << 32):
        raise ValueError("%s must be a whole number, 0 .. 2^32 - 1" % name)
    return int(v)


class _StreamOp(object):
    """What the classes of the stream operators share (chanemu, rfchain, cfr, rfcal, dpd, mpd, pamem): the handle of mcrx_hip_<_op>_create, errors through
    mcrx_hip_<_op>_last_error, the clip count, close, and what execute checks of x and out.  _what: who takes the samples, and the noun
    of "this ..." in the messages."""
    _op, _what, _h = None, None, None

    @classmethod
    def _call(cls, name, *args):
        name = "mcrx_hip_%s_%s" % (cls._op, name)
        cls._chk(getattr(lib(), name)(*args), name)

    @classmethod
    def _chk(cls, rc, name):
        _raise_rc(rc, name, getattr(lib(), "mcrx_hip_%s_last_error" % cls._op))

    def _create(self, cfg):
        self._h = C.c_void_p()
        try:
            self._call("create", C.byref(self._h), C.addressof(cfg))
        except Exception:
            self._h = C.c_void_p()
            raise

    def _in(self, x, in16):
        """The number of samples in x: a contiguous CUDA tensor, complex64 or (in16) int16 pairs."""
        import torch
        if in16:
            n = _sc16_device_samples(x, self._what[1])
        else:
            if x.dtype != torch.complex64:
                raise TypeError("%s takes complex64 device tensors, not %s" % (self._what[0], x.dtype))
            n = int(x.numel())
        if not x.is_cuda or not x.is_contiguous():
            raise ValueError("device samples must be contiguous CUDA tensors")
        return n

    def _out(self, n, out, out16, device):
        """(out, view): out as given, or made, with room for n samples of the output format, and its first n samples as execute returns them."""
        import torch
        if out is None:
            out = _empty_samples(n, self.output_format, device)
        else:
            if out.dtype != (torch.int16 if out16 else torch.complex64):
                raise TypeError("out must be %s for this %s" % ("int16" if out16 else "complex64", self._what[1]))
            if not out.is_cuda or not out.is_contiguous() or int(out.numel()) < (2 * n if out16 else n):
                raise ValueError("out must be a contiguous CUDA tensor with room for %d samples" % n)
        return out, (out.view(-1, 2)[:n] if out16 else out.view(-1)[:n])

    def _io(self, x, out, in16, out16):
        """(n, out, view) of an execute call on x: _in, then _out.  With n == 0 there is no address to pass: execute returns the view."""
        n = self._in(x, in16)
        return (n,) + self._out(n, out, out16, x.device)

    @staticmethod
    def _stream(stream, x):
        """the stream to pass: the one given, or torch's current stream of x's device"""
        import torch
        return _stream_ptr(torch.cuda.current_stream(x.device) if stream is None else stream)

    @staticmethod
    def _current(stream):
        """the stream to pass where no tensor names a device: the one given, or torch's current stream"""
        import torch
        return _stream_ptr(torch.cuda.current_stream() if stream is None else stream)

    def clipped(self, reset=False):
        """Samples clipped by the sc16-out calls since the count was last reset (waits for the last such call only); 0 on a cf32 one."""
        n = C.c_uint64(0)
        self._call("clipped", self._h, C.byref(n), 1 if reset else 0)
        return int(n.value)

    def close(self):
        if self._h:
            getattr(lib(), "mcrx_hip_%s_destroy" % self._op)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class chanemu(_StreamOp):
    """Channel emulator on the wideband stream, between multichanneltx and multichannelrx / msresamp (mcrx_hip_chanemu_*):

        chanemu(taps=[(delay, complex), ...], cfo_step=0, phase0=0, gain=1.0, noise_std=0.0, seed=0, output_format="cf32")

    1 .. 8 taps, delays in wideband samples (<= 65535), summed in the order given; cfo_step / phase0 are 32-bit phases (chanemu_cfo_step);
    noise_std is per component.  Everything is a function of the absolute sample index, so a stream may be cut into execute calls
    anywhere.  execute(x) takes a torch complex64 CUDA tensor and returns complex64, or with output_format="sc16" a contiguous int16
    tensor of shape (n, 2) -- the transmitter's quantiser applied to what a cf32 emulator returns; clipped() counts the samples that
    left the int16 range.

    fading=dict(doppler=..., rice_k=..., los_doppler=..., los_phase=..., sinusoids=16, log2_block=10, seed=0, table_rows=0) turns every
    ray into a Rayleigh (rice_k = 0) or Rician fading one: Doppler in cycles per wideband sample (chanemu_doppler), per ray or one
    value for all; the gains are updated every 2^log2_block samples and interpolated linearly between.  set_fading(None | dict) changes
    it between any two execute calls; it holds no stream state."""

    _op, _what = "chanemu", ("the emulator", "emulator")

    def __init__(self, taps=((0, 1.0),), cfo_step=0, phase0=0, gain=1.0, noise_std=0.0, seed=0, output_format="cf32", fading=None):
        output_format = _format_code(output_format, OUTPUT_FORMATS, "output_format")
        taps = list(taps)
        if not 1 <= len(taps) <= CHANEMU_MAX_TAPS:
            raise ValueError("1 .. %d taps" % CHANEMU_MAX_TAPS)
        c = ChanemuConfig()
        c.struct_size, c.num_taps = C.sizeof(ChanemuConfig), len(taps)
        for i, (d, a) in enumerate(taps):
            if int(d) != d or not 0 <= int(d) < (1 << 32):
                raise ValueError("a delay is a whole number of wideband samples, 0 .. %d" % CHANEMU_MAX_DELAY)
            c.delay[i], c.tap_re[i], c.tap_im[i] = int(d), complex(a).real, complex(a).imag
        c.cfo_step, c.phase0 = int(cfo_step) % (1 << 32), int(phase0) % (1 << 32)
        c.gain, c.noise_std, c.seed, c.output_format = float(gain), float(noise_std), int(seed) % (1 << 64), output_format
        fading = self._fading_struct(len(taps), fading)
        self._create(c)
        self.taps, self.output_format = [(int(d), complex(a)) for d, a in taps], output_format
        if fading is not None:
            self._chk(lib().mcrx_hip_chanfade_set(self._h, C.addressof(fading)), "mcrx_hip_chanfade_set")

    @staticmethod
    def _fading_struct(num_taps, fading):
        if fading is None:
            return None
        if not isinstance(fading, dict) or any(k not in _FADING_KEYS for k in fading):
            raise ValueError("fading is None or a dict with keys of %s" % (_FADING_KEYS,))
        return chanemu_fading(num_taps, **fading)

    def set_fading(self, fading):
        """None: fading off (the emulator of constant rays); a dict as at construction: fading on with these parameters.  The gains
        are a function of the absolute sample index, so this may be called between any two execute calls."""
        f = self._fading_struct(len(self.taps), fading)
        self._chk(lib().mcrx_hip_chanfade_set(self._h, C.addressof(f) if f is not None else None), "mcrx_hip_chanfade_set")

    def fading_on(self):
        return bool(lib().mcrx_hip_chanfade_on(self._h))

    def gains(self, first_row, rows, stream=None):
        """The gain table's rows first_row .. first_row + rows - 1 (grid row b = n >> log2_block) as a complex64 CUDA tensor
        [rows, num_taps]: what the execute calls interpolate between.  For tests and measurements."""
        import torch
        out = torch.zeros((int(rows), CHANEMU_MAX_TAPS), dtype=torch.complex64, device="cuda")
        if stream is None:
            stream = torch.cuda.current_stream(out.device)
        self._chk(lib().mcrx_hip_chanfade_gains(self._h, int(first_row) % (1 << 64), int(rows), _dptr(out), _stream_ptr(stream)),
                  "mcrx_hip_chanfade_gains")
        return out[:, :len(self.taps)]

    def execute(self, x, out=None, stream=None):
        """x: the next samples of the stream, a contiguous torch complex64 CUDA tensor.  out (optional): where they go -- complex64 of
        at least as many elements, or on an sc16 emulator int16 of shape (>= n, 2); it must not overlap x.  Returns the n samples
        written.  Asynchronous on `stream` (default: torch's current stream of x's device)."""
        n, out, view = self._io(x, out, False, self.output_format == OUTPUT_FORMATS["sc16"])
        if n:
            self._call("execute_device", self._h, _dptr(x), n, _dptr(out), self._stream(stream, x))
        return view

    def reset(self, at=0):
        """Zero history; the stream continues at absolute sample `at` (any 64-bit value): phase and noise follow from it."""
        self._chk(lib().mcrx_hip_chanemu_reset_at(self._h, int(at) % (1 << 64)), "mcrx_hip_chanemu_reset_at")

    def position(self):
        """absolute index of the next input sample"""
        return int(lib().mcrx_hip_chanemu_position(self._h))


RFCHAIN_MIXER, RFCHAIN_OSCILLATOR, RFCHAIN_AMPLIFIER = 1, 2, 4      # MCRX_RFCHAIN_* stage bits
RFCHAIN_ORDERS = {"tx": 0, "rx": 1}                                 # mixer, oscillator, amplifier / amplifier, oscillator, mixer


class RfchainConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("order", C.c_uint32), ("stages", C.c_uint32), ("input_format", C.c_uint32),
                ("output_format", C.c_uint32), ("alpha_re", C.c_float), ("alpha_im", C.c_float), ("beta_re", C.c_float),
                ("beta_im", C.c_float), ("dc_re", C.c_float), ("dc_im", C.c_float), ("pn_sinusoids", C.c_uint32),
                ("pn_log2_block", C.c_uint32), ("pn_table_rows", C.c_uint32), ("pn_rms", C.c_float), ("pn_bandwidth", C.c_double),
                ("pn_seed", C.c_uint64), ("amp_sat", C.c_float), ("amp_gain", C.c_float), ("amp_ampm", C.c_float),
                ("amp_smooth", C.c_uint32), ("gain", C.c_float)]


def rfchain_iq(gain_db, phase_deg, side="tx"):
    """The mixer coefficients dict(alpha=, beta=) of a modulator (side="tx") or demodulator ("rx") whose Q arm has gain_db more gain and
    phase_deg more phase than its I arm.  The image rejection is |alpha|^2 / |beta|^2."""
    if side not in ("tx", "rx"):
        raise ValueError("side must be 'tx' or 'rx', not %r" % (side,))
    g, phi = 10.0 ** (float(gain_db) / 20.0), math.radians(float(phase_deg))
    e = complex(math.cos(phi), math.sin(phi))
    alpha = (1.0 + g * e) / 2.0 if side == "tx" else (1.0 + g * e.conjugate()) / 2.0
    return dict(alpha=alpha, beta=(1.0 - g * e) / 2.0)


def rfchain_backoff(ibo_db, rms):
    """The amplifier's saturation amplitude A that puts a signal of amplitude `rms` ibo_db below it (input back-off)."""
    return float(rms) * 10.0 ** (float(ibo_db) / 20.0)


def rfchain_config(order="tx", mixer=None, phase_noise=None, amplifier=None, gain=1.0, input_format="cf32", output_format="cf32"):
    """The mcrx_hip_rfchain_config of rfchain's arguments.  ValueError for a malformed argument; the values themselves are judged by
    the library (mcrx_hip_rfchain_create, before it looks for a device)."""
    def section(d, name, required, optional):
        if d is None:
            return None
        if not isinstance(d, dict) or any(k not in required and k not in optional for k in d) or any(k not in d for k in required):
            raise ValueError("%s is None or a dict with %s and optionally %s" % (name, required, tuple(optional)))
        return dict(optional, **d)

    def whole(v, name, bits=32):
        if int(v) != v or not 0 <= int(v) < (1 << bits):
            raise ValueError("%s must be a whole number, 0 .. 2^%d - 1" % (name, bits))
        return int(v)
    c = RfchainConfig()
    c.struct_size = C.sizeof(RfchainConfig)
    if order not in RFCHAIN_ORDERS:
        raise ValueError("order must be 'tx' or 'rx', not %r" % (order,))
    c.order = RFCHAIN_ORDERS[order]
    c.input_format = _format_code(input_format, INPUT_FORMATS, "input_format")
    c.output_format = _format_code(output_format, OUTPUT_FORMATS, "output_format")
    c.gain = float(gain)
    m = section(mixer, "mixer", ("alpha", "beta"), dict(dc=0.0))
    if m is not None:
        al, be, dc = complex(m["alpha"]), complex(m["beta"]), complex(m["dc"])
        c.alpha_re, c.alpha_im, c.beta_re, c.beta_im, c.dc_re, c.dc_im = al.real, al.imag, be.real, be.imag, dc.real, dc.imag
        c.stages |= RFCHAIN_MIXER
    p = section(phase_noise, "phase_noise", ("rms_deg", "bandwidth"), dict(sinusoids=16, log2_block=10, seed=0, table_rows=0))
    if p is not None:
        c.pn_sinusoids, c.pn_log2_block = whole(p["sinusoids"], "sinusoids"), whole(p["log2_block"], "log2_block")
        c.pn_table_rows, c.pn_seed = whole(p["table_rows"], "table_rows"), int(p["seed"]) % (1 << 64)
        c.pn_rms, c.pn_bandwidth = math.radians(float(p["rms_deg"])), float(p["bandwidth"])
        c.stages |= RFCHAIN_OSCILLATOR
    a = section(amplifier, "amplifier", ("sat",), dict(smooth=2, gain=1.0, ampm_deg=0.0))
    if a is not None:
        c.amp_sat, c.amp_gain, c.amp_ampm = float(a["sat"]), float(a["gain"]), float(a["ampm_deg"]) / 360.0
        c.amp_smooth = whole(a["smooth"], "smooth")
        c.stages |= RFCHAIN_AMPLIFIER
    return c


def rfchain_integers(cfg):
    """(steps, phases, c) of the oscillator of an RfchainConfig: the library's own integers N_k, Phi_k and its fp32 coefficient
    (mcrx_hip_rfchain_selftest; host only)."""
    S = int(cfg.pn_sinusoids)
    steps, phases, coef = (C.c_int64 * 16)(), (C.c_uint32 * 16)(), C.c_float()
    _raise_rc(lib().mcrx_hip_rfchain_selftest(C.addressof(cfg), steps, phases, C.byref(coef)), "mcrx_hip_rfchain_selftest",
              lib().mcrx_hip_rfchain_last_error)
    return [int(v) for v in steps[:S]], [int(v) for v in phases[:S]], float(coef.value)


class rfchain(_StreamOp):
    """RF front end on the wideband stream (mcrx_hip_rfchain_*): the radios at either end of the air.

        rfchain(order="tx", mixer=None | dict(alpha, beta, dc=0), phase_noise=None | dict(rms_deg, bandwidth, sinusoids=16,
                log2_block=10, seed=0, table_rows=0), amplifier=None | dict(sat, smooth=2, gain=1.0, ampm_deg=0.0), gain=1.0,
                input_format="cf32", output_format="cf32")

    mixer: u = alpha z + beta conj(z) + dc (rfchain_iq makes alpha, beta of an imbalance in dB and degrees); phase_noise: a stationary
    phase of rms_deg degrees rms with a Lorentzian line of half-width `bandwidth` cycles per sample, common to all channels;
    amplifier: Rapp AM/AM of smoothness 1, 2 or 4 that saturates at amplitude `sat` (rfchain_backoff) with a Saleh-shaped AM/PM that
    tends to ampm_deg.  order "tx" runs mixer, oscillator, amplifier; "rx" the reverse.  A section that is None is not computed.
    The operator is memoryless and stateless: execute(x, first_sample) takes the absolute index of x[0], so a stream may be cut, or
    sharded in time over GPUs, anywhere.  sc16 tensors are contiguous int16 of shape (n, 2)."""

    _op, _what = "rfchain", ("this front end", "front end")

    def __init__(self, order="tx", mixer=None, phase_noise=None, amplifier=None, gain=1.0, input_format="cf32", output_format="cf32"):
        c = rfchain_config(order, mixer, phase_noise, amplifier, gain, input_format, output_format)
        self._create(c)
        self.config, self.input_format, self.output_format, self.stages = c, int(c.input_format), int(c.output_format), int(c.stages)

    def execute(self, x, first_sample=0, out=None, stream=None):
        """x: samples first_sample .. first_sample + n - 1 of the stream, a contiguous CUDA tensor: complex64, or on an sc16-in handle
        int16 of shape (n, 2).  out (optional): where they go, in the output format, with room for n samples; `out is x` (the same
        address) is allowed with equal formats, any other overlap is refused.  Returns the n samples written.  Asynchronous on
        `stream` (default: torch's current stream of x's device)."""
        n, out, view = self._io(x, out, self.input_format == INPUT_FORMATS["sc16"], self.output_format == OUTPUT_FORMATS["sc16"])
        if n:
            self._call("execute_device", self._h, _dptr(x), int(first_sample) % (1 << 64), n, _dptr(out), self._stream(stream, x))
        return view

    def phase_rows(self, first_row, rows, stream=None):
        """The oscillator's table rows first_row .. first_row + rows - 1 (grid row b = n >> log2_block), in turns, as a float32 CUDA
        tensor: what the execute calls interpolate between.  For tests and measurements."""
        import torch
        out = torch.zeros(int(rows), dtype=torch.float32, device="cuda")
        if stream is None:
            stream = torch.cuda.current_stream(out.device)
        self._chk(lib().mcrx_hip_rfchain_phase_rows(self._h, int(first_row) % (1 << 64), int(rows), _dptr(out), _stream_ptr(stream)),
                  "mcrx_hip_rfchain_phase_rows")
        return out


CFR_MAX_HALF_LEN, CFR_MAX_PASSES = 64, 4      # MCRX_CFR_MAX_HALF_LEN, MCRX_CFR_MAX_PASSES


class CfrConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("half_len", C.c_uint32), ("passes", C.c_uint32), ("output_format", C.c_uint32),
                ("threshold", C.c_float), ("gain", C.c_float), ("taps", C.c_float * (CFR_MAX_HALF_LEN + 1))]


def cfr_lowpass(half_len, cutoff, beta):
    """The taps h[0 .. half_len] (float32) of the library's Kaiser-windowed low-pass of 2 half_len + 1 taps with its edge at `cutoff`
    cycles per sample, scaled to unit gain at zero frequency (mcrx_hip_cfr_design; host only)."""
    if int(half_len) != half_len or not 1 <= int(half_len) <= CFR_MAX_HALF_LEN:
        raise ValueError("half_len must be a whole number, 1 .. %d" % CFR_MAX_HALF_LEN)
    h = (C.c_float * (CFR_MAX_HALF_LEN + 1))()
    _raise_rc(lib().mcrx_hip_cfr_design(int(half_len), float(cutoff), float(beta), h), "mcrx_hip_cfr_design", lib().mcrx_hip_cfr_last_error)
    return np.array(h[:int(half_len) + 1], np.float32)


def cfr_threshold(papr_db, rms):
    """The threshold A that lies papr_db above a signal of amplitude `rms`: an absolute amplitude against the full scale 1.0."""
    return float(rms) * 10.0 ** (float(papr_db) / 20.0)


def cfr_config(threshold, taps=None, half_len=31, cutoff=0.28, beta=5.65, passes=1, gain=1.0, output_format="cf32"):
    """The mcrx_hip_cfr_config of cfr's arguments.  ValueError for a malformed argument; the values themselves are judged by the
    library (mcrx_hip_cfr_create, before it looks for a device)."""
    c = CfrConfig()
    c.struct_size = C.sizeof(CfrConfig)
    c.output_format = _format_code(output_format, OUTPUT_FORMATS, "output_format")
    if int(passes) != passes or not 0 <= int(passes) < (1 << 32):
        raise ValueError("passes must be a whole number")
    c.passes, c.threshold, c.gain = int(passes), float(threshold), float(gain)
    if taps is None:
        taps = cfr_lowpass(half_len, cutoff, beta)
    taps = np.asarray(taps)
    if taps.ndim != 1 or not 2 <= taps.size <= CFR_MAX_HALF_LEN + 1 or taps.dtype.kind not in "fiu":
        raise ValueError("taps are the real numbers h[0 .. H], H = 1 .. %d" % CFR_MAX_HALF_LEN)
    c.half_len = int(taps.size) - 1
    for k, v in enumerate(taps):
        c.taps[k] = float(v)
    return c


class cfr(_StreamOp):
    """Crest-factor reduction on the wideband stream (mcrx_hip_cfr_*): clip-and-filter between the transmitter and its DAC or amplifier.

        cfr(threshold, taps=None, half_len=31, cutoff=0.28, beta=5.65, passes=1, gain=1.0, output_format="cf32")

    What exceeds the amplitude `threshold` (absolute, against the full scale 1.0: cfr_threshold makes it of a level over the rms) is
    taken out of the stream, band-limited by the symmetric low-pass `taps` = h[0 .. H] (default: cfr_lowpass(half_len, cutoff, beta)),
    `passes` times over; then the gain, then cf32 or sc16.  It lowers the peaks and keeps the correction inside the occupied band; it
    adds in-band error to every channel.  The operator is stateless and non-causal: execute(x) takes n + 2 halo samples and returns
    the n in the middle, so a stream may be cut anywhere when each piece brings `halo` samples of its neighbours (zeros at the ends
    of the stream: pad=True).  With passes > 1 the calls on one handle must be ordered on the device."""

    _op, _what = "cfr", ("cfr", "handle")

    def __init__(self, threshold, taps=None, half_len=31, cutoff=0.28, beta=5.65, passes=1, gain=1.0, output_format="cf32"):
        c = cfr_config(threshold, taps, half_len, cutoff, beta, passes, gain, output_format)
        self._create(c)
        self.config, self.output_format, self.passes, self.half_len = c, int(c.output_format), int(c.passes), int(c.half_len)
        self.halo = int(lib().mcrx_hip_cfr_halo(self._h))
        self.taps = np.array(c.taps[:self.half_len + 1], np.float32)

    def execute(self, x, out=None, pad=False, stream=None):
        """x: a contiguous complex64 CUDA tensor of n + 2 halo samples -- the n samples to correct with `halo` of their neighbours on
        either side -- or, with pad=True, a whole stream of n samples, which gets zeros there.  out (optional): where the n samples
        go, in the output format; it must not overlap x.  Returns the n samples written.  Asynchronous on `stream` (default: torch's
        current stream of x's device)."""
        import torch
        self._in(x, False)
        if pad:
            padded = torch.zeros(int(x.numel()) + 2 * self.halo, dtype=torch.complex64, device=x.device)
            padded[self.halo:self.halo + int(x.numel())].copy_(x.view(-1))
            x = padded
        n = int(x.numel()) - 2 * self.halo
        if n < 0:
            raise ValueError("x must hold the halo on either side: at least %d samples" % (2 * self.halo))
        out, view = self._out(n, out, self.output_format == OUTPUT_FORMATS["sc16"], x.device)
        if n:
            self._call("execute_device", self._h, _dptr(x), n, _dptr(out), self._stream(stream, x))
        return view

    def stats(self, reset=False):
        """(over, peak2) since the last reset: over[p] = samples above the threshold at the input of pass p, among the samples of the
        outputs only; peak2 = the largest |y|^2 behind the last pass, before the gain.  Waits for the handle's last call."""
        over, peak2 = (C.c_uint64 * CFR_MAX_PASSES)(), C.c_float(0.0)
        self._chk(lib().mcrx_hip_cfr_stats(self._h, over, C.byref(peak2), 1 if reset else 0), "mcrx_hip_cfr_stats")
        return [int(v) for v in over[:self.passes]], float(peak2.value)


RFCAL_DC, RFCAL_IQ = 1, 2      # MCRX_RFCAL_* stage bits


class RfcalConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("stages", C.c_uint32), ("input_format", C.c_uint32), ("output_format", C.c_uint32),
                ("period_log2", C.c_uint32), ("forget_log2", C.c_uint32), ("gain", C.c_float)]


class RfcalState(C.Structure):
    _fields_ = [("m_re", C.c_float), ("m_im", C.c_float), ("w_re", C.c_float), ("w_im", C.c_float), ("mean", C.c_double * 5),
                ("acc", C.c_double * 5), ("acc_int", C.c_int64 * 5), ("count", C.c_uint64), ("updates", C.c_uint64),
                ("measured", C.c_uint64), ("degenerate", C.c_uint64)]


def rfcal_config(dc=True, iq=True, period_log2=0, forget_log2=30, gain=1.0, input_format="cf32", output_format="cf32"):
    """The mcrx_hip_rfcal_config of rfcal's arguments.  ValueError for a malformed argument; the values themselves are judged by the
    library (mcrx_hip_rfcal_create, before it looks for a device)."""
    c = RfcalConfig()
    c.struct_size = C.sizeof(RfcalConfig)
    if not isinstance(dc, (bool, np.bool_)) or not isinstance(iq, (bool, np.bool_)):
        raise ValueError("dc and iq are True or False")
    c.stages = (RFCAL_DC if dc else 0) | (RFCAL_IQ if iq else 0)
    c.input_format = _format_code(input_format, INPUT_FORMATS, "input_format")
    c.output_format = _format_code(output_format, OUTPUT_FORMATS, "output_format")
    c.period_log2, c.forget_log2 = _whole(period_log2, "period_log2"), _whole(forget_log2, "forget_log2")
    c.gain = float(gain)
    return c


def rfcal_segments(cfg, pos, n, cap=None):
    """(lengths, ends_block) of the segments the library splits the call (pos, n) of an RfcalConfig into (mcrx_hip_rfcal_selftest; host
    only); at most `cap` of them are listed (default: all).  ValueError where execute would refuse the call."""
    nseg = C.c_uint64(0)
    err = lib().mcrx_hip_rfcal_last_error
    _raise_rc(lib().mcrx_hip_rfcal_selftest(C.addressof(cfg), int(pos) % (1 << 64), int(n), None, None, 0, C.byref(nseg)),
              "mcrx_hip_rfcal_selftest", err)
    k = int(nseg.value) if cap is None else min(int(cap), int(nseg.value))
    lens, ends = (C.c_uint64 * max(k, 1))(), (C.c_uint32 * max(k, 1))()
    _raise_rc(lib().mcrx_hip_rfcal_selftest(C.addressof(cfg), int(pos) % (1 << 64), int(n), lens, ends, k, C.byref(nseg)),
              "mcrx_hip_rfcal_selftest", err)
    return [int(v) for v in lens[:k]], [bool(v) for v in ends[:k]]


def rfcal_as_mixer(m, w):
    """The rfchain mixer dict(alpha, beta, dc) that applies the correction (u - m) - w conj(u - m) of a finished calibration:
    rfchain(order="rx", mixer=rfcal_as_mixer(m, w)) is the frozen corrector."""
    m, w = complex(m), complex(w)
    return dict(alpha=1.0 + 0.0j, beta=-w, dc=-m + w * m.conjugate())


class rfcal(_StreamOp):
    """Receiver calibration on the wideband stream (mcrx_hip_rfcal_*): blind DC offset and IQ correction.

        rfcal(dc=True, iq=True, period_log2=0, forget_log2=30, gain=1.0, input_format="cf32", output_format="cf32")

    Stateful: the handle keeps the absolute position of its next sample, the moments of the raw input and the coefficients (m, w) made
    of them, all on the device.  execute(x) corrects x with the coefficients the handle holds and measures it for the next ones;
    measure(x) only measures.  period_log2 = k in 6 .. 30: the coefficients are renewed by themselves at every multiple of 2^k of the
    absolute index; 0: by update().  The running means are the cumulative mean of the blocks until 2^-forget_log2 is the larger weight.
    Calls on one handle must be ordered on the device.  sc16 tensors are contiguous int16 of shape (n, 2)."""

    _op, _what = "rfcal", ("this calibration", "calibration")

    def __init__(self, dc=True, iq=True, period_log2=0, forget_log2=30, gain=1.0, input_format="cf32", output_format="cf32"):
        c = rfcal_config(dc, iq, period_log2, forget_log2, gain, input_format, output_format)
        self._create(c)
        self.config, self.input_format, self.output_format = c, int(c.input_format), int(c.output_format)

    def execute(self, x, out=None, stream=None):
        """x: the next n samples of the stream, a contiguous CUDA tensor: complex64, or on an sc16-in handle int16 of shape (n, 2).
        out (optional): where the corrected samples go, in the output format, with room for n; `out is x` is allowed with equal
        formats, any other overlap is refused.  Returns the n samples written.  Asynchronous on `stream` (default: torch's current
        stream of x's device)."""
        n, out, view = self._io(x, out, self.input_format == INPUT_FORMATS["sc16"], self.output_format == OUTPUT_FORMATS["sc16"])
        if n:
            self._call("execute_device", self._h, _dptr(x), n, _dptr(out), self._stream(stream, x))
        return view

    def measure(self, x, stream=None):
        """The next n samples of the stream, measured only (nothing is written); returns n."""
        n = self._in(x, self.input_format == INPUT_FORMATS["sc16"])
        if n:
            self._call("execute_device", self._h, _dptr(x), n, None, self._stream(stream, x))
        return n

    def update(self, stream=None):
        """Make the coefficients of what has been measured (period_log2 = 0 handles only: ValueError otherwise)."""
        self._chk(lib().mcrx_hip_rfcal_update(self._h, self._current(stream)), "mcrx_hip_rfcal_update")

    def hold(self, on=True):
        """While held the handle measures nothing and no update runs: execute only applies."""
        self._chk(lib().mcrx_hip_rfcal_hold(self._h, 1 if on else 0), "mcrx_hip_rfcal_hold")

    def set(self, m, w, stream=None):
        """Write the coefficients: the DC offset m and the image coefficient w (complex, finite)."""
        m, w = complex(m), complex(w)
        self._chk(lib().mcrx_hip_rfcal_set(self._h, m.real, m.imag, w.real, w.imag, self._current(stream)), "mcrx_hip_rfcal_set")

    def read(self, stream=None):
        """The handle's state as a dict (waits for the handle's work on `stream`): m, w (complex, the fp32 coefficients), mean (the
        five running means s1.re, s1.im, s2.re, s2.im, p), acc (the block accumulators: exact Python ints on an sc16-in handle, floats
        otherwise), count, updates, measured, degenerate, and irr_db = -20 log10 |w| (inf while w is 0)."""
        s = RfcalState()
        self._chk(lib().mcrx_hip_rfcal_read(self._h, C.addressof(s), self._current(stream)), "mcrx_hip_rfcal_read")
        w = complex(s.w_re, s.w_im)
        acc = [int(v) for v in s.acc_int] if self.input_format == INPUT_FORMATS["sc16"] else [float(v) for v in s.acc]
        return dict(m=complex(s.m_re, s.m_im), w=w, mean=[float(v) for v in s.mean], acc=acc, count=int(s.count), updates=int(s.updates),
                    measured=int(s.measured), degenerate=int(s.degenerate), irr_db=-20.0 * math.log10(abs(w)) if abs(w) > 0.0 else math.inf)

    def reset_at(self, pos):
        """The next sample is absolute sample pos; coefficients, means, accumulators and counters are cleared (no synchronisation)."""
        self._chk(lib().mcrx_hip_rfcal_reset_at(self._h, int(pos) % (1 << 64)), "mcrx_hip_rfcal_reset_at")

    def position(self):
        return int(lib().mcrx_hip_rfcal_position(self._h))


class _Predistorter(_StreamOp):
    """What dpd and mpd share: a cf32-in handle with tables that measure and update learn or set_table(s) writes.  _pad: whether learn's
    execute pads the history."""
    _what, _pad = ("this predistorter", "predistorter"), {}

    def _measure(self, u, z, stream):
        """the samples of a measure call on u and z, offered to the library"""
        n = self._in(u, False)
        if self._in(z, False) != n:
            raise ValueError("u and z must hold equally many samples")
        if n:
            self._call("measure_device", self._h, _dptr(u), _dptr(z), n, self._stream(stream, u))
        return n

    def _set(self, name, F, shape, what, stream):
        """set_table / set_tables: F as complex64 of `shape`, written by the library's `name`"""
        F = np.ascontiguousarray(F, np.complex64)
        if F.shape != shape:
            raise ValueError("the %s complex entries" % (what % shape))
        self._call(name, self._h, F.ctypes.data, self._current(stream))

    def update(self, stream=None):
        """Make the table(s) of what has been measured (on the device, no synchronisation)."""
        self._call("update", self._h, self._current(stream))

    def reset(self):
        """Tables, sums and counters as after construction; execute copies again (no synchronisation)."""
        self._call("reset", self._h)

    def learn(self, x, amplifier, rounds=3, first_sample=0, stream=None, aligner=None):
        """`rounds` times: execute(x) (mpd: with pad=True) -> amplifier.execute(u, first_sample, stream=) -> measure -> update;
        `amplifier` is any object with such an execute that returns as many cf32 samples as it gets, an rfchain with cf32 in and out
        for one.  Returns the amplifier's output of the last round, which the table(s) of the round before it shaped.  With an
        `aligner` (an fbalign) the amplifier's output is what an observation receiver returned, as many samples in the aligner's input
        format: measure gets aligner.align(u, z, stream=)'s trimmed u and aligned capture instead of (u, z)."""
        if self.output_format != OUTPUT_FORMATS["cf32"]:
            raise ValueError("learn needs a cf32 predistorter: the feedback is the handle's cf32 output")
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(x.device)
        z = None
        for _ in range(int(rounds)):
            u = self.execute(x, stream=stream, **self._pad)
            z = amplifier.execute(u, first_sample, stream=stream)
            if aligner is None:
                self.measure(u, z, stream=stream)
            else:
                self.measure(*aligner.align(u, z, stream=stream), stream=stream)
            self.update(stream=stream)
        return z


DPD_MIN_LOG2, DPD_MAX_LOG2, DPD_MAX_FORGET, DPD_GUARD_LOG2 = 5, 10, 8, 28


class DpdConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("table_log2", C.c_uint32), ("full_scale", C.c_float), ("target_gain", C.c_float),
                ("min_count", C.c_uint32), ("forget_shift", C.c_uint32), ("gain", C.c_float), ("output_format", C.c_uint32)]


class DpdState(C.Structure):
    _fields_ = [("updates", C.c_uint64), ("skipped", C.c_uint64), ("degenerate", C.c_uint64)]


def dpd_config(table_log2=7, full_scale=None, target_gain=None, min_count=8, forget_shift=0, gain=1.0, output_format="cf32"):
    """The mcrx_hip_dpd_config of dpd's arguments.  ValueError for a malformed or missing argument and for every value the library
    refuses (mcrx_hip_dpd_selftest judges them on the host: no device is looked for)."""
    if full_scale is None or target_gain is None:
        raise ValueError("full_scale and target_gain must be given")
    c = DpdConfig()
    c.struct_size = C.sizeof(DpdConfig)
    c.output_format = _format_code(output_format, OUTPUT_FORMATS, "output_format")
    c.table_log2, c.min_count, c.forget_shift = _whole(table_log2, "table_log2"), _whole(min_count, "min_count"), _whole(forget_shift, "forget_shift")
    c.full_scale, c.target_gain, c.gain = float(full_scale), float(target_gain), float(gain)
    _raise_rc(lib().mcrx_hip_dpd_selftest(C.addressof(c), None, None, None, None, None, 0, None), "mcrx_hip_dpd_selftest",
              lib().mcrx_hip_dpd_last_error)
    return c


def dpd_constants(cfg):
    """(inv_step, step, e) of a DpdConfig: the library's own fp32 K / full_scale, its double full_scale / K and the exponent of the
    least power of two that is at least full_scale (mcrx_hip_dpd_selftest; host only)."""
    inv_step, step, e = C.c_float(), C.c_double(), C.c_int()
    _raise_rc(lib().mcrx_hip_dpd_selftest(C.addressof(cfg), C.byref(inv_step), C.byref(step), C.byref(e), None, None, 0, None),
              "mcrx_hip_dpd_selftest", lib().mcrx_hip_dpd_last_error)
    return float(inv_step.value), float(step.value), int(e.value)


def dpd_bins(cfg, u, z):
    """The bin of every pair (u[i], z[i]) as the measuring kernel finds it, -1 where the pair is not eligible (int32 array; host only)."""
    u, z = np.ascontiguousarray(u, np.complex64), np.ascontiguousarray(z, np.complex64)
    if u.ndim != 1 or u.shape != z.shape:
        raise ValueError("u and z are one-dimensional and equally long")
    out = np.zeros(len(u), np.int32)
    if len(u):
        _raise_rc(lib().mcrx_hip_dpd_selftest(C.addressof(cfg), None, None, None, u.ctypes.data, z.ctypes.data, len(u), out.ctypes.data),
                  "mcrx_hip_dpd_selftest", lib().mcrx_hip_dpd_last_error)
    return out


class dpd(_Predistorter):
    """Digital predistortion on the wideband stream (mcrx_hip_dpd_*): between cfr and the amplifier.

        dpd(table_log2=7, full_scale=, target_gain=, min_count=8, forget_shift=0, gain=1.0, output_format="cf32")

    A complex gain looked up by amplitude in a table of 2^table_log2 intervals up to `full_scale` and interpolated; it makes the
    amplifier behind it look like the linear gain `target_gain` below saturation.  It cannot undo saturation: put cfr in front, so
    that the peaks lie below it.  The table is learned on the device: measure(u, z) adds what went into the amplifier (u: this
    handle's cf32 output) and what came out (z, aligned and scaled by the caller) to integer sums per amplitude bin, update() makes
    the table of them; set_table writes one.  Until the first of either, execute copies.  Memoryless: a stream may be cut anywhere,
    and `out is x` is allowed on a cf32 handle.  Calls on one handle must be ordered on the device."""

    _op = "dpd"

    def __init__(self, table_log2=7, full_scale=None, target_gain=None, min_count=8, forget_shift=0, gain=1.0, output_format="cf32"):
        c = dpd_config(table_log2, full_scale, target_gain, min_count, forget_shift, gain, output_format)
        self._create(c)
        self.config, self.output_format, self.K = c, int(c.output_format), 1 << int(c.table_log2)

    def execute(self, x, out=None, stream=None):
        """x: n samples, a contiguous complex64 CUDA tensor.  out (optional): where they go, in the output format, with room for n;
        `out is x` is allowed with equal formats, any other overlap is refused.  Returns the n samples written.  Asynchronous on
        `stream` (default: torch's current stream of x's device)."""
        n, out, view = self._io(x, out, False, self.output_format == OUTPUT_FORMATS["sc16"])
        if n:
            self._call("execute_device", self._h, _dptr(x), n, _dptr(out), self._stream(stream, x))
        return view

    def measure(self, u, z, stream=None):
        """u, z: equally many samples into and out of the amplifier (contiguous complex64 CUDA tensors); returns their number.
        ValueError, nothing measured, where it would take the samples offered since the last reset above 2^28."""
        return self._measure(u, z, stream)

    def set_table(self, F, stream=None):
        """Write the table: K + 1 finite complex gains F[0 .. K]."""
        self._set("set_table", F, (self.K + 1,), "table holds %d", stream)

    def read(self, stream=None):
        """The handle's state as a dict (waits for the handle's work on `stream`): F (complex64 [K + 1]), cnt, Sre, Sim, Suu (int64
        [K + 1] each), updates, skipped, degenerate."""
        s, F, acc = DpdState(), np.zeros(self.K + 1, np.complex64), np.zeros((self.K + 1, 4), np.int64)
        self._call("read", self._h, C.addressof(s), F.ctypes.data, acc.ctypes.data, self._current(stream))
        return dict(F=F, cnt=acc[:, 0].copy(), Sre=acc[:, 1].copy(), Sim=acc[:, 2].copy(), Suu=acc[:, 3].copy(), updates=int(s.updates),
                    skipped=int(s.skipped), degenerate=int(s.degenerate))


MPD_MAX_BRANCHES, MPD_MAX_DELAY, MPD_MAX_ORDER, MPD_QB, MPD_GUARD_LOG2, MPD_MAX_WGS = 4, 16, 5, 17, 26, 1024


class MpdConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("branches", C.c_uint32), ("delay", C.c_uint32 * MPD_MAX_BRANCHES), ("order", C.c_uint32),
                ("table_log2", C.c_uint32), ("full_scale", C.c_float), ("target_gain", C.c_float), ("min_rows", C.c_uint32),
                ("ridge_log2", C.c_uint32), ("forget_shift", C.c_uint32), ("gain", C.c_float), ("output_format", C.c_uint32)]


class MpdState(C.Structure):
    _fields_ = [("updates", C.c_uint64), ("skipped", C.c_uint64), ("degenerate", C.c_uint64), ("rows", C.c_int64), ("res", C.c_double)]


def mpd_config(branches=None, delays=None, order=5, table_log2=7, full_scale=None, target_gain=None, min_rows=None, ridge_log2=30,
               forget_shift=0, gain=1.0, output_format="cf32"):
    """The mcrx_hip_mpd_config of mpd's arguments (min_rows: default 64 rows a coefficient).  ValueError for a malformed or missing
    argument and for every value the library refuses (mcrx_hip_mpd_selftest judges them on the host: no device is looked for)."""
    if branches is None or delays is None or full_scale is None or target_gain is None:
        raise ValueError("branches, delays, full_scale and target_gain must be given")
    c = MpdConfig()
    c.struct_size = C.sizeof(MpdConfig)
    c.output_format = _format_code(output_format, OUTPUT_FORMATS, "output_format")
    c.branches, c.order, c.table_log2 = _whole(branches, "branches"), _whole(order, "order"), _whole(table_log2, "table_log2")
    delays = [_whole(d, "a delay") for d in delays]
    if len(delays) != c.branches or not 1 <= len(delays) <= MPD_MAX_BRANCHES:
        raise ValueError("delays: one for each of the 1 .. %d branches" % MPD_MAX_BRANCHES)
    for m, d in enumerate(delays):
        c.delay[m] = d
    c.min_rows = _whole(64 * c.branches * c.order if min_rows is None else min_rows, "min_rows")
    c.ridge_log2, c.forget_shift = _whole(ridge_log2, "ridge_log2"), _whole(forget_shift, "forget_shift")
    c.full_scale, c.target_gain, c.gain = float(full_scale), float(target_gain), float(gain)
    _raise_rc(lib().mcrx_hip_mpd_selftest(C.addressof(c), None, None, None, None, None, None, 0, None, None, None), "mcrx_hip_mpd_selftest",
              lib().mcrx_hip_mpd_last_error)
    return c


def mpd_constants(cfg):
    """(inv_step, step, e, inv_g0) of an MpdConfig as the library makes them (mcrx_hip_mpd_selftest; host only)."""
    inv_step, step, e, inv_g0 = C.c_float(), C.c_double(), C.c_int(), C.c_float()
    _raise_rc(lib().mcrx_hip_mpd_selftest(C.addressof(cfg), C.byref(inv_step), C.byref(step), C.byref(e), C.byref(inv_g0), None, None, 0, None,
                                          None, None), "mcrx_hip_mpd_selftest", lib().mcrx_hip_mpd_last_error)
    return float(inv_step.value), float(step.value), int(e.value), float(inv_g0.value)


def mpd_integers(cfg, u, z):
    """(Z, U, good) as the measuring kernel makes them of the samples u[i] and z[i]: Z int32 [n, P, 2], the regressors of z[i]; U int32
    [n, 2]; good int32 [n] = 1 (z[i] good) + 2 (u[i] good).  Host only."""
    u, z = np.ascontiguousarray(u, np.complex64), np.ascontiguousarray(z, np.complex64)
    if u.ndim != 1 or u.shape != z.shape:
        raise ValueError("u and z are one-dimensional and equally long")
    n, P = len(u), int(cfg.order)
    Z, U, good = np.zeros((n, P, 2), np.int32), np.zeros((n, 2), np.int32), np.zeros(n, np.int32)
    if n:
        _raise_rc(lib().mcrx_hip_mpd_selftest(C.addressof(cfg), None, None, None, None, u.ctypes.data, z.ctypes.data, n, Z.ctypes.data,
                                              U.ctypes.data, good.ctypes.data), "mcrx_hip_mpd_selftest", lib().mcrx_hip_mpd_last_error)
    return Z, U, good


class mpd(_Predistorter):
    """Predistortion with memory on the wideband stream (mcrx_hip_mpd_*): between cfr and an amplifier that is not memoryless.

        mpd(branches, delays, order=5, table_log2=7, full_scale=, target_gain=, min_rows=None, ridge_log2=30, forget_shift=0, gain=1.0,
            output_format="cf32")

    A diagonal memory polynomial: branch m is a complex gain looked up by the amplitude of the sample delays[m] back (a table of
    2^table_log2 intervals up to `full_scale`) times that sample; the output is the sum of the branches.  The branch gains are
    polynomials of `order` coefficients in the amplitude, learned on the device: measure(u, z) adds what went into the amplifier (u:
    this handle's cf32 output) and what came out (z, aligned by the caller) to exact integer sums, update() solves the least squares
    problem in fp64 and tabulates; set_tables writes tables.  Until the first of either, execute copies.  execute takes lead =
    delays[-1] samples of history in front of the n it returns (pad=True: zeros).  Calls on one handle must be ordered on the device."""

    _op, _pad = "mpd", dict(pad=True)

    def __init__(self, branches=None, delays=None, order=5, table_log2=7, full_scale=None, target_gain=None, min_rows=None, ridge_log2=30,
                 forget_shift=0, gain=1.0, output_format="cf32"):
        c = mpd_config(branches, delays, order, table_log2, full_scale, target_gain, min_rows, ridge_log2, forget_shift, gain, output_format)
        self._create(c)
        self.config, self.output_format, self.K = c, int(c.output_format), 1 << int(c.table_log2)
        self.M, self.P = int(c.branches), int(c.order)
        self.L = self.M * self.P
        self.lead = int(lib().mcrx_hip_mpd_lead(self._h))

    def execute(self, x, out=None, pad=False, stream=None):
        """x: a contiguous complex64 CUDA tensor of lead + n samples, the history in front -- or, with pad=True, n samples, which get
        `lead` zeros in front.  out (optional): where the n samples go, in the output format; it must not overlap x.  Returns the n
        samples written.  Asynchronous on `stream` (default: torch's current stream of x's device)."""
        import torch
        self._in(x, False)
        if pad and self.lead:
            padded = torch.zeros(int(x.numel()) + self.lead, dtype=torch.complex64, device=x.device)
            padded[self.lead:].copy_(x.view(-1))
            x = padded
        n = int(x.numel()) - self.lead
        if n < 0:
            raise ValueError("x must hold the history in front: at least %d samples" % self.lead)
        out, view = self._out(n, out, self.output_format == OUTPUT_FORMATS["sc16"], x.device)
        if n:
            self._call("execute_device", self._h, _dptr(x), n, _dptr(out), self._stream(stream, x))
        return view

    def measure(self, u, z, stream=None):
        """u, z: equally many samples into and out of the amplifier (contiguous complex64 CUDA tensors); the first `lead` are history
        only.  Returns the number of rows offered.  ValueError, nothing measured, where that would take the rows offered since the
        last reset above 2^26."""
        return max(self._measure(u, z, stream) - self.lead, 0)

    def set_tables(self, F, stream=None):
        """Write the tables: finite complex gains F[m, 0 .. K]."""
        self._set("set_tables", F, (self.M, self.K + 1), "tables hold %d x %d", stream)

    def read(self, stream=None):
        """The handle's state as a dict (waits for the handle's work on `stream`): F (complex64 [M, K + 1]), c (complex128 [M, P]), res,
        rows, updates, skipped, degenerate, and the raw sums: sums (int64 [(L + 1)(L + 2) / 2, 2], the upper triangle row by row) and,
        made of them, A (L x L Python-int complex pairs as int64 [L, L, 2], upper triangle), b (int64 [L, 2]), Suu (int)."""
        L = self.L
        ne = (L + 1) * (L + 2) // 2
        s, F, c, sums = MpdState(), np.zeros((self.M, self.K + 1), np.complex64), np.zeros((self.M, self.P), np.complex128), np.zeros((ne, 2), np.int64)
        self._call("read", self._h, C.addressof(s), F.ctypes.data, c.ctypes.data, sums.ctypes.data, self._current(stream))
        A, b, ent = np.zeros((L, L, 2), np.int64), np.zeros((L, 2), np.int64), 0
        for p in range(L + 1):
            for q in range(p, L + 1):
                if q < L:
                    A[p, q] = sums[ent]
                elif p < L:
                    b[p] = sums[ent]
                ent += 1
        return dict(F=F, c=c, res=float(s.res), rows=int(s.rows), updates=int(s.updates), skipped=int(s.skipped), degenerate=int(s.degenerate),
                    sums=sums, A=A, b=b, Suu=int(sums[ne - 1, 0]))


PAMEM_MAX_BRANCHES, PAMEM_MAX_TAPS, PAMEM_MAX_DELAY = 4, 8, 16     # MCRX_PAMEM_MAX_*


class PamemBranch(C.Structure):
    _fields_ = [("sat", C.c_float), ("amp_gain", C.c_float), ("ampm", C.c_float), ("smooth", C.c_uint32), ("taps", C.c_uint32),
                ("delay", C.c_uint32 * PAMEM_MAX_TAPS), ("h_re", C.c_float * PAMEM_MAX_TAPS), ("h_im", C.c_float * PAMEM_MAX_TAPS)]


class PamemConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("branches", C.c_uint32), ("input_format", C.c_uint32), ("output_format", C.c_uint32),
                ("gain", C.c_float), ("branch", PamemBranch * PAMEM_MAX_BRANCHES)]


def pamem_config(branches=None, gain=1.0, input_format="cf32", output_format="cf32"):
    """The mcrx_hip_pamem_config of pamem's arguments.  ValueError for a malformed or missing argument and for every value the library
    refuses (mcrx_hip_pamem_selftest judges them on the host: no device is looked for)."""
    required, optional = ("sat",), dict(smooth=2, gain=1.0, ampm_deg=0.0, taps=((0, 1.0),))
    if not isinstance(branches, (list, tuple)) or not 1 <= len(branches) <= PAMEM_MAX_BRANCHES:
        raise ValueError("branches: a list of 1 .. %d dicts" % PAMEM_MAX_BRANCHES)
    c = PamemConfig()
    c.struct_size, c.branches, c.gain = C.sizeof(PamemConfig), len(branches), float(gain)
    c.input_format = _format_code(input_format, INPUT_FORMATS, "input_format")
    c.output_format = _format_code(output_format, OUTPUT_FORMATS, "output_format")
    for b, d in enumerate(branches):
        if not isinstance(d, dict) or any(k not in required and k not in optional for k in d) or any(k not in d for k in required):
            raise ValueError("a branch is a dict with %s and optionally %s" % (required, tuple(optional)))
        d, br = dict(optional, **d), c.branch[b]
        br.sat, br.amp_gain, br.ampm, br.smooth = float(d["sat"]), float(d["gain"]), float(d["ampm_deg"]) / 360.0, _whole(d["smooth"], "smooth")
        taps = list(d["taps"]) if isinstance(d["taps"], (list, tuple)) else None
        if taps is None or not 1 <= len(taps) <= PAMEM_MAX_TAPS or any(not isinstance(t, (list, tuple)) or len(t) != 2 for t in taps):
            raise ValueError("taps: 1 .. %d pairs (delay, weight)" % PAMEM_MAX_TAPS)
        br.taps = len(taps)
        for k, (delay, weight) in enumerate(taps):
            br.delay[k], weight = _whole(delay, "a delay"), complex(weight)
            br.h_re[k], br.h_im[k] = weight.real, weight.imag
    _raise_rc(lib().mcrx_hip_pamem_selftest(C.addressof(c), None, None, None, None, None, None), "mcrx_hip_pamem_selftest",
              lib().mcrx_hip_pamem_last_error)
    return c


def pamem_constants(cfg):
    """(lead, [r_b], [(branch, delay, weight), ...]) of a PamemConfig as the library makes them: r_b = fp32(1 / sat_b^2) and the taps in
    the order the sum runs (mcrx_hip_pamem_selftest; host only)."""
    most = PAMEM_MAX_BRANCHES * PAMEM_MAX_TAPS
    lead, count, r = C.c_uint32(), C.c_uint32(), (C.c_float * PAMEM_MAX_BRANCHES)()
    tb, td, th = (C.c_uint32 * most)(), (C.c_uint32 * most)(), (C.c_float * (2 * most))()
    _raise_rc(lib().mcrx_hip_pamem_selftest(C.addressof(cfg), C.byref(lead), r, C.byref(count), tb, td, th), "mcrx_hip_pamem_selftest",
              lib().mcrx_hip_pamem_last_error)
    return (int(lead.value), [float(v) for v in r[:int(cfg.branches)]],
            [(int(tb[i]), int(td[i]), complex(th[2 * i], th[2 * i + 1])) for i in range(int(count.value))])


def pamem_small_signal(branches):
    """The complex taps H[0 .. lead] of the linear regime of pamem(branches), float64 on the host: H[d] = the sum over the taps (b, k)
    at delay d of gain_b * h_{b,k}, with the fp32 values the handle holds.  Far below saturation the operator is this FIR (times its
    gain); its group delay is what fbalign counts as the path's."""
    c = pamem_config(branches)
    lead, _, taps = pamem_constants(c)
    H = np.zeros(lead + 1, np.complex128)
    for b, d, h in taps:
        H[d] += float(c.branch[b].amp_gain) * h
    return H


class pamem(_StreamOp):
    """Amplifier with memory on the wideband stream (mcrx_hip_pamem_*): a parallel Hammerstein model, the amplifier mpd straightens.

        pamem(branches=[dict(sat, smooth=2, gain=1.0, ampm_deg=0.0, taps=[(delay, weight), ...]), ...], gain=1.0,
              input_format="cf32", output_format="cf32")

    1 .. 4 branches, each rfchain's amplifier (Rapp AM/AM of smoothness 1, 2 or 4 that saturates at `sat`, AM/PM that tends to ampm_deg)
    behind it 1 .. 8 taps: delays 0 .. 16, strictly increasing, complex weights.  y[i] = gain * sum_b sum_k h_bk A_b(u[i - d_bk]).
    Stateless and time-invariant; lead = the largest delay.  sc16 tensors are contiguous int16 of shape (n, 2).  A pamem is directly
    the `amplifier` of dpd.learn / mpd.learn."""

    _op, _what = "pamem", ("this amplifier", "amplifier")

    def __init__(self, branches=None, gain=1.0, input_format="cf32", output_format="cf32"):
        c = pamem_config(branches, gain, input_format, output_format)
        self._create(c)
        self.config, self.input_format, self.output_format = c, int(c.input_format), int(c.output_format)
        self.lead = int(lib().mcrx_hip_pamem_lead(self._h))

    def execute(self, x, first_sample=0, out=None, pad=True, stream=None):
        """x: n samples, which get `lead` zeros in front (pad=True, the default: as many samples out as in) -- or, with pad=False,
        lead + n samples, the history in front.  A contiguous CUDA tensor: complex64, or on an sc16-in handle int16 of shape (n, 2).
        first_sample is accepted and ignored: the operator does not depend on position.  out (optional): where the n samples go, in
        the output format; it must not overlap x.  Returns the n samples written.  Asynchronous on `stream` (default: torch's current
        stream of x's device)."""
        import torch
        in16 = self.input_format == INPUT_FORMATS["sc16"]
        m = self._in(x, in16)
        if pad and self.lead:
            padded = torch.zeros((m + self.lead, 2), dtype=torch.int16, device=x.device) if in16 else \
                torch.zeros(m + self.lead, dtype=torch.complex64, device=x.device)
            padded[self.lead:].copy_(x.view(-1, 2) if in16 else x.view(-1))
            x = padded
        n = (m if pad else m - self.lead)
        if n < 0:
            raise ValueError("x must hold the history in front: at least %d samples" % self.lead)
        out, view = self._out(n, out, self.output_format == OUTPUT_FORMATS["sc16"], x.device)
        if n:
            self._call("execute_device", self._h, _dptr(x), n, _dptr(out), self._stream(stream, x))
        return view


FBALIGN_MIN_LAG, FBALIGN_MAX_LAG, FBALIGN_H, FBALIGN_TAPS, FBALIGN_GUARD_LOG2, FBALIGN_MAX_WGS = 8, 64, 8, 32, 31, 256


class FbalignConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_lag", C.c_uint32), ("full_scale", C.c_float), ("target_gain", C.c_float),
                ("min_rows", C.c_uint32), ("input_format", C.c_uint32)]


class FbalignState(C.Structure):
    _fields_ = [("tau_fp", C.c_int64), ("s_re", C.c_double), ("s_im", C.c_double), ("res", C.c_double), ("updates", C.c_uint64),
                ("degenerate", C.c_uint64), ("clamped", C.c_uint64), ("rows", C.c_int64), ("offered", C.c_uint64)]


def fbalign_config(max_lag=32, full_scale=None, target_gain=None, min_rows=1024, input_format="cf32"):
    """The mcrx_hip_fbalign_config of fbalign's arguments.  ValueError for a malformed or missing argument and for every value the
    library refuses (mcrx_hip_fbalign_selftest judges them on the host: no device is looked for)."""
    if full_scale is None or target_gain is None:
        raise ValueError("full_scale and target_gain must be given")
    c = FbalignConfig()
    c.struct_size = C.sizeof(FbalignConfig)
    c.input_format = _format_code(input_format, INPUT_FORMATS, "input_format")
    c.max_lag, c.min_rows = _whole(max_lag, "max_lag"), _whole(min_rows, "min_rows")
    c.full_scale, c.target_gain = float(full_scale), float(target_gain)
    _raise_rc(lib().mcrx_hip_fbalign_selftest(C.addressof(c), None, None, None, 0, None, None, 0, None, None), "mcrx_hip_fbalign_selftest",
              lib().mcrx_hip_fbalign_last_error)
    return c


def fbalign_constants(cfg):
    """(e, taps) of an FbalignConfig as the library makes them: the exponent of the least power of two that is at least full_scale and
    the differentiator's h_1 .. h_8 (float32 array).  Host only."""
    e, taps = C.c_int(), np.zeros(FBALIGN_H, np.float32)
    _raise_rc(lib().mcrx_hip_fbalign_selftest(C.addressof(cfg), C.byref(e), taps.ctypes.data, None, 0, None, None, 0, None, None),
              "mcrx_hip_fbalign_selftest", lib().mcrx_hip_fbalign_last_error)
    return int(e.value), taps


def fbalign_q15(cfg, v):
    """(q15, bad) as the measuring kernel makes them of the float32 components v: int32 arrays.  Host only."""
    v = np.ascontiguousarray(v, np.float32).reshape(-1)
    q, bad = np.zeros(len(v), np.int32), np.zeros(len(v), np.int32)
    if len(v):
        _raise_rc(lib().mcrx_hip_fbalign_selftest(C.addressof(cfg), None, None, v.ctypes.data, len(v), q.ctypes.data, bad.ctypes.data, 0, None, None),
                  "mcrx_hip_fbalign_selftest", lib().mcrx_hip_fbalign_last_error)
    return q, bad


def fbalign_coefficients(cfg, tau_fp):
    """(c, nd): the 32 fp32 coefficients and the whole-sample offset apply uses at the delay tau_fp (Q32 samples).  Host only."""
    c, nd = np.zeros(FBALIGN_TAPS, np.float32), C.c_int()
    _raise_rc(lib().mcrx_hip_fbalign_selftest(C.addressof(cfg), None, None, None, 0, None, None, int(tau_fp), c.ctypes.data, C.byref(nd)),
              "mcrx_hip_fbalign_selftest", lib().mcrx_hip_fbalign_last_error)
    return c, int(nd.value)


class fbalign(_StreamOp):
    """Feedback alignment for the predistorters (mcrx_hip_fbalign_*): between an observation receiver and dpd.measure / mpd.measure.

        fbalign(max_lag=32, full_scale=, target_gain=, min_rows=1024, input_format="cf32")

    The receiver returns the amplifier's output late by up to max_lag samples and a fraction, at its own gain and phase, as cf32 or
    sc16.  execute(z) delays the capture by -tau through a 32-tap interpolator and scales it by s; measure(u, zh) correlates the
    amplifier's input with the aligned capture into exact integer sums; update() moves tau and s by one Gauss-Newton step on the
    device; set writes a known path.  Until the first update or set, execute copies.  Stateless in the samples and non-causal:
    execute takes n + 2 halo samples and returns the n in the middle.  The aligner counts the amplifier's own group delay as the
    path's.  Calls on one handle must be ordered on the device."""

    _op, _what = "fbalign", ("this aligner", "aligner")

    def __init__(self, max_lag=32, full_scale=None, target_gain=None, min_rows=1024, input_format="cf32"):
        c = fbalign_config(max_lag, full_scale, target_gain, min_rows, input_format)
        self._create(c)
        self.config, self.input_format, self.output_format, self.max_lag = c, int(c.input_format), OUTPUT_FORMATS["cf32"], int(c.max_lag)
        self.R = self.max_lag + FBALIGN_H
        self.halo = int(lib().mcrx_hip_fbalign_halo(self._h))

    def execute(self, z, out=None, pad=False, stream=None):
        """z: a contiguous CUDA tensor of n + 2 halo capture samples (complex64, or on an sc16-in handle int16 of shape (n, 2)) -- or,
        with pad=True, n samples, which get `halo` zeros on either side.  out (optional): where the n complex64 samples go; it must not
        overlap z.  Returns the n samples written.  Asynchronous on `stream` (default: torch's current stream of z's device)."""
        import torch
        in16 = self.input_format == INPUT_FORMATS["sc16"]
        m = self._in(z, in16)
        if pad:
            padded = torch.zeros((m + 2 * self.halo, 2), dtype=torch.int16, device=z.device) if in16 else \
                torch.zeros(m + 2 * self.halo, dtype=torch.complex64, device=z.device)
            padded[self.halo:self.halo + m].copy_(z.view(-1, 2) if in16 else z.view(-1))
            z, m = padded, m + 2 * self.halo
        n = m - 2 * self.halo
        if n < 0:
            raise ValueError("z must hold the halo on either side: at least %d samples" % (2 * self.halo))
        out, view = self._out(n, out, False, z.device)
        if n:
            self._call("execute_device", self._h, _dptr(z), n, _dptr(out), self._stream(stream, z))
        return view

    def measure(self, u, zh, stream=None):
        """u, zh: equally many complex64 samples -- the amplifier's input and the aligned capture that execute wrote.  Returns the
        number of rows offered (the first and last R = max_lag + 8 samples are no rows).  ValueError, nothing measured, where that
        would take the rows offered since the last update or reset above 2^31."""
        n = self._in(u, False)
        if self._in(zh, False) != n:
            raise ValueError("u and zh must hold equally many samples")
        if n:
            self._call("measure_device", self._h, _dptr(u), _dptr(zh), n, self._stream(stream, u))
        return max(n - 2 * self.R, 0)

    def update(self, stream=None):
        """Move tau and s by what has been measured (on the device, no synchronisation) and clear the sums."""
        self._call("update", self._h, self._current(stream))

    def set(self, tau_fp, s=1.0, stream=None):
        """Write a known path: tau_fp (an integer, Q32 samples: the capture lags u by tau_fp / 2^32) and the complex scale s."""
        s = complex(s)
        if isinstance(tau_fp, bool) or int(tau_fp) != tau_fp or abs(int(tau_fp)) >= 1 << 63:
            raise ValueError("tau_fp is an integer in Q32 samples")
        self._call("set", self._h, int(tau_fp), s.real, s.imag, self._current(stream))

    def clipped(self, reset=False):
        """0: the output is cf32 (samples that clamp in measure are read()'s `clamped`)."""
        return 0

    def reset(self):
        """tau = 0, s = 1, sums and counters cleared; execute copies again (no synchronisation)."""
        self._call("reset", self._h)

    def read(self, stream=None):
        """The handle's state as a dict (waits for the handle's work on `stream`): tau_fp (int), tau (float samples), s (complex), res,
        rows, updates, degenerate, clamped, offered (the guard's count of rows since the last update or reset), coef (float32 [32]), scale (the fp32 s as complex), nd, and the sums as int64 arrays of
        (re, im): C [2 R + 1, 2] (lags -R .. R), A [17, 2], and Szz (int)."""
        ns = 2 * self.R + 19
        s, coef, sums = FbalignState(), np.zeros(FBALIGN_TAPS + 3, np.float32), np.zeros((ns, 2), np.int64)
        self._call("read", self._h, C.addressof(s), coef.ctypes.data, sums.ctypes.data, self._current(stream))
        return dict(tau_fp=int(s.tau_fp), tau=float(s.tau_fp) * 2.0 ** -32, s=complex(s.s_re, s.s_im), res=float(s.res), rows=int(s.rows),
                    updates=int(s.updates), degenerate=int(s.degenerate), clamped=int(s.clamped), offered=int(s.offered), coef=coef[:FBALIGN_TAPS].copy(),
                    scale=complex(coef[FBALIGN_TAPS], coef[FBALIGN_TAPS + 1]), nd=int(coef[FBALIGN_TAPS + 2]), C=sums[:2 * self.R + 1].copy(),
                    A=sums[2 * self.R + 1:ns - 1].copy(), Szz=int(sums[ns - 1, 0]), sums=sums)

    def align(self, u, z, rounds=3, stream=None):
        """u: n complex64 samples into the amplifier; z: the n capture samples the receiver returned for them, in the input format.
        `rounds` times execute(z) -> measure -> update, then execute once more.  Returns (u[halo : n - halo], the aligned capture):
        n - 2 halo samples each, ready for dpd.measure or mpd.measure."""
        in16 = self.input_format == INPUT_FORMATS["sc16"]
        n = self._in(u, False)
        if self._in(z, in16) != n:
            raise ValueError("u and z must hold equally many samples")
        if n < 2 * self.halo:
            raise ValueError("u and z must hold the halo on either side: at least %d samples" % (2 * self.halo))
        ut = u.view(-1)[self.halo:n - self.halo]
        for _ in range(int(rounds)):
            self.measure(ut, self.execute(z, stream=stream), stream=stream)
            self.update(stream=stream)
        return ut, self.execute(z, stream=stream)


USERCHAN_MAX_RAYS, USERCHAN_MAX_DELAY, USERCHAN_MAX_CHANNELS = 4, 255, 1024      # MCRX_USERCHAN_MAX_RAYS, _MAX_DELAY, _MAX_CHANNELS
USERCHAN_SYNTH_LEAD = 32      # blocks of filter history userchan.generate gives the synthesis bank: >= 25, a multiple of 8


class UserchanChannel(C.Structure):
    _fields_ = [("num_rays", C.c_uint32), ("delay", C.c_uint32 * USERCHAN_MAX_RAYS),
                ("tap_re", C.c_float * USERCHAN_MAX_RAYS), ("tap_im", C.c_float * USERCHAN_MAX_RAYS),
                ("gain", C.c_float), ("cfo_step", C.c_uint32), ("phase0", C.c_uint32)]


_USERCHAN_KEYS = ("taps", "gain_db", "cfo_step", "phase0", "delay")


def userchan_cfo_step(spacings, M):
    """The userchan cfo_step (2^32 * cycles per channel-rate sample, mod 2^32) of a user's oscillator that is off by `spacings`
    subcarrier spacings: a spacing is 1 / M cycles per channel-rate sample."""
    return int(round(float(spacings) / M * 4294967296.0)) % (1 << 32)


def userchan_channel(taps=((0, 1.0),), gain_db=0.0, cfo_step=0, phase0=0, delay=0):
    """The mcrx_hip_userchan_channel structure of one user: rays (delay, a) in channel-rate samples, summed in the order given; `delay`
    (the user's timing offset) is added to every ray's; gain = float32(10 ** (gain_db / 20)).  ValueError for what the library refuses."""
    taps = list(taps)
    if not 1 <= len(taps) <= USERCHAN_MAX_RAYS:
        raise ValueError("1 .. %d rays a channel" % USERCHAN_MAX_RAYS)
    if int(delay) != delay or int(delay) < 0:
        raise ValueError("a timing offset is a whole number of channel-rate samples, not negative")
    u = UserchanChannel()
    u.num_rays = len(taps)
    for i, (d, a) in enumerate(taps):
        if int(d) != d or not 0 <= int(d) + int(delay) <= USERCHAN_MAX_DELAY:
            raise ValueError("a delay (with the timing offset) is a whole number of channel-rate samples, 0 .. %d" % USERCHAN_MAX_DELAY)
        a = np.complex64(complex(a))
        if not (np.isfinite(a.real) and np.isfinite(a.imag)):
            raise ValueError("taps must be finite")
        u.delay[i], u.tap_re[i], u.tap_im[i] = int(d) + int(delay), float(a.real), float(a.imag)
    try:
        with np.errstate(over="ignore"):
            gain = np.float32(10.0 ** (float(gain_db) / 20.0))
    except OverflowError:
        gain = np.float32("inf")
    if not np.isfinite(gain):
        raise ValueError("gain_db must be finite and its gain must fit fp32")
    u.gain, u.cfo_step, u.phase0 = float(gain), int(cfo_step) % (1 << 32), int(phase0) % (1 << 32)
    return u


USERFADE_MIN_LOG2_BLOCK, USERFADE_MAX_LOG2_BLOCK = 3, 20      # MCRX_USERFADE_MIN_LOG2_BLOCK, _MAX_LOG2_BLOCK


class UserfadeUser(C.Structure):
    _fields_ = [("enabled", C.c_uint32), ("id", C.c_uint32), ("doppler", C.c_double * USERCHAN_MAX_RAYS),
                ("los_doppler", C.c_double * USERCHAN_MAX_RAYS), ("rice_k", C.c_float * USERCHAN_MAX_RAYS),
                ("los_phase", C.c_uint32 * USERCHAN_MAX_RAYS)]


class UserfadeConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("user_struct_size", C.c_uint32), ("log2_block", C.c_uint32), ("num_sinusoids", C.c_uint32),
                ("table_rows", C.c_uint32), ("reserved", C.c_uint32), ("seed", C.c_uint64)]


_USERFADE_KEYS = ("log2_block", "sinusoids", "seed", "table_rows", "users")
_USERFADE_USER_KEYS = ("doppler", "rice_k", "los_doppler", "los_phase", "id")


def userchan_doppler(cycles_per_ofdm_symbol, M, cp):
    """The userchan Doppler (cycles per channel-rate sample) of a gain that turns `cycles_per_ofdm_symbol` cycles in one OFDM symbol
    of M + cp channel-rate samples."""
    return float(cycles_per_ofdm_symbol) / (M + cp)


def userfade_user(num_rays, log2_block, index, doppler, rice_k=0.0, los_doppler=0.0, los_phase=0, id=None):
    """The mcrx_hip_userfade_user structure of one fading user with `num_rays` rays: per-ray entries are scalars (every ray gets them) or
    sequences of num_rays values; id defaults to `index`, the user's place in the table.  ValueError for what the library refuses."""
    def per_ray(v, name, conv):
        vals = [conv(x) for x in v] if hasattr(v, "__len__") else [conv(v)] * num_rays
        if len(vals) != num_rays:
            raise ValueError("fading: %s has %d entries for %d rays" % (name, len(vals), num_rays))
        return vals
    u = UserfadeUser()
    uid = index if id is None else id
    if int(uid) != uid or not 0 <= int(uid) < (1 << 32):
        raise ValueError("fading: a user's id is a whole number, 0 .. 2^32 - 1")
    u.enabled, u.id = 1, int(uid)
    B = float(1 << int(log2_block))
    fd, fl = per_ray(doppler, "doppler", float), per_ray(los_doppler, "los_doppler", float)
    rk, ph = per_ray(rice_k, "rice_k", float), per_ray(los_phase, "los_phase", int)
    for i in range(num_rays):
        if not (math.isfinite(fd[i]) and math.isfinite(fl[i])):
            raise ValueError("fading: a Doppler is not finite")
        if fd[i] < 0.0 or fd[i] * B > 0.125 or abs(fl[i]) * B > 0.125:
            raise ValueError("fading: 0 <= doppler and doppler * 2^log2_block <= 1/8 (|los_doppler| likewise): the grid must sample the gain")
        if not (math.isfinite(rk[i]) and rk[i] >= 0.0 and math.isfinite(C.c_float(rk[i]).value)):
            raise ValueError("fading: rice_k must be finite and not negative")
        u.doppler[i], u.los_doppler[i], u.rice_k[i], u.los_phase[i] = fd[i], fl[i], rk[i], ph[i] % (1 << 32)
    return u


def userchan_fading(rays, log2_block=4, sinusoids=16, seed=0, table_rows=0, users=None):
    """(mcrx_hip_userfade_config, mcrx_hip_userfade_user[len(rays)]) of a fading description for channels with rays[c] rays each:
    users[c] is None (that user does not fade), a dict(doppler, rice_k=0, los_doppler=0, los_phase=0, id=None) or a UserfadeUser."""
    for v, name, lo, hi in ((log2_block, "log2_block", USERFADE_MIN_LOG2_BLOCK, USERFADE_MAX_LOG2_BLOCK),
                            (sinusoids, "sinusoids", 1, CHANEMU_MAX_SINUSOIDS)):
        if int(v) != v or not lo <= int(v) <= hi:
            raise ValueError("fading: %s must be %d .. %d" % (name, lo, hi))
    if int(table_rows) != table_rows or int(table_rows) == 1 or not 0 <= int(table_rows) < (1 << 32):
        raise ValueError("fading: table_rows must be 0 (default) or 2 .. 2^32 - 1")
    users = list(users) if users is not None else []
    if len(users) != len(rays):
        raise ValueError("fading: users has %d entries for %d channels" % (len(users), len(rays)))
    f = UserfadeConfig()
    f.struct_size, f.user_struct_size = C.sizeof(UserfadeConfig), C.sizeof(UserfadeUser)
    f.log2_block, f.num_sinusoids, f.table_rows, f.seed = int(log2_block), int(sinusoids), int(table_rows), int(seed) % (1 << 64)
    table = (UserfadeUser * len(rays))()
    for c, u in enumerate(users):
        if u is None:
            table[c].id = c
        elif isinstance(u, UserfadeUser):
            table[c] = u
        elif isinstance(u, dict) and "doppler" in u and all(k in _USERFADE_USER_KEYS for k in u):
            table[c] = userfade_user(rays[c], f.log2_block, c, **u)
        else:
            raise ValueError("fading: a user is None or a dict with 'doppler' and keys of %s" % (_USERFADE_USER_KEYS,))
    return f, table


USERCLOCK_TAPS, USERCLOCK_PHASES, USERCLOCK_MIN_DELAY, USERCLOCK_MAX_DELAY = 32, 64, 15, 255     # MCRX_USERCLOCK_*
USERCLOCK_MAX_SCO = 1 << 38       # |sco|, 2^-48 samples per sample: about 977 ppm


class UserclockUser(C.Structure):
    _fields_ = [("enabled", C.c_uint32), ("reserved", C.c_uint32), ("delay_fp", C.c_uint64), ("sco", C.c_int64), ("origin", C.c_int64)]


class UserclockConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("user_struct_size", C.c_uint32), ("max_delay", C.c_uint32), ("span_blocks", C.c_uint32)]


_USERCLOCK_KEYS = ("max_delay", "span_blocks", "users")
_USERCLOCK_USER_KEYS = ("delay", "ppm", "origin")


def userclock_user(max_delay, delay, ppm=0.0, origin=0):
    """The mcrx_hip_userclock_user structure of one user with a clock of their own: delay_fp = rint(delay * 2^32) (delay in channel-rate
    samples at block `origin`, its whole part 15 .. max_delay), sco = rint(ppm * 1e-6 * 2^48).  ValueError for what the library refuses."""
    delay, ppm = float(delay), float(ppm)
    if not (math.isfinite(delay) and math.isfinite(ppm)):
        raise ValueError("clock: delay and ppm must be finite")
    dfp, sco = int(np.rint(delay * 4294967296.0)), int(np.rint(ppm * 1e-6 * 281474976710656.0))
    if not USERCLOCK_MIN_DELAY <= (dfp >> 32) <= int(max_delay):
        raise ValueError("clock: the whole samples of a delay are %d .. max_delay (%d)" % (USERCLOCK_MIN_DELAY, int(max_delay)))
    if abs(sco) > USERCLOCK_MAX_SCO:
        raise ValueError("clock: |ppm| is at most 2^38 * 2^-48 * 1e6, about 976.56")
    if int(origin) != origin or not -(1 << 63) <= int(origin) < (1 << 63):
        raise ValueError("clock: origin is a signed 64-bit block index")
    u = UserclockUser()
    u.enabled, u.delay_fp, u.sco, u.origin = 1, dfp, sco, int(origin)
    return u


def userchan_clock(num_channels, max_delay=64, span_blocks=0, users=None):
    """(mcrx_hip_userclock_config, mcrx_hip_userclock_user[num_channels]) of a clock description: users[c] is None (that user keeps the
    receiver's clock: z = x), a dict(delay, ppm=0.0, origin=0) or a UserclockUser."""
    if int(max_delay) != max_delay or not USERCLOCK_MIN_DELAY <= int(max_delay) <= USERCLOCK_MAX_DELAY:
        raise ValueError("clock: max_delay must be %d .. %d" % (USERCLOCK_MIN_DELAY, USERCLOCK_MAX_DELAY))
    if int(span_blocks) != span_blocks or int(span_blocks) % 8 or not 0 <= int(span_blocks) < (1 << 32):
        raise ValueError("clock: span_blocks must be 0 (default) or a multiple of 8 below 2^32")
    users = list(users) if users is not None else []
    if len(users) != num_channels:
        raise ValueError("clock: users has %d entries for %d channels" % (len(users), num_channels))
    f = UserclockConfig()
    f.struct_size, f.user_struct_size = C.sizeof(UserclockConfig), C.sizeof(UserclockUser)
    f.max_delay, f.span_blocks = int(max_delay), int(span_blocks)
    table = (UserclockUser * num_channels)()
    for c, u in enumerate(users):
        if u is None:
            continue
        if isinstance(u, UserclockUser):
            table[c] = u
        elif isinstance(u, dict) and "delay" in u and all(k in _USERCLOCK_USER_KEYS for k in u):
            table[c] = userclock_user(f.max_delay, **u)
        else:
            raise ValueError("clock: a user is None or a dict with 'delay' and keys of %s" % (_USERCLOCK_USER_KEYS,))
    return f, table


class userchan(object):
    """Per-user channel emulator on the transmitter's channel tiles, between TxTraffic.tiles and multichanneltx.synthesize
    (mcrx_hip_userchan_*): every channel has its own multipath, oscillator, timing and level, at the channel rate.

        userchan(channels=[dict(taps=[(delay, a), ...], gain_db=0.0, cfo_step=0, phase0=0, delay=0), ...])

    One entry per local channel (1 .. 1024): 1 .. 4 rays with delays in channel-rate samples (<= 255 with the timing offset `delay`
    added), cfo_step / phase0 32-bit phases per channel-rate sample (userchan_cfo_step).  The operator keeps no state: apply() is a
    function of the absolute block index and of the tiles it is handed, which include `lead_blocks` blocks in front of the output's
    first.  When no channel has a step or a start phase the rotation is not computed; otherwise every channel is rotated.

    fading=dict(log2_block=4, sinusoids=16, seed=0, table_rows=0, users=[None | dict(doppler, rice_k=0, los_doppler=0, los_phase=0,
    id=None), ...]) makes the rays of the users named Rayleigh (rice_k = 0) or Rician fading ones (mcrx_hip_userfade_*): one entry per
    channel, None for a user who does not fade; Dopplers in cycles per channel-rate sample (userchan_doppler), each of doppler, rice_k,
    los_doppler, los_phase one value or one per ray; the gains are updated every 2^log2_block blocks (3 .. 20) and interpolated
    linearly between.  A user's gains follow from the seed and their id (default: their index), which shard() keeps.  Calls on a
    fading handle share its gain table: keep them ordered on the device (one stream, or events).

    clock=dict(max_delay=64, span_blocks=0, users=[None | dict(delay=16.25, ppm=20.0, origin=0), ...]) gives the users named a sample
    clock and a fractional timing of their own (mcrx_hip_userclock_*), in front of their multipath: they transmit x(b - tau(b)) with
    tau = delay + ppm 1e-6 (b - origin) channel-rate samples, interpolated by 32 taps; the whole samples of tau must stay within
    15 .. max_delay on every block of a call (a call that leaves the range is refused), and lead_blocks grows by max_delay + 16.
    None for a user on the receiver's clock.  Calls on a clocked handle share its scratch buffer: keep them ordered on the device."""

    def __init__(self, channels, fading=None, clock=None):
        self._h = C.c_void_p()
        self._fading = None
        self._clock = None
        chans = []
        for ch in channels:
            if isinstance(ch, UserchanChannel):
                chans.append(ch)
                continue
            if not isinstance(ch, dict) or any(k not in _USERCHAN_KEYS for k in ch):
                raise ValueError("a channel is a dict with keys of %s" % (_USERCHAN_KEYS,))
            chans.append(userchan_channel(**ch))
        if not 1 <= len(chans) <= USERCHAN_MAX_CHANNELS:
            raise ValueError("1 .. %d channels a handle" % USERCHAN_MAX_CHANNELS)
        self._table = (UserchanChannel * len(chans))(*chans)
        fading = self._fading_structs(fading)
        clock = self._clock_structs(clock)
        rc = lib().mcrx_hip_userchan_create(C.byref(self._h), len(chans), C.addressof(self._table), C.sizeof(UserchanChannel))
        if rc != MCRX_OK:
            self._h = C.c_void_p()
            self._chk(rc, "mcrx_hip_userchan_create")
        if fading is not None:
            self._set_fading(fading)
        if clock is not None:
            self._set_clock(clock)

    @staticmethod
    def _chk(rc, name):
        _raise_rc(rc, name, lib().mcrx_hip_userchan_last_error)

    def _fading_structs(self, fading):
        if fading is None:
            return None
        if not isinstance(fading, dict) or any(k not in _USERFADE_KEYS for k in fading):
            raise ValueError("fading is None or a dict with keys of %s" % (_USERFADE_KEYS,))
        return userchan_fading([int(u.num_rays) for u in self._table], **fading)

    def _set_fading(self, structs):
        if structs is None:
            self._chk(lib().mcrx_hip_userfade_set(self._h, None, None), "mcrx_hip_userfade_set")
        else:
            self._chk(lib().mcrx_hip_userfade_set(self._h, C.addressof(structs[0]), C.addressof(structs[1])), "mcrx_hip_userfade_set")
        self._fading = structs

    def set_fading(self, fading):
        """None: fading off (the emulator of constant rays, the present kernels); a dict as at construction: fading on with these
        parameters.  Waits for the device before the handle's tables change."""
        self._set_fading(self._fading_structs(fading))

    def fading_on(self):
        return bool(lib().mcrx_hip_userfade_on(self._h))

    def _clock_structs(self, clock):
        if clock is None:
            return None
        if not isinstance(clock, dict) or any(k not in _USERCLOCK_KEYS for k in clock):
            raise ValueError("clock is None or a dict with keys of %s" % (_USERCLOCK_KEYS,))
        return userchan_clock(len(self._table), **clock)

    def _set_clock(self, structs):
        if structs is None:
            self._chk(lib().mcrx_hip_userclock_set(self._h, None, None), "mcrx_hip_userclock_set")
        else:
            self._chk(lib().mcrx_hip_userclock_set(self._h, C.addressof(structs[0]), C.addressof(structs[1])), "mcrx_hip_userclock_set")
        self._clock = structs

    def set_clock(self, clock):
        """None: every user on the receiver's clock again (the present kernels, the present lead); a dict as at construction: these
        clocks.  Waits for the device before the handle's tables change."""
        self._set_clock(self._clock_structs(clock))

    def clock_on(self):
        return bool(lib().mcrx_hip_userclock_on(self._h))

    @property
    def clock_lead_blocks(self):
        """blocks resample() needs in front of its output's first: max_delay + 16 rounded up to 8 (0 with the clock off)"""
        return int(lib().mcrx_hip_userclock_lead_blocks(self._h))

    def resample(self, tiles, first_block, nblocks, lead_blocks=None, out=None, stream=None):
        """The clock stage alone: z of blocks [first_block, first_block + nblocks) -- what the users transmit, in front of their rays --
        from tiles as apply() takes them, with lead_blocks (default: clock_lead_blocks) blocks in front.  For tests and measurements."""
        return self._on_tiles(lib().mcrx_hip_userclock_apply_tiles, "mcrx_hip_userclock_apply_tiles",
                              self.clock_lead_blocks if lead_blocks is None else int(lead_blocks), tiles, first_block, nblocks, out, stream)

    def gains(self, first_row, rows, stream=None):
        """The gain table's rows first_row .. first_row + rows - 1 (grid row = block >> log2_block, signed) as a complex64 CUDA tensor
        [rows, num_channels, 4]: what apply() interpolates between; entries of rays a channel does not have, and of users who do not
        fade, are 1.  For tests and measurements."""
        import torch
        out = torch.zeros((int(rows), len(self._table), USERCHAN_MAX_RAYS), dtype=torch.complex64, device="cuda")
        if stream is None:
            stream = torch.cuda.current_stream(out.device)
        self._chk(lib().mcrx_hip_userfade_gains(self._h, int(first_row), int(rows), _dptr(out), _stream_ptr(stream)),
                  "mcrx_hip_userfade_gains")
        return out

    @property
    def num_channels(self):
        return int(lib().mcrx_hip_userchan_num_channels(self._h))

    @property
    def lead_blocks(self):
        """blocks apply() needs in front of its output's first: the largest delay rounded up to 8; with a clock on the largest delay +
        max_delay + 16, rounded up to 8"""
        return int(lib().mcrx_hip_userchan_lead_blocks(self._h))

    def shard(self, first, count):
        """A new handle for local channels [first, first + count): what a channel shard of the transmitter (TxTraffic) applies."""
        if int(first) != first or int(count) != count or not (0 <= first and 1 <= count and first + count <= len(self._table)):
            raise ValueError("a shard is channels [first, first + count) of this handle's %d" % len(self._table))
        sel = range(int(first), int(first) + int(count))
        fading = None
        if self._fading is not None:          # the users keep their ids, and with them their gains
            f, users = self._fading
            fading = dict(log2_block=f.log2_block, sinusoids=f.num_sinusoids, seed=f.seed, table_rows=f.table_rows,
                          users=[users[c] for c in sel])
        clock = None
        if self._clock is not None:           # ... and their clocks
            f, users = self._clock
            clock = dict(max_delay=f.max_delay, span_blocks=f.span_blocks, users=[users[c] for c in sel])
        return userchan([self._table[c] for c in sel], fading=fading, clock=clock)

    def apply(self, tiles, first_block, nblocks, lead_blocks=None, out=None, stream=None):
        """tiles: granules [tile][channel][8] of blocks [first_block - lead_blocks, first_block + nblocks), a contiguous torch complex64
        CUDA tensor (TxTraffic.tiles' layout for this handle's channels); lead_blocks defaults to the handle's.  Returns the granules
        of blocks [first_block, first_block + nblocks) -- in `out` when given, which must not overlap `tiles`.  Asynchronous on
        `stream` (default: torch's current stream of the tiles' device)."""
        return self._on_tiles(lib().mcrx_hip_userchan_apply_tiles, "mcrx_hip_userchan_apply_tiles",
                              self.lead_blocks if lead_blocks is None else int(lead_blocks), tiles, first_block, nblocks, out, stream)

    def _on_tiles(self, fn, name, lead, tiles, first_block, nblocks, out, stream):
        import torch
        C_ = len(self._table)
        nblocks = int(nblocks)
        if nblocks < 0 or lead < 0:
            raise ValueError("block counts are not negative")
        for t, need, what in ((tiles, (lead + nblocks) * C_, "tiles"), (out, nblocks * C_, "out")):
            if t is None:
                continue
            if t.dtype != torch.complex64:
                raise TypeError("%s must be complex64, not %s" % (what, t.dtype))
            if not t.is_cuda or not t.is_contiguous() or int(t.numel()) < need:
                raise ValueError("%s must be a contiguous CUDA tensor of at least %d samples" % (what, need))
        if out is None:
            out = torch.empty(nblocks * C_, dtype=torch.complex64, device=tiles.device)
        if nblocks:              # (an empty tensor has no address to pass)
            if stream is None:
                stream = torch.cuda.current_stream(tiles.device)
            self._chk(fn(self._h, _dptr(tiles), int(first_block), nblocks, lead, _dptr(out), _stream_ptr(stream)), name)
        return out.view(-1)[:nblocks * C_]

    def generate(self, tx, frames_per_channel, payload_len, mod=LIQUID_MODEM_QPSK, fec0=LIQUID_FEC_NONE, fec1=LIQUID_FEC_HAMMING128,
                 gain=None, seed=0):
        """multichanneltx.generate with every user behind their own channel, in one call: tx.traffic(0, N, ...) -> tiles of blocks
        [-(lead_synth + lead_blocks), blocks) -> apply -> tx.synthesize.  -> (iq, sent), `gain` and `sent` as multichanneltx.generate
        has them; iq holds the blocks generate() returns for the same arguments."""
        import torch
        if self.num_channels != tx.N:
            raise ValueError("this handle has %d channels, the transmitter %d" % (self.num_channels, tx.N))
        tr = tx.traffic(0, tx.N, frames_per_channel, payload_len, mod, fec0, fec1, seed)
        try:
            nb, ls, lu = tr.blocks, USERCHAN_SYNTH_LEAD, self.lead_blocks
            tiles = torch.empty((ls + lu + nb) * tx.N, dtype=torch.complex64, device="cuda")
            tr.tiles(-(ls + lu), ls + lu + nb, tiles)
            mid = self.apply(tiles, -ls, ls + nb, lu)
            iq = tx.synthesize(mid, 1, 0, nb, ls, 0, gain)
            sent = tr.sent
        finally:
            tr.close()
        return iq, sent

    def close(self):
        if self._h:
            lib().mcrx_hip_userchan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TxTraffic(object):
    """The frames of one channel shard of a multichanneltx, modulated and resident in HBM (mctx_hip_traffic_*).
    sent[c] = [(header, payload), ...] for local channel c (global channel = channel_first + c)."""

    def __init__(self, tx, channel_first, channel_count, frames, payload_len, mod, fec0, fec1, seed, stream=None):
        import torch
        self._t = C.c_void_p()
        self.tx, self.channel_first, self.channel_count = tx, channel_first, channel_count
        hdr = np.zeros((channel_count, frames, 8), np.uint8)
        pay = np.zeros((channel_count, frames, max(payload_len, 1)), np.uint8)
        st = stream if stream is not None else torch.cuda.current_stream()
        rc = lib().mctx_hip_traffic_create(tx._h, C.byref(self._t), channel_first, channel_count, frames, payload_len, mod, fec0,
                                           fec1, seed & 0xFFFFFFFF, hdr.ctypes.data, pay.ctypes.data, _stream_ptr(st))
        if rc != MCRX_OK:
            self._t = C.c_void_p()
            _raise_rc(rc, "mctx_hip_traffic_create", lib().mctx_hip_last_error)
        self.blocks = int(lib().mctx_hip_blocks_for(tx._h, frames, payload_len, mod, fec0, fec1))
        self.sent = [[(bytes(hdr[c, f]), bytes(pay[c, f, :payload_len])) for f in range(frames)] for c in range(channel_count)]

    def tiles(self, first_block, nblocks, out, stream=None):
        """Channel-rate granules out[tile][c][8] of blocks [first_block, first_block+nblocks) (zeros outside the traffic)."""
        import torch
        assert nblocks % 8 == 0 and out.numel() >= nblocks * self.channel_count
        st = stream if stream is not None else torch.cuda.current_stream(out.device)
        _raise_rc(lib().mctx_hip_traffic_tiles(self._t, first_block, nblocks, _dptr(out), _stream_ptr(st)),
                  "mctx_hip_traffic_tiles", lib().mctx_hip_last_error, False)
        return out

    def close(self):
        if getattr(self, "_t", None) is not None and self._t:
            lib().mctx_hip_traffic_destroy(self._t)
            self._t = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class pipeline(object):
    """The C-ABI multi-GPU receive pipeline (mcrx_hip_pipeline_*: csrc/pipeline.hip) -- sharding.Pipeline's schedule without
    Python between the stages, the exchange as grouped ncclSend / ncclRecv.  `rx` is this rank's receiver handle (its channel
    shard, defer_samples set); world > 1: `unique_id` = the 128 bytes rank 0 got from pipeline.unique_id()."""

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        pipeline._chk(lib().mcrx_hip_pipeline_unique_id(buf), "unique_id")
        return bytes(buf)

    def __init__(self, rx, rank, world, sub_blocks, unique_id=None, nbuf=3):
        self._h = C.c_void_p()
        self.rx, self.rank, self.world, self.Tc = rx, rank, world, sub_blocks
        uid = None if unique_id is None else (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._chk(lib().mcrx_hip_pipeline_create(C.byref(self._h), rx._h, rank, world, uid, sub_blocks, nbuf), "create")
        self.rounds = 0

    @staticmethod
    def _chk(rc, what):
        _raise_rc(rc, "mcrx_hip_pipeline_" + what, lib().mcrx_hip_pipeline_last_error, False)

    def push(self, iq_sub, halo=None, after=None, ready=False):
        """`after`: the torch stream that produced iq_sub / halo (default: the current one) -- the round starts behind what is enqueued
        there.  ready=True: the buffers are complete (the caller has synchronized since writing them), wait for nothing
        (MCRX_STREAM_READY).  Mind that torch's default stream is HIP's legacy NULL stream: an event recorded there is a barrier
        across every blocking stream of the process, the handle's own included -- a caller that pushes from the default stream
        every round serializes its rounds (bench.py --pipeline: 170 -> 70 Gsample/s); push from a side stream, or say ready."""
        import torch
        if ready:
            ptr = C.c_void_p(-1 & 0xFFFFFFFFFFFFFFFF)
        else:
            st = after if after is not None else torch.cuda.current_stream(iq_sub.device)
            ptr = _stream_ptr(st)
        self._chk(lib().mcrx_hip_pipeline_push(self._h, _dptr(iq_sub), _dptr(halo), ptr), "push")
        self.rounds += 1

    def wait(self):
        self._chk(lib().mcrx_hip_pipeline_wait(self._h), "wait")

    def time_exchange(self, on=True):
        self._chk(lib().mcrx_hip_pipeline_time_exchange(self._h, 1 if on else 0), "time_exchange")

    def exchange_ms(self, reset=True):
        ms, n = C.c_double(), C.c_uint64()
        self._chk(lib().mcrx_hip_pipeline_exchange_ms(self._h, C.byref(ms), C.byref(n), 1 if reset else 0), "exchange_ms")
        return ms.value, int(n.value)

    def bytes_sent_per_round(self):
        return int(lib().mcrx_hip_pipeline_bytes_sent_per_round(self._h))

    def comm_count(self):
        """Ranks of the RCCL communicator behind the exchange, as ncclCommCount reports them (1 at world 1; -1: call missing)."""
        return int(lib().mcrx_hip_pipeline_comm_count(self._h))

    def reset(self, extra_samples=0):
        """multichannelrx::Reset() for the sharded receiver (every rank, same point of the stream): mcrx_hip_pipeline_reset."""
        self._chk(lib().mcrx_hip_pipeline_reset(self._h, int(extra_samples)), "reset")
        self.rounds = 0

    def close(self):
        if self._h:
            lib().mcrx_hip_pipeline_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class multichanneltx(object):
    """GPU multichannel OFDM transmitter used as the synthetic IQ source
    (reference: lib/multichanneltx.cc + the traffic loop of src/multichannel_tx.cc:163-213).

    generate(frames_per_channel, payload_len, ...) -> (iq, sent): iq is a torch complex64 CUDA
    tensor with the wideband stream, sent[ch] = [(header, payload), ...].

    output_format="sc16" (or 1) makes a transmitter of 16-bit integer IQ: generate, generate_ragged and synthesize then return (or
    take as `out`) a contiguous torch int16 CUDA tensor of shape (samples, 2) -- re, im of clamp(rint(v * 32768)), v the cf32
    transmitter's value, so `gain` sets the level against the full scale 1.0 -- which multichannelrx(..., input_format="sc16").Execute
    takes as it stands.  clipped() counts the samples that hit the range.  The host paths (GenerateSamples, UpdateData, frame) are
    cf32 only and raise McrxError there."""

    def __init__(self, num_channels, M, cp_len, taper_len, p=None, max_payload_len=2048, output_format="cf32"):
        self._h = C.c_void_p()
        output_format = _format_code(output_format, OUTPUT_FORMATS, "output_format")
        self.N, self.K, self.M, self.cp = num_channels, 2 * num_channels, M, cp_len
        self.max_payload_len, self._stream_max = max_payload_len, -1
        parr = None if p is None else np.ascontiguousarray(np.frombuffer(bytes(bytearray(p)), np.uint8))
        rc = lib().mctx_hip_create(C.byref(self._h), num_channels, M, cp_len, taper_len,
                                   None if parr is None else parr.ctypes.data)
        if rc != MCRX_OK:
            self._h = C.c_void_p()
            self._chk(rc, "mctx_hip_create")
        if output_format:
            self._chk(lib().mctx_hip_set_output_format(self._h, output_format), "mctx_hip_set_output_format")

    def GetNumChannels(self):
        return self.N

    @property
    def output_format(self):
        """0 (cf32) or 1 (sc16): OUTPUT_FORMATS"""
        return int(lib().mctx_hip_output_format(self._h))

    def clipped(self, reset=False):
        """Samples whose re or im hit the int16 range, over every generate / generate_ragged / synthesize since the last reset (waits
        for them); always 0 on a cf32 transmitter."""
        n = C.c_uint64(0)
        self._chk(lib().mctx_hip_clipped(self._h, C.byref(n), 1 if reset else 0), "mctx_hip_clipped")
        return int(n.value)

    def _slab(self, nsamples, device):
        """an output buffer of nsamples wideband samples in the transmitter's format"""
        return _empty_samples(nsamples, self.output_format, device)

    def generate(self, frames_per_channel, payload_len, mod=LIQUID_MODEM_QPSK, fec0=LIQUID_FEC_NONE,
                 fec1=LIQUID_FEC_HAMMING128, gain=None, seed=0xC0FFEE, nblocks=None, device=None):
        import torch
        nb = int(lib().mctx_hip_blocks_for(self._h, frames_per_channel, payload_len, mod, fec0, fec1))
        if nblocks is not None:
            nb = max(nb, (int(nblocks) + TILE - 1) // TILE * TILE)
        iq = self._slab(nb * self.K, device or "cuda")
        hdr = np.zeros((self.N, frames_per_channel, 8), np.uint8)
        pay = np.zeros((self.N, frames_per_channel, max(payload_len, 1)), np.uint8)
        g = (1.0 / self.N) if gain is None else gain
        stream = torch.cuda.current_stream(iq.device)
        rc = lib().mctx_hip_generate(self._h, _dptr(iq), nb, frames_per_channel, payload_len, mod, fec0, fec1, g,
                                     seed & 0xFFFFFFFF, hdr.ctypes.data, pay.ctypes.data, _stream_ptr(stream))
        self._chk(rc, "mctx_hip_generate", False)
        sent = [[(bytes(hdr[c, f]), bytes(pay[c, f, :payload_len])) for f in range(frames_per_channel)]
                for c in range(self.N)]
        return iq, sent

    def generate_ragged(self, nblocks, len_lo=64, len_hi=1200, gap_max=3, long_every=8, long_max=184, mod=LIQUID_MODEM_QPSK,
                        fec0=LIQUID_FEC_NONE, fec1=LIQUID_FEC_HAMMING128, gain=None, seed=0xC0FFEE, device=None):
        """Ragged traffic (src/multichannel_txrx.cc:227-267): frames of len_lo .. len_hi bytes after 0 .. gap_max idle symbols,
        a longer silence (16 .. 16 + long_max symbols) once in long_every frames, until `nblocks` blocks are full.
        -> (iq, sent, starts): sent[ch] = [(header, payload)], starts[ch] = [block index of each frame's first sample]."""
        import torch
        nb = (int(nblocks) + TILE - 1) // TILE * TILE
        L = self.M + self.cp
        shortest = int(lib().mctx_hip_blocks_for(self._h, 1, len_lo, mod, fec0, fec1)) - 64
        maxf = nb // max(shortest, L) + 2
        iq = self._slab(nb * self.K, device or "cuda")
        cnt = np.zeros(self.N, np.uint32); hdr = np.zeros((self.N, maxf, 8), np.uint8); ln = np.zeros((self.N, maxf), np.uint32)
        pay = np.zeros((self.N, maxf, max(len_hi, 1)), np.uint8); start = np.zeros((self.N, maxf), np.uint64)
        g = (1.0 / self.N) if gain is None else gain
        stream = torch.cuda.current_stream(iq.device)
        rc = lib().mctx_hip_generate_ragged(self._h, _dptr(iq), nb, maxf, len_lo, len_hi, gap_max, long_every, long_max, mod, fec0, fec1,
                                            g, seed & 0xFFFFFFFF, cnt.ctypes.data, hdr.ctypes.data, ln.ctypes.data, pay.ctypes.data,
                                            start.ctypes.data, _stream_ptr(stream))
        self._chk(rc, "mctx_hip_generate_ragged", False)
        sent = [[(bytes(hdr[c, f]), bytes(pay[c, f, :ln[c, f]])) for f in range(int(cnt[c]))] for c in range(self.N)]
        starts = [[int(start[c, f]) for f in range(int(cnt[c]))] for c in range(self.N)]
        return iq, sent, starts

    # ---- sharded form: channel-sharded frame generators, time-sharded synthesis bank (see sharding.TxPipeline)
    def traffic(self, channel_first, channel_count, frames_per_channel, payload_len, mod=LIQUID_MODEM_QPSK,
                fec0=LIQUID_FEC_NONE, fec1=LIQUID_FEC_HAMMING128, seed=0xC0FFEE, stream=None):
        """Frames of a channel shard (same recipe and seeds as generate()): a TxTraffic with .tiles() and .sent."""
        return TxTraffic(self, channel_first, channel_count, frames_per_channel, payload_len, mod, fec0, fec1, seed, stream)

    def synthesize(self, tiles, groups, first_block, nblocks, lead_blocks, keep_blocks=0, gain=None, out=None, stream=None):
        """Wideband samples of blocks [first_block-keep, first_block+nblocks) from exchanged channel-rate granules
        tiles[groups][(lead+nblocks)/8][N/groups][8] (mctx_hip_synthesize_tiles).  `out`: complex64, or on an sc16 transmitter
        a contiguous int16 tensor of (re, im) pairs; TypeError on the wrong dtype for the format."""
        import torch
        sc16 = self.output_format == OUTPUT_FORMATS["sc16"]
        if out is None:
            out = self._slab((keep_blocks + nblocks) * self.K, tiles.device)
        elif out.dtype != (torch.int16 if sc16 else torch.complex64):
            raise TypeError("this transmitter writes %s, not %s" % ("int16 (re, im) pairs" if sc16 else "complex64", out.dtype))
        elif sc16 and not out.is_contiguous():
            raise ValueError("device samples must be contiguous")
        assert tiles.numel() >= (lead_blocks + nblocks) * self.N and out.numel() >= (keep_blocks + nblocks) * self.K * (2 if sc16 else 1)
        g = (1.0 / self.N) if gain is None else gain
        st = stream if stream is not None else torch.cuda.current_stream(tiles.device)
        self._chk(lib().mctx_hip_synthesize_tiles(self._h, _dptr(tiles), groups, first_block, nblocks, lead_blocks, keep_blocks,
                                                  g, _dptr(out), _stream_ptr(st)), "mctx_hip_synthesize_tiles")
        return out

    # ---- class interface of the reference (lib/multichanneltx.cc:126-227), served by the GPU one symbol period at a time
    def _begin(self, payload_len):
        if self._stream_max < 0:
            self._stream_max = max(int(self.max_payload_len), int(payload_len))
            self._chk(lib().mctx_hip_stream_begin(self._h, self._stream_max), "mctx_hip_stream_begin")

    @staticmethod
    def _chk(rc, what, einval_is_value_error=True):
        _raise_rc(rc, what, lib().mctx_hip_last_error, einval_is_value_error)

    def Reset(self):
        if self._stream_max >= 0:
            self._chk(lib().mctx_hip_stream_reset(self._h), "mctx_hip_stream_reset")

    def IsChannelReadyForData(self, channel_id):
        if not 0 <= channel_id < self.N:
            raise ValueError("error: multichanneltx::IsChannelReadyForData(), invalid channel id")
        if self._stream_max < 0:
            return True
        return lib().mctx_hip_stream_ready(self._h, channel_id) == 1

    def UpdateData(self, channel_id, header, payload, mod=LIQUID_MODEM_QPSK, fec0=LIQUID_FEC_NONE, fec1=LIQUID_FEC_HAMMING128):
        """Returns False (the reference prints a warning and returns) when the channel is busy."""
        if not 0 <= channel_id < self.N:
            raise ValueError("error: multichanneltx::UpdateData(), invalid channel id")
        h = np.frombuffer(bytes(bytearray(header))[:8].ljust(8, b"\0"), np.uint8)
        pl = np.frombuffer(bytes(bytearray(payload)), np.uint8)
        self._begin(len(pl))
        rc = lib().mctx_hip_stream_update(self._h, channel_id, h.ctypes.data, pl.ctypes.data if len(pl) else None, len(pl), mod, fec0, fec1)
        if rc == MCRX_EBUSY:
            return False
        self._chk(rc, "mctx_hip_stream_update")
        return True

    def GenerateSamples(self, buffer=None):
        """The next 2N wideband samples (host numpy complex64; written into `buffer` when given)."""
        self._begin(0)
        out = np.empty(self.K, np.complex64) if buffer is None else buffer
        assert out.dtype == np.complex64 and out.size >= self.K and out.flags.c_contiguous
        self._chk(lib().mctx_hip_stream_generate(self._h, out.ctypes.data), "mctx_hip_stream_generate")
        return out

    def frame(self, header, payload, mod=LIQUID_MODEM_QPSK, fec0=LIQUID_FEC_NONE, fec1=LIQUID_FEC_HAMMING128, gain=1.0):
        """All samples of one frame of one frame generator (ofdmflexframegen assemble + writesymbol to the last
        symbol, lib/ofdmtxrx.cc:297-342), channel rate, host numpy complex64."""
        h = np.frombuffer(bytes(bytearray(header))[:8].ljust(8, b"\0"), np.uint8)
        pl = np.frombuffer(bytes(bytearray(payload)), np.uint8)
        n = int(lib().mctx_hip_frame_len(self._h, len(pl), mod, fec0, fec1))
        if n == 0:
            raise ValueError("unsupported frame properties")
        out = np.empty(n, np.complex64)
        self._chk(lib().mctx_hip_frame(self._h, h.ctypes.data, pl.ctypes.data if len(pl) else None, len(pl), mod, fec0, fec1,
                                       gain, out.ctypes.data, n), "mctx_hip_frame")
        return out

    def close(self):
        if self._h:
            lib().mctx_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class firpfbch2(object):
    """2x-oversampled analysis bank on the GPU (liquid firpfbch2_crcf analyzer): M channels, M/2 samples per step.

    analyze(x) takes a torch complex64 CUDA tensor holding a whole number of steps and returns [nsteps, M];
    the filter state carries over between calls (the last 2*m*M samples are kept in HBM)."""

    def __init__(self, num_channels, m, As=60.0):
        self._h = C.c_void_p()
        self.M, self.m = num_channels, m
        rc = lib().mcrx_hip_pfb2_create(C.byref(self._h), num_channels, m, As)
        if rc != MCRX_OK:
            self._h = C.c_void_p()
            _raise_rc(rc, "mcrx_hip_pfb2_create", lib().mcrx_hip_pfb2_last_error)
        self._hist = None
        self._step = 0

    def taps(self):
        h = np.zeros(2 * self.m * self.M, np.float32)
        _check(lib().mcrx_hip_pfb2_get_taps(self._h, h.ctypes.data, h.size))
        return h

    def reset(self):
        self._hist, self._step = None, 0

    def analyze(self, x):
        import torch
        M2, depth = self.M // 2, 2 * self.m * self.M
        n = int(x.numel())
        if n % M2:
            raise ValueError("input must be a whole number of M/2-sample steps")
        ns = n // M2
        lead = 0 if self._hist is None else int(self._hist.numel())
        buf = x if lead == 0 else torch.cat([self._hist, x])
        out = torch.empty((ns, self.M), dtype=torch.complex64, device=x.device)
        stream = torch.cuda.current_stream(x.device)
        rc = lib().mcrx_hip_pfb2_analyze(self._h, C.c_void_p(buf.data_ptr() + 8 * lead), lead, ns, self._step, _dptr(out),
                                         _stream_ptr(stream))
        _raise_rc(rc, "mcrx_hip_pfb2_analyze", lib().mcrx_hip_pfb2_last_error, False)
        self._hist = buf[-depth:].clone() if buf.numel() > depth else buf.clone()
        self._step += ns
        return out

    def close(self):
        if self._h:
            lib().mcrx_hip_pfb2_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ofdmflexframesync(multichannelrx):
    """One frame synchronizer fed its channel's samples directly -- the receive half of the reference's
    ofdmtxrx (lib/ofdmtxrx.cc:91,620-626) -- on the same kernels as the multichannel bank, without a channelizer.
    callback(header, header_valid, payload, payload_len, payload_valid, stats, userdata)."""

    def __init__(self, M, cp_len, taper_len, p=None, callback=None, userdata=None, **cfg):
        multichannelrx.__init__(self, 1, M, cp_len, taper_len, p, [userdata], [callback], single_channel=1, **cfg)
        self.K = 1

    execute = multichannelrx.Execute
    reset = multichannelrx.Reset


def ofdmflexframegen(M, cp_len, taper_len, p=None):
    """One frame generator (the transmit half of ofdmtxrx): .frame(header, payload, mod, fec0, fec1, gain)."""
    return multichanneltx(1, M, cp_len, taper_len, p)


def tiles_to_channels(chan, nch):
    """[tile][ch][TILE] (torch or numpy, complex) -> [ch][time] numpy array (test helper)."""
    a = chan.cpu().numpy() if hasattr(chan, "cpu") else np.asarray(chan)
    a = a.reshape(-1, nch, TILE)
    return np.ascontiguousarray(a.transpose(1, 0, 2)).reshape(nch, -1)
