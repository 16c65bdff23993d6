"""The sc16 transmitter's quantiser as numpy (include/mcrx_hip.h, mctx_hip_set_output_format): for the fp32 value v a cf32 transmitter
stores, Q(v) = clamp(r, -32768, 32767) with r = rint(v * 32768) in fp32, round half to even; NaN -> 0; a sample is clipped when r is
outside the range for its re or its im (NaN does not count)."""
import numpy as np

FULL_SCALE = np.float32(32768.0)


def rounded(v):
    """r = rint(v * 32768), in fp32 (the multiply is exact up to overflow, which gives the infinity that saturates)"""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.rint(v * FULL_SCALE)


def quantise(v):
    """float32 components -> int16"""
    r = rounded(v)
    r = np.where(np.isnan(r), np.float32(0.0), r)
    return np.clip(r, -32768.0, 32767.0).astype(np.int16)


def outside(v):
    """per component: r outside [-32768, 32767] (False for NaN)"""
    r = rounded(v)
    with np.errstate(invalid="ignore"):
        return (r > 32767.0) | (r < -32768.0)


def quantise_iq(x):
    """complex64 samples -> int16 [n, 2] (re, im)"""
    x = np.ascontiguousarray(x, np.complex64)
    return quantise(x.view(np.float32)).reshape(-1, 2)


def clipped_samples(x):
    """number of samples with a component outside the range"""
    x = np.ascontiguousarray(x, np.complex64)
    return int(np.count_nonzero(outside(x.view(np.float32)).reshape(-1, 2).any(axis=1)))
