"""16-bit integer IQ (sc16) straight out of the resampler, the part that needs no GPU: the five entry points are declared, exported
and bound; a bad output_format and a gain that is not finite are argument errors before any device is looked for; NULL handles are
refused."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["msresamp_hip_set_output_format", "msresamp_hip_output_format", "msresamp_hip_set_output_gain", "msresamp_hip_output_gain",
       "msresamp_hip_clipped"]


def test_resampler_sc16_output_symbols_are_declared_exported_and_bound(product):
    text = open(os.path.join(ROOT, "include", "mcrx_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    path = product.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    L = product.lib()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in product.exported_symbols(), s
        assert re.search(r" T %s\b" % s, out), s
        assert getattr(L, s).argtypes is not None, s


def test_bad_resampler_output_format_is_an_argument_error_without_a_device(product):
    for bad in ("sc8", 7):
        with pytest.raises(ValueError) as ei:
            product.msresamp(2.0, output_format=bad)
        assert "output_format" in str(ei.value)


def test_gain_that_is_not_finite_is_an_argument_error_without_a_device(product):
    for bad in (float("nan"), float("inf"), -float("inf")):
        for fmt in ("cf32", "sc16"):
            with pytest.raises(ValueError) as ei:
                product.msresamp(2.0, output_format=fmt, gain=bad)
            assert "gain" in str(ei.value)


def test_null_resampler_handle_is_refused(product):
    L = product.lib()
    n = ctypes.c_uint64(5)
    assert L.msresamp_hip_set_output_format(None, 1) == product.MCRX_EINVAL
    assert L.msresamp_hip_set_output_format(None, 0) == product.MCRX_EINVAL
    assert L.msresamp_hip_set_output_gain(None, 1.0) == product.MCRX_EINVAL
    assert L.msresamp_hip_clipped(None, ctypes.byref(n), 0) == product.MCRX_EINVAL
    assert L.msresamp_hip_clipped(None, None, 1) == product.MCRX_EINVAL
    assert L.msresamp_hip_output_format(None) == 0
    assert L.msresamp_hip_output_gain(None) == 0.0
