"""16-bit integer IQ (sc16) straight into the resampler, the part that needs no GPU: the three entry points are declared, exported
and bound; a bad input_format is an argument error before any device is looked for; NULL handles are refused."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["msresamp_hip_set_input_format", "msresamp_hip_input_format", "msresamp_hip_execute_device_sc16"]


def test_resampler_sc16_symbols_are_declared_exported_and_bound(product):
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


def test_bad_resampler_input_format_is_an_argument_error_without_a_device(product):
    for bad in ("sc8", 7):
        with pytest.raises(ValueError) as ei:
            product.msresamp(0.5, input_format=bad)
        assert "input_format" in str(ei.value)


def test_null_resampler_handle_is_refused(product):
    L = product.lib()
    buf = (ctypes.c_int16 * 8)()
    out = (ctypes.c_float * 16)()
    nout = ctypes.c_size_t(5)
    assert L.msresamp_hip_set_input_format(None, 1) == product.MCRX_EINVAL
    assert L.msresamp_hip_input_format(None) == 0
    assert L.msresamp_hip_execute_device_sc16(None, buf, 4, out, 8, ctypes.byref(nout), None) == product.MCRX_EINVAL
