"""16-bit integer IQ (sc16) input, the part that needs no GPU: the two entry points are declared, exported and bound; a bad
input_format is an argument error before any device is looked for; NULL handles are refused."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mcrx_hip_execute_host_sc16", "mcrx_hip_execute_device_sc16"]


def test_sc16_symbols_are_declared_exported_and_bound(product):
    text = open(os.path.join(ROOT, "include", "mcrx_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    path = product.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in product.exported_symbols(), s
        assert re.search(r" T %s\b" % s, out), s
    assert re.search(r"uint32_t\s+input_format\s*;", text)
    assert product.Config._fields_[-1][0] == "input_format"          # appended: older callers' struct_size ends before it
    assert product.INPUT_FORMATS == {"cf32": 0, "sc16": 1}


def test_bad_input_format_is_an_argument_error_without_a_device(product):
    with pytest.raises(ValueError) as ei:
        product.multichannelrx(2, 64, 8, 4, input_format=7)
    assert "input_format" in str(ei.value)
    with pytest.raises(ValueError):
        product.multichannelrx(2, 64, 8, 4, input_format="sc8")
    # (the C-ABI itself, through struct_size: a caller whose struct ends before the field is a cf32 caller, whatever follows)
    c = product.Config()
    c.struct_size, c.payload_soft, c.input_format = ctypes.sizeof(product.Config), 1, 7
    h = ctypes.c_void_p()
    assert product.lib().mcrx_hip_create(ctypes.byref(h), 2, 64, 8, 4, None, ctypes.addressof(c)) == product.MCRX_EINVAL
    assert b"input_format" in product.lib().mcrx_hip_last_error()
    assert not h.value


def test_null_handle_is_refused(product):
    L = product.lib()
    buf = (ctypes.c_int16 * 8)()
    assert L.mcrx_hip_execute_host_sc16(None, buf, 4) == product.MCRX_EINVAL
    assert L.mcrx_hip_execute_device_sc16(None, buf, 4, None) == product.MCRX_EINVAL
    assert L.mcrx_hip_input_format(None) == 0
