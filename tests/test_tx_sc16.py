"""16-bit integer IQ (sc16) out of the transmitter, the part that needs no GPU: the numpy model of the quantiser pinned by hand-written
values; the new entry points declared, exported and bound; NULL handles answered; a bad output_format refused before any device is
looked for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import tx_sc16_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mctx_hip_set_output_format", "mctx_hip_output_format", "mctx_hip_clipped", "mctx_hip_selftest_quantise"]
LSB = 1.0 / 32768.0


def test_model_rounds_ties_to_even():
    lsb = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5, 0.49, 0.51, -0.51, 1000.5, 1001.5], np.float64)
    want = [0, 2, 2, 4, 0, -2, -2, -4, 0, 1, -1, 1000, 1002]
    assert model.quantise((lsb * LSB).astype(np.float32)).tolist() == want


def test_model_saturates_at_both_edges_and_counts_them():
    lsb = np.array([32767.0, 32767.4, 32767.5, 32768.0, 1e9, -32768.0, -32768.4, -32768.5, -32768.6, -32769.0, -1e9], np.float64)
    v = (lsb * LSB).astype(np.float32)
    assert model.quantise(v).tolist() == [32767, 32767, 32767, 32767, 32767, -32768, -32768, -32768, -32768, -32768, -32768]
    #                                 32767.5 rounds to 32768: outside          -32768.5 rounds to -32768: inside
    assert model.outside(v).tolist() == [False, False, True, True, True, False, False, False, True, True, True]
    inf = np.array([np.inf, -np.inf], np.float32)
    assert model.quantise(inf).tolist() == [32767, -32768] and model.outside(inf).tolist() == [True, True]


def test_model_stores_zero_for_nan_and_does_not_count_it():
    v = np.array([np.nan, -np.nan, 0.0, -0.0, np.float32(1e-45)], np.float32)
    assert model.quantise(v).tolist() == [0, 0, 0, 0, 0]
    assert not model.outside(v).any()
    x = np.array([complex(np.nan, 0.25), complex(0.5, -0.25), complex(1.0, 0.0), complex(0.0, -1.0), complex(0.0, -1.5)], np.complex64)
    assert model.quantise_iq(x).tolist() == [[0, 8192], [16384, -8192], [32767, 0], [0, -32768], [0, -32768]]
    assert model.clipped_samples(x) == 2                # +1.0 is one step past the largest integer, -1.0 is the smallest one


def test_new_symbols_are_declared_exported_and_bound(product):
    text = open(os.path.join(ROOT, "include", "mcrx_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    path = product.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in product.exported_symbols(), s
        assert re.search(r" T %s\b" % s, out), s
    assert product.OUTPUT_FORMATS == {"cf32": 0, "sc16": 1}


def test_null_handle_answers(product):
    L = product.lib()
    n = ctypes.c_uint64(7)
    assert L.mctx_hip_output_format(None) == 0
    assert L.mctx_hip_set_output_format(None, 1) == product.MCRX_EINVAL
    assert L.mctx_hip_set_output_format(None, 0) == product.MCRX_EINVAL
    assert L.mctx_hip_clipped(None, ctypes.byref(n), 0) == product.MCRX_EINVAL
    assert L.mctx_hip_clipped(None, None, 1) == product.MCRX_EINVAL


def test_unknown_output_format_is_an_argument_error_without_a_device(product):
    for bad in ("sc8", "", "SC16", 2, -1):
        with pytest.raises(ValueError) as ei:
            product.multichanneltx(2, 64, 8, 4, output_format=bad)
        assert "output_format" in str(ei.value)
