"""The spans of the block-rate tables (chanemu's fading gains, rfchain's oscillator phase, userchan's fading gains), the part that needs
no GPU: host/span_plan_test.cc (host compiler only) replays tests/golden/span_plan_cases.txt through csrc/span_plan.hpp -- cap, the rows
asked for and every span (m, row0, rows) must equal what the three execute loops computed while this arithmetic lived between their
launch calls -- and holds every case to what the plan promises: the spans tile the call, fit the table, end on grid rows, keep
userchan's granules of 8 and make progress.

On the GPU the spans are reached by test_gpu_chanemu_fading.py::test_cut_anywhere (its table_rows cases), test_gpu_rfchain.py::
test_cuts_spans_and_in_place and test_gpu_userchan_fading.py::test_spans_of_the_gain_table."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_span_plan_replays_the_recorded_spans():
    host = os.path.join(ROOT, "liquid-usrp_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "span_plan_test"])
    out = subprocess.run([os.path.join(ROOT, "liquid-usrp_amd", "lib", "span_plan_test"), os.path.join(ROOT, "tests", "golden", "span_plan_cases.txt")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("span_plan_test ok"), out.stdout
    assert "240 chanemu, 160 rfchain, 240 userchan cases replayed" in out.stdout, out.stdout
