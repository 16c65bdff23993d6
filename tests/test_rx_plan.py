"""The receiver's creation path, the part that needs no GPU: host/rx_plan_test.cc (host compiler only) replays tests/golden/rx_plan_cases.txt
through csrc/rx_plan.hpp -- every size, build selector and refusal must equal what mcrx_hip_create derived while the arithmetic lived
in its body -- and holds the accepted cases to what the code's comments promise about those sizes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rx_plan_replays_the_recorded_sizes_and_refusals():
    host = os.path.join(ROOT, "liquid-usrp_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "rx_plan_test"])
    out = subprocess.run([os.path.join(ROOT, "liquid-usrp_amd", "lib", "rx_plan_test"), os.path.join(ROOT, "tests", "golden", "rx_plan_cases.txt")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok"), out.stdout
    assert "accepted" in out.stdout and "refused" in out.stdout, out.stdout
