"""The receiver's host-side launch path, the part that needs no GPU: host/acq_plan_test.cc (host compiler only) replays the recorded
launch sequences of tests/golden/acq_plan_cases.txt through csrc/acq_plan.hpp -- every decision of every launch must equal what the
policy decided while it lived inside launch_sync -- checks the plan's invariants, and holds csrc/config_read.hpp to the struct_size rule."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_acq_plan_replays_the_recorded_policy_and_config_cuts():
    host = os.path.join(ROOT, "liquid-usrp_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "acq_plan_test"])
    out = subprocess.run([os.path.join(ROOT, "liquid-usrp_amd", "lib", "acq_plan_test"), os.path.join(ROOT, "tests", "golden", "acq_plan_cases.txt")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok"), out.stdout
    assert "sequences" in out.stdout and "cuts" in out.stdout, out.stdout
