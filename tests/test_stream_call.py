"""What execute_device of chanemu, rfchain, rfcal and cfr checks about a call, the part that needs no GPU: host/stream_call_test.cc
(host compiler only) puts to csrc/stream_call.hpp, on integers, the calls that tests/test_gpu_{chanemu,rfchain,rfcal,cfr}.py make with
real pointers -- misaligned buffers per format, in place with equal and unequal formats, first-on-last overlaps in both directions,
adjacent buffers, the 2^32 limit with and without cfr's halos, a null d_out allowed and refused -- and asks for the message of each."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_call_check_judges_the_calls_of_the_gpu_tests():
    host = os.path.join(ROOT, "liquid-usrp_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "stream_call_test"])
    out = subprocess.run([os.path.join(ROOT, "liquid-usrp_amd", "lib", "stream_call_test")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert out.returncode == 0 and b"stream_call_test ok" in out.stdout, out.stdout.decode()
