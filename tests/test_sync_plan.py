"""The synchronizer's launchers, the part that needs no GPU: host/sync_plan_test.cc (host compiler only) replays
tests/golden/sync_plan_cases.txt through csrc/sync_plan.hpp -- every kernel, grid, block, LDS size and rewritten SyncArgs field must equal
what the launchers issued while the decisions lived between their launch calls -- and holds every case to what the code promises about them.

On the GPU each launch target (SyncKernel) is reached by these tests, going by their configurations:
  sync_kernel<1>                      test_gpu_alloc.py::test_receiver_with_a_custom_allocation_matches_oracle[one_kernel_scout-*] (acquisition = 4)
  sync_kernel<2>, sync_lean_kernel<2> test_gpu_parity.py::test_alternate_scouts_at_two_samples_per_lane[one_kernel_scout], [budgeted_scout]
  sync_kernel<4 | 8 | 16>             test_gpu_parity.py::test_wide_symbols_take_the_lean_path[256 | 512 | 1024] (scout and tail of E >= 4; 1024: not a fast design)
  sync_spec_kernel<1>, sync_tail_kernel<1>, sync_walk_kernel<1>
                                      test_gpu_parity.py::test_both_builds_of_the_rounds_scout_equal_the_oracle[0]
  sync_spec_ / _tail_ / _walk_kernel<2>, sync_spec_kernel<4 | 8>
                                      test_gpu_parity.py::test_wide_symbols_take_the_lean_path[128], [256 | 512]
  sync_lean_kernel<1>, acq_lean_kernel<63, 64>
                                      test_gpu_parity.py::test_both_builds_of_the_rounds_scout_equal_the_oracle[1], [2]
  acq_lean_kernel<63, 48>, payload_lean_kernel<63, 48>, payload_lean_rest_kernel<63, 48>
                                      test_gpu_stream.py::test_reference_app_default_numerology_takes_the_lean_path[40-6-300-2], [40-6-300-0]
  payload_lean_kernel + payload_lean_rest_kernel <63> | <0>, payload_multi_kernel<1>
                                      test_gpu_stream.py::test_lean_payload_workers_every_modem_in_one_slab[0] | [1], [2]
  payload_multi_kernel<2 | 4>, payload_kernel<1, true>
                                      test_gpu_stream.py::test_payload_worker_builds_agree[3 | 4], [5]
  payload_wide_kernel<63, 2 | 4>, payload_kernel<2 | 4, true>
                                      test_gpu_parity.py::test_wide_payload_workers[*-128-16 | *-256-32] (worker_build 0, 5)
  payload_kernel<8, true>, payload_kernel<16, false>
                                      test_gpu_parity.py::test_wide_symbols_take_the_lean_path[512], [1024]
  place_jobs_kernel, decode_kernel    every receiver test of a fast design; decode_general_kernel's list is filled by
                                      test_gpu_parity.py::test_convolutional_k7_rate_half_viterbi
No test reaches sync_spec_kernel<16> and payload_kernel<16, true> (1024 subcarriers with at most 64 pilots: a custom allocation, whose symbol
error at that width lies at the parity bar) nor payload_kernel<1 | 2 | 4 | 8, false> (designs off the fast path at those widths -- not 64 E
subcarriers, or more than 64 pilots -- or MCRX_NO_FAST in a development build)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sync_plan_replays_the_recorded_launches():
    host = os.path.join(ROOT, "liquid-usrp_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "sync_plan_test"])
    out = subprocess.run([os.path.join(ROOT, "liquid-usrp_amd", "lib", "sync_plan_test"), os.path.join(ROOT, "tests", "golden", "sync_plan_cases.txt")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok"), out.stdout
    assert "acquisition" in out.stdout and "payload cases replayed" in out.stdout, out.stdout
