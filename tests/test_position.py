"""CPU checks of tests/position_model.py: the identities the far-position GPU tests (tests/test_gpu_position.py) lean on,
verified with Python integers and float64 before anything on the GPU is compared through them."""
import math

import numpy as np
import pytest

import position_model as pm

RATES = [0.5, 0.37, 0.8, 0.2, 0.11, 2.0, 1.5, 4.0, 6.3, 0.25, 0.45, 0.06]      # test_msresamp_front_end_matches_oracle's


@pytest.mark.parametrize("N", [3, 8])
@pytest.mark.parametrize("s0", [(1 << 32) - 32 * 16, 5 * 16 * 16 + (1 << 52), (1 << 40) + 12345])
def test_moving_the_origin_rotates_by_one_constant(N, s0):
    """Mixing sample by sample with the exact 32-bit phase word of t = s0 + i equals mixing from origin 0 and multiplying by
    origin_rotation(s0): the phase words add modulo 2^32, wrap inside the span included.  float64; the two sides differ by
    the rounding of one complex multiply."""
    dth = pm.nco_dtheta(N)
    assert 0 < dth < 1 << 32
    n = 96 * 2 * N
    rng = np.random.RandomState(N)
    x = rng.randn(n) + 1j * rng.randn(n)
    w = 2.0 * math.pi / 2.0 ** 32
    far = x * np.exp(-1j * w * np.array([pm.nco_phase(s0 + i, dth) for i in range(n)], np.float64))
    org = x * np.exp(-1j * w * np.array([pm.nco_phase(i, dth) for i in range(n)], np.float64))
    assert any(pm.nco_phase(s0 + i + 1, dth) < pm.nco_phase(s0 + i, dth) for i in range(n - 1))     # (the word wraps inside the span)
    c = pm.origin_rotation(s0, dth)
    assert abs(abs(c) - 1.0) < 1e-15
    assert np.max(np.abs(far - c * org)) <= 8 * np.finfo(np.float64).eps * np.max(np.abs(x))
    # only the low 32 bits of the origin count
    assert pm.origin_rotation(s0 + (7 << 32), dth) == c
    # negative origins (history in front of sample 0) follow the same rule
    assert abs(pm.origin_rotation(-s0, dth) - c.conjugate()) < 1e-15


@pytest.mark.parametrize("rate", RATES)
def test_resampler_plan_and_aligned_positions(rate):
    p = pm.ResampPlan(rate)
    assert 0.5 <= p.rate_arb <= 2.0
    assert abs(p.rate_arb * (2.0 if p.interp else 0.5) ** p.num_stages - float(np.float32(rate))) < 1e-12
    assert p.step == int(round(2 ** 24 / p.rate_arb)) and p.per_in * p.g == p.step and p.per_out * p.g == 1 << 24
    assert math.gcd(p.per_in, p.per_out) == 1
    for target in (1 << 40, 1 << 41, 1 << 48, 1 << 56):
        raw = p.aligned_raw_at_or_above(target)
        k = p.raw_per_arb()
        assert raw >= target and raw % (1 << p.num_stages) == 0 and raw % k == 0
        a = raw // k
        assert a % p.per_in == 0
        j = p.first_output(a)
        assert p.phase(j) == (a, 0)                                  # the output that reads from there has phase fraction 0, like output 0
        assert j % p.per_out == 0 and j // p.per_out == a // p.per_in
        assert raw - target < p.unit * k                             # ... and it is the first such position
        for d in (1, 2, 1000):                                       # the phases that follow are those after the origin
            assert p.phase(j + d) == (a + p.phase(d)[0], p.phase(d)[1])
    assert p.aligned_arb_at_or_below((1 << 40) - 4096) <= (1 << 40) - 4096 < p.aligned_arb_at_or_below((1 << 40) - 4096) + p.unit


@pytest.mark.parametrize("rate", [0.5, 0.8, 2.0, 1.5, 0.37, 6.3])
def test_crossing_plan(rate):
    p = pm.ResampPlan(rate)
    seek, sizes, straddle = pm.crossing_plan(p)
    k = p.raw_per_arb()
    assert seek % k == 0 and (seek // k) % p.per_in == 0 and seek // k <= (1 << 40) - 4096
    assert sum(sizes) <= 1 << 27 and all(0 < s <= 4 << 20 for s in sizes)
    cross = ((1 << 40) - seek // k) * k
    ends = np.cumsum(sizes)
    assert ends[straddle - 1] < cross <= ends[straddle - 1] + 8          # one push ends just before the boundary,
    assert ends[straddle] > cross                                        # the next straddles it,
    assert straddle + 2 == len(sizes) and ends[-1] == cross + 64 * 1024  # and one starts after it
    if rate in (0.5, 0.8, 2.0):
        assert (1 << 40) - 4096 - seek // k < 16                         # (large gcd: alignment within a few samples of any target)
    else:
        assert p.per_in > 1 << 20                                             # (2^24 / 1.5 is no integer: its step is odd, like 0.37's)
