"""Exact integer models of the position arithmetic, for the far-position tests (tests/test_gpu_position.py; checked on the
CPU by tests/test_position.py).  Python integers throughout: nothing here can wrap.

Oscillator (csrc/channelizer.hip): wideband sample t is mixed down by the phase word (t * dtheta) mod 2^32, so moving the
origin of a stream by s samples multiplies every output of the (linear) bank by one constant, origin_rotation(s, dtheta).

Resampler (csrc/msresamp.hip, msresamp_hip_create): the rate is halved or doubled into [0.5, 2]; the arbitrary stage steps a
24-bit fractional phase by step = round(2^24 / rate_arb) per output.  Its phase fraction is exactly 0 -- as at the origin --
at the input indices m * step / gcd(step, 2^24): the ALIGNED positions, from which the output is bit-identical to a fresh
stream's."""
import math

import numpy as np

PHASE_BITS = 24


def nco_dtheta(N):
    """The receiver's 32-bit phase step per wideband sample (mcrx_hip_nco_step): -(N-1)/N * pi/2 ... as float32, like the reference."""
    f = np.float32(-0.5) * np.float32(N - 1) / np.float32(N)
    p = float(np.float32(float(f) * np.pi)) / (2 * np.pi)
    return int(np.rint((p - np.floor(p)) * 2.0 ** 32)) & 0xFFFFFFFF


def nco_phase(t, dtheta):
    """Phase word of sample t (any integer, negative too)."""
    return (int(t) * int(dtheta)) % (1 << 32)


def origin_rotation(s, dtheta):
    """c with output(origin s) = c * output(origin 0) for a mix-DOWN by the phase word: exp(-j 2 pi ((s dtheta) mod 2^32) / 2^32).
    (The transmitter mixes up: its constant is the conjugate.)"""
    th = 2.0 * math.pi * nco_phase(s, dtheta) / 2.0 ** 32
    return complex(math.cos(th), -math.sin(th))


class ResampPlan(object):
    """msresamp_hip_create's decomposition of a float32 rate."""

    def __init__(self, rate):
        r = float(np.float32(rate))
        self.rate = r
        self.interp = r > 1.0
        self.num_stages = 0
        while (r > 2.0) if self.interp else (r < 0.5):
            r = r * 0.5 if self.interp else r * 2.0
            self.num_stages += 1
        self.rate_arb = r
        self.step = int(round((1 << PHASE_BITS) / r))            # (llrint: both round half to even)
        self.g = math.gcd(self.step, 1 << PHASE_BITS)
        self.per_in = self.step // self.g                       # aligned positions: multiples of this many arbitrary-stage inputs
        self.per_out = (1 << PHASE_BITS) // self.g              # ... which is this many of its outputs
        # msresamp_hip_reset_at takes multiples of 2^num_stages only.  A decimator's arbitrary stage sits behind the half-band
        # stages, so every one of its input indices is such a position; an interpolator's comes first: every 2^num_stages-th
        # aligned index (at most) is one.
        self.unit = self.per_in * (1 << self.num_stages) // math.gcd(self.per_in, 1 << self.num_stages) if self.interp else self.per_in

    def raw_per_arb(self):
        """Resampler input samples per input sample of the arbitrary stage (decimating: the half-band stages come first)."""
        return 1 if self.interp else 1 << self.num_stages

    def phase(self, j):
        """(input index, 24-bit fraction) of output j of the arbitrary stage."""
        p = j * self.step
        return p >> PHASE_BITS, p & ((1 << PHASE_BITS) - 1)

    def first_output(self, a):
        """First output of the arbitrary stage that reads input index >= a."""
        return -((-(a << PHASE_BITS)) // self.step)

    def aligned_arb_at_or_above(self, a):
        return -((-a) // self.unit) * self.unit

    def aligned_arb_at_or_below(self, a):
        return a // self.unit * self.unit

    def aligned_raw_at_or_above(self, raw):
        """First aligned position (as a resampler input position) at or above input sample `raw`."""
        k = self.raw_per_arb()
        return self.aligned_arb_at_or_above(-((-raw) // k)) * k


def crossing_plan(plan, boundary_arb=1 << 40, margin_arb=4096, tail_raw=64 * 1024, push_max=4 << 20, near=8):
    """Where to seek and how to push so that the arbitrary stage's input index crosses `boundary_arb`:
    (seek position [raw], push sizes [raw], index of the push that straddles the boundary).  The seek position is the largest
    aligned one at least margin_arb arbitrary-stage inputs below the boundary; pushes of at most push_max samples; one push ends
    `near` raw samples before the boundary, the next straddles it, the last starts after it and ends tail_raw samples past it."""
    k = plan.raw_per_arb()
    a0 = plan.aligned_arb_at_or_below(boundary_arb - margin_arb)
    cross = (boundary_arb - a0) * k                               # raw samples from the seek position to the boundary
    cuts, pos = [], 0
    while cross - near - pos > push_max:
        pos += push_max
        cuts.append(pos)
    cuts += [cross - near, cross + tail_raw // 2, cross + tail_raw]
    sizes = [b - a for a, b in zip([0] + cuts[:-1], cuts)]
    return a0 * k, sizes, len(sizes) - 2
