#!/usr/bin/env python3
"""What the amplifier with memory (mcrx_hip_pamem_*, csrc/pamem.hip) costs on the wideband stream.  A secondary measurement -- bench.py
holds the headline metric.

    python bench_pamem.py [--samples N --steps K --warmup W --reps R --rms LEVEL --out FILE]

One slab of --samples samples (default: the 512-channel slab, 207.7 M) of complex Gaussian samples through handles of one process, into
buffers allocated beforehand, through the C-ABI on a side stream, HIP events around --steps calls; the median of --reps repetitions
with its spread (max - min) / median.  The amplifiers are mpd_model.SEVERITY's: Rapp p = 2 at 10 / 7 / 12 dB input back-off with
+5 / -8 / +3 degrees of AM/PM.  Legs, all in one session:
    rfchain_none              the streaming floor: rfchain with no stage on, cf32 to cf32 (8 B in + 8 B out a sample)
    rfchain_amplifier         rfchain's amplifier alone (the first of the three)
    pamem_b1_t1               one branch, the tap (0, 1): the same arithmetic through this kernel
    pamem_severity            SEVERITY's three single-tap branches on delays 0, 1, 2 (pamem_severity_sc16: sc16 in and out)
    pamem_b3_t3               three branches of three taps
    pamem_b4_t8               four branches of eight taps, delays up to 16
    composition_severity      what pamem_severity replaces: three rfchain launches and the torch shifts, weights and sums of the
                              tests' MemoryAmplifier (with the allocations torch makes for it)
Every leg reports ms a call, its algorithmic GB, that traffic as a fraction of 8 TB/s (HBM peak) and its time over the floor's: a leg
near 1 sits at the streaming floor, one far above it is bound by its arithmetic or by LDS (the record says which is the larger count:
amplifier evaluations a sample, taps a sample).  One JSON line; --out also writes it to a file.  Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8.0e12
IBO_DB, AMPM_DEG, SMOOTH = (10.0, 7.0, 12.0), (5.0, -8.0, 3.0), 2      # tests/mpd_model.py's SEVERITY
WEIGHTS = (1.0, 0.08 * np.exp(0.7j), -0.032 * np.exp(-0.4j))


def report(n, bytes_per_sample, ms):
    med = statistics.median(ms)
    gb = n * bytes_per_sample / 1e9
    return {"ms": round(med, 4), "reps_ms": [round(v, 4) for v in ms], "spread": round((max(ms) - min(ms)) / med, 4),
            "algorithmic_gb": round(gb, 4), "gsamples_per_s": round(n / med / 1e6, 2),
            "fraction_of_8_tb_per_s": round(gb * 1e9 / (med * 1e-3) / PEAK_BYTES_PER_S, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=207700000)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rms", type=float, default=0.1, help="level of the input per component against the full scale 1.0")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "pamem.json"))
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_product
    assert torch.cuda.is_available(), "bench_pamem.py needs the GPU"
    prod = load_product()
    L = prod.lib()
    dev = torch.device("cuda", 0)
    n = args.samples
    gen = torch.Generator(device=dev)
    gen.manual_seed(25)
    d_x = torch.view_as_complex(torch.randn((n, 2), generator=gen, device=dev) * args.rms)
    d_f = torch.empty(n, dtype=torch.complex64, device=dev)
    side = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(side.cuda_stream)
    amp_rms = args.rms * 2.0 ** 0.5
    amps = [dict(sat=prod.rfchain_backoff(ibo, amp_rms), smooth=SMOOTH, gain=1.0, ampm_deg=deg) for ibo, deg in zip(IBO_DB, AMPM_DEG)]

    def timed(fn, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            a.record(side)
            for _ in range(k):
                fn()
            b.record(side)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / k

    def measure(fn):
        timed(fn, args.warmup)
        return [timed(fn, args.steps) for _ in range(args.reps)]

    def ok(rc, what, err):
        if rc != prod.MCRX_OK:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, err().decode()))

    out = {"metric": "amplifier with memory on the wideband stream", "device": torch.cuda.get_device_name(0), "samples": n, "rms": args.rms,
           "steps": args.steps, "reps": args.reps, "legs": {}}

    def rfchain_leg(name, **kw):
        h = prod.rfchain(**kw)

        def call():
            ok(L.mcrx_hip_rfchain_execute_device(h._h, C.c_void_p(d_x.data_ptr()), 0, n, C.c_void_p(d_f.data_ptr()), sp),
               "mcrx_hip_rfchain_execute_device", L.mcrx_hip_rfchain_last_error)
        out["legs"][name] = report(n, 16, measure(call))
        h.close()
    rfchain_leg("rfchain_none")
    rfchain_leg("rfchain_amplifier", amplifier=amps[0])

    def pamem_leg(name, branches, src, dst, nbytes, **kw):
        h = prod.pamem(branches, **kw)
        count = n - h.lead

        def call():
            ok(L.mcrx_hip_pamem_execute_device(h._h, C.c_void_p(src.data_ptr()), count, C.c_void_p(dst.data_ptr()), sp),
               "mcrx_hip_pamem_execute_device", L.mcrx_hip_pamem_last_error)
        out["legs"][name] = report(count, nbytes, measure(call))
        out["legs"][name].update(branches=len(branches), taps=sum(len(b["taps"]) for b in branches), lead=h.lead)
        if kw.get("output_format") == "sc16":
            out["legs"][name]["clipped_per_call"] = h.clipped() // (args.warmup + args.steps * args.reps)
        h.close()

    def tap(k):
        return complex(0.5 ** k * np.exp(0.7j * k))
    severity = [dict(a, taps=[(b, w)]) for b, (a, w) in enumerate(zip(amps, WEIGHTS))]
    pamem_leg("pamem_b1_t1", [dict(amps[0], taps=[(0, 1.0)])], d_x, d_f, 16)
    pamem_leg("pamem_severity", severity, d_x, d_f, 16)
    pamem_leg("pamem_b3_t3", [dict(a, taps=[(b, tap(0)), (b + 3, tap(1)), (b + 7, tap(2))]) for b, a in enumerate(amps)], d_x, d_f, 16)
    pamem_leg("pamem_b4_t8", [dict(a, taps=[((0, 1, 0, 2)[b] + 2 * k, tap(k)) for k in range(8)]) for b, a in enumerate(amps + amps[:1])], d_x, d_f, 16)
    d_i = torch.view_as_real(d_f).view(torch.int16).view(-1, 2)[:n]     # the sc16 legs' input lives in the first half of d_f, their output behind it
    d_o = torch.view_as_real(d_f).view(torch.int16).view(-1, 2)[n:2 * n]
    d_i.copy_((torch.view_as_real(d_x) * 32768.0).round_().clamp_(-32768, 32767).to(torch.int16))
    torch.cuda.synchronize()
    pamem_leg("pamem_severity_sc16", severity, d_i, d_o, 8, input_format="sc16", output_format="sc16")

    # the composition: tests/test_gpu_mpd.py's MemoryAmplifier, call for call
    hs = [prod.rfchain(amplifier=a) for a in amps]
    ws = [complex(w) for w in WEIGHTS]

    def composition():
        z = hs[0].execute(d_x, 0, stream=side) * ws[0]
        for b in (1, 2):
            z[b:] += hs[b].execute(d_x, 0, stream=side)[:n - b] * ws[b]
        return z
    timed(composition, 1)
    ms = [timed(composition, 1) for _ in range(args.reps)]
    out["legs"]["composition_severity"] = report(n, 16, ms)
    for h in hs:
        h.close()
    rfchain_leg("rfchain_none_again")

    legs = out["legs"]
    for name, leg in legs.items():
        leg["over_floor"] = round(leg["ms"] / legs["rfchain_none"]["ms"], 4)
    out["severity_over_composition"] = round(legs["pamem_severity"]["ms"] / legs["composition_severity"]["ms"], 4)
    out["severity_is_faster_than_the_composition"] = legs["pamem_severity"]["ms"] < legs["composition_severity"]["ms"]
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)
    if not out["severity_is_faster_than_the_composition"]:
        sys.exit("pamem_severity is not faster than the composition it replaces")


if __name__ == "__main__":
    main()
