#!/usr/bin/env python3
"""What the receiver calibration (mcrx_hip_rfcal_*, csrc/rfcal.hip) costs on the wideband stream.  A secondary measurement -- bench.py
holds the headline metric.

    python bench_rfcal.py [--samples N --steps K --warmup W --reps R --rms LEVEL --out FILE]

One slab of --samples samples (default: the 512-channel slab, 207.7 M) through handles of one process, into output buffers allocated
beforehand, through the C-ABI on a side stream, HIP events around --steps calls; the median of --reps repetitions with its spread
(max - min) / median.  Legs:
    copy_d2d          hipMemcpyAsync device to device of the same 8 B a sample, timed in the same session
    rfchain_none      the streaming floor: rfchain with no stage on, cf32 to cf32 (8 B in + 8 B out a sample), rerun here
    measure_cf32, measure_sc16        measure only (8 B / 4 B in, nothing out), one update a call
    apply_only        a held handle with coefficients set: cf32 to cf32, nothing measured
    fused             apply and measure in one pass, period_log2 = 0, one update a call
    fused_p16, fused_p20, fused_p24   the same with automatic blocks of 2^16, 2^20, 2^24 samples: a kernel and a fold per block
    fused_sc16        sc16 in, sc16 out, period_log2 = 0
    torch_composed    the five sums and the correction as torch expressions on the slab
"separate" is measure_cf32 + apply_only, what the fused pass is compared with.  Every leg reports ms a call, its algorithmic GB and
that traffic as a fraction of 8 TB/s (HBM peak).  One JSON line; --out also writes it to a file.  Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8.0e12


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
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "rfcal.json"))
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_product
    assert torch.cuda.is_available(), "bench_rfcal.py needs the GPU"
    prod = load_product()
    L = prod.lib()
    dev = torch.device("cuda", 0)
    n = args.samples
    gen = torch.Generator(device=dev)
    gen.manual_seed(16)
    mix = prod.rfchain_iq(1.0, 5.0, "rx")
    d_x = torch.view_as_complex(torch.randn((n, 2), generator=gen, device=dev) * args.rms)
    imp = prod.rfchain(order="rx", mixer=dict(mix, dc=0.01 + 0.005j))   # the slab a receive mixer left: there is something to estimate
    imp.execute(d_x, out=d_x)
    imp.close()
    d_f = torch.empty(n, dtype=torch.complex64, device=dev)
    d_i = torch.empty((n, 2), dtype=torch.int16, device=dev)
    side = torch.cuda.Stream(device=dev)
    conv = prod.rfchain(output_format="sc16")                          # the sc16 legs' input: Q of the slab
    d_xi = conv.execute(d_x).clone()
    conv.close()
    torch.cuda.synchronize()
    sp = C.c_void_p(side.cuda_stream)

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

    out = {"metric": "receiver calibration on the wideband stream", "device": torch.cuda.get_device_name(0), "samples": n, "rms": args.rms,
           "steps": args.steps, "reps": args.reps, "legs": {}}

    def copy():
        d_f.copy_(d_x, non_blocking=True)
    out["legs"]["copy_d2d"] = report(n, 16, measure(copy))

    rf = prod.rfchain()

    def floor():
        rc = L.mcrx_hip_rfchain_execute_device(rf._h, C.c_void_p(d_x.data_ptr()), 0, n, C.c_void_p(d_f.data_ptr()), sp)
        if rc != prod.MCRX_OK:
            raise RuntimeError("mcrx_hip_rfchain_execute_device failed (%d)" % rc)
    out["legs"]["rfchain_none"] = report(n, 16, measure(floor))
    rf.close()

    # (name, constructor arguments, writes?, held with coefficients set?)
    legs = [("measure_cf32", dict(), False, False), ("measure_sc16", dict(input_format="sc16"), False, False),
            ("apply_only", dict(), True, True), ("fused", dict(), True, False),
            ("fused_p16", dict(period_log2=16, forget_log2=3), True, False), ("fused_p20", dict(period_log2=20, forget_log2=3), True, False),
            ("fused_p24", dict(period_log2=24, forget_log2=3), True, False),
            ("fused_sc16", dict(input_format="sc16", output_format="sc16"), True, False)]
    for name, kw, writes, held in legs:
        cal = prod.rfcal(**kw)
        src = d_xi if cal.input_format else d_x
        dst = (d_i if cal.output_format else d_f) if writes else None
        manual = int(cal.config.period_log2) == 0
        if held:
            cal.set(0.01 + 0.005j, mix["beta"] / mix["alpha"].conjugate(), stream=side)
            cal.hold(True)
        elif writes:                                                    # a first pass, so that the timed ones carry the apply code
            cal.measure(src[:1 << 24], stream=side)
            if manual:
                cal.update(stream=side)

        def call(cal=cal, src=src, dst=dst, manual=manual, held=held):
            rc = L.mcrx_hip_rfcal_execute_device(cal._h, C.c_void_p(src.data_ptr()), n, C.c_void_p(dst.data_ptr()) if dst is not None else None, sp)
            if rc == prod.MCRX_OK and manual and not held:
                rc = L.mcrx_hip_rfcal_update(cal._h, sp)
            if rc != prod.MCRX_OK:
                raise RuntimeError("mcrx_hip_rfcal call failed (%d): %s" % (rc, L.mcrx_hip_rfcal_last_error().decode()))
        nbytes = (4 if cal.input_format else 8) + ((4 if cal.output_format else 8) if writes else 0)
        out["legs"][name] = report(n, nbytes, measure(call))
        st = cal.read(stream=side)
        out["legs"][name].update(updates=st["updates"], irr_db=round(st["irr_db"], 2) if st["irr_db"] != float("inf") else None,
                                 launches_per_call=(1 if held else 2 * len(prod.rfcal_segments(cal.config, 0, n)[0]) + (1 if manual else 0)))
        if writes and cal.output_format:
            out["legs"][name]["clipped_per_call"] = cal.clipped() // (args.warmup + args.steps * args.reps)
        cal.close()
    legs_ = out["legs"]
    out["separate_ms"] = round(legs_["measure_cf32"]["ms"] + legs_["apply_only"]["ms"], 4)
    out["fused_over_separate"] = round(legs_["fused"]["ms"] / out["separate_ms"], 4)
    out["apply_only_over_floor"] = round(legs_["apply_only"]["ms"] / legs_["rfchain_none"]["ms"], 4)
    out["fused_over_floor"] = round(legs_["fused"]["ms"] / legs_["rfchain_none"]["ms"], 4)

    w = mix["beta"] / mix["alpha"].conjugate()

    def torch_composed():
        s1 = d_x.sum(dtype=torch.complex128)
        s2 = (d_x * d_x).sum(dtype=torch.complex128)
        p = (d_x.real * d_x.real + d_x.imag * d_x.imag).sum(dtype=torch.float64)
        t = d_x - (0.01 + 0.005j)
        return t - w * t.conj(), s1, s2, p
    out["legs"]["torch_composed"] = report(n, 16, measure(torch_composed))
    out["legs"]["copy_d2d_again"] = report(n, 16, measure(copy))
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
