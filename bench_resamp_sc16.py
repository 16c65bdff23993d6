#!/usr/bin/env python3
"""What 16-bit integer IQ into the resampler (msresamp_hip_set_input_format = 1, sc16) is worth against cf32.  A secondary
measurement, bench_sc16.py's sibling -- bench.py holds the headline metric.

    python bench_resamp_sc16.py [--samples N --steps K --warmup W --reps R --out FILE]

One rate per first-stage kernel build, and the interpolating case: r = 0.5 and 0.8 (arbitrary stage, one branch per thread), 0.37
(arbitrary stage with a table and the half-band decimator folded in), 0.2 and 0.06 (halfband_kernel in front), 2.0 (interpolating).
The same 77.9 M input samples (profiles/r6_resamp_roofline.csv's) as int16 and as exactly the dequantised floats, through a cf32 and
an sc16 handle of one process, alternating rep by rep; medians of --reps repetitions of --steps calls:
(a) the first-stage kernel alone (HIP events around its launch, msresamp_hip_time_first_stage): its algorithmic bytes -- the input
    read once, the output written once -- and what fraction of the 8 TB/s HBM peak they make;
(b) the whole execute (HIP events around --steps calls on a side stream);
(c) a copy from pinned host memory to the device + execute, wall clock: the host link carries half the bytes.
Every median comes with the spread (max - min) / median of its repetitions: an sc16 figure is slower than the cf32 one only where the
ratio exceeds 1 by more than the cf32 build's own spread (`sc16_slower_beyond_cf32_spread`).  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0
FORMATS = ("cf32", "sc16")
IN_BYTES = {"cf32": 8, "sc16": 4}
RATES = (0.5, 0.8, 0.37, 0.2, 0.06, 2.0)


def first_stage(rate):
    """(kernel, output bytes of the first stage per input sample)"""
    if rate > 1.0:
        return "arbitrary_kernel (interpolating)", 8.0 * min(rate, 2.0)
    if rate >= 0.5:
        return "arbitrary_kernel", 8.0 * rate
    if rate >= 0.25:
        return "arbitrary_kernel, half-band folded in", 8.0 * rate
    return "halfband_kernel", 4.0


def summary(ms):
    med = {f: statistics.median(ms[f]) for f in FORMATS}
    out = {"ms": {f: round(med[f], 4) for f in FORMATS},
           "spread": {f: round((max(ms[f]) - min(ms[f])) / med[f], 4) for f in FORMATS},
           "sc16_over_cf32": round(med["sc16"] / med["cf32"], 4)}
    out["sc16_slower_beyond_cf32_spread"] = bool(out["sc16_over_cf32"] > 1.0 + out["spread"]["cf32"])
    return out, med


def leg(prod, torch, dev, rate, d_q, d_x, h_q, h_x, steps, warmup, reps):
    n = int(d_x.numel())
    dev_in, host_in = {"cf32": d_x, "sc16": d_q}, {"cf32": h_x, "sc16": h_q}
    rs = {f: prod.msresamp(rate, input_format=f) for f in FORMATS}
    side = torch.cuda.Stream(device=dev)
    kernel, out_bytes = first_stage(rate)
    out = {"rate": rate, "first_stage": kernel, "input_samples": n, "steps": steps, "reps": reps}

    # (a) the first stage alone
    def first(f, k):
        rs[f].time_first_stage(True)
        tot = 0.0
        with torch.cuda.stream(side):
            for _ in range(k):
                rs[f].reset()
                y = rs[f].execute(dev_in[f], stream=side)
                tot += rs[f].first_stage_ms()
                del y
        rs[f].time_first_stage(False)
        return tot / k

    # (b) the whole execute
    def whole(f, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            ys = []
            rs[f].reset()
            a.record(side)
            for _ in range(k):
                ys.append(rs[f].execute(dev_in[f], stream=side))
            b.record(side)
        torch.cuda.synchronize()
        del ys
        return a.elapsed_time(b) / k

    # (c) pinned host -> device + execute
    stage = {f: torch.empty_like(dev_in[f]) for f in FORMATS}

    def linked(f, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(side):
            for _ in range(k):
                stage[f].copy_(host_in[f], non_blocking=True)
                y = rs[f].execute(stage[f], stream=side)
        torch.cuda.synchronize()
        del y
        return (time.perf_counter() - t0) * 1e3 / k

    for name, fn in (("first_stage", first), ("execute", whole), ("host_copy_and_execute", linked)):
        for f in FORMATS:
            rs[f].reset()
            fn(f, warmup)
        ms = {f: [] for f in FORMATS}
        for _ in range(reps):
            for f in FORMATS:
                ms[f].append(fn(f, steps))
        out[name], med = summary(ms)
        if name == "first_stage":
            byts = {f: (IN_BYTES[f] + out_bytes) * n for f in FORMATS}
            out[name]["algorithmic_bytes_per_input_sample"] = {f: round(IN_BYTES[f] + out_bytes, 3) for f in FORMATS}
            out[name]["gbytes_per_s"] = {f: round(byts[f] / med[f] / 1e6, 1) for f in FORMATS}
            out[name]["frac_of_hbm_peak"] = {f: round(byts[f] / med[f] / 1e6 / HBM_PEAK_GBS, 4) for f in FORMATS}
        elif name == "execute":
            out[name]["input_gsamples_per_s"] = {f: round(n / med[f] / 1e6, 2) for f in FORMATS}
        else:
            out[name]["host_link_gbytes_per_s"] = {f: round(IN_BYTES[f] * n / med[f] / 1e6, 2) for f in FORMATS}
    for q in rs.values():
        q.close()
    del stage
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=77900000)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rates", type=str, default=",".join(str(r) for r in RATES))
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_product
    prod = load_product()
    dev = torch.device("cuda", 0)
    n = args.samples
    gen = torch.Generator(device=dev)
    gen.manual_seed(16)
    # a quarter of full scale rms: noise clipped to the int16 range (the kernels' time does not depend on the values)
    d_q = torch.clamp(torch.round(torch.randn(2 * n, generator=gen, device=dev) * 8192.0), -32768.0, 32767.0).to(torch.int16)
    d_x = torch.view_as_complex((d_q.to(torch.float32) * 2.0 ** -15).reshape(-1, 2)).contiguous()
    h_q, h_x = d_q.cpu().pin_memory(), d_x.cpu().pin_memory()
    out = {"metric": "sc16 against cf32 input of msresamp", "device": torch.cuda.get_device_name(0), "legs": []}
    for r in (float(v) for v in args.rates.split(",")):
        out["legs"].append(leg(prod, torch, dev, r, d_q, d_x, h_q, h_x, args.steps, args.warmup, args.reps))
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
