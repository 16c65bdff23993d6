#!/usr/bin/env python3
"""What 16-bit integer IQ out of the resampler (msresamp_hip_set_output_format = 1, sc16) is worth against cf32.  A secondary
measurement, bench_resamp_sc16.py's sibling -- bench.py holds the headline metric.

    python bench_resamp_sc16_out.py [--samples N --steps K --warmup W --reps R --rates ... --out FILE]

Rates: 2.0 and 1.5 (the arbitrary stage is last, interpolating), 4.0 (the half-band interpolator is last), 0.5 and 0.8 (decimating).
The same 77.9 M cf32 input samples (bench_resamp_sc16.py's) through a cf32-output and an sc16-output handle of one process, gain 1,
alternating rep by rep; medians of --reps repetitions of --steps calls:
(a) the whole execute (HIP events around --steps calls on a side stream);
(b) the cf32 execute plus the torch pass sc16 output replaces (round(v * 32768), clamp, cast to int16), against the sc16 execute;
(c) execute plus a copy of its output to pinned host memory, wall clock: the host link carries half the bytes;
(d) at r = 2.0 also int16 in AND out (input_format = output_format = sc16) against cf32 on both sides, the whole execute, with the
    algorithmic bytes per input sample of each case -- the input read once, the output written once.
The calls go through the C-ABI into output buffers allocated beforehand: msresamp.execute allocates its output, and outputs of 8 and
of 4 bytes a sample, alternating, make torch's caching allocator split and re-request blocks inside the timed region (a spread of
16 - 25 % when this was tried).
Every median comes with the spread (max - min) / median of its repetitions: a ratio says something only where it leaves 1 by more
than the cf32 build's own spread (`beyond_cf32_spread`).  One JSON line; --out also writes it to a file."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
FORMATS = ("cf32", "sc16")
BYTES = {"cf32": 8, "sc16": 4}
RATES = (2.0, 1.5, 4.0, 0.5, 0.8)


def last_stage(rate):
    if rate > 2.0:
        return "halfband_interp_kernel"
    if rate > 1.0:
        return "arbitrary_kernel (interpolating)"
    return "arbitrary_kernel" if rate >= 0.5 else "arbitrary_kernel, half-band folded in"


def summary(ms):
    med = {f: statistics.median(ms[f]) for f in FORMATS}
    out = {"ms": {f: round(med[f], 4) for f in FORMATS}, "reps_ms": {f: [round(v, 4) for v in ms[f]] for f in FORMATS},
           "spread": {f: round((max(ms[f]) - min(ms[f])) / med[f], 4) for f in FORMATS},
           "sc16_over_cf32": round(med["sc16"] / med["cf32"], 4)}
    out["beyond_cf32_spread"] = bool(abs(out["sc16_over_cf32"] - 1.0) > out["spread"]["cf32"])
    return out


def measure(fn, steps, warmup, reps):
    for f in FORMATS:
        fn(f, warmup)
    ms = {f: [] for f in FORMATS}
    for _ in range(reps):
        for f in FORMATS:
            ms[f].append(fn(f, steps))
    return summary(ms)


def leg(prod, torch, dev, rate, d_x, d_q, steps, warmup, reps):
    n = int(d_x.numel())
    L = prod.lib()
    rs = {f: prod.msresamp(rate, output_format=f) for f in FORMATS}
    side = torch.cuda.Stream(device=dev)
    cap = int(L.msresamp_hip_max_output(rs["cf32"]._h, n)) + 8
    nbuf = max(steps, warmup)
    bufs = {"cf32": [torch.empty(cap, dtype=torch.complex64, device=dev) for _ in range(nbuf)],
            "sc16": [torch.empty((cap, 2), dtype=torch.int16, device=dev) for _ in range(nbuf)]}

    def execute(h, src, dst):
        """one call of the C-ABI on the side stream: the first *nout samples of dst"""
        fn = L.msresamp_hip_execute_device_sc16 if src.dtype == torch.int16 else L.msresamp_hip_execute_device
        nout = C.c_size_t(0)
        rc = fn(h._h, C.c_void_p(src.data_ptr()), n, C.c_void_p(dst.data_ptr()), cap, C.byref(nout), C.c_void_p(side.cuda_stream))
        if rc != prod.MCRX_OK:
            raise RuntimeError("msresamp_hip_execute_device failed (%d): %s" % (rc, L.msresamp_hip_last_error().decode()))
        return dst[:nout.value]
    out = {"rate": rate, "last_stage": last_stage(rate), "input_samples": n, "steps": steps, "reps": reps,
           "algorithmic_bytes_per_input_sample": {"cf32_in_cf32_out": round(8 + 8 * rate, 3), "cf32_in_sc16_out": round(8 + 4 * rate, 3)}}

    def quantise(y):            # the pass a caller with a 16-bit radio runs behind a cf32 resampler
        return torch.clamp(torch.round(torch.view_as_real(y) * 32768.0), -32768.0, 32767.0).to(torch.int16)

    def timed(handles, src, post):
        def fn(f, k):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(side):
                ys = []
                handles[f].reset()
                a.record(side)
                for i in range(k):
                    y = execute(handles[f], src[f], bufs[f][i])
                    ys.append(quantise(y) if post and f == "cf32" else y)
                b.record(side)
            torch.cuda.synchronize()
            del ys, y
            return a.elapsed_time(b) / k
        return fn

    x_in = {f: d_x for f in FORMATS}
    out["execute"] = measure(timed(rs, x_in, False), steps, warmup, reps)
    out["execute"]["output_gsamples_per_s"] = {f: round(rate * n / out["execute"]["ms"][f] / 1e6, 2) for f in FORMATS}
    out["execute_and_quantise"] = measure(timed(rs, x_in, True), steps, warmup, reps)

    # (c) execute + device -> pinned host copy of the output
    rs["cf32"].reset()          # (every call below starts a stream anew, so that all of them make nout samples)
    nout = int(execute(rs["cf32"], d_x, bufs["cf32"][0]).shape[0])
    host = {"cf32": torch.empty(nout, dtype=torch.complex64).pin_memory(), "sc16": torch.empty((nout, 2), dtype=torch.int16).pin_memory()}

    def linked(f, k):
        rs[f].reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(side):
            for i in range(k):
                host[f].copy_(execute(rs[f], d_x, bufs[f][i]), non_blocking=True)
                rs[f].reset()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k

    out["execute_and_host_copy"] = measure(linked, steps, warmup, reps)
    out["execute_and_host_copy"]["host_link_gbytes_per_s"] = {
        f: round(BYTES[f] * nout / out["execute_and_host_copy"]["ms"][f] / 1e6, 2) for f in FORMATS}
    del host

    if rate == 2.0:             # (d) int16 on both sides
        both = {"cf32": rs["cf32"], "sc16": prod.msresamp(rate, input_format="sc16", output_format="sc16")}
        out["execute_sc16_in_and_out"] = measure(timed(both, {"cf32": d_x, "sc16": d_q}, False), steps, warmup, reps)
        out["algorithmic_bytes_per_input_sample"]["sc16_in_sc16_out"] = round(4 + 4 * rate, 3)
        both["sc16"].close()
    for q in rs.values():
        q.close()
    del bufs
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=77900000)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rates", type=str, default=",".join(str(r) for r in RATES))
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "resamp_sc16_out.json"))
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
    out = {"metric": "sc16 against cf32 output of msresamp", "device": torch.cuda.get_device_name(0), "legs": []}
    for r in (float(v) for v in args.rates.split(",")):
        out["legs"].append(leg(prod, torch, dev, r, d_x, d_q, args.steps, args.warmup, args.reps))
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
