#!/usr/bin/env python3
"""What the channel emulator (mcrx_hip_chanemu_*, csrc/chanemu.hip) costs on the wideband stream.  A secondary measurement --
bench.py holds the headline metric.

    python bench_chanemu.py [--samples N --steps K --warmup W --reps R --rms LEVEL --out FILE]

One slab of --samples cf32 samples (default: the 512-channel slab, 207.7 M) through emulators of one process, into output buffers
allocated beforehand, through the C-ABI on a side stream, HIP events around --steps calls; the median of --reps repetitions with
its spread (max - min) / median.  Legs:
    T1                one tap, no rotation, no noise: the copy bound (8 B in + 8 B out a sample)
    T3, T8            three / eight rays: the same algorithmic bytes, the tap reads are served from cache
    T3_cfo_awgn       three rays, carrier offset, noise, cf32 out
    T3_cfo_awgn_sc16  ... to sc16 (8 B in + 4 B out)
    torch_awgn        v + nstd * randn(v.shape), the expression of bench.py's noisy leg that the emulator replaces
    torch_3ray        a three-term sum of shifted slices, a0 x[n] + a1 x[n - d1] + a2 x[n - d2]
Every leg reports ms a call, its algorithmic GB and that traffic as a fraction of 8 TB/s (HBM peak).  The torch expressions move more
than their algorithmic bytes (temporaries); the fraction says what a caller gets, not how busy the memory is.
One JSON line; --out also writes it to a file.  Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8.0e12


def report(n, out_bytes, ms):
    med = statistics.median(ms)
    gb = n * (8 + out_bytes) / 1e9
    return {"ms": round(med, 4), "reps_ms": [round(v, 4) for v in ms], "spread": round((max(ms) - min(ms)) / med, 4),
            "algorithmic_gb": round(gb, 4), "gsamples_per_s": round(n / med / 1e6, 2),
            "fraction_of_8_tb_per_s": round(gb * 1e9 / (med * 1e-3) / PEAK_BYTES_PER_S, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=207700000)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rms", type=float, default=0.1, help="level of the input per component against the full scale 1.0 (0.1: no sample "
                    "clips; a clipping wave adds to the handle's counter with one atomic, and many of them queue on its one address)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "chanemu.json"))
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_product
    assert torch.cuda.is_available(), "bench_chanemu.py needs the GPU"
    prod = load_product()
    L = prod.lib()
    dev = torch.device("cuda", 0)
    n, K = args.samples, 1024
    gen = torch.Generator(device=dev)
    gen.manual_seed(16)
    d_x = torch.view_as_complex(torch.randn((n, 2), generator=gen, device=dev) * args.rms)
    d_f = torch.empty(n, dtype=torch.complex64, device=dev)
    d_i = torch.empty((n, 2), dtype=torch.int16, device=dev)
    side = torch.cuda.Stream(device=dev)
    rays3 = [(0, 1.0), (K + 3, 0.35 - 0.2j), (3 * K, -0.15 + 0.2j)]
    rays8 = rays3 + [(1, 0.1 + 0.1j), (37, -0.05 + 0.2j), (4099, 0.1 - 0.1j), (20000, 0.05j), (65535, -0.05)]
    step, nstd = prod.chanemu_cfo_step(0.3, 64, K // 2), args.rms * 10.0 ** (-30.0 / 20.0)
    legs = [("T1", dict(taps=[(0, 1.0)])), ("T3", dict(taps=rays3)), ("T8", dict(taps=rays8)),
            ("T3_cfo_awgn", dict(taps=rays3, cfo_step=step, noise_std=nstd, seed=1)),
            ("T3_cfo_awgn_sc16", dict(taps=rays3, cfo_step=step, noise_std=nstd, seed=1, output_format="sc16"))]

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

    out = {"metric": "channel emulator on the wideband stream", "device": torch.cuda.get_device_name(0), "samples": n, "rms": args.rms,
           "steps": args.steps, "reps": args.reps, "legs": {}}
    for name, cfg in legs:
        ce = prod.chanemu(**cfg)
        dst = d_i if ce.output_format else d_f

        def call(ce=ce, dst=dst):
            rc = L.mcrx_hip_chanemu_execute_device(ce._h, C.c_void_p(d_x.data_ptr()), n, C.c_void_p(dst.data_ptr()), C.c_void_p(side.cuda_stream))
            if rc != prod.MCRX_OK:
                raise RuntimeError("mcrx_hip_chanemu_execute_device failed (%d): %s" % (rc, L.mcrx_hip_chanemu_last_error().decode()))
        out["legs"][name] = report(n, 4 if ce.output_format else 8, measure(call))
        out["legs"][name]["taps"] = len(cfg["taps"])
        if ce.output_format:
            out["legs"][name]["clipped_per_call"] = ce.clipped() // (args.warmup + args.steps * args.reps)
        ce.close()

    v = torch.view_as_real(d_x)
    tgen = torch.Generator(device=dev)
    tgen.manual_seed(1)

    def torch_awgn():
        return torch.view_as_complex(v + nstd * torch.randn(v.shape, generator=tgen, device=dev, dtype=v.dtype))

    (d1, a1), (d2, a2) = rays3[1:]

    def torch_3ray():
        y = d_x.clone()
        y[d1:] += a1 * d_x[:n - d1]
        y[d2:] += a2 * d_x[:n - d2]
        return y
    for name, fn in (("torch_awgn", torch_awgn), ("torch_3ray", torch_3ray)):
        out["legs"][name] = report(n, 8, measure(fn))
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
