#!/usr/bin/env python3
"""What fading rays (mcrx_hip_chanfade_*, csrc/chanemu.hip) cost on the wideband stream, next to the static
emulator's legs of bench_chanemu.py.  A secondary measurement -- bench.py holds the headline metric.

    python bench_chanemu_fading.py [--samples N --steps K --warmup W --reps R --rms LEVEL --static-only --out FILE]

The shape of bench_chanemu.py: one slab of --samples cf32 samples (default: the 512-channel slab, 207.7 M), output buffers allocated
beforehand, C-ABI calls on a side stream, HIP events around --steps calls, the median of --reps repetitions with its spread.  Legs:
    T1, T3, T8, T3_cfo_awgn_sc16      the static emulator (fading off).  --static-only stops here and needs nothing of the fading
                                      interface: run it on the commit before fading to see that nothing existing moved
    T3_fade_L10, T3_fade_L6, T8_...   three / eight fading rays (S = 16 sinusoids each), gains updated every 2^10 / 2^6 samples, cf32 out
    ..._sc16                          the same to sc16
    gain_T8_L6                        the gain kernel alone: the rows the slab needs at L = 6, eight rays, into a buffer of the caller's
Every fading leg also reports its time over the static leg of the same ray count, per ray.  One JSON line; --out also writes it to a file.
Needs the GPU: there is no fallback."""
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
    ap.add_argument("--rms", type=float, default=0.1, help="level of the input per component against the full scale 1.0 (no sample clips)")
    ap.add_argument("--static-only", action="store_true", help="the static legs only (runs on a library without the fading interface)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "chanemu_fading.json"))
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_product
    assert torch.cuda.is_available(), "bench_chanemu_fading.py needs the GPU"
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
            ("T3_cfo_awgn_sc16", dict(taps=rays3, cfo_step=step, noise_std=nstd, seed=1, output_format="sc16"))]
    if not args.static_only:
        for T, rays in ((3, rays3), (8, rays8)):
            for Lb in (10, 6):
                for fmt in ("cf32", "sc16"):
                    fading = dict(doppler=prod.chanemu_doppler(0.02, 64, 8, K // 2), rice_k=[4.0] + [0.0] * (T - 1), sinusoids=16,
                                  log2_block=Lb, seed=5)
                    legs.append(("T%d_fade_L%d%s" % (T, Lb, "_sc16" if fmt == "sc16" else ""), dict(taps=rays, output_format=fmt, fading=fading)))

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

    out = {"metric": "channel emulator with fading rays on the wideband stream", "device": torch.cuda.get_device_name(0), "samples": n,
           "rms": args.rms, "steps": args.steps, "reps": args.reps, "static_only": bool(args.static_only), "legs": {}}
    for name, cfg in legs:
        ce = prod.chanemu(**cfg)
        dst = d_i if ce.output_format else d_f

        def call(ce=ce, dst=dst):
            rc = L.mcrx_hip_chanemu_execute_device(ce._h, C.c_void_p(d_x.data_ptr()), n, C.c_void_p(dst.data_ptr()), C.c_void_p(side.cuda_stream))
            if rc != prod.MCRX_OK:
                raise RuntimeError("mcrx_hip_chanemu_execute_device failed (%d): %s" % (rc, L.mcrx_hip_chanemu_last_error().decode()))
        leg = out["legs"][name] = report(n, 4 if ce.output_format else 8, measure(call))
        leg["taps"] = len(cfg["taps"])
        if ce.output_format:
            leg["clipped_per_call"] = ce.clipped() // (args.warmup + args.steps * args.reps)
        if "fading" in cfg:
            leg["log2_block"] = cfg["fading"]["log2_block"]
            if not ce.output_format:
                leg["ms_over_static_per_ray"] = round((leg["ms"] - out["legs"]["T%d" % leg["taps"]]["ms"]) / leg["taps"], 4)
        ce.close()
    if not args.static_only:
        Lb = 6
        rows = (n >> Lb) + 2
        ce = prod.chanemu(taps=rays8, fading=dict(doppler=prod.chanemu_doppler(0.02, 64, 8, K // 2), sinusoids=16, log2_block=Lb, seed=5))
        d_g = torch.empty((rows, 8), dtype=torch.complex64, device=dev)

        def gains():
            rc = L.mcrx_hip_chanfade_gains(ce._h, 0, rows, C.c_void_p(d_g.data_ptr()), C.c_void_p(side.cuda_stream))
            if rc != prod.MCRX_OK:
                raise RuntimeError("mcrx_hip_chanfade_gains failed (%d): %s" % (rc, L.mcrx_hip_chanemu_last_error().decode()))
        ms = measure(gains)
        med = statistics.median(ms)
        out["legs"]["gain_T8_L6"] = {"ms": round(med, 4), "reps_ms": [round(v, 4) for v in ms], "spread": round((max(ms) - min(ms)) / med, 4),
                                     "rows": rows, "rays": 8, "sinusoids": 16, "ns_per_row_and_ray": round(med * 1e6 / (rows * 8), 4)}
        ce.close()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
