#!/usr/bin/env python3
"""What the RF front end (mcrx_hip_rfchain_*, csrc/rfchain.hip) costs on the wideband stream.  A secondary measurement -- bench.py
holds the headline metric.

    python bench_rfchain.py [--samples N --steps K --warmup W --reps R --rms LEVEL --out FILE]

One slab of --samples samples (default: the 512-channel slab, 207.7 M) through front ends of one process, into output buffers
allocated beforehand, through the C-ABI on a side stream, HIP events around --steps calls; the median of --reps repetitions with
its spread (max - min) / median.  Legs:
    copy_d2d          hipMemcpyAsync device to device of the same 8 B a sample, timed in the same session: the bound
    none              no stage on, cf32 to cf32 (8 B in + 8 B out a sample): load, store
    mixer, oscillator, amplifier      each stage alone (oscillator: L = 10; amplifier: p = 2 with AM/PM)
    all               the three stages, transmitter order
    all_sc16          ... sc16 in and sc16 out (4 B + 4 B)
    oscillator_L6     the oscillator alone with a grid of 64 samples: 16 times the table rows and 13 spans a call
    torch_chain       the same three stages as torch expressions on the slab, the angle theta(n) handed over precomputed
Every leg reports ms a call, its algorithmic GB and that traffic as a fraction of 8 TB/s (HBM peak).  The torch expressions move more
than their algorithmic bytes (temporaries); the fraction says what a caller gets, not how busy the memory is.
One JSON line; --out also writes it to a file.  Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import math
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
    ap.add_argument("--rms", type=float, default=0.1, help="level of the input per component against the full scale 1.0 (0.1: no sample "
                    "clips; a clipping wave adds to the handle's counter with one atomic, and many of them queue on its one address)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "rfchain.json"))
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_product
    assert torch.cuda.is_available(), "bench_rfchain.py needs the GPU"
    prod = load_product()
    L = prod.lib()
    dev = torch.device("cuda", 0)
    n = args.samples
    gen = torch.Generator(device=dev)
    gen.manual_seed(16)
    d_x = torch.view_as_complex(torch.randn((n, 2), generator=gen, device=dev) * args.rms)
    d_f = torch.empty(n, dtype=torch.complex64, device=dev)
    d_i = torch.empty((n, 2), dtype=torch.int16, device=dev)
    side = torch.cuda.Stream(device=dev)
    conv = prod.rfchain(output_format="sc16")                          # the sc16 leg's input: Q of the slab
    d_xi = conv.execute(d_x).clone()
    conv.close()
    torch.cuda.synchronize()
    mixer = dict(prod.rfchain_iq(0.5, 3.0, "tx"), dc=0.001 + 0.001j)
    pn10 = dict(rms_deg=1.0, bandwidth=1e-5, log2_block=10, seed=1)
    pn6 = dict(pn10, log2_block=6)
    amp = dict(sat=prod.rfchain_backoff(8.0, args.rms * math.sqrt(2.0)), smooth=2, ampm_deg=5.0)
    legs = [("none", dict()), ("mixer", dict(mixer=mixer)), ("oscillator", dict(phase_noise=pn10)), ("amplifier", dict(amplifier=amp)),
            ("all", dict(mixer=mixer, phase_noise=pn10, amplifier=amp)),
            ("all_sc16", dict(mixer=mixer, phase_noise=pn10, amplifier=amp, input_format="sc16", output_format="sc16")),
            ("oscillator_L6", dict(phase_noise=pn6))]

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

    out = {"metric": "RF front end on the wideband stream", "device": torch.cuda.get_device_name(0), "samples": n, "rms": args.rms,
           "steps": args.steps, "reps": args.reps, "legs": {}}

    def copy():
        d_f.copy_(d_x, non_blocking=True)                               # (contiguous, same dtype and device: hipMemcpyAsync device to device)
    out["legs"]["copy_d2d"] = report(n, 16, measure(copy))
    for name, cfg in legs:
        rf = prod.rfchain(**cfg)
        src = d_xi if rf.input_format else d_x
        dst = d_i if rf.output_format else d_f

        def call(rf=rf, src=src, dst=dst):
            rc = L.mcrx_hip_rfchain_execute_device(rf._h, C.c_void_p(src.data_ptr()), 0, n, C.c_void_p(dst.data_ptr()), C.c_void_p(side.cuda_stream))
            if rc != prod.MCRX_OK:
                raise RuntimeError("mcrx_hip_rfchain_execute_device failed (%d): %s" % (rc, L.mcrx_hip_rfchain_last_error().decode()))
        out["legs"][name] = report(n, (4 if rf.input_format else 8) + (4 if rf.output_format else 8), measure(call))
        out["legs"][name]["stages"] = rf.stages
        if rf.output_format:
            out["legs"][name]["clipped_per_call"] = rf.clipped() // (args.warmup + args.steps * args.reps)
        rf.close()
    out["legs"]["copy_d2d_again"] = report(n, 16, measure(copy))

    # the same chain as torch expressions; theta(n) in radians is handed over (a caller would have to make it as well)
    cfg = prod.rfchain_config(mixer=mixer, phase_noise=pn10, amplifier=amp)
    al, be, dc = complex(cfg.alpha_re, cfg.alpha_im), complex(cfg.beta_re, cfg.beta_im), complex(cfg.dc_re, cfg.dc_im)
    r, g, am = 1.0 / (cfg.amp_sat * cfg.amp_sat), cfg.amp_gain, 2.0 * math.pi * cfg.amp_ampm
    rf = prod.rfchain(phase_noise=pn10)
    rows = rf.phase_rows(0, (n >> 10) + 2)
    rf.close()
    frac = (torch.arange(n, device=dev, dtype=torch.int32) & 1023).to(torch.float32) / 1024.0
    idx = torch.arange(n, device=dev, dtype=torch.int64) >> 10
    theta = (rows[idx] + frac * (rows[idx + 1] - rows[idx])) * (2.0 * math.pi)
    del frac, idx

    def torch_chain():
        z = al * d_x + be * d_x.conj() + dc
        z = z * torch.polar(torch.ones_like(theta), theta)
        t = (z.real * z.real + z.imag * z.imag) * r
        z = z * torch.polar(g / torch.sqrt(torch.sqrt(1.0 + t * t)), am * t / (1.0 + t))
        return z
    out["legs"]["torch_chain"] = report(n, 16, measure(torch_chain))
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
