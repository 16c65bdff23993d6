#!/usr/bin/env python3
"""What the crest-factor reduction (mcrx_hip_cfr_*, csrc/cfr.hip) costs on the wideband stream.  A secondary measurement -- bench.py
holds the headline metric.

    python bench_cfr.py [--samples N --steps K --warmup W --reps R --rms LEVEL --out FILE]

One slab of --samples output samples (default: the 512-channel slab, 207.7 M) of Gaussian noise, with the halos of the widest leg
around it, through handles of one process, into output buffers allocated beforehand, through the C-ABI on a side stream, HIP events
around --steps calls; the median of --reps repetitions with its spread (max - min) / median.  Legs:
    copy_d2d          hipMemcpyAsync device to device of the same 8 B a sample, timed in the same session
    rfchain_none      the RF front end with no stage on, cf32 to cf32: the streaming floor of this project's operators
    no_clipping       the threshold above every sample, H = 31, one pass: every wave copies -- the floor of this operator
    p1, p2, p3        the threshold 7 dB over the rms, H = 31, one, two and three passes
    h63               ... H = 63, one pass
    sc16              ... H = 31, one pass, sc16 out (8 B in + 4 B out a sample)
    torch_conv1d      one pass as torch expressions and conv1d, on --torch-samples samples (default: an eighth of the slab)
Every leg reports ms a call, its algorithmic GB (the bytes one pass has to move: the passes between the first and the last move
theirs through the scratch buffers on top of that, which the figure does not count) and that traffic as a fraction of 8 TB/s (HBM
peak).  `windows_above`: the share of the waves' windows (512 outputs and H on either side) that hold a sample above the threshold,
counted from the input with torch: the waves that must run the filter (the kernel decides in units of eight samples, so it runs a few
more).  One JSON line; --out also writes it to a file.  Needs the GPU: there is no fallback."""
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
    ap.add_argument("--torch-samples", type=int, default=0, help="samples of the torch leg (0: an eighth of --samples)")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rms", type=float, default=0.1, help="level of the input per component against the full scale 1.0")
    ap.add_argument("--papr-db", type=float, default=7.0, help="the threshold of the clipping legs over the rms of the input")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "cfr.json"))
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_product
    assert torch.cuda.is_available(), "bench_cfr.py needs the GPU"
    prod = load_product()
    L = prod.lib()
    dev = torch.device("cuda", 0)
    n = args.samples
    reach = 3 * 31                                                      # the widest halo of the legs (three passes of H = 31; H = 63 once)
    gen = torch.Generator(device=dev)
    gen.manual_seed(16)
    d_x = torch.view_as_complex(torch.randn((n + 2 * reach, 2), generator=gen, device=dev) * args.rms)
    d_f = torch.empty(n, dtype=torch.complex64, device=dev)
    d_i = torch.empty((n, 2), dtype=torch.int16, device=dev)
    side = torch.cuda.Stream(device=dev)
    rms = args.rms * math.sqrt(2.0)
    A = prod.cfr_threshold(args.papr_db, rms)
    legs = [("no_clipping", dict(threshold=1e3, half_len=31)), ("p1", dict(threshold=A, half_len=31)),
            ("p2", dict(threshold=A, half_len=31, passes=2)), ("p3", dict(threshold=A, half_len=31, passes=3)),
            ("h63", dict(threshold=A, half_len=63)), ("sc16", dict(threshold=A, half_len=31, output_format="sc16"))]

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

    out = {"metric": "crest-factor reduction on the wideband stream", "device": torch.cuda.get_device_name(0), "samples": n,
           "rms": args.rms, "papr_db": args.papr_db, "threshold": A, "steps": args.steps, "reps": args.reps, "legs": {}}

    def copy():
        d_f.copy_(d_x[:n], non_blocking=True)                           # (contiguous, same dtype and device: hipMemcpyAsync device to device)
    out["legs"]["copy_d2d"] = report(n, 16, measure(copy))
    rf = prod.rfchain()

    def floor():
        rc = L.mcrx_hip_rfchain_execute_device(rf._h, C.c_void_p(d_x.data_ptr()), 0, n, C.c_void_p(d_f.data_ptr()), C.c_void_p(side.cuda_stream))
        if rc != prod.MCRX_OK:
            raise RuntimeError("mcrx_hip_rfchain_execute_device failed (%d)" % rc)
    out["legs"]["rfchain_none"] = report(n, 16, measure(floor))
    for name, cfg in legs:
        cf = prod.cfr(**cfg)
        dst = d_i if cf.output_format else d_f
        src = d_x[reach - cf.halo:]                                     # the slab's n samples with this leg's halos

        def call(cf=cf, src=src, dst=dst):
            rc = L.mcrx_hip_cfr_execute_device(cf._h, C.c_void_p(src.data_ptr()), n, C.c_void_p(dst.data_ptr()), C.c_void_p(side.cuda_stream))
            if rc != prod.MCRX_OK:
                raise RuntimeError("mcrx_hip_cfr_execute_device failed (%d): %s" % (rc, L.mcrx_hip_cfr_last_error().decode()))
        cf.stats(reset=True)
        leg = report(n, 8 + (4 if cf.output_format else 8), measure(call))
        calls = args.warmup + args.steps * args.reps
        over, peak2 = cf.stats()
        leg.update(half_len=cf.half_len, passes=cf.passes, over_per_call=[v // calls for v in over], peak_over_threshold=round(math.sqrt(peak2) / cfg["threshold"], 4))
        if cf.output_format:
            leg["clipped_per_call"] = cf.clipped() // calls
        # the waves that must run the filter, first pass: windows of 512 outputs and H on either side with a sample above the threshold
        H = cf.half_len
        first = src[:n + 2 * cf.halo]
        above = torch.zeros(first.numel() + 1, dtype=torch.int32, device=dev)
        torch.cumsum((torch.view_as_real(first).pow(2).sum(dim=1) > cf.config.threshold ** 2).to(torch.int32), 0, out=above[1:])
        m = first.numel() - 2 * H
        lo = torch.arange(0, m, 512, device=dev)
        hi = torch.clamp(lo + 512 + 2 * H, max=first.numel())
        leg["windows_above"] = round(float((above[hi] - above[lo] > 0).double().mean()), 4)
        del above, lo, hi
        out["legs"][name] = leg
        cf.close()
    out["legs"]["rfchain_none_again"] = report(n, 16, measure(floor))
    rf.close()
    out["legs"]["copy_d2d_again"] = report(n, 16, measure(copy))

    # one pass as torch expressions: e where |x|^2 > A^2, conv1d over re and im as two channels, the subtraction
    nt = args.torch_samples or n // 8
    H = 31
    h = torch.from_numpy(prod.cfr_lowpass(H, 0.28, 5.65)).to(dev)
    kernel = torch.cat([h.flip(0)[:-1], h]).view(1, 1, -1).repeat(2, 1, 1)
    x_t = d_x[:nt + 2 * H]

    def torch_pass():
        t = x_t.real * x_t.real + x_t.imag * x_t.imag
        s = torch.where(t > A * A, 1.0 - A / torch.sqrt(t), torch.zeros_like(t))
        e = torch.view_as_real(x_t * s).t().unsqueeze(0)                # [1, 2, samples]
        c = torch.nn.functional.conv1d(e, kernel, groups=2)[0]
        return x_t[H:H + nt] - torch.complex(c[0], c[1])
    try:
        out["legs"]["torch_conv1d"] = report(nt, 16, measure(torch_pass))
        out["legs"]["torch_conv1d"]["samples"] = nt
    except Exception as err:                                            # (for scale only: a failure of torch's convolution is reported, not hidden)
        out["legs"]["torch_conv1d"] = {"error": "%s: %s" % (type(err).__name__, str(err)[:200])}
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
