#!/usr/bin/env python3
"""What the feedback aligner (mcrx_hip_fbalign_*, csrc/fbalign.hip) costs on the wideband stream.  A secondary measurement -- bench.py
holds the headline metric.  First figures, no target.

    python bench_fbalign.py [--samples N --rows R --steps K --warmup W --reps R --rms LEVEL --out FILE]

One slab of --samples samples (default: the 512-channel slab, 207.7 M) of complex Gaussian samples through handles of one process, into
buffers allocated beforehand, through the C-ABI on a side stream, HIP events around --steps calls; the median of --reps repetitions
with its spread (max - min) / median.  Legs:
    copy_d2d                  hipMemcpyAsync device to device of the same 8 B a sample, timed in the same session
    rfchain_none              the streaming floor: rfchain with no stage on, cf32 to cf32 (8 B in + 8 B out a sample), rerun here
    untouched_cf32, _sc16     a handle without an update or a set: the copy build (cf32 in: 16 B a sample; sc16 in: 12 B)
    apply_cf32, apply_sc16    the 32-tap filter at a delay of 7.37 samples and a scale of 1.67 e^{-1.1j} (max_lag 16)
    measure_l8, _l32, _l64    reset + measure of --rows rows (default 2^22) at max_lag 8, 32 and 64 (16 B in a row)
    update_l32                the update alone, one launch a repetition, each behind a measure of its own that is not timed
Every leg reports ms a call, its algorithmic GB and that traffic as a fraction of 8 TB/s (HBM peak).  One JSON line; --out also writes it
to a file.  Needs the GPU: there is no fallback."""
import argparse
import cmath
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
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rms", type=float, default=0.1, help="level of the input per component against the full scale 1.0")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "fbalign.json"))
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_product
    assert torch.cuda.is_available(), "bench_fbalign.py needs the GPU"
    prod = load_product()
    L = prod.lib()
    dev = torch.device("cuda", 0)
    n, rows = args.samples, args.rows
    assert 1 << 16 <= rows <= n - 200, "rows: at least 2^16, and inside the slab"
    gen = torch.Generator(device=dev)
    gen.manual_seed(21)
    d_x = torch.view_as_complex(torch.randn((n, 2), generator=gen, device=dev) * args.rms)
    d_f = torch.empty(n, dtype=torch.complex64, device=dev)
    d_i = (torch.view_as_real(d_x) * 32768.0).round_().clamp_(-32768, 32767).to(torch.int16)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    sp = C.c_void_p(side.cuda_stream)
    err = L.mcrx_hip_fbalign_last_error

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

    def ok(rc, what, e=err):
        if rc != prod.MCRX_OK:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, e().decode()))

    out = {"metric": "feedback alignment on the wideband stream", "device": torch.cuda.get_device_name(0), "samples": n, "rows": rows,
           "rms": args.rms, "steps": args.steps, "reps": args.reps, "legs": {}}

    def copy():
        d_f.copy_(d_x, non_blocking=True)
    out["legs"]["copy_d2d"] = report(n, 16, measure(copy))

    rf = prod.rfchain()

    def floor():
        ok(L.mcrx_hip_rfchain_execute_device(rf._h, C.c_void_p(d_x.data_ptr()), 0, n, C.c_void_p(d_f.data_ptr()), sp), "mcrx_hip_rfchain_execute_device",
           L.mcrx_hip_rfchain_last_error)
    out["legs"]["rfchain_none"] = report(n, 16, measure(floor))
    rf.close()

    for fin, src, nbytes in (("cf32", d_x, 16), ("sc16", d_i, 12)):
        h = prod.fbalign(16, 1.0, 1.0, input_format=fin)
        count = n - 2 * h.halo

        def call(h=h, src=src, count=count):
            ok(L.mcrx_hip_fbalign_execute_device(h._h, C.c_void_p(src.data_ptr()), count, C.c_void_p(d_f.data_ptr()), sp), "mcrx_hip_fbalign_execute_device")
        out["legs"]["untouched_" + fin] = report(count, nbytes, measure(call))
        h.set(int(round(7.37 * 2.0 ** 32)), cmath.rect(1.0 / 0.6, -1.1), stream=side)
        out["legs"]["apply_" + fin] = report(count, nbytes, measure(call))
        h.close()

    d_z = d_x[3:3 + rows + 200].clone()
    for Lm in (8, 32, 64):
        h = prod.fbalign(Lm, 1.0, 1.0)
        count = rows + 2 * h.R

        def meas(h=h, count=count):
            ok(L.mcrx_hip_fbalign_reset(h._h), "mcrx_hip_fbalign_reset")
            ok(L.mcrx_hip_fbalign_measure_device(h._h, C.c_void_p(d_x.data_ptr()), C.c_void_p(d_z.data_ptr()), count, sp), "mcrx_hip_fbalign_measure_device")
        name = "measure_l%d" % Lm
        out["legs"][name] = report(rows, 16, measure(meas))
        st = h.read(stream=side)
        out["legs"][name].update(rows=st["rows"], clamped=st["clamped"])
        if Lm == 32:
            def upd(h=h):
                ok(L.mcrx_hip_fbalign_update(h._h, sp), "mcrx_hip_fbalign_update")

            def one_update(meas=meas, upd=upd):                         # an update clears the sums: each timed one has its own measure in front, untimed
                with torch.cuda.stream(side):
                    meas()
                torch.cuda.synchronize()
                return timed(upd, 1)
            one_update()
            out["legs"]["update_l32"] = report(0, 0, [one_update() for _ in range(args.reps)])
            st = h.read(stream=side)
            out["legs"]["update_l32"].update(updates=st["updates"], degenerate=st["degenerate"])
        h.close()

    legs = out["legs"]
    for name in ("untouched_cf32", "untouched_sc16", "apply_cf32", "apply_sc16"):
        out[name + "_over_floor"] = round(legs[name]["ms"] / legs["rfchain_none"]["ms"], 4)
    out["legs"]["copy_d2d_again"] = report(n, 16, measure(copy))
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
