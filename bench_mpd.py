#!/usr/bin/env python3
"""What the memory-polynomial predistorter (mcrx_hip_mpd_*, csrc/mpd.hip) costs on the wideband stream.  A secondary measurement --
bench.py holds the headline metric.

    python bench_mpd.py [--samples N --rows R --steps K --warmup W --reps R --rms LEVEL --out FILE]

One slab of --samples samples (default: the 512-channel slab, 207.7 M) of complex Gaussian samples through handles of one process, into
buffers allocated beforehand, through the C-ABI on a side stream, HIP events around --steps calls; the median of --reps repetitions
with its spread (max - min) / median.  The main table is dpd's, learned on the slab's first 2^24 samples from a Rapp amplifier at 10 dB
back-off with 5 degrees of AM/PM (rfchain); the side branches' tables are a tenth of it (the time does not depend on the entries).  Legs:
    copy_d2d                  hipMemcpyAsync device to device of the same 8 B a sample, timed in the same session
    rfchain_none              the streaming floor: rfchain with no stage on, cf32 to cf32 (8 B in + 8 B out a sample), rerun here
    dpd_apply_k128            dpd's apply with the same table, in the same session
    apply_m1 .. apply_m4      mpd's apply at K = 128 with 1 .. 4 branches on delays 0, 1, 2, 3 (cf32; apply_m3_sc16: sc16 out)
    untouched_m3              a three-branch handle without tables: the copy build
    measure_l5, _l15, _l20    reset + measure of --rows rows (default 2^24) with 1, 3 and 4 branches of five powers (16 B in a row)
    update_l15                the update alone (K = 128)
    torch_apply_m3            the three-branch apply in torch: bucketize + gather + lerp + complex multiply per branch, summed
Every leg reports ms a call, its algorithmic GB and that traffic as a fraction of 8 TB/s (HBM peak).  One JSON line; --out also writes it
to a file.  Needs the GPU: there is no fallback."""
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


def report(n, bytes_per_sample, ms):
    med = statistics.median(ms)
    gb = n * bytes_per_sample / 1e9
    return {"ms": round(med, 4), "reps_ms": [round(v, 4) for v in ms], "spread": round((max(ms) - min(ms)) / med, 4),
            "algorithmic_gb": round(gb, 4), "gsamples_per_s": round(n / med / 1e6, 2),
            "fraction_of_8_tb_per_s": round(gb * 1e9 / (med * 1e-3) / PEAK_BYTES_PER_S, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=207700000)
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rms", type=float, default=0.1, help="level of the input per component against the full scale 1.0")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mpd.json"))
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_product
    assert torch.cuda.is_available(), "bench_mpd.py needs the GPU"
    prod = load_product()
    L = prod.lib()
    dev = torch.device("cuda", 0)
    n, rows = args.samples, args.rows
    assert 1 << 16 <= rows <= min(1 << prod.MPD_GUARD_LOG2, n - 16), "rows: 2^16 .. 2^26, and inside the slab"
    gen = torch.Generator(device=dev)
    gen.manual_seed(21)
    d_x = torch.view_as_complex(torch.randn((n, 2), generator=gen, device=dev) * args.rms)
    d_f = torch.empty(n, dtype=torch.complex64, device=dev)
    d_i = torch.empty((n, 2), dtype=torch.int16, device=dev)
    side = torch.cuda.Stream(device=dev)
    amp_rms = args.rms * 2.0 ** 0.5
    full_scale = 6.0 * amp_rms                                          # e^-36 of the samples lie beyond the table
    amp = prod.rfchain(amplifier=dict(sat=prod.rfchain_backoff(10.0, amp_rms), smooth=2, ampm_deg=5.0))
    d_z = amp.execute(d_x[:rows + 16]).clone()                          # the feedback of the measure legs
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

    def measure_few(fn):                                                # the torch leg: a fraction of a second a call
        timed(fn, 1)
        return [timed(fn, 1) for _ in range(3)]

    def ok(rc, what, err):
        if rc != prod.MCRX_OK:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, err().decode()))

    out = {"metric": "predistortion with memory on the wideband stream", "device": torch.cuda.get_device_name(0), "samples": n, "rows": rows,
           "rms": args.rms, "full_scale": full_scale, "steps": args.steps, "reps": args.reps, "legs": {}}

    def copy():
        d_f.copy_(d_x, non_blocking=True)
    out["legs"]["copy_d2d"] = report(n, 16, measure(copy))

    rf = prod.rfchain()

    def floor():
        ok(L.mcrx_hip_rfchain_execute_device(rf._h, C.c_void_p(d_x.data_ptr()), 0, n, C.c_void_p(d_f.data_ptr()), sp), "mcrx_hip_rfchain_execute_device",
           L.mcrx_hip_rfchain_last_error)
    out["legs"]["rfchain_none"] = report(n, 16, measure(floor))
    rf.close()

    d = prod.dpd(7, full_scale, 1.0)
    with torch.cuda.stream(side):
        d.learn(d_x[:1 << 24], amp, 3, stream=side)
    F0 = d.read(stream=side)["F"]

    def dpd_call():
        ok(L.mcrx_hip_dpd_execute_device(d._h, C.c_void_p(d_x.data_ptr()), n, C.c_void_p(d_f.data_ptr()), sp), "mcrx_hip_dpd_execute_device",
           L.mcrx_hip_dpd_last_error)
    out["legs"]["dpd_apply_k128"] = report(n, 16, measure(dpd_call))
    d.close()
    amp.close()

    def execute_leg(h, dst):
        count = n - h.lead

        def call():
            ok(L.mcrx_hip_mpd_execute_device(h._h, C.c_void_p(d_x.data_ptr()), count, C.c_void_p(dst.data_ptr()), sp), "mcrx_hip_mpd_execute_device",
               L.mcrx_hip_mpd_last_error)
        return count, measure(call)

    for M in (1, 2, 3, 4):
        for fout, dst, nbytes in (("cf32", d_f, 16), ("sc16", d_i, 12)):
            if fout == "sc16" and M != 3:
                continue
            h = prod.mpd(M, tuple(range(M)), 5, 7, full_scale, 1.0, output_format=fout)
            if M == 3 and fout == "cf32":
                count, ms = execute_leg(h, dst)
                out["legs"]["untouched_m3"] = report(count, nbytes, ms)
            h.set_tables(np.stack([F0 if m == 0 else np.complex64(0.1) * F0 for m in range(M)]), stream=side)
            count, ms = execute_leg(h, dst)
            name = "apply_m%d" % M + ("_sc16" if fout == "sc16" else "")
            out["legs"][name] = report(count, nbytes, ms)
            if fout == "sc16":
                out["legs"][name]["clipped_per_call"] = h.clipped() // (args.warmup + args.steps * args.reps)
            h.close()

    for M in (1, 3, 4):
        h = prod.mpd(M, tuple(range(M)), 5, 7, full_scale, 1.0)
        count = rows + h.lead

        def meas(h=h, count=count):
            ok(L.mcrx_hip_mpd_reset(h._h), "mcrx_hip_mpd_reset", L.mcrx_hip_mpd_last_error)
            ok(L.mcrx_hip_mpd_measure_device(h._h, C.c_void_p(d_x.data_ptr()), C.c_void_p(d_z.data_ptr()), count, sp), "mcrx_hip_mpd_measure_device",
               L.mcrx_hip_mpd_last_error)
        name = "measure_l%d" % (5 * M)
        out["legs"][name] = report(rows, 16, measure(meas))
        st = h.read(stream=side)
        out["legs"][name].update(eligible_rows=st["rows"], skipped=st["skipped"])
        if M == 3:
            def upd(h=h):
                ok(L.mcrx_hip_mpd_update(h._h, sp), "mcrx_hip_mpd_update", L.mcrx_hip_mpd_last_error)
            out["legs"]["update_l15"] = report(0, 0, measure(upd))
            st = h.read(stream=side)
            out["legs"]["update_l15"].update(updates=st["updates"], degenerate=st["degenerate"])
        h.close()

    legs = out["legs"]
    for name in ("dpd_apply_k128", "untouched_m3", "apply_m1", "apply_m2", "apply_m3", "apply_m4"):
        out[name + "_over_floor"] = round(legs[name]["ms"] / legs["rfchain_none"]["ms"], 4)
    out["apply_m1_over_dpd_apply"] = round(legs["apply_m1"]["ms"] / legs["dpd_apply_k128"]["ms"], 4)

    # the three-branch apply in torch
    K = 128
    inv_step = K / full_scale
    Ft = [torch.from_numpy(F0 if m == 0 else np.complex64(0.1) * F0).to(dev) for m in range(3)]
    edges = torch.arange(1, K, device=dev, dtype=torch.float32) / inv_step
    del d_i, d_z
    torch.cuda.empty_cache()

    def torch_apply():
        a = d_x.abs()
        k = torch.bucketize(a, edges)
        f = (a * inv_step - k).clamp_(0.0, 1.0).to(torch.complex64)
        y = None
        for m in range(3):
            p = torch.lerp(Ft[m][k], Ft[m][k + 1], f) * d_x
            y = p[2:] if m == 0 else y + p[2 - m:n - m]
        return y
    out["legs"]["torch_apply_m3"] = report(n, 16, measure_few(torch_apply))
    out["legs"]["copy_d2d_again"] = report(n, 16, measure(copy))
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
