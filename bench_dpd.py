#!/usr/bin/env python3
"""What the digital predistorter (mcrx_hip_dpd_*, csrc/dpd.hip) costs on the wideband stream.  A secondary measurement -- bench.py holds
the headline metric.

    python bench_dpd.py [--samples N --steps K --warmup W --reps R --rms LEVEL --out FILE]

One slab of --samples samples (default: the 512-channel slab, 207.7 M) of complex Gaussian samples -- Rayleigh amplitudes, as crowded
into a few bins as OFDM's -- through handles of one process, into buffers allocated beforehand, through the C-ABI on a side stream, HIP
events around --steps calls; the median of --reps repetitions with its spread (max - min) / median.  The tables are learned first, on
the slab's first 2^24 samples, from a Rapp amplifier at 10 dB back-off with 5 degrees of AM/PM (rfchain).  Legs:
    copy_d2d                  hipMemcpyAsync device to device of the same 8 B a sample, timed in the same session
    rfchain_none              the streaming floor: rfchain with no stage on, cf32 to cf32 (8 B in + 8 B out a sample), rerun here
    untouched_cf32            a handle without a table: the copy build
    apply_cf32_k128, apply_sc16_k128, apply_cf32_k1024, apply_sc16_k1024      the apply builds at both table sizes
    measure_k128, measure_k1024     reset + measure of the whole slab (16 B in a sample, nothing out)
    measure_k128_one_bin, measure_k128_uniform      the same with every amplitude in one bin, and spread evenly over the table: what crowding costs
    update_k128, update_k1024       the one-lane update alone
    torch_apply               the same apply in torch: bucketize + gather + lerp + complex multiply
    torch_measure             the same sums in torch: rint, mask, and index_add_ into int64 accumulators
Every leg reports ms a call, its algorithmic GB and that traffic as a fraction of 8 TB/s (HBM peak).  One JSON line; --out also writes it
to a file.  Needs the GPU: there is no fallback."""
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
    ap.add_argument("--rms", type=float, default=0.1, help="level of the input per component against the full scale 1.0")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "dpd.json"))
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_product
    assert torch.cuda.is_available(), "bench_dpd.py needs the GPU"
    prod = load_product()
    L = prod.lib()
    dev = torch.device("cuda", 0)
    n = args.samples
    assert n <= 1 << prod.DPD_GUARD_LOG2, "the measure legs offer the whole slab in one call: at most 2^28 samples"
    gen = torch.Generator(device=dev)
    gen.manual_seed(21)
    d_x = torch.view_as_complex(torch.randn((n, 2), generator=gen, device=dev) * args.rms)
    d_f = torch.empty(n, dtype=torch.complex64, device=dev)
    d_i = torch.empty((n, 2), dtype=torch.int16, device=dev)
    side = torch.cuda.Stream(device=dev)
    amp_rms = args.rms * 2.0 ** 0.5
    full_scale = 6.0 * amp_rms                                          # e^-36 of the samples lie beyond the table
    amp = prod.rfchain(amplifier=dict(sat=prod.rfchain_backoff(10.0, amp_rms), smooth=2, ampm_deg=5.0))
    d_z = amp.execute(d_x).clone()                                      # the feedback of the measure legs
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

    def measure_few(fn):                                                # the torch legs: seconds a call
        timed(fn, 1)
        return [timed(fn, 1) for _ in range(3)]

    def ok(rc, what):
        if rc != prod.MCRX_OK:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, L.mcrx_hip_dpd_last_error().decode()))

    out = {"metric": "digital predistortion on the wideband stream", "device": torch.cuda.get_device_name(0), "samples": n, "rms": args.rms,
           "full_scale": full_scale, "steps": args.steps, "reps": args.reps, "legs": {}}

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

    def execute_leg(d, dst):
        def call():
            ok(L.mcrx_hip_dpd_execute_device(d._h, C.c_void_p(d_x.data_ptr()), n, C.c_void_p(dst.data_ptr()), sp), "mcrx_hip_dpd_execute_device")
        return measure(call)

    d = prod.dpd(7, full_scale, 1.0)
    out["legs"]["untouched_cf32"] = report(n, 16, execute_leg(d, d_f))
    d.close()
    tables = {}
    for log2 in (7, 10):
        K = 1 << log2
        for fout, dst, nbytes in (("cf32", d_f, 16), ("sc16", d_i, 12)):
            d = prod.dpd(log2, full_scale, 1.0, output_format=fout)
            if fout == "cf32":
                with torch.cuda.stream(side):
                    d.learn(d_x[:1 << 24], amp, 3, stream=side)
                st = d.read(stream=side)
                tables[log2] = st["F"]
                out["legs"]["learned_k%d" % K] = {"updates": st["updates"], "valid_bins": int(((st["cnt"] >= 8) & (st["Suu"] > 0)).sum()),
                                                  "skipped": st["skipped"]}
            else:
                d.set_table(tables[log2], stream=side)
            name = "apply_%s_k%d" % (fout, K)
            out["legs"][name] = report(n, nbytes, execute_leg(d, dst))
            if fout == "sc16":
                out["legs"][name]["clipped_per_call"] = d.clipped() // (args.warmup + args.steps * args.reps)
            else:
                def meas(d=d):
                    ok(L.mcrx_hip_dpd_reset(d._h), "mcrx_hip_dpd_reset")
                    ok(L.mcrx_hip_dpd_measure_device(d._h, C.c_void_p(d_x.data_ptr()), C.c_void_p(d_z.data_ptr()), n, sp), "mcrx_hip_dpd_measure_device")
                out["legs"]["measure_k%d" % K] = report(n, 16, measure(meas))
                st = d.read(stream=side)
                out["legs"]["measure_k%d" % K].update(occupied_bins=int((st["cnt"] > 0).sum()), largest_bin_share=round(float(st["cnt"].max()) / n, 4),
                                                      skipped=st["skipped"])

                if log2 == 7:                                           # what the crowding of the bins costs: every sample in one bin, and none crowded
                    unit = d_x / d_x.abs().clamp_(min=1e-30)
                    for tag, amp_of in (("one_bin", lambda: torch.full((n,), 0.4 * full_scale, device=dev)),
                                        ("uniform", lambda: torch.rand(n, generator=gen, device=dev) * full_scale)):
                        d_u = (unit * amp_of()).contiguous()
                        torch.cuda.synchronize()

                        def meas_u(d=d, d_u=d_u):
                            ok(L.mcrx_hip_dpd_reset(d._h), "mcrx_hip_dpd_reset")
                            ok(L.mcrx_hip_dpd_measure_device(d._h, C.c_void_p(d_u.data_ptr()), C.c_void_p(d_z.data_ptr()), n, sp), "mcrx_hip_dpd_measure_device")
                        out["legs"]["measure_k128_" + tag] = report(n, 16, measure(meas_u))
                        st = d.read(stream=side)
                        out["legs"]["measure_k128_" + tag].update(occupied_bins=int((st["cnt"] > 0).sum()), largest_bin_share=round(float(st["cnt"].max()) / n, 4))
                        del d_u
                    del unit

                def upd(d=d):
                    ok(L.mcrx_hip_dpd_update(d._h, sp), "mcrx_hip_dpd_update")
                out["legs"]["update_k%d" % K] = report(0, 0, measure(upd))
            d.close()
    amp.close()
    legs = out["legs"]
    for name in ("untouched_cf32", "apply_cf32_k128", "apply_cf32_k1024", "measure_k128", "measure_k1024"):
        out[name + "_over_floor"] = round(legs[name]["ms"] / legs["rfchain_none"]["ms"], 4)

    # the same work in torch
    K = 128
    inv_step = K / full_scale
    F = torch.from_numpy(tables[7]).to(dev)
    edges = torch.arange(1, K, device=dev, dtype=torch.float32) / inv_step

    def torch_apply():
        a = d_x.abs()
        k = torch.bucketize(a, edges)
        f = (a * inv_step - k).clamp_(0.0, 1.0)
        return torch.lerp(F[k], F[k + 1], f.to(torch.complex64)) * d_x
    out["legs"]["torch_apply"] = report(n, 16, measure_few(torch_apply))
    acc = torch.zeros((K + 2, 4), dtype=torch.int64, device=dev)
    scale = 2.0 ** (32 - 2 * math.ceil(math.log2(full_scale)))

    def torch_measure():
        j = torch.round(d_x.abs() * inv_step).clamp_(max=K + 1).long()
        p = d_z.to(torch.complex128) * d_x.conj().to(torch.complex128)
        uu = (d_x.real.double() ** 2 + d_x.imag.double() ** 2)
        t = torch.stack([torch.ones_like(uu), p.real * scale, p.imag * scale, uu * scale], dim=1).round_().long()
        acc.zero_()
        acc.index_add_(0, j, t)
    out["legs"]["torch_measure"] = report(n, 16, measure_few(torch_measure))
    out["legs"]["copy_d2d_again"] = report(n, 16, measure(copy))
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
