#!/usr/bin/env python3
"""What the channel monitor (csrc/monitor.hip, mcrx_hip_monitor_*) costs.  A secondary measurement -- bench.py holds the headline
metric, which is by construction the monitor-off path.

    python bench_monitor.py [--steps K --warmup W --reps R]

1. the kernel alone: a serial handle (every kernel of a push in order on one stream) pushed with the monitor off and on, alternating;
   the difference of the medians is the monitor's kernels by themselves.  Bytes it has to fetch: 4 per wideband sample.
   (`rocprofv3 --kernel-trace --stats -- python bench_monitor.py --kernel-only` names the kernels one by one; counters in a run of their own.)
2. the 512-channel headline shape and the 8-channel long-push shape of bench.py as continuous streams through two un-restarted
   receivers of one process, monitor off and on, alternating rep by rep; medians of --reps repetitions.
One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0


def make_slabs(prod, dev, N, M, cp, frames, plen):
    tx = prod.multichanneltx(N, M, cp, 4)
    base = int(prod.lib().mctx_hip_blocks_for(tx._h, frames, plen, 40, 1, 6))
    slabs = [tx.generate(frames, plen, seed=0xBEEF + 7919 * i, nblocks=base + (0, 48)[i], device=dev)[0] for i in range(2)]
    tx.close()
    return slabs


def stream_leg(prod, torch, dev, N, M, cp, frames, plen, steps, warmup, reps, serial=False, nfft=64):
    slabs = make_slabs(prod, dev, N, M, cp, frames, plen)
    torch.cuda.synchronize()
    cfg = dict(max_payload_len=plen, max_frames=N * frames + 64, skip_framesyms=1)
    if serial:
        cfg["serial"] = 1
    rxs = {"off": prod.multichannelrx(N, M, cp, 4, **cfg), "on": prod.multichannelrx(N, M, cp, 4, **cfg)}
    rxs["on"].monitor_enable(nfft, "hann")
    side = torch.cuda.Stream(device=dev)            # not the legacy default stream: that one is a barrier across the handle's streams

    def run(rx, n):
        with torch.cuda.stream(side):
            for _ in range(n):
                for x in slabs:
                    rx.Execute(x, stream=side)
                    rx.Discard()
        torch.cuda.synchronize()

    samples = sum(int(x.numel()) for x in slabs)
    for rx in rxs.values():
        run(rx, warmup)
    ms = {"off": [], "on": []}
    for _ in range(reps):
        for which in ("off", "on"):
            t0 = time.perf_counter()
            run(rxs[which], steps)
            ms[which].append((time.perf_counter() - t0) * 1e3 / steps)
    r = rxs["on"].monitor_read()
    assert r.nsamp > 0 and r.nseg > 0 and (r.level > 0).all()
    for rx in rxs.values():
        rx.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"channels": N, "frames_per_channel_and_slab": frames, "samples_per_step": samples, "steps": steps, "reps": reps, "nfft": nfft,
            "ms_per_step_off": [round(v, 4) for v in ms["off"]], "ms_per_step_on": [round(v, 4) for v in ms["on"]],
            "median_ms_off": round(med["off"], 4), "median_ms_on": round(med["on"], 4),
            "gsamples_per_s_off": round(samples / med["off"] / 1e6, 2), "gsamples_per_s_on": round(samples / med["on"] / 1e6, 2),
            "on_over_off": round(med["on"] / med["off"], 4), "monitor_bytes_per_step": 4 * samples}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true", help="only the serial leg (for a profiler run)")
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_product
    prod = load_product()
    dev = torch.device("cuda", 0)
    out = {"metric": "channel monitor cost", "device": torch.cuda.get_device_name(0)}
    k = stream_leg(prod, torch, dev, 512, 64, 8, 16, 1200, args.steps, args.warmup, args.reps, serial=True)
    d_ms = k["median_ms_on"] - k["median_ms_off"]
    k["monitor_kernels_ms_per_step"] = round(d_ms, 4)
    if d_ms > 0:
        k["monitor_gbytes_per_s"] = round(k["monitor_bytes_per_step"] / d_ms / 1e6, 1)
        k["monitor_frac_of_hbm_peak"] = round(k["monitor_bytes_per_step"] / d_ms / 1e6 / HBM_PEAK_GBS, 4)
    out["kernel_alone_serial_512ch"] = k
    torch.cuda.empty_cache()
    if not args.kernel_only:
        out["headline_512ch"] = stream_leg(prod, torch, dev, 512, 64, 8, 16, 1200, args.steps, args.warmup, args.reps)
        torch.cuda.empty_cache()
        out["8ch_long_pushes"] = stream_leg(prod, torch, dev, 8, 64, 8, 400, 1200, args.steps, args.warmup, args.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
