#!/usr/bin/env python3
"""What 16-bit integer IQ (mcrx_hip_config::input_format = 1, sc16) is worth against cf32.  A secondary measurement -- bench.py holds
the headline metric, which is the cf32 path.

    python bench_sc16.py [--steps K --warmup W --reps R]

At 512 channels, front_end 0 and 1, the same slab of traffic -- quantised to int16, and the cf32 receiver gets exactly the dequantised
floats -- through a cf32 and an sc16 receiver of one process, alternating rep by rep; medians of --reps repetitions:
1. the channelizer alone (mcrx_hip_channelize, HIP events around --steps launches): algorithmic bytes 8 + 4 per wideband sample for
   cf32, 4 + 4 for sc16, and what fraction of the 8 TB/s HBM peak that is;
2. the pushed receiver (execute_device / execute_device_sc16 + discard, as bench.py pushes);
3. execute_host / execute_host_sc16 from pageable host memory, flushed (the host link carries half the bytes).
One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0
FORMATS = ("cf32", "sc16")
BYTES_PER_SAMPLE = {"cf32": 12, "sc16": 8}          # channelizer: read + written


def median_ms(ms):
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}


def leg(prod, torch, dev, N, M, cp, frames, plen, front_end, steps, warmup, reps):
    tx = prod.multichanneltx(N, M, cp, 4)
    iq, _ = tx.generate(frames, plen, seed=0xBEEF, device=dev)
    tx.close()
    K = 2 * N
    n = int(iq.numel()) // (prod.TILE * K) * (prod.TILE * K)
    peak = float(torch.view_as_real(iq[:n]).abs().max())
    d_q = torch.round(torch.view_as_real(iq[:n]) * (0.45 / peak * 32768.0)).to(torch.int16).reshape(-1).contiguous()
    d_x = torch.view_as_complex((d_q.to(torch.float32) * 2.0 ** -15).reshape(-1, 2)).contiguous()
    del iq
    dev_in = {"cf32": d_x, "sc16": d_q}
    host_in = {"cf32": d_x.cpu().numpy(), "sc16": d_q.cpu().numpy()}
    cfg = dict(max_payload_len=plen, max_frames=N * frames + 64, skip_framesyms=1, front_end=front_end)
    rxs = {f: prod.multichannelrx(N, M, cp, 4, input_format=f, **cfg) for f in FORMATS}
    nblocks = n // K
    d_out = torch.empty(nblocks * N, dtype=torch.complex64, device=dev)
    side = torch.cuda.Stream(device=dev)            # not the legacy default stream: that one is a barrier across the handle's streams
    out = {"channels": N, "front_end": front_end, "samples_per_step": n, "steps": steps, "reps": reps}

    # 1. the channelizer alone
    def chan(f, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            a.record(side)
            for _ in range(k):
                rxs[f].channelize(dev_in[f], nblocks, 0, d_out, stream=side)
            b.record(side)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / k
    for f in FORMATS:
        chan(f, warmup)
    ms = {f: [] for f in FORMATS}
    for _ in range(reps):
        for f in FORMATS:
            ms[f].append(chan(f, steps))
    med = median_ms(ms)
    out["channelizer_ms"] = med
    out["channelizer_ms_all"] = {f: [round(v, 4) for v in ms[f]] for f in FORMATS}
    out["channelizer_gbytes_per_s"] = {f: round(BYTES_PER_SAMPLE[f] * n / med[f] / 1e6, 1) for f in FORMATS}
    out["channelizer_frac_of_hbm_peak"] = {f: round(BYTES_PER_SAMPLE[f] * n / med[f] / 1e6 / HBM_PEAK_GBS, 4) for f in FORMATS}
    out["channelizer_sc16_over_cf32"] = round(med["sc16"] / med["cf32"], 4)

    # 2. the pushed receiver
    def push(f, k):
        t0 = time.perf_counter()
        with torch.cuda.stream(side):
            for _ in range(k):
                rxs[f].Execute(dev_in[f], stream=side)
                rxs[f].Discard()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k
    for f in FORMATS:
        push(f, warmup)
    ms = {f: [] for f in FORMATS}
    for _ in range(reps):
        for f in FORMATS:
            ms[f].append(push(f, steps))
    med = median_ms(ms)
    out["pushed_receiver_ms"] = med
    out["pushed_receiver_gsamples_per_s"] = {f: round(n / med[f] / 1e6, 2) for f in FORMATS}
    out["pushed_receiver_sc16_over_cf32"] = round(med["sc16"] / med["cf32"], 4)

    # 3. from host memory
    def host(f, k):
        t0 = time.perf_counter()
        for _ in range(k):
            rxs[f].Execute(host_in[f])
            rxs[f].Flush()
            del rxs[f].frames[:]
        return (time.perf_counter() - t0) * 1e3 / k
    hsteps = max(1, steps // 2)
    for f in FORMATS:
        rxs[f].Flush(); del rxs[f].frames[:]
        host(f, 1)
    ms = {f: [] for f in FORMATS}
    for _ in range(reps):
        for f in FORMATS:
            ms[f].append(host(f, hsteps))
    med = median_ms(ms)
    out["execute_host_ms"] = med
    out["execute_host_gsamples_per_s"] = {f: round(n / med[f] / 1e6, 3) for f in FORMATS}
    out["execute_host_link_gbytes_per_s"] = {f: round((8 if f == "cf32" else 4) * n / med[f] / 1e6, 2) for f in FORMATS}
    out["execute_host_sc16_over_cf32"] = round(med["sc16"] / med["cf32"], 4)
    for rx in rxs.values():
        rx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--channels", type=int, default=512)
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_product
    prod = load_product()
    dev = torch.device("cuda", 0)
    out = {"metric": "sc16 against cf32 input", "device": torch.cuda.get_device_name(0)}
    for fe in (0, 1):
        out["front_end_%d" % fe] = leg(prod, torch, dev, args.channels, 64, 8, 16, 1200, fe, args.steps, args.warmup, args.reps)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
