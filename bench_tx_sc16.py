#!/usr/bin/env python3
"""What 16-bit integer IQ out of the transmitter (mctx_hip_set_output_format = 1, sc16) is worth against cf32.  A secondary
measurement -- bench.py holds the headline metric, which this does not touch.

    python bench_tx_sc16.py [--reps R --warmup W --frames F]

At 512 channels, M = 64, the slab of bench.py's headline (16 frames of 1200 bytes per channel: 207.7 M wideband samples), a cf32 and an
sc16 transmitter of one process alternating rep by rep; medians of --reps repetitions, HIP events on a side stream:
a. generate() on the device (host frame assembly, symbol kernel and synthesis: the whole call);
b. synthesize() alone from resident channel-rate tiles: algorithmic bytes 4 + 8 per wideband sample for cf32, 4 + 4 for sc16, and what
   fraction of the 8 TB/s HBM peak that is;
c. (a) followed by a copy of the slab to pinned host memory (the link carries half the bytes);
d. the quantisation pass sc16 users ran before (torch: scale, round, clamp, convert), alone and added to the cf32 time of (a).
One JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0
FORMATS = ("cf32", "sc16")
SYNTH_BYTES_PER_SAMPLE = {"cf32": 12, "sc16": 8}       # tiles read + slab written
SLAB_BYTES_PER_SAMPLE = {"cf32": 8, "sc16": 4}


def med(ms):
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--synth-steps", type=int, default=4, help="synthesize() launches per timed repetition of (b)")
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--payload", type=int, default=1200)
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_product
    prod = load_product()
    dev = torch.device("cuda", 0)
    N, M, cp, nf, plen = args.channels, 64, 8, args.frames, args.payload
    K = 2 * N
    txs = {f: prod.multichanneltx(N, M, cp, 4, output_format=f) for f in FORMATS}
    side = torch.cuda.Stream(device=dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            a.record(side)
            r = fn()
            b.record(side)
        torch.cuda.synchronize()
        return a.elapsed_time(b), r

    def alternate(fn, reps, warmup):
        for f in FORMATS:
            for _ in range(warmup):
                timed(lambda: fn(f))
        ms = {f: [] for f in FORMATS}
        for _ in range(reps):
            for f in FORMATS:
                ms[f].append(timed(lambda: fn(f))[0])
        return ms

    # a. generate on the device
    slab = {}

    def gen(f):
        slab[f] = None
        slab[f] = txs[f].generate(nf, plen, seed=0xBEEF, device=dev)[0]
    ms = alternate(gen, args.reps, args.warmup)
    n = int(slab["cf32"].numel())
    out = {"metric": "sc16 against cf32 output of the transmitter", "device": torch.cuda.get_device_name(0), "channels": N,
           "frames_per_channel": nf, "payload_len": plen, "samples": n, "reps": args.reps}
    gen_med = med(ms)
    out["generate_ms"] = gen_med
    out["generate_ms_all"] = {f: [round(v, 3) for v in ms[f]] for f in FORMATS}
    out["generate_sc16_over_cf32"] = round(gen_med["sc16"] / gen_med["cf32"], 4)
    out["clipped_samples"] = txs["sc16"].clipped(reset=True)

    # d. the quantisation pass in torch that the sc16 transmitter replaces
    def torch_pass(_f):
        return torch.clamp(torch.round(torch.view_as_real(slab["cf32"]) * 32768.0), -32768.0, 32767.0).to(torch.int16)
    tp = [timed(lambda: torch_pass("cf32"))[0] for _ in range(args.warmup + args.reps)][args.warmup:]
    same = bool(torch.equal(torch_pass("cf32"), slab["sc16"]))
    out["torch_quantise_ms"] = round(statistics.median(tp), 4)
    out["cf32_generate_plus_torch_quantise_ms"] = round(gen_med["cf32"] + statistics.median(tp), 4)
    out["sc16_equals_torch_quantise_of_cf32"] = same

    # c. generate, then the slab to pinned host memory
    pinned = {"cf32": torch.empty(n, dtype=torch.complex64).pin_memory(), "sc16": torch.empty((n, 2), dtype=torch.int16).pin_memory()}

    def gen_copy(f):
        gen(f)
        pinned[f].copy_(slab[f], non_blocking=True)
    ms = alternate(gen_copy, args.reps, args.warmup)
    m = med(ms)
    out["generate_to_pinned_host_ms"] = m
    out["generate_to_pinned_host_sc16_over_cf32"] = round(m["sc16"] / m["cf32"], 4)
    out["host_copy_ms"] = {f: round(m[f] - gen_med[f], 4) for f in FORMATS}
    out["host_link_gbytes_per_s"] = {f: round(SLAB_BYTES_PER_SAMPLE[f] * n / max(m[f] - gen_med[f], 1e-6) / 1e6, 2) for f in FORMATS}
    del pinned
    slab.clear()
    torch.cuda.empty_cache()

    # b. the synthesis kernel alone, from resident tiles
    lead = 48
    nb = n // K
    tr = txs["cf32"].traffic(0, N, nf, plen, seed=0xBEEF)
    tiles = torch.empty((lead + nb) * N, dtype=torch.complex64, device=dev)
    tr.tiles(-lead, lead + nb, tiles)
    torch.cuda.synchronize()
    outs = {f: txs[f]._slab(nb * K, dev) for f in FORMATS}

    def synth(f):
        for _ in range(args.synth_steps):
            txs[f].synthesize(tiles, 1, 0, nb, lead, 0, out=outs[f], stream=side)
    ms = alternate(synth, args.reps, args.warmup)
    ms = {f: [v / args.synth_steps for v in ms[f]] for f in FORMATS}
    m = med(ms)
    out["synthesize_ms"] = m
    out["synthesize_ms_all"] = {f: [round(v, 4) for v in ms[f]] for f in FORMATS}
    out["synthesize_bytes_per_sample"] = SYNTH_BYTES_PER_SAMPLE
    out["synthesize_gbytes_per_s"] = {f: round(SYNTH_BYTES_PER_SAMPLE[f] * n / m[f] / 1e6, 1) for f in FORMATS}
    out["synthesize_frac_of_hbm_peak"] = {f: round(SYNTH_BYTES_PER_SAMPLE[f] * n / m[f] / 1e6 / HBM_PEAK_GBS, 4) for f in FORMATS}
    out["synthesize_gsamples_per_s"] = {f: round(n / m[f] / 1e6, 2) for f in FORMATS}
    out["synthesize_sc16_over_cf32"] = round(m["sc16"] / m["cf32"], 4)
    tr.close()
    for tx in txs.values():
        tx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
