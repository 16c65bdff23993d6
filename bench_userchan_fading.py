#!/usr/bin/env python3
"""What fading rays per user (mcrx_hip_userfade_*, csrc/userchan.hip) cost on the transmitter's channel tiles,
next to the static emulator on the same tiles.  A secondary measurement -- bench.py holds the headline metric.

    python bench_userchan_fading.py [--channels C --blocks B --steps K --warmup W --reps R --out FILE --leg-timeout S]

The tiles of the 512-channel slab (default: 202 848 blocks x 512 channels, 0.83 GB in and 0.83 GB out), as bench_userchan.py has them:
an output buffer allocated beforehand, the C-ABI on a side stream, HIP events around --steps calls, the median of --reps repetitions with
its spread (max - min) / median.  Legs:
    static_T3         three static rays a channel, no rotation, a handle that never faded (bench_userchan.py's T3)
    static_T3_after   the same table in a handle made with fading and switched off again: the same kernel
    fade_T3_L4        three fading rays on every channel, the gains updated every 16 blocks
    fade_T3_L8        ... every 256 blocks
    fade_T4_L4        four fading rays, every 16 blocks
    gains_T3_L4       the gain kernel alone: the rows fade_T3_L4 writes, in that leg's spans
Every leg is a process of its own, started under `timeout` one after the other; the first that fails ends the run (nothing is started on
the GPU behind a fault or a hang).  A fading leg also reports the rows and bytes of gain table a call writes, its spans, and its
algorithmic GB: input once + output once + table written + table read once.  One JSON line; --out also writes it to a file.
Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8.0e12
LEGS = {"static_T3": (3, None, False), "static_T3_after": (3, 4, False), "fade_T3_L4": (3, 4, True), "fade_T3_L8": (3, 8, True),
        "fade_T4_L4": (4, 4, True), "gains_T3_L4": (3, 4, True)}           # rays, log2_block, fading left on


def report(samples, table_bytes, ms):
    med = statistics.median(ms)
    gb = (samples * 16 + 2 * table_bytes) / 1e9
    return {"ms": round(med, 4), "reps_ms": [round(v, 4) for v in ms], "spread": round((max(ms) - min(ms)) / med, 4),
            "algorithmic_gb": round(gb, 4), "gsamples_per_s": round(samples / med / 1e6, 2),
            "fraction_of_8_tb_per_s": round(gb * 1e9 / (med * 1e-3) / PEAK_BYTES_PER_S, 4)}


def fading_of(Cn, rays, log2_block):
    """every user fades: Dopplers of 0.05 .. 0.1 cycles per update interval, Rice factors 0, 1, 8, each user their own"""
    B = float(1 << log2_block)
    users = [dict(doppler=[(0.05 + 0.05 * ((c * 7 + i) % 11) / 10.0) / B for i in range(rays)], rice_k=[float((0, 1, 8)[(c + i) % 3]) for i in range(rays)],
                  los_doppler=0.02 / B, los_phase=(c * 0x9E3779B9) % (1 << 32)) for c in range(Cn)]
    return dict(log2_block=log2_block, sinusoids=16, seed=16, users=users)


def run_leg(args):
    import torch
    from __graft_entry__ import load_product
    from bench_userchan import channels_of
    assert torch.cuda.is_available(), "bench_userchan_fading.py needs the GPU"
    prod = load_product()
    L = prod.lib()
    dev = torch.device("cuda", 0)
    rays, log2_block, on = LEGS[args.leg]
    Cn, nb, lead = args.channels, args.blocks // 8 * 8, 32
    n = nb * Cn
    gen = torch.Generator(device=dev)
    gen.manual_seed(16)
    d_x = torch.view_as_complex(torch.randn(((lead + nb) * Cn, 2), generator=gen, device=dev))
    d_y = torch.empty(n, dtype=torch.complex64, device=dev)
    side = torch.cuda.Stream(device=dev)
    st = C.c_void_p(side.cuda_stream)

    def timed(fn, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            a.record(side)
            for _ in range(k):
                fn()
            b.record(side)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / k

    uc = prod.userchan(channels=channels_of(Cn, rays, False), fading=None if log2_block is None else fading_of(Cn, rays, log2_block))
    assert uc.lead_blocks <= lead
    if not on:
        uc.set_fading(None)
    assert uc.fading_on() == on
    rows = spans = table_bytes = 0
    span_rows = []
    if on:                                                              # the spans of a call from block 0, as apply_tiles cuts them
        B = 1 << log2_block
        cap = min(((nb - 1) >> log2_block) + 2, (64 << 20) // (Cn * 32))
        off = 0
        while off < nb:
            m = min(nb - off, (cap - 1) * B - off % B)
            span_rows.append((off >> log2_block, ((off % B + m - 1) >> log2_block) + 2))
            off += m
        rows, spans = sum(r for _, r in span_rows), len(span_rows)
        table_bytes = rows * Cn * 32

    def check(rc, what):
        if rc != prod.MCRX_OK:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, L.mcrx_hip_userchan_last_error().decode()))

    if args.leg.startswith("gains"):
        d_t = torch.empty(max(r for _, r in span_rows) * Cn * 4, dtype=torch.complex64, device=dev)

        def call():
            for first, r in span_rows:
                check(L.mcrx_hip_userfade_gains(uc._h, first, r, C.c_void_p(d_t.data_ptr()), st), "mcrx_hip_userfade_gains")
        samples, tb = 0, table_bytes / 2.0                              # (written only)
    else:
        def call():
            check(L.mcrx_hip_userchan_apply_tiles(uc._h, C.c_void_p(d_x.data_ptr()), 0, nb, lead, C.c_void_p(d_y.data_ptr()), st),
                  "mcrx_hip_userchan_apply_tiles")
        samples, tb = n, table_bytes
    timed(call, args.warmup)
    rec = report(samples, tb, [timed(call, args.steps) for _ in range(args.reps)])
    rec.update(rays=rays, log2_block=log2_block, fading=on, table_rows_per_call=rows, table_bytes_per_call=table_bytes, spans=spans,
               device=torch.cuda.get_device_name(0))
    uc.close()
    print("LEG " + json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=202848)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="run this leg in this process (what the driver starts)")
    ap.add_argument("--legs", type=str, default=",".join(LEGS), help="the legs the driver runs, in this order")
    ap.add_argument("--leg-timeout", type=int, default=120, help="seconds a leg's process may take")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "userchan_fading.json"))
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    out = {"metric": "per-user channel emulator with fading rays on the channel tiles", "channels": args.channels,
           "blocks": args.blocks // 8 * 8, "lead_blocks": 32, "steps": args.steps, "reps": args.reps, "legs": {}}
    for leg in args.legs.split(","):
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg, "--channels", str(args.channels),
               "--blocks", str(args.blocks), "--steps", str(args.steps), "--warmup", str(args.warmup), "--reps", str(args.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG ")]
        if p.returncode != 0 or not lines:                              # a fault, a hang or an error: nothing more is started
            out["stopped_at"] = {"leg": leg, "exit_status": p.returncode}
            break
        rec = json.loads(lines[-1][4:])
        out.setdefault("device", rec.pop("device"))
        rec.pop("device", None)
        out["legs"][leg] = rec
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)
    return 1 if "stopped_at" in out else 0


if __name__ == "__main__":
    sys.exit(main())
