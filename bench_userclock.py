#!/usr/bin/env python3
"""What each user's own sample clock (mcrx_hip_userclock_*, csrc/userchan.hip) costs on the transmitter's
channel tiles, next to the static emulator on the same tiles.  A secondary measurement -- bench.py holds the headline metric.

    python bench_userclock.py [--channels C --blocks B --steps K --warmup W --reps R --parent-lib FILE --out FILE --leg-timeout S]

The tiles of the 512-channel slab (default: 202 848 blocks x 512 channels, 0.83 GB in and 0.83 GB out), as bench_userchan.py has them:
an output buffer allocated beforehand, the C-ABI on a side stream, HIP events around --steps calls, the median of --reps repetitions with
its spread (max - min) / median.  Every user has a fraction of a sample of their own (20 + (c * 37 % 64) / 64) and max_delay = 64.  Legs:
    clock_0ppm        the clock stage alone (mcrx_hip_userclock_apply_tiles), every user at 0 ppm: mu is constant per channel
    clock_20ppm       the clock stage alone, +-20 ppm alternating between the users: mu moves, n steps four times in the call
    clock20_T1        apply_tiles: the clock at 20 ppm and one ray behind it
    clock20_T3        apply_tiles: the clock at 20 ppm and three rays behind it
    static_T3         three static rays, no rotation, in a handle made with clocks and switched off again: the parent's kernel
    static_T3_parent  the same table through the C-ABI of the library --parent-lib names (the parent commit's build); without the
                      option the leg is recorded as not run
    conv1d            for scale: torch.nn.functional.conv1d of 32 static taps per channel (groups = 2 C real channels, channel-major)
Every leg is a process of its own, started under `timeout` one after the other; the first that fails ends the run (nothing is started on
the GPU behind a fault or a hang).  The two static legs use the library through ctypes alone, the same code on both sides.  A clock leg
also reports its spans and its algorithmic GB: input once + output once, and for apply_tiles z written and read once.  One JSON line;
--out also writes it to a file.  Needs the GPU: there is no fallback."""
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
LEGS = ["clock_0ppm", "clock_20ppm", "clock20_T1", "clock20_T3", "static_T3", "static_T3_parent", "conv1d"]
MAX_DELAY = 64


def report(samples, extra_bytes, ms):
    med = statistics.median(ms)
    gb = (samples * 16 + extra_bytes) / 1e9
    return {"ms": round(med, 4), "reps_ms": [round(v, 4) for v in ms], "spread": round((max(ms) - min(ms)) / med, 4),
            "algorithmic_gb": round(gb, 4), "gsamples_per_s": round(samples / med / 1e6, 2),
            "fraction_of_8_tb_per_s": round(gb * 1e9 / (med * 1e-3) / PEAK_BYTES_PER_S, 4)}


def clock_of(Cn, ppm):
    return dict(max_delay=MAX_DELAY, users=[dict(delay=20.0 + ((c * 37) % 64) / 64.0, ppm=ppm if c % 2 == 0 else -ppm, origin=0) for c in range(Cn)])


def run_leg(args):
    import torch
    from __graft_entry__ import load_product
    from bench_userchan import channels_of
    assert torch.cuda.is_available(), "bench_userclock.py needs the GPU"
    prod = load_product()
    dev = torch.device("cuda", 0)
    leg = args.leg
    Cn, nb = args.channels, args.blocks // 8 * 8
    lead = 32 if leg.startswith("static") else 128
    n = nb * Cn
    gen = torch.Generator(device=dev)
    gen.manual_seed(17)
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

    extra = {}
    if leg == "conv1d":
        x = torch.randn((1, 2 * Cn, 31 + nb), generator=gen, device=dev)
        w = torch.randn((2 * Cn, 1, 32), generator=gen, device=dev)

        def call():
            torch.nn.functional.conv1d(x, w, groups=2 * Cn)
        samples, more = n, 0
    else:
        d_x = torch.view_as_complex(torch.randn(((lead + nb) * Cn, 2), generator=gen, device=dev))
        d_y = torch.empty(n, dtype=torch.complex64, device=dev)
        rays = 1 if leg.endswith("T1") else 3
        chans = [prod.userchan_channel(**ch) for ch in channels_of(Cn, rays, False)]
        if leg.startswith("static"):                                    # ctypes alone: the parent's library has no clock to bind
            if leg == "static_T3_parent" and not args.parent_lib:
                print("LEG " + json.dumps({"not_run": "no --parent-lib given", "device": torch.cuda.get_device_name(0)}))
                return
            L = C.CDLL(args.parent_lib if leg == "static_T3_parent" else prod.build())
            table = (prod.UserchanChannel * Cn)(*chans)
            h = C.c_void_p()
            L.mcrx_hip_userchan_create.argtypes = [C.POINTER(C.c_void_p), C.c_uint, C.c_void_p, C.c_size_t]
            L.mcrx_hip_userchan_apply_tiles.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
            L.mcrx_hip_userchan_destroy.argtypes = [C.c_void_p]
            assert L.mcrx_hip_userchan_create(C.byref(h), Cn, C.addressof(table), C.sizeof(prod.UserchanChannel)) == 0
            if leg == "static_T3":                                      # a clock on and off again: the handle the parent's kernels run on
                f, users = prod.userchan_clock(Cn, **clock_of(Cn, 20.0))
                L.mcrx_hip_userclock_set.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
                assert L.mcrx_hip_userclock_set(h, C.addressof(f), C.addressof(users)) == 0 and L.mcrx_hip_userclock_set(h, None, None) == 0
            fn, handle = L.mcrx_hip_userchan_apply_tiles, h
            spans = 0
        else:
            uc = prod.userchan(channels=chans, clock=clock_of(Cn, 0.0 if leg == "clock_0ppm" else 20.0))
            need = uc.clock_lead_blocks if leg.startswith("clock_") else uc.lead_blocks
            assert uc.clock_on() and need <= lead, (need, lead)
            L = prod.lib()
            fn = L.mcrx_hip_userclock_apply_tiles if leg.startswith("clock_") else L.mcrx_hip_userchan_apply_tiles
            handle = uc._h
            span = (64 << 20) // (Cn * 8) // 128 * 128
            spans = 1 if leg.startswith("clock_") else (nb + span - 1) // span
            extra.update(spans=spans, max_delay=MAX_DELAY)

        def call():
            rc = fn(handle, C.c_void_p(d_x.data_ptr()), 0, nb, lead, C.c_void_p(d_y.data_ptr()), st)
            if rc != 0:
                raise RuntimeError("%s: the call failed (%d)" % (leg, rc))
        samples = n
        more = 0 if spans == 0 or leg.startswith("clock_") else n * 16   # z written and read once
    timed(call, args.warmup)
    rec = report(samples, more, [timed(call, args.steps) for _ in range(args.reps)])
    rec.update(extra, lead_blocks=lead, device=torch.cuda.get_device_name(0))
    print("LEG " + json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=202848)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", type=str, default=None, help="libmcrx_hip.so of the parent commit, for static_T3_parent")
    ap.add_argument("--leg", choices=LEGS, default=None, help="run this leg in this process (what the driver starts)")
    ap.add_argument("--legs", type=str, default=",".join(LEGS), help="the legs the driver runs, in this order")
    ap.add_argument("--leg-timeout", type=int, default=120, help="seconds a leg's process may take")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "userclock.json"))
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    out = {"metric": "per-user channel emulator with each user's own sample clock on the channel tiles", "channels": args.channels,
           "blocks": args.blocks // 8 * 8, "steps": args.steps, "reps": args.reps, "legs": {}}
    for leg in args.legs.split(","):
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg, "--channels", str(args.channels),
               "--blocks", str(args.blocks), "--steps", str(args.steps), "--warmup", str(args.warmup), "--reps", str(args.reps)]
        if args.parent_lib:
            cmd += ["--parent-lib", args.parent_lib]
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
