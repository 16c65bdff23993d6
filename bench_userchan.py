#!/usr/bin/env python3
"""What the per-user channel emulator (mcrx_hip_userchan_*, csrc/userchan.hip) costs on the transmitter's channel tiles.  A secondary
measurement -- bench.py holds the headline metric.

    python bench_userchan.py [--channels C --blocks B --steps K --warmup W --reps R --out FILE --no-pipeline]

The tiles of the 512-channel slab (default: 202 848 blocks x 512 channels, 0.83 GB in and 0.83 GB out) through handles of one process,
into an output buffer allocated beforehand, through the C-ABI on a side stream, HIP events around --steps calls; the median of --reps
repetitions with its spread (max - min) / median.  Legs:
    copy              a device-to-device copy of the output's bytes: the byte bound (8 B in + 8 B out a sample)
    T1                one ray at delay 0, no rotation
    T3                three rays a channel (delays differ from channel to channel, odd and even), no rotation
    T3_even, T3_odd   three rays, every delay even (16-byte loads only) / odd (8-byte loads only), no rotation
    T3_rot, T4_rot    three / four rays, every channel with its own oscillator
    torch_3ray_rot    the T3_rot case composed in torch on a channel-major copy of the samples: three shifted slices (ONE delay per ray
                      for all channels -- per-channel delays would be a loop over channels), a complex multiply by a precomputed phasor
                      tensor, the gain
    tx_plain, tx_userchan   traffic_tiles + synthesize_tiles, and traffic_tiles + apply_tiles + synthesize_tiles, for the slab of
                      bench.py's headline (16 frames of 1200 bytes on each of 512 channels); skipped with --no-pipeline
Every emulator leg reports ms a call, its algorithmic GB (input once, output once) and that traffic as a fraction of 8 TB/s (HBM peak).
One JSON line; --out also writes it to a file.  Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8.0e12


def report(samples, ms):
    med = statistics.median(ms)
    gb = samples * 16 / 1e9
    return {"ms": round(med, 4), "reps_ms": [round(v, 4) for v in ms], "spread": round((max(ms) - min(ms)) / med, 4),
            "algorithmic_gb": round(gb, 4), "gsamples_per_s": round(samples / med / 1e6, 2),
            "fraction_of_8_tb_per_s": round(gb * 1e9 / (med * 1e-3) / PEAK_BYTES_PER_S, 4)}


def channels_of(Cn, rays, rot, M=64, parity=None):
    """Cn users: `rays` rays each, the second at 1 + c % 3, a timing offset c % 13, levels over 30 dB, oscillators over +-0.45 spacings.
    parity 0 / 1: every delay of the table even / odd instead (rays at 0, 2, 4, 8 behind a timing offset 2 (c % 7) + parity) -- the
    16-byte and the 8-byte loads on their own"""
    from __graft_entry__ import load_product
    prod = load_product()
    table = [(0, 1.0), (1, 0.25 - 0.15j), (4, -0.10 + 0.15j), (9, 0.05 + 0.05j)]
    out = []
    for c in range(Cn):
        taps = [(d + (c % 3 if i == 1 else 0), a) for i, (d, a) in enumerate(table[:rays])]
        ch = dict(taps=taps, gain_db=-30.0 * (c % 16) / 15.0, delay=(c % 13) if rays > 1 else 0)
        if parity is not None:
            ch.update(taps=[(d, a) for d, (_, a) in zip((0, 2, 4, 8), taps)], delay=2 * (c % 7) + parity)
        if rot:
            ch.update(cfo_step=prod.userchan_cfo_step(0.9 * ((c * 37) % 101) / 100.0 - 0.45, M), phase0=(c * 0x9E3779B9) % (1 << 32))
        out.append(ch)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=202848)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "userchan.json"))
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_product
    assert torch.cuda.is_available(), "bench_userchan.py needs the GPU"
    prod = load_product()
    L = prod.lib()
    dev = torch.device("cuda", 0)
    Cn, nb, lead = args.channels, args.blocks // 8 * 8, 32
    n = nb * Cn
    gen = torch.Generator(device=dev)
    gen.manual_seed(16)
    d_x = torch.view_as_complex(torch.randn(((lead + nb) * Cn, 2), generator=gen, device=dev))
    d_y = torch.empty(n, dtype=torch.complex64, device=dev)
    side = torch.cuda.Stream(device=dev)

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

    out = {"metric": "per-user channel emulator on the channel tiles", "device": torch.cuda.get_device_name(0), "channels": Cn, "blocks": nb,
           "lead_blocks": lead, "steps": args.steps, "reps": args.reps, "legs": {}}
    src = d_x[lead * Cn:]
    out["legs"]["copy"] = report(n, measure(lambda: d_y.copy_(src)))
    for name, rays, rot, parity in (("T1", 1, False, None), ("T3", 3, False, None), ("T3_even", 3, False, 0), ("T3_odd", 3, False, 1),
                                    ("T3_rot", 3, True, None), ("T4_rot", 4, True, None)):
        uc = prod.userchan(channels=channels_of(Cn, rays, rot, parity=parity))
        assert uc.lead_blocks <= lead

        def call(uc=uc):
            rc = L.mcrx_hip_userchan_apply_tiles(uc._h, C.c_void_p(d_x.data_ptr()), 0, nb, lead, C.c_void_p(d_y.data_ptr()), C.c_void_p(side.cuda_stream))
            if rc != prod.MCRX_OK:
                raise RuntimeError("mcrx_hip_userchan_apply_tiles failed (%d): %s" % (rc, L.mcrx_hip_userchan_last_error().decode()))
        out["legs"][name] = report(n, measure(call))
        out["legs"][name].update(rays=rays, rotation=rot)
        uc.close()

    # the torch composition of T3_rot: channel-major samples, one delay per ray, the phasors precomputed
    chans = channels_of(Cn, 3, True)
    xc = d_x.view(-1, Cn, 8).permute(1, 0, 2).reshape(Cn, -1).contiguous()
    del d_x
    a = [torch.tensor([complex(ch["taps"][i][1]) for ch in chans], dtype=torch.complex64, device=dev)[:, None] for i in range(3)]
    g = torch.tensor([10.0 ** (ch["gain_db"] / 20.0) for ch in chans], dtype=torch.float32, device=dev)[:, None]
    step = torch.tensor([ch["cfo_step"] for ch in chans], dtype=torch.float64, device=dev)[:, None]
    ph0 = torch.tensor([ch["phase0"] for ch in chans], dtype=torch.float64, device=dev)[:, None]
    phasor = torch.empty((Cn, nb), dtype=torch.complex64, device=dev)
    for b0 in range(0, nb, 1 << 15):                                    # (in pieces: the float64 phases of the whole slab are 0.8 GB)
        b = torch.arange(b0, min(b0 + (1 << 15), nb), dtype=torch.float64, device=dev)[None, :]
        th = torch.remainder(ph0 + step * b, 4294967296.0) * (2.0 * 3.141592653589793 / 4294967296.0)
        phasor[:, b0:b0 + th.shape[1]] = torch.polar(torch.ones_like(th), th).to(torch.complex64)
    d1, d2 = 2, 4
    yc = d_y.view(Cn, nb)

    def torch_3ray_rot():
        y = a[0] * xc[:, lead:]
        y += a[1] * xc[:, lead - d1:lead - d1 + nb]
        y += a[2] * xc[:, lead - d2:lead - d2 + nb]
        y *= phasor
        torch.mul(y, g, out=yc)
    out["legs"]["torch_3ray_rot"] = report(n, measure(torch_3ray_rot))
    del xc, phasor, yc

    if not args.no_pipeline and Cn == 512:
        N, M, cp, taper, frames, plen = 512, 64, 8, 4, 16, 1200
        tx = prod.multichanneltx(N, M, cp, taper)
        tr = tx.traffic(0, N, frames, plen)
        blocks, ls = tr.blocks, prod.USERCHAN_SYNTH_LEAD
        uc = prod.userchan(channels=channels_of(N, 3, True))
        lu = uc.lead_blocks
        tiles = torch.empty((ls + lu + blocks) * N, dtype=torch.complex64, device=dev)
        mid = d_y if int(d_y.numel()) >= (ls + blocks) * N else torch.empty((ls + blocks) * N, dtype=torch.complex64, device=dev)
        iq = torch.empty(blocks * 2 * N, dtype=torch.complex64, device=dev)
        st = C.c_void_p(side.cuda_stream)

        def chk(rc, what):
            if rc != prod.MCRX_OK:
                raise RuntimeError("%s failed (%d)" % (what, rc))

        def tx_plain():
            chk(L.mctx_hip_traffic_tiles(tr._t, -ls, ls + blocks, C.c_void_p(tiles.data_ptr()), st), "traffic_tiles")
            chk(L.mctx_hip_synthesize_tiles(tx._h, C.c_void_p(tiles.data_ptr()), 1, 0, blocks, ls, 0, 1.0 / N, C.c_void_p(iq.data_ptr()), st), "synthesize_tiles")

        def tx_userchan():
            chk(L.mctx_hip_traffic_tiles(tr._t, -(ls + lu), ls + lu + blocks, C.c_void_p(tiles.data_ptr()), st), "traffic_tiles")
            chk(L.mcrx_hip_userchan_apply_tiles(uc._h, C.c_void_p(tiles.data_ptr()), -ls, ls + blocks, lu, C.c_void_p(mid.data_ptr()), st), "apply_tiles")
            chk(L.mctx_hip_synthesize_tiles(tx._h, C.c_void_p(mid.data_ptr()), 1, 0, blocks, ls, 0, 1.0 / N, C.c_void_p(iq.data_ptr()), st), "synthesize_tiles")
        ms_p, ms_u = [], []
        timed(tx_plain, args.warmup); timed(tx_userchan, args.warmup)
        for _ in range(args.reps):                                      # alternating: both see the same machine
            ms_p.append(timed(tx_plain, args.steps)); ms_u.append(timed(tx_userchan, args.steps))
        for name, ms in (("tx_plain", ms_p), ("tx_userchan", ms_u)):
            med = statistics.median(ms)
            out["legs"][name] = {"ms": round(med, 4), "reps_ms": [round(v, 4) for v in ms], "spread": round((max(ms) - min(ms)) / med, 4),
                                 "blocks": blocks, "wideband_gsamples_per_s": round(blocks * 2 * N / med / 1e6, 2)}
        uc.close(); tr.close(); tx.close()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
