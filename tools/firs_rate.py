"""Channel-FIR bank rate (dspfx_firs_*) beside the uniform engine on the same buffers.  Setup: B = 128, two alternating input
blocks filled with noise of amplitude 2.5, two output blocks.  At each --channels, each --taps and each --tile:
  none      a fresh bank: a copy through the bank's kernel
  uniform   one response of T taps everywhere; beside it Engine([Fir(h)], link_flags=0)
  distinct  every channel its own T taps, stored in ranges of 65536 channels per call (the table's bytes are the same as uniform's)
  general   the same with the bank made to take the frames one at a time everywhere (general_only): the general body of the
            kernel against the steady one
  half      the node dropped on every other span of 256 channels
  mixed     channel c carries T = (1 2 3 4 5 8 15 16 17 31 32 33 64)[c % 13] (up to --taps' largest): lanes of different T in every
            wave, so the general body (--mixed 0 leaves it out: one store per channel)
  copy      a flat torch copy of one block
--tile 0 is frame-major.  The bank's own bytes per block: block in, block out, T taps of 8 bytes, T samples of history read and
128 written, per channel.  Device events around every call, --reps runs after 5 warm-ups (5 x 128 frames: every deque is full, so
the waves of `uniform`, `distinct` and `half` take the steady body), the median; the fraction of peak is those bytes / time / 8 TB/s.
One JSON line per case set, then a table.

  python tools/firs_rate.py [--channels 65536,1048576] [--taps 8,16,32,64] [--tile 256] [--reps 20] [--mixed 0]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()

B = 128
PEAK = 8.0e12
LIST = (1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 64)


def timed(torch, fn, reps):
    for i in range(5):
        fn(i)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    for i in range(reps):
        fn(i)
        ev[i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]))


def measure(torch, n, T, tile, reps, mixed):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(94)
    xs = [torch.rand(B * n, dtype=torch.float32, device=dev, generator=gen) * 5 - 2.5 for _ in range(2)]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    rng = np.random.default_rng(95)
    tile = tile if tile and n % tile == 0 else 0
    max_taps = max(T, 64)
    r = {"channels": n, "taps": T, "tile": tile, "bytes": n * (2 * B * 4 + 12 * T + 4 * B), "table_bytes": pkg.firs_plan(n, max_taps)}
    h = rng.uniform(-1.0, 1.0, T)
    for name, general in (("", False), ("general", True)):
        bank = pkg.ChannelFirs(n, max_taps=max_taps, tile_channels=tile, max_frames=B, general_only=general)
        run = lambda: timed(torch, lambda i: bank.run(xs[i % 2], B, out=ys[i % 2]), reps)     # noqa: E731
        if general:
            bank.set_taps(h)
            r["general_ms"] = run()
            bank.close()
            break
        r["none_ms"] = run()
        bank.set_taps(h)
        r["uniform_ms"] = run()
        for c0 in range(0, n, 65536):
            bank.set_taps(rng.uniform(-1.0, 1.0, (min(65536, n - c0), T)), first_channel=c0)
        r["distinct_ms"] = run()
        for s in range(0, (n + 255) // 256, 2):
            bank.drop(s * 256, min(256, n - s * 256))
        r["half_ms"] = run()
        if mixed:
            bank.drop()
            for c in range(n):
                t = min(LIST[c % 13], T)
                bank.set_taps(rng.uniform(-1.0, 1.0, (1, t)), first_channel=c)
                if c % 4096 == 4095:                              # a run now and then brings the small stores' staging buffers back
                    bank.run(xs[0], B, out=ys[0])
                    torch.cuda.synchronize()
            r["mixed_ms"] = run()
        bank.close()
    eng = pkg.Engine(n, B, link_flags=0, tile_channels=tile)
    eng.set_chain([pkg.Fir(h)])
    r["uniform_engine_ms"] = timed(torch, lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=B), reps)
    eng.close()
    r["copy_ms"] = timed(torch, lambda i: ys[i % 2].copy_(xs[i % 2]), reps)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="65536,1048576")
    ap.add_argument("--taps", default="8,16,32,64")
    ap.add_argument("--tile", default="256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mixed", type=int, default=0)
    a = ap.parse_args()
    import torch
    rows = []
    for n in (int(s) for s in a.channels.split(",")):
        for tile in (int(s) for s in a.tile.split(",")):
            for T in (int(s) for s in a.taps.split(",")):
                rows.append(measure(torch, n, T, tile, a.reps, a.mixed))
                torch.cuda.empty_cache()
    cases = ["none", "uniform", "distinct", "general", "half", "mixed", "copy"]
    print(f"\ntimes in ms, median of {a.reps}; (fraction of the 8 TB/s HBM peak on the bank's own bytes); [x the uniform engine]")
    for r in rows:
        print(f"{r['channels']} channels, {r['taps']} taps, tile {r['tile']}, tables {r['table_bytes'] / 2**20:.0f} MiB")
        for c in cases:
            if c + "_ms" not in r:
                continue
            t = r[c + "_ms"]
            eng = f"  [engine {r[c + '_engine_ms']:.4f} ms, bank x {t / r[c + '_engine_ms']:.2f}]" if c + "_engine_ms" in r else ""
            print(f"  {c:>10} {t:>8.4f} ({r['bytes'] / (t * 1e-3) / PEAK:.3f}){eng}")


if __name__ == "__main__":
    main()
