"""Channel-canceller bank rate (dspfx_cancel_*).  Setup: B = 128, two alternating triples of blocks (mic, ref, out), mic and ref
noise of amplitude 1.  At each --channels, each --taps and each --tile:
  none      a fresh bank: a copy of mic through the bank's kernel
  adapting  T taps everywhere, every channel adapting, a delay of its own per channel (0 .. --delay)
  frozen    the same with adapt off everywhere: the filter alone
  half      the node dropped on every other span of 256 channels (adapting)
  general   the same bank made to take the frames one at a time everywhere (general_only): the general body of the kernel against
            the fast one
  mixed     channel c carries T = (1 2 3 4 5 8 15 16 17 31 32 33 64)[c % 13] (up to --taps' largest): lanes of different T in every
            wave, so the general body
  copy      a flat torch copy of one block
--tile 0 is frame-major.  The bank's own bytes per block and channel: mic and ref in, out, T weights read and written, 128 ring rows
written and 128 + T - 1 read, 4 bytes each.  Device events around every call, --reps runs after 5 warm-ups, the median; the fraction
of peak is those bytes / time / 8 TB/s.  One JSON line per case set, then a table.

  python tools/cancel_rate.py [--channels 65536,1048576] [--taps 8,16,32,64] [--tile 256] [--delay 255] [--reps 20] [--mixed 1]
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


def measure(torch, n, T, tile, max_delay, reps, mixed):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(94)
    ms = [torch.rand(B * n, dtype=torch.float32, device=dev, generator=gen) * 2 - 1 for _ in range(2)]
    rs = [torch.rand(B * n, dtype=torch.float32, device=dev, generator=gen) * 2 - 1 for _ in range(2)]
    ys = [torch.empty_like(ms[0]) for _ in range(2)]
    tile = tile if tile and n % tile == 0 else 0
    max_taps = max(T, 64)
    delay = (np.arange(n, dtype=np.int64) * 37) % (max_delay + 1)
    r = {"channels": n, "taps": T, "tile": tile, "bytes": n * 4 * (3 * B + 2 * T + B + B + T - 1),
         "table_bytes": pkg.cancel_plan(n, max_taps, max_delay)}
    for general in (False, True):
        bank = pkg.ChannelCancellers(n, max_taps=max_taps, max_delay=max_delay, tile_channels=tile, max_frames=B, general_only=general)
        run = lambda: timed(torch, lambda i: bank.run(ms[i % 2], B, ref=rs[i % 2], out=ys[i % 2]), reps)     # noqa: E731
        if general:
            bank.set(taps=T, delay=delay)
            r["general_ms"] = run()
            bank.close()
            break
        r["none_ms"] = run()
        bank.set(taps=T, delay=delay)
        r["adapting_ms"] = run()
        bank.set(adapt=False)
        r["frozen_ms"] = run()
        bank.set(adapt=True)
        for s in range(0, (n + 255) // 256, 2):
            bank.drop(s * 256, min(256, n - s * 256))
        r["half_ms"] = run()
        if mixed:
            bank.drop()
            bank.set(taps=np.minimum(np.array(LIST)[np.arange(n) % 13], T), delay=delay)
            r["mixed_ms"] = run()
        bank.close()
    r["copy_ms"] = timed(torch, lambda i: ys[i % 2].copy_(ms[i % 2]), reps)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="65536,1048576")
    ap.add_argument("--taps", default="8,16,32,64")
    ap.add_argument("--tile", default="256")
    ap.add_argument("--delay", type=int, default=255)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mixed", type=int, default=1)
    a = ap.parse_args()
    import torch
    rows = []
    for n in (int(s) for s in a.channels.split(",")):
        for tile in (int(s) for s in a.tile.split(",")):
            for T in (int(s) for s in a.taps.split(",")):
                rows.append(measure(torch, n, T, tile, a.delay, a.reps, a.mixed))
                torch.cuda.empty_cache()
    cases = ["none", "adapting", "frozen", "half", "general", "mixed", "copy"]
    print(f"\ntimes in ms, median of {a.reps}; (fraction of the 8 TB/s HBM peak on the bank's own bytes)")
    for r in rows:
        print(f"{r['channels']} channels, {r['taps']} taps, tile {r['tile']}, tables {r['table_bytes'] / 2**20:.0f} MiB")
        for c in cases:
            if c + "_ms" in r:
                t = r[c + "_ms"]
                print(f"  {c:>10} {t:>8.4f} ({r['bytes'] / (t * 1e-3) / PEAK:.3f})")


if __name__ == "__main__":
    main()
