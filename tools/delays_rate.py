"""Channel-delay bank rate (dspfx_delays_*) beside the engine on the same buffers.  Setup: B = 128, tiled W = 256, two alternating
input blocks filled with noise, two output blocks, rings of --max-seconds (0.02: 960 frames, 3.75 GiB at 2^20 channels), every
channel present with a ring length drawn from 128 .. cap and a decay from -0.9 .. 0.9 (a fixed seed).  At each --channels:
  delays   ChannelDelays.run
  copy     a flat torch copy of the same bytes: two block-units in, two out
  engine   Engine.process of [Reverb(seconds, 0.5)] with one length for all channels: what the bank generalises
  nodeless ChannelDelays.run of a fresh bank: a copy of the block
The bank's own bytes per block are four block-units when every channel carries a node: block in, block out, ring in, ring out
(plus 16 bytes of tables per channel, not counted).  Device events around every call, --reps runs after 10 warm-ups (1280 frames:
every ring has wrapped, no tap is a still-zero one), the median; the fraction of peak is those bytes / time / 8 TB/s.  One JSON
line per case, then a table.

  python tools/delays_rate.py [--channels 65536,262144,1048576] [--max-seconds 0.02] [--reps 20] [--link-flags 0]
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

B, W = 128, 256
PEAK = 8.0e12


def timed(torch, fn, reps):
    for i in range(10):
        fn(i)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    for i in range(reps):
        fn(i)
        ev[i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]))


def measure(torch, n, max_seconds, reps, flags):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(91)
    cap, ring_bytes = pkg.delays_plan(n, max_seconds)
    eng = pkg.Engine(n, B, link_flags=flags, device=0, tile_channels=W)
    eng.set_chain([pkg.Reverb(max_seconds / 2, 0.5)])
    eng.kernels_ready()
    xs = [torch.empty(B * n, dtype=torch.float32, device=dev) for _ in range(2)]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    for i, x in enumerate(xs):
        eng.fill_noise(x, B, 1000 * i)
    engine = timed(torch, lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=B), reps)
    eng.close()
    bank = pkg.ChannelDelays(n, max_seconds, tile_channels=W, max_frames=B, link_flags=flags)
    nodeless = timed(torch, lambda i: bank.run(xs[i % 2], B, out=ys[i % 2]), reps)
    lengths = rng.integers(128, cap + 1, n)
    bank.set_delay(((lengths + 0.5) / 48000.0).astype(np.float32), rng.uniform(-0.9, 0.9, n).astype(np.float32))
    assert np.array_equal(bank.lengths(), lengths)
    ms = timed(torch, lambda i: bank.run(xs[i % 2], B, out=ys[i % 2]), reps)
    bank.close()
    torch.cuda.empty_cache()
    a, b = torch.cat(xs), torch.empty(2 * B * n, dtype=torch.float32, device=dev)
    copy = timed(torch, lambda i: b.copy_(a), reps)
    own = 4 * B * n * 4
    r = {"channels": n, "cap": cap, "ring_bytes": ring_bytes, "link_flags": flags, "ms": ms, "bytes": own, "fraction_of_peak": own / (ms * 1e-3) / PEAK,
         "copy_ms": copy, "engine_ms": engine, "nodeless_ms": nodeless}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="65536,262144,1048576")
    ap.add_argument("--max-seconds", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--link-flags", type=int, default=0)
    a = ap.parse_args()
    import torch
    rows = []
    for n in (int(s) for s in a.channels.split(",")):
        rows.append(measure(torch, n, a.max_seconds, a.reps, a.link_flags))
        torch.cuda.empty_cache()
    print(f"\ntimes in ms, median of {a.reps}; fraction of the 8 TB/s HBM peak on four block-units")
    print(f"{'channels':>9} {'cap':>5} {'delays':>8} {'of peak':>8} {'copy':>8} {'x copy':>7} {'engine':>8} {'x engine':>8} {'nodeless':>8}")
    for r in rows:
        print(f"{r['channels']:>9} {r['cap']:>5} {r['ms']:>8.4f} {r['fraction_of_peak']:>8.3f} {r['copy_ms']:>8.4f} {r['ms'] / r['copy_ms']:>7.2f} "
              f"{r['engine_ms']:>8.4f} {r['ms'] / r['engine_ms']:>8.2f} {r['nodeless_ms']:>8.4f}")


if __name__ == "__main__":
    main()
