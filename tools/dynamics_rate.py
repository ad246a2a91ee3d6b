"""Channel-dynamics bank rate (dspfx_dynamics_*) beside the talker bank on the same buffers.  Setup: B = 128, tiled W = 256, two
alternating input blocks filled with noise, two output blocks, a third block as the key; every channel carries a node unless
--present FRACTION says otherwise (the channels without one are drawn at random, in runs of 64), thresholds, makeups, attacks and releases drawn
per channel from small sets.  At each --channels:
  plain    ChannelDynamics.run: block in, block out
  keyed    ChannelDynamics.run(key=..): block and key in, block out
  talkers  a gated Talkers.run (rooms of 256, top 3, attack 48, release 24000): the same two block-units and the same recurrence
  copy     a flat torch copy of the plain run's bytes: one block-unit in, one out
The bank's own bytes per block are two block-units plain and three keyed (plus 29 bytes of tables per channel, not counted).
Device events around every call, --reps runs after 5 warm-ups, the median; the fraction of peak is those bytes / time / 8 TB/s.
One JSON line per case, then a table.

  python tools/dynamics_rate.py [--channels 65536,262144,1048576] [--present 1.0] [--reps 20]
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
THRESHOLDS, MAKEUPS = [0.0125, 0.1, 0.25, 0.5], [1.0, 0.7, 3.0, 8.0]
ATTACKS, RELEASES = [0, 1, 48, 1000], [0, 1, 1000, 24000]


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


def measure(torch, n, present, reps):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(93)
    gen = torch.Generator(device=dev).manual_seed(93)
    xs = [torch.rand(B * n, dtype=torch.float32, device=dev, generator=gen) * 2 - 1 for _ in range(2)]
    key = torch.rand(B * n, dtype=torch.float32, device=dev, generator=gen) * 2 - 1
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    bank = pkg.ChannelDynamics(n, tile_channels=W, max_frames=B)
    bank.set(threshold=rng.choice(THRESHOLDS, n).astype(np.float32), makeup=rng.choice(MAKEUPS, n).astype(np.float32),
             attack=rng.choice(ATTACKS, n).astype(np.float32), release=rng.choice(RELEASES, n).astype(np.float32))
    if present < 1.0:
        for g in np.flatnonzero(rng.random((n + 63) // 64) >= present):
            bank.drop(int(g) * 64, min(64, n - int(g) * 64))
    nodes = int(bank.present().sum())
    plain = timed(torch, lambda i: bank.run(xs[i % 2], B, out=ys[i % 2]), reps)
    keyed = timed(torch, lambda i: bank.run(xs[i % 2], B, out=ys[i % 2], key=key), reps)
    torch.cuda.synchronize()
    turned_down = int((bank.reductions() < 1).sum())
    bank.close()
    talk = pkg.Talkers(n, group_size=min(256, n), top=3, tile_channels=W, max_frames=B)
    talk.set_detector(48.0, 24000.0)
    talkers = timed(torch, lambda i: talk.run(xs[i % 2], B, out=ys[i % 2]), reps)
    talk.close()
    copy = timed(torch, lambda i: ys[i % 2].copy_(xs[i % 2]), reps)
    unit = B * n * 4
    r = {"channels": n, "nodes": nodes, "turned_down": turned_down, "plain_ms": plain, "plain_bytes": 2 * unit,
         "plain_fraction_of_peak": 2 * unit / (plain * 1e-3) / PEAK, "keyed_ms": keyed, "keyed_bytes": 3 * unit,
         "keyed_fraction_of_peak": 3 * unit / (keyed * 1e-3) / PEAK, "talkers_ms": talkers, "copy_ms": copy}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="65536,262144,1048576")
    ap.add_argument("--present", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    rows = []
    for n in (int(s) for s in a.channels.split(",")):
        rows.append(measure(torch, n, a.present, a.reps))
        torch.cuda.empty_cache()
    print(f"\ntimes in ms, median of {a.reps}; fractions of the 8 TB/s HBM peak on two block-units (plain) and three (keyed)")
    print(f"{'channels':>9} {'nodes':>8} {'plain':>8} {'of peak':>8} {'keyed':>8} {'of peak':>8} {'talkers':>8} {'x talk':>7} {'copy':>8} {'x copy':>7}")
    for r in rows:
        print(f"{r['channels']:>9} {r['nodes']:>8} {r['plain_ms']:>8.4f} {r['plain_fraction_of_peak']:>8.3f} {r['keyed_ms']:>8.4f} "
              f"{r['keyed_fraction_of_peak']:>8.3f} {r['talkers_ms']:>8.4f} {r['plain_ms'] / r['talkers_ms']:>7.2f} {r['copy_ms']:>8.4f} "
              f"{r['plain_ms'] / r['copy_ms']:>7.2f}")


if __name__ == "__main__":
    main()
