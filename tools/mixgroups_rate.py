"""Mix-group bank rate (dspfx_mixgroups_*) beside a [Gain(1.0)] chain on the same buffers.  Setup: B = 128, tiled W = 256, two
alternating input blocks filled with noise, every channel with a fader stored (the kernel reads the table).  At each --channels:
  (a)      uniform groups of 256 channels (one room per tile)
  (b)      a ragged table drawn from a fixed seed, sizes 1 .. channels / 4 (mixgroups_ref.ragged_table's rule)
  nogain   (a) with no fader stored
  chain    Engine.process of [Gain(1.0)], which reads AND writes the block: twice the bank's bytes
  returns  MixGroups.returns (every channel's room minus itself) into a third buffer: run's read, one more read and one write of
           the block, three times the bank's bytes
--seating S (contiguous | movers | random) reseats case (a) through MixGroups.assign first, so that the mapped kernels run:
contiguous is the create table assigned unchanged, movers swaps one channel in 64 with a channel of another room, random
permutes the rooms over the channels; the row's "pieces" is the seating's piece count (0 without --seating: no map).
Device events around every call, --reps runs after 5 warm-ups, the median; the fraction of peak is block bytes / time / 8 TB/s.
One JSON line per case, then a table.

  python tools/mixgroups_rate.py [--channels 65536,262144,1048576] [--reps 20] [--seating contiguous|movers|random]
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


def ragged_table(n, seed, max_size):
    rng = np.random.default_rng(seed)
    gs = [0]
    while gs[-1] < n:
        gs.append(min(n, gs[-1] + max(1, int(round(float(np.exp(rng.uniform(0.0, np.log(max_size)))))))))
    return np.asarray(gs, np.uint64)


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


def seating_of(name, n):
    """the room of every channel for case (a), reseated"""
    rng = np.random.default_rng(71)
    room = (np.arange(n) // 256).astype(np.uint32)
    if name == "movers":
        pick = np.arange(0, n, 64) + rng.integers(0, 64, n // 64)
        partner = np.roll(pick, 7)
        room[pick], room[partner] = room[partner].copy(), room[pick].copy()
    elif name == "random":
        room = rng.permutation(room)
    return room


def measure(torch, n, reps, seating=None):
    dev = torch.device("cuda:0")
    eng = pkg.Engine(n, B, link_flags=0, device=0, tile_channels=W)
    eng.set_chain([pkg.Gain(1.0)])
    eng.kernels_ready()
    xs = [torch.empty(B * n, dtype=torch.float32, device=dev) for _ in range(2)]
    y = torch.empty_like(xs[0])
    for i, x in enumerate(xs):
        eng.fill_noise(x, B, 1000 * i)
    rows = []
    chain = timed(torch, lambda i: eng.process(xs[i % 2], out=y, n_frames=B), reps)
    tables = {"a": np.arange(0, n + 1, 256, dtype=np.uint64), "b": ragged_table(n, 20260101, n // 4)}
    for case, table, fader in (("a", tables["a"], True), ("b", tables["b"], True), ("nogain", tables["a"], False)):
        mg = pkg.MixGroups(n, group_start=table, tile_channels=W, max_frames=B)
        if fader:
            mg.set_gains(np.random.default_rng(61).uniform(0.0, 4.0, n).astype(np.float32))
        if seating and case != "b":
            mg.assign(seating_of(seating, n))
        buses = torch.empty((B, mg.groups), dtype=torch.float32, device=dev)
        ms = timed(torch, lambda i: mg.run(xs[i % 2], B, out=buses), reps)
        ret = timed(torch, lambda i: mg.returns(xs[i % 2], B, out=y), reps)
        r = {"channels": n, "case": case, "groups": mg.groups, "ms": ms, "fraction_of_peak": B * n * 4 / (ms * 1e-3) / PEAK,
             "returns_ms": ret, "returns_fraction_of_peak": 3 * B * n * 4 / (ret * 1e-3) / PEAK,
             "chain_ms": chain, "chain_fraction_of_peak": 2 * B * n * 4 / (chain * 1e-3) / PEAK, "depth_max": int(mg.depth().max()),
             "seating": seating if case != "b" else None, "pieces": mg.pieces()}
        print(json.dumps(r), flush=True)
        rows.append(r)
        mg.close()
    eng.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="65536,262144,1048576")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seating", choices=["contiguous", "movers", "random"], default=None,
                    help="reseat the uniform cases through assign(): the mapped kernels")
    a = ap.parse_args()
    import torch
    rows = []
    for n in (int(s) for s in a.channels.split(",")):
        rows += measure(torch, n, a.reps, a.seating)
        torch.cuda.empty_cache()
    print(f"\ntimes in ms, median of {a.reps}; fractions of the 8 TB/s HBM peak")
    print(f"{'channels':>9} {'case':>7} {'groups':>7} {'bank':>8} {'of peak':>8} {'chain':>8} {'of peak':>8} {'bank/chain':>10} "
          f"{'returns':>8} {'of peak':>8} {'pieces':>8}")
    for r in rows:
        print(f"{r['channels']:>9} {r['case']:>7} {r['groups']:>7} {r['ms']:>8.4f} {r['fraction_of_peak']:>8.3f} {r['chain_ms']:>8.4f} "
              f"{r['chain_fraction_of_peak']:>8.3f} {r['ms'] / r['chain_ms']:>10.2f} {r['returns_ms']:>8.4f} "
              f"{r['returns_fraction_of_peak']:>8.3f} {r['pieces']:>8}")


if __name__ == "__main__":
    main()
