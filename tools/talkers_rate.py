"""Talker bank rate (dspfx_talkers_*) beside the engine on the same buffers.  Setup: B = 128, tiled W = 256, two alternating input
blocks filled with noise, two output blocks, rooms of --room members, every room's top --top, attack 48 and release 24000 frames on
every channel.  --moved FRACTION first reseats that share of the channels at random (one assign that shuffles the moved channels'
rooms among them, so every room keeps its size): a room's members are then scattered over the block.  At each --channels:
  gated    Talkers.run: block in, block out, the levels and the selection
  meter    Talkers.run(gate=False): block in, the levels and the selection
  engine   Engine.process of [Envelope(48, 24000)] with one detector for all channels: what the bank generalises
  copy     a flat torch copy of the gated run's bytes: one block-unit in, one out
The bank's own bytes per block are two block-units gated and one metering (plus about 45 bytes of tables per channel, not
counted).  Device events around every call, --reps runs after 5 warm-ups, the median; the fraction of peak is those bytes / time /
8 TB/s.  One JSON line per case, then a table.

  python tools/talkers_rate.py [--channels 65536,262144,1048576] [--room 256] [--top 3] [--moved 0.0] [--reps 20]
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
ATTACK, RELEASE = 48.0, 24000.0


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


def reseat(bank, n, groups, fraction, rng):
    """a random room for `fraction` of the channels, in one assign: a shuffle of the moved channels' own rooms, so every room keeps
    its member count"""
    room = bank.room_of()
    moved = np.flatnonzero(rng.random(n) < fraction)
    room[moved] = room[rng.permutation(moved)]
    bank.assign(room)
    assert np.array_equal(bank.room_of(), room)
    return len(moved)


def measure(torch, n, room, top, moved, reps):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(92)
    eng = pkg.Engine(n, B, link_flags=0, device=0, tile_channels=W)
    eng.set_chain([pkg.Envelope(ATTACK, RELEASE)])
    eng.kernels_ready()
    xs = [torch.empty(B * n, dtype=torch.float32, device=dev) for _ in range(2)]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    for i, x in enumerate(xs):
        eng.fill_noise(x, B, 1000 * i)
    bank = pkg.Talkers(n, group_size=room, top=top, tile_channels=W, max_frames=B)
    bank.set_detector(ATTACK, RELEASE)
    n_moved = reseat(bank, n, n // room, moved, rng) if moved > 0 else 0
    gated = timed(torch, lambda i: bank.run(xs[i % 2], B, out=ys[i % 2]), reps)
    meter = timed(torch, lambda i: bank.run(xs[i % 2], B, gate=False), reps)
    torch.cuda.synchronize()
    named = int((bank.talkers() >= 0).sum())
    bank.close()
    engine = timed(torch, lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=B), reps)
    eng.close()
    copy = timed(torch, lambda i: ys[i % 2].copy_(xs[i % 2]), reps)
    unit = B * n * 4
    r = {"channels": n, "room": room, "top": top, "moved": n_moved, "talkers": named, "gated_ms": gated, "gated_bytes": 2 * unit,
         "gated_fraction_of_peak": 2 * unit / (gated * 1e-3) / PEAK, "meter_ms": meter, "meter_bytes": unit,
         "meter_fraction_of_peak": unit / (meter * 1e-3) / PEAK, "engine_ms": engine, "copy_ms": copy}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="65536,262144,1048576")
    ap.add_argument("--room", type=int, default=256)
    ap.add_argument("--top", type=int, default=3)
    ap.add_argument("--moved", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    rows = []
    for n in (int(s) for s in a.channels.split(",")):
        rows.append(measure(torch, n, a.room, a.top, a.moved, a.reps))
        torch.cuda.empty_cache()
    print(f"\ntimes in ms, median of {a.reps}; fractions of the 8 TB/s HBM peak on two block-units (gated) and one (meter)")
    print(f"{'channels':>9} {'moved':>8} {'gated':>8} {'of peak':>8} {'meter':>8} {'of peak':>8} {'engine':>8} {'x engine':>8} {'copy':>8} {'x copy':>7}")
    for r in rows:
        print(f"{r['channels']:>9} {r['moved']:>8} {r['gated_ms']:>8.4f} {r['gated_fraction_of_peak']:>8.3f} {r['meter_ms']:>8.4f} "
              f"{r['meter_fraction_of_peak']:>8.3f} {r['engine_ms']:>8.4f} {r['gated_ms'] / r['engine_ms']:>8.2f} {r['copy_ms']:>8.4f} "
              f"{r['gated_ms'] / r['copy_ms']:>7.2f}")


if __name__ == "__main__":
    main()
