"""Channel-blend bank rate (dspfx_blends_*) beside the uniform engine on the same buffers.  Setup: B = 128, tiled W = 256, two
alternating blocks of a, of the second input and of the output; the bus block has one channel per room of --room channels.  At each
--channels, with the second input --mode block, bus or both:
  mix        every channel Mix(0.3); in block mode beside it Engine([Mix(0.3)], link_flags=0) with side
  add        every channel Add; in block mode beside it Engine([Add()], link_flags=0) with side
  send       the mix bank with a send of 0.5 on every channel
  mixed      span s of 256 channels carries kind s % 3 (none, Add, Mix)
  present    the mix bank with only the first --present of the channels carrying a node: the other lanes read neither the second
             input nor the control block
  ratio      the mix bank with the ratio control block: one more block-unit read
  none       a fresh bank: a copy through the bank's kernel
  copy       a flat torch copy: one block-unit in, one out
In bus mode every case runs with --ids contiguous (rooms are whole spans of --room channels: whole waves share a bus id), shuffled
(a random permutation of those ids: every channel gathers its own), or both.
The bank's own bytes per run are the block-units it reads and writes (plus 13 bytes of tables per channel and the bus block, not
counted): three in block mode, two in bus mode and without a second input, one more with the control block; lanes without a node
move two.  Device events around every call, --reps runs after 5 warm-ups, the median; the fraction of peak is those bytes / time /
8 TB/s.  One JSON line per channel count and mode, then a table.

  python tools/blends_rate.py [--channels 65536,262144,1048576] [--mode both] [--ids both] [--present 0.5] [--room 256] [--reps 20]
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
CASES = ["none", "mix", "add", "send", "mixed", "present", "ratio"]


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


def measure(torch, n, mode, ids, present, room, reps):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(96)
    xs = [torch.rand(B * n, dtype=torch.float32, device=dev, generator=gen) * 2 - 1 for _ in range(2)]
    ss = [torch.rand(B * n, dtype=torch.float32, device=dev, generator=gen) * 2 - 1 for _ in range(2)]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    G = (n + room - 1) // room
    bus = torch.rand(B * G, dtype=torch.float32, device=dev, generator=gen) * 2 - 1
    tile = W if n % W == 0 else 0
    bank = pkg.ChannelBlends(n, buses=G, tile_channels=tile, max_frames=B)
    of = (np.arange(n) // room).astype(np.uint32)
    bank.assign(np.random.default_rng(4).permutation(of) if ids == "shuffled" else of)
    second = (lambda i: dict(b=ss[i % 2])) if mode == "block" else (lambda i: dict(bus=bus))
    run = lambda ctl=False: timed(torch, lambda i: bank.run(xs[i % 2], B, out=ys[i % 2], ratio=ss[(i + 1) % 2] if ctl else None, **second(i)), reps)   # noqa: E731
    side_units = 1 if mode == "block" else 0
    r = {"channels": n, "mode": mode, "ids": ids if mode == "bus" else None, "rooms": G, "unit_bytes": B * n * 4, "units": {}}

    def case(name, units, ctl=False):
        r[name + "_ms"] = run(ctl)
        r["units"][name] = units

    case("none", 2)
    bank.set_mix(0.3)
    case("mix", 2 + side_units)
    case("ratio", 3 + side_units, ctl=True)
    bank.set_send(0.5)
    case("send", 2 + side_units)
    bank.set_send(None)
    k = int(n * present) // 4 * 4
    bank.drop(k, n - k)
    case("present", 2 + side_units * k / n)
    bank.set_add()
    case("add", 2 + side_units)
    for sp in range(0, (n + 255) // 256):                 # span sp of 256 channels: kind sp % 3 (none, Add, Mix)
        c0, m = sp * 256, min(256, n - sp * 256)
        if sp % 3 == 0:
            bank.drop(c0, m)
        elif sp % 3 == 2:
            bank.set_mix(0.3, c0, m)
    case("mixed", 2 + side_units * 2 / 3)
    bank.close()
    if mode == "block":
        for name, node in (("mix", pkg.Mix(0.3)), ("add", pkg.Add())):
            eng = pkg.Engine(n, B, link_flags=0, tile_channels=tile)
            eng.set_chain([node])
            r[name + "_engine_ms"] = timed(torch, lambda i: eng.process(xs[i % 2], out=ys[i % 2], side=ss[i % 2], n_frames=B), reps)
            eng.close()
    r["copy_ms"] = timed(torch, lambda i: ys[i % 2].copy_(xs[i % 2]), reps)
    r["units"]["copy"] = 2
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="65536,262144,1048576")
    ap.add_argument("--mode", default="both", choices=["block", "bus", "both"])
    ap.add_argument("--ids", default="both", choices=["contiguous", "shuffled", "both"])
    ap.add_argument("--present", type=float, default=0.5)
    ap.add_argument("--room", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    runs = []
    for m in (["block", "bus"] if a.mode == "both" else [a.mode]):
        for i in ((["contiguous", "shuffled"] if a.ids == "both" else [a.ids]) if m == "bus" else ["contiguous"]):
            runs.append((m, i))
    rows = []
    for n in (int(s) for s in a.channels.split(",")):
        for m, i in runs:
            rows.append(measure(torch, n, m, i, a.present, a.room, a.reps))
            torch.cuda.empty_cache()
    print(f"\ntimes in ms, median of {a.reps}; (fraction of the 8 TB/s HBM peak on the run's own block-units); [x the uniform engine]")
    for r in rows:
        print(f"{r['channels']} channels, {r['mode']} mode" + (f", {r['rooms']} rooms, {r['ids']} ids" if r["mode"] == "bus" else ""))
        for c in CASES + ["copy"]:
            t = r[c + "_ms"]
            eng = f"  [engine {r[c + '_engine_ms']:.4f} ms, bank x {t / r[c + '_engine_ms']:.2f}]" if c + "_engine_ms" in r else ""
            print(f"  {c:>10} {t:>8.4f} ({r['units'][c] * r['unit_bytes'] / (t * 1e-3) / PEAK:.3f} on {r['units'][c]:g} units){eng}")


if __name__ == "__main__":
    main()
