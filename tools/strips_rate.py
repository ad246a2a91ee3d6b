"""Channel-strip bank rate (dspfx_strips_*) beside the engine on the same buffers.  Setup: B = 128, tiled W = 256, two alternating
input blocks filled with noise, two output blocks, every node of every channel present (levels and stable BiQuads drawn from a
fixed seed).  At each --channels and each --bands K:
  strips   ChannelStrips.run with K bands
  copy     a flat torch copy of the block's bytes
  gain     Engine.process of [Gain(0.7)]
  chain    Engine.process of [Gain, BiQuad x K] with one set of sliders for all channels: what the bank generalises
The bank's own bytes per block: 8 per sample, plus per channel 20 K of coefficients, 32 K of state (read and written), the level
and the node mask.  Device events around every call, --reps runs after 5 warm-ups, the median; the fraction of peak is the
bank's own bytes / time / 8 TB/s.  One JSON line per case, then a table.

  python tools/strips_rate.py [--channels 65536,262144,1048576] [--bands 1,2,4,8] [--reps 20] [--link-flags 0]
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


def stable_raw6(rng, n):
    r, th = rng.uniform(0.0, 0.95, n), rng.uniform(0.0, np.pi, n)
    a = np.stack([np.ones(n), -2.0 * r * np.cos(th), r * r], 1)
    return np.concatenate([a, rng.uniform(-1.0, 1.0, (n, 3))], 1).astype(np.float32)


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


def measure(torch, n, bands, reps, flags):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(81)
    eng = pkg.Engine(n, B, link_flags=flags, device=0, tile_channels=W)
    eng.set_chain([pkg.Gain(0.7)])
    eng.kernels_ready()
    xs = [torch.empty(B * n, dtype=torch.float32, device=dev) for _ in range(2)]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    for i, x in enumerate(xs):
        eng.fill_noise(x, B, 1000 * i)
    copy = timed(torch, lambda i: ys[i % 2].copy_(xs[i % 2]), reps)
    gain = timed(torch, lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=B), reps)
    raw = stable_raw6(rng, 4096)
    rows = []
    for K in bands:
        bank = pkg.ChannelStrips(n, bands=K, tile_channels=W, max_frames=B, link_flags=flags)
        bank.set_gain(rng.uniform(0.5, 1.5, n).astype(np.float32))
        for b in range(K):
            bank.set_band(b, np.tile(np.roll(raw, b, axis=0), (max(1, n // 4096), 1))[:n])
        ms = timed(torch, lambda i: bank.run(xs[i % 2], B, out=ys[i % 2]), reps)
        bank.close()
        ce = pkg.Engine(n, B, link_flags=flags, device=0, tile_channels=W)
        ce.set_chain([pkg.Gain(0.7)] + [pkg.BiQuad(*[float(q) for q in raw[b]]) for b in range(K)])
        ce.kernels_ready()
        chain = timed(torch, lambda i: ce.process(xs[i % 2], out=ys[i % 2], n_frames=B), reps)
        ce.close()
        own = B * n * 8 + n * (20 * K + 32 * K + 8)
        r = {"channels": n, "bands": K, "link_flags": flags, "ms": ms, "bytes": own, "fraction_of_peak": own / (ms * 1e-3) / PEAK,
             "copy_ms": copy, "gain_ms": gain, "chain_ms": chain}
        print(json.dumps(r), flush=True)
        rows.append(r)
    eng.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="65536,262144,1048576")
    ap.add_argument("--bands", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--link-flags", type=int, default=0)
    a = ap.parse_args()
    import torch
    rows = []
    for n in (int(s) for s in a.channels.split(",")):
        rows += measure(torch, n, [int(s) for s in a.bands.split(",")], a.reps, a.link_flags)
        torch.cuda.empty_cache()
    print(f"\ntimes in ms, median of {a.reps}; fraction of the 8 TB/s HBM peak on the bank's own bytes")
    print(f"{'channels':>9} {'bands':>5} {'strips':>8} {'of peak':>8} {'copy':>8} {'x copy':>7} {'gain':>8} {'x gain':>7} {'chain':>8} {'x chain':>8}")
    for r in rows:
        print(f"{r['channels']:>9} {r['bands']:>5} {r['ms']:>8.4f} {r['fraction_of_peak']:>8.3f} {r['copy_ms']:>8.4f} {r['ms'] / r['copy_ms']:>7.2f} "
              f"{r['gain_ms']:>8.4f} {r['ms'] / r['gain_ms']:>7.2f} {r['chain_ms']:>8.4f} {r['ms'] / r['chain_ms']:>8.2f}")


if __name__ == "__main__":
    main()
