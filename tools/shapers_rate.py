"""Channel-shaper bank rate (dspfx_shapers_*) beside the uniform engine on the same buffers.  Setup: B = 128, tiled W = 256, two
alternating input blocks filled with noise of amplitude 2.5, two output blocks.  At each --channels:
  softclip   every channel Distort(3, SoftClip); beside it Engine([Distort(3, SoftClip)], link_flags=0)
  tanh       every channel Distort(3, Tanh); beside it that engine
  overdrive  every channel Overdrive(5, 0.7, 0.9); beside it that engine
  chebyshev  every channel Chebyshev(2, 7.5); beside it that engine
  clustered  span s of 256 channels carries pointwise kind s % 10 (the eight Distort modes but Fuzz, Overdrive, Chebyshev): every
             wave of the four-channel kernel holds one kind
  spans64    the same by spans of 64 channels: a wave holds four kinds
  mixed      channel c carries kind c % 13 (the nine modes, Fuzz among them, Overdrive, Chebyshev, none, none): every wave holds
             all of them (--mixed 0 leaves it out: its 240 000 single-channel stores take seconds at 2^20 channels)
  fuzz1      Distort(3, SoftClip) with every hundredth channel Fuzz: the second kernel runs, most of its workgroups leave at once
  none       a fresh bank: a copy through the bank's kernel
  copy       a flat torch copy of the same bytes: one block-unit in, one out
The bank's own bytes per block are two block-units (plus 13 bytes of tables per channel, not counted).  Device events around every
call, --reps runs after 5 warm-ups, the median; the fraction of peak is those bytes / time / 8 TB/s.  One JSON line per channel
count, then a table.

  python tools/shapers_rate.py [--channels 65536,262144,1048576] [--reps 20] [--mixed 1]
"""
import argparse
import ctypes as C
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
POINTWISE = [m for m in range(9) if m != pkg.FUZZ]


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


def spans(bank, n, width):
    s = np.arange(n) // width
    bank.set_distort(3.0, np.asarray(POINTWISE, np.uint32)[s % 8])
    for k in range((n + width - 1) // width):
        first, count = k * width, min(width, n - k * width)
        if k % 10 == 8:
            bank.set_overdrive(5.0, 0.7, 0.9, first_channel=first, count=count)
        elif k % 10 == 9:
            bank.set_chebyshev(2.0, 7.5, first_channel=first, count=count)


def interleave(torch, bank, n, x, y):
    """kind c % 13: the modes in one store, the rest channel by channel through the C entry points, a run now and then so that the
    small stores' staging buffers come back"""
    bank.set_distort(3.0, (np.arange(n) % 13 % 9).astype(np.uint32))
    v = np.asarray([5.0, 0.7, 0.9, 2.0, 7.5], np.float32)
    p = [v[i:].ctypes.data_as(C.POINTER(C.c_float)) for i in range(5)]
    L, h = bank.L, bank.h
    for c0 in range(0, n, 13):
        if c0 + 9 < n:
            L.dspfx_shapers_set_overdrive(h, p[0], p[1], p[2], c0 + 9, 1)
        if c0 + 10 < n:
            L.dspfx_shapers_set_chebyshev(h, p[3], p[4], c0 + 10, 1)
        if c0 + 11 < n:
            L.dspfx_shapers_drop(h, c0 + 11, min(2, n - c0 - 11))
        if (c0 // 13) % 1024 == 1023:
            bank.run(x, B, out=y)
            torch.cuda.synchronize()


def measure(torch, n, reps, mixed):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(94)
    xs = [torch.rand(B * n, dtype=torch.float32, device=dev, generator=gen) * 5 - 2.5 for _ in range(2)]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    bank = pkg.ChannelShapers(n, tile_channels=W if n % W == 0 else 0, max_frames=B)
    run = lambda: timed(torch, lambda i: bank.run(xs[i % 2], B, out=ys[i % 2]), reps)     # noqa: E731
    r = {"channels": n, "bytes": 2 * B * n * 4}
    r["none_ms"] = run()
    uniform = {"softclip": pkg.Distort(3.0, pkg.SOFT_CLIP), "tanh": pkg.Distort(3.0, pkg.TANH), "overdrive": pkg.Overdrive(5.0, 0.7, 0.9),
               "chebyshev": pkg.Chebyshev(2.0, 7.5)}
    for name, node in uniform.items():
        if node.kind == pkg.DISTORT:
            bank.set_distort(node.params[0], node.mode)
        elif node.kind == pkg.OVERDRIVE:
            bank.set_overdrive(*node.params[:3])
        else:
            bank.set_chebyshev(*node.params[:2])
        r[name + "_ms"] = run()
        eng = pkg.Engine(n, B, link_flags=0, tile_channels=bank.tile_channels)
        eng.set_chain([node])
        r[name + "_engine_ms"] = timed(torch, lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=B), reps)
        eng.close()
    spans(bank, n, 256)
    r["clustered_ms"] = run()
    spans(bank, n, 64)
    r["spans64_ms"] = run()
    bank.set_distort(3.0, np.where(np.arange(n) % 100 == 0, pkg.FUZZ, pkg.SOFT_CLIP).astype(np.uint32))
    r["fuzz1_ms"] = run()
    if mixed:
        interleave(torch, bank, n, xs[0], ys[0])
        r["mixed_ms"] = run()
    bank.close()
    r["copy_ms"] = timed(torch, lambda i: ys[i % 2].copy_(xs[i % 2]), reps)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="65536,262144,1048576")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mixed", type=int, default=1)
    a = ap.parse_args()
    import torch
    rows = []
    for n in (int(s) for s in a.channels.split(",")):
        rows.append(measure(torch, n, a.reps, a.mixed))
        torch.cuda.empty_cache()
    cases = ["none", "softclip", "tanh", "overdrive", "chebyshev", "clustered", "spans64", "fuzz1", "mixed", "copy"]
    print(f"\ntimes in ms, median of {a.reps}; (fraction of the 8 TB/s HBM peak on two block-units); [x the uniform engine]")
    for r in rows:
        print(f"{r['channels']} channels")
        for c in cases:
            if c + "_ms" not in r:
                continue
            t = r[c + "_ms"]
            eng = f"  [engine {r[c + '_engine_ms']:.4f} ms, bank x {t / r[c + '_engine_ms']:.2f}]" if c + "_engine_ms" in r else ""
            print(f"  {c:>10} {t:>8.4f} ({r['bytes'] / (t * 1e-3) / PEAK:.3f}){eng}")


if __name__ == "__main__":
    main()
