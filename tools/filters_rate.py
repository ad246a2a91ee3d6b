"""Channel-filter bank rate (dspfx_filters_*) beside the uniform engine on the same buffers.  Setup: B = 128, two alternating input
blocks filled with noise of amplitude 2.5, two output blocks.  At each --channels, each --stages and each --tile:
  none         a fresh bank: a copy through the bank's kernel
  lowpass      every slot LowPass(0.93); beside it Engine([LowPass(0.93)] * stages, link_flags=0)
  highpass     every slot HighPass(0.05); beside it that engine
  envelope     every slot Envelope(5, 64); beside it that engine
  chain        slot t carries (HighPass, LowPass, Envelope, LowPass)[t] with own sliders per channel; beside it the engine of that
               chain with one slider set
  half         the chain on every other span of 256 channels, the rest empty
  clustered    span s of 256 channels carries kind (s + t) % 4 of none / LowPass / HighPass / Envelope in slot t: every wave of the
               four-channel kernel holds one kind per stage
  interleaved  channel c carries kind (c + t) % 4 in slot t: a lane's four channels differ in every stage (--interleaved 0 leaves
               it out: its three single-channel stores per four channels and stage take 11 s per stage at 2^20 channels)
  copy         a flat torch copy of the same bytes: one block-unit in, one out
--tile 0 is frame-major; --unaligned 1 also runs `chain` from blocks that start 4 bytes past a 16-byte boundary, so a lane takes
one channel (the scalar-access path).  The bank's own bytes per block are two block-units (plus 13 bytes of tables per channel
and stage, not counted).  Device events around every call, --reps runs after 5 warm-ups, the median; the fraction of peak is those
bytes / time / 8 TB/s.  One JSON line per case set, then a table.

  python tools/filters_rate.py [--channels 65536,1048576] [--stages 1,2,4] [--tile 256] [--reps 20] [--interleaved 1] [--unaligned 0]
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

B = 128
PEAK = 8.0e12
F = np.float32


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


def set_kind(bank, t, k, first, count):
    if k == 1:
        bank.set_low_pass(t, 0.93, first_channel=first, count=count)
    elif k == 2:
        bank.set_high_pass(t, 0.05, first_channel=first, count=count)
    elif k == 3:
        bank.set_envelope(t, 5.0, 64.0, first_channel=first, count=count)


def set_chain(bank, n, stages, rng, first=0, count=None):
    m = n if count is None else count
    for t in range(stages):
        if t == 0:
            bank.set_high_pass(t, rng.uniform(0.01, 0.1, m).astype(F), first_channel=first)
        elif t == 2:
            bank.set_envelope(t, rng.uniform(0.0, 48.0, m).astype(F), rng.uniform(0.0, 2400.0, m).astype(F), first_channel=first)
        else:
            bank.set_low_pass(t, rng.uniform(0.5, 0.95, m).astype(F), first_channel=first)


def clear(bank, stages):
    for t in range(stages):
        bank.drop(t)


def interleave(torch, bank, n, stages, x, y):
    """kind (c + t) % 4 channel by channel through the C entry points, a run now and then so that the small stores' staging buffers
    come back"""
    v = np.asarray([0.93, 0.05, 5.0, 64.0], F)
    p = [v[i:].ctypes.data_as(C.POINTER(C.c_float)) for i in range(4)]
    L, h = bank.L, bank.h
    for t in range(stages):
        for c in range(n):
            k = (c + t) % 4
            if k == 1:
                L.dspfx_filters_set_low_pass(h, t, p[0], c, 1)
            elif k == 2:
                L.dspfx_filters_set_high_pass(h, t, p[1], c, 1)
            elif k == 3:
                L.dspfx_filters_set_envelope(h, t, p[2], p[3], c, 1)
            if c % 4096 == 4095:
                bank.run(x, B, out=y)
                torch.cuda.synchronize()


def measure(torch, n, stages, tile, reps, interleaved, unaligned):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(94)
    xs = [torch.rand(B * n + 4, dtype=torch.float32, device=dev, generator=gen) * 5 - 2.5 for _ in range(2)]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    rng = np.random.default_rng(95)
    tile = tile if tile and n % tile == 0 else 0
    bank = pkg.ChannelFilters(n, stages=stages, tile_channels=tile, max_frames=B)
    run = lambda off=0: timed(torch, lambda i: bank.run(xs[i % 2][off:off + B * n], B, out=ys[i % 2][off:off + B * n]), reps)     # noqa: E731
    r = {"channels": n, "stages": stages, "tile": tile, "bytes": 2 * B * n * 4}
    r["none_ms"] = run()
    chain = [pkg.HighPass(0.05), pkg.LowPass(0.93), pkg.Envelope(5.0, 64.0), pkg.LowPass(0.5)][:stages]
    for name, k, nodes in (("lowpass", 1, [pkg.LowPass(0.93)] * stages), ("highpass", 2, [pkg.HighPass(0.05)] * stages),
                           ("envelope", 3, [pkg.Envelope(5.0, 64.0)] * stages), ("chain", 0, chain)):
        if k:
            for t in range(stages):
                set_kind(bank, t, k, 0, n)
        else:
            set_chain(bank, n, stages, rng)
        r[name + "_ms"] = run()
        eng = pkg.Engine(n, B, link_flags=0, tile_channels=tile)
        eng.set_chain(nodes)
        r[name + "_engine_ms"] = timed(torch, lambda i: eng.process(xs[i % 2][:B * n], out=ys[i % 2][:B * n], n_frames=B), reps)
        eng.close()
    if unaligned:
        r["chain_unaligned_ms"] = run(1)
    clear(bank, stages)
    for s in range(0, (n + 255) // 256, 2):
        set_chain(bank, n, stages, rng, s * 256, min(256, n - s * 256))
    r["half_ms"] = run()
    clear(bank, stages)
    for t in range(stages):
        for s in range((n + 255) // 256):
            set_kind(bank, t, (s + t) % 4, s * 256, min(256, n - s * 256))
    r["clustered_ms"] = run()
    if interleaved:
        clear(bank, stages)
        interleave(torch, bank, n, stages, xs[0][:B * n], ys[0][:B * n])
        r["interleaved_ms"] = run()
    bank.close()
    r["copy_ms"] = timed(torch, lambda i: ys[i % 2].copy_(xs[i % 2]), reps)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="65536,1048576")
    ap.add_argument("--stages", default="1,2,4")
    ap.add_argument("--tile", default="256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--interleaved", type=int, default=1)
    ap.add_argument("--unaligned", type=int, default=0)
    a = ap.parse_args()
    import torch
    rows = []
    for n in (int(s) for s in a.channels.split(",")):
        for tile in (int(s) for s in a.tile.split(",")):
            for stages in (int(s) for s in a.stages.split(",")):
                rows.append(measure(torch, n, stages, tile, a.reps, a.interleaved, a.unaligned))
                torch.cuda.empty_cache()
    cases = ["none", "lowpass", "highpass", "envelope", "chain", "chain_unaligned", "half", "clustered", "interleaved", "copy"]
    print(f"\ntimes in ms, median of {a.reps}; (fraction of the 8 TB/s HBM peak on two block-units); [x the uniform engine]")
    for r in rows:
        print(f"{r['channels']} channels, {r['stages']} stages, tile {r['tile']}")
        for c in cases:
            if c + "_ms" not in r:
                continue
            t = r[c + "_ms"]
            eng = f"  [engine {r[c + '_engine_ms']:.4f} ms, bank x {t / r[c + '_engine_ms']:.2f}]" if c + "_engine_ms" in r else ""
            print(f"  {c:>15} {t:>8.4f} ({r['bytes'] / (t * 1e-3) / PEAK:.3f}){eng}")


if __name__ == "__main__":
    main()
