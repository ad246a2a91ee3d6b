"""Channel-rack bank rate (dspfx_racks_*) beside the three-bank sequence it replaces and the uniform engine, on the same buffers.
Setup: B = 128, two alternating input blocks filled with noise of amplitude 2.5, two output blocks.  The chain is HighPass, Gain,
BiQuad, SoftClip Distort, cut to --slots.  At each --channels, each --slots and each --tile:
  none         a fresh bank: a copy through the rack's kernel
  chain        slot t carries the chain's node t with own sliders per channel; beside it the sequence ChannelFilters(1) ->
               ChannelStrips(bands=1) -> ChannelShapers with the same sliders (the banks the chain needs), and the engine of that
               chain with one slider set
  tanh         the chain with Tanh instead of SoftClip in its Distort slot (a chain without one: in its last slot): the
               instantiation with the f64 bodies
  half         the chain on every other span of 256 channels, the rest empty
  clustered    span s of 256 channels carries the chain rotated by s: every wave holds one kind per slot, the kinds differ by wave
  interleaved  channel c carries the chain rotated by c: a lane's channels differ in every slot (--interleaved 0 leaves it out:
               a single-channel store per channel and slot)
  copy         a flat torch copy of the block: one block-unit in, one out
--tile 0 is frame-major; --unaligned 1 also runs `chain` from blocks that start 4 bytes past a 16-byte boundary, so a lane takes
one channel (the scalar-access path).  The fraction of peak is on two block-units (the tables, 37 bytes per channel and slot at
most, are not counted).  Device events around every call, --reps runs after 5 warm-ups, the median.  One JSON line per case set,
then a table.

  python tools/racks_rate.py [--channels 65536,1048576] [--slots 1,2,4] [--tile 256] [--reps 20] [--interleaved 1] [--unaligned 0]
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
RAW = (1.0, -1.8, 0.81, 0.0025, 0.005, 0.0025)


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


def uniform_chain(slots, mode=None):
    return [pkg.HighPass(0.05), pkg.Gain(1.75), pkg.BiQuad(*RAW), pkg.Distort(3.0, pkg.SOFT_CLIP if mode is None else mode)][:slots]


def own_sliders(rng, m, slots, mode=None):
    """the chain with one slider value per channel"""
    raw = np.tile(np.asarray(RAW, F), (m, 1)) * rng.uniform(0.5, 2.0, (m, 1)).astype(F)
    nodes = [pkg.HighPass(rng.uniform(0.01, 0.1, m).astype(F)), pkg.Gain(rng.uniform(0.25, 4.0, m).astype(F)),
             pkg.BiQuad(*[np.ascontiguousarray(raw[:, j]) for j in range(6)]),
             pkg.Distort(rng.uniform(1.0, 8.0, m).astype(F), pkg.SOFT_CLIP if mode is None else mode)]
    return nodes[:slots]


def spans(bank, torch, n, slots, x, y, rotate, every=1):
    """span s of 256 channels: the uniform chain rotated by s (rotate) on every `every`-th span; a run now and then so that the
    stores' staging buffers come back"""
    chain = uniform_chain(4)
    made = 0
    for s in range(0, (n + 255) // 256, every):
        first, count = s * 256, min(256, n - s * 256)
        for t in range(slots):
            bank.set(t, chain[(t + (s if rotate else 0)) % 4], first_channel=first, count=count)
            made += 1
            if made % 2048 == 0:
                bank.run(x, B, out=y)
                torch.cuda.synchronize()


def interleave(torch, bank, n, slots, x, y):
    """the chain rotated by the channel, channel by channel through the C entry point"""
    fp = C.POINTER(C.c_float)
    chain = uniform_chain(4)
    six = []
    for sp in chain:
        v = np.asarray(list(sp.params) + [0.0] * (6 - len(sp.params)), F)
        six.append(((fp * 6)(*[v[j:].ctypes.data_as(fp) for j in range(6)]), v))
    mode = (C.c_uint32 * 1)(pkg.SOFT_CLIP)
    L, h = bank.L, bank.h
    for c in range(n):
        for t in range(slots):
            k = (t + c) % 4
            L.dspfx_racks_set(h, t, chain[k].kind, six[k][0], mode, c, 1)
        if c % 4096 == 4095:
            bank.run(x, B, out=y)
            torch.cuda.synchronize()


def measure(torch, n, slots, tile, reps, interleaved, unaligned):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(94)
    xs = [torch.rand(B * n + 4, dtype=torch.float32, device=dev, generator=gen) * 5 - 2.5 for _ in range(2)]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    rng = np.random.default_rng(95)
    tile = tile if tile and n % tile == 0 else 0
    bank = pkg.ChannelRacks(n, slots=slots, tile_channels=tile, max_frames=B)
    run = lambda off=0: timed(torch, lambda i: bank.run(xs[i % 2][off:off + B * n], B, out=ys[i % 2][off:off + B * n]), reps)     # noqa: E731
    x0, y0 = xs[0][:B * n], ys[0][:B * n]
    r = {"channels": n, "slots": slots, "tile": tile, "bytes": 2 * B * n * 4}
    r["none_ms"] = run()
    nodes = own_sliders(rng, n, slots)
    bank.set_chain(nodes)
    r["chain_ms"] = run()
    if unaligned:
        r["chain_unaligned_ms"] = run(1)
    # the banks the chain needs, with the same sliders, one after the other on the output block
    seq = [pkg.ChannelFilters(n, stages=1, tile_channels=tile, max_frames=B)]
    seq[0].set_high_pass(0, nodes[0].params[0])
    if slots >= 2:
        seq.append(pkg.ChannelStrips(n, bands=1, tile_channels=tile, max_frames=B))
        seq[1].set_gain(nodes[1].params[0])
    if slots >= 3:
        seq[1].set_band(0, np.stack(nodes[2].params, 1))
    if slots >= 4:
        seq.append(pkg.ChannelShapers(n, tile_channels=tile, max_frames=B))
        seq[2].set_distort(nodes[3].params[0], pkg.SOFT_CLIP)

    def sequence(i):
        src = xs[i % 2][:B * n]
        for b in seq:
            b.run(src, B, out=ys[i % 2][:B * n])
            src = ys[i % 2][:B * n]

    r["chain_sequence_ms"] = timed(torch, sequence, reps)
    for b in seq:
        b.close()
    eng = pkg.Engine(n, B, link_flags=0, tile_channels=tile)
    eng.set_chain(uniform_chain(slots))
    r["chain_engine_ms"] = timed(torch, lambda i: eng.process(xs[i % 2][:B * n], out=ys[i % 2][:B * n], n_frames=B), reps)
    eng.close()
    bank.set(slots - 1, pkg.Distort(3.0, pkg.TANH))
    r["tanh_ms"] = run()
    bank.set_chain([])
    spans(bank, torch, n, slots, x0, y0, rotate=False, every=2)
    r["half_ms"] = run()
    bank.set_chain([])
    spans(bank, torch, n, slots, x0, y0, rotate=True)
    r["clustered_ms"] = run()
    if interleaved:
        interleave(torch, bank, n, slots, x0, y0)
        r["interleaved_ms"] = run()
    bank.close()
    r["copy_ms"] = timed(torch, lambda i: ys[i % 2].copy_(xs[i % 2]), reps)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="65536,1048576")
    ap.add_argument("--slots", default="1,2,4")
    ap.add_argument("--tile", default="256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--interleaved", type=int, default=1)
    ap.add_argument("--unaligned", type=int, default=0)
    a = ap.parse_args()
    import torch
    rows = []
    for n in (int(s) for s in a.channels.split(",")):
        for tile in (int(s) for s in a.tile.split(",")):
            for slots in (int(s) for s in a.slots.split(",")):
                rows.append(measure(torch, n, slots, tile, a.reps, a.interleaved, a.unaligned))
                torch.cuda.empty_cache()
    cases = ["none", "chain", "chain_unaligned", "tanh", "half", "clustered", "interleaved", "copy"]
    print(f"\ntimes in ms, median of {a.reps}; (fraction of the 8 TB/s HBM peak on two block-units); [x the sequence of banks, x the uniform engine]")
    for r in rows:
        print(f"{r['channels']} channels, {r['slots']} slots, tile {r['tile']}")
        for c in cases:
            if c + "_ms" not in r:
                continue
            t = r[c + "_ms"]
            more = ""
            if c + "_sequence_ms" in r:
                more = (f"  [sequence {r[c + '_sequence_ms']:.4f} ms, rack x {t / r[c + '_sequence_ms']:.2f}; "
                        f"engine {r[c + '_engine_ms']:.4f} ms, rack x {t / r[c + '_engine_ms']:.2f}]")
            print(f"  {c:>15} {t:>8.4f} ({r['bytes'] / (t * 1e-3) / PEAK:.3f}){more}")


if __name__ == "__main__":
    main()
