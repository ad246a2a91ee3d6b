"""Output resampler bank rate (dspfx_resample_*) beside the chain5 engine, against the 48 kHz block budget (2.667 ms per 128
frames).  Setup: chain5, B = 128, tiled W = 256, the engine writing straight into the bank's slot.  At each --channels, for each
of 44 100 and 96 000 Hz as f32 mono and as i16 stereo, with device events around each call, median over --reps:
  chain      one chain5 block, Engine.process, written into the slot
  push       the zero-copy push of that block (a host counter)
  pull       one callback's launch: the plan copy and resample_pull (n_out = the device frames of 128 source frames)
  all        chain + push + pull together, its own measurement
  base       the best equivalent without the bank: dspfx_process_pcm to the same format at 48 kHz, no resampling
  copy       a flat device-to-device copy moving the pull's bytes: frames pulled + the 16-frame state read, outputs + state written
One JSON line per case, then a table with pull / copy, and the largest power-of-two channel count whose `all` fits the budget.

  python tools/resample_rate.py [--channels 65536,131072,262144,524288,1048576] [--reps 5]
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
from dsp_stuff_amd import workloads  # noqa: E402

B, W = 128, 256
BUDGET_MS = 1000.0 * B / 48000.0
CASES = [(44100, pkg.SAMPLE_F32, 1), (44100, pkg.SAMPLE_I16, 2), (96000, pkg.SAMPLE_F32, 1), (96000, pkg.SAMPLE_I16, 2)]
NAMES = {pkg.SAMPLE_F32: "f32", pkg.SAMPLE_I16: "i16"}


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(torch, n, hz, fmt, ch, reps):
    dev = torch.device("cuda:0")
    eng = pkg.Engine(n, B, link_flags=3, device=0, tile_channels=W)
    eng.set_chain(workloads.chain5(pkg))
    bank = pkg.Resampler(n, hz, tile_channels=W, slots=4, out_format=fmt, out_channels=ch)
    n_out = -(-B * hz // 48000)                          # 118 (input_len 128; 128 or 129 frames a callback) / 256
    dtype = torch.float32 if fmt == pkg.SAMPLE_F32 else torch.int16
    esz = 4 if fmt == pkg.SAMPLE_F32 else 2
    x = torch.empty(B * n, dtype=torch.float32, device=dev)
    out = torch.empty(n_out * n * ch, dtype=dtype, device=dev)
    pcm = torch.empty(B * n * ch, dtype=dtype, device=dev)
    rec = {k: [] for k in ("chain", "push", "pull", "all", "base", "copy")}
    frame = 0

    def block():
        nonlocal frame
        eng.fill_noise(x, B, frame)
        frame += B
        return bank.slot_tensor()

    s = block()                                          # one block of slack: a 44.1 kHz callback takes 128.4 frames on average
    eng.process(x, out=s, n_frames=B)
    bank.push(s, B)
    for k in range(3):                                   # warm-up: past the interpolator's first frames, every kernel loaded
        s = block()
        eng.process(x, out=s, n_frames=B)
        bank.push(s, B)
        bank.pull(n_out, out=out)
        eng.process_pcm(x, pcm, out_channels=ch, n_frames=B)
    consumed = []
    for rep in range(reps):
        s = block()
        rec["chain"].append(timed(torch, lambda: eng.process(x, out=s, n_frames=B)))
        rec["push"].append(timed(torch, lambda: bank.push(s, B)))
        got = []
        rec["pull"].append(timed(torch, lambda: got.append(bank.pull(n_out, out=out))))
        assert not got[0][2], "underrun in the timed loop"
        consumed.append(got[0][1])
        s2 = block()
        rec["all"].append(timed(torch, lambda: (eng.process(x, out=s2, n_frames=B), bank.push(s2, B), bank.pull(n_out, out=out))))
        rec["base"].append(timed(torch, lambda: eng.process_pcm(x, pcm, out_channels=ch, n_frames=B)))
    pulled = int(np.median(consumed))
    moved = (pulled + 16) * n * 4 + n_out * n * ch * esz + 16 * n * 4
    a = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    b.copy_(a)
    for rep in range(reps):
        rec["copy"].append(timed(torch, lambda: b.copy_(a)))
    torch.cuda.synchronize()
    r = {k: float(np.median(v)) for k, v in rec.items()}
    r.update(channels=n, hz=hz, format=f"{NAMES[fmt]}x{ch}", n_out=n_out, pulled=pulled, pull_bytes=moved,
             pull_over_copy=r["pull"] / r["copy"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="65536,131072,262144,524288,1048576")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    rows = []
    for n in (int(s) for s in a.channels.split(",")):
        for hz, fmt, ch in CASES:
            r = measure(torch, n, hz, fmt, ch, a.reps)
            print(json.dumps(r), flush=True)
            rows.append(r)
            torch.cuda.empty_cache()
    print(f"\nbudget {BUDGET_MS:.3f} ms per 128-frame block; times in ms, median of {a.reps}")
    print(f"{'channels':>9} {'hz':>6} {'format':>6} {'chain':>7} {'push':>6} {'pull':>7} {'all':>7} {'base':>7} {'copy':>7} {'pull/copy':>9}  fits")
    best = {}
    for r in rows:
        fits = r["all"] <= BUDGET_MS
        key = (r["hz"], r["format"])
        if fits:
            best[key] = max(best.get(key, 0), r["channels"])
        print(f"{r['channels']:>9} {r['hz']:>6} {r['format']:>6} {r['chain']:>7.3f} {r['push']:>6.3f} {r['pull']:>7.3f} {r['all']:>7.3f} "
              f"{r['base']:>7.3f} {r['copy']:>7.3f} {r['pull_over_copy']:>9.2f}  {'yes' if fits else 'no'}")
    for key in sorted(set((r["hz"], r["format"]) for r in rows)):
        print(f"{key[0]} Hz {key[1]}: largest channel count measured whose chain + push + pull fits the budget: {best.get(key)}")


if __name__ == "__main__":
    main()
