"""Pitch Detector bank rate (dspfx_pitch_*) beside the chain5 engine, against the 48 kHz block budget (2.667 ms per 128 frames).
At each --channels, with device events around each call, median over --reps:
  chain        one chain5 block, Engine.process, written straight into the bank's slot
  push_slot    the zero-copy push of that block (no detection due)
  push_copy    a copying push of one 128-frame block (no detection due)
  detect       the push that runs a detection (slot path: the launch of pitch_detect alone)
  chain+detect the block on which a window falls due, chain and detection together
One JSON line per channel count, then a table.  The largest power-of-two channel count whose chain+detect fits the budget
is reported at the end.

  python tools/pitch_rate.py [--channels 65536,131072,262144,524288,1048576] [--reps 5]
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

B = 128
BUDGET_MS = 1000.0 * B / 48000.0


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(torch, n, reps):
    dev = torch.device("cuda:0")
    eng = pkg.Engine(n, B, link_flags=3, device=0)
    eng.set_chain(workloads.chain5(pkg))
    bank = pkg.PitchBank(n)
    x = torch.empty((B, n), dtype=torch.float32, device=dev)
    blk = torch.randn((B, n), dtype=torch.float32, device=dev)
    rec = {k: [] for k in ("chain", "push_slot", "push_copy", "detect", "chain+detect")}
    frame = 0
    for rep in range(reps + 1):
        for k in range(8):                             # blocks 8w + k of window w
            eng.fill_noise(x, B, frame)
            frame += B
            slot = bank.slot_tensor().view(B, n)
            if k == 0 and rep > 0:
                # the block whose push runs window rep - 1: chain into the slot, then the detection
                t_all = timed(torch, lambda: (eng.process(x, out=slot), bank.push(slot, B)))
                rec["chain+detect"].append(t_all)
                continue
            if k == 1:
                rec["chain"].append(timed(torch, lambda: eng.process(x, out=slot)))
                rec["push_slot"].append(timed(torch, lambda: bank.push(slot, B)))
                continue
            eng.process(x, out=slot)
            bank.push(slot, B)
    # copying pushes and bare detections on a bank of their own
    side = pkg.PitchBank(n)
    for rep in range(reps):
        for k in range(8):
            if k == 7:
                rec["push_copy"].append(timed(torch, lambda: side.push(blk, B)))
            else:
                side.push(blk, B)
        s = side.slot_tensor()
        rec["detect"].append(timed(torch, lambda: side.push(s, B)))
        # the frames just pushed through the slot belong to the next window
        for k in range(7):
            side.push(blk, B)
        side.reset()
    torch.cuda.synchronize()
    out = {k: float(np.median(v)) for k, v in rec.items() if v}
    out["channels"] = n
    out["windows"] = bank.windows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="65536,131072,262144,524288,1048576")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    rows = []
    for n in (int(s) for s in a.channels.split(",")):
        r = measure(torch, n, a.reps)
        print(json.dumps(r), flush=True)
        rows.append(r)
        torch.cuda.empty_cache()
    print(f"\nbudget {BUDGET_MS:.3f} ms per 128-frame block")
    print(f"{'channels':>9} {'chain':>8} {'push_slot':>9} {'push_copy':>9} {'detect':>8} {'chain+detect':>12}  fits")
    best = None
    for r in rows:
        fits = r["chain+detect"] <= BUDGET_MS
        if fits:
            best = r["channels"]
        print(f"{r['channels']:>9} {r['chain']:>8.3f} {r['push_slot']:>9.3f} {r['push_copy']:>9.3f} {r['detect']:>8.3f} "
              f"{r['chain+detect']:>12.3f}  {'yes' if fits else 'no'}")
    print(f"largest channel count measured whose chain + detection fits the budget: {best}")


if __name__ == "__main__":
    main()
