"""Channel-generator bank rate (dspfx_gens_*) beside the uniform engine on the same buffers.  Setup: B = 128, tiled W = 256, two
alternating output blocks; two noise blocks serve as add_to and as the control blocks.  At each --channels:
  sine       every channel SignalGen(0.5, 441, Sine); beside it Engine([SignalGen(0.5, 441, Sine)], link_flags=0)
  triangle   ... Triangle; beside it that engine
  square     ... Square; beside it that engine
  constant   ... Constant; beside it that engine
  clustered  span s of 256 channels carries mode s % 4: every wave of the four-channel kernel holds one mode
  mixed      channel c carries mode c % 4: a lane's four channels hold the four modes, every wave runs the four bodies
  half       the sine bank with every second span of 256 channels dropped: half the waves do no arithmetic
  none       a fresh bank: zeros through the bank's kernel
  add_to     the mixed bank added into a block, out of place: one block-unit read, one written
  ports      the mixed bank with both control blocks: two block-units read, one written
  write      a flat device write (torch fill_) of one block-unit
  copy       a flat torch copy: one block-unit in, one out
The bank's own bytes per run are the block-units it reads and writes (plus 13 bytes of tables per channel, not counted): one for a
plain run, two with add_to, three with both ports.  Device events around every call, --reps runs after 5 warm-ups, the median; the
fraction of peak is those bytes / time / 8 TB/s.  One JSON line per channel count, then a table.

  python tools/gens_rate.py [--channels 65536,262144,1048576] [--reps 20]
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
UNITS = {"add_to": 2, "ports": 3, "copy": 2}          # block-units a case moves; every other case writes one


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


def measure(torch, n, reps):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(95)
    xs = [torch.rand(B * n, dtype=torch.float32, device=dev, generator=gen) * 2 - 1 for _ in range(2)]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    bank = pkg.ChannelGenerators(n, tile_channels=W if n % W == 0 else 0, max_frames=B)
    run = lambda **kw: timed(torch, lambda i: bank.run(B, ys[i % 2], **{k: v[i % 2] for k, v in kw.items()}), reps)     # noqa: E731
    r = {"channels": n, "unit_bytes": B * n * 4}
    r["none_ms"] = run()
    for name, mode in (("sine", pkg.SIG_SINE), ("triangle", pkg.SIG_TRIANGLE), ("square", pkg.SIG_SQUARE), ("constant", pkg.SIG_CONSTANT)):
        bank.set(0.5, 441.0, mode)
        r[name + "_ms"] = run()
        eng = pkg.Engine(n, B, link_flags=0, tile_channels=bank.tile_channels)
        eng.set_chain([pkg.SignalGen(0.5, 441.0, mode)])
        r[name + "_engine_ms"] = timed(torch, lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=B), reps)
        eng.close()
    span = np.arange(n) // 256
    bank.set(mode=(span % 4).astype(np.uint32))
    r["clustered_ms"] = run()
    bank.set(mode=pkg.SIG_SINE)
    for s in range(1, (n + 255) // 256, 2):
        bank.drop(s * 256, min(256, n - s * 256))
    r["half_ms"] = run()
    bank.set(0.5, 441.0, (np.arange(n) % 4).astype(np.uint32))
    r["mixed_ms"] = run()
    r["add_to_ms"] = run(add_to=xs)
    r["ports_ms"] = run(amplitude=xs, frequency=xs[::-1])
    bank.close()
    r["write_ms"] = timed(torch, lambda i: ys[i % 2].fill_(0.25), reps)
    r["copy_ms"] = timed(torch, lambda i: ys[i % 2].copy_(xs[i % 2]), reps)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="65536,262144,1048576")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    rows = []
    for n in (int(s) for s in a.channels.split(",")):
        rows.append(measure(torch, n, a.reps))
        torch.cuda.empty_cache()
    cases = ["none", "sine", "triangle", "square", "constant", "clustered", "mixed", "half", "add_to", "ports", "write", "copy"]
    print(f"\ntimes in ms, median of {a.reps}; (fraction of the 8 TB/s HBM peak on the run's own block-units); [x the uniform engine]")
    for r in rows:
        print(f"{r['channels']} channels")
        for c in cases:
            t = r[c + "_ms"]
            eng = f"  [engine {r[c + '_engine_ms']:.4f} ms, bank x {t / r[c + '_engine_ms']:.2f}]" if c + "_engine_ms" in r else ""
            print(f"  {c:>10} {t:>8.4f} ({UNITS.get(c, 1) * r['unit_bytes'] / (t * 1e-3) / PEAK:.3f}){eng}")


if __name__ == "__main__":
    main()
