"""Convolver bank rate (dspfx_convolve_*) beside a flat device copy of the bytes its accumulation reads.  Setup: B = 128,
frame-major, a decaying noise response of --taps taps, two alternating input blocks of noise.  At each --channels the bank runs
past P blocks first, so that every ring slot is live; then device events around every run, --reps runs after 5 warm-ups, the
median.  The bytes of one block are the ring read, P * 1024 * channels (the forward and inverse transforms move 2 KiB per
channel more, which is not counted); `copy` is torch's copy_ of that many bytes (it reads AND writes them).  The fraction of
peak is ring bytes / time / 8 TB/s.  One JSON line per case, then a table.
With --responses R > 1 the bank holds R responses of --taps taps each and the channels carry them by --pattern: `ranges` (R equal
contiguous ranges: a hall's buses adjacent) or `interleaved` (c % R: every wave mixed).  The bank of one response is timed first
on the same ring, then the ids are assigned and the bank timed again: ms per block, the fraction of 8 TB/s, and the ratio of the
two.

  python tools/convolve_rate.py [--channels 1024,4096] [--taps 4096,48000,144000] [--reps 20] [--responses 4 --pattern ranges]
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

B = 128
PEAK = 8.0e12


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


def measure(torch, n, taps, reps, responses=1, pattern="ranges"):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    h = rng.standard_normal(taps) * np.exp(-6.9 * np.arange(taps) / taps)
    bank = pkg.Convolver(n, h)
    xs = [torch.empty(B * n, dtype=torch.float32, device=dev).uniform_(-1.0, 1.0) for _ in range(2)]
    y = torch.empty_like(xs[0])
    for i in range(bank.partitions):
        bank.run(xs[i % 2], B, out=y)
    ms = timed(torch, lambda i: bank.run(xs[i % 2], B, out=y), reps)
    nbytes = bank.partitions * 1024 * n
    src = torch.empty(nbytes // 4, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    copy = timed(torch, lambda i: dst.copy_(src), reps)
    r = {"channels": n, "taps": taps, "partitions": bank.partitions, "ms": ms, "block_budget_ms": B / 48.0,
         "ring_bytes": nbytes, "fraction_of_peak": nbytes / (ms * 1e-3) / PEAK, "copy_ms": copy, "run_over_copy": ms / copy}
    if responses > 1:
        del src, dst
        for i in range(1, responses):
            bank.add_response(rng.standard_normal(taps) * np.exp(-6.9 * np.arange(taps) / taps))
        c = np.arange(n)
        bank.assign(c % responses if pattern == "interleaved" else c * responses // n)
        multi = timed(torch, lambda i: bank.run(xs[i % 2], B, out=y), reps)
        r.update({"responses": responses, "pattern": pattern, "single_ms": ms, "ms": multi,
                  "fraction_of_peak": nbytes / (multi * 1e-3) / PEAK, "multi_over_single": multi / ms, "run_over_copy": multi / copy})
    print(json.dumps(r), flush=True)
    bank.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="1024,4096")
    ap.add_argument("--taps", default="4096,48000,144000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--responses", type=int, default=1, help="responses the bank holds (up to %d)" % pkg.CONVOLVE_MAX_RESPONSES)
    ap.add_argument("--pattern", choices=("ranges", "interleaved"), default="ranges", help="how the channels carry them")
    a = ap.parse_args()
    import torch
    rows = []
    for n in (int(s) for s in a.channels.split(",")):
        for t in (int(s) for s in a.taps.split(",")):
            rows.append(measure(torch, n, t, a.reps, a.responses, a.pattern))
            torch.cuda.empty_cache()
    print(f"\ntimes in ms, median of {a.reps}; a block lasts {B / 48.0:.3f} ms; fractions of the 8 TB/s HBM peak")
    print(f"{'channels':>9} {'taps':>7} {'P':>5} {'run':>8} {'of peak':>8} {'copy':>8} {'run/copy':>9}")
    for r in rows:
        print(f"{r['channels']:>9} {r['taps']:>7} {r['partitions']:>5} {r['ms']:>8.4f} {r['fraction_of_peak']:>8.3f} "
              f"{r['copy_ms']:>8.4f} {r['run_over_copy']:>9.2f}"
              + (f"   {r['responses']} responses, {r['pattern']}: {r['multi_over_single']:.2f} x the single-response bank "
                 f"({r['single_ms']:.4f} ms)" if "responses" in r else ""))


if __name__ == "__main__":
    main()
