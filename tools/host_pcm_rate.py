"""Host-path rate in device sample formats (dspfx_process_host_pcm) against the f32 host path (dspfx_process_host), from
page-locked buffers, on the chain5 engine of tools/host_rate.py: a host clock around the synchronous calls, 2 warm-up blocks
then --blocks timed ones, ms per block for
  f32                  dspfx_process_host
  i16                  I16 mono in / I16 mono out
  i16->f32             I16 mono in / F32 out
  i16x2->i16           I16 stereo in (folded to mono as a + b) / I16 mono out
at each --channels, and p50 / p99 over --tail-blocks blocks at --tail-channels for f32 and i16.  One JSON line per
measurement, then a summary table.  Budget: 2.667 ms per 128-frame block at 48 kHz.

  python tools/host_pcm_rate.py [--channels 131072,262144,1048576] [--blocks 20] [--tail-channels 262144] [--tail-blocks 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
from dsp_stuff_amd import workloads  # noqa: E402

B = 128
FORMS = ("f32", "i16", "i16->f32", "i16x2->i16")


def buffers(form, n):
    """(in, out, kwargs of the call) over page-locked memory"""
    if form == "f32":
        return pkg.PinnedArray((B, n)), pkg.PinnedArray((B, n)), {}
    if form == "i16":
        return pkg.PinnedArray((B, n), np.int16), pkg.PinnedArray((B, n), np.int16), {}
    if form == "i16->f32":
        return pkg.PinnedArray((B, n), np.int16), pkg.PinnedArray((B, n)), {}
    return pkg.PinnedArray((B, 2 * n), np.int16), pkg.PinnedArray((B, n), np.int16), {"in_channels": 2}


def fill(a, rng):
    if a.dtype == np.float32:
        a[:] = rng.uniform(-1, 1, a.shape).astype(np.float32)
    else:
        a[:] = rng.integers(-32768, 32767, a.shape, endpoint=True, dtype=np.int16)


def timed(eng, form, x, y, kw, blocks):
    call = (lambda: eng.process_host(x, out=y)) if form == "f32" else (lambda: eng.process_host_pcm(x, out=y, **kw))
    for _ in range(2):
        call()
    t = np.empty(blocks)
    for i in range(blocks):
        t0 = time.perf_counter()
        call()
        t[i] = time.perf_counter() - t0
    return t * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="131072,262144,1048576")
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--tail-channels", type=int, default=262144)
    ap.add_argument("--tail-blocks", type=int, default=200)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    rows = []
    for n in [int(v) for v in a.channels.split(",") if v]:
        eng = pkg.Engine(n, B)
        eng.set_chain(workloads.chain5(pkg, 24000))
        eng.kernels_ready()
        for form in FORMS:
            px, py, kw = buffers(form, n)
            fill(px.array, rng)
            t = timed(eng, form, px.array, py.array, kw, a.blocks)
            r = {"channels": n, "form": form, "blocks": a.blocks, "ms_mean": round(float(t.mean()), 3),
                 "ms_min": round(float(t.min()), 3), "bytes_in": px.array.nbytes, "bytes_out": py.array.nbytes}
            print(json.dumps(r), flush=True)
            rows.append(r)
            px.close()
            py.close()
        eng.close()
    if a.tail_blocks:
        n = a.tail_channels
        eng = pkg.Engine(n, B)
        eng.set_chain(workloads.chain5(pkg, 24000))
        eng.kernels_ready()
        for form in ("f32", "i16"):
            px, py, kw = buffers(form, n)
            fill(px.array, rng)
            t = timed(eng, form, px.array, py.array, kw, a.tail_blocks)
            r = {"channels": n, "form": form, "blocks": a.tail_blocks, "p50_ms": round(float(np.percentile(t, 50)), 3),
                 "p99_ms": round(float(np.percentile(t, 99)), 3), "max_ms": round(float(t.max()), 3)}
            print(json.dumps(r), flush=True)
            px.close()
            py.close()
        eng.close()
    print("\nms per block (mean of %d), pinned buffers, chain5:" % a.blocks)
    chans = sorted({r["channels"] for r in rows})
    print("%-12s" % "form" + "".join("%12d" % c for c in chans))
    for form in FORMS:
        print("%-12s" % form + "".join("%12.2f" % next(r["ms_mean"] for r in rows if r["channels"] == c and r["form"] == form)
                                       for c in chans))


if __name__ == "__main__":
    main()
