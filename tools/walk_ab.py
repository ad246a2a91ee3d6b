#!/usr/bin/env python3
"""In-process interleaved A/B of the tile walk and the stream policy (profiles/llc_reuse.txt): one engine per arm, placement
tuned, two alternating inputs and one output buffer per arm as bench.py has them, >= 200 launches per arm.
Each arm = "name[:key=val,...]" with keys
  lib=<path to a libdspfx build>   walk=0|1 (DSPFX_WALK)   zone=<MiB> (DSPFX_WALK_ZONE_MIB)
  head=0|1 (DSPFX_WALK_HEAD: the head zone's stores on the default policy | with the hint)   tail=<MiB> (DSPFX_WALK_TAIL_MIB)
Example (parent/libdspfx.so: the parent commit's build of the library):
  python tools/walk_ab.py parent:lib=parent/libdspfx.so fwd:walk=0 alt:walk=1 alt64:walk=1,zone=64
  python tools/walk_ab.py --chain chain3 --channels 131072 --tune 0 parent:lib=parent/libdspfx.so branch
Engines of different arms land on different physical pages, which alone moves config 5 by several percent in unlucky cases
(profiles/r01_placement.txt): judge an arm against the SAME arm of another process, or keep to two arms per process."""
import argparse
import importlib.util
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ENV = {"walk": "DSPFX_WALK", "zone": "DSPFX_WALK_ZONE_MIB", "head": "DSPFX_WALK_HEAD", "tail": "DSPFX_WALK_TAIL_MIB"}


def load_pkg(lib_path, tag):
    if lib_path:
        os.environ["DSPFX_LIB"] = lib_path if os.path.isabs(lib_path) else os.path.join(ROOT, lib_path)
    else:
        os.environ.pop("DSPFX_LIB", None)
    name = f"dsp_stuff_amd_{tag}"
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "dsp-stuff_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    mod.lib()
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("arms", nargs="+")
    ap.add_argument("--channels", type=int, default=1 << 20)
    ap.add_argument("--delay", type=int, default=24000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--chain", default="chain5", choices=["chain3", "chain5"])
    ap.add_argument("--tune", type=int, default=1)
    args = ap.parse_args()
    import torch
    import chains
    dev = torch.device("cuda", 0)
    N, B = args.channels, 128
    xs = [torch.empty(B * N, dtype=torch.float32, device=dev) for _ in range(2)]
    arms = []
    for i, spec in enumerate(args.arms):
        name, _, rest = spec.partition(":")
        kv = dict(x.split("=", 1) for x in rest.split(",") if x)
        pkg = load_pkg(kv.get("lib"), str(i))
        for k, env in ENV.items():
            if k in kv:
                os.environ[env] = kv[k]
            else:
                os.environ.pop(env, None)
        eng = pkg.Engine(N, B, link_flags=3, tile_channels=256)
        eng.set_chain(getattr(chains, args.chain)(pkg, args.delay))
        y = torch.empty(B * N, dtype=torch.float32, device=dev)
        if i == 0:
            eng.fill_noise(xs[0], B, 0)
            eng.fill_noise(xs[1], B, B)
        if args.tune:
            eng.tune_placement(xs[0], y, B)
        desc = eng.describe().strip().splitlines()
        print(f"# {name}: {[l for l in desc if l.startswith('stage')][-1]} | {[l for l in desc if 'walk' in l]}", flush=True)
        arms.append(dict(name=name, eng=eng, mix=torch.zeros(B, dtype=torch.float32, device=dev), y=y, ms=[], k=0))
    stream = torch.cuda.current_stream().cuda_stream

    def run(a, n):
        for _ in range(n):
            a["eng"].process(xs[a["k"] & 1], out=a["y"], mix=a["mix"], n_frames=B, stream=stream)
            a["k"] += 1

    for a in arms:
        a["eng"].profile_enable(args.steps + 4)
        a["eng"].profile_enable(0)
        run(a, max(8, args.delay // B + 2))
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for a in (arms if r % 2 == 0 else arms[::-1]):
            run(a, 4)                       # back in the cache state of this arm's own steady state
            a["eng"].profile_enable(1)
            run(a, args.steps)
            torch.cuda.synchronize()
            a["eng"].profile_enable(0)
            ms, n, kern = a["eng"].profile_read()
            a["ms"].append(ms / max(n, 1))
            a["kern"] = kern
    base = statistics.median(arms[0]["ms"])
    for a in arms:
        med = statistics.median(a["ms"])
        print(f"{a['name']:>12s} {a['kern']:>12s} N={N} median {med * 1000:8.2f} us  min {min(a['ms']) * 1000:8.2f}  "
              f"max {max(a['ms']) * 1000:8.2f}  vs first {base / med:.4f}x  ({args.rounds} x {args.steps} launches)")


if __name__ == "__main__":
    main()
