"""Mix-matrix bank rate (dspfx_mixmatrix_*) beside MixGroups.returns on the same buffers.  Setup: B = 128, tiled W = 256, one input
block of uniform noise, one output block, uniform rooms of --room members, fresh (mix-minus) matrices plus a few stored rows.  At each
--channels and each --room:
  matrix   MixMatrix.run
  returns  MixGroups.returns with the same table (what a fresh matrix computes, in O(n) per room instead of O(n^2))
  copy     a flat torch copy of the block's bytes
flop = 2 * channels * room * frames; the bank's own bytes = the block in, the block out and every matrix once (edges padded to 32).
Device events around every call, --reps runs after 5 warm-ups, the median.  The fractions are of the 157.3 TFLOP/s f32 peak and of the
8 TB/s HBM peak.  One JSON line per case, then a table.

  python tools/mixmatrix_rate.py [--channels 65536,262144,1048576] [--room 32,256,1024] [--reps 20]

--seats S measures the seated bank beside the unseated one, at identity seating and after each share of --moved of the channels has
been reseated at random; --staged adds, beside every one of those columns, the same bank on the same buffers in
MIXMATRIX_STAGED, and the seating's lines per chunk (MixMatrix.scatter), the figure a host decides the mode by:

  python tools/mixmatrix_rate.py --channels 1048576 --room 256 --seats 256 --moved 0,0.01,0.1,1 --staged

--sparse K adds the sparse run (MixMatrix.run(sources=...), dspfx_mixmatrix_run_sparse) with K listed sources per room, drawn at
random, beside every dense figure: a column of the plain table, and with --seats a table of its own (direct, and staged with --staged):

  python tools/mixmatrix_rate.py --channels 1048576 --room 256 --sparse 6
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
PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12


def timed(torch, fn, reps):
    for _ in range(5):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]))


def listed_sources(torch, mix, k, rng):
    """(list, start, count) on the device for MixMatrix.run(sources=...): k members of every room (all of a smaller one), drawn at
    random by the bank's seating so far, each segment ascending"""
    room_of = mix.room_of()
    order = np.argsort(room_of, kind="stable")           # members by (room, channel); the channels in no room come last
    sizes = np.bincount(room_of[room_of != pkg.NO_ROOM].astype(np.int64), minlength=mix.groups)
    first = np.concatenate([[0], np.cumsum(sizes)])
    segs = [np.sort(rng.choice(order[first[g]:first[g + 1]], min(k, int(sizes[g])), replace=False)) for g in range(mix.groups)]
    count = np.asarray([len(s) for s in segs], np.uint32)
    start = np.concatenate([[0], np.cumsum(count)]).astype(np.uint32)
    lst = np.concatenate(segs + [np.full(1, -1, np.int64)]).astype(np.int32)
    return tuple(torch.from_numpy(v).cuda() for v in (lst, start, count))


def measure(torch, n, room, reps, sparse=0):
    dev = torch.device("cuda:0")
    torch.manual_seed(91)
    x = torch.rand(B * n, dtype=torch.float32, device=dev) * 2.0 - 1.0
    y = torch.empty_like(x)
    _, _, _, table_bytes = pkg.mixmatrix_plan(n, group_size=room, tile_channels=W)
    mix = pkg.MixMatrix(n, group_size=room, tile_channels=W, max_frames=B)
    rooms = pkg.MixGroups(n, group_size=room, tile_channels=W, max_frames=B)
    rows = np.random.default_rng(92).uniform(0.0, 10.0, (min(3, room), room)).astype(np.float32)
    mix.set_rows(rows, 0)
    mix.set_rows(rows, n - room)
    ms = timed(torch, lambda: mix.run(x, B, out=y), reps)
    ret = timed(torch, lambda: rooms.returns(x, B, out=y), reps)
    copy = timed(torch, lambda: y.copy_(x), reps)
    flop, own = 2.0 * n * room * B, 2 * B * n * 4 + table_bytes
    r = {"channels": n, "room": room, "ms": ms, "tflops": flop / (ms * 1e-3) / 1e12, "fraction_of_flop_peak": flop / (ms * 1e-3) / PEAK_FLOPS,
         "bytes": own, "gbs": own / (ms * 1e-3) / 1e9, "fraction_of_hbm_peak": own / (ms * 1e-3) / PEAK_BYTES, "returns_ms": ret,
         "x_returns": ms / ret, "copy_ms": copy}
    if sparse:
        src = listed_sources(torch, mix, sparse, np.random.default_rng(94))
        r["sparse"], r["sparse_ms"] = sparse, timed(torch, lambda: mix.run(x, B, out=y, sources=src), reps)
        r["sparse_x_dense"] = r["sparse_ms"] / ms
    mix.close()
    rooms.close()
    print(json.dumps(r), flush=True)
    return r


def measure_seated(torch, n, room, seats, moved, reps, movers=16, staged=False, sparse=0):
    """The seated bank beside the unseated one on the same buffers: ms per run unseated, seated at identity seating, and seated
    after each share of `moved` of the channels (cumulatively, in the order given) has been reseated into a random room with room;
    and the ms of the first run after an assign of `movers` channels (the queued seats, lines and recounts ride ahead of it).
    staged: beside every seated figure the same run in MIXMATRIX_STAGED (same process, same bank, same buffers), and the lines per
    chunk of the seating."""
    dev = torch.device("cuda:0")
    torch.manual_seed(91)
    rng = np.random.default_rng(93)
    x = torch.rand(B * n, dtype=torch.float32, device=dev) * 2.0 - 1.0
    y = torch.empty_like(x)
    plain = pkg.MixMatrix(n, group_size=room, tile_channels=W, max_frames=B)
    r = {"channels": n, "room": room, "seats": seats, "unseated_ms": timed(torch, lambda: plain.run(x, B, out=y), reps)}
    plain.close()
    mix = pkg.MixMatrix(n, group_size=room, tile_channels=W, max_frames=B, seats=seats)
    S = int(mix.seats[0])
    r["identity_ms"] = timed(torch, lambda: mix.run(x, B, out=y), reps)
    r["identity_x_unseated"] = r["identity_ms"] / r["unseated_ms"]

    def staged_too(into, key):
        chunks, lines = mix.scatter()
        r.setdefault("lines_per_chunk", {})[key] = lines / max(chunks, 1)
        mix.set_staging(pkg.MIXMATRIX_STAGED)
        into[key] = timed(torch, lambda: mix.run(x, B, out=y), reps)
        mix.set_staging(pkg.MIXMATRIX_DIRECT)

    def sparse_too(key):
        """the sparse run over `sparse` listed sources per room at this seating, direct and (with staged) staged"""
        if not sparse:
            return
        src = listed_sources(torch, mix, sparse, rng)
        r.setdefault("sparse_ms", {})[key] = timed(torch, lambda: mix.run(x, B, out=y, sources=src), reps)
        if staged:
            mix.set_staging(pkg.MIXMATRIX_STAGED)
            r.setdefault("sparse_staged_ms", {})[key] = timed(torch, lambda: mix.run(x, B, out=y, sources=src), reps)
            mix.set_staging(pkg.MIXMATRIX_DIRECT)

    r["staged_ms"] = {}
    if staged:
        r["staging_bytes"] = pkg.mixmatrix_staging_bytes(n, seats, group_size=room, tile_channels=W, max_frames=B)
        staged_too(r["staged_ms"], "identity")
    sparse_too("identity")
    # the first run after a small assign, from (nearly) identity seating: `movers` channels swap rooms pairwise, then swap back
    firsts = []
    for _ in range(reps):
        room_of = mix.room_of()
        who = rng.choice(n, movers, replace=False)
        ids = room_of.copy()
        ids[who[0::2]], ids[who[1::2]] = room_of[who[1::2]], room_of[who[0::2]]
        mix.assign(ids)                                   # (one call over all channels; leaves come before enters: full rooms can swap)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        mix.run(x, B, out=y)
        ev[1].record()
        torch.cuda.synchronize()
        firsts.append(ev[0].elapsed_time(ev[1]))
        mix.assign(room_of)
        mix.run(x, B, out=y)
    r["first_run_after_assign_ms"], r["movers"] = float(np.median(firsts)), movers
    r["moved_ms"] = {}
    for share in moved:
        k = int(round(share * n))
        if k:
            # everybody chosen leaves, then each enters a random room that still has a seat (a full table when seats == room: they
            # are dealt back into the seats the leavers freed, in another order)
            who = np.sort(rng.choice(n, k, replace=False))
            ids = mix.room_of()
            ids[who] = pkg.NO_ROOM
            mix.assign(ids)                               # (one call over all channels: those whose id is their room stay)
            free = S - mix.occupancy().astype(np.int64)
            ids[who] = rng.permutation(np.repeat(np.arange(len(free)), free))[:k]
            mix.assign(ids)
        r["moved_ms"][str(share)] = timed(torch, lambda: mix.run(x, B, out=y), reps)
        if staged:
            staged_too(r["staged_ms"], str(share))
        sparse_too(str(share))
    mix.close()
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="65536,262144,1048576")
    ap.add_argument("--room", default="32,256,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seats", type=int, default=0, help="S: measure the seated bank with S seats per room beside the unseated one")
    ap.add_argument("--moved", default="0,0.01,0.1,1", help="with --seats: the shares of the channels reseated at random, cumulatively")
    ap.add_argument("--staged", action="store_true", help="with --seats: a MIXMATRIX_STAGED column beside every seated one, and the lines per chunk")
    ap.add_argument("--sparse", type=int, default=0, help="K: also MixMatrix.run(sources=...) with K listed sources per room, beside every dense figure")
    a = ap.parse_args()
    import torch
    if a.seats:
        moved = [float(s) for s in a.moved.split(",")]
        out = []
        for n in (int(s) for s in a.channels.split(",")):
            for room in (int(s) for s in a.room.split(",")):
                if room <= a.seats:
                    out.append(measure_seated(torch, n, room, a.seats, moved, a.reps, staged=a.staged, sparse=a.sparse))
                    torch.cuda.empty_cache()
        if a.sparse:
            print(f"\nthe sparse run, {a.sparse} listed sources per room, ms, median of {a.reps}; per seating: direct" + (" | staged" if a.staged else ""))
            print(f"{'channels':>9} {'room':>5} {'seats':>5} {'identity':>19} " + " ".join(f"{'moved ' + str(m):>19}" for m in moved))
            for r in out:
                keys = ["identity"] + [str(m) for m in moved]
                print(f"{r['channels']:>9} {r['room']:>5} {r['seats']:>5} "
                      + " ".join(f"{r['sparse_ms'][k]:>9.4f}" + (f" |{r['sparse_staged_ms'][k]:>8.4f}" if a.staged else " " * 10) for k in keys))
        if a.staged:
            print(f"\ntimes in ms, median of {a.reps}; per seating: direct | staged | lines per chunk (MixMatrix.scatter)")
            print(f"{'channels':>9} {'room':>5} {'seats':>5} {'unseated':>9} {'identity':>26} " + " ".join(f"{'moved ' + str(m):>26}" for m in moved)
                  + f" {'staging MiB':>12}")
            for r in out:
                cols = [(r["identity_ms"], r["staged_ms"]["identity"], r["lines_per_chunk"]["identity"])]
                cols += [(r["moved_ms"][str(m)], r["staged_ms"][str(m)], r["lines_per_chunk"][str(m)]) for m in moved]
                print(f"{r['channels']:>9} {r['room']:>5} {r['seats']:>5} {r['unseated_ms']:>9.4f} "
                      + " ".join(f"{d:>8.4f} |{s:>8.4f} |{l:>6.2f}" for d, s, l in cols) + f" {r['staging_bytes'] / 2**20:>12.0f}")
            return
        print(f"\ntimes in ms, median of {a.reps}; moved: the share of the channels reseated at random so far")
        print(f"{'channels':>9} {'room':>5} {'seats':>5} {'unseated':>9} {'identity':>9} {'x':>6} " + " ".join(f"{'moved ' + str(m):>11}" for m in moved)
              + f" {'first run after assign':>23}")
        for r in out:
            print(f"{r['channels']:>9} {r['room']:>5} {r['seats']:>5} {r['unseated_ms']:>9.4f} {r['identity_ms']:>9.4f} {r['identity_x_unseated']:>6.3f} "
                  + " ".join(f"{r['moved_ms'][str(m)]:>11.4f}" for m in moved) + f" {r['first_run_after_assign_ms']:>23.4f}")
        return
    rows = []
    for n in (int(s) for s in a.channels.split(",")):
        for room in (int(s) for s in a.room.split(",")):
            rows.append(measure(torch, n, room, a.reps, a.sparse))
            torch.cuda.empty_cache()
    print(f"\ntimes in ms, median of {a.reps}; TFLOP/s of 157.3; GB/s on the bank's own bytes of 8 TB/s")
    print(f"{'channels':>9} {'room':>5} {'matrix':>8} {'TFLOP/s':>8} {'of peak':>8} {'GB/s':>8} {'of peak':>8} {'returns':>8} {'x returns':>9} {'copy':>8}")
    for r in rows:
        print(f"{r['channels']:>9} {r['room']:>5} {r['ms']:>8.4f} {r['tflops']:>8.1f} {r['fraction_of_flop_peak']:>8.3f} {r['gbs']:>8.0f} "
              f"{r['fraction_of_hbm_peak']:>8.3f} {r['returns_ms']:>8.4f} {r['x_returns']:>9.2f} {r['copy_ms']:>8.4f}"
              + (f"   sparse, {r['sparse']} listed per room: {r['sparse_ms']:.4f} ms, x {r['sparse_x_dense']:.3f} of the dense run" if a.sparse else ""))


if __name__ == "__main__":
    main()
