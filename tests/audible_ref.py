"""What the audible-list and sparse-run tests share, written from the rules in include/dspfx.h and not from the product code:
the audible rule in numpy, a CPU model of the sparse mix-matrix chain, and the 12-block script that drives a talker bank through
talker changes, an OPEN and a SHUT pin, a reset and an assign.

THE RULE.  A channel is audible in a gated run iff its gate or its target, as the run finds them, is not +-0.0: only then can
gate + (target - gate) * r[f] be non-zero.  Room r's audible members, in ascending channel order, are
list[start[r] : start[r] + count[r]], start being the members' prefix table."""
import numpy as np

import mixmatrix_ref as X
import talkers_ref as R

NO_ROOM = R.NO_ROOM
TABLE = [0, 1, 3, 34, 66, 99, 259, 320]                  # rooms of 1, 2, 31, 32, 33, 160 and 61 (tests/test_mixmatrix_seats_gpu.py)
SEATS = [32, 32, 32, 64, 64, 192, 64]
N, G = TABLE[-1], len(TABLE) - 1
NF, BLOCKS, TOP = 128, 12, 3
OPEN_AT, SHUT_AT = 120, 40                               # rooms 5 and 3
RESET_BLOCK, RESET = 5, (34, 65)                         # first channel, count: rooms 3 and 4
ASSIGN_BLOCK, ASSIGN_IDS, ASSIGN_FIRST = 8, [5, NO_ROOM, 3, 4], 64      # channels 64 .. 67 (rooms 3, 3, 4, 4): the last one stays


def audible(gate, target, room_of, groups):
    """-> (lists: per room the audible channels, ascending; start uint32[G + 1]; count uint32[G])"""
    gate, target, room_of = np.asarray(gate, np.float32), np.asarray(target, np.float32), np.asarray(room_of, np.uint32)
    aud = (gate != 0) | (target != 0)
    lists = [np.flatnonzero((room_of == g) & aud) for g in range(groups)]
    members = np.bincount(room_of[room_of != NO_ROOM].astype(np.int64), minlength=groups)
    start = np.concatenate([[0], np.cumsum(members)]).astype(np.uint32)
    return lists, start, np.asarray([len(l) for l in lists], np.uint32)


def check_tables(got, gate, target, room_of, groups):
    """(list, start, count) arrays against the rule, over each segment's first count[r] entries"""
    lst, start, count = (np.asarray(v) for v in got)
    lists, want_start, want_count = audible(gate, target, room_of, groups)
    assert lst.dtype == np.int32 and start.dtype == np.uint32 and count.dtype == np.uint32
    assert np.array_equal(start, want_start), (start, want_start)
    assert np.array_equal(count, want_count), (count, want_count)
    for g in range(groups):
        assert np.array_equal(lst[start[g]:start[g] + count[g]], lists[g]), g
    return lists


def script(seed=21):
    """-> (ref, blocks): a talkers_ref bank with the pins and the detector set, and per block (x [NF][N], what to do before
    the run: None, ("reset", first, count) or ("assign", ids, first)).  Every block gives every channel a loudness of its
    own, so the talkers change from block to block."""
    rng = np.random.default_rng(seed)
    ref = R.Talkers(N, TABLE, top=TOP)
    assert ref.set_detector(48.0, 2000.0)
    pins = np.zeros(N, np.uint8)
    pins[OPEN_AT], pins[SHUT_AT] = R.OPEN, R.SHUT
    assert ref.set_pin(pins)
    blocks = []
    for b in range(BLOCKS):
        x = (R.noise(rng, NF, N) * rng.uniform(0.05, 1.0, N).astype(np.float32)[None, :]).astype(np.float32)
        act = None
        if b == RESET_BLOCK:
            act = ("reset",) + RESET
        if b == ASSIGN_BLOCK:
            act = ("assign", ASSIGN_IDS, ASSIGN_FIRST)
        blocks.append((x, act))
    return ref, pins, blocks


def gathered_problem(x, room_of, groups):
    """the contiguous problem mixmatrix_ref takes: -> (xg [F][members], table, order: the channel of every gathered column).
    A room's members keep their channel order"""
    room_of = np.asarray(room_of, np.uint32)
    order = np.concatenate([np.flatnonzero(room_of == g) for g in range(groups)]).astype(np.int64)
    sizes = [int((room_of == g).sum()) for g in range(groups)]
    return np.ascontiguousarray(np.asarray(x, np.float32)[:, order]), [0] + [int(v) for v in np.cumsum(sizes)], order


def eval_sparse_f32(x, table, mats, listed, normalise=True):
    """mixmatrix_ref.eval_f32's ascending chain over the LISTED sources only: listed[r] = room-local indices, any order, duplicates
    allowed (they count once).  The divisors are those of the whole rows.  -> [F][N] f32"""
    x = np.asarray(x, np.float32)
    out = np.zeros_like(x)
    d, wired = X.divisors(mats, normalise)
    for (c0, n), m, ls in zip(X.rooms(table), mats, listed):
        m = np.asarray(m, np.float32)
        acc = np.zeros((x.shape[0], n), np.float32)
        for s in sorted(set(int(v) for v in ls)):
            assert 0 <= s < n
            acc = (acc + (x[:, None, c0 + s] * m[None, :, s]).astype(np.float32)).astype(np.float32)
        out[:, c0:c0 + n] = acc
    out = (out / d.astype(np.float32)[None, :]).astype(np.float32) if normalise else out
    out[:, ~wired] = np.float32(0.0)
    return out


def signed_mats(table, seed):
    """random_mats minus 3: finite entries of both signs in [-3, 7), about a third of them exactly -3"""
    return [(m - np.float32(3.0)).astype(np.float32) for m in X.random_mats(table, seed)]
