"""The seating of the mix-group bank without a GPU: dspfx_mixgroups_room_plan (a pure host function) -- validation, member
counts, depth and pieces for the seatings the GPU tests use, independence of a room's figures from the other rooms -- and the
documented bound against the literal reference order on the tests' own data."""
import ctypes as C

import numpy as np
import pytest

import mixrooms_ref as M

INVALID = -1
NO = M.NO_ROOM


def _ceil_log2(n):
    return (int(n) - 1).bit_length()


def test_the_entry_points_exist(dspfx):
    L = dspfx.lib()
    for name in ("dspfx_mixgroups_assign", "dspfx_mixgroups_rooms", "dspfx_mixgroups_room_plan"):
        assert name in dspfx.EXPORTS and hasattr(L, name), name
    assert dspfx.NO_ROOM == NO
    for m in ("assign", "room_of", "counts", "depth"):
        assert hasattr(dspfx.MixGroups, m), m
    assert L.dspfx_mixgroups_assign(None, None, 0, 0) == INVALID
    assert L.dspfx_mixgroups_rooms(None, None, 0, 0) == INVALID


@pytest.mark.parametrize("room,groups,tile,word", [
    ([0, 1, 5, 2], 5, 0, "room 5"),                       # an id >= G
    ([0, 1, 2, 3] * 250, 4, 48, "power of two"),          # a tile that is no power of two
    ([0, 1, 2, 3] * 250, 4, 64, "divides"),               # a power of two that does not divide N = 1000
])
def test_room_plan_rejects_with_a_reason(dspfx, room, groups, tile, word):
    with pytest.raises(dspfx.DspfxError) as e:
        dspfx.mixgroups_room_plan(np.asarray(room, np.uint32), groups, tile)
    assert e.value.status == INVALID and word in str(e.value), str(e.value)


def test_room_plan_null_and_no_rooms(dspfx):
    L = dspfx.lib()
    ids = (C.c_uint32 * 4)(0, 0, 0, 0)
    assert L.dspfx_mixgroups_room_plan(None, 4, 1, 0, None, None, None) == INVALID
    assert L.dspfx_mixgroups_room_plan(ids, 4, 0, 0, None, None, None) == INVALID
    assert L.dspfx_mixgroups_last_error(None)
    assert L.dspfx_mixgroups_room_plan(ids, 4, 1, 0, None, None, None) == 0      # every output may be NULL


def _seatings(n, G):
    span_member = np.full(n, NO, np.uint32)
    span_member[np.arange(0, n, 256) + 17] = 0                                  # room 0: one member per span
    return {
        "contiguous": (np.arange(n) * G // n).astype(np.uint32),
        "modulo": (np.arange(n) % G).astype(np.uint32),
        "one_room": np.zeros(n, np.uint32),
        "unseated": np.full(n, NO, np.uint32),
        "one_per_span": span_member,
    }


@pytest.mark.parametrize("name", ["contiguous", "modulo", "one_room", "unseated", "one_per_span"])
@pytest.mark.parametrize("n,tile", [(1024, 256), (1000, 0), (32768, 256)])
def test_room_plan_figures(dspfx, n, tile, name):
    G = 5
    room = _seatings(n, G)[name]
    count, depth, pieces = dspfx.mixgroups_room_plan(room, G, tile)
    assert np.array_equal(count, M.counts(room, G))
    nspans = (n + 255) // 256
    for g, m in enumerate(M.members(room, G)):
        assert depth[g] <= M.cap(len(m)), (g, depth[g], len(m))
        per_span = np.bincount(m // 256, minlength=nspans)
        assert pieces[g] == (per_span > 0).sum(), g                             # one piece per span the room has members in
        if len(m) == 0:
            assert depth[g] == 0 and pieces[g] == 0
    if name == "one_per_span":
        # pieces of one member need no addition; the reduce adds them 64 at a time: 15 + 2 a round of 64, then the rounds' results
        want = 0 if nspans == 1 else (nspans + 3) // 4 - 1 + 2 if nspans <= 64 else 17 + ((nspans // 64 + 3) // 4 - 1) + (2 if nspans // 64 >= 3 else 1)
        assert depth[0] == want, (depth[0], want)
    if name == "one_room" and n % 256 == 0:
        assert pieces[0] == nspans and depth[0] >= 8                            # whole spans: the lane tree is 8 deep
    if name == "modulo":
        assert pieces.sum() == G * nspans


def test_rooms_of_one(dspfx):
    n = 1024
    count, depth, pieces = dspfx.mixgroups_room_plan(np.arange(n, dtype=np.uint32), n, 256)
    assert (count == 1).all() and (depth == 0).all() and (pieces == 1).all()


def test_a_rooms_plan_does_not_depend_on_the_other_rooms(dspfx):
    n, G = 4096, 7
    rng = np.random.default_rng(5)
    mine = np.sort(rng.choice(n, 300, replace=False))
    figures = []
    for trial in range(4):
        room = rng.integers(1, G, n).astype(np.uint32) if trial < 3 else np.full(n, NO, np.uint32)
        if trial == 2:
            room[rng.choice(n, 1000, replace=False)] = NO
        g = [0, 3, 6, 0][trial]                                                 # ... nor on its own number
        room[room == g] = (g + 1) % G
        room[mine] = g
        count, depth, pieces = dspfx.mixgroups_room_plan(room, G, 256)
        assert count[g] == 300
        figures.append((int(depth[g]), int(pieces[g])))
    assert len(set(figures)) == 1, figures
    assert figures[0][1] == len(set((mine // 256).tolist()))


def _sequential_sum(t):
    s = t[:, 0].copy()
    for c in range(1, t.shape[1]):
        s = (s + t[:, c]).astype(np.float32)
    return s


@pytest.mark.parametrize("with_gain", [False, True], ids=["nogain", "gain"])
@pytest.mark.parametrize("name", ["contiguous", "modulo", "one_per_span"])
def test_literal_reference_order_stays_inside_the_bound(name, with_gain):
    """The reference adds a room's pipes one after the other in f32 (collect_and_average): n - 1 dependent additions.  On the
    GPU tests' own data that order is inside the documented bound with D = n - 1, for the bus and for a return."""
    n, G, nf = 1000, 5, 7
    rng = np.random.default_rng(77)
    room = _seatings(n, G)[name]
    x = (rng.uniform(-1.0, 1.0, (nf, n)) * 10.0 ** rng.uniform(-3.0, 0.0, n)[None, :]).astype(np.float32)
    gain = rng.uniform(0.0, 4.0, n).astype(np.float32) if with_gain else None
    t = M.terms(x, gain)
    ref, sabs = M.buses(x, room, G, gain)
    rref, rsabs = M.returns_exact(x, room, G, gain)
    for g, m in enumerate(M.members(room, G)):
        if len(m) == 0:
            continue
        lit = (_sequential_sum(t[:, m]) / M.link_divisor(len(m))).astype(np.float32).astype(np.float64)
        assert (np.abs(lit - ref[:, g]) <= M.bound(sabs[:, g], ref[:, g], len(m) - 1)).all(), g
        if len(m) >= 2:
            c = m[len(m) // 2]                                                  # this member's Output node: the other pipes, in order
            others = t[:, m[m != c]]
            lit = (_sequential_sum(others) / M.link_divisor(len(m) - 1)).astype(np.float32).astype(np.float64)
            assert (np.abs(lit - rref[:, c]) <= M.bound(rsabs[:, c], rref[:, c], len(m) - 1)).all(), (g, c)


def test_restatement_bookkeeping():
    x = np.arange(1, 13, dtype=np.float32).reshape(2, 6)
    room = np.asarray([2, 0, NO, 2, 0, 2], np.uint32)      # room 2 = {0, 3, 5}, room 0 = {1, 4}, room 1 empty, channel 2 unseated
    ref, sabs = M.buses(x, room, 3, normalise=False)
    assert np.array_equal(ref, [[7, 0, 11], [19, 0, 29]]) and np.array_equal(sabs, ref)
    rref, rsabs = M.returns_exact(x, room, 3, normalise=False)
    assert np.array_equal(rref, [[10, 5, 0, 7, 2, 5], [22, 11, 0, 19, 8, 17]])
    assert np.array_equal(rsabs, [[11, 7, 0, 11, 7, 11], [29, 19, 0, 29, 19, 29]])
