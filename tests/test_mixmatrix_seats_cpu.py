"""The seated mix-matrix bank without a GPU: the seating rule as the library applies it to host arrays (dspfx_mixmatrix_reseat, which
dspfx_mixmatrix_assign uses) against its restatement (mixseats_ref), its invariants, its refusals, and the plan of a seated bank."""
import numpy as np
import pytest

import mixseats_ref as S

TABLE = [0, 1, 3, 34, 66, 99, 259, 320]                  # rooms of 1, 2, 31, 32, 33, 160 and 61
SEATS = [32, 32, 32, 64, 64, 192, 64]
NONE = S.NONE
WHY = {"range": "not inside", "id": "is given room", "capacity": "capacity"}     # the words of the library's reason for each refusal


def random_call(rng, room_of, seats):
    """a range of channels and an id for each: mostly a room with room left, sometimes NONE, sometimes the room they are in"""
    n, g = len(room_of), len(seats)
    count = int(rng.integers(1, 9)) if rng.random() < 0.8 else int(rng.integers(1, 80))
    first = int(rng.integers(0, n - count + 1))
    ids = []
    for i in range(count):
        u = rng.random()
        if u < 0.2:
            ids.append(NONE)
        elif u < 0.35:
            ids.append(int(room_of[first + i]))
        else:
            ids.append(int(rng.integers(0, g)))
    return ids, first


def test_reseat_follows_the_rule_over_random_call_sequences(dspfx):
    """300 sequences of 12 calls from the fresh seating: after every call the library's arrays are the restatement's, and -- stated
    without the restatement -- no seat is held twice, every entering channel holds the lowest seat that was free after the call's
    leaves (in ascending channel order), and the channels the call did not move are where they were.  A call the restatement
    refuses is refused by the library for the same reason, and changes nothing."""
    rng = np.random.default_rng(71)
    seats = S.round32(SEATS)
    refused = 0
    for _ in range(300):
        room_of, seat_of = S.initial(TABLE, SEATS)
        for _ in range(12):
            ids, first = random_call(rng, room_of, seats)
            r32, q32 = room_of.astype(np.uint32), seat_of.astype(np.uint32)
            try:
                want_r, want_q, moves = S.reseat(room_of, seat_of, SEATS, ids, first)
            except S.Refused as e:
                refused += 1
                with pytest.raises(dspfx.DspfxError) as err:
                    dspfx.mixmatrix_reseat(r32, q32, SEATS, ids, first)
                assert err.value.status == -1 and WHY[e.what] in str(err.value), (e, err.value)
                continue
            got_r, got_q = dspfx.mixmatrix_reseat(r32, q32, SEATS, ids, first)
            assert (r32 == room_of).all() and (q32 == seat_of).all()            # (the inputs are copied, not changed)
            assert (got_r == want_r.astype(np.uint32)).all() and (got_q == want_q.astype(np.uint32)).all()
            # the invariants, from the arrays alone
            moved = {m[0] for m in moves}
            stay = np.ones(len(room_of), bool)
            stay[sorted(moved)] = False
            sits = got_r != NONE
            held = got_r[sits].astype(np.int64) * 2048 + got_q[sits]
            assert (got_q[sits] < seats[got_r[sits]]).all() and len(np.unique(held)) == len(held) and (got_q[~sits] == NONE).all()
            assert (got_r[stay] == room_of[stay]).all() and (got_q[stay] == seat_of[stay]).all()
            free = {int(g): set(range(int(seats[g]))) - set(seat_of[stay & (room_of == g)].tolist()) for g in set(got_r[sorted(moved)].tolist()) - {NONE}}
            for c in sorted(moved):
                assert got_r[c] == (ids[c - first] & 0xFFFFFFFF)
                if got_r[c] != NONE:
                    assert got_q[c] == min(free[int(got_r[c])])
                    free[int(got_r[c])].remove(int(got_q[c]))
            room_of, seat_of = want_r, want_q
    assert refused > 20                                   # (the capacity refusal is really exercised: rooms of 32 seats fill up)


def test_two_channels_swap_between_two_full_rooms_in_one_call(dspfx):
    room_of, seat_of = S.initial([0, 32, 64], [32, 32])
    ids = [0] * 32 + [1] * 32
    ids[3], ids[40] = 1, 0
    r, q = dspfx.mixmatrix_reseat(room_of, seat_of, [32, 32], ids, 0)
    assert (r[3], q[3], r[40], q[40]) == (1, 8, 0, 3)     # each takes the seat the other left: the only free one
    with pytest.raises(dspfx.DspfxError) as e:           # ... and one more into a full room is over capacity
        dspfx.mixmatrix_reseat(room_of, seat_of, [32, 32], [1], 3)
    assert "capacity" in str(e.value) and "room 1" in str(e.value)


def test_who_returns_gets_the_lowest_free_seat(dspfx):
    room_of, seat_of = S.initial([0, 8], [32])
    r, q = dspfx.mixmatrix_reseat(room_of, seat_of, [32], [NONE, 0, 0, 0, NONE], 2)      # channels 2 and 6 leave
    assert (r[2], r[6], q[2]) == (NONE, NONE, NONE)
    r, q = dspfx.mixmatrix_reseat(r, q, [32], [0], 6)
    assert (r[6], q[6]) == (0, 2)                         # not seat 6


BAD = {
    "range_past_n": (dict(ids=[0, 0], first=319), "not inside"),
    "range_from_n": (dict(ids=[0], first=320), "not inside"),
    "no_ids": (dict(ids=[], first=0), "no ids"),
    "id_is_g": (dict(ids=[0, 7], first=5), "channel 6 is given room 7"),
    "capacity": (dict(ids=[0] * 32, first=3), "capacity"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_a_bad_call_changes_nothing_and_says_which(dspfx, case):
    kw, why = BAD[case]
    room_of, seat_of = S.initial(TABLE, SEATS)
    with pytest.raises(S.Refused):
        S.reseat(room_of, seat_of, SEATS, kw["ids"], kw["first"])
    r, q = room_of.astype(np.uint32), seat_of.astype(np.uint32)
    L = dspfx.lib()
    import ctypes as C
    u32 = C.POINTER(C.c_uint32)
    ids = np.asarray(kw["ids"], np.uint32)
    seats = np.asarray(SEATS, np.uint32)
    rc = L.dspfx_mixmatrix_reseat(r.ctypes.data_as(u32), q.ctypes.data_as(u32), seats.ctypes.data_as(u32), len(seats), len(r),
                                  ids.ctypes.data_as(u32), kw["first"], len(ids))
    assert rc == -1 and why in L.dspfx_mixmatrix_last_error(None).decode()
    assert (r == room_of).all() and (q == seat_of).all()  # in place, and still untouched


def test_reseat_refuses_a_seating_that_is_none(dspfx):
    with pytest.raises(dspfx.DspfxError):                # two channels in one seat
        dspfx.mixmatrix_reseat([0, 0], [1, 1], [32], [0], 0)
    with pytest.raises(dspfx.DspfxError):                # a seat the room does not have
        dspfx.mixmatrix_reseat([0, 0], [1, 32], [32], [0], 0)
    with pytest.raises(dspfx.DspfxError):                # a room of 1025 seats
        dspfx.mixmatrix_reseat([0], [0], [1025], [0], 0)


def test_plan_seats(dspfx):
    count, edge, offset, total = dspfx.mixmatrix_plan(320, group_start=TABLE, seats=SEATS)
    assert count.tolist() == [1, 2, 31, 32, 33, 160, 61] and edge.tolist() == SEATS
    sq = np.asarray(SEATS, np.int64) ** 2
    assert offset.tolist() == [0] + np.cumsum(sq)[:-1].tolist() and total == 4 * int(sq.sum())
    _, edge, _, total = dspfx.mixmatrix_plan(320, group_start=TABLE, seats=[1, 2, 31, 33, 33, 161, 61])       # rounded up to 32
    assert edge.tolist() == [32, 32, 32, 64, 64, 192, 64] and total == 4 * int(sq.sum())
    _, edge, _, total = dspfx.mixmatrix_plan(1 << 20, group_size=256, tile_channels=256, seats=256)
    assert (edge == 256).all() and total == 1 << 30
    _, edge, _, _ = dspfx.mixmatrix_plan(320, group_start=TABLE, seats=1024)
    assert (edge == 1024).all()
    for seats, why in (([32, 32, 30, 64, 64, 192, 64], "room 2 is given 30 seats"), ([32, 32, 32, 64, 64, 1025, 64], "room 5 is given 1025 seats"),
                       (0, "room 0 is given 0 seats")):
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.mixmatrix_plan(320, group_start=TABLE, seats=seats)
        assert e.value.status == -1 and why in str(e.value), e.value
    with pytest.raises(dspfx.DspfxError):                # what the table's own check refuses is still refused
        dspfx.mixmatrix_plan(8, group_start=[0, 4, 4, 8], seats=32)


def test_create_seats_checks_before_the_device(dspfx):
    """No GPU here: seats below the members or above the limit are DSPFX_ERR_INVALID with the reason, not "no device"."""
    for seats in ([32, 32, 30, 64, 64, 192, 64], 2048):
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.MixMatrix(320, group_start=TABLE, seats=seats)
        assert e.value.status == -1 and "seats" in str(e.value), e.value
