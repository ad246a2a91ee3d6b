"""The staged mode of the seated mix-matrix bank without a GPU: dspfx_mixmatrix_scatter against a few lines of numpy over random
call sequences of the seating rule (mixseats_ref), its fixed points, its refusals, and dspfx_mixmatrix_staging_bytes against its
formula.  (set_staging's own refusals need a bank, and a bank needs a device: they are in test_mixmatrix_staged_gpu.py.)"""
import numpy as np
import pytest

import mixseats_ref as S

TABLE = [0, 1, 3, 34, 66, 99, 259, 320]                  # rooms of 1, 2, 31, 32, 33, 160 and 61
SEATS = [32, 32, 32, 64, 64, 192, 64]
NONE = S.NONE


def scatter_ref(room_of, seat_of, seats):
    """(chunks, lines): per room and run of 32 consecutive seats that holds anybody, 1 and the distinct channel // 32 among them"""
    chunks = lines = 0
    for g, s in enumerate(S.round32(seats)):
        c = np.nonzero(np.asarray(room_of) == g)[0]
        run_of = np.asarray(seat_of)[c] // 32
        for k in range(int(s) // 32):
            here = c[run_of == k]
            chunks += len(here) > 0
            lines += len(np.unique(here // 32))
    return int(chunks), int(lines)


def random_call(rng, room_of, groups):
    """a range of channels and an id for each: mostly some room, sometimes NONE, sometimes the room they are in"""
    count = int(rng.integers(1, 9)) if rng.random() < 0.8 else int(rng.integers(1, 80))
    first = int(rng.integers(0, len(room_of) - count + 1))
    u = rng.random(count)
    ids = np.where(u < 0.2, NONE, np.where(u < 0.35, room_of[first:first + count], rng.integers(0, groups, count)))
    return [int(v) for v in ids], first


def test_scatter_is_the_numpy_count_over_random_call_sequences(dspfx):
    rng = np.random.default_rng(81)
    calls = grown = 0
    for _ in range(60):
        room_of, seat_of = S.initial(TABLE, SEATS)
        before = scatter_ref(room_of, seat_of, SEATS)
        assert dspfx.mixmatrix_scatter(room_of.astype(np.uint32), seat_of.astype(np.uint32), SEATS) == before
        for _ in range(12):
            ids, first = random_call(rng, room_of, len(SEATS))
            try:
                room_of, seat_of, _ = S.reseat(room_of, seat_of, SEATS, ids, first)
            except S.Refused:
                continue
            want = scatter_ref(room_of, seat_of, SEATS)
            got = dspfx.mixmatrix_scatter(room_of.astype(np.uint32), seat_of.astype(np.uint32), SEATS)
            assert got == want, (got, want)
            assert got[0] <= got[1] <= 32 * got[0]
            calls += 1
        grown += want[1] > before[1]
    assert calls > 400 and grown > 30                     # (the sequences really scatter the seating)


def test_identity_seating_on_aligned_rooms_reads_one_line_per_chunk(dspfx):
    table = [0, 32, 96, 352, 384]                         # rooms of 32, 64, 256 and 32, every one from a multiple of 32
    for seats in ([32, 64, 256, 32], [64, 64, 512, 96], [1024] * 4):
        room_of, seat_of = S.initial(table, seats)
        chunks, lines = dspfx.mixmatrix_scatter(room_of.astype(np.uint32), seat_of.astype(np.uint32), seats)
        assert chunks == lines == 384 // 32               # the empty runs of 32 seats are not counted
    # ... and the seats test's table, whose rooms begin anywhere: a chunk can straddle two lines
    room_of, seat_of = S.initial(TABLE, SEATS)
    chunks, lines = dspfx.mixmatrix_scatter(room_of.astype(np.uint32), seat_of.astype(np.uint32), SEATS)
    assert (chunks, lines) == scatter_ref(room_of, seat_of, SEATS) and chunks == 1 + 1 + 1 + 1 + 2 + 5 + 2 and lines > chunks


def test_a_small_case_checked_by_hand(dspfx):
    """Two rooms of 64 seats over 200 channels.  Room 0: seats 0 .. 31 hold channels 0, 31 (line 0), 32 (line 1) and 199 (line 6):
    1 chunk, 3 lines; seat 40 holds channel 64: 1 chunk, 1 line.  Room 1: seats 32 and 63 hold channels 96 and 127, both of line 3:
    1 chunk, 1 line; its seats 0 .. 31 are empty: no chunk.  Everybody else is in no room."""
    room_of, seat_of = np.full(200, NONE, np.uint32), np.full(200, NONE, np.uint32)
    for c, g, q in ((0, 0, 0), (31, 0, 5), (32, 0, 31), (199, 0, 7), (64, 0, 40), (96, 1, 32), (127, 1, 63)):
        room_of[c], seat_of[c] = g, q
    assert dspfx.mixmatrix_scatter(room_of, seat_of, [64, 64]) == (3, 5)
    room_of[:], seat_of[:] = NONE, NONE
    assert dspfx.mixmatrix_scatter(room_of, seat_of, [64, 64]) == (0, 0)


def test_a_shuffled_seating_approaches_32_lines_per_chunk(dspfx):
    n, size = 1 << 16, 256
    rng = np.random.default_rng(82)
    perm = rng.permutation(n)
    room_of, seat_of = (perm // size).astype(np.uint32), (perm % size).astype(np.uint32)
    chunks, lines = dspfx.mixmatrix_scatter(room_of, seat_of, [size] * (n // size))
    assert chunks == n // 32 and (chunks, lines) == scatter_ref(room_of, seat_of, [size] * (n // size))
    assert 31.0 < lines / chunks <= 32.0                  # 32 draws from 2048 lines: 32 - C(32, 2) / 2048 = 31.76 expected


def test_scatter_refuses_what_reseat_refuses(dspfx):
    for room_of, seat_of, seats in (([0, 0], [1, 1], [32]), ([0, 0], [1, 32], [32]), ([0], [0], [1025]), ([1], [0], [32])):
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.mixmatrix_scatter(room_of, seat_of, seats)
        assert e.value.status == -1 and "mixmatrix scatter" in str(e.value), e.value
    with pytest.raises(dspfx.DspfxError):
        dspfx.mixmatrix_scatter([0, 0], [0], [32])


def test_staging_bytes_is_its_formula(dspfx):
    for table, seats, tile, nf in ((TABLE, SEATS, 0, 128), (TABLE, SEATS, 64, 161), (TABLE, [1, 2, 31, 33, 33, 160, 61], 0, 1),
                                   ([0, 5, 325], [32, 1024], 0, 37)):
        _, edge, _, _ = dspfx.mixmatrix_plan(table[-1], group_start=table, tile_channels=tile, seats=seats)
        assert (edge == S.round32(seats)).all()
        want = 2 * int(edge.astype(np.int64).sum()) * nf * 4 + 4 * table[-1]
        assert dspfx.mixmatrix_staging_bytes(table[-1], seats, group_start=table, tile_channels=tile, max_frames=nf) == want
    # the headline size: 4096 rooms of 256 seats, 128 frames: two copies of 512 MiB and 4 MiB of table
    assert dspfx.mixmatrix_staging_bytes(1 << 20, 256, group_size=256, tile_channels=256, max_frames=128) == (1 << 30) + (4 << 20)
    for kw in (dict(seats=[32] * 7), dict(seats=SEATS, max_frames=0), dict(seats=SEATS, tile_channels=48)):      # fewer seats than members; ...
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.mixmatrix_staging_bytes(TABLE[-1], kw.pop("seats"), group_start=TABLE, **kw)
        assert e.value.status == -1


def test_the_modes_are_named(dspfx):
    assert (dspfx.MIXMATRIX_DIRECT, dspfx.MIXMATRIX_STAGED) == (0, 1)
