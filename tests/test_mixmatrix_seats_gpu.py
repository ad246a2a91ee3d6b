"""The seated mix-matrix bank on the GPU (dspfx_mixmatrix_create_seats, _assign, _set_pairs): a room of seats computes, bit for
bit, what the unseated bank computes on the equivalent contiguous problem (mixseats_ref.gathered); a scripted walk through the
seating rule with the tables checked exactly on integers, by bits against the unseated bank and inside the derived bound with the
recounted divisors; channels in no room; stream order; refusals; stores by seat; moves from a second thread; and the standing
real-time condition at 2^20 channels."""
import threading

import numpy as np
import pytest

import mixmatrix_ref as X
import mixseats_ref as S

pytestmark = pytest.mark.gpu

TABLE = [0, 1, 3, 34, 66, 99, 259, 320]                  # rooms of 1, 2, 31, 32, 33, 160 and 61
SEATS = [32, 32, 32, 64, 64, 192, 64]                    # one chunk; two chunks; 192: wider than a workgroup's 128 listeners
N = TABLE[-1]
NONE = S.NONE
SENTINEL = 0x7FC0BEEF                                    # a NaN no arithmetic produces
SLACK = 4096
LAYOUTS = [0, 64]                                        # frame-major; tiled 64 (320 = 5 tiles)
FRAMES = [37, 128, 161]                                  # 161: a second frame pass


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def device_block(dspfx, torch, x, tile):
    return torch.from_numpy(dspfx.to_layout(np.ascontiguousarray(x, np.float32), tile).reshape(-1).copy()).cuda()


def fresh_out(torch, size):
    return torch.full((size + SLACK,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def read_out(dspfx, out, nf, n, tile):
    h = out.cpu().numpy()
    assert (h[nf * n:].view(np.uint32) == SENTINEL).all(), "something was written past the block"
    return dspfx.from_layout(h[:nf * n], nf, n, tile)


def run(dspfx, torch, mm, x, tile=0):
    nf, n = x.shape
    out = fresh_out(torch, nf * n)
    mm.run(device_block(dspfx, torch, x, tile), nf, out=out)
    torch.cuda.synchronize()
    return read_out(dspfx, out, nf, n, tile)


def noise(nf, n, seed):
    return (np.random.default_rng(seed).uniform(-1.0, 1.0, (nf, n)) + 0.25).astype(np.float32)


def integers(nf, n, seed):
    return np.random.default_rng(seed).integers(-512, 513, (nf, n)).astype(np.float32)


def seated(dspfx, tile=0, nf=128, normalise=True, seats=SEATS, table=TABLE):
    return dspfx.MixMatrix(int(table[-1]), group_start=table, tile_channels=tile, max_frames=nf, normalise=normalise, seats=seats)


class Gathered:
    """An unseated, frame-major bank for the equivalent contiguous problem of a model: sum S_r channels in seat order."""

    def __init__(self, dspfx, torch, model, nf, normalise=True):
        self.dspfx, self.torch, self.model = dspfx, torch, model
        self.table = model.gtable()
        self.mm = dspfx.MixMatrix(self.table[-1], group_start=self.table, max_frames=nf, normalise=normalise)

    def run(self, x):
        """the model's matrices on x [F][N] -> [F][N] by channel (+0.0 for a channel in no room)"""
        for c0, m in zip(self.table, self.model.mats):
            self.mm.set_rows(m, c0)
        xg, _ = self.model.gathered(x)
        return self.model.scatter(run(self.dspfx, self.torch, self.mm, xg))

    def close(self):
        self.mm.close()


def gain(l, s):
    """the integer gain of the exactness checks, by CHANNEL number: in [-3, 3], not symmetric"""
    return float(((3 * int(l) + 5 * int(s)) % 7) - 3)


def int_lines(model, g, channels, cols=False):
    """[len(channels)][S_g] by seat: gain() towards the channel in every taken seat, and 9.0 at the empty ones (which the bank
    must store as +0.0)"""
    chan = model.chan(g)
    return np.asarray([[9.0 if o == NONE else (gain(o, c) if cols else gain(c, o)) for o in chan] for c in channels], np.float32)


# ---- 1. identity ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("tile", LAYOUTS)
def test_identity_seating_gives_the_unseated_bits(dspfx, torch_cuda, tile, nf):
    """seats = the members rounded up to 32: the seated bank has the tables of the unseated one, and its bits on the same block.
    With more seats than that it has the bits of the unseated bank on the gathered problem.  Random matrices, a third zeros."""
    x = noise(nf, N, 100 + nf)
    mats = X.random_mats(TABLE, 3)
    plain = dspfx.MixMatrix(N, group_start=TABLE, tile_channels=tile, max_frames=nf)
    for (c0, n), m in zip(X.rooms(TABLE), mats):
        plain.set_rows(m, c0)
    try:
        want = run(dspfx, torch_cuda, plain, x, tile)
    finally:
        plain.close()
    for seats in ([n for _, n in X.rooms(TABLE)], SEATS):
        model = S.Bank(TABLE, seats)
        mm = seated(dspfx, tile, nf, seats=seats)
        ref = Gathered(dspfx, torch_cuda, model, nf)
        try:
            assert (mm.seats == model.S).all() and (mm.seat_of() == model.seat_of).all() and (mm.occupancy() == model.occupancy()).all()
            for g, ((c0, n), m) in enumerate(zip(X.rooms(TABLE), mats)):
                rows = np.full((n, int(model.S[g])), 7.0, np.float32)            # (7.0 at the empty seats: stored as +0.0)
                rows[:, :n] = m
                mm.set_rows(rows, c0)
                model.set_lines(rows, c0)
            got = run(dspfx, torch_cuda, mm, x, tile)
            assert np.isfinite(got).all()
            assert (bits(got) == bits(want)).all(), np.argwhere(bits(got) != bits(want))[:5]
            assert (bits(got) == bits(ref.run(x))).all()
        finally:
            mm.close()
            ref.close()


# ---- 2. a scripted walk ---------------------------------------------------------------------------------------------------------

WALK = [                                                 # (what, ids, first_channel, {channel: (room, seat)} afterwards)
    ("two leave for no room", [NONE, 3, 3, 3, NONE], 36, {36: (NONE, NONE), 40: (NONE, NONE), 37: (3, 3)}),
    ("into a fuller room, past seat 32", [4], 5, {5: (4, 33)}),
    ("past seat 128 of the 192-seat room (and room 0 is empty)", [5], 0, {0: (5, 160)}),
    ("two rooms filled to their 32 seats", [1] * 30 + [2] * 2, 100, {100: (1, 2), 129: (1, 31), 130: (2, 2), 131: (2, 31)}),
    ("a swap between the two full rooms in one call", [2, 1, 2, 2, 4, 2, 2, 2, 2, 1], 1, {1: (2, 7), 10: (1, 0), 2: (1, 1), 5: (4, 33)}),
    ("back to the old room: the lowest free seat, not the old one", [3], 40, {40: (3, 2)}),
]


def check_walk_state(dspfx, torch, tile, nf, step, raw, model_raw, mm, model, ref):
    # the seating itself
    for bank, mod in ((raw, model_raw), (mm, model)):
        assert (bank.room_of() == mod.room_of.astype(np.uint32)).all() and (bank.seat_of() == mod.seat_of.astype(np.uint32)).all(), step
        assert (bank.occupancy() == mod.occupancy()).all(), step
    # (a) integers, raw sums: the int64 product of the host model, bit for bit (every order is exact below 2^24: asserted inside)
    k = integers(nf, N, 7 * step + nf)
    kg, gt = model_raw.gathered(k)
    want = model_raw.scatter(X.scaled_int_product(kg, gt, model_raw.mats, 0))
    got = run(dspfx, torch, raw, k, tile)
    assert (bits(got) == bits(want)).all(), (step, np.argwhere(bits(got) != bits(want))[:5])
    # (b) noise, the default wiring: the bits of an unseated bank on the gathered problem
    x = noise(nf, N, 11 * step + nf)
    got = run(dspfx, torch, mm, x, tile)
    want = ref.run(x)
    assert (bits(got) == bits(want)).all(), (step, np.argwhere(bits(got) != bits(want))[:5])
    # (c) normalised: inside the derived bound of the float64 value, n = the taken seats: the divisors were recounted
    xg, gt = model.gathered(x)
    exact, sabs, _ = X.exact(xg, gt, model.mats, True)
    err = np.abs(model.gathered(got)[0].astype(np.float64) - exact)
    bnd = X.bound(sabs, model.occupied_of())
    assert (err <= bnd).all(), (step, float((err / bnd).max()))
    assert (bits(got[:, model.room_of == NONE]) == 0).all()


@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("tile", LAYOUTS)
def test_a_scripted_walk(dspfx, torch_cuda, tile, nf):
    """`raw`: normalise=False, integer gains by channel number, newcomers seated with MIXMATRIX_ZERO and wired by set_pairs (the
    last one by set_rows and set_cols, by seat).  `mm`: the default bank, newcomers seated with MIXMATRIX_MIX_MINUS."""
    torch = torch_cuda
    model_raw, model = S.Bank(TABLE, SEATS), S.Bank(TABLE, SEATS)
    raw, mm = seated(dspfx, tile, nf, normalise=False), seated(dspfx, tile, nf)
    ref = Gathered(dspfx, torch, model, nf)
    try:
        for g, (c0, n) in enumerate(X.rooms(TABLE)):
            rows = int_lines(model_raw, g, range(c0, c0 + n))
            raw.set_rows(rows, c0)
            model_raw.set_lines(rows, c0)
        check_walk_state(dspfx, torch, tile, nf, 0, raw, model_raw, mm, model, ref)
        for step, (what, ids, first, after) in enumerate(WALK, 1):
            mm.assign(ids, first)
            model.assign(ids, first, S.MIX_MINUS)
            raw.assign(ids, first, dspfx.MIXMATRIX_ZERO)
            moves = model_raw.assign(ids, first, S.ZERO)
            for c, (g, q) in after.items():
                assert (model.room_of[c], model.seat_of[c]) == (g, q), (what, c)     # (the script does what its name says)
            entered = [(c, g) for c, _, _, g, _ in moves if g != NONE]
            if step == len(WALK):                        # by seat: one row and one column of S_r values
                (c, g), = entered
                for cols, store in ((False, raw.set_rows), (True, raw.set_cols)):
                    line = int_lines(model_raw, g, [c], cols)
                    store(line, c)
                    model_raw.set_lines(line, c, cols)
            elif entered:                                # by channel number
                ls, ss, gs = [], [], []
                for c, g in entered:
                    for o in model_raw.chan(g):
                        if o != NONE:
                            ls += [c, int(o)]
                            ss += [int(o), c]
                            gs += [gain(c, o), gain(o, c)]
                raw.set_pairs(ls, ss, gs)
                model_raw.set_pairs(ls, ss, gs)
            check_walk_state(dspfx, torch, tile, nf, step, raw, model_raw, mm, model, ref)
        # everybody's gains are gain() of the two channel numbers still: nothing between two who stayed was ever touched
        for g in range(len(SEATS)):
            chan = model_raw.chan(g)
            for l, cl in enumerate(chan):
                for s, cs in enumerate(chan):
                    assert model_raw.mats[g][l, s] == (gain(cl, cs) if cl != NONE and cs != NONE else 0.0)
    finally:
        raw.close()
        mm.close()
        ref.close()


# ---- 3. no room ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", LAYOUTS)
def test_no_room_reads_zero_and_a_nan_follows_the_mover(dspfx, torch_cuda, tile):
    nf = 37
    x = noise(nf, N, 31)
    mm = seated(dspfx, tile, nf)
    try:
        mm.assign(NONE, 36)
        xp = x.copy()
        xp[:, 36] = np.nan
        xp[5, 36] = np.inf
        got = run(dspfx, torch_cuda, mm, xp, tile)
        assert np.isfinite(got).all(), "a channel in no room reached somebody"
        assert (bits(got[:, 36]) == 0).all()              # +0.0 by bits, in every frame
        mm.assign(2, 70)                                  # from room 4 to room 2, carrying NaN
        xp = x.copy()
        xp[:, 70] = np.nan
        got = run(dspfx, torch_cuda, mm, xp, tile)
        room = mm.room_of()
        assert room[70] == 2 and mm.seat_of()[70] == 31
        assert np.isnan(got[:, room == 2]).all(), "the NaN reaches every listener of the new room"
        assert np.isfinite(got[:, room != 2]).all(), "... and nobody of the old one, or of any other"
        assert (bits(got[:, 36]) == 0).all()
    finally:
        mm.close()


# ---- 4. stream order -------------------------------------------------------------------------------------------------------------

def test_an_assign_between_two_runs_changes_the_second_only(dspfx, torch_cuda):
    torch = torch_cuda
    nf = 128
    x = noise(nf, N, 41)
    dx = device_block(dspfx, torch, x, 0)
    model = S.Bank(TABLE, SEATS)
    mm = seated(dspfx, 0, nf)
    ref = Gathered(dspfx, torch, model, nf)
    try:
        old = ref.run(x)
        ids, first = [5, NONE, 3, 4], 64                  # channels 64 .. 67 (rooms 3, 4, 4, 4): one stays in room 4
        model.assign(ids, first)
        new = ref.run(x)
        assert (bits(old) != bits(new)).any()
        o1, o2 = fresh_out(torch, x.size), fresh_out(torch, x.size)
        mm.run(dx, nf, out=o1)                            # (no synchronisation between the three calls)
        mm.assign(ids, first)
        mm.run(dx, nf, out=o2)
        torch.cuda.synchronize()
        assert (bits(read_out(dspfx, o1, nf, N, 0)) == bits(old)).all()
        assert (bits(read_out(dspfx, o2, nf, N, 0)) == bits(new)).all()
    finally:
        mm.close()
        ref.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------

def test_a_refused_call_changes_nothing(dspfx, torch_cuda):
    nf = 37
    x = noise(nf, N, 51)
    mm = seated(dspfx, 0, nf)
    plain = dspfx.MixMatrix(N, group_start=TABLE, max_frames=nf)
    try:
        mm.assign(4, 5)                                   # (not the fresh seating)
        before, rooms, seats = run(dspfx, torch_cuda, mm, x), mm.room_of(), mm.seat_of()
        for ids, first, why in (([0] * 32, 3, "capacity"), ([7], 5, "is given room 7"), ([0, 0], 319, "not inside"), ([0], 320, "not inside")):
            with pytest.raises(dspfx.DspfxError) as e:
                mm.assign(ids, first)
            assert e.value.status == -1 and why in str(e.value), e.value
        with pytest.raises(dspfx.DspfxError) as e:
            mm.assign(0, 5, 7)                            # no such preset
        assert e.value.status == -1
        for l, s in (([3, 5], [4, 4]), ([3], [320]), ([36], [NONE])):      # channel 5 sits in room 4 now, 3 and 4 in room 2
            with pytest.raises(dspfx.DspfxError) as e:
                mm.set_pairs(l, s, 2.0)
            assert e.value.status == -1 and "one room" in str(e.value), e.value
        assert (mm.room_of() == rooms).all() and (mm.seat_of() == seats).all()
        assert (bits(run(dspfx, torch_cuda, mm, x)) == bits(before)).all()
        with pytest.raises(dspfx.DspfxError) as e:
            plain.assign(0, 5)
        assert e.value.status == -6                       # DSPFX_ERR_STATE: a bank without seats
        assert (plain.room_of()[[0, 5, 319]] == [0, 2, 6]).all() and (plain.seat_of()[[0, 5, 319]] == [0, 2, 60]).all()
        assert plain.occupancy().tolist() == [1, 2, 31, 32, 33, 160, 61]
    finally:
        mm.close()
        plain.close()


def test_set_pairs_on_an_unseated_bank(dspfx, torch_cuda):
    """Gains by channel number on the bank without seats: the same store as set_rows, a later duplicate wins, the divisors follow."""
    nf = 37
    k = integers(nf, N, 55)
    mats = [X.asymmetric(n) for _, n in X.rooms(TABLE)]
    mm = dspfx.MixMatrix(N, group_start=TABLE, max_frames=nf, normalise=True)
    try:
        for (c0, n), m in zip(X.rooms(TABLE), mats):
            mm.set_rows(m, c0)
        mm.set_pairs([40, 100, 100, 258, 2], [35, 258, 258, 99, 1], [2.0, 1.0, -3.0, 0.0, 0.0])
        mats[3][6, 1], mats[5][1, 159], mats[5][159, 0], mats[1][1, 0] = 2.0, -3.0, 0.0, 0.0
        got = run(dspfx, torch_cuda, mm, k)
    finally:
        mm.close()
    d, wired = X.divisors(mats, True)
    want = (X.scaled_int_product(k, TABLE, mats, 0) / d.astype(np.float32)[None, :]).astype(np.float32)
    want[:, ~wired] = 0.0
    assert (bits(got) == bits(want)).all()


# ---- 6. stores by seat -----------------------------------------------------------------------------------------------------------

def test_stores_on_a_seated_bank_are_by_seat(dspfx, torch_cuda):
    nf = 37
    k = integers(nf, N, 61)
    model = S.Bank(TABLE, SEATS)
    mm = seated(dspfx, 0, nf, normalise=False)
    try:
        for ids, first in (([NONE, 3, 3, 3, NONE], 36), ([3], 5), ([3], 70)):      # room 3: seats 2 and 6 go to channels 5 and 70
            mm.assign(ids, first)
            model.assign(ids, first)
        assert model.seat_of[5] == 2 and model.seat_of[70] == 6 and model.seat_of[65] == 31
        rng = np.random.default_rng(62)
        for first, count, cols in ((5, 1, False), (70, 1, True), (37, 3, False), (64, 2, True)):
            lines = rng.integers(-3, 4, (count, 64)).astype(np.float32)
            lines[:, 32:] = 5.0                           # seats 32 .. 63 of room 3 are empty: these change nothing
            (mm.set_cols if cols else mm.set_rows)(lines, first)
            model.set_lines(lines, first, cols)
        mm.fill(4, dspfx.MIXMATRIX_MIX_MINUS)             # room 4 lost channel 70: 1.0 between the 32 taken seats only
        model.fill(4, S.MIX_MINUS)
        assert model.mats[4].sum() == 32 * 31 and (model.mats[3][:, 32:] == 0).all() and (model.mats[3][32:, :] == 0).all()
        kg, gt = model.gathered(k)
        want = model.scatter(X.scaled_int_product(kg, gt, model.mats, 0))
        got = run(dspfx, torch_cuda, mm, k)
        assert (bits(got) == bits(want)).all(), np.argwhere(bits(got) != bits(want))[:5]
        bad = [(np.ones((1, 32), np.float32), 34, "64 seats"),           # a line is S_r long, not n_r
               (np.ones((2, 64), np.float32), 35, "one room"),           # 35 sits in room 3, 36 in none
               (np.ones((2, 64), np.float32), 4, "one room"),            # 4 in room 2, 5 in room 3
               (np.ones((1, 64), np.float32), 36, "one room"),           # in no room
               (np.ones((1, 64), np.float32), 320, "not inside")]
        for lines, first, why in bad:
            for store in (mm.set_rows, mm.set_cols):
                with pytest.raises(dspfx.DspfxError) as e:
                    store(lines, first)
                assert e.value.status == -1 and why in str(e.value), e.value
        assert (bits(run(dspfx, torch_cuda, mm, k)) == bits(want)).all()
    finally:
        mm.close()


# ---- 7. a second thread ----------------------------------------------------------------------------------------------------------

def test_moves_from_another_thread_are_seen_whole(dspfx, torch_cuda):
    """Room 3 is full at 32 seats.  While 50 blocks are submitted, another thread moves channel 40 out of it and back in: its seat
    is the only free one each time, and MIX_MINUS wires it as it was.  Every block's output for the room is that of one of the two
    seatings, wholly."""
    torch = torch_cuda
    nf = 128
    seats = [32, 32, 32, 32, 64, 192, 64]
    x = noise(nf, N, 71)
    dx = device_block(dspfx, torch, x, 0)
    mm = seated(dspfx, 0, nf, seats=seats)
    room = slice(34, 66)
    try:
        inside = run(dspfx, torch_cuda, mm, x)
        mm.assign(NONE, 40)
        outside = run(dspfx, torch_cuda, mm, x)
        mm.assign(3, 40)
        assert mm.seat_of()[40] == 6 and (bits(run(dspfx, torch_cuda, mm, x)) == bits(inside)).all()
        assert (bits(inside[:, room]) != bits(outside[:, room])).any() and (bits(outside[:, 40]) == 0).all()
        outs = [fresh_out(torch, x.size) for _ in range(50)]
        stop = threading.Event()
        moves = [0]

        def mover():
            while not stop.is_set() and moves[0] < 400:   # (bounded: every move waits in the queue until the next run takes it)
                mm.assign(NONE, 40)
                mm.assign(3, 40)
                moves[0] += 2

        t = threading.Thread(target=mover)
        t.start()
        try:
            for o in outs:
                mm.run(dx, nf, out=o)
        finally:
            stop.set()
            t.join()
        torch.cuda.synchronize()
        last = run(dspfx, torch_cuda, mm, x)
        assert moves[0] > 0 and (bits(last) == bits(inside)).all()
        for o in outs:
            got = bits(read_out(dspfx, o, nf, N, 0))
            is_in = (got[:, room] == bits(inside[:, room])).all()
            assert is_in or (got[:, room] == bits(outside[:, room])).all(), "a run saw half a move"
            others = np.ones(N, bool)
            others[room] = False
            assert (got[:, others] == bits(inside[:, others])).all()
    finally:
        mm.close()


# ---- 8. the full size ------------------------------------------------------------------------------------------------------------

def test_full_size_identity_seating(dspfx, torch_cuda):
    """N = 2^20 in 4096 rooms of 256 with 256 seats each, 128 frames, tiled 256, identity seating: a run takes no longer than the
    2.667 ms a block lasts (the standing condition for every bank).  The ratio to the unseated bank on the same buffers is
    printed, not asserted."""
    torch = torch_cuda
    n, size, nf, tile = 1 << 20, 256, 128, 256
    free, _ = torch.cuda.mem_get_info()
    if free < 5 << 30:                                    # two tables of 1 GiB, two blocks of 512 MiB, and room to spare
        pytest.skip("device memory is short")
    torch.manual_seed(7)
    dx = torch.rand(nf * n, dtype=torch.float32, device="cuda") * 2.0 - 0.75
    out = torch.empty_like(dx)
    plain = dspfx.MixMatrix(n, group_size=size, tile_channels=tile, max_frames=nf)
    mm = dspfx.MixMatrix(n, group_size=size, tile_channels=tile, max_frames=nf, seats=size)
    rows = np.random.default_rng(8).uniform(0.0, 10.0, (3, size)).astype(np.float32)
    rows[1, 5] = 0.0
    try:
        for bank in (plain, mm):
            bank.set_rows(rows, 0)
            bank.set_rows(rows, n - size + 100)

        def timed(fn):
            for _ in range(5):
                fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
            for a, b in ev:
                a.record()
                fn()
                b.record()
            torch.cuda.synchronize()
            return float(np.median([a.elapsed_time(b) for a, b in ev]))

        ms_plain = timed(lambda: plain.run(dx, nf, out=out))
        want_first, want_last = out[:nf * size].clone(), out[-nf * size:].clone()
        ms = timed(lambda: mm.run(dx, nf, out=out))
        torch.cuda.synchronize()
        assert torch.equal(out[:nf * size].view(torch.int32), want_first.view(torch.int32))       # the first and the last room: the unseated bits
        assert torch.equal(out[-nf * size:].view(torch.int32), want_last.view(torch.int32))
    finally:
        plain.close()
        mm.close()
    print(f"mixmatrix seated, identity seating, full size: {ms:.4f} ms per run | unseated {ms_plain:.4f} ms | x {ms / ms_plain:.3f}")
    assert ms <= 128.0 / 48000.0 * 1e3, f"{ms:.4f} ms per run, and a block lasts 2.667 ms"
