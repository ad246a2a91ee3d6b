"""The staged mode of the seated mix-matrix bank on the GPU (dspfx_mixmatrix_set_staging): the block is transposed into a
seat-ordered copy, the direct run's chain runs over it, and the result is transposed back.  The staged run has the direct run's
bits at every seating of the seats tests' scripted walk and at a seating where everybody has moved; it equals the int64 product of
the host model on integers; the stale row of an emptied seat reaches nobody; out == block works in place; the mode is switched in
order with the stores and from a second thread; and at 2^20 channels, every one of them reseated at random, a staged run fits the
block and beats the direct run."""
import threading

import numpy as np
import pytest

import mixmatrix_ref as X
import mixseats_ref as S
from test_mixmatrix_seats_gpu import WALK               # the scripted walk itself: the six steps, not a copy of them

pytestmark = pytest.mark.gpu

TABLE = [0, 1, 3, 34, 66, 99, 259, 320]                  # rooms of 1, 2, 31, 32, 33, 160 and 61
SEATS = [32, 32, 32, 64, 64, 192, 64]
TABLE325, SEATS325 = TABLE + [325], SEATS + [32]         # one more room of 5: N is no multiple of 32 (nor of the transposes' 64)
CASES = [(TABLE, SEATS, 0), (TABLE, SEATS, 64), (TABLE325, SEATS325, 0)]      # frame-major; tiled 64; the odd N, frame-major only
CASE_IDS = ["n320-frame-major", "n320-tiled64", "n325-frame-major"]
FRAMES = [1, 37, 64, 128, 161]                           # 161: a second frame pass with an odd tail (and rows of the copies that start anywhere)
NONE = S.NONE
SENTINEL = 0x7FC0BEEF                                    # a NaN no arithmetic produces
SLACK = 4096


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


def run(dspfx, torch, mm, x, tile=0, mode=None):
    """one run in `mode` (None: the bank's) -> [F][N]; every sample of the block was written, and nothing past it"""
    if mode is not None:
        mm.set_staging(mode)
    nf, n = x.shape
    out = fresh_out(torch, nf * n)
    mm.run(device_block(dspfx, torch, x, tile), nf, out=out)
    torch.cuda.synchronize()
    got = read_out(dspfx, out, nf, n, tile)
    assert (bits(got) != SENTINEL).all(), "a sample of the block was not written"
    return got


def both(dspfx, torch, mm, x, tile=0):
    """-> (direct, staged) on the same bank and block"""
    return run(dspfx, torch, mm, x, tile, dspfx.MIXMATRIX_DIRECT), run(dspfx, torch, mm, x, tile, dspfx.MIXMATRIX_STAGED)


def noise(nf, n, seed):
    return (np.random.default_rng(seed).uniform(-1.0, 1.0, (nf, n)) + 0.25).astype(np.float32)


def integers(nf, n, seed):
    return np.random.default_rng(seed).integers(-512, 513, (nf, n)).astype(np.float32)


def seated(dspfx, table=TABLE, seats=SEATS, tile=0, nf=128, normalise=True):
    return dspfx.MixMatrix(int(table[-1]), group_start=table, tile_channels=tile, max_frames=nf, normalise=normalise, seats=seats)


def gain(l, s):
    """an integer gain by CHANNEL number: in [-3, 3], not symmetric"""
    return float(((3 * int(l) + 5 * int(s)) % 7) - 3)


def everybody_moves(model, seed):
    """-> [(ids, first)]: everybody leaves, then everybody enters a room drawn at random (as many per room as before).  Applied to
    the model here; the caller gives the same calls to the bank"""
    before = (model.room_of.copy(), model.seat_of.copy())
    ids = np.random.default_rng(seed).permutation(model.room_of)
    calls = [([NONE] * model.N, 0), ([int(g) for g in ids], 0)]
    for c in calls:
        model.assign(*c, S.ZERO)
    assert ((model.room_of != before[0]) | (model.seat_of != before[1])).mean() > 0.9      # (a few land where they sat)
    return calls


def wire_by_channel(bank, model):
    """gain() between every two channels of a room, into the bank (by channel number) and the model"""
    ls, ss, gs = [], [], []
    for g in range(model.G):
        chan = [int(c) for c in model.chan(g) if c != NONE]
        for l in chan:
            for s in chan:
                ls.append(l), ss.append(s), gs.append(gain(l, s))
    bank.set_pairs(ls, ss, gs)
    model.set_pairs(ls, ss, gs)


def int_product(model, k):
    kg, gt = model.gathered(k)
    return model.scatter(X.scaled_int_product(kg, gt, model.mats, 0))


# ---- 1. the bits of the direct mode --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalise", [True, False], ids=["normalised", "raw"])
@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_staged_run_has_the_direct_bits(dspfx, torch_cuda, case, nf, normalise):
    """One bank, one noise block: at the fresh seating, after every step of the scripted walk (two leave; a seat past 32; a seat
    past 128; two rooms filled; a swap in one call; a return to the lowest free seat) and once everybody has moved.  Random gains
    by seat, a third of them zeros; the newcomers are wired mix-minus."""
    table, seats, tile = case
    n = table[-1]
    x = noise(nf, n, 300 + nf)
    model = S.Bank(table, seats)
    mm = seated(dspfx, table, seats, tile, nf, normalise)
    rng = np.random.default_rng(301)
    try:
        for g, (c0, cnt) in enumerate(X.rooms(table)):
            rows = rng.uniform(0.0, 10.0, (cnt, int(model.S[g]))).astype(np.float32)
            rows[rng.uniform(0.0, 1.0, rows.shape) < 1.0 / 3.0] = 0.0
            mm.set_rows(rows, c0)
        steps = [("the fresh seating", None, None)] + [(what, ids, first) for what, ids, first, _ in WALK]
        steps += [("everybody has moved", ids, first) for ids, first in everybody_moves(model, 302)]
        seen = []
        for what, ids, first in steps:
            if ids is not None:
                mm.assign(ids, first)
            direct, staged = both(dspfx, torch_cuda, mm, x, tile)
            assert (bits(staged) == bits(direct)).all(), (what, np.argwhere(bits(staged) != bits(direct))[:5])
            assert (bits(staged[:, mm.room_of() == NONE]) == 0).all(), what
            seen.append(bits(staged).copy())
        assert all((a != b).any() for a, b in zip(seen[:-2], seen[1:-1])), "a step of the walk changed nothing"
        assert (mm.room_of() != NONE).all() and (seen[-1] != seen[0]).any()
    finally:
        mm.close()


# ---- 2. independent of the direct kernel ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_integers_give_the_int64_product_at_a_scattered_seating(dspfx, torch_cuda, case, nf):
    """Integer gains by channel number, integer samples, raw sums: every order of summation is exact below 2^24 (asserted by the
    product), so the staged run must give the host model's int64 product bit for bit -- whatever the direct kernel gives."""
    table, seats, tile = case
    k = integers(nf, table[-1], 400 + nf)
    model = S.Bank(table, seats)
    mm = seated(dspfx, table, seats, tile, nf, normalise=False)
    try:
        mm.set_staging(dspfx.MIXMATRIX_STAGED)
        for ids, first in everybody_moves(model, 401):
            mm.assign(ids, first, dspfx.MIXMATRIX_ZERO)
        assert (mm.room_of() == model.room_of).all() and (mm.seat_of() == model.seat_of).all()
        wire_by_channel(mm, model)
        want = int_product(model, k)
        assert (want != 0).mean() > 0.5
        got = run(dspfx, torch_cuda, mm, k, tile)
        assert mm.staging == dspfx.MIXMATRIX_STAGED
        assert (bits(got) == bits(want)).all(), np.argwhere(bits(got) != bits(want))[:5]
    finally:
        mm.close()


# ---- 3. stale rows of the copies reach nobody ----------------------------------------------------------------------------------

@pytest.mark.parametrize("nf", [37, 161])
@pytest.mark.parametrize("tile", [0, 64])
def test_the_stale_row_of_an_emptied_seat_reaches_nobody(dspfx, torch_cuda, tile, nf):
    x = noise(nf, TABLE[-1], 500 + nf)
    mm = seated(dspfx, tile=tile, nf=nf)
    staged = dspfx.MIXMATRIX_STAGED
    try:
        xp = x.copy()
        xp[:, 36] = np.nan                                # channel 36: seat 2 of room 3 (channels 34 .. 65)
        xp[nf // 2, 36] = np.inf
        got = run(dspfx, torch_cuda, mm, xp, tile, staged)
        assert (~np.isfinite(got[:, 34:66])).all() and np.isfinite(got[:, :34]).all() and np.isfinite(got[:, 66:]).all()
        mm.assign(NONE, 36)                               # the seat is empty now, and its row of the copy still holds the NaNs
        got = run(dspfx, torch_cuda, mm, xp, tile, staged)
        assert np.isfinite(got).all(), "the row an occupant left behind reached somebody"
        assert (bits(got[:, 36]) == 0).all()              # in no room: +0.0 by bits in every frame, whatever it carries
        assert (bits(got) == bits(run(dspfx, torch_cuda, mm, xp, tile, dspfx.MIXMATRIX_DIRECT))).all()
        mm.assign(2, 70)                                  # from room 4 to room 2, carrying NaN
        xp = x.copy()
        xp[:, 70] = np.nan
        got = run(dspfx, torch_cuda, mm, xp, tile, staged)
        room = mm.room_of()
        assert room[70] == 2 and mm.seat_of()[70] == 31
        assert np.isnan(got[:, room == 2]).all(), "the NaN reaches every listener of the new room"
        assert np.isfinite(got[:, room != 2]).all(), "... and nobody of the old one (where its row still holds it), or of any other"
        assert (bits(got[:, 36]) == 0).all()
    finally:
        mm.close()


# ---- 4. in place ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nf", [64, 161])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_a_staged_run_works_in_place_and_a_direct_one_does_not(dspfx, torch_cuda, case, nf):
    torch = torch_cuda
    table, seats, tile = case
    n = table[-1]
    x = noise(nf, n, 600 + nf)
    mm = seated(dspfx, table, seats, tile, nf)
    try:
        mm.assign([5, NONE, 3, 4], 64)
        want = run(dspfx, torch, mm, x, tile, dspfx.MIXMATRIX_STAGED)
        buf = fresh_out(torch, nf * n)
        dx = device_block(dspfx, torch, x, tile)
        buf[:nf * n] = dx
        block = buf[:nf * n]
        mm.run(block, nf, out=block)
        torch.cuda.synchronize()
        assert (bits(read_out(dspfx, buf, nf, n, tile)) == bits(want)).all()
        # a partial overlap, either way round, is refused in staged mode too, and nothing is launched
        buf[:nf * n] = dx
        for a, b in ((0, 16), (16, 0), (0, SLACK - 1)):
            with pytest.raises(dspfx.DspfxError) as e:
                mm.run(buf[a:a + nf * n], nf, out=buf[b:b + nf * n])
            assert e.value.status == -1 and "overlaps" in str(e.value), e.value
        # out == block in direct mode: refused as ever
        mm.set_staging(dspfx.MIXMATRIX_DIRECT)
        with pytest.raises(dspfx.DspfxError) as e:
            mm.run(block, nf, out=block)
        assert e.value.status == -1 and "overlaps" in str(e.value), e.value
        torch.cuda.synchronize()
        assert torch.equal(buf[:nf * n].view(torch.int32), dx.view(torch.int32)) and (buf[nf * n:].view(torch.int32) == SENTINEL).all()
    finally:
        mm.close()


# ---- 5. mode switches ----------------------------------------------------------------------------------------------------------

def test_set_staging_refusals(dspfx, torch_cuda):
    nf = 37
    x = noise(nf, TABLE[-1], 701)
    plain = dspfx.MixMatrix(TABLE[-1], group_start=TABLE, max_frames=nf)
    mm = seated(dspfx, nf=nf)
    try:
        for mode in (dspfx.MIXMATRIX_STAGED, dspfx.MIXMATRIX_DIRECT):
            with pytest.raises(dspfx.DspfxError) as e:
                plain.set_staging(mode)
            assert e.value.status == -6 and "no seats" in str(e.value)           # DSPFX_ERR_STATE
        assert plain.staging == dspfx.MIXMATRIX_DIRECT
        with pytest.raises(dspfx.DspfxError) as e:
            plain.scatter()
        assert e.value.status == -6
        assert mm.staging == dspfx.MIXMATRIX_DIRECT       # a fresh bank runs direct
        direct = run(dspfx, torch_cuda, mm, x)
        for now in (dspfx.MIXMATRIX_DIRECT, dspfx.MIXMATRIX_STAGED, dspfx.MIXMATRIX_DIRECT):
            mm.set_staging(now)
            for bad in (2, 7, 0xFFFFFFFF):
                with pytest.raises(dspfx.DspfxError) as e:
                    mm.set_staging(bad)
                assert e.value.status == -1 and "mode" in str(e.value)
                assert mm.staging == now
            assert (bits(run(dspfx, torch_cuda, mm, x)) == bits(direct)).all()
        # scatter() is mixmatrix_scatter of the bank's seating
        mm.assign([5, NONE, 3, 4], 64)
        assert mm.scatter() == dspfx.mixmatrix_scatter(mm.room_of(), mm.seat_of(), mm.seats)
    finally:
        plain.close()
        mm.close()


def test_an_assign_between_a_direct_and_a_staged_run_changes_the_second_only(dspfx, torch_cuda):
    torch = torch_cuda
    nf = 128
    k = integers(nf, TABLE[-1], 711)
    dk = device_block(dspfx, torch, k, 0)
    model = S.Bank(TABLE, SEATS)
    mm = seated(dspfx, nf=nf, normalise=False)
    try:
        old = int_product(model, k)                       # (mix-minus: gains of 0 and 1)
        ids, first = [5, NONE, 3, 4], 64                  # channels 64 .. 67 (rooms 3, 4, 4, 4): one stays in room 4
        model.assign(ids, first)
        new = int_product(model, k)
        assert (bits(old) != bits(new)).any()
        model.assign([4, 4, 4], 64)
        third = int_product(model, k)
        o1, o2, o3 = (fresh_out(torch, k.size) for _ in range(3))
        mm.run(dk, nf, out=o1)                            # (no synchronisation between the calls)
        mm.set_staging(dspfx.MIXMATRIX_STAGED)
        mm.assign(ids, first)
        mm.run(dk, nf, out=o2)
        mm.assign([4, 4, 4], 64)
        mm.set_staging(dspfx.MIXMATRIX_DIRECT)
        mm.run(dk, nf, out=o3)
        torch.cuda.synchronize()
        for o, want in ((o1, old), (o2, new), (o3, third)):
            assert (bits(read_out(dspfx, o, nf, TABLE[-1], 0)) == bits(want)).all()
    finally:
        mm.close()


def test_stores_made_while_staged_govern_the_next_run(dspfx, torch_cuda):
    """set_rows, set_cols, set_pairs and fill on a staged bank whose seating has changed: the next staged run is the host model's
    int64 product, and the direct run's bits."""
    nf = 37
    k = integers(nf, TABLE[-1], 721)
    model = S.Bank(TABLE, SEATS)
    mm = seated(dspfx, nf=nf, normalise=False)
    try:
        mm.set_staging(dspfx.MIXMATRIX_STAGED)
        for ids, first in (([NONE, 3, 3, 3, NONE], 36), ([3], 5), ([3], 70)):      # room 3: seats 2 and 6 go to channels 5 and 70
            mm.assign(ids, first)
            model.assign(ids, first)
        assert (bits(run(dspfx, torch_cuda, mm, k)) == bits(int_product(model, k))).all()
        rng = np.random.default_rng(722)
        for first, count, cols in ((5, 1, False), (70, 1, True), (37, 3, False), (64, 2, True)):
            lines = rng.integers(-3, 4, (count, 64)).astype(np.float32)
            lines[:, 32:] = 5.0                           # seats 32 .. 63 of room 3 are empty: these change nothing
            (mm.set_cols if cols else mm.set_rows)(lines, first)
            model.set_lines(lines, first, cols)
            assert (bits(run(dspfx, torch_cuda, mm, k)) == bits(int_product(model, k))).all(), (first, cols)
        pairs = ([100, 258, 5], [258, 99, 70], [-3.0, 2.0, 0.0])
        mm.set_pairs(*pairs)
        model.set_pairs(*pairs)
        assert (bits(run(dspfx, torch_cuda, mm, k)) == bits(int_product(model, k))).all()
        mm.fill(4, dspfx.MIXMATRIX_MIX_MINUS)             # room 4 lost channel 70
        model.fill(4, S.MIX_MINUS)
        mm.fill(1, dspfx.MIXMATRIX_ZERO)
        model.fill(1, S.ZERO)
        want = int_product(model, k)
        direct, staged = both(dspfx, torch_cuda, mm, k)
        assert (bits(staged) == bits(want)).all() and (bits(direct) == bits(want)).all()
        assert (bits(staged[:, 1:3]) == 0).all()
    finally:
        mm.close()


def test_toggles_and_moves_from_another_thread_are_seen_whole(dspfx, torch_cuda):
    """Room 3 is full at 32 seats.  While 50 blocks are submitted, another thread moves channel 40 out of it and back in and
    switches the mode at every move.  Every block's output is the host model's for one of the two seatings, wholly, whichever
    mode the run was in (integers, raw sums: the model is exact)."""
    torch = torch_cuda
    nf = 128
    seats = [32, 32, 32, 32, 64, 192, 64]
    k = integers(nf, TABLE[-1], 731)
    dk = device_block(dspfx, torch, k, 0)
    model = S.Bank(TABLE, seats)
    mm = seated(dspfx, seats=seats, nf=nf, normalise=False)
    try:
        inside = bits(int_product(model, k))
        model.assign(NONE, 40)
        outside = bits(int_product(model, k))
        assert (inside[:, 34:66] != outside[:, 34:66]).any() and (outside[:, 40] == 0).all()
        mm.set_staging(dspfx.MIXMATRIX_STAGED)            # (the copies are allocated here, not by the thread's first toggle)
        assert (bits(run(dspfx, torch, mm, k)) == inside).all()
        outs = [fresh_out(torch, k.size) for _ in range(50)]
        stop = threading.Event()
        moves = [0]

        def mover():
            while not stop.is_set() and moves[0] < 400:   # (bounded: every move waits in the queue until the next run takes it)
                mm.assign(NONE, 40)
                mm.set_staging(dspfx.MIXMATRIX_DIRECT)
                mm.assign(3, 40)
                mm.set_staging(dspfx.MIXMATRIX_STAGED)
                moves[0] += 2

        t = threading.Thread(target=mover)
        t.start()
        try:
            for o in outs:
                mm.run(dk, nf, out=o)
        finally:
            stop.set()
            t.join()
        torch.cuda.synchronize()
        assert moves[0] > 0 and mm.staging == dspfx.MIXMATRIX_STAGED and mm.seat_of()[40] == 6
        assert (bits(run(dspfx, torch, mm, k)) == inside).all()
        for o in outs:
            got = bits(read_out(dspfx, o, nf, TABLE[-1], 0))
            assert (got == inside).all() or (got == outside).all(), "a run saw half a move, or half a mode"
    finally:
        mm.close()


# ---- 6. the full size ----------------------------------------------------------------------------------------------------------

def test_full_size_every_channel_reseated_at_random(dspfx, torch_cuda):
    """N = 2^20 in 4096 rooms of 256 with 256 seats each, 128 frames, tiled 256, every channel reseated at random by assign (as
    tools/mixmatrix_rate.py --moved 1 does).  Device events, the median of 20 after 5 warm-ups.  Asserted: a staged run takes no
    longer than the 2.667 ms a block lasts, and less than the direct run at the same seating.  Printed: both modes at identity
    seating and their ratio, the staged run's fraction of 8 TB/s on its own bytes, and its ratio to a flat copy of the block."""
    torch = torch_cuda
    n, size, nf, tile = 1 << 20, 256, 128, 256
    torch.manual_seed(7)
    dx = torch.rand(nf * n, dtype=torch.float32, device="cuda") * 2.0 - 0.75
    out = torch.empty_like(dx)
    mm = dspfx.MixMatrix(n, group_size=size, tile_channels=tile, max_frames=nf, seats=size)
    rows = np.random.default_rng(8).uniform(0.0, 10.0, (3, size)).astype(np.float32)
    rows[1, 5] = 0.0
    _, _, _, table_bytes = dspfx.mixmatrix_plan(n, group_size=size, tile_channels=tile, seats=size)
    extra = dspfx.mixmatrix_staging_bytes(n, size, group_size=size, tile_channels=tile, max_frames=nf)
    assert extra == (1 << 30) + (4 << 20)

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

    def both_modes():
        ms = {}
        for name, mode in (("direct", dspfx.MIXMATRIX_DIRECT), ("staged", dspfx.MIXMATRIX_STAGED)):
            mm.set_staging(mode)
            ms[name] = timed(lambda: mm.run(dx, nf, out=out))
            ms[name + " bits"] = (out[:nf * size].view(torch.int32).clone(), out[-nf * size:].view(torch.int32).clone(),
                                  int(out.view(torch.int32).to(torch.int64).sum().item()))
        assert all(torch.equal(a, b) if torch.is_tensor(a) else a == b for a, b in zip(ms["direct bits"], ms["staged bits"])), "the modes differ"
        return ms

    try:
        mm.set_rows(rows, 0)
        mm.set_rows(rows, n - size + 100)
        assert mm.scatter() == (n // 32, n // 32)
        identity = both_modes()
        rng = np.random.default_rng(9)                   # everybody leaves, then everybody is dealt back into the freed seats
        mm.assign(np.full(n, dspfx.NO_ROOM, np.uint32))
        mm.assign(rng.permutation(np.repeat(np.arange(n // size), size)).astype(np.uint32))
        chunks, lines = mm.scatter()
        assert chunks == n // 32 and lines / chunks > 31.0
        shuffled = both_modes()
        ms_copy = timed(lambda: out.copy_(dx))
    finally:
        mm.close()
    own = 2 * nf * n * 4 + table_bytes + 4 * (nf * n * 4)   # the block in and out, the tables, and four more passes over the block
    staged, direct = shuffled["staged"], shuffled["direct"]
    print(f"mixmatrix staged, full size, every channel reseated ({lines / chunks:.2f} lines per chunk): staged {staged:.4f} ms | direct {direct:.4f} ms"
          f" | identity seating: staged {identity['staged']:.4f} ms, direct {identity['direct']:.4f} ms, x {identity['staged'] / identity['direct']:.3f}"
          f" | staged on its own {own / 2**30:.2f} GiB: {own / (staged * 1e-3) / 8e12:.3f} of 8 TB/s | flat copy {ms_copy:.4f} ms, x {staged / ms_copy:.2f}")
    assert staged <= 128.0 / 48000.0 * 1e3, f"{staged:.4f} ms per staged run, and a block lasts 2.667 ms"
    assert staged < direct, f"staged {staged:.4f} ms, direct {direct:.4f} ms at the same seating"
