"""The sparse mix-matrix run on the GPU (dspfx_mixmatrix_run_sparse, MixMatrix.run(sources=...)) and the talker bank's audible list
(dspfx_talkers_audible_views, Talkers.audible()).  The dense run of the same bank is the oracle: sparse on the UNMASKED block equals
dense on the block with every unlisted channel set to +0.0 (and to -0.0), compared as uint32 -- unseated, seated at the identity
seating and after the scripted walk of tests/test_mixmatrix_seats_gpu.py.  Then integers against the int64 product, list hygiene,
unlisted NaNs, the other rows of the contract, the staged mode, the two banks end to end on one stream, and the full size."""
import numpy as np
import pytest

import audible_ref as A
import mixmatrix_ref as X
import mixseats_ref as S

pytestmark = pytest.mark.gpu

TABLE, SEATS, N, G = A.TABLE, A.SEATS, A.N, A.G
NONE = S.NONE
SENTINEL = 0x7FC0BEEF                                    # a NaN no arithmetic produces
SLACK = 4096
LAYOUTS = [0, 64]                                        # frame-major; tiled 64 (320 = 5 tiles)
FRAMES = [37, 128, 161]                                  # 161: a second frame pass
KS = [0, 1, 2, 3, 32, 33, None]                          # listed sources per room; None: all members.  32 / 33: one chunk, and one more
KINDS = ["plain", "seated", "walked"]
WALK = [([NONE, 3, 3, 3, NONE], 36), ([4], 5), ([5], 0), ([1] * 30 + [2] * 2, 100), ([2, 1, 2, 2, 4, 2, 2, 2, 2, 1], 1), ([3], 40)]


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
    got = dspfx.from_layout(h[:nf * n], nf, n, tile)
    assert (bits(got) != SENTINEL).all(), "a sample of the block was not written"
    return got


def run(dspfx, torch, mm, x, tile=0, sources=None):
    nf, n = x.shape
    out = fresh_out(torch, nf * n)
    mm.run(device_block(dspfx, torch, x, tile), nf, out=out, sources=sources)
    torch.cuda.synchronize()
    return read_out(dspfx, out, nf, n, tile)


def noise(nf, n, seed):
    return (np.random.default_rng(seed).uniform(-1.0, 1.0, (nf, n)) + 0.25).astype(np.float32)


def integers(nf, n, seed):
    return np.random.default_rng(seed).integers(-512, 513, (nf, n)).astype(np.float32)


def weights(seed):
    """a signed finite gain for every (listener, source) pair of channel numbers: random_mats' distribution minus 3"""
    return A.signed_mats([0, N], seed)[0]


def bank(dspfx, kind, tile=0, nf=128, normalise=True, mats=None, seed=3):
    """-> a bank of `kind` holding `mats` (per room of TABLE, [n][n]; None: signed random ones).  "walked": the seated bank after
    the scripted walk, wired between every two channels of a room by weights()"""
    if mats is None:
        mats = A.signed_mats(TABLE, seed)
    if kind == "plain":
        mm = dspfx.MixMatrix(N, group_start=TABLE, tile_channels=tile, max_frames=nf, normalise=normalise)
        for (c0, n), m in zip(X.rooms(TABLE), mats):
            mm.set_rows(m, c0)
        return mm
    mm = dspfx.MixMatrix(N, group_start=TABLE, tile_channels=tile, max_frames=nf, normalise=normalise, seats=SEATS)
    if kind == "seated":
        for g, ((c0, n), m) in enumerate(zip(X.rooms(TABLE), mats)):
            rows = np.zeros((n, int(mm.seats[g])), np.float32)
            rows[:, :n] = m
            mm.set_rows(rows, c0)
        return mm
    for ids, first in WALK:
        mm.assign(ids, first)
    rewire(mm, weights(seed))
    return mm


def rewire(mm, w):
    """w[l][s] between every two channels of a room, by channel number"""
    room = mm.room_of()
    ls, ss = [], []
    for g in range(G):
        chan = np.flatnonzero(room == g)
        l, s = np.meshgrid(chan, chan, indexing="ij")
        ls.append(l.reshape(-1)), ss.append(s.reshape(-1))
    ls, ss = np.concatenate(ls), np.concatenate(ss)
    mm.set_pairs(ls, ss, w[ls, ss])


def choose(room_of, rot, seed):
    """per room a list of K of its channels, ascending; K = KS rotated by `rot` over the rooms, at most the room's members"""
    rng = np.random.default_rng(1000 * seed + rot)
    lists = []
    for g in range(G):
        chan = np.flatnonzero(room_of == g)
        k = KS[(g + rot) % len(KS)]
        k = len(chan) if k is None else min(k, len(chan))
        lists.append(np.sort(rng.choice(chan, k, replace=False)).astype(np.int64))
    return lists


def pack(torch, segments, counts=None, tail=()):
    """segments: per room the entries of its segment, as given -> (list int32, start uint32[G + 1], count uint32[G]) on the device;
    counts overrides the segments' lengths; tail: entries behind the last segment"""
    start = np.concatenate([[0], np.cumsum([len(s) for s in segments])]).astype(np.uint32)
    count = np.asarray([len(s) for s in segments] if counts is None else counts, np.uint32)
    lst = np.concatenate([np.asarray(s, np.int64) for s in segments] + [np.asarray(tail, np.int64)]).astype(np.int32)
    if len(lst) == 0:
        lst = np.full(1, -1, np.int32)
    return torch.from_numpy(lst).cuda(), torch.from_numpy(start).cuda(), torch.from_numpy(count).cuda()


def masked(x, lists, room_of, zero=0.0):
    """x with every channel that is not listed IN ITS OWN ROOM set to `zero`"""
    keep = np.zeros(x.shape[1], bool)
    for g, l in enumerate(lists):
        l = np.asarray(l, np.int64)
        l = l[(l >= 0) & (l < x.shape[1])]
        keep[l[room_of[l] == g]] = True
    out = x.copy()
    out[:, ~keep] = np.float32(zero)
    return out


def same(got, want, what=""):
    assert (bits(got) == bits(want)).all(), (what, np.argwhere(bits(got) != bits(want))[:5])


# ---- 1. the dense run as the oracle ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("tile", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_sparse_on_the_block_is_dense_on_the_masked_block(dspfx, torch_cuda, kind, tile, nf):
    torch = torch_cuda
    x = noise(nf, N, 200 + nf)
    mm = bank(dspfx, kind, tile, nf)
    try:
        room = mm.room_of()
        ks = set()
        for rot in range(len(KS)):                        # every room meets every K
            lists = choose(room, rot, nf)
            ks |= {len(l) for l in lists}
            got = run(dspfx, torch, mm, x, tile, pack(torch, lists))
            assert np.isfinite(got).all()
            same(got, run(dspfx, torch, mm, masked(x, lists, room, 0.0), tile), (rot, "+0.0"))
            same(got, run(dspfx, torch, mm, masked(x, lists, room, -0.0), tile), (rot, "-0.0"))
        assert {0, 1, 2, 3, 32, 33} <= ks and max(ks) == np.bincount(room[room != NONE]).max() >= 129      # (129: the largest room after the walk)
        everybody = [np.flatnonzero(room == g) for g in range(G)]
        same(run(dspfx, torch, mm, x, tile, pack(torch, everybody)), run(dspfx, torch, mm, x, tile), "everybody listed")
        assert (bits(got[:, room == NONE]) == 0).all()
    finally:
        mm.close()


# ---- 2. integers ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("tile", LAYOUTS)
@pytest.mark.parametrize("kind", ["plain", "seated"])
def test_integers_give_the_int64_product_of_the_listed_sources(dspfx, torch_cuda, kind, tile, nf):
    torch = torch_cuda
    k = integers(nf, N, 300 + nf)
    mats = [X.asymmetric(n) for _, n in X.rooms(TABLE)]
    mm = bank(dspfx, kind, tile, nf, normalise=False, mats=mats)
    try:
        room = mm.room_of()
        for rot in (0, 2, 5):
            lists = choose(room, rot, 7 + nf)
            want = X.scaled_int_product(masked(k, lists, room), TABLE, mats, 0)
            same(run(dspfx, torch, mm, k, tile, pack(torch, lists)), want, rot)
    finally:
        mm.close()


# ---- 3. list hygiene --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_a_dirty_list_gives_the_bits_of_the_clean_one(dspfx, torch_cuda, kind):
    """duplicates, channels of another room, entries >= N, negative entries, a descending segment, and a count that reaches past
    list_len (behind which the tensor goes on with entries that would count)"""
    torch = torch_cuda
    nf = 37
    x = noise(nf, N, 41)
    mm = bank(dspfx, kind, 0, nf)
    try:
        room = mm.room_of()
        rng = np.random.default_rng(42)
        clean = choose(room, 3, 43)
        want = run(dspfx, torch, mm, x, 0, pack(torch, clean))
        same(want, run(dspfx, torch, mm, masked(x, clean, room), 0))
        dirty = []
        for g, l in enumerate(clean):
            others = np.flatnonzero((room != g) & (room != NONE))
            seg = np.concatenate([l[::-1], l[:3], rng.choice(others, 5), [N, N + 5, 2 ** 31 - 1, -1, -7, -2 ** 31], l[-2:]])
            dirty.append(seg[rng.permutation(len(seg))] if g % 2 else seg)
        same(run(dspfx, torch, mm, x, 0, pack(torch, dirty)), want, "dirty")
        # the last room's count reaches 50 entries past list_len; the tensor goes on there with unlisted members of that room
        unlisted = np.setdiff1d(np.flatnonzero(room == G - 1), clean[G - 1])
        assert len(unlisted) >= 8
        counts = [len(l) for l in clean]
        counts[G - 1] += 50
        lst, start, count = pack(torch, clean, counts, tail=unlisted[:8])
        same(run(dspfx, torch, mm, x, 0, (lst[:len(lst) - 8], start, count)), want, "count past list_len")
        # ... which do count once list_len covers them
        more = [l.copy() for l in clean]
        more[G - 1] = np.sort(np.concatenate([clean[G - 1], unlisted[:8]]))
        same(run(dspfx, torch, mm, x, 0, (lst, start, count)), run(dspfx, torch, mm, x, 0, pack(torch, more)), "the control")
        assert (bits(run(dspfx, torch, mm, x, 0, pack(torch, more))) != bits(want)).any()
        # a start past the list, and a count above the largest room: nothing is read outside the list
        far = (lst, torch.from_numpy(np.full(G + 1, 2 ** 32 - 1, np.uint32)).cuda(), torch.from_numpy(np.full(G, 2 ** 32 - 1, np.uint32)).cuda())
        same(run(dspfx, torch, mm, x, 0, far), run(dspfx, torch, mm, x, 0, pack(torch, [[] for _ in range(G)])), "start past the list")
    finally:
        mm.close()


# ---- 4. unlisted sources are not read -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_an_unlisted_nan_reaches_nobody_and_a_listed_one_its_own_room(dspfx, torch_cuda, kind, tile):
    torch = torch_cuda
    nf = 37
    x = noise(nf, N, 51)
    mm = bank(dspfx, kind, tile, nf)
    try:
        room = mm.room_of()
        lists = choose(room, 4, 52)                       # (no room lists everybody it could: rot 4 gives room 5 K = 2)
        src = pack(torch, lists)
        xp = x.copy()
        for g in range(G):
            out = np.setdiff1d(np.flatnonzero(room == g), lists[g])
            if len(out):
                xp[:, out[0]] = np.nan
                xp[3, out[-1]] = np.inf if g % 2 else -np.inf
        assert not np.isfinite(xp).all()
        got = run(dspfx, torch, mm, xp, tile, src)
        assert np.isfinite(got).all(), "an unlisted source was read"
        same(got, run(dspfx, torch, mm, masked(x, lists, room), tile))
        assert not np.isfinite(run(dspfx, torch, mm, xp, tile)).all(), "(the dense run does read them)"
        g = next(g for g in range(G) if len(lists[g]) >= 2)
        xl = x.copy()
        xl[:, lists[g][1]] = np.nan
        got = run(dspfx, torch, mm, xl, tile, src)
        assert np.isnan(got[:, room == g]).all(), "a listed NaN reaches every listener of its room"
        assert np.isfinite(got[:, room != g]).all(), "... and nobody else"
    finally:
        mm.close()


# ---- 5. the other rows of the contract ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_unwired_rows_raw_sums_and_no_room(dspfx, torch_cuda, kind):
    torch = torch_cuda
    nf = 37
    x = noise(nf, N, 61)
    for normalise in (True, False):
        mm = bank(dspfx, kind, 0, nf, normalise=normalise)
        try:
            room = mm.room_of()
            quiet = [int(np.flatnonzero(room == g)[-1]) for g in (2, 5)]         # two listeners hear nobody
            for c in quiet:
                others = np.flatnonzero(room == room[c])
                mm.set_pairs(np.full(len(others), c), others, 0.0)
            if kind != "plain":
                mm.assign(NONE, 70)
                room = mm.room_of()
                assert room[70] == NONE
            lists = choose(room, 1, 62)
            lists[4] = np.sort(np.append(lists[4], 70))                          # channel 70 sat in room 4
            got = run(dspfx, torch, mm, x, 0, pack(torch, lists))
            same(got, run(dspfx, torch, mm, masked(x, lists, room), 0), normalise)
            assert (bits(got[:, quiet]) == 0).all(), "a row without a wired entry gives +0.0"
            assert (bits(got[:, room == NONE]) == 0).all(), "a channel in no room reads +0.0"
            assert np.abs(got).max() > 0
        finally:
            mm.close()


@pytest.mark.parametrize("kind", ["plain", "walked"])
def test_stores_between_two_sparse_runs_govern_the_second_only(dspfx, torch_cuda, kind):
    """set_rows / set_pairs (and an assign on the seated bank) queued between two sparse runs, with no synchronisation: a twin bank's
    dense runs on the masked block, before and after the same stores, are the oracle"""
    torch = torch_cuda
    nf = 128
    x = noise(nf, N, 71)
    dx = device_block(dspfx, torch, x, 0)
    mm, twin = bank(dspfx, kind, 0, nf), bank(dspfx, kind, 0, nf)
    try:
        room = mm.room_of()
        lists = choose(room, 1, 72)                       # (rot 1: the rooms the stores touch, 3, 4 and 5, list 32, 33 and everybody)
        src = pack(torch, lists)
        w = weights(73)

        def stores(b):
            if kind == "plain":
                b.set_rows(np.full((2, 160), -2.5, np.float32), 100)
            else:
                b.assign([5, NONE, 3, 4], 64)
                rewire(b, w)
            b.set_pairs([120], [121], [0.0])

        old = run(dspfx, torch, twin, masked(x, lists, room), 0)
        stores(twin)
        room2 = twin.room_of()
        new = run(dspfx, torch, twin, masked(x, lists, room2), 0)
        assert (bits(old) != bits(new)).any()
        o1, o2 = fresh_out(torch, x.size), fresh_out(torch, x.size)
        mm.run(dx, nf, out=o1, sources=src)               # (no synchronisation between the calls)
        stores(mm)
        mm.run(dx, nf, out=o2, sources=src)
        torch.cuda.synchronize()
        same(read_out(dspfx, o1, nf, N, 0), old, "the first run")
        same(read_out(dspfx, o2, nf, N, 0), new, "the second run")
    finally:
        mm.close()
        twin.close()


# ---- 6. the staged mode -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("tile", LAYOUTS)
def test_the_staged_sparse_run_has_the_direct_bits_in_place_too(dspfx, torch_cuda, tile, nf):
    """after a shuffle of all seats: everybody leaves, then enters a room drawn at random"""
    torch = torch_cuda
    x = noise(nf, N, 81 + nf)
    mm = dspfx.MixMatrix(N, group_start=TABLE, tile_channels=tile, max_frames=nf, seats=SEATS)
    try:
        ids = np.random.default_rng(82).permutation(mm.room_of())
        mm.assign([NONE] * N, 0)
        mm.assign(ids, 0)
        rewire(mm, weights(83))
        room = mm.room_of()
        assert (room == ids).all() and mm.scatter()[1] > 2 * mm.scatter()[0]
        for rot in (0, 3, 6):
            lists = choose(room, rot, 84)
            src = pack(torch, lists)
            mm.set_staging(dspfx.MIXMATRIX_DIRECT)
            want = run(dspfx, torch, mm, x, tile, src)
            same(want, run(dspfx, torch, mm, masked(x, lists, room), tile), rot)
            dx = device_block(dspfx, torch, x, tile)
            with pytest.raises(dspfx.DspfxError) as e:
                mm.run(dx, nf, out=dx, sources=src)
            assert e.value.status == -1 and "overlaps" in str(e.value)
            mm.set_staging(dspfx.MIXMATRIX_STAGED)
            same(run(dspfx, torch, mm, x, tile, src), want, (rot, "staged"))
            buf = fresh_out(torch, x.size)
            buf[:x.size] = dx
            assert mm.run(buf, nf, out=buf, sources=src) is buf
            torch.cuda.synchronize()
            same(read_out(dspfx, buf, nf, N, tile), want, (rot, "staged, in place"))
            with pytest.raises(dspfx.DspfxError):
                mm.run(buf, nf, out=buf[4:], sources=src)                        # a partial overlap
    finally:
        mm.close()


def test_refusals(dspfx, torch_cuda):
    torch = torch_cuda
    nf = 37
    mm = bank(dspfx, "plain", 0, nf)
    try:
        dx, out = device_block(dspfx, torch, noise(nf, N, 91), 0), fresh_out(torch, nf * N)
        lst, start, count = pack(torch, choose(mm.room_of(), 0, 92))
        for args in ((lst, start[:-1], count), (lst, start, count[:-1]), (lst.float(), start, count)):
            with pytest.raises(dspfx.DspfxError) as e:
                mm.run(dx, nf, out=out, sources=args)
            assert e.value.status == -1
        with pytest.raises(dspfx.DspfxError):
            mm.run(dx, nf + 1, out=out, sources=(lst, start, count))
        L = dspfx.lib()
        assert L.dspfx_mixmatrix_run_sparse(mm.h, dx.data_ptr(), nf, out.data_ptr(), None, 0, start.data_ptr(), count.data_ptr(), None) == -1
        assert b"run_sparse" in L.dspfx_mixmatrix_last_error(mm.h)
        torch.cuda.synchronize()
        assert (out.view(torch.int32) == SENTINEL).all(), "a refused run writes nothing"
    finally:
        mm.close()


# ---- 7. the two banks end to end ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", LAYOUTS)
def test_talkers_into_the_sparse_run_on_one_stream(dspfx, torch_cuda, tile):
    """the script of audible_ref (12 blocks, talkers changing, an OPEN and a SHUT pin, a reset, an assign made in both banks): every
    block the sparse run over Talkers.audible() equals the dense run on the same gated block, and the device tables equal
    dspfx_talkers_audible of the restatement's gate and target.  A second bank that never asks for the list gives what it always
    gave."""
    torch = torch_cuda
    ref, pins, blocks = A.script()
    stream = torch.cuda.Stream()
    talk = dspfx.Talkers(N, group_start=TABLE, top=A.TOP, tile_channels=tile, max_frames=A.NF)
    quiet = dspfx.Talkers(N, group_start=TABLE, top=A.TOP, tile_channels=tile, max_frames=A.NF)        # never calls audible()
    mm = dspfx.MixMatrix(N, group_start=TABLE, tile_channels=tile, max_frames=A.NF, seats=SEATS)
    try:
        rewire(mm, weights(93))
        for b in (talk, quiet):
            b.set_detector(48.0, 2000.0)
            b.set_pin(pins)
        aud = talk.audible()
        assert [tuple(t.shape) for t in aud] == [(N,), (G + 1,), (G,)] and all(t.is_cuda for t in aud)
        assert [t.data_ptr() for t in talk.audible()] == [t.data_ptr() for t in aud], "the pointers are stable"
        sparse_rooms = 0
        for b, (x, act) in enumerate(blocks):
            if act and act[0] == "reset":
                for t in (talk, quiet, ref):
                    t.reset(act[1], act[2])
            if act and act[0] == "assign":
                for t in (talk, quiet, ref, mm):
                    assert t.assign(act[1], act[2]) is not False
            gate, target, room = ref.gate.copy(), ref.target.copy(), ref.room_of()
            want = ref.run(x)
            dx = device_block(dspfx, torch, x, tile)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):               # the list's producer and its consumer on one stream, nothing between them
                dy = talk.run(dx, A.NF, stream=stream.cuda_stream)
                sparse = mm.run(dy, A.NF, out=fresh_out(torch, x.size), stream=stream.cuda_stream, sources=aud)
                dense = mm.run(dy, A.NF, out=fresh_out(torch, x.size), stream=stream.cuda_stream)
            stream.synchronize()
            y = dspfx.from_layout(dy.cpu().numpy(), A.NF, N, tile)
            same(y, want, (b, "the gated block"))
            same(read_out(dspfx, sparse, A.NF, N, tile), read_out(dspfx, dense, A.NF, N, tile), (b, "sparse against dense"))
            got = tuple(t.cpu().numpy() for t in aud)
            lists = A.check_tables(got, gate, target, room, G)
            A.check_tables(dspfx.talkers_audible(gate, target, room, G), gate, target, room, G)
            assert (mm.room_of() == room).all()
            sparse_rooms += sum(len(l) < (room == g).sum() for g, l in enumerate(lists))
            # the bank that never asked: the same output as the restatement, as always
            qy = quiet.run(dx, A.NF)
            torch.cuda.synchronize()
            same(dspfx.from_layout(qy.cpu().numpy(), A.NF, N, tile), want, (b, "the bank without a list"))
            # a metering run leaves the list's tables
            if b in (3, 9):
                talk.run(dx, A.NF, gate=False)
                quiet.run(dx, A.NF, gate=False)
                ref.run(x, gate=False)
                torch.cuda.synchronize()
                for t, g in zip(aud, got):
                    assert np.array_equal(t.cpu().numpy(), g), "a metering run wrote the tables"
            for bankk in (talk, quiet):                   # both banks' tables are the restatement's
                assert np.array_equal(bits(bankk.levels().cpu().numpy()), bits(ref.level)), b
                assert np.array_equal(bankk.talkers().cpu().numpy(), ref.talkers), b
                assert np.array_equal(bits(bankk.targets().cpu().numpy()), bits(ref.target)), b
        assert sparse_rooms > 30, "most rooms, most blocks, list fewer than their members"
    finally:
        talk.close()
        quiet.close()
        mm.close()


# ---- 8. the full size -----------------------------------------------------------------------------------------------------------

def test_full_size(dspfx, torch_cuda):
    """N = 2^20 in 4096 rooms of 256, 128 frames, tiled 256, top 3, noise with a loudness per channel, two blocks in turn so that
    the talkers change and a room lists up to 2 * top members.  The sparse run fits the 2.667 ms block and takes at most the dense
    run on the same buffers (a guard against a spill or an uncoalesced path: with at most 6 of 256 sources listed it does strictly
    less of every kind of work).

    Measured, one box, one run: the line this test prints is quoted in DESIGN.md section 8."""
    torch = torch_cuda
    n, size, nf, tile, top = 1 << 20, 256, 128, 256, 3
    free, _ = torch.cuda.mem_get_info()
    if free < 6 << 30:                                    # a table of 1 GiB, four blocks of 512 MiB, and room to spare
        pytest.skip("device memory is short")
    torch.manual_seed(11)
    blocks = []
    for _ in range(2):                                    # [tile][frame][channel of the tile]: a loudness per channel
        loud = torch.rand(n // tile, 1, tile, device="cuda") * 0.95 + 0.05
        blocks.append(((torch.rand(n // tile, nf, tile, device="cuda") * 2.0 - 1.0) * loud).reshape(-1))
    y, out = torch.empty_like(blocks[0]), torch.empty_like(blocks[0])
    talk = dspfx.Talkers(n, group_size=size, top=top, tile_channels=tile, max_frames=nf)
    off = dspfx.Talkers(n, group_size=size, top=top, tile_channels=tile, max_frames=nf)
    mm = dspfx.MixMatrix(n, group_size=size, tile_channels=tile, max_frames=nf)
    rows = np.random.default_rng(12).uniform(-3.0, 7.0, (3, size)).astype(np.float32)
    rows[1, 5] = 0.0
    try:
        mm.set_rows(rows, 0)
        mm.set_rows(rows, n - size + 100)
        for t in (talk, off):
            t.set_detector(48.0, 2000.0)
        aud = talk.audible()
        for i in range(6):                                # the steady state: from the third block a room lists talkers and faders only
            talk.run(blocks[i % 2], nf, out=y)
            off.run(blocks[i % 2], nf, out=out)
        torch.cuda.synchronize()
        count = aud[2].cpu().numpy()
        assert 1 <= count.min() and count.max() <= 2 * top, (count.min(), count.max())

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

        # y is the last gated block and the tables are its own: the mixes first, the talker banks (which move on) last
        ms_dense = timed(lambda: mm.run(y, nf, out=out))
        dense_first, dense_last = out[:nf * size].clone(), out[-nf * size:].clone()
        ms_copy = timed(lambda: out.copy_(y))
        out.fill_(float("nan"))
        ms = timed(lambda: mm.run(y, nf, out=out, sources=aud))
        torch.cuda.synchronize()
        sparse_first, sparse_last = out[:nf * size].clone(), out[-nf * size:].clone()
        y_first, y_last = y[:nf * size].clone(), y[-nf * size:].clone()
        turn = [0]

        def gated(t):
            turn[0] += 1
            t.run(blocks[turn[0] % 2], nf, out=out)

        ms_on = timed(lambda: gated(talk))
        ms_off = timed(lambda: gated(off))
        listed = int(count.sum())
        moved = 4 * (n * nf + 2 * listed * nf + listed * size)                   # out, the listed samples per listener tile, their table rows
        print(f"mixmatrix sparse, full size, {listed / len(count):.2f} of {size} sources listed per room: {ms:.4f} ms per run "
              f"({moved / (ms * 1e-3) / 8e12:.3f} of 8 TB/s on its own {moved / 2 ** 20:.0f} MiB) | dense {ms_dense:.4f} ms | flat copy {ms_copy:.4f} ms | "
              f"talkers gated run with the list {ms_on:.4f} ms, without {ms_off:.4f} ms (talkers_audible: {ms_on - ms_off:+.4f} ms)")
        # the first and the last room against float64, and against the dense run's bits (every unlisted sample of y is a zero)
        for c0, sparse, yr, dense in ((0, sparse_first, y_first, dense_first), (n - size, sparse_last, y_last, dense_last)):
            got = sparse.cpu().numpy().reshape(nf, size)
            xr = yr.cpu().numpy().reshape(nf, size)
            m = (1.0 - np.eye(size)).astype(np.float32)
            r0 = 0 if c0 == 0 else 100
            m[r0:r0 + 3] = rows
            exact, sabs, _ = X.exact(xr, [0, size], [m], True)
            k = float(count[0 if c0 == 0 else -1])
            err = np.abs(got.astype(np.float64) - exact)
            assert (err <= X.bound(sabs, np.full(size, k))).all(), float((err / X.bound(sabs, np.full(size, k))).max())
            assert np.array_equal(bits(got), bits(dense.cpu().numpy().reshape(nf, size)))
        assert ms <= 128.0 / 48000.0 * 1e3, f"{ms:.4f} ms per run, and a block lasts 2.667 ms"
        assert ms <= ms_dense, f"the sparse run takes {ms:.4f} ms and the dense run {ms_dense:.4f} ms"
    finally:
        talk.close()
        off.close()
        mm.close()
