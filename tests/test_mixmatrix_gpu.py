"""The mix-matrix bank on the GPU (dspfx_mixmatrix_*, through the C ABI): exact on integers, inside the derived bound against
float64 (mixmatrix_ref: no measured constant), a fresh bank against MixGroups.returns, a room's bits independent of everything but
the room, the store contract, and the standing real-time condition at 2^20 channels."""
import threading

import numpy as np
import pytest

import mixgroups_ref as R
import mixmatrix_ref as X
import mixreturns_ref as M

pytestmark = pytest.mark.gpu

RAGGED = [0, 1, 3, 34, 66, 99, 355, 612, 1636]          # n = 1, 2, 31, 32, 33, 256, 257, 1024
PADDED = RAGGED + [1700, 1764, 1792]                     # ... padded up to a multiple of 256 by rooms of 64 (and the 28 left)
SENTINEL = 0x7FC0BEEF                                    # a NaN no arithmetic produces
SLACK = 4096


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bank(dspfx, table, tile=0, nf=128, normalise=True, mats=None):
    mm = dspfx.MixMatrix(int(table[-1]), group_start=table, tile_channels=tile, max_frames=nf, normalise=normalise)
    if mats is not None:
        for (c0, n), m in zip(X.rooms(table), mats):
            mm.set_rows(m, c0)
    return mm


def device_block(dspfx, torch, x, tile):
    return torch.from_numpy(dspfx.to_layout(np.ascontiguousarray(x, np.float32), tile).reshape(-1).copy()).cuda()


def fresh_out(torch, size):
    return torch.full((size + SLACK,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def read_out(dspfx, out, nf, n, tile):
    """-> [nf][n] frame-major on the host; the slack behind the block must still hold the sentinel"""
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


def int_product(x, table, mats):
    """the int64 result of integer matrices on integer samples, as f32"""
    out = np.zeros(x.shape, np.int64)
    xi = x.astype(np.int64)
    for (c0, n), m in zip(X.rooms(table), mats):
        out[:, c0:c0 + n] = xi[:, c0:c0 + n] @ np.asarray(m).astype(np.int64).T
    assert np.abs(out).max() < 1 << 24
    return out.astype(np.float32)


# ---- 1. exact on integers ------------------------------------------------------------------------------------------------------

LAYOUTS = {"fm1636": (RAGGED, 0), "fm1637": (RAGGED + [1637], 0), "tile64": (PADDED, 64), "tile256": (PADDED, 256)}


@pytest.mark.parametrize("nf", [1, 31, 37, 128])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_exact_integers(dspfx, torch_cuda, layout, nf):
    """Asymmetric integer matrices in [-3, 3] on integer samples in [-512, 512], raw sums: every partial sum is below
    1024 * 3 * 512 < 2^24, so any order is exact and the output is the int64 product bit for bit.  A transposed operand, a wrong
    k map or a row-column swap in the C write all change it."""
    table, tile = LAYOUTS[layout]
    mats = [X.asymmetric(n) for _, n in X.rooms(table)]
    x = integers(nf, table[-1], nf)
    mm = bank(dspfx, table, tile, nf, normalise=False, mats=mats)
    try:
        got = run(dspfx, torch_cuda, mm, x, tile)
    finally:
        mm.close()
    want = int_product(x, table, mats)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, (len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


def test_exact_integers_second_frame_pass(dspfx, torch_cuda):
    """161 frames: a workgroup takes 128, so the block needs a second pass, cut at frame 33 of its tile (tiled 64: the rows of a
    tile are 161 apart)."""
    table, tile, nf = PADDED, 64, 161
    mats = [X.asymmetric(n) for _, n in X.rooms(table)]
    x = integers(nf, table[-1], nf)
    mm = bank(dspfx, table, tile, nf, normalise=False, mats=mats)
    try:
        got = run(dspfx, torch_cuda, mm, x, tile)
    finally:
        mm.close()
    assert (bits(got) == bits(int_product(x, table, mats))).all()


# ---- 2. the bound against float64 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalise", [True, False], ids=["normalise", "raw"])
@pytest.mark.parametrize("tile", [0, 256])
def test_bound_against_float64(dspfx, torch_cuda, tile, normalise):
    table, nf = PADDED, 37
    n = table[-1]
    x = noise(nf, n, 21)
    mats = X.random_mats(table, 22)
    silent = [(5, 7), (6, 256), (7, 1023), (4, 0)]       # (room, listener): rows of all zeros
    for r, l in silent:
        mats[r][l, :] = 0.0
    mm = bank(dspfx, table, tile, nf, normalise, mats)
    try:
        got = run(dspfx, torch_cuda, mm, x, tile)
    finally:
        mm.close()
    ref, sabs, n_of = X.exact(x, table, mats, normalise)
    bnd = X.bound(sabs, n_of)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / bnd).max())
    print(f"tile {tile} normalise {normalise}: worst err / bound = {worst:.4f}")
    assert np.isfinite(got).all()
    assert (err <= bnd).all(), (worst, np.argwhere(err > bnd)[:5])
    for r, l in silent:
        assert (bits(got[:, table[r] + l]) == 0).all(), "a row of zeros gives +0.0"


# ---- 3. a fresh bank is returns ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalise", [True, False], ids=["normalise", "raw"])
@pytest.mark.parametrize("tile", [0, 256])
def test_fresh_bank_equals_returns(dspfx, torch_cuda, tile, normalise):
    torch = torch_cuda
    table, nf = PADDED, 37
    n = table[-1]
    x = noise(nf, n, 31)
    dx = device_block(dspfx, torch, x, tile)
    mm = bank(dspfx, table, tile, nf, normalise)
    mg = dspfx.MixGroups(n, group_start=table, tile_channels=tile, max_frames=nf, normalise=normalise)
    try:
        out = fresh_out(torch, nf * n)
        mm.run(dx, nf, out=out)
        ret = mg.returns(dx, nf)
        torch.cuda.synchronize()
        got = read_out(dspfx, out, nf, n, tile)
        want = dspfx.from_layout(ret.cpu().numpy(), nf, n, tile)
        depth = dspfx.mixgroups_plan(n, group_start=table, tile_channels=tile).astype(np.float64)
    finally:
        mm.close()
        mg.close()
    ref, sabs, n_of = X.exact(x, table, X.mix_minus(table), normalise)
    rref, rsabs = M.returns_exact(x, table, None, normalise)
    both = X.bound(sabs, n_of) + R.bound(rsabs, rref, depth[M.group_of(table, n)][None, :] + 1.0)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"tile {tile} normalise {normalise}: worst |matrix - returns| / (sum of the bounds) = {float((err / both).max()):.4f}")
    assert (err <= both).all(), np.argwhere(err > both)[:5]
    assert (bits(got[:, 0]) == 0).all() and (bits(want[:, 0]) == 0).all()       # the room of one


# ---- 4. a room's bits depend on the room alone --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def base(dspfx, torch_cuda):
    """frame-major, 128 frames, the padded table, random matrices: what every independence check compares with"""
    x = noise(128, PADDED[-1], 41)
    mats = X.random_mats(PADDED, 42)
    mm = bank(dspfx, PADDED, 0, 128, True, mats)
    try:
        first = run(dspfx, torch_cuda, mm, x, 0)
        again = run(dspfx, torch_cuda, mm, x, 0)
    finally:
        mm.close()
    return x, mats, first, again


def test_same_bits_from_run_to_run(base):
    _, _, first, again = base
    assert np.isfinite(first).all() and (bits(first) == bits(again)).all()


@pytest.mark.parametrize("tile", [64, 256])
def test_same_bits_frame_major_and_tiled(dspfx, torch_cuda, base, tile):
    x, mats, first, _ = base
    mm = bank(dspfx, PADDED, tile, 128, True, mats)
    try:
        got = run(dspfx, torch_cuda, mm, x, tile)
    finally:
        mm.close()
    assert (bits(got) == bits(first)).all()


@pytest.mark.parametrize("tile", [0, 256])
def test_same_bits_with_37_frames(dspfx, torch_cuda, base, tile):
    x, mats, first, _ = base
    mm = bank(dspfx, PADDED, tile, 128, True, mats)
    try:
        got = run(dspfx, torch_cuda, mm, x[:37], tile)
    finally:
        mm.close()
    assert (bits(got) == bits(first[:37])).all()


@pytest.mark.parametrize("room", [1, 4, 6, 7, 10])
def test_same_bits_alone_and_among_neighbours(dspfx, torch_cuda, base, room):
    x, mats, first, _ = base
    c0, n = X.rooms(PADDED)[room]
    mm = bank(dspfx, [0, n], 0, 128, True, [mats[room]])
    try:
        got = run(dspfx, torch_cuda, mm, x[:, c0:c0 + n], 0)
    finally:
        mm.close()
    assert (bits(got) == bits(first[:, c0:c0 + n])).all()


@pytest.mark.parametrize("tile", [0, 64])
def test_neighbours_samples_never_reach_a_room(dspfx, torch_cuda, base, tile):
    """The masked-load case: every OTHER room carries NaN, +-inf and 1e38; the room itself keeps its finite samples and its bits.
    A lane past n_r that loaded the neighbour's sample against a zero matrix entry would turn the room NaN."""
    x, mats, first, _ = base
    poison = np.asarray([np.nan, np.inf, -np.inf, 1e38], np.float32)
    mm = bank(dspfx, PADDED, tile, 128, True, mats)
    try:
        for c0, n in X.rooms(PADDED):
            xp = np.tile(poison, (x.shape[0], x.shape[1] // 4 + 1))[:, :x.shape[1]].copy()
            xp[:, c0:c0 + n] = x[:, c0:c0 + n]
            got = run(dspfx, torch_cuda, mm, xp, tile)
            assert (bits(got[:, c0:c0 + n]) == bits(first[:, c0:c0 + n])).all(), (c0, n)
    finally:
        mm.close()


# ---- 5. stores -----------------------------------------------------------------------------------------------------------------

SMALL = [0, 5, 38, 294]                                  # n = 5, 33, 256


def small_int_mats(seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(-3, 4, (n, n)).astype(np.float32) for _, n in X.rooms(SMALL)]


def test_rows_then_columns_land_in_call_order(dspfx, torch_cuda):
    mats = small_int_mats(51)
    x = integers(37, SMALL[-1], 52)
    rows = np.full((4, 33), 2.0, np.float32)             # listeners 3..6 of the room of 33
    cols = np.full((3, 33), -3.0, np.float32)            # sources 5..7: overlaps the rows in a 2 x 3 patch, and must win there
    mm = bank(dspfx, SMALL, 0, 37, False, mats)
    try:
        mm.set_rows(rows, 5 + 3)
        mm.set_cols(cols, 5 + 5)
        got = run(dspfx, torch_cuda, mm, x)
        mm.set_cols(cols, 5 + 5)                         # ... and the other way round: the rows win
        mm.set_rows(rows, 5 + 3)
        got2 = run(dspfx, torch_cuda, mm, x)
    finally:
        mm.close()
    mats[1][3:7, :] = rows
    mats[1][:, 5:8] = cols.T
    assert (bits(got) == bits(int_product(x, SMALL, mats))).all()
    mats[1][3:7, :] = rows
    assert (bits(got2) == bits(int_product(x, SMALL, mats))).all()


def test_a_store_between_two_runs_changes_the_second_only(dspfx, torch_cuda):
    torch = torch_cuda
    mats = small_int_mats(53)
    new = small_int_mats(54)[2]
    x = integers(128, SMALL[-1], 55)
    dx = device_block(dspfx, torch, x, 0)
    mm = bank(dspfx, SMALL, 0, 128, False, mats)
    try:
        o1, o2 = fresh_out(torch, x.size), fresh_out(torch, x.size)
        mm.run(dx, 128, out=o1)                          # (no synchronisation between the three calls)
        mm.set_rows(new, 38)
        mm.run(dx, 128, out=o2)
        torch.cuda.synchronize()
        got1, got2 = read_out(dspfx, o1, 128, x.shape[1], 0), read_out(dspfx, o2, 128, x.shape[1], 0)
    finally:
        mm.close()
    assert (bits(got1) == bits(int_product(x, SMALL, mats))).all()
    assert (bits(got2) == bits(int_product(x, SMALL, mats[:2] + [new]))).all()


def test_fill_and_reset_restore_mix_minus(dspfx, torch_cuda):
    x = noise(37, SMALL[-1], 56)
    mm = bank(dspfx, SMALL, 0, 37, True)
    try:
        fresh = run(dspfx, torch_cuda, mm, x)
        for (c0, n), m in zip(X.rooms(SMALL), X.random_mats(SMALL, 57)):
            mm.set_rows(m, c0)
        changed = run(dspfx, torch_cuda, mm, x)
        assert (bits(changed) != bits(fresh)).any()
        mm.fill(1, dspfx.MIXMATRIX_ZERO)
        zeroed = run(dspfx, torch_cuda, mm, x)
        assert (bits(zeroed[:, 5:38]) == 0).all() and (bits(zeroed[:, 38:]) == bits(changed[:, 38:])).all()
        for room in range(3):
            mm.fill(room, dspfx.MIXMATRIX_MIX_MINUS)
        assert (bits(run(dspfx, torch_cuda, mm, x)) == bits(fresh)).all()
        mm.fill(None, dspfx.MIXMATRIX_ZERO)
        assert (bits(run(dspfx, torch_cuda, mm, x)) == 0).all()
        mm.reset()
        assert (bits(run(dspfx, torch_cuda, mm, x)) == bits(fresh)).all()
    finally:
        mm.close()


def test_a_bad_store_changes_nothing_and_says_why(dspfx, torch_cuda):
    x = noise(37, SMALL[-1], 58)
    mm = bank(dspfx, SMALL, 0, 37, True)
    try:
        fresh = run(dspfx, torch_cuda, mm, x)
        bad = [
            (mm.set_rows, np.ones((2, 5), np.float32), 4, "one room"),           # listeners 4 and 5 sit in two rooms
            (mm.set_cols, np.ones((2, 33), np.float32), 37, "one room"),
            (mm.set_rows, np.ones((1, 256), np.float32), 294, "not inside"),     # past N
            (mm.set_rows, np.ones((257, 256), np.float32), 38, "not inside"),
            (mm.set_rows, np.ones((2, 32), np.float32), 5, "33 members"),        # a wrong row length
            (mm.set_cols, np.ones((1, 257), np.float32), 38, "256 members"),
        ]
        for fn, values, first, why in bad:
            with pytest.raises(dspfx.DspfxError) as e:
                fn(values, first)
            assert e.value.status == -1 and why in str(e.value), e.value
        with pytest.raises(dspfx.DspfxError):
            mm.fill(3)
        with pytest.raises(dspfx.DspfxError):
            mm.fill(0, 7)
        assert (bits(run(dspfx, torch_cuda, mm, x)) == bits(fresh)).all()
    finally:
        mm.close()


def test_the_divisor_follows_the_wired_count(dspfx, torch_cuda):
    """normalise = 1 on integers: the sum is exact, so the output is fl32(sum / link_divisor(w)) bit for bit, with w counted after
    a row store (listeners 2 .. 4 of the room of 33) and a column store (source 9 muted for everybody, -0.0 counting as unwired)."""
    mats = small_int_mats(59)
    x = integers(37, SMALL[-1], 60)
    rows = np.zeros((3, 33), np.float32)
    rows[0, :4] = 1.0                                    # w = 4
    rows[1, 20] = -2.0                                   # w = 1
    rows[2, :] = 0.0                                     # w = 0: +0.0
    mute = np.full((1, 33), -0.0, np.float32)
    mm = bank(dspfx, SMALL, 0, 37, True, mats)
    try:
        mm.set_rows(rows, 5 + 2)
        mm.set_cols(mute, 5 + 9)
        got = run(dspfx, torch_cuda, mm, x)
    finally:
        mm.close()
    mats[1][2:5, :] = rows
    mats[1][:, 9] = 0.0
    d, wired = X.divisors(mats, True)
    assert not wired[5 + 4] and d[5 + 2] == float(R.link_divisor(4)) and d[5 + 3] == float(R.link_divisor(1))
    want = (int_product(x, SMALL, mats) / d.astype(np.float32)[None, :]).astype(np.float32)
    want[:, ~wired] = 0.0
    assert (bits(got) == bits(want)).all()


def test_out_overlapping_the_block_is_refused(dspfx, torch_cuda):
    torch = torch_cuda
    n, nf = SMALL[-1], 37
    buf = torch.zeros(2 * nf * n, dtype=torch.float32, device="cuda")
    mm = bank(dspfx, SMALL, 0, nf, True)
    try:
        s = nf * n
        # in place; out's first element on the block's last; out's last element on the block's first
        for block, out in ((buf[:s], buf[:s]), (buf[:s], buf[s - 1:]), (buf[s - 1:], buf[:s])):
            with pytest.raises(dspfx.DspfxError) as e:
                mm.run(block, nf, out=out)
            assert e.value.status == -1 and "overlaps" in str(e.value)
        mm.run(buf[:nf * n], nf, out=buf[nf * n:])        # back to back is no overlap
        torch.cuda.synchronize()
    finally:
        mm.close()


def test_a_store_from_another_thread_is_seen_whole(dspfx, torch_cuda):
    """One store from a second thread while six runs are submitted: every run's output is the old matrix's result or the new
    one's, wholly, and a run submitted after the store returned sees the new one."""
    torch = torch_cuda
    mats = small_int_mats(61)
    new = small_int_mats(62)[2]
    x = integers(128, SMALL[-1], 63)
    dx = device_block(dspfx, torch, x, 0)
    old_bits = bits(int_product(x, SMALL, mats))
    new_bits = bits(int_product(x, SMALL, mats[:2] + [new]))
    mm = bank(dspfx, SMALL, 0, 128, False, mats)
    try:
        outs = [fresh_out(torch, x.size) for _ in range(7)]
        t = threading.Thread(target=lambda: mm.set_rows(new, 38))
        mm.run(dx, 128, out=outs[0])
        t.start()
        for o in outs[1:6]:
            mm.run(dx, 128, out=o)
        t.join()
        mm.run(dx, 128, out=outs[6])
        torch.cuda.synchronize()
        got = [bits(read_out(dspfx, o, 128, x.shape[1], 0)) for o in outs]
    finally:
        mm.close()
    assert (got[0] == old_bits).all() and (got[6] == new_bits).all()
    seen_new = False
    for g in got:
        is_new = (g == new_bits).all()
        assert is_new or (g == old_bits).all(), "a run saw half a store"
        assert is_new or not seen_new, "a later run went back to the old matrix"
        seen_new = seen_new or is_new


# ---- 6. the full size ----------------------------------------------------------------------------------------------------------

def test_full_size(dspfx, torch_cuda):
    """N = 2^20 in 4096 rooms of 256, 128 frames, tiled 256: a run takes no longer than the 2.667 ms a block lasts (the standing
    condition for every bank).  Everything else is printed, not asserted: nobody has measured it before.  Whoever runs this writes
    the printed values into DESIGN.md section 8 and the README sentence."""
    torch = torch_cuda
    n, size, nf, tile = 1 << 20, 256, 128, 256
    torch.manual_seed(7)
    dx = torch.rand(nf * n, dtype=torch.float32, device="cuda") * 2.0 - 0.75
    out = torch.empty_like(dx)
    ret = torch.empty_like(dx)
    mm = dspfx.MixMatrix(n, group_size=size, tile_channels=tile, max_frames=nf)
    mg = dspfx.MixGroups(n, group_size=size, tile_channels=tile, max_frames=nf)
    rows = np.random.default_rng(8).uniform(0.0, 10.0, (3, size)).astype(np.float32)
    rows[1, 5] = 0.0                                     # "A mutes B for themself"
    last = n - size
    try:
        mm.set_rows(rows, 0)
        mm.set_rows(rows, last + 100)

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

        ms = timed(lambda: mm.run(dx, nf, out=out))
        ms_ret = timed(lambda: mg.returns(dx, nf, out=ret))
        ms_copy = timed(lambda: out.copy_(dx))
        mm.run(dx, nf, out=out)
        torch.cuda.synchronize()
        # the first and the last room against float64 (tiled 256: room g is tile g, [128][256] back to back)
        for g, c0 in ((0, 0), (n // size - 1, 100)):
            xs = dx[g * nf * size:(g + 1) * nf * size].cpu().numpy().reshape(nf, size)
            got = out[g * nf * size:(g + 1) * nf * size].cpu().numpy().reshape(nf, size)
            m = X.mix_minus([0, size])[0]
            m[c0:c0 + 3, :] = rows
            ref, sabs, n_of = X.exact(xs, [0, size], [m])
            assert (np.abs(got.astype(np.float64) - ref) <= X.bound(sabs, n_of)).all()
    finally:
        mm.close()
        mg.close()
    flop = 2.0 * n * size * nf
    gib2 = 2.0 * 2 ** 30
    tf = flop / (ms * 1e-3) / 1e12
    bw = gib2 / (ms * 1e-3) / 1e12
    print(f"mixmatrix full size: {ms:.4f} ms per run | {tf:.1f} TFLOP/s = {tf / 157.3:.3f} of 157.3 | {bw:.2f} TB/s on 2 GiB = "
          f"{bw / 8.0:.3f} of 8 TB/s | x {ms / ms_ret:.2f} of MixGroups.returns ({ms_ret:.4f} ms) | x {ms / ms_copy:.2f} of a flat "
          f"torch copy ({ms_copy:.4f} ms)")
    assert ms <= 128.0 / 48000.0 * 1e3, f"{ms:.4f} ms per run, and a block lasts 2.667 ms"
