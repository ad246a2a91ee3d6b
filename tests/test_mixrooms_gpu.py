"""The mix-group bank in mapped mode on the GPU (dspfx_mixgroups_assign, through the C ABI): a room id per channel, reseated
live.  Accuracy is checked against the float64 restatement (mixrooms_ref) inside the documented bound with the depth
dspfx_mixgroups_room_plan reports -- no measured constant; the order's independence of everything but the room's member set is
checked bit for bit."""
import threading

import numpy as np
import pytest

import mixrooms_ref as M

pytestmark = pytest.mark.gpu

NO = M.NO_ROOM
G5 = 5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def data(nf, n, seed):
    """amplitudes spread over 1e-3 .. 1 per channel"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1.0, 1.0, (nf, n)) * 10.0 ** rng.uniform(-3.0, 0.0, n)[None, :]).astype(np.float32)


def half_faders(n, seed=9):
    """(first channel, values): faders on the first half of the channels"""
    return 0, np.random.default_rng(seed).uniform(0.0, 4.0, n // 2).astype(np.float32)


def gain_vector(n, faders):
    g = np.ones(n, np.float32)
    if faders is not None:
        g[faders[0]:faders[0] + len(faders[1])] = faders[1]
    return g


def contiguous(n, groups):
    return (np.arange(n, dtype=np.int64) * groups // n).astype(np.uint32)


def table_of(n, groups):
    """the create table whose ranges are contiguous(n, groups)"""
    return np.searchsorted(contiguous(n, groups), np.arange(groups + 1), side="left").astype(np.uint64)


class Bank:
    """A bank of `groups` rooms with the create table of contiguous(n, groups) and faders on half the channels"""

    def __init__(self, dspfx, torch, n, tile, nf, groups=G5, normalise=True, faders=True):
        self.dspfx, self.torch, self.n, self.tile, self.nf, self.groups = dspfx, torch, n, tile, nf, groups
        self.mg = dspfx.MixGroups(n, group_start=table_of(n, groups), tile_channels=tile, max_frames=nf, normalise=normalise)
        self.faders = half_faders(n) if faders else None
        if faders:
            self.mg.set_gains(self.faders[1], first_channel=self.faders[0])
        self.gain = gain_vector(n, self.faders) if faders else None

    def device(self, x):
        return self.torch.from_numpy(self.dspfx.to_layout(x, self.tile).reshape(-1).copy()).cuda()

    def outputs(self, x):
        """-> (bus by run, returns, returns in place, buses by returns(buses=)) on the host, frame-major"""
        torch, mg, nf, n = self.torch, self.mg, x.shape[0], self.n
        dx = self.device(x)
        bus = mg.run(dx, nf)
        ret = mg.returns(dx, nf, out=torch.full_like(dx, float("nan")))
        b2 = torch.full((nf, self.groups), float("nan"), dtype=torch.float32, device="cuda")
        inp = dx.clone()
        assert mg.returns(inp, nf, out=inp, buses=b2) is inp
        torch.cuda.synchronize()
        back = lambda t: self.dspfx.from_layout(t.cpu().numpy(), nf, n, self.tile)  # noqa: E731
        return bus.cpu().numpy(), back(ret), back(inp), b2.cpu().numpy()

    def close(self):
        self.mg.close()


def check_bound(dspfx, x, room, groups, tile, gain, outs, what, normalise=True):
    bus, ret, inp, b2 = outs
    count, depth, pieces = dspfx.mixgroups_room_plan(room, groups, tile)
    ref, sabs = M.buses(x, room, groups, gain, normalise)
    bb = M.bus_bound(sabs, ref, depth)
    rref, rsabs = M.returns_exact(x, room, groups, gain, normalise)
    rb = M.returns_bound(rsabs, rref, depth, room)
    e_bus = np.abs(bus.astype(np.float64) - ref)
    e_ret = np.abs(ret.astype(np.float64) - rref)
    print(f"{what}: pieces {int(pieces.sum())}, max depth {int(depth.max())}, worst bus err / bound {float((e_bus / bb).max()):.3f}, "
          f"returns {float((e_ret / rb).max()):.3f}")
    assert np.isfinite(bus).all() and np.isfinite(ret).all(), what
    assert (e_bus <= bb).all(), (what, np.argwhere(e_bus > bb)[:5])
    assert (e_ret <= rb).all(), (what, np.argwhere(e_ret > rb)[:5])
    assert np.array_equal(bits(inp), bits(ret)), (what, "in place")
    assert np.array_equal(bits(b2), bits(bus)), (what, "buses= is what run writes")
    empty = np.flatnonzero(count == 0)
    assert (bits(bus[:, empty]) == 0).all(), (what, "an empty room gives +0.0")
    r = np.asarray(room, np.int64)
    silent = (r == NO) | (np.append(count, 0)[np.where(r == NO, groups, r)] == 1)
    assert (bits(ret[:, silent]) == 0).all(), (what, "unseated channels and rooms of one get +0.0")


SHAPES = [(1024, 256), (1000, 0)]
FRAMES = [1, 7, 128]


def seating(name, n, groups=G5):
    room = contiguous(n, groups)
    if name == "modulo":
        room = (np.arange(n) % groups).astype(np.uint32)
    elif name == "swap":                                     # two channels of different rooms, in different spans
        a, b = 3, n - 300
        assert room[a] != room[b] and a // 256 != b // 256
        room[a], room[b] = room[b], room[a]
    elif name == "scattered":                                # room 4 = 40 members scattered inside span 1, its others join room 3
        room[room == 4] = 3
        room[np.random.default_rng(4).choice(np.arange(256, 512), 40, replace=False)] = 4
    elif name == "empty":
        room[room == 2] = 1
    return room


@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("name", ["contiguous", "modulo", "swap", "scattered", "empty"])
@pytest.mark.parametrize("n,tile", SHAPES)
def test_seatings_stay_inside_the_bound(dspfx, torch_cuda, n, tile, name, nf):
    x = data(nf, n, 100 + nf)
    room = seating(name, n)
    for normalise in (True, False):
        b = Bank(dspfx, torch_cuda, n, tile, nf, normalise=normalise)
        try:
            b.mg.assign(room)
            assert np.array_equal(b.mg.room_of(), room) and np.array_equal(b.mg.counts(), M.counts(room, G5))
            assert np.array_equal(b.mg.depth(), dspfx.mixgroups_room_plan(room, G5, tile)[1])
            check_bound(dspfx, x, room, G5, tile, b.gain, b.outputs(x), f"n {n} tile {tile} {name} nf {nf} normalise {normalise}", normalise)
        finally:
            b.close()


@pytest.mark.parametrize("nf", [7, 128])
def test_rooms_of_one(dspfx, torch_cuda, nf):
    n, tile = 1024, 256
    x = data(nf, n, 5)
    b = Bank(dspfx, torch_cuda, n, tile, nf, groups=n)
    try:
        room = np.random.default_rng(6).permutation(n).astype(np.uint32)
        b.mg.assign(room)
        outs = b.outputs(x)
        check_bound(dspfx, x, room, n, tile, b.gain, outs, f"rooms of one nf {nf}")
        t = M.terms(x, b.gain)
        want = np.zeros_like(t)
        want[:, room] = (t / M.link_divisor(1)).astype(np.float32)
        assert np.array_equal(bits(outs[0]), bits(want)), "the bus of a room of one is t / divisor(1)"
        assert (bits(outs[1]) == 0).all()
    finally:
        b.close()


@pytest.mark.parametrize("n,tile", SHAPES)
def test_unseated_channels_reach_nothing(dspfx, torch_cuda, n, tile):
    nf = 7
    x = data(nf, n, 7)
    room = seating("modulo", n)
    out = [5, 300, 301, n - 1, 700]
    room[out] = NO
    x[:, 300] = np.nan
    x[:, n - 1] = np.inf
    x[3, 5] = -np.inf
    b = Bank(dspfx, torch_cuda, n, tile, nf)
    try:
        b.mg.assign(room)
        bus, ret, inp, b2 = b.outputs(x)
        assert np.isfinite(bus).all() and np.isfinite(ret).all()
        assert (bits(ret[:, out]) == 0).all(), "an unseated channel's return is +0.0 whatever it carries"
        clean = x.copy()
        clean[:, out] = 0.0
        check_bound(dspfx, clean, room, G5, tile, b.gain, (bus, ret, inp, b2), f"unseated n {n}")
    finally:
        b.close()


def test_second_reduce_round(dspfx, torch_cuda):
    """N = 32 768: room 0 holds exactly one channel of every span, 128 pieces of one member: two reduce rounds"""
    n, tile, nf = 32768, 256, 7
    x = data(nf, n, 8)
    room = contiguous(n, G5)
    room[room == 0] = 1
    room[np.arange(0, n, 256) + (np.arange(n // 256) * 37) % 256] = 0
    assert dspfx.mixgroups_room_plan(room, G5, tile)[2][0] == 128
    b = Bank(dspfx, torch_cuda, n, tile, nf)
    try:
        b.mg.assign(room)
        check_bound(dspfx, x, room, G5, tile, b.gain, b.outputs(x), "one member per span")
    finally:
        b.close()


# ---- bit for bit ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,tile", SHAPES)
def test_a_room_depends_on_its_member_set_alone(dspfx, torch_cuda, n, tile):
    """Two maps that share one room's member set, under different ids and with everything else different: that room's bus and
    returns are the same bits.  And permuted ids give permuted buses."""
    nf = 7
    x = data(nf, n, 11)
    rng = np.random.default_rng(12)
    mine = np.sort(rng.choice(n, 150, replace=False))
    a = seating("modulo", n)
    a[a == 2] = 3
    a[mine] = 2
    c = rng.integers(1, G5, n).astype(np.uint32)
    c[rng.choice(n, 100, replace=False)] = NO
    c[c == 0] = 1
    c[mine] = 0
    perm = np.asarray([3, 0, 4, 1, 2], np.uint32)
    p = np.where(a == NO, a, perm[np.minimum(a, G5 - 1)]).astype(np.uint32)
    outs = []
    for room in (a, c, p):
        b = Bank(dspfx, torch_cuda, n, tile, nf)
        try:
            b.mg.assign(room)
            outs.append(b.outputs(x))
        finally:
            b.close()
    assert np.array_equal(bits(outs[0][0][:, 2]), bits(outs[1][0][:, 0]))
    assert np.array_equal(bits(outs[0][1][:, mine]), bits(outs[1][1][:, mine]))
    assert np.array_equal(bits(outs[2][0][:, perm]), bits(outs[0][0])), "the same sets under other numbers"
    assert np.array_equal(bits(outs[2][1]), bits(outs[0][1]))


def test_one_assign_or_three_overlapping_ones_twice_and_on_two_streams(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile, nf = 1024, 256, 7
    x = data(nf, n, 13)
    room = seating("scattered", n)
    room[[1, 2, 900]] = NO
    one = Bank(dspfx, torch, n, tile, nf)
    three = Bank(dspfx, torch, n, tile, nf)
    try:
        one.mg.assign(room)
        three.mg.assign(np.full(600, 1, np.uint32), first_channel=100)
        three.mg.assign(room[:500])
        three.mg.assign(room[400:], first_channel=400)
        assert np.array_equal(three.mg.room_of(), room)
        o1, o3 = one.outputs(x), three.outputs(x)
        for u, v in zip(o1, o3):
            assert np.array_equal(bits(u), bits(v))
        again = one.outputs(x)
        for u, v in zip(o1, again):
            assert np.array_equal(bits(u), bits(v))
        dx = one.device(x)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        got = [(one.mg.run(dx, nf, stream=streams[i % 2].cuda_stream), one.mg.returns(dx, nf, stream=streams[(i + 1) % 2].cuda_stream))
               for i in range(4)]
        torch.cuda.synchronize()
        for bus, ret in got:
            assert np.array_equal(bits(bus.cpu().numpy()), bits(o1[0]))
            assert np.array_equal(bits(dspfx.from_layout(ret.cpu().numpy(), nf, n, tile)), bits(o1[1]))
    finally:
        one.close()
        three.close()


def test_edge_values_inside_a_seated_room(dspfx, torch_cuda):
    n, tile, nf = 1024, 256, 7
    x = data(nf, n, 14)
    room = seating("modulo", n)
    x[:, 5] = np.inf                                         # room 0
    x[:, 6 + 512] = np.nan                                   # room 3
    b = Bank(dspfx, torch_cuda, n, tile, nf, faders=False)
    try:
        b.mg.assign(room)
        bus, ret, _, _ = b.outputs(x)
    finally:
        b.close()
    r0 = np.flatnonzero(room == 0)
    assert np.isnan(ret[:, 5]).all() and (ret[:, r0[r0 != 5]] == np.inf).all()
    assert np.isnan(ret[:, room == 3]).all() and np.isnan(bus[:, 3]).all() and (bus[:, 0] == np.inf).all()
    assert np.isfinite(bus[:, [1, 2, 4]]).all() and np.isfinite(ret[:, (room != 0) & (room != 3)]).all()


def test_bad_assigns_change_nothing(dspfx, torch_cuda):
    n, tile, nf = 1024, 256, 7
    x = data(nf, n, 15)
    b = Bank(dspfx, torch_cuda, n, tile, nf)
    try:
        room = seating("swap", n)
        b.mg.assign(room)
        before = b.outputs(x)
        for ids, first, word in (([0, 1, G5], 10, "room 5"), (np.zeros(10, np.uint32), n - 9, "not inside"), ([0], n, "not inside")):
            with pytest.raises(dspfx.DspfxError) as e:
                b.mg.assign(ids, first_channel=first)
            assert e.value.status == -1 and word in str(e.value), str(e.value)
            assert np.array_equal(b.mg.room_of(), room)
        for u, v in zip(before, b.outputs(x)):
            assert np.array_equal(bits(u), bits(v))
    finally:
        b.close()
    fresh = Bank(dspfx, torch_cuda, n, tile, nf)                # a refused first assign leaves the bank without a map
    try:
        plain = fresh.outputs(x)
        with pytest.raises(dspfx.DspfxError):
            fresh.mg.assign([G5])
        assert np.array_equal(fresh.mg.room_of(), contiguous(n, G5))
        for u, v in zip(plain, fresh.outputs(x)):
            assert np.array_equal(bits(u), bits(v))
    finally:
        fresh.close()


def test_assign_from_a_second_thread_while_blocks_are_submitted(dspfx, torch_cuda):
    """64 blocks of one known input; a second thread reseats once meanwhile.  Every block is the old or the new seating's
    output, bit for bit, and once it is the new one it stays the new one."""
    torch = torch_cuda
    n, tile, nf, blocks = 1024, 256, 128, 64
    x = data(nf, n, 16)
    old, new = seating("contiguous", n), seating("modulo", n)
    b = Bank(dspfx, torch, n, tile, nf)
    try:
        want = {}
        for name, room in (("old", old), ("new", new)):
            b.mg.assign(room)
            want[name] = b.outputs(x)
        b.mg.assign(old)
        dx = b.device(x)
        buses = torch.empty((blocks, nf, G5), dtype=torch.float32, device="cuda")
        rets = torch.empty((blocks, nf * n), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        started = threading.Event()
        errors = []

        def reseat():
            try:
                started.wait()
                b.mg.assign(new)
            except Exception as e:                               # noqa: BLE001
                errors.append(e)

        th = threading.Thread(target=reseat)
        th.start()
        for i in range(blocks):
            b.mg.returns(dx, nf, out=rets[i], buses=buses[i])
            if i == 8:
                started.set()
        th.join()
        last = b.outputs(x)
        torch.cuda.synchronize()
        assert not errors, errors
        hb, hr = buses.cpu().numpy(), rets.cpu().numpy()
        state = []
        for i in range(blocks):
            ret = dspfx.from_layout(hr[i], nf, n, tile)
            is_old = np.array_equal(bits(hb[i]), bits(want["old"][0])) and np.array_equal(bits(ret), bits(want["old"][1]))
            is_new = np.array_equal(bits(hb[i]), bits(want["new"][0])) and np.array_equal(bits(ret), bits(want["new"][1]))
            assert is_old != is_new, i
            state.append(is_new)
        assert state == sorted(state), "once the output is the new seating's it never goes back"
        assert not state[0]
        assert np.array_equal(b.mg.room_of(), new)
        for u, v in zip(last, want["new"]):
            assert np.array_equal(bits(u), bits(v))
    finally:
        b.close()


# ---- full size -----------------------------------------------------------------------------------------------------------------

def test_full_size(dspfx, torch_cuda):
    """2^20 channels x 128 frames, 4096 rooms of 256, tiled 256, two alternating buffer pairs, device events, median of 20 after
    5 warm-ups.  Timed in the same test: the unmapped bank's run and the Gain chain on the same buffers.  For the contiguous
    seating and for movers (one channel in 64 swapped with a channel of another room): t_run_mapped <= t_gain, the condition
    test_mixgroups_gpu.py::test_full_size puts on run, and t_returns_mapped <= t_run_unmapped + 2 t_gain, the existing returns
    condition with the unmapped run as the term.  The random seating is printed and not asserted."""
    torch = torch_cuda
    n, nf, tile, G = 1 << 20, 128, 256, 4096
    table = np.arange(0, n + 1, 256, dtype=np.uint64)
    eng = dspfx.Engine(n, nf, link_flags=0, tile_channels=tile)
    eng.set_chain([dspfx.Gain(1.0)])
    assert eng.kernels_ready()
    xs = [torch.empty(nf * n, dtype=torch.float32, device="cuda") for _ in range(2)]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    for i, x in enumerate(xs):
        eng.fill_noise(x, nf, 1000 * i)
    buses = torch.empty((nf, G), dtype=torch.float32, device="cuda")

    def timed(fn):
        for i in range(5):
            fn(i)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(21)]
        torch.cuda.synchronize()
        ev[0].record()
        for i in range(20):
            fn(i)
            ev[i + 1].record()
        torch.cuda.synchronize()
        return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(20)]))

    rng = np.random.default_rng(71)
    cont = (np.arange(n) // 256).astype(np.uint32)
    movers = cont.copy()
    pick = np.arange(0, n, 64) + rng.integers(0, 64, n // 64)
    partner = np.roll(pick, 7)                                   # a channel 7 * 64 on: another room
    movers[pick], movers[partner] = cont[partner], cont[pick]
    assert (movers[pick] != cont[pick]).all()
    seatings = {"contiguous": cont, "movers": movers, "random": rng.permutation(cont)}

    plain = dspfx.MixGroups(n, group_start=table, tile_channels=tile, max_frames=nf)
    t_gain = timed(lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=nf))
    t_plain = timed(lambda i: plain.run(xs[i % 2], nf, out=buses))
    blk = nf * n * 4
    print(f"full size: Gain chain {t_gain:.4f} ms ({2 * blk / t_gain / 1e9 / 8.0:.3f} of 8 TB/s), unmapped run {t_plain:.4f} ms "
          f"({blk / t_plain / 1e9 / 8.0:.3f})")
    plain.close()
    results = {}
    for name, room in seatings.items():
        mg = dspfx.MixGroups(n, group_start=table, tile_channels=tile, max_frames=nf)
        mg.assign(room)
        pieces = mg.pieces()
        t_run = timed(lambda i: mg.run(xs[i % 2], nf, out=buses))
        if name == "contiguous":                                 # the sums themselves, on a sample of rooms, inside the bound
            torch.cuda.synchronize()
            got = buses.cpu().numpy()
            xt = xs[1].view(n // tile, nf, tile)
            for g in (0, 1, 2047, 4095):
                t = xt[g].cpu().numpy().astype(np.float64)
                ref = t.sum(axis=1) / float(M.link_divisor(256))
                bound = M.bound(np.abs(t).sum(axis=1) / float(M.link_divisor(256)), ref, 8)
                assert (np.abs(got[:, g] - ref) <= bound).all(), g
        t_ret = timed(lambda i: mg.returns(xs[i % 2], nf, out=ys[i % 2]))
        mg.close()
        results[name] = (t_run, t_ret)
        print(f"full size {name}: pieces {pieces}, run {t_run:.4f} ms ({blk / t_run / 1e9 / 8.0:.3f} of 8 TB/s, {t_run / t_plain:.3f} x unmapped), "
              f"returns {t_ret:.4f} ms ({3 * blk / t_ret / 1e9 / 8.0:.3f} of 8 TB/s, returns / (unmapped run + 2 gain) = "
              f"{t_ret / (t_plain + 2 * t_gain):.3f})")
    eng.close()
    for name in ("contiguous", "movers"):
        t_run, t_ret = results[name]
        assert t_run <= t_gain, (name, t_run, t_gain)
        assert t_ret <= t_plain + 2 * t_gain, (name, t_ret, t_plain, t_gain)
