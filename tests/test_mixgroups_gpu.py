"""The mix-group bank on the GPU (dspfx_mixgroups_*, through the C ABI) against the float64 restatement in mixgroups_ref.py.
The bound of every accuracy check is mixgroups_ref.bound with the depth dspfx_mixgroups_plan reports for the group: it holds
for any summation order of that depth and contains no measured constant.  On exactly representable data the bus is compared
bit for bit."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import mixgroups_ref as R
import oracle as O
import resample_ref

pytestmark = pytest.mark.gpu

B = 128


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dc_heavy(frames, n, seed):
    """0.9 DC plus 1e-3 noise on every channel: the terms barely cancel, so the sum is as large as sum|t|"""
    rng = np.random.default_rng(seed)
    return (np.float32(0.9) + np.float32(1e-3) * rng.standard_normal((frames, n)).astype(np.float32)).astype(np.float32)


def ragged(n, tile):
    """cuts inside a wave (64), inside a span of 256 and inside a tile, single channels, an empty group, a long group"""
    t = [0, 1, 2, 40, 40, 100, 129, 300, 301, 1000, 1023, 1024, 1500, 2048, 2049, n - 700, n - 3, n]
    assert all(a <= b for a, b in zip(t, t[1:])) and (not tile or any(v % tile for v in t))
    return np.asarray(t, np.uint64)


def run_bank(dspfx, torch, x, table, tile, gain=None, normalise=True, max_frames=None, stream=0):
    """x [F][N] f32 (frame-major, host) -> buses [F][G] f32 (host) through the C ABI"""
    L = dspfx.lib()
    nf, n = x.shape
    t = np.ascontiguousarray(table, np.uint64)
    d = dspfx._MixGroupsDesc(dspfx.ABI_VERSION, 0, n, max_frames or nf, tile, len(t) - 1, int(normalise),
                             t.ctypes.data_as(C.POINTER(C.c_uint64)))
    h = C.c_void_p()
    rc = L.dspfx_mixgroups_create(C.byref(d), C.byref(h))
    assert rc == 0, (rc, L.dspfx_mixgroups_last_error(None))
    try:
        dx = torch.from_numpy(dspfx.to_layout(x, tile).reshape(-1).copy()).cuda()
        out = torch.full((nf, len(t) - 1), float("nan"), dtype=torch.float32, device="cuda")
        if gain is not None:
            g = np.ascontiguousarray(gain, np.float32)
            assert L.dspfx_mixgroups_set_gains(h, g.ctypes.data_as(C.POINTER(C.c_float)), 0, len(g)) == 0
        rc = L.dspfx_mixgroups_run(h, C.c_void_p(dx.data_ptr()), nf, C.c_void_p(out.data_ptr()), C.c_void_p(stream) if stream else None)
        assert rc == 0, (rc, L.dspfx_mixgroups_last_error(h))
        torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        assert L.dspfx_mixgroups_destroy(h) == 0


def check(dspfx, got, x, table, tile, gain, normalise=True, groups=None, what=""):
    depth = dspfx.mixgroups_plan(x.shape[1], group_start=table, tile_channels=tile)
    sizes = np.diff(np.asarray(table, np.int64))
    groups = list(range(len(sizes))) if groups is None else list(groups)
    for g in groups:
        assert depth[g] <= R.cap(sizes[g]), (g, sizes[g], depth[g])
    ref, sabs, _ = R.buses(x, table, gain, normalise, groups)
    bound = R.bound(sabs, ref, depth[groups][None, :].astype(np.float64))
    err = np.abs(got[:, groups].astype(np.float64) - ref)
    worst = float((err / bound).max())
    print(f"{what}: worst err / bound = {worst:.3f} over {len(groups)} groups, depth {int(depth[groups].min())}..{int(depth[groups].max())}")
    assert np.isfinite(got[:, groups]).all(), what
    assert (err <= bound).all(), (what, worst, np.argwhere(err > bound)[:5])
    for g in groups:
        if sizes[g] == 0:
            assert (bits(got[:, g]) == 0).all(), "an empty group gives +0.0"


# ---- accuracy -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_gain", [False, True], ids=["nogain", "gain"])
@pytest.mark.parametrize("family", ["noise", "dc"])
@pytest.mark.parametrize("nf", [1, 37, 128, 256])
@pytest.mark.parametrize("table", ["uniform", "ragged"])
@pytest.mark.parametrize("tile", [0, 256])
def test_accuracy(dspfx, torch_cuda, tile, table, nf, family, with_gain):
    torch = torch_cuda
    n = 8192
    if family == "noise":
        eng = dspfx.Engine(n, nf, tile_channels=0)
        dx = torch.empty((nf, n), dtype=torch.float32, device="cuda")
        eng.fill_noise(dx, nf, 1000)
        torch.cuda.synchronize()
        x = dx.cpu().numpy()
        eng.close()
    else:
        x = dc_heavy(nf, n, nf)
    t = np.arange(0, n + 1, 256, dtype=np.uint64) if table == "uniform" else ragged(n, tile)
    gain = np.random.default_rng(3).uniform(0.0, 10.0, n).astype(np.float32) if with_gain else None
    got = run_bank(dspfx, torch, x, t, tile, gain)
    check(dspfx, got, x, t, tile, gain, what=f"tile {tile} {table} nf {nf} {family} gain {with_gain}")


@pytest.mark.parametrize("n,tile,table", [
    (1000, 0, [0, 333, 1000]),                        # N not a multiple of 4: the scalar loads, and a last span cut by N
    (4096, 64, [0, 64, 100, 4096]),                   # tiles narrower than a span
    (4096, 0, list(range(4097))),                     # N groups of 1
    (1 << 17, 256, [0, 1 << 17]),                     # one group of N: two reduce levels
    (1 << 17, 0, [0, 5, (1 << 17) - 9, 1 << 17]),     # ... that begins and ends inside spans
])
def test_accuracy_shapes(dspfx, torch_cuda, n, tile, table):
    x = np.random.default_rng(n).uniform(-1.0, 1.0, (37, n)).astype(np.float32) + np.float32(0.25)
    gain = np.random.default_rng(4).uniform(0.0, 2.0, n).astype(np.float32)
    for g in (None, gain):
        got = run_bank(dspfx, torch_cuda, x, table, tile, g)
        check(dspfx, got, x, table, tile, g, what=f"n {n} tile {tile} G {len(table) - 1}")


# ---- exact cases -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [0, 256])
def test_exact_on_integers(dspfx, torch_cuda, tile):
    """Integer samples, power-of-two faders, |sum| < 2^24: every partial sum is exact in f32 whatever the order, so the bus
    is f32(exact sum) / div bit for bit, and the exact integer with normalise = 0."""
    n, nf = 8192, 37
    rng = np.random.default_rng(11)
    x = rng.integers(-64, 65, (nf, n)).astype(np.float32)
    gain = (2.0 ** rng.integers(-2, 3, n)).astype(np.float32)
    for table in (np.arange(0, n + 1, 256, dtype=np.uint64), ragged(n, tile), np.asarray([0, n], np.uint64)):
        sizes = np.diff(table.astype(np.int64))
        exact = np.stack([(x.astype(np.float64) * gain)[:, int(a):int(b)].sum(axis=1) for a, b in zip(table[:-1], table[1:])], axis=1)
        assert np.abs(exact).max() < 2 ** 24 and (exact * 4 == np.round(exact * 4)).all()
        raw = run_bank(dspfx, torch_cuda, x, table, tile, gain, normalise=False)
        assert np.array_equal(raw.astype(np.float64), exact)
        div = np.asarray([R.link_divisor(s) for s in sizes], np.float32)
        want = (exact.astype(np.float32) / div[None, :]).astype(np.float32)
        got = run_bank(dspfx, torch_cuda, x, table, tile, gain)
        assert np.array_equal(bits(got), bits(want))


# ---- group independence, repeatability ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [0, 256])
def test_a_groups_bus_does_not_depend_on_its_neighbours(dspfx, torch_cuda, tile):
    n, nf = 8192, 128
    x = np.random.default_rng(21).uniform(-1.0, 1.0, (nf, n)).astype(np.float32)
    gain = np.random.default_rng(22).uniform(0.0, 10.0, n).astype(np.float32)
    for a, b in ((1000, 5000), (256, 512), (300, 310), (2047, 6145)):
        big = [0, a, b, n]
        small = sorted(set(list(range(0, a, 7)) + [a, b] + list(range(b, n, 13)) + [n]))
        one = run_bank(dspfx, torch_cuda, x, big, tile, gain)[:, 1]
        many = run_bank(dspfx, torch_cuda, x, small, tile, gain)[:, small.index(a)]
        assert np.array_equal(bits(one), bits(many)), (a, b)


def test_repeated_runs_on_two_streams_are_bit_identical(dspfx, torch_cuda):
    torch = torch_cuda
    n, nf, tile = 1 << 16, 128, 256
    table = R.ragged_table(n, 5, 1 << 14)
    mg = dspfx.MixGroups(n, group_start=table, tile_channels=tile, max_frames=nf)
    mg.set_gains(np.random.default_rng(1).uniform(0.0, 4.0, n).astype(np.float32))
    x = torch.from_numpy(np.random.default_rng(2).uniform(-1.0, 1.0, nf * n).astype(np.float32)).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs = [mg.run(x, nf, stream=streams[i % 2].cuda_stream) for i in range(20)]
    torch.cuda.synchronize()
    first = outs[0].cpu().numpy()
    for o in outs[1:]:
        assert np.array_equal(bits(o.cpu().numpy()), bits(first))
    mg.close()


# ---- consistency with the engine's bus -----------------------------------------------------------------------------------------

def test_one_group_agrees_with_process_bus(dspfx, torch_cuda):
    torch = torch_cuda
    n, nf = 1 << 16, 128
    eng = dspfx.Engine(n, nf, link_flags=0, tile_channels=256)
    eng.set_chain([dspfx.Gain(1.0)])
    x = torch.empty(nf * n, dtype=torch.float32, device="cuda")
    y = torch.empty_like(x)
    mix = torch.empty(nf, dtype=torch.float32, device="cuda")
    eng.fill_noise(x, nf, 0)
    eng.process_bus(x, y, mix, nf, n_connected=n)
    mg = dspfx.MixGroups(n, group_start=[0, n], tile_channels=256, max_frames=nf)
    bus = mg.run(y, nf)
    torch.cuda.synchronize()
    xs = dspfx.from_layout(y.cpu().numpy(), nf, n, 256)
    ref, sabs, _ = R.buses(xs, [0, n])
    d = float(mg.depth()[0])
    # the engine's tree is another one of depth at most 64 + log2 n (include/dspfx.h): the sum of both bounds
    both = R.bound(sabs, ref, d) + R.bound(sabs, ref, R.cap(n))
    err = np.abs(bus.cpu().numpy().astype(np.float64)[:, 0] - mix.cpu().numpy().astype(np.float64))
    assert (err <= both[:, 0]).all(), (err / both[:, 0]).max()
    mg.close()
    eng.close()


# ---- fader stores ------------------------------------------------------------------------------------------------------------

def test_a_store_between_two_runs_changes_exactly_the_second(dspfx, torch_cuda):
    torch = torch_cuda
    n, nf = 4096, 128
    table = ragged(n, 0)
    xh = np.random.default_rng(31).uniform(-1.0, 1.0, (nf, n)).astype(np.float32)
    x = torch.from_numpy(xh).cuda()
    g1 = np.random.default_rng(32).uniform(0.0, 10.0, n).astype(np.float32)
    mg = dspfx.MixGroups(n, group_start=table, max_frames=nf)
    plain = mg.run(x, nf)
    mg.set_gains(g1)
    faded = mg.run(x, nf)
    mg.set_gains(g1[100:200] * 2, first_channel=100)
    part = mg.run(x, nf)
    mg.set_gains(None)
    back = mg.run(x, nf)
    torch.cuda.synchronize()
    plain, faded, part, back = (t.cpu().numpy() for t in (plain, faded, part, back))
    g2 = g1.copy()
    g2[100:200] *= 2
    check(dspfx, plain, xh, table, 0, None, what="before the store")
    check(dspfx, faded, xh, table, 0, g1, what="after the store")
    check(dspfx, part, xh, table, 0, g2, what="after the partial store")
    assert not np.array_equal(bits(plain), bits(faded))
    assert np.array_equal(bits(back), bits(plain)), "a NULL store restores the no-gain bits"
    assert np.array_equal(bits(faded), bits(run_bank(dspfx, torch, xh, table, 0, g1)))
    mg.close()


def test_stores_from_a_second_thread_while_runs_are_in_flight(dspfx, torch_cuda):
    """500 runs while another thread stores whole tables at 60 Hz: every run's buses are those of ONE of the stored tables
    (table k multiplies every channel by 2^k or 2^-k: exact), never a mixture, and the tables seen never go back."""
    torch = torch_cuda
    n, nf, runs = 1 << 14, 64, 500
    table = np.arange(0, n + 1, 1 << 10, dtype=np.uint64)
    rng = np.random.default_rng(41)
    xh = rng.integers(-8, 9, (nf, n)).astype(np.float32)
    x = torch.from_numpy(xh).cuda()
    mg = dspfx.MixGroups(n, group_start=table, max_frames=nf, normalise=False)
    levels = [np.float32(2.0 ** ((k % 9) - 4)) for k in range(1, 40)]
    base = run_bank(dspfx, torch, xh, table, 0, None, normalise=False)          # exact integers
    stop = threading.Event()
    stored = []

    def gui():
        for lv in levels:
            if stop.is_set():
                break
            mg.set_gains(np.full(n, lv, np.float32))
            stored.append(lv)
            time.sleep(1.0 / 60.0)

    th = threading.Thread(target=gui)
    outs = torch.empty((runs, nf, len(table) - 1), dtype=torch.float32, device="cuda")
    th.start()
    for i in range(runs):
        mg.run(x, nf, out=outs[i])
        if i % 10 == 9:
            time.sleep(0.002)
    stop.set()
    th.join()
    torch.cuda.synchronize()
    got = outs.cpu().numpy()
    seen = []
    candidates = [np.float32(1.0)] + stored
    for i in range(runs):
        k = [j for j, lv in enumerate(candidates) if np.array_equal(got[i], base * lv)]
        assert k, f"run {i} matches no stored table"
        # (levels repeat with period 9: take the first match not below the last one seen)
        later = [j for j in k if not seen or j >= seen[-1]]
        assert later, f"run {i} went back from table {seen[-1]} to {k}"
        seen.append(later[0])
    assert seen == sorted(seen)
    assert seen[-1] >= 1, "no store was seen at all"
    mg.close()


# ---- composition ---------------------------------------------------------------------------------------------------------------

def test_rooms_master_chain_resampler_without_a_host_copy(dspfx, torch_cuda):
    """Engine(N) chain -> MixGroups -> Engine(G, tile_channels=0) master chain -> Resampler(G, 44100), device to device; each
    stage checked with its own test's tolerance on what the stage before it really produced: the chains within 1 ulp of the
    oracle (test_gpu_parity), the buses within the restatement's bound, the resampler's bytes equal to its restatement."""
    torch = torch_cuda
    n, rooms, tile, blocks = 4096, 16, 256, 3
    table = np.arange(0, n + 1, n // rooms, dtype=np.uint64)
    chain = [dspfx.BiQuad(1.0, -1.8, 0.81, 0.0025, 0.005, 0.0025), dspfx.Gain(0.5)]
    master = [dspfx.LowPass(0.25), dspfx.Gain(2.0)]
    eng = dspfx.Engine(n, B, link_flags=3, tile_channels=tile)
    eng.set_chain(chain)
    meng = dspfx.Engine(rooms, B, link_flags=3, tile_channels=0)
    meng.set_chain(master)
    mg = dspfx.MixGroups(n, group_start=table, tile_channels=tile, max_frames=B)
    fader = np.random.default_rng(51).uniform(0.0, 2.0, n).astype(np.float32)
    mg.set_gains(fader)
    rs = dspfx.Resampler(rooms, 44100, slots=4)
    ref_rs = resample_ref.Resampler(rooms, 44100)
    x = torch.empty(B * n, dtype=torch.float32, device="cuda")
    y = torch.empty_like(x)
    buses = torch.empty((B, rooms), dtype=torch.float32, device="cuda")
    chans = [0, 1, 255, 256, 1000, n - 1]
    nodes_c, nodes_m = [], []
    fifo = np.zeros((0, rooms), np.float32)
    for b in range(blocks):
        eng.fill_noise(x, B, b * B)
        eng.process(x, out=y, n_frames=B)
        mg.run(y, B, out=buses)
        slot = rs.slot_tensor()
        meng.process(buses, out=slot, n_frames=B)
        rs.push(slot, B)
        out, used, under = rs.pull(100)
        torch.cuda.synchronize()
        xh = dspfx.from_layout(x.cpu().numpy(), B, n, tile)
        yh = dspfx.from_layout(y.cpu().numpy(), B, n, tile)
        want_y = O.run_channels([c.oracle_desc() for c in chain], xh[:, chans], 3, nodes_out=nodes_c)
        ulp = np.abs(yh[:, chans].view(np.int32).astype(np.int64) - want_y.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, ulp.max()
        bh = buses.cpu().numpy()
        check(dspfx, bh, yh, table, tile, fader, what=f"block {b} buses")
        mh = slot.cpu().numpy().reshape(B, rooms)
        want_m = O.run_channels([c.oracle_desc() for c in master], bh, 3, nodes_out=nodes_m)
        ulp = np.abs(mh.view(np.int32).astype(np.int64) - want_m.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, ulp.max()
        fifo = np.concatenate([fifo, mh])
        want_out, want_used = ref_rs.callback(fifo, 100)
        assert not under and used == want_used
        fifo = fifo[want_used:]
        assert np.array_equal(out.cpu().numpy().view(np.uint8), np.ascontiguousarray(want_out).reshape(-1).view(np.uint8))
    for o in (rs, mg, meng, eng):
        o.close()


# ---- full size -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["a", "b"])
def test_full_size(dspfx, torch_cuda, case):
    """2^20 channels, 128 frames, tile 256: (a) 4096 groups of 256, (b) a ragged table from a fixed seed, sizes 1 .. 2^18.
    Sampled groups against the restatement; and a run takes no longer than Engine.process of a [Gain(1.0)] chain on the same
    buffers (which reads AND writes the block: twice the bytes), 20 runs after 5 warm-ups on two alternating inputs."""
    torch = torch_cuda
    n, nf, tile = 1 << 20, 128, 256
    table = np.arange(0, n + 1, 256, dtype=np.uint64) if case == "a" else R.ragged_table(n, 20260101, 1 << 18)
    sizes = np.diff(table.astype(np.int64))
    assert sizes.min() >= 1 and sizes.max() <= 1 << 18 and (case == "a" or (sizes.max() > 1 << 16 and sizes.min() < 16))
    eng = dspfx.Engine(n, nf, link_flags=0, tile_channels=tile)
    eng.set_chain([dspfx.Gain(1.0)])
    assert eng.kernels_ready()
    xs = [torch.empty(nf * n, dtype=torch.float32, device="cuda") for _ in range(2)]
    y = torch.empty_like(xs[0])
    for i, x in enumerate(xs):
        eng.fill_noise(x, nf, 1000 * i)
    mg = dspfx.MixGroups(n, group_start=table, tile_channels=tile, max_frames=nf)
    mg.set_gains(np.random.default_rng(61).uniform(0.0, 4.0, n).astype(np.float32))
    buses = torch.empty((nf, len(sizes)), dtype=torch.float32, device="cuda")
    mg.run(xs[0], nf, out=buses)
    torch.cuda.synchronize()
    got = buses.cpu().numpy()
    order = np.argsort(sizes)
    sample = sorted(set(np.random.default_rng(62).choice(len(sizes), min(24, len(sizes)), replace=False).tolist()
                        + order[:3].tolist() + order[-3:].tolist() + [0, len(sizes) - 1]))
    xh = dspfx.from_layout(xs[0].cpu().numpy(), nf, n, tile)
    gain = np.random.default_rng(61).uniform(0.0, 4.0, n).astype(np.float32)
    check(dspfx, got, xh, table, tile, gain, groups=sample, what=f"full size ({case})")

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
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(20)]

    t_chain = timed(lambda i: eng.process(xs[i % 2], out=y, n_frames=nf))
    t_bank = timed(lambda i: mg.run(xs[i % 2], nf, out=buses))
    chain_ms = float(np.median(t_chain))
    bank_ms = float(np.median(t_bank))
    print(f"full size ({case}): {len(sizes)} groups, MixGroups {bank_ms:.4f} ms ({nf * n * 4 / bank_ms / 1e9 / 8.0:.3f} of 8 TB/s), "
          f"Gain chain {chain_ms:.4f} ms")
    assert bank_ms <= chain_ms, (bank_ms, chain_ms)
    mg.close()
    eng.close()
