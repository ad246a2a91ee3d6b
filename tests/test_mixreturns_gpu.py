"""The mix-group bank's per-channel returns on the GPU (dspfx_mixgroups_returns, through the C ABI).  The kernel is compared
bit for bit with the definition (mixreturns_ref.returns_bits) evaluated in numpy float32 from the raw sums that a second bank
with the same table, layout and normalise = 0 writes as its bus; and against the float64 sum of the others inside
mixgroups_ref.bound with the depth dspfx_mixgroups_plan reports plus one (the subtraction): no measured constant."""
import numpy as np
import pytest

import mixgroups_ref as R
import mixreturns_ref as M
import resample_ref
from test_mixgroups_gpu import bits, dc_heavy, ragged, run_bank

pytestmark = pytest.mark.gpu

B = 128


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def noise(nf, n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (nf, n)).astype(np.float32)


def faders(n, seed=3):
    return np.random.default_rng(seed).uniform(0.0, 10.0, n).astype(np.float32)


def run_returns(dspfx, torch, x, table, tile, gain=None, normalise=True, want_buses=False, in_place=False):
    """x [F][N] f32 (frame-major, host) -> (returns [F][N] f32 frame-major on the host, buses [F][G] or None)"""
    nf, n = x.shape
    mg = dspfx.MixGroups(n, group_start=table, tile_channels=tile, max_frames=nf, normalise=normalise)
    try:
        if gain is not None:
            mg.set_gains(gain)
        dx = torch.from_numpy(dspfx.to_layout(x, tile).reshape(-1).copy()).cuda()
        out = dx if in_place else torch.full_like(dx, float("nan"))
        buses = torch.full((nf, mg.groups), float("nan"), dtype=torch.float32, device="cuda") if want_buses else None
        got = mg.returns(dx, nf, out=out, buses=buses)
        assert got is out
        torch.cuda.synchronize()
        return dspfx.from_layout(out.cpu().numpy(), nf, n, tile), None if buses is None else buses.cpu().numpy()
    finally:
        mg.close()


def expected_bits(dspfx, torch, x, table, tile, gain=None, normalise=True):
    """the definition from the raw sums of a second bank with normalise = 0"""
    S_raw = run_bank(dspfx, torch, x, table, tile, gain, normalise=False)
    return M.returns_bits(S_raw, x, table, gain, normalise)


def check_bits(dspfx, torch, x, table, tile, gain, what):
    for normalise in (True, False):
        got, _ = run_returns(dspfx, torch, x, table, tile, gain, normalise)
        want = expected_bits(dspfx, torch, x, table, tile, gain, normalise)
        bad = np.argwhere(bits(got) != bits(want))
        assert len(bad) == 0, (what, normalise, len(bad), bad[:5])


def tables(n, tile):
    return {"uniform": np.arange(0, n + 1, 256, dtype=np.uint64), "ragged": ragged(n, tile)}


# ---- 1. bit-exact against the definition -------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_gain", [False, True], ids=["nogain", "gain"])
@pytest.mark.parametrize("nf", [1, 16, 17, 128])
@pytest.mark.parametrize("table", ["uniform", "ragged"])
@pytest.mark.parametrize("tile", [0, 256])
def test_bit_exact_against_the_definition(dspfx, torch_cuda, tile, table, nf, with_gain):
    n = 8192
    x = noise(nf, n, nf) + np.float32(0.25)
    check_bits(dspfx, torch_cuda, x, tables(n, tile)[table], tile, faders(n) if with_gain else None,
               f"tile {tile} {table} nf {nf} gain {with_gain}")


@pytest.mark.parametrize("n,tile,table,nf", [
    (1000, 0, [0, 333, 1000], 37),                    # a last span cut by N, rows that are no multiple of a span
    (1001, 0, [0, 333, 1001], 37),                    # N not a multiple of 4: the scalar loads and stores
    (4096, 64, [0, 64, 100, 4096], 37),               # tiles narrower than a span
    (4096, 0, list(range(4097)), 37),                 # N groups of one: all +0.0
    (4096, 0, list(range(0, 4097, 8)), 37),           # every span cut 32 times
    (1 << 17, 256, [0, 1 << 17], 16),                 # one group of N: two reduce levels
], ids=["n1000", "n1001", "tile64", "ones", "uniform8", "one_group"])
def test_bit_exact_shapes(dspfx, torch_cuda, n, tile, table, nf):
    x = noise(nf, n, n) + np.float32(0.25)
    for gain in (None, faders(n, 4)):
        check_bits(dspfx, torch_cuda, x, table, tile, gain, f"n {n} tile {tile} G {len(table) - 1}")
    if len(table) == n + 1:
        got, _ = run_returns(dspfx, torch_cuda, x, table, tile, None)
        assert (bits(got) == 0).all(), "groups of one give +0.0"


# ---- 2. accuracy against float64 ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_gain", [False, True], ids=["nogain", "gain"])
@pytest.mark.parametrize("family", ["noise", "dc_heavy"])
@pytest.mark.parametrize("nf", [17, 128])
@pytest.mark.parametrize("table", ["uniform", "ragged"])
@pytest.mark.parametrize("tile", [0, 256])
def test_accuracy_against_float64(dspfx, torch_cuda, tile, table, nf, family, with_gain):
    n = 8192
    x = noise(nf, n, 7 * nf) if family == "noise" else dc_heavy(nf, n, nf)
    t = tables(n, tile)[table]
    gain = faders(n) if with_gain else None
    got, _ = run_returns(dspfx, torch_cuda, x, t, tile, gain)
    depth = dspfx.mixgroups_plan(n, group_start=t, tile_channels=tile).astype(np.float64)
    ref, sabs = M.returns_exact(x, t, gain)
    bound = M.bound(sabs, ref, depth[M.group_of(t, n)][None, :] + 1.0)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / bound).max())
    print(f"tile {tile} {table} nf {nf} {family} gain {with_gain}: worst err / bound = {worst:.3f}")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), (worst, np.argwhere(err > bound)[:5])


# ---- 3. exact on integers ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [0, 256])
def test_exact_on_integers(dspfx, torch_cuda, tile):
    """Integer samples and integer faders, every |partial sum| <= 8192 * 64 * 4 < 2^24: all sums and the subtraction are exact
    in f32, so with normalise = 0 a return is the integer sum of the others."""
    n, nf = 8192, 37
    rng = np.random.default_rng(11)
    x = rng.integers(-64, 65, (nf, n)).astype(np.float32)
    gain = rng.integers(1, 5, n).astype(np.float32)
    for table in (np.arange(0, n + 1, 256, dtype=np.uint64), ragged(n, tile), np.asarray([0, n], np.uint64)):
        want, _ = M.returns_exact(x, table, gain, normalise=False)
        assert np.abs(want).max() < 2 ** 24 and (want == np.round(want)).all()
        got, _ = run_returns(dspfx, torch_cuda, x, table, tile, gain, normalise=False)
        assert np.array_equal(got.astype(np.float64), want)


# ---- 4. groups of one and empty groups -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [0, 256])
def test_groups_of_one_give_plus_zero_and_empty_groups_nothing(dspfx, torch_cuda, tile):
    n, nf = 2048, 17
    table = [0, 0, 1, 2, 2, 2, 130, 131, 131, 256, 257, 600, 600, 1023, 1024, 1025, n - 1, n, n]
    sizes = np.diff(np.asarray(table))
    single = np.flatnonzero(sizes[M.group_of(table, n)] == 1)
    assert len(single) == 7 and (sizes == 0).sum() == 6
    x = noise(nf, n, 41)
    clean = x.copy()
    x[:, single[0::3]] = np.nan
    x[:, single[1::3]] = np.inf
    x[:, single[2::3]] = -np.inf
    others = np.setdiff1d(np.arange(n), single)
    for gain in (None, faders(n, 42)):
        got, _ = run_returns(dspfx, torch_cuda, x, table, tile, gain)
        assert (bits(got[:, single]) == 0).all(), "a group of one returns +0.0 whatever the sample is"
        want = expected_bits(dspfx, torch_cuda, clean, table, tile, gain)
        assert np.array_equal(bits(got[:, others]), bits(want[:, others])), "the neighbours are unaffected"
        assert np.isfinite(got).all()


# ---- 5. buses, 6. in place -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalise", [True, False])
@pytest.mark.parametrize("tile", [0, 256])
def test_buses_output_is_runs_and_leaves_the_returns_alone(dspfx, torch_cuda, tile, normalise):
    n, nf = 8192, 37
    x = noise(nf, n, 51)
    gain = faders(n, 52)
    for table in (ragged(n, tile), [0, n], list(range(0, n + 1, 256))):
        ret, buses = run_returns(dspfx, torch_cuda, x, table, tile, gain, normalise, want_buses=True)
        assert np.array_equal(bits(buses), bits(run_bank(dspfx, torch_cuda, x, table, tile, gain, normalise)))
        alone, none = run_returns(dspfx, torch_cuda, x, table, tile, gain, normalise)
        assert none is None and np.array_equal(bits(ret), bits(alone))


@pytest.mark.parametrize("n,tile", [(8192, 0), (8192, 256), (1001, 0)])
def test_in_place_gives_the_same_bits(dspfx, torch_cuda, n, tile):
    nf = 37
    x = noise(nf, n, 61)
    table = ragged(n, tile) if n == 8192 else [0, 333, n]
    for gain in (None, faders(n, 62)):
        out, _ = run_returns(dspfx, torch_cuda, x, table, tile, gain)
        inp, _ = run_returns(dspfx, torch_cuda, x, table, tile, gain, in_place=True)
        assert np.array_equal(bits(out), bits(inp))


# ---- 7. independence of the neighbours, 8. repeatability ---------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [0, 256])
def test_a_rooms_returns_do_not_depend_on_its_neighbours(dspfx, torch_cuda, tile):
    n, nf = 8192, 37
    x = noise(nf, n, 21)
    gain = faders(n, 22)
    for a, b in ((1000, 5000), (256, 512), (300, 310), (2047, 6145)):
        big = [0, a, b, n]
        small = sorted(set(list(range(0, a, 7)) + [a, b] + list(range(b, n, 13)) + [n]))
        one, _ = run_returns(dspfx, torch_cuda, x, big, tile, gain)
        many, _ = run_returns(dspfx, torch_cuda, x, small, tile, gain)
        assert np.array_equal(bits(one[:, a:b]), bits(many[:, a:b])), (a, b)


def test_repeated_calls_on_two_streams_are_bit_identical(dspfx, torch_cuda):
    torch = torch_cuda
    n, nf, tile = 1 << 14, 64, 256
    table = R.ragged_table(n, 5, 1 << 12)
    mg = dspfx.MixGroups(n, group_start=table, tile_channels=tile, max_frames=nf)
    mg.set_gains(np.random.default_rng(1).uniform(0.0, 4.0, n).astype(np.float32))
    x = torch.from_numpy(noise(1, nf * n, 2).reshape(-1)).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    rets, buses = [], []
    for i in range(12):
        s = streams[i % 2].cuda_stream
        rets.append(mg.returns(x, nf, stream=s))
        buses.append(mg.run(x, nf, stream=streams[(i + 1) % 2].cuda_stream))
    torch.cuda.synchronize()
    first, bus0 = rets[0].cpu().numpy(), buses[0].cpu().numpy()
    assert np.isfinite(first).all()
    for r, b in zip(rets[1:], buses[1:]):
        assert np.array_equal(bits(r.cpu().numpy()), bits(first))
        assert np.array_equal(bits(b.cpu().numpy()), bits(bus0))
    xh = dspfx.from_layout(x.cpu().numpy(), nf, n, tile)
    gain = np.random.default_rng(1).uniform(0.0, 4.0, n).astype(np.float32)
    assert np.array_equal(bits(dspfx.from_layout(first, nf, n, tile)), bits(expected_bits(dspfx, torch, xh, table, tile, gain)))
    mg.close()


# ---- 9. fader stores -----------------------------------------------------------------------------------------------------------

def test_a_store_between_two_calls_changes_exactly_the_second(dspfx, torch_cuda):
    torch = torch_cuda
    n, nf = 4096, 37
    table = ragged(n, 0)
    xh = noise(nf, n, 31)
    x = torch.from_numpy(xh).cuda()
    g1 = faders(n, 32)
    g2 = g1.copy()
    g2[100:200] *= 2
    mg = dspfx.MixGroups(n, group_start=table, max_frames=nf)
    plain = mg.returns(x, nf)
    mg.set_gains(g1)
    faded = mg.returns(x, nf)
    mg.set_gains(g2[100:200], first_channel=100)
    part = mg.returns(x, nf)
    mg.set_gains(None)
    back = mg.returns(x, nf)
    torch.cuda.synchronize()
    plain, faded, part, back = (t.cpu().numpy().reshape(nf, n) for t in (plain, faded, part, back))
    mg.close()
    # each call matches the definition with the table of its own time, in the sum AND in the own term
    assert np.array_equal(bits(plain), bits(expected_bits(dspfx, torch, xh, table, 0, None)))
    assert np.array_equal(bits(faded), bits(expected_bits(dspfx, torch, xh, table, 0, g1)))
    assert np.array_equal(bits(part), bits(expected_bits(dspfx, torch, xh, table, 0, g2)))
    assert np.array_equal(bits(back), bits(plain))
    assert not np.array_equal(bits(plain), bits(faded)) and not np.array_equal(bits(faded), bits(part))


# ---- 10. rooms without a host copy ---------------------------------------------------------------------------------------------

def test_returns_go_straight_into_a_resampler_slot(dspfx, torch_cuda):
    """Engine(N) chain -> returns straight into Resampler(N, 44100).slot_tensor() -> push -> pull, device to device: the pull is
    resample_ref applied to the bit-exact returns (the definition from a normalise = 0 bank's sums of what the chain wrote)."""
    torch = torch_cuda
    n, tile, blocks = 512, 256, 3
    table = np.arange(0, n + 1, 64, dtype=np.uint64)
    eng = dspfx.Engine(n, B, link_flags=3, tile_channels=tile)
    eng.set_chain([dspfx.BiQuad(1.0, -1.8, 0.81, 0.0025, 0.005, 0.0025), dspfx.Gain(0.5)])
    rooms = dspfx.MixGroups(n, group_start=table, tile_channels=tile, max_frames=B)
    fader = faders(n, 51) / np.float32(5.0)
    rooms.set_gains(fader)
    listeners = dspfx.Resampler(n, 44100, tile_channels=tile, slots=4)
    ref_rs = resample_ref.Resampler(n, 44100)
    x = torch.empty(B * n, dtype=torch.float32, device="cuda")
    y = torch.empty_like(x)
    fifo = np.zeros((0, n), np.float32)
    for b in range(blocks):
        eng.fill_noise(x, B, b * B)
        eng.process(x, out=y, n_frames=B)
        slot = listeners.slot_tensor()
        assert rooms.returns(y, B, out=slot) is slot
        listeners.push(slot)
        out, used, under = listeners.pull(100)
        torch.cuda.synchronize()
        yh = dspfx.from_layout(y.cpu().numpy(), B, n, tile)
        want_ret = expected_bits(dspfx, torch, yh, table, tile, fader)
        assert np.array_equal(bits(dspfx.from_layout(slot.cpu().numpy(), B, n, tile)), bits(want_ret))
        fifo = np.concatenate([fifo, want_ret])
        want_out, want_used = ref_rs.callback(fifo, 100)
        assert not under and used == want_used
        fifo = fifo[want_used:]
        want_flat = dspfx.to_layout(np.ascontiguousarray(want_out), tile).reshape(-1)
        assert np.array_equal(out.cpu().numpy().view(np.uint8), np.ascontiguousarray(want_flat).view(np.uint8))
    for o in (listeners, rooms, eng):
        o.close()


# ---- 11. full size ---------------------------------------------------------------------------------------------------------------

def test_full_size(dspfx, torch_cuda):
    """2^20 channels x 128 frames, 4096 rooms of 256, tiled 256, two alternating buffer pairs (1 GiB a pair: nothing of a call's
    block is left in the 256 MiB Infinity Cache by the call before).  Sampled rooms bit for bit as in case 1; and, with device
    events, median of 20 after 5 warm-ups, t_returns <= t_run + 2 t_gain: the call moves run's read plus one read and one write
    of the block, which is the Gain chain's traffic, and the margin is a whole second t_gain.  A condition that catches an
    uncoalesced second pass or a search per element, not a target."""
    torch = torch_cuda
    n, nf, tile = 1 << 20, 128, 256
    table = np.arange(0, n + 1, 256, dtype=np.uint64)
    eng = dspfx.Engine(n, nf, link_flags=0, tile_channels=tile)
    eng.set_chain([dspfx.Gain(1.0)])
    assert eng.kernels_ready()
    xs = [torch.empty(nf * n, dtype=torch.float32, device="cuda") for _ in range(2)]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    for i, x in enumerate(xs):
        eng.fill_noise(x, nf, 1000 * i)
    gain = np.random.default_rng(61).uniform(0.0, 4.0, n).astype(np.float32)
    mg = dspfx.MixGroups(n, group_start=table, tile_channels=tile, max_frames=nf)
    raw = dspfx.MixGroups(n, group_start=table, tile_channels=tile, max_frames=nf, normalise=False)
    mg.set_gains(gain)
    raw.set_gains(gain)
    buses = torch.empty((nf, len(table) - 1), dtype=torch.float32, device="cuda")
    mg.returns(xs[0], nf, out=ys[0])
    S_raw = raw.run(xs[0], nf)
    torch.cuda.synchronize()
    sample = sorted(set(np.random.default_rng(62).choice(len(table) - 1, 24, replace=False).tolist() + [0, len(table) - 2]))
    xt = xs[0].view(n // tile, nf, tile)
    yt = ys[0].view(n // tile, nf, tile)
    S_h = S_raw.cpu().numpy()
    for g in sample:                                   # a room of 256 at tile 256 is one tile: [nf][256]
        xg, got = xt[g].cpu().numpy(), yt[g].cpu().numpy()
        want = M.returns_bits(S_h[:, g:g + 1], xg, [0, 256], gain[g * 256:(g + 1) * 256])
        assert np.array_equal(bits(got), bits(want)), g
    raw.close()

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

    t_gain = timed(lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=nf))
    t_run = timed(lambda i: mg.run(xs[i % 2], nf, out=buses))
    t_ret = timed(lambda i: mg.returns(xs[i % 2], nf, out=ys[i % 2]))
    blk = nf * n * 4
    print(f"full size: 4096 rooms of 256, run {t_run:.4f} ms ({blk / t_run / 1e9 / 8.0:.3f} of 8 TB/s), Gain chain {t_gain:.4f} ms "
          f"({2 * blk / t_gain / 1e9 / 8.0:.3f}), returns {t_ret:.4f} ms ({3 * blk / t_ret / 1e9 / 8.0:.3f}); "
          f"returns / (run + 2 gain) = {t_ret / (t_run + 2 * t_gain):.3f}")
    assert t_ret <= t_run + 2 * t_gain, (t_ret, t_run, t_gain)
    mg.close()
    eng.close()
