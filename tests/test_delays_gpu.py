"""The channel-delay bank on the GPU (dspfx_delays_*, through the Python class): per-channel Reverb sliders and rings.  Parity
and the edge values are against the oracle's Reverb (oracle.chain_run per channel), bit for bit; everything about forms, frame
counts, stores and threads is checked bit for bit too, with delays_ref (which tests/test_delays_cpu.py holds to the oracle bit
for bit) where a reference is needed.  One exception, the project's own (tests/edge_values.py): where the reference gives a NaN
the bank must give a NaN, its sign and payload are not compared -- x86 and the GPU make them differently."""
import threading

import numpy as np
import pytest

import delays_ref as R
import edge_values as E
import oracle as O

pytestmark = pytest.mark.gpu

NF = 128
SHAPES = [(64, 0), (256, 64), (70, 0), (1, 0)]                   # vector lanes; tiled; scalar accesses and a ragged last workgroup; one channel
TWO = [(256, 64), (70, 0)]
MAXS = 0.02                                                      # a ring of 960 frames per channel


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Setup:
    """channel c carries pattern c mod len(lengths) of `lengths` (0: no node); decays random in [-1, 1] with one +1, one -1, one 0"""

    def __init__(self, dspfx, n, seed, lengths=None, page_round=False):
        rng = np.random.default_rng(seed)
        lengths = R.PATTERN_LENGTHS if lengths is None else lengths
        self.n, self.page_round = n, page_round
        self.D = np.asarray([lengths[c % len(lengths)] for c in range(n)], np.uint32)
        self.sec = np.asarray([(d - 0.5) / 48000.0 if page_round else (d + 0.5) / 48000.0 for d in self.D], np.float32)
        for c in np.flatnonzero(self.D):
            assert dspfx.delay_len(self.sec[c], page_round) == self.D[c]
        self.dec = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        for c, v in zip(np.flatnonzero(self.D)[:3], (1.0, -1.0, 0.0)):
            self.dec[c] = v

    def store(self, bank):
        """the same stores into a ChannelDelays or a delays_ref.Delays: every run of present channels as one range"""
        c = 0
        while c < self.n:
            if not self.D[c]:
                c += 1
                continue
            e = c
            while e < self.n and self.D[e]:
                e += 1
            bank.set_delay(self.sec[c:e], self.dec[c:e], first_channel=c)
            c = e

    def oracle(self, x, flags):
        """[frames][n] through the oracle, channel by channel, 128-frame blocks"""
        out = np.empty_like(x)
        for c in range(self.n):
            out[:, c] = R.oracle_channel(O, x[:, c], int(self.D[c]), self.dec[c], flags, self.page_round)
        return out

    def ref(self, max_seconds, flags):
        r = R.Delays(self.n, max_seconds, flags, self.page_round)
        self.store(r)
        return r


def device(dspfx, torch, x, tile):
    return torch.from_numpy(dspfx.to_layout(x, tile).reshape(-1).copy()).cuda()


def host(dspfx, t, nf, n, tile):
    return dspfx.from_layout(t.cpu().numpy(), nf, n, tile)


def run_blocks(dspfx, torch, bank, x, n, tile, nf=NF, inplace=False):
    outs = []
    for f0 in range(0, x.shape[0], nf):
        blk = x[f0:f0 + nf]
        dx = device(dspfx, torch, blk, tile)
        dy = bank.run(dx, len(blk), out=dx if inplace else torch.full_like(dx, float("nan")))
        torch.cuda.synchronize()
        outs.append(host(dspfx, dy, len(blk), n, tile))
    return np.concatenate(outs)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("n,tile", SHAPES)
def test_parity_with_the_oracle(dspfx, torch_cuda, n, tile, flags):
    """12 blocks of 128: every ring wraps, and for the odd lengths the zero taps run out in mid-block"""
    su = Setup(dspfx, n, 1000 + flags)
    x = R.noise(np.random.default_rng(n), 12 * NF, n)
    bank = dspfx.ChannelDelays(n, MAXS, tile_channels=tile, max_frames=NF, link_flags=flags)
    fresh = run_blocks(dspfx, torch_cuda, bank, x[:NF], n, tile)
    assert np.array_equal(bits(fresh), bits(x[:NF])), "a fresh bank copies in to out bit for bit"
    su.store(bank)
    assert np.array_equal(bank.lengths(), su.D) and np.array_equal(bank.present(), (su.D != 0).astype(np.uint32))
    got = run_blocks(dspfx, torch_cuda, bank, x, n, tile)
    bank.close()
    ref = su.oracle(x, flags)
    bad = bits(got) != bits(ref)
    print(f"delays parity N={n} tile={tile} link_flags={flags}: {int(bad.sum())} of {bad.size} samples differ")
    assert np.isfinite(got).all()
    assert not bad.any(), np.argwhere(bad)[0]


@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("n,tile", TWO)
def test_parity_with_the_oracle_page_rounded(dspfx, torch_cuda, n, tile, flags):
    su = Setup(dspfx, n, 1100 + flags, lengths=[0, 1024, 2048], page_round=True)
    x = R.noise(np.random.default_rng(n + 1), 12 * NF, n)
    assert dspfx.delays_plan(n, 0.03, True) == (2048, n * 2048 * 4)
    bank = dspfx.ChannelDelays(n, 0.03, tile_channels=tile, max_frames=NF, link_flags=flags, page_round=True)
    su.store(bank)
    assert np.array_equal(bank.lengths(), su.D)
    got = run_blocks(dspfx, torch_cuda, bank, x, n, tile)
    bank.close()
    ref = su.oracle(x, flags)
    bad = bits(got) != bits(ref)
    assert not bad.any(), np.argwhere(bad)[0]


# ---- 2. the same bits across forms ----------------------------------------------------------------------------------------
def test_same_bits_across_forms(dspfx, torch_cuda):
    torch = torch_cuda
    n, flags = 256, 3
    su = Setup(dspfx, n, 21)
    x = R.noise(np.random.default_rng(22), 9 * NF, n)
    base = su.ref(MAXS, flags).run_blocks(x)
    for name, tile, inplace in [("frame-major", 0, False), ("tiled", 64, False), ("in place", 64, True), ("in place frame-major", 0, True)]:
        bank = dspfx.ChannelDelays(n, MAXS, tile_channels=tile, max_frames=NF, link_flags=flags)
        su.store(bank)
        o = run_blocks(dspfx, torch, bank, x, n, tile, NF, inplace)
        bank.close()
        assert np.array_equal(bits(o), bits(base)), name
    # a channel alone in a bank of one, and the scalar-access kernel (N = 70 is no multiple of 4)
    for c in (4, 171):
        bank = dspfx.ChannelDelays(1, MAXS, max_frames=NF, link_flags=flags)
        bank.set_delay(su.sec[c], su.dec[c])
        o = run_blocks(dspfx, torch, bank, x[:, c:c + 1], 1, 0)
        bank.close()
        assert np.array_equal(bits(o[:, 0]), bits(base[:, c])), c
    m = 70
    bank = dspfx.ChannelDelays(m, MAXS, max_frames=NF, link_flags=flags)
    sub = Setup(dspfx, m, 21)
    sub.dec = su.dec[:m]
    sub.store(bank)
    o = run_blocks(dspfx, torch, bank, x[:, :m], m, 0)
    bank.close()
    assert np.array_equal(bits(o), bits(base[:, :m])), "scalar accesses"


# ---- 3. odd frame counts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf,runs", [(1, 200), (37, 30)])
@pytest.mark.parametrize("n,tile", TWO)
def test_odd_frame_counts(dspfx, torch_cuda, n, tile, nf, runs):
    """n_frames = 1 and 37 again and again: ring positions off every alignment, the rings of 128 .. 300 wrap (all of them at 37)"""
    flags = 3
    su = Setup(dspfx, n, 31)
    x = R.noise(np.random.default_rng(32), runs * nf, n)
    bank = dspfx.ChannelDelays(n, MAXS, tile_channels=tile, max_frames=NF, link_flags=flags)
    su.store(bank)
    got = run_blocks(dspfx, torch_cuda, bank, x, n, tile, nf)
    bank.close()
    assert np.array_equal(bits(got), bits(su.ref(MAXS, flags).run_blocks(x, nf)))


@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("n,tile", TWO)
def test_more_frames_than_the_ring_holds(dspfx, torch_cuda, n, tile, flags):
    """max_frames = 256; after three runs of 128 a run of 161: the channels with rings of 128, 129 and 160 are copied (behind
    their hop) and their rings stay as they were, which the next run of 128 shows; 300 and 960 are processed, in two chunks"""
    su = Setup(dspfx, n, 33)
    x = R.noise(np.random.default_rng(34), 384 + 161 + 128, n)
    bank = dspfx.ChannelDelays(n, MAXS, tile_channels=tile, max_frames=256, link_flags=flags)
    ref = su.ref(MAXS, flags)
    su.store(bank)
    cuts = [(0, 384, 128), (384, 545, 161), (545, 673, 128)]
    got = [run_blocks(dspfx, torch_cuda, bank, x[a:b], n, tile, nf) for a, b, nf in cuts]
    want = [ref.run_blocks(x[a:b], nf) for a, b, nf in cuts]
    bank.close()
    for g, w in zip(got, want):
        assert np.array_equal(bits(g), bits(w))
    short = (su.D != 0) & (su.D < 161)
    if flags == 0:
        assert np.array_equal(bits(got[1][:, short]), bits(x[384:545, short])), "n_frames > D: out = in"
    wrapped = su.D == 300                                        # (a ring of 960 still gives its zero taps at frame 545)
    assert (bits(got[1][:, wrapped]) != bits(x[384:545, wrapped])).any(axis=0).all(), "n_frames <= D: the ring is heard"
    # the rings of the short channels: a twin that never saw the 161 frames gives the same last block
    twin = su.ref(MAXS, flags)
    twin.run_blocks(x[0:384])
    assert np.array_equal(bits(got[2][:, short]), bits(twin.run(x[545:673])[:, short])), "n_frames > D: ring and position untouched"


# ---- 4. store semantics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", TWO)
def test_store_semantics(dspfx, torch_cuda, n, tile):
    torch = torch_cuda
    flags = 0
    su = Setup(dspfx, n, 41, lengths=[300, 129, 160, 960])       # a node everywhere
    rng = np.random.default_rng(42)
    x = R.noise(rng, 6 * NF, n)
    lo, hi = n // 4, n // 4 + max(1, n // 8)                     # the stored channels: a range inside a workgroup
    rest = np.r_[0:lo, hi:n]
    bank, ref = dspfx.ChannelDelays(n, MAXS, tile_channels=tile, max_frames=NF, link_flags=flags), su.ref(MAXS, flags)
    su.store(bank)
    base = su.ref(MAXS, flags).run_blocks(x)                     # no further store at all

    def both(call):
        return call(bank), call(ref)

    def step(a, b, why):
        g = run_blocks(dspfx, torch, bank, x[a * NF:b * NF], n, tile)
        assert np.array_equal(bits(g), bits(ref.run_blocks(x[a * NF:b * NF]))), why
        return g

    g = step(0, 3, "before any further store")
    assert np.array_equal(bits(g), bits(base[:3 * NF]))
    # decay alone: the stored channels start from a zero ring (the tail is cut), their seconds kept; the others go on
    both(lambda b: b.set_delay(decay=0.25, first_channel=lo, count=hi - lo))
    assert np.array_equal(bank.lengths(), su.D), "an omitted slider keeps its value"
    g = step(3, 4, "a store of decay alone")
    assert np.array_equal(bits(g[:, rest]), bits(base[3 * NF:4 * NF, rest])), "a store zeroes only the stored channels' rings"
    assert np.array_equal(bits(g[:, lo:hi]), bits(x[3 * NF:4 * NF, lo:hi])), "decay alone cuts the tail: 128 frames of zero taps"
    # seconds alone: the decay of the store before is kept
    both(lambda b: b.set_delay(seconds=np.float32(200.5 / 48000), first_channel=lo, count=hi - lo))
    assert (bank.lengths(lo, hi - lo) == 200).all()
    step(4, 6, "a store of seconds alone")
    # a drop makes the channel a copy; a later store starts from a zero ring and from the default sliders
    both(lambda b: b.set_delay(None, first_channel=lo, count=1))
    assert bank.present(lo, 1)[0] == 0 and bank.lengths(lo, 1)[0] == 0 and bank.present().sum() == n - 1
    g = step(0, 1, "a drop")
    assert np.array_equal(bits(g[:, lo]), bits(x[:NF, lo]))
    both(lambda b: b.set_delay(seconds=np.float32(150.5 / 48000), first_channel=lo, count=1))
    g = step(1, 3, "a store after a drop")
    # refusals change nothing: D above the ring, a range past the channels, an omitted seconds that is the default 0.5
    before = bank.lengths()
    for call in (lambda: bank.set_delay(0.5, 0.1, first_channel=lo, count=2), lambda: bank.set_delay(0.01, 0.1, first_channel=n - 1, count=2),
                 lambda: bank.set_delay(None, first_channel=n, count=1),
                 lambda: bank.set_delay(np.asarray([0.01, 0.021], np.float32), 0.3, first_channel=0)):
        with pytest.raises(dspfx.DspfxError) as e:
            call()
        assert e.value.status == -1 and "delays" in str(e.value)
    assert np.array_equal(bank.lengths(), before)
    step(3, 4, "refused stores leave the outputs unchanged")
    # reset: every ring back to zeros, the sliders kept
    bank.reset()
    ref.reset()
    assert np.array_equal(bank.lengths(), before)
    step(4, 6, "reset")
    bank.close()


def test_stream_order_across_two_streams(dspfx, torch_cuda):
    """runs alternate between two streams with nothing between them: each is ordered after the one before"""
    torch = torch_cuda
    n, tile, flags = 256, 64, 0
    su = Setup(dspfx, n, 45)
    x = R.noise(np.random.default_rng(46), 8 * NF, n)
    bank = dspfx.ChannelDelays(n, MAXS, tile_channels=tile, max_frames=NF, link_flags=flags)
    su.store(bank)
    dxs = [device(dspfx, torch, x[i * NF:(i + 1) * NF], tile) for i in range(8)]
    dys = [torch.empty_like(d) for d in dxs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i in range(8):
        bank.run(dxs[i], NF, out=dys[i], stream=streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    got = np.concatenate([host(dspfx, d, NF, n, tile) for d in dys])
    bank.close()
    assert np.array_equal(bits(got), bits(su.ref(MAXS, flags).run_blocks(x)))


# ---- 5. edge values -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("n,tile", TWO)
def test_edge_values_equal_the_oracle(dspfx, torch_cuda, n, tile, flags):
    """-0.0 samples under decays +1 and -1 while the taps are still zeros (-0.0 + +0.0 * -1.0), decays of inf (+0.0 * inf) and NaN,
    subnormal samples: the oracle's bits; NaN for NaN"""
    rng = np.random.default_rng(51)
    decs = [1.0, -1.0, np.inf, -np.inf, np.nan, 0.5, -0.75]
    lens = [128, 129, 300]
    su = Setup(dspfx, n, 52, lengths=lens)
    su.dec = np.asarray([decs[(c // len(lens)) % len(decs)] for c in range(n)], np.float32)
    x = R.noise(rng, 4 * NF, n)
    kind = np.arange(n) // (len(lens) * len(decs)) % 3
    x[:, kind == 0] = np.float32(-0.0)                           # silence of negative zeros, then a burst, then zeros again
    x[200:210, kind == 0] = R.noise(rng, 10, n)[:, kind == 0]
    sub = (rng.integers(1, 1 << 23, x.shape).astype(np.uint32) | (rng.integers(0, 2, x.shape).astype(np.uint32) << 31)).view(np.float32)
    x[:, kind == 1] = sub[:, kind == 1]                          # subnormals of both signs
    x[::7, kind == 2] = np.float32(-0.0)                         # noise with negative zeros in it
    bank = dspfx.ChannelDelays(n, MAXS, tile_channels=tile, max_frames=NF, link_flags=flags)
    su.store(bank)
    got = run_blocks(dspfx, torch_cuda, bank, x, n, tile)
    bank.close()
    ref = su.oracle(x, flags)
    assert np.isnan(ref).any() and E.is_subnormal(ref).any()
    assert flags or (bits(ref) == 0x80000000).any()             # (behind a hop, 0.0 + -0.0, there is no negative zero left)
    E.same_bits_or_nan(got, ref, None, f"delays edge values N={n} tile={tile} link_flags={flags}")


# ---- 6. isolation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", TWO)
def test_a_nan_and_a_huge_channel_change_no_other_channel(dspfx, torch_cuda, n, tile):
    flags = 3
    su = Setup(dspfx, n, 61, lengths=[128, 129, 160, 300, 960])
    x = R.noise(np.random.default_rng(62), 4 * NF, n)
    bad = x.copy()
    v_nan, v_big = n // 2 + 1, n // 2 + 2
    bad[:, v_nan] = np.nan
    bad[:, v_big] = np.float32(1e38)
    su.dec[v_big] = 1.0                                          # 1e38 doubles into infinity on the ring's first return
    outs = []
    for data in (x, bad):
        bank = dspfx.ChannelDelays(n, MAXS, tile_channels=tile, max_frames=NF, link_flags=flags)
        su.store(bank)
        outs.append(run_blocks(dspfx, torch_cuda, bank, data, n, tile))
        bank.close()
    others = (np.arange(n) != v_nan) & (np.arange(n) != v_big)
    assert np.array_equal(bits(outs[0][:, others]), bits(outs[1][:, others]))
    assert np.isnan(outs[1][:, v_nan]).all() and np.isinf(outs[1][-1, v_big])


# ---- 7. against what it generalises ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("n,tile", TWO)
def test_a_uniform_bank_equals_the_engine(dspfx, torch_cuda, n, tile, flags):
    torch = torch_cuda
    seconds, decay = float(np.float32(300.5 / 48000)), 0.4
    x = R.noise(np.random.default_rng(70), 6 * NF, n)
    bank = dspfx.ChannelDelays(n, MAXS, tile_channels=tile, max_frames=NF, link_flags=flags)
    bank.set_delay(seconds, decay)
    assert (bank.lengths() == 300).all()
    got = run_blocks(dspfx, torch, bank, x, n, tile)
    bank.close()
    eng = dspfx.Engine(n, NF, link_flags=flags, tile_channels=tile)
    eng.set_chain([dspfx.Reverb(seconds, decay)])
    outs = []
    for f0 in range(0, len(x), NF):
        dx = device(dspfx, torch, x[f0:f0 + NF], tile)
        dy = torch.empty_like(dx)
        eng.process(dx, out=dy, n_frames=NF)
        torch.cuda.synchronize()
        outs.append(host(dspfx, dy, NF, n, tile))
    eng.close()
    assert np.array_equal(bits(got), bits(np.concatenate(outs)))


# ---- 8. threads -----------------------------------------------------------------------------------------------------------
def test_stores_from_a_second_thread(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile, flags = 256, 64, 3
    rng = np.random.default_rng(80)
    x = R.noise(rng, NF, n)
    dx = device(dspfx, torch, x, tile)
    dy = torch.empty_like(dx)
    bank = dspfx.ChannelDelays(n, MAXS, tile_channels=tile, max_frames=NF, link_flags=flags)
    ref = R.Delays(n, MAXS, flags)
    bank.set_delay(0.01, 0.5)
    ref.set_delay(0.01, 0.5)
    sim = R.Delays(n, MAXS, flags)                               # only to keep refused stores out of the list
    sim.set_delay(0.01, 0.5)
    calls = []
    for i in range(200):
        first, count = int(rng.integers(0, n)), int(rng.integers(1, 40))
        count = min(count, n - first)
        sec = (rng.integers(128, 961, count) + 0.5).astype(np.float32) / np.float32(48000)
        dec = rng.uniform(-1.0, 1.0, count).astype(np.float32)
        kind = i % 10
        s, d = (None, None) if kind == 9 else (sec, None) if kind == 8 else (None, dec) if kind == 7 else (sec, dec)
        if not sim.set_delay(s, d, first_channel=first, count=count):      # decay alone on a dropped channel: the default 0.5 s
            s, d = sec, dec
            assert sim.set_delay(s, d, first_channel=first, count=count)
        calls.append((s, d, first, count))
    errors = []

    def storer():
        try:
            for s, d, first, count in calls:
                bank.set_delay(s, d, first_channel=first, count=count)
        except Exception as e:                                   # noqa: BLE001
            errors.append(e)

    t = threading.Thread(target=storer)
    t.start()
    for _ in range(50):
        bank.run(dx, NF, out=dy)
    t.join()
    assert not errors, errors
    for s, d, first, count in calls:
        assert ref.set_delay(s, d, first_channel=first, count=count)
    assert np.array_equal(bank.present(), ref.present()) and np.array_equal(bank.lengths(), ref.lengths())
    bank.reset()
    ref.reset()
    outs = []
    for _ in range(3):
        bank.run(dx, NF, out=dy)
        torch.cuda.synchronize()
        outs.append(host(dspfx, dy, NF, n, tile))
    bank.close()
    assert np.array_equal(bits(np.concatenate(outs)), bits(np.concatenate([ref.run(x) for _ in range(3)])))


# ---- 9. full size ---------------------------------------------------------------------------------------------------------
def test_full_size(dspfx, torch_cuda):
    """2^20 channels x 128 frames, tiled 256, rings of 960 frames (3.75 GiB), every channel present with a length drawn from
    128 .. 960, two alternating buffer pairs, device events, median of 20 after 10 warm-ups (1280 frames: every ring has wrapped,
    no tap is a still-zero one).  Asserted: one run fits the 2.667 ms a 128-frame block lasts at 48 kHz.  Printed in the same
    run: the time, the fraction of 8 TB/s on four block-units (block in, block out, ring in, ring out), and the ratios to a flat
    copy of the same bytes and to Engine([Reverb]) on the same buffers."""
    torch = torch_cuda
    n, nf, tile = 1 << 20, 128, 256
    rng = np.random.default_rng(91)
    eng = dspfx.Engine(n, nf, link_flags=0, tile_channels=tile)
    eng.set_chain([dspfx.Reverb(0.01, 0.5)])
    assert eng.kernels_ready()
    xs = [torch.empty(nf * n, dtype=torch.float32, device="cuda") for _ in range(2)]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    for i, x in enumerate(xs):
        eng.fill_noise(x, nf, 1000 * i)

    def timed(fn):
        for i in range(10):
            fn(i)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(21)]
        torch.cuda.synchronize()
        ev[0].record()
        for i in range(20):
            fn(i)
            ev[i + 1].record()
        torch.cuda.synchronize()
        return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(20)]))

    assert dspfx.delays_plan(n, MAXS) == (960, 3840 << 20)
    bank = dspfx.ChannelDelays(n, MAXS, tile_channels=tile, max_frames=nf)
    D = rng.integers(128, 961, n).astype(np.uint32)
    bank.set_delay((D + np.float32(0.5)) / np.float32(48000), rng.uniform(-0.9, 0.9, n).astype(np.float32))
    assert np.array_equal(bank.lengths(), D)
    t_bank = timed(lambda i: bank.run(xs[i % 2], nf, out=ys[i % 2]))
    torch.cuda.synchronize()
    assert torch.isfinite(ys[1][:1 << 16]).all() and not torch.equal(ys[1][:1 << 16], xs[1][:1 << 16])
    bank.close()
    t_eng = timed(lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=nf))
    eng.close()
    torch.cuda.empty_cache()
    a, b = torch.cat(xs), torch.empty(2 * nf * n, dtype=torch.float32, device="cuda")      # two block-units in, two out
    t_copy = timed(lambda i: b.copy_(a))
    own = 4 * nf * n * 4
    print(f"full size delays: {t_bank:.4f} ms ({own / t_bank / 1e9 / 8.0:.3f} of 8 TB/s on {own / 2**20:.0f} MiB), "
          f"x flat copy of the same bytes {t_bank / t_copy:.3f} (copy {t_copy:.4f} ms), x Engine([Reverb]) {t_bank / t_eng:.3f} (engine {t_eng:.4f} ms)")
    assert t_bank <= 2.667, t_bank
