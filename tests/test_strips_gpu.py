"""The channel-strip bank on the GPU (dspfx_strips_*, through the Python class): per-channel Gain and BiQuad sliders.  Parity is
against the oracle (oracle.chain_run on each channel's own present nodes) at the bar tests/test_gpu_parity.py holds the
engine's BiQuad to, 1 ulp; everything about forms, stores and isolation is checked bit for bit, with strips_ref (which
tests/test_strips_cpu.py holds to the oracle bit for bit) where a reference is needed."""
import threading

import numpy as np
import pytest

import oracle as O
import strips_ref as S

pytestmark = pytest.mark.gpu

NF = 128
SHAPES = [(64, 0), (256, 64), (70, 0), (1, 0)]                   # vector lanes; tiled; scalar lanes with a ragged last group; one channel


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ulps(a, b):
    return np.abs(bits(a).view(np.int32).astype(np.int64) - bits(b).view(np.int32).astype(np.int64))


class Setup:
    """masks, levels and raw sliders for n channels of K bands: channel c carries pattern c mod 5 (those that fit in K bands)"""

    def __init__(self, n, K, seed):
        rng = np.random.default_rng(seed)
        pats = S.patterns(K)
        self.n, self.K = n, K
        self.masks = np.asarray([pats[c % len(pats)] for c in range(n)], np.uint32)
        self.level = rng.uniform(0.0, 4.0, n).astype(np.float32)
        self.raw = np.stack([S.stable_raw6(rng, n) for _ in range(K)])       # [band][channel][6]

    def store(self, bank):
        """the same stores into a ChannelStrips or a strips_ref.Strips: runs of equal channels as ranges"""
        for c in range(self.n):
            if self.masks[c] & 1:
                bank.set_gain(self.level[c:c + 1], c)
            for b in range(self.K):
                if self.masks[c] & (1 << (1 + b)):
                    bank.set_band(b, self.raw[b, c:c + 1], c)

    def oracle(self, x, flags):
        """[frames][n] through the oracle, channel by channel, 128-frame blocks"""
        out = np.empty_like(x)
        for c in range(self.n):
            nodes = S.oracle_nodes(O, int(self.masks[c]), self.level[c], [self.raw[b, c] for b in range(self.K)])
            out[:, c] = O.chain_run(nodes, x[:, c], flags)
        return out


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
@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("n,tile", SHAPES)
def test_parity_with_the_oracle(dspfx, torch_cuda, n, tile, K, flags):
    su = Setup(n, K, 1000 + 10 * K + flags)
    x = S.noise(np.random.default_rng(n + K), 3 * NF, n)
    bank = dspfx.ChannelStrips(n, bands=K, tile_channels=tile, max_frames=NF, link_flags=flags)
    fresh = run_blocks(dspfx, torch_cuda, bank, x[:NF], n, tile)
    assert np.array_equal(bits(fresh), bits(x[:NF])), "a fresh bank copies in to out bit for bit"
    su.store(bank)
    assert np.array_equal(bank.present(), su.masks)
    got = run_blocks(dspfx, torch_cuda, bank, x, n, tile)
    bank.close()
    ref = su.oracle(x, flags)
    u = ulps(got, ref).max(axis=0)
    print(f"strips parity N={n} tile={tile} K={K} link_flags={flags}: worst {int(u.max())} ulp")
    assert np.isfinite(got).all()
    assert u.max() <= 1, (np.argmax(u), int(u.max()))
    plain = (su.masks & ~np.uint32(1)) == 0                      # no band: nodeless or Gain only
    assert u[plain].max(initial=0) == 0, "Gain-only and nodeless channels are 0 ulp"


# ---- 2. the same bits across forms ----------------------------------------------------------------------------------------
def test_same_bits_across_forms(dspfx, torch_cuda):
    torch = torch_cuda
    n, K, flags = 256, 3, 3
    su = Setup(n, K, 21)
    x = S.noise(np.random.default_rng(22), 2 * NF, n)
    outs = {}
    for name, tile, nf, inplace in [("frame-major", 0, NF, False), ("tiled", 64, NF, False), ("in place", 64, NF, True),
                                    ("in place frame-major", 0, NF, True), ("one call of 256", 64, 2 * NF, False),
                                    ("one call of 256 frame-major", 0, 2 * NF, False)]:
        bank = dspfx.ChannelStrips(n, bands=K, tile_channels=tile, max_frames=2 * NF, link_flags=flags)
        su.store(bank)
        outs[name] = run_blocks(dspfx, torch, bank, x, n, tile, nf, inplace)
        bank.close()
    base = outs.pop("frame-major")
    for name, o in outs.items():
        assert np.array_equal(bits(o), bits(base)), name
    # the scalar-lane kernel (N = 70 is no multiple of 4) gives its channels the same bits too
    m = 70
    sub = Setup(n, K, 21)
    sub.n, sub.masks, sub.level, sub.raw = m, su.masks[:m], su.level[:m], su.raw[:, :m]
    bank = dspfx.ChannelStrips(m, bands=K, max_frames=NF, link_flags=flags)
    sub.store(bank)
    o = run_blocks(dspfx, torch, bank, x[:, :m], m, 0)
    bank.close()
    assert np.array_equal(bits(o), bits(base[:, :m])), "one channel a lane"


@pytest.mark.parametrize("nf", [1, 37, 4, 8, 9])
@pytest.mark.parametrize("n,tile", [(256, 64), (70, 0)])
def test_odd_frame_counts(dspfx, torch_cuda, n, tile, nf):
    """n_frames = 1 and 37: whole chunks and the rows left over; 4, 8 and 9: the chunk loop's boundaries with 4 or 8 rows a chunk (one
    chunk and no row left, two chunks, chunks and one row); three calls, the state carried between them"""
    K, flags = 3, 3
    su = Setup(n, K, 31)
    x = S.noise(np.random.default_rng(32), 3 * nf, n)
    bank = dspfx.ChannelStrips(n, bands=K, tile_channels=tile, max_frames=NF, link_flags=flags)
    su.store(bank)
    got = run_blocks(dspfx, torch_cuda, bank, x, n, tile, nf)
    bank.close()
    ref = S.Strips(n, K, flags)
    su.store(ref)
    # the reference takes its hops per 128-frame block, but a hop is per sample: the block length changes nothing
    assert ulps(got, ref.run(x)).max() <= 1


# ---- 3. store semantics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", [(256, 64), (70, 0)])
def test_store_semantics(dspfx, torch_cuda, n, tile):
    torch = torch_cuda
    K, flags = 3, 0
    su = Setup(n, K, 41)
    su.masks[:] = (1 << (1 + K)) - 1                             # every node everywhere
    rng = np.random.default_rng(42)
    x = S.noise(rng, 3 * NF, n)
    new = S.stable_raw6(rng, n)
    lo, hi = n // 4, n // 4 + max(1, n // 8)                     # the stored channels: a range inside a wave

    def bank_and_ref():
        b, r = dspfx.ChannelStrips(n, bands=K, tile_channels=tile, max_frames=NF, link_flags=flags), S.Strips(n, K, flags)
        su.store(b)
        su.store(r)
        return b, r

    # no store at all: the baseline
    bank, _ = bank_and_ref()
    base = run_blocks(dspfx, torch, bank, x, n, tile)
    bank.close()
    # a band store between blocks 1 and 2
    bank, ref = bank_and_ref()
    g0 = run_blocks(dspfx, torch, bank, x[:NF], n, tile)
    r0 = ref.run(x[:NF])
    bank.set_band(1, new[lo:hi], lo)
    ref.set_band(1, new[lo:hi], lo)
    g1 = run_blocks(dspfx, torch, bank, x[NF:], n, tile)
    r1 = ref.run(x[NF:])
    assert np.array_equal(bits(g0), bits(base[:NF])), "a store applies from the next submitted run on"
    untouched = np.r_[0:lo, hi:n]
    assert np.array_equal(bits(g1[:, untouched]), bits(base[NF:, untouched])), "the untouched channels: the bits of a run with no store"
    assert not np.array_equal(bits(g1[:, lo:hi]), bits(base[NF:, lo:hi]))
    assert ulps(np.concatenate([g0, g1]), np.concatenate([r0, r1])).max() <= 1, "the stored band starts from zero state, the others go on"
    # the stored channels equal a bank that had the new band from the start but whose band-1 state is zero at block 2, and
    # whose other bands carry on: exactly what the restatement did above.  Now drop the band and store it again
    bank.set_band(1, None, lo, hi - lo)
    ref.set_band(1, None, lo, hi - lo)
    assert (bank.present(lo, hi - lo) == (((1 << (1 + K)) - 1) & ~(1 << 2))).all()
    g2 = run_blocks(dspfx, torch, bank, x[:NF], n, tile)
    r2 = ref.run(x[:NF])
    assert ulps(g2, r2).max() <= 1, "a dropped band is left out"
    bank.set_band(1, new[lo:hi], lo)
    ref.set_band(1, new[lo:hi], lo)
    g3 = run_blocks(dspfx, torch, bank, x[NF:2 * NF], n, tile)
    r3 = ref.run(x[NF:2 * NF])
    assert ulps(g3, r3).max() <= 1, "dropping a node and storing it again starts from zero state"
    # a bad band or a bad range stores nothing
    before = bank.present()
    for call in (lambda: bank.set_band(K, new[lo:hi], lo), lambda: bank.set_band(0, new, 1), lambda: bank.set_gain(su.level, 1),
                 lambda: bank.set_gain(None, n, 1), lambda: bank.set_band(0, None, 0, n + 1)):
        with pytest.raises(dspfx.DspfxError) as e:
            call()
        assert e.value.status == -1 and "strips" in str(e.value)
    assert np.array_equal(bank.present(), before)
    g4 = run_blocks(dspfx, torch, bank, x[2 * NF:], n, tile)
    r4 = ref.run(x[2 * NF:])
    assert ulps(g4, r4).max() <= 1, "refused stores leave the outputs unchanged"
    # the same run on a bank that never saw the refused calls: the same bits
    twin, _ = bank_and_ref()
    run_blocks(dspfx, torch, twin, x[:NF], n, tile)
    twin.set_band(1, new[lo:hi], lo)
    run_blocks(dspfx, torch, twin, x[NF:], n, tile)
    twin.set_band(1, None, lo, hi - lo)
    run_blocks(dspfx, torch, twin, x[:NF], n, tile)
    twin.set_band(1, new[lo:hi], lo)
    run_blocks(dspfx, torch, twin, x[NF:2 * NF], n, tile)
    t4 = run_blocks(dspfx, torch, twin, x[2 * NF:], n, tile)
    assert np.array_equal(bits(g4), bits(t4))
    bank.close()
    twin.close()


# ---- 4. isolation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", [(256, 64), (70, 0)])
def test_a_nan_channel_changes_no_other_channel(dspfx, torch_cuda, n, tile):
    K, flags = 3, 3
    su = Setup(n, K, 51)
    x = S.noise(np.random.default_rng(52), 2 * NF, n)
    bad = x.copy()
    victim = n // 2 + 1
    bad[:, victim] = np.nan
    outs = []
    for data in (x, bad):
        bank = dspfx.ChannelStrips(n, bands=K, tile_channels=tile, max_frames=NF, link_flags=flags)
        su.store(bank)
        outs.append(run_blocks(dspfx, torch_cuda, bank, data, n, tile))
        bank.close()
    others = np.arange(n) != victim
    assert np.array_equal(bits(outs[0][:, others]), bits(outs[1][:, others]))
    assert np.isnan(outs[1][:, victim]).all()


# ---- 5. against what it generalises ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("n,tile", [(256, 64), (70, 0)])
def test_uniform_strips_equal_the_engine(dspfx, torch_cuda, n, tile, K, flags):
    torch = torch_cuda
    rng = np.random.default_rng(60 + K)
    raw = S.stable_raw6(rng, K)
    level = 0.7
    x = S.noise(rng, 3 * NF, n)
    bank = dspfx.ChannelStrips(n, bands=K, tile_channels=tile, max_frames=NF, link_flags=flags)
    bank.set_gain(level)
    for b in range(K):
        bank.set_band(b, raw[b])
    got = run_blocks(dspfx, torch, bank, x, n, tile)
    bank.close()
    eng = dspfx.Engine(n, NF, link_flags=flags, tile_channels=tile)
    eng.set_chain([dspfx.Gain(level)] + [dspfx.BiQuad(*[float(q) for q in raw[b]]) for b in range(K)])
    outs = []
    for f0 in range(0, len(x), NF):
        dx = device(dspfx, torch, x[f0:f0 + NF], tile)
        dy = torch.empty_like(dx)
        eng.process(dx, out=dy, n_frames=NF)
        torch.cuda.synchronize()
        outs.append(host(dspfx, dy, NF, n, tile))
    eng.close()
    want = np.concatenate(outs)
    u = ulps(got, want)
    print(f"strips vs engine N={n} tile={tile} K={K} link_flags={flags}: {int((u != 0).sum())} of {u.size} samples differ, worst {int(u.max())} ulp")
    assert u.max() <= 1


# ---- 6. threads -----------------------------------------------------------------------------------------------------------
def test_stores_from_a_second_thread(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile, K, flags = 256, 64, 3, 3
    rng = np.random.default_rng(70)
    x = S.noise(rng, NF, n)
    dx = device(dspfx, torch, x, tile)
    dy = torch.empty_like(dx)
    bank = dspfx.ChannelStrips(n, bands=K, tile_channels=tile, max_frames=NF, link_flags=flags)
    ref = S.Strips(n, K, flags)
    calls = []
    for i in range(200):
        first, count = int(rng.integers(0, n)), int(rng.integers(1, 40))
        count = min(count, n - first)
        if i % 2:
            calls.append(("gain", rng.uniform(0.0, 4.0, count).astype(np.float32) if i % 10 != 9 else None, first, count))
        else:
            calls.append(("band", int(rng.integers(0, K)), S.stable_raw6(rng, count) if i % 10 != 8 else None, first, count))
    errors = []

    def storer():
        try:
            for c in calls:
                if c[0] == "gain":
                    bank.set_gain(c[1], c[2], c[3])
                else:
                    bank.set_band(c[1], c[2], c[3], c[4])
        except Exception as e:                                   # noqa: BLE001
            errors.append(e)

    t = threading.Thread(target=storer)
    t.start()
    for _ in range(50):
        bank.run(dx, NF, out=dy)
    t.join()
    assert not errors, errors
    for c in calls:
        if c[0] == "gain":
            ref.set_gain(c[1], c[2], c[3])
        else:
            ref.set_band(c[1], c[2], c[3], c[4])
    assert np.array_equal(bank.present(), ref.mask)
    bank.reset()
    bank.run(dx, NF, out=dy)
    torch.cuda.synchronize()
    got = host(dspfx, dy, NF, n, tile)
    bank.close()
    ref.reset()
    assert ulps(got, ref.run(x)).max() <= 1


# ---- 7. full size ---------------------------------------------------------------------------------------------------------
def test_full_size(dspfx, torch_cuda):
    """2^20 channels x 128 frames, K = 4, tiled 256, every node present, two alternating buffer pairs, device events, median of
    20 after 5 warm-ups.  Asserted: one run fits the 2.667 ms a 128-frame block lasts at 48 kHz.  Printed in the same run: the
    time, the fraction of 8 TB/s on the bank's own bytes, and the ratios to a flat copy, to a Gain-chain Engine and to the
    [Gain, BiQuad x 4] Engine on the same buffers."""
    torch = torch_cuda
    n, nf, tile, K = 1 << 20, 128, 256, 4
    rng = np.random.default_rng(81)
    eng = dspfx.Engine(n, nf, link_flags=0, tile_channels=tile)
    eng.set_chain([dspfx.Gain(0.7)])
    assert eng.kernels_ready()
    xs = [torch.empty(nf * n, dtype=torch.float32, device="cuda") for _ in range(2)]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    for i, x in enumerate(xs):
        eng.fill_noise(x, nf, 1000 * i)

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

    bank = dspfx.ChannelStrips(n, bands=K, tile_channels=tile, max_frames=nf, link_flags=0)
    bank.set_gain(rng.uniform(0.5, 1.5, n).astype(np.float32))
    raw = S.stable_raw6(rng, 4096)
    for b in range(K):
        bank.set_band(b, np.tile(np.roll(raw, b, axis=0), (n // 4096, 1)))
    assert (bank.present() == (1 << (1 + K)) - 1).all()
    t_strips = timed(lambda i: bank.run(xs[i % 2], nf, out=ys[i % 2]))
    # a sample of channels of the last run (block 1 into ys[1]) is finite and differs from its input
    torch.cuda.synchronize()
    assert torch.isfinite(ys[1][:1 << 16]).all() and not torch.equal(ys[1][:1 << 16], xs[1][:1 << 16])
    bank.close()
    t_copy = timed(lambda i: ys[i % 2].copy_(xs[i % 2]))
    t_gain = timed(lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=nf))
    eng.close()
    eng = dspfx.Engine(n, nf, link_flags=0, tile_channels=tile)
    eng.set_chain([dspfx.Gain(0.7)] + [dspfx.BiQuad(*[float(q) for q in raw[b]]) for b in range(K)])
    eng.kernels_ready(20000)                                     # (printed only: whichever kernel serves by then is what is timed)
    t_chain = timed(lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=nf))
    eng.close()
    own = nf * n * 8 + n * (K * 5 * 4 + 2 * K * 4 * 4 + 4 + 4)   # the block in and out; coefficients, state in and out, levels, masks
    print(f"full size strips K={K}: {t_strips:.4f} ms ({own / t_strips / 1e9 / 8.0:.3f} of 8 TB/s on {own / 2**20:.0f} MiB), "
          f"x flat copy {t_strips / t_copy:.3f} (copy {t_copy:.4f} ms), x Gain chain {t_strips / t_gain:.3f} (Gain {t_gain:.4f} ms), "
          f"x [Gain, BiQuad x 4] engine {t_strips / t_chain:.3f} (engine {t_chain:.4f} ms)")
    assert t_strips <= 2.667, t_strips
