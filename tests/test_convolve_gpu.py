"""The convolver bank on the GPU (dspfx_convolve_*) against the exact float64 convolution in convolve_ref.py.  The bars are
the FIR row's: relative RMS <= 1e-6 per channel over the run, and per block an error RMS <= 1e-6 of the
channel's RMS over the run.  The float32 restatement's own error is printed beside the GPU's and is never a bar."""
import numpy as np
import pytest

import convolve_ref as R
import mixgroups_ref
import oracle as O

pytestmark = pytest.mark.gpu

B = 128
LAYOUTS = [(64, 0), (256, 64)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_cache = {}


def case(T, N, blocks, seed=0):
    """(h, x, exact y), computed once and shared; nobody writes into them"""
    key = (T, N, blocks, seed)
    if key not in _cache:
        h = R.response(T, seed=seed)
        x = R.noise(blocks * B, N, seed=seed)
        want = R.exact(x, h)
        for a in (h, x, want):
            a.setflags(write=False)
        _cache[key] = (h, x, want)
    return _cache[key]


def feed(dspfx, torch, bank, x, tile, n_frames=B, in_place=False, first_block=0):
    """x [F][N] (host, frame-major) through `bank`, n_frames per call -> [F][N] (host); one synchronisation at the end"""
    F, N = x.shape
    calls = F // n_frames
    lay = np.stack([dspfx.to_layout(x[i * n_frames:(i + 1) * n_frames], tile).reshape(-1) for i in range(calls)])
    dx = torch.from_numpy(lay).cuda()
    dy = dx if in_place else torch.full_like(dx, float("nan"))
    for i in range(calls):
        bank.run(dx[i], n_frames, out=dy[i])
    torch.cuda.synchronize()
    out = dy.cpu().numpy()
    return np.concatenate([dspfx.from_layout(out[i], n_frames, N, tile) for i in range(calls)])


def report(what, got, want, ref32=None):
    rr, br = R.rel_rms(got, want), R.block_rms(got, want)
    line = f"{what}: GPU rel RMS {rr.max():.3e}, worst block {br.max():.3e}"
    if ref32 is not None:
        line += f" | float32 restatement rel RMS {R.rel_rms(ref32, want[:, :ref32.shape[1]]).max():.3e}, " \
                f"worst block {R.block_rms(ref32, want[:, :ref32.shape[1]]).max():.3e}"
    print(line)
    return rr, br


# ---- accuracy -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,tile", LAYOUTS, ids=["n64", "n256_tile64"])
@pytest.mark.parametrize("T", R.SIZES)
def test_accuracy(dspfx, torch_cuda, T, N, tile):
    P = R.partitions(T)
    blocks = max(2 * P + 3, 6)                                                  # the ring wraps twice
    h, x, want = case(T, N, blocks)
    bank = dspfx.Convolver(N, h, tile_channels=tile)
    assert bank.partitions == P
    got = feed(dspfx, torch_cuda, bank, x, tile)
    bank.close()
    ref32 = R.Partitioned(8, h).run_all(x[:, :8])
    rr, br = report(f"T={T} P={P} N={N} tile={tile} blocks={blocks}", got, want, ref32)
    assert np.isfinite(got).all()
    assert rr.max() <= R.BAR and br.max() <= R.BAR


def test_accuracy_of_a_one_second_room(dspfx, torch_cuda):
    """T = 48 000 (P = 375) at N = 64 over 400 blocks: the ring wraps and every slot is live."""
    T, N, blocks = 48000, 64, 400
    h, x, want = case(T, N, blocks)
    bank = dspfx.Convolver(N, h)
    assert bank.partitions == 375
    got = feed(dspfx, torch_cuda, bank, x, 0)
    bank.close()
    ref32 = R.Partitioned(2, h).run_all(x[:, :2])
    rr, br = report(f"T={T} P=375 N={N} blocks={blocks}", got, want, ref32)
    assert rr.max() <= R.BAR and br.max() <= R.BAR


# ---- unit impulse ---------------------------------------------------------------------------------------------------

def dyadic_period4(frames, N, seed):
    """Every channel repeats four multiples of 1/8 in [-1, 1] \\ {0}.  Such a window's spectrum lies on DC, Nyquist and bin 64
    alone, where every twiddle is +-1 or +-i (the tables hold them exactly) and every sum is a small dyadic number, so each
    step of both transforms is exact in f32: the one kind of data on which an FFT can return the input bit for bit."""
    rng = np.random.default_rng(seed)
    pat = rng.integers(1, 9, (4, N)) * rng.choice([-1, 1], (4, N))
    return (np.tile(pat, (frames // 4, 1)) / 8.0).astype(np.float32)


@pytest.mark.parametrize("N,tile", LAYOUTS, ids=["n64", "n256_tile64"])
def test_unit_impulse_balanced(dspfx, torch_cuda, N, tile):
    """T = 1, h = [1]: the output is the input bit for bit wherever the arithmetic is exact (from block 1 on, whose window
    is periodic), and on noise it meets the accuracy bar (an FFT round trip in f32 cannot be bit-exact on arbitrary data: the
    figure is printed)."""
    x = dyadic_period4(6 * B, N, 3)
    bank = dspfx.Convolver(N, [1.0], tile_channels=tile)
    got = feed(dspfx, torch_cuda, bank, x, tile)
    assert np.array_equal(bits(got[B:]), bits(x[B:]))
    rr, br = report("T=1 block 0 (silence then the pattern)", got[:B], x[:B].astype(np.float64))
    assert rr.max() <= R.BAR
    bank.reset()
    xn = R.noise(6 * B, N, seed=5)
    gn = feed(dspfx, torch_cuda, bank, xn, tile)
    bank.close()
    ulp = np.abs(gn.view(np.int32).astype(np.int64) - xn.view(np.int32).astype(np.int64))
    print(f"T=1 on noise: {np.count_nonzero(ulp)} of {ulp.size} samples differ, median {np.median(ulp):.0f} ulp")
    rr, br = report("T=1 on noise", gn, xn.astype(np.float64))
    assert rr.max() <= R.BAR and br.max() <= R.BAR


@pytest.mark.parametrize("N,tile", LAYOUTS, ids=["n64", "n256_tile64"])
def test_unit_impulse_average_delayed(dspfx, torch_cuda, N, tile):
    """T = 300 with the impulse on the last tap, Average: y[n] = x[n - 299] * (1.0f / 300.0f), to 1 ulp from block 3 on
    (all three partitions' windows periodic); the blocks before, and noise, meet the accuracy bar."""
    T = 300
    h = np.zeros(T)
    h[T - 1] = 1.0
    div = np.float32(1.0) / np.float32(T)
    x = dyadic_period4(8 * B, N, 4)
    bank = dspfx.Convolver(N, h, mode=dspfx.FIR_AVERAGE, tile_channels=tile)
    assert bank.partitions == 3
    got = feed(dspfx, torch_cuda, bank, x, tile)
    want = np.zeros_like(x)
    want[T - 1:] = x[:-(T - 1)] * div
    ulp = np.abs(got[3 * B:].view(np.int32).astype(np.int64) - want[3 * B:].view(np.int32).astype(np.int64))
    print(f"T=300 Average, delayed impulse: max {ulp.max()} ulp from block 3 on")
    assert ulp.max() <= 1
    exact = R.exact(x, h, 1.0 / T)
    assert R.rel_rms(got, exact).max() <= R.BAR
    bank.reset()
    xn = R.noise(8 * B, N, seed=6)
    gn = feed(dspfx, torch_cuda, bank, xn, tile)
    bank.close()
    rr, br = report("T=300 Average on noise", gn, R.exact(xn, h, float(div)))
    assert rr.max() <= R.BAR and br.max() <= R.BAR


# ---- same bits ------------------------------------------------------------------------------------------------------

def test_same_bits_across_layouts_resets_in_place_and_call_sizes(dspfx, torch_cuda):
    T, N = 1000, 256
    h, x, want = case(T, N, 20)
    frame_major = dspfx.Convolver(N, h)
    a = feed(dspfx, torch_cuda, frame_major, x, 0)
    assert R.rel_rms(a, want).max() <= R.BAR
    tiled = dspfx.Convolver(N, h, tile_channels=64)
    assert np.array_equal(bits(a), bits(feed(dspfx, torch_cuda, tiled, x, 64))), "frame-major against tiled"
    for bank, tile in ((frame_major, 0), (tiled, 64)):
        bank.reset()
        assert np.array_equal(bits(a), bits(feed(dspfx, torch_cuda, bank, x, tile))), "two runs after reset"
        bank.reset()
        assert np.array_equal(bits(a), bits(feed(dspfx, torch_cuda, bank, x, tile, in_place=True))), "out == in"
        bank.reset()
        assert np.array_equal(bits(a), bits(feed(dspfx, torch_cuda, bank, x, tile, n_frames=2 * B))), "256 frames a call"
        bank.reset()
        assert np.array_equal(bits(a), bits(feed(dspfx, torch_cuda, bank, x, tile, n_frames=2 * B, in_place=True)))
        bank.close()
    L = dspfx.lib()
    bank = dspfx.Convolver(N, h)
    t = torch_cuda.zeros(B * N, device="cuda")
    for n_frames in (0, 1, 127, 129, 200):
        with pytest.raises(dspfx.DspfxError) as ei:
            bank.run(t, n_frames, out=t)
        assert ei.value.status == -1
    assert L.dspfx_convolve_run(bank.h, None, None, B, None) == -1
    bank.close()


# ---- channel independence -------------------------------------------------------------------------------------------

def test_channel_independence_and_a_nan_neighbour(dspfx, torch_cuda):
    T, blocks = 1000, 24
    P = R.partitions(T)
    h, x256, _ = case(T, 256, blocks, seed=9)
    x64 = x256[:, :64]
    nan_at = 5 * B + 77                                                         # one NaN sample on channel 6, in block 5

    def run(x, N):
        bank = dspfx.Convolver(N, h)
        y = feed(dspfx, torch_cuda, bank, x, 0)
        bank.close()
        return y

    base = run(x64, 64)
    five = bits(base[:, 5])
    assert np.array_equal(five, bits(run(x256, 256)[:, 5])), "64 or 256 channels wide"
    silent = np.zeros_like(x64)
    silent[:, 5] = x64[:, 5]
    assert np.array_equal(five, bits(run(silent, 64)[:, 5])), "neighbours silent"
    loud = (x64 * np.float32(100.0)).astype(np.float32)
    loud[:, 5] = x64[:, 5]
    assert np.array_equal(five, bits(run(loud, 64)[:, 5])), "neighbours 100 times louder"
    poisoned = x64.copy()
    poisoned[nan_at, 6] = np.nan
    y = run(poisoned, 64)
    assert np.array_equal(five, bits(y[:, 5])), "a neighbour carrying one NaN"
    others = [c for c in range(64) if c != 6]
    assert np.array_equal(bits(y[:, others]), bits(base[:, others]))
    bad = np.isnan(y[:, 6]).reshape(blocks, B).any(axis=1)
    first = nan_at // B
    # the sample is in the windows of blocks `first` and `first + 1`, and each spectrum is read for P blocks
    assert not bad[:first].any() and bad[first] and not bad[first + P + 1:].any(), bad
    assert bad.sum() <= P + 1
    assert np.isfinite(y[(first + P + 1) * B:, 6]).all()
    assert np.array_equal(bits(y[:first * B, 6]), bits(base[:first * B, 6]))


# ---- reload ---------------------------------------------------------------------------------------------------------

def test_reload_keeps_the_history(dspfx, torch_cuda):
    N = 64
    ha, hb, hc = R.response(1000, seed=1), R.response(1000, seed=2), R.response(4096, seed=3)
    x = R.noise(56 * B, N, seed=8)
    cut1, cut2 = 12 * B, 24 * B
    bank = dspfx.Convolver(N, ha, max_taps=4096)
    a = feed(dspfx, torch_cuda, bank, x[:cut1], 0)
    bank.set_taps(hb)
    assert bank.partitions == 8
    b = feed(dspfx, torch_cuda, bank, x[cut1:cut2], 0)
    bank.set_taps(hc)
    assert bank.partitions == 32
    c = feed(dspfx, torch_cuda, bank, x[cut2:cut2 + 6 * B], 0)
    # 4097 taps: refused, and the next block is what it would have been
    with pytest.raises(dspfx.DspfxError) as ei:
        bank.set_taps(R.response(4097))
    assert ei.value.status == -1 and bank.partitions == 32
    c2 = feed(dspfx, torch_cuda, bank, x[cut2 + 6 * B:], 0)
    bank.close()
    # from each reload's block on: the new response convolved with the whole input since reset
    for what, got, hh, lo, hi in (("first response", a, ha, 0, cut1), ("reload to 1000 taps", b, hb, cut1, cut2),
                                  ("reload to 4096 taps", np.concatenate([c, c2]), hc, cut2, len(x))):
        want = R.exact(x, hh)[lo:hi]
        rr, br = report(what, got, want)
        assert rr.max() <= R.BAR and br.max() <= R.BAR, what
    fresh = dspfx.Convolver(N, hc, max_taps=4096)                               # the same bits as a bank that was never refused
    f = feed(dspfx, torch_cuda, fresh, x, 0)
    fresh.close()
    assert R.rel_rms(f, R.exact(x, hc)).max() <= R.BAR


# ---- pipeline -------------------------------------------------------------------------------------------------------

def test_rooms_reverb_master_chain_without_a_host_copy(dspfx, torch_cuda):
    """Engine(256) -> MixGroups(group_size=64) -> Convolver(4, T=1000) -> Engine(4, tile_channels=0), device to device; each
    stage against its own reference on what the stage before it really produced."""
    torch = torch_cuda
    n, rooms, T, blocks = 256, 4, 1000, 19
    chain = [dspfx.BiQuad(1.0, -1.8, 0.81, 0.0025, 0.005, 0.0025), dspfx.Gain(0.5)]
    master = [dspfx.LowPass(0.25), dspfx.Gain(2.0)]
    h = R.response(T, seed=4)
    eng = dspfx.Engine(n, B, link_flags=3, tile_channels=0)
    eng.set_chain(chain)
    mg = dspfx.MixGroups(n, group_size=64, max_frames=B)
    reverb = dspfx.Convolver(mg.groups, h)
    meng = dspfx.Engine(rooms, B, link_flags=3, tile_channels=0)
    meng.set_chain(master)
    x = torch.empty(B * n, dtype=torch.float32, device="cuda")
    y = torch.empty_like(x)
    buses = torch.empty((blocks, B, rooms), dtype=torch.float32, device="cuda")
    wet = torch.empty_like(buses)
    out = torch.empty_like(buses)
    xs, ys = [], []
    for b in range(blocks):
        eng.fill_noise(x, B, b * B)
        eng.process(x, out=y, n_frames=B)
        mg.run(y, B, out=buses[b])
        reverb.run(buses[b], B, out=wet[b])
        meng.process(wet[b], out=out[b], n_frames=B)
        xs.append(x.cpu().numpy().reshape(B, n))
        ys.append(y.cpu().numpy().reshape(B, n))
    torch.cuda.synchronize()
    xh, yh = np.concatenate(xs), np.concatenate(ys)
    bh, wh, oh = (t.cpu().numpy().reshape(blocks * B, rooms) for t in (buses, wet, out))
    chans = [0, 1, 63, 64, 200, n - 1]
    want_y = O.run_channels([c.oracle_desc() for c in chain], xh[:, chans], 3)
    assert np.abs(yh[:, chans].view(np.int32).astype(np.int64) - want_y.view(np.int32).astype(np.int64)).max() <= 1
    table = np.arange(0, n + 1, 64, dtype=np.uint64)
    depth = dspfx.mixgroups_plan(n, group_start=table)
    ref, sabs, _ = mixgroups_ref.buses(yh, table, None, True, list(range(rooms)))
    assert (np.abs(bh.astype(np.float64) - ref) <= mixgroups_ref.bound(sabs, ref, depth[None, :].astype(np.float64))).all()
    rr, br = report("reverb on the buses", wh, R.exact(bh, h))
    assert rr.max() <= R.BAR and br.max() <= R.BAR
    want_o = O.run_channels([c.oracle_desc() for c in master], wh, 3)
    assert np.abs(oh.view(np.int32).astype(np.int64) - want_o.view(np.int32).astype(np.int64)).max() <= 1
    for o in (meng, reverb, mg, eng):
        o.close()


# ---- full size ------------------------------------------------------------------------------------------------------

def test_full_size(dspfx, torch_cuda):
    """N = 4096 buses, T = 48 000 (P = 375), one 128-frame block: a run takes no longer than the 2.667 ms a block lasts (the
    project's own budget).  Device events, the median of 20 after warm-up runs past P blocks so that every slot is live.  A flat
    torch copy of the bytes the accumulation reads (P * 1024 * N = 1.5 GiB) is timed in the same run and the ratio PRINTED."""
    torch = torch_cuda
    N, T, reps = 4096, 48000, 20
    h = R.response(T)
    bank = dspfx.Convolver(N, h)
    P = bank.partitions
    x = torch.from_numpy(R.noise(B, N, seed=11).reshape(-1)).cuda()
    y = torch.empty_like(x)
    for _ in range(P + 5):                                                      # warm-up: past P blocks
        bank.run(x, B, out=y)
    torch.cuda.synchronize()

    def timed(fn):
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    run_ms = timed(lambda: bank.run(x, B, out=y))
    nbytes = P * 1024 * N
    src = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    for _ in range(5):
        dst.copy_(src)
    torch.cuda.synchronize()
    copy_ms = timed(lambda: dst.copy_(src))
    got = y.cpu().numpy().reshape(B, N)
    bank.close()
    print(f"full size: N={N} T={T} P={P}: {run_ms:.3f} ms per run (budget 2.667), flat copy of {nbytes / 2**30:.2f} GiB "
          f"{copy_ms:.3f} ms, run / copy = {run_ms / copy_ms:.2f}; the ring read alone is "
          f"{nbytes / (run_ms * 1e-3) / 8e12:.2f} of the 8 TB/s peak")
    assert np.isfinite(got).all() and got.any()
    assert run_ms <= 128 / 48000 * 1e3
