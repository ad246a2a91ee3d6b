"""The channel-dynamics bank on the GPU (dspfx_dynamics_*, through the Python class): per-channel envelopes, the gain computer, the
key, the stores.  Everything is compared bit for bit with dynamics_ref, which tests/test_dynamics_cpu.py holds to the oracle's
Envelope and Gain nodes bit for bit.  One exception, the project's own (tests/edge_values.py): where the restatement gives a NaN the
bank must give a NaN, its sign and payload are not compared -- x86 and the GPU make them differently."""
import threading

import numpy as np
import pytest

import dynamics_ref as R
import edge_values as E

pytestmark = pytest.mark.gpu

NF = 128
F = np.float32
SHAPES = [(64, 0), (256, 64), (70, 0), (1, 0)]                   # vector lanes; tiled; scalar accesses and a ragged last workgroup; one channel
TWO = [(256, 64), (70, 0)]
ATTACKS, RELEASES = [0, 1, 48, 1000], [0, 1, 1000, 24000]
THRESHOLDS, MAKEUPS = [0.0125, 0.1, 0.25, 0.5], [1.0, 0.7, 3.0, 8.0]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def noise(rng, nf, n):
    return rng.uniform(-1.0, 1.0, (nf, n)).astype(F)


def device(dspfx, torch, x, tile):
    return torch.from_numpy(dspfx.to_layout(x, tile).reshape(-1).copy()).cuda()


def host(dspfx, t, nf, n, tile):
    return dspfx.from_layout(t.cpu().numpy(), nf, n, tile)


def sliders(rng, n):
    return dict(threshold=rng.choice(THRESHOLDS, n).astype(F), makeup=rng.choice(MAKEUPS, n).astype(F),
                attack=rng.choice(ATTACKS, n).astype(F), release=rng.choice(RELEASES, n).astype(F))


def both(bank, ref, call):
    call(bank)
    assert call(ref) is not False


def pair(dspfx, n, tile, seed=None, nodeless=True):
    """a bank and its restatement; seed: every channel's sliders drawn from the small sets, and (nodeless) every third channel left
    without a node"""
    bank, ref = dspfx.ChannelDynamics(n, tile_channels=tile, max_frames=NF), R.ChannelDynamics(n)
    if seed is not None:
        kw = sliders(np.random.default_rng(seed), n)
        both(bank, ref, lambda b: b.set(**kw))
        if nodeless:
            for c in range(1, n, 3):
                both(bank, ref, lambda b: b.drop(c, 1))
    return bank, ref


def tables_equal(torch, bank, ref, what):
    torch.cuda.synchronize()
    assert np.array_equal(bits(bank.levels().cpu().numpy()), bits(ref.level)), f"{what}: levels"
    assert np.array_equal(bits(bank.reductions().cpu().numpy()), bits(ref.reduction)), f"{what}: reductions"
    assert np.array_equal(bank.present(), ref.present()), f"{what}: presence"


def step(dspfx, torch, bank, ref, blk, n, tile, what, inplace=False, key=None, key_is_block=False):
    """one block through both; the output (NaN judged by isnan), the levels and the reductions bit for bit.  Out of place the
    output starts as NaN everywhere: every sample is written"""
    dx = device(dspfx, torch, blk, tile)
    dk = dx if key_is_block else None if key is None else device(dspfx, torch, key, tile)
    want = ref.run(blk, key)
    dy = bank.run(dx, len(blk), out=dx if inplace else torch.full_like(dx, float("nan")), key=dk)
    torch.cuda.synchronize()
    got = host(dspfx, dy, len(blk), n, tile)
    E.same_bits_or_nan(got, want, None, f"{what}: output")
    tables_equal(torch, bank, ref, what)
    return got


def loudness(rng, runs, nf, n):
    """per channel and block 0.05 or 1.0: channels cross their thresholds both ways"""
    return rng.choice([0.05, 1.0], (runs, 1, n)).astype(F).repeat(nf, 1).reshape(runs * nf, n)


# ---- 1. several blocks against the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("nf,runs", [(1, 40), (37, 6), (128, 6)])
@pytest.mark.parametrize("n,tile", SHAPES)
def test_output_levels_and_reductions_equal_the_restatement(dspfx, torch_cuda, n, tile, nf, runs):
    """every channel its own sliders, a third of them without a node; with one-frame blocks the level is the envelope after every
    single frame"""
    rng = np.random.default_rng(100 + n + nf)
    x = noise(rng, (runs + 1) * nf, n) * loudness(rng, runs + 1, nf, n)
    bank, ref = pair(dspfx, n, tile)
    got = step(dspfx, torch_cuda, bank, ref, x[:nf], n, tile, "fresh")
    assert np.array_equal(bits(got), bits(x[:nf])) and not ref.level.any() and (ref.reduction == 1).all(), "a fresh bank's first run is a copy"
    kw = sliders(np.random.default_rng(n), n)
    both(bank, ref, lambda b: b.set(**kw))
    for c in range(1, n, 3):
        both(bank, ref, lambda b: b.drop(c, 1))
    above, below = np.zeros(n, bool), np.zeros(n, bool)
    for b in range(1, runs + 1):
        blk = x[b * nf:(b + 1) * nf]
        got = step(dspfx, torch_cuda, bank, ref, blk, n, tile, f"N={n} tile={tile} nf={nf} block {b}")
        above |= ref.on & (ref.reduction < 1)
        below |= ref.on & (ref.reduction == 1)
        if nf == 1:
            assert np.array_equal(bits(ref.level), bits(np.where(ref.on, ref.envs[0], F(0))))
        assert np.array_equal(bits(got[:, ~ref.on]), bits(blk[:, ~ref.on])), "no node: a copy"
    assert (ref.level[~ref.on] == 0).all() and (ref.reduction[~ref.on] == 1).all()
    assert n < 64 or (above & below).any(), "channels are above their threshold in one block and below it in another"
    bank.close()


# ---- 2. layout and neighbour independence ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", SHAPES)
def test_in_place_equals_out_of_place(dspfx, torch_cuda, n, tile):
    rng = np.random.default_rng(200 + n)
    x = noise(rng, 3 * NF, n) * loudness(rng, 3, NF, n)
    bank, ref = pair(dspfx, n, tile, seed=20 + n)
    for b in range(3):
        step(dspfx, torch_cuda, bank, ref, x[b * NF:(b + 1) * NF], n, tile, f"N={n} block {b}", inplace=b != 1)
    bank.close()


@pytest.mark.parametrize("n,tile", [(64, 0), (256, 64), (70, 0)])
def test_a_channels_bits_do_not_depend_on_its_neighbours(dspfx, torch_cuda, n, tile):
    """the kept channels (one of each lane's four, and the last) get the same samples and sliders in two banks; every other
    channel differs in both, has no node, or carries NaN samples"""
    torch = torch_cuda
    rng = np.random.default_rng(210 + n)
    keep = np.zeros(n, bool)
    keep[(np.arange(n) % 4) == (np.arange(n) // 4) % 4] = True
    keep[n - 1] = True
    x = noise(rng, 2 * NF, n)
    x2 = np.where(keep, x, noise(rng, 2 * NF, n) * F(5))
    x2[:, np.flatnonzero(~keep)[::3]] = np.nan
    kw = sliders(rng, n)
    kw2 = {k: np.where(keep, v, w) for (k, v), w in zip(kw.items(), sliders(rng, n).values())}
    a, ra = pair(dspfx, n, tile)
    b, rb = pair(dspfx, n, tile)
    both(a, ra, lambda t: t.set(**kw))
    both(b, rb, lambda t: t.set(**kw2))
    for c in np.flatnonzero(~keep)[1::3]:
        both(b, rb, lambda t: t.drop(int(c), 1))
    for blk in range(2):
        sl = slice(blk * NF, (blk + 1) * NF)
        ya = step(dspfx, torch, a, ra, x[sl], n, tile, f"bank a block {blk}")
        yb = step(dspfx, torch, b, rb, x2[sl], n, tile, f"bank b block {blk}")
        assert np.array_equal(bits(ya[:, keep]), bits(yb[:, keep]))
        for va, vb in ((a.levels(), b.levels()), (a.reductions(), b.reductions())):
            assert np.array_equal(bits(va.cpu().numpy()[keep]), bits(vb.cpu().numpy()[keep]))
    a.close()
    b.close()


# ---- 3. the key ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", SHAPES)
def test_the_key(dspfx, torch_cuda, n, tile):
    """key == block is no key; another key drives the envelope and the block takes the gain; a key works in place"""
    torch = torch_cuda
    rng = np.random.default_rng(300 + n)
    x = noise(rng, 4 * NF, n)
    k = noise(rng, 4 * NF, n) * loudness(rng, 4, NF, n)
    bank, ref = pair(dspfx, n, tile, seed=30 + n)
    plain, rp = pair(dspfx, n, tile, seed=30 + n)
    for b, nf in enumerate([NF, NF, 37, 1]):                     # (37: whole chunks of 4 and one row left)
        sl = slice(b * NF, b * NF + nf)
        step(dspfx, torch, bank, ref, x[sl], n, tile, f"N={n} keyed block {b}", inplace=b == 1, key=k[sl])
        step(dspfx, torch, plain, rp, k[sl], n, tile, f"N={n} key == block, block {b}", inplace=b == 1, key_is_block=True)
        # the keyed bank's envelope is the plain bank's, whose block is the key
        assert np.array_equal(bits(ref.env), bits(rp.env)) and np.array_equal(bits(ref.level), bits(rp.level))
    bank.close()
    plain.close()


# ---- 4. stores -------------------------------------------------------------------------------------------------------------
def test_a_store_between_two_submitted_runs_changes_exactly_the_second(dspfx, torch_cuda):
    """nothing waits between the calls: run, store, run, partial store, run, drop, run, re-add, run -- then everything is read"""
    torch = torch_cuda
    n, tile = 256, 64
    rng = np.random.default_rng(400)
    x = noise(rng, 6 * NF, n)
    bank, ref = pair(dspfx, n, tile, seed=40)
    dxs = [device(dspfx, torch, x[i * NF:(i + 1) * NF], tile) for i in range(6)]
    dys = [torch.full_like(d, float("nan")) for d in dxs]
    torch.cuda.synchronize()
    kw = sliders(rng, 100)
    stores = {
        1: lambda b: b.set(first_channel=50, **kw),
        2: lambda b: b.set(makeup=0.5, first_channel=70, count=30),     # a partial store keeps threshold, attack and release
        3: lambda b: b.drop(0, 64),
        4: lambda b: b.set(threshold=0.1, release=48.0, first_channel=0, count=64),      # re-added: a zero envelope, default makeup and attack
        5: lambda b: b.reset(100, 50),
    }
    want = []
    for i in range(6):
        if i in stores:
            both(bank, ref, stores[i])
        bank.run(dxs[i], NF, out=dys[i])
        want.append(ref.run(x[i * NF:(i + 1) * NF]))
        if i == 3:
            assert not ref.env[:64].any() and not ref.on[:64].any()
    torch.cuda.synchronize()
    for i in range(6):
        E.same_bits_or_nan(host(dspfx, dys[i], NF, n, tile), want[i], None, f"run {i}")
    tables_equal(torch, bank, ref, "after the stores")
    assert ref.mk[70] == F(0.5) and ref.thr[70] == kw["threshold"][20] and ref.gr[70] == R.envelope_gain(kw["release"][20])
    assert ref.thr[0] == F(0.1) and ref.mk[0] == 1 and ref.ga[0] == 0
    bank.close()


def test_a_refused_store_changes_nothing(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile = 70, 0
    rng = np.random.default_rng(410)
    x = noise(rng, 2 * NF, n)
    bank, ref = pair(dspfx, n, tile, seed=41)
    step(dspfx, torch, bank, ref, x[:NF], n, tile, "before")
    bad = [dict(threshold=float("nan")), dict(threshold=-0.5), dict(threshold=-0.0), dict(threshold=[0.5, float("nan")], makeup=[1.0, 1.0]),
           dict(makeup=float("nan")), dict(makeup=float("inf")), dict(makeup=-1.0), dict(makeup=-0.0),
           dict(threshold=0.5, first_channel=n - 1, count=2), dict(threshold=0.5, first_channel=n + 1, count=0)]
    words = ["threshold"] * 4 + ["makeup"] * 4 + ["channels"] * 2
    for kw, word in zip(bad, words):
        with pytest.raises(dspfx.DspfxError) as e:
            bank.set(**kw)
        assert e.value.status == -1 and word in str(e.value) and "dynamics" in str(e.value), str(e.value)
        assert ref.set(**kw) is False, kw
    for call in (lambda b: b.drop(n, 1), lambda b: b.reset(n - 1, 2), lambda b: b.present(1, n)):
        with pytest.raises(dspfx.DspfxError) as e:
            call(bank)
        assert e.value.status == -1 and "dynamics" in str(e.value), str(e.value)
    with pytest.raises(dspfx.DspfxError):
        bank.run(device(dspfx, torch, x[:NF], tile), NF + 1)
    step(dspfx, torch, bank, ref, x[NF:], n, tile, "after the refused stores")
    both(bank, ref, lambda b: b.set(threshold=float("inf"), first_channel=0, count=4))       # allowed: never turned down
    both(bank, ref, lambda b: b.set(threshold=0.0, makeup=0.0, first_channel=4, count=4))
    step(dspfx, torch, bank, ref, x[NF:], n, tile, "an infinite and a zero threshold")
    assert (ref.reduction[:4] == 1).all() and not ref.reduction[4:8].any()
    bank.close()


def test_a_second_thread_repeating_the_same_stores(dspfx, torch_cuda):
    """the stores a second thread makes while 100 runs go are the ones already made, piece by piece: idempotent, so whichever runs
    they land between, the result is the restatement's"""
    torch = torch_cuda
    n, tile, runs = 256, 64, 100
    rng = np.random.default_rng(420)
    x = noise(rng, 4 * NF, n) * loudness(rng, 4, NF, n)
    bank, ref = pair(dspfx, n, tile, seed=42, nodeless=False)
    kw = sliders(np.random.default_rng(42), n)                   # what pair() stored
    dxs = [device(dspfx, torch, x[i * NF:(i + 1) * NF], tile) for i in range(4)]
    dys = [torch.empty_like(dxs[0]) for _ in range(runs)]
    torch.cuda.synchronize()
    done, errors, made = threading.Event(), [], [0]

    def storer():
        try:
            r = np.random.default_rng(1)
            while not done.is_set() or made[0] < 20:
                first = int(r.integers(0, n))
                count = int(min(r.integers(1, 60), n - first))
                part = {k: v[first:first + count] for k, v in kw.items() if r.random() < 0.7}
                bank.set(first_channel=first, count=count, **part)
                made[0] += 1
        except Exception as e:                                   # noqa: BLE001
            errors.append(e)

    t = threading.Thread(target=storer)
    t.start()
    for i in range(runs):
        bank.run(dxs[i % 4], NF, out=dys[i])
    done.set()
    t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    assert made[0] >= 20
    for i in range(runs):
        want = ref.run(x[(i % 4) * NF:(i % 4 + 1) * NF])
        assert np.array_equal(bits(host(dspfx, dys[i], NF, n, tile)), bits(want)), f"run {i}"
    tables_equal(torch, bank, ref, "after the threads")
    bank.close()


# ---- 5. the brick wall -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", TWO)
def test_brick_wall(dspfx, torch_cuda, n, tile):
    """attack 0, noise of amplitude 4, threshold 0.25: |out| <= thr * mk * (1 + 2^-24)^3 on every sample, and the restatement's bits"""
    torch = torch_cuda
    rng = np.random.default_rng(500 + n)
    x = noise(rng, 4 * NF, n) * F(4)
    mk = rng.choice([0.7, 1.0, 3.0], n).astype(F)
    rel = rng.choice([0, 1, 48, 1000, 24000], n).astype(F)
    bank, ref = pair(dspfx, n, tile)
    both(bank, ref, lambda b: b.set(threshold=0.25, makeup=mk, attack=0.0, release=rel))
    bound = (np.float64(F(0.25)) * mk.astype(np.float64) * (1.0 + 2.0 ** -24) ** 3)
    for b in range(4):
        got = step(dspfx, torch, bank, ref, x[b * NF:(b + 1) * NF], n, tile, f"N={n} block {b}")
        assert (np.abs(got.astype(np.float64)) <= bound).all()
        assert (ref.reduction < 1).all() and (ref.level >= np.abs(x[b * NF:(b + 1) * NF]).max(axis=0)).all()
    bank.close()


# ---- 6. edge values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_key", [False, True])
@pytest.mark.parametrize("n,tile", TWO)
def test_edge_values(dspfx, torch_cuda, n, tile, as_key):
    """NaN, both infinities, signed zeros and subnormals in the samples, or in the key over plain noise; the non-finite values sit
    in the second block, taken frame by frame.  A NaN envelope stays NaN, gives q = 1 and never raises the level; a reset ends it"""
    torch = torch_cuda
    edge, tab = E.edge_block(n, 3 * NF)
    plain = noise(np.random.default_rng(600 + n), 3 * NF, n)
    x, k = (plain, edge) if as_key else (edge, None)
    bank, ref = pair(dspfx, n, tile)
    kw = sliders(np.random.default_rng(60), n)
    kw["threshold"][:len(E.CLASS_NAMES)] = [0.0, 2.0 ** -140, 0.25, np.inf, 1e-30, 0.5, 3e38, 0.25, 0.1, 0.25]
    both(bank, ref, lambda b: b.set(**kw))
    both(bank, ref, lambda b: b.drop(n - 2, 1))                  # an edge class through a channel without a node: its very bits
    sub = lambda a, s: None if a is None else a[s]               # noqa: E731
    step(dspfx, torch, bank, ref, x[:NF], n, tile, "the clean block", key=sub(k, slice(0, NF)))
    for f in range(NF, 2 * NF):
        step(dspfx, torch, bank, ref, x[f:f + 1], n, tile, f"frame {f}", key=sub(k, slice(f, f + 1)))
        with np.errstate(invalid="ignore"):
            assert np.array_equal(bits(ref.level), bits(np.where(ref.on & (ref.envs[0] > 0), ref.envs[0], F(0))))
    poisoned = np.flatnonzero(np.isnan(ref.env))
    assert len(poisoned) >= 1 and all(tab[c] in ("nan", "inf_pair", "inf") for c in poisoned)
    got = step(dspfx, torch, bank, ref, x[2 * NF:], n, tile, "after the poison", inplace=True, key=sub(k, slice(2 * NF, 3 * NF)))
    assert not ref.level[poisoned].any() and (ref.reduction[poisoned] == 1).all(), "a NaN envelope: q = 1, no level"
    if as_key:
        assert np.isfinite(got).all(), "the key's NaN reaches the envelope, never the sample"
    for c in poisoned:
        both(bank, ref, lambda b: b.reset(int(c), 1))
    step(dspfx, torch, bank, ref, x[:NF], n, tile, "after the reset", key=sub(k, slice(0, NF)))
    assert np.isfinite(ref.env).all() and (ref.level[poisoned] > 0).all()
    bank.close()


# ---- 7. streams ------------------------------------------------------------------------------------------------------------
def test_runs_alternating_between_two_streams_equal_one_stream(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile = 256, 64
    bank, ref = pair(dspfx, n, tile, seed=70)
    x = noise(np.random.default_rng(71), 8 * NF, n)
    dxs = [device(dspfx, torch, x[i * NF:(i + 1) * NF], tile) for i in range(8)]
    dys = [torch.empty_like(d) for d in dxs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i in range(8):
        bank.run(dxs[i], NF, out=dys[i], stream=streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    got = np.concatenate([host(dspfx, d, NF, n, tile) for d in dys])
    assert np.array_equal(bits(got), bits(ref.run_blocks(x)))
    tables_equal(torch, bank, ref, "two streams")
    bank.close()


# ---- 8. full size ----------------------------------------------------------------------------------------------------------
def test_full_size(dspfx, torch_cuda):
    """2^20 channels x 128 frames, tiled 256, every channel present with its own sliders, noise in every channel; two alternating
    buffer pairs, device events, median of 20 after 5 warm-ups.  Asserted: the first and last 256 channels equal the restatement
    over two blocks from a reset; one run fits the 2.667 ms a 128-frame block lasts at 48 kHz; one run takes at most twice a gated
    Talkers run (the code as it stood before this bank: the same two block-units moved, the same recurrence) on the same buffers,
    timed here -- room for the one division per sample, a guard against a spill or a scalarised path, not a target.  Printed:
    milliseconds, the fraction of 8 TB/s on the run's own bytes, the ratio to the talker run and to a flat copy.
    Not measured here: a keyed run at full size and partly present banks (tools/dynamics_rate.py times both), the scalar path."""
    torch = torch_cuda
    n, nf, tile = 1 << 20, 128, 256
    gen = torch.Generator(device="cuda").manual_seed(8)
    xs = [torch.rand(nf * n, dtype=torch.float32, device="cuda", generator=gen) * 2 - 1 for _ in range(2)]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]

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

    assert dspfx.dynamics_plan(n) == 29 * n
    kw = sliders(np.random.default_rng(80), n)
    bank = dspfx.ChannelDynamics(n, tile_channels=tile, max_frames=nf)
    bank.set(**kw)
    t_dyn = timed(lambda i: bank.run(xs[i % 2], nf, out=ys[i % 2]))
    assert float(bank.reductions().max()) <= 1.0 and float((bank.reductions() < 1).float().mean()) > 0.5
    # the two ends against the restatement: a tile is 256 channels, nf * 256 contiguous floats
    ends = np.r_[0:256, n - 256:n]
    ref = R.ChannelDynamics(512)
    assert ref.set(**{k: v[ends] for k, v in kw.items()})
    bank.reset()
    span = nf * tile
    for i in range(2):
        bank.run(xs[i], nf, out=ys[i])
        torch.cuda.synchronize()
        blk = np.concatenate([xs[i][:span].cpu().numpy().reshape(nf, tile), xs[i][-span:].cpu().numpy().reshape(nf, tile)], axis=1)
        got = np.concatenate([ys[i][:span].cpu().numpy().reshape(nf, tile), ys[i][-span:].cpu().numpy().reshape(nf, tile)], axis=1)
        assert np.array_equal(bits(got), bits(ref.run(blk))), f"block {i}"
        assert np.array_equal(bits(bank.levels().cpu().numpy()[ends]), bits(ref.level))
        assert np.array_equal(bits(bank.reductions().cpu().numpy()[ends]), bits(ref.reduction))
    bank.close()
    talk = dspfx.Talkers(n, group_size=256, top=3, tile_channels=tile, max_frames=nf)
    talk.set_detector(48.0, 24000.0)
    t_talk = timed(lambda i: talk.run(xs[i % 2], nf, out=ys[i % 2]))
    talk.close()
    t_copy = timed(lambda i: ys[i % 2].copy_(xs[i % 2]))
    unit = nf * n * 4
    print(f"full size dynamics, one box, one run: {t_dyn:.4f} ms ({2 * unit / t_dyn / 1e9 / 8.0:.3f} of 8 TB/s on {2 * unit / 2**20:.0f} MiB), "
          f"gated Talkers run {t_talk:.4f} ms (dynamics x {t_dyn / t_talk:.3f}), flat copy of the same bytes {t_copy:.4f} ms "
          f"(dynamics x {t_dyn / t_copy:.3f})")
    assert t_dyn * 1e-3 <= 128 / 48000, t_dyn
    assert t_dyn <= 2 * t_talk, (t_dyn, t_talk)
