"""The channel-shaper bank on the GPU (dspfx_shapers_*, through the Python class): per-channel Distort, Overdrive and Chebyshev.
A channel's output is compared bit for bit with Engine([that node], link_flags=0) -- one engine run per distinct setting, made
once per module and shared -- and, through shapers_ref (one oracle node per channel), with the oracle at the bars
tests/test_gpu_parity.py holds the engine to.  Where the expectation is a NaN (Fuzz over a block it cannot normalise, NaN samples)
the bank must give a NaN; its sign and payload are not compared (edge_values.same_bits_or_nan).  Out-of-place outputs start as
NaN everywhere, so every sample is shown to be written."""
import ctypes as C
import threading

import numpy as np
import pytest

import edge_values as E
import oracle as O
import shapers_ref as R
from chains import ulp_diff
from test_gpu_parity import LIBM_COMPOSITE_ULP, LIBM_ULP

pytestmark = pytest.mark.gpu

NF = 128
F = np.float32
SHAPES = [(64, 0), (256, 64), (70, 0), (1, 0)]                   # vector lanes; tiled; scalar accesses and a ragged last workgroup; one channel
THREE = [(64, 0), (256, 64), (70, 0)]
TWO = [(256, 64), (70, 0)]
FRAMES = [1, 37, 128]
EDGES = FRAMES + [4, 8, 9]                                       # the frame loop's boundaries with 4 or 8 rows a chunk: one chunk, two, chunks and a row
NX = 256                                                         # the channels of the shared input and of the engines that give the expectations
FUZZ = 4
LEVELS = (0.0, 0.0009, 0.001, 1.0, 3.0, 30.0)
OVERDRIVES = ((5.0, 0.7, 0.9), (5.0, 0.7, 0.0009), (0.0, 0.0, 0.0))                 # test_overdrive_chebyshev's settings
CHEBYSHEVS = ((4.0, 0.0), (2.0, 7.5), (0.0, 0.0))
# a setting: ("d", level, mode) | ("o", boost, drive, level) | ("c", level_pos, level_neg) | None
UNIFORM = [("d", lv, m) for m in range(9) for lv in LEVELS] + [("o",) + s for s in OVERDRIVES] + [("c",) + s for s in CHEBYSHEVS]
MIX_LEVELS = (0.0009, 1.0, 3.0, 30.0)
MIX_OVERDRIVES = ((5.0, 0.7, 0.9), (5.0, 0.7, 0.0009), (30.0, 1.0, 1.0))
MIX_CHEBYSHEVS = ((4.0, 0.0), (2.0, 7.5), (0.5, 0.5))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_X = {}


def noise_x(nf=2 * NF):
    """noise_block * 2.5 with the fixed first values of test_distort_arithmetic_modes: [2 * 128][NX], left unchanged"""
    if "x" not in _X:
        x = O.noise(0x5EED0001, np.arange(NX), np.arange(2 * NF)) * F(2.5)
        x[0, :10] = [0, -0.0, 0.25, -0.25, 0.5, -0.5, 1, -1, 2, -2]
        x.setflags(write=False)
        _X["x"] = x
    return _X["x"][:nf]


def node_of(dspfx, s):
    return dspfx.Distort(s[1], s[2]) if s[0] == "d" else dspfx.Overdrive(*s[1:]) if s[0] == "o" else dspfx.Chebyshev(*s[1:])


def engine_run(dspfx, torch, s, x):
    """Engine([the node of setting s], link_flags=0) over x, 128 frames at a time"""
    eng = dspfx.Engine(x.shape[1], NF, link_flags=0)
    eng.set_chain([node_of(dspfx, s)])
    y = np.empty_like(x)
    for f0 in range(0, len(x), NF):
        dx = torch.from_numpy(x[f0:f0 + NF].copy()).cuda()
        dy = torch.full_like(dx, float("nan"))
        eng.process(dx, out=dy, n_frames=len(dx))
        torch.cuda.synchronize()
        y[f0:f0 + NF] = dy.cpu().numpy()
    eng.close()
    return y


_ENGINE = {}


def engine_ref(dspfx, torch, s):
    """the engine's output for setting s on noise_x(), [256][NX]: computed once, shared, left unchanged.  A pointwise kind's row f
    is what any n_frames > f gives; Fuzz is per 128-frame block"""
    if s not in _ENGINE:
        y = engine_run(dspfx, torch, s, noise_x())
        y.setflags(write=False)
        _ENGINE[s] = y
    return _ENGINE[s]


def expected(dspfx, torch, settings, nf, cols=None):
    """[nf][len(settings)]: channel c as the engine of its own setting gives column cols[c] of noise_x (default: c); no node: a copy"""
    cols = np.arange(len(settings)) % NX if cols is None else cols
    want = np.empty((nf, len(settings)), F)
    where = {}
    for c, s in enumerate(settings):
        where.setdefault(s, []).append(c)
    for s, cs in where.items():
        src = noise_x(nf) if s is None else engine_ref(dspfx, torch, s)[:nf]
        want.view(np.uint32)[:, cs] = src.view(np.uint32)[:, cols[cs]]
    return want


def store(b, settings, first=0):
    """the settings onto a bank or its restatement: consecutive channels of one family in one store"""
    c, n = 0, len(settings)
    while c < n:
        fam = None if settings[c] is None else settings[c][0]
        e = c
        while e < n and (None if settings[e] is None else settings[e][0]) == fam:
            e += 1
        run = settings[c:e]
        col = lambda k: np.asarray([s[k] for s in run], F)       # noqa: E731
        if fam is None:
            ok = b.drop(first + c, e - c)
        elif fam == "d":
            ok = b.set_distort(col(1), np.asarray([s[2] for s in run], np.uint32), first_channel=first + c)
        elif fam == "o":
            ok = b.set_overdrive(col(1), col(2), col(3), first_channel=first + c)
        else:
            ok = b.set_chebyshev(col(1), col(2), first_channel=first + c)
        assert ok is not False
        c = e


def mixed(n, nf, seed):
    """channel c gets kind c % 13 -- the nine Distort modes (Fuzz only with whole 128-frame blocks, HardClip otherwise), Overdrive,
    Chebyshev, none, none: a lane's four channels hold four different kinds and every wave holds all of them; sliders from small sets"""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        k = c % 13
        if k < 9:
            mode = k if k != FUZZ or nf % NF == 0 else 0
            out.append(("d", float(rng.choice(MIX_LEVELS if mode != FUZZ else (1.0, 3.0, 30.0))), mode))
        elif k == 9:
            out.append(("o",) + MIX_OVERDRIVES[rng.integers(3)])
        elif k == 10:
            out.append(("c",) + MIX_CHEBYSHEVS[rng.integers(3)])
        else:
            out.append(None)
    return out


def device(dspfx, torch, x, tile):
    return torch.from_numpy(dspfx.to_layout(np.ascontiguousarray(x), tile).reshape(-1).copy()).cuda()


def host(dspfx, t, nf, n, tile):
    return dspfx.from_layout(t.cpu().numpy(), nf, n, tile)


def run(dspfx, torch, bank, x, n, tile, inplace=False):
    dx = device(dspfx, torch, x, tile)
    dy = bank.run(dx, len(x), out=dx if inplace else torch.full_like(dx, float("nan")))
    torch.cuda.synchronize()
    return host(dspfx, dy, len(x), n, tile)


def tables(settings):
    kinds = [R.NONE if s is None else {"d": R.DISTORT, "o": R.OVERDRIVE, "c": R.CHEBYSHEV}[s[0]] for s in settings]
    modes = [s[2] if s is not None and s[0] == "d" else R.NONE for s in settings]
    return np.asarray(kinds, np.uint32), np.asarray(modes, np.uint32)


# ---- 1. a fresh bank -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", EDGES)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_a_fresh_bank_copies(dspfx, torch_cuda, n, tile, nf):
    bank = dspfx.ChannelShapers(n, tile_channels=tile, max_frames=NF)
    x = noise_x(nf)[:, :n]
    assert np.array_equal(bits(run(dspfx, torch_cuda, bank, x, n, tile)), bits(x))
    assert not bank.present().any() and (bank.kinds() == dspfx.SHAPERS_NONE).all() and (bank.modes() == dspfx.SHAPERS_NONE).all()
    assert not bank.sliders().any() and bank.sliders().shape == (n, 3)
    bank.close()


# ---- 2. one setting everywhere equals that engine ------------------------------------------------------------------------
@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_one_setting_everywhere_equals_that_engine(dspfx, torch_cuda, n, tile, nf):
    """every Distort mode at levels 0, 0.0009, 0.001, 1, 3, 30 (Fuzz with the whole block of 128 frames), the Overdrive and
    Chebyshev settings of test_overdrive_chebyshev; the stores follow each other on one bank, so every family replaces another"""
    torch = torch_cuda
    bank = dspfx.ChannelShapers(n, tile_channels=tile, max_frames=NF)
    x = noise_x(nf)[:, :n]
    for s in UNIFORM:
        if s[0] == "d" and s[2] == FUZZ and nf % NF:
            continue
        store(bank, [s] * n)
        got = run(dspfx, torch, bank, x, n, tile)
        E.same_bits_or_nan(got, engine_ref(dspfx, torch, s)[:nf, :n], None, f"N={n} tile={tile} nf={nf} {s}")
        bypass = (s[0] == "d" and s[2] != FUZZ and s[1] < 0.001) or (s[0] == "o" and s[3] < 0.001) or s == ("c", 0.0, 0.0)
        if bypass:
            assert np.array_equal(bits(got), bits(x)), f"{s}: the bypass keeps the sample's bits"
        k, m = tables([s])
        assert (bank.kinds() == k[0]).all() and (bank.modes() == m[0]).all() and bank.present().all()
    bank.close()


# ---- 3. a mixed bank -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("n,tile", SHAPES + [(13 * 256, 256)])
def test_mixed_bank_every_channel_equals_the_engine_of_its_own_setting(dspfx, torch_cuda, n, tile, nf):
    """kind c % 13; then the same settings sorted by kind, so that whole waves share one (at N = 13 * 256 each of the 13 spans of 256
    channels is one wave of the four-channel kernel): the same bits per channel"""
    torch = torch_cuda
    settings = mixed(n, nf, 30 + n)
    cols = np.arange(n) % NX
    x = noise_x(nf)[:, cols]
    want = expected(dspfx, torch, settings, nf)
    bank = dspfx.ChannelShapers(n, tile_channels=tile, max_frames=NF)
    store(bank, settings)
    k, m = tables(settings)
    assert np.array_equal(bank.kinds(), k) and np.array_equal(bank.modes(), m) and np.array_equal(bank.present(), (k != R.NONE).astype(np.uint32))
    E.same_bits_or_nan(run(dspfx, torch, bank, x, n, tile), want, None, f"N={n} tile={tile} nf={nf} interleaved")
    bank.close()
    order = np.argsort(k.astype(np.int64) * 16 + np.where(m == R.NONE, 15, m), kind="stable")
    srt = dspfx.ChannelShapers(n, tile_channels=tile, max_frames=NF)
    store(srt, [settings[c] for c in order])
    got = run(dspfx, torch, srt, x[:, order], n, tile)
    E.same_bits_or_nan(got, want[:, order], None, f"N={n} tile={tile} nf={nf} sorted")
    srt.close()


# ---- 4. neighbours ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", THREE)
def test_a_channels_bits_do_not_depend_on_its_neighbours(dspfx, torch_cuda, n, tile):
    """the kept channels (one of each lane's four, and the last) get the same settings and samples in two banks; every other
    channel differs in kind, in sliders, or carries NaN samples"""
    torch = torch_cuda
    keep = np.zeros(n, bool)
    keep[(np.arange(n) % 4) == (np.arange(n) // 4) % 4] = True
    keep[n - 1] = True
    sa = mixed(n, NF, 40 + n)
    other = mixed(n + 5, NF, 41 + n)[5:]                          # the kinds shifted by five, other sliders
    sb = [sa[c] if keep[c] else other[c] for c in range(n)]
    x = noise_x(NF)[:, :n]
    x2 = np.where(keep, x, noise_x(2 * NF)[NF:, :n] * F(5))
    x2[:, np.flatnonzero(~keep)[::3]] = np.nan
    a = dspfx.ChannelShapers(n, tile_channels=tile, max_frames=NF)
    b = dspfx.ChannelShapers(n, tile_channels=tile, max_frames=NF)
    store(a, sa)
    store(b, sb)
    ya = run(dspfx, torch, a, x, n, tile)
    yb = run(dspfx, torch, b, x2, n, tile)
    E.same_bits_or_nan(ya, expected(dspfx, torch, sa, NF), None, "bank a")
    assert np.array_equal(bits(ya[:, keep]), bits(yb[:, keep]))
    assert not np.array_equal(bits(ya[:, ~keep]), bits(yb[:, ~keep]))
    a.close()
    b.close()


# ---- 5. in place -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", EDGES)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_in_place_equals_out_of_place(dspfx, torch_cuda, n, tile, nf):
    torch = torch_cuda
    bank = dspfx.ChannelShapers(n, tile_channels=tile, max_frames=NF)
    store(bank, mixed(n, nf, 50 + n))
    x = noise_x(nf)[:, :n]
    out = run(dspfx, torch, bank, x, n, tile)
    assert np.array_equal(bits(run(dspfx, torch, bank, x, n, tile, inplace=True)), bits(out))
    assert not np.isnan(out[:, [c for c in range(n) if c % 13 != FUZZ]]).any()
    bank.close()


# ---- 6. Fuzz ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [128, 256])
@pytest.mark.parametrize("n,tile", THREE)
def test_fuzz_channels_among_other_kinds(dspfx, torch_cuda, n, tile, nf):
    """every third channel carries Fuzz (three levels), the next another kind, the next none; one Fuzz channel is all zeros: NaN
    in that channel and nowhere else.  n_frames = 64 is refused while a Fuzz channel exists, accepted after its drop, and accepted
    on a bank that never had one"""
    torch = torch_cuda
    others = [s for s in mixed(3 * n, 1, 60 + n) if s is not None]
    settings = [("d", (1.0, 3.0, 30.0)[(c // 3) % 3], FUZZ) if c % 3 == 0 else others[c] if c % 3 == 1 else None for c in range(n)]
    silent = 3 * ((n // 3) // 2)
    x = noise_x(nf)[:, :n].copy()
    x[:, silent] = 0.0
    want = expected(dspfx, torch, settings, nf)
    want[:, silent] = np.nan
    bank = dspfx.ChannelShapers(n, tile_channels=tile, max_frames=256)
    store(bank, settings)
    for inplace in (False, True):
        got = run(dspfx, torch, bank, x, n, tile, inplace=inplace)
        E.same_bits_or_nan(got, want, None, f"N={n} tile={tile} nf={nf} in place {inplace}")
        assert np.isnan(got[:, silent]).all() and not np.isnan(np.delete(got, silent, axis=1)).any()
    with pytest.raises(dspfx.DspfxError) as e:
        bank.run(device(dspfx, torch, x[:64], tile), 64)
    assert e.value.status == -1 and "128" in str(e.value) and "Fuzz" in str(e.value), str(e.value)
    for c in range(0, n, 3):
        bank.drop(c, 1)
    got = run(dspfx, torch, bank, x[:64], n, tile)
    fz = np.arange(n) % 3 == 0
    assert np.array_equal(bits(got[:, fz]), bits(x[:64, fz])), "dropped: a copy again"
    E.same_bits_or_nan(got[:, ~fz], want[:64, ~fz], None, "the others after the drop")
    bank.close()
    plain = dspfx.ChannelShapers(n, tile_channels=tile, max_frames=256)
    store(plain, others[:n])
    run(dspfx, torch, plain, x[:64], n, tile)
    plain.close()


# ---- 7. store order --------------------------------------------------------------------------------------------------------
def test_a_store_after_a_submitted_run_does_not_change_it_and_a_new_family_starts_from_the_defaults(dspfx, torch_cuda):
    """nothing waits between the calls; everything is read at the end"""
    torch = torch_cuda
    n, tile = 256, 64
    x = noise_x(NF)[:, :n]
    old, new, cheb = ("d", 3.0, 1), ("o", 5.0, 0.7, 0.9), ("c", 2.0, 0.0)
    bank = dspfx.ChannelShapers(n, tile_channels=tile, max_frames=NF)
    dx = device(dspfx, torch, x, tile)
    dys = [torch.full_like(dx, float("nan")) for _ in range(4)]
    torch.cuda.synchronize()
    store(bank, [old] * n)
    bank.run(dx, NF, out=dys[0])
    store(bank, [new] * n)
    bank.run(dx, NF, out=dys[1])
    bank.set_overdrive(boost=30.0, first_channel=0, count=64)            # the same family: drive and level are kept
    bank.drop(64, 64)
    bank.set_chebyshev(level_pos=2.0, first_channel=64, count=64)        # set -> drop -> set of another family: level_neg is the default
    bank.set_chebyshev(level_pos=2.0, first_channel=128, count=64)       # ... and without the drop: replaced, the defaults too
    bank.run(dx, NF, out=dys[2])
    bank.set_distort(mode=dspfx.SQUARE, first_channel=192, count=64)     # replaced by a Distort: level 0, a bypass
    bank.run(dx, NF, out=dys[3])
    torch.cuda.synchronize()
    got = [host(dspfx, d, NF, n, tile) for d in dys]
    ref = lambda s: engine_ref(dspfx, torch, s)[:NF, :n]         # noqa: E731
    assert np.array_equal(bits(got[0]), bits(ref(old))) and np.array_equal(bits(got[1]), bits(ref(new)))
    want = np.concatenate([ref(("o", 30.0, 0.7, 0.9))[:, :64], ref(cheb)[:, 64:192], ref(new)[:, 192:]], axis=1)
    assert np.array_equal(bits(got[2]), bits(want))
    assert np.array_equal(bits(got[3][:, :192]), bits(want[:, :192])) and np.array_equal(bits(got[3][:, 192:]), bits(x[:, 192:]))
    sl = bank.sliders()
    assert [list(sl[c]) for c in (0, 64, 128, 192)] == [[30.0, F(0.7), F(0.9)], [2.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    assert list(bank.kinds()[[0, 64, 128, 192]]) == [R.OVERDRIVE, R.CHEBYSHEV, R.CHEBYSHEV, R.DISTORT] and bank.modes()[192] == dspfx.SQUARE
    bank.close()


def test_a_refused_store_changes_nothing(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile = 70, 0
    settings = mixed(n, NF, 71)
    bank, ref = dspfx.ChannelShapers(n, tile_channels=tile, max_frames=NF), R.ChannelShapers(n)
    store(bank, settings)
    store(ref, settings)
    x = noise_x(NF)[:, :n]
    before = run(dspfx, torch, bank, x, n, tile)
    bad = [(lambda b: b.set_distort(1.0, 9), "mode"), (lambda b: b.set_distort(1.0, np.r_[np.zeros(n - 1, np.uint32), 77]), "mode"),
           (lambda b: b.set_distort(1.0, 1, first_channel=n - 1, count=2), "channels"), (lambda b: b.set_overdrive(1.0, first_channel=n + 1, count=0), "channels"),
           (lambda b: b.set_chebyshev(1.0, first_channel=0, count=n + 1), "channels"), (lambda b: b.drop(n, 1), "channels")]
    for call, word in bad:
        with pytest.raises(dspfx.DspfxError) as e:
            call(bank)
        assert e.value.status == -1 and word in str(e.value) and "shapers" in str(e.value), str(e.value)
        assert call(ref) is False
    with pytest.raises(dspfx.DspfxError):
        bank.present(1, n)
    with pytest.raises(dspfx.DspfxError):
        bank.run(device(dspfx, torch, noise_x(2 * NF)[:, :n], tile), 2 * NF)
    k, m = tables(settings)
    assert np.array_equal(bank.kinds(), k) and np.array_equal(bank.modes(), m) and np.array_equal(bank.kinds(), ref.kind) and np.array_equal(bank.modes(), ref.mode)
    assert np.array_equal(bits(bank.sliders()), bits(ref.p))
    E.same_bits_or_nan(run(dspfx, torch, bank, x, n, tile), before, None, "after the refused stores")
    store(bank, [("d", float("nan"), 1), ("d", float("inf"), 0), ("o", -1.0, 2.0, float("nan")), ("c", float("nan"), -3.0)])       # taken as given
    got = run(dspfx, torch, bank, x, n, tile)
    assert np.isnan(got[:, 0]).all() and np.isnan(bank.sliders()[0, 0]) and bank.sliders()[3, 1] == -3.0
    bank.close()


def test_a_thread_storing_whole_range_settings_while_blocks_are_submitted(dspfx, torch_cuda):
    """every block equals the all-old or the all-new expectation: a store is whole"""
    torch = torch_cuda
    n, tile, runs = 256, 64, 60
    old, new = ("d", 3.0, 2), ("o", 5.0, 0.7, 0.9)
    x = noise_x(NF)[:, :n]
    wants = [bits(engine_ref(dspfx, torch, s)[:NF, :n]) for s in (old, new)]
    bank = dspfx.ChannelShapers(n, tile_channels=tile, max_frames=NF)
    store(bank, [old] * n)
    dx = device(dspfx, torch, x, tile)
    dys = [torch.full_like(dx, float("nan")) for _ in range(runs)]
    torch.cuda.synchronize()
    done, errors, made = threading.Event(), [], [0]

    def storer():
        try:
            while not done.is_set() or made[0] < 20:
                store(bank, [(new, old)[made[0] % 2]] * n)
                made[0] += 1
        except Exception as e:                                   # noqa: BLE001
            errors.append(e)

    t = threading.Thread(target=storer)
    t.start()
    for i in range(runs):
        bank.run(dx, NF, out=dys[i])
    done.set()
    t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for i in range(runs):
        got = bits(host(dspfx, dys[i], NF, n, tile))
        which = [np.array_equal(got, w) for w in wants]
        assert any(which), f"run {i} is neither all old nor all new"
    bank.close()


def test_each_run_goes_by_the_tables_it_drained(dspfx, torch_cuda):
    """a Fuzz set is queued, a run submitted, the drop queued, a run submitted, and nothing waits in between: the first run has
    its Fuzz pass and wants whole blocks, the second is a copy and takes 64 frames.  The drop is in the host tables before the
    first run has executed; the decision is not made by them"""
    torch = torch_cuda
    n, tile = 256, 64
    x = noise_x(NF)[:, :n]
    bank = dspfx.ChannelShapers(n, tile_channels=tile, max_frames=NF)
    dx = device(dspfx, torch, x, tile)
    dys = [torch.full_like(dx, float("nan")) for _ in range(2)]
    dx64 = device(dspfx, torch, x[:64], tile)
    dy64 = torch.full_like(dx64, float("nan"))
    torch.cuda.synchronize()
    bank.set_distort(3.0, dspfx.FUZZ, first_channel=8, count=100)
    bank.run(dx, NF, out=dys[0])
    bank.drop(8, 100)
    assert not bank.present().any(), "the host tables already show the drop"
    bank.run(dx, NF, out=dys[1])
    bank.set_distort(3.0, dspfx.FUZZ, first_channel=8, count=1)
    bank.drop(8, 1)
    bank.run(dx64, 64, out=dy64)                                 # queued set and drop both drained: no Fuzz channel, any n_frames
    bank.set_distort(3.0, dspfx.FUZZ, first_channel=200, count=1)
    with pytest.raises(dspfx.DspfxError):
        bank.run(dx64, 64, out=dy64)
    torch.cuda.synchronize()
    fz = engine_ref(dspfx, torch, ("d", 3.0, FUZZ))[:NF, :n]
    want = np.concatenate([x[:, :8], fz[:, 8:108], x[:, 108:]], axis=1)
    assert np.array_equal(bits(host(dspfx, dys[0], NF, n, tile)), bits(want))
    assert np.array_equal(bits(host(dspfx, dys[1], NF, n, tile)), bits(x))
    assert np.array_equal(bits(host(dspfx, dy64, 64, n, tile)), bits(x[:64]))
    bank.close()


# ---- 8. edge values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", TWO)
def test_edge_values_through_every_kind(dspfx, torch_cuda, n, tile):
    """NaN, both infinities, signed zeros, subnormals, the clip points and the fast f64 functions' switch points, each class in
    a channel of its own, through a bank of each kind against the engine of that kind on the same block"""
    torch = torch_cuda
    x, tab = E.edge_block(n, NF)
    bank = dspfx.ChannelShapers(n, tile_channels=tile, max_frames=NF)
    for s in [("d", 3.0, m) for m in range(9)] + [("o", 5.0, 0.7, 0.9), ("c", 2.0, 7.5), ("c", 4.0, 0.0)]:
        store(bank, [s] * n)
        got = run(dspfx, torch, bank, x, n, tile)
        E.same_bits_or_nan(got, engine_run(dspfx, torch, s, x), tab, f"N={n} {s}")
    bank.drop()
    assert np.array_equal(bits(run(dspfx, torch, bank, x, n, tile)), bits(x)), "no node: every edge value's very bits"
    bank.close()


# ---- 9. the oracle ---------------------------------------------------------------------------------------------------------
def test_against_the_oracle_through_the_restatement(dspfx, torch_cuda):
    """a mixed bank and shapers_ref with the same stores: at most 1 ulp for the arithmetic modes, LIBM_ULP for Tanh / Sin / Atan,
    LIBM_COMPOSITE_ULP for Overdrive and Chebyshev, a copy bit for bit"""
    torch = torch_cuda
    n, tile = 256, 64
    settings = mixed(n, 1, 90)                                   # (no Fuzz here: it has its own bars below)
    bank, ref = dspfx.ChannelShapers(n, tile_channels=tile, max_frames=NF), R.ChannelShapers(n)
    store(bank, settings)
    store(ref, settings)
    assert np.array_equal(bank.kinds(), ref.kind) and np.array_equal(bank.modes(), ref.mode) and np.array_equal(bits(bank.sliders()), bits(ref.p))
    x = noise_x(NF)[:, :n]
    got, want = run(dspfx, torch, bank, x, n, tile), ref.run(x)
    d = ulp_diff(got, want)
    for c, s in enumerate(settings):
        if s is None:
            assert np.array_equal(bits(got[:, c]), bits(want[:, c])), c
            continue
        bar = LIBM_COMPOSITE_ULP if s[0] != "d" else LIBM_ULP.get(s[2], 1)
        print(f"channel {c} {s}: {d[:, c].max()} ulp (bar {bar})")
        assert d[:, c].max() <= bar, (c, s, int(d[:, c].max()))
    bank.close()


def test_fuzz_against_the_oracle_through_the_restatement(dspfx, torch_cuda):
    """test_fuzz's input and level: within 4e-6 of the block's peak, under 2 % of the samples beyond 1 ulp"""
    torch = torch_cuda
    n = 100
    x = O.noise(0x5EED0001, np.arange(n), np.arange(256))
    bank, ref = dspfx.ChannelShapers(n, max_frames=256), R.ChannelShapers(n)
    for b in (bank, ref):
        assert b.set_distort(3.0, dspfx.FUZZ) is not False
    got, want = run(dspfx, torch, bank, x, n, 0), ref.run(x)
    err, beyond = np.abs(got - want).max() / np.abs(want).max(), (ulp_diff(got, want) > 1).mean()
    print(f"Fuzz against the oracle: {err:.3e} of the peak (bar 4e-6), {100 * beyond:.3f} % beyond 1 ulp (bar 2 %)")
    assert err <= 4e-6
    assert beyond < 0.02
    bank.close()


# ---- 10. full size ---------------------------------------------------------------------------------------------------------
def test_full_size(dspfx, torch_cuda):
    """2^20 channels x 128 frames, tiled 256, noise in every channel; two alternating buffer pairs, device events, median of 20
    after 5 warm-ups.  Asserted: a SoftClip-everywhere bank and a Tanh-everywhere bank each take at most twice their
    Engine([Distort]) on the same buffers, timed here (twice is the margin every bank here gets over its engine), and equal it bit
    for bit; a bank clustered by spans of 256 channels over all pointwise kinds fits the 2.667 ms a 128-frame block lasts at
    48 kHz.  Printed, not asserted: the fully interleaved bank (c % 13) and a bank with 1 % Fuzz channels; milliseconds, the
    fraction of 8 TB/s on the bank's two block-units, a flat copy of the same bytes."""
    torch = torch_cuda
    n, nf, tile = 1 << 20, 128, 256
    gen = torch.Generator(device="cuda").manual_seed(8)
    xs = [torch.rand(nf * n, dtype=torch.float32, device="cuda", generator=gen) * 5 - 2.5 for _ in range(2)]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    unit = nf * n * 4

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

    assert dspfx.shapers_plan(n) == 13 * n
    bank = dspfx.ChannelShapers(n, tile_channels=tile, max_frames=nf)
    times = {}
    for name, mode in (("SoftClip", dspfx.SOFT_CLIP), ("Tanh", dspfx.TANH)):
        bank.set_distort(3.0, mode)
        t_bank = timed(lambda i: bank.run(xs[i % 2], nf, out=ys[i % 2]))
        torch.cuda.synchronize()
        mine = ys[1].clone()
        eng = dspfx.Engine(n, nf, link_flags=0, tile_channels=tile)
        eng.set_chain([dspfx.Distort(3.0, mode)])
        t_eng = timed(lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=nf))
        torch.cuda.synchronize()
        assert torch.equal(mine.view(torch.int32), ys[1].view(torch.int32)), f"{name}: the bank's bits are the engine's"
        eng.close()
        times[name] = (t_bank, t_eng)
    # clustered: span s of 256 channels carries pointwise kind s % 10 (the eight Distort modes but Fuzz, Overdrive, Chebyshev)
    span = np.arange(n) // 256
    pointwise = [m for m in range(9) if m != FUZZ]
    bank.set_distort(3.0, np.asarray(pointwise, np.uint32)[span % 8])
    for s in range(n // 256):
        if s % 10 == 8:
            bank.set_overdrive(5.0, 0.7, 0.9, first_channel=s * 256, count=256)
        elif s % 10 == 9:
            bank.set_chebyshev(2.0, 7.5, first_channel=s * 256, count=256)
    t_cluster = timed(lambda i: bank.run(xs[i % 2], nf, out=ys[i % 2]))
    # 1 % Fuzz among SoftClip
    bank.set_distort(3.0, np.where(np.arange(n) % 100 == 0, FUZZ, dspfx.SOFT_CLIP).astype(np.uint32))
    t_fuzz = timed(lambda i: bank.run(xs[i % 2], nf, out=ys[i % 2]))
    # fully interleaved, c % 13: the Distort modes in one store, then Overdrive, Chebyshev and the two without a node channel by
    # channel, a run now and then so that the staging buffers of the small stores come back
    # (240 000 stores: through the C entry points on four floats made once, not through 240 000 numpy arrays)
    bank.set_distort(3.0, (np.arange(n) % 13 % 9).astype(np.uint32))
    v = np.asarray([5.0, 0.7, 0.9, 2.0, 7.5], F)
    p = [v[i:].ctypes.data_as(C.POINTER(C.c_float)) for i in range(5)]
    L, h = bank.L, bank.h
    for c0 in range(0, n, 13):
        if c0 + 9 < n:
            assert L.dspfx_shapers_set_overdrive(h, p[0], p[1], p[2], c0 + 9, 1) == 0
        if c0 + 10 < n:
            assert L.dspfx_shapers_set_chebyshev(h, p[3], p[4], c0 + 10, 1) == 0
        if c0 + 11 < n:
            assert L.dspfx_shapers_drop(h, c0 + 11, min(2, n - c0 - 11)) == 0
        if (c0 // 13) % 1024 == 1023:
            bank.run(xs[0], nf, out=ys[0])
            torch.cuda.synchronize()
    k = bank.kinds(0, 26)
    assert list(k[9:13]) == [R.OVERDRIVE, R.CHEBYSHEV, R.NONE, R.NONE] and list(bank.modes(13, 9)) == list(range(9))
    t_mixed = timed(lambda i: bank.run(xs[i % 2], nf, out=ys[i % 2]))
    bank.close()
    t_copy = timed(lambda i: ys[i % 2].copy_(xs[i % 2]))
    frac = lambda t: 2 * unit / t / 1e9 / 8.0                    # noqa: E731
    print(f"full size shapers, one box, one run, {2 * unit / 2**20:.0f} MiB: "
          + ", ".join(f"{name} {tb:.4f} ms ({frac(tb):.3f} of 8 TB/s; Engine([Distort]) {te:.4f} ms, bank x {tb / te:.3f})" for name, (tb, te) in times.items())
          + f", clustered by spans of 256 over the pointwise kinds {t_cluster:.4f} ms ({frac(t_cluster):.3f}), interleaved c % 13 {t_mixed:.4f} ms "
          f"({frac(t_mixed):.3f}), 1 % Fuzz among SoftClip {t_fuzz:.4f} ms ({frac(t_fuzz):.3f}), flat copy of the same bytes {t_copy:.4f} ms")
    for name, (tb, te) in times.items():
        assert tb <= 2 * te, (name, tb, te)
    assert t_cluster * 1e-3 <= 128 / 48000, t_cluster
