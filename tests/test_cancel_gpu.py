"""The channel-canceller bank on the GPU (dspfx_cancel_*, through the Python class): per-channel adaptive (NLMS) FIR filters whose
taps the device updates every frame.  A channel's output, its weights and its levels are compared BIT FOR BIT with cancel_ref
(the rule of include/dspfx.h in numpy float32, which tests/test_cancel_cpu.py holds to a model of the kernel's lane) after every
run.  The tap counts 1 2 3 4 5 8 15 16 17 31 32 33 64 stand on both sides of every multiple of 4 and of the kernel's tap classes,
and every sequence runs 37 + 128 + 91 + 128 frames.  Out-of-place outputs start as NaN everywhere, so every sample is shown to be
written."""
import ctypes as C
import threading

import numpy as np
import pytest

import cancel_ref as R
import edge_values as E
import oracle as O

pytestmark = pytest.mark.gpu

NF = 128
F = np.float32
SHAPES = [(64, 0), (256, 64), (70, 0), (1, 0)]                   # a full wave; tiled, more than one wave; a ragged last wave; one channel
TWO = [(256, 64), (70, 0)]
CUTS = R.CUTS
NX = 256
LIST = R.T_LIST
MAX_TAPS = 64
MAX_DELAY = 100


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


bits = R.bits
_X = {}


def signals(nf=sum(CUTS)):
    """(mic, ref): noise of amplitude 1, [4 * 128][NX] each, made once, left unchanged"""
    if "x" not in _X:
        mic = O.noise(0x5EED0AEC, np.arange(NX), np.arange(4 * NF)).copy()
        far = O.noise(0x5EED0FA2, np.arange(NX), np.arange(4 * NF)).copy()
        mic[0, :10] = [0, -0.0, 0.25, -0.25, 0.5, -0.5, 1, -1, 2, -2]
        far[1, :10] = [0, -0.0, 0.25, -0.25, 0.5, -0.5, 1, -1, 2, -2]
        mic.setflags(write=False)
        far.setflags(write=False)
        _X["x"] = (mic, far)
    return _X["x"][0][:nf], _X["x"][1][:nf]


def device(dspfx, torch, x, tile):
    return torch.from_numpy(dspfx.to_layout(np.ascontiguousarray(x), tile).reshape(-1).copy()).cuda()


def host(dspfx, t, nf, n, tile):
    return dspfx.from_layout(t.cpu().numpy(), nf, n, tile)


def run(dspfx, torch, bank, mic, far, n, tile, inplace=False, stream=0):
    dm, dr = device(dspfx, torch, mic, tile), device(dspfx, torch, far, tile)
    out = dm if inplace else torch.full_like(dm, float("nan"))
    torch.cuda.synchronize()
    dy = bank.run(dm, len(mic), ref=dr, out=out, stream=stream)
    torch.cuda.synchronize()
    return host(dspfx, dy, len(mic), n, tile)


def state(torch, bank):
    torch.cuda.synchronize()
    return bank.weights().cpu().numpy(), bank.levels().cpu().numpy()


def agree(torch, bank, ref, got, want, what=""):
    """output, weights() and levels() are the restatement's bits, and the weights table is +0.0 in every row k >= T"""
    w, lev = state(torch, bank)
    assert np.array_equal(bits(got), bits(want)), (what, "out", np.argwhere(bits(got) != bits(want))[:4])
    assert np.array_equal(bits(w), bits(ref.weights())), (what, "weights", np.argwhere(bits(w) != bits(ref.weights()))[:4])
    assert np.array_equal(bits(lev), bits(ref.lev)), (what, "levels")
    dead = np.arange(w.shape[0])[:, None] >= bank.lengths()[None, :]
    assert not bits(w)[dead].any(), (what, "a weight in a row k >= T")


def both_cuts(dspfx, torch, bank, ref, mic, far, n, tile, cuts=CUTS, inplace=False, what=""):
    f0 = 0
    for k in cuts:
        got = run(dspfx, torch, bank, mic[f0:f0 + k], far[f0:f0 + k], n, tile, inplace=inplace)
        agree(torch, bank, ref, got, ref.run(mic[f0:f0 + k], far[f0:f0 + k]), (what, f0, k))
        f0 += k


def pair(dspfx, n, tile, max_frames=NF, **kw):
    return (dspfx.ChannelCancellers(n, max_taps=MAX_TAPS, max_delay=MAX_DELAY, tile_channels=tile, max_frames=max_frames, **kw),
            R.CancelRef(n, MAX_TAPS, MAX_DELAY))


def mixed(n):
    """channel c: T = LIST[c % 13], a delay, a mu and an eps of its own"""
    c = np.arange(n)
    return dict(taps=np.array(LIST)[c % 13], delay=(c * 5) % 38, mu=(F(0.125) * (1 + c % 5)).astype(F), eps=(F(1e-6) * (1 + c % 3)).astype(F))


def tables_agree(bank, ref):
    assert np.array_equal(bank.present(), ref.T > 0) and np.array_equal(bank.lengths(), ref.T) and np.array_equal(bank.delays(), ref.D)
    assert np.array_equal(bank.adapting(), ref.adapt) and np.array_equal(bits(bank.sliders()), bits(np.stack([ref.mu, ref.eps], axis=1)))


# ---- 1. a fresh bank -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [1, 37, 128])
@pytest.mark.parametrize("n,tile", SHAPES)
def test_a_fresh_bank_copies(dspfx, torch_cuda, n, tile, nf):
    bank, ref = pair(dspfx, n, tile)
    mic = signals(nf)[0][:, :n].copy()
    mic[0, 0] = np.float32(np.nan)
    far = np.full_like(mic, np.nan)
    for inplace in (False, True):
        got = run(dspfx, torch_cuda, bank, mic, far, n, tile, inplace=inplace)
        agree(torch_cuda, bank, ref, got, ref.run(mic, far))
        assert np.array_equal(bits(got), bits(mic))
    assert not bank.present().any() and not bank.lengths().any()
    bank.close()


# ---- 2. one T everywhere ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", LIST)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_one_tap_count_everywhere(dspfx, torch_cuda, n, tile, T):
    """every channel T taps, a delay of 3 and a mu of its own: the fast body over the whole blocks, the general body behind them"""
    bank, ref = pair(dspfx, n, tile)
    mu = (F(0.125) * (1 + np.arange(n) % 5)).astype(F)
    for k in (bank, ref):
        k.set(taps=T, delay=3, mu=mu)
    mic, far = signals()
    both_cuts(dspfx, torch_cuda, bank, ref, mic[:, :n], far[:, :n], n, tile, what=f"T={T}")
    tables_agree(bank, ref)
    bank.close()


# ---- 3. a mixed bank: the general body -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", SHAPES)
def test_mixed_bank_every_channel_equals_the_rule(dspfx, torch_cuda, n, tile):
    bank, ref = pair(dspfx, n, tile)
    for k in (bank, ref):
        k.set(**mixed(n))
    mic, far = signals()
    both_cuts(dspfx, torch_cuda, bank, ref, mic[:, :n], far[:, :n], n, tile)
    tables_agree(bank, ref)
    bank.close()


# ---- 4. the two bodies -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [32, 64])
@pytest.mark.parametrize("n,tile", SHAPES)
def test_the_fast_body_and_the_general_body_give_the_same_bits(dspfx, torch_cuda, n, tile, T):
    """T uniform with a delay per channel; the second bank is general_only.  Both equal the restatement after every run"""
    torch = torch_cuda
    mic, far = signals()
    delay = (np.arange(n) * 7) % (MAX_DELAY + 1)
    outs = []
    for general_only in (False, True):
        bank, ref = pair(dspfx, n, tile, general_only=general_only)
        for k in (bank, ref):
            k.set(taps=T, delay=delay)
        both_cuts(dspfx, torch, bank, ref, mic[:, :n], far[:, :n], n, tile, what=f"general_only={general_only}")
        outs.append(state(torch, bank))
        bank.close()
    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])) and np.array_equal(bits(outs[0][1]), bits(outs[1][1]))


# ---- 5. stores -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("n,tile", TWO)
def test_store_rules_on_the_device_follow_the_restatement(dspfx, torch_cuda, n, tile, uniform):
    """set to a shorter and a longer T, load, reset, drop then set, adapt toggled between runs, a new delay: the weights and the
    history are kept or cleared as the rule says.  uniform: one T everywhere (the fast body), else the mixed bank"""
    torch = torch_cuda
    bank, ref = pair(dspfx, n, tile)
    mic, far = signals()
    mic, far = mic[:, :n], far[:, :n]
    cfg = dict(taps=16, delay=2) if uniform else mixed(n)
    Ts = np.broadcast_to(np.asarray(cfg["taps"]), (n,))
    f0 = [0]

    def step(nf, what):
        a, b = f0[0], f0[0] + nf
        got = run(dspfx, torch, bank, mic[a:b], far[a:b], n, tile)
        agree(torch, bank, ref, got, ref.run(mic[a:b], far[a:b]), what)
        tables_agree(bank, ref)
        f0[0] = b

    for k in (bank, ref):
        k.set(**cfg)
    step(37, "new nodes")
    step(64, "second run")
    short, longer = np.maximum(1, Ts // 2), np.minimum(MAX_TAPS, Ts + 3)
    for k in (bank, ref):
        k.set(taps=short)
    step(24, "a shorter T")
    for k in (bank, ref):
        k.set(taps=longer)
    step(40, "a longer T")
    rows = np.random.default_rng(5).uniform(-0.25, 0.25, (n, MAX_TAPS)).astype(F)
    if uniform:
        for k in (bank, ref):
            k.load(rows[:, :longer[0]])
            k.load(rows[0, :longer[0]], first_channel=n // 2)                   # one row for the upper half
    else:
        for c in range(n):
            for k in (bank, ref):
                k.load(rows[c, :longer[c]], first_channel=c, count=1)
    step(24, "load")
    for k in (bank, ref):
        k.set(adapt=False, first_channel=n // 3)
    step(24, "frozen from n / 3 on")
    for k in (bank, ref):
        k.set(adapt=np.arange(n) % 2 == 0)
    step(24, "every second channel adapting")
    for k in (bank, ref):
        k.reset(0, n // 2)
        k.set(delay=(np.arange(n) * 3) % (MAX_DELAY + 1), adapt=True)
    step(37, "reset of the lower half, a new delay everywhere")
    for k in (bank, ref):
        k.drop(n // 4, n // 2)
    step(16, "a drop")
    for k in (bank, ref):
        k.set(taps=8, mu=0.75, first_channel=n // 4, count=n // 2)
    step(64, "drop then set: new nodes")
    bank.close()


def test_a_refused_store_changes_nothing(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile = 70, 0
    bank, ref = pair(dspfx, n, tile)
    for k in (bank, ref):
        k.set(**mixed(n))
    mic, far = signals(2 * NF)
    mic, far = mic[:, :n], far[:, :n]
    got = run(dspfx, torch, bank, mic[:NF], far[:NF], n, tile)
    agree(torch, bank, ref, got, ref.run(mic[:NF], far[:NF]))
    for call, word in ((lambda: bank.set(taps=0), "taps"), (lambda: bank.set(taps=MAX_TAPS + 1), "taps"), (lambda: bank.set(delay=MAX_DELAY + 1), "delay"),
                       (lambda: bank.set(taps=4, first_channel=n - 1, count=2), "not inside"), (lambda: bank.set(taps=[4, 4], mu=[0.5] * 3), "different"),
                       (lambda: bank.load(np.zeros(MAX_TAPS + 2, F), first_channel=12, count=1), "carries"),
                       (lambda: bank.load(np.zeros((2, 3), F), first_channel=0), "carries"), (lambda: bank.drop(0, n + 1), "not inside"),
                       (lambda: bank.reset(n, 1), "not inside")):
        with pytest.raises(dspfx.DspfxError) as e:
            call()
        assert e.value.status == -1 and word in str(e.value), str(e.value)
    bank.drop(5, 1)
    ref.drop(5, 1)
    with pytest.raises(dspfx.DspfxError) as e:
        bank.load(np.zeros(4, F), first_channel=5, count=1)
    assert "no node" in str(e.value)
    tables_agree(bank, ref)
    got = run(dspfx, torch, bank, mic[NF:], far[NF:], n, tile)
    agree(torch, bank, ref, got, ref.run(mic[NF:], far[NF:]), "after the refused stores")
    bank.close()


def test_a_run_without_ref_or_onto_ref_is_refused(dspfx, torch_cuda):
    torch = torch_cuda
    n = 64
    bank, _ = pair(dspfx, n, 0)
    bank.set(taps=8)
    mic, far = signals(NF)
    dm, dr = device(dspfx, torch, mic[:, :n], 0), device(dspfx, torch, far[:, :n], 0)
    with pytest.raises(dspfx.DspfxError) as e:
        bank.run(dm, NF, out=dm)
    assert e.value.status == -1 and "no ref" in str(e.value), str(e.value)
    whole = torch.cat([dr, dr])
    # out is ref; out ends inside ref (its last frame is ref's first); out starts inside ref (its first frame is ref's last)
    for out, ref_block in ((dr, dr), (whole[n:n * (NF + 1)], whole[n * NF:]), (whole[n * (NF - 1):n * (2 * NF - 1)], whole[:n * NF])):
        with pytest.raises(dspfx.DspfxError) as e:
            bank.run(dm, NF, ref=ref_block, out=out)
        assert e.value.status == -1 and "overlaps ref" in str(e.value), str(e.value)
    bank.run(dm, NF, ref=whole[:n * NF], out=whole[n * NF:])       # an out that begins where ref ends is no overlap
    L, p = bank.L, C.c_void_p(dm.data_ptr())
    assert L.dspfx_cancel_run(bank.h, None, p, p, NF, None) == -1 and b"cancel run" in L.dspfx_cancel_last_error(bank.h)
    for nf in (0, NF + 1):
        with pytest.raises(dspfx.DspfxError) as e:
            bank.run(dm, nf, ref=dr, out=dm)
        assert "n_frames" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert np.array_equal(bits(dm.cpu().numpy().reshape(NF, n)), bits(mic[:, :n])), "a refused run writes nothing"
    bank.close()


def test_a_thread_storing_while_blocks_are_submitted(dspfx, torch_cuda):
    """a second thread loads weights A / B into the frozen upper half, alternating, while the first submits runs of one block,
    and nothing waits.  A frozen node's output depends on its weights and the reference's history alone, so run i of an upper
    channel is block i under A or under B: the store stood before the run or behind it, and a store is whole.  The lower half
    adapts throughout and equals the restatement"""
    torch = torch_cuda
    n, tile, runs, T = 64, 0, 24, 8
    mic, far = signals(NF)
    mic, far = mic[:, :n], far[:, :n]
    ws = [np.random.default_rng(s).uniform(-0.5, 0.5, T).astype(F) for s in (1, 2)]
    blocks = []
    for w in ws:
        ref = R.CancelRef(n, MAX_TAPS, MAX_DELAY)
        ref.set(taps=T, delay=1)
        ref.set(adapt=False, first_channel=n // 2)
        ref.load(w, first_channel=n // 2)
        blocks.append([bits(ref.run(mic, far)) for _ in range(runs)])
    bank, _ = pair(dspfx, n, tile)
    bank.set(taps=T, delay=1)
    bank.set(adapt=False, first_channel=n // 2)
    bank.load(ws[0], first_channel=n // 2)
    dm, dr = device(dspfx, torch, mic, tile), device(dspfx, torch, far, tile)
    dys = [torch.full_like(dm, float("nan")) for _ in range(runs)]
    torch.cuda.synchronize()
    done, errors, made = threading.Event(), [], [0]

    def storer():
        try:
            while not done.is_set() or made[0] < 20:
                bank.load(ws[(made[0] + 1) % 2], first_channel=n // 2)
                made[0] += 1
        except Exception as e:                                   # noqa: BLE001
            errors.append(e)

    t = threading.Thread(target=storer)
    t.start()
    for i in range(runs):
        bank.run(dm, NF, ref=dr, out=dys[i])
    done.set()
    t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for i in range(runs):
        got = bits(host(dspfx, dys[i], NF, n, tile))
        assert np.array_equal(got[:, :n // 2], blocks[0][i][:, :n // 2]), f"run {i}: the adapting half"
        assert any(np.array_equal(got[:, n // 2:], blocks[k][i][:, n // 2:]) for k in range(2)), f"run {i} is block {i} under neither row of weights"
    bank.close()


# ---- 6. invariance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", SHAPES)
def test_in_place_equals_out_of_place(dspfx, torch_cuda, n, tile):
    torch = torch_cuda
    mic, far = signals()
    half = max(n // 2, 1)
    for inplace in (False, True):
        bank, ref = pair(dspfx, n, tile)
        for k in (bank, ref):
            k.set(**{key: v[:half] for key, v in mixed(n).items()})
            if n > half:
                k.set(taps=32, delay=1, first_channel=half)
        both_cuts(dspfx, torch, bank, ref, mic[:, :n], far[:, :n], n, tile, inplace=inplace, what=f"inplace={inplace}")
        bank.close()


def test_three_layouts_give_the_same_bits(dspfx, torch_cuda):
    torch = torch_cuda
    n = 256
    mic, far = signals()
    for tile in (0, 64, 256):
        bank, ref = pair(dspfx, n, tile)
        for k in (bank, ref):
            k.set(**{key: v[:128] for key, v in mixed(n).items()})
            k.set(taps=32, first_channel=128)
        both_cuts(dspfx, torch, bank, ref, mic, far, n, tile, what=f"tile={tile}")
        bank.close()


def test_blocks_at_unaligned_pointers(dspfx, torch_cuda):
    """the blocks start 4, 8 and 12 bytes past a 16-byte boundary: a lane's accesses are single floats on any pointer"""
    torch = torch_cuda
    n, tile, nf = 64, 0, 37
    bank, ref = pair(dspfx, n, tile)
    for k in (bank, ref):
        k.set(taps=5, delay=2)
    mic, far = signals(nf)
    mic, far = mic[:, :n], far[:, :n]
    bm = torch.zeros(nf * n + 8, dtype=torch.float32, device="cuda")
    br = torch.zeros(nf * n + 8, dtype=torch.float32, device="cuda")
    out = torch.full((nf * n + 8,), float("nan"), dtype=torch.float32, device="cuda")
    bm[1:1 + nf * n] = device(dspfx, torch, mic, tile)
    br[2:2 + nf * n] = device(dspfx, torch, far, tile)
    dm, dr, dy = bm[1:1 + nf * n], br[2:2 + nf * n], out[3:3 + nf * n]
    assert dm.data_ptr() % 16 == 4 and dr.data_ptr() % 16 == 8 and dy.data_ptr() % 16 == 12
    bank.run(dm, nf, ref=dr, out=dy)
    torch.cuda.synchronize()
    agree(torch, bank, ref, host(dspfx, dy, nf, n, tile), ref.run(mic, far))
    assert np.isnan(out[:3].cpu().numpy()).all() and np.isnan(out[3 + nf * n:].cpu().numpy()).all(), "nothing outside the block is written"
    bank.close()


def test_a_run_of_256_frames_on_a_bank_that_allows_them(dspfx, torch_cuda):
    n, tile = 256, 64
    bank, ref = pair(dspfx, n, tile, max_frames=256)
    for k in (bank, ref):
        k.set(**{key: v[:128] for key, v in mixed(n).items()})
        k.set(taps=16, first_channel=128)
    mic, far = signals(4 * NF)
    both_cuts(dspfx, torch_cuda, bank, ref, mic, far, n, tile, cuts=(256, 256))
    bank.close()


def test_two_streams(dspfx, torch_cuda):
    """the cuts alternate between two streams and nothing waits in between: the state is the bank's, so a run on another stream
    waits on the device for the one before"""
    torch = torch_cuda
    n, tile = 256, 64
    bank, ref = pair(dspfx, n, tile)
    for k in (bank, ref):
        k.set(**{key: v[:128] for key, v in mixed(n).items()})
        k.set(taps=32, first_channel=128)
    mic, far = signals()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    dms, drs, dys, f0 = [], [], [], 0
    for k in CUTS:
        dms.append(device(dspfx, torch, mic[f0:f0 + k], tile))
        drs.append(device(dspfx, torch, far[f0:f0 + k], tile))
        dys.append(torch.full_like(dms[-1], float("nan")))
        f0 += k
    torch.cuda.synchronize()
    for i, k in enumerate(CUTS):
        bank.run(dms[i], k, ref=drs[i], out=dys[i], stream=streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    got = np.concatenate([host(dspfx, dys[i], k, n, tile) for i, k in enumerate(CUTS)])
    want = np.concatenate([ref.run(mic[a:a + k], far[a:a + k]) for a, k in zip(np.cumsum((0,) + CUTS[:-1]), CUTS)])
    agree(torch, bank, ref, got, want)
    bank.close()


# ---- 7. containment and padding --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("n,tile", TWO)
def test_a_nan_stays_in_its_channel_until_reset(dspfx, torch_cuda, n, tile, uniform):
    """a NaN in channel 3's ref and in channel 9's mic: every other channel's output, weights and levels are the bits of a run
    without it, the two channels follow the restatement (NaN judged by isnan), and reset is their way out"""
    torch = torch_cuda
    mic, far = signals(3 * NF)
    mic, far = mic[:, :n].copy(), far[:, :n].copy()
    clean = []
    cfg = dict(taps=32, delay=1) if uniform else mixed(n)
    for poisoned in (False, True):
        bank, ref = pair(dspfx, n, tile)
        for k in (bank, ref):
            k.set(**cfg)
        if poisoned:
            far[40, 3] = np.nan
            mic[41, 9] = np.nan
        outs = []
        for b in range(2):
            sl = slice(b * NF, (b + 1) * NF)
            got = run(dspfx, torch, bank, mic[sl], far[sl], n, tile)
            want = ref.run(mic[sl], far[sl])
            w, lev = state(torch, bank)
            assert E.same_bits_or_nan(got, want) and E.same_bits_or_nan(w, ref.weights()) and E.same_bits_or_nan(lev, ref.lev)
            outs.append((got, w, lev))
        if not poisoned:
            clean = outs
            bank.close()
            continue
        others = np.ones(n, bool)
        others[[3, 9]] = False
        for (got, w, lev), (g0, w0, l0) in zip(outs, clean):
            assert np.array_equal(bits(got[:, others]), bits(g0[:, others])) and np.array_equal(bits(w[:, others]), bits(w0[:, others]))
            assert np.array_equal(bits(lev[:, others]), bits(l0[:, others]))
        assert np.isnan(outs[1][1][0, [3, 9]]).all(), "the NaN reached both channels' weights and stays"
        for k in (bank, ref):
            k.reset(3, 1)
            k.reset(9, 1)
        sl = slice(2 * NF, 3 * NF)
        got = run(dspfx, torch, bank, mic[sl], far[sl], n, tile)
        agree(torch, bank, ref, got, ref.run(mic[sl], far[sl]), "after the reset")
        assert np.isfinite(got).all()
        bank.close()


@pytest.mark.parametrize("general_only", [False, True])
@pytest.mark.parametrize("T", [5, 32, 64])
def test_an_infinity_just_outside_the_window_is_never_multiplied(dspfx, torch_cuda, T, general_only):
    """ref holds an infinity at the frames that lie exactly T and T + 1 frames behind a run's first frame.  During the run before,
    a delay of 100 keeps the window far behind them; then the delay becomes 0 and the window of the first frame ends one frame in
    front of them.  A padded tap multiplied by a zero weight would make a NaN of it; the channel stays finite and equal to the
    restatement"""
    torch = torch_cuda
    n, tile = 70, 0
    mic, far = signals(2 * NF)
    mic, far = mic[:, :n], far[:, :n].copy()
    far[NF - T, 0::2] = np.inf
    far[NF - T - 1, 1::2] = -np.inf
    bank, ref = pair(dspfx, n, tile, general_only=general_only)
    for k in (bank, ref):
        k.set(taps=T, delay=MAX_DELAY)
    got = run(dspfx, torch, bank, mic[:NF], far[:NF], n, tile)
    agree(torch, bank, ref, got, ref.run(mic[:NF], far[:NF]), "behind the infinities")
    for k in (bank, ref):
        k.set(delay=0)
    got = run(dspfx, torch, bank, mic[NF:NF + 37], far[NF:NF + 37], n, tile)
    agree(torch, bank, ref, got, ref.run(mic[NF:NF + 37], far[NF:NF + 37]), "one frame in front of them")
    w, lev = state(torch, bank)
    assert np.isfinite(got).all() and np.isfinite(w).all() and np.isfinite(lev).all()
    bank.close()


@pytest.mark.parametrize("T", [5, 32])
@pytest.mark.parametrize("n,tile", TWO)
def test_edge_values_in_mic_and_ref(dspfx, torch_cuda, n, tile, T):
    """NaN, both infinities, signed zeros, subnormals, each class in a channel of its own next to plain noise: in mic for the
    first channels' classes, in ref for the last channels' (the two tables of edge_block meet different channels).  NaN is judged
    by isnan, every other bit is the restatement's"""
    torch = torch_cuda
    xm, tab = E.edge_block(n, 3 * NF, level=1.0)
    xr, _ = E.edge_block(n, 3 * NF, level=1.0, seed=0x5EED0E02)
    k = len(E.CLASS_NAMES)
    clean_m, clean_r = signals(3 * NF)
    mic, far = xm.copy(), clean_r[:, :n].copy()
    mic[:, k:] = clean_m[:, k:n]                                   # mic: the classes in the first channels only
    far[:, n - k:] = xr[:, n - k:]                                 # ref: the classes in the last channels only
    bank, ref = pair(dspfx, n, tile)
    for kk in (bank, ref):
        kk.set(taps=T, delay=1)
    for b in range(3):
        sl = slice(b * NF, (b + 1) * NF)
        got = run(dspfx, torch, bank, mic[sl], far[sl], n, tile)
        with np.errstate(all="ignore"):
            want = ref.run(mic[sl], far[sl])
        w, lev = state(torch, bank)
        assert E.same_bits_or_nan(got, want, tab, f"out, block {b}") and E.same_bits_or_nan(w, ref.weights(), None, f"weights, block {b}")
        assert E.same_bits_or_nan(lev, ref.lev, None, f"levels, block {b}")
    assert np.isnan(want).any() and np.isfinite(want[:, k:n - k]).all(), "the edge values reach the output and stay in their channels"
    bank.close()


# ---- 8. full size ----------------------------------------------------------------------------------------------------------
def test_full_size(dspfx, torch_cuda):
    """2^20 channels x 128 frames, tiled 256, T = 32 with every channel adapting and a delay of its own, noise of amplitude 1;
    two alternating buffer triples, device events, median of 20 after 5 warm-ups.  Asserted: sampled channels equal the
    restatement on a first block, and the run fits the 2.667 ms a 128-frame block lasts at 48 kHz.  Printed, not asserted: the
    time and the fraction of 8 TB/s on the bank's own bytes (mic and ref in, out, T weights read and written, 128 ring rows
    written and 128 + T - 1 read), the frozen run, T = 64, the general body forced, a half-present bank, ChannelFirs at T = 32,
    a flat copy of one block on the same buffers."""
    torch = torch_cuda
    n, nf, tile, T = 1 << 20, 128, 256, 32
    gen = torch.Generator(device="cuda").manual_seed(8)
    ms = [torch.rand(nf * n, dtype=torch.float32, device="cuda", generator=gen) * 2 - 1 for _ in range(2)]
    rs = [torch.rand(nf * n, dtype=torch.float32, device="cuda", generator=gen) * 2 - 1 for _ in range(2)]
    ys = [torch.empty_like(ms[0]) for _ in range(2)]

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

    def own_bytes(T):
        return n * 4 * (3 * nf + 2 * T + nf + nf + T - 1)

    max_delay = 255
    assert dspfx.cancel_plan(n, MAX_TAPS, max_delay) == n * (4 * MAX_TAPS + 4 * ((max_delay + MAX_TAPS + 16 + 7) // 8 * 8) + 24)
    delay = (np.arange(n, dtype=np.int64) * 37) % (max_delay + 1)
    bank = dspfx.ChannelCancellers(n, max_taps=MAX_TAPS, max_delay=max_delay, tile_channels=tile, max_frames=nf)
    bank.set(taps=T, delay=delay)
    bank.run(ms[0], nf, ref=rs[0], out=ys[0])
    torch.cuda.synchronize()
    # sampled channels of the first block: both ends, the tile edges, a stride through the middle
    chans = np.unique(np.concatenate([np.arange(0, 70), np.arange(250, 260), np.arange(n - 70, n), np.arange(0, n, 8191)]))

    def lane_view(t):
        return t.view(n // tile, nf, tile)

    def sample(t):
        v = lane_view(t)[torch.from_numpy(chans // tile).cuda(), :, torch.from_numpy(chans % tile).cuda()]
        return np.ascontiguousarray(v.cpu().numpy().T)

    ref = R.CancelRef(len(chans), MAX_TAPS, max_delay)
    ref.set(taps=T, delay=delay[chans])
    want = ref.run(sample(ms[0]), sample(rs[0]))
    assert np.array_equal(bits(sample(ys[0])), bits(want)), "sampled channels of the first block"
    w = bank.weights()[:, torch.from_numpy(chans).cuda()].cpu().numpy()
    lev = bank.levels()[:, torch.from_numpy(chans).cuda()].cpu().numpy()
    assert np.array_equal(bits(w), bits(ref.weights())) and np.array_equal(bits(lev), bits(ref.lev))
    t = {}
    t[32] = timed(lambda i: bank.run(ms[i % 2], nf, ref=rs[i % 2], out=ys[i % 2]))
    torch.cuda.synchronize()
    assert torch.isfinite(bank.weights()).all(), "the weights stay finite on noise"
    bank.set(adapt=False)
    t_frozen = timed(lambda i: bank.run(ms[i % 2], nf, ref=rs[i % 2], out=ys[i % 2]))
    bank.set(adapt=True)
    for s in range(0, n // 256, 2):
        bank.drop(s * 256, 256)
    t_half = timed(lambda i: bank.run(ms[i % 2], nf, ref=rs[i % 2], out=ys[i % 2]))
    bank.drop()
    bank.set(taps=64, delay=delay)
    t[64] = timed(lambda i: bank.run(ms[i % 2], nf, ref=rs[i % 2], out=ys[i % 2]))
    bank.close()
    gbank = dspfx.ChannelCancellers(n, max_taps=MAX_TAPS, max_delay=max_delay, tile_channels=tile, max_frames=nf, general_only=True)
    gbank.set(taps=T, delay=delay)
    t_general = timed(lambda i: gbank.run(ms[i % 2], nf, ref=rs[i % 2], out=ys[i % 2]))
    gbank.close()
    firs = dspfx.ChannelFirs(n, max_taps=MAX_TAPS, tile_channels=tile, max_frames=nf)
    firs.set_taps(np.random.default_rng(3).uniform(-1.0, 1.0, T))
    t_firs = timed(lambda i: firs.run(ms[i % 2], nf, out=ys[i % 2]))
    firs.close()
    t_copy = timed(lambda i: ys[i % 2].copy_(ms[i % 2]))
    frac = lambda T, v: own_bytes(T) / v / 1e9 / 8.0             # noqa: E731
    print(f"full size cancellers, one box, one run: T = 32 adapting {t[32]:.4f} ms ({frac(32, t[32]):.3f} of 8 TB/s on {own_bytes(32) / 2**20:.0f} MiB); "
          f"frozen {t_frozen:.4f} ms; on half the spans of 256 {t_half:.4f} ms; T = 64 {t[64]:.4f} ms ({frac(64, t[64]):.3f} of 8 TB/s); "
          f"T = 32 with the general body forced {t_general:.4f} ms (fast x {t_general / t[32]:.2f}); ChannelFirs at T = 32 {t_firs:.4f} ms; "
          f"flat copy of one block {t_copy:.4f} ms")
    assert t[32] * 1e-3 <= 128 / 48000, t[32]
