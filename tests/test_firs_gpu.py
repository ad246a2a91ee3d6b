"""The channel-FIR bank on the GPU (dspfx_firs_*, through the Python class): per-channel FIR nodes, each with its own taps.  A
channel's output is compared BIT FOR BIT with firs_ref (one oracle FIR node per channel, the bank's store rules), which
tests/test_firs_cpu.py holds to oracle/numpy_model.Fir; below 16 taps also with Engine([Fir(h)], link_flags=0), which runs its
exact kernel there.  The tap counts 1 2 3 4 5 8 15 16 17 31 32 33 64 stand on both sides of every capacity doubling of the
reference's VecDeque, and every sequence runs 37 + 128 + 91 + 128 frames: T + 2 cap = 320 frames past the first run for T = 64, so
the split point of the two sums wraps.  Out-of-place outputs start as NaN everywhere, so every sample is shown to be written."""
import ctypes as C
import threading

import numpy as np
import pytest

import edge_values as E
import firs_ref as R
import oracle as O

pytestmark = pytest.mark.gpu

NF = 128
F = np.float32
SHAPES = [(64, 0), (256, 64), (70, 0), (1, 0)]                   # a full wave; tiled, more than one wave; a ragged last wave; one channel
THREE = [(64, 0), (256, 64), (70, 0)]
TWO = [(256, 64), (70, 0)]
FRAMES = [1, 37, 128]
CUTS = (37, 128, 91, 128)
NX = 256
LIST = R.TAP_COUNTS
MAX_TAPS = 64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_X = {}


def noise_x(nf=sum(CUTS)):
    """noise * 2.5: [4 * 128][NX], made once, left unchanged"""
    if "x" not in _X:
        x = O.noise(0x5EED0F12, np.arange(NX), np.arange(4 * NF)) * F(2.5)
        x[0, :10] = [0, -0.0, 0.25, -0.25, 0.5, -0.5, 1, -1, 2, -2]
        x.setflags(write=False)
        _X["x"] = x
    return _X["x"][:nf]


def response(T, seed):
    return np.random.default_rng(1000 * T + seed).uniform(-1.0, 1.0, T)


def device(dspfx, torch, x, tile):
    return torch.from_numpy(dspfx.to_layout(np.ascontiguousarray(x), tile).reshape(-1).copy()).cuda()


def host(dspfx, t, nf, n, tile):
    return dspfx.from_layout(t.cpu().numpy(), nf, n, tile)


def run(dspfx, torch, bank, x, n, tile, inplace=False, stream=0):
    dx = device(dspfx, torch, x, tile)
    out = dx if inplace else torch.full_like(dx, float("nan"))
    torch.cuda.synchronize()
    dy = bank.run(dx, len(x), out=out, stream=stream)
    torch.cuda.synchronize()
    return host(dspfx, dy, len(x), n, tile)


def run_cuts(dspfx, torch, bank, x, n, tile, cuts=CUTS, inplace=False, each=None):
    out, f0 = [], 0
    for k in cuts:
        out.append(run(dspfx, torch, bank, x[f0:f0 + k], n, tile, inplace=inplace))
        f0 += k
        if each:
            each()
    return np.concatenate(out)


def ref_cuts(ref, x, cuts=CUTS, each=None):
    out, f0 = [], 0
    for k in cuts:
        out.append(ref.run(x[f0:f0 + k]))
        f0 += k
        if each:
            each()
    return np.concatenate(out)


def deque_of(torch, bank):
    torch.cuda.synchronize()
    return bank.deque().cpu().numpy()


def pair(dspfx, n, tile, max_frames=NF, **kw):
    return dspfx.ChannelFirs(n, max_taps=MAX_TAPS, tile_channels=tile, max_frames=max_frames, **kw), R.ChannelFirs(n, MAX_TAPS)


def mixed(n):
    """channel c: T = LIST[c % 13], its own taps, Average on every second group of 13"""
    return [(response(LIST[c % 13], c), R.AVERAGE if (c // 13) % 2 else R.BALANCED) for c in range(n)]


def store_mixed(k, settings, first=0):
    for c, (h, mode) in enumerate(settings):
        assert k.set_taps(h[None, :], first_channel=first + c, mode=mode) is not False


def tables_agree(bank, ref):
    assert np.array_equal(bank.present(), ref.present()) and np.array_equal(bank.lengths(), ref.lengths())
    assert np.array_equal(bank.modes(), ref.modes())
    for c in (0, ref.n // 2, ref.n - 1):
        want = np.zeros(0) if ref.h[c] is None else ref.h[c]
        assert np.array_equal(bank.taps(c).view(np.uint64), want.view(np.uint64)), c


_ENGINE = {}


def engine_ref(dspfx, torch, T, mode):
    """Engine([Fir(response(T, 0), mode)], link_flags=0) on noise_x() over 128-frame blocks, [4 * 128][NX]: made once, shared"""
    if (T, mode) not in _ENGINE:
        x = noise_x(4 * NF)
        eng = dspfx.Engine(NX, NF, link_flags=0)
        eng.set_chain([dspfx.Fir(response(T, 0), mode)])
        y = np.empty_like(x)
        for b in range(4):
            dx = torch.from_numpy(x[b * NF:(b + 1) * NF].copy()).cuda()
            dy = torch.full_like(dx, float("nan"))
            eng.process(dx, out=dy, n_frames=NF)
            torch.cuda.synchronize()
            y[b * NF:(b + 1) * NF] = dy.cpu().numpy()
        eng.close()
        y.setflags(write=False)
        _ENGINE[(T, mode)] = y
    return _ENGINE[(T, mode)]


# ---- 1. a fresh bank -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_a_fresh_bank_copies(dspfx, torch_cuda, n, tile, nf):
    bank = dspfx.ChannelFirs(n, max_taps=MAX_TAPS, tile_channels=tile, max_frames=NF)
    x = noise_x(nf)[:, :n]
    assert np.array_equal(bits(run(dspfx, torch_cuda, bank, x, n, tile)), bits(x))
    assert np.array_equal(bits(run(dspfx, torch_cuda, bank, x, n, tile, inplace=True)), bits(x))
    assert not bank.present().any() and not bank.lengths().any() and (bank.modes() == dspfx.FIRS_NONE).all()
    assert bank.taps(0).shape == (0,) and not deque_of(torch_cuda, bank).any() and deque_of(torch_cuda, bank).shape == (3, n)
    bank.close()


# ---- 2. one response everywhere ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [R.BALANCED, R.AVERAGE])
@pytest.mark.parametrize("n,tile", SHAPES)
def test_one_response_everywhere_equals_the_oracle_and_the_exact_engine(dspfx, torch_cuda, n, tile, mode):
    """every T of the list on one bank, a drop between them (drop then set is a new node); below 16 taps the engine's bits too"""
    torch = torch_cuda
    bank, ref = pair(dspfx, n, tile)
    x = noise_x()[:, :n]
    for T in LIST:
        h = response(T, 0)
        for k in (bank, ref):
            assert k.drop() is not False and k.set_taps(h, mode=mode) is not False
        got = run_cuts(dspfx, torch, bank, x, n, tile)
        assert np.array_equal(bits(got), bits(ref_cuts(ref, x))), f"N={n} tile={tile} T={T} mode={mode}"
        assert np.array_equal(deque_of(torch, bank), ref.deque()), T
        if T <= 15:
            assert np.array_equal(bits(got), bits(engine_ref(dspfx, torch, T, mode)[:len(x), :n])), f"the engine: N={n} tile={tile} T={T}"
        assert (bank.lengths() == T).all() and (bank.modes() == mode).all() and np.array_equal(bank.taps(n - 1), h)
    bank.close()


# ---- 3, 4. a mixed bank, a bank of one T with distinct taps; the deque words ---------------------------------------------
@pytest.mark.parametrize("n,tile", SHAPES)
def test_mixed_bank_every_channel_equals_the_oracle_of_its_own_node(dspfx, torch_cuda, n, tile):
    """T = LIST[c % 13]: lanes of different T, in the fill phase for different numbers of frames, in one wave -- the general
    body; len, cap and head after every run"""
    torch = torch_cuda
    bank, ref = pair(dspfx, n, tile)
    settings = mixed(n)
    store_mixed(bank, settings)
    store_mixed(ref, settings)
    tables_agree(bank, ref)
    x = noise_x()[:, :n]
    got_dq, want_dq = [], []
    got = run_cuts(dspfx, torch, bank, x, n, tile, each=lambda: got_dq.append(deque_of(torch, bank)))
    want = ref_cuts(ref, x, each=lambda: want_dq.append(ref.deque()))
    assert np.array_equal(bits(got), bits(want)), f"N={n} tile={tile}: channels {np.flatnonzero((bits(got) != bits(want)).any(axis=0))[:8]}"
    for i, (g, w) in enumerate(zip(got_dq, want_dq)):
        assert np.array_equal(g, w), f"deque words after run {i}"
    bank.close()


@pytest.mark.parametrize("n,tile", SHAPES)
def test_one_tap_count_distinct_taps_and_the_two_bodies_agree(dspfx, torch_cuda, n, tile):
    """T = 32 everywhere, every channel its own taps, stored as one [n][32] array: from the run in which every deque is full the
    waves take the steady body.  A second bank that is made to take the general body everywhere gives the same bits"""
    torch = torch_cuda
    rows = np.stack([response(32, c) for c in range(n)])
    x = noise_x()[:, :n]
    ref = R.ChannelFirs(n, MAX_TAPS)
    assert ref.set_taps(rows)
    want_dq = []
    want = ref_cuts(ref, x, each=lambda: want_dq.append(ref.deque()))
    for general in (False, True):
        bank = dspfx.ChannelFirs(n, max_taps=MAX_TAPS, tile_channels=tile, max_frames=NF, general_only=general)
        bank.set_taps(rows)
        tables_agree(bank, ref)
        got_dq = []
        got = run_cuts(dspfx, torch, bank, x, n, tile, each=lambda: got_dq.append(deque_of(torch, bank)))
        assert np.array_equal(bits(got), bits(want)), f"N={n} tile={tile} general_only={general}"
        assert all(np.array_equal(g, w) for g, w in zip(got_dq, want_dq)), "deque words after every run"
        bank.close()


# ---- 5. store rules --------------------------------------------------------------------------------------------------------
def test_store_rules_on_the_device_follow_the_restatement(dspfx, torch_cuda):
    """between runs, nothing waiting in between: a reload to a shorter and to a longer response keeps the deque, set_mode alone,
    reset, drop then set (a new node), drop; the bank and firs_ref get the same calls"""
    torch = torch_cuda
    n, tile = 70, 0
    x = noise_x(3 * NF)[:, :n]
    bank, ref = pair(dspfx, n, tile)
    h17, h5, h33 = response(17, 1), response(5, 2), response(33, 3)
    rows5 = np.stack([response(5, 40 + c) for c in range(10)])
    both = (bank, ref)
    for k in both:
        assert k.set_taps(h17) is not False
    a = run(dspfx, torch, bank, x[:NF], n, tile)
    assert np.array_equal(bits(a), bits(ref.run(x[:NF])))
    for k in both:
        assert k.set_taps(h5, first_channel=0, count=10) is not False                    # the reload, shorter: the deque stays 17 long
        assert k.set_taps(h33, first_channel=10, count=10) is not False                  # the reload, longer: the deque goes on growing
        assert k.set_mode(R.AVERAGE, first_channel=20, count=10) is not False            # the mode alone
        assert k.reset(30, 10) is not False                                              # the deque emptied
        assert k.drop(40, 10) is not False and k.set_taps(rows5, first_channel=40, mode=R.AVERAGE) is not False      # a new node
        assert k.drop(50, 10) is not False                                               # a copy again
    tables_agree(bank, ref)
    assert list(bank.lengths()[[0, 10, 20, 30, 40, 50, 60]]) == [5, 33, 17, 17, 5, 0, 17]
    assert list(bank.modes()[[0, 20, 40, 50]]) == [R.BALANCED, R.AVERAGE, R.AVERAGE, dspfx.FIRS_NONE]
    b = run(dspfx, torch, bank, x[NF:2 * NF], n, tile)
    wb = ref.run(x[NF:2 * NF])
    assert np.array_equal(bits(b), bits(wb)), np.flatnonzero((bits(b) != bits(wb)).any(axis=0))
    dq = deque_of(torch, bank)
    assert np.array_equal(dq, ref.deque())
    assert dq[0, 0] == 17 and dq[0, 10] == 33 and dq[0, 30] == 17 and dq[0, 40] == 5 and not dq[:, 50:60].any()
    assert np.array_equal(bits(b[:, 50:60]), bits(x[NF:2 * NF, 50:60])), "dropped: a copy"
    c = run(dspfx, torch, bank, x[2 * NF:], n, tile)
    assert np.array_equal(bits(c), bits(ref.run(x[2 * NF:])))
    assert np.array_equal(deque_of(torch, bank), ref.deque())
    bank.close()


def test_a_refused_store_changes_nothing(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile = 70, 0
    bank, ref = pair(dspfx, n, tile)
    settings = mixed(n)
    store_mixed(bank, settings)
    store_mixed(ref, settings)
    x = noise_x(2 * NF)[:, :n]
    first = run(dspfx, torch, bank, x[:NF], n, tile)
    bad = [(lambda k: k.set_taps(np.zeros(0)), "taps"), (lambda k: k.set_taps(np.zeros(MAX_TAPS + 1)), "max_taps"),
           (lambda k: k.set_taps(np.zeros((2, 0)), first_channel=0), "taps"), (lambda k: k.set_taps(np.ones(4), first_channel=n - 1, count=2), "channels"),
           (lambda k: k.set_taps(np.ones((3, 4)), first_channel=n - 2), "channels"), (lambda k: k.set_taps(np.ones((3, 4)), first_channel=0, count=2), "[count][T]"),
           (lambda k: k.set_taps(np.ones((1, 2, 2))), "[count][T]"), (lambda k: k.set_taps(np.ones(4), mode=2), "mode"),
           (lambda k: k.set_mode(2), "mode"), (lambda k: k.set_mode(R.AVERAGE, n, 1), "channels"), (lambda k: k.drop(0, n + 1), "channels"),
           (lambda k: k.reset(n + 1, 0), "channels")]
    for call, word in bad:
        with pytest.raises(dspfx.DspfxError) as e:
            call(bank)
        assert e.value.status == -1 and word in str(e.value) and "firs" in str(e.value), str(e.value)
        assert call(ref) is False
    for call in (lambda: bank.taps(n), lambda: bank.present(1, n), lambda: bank.lengths(n, 1)):
        with pytest.raises(dspfx.DspfxError):
            call()
    assert bank.L.dspfx_firs_set_taps(bank.h, None, 4, 0, 0, 0, 1) == -1 and b"no taps" in bank.L.dspfx_firs_last_error(bank.h)
    tables_agree(bank, ref)
    got = np.concatenate([first, run(dspfx, torch, bank, x[NF:], n, tile)])
    assert np.array_equal(bits(got), bits(ref_cuts(ref, x, (NF, NF)))), "after the refused stores: the nodes and their deques as they were"
    bank.close()


def test_a_thread_storing_reloads_while_blocks_are_submitted(dspfx, torch_cuda):
    """a second thread reloads response A / B over the whole range, alternating, while the first submits runs of one block, and
    nothing waits.  A reload keeps the deque, so run i is block i of the restatement under A throughout or under B throughout:
    the store stood before the run or behind it, and a store is whole"""
    torch = torch_cuda
    n, tile, runs = 64, 0, 24
    hs = (response(8, 1), response(8, 2))
    x = noise_x(NF)[:, :n]
    blocks = []
    for h in hs:
        ref = R.ChannelFirs(n, MAX_TAPS)
        assert ref.set_taps(h)
        blocks.append([bits(ref.run(x)) for _ in range(runs)])
    bank = dspfx.ChannelFirs(n, max_taps=MAX_TAPS, tile_channels=tile, max_frames=NF)
    bank.set_taps(hs[0])
    dx = device(dspfx, torch, x, tile)
    dys = [torch.full_like(dx, float("nan")) for _ in range(runs)]
    torch.cuda.synchronize()
    done, errors, made = threading.Event(), [], [0]

    def storer():
        try:
            while not done.is_set() or made[0] < 20:
                bank.set_taps(hs[(made[0] + 1) % 2])
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
        assert any(np.array_equal(got, blocks[k][i]) for k in range(2)), f"run {i} is block {i} under neither response"
    bank.close()


# ---- 6. invariance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", THREE)
def test_a_channels_bits_do_not_depend_on_its_neighbours(dspfx, torch_cuda, n, tile):
    """the kept channels (every third, and the last) get the same nodes and samples in three banks; every other channel is empty
    in the second, and carries another tap count, other taps and NaN samples in the third"""
    torch = torch_cuda
    keep = np.zeros(n, bool)
    keep[::3] = True
    keep[n - 1] = True
    sa = mixed(n)
    other = [(response(LIST[(c + 5) % 13], c + 999), R.AVERAGE) for c in range(n)]
    x = noise_x()[:, :n]
    x3 = np.where(keep, x, noise_x(4 * NF)[NF // 2:NF // 2 + len(x), :n] * F(5))
    x3[:, np.flatnonzero(~keep)[::3]] = np.nan
    outs = []
    for which, xx in ((0, x), (1, x), (2, x3)):
        bank = dspfx.ChannelFirs(n, max_taps=MAX_TAPS, tile_channels=tile, max_frames=NF)
        for c in range(n):
            if keep[c] or which == 0:
                bank.set_taps(sa[c][0][None, :], first_channel=c, mode=sa[c][1])
            elif which == 2:
                bank.set_taps(other[c][0][None, :], first_channel=c, mode=other[c][1])
        outs.append((run_cuts(dspfx, torch, bank, xx, n, tile), deque_of(torch, bank)))
        bank.close()
    for y, dq in outs[1:]:
        assert np.array_equal(bits(y[:, keep]), bits(outs[0][0][:, keep])) and np.array_equal(dq[:, keep], outs[0][1][:, keep])
    assert np.array_equal(bits(outs[1][0][:, ~keep]), bits(x[:, ~keep])), "the empty neighbours copy"


@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_in_place_equals_out_of_place(dspfx, torch_cuda, n, tile, nf):
    """the cuts are nf frames long, so a bank sees runs of 1, of 37 and of 128 frames in the fill phase and behind it"""
    torch = torch_cuda
    x = noise_x(3 * NF)[:, :n]
    cuts = (nf,) * (24 if nf == 1 else 3)
    x = x[:sum(cuts)]
    half = max(n // 2, 1)

    def store(k):
        """the lower half mixed, the upper half 8 taps of its own per channel"""
        store_mixed(k, mixed(n)[:half])
        if n > half:
            assert k.set_taps(np.stack([response(8, c) for c in range(n - half)]), first_channel=half) is not False

    outs = []
    for inplace in (False, True):
        bank = dspfx.ChannelFirs(n, max_taps=MAX_TAPS, tile_channels=tile, max_frames=NF)
        store(bank)
        outs.append(run_cuts(dspfx, torch, bank, x, n, tile, cuts=cuts, inplace=inplace))
        bank.close()
    assert np.array_equal(bits(outs[0]), bits(outs[1])) and not np.isnan(outs[0]).any()
    ref = R.ChannelFirs(n, MAX_TAPS)
    store(ref)
    assert np.array_equal(bits(outs[0]), bits(ref.run(x)))


def test_both_layouts_give_the_same_bits(dspfx, torch_cuda):
    torch = torch_cuda
    n = 256
    outs = []
    for tile in (0, 64, 256):
        bank = dspfx.ChannelFirs(n, max_taps=MAX_TAPS, tile_channels=tile, max_frames=NF)
        store_mixed(bank, mixed(n)[:128])
        bank.set_taps(np.stack([response(32, c) for c in range(128)]), first_channel=128)
        outs.append((run_cuts(dspfx, torch, bank, noise_x()[:, :n], n, tile), deque_of(torch, bank)))
        bank.close()
    for y, dq in outs[1:]:
        assert np.array_equal(bits(y), bits(outs[0][0])) and np.array_equal(dq, outs[0][1])


def test_out_of_place_from_an_unaligned_pointer_takes_the_scalar_path(dspfx, torch_cuda):
    """the blocks start 4 and 12 bytes past a 16-byte boundary: a lane's accesses are single floats on any pointer"""
    torch = torch_cuda
    n, tile, nf = 64, 0, 37
    bank, ref = pair(dspfx, n, tile)
    rows = np.stack([response(5, c) for c in range(n)])
    bank.set_taps(rows)
    assert ref.set_taps(rows)
    x = noise_x(nf)[:, :n]
    big = torch.zeros(nf * n + 8, dtype=torch.float32, device="cuda")
    out = torch.full((nf * n + 8,), float("nan"), dtype=torch.float32, device="cuda")
    big[1:1 + nf * n] = device(dspfx, torch, x, tile)
    dx, dy = big[1:1 + nf * n], out[3:3 + nf * n]
    assert dx.data_ptr() % 16 == 4 and dy.data_ptr() % 16 == 12
    bank.run(dx, nf, out=dy)
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(dspfx, dy, nf, n, tile)), bits(ref.run(x)))
    assert np.isnan(out[:3].cpu().numpy()).all() and np.isnan(out[3 + nf * n:].cpu().numpy()).all(), "nothing outside the block is written"
    bank.close()


def test_a_null_pointer_or_no_frames_is_refused(dspfx, torch_cuda):
    torch = torch_cuda
    n = 64
    bank = dspfx.ChannelFirs(n, max_taps=MAX_TAPS, max_frames=NF)
    bank.set_taps(response(8, 0))
    dx = device(dspfx, torch, noise_x(NF)[:, :n], 0)
    L, p = bank.L, C.c_void_p(dx.data_ptr())
    assert L.dspfx_firs_run(bank.h, None, p, NF, None) == -1 and b"firs run" in L.dspfx_firs_last_error(bank.h)
    assert L.dspfx_firs_run(bank.h, p, None, NF, None) == -1
    for nf in (0, NF + 1):
        with pytest.raises(dspfx.DspfxError) as e:
            bank.run(dx, nf, out=dx)
        assert e.value.status == -1 and "n_frames" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert np.array_equal(bits(dx.cpu().numpy().reshape(NF, n)), bits(noise_x(NF)[:, :n])), "a refused run writes nothing"
    bank.close()


def test_a_run_of_256_frames_on_a_bank_that_allows_them(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile = 256, 64
    bank, ref = pair(dspfx, n, tile, max_frames=256)
    store_mixed(bank, mixed(n))
    store_mixed(ref, mixed(n))
    x = noise_x(4 * NF)[:, :n]
    got = run_cuts(dspfx, torch, bank, x, n, tile, cuts=(256, 256))
    assert np.array_equal(bits(got), bits(ref.run(x)))
    assert np.array_equal(deque_of(torch, bank), ref.deque())
    bank.close()


def test_two_streams(dspfx, torch_cuda):
    """the cuts alternate between two streams and nothing waits in between: the state is the bank's, so a run on another stream
    waits on the device for the one before"""
    torch = torch_cuda
    n, tile = 256, 64
    bank, ref = pair(dspfx, n, tile)
    store_mixed(bank, mixed(n))
    store_mixed(ref, mixed(n))
    x = noise_x()[:, :n]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    dxs, dys, f0 = [], [], 0
    for k in CUTS:
        dxs.append(device(dspfx, torch, x[f0:f0 + k], tile))
        dys.append(torch.full_like(dxs[-1], float("nan")))
        f0 += k
    torch.cuda.synchronize()
    for i, k in enumerate(CUTS):
        bank.run(dxs[i], k, out=dys[i], stream=streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    got = np.concatenate([host(dspfx, dys[i], k, n, tile) for i, k in enumerate(CUTS)])
    assert np.array_equal(bits(got), bits(ref.run(x))) and np.array_equal(deque_of(torch, bank), ref.deque())
    bank.close()


# ---- 7. edge values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [5, 32])
@pytest.mark.parametrize("n,tile", TWO)
def test_edge_values_in_the_samples_and_in_single_taps(dspfx, torch_cuda, n, tile, T):
    """NaN, both infinities, signed zeros, subnormals, each class in a channel of its own next to plain noise, through T taps
    (T = 32: the steady body from the second block on); then the same kinds of value in ONE tap of a channel's response.  NaN is
    judged by isnan, the sign of every infinity and zero and every other bit must be the oracle's"""
    torch = torch_cuda
    x, tab = E.edge_block(n, 3 * NF)
    bank, ref = pair(dspfx, n, tile)
    rows = np.stack([response(T, c) for c in range(n)])
    specials = [np.nan, np.inf, -np.inf, -0.0, 0.0, 5e-324, -2.0 ** -1060, 1e300, -1e300]
    for c in range(n // 2, n):                                    # the upper half: an edge value in one tap, noise in the samples
        rows[c, (c * 7) % T] = specials[c % len(specials)]
    for k in (bank, ref):
        assert k.set_taps(rows) is not False
    xs = x.copy()
    xs[:, n // 2:] = noise_x(3 * NF)[:, :n - n // 2]
    for c in list(tab):
        if c >= n // 2:
            tab.pop(c)
    got = run_cuts(dspfx, torch, bank, xs, n, tile, cuts=(NF, NF, NF))
    with np.errstate(all="ignore"):
        want = ref.run(xs)
    assert E.same_values(got, want, 0, tab, f"N={n} T={T}")
    assert np.isnan(want).any() and np.isinf(want).any(), "the edge values reach the output"
    bank.close()


# ---- 8. full size ----------------------------------------------------------------------------------------------------------
def test_full_size(dspfx, torch_cuda):
    """2^20 channels x 128 frames, tiled 256, noise in every channel; two alternating buffer pairs, device events, median of 20
    after 5 warm-ups.  Asserted: a T = 8 bank with one response everywhere equals Engine([Fir(h8)]) on the same buffers bit for
    bit on a first block; a bank with T = 32 and distinct taps on every channel, stored in ranges of 65 536 channels per call,
    fits the 2.667 ms a 128-frame block lasts at 48 kHz.  Printed, not asserted: T = 8, 16, 32 and 64, the engine at the same
    uniform taps, the general body forced against the steady one, a half-present bank, the first block behind a reset of every
    channel, at 2^18 channels the deques of a wave's lanes in step against 64 different heads, a flat copy of one block;
    milliseconds and the fraction of 8 TB/s on the bank's own bytes: block in, block out, T taps of 8 bytes, T samples of history
    read and 128 written."""
    torch = torch_cuda
    n, nf, tile = 1 << 20, 128, 256
    gen = torch.Generator(device="cuda").manual_seed(8)
    xs = [torch.rand(nf * n, dtype=torch.float32, device="cuda", generator=gen) * 5 - 2.5 for _ in range(2)]
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

    def own_bytes(T):
        return n * (2 * nf * 4 + 8 * T + 4 * T + 4 * nf)

    assert dspfx.firs_plan(n, MAX_TAPS) == n * (12 * MAX_TAPS + 80)
    # T = 8, one response everywhere: the engine's bits on a first block
    h8 = response(8, 0)
    bank = dspfx.ChannelFirs(n, max_taps=MAX_TAPS, tile_channels=tile, max_frames=nf)
    bank.set_taps(h8)
    eng = dspfx.Engine(n, nf, link_flags=0, tile_channels=tile)
    eng.set_chain([dspfx.Fir(h8)])
    bank.run(xs[0], nf, out=ys[0])
    eng.process(xs[0], out=ys[1], n_frames=nf)
    torch.cuda.synchronize()
    assert torch.equal(ys[0].view(torch.int32), ys[1].view(torch.int32)), "T = 8: the bank's bits are the engine's"
    t, t_eng = {}, {}
    t_eng[8] = timed(lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=nf))
    torch.cuda.synchronize()
    eng.close()
    t[8] = timed(lambda i: bank.run(xs[i % 2], nf, out=ys[i % 2]))
    # T = 32, distinct taps on every channel, in ranges of 65 536 channels per call: the real-time condition
    rng = np.random.default_rng(9)
    for c0 in range(0, n, 65536):
        bank.set_taps(rng.uniform(-1.0, 1.0, (65536, 32)), first_channel=c0)
    assert (bank.lengths() == 32).all()
    t[32] = timed(lambda i: bank.run(xs[i % 2], nf, out=ys[i % 2]))
    torch.cuda.synchronize()
    dq = bank.deque().cpu().numpy()
    assert (dq[0] == 32).all() and (dq[1] == 64).all(), "every deque full: the steady body"
    # the first block of new nodes everywhere (reset: every deque empty): 33 frames of fill in the general body, then the steady one
    def first_block(i):
        bank.reset()
        bank.run(xs[i % 2], nf, out=ys[i % 2])

    t_first = timed(first_block)
    for i in range(5):
        bank.run(xs[i % 2], nf, out=ys[i % 2])
    # half present: the node dropped on every other span of 256
    for s in range(0, n // 256, 2):
        bank.drop(s * 256, 256)
    t_half = timed(lambda i: bank.run(xs[i % 2], nf, out=ys[i % 2]))
    for T in (16, 64):
        bank.drop()
        bank.set_taps(response(T, 0))
        t[T] = timed(lambda i: bank.run(xs[i % 2], nf, out=ys[i % 2]))
    bank.close()
    # the general body forced, T = 32 (one response everywhere: the table is per channel all the same)
    gbank = dspfx.ChannelFirs(n, max_taps=MAX_TAPS, tile_channels=tile, max_frames=nf, general_only=True)
    gbank.set_taps(response(32, 0))
    t_general = timed(lambda i: gbank.run(xs[i % 2], nf, out=ys[i % 2]))
    gbank.close()
    for T in (16, 32, 64):
        eng = dspfx.Engine(n, nf, link_flags=0, tile_channels=tile)
        eng.set_chain([dspfx.Fir(response(T, 0))])
        t_eng[T] = timed(lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=nf))
        torch.cuda.synchronize()
        eng.close()
    # the deques of a wave's lanes out of step: at 2^18 channels (one reset per channel), channel c is reset c % 64 frames after
    # channel c - c % 64, so the slices of the 64 lanes end at 64 different taps; beside it the same bank with the deques in step
    m = n // 4
    qbank = dspfx.ChannelFirs(m, max_taps=MAX_TAPS, tile_channels=tile, max_frames=nf)
    qbank.set_taps(response(32, 0))
    t_step = timed(lambda i: qbank.run(xs[i % 2], nf, out=ys[i % 2]))
    for j in range(64):
        for c in range(j, m, 64):
            assert qbank.L.dspfx_firs_reset(qbank.h, c, 1) == 0
        qbank.run(xs[0], 1, out=ys[0])
    t_phase = timed(lambda i: qbank.run(xs[i % 2], nf, out=ys[i % 2]))
    torch.cuda.synchronize()
    assert len(set(qbank.deque()[2, :64].cpu().numpy().tolist())) == 64, "64 heads in one wave"
    qbank.close()
    t_copy = timed(lambda i: ys[i % 2].copy_(xs[i % 2]))
    frac = lambda T, ms: own_bytes(T) / ms / 1e9 / 8.0           # noqa: E731
    print("full size firs, one box, one run: " + ", ".join(
        f"T = {T} {t[T]:.4f} ms ({frac(T, t[T]):.3f} of 8 TB/s on {own_bytes(T) / 2**20:.0f} MiB; Engine([Fir]) {t_eng[T]:.4f} ms)" for T in (8, 16, 32, 64))
        + f"; T = 32 with the general body forced {t_general:.4f} ms (steady x {t_general / t[32]:.2f}); T = 32 on half the spans of 256 {t_half:.4f} ms; "
        f"T = 32, the first block behind a reset of every channel {t_first:.4f} ms; "
        f"T = 32 at 2^18 channels with the deques in step {t_step:.4f} ms, with the 64 lanes of every wave at 64 heads {t_phase:.4f} ms; "
        f"flat copy of one block {t_copy:.4f} ms")
    assert t[32] * 1e-3 <= 128 / 48000, t[32]
