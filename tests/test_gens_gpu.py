"""The channel-generator bank on the GPU (dspfx_gens_*, through the Python class): per-channel Signal Generators.  A channel's
output is compared bit for bit with Engine([SignalGen(amplitude, frequency, mode)], link_flags=0) over the same sequence of block
lengths -- one engine per mode, one run per distinct setting, made once per module and shared -- and, through gens_ref (one oracle
node per channel), with the oracle at the bars tests/test_gpu_parity.py holds the engine's generator to: 0 ulp for Triangle, Square
and Constant, at most 2 ulp for Sine.  Where the expectation is a NaN the bank must give a NaN; its sign and payload are not
compared (edge_values.same_bits_or_nan).  Outputs start as NaN everywhere, so every sample is shown to be written."""
import threading

import numpy as np
import pytest

import edge_values as E
import gens_ref as R
import oracle as O
from chains import ulp_diff

pytestmark = pytest.mark.gpu

NF = 128
F = np.float32
SHAPES = [(64, 0), (256, 64), (70, 0), (1, 0)]                   # vector lanes; tiled; scalar accesses and a ragged last workgroup; one channel
THREE = [(64, 0), (256, 64), (70, 0)]
FRAMES = [1, 37, 128, 256]                                       # 256 on a bank of max_frames 256: a clock wraps inside a run
PAIRS = ((100.0, 0.5), (12000.0, 1.0), (0.1, -0.3), (19999.0, 0.7), (441.0, -1.0))       # (frequency, amplitude): test_signal_gen_modes
MIX_AMPS = (0.5, -1.0, 0.25)
MIX_FREQS = (100.0, 441.0, 12000.0, 19999.0)
SINE_ULP = 2                                                     # test_signal_gen_modes' bar for Sine; every other mode is exact
EDGE = (float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 1e-40, 1e12, -100.0)
EC = 64                                                          # the channels of the engines that give the expectations


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_ENG, _COL = {}, {}


@pytest.fixture(scope="module", autouse=True)
def engines():
    yield
    for e in _ENG.values():
        e.close()
    _ENG.clear()
    _COL.clear()


def engine_col(dspfx, torch, s, lengths):
    """what Engine([SignalGen(amplitude, frequency, mode)], link_flags=0) writes for a channel over consecutive runs of `lengths`
    frames from clock 0, s = (amplitude, frequency, mode) -> [sum(lengths)]; computed once per (s, lengths), shared, left unchanged.
    One engine per mode: the sliders are stored and the clock reset for every setting"""
    lengths = tuple(lengths)
    key = (tuple(np.asarray(s[:2], F).view(np.uint32).tolist()), s[2], lengths)
    if key not in _COL:
        if s[2] not in _ENG:
            _ENG[s[2]] = dspfx.Engine(EC, 256, link_flags=0)
            _ENG[s[2]].set_chain([dspfx.SignalGen(0.5, 100.0, s[2])])
        eng = _ENG[s[2]]
        eng.set_param(0, 0, s[0])
        eng.set_param(0, 1, s[1])
        eng.reset()
        outs = []
        for k in lengths:
            dx = torch.zeros(k * EC, dtype=torch.float32, device="cuda")
            dy = torch.full_like(dx, float("nan"))
            eng.process(dx, out=dy, n_frames=k)
            outs.append(dy)
        torch.cuda.synchronize()
        y = np.concatenate([d.cpu().numpy().reshape(-1, EC) for d in outs])
        assert np.array_equal(bits(y), bits(np.repeat(y[:, :1], EC, axis=1))), "the engine's channels are identical"
        col = y[:, 0].copy()
        col.setflags(write=False)
        _COL[key] = col
    return _COL[key]


def expected(dspfx, torch, settings, lengths):
    """[sum(lengths)][len(settings)]: channel c as the engine of its own setting gives it; None: +0.0"""
    want = np.zeros((sum(lengths), len(settings)), F)
    for c, s in enumerate(settings):
        if s is not None:
            want[:, c] = engine_col(dspfx, torch, s, lengths)
    return want


def store(b, settings, first=0):
    """the settings onto a bank or its restatement: consecutive present channels in one store, absent ones dropped"""
    c, n = 0, len(settings)
    while c < n:
        e = c
        while e < n and (settings[e] is None) == (settings[c] is None):
            e += 1
        run = settings[c:e]
        if settings[c] is None:
            ok = b.drop(first + c, e - c)
        else:
            ok = b.set(np.asarray([s[0] for s in run], F), np.asarray([s[1] for s in run], F), np.asarray([s[2] for s in run], np.uint32),
                       first_channel=first + c)
        assert ok is not False
        c = e


def mixed(n, seed):
    """channel c gets mode c % 5 (4: no node): a lane's four channels hold different modes and every wave holds all of them, absent
    ones among them; sliders from small sets"""
    rng = np.random.default_rng(seed)
    return [None if c % 5 == 4 else (float(rng.choice(MIX_AMPS)), float(rng.choice(MIX_FREQS)), c % 5) for c in range(n)]


def device(dspfx, torch, x, tile):
    return torch.from_numpy(dspfx.to_layout(np.ascontiguousarray(x, F), tile).reshape(-1).copy()).cuda()


def host(dspfx, t, nf, n, tile):
    return dspfx.from_layout(t.cpu().numpy(), nf, n, tile)


def run(dspfx, torch, bank, nf, add_to=None, amplitude=None, frequency=None, inplace=False):
    """one run of the bank -> [nf][N] on the host; the blocks given are [nf][N] host arrays"""
    n, tile = bank.channels, bank.tile_channels
    dev = [None if b is None else device(dspfx, torch, b, tile) for b in (add_to, amplitude, frequency)]
    out = dev[0] if inplace else torch.full((nf * n,), float("nan"), dtype=torch.float32, device="cuda")
    dy = bank.run(nf, out, add_to=dev[0], amplitude=dev[1], frequency=dev[2])
    torch.cuda.synchronize()
    return host(dspfx, dy, nf, n, tile)


def noise(n, nf, seed):
    return O.noise(seed, np.arange(n), np.arange(nf))


def held_to_the_restatement(got, want, modes, what):
    """the engine's bars: 0 ulp for Triangle, Square and Constant and without a node, SINE_ULP for Sine"""
    d = ulp_diff(got, want)
    sine = np.asarray(modes) == R.SINE
    assert np.array_equal(bits(got[:, ~sine]), bits(want[:, ~sine])), what
    if sine.any():
        print(f"{what}: Sine at most {int(d[:, sine].max())} ulp from the restatement (bar {SINE_ULP})")
        assert d[:, sine].max() <= SINE_ULP, (what, int(d[:, sine].max()))


# ---- 1. a fresh bank -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_a_fresh_bank_writes_zeros_and_copies_add_to(dspfx, torch_cuda, n, tile, nf):
    bank = dspfx.ChannelGenerators(n, tile_channels=tile, max_frames=256)
    assert not bits(run(dspfx, torch_cuda, bank, nf)).any(), "+0.0 everywhere"
    base = noise(n, nf, 5)
    base[0, 0] = -0.0
    base.view(np.uint32)[nf // 2, n // 2] = 0x7FC12345                       # a NaN with a payload
    base.view(np.uint32)[nf - 1, n - 1] = 0xFFC00001
    for inplace in (False, True):
        assert np.array_equal(bits(run(dspfx, torch_cuda, bank, nf, add_to=base, inplace=inplace)), bits(base)), "add_to's very bits"
    assert not bank.present().any() and (bank.modes() == dspfx.GENS_NONE).all()
    assert not bank.sliders().any() and bank.sliders().shape == (n, 2)
    assert not bits(bank.clocks().cpu().numpy()).any() and tuple(bank.clocks().shape) == (n,)
    bank.close()


# ---- 2. one setting everywhere equals that engine ------------------------------------------------------------------------
@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_one_setting_everywhere_equals_that_engine(dspfx, torch_cuda, n, tile, nf):
    """the four modes at the (frequency, amplitude) pairs of test_signal_gen_modes, three consecutive runs each, so the clock
    carries; a drop between the settings, so each starts at clock 0 as its engine does"""
    torch = torch_cuda
    bank = dspfx.ChannelGenerators(n, tile_channels=tile, max_frames=256)
    for mode in range(4):
        for freq, amp in PAIRS:
            bank.drop()
            bank.set(amp, freq, mode)
            want = engine_col(dspfx, torch, (amp, freq, mode), (nf,) * 3)
            for k in range(3):
                got = run(dspfx, torch, bank, nf)
                assert np.array_equal(bits(got), bits(np.repeat(want[k * nf:(k + 1) * nf, None], n, axis=1))), f"N={n} tile={tile} nf={nf} run {k} {(amp, freq, mode)}"
            assert (bank.modes() == mode).all() and bank.present().all()
            assert np.array_equal(bits(bank.sliders()), bits(np.tile(F([amp, freq]), (n, 1))))
    bank.close()


# ---- 3. a mixed bank -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("n,tile", SHAPES + [(13 * 256, 256)])
def test_mixed_bank_every_channel_equals_the_engine_of_its_own_setting(dspfx, torch_cuda, n, tile, nf):
    """mode c % 5 with sliders per channel, over two runs; then the same settings sorted by mode, so that whole waves share one:
    the same bits per channel"""
    torch = torch_cuda
    settings = mixed(n, 30 + n)
    want = expected(dspfx, torch, settings, (nf, nf))
    bank = dspfx.ChannelGenerators(n, tile_channels=tile, max_frames=256)
    store(bank, settings)
    modes = np.asarray([R.NONE if s is None else s[2] for s in settings], np.uint32)
    assert np.array_equal(bank.modes(), modes) and np.array_equal(bank.present(), (modes != R.NONE).astype(np.uint32))
    got = np.concatenate([run(dspfx, torch, bank, nf) for _ in range(2)])
    assert np.array_equal(bits(got), bits(want)), f"N={n} tile={tile} nf={nf} interleaved"
    bank.close()
    order = np.argsort(modes.astype(np.int64), kind="stable")
    srt = dspfx.ChannelGenerators(n, tile_channels=tile, max_frames=256)
    store(srt, [settings[c] for c in order])
    got = np.concatenate([run(dspfx, torch, srt, nf) for _ in range(2)])
    assert np.array_equal(bits(got), bits(want[:, order])), f"N={n} tile={tile} nf={nf} sorted"
    srt.close()


@pytest.mark.parametrize("n,tile", [(256, 0), (256, 64)])
def test_the_tiled_and_the_frame_major_bank_agree(dspfx, torch_cuda, n, tile):
    torch = torch_cuda
    settings = mixed(n, 33)
    base = noise(n, 37, 6)
    outs = []
    for t in (0, 64):
        bank = dspfx.ChannelGenerators(n, tile_channels=t, max_frames=NF)
        store(bank, settings)
        outs.append(np.concatenate([run(dspfx, torch, bank, NF), run(dspfx, torch, bank, 37, add_to=base)]))
        bank.close()
    assert np.array_equal(bits(outs[0]), bits(outs[1]))


# ---- 4. neighbours ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", THREE)
def test_a_channels_bits_do_not_depend_on_its_neighbours(dspfx, torch_cuda, n, tile):
    """the kept channels (one of each lane's four, and the last) get the same settings in two banks; every other channel differs in
    mode, in sliders or in presence, or carries NaN sliders"""
    torch = torch_cuda
    keep = np.zeros(n, bool)
    keep[(np.arange(n) % 4) == (np.arange(n) // 4) % 4] = True
    keep[n - 1] = True
    sa = mixed(n, 40 + n)
    other = mixed(n + 2, 41 + n)[2:]                              # the modes shifted by two, other sliders
    sb = [sa[c] if keep[c] else other[c] for c in range(n)]
    for c in np.flatnonzero(~keep)[::3]:
        sb[c] = (float("nan"), float("nan"), int(c) % 4)
    a = dspfx.ChannelGenerators(n, tile_channels=tile, max_frames=NF)
    b = dspfx.ChannelGenerators(n, tile_channels=tile, max_frames=NF)
    store(a, sa)
    store(b, sb)
    ya = np.concatenate([run(dspfx, torch, a, NF) for _ in range(2)])
    yb = np.concatenate([run(dspfx, torch, b, NF) for _ in range(2)])
    assert np.array_equal(bits(ya), bits(expected(dspfx, torch, sa, (NF, NF)))), "bank a"
    assert np.array_equal(bits(ya[:, keep]), bits(yb[:, keep]))
    assert not np.array_equal(bits(ya[:, ~keep]), bits(yb[:, ~keep]))
    a.close()
    b.close()


# ---- 5. add_to -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_add_to_is_one_f32_addition_in_place_or_not(dspfx, torch_cuda, n, tile, nf):
    torch = torch_cuda
    settings = mixed(n, 50 + n)
    base = noise(n, nf, 9) * F(0.75)
    base[0, 0] = -0.0
    sample = expected(dspfx, torch, settings, (nf,))
    present = np.asarray([s is not None for s in settings])
    want = np.where(present, (base + sample).astype(F), base)
    outs = []
    for inplace in (False, True):
        bank = dspfx.ChannelGenerators(n, tile_channels=tile, max_frames=256)
        store(bank, settings)
        outs.append(run(dspfx, torch, bank, nf, add_to=base, inplace=inplace))
        bank.close()
    assert np.array_equal(bits(outs[0]), bits(want)), "add_to + the engine's sample, np.float32"
    assert np.array_equal(bits(outs[0][:, ~present]), bits(base[:, ~present])), "no node: add_to's bits"
    assert np.array_equal(bits(outs[1]), bits(outs[0])), "in place equals out of place"


# ---- 6. control ports ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ports", [(0,), (1,), (0, 1)])
@pytest.mark.parametrize("n,tile", THREE)
def test_ports_against_the_restatement_and_no_latch(dspfx, torch_cuda, n, tile, ports):
    """test_signal_gen_control_ports_and_state's blocks (noise on the amplitude, the frequency around 1 kHz) on a mixed bank: a
    run of 128 and one of 37 with the ports, then a run without, which goes by the stored sliders.  The port blocks hold NaN in the
    channels without a node: it reaches nothing"""
    torch = torch_cuda
    settings = mixed(n, 60 + n)
    modes = [R.NONE if s is None else s[2] for s in settings]
    absent = np.asarray([s is None for s in settings])
    bank, ref = dspfx.ChannelGenerators(n, tile_channels=tile, max_frames=NF), R.ChannelGenerators(n)
    store(bank, settings)
    store(ref, settings)
    f0 = 0
    for nf in (NF, 37):
        ca = (noise(n, nf, 31 + f0) * F(1.3)).astype(F)
        cf = (noise(n, nf, 32 + f0) * F(0.02) - F(0.9)).astype(F)
        ca[:, absent] = np.nan
        cf[:, absent] = np.nan
        kw = dict(amplitude=ca if 0 in ports else None, frequency=cf if 1 in ports else None)
        got, want = run(dspfx, torch, bank, nf, **kw), ref.run(nf, **kw)
        assert not bits(got[:, absent]).any(), "no node: +0.0, whatever the port blocks hold"
        held_to_the_restatement(got, want, modes, f"N={n} tile={tile} ports {ports} nf={nf}")
        f0 += 100
    assert np.array_equal(bits(bank.sliders()), bits(ref.sliders())), "the stored sliders are untouched"
    assert np.array_equal(bits(bank.clocks().cpu().numpy()), bits(ref.clocks()))
    got, want = run(dspfx, torch, bank, NF), ref.run(NF)
    held_to_the_restatement(got, want, modes, f"N={n} tile={tile} after ports {ports}")
    const = [c for c, s in enumerate(settings) if s is not None and s[2] == R.CONSTANT]
    assert np.array_equal(bits(got[:, const]), bits(np.tile(F([settings[c][0] for c in const]), (NF, 1)))), "Constant: the stored amplitude"
    bank.close()


# ---- 7. stores -------------------------------------------------------------------------------------------------------------
def test_stores_between_submitted_runs_drop_set_and_reset(dspfx, torch_cuda):
    """nothing waits between the calls; everything is read at the end.  Triangle, Square and Constant only, so that the restatement
    is the expectation bit for bit; a Sine channel rides along for its clock"""
    torch = torch_cuda
    n, tile = 256, 64
    bank, ref = dspfx.ChannelGenerators(n, tile_channels=tile, max_frames=NF), R.ChannelGenerators(n)
    dys = [torch.full((NF * n,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(6)]
    torch.cuda.synchronize()
    wants = []

    def both(call):
        for b in (bank, ref):
            assert call(b) is not False

    def submit(i, nf=NF):
        bank.run(nf, dys[i])
        wants.append(ref.run(nf))

    both(lambda b: b.set(0.5, 441.0, R.TRIANGLE))
    both(lambda b: b.set(mode=R.SINE, first_channel=255, count=1))
    submit(0)
    both(lambda b: b.set(-1.0, 12000.0, R.SQUARE, first_channel=0, count=128))        # a store after a submitted run does not change it
    submit(1, 37)
    both(lambda b: b.drop(64, 64))
    both(lambda b: b.set(frequency=19999.0, mode=R.TRIANGLE, first_channel=96, count=64))  # 96 .. 127 restart at clock 0 from the defaults, 128 .. 159 keep their phase
    submit(2)
    both(lambda b: b.reset(0, 32))
    both(lambda b: b.set(amplitude=0.25, mode=R.CONSTANT, first_channel=200, count=20))
    submit(3)
    both(lambda b: b.set(mode=R.TRIANGLE, first_channel=200, count=20))                # Constant left the clock alone
    submit(4)
    both(lambda b: b.drop(64, 1))
    assert bank.present()[64] == 0, "the host tables already show the drop"
    submit(5)
    torch.cuda.synchronize()
    sine = np.arange(n) == 255
    for i, want in enumerate(wants):
        got = host(dspfx, dys[i][:len(want) * n], len(want), n, tile)
        assert np.array_equal(bits(got[:, ~sine]), bits(want[:, ~sine])), f"run {i}"
        assert ulp_diff(got[:, sine], want[:, sine]).max() <= SINE_ULP
    assert not bits(host(dspfx, dys[2], NF, n, tile)[:, 64:96]).any(), "dropped: +0.0"
    assert np.array_equal(bits(bank.clocks().cpu().numpy()), bits(ref.clocks())), "clocks() equals the restatement's"
    assert np.array_equal(bank.present(), ref.present()) and np.array_equal(bank.modes(), ref.modes())
    assert np.array_equal(bits(bank.sliders()), bits(ref.sliders()))
    assert list(bank.sliders()[96]) == [0.5, F(19999.0)] and list(bank.sliders()[128]) == [0.5, F(19999.0)] and list(bank.sliders()[0]) == [-1.0, 12000.0]
    # the restart at clock 0 beside a neighbour that kept its phase, against the engine
    got2 = host(dspfx, dys[2], NF, n, tile)
    assert np.array_equal(bits(got2[:, 100]), bits(engine_col(dspfx, torch, (0.5, 19999.0, R.TRIANGLE), (NF,))))
    assert not np.array_equal(bits(got2[:, 130]), bits(got2[:, 100]))
    bank.close()


def test_a_refused_store_changes_nothing(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile = 70, 0
    settings = mixed(n, 71)
    bank, ref = dspfx.ChannelGenerators(n, tile_channels=tile, max_frames=NF), R.ChannelGenerators(n)
    store(bank, settings)
    store(ref, settings)
    run(dspfx, torch, bank, NF)
    clocks = bank.clocks().cpu().numpy().copy()
    bad = [(lambda b: b.set(1.0, 1.0, 4), "mode"), (lambda b: b.set(1.0, 1.0, np.r_[np.zeros(n - 1, np.uint32), 77]), "mode"),
           (lambda b: b.set(1.0, first_channel=n - 1, count=2), "channels"), (lambda b: b.set(1.0, first_channel=n + 1, count=0), "channels"),
           (lambda b: b.set(1.0, first_channel=0, count=n + 1), "channels"), (lambda b: b.drop(n, 1), "channels"), (lambda b: b.reset(n - 3, 4), "channels")]
    for call, word in bad:
        with pytest.raises(dspfx.DspfxError) as e:
            call(bank)
        assert e.value.status == -1 and word in str(e.value) and "gens" in str(e.value), str(e.value)
        assert call(ref) is False
    with pytest.raises(dspfx.DspfxError):
        bank.present(1, n)
    with pytest.raises(dspfx.DspfxError):
        bank.run(2 * NF, torch.empty(2 * NF * n, dtype=torch.float32, device="cuda"))
    with pytest.raises(dspfx.DspfxError):
        bank.run(0, torch.empty(n, dtype=torch.float32, device="cuda"))
    assert np.array_equal(bank.modes(), ref.modes()) and np.array_equal(bank.present(), ref.present()) and np.array_equal(bits(bank.sliders()), bits(ref.sliders()))
    got = np.concatenate([run(dspfx, torch, bank, NF)])
    assert np.array_equal(bits(got), bits(expected(dspfx, torch, settings, (NF, NF))[NF:])), "the second run of the unchanged settings"
    assert not np.array_equal(bits(bank.clocks().cpu().numpy()), bits(clocks))
    bank.close()


def test_a_thread_storing_whole_range_settings_while_blocks_are_submitted(dspfx, torch_cuda):
    """two settings of one frequency, so the clock of run i is the same under either: every block equals the all-old or the all-new
    expectation of its run -- a store is whole"""
    torch = torch_cuda
    n, tile, runs = 256, 64, 60
    old, new = (0.5, 441.0, R.TRIANGLE), (-1.0, 441.0, R.SINE)
    wants = [engine_col(dspfx, torch, s, (NF,) * runs).reshape(runs, NF) for s in (old, new)]
    bank = dspfx.ChannelGenerators(n, tile_channels=tile, max_frames=NF)
    store(bank, [old] * n)
    dys = [torch.full((NF * n,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(runs)]
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
        bank.run(NF, dys[i])
    done.set()
    t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for i in range(runs):
        got = bits(host(dspfx, dys[i], NF, n, tile))
        which = [np.array_equal(got, bits(np.repeat(w[i][:, None], n, axis=1))) for w in wants]
        assert any(which), f"run {i} is neither all old nor all new"
    bank.close()


# ---- 8. edge sliders -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", range(4))
def test_edge_sliders(dspfx, torch_cuda, mode):
    """frequency and amplitude from NaN, both infinities, signed zeros, a subnormal, 1e12 (sin_cr's library branch) and -100, every
    pair in a channel of its own, two runs: the engine's bits, and the restatement's at the engine's bars where it is finite"""
    torch = torch_cuda
    n = len(EDGE) ** 2
    settings = [(EDGE[c // len(EDGE)], EDGE[c % len(EDGE)], mode) for c in range(n)]
    bank, ref = dspfx.ChannelGenerators(n, max_frames=NF), R.ChannelGenerators(n)
    store(bank, settings)
    store(ref, settings)
    assert np.array_equal(bits(bank.sliders()), bits(ref.sliders())), "values are taken as given"
    got = np.concatenate([run(dspfx, torch, bank, NF) for _ in range(2)])
    E.same_bits_or_nan(got, expected(dspfx, torch, settings, (NF, NF)), None, f"mode {mode} against the engine")
    want = np.concatenate([ref.run(NF) for _ in range(2)])
    fin = np.isfinite(want)
    assert np.isfinite(got[fin]).all()
    d = ulp_diff(got[fin], want[fin])
    print(f"mode {mode}: {int(fin.sum())} finite samples of {fin.size}, at most {int(d.max())} ulp from the restatement")
    assert d.max() <= (SINE_ULP if mode == R.SINE else 0)
    bank.close()


# ---- 9. the oracle ---------------------------------------------------------------------------------------------------------
def test_against_the_oracle_through_the_restatement(dspfx, torch_cuda):
    """all four modes and no node side by side, six blocks of 128 in runs of 128, 256 and 384 frames"""
    torch = torch_cuda
    n, tile = 256, 64
    settings = mixed(n, 90)
    modes = [R.NONE if s is None else s[2] for s in settings]
    bank, ref = dspfx.ChannelGenerators(n, tile_channels=tile, max_frames=384), R.ChannelGenerators(n)
    store(bank, settings)
    store(ref, settings)
    for nf in (128, 256, 384):
        held_to_the_restatement(run(dspfx, torch, bank, nf), ref.run(nf), modes, f"a run of {nf} frames")
    assert np.array_equal(bits(bank.clocks().cpu().numpy()), bits(ref.clocks()))
    bank.close()


# ---- 10. full size ---------------------------------------------------------------------------------------------------------
def test_full_size(dspfx, torch_cuda):
    """2^20 channels x 128 frames, tiled 256; two alternating output buffers, device events, median of 20 after 5 warm-ups.
    Asserted: a Sine-everywhere bank and a Triangle-everywhere bank each take at most twice their Engine([SignalGen]) on the same
    buffers, timed here (twice is the margin every bank here gets over its engine), and equal it bit for bit after the same number
    of runs; a bank clustered by spans of 256 channels over the four modes fits the 2.667 ms a 128-frame block lasts at 48 kHz.
    Printed, not asserted: the interleaved bank (c % 4) and a run with add_to; milliseconds, the fraction of 8 TB/s on the run's
    own bytes (one block-unit written, two with add_to), a flat device write of the same bytes."""
    torch = torch_cuda
    n, nf, tile = 1 << 20, 128, 256
    xs = [torch.zeros(nf * n, dtype=torch.float32, device="cuda") for _ in range(2)]
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

    assert dspfx.gens_plan(n) == 13 * n
    bank = dspfx.ChannelGenerators(n, tile_channels=tile, max_frames=nf)
    times = {}
    for name, mode in (("Sine", dspfx.SIG_SINE), ("Triangle", dspfx.SIG_TRIANGLE)):
        bank.set(0.5, 441.0, mode)
        bank.reset()
        t_bank = timed(lambda i: bank.run(nf, ys[i % 2]))
        torch.cuda.synchronize()
        mine = ys[1].clone()
        eng = dspfx.Engine(n, nf, link_flags=0, tile_channels=tile)
        eng.set_chain([dspfx.SignalGen(0.5, 441.0, mode)])
        t_eng = timed(lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=nf))
        torch.cuda.synchronize()
        assert torch.equal(mine.view(torch.int32), ys[1].view(torch.int32)), f"{name}: the bank's bits are the engine's"
        eng.close()
        times[name] = (t_bank, t_eng)
    span = np.arange(n) // 256
    bank.set(mode=(span % 4).astype(np.uint32))
    t_cluster = timed(lambda i: bank.run(nf, ys[i % 2]))
    bank.set(mode=(np.arange(n) % 4).astype(np.uint32))
    t_mixed = timed(lambda i: bank.run(nf, ys[i % 2]))
    t_add = timed(lambda i: bank.run(nf, ys[i % 2], add_to=xs[i % 2]))
    bank.close()
    t_write = timed(lambda i: ys[i % 2].fill_(0.25))
    frac = lambda t, units=1: units * unit / t / 1e9 / 8.0      # noqa: E731
    print(f"full size generators, one box, one run, {unit / 2**20:.0f} MiB written: "
          + ", ".join(f"{name} {tb:.4f} ms ({frac(tb):.3f} of 8 TB/s; Engine([SignalGen]) {te:.4f} ms, bank x {tb / te:.3f})" for name, (tb, te) in times.items())
          + f", clustered by spans of 256 over the four modes {t_cluster:.4f} ms ({frac(t_cluster):.3f}), interleaved c % 4 {t_mixed:.4f} ms "
          f"({frac(t_mixed):.3f}), interleaved with add_to {t_add:.4f} ms ({frac(t_add, 2):.3f} on two units), flat write of the same bytes {t_write:.4f} ms")
    for name, (tb, te) in times.items():
        assert tb <= 2 * te, (name, tb, te)
    assert t_cluster * 1e-3 <= 128 / 48000, t_cluster
