"""The channel-blend bank on the GPU (dspfx_blends_*, through the Python class): per-channel Add and Mix nodes, sends and buses.  A
channel's output is compared bit for bit with Engine([Mix(r)], link_flags=0).process(a, side=b) or Engine([Add()], link_flags=0) of
its own setting -- with a send, fed b that has gone through Engine([Gain(level)]) -- and with blends_ref, the restatement made of the
oracle's numpy nodes.  Where the expectation is a NaN the bank must give a NaN; its sign and payload are not compared
(edge_values.same_bits_or_nan).  Outputs start as NaN everywhere, so every sample is shown to be written."""
import threading

import numpy as np
import pytest

import blends_ref as R
import edge_values as E
import oracle as O

pytestmark = pytest.mark.gpu

NF = 128
F = np.float32
SHAPES = [(64, 0), (256, 64), (70, 0), (1, 0)]                   # vector lanes; tiled; scalar accesses and a ragged last workgroup; one channel
THREE = [(64, 0), (256, 64), (70, 0)]
FRAMES = [1, 37, 128, 256]                                       # 256 on a bank of max_frames 256
RATIOS = (0.0, 0.25, 0.5, 1.0, 1.5, -0.5, float("nan"))
MIX_RATIOS = (0.25, 0.5, 1.5)
MIX_LEVELS = (0.5, 2.0)
NO_BUS = R.NO_BUS


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_ENG = {}


@pytest.fixture(scope="module", autouse=True)
def engines():
    yield
    for e in _ENG.values():
        e.close()
    _ENG.clear()


def engine(dspfx, torch, kind, value, a, side=None, ctl=None, fresh=False):
    """what Engine([node], link_flags=0) writes from the frame-major blocks a and side -> [nf][n].  kind "add", "mix" (value: the
    ratio) or "gain" (value: the level); one engine per (kind, n), its slider stored for every call (a store also ends a latch)"""
    nf, n = a.shape
    key = (kind, n)
    if fresh or key not in _ENG:
        eng = dspfx.Engine(n, 256, link_flags=0)
        eng.set_chain([{"add": dspfx.Add, "mix": dspfx.Mix, "gain": dspfx.Gain}[kind]()])
        if fresh:
            key = (kind, n, "fresh")
            if key in _ENG:
                _ENG[key].close()
        _ENG[key] = eng
    eng = _ENG[key]
    if kind != "add":
        eng.set_param(0, 0, float(value))
    dev = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x, F).reshape(-1).copy()).cuda()      # noqa: E731
    dx, ds, dc = dev(a), dev(side), dev(ctl)
    dy = torch.full_like(dx, float("nan"))
    eng.process(dx, out=dy, side=ds, n_frames=nf, ctl={(0, 0): dc} if dc is not None else None)
    torch.cuda.synchronize()
    return dy.cpu().numpy().reshape(nf, n)


def expected(dspfx, torch, settings, a, B):
    """channel c as the engine of its own setting gives it; settings[c] = None or (kind, ratio, level or None); B the N-channel
    second input or None.  One engine run per distinct setting, one Gain run per distinct level"""
    want = a.copy()
    zero = np.zeros_like(a)
    gained, runs = {}, {}
    for c, s in enumerate(settings):
        if s is None:
            continue
        kind, r, level = s
        key = (kind, None if kind == "add" else bits(F(r)).item(), None if level is None else bits(F(level)).item())
        if key not in runs:
            side = B
            if level is not None:
                if key[2] not in gained:
                    gained[key[2]] = engine(dspfx, torch, "gain", level, zero if B is None else B)
                side = gained[key[2]]
            runs[key] = engine(dspfx, torch, kind, r, a, side)
        want[:, c] = runs[key][:, c]
    return want


def store(b, settings, first=0):
    """the settings onto a bank or its restatement, a channel at a time where they differ"""
    c, n = 0, len(settings)
    while c < n:
        e = c
        while e < n and settings[e] == settings[c]:
            e += 1
        s = settings[c]
        if s is None:
            ok = b.drop(first + c, e - c)
        else:
            ok = b.set_add(first + c, e - c) if s[0] == "add" else b.set_mix(s[1], first + c, e - c)
            assert ok is not False
            ok = b.set_send(s[2], first + c, e - c)
        assert ok is not False
        c = e


def mixed(n, seed):
    """channel c gets kind c % 3 (0: no node, 1: Add, 2: Mix), a send on every other present channel, values from small sets"""
    rng = np.random.default_rng(seed)
    out, present = [], 0
    for c in range(n):
        if c % 3 == 0:
            out.append(None)
            continue
        level = float(rng.choice(MIX_LEVELS)) if present % 2 else None
        present += 1
        out.append(("add", None, level) if c % 3 == 1 else ("mix", float(rng.choice(MIX_RATIOS)), level))
    return out


def device(dspfx, torch, x, tile):
    return torch.from_numpy(dspfx.to_layout(np.ascontiguousarray(x, F), tile).reshape(-1).copy()).cuda()


def host(dspfx, t, nf, n, tile):
    return dspfx.from_layout(t.cpu().numpy(), nf, n, tile)


def run(dspfx, torch, bank, a, b=None, bus=None, ratio=None, inplace=None):
    """one run of the bank -> [nf][N] on the host; a, b, ratio are [nf][N] host arrays, bus [nf][G]; inplace: out is "a" or "b" itself"""
    n, tile, nf = bank.channels, bank.tile_channels, a.shape[0]
    da, db, dr = [None if x is None else device(dspfx, torch, x, tile) for x in (a, b, ratio)]
    dbus = None if bus is None else torch.from_numpy(np.ascontiguousarray(bus, F).reshape(-1).copy()).cuda()
    out = da if inplace == "a" else db if inplace == "b" else torch.full((nf * n,), float("nan"), dtype=torch.float32, device="cuda")
    dy = bank.run(da, nf, b=db, bus=dbus, ratio=dr, out=out)
    torch.cuda.synchronize()
    return host(dspfx, dy, nf, n, tile)


def noise(n, nf, seed, scale=1.0):
    return (O.noise(seed, np.arange(n), np.arange(nf)) * F(scale)).astype(F)


def special(a):
    """NaN payloads, -0.0 and subnormals into a block"""
    nf, n = a.shape
    a[0, 0] = -0.0
    a.view(np.uint32)[nf // 2, n // 2] = 0x7FC12345
    a.view(np.uint32)[nf - 1, n - 1] = 0xFFC00001
    a.view(np.uint32)[nf // 3, n // 3] = 0x00000001
    a.view(np.uint32)[(2 * nf) // 3, (2 * n) // 3] = 0x807FFFFF
    return a


def gathered(bus, ids):
    """B[f][c] = bus[f][ids[c]], +0.0 on NO_BUS"""
    ids = np.asarray(ids, np.int64)
    B = np.zeros((bus.shape[0], len(ids)), F)
    on = ids != NO_BUS
    B[:, on] = bus[:, ids[on]]
    return B


def tables(b):
    return [np.asarray(t).copy() for t in (b.kinds(), b.ratios(), *b.sends(), b.bus_of())]


def same_tables(u, v):
    return all(np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y) for x, y in zip(u, v))


# ---- 1. a fresh bank -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_a_fresh_bank_copies_a_in_all_three_input_modes(dspfx, torch_cuda, n, tile, nf):
    bank = dspfx.ChannelBlends(n, buses=3, tile_channels=tile, max_frames=256)
    a = special(noise(n, nf, 5))
    b, bus = noise(n, nf, 6), noise(3, nf, 7)
    b[0, 0] = np.nan
    for kw in (dict(), dict(b=b), dict(bus=bus), dict(b=b, ratio=b), dict(inplace="a"), dict(b=b, inplace="b")):
        assert np.array_equal(bits(run(dspfx, torch_cuda, bank, a, **kw)), bits(a)), f"a's very bits, {sorted(kw)}"
    assert (bank.kinds() == dspfx.BLENDS_NONE).all() and not bank.ratios().any() and (bank.bus_of() == dspfx.BLENDS_NO_BUS).all()
    assert not bank.sends()[0].any() and not bank.sends()[1].any()
    bank.close()


# ---- 2. one setting everywhere equals that engine ------------------------------------------------------------------------
@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_one_setting_everywhere_equals_that_engine(dspfx, torch_cuda, n, tile, nf):
    """Add, and Mix at every ratio of the issue's set, with b and with b unconnected; b holds an infinity, so Mix at r = 0 gives
    the engine's NaN"""
    torch = torch_cuda
    a, b = special(noise(n, nf, 11)), noise(n, nf, 12, 0.75)
    b[nf // 2, 0] = np.inf
    bank = dspfx.ChannelBlends(n, tile_channels=tile, max_frames=256)
    for side in (b, None):
        bank.set_add()
        E.same_bits_or_nan(run(dspfx, torch, bank, a, b=side), engine(dspfx, torch, "add", None, a, side), None, f"Add N={n} tile={tile} nf={nf}")
        assert (bank.kinds() == dspfx.ADD).all()
        for r in RATIOS:
            bank.set_mix(r)
            got = run(dspfx, torch, bank, a, b=side)
            E.same_bits_or_nan(got, engine(dspfx, torch, "mix", r, a, side), None, f"Mix({r}) N={n} tile={tile} nf={nf} side={side is not None}")
            assert (bank.kinds() == dspfx.MIX).all() and np.array_equal(bits(bank.ratios()), bits(np.full(n, r, F)))
    bank.set_mix(0.0)
    assert np.isnan(run(dspfx, torch, bank, a, b=b)[nf // 2, 0]), "every weight is a multiplication: 0 * inf"
    bank.close()


@pytest.mark.parametrize("n,tile", THREE)
def test_the_control_block_equals_a_fresh_engines_first_block_and_is_not_latched(dspfx, torch_cuda, n, tile):
    torch = torch_cuda
    a, b = special(noise(n, NF, 13)), noise(n, NF, 14, 0.75)
    ctl = noise(n, NF, 15, 1.6)
    ctl[3, :], ctl[4, :], ctl[5, :] = -1.5, 1.25, np.nan
    assert np.nanmin(ctl) < -1 and np.nanmax(ctl) > 1
    bank = dspfx.ChannelBlends(n, tile_channels=tile, max_frames=NF)
    bank.set_mix(0.3)
    got = run(dspfx, torch, bank, a, b=b, ratio=ctl)
    E.same_bits_or_nan(got, engine(dspfx, torch, "mix", 0.3, a, b, ctl, fresh=True), None, f"ratio block N={n} tile={tile}")
    assert np.isnan(got[5]).all()
    assert np.array_equal(bits(bank.ratios()), bits(np.full(n, 0.3, F))), "the stored ratio is untouched"
    E.same_bits_or_nan(run(dspfx, torch, bank, a, b=b), engine(dspfx, torch, "mix", 0.3, a, b), None, "a later run without the block: the stored ratio")
    bank.close()


# ---- 3. a mixed bank -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("n,tile", SHAPES + [(13 * 256, 256)])
def test_mixed_bank_every_channel_equals_the_restatement_and_the_engine_of_its_own_setting(dspfx, torch_cuda, n, tile, nf):
    torch = torch_cuda
    settings = mixed(n, 30 + n)
    a, b = special(noise(n, nf, 21)), noise(n, nf, 22, 0.75)
    bank, ref = dspfx.ChannelBlends(n, tile_channels=tile, max_frames=256), R.ChannelBlends(n, max_frames=256)
    store(bank, settings)
    store(ref, settings)
    assert same_tables(tables(bank), tables(ref))
    for side in (b, None):
        got = run(dspfx, torch, bank, a, b=side)
        E.same_bits_or_nan(got, ref.run(a, b=side), None, f"restatement N={n} tile={tile} nf={nf}")
        E.same_bits_or_nan(got, expected(dspfx, torch, settings, a, side), None, f"engines N={n} tile={tile} nf={nf}")
        absent = [c for c, s in enumerate(settings) if s is None]
        assert np.array_equal(bits(got[:, absent]), bits(a[:, absent])), "no node: a's very bits"
    bank.close()


# ---- 4. bus mode -----------------------------------------------------------------------------------------------------------
def bus_ids(n, G, how):
    if how == "spans":
        ids = np.minimum(np.arange(n) // max(1, -(-n // G)), G - 1)
    elif how == "rooms64":
        ids = (np.arange(n) // 64) % G
    elif how == "interleaved":
        ids = np.arange(n) % G
    else:
        ids = np.random.default_rng(n + G).permutation(np.arange(n) % G)
    ids = ids.astype(np.uint32)
    if how == "fifth":
        ids[::5] = NO_BUS
    return ids


@pytest.mark.parametrize("how", ["spans", "rooms64", "interleaved", "permutation", "fifth"])
@pytest.mark.parametrize("G", [1, 3, 4])
@pytest.mark.parametrize("n,tile", SHAPES)
def test_bus_mode_equals_block_mode_on_the_gathered_block(dspfx, torch_cuda, n, tile, G, how):
    """contiguous spans, contiguous rooms of 64, interleaved c % G, a random permutation, NO_BUS on every fifth channel; on a mixed
    bank and on a Mix-everywhere bank (whole waves of one id take the wave-uniform path); 37 and 128 frames"""
    torch = torch_cuda
    ids = bus_ids(n, G, how)
    for settings in (mixed(n, 40 + n), [("mix", 0.25, 0.5)] * n):
        bank, ref = dspfx.ChannelBlends(n, buses=G, tile_channels=tile, max_frames=NF), R.ChannelBlends(n, buses=G)
        store(bank, settings)
        store(ref, settings)
        bank.assign(ids)
        assert ref.assign(ids) and np.array_equal(bank.bus_of(), ids)
        for nf in (37, NF):
            a, bus = special(noise(n, nf, 41)), noise(G, nf, 42, 0.75)
            got = run(dspfx, torch, bank, a, bus=bus)
            E.same_bits_or_nan(got, run(dspfx, torch, bank, a, b=gathered(bus, ids)), None, f"block mode N={n} tile={tile} G={G} {how} nf={nf}")
            E.same_bits_or_nan(got, ref.run(a, bus=bus), None, f"restatement N={n} tile={tile} G={G} {how} nf={nf}")
        bank.close()


def test_an_id_moved_between_two_submitted_runs_governs_only_the_later_run(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile, G = 256, 64, 4
    bank = dspfx.ChannelBlends(n, tile_channels=tile, max_frames=NF, group_size=64)
    assert bank.buses == G and np.array_equal(bank.bus_of(), np.arange(n) // 64)
    bank.set_add()
    a, bus = noise(n, NF, 43), noise(G, NF, 44)
    da = device(dspfx, torch, a, tile)
    dbus = torch.from_numpy(bus.reshape(-1).copy()).cuda()
    dys = [torch.full((NF * n,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    bank.run(da, NF, bus=dbus, out=dys[0])
    bank.assign([3, NO_BUS], 10)
    bank.run(da, NF, bus=dbus, out=dys[1])
    torch.cuda.synchronize()
    ids = np.arange(n) // 64
    assert np.array_equal(bits(host(dspfx, dys[0], NF, n, tile)), bits((a + gathered(bus, ids)).astype(F))), "the run submitted before the assign"
    ids[10], ids[11] = 3, NO_BUS
    assert np.array_equal(bits(host(dspfx, dys[1], NF, n, tile)), bits((a + gathered(bus, ids)).astype(F))), "the run submitted after it"
    bank.close()


# ---- 5. layouts, neighbours, in place --------------------------------------------------------------------------------------
def test_the_tiled_and_the_frame_major_bank_agree(dspfx, torch_cuda):
    torch = torch_cuda
    n, G = 256, 4
    settings, ids = mixed(n, 33), bus_ids(n, G, "fifth")
    a, b, bus, ctl = special(noise(n, 37, 51)), noise(n, 37, 52), noise(G, 37, 53), noise(n, 37, 54, 1.5)
    outs = []
    for t in (0, 64):
        bank = dspfx.ChannelBlends(n, buses=G, tile_channels=t, max_frames=NF)
        store(bank, settings)
        bank.assign(ids)
        outs.append(np.concatenate([run(dspfx, torch, bank, a), run(dspfx, torch, bank, a, b=b), run(dspfx, torch, bank, a, bus=bus),
                                    run(dspfx, torch, bank, a, b=b, ratio=ctl), run(dspfx, torch, bank, a, bus=bus, ratio=ctl)]))
        bank.close()
    assert np.array_equal(bits(outs[0]), bits(outs[1]))


@pytest.mark.parametrize("n,tile", THREE)
def test_a_channels_bits_do_not_depend_on_its_neighbours(dspfx, torch_cuda, n, tile):
    """the kept channels (one of each lane's four, and the last) get the same settings, samples and bus in two banks; every other
    channel differs in kind, in values, in its bus or in its samples (NaN among them)"""
    torch = torch_cuda
    G = 3
    keep = np.zeros(n, bool)
    keep[(np.arange(n) % 4) == (np.arange(n) // 4) % 4] = True
    keep[n - 1] = True
    sa = mixed(n, 60 + n)
    other = mixed(n + 1, 61 + n)[1:]                              # the kinds shifted by one, other values
    sb = [sa[c] if keep[c] else other[c] for c in range(n)]
    ia, ib = bus_ids(n, G, "interleaved"), bus_ids(n, G, "permutation")
    ib[keep] = ia[keep]
    a, b, bus = noise(n, NF, 62), noise(n, NF, 63), noise(G, NF, 64)
    a2, b2 = a.copy(), b.copy()
    a2[:, ~keep] = noise(n, NF, 65)[:, ~keep]
    b2[:, ~keep] = np.nan
    outs = []
    for s, ids, x, y in ((sa, ia, a, b), (sb, ib, a2, b2)):
        bank = dspfx.ChannelBlends(n, buses=G, tile_channels=tile, max_frames=NF)
        store(bank, s)
        bank.assign(ids)
        outs.append(np.concatenate([run(dspfx, torch, bank, x, b=y), run(dspfx, torch, bank, x, bus=bus)]))
        bank.close()
    assert np.array_equal(bits(outs[0][:, keep]), bits(outs[1][:, keep]))
    assert not np.array_equal(bits(outs[0][:, ~keep]), bits(outs[1][:, ~keep]))


@pytest.mark.parametrize("nf", [37, NF])
@pytest.mark.parametrize("n,tile", SHAPES)
def test_in_place_equals_out_of_place(dspfx, torch_cuda, n, tile, nf):
    torch = torch_cuda
    settings = mixed(n, 70 + n)
    a, b, bus = special(noise(n, nf, 71)), noise(n, nf, 72), noise(2, nf, 73)
    bank = dspfx.ChannelBlends(n, buses=2, tile_channels=tile, max_frames=NF)
    store(bank, settings)
    bank.assign(bus_ids(n, 2, "interleaved"))
    want = run(dspfx, torch, bank, a, b=b)
    assert np.array_equal(bits(run(dspfx, torch, bank, a, b=b, inplace="a")), bits(want)), "out is a"
    assert np.array_equal(bits(run(dspfx, torch, bank, a, b=b, inplace="b")), bits(want)), "out is b"
    assert np.array_equal(bits(run(dspfx, torch, bank, a, bus=bus, inplace="a")), bits(run(dspfx, torch, bank, a, bus=bus))), "bus mode, out is a"
    bank.close()


# ---- 6. refusals and stores ------------------------------------------------------------------------------------------------
def test_refusals_leave_every_table_unchanged(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile, G = 70, 0, 3
    settings = mixed(n, 81)
    bank, ref = dspfx.ChannelBlends(n, buses=G, tile_channels=tile, max_frames=NF), R.ChannelBlends(n, buses=G)
    plain = dspfx.ChannelBlends(n, tile_channels=tile, max_frames=NF)
    for b in (bank, ref):
        store(b, settings)
        assert b.assign(bus_ids(n, G, "fifth")) is not False
    a, side, bus = noise(n, NF, 82), noise(n, NF, 83), noise(G, NF, 84)
    want = run(dspfx, torch, bank, a, bus=bus)
    before = tables(bank)
    dev = lambda x: torch.from_numpy(x.reshape(-1).copy()).cuda()      # noqa: E731
    da, ds, dbus = dev(a), dev(side), dev(bus)
    big = torch.zeros(2 * NF * n, dtype=torch.float32, device="cuda")
    bad = [(lambda b: b.run(da, NF, b=ds, bus=dbus), "both"), (lambda b: plain.run(da, NF, bus=dbus), "n_buses"),
           (lambda b: b.assign([0, G], 0), "bus"), (lambda b: b.assign(G), "bus"), (lambda b: b.assign([0, 1], n - 1), "channels"),
           (lambda b: b.set_mix(0.1, n - 1, 2), "channels"), (lambda b: b.set_mix(np.zeros(n + 1, F)), "channels"), (lambda b: b.set_add(n + 1, 0), "channels"),
           (lambda b: b.set_send(1.0, 0, n + 1), "channels"), (lambda b: b.drop(n, 1), "channels"), (lambda b: b.run(big, 2 * NF), "n_frames"),
           (lambda b: b.run(da, 0), "n_frames")]
    for call, word in bad:
        with pytest.raises(dspfx.DspfxError) as e:
            call(bank)
        assert e.value.status == -1 and word in str(e.value) and "blends" in str(e.value), str(e.value)
    for call in (lambda: ref.assign([0, G], 0), lambda: ref.assign([0, 1], n - 1), lambda: ref.set_mix(0.1, n - 1, 2), lambda: ref.set_send(1.0, 0, n + 1),
                 lambda: ref.drop(n, 1), lambda: ref.run(a, b=side, bus=bus), lambda: ref.run(np.zeros((2 * NF, n), F))):
        assert call() is False
    with pytest.raises(dspfx.DspfxError):
        bank.kinds(1, n)
    assert same_tables(before, tables(bank)) and same_tables(before, tables(ref))
    assert np.array_equal(bits(run(dspfx, torch, bank, a, bus=bus)), bits(want)), "a following run: the unchanged settings"
    E.same_bits_or_nan(want, ref.run(a, bus=bus), None, "the restatement")
    bank.close()
    plain.close()


def test_stores_between_submitted_runs(dspfx, torch_cuda):
    """nothing waits between the calls; everything is read at the end.  set_mix(None) over Add, drop keeps the bus, a send removed"""
    torch = torch_cuda
    n, tile, G = 256, 64, 2
    bank, ref = dspfx.ChannelBlends(n, buses=G, tile_channels=tile, max_frames=NF), R.ChannelBlends(n, buses=G)
    a, bus = noise(n, NF, 85), noise(G, NF, 86)
    da = device(dspfx, torch, a, tile)
    dbus = torch.from_numpy(bus.reshape(-1).copy()).cuda()
    dys = [torch.full((NF * n,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(6)]
    torch.cuda.synchronize()
    wants = []

    def both(call):
        for b in (bank, ref):
            assert call(b) is not False

    def submit(i):
        bank.run(da, NF, bus=dbus, out=dys[i])
        wants.append(ref.run(a, bus=bus))

    both(lambda b: b.assign((np.arange(n) % G).astype(np.uint32)))
    both(lambda b: b.set_add(0, 128))
    submit(0)
    both(lambda b: b.set_mix(None, 64, 128))                     # 64 .. 127 over Add: 0.5; 128 .. 191 new: 0.5
    both(lambda b: b.set_send(0.25, 96, 64))
    submit(1)
    both(lambda b: b.set_mix(np.linspace(-1, 2, 32).astype(F), 100))
    both(lambda b: b.set_mix(None, 96, 16))                      # a Mix node keeps its ratio
    submit(2)
    both(lambda b: b.drop(96, 8))
    both(lambda b: b.set_send(None, 104, 8))
    submit(3)
    both(lambda b: b.set_add(96, 4))                             # after the drop: no send, the bus it had
    both(lambda b: b.assign(NO_BUS, 97))
    submit(4)
    both(lambda b: b.drop())
    assert (bank.kinds() == dspfx.BLENDS_NONE).all(), "the host tables already show the drop"
    submit(5)
    torch.cuda.synchronize()
    for i, want in enumerate(wants):
        E.same_bits_or_nan(host(dspfx, dys[i], NF, n, tile), want, None, f"run {i}")
    assert np.array_equal(bits(host(dspfx, dys[5], NF, n, tile)), bits(a))
    assert same_tables(tables(bank), tables(ref))
    assert bank.bus_of()[96] == 0 and bank.bus_of()[97] == NO_BUS
    bank.close()


def test_a_thread_storing_whole_range_settings_while_blocks_are_submitted(dspfx, torch_cuda):
    """every block equals the all-old or the all-new expectation -- a store is whole"""
    torch = torch_cuda
    n, tile, runs = 256, 64, 60
    a, b = noise(n, NF, 87), noise(n, NF, 88)
    wants = [bits(engine(dspfx, torch, "mix", r, a, b)) for r in (0.25, 0.75)]
    bank = dspfx.ChannelBlends(n, tile_channels=tile, max_frames=NF)
    bank.set_mix(0.25)
    da, db = device(dspfx, torch, a, tile), device(dspfx, torch, b, tile)
    dys = [torch.full((NF * n,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(runs)]
    torch.cuda.synchronize()
    done, errors, made = threading.Event(), [], [0]

    def storer():
        try:
            while not done.is_set() or made[0] < 20:
                bank.set_mix(np.full(n, (0.75, 0.25)[made[0] % 2], F))
                made[0] += 1
        except Exception as e:                                   # noqa: BLE001
            errors.append(e)

    t = threading.Thread(target=storer)
    t.start()
    for i in range(runs):
        bank.run(da, NF, b=db, out=dys[i])
    done.set()
    t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for i in range(runs):
        got = bits(host(dspfx, dys[i], NF, n, tile))
        assert any(np.array_equal(got, w) for w in wants), f"run {i} is neither all old nor all new"
    bank.close()


# ---- 7. edge values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["add", "mix"])
def test_edge_values(dspfx, torch_cuda, kind):
    """a, b, the ratio, the level and the control block drawn from edge_values' set -- NaN with payloads, infinities, signed zeros,
    subnormals, the largest finite value -- each channel its own ratio and level"""
    torch = torch_cuda
    vals = []
    for v, _ in E.edge_classes(1.0).values():
        for x in v:
            vals.extend(x if isinstance(x, tuple) else (x,))
    vals = np.asarray(vals, F)
    rng = np.random.default_rng(7)
    n, nf = 256, NF
    draw = lambda *shape: vals[rng.integers(0, len(vals), shape)]      # noqa: E731
    a, b, ctl = draw(nf, n), draw(nf, n), draw(nf, n)
    bank, ref = dspfx.ChannelBlends(n, tile_channels=64, max_frames=NF), R.ChannelBlends(n)
    ratios, levels = draw(n), draw(n // 2)
    for x in (bank, ref):
        assert (x.set_add() if kind == "add" else x.set_mix(ratios)) is not False
        assert x.set_send(levels, n // 2) is not False
    assert same_tables(tables(bank), tables(ref)), "values are taken as given"
    E.same_bits_or_nan(run(dspfx, torch, bank, a, b=b), ref.run(a, b=b), None, f"{kind} block")
    E.same_bits_or_nan(run(dspfx, torch, bank, a), ref.run(a), None, f"{kind} unconnected")
    if kind == "mix":
        E.same_bits_or_nan(run(dspfx, torch, bank, a, b=b, ratio=ctl), ref.run(a, b=b, ratio=ctl), None, "mix with the control block")
    bank.close()


# ---- 8. full size ----------------------------------------------------------------------------------------------------------
def test_full_size(dspfx, torch_cuda):
    """2^20 channels x 128 frames, tiled 256; two alternating buffers, device events, median of 20 after 5 warm-ups.
    Asserted: a Mix-everywhere bank in block mode takes at most twice Engine([Mix(0.3)], link_flags=0) with side on the same buffers,
    timed here (twice is the margin every bank here gets over its engine), and equals it bit for bit; the same bank in bus mode with
    4096 contiguous rooms of 256 fits the 2.667 ms a 128-frame block lasts at 48 kHz and takes at most that same doubled engine time.
    Printed, not asserted: bus mode with fully shuffled ids, a half-present bank, a run with the ratio control block; milliseconds,
    the fraction of 8 TB/s on each run's own bytes (three block-units in block mode, two in bus mode, four with the control
    block), a flat copy of the same bytes."""
    torch = torch_cuda
    n, nf, tile, G = 1 << 20, 128, 256, 4096
    gen = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.rand(nf * n, dtype=torch.float32, device="cuda", generator=gen) - 0.5 for _ in range(2)]
    ss = [torch.rand(nf * n, dtype=torch.float32, device="cuda", generator=gen) - 0.5 for _ in range(2)]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    bus = torch.rand(nf * G, dtype=torch.float32, device="cuda", generator=gen) - 0.5
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

    assert dspfx.blends_plan(n) == 13 * n
    bank = dspfx.ChannelBlends(n, tile_channels=tile, max_frames=nf, group_size=256)
    assert bank.buses == G
    bank.set_mix(0.3)
    t_block = timed(lambda i: bank.run(xs[i % 2], nf, b=ss[i % 2], out=ys[i % 2]))
    torch.cuda.synchronize()
    mine = ys[1].clone()
    eng = dspfx.Engine(n, nf, link_flags=0, tile_channels=tile)
    eng.set_chain([dspfx.Mix(0.3)])
    t_eng = timed(lambda i: eng.process(xs[i % 2], out=ys[i % 2], side=ss[i % 2], n_frames=nf))
    torch.cuda.synchronize()
    equal = torch.equal(mine.view(torch.int32), ys[1].view(torch.int32))
    eng.close()
    t_bus = timed(lambda i: bank.run(xs[i % 2], nf, bus=bus, out=ys[i % 2]))
    t_ctl = timed(lambda i: bank.run(xs[i % 2], nf, b=ss[i % 2], ratio=ss[(i + 1) % 2], out=ys[i % 2]))
    bank.assign(np.random.default_rng(3).permutation(n).astype(np.uint32) % G)
    t_shuffled = timed(lambda i: bank.run(xs[i % 2], nf, bus=bus, out=ys[i % 2]))
    bank.drop()
    bank.set_mix(0.3, 0, n // 2)                                # the second half of the channels carries no node
    t_half = timed(lambda i: bank.run(xs[i % 2], nf, b=ss[i % 2], out=ys[i % 2]))
    bank.close()
    t_copy = timed(lambda i: ys[i % 2].copy_(xs[i % 2]))
    frac = lambda t, units: units * unit / t / 1e9 / 8.0      # noqa: E731
    print(f"full size blends, one box, one run, a block-unit is {unit / 2**20:.0f} MiB: Mix everywhere, block mode {t_block:.4f} ms "
          f"({frac(t_block, 3):.3f} of 8 TB/s on three units; Engine([Mix]) with side {t_eng:.4f} ms, bank x {t_block / t_eng:.3f}), "
          f"bus mode, 4096 contiguous rooms of 256 {t_bus:.4f} ms ({frac(t_bus, 2):.3f} on two units), bus mode, shuffled ids {t_shuffled:.4f} ms "
          f"({frac(t_shuffled, 2):.3f}), the first half of the channels present, block mode {t_half:.4f} ms ({frac(t_half, 2.5):.3f} on two and a half units), "
          f"block mode with the ratio control block {t_ctl:.4f} ms ({frac(t_ctl, 4):.3f} on four units), flat copy of one unit {t_copy:.4f} ms "
          f"({frac(t_copy, 2):.3f} on two units)")
    assert equal, "the bank's bits are the engine's"
    assert t_block <= 2 * t_eng, (t_block, t_eng)
    assert t_bus * 1e-3 <= 128 / 48000, t_bus
    assert t_bus <= 2 * t_eng, (t_bus, t_eng)
