"""The channel-filter bank on the GPU (dspfx_filters_*, through the Python class): per-channel LowPass, HighPass and Envelope in
1 .. 4 slots.  A channel's output and state are compared bit for bit with Engine([its present nodes in slot order], link_flags=0)
-- one engine run per distinct chain, made once per module and shared -- and, through filters_ref (one oracle chain per channel),
with the oracle at the bars tests/test_gpu_parity.py holds the engine to: 1 ulp where a one-pole is in the chain (test_one_pole's),
0 for Envelope alone (test_envelope_follower's).  The engines run blocks of 128 frames; the banks run the same frames cut into
37 + 128 + 91, since the recurrences carry no block structure.  Out-of-place outputs start as NaN everywhere, so every sample is
shown to be written."""
import ctypes as C
import threading

import numpy as np
import pytest

import edge_values as E
import filters_ref as R
import oracle as O
from chains import ulp_diff

pytestmark = pytest.mark.gpu

NF = 128
F = np.float32
SHAPES = [(64, 0), (256, 64), (70, 0), (1, 0)]                   # vector lanes; tiled; scalar accesses and a ragged last workgroup; one channel
THREE = [(64, 0), (256, 64), (70, 0)]
TWO = [(256, 64), (70, 0)]
FRAMES = [1, 37, 128]
EDGES = FRAMES + [4, 8, 9]                                       # the frame loop's boundaries with 4 or 8 rows a chunk: one chunk, two, chunks and a row
CUTS = (37, 128, 91)
NX = 256                                                         # the channels of the shared input and of the engines that give the expectations
RATIOS = (0.0, 0.5, 0.93, 1.0)                                                   # test_one_pole's
ENVELOPES = ((0.0, 0.0), (0.0, 64.0), (5.0, 0.0), (48.0, 1000.0), (0.5, 0.25))   # test_envelope_follower's
# a slot: ("lp", ratio) | ("hp", ratio) | ("env", attack, release) | None; a channel's setting: a tuple of `stages` slots
UNIFORM = [("lp", r) for r in RATIOS] + [("hp", r) for r in RATIOS] + [("env",) + e for e in ENVELOPES]
MIX = {"lp": (("lp", 0.93), ("lp", 0.5)), "hp": (("hp", 0.05), ("hp", 0.5)), "env": (("env", 5.0, 64.0), ("env", 48.0, 1000.0))}
CODE = {"lp": R.LOW_PASS, "hp": R.HIGH_PASS, "env": R.ENVELOPE}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_X = {}


def noise_x(nf=2 * NF):
    """noise * 2.5 with the fixed first values of test_distort_arithmetic_modes: [2 * 128][NX], left unchanged"""
    if "x" not in _X:
        x = O.noise(0x5EED0001, np.arange(NX), np.arange(2 * NF)) * F(2.5)
        x[0, :10] = [0, -0.0, 0.25, -0.25, 0.5, -0.5, 1, -1, 2, -2]
        x.setflags(write=False)
        _X["x"] = x
    return _X["x"][:nf]


def node_of(dspfx, s):
    return dspfx.LowPass(s[1]) if s[0] == "lp" else dspfx.HighPass(s[1]) if s[0] == "hp" else dspfx.Envelope(s[1], s[2])


def engine_run(dspfx, torch, chain, x, blocks=None):
    """Engine([the nodes of `chain`], link_flags=0) over x, 128 frames at a time (`blocks`: x again and again, that many times)
    -> (the output, the exported state of every node after the last block)"""
    eng = dspfx.Engine(x.shape[1], NF, link_flags=0)
    eng.set_chain([node_of(dspfx, s) for s in chain])
    spans = [(f0, min(f0 + NF, len(x))) for f0 in range(0, len(x), NF)] if blocks is None else [(0, len(x))] * blocks
    y = np.empty((sum(b - a for a, b in spans), x.shape[1]), F)
    at = 0
    for a, b in spans:
        dx = torch.from_numpy(x[a:b].copy()).cuda()
        dy = torch.full_like(dx, float("nan"))
        eng.process(dx, out=dy, n_frames=b - a)
        torch.cuda.synchronize()
        y[at:at + b - a] = dy.cpu().numpy()
        at += b - a
    states = [eng.state_export(i).view(np.float32).copy() for i in range(len(chain))]
    eng.close()
    return y, states


_ENGINE = {}


def engine_ref(dspfx, torch, chain):
    """the engine's output and final states for `chain` (the present slots, in order) on noise_x(), [256][NX] and [NX] per node:
    computed once, shared, left unchanged.  Row f is what any cut of the frames gives"""
    if chain not in _ENGINE:
        y, states = engine_run(dspfx, torch, chain, noise_x())
        y.setflags(write=False)
        _ENGINE[chain] = (y, states)
    return _ENGINE[chain]


def present(setting):
    return tuple(s for s in setting if s is not None)


def expected(dspfx, torch, settings, nf, cols=None):
    """([nf][n] outputs, [stages][n] states after 256 frames): channel c as the engine of its own chain gives column cols[c] of
    noise_x (default: c); no node: a copy, state +0.0"""
    n, stages = len(settings), len(settings[0])
    cols = np.arange(n) % NX if cols is None else cols
    want, state = np.empty((nf, n), F), np.zeros((stages, n), F)
    where = {}
    for c, s in enumerate(settings):
        where.setdefault(s, []).append(c)
    for s, cs in where.items():
        chain = present(s)
        if not chain:
            want.view(np.uint32)[:, cs] = noise_x(nf).view(np.uint32)[:, cols[cs]]
            continue
        y, st = engine_ref(dspfx, torch, chain)
        want.view(np.uint32)[:, cs] = y[:nf].view(np.uint32)[:, cols[cs]]
        k = 0
        for t, slot in enumerate(s):
            if slot is not None:
                state[t, cs] = st[k][cols[cs]]
                k += 1
    return want, state


def store(b, settings, first=0):
    """the settings onto a bank or its restatement: per stage, consecutive channels of one kind in one store"""
    n = len(settings)
    for t in range(len(settings[0])):
        c = 0
        while c < n:
            fam = None if settings[c][t] is None else settings[c][t][0]
            e = c
            while e < n and (None if settings[e][t] is None else settings[e][t][0]) == fam:
                e += 1
            col = lambda k: np.asarray([s[t][k] for s in settings[c:e]], F)       # noqa: E731
            if fam is None:
                ok = b.drop(t, first + c, e - c)
            elif fam == "env":
                ok = b.set_envelope(t, col(1), col(2), first_channel=first + c)
            else:
                ok = getattr(b, "set_low_pass" if fam == "lp" else "set_high_pass")(t, col(1), first_channel=first + c)
            assert ok is not False
            c = e


def mixed(n, stages, shift=0):
    """slot kinds (c + stage + shift) % 4 over none / LowPass / HighPass / Envelope: a lane's four channels differ in every stage
    and every wave holds every kind; the sliders alternate between two sets from one group of four channels to the next"""
    order = (None, "lp", "hp", "env")
    return [tuple(None if order[(c + t + shift) % 4] is None else MIX[order[(c + t + shift) % 4]][(c // 4) % 2] for t in range(stages)) for c in range(n)]


def tables(settings):
    return np.asarray([[R.NONE if s[t] is None else CODE[s[t][0]] for s in settings] for t in range(len(settings[0]))], np.uint32)


def bars(settings):
    """per channel, against the oracle: 1 ulp where a one-pole is in the chain, 0 for Envelope alone and for a copy"""
    return np.asarray([int(any(slot is not None and slot[0] != "env" for slot in s)) for s in settings])


def near_oracle(got, want, settings, what):
    bar = bars(settings)
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(got)), what
    with np.errstate(invalid="ignore"):
        d = np.where(nan, 0, ulp_diff(got, want)).max(axis=0)
    print(f"{what}: worst {int(d.max())} ulp against the oracle (bars 1 with a one-pole, 0 without)")
    assert (d <= bar).all(), (what, np.flatnonzero(d > bar)[:8], d[d > bar][:8])


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


def run_cuts(dspfx, torch, bank, x, n, tile, cuts=CUTS, inplace=False):
    out, f0 = [], 0
    for k in cuts:
        out.append(run(dspfx, torch, bank, x[f0:f0 + k], n, tile, inplace=inplace))
        f0 += k
    return np.concatenate(out)


def states(torch, bank):
    torch.cuda.synchronize()
    return np.stack([bank.state(t).cpu().numpy() for t in range(bank.stages)])


# ---- 1. a fresh bank -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", EDGES)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_a_fresh_bank_copies(dspfx, torch_cuda, n, tile, nf):
    stages = 1 + (n + nf) % 4
    bank = dspfx.ChannelFilters(n, stages=stages, tile_channels=tile, max_frames=NF)
    x = noise_x(nf)[:, :n]
    assert np.array_equal(bits(run(dspfx, torch_cuda, bank, x, n, tile)), bits(x))
    assert not bank.present().any() and not bits(states(torch_cuda, bank)).any(), "every table at rest"
    for t in range(stages):
        assert (bank.kinds(t) == dspfx.FILTERS_NONE).all() and not bank.sliders(t).any() and bank.sliders(t).shape == (n, 2)
    bank.close()


# ---- 2. one setting everywhere equals that engine ------------------------------------------------------------------------
@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_one_setting_everywhere_equals_that_engine(dspfx, torch_cuda, n, tile, nf):
    """LowPass and HighPass at test_one_pole's ratios, Envelope at test_envelope_follower's pairs; the stores follow each other on
    one bank with a reset between the ratios of one kind (a store of the same kind keeps the state)"""
    torch = torch_cuda
    bank = dspfx.ChannelFilters(n, stages=1, tile_channels=tile, max_frames=NF)
    x = noise_x(nf)[:, :n]
    for s in UNIFORM:
        store(bank, [(s,)] * n)
        bank.reset()
        got = run(dspfx, torch, bank, x, n, tile)
        want, _ = engine_ref(dspfx, torch, (s,))
        assert np.array_equal(bits(got), bits(want[:nf, :n])), f"N={n} tile={tile} nf={nf} {s}"
        ref = R.ChannelFilters(n)
        store(ref, [(s,)] * n)
        near_oracle(got, ref.run(x), [(s,)] * n, f"N={n} tile={tile} nf={nf} {s}")
        assert (bank.kinds(0) == CODE[s[0]]).all() and bank.present().all()
        assert np.array_equal(bank.sliders(0), np.tile(np.asarray((s[1:] + (0.0,))[:2], F), (n, 1)))
    bank.close()


# ---- 3. a mixed bank -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages", [1, 2, 4])
@pytest.mark.parametrize("n,tile", SHAPES)
def test_mixed_bank_every_channel_equals_the_engine_of_its_own_chain(dspfx, torch_cuda, n, tile, stages):
    """slot kinds (c + stage) % 4 over 37 + 128 + 91 frames: outputs and states"""
    torch = torch_cuda
    settings = mixed(n, stages)
    x = noise_x()[:, :n]
    want, want_state = expected(dspfx, torch, settings, 2 * NF)
    bank = dspfx.ChannelFilters(n, stages=stages, tile_channels=tile, max_frames=NF)
    store(bank, settings)
    k = tables(settings)
    for t in range(stages):
        assert np.array_equal(bank.kinds(t), k[t])
    assert np.array_equal(bank.present(), (k != R.NONE).any(axis=0).astype(np.uint32))
    got = run_cuts(dspfx, torch, bank, x, n, tile)
    assert np.array_equal(bits(got), bits(want)), f"N={n} tile={tile} stages={stages}"
    assert np.array_equal(bits(states(torch, bank)), bits(want_state)), "the state tables are the engine's exported node states"
    bank.close()


def test_a_run_of_256_frames_on_a_bank_that_allows_them(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile = 256, 64
    settings = mixed(n, 2)
    want, want_state = expected(dspfx, torch, settings, 2 * NF)
    bank = dspfx.ChannelFilters(n, stages=2, tile_channels=tile, max_frames=256)
    store(bank, settings)
    assert np.array_equal(bits(run(dspfx, torch, bank, noise_x()[:, :n], n, tile)), bits(want))
    assert np.array_equal(bits(states(torch, bank)), bits(want_state))
    bank.close()


def test_against_the_oracle_through_the_restatement(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile, stages = 70, 0, 4
    settings = mixed(n, stages)
    bank, ref = dspfx.ChannelFilters(n, stages=stages, tile_channels=tile, max_frames=NF), R.ChannelFilters(n, stages)
    store(bank, settings)
    store(ref, settings)
    for t in range(stages):
        assert np.array_equal(bank.kinds(t), ref.kind[t]) and np.array_equal(bits(bank.sliders(t)), bits(ref.p[t]))
    x = noise_x()[:, :n]
    got = run_cuts(dspfx, torch, bank, x, n, tile)
    near_oracle(got, np.concatenate([ref.run(x[:37]), ref.run(x[37:165]), ref.run(x[165:])]), settings, "mixed, four stages")
    bank.close()


# ---- 4. neighbours ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", THREE)
def test_a_channels_bits_do_not_depend_on_its_neighbours(dspfx, torch_cuda, n, tile):
    """the kept channels (one of each lane's four, and the last) get the same chains and samples in three banks; every other
    channel is empty in the second and carries other kinds, other sliders or NaN samples in the third"""
    torch = torch_cuda
    keep = np.zeros(n, bool)
    keep[(np.arange(n) % 4) == (np.arange(n) // 4) % 4] = True
    keep[n - 1] = True
    sa = mixed(n, 2)
    other = mixed(n, 2, shift=1)
    empty = (None, None)
    sb = [sa[c] if keep[c] else empty for c in range(n)]
    sc = [sa[c] if keep[c] else other[c] for c in range(n)]
    x = noise_x(NF)[:, :n]
    x3 = np.where(keep, x, noise_x(2 * NF)[NF:, :n] * F(5))
    x3[:, np.flatnonzero(~keep)[::3]] = np.nan
    outs = []
    for s, xx in ((sa, x), (sb, x), (sc, x3)):
        bank = dspfx.ChannelFilters(n, stages=2, tile_channels=tile, max_frames=NF)
        store(bank, s)
        outs.append((run(dspfx, torch, bank, xx, n, tile), states(torch, bank)))
        bank.close()
    assert np.array_equal(bits(outs[0][0]), bits(expected(dspfx, torch, sa, NF)[0])), "bank a"
    for y, st in outs[1:]:
        assert np.array_equal(bits(y[:, keep]), bits(outs[0][0][:, keep])) and np.array_equal(bits(st[:, keep]), bits(outs[0][1][:, keep]))
    assert not np.array_equal(bits(outs[0][0][:, ~keep]), bits(outs[2][0][:, ~keep]))


# ---- 5. in place, layouts, pointers, streams -----------------------------------------------------------------------------
@pytest.mark.parametrize("nf", EDGES)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_in_place_equals_out_of_place(dspfx, torch_cuda, n, tile, nf):
    torch = torch_cuda
    bank = dspfx.ChannelFilters(n, stages=2, tile_channels=tile, max_frames=NF)
    settings = mixed(n, 2)
    store(bank, settings)
    x = noise_x(nf)[:, :n]
    out = run(dspfx, torch, bank, x, n, tile)
    bank.reset()
    assert np.array_equal(bits(run(dspfx, torch, bank, x, n, tile, inplace=True)), bits(out))
    assert np.array_equal(bits(out), bits(expected(dspfx, torch, settings, nf)[0])) and not np.isnan(out).any()
    bank.close()


def test_both_layouts_give_the_same_bits(dspfx, torch_cuda):
    torch = torch_cuda
    n = 256
    settings = mixed(n, 4)
    outs = []
    for tile in (0, 64, 256):
        bank = dspfx.ChannelFilters(n, stages=4, tile_channels=tile, max_frames=NF)
        store(bank, settings)
        outs.append((run_cuts(dspfx, torch, bank, noise_x()[:, :n], n, tile), states(torch, bank)))
        bank.close()
    for y, st in outs[1:]:
        assert np.array_equal(bits(y), bits(outs[0][0])) and np.array_equal(bits(st), bits(outs[0][1]))


def test_out_of_place_from_an_unaligned_pointer_takes_the_scalar_path(dspfx, torch_cuda):
    """N = 64 would take four channels per lane; the blocks start 4 bytes past a 16-byte boundary, so a lane takes one"""
    torch = torch_cuda
    n, tile, nf = 64, 0, 37
    settings = mixed(n, 2)
    bank = dspfx.ChannelFilters(n, stages=2, tile_channels=tile, max_frames=NF)
    store(bank, settings)
    x = noise_x(nf)[:, :n]
    big = torch.zeros(nf * n + 8, dtype=torch.float32, device="cuda")
    out = torch.full((nf * n + 8,), float("nan"), dtype=torch.float32, device="cuda")
    big[1:1 + nf * n] = device(dspfx, torch, x, tile)
    dx, dy = big[1:1 + nf * n], out[3:3 + nf * n]
    assert dx.data_ptr() % 16 == 4 and dy.data_ptr() % 16 == 12
    bank.run(dx, nf, out=dy)
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(dspfx, dy, nf, n, tile)), bits(expected(dspfx, torch, settings, nf)[0]))
    assert np.isnan(out[:3].cpu().numpy()).all() and np.isnan(out[3 + nf * n:].cpu().numpy()).all(), "nothing outside the block is written"
    bank.close()


def test_a_null_pointer_or_no_frames_is_refused(dspfx, torch_cuda):
    torch = torch_cuda
    n = 64
    bank = dspfx.ChannelFilters(n, stages=1, max_frames=NF)
    dx = device(dspfx, torch, noise_x(NF)[:, :n], 0)
    L, p = bank.L, C.c_void_p(dx.data_ptr())
    assert L.dspfx_filters_run(bank.h, None, p, NF, None) == -1 and b"filters run" in L.dspfx_filters_last_error(bank.h)
    assert L.dspfx_filters_run(bank.h, p, None, NF, None) == -1
    for nf in (0, NF + 1):
        with pytest.raises(dspfx.DspfxError) as e:
            bank.run(dx, nf, out=dx)
        assert e.value.status == -1 and "n_frames" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert np.array_equal(bits(dx.cpu().numpy().reshape(NF, n)), bits(noise_x(NF)[:, :n])), "a refused run writes nothing"
    bank.close()


def test_two_streams(dspfx, torch_cuda):
    """the cuts alternate between two streams and nothing waits in between: the state is the bank's, so a run on another stream
    waits on the device for the one before"""
    torch = torch_cuda
    n, tile = 256, 64
    settings = mixed(n, 2)
    x = noise_x()[:, :n]
    bank = dspfx.ChannelFilters(n, stages=2, tile_channels=tile, max_frames=NF)
    store(bank, settings)
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
    want, want_state = expected(dspfx, torch, settings, 2 * NF)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(states(torch, bank)), bits(want_state))
    bank.close()


# ---- 6. store rules --------------------------------------------------------------------------------------------------------
def test_store_rules_on_the_device_follow_the_restatement(dspfx, torch_cuda):
    """between two runs: a store of the same kind keeps the state (and the slider left out), a kind change zeroes it, drop, reset
    of a sub-range and of one stage; nothing waits between the calls of a round.  The bank and filters_ref get the same calls"""
    torch = torch_cuda
    n, tile = 70, 0
    x = noise_x()[:, :n]
    a, b = x[:37], x[37:165]
    bank, ref = dspfx.ChannelFilters(n, stages=2, tile_channels=tile, max_frames=NF), R.ChannelFilters(n, 2)
    both = (bank, ref)
    base = [(("hp", 0.05), ("lp", 0.93))] * n
    for k in both:
        store(k, base)
    got_a = run(dspfx, torch, bank, a, n, tile)
    near_oracle(got_a, ref.run(a), base, "before the stores")
    z_before = states(torch, bank)
    for k in both:
        assert k.set_low_pass(1, first_channel=0, count=10) is not False                # the same kind, nothing given: all is kept
        assert k.set_low_pass(1, 0.5, first_channel=10, count=10) is not False           # the same kind, a new ratio: the state is kept
        assert k.set_high_pass(1, first_channel=20, count=10) is not False               # another kind: ratio 0.5, state +0.0
        assert k.set_envelope(0, release=64.0, first_channel=20, count=10) is not False  # another kind: attack 0, state +0.0
        assert k.drop(0, 30, 10) is not False                                            # stage 0 copies again
        assert k.reset(first_channel=40, count=10) is not False                          # every stage of a sub-range
        assert k.reset(first_channel=50, count=10, stage=1) is not False                 # one stage
        assert k.drop(1, 60, 5) is not False and k.set_low_pass(1, first_channel=60, count=5) is not False       # dropped, set again: new
    after = ([base[0]] * 10 + [(("hp", 0.05), ("lp", 0.5))] * 10 + [(("env", 0.0, 64.0), ("hp", 0.5))] * 10 + [(None, ("lp", 0.93))] * 10
             + [base[0]] * 20 + [(("hp", 0.05), ("lp", 0.5))] * 5 + [base[0]] * 5)
    for t in range(2):
        assert np.array_equal(bank.kinds(t), ref.kind[t]) and np.array_equal(bank.kinds(t), tables(after)[t])
        assert np.array_equal(bits(bank.sliders(t)), bits(ref.p[t]))
    got_b = run(dspfx, torch, bank, b, n, tile)
    near_oracle(got_b, ref.run(b), after, "after the stores")
    z = states(torch, bank)
    # what the rules mean for the bits, beside the restatement: kept state continues, a zeroed one starts as a fresh bank does
    fresh = dspfx.ChannelFilters(n, stages=2, tile_channels=tile, max_frames=NF)
    store(fresh, after)
    got_fresh = run(dspfx, torch, fresh, b, n, tile)
    fresh.close()
    cont = expected(dspfx, torch, base, 165)[0][37:]
    assert np.array_equal(bits(got_b[:, :10]), bits(cont[:, :10])) and np.array_equal(bits(got_b[:, 65:]), bits(cont[:, 65:])), "kept: as if nothing was stored"
    assert not np.array_equal(bits(got_b[:, 10:20]), bits(got_fresh[:, 10:20])), "a new ratio on the old state"
    assert np.array_equal(bits(got_b[:, 20:30]), bits(got_fresh[:, 20:30])), "a kind change starts from +0.0"
    assert np.array_equal(bits(got_b[:, 40:50]), bits(got_fresh[:, 40:50])), "reset of every stage"
    assert not np.array_equal(bits(got_b[:, 30:40]), bits(got_fresh[:, 30:40])), "a drop of stage 0 leaves stage 1's state"
    assert not np.array_equal(bits(got_b[:, 50:60]), bits(got_fresh[:, 50:60])), "reset of stage 1 leaves stage 0's state"
    assert np.array_equal(bits(got_b[:, 50:60]), bits(run_stage1_new(dspfx, torch, base, a, b, n, tile)[:, 50:60])), "... and zeroes stage 1's"
    assert np.array_equal(bits(got_b[:, 60:65]), bits(run_stage1_new(dspfx, torch, after, a, b, n, tile)[:, 60:65])), "dropped and set again: a new node"
    assert not bits(z[0, 30:40]).any() and bits(z_before[0, 30:40]).any(), "a dropped slot's state is +0.0"
    bank.close()


def run_stage1_new(dspfx, torch, base, a, b, n, tile):
    """stage 0 carried over a and b, stage 1 new before b"""
    bank = dspfx.ChannelFilters(n, stages=2, tile_channels=tile, max_frames=NF)
    store(bank, base)
    run(dspfx, torch, bank, a, n, tile)
    bank.reset(stage=1)
    out = run(dspfx, torch, bank, b, n, tile)
    bank.close()
    return out


def test_a_refused_store_changes_nothing(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile = 70, 0
    settings = mixed(n, 2)
    bank, ref = dspfx.ChannelFilters(n, stages=2, tile_channels=tile, max_frames=NF), R.ChannelFilters(n, 2)
    store(bank, settings)
    store(ref, settings)
    x = noise_x()[:, :n]
    first = run(dspfx, torch, bank, x[:NF], n, tile)
    bad = [(lambda k: k.set_low_pass(2, 0.5), "stage"), (lambda k: k.set_high_pass(4, 0.5, first_channel=0, count=1), "stage"),
           (lambda k: k.set_envelope(0, 1.0, 2.0, first_channel=n - 1, count=2), "channels"), (lambda k: k.set_low_pass(0, 0.5, first_channel=n + 1, count=0), "channels"),
           (lambda k: k.set_envelope(1, np.ones(3, F), np.ones(4, F)), "different numbers"), (lambda k: k.drop(2, 0, 1), "stage"),
           (lambda k: k.drop(0, n, 1), "channels"), (lambda k: k.reset(stage=2), "stage"), (lambda k: k.reset(first_channel=0, count=n + 1), "channels")]
    for call, word in bad:
        with pytest.raises(dspfx.DspfxError) as e:
            call(bank)
        assert e.value.status == -1 and word in str(e.value) and "filters" in str(e.value), str(e.value)
        assert call(ref) is False
    for call in (lambda: bank.kinds(2), lambda: bank.sliders(2), lambda: bank.state(2), lambda: bank.present(1, n)):
        with pytest.raises(dspfx.DspfxError):
            call()
    for t in range(2):
        assert np.array_equal(bank.kinds(t), ref.kind[t]) and np.array_equal(bits(bank.sliders(t)), bits(ref.p[t]))
    got = np.concatenate([first, run(dspfx, torch, bank, x[NF:], n, tile)])
    assert np.array_equal(bits(got), bits(expected(dspfx, torch, settings, 2 * NF)[0])), "after the refused stores: the state and the nodes as they were"
    bank.set_low_pass(0, [float("nan"), float("inf"), -3.0, 7.5], first_channel=0)                  # taken as given
    bank.set_envelope(1, float("nan"), -1.0, first_channel=0, count=1)
    assert np.isnan(bank.sliders(0)[0, 0]) and list(bank.sliders(0)[1:4, 0]) == [np.inf, -3.0, 7.5] and bank.sliders(1)[0, 1] == -1.0
    assert np.isnan(run(dspfx, torch, bank, x[:NF], n, tile)[:, 0]).all()
    bank.close()


def test_a_thread_storing_kind_changes_while_blocks_are_submitted(dspfx, torch_cuda):
    """a second thread stores HighPass / Envelope over the whole range, alternating, while the first submits runs of one block, and
    nothing waits.  Every store changes the kind, so it makes new nodes: a run equals block j of the engine of one kind, where j
    counts the runs since the last store it saw -- and then the run before it was block j - 1 of the same kind.  A store is whole"""
    torch = torch_cuda
    n, tile, runs = 256, 64, 40
    kinds = (("hp", 0.05), ("env", 5.0, 64.0))
    x = noise_x(NF)[:, :n]
    blocks = [bits(engine_run(dspfx, torch, (s,), np.ascontiguousarray(x), blocks=runs)[0]).reshape(runs, NF, n) for s in kinds]
    bank = dspfx.ChannelFilters(n, stages=1, tile_channels=tile, max_frames=NF)
    store(bank, [(kinds[0],)] * n)
    dx = device(dspfx, torch, x, tile)
    dys = [torch.full_like(dx, float("nan")) for _ in range(runs)]
    torch.cuda.synchronize()
    done, errors, made = threading.Event(), [], [0]

    def storer():
        try:
            while not done.is_set() or made[0] < 20:
                store(bank, [(kinds[(made[0] + 1) % 2],)] * n)
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
    before = set()                                              # (a one-pole forgets: later blocks of one kind may be the same bits)
    for i in range(runs):
        got = bits(host(dspfx, dys[i], NF, n, tile))
        match = {(k, j) for k in range(2) for j in range(i + 1) if np.array_equal(got, blocks[k][j])}
        assert match, f"run {i} is no block of either kind"
        assert any(j == 0 or (k, j - 1) in before for k, j in match), f"run {i} is block {sorted(match)}, the run before was {sorted(before)}"
        before = match
    bank.close()


# ---- 7. edge values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", TWO)
def test_edge_values_through_every_kind(dspfx, torch_cuda, n, tile):
    """NaN, both infinities, signed zeros, subnormals, each class in a channel of its own, through a bank of each kind against the
    engine of that kind on the same block; then through empty slots: every edge value's very bits"""
    torch = torch_cuda
    x, tab = E.edge_block(n, 2 * NF)
    bank = dspfx.ChannelFilters(n, stages=1, tile_channels=tile, max_frames=2 * NF)
    for s in (("lp", 0.93), ("lp", 1.0), ("hp", 0.05), ("hp", 0.0), ("env", 5.0, 64.0), ("env", 0.0, 0.0)):
        store(bank, [(s,)] * n)
        bank.reset()
        got = run(dspfx, torch, bank, x, n, tile)
        E.same_bits_or_nan(got, engine_run(dspfx, torch, (s,), x)[0], tab, f"N={n} {s}")
    bank.drop(0)
    assert np.array_equal(bits(run(dspfx, torch, bank, x, n, tile)), bits(x)), "no node: every edge value's very bits"
    bank.close()


# ---- 8. full size ----------------------------------------------------------------------------------------------------------
def test_full_size(dspfx, torch_cuda):
    """2^20 channels x 128 frames, tiled 256, noise in every channel; two alternating buffer pairs, device events, median of 20
    after 5 warm-ups.  Asserted: a LowPass-everywhere bank of one stage equals Engine([LowPass]) on the same buffers bit for bit and
    takes at most twice its time (the margin every bank here gets over its uniform engine); a bank of four stages -- HighPass,
    LowPass, Envelope, LowPass present everywhere, own sliders per channel -- takes at most twice the engine of that four-node
    chain; both fit the 2.667 ms a 128-frame block lasts at 48 kHz.  Printed, not asserted: one stage with the kinds clustered by
    spans of 256; at 2^18 channels (the stores of an interleaved bank are three per four channels) the kinds interleaved per
    channel (c % 4) against the same kinds clustered; a half-present bank; a flat copy of the same bytes; milliseconds and the
    fraction of 8 TB/s on the bank's two block-units."""
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

    def engine_time(chain):
        eng = dspfx.Engine(n, nf, link_flags=0, tile_channels=tile)
        eng.set_chain(chain)
        t = timed(lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=nf))
        torch.cuda.synchronize()
        eng.close()
        return t

    assert dspfx.filters_plan(n, 4) == 13 * 4 * n
    rng = np.random.default_rng(9)
    # one stage, LowPass everywhere: the bits and the time of its engine.  25 timed runs + this one from a reset state against the
    # engine's 26th block would differ in state, so the bits are compared on a first block each
    one = dspfx.ChannelFilters(n, stages=1, tile_channels=tile, max_frames=nf)
    one.set_low_pass(0, 0.93)
    eng = dspfx.Engine(n, nf, link_flags=0, tile_channels=tile)
    eng.set_chain([dspfx.LowPass(0.93)])
    one.run(xs[0], nf, out=ys[0])
    eng.process(xs[0], out=ys[1], n_frames=nf)
    torch.cuda.synchronize()
    assert torch.equal(ys[0].view(torch.int32), ys[1].view(torch.int32)), "LowPass: the bank's bits are the engine's"
    eng.close()
    t_one = timed(lambda i: one.run(xs[i % 2], nf, out=ys[i % 2]))
    t_one_eng = engine_time([dspfx.LowPass(0.93)])
    # the same bank with the kinds clustered by spans of 256 channels: span s carries kind s % 4 of none / LP / HP / Env
    def cluster(bank, channels):
        bank.drop(0)
        for s in range(channels // 256):
            k = s % 4
            if k == 1:
                bank.set_low_pass(0, 0.93, first_channel=s * 256, count=256)
            elif k == 2:
                bank.set_high_pass(0, 0.05, first_channel=s * 256, count=256)
            elif k == 3:
                bank.set_envelope(0, 5.0, 64.0, first_channel=s * 256, count=256)

    cluster(one, n)
    assert list(one.kinds(0)[[0, 256, 512, 768]]) == [R.NONE, R.LOW_PASS, R.HIGH_PASS, R.ENVELOPE]
    t_cluster = timed(lambda i: one.run(xs[i % 2], nf, out=ys[i % 2]))
    # clustered against interleaved per channel (c % 4) on a quarter of the channels: an interleaved bank takes three stores per
    # four channels (through the C entry points on floats made once; a run now and then brings the small stores' staging buffers
    # back), which at 2^20 channels would be most of a minute
    m = n // 4
    small = dspfx.ChannelFilters(m, stages=1, tile_channels=tile, max_frames=nf)
    cluster(small, m)
    t_cluster_q = timed(lambda i: small.run(xs[i % 2], nf, out=ys[i % 2]))
    v = np.asarray([0.93, 0.05, 5.0, 64.0], F)
    p = [v[i:].ctypes.data_as(C.POINTER(C.c_float)) for i in range(4)]
    L, h = small.L, small.h
    small.drop(0)
    for c0 in range(0, m, 4):
        assert L.dspfx_filters_set_low_pass(h, 0, p[0], c0 + 1, 1) == 0
        assert L.dspfx_filters_set_high_pass(h, 0, p[1], c0 + 2, 1) == 0
        assert L.dspfx_filters_set_envelope(h, 0, p[2], p[3], c0 + 3, 1) == 0
        if (c0 // 4) % 1024 == 1023:
            small.run(xs[0], nf, out=ys[0])
            torch.cuda.synchronize()
    assert list(small.kinds(0, 0, 8)) == [R.NONE, R.LOW_PASS, R.HIGH_PASS, R.ENVELOPE] * 2
    t_inter_q = timed(lambda i: small.run(xs[i % 2], nf, out=ys[i % 2]))
    small.close()
    # half present: LowPass on every other span of 256
    one.drop(0)
    for s in range(0, n // 256, 2):
        one.set_low_pass(0, 0.93, first_channel=s * 256, count=256)
    t_half = timed(lambda i: one.run(xs[i % 2], nf, out=ys[i % 2]))
    one.close()
    # four stages, every slot present, own sliders per channel
    four = dspfx.ChannelFilters(n, stages=4, tile_channels=tile, max_frames=nf)
    four.set_high_pass(0, rng.uniform(0.01, 0.1, n).astype(F))
    four.set_low_pass(1, rng.uniform(0.5, 0.95, n).astype(F))
    four.set_envelope(2, rng.uniform(0.0, 48.0, n).astype(F), rng.uniform(0.0, 2400.0, n).astype(F))
    four.set_low_pass(3, rng.uniform(0.5, 0.95, n).astype(F))
    t_four = timed(lambda i: four.run(xs[i % 2], nf, out=ys[i % 2]))
    four.close()
    t_four_eng = engine_time([dspfx.HighPass(0.05), dspfx.LowPass(0.93), dspfx.Envelope(5.0, 64.0), dspfx.LowPass(0.5)])
    t_copy = timed(lambda i: ys[i % 2].copy_(xs[i % 2]))
    frac = lambda t: 2 * unit / t / 1e9 / 8.0                    # noqa: E731
    print(f"full size filters, one box, one run, {2 * unit / 2**20:.0f} MiB: one stage LowPass everywhere {t_one:.4f} ms ({frac(t_one):.3f} of 8 TB/s; "
          f"Engine([LowPass]) {t_one_eng:.4f} ms, bank x {t_one / t_one_eng:.3f}), four stages HP LP Env LP with own sliders {t_four:.4f} ms "
          f"({frac(t_four):.3f}; Engine of that chain {t_four_eng:.4f} ms, bank x {t_four / t_four_eng:.3f}), one stage none / LP / HP / Env clustered by "
          f"spans of 256 {t_cluster:.4f} ms ({frac(t_cluster):.3f}), at 2^18 channels clustered {t_cluster_q:.4f} ms against interleaved c % 4 "
          f"{t_inter_q:.4f} ms, LowPass on half the spans "
          f"{t_half:.4f} ms ({frac(t_half):.3f}), flat copy of the same bytes {t_copy:.4f} ms")
    assert t_one <= 2 * t_one_eng, (t_one, t_one_eng)
    assert t_four <= 2 * t_four_eng, (t_four, t_four_eng)
    assert t_one * 1e-3 <= 128 / 48000 and t_four * 1e-3 <= 128 / 48000, (t_one, t_four)
