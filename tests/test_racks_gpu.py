"""The channel-rack bank on the GPU (dspfx_racks_*, through the Python class): a per-channel chain of mixed nodes in 1 .. 4 slots,
one pass.  The contract is stated against banks that are already merged, and so are the tests: Sequence below builds, for a rack
table, the 3 x slots existing banks -- per slot a ChannelFilters of one stage, a ChannelStrips of one band with link_flags 0 and a
ChannelShapers, each persistent across runs and each carrying the slot's node on exactly the channels whose slot holds a kind of
its family -- mirrors every store onto them and runs them slot after slot on the same block; the rack's outputs and every slot's
state are compared with theirs bit for bit.  (The strips bank exports no state: a BiQuad slot's four state rows are held to the
sequence through the second block's output, which they determine, and to +0.0 wherever no BiQuad sits.)  Beside that: a
BiQuad-free channel equals Engine([its present nodes in slot order], link_flags=0) bit for bit, one engine per distinct chain,
made once per module and shared; a BiQuad slot is within 1 ulp of the engine's; single-node racks meet the oracle through
racks_ref at the bars tests/test_gpu_parity.py holds each node to.  Out-of-place outputs start as NaN everywhere, so every sample
is shown to be written."""
import ctypes as C
import threading

import numpy as np
import pytest

import edge_values as E
import racks_ref as R
import test_filters_gpu as TF
import test_racks_cpu as TC
from chains import ulp_diff
from test_gpu_parity import LIBM_COMPOSITE_ULP, LIBM_ULP

pytestmark = pytest.mark.gpu

NF = 128
F = np.float32
SHAPES = [(64, 0), (256, 64), (70, 0), (1, 0)]                   # vector lanes; tiled; scalar lanes with a ragged tail; one channel
WAVES = [(1028, 256), (261, 64)]                                 # (channels, the channels of one wave): test_wave_kinds_gpu's two shapes
FRAMES = [1, 37, 128]
EDGES = FRAMES + [4, 8, 9]                                       # the frame loop's boundaries with 4 or 8 rows a chunk: one chunk, two, chunks and a row
CUTS = (37, 128, 91)
NX = TF.NX
ENGINE_CHANNELS = 24                                             # the channels of a table that are also held to the engine of their chain
FILTER_KINDS, STRIP_KINDS, SHAPER_KINDS = (R.LOW_PASS, R.HIGH_PASS, R.ENVELOPE), (R.GAIN, R.BIQUAD), (R.DISTORT, R.OVERDRIVE, R.CHEBYSHEV)
bits, noise_x, device, host, run, run_cuts = TF.bits, TF.noise_x, TF.device, TF.host, TF.run, TF.run_cuts


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def singles(dspfx):
    """one node of every kind that is not a BiQuad, every Distort mode: the sliders the banks' own tests use"""
    return ([dspfx.Gain(1.75), dspfx.LowPass(0.93), dspfx.HighPass(0.05), dspfx.Envelope(5.0, 64.0), dspfx.Overdrive(5.0, 0.7, 0.9),
             dspfx.Chebyshev(2.0, 7.5)] + [dspfx.Distort(3.0, m) for m in TC.MODES])


def key(sp):
    return None if sp is None else (int(sp.kind), tuple(float(v) for v in sp.params), int(sp.mode))


def oracle_bar(sp):
    """the bar tests/test_gpu_parity.py holds the node to, in ulp"""
    k = int(sp.kind)
    if k in (R.GAIN, R.ENVELOPE):
        return 0
    if k in (R.OVERDRIVE, R.CHEBYSHEV):
        return LIBM_COMPOSITE_ULP
    return LIBM_ULP.get(int(sp.mode), 1) if k == R.DISTORT else 1


_ENGINE = {}


def engine_ref(dspfx, torch, chain):
    """Engine(chain, link_flags=0) on noise_x(), [256][NX], 128 frames at a time: computed once per distinct chain, shared, left
    unchanged.  Row f is what any cut of the frames gives"""
    k = tuple(key(sp) for sp in chain)
    if k not in _ENGINE:
        x = noise_x()
        eng = dspfx.Engine(NX, NF, link_flags=0)
        eng.set_chain(list(chain))
        y = np.empty_like(x)
        for f0 in range(0, len(x), NF):
            dx = torch.from_numpy(x[f0:f0 + NF].copy()).cuda()
            dy = torch.full_like(dx, float("nan"))
            eng.process(dx, out=dy, n_frames=NF)
            torch.cuda.synchronize()
            y[f0:f0 + NF] = dy.cpu().numpy()
        eng.close()
        y.setflags(write=False)
        _ENGINE[k] = y
    return _ENGINE[k]


class Sequence:
    """The 3 x slots existing banks of the contract, with the rack's methods: every store goes through racks_ref's tables (the
    store rules: what None keeps, what a new node starts from) and from there, resolved, onto the bank of the kind's family,
    while the slot's nodes of the other families are dropped on the stored channels.  A same-kind store reaches the filters bank
    as a same-kind store (the state stays) and the strips bank as a band store (the state is zeroed), as the banks have it."""

    def __init__(self, dspfx, n, slots, tile, max_frames=NF):
        self.n, self.slots = n, slots
        self.ref = R.ChannelRacks(n, slots, nodes=False)
        self.filters = [dspfx.ChannelFilters(n, stages=1, tile_channels=tile, max_frames=max_frames) for _ in range(slots)]
        self.strips = [dspfx.ChannelStrips(n, bands=1, tile_channels=tile, max_frames=max_frames, link_flags=0) for _ in range(slots)]
        self.shapers = [dspfx.ChannelShapers(n, tile_channels=tile, max_frames=max_frames) for _ in range(slots)]

    def set(self, slot, sp, first_channel=0, count=None):
        span = self.ref._span(slot, first_channel, count, list(sp.params) + [sp.mode if sp.kind == R.DISTORT else None])
        if not self.ref.set(slot, sp, first_channel, count):
            return False
        a, b = span
        if b == a:
            return True
        k, p, m = int(sp.kind), self.ref.p[slot, a:b], self.ref.mode[slot, a:b]
        f, s, h = self.filters[slot], self.strips[slot], self.shapers[slot]
        col = lambda t: np.ascontiguousarray(p[:, t])             # noqa: E731
        if k == R.LOW_PASS:
            f.set_low_pass(0, col(0), first_channel=a)
        elif k == R.HIGH_PASS:
            f.set_high_pass(0, col(0), first_channel=a)
        elif k == R.ENVELOPE:
            f.set_envelope(0, col(0), col(1), first_channel=a)
        else:
            f.drop(0, a, b - a)
        s.set_gain(col(0) if k == R.GAIN else None, a, b - a)
        s.set_band(0, np.ascontiguousarray(p) if k == R.BIQUAD else None, a, b - a)
        if k == R.DISTORT:
            h.set_distort(col(0), np.ascontiguousarray(m), first_channel=a)
        elif k == R.OVERDRIVE:
            h.set_overdrive(col(0), col(1), col(2), first_channel=a)
        elif k == R.CHEBYSHEV:
            h.set_chebyshev(col(0), col(1), first_channel=a)
        else:
            h.drop(a, b - a)
        return True

    def set_chain(self, specs, first_channel=0, count=None):
        specs = list(specs)
        for t, sp in enumerate(specs):
            self.set(t, sp, first_channel, count)
        for t in range(len(specs), self.slots):
            self.drop(t, first_channel, count)

    def drop(self, slot, first_channel=0, count=None):
        if not self.ref.drop(slot, first_channel, count):
            return False
        n = self.n - first_channel if count is None else count
        if n:
            self.filters[slot].drop(0, first_channel, n)
            self.strips[slot].set_gain(None, first_channel, n)
            self.strips[slot].set_band(0, None, first_channel, n)
            self.shapers[slot].drop(first_channel, n)
        return True

    def reset(self, first_channel=0, count=None, slot=None):
        if not self.ref.reset(first_channel, count, slot):
            return False
        n = self.n - first_channel if count is None else count
        for t in range(self.slots) if slot is None else (slot,):
            if n:
                self.filters[t].reset(first_channel, n, stage=0)
            for c in range(first_channel, first_channel + n):        # the strips bank zeroes a band's state through a band store
                if self.ref.kind[t, c] == R.BIQUAD:
                    self.strips[t].set_band(0, self.ref.p[t, c:c + 1], c)
        return True

    def run_inplace(self, dx, nf, stream=0):
        for t in range(self.slots):
            self.filters[t].run(dx, nf, out=dx, stream=stream)
            self.strips[t].run(dx, nf, out=dx, stream=stream)
            self.shapers[t].run(dx, nf, out=dx, stream=stream)
        return dx

    def run(self, dspfx, torch, x, tile):
        dx = device(dspfx, torch, x, tile)
        torch.cuda.synchronize()
        self.run_inplace(dx, len(x))
        torch.cuda.synchronize()
        return host(dspfx, dx, len(x), self.n, tile)

    def run_cuts(self, dspfx, torch, x, tile, cuts=CUTS):
        out, f0 = [], 0
        for k in cuts:
            out.append(self.run(dspfx, torch, x[f0:f0 + k], tile))
            f0 += k
        return np.concatenate(out)

    def filter_state(self, torch, slot):
        torch.cuda.synchronize()
        return self.filters[slot].state(0).cpu().numpy()

    def close(self):
        for b in self.filters + self.strips + self.shapers:
            b.close()


def store(banks, table):
    """table[c][slot] (a NodeSpec or None) onto every bank of `banks` (a rack, a Sequence, a racks_ref): per slot, consecutive
    channels of one kind in one store, the sliders and the modes as arrays"""
    n, slots = len(table), len(table[0])
    for t in range(slots):
        c = 0
        while c < n:
            k = None if table[c][t] is None else table[c][t].kind
            e = c
            while e < n and (None if table[e][t] is None else table[e][t].kind) == k:
                e += 1
            for b in banks:
                if k is None:
                    assert b.drop(t, c, e - c) is not False
                else:
                    sps = [table[i][t] for i in range(c, e)]
                    cols = [np.asarray([sp.params[j] for sp in sps], F) for j in range(len(sps[0].params))]
                    node = type(sps[0])(k, cols, mode=np.asarray([sp.mode for sp in sps], np.uint32) if k == R.DISTORT else 0)
                    assert b.set(t, node, first_channel=c) is not False
            c = e


def rotating(dspfx, n, slots, shift=0):
    """kinds (c + slot + shift) % 9 over empty and the eight kinds, Distort modes rotating with c, two slider sets alternating every
    four channels (test_racks_cpu.spec)"""
    return [tuple(TC.spec(dspfx, (c + t + shift) % 9, c) for t in range(slots)) for c in range(n)]


def rack_states(torch, rack):
    torch.cuda.synchronize()
    return np.stack([rack.state(t).cpu().numpy() for t in range(rack.slots)])


def same_states(torch, rack, seq, what):
    """row 0 is the filters bank's state wherever the slot carries no BiQuad; rows 1 .. 3 are +0.0 there"""
    st = rack_states(torch, rack)
    assert st.shape == (rack.slots, 4, rack.channels)
    for t in range(rack.slots):
        bq = seq.ref.kind[t] == R.BIQUAD
        assert np.array_equal(bits(st[t, 0][~bq]), bits(seq.filter_state(torch, t)[~bq])), (what, "slot", t)
        assert not bits(st[t, 1:][:, ~bq]).any(), (what, "slot", t, "rows 1 .. 3 without a BiQuad")
        stateless = ~np.isin(seq.ref.kind[t], FILTER_KINDS + (R.BIQUAD,))
        assert not bits(st[t][:, stateless]).any(), (what, "slot", t, "a slot without state is at rest")


def same_tables(rack, ref):
    for t in range(rack.slots):
        assert np.array_equal(rack.kinds(t), ref.kind[t]) and np.array_equal(rack.modes(t), ref.mode[t]), t
        assert np.array_equal(bits(rack.sliders(t)), bits(ref.p[t])), t
    assert np.array_equal(rack.present(), ref.present())


def engine_columns(dspfx, torch, got, table, cols, nf, what, channels=ENGINE_CHANNELS):
    """the first `channels` channels that carry no BiQuad: the bits of the engine of their own chain on column cols[c] of noise_x"""
    for c in range(min(channels, len(table))):
        chain = [sp for sp in table[c] if sp is not None]
        if not chain or any(sp.kind == R.BIQUAD for sp in chain):
            continue
        want = engine_ref(dspfx, torch, chain)[:nf, cols[c]]
        assert np.array_equal(bits(got[:nf, c]), bits(want)), (what, "channel", c, [key(sp) for sp in chain])


# ---- 1. a fresh bank -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", EDGES)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_a_fresh_bank_copies(dspfx, torch_cuda, n, tile, nf):
    slots = 1 + (n + nf) % 4
    rack = dspfx.ChannelRacks(n, slots=slots, tile_channels=tile, max_frames=NF)
    x = noise_x(nf)[:, :n]
    assert np.array_equal(bits(run(dspfx, torch_cuda, rack, x, n, tile)), bits(x))
    assert not rack.present().any() and not bits(rack_states(torch_cuda, rack)).any(), "every table at rest"
    for t in range(slots):
        assert (rack.kinds(t) == dspfx.RACKS_NONE).all() and (rack.modes(t) == dspfx.RACKS_NONE).all()
        assert not rack.sliders(t).any() and rack.sliders(t).shape == (n, 6)
    rack.close()


# ---- 2. one node everywhere equals that engine -----------------------------------------------------------------------------
@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_one_node_everywhere_equals_that_engine(dspfx, torch_cuda, n, tile, nf):
    """every kind but BiQuad and each of the eight Distort modes, in the first and in the last slot of a rack of four"""
    torch = torch_cuda
    rack = dspfx.ChannelRacks(n, slots=4, tile_channels=tile, max_frames=NF)
    x = noise_x(nf)[:, :n]
    for slot in (0, 3):
        for sp in singles(dspfx):
            rack.set_chain([])
            rack.set(slot, sp)
            got = run(dspfx, torch, rack, x, n, tile)
            want = engine_ref(dspfx, torch, [sp])
            assert np.array_equal(bits(got), bits(want[:nf, :n])), f"N={n} tile={tile} nf={nf} slot={slot} {key(sp)}"
            assert (rack.kinds(slot) == sp.kind).all() and (rack.present() == 1 << slot).all()
    rack.close()


@pytest.mark.parametrize("n,tile", SHAPES)
def test_biquad_everywhere_equals_the_strips_bank_and_is_within_1_ulp_of_the_engine(dspfx, torch_cuda, n, tile):
    torch = torch_cuda
    x = noise_x()[:, :n]
    for raw in TC.RAW:
        sp = dspfx.BiQuad(*raw)
        want_engine = engine_ref(dspfx, torch, [sp])[:, :n]
        strips = dspfx.ChannelStrips(n, bands=1, tile_channels=tile, max_frames=NF)
        strips.set_band(0, raw)
        want = run_cuts(dspfx, torch, strips, x, n, tile)
        strips.close()
        for slot in (0, 3):
            rack = dspfx.ChannelRacks(n, slots=4, tile_channels=tile, max_frames=NF)
            rack.set(slot, sp)
            got = run_cuts(dspfx, torch, rack, x, n, tile)
            assert np.array_equal(bits(got), bits(want)), f"N={n} tile={tile} slot={slot} {raw}: the strips bank's bits"
            d = int(ulp_diff(got, want_engine).max())
            print(f"N={n} tile={tile} slot={slot} {raw}: {d} ulp from the engine's BiQuad (bar 1)")
            assert d <= 1
            st = rack_states(torch, rack)[slot]
            assert np.array_equal(bits(st[0]), bits(x[-1])) and np.array_equal(bits(st[1]), bits(x[-2])), "x1, x2: the last two inputs"
            assert np.array_equal(bits(st[2]), bits(got[-1])) and np.array_equal(bits(st[3]), bits(got[-2])), "y1, y2: the last two outputs"
            rack.close()


# ---- 3. the sequence -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [1, 2, 4])
@pytest.mark.parametrize("n,tile", SHAPES)
def test_the_sequence_of_existing_banks_gives_the_same_bits_and_states(dspfx, torch_cuda, n, tile, slots):
    """kinds (c + slot) % 9, the Distort modes rotating with c, two slider sets, over two consecutive blocks"""
    torch = torch_cuda
    table = rotating(dspfx, n, slots)
    x = noise_x()[:, :n]
    rack, seq = dspfx.ChannelRacks(n, slots=slots, tile_channels=tile, max_frames=NF), Sequence(dspfx, n, slots, tile)
    store((rack, seq), table)
    same_tables(rack, seq.ref)
    for blk in range(2):
        xb = x[blk * NF:(blk + 1) * NF]
        got, want = run(dspfx, torch, rack, xb, n, tile), seq.run(dspfx, torch, xb, tile)
        bad = np.flatnonzero((bits(got) != bits(want)).any(axis=0))
        assert not len(bad), (f"N={n} tile={tile} slots={slots} block {blk}", bad[:8], [[key(sp) for sp in table[c]] for c in bad[:4]])
        same_states(torch, rack, seq, f"N={n} tile={tile} slots={slots} block {blk}")
        engine_columns(dspfx, torch, got, table, np.arange(n), NF, f"N={n} slots={slots}") if blk == 0 else None
    rack.close()
    seq.close()


def wave_layout(n, span, a, b, c, shift=0):
    """test_wave_kinds_gpu.layout: wave 0 carries a, wave 1 b, wave 2 a, b and empty interleaved, wave 3 nothing, the last lane c"""
    per_lane = span // 64
    wave = ([a] * span, [b] * span, [(a, b, None)[i % 3] for i in range(span)], [None] * span)
    out = [wave[(ch // span - shift) % 4][ch % span] for ch in range(4 * span)] + [None] * (n - 4 * span)
    out[n - per_lane:] = [c] * per_lane
    return out


@pytest.mark.parametrize("light", [False, True])
@pytest.mark.parametrize("n,span", WAVES)
def test_whole_waves_that_differ_in_their_kinds(dspfx, torch_cuda, n, span, light):
    """N = 1028 at four channels per lane (a 257th lane alone in a second workgroup), N = 261 at one; slot 1 is laid out one wave
    further on than slot 0.  light: kinds that take the instantiation without the f64 bodies"""
    torch = torch_cuda
    if light:
        a, b, c = dspfx.BiQuad(*TC.RAW[0]), dspfx.Distort(3.0, dspfx.SOFT_CLIP), dspfx.HighPass(0.05)
    else:
        a, b, c = dspfx.Envelope(5.0, 64.0), dspfx.Overdrive(5.0, 0.7, 0.9), dspfx.Chebyshev(2.0, 7.5)
    table = list(zip(wave_layout(n, span, a, b, c), wave_layout(n, span, a, b, None, shift=1)))
    cols = np.arange(n) % NX
    x = noise_x(37)[:, cols]
    rack, seq = dspfx.ChannelRacks(n, slots=2, max_frames=NF), Sequence(dspfx, n, 2, 0)
    store((rack, seq), table)
    got, want = run(dspfx, torch, rack, x, n, 0), seq.run(dspfx, torch, x, 0)
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=0))
    assert not len(bad), (f"N={n} light={light}", bad[:8])
    same_states(torch, rack, seq, f"N={n} light={light}")
    pick = [0, span, 2 * span, 2 * span + 1, 2 * span + 2, 3 * span, n - 1]       # one channel of every wave's kinds, and the last
    engine_columns(dspfx, torch, got[:, pick], [table[i] for i in pick], cols[pick], 37, f"waves N={n}", channels=len(pick))
    rack.close()
    seq.close()


# ---- 4. cuts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", SHAPES)
def test_however_the_frames_are_cut_the_bits_are_those_of_one_run(dspfx, torch_cuda, n, tile):
    torch = torch_cuda
    table = rotating(dspfx, n, 4)
    x = noise_x()[:, :n]
    outs = []
    for cuts in ((256,), CUTS, (1, 127, 3, 125)):
        rack = dspfx.ChannelRacks(n, slots=4, tile_channels=tile, max_frames=256)
        store((rack,), table)
        outs.append((run_cuts(dspfx, torch, rack, x, n, tile, cuts=cuts), rack_states(torch, rack)))
        rack.close()
    for y, st in outs[1:]:
        assert np.array_equal(bits(y), bits(outs[0][0])) and np.array_equal(bits(st), bits(outs[0][1]))
    assert not np.isnan(outs[0][0]).any()


# ---- 5. neighbours ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", [(64, 0), (256, 64), (70, 0)])
def test_a_nan_and_an_infinity_in_one_channel_change_no_other_channels_bits(dspfx, torch_cuda, n, tile):
    """... and neither do the neighbours' kinds: the kept channels (one of each lane's four, and the last) carry the same chains in
    a second rack whose other channels carry other kinds and NaN or infinite samples"""
    torch = torch_cuda
    keep = np.zeros(n, bool)
    keep[(np.arange(n) % 4) == (np.arange(n) // 4) % 4] = True
    keep[n - 1] = True
    ta, other = rotating(dspfx, n, 4), rotating(dspfx, n, 4, shift=5)
    tb = [ta[c] if keep[c] else other[c] for c in range(n)]
    x = noise_x(NF)[:, :n]
    xb = x.copy()
    xb[:, np.flatnonzero(~keep)[::2]] = np.nan
    xb[5:, np.flatnonzero(~keep)[1::2]] = np.inf
    outs = []
    for table, xx in ((ta, x), (tb, xb)):
        rack = dspfx.ChannelRacks(n, slots=4, tile_channels=tile, max_frames=NF)
        store((rack,), table)
        outs.append((run(dspfx, torch, rack, xx, n, tile), rack_states(torch, rack)))
        rack.close()
    assert np.array_equal(bits(outs[0][0][:, keep]), bits(outs[1][0][:, keep])) and np.array_equal(bits(outs[0][1][:, :, keep]), bits(outs[1][1][:, :, keep]))
    assert not np.isnan(outs[0][0]).any() and np.isnan(outs[1][0][:, ~keep]).any()
    # one poisoned channel in an otherwise equal rack: every other column keeps its bits
    rack = dspfx.ChannelRacks(n, slots=4, tile_channels=tile, max_frames=NF)
    store((rack,), ta)
    xc = x.copy()
    xc[3, n // 2], xc[9, n // 2] = np.nan, np.inf
    got = run(dspfx, torch, rack, xc, n, tile)
    rack.close()
    others = np.arange(n) != n // 2
    assert np.array_equal(bits(got[:, others]), bits(outs[0][0][:, others]))


# ---- 6. the run's forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", EDGES)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_in_place_equals_out_of_place(dspfx, torch_cuda, n, tile, nf):
    torch = torch_cuda
    rack = dspfx.ChannelRacks(n, slots=4, tile_channels=tile, max_frames=NF)
    store((rack,), rotating(dspfx, n, 4))
    x = noise_x(nf)[:, :n]
    out = run(dspfx, torch, rack, x, n, tile)
    rack.reset()
    assert np.array_equal(bits(run(dspfx, torch, rack, x, n, tile, inplace=True)), bits(out)) and not np.isnan(out).any()
    rack.close()


@pytest.mark.parametrize("slots", [2, 3, 4])
def test_both_layouts_give_the_same_bits(dspfx, torch_cuda, slots):
    torch = torch_cuda
    n = 256
    table = rotating(dspfx, n, slots)
    outs = []
    for tile in (0, 64, 256):
        rack = dspfx.ChannelRacks(n, slots=slots, tile_channels=tile, max_frames=NF)
        store((rack,), table)
        outs.append((run_cuts(dspfx, torch, rack, noise_x()[:, :n], n, tile), rack_states(torch, rack)))
        rack.close()
    for y, st in outs[1:]:
        assert np.array_equal(bits(y), bits(outs[0][0])) and np.array_equal(bits(st), bits(outs[0][1]))
    engine_columns(dspfx, torch, outs[0][0], table, np.arange(n), 2 * NF, f"slots={slots}")


@pytest.mark.parametrize("slots", [2, 4])
def test_out_of_place_from_an_unaligned_pointer_takes_the_scalar_path(dspfx, torch_cuda, slots):
    """N = 64 would take four (two at four slots) channels per lane; the blocks start 4 bytes past a 16-byte boundary, so a lane
    takes one"""
    torch = torch_cuda
    n, tile, nf = 64, 0, 37
    table = rotating(dspfx, n, slots)
    rack, twin = (dspfx.ChannelRacks(n, slots=slots, tile_channels=tile, max_frames=NF) for _ in range(2))
    store((rack, twin), table)
    x = noise_x(nf)[:, :n]
    big = torch.zeros(nf * n + 8, dtype=torch.float32, device="cuda")
    out = torch.full((nf * n + 8,), float("nan"), dtype=torch.float32, device="cuda")
    big[1:1 + nf * n] = device(dspfx, torch, x, tile)
    dx, dy = big[1:1 + nf * n], out[3:3 + nf * n]
    assert dx.data_ptr() % 16 == 4 and dy.data_ptr() % 16 == 12
    rack.run(dx, nf, out=dy)
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(dspfx, dy, nf, n, tile)), bits(run(dspfx, torch, twin, x, n, tile)))
    assert np.isnan(out[:3].cpu().numpy()).all() and np.isnan(out[3 + nf * n:].cpu().numpy()).all(), "nothing outside the block is written"
    assert np.array_equal(bits(rack_states(torch, rack)), bits(rack_states(torch, twin)))
    rack.close()
    twin.close()


def test_a_null_pointer_or_no_frames_is_refused(dspfx, torch_cuda):
    torch = torch_cuda
    n = 64
    rack = dspfx.ChannelRacks(n, slots=1, max_frames=NF)
    dx = device(dspfx, torch, noise_x(NF)[:, :n], 0)
    L, p = rack.L, C.c_void_p(dx.data_ptr())
    assert L.dspfx_racks_run(rack.h, None, p, NF, None) == -1 and b"racks run" in L.dspfx_racks_last_error(rack.h)
    assert L.dspfx_racks_run(rack.h, p, None, NF, None) == -1
    for nf in (0, NF + 1):
        with pytest.raises(dspfx.DspfxError) as e:
            rack.run(dx, nf, out=dx)
        assert e.value.status == -1 and "n_frames" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert np.array_equal(bits(dx.cpu().numpy().reshape(NF, n)), bits(noise_x(NF)[:, :n])), "a refused run writes nothing"
    rack.close()


def test_two_streams(dspfx, torch_cuda):
    """the cuts alternate between two streams and nothing waits in between: the state is the bank's, so a run on another stream
    waits on the device for the one before"""
    torch = torch_cuda
    n, tile = 256, 64
    table = rotating(dspfx, n, 4)
    x = noise_x()[:, :n]
    rack, twin = (dspfx.ChannelRacks(n, slots=4, tile_channels=tile, max_frames=NF) for _ in range(2))
    store((rack, twin), table)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    dxs, dys, f0 = [], [], 0
    for k in CUTS:
        dxs.append(device(dspfx, torch, x[f0:f0 + k], tile))
        dys.append(torch.full_like(dxs[-1], float("nan")))
        f0 += k
    torch.cuda.synchronize()
    for i, k in enumerate(CUTS):
        rack.run(dxs[i], k, out=dys[i], stream=streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    got = np.concatenate([host(dspfx, dys[i], k, n, tile) for i, k in enumerate(CUTS)])
    assert np.array_equal(bits(got), bits(run_cuts(dspfx, torch, twin, x, n, tile)))
    assert np.array_equal(bits(rack_states(torch, rack)), bits(rack_states(torch, twin)))
    rack.close()
    twin.close()


# ---- 7. store rules --------------------------------------------------------------------------------------------------------
def test_store_rules_on_the_device_follow_the_restatement_and_the_sequence(dspfx, torch_cuda):
    """between two runs: same-kind stores (the state stays, a BiQuad's is zeroed), kind changes, a drop, resets of a sub-range and
    of one slot, a drop followed by a set, set_chain; nothing waits between the calls of a round.  The rack, the sequence and
    racks_ref get the same calls"""
    torch = torch_cuda
    n, tile = 70, 0
    x = noise_x()[:, :n]
    a, b = x[:37], x[37:165]
    rack, seq, ref = dspfx.ChannelRacks(n, slots=2, tile_channels=tile, max_frames=NF), Sequence(dspfx, n, 2, tile), R.ChannelRacks(n, 2)
    all3 = (rack, seq, ref)
    base = [(dspfx.HighPass(0.05), dspfx.BiQuad(*TC.RAW[0]))] * n
    store(all3, base)
    got_a = run(dspfx, torch, rack, a, n, tile)
    assert np.array_equal(bits(got_a), bits(seq.run(dspfx, torch, a, tile)))
    ref.run(a)
    z_before = rack_states(torch, rack)
    for k in all3:
        assert k.set(0, dspfx.HighPass(None), first_channel=0, count=5) is not False                  # the same kind, nothing given: all is kept
        assert k.set(0, dspfx.HighPass(0.5), first_channel=5, count=5) is not False                   # the same kind, a new ratio: the state is kept
        assert k.set(1, dspfx.BiQuad(None, None, None, None, None, None), first_channel=0, count=3) is not False     # a BiQuad store zeroes the state
        assert k.set(1, dspfx.BiQuad(b0=0.5), first_channel=3, count=3) is not False                  # (every slider given here: the defaults' a0 .. a2)
        assert k.set(0, dspfx.LowPass(None), first_channel=10, count=5) is not False                  # another kind: ratio 0.5, state +0.0
        assert k.set(1, dspfx.Envelope(None, 64.0), first_channel=10, count=5) is not False           # BiQuad -> Envelope: attack 0, state +0.0
        assert k.set(0, dspfx.Distort(3.0, dspfx.TANH), first_channel=15, count=5) is not False       # a filter becomes a shaper
        assert k.set(0, dspfx.Distort(None, dspfx.SIN), first_channel=17, count=3) is not False       # the level is kept
        assert k.set(1, dspfx.Gain([0.5, 1.5, 2.5, 3.5, 4.5]), first_channel=20) is not False         # a BiQuad becomes a Gain
        assert k.drop(0, 30, 10) is not False                                                         # slot 0 copies again
        assert k.reset(first_channel=40, count=10) is not False                                       # every slot of a sub-range
        assert k.reset(first_channel=50, count=10, slot=1) is not False                               # one slot
        assert k.drop(1, 60, 5) is not False and k.set(1, dspfx.BiQuad(*TC.RAW[1]), first_channel=60, count=5) is not False   # dropped, set again
        k.set_chain([dspfx.Overdrive(5, .7, .9)], first_channel=65, count=3)                         # slot 1 is dropped behind the list
        k.set_chain([dspfx.Overdrive(None, None, 0.0005), dspfx.LowPass(0.9)], first_channel=67, count=1)     # a bypassed Overdrive, then a LowPass
    same_tables(rack, ref)
    assert list(rack.kinds(1, 65, 5)) == [R.NONE, R.NONE, R.LOW_PASS, R.BIQUAD, R.BIQUAD] and list(rack.sliders(0, 67, 1)[0, :3]) == [5.0, F(0.7), F(0.0005)]
    assert list(rack.modes(0, 15, 5)) == [dspfx.TANH, dspfx.TANH, dspfx.SIN, dspfx.SIN, dspfx.SIN] and (rack.sliders(0, 15, 5)[:, 0] == 3.0).all()
    got_b = run(dspfx, torch, rack, b, n, tile)
    want_b = seq.run(dspfx, torch, b, tile)
    bad = np.flatnonzero((bits(got_b) != bits(want_b)).any(axis=0))
    assert not len(bad), ("after the stores", bad)
    same_states(torch, rack, seq, "after the stores")
    z = rack_states(torch, rack)
    # ... and the restatement's run: LowPass then Envelope on channels 10 .. 14, at the filters bank's bar for a chain with a one-pole
    d = int(ulp_diff(got_b[:, 10:15], ref.run(b)[:, 10:15]).max())
    print(f"LowPass(0.5) -> Envelope(0, 64) after the stores, against the oracle through racks_ref: {d} ulp (bar 1)")
    assert d <= 1
    # what the rules mean for the bits: kept state continues, a zeroed one starts as a fresh bank does
    fresh = dspfx.ChannelRacks(n, slots=2, tile_channels=tile, max_frames=NF)
    for t in range(2):
        for c in range(n):
            k = int(ref.kind[t, c])
            if k != R.NONE:
                fresh.set(t, dspfx.NodeSpec(k, [float(v) for v in ref.p[t, c, :R.SLIDERS[k]]], mode=int(ref.mode[t, c]) if k == R.DISTORT else 0), first_channel=c, count=1)
    got_fresh = run(dspfx, torch, fresh, b, n, tile)
    fresh.close()
    assert not np.array_equal(bits(got_b[:, 6:10]), bits(got_fresh[:, 6:10])), "a new ratio on the old state"
    assert np.array_equal(bits(got_b[:, 10:15]), bits(got_fresh[:, 10:15])), "kind changes in both slots start from +0.0"
    assert not np.array_equal(bits(got_b[:, 15:25]), bits(got_fresh[:, 15:25])), "a kind change in one slot leaves the other slot's state"
    assert np.array_equal(bits(got_b[:, 40:50]), bits(got_fresh[:, 40:50])), "reset of every slot"
    assert not np.array_equal(bits(got_b[:, 30:40]), bits(got_fresh[:, 30:40])), "a drop of slot 0 leaves slot 1's state"
    assert not np.array_equal(bits(got_b[:, 50:60]), bits(got_fresh[:, 50:60])), "reset of slot 1 leaves slot 0's state"
    assert not bits(z[0, :, 30:40]).any() and bits(z_before[0, 0, 30:40]).any(), "a dropped slot's state is +0.0"
    rack.close()
    seq.close()


def test_a_refused_store_changes_nothing(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile = 70, 0
    table = rotating(dspfx, n, 2)
    rack = dspfx.ChannelRacks(n, slots=2, tile_channels=tile, max_frames=NF)
    twin = dspfx.ChannelRacks(n, slots=2, tile_channels=tile, max_frames=NF)
    ref = R.ChannelRacks(n, 2, nodes=False)
    store((rack, twin, ref), table)
    x = noise_x()[:, :n]
    first = run(dspfx, torch, rack, x[:NF], n, tile)
    bad = [(lambda k: k.set(2, dspfx.Gain(1.0)), "slot"), (lambda k: k.set(4, dspfx.Gain(1.0), first_channel=0, count=1), "slot"),
           (lambda k: k.set(0, dspfx.Envelope(1.0, 2.0), first_channel=n - 1, count=2), "channels"),
           (lambda k: k.set(0, dspfx.Gain(1.0), first_channel=n + 1, count=0), "channels"),
           (lambda k: k.set(1, dspfx.Envelope(np.ones(3, F), np.ones(4, F))), "different numbers"),
           (lambda k: k.set(0, dspfx.Reverb(0.1)), "delays"), (lambda k: k.set(0, dspfx.Fir()), "firs"), (lambda k: k.set(0, dspfx.Add()), "blends"),
           (lambda k: k.set(0, dspfx.Mix(0.5)), "blends"), (lambda k: k.set(0, dspfx.SignalGen()), "gens"),
           (lambda k: k.set(0, dspfx.NodeSpec(13, [1.0])), "kind"), (lambda k: k.set(0, dspfx.Distort(3.0, dspfx.FUZZ)), "shapers"),
           (lambda k: k.set(0, dspfx.Distort(3.0, [1, 2, dspfx.FUZZ]), first_channel=4), "Fuzz"), (lambda k: k.set(0, dspfx.Distort(3.0, 9)), "mode"),
           (lambda k: k.drop(2, 0, 1), "slot"), (lambda k: k.drop(0, n, 1), "channels"), (lambda k: k.reset(slot=2), "slot"),
           (lambda k: k.reset(first_channel=0, count=n + 1), "channels")]
    for call, word in bad:
        with pytest.raises(dspfx.DspfxError) as e:
            call(rack)
        assert e.value.status == -1 and word in str(e.value) and "racks" in str(e.value), str(e.value)
        if word != "different numbers":                          # (that one is the Python layer's: C arrays carry no lengths)
            assert word.encode() in rack.L.dspfx_racks_last_error(rack.h)
        assert call(ref) is False
    for call in (lambda: rack.kinds(2), lambda: rack.modes(2), lambda: rack.sliders(2), lambda: rack.state(2), lambda: rack.present(1, n)):
        with pytest.raises(dspfx.DspfxError):
            call()
    same_tables(rack, ref)
    got = np.concatenate([first, run(dspfx, torch, rack, x[NF:], n, tile)])
    assert np.array_equal(bits(got), bits(run_cuts(dspfx, torch, twin, x, n, tile, cuts=(NF, NF)))), "after the refused stores: the state and the nodes as they were"
    assert np.array_equal(bits(rack_states(torch, rack)), bits(rack_states(torch, twin)))
    rack.set(0, dspfx.Gain([float("nan"), float("inf"), -3.0, 75.0]), first_channel=0)                  # taken as given
    rack.set(1, dspfx.Envelope(float("nan"), -1.0), first_channel=0, count=1)
    assert np.isnan(rack.sliders(0)[0, 0]) and list(rack.sliders(0)[1:4, 0]) == [np.inf, -3.0, 75.0] and rack.sliders(1)[0, 1] == -1.0
    assert np.isnan(run(dspfx, torch, rack, x[:NF], n, tile)[:, 0]).all()
    rack.close()
    twin.close()


def test_a_thread_storing_kind_changes_while_blocks_are_submitted(dspfx, torch_cuda):
    """a second thread stores HighPass / Envelope over the whole range of slot 1, alternating, while the first submits runs of one
    block, and nothing waits.  Every store changes the kind, so it makes new nodes: a run equals block j of the engine of one
    chain, where j counts the runs since the last store it saw -- and then the run before it was block j - 1 of the same chain.
    Slot 0's Gain and slot 2's SoftClip stay.  A store is whole"""
    torch = torch_cuda
    n, tile, runs = 256, 64, 40
    kinds = (dspfx.HighPass(0.05), dspfx.Envelope(5.0, 64.0))
    gain, clip = dspfx.Gain(1.75), dspfx.Distort(3.0, dspfx.SOFT_CLIP)
    x = noise_x(NF)[:, :n]
    blocks = []
    for sp in kinds:
        eng = dspfx.Engine(n, NF, link_flags=0)
        eng.set_chain([gain, sp, clip])
        dx = torch.from_numpy(x.copy()).cuda()
        ys = []
        for _ in range(runs):
            dy = torch.full_like(dx, float("nan"))
            eng.process(dx, out=dy, n_frames=NF)
            ys.append(dy)
        torch.cuda.synchronize()
        blocks.append(np.stack([bits(y.cpu().numpy()) for y in ys]))
        eng.close()
    rack = dspfx.ChannelRacks(n, slots=3, tile_channels=tile, max_frames=NF)
    rack.set_chain([gain, kinds[0], clip])
    dx = device(dspfx, torch, x, tile)
    dys = [torch.full_like(dx, float("nan")) for _ in range(runs)]
    torch.cuda.synchronize()
    done, errors, made = threading.Event(), [], [0]

    def storer():
        try:
            while not done.is_set() or made[0] < 20:
                rack.set(1, kinds[(made[0] + 1) % 2])
                made[0] += 1
        except Exception as e:                                   # noqa: BLE001
            errors.append(e)

    t = threading.Thread(target=storer)
    t.start()
    for i in range(runs):
        rack.run(dx, NF, out=dys[i])
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
    assert rack.kinds(1)[0] in (R.HIGH_PASS, R.ENVELOPE) and (rack.kinds(0) == R.GAIN).all() and (rack.kinds(2) == R.DISTORT).all()
    rack.close()


# ---- 8. edge values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", [(256, 64), (70, 0)])
def test_edge_values_through_every_kind(dspfx, torch_cuda, n, tile):
    """NaN, both infinities, signed zeros, subnormals, each class in a channel of its own, through a rack of each kind against
    the sequence's bank of that kind on the same block: NaN positions and all other bits; then through empty slots: every edge
    value's very bits"""
    torch = torch_cuda
    x, tab = E.edge_block(n, 2 * NF)
    rack, seq = dspfx.ChannelRacks(n, slots=1, tile_channels=tile, max_frames=2 * NF), Sequence(dspfx, n, 1, tile, max_frames=2 * NF)
    for sp in singles(dspfx) + [dspfx.BiQuad(*TC.RAW[0]), dspfx.LowPass(1.0), dspfx.HighPass(0.0), dspfx.Envelope(0.0, 0.0), dspfx.Gain(0.0)]:
        for k in (rack, seq):
            k.set(0, sp)
            k.reset()
        got, want = run(dspfx, torch, rack, x, n, tile), seq.run(dspfx, torch, x, tile)
        E.same_bits_or_nan(got, want, tab, f"N={n} {key(sp)}")
    rack.drop(0)
    assert np.array_equal(bits(run(dspfx, torch, rack, x, n, tile)), bits(x)), "no node: every edge value's very bits"
    rack.close()
    seq.close()


# ---- 9. the oracle ---------------------------------------------------------------------------------------------------------
def test_single_node_racks_against_the_oracle_through_the_restatement(dspfx, torch_cuda):
    """each kind alone in a slot over 37 + 128 + 91 frames, at the bar tests/test_gpu_parity.py holds that node to: Gain and
    Envelope 0 ulp, BiQuad, the one-poles and the arithmetic Distort modes 1, Tanh 2, Sin and Atan 1, Overdrive and Chebyshev 4"""
    torch = torch_cuda
    n, tile = 70, 0
    x = noise_x()[:, :n]
    for sp in singles(dspfx) + [dspfx.BiQuad(*raw) for raw in TC.RAW]:
        rack, ref = dspfx.ChannelRacks(n, slots=2, tile_channels=tile, max_frames=NF), R.ChannelRacks(n, 2)
        for k in (rack, ref):
            assert k.set(1, sp) is not False
        got = run_cuts(dspfx, torch, rack, x, n, tile)
        want = np.concatenate([ref.run(x[:37]), ref.run(x[37:165]), ref.run(x[165:])])
        rack.close()
        assert np.array_equal(np.isnan(got), np.isnan(want)), key(sp)
        d = int(ulp_diff(got, want).max())
        print(f"{key(sp)}: {d} ulp against the oracle (bar {oracle_bar(sp)})")
        assert d <= oracle_bar(sp), (key(sp), d)


# ---- 10. full size ---------------------------------------------------------------------------------------------------------
def test_full_size(dspfx, torch_cuda):
    """2^20 channels x 128 frames, tiled 256, noise in every channel; two alternating buffer pairs, device events, median of 20
    after 5 warm-ups.  Every channel carries HighPass, Gain, BiQuad, SoftClip Distort with its own sliders.  Asserted: the first
    block's bits equal those of ChannelFilters(1) -> ChannelStrips(bands=1) with gain -> ChannelShapers on the same buffers; the
    rack's time is less than that three-bank sequence's time measured here, and fits the 2.667 ms a 128-frame block lasts at
    48 kHz.  Printed, not asserted: milliseconds and the fraction of 8 TB/s on the rack's own bytes (block in, block out, tables
    read, state written); the ratio to the sequence; the ratio to Engine([HighPass, Gain, BiQuad, Distort]) with uniform sliders;
    a flat copy of the block; a rack with a Tanh slot (the f64 instantiation); kinds clustered by spans of 256; at 2^18 channels
    (an interleaved bank takes a store per channel and slot) kinds interleaved per channel in the first slot against the same kinds
    clustered; a
    half-present bank."""
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

    assert dspfx.racks_plan(n, 4) == 37 * 4 * n
    rng = np.random.default_rng(9)
    hp, lv = rng.uniform(0.01, 0.1, n).astype(F), rng.uniform(0.25, 4.0, n).astype(F)
    raw, dl = R.strips_ref.stable_raw6(rng, n), rng.uniform(1.0, 8.0, n).astype(F)
    rack = dspfx.ChannelRacks(n, slots=4, tile_channels=tile, max_frames=nf)
    rack.set_chain([dspfx.HighPass(hp), dspfx.Gain(lv), dspfx.BiQuad(*[np.ascontiguousarray(raw[:, j]) for j in range(6)]), dspfx.Distort(dl, dspfx.SOFT_CLIP)])
    filt = dspfx.ChannelFilters(n, stages=1, tile_channels=tile, max_frames=nf)
    filt.set_high_pass(0, hp)
    strips = dspfx.ChannelStrips(n, bands=1, tile_channels=tile, max_frames=nf)
    strips.set_gain(lv)
    strips.set_band(0, raw)
    shap = dspfx.ChannelShapers(n, tile_channels=tile, max_frames=nf)
    shap.set_distort(dl, dspfx.SOFT_CLIP)

    def sequence(i):
        filt.run(xs[i % 2], nf, out=ys[i % 2])
        strips.run(ys[i % 2], nf, out=ys[i % 2])
        shap.run(ys[i % 2], nf, out=ys[i % 2])

    rack.run(xs[0], nf, out=ys[0])
    torch.cuda.synchronize()
    first = ys[0].clone()
    filt.run(xs[0], nf, out=ys[1])                               # (the three banks are fresh: their first block too)
    strips.run(ys[1], nf, out=ys[1])
    shap.run(ys[1], nf, out=ys[1])
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), ys[1].view(torch.int32)), "the rack's bits are the three-bank sequence's"
    del first
    t_rack = timed(lambda i: rack.run(xs[i % 2], nf, out=ys[i % 2]))
    t_seq = timed(sequence)
    for b in (filt, strips, shap):
        b.close()
    eng = dspfx.Engine(n, nf, link_flags=0, tile_channels=tile)
    eng.set_chain([dspfx.HighPass(0.05), dspfx.Gain(1.75), dspfx.BiQuad(*TC.RAW[0]), dspfx.Distort(3.0, dspfx.SOFT_CLIP)])
    t_eng = timed(lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=nf))
    torch.cuda.synchronize()
    eng.close()
    t_copy = timed(lambda i: ys[i % 2].copy_(xs[i % 2]))
    # the rack's own bytes: block in, block out, per slot the kind byte, the slider fields read and the state rows read and written
    own = 2 * unit + n * ((1 + 4 + 2 * 4) + (1 + 4) + (1 + 5 * 4 + 2 * 4 * 4) + (1 + 4))
    # a Tanh in the last slot: the instantiation with the f64 bodies
    rack.set(3, dspfx.Distort(dl, dspfx.TANH))
    t_tanh = timed(lambda i: rack.run(xs[i % 2], nf, out=ys[i % 2]))
    # kinds clustered by spans of 256: span s carries the chain rotated by s (every wave one kind per slot, the kinds differ by wave)
    chain = [dspfx.HighPass(0.05), dspfx.Gain(1.75), dspfx.BiQuad(*TC.RAW[0]), dspfx.Distort(3.0, dspfx.SOFT_CLIP)]

    def cluster(bank, channels, span):
        made = 0
        for t in range(4):
            for r in range(4):
                sp = chain[(t + r) % 4]
                cols = [np.repeat(np.asarray([v], F), span) for v in sp.params]
                for s in range(r, channels // span, 4):
                    bank.set(t, dspfx.NodeSpec(sp.kind, cols, mode=sp.mode), first_channel=s * span)
                    made += 1
                    if made % 2048 == 0:                         # (a run now and then brings the stores' staging buffers back)
                        bank.run(xs[0], nf, out=ys[0])
                        torch.cuda.synchronize()

    cluster(rack, n, 256)
    assert list(rack.kinds(0)[[0, 256, 512, 768]]) == [R.HIGH_PASS, R.GAIN, R.BIQUAD, R.DISTORT]
    t_cluster = timed(lambda i: rack.run(xs[i % 2], nf, out=ys[i % 2]))
    # half present: every other span of 256 empty in every slot
    for t in range(4):
        for s in range(0, n // 256, 2):
            rack.drop(t, s * 256, 256)
    t_half = timed(lambda i: rack.run(xs[i % 2], nf, out=ys[i % 2]))
    rack.close()
    # clustered against interleaved per channel on a quarter of the channels: slot 0 carries the chain rotated by the channel (a
    # lane's channels differ, every wave holds all four kinds), slots 1 .. 3 stay clustered: one store per channel through the C
    # entry point on floats made once (a run now and then brings the small stores' staging buffers back); all four slots that
    # way would be a million stores
    m = n // 4
    small = dspfx.ChannelRacks(m, slots=4, tile_channels=tile, max_frames=nf)
    cluster(small, m, 256)
    t_cluster_q = timed(lambda i: small.run(xs[i % 2], nf, out=ys[i % 2]))
    L, h = small.L, small.h
    fp = C.POINTER(C.c_float)
    six = []
    for sp in chain:
        v = np.asarray(list(sp.params) + [0.0] * (6 - len(sp.params)), F)
        six.append(((fp * 6)(*[v[j:].ctypes.data_as(fp) for j in range(6)]), v))
    mode = (C.c_uint32 * 1)(dspfx.SOFT_CLIP)
    for c in range(m):
        assert L.dspfx_racks_set(h, 0, chain[c % 4].kind, six[c % 4][0], mode, c, 1) == 0
        if c % 4096 == 4095:
            small.run(xs[0], nf, out=ys[0])
            torch.cuda.synchronize()
    assert list(small.kinds(0, 0, 8)) == [R.HIGH_PASS, R.GAIN, R.BIQUAD, R.DISTORT] * 2 and list(small.kinds(1, 0, 4)) == [R.GAIN] * 4
    t_inter_q = timed(lambda i: small.run(xs[i % 2], nf, out=ys[i % 2]))
    small.close()
    frac = lambda t, b=own: b / t / 1e9 / 8.0                    # noqa: E731
    print(f"full size racks, one box, one run, 2^20 x 128, {own / 2**20:.0f} MiB of the rack's own bytes: HighPass, Gain, BiQuad, SoftClip with own sliders "
          f"{t_rack:.4f} ms ({frac(t_rack):.3f} of 8 TB/s); the three-bank sequence {t_seq:.4f} ms, rack x {t_rack / t_seq:.3f}; "
          f"Engine of that chain, uniform sliders {t_eng:.4f} ms, rack x {t_rack / t_eng:.3f}; flat copy of the block {t_copy:.4f} ms; "
          f"Tanh in the last slot (the f64 instantiation) {t_tanh:.4f} ms; the four kinds clustered by spans of 256, rotated per span {t_cluster:.4f} ms; "
          f"half of the spans empty {t_half:.4f} ms; at 2^18 channels clustered {t_cluster_q:.4f} ms against slot 0 interleaved per channel {t_inter_q:.4f} ms")
    assert t_rack < t_seq, (t_rack, t_seq)
    assert t_rack * 1e-3 <= 128 / 48000, t_rack
