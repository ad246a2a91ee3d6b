"""The wave-uniform kind word of the shaper, generator and filter banks (one ballot per kind behind lane_io.hip.h's lane_channel) at
the shapes no other test has: whole waves that differ in their kind sets, and a bank that crosses a workgroup on the vector path.

Per case the first workgroup's wave 0 carries kind A only, wave 1 kind B only, wave 2 A, B and empty channels interleaved, wave 3
no node at all; the last lane, alone in the second workgroup at N = 1028, carries a kind C that no other channel has.  N = 1028
(tile 0, aligned blocks) is four channels per lane: 257 lanes, waves of 256 channels.  N = 261 is one channel per lane: waves of 64
channels and a second workgroup of 5 lanes.  37 frames are nine 4-row chunks and a row for the filters at four channels per lane,
four 8-row chunks and five rows everywhere else.  The filters have two stages, stage 1 laid out as stage 0 one wave further on.

Every channel's bits are those of the engine of its own setting, through each bank's own expected(): one engine per distinct
setting, shared with the banks' own tests."""
import numpy as np
import pytest

import test_filters_gpu as TF
import test_gens_gpu as TG
import test_shapers_gpu as TS

pytestmark = pytest.mark.gpu

NF = 37
SHAPES = [(1028, 256), (261, 64)]                                # (channels, the channels of one wave)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module", autouse=True)
def gens_engines():
    """test_gens_gpu keeps one engine per mode open for its expectations: closed here as its own module closes them"""
    yield
    for e in TG._ENG.values():
        e.close()
    TG._ENG.clear()
    TG._COL.clear()


def layout(n, span, a, b, c, shift=0):
    """the setting of every channel: waves 0 .. 3 as above, moved `shift` waves on (cyclic over the four); behind them nothing,
    but `c` on the last lane's channels"""
    per_lane = span // 64
    wave = ([a] * span, [b] * span, [(a, b, None)[i % 3] for i in range(span)], [None] * span)
    out = [wave[(ch // span - shift) % 4][ch % span] for ch in range(4 * span)] + [None] * (n - 4 * span)
    out[n - per_lane:] = [c] * per_lane
    return out


def check(got, want, settings, what):
    bad = np.flatnonzero((TS.bits(got) != TS.bits(want)).any(axis=0))
    assert not len(bad), (what, "channels", bad[:8], [settings[c] for c in bad[:8]])


@pytest.mark.parametrize("n,span", SHAPES)
def test_shapers(dspfx, torch_cuda, n, span):
    """A: Distort Tanh, B: Overdrive, C: Chebyshev: all three evaluate in f64, the heavy kernel (none gives a NaN on this input)"""
    settings = layout(n, span, ("d", 3.0, 2), ("o", 5.0, 0.7, 0.9), ("c", 2.0, 7.5))
    cols = np.arange(n) % TS.NX
    want = TS.expected(dspfx, torch_cuda, settings, NF, cols)
    bank = dspfx.ChannelShapers(n, max_frames=TS.NF)
    TS.store(bank, settings)
    check(TS.run(dspfx, torch_cuda, bank, TS.noise_x(NF)[:, cols], n, 0), want, settings, f"shapers N={n}")
    bank.close()


@pytest.mark.parametrize("n,span", SHAPES)
def test_shapers_without_a_heavy_kind(dspfx, torch_cuda, n, span):
    """A, B, C: HardClip, SoftClip and RecipSoftClip, plain arithmetic, so the run takes the light kernel"""
    settings = layout(n, span, ("d", 3.0, 0), ("d", 30.0, 1), ("d", 1.0, 3))
    cols = np.arange(n) % TS.NX
    want = TS.expected(dspfx, torch_cuda, settings, NF, cols)
    bank = dspfx.ChannelShapers(n, max_frames=TS.NF)
    TS.store(bank, settings)
    check(TS.run(dspfx, torch_cuda, bank, TS.noise_x(NF)[:, cols], n, 0), want, settings, f"light shapers N={n}")
    bank.close()


@pytest.mark.parametrize("n,span", SHAPES)
def test_gens(dspfx, torch_cuda, n, span):
    """A: Sine, B: Square, C: Constant, whose wave advances no clock"""
    settings = layout(n, span, (0.5, 100.0, 0), (-1.0, 441.0, 2), (0.25, 12000.0, 3))
    want = TG.expected(dspfx, torch_cuda, settings, (NF,))
    bank = dspfx.ChannelGenerators(n, max_frames=256)
    TG.store(bank, settings)
    check(TG.run(dspfx, torch_cuda, bank, NF), want, settings, f"gens N={n}")
    bank.close()


@pytest.mark.parametrize("n,span", SHAPES)
def test_filters(dspfx, torch_cuda, n, span):
    """A: LowPass, B: Envelope, C: HighPass, in stage 0 on the last lane only; stage 1 has no node behind the four waves"""
    a, b, c = ("lp", 0.93), ("env", 5.0, 64.0), ("hp", 0.05)
    settings = list(zip(layout(n, span, a, b, c), layout(n, span, a, b, None, shift=1)))
    cols = np.arange(n) % TF.NX
    want, _ = TF.expected(dspfx, torch_cuda, settings, NF, cols)
    bank = dspfx.ChannelFilters(n, stages=2, max_frames=TF.NF)
    TF.store(bank, settings)
    check(TF.run(dspfx, torch_cuda, bank, TF.noise_x(NF)[:, cols], n, 0), want, settings, f"filters N={n}")
    bank.close()
