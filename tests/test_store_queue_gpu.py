"""The staged-store queue the three slider banks share (csrc/store_queue.hip.h), driven through each of them: staging buffers of
mixed sizes that are reaped after a run and handed out again, and stores that are still queued when the bank is closed.  Everything
is bit for bit against a twin bank -- both sides run the same kernels, so there is no tolerance."""
import numpy as np
import pytest

import strips_ref as S

pytestmark = pytest.mark.gpu

NF = 128
SHAPES = [(256, 64), (70, 0)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


class MixGroupsCase:
    """faders: 3 channels, all n, 5 channels"""

    def __init__(self, dspfx, n, tile):
        self.dspfx, self.n, self.tile = dspfx, n, tile

    def make(self):
        return self.dspfx.MixGroups(self.n, group_start=[0, self.n // 3, self.n], tile_channels=self.tile, max_frames=NF)

    def stores(self, rng):
        n = self.n
        vals = [rng.uniform(-2.0, 2.0, k).astype(np.float32) for k in (3, n, 5)]
        return [lambda b, v=vals[0]: b.set_gains(v, 1), lambda b, v=vals[1]: b.set_gains(v, 0), lambda b, v=vals[2]: b.set_gains(v, n - 7)]


class StripsCase:
    """a Gain store of 3 levels, a band store of all n channels ([5][n] staged, and the band's state zeroed everywhere, so the
    first bank's earlier run leaves no trace), a Gain store of 5 levels"""

    def __init__(self, dspfx, n, tile):
        self.dspfx, self.n, self.tile = dspfx, n, tile

    def make(self):
        return self.dspfx.ChannelStrips(self.n, bands=1, tile_channels=self.tile, max_frames=NF, link_flags=3)

    def stores(self, rng):
        n = self.n
        g0, g1 = rng.uniform(0.0, 4.0, 3).astype(np.float32), rng.uniform(0.0, 4.0, 5).astype(np.float32)
        raw = S.stable_raw6(rng, n)
        return [lambda b: b.set_gain(g0, 1), lambda b: b.set_band(0, raw, 0), lambda b: b.set_gain(g1, n - 7)]


class MixMatrixCase:
    """two rooms of n // 3 and n - n // 3 members: one row of the small room, every row of the large one, two rows of the small one"""

    def __init__(self, dspfx, n, tile):
        self.dspfx, self.n, self.tile = dspfx, n, tile

    def make(self):
        return self.dspfx.MixMatrix(self.n, group_start=[0, self.n // 3, self.n], tile_channels=self.tile, max_frames=NF)

    def stores(self, rng):
        n0 = self.n // 3
        n1 = self.n - n0
        rows = [rng.uniform(-1.0, 1.0, shape).astype(np.float32) for shape in ((1, n0), (n1, n1), (2, n0))]
        return [lambda b: b.set_rows(rows[0], 1), lambda b: b.set_rows(rows[1], n0), lambda b: b.set_rows(rows[2], n0 - 2)]


CASES = {"mixgroups": MixGroupsCase, "strips": StripsCase, "mixmatrix": MixMatrixCase}


def run(torch, bank, dx):
    out = bank.run(dx, NF)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("n,tile", SHAPES)
@pytest.mark.parametrize("which", sorted(CASES))
def test_buffers_are_reaped_reused_and_freed_from_the_queue(dspfx, torch_cuda, which, n, tile):
    torch = torch_cuda
    case = CASES[which](dspfx, n, tile)
    rng = np.random.default_rng(n + len(which))
    x = [torch.from_numpy(dspfx.to_layout(S.noise(rng, NF, n), tile).reshape(-1).copy()).cuda() for _ in range(2)]
    first, final = case.stores(rng), case.stores(rng)            # small, large, small -- and the same three with new values
    # (every `final` round rewrites all that the round before it and the runs since left behind, a band's state included)

    twin = case.make()
    for st in final:
        st(twin)
    ref = run(torch, twin, x[1])
    twin.close()

    bank = case.make()
    for st in first:
        st(bank)
    run(torch, bank, x[0])
    # a buffer goes back when a later run drains the queue, not at a synchronize: these three are staged in new buffers, and the run
    # that takes them reaps the first three
    for st in final:
        st(bank)
    got = run(torch, bank, x[1])
    assert np.array_equal(got, ref), "a store after a run gives the bits of a first-time store"
    for st in final:
        st(bank)                                                 # served from the spare buffers, first fit
    got = run(torch, bank, x[1])
    assert np.array_equal(got, ref), "stores through reaped and reused staging buffers give the bits of first-time stores"

    first[0](bank)                                               # two stores that no run ever drains: close frees them
    first[1](bank)
    bank.close()
    fresh = case.make()
    for st in final:
        st(fresh)
    again = run(torch, fresh, x[1])
    fresh.close()
    assert np.array_equal(again, ref)
