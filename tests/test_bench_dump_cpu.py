"""bench.py --dump-outputs without a GPU: dump_outputs() turns the engine-layout output buffer into [frames][channels] as
pkg.from_layout does, for every channel when they fit its share of the 64 MB a dump may take, else for a fixed seeded sample."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def _buffer(dspfx, N, B, tile):
    """An engine-layout buffer whose every sample names its own (frame, channel): frame * N + channel, exact in f32."""
    import torch
    fm = (np.arange(B)[:, None] * N + np.arange(N)[None, :]).astype(np.float32)
    return fm, torch.from_numpy(dspfx.to_layout(fm, tile).reshape(-1).copy())


@pytest.mark.parametrize("tile", [0, 256])
def test_every_channel_when_it_fits(tmp_path, bench, dspfx, tile):
    import torch
    N, B = 4096, 128
    fm, y = _buffer(dspfx, N, B, tile)
    mix = torch.arange(B, dtype=torch.float32)
    bench.dump_outputs(torch, str(tmp_path), y, mix, N, B, tile, 1, 0)
    assert sorted(os.listdir(tmp_path)) == ["mix.npy", "out.npy"]
    out = np.load(tmp_path / "out.npy")
    assert out.dtype == np.float32 and np.array_equal(out, fm)
    assert np.array_equal(np.load(tmp_path / "mix.npy"), mix.numpy())


@pytest.mark.parametrize("tile", [0, 256])
def test_a_fixed_sample_of_channels_when_it_does_not(tmp_path, bench, dspfx, monkeypatch, tile):
    import torch
    N, B = 8192, 128
    monkeypatch.setattr(bench, "DUMP_OUT_BYTES", 4 * B * 1000)           # room for 1000 channels
    fm, y = _buffer(dspfx, N, B, tile)
    outs = []
    for run in range(2):
        d = tmp_path / str(run)
        bench.dump_outputs(torch, str(d), y, None, N, B, tile, 1, 0)
        assert os.listdir(d) == ["out.npy"]
        outs.append(np.load(d / "out.npy"))
    assert np.array_equal(outs[0], outs[1]) and outs[0].shape == (B, 1000)
    ch = outs[0][0].astype(np.int64)                                       # frame 0 holds the channel numbers
    assert np.all(np.diff(ch) > 0) and ch[-1] < N and np.array_equal(outs[0], fm[:, ch])


def test_ranks_share_the_budget_and_name_their_files(tmp_path, bench, dspfx):
    import torch
    N, B = 1 << 16, 128
    fm, y = _buffer(dspfx, N, B, 256)
    for r in range(2):
        bench.dump_outputs(torch, str(tmp_path), y, torch.zeros(B), N, B, 256, 2, r)
    assert sorted(os.listdir(tmp_path)) == ["mix_rank0.npy", "mix_rank1.npy", "out_rank0.npy", "out_rank1.npy"]
    total = sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path))
    assert total <= 64 << 20 and np.load(tmp_path / "out_rank0.npy").shape == (B, (bench.DUMP_OUT_BYTES // 2) // (4 * B))
