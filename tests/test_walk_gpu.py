"""The alternating tile walk (DSPFX_WALK, chain_kernels.hip.h work_block): consecutive launches over all channels walk their
tiles in opposite directions, so that a launch starts where the one before it ended and finds those lines in the last-level
cache.  Only the order of the workgroups changes: every output block and every bus is bit for bit what the forward walk
gives, block after block.  Each case builds one engine per setting (the switch is read at setup) in one process."""
import pytest

from chains import chain3, chain5

pytestmark = pytest.mark.gpu
B = 128
BLOCKS = 5
SEED = 0x5EED0021


def _pair(dspfx, monkeypatch, make):
    """[engine with DSPFX_WALK=0, engine with DSPFX_WALK=1], built by make() under that environment"""
    engs = []
    for w in ("0", "1"):
        monkeypatch.setenv("DSPFX_WALK", w)
        engs.append(make())
    assert "every launch front to back" in engs[0].describe(), engs[0].describe()
    assert "alternate" in engs[1].describe(), engs[1].describe()
    return engs


def _same(torch, a, b, what):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what


def _run_blocks(dspfx, torch, engs, N, nf, blocks, call, between=None, first=0):
    """`blocks` blocks of seeded noise through both engines; outputs and buses compared after every block.
    call(eng, x, y, mix, k) runs block k; between(k, engs) runs before block k."""
    x = torch.empty(nf * N, dtype=torch.float32, device="cuda")
    ys = [torch.full((nf * N,), 7.0, dtype=torch.float32, device="cuda") for _ in engs]
    ms = [torch.full((nf,), 7.0, dtype=torch.float32, device="cuda") for _ in engs]
    for k in range(first, first + blocks):
        if between:
            between(k, engs)
        engs[0].fill_noise(x, nf, k * nf, SEED)
        for e, y, m in zip(engs, ys, ms):
            call(e, x, y, m, k)
        torch.cuda.synchronize()
        _same(torch, ys[0], ys[1], ("out", N, nf, k))
        _same(torch, ms[0], ms[1], ("bus", N, nf, k))


def _close(engs):
    for e in engs:
        e.close()


def _kernel(eng):
    return [l for l in eng.describe().splitlines() if l.startswith("stage")][-1]


@pytest.mark.parametrize("tile", [256, 0])
@pytest.mark.parametrize("wgs", [1, 7, 8, 9, 16, 24])
def test_chain5_standard_kernel_workgroup_counts(dspfx, monkeypatch, wgs, tile):
    """512 channels per workgroup (two per lane): workgroup counts off and on the multiple of 8 that turns the XCD remap
    on, one and three tiles per XCD; same-block bus."""
    import torch
    monkeypatch.setenv("DSPFX_VARIANT", "static=1,f=8,cpl=2,ts=0")
    N = 512 * wgs
    engs = _pair(dspfx, monkeypatch, lambda: _chain_engine(dspfx, N, B, tile, chain5(dspfx, 300)))
    assert "s5h_f8_c2" in _kernel(engs[1]) and "time-sliced" not in _kernel(engs[1]), engs[1].describe()
    _run_blocks(dspfx, torch, engs, N, B, BLOCKS, lambda e, x, y, m, k: e.process(x, out=y, mix=m, n_frames=B))
    _close(engs)


def _chain_engine(dspfx, N, nf, tile, chain, link_flags=3):
    e = dspfx.Engine(N, nf, link_flags=link_flags, tile_channels=tile)
    e.set_chain(chain)
    return e


def test_chain5_ragged_tail_beside_a_mirrored_main_launch(dspfx, monkeypatch):
    """512 x 8 + 37 channels (frame-major: a tiled engine is whole tiles): the guarded launch for the channels left over
    runs beside a mirrored main launch; its rows of the bus stay where they were."""
    import torch
    monkeypatch.setenv("DSPFX_VARIANT", "static=1,f=8,cpl=2,ts=0")
    N = 512 * 8 + 37
    for ts_tail in ("0", "1"):              # the interpreter's one-wave launch, and the guarded time-sliced one
        monkeypatch.setenv("DSPFX_TS_TAIL", ts_tail)
        engs = _pair(dspfx, monkeypatch, lambda: _chain_engine(dspfx, N, B, 0, chain5(dspfx, 300)))
        _run_blocks(dspfx, torch, engs, N, B, BLOCKS, lambda e, x, y, m, k: e.process(x, out=y, mix=m, n_frames=B))
        _close(engs)


@pytest.mark.parametrize("wgs", [8, 9, 65])
def test_process_bus_more_and_fewer_rows_than_slices(dspfx, monkeypatch, wgs):
    """dspfx_process_bus with the Output hop: more and fewer rows than the bus' 64 slices; the last ticket is drawn by a
    different workgroup in the mirrored walk, the sums and their order are the same."""
    import torch
    monkeypatch.setenv("DSPFX_VARIANT", "static=1,f=8,cpl=2,ts=0")
    N = 512 * wgs
    engs = _pair(dspfx, monkeypatch, lambda: _chain_engine(dspfx, N, B, 256, chain5(dspfx, 300)))
    _run_blocks(dspfx, torch, engs, N, B, BLOCKS, lambda e, x, y, m, k: e.process_bus(x, y, m, B, n_connected=N))
    _close(engs)


def test_mixpipe_rows_of_launches_in_opposite_directions(dspfx, monkeypatch):
    """dspfx_process_mixpipe: the rows of two earlier launches, written in opposite directions, are reduced in the first
    workgroups of a later one; then the flush."""
    import torch
    monkeypatch.setenv("DSPFX_VARIANT", "static=1,f=8,cpl=2,ts=0")
    N = 512 * 8
    engs = _pair(dspfx, monkeypatch, lambda: _chain_engine(dspfx, N, B, 256, chain5(dspfx, 300)))
    _run_blocks(dspfx, torch, engs, N, B, BLOCKS + 1, lambda e, x, y, m, k: e.process_mixpipe(x, y, m if k >= 2 else None, B))
    older = [torch.zeros(B, device="cuda") for _ in engs]
    newer = [torch.zeros(B, device="cuda") for _ in engs]
    for e, o, n in zip(engs, older, newer):
        e.mixpipe_flush(o, n)
    torch.cuda.synchronize()
    _same(torch, older[0], older[1], "flush, older")
    _same(torch, newer[0], newer[1], "flush, newer")
    # 72 x 512 channels: more workgroups than slices, so the earlier blocks' stages ride in this launch's first workgroups
    _close(engs)
    N = 512 * 72
    engs = _pair(dspfx, monkeypatch, lambda: _chain_engine(dspfx, N, B, 256, chain5(dspfx, 300)))
    _run_blocks(dspfx, torch, engs, N, B, BLOCKS + 1, lambda e, x, y, m, k: e.process_mixpipe(x, y, m if k >= 2 else None, B))
    _close(engs)


@pytest.mark.parametrize("nf", [192, 256])
def test_two_launches_per_call(dspfx, monkeypatch, nf):
    """A 128-sample delay line cuts a call of 192 / 256 frames into two launches (two bus segments per call): the parity
    advances per launch, not per call."""
    import torch
    monkeypatch.setenv("DSPFX_VARIANT", "static=1,f=8,cpl=2,ts=0")
    N = 512 * 8
    engs = _pair(dspfx, monkeypatch, lambda: _chain_engine(dspfx, N, nf, 256, chain5(dspfx, 128)))
    _run_blocks(dspfx, torch, engs, N, nf, BLOCKS, lambda e, x, y, m, k: e.process(x, out=y, mix=m, n_frames=nf))
    _close(engs)


@pytest.mark.parametrize("N", [8192, 8192 + 37])
def test_time_sliced_kernel_and_its_guarded_tail(dspfx, monkeypatch, N):
    """gain > biquad > reverb at few channels: chain_ts_kernel takes its channel groups from work_block() as well, but the
    engine keeps its launches on the forward walk (nothing of theirs stays in the cache, and mirrored they ran slower); the
    parity still advances, and the guarded launch beside it stays where it was."""
    import torch
    engs = _pair(dspfx, monkeypatch, lambda: _chain_engine(dspfx, N, B, 0, chain3(dspfx, 300)))
    assert "time-sliced" in _kernel(engs[1]), engs[1].describe()
    _run_blocks(dspfx, torch, engs, N, B, BLOCKS, lambda e, x, y, m, k: e.process(x, out=y, mix=m, n_frames=B))
    _close(engs)


def test_interpreter_then_run_time_kernel(dspfx, monkeypatch, tmp_path):
    """A chain the library has no compiled-in kernel for starts on the interpreter (chain_dyn_kernel) and adopts its
    run-time kernel at a block boundary: the parity is the engine's, not the kernel's, and carries over."""
    import torch
    monkeypatch.setenv("DSPFX_CACHE_DIR", str(tmp_path))          # an empty cache: the shape has to be compiled
    N, nf = 512 * 8, 96                                           # 96-frame blocks: the standard kernels, never the time-sliced one
    chain = [dspfx.Gain(0.7), dspfx.LowPass(0.3), dspfx.Reverb(delay_samples=200, decay=0.4), dspfx.HighPass(0.2)]
    engs = _pair(dspfx, monkeypatch, lambda: _chain_engine(dspfx, N, nf, 256, chain))
    call = lambda e, x, y, m, k: e.process(x, out=y, mix=m, n_frames=nf)
    _run_blocks(dspfx, torch, engs, N, nf, 3, call)                # an odd number: the parities are 1 at the switch

    def adopt(k, es):
        if k == 3:
            for e in es:
                assert e.kernels_ready(120000), e.describe()
            assert "jit_" in _kernel(es[1]), es[1].describe()
    _run_blocks(dspfx, torch, engs, N, nf, 4, call, between=adopt, first=3)
    _close(engs)


def test_graph_kernel(dspfx, monkeypatch):
    """A three-node DAG through dspfx_graph_set: graph_kernel takes its tiles from the same function."""
    import torch
    E = dspfx
    N, M = 512 * 8, dspfx.PORT_MAIN
    nodes = [E.Gain(0.8), E.BiQuad(), E.LowPass(0.3)]
    links = [(E.GRAPH_INPUT, 0, M), (0, 1, M), (0, 2, M), (1, 3, M), (2, 3, M)]

    def make():
        e = E.Engine(N, B, link_flags=3, tile_channels=256)
        e.set_graph(nodes, links)
        return e
    engs = _pair(dspfx, monkeypatch, make)
    _run_blocks(dspfx, torch, engs, N, B, BLOCKS, lambda e, x, y, m, k: e.process(x, out=y, mix=m, n_frames=B))
    _close(engs)


def test_parity_survives_reset_slider_store_and_placement_tuning(dspfx, monkeypatch):
    """dspfx_reset, a Reverb slider store (a new zero ring) and dspfx_tune_placement between blocks 2 and 3: whatever they
    do to the engine, the next launches' directions stay defined and the results equal the forward walk's."""
    import torch
    monkeypatch.setenv("DSPFX_TUNE_FAKE_SLOW", "2")               # the tuner re-places groups only where it finds a slow one
    N = 131072                                                    # 64 MiB ring groups: the tuner engages
    for what in ("reset", "store", "tune"):
        engs = _pair(dspfx, monkeypatch, lambda: _chain_engine(dspfx, N, B, 256, chain5(dspfx, 300)))
        scratch = torch.empty(B * N, dtype=torch.float32, device="cuda")
        probe_in = torch.zeros(B * N, dtype=torch.float32, device="cuda")

        def between(k, es):
            if k != 3:
                return
            for e in es:
                if what == "reset":
                    e.reset()
                elif what == "store":
                    e.set_param(2, 0, 0.4)
                else:
                    e.tune_placement(probe_in, scratch, B)
        _run_blocks(dspfx, torch, engs, N, B, 6, lambda e, x, y, m, k: e.process(x, out=y, mix=m, n_frames=B), between=between)
        _close(engs)
