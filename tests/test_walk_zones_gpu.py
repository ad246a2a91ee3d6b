"""The cached output zones of the alternating tile walk (chain_kernels.hip.h walk_cached_out; DSPFX_WALK_ZONE_MIB,
DSPFX_WALK_TAIL_MIB, DSPFX_WALK_HEAD): the last workgroups of a launch -- the tail zone -- store their output rows on the
default cache policy, the first ones -- the head zone -- on the default policy or with the hint, everything between with the
hint.  Only the cache policy of stores changes: every output block and every bus is bit for bit what the forward walk gives.
At two channels per lane and 128 frames a workgroup writes 256 KiB of output rows, so 1 MiB of zone is 4 workgroups; the shapes
are the smallest at which each zone geometry exists."""
import pytest

from chains import chain5

pytestmark = pytest.mark.gpu
B = 128
BLOCKS = 5
SEED = 0x5EED0031
HEAD_POLICIES = ["0", "1"]          # DSPFX_WALK_HEAD: default-policy stores, stores with the nontemporal hint

# (channels, tile width, DSPFX_WALK_ZONE_MIB, DSPFX_WALK_TAIL_MIB or None)
GEOMETRIES = {
    "disjoint_with_a_middle_remap_on": (512 * 24, 256, "1", None),
    "disjoint_with_a_middle_remap_off": (512 * 25, 256, "1", None),
    "exactly_meeting": (512 * 8, 256, "1", None),
    "overlapping_9_workgroups": (512 * 9, 256, "2", None),
    "overlapping_3_workgroups": (512 * 3, 256, "1", None),
    "head_1_mib_tail_3_mib": (512 * 24, 256, "1", "3"),
    "ragged_tail_beside_the_main_launch": (512 * 8 + 37, 0, "1", None),
}


def _same(torch, a, b, what):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what


def _pair(dspfx, monkeypatch, N, nf, tile, chain, zone, tail, head):
    """[engine with DSPFX_WALK=0, engine with the walk on], both built under the zone switches being tested"""
    monkeypatch.setenv("DSPFX_VARIANT", "static=1,f=8,cpl=2,ts=0")
    monkeypatch.setenv("DSPFX_WALK_ZONE_MIB", zone)
    monkeypatch.setenv("DSPFX_WALK_HEAD", head)
    if tail is None:
        monkeypatch.delenv("DSPFX_WALK_TAIL_MIB", raising=False)
    else:
        monkeypatch.setenv("DSPFX_WALK_TAIL_MIB", tail)
    engs = []
    for w in ("0", "1"):
        monkeypatch.setenv("DSPFX_WALK", w)
        e = dspfx.Engine(N, nf, link_flags=3, tile_channels=tile)
        e.set_chain(chain)
        engs.append(e)
    assert "every launch front to back" in engs[0].describe(), engs[0].describe()
    assert "alternate" in engs[1].describe(), engs[1].describe()
    stage = [l for l in engs[1].describe().splitlines() if l.startswith("stage")][-1]
    assert "time-sliced" not in stage.split(";")[0], engs[1].describe()
    if N % 512 == 0:        # (an odd frame-major row length leaves one channel per lane: no zones, the ragged launch beside it)
        assert "s5h_f8_c2" in stage, engs[1].describe()
    return engs


def _run_blocks(torch, engs, N, nf, call):
    x = torch.empty(nf * N, dtype=torch.float32, device="cuda")
    ys = [torch.full((nf * N,), 7.0, dtype=torch.float32, device="cuda") for _ in engs]
    ms = [torch.full((nf,), 7.0, dtype=torch.float32, device="cuda") for _ in engs]
    for k in range(BLOCKS):
        engs[0].fill_noise(x, nf, k * nf, SEED)
        for e, y, m in zip(engs, ys, ms):
            call(e, x, y, m)
        torch.cuda.synchronize()
        _same(torch, ys[0], ys[1], ("out", N, nf, k))
        _same(torch, ms[0], ms[1], ("bus", N, nf, k))
    for e in engs:
        e.close()


@pytest.mark.parametrize("head", HEAD_POLICIES)
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_zone_geometries_through_process_and_process_bus(dspfx, monkeypatch, geometry, head):
    import torch
    N, tile, zone, tail = GEOMETRIES[geometry]
    engs = _pair(dspfx, monkeypatch, N, B, tile, chain5(dspfx, 300), zone, tail, head)
    _run_blocks(torch, engs, N, B, lambda e, x, y, m: e.process(x, out=y, mix=m, n_frames=B))
    engs = _pair(dspfx, monkeypatch, N, B, tile, chain5(dspfx, 300), zone, tail, head)
    _run_blocks(torch, engs, N, B, lambda e, x, y, m: e.process_bus(x, y, m, B, n_connected=N))


@pytest.mark.parametrize("head", HEAD_POLICIES)
def test_two_launches_per_call(dspfx, monkeypatch, head):
    """A 128-sample delay line cuts a call of 256 frames into two launches: the parity, and with it which rows the head zone
    finds resident, advances per launch."""
    import torch
    N, nf = 512 * 24, 256
    engs = _pair(dspfx, monkeypatch, N, nf, 256, chain5(dspfx, 128), "1", None, head)
    _run_blocks(torch, engs, N, nf, lambda e, x, y, m: e.process(x, out=y, mix=m, n_frames=nf))


@pytest.mark.parametrize("head,policy", [("0", "default-policy stores"), ("1", "nontemporal hint")])
def test_describe_names_the_head_policy_and_both_sizes(dspfx, monkeypatch, head, policy):
    monkeypatch.setenv("DSPFX_WALK", "1")
    monkeypatch.setenv("DSPFX_WALK_HEAD", head)
    monkeypatch.setenv("DSPFX_WALK_ZONE_MIB", "5")
    monkeypatch.setenv("DSPFX_WALK_TAIL_MIB", "7")
    e = dspfx.Engine(512 * 8, B, link_flags=3, tile_channels=256)
    e.set_chain(chain5(dspfx, 300))
    walk = [l for l in e.describe().splitlines() if l.startswith("tile walk")]
    e.close()
    assert len(walk) == 1 and "alternate" in walk[0], walk
    assert "last 7 MiB" in walk[0] and "head zone: 5 MiB" in walk[0] and policy in walk[0], walk
    # DSPFX_WALK_ZONE_MIB alone keeps its meaning: it sets both sizes
    monkeypatch.delenv("DSPFX_WALK_TAIL_MIB")
    e = dspfx.Engine(512 * 8, B, link_flags=3, tile_channels=256)
    e.set_chain(chain5(dspfx, 300))
    walk = [l for l in e.describe().splitlines() if l.startswith("tile walk")]
    e.close()
    assert "last 5 MiB" in walk[0] and "head zone: 5 MiB" in walk[0], walk
