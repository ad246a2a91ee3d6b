"""Structure of the alternating tile walk (no device needed): the switches are setup-time switches, the direction travels in the
call, and every kernel takes its tile from the one function that mirrors it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dsp-stuff_amd", "csrc")


def _code(name):
    """the file without // comments"""
    return "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, name), errors="ignore").read().splitlines())


def _struct(src, head):
    start = src.index(head)
    depth = 0
    for end in range(start, len(src)):
        depth += {"{": 1, "}": -1}.get(src[end], 0)
        if depth == 0 and src[end] == "}":
            return src[start:end]
    raise AssertionError(head)


def test_the_walk_switches_are_read_at_setup_only():
    """DSPFX_WALK and DSPFX_WALK_ZONE_MIB live in EnvSwitches and are named in read_env_switches() alone: the per-block path
    reads the engine's snapshot."""
    env = _struct(_code("engine.h"), "struct EnvSwitches {")
    assert re.search(r"\bint walk\b", env) and re.search(r"\bint walk_zone_mib\b", env), env
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h")):
            continue
        src = _code(name)
        if name == "plan.hip":
            body = src[src.index("EnvSwitches read_env_switches()"):]
            body = body[:body.index("\n}\n")]
            assert '"DSPFX_WALK"' in body and '"DSPFX_WALK_ZONE_MIB"' in body
            assert src.count('"DSPFX_WALK') == body.count('"DSPFX_WALK'), "plan.hip names the switch outside read_env_switches()"
        else:
            assert '"DSPFX_WALK' not in src, f"{name} names DSPFX_WALK: switches are read in read_env_switches() only"
    run = _code("dspfx.hip")
    assert "walk_alternates(e)" in run and "e->walk_parity" in run


def test_the_direction_travels_in_the_call_and_the_parity_in_the_engine():
    hdr = _code("engine.h")
    assert re.search(r"\bbool walk_rev\b", _struct(hdr, "struct BlockCall {"))
    assert re.search(r"\bwalk_parity\b", _struct(hdr, "struct dspfx_engine {"))
    # window launches of the host path and the placement probe build their own BlockCall and never touch the parity
    for name in ("host_pipe.hip", "placement.hip"):
        assert "walk_parity" not in _code(name) and "walk_rev" not in _code(name), name


def test_every_kernel_takes_its_tile_from_work_block():
    """chain_kernel, chain_dyn_kernel, chain_ts_kernel, graph_kernel, the bus epilogue and the bus tail: each call of
    work_block() passes the launch's direction, and nothing else turns blockIdx.x into a tile."""
    for name in ("chain_kernels.hip.h", "graph_kernel.hip.h"):
        src = _code(name)
        calls = re.findall(r"work_block\(([^)]*)\)", src)
        uses = [c for c in calls if not c.startswith("int ")]
        assert uses, name
        for c in uses:
            assert c.replace(" ", "") == "a.xcd_remap,a.walk_rev", (name, c)
    src = _code("chain_kernels.hip.h")
    assert len(re.findall(r"work_block\(a\.xcd_remap, a\.walk_rev\)", src)) >= 5
    # blockIdx.x by itself: the mirrored index, the earlier blocks' bus stages (first workgroups of a launch), the one-wave
    # guarded launches (which are never mirrored), and the workgroups at the two ends of a launch in dispatch order
    for ln in src.splitlines():
        if "blockIdx.x" in ln:
            assert any(k in ln for k in ("const unsigned b = blockIdx.x", "blockDim.x == WG ? work_block", "blockIdx.x < zone")), ln
