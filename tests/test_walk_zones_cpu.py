"""The switches of the cached output zones (no device needed): DSPFX_WALK_HEAD and DSPFX_WALK_TAIL_MIB are setup-time switches
like DSPFX_WALK itself -- fields of EnvSwitches, named in read_env_switches() alone -- and the zone widths travel in ChainArgs."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dsp-stuff_amd", "csrc")


def _code(name):
    """the file without // comments"""
    return "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, name), errors="ignore").read().splitlines())


def _block(src, head):
    start = src.index(head)
    depth = 0
    for end in range(start, len(src)):
        depth += {"{": 1, "}": -1}.get(src[end], 0)
        if depth == 0 and src[end] == "}":
            return src[start:end]
    raise AssertionError(head)


def test_the_zone_switches_are_fields_of_env_switches():
    env = _block(_code("engine.h"), "struct EnvSwitches {")
    assert re.search(r"\bint walk_head\b", env) and re.search(r"\bint walk_tail_mib\b", env), env


def test_plan_names_the_zone_switches_in_read_env_switches_only():
    src = _code("plan.hip")
    body = _block(src, "EnvSwitches read_env_switches()")
    for name in ('"DSPFX_WALK_HEAD"', '"DSPFX_WALK_TAIL_MIB"'):
        assert body.count(name) == 1, name
        assert src.count(name) == 1, f"plan.hip names {name} outside read_env_switches()"
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")) and name != "plan.hip":
            assert "DSPFX_WALK_HEAD" not in _code(name) and "DSPFX_WALK_TAIL_MIB" not in _code(name), name


def test_both_zone_widths_travel_in_chain_args():
    args = _block(_code("chain_kernels.hip.h"), "struct ChainArgs {")
    assert re.search(r"\bunsigned walk_zone\b", args) and re.search(r"\bunsigned walk_tail\b", args), args
    assert "walk_cached_out(a.walk_zone, a.walk_tail)" in _code("chain_kernels.hip.h")
