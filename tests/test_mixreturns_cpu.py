"""The mix-group bank's per-channel returns (dspfx_mixgroups_returns), the parts that need no GPU: the entry point in the
library and in its Python, C++ and Rust mirrors, and the definition (mixreturns_ref.returns_bits: room sum minus the own term)
inside its bound against the float64 sum of the others, beside the reference taken literally (collect_and_average over the
other n - 1 pipes)."""
import os
import re

import numpy as np
import pytest

import mixreturns_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
HPP = open(os.path.join(ROOT, "include", "dspfx.hpp")).read()
FFI = open(os.path.join(ROOT, "host", "rust", "src", "ffi.rs")).read()
RS = open(os.path.join(ROOT, "host", "rust", "src", "mix_groups.rs")).read()
SYM = "dspfx_mixgroups_returns"


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


# ---- the ABI and its mirrors -------------------------------------------------------------------------------------------------

def test_symbol_is_exported_and_built(dspfx):
    assert SYM in dspfx.EXPORTS
    fn = getattr(dspfx.lib(), SYM)
    assert len(fn.argtypes) == 6
    assert callable(getattr(dspfx.MixGroups, "returns"))


def test_declared_with_six_arguments_and_mirrored():
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % SYM, _strip_comments(HDR))
    assert m, "not declared in dspfx.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 6, args
    assert [a.split()[-1].lstrip("*") for a in args] == ["m", "block", "n_frames", "buses", "returns", "stream"]
    r = re.search(r"pub fn %s\s*\(([^)]*)\)\s*->\s*c_int\s*;" % SYM, FFI)
    assert r, "not bound in ffi.rs"
    assert len([a for a in r.group(1).split(",") if a.strip()]) == 6
    assert SYM in _strip_comments(HPP), "no C++ mirror"
    assert SYM in RS and re.search(r"pub unsafe fn returns\s*\(", RS), "no safe wrapper in mix_groups.rs"


def test_abi_version_stays_2(dspfx):
    assert re.search(r"#define\s+DSPFX_ABI_VERSION\s+2u?\b", HDR)
    assert dspfx.ABI_VERSION == 2 and dspfx.lib().dspfx_abi_version() == 2


# ---- the definition against the float64 sum of the others --------------------------------------------------------------------

def _data(family, nf, n, rng):
    if family == "noise":
        return rng.uniform(-1.0, 1.0, (nf, n)).astype(np.float32)
    noise = np.float32(1e-3) * rng.standard_normal((nf, n)).astype(np.float32)
    if family == "dc_heavy":
        return (np.float32(0.9) + noise).astype(np.float32)
    x = noise.astype(np.float32)                  # "dominant": one channel at 0.99 among 1e-3 noise, the cancellation case
    x[:, n // 3] = np.float32(0.99)
    return x


def _sequential_sum(t):
    """[F][n] f32 -> [F] f32, the terms added one after the other from the first: n - 1 dependent additions"""
    s = t[:, 0].copy()
    for c in range(1, t.shape[1]):
        s = (s + t[:, c]).astype(np.float32)
    return s


@pytest.mark.parametrize("with_gain", [False, True], ids=["nogain", "gain"])
@pytest.mark.parametrize("family", ["noise", "dc_heavy", "dominant"])
@pytest.mark.parametrize("n", [2, 3, 64, 256, 1000])
def test_definition_and_literal_reference_stay_inside_the_bound(n, family, with_gain):
    nf = 16
    rng = np.random.default_rng(1000 * n + len(family))
    x = _data(family, nf, n, rng)
    gain = rng.uniform(0.0, 10.0, n).astype(np.float32) if with_gain else None
    table = [0, n]
    ref, sabs = M.returns_exact(x, table, gain)
    t = M.terms(x, gain)
    # brute force on the first frame: the restatement's prefix sums are the sum of the others
    div = float(M.link_divisor(n - 1))
    for c in (0, n // 3, n - 1):
        others = np.delete(t[0].astype(np.float64), c).sum() / div
        assert abs(ref[0, c] - others) <= 1e-12 * max(1.0, sabs[0, c])
    depth = n - 1
    S = _sequential_sum(t)[:, None]
    got = M.returns_bits(S, x, table, gain).astype(np.float64)
    bnd = M.bound(sabs, ref, depth + 1)
    worst = float((np.abs(got - ref) / bnd).max())
    assert (np.abs(got - ref) <= bnd).all(), worst
    lit = M.collect_and_average(t[:, 1:].T).astype(np.float64)        # channel 0's Output node: the other n - 1 pipes
    bl = M.bound(sabs[:, 0], ref[:, 0], n - 1)
    worst_lit = float((np.abs(lit - ref[:, 0]) / bl).max())
    print(f"n {n} {family} gain {with_gain}: definition err / bound {worst:.3f}, literal reference {worst_lit:.3f}")
    assert (np.abs(lit - ref[:, 0]) <= bl).all(), worst_lit


def test_restatement_bookkeeping():
    x = np.arange(1, 13, dtype=np.float32).reshape(2, 6)
    table = [0, 3, 3, 4, 6]                        # a group of three, an empty one, a group of one, a group of two
    ref, sabs = M.returns_exact(x, table, normalise=False)
    assert np.array_equal(ref, [[5, 4, 3, 0, 6, 5], [17, 16, 15, 0, 12, 11]])
    assert np.array_equal(sabs, [[6, 6, 6, 0, 11, 11], [24, 24, 24, 0, 23, 23]])
    assert np.array_equal(M.group_of(table, 6), [0, 0, 0, 2, 3, 3])
    S = np.asarray([[6, 0, 4, 11], [24, 0, 10, 23]], np.float32)
    assert np.array_equal(M.returns_bits(S, x, table, normalise=False), ref.astype(np.float32))
    d = M.returns_divisors(table)
    assert d[0] == M.link_divisor(2) and d[3] == M.link_divisor(1) and d[1] == 1.0 and d[2] == 1.0
    got = M.returns_bits(S, x, table)
    assert np.array_equal(got[:, :3], (ref[:, :3].astype(np.float32) / d[0]).astype(np.float32))
    xn = x.copy()
    xn[0, 3] = np.nan                              # a group of one: +0.0 whatever the sample is
    assert (M.returns_bits(S, xn, table).view(np.uint32)[:, 3] == 0).all()
