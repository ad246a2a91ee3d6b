"""The mix-group bank, the parts that need no GPU: the restatement in mixgroups_ref.py against a literal sequential-f32
collect_and_average, dspfx_mixgroups_plan (a pure host function) on good and bad tables, the depth it reports against the cap
64 + ceil(log2 n), and the ABI and its Python, C++ and Rust mirrors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mixgroups_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
HPP = open(os.path.join(ROOT, "include", "dspfx.hpp")).read()
FFI = open(os.path.join(ROOT, "host", "rust", "src", "ffi.rs")).read()
NEW = {"dspfx_mixgroups_create": 2, "dspfx_mixgroups_destroy": 1, "dspfx_mixgroups_last_error": 1, "dspfx_mixgroups_run": 5,
       "dspfx_mixgroups_set_gains": 4, "dspfx_mixgroups_plan": 5}
FIELDS = [("uint32_t", "abi_version"), ("int32_t", "device"), ("uint32_t", "n_channels"), ("uint32_t", "max_frames"),
          ("uint32_t", "tile_channels"), ("uint32_t", "n_groups"), ("uint32_t", "normalise"), ("const uint64_t *", "group_start")]
CTYPE = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "const uint64_t *": C.POINTER(C.c_uint64)}
RUST = {"uint32_t": "u32", "int32_t": "i32", "const uint64_t *": "*const u64"}
INVALID = -1


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


# ---- the restatement ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 7, 16, 61])
@pytest.mark.parametrize("with_gain", [False, True])
def test_restatement_against_sequential_collect_and_average(n, with_gain):
    """A Gain node per channel in front of an Output node with n pipes, evaluated as the reference does (f32, one after the
    other), is within bound(n, n - 1) of the restatement: a sequential sum is a chain of n - 1 ... n additions from 0.0."""
    rng = np.random.default_rng(100 + n)
    x = rng.uniform(-1.0, 1.0, (37, n)).astype(np.float32)
    x[:, 0] += np.float32(0.9)                                    # a DC-heavy pipe
    gain = rng.uniform(0.0, 10.0, n).astype(np.float32) if with_gain else None
    pipes = R.terms(x, gain).T                                    # [n][F]: what each Gain node hands on, x * level in f32
    lit = R.collect_and_average(pipes).astype(np.float64)
    ref, sabs, div = R.buses(x, [0, n], gain)
    assert div[0] == float(R.link_divisor(n))
    err = np.abs(lit - ref[:, 0])
    assert (err <= R.bound(sabs[:, 0], ref[:, 0], n - 1)).all(), (n, err.max())


def test_restatement_bookkeeping():
    x = np.arange(24, dtype=np.float32).reshape(2, 12)
    ref, sabs, div = R.buses(x, [0, 3, 3, 12], normalise=False)
    assert np.array_equal(ref, [[3.0, 0.0, 63.0], [39.0, 0.0, 171.0]]) and np.array_equal(div, [1.0, 1.0, 1.0])
    assert np.array_equal(sabs, ref)
    ref, _, div = R.buses(x, [0, 3, 3, 12], gain=np.full(12, 2.0, np.float32), groups=[2])
    assert div[0] == float(R.link_divisor(9)) and ref.shape == (2, 1) and ref[0, 0] == 126.0 / div[0]
    assert R.cap(1) == 64 and R.cap(2) == 65 and R.cap(3) == 66 and R.cap(256) == 72 and R.cap(257) == 73 and R.cap(0) == 64
    t = R.ragged_table(1 << 20, 7, 1 << 18)
    assert t[0] == 0 and t[-1] == 1 << 20 and (np.diff(t.astype(np.int64)) >= 1).all()
    assert np.array_equal(t, R.ragged_table(1 << 20, 7, 1 << 18))


def test_link_divisor_is_the_librarys(dspfx):
    for n in (0, 1, 2, 255, 256, 1000, 65536):
        assert R.link_divisor(n) == dspfx.link_divisor(n), n


# ---- dspfx_mixgroups_plan ----------------------------------------------------------------------------------------------------

def _good_tables():
    n = 4096
    return {
        "uniform": (n, np.arange(0, n + 1, 256), 256),
        "ragged": (n, [0, 1, 2, 70, 100, 700, 701, 2000, 4095, n], 0),
        "empty groups": (n, [0, 0, 100, 100, 100, 3000, n, n], 64),
        "one group of N": (n, [0, n], 256),
        "N groups of 1": (n, np.arange(n + 1), 0),
        "odd N": (1000, [0, 333, 1000], 0),
    }


@pytest.mark.parametrize("name", list(_good_tables()))
def test_plan_accepts_good_tables(dspfx, name):
    n, table, tile = _good_tables()[name]
    depth = dspfx.mixgroups_plan(n, group_start=table, tile_channels=tile)
    sizes = np.diff(np.asarray(table, np.int64))
    assert depth.dtype == np.uint32 and depth.shape == sizes.shape
    for d, s in zip(depth, sizes):
        assert d <= R.cap(s), (name, s, d)
        assert d >= (int(s) - 1).bit_length() if s > 0 else d == 0, (name, s, d)     # no tree over s terms is shallower
    assert dspfx.lib().dspfx_mixgroups_last_error(None) == b""


def test_plan_depends_on_the_group_alone(dspfx):
    """A group's depth (its summation tree) follows from its own start and length, not from its neighbours."""
    n = 1 << 16
    a = dspfx.mixgroups_plan(n, group_start=[0, 1000, 5000, n])
    b = dspfx.mixgroups_plan(n, group_start=[0, 10, 20, 999, 1000, 5000, 5001, 60000, n])
    assert a[1] == b[4]


@pytest.mark.parametrize("table,n,tile,word", [
    ([0, 5, 4, 10], 10, 0, "decreases"),
    ([1, 5, 10], 10, 0, "group_start[0]"),
    ([0, 5, 9], 10, 0, "n_channels"),
    ([0, 500, 1000], 1000, 64, "tile_channels"),
    ([0, 500, 1000], 1000, 24, "tile_channels"),
])
def test_plan_rejects_bad_tables_with_a_reason(dspfx, table, n, tile, word):
    L = dspfx.lib()
    t = np.asarray(table, np.uint64)
    rc = L.dspfx_mixgroups_plan(t.ctypes.data_as(C.POINTER(C.c_uint64)), len(t) - 1, n, tile, None)
    assert rc == INVALID
    msg = L.dspfx_mixgroups_last_error(None).decode()
    assert word in msg, msg
    with pytest.raises(dspfx.DspfxError) as ei:
        dspfx.mixgroups_plan(n, group_start=table, tile_channels=tile)
    assert ei.value.status == INVALID and word in str(ei.value)
    assert L.dspfx_mixgroups_plan(None, 1, 10, 0, None) == INVALID
    assert L.dspfx_mixgroups_plan(t.ctypes.data_as(C.POINTER(C.c_uint64)), 0, n, tile, None) == INVALID


def test_depth_is_under_the_cap_for_sizes_1_to_2_pow_24(dspfx):
    """One group of n channels from channel 0, and the same group behind an odd offset (so that it starts and ends inside
    spans): every power of two, its neighbours, and a log-uniform sample."""
    rng = np.random.default_rng(5)
    sizes = {1 << k for k in range(25)} | {(1 << k) + 1 for k in range(24)} | {(1 << k) - 1 for k in range(1, 25)}
    sizes |= {int(v) for v in np.exp(rng.uniform(0.0, np.log(2.0 ** 24), 400))}
    worst = 0
    for n in sorted(sizes):
        assert 1 <= n <= 1 << 24
        d0 = int(dspfx.mixgroups_plan(n, group_start=[0, n])[0])
        d1 = int(dspfx.mixgroups_plan(n + 357, group_start=[0, 101, 101 + n, n + 357])[1])
        for d in (d0, d1):
            assert (n - 1).bit_length() <= d <= R.cap(n), (n, d, R.cap(n))
        worst = max(worst, d0, d1)
    assert worst <= 64                 # the design: far below 64 + log2 n at every size


# ---- the ABI and its mirrors --------------------------------------------------------------------------------------------------

def _header_desc_fields():
    m = re.search(r"typedef struct dspfx_mixgroups_desc\s*\{(.*?)\}\s*dspfx_mixgroups_desc;", _strip_comments(HDR), re.S)
    assert m
    out = []
    for d in m.group(1).split(";"):
        if d.strip():
            t, name = re.match(r"\s*(.*?)(\w+)\s*$", d, re.S).groups()
            out.append((" ".join(t.split()), name))
    return out


def test_entry_points_declared_listed_and_exported(dspfx):
    protos = {m.group(1): len(m.group(2).split(","))
              for m in re.finditer(r"\b(dspfx_\w+)\s*\(([^;{}]*?)\)\s*;", _strip_comments(HDR))}
    for name, arity in NEW.items():
        assert protos.get(name) == arity, name
        assert name in dspfx.EXPORTS, name
    L = C.CDLL(dspfx.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
    section = HDR[HDR.index("mix groups: one Output bus per channel range"):]
    assert "64 + ceil(log2(max(n, 1)))" in section and "no atomics" in section
    assert re.search(r"#define DSPFX_ABI_VERSION\s+2\b", HDR) and dspfx.ABI_VERSION == 2


def test_mirrors_name_every_new_symbol(dspfx):
    fields = _header_desc_fields()
    assert fields == FIELDS
    py = dspfx._MixGroupsDesc._fields_
    assert [f[0] for f in py] == [name for _, name in fields]
    assert [t for _, t in py] == [CTYPE[t] for t, _ in fields]
    assert C.sizeof(dspfx._MixGroupsDesc) == 40 and dspfx._MixGroupsDesc.group_start.offset == 32
    ffi = _strip_comments(FFI)
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct dspfx_mixgroups_desc\s*\{(.*?)\}", ffi, re.S)
    assert m, "dspfx_mixgroups_desc is not a #[repr(C)] struct in ffi.rs"
    got = [f.strip().replace("pub ", "") for f in m.group(1).split(",") if f.strip()]
    assert got == [f"{n}: {RUST[t]}" for t, n in fields], got
    rs = _strip_comments(open(os.path.join(ROOT, "host", "rust", "src", "mix_groups.rs")).read())
    assert "pub struct MixGroups" in rs and "impl Drop for MixGroups" in rs
    assert "pub mod mix_groups;" in open(os.path.join(ROOT, "host", "rust", "src", "mod.rs")).read()
    for name, arity in NEW.items():
        m = re.search(r"pub fn %s\s*\(([^)]*)\)" % name, ffi)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == arity, name
        assert name + "(" in rs, name
        assert name + "(" in HPP, name
    assert "class MixGroups" in HPP and "mixgroups_plan" in HPP
    for attr in ("run", "set_gains", "close", "depth"):
        assert hasattr(dspfx.MixGroups, attr), attr
    assert callable(dspfx.mixgroups_plan)


def test_python_table_helpers(dspfx):
    assert np.array_equal(dspfx._group_table(1024, group_size=256), [0, 256, 512, 768, 1024])
    with pytest.raises(ValueError):
        dspfx._group_table(1000, group_size=256)
    with pytest.raises(ValueError):
        dspfx._group_table(1000)
    with pytest.raises(ValueError):
        dspfx._group_table(1000, group_start=[0, 1000], group_size=10)
    assert dspfx._group_table(10, group_start=[0, 4, 10]).dtype == np.uint64


def test_no_device_is_an_error_not_a_fallback(dspfx):
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(dspfx.DspfxError) as ei:
        dspfx.MixGroups(1024, group_size=256)
    assert ei.value.status == -2       # DSPFX_ERR_NO_DEVICE
    with pytest.raises(dspfx.DspfxError) as ei:
        dspfx.MixGroups(1024, group_start=[0, 2000])
    assert ei.value.status == INVALID and "n_channels" in str(ei.value)      # the table is checked before any device work
