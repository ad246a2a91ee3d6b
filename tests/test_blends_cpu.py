"""The channel-blend bank without a GPU: the restatement the GPU tests lean on (blends_ref: one reference node per channel, from
numpy_model's add, mix, gain and slider_input) against oracle.run_channels bit for bit -- Add, Mix with a scalar and with a per-sample
ratio, with a send and without, with an unconnected b; its store rules; dspfx_blends_plan; the create refusals and the argument
checks that need no device; header, EXPORTS, the ctypes signatures and ffi.rs agree.  A store's own checks need a bank and so a
device: here the restatement refuses them, tests/test_blends_gpu.py holds the bank to that."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import blends_ref as R
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
FFI = open(os.path.join(ROOT, "host", "rust", "src", "ffi.rs")).read()
INVALID = -1
F = np.float32
NAMES = ("dspfx_blends_plan", "dspfx_blends_create", "dspfx_blends_destroy", "dspfx_blends_last_error", "dspfx_blends_run",
         "dspfx_blends_set_mix", "dspfx_blends_set_add", "dspfx_blends_set_send", "dspfx_blends_assign", "dspfx_blends_drop",
         "dspfx_blends_kinds", "dspfx_blends_ratios", "dspfx_blends_sends", "dspfx_blends_bus_of")
RATIOS = (0.0, 0.25, 0.5, 1.0, 1.5, -0.5, float("nan"))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want):
    """bit for bit; where the expectation is a NaN, a NaN"""
    got, want = np.asarray(got, F), np.asarray(want, F)
    return bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def blocks(n, nf, seed):
    a = O.noise(seed, np.arange(n), np.arange(nf))
    b = (O.noise(seed + 1, np.arange(n), np.arange(nf)) * F(0.75)).astype(F)
    a[0, 0], b[1 % nf, :] = -0.0, np.inf
    a.view(np.uint32)[nf // 2, n // 2] = 0x7FC12345
    return a, b


def test_the_entry_points_exist_in_the_header_the_exports_and_the_rust_bindings_with_the_declared_signatures(dspfx):
    L = dspfx.lib()
    body = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    for name in NAMES:
        assert name in dspfx.EXPORTS and hasattr(L, name), name
        m = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % name, body)
        assert m, name
        assert re.search(r"pub fn %s\s*\(" % name, FFI), name
        assert len(getattr(L, name).argtypes) == len(m.group(1).split(",")), (name, "the ctypes mirror takes as many arguments as the header declares")
    assert sorted(n for n in dspfx.EXPORTS if n.startswith("dspfx_blends_")) == sorted(NAMES)
    assert sorted(set(re.findall(r"\b(dspfx_blends_[a-z_]+)\s*\(", body))) == sorted(NAMES)
    fields = [d.strip().split()[-1] for d in re.search(r"typedef struct dspfx_blends_desc\s*\{(.*?)\}", body, re.S).group(1).split(";") if d.strip()]
    assert fields == [f for f, _ in dspfx._BlendsDesc._fields_] == ["abi_version", "device", "n_channels", "max_frames", "tile_channels", "n_buses"]
    assert L.dspfx_blends_run.argtypes[-2] is C.c_uint32 and L.dspfx_blends_assign.argtypes[1] is C.POINTER(C.c_uint32)
    assert L.dspfx_blends_last_error.restype is C.c_char_p
    for m in ("run", "set_mix", "set_add", "set_send", "assign", "drop", "kinds", "ratios", "sends", "bus_of", "close"):
        assert hasattr(dspfx.ChannelBlends, m), m
    assert callable(dspfx.blends_plan)
    assert "#define DSPFX_BLENDS_NO_BUS 0xFFFFFFFFu" in HDR and dspfx.BLENDS_NO_BUS == dspfx.NO_ROOM == R.NO_BUS == 0xFFFFFFFF
    assert "#define DSPFX_BLENDS_NONE 0xFFFFFFFFu" in HDR and dspfx.BLENDS_NONE == R.NONE == 0xFFFFFFFF
    assert "pub const DSPFX_BLENDS_NO_BUS: u32 = 0xFFFF_FFFF;" in FFI and "pub const DSPFX_BLENDS_NONE: u32 = 0xFFFF_FFFF;" in FFI
    assert "pub struct dspfx_blends_desc" in FFI
    assert (R.ADD, R.MIX) == (dspfx.ADD, dspfx.MIX)


def test_the_restatements_default_ratio_is_dspfx_node_defaults(dspfx):
    d = dspfx._NodeDesc()
    assert dspfx.lib().dspfx_node_defaults(dspfx.MIX, C.byref(d)) == 0
    assert float(d.params[0]) == R.DEFAULT_RATIO == 0.5


@pytest.mark.parametrize("send", [None, 0.7, 0.0])
def test_restatement_add_and_mix_equal_the_oracle_bit_for_bit(dspfx, send):
    """channel c: Add, then Mix at each of RATIOS; b a block, and b unconnected.  With a send the oracle's side block is b through
    the oracle's Gain node"""
    n, nf = 1 + len(RATIOS), 100
    a, b = blocks(n, nf, 3)
    ref = R.ChannelBlends(n)
    assert ref.set_add(0, 1) and ref.set_mix(np.asarray(RATIOS, F), first_channel=1)
    if send is not None:
        assert ref.set_send(send)
    descs = [dspfx.Add().oracle_desc()] + [dspfx.Mix(r).oracle_desc() for r in RATIOS]
    for second in (b, None):
        got = ref.run(a, b=second)
        side = None
        if second is not None:
            side = second if send is None else O.run_channels([dspfx.Gain(send).oracle_desc()], second, 0)
        elif send is not None:
            side = O.run_channels([dspfx.Gain(send).oracle_desc()], np.zeros_like(a), 0)
        for c in range(n):
            want = O.run_channels([descs[c]], a[:, c:c + 1], 0, None if side is None else side[:, c:c + 1])
            assert same(got[:, c:c + 1], want), (c, send, second is None)


def test_restatement_mix_with_a_per_sample_ratio_equals_the_oracle_bit_for_bit(dspfx):
    """the control block holds values below -1, above 1 and NaN; a fresh oracle node's first block, so its latch is not seen.  Add
    and absent channels do not read the block"""
    n, nf = 4, 128
    a, b = blocks(n, nf, 5)
    ctl = (O.noise(9, np.arange(n), np.arange(nf)) * F(1.6)).astype(F)
    ctl[3, :], ctl[4, :], ctl[5, :] = -1.5, 1.25, np.nan
    ref = R.ChannelBlends(n)
    assert ref.set_mix(0.3, 0, 2) and ref.set_add(2, 1) and ref.set_send(0.4, 1, 1)
    got = ref.run(a, b=b, ratio=ctl)
    assert np.nanmin(ctl) < -1 and np.nanmax(ctl) > 1 and np.isnan(ctl).any()
    for c in range(2):
        side = b[:, c:c + 1] if c == 0 else O.run_channels([dspfx.Gain(0.4).oracle_desc()], b[:, c:c + 1], 0)
        want = O.run_channels([dspfx.Mix(0.3).oracle_desc()], a[:, c:c + 1], 0, side, ctl={(0, 0): ctl[:, c:c + 1]})
        assert same(got[:, c:c + 1], want), c
    assert same(got[:, 2:3], O.run_channels([dspfx.Add().oracle_desc()], a[:, 2:3], 0, b[:, 2:3]))
    assert np.array_equal(bits(got[:, 3]), bits(a[:, 3])), "no node: a's very bits"
    assert list(ref.ratios()) == [F(0.3), F(0.3), 0, 0], "no latch"
    assert same(ref.run(a, b=b)[:, :1], O.run_channels([dspfx.Mix(0.3).oracle_desc()], a[:, :1], 0, b[:, :1])), "a later run goes by the stored ratio"


def test_restatement_bus_mode_is_block_mode_on_the_gathered_block():
    n, nf, G = 12, 37, 3
    a, _ = blocks(n, nf, 7)
    bus = O.noise(11, np.arange(G), np.arange(nf))
    ref = R.ChannelBlends(n, buses=G)
    assert ref.set_mix(0.25, 0, 6) and ref.set_add(6, 5) and ref.set_send(2.0, 3, 6)
    ids = np.arange(n) % G
    ids[::5] = R.NO_BUS
    assert ref.assign(ids)
    B = np.zeros((nf, n), F)
    for c in range(n):
        if ids[c] != R.NO_BUS:
            B[:, c] = bus[:, ids[c]]
    assert same(ref.run(a, bus=bus), ref.run(a, b=B))
    assert np.array_equal(bits(ref.run(a, bus=bus)[:, 11]), bits(a[:, 11])), "no node"


def test_restatement_store_rules():
    ref = R.ChannelBlends(6, buses=2)
    assert (ref.kinds() == R.NONE).all() and not ref.ratios().any() and not ref.sends()[1].any() and (ref.bus_of() == R.NO_BUS).all()
    assert ref.set_mix(first_channel=1, count=2) and list(ref.ratios()) == [0, 0.5, 0.5, 0, 0, 0], "a new Mix node: 0.5"
    assert ref.set_mix(0.8, 2, 1) and ref.set_mix(first_channel=1, count=2) and list(ref.ratios()[1:3]) == [0.5, F(0.8)], "None keeps a Mix node's ratio"
    assert ref.set_add(2, 2) and list(ref.kinds()[1:4]) == [R.MIX, R.ADD, R.ADD] and ref.ratios()[2] == 0
    assert ref.set_mix(None, 2, 1) and ref.ratios()[2] == 0.5, "set_mix(None) over an Add node gives 0.5"
    assert ref.set_send(0.3, 0, 2) and list(ref.sends()[1]) == [1, 1, 0, 0, 0, 0] and ref.kinds()[0] == R.NONE, "a send names no node"
    assert ref.set_send(float("nan"), 1, 1) and np.isnan(ref.sends()[0][1]) and ref.sends()[1][1] == 1, "values are taken as given"
    assert ref.set_mix(float("inf"), 4, 1) and np.isinf(ref.ratios()[4]) and ref.set_mix(-3.0, 4, 1) and ref.ratios()[4] == -3.0, "no clamp"
    assert ref.assign([0, 1, R.NO_BUS, 1], 1) and list(ref.bus_of()) == [R.NO_BUS, 0, 1, R.NO_BUS, 1, R.NO_BUS]
    before = [t.copy() for t in (ref.kinds(), ref.ratios(), *ref.sends(), ref.bus_of())]
    for call in (lambda: ref.set_mix(0.1, 5, 2), lambda: ref.set_mix([0.1] * 7), lambda: ref.set_add(7, 0), lambda: ref.set_send(1.0, 3, 4),
                 lambda: ref.assign([0, 2], 0), lambda: ref.assign(2, 0), lambda: ref.assign([0, 0], 5), lambda: ref.drop(6, 1),
                 lambda: ref.run(np.zeros((4, 6), F), b=np.zeros((4, 6), F), bus=np.zeros((4, 2), F)), lambda: ref.run(np.zeros((129, 6), F))):
        assert call() is False
    assert R.ChannelBlends(6).run(np.zeros((4, 6), F), bus=np.zeros((4, 2), F)) is False, "bus on a bank without buses"
    assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(before, (ref.kinds(), ref.ratios(), *ref.sends(), ref.bus_of()))), "a refused store changes nothing"
    assert ref.drop(1, 2) and list(ref.kinds()[:3]) == [R.NONE] * 3 and not ref.ratios()[1:3].any() and list(ref.sends()[1][:3]) == [1, 0, 0]
    assert list(ref.bus_of()[1:3]) == [0, 1], "drop keeps the bus id"
    assert ref.set_mix(first_channel=2, count=1) and ref.ratios()[2] == 0.5, "after a drop: the default"
    assert ref.set_send(None, 0, 1) and not ref.sends()[1][0] and ref.sends()[0][0] == 0


def test_plan_is_the_formula(dspfx):
    for n in (1, 70, 256, 1 << 20, 0xFFFFFF00):
        assert dspfx.blends_plan(n) == 13 * n, "ratio, send level, bus id: 4 bytes each; the kind / presence byte"
    for n in (0, 1 << 32, 0xFFFFFF01):
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.blends_plan(n)
        assert e.value.status == INVALID and "n_channels" in str(e.value) and "blends" in str(e.value), str(e.value)


@pytest.mark.parametrize("kw,word", [
    (dict(tile_channels=48), "power of two"),
    (dict(tile_channels=64), "divides"),
    (dict(channels=0), "n_channels"),
    (dict(max_frames=0), "max_frames"),
    (dict(max_frames=(1 << 20) + 1), "max_frames"),
])
def test_create_rejects_a_bad_descriptor_before_any_device_work(dspfx, kw, word):
    args = dict(channels=1000, tile_channels=0, max_frames=128)
    args.update(kw)
    with pytest.raises(dspfx.DspfxError) as e:
        dspfx.ChannelBlends(**args)
    assert e.value.status == INVALID and word in str(e.value) and "blends" in str(e.value), str(e.value)


def test_create_rejects_another_abi_version(dspfx):
    L = dspfx.lib()
    h = C.c_void_p()
    d = dspfx._BlendsDesc(dspfx.ABI_VERSION + 1, 0, 1000, 128, 0, 0)
    assert L.dspfx_blends_create(C.byref(d), C.byref(h)) == INVALID and not h.value
    assert b"abi_version" in L.dspfx_blends_last_error(None)


def test_null_arguments_are_invalid(dspfx):
    L = dspfx.lib()
    h = C.c_void_p()
    assert L.dspfx_blends_create(None, C.byref(h)) == INVALID
    assert L.dspfx_blends_last_error(None)
    assert L.dspfx_blends_destroy(None) == INVALID
    assert L.dspfx_blends_run(None, None, None, None, None, None, 128, None) == INVALID
    assert L.dspfx_blends_set_mix(None, None, 0, 0) == INVALID
    assert L.dspfx_blends_set_add(None, 0, 0) == INVALID
    assert L.dspfx_blends_set_send(None, None, 0, 0) == INVALID
    assert L.dspfx_blends_assign(None, None, 0, 0) == INVALID
    assert L.dspfx_blends_drop(None, 0, 0) == INVALID
    for name in ("kinds", "ratios", "bus_of"):
        assert getattr(L, "dspfx_blends_" + name)(None, None, 0, 0) == INVALID
    assert L.dspfx_blends_sends(None, None, None, 0, 0) == INVALID
    assert L.dspfx_blends_plan(8, None) == 0
