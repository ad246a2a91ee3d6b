"""The channel-shaper bank without a GPU: the restatement the GPU tests lean on (shapers_ref: one oracle node per channel) against
oracle.run_channels bit for bit for every kind, the bypass levels among them; its store rules (a set of another family replaces
the node from the reference's defaults, a set of the same family keeps the sliders left out, a drop makes a copy again);
dspfx_shapers_plan; the create refusals and the argument checks that need no device; header, EXPORTS and ffi.rs agree.  A store's
own checks need a bank and so a device: here the restatement refuses them, tests/test_shapers_gpu.py holds the bank to that."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O
import shapers_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
FFI = open(os.path.join(ROOT, "host", "rust", "src", "ffi.rs")).read()
INVALID = -1
NF = 128
F = np.float32
NAMES = ("dspfx_shapers_plan", "dspfx_shapers_create", "dspfx_shapers_destroy", "dspfx_shapers_last_error", "dspfx_shapers_run",
         "dspfx_shapers_set_distort", "dspfx_shapers_set_overdrive", "dspfx_shapers_set_chebyshev", "dspfx_shapers_drop",
         "dspfx_shapers_present", "dspfx_shapers_kinds", "dspfx_shapers_modes", "dspfx_shapers_sliders")
LEVELS = (0.0, 0.0009, 0.001, 1.0, 3.0, 30.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def noise_block(n, nf):
    x = O.noise(0x5EED0001, np.arange(n), np.arange(nf)) * F(2.5)
    x[0, :10] = [0, -0.0, 0.25, -0.25, 0.5, -0.5, 1, -1, 2, -2]      # (tests/test_gpu_parity.py, test_distort_arithmetic_modes)
    return x


def same(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(got)) and np.array_equal(bits(got)[~nan], bits(want)[~nan]), what


def test_the_entry_points_exist_in_the_header_the_exports_and_the_rust_bindings(dspfx):
    L = dspfx.lib()
    for name in NAMES:
        assert name in dspfx.EXPORTS and hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, HDR), name
        assert re.search(r"pub fn %s\s*\(" % name, FFI), name
    assert sorted(n for n in dspfx.EXPORTS if n.startswith("dspfx_shapers_")) == sorted(NAMES)
    assert sorted(set(re.findall(r"\b(dspfx_shapers_[a-z_]+)\s*\(", HDR))) == sorted(NAMES)
    for m in ("run", "set_distort", "set_overdrive", "set_chebyshev", "drop", "present", "kinds", "modes", "sliders", "close"):
        assert hasattr(dspfx.ChannelShapers, m), m
    assert not hasattr(dspfx.ChannelShapers, "reset"), "the shapers have no state"
    assert callable(dspfx.shapers_plan)
    assert "#define DSPFX_SHAPERS_NONE 0xFFFFFFFFu" in HDR and dspfx.SHAPERS_NONE == R.NONE == 0xFFFFFFFF
    assert "pub const DSPFX_SHAPERS_NONE: u32 = 0xFFFF_FFFF;" in FFI and "pub struct dspfx_shapers_desc" in FFI
    assert (R.DISTORT, R.OVERDRIVE, R.CHEBYSHEV, R.FUZZ) == (dspfx.DISTORT, dspfx.OVERDRIVE, dspfx.CHEBYSHEV, dspfx.FUZZ)
    assert R.N_MODES == len(dspfx.DISTORT_MODES)
    assert dspfx.ABI_VERSION == 2 and L.dspfx_abi_version() == 2


def test_the_restatements_defaults_are_dspfx_node_defaults(dspfx):
    d = dspfx._NodeDesc()
    for kind in (R.DISTORT, R.OVERDRIVE, R.CHEBYSHEV):
        assert dspfx.lib().dspfx_node_defaults(kind, C.byref(d)) == 0
        assert [float(v) for v in d.params[:3]] == [0.0, 0.0, 0.0], kind
        if kind == R.DISTORT:
            assert d.mode == R.DEFAULT_MODE == dspfx.SOFT_CLIP


@pytest.mark.parametrize("mode", range(9))
def test_restatement_distort_equals_the_oracle_bit_for_bit(dspfx, mode):
    """every level of test_distort_arithmetic_modes, the bypass levels 0, 0.0009 and 0.001 among them, in channels side by side"""
    n = 12
    x = noise_block(n, 2 * NF)
    for level in LEVELS:
        ref = R.ChannelShapers(n)
        assert ref.set_distort(level, mode)
        got = ref.run(x)
        want = O.run_channels([dspfx.Distort(level, mode).oracle_desc()], x, 0)
        same(got, want, (mode, level))
        if level < 0.001 and mode != dspfx.FUZZ:
            assert np.array_equal(bits(got), bits(x)), "the bypass keeps the sample's bits"
        elif mode != dspfx.FUZZ:
            assert not np.array_equal(bits(got), bits(x))


def test_restatement_overdrive_and_chebyshev_equal_the_oracle_bit_for_bit(dspfx):
    n = 12
    x = noise_block(n, 2 * NF)
    for boost, drive, level in ((5.0, 0.7, 0.9), (5.0, 0.7, 0.0009), (5.0, 0.7, 0.001), (5.0, 0.7, 0.0), (0.0, 0.0, 0.0), (30.0, 1.0, 1.0)):
        ref = R.ChannelShapers(n)
        assert ref.set_overdrive(boost, drive, level)
        want = O.run_channels([dspfx.Overdrive(boost, drive, level).oracle_desc()], x, 0)
        same(ref.run(x), want, (boost, drive, level))
        if level < 0.001:
            assert np.array_equal(bits(want), bits(x))
    for lp, ln in ((4.0, 0.0), (2.0, 7.5), (0.0, 0.0), (0.0009, 3.0), (0.001, 0.0009), (0.0, 0.001)):
        ref = R.ChannelShapers(n)
        assert ref.set_chebyshev(lp, ln)
        want = O.run_channels([dspfx.Chebyshev(lp, ln).oracle_desc()], x, 0)
        same(ref.run(x), want, (lp, ln))
        pos = x >= 0
        if lp < 0.001:
            assert np.array_equal(bits(want)[pos], bits(x)[pos]), "Chebyshev bypasses per branch"
        if ln < 0.001:
            assert np.array_equal(bits(want)[~pos], bits(x)[~pos])


def test_restatement_every_channel_its_own_kind(dspfx):
    """channel c carries kind c % 13: each column is the oracle's run of that node alone, whatever stands beside it"""
    n = 26
    x = noise_block(n, 2 * NF)
    ref = R.ChannelShapers(n)
    descs = {}
    for c in range(n):
        k = c % 13
        if k < 9:
            assert ref.set_distort(3.0, k, first_channel=c, count=1)
            descs[c] = dspfx.Distort(3.0, k)
        elif k == 9:
            assert ref.set_overdrive(5.0, 0.7, 0.9, first_channel=c, count=1)
            descs[c] = dspfx.Overdrive(5.0, 0.7, 0.9)
        elif k == 10:
            assert ref.set_chebyshev(2.0, 7.5, first_channel=c, count=1)
            descs[c] = dspfx.Chebyshev(2.0, 7.5)
    got = ref.run(x)
    for c in range(n):
        if c in descs:
            want = O.run_channels([descs[c].oracle_desc()], x[:, c:c + 1], 0)
            same(got[:, c:c + 1], want, c)
        else:
            assert np.array_equal(bits(got[:, c]), bits(x[:, c])), "no node: a copy"
    assert list(ref.present()) == [0 if c % 13 > 10 else 1 for c in range(n)]
    assert ref.run(x[:64]) is False and ref.drop(4, 1) and ref.drop(17, 1) and ref.run(x[:64]) is not False, "Fuzz needs whole blocks"


def test_restatement_store_rules():
    ref = R.ChannelShapers(6)
    assert ref.set_distort(level=3.0, mode=R.FUZZ, first_channel=1, count=2)
    assert list(ref.kind) == [R.NONE, R.DISTORT, R.DISTORT, R.NONE, R.NONE, R.NONE] and list(ref.mode[1:3]) == [R.FUZZ, R.FUZZ]
    assert ref.set_distort(level=[1.0, 2.0], first_channel=2) and ref.mode[2] == R.FUZZ and ref.mode[3] == R.DEFAULT_MODE, "the same family keeps the mode; a new node takes the default"
    assert ref.set_distort(mode=0, first_channel=2, count=1) and ref.p[2, 0] == 1.0, "... and keeps the level"
    assert ref.set_overdrive(drive=0.7, first_channel=2, count=1) and list(ref.p[2]) == [0.0, F(0.7), 0.0] and ref.mode[2] == R.NONE, "another family: the defaults"
    assert ref.set_overdrive(boost=5.0, first_channel=2, count=1) and list(ref.p[2]) == [5.0, F(0.7), 0.0]
    assert ref.set_chebyshev(level_neg=7.5, first_channel=2, count=1) and list(ref.p[2]) == [0.0, 7.5, 0.0]
    assert ref.set_distort(first_channel=2, count=1) and ref.p[2, 0] == 0 and ref.mode[2] == R.DEFAULT_MODE
    before = [t.copy() for t in (ref.kind, ref.mode, ref.p)]
    for call in (lambda: ref.set_distort(1.0, 9), lambda: ref.set_distort(1.0, [1, 2, 3, 4, 5, -1]), lambda: ref.set_distort(1.0, 1, first_channel=5, count=2),
                 lambda: ref.set_overdrive(1.0, first_channel=7, count=0), lambda: ref.set_chebyshev(1.0, first_channel=0, count=7), lambda: ref.drop(6, 1)):
        assert call() is False
    assert all(np.array_equal(u, v) for u, v in zip(before, (ref.kind, ref.mode, ref.p)))
    assert ref.drop(1, 1) and ref.kind[1] == R.NONE and ref.set_distort(mode=R.FUZZ, first_channel=1, count=1) and ref.p[1, 0] == 0, "after a drop: the defaults"
    assert ref.set_distort(float("nan"), 2, first_channel=0, count=1) and np.isnan(ref.p[0, 0]), "values are taken as given"


def test_plan_is_the_formula(dspfx):
    for n in (1, 70, 256, 1 << 20, 0xFFFFFF00):
        assert dspfx.shapers_plan(n) == 13 * n
    for n in (0, 1 << 32, 0xFFFFFF01):
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.shapers_plan(n)
        assert e.value.status == INVALID and "n_channels" in str(e.value) and "shapers" in str(e.value), str(e.value)


@pytest.mark.parametrize("kw,word", [
    (dict(tile_channels=48), "power of two"),
    (dict(tile_channels=64), "divides"),
    (dict(channels=0), "n_channels"),
    (dict(channels=0xFFFFFF01), "n_channels"),
    (dict(max_frames=0), "max_frames"),
    (dict(max_frames=(1 << 20) + 1), "max_frames"),
])
def test_create_rejects_a_bad_descriptor_before_any_device_work(dspfx, kw, word):
    args = dict(channels=1000, tile_channels=0, max_frames=128)
    args.update(kw)
    with pytest.raises(dspfx.DspfxError) as e:
        dspfx.ChannelShapers(**args)
    assert e.value.status == INVALID and word in str(e.value) and "shapers" in str(e.value), str(e.value)


def test_null_arguments_are_invalid(dspfx):
    L = dspfx.lib()
    h = C.c_void_p()
    assert L.dspfx_shapers_create(None, C.byref(h)) == INVALID
    assert L.dspfx_shapers_last_error(None)
    assert L.dspfx_shapers_destroy(None) == INVALID
    assert L.dspfx_shapers_run(None, None, None, 128, None) == INVALID
    assert L.dspfx_shapers_set_distort(None, None, None, 0, 0) == INVALID
    assert L.dspfx_shapers_set_overdrive(None, None, None, None, 0, 0) == INVALID
    assert L.dspfx_shapers_set_chebyshev(None, None, None, 0, 0) == INVALID
    assert L.dspfx_shapers_drop(None, 0, 0) == INVALID
    for name in ("present", "kinds", "modes", "sliders"):
        assert getattr(L, "dspfx_shapers_" + name)(None, None, 0, 0) == INVALID
    assert L.dspfx_shapers_plan(8, None) == 0
