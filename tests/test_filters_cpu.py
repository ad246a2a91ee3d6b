"""The channel-filter bank without a GPU: the restatement the GPU tests lean on (filters_ref: one oracle chain per channel) against
oracle.run_channels bit for bit for each kind and for the two-stage chains, with the state carried over runs of 37 + 128 + 91
frames; a plain numpy float32 model of the three recurrences, in the operation order the kernel states, against the oracle bit for
bit -- the check that the kernel's explicit-rounding restatement is the reference's arithmetic; the store rules (the same kind
keeps the state and the sliders left out, another kind starts from the defaults and a zero state, drop, reset, refusals);
dspfx_filters_plan; the create refusals and the argument checks that need no device; header, EXPORTS, ctypes signatures and ffi.rs
agree.  A store's own checks need a bank and so a device: here the restatement refuses them, tests/test_filters_gpu.py holds the
bank to that."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import filters_ref as R
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
FFI = open(os.path.join(ROOT, "host", "rust", "src", "ffi.rs")).read()
INVALID = -1
F = np.float32
NAMES = ("dspfx_filters_plan", "dspfx_filters_create", "dspfx_filters_destroy", "dspfx_filters_last_error", "dspfx_filters_run",
         "dspfx_filters_set_low_pass", "dspfx_filters_set_high_pass", "dspfx_filters_set_envelope", "dspfx_filters_drop",
         "dspfx_filters_reset", "dspfx_filters_present", "dspfx_filters_kinds", "dspfx_filters_sliders", "dspfx_filters_state")
RATIOS = (0.0, 0.5, 0.93, 1.0)                                                   # test_one_pole's
ENVELOPES = ((0.0, 0.0), (0.0, 64.0), (5.0, 0.0), (48.0, 1000.0), (0.5, 0.25))   # test_envelope_follower's
CUTS = (37, 128, 91)
NF = sum(CUTS)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def noise_block(n, nf):
    x = O.noise(0x5EED0001, np.arange(n), np.arange(nf)) * F(2.5)
    x[0, :10] = [0, -0.0, 0.25, -0.25, 0.5, -0.5, 1, -1, 2, -2][:n]
    return x


def in_cuts(ref, x):
    """x through ref in runs of 37 + 128 + 91 frames"""
    out, f0 = [], 0
    for n in CUTS:
        out.append(ref.run(x[f0:f0 + n]))
        f0 += n
    return np.concatenate(out)


def model(dspfx, kind, sliders, x, z=None):
    """the three recurrences in numpy float32, one rounding per operation, in the order filters_kernels.hip states them:
    LowPass fadd(fmul(x, fsub(1, r)), fmul(r, z)); HighPass the same z, then x - z; Envelope d = x < 0 ? -x : x,
    g = z < d ? ga : gr, z = d + (z + (-d)) * g.  -> (y, z)"""
    x = np.ascontiguousarray(x, F)
    z = np.zeros(x.shape[1], F) if z is None else z.copy()
    y = np.empty_like(x)
    with np.errstate(all="ignore"):
        if kind == R.ENVELOPE:
            ga, gr = dspfx.envelope_gain(sliders[0]), dspfx.envelope_gain(sliders[1])
            for f in range(len(x)):
                d = np.where(x[f] < 0, -x[f], x[f])
                g = np.where(z < d, F(ga), F(gr))
                z = d + (z + (-d)) * g
                y[f] = z
        else:
            r = F(sliders[0])
            omr = F(1) - r
            for f in range(len(x)):
                z = x[f] * omr + r * z
                y[f] = x[f] - z if kind == R.HIGH_PASS else z
    assert y.dtype == F and z.dtype == F
    return y, z


def test_the_entry_points_exist_in_the_header_the_exports_and_the_rust_bindings(dspfx):
    L = dspfx.lib()
    assert len(NAMES) == 14
    for name in NAMES:
        assert name in dspfx.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
        assert re.search(r"\b%s\s*\(" % name, HDR), name
        assert re.search(r"pub fn %s\s*\(" % name, FFI), name
    assert sorted(n for n in dspfx.EXPORTS if n.startswith("dspfx_filters_")) == sorted(NAMES)
    assert sorted(set(re.findall(r"\b(dspfx_filters_[a-z_]+)\s*\(", HDR))) == sorted(NAMES)
    assert sorted(set(re.findall(r"pub fn (dspfx_filters_[a-z_]+)\s*\(", FFI))) == sorted(NAMES)
    for m in ("run", "set_low_pass", "set_high_pass", "set_envelope", "drop", "reset", "present", "kinds", "sliders", "state", "close"):
        assert hasattr(dspfx.ChannelFilters, m), m
    assert callable(dspfx.filters_plan)
    assert "#define DSPFX_FILTERS_NONE 0xFFFFFFFFu" in HDR and dspfx.FILTERS_NONE == R.NONE == 0xFFFFFFFF
    assert "pub const DSPFX_FILTERS_NONE: u32 = 0xFFFF_FFFF;" in FFI and "pub struct dspfx_filters_desc" in FFI
    assert [f for f, _ in dspfx._FiltersDesc._fields_] == ["abi_version", "device", "n_channels", "max_frames", "tile_channels", "stages"]
    assert re.search(r"typedef struct dspfx_filters_desc \{[^}]*abi_version;[^}]*device;[^}]*n_channels;[^}]*max_frames;[^}]*tile_channels;[^}]*stages;[^}]*\}", HDR)
    assert (R.LOW_PASS, R.HIGH_PASS, R.ENVELOPE) == (dspfx.LOW_PASS, dspfx.HIGH_PASS, dspfx.ENVELOPE)
    assert dspfx.ABI_VERSION == 2 and L.dspfx_abi_version() == 2 and "#define DSPFX_ABI_VERSION 2" in HDR


def test_the_restatements_defaults_are_dspfx_node_defaults(dspfx):
    d = dspfx._NodeDesc()
    for kind in (R.LOW_PASS, R.HIGH_PASS, R.ENVELOPE):
        assert dspfx.lib().dspfx_node_defaults(kind, C.byref(d)) == 0
        assert tuple(float(v) for v in d.params[:2]) == R.DEFAULTS[kind], kind


@pytest.mark.parametrize("kind", ["low_pass", "high_pass"])
def test_restatement_and_model_of_the_one_poles_equal_the_oracle_bit_for_bit(dspfx, kind):
    n = 12
    x = noise_block(n, NF)
    mk, code = (dspfx.LowPass, R.LOW_PASS) if kind == "low_pass" else (dspfx.HighPass, R.HIGH_PASS)
    for r in RATIOS:
        want = O.run_channels([mk(r).oracle_desc()], x, 0)
        ref = R.ChannelFilters(n)
        assert getattr(ref, "set_" + kind)(0, r)
        assert np.array_equal(bits(in_cuts(ref, x)), bits(want)), (kind, r)
        assert np.array_equal(bits(model(dspfx, code, (r,), x)[0]), bits(want)), ("the numpy model", kind, r)


def test_restatement_and_model_of_the_envelope_equal_the_oracle_bit_for_bit(dspfx):
    n = 12
    x = noise_block(n, NF)
    for att, rel in ENVELOPES:
        want = O.run_channels([dspfx.Envelope(att, rel).oracle_desc()], x, 0)
        ref = R.ChannelFilters(n)
        assert ref.set_envelope(0, att, rel)
        assert np.array_equal(bits(in_cuts(ref, x)), bits(want)), (att, rel)
        assert np.array_equal(bits(model(dspfx, R.ENVELOPE, (att, rel), x)[0]), bits(want)), ("the numpy model", att, rel)


def test_restatement_and_model_of_the_two_stage_chains_equal_the_oracle_bit_for_bit(dspfx):
    """HighPass -> LowPass (the band-pass) and Envelope -> LowPass (the smoothed follower), every channel its own sliders' turn"""
    n = 12
    x = noise_block(n, NF)
    for hp, lp in ((0.05, 0.93), (0.5, 0.5), (1.0, 0.0)):
        want = O.run_channels([dspfx.HighPass(hp).oracle_desc(), dspfx.LowPass(lp).oracle_desc()], x, 0)
        ref = R.ChannelFilters(n, 2)
        assert ref.set_high_pass(0, hp) and ref.set_low_pass(1, lp)
        assert np.array_equal(bits(in_cuts(ref, x)), bits(want)), (hp, lp)
        mid, _ = model(dspfx, R.HIGH_PASS, (hp,), x)
        assert np.array_equal(bits(model(dspfx, R.LOW_PASS, (lp,), mid)[0]), bits(want)), ("the numpy model", hp, lp)
    for (att, rel), lp in (((48.0, 1000.0), 0.93), ((0.0, 64.0), 0.5)):
        want = O.run_channels([dspfx.Envelope(att, rel).oracle_desc(), dspfx.LowPass(lp).oracle_desc()], x, 0)
        ref = R.ChannelFilters(n, 2)
        assert ref.set_envelope(0, att, rel) and ref.set_low_pass(1, lp)
        assert np.array_equal(bits(in_cuts(ref, x)), bits(want)), (att, rel, lp)
        mid, _ = model(dspfx, R.ENVELOPE, (att, rel), x)
        assert np.array_equal(bits(model(dspfx, R.LOW_PASS, (lp,), mid)[0]), bits(want)), ("the numpy model", att, rel, lp)


def test_restatement_every_channel_its_own_chain(dspfx):
    """slot kinds (c + stage) % 4 over none / LowPass / HighPass / Envelope, four stages: each column is the oracle's run of that
    channel's present nodes alone, whatever stands beside it; an empty channel is a copy"""
    n, stages = 13, 4
    x = noise_block(n, NF)
    ref = R.ChannelFilters(n, stages)
    chains = {}
    for c in range(n):
        for s in range(stages):
            k = (c + s) % 4
            if c == 12:
                continue
            if k == 1:
                assert ref.set_low_pass(s, 0.93, first_channel=c, count=1)
                chains.setdefault(c, []).append(dspfx.LowPass(0.93))
            elif k == 2:
                assert ref.set_high_pass(s, 0.05, first_channel=c, count=1)
                chains.setdefault(c, []).append(dspfx.HighPass(0.05))
            elif k == 3:
                assert ref.set_envelope(s, 5.0, 64.0, first_channel=c, count=1)
                chains.setdefault(c, []).append(dspfx.Envelope(5.0, 64.0))
    got = in_cuts(ref, x)
    for c in range(n):
        if c in chains:
            want = O.run_channels([nd.oracle_desc() for nd in chains[c]], x[:, c:c + 1], 0)
            assert np.array_equal(bits(got[:, c:c + 1]), bits(want)), c
        else:
            assert np.array_equal(bits(got[:, c]), bits(x[:, c])), "no node: a copy"
    assert list(ref.present()) == [1] * 12 + [0]


def test_restatement_store_rules(dspfx):
    n = 6
    x = noise_block(n, NF)
    a, b = x[:37], x[37:165]
    ref = R.ChannelFilters(n, 2)
    assert ref.set_low_pass(0, 0.93, first_channel=1, count=2)
    assert list(ref.kind[0]) == [R.NONE, R.LOW_PASS, R.LOW_PASS, R.NONE, R.NONE, R.NONE] and (ref.kind[1] == R.NONE).all()
    assert list(ref.present()) == [0, 1, 1, 0, 0, 0]
    ya = ref.run(a)
    z_lp = ya[-1, 1].copy()
    assert z_lp != 0
    # the same kind: the slider left out is kept, and the state: the next sample continues from z
    assert ref.set_low_pass(0, first_channel=1, count=1) and ref.p[0, 1, 0] == F(0.93)
    assert ref.set_low_pass(0, 0.5, first_channel=2, count=1) and ref.p[0, 2, 0] == F(0.5)
    yb = ref.run(b)
    assert np.array_equal(bits(yb[:, 1]), bits(model(dspfx, R.LOW_PASS, (0.93,), b[:, 1:2], ya[-1, 1:2])[0][:, 0])), "the state is kept"
    assert np.array_equal(bits(yb[:, 2]), bits(model(dspfx, R.LOW_PASS, (0.5,), b[:, 2:3], ya[-1, 2:3])[0][:, 0])), "a new ratio, the old z"
    # another kind: the defaults and a zero state
    assert ref.set_high_pass(0, first_channel=1, count=1) and ref.kind[0, 1] == R.HIGH_PASS and ref.p[0, 1, 0] == F(0.5)
    assert np.array_equal(bits(ref.run(b)[:, 1]), bits(model(dspfx, R.HIGH_PASS, (0.5,), b[:, 1:2])[0][:, 0])), "a new node starts at +0.0"
    assert ref.set_envelope(0, release=64.0, first_channel=1, count=1) and list(ref.p[0, 1]) == [0.0, 64.0]
    assert ref.set_envelope(0, attack=5.0, first_channel=1, count=1) and list(ref.p[0, 1]) == [5.0, 64.0], "the same kind keeps the release"
    # drop: the slot copies again and a later store starts from the defaults
    assert ref.drop(0, 1, 1) and ref.kind[0, 1] == R.NONE and list(ref.p[0, 1]) == [0.0, 0.0]
    assert np.array_equal(bits(ref.run(a)[:, 1]), bits(a[:, 1]))
    assert ref.set_envelope(0, first_channel=1, count=1) and list(ref.p[0, 1]) == [0.0, 0.0]
    # reset: the state back to +0.0, nodes and sliders stay; of one stage, and of a sub-range
    two = R.ChannelFilters(n, 2)
    assert two.set_high_pass(0, 0.05) and two.set_low_pass(1, 0.93)
    first = two.run(a)
    assert two.reset(first_channel=2, count=2) and two.reset(stage=1, first_channel=5, count=1)
    again = two.run(a)
    assert np.array_equal(bits(again[:, 2:4]), bits(first[:, 2:4])) and not np.array_equal(bits(again[:, :2]), bits(first[:, :2]))
    assert not np.array_equal(bits(again[:, 5]), bits(first[:, 5])) and (two.kind[0] == R.HIGH_PASS).all() and (two.p[1, :, 0] == F(0.93)).all()
    # refusals: nothing changes
    before = [t.copy() for t in (ref.kind, ref.p)]
    for call in (lambda: ref.set_low_pass(2, 0.5), lambda: ref.set_high_pass(-1, 0.5), lambda: ref.set_envelope(0, 1.0, 2.0, first_channel=5, count=2),
                 lambda: ref.set_envelope(0, [1.0, 2.0], [1.0, 2.0, 3.0]), lambda: ref.set_low_pass(0, 0.5, first_channel=7, count=0),
                 lambda: ref.drop(2, 0, 1), lambda: ref.drop(0, 6, 1), lambda: ref.reset(stage=2), lambda: ref.reset(first_channel=0, count=7)):
        assert call() is False
    assert all(np.array_equal(u, v) for u, v in zip(before, (ref.kind, ref.p)))
    assert ref.set_low_pass(1, float("nan"), first_channel=0, count=1) and np.isnan(ref.p[1, 0, 0]), "values are taken as given"
    assert ref.set_low_pass(1, 7.5, first_channel=0, count=1) and ref.p[1, 0, 0] == 7.5


def test_plan_is_the_formula(dspfx):
    for n in (1, 70, 256, 1 << 20, 0xFFFFFF00):
        for stages in (1, 2, 3, 4):
            assert dspfx.filters_plan(n, stages) == 13 * stages * n
    for n in (0, 1 << 32, 0xFFFFFF01):
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.filters_plan(n, 2)
        assert e.value.status == INVALID and "n_channels" in str(e.value) and "filters" in str(e.value), str(e.value)
    for stages in (0, 5, 0xFFFFFFFF):
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.filters_plan(256, stages)
        assert e.value.status == INVALID and "stages" in str(e.value) and "filters" in str(e.value), str(e.value)


@pytest.mark.parametrize("kw,word", [
    (dict(stages=0), "stages"),
    (dict(stages=5), "stages"),
    (dict(tile_channels=48), "power of two"),
    (dict(tile_channels=64), "divides"),
    (dict(channels=0), "n_channels"),
    (dict(channels=0xFFFFFF01), "n_channels"),
    (dict(max_frames=0), "max_frames"),
    (dict(max_frames=(1 << 20) + 1), "max_frames"),
])
def test_create_rejects_a_bad_descriptor_before_any_device_work(dspfx, kw, word):
    args = dict(channels=1000, stages=2, tile_channels=0, max_frames=128)
    args.update(kw)
    with pytest.raises(dspfx.DspfxError) as e:
        dspfx.ChannelFilters(**args)
    assert e.value.status == INVALID and word in str(e.value) and "filters" in str(e.value), str(e.value)


def test_create_rejects_another_abi_version(dspfx):
    L = dspfx.lib()
    h = C.c_void_p()
    d = dspfx._FiltersDesc(dspfx.ABI_VERSION + 1, 0, 1000, 128, 0, 2)
    assert L.dspfx_filters_create(C.byref(d), C.byref(h)) == INVALID and not h.value
    assert b"abi_version" in L.dspfx_filters_last_error(None)


def test_null_arguments_are_invalid(dspfx):
    L = dspfx.lib()
    h = C.c_void_p()
    assert L.dspfx_filters_create(None, C.byref(h)) == INVALID
    assert L.dspfx_filters_last_error(None)
    assert L.dspfx_filters_destroy(None) == INVALID
    assert L.dspfx_filters_run(None, None, None, 128, None) == INVALID
    assert L.dspfx_filters_set_low_pass(None, 0, None, 0, 0) == INVALID
    assert L.dspfx_filters_set_high_pass(None, 0, None, 0, 0) == INVALID
    assert L.dspfx_filters_set_envelope(None, 0, None, None, 0, 0) == INVALID
    assert L.dspfx_filters_drop(None, 0, 0, 0) == INVALID
    assert L.dspfx_filters_reset(None, 0, 0, 0) == INVALID
    assert L.dspfx_filters_present(None, None, 0, 0) == INVALID
    assert L.dspfx_filters_kinds(None, 0, None, 0, 0) == INVALID
    assert L.dspfx_filters_sliders(None, 0, None, 0, 0) == INVALID
    assert L.dspfx_filters_state(None, 0, None) == INVALID
    assert L.dspfx_filters_plan(8, 1, None) == 0
