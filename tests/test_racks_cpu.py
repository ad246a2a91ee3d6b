"""The channel-rack bank without a GPU: the restatement the GPU tests lean on (racks_ref: one oracle chain per channel) against
oracle.run_channels bit for bit over mixed tables, the store rules and cuts of the frames into 37 + 128 + 91; dspfx_racks_plan
against the documented 37 bytes per channel and slot, and its refusals; the create refusals and the Python argument errors that
are raised before the library is called; header, EXPORTS, ctypes signatures and ffi.rs agree.  A store's own checks need a bank
and so a device: here the restatement refuses them, tests/test_racks_gpu.py holds the bank to that."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O
import racks_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
FFI = open(os.path.join(ROOT, "host", "rust", "src", "ffi.rs")).read()
INVALID = -1
F = np.float32
NAMES = ("dspfx_racks_plan", "dspfx_racks_create", "dspfx_racks_destroy", "dspfx_racks_last_error", "dspfx_racks_run", "dspfx_racks_set",
         "dspfx_racks_drop", "dspfx_racks_reset", "dspfx_racks_present", "dspfx_racks_kinds", "dspfx_racks_modes", "dspfx_racks_sliders",
         "dspfx_racks_state")
CUTS = (37, 128, 91)
NF = sum(CUTS)
MODES = (0, 1, 2, 3, 5, 6, 7, 8)                 # every Distort mode but Fuzz
RAW = ((1.0, -1.8, 0.81, 0.0025, 0.005, 0.0025), (-2.0, 0.6, -0.5, 1.5, 0.25, -0.75))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def noise_block(n, nf):
    x = O.noise(0x5EED0001, np.arange(n), np.arange(nf)) * F(2.5)
    x[0, :10] = [0, -0.0, 0.25, -0.25, 0.5, -0.5, 1, -1, 2, -2][:n]
    return x


def in_cuts(ref, x):
    out, f0 = [], 0
    for n in CUTS:
        out.append(ref.run(x[f0:f0 + n]))
        f0 += n
    return np.concatenate(out)


def spec(dspfx, k, c):
    """kind k of (empty, the eight kinds) with the slider set of channel c: two sets alternate every four channels, the Distort
    modes rotate with c"""
    a = (c // 4) % 2
    return (None, dspfx.Gain((0.5, 1.75)[a]), dspfx.BiQuad(*RAW[a]), dspfx.LowPass((0.93, 0.5)[a]), dspfx.HighPass((0.05, 0.5)[a]),
            dspfx.Envelope(*((5.0, 64.0), (48.0, 1000.0))[a]), dspfx.Distort((3.0, 30.0)[a], MODES[c % 8]),
            dspfx.Overdrive(*((5.0, 0.7, 0.9), (2.0, 0.25, 1.5))[a]), dspfx.Chebyshev(*((2.0, 7.5), (0.5, 3.0))[a]))[k]


def rotating(dspfx, ref, n, slots):
    """kinds (c + slot) % 9 over empty and the eight kinds -> {channel: [its NodeSpecs in slot order]}"""
    chains = {}
    for c in range(n):
        for s in range(slots):
            sp = spec(dspfx, (c + s) % 9, c)
            if sp is not None:
                assert ref.set(s, sp, first_channel=c, count=1)
                chains.setdefault(c, []).append(sp)
    return chains


def test_the_entry_points_exist_in_the_header_the_exports_and_the_rust_bindings(dspfx):
    L = dspfx.lib()
    for name in NAMES:
        assert name in dspfx.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
        assert re.search(r"\b%s\s*\(" % name, HDR), name
        assert re.search(r"pub fn %s\s*\(" % name, FFI), name
    assert sorted(n for n in dspfx.EXPORTS if n.startswith("dspfx_racks_")) == sorted(NAMES)
    assert sorted(set(re.findall(r"\b(dspfx_racks_[a-z_]+)\s*\(", HDR))) == sorted(NAMES)
    assert sorted(set(re.findall(r"pub fn (dspfx_racks_[a-z_]+)\s*\(", FFI))) == sorted(NAMES)
    for m in ("run", "set", "set_chain", "drop", "reset", "present", "kinds", "modes", "sliders", "state", "close"):
        assert hasattr(dspfx.ChannelRacks, m), m
    assert callable(dspfx.racks_plan)
    assert "#define DSPFX_RACKS_NONE 0xFFFFFFFFu" in HDR and dspfx.RACKS_NONE == R.NONE == 0xFFFFFFFF
    assert "#define DSPFX_RACKS_MAX_SLOTS 4" in HDR and dspfx.RACKS_MAX_SLOTS == R.MAX_SLOTS == 4
    assert "pub const DSPFX_RACKS_NONE: u32 = 0xFFFF_FFFF;" in FFI and "pub struct dspfx_racks_desc" in FFI
    assert [f for f, _ in dspfx._RacksDesc._fields_] == ["abi_version", "device", "n_channels", "max_frames", "tile_channels", "slots"]
    assert re.search(r"typedef struct dspfx_racks_desc \{[^}]*abi_version;[^}]*device;[^}]*n_channels;[^}]*max_frames;[^}]*tile_channels;[^}]*slots;[^}]*\}", HDR)
    for k in ("GAIN", "BIQUAD", "LOW_PASS", "HIGH_PASS", "ENVELOPE", "DISTORT", "OVERDRIVE", "CHEBYSHEV", "REVERB", "FIR", "ADD", "MIX", "SIGNAL_GEN"):
        assert getattr(R, k) == getattr(dspfx, k), k
    assert R.FUZZ == dspfx.FUZZ and R.LAST_MODE == dspfx.CHEBYSHEV4 and R.DEFAULT_MODE == dspfx.SOFT_CLIP


def test_the_restatements_defaults_are_dspfx_node_defaults(dspfx):
    d = dspfx._NodeDesc()
    for kind, n in R.SLIDERS.items():
        assert dspfx.lib().dspfx_node_defaults(kind, C.byref(d)) == 0
        assert tuple(F(v) for v in d.params[:n]) == tuple(F(v) for v in R.DEFAULTS[kind]), kind
        assert not any(d.params[n:8]), kind
    assert dspfx.lib().dspfx_node_defaults(R.DISTORT, C.byref(d)) == 0 and d.mode == R.DEFAULT_MODE


def test_restatement_of_every_single_kind_equals_the_oracle_bit_for_bit(dspfx):
    n = 12
    x = noise_block(n, NF)
    specs = [spec(dspfx, k, c) for k in (1, 2, 3, 4, 5, 7, 8) for c in (0, 4)] + [dspfx.Distort(3.0, m) for m in MODES] + [dspfx.Distort(0.0005, 2)]
    for sp in specs:
        for slot in (0, 3):
            ref = R.ChannelRacks(n, 4)
            assert ref.set(slot, sp)
            want = O.run_channels([sp.oracle_desc()], x, 0)
            assert np.array_equal(bits(in_cuts(ref, x)), bits(want)), (sp, slot)


def test_the_biquad_through_strips_ref_coeffs_is_the_oracles_own_normalisation(dspfx):
    """the restatement hands the oracle a0 = 1 and the five f32 quotients; the oracle given the raw sliders divides the same"""
    n = 6
    x = noise_block(n, 128)
    for raw in RAW + ((0.0, 1.0, 1.0, 1.0, 1.0, 1.0), (float("nan"), 1.0, 0.0, 1.0, 0.0, 0.0)):
        ref = R.ChannelRacks(n, 1)
        assert ref.set(0, dspfx.BiQuad(*raw))
        want = O.run_channels([dspfx.BiQuad(*raw).oracle_desc()], x, 0)
        got = ref.run(x)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(bits(got)[~np.isnan(want)], bits(want)[~np.isnan(want)]), raw
        assert np.array_equal(bits(dspfx.strips_coeffs(raw)), bits(R.strips_ref.coeffs(raw)))


@pytest.mark.parametrize("slots", [1, 2, 4])
def test_restatement_every_channel_its_own_chain(dspfx, slots):
    """kinds (c + slot) % 9, the Distort modes rotating with c, two slider sets: each column is the oracle's run of that channel's
    present nodes alone, whatever stands beside it; an empty channel is a copy"""
    n = 19
    x = noise_block(n, NF)
    ref = R.ChannelRacks(n, slots)
    chains = rotating(dspfx, ref, n, slots)
    got = in_cuts(ref, x)
    for c in range(n):
        if c in chains:
            want = O.run_channels([nd.oracle_desc() for nd in chains[c]], x[:, c:c + 1], 0)
            assert np.array_equal(bits(got[:, c:c + 1]), bits(want)), (c, chains[c])
            assert [d["kind"] for d in ref.descs(c)] == [nd.kind for nd in chains[c]]
        else:
            assert np.array_equal(bits(got[:, c]), bits(x[:, c])), "no node: a copy"
    assert list(ref.present()) == [sum(((c + s) % 9 != 0) << s for s in range(slots)) for c in range(n)]


def test_restatement_store_rules(dspfx):
    n = 8
    x = noise_block(n, NF)
    a, b = x[:37], x[37:165]
    one = lambda sp, xx: O.run_channels([sp.oracle_desc()], xx, 0)      # noqa: E731
    ref = R.ChannelRacks(n, 2)
    assert ref.set(0, dspfx.LowPass(0.93), first_channel=1, count=2) and ref.set(0, dspfx.BiQuad(*RAW[0]), first_channel=3, count=2)
    assert list(ref.kind[0]) == [R.NONE, R.LOW_PASS, R.LOW_PASS, R.BIQUAD, R.BIQUAD, R.NONE, R.NONE, R.NONE] and (ref.kind[1] == R.NONE).all()
    assert list(ref.present()) == [0, 1, 1, 1, 1, 0, 0, 0]
    ref.run(a)
    # the same kind: what is None is kept; a one-pole keeps its state, a BiQuad's is zeroed on the stored channels only
    assert ref.set(0, dspfx.LowPass(None), first_channel=1, count=1) and ref.p[0, 1, 0] == F(0.93)
    assert ref.set(0, dspfx.BiQuad(None, None, None, None, None, None), first_channel=3, count=1) and np.array_equal(ref.p[0, 3], np.asarray(RAW[0], F))
    yb = ref.run(b)
    cont = O.run_channels([dspfx.LowPass(0.93).oracle_desc()], x[:165, 1:2], 0)[37:]
    assert np.array_equal(bits(yb[:, 1:2]), bits(cont)), "a LowPass store of the same kind keeps the state"
    assert np.array_equal(bits(yb[:, 3:4]), bits(one(dspfx.BiQuad(*RAW[0]), b[:, 3:4]))), "a BiQuad store zeroes the state"
    assert np.array_equal(bits(yb[:, 4:5]), bits(one(dspfx.BiQuad(*RAW[0]), x[:165, 4:5])[37:])), "... on the stored channels only"
    # another kind: the defaults and a zero state
    assert ref.set(0, dspfx.HighPass(None), first_channel=1, count=1) and ref.kind[0, 1] == R.HIGH_PASS and ref.p[0, 1, 0] == F(0.5)
    assert np.array_equal(bits(ref.run(b)[:, 1:2]), bits(one(dspfx.HighPass(0.5), b[:, 1:2])))
    assert ref.set(0, dspfx.Envelope(None, 64.0), first_channel=1, count=1) and list(ref.p[0, 1]) == [0.0, 64.0, 0, 0, 0, 0]
    assert ref.set(0, dspfx.Envelope(5.0, None), first_channel=1, count=1) and list(ref.p[0, 1, :2]) == [5.0, 64.0], "the same kind keeps the release"
    assert ref.set(1, dspfx.Distort(3.0, dspfx.TANH), first_channel=1, count=1) and ref.mode[1, 1] == dspfx.TANH
    assert ref.set(1, dspfx.Distort(None, dspfx.SIN), first_channel=1, count=1) and ref.p[1, 1, 0] == 3.0 and ref.mode[1, 1] == dspfx.SIN
    assert ref.set(1, dspfx.Gain(None), first_channel=1, count=1) and ref.p[1, 1, 0] == 1.0 and ref.mode[1, 1] == R.NONE
    # drop: the slot copies again and a later store starts from the defaults; set_chain drops the slots behind the list
    assert ref.drop(0, 1, 1) and ref.kind[0, 1] == R.NONE and not ref.p[0, 1].any()
    assert ref.drop(1, 1, 1) and np.array_equal(bits(ref.run(a)[:, 1]), bits(a[:, 1]))
    assert ref.set(0, dspfx.Envelope(None, None), first_channel=1, count=1) and not ref.p[0, 1].any()
    assert ref.set(1, dspfx.Gain(2.0), first_channel=6, count=2) and ref.set_chain([dspfx.Overdrive(5, .7, .9)], first_channel=6, count=1)
    assert list(ref.kind[:, 6]) == [R.OVERDRIVE, R.NONE] and list(ref.kind[:, 7]) == [R.NONE, R.GAIN]
    # reset: the state back to +0.0, nodes and sliders stay; of one slot, and of a sub-range
    two = R.ChannelRacks(n, 2)
    assert two.set(0, dspfx.HighPass(0.05)) and two.set(1, dspfx.BiQuad(*RAW[0]))
    first = two.run(a)
    assert two.reset(first_channel=2, count=2) and two.reset(slot=1, first_channel=5, count=1)
    again = two.run(a)
    assert np.array_equal(bits(again[:, 2:4]), bits(first[:, 2:4])) and not np.array_equal(bits(again[:, :2]), bits(first[:, :2]))
    assert not np.array_equal(bits(again[:, 5]), bits(first[:, 5])) and (two.kind[0] == R.HIGH_PASS).all() and (two.p[1, :, 1] == F(-1.8)).all()
    # refusals: nothing changes
    before = [t.copy() for t in (ref.kind, ref.mode, ref.p)]
    for call in (lambda: ref.set(2, dspfx.Gain(1.0)), lambda: ref.set(-1, dspfx.Gain(1.0)), lambda: ref.set(0, dspfx.Gain(1.0), first_channel=7, count=2),
                 lambda: ref.set(0, dspfx.Envelope([1.0, 2.0], [1.0, 2.0, 3.0])), lambda: ref.set(0, dspfx.Gain(1.0), first_channel=9, count=0),
                 lambda: ref.set(0, dspfx.Reverb(0.1)), lambda: ref.set(0, dspfx.Fir()), lambda: ref.set(0, dspfx.Add()), lambda: ref.set(0, dspfx.Mix()),
                 lambda: ref.set(0, dspfx.SignalGen()), lambda: ref.set(0, dspfx.Distort(3.0, dspfx.FUZZ)), lambda: ref.set(0, dspfx.Distort(3.0, 9)),
                 lambda: ref.set(0, dspfx.Distort(3.0, [1, 1, dspfx.FUZZ])), lambda: ref.set_chain([dspfx.Gain(1.0)] * 3),
                 lambda: ref.drop(2, 0, 1), lambda: ref.drop(0, 8, 1), lambda: ref.reset(slot=2), lambda: ref.reset(first_channel=0, count=9)):
        assert call() is False
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(before, (ref.kind, ref.mode, ref.p)))
    assert ref.set(1, dspfx.LowPass(float("nan")), first_channel=0, count=1) and np.isnan(ref.p[1, 0, 0]), "values are taken as given"
    assert ref.set(1, dspfx.LowPass(7.5), first_channel=0, count=1) and ref.p[1, 0, 0] == 7.5


def test_plan_is_the_formula(dspfx):
    for n in (1, 70, 256, 1 << 20, 0xFFFFFF00):
        for slots in (1, 2, 3, 4):
            assert dspfx.racks_plan(n, slots) == R.BYTES_PER_SLOT * slots * n == 37 * slots * n
    for n in (0, 1 << 32, 0xFFFFFF01):
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.racks_plan(n, 2)
        assert e.value.status == INVALID and "n_channels" in str(e.value) and "racks" in str(e.value), str(e.value)
    for slots in (0, 5, 0xFFFFFFFF):
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.racks_plan(256, slots)
        assert e.value.status == INVALID and "slots" in str(e.value) and "racks" in str(e.value), str(e.value)


@pytest.mark.parametrize("kw,word", [
    (dict(slots=0), "slots"),
    (dict(slots=5), "slots"),
    (dict(tile_channels=48), "power of two"),
    (dict(tile_channels=64), "divides"),
    (dict(channels=0), "n_channels"),
    (dict(channels=0xFFFFFF01), "n_channels"),
    (dict(max_frames=0), "max_frames"),
    (dict(max_frames=(1 << 20) + 1), "max_frames"),
])
def test_create_rejects_a_bad_descriptor_before_any_device_work(dspfx, kw, word):
    args = dict(channels=1000, slots=2, tile_channels=0, max_frames=128)
    args.update(kw)
    with pytest.raises(dspfx.DspfxError) as e:
        dspfx.ChannelRacks(**args)
    assert e.value.status == INVALID and word in str(e.value) and "racks" in str(e.value), str(e.value)


def test_create_rejects_another_abi_version(dspfx):
    L = dspfx.lib()
    h = C.c_void_p()
    d = dspfx._RacksDesc(dspfx.ABI_VERSION + 1, 0, 1000, 128, 0, 2)
    assert L.dspfx_racks_create(C.byref(d), C.byref(h)) == INVALID and not h.value
    assert b"abi_version" in L.dspfx_racks_last_error(None)


def test_null_arguments_are_invalid(dspfx):
    L = dspfx.lib()
    h = C.c_void_p()
    assert L.dspfx_racks_create(None, C.byref(h)) == INVALID
    assert L.dspfx_racks_last_error(None)
    assert L.dspfx_racks_destroy(None) == INVALID
    assert L.dspfx_racks_run(None, None, None, 128, None) == INVALID
    assert L.dspfx_racks_set(None, 0, 0, None, None, 0, 0) == INVALID
    assert L.dspfx_racks_drop(None, 0, 0, 0) == INVALID
    assert L.dspfx_racks_reset(None, 0, 0, 0) == INVALID
    assert L.dspfx_racks_present(None, None, 0, 0) == INVALID
    assert L.dspfx_racks_kinds(None, 0, None, 0, 0) == INVALID
    assert L.dspfx_racks_modes(None, 0, None, 0, 0) == INVALID
    assert L.dspfx_racks_sliders(None, 0, None, 0, 0) == INVALID
    assert L.dspfx_racks_state(None, 0, None) == INVALID


class _NoLibrary:
    """a ChannelRacks whose every library call fails the test: the argument errors below are raised before one is made"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called: {name}")


def test_python_argument_errors_are_raised_before_the_library_is_called(dspfx):
    bank = dspfx.ChannelRacks.__new__(dspfx.ChannelRacks)
    bank.L, bank.h, bank.channels, bank.slots = _NoLibrary(), None, 16, 2
    for call, word in ((lambda: bank.set(0, "gain"), "NodeSpec"), (lambda: bank.set(0, None), "NodeSpec"),
                       (lambda: bank.set(0, dspfx.Envelope(np.ones(3), np.ones(4))), "different numbers"),
                       (lambda: bank.set(0, dspfx.Distort(np.ones(3), np.ones(2, np.uint32))), "different numbers"),
                       (lambda: bank.set(0, dspfx.Distort(1.0, 1.5)), "mode"), (lambda: bank.set(0, dspfx.Distort(1.0, -1)), "mode"),
                       (lambda: bank.set(0, dspfx.NodeSpec(dspfx.GAIN, [1.0, 2.0])), "sliders"),
                       (lambda: bank.set_chain([dspfx.Gain(1.0)] * 3), "slots"), (lambda: bank.set_chain([dspfx.Gain(1.0), 3.0]), "NodeSpec")):
        with pytest.raises(dspfx.DspfxError) as e:
            call()
        assert e.value.status == INVALID and word in str(e.value) and "racks" in str(e.value), str(e.value)
    bank.h = None                                # (nothing to destroy)
