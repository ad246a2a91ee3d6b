"""The talker bank without a GPU: the numpy restatement the GPU tests lean on (talkers_ref) against the oracle's Envelope node
(oracle.chain_run) bit for bit, a detector store in mid-stream included; dspfx_envelope_gain, dspfx_talkers_select and
dspfx_talkers_plan (pure host functions) against the oracle, the restatement and the formula; the exports, and the argument
checks that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O
import talkers_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
INVALID = -1
NF = 128
NAMES = ("dspfx_envelope_gain", "dspfx_talkers_plan", "dspfx_talkers_select", "dspfx_talkers_create", "dspfx_talkers_destroy",
         "dspfx_talkers_last_error", "dspfx_talkers_run", "dspfx_talkers_assign", "dspfx_talkers_set_detector", "dspfx_talkers_set_pin",
         "dspfx_talkers_set_top", "dspfx_talkers_set_floor", "dspfx_talkers_reset", "dspfx_talkers_views", "dspfx_talkers_room_of",
         "dspfx_talkers_counts")
ATTACKS, RELEASES = [0, 1, 48, 1000], [0, 1, 1000, 24000]
FRAMES = [0.0, 1.0, 0.5, 2.0, 48.0, 1000.0, 24000.0, 1e-3, 1e9, -1.0, -48.0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_entry_points_exist(dspfx):
    L = dspfx.lib()
    for name in NAMES:
        assert name in dspfx.EXPORTS and hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, HDR), name
    for m in ("run", "set_detector", "set_pin", "set_top", "set_floor", "assign", "reset", "room_of", "counts", "levels", "targets",
              "talkers", "talker_levels", "close"):
        assert hasattr(dspfx.Talkers, m), m
    for name, v in (("MAX_ROOM", 1024), ("MAX_TOP", 8), ("AUTO", 0), ("OPEN", 1), ("SHUT", 2)):
        assert getattr(dspfx, "TALKERS_" + name) == getattr(R, name) == v
        assert re.search(r"#define DSPFX_TALKERS_%s %d\b" % (name, v), HDR), name
    assert "#define DSPFX_TALKERS_NO_ROOM 0xFFFFFFFFu" in HDR and dspfx.NO_ROOM == R.NO_ROOM


def test_the_abi_version_is_still_2(dspfx):
    assert dspfx.ABI_VERSION == 2 and dspfx.lib().dspfx_abi_version() == 2
    assert "#define DSPFX_ABI_VERSION 2" in HDR


def oracle_gain(frames):
    """the release gain as the oracle's node applies it: attack 0 puts env at 1.0, then one frame of silence leaves 1.0 * gain"""
    return O.chain_run([O.Node(O.ENVELOPE, [0.0, float(frames)])], np.asarray([1.0, 0.0], np.float32), 0)[1]


def test_envelope_gain_equals_the_oracle(dspfx):
    for f in FRAMES:
        want = oracle_gain(f)
        assert bits(dspfx.envelope_gain(f)) == bits(want), f
        assert bits(R.envelope_gain(f)) == bits(want), f
    assert bits(dspfx.envelope_gain(0.0)) == 0 and bits(dspfx.envelope_gain(-0.0)) == 0


def test_restatement_equals_the_oracle_bit_for_bit():
    """every attack under every release, 6 blocks of 128, and after the third a detector store, which keeps env: the oracle's
    slider change sets only the gain"""
    rng = np.random.default_rng(3)
    combos = [(a, r) for a in ATTACKS for r in RELEASES]
    n = len(combos)
    x = R.noise(rng, 6 * NF, n)
    x[NF:NF + 40] *= np.float32(0.01)                            # a quiet stretch: the release is heard
    x[2 * NF + 5:2 * NF + 9] = np.float32(-0.0)
    x[5 * NF:] = 0
    ref = R.Talkers(n, [0, n])
    assert ref.set_detector(np.asarray([a for a, _ in combos], np.float32), np.asarray([r for _, r in combos], np.float32))
    later = [(combos[(i + 5) % n][0], combos[(i + 3) % n][1]) for i in range(n)]
    envs = []
    for b in range(6):
        if b == 3:
            assert ref.set_detector(np.asarray([a for a, _ in later], np.float32), np.asarray([r for _, r in later], np.float32))
        ref.run(x[b * NF:(b + 1) * NF])
        envs.append(ref.envs)
        assert np.array_equal(bits(ref.level), bits(ref.envs.max(axis=0))), "the level is the block's largest envelope"
    envs = np.concatenate(envs)
    for c, (a, r) in enumerate(combos):
        node = O.Node(O.ENVELOPE, [float(a), float(r)])
        first = O.chain_run([node], x[:3 * NF, c], 0)
        node.set_param(0, float(later[c][0]))
        node.set_param(1, float(later[c][1]))
        want = np.concatenate([first, O.chain_run([node], x[3 * NF:, c], 0)])
        assert np.array_equal(bits(envs[:, c]), bits(want)), (a, r)


def test_restatement_gate_and_run_order():
    """the four ramp cases, the last frame at the target, a selection audible one run later, gate=False"""
    rng = np.random.default_rng(4)
    n = 4
    x = R.noise(rng, 37, n)
    ref = R.Talkers(n, [0, n], top=1)
    x[:, 0] *= np.float32(4.0)                                   # channel 0 is the loudest
    y = ref.run(x)
    assert np.array_equal(bits(y), bits(x)), "a fresh bank passes its first block"
    assert list(ref.talkers[0]) == [0] + [-1] * 7 and list(ref.target) == [1, 0, 0, 0]
    y = ref.run(x)
    r = (np.arange(1, 38, dtype=np.float32) / np.float32(37))
    assert np.array_equal(bits(y[:, 0]), bits(x[:, 0])) and np.array_equal(bits(y[:, 1]), bits(x[:, 1] * (np.float32(1) + np.float32(-1) * r)))
    assert not y[-1, 1:].any(), "the last frame is at the target"
    x2 = x[:, [1, 0, 2, 3]]                                      # now channel 1 is the loudest
    gate = ref.gate.copy()
    assert ref.run(x2, gate=False) is None and np.array_equal(ref.gate, gate) and list(ref.target) == [0, 1, 0, 0]
    y = ref.run(x2)
    assert np.array_equal(bits(y[:, 0]), bits(x2[:, 0] * (np.float32(1) + np.float32(-1) * r))), "a ramp down"
    assert np.array_equal(bits(y[:, 1]), bits(x2[:, 1] * (np.float32(0) + np.float32(1) * r))), "a ramp up"
    assert np.array_equal(bits(y[:, 2]), np.zeros(37, np.uint32) | (bits(x2[:, 2]) & 0x80000000)), "closed: a zero with the sample's sign"


def both_select(dspfx, levels, room_of, groups, top, floor=0.0, pins=None):
    got = dspfx.talkers_select(levels, room_of, groups, top, floor, pins)
    want = R.select(levels, room_of, groups, top, floor, pins)
    for g, w, name in zip(got, want, ("talkers", "talker_levels", "target")):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint32), w.view(np.uint32)), name
    return got


def test_select_equals_the_restatement(dspfx):
    rng = np.random.default_rng(5)
    n, G = 1280, 7
    sizes = [1024, 1, 2, 33, 64, 65, 91]
    room = np.repeat(np.arange(G, dtype=np.uint32), sizes)
    lv = rng.uniform(0.0, 1.0, n).astype(np.float32)
    for top in (1, 3, 8):
        both_select(dspfx, lv, room, G, top)
    t, _, _ = both_select(dspfx, lv, room, G, np.asarray([8, 8, 8, 1, 2, 3, 4], np.uint8))
    assert (t[1] == [1024] + [-1] * 7).all() and (t[2, :2] >= 0).all() and (t[2, 2:] == -1).all(), "top above the room size"
    # an all-equal room: the lowest channel numbers, ascending
    eq = lv.copy()
    eq[:1024] = np.float32(0.25)
    t, _, _ = both_select(dspfx, eq, room, G, 8)
    assert list(t[0]) == list(range(8))
    # ties across and inside groups of 16 (a lane's members) and of 64 (the wave)
    ties = lv.copy() * np.float32(0.5)
    for c in (1000, 17, 16, 15, 64, 63, 700):
        ties[c] = np.float32(0.75)
    ties[3], ties[1023] = np.float32(0.8), np.float32(0.8)
    t, tl, _ = both_select(dspfx, ties, room, G, 8)
    assert list(t[0]) == [3, 1023, 15, 16, 17, 63, 64, 700]
    # levels equal to the floor are not selected; a floor above everything; a negative floor takes silent channels too
    fl = np.float32(0.5)
    at = lv.copy()
    at[1024:] = fl
    at[1100] = np.nextafter(fl, np.float32(1))
    t, _, tg = both_select(dspfx, at, room, G, 3, floor=fl)
    assert (t[1:4] == -1).all() and t[4, 0] == 1100 and t[4, 1] == -1 and tg[1024:].sum() == 1
    assert (both_select(dspfx, lv, room, G, 8, floor=2.0)[0] == -1).all()
    assert both_select(dspfx, np.zeros(n, np.float32), room, G, 2, floor=-1.0)[0][0, 1] == 1
    assert (both_select(dspfx, lv, room, G, 8, floor=float("nan"))[0] == -1).all()
    # pins: OPEN is passed and takes no slot, SHUT is neither passed nor ranked
    pins = np.zeros(n, np.uint8)
    order = np.argsort(-lv[:1024], kind="stable")
    pins[order[0]], pins[order[1]] = R.OPEN, R.SHUT
    t, _, tg = both_select(dspfx, lv, room, G, 3, pins=pins)
    assert list(t[0, :3]) == list(order[2:5]) and tg[order[0]] == 1 and tg[order[1]] == 0 and tg[:1024].sum() == 4
    # NO_ROOM and a reseated table: rooms scattered over the channels, a third of them in no room
    scattered = rng.integers(0, G, n).astype(np.uint32)
    scattered[rng.random(n) < 0.33] = R.NO_ROOM
    pins[rng.integers(0, n, 50)] = R.OPEN
    t, _, tg = both_select(dspfx, lv, scattered, G, 3, pins=pins)
    out = scattered == R.NO_ROOM
    assert np.array_equal(tg[out], (pins[out] == R.OPEN).astype(np.float32)), "no room: only an OPEN pin passes"
    assert not np.isin(t, np.flatnonzero(out)).any()
    moved = scattered.copy()
    moved[::3] = (moved[::3] + 1) % G
    both_select(dspfx, lv, moved, G, np.asarray([1, 2, 3, 4, 5, 6, 7], np.uint8), pins=pins)


@pytest.mark.parametrize("kw,word", [
    (dict(group_start=[0, 1025, 1280]), "DSPFX_TALKERS_MAX_ROOM"),
    (dict(top=0), "top"),
    (dict(top=9), "top"),
    (dict(group_start=[0, 640, 1281]), "n_channels"),            # a table past N
    (dict(group_start=[0, 640, 640, 1280]), "empty"),
    (dict(tile_channels=48), "power of two"),
    (dict(channels=0, group_start=[0, 0]), "n_channels"),
    (dict(max_frames=0), "max_frames"),
])
def test_create_rejects_a_bad_descriptor_before_any_device_work(dspfx, kw, word):
    args = dict(channels=1280, group_start=[0, 640, 1280], top=3, tile_channels=0, max_frames=128)
    args.update(kw)
    with pytest.raises(dspfx.DspfxError) as e:
        dspfx.Talkers(**args)
    assert e.value.status == INVALID and word in str(e.value) and "talkers" in str(e.value), str(e.value)


@pytest.mark.parametrize("kw,word", [
    (dict(room_of=np.r_[np.zeros(1025, np.uint32), np.ones(255, np.uint32)]), "DSPFX_TALKERS_MAX_ROOM"),
    (dict(top=0), "top"),
    (dict(top=9), "top"),
    (dict(top=np.asarray([3, 0], np.uint8)), "room 1"),
    (dict(room_of=np.r_[np.zeros(640, np.uint32), np.full(640, 2, np.uint32)]), "channel 640 is given room 2"),
    (dict(groups=0), "n_groups"),
])
def test_select_refuses_whole_and_gives_its_reason(dspfx, kw, word):
    args = dict(levels=np.ones(1280, np.float32), room_of=np.repeat(np.arange(2, dtype=np.uint32), 640), groups=2, top=3)
    args.update(kw)
    with pytest.raises(dspfx.DspfxError) as e:
        dspfx.talkers_select(**args)
    assert e.value.status == INVALID and word in str(e.value) and "talkers" in str(e.value), str(e.value)


def test_plan_is_the_formula(dspfx):
    for n, g in [(1, 1), (70, 3), (1280, 7), (1 << 20, 4096), (0xFFFFFF00, 1 << 22)]:
        assert dspfx.talkers_plan(n, g) == 29 * n + 69 * g + 4
    for args, word in (((0, 1), "n_channels"), ((1 << 32, 1), "n_channels"), ((8, 0), "rooms")):
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.talkers_plan(*args)
        assert e.value.status == INVALID and word in str(e.value), str(e.value)


def test_null_arguments_are_invalid(dspfx):
    L = dspfx.lib()
    h = C.c_void_p()
    assert L.dspfx_talkers_create(None, C.byref(h)) == INVALID
    assert L.dspfx_talkers_last_error(None)
    assert L.dspfx_talkers_destroy(None) == INVALID
    assert L.dspfx_talkers_run(None, None, None, 128, None) == INVALID
    assert L.dspfx_talkers_assign(None, None, 0, 0) == INVALID
    assert L.dspfx_talkers_set_detector(None, None, None, 0, 0) == INVALID
    assert L.dspfx_talkers_set_pin(None, None, 0, 0) == INVALID
    assert L.dspfx_talkers_set_top(None, None, 0, 0) == INVALID
    assert L.dspfx_talkers_set_floor(None, 0.0) == INVALID
    assert L.dspfx_talkers_reset(None, 0, 0) == INVALID
    assert L.dspfx_talkers_views(None, None, None, None, None) == INVALID
    assert L.dspfx_talkers_room_of(None, None, 0, 0) == INVALID
    assert L.dspfx_talkers_counts(None, None) == INVALID
    assert L.dspfx_talkers_select(None, None, 8, 1, None, 0.0, None, None, None, None) == INVALID
    assert L.dspfx_talkers_plan(8, 1, None) == 0
