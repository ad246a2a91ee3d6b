"""The audible list without a GPU: dspfx_talkers_audible (a pure host function) against a numpy restatement of the rule in
include/dspfx.h, over 12 blocks of the talker bank's restatement (talkers_ref) with an OPEN and a SHUT pin, a reset and an assign
in mid-stream; that every sample the rule leaves out is exactly zero; the bound on a room's list; the refusals; the exports; and a
CPU model of the sparse mix-matrix chain against mixmatrix_ref.eval_f32 on the gated block, bit for bit -- the claim the GPU tests
of dspfx_mixmatrix_run_sparse lean on."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import audible_ref as A
import mixmatrix_ref as X
import talkers_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
INVALID = -1
NAMES = ("dspfx_talkers_audible", "dspfx_talkers_audible_views", "dspfx_mixmatrix_run_sparse")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def played():
    """the script, played once on the restatement: per block (gate, target, room_of as the run found them; the gated block y)"""
    ref, pins, blocks = A.script()
    out = []
    for x, act in blocks:
        if act and act[0] == "reset":
            ref.reset(act[1], act[2])
        if act and act[0] == "assign":
            assert ref.assign(act[1], act[2])
        gate, target, room = ref.gate.copy(), ref.target.copy(), ref.room_of()
        out.append((gate, target, room, ref.run(x)))
    return ref, pins, out


def test_the_entry_points_exist(dspfx):
    L = dspfx.lib()
    for name in NAMES:
        assert name in dspfx.EXPORTS and hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, HDR), name
    assert callable(dspfx.talkers_audible) and hasattr(dspfx.Talkers, "audible")
    assert "sources" in inspect.signature(dspfx.MixMatrix.run).parameters
    assert dspfx.ABI_VERSION == 2 and "#define DSPFX_ABI_VERSION 2" in HDR      # additions only


def test_audible_equals_the_restatement_over_the_script(dspfx, played):
    ref, pins, out = played
    changed = 0
    for b, (gate, target, room, y) in enumerate(out):
        lists = A.check_tables(dspfx.talkers_audible(gate, target, room, A.G), gate, target, room, A.G)
        # every sample the rule leaves out is exactly zero (of either sign)
        quiet = np.ones(A.N, bool)
        quiet[np.concatenate(lists)] = False
        quiet &= room != A.NO_ROOM
        assert ((bits(y[:, quiet]) & 0x7FFFFFFF) == 0).all(), b
        if b and not np.array_equal(out[b - 1][1], target):
            changed += 1
        # from the third block after a fresh state a room lists its talkers, those fading out, and its OPEN pins
        if b >= 2 and b not in (A.RESET_BLOCK, A.RESET_BLOCK + 1):
            for g in range(A.G):
                n_open = int(((room == g) & (pins == R.OPEN)).sum())
                assert len(lists[g]) <= 2 * int(ref.top[g]) + n_open, (b, g, len(lists[g]))
    assert changed >= 6, "the script's talkers change from block to block"
    first = A.audible(*out[0][:3], A.G)[2]
    assert (first == np.diff(A.TABLE)).all(), "a fresh bank passes everybody"
    room = out[-1][2]
    assert room[65] == A.NO_ROOM and room[64] == 5, "the assign was played"
    assert not np.isin(A.SHUT_AT, np.concatenate(A.audible(*out[4][:3], A.G)[0])) and A.OPEN_AT in A.audible(*out[4][:3], A.G)[0][5]


def test_audible_on_a_scattered_seating_with_no_room_and_an_empty_room(dspfx):
    rng = np.random.default_rng(31)
    n, G = 700, 6
    room = rng.integers(0, G, n).astype(np.uint32)
    room[room == 2] = 4                                      # room 2 is empty
    room[rng.random(n) < 0.3] = A.NO_ROOM
    vals = np.asarray([0.0, -0.0, 1.0, 0.25, -1.0, 1e-45, np.nan], np.float32)
    gate, target = vals[rng.integers(0, len(vals), n)], vals[rng.integers(0, len(vals), n)]
    got = dspfx.talkers_audible(gate, target, room, G)
    lists = A.check_tables(got, gate, target, room, G)
    assert got[2][2] == 0 and got[1][2] == got[1][3]
    both_zero = (bits(gate) & 0x7FFFFFFF == 0) & (bits(target) & 0x7FFFFFFF == 0)
    assert both_zero.any() and not np.isin(np.flatnonzero(both_zero), np.concatenate(lists)).any(), "-0.0 is a zero"
    # one room of the largest size, all audible; and nobody audible
    one = np.zeros(1024, np.uint32)
    A.check_tables(dspfx.talkers_audible(np.ones(1024, np.float32), np.zeros(1024, np.float32), one, 1), np.ones(1024), np.zeros(1024), one, 1)
    lst, start, count = dspfx.talkers_audible(np.zeros(9, np.float32), np.zeros(9, np.float32), np.zeros(9, np.uint32), 2)
    assert count.tolist() == [0, 0] and start.tolist() == [0, 9, 9]


def test_audible_refuses_whole_and_gives_its_reason(dspfx):
    L = dspfx.lib()
    ones, room = np.ones(8, np.float32), np.zeros(8, np.uint32)
    bad = room.copy()
    bad[5] = 3
    for kw, word in ((dict(room_of=bad, groups=3), "channel 5 is given room 3"), (dict(groups=0), "n_groups"),
                     (dict(gate=np.ones(1025, np.float32), target=np.ones(1025, np.float32), room_of=np.zeros(1025, np.uint32)), "DSPFX_TALKERS_MAX_ROOM")):
        args = dict(gate=ones, target=ones, room_of=room, groups=1)
        args.update(kw)
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.talkers_audible(**args)
        assert e.value.status == INVALID and word in str(e.value) and "talkers" in str(e.value), str(e.value)
    fp, u32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    lst, start, count = np.zeros(8, np.int32), np.zeros(2, np.uint32), np.zeros(1, np.uint32)
    good = [ones.ctypes.data_as(fp), ones.ctypes.data_as(fp), room.ctypes.data_as(u32p), 8, 1, lst.ctypes.data_as(i32p), start.ctypes.data_as(u32p),
            count.ctypes.data_as(u32p)]
    assert L.dspfx_talkers_audible(*good) == 0 and count[0] == 8
    for i in (0, 1, 2, 5, 6, 7):                             # every pointer
        args = list(good)
        args[i] = None
        assert L.dspfx_talkers_audible(*args) == INVALID, i
        assert b"talkers audible" in L.dspfx_talkers_last_error(None)
    assert L.dspfx_talkers_audible_views(None, None, None, None) == INVALID
    assert L.dspfx_mixmatrix_run_sparse(None, None, 128, None, None, 0, None, None, None) == INVALID


def test_the_sparse_chain_is_the_dense_chain_on_the_gated_block(played):
    """eval_f32 restricted to the audible sources == eval_f32 on the whole gated block, bit for bit, for signed finite matrices:
    an unlisted sample is +-0.0, its product an exact zero, and adding one changes neither a non-zero sum nor the +0.0 the chain
    starts from."""
    ref, pins, out = played
    for b, (gate, target, room, y) in enumerate(out):
        yg, table, order = A.gathered_problem(y, room, A.G)
        mats = A.signed_mats(table, 40 + b)
        lists = A.audible(gate, target, room, A.G)[0]
        where = {int(c): i for i, c in enumerate(order)}
        listed = [[where[int(c)] - table[g] for c in lists[g]] for g in range(A.G)]
        dense = X.eval_f32(yg, table, mats)
        sparse = A.eval_sparse_f32(yg, table, mats, listed)
        assert np.isfinite(dense).all()
        assert (bits(sparse) == bits(dense)).all(), (b, np.argwhere(bits(sparse) != bits(dense))[:5])
        if b >= 2 and b not in (A.RESET_BLOCK, A.RESET_BLOCK + 1):
            assert sum(len(l) for l in listed) < len(order) // 4, "the lists are short: the comparison is not dense against dense"
