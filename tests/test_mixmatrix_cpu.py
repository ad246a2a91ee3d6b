"""The mix-matrix bank without a GPU: the host-only plan (dspfx_mixmatrix_plan), the descriptor checks of dspfx_mixmatrix_create --
which must answer DSPFX_ERR_INVALID with a reason on a machine without a device, so they run before any device work -- and the
identities of the float64 reference the GPU tests lean on (mixmatrix_ref)."""
import ctypes as C

import numpy as np
import pytest

import mixgroups_ref as R
import mixmatrix_ref as X
import mixreturns_ref as M

RAGGED = [0, 1, 3, 34, 66, 99, 355, 612, 1636]          # n = 1, 2, 31, 32, 33, 256, 257, 1024


def check_plan(dspfx, channels, table, **kw):
    count, edge, offset, total = dspfx.mixmatrix_plan(channels, **kw)
    sizes = np.diff(np.asarray(table, np.int64))
    assert count.tolist() == sizes.tolist()
    assert edge.tolist() == [(int(n) + 31) // 32 * 32 for n in sizes]
    # the tables are disjoint and back to back: each starts where the one before ends
    ends = offset.astype(np.int64) + edge.astype(np.int64) ** 2
    assert offset[0] == 0 and (offset[1:].astype(np.int64) == ends[:-1]).all()
    assert total == 4 * int(ends[-1])
    return count, edge, offset, total


def test_plan_uniform(dspfx):
    _, edge, _, total = check_plan(dspfx, 1 << 20, np.arange(0, (1 << 20) + 1, 256), group_size=256)
    assert (edge == 256).all() and total == 1 << 30        # 4096 rooms of 256: 1 GiB
    check_plan(dspfx, 96, [0, 32, 64, 96], group_size=32, tile_channels=32)
    check_plan(dspfx, 7, list(range(8)), group_size=1)


def test_plan_ragged(dspfx):
    count, edge, _, total = check_plan(dspfx, 1636, RAGGED, group_start=RAGGED)
    assert count.tolist() == [1, 2, 31, 32, 33, 256, 257, 1024]
    assert edge.tolist() == [32, 32, 32, 32, 64, 256, 288, 1024]
    assert total == 4 * (4 * 32 * 32 + 64 * 64 + 256 * 256 + 288 * 288 + 1024 * 1024)
    check_plan(dspfx, 1637, RAGGED + [1637], group_start=RAGGED + [1637])
    assert dspfx.MIXMATRIX_MAX_ROOM == 1024 and (dspfx.MIXMATRIX_MIX_MINUS, dspfx.MIXMATRIX_ZERO) == (0, 1)


BAD = {
    "decreasing": dict(channels=8, group_start=[0, 6, 4, 8]),
    "not_from_zero": dict(channels=8, group_start=[1, 4, 8]),
    "not_to_n": dict(channels=8, group_start=[0, 4, 7]),
    "above_1024": dict(channels=2048, group_start=[0, 1025, 2048]),
    "empty_room": dict(channels=8, group_start=[0, 4, 4, 8]),
    "tile_not_pow2": dict(channels=96, group_size=32, tile_channels=48),
    "tile_not_dividing": dict(channels=96, group_size=32, tile_channels=64),
    "abi_version": dict(channels=8, group_size=4, abi_version=1),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_descriptor_is_refused_before_the_device(dspfx, case):
    """No GPU here: a bad descriptor still gets DSPFX_ERR_INVALID and a reason, so the checks come before any device work."""
    with pytest.raises(dspfx.DspfxError) as e:
        dspfx.MixMatrix(**BAD[case])
    assert e.value.status == -1, e.value
    reason = dspfx.lib().dspfx_mixmatrix_last_error(None).decode()
    assert reason.startswith("mixmatrix:") and len(reason) > len("mixmatrix:") and reason in str(e.value)


def test_invalid_descriptor_leaves_no_handle(dspfx):
    L = dspfx.lib()
    table = (C.c_uint64 * 3)(0, 4, 4)
    d = dspfx._MixMatrixDesc(dspfx.ABI_VERSION, 0, 4, 128, 0, 2, 1, table)
    h = C.c_void_p(0xDEAD)
    assert L.dspfx_mixmatrix_create(C.byref(d), C.byref(h)) == -1
    assert not h.value
    assert L.dspfx_mixmatrix_last_error(None).decode()
    for k in BAD:                                         # the plan refuses what create refuses in a table
        if k != "abi_version":
            with pytest.raises(dspfx.DspfxError):
                dspfx.mixmatrix_plan(**BAD[k])


def test_mix_minus_is_the_returns_definition():
    """A mix-minus matrix in float64 is mixreturns_ref's definition -- the sum of the others over link_divisor(n - 1) -- within
    both references' bounds (they differ only by float64 rounding)."""
    rng = np.random.default_rng(5)
    x = (rng.uniform(-1.0, 1.0, (9, 1636)) + 0.25).astype(np.float32)
    for normalise in (True, False):
        ref, sabs, n_of = X.exact(x, RAGGED, X.mix_minus(RAGGED), normalise)
        rref, rsabs = M.returns_exact(x, RAGGED, None, normalise)
        err = np.abs(ref - rref)
        assert (err <= X.bound(sabs, n_of)).all() and (err <= R.bound(rsabs, rref, 1.0)).all()
        assert (ref[:, 0] == 0).all()                     # a room of one: no other pipe


@pytest.mark.parametrize("normalise", [True, False])
def test_the_bound_holds_for_float32_in_two_orders(normalise):
    rng = np.random.default_rng(6)
    table = [0, 1, 3, 34, 66, 99, 355]
    x = (rng.uniform(-1.0, 1.0, (5, 355)) + 0.25).astype(np.float32)
    mats = X.random_mats(table, 8)
    mats[5][7, :] = 0.0                                   # a listener without a wire
    ref, sabs, n_of = X.exact(x, table, mats, normalise)
    bnd = X.bound(sabs, n_of)
    outs = [X.eval_f32(x, table, mats, normalise, order) for order in ("ascending", "pairwise")]
    assert (outs[0] != outs[1]).any(), "the two orders are different roundings"
    for got in outs:
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= bnd).all(), float((err / bnd).max())
        assert (got[:, 99 + 7].view(np.uint32) == 0).all()
