"""The output resampler bank on the GPU on edge values, against the numpy restatement in resample_ref.py: the edge block through
every device format; its neighbours; one infinity pair and one NaN leaving with the 16-frame ring, from the window the steady
kernel holds for one call and from the ring kept in memory between calls; a stream of subnormals.  The streams, and what the
restatement makes of them, are in test_edge_output_banks_cpu.py; the restatement of a stream is computed once there and replayed
to every Pair that is fed that stream.

Shapes (N, tile, DSPFX_RESAMPLE_VEC) = (96, 32, "1"), four channels a lane, and (77, 0, "1"), one; rates 44100, 96000 and 8000.
Integer formats are compared by raw bytes.  F32 is compared by bits wherever the restatement is not NaN, and by the isnan
pattern: the sign and payload of a NaN differ between x86 and the GPU."""
import numpy as np
import pytest

import resample_ref as R
from edge_values import classes_present, is_subnormal, same_bits_or_nan, same_values
from test_edge_output_banks_cpu import (POISON_PLACES, RS_CALLBACKS, RS_RATES, RS_SHAPES, SUB_NEG0, Replay, f32_layout, n_outs_of,
                                        outputs_of, per_of, poison_case, resample_edge_case, subnormal_case)
from test_resample_gpu import F32, I16, I32, NP_OUT, U16, Pair, expected_bytes, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def strict(table=None):
    """the comparison of a pull for every format: F32 by same_values at bar 0 plus bit equality off NaN, the rest by bytes"""

    def compare(p, got, want):
        what = f"pull {p.pulls} ({len(want)} frames)"
        if p.fmt == F32:
            g, e = got.view(np.float32), f32_layout(p.dspfx, want, p.tile)
            same_values(g, e, 0, what=what)
            same_bits_or_nan(g, e, what=what)
        else:
            exp = expected_bytes(p.dspfx, want, p.tile, p.fmt, p.ch)
            bad = np.nonzero(got != exp)[0]
            assert not len(bad), f"{what}: {len(bad)} bytes differ, first at {bad[0]}"

    return compare


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def device_frames(p, got, n_out):
    """the bytes of a pull -> [n_out][N] in the format's dtype, the first device channel of each frame"""
    flat = got.view(NP_OUT[p.fmt]).reshape(-1, p.ch)[:, 0]
    return p.dspfx.from_layout(np.ascontiguousarray(flat), n_out, p.n, p.tile)


@pytest.mark.parametrize("fmt,ch", [(F32, 1), (I16, 1), (I16, 2), (U16, 1), (I32, 1)])
@pytest.mark.parametrize("hz", RS_RATES)
@pytest.mark.parametrize("n,tile,vec", RS_SHAPES)
def test_edge_block_in_every_format(dspfx, torch_cuda, monkeypatch, n, tile, vec, hz, fmt, ch):
    """edge_block(N, 24 * 128, level=1.0) (with its non-finite samples once more, negated: resample_edge_case) through 40
    callbacks of the lengths of test_stream_of_callbacks_is_bit_identical.  The restatement's f32 output holds NaN, both
    infinities and subnormals, so the f64 product rounded once into the subnormals, the 16 additions with infinite and NaN terms
    and from_f32 of all of them are what is compared; the integer outputs hold both saturation values, and a NaN is 0 (0x8000
    for U16) on the device."""
    monkeypatch.setenv("DSPFX_RESAMPLE_VEC", vec)
    x, plain, table, rows, _ = resample_edge_case(n, hz)
    assert {"nan", "+inf", "-inf", "subnormal"} <= classes_present(outputs_of(rows))
    seen = {"lo": False, "hi": False, "nan": 0}
    inner = strict()

    def compare(p, got, want):
        inner(p, got, want)
        if fmt != F32:
            dev = device_frames(p, got, len(want))
            info = np.iinfo(NP_OUT[fmt])
            seen["lo"] |= bool((dev == info.min).any())
            seen["hi"] |= bool((dev == info.max).any())
            nan = np.isnan(want)
            assert (dev[nan] == (0x8000 if fmt == U16 else 0)).all()
            seen["nan"] += int(nan.sum())

    p = Pair(dspfx, torch_cuda, n, hz, tile, fmt, ch, compare=compare)
    p.ref = Replay(rows)
    pushed = stream(p, x, n_outs_of(hz), RS_CALLBACKS)
    assert p.pulls == RS_CALLBACKS and pushed == len(x)
    if fmt != F32:
        assert seen["lo"] and seen["hi"] and seen["nan"] >= 10, seen


@pytest.mark.parametrize("fmt,ch", [(F32, 1), (I16, 2)])
@pytest.mark.parametrize("hz", RS_RATES)
@pytest.mark.parametrize("n,tile,vec", RS_SHAPES)
def test_edge_channels_change_no_neighbour(dspfx, torch_cuda, monkeypatch, n, tile, vec, hz, fmt, ch):
    """Every channel outside the table has the bytes of the same stream with plain noise in the edge channels (the restatement
    of that plain stream: finite everywhere, so bytes in F32 too).  In the four-channel kernel the classes share lanes with each
    other and, at the table's ends, with innocent channels."""
    monkeypatch.setenv("DSPFX_RESAMPLE_VEC", vec)
    x, plain, table, rows, rows_plain = resample_edge_case(n, hz)
    others = np.asarray([c for c in range(n) if c not in table])
    wants = iter(rows_plain)
    checked = [0]

    def compare(p, got, want):
        clean, _, _ = next(wants)
        if clean is None:
            clean = np.zeros_like(want)
        dev = device_frames(p, got, len(want))
        exp = R.to_device(clean, fmt, 1)
        assert np.array_equal(raw(dev[:, others]), raw(exp[:, others])), f"pull {p.pulls}"
        checked[0] += dev[:, others].size

    p = Pair(dspfx, torch_cuda, n, hz, tile, fmt, ch, compare=compare)
    p.ref = Replay(rows)
    stream(p, x, n_outs_of(hz), RS_CALLBACKS)
    assert checked[0] >= 12 * len(others)


@pytest.mark.parametrize("fmt", [F32, I32])
@pytest.mark.parametrize("place", POISON_PLACES)
@pytest.mark.parametrize("hz", RS_RATES)
@pytest.mark.parametrize("n,tile,vec", RS_SHAPES)
def test_poison_leaves_with_the_ring(dspfx, torch_cuda, monkeypatch, n, tile, vec, hz, place, fmt):
    """One inf, -inf pair in channel 1 and one NaN in channel 2, inside one callback's input (poison_case): `inside`, they leave
    the 16-frame window within the pull that met them, which the steady kernel holds in f64 registers; `carried`, the call ends
    while they are in the ring, so the ring saved in memory hands them to the next call, which has to let them go; `warm`, they
    sit in the first 8 frames after create, in the warm-up kernel.  test_poison_leaves_the_restatement_with_the_ring shows that
    the restatement is finite and equal to the clean stream from the first output whose ring is free of them; here the device
    equals the restatement through all six callbacks, and its output after that point is that of the clean stream."""
    monkeypatch.setenv("DSPFX_RESAMPLE_VEC", vec)
    x, clean, rows, rows_clean, where, pulled = poison_case(n, hz, place)
    last = max(b for _, b in where.values())
    inner = strict()
    k = [0]
    free = [0]

    def compare(p, got, want):
        inner(p, got, want)
        gone = pulled[k[0]] - R.TAPS > last
        dev = device_frames(p, got, len(want))
        exp = R.to_device(rows_clean[k[0]][0], fmt, 1)
        assert np.array_equal(raw(dev[gone]), raw(exp[gone])), f"pull {k[0]}"
        free[0] += int(gone.sum())
        k[0] += 1

    p = Pair(dspfx, torch_cuda, n, hz, tile, fmt, 1, compare=compare)
    p.ref = Replay(rows)
    stream(p, x, [per_of(hz)], 6)
    assert p.pulls == 6 and free[0] >= 2 * per_of(hz)


@pytest.mark.parametrize("hz", RS_RATES)
@pytest.mark.parametrize("n,tile,vec", RS_SHAPES)
def test_subnormal_stream_is_not_flushed(dspfx, torch_cuda, monkeypatch, n, tile, vec, hz):
    """Every channel carries k 2^-149, |k| <= 512; one is all -0.0, one alternates +-FLT_MAX, one is +-FLT_MAX constant
    (subnormal_case).  No NaN arises, so F32 is compared by bytes: every f64 product is rounded once to a subnormal f32 and the
    sums stay subnormal; more than half of the restatement's non-zero outputs are subnormal; the -0.0 channel reads +0.0 bits
    (the sum starts from +0.0); the constant channel's sum overflows to an infinity in f32 wherever the phase is not 0."""
    monkeypatch.setenv("DSPFX_RESAMPLE_VEC", vec)
    x, rows = subnormal_case(n, hz)
    out = outputs_of(rows)
    nz = out[out != 0]
    assert not np.isnan(out).any() and is_subnormal(nz).mean() > 0.5 and (out[:, SUB_NEG0].view(np.uint32) == 0).all()
    zeros = [0]

    def compare(p, got, want):
        exp = expected_bytes(p.dspfx, want, p.tile, F32, 1)
        bad = np.nonzero(got != exp)[0]
        assert not len(bad), f"pull {p.pulls}: {len(bad)} bytes differ, first at {bad[0]}"
        dev = device_frames(p, got, len(want))
        assert (dev[:, SUB_NEG0].view(np.uint32) == 0).all()
        zeros[0] += len(want)

    p = Pair(dspfx, torch_cuda, n, hz, tile, F32, 1, compare=compare)
    p.ref = Replay(rows)
    stream(p, x, n_outs_of(hz), 10)
    assert p.pulls == 10 and zeros[0] >= len(out)
