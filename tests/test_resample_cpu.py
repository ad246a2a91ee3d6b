"""The output resampler bank, the parts that need no GPU: the ABI and its mirrors, dspfx_resample_plan (a pure host function)
against the numpy restatement in resample_ref.py bit for bit, the frames pulled per callback, a cross-check of the f32
restatement against the f64 one the IR loader uses (ir.resample_dasp_sinc), and the ring's 16th tap."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
HPP = open(os.path.join(ROOT, "include", "dspfx.hpp")).read()
FFI = open(os.path.join(ROOT, "host", "rust", "src", "ffi.rs")).read()
ENGINE_RS = open(os.path.join(ROOT, "host", "rust", "src", "engine.rs")).read()
NEW = {"dspfx_resample_create": 2, "dspfx_resample_destroy": 1, "dspfx_resample_push": 4, "dspfx_resample_slot": 1,
       "dspfx_resample_pull": 6, "dspfx_resample_available": 1, "dspfx_resample_skip": 2, "dspfx_resample_reset": 1,
       "dspfx_resample_plan": 9}
CTYPE = {"uint32_t": C.c_uint32, "int32_t": C.c_int32}
RUST = {"uint32_t": "u32", "int32_t": "i32"}
RATES = (8000, 22050, 44100, 48000, 96000, 192000)


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _header_desc_fields():
    m = re.search(r"typedef struct dspfx_resample_desc\s*\{(.*?)\}\s*dspfx_resample_desc;", _strip_comments(HDR), re.S)
    assert m
    return [tuple(d.split()) for d in m.group(1).split(";") if d.strip()]


def test_entry_points_declared_listed_and_exported(dspfx):
    protos = {m.group(1): len(m.group(2).split(","))
              for m in re.finditer(r"\b(dspfx_\w+)\s*\(([^;{}]*?)\)\s*;", _strip_comments(HDR))}
    for name, arity in NEW.items():
        assert protos.get(name) == arity, name
        assert name in dspfx.EXPORTS, name
    L = C.CDLL(dspfx.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
    assert "AS RECALLED, UNPINNED" in HDR[HDR.index("output resampler bank"):]


def test_mirrors_match_the_header(dspfx):
    fields = _header_desc_fields()
    assert [f[1] for f in fields] == ["abi_version", "device", "channels", "tile_channels", "block_frames", "slots", "target_hz",
                                      "out_format", "out_channels"]
    py = dspfx._ResampleDesc._fields_
    assert [f[0] for f in py] == [f[1] for f in fields]
    assert [t for _, t in py] == [CTYPE[f[0]] for f in fields]
    assert C.sizeof(dspfx._ResampleDesc) == 36
    assert "#define DSPFX_RESAMPLE_MAX_FRAMES 4096" in HDR and dspfx.RESAMPLE_MAX_FRAMES == 4096
    ffi = _strip_comments(FFI)
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct dspfx_resample_desc\s*\{(.*?)\}", ffi, re.S)
    assert m, "dspfx_resample_desc is not a #[repr(C)] struct in ffi.rs"
    got = [f.strip().replace("pub ", "") for f in m.group(1).split(",") if f.strip()]
    assert got == [f"{n}: {RUST[t]}" for t, n in fields], got
    for name, arity in NEW.items():
        m = re.search(r"pub fn %s\s*\(([^)]*)\)" % name, ffi)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == arity, name
    rs = _strip_comments(ENGINE_RS)
    assert "pub struct Resampler" in rs and "impl Drop for Resampler" in rs
    for name in NEW:
        if name != "dspfx_resample_plan":
            assert name + "(" in rs, name
        assert name + "(" in HPP, name
    assert "class Resampler" in HPP


def _n_out_for(hz):
    """the callback length the issue's figures use: the shortest one whose input_len is 128 (8 kHz: 21 frames, input_len 126)"""
    return 21 if hz == 8000 else next(n for n in range(1, 4096) if R.input_len(n, hz) == 128)


@pytest.mark.parametrize("hz", RATES)
def test_plan_equals_the_restatement_bit_for_bit(dspfx, hz):
    n_out = _n_out_for(hz)
    ref = R.Resampler(1, hz)
    value, idx = 0.0, 0
    for cb in range(60):
        rows = ref.plan(n_out)
        p = dspfx.resample_plan(hz, value, idx, n_out)
        value, idx = p["value"], p["idx"]
        assert p["input_len"] == R.input_len(n_out, hz)
        assert p["pulled"] == sum(r[0] for r in rows)
        assert [r[0] for r in rows] == p["advance"].tolist(), cb
        assert [r[1] for r in rows] == p["depth"].tolist(), cb
        want = np.array([[c for _, c in r[2]] + [0.0] * (16 - 2 * r[1]) for r in rows], np.float64)
        assert np.array_equal(want.view(np.uint64), p["coeff"].view(np.uint64)), cb       # bit for bit: the same C library
        assert np.float64(value).tobytes() == np.float64(ref.value).tobytes() and idx == ref.idx, cb


def test_frames_pulled_per_callback(dspfx):
    """the counts the restatement gives on the CPU: input_len + 1 really occurs, so the interface reports the count"""
    want = {44100: [127, 128, 129, 128, 129, 128], 22050: [126, 128, 129, 128, 129, 128], 48000: [127] + [128] * 5,
            96000: [127] + [128] * 5, 192000: [127] + [128] * 5, 8000: [120] + [126] * 5}
    for hz, counts in want.items():
        n_out = _n_out_for(hz)
        assert R.input_len(n_out, hz) == (126 if hz == 8000 else 128)
        value, idx, got = 0.0, 0, []
        ref = R.Resampler(2, hz)
        x = np.zeros((4096, 2), np.float32)
        for cb in range(6):
            p = dspfx.resample_plan(hz, value, idx, n_out)
            value, idx = p["value"], p["idx"]
            got.append(p["pulled"])
            assert ref.callback(x, n_out)[1] == p["pulled"]
        assert got == counts, (hz, got)


def test_plan_argument_errors(dspfx):
    for args in ((0, 0.0, 0, 4), (44100, 0.0, 0, 4097), (44100, 0.0, 9, 4), (44100, -1.0, 0, 4), (44100, float("nan"), 0, 4)):
        with pytest.raises(dspfx.DspfxError) as ei:
            dspfx.resample_plan(*args)
        assert ei.value.status == -1   # DSPFX_ERR_INVALID
    v, i = C.c_double(0.5), C.c_uint32(3)                        # the arrays are optional: only the state is stepped
    assert dspfx.lib().dspfx_resample_plan(44100, C.byref(v), C.byref(i), 10, None, None, None, None, None) == 0
    p = dspfx.resample_plan(44100, 0.5, 3, 10)
    assert (v.value, i.value) == (p["value"], p["idx"])


def test_f32_restatement_against_the_f64_one():
    """ir.resample_dasp_sinc is the same state machine over f64 frames: fed the same x in one long callback, the two differ
    only by the f32 rounding of 16 products and 16 sums per output."""
    from dsp_stuff_amd import ir
    rng = np.random.default_rng(1)
    x = rng.uniform(-1.0, 1.0, 4000).astype(np.float32)
    y64 = ir.resample_dasp_sinc(x.astype(np.float64), 48000, 44100)
    n = len(y64) - 40                                            # short of the end: the callback needs input_len frames waiting
    out, used = R.Resampler(1, 44100).callback(x[:, None], n)
    assert out is not None and used > 3900
    unit = 16 * 2.0 ** -24 * float(np.abs(x).max())
    worst = float(np.abs(out[:, 0].astype(np.float64) - y64[:n]).max()) / unit
    print(f"f32 vs f64 restatement: {worst:.3f} x 16 * 2^-24 * max|x|")
    assert worst <= 0.64                                         # observed here: 0.320; the bound is twice that


def test_the_sixteenth_tap_reads_the_oldest_frame(dspfx):
    """In steady state nl = 8, nr = 9 and the last right tap is ring[(9 + 7) % 16] = ring[0]: the OLDEST frame, not the one
    after the newest.  44.1 kHz shows it (at 48 kHz the phase is always 0 and that coefficient is about 1e-17)."""
    p = dspfx.resample_plan(44100, 0.0, 0, 30)
    rows = R.Resampler(1, 44100).plan(30)
    for o in (20, 21, 22):
        assert p["depth"][o] == 8 and len(rows[o][2]) == 16
        k, c = rows[o][2][-1]
        assert k == 0
        assert c == p["coeff"][o][15] and -7e-4 <= c <= -2e-4, c
    # an input that is non-zero only in the oldest frame of the window of output 21
    pulled = int(p["advance"][:22].sum())
    x = np.zeros((64, 1), np.float32)
    x[pulled - 16] = np.float32(0.75)
    out, _ = R.Resampler(1, 44100).callback(x, 30)
    want = np.float32(p["coeff"][21][15] * np.float64(np.float32(0.75)))
    assert out[21, 0] == want and want != 0
