"""The convolver bank, the parts that need no GPU: the ABI and its mirrors, the descriptor checks that run before any device
work, dspfx_convolve_plan (a pure host function: the f32 response table exactly as the device gets it) against numpy's f64
rfft of the zero-padded partitions, and the float32 restatement in convolve_ref.py against the exact convolution."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import convolve_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
HPP = open(os.path.join(ROOT, "include", "dspfx.hpp")).read()
FFI = open(os.path.join(ROOT, "host", "rust", "src", "ffi.rs")).read()
NEW = {"dspfx_convolve_create": 2, "dspfx_convolve_destroy": 1, "dspfx_convolve_reset": 1, "dspfx_convolve_run": 5,
       "dspfx_convolve_set_taps": 4, "dspfx_convolve_plan": 4}
FIELDS = [("uint32_t", "abi_version"), ("int32_t", "device"), ("uint32_t", "channels"), ("uint32_t", "tile_channels"),
          ("uint32_t", "n_taps"), ("uint32_t", "max_taps"), ("int32_t", "mode"), ("const double *", "taps_reversed")]
CTYPE = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "const double *": C.POINTER(C.c_double)}
RUST = {"uint32_t": "u32", "int32_t": "i32", "const double *": "*const f64"}
INVALID, NO_DEVICE = -1, -2
MAX_TAPS = 524288


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _header_desc_fields():
    m = re.search(r"typedef struct dspfx_convolve_desc\s*\{(.*?)\}\s*dspfx_convolve_desc;", _strip_comments(HDR), re.S)
    assert m, "include/dspfx.h has no dspfx_convolve_desc"
    out = []
    for d in m.group(1).split(";"):
        if d.strip():
            t, name = re.match(r"\s*(.*?)(\w+)\s*$", d, re.S).groups()
            out.append((" ".join(t.split()), name))
    return out


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_entry_points_declared_listed_and_exported(dspfx):
    protos = {m.group(1): len(m.group(2).split(","))
              for m in re.finditer(r"\b(dspfx_\w+)\s*\(([^;{}]*?)\)\s*;", _strip_comments(HDR))}
    for name, arity in NEW.items():
        assert protos.get(name) == arity, name
        assert name in dspfx.EXPORTS, name
    L = C.CDLL(dspfx.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
    section = HDR[HDR.index("convolver bank"):]
    assert "(P_max + 2) * 1024 * channels" in section and "P_max * 1024 of table" in section      # the allocation is stated
    assert "FILL PHASE" in section and "NOT restated" in section
    assert re.search(r"#define DSPFX_ABI_VERSION\s+2\b", HDR) and dspfx.ABI_VERSION == 2


def test_mirrors_match_the_header(dspfx):
    fields = _header_desc_fields()
    assert fields == FIELDS
    py = dspfx._ConvolveDesc._fields_
    assert [f[0] for f in py] == [name for _, name in fields]
    assert [t for _, t in py] == [CTYPE[t] for t, _ in fields]
    assert C.sizeof(dspfx._ConvolveDesc) == 40 and dspfx._ConvolveDesc.taps_reversed.offset == 32
    assert "#define DSPFX_CONVOLVE_MAX_TAPS %d" % MAX_TAPS in HDR and dspfx.CONVOLVE_MAX_TAPS == MAX_TAPS
    ffi = _strip_comments(FFI)
    assert "pub const DSPFX_CONVOLVE_MAX_TAPS: u32 = %d;" % MAX_TAPS in ffi
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct dspfx_convolve_desc\s*\{(.*?)\}", ffi, re.S)
    assert m, "dspfx_convolve_desc is not a #[repr(C)] struct in ffi.rs"
    got = [f.strip().replace("pub ", "") for f in m.group(1).split(",") if f.strip()]
    assert got == [f"{n}: {RUST[t]}" for t, n in fields], got
    for name, arity in NEW.items():
        m = re.search(r"pub fn %s\s*\(([^)]*)\)" % name, ffi)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == arity, name
    src = os.path.join(ROOT, "host", "rust", "src")
    rs = _strip_comments(open(os.path.join(src, "convolver.rs")).read())
    assert "pub struct Convolver" in rs and "impl Drop for Convolver" in rs
    assert "pub mod convolver;" in open(os.path.join(src, "mod.rs")).read()
    for name in NEW:
        assert name + "(" in rs, name
        assert name + "(" in HPP, name
    # every call convolver.rs makes passes as many arguments as the header's prototype takes (no rustc here)
    for m in re.finditer(r"\b(dspfx_convolve_\w+)\s*\(([^()]*(?:\([^()]*\)[^()]*)*)\)", rs):
        args = [a for a in re.sub(r"\([^()]*\)", "", m.group(2)).split(",") if a.strip()]
        assert len(args) == NEW[m.group(1)], m.group(0)
    assert "class Convolver" in HPP
    for attr in ("run", "set_taps", "reset", "partitions", "from_wav"):
        assert hasattr(dspfx.Convolver, attr), attr
    assert callable(dspfx.convolve_plan)


def test_create_checks_the_descriptor_before_any_device_work(dspfx):
    """Every check of the descriptor runs before the first HIP call, so these codes come back with or without a GPU; a
    good descriptor on a host without a GPU is NO_DEVICE (asserted only where there is none)."""
    L = dspfx.lib()
    good = np.ones(1000)

    def create(abi=2, ch=64, tile=0, taps=good, n=None, max_taps=0, mode=0):
        n = (0 if taps is None else len(taps)) if n is None else n
        d = dspfx._ConvolveDesc(abi, 0, ch, tile, n, max_taps, mode, None if taps is None else _dp(taps))
        h = C.c_void_p()
        rc = L.dspfx_convolve_create(C.byref(d), C.byref(h))
        if rc == 0:
            L.dspfx_convolve_destroy(h)
        else:
            assert not h.value
        return rc

    assert create(n=0) == INVALID
    assert create(n=MAX_TAPS + 1) == INVALID                                    # rejected on the count: the taps are not read
    assert create(n=0xFFFFFFFF) == INVALID
    assert create(max_taps=999) == INVALID                                      # below n_taps
    assert create(max_taps=MAX_TAPS + 1) == INVALID
    assert create(taps=None, n=1000) == INVALID
    for bad in (np.nan, np.inf, -np.inf):
        t = good.copy()
        t[617] = bad
        assert create(taps=t) == INVALID, bad
    assert create(ch=0) == INVALID
    assert create(ch=96, tile=64) == INVALID                                    # the tile does not divide N
    assert create(ch=96, tile=3) == INVALID                                     # not a power of two
    assert create(abi=1) == INVALID
    for mode in (-1, 2, 7):
        assert create(mode=mode) == INVALID, mode
    assert L.dspfx_convolve_create(None, None) == INVALID
    assert L.dspfx_convolve_destroy(None) == INVALID and L.dspfx_convolve_reset(None) == INVALID
    assert L.dspfx_convolve_run(None, None, None, 128, None) == INVALID
    assert L.dspfx_convolve_set_taps(None, _dp(good), 1000, 0) == INVALID
    if dspfx.device_count() < 1:
        for kw in ({}, {"max_taps": 1000}, {"max_taps": 4096, "mode": 1}, {"ch": 256, "tile": 64}, {"taps": np.ones(1)}):
            assert create(**kw) == NO_DEVICE, kw
        with pytest.raises(dspfx.DspfxError) as ei:
            dspfx.Convolver(64, good)
        assert ei.value.status == NO_DEVICE
    with pytest.raises(dspfx.DspfxError) as ei:
        dspfx.Convolver(64, np.zeros(0))
    assert ei.value.status == INVALID
    with pytest.raises(dspfx.DspfxError) as ei:
        dspfx.Convolver(64, good, mode=5)
    assert ei.value.status == INVALID


def test_plan_argument_errors(dspfx):
    L = dspfx.lib()
    parts = C.c_uint32(77)
    good = np.ones(300)
    assert L.dspfx_convolve_plan(None, 300, C.byref(parts), None) == INVALID
    assert L.dspfx_convolve_plan(_dp(good), 0, C.byref(parts), None) == INVALID
    assert L.dspfx_convolve_plan(_dp(good), MAX_TAPS + 1, C.byref(parts), None) == INVALID
    bad = good.copy()
    bad[0] = np.nan
    assert L.dspfx_convolve_plan(_dp(bad), 300, C.byref(parts), None) == INVALID
    assert parts.value == 77                                                    # untouched by a refused call
    assert L.dspfx_convolve_plan(_dp(good), 300, None, None) == 0               # both outputs are optional
    assert L.dspfx_convolve_plan(_dp(good), 300, C.byref(parts), None) == 0 and parts.value == 3
    with pytest.raises(dspfx.DspfxError):
        dspfx.convolve_plan(np.zeros(0))
    with pytest.raises(dspfx.DspfxError):
        dspfx.convolve_plan([1.0, np.inf])


@pytest.mark.parametrize("T", sorted(R.PARTS))
def test_plan_is_the_f64_transform_rounded_once(dspfx, T):
    """Every table entry lies within 2^-24 |ref| + 2^-40 ||h_p||_1 of numpy's float64 rfft of the zero-padded partition: the
    first term is the one rounding to f32, the second bounds what a 256-point f64 transform can err (each of its 128 terms is
    within a few 2^-53 of |h|, far below 2^-40 of their sum)."""
    h = R.response(T, seed=T)
    P, table = dspfx.convolve_plan(h)
    assert P == R.PARTS[T] == R.partitions(T)
    assert table.dtype == np.float32 and table.shape == (128, P, 2)
    ref = R.table_f64(h)                                                        # [128, P] complex128
    l1 = R.partition_l1(h)[None, :]
    for part, want in ((table[:, :, 0], ref.real), (table[:, :, 1], ref.imag)):
        assert np.all(np.abs(part.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 2.0 ** -40 * l1)
    # the packed element 0 is (DC, Nyquist)
    hp = np.zeros(P * 128)
    hp[:T] = h
    hp = hp.reshape(P, 128)
    dc, ny = hp.sum(axis=1), (hp * (-1.0) ** np.arange(128)).sum(axis=1)
    assert np.allclose(table[0, :, 0], dc, rtol=2.0 ** -23, atol=2.0 ** -40 * l1.max())
    assert np.allclose(table[0, :, 1], ny, rtol=2.0 ** -23, atol=2.0 ** -40 * l1.max())


def test_plan_of_a_unit_impulse(dspfx):
    for T in (1, 128, 300):
        h = np.zeros(T)
        h[0] = 1.0
        P, table = dspfx.convolve_plan(h)
        assert P == R.partitions(T)
        assert np.all(table[:, 0, 0] == 1.0)                                    # ones in partition 0 ...
        assert np.all(table[1:, 0, 1] == 0.0) and table[0, 0, 1] == 1.0         # ... purely real; element 0 is (DC, Nyquist) = (1, 1)
        assert not table[:, 1:].any()                                           # zeros elsewhere
    # a delay of d < 128 frames is the phase ramp, and of 128 p frames a one in partition p
    h = np.zeros(300)
    h[256] = 1.0
    _, table = dspfx.convolve_plan(h)
    assert np.all(table[:, 2, 0] == 1.0) and not table[:, :2].any()
    h = np.zeros(64)
    h[32] = 1.0                                                                 # exp(-2 pi i k 32 / 256) = (-i)^(k / 2) at even k
    _, table = dspfx.convolve_plan(h)
    assert table[4, 0].tolist() == [-1.0, 0.0] and table[2, 0].tolist() == [0.0, -1.0] and table[0, 0].tolist() == [1.0, 1.0]


def test_restatement_meets_the_bar_it_is_printed_beside():
    """convolve_ref itself: the float32 restatement against the exact convolution, ring wrap and reload included."""
    T, N = 1000, 3
    h = R.response(T)
    x = R.noise((2 * 8 + 3) * 128, N)
    want = R.exact(x, h)
    got = R.Partitioned(N, h).run_all(x)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert R.rel_rms(got, want).max() < R.BAR and R.block_rms(got, want).max() < R.BAR
    # an impulse response: the exact answer is the input
    assert np.array_equal(R.exact(x, [1.0]), x.astype(np.float64))
    d = np.zeros(300)
    d[299] = 1.0
    assert np.allclose(R.exact(x, d)[299:], x[:-299].astype(np.float64), rtol=0, atol=1e-12)
    # reload keeps the history
    h2 = R.response(T, seed=1)
    bank = R.Partitioned(N, h, max_taps=4096)
    a = bank.run_all(x[:12 * 128])
    bank.set_taps(h2)
    b = bank.run_all(x[12 * 128:])
    assert R.rel_rms(a, want[:12 * 128]).max() < R.BAR
    assert R.rel_rms(b, R.exact(x, h2)[12 * 128:]).max() < R.BAR
