"""Device sample formats at the process boundary (dspfx_process_pcm / dspfx_process_host_pcm), the parts that need no GPU: the
ABI and its mirrors (EXPORTS, the built library, host/rust/src/ffi.rs and engine.rs) and known answers of the numpy
restatement the GPU tests compare against."""
import ctypes as C
import os
import re

import numpy as np

from pcm_ref import F32, I16, I32, U16, narrow_np, widen_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
FFI = open(os.path.join(ROOT, "host", "rust", "src", "ffi.rs")).read()
ENGINE_RS = open(os.path.join(ROOT, "host", "rust", "src", "engine.rs")).read()
NEW = ("dspfx_process_pcm", "dspfx_process_host_pcm")


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _c_protos():
    out = {}
    for m in re.finditer(r"\b(dspfx_\w+)\s*\(([^;{}]*?)\)\s*;", _strip_comments(HDR)):
        out[m.group(1)] = len(m.group(2).split(","))
    return out


def test_entry_points_declared_listed_and_exported(dspfx):
    protos = _c_protos()
    assert protos.get("dspfx_process_pcm") == 8 and protos.get("dspfx_process_host_pcm") == 7, protos
    for name in NEW:
        assert name in dspfx.EXPORTS, name
    L = C.CDLL(dspfx.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name


def test_header_format_enum_and_io_struct():
    body = _strip_comments(HDR)
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(DSPFX_SAMPLE_[A-Z0-9]+)\s*=\s*(\d+)", body)}
    assert consts == {"DSPFX_SAMPLE_F32": 0, "DSPFX_SAMPLE_I16": 1, "DSPFX_SAMPLE_U16": 2, "DSPFX_SAMPLE_I32": 3}
    m = re.search(r"typedef struct dspfx_pcm_io\s*\{(.*?)\}\s*dspfx_pcm_io;", body, re.S)
    assert m
    fields = [d.split() for d in m.group(1).split(";") if d.strip()]
    assert fields == [["int32_t", "in_format"], ["int32_t", "in_channels"], ["int32_t", "out_format"], ["int32_t", "out_channels"]]


def test_python_mirror(dspfx):
    assert (dspfx.SAMPLE_F32, dspfx.SAMPLE_I16, dspfx.SAMPLE_U16, dspfx.SAMPLE_I32) == (0, 1, 2, 3)
    assert [f[0] for f in dspfx._PcmIo._fields_] == ["in_format", "in_channels", "out_format", "out_channels"]
    assert C.sizeof(dspfx._PcmIo) == 16


def test_rust_mirror():
    ffi = _strip_comments(FFI)
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct dspfx_pcm_io\s*\{(.*?)\}", ffi, re.S)
    assert m, "dspfx_pcm_io is not a #[repr(C)] struct in ffi.rs"
    fields = [f.strip().replace("pub ", "") for f in m.group(1).split(",") if f.strip()]
    assert fields == ["in_format: i32", "in_channels: i32", "out_format: i32", "out_channels: i32"], fields
    for k, v in (("F32", 0), ("I16", 1), ("U16", 2), ("I32", 3)):
        assert re.search(r"pub const DSPFX_SAMPLE_%s: i32 = %d;" % (k, v), ffi), k
    for name, arity in (("dspfx_process_pcm", 8), ("dspfx_process_host_pcm", 7)):
        m = re.search(r"pub fn %s\s*\(([^)]*)\)" % name, ffi)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == arity, name


def test_rust_engine_calls_the_host_entry_point():
    src = re.sub(r'"(?:[^"\\]|\\.)*"', '""', _strip_comments(ENGINE_RS))
    m = re.search(r"\bdspfx_process_host_pcm\s*\(", src)
    assert m, "engine.rs does not call dspfx_process_host_pcm"
    depth, k = 1, m.end()
    while depth:
        depth += {"(": 1, ")": -1}.get(src[k], 0)
        k += 1
    args, d, n = src[m.end():k - 1], 0, 1
    for ch in args:
        d += {"(": 1, "[": 1, "{": 1, ")": -1, "]": -1, "}": -1}.get(ch, 0)
        n += ch == "," and d == 0
    assert n == 7, args
    assert "pub fn process_host_pcm" in src
    for t in ("f32", "i16", "u16", "i32"):
        assert re.search(r"impl PcmSample for %s\b" % t, src), t


def test_known_answers_widen():
    assert widen_np(np.array([-32768, 32767, 0], np.int16), I16).tolist() == [-1.0, 0.999969482421875, 0.0]
    assert widen_np(np.array([0, 32768, 65535], np.uint16), U16).tolist() == [-1.0, 0.0, 0.999969482421875]
    i32 = widen_np(np.array([2**31 - 1, -2**31, 2**24 + 1, 2**24 + 3], np.int32), I32)
    assert i32.dtype == np.float32
    # 2^31 - 1 rounds up to 2^31; the ties round to even
    assert i32.tolist() == [1.0, -1.0, 2.0**24 / 2**31, (2.0**24 + 4) / 2**31]
    pair = widen_np(np.array([[16384, 16384, -32768, 32767]], np.int16), I16, 2)
    assert pair.tolist() == [[1.0, np.float32(-1.0) + np.float32(32767 / 32768)]]     # a + b, no halving
    assert widen_np(np.array([0.25, -2.0], np.float32), F32).tolist() == [0.25, -2.0]


def test_known_answers_narrow():
    x = np.array([1.0, -1.0, 0.99999, -1e-5, np.nan, np.inf, -np.inf, 0.0, -0.0], np.float32)
    assert narrow_np(x, I16).tolist() == [32767, -32768, 32767, 0, 0, 32767, -32768, 0, 0]
    assert narrow_np(x, U16).tolist() == [65535, 0, 65535, 32768, 32768, 65535, 0, 32768, 32768]
    # f32(0.99999) * 2^31 is an integer (24-bit mantissa); f32(-1e-5) * 2^31 = -21474.83... truncates to -21474
    assert narrow_np(x, I32).tolist() == [2147483647, -2147483648, 2147462144, -21474, 0, 2147483647, -2147483648, 0, 0]
    # truncation toward zero at +-0.5 LSB and +-1.5 LSB
    lsb = np.array([0.5, -0.5, 1.5, -1.5], np.float32) / np.float32(32768)
    assert narrow_np(lsb, I16).tolist() == [0, 0, 1, -1]
    assert narrow_np(np.array([0.5], np.float32), I16, 2).tolist() == [16384, 16384]
    assert narrow_np(np.array([1.0], np.float32), I32).dtype == np.int32
    assert narrow_np(np.array([1.0], np.float32), I32).tolist() == [2147483647]


def test_argument_checks_without_a_device(dspfx):
    """With no engine to act on (nothing can be created without a GPU), both entry points refuse at once -- a NULL engine,
    a NULL io, a format of 4 or a channel count of 3 never reach a HIP call."""
    L = dspfx.lib()
    buf = (C.c_float * 4)()
    for io in (None, dspfx._PcmIo(4, 1, 0, 1), dspfx._PcmIo(0, 3, 0, 1), dspfx._PcmIo(0, 1, 0, 3)):
        p = C.byref(io) if io is not None else None
        assert L.dspfx_process_pcm(None, p, buf, None, buf, None, 1, None) == -1
        assert L.dspfx_process_host_pcm(None, p, buf, None, buf, None, 1) == -1
