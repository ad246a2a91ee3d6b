"""Several responses on one convolver bank (dspfx_convolve_response_add / _response_set / _assign / _response_count), the parts
that need no GPU: the four entry points and the constant in the header and in every mirror, and the argument checks that run
before any device work."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
HPP = open(os.path.join(ROOT, "include", "dspfx.hpp")).read()
SRC = os.path.join(ROOT, "host", "rust", "src")
FFI = open(os.path.join(SRC, "ffi.rs")).read()
NEW = {"dspfx_convolve_response_add": 5, "dspfx_convolve_response_set": 5, "dspfx_convolve_assign": 4,
       "dspfx_convolve_response_count": 1}
MAX_RESPONSES = 256
INVALID = -1


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_entry_points_declared_listed_exported_and_bound(dspfx):
    protos = {m.group(1): len(m.group(2).split(","))
              for m in re.finditer(r"\b(dspfx_\w+)\s*\(([^;{}]*?)\)\s*;", _strip_comments(HDR))}
    ffi = _strip_comments(FFI)
    L = C.CDLL(dspfx.LIB_PATH)
    for name, arity in NEW.items():
        assert protos.get(name) == arity, name
        assert name in dspfx.EXPORTS, name
        assert hasattr(L, name), name
        m = re.search(r"pub fn %s\s*\(([^)]*)\)" % name, ffi)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == arity, name
        assert name + "(" in HPP, name
        assert len(getattr(dspfx.lib(), name).argtypes) == arity, name
    # the new text is in the convolver section, after what was there
    section = HDR[HDR.index("convolver bank"):]
    for name in NEW:
        assert name in section, name


def test_the_safe_rust_wrappers_are_in_their_own_file():
    assert "pub mod convolver_responses;" in open(os.path.join(SRC, "mod.rs")).read()
    rs = _strip_comments(open(os.path.join(SRC, "convolver_responses.rs")).read())
    assert "impl Convolver" in rs
    called = set()
    # every call passes as many arguments as the header's prototype takes (no rustc here)
    for m in re.finditer(r"\b(dspfx_convolve_\w+)\s*\(([^()]*(?:\([^()]*\)[^()]*)*)\)", rs):
        args = [a for a in re.sub(r"\([^()]*\)", "", m.group(2)).split(",") if a.strip()]
        assert m.group(1) in NEW, m.group(0)
        assert len(args) == NEW[m.group(1)], m.group(0)
        called.add(m.group(1))
    assert called == set(NEW)
    for fn in ("add_response", "set_response", "assign", "responses"):
        assert re.search(r"pub fn %s\s*\(" % fn, rs), fn


def test_the_constant_is_mirrored(dspfx):
    assert re.search(r"#define DSPFX_CONVOLVE_MAX_RESPONSES\s+%d\b" % MAX_RESPONSES, HDR)
    assert dspfx.CONVOLVE_MAX_RESPONSES == MAX_RESPONSES
    assert "pub const DSPFX_CONVOLVE_MAX_RESPONSES: u32 = %d;" % MAX_RESPONSES in _strip_comments(FFI)
    assert "CONVOLVE_MAX_RESPONSES = DSPFX_CONVOLVE_MAX_RESPONSES;" in _strip_comments(HPP)   # C++ takes the header's own
    kernels = open(os.path.join(ROOT, "dsp-stuff_amd", "csrc", "convolve_kernels.hip")).read()
    assert "DSPFX_CONVOLVE_MAX_RESPONSES" in kernels
    assert MAX_RESPONSES <= 1 << 16                                             # an id is a uint16_t


def test_convolver_methods_exist(dspfx):
    for attr in ("add_response", "add_wav", "set_response", "assign", "responses", "response_of"):
        assert hasattr(dspfx.Convolver, attr), attr
    assert isinstance(dspfx.Convolver.responses, property) and isinstance(dspfx.Convolver.response_of, property)
    for method in ("add_response", "set_response", "assign", "responses"):
        assert re.search(r"\b%s\s*\(" % method, HPP[HPP.index("class Convolver"):]), method


def test_argument_errors_need_no_device(dspfx):
    """The checks that need no device come first, so they answer with or without a GPU.  A bank cannot be created without one,
    so beside the NULL handle the calls get a block of zeros for a handle: a check that comes first returns before the bank
    is looked at (and a bank of zeros has no channels and takes no taps, so nothing here could go further than a refusal)."""
    L = dspfx.lib()
    good = np.ones(300)
    ids = (C.c_uint16 * 4)(0, 0, 0, 0)
    rid = C.c_uint32(77)
    assert L.dspfx_convolve_response_add(None, _dp(good), 300, 0, C.byref(rid)) == INVALID
    assert L.dspfx_convolve_response_set(None, 0, _dp(good), 300, 0) == INVALID
    assert L.dspfx_convolve_assign(None, ids, 0, 4) == INVALID
    assert L.dspfx_convolve_response_count(None) == INVALID
    zeros = C.create_string_buffer(1 << 16)
    fake = C.cast(zeros, C.c_void_p)
    nan, inf = good.copy(), good.copy()
    nan[299] = np.nan
    inf[0] = -np.inf
    for call in (lambda t, n, mode: L.dspfx_convolve_response_add(fake, t, n, mode, C.byref(rid)),
                 lambda t, n, mode: L.dspfx_convolve_response_set(fake, 0, t, n, mode),
                 lambda t, n, mode: L.dspfx_convolve_set_taps(fake, t, n, mode)):
        assert call(None, 300, 0) == INVALID                                    # null taps
        assert call(_dp(good), 0, 0) == INVALID                                 # 0 taps
        assert call(_dp(good), dspfx.CONVOLVE_MAX_TAPS + 1, 0) == INVALID       # refused on the count: the taps are not read
        assert call(_dp(nan), 300, 0) == INVALID and call(_dp(inf), 300, 1) == INVALID
        for mode in (-1, 2, 7):
            assert call(_dp(good), 300, mode) == INVALID, mode
    assert rid.value == 77                                                      # untouched by a refused call
    assert L.dspfx_convolve_assign(fake, None, 0, 4) == INVALID                 # null ids
    assert L.dspfx_convolve_assign(fake, ids, 0, 0) == INVALID                  # count == 0
    assert not any(zeros.raw)                                                   # and nothing was written through the handle
