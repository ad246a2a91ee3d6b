"""The Spectrogram bank, the parts that need no GPU: the ABI and its mirrors, dspfx_spectrum_plan (a pure host function)
against the numpy restatement in spectrum_ref.py, the descriptor checks that run before any device work, the importer's
spectrum taps, the bin range of a frequency bound, and the restatement's own bookkeeping."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import graphs
import spectrum_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
HPP = open(os.path.join(ROOT, "include", "dspfx.hpp")).read()
FFI = open(os.path.join(ROOT, "host", "rust", "src", "ffi.rs")).read()
ENGINE_RS = open(os.path.join(ROOT, "host", "rust", "src", "engine.rs")).read()
NEW = {"dspfx_spectrum_create": 2, "dspfx_spectrum_destroy": 1, "dspfx_spectrum_push": 4, "dspfx_spectrum_slot": 1,
       "dspfx_spectrum_column": 2, "dspfx_spectrum_reset": 1, "dspfx_spectrum_windows": 1, "dspfx_spectrum_plan": 3}
FIELDS = [("uint32_t", "abi_version"), ("int32_t", "device"), ("uint32_t", "channels"), ("uint32_t", "tile_channels"),
          ("uint32_t", "fft_size"), ("uint32_t", "columns"), ("const float *", "window"), ("const float *", "gain")]
CTYPE = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "const float *": C.POINTER(C.c_float)}
RUST = {"uint32_t": "u32", "int32_t": "i32", "const float *": "*const f32"}
INVALID, NO_DEVICE, UNSUPPORTED = -1, -2, -5


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _header_desc_fields():
    m = re.search(r"typedef struct dspfx_spectrum_desc\s*\{(.*?)\}\s*dspfx_spectrum_desc;", _strip_comments(HDR), re.S)
    assert m
    out = []
    for d in m.group(1).split(";"):
        if d.strip():
            t, name = re.match(r"\s*(.*?)(\w+)\s*$", d, re.S).groups()
            out.append((" ".join(t.split()), name))
    return out


def test_entry_points_declared_listed_and_exported(dspfx):
    protos = {m.group(1): len(m.group(2).split(","))
              for m in re.finditer(r"\b(dspfx_\w+)\s*\(([^;{}]*?)\)\s*;", _strip_comments(HDR))}
    for name, arity in NEW.items():
        assert protos.get(name) == arity, name
        assert name in dspfx.EXPORTS, name
    L = C.CDLL(dspfx.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
    section = HDR[HDR.index("spectrogram bank"):]
    assert "AS RECALLED, UNPINNED" in section
    assert "columns * (fft_size / 2) * channels * 4" in section               # the allocation is stated
    assert re.search(r"#define DSPFX_ABI_VERSION\s+2\b", HDR) and dspfx.ABI_VERSION == 2


def test_mirrors_match_the_header(dspfx):
    fields = _header_desc_fields()
    assert fields == FIELDS
    py = dspfx._SpectrumDesc._fields_
    assert [f[0] for f in py] == [name for _, name in fields]
    assert [t for _, t in py] == [CTYPE[t] for t, _ in fields]
    assert C.sizeof(dspfx._SpectrumDesc) == 40 and dspfx._SpectrumDesc.window.offset == 24
    assert "#define DSPFX_SPECTRUM_MIN_FFT 128" in HDR and "#define DSPFX_SPECTRUM_MAX_FFT 8192" in HDR
    assert (dspfx.SPECTRUM_MIN_FFT, dspfx.SPECTRUM_MAX_FFT) == (128, 8192)
    ffi = _strip_comments(FFI)
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct dspfx_spectrum_desc\s*\{(.*?)\}", ffi, re.S)
    assert m, "dspfx_spectrum_desc is not a #[repr(C)] struct in ffi.rs"
    got = [f.strip().replace("pub ", "") for f in m.group(1).split(",") if f.strip()]
    assert got == [f"{n}: {RUST[t]}" for t, n in fields], got
    for name, arity in NEW.items():
        m = re.search(r"pub fn %s\s*\(([^)]*)\)" % name, ffi)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == arity, name
    rs = _strip_comments(ENGINE_RS)
    assert "pub struct SpectrumBank" in rs and "impl Drop for SpectrumBank" in rs
    for name in NEW:
        assert name + "(" in rs, name
        assert name + "(" in HPP, name
    assert "class SpectrumBank" in HPP
    for attr in ("push", "slot_tensor", "column", "windows", "reset", "bins"):
        assert hasattr(dspfx.SpectrumBank, attr), attr


@pytest.mark.parametrize("n", R.SIZES)
def test_plan_equals_the_restatement(dspfx, n):
    win, hz = dspfx.spectrum_plan(n)
    assert win.dtype == np.float32 and win.shape == (n,) and hz.shape == (n // 2,)
    want = R.hann(n)
    assert np.array_equal(win.view(np.uint32), want.view(np.uint32))           # bit for bit: the same C library's cos
    assert win[0] == 0.0 and win[n - 1] == 0.0
    assert np.array_equal(win, win[::-1])
    # the mirrored half is the formula's own value there, to the rounding of one f32
    i = np.arange(n, dtype=np.float64)
    direct = 0.5 - 0.5 * np.cos(2.0 * np.pi * i / (n - 1))
    assert np.abs(win.astype(np.float64) - direct).max() <= 2.0 ** -24
    assert 0.999 < win.max() <= 1.0
    exact = np.arange(n // 2, dtype=np.float64) * 48000.0 / n
    assert np.array_equal(hz.astype(np.float64), exact)                        # k * 48000 / n is exact in f32
    assert np.array_equal(hz, R.bin_hz(n))


def test_plan_argument_errors(dspfx):
    L = dspfx.lib()
    for n, code in ((0, INVALID), (64, INVALID), (127, INVALID), (8193, INVALID), (16384, INVALID), (1 << 31, INVALID),
                    (129, UNSUPPORTED), (1000, UNSUPPORTED), (8191, UNSUPPORTED)):
        assert L.dspfx_spectrum_plan(n, None, None) == code, n
        with pytest.raises(dspfx.DspfxError) as ei:
            dspfx.spectrum_plan(n)
        assert ei.value.status == code
    assert L.dspfx_spectrum_plan(512, None, None) == 0                          # both tables are optional


def test_create_checks_the_descriptor_before_any_device_work(dspfx):
    """Every check of the descriptor runs before the first HIP call, so these codes come back with or without a GPU.
    What does need a device: a device ordinal out of range (INVALID), an allocation that fails (OOM) -- and a good
    descriptor, which on a host without a GPU is NO_DEVICE (asserted below only where there is none)."""
    L = dspfx.lib()

    def create(abi=2, ch=64, tile=0, n=512, cols=1):
        d = dspfx._SpectrumDesc(abi, 0, ch, tile, n, cols, None, None)
        h = C.c_void_p()
        rc = L.dspfx_spectrum_create(C.byref(d), C.byref(h))
        if rc == 0:
            L.dspfx_spectrum_destroy(h)
        else:
            assert not h.value
        return rc

    for n in (0, 1, 64, 127, 8193, 16384):
        assert create(n=n) == INVALID, n
    for n in (129, 500, 1000, 4095, 8191):
        assert create(n=n) == UNSUPPORTED, n
    assert create(cols=0) == INVALID
    assert create(ch=0) == INVALID
    assert create(ch=96, tile=64) == INVALID                                    # the tile does not divide N
    assert create(ch=96, tile=3) == INVALID                                     # not a power of two
    assert create(abi=1) == INVALID
    assert create(n=1000, cols=0) == INVALID                                    # INVALID wins over UNSUPPORTED
    assert L.dspfx_spectrum_create(None, None) == INVALID
    assert L.dspfx_spectrum_destroy(None) == INVALID and L.dspfx_spectrum_reset(None) == INVALID
    assert L.dspfx_spectrum_push(None, None, 128, None) == INVALID
    assert L.dspfx_spectrum_slot(None) is None and L.dspfx_spectrum_column(None, 0) is None
    assert L.dspfx_spectrum_windows(None) == INVALID
    if dspfx.device_count() < 1:
        for n in R.SIZES:
            assert create(n=n) == NO_DEVICE, n
        with pytest.raises(dspfx.DspfxError) as ei:
            dspfx.SpectrumBank(64)
        assert ei.value.status == NO_DEVICE
    with pytest.raises(ValueError):
        dspfx.SpectrumBank(64, fft_size=512, window=np.ones(511, np.float32))   # table lengths are checked on the host
    with pytest.raises(ValueError):
        dspfx.SpectrumBank(64, fft_size=512, gain=np.ones(512, np.float32))


def test_bins_of_the_default_bounds(dspfx):
    n = 512
    ks = [k for k in range(n // 2) if 20 <= k * 48000 / n <= 20000]
    assert (ks[0], ks[-1]) == (1, 213)                                          # 93.75 Hz per bin
    k_lo, k_hi, hz = dspfx.spectrum_bins(n, 20, 20000)
    assert (k_lo, k_hi) == (ks[0], ks[-1] + 1) == R.bins(n, 20, 20000)
    assert hz.tolist() == [k * 48000 / n for k in ks]
    for n in R.SIZES:
        for lo, hi in ((20, 20000), (20, 20), (0, 24000), (1000, 1200), (23999, 24000)):
            k_lo, k_hi, hz = dspfx.spectrum_bins(n, lo, hi)
            ks = [k for k in range(n // 2) if lo <= k * 48000 / n <= hi]
            assert (k_lo, k_hi) == ((ks[0], ks[-1] + 1) if ks else (0, 0)), (n, lo, hi)
            assert hz.tolist() == [k * 48000 / n for k in ks]


def _with_spectrograms(text, specs):
    """the document `text` plus Spectrogram nodes: specs = [(node id, saved fields, [(producer id, output port name)])]"""
    doc = json.loads(text)
    by_id = {n["id"]: n for n in doc["nodes"]}
    for nid, fields, srcs in specs:
        cfg = {"id": nid, "inputs": {"in": nid + 1000}}
        cfg.update(fields)
        doc["nodes"].append({"id": nid, "typename": "spectrogram", "position": [0.0, 0.0], "cfg": cfg})
        for s, o in srcs:
            doc["links"].append({"lhs": [s, by_id[s]["cfg"]["outputs"][o]], "rhs": [nid, nid + 1000]})
    return json.dumps(doc)


SAVED = {"buffer_size": 100, "fft_size": 2048, "upper_bound": 12000, "lower_bound": 40}


def test_graph_spectrum_taps_from_a_saved_document(dspfx):
    from dsp_stuff_amd import config, graph as G
    base = graphs.diamond()
    text = _with_spectrograms(base, [(500, SAVED, [(2, "out"), (5, "out")]), (510, {}, [])])
    g = G.Graph(text)
    assert g.dropped == [500, 510] and list(g.spectrum_taps) == [500, 510] and g.pitch_taps == {}
    a, b = g.spectrum_taps[500], g.spectrum_taps[510]
    assert a.links == [2, 5] and (a.fft_size, a.buffer_size, a.lower_bound, a.upper_bound) == (2048, 100, 40, 12000)
    assert b.links == [] and (b.fft_size, b.buffer_size, b.lower_bound, b.upper_bound) == (512, 250, 20, 20000)   # spectrogram.rs:198-201
    plain = G.Graph(base)
    assert plain.spectrum_taps == {} and set(g.nodes) == set(plain.nodes) and g.order == plain.order
    assert [n.outs for n in g.nodes.values()] == [n.outs for n in plain.nodes.values()]   # the taps change no plan
    # a link into a port the node does not have
    doc = json.loads(text)
    doc["links"].append({"lhs": doc["links"][-1]["lhs"], "rhs": [510, 7]})
    with pytest.raises(config.DspConfigError, match="unknown input port"):
        G.Graph(json.dumps(doc))


def test_a_demux_unselected_port_feeds_zeros(dspfx):
    from dsp_stuff_amd import graph as G
    text = _with_spectrograms(graphs.routing(out_port="A"), [(500, {}, [(4, "b"), (4, "a"), (1, "out")])])
    g = G.Graph(text)
    assert g.spectrum_taps[500].links == [G.ZERO, 4, 1]                         # a connected pipe of zeros still counts
    text = _with_spectrograms(graphs.routing(out_port="B"), [(500, {}, [(4, "b"), (4, "a")])])
    assert G.Graph(text).spectrum_taps[500].links == [4, G.ZERO]
    # pitch and spectrogram taps side by side
    doc = json.loads(text)
    doc["nodes"].append({"id": 600, "typename": "pitch", "position": [0, 0], "cfg": {"id": 600, "inputs": {"in": 601}, "outputs": {}}})
    doc["links"].append({"lhs": doc["links"][0]["lhs"], "rhs": [600, 601]})
    g = G.Graph(json.dumps(doc))
    assert list(g.pitch_taps) == [600] and list(g.spectrum_taps) == [500] and g.dropped == [500, 600]


def test_a_saved_size_that_is_no_power_of_two_raises_only_with_spectrum(dspfx):
    """The importer keeps what was saved; only GraphEngine(spectrum=True) needs a size the bank takes, and it says so
    before it touches a device (so this runs without a GPU)."""
    from dsp_stuff_amd import config, graph as G
    text = _with_spectrograms(graphs.diamond(), [(500, dict(SAVED, fft_size=1000), [(2, "out")])])
    g = G.Graph(text)
    assert g.spectrum_taps[500].fft_size == 1000
    with pytest.raises(config.DspConfigError, match="fft_size 1000"):
        G.check_spectrum_sizes(g)
    with pytest.raises(config.DspConfigError, match="fft_size 1000"):
        G.GraphEngine(text, 64, spectrum=True)
    for bad in (64, 16384, 0):
        with pytest.raises(config.DspConfigError, match="fft_size"):
            G.check_spectrum_sizes(G.Graph(_with_spectrograms(graphs.diamond(), [(500, {"fft_size": bad}, [])])))
    for n in R.SIZES:
        G.check_spectrum_sizes(G.Graph(_with_spectrograms(graphs.diamond(), [(500, {"fft_size": n}, [])])))
    with pytest.raises(config.DspConfigError, match="not integers"):
        G.Graph(_with_spectrograms(graphs.diamond(), [(500, {"fft_size": "big"}, [])]))


def test_plans_carry_the_spectrum_taps(dspfx):
    """spectrum=True's plans take the tap's producer list exactly as pitch=True's do: an extra output block of the one
    kernel, averaged in link order.  Without taps nothing changes."""
    from dsp_stuff_amd import config, graph as G
    chain = [dspfx.BiQuad(), dspfx.Gain(0.5), dspfx.HighPass(0.2)]
    text = config.dump_dspconfig(chain)
    doc = json.loads(text)
    srcs = [(doc["nodes"][1]["id"], "out"), (doc["nodes"][2]["id"], "out")]
    g = G.Graph(_with_spectrograms(text, [(500, {}, srcs)]))
    taps = [g.spectrum_taps[500].links]
    assert taps == [[s for s, _ in srcs]]
    specs, links = G.fused_plan(g)
    specs_t, links_t = G.fused_plan(g, taps)
    assert links == G.fused_plan(G.Graph(text))[1] and len(specs_t) == len(specs)
    n_nodes = len(specs)
    assert links_t[:len(links)] == links
    assert links_t[len(links):] == [(0, n_nodes + 1, dspfx.PORT_MAIN), (1, n_nodes + 1, dspfx.PORT_MAIN)]   # output block 1, link order


def test_restatement_bookkeeping_and_structure():
    """spectrum_ref itself: an impulse, a constant and an on-bin cosine through a window of ones; the Hann triple; windows
    fall due with their last frame; the history keeps the newest columns."""
    n = 256
    ones = np.ones(n, np.float32)
    x = np.zeros((n, 3), np.float32)
    x[17, 0] = 1.0
    x[:, 1] = 3.0
    m = 40
    x[:, 2] = np.cos(2 * np.pi * m * np.arange(n) / n)
    v = R.column(x, window=ones)
    assert v.shape == (n // 2, 3)
    assert np.allclose(v[:, 0], 1.0, atol=1e-12)
    assert np.isclose(v[0, 1], 3.0 * n) and np.abs(v[1:, 1]).max() < 1e-9
    assert np.isclose(v[m, 2], n / 2, rtol=1e-6) and np.abs(np.delete(v[:, 2], m)).max() < 1e-4
    h = R.column(x[:, 2:3])[:, 0]                                               # Hann: the triple at m - 1, m, m + 1
    assert h[m] > 0.49 * n / 2 and abs(h[m - 1] / h[m] - 0.5) < 0.02 and abs(h[m + 1] / h[m] - 0.5) < 0.02
    assert np.delete(h, [m - 1, m, m + 1]).max() < 0.02 * h[m]
    rng = np.random.default_rng(1)
    sig = rng.standard_normal((4 * n + 134, 2)).astype(np.float32)
    bank = R.HostBank(2, n, columns=2)
    f = 0
    for size in (1, 127, 128, 129, n - 1, n, n + 1, 5):
        bank.push(sig[f:f + size])
        f += size
        assert bank.windows == f // n and bank.slot_free() == (f % 128 == 0)
    assert f == 4 * n + 134 and bank.due_at == [n, 2 * n, 3 * n, 4 * n]
    assert np.array_equal(bank.column(0), R.column(sig[3 * n:4 * n])) and np.array_equal(bank.column(1), R.column(sig[2 * n:3 * n]))
    assert bank.column(2) is None
    g = rng.uniform(0.5, 2.0, n // 2).astype(np.float32)
    assert np.allclose(R.column(sig[:n], gain=g), R.column(sig[:n]) * g[:, None].astype(np.float64), rtol=1e-15)
    assert R.ceiling(512) == (7 * 9 + 4) * 2.0 ** -24
