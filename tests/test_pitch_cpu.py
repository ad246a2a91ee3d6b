"""The Pitch Detector bank, the parts that need no GPU: the ABI and its mirrors (EXPORTS, the ctypes struct, the built library,
ffi.rs, engine.rs, dspfx.hpp), known answers of the float64 restatement in pitch_ref.py, the frame rule, and the graph importer's
pitch taps."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import pitch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
HPP = open(os.path.join(ROOT, "include", "dspfx.hpp")).read()
FFI = open(os.path.join(ROOT, "host", "rust", "src", "ffi.rs")).read()
ENGINE_RS = open(os.path.join(ROOT, "host", "rust", "src", "engine.rs")).read()
NEW = {"dspfx_pitch_create": 2, "dspfx_pitch_destroy": 1, "dspfx_pitch_push": 4, "dspfx_pitch_slot": 1,
       "dspfx_pitch_set_param": 3, "dspfx_pitch_read": 4, "dspfx_pitch_reset": 1, "dspfx_pitch_windows": 1}
CTYPE = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "float": C.c_float}
RUST = {"uint32_t": "u32", "int32_t": "i32", "float": "f32"}


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _header_desc_fields():
    m = re.search(r"typedef struct dspfx_pitch_desc\s*\{(.*?)\}\s*dspfx_pitch_desc;", _strip_comments(HDR), re.S)
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


def test_ctypes_desc_matches_the_header_field_by_field(dspfx):
    fields = _header_desc_fields()
    assert [f[1] for f in fields] == ["abi_version", "device", "channels", "tile_channels", "power_thresh", "clarity_thresh",
                                      "pick_thresh"]
    py = dspfx._PitchDesc._fields_
    assert [f[0] for f in py] == [f[1] for f in fields]
    assert [t for _, t in py] == [CTYPE[f[0]] for f in fields]
    assert C.sizeof(dspfx._PitchDesc) == 28
    body = _strip_comments(HDR)
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(DSPFX_PITCH_[A-Z]+)\s*=\s*(\d+)", body)}
    assert consts == {"DSPFX_PITCH_POWER": 0, "DSPFX_PITCH_CLARITY": 1, "DSPFX_PITCH_PICK": 2}
    assert (dspfx.PITCH_POWER, dspfx.PITCH_CLARITY, dspfx.PITCH_PICK, dspfx.PITCH_WINDOW) == (0, 1, 2, 1024)


def test_rust_and_cpp_mirrors():
    ffi = _strip_comments(FFI)
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct dspfx_pitch_desc\s*\{(.*?)\}", ffi, re.S)
    assert m, "dspfx_pitch_desc is not a #[repr(C)] struct in ffi.rs"
    fields = [f.strip().replace("pub ", "") for f in m.group(1).split(",") if f.strip()]
    assert fields == [f"{n}: {RUST[t]}" for t, n in _header_desc_fields()], fields
    for name, arity in NEW.items():
        m = re.search(r"pub fn %s\s*\(([^)]*)\)" % name, ffi)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == arity, name
    src = re.sub(r'"(?:[^"\\]|\\.)*"', '""', _strip_comments(ENGINE_RS))
    assert "pub struct PitchBank" in src and "impl Drop for PitchBank" in src
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert re.search(r"\b%s\s*\(" % name, HPP), name
    assert "class PitchBank" in HPP


def test_restatement_finds_a_440hz_sine():
    t = np.arange(R.WINDOW) / R.RATE
    found, tau, freq, clarity, margin = R.detect(0.5 * np.sin(2 * np.pi * 440.0 * t))
    assert found and tau == 109
    assert abs(freq - 440.0) < 0.05
    assert abs(clarity - 1.0) < 1e-3 and margin > 1e-4


def test_power_below_the_threshold_is_none():
    t = np.arange(R.WINDOW) / R.RATE
    x = 0.02 * np.sin(2 * np.pi * 440.0 * t)          # sum x^2 = 0.2
    assert np.sum(x * x) < 0.5
    assert not R.detect(x)[0]
    assert R.detect(x, P=0.1)[0]
    assert not R.detect(np.zeros(R.WINDOW))[0]
    y = 0.5 * np.sin(2 * np.pi * 440.0 * t)
    y[7] = np.nan
    assert not R.detect(y)[0]


def test_aliasing_term_matches_the_direct_sum():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(R.WINDOW) * np.hanning(R.WINDOW)
    r = R.autocorr(x)
    d = R.autocorr_direct(x)
    assert np.allclose(r, d, rtol=0, atol=1e-9 * d[0])
    lin = np.correlate(x, x, mode="full")[R.WINDOW - 1:]
    assert np.array_equal(r[:R.PADDING + 1], lin[:R.PADDING + 1])       # no alias up to lag 512
    assert np.abs(r[R.PADDING + 1:] - lin[R.PADDING + 1:]).max() > 1.0  # and a real one above it


def test_normalisation_is_bounded_and_the_alias_moves_only_low_pitches():
    rng = np.random.default_rng(4)
    for _ in range(5):
        n = R.nsdf(rng.standard_normal(R.WINDOW))
        assert np.abs(n).max() <= 1.0 + 1e-12
    t = np.arange(R.WINDOW) / R.RATE
    for f in (100.0, 200.0, 440.0, 1000.0, 4000.0):
        found, _, fr, _, _ = R.detect(0.5 * np.sin(2 * np.pi * f * t + 0.3))
        assert found and abs(fr / f - 1.0) < 2e-3, f
    found, _, fr, _, _ = R.detect(0.5 * np.sin(2 * np.pi * 80.0 * t + 0.3))
    assert found and abs(fr / 80.0 - 1.0) > 0.01                        # below ~94 Hz the 1536-point alias wins


@pytest.mark.parametrize("size", [128, 1000, 37])
def test_frame_rule_on_the_host(size):
    pushes = [size] * (5000 // size + 2)
    due = R.windows_due(pushes)
    f = 0
    seen = []
    for n, ws in zip(pushes, due):
        f0, f = f, f + n
        for w in ws:
            assert f >= 1024 * (w + 1) + 1 and f0 < 1024 * (w + 1) + 1
        seen += ws
    assert seen == list(range(len(seen)))                            # every window once, in order
    assert len(seen) == (f - 1) // 1024
    if size == 128:
        assert [k for k, ws in enumerate(due) if ws] == [8, 16, 24, 32, 40]   # window w at the start of call 8 (w + 1)


def _doc_with_pitch(dspfx, links_into_in=1, cfg_extra=None, slider_link=False):
    from dsp_stuff_amd import config
    chain = [dspfx.BiQuad(), dspfx.Gain(0.5), dspfx.HighPass(0.2)]
    doc = json.loads(config.dump_dspconfig(chain))
    nid, pid = 500, 600
    cfg = {"id": nid, "inputs": {"in": pid, "power_thresh": 601}, "outputs": {}}
    cfg.update(cfg_extra or {})
    doc["nodes"].append({"id": nid, "typename": "pitch", "position": [0, 0], "cfg": cfg})
    taps = [doc["nodes"][1], doc["nodes"][3]][:links_into_in]
    for tap in taps:
        doc["links"].append({"lhs": [tap["id"], tap["cfg"]["outputs"]["out"]], "rhs": [nid, pid]})
    if slider_link:
        doc["links"].append({"lhs": [doc["nodes"][2]["id"], doc["nodes"][2]["cfg"]["outputs"]["out"]], "rhs": [nid, 601]})
    return doc, [t["id"] for t in taps]


def test_graph_pitch_taps_from_a_saved_document(dspfx):
    from dsp_stuff_amd import config, graph as G
    doc, srcs = _doc_with_pitch(dspfx, 2, {"power_thresh": 0.25, "clarity_thresh": 0.75, "pick_thresh": 0.9})
    g = G.Graph(json.dumps(doc))
    assert g.dropped == [500] and list(g.pitch_taps) == [500]
    tap = g.pitch_taps[500]
    assert tap.links == srcs and tap.thresholds == (0.25, 0.75, 0.9)
    plain = G.Graph(config.dump_dspconfig([dspfx.BiQuad(), dspfx.Gain(0.5), dspfx.HighPass(0.2)]))
    assert set(g.nodes) == set(plain.nodes) and plain.pitch_taps == {}
    assert [n.outs for n in g.nodes.values()] == [n.outs for n in plain.nodes.values()]   # the tap changes no plan
    doc, _ = _doc_with_pitch(dspfx, 1)
    assert G.Graph(json.dumps(doc)).pitch_taps[500].thresholds == (0.5, 0.5, 0.5)      # the sliders' defaults


def test_a_driven_threshold_is_rejected(dspfx):
    from dsp_stuff_amd import config, graph as G
    doc, _ = _doc_with_pitch(dspfx, 1, slider_link=True)
    with pytest.raises(config.DspConfigError, match="driven by a link"):
        G.Graph(json.dumps(doc))


def test_plans_carry_the_taps(dspfx):
    """pitch=True's plans: the tap is output block 1 of the one kernel and of the last region, averaged like the Output
    node's port, in link order; the run-by-run plan ends a run at every tapped node.  Without taps nothing changes."""
    from dsp_stuff_amd import graph as G
    doc, srcs = _doc_with_pitch(dspfx, 2)
    doc["nodes"][-1]["cfg"]["inputs"].pop("power_thresh")
    g = G.Graph(json.dumps(doc))
    taps = [g.pitch_taps[500].links]
    specs, links = G.fused_plan(g)
    specs_t, links_t = G.fused_plan(g, taps)
    order = [nid for nid in g.order if g.nodes[nid].spec is not None]
    assert specs_t == specs and links_t[:len(links)] == links
    assert links_t[len(links):] == [(order.index(s), len(order) + 1, dspfx.PORT_MAIN) for s in srcs]
    steps = G.region_plan(g)
    steps_t = G.region_plan(g, taps=taps)
    assert len(steps) == len(steps_t) == 1 and steps_t[0][4] == steps[0][4] + 1
    assert [l for l in steps_t[0][2] if l[1] == len(order) + 1] == links_t[len(links):]
    runs, _ = G.plan_runs(g)
    runs_t, _ = G.plan_runs(g, keep=set(srcs))
    assert [[m.id for m in r.nodes] for r in runs] == [order]
    assert [[m.id for m in r.nodes] for r in runs_t] == [[order[0]], order[1:]]
    assert G.fused_plan(g, [srcs] * 16) is None                       # more output blocks than a kernel has
