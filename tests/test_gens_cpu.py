"""The channel-generator bank without a GPU: the restatement the GPU tests lean on (gens_ref: one oracle Signal Generator per
channel) against oracle.run_channels bit for bit for the four modes, over several blocks, over a block length that is no multiple of
128, with and without control ports; its store rules (the defaults on the first store, None keeps, a refused store changes
nothing, a drop then a set starts at clock 0, reset); dspfx_gens_plan; the create refusals and the argument checks that need no
device; header, EXPORTS, the ctypes signatures and ffi.rs agree.  A store's own checks need a bank and so a device: here the
restatement refuses them, tests/test_gens_gpu.py holds the bank to that."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gens_ref as R
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
FFI = open(os.path.join(ROOT, "host", "rust", "src", "ffi.rs")).read()
INVALID = -1
NF = 128
F = np.float32
NAMES = ("dspfx_gens_plan", "dspfx_gens_create", "dspfx_gens_destroy", "dspfx_gens_last_error", "dspfx_gens_run", "dspfx_gens_set",
         "dspfx_gens_drop", "dspfx_gens_reset", "dspfx_gens_present", "dspfx_gens_modes", "dspfx_gens_sliders", "dspfx_gens_clocks")
PAIRS = ((100.0, 0.5), (12000.0, 1.0), (0.1, -0.3), (19999.0, 0.7), (441.0, -1.0))       # (frequency, amplitude): test_signal_gen_modes


@pytest.fixture(autouse=True)
def platform_sine(monkeypatch):
    """The numpy model takes the sine correctly rounded, the C oracle calls the platform's sinf, and the two differ by an ulp here
    and there.  As tests/test_edge_values_cpu.py does, the model's math-library calls are pointed at the platform's for these
    tests: for Sine, what is held to the oracle bit for bit is every line AROUND that call."""
    import numpy_model as M
    from test_edge_values_cpu import _platform_libm
    monkeypatch.setattr(M, "LIBM", _platform_libm())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def desc(dspfx, amp, freq, mode):
    return dspfx.SignalGen(amp, freq, mode).oracle_desc()


def oracle_runs(descs, lengths, ctl=None):
    """oracle.run_channels over consecutive runs of `lengths` frames, each cut into blocks of 128 from its frame 0, state carried:
    one column"""
    nodes, out, f0 = [], [], 0
    for n in lengths:
        for b0 in range(0, n, NF):
            b1 = min(n, b0 + NF)
            sl = slice(f0 + b0, f0 + b1)
            out.append(O.run_channels(descs, np.zeros((b1 - b0, 1), F), 0, block=NF, ctl={k: v[sl] for k, v in ctl.items()} if ctl else None,
                                      nodes_out=nodes))
        f0 += n
    return np.concatenate(out)


def test_the_entry_points_exist_in_the_header_the_exports_and_the_rust_bindings_with_the_declared_signatures(dspfx):
    L = dspfx.lib()
    body = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    for name in NAMES:
        assert name in dspfx.EXPORTS and hasattr(L, name), name
        m = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % name, body)
        assert m, name
        assert re.search(r"pub fn %s\s*\(" % name, FFI), name
        assert len(getattr(L, name).argtypes) == len(m.group(1).split(",")), (name, "the ctypes mirror takes as many arguments as the header declares")
    assert sorted(n for n in dspfx.EXPORTS if n.startswith("dspfx_gens_")) == sorted(NAMES)
    assert sorted(set(re.findall(r"\b(dspfx_gens_[a-z_]+)\s*\(", HDR))) == sorted(NAMES)
    fields = [d.strip().split()[-1] for d in re.search(r"typedef struct dspfx_gens_desc\s*\{(.*?)\}", body, re.S).group(1).split(";") if d.strip()]
    assert fields == [f for f, _ in dspfx._GensDesc._fields_] == ["abi_version", "device", "n_channels", "max_frames", "tile_channels"]
    assert L.dspfx_gens_run.argtypes[-2] is C.c_uint32 and L.dspfx_gens_set.argtypes[3] is C.POINTER(C.c_uint32)
    assert L.dspfx_gens_last_error.restype is C.c_char_p
    for m in ("run", "set", "drop", "reset", "present", "modes", "sliders", "clocks", "close"):
        assert hasattr(dspfx.ChannelGenerators, m), m
    assert callable(dspfx.gens_plan)
    assert "#define DSPFX_GENS_NONE 0xFFFFFFFFu" in HDR and dspfx.GENS_NONE == R.NONE == 0xFFFFFFFF
    assert "pub const DSPFX_GENS_NONE: u32 = 0xFFFF_FFFF;" in FFI and "pub struct dspfx_gens_desc" in FFI
    assert (R.SINE, R.TRIANGLE, R.SQUARE, R.CONSTANT) == (dspfx.SIG_SINE, dspfx.SIG_TRIANGLE, dspfx.SIG_SQUARE, dspfx.SIG_CONSTANT)
    assert dspfx.ABI_VERSION == 2 and L.dspfx_abi_version() == 2


def test_the_restatements_defaults_are_dspfx_node_defaults(dspfx):
    d = dspfx._NodeDesc()
    assert dspfx.lib().dspfx_node_defaults(dspfx.SIGNAL_GEN, C.byref(d)) == 0
    assert [float(v) for v in d.params[:2]] == [R.DEFAULT_AMPLITUDE, R.DEFAULT_FREQUENCY] and d.mode == R.DEFAULT_MODE == dspfx.SIG_SINE


@pytest.mark.parametrize("mode", range(4))
def test_restatement_equals_the_oracle_bit_for_bit(dspfx, mode):
    """the (frequency, amplitude) pairs of test_signal_gen_modes in channels side by side: six blocks of 128 in one run, in runs of
    128, 256 and 384, and in six runs of 100 frames, which end the generator's block with them"""
    n = len(PAIRS)
    for lengths in ((768,), (128, 256, 384), (100,) * 6):
        ref = R.ChannelGenerators(n)
        assert ref.set([a for _, a in PAIRS], [f for f, _ in PAIRS], mode)
        got = np.concatenate([ref.run(k) for k in lengths])
        for c, (freq, amp) in enumerate(PAIRS):
            want = oracle_runs([desc(dspfx, amp, freq, mode)], lengths)
            assert np.array_equal(bits(got[:, c:c + 1]), bits(want)), (mode, lengths, freq, amp)
        if mode == R.CONSTANT:
            assert not ref.clocks().any(), "Constant leaves the clock alone"
        else:
            assert ref.clocks().any()


@pytest.mark.parametrize("mode", range(4))
def test_restatement_with_ports_equals_the_oracle_bit_for_bit(dspfx, mode):
    """amplitude, frequency and both (test_signal_gen_control_ports_and_state's blocks) on every block of the run: a port that
    stays connected never shows the oracle's latch.  Then a run without ports: the restatement goes by its stored sliders where the
    oracle would go by the latch"""
    n, nf = 3, 3 * NF + 37
    ca = (O.noise(31, np.arange(n), np.arange(nf)) * F(1.3)).astype(F)
    cf = (O.noise(32, np.arange(n), np.arange(nf)) * F(0.02) - F(0.9)).astype(F)
    for ports in ((0,), (1,), (0, 1)):
        ref = R.ChannelGenerators(n)
        assert ref.set(0.5, 300.0, mode)
        got = ref.run(nf, amplitude=ca if 0 in ports else None, frequency=cf if 1 in ports else None)
        for c in range(n):
            ctl = {(0, k): (ca, cf)[k][:, c:c + 1] for k in ports}
            want = oracle_runs([desc(dspfx, 0.5, 300.0, mode)], (nf,), ctl)
            assert np.array_equal(bits(got[:, c:c + 1]), bits(want)), (mode, ports, c)
        assert np.array_equal(ref.sliders(), np.tile(F([0.5, 300.0]), (n, 1))), "no latch"
        clocks = ref.clocks()
        after = ref.run(NF)
        plain = R.ChannelGenerators(n)
        assert plain.set(0.5, 300.0, mode)
        for c in range(n):
            plain.node[c].impl.clock = clocks[c]
        assert np.array_equal(bits(after), bits(plain.run(NF))), "a later run without the block uses what the stores left"


def test_restatement_every_channel_its_own_generator_and_add_to(dspfx):
    """mode c % 5 (4: no node), sliders per channel; add_to is one f32 addition, a channel without a node keeps add_to's bits"""
    n, nf = 20, 2 * NF
    ref = R.ChannelGenerators(n)
    settings = {}
    for c in range(n):
        if c % 5 < 4:
            settings[c] = (0.1 * (c + 1) - 1.0, 50.0 * (c + 1) ** 2, c % 5)
            assert ref.set(*settings[c], first_channel=c, count=1)
    twin = R.ChannelGenerators(n)
    for c, s in settings.items():
        assert twin.set(*s, first_channel=c, count=1)
    base = O.noise(7, np.arange(n), np.arange(nf))
    base[3, :4] = [np.nan, -0.0, np.inf, 0.0]
    base.view(np.uint32)[5, 4] = 0x7FC12345
    got, added = ref.run(nf), twin.run(nf, add_to=base)
    for c in range(n):
        if c in settings:
            amp, freq, mode = settings[c]
            want = oracle_runs([desc(dspfx, amp, freq, mode)], (nf,))
            assert np.array_equal(bits(got[:, c:c + 1]), bits(want)), c
            w = (base[:, c] + got[:, c]).astype(F)
            ok = (bits(added[:, c]) == bits(w)) | (np.isnan(w) & np.isnan(added[:, c]))
            assert ok.all(), c
        else:
            assert not bits(got[:, c]).any(), "no node: +0.0"
            assert np.array_equal(bits(added[:, c]), bits(base[:, c])), "no node: add_to's very bits"
    assert list(ref.present()) == [0 if c % 5 == 4 else 1 for c in range(n)]
    assert list(ref.modes()) == [R.NONE if c % 5 == 4 else c % 5 for c in range(n)]


def test_restatement_store_rules():
    ref = R.ChannelGenerators(6)
    assert not ref.present().any() and (ref.modes() == R.NONE).all() and not ref.sliders().any() and not ref.clocks().any()
    assert ref.set(first_channel=1, count=2)
    assert list(ref.present()) == [0, 1, 1, 0, 0, 0] and list(ref.modes()[1:3]) == [R.SINE] * 2, "the defaults on the first store"
    assert [list(r) for r in ref.sliders()[1:3]] == [[0.5, 100.0]] * 2
    assert ref.set(frequency=[1000.0, 2000.0], first_channel=2) and list(ref.sliders()[2]) == [0.5, 1000.0] and list(ref.sliders()[3]) == [0.5, 2000.0]
    assert ref.set(mode=R.SQUARE, first_channel=2, count=1) and list(ref.sliders()[2]) == [0.5, 1000.0] and ref.modes()[2] == R.SQUARE, "None keeps"
    assert ref.set(amplitude=-0.25, first_channel=2, count=1) and list(ref.sliders()[2]) == [-0.25, 1000.0] and ref.modes()[2] == R.SQUARE
    ref.run(NF)
    clocks = ref.clocks()
    assert clocks[1] != 0 and clocks[2] != 0 and clocks[0] == 0
    assert ref.set(frequency=3000.0, mode=R.TRIANGLE, first_channel=1, count=2) and np.array_equal(ref.clocks(), clocks), "a set keeps the clock"
    before = [t.copy() for t in (ref.present(), ref.modes(), ref.sliders(), ref.clocks())]
    for call in (lambda: ref.set(1.0, 1.0, 4), lambda: ref.set(1.0, 1.0, [0, 1, 2, 3, 0, -1]), lambda: ref.set(1.0, first_channel=5, count=2),
                 lambda: ref.set(1.0, first_channel=7, count=0), lambda: ref.set(1.0, first_channel=0, count=7), lambda: ref.drop(6, 1),
                 lambda: ref.reset(3, 4)):
        assert call() is False
    assert all(np.array_equal(u, v) for u, v in zip(before, (ref.present(), ref.modes(), ref.sliders(), ref.clocks()))), "a refused store changes nothing"
    assert ref.drop(1, 1) and ref.present()[1] == 0 and ref.modes()[1] == R.NONE and not ref.sliders()[1].any() and ref.clocks()[1] == 0
    assert ref.set(mode=R.TRIANGLE, first_channel=1, count=1) and list(ref.sliders()[1]) == [0.5, 100.0] and ref.clocks()[1] == 0, "after a drop: the defaults, clock 0"
    assert ref.clocks()[2] == clocks[2], "the neighbour keeps its phase"
    assert ref.reset(0, 3) and not ref.clocks()[:3].any() and ref.clocks()[3] == clocks[3] and list(ref.present()) == [0, 1, 1, 1, 0, 0]
    assert ref.set(float("nan"), float("inf"), first_channel=0, count=1) and np.isnan(ref.sliders()[0, 0]) and np.isinf(ref.sliders()[0, 1]), "values are taken as given"
    assert ref.set(5.0, 1e12, first_channel=0, count=1) and list(ref.sliders()[0]) == [5.0, F(1e12)], "no clamp to the slider's range"


def test_a_dropped_and_reset_channel_restart_at_clock_zero(dspfx):
    """the first block after a drop + set, and after a reset, is the first block of a fresh oracle node"""
    ref = R.ChannelGenerators(3)
    assert ref.set(0.7, 777.0, R.TRIANGLE)
    first = ref.run(100)
    ref.run(NF)
    assert ref.drop(0, 1) and ref.set(0.7, 777.0, R.TRIANGLE, first_channel=0, count=1) and ref.reset(1, 1)
    again = ref.run(100)
    assert np.array_equal(bits(again[:, :2]), bits(first[:, :2])) and not np.array_equal(bits(again[:, 2]), bits(first[:, 2]))
    want = oracle_runs([desc(dspfx, 0.7, 777.0, R.TRIANGLE)], (100, 128, 100))
    assert np.array_equal(bits(again[:, 2:]), bits(want[228:]))


def test_plan_is_the_formula(dspfx):
    for n in (1, 70, 256, 1 << 20, 0xFFFFFF00):
        assert dspfx.gens_plan(n) == 13 * n
    for n in (0, 1 << 32, 0xFFFFFF01):
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.gens_plan(n)
        assert e.value.status == INVALID and "n_channels" in str(e.value) and "gens" in str(e.value), str(e.value)


@pytest.mark.parametrize("kw,word", [
    (dict(tile_channels=48), "power of two"),
    (dict(tile_channels=64), "divides"),
    (dict(channels=0), "n_channels"),
    (dict(channels=0xFFFFFF01), "n_channels"),
    (dict(max_frames=0), "max_frames"),
    (dict(max_frames=(1 << 20) + 1), "max_frames"),
])
def test_create_rejects_a_bad_descriptor_before_any_device_work(dspfx, kw, word):
    args = dict(channels=1000, tile_channels=0, max_frames=128)
    args.update(kw)
    with pytest.raises(dspfx.DspfxError) as e:
        dspfx.ChannelGenerators(**args)
    assert e.value.status == INVALID and word in str(e.value) and "gens" in str(e.value), str(e.value)


def test_null_arguments_are_invalid(dspfx):
    L = dspfx.lib()
    h = C.c_void_p()
    assert L.dspfx_gens_create(None, C.byref(h)) == INVALID
    assert L.dspfx_gens_last_error(None)
    assert L.dspfx_gens_destroy(None) == INVALID
    assert L.dspfx_gens_run(None, None, None, None, None, 128, None) == INVALID
    assert L.dspfx_gens_set(None, None, None, None, 0, 0) == INVALID
    assert L.dspfx_gens_drop(None, 0, 0) == INVALID
    assert L.dspfx_gens_reset(None, 0, 0) == INVALID
    for name in ("present", "modes", "sliders"):
        assert getattr(L, "dspfx_gens_" + name)(None, None, 0, 0) == INVALID
    assert L.dspfx_gens_clocks(None, None) == INVALID
    assert L.dspfx_gens_plan(8, None) == 0
