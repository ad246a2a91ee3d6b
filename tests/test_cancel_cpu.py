"""The channel-canceller bank without a GPU: the numpy model of ONE LANE of cancel_kernels.hip (cancel_ref.LaneModel: ring rows,
the general body, the fast body with its tap classes and sliding window) against the rule's restatement (cancel_ref.CancelRef) bit
for bit; that the rule does what it is for (it converges on an echo path, a frozen node keeps its weights); the f32 recursion
against a float64 one; the store rules; dspfx_cancel_plan against its written formula; the refusals and argument checks that need
no device; header, EXPORTS, ctypes signatures and ffi.rs agree."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cancel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
FFI = open(os.path.join(ROOT, "host", "rust", "src", "ffi.rs")).read()
INVALID = -1
F = np.float32
NAMES = ("dspfx_cancel_plan", "dspfx_cancel_create", "dspfx_cancel_destroy", "dspfx_cancel_last_error", "dspfx_cancel_run", "dspfx_cancel_set",
         "dspfx_cancel_load", "dspfx_cancel_drop", "dspfx_cancel_reset", "dspfx_cancel_present", "dspfx_cancel_lengths", "dspfx_cancel_sliders",
         "dspfx_cancel_delays", "dspfx_cancel_adapting", "dspfx_cancel_weights_view", "dspfx_cancel_levels_view")
DELAYS = (0, 1, 37)


def noise(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(F)


@pytest.mark.parametrize("general_only", [False, True])
def test_lane_model_is_the_rule(general_only):
    """Channel c = (T, D) for every T of the list and D of 0, 1, 37, all in one restated bank; one LaneModel each.  Output, weights
    and levels after every run, through the four cuts, a shorter and a longer T, a load, a reset, drop then set, adapt off then on."""
    combos = [(T, D) for T in R.T_LIST for D in DELAYS]
    n = len(combos)
    Ts, Ds = np.array([c[0] for c in combos]), np.array([c[1] for c in combos])
    ref = R.CancelRef(n, max_taps=64, max_delay=37)
    lanes = [R.LaneModel(64, 37, general_only) for _ in combos]
    seed = [0]

    def run(nf):
        seed[0] += 1
        mic, far = noise((nf, n), 100 + seed[0]), noise((nf, n), 200 + seed[0])
        want = ref.run(mic, far)
        for c, lane in enumerate(lanes):
            got = lane.run(mic[:, c], far[:, c])
            assert R.same_bits(got, want[:, c]), (combos[c], nf, "out")
            assert R.same_bits(lane.w, ref.w[c]), (combos[c], nf, "weights")
            assert R.same_bits(lane.lev, ref.lev[:, c]), (combos[c], nf, "levels")
            assert not lane.w[lane.T:].any() and not np.signbit(lane.w[lane.T:]).any()

    run(16)                                                                    # no node anywhere: copies, the row counter moves
    ref.set(taps=Ts, delay=Ds, mu=0.5, eps=1e-6)
    for c, lane in enumerate(lanes):
        lane.set(taps=Ts[c], delay=Ds[c], mu=0.5, eps=1e-6)
    for nf in R.CUTS:
        run(nf)
    short, longer = np.maximum(1, Ts // 2), np.minimum(64, Ts + 3)
    for new in (short, longer):
        ref.set(taps=new)
        for c, lane in enumerate(lanes):
            lane.set(taps=new[c])
        run(37)
        run(16)
    rows = noise((n, 64), 7) * F(0.25)
    for c, lane in enumerate(lanes):
        ref.load(rows[c, :longer[c]], first_channel=c, count=1)
        lane.load(rows[c, :longer[c]])
    run(24)
    ref.reset()
    for lane in lanes:
        lane.reset()
    run(37)
    ref.drop()
    for lane in lanes:
        lane.drop()
    run(9)
    ref.set(taps=Ts, delay=Ds[::-1].copy(), mu=0.25, eps=1e-3)
    for c, lane in enumerate(lanes):
        lane.set(taps=Ts[c], delay=Ds[::-1][c], mu=0.25, eps=1e-3)
    run(40)
    for adapt in (False, True):
        ref.set(adapt=adapt)
        for lane in lanes:
            lane.set(adapt=adapt)
        run(24)
    ref.set(delay=Ds)                                                          # a new delay keeps weights and history
    for c, lane in enumerate(lanes):
        lane.set(delay=Ds[c])
    run(24)


def echo_case(T, channels, frames, seed):
    """white noise in [-1, 1] as ref, a path of T taps uniform in [-0.5, 0.5] per channel, d its exact echo (f64, rounded to f32)"""
    rng = np.random.default_rng(seed)
    far = rng.uniform(-1.0, 1.0, (frames, channels)).astype(F)
    path = rng.uniform(-0.5, 0.5, (channels, T))
    mic = np.stack([np.convolve(far[:, c].astype(np.float64), path[c])[:frames] for c in range(channels)], axis=1).astype(F)
    return far, path, mic


@pytest.mark.parametrize("T", [8, 32, 64])
def test_the_rule_converges_and_a_frozen_node_keeps_its_weights(T):
    """Over frames [20 T, 20 T + 128) the echo return loss 10 log10(sum d^2 / sum e^2) is at least 40 dB on every channel (a floor
    with room: on these signals the rule gives 60 dB or more at these T); then adapt off: the weights stay, bit for bit."""
    n = 16
    far, path, mic = echo_case(T, n, 20 * T + 256, 0xA5C0 + T)
    ref = R.CancelRef(n, max_taps=T)
    ref.set(taps=T, mu=0.5, eps=1e-6)
    ref.run(mic[:20 * T], far[:20 * T])
    ref.run(mic[20 * T:20 * T + 128], far[20 * T:20 * T + 128])
    erle = 10.0 * np.log10(ref.lev[0].astype(np.float64) / ref.lev[1].astype(np.float64))
    print(f"T={T}: ERLE over [20T, 20T+128) min {erle.min():.1f} dB, max {erle.max():.1f} dB")
    assert (erle >= 40.0).all(), erle
    ref.set(adapt=False)
    before = ref.w.copy()
    out = ref.run(mic[20 * T + 128:], far[20 * T + 128:])
    assert R.same_bits(ref.w, before)
    assert np.abs(out).max() < 1e-2                                            # (it still filters)


# max over channels and T of max_k |w32[k] - w64[k]| after 40 T frames, as measured on the CPU: see the test's docstring
W_DISTANCE = {8: 2 * 5.556e-8, 32: 2 * 1.233e-7}


@pytest.mark.parametrize("T", [8, 32])
def test_f32_weights_follow_a_float64_nlms(T):
    """The f32 rule against a float64 NLMS of the same recursion (cancel_ref.nlms64) after 40 T frames of the echo case, 4 channels.
    No useful bound follows from the rounding model alone (the recursion's error feeds back through e and is contracted by the
    adaptation itself, which a worst-case rounding bound does not see), so the distance max_k |w32[k] - w64[k]| was measured on the
    CPU: 5.556e-08 at T = 8 and 1.233e-07 at T = 32 (weights of magnitude up to 0.5, whose ulp is 6e-8: one and two ulp).  The test
    asserts twice the measured value."""
    n = 4
    far, path, mic = echo_case(T, n, 40 * T, 0xF640 + T)
    ref = R.CancelRef(n, max_taps=T)
    ref.set(taps=T, mu=0.5, eps=1e-6)
    for f in range(0, 40 * T, 128):
        ref.run(mic[f:f + 128], far[f:f + 128])
    worst = 0.0
    for c in range(n):
        _, w64 = R.nlms64(mic[:, c], far[:, c], T)
        worst = max(worst, float(np.abs(ref.w[c, :T].astype(np.float64) - w64).max()))
        assert np.abs(w64 - path[c]).max() < 1e-4                              # (both found the path)
    print(f"T={T}: max |w32 - w64| = {worst:.3e}")
    assert worst <= W_DISTANCE[T], worst


def test_restatement_store_rules():
    ref = R.CancelRef(6, max_taps=16, max_delay=10)
    ref.set(taps=[4, 5, 6], first_channel=2)
    assert list(ref.T) == [0, 0, 4, 5, 6, 0] and list(ref.adapt) == [False, False, True, True, True, False]
    assert list(ref.mu[2:5]) == [F(0.5)] * 3 and list(ref.eps[2:5]) == [F(1e-6)] * 3 and list(ref.D) == [0] * 6
    ref.set(adapt=False, first_channel=1, count=2)                             # a new node of max_taps taps, and a kept one
    assert list(ref.T) == [0, 16, 4, 5, 6, 0] and list(ref.adapt) == [False, False, False, True, True, False]
    ref.load(np.arange(1, 6, dtype=F), first_channel=3, count=1)
    ref.set(taps=3, mu=0.25, first_channel=3, count=1)
    assert list(ref.w[3]) == [1, 2, 3] + [0] * 13 and ref.mu[3] == F(0.25) and ref.eps[3] == F(1e-6), "a shorter T zeroes the rows it leaves"
    ref.set(taps=5, first_channel=3, count=1)
    assert list(ref.w[3]) == [1, 2, 3] + [0] * 13, "a longer T starts the new rows at +0.0"
    ref.set(delay=10, mu=np.nan, first_channel=3, count=1)
    assert ref.D[3] == 10 and np.isnan(ref.mu[3]) and list(ref.w[3][:3]) == [1, 2, 3], "values as given; a delay keeps the weights"
    snap = (ref.T.copy(), ref.D.copy(), ref.w.copy())
    for call in (lambda: ref.set(taps=0), lambda: ref.set(taps=17), lambda: ref.set(delay=11), lambda: ref.set(taps=4, first_channel=5, count=2),
                 lambda: ref.set(taps=[4, 4], mu=[0.5, 0.5, 0.5]), lambda: ref.load(np.zeros(4, F), first_channel=0, count=1),
                 lambda: ref.load(np.zeros(4, F), first_channel=3, count=1), lambda: ref.load(np.zeros((2, 4), F), first_channel=2),
                 lambda: ref.drop(0, 7), lambda: ref.reset(7, 1)):
        with pytest.raises(ValueError):
            call()
    assert all(np.array_equal(u, v) for u, v in zip(snap, (ref.T, ref.D, ref.w))), "a refused store stores nothing"
    ref.reset(3, 1)
    assert not ref.w[3].any() and ref.T[3] == 5 and ref.D[3] == 10, "reset keeps the sliders"
    ref.drop(3, 1)
    assert ref.T[3] == 0 and not ref.adapt[3]


def test_plan_is_the_formula(dspfx):
    """include/dspfx.h: channels * (4 * max_taps + 4 * R + 16 + 8), R = max_delay + max_taps + 16 rounded up to a multiple of 8"""
    for n in (1, 70, 256, 1 << 20, 0xFFFFFF00):
        for max_taps in (1, 5, 64, 1024):
            for max_delay in (0, 37, 960, 65535):
                rows = (max_delay + max_taps + R.RING_PAD + 7) // 8 * 8
                assert rows == R.LaneModel(max_taps, max_delay).R
                assert dspfx.cancel_plan(n, max_taps, max_delay) == n * (4 * max_taps + 4 * rows + 16 + 8)
    assert dspfx.cancel_plan(1 << 20) == dspfx.cancel_plan(1 << 20, 64, 0)
    for n in (0, 1 << 32, 0xFFFFFF01):
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.cancel_plan(n, 64)
        assert e.value.status == INVALID and "n_channels" in str(e.value) and "cancel" in str(e.value), str(e.value)
    for max_taps in (0, 1025, 0xFFFFFFFF):
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.cancel_plan(256, max_taps)
        assert e.value.status == INVALID and "max_taps" in str(e.value) and "cancel" in str(e.value), str(e.value)
    with pytest.raises(dspfx.DspfxError) as e:
        dspfx.cancel_plan(256, 64, 65536)
    assert e.value.status == INVALID and "max_delay" in str(e.value), str(e.value)


@pytest.mark.parametrize("kw,word", [
    (dict(max_taps=0), "max_taps"),
    (dict(max_taps=1025), "max_taps"),
    (dict(max_delay=65536), "max_delay"),
    (dict(tile_channels=48), "power of two"),
    (dict(tile_channels=64), "divides"),
    (dict(channels=0), "n_channels"),
    (dict(channels=0xFFFFFF01), "n_channels"),
    (dict(max_frames=0), "max_frames"),
    (dict(max_frames=(1 << 20) + 1), "max_frames"),
])
def test_create_rejects_a_bad_descriptor_before_any_device_work(dspfx, kw, word):
    args = dict(channels=1000, max_taps=64, max_delay=0, tile_channels=0, max_frames=128)
    args.update(kw)
    with pytest.raises(dspfx.DspfxError) as e:
        dspfx.ChannelCancellers(**args)
    assert e.value.status == INVALID and word in str(e.value) and "cancel" in str(e.value), str(e.value)


def test_create_rejects_another_abi_version(dspfx):
    L = dspfx.lib()
    h = C.c_void_p()
    d = dspfx._CancelDesc(dspfx.ABI_VERSION + 1, 0, 1000, 128, 0, 64, 0, 0)
    assert L.dspfx_cancel_create(C.byref(d), C.byref(h)) == INVALID and not h.value
    assert b"abi_version" in L.dspfx_cancel_last_error(None)


def test_null_arguments_are_invalid(dspfx):
    L = dspfx.lib()
    h = C.c_void_p()
    assert L.dspfx_cancel_create(None, C.byref(h)) == INVALID
    assert L.dspfx_cancel_last_error(None)
    assert L.dspfx_cancel_create(C.byref(dspfx._CancelDesc(dspfx.ABI_VERSION, 0, 1000, 128, 0, 64, 0, 0)), None) == INVALID
    assert L.dspfx_cancel_destroy(None) == INVALID
    assert L.dspfx_cancel_run(None, None, None, None, 128, None) == INVALID
    assert L.dspfx_cancel_set(None, None, None, None, None, None, 0, 0) == INVALID
    assert L.dspfx_cancel_load(None, None, 1, 0, 0, 0) == INVALID
    assert L.dspfx_cancel_drop(None, 0, 0) == INVALID
    assert L.dspfx_cancel_reset(None, 0, 0) == INVALID
    for name in ("present", "lengths", "sliders", "delays", "adapting"):
        assert getattr(L, f"dspfx_cancel_{name}")(None, None, 0, 0) == INVALID
    assert L.dspfx_cancel_weights_view(None, None) == INVALID
    assert L.dspfx_cancel_levels_view(None, None) == INVALID
    assert L.dspfx_cancel_plan(8, 64, 0, None) == 0


def test_python_refuses_arrays_of_different_lengths_without_a_bank(dspfx):
    bank = object.__new__(dspfx.ChannelCancellers)
    bank.channels = 8
    with pytest.raises(dspfx.DspfxError) as e:
        bank.set(taps=[4, 4], mu=[0.5, 0.5, 0.5])
    assert "different numbers of channels" in str(e.value)
    with pytest.raises(dspfx.DspfxError) as e:
        bank.load(np.zeros((2, 2, 2), F))
    assert "[T]" in str(e.value)
    bank.h = None                                                              # (nothing to destroy)


def _protos(text, fn_re):
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()]) for m in re.finditer(fn_re, text)}


def test_header_exports_ctypes_and_ffi_name_the_same_entry_points(dspfx):
    body = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    c = {k: v for k, v in _protos(body, r"\b(dspfx_cancel_\w+)\s*\(([^;{}]*?)\)\s*;").items()}
    rust = _protos(re.sub(r"//[^\n]*", "", FFI), r"pub fn (dspfx_cancel_\w+)\s*\(([^)]*)\)")
    assert set(c) == set(NAMES) == set(rust) == {e for e in dspfx.EXPORTS if e.startswith("dspfx_cancel_")}
    assert rust == c
    L = dspfx.lib()
    for name in NAMES:
        assert len(getattr(L, name).argtypes) == c[name], name
    for k in ("abi_version", "device", "n_channels", "max_frames", "tile_channels", "max_taps", "max_delay", "general_only"):
        assert k in [f[0] for f in dspfx._CancelDesc._fields_]
    m = re.search(r"pub struct dspfx_cancel_desc\s*\{(.*?)\}", re.sub(r"//[^\n]*", "", FFI), re.S)
    assert [f.strip().split(":")[0].replace("pub ", "").strip() for f in m.group(1).split(",") if f.strip()] == [f[0] for f in dspfx._CancelDesc._fields_]
    assert dspfx.CANCEL_MAX_TAPS == 1024 and "#define DSPFX_CANCEL_MAX_TAPS 1024u" in HDR
    assert dspfx.CANCEL_MAX_DELAY == 65535 and "#define DSPFX_CANCEL_MAX_DELAY 65535u" in HDR
