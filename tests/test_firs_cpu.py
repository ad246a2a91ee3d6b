"""The channel-FIR bank without a GPU: the restatement the GPU tests lean on (firs_ref: one oracle FIR node and one numpy VecDeque
per channel) against oracle/numpy_model.Fir bit for bit through the fill phase, a steady state long enough for `head` to wrap
twice, a reload to a shorter and to a longer response, Average mode, reset, and drop then set; a plain numpy model of ONE LANE of
firs_kernels.hip -- the ring in time, the three deque words stepped per frame, the general body and the steady body with its
sliding window and its running sum per frame, cut where the first slice ends -- against the same, the check that the kernel's indexing is the reference's
arithmetic; the store rules; dspfx_firs_plan against its written formula; the create refusals and the argument checks that need
no device; header, EXPORTS, ctypes signatures and ffi.rs agree."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import firs_ref as R
import numpy_model as M
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
FFI = open(os.path.join(ROOT, "host", "rust", "src", "ffi.rs")).read()
INVALID = -1
F = np.float32
NAMES = ("dspfx_firs_plan", "dspfx_firs_create", "dspfx_firs_destroy", "dspfx_firs_last_error", "dspfx_firs_run", "dspfx_firs_set_taps",
         "dspfx_firs_set_mode", "dspfx_firs_drop", "dspfx_firs_reset", "dspfx_firs_present", "dspfx_firs_lengths", "dspfx_firs_modes",
         "dspfx_firs_taps", "dspfx_firs_deque")
FB = 16                                          # firs_kernels.hip: frames per block of the steady body


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def signal(n, seed=0x5EED0F12, c=0):
    return np.ascontiguousarray(O.noise(seed, np.arange(c, c + 1), np.arange(n))[:, 0] * F(2.5))


def response(T, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, T)


def frames_for(T):
    """past the fill phase by T + 2 cap frames and more: the split point wraps at least twice"""
    cap = 4
    while cap <= T:
        cap *= 2
    return max(128 + T + 2 * cap, 37 + 128 + 91) + 37


class Lane:
    """one lane of firs_run: `row` is the bank's, len / cap / head and the ring column the channel's"""

    def __init__(self, max_taps):
        self.R = max_taps + FB
        self.ring = np.full(self.R, np.nan, F)   # never cleared
        self.row = 0
        self.len = self.cap = self.head = 0
        self.blocks = 0                          # blocks the steady body took

    def deque_step(self, T):
        if self.len == self.cap:
            old, ncap = self.cap, self.cap * 2 if self.cap else 4
            if self.head > old - self.len:
                head_len = old - self.head
                tail_len = self.len - head_len
                if not (head_len > tail_len and ncap - old >= tail_len):
                    self.head = ncap - head_len
            self.cap = ncap
        self.len += 1
        if self.len > T:
            self.head = 0 if self.head + 1 == self.cap else self.head + 1
            self.len -= 1
        return min(self.len, self.cap - self.head)

    def frame(self, taps, div, row):
        T, R = len(taps), self.R
        na = self.deque_step(T)
        la = min(na, T)
        lb = min(self.len - na, T - na) if na < T else 0
        r = row + R - self.len + 1
        if r >= R:
            r -= R
        acc = np.float64(0)
        for k in range(la):
            acc = acc + np.float64(self.ring[r]) * taps[k]
            r = 0 if r + 1 == R else r + 1
        accb = np.float64(0)
        for k in range(lb):
            accb = accb + np.float64(self.ring[r]) * taps[na + k]
            r = 0 if r + 1 == R else r + 1
        return F(F(F(acc) + F(accb)) * div)

    def run(self, taps, x, average=False, general_only=False):
        """taps: reversed, f64"""
        T, R = len(taps), self.R
        div = F(1.0) / F(T) if average else F(1.0)
        y = np.empty(len(x), F)
        f = 0
        with np.errstate(all="ignore"):
            while f < len(x):
                if general_only or f + FB > len(x) or self.len != T or self.cap <= T:        # the general body: one frame
                    self.ring[self.row] = x[f]
                    y[f] = self.frame(taps, div, self.row)
                    self.row = 0 if self.row + 1 == R else self.row + 1
                    f += 1
                    continue
                na, r = [], self.row
                for i in range(FB):
                    self.ring[r] = x[f + i]
                    r = 0 if r + 1 == R else r + 1
                    self.head = 0 if self.head + 1 == self.cap else self.head + 1
                    na.append(min(T, self.cap - self.head))
                r = self.row + R - T + 1
                if r >= R:
                    r -= R
                w = [None] * FB
                S, fa = [np.float64(0)] * FB, [F(0)] * FB
                for j in range(FB - 1):
                    w[j] = np.float64(self.ring[r])
                    r = 0 if r + 1 == R else r + 1
                for k in range(T):
                    kk = k % FB
                    w[(kk + FB - 1) % FB] = np.float64(self.ring[r])
                    r = 0 if r + 1 == R else r + 1
                    for i in range(FB):
                        if k == na[i]:                         # the first slice ends: its sum rounded, the second from +0.0
                            fa[i], S[i] = F(S[i]), np.float64(0)
                        S[i] = S[i] + w[(i + kk) % FB] * taps[k]
                for i in range(FB):
                    two = na[i] < T
                    y[f + i] = F(F((fa[i] if two else F(S[i])) + (F(S[i]) if two else F(0))) * div)
                self.row = (self.row + FB) % R
                f += FB
                self.blocks += 1
        return y


def test_the_entry_points_exist_in_the_header_the_exports_and_the_rust_bindings(dspfx):
    L = dspfx.lib()
    assert len(NAMES) == 14
    for name in NAMES:
        assert name in dspfx.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
        assert re.search(r"\b%s\s*\(" % name, HDR), name
        assert re.search(r"pub fn %s\s*\(" % name, FFI), name
    assert sorted(n for n in dspfx.EXPORTS if n.startswith("dspfx_firs_")) == sorted(NAMES)
    assert sorted(set(re.findall(r"\b(dspfx_firs_[a-z_]+)\s*\(", HDR))) == sorted(NAMES)
    assert sorted(set(re.findall(r"pub fn (dspfx_firs_[a-z_]+)\s*\(", FFI))) == sorted(NAMES)
    for m in ("run", "set_taps", "set_mode", "drop", "reset", "present", "lengths", "modes", "taps", "deque", "close"):
        assert hasattr(dspfx.ChannelFirs, m), m
    assert callable(dspfx.firs_plan)
    assert "#define DSPFX_FIRS_NONE 0xFFFFFFFFu" in HDR and dspfx.FIRS_NONE == R.NONE == 0xFFFFFFFF
    assert "#define DSPFX_FIRS_MAX_TAPS 1024u" in HDR and dspfx.FIRS_MAX_TAPS == R.MAX_TAPS == 1024
    assert "pub const DSPFX_FIRS_NONE: u32 = 0xFFFF_FFFF;" in FFI and "pub struct dspfx_firs_desc" in FFI
    fields = ["abi_version", "device", "n_channels", "max_frames", "tile_channels", "max_taps", "general_only"]
    assert [f for f, _ in dspfx._FirsDesc._fields_] == fields
    assert re.search(r"typedef struct dspfx_firs_desc \{" + "".join(r"[^}]*%s;" % f for f in fields) + r"[^}]*\}", HDR)
    m = re.search(r"pub struct dspfx_firs_desc\s*\{(.*?)\}", FFI, re.S)
    assert [f.strip().split(":")[0].replace("pub ", "").strip() for f in m.group(1).split(",") if f.strip()] == fields
    assert (R.BALANCED, R.AVERAGE) == (dspfx.FIR_BALANCED, dspfx.FIR_AVERAGE)
    assert os.path.exists(os.path.join(ROOT, "host", "rust", "src", "channel_firs.rs"))


@pytest.mark.parametrize("average", [False, True])
def test_restatement_and_lane_model_equal_the_numpy_oracle_bit_for_bit(average):
    """every tap count of the list through the fill phase and two wraps of the split point, in runs of 37 + 128 + 91 + the rest;
    the lane model with the steady body, and with the general body alone; the deque words after every run"""
    for T in R.TAP_COUNTS:
        n = frames_for(T)
        x, h = signal(n, c=T), response(T, T)
        want = M.Fir(h[::-1], average).run(x)
        ref = R.ChannelFirs(1)
        assert ref.set_taps(h, mode=R.AVERAGE if average else None)
        lanes = [Lane(64), Lane(64)]
        model = M.VecDeque()
        got, outs, f0 = [], [[], []], 0
        for nf in (37, 128, 91, n - 256):
            got.append(ref.run(x[f0:f0 + nf, None])[:, 0])
            for lane, out, general in zip(lanes, outs, (False, True)):
                out.append(lane.run(h[::-1], x[f0:f0 + nf], average, general))
            for _ in range(nf):
                model.push_back(0.0)
                if model.len > T:
                    model.pop_front()
            words = (model.len, model.cap, model.head)
            assert tuple(ref.deque()[:, 0]) == words, (T, f0)
            for lane in lanes:
                assert (lane.len, lane.cap, lane.head) == words, (T, f0)
            f0 += nf
        assert np.array_equal(bits(np.concatenate(got)), bits(want)), T
        for out, what in zip(outs, ("steady", "general")):
            assert np.array_equal(bits(np.concatenate(out)), bits(want)), (T, what)
        assert lanes[0].blocks > 0 and lanes[1].blocks == 0, T
        assert model.cap > T and n - 128 >= T + 2 * model.cap, "the split point wrapped twice"


def test_reloads_reset_and_drop_then_set():
    """a reload to a shorter response keeps the longer deque (an extra delay), one to a longer response goes on growing; reset
    empties the deque and keeps taps and mode; drop then set is a new node"""
    x = signal(6 * 128)
    h17, h5, h33 = response(17, 1), response(5, 2), response(33, 3)
    fir = M.Fir(h17[::-1])
    ref = R.ChannelFirs(3, max_taps=64)
    lane = Lane(64)
    assert ref.set_taps(h17, first_channel=1, count=1)
    want, got, mod = [], [], []

    def block(b, taps):
        seg = x[b * 128:(b + 1) * 128]
        want.append(fir.run(seg))
        got.append(ref.run(np.stack([seg, seg, seg], axis=1)))
        mod.append(lane.run(taps[::-1], seg))
        assert tuple(ref.deque()[:, 1]) == (fir.state.len, fir.state.cap, fir.state.head) == (lane.len, lane.cap, lane.head)

    block(0, h17)
    fir.set_taps(h5[::-1])
    assert ref.set_taps(h5, first_channel=1, count=1)
    block(1, h5)
    assert fir.state.len == 17, "the deque stays longer than the shorter response"
    fir.set_taps(h33[::-1])
    assert ref.set_taps(h33, first_channel=1, count=1)
    block(2, h33)
    assert fir.state.len == 33
    fir.state = M.VecDeque()
    lane.len = lane.cap = lane.head = 0
    assert ref.reset(1, 1)
    block(3, h33)
    assert list(ref.lengths()) == [0, 33, 0] and list(ref.modes()) == [R.NONE, R.BALANCED, R.NONE]
    fir = M.Fir(h5[::-1], average=True)
    lane.len = lane.cap = lane.head = 0
    assert ref.drop(1, 1) and list(ref.present()) == [0, 0, 0]
    assert ref.set_taps(h5, first_channel=1, count=1, mode=R.AVERAGE)
    seg = x[4 * 128:5 * 128]
    y = ref.run(np.stack([seg, seg, seg], axis=1))
    assert np.array_equal(bits(y[:, 1]), bits(fir.run(seg))) and np.array_equal(bits(y[:, 0]), bits(seg))
    assert np.array_equal(bits(lane.run(h5[::-1], seg, average=True)), bits(y[:, 1]))
    got = np.concatenate(got)
    assert np.array_equal(bits(got[:, 1]), bits(np.concatenate(want)))
    assert np.array_equal(bits(np.concatenate(mod)), bits(np.concatenate(want))), "the lane model"
    assert np.array_equal(bits(got[:, 0]), bits(x[:4 * 128])) and np.array_equal(bits(got[:, 2]), bits(x[:4 * 128])), "no node: a copy"


def test_restatement_store_rules():
    n = 6
    ref = R.ChannelFirs(n, max_taps=16)
    rows = np.stack([response(4, c) for c in range(3)])
    assert ref.set_taps(rows, first_channel=2)
    assert list(ref.present()) == [0, 0, 1, 1, 1, 0] and list(ref.lengths()) == [0, 0, 4, 4, 4, 0]
    assert list(ref.modes()) == [R.NONE, R.NONE, R.BALANCED, R.BALANCED, R.BALANCED, R.NONE]
    assert np.array_equal(ref.h[3], rows[1])
    assert ref.set_mode(R.AVERAGE) and list(ref.modes()) == [R.NONE, R.NONE, R.AVERAGE, R.AVERAGE, R.AVERAGE, R.NONE], "a mode makes no node"
    assert ref.set_taps(response(7, 9), first_channel=1, count=2)
    assert list(ref.lengths()) == [0, 7, 7, 4, 4, 0] and list(ref.modes())[1:3] == [R.BALANCED, R.AVERAGE], "a reload keeps the mode, a new node is Balanced"
    assert ref.set_taps(response(2, 1), first_channel=2, count=1, mode=R.BALANCED) and ref.modes()[2] == R.BALANCED
    before = (ref.present(), ref.lengths(), ref.modes(), [None if h is None else h.copy() for h in ref.h])
    for call in (lambda: ref.set_taps(np.zeros(0)), lambda: ref.set_taps(np.zeros(17)), lambda: ref.set_taps(np.zeros((2, 0)), first_channel=0),
                 lambda: ref.set_taps(np.zeros(4), first_channel=5, count=2), lambda: ref.set_taps(np.zeros((3, 4)), first_channel=4),
                 lambda: ref.set_taps(np.zeros((3, 4)), first_channel=0, count=2), lambda: ref.set_taps(np.zeros((1, 2, 2))),
                 lambda: ref.set_taps(np.zeros(4), mode=2), lambda: ref.set_mode(2), lambda: ref.set_mode(R.AVERAGE, 6, 1),
                 lambda: ref.drop(0, 7), lambda: ref.reset(7, 0), lambda: ref.set_taps(np.float64(1.0))):
        assert call() is False
    after = (ref.present(), ref.lengths(), ref.modes(), ref.h)
    assert all(np.array_equal(u, v) for u, v in zip(before[:3], after[:3]))
    assert all((u is None and v is None) or np.array_equal(u, v) for u, v in zip(before[3], after[3]))
    assert ref.set_taps([np.nan, np.inf, -0.0], first_channel=0, count=1) and np.isnan(ref.h[0][0]), "values are taken as given"


def test_plan_is_the_formula(dspfx):
    """include/dspfx.h: channels * (8 * max_taps + 4 * (max_taps + 16) + 4 + 12)"""
    for n in (1, 70, 256, 1 << 20, 0xFFFFFF00):
        for max_taps in (1, 5, 64, 1024):
            assert dspfx.firs_plan(n, max_taps) == n * (8 * max_taps + 4 * (max_taps + FB) + 4 + 12) == n * (12 * max_taps + 80)
    assert dspfx.firs_plan(1 << 20) == dspfx.firs_plan(1 << 20, 64)
    for n in (0, 1 << 32, 0xFFFFFF01):
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.firs_plan(n, 64)
        assert e.value.status == INVALID and "n_channels" in str(e.value) and "firs" in str(e.value), str(e.value)
    for max_taps in (0, 1025, 0xFFFFFFFF):
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.firs_plan(256, max_taps)
        assert e.value.status == INVALID and "max_taps" in str(e.value) and "firs" in str(e.value), str(e.value)


@pytest.mark.parametrize("kw,word", [
    (dict(max_taps=0), "max_taps"),
    (dict(max_taps=1025), "max_taps"),
    (dict(tile_channels=48), "power of two"),
    (dict(tile_channels=64), "divides"),
    (dict(channels=0), "n_channels"),
    (dict(channels=0xFFFFFF01), "n_channels"),
    (dict(max_frames=0), "max_frames"),
    (dict(max_frames=(1 << 20) + 1), "max_frames"),
])
def test_create_rejects_a_bad_descriptor_before_any_device_work(dspfx, kw, word):
    args = dict(channels=1000, max_taps=64, tile_channels=0, max_frames=128)
    args.update(kw)
    with pytest.raises(dspfx.DspfxError) as e:
        dspfx.ChannelFirs(**args)
    assert e.value.status == INVALID and word in str(e.value) and "firs" in str(e.value), str(e.value)


def test_create_rejects_another_abi_version(dspfx):
    L = dspfx.lib()
    h = C.c_void_p()
    d = dspfx._FirsDesc(dspfx.ABI_VERSION + 1, 0, 1000, 128, 0, 64, 0)
    assert L.dspfx_firs_create(C.byref(d), C.byref(h)) == INVALID and not h.value
    assert b"abi_version" in L.dspfx_firs_last_error(None)


def test_null_arguments_are_invalid(dspfx):
    L = dspfx.lib()
    h = C.c_void_p()
    assert L.dspfx_firs_create(None, C.byref(h)) == INVALID
    assert L.dspfx_firs_last_error(None)
    assert L.dspfx_firs_create(C.byref(dspfx._FirsDesc(dspfx.ABI_VERSION, 0, 1000, 128, 0, 64, 0)), None) == INVALID
    assert L.dspfx_firs_destroy(None) == INVALID
    assert L.dspfx_firs_run(None, None, None, 128, None) == INVALID
    assert L.dspfx_firs_set_taps(None, None, 1, 0, 0, 0, 0) == INVALID
    assert L.dspfx_firs_set_mode(None, 0, 0, 0) == INVALID
    assert L.dspfx_firs_drop(None, 0, 0) == INVALID
    assert L.dspfx_firs_reset(None, 0, 0) == INVALID
    assert L.dspfx_firs_present(None, None, 0, 0) == INVALID
    assert L.dspfx_firs_lengths(None, None, 0, 0) == INVALID
    assert L.dspfx_firs_modes(None, None, 0, 0) == INVALID
    assert L.dspfx_firs_taps(None, 0, None, None) == INVALID
    assert L.dspfx_firs_deque(None, None) == INVALID
    assert L.dspfx_firs_plan(8, 64, None) == 0
