"""An independent numpy restatement of the talker bank (include/dspfx.h, dspfx_talkers_*): the f32 envelope recurrence, the gate's
ramp, the selection by sort, and the order of one run.  tests/test_talkers_cpu.py holds its envelope to the oracle's Envelope node
bit for bit; tests/test_talkers_gpu.py holds the bank to it bit for bit.  Blocks are [n_frames][N] frame-major float32."""
import ctypes
import ctypes.util

import numpy as np

F = np.float32
AUTO, OPEN, SHUT = 0, 1, 2
NO_ROOM = 0xFFFFFFFF
MAX_ROOM, MAX_TOP = 1024, 8

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def envelope_gain(frames):
    """dasp_envelope's calc_gain with the C library's powf, which is what the reference calls"""
    frames = F(frames)
    if frames == 0:
        return F(0.0)
    with np.errstate(all="ignore"):
        return F(_libm.powf(F(2.71828182845904523536028747135266250), F(-1.0) / frames))


def noise(rng, nf, n):
    return rng.uniform(-1.0, 1.0, (nf, n)).astype(F)


def select(levels, room_of, groups, top, floor=0.0, pins=None):
    """-> (talkers int32[G][8], talker_levels f32[G][8], target f32[N]) by sorting every room's candidates"""
    levels = np.asarray(levels, F)
    room_of = np.asarray(room_of, np.uint32)
    n = len(levels)
    pins = np.zeros(n, np.uint8) if pins is None else np.broadcast_to(np.asarray(pins, np.uint8), (n,))
    top = np.broadcast_to(np.asarray(top, np.uint8), (groups,))
    talkers = np.full((groups, MAX_TOP), -1, np.int32)
    tl = np.zeros((groups, MAX_TOP), F)
    target = (pins == OPEN).astype(F)
    with np.errstate(invalid="ignore"):
        cand = (pins == AUTO) & (levels > F(floor))
    for g in range(groups):
        m = np.flatnonzero((room_of == g) & cand)
        order = sorted(m, key=lambda c: (-float(levels[c]), int(c)))[:int(top[g])]
        for t, c in enumerate(order):
            talkers[g, t] = c
            tl[g, t] = levels[c]
            target[c] = 1.0
    return talkers, tl, target


class Talkers:
    """The bank's methods with the bank's meaning; a store that the bank refuses returns False and changes nothing."""

    def __init__(self, n, group_start, top=3):
        gs = np.asarray(group_start, np.int64)
        self.n, self.groups = int(n), len(gs) - 1
        self.room = np.zeros(n, np.uint32)
        for g in range(self.groups):
            self.room[gs[g]:gs[g + 1]] = g
        self.env, self.level = np.zeros(n, F), np.zeros(n, F)
        self.gate, self.target = np.ones(n, F), np.ones(n, F)
        self.ga, self.gr = np.zeros(n, F), np.zeros(n, F)
        self.pin = np.zeros(n, np.uint8)
        self.top = np.full(self.groups, top, np.uint8)
        self.floor = F(0.0)
        self.talkers = np.full((self.groups, MAX_TOP), -1, np.int32)
        self.talker_levels = np.zeros((self.groups, MAX_TOP), F)

    def _span(self, first, count, values, total):
        if values is not None and np.ndim(values) != 0:
            count = np.size(values)
        elif count is None:
            count = total - first
        return (first, first + count) if 0 <= first and first + count <= total else None

    def set_detector(self, attack=None, release=None, first_channel=0, count=None):
        span = self._span(first_channel, count, attack if np.ndim(attack) else release, self.n)
        if span is None:
            return False
        a, b = span
        for v, tab in ((attack, self.ga), (release, self.gr)):
            if v is not None:
                tab[a:b] = [envelope_gain(f) for f in np.broadcast_to(np.asarray(v, F).reshape(-1), (b - a,))]
        return True

    def set_pin(self, pins, first_channel=0, count=None):
        span = self._span(first_channel, count, pins, self.n)
        if span is None or np.max(pins) > SHUT:
            return False
        self.pin[span[0]:span[1]] = pins
        return True

    def set_top(self, tops, first_room=0, count=None):
        span = self._span(first_room, count, tops, self.groups)
        if span is None or np.min(tops) < 1 or np.max(tops) > MAX_TOP:
            return False
        self.top[span[0]:span[1]] = tops
        return True

    def set_floor(self, floor):
        self.floor = F(floor)

    def assign(self, ids, first_channel=0):
        ids = np.atleast_1d(np.asarray(ids, np.uint32))
        if first_channel + len(ids) > self.n or ((ids >= self.groups) & (ids != NO_ROOM)).any():
            return False
        room = self.room.copy()
        room[first_channel:first_channel + len(ids)] = ids
        if np.bincount(room[room != NO_ROOM], minlength=self.groups).max() > MAX_ROOM:
            return False
        self.room = room
        return True

    def reset(self, first_channel=0, count=None):
        b = self.n if count is None else first_channel + count
        self.env[first_channel:b] = 0.0
        self.level[first_channel:b] = 0.0
        self.gate[first_channel:b] = 1.0
        self.target[first_channel:b] = 1.0

    def room_of(self):
        return self.room.copy()

    def counts(self):
        return np.bincount(self.room[self.room != NO_ROOM], minlength=self.groups).astype(np.uint32)

    def run(self, x, gate=True):
        """one block: gate with the targets the run before left, meter, select; -> the gated block (None with gate=False).
        self.envs is every frame's envelope, [n_frames][N]"""
        x = np.asarray(x, F)
        nf = x.shape[0]
        env, lvl = self.env.copy(), np.zeros(self.n, F)
        y = np.empty_like(x) if gate else None
        self.envs = np.empty_like(x)
        with np.errstate(all="ignore"):
            for f in range(nf):
                xf = x[f]
                d = np.where(xf < 0, -xf, xf)
                gain = np.where(env < d, self.ga, self.gr)
                env = d + (env + (-d)) * gain
                self.envs[f] = env
                lvl = np.where(env > lvl, env, lvl)
                if gate:
                    r = F(f + 1) / F(nf)
                    y[f] = xf * (self.gate + (self.target - self.gate) * r)
        assert env.dtype == F and (y is None or y.dtype == F)
        self.env, self.level = env, lvl
        if gate:
            self.gate = self.target.copy()
        self.talkers, self.talker_levels, self.target = select(lvl, self.room, self.groups, self.top, self.floor, self.pin)
        return y

    def run_blocks(self, x, nf=128, gate=True):
        outs = [self.run(x[f0:f0 + nf], gate) for f0 in range(0, len(x), nf)]
        return np.concatenate(outs) if gate else None
