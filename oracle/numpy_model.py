"""Independent numpy-float32 model of the reference effect arithmetic.

TEST INFRASTRUCTURE ONLY -- PARITY UNPINNED (see dspfx_oracle.h).  Written
separately from the C oracle (different language, vectorised where the maths
allows) so the two restatements can cross-check each other and generate the
golden vectors in tests/golden/.  Citations relative to /root/reference/.
"""
from __future__ import annotations

import numpy as np

F = np.float32
BUF_SIZE = 128  # dsp-stuff/src/node.rs:257

# The reference's f32 math-library calls (Rust's f32::tanh / sin / atan / exp / powf go to the platform's libm).  By default
# numpy's own float32 routines -- and, where this model always took the correctly rounded value, float64 rounded once
# ("sin_cr", "powf").  A test that wants to compare everything AROUND these calls bit for bit with the C oracle swaps in the
# platform's routines here (tests/test_edge_values_cpu.py).
LIBM = {
    "tanh": np.tanh, "sin": np.sin, "atan": np.arctan, "exp": np.exp,
    "sin_cr": lambda v: np.sin(np.asarray(v, F).astype(np.float64)).astype(F),
    "powf": lambda base, x: F(np.power(np.float64(base), np.float64(x))),
}


def link_scale(x):
    """node.rs:162-194 with ONE connected pipe: (0 + x) / f32(0.0001 + 1)."""
    div = F(F(0.0001) + F(1.0))
    return ((F(0.0) + np.asarray(x, F)) / div).astype(F)


def slider_input(ctl, lo, hi):
    """dsp-stuff-derive/src/lib.rs:141-146"""
    y = (np.asarray(ctl, F) + F(1.0)) / F(2.0)
    z = np.where(y < F(0), F(0), y)
    z = np.where(z > F(1), F(1), z).astype(F)
    return (F(lo) + (F(hi) - F(lo)) * z).astype(F)


def gain(x, level):
    """gain.rs:33-37"""
    return (np.asarray(x, F) * F(level)).astype(F)


class Biquad:
    """biquad.rs:48-88 + biquad 0.4.2 DirectForm1 (restated)."""

    def __init__(self, a0=1.0, a1=-0.24, a2=0.0, b0=0.758, b1=0.0, b2=0.0, normalise=True):
        a0 = F(a0)
        if normalise:  # regenerate_filter, biquad.rs:62-76
            self.a1, self.a2 = F(a1) / a0, F(a2) / a0
            self.b0, self.b1, self.b2 = F(b0) / a0, F(b1) / a0, F(b2) / a0
        else:          # initial_filter, biquad.rs:48-60
            self.a1, self.a2, self.b0, self.b1, self.b2 = F(a1), F(a2), F(b0), F(b1), F(b2)
        self.x1 = self.x2 = self.y1 = self.y2 = F(0)

    def run(self, x):
        out = np.empty(len(x), F)
        for i, v in enumerate(np.asarray(x, F)):
            y = F(F(F(F(self.b0 * v) + F(self.b1 * self.x1)) + F(self.b2 * self.x2))
                  - F(self.a1 * self.y1)) - F(self.a2 * self.y2)
            y = F(y)
            self.x2, self.x1, self.y2, self.y1 = self.x1, v, self.y1, y
            out[i] = y
        return out


class OnePole:
    def __init__(self, ratio=0.5, high=False):
        self.r, self.z, self.high = F(ratio), F(0), high

    def run(self, x):
        out = np.empty(len(x), F)
        one_m = F(F(1.0) - self.r)
        for i, v in enumerate(np.asarray(x, F)):
            t = F(F(v * one_m) + F(self.r * self.z))
            if self.high:   # high_pass.rs:36-39
                self.z = t
                out[i] = F(v - t)
            else:           # low_pass.rs:36-39
                out[i] = t
                self.z = t
        return out


def delay_len_from_seconds(seconds, page_round=False):
    """reverb.rs:58: ((seconds * 48000.0) as usize).max(128), f32 product, truncating cast; page_round: the reading in which
    rivulet rounds the ring to whole 4 KiB pages (1024 f32)."""
    s = F(F(seconds) * F(48000.0))
    d = 0 if not s > 0 else int(min(float(s), 4294967295.0))
    d = max(d, 128)
    return (d + 1023) // 1024 * 1024 if page_round else d


class Reverb:
    """reverb.rs:76-110 as y[n] = x[n] + decay*y[n-D], zero history."""

    def __init__(self, d, decay=0.5):
        self.hist = np.zeros(int(d), F)
        self.d, self.decay, self.n = int(d), F(decay), 0

    def run(self, x):
        out = np.empty(len(x), F)
        for i, v in enumerate(np.asarray(x, F)):
            p = (self.n + i) % self.d
            y = F(v + F(self.hist[p] * self.decay))
            self.hist[p] = y
            out[i] = y
        self.n += len(x)
        return out


def _clip(s):
    s = np.asarray(s, F)
    return np.where(s < F(-1), F(-1), np.where(s > F(1), F(1), s)).astype(F)


def _signum(x):
    x = np.asarray(x, F)
    s = np.where(np.signbit(x), F(-1), F(1)).astype(F)
    return np.where(np.isnan(x), x, s).astype(F)


def distort(x, level, mode):
    """distort.rs:63-172 (one reference block for Fuzz)."""
    x = np.asarray(x, F)
    L = F(level)
    if mode != 4 and L < F(0.001):
        return x.copy()
    with np.errstate(all="ignore"):
        if mode == 0:
            return (_clip(x * L) / L).astype(F)
        if mode == 1:
            s = (x * L).astype(F)
            cube = ((s * s).astype(F) * s).astype(F)
            mid = (s - (cube / F(3.0)).astype(F)).astype(F)
            t = np.where(s > F(1), F(2.0) / F(3.0),
                         np.where((s >= F(-1)) & (s <= F(1)), mid, F(-2.0) / F(3.0))).astype(F)
            return (_clip(t) / L).astype(F)
        if mode == 2:
            return LIBM["tanh"]((x * L).astype(F)).astype(F)
        if mode == 3:
            den = ((np.abs(x) * L).astype(F) + F(1)).astype(F)
            return (_signum(x) * (F(1) - (F(1) / den).astype(F)).astype(F)).astype(F)
        if mode == 4:
            lv = np.full(len(x), L, F)
            mx = np.abs(x).max() if not np.isnan(x).any() else F(np.nan)
            q = (_clip(x * lv) / mx).astype(F)
            z = (-np.abs(F(1) - LIBM["exp"](-np.abs(q)).astype(F))).astype(F)
            mz = np.abs(z).max() if not np.isnan(z).any() else F(np.nan)
            y = (_clip((z * mx).astype(F)) / mz).astype(F)
            my = np.abs(y).max() if not np.isnan(y).any() else F(np.nan)
            return ((y * mx).astype(F) / my).astype(F)
        if mode == 5:
            return LIBM["sin"]((x * L).astype(F)).astype(F)
        if mode == 6:
            return LIBM["atan"]((x * L).astype(F)).astype(F)
        if mode == 7:
            v = (x * L).astype(F)
            return ((v * v).astype(F) * _signum(v)).astype(F)
        if mode == 8:
            v = (x * L).astype(F)
            v2 = (v * v).astype(F)
            v4 = (v2 * v2).astype(F)
            return (((F(8) * v4).astype(F) - (F(8) * v2).astype(F)).astype(F) + F(1)).astype(F)
    raise ValueError(mode)


def overdrive(x, boost, drive, level):
    """overdrive.rs:31-43"""
    x = np.asarray(x, F)
    if F(level) < F(0.001):
        return x.copy()
    a = (x * F(boost)).astype(F)
    b = (F(np.pi / 4) * a).astype(F)
    c = LIBM["atan"](b).astype(F)
    d = (F(2 / np.pi) * c).astype(F)
    mix = ((F(drive) * d).astype(F) + (F(F(1) - F(drive)) * x).astype(F)).astype(F)
    return (mix * F(level)).astype(F)


def chebyshev(x, level_pos, level_neg):
    """chebyshev.rs:28-42"""
    x = np.asarray(x, F)
    out = x.copy()
    lp, ln = F(level_pos), F(level_neg)
    pos = x >= F(0)
    if lp >= F(0.001):
        out[pos] = (LIBM["tanh"]((x[pos] * lp).astype(F)).astype(F) / LIBM["tanh"](lp)).astype(F)
    neg = ~pos
    if ln >= F(0.001):
        out[neg] = (LIBM["tanh"]((x[neg] * ln).astype(F)).astype(F) / LIBM["tanh"](ln)).astype(F)
    return out


class VecDeque:
    """Index bookkeeping of Rust's std VecDeque<f64> (the part Fir's `as_slices` split depends on, fir.rs:201-202):
    a ring of capacity `cap` (0, then doubling from 4: RawVec's amortised growth for 8-byte elements), `head` the
    physical index of the front, `len` elements.  Growing a wrapped ring moves its shorter part
    (VecDeque::handle_capacity_increase): contiguous -> nothing; short wrapped front part -> copied behind the old
    capacity; otherwise the [head, old_cap) part moves to the end of the new buffer."""

    def __init__(self):
        self.buf = np.zeros(0, np.float64)
        self.head, self.len = 0, 0

    @property
    def cap(self):
        return len(self.buf)

    def push_back(self, v):
        if self.len == self.cap:
            old = self.cap
            new = old * 2 if old else 4
            nb = np.zeros(new, np.float64)
            nb[:old] = self.buf
            if self.head > old - self.len:                       # wrapped
                head_len = old - self.head
                tail_len = self.len - head_len
                if head_len > tail_len and new - old >= tail_len:
                    nb[old:old + tail_len] = nb[:tail_len]
                else:
                    nb[new - head_len:new] = self.buf[self.head:old]
                    self.head = new - head_len
            self.buf = nb
        self.buf[(self.head + self.len) % self.cap] = v
        self.len += 1

    def pop_front(self):
        self.head = (self.head + 1) % self.cap
        self.len -= 1

    def as_slices(self):
        if self.head + self.len <= self.cap:
            return self.buf[self.head:self.head + self.len], self.buf[:0]
        return self.buf[self.head:], self.buf[:self.head + self.len - self.cap]


class Fir:
    """fir.rs:180-224: per sample push, pop at most ONE sample when the deque is longer than the taps, then
    `a` = sum over the deque's first slice zipped with the taps (f64, sequential, cast to f32), `b` likewise over the
    second slice with taps[n_a..]; out = (a + b) * divisor.  `set_taps` is the impulse-response reload
    (fir.rs:153-171): it replaces the taps ONLY -- `state` is never cleared (fir.rs:64-65), so a deque longer than
    the new tap count stays longer (its oldest samples pair with the taps: an extra delay of len - T samples) and a
    shorter one goes on growing front-aligned like the warm-up."""

    def __init__(self, taps_reversed, average=False):
        self.state = VecDeque()
        self.average = average
        self.set_taps(taps_reversed)

    def set_taps(self, taps_reversed):
        self.t = np.asarray(taps_reversed, np.float64).copy()

    @staticmethod
    def _dot(xs, cs):
        acc = np.float64(0)
        for x, c in zip(xs, cs):            # zip stops at the shorter; sequential f64 sum like Iterator::sum
            acc += x * c
        return F(acc)

    def run(self, x):
        out = np.empty(len(x), F)
        T = len(self.t)
        div = F(1.0) / F(T) if self.average else F(1.0)          # fir.rs:187-190
        for i, v in enumerate(np.asarray(x, F)):
            self.state.push_back(np.float64(v))
            if self.state.len > T:
                self.state.pop_front()
            a, b = self.state.as_slices()
            n_a = len(a)
            fa = self._dot(a, self.t)
            fb = self._dot(b, self.t[n_a:]) if n_a < T else F(0.0)
            out[i] = F(F(fa + fb) * div)
        return out


def add(a, b):
    return (np.asarray(a, F) + np.asarray(b, F)).astype(F)


def mix(a, b, ratio):
    """mix.rs:41-46"""
    r = F(ratio)
    return ((np.asarray(b, F) * r).astype(F) + (np.asarray(a, F) * F(F(1) - r)).astype(F)).astype(F)


class SignalGen:
    """signal_gen.rs:57-129, one channel.  mode: 0 Sine, 1 Triangle, 2 Square, 3 Constant.
    float32 sin is taken as the correctly rounded value (numpy's float64 sin, rounded once)."""

    TAU = F(6.283185307179586)

    def __init__(self, amplitude=0.5, frequency=100.0, mode=0):
        self.amplitude, self.frequency, self.mode = F(amplitude), F(frequency), mode
        self.clock = F(0.0)

    def process(self, n=BUF_SIZE, amplitude=None, frequency=None):
        """One block of n frames; amplitude / frequency are optional per-sample (control port) arrays."""
        amp = np.full(n, self.amplitude, F) if amplitude is None else np.asarray(amplitude, F)
        frq = np.full(n, self.frequency, F) if frequency is None else np.asarray(frequency, F)
        if self.mode == 3:
            return amp.copy()
        step = (frq / F(48000.0)).astype(F)
        total = np.empty(n, F)
        acc = F(0.0)
        for i in range(n):            # sequential f32 accumulation (signal_gen.rs:65)
            acc = F(acc + step[i])
            total[i] = acc
        ph = (self.clock + total).astype(F)
        if self.mode == 0:
            out = (LIBM["sin_cr"]((ph * self.TAU).astype(F)) * amp).astype(F)
        elif self.mode == 1:
            out = ((F(2.0) * np.fmod(ph, F(1.0)).astype(F) - F(1.0)).astype(F) * amp).astype(F)
        else:
            out = (np.where(total > F(0.5), F(1.0), F(-1.0)).astype(F) * amp).astype(F)
        self.clock = F(np.fmod(F(self.clock + acc), F(1.0)))
        return out


class Envelope:
    """envelope.rs:34-52 over dasp_envelope 0.11.0 Detector<f32, Peak<FullWave>> (restated as recalled, see
    dspfx_oracle.h): env = d + (env - d) * gain, d = |x|, gain = attack gain while env < d else release gain."""

    E = F(2.718281828459045)

    def __init__(self, attack=0.0, release=0.0):
        self.attack, self.release = F(attack), F(release)
        self.env = F(0.0)

    @classmethod
    def calc_gain(cls, n_frames):
        n = F(n_frames)
        if n == F(0):
            return F(0.0)
        # powf(e_f32, x): evaluated in float64 and rounded once (glibc powf is within 1 ulp of that)
        return F(LIBM["powf"](cls.E, F(-1.0) / n))

    def process(self, x):
        x = np.asarray(x, F)
        ga, gr = self.calc_gain(self.attack), self.calc_gain(self.release)
        out = np.empty_like(x)
        l = self.env
        for i in range(x.size):
            d = -x[i] if x[i] < F(0) else x[i]
            g = ga if l < d else gr
            l = F(d + F(F(l + (-d)) * g))
            out[i] = l
        self.env = l
        return out


# --------------------------------------------------------------------------------------------------------------
# Node wrappers, chains and whole graphs: the second restatement of SimpleNode::process for every kind, the derive
# macro's `<field>_input` helpers (dsp-stuff-derive/src/lib.rs:122-161: per-sample map of a connected slider port and
# the latch of its first value into the slider) and the `Perform` wrapper's port semantics (node.rs:162-194,267-352).
# Numeric kind / mode values are those of include/dspfx.h.

K_GAIN, K_BIQUAD, K_LOW_PASS, K_HIGH_PASS, K_REVERB, K_DISTORT, K_OVERDRIVE, K_CHEBYSHEV, K_FIR, K_ADD, K_MIX, \
    K_SIGNAL_GEN, K_ENVELOPE = range(13)
_SLIDER_RANGES = {K_GAIN: [(0.0, 10.0)], K_DISTORT: [(0.0, 30.0)], K_OVERDRIVE: [(0.0, 30.0), (0.0, 1.0), (0.0, 1.0)],
                  K_MIX: [(0.0, 1.0)], K_SIGNAL_GEN: [(-1.0, 1.0), (0.1, 20000.0)]}


def collect_and_average(pipes, n):
    """node.rs:162-194: a zeroed buffer, every connected pipe added in link order, one division by the f32 count
    0.0001 (+ 1.0 per pipe).  Returns (buffer, present)."""
    buf = np.zeros(n, F)
    num = F(0.0001)
    for p in pipes:
        num = F(num + F(1.0))
        buf = (buf + np.asarray(p, F)).astype(F)
    with np.errstate(all="ignore"):
        return (buf / num).astype(F), len(pipes) > 0


def distort_per_sample(x, level, mode):
    """distort.rs:63-145 with a level per sample (`apply` zips the level block, 88-94 etc.); Fuzz is block-global."""
    x, level = np.asarray(x, F), np.asarray(level, F)
    if mode == 4:
        with np.errstate(all="ignore"):
            def amax(v):
                return F(np.nan) if np.isnan(v).any() else np.abs(v).max()       # max_by(total_cmp): NaN is largest
            mx = amax(x)
            q = (_clip((x * level).astype(F)) / mx).astype(F)
            z = (-np.abs(F(1) - LIBM["exp"](-np.abs(q)).astype(F))).astype(F)
            mz = amax(z)
            y = (_clip((z * mx).astype(F)) / mz).astype(F)
            my = amax(y)
            return ((y * mx).astype(F) / my).astype(F)
    out = np.empty_like(x)
    for lv in np.unique(level):                                   # the scalar-level restatement, level by level
        sel = level == lv
        out[sel] = distort(x[sel], lv, mode)
    nan = np.isnan(level)                                         # `level < 0.001` is false for NaN: the formula runs
    if nan.any():
        with np.errstate(all="ignore"):
            out[nan] = (x[nan] * level[nan]).astype(F)
    return out


class NodeModel:
    """One reference node for one mono channel: `process(a, b, ctl)` on one block of <= 128 frames, `a` / `b` the
    already averaged port buffers (zeros when unconnected), ctl[k] the averaged buffer of slider port k or None."""

    def __init__(self, kind, params=None, mode=0, delay_len=None, taps_reversed=None):
        self.kind, self.mode = int(kind), int(mode or 0)
        self.p = [F(v) for v in (params or [])] + [F(0)] * (8 - len(params or []))
        self.impl = None
        if kind == K_BIQUAD:
            self.impl = Biquad(*[float(v) for v in self.p[:6]])
        elif kind in (K_LOW_PASS, K_HIGH_PASS):
            self.impl = OnePole(self.p[0], high=kind == K_HIGH_PASS)
        elif kind == K_REVERB:                                    # make_buffer(): 128 zeros (reverb.rs:44-52) unless D is named
            if params is None or len(params) < 2:                 # no seconds slider given: the default one (0.5 s) for a fresh
                self.p[1] = F(0.0) if delay_len else F(0.5)       # node, none to refresh from beside an explicit ring
            self.seconds_given = bool(self.p[1] > 0)              # 0 in a descriptor: "not given"; a STORED 0.0 is a value (128 samples)
            # ... 128 zeros, or the 1024 of the page-rounded reading (mode bit 0): make_buffer() is refresh_seconds' three calls
            self.impl = Reverb(delay_len or delay_len_from_seconds(0.0, bool(self.mode & 1)), self.p[0])
        elif kind == K_FIR:
            self.impl = Fir(taps_reversed if taps_reversed is not None else [1.0], average=self.mode == 1)
        elif kind == K_SIGNAL_GEN:
            self.impl = SignalGen(self.p[0], self.p[1], self.mode)
        elif kind == K_ENVELOPE:
            self.impl = Envelope(self.p[0], self.p[1])

    def set_param(self, idx, v):
        self.p[idx] = F(v)
        if self.kind == K_REVERB and idx == 1:
            self.seconds_given = True
        if self.kind == K_BIQUAD:                                 # after_settings_change: new filter, state reset
            self.impl = Biquad(*[float(q) for q in self.p[:6]])
        elif self.kind in (K_LOW_PASS, K_HIGH_PASS):
            self.impl.r = F(v)
        elif self.kind == K_REVERB:
            # after_settings_change = Reverb::refresh_seconds (reverb.rs:19, 55-71), run by the generated render() whenever
            # ANY widget of the node changed (dsp-stuff-derive/src/lib.rs:487-497, 560-568): decay AND seconds both swap in
            # a NEW zero ring of max((seconds * 48000) as usize, 128) samples -- of the current length when the node was
            # not given its seconds slider (the ring length is explicit in this restatement)
            d = delay_len_from_seconds(self.p[1], bool(self.mode & 1)) if self.seconds_given else self.impl.d
            self.impl = Reverb(d, self.p[0])
        elif self.kind == K_ENVELOPE:
            self.impl.attack, self.impl.release = self.p[0], self.p[1]

    def _slider(self, k, ctl, n):
        """`<field>_input`: connected -> per-sample map + latch of element 0; else the slider's value."""
        lo, hi = _SLIDER_RANGES[self.kind][k]
        c = ctl[k] if ctl is not None and k < len(ctl) else None
        if c is not None:
            v = slider_input(c, lo, hi)
            if n:
                self.p[k] = F(v[0])
            return v
        return np.full(n, self.p[k], F)

    def process(self, a, b=None, ctl=None):
        a = np.asarray(a, F)
        n = len(a)
        k = self.kind
        with np.errstate(all="ignore"):
            if k == K_GAIN:
                return (a * self._slider(0, ctl, n)).astype(F)
            if k in (K_BIQUAD, K_LOW_PASS, K_HIGH_PASS, K_REVERB, K_FIR):
                return self.impl.run(a)
            if k == K_DISTORT:
                return distort_per_sample(a, self._slider(0, ctl, n), self.mode)
            if k == K_OVERDRIVE:                                  # overdrive.rs:58-72 (helpers in field order)
                boost, drive, level = self._slider(0, ctl, n), self._slider(1, ctl, n), self._slider(2, ctl, n)
                t = (F(np.pi / 4) * (a * boost).astype(F)).astype(F)
                d = (F(2 / np.pi) * LIBM["atan"](t).astype(F)).astype(F)
                m = ((drive * d).astype(F) + ((F(1) - drive).astype(F) * a).astype(F)).astype(F)
                return np.where(level < F(0.001), a, (m * level).astype(F)).astype(F)
            if k == K_CHEBYSHEV:
                return chebyshev(a, self.p[0], self.p[1])
            if k == K_ADD:
                return add(a, np.zeros(n, F) if b is None else b)
            if k == K_MIX:
                r = self._slider(0, ctl, n)
                bb = np.zeros(n, F) if b is None else np.asarray(b, F)
                return ((bb * r).astype(F) + (a * (F(1) - r).astype(F)).astype(F)).astype(F)
            if k == K_SIGNAL_GEN:
                am = self._slider(0, ctl, n)
                fr = self._slider(1, ctl, n)
                self.impl.mode = self.mode
                return self.impl.process(n, am, fr)
            if k == K_ENVELOPE:
                return self.impl.process(a)
        raise ValueError(k)


def make_node(desc):
    """desc = NodeSpec.oracle_desc(): {"kind", "params", "mode", "delay_len", "taps_reversed"}."""
    return NodeModel(desc["kind"], desc.get("params"), desc.get("mode") or 0, desc.get("delay_len"), desc.get("taps_reversed"))


def chain_run(nodes, x, link_flags=3, side=None, ctl=None, block=BUF_SIZE):
    """One channel through a linear chain of NodeModel (state carried in them), block by block.
    link_flags bit 0: the hops between chain nodes -- and every side / control link -- go through collect_and_average
    with one pipe; bit 1: so does the hop into the first node.  ctl: {(node, slider): signal}."""
    x = np.asarray(x, F)
    out = np.empty_like(x)
    for f0 in range(0, len(x), block):
        sl = slice(f0, min(len(x), f0 + block))
        cur = x[sl]
        n = len(cur)
        for k, node in enumerate(nodes):
            hop = (link_flags & 2) if k == 0 else (link_flags & 1)
            a = collect_and_average([cur], n)[0] if hop else cur
            b = None
            if side is not None and node.kind in (K_ADD, K_MIX):
                b = np.asarray(side, F)[sl]
                if link_flags & 1:
                    b = collect_and_average([b], n)[0]
            cs = None
            if ctl:
                cs = [None, None, None]
                for (kk, j), sig in ctl.items():
                    if kk == k:
                        c = np.asarray(sig, F)[sl]
                        cs[j] = collect_and_average([c], n)[0] if link_flags & 1 else c
            cur = node.process(a, b, cs)
        out[sl] = cur
    return out


def run_graph(graph, x, block=BUF_SIZE):
    """A parsed saved graph (dsp_stuff_amd.graph.Graph: structure and node descriptors only) evaluated the way the
    reference's scheduler does, node by node per 128-frame block: every input port -- main, "b", slider ports --
    is collect_and_average over its pipes in link order (node.rs:290-299), a slider port without pipes keeps its
    slider (get_checked, node.rs:230-237), then `process`.  x: [n_frames][n_channels] -> the Output node's signal."""
    x = np.asarray(x, F)
    nf_total, N = x.shape
    out = np.empty_like(x)
    for c in range(N):
        nodes = {i: make_node(n.spec.oracle_desc()) for i, n in graph.nodes.items() if n.spec is not None}
        for f0 in range(0, nf_total, block):
            nf = min(block, nf_total - f0)
            val = {-1: np.zeros(nf, F)}                       # graph.ZERO: the unselected output port of a demux
            for nid in graph.order:
                n = graph.nodes[nid]
                if n.typename == "input":
                    val[nid] = x[f0:f0 + nf, c]
                    continue
                a = collect_and_average([val[s] for s in n.main], nf)[0]
                if n.typename == "output":
                    out[f0:f0 + nf, c] = a
                    continue
                b = collect_and_average([val[s] for s in n.side], nf)[0] if n.side else None
                cs = None
                if n.ctl:
                    cs = [None, None, None]
                    for k, srcs in n.ctl.items():
                        cs[k] = collect_and_average([val[s] for s in srcs], nf)[0]
                val[nid] = nodes[nid].process(a, b, cs)
    return out
