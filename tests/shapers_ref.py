"""A restatement of the channel-shaper bank (include/dspfx.h, dspfx_shapers_*): the kinds, modes and sliders per channel with the
bank's store rules, and a run that is the oracle's own Distort / Overdrive / Chebyshev node, one instance per channel, fed one
128-frame reference block at a time.  tests/test_shapers_cpu.py holds it to oracle.run_channels bit for bit for every kind;
tests/test_shapers_gpu.py holds the bank to it at the bars tests/test_gpu_parity.py holds the engine to.  Blocks are
[n_frames][N] frame-major float32."""
import numpy as np

import oracle as O

F = np.float32
NONE = 0xFFFFFFFF
DISTORT, OVERDRIVE, CHEBYSHEV = 5, 6, 7          # dspfx_kind
N_MODES = 9                                      # dspfx_distort_mode: HardClip .. Chebyshev4
FUZZ = 4
SLIDERS = {DISTORT: 1, OVERDRIVE: 3, CHEBYSHEV: 2}
# a node fresh from the menu (distort.rs:46-50, overdrive.rs:21-28, chebyshev.rs:21-25): every slider 0, mode SoftClip
DEFAULT_MODE = 1


def node(kind, sliders, mode=0):
    """the oracle node of one channel"""
    return O.Node(int(kind), [float(v) for v in sliders[:SLIDERS[int(kind)]]], int(mode) if kind == DISTORT else None)


class ChannelShapers:
    """The bank's methods with the bank's meaning; a store that the bank refuses returns False and changes nothing."""

    def __init__(self, n):
        self.n = int(n)
        self.kind = np.full(n, NONE, np.uint32)
        self.mode = np.full(n, NONE, np.uint32)
        self.p = np.zeros((n, 3), F)

    def _span(self, first, count, values):
        n = None
        for v in values:
            if v is not None and np.ndim(v) != 0:
                n = np.size(v)
        if n is None:
            n = self.n - first if count is None else count
        return (first, first + n) if 0 <= first and n >= 0 and first + n <= self.n else None

    def _set(self, kind, values, mode, first, count):
        span = self._span(first, count, tuple(values) + (mode,))
        if span is None:
            return False
        a, b = span
        if mode is not None:
            m = np.broadcast_to(np.asarray(mode, np.int64).reshape(-1), (b - a,))
            if ((m < 0) | (m >= N_MODES)).any():
                return False
        other = self.kind[a:b] != kind                           # the node is replaced: the defaults, then what the call gives
        self.p[a:b][other] = 0.0
        if kind == DISTORT:
            self.mode[a:b][other] = DEFAULT_MODE
            if mode is not None:
                self.mode[a:b] = m
        else:
            self.mode[a:b] = NONE
        for t, v in enumerate(values):
            if v is not None:
                self.p[a:b, t] = np.broadcast_to(np.asarray(v, F).reshape(-1), (b - a,))
        self.kind[a:b] = kind
        return True

    def set_distort(self, level=None, mode=None, first_channel=0, count=None):
        return self._set(DISTORT, (level,), mode, first_channel, count)

    def set_overdrive(self, boost=None, drive=None, level=None, first_channel=0, count=None):
        return self._set(OVERDRIVE, (boost, drive, level), None, first_channel, count)

    def set_chebyshev(self, level_pos=None, level_neg=None, first_channel=0, count=None):
        return self._set(CHEBYSHEV, (level_pos, level_neg), None, first_channel, count)

    def drop(self, first_channel=0, count=None):
        span = self._span(first_channel, count, ())
        if span is None:
            return False
        a, b = span
        self.kind[a:b] = self.mode[a:b] = NONE
        self.p[a:b] = 0.0
        return True

    def present(self):
        return (self.kind != NONE).astype(np.uint32)

    def has_fuzz(self):
        return bool(((self.kind == DISTORT) & (self.mode == FUZZ)).any())

    def run(self, x, block=128):
        """frames of any number -> the output; a channel's node sees the reference's blocks of `block` frames (the last one may be
        short; the bank refuses that while a channel carries Fuzz, and so does this)"""
        x = np.ascontiguousarray(x, F)
        assert x.shape[1] == self.n
        if self.has_fuzz() and len(x) % block:
            return False
        y = np.empty_like(x)
        for c in range(self.n):
            if self.kind[c] == NONE:
                y.view(np.uint32)[:, c] = x.view(np.uint32)[:, c]                # a copy keeps the sample's very bits
                continue
            nd = node(self.kind[c], self.p[c], self.mode[c])
            for f0 in range(0, len(x), block):
                y[f0:f0 + block, c] = nd.process(x[f0:f0 + block, c])
        return y
