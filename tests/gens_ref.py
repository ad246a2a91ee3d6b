"""A restatement of the channel-generator bank (include/dspfx.h, dspfx_gens_*): presence, sliders, mode and clock per channel with
the bank's store rules, and a run that is the oracle's own Signal Generator (numpy_model.NodeModel(K_SIGNAL_GEN)), one instance per
channel, fed one reference block of at most 128 frames at a time.  Control blocks go in as the node's `ctl`; the node's sliders are
put back after every block, so that the oracle's latch does not leak into a later run: the bank's stated divergence (a port is
connected per call).  tests/test_gens_cpu.py holds it to oracle.run_channels bit for bit; tests/test_gens_gpu.py holds the bank to
it at the bars tests/test_gpu_parity.py holds the engine's generator to.  Blocks are [n_frames][N] frame-major float32."""
import numpy as np

import numpy_model as M

F = np.float32
NONE = 0xFFFFFFFF
SINE, TRIANGLE, SQUARE, CONSTANT = range(4)      # dspfx_signal_mode
N_MODES = 4
# a node fresh from the menu (signal_gen.rs:40-52)
DEFAULT_AMPLITUDE, DEFAULT_FREQUENCY, DEFAULT_MODE = 0.5, 100.0, SINE


class ChannelGenerators:
    """The bank's methods with the bank's meaning; a store that the bank refuses returns False and changes nothing."""

    def __init__(self, n):
        self.n = int(n)
        self.node = [None] * self.n              # the channel's NodeModel: it carries the clock
        self.mode = np.full(n, NONE, np.uint32)
        self.p = np.zeros((n, 2), F)             # amplitude, frequency

    def _span(self, first, count, values):
        n = None
        for v in values:
            if v is not None and np.ndim(v) != 0:
                n = np.size(v)
        if n is None:
            n = self.n - first if count is None else count
        return (first, first + n) if 0 <= first and n >= 0 and first + n <= self.n else None

    def set(self, amplitude=None, frequency=None, mode=None, first_channel=0, count=None):
        span = self._span(first_channel, count, (amplitude, frequency, mode))
        if span is None:
            return False
        a, b = span
        if mode is not None:
            m = np.broadcast_to(np.asarray(mode, np.int64).reshape(-1), (b - a,))
            if ((m < 0) | (m >= N_MODES)).any():
                return False
        for c in range(a, b):
            if self.node[c] is None:             # a fresh node: the defaults, clock +0.0
                self.node[c] = M.NodeModel(M.K_SIGNAL_GEN, [DEFAULT_AMPLITUDE, DEFAULT_FREQUENCY], DEFAULT_MODE)
                self.p[c] = (DEFAULT_AMPLITUDE, DEFAULT_FREQUENCY)
                self.mode[c] = DEFAULT_MODE
        for t, v in enumerate((amplitude, frequency)):
            if v is not None:
                self.p[a:b, t] = np.broadcast_to(np.asarray(v, F).reshape(-1), (b - a,))
        if mode is not None:
            self.mode[a:b] = m
        return True

    def drop(self, first_channel=0, count=None):
        span = self._span(first_channel, count, ())
        if span is None:
            return False
        a, b = span
        self.node[a:b] = [None] * (b - a)
        self.mode[a:b] = NONE
        self.p[a:b] = 0.0
        return True

    def reset(self, first_channel=0, count=None):
        span = self._span(first_channel, count, ())
        if span is None:
            return False
        for c in range(*span):
            if self.node[c] is not None:
                self.node[c].impl.clock = F(0.0)
        return True

    def present(self):
        return np.asarray([nd is not None for nd in self.node], np.uint32)

    def modes(self):
        return self.mode.copy()

    def sliders(self):
        return self.p.copy()

    def clocks(self):
        return np.asarray([F(0.0) if nd is None else nd.impl.clock for nd in self.node], F)

    def run(self, n_frames, add_to=None, amplitude=None, frequency=None, block=128):
        """one run of the bank: n_frames frames, cut into the reference's blocks of `block` frames from frame 0 (the last one may be
        short) -> [n_frames][N].  add_to, amplitude, frequency: [n_frames][N] or None"""
        out = np.zeros((n_frames, self.n), F)
        ports = [None if b is None else np.ascontiguousarray(b, F) for b in (amplitude, frequency)]
        if add_to is not None:
            add_to = np.ascontiguousarray(add_to, F)
            out.view(np.uint32)[:] = add_to.view(np.uint32)          # without a node: the block's very bits
        zeros = np.zeros(block, F)
        with np.errstate(all="ignore"):
            for c, nd in enumerate(self.node):
                if nd is None:
                    continue
                nd.mode = int(self.mode[c])
                for f0 in range(0, n_frames, block):
                    f1 = min(n_frames, f0 + block)
                    nd.p[0], nd.p[1] = self.p[c]
                    y = nd.process(zeros[:f1 - f0], None, [None if b is None else b[f0:f1, c] for b in ports])
                    nd.p[0], nd.p[1] = self.p[c]                     # no latch: what the stores left
                    out[f0:f1, c] = y if add_to is None else (add_to[f0:f1, c] + y).astype(F)
        return out
