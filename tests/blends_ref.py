"""A restatement of the channel-blend bank (include/dspfx.h, dspfx_blends_*): a node (none, Add, Mix with its ratio), a send and a bus
id per channel with the bank's store rules, and a run that is one reference node per channel, made of the oracle's own numpy
restatements: numpy_model.add, .mix, .gain and .slider_input.  A store or a run that the bank refuses returns False and changes
nothing.  tests/test_blends_cpu.py holds it to oracle.run_channels bit for bit; tests/test_blends_gpu.py holds the bank to it.
Blocks are [n_frames][N] frame-major float32, a bus block [n_frames][buses]."""
import numpy as np

import numpy_model as M

F = np.float32
NONE = 0xFFFFFFFF                # DSPFX_BLENDS_NONE
NO_BUS = 0xFFFFFFFF              # DSPFX_BLENDS_NO_BUS
ADD, MIX = 9, 10                 # dspfx_node_kind
DEFAULT_RATIO = 0.5              # a Mix node fresh from the menu (mix.rs)


class ChannelBlends:
    """The bank's methods with the bank's meaning."""

    def __init__(self, n, buses=0, max_frames=128):
        self.n, self.buses, self.max_frames = int(n), int(buses), int(max_frames)
        self.kind = np.full(n, NONE, np.uint32)
        self.ratio = np.zeros(n, F)              # 0 without a Mix node
        self.level = np.zeros(n, F)              # 0 without a send
        self.send = np.zeros(n, np.uint32)
        self.bus = np.full(n, NO_BUS, np.uint32)

    def _span(self, first, count, values=()):
        n = None
        for v in values:
            if v is not None and np.ndim(v) != 0:
                n = np.size(v)
        if n is None:
            n = self.n - first if count is None else count
        return (first, first + n) if 0 <= first and n >= 0 and first + n <= self.n else None

    def set_mix(self, ratio=None, first_channel=0, count=None):
        span = self._span(first_channel, count, (ratio,))
        if span is None:
            return False
        a, b = span
        if ratio is None:                        # kept on a Mix node, the default over none or an Add node
            self.ratio[a:b] = np.where(self.kind[a:b] == MIX, self.ratio[a:b], F(DEFAULT_RATIO))
        else:
            self.ratio[a:b] = np.broadcast_to(np.asarray(ratio, F).reshape(-1), (b - a,))
        self.kind[a:b] = MIX
        return True

    def set_add(self, first_channel=0, count=None):
        span = self._span(first_channel, count)
        if span is None:
            return False
        a, b = span
        self.kind[a:b] = ADD
        self.ratio[a:b] = 0
        return True

    def set_send(self, level, first_channel=0, count=None):
        span = self._span(first_channel, count, (level,))
        if span is None:
            return False
        a, b = span
        self.send[a:b] = level is not None
        self.level[a:b] = 0 if level is None else np.broadcast_to(np.asarray(level, F).reshape(-1), (b - a,))
        return True

    def assign(self, ids, first_channel=0):
        v = np.atleast_1d(np.asarray(ids, np.int64)).reshape(-1)
        span = self._span(first_channel, len(v))
        if span is None or (((v < 0) | (v >= self.buses)) & (v != NO_BUS)).any():
            return False
        self.bus[span[0]:span[1]] = v
        return True

    def drop(self, first_channel=0, count=None):
        span = self._span(first_channel, count)
        if span is None:
            return False
        a, b = span
        self.kind[a:b] = NONE
        self.ratio[a:b] = 0
        self.level[a:b] = 0
        self.send[a:b] = 0                       # the bus id stays
        return True

    def kinds(self):
        return self.kind.copy()

    def ratios(self):
        return self.ratio.copy()

    def sends(self):
        return self.level.copy(), self.send.copy()

    def bus_of(self):
        return self.bus.copy()

    def second_input(self, n_frames, b=None, bus=None):
        """the N-channel block the nodes' `b` ports see: b itself, bus[f][bus_of[c]] (+0.0 on NO_BUS), or +0.0"""
        if b is not None:
            return np.ascontiguousarray(b, F)
        B = np.zeros((n_frames, self.n), F)
        if bus is not None:
            on = self.bus != NO_BUS
            B[:, on] = np.ascontiguousarray(bus, F)[:, self.bus[on]]
        return B

    def run(self, a, b=None, bus=None, ratio=None):
        """one run of the bank -> [n_frames][N]; ratio: the control block [n_frames][N] or None"""
        a = np.ascontiguousarray(a, F)
        nf = a.shape[0]
        if (b is not None and bus is not None) or (bus is not None and self.buses == 0) or nf == 0 or nf > self.max_frames:
            return False
        B = self.second_input(nf, b, bus)
        out = a.copy()                           # without a node: a's very bits
        with np.errstate(all="ignore"):
            for c in range(self.n):
                if self.kind[c] == NONE:
                    continue
                bb = M.gain(B[:, c], self.level[c]) if self.send[c] else B[:, c]
                if self.kind[c] == ADD:
                    out[:, c] = M.add(a[:, c], bb)
                else:                            # no latch: the stored ratio is not changed
                    r = self.ratio[c] if ratio is None else M.slider_input(np.ascontiguousarray(ratio, F)[:, c], 0.0, 1.0)
                    out[:, c] = M.mix(a[:, c], bb, r)
        return out
