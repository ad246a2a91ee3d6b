"""A restatement of the channel-filter bank (include/dspfx.h, dspfx_filters_*): the kinds and sliders per channel and stage with the
bank's store rules, and a run that is the oracle's own LowPass / HighPass / Envelope node, one chain per channel -- its present
nodes in slot order, link_flags 0 -- with the state carried in the oracle's nodes from run to run.  A store of the kind a slot
carries changes its slider through the oracle's set_param, the reference's slider change (none of the three nodes has an
after_settings_change: the state stays); a store of another kind, a drop and a reset make a new oracle node.
tests/test_filters_cpu.py holds it to oracle.run_channels bit for bit; tests/test_filters_gpu.py holds the bank to it at the bars
tests/test_gpu_parity.py holds the engine to.  Blocks are [n_frames][N] frame-major float32."""
import numpy as np

import oracle as O

F = np.float32
NONE = 0xFFFFFFFF
LOW_PASS, HIGH_PASS, ENVELOPE = 2, 3, 12         # dspfx_kind
SLIDERS = {LOW_PASS: 1, HIGH_PASS: 1, ENVELOPE: 2}
# a node fresh from the menu (low_pass.rs, high_pass.rs: ratio 0.5; envelope.rs:27-30: attack 0, release 0)
DEFAULTS = {LOW_PASS: (0.5, 0.0), HIGH_PASS: (0.5, 0.0), ENVELOPE: (0.0, 0.0)}
MAX_STAGES = 4


def node(kind, sliders):
    """the oracle node of one slot, state at rest"""
    return O.Node(int(kind), [float(v) for v in sliders[:SLIDERS[int(kind)]]])


class ChannelFilters:
    """The bank's methods with the bank's meaning; a store that the bank refuses returns False and changes nothing."""

    def __init__(self, n, stages=1):
        assert 1 <= stages <= MAX_STAGES
        self.n, self.stages = int(n), int(stages)
        self.kind = np.full((stages, n), NONE, np.uint32)
        self.p = np.zeros((stages, n, 2), F)
        self.nodes = [[None] * n for _ in range(stages)]

    def _span(self, stage, first, count, values):
        if stage is not None and not 0 <= stage < self.stages:
            return None
        n = None
        for v in values:
            if v is not None and np.ndim(v) != 0:
                if n is not None and np.size(v) != n:
                    return None
                n = np.size(v)
        if n is None:
            n = self.n - first if count is None else count
        return (first, first + n) if 0 <= first and n >= 0 and first + n <= self.n else None

    def _set(self, kind, stage, values, first, count):
        span = self._span(stage, first, count, values)
        if span is None:
            return False
        a, b = span
        vals = [None if v is None else np.broadcast_to(np.asarray(v, F).reshape(-1), (b - a,)) for v in values]
        for c in range(a, b):
            same = self.kind[stage, c] == kind
            if not same:                                          # a new node: the defaults, state +0.0
                self.p[stage, c] = DEFAULTS[kind]
                self.kind[stage, c] = kind
            for t, v in enumerate(vals):
                if v is not None:
                    self.p[stage, c, t] = v[c - a]
            if same:                                              # the reference's slider change: the state stays
                for t, v in enumerate(vals):
                    if v is not None:
                        self.nodes[stage][c].set_param(t, float(v[c - a]))
            else:
                self.nodes[stage][c] = node(kind, self.p[stage, c])
        return True

    def set_low_pass(self, stage, ratio=None, first_channel=0, count=None):
        return self._set(LOW_PASS, stage, (ratio,), first_channel, count)

    def set_high_pass(self, stage, ratio=None, first_channel=0, count=None):
        return self._set(HIGH_PASS, stage, (ratio,), first_channel, count)

    def set_envelope(self, stage, attack=None, release=None, first_channel=0, count=None):
        return self._set(ENVELOPE, stage, (attack, release), first_channel, count)

    def drop(self, stage, first_channel=0, count=None):
        span = self._span(stage, first_channel, count, ())
        if span is None:
            return False
        a, b = span
        self.kind[stage, a:b] = NONE
        self.p[stage, a:b] = 0.0
        self.nodes[stage][a:b] = [None] * (b - a)
        return True

    def reset(self, first_channel=0, count=None, stage=None):
        span = self._span(stage, first_channel, count, ())
        if span is None:
            return False
        for s in range(self.stages) if stage is None else (stage,):
            for c in range(*span):
                if self.kind[s, c] != NONE:
                    self.nodes[s][c] = node(self.kind[s, c], self.p[s, c])
        return True

    def present(self):
        return (self.kind != NONE).any(axis=0).astype(np.uint32)

    def run(self, x, block=128):
        """frames of any number -> the output; a channel's chain sees the reference's blocks of `block` frames (the last one may
        be short: the recurrences carry no block structure)"""
        x = np.ascontiguousarray(x, F)
        assert x.shape[1] == self.n
        y = np.empty_like(x)
        for c in range(self.n):
            chain = [self.nodes[s][c] for s in range(self.stages) if self.kind[s, c] != NONE]
            if not chain:
                y.view(np.uint32)[:, c] = x.view(np.uint32)[:, c]                # a copy keeps the sample's very bits
            else:
                y[:, c] = O.chain_run(chain, np.ascontiguousarray(x[:, c]), 0, None, block)
        return y
