"""A restatement of the channel-rack bank (include/dspfx.h, dspfx_racks_*): the kinds, modes and raw sliders per slot and channel
with the bank's store rules, and a run that is the oracle's own nodes, one chain per channel -- its present nodes in slot order,
link_flags 0 -- with the state carried in the oracle's nodes from run to run.  A store of the kind a slot carries keeps what is
None; for LowPass, HighPass and Envelope it goes through the oracle's set_param, the reference's slider change (no
after_settings_change: the state stays); for BiQuad it makes a new oracle node (biquad.rs:62-76: the state is zeroed), from the
coefficients strips_ref.coeffs gives with a0 = 1; the stateless kinds get a new node, which is the same thing.  A store of another
kind, a drop and a reset make new nodes.  A node is anything with .kind, .params and .mode: the product's NodeSpec.
tests/test_racks_cpu.py holds it to oracle.run_channels bit for bit; tests/test_racks_gpu.py holds the bank to it at the bars
tests/test_gpu_parity.py holds the engine to.  Blocks are [n_frames][N] frame-major float32."""
import numpy as np

import oracle as O
import strips_ref

F = np.float32
NONE = 0xFFFFFFFF
GAIN, BIQUAD, LOW_PASS, HIGH_PASS, REVERB, DISTORT, OVERDRIVE, CHEBYSHEV, FIR, ADD, MIX, SIGNAL_GEN, ENVELOPE = range(13)      # dspfx_kind
FUZZ, LAST_MODE = 4, 8                           # dspfx_distort_mode
SLIDERS = {GAIN: 1, BIQUAD: 6, LOW_PASS: 1, HIGH_PASS: 1, ENVELOPE: 2, DISTORT: 1, OVERDRIVE: 3, CHEBYSHEV: 2}
# a node fresh from the menu (dspfx_node_defaults)
DEFAULTS = {GAIN: (1.0,), BIQUAD: (1.0, -0.24, 0.0, 0.758, 0.0, 0.0), LOW_PASS: (0.5,), HIGH_PASS: (0.5,), ENVELOPE: (0.0, 0.0),
            DISTORT: (0.0,), OVERDRIVE: (0.0, 0.0, 0.0), CHEBYSHEV: (0.0, 0.0)}
DEFAULT_MODE = 1                                 # SoftClip
KEEPS_STATE = (LOW_PASS, HIGH_PASS, ENVELOPE)
MAX_SLOTS = 4
BYTES_PER_SLOT = 37                              # five slider fields, four state floats, the kind byte


def node(kind, sliders, mode):
    """the oracle node of one slot, state at rest"""
    kind = int(kind)
    p = [float(v) for v in sliders[:SLIDERS[kind]]]
    if kind == BIQUAD:
        with np.errstate(all="ignore"):
            p = [1.0] + [float(v) for v in strips_ref.coeffs(np.asarray(sliders[:6], F))]
    return O.Node(kind, p, int(mode) if kind == DISTORT else None)


class ChannelRacks:
    """The bank's methods with the bank's meaning; a store that the bank refuses returns False and changes nothing."""

    def __init__(self, n, slots=4, nodes=True):
        """nodes=False: the tables and the store rules alone, no oracle node behind a slot and no run"""
        assert 1 <= slots <= MAX_SLOTS
        self.n, self.slots, self.with_nodes = int(n), int(slots), bool(nodes)
        self.kind = np.full((slots, n), NONE, np.uint32)
        self.mode = np.full((slots, n), NONE, np.uint32)
        self.p = np.zeros((slots, n, 6), F)
        self.nodes = [[None] * n for _ in range(slots)]

    def _span(self, slot, first, count, values):
        if slot is not None and not 0 <= slot < self.slots:
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

    def set(self, slot, spec, first_channel=0, count=None):
        kind = int(spec.kind)
        values = list(spec.params)
        if kind not in SLIDERS or len(values) > SLIDERS[kind]:
            return False
        modes = spec.mode if kind == DISTORT else None
        span = self._span(slot, first_channel, count, values + [modes])
        if span is None:
            return False
        a, b = span
        vals = [None if v is None else np.broadcast_to(np.asarray(v, F).reshape(-1), (b - a,)) for v in values]
        if modes is not None:
            modes = np.broadcast_to(np.asarray(modes).reshape(-1), (b - a,))
            if ((modes < 0) | (modes > LAST_MODE) | (modes == FUZZ)).any():
                return False
        for c in range(a, b):
            same = self.kind[slot, c] == kind
            if not same:                                          # a new node: the defaults, state +0.0
                self.p[slot, c] = 0.0
                self.p[slot, c, :SLIDERS[kind]] = DEFAULTS[kind]
                self.kind[slot, c] = kind
                self.mode[slot, c] = DEFAULT_MODE if kind == DISTORT else NONE
            for t, v in enumerate(vals):
                if v is not None:
                    self.p[slot, c, t] = v[c - a]
            if modes is not None:
                self.mode[slot, c] = modes[c - a]
            if not self.with_nodes:
                continue
            if same and kind in KEEPS_STATE:                      # the reference's slider change: the state stays
                for t, v in enumerate(vals):
                    if v is not None:
                        self.nodes[slot][c].set_param(t, float(v[c - a]))
            else:
                self.nodes[slot][c] = node(kind, self.p[slot, c], self.mode[slot, c])
        return True

    def set_chain(self, specs, first_channel=0, count=None):
        specs = list(specs)
        if len(specs) > self.slots:
            return False
        ok = True
        for t, s in enumerate(specs):
            ok = self.set(t, s, first_channel, count) and ok
        for t in range(len(specs), self.slots):
            ok = self.drop(t, first_channel, count) and ok
        return ok

    def drop(self, slot, first_channel=0, count=None):
        span = self._span(slot, first_channel, count, ())
        if span is None:
            return False
        a, b = span
        self.kind[slot, a:b] = NONE
        self.mode[slot, a:b] = NONE
        self.p[slot, a:b] = 0.0
        self.nodes[slot][a:b] = [None] * (b - a)
        return True

    def reset(self, first_channel=0, count=None, slot=None):
        span = self._span(slot, first_channel, count, ())
        if span is None:
            return False
        for s in range(self.slots) if slot is None else (slot,):
            for c in range(*span):
                if self.kind[s, c] != NONE and self.with_nodes:
                    self.nodes[s][c] = node(self.kind[s, c], self.p[s, c], self.mode[s, c])
        return True

    def present(self):
        return ((self.kind != NONE).astype(np.uint32) << np.arange(self.slots, dtype=np.uint32)[:, None]).sum(axis=0).astype(np.uint32)

    def descs(self, c):
        """channel c's present nodes in slot order as oracle descs (fresh state): what oracle.run_channels takes"""
        out = []
        for s in range(self.slots):
            k = int(self.kind[s, c])
            if k != NONE:
                out.append({"kind": k, "params": [float(v) for v in self.p[s, c, :SLIDERS[k]]], "mode": int(self.mode[s, c]) if k == DISTORT else None})
        return out

    def run(self, x, block=128):
        """frames of any number -> the output; a channel's chain sees the reference's blocks of `block` frames (the last one may
        be short: none of the kinds carries a block structure)"""
        x = np.ascontiguousarray(x, F)
        assert x.shape[1] == self.n and self.with_nodes
        y = np.empty_like(x)
        for c in range(self.n):
            chain = [self.nodes[s][c] for s in range(self.slots) if self.kind[s, c] != NONE]
            if not chain:
                y.view(np.uint32)[:, c] = x.view(np.uint32)[:, c]                # a copy keeps the sample's very bits
            else:
                y[:, c] = O.chain_run(chain, np.ascontiguousarray(x[:, c]), 0, None, block)
        return y
