"""A restatement of the channel-FIR bank (include/dspfx.h, dspfx_firs_*): one oracle FIR node per channel (oracle.Node(O.FIR,
mode=.., taps_reversed=..)) with the bank's store rules -- a new node on the first set_taps that names a channel, Node.set_taps (the
reference's reload: the deque is kept) on a channel that carries one, Node.reset for reset, the node discarded by drop; a store
the bank refuses returns False and changes nothing -- and beside every node a pure-numpy VecDeque (oracle/numpy_model.py) stepped
as fir.rs:193-197 steps it, which gives the (len, cap, head) the bank keeps on the device.
tests/test_firs_cpu.py holds it to oracle/numpy_model.Fir bit for bit; tests/test_firs_gpu.py holds the bank to it at 0 ulp.
Blocks are [n_frames][N] frame-major float32; responses are in time order, as the bank takes them."""
import numpy as np

import numpy_model as M
import oracle as O

F = np.float32
NONE = 0xFFFFFFFF
BALANCED, AVERAGE = O.FIR_BALANCED, O.FIR_AVERAGE
MAX_TAPS = 1024
# both sides of every capacity doubling of the VecDeque (4, 8, 16, 32, 64)
TAP_COUNTS = (1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 64)


class ChannelFirs:
    """The bank's methods with the bank's meaning."""

    def __init__(self, n, max_taps=64):
        assert 1 <= max_taps <= MAX_TAPS
        self.n, self.max_taps = int(n), int(max_taps)
        self.nodes = [None] * n
        self.dq = [None] * n                     # numpy_model.VecDeque: the indices only, stepped when they are asked for (_step)
        self.due = [0] * n                       # frames the node has seen since its deque was stepped last
        self.h = [None] * n                      # the response as given
        self.mode = np.full(n, NONE, np.uint32)

    def _span(self, first, count):
        n = self.n - first if count is None else count
        return (first, first + n) if 0 <= first <= self.n and 0 <= n <= self.n - first else None

    def _step(self, c):
        """fir.rs:193-197 on the indices, for the frames channel c has seen under its present T"""
        d, T = self.dq[c], len(self.h[c])
        for _ in range(self.due[c]):
            d.push_back(0.0)
            if d.len > T:
                d.pop_front()
        self.due[c] = 0

    def set_taps(self, h, first_channel=0, count=None, mode=None):
        h = np.asarray(h, np.float64)
        if h.ndim == 1:
            span = self._span(first_channel, count)
        elif h.ndim == 2 and (count is None or count == h.shape[0]):
            span = self._span(first_channel, h.shape[0])
        else:
            return False
        T = h.shape[-1]
        if span is None or not 1 <= T <= self.max_taps or mode not in (None, BALANCED, AVERAGE):
            return False
        for c in range(*span):
            row = h if h.ndim == 1 else h[c - span[0]]
            rev = np.ascontiguousarray(row[::-1])                  # fir.rs:163,168
            if self.nodes[c] is None:                              # a new node: an empty deque
                self.mode[c] = BALANCED if mode is None else mode
                self.nodes[c] = O.Node(O.FIR, mode=int(self.mode[c]), taps_reversed=rev)
                self.dq[c], self.due[c] = M.VecDeque(), 0
            else:                                                  # the reload: taps only
                self._step(c)
                self.nodes[c].set_taps(rev)
                if mode is not None:
                    self._mode(c, mode)
            self.h[c] = row.copy()
        return True

    def _mode(self, c, mode):
        self.mode[c] = mode
        self.nodes[c].L.orc_node_set_mode(self.nodes[c].h, int(mode))

    def set_mode(self, mode, first_channel=0, count=None):
        span = self._span(first_channel, count)
        if span is None or mode not in (BALANCED, AVERAGE):
            return False
        for c in range(*span):
            if self.nodes[c] is not None:
                self._mode(c, mode)
        return True

    def drop(self, first_channel=0, count=None):
        span = self._span(first_channel, count)
        if span is None:
            return False
        for c in range(*span):
            self.nodes[c] = self.dq[c] = self.h[c] = None
            self.mode[c], self.due[c] = NONE, 0
        return True

    def reset(self, first_channel=0, count=None):
        span = self._span(first_channel, count)
        if span is None:
            return False
        for c in range(*span):
            if self.nodes[c] is not None:
                self.nodes[c].reset()
                self.dq[c], self.due[c] = M.VecDeque(), 0
        return True

    def present(self):
        return np.array([nd is not None for nd in self.nodes], np.uint32)

    def lengths(self):
        return np.array([0 if h is None else len(h) for h in self.h], np.uint32)

    def modes(self):
        return self.mode.copy()

    def deque(self):
        """int32 [3][N]: len, cap, head; zeros without a node"""
        out = np.zeros((3, self.n), np.int32)
        for c, d in enumerate(self.dq):
            if d is not None:
                self._step(c)
                out[:, c] = (d.len, d.cap, d.head)
        return out

    def run(self, x):
        """frames of any number -> the output (the FIR node carries no block structure: the oracle takes them 128 at a time)"""
        x = np.ascontiguousarray(x, F)
        assert x.shape[1] == self.n
        y = np.empty_like(x)
        for c in range(self.n):
            if self.nodes[c] is None:
                y.view(np.uint32)[:, c] = x.view(np.uint32)[:, c]                # a copy keeps the sample's very bits
                continue
            y[:, c] = O.chain_run([self.nodes[c]], np.ascontiguousarray(x[:, c]), 0, None, O.BUF_SIZE)
            self.due[c] += len(x)
        return y
