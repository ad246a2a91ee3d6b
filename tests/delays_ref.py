"""numpy float32 restatement of the channel-delay bank (include/dspfx.h, dspfx_delays_*), no product import: per channel an
optional Reverb node (reverb.rs:55-110) with its own seconds and decay sliders and its own ring, and the collect_and_average hop
of LINK_INPUT ahead of it (node.rs:162-194, one connected pipe).  Vectorised over the channels; time is stepped frame by frame.
A store really zeroes the stored channels' rings here: the bank's "these taps still read as zero" count is its way to the same."""
import numpy as np

F = np.float32
LINK_INTERNAL, LINK_INPUT = 1, 2
HOP_DIV = F(F(0.0001) + F(1.0))
PATTERN_LENGTHS = [0, 128, 129, 160, 300, 960]               # channel c of the GPU tests carries pattern c mod 6; 0: no node


def delay_len(seconds, page_round=False):
    """reverb.rs:58: ((seconds * 48000.0) as usize).max(128), `as` truncating and saturating (NaN -> 0); page_round: up to 1024s"""
    with np.errstate(all="ignore"):
        s = F(F(seconds) * F(48000.0))
    if not s > 0:
        d = 0
    elif s >= F(4294967040.0):
        d = 0xFFFFFFFF
    else:
        d = int(s)
    d = max(d, 128)
    if page_round:
        d = (d + 1023) // 1024 * 1024 & 0xFFFFFFFF
    return d


def seconds_for(d):
    """a seconds value whose exact reading is d frames"""
    s = F((d + 0.5) / 48000.0)
    assert delay_len(s) == d, d
    return s


class Delays:
    def __init__(self, channels, max_seconds=0.5, link_flags=0, page_round=False):
        self.n, self.flags, self.page_round = int(channels), int(link_flags), bool(page_round)
        self.cap = delay_len(max_seconds, page_round)
        self.D = np.zeros(self.n, np.int64)                      # 0: no node
        self.pos = np.zeros(self.n, np.int64)
        self.sec = np.full(self.n, 0.5, F)
        self.dec = np.full(self.n, 0.5, F)
        self.ring = np.zeros((self.n, self.cap), F)

    def set_delay(self, seconds=None, decay=None, first_channel=0, count=None):
        """as ChannelDelays.set_delay; returns False (and changes nothing) for a store the bank refuses"""
        first = int(first_channel)
        n = None
        for v in (seconds, decay):
            if v is not None and np.ndim(v) != 0:
                n = int(np.size(v))
        if n is None:
            n = self.n - first if count is None else int(count)
        if first < 0 or n < 0 or first + n > self.n:
            return False
        sl = slice(first, first + n)
        if seconds is None and decay is None:
            self.D[sl] = 0
            self.sec[sl] = self.dec[sl] = F(0.5)
            return True
        sec = self.sec[sl].copy() if seconds is None else np.broadcast_to(np.asarray(seconds, F).reshape(-1), (n,)).copy()
        d = np.asarray([delay_len(s, self.page_round) for s in sec], np.int64)
        if (d > self.cap).any():
            return False
        self.sec[sl] = sec
        if decay is not None:
            self.dec[sl] = np.broadcast_to(np.asarray(decay, F).reshape(-1), (n,))
        self.D[sl] = d                                           # refresh_seconds: a new zero ring, whichever slider moved
        self.pos[sl] = 0
        self.ring[sl] = 0
        return True

    def reset(self):
        self.ring[:] = 0
        self.pos[:] = 0

    def present(self):
        return (self.D != 0).astype(np.uint32)

    def lengths(self):
        return self.D.astype(np.uint32)

    def run(self, x):
        """one run: x is [n_frames][channels] frame-major -> the same shape"""
        v = np.array(x, F, copy=True)
        nf = v.shape[0]
        has = self.D != 0
        with np.errstate(all="ignore"):
            if self.flags & LINK_INPUT:
                v = np.where(has[None, :], ((F(0.0) + v) / HOP_DIV).astype(F), v)
            live = np.flatnonzero(has & (nf <= self.D))          # nf > D: "Reverb buffer is empty", the node copies
            if live.size:
                D, pos, dec = self.D[live], self.pos[live], self.dec[live]
                for i in range(nf):
                    slot = (pos + i) % D
                    tap = self.ring[live, slot]
                    y = (v[i, live] + (tap * dec).astype(F)).astype(F)
                    self.ring[live, slot] = y
                    v[i, live] = y
                self.pos[live] = (pos + nf) % D
        return v

    def run_blocks(self, x, nf=128):
        return np.concatenate([self.run(x[f0:f0 + nf]) for f0 in range(0, len(x), nf)])


def noise(rng, nf, n):
    """finite noise, amplitudes spread over 1e-3 .. 1 per channel"""
    return (rng.uniform(-1.0, 1.0, (nf, n)) * 10.0 ** rng.uniform(-3.0, 0.0, n)[None, :]).astype(F)


def oracle_channel(O, x, length, decay, flags, page_round=False):
    """one channel through the reference's Reverb with a ring of `length` frames, 128-frame blocks; length 0: no node"""
    if not length:
        return np.array(x, F, copy=True)
    return O.chain_run([O.Node(O.REVERB, [float(decay), None], mode=int(page_round), delay_len=int(length))], x, flags)
