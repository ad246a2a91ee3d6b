"""The channel cancellers' rule (include/dspfx.h, dspfx_cancel_*) restated in numpy float32, written from the rule's text and not
from the kernel: CancelRef, a whole bank, vectorised over the channels.  Beside it LaneModel, a numpy model of ONE lane of the
kernel (cancel_kernels.hip): the ring rows and the row counter, the general body and the fast body with its tap classes, the
sliding window and the weights kept across the blocks of a run.  Every numpy float32 operation is rounded once, which is what the
kernel's __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn do, so all three give the same bits.

For frame n of a channel with T taps, weights w, delay D:
    u[k] = ref[n - D - k], k < T          +0.0 before the node's first frame (its creation or its last reset)
    dot(a, b) = (s0 + s1) + (s2 + s3)     chain j: the k = j (mod 4) in ascending k, s_j = s_j + (a[k] * b[k]), from +0.0
    y = dot(w, u); e = d[n] - y; out[n] = e
    adapt: p = dot(u, u); g = (mu * e) / (p + eps); w[k] = w[k] + (g * u[k]), k < T
    levels: sum d * d and sum e * e over the run, in frame order, from +0.0
"""
import numpy as np

F = np.float32
T_LIST = (1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 64)        # both sides of every multiple of 4 and of the tap classes
CUTS = (37, 128, 91, 128)


def _per_channel(v, n, dtype):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype).reshape(-1), (n,)))


def dot4(a, b, T):
    """a, b: [N, K] float32; T: [N] -> [N] float32.  No term k >= T exists."""
    s = np.zeros((4, a.shape[0]), F)
    with np.errstate(all="ignore"):
        for k in range(int(T.max()) if len(T) else 0):
            live = k < T
            s[k & 3] = np.where(live, s[k & 3] + (a[:, k] * b[:, k]), s[k & 3])
        return (s[0] + s[1]) + (s[2] + s[3])


class CancelRef:
    """A bank of N channels.  Blocks are [frames, N] float32 arrays (the layout is the device's business)."""

    def __init__(self, channels, max_taps=64, max_delay=0):
        if not 1 <= max_taps <= 1024:
            raise ValueError("max_taps")
        self.N, self.K, self.MD = int(channels), int(max_taps), int(max_delay)
        self.T = np.zeros(self.N, np.int64)
        self.D = np.zeros(self.N, np.int64)
        self.mu = np.zeros(self.N, F)
        self.eps = np.zeros(self.N, F)
        self.adapt = np.zeros(self.N, bool)
        self.w = np.zeros((self.N, self.K), F)
        self.H = self.MD + self.K                              # the reference frames a window can reach back to
        self.hist = np.zeros((self.N, self.H), F)              # hist[:, H - 1 - j] = ref[n - 1 - j]
        self.lev = np.zeros((2, self.N), F)

    def _span(self, first, count, arrays=()):
        n = None
        for v in arrays:
            if v is not None and np.ndim(v) != 0:
                if n is not None and np.size(v) != n:
                    raise ValueError("arrays of different lengths")
                n = int(np.size(v))
        if n is None:
            n = self.N - first if count is None else int(count)
        if first < 0 or n < 0 or first + n > self.N:
            raise ValueError("a range past the channels")
        return n

    def set(self, taps=None, mu=None, eps=None, delay=None, adapt=None, first_channel=0, count=None):
        n = self._span(first_channel, count, (taps, mu, eps, delay, adapt))
        sl = slice(first_channel, first_channel + n)
        if taps is not None:
            t = _per_channel(taps, n, np.int64)
            if n and (t.min() < 1 or t.max() > self.K):
                raise ValueError("taps")
        if delay is not None:
            d = _per_channel(delay, n, np.int64)
            if n and (d.min() < 0 or d.max() > self.MD):
                raise ValueError("delay")
        fresh = self.T[sl] == 0
        # a new node: weights +0.0 (they are), history +0.0, mu 0.5, eps 1e-6, delay 0, adapting, max_taps taps
        self.hist[sl][fresh] = 0
        self.T[sl] = t if taps is not None else np.where(fresh, self.K, self.T[sl])
        self.D[sl] = d if delay is not None else np.where(fresh, 0, self.D[sl])
        self.mu[sl] = _per_channel(mu, n, F) if mu is not None else np.where(fresh, F(0.5), self.mu[sl])
        self.eps[sl] = _per_channel(eps, n, F) if eps is not None else np.where(fresh, F(1e-6), self.eps[sl])
        self.adapt[sl] = _per_channel(adapt, n, bool) if adapt is not None else np.where(fresh, True, self.adapt[sl])
        self.w[sl][np.arange(self.K)[None, :] >= self.T[sl][:, None]] = 0       # a smaller T zeroes the rows it leaves

    def load(self, rows, first_channel=0, count=None):
        rows = np.asarray(rows, F)
        n = self._span(first_channel, count) if rows.ndim == 1 else rows.shape[0]
        if rows.ndim == 2 and count is not None and count != n:
            raise ValueError("count")
        self._span(first_channel, n)
        sl = slice(first_channel, first_channel + n)
        if n and not (self.T[sl] == rows.shape[-1]).all():
            raise ValueError("load on a channel without a node or with another T")
        self.w[sl, :rows.shape[-1]] = rows

    def drop(self, first_channel=0, count=None):
        n = self._span(first_channel, count)
        sl = slice(first_channel, first_channel + n)
        self.T[sl] = 0
        self.D[sl] = 0
        self.mu[sl] = 0
        self.eps[sl] = 0
        self.adapt[sl] = False
        self.w[sl] = 0

    def reset(self, first_channel=0, count=None):
        n = self._span(first_channel, count)
        sl = slice(first_channel, first_channel + n)
        self.w[sl] = 0
        self.hist[sl] = 0

    def run(self, mic, ref):
        """mic, ref: [nf, N] -> out [nf, N]; self.w and self.lev afterwards."""
        mic, ref = np.asarray(mic, F), np.asarray(ref, F)
        nf = mic.shape[0]
        buf = np.concatenate([self.hist, ref.T], axis=1)
        out = mic.copy()
        here = self.T > 0
        ks = np.arange(self.K)[None, :]
        live = ks < self.T[:, None]
        sd, se = np.zeros(self.N, F), np.zeros(self.N, F)
        with np.errstate(all="ignore"):
            for f in range(nf):
                u = np.take_along_axis(buf, (self.H + f - self.D)[:, None] - ks, axis=1)
                d = mic[f]
                e = d - dot4(self.w, u, self.T)
                out[f] = np.where(here, e, d)
                sd = sd + (d * d)
                se = se + (e * e)
                p = dot4(u, u, self.T)
                g = (self.mu * e) / (p + self.eps)
                self.w = np.where(live & self.adapt[:, None], self.w + (g[:, None] * u), self.w)
        self.hist = np.ascontiguousarray(buf[:, nf:])
        self.lev = np.stack([np.where(here, sd, F(0)), np.where(here, se, F(0))]).astype(F)
        return out

    def weights(self):
        """[max_taps, N], as the device's table"""
        return np.ascontiguousarray(self.w.T)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- one lane of the kernel ----------------------------------------------------------------------------------------------------
FB = 8              # frames per block of the fast body
RING_PAD = 16
FAST_MAX_T = 64


def _end(s):
    return (s[0] + s[1]) + (s[2] + s[3])


class LaneModel:
    """One channel as cancel_kernels.hip runs it: the ring of max_delay + max_taps + 16 rows (rounded up to 8) with the bank's row counter, the
    weights column, the stores' clearing, and a run as the kernel takes it: the fast body over every whole block of FB frames (T
    <= 64; tap class TP of 8, 16, 32, 64, every term under a select on k < T unless T == TP), then the general body frame by frame."""

    def __init__(self, max_taps=64, max_delay=0, general_only=False):
        self.K, self.MD, self.general_only = int(max_taps), int(max_delay), general_only
        self.R = (self.MD + self.K + RING_PAD + 7) // 8 * 8    # (the rows stand in groups of 8; one lane sees only their order)
        self.ring = np.full(self.R, np.nan, F)                 # never cleared as a whole: a new node clears it
        self.w = np.zeros(self.K, F)
        self.T, self.D, self.mu, self.eps, self.adapt = 0, 0, F(0), F(0), False
        self.row = 0
        self.lev = np.zeros(2, F)

    def set(self, taps=None, mu=None, eps=None, delay=None, adapt=None):
        fresh = self.T == 0
        old = self.T
        self.T = int(taps) if taps is not None else self.K if fresh else self.T
        self.D = int(delay) if delay is not None else 0 if fresh else self.D
        self.mu = F(mu) if mu is not None else F(0.5) if fresh else self.mu
        self.eps = F(eps) if eps is not None else F(1e-6) if fresh else self.eps
        self.adapt = bool(adapt) if adapt is not None else True if fresh else self.adapt
        self.w[self.T:max(old, self.T)] = 0
        if fresh:
            self.ring[:] = 0

    def load(self, row):
        assert len(row) == self.T
        self.w[:self.T] = np.asarray(row, F)

    def drop(self):
        self.T = 0
        self.w[:] = 0

    def reset(self):
        self.w[:] = 0
        self.ring[:] = 0

    def skip(self, nf):
        """a run while the lane carries no node: only the bank's row counter moves"""
        self.row = (self.row + nf) % self.R
        self.lev[:] = 0

    def _frame(self, d, r0):
        T, R = self.T, self.R
        s, p = [F(0)] * 4, [F(0)] * 4
        for k in range(T):
            u = self.ring[(r0 - k) % R]
            s[k & 3] = s[k & 3] + (self.w[k] * u)
            p[k & 3] = p[k & 3] + (u * u)
        e = d - _end(s)
        if self.adapt:
            g = (self.mu * e) / (_end(p) + self.eps)
            for k in range(T):
                self.w[k] = self.w[k] + (g * self.ring[(r0 - k) % R])
        return e

    def _fast(self, mic, ref, out, sums):
        T, R = self.T, self.R
        TP = 8 if T <= 8 else 16 if T <= 16 else 32 if T <= 32 else 64
        full = T == TP
        w = [self.w[k] if (full or k < T) else F(0) for k in range(TP)]
        win = [F(0)] * (TP + FB - 1)
        rd = (self.row - self.D) % R
        for j in range(TP - 1):
            if full or j + T >= TP:
                win[j] = self.ring[(rd - (TP - 1 - j)) % R]
        f = 0
        while f + FB <= len(mic):
            for i in range(FB):
                self.ring[(self.row + i) % R] = ref[f + i]
            for i in range(FB):
                win[TP - 1 + i] = self.ring[(rd + i) % R]
            rd = (rd + FB) % R
            self.row = (self.row + FB) % R
            for i in range(FB):
                s = [F(0)] * 4
                for k in range(TP):
                    sk = s[k & 3] + (w[k] * win[i + TP - 1 - k])
                    s[k & 3] = sk if (full or k < T) else s[k & 3]
                d = mic[f + i]
                e = d - _end(s)
                sums[0] = sums[0] + (d * d)
                sums[1] = sums[1] + (e * e)
                out[f + i] = e
                if self.adapt:
                    p = [F(0)] * 4
                    for k in range(TP):
                        u = win[i + TP - 1 - k]
                        pk = p[k & 3] + (u * u)
                        p[k & 3] = pk if (full or k < T) else p[k & 3]
                    g = (self.mu * e) / (_end(p) + self.eps)
                    for k in range(TP):
                        nw = w[k] + (g * win[i + TP - 1 - k])
                        w[k] = nw if (full or k < T) else w[k]
            for j in range(TP - 1):
                win[j] = win[j + FB]
            f += FB
        if self.adapt:
            for k in range(TP):
                if full or k < T:
                    self.w[k] = w[k]
        return f

    def run(self, mic, ref):
        """mic, ref: [nf] -> out [nf]"""
        if self.T == 0:
            self.skip(len(mic))
            return np.array(mic, F)
        mic, ref = np.asarray(mic, F), np.asarray(ref, F)
        out = np.empty(len(mic), F)
        sums = [F(0), F(0)]
        f = 0
        with np.errstate(all="ignore"):
            if not self.general_only and self.T <= FAST_MAX_T and len(mic) >= FB:
                f = self._fast(mic, ref, out, sums)
            for f in range(f, len(mic)):
                self.ring[self.row] = ref[f]
                d = mic[f]
                e = self._frame(d, (self.row - self.D) % self.R)
                sums[0] = sums[0] + (d * d)
                sums[1] = sums[1] + (e * e)
                out[f] = e
                self.row = (self.row + 1) % self.R
        self.lev = np.array(sums, F)
        return out


def nlms64(mic, ref, T, mu=0.5, eps=1e-6, delay=0):
    """The same recursion in float64 with plain sums (one channel) -> (e, w)."""
    w = np.zeros(T)
    x = np.concatenate([np.zeros(T + delay), np.asarray(ref, np.float64)])
    e = np.zeros(len(mic))
    for n in range(len(mic)):
        u = x[n + T - np.arange(T)]                                    # ref[n - delay - k]
        e[n] = mic[n] - w @ u
        w = w + (mu * e[n] / (u @ u + eps)) * u
    return e, w
