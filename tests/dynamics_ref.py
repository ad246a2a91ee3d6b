"""An independent numpy restatement of the channel-dynamics bank (include/dspfx.h, dspfx_dynamics_*): the f32 envelope recurrence,
the gain computer with its one division, the block's level and reduction, presence, and the stores.  tests/test_dynamics_cpu.py
holds its envelope to the oracle's Envelope node and its quiet channels to the oracle's Gain node bit for bit;
tests/test_dynamics_gpu.py holds the bank to it bit for bit.  Blocks are [n_frames][N] frame-major float32."""
import numpy as np

from talkers_ref import envelope_gain

F = np.float32


def gain(env, thr, mk):
    """-> (mk * q, q), q = env > thr ? thr / env : 1, elementwise in f32"""
    env, thr, mk = np.asarray(env, F), np.asarray(thr, F), np.asarray(mk, F)
    with np.errstate(all="ignore"):
        q = np.where(env > thr, thr / env, F(1.0)).astype(F)
        return (mk * q).astype(F), q


class ChannelDynamics:
    """The bank's methods with the bank's meaning; a store that the bank refuses returns False and changes nothing."""

    def __init__(self, n):
        self.n = int(n)
        self.env, self.level, self.reduction = np.zeros(n, F), np.zeros(n, F), np.ones(n, F)
        self.ga, self.gr = np.zeros(n, F), np.zeros(n, F)
        self.thr, self.mk = np.ones(n, F), np.ones(n, F)
        self.on = np.zeros(n, bool)

    def _span(self, first, count, values):
        n = None
        for v in values:
            if v is not None and np.ndim(v) != 0:
                n = np.size(v)
        if n is None:
            n = self.n - first if count is None else count
        return (first, first + n) if 0 <= first and n >= 0 and first + n <= self.n else None

    def set(self, threshold=None, makeup=None, attack=None, release=None, first_channel=0, count=None):
        span = self._span(first_channel, count, (threshold, makeup, attack, release))
        if span is None:
            return False
        a, b = span
        with np.errstate(invalid="ignore"):
            if threshold is not None:
                t = np.asarray(threshold, F)
                if (~(t >= 0) | np.signbit(t)).any():
                    return False
            if makeup is not None:
                m = np.asarray(makeup, F)
                if (~(m >= 0) | np.signbit(m) | np.isinf(m)).any():
                    return False
        for v, tab in ((attack, self.ga), (release, self.gr)):
            if v is not None:
                tab[a:b] = [envelope_gain(f) for f in np.broadcast_to(np.asarray(v, F).reshape(-1), (b - a,))]
        if threshold is not None:
            self.thr[a:b] = threshold
        if makeup is not None:
            self.mk[a:b] = makeup
        self.on[a:b] = True
        return True

    def drop(self, first_channel=0, count=None):
        span = self._span(first_channel, count, ())
        if span is None:
            return False
        a, b = span
        self.on[a:b] = False
        self.ga[a:b] = self.gr[a:b] = 0.0
        self.thr[a:b] = self.mk[a:b] = 1.0
        self.env[a:b] = self.level[a:b] = 0.0
        self.reduction[a:b] = 1.0
        return True

    def reset(self, first_channel=0, count=None):
        span = self._span(first_channel, count, ())
        if span is None:
            return False
        a, b = span
        self.env[a:b] = self.level[a:b] = 0.0
        self.reduction[a:b] = 1.0
        return True

    def present(self):
        return self.on.astype(np.uint32)

    def run(self, x, key=None):
        """one block -> the output block.  self.envs is every frame's envelope, [n_frames][N] (a channel without a node: its
        envelope at rest)"""
        x = np.asarray(x, F)
        k = x if key is None else np.asarray(key, F)
        assert k.shape == x.shape
        env, lvl, red = self.env.copy(), np.zeros(self.n, F), np.ones(self.n, F)
        y = np.empty_like(x)
        self.envs = np.empty_like(x)
        on = self.on
        with np.errstate(all="ignore"):
            for f in range(x.shape[0]):
                kf = k[f]
                d = np.where(kf < 0, -kf, kf)
                g = np.where(env < d, self.ga, self.gr)
                e = d + (env + (-d)) * g
                env = np.where(on, e, env)
                q = np.where(env > self.thr, self.thr / env, F(1.0))
                y[f] = np.where(on, x[f] * (self.mk * q), x[f])
                self.envs[f] = env
                lvl = np.where(on & (env > lvl), env, lvl)
                red = np.where(on & (q < red), q, red)
        assert env.dtype == F and y.dtype == F and lvl.dtype == F and red.dtype == F
        # a copy keeps the sample's very bits, a signalling NaN's too
        y.view(np.uint32)[:, ~on] = x.view(np.uint32)[:, ~on]
        self.env, self.level, self.reduction = env, lvl, red
        return y

    def run_blocks(self, x, nf=128, key=None):
        return np.concatenate([self.run(x[f0:f0 + nf], None if key is None else key[f0:f0 + nf]) for f0 in range(0, len(x), nf)])
