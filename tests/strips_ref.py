"""numpy float32 restatement of the channel-strip bank (include/dspfx.h, dspfx_strips_*), no product import: per channel a chain
of up to 1 + K optional nodes in a fixed order -- a Gain node (gain.rs:25-38), then BiQuad bands 0 .. K-1 (biquad.rs:62-88) --
with the channel's own slider values, and the collect_and_average hops of link_flags (node.rs:162-194, one connected pipe).
Vectorised over the channels; time is stepped frame by frame."""
import numpy as np

F = np.float32
LINK_INTERNAL, LINK_INPUT = 1, 2
GAIN_BIT = 1
HOP_DIV = F(F(0.0001) + F(1.0))


def coeffs(raw6):
    """regenerate_filter (biquad.rs:66-70): raw a0, a1, a2, b0, b1, b2 -> a1, a2, b0, b1, b2, each divided by a0 in f32."""
    r = np.asarray(raw6, F)
    with np.errstate(all="ignore"):
        return (r[..., 1:6] / r[..., 0:1]).astype(F)


class Strips:
    def __init__(self, channels, bands, link_flags=0):
        self.n, self.k, self.flags = int(channels), int(bands), int(link_flags)
        self.mask = np.zeros(self.n, np.uint32)
        self.level = np.ones(self.n, F)
        self.coef = np.zeros((self.k, 5, self.n), F)             # a1, a2, b0, b1, b2
        self.state = np.zeros((self.k, 4, self.n), F)            # x1, x2, y1, y2

    def set_gain(self, levels, first=0, count=None):
        if levels is None:
            n = self.n - first if count is None else count
            self.mask[first:first + n] &= ~np.uint32(GAIN_BIT)
            return
        v = np.asarray(levels, F).reshape(-1) if np.ndim(levels) else np.full(self.n - first if count is None else count, levels, F)
        self.level[first:first + len(v)] = v
        self.mask[first:first + len(v)] |= np.uint32(GAIN_BIT)

    def set_band(self, band, raw6, first=0, count=None):
        bit = np.uint32(1 << (1 + band))
        if raw6 is None:
            n = self.n - first if count is None else count
            self.mask[first:first + n] &= ~bit
            return
        r = np.asarray(raw6, F)
        if r.ndim == 1:
            r = np.tile(r.reshape(1, 6), (self.n - first if count is None else count, 1))
        sl = slice(first, first + len(r))
        self.coef[band, :, sl] = coeffs(r).T
        self.state[band, :, sl] = 0                              # reset_state, biquad.rs:74
        self.mask[sl] |= bit

    def reset(self):
        self.state[:] = 0

    def _hop(self, v, node_bit, seen):
        """the hop in front of a node, on the channels that carry it: LINK_INPUT for a channel's first node, LINK_INTERNAL later"""
        has = (self.mask & np.uint32(node_bit)) != 0
        want = has & np.where(seen, bool(self.flags & LINK_INTERNAL), bool(self.flags & LINK_INPUT))
        with np.errstate(all="ignore"):
            h = ((F(0.0) + v) / HOP_DIV).astype(F)
        return np.where(want[None, :], h, v), has

    def run(self, x):
        """x: [n_frames][channels] frame-major -> the same shape"""
        v = np.array(x, F, copy=True)
        seen = np.zeros(self.n, bool)
        with np.errstate(all="ignore"):
            v, has = self._hop(v, GAIN_BIT, seen)
            v = np.where(has[None, :], (v * self.level[None, :]).astype(F), v)
            seen |= has
            for b in range(self.k):
                v, has = self._hop(v, 1 << (1 + b), seen)
                seen |= has
                if not has.any():
                    continue
                a1, a2, b0, b1, b2 = self.coef[b]
                x1, x2, y1, y2 = (self.state[b, r].copy() for r in range(4))
                for f in range(v.shape[0]):
                    xi = v[f]
                    y = F(b0 * xi) + F(b1 * x1)
                    y = (y + F(b2 * x2)).astype(F)
                    y = (y - F(a1 * y1)).astype(F)
                    y = (y - F(a2 * y2)).astype(F)
                    x2, x1 = np.where(has, x1, x2), np.where(has, xi, x1)
                    y2, y1 = np.where(has, y1, y2), np.where(has, y, y1)
                    v[f] = np.where(has, y, xi)
                self.state[b] = np.stack([x1, x2, y1, y2])
        return v


# ---- the presence patterns and data the CPU and the GPU tests share -----------------------------------------------------
def patterns(bands):
    """node masks: none; Gain only; band 1 only; Gain + bands {0, 2}; all -- those that fit in `bands` bands"""
    full = (1 << (1 + bands)) - 1
    p = [0, GAIN_BIT, 1 << 2, GAIN_BIT | (1 << 1) | (1 << 3), full]
    return [m for m in p if m <= full]


def stable_raw6(rng, n):
    """n random stable BiQuads as raw sliders: poles inside radius 0.95, any zeros, a0 away from 0 (both signs)"""
    r, th = rng.uniform(0.0, 0.95, n), rng.uniform(0.0, np.pi, n)
    a0 = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    a = np.stack([np.ones(n), -2.0 * r * np.cos(th), r * r], 1)
    b = rng.uniform(-1.0, 1.0, (n, 3))
    return (np.concatenate([a, b], 1) * a0[:, None]).astype(F)


def noise(rng, nf, n):
    """finite noise, amplitudes spread over 1e-3 .. 1 per channel"""
    return (rng.uniform(-1.0, 1.0, (nf, n)) * 10.0 ** rng.uniform(-3.0, 0.0, n)[None, :]).astype(F)


def oracle_nodes(O, mask, level, raw6_by_band):
    """the reference nodes of one channel: exactly its present nodes, with its slider values"""
    nodes = []
    if mask & GAIN_BIT:
        nodes.append(O.Node(O.GAIN, [float(level)]))
    for b, raw in enumerate(raw6_by_band):
        if mask & (1 << (1 + b)):
            nodes.append(O.Node(O.BIQUAD, [float(q) for q in raw]))
    return nodes
