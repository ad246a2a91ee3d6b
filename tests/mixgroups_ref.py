"""float64 restatement of the mix-group bank (include/dspfx.h, dspfx_mixgroups_*), for the mix-group tests.  Written from the
formula in the header, not from the product code:
      buses[f][g] = (sum over the channels c of group g of fl32(x[f][c] * gain[c])) / link_divisor(n_g)
The terms are formed in numpy float32 (one rounding, as the bank's multiply), summed in float64 and divided by the float64
value of the f32 divisor.  bound() is the standard error bound of ANY summation order whose longest chain of dependent f32
additions is D (each partial sum is rounded at most D times on the way up, Higham, Accuracy and Stability, 4.2), plus one
rounding for the division and the smallest subnormal: it holds no measured constant."""
import numpy as np

U = 2.0 ** -24


def link_divisor(n):
    """node.rs:166,179: f32 0.0001 incremented by 1.0 per connected pipe."""
    d = np.float32(0.0001)
    one = np.float32(1.0)
    for _ in range(int(n)):
        nxt = np.float32(d + one)
        if nxt == d:
            break
        d = nxt
    return d


def terms(x, gain=None):
    """x [F][N] f32, gain [N] f32 or None -> the f32 terms fl32(x * gain) (x itself without a gain)"""
    x = np.asarray(x, np.float32)
    if gain is None:
        return x
    with np.errstate(over="ignore", invalid="ignore"):
        return (x * np.asarray(gain, np.float32)[None, :]).astype(np.float32)


def buses(x, group_start, gain=None, normalise=True, groups=None):
    """-> (ref [F][len(groups)] f64, sabs [F][len(groups)] f64 = sum|t| / div, div [len(groups)] f64) for the listed groups
    (default: all).  An empty group gives 0."""
    t = terms(x, gain).astype(np.float64)
    gs = [int(v) for v in group_start]
    groups = range(len(gs) - 1) if groups is None else groups
    ref = np.zeros((t.shape[0], len(groups)))
    sabs = np.zeros_like(ref)
    div = np.ones(len(groups))
    for i, g in enumerate(groups):
        a, b = gs[g], gs[g + 1]
        if normalise:
            div[i] = float(link_divisor(b - a))
        if b > a:
            ref[:, i] = t[:, a:b].sum(axis=1) / div[i]
            sabs[:, i] = np.abs(t[:, a:b]).sum(axis=1) / div[i]
    return ref, sabs, div


def bound(sabs, ref, depth):
    """(D + 1) 2^-24 sum|t| / div + 2^-24 |ref| + 2^-149; sabs already holds sum|t| / div; depth broadcasts over groups"""
    return (np.asarray(depth, np.float64) + 1.0) * U * sabs + U * np.abs(ref) + 2.0 ** -149


def collect_and_average(pipes):
    """node.rs:162-194 literally: f32, sequential, for `pipes` [n][F] -> [F] f32"""
    pipes = np.asarray(pipes, np.float32)
    out = np.zeros(pipes.shape[1], np.float32)
    num = np.float32(0.0001)
    for p in pipes:
        out = (out + p).astype(np.float32)
        num = np.float32(num + np.float32(1.0))
    return (out / num).astype(np.float32)


def cap(n):
    """the issue's cap on the depth for a group of n channels: 64 + ceil(log2(max(n, 1)))"""
    n = max(int(n), 1)
    return 64 + (n - 1).bit_length()


def ragged_table(n_channels, seed, max_size, min_size=1):
    """A table drawn from a fixed seed: sizes log-uniform in [min_size, max_size] until the channels run out."""
    rng = np.random.default_rng(seed)
    gs = [0]
    while gs[-1] < n_channels:
        size = int(round(float(np.exp(rng.uniform(np.log(min_size), np.log(max_size))))))
        gs.append(min(n_channels, gs[-1] + max(min_size, size)))
    return np.asarray(gs, np.uint64)
