"""float64 restatement of the mix-group bank's per-channel returns (include/dspfx.h, dspfx_mixgroups_returns), for the returns
tests.  Written from the formula in the header, not from the product code: for channel c of group g with n_g channels and
terms t[f][c] = fl32(x[f][c] * gain[c]) (mixgroups_ref.terms),
      returns[f][c] = fl32( fl32(S[f][g] - t[f][c]) / link_divisor(n_g - 1) )      n_g >= 2
      returns[f][c] = +0.0                                                         n_g == 1
returns_exact is what that approximates: the float64 sum of the OTHER channels' f32 terms over the float64 value of the f32
divisor.  returns_bits is the definition itself in numpy float32 from given raw sums S.  The bound of every accuracy check is
mixgroups_ref.bound(sabs, ref, D + 1): the bus bound of a sum of depth D with one more rounding, for the subtraction, where
sabs is taken over the WHOLE group's terms (the own term cancels; its rounding errors do not)."""
import numpy as np

from mixgroups_ref import bound, collect_and_average, link_divisor, terms  # noqa: F401  (re-exported for the tests)


def group_of(table, n):
    """-> int64[n]: the group of every channel"""
    gs = np.asarray([int(v) for v in table], np.int64)
    return np.searchsorted(gs, np.arange(n), side="right") - 1


def returns_divisors(table, normalise=True):
    """-> f32[G]: link_divisor(n_g - 1) per group (1.0 without normalise and for groups of fewer than two channels)"""
    sizes = np.diff(np.asarray([int(v) for v in table], np.int64))
    cache = {}
    div = np.ones(len(sizes), np.float32)
    for g, n in enumerate(sizes):
        if normalise and n >= 2:
            if n not in cache:
                cache[n] = link_divisor(n - 1)
            div[g] = cache[n]
    return div


def returns_exact(x, table, gain=None, normalise=True):
    """-> (ref [F][N] f64, sabs [F][N] f64): ref = (float64 sum of the other channels' f32 terms) / divisor(n_g - 1), sabs =
    (sum of |t| over the whole group) / divisor(n_g - 1); a group of one gives 0 in both."""
    t = terms(x, gain).astype(np.float64)
    gs = [int(v) for v in table]
    div = returns_divisors(table, normalise).astype(np.float64)
    ref = np.zeros_like(t)
    sabs = np.zeros_like(t)
    for g, (a, b) in enumerate(zip(gs[:-1], gs[1:])):
        if b - a < 2:
            continue
        # the sum of the others, without cancellation: prefix sums from the left plus from the right
        left = np.concatenate([np.zeros((t.shape[0], 1)), np.cumsum(t[:, a:b - 1], axis=1)], axis=1)
        right = np.concatenate([np.cumsum(t[:, b - 1:a:-1], axis=1)[:, ::-1], np.zeros((t.shape[0], 1))], axis=1)
        ref[:, a:b] = (left + right) / div[g]
        sabs[:, a:b] = (np.abs(t[:, a:b]).sum(axis=1) / div[g])[:, None]
    return ref, sabs


def returns_bits(S_raw, x, table, gain=None, normalise=True):
    """The definition in numpy float32 from given raw sums S_raw [F][G]: ((S_raw[:, g(c)] - t).astype(f32) / div).astype(f32),
    and +0.0 for groups of one.  Without normalise the division is left out."""
    t = terms(x, gain)
    S = np.asarray(S_raw, np.float32)
    g = group_of(table, t.shape[1])
    sizes = np.diff(np.asarray([int(v) for v in table], np.int64))
    with np.errstate(over="ignore", invalid="ignore"):
        d = (S[:, g] - t).astype(np.float32)
        if normalise:
            d = (d / returns_divisors(table, True)[g][None, :]).astype(np.float32)
    d[:, sizes[g] == 1] = np.float32(0.0)
    return d
