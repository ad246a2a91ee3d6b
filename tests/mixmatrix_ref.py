"""float64 restatement of the mix-matrix bank (include/dspfx.h, dspfx_mixmatrix_*), for the mix-matrix tests.  Written from the
formula in the header, not from the product code: room r of n_r contiguous channels owns M_r[l][s] (listener, source) and
      out[f][c0 + l] = (sum over s in [0, n_r) of M_r[l][s] * x[f][c0 + s]) / d[c0 + l]
d = link_divisor(w), w = the entries of the listener's row that are not +-0.0; a row without one gives +0.0; normalise = False
leaves the division out.  exact() evaluates that in float64 from the f32 inputs (the products of two f32 are exact in f64).
bound() is the error bound of ANY order of n rounded products and n - 1 rounded additions plus one division -- and all the more
of an fma chain, which rounds once per term:
      |got - exact| <= (n + 2) 2^-24 (sum_s |M[l][s] x[s]|) / d + 2^-149
(Higham, Accuracy and Stability, 3.1: gamma_n for the dot product, one more rounding for the division, one in hand for the
second-order terms; the smallest subnormal covers a result that underflows).  It is derived, not measured."""
import numpy as np

from mixgroups_ref import link_divisor

U = 2.0 ** -24


def rooms(table):
    """-> [(c0, n)] per room"""
    gs = [int(v) for v in table]
    return [(a, b - a) for a, b in zip(gs[:-1], gs[1:])]


def mix_minus(table):
    """the fresh bank: 1.0 off the diagonal, +0.0 on it"""
    return [(1.0 - np.eye(n)).astype(np.float32) for _, n in rooms(table)]


def divisors(mats, normalise=True):
    """-> (d f64[N], wired bool[N]): the f64 value of the f32 link divisor of every listener's wired count (1.0 without
    normalise or without a wired entry), and whether the listener has a wired entry at all"""
    cache = {}
    d, wired = [], []
    for m in mats:
        w = (np.asarray(m, np.float32) != 0).sum(axis=1)
        for k in w:
            k = int(k)
            if k not in cache:
                cache[k] = float(link_divisor(k)) if k else 1.0
            d.append(cache[k] if normalise else 1.0)
            wired.append(k > 0)
    return np.asarray(d, np.float64), np.asarray(wired, bool)


def exact(x, table, mats, normalise=True):
    """x [F][N] f32 -> (ref [F][N] f64, sabs [F][N] f64 = sum_s |M x| / d, n_of f64[N] = the room size of every channel)"""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    ref = np.zeros_like(x64)
    sabs = np.zeros_like(x64)
    n_of = np.zeros(x64.shape[1])
    d, wired = divisors(mats, normalise)
    for (c0, n), m in zip(rooms(table), mats):
        m64 = np.asarray(m, np.float32).astype(np.float64)
        assert m64.shape == (n, n)
        ref[:, c0:c0 + n] = x64[:, c0:c0 + n] @ m64.T
        sabs[:, c0:c0 + n] = np.abs(x64[:, c0:c0 + n]) @ np.abs(m64).T
        n_of[c0:c0 + n] = n
    ref /= d[None, :]
    sabs /= d[None, :]
    ref[:, ~wired] = 0.0
    sabs[:, ~wired] = 0.0
    return ref, sabs, n_of


def bound(sabs, n_of):
    """(n + 2) 2^-24 sabs + 2^-149, in float64; sabs already holds sum|M x| / d"""
    return (np.asarray(n_of, np.float64)[None, :] + 2.0) * U * sabs + 2.0 ** -149


def eval_f32(x, table, mats, normalise=True, order="ascending"):
    """The definition in numpy float32, rounded products and rounded additions, in one of two orders: "ascending" adds the sources
    one after the other from s = 0, "pairwise" adds neighbours in a tree.  -> [F][N] f32"""
    x = np.asarray(x, np.float32)
    out = np.zeros_like(x)
    d, wired = divisors(mats, normalise)
    for (c0, n), m in zip(rooms(table), mats):
        m = np.asarray(m, np.float32)
        prod = (x[:, None, c0:c0 + n] * m[None, :, :]).astype(np.float32)        # [F][l][s]
        if order == "ascending":
            acc = np.zeros(prod.shape[:2], np.float32)
            for s in range(n):
                acc = (acc + prod[:, :, s]).astype(np.float32)
        else:
            t = prod
            while t.shape[2] > 1:
                if t.shape[2] % 2:
                    t = np.concatenate([t, np.zeros(t.shape[:2] + (1,), np.float32)], axis=2)
                t = (t[:, :, 0::2] + t[:, :, 1::2]).astype(np.float32)
            acc = t[:, :, 0]
        out[:, c0:c0 + n] = acc
    out = (out / d.astype(np.float32)[None, :]).astype(np.float32) if normalise else out
    out[:, ~wired] = np.float32(0.0)
    return out


def asymmetric(n):
    """the integer matrix of the exactness test: M[l][s] = ((3 l + 5 s) % 7) - 3, entries in [-3, 3], M != M^T"""
    l, s = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return (((3 * l + 5 * s) % 7) - 3).astype(np.float32)


def random_mats(table, seed, zero_fraction=1.0 / 3.0):
    """uniform [0, 10) entries with about `zero_fraction` of them set to +0.0"""
    rng = np.random.default_rng(seed)
    out = []
    for _, n in rooms(table):
        m = rng.uniform(0.0, 10.0, (n, n)).astype(np.float32)
        m[rng.uniform(0.0, 1.0, (n, n)) < zero_fraction] = np.float32(0.0)
        out.append(m)
    return out
