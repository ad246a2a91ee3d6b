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


CLASSES = ("finite", "nan", "+inf", "-inf")


def classify(x, table, mats, normalise=True):
    """-> [F][N] array of "nan", "+inf", "-inf" or "finite": what the output of frame f and listener l must be, from the terms
    x[f][s] * M[l][s] formed in numpy float32 alone.  "nan": some term is NaN (0 * inf is one), or infinite terms of both signs are
    present; a signed infinity: infinite terms of that sign only; "finite" otherwise -- and for a row without a wired entry, whose
    output is +0.0 whatever the samples are (the documented rule).  A division by the link divisor (finite, >= 1) changes no class,
    so `normalise` changes nothing here; it is taken so that the call reads like exact() and eval_f32().
    This classification is independent of the summation order and of fusing only while no FINITE product or partial sum can
    overflow: an order that overflows to +inf on the way and meets -inf later gives NaN where another order gives -inf.  So the
    inputs must satisfy  max|x finite| * max|M finite| * n < 2^120  (asserted), which keeps every finite partial sum eight binades
    under the f32 maximum; 3.4e38 therefore has no place in a mix-matrix edge block."""
    x = np.asarray(x, np.float32)
    out = np.full(x.shape, "finite", dtype="<U6")
    _, wired = divisors(mats, normalise)
    for (c0, n), m in zip(rooms(table), mats):
        m = np.asarray(m, np.float32)
        xs = x[:, c0:c0 + n]
        big_x = np.abs(xs[np.isfinite(xs)]).max(initial=0.0)
        big_m = np.abs(m[np.isfinite(m)]).max(initial=0.0)
        assert float(big_x) * float(big_m) * n < 2.0 ** 120, (c0, n, big_x, big_m)
        with np.errstate(all="ignore"):
            prod = (xs[:, None, :] * m[None, :, :]).astype(np.float32)            # [F][l][s]
        nan = np.isnan(prod).any(axis=2)
        pos, neg = np.isposinf(prod).any(axis=2), np.isneginf(prod).any(axis=2)
        room = np.full(nan.shape, "finite", dtype="<U6")
        room[pos & ~neg] = "+inf"
        room[neg & ~pos] = "-inf"
        room[nan | (pos & neg)] = "nan"
        out[:, c0:c0 + n] = room
    out[:, ~wired] = "finite"
    return out


def scaled_int_product(k, table, mats, e):
    """Integer samples k [F][N] standing for x = k * 2^e, integer-valued matrices: -> the f32 of (int64 product) * 2^e.  Asserted:
    sum_s |M[l][s] k[f][s]| < 2^24 for every output, so every partial sum of every order is an integer below 2^24 times 2^e --
    exactly representable in f32 down to e = -149, where inputs and outputs are subnormal or barely normal -- and the result is
    the only value a correct kernel of any summation order can give."""
    ki = np.asarray(k).astype(np.int64)
    assert (ki == np.asarray(k)).all() and e >= -149
    out = np.zeros(ki.shape, np.int64)
    for (c0, n), m in zip(rooms(table), mats):
        mi = np.asarray(m).astype(np.int64)
        assert (mi == np.asarray(m)).all() and mi.shape == (n, n)
        out[:, c0:c0 + n] = ki[:, c0:c0 + n] @ mi.T
        assert (np.abs(ki[:, c0:c0 + n]) @ np.abs(mi).T).max() < 1 << 24
    return np.ldexp(out.astype(np.float64), e).astype(np.float32)
