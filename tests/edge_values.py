"""Edge-value blocks and the strict comparison for them: NaN, infinities, signed zeros, subnormals, the clip points and
the fast f64 functions' own switch points, each class in a channel of its own next to plain-noise neighbours.

`ulp_diff` (chains.py) maps +0.0 and -0.0 to one point and NaN == NaN to 0; `same_values` adds what it leaves out: the NaN
pattern, the sign of infinities and the sign of every zero the reference gives."""
import numpy as np

import oracle as O
from chains import ulp_diff

F = np.float32
U = np.uint32


def _bits(v):
    return np.array(v, U).view(F)


def _around(v):
    """v and its two f32 neighbours."""
    v = F(v)
    return [np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]


def _pm(vals):
    vals = [F(v) for v in vals]
    return vals + [F(-v) for v in vals]


def edge_classes(level):
    """name -> (values, finite).  A tuple among the values is written into consecutive frames."""
    L = F(level)
    sub_max = _bits(0x007FFFFF)
    nan_q, nan_neg, nan_payload = _bits(0x7FC00000), _bits(0xFFC00000), _bits(0x7FC12345)
    return {
        "zeros_subnormals": (_pm([0.0, 2.0 ** -149, sub_max, 2.0 ** -126]), True),
        "clip_unit": (_pm(_around(1.0)), True),
        "clip_level": (_pm(_around(F(1.0) / L)), True),
        "tanh_clamp_20": (_pm(_around(F(20.0) / L)), True),
        "sin_handover_2p22": (_pm(_around(F(2.0 ** 22) / L)), True),
        "exp_clamp": (_around(F(89.0) / L) + _around(F(-160.0) / L) + [F(-89.0) / L, F(160.0) / L], True),
        "large": (_pm([3.4028235e38, 1e15, 1e20]), True),
        "inf": ([F(np.inf), F(-np.inf)], False),
        "inf_pair": ([(F(np.inf), F(-np.inf))], False),
        "nan": ([nan_q, nan_neg, nan_payload], False),
    }


CLASS_NAMES = list(edge_classes(1.0))


def edge_channels(N):
    """channel -> class name.  Every class sits once in the first channels (consecutive: both halves of a lane pair of the
    two-channel-per-lane kernels) and, when there is room, once more in the last channels (the guarded tail of a ragged
    engine: N = 100 -> channels 90..99, N = 418 -> 408..417); every other channel is an innocent neighbour."""
    k = len(CLASS_NAMES)
    assert N >= k, N
    table = {i: name for i, name in enumerate(CLASS_NAMES)}
    if N >= 2 * k + 2:
        for i, name in enumerate(CLASS_NAMES):
            table[N - k + (i + 1) % k] = name     # rotated by one: a class meets the other half of a lane pair there
    return table


def edge_block(N, frames, level=3.0, seed=0x5EED0E01, block=128):
    """([frames][N] f32, {channel: class name}).  The layout, all of it:
      * channels outside the table are plain O.noise: the innocent neighbours;
      * an edge channel is noise in which ONE class is written, so a block-global maximum (Fuzz's) can be attributed;
      * a finite class is written into every 128-frame block, a non-finite one into the second block only (every block
        when there is just one), so that a recurrence is seen clean, poisoned, and after the poison;
      * in a block that is written, value k of the class goes to frame 3 + 7 k, and frame 0 -- the sample a control-port
        latch takes -- gets value (block index) mod (number of values);
      * the zeros / subnormals channel is silent instead of noisy in its first block, so that a filter's state stays tiny
        and its answer subnormal."""
    x = O.noise(seed, np.arange(N), np.arange(frames)).copy()
    table = edge_channels(N)
    classes = edge_classes(level)
    n_blocks = max(1, frames // block)
    for c, name in table.items():
        vals, finite = classes[name]
        if name == "zeros_subnormals":
            x[:min(block, frames), c] = 0.0
        for b in (range(n_blocks) if finite or n_blocks == 1 else [1]):
            f0 = b * block
            for k, v in enumerate(vals):
                f = f0 + 3 + 7 * k
                for j, w in enumerate(v if isinstance(v, tuple) else (v,)):
                    if f + j < min(frames, f0 + block):
                        x[f + j, c] = w
            first = vals[b % len(vals)]
            x[f0, c] = first[0] if isinstance(first, tuple) else first
    return x, table


def classes_present(a):
    """Which of the special classes occur in an array."""
    a = np.asarray(a, F)
    out = set()
    if np.isnan(a).any():
        out.add("nan")
    if np.isposinf(a).any():
        out.add("+inf")
    if np.isneginf(a).any():
        out.add("-inf")
    if ((a == 0) & np.signbit(a)).any():
        out.add("-0")
    if ((a != 0) & (np.abs(a) < F(2.0 ** -126))).any():
        out.add("subnormal")
    return out


def is_subnormal(a):
    a = np.asarray(a, F)
    with np.errstate(invalid="ignore"):
        return (a != 0) & (np.abs(a) < F(2.0 ** -126))


def first_difference(got, ref, bar):
    """Index of the first element where `got` is not `ref` in the strict sense, with a word on why; None when equal."""
    got, ref = np.asarray(got, F), np.asarray(ref, F)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    gi, ri = np.isinf(got), np.isinf(ref)
    with np.errstate(invalid="ignore"):
        bad_nan = gn != rn
        bad_inf = ((gi | ri) & ~(gn | rn)) & ((gi != ri) | (np.signbit(got) != np.signbit(ref)))
        bad_zero = (ref == 0) & ~gn & (np.signbit(got) != np.signbit(ref))
        d = ulp_diff(got, ref)
        bad_ulp = ~(gn | rn | gi | ri) & (d > bar)
    bad = bad_nan | bad_inf | bad_zero | bad_ulp
    if not bad.any():
        return None
    idx = tuple(int(i) for i in np.argwhere(bad)[0])
    why = "NaN pattern" if bad_nan[idx] else "infinity" if bad_inf[idx] else "sign of zero" if bad_zero[idx] else "%d ulp > %d" % (d[idx], bar)
    return idx, why, int(bad.sum())


def same_values(got, ref, bar, table=None, what=""):
    """The strict comparison: the isnan patterns are equal (payload and sign of a NaN are NOT compared: x86 and the GPU
    propagate them differently), infinities are equal with their sign, where `ref` is +-0 `got` has its sign bit, and
    everywhere else ulp_diff <= bar.  Raises AssertionError naming the frame, channel and channel class of the first
    difference; returns True otherwise."""
    diff = first_difference(got, ref, bar)
    if diff is None:
        return True
    idx, why, count = diff
    got, ref = np.asarray(got, F), np.asarray(ref, F)
    cls = None
    if table is not None and len(idx) == 2:
        cls = table.get(idx[1], "noise")
    where = "frame %d channel %d (%s)" % (idx[0], idx[1], cls) if len(idx) == 2 else "index %r" % (idx,)
    raise AssertionError("%s: %s at %s: got %r (0x%08x), reference %r (0x%08x); %d elements differ" % (
        what, why, where, float(got[idx]), int(got.view(U)[idx]), float(ref[idx]), int(ref.view(U)[idx]), count))


def same_bits_or_nan(got, base, table=None, what=""):
    """Two kernels that perform the same operations: the same bits, NaN judged by isnan."""
    got, base = np.asarray(got, F), np.asarray(base, F)
    nan = np.isnan(base)
    ok = (got.view(U) == base.view(U)) | (nan & np.isnan(got))
    if ok.all():
        return True
    idx = tuple(int(i) for i in np.argwhere(~ok)[0])
    cls = table.get(idx[-1], "noise") if table is not None else None
    raise AssertionError("%s: bits differ at %r (%s): 0x%08x against 0x%08x; %d elements differ" % (
        what, idx, cls, int(got.view(U)[idx]), int(base.view(U)[idx]), int((~ok).sum())))


def worst_ulp_by_class(got, ref, table):
    """{class name: the largest ulp_diff over the elements where both are finite}, "noise" for the channels outside the table."""
    got, ref = np.asarray(got, F), np.asarray(ref, F)
    fin = np.isfinite(got) & np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        d = np.where(fin, ulp_diff(got, ref), 0)
    worst = {}
    for c in range(ref.shape[1]):
        name = table.get(c, "noise")
        worst[name] = max(worst.get(name, 0), int(d[:, c].max()))
    return worst
