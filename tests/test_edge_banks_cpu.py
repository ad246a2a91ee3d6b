"""Edge values through the restatements of the strips, mix-matrix and mix-group banks, without a GPU: what lets
tests/test_edge_banks_gpu.py lean on them.  strips_ref against the oracle on the edge block bit for bit; mixmatrix_ref.classify
against the two summation orders of eval_f32 on the poisoned blocks the GPU test uses; scaled_int_product against eval_f32 on
subnormal data; and the sign of a sum of negative zeros, sequential against tree.  The blocks, matrices and tables of the GPU
test are built here, once, and imported there."""
import numpy as np
import pytest

import mixgroups_ref as R
import mixmatrix_ref as X
import oracle as O
import strips_ref as S
from edge_values import classes_present, edge_block, edge_channels, is_subnormal, same_bits_or_nan

F = np.float32
NF = 128

# ---- shared with the GPU half ----------------------------------------------------------------------------------------------------
T = [0, 1, 3, 34, 66, 99, 355]                       # rooms of 1, 2, 31, 32, 33 and 256
T64 = T + [384]                                      # ... padded to a multiple of the 64-channel tile by one more room (of 29)
BIG = [0, 1024]                                      # one room of 1024 alone
ROOM33, ROOM256 = 4, 5                               # indices into X.rooms(T)
MM_FRAMES = 37
GROUPS = [0, 1, 2, 40, 40, 100, 129, 300, 301, 1000, 1023, 1024, 1500, 2048]     # the mix-group table, N = 2048


class StripSetup:
    """masks, levels and raw sliders for n channels of K bands: channel c carries pattern c mod len(patterns(K)), as the strips'
    own GPU tests do; the oracle runs each channel's present nodes, and keeps them, so state carries from call to call."""

    def __init__(self, n, K, seed):
        rng = np.random.default_rng(seed)
        pats = S.patterns(K)
        self.n, self.K = n, K
        self.masks = np.asarray([pats[c % len(pats)] for c in range(n)], np.uint32)
        self.level = rng.uniform(0.0, 4.0, n).astype(F)
        self.raw = np.stack([S.stable_raw6(rng, n) for _ in range(K)])           # [band][channel][6]
        self._nodes = None

    def store(self, bank):
        """the same stores into a ChannelStrips or a strips_ref.Strips"""
        for c in range(self.n):
            if self.masks[c] & 1:
                bank.set_gain(self.level[c:c + 1], c)
            for b in range(self.K):
                if self.masks[c] & (1 << (1 + b)):
                    bank.set_band(b, self.raw[b, c:c + 1], c)

    def oracle(self, x, flags):
        """[frames][n] through the oracle, channel by channel, 128-frame blocks; the nodes are made at the first call"""
        if self._nodes is None:
            self._nodes = [S.oracle_nodes(O, int(self.masks[c]), self.level[c], [self.raw[b, c] for b in range(self.K)])
                           for c in range(self.n)]
        out = np.empty_like(x)
        for c in range(self.n):
            out[:, c] = O.chain_run(self._nodes[c], x[:, c], flags)
        return out


def strips_edge_block(n):
    """the edge block of the strips tests: level 1.0 (the clip and switch-point classes are ordinary finite values), 3 x 128"""
    return edge_block(n, 3 * NF, level=1.0)


def mm_noise(nf, n, seed):
    """the mix-matrix tests' noise: uniform in [-0.75, 1.25)"""
    return (np.random.default_rng(seed).uniform(-1.0, 1.0, (nf, n)) + 0.25).astype(F)


def poison_cases(table=T):
    """The mix-matrix edge blocks: name -> (x [37][N], mats, poisoned room index).  Every block is mm_noise with ONE room poisoned;
    the matrices are random with a third of the entries +0.0 (so a poisoned source meets wired and unwired entries), some columns
    negated, and silent rows in the poisoned rooms.
      nan_source   source 5 of the room of 33 is NaN in every frame
      inf_pair     source 7 of the room of 33 is +inf at frames 3 and 10, source 20 is -inf at frame 10
      inf_vs_zero  source 17 of the room of 256 is +inf at frames 3 and 10; listeners 0 .. 99 hold no zero entry (that column
                   positive for 0 .. 49, negative for 50 .. 99), listeners 100 .. 199 hold 0.0 in that column"""
    n_ch = table[-1]
    clean = mm_noise(MM_FRAMES, n_ch, 71)
    rooms = X.rooms(table)

    def mats():
        ms = X.random_mats(table, 72)
        m = ms[ROOM33]
        m[1::2, 7] *= F(-1.0)                         # odd listeners hear source 7 inverted
        m[0::3, 20] *= F(-1.0)
        m[11, :] = 0.0                                # silent rows
        m[30, :] = 0.0
        m = ms[ROOM256]
        rng = np.random.default_rng(73)
        m[:100, :] = rng.uniform(0.5, 10.0, (100, 256)).astype(F)
        m[50:100, 17] *= F(-1.0)
        m[100:200, 17] = 0.0
        m[210, :] = 0.0
        return ms

    cases = {}
    c33, c256 = rooms[ROOM33][0], rooms[ROOM256][0]
    x = clean.copy()
    x[:, c33 + 5] = np.nan
    cases["nan_source"] = (x, mats(), ROOM33)
    x = clean.copy()
    x[[3, 10], c33 + 7] = np.inf
    x[10, c33 + 20] = -np.inf
    cases["inf_pair"] = (x, mats(), ROOM33)
    x = clean.copy()
    x[[3, 10], c256 + 17] = np.inf
    cases["inf_vs_zero"] = (x, mats(), ROOM256)
    return clean, cases


def tree_sum(t):
    """[n][F] -> [F]: neighbours added pairwise in a tree, numpy float32 -- the shape of the bank's (x0 + x1) + (x2 + x3) and of
    its lane reductions; an odd element is carried up unchanged"""
    t = [np.asarray(r, F) for r in t]
    while len(t) > 1:
        nxt = [(a + b).astype(F) for a, b in zip(t[0::2], t[1::2])]
        if len(t) % 2:
            nxt.append(t[-1])
        t = nxt
    return t[0]


# ---- B1. strips_ref against the oracle on the edge block ---------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 3])
def test_strips_ref_equals_the_oracle_on_the_edge_block(flags):
    """N = 70, K = 3, every presence pattern, three blocks of 128: the numpy restatement gives the oracle's bits on NaN, +-inf,
    the inf / -inf pair, signed zeros, subnormals and huge values (NaN judged by isnan: x86 and numpy agree on the pattern, the
    payload is not compared).  This is what lets the GPU tests take either as the reference after a store or a reset."""
    n, K = 70, 3
    su = StripSetup(n, K, 900 + flags)
    x, table = strips_edge_block(n)
    ref = S.Strips(n, K, flags)
    su.store(ref)
    got = np.concatenate([ref.run(x[f0:f0 + NF]) for f0 in range(0, len(x), NF)])
    want = su.oracle(x, flags)
    same_bits_or_nan(got, want, table, "strips_ref against the oracle, link_flags %d" % flags)
    assert {"nan", "+inf", "-inf", "-0", "subnormal"} <= classes_present(want), classes_present(want)
    edge = sorted(edge_channels(n))
    assert np.isnan(want[:, edge]).sum() >= 100 and is_subnormal(want[:, edge]).sum() >= 4


# ---- B2. classify against the two orders of eval_f32 -------------------------------------------------------------------------------
@pytest.mark.parametrize("normalise", [True, False], ids=["normalise", "raw"])
@pytest.mark.parametrize("case", ["nan_source", "inf_pair", "inf_vs_zero"])
def test_classify_agrees_with_both_summation_orders(case, normalise):
    """The classification from the terms alone equals the NaN / +inf / -inf pattern of the ascending and of the pairwise f32
    evaluation, and where it says finite both lie inside the derived bound: the pattern is a property of the inputs, not of an
    order, which is why the GPU test may demand it of the MFMA chain."""
    clean, cases = poison_cases()
    x, mats, room = cases[case]
    cls = X.classify(x, T, mats, normalise)
    with np.errstate(all="ignore"):
        ref, sabs, n_of = X.exact(x, T, mats, normalise)
        bnd = X.bound(sabs, n_of)
        for order in ("ascending", "pairwise"):
            got = X.eval_f32(x, T, mats, normalise, order)
            assert np.array_equal(np.isnan(got), cls == "nan"), (order, np.argwhere(np.isnan(got) != (cls == "nan"))[:4])
            assert np.array_equal(np.isposinf(got), cls == "+inf"), order
            assert np.array_equal(np.isneginf(got), cls == "-inf"), order
            fin = cls == "finite"
            assert (np.abs(got[fin].astype(np.float64) - ref[fin]) <= bnd[fin]).all(), order
    c0, n = X.rooms(T)[room]
    inside = cls[:, c0:c0 + n]
    assert {"nan", "finite"} <= set(np.unique(inside)), np.unique(inside)
    if case != "nan_source":
        assert set(np.unique(inside)) == set(X.CLASSES), np.unique(inside)
    outside = np.delete(cls, np.s_[c0:c0 + n], axis=1)
    assert (outside == "finite").all()


def test_classify_refuses_inputs_that_could_overflow():
    x = np.full((1, 2), 1e30, F)
    with pytest.raises(AssertionError):
        X.classify(x, [0, 2], [np.full((2, 2), 1e30, F)])


# ---- B3. scaled_int_product ----------------------------------------------------------------------------------------------------------
def test_scaled_int_product_equals_eval_f32_on_subnormals():
    """Samples k * 2^-149, k integer in [-512, 512], asymmetric integer matrices in [-3, 3]: both f32 orders give the scaled
    integer product bit for bit at rooms of 1, 2, 31, 32, 33 and 256 members, and every nonzero output of a room of up to 33
    members is subnormal (33 * 3 * 512 < 2^23 = 2^-126 / 2^-149)."""
    k = np.random.default_rng(81).integers(-512, 513, (MM_FRAMES, T[-1]))
    x = np.ldexp(k.astype(np.float64), -149).astype(F)
    mats = [X.asymmetric(n) for _, n in X.rooms(T)]
    want = X.scaled_int_product(k, T, mats, -149)
    for order in ("ascending", "pairwise"):
        got = X.eval_f32(x, T, mats, False, order)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), order
    for c0, n in X.rooms(T):
        w = want[:, c0:c0 + n]
        assert (w != 0).mean() > 0.5, (c0, n)
        if n <= 33:
            assert is_subnormal(w[w != 0]).all(), (c0, n)
    assert is_subnormal(x[x != 0]).all() and (x != 0).mean() > 0.99


# ---- B4. the sign of a sum of negative zeros -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4, 59, 256, 699])
def test_sequential_sum_of_negative_zeros_is_plus_zero_and_a_tree_is_not(n):
    """collect_and_average (node.rs:162-194) starts from +0.0 and adds pipe by pipe: pipes that are all -0.0 -- silence through
    a negative fader, +0.0 * -1.0 -- give +0.0.  The same values added in a tree give -0.0, (-0) + (-0) = -0: a bank that sums
    in a tree has to add +0.0 to the finished sum to give the reference's bus."""
    pipes = (np.zeros((n, 5), F) * F(-1.0)).astype(F)
    assert np.signbit(pipes).all()
    ref = R.collect_and_average(pipes)
    assert (ref.view(np.uint32) == 0).all()
    tree = tree_sum(pipes)
    assert (tree.view(np.uint32) == 0x80000000).all()
    assert ((F(0.0) + tree).astype(F).view(np.uint32) == 0).all()
