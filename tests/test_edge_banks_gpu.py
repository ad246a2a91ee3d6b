"""Edge-value parity for the three banks that carry samples: channel strips, mix matrix, mix groups with their returns.
NaN, +-inf, the inf / -inf pair, signed zeros, subnormals and huge values, through the strict comparison of tests/edge_values.py.
No assertion rests on a measured constant: the strips have the oracle at their existing bars (1 ulp, 0 for nodeless and
Gain-only channels); the mix matrix and the buses have cases that are exact in f32, whose bits follow from integer arithmetic
(mixmatrix_ref.scaled_int_product), the derived bounds (mixmatrix_ref.bound), and non-finite patterns that follow from
classifying the terms (mixmatrix_ref.classify).  Every test asserts that its reference really holds the classes it is about.
The blocks, tables and matrices are built in tests/test_edge_banks_cpu.py, which checks the references themselves."""
import numpy as np
import pytest

import mixgroups_ref as R
import mixmatrix_ref as X
import mixreturns_ref as M
import oracle as O
import strips_ref as S
import test_mixmatrix_gpu as MMT
from edge_values import classes_present, is_subnormal, same_bits_or_nan, same_values, worst_ulp_by_class
from test_edge_banks_cpu import (BIG, GROUPS, MM_FRAMES, NF, ROOM33, ROOM256, T, T64, StripSetup, mm_noise, poison_cases,
                                 strips_edge_block)
from test_strips_gpu import bits, run_blocks, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
STRIP_SHAPES = [(70, 0), (256, 64)]      # scalar lanes with a ragged last group; four channels a lane at K = 2, two at K = 3
TINY = 2.0 ** -149


# =================================================================================================================================
# C. channel strips
# =================================================================================================================================
_strip_refs = {}


def strips_case(n, K, flags):
    """(setup, edge block, channel table, the oracle's output), made once per case and left unchanged"""
    key = (n, K, flags)
    if key not in _strip_refs:
        su = StripSetup(n, K, 1100 + 10 * K + flags)
        x, table = strips_edge_block(n)
        ref = su.oracle(x, flags)
        ref.setflags(write=False)
        _strip_refs[key] = (su, x, table, ref)
    return _strip_refs[key]


def strips_bank(dspfx, su, tile, flags, nf=NF):
    bank = dspfx.ChannelStrips(su.n, bands=su.K, tile_channels=tile, max_frames=nf, link_flags=flags)
    su.store(bank)
    return bank


def plain_channels(su):
    return (su.masks & ~np.uint32(1)) == 0                       # no band: nodeless or Gain only


def strict(got, ref, su, table, what):
    """the bank's existing bars in the strict sense: 1 ulp everywhere, 0 on the nodeless and the Gain-only channels"""
    same_values(got, ref, 1, table, what)
    plain = np.flatnonzero(plain_channels(su))
    same_values(got[:, plain], ref[:, plain], 0, {i: "%s, channel %d" % (table.get(c, "noise") if table else "?", c) for i, c in enumerate(plain)},
                what + ", nodeless and Gain-only channels")


@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("n,tile", STRIP_SHAPES)
def test_strips_parity_on_the_edge_block(dspfx, torch_cuda, n, tile, K, flags):
    """The edge block through every presence pattern against the oracle: NaN pattern, signed infinities, the sign of every zero
    the oracle gives, then 1 ulp (0 on nodeless and Gain-only channels).  The edge channels at both ends of the block meet
    different node sets, and in the vector form several classes share one lane, so a `pick` that takes the wrong side, a
    band-less channel's discarded y leaking out, or a wave-uniform skip decided on the wrong lanes changes a NaN pattern here;
    a kernel that flushes subnormals loses the subnormal class of the Gain-only channels (0 ulp bar).  K = 2 launches
    strips_run<2, 4> (256 tiled) and strips_run<2, 1> (70), which no other shape of the suite reaches."""
    su, x, table, ref = strips_case(n, K, flags)
    bank = strips_bank(dspfx, su, tile, flags)
    got = run_blocks(dspfx, torch_cuda, bank, x, n, tile)
    bank.close()
    print("strips edge block N=%d tile=%d K=%d link_flags=%d: worst ulp per class %r" % (n, tile, K, flags, worst_ulp_by_class(got, ref, table)))
    strict(got, ref, su, table, "strips N=%d tile=%d K=%d lf=%d" % (n, tile, K, flags))
    assert {"nan", "+inf", "-inf", "-0", "subnormal"} <= classes_present(ref), classes_present(ref)
    edge = sorted(table)
    assert np.isnan(ref[:, edge]).sum() >= 100 and is_subnormal(ref[:, edge]).sum() >= 4
    assert np.isfinite(ref[:, [c for c in range(n) if c not in table]]).all()


@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("n,tile", STRIP_SHAPES)
def test_strips_edge_channels_change_no_neighbour(dspfx, torch_cuda, n, tile, K, flags):
    """Every channel outside the edge channels has the bits of a run in which the edge channels carried plain noise: a select
    that leaks a lane-mate's NaN, infinity or state (four channels share a lane at K = 2) fails here."""
    su, x, table, ref = strips_case(n, K, flags)
    plain = O.noise(0x5EED0E01, np.arange(n), np.arange(len(x))).copy()
    others = np.asarray([c for c in range(n) if c not in table])
    assert np.array_equal(bits(plain[:, others]), bits(x[:, others])) and not np.isfinite(x[:, sorted(table)]).all()
    outs = []
    for data in (plain, x):
        bank = strips_bank(dspfx, su, tile, flags)
        outs.append(run_blocks(dspfx, torch_cuda, bank, data, n, tile))
        bank.close()
    assert np.isfinite(outs[0]).all()
    assert np.array_equal(bits(outs[0][:, others]), bits(outs[1][:, others]))
    assert np.array_equal(np.isnan(outs[1]), np.isnan(ref)) and np.isnan(ref).any()


TAIL_RAW = np.asarray([1.0, -0.5, 0.25, 1.0, 0.0, 0.0], F)       # poles of radius 0.5 (z^2 - 0.5 z + 0.25), b0 = 1
TAIL_AT = NF - 40                                                # the impulse's frame: 2^-100 x 0.5^40 is subnormal where the first call ends


def tails_case(n):
    """masks, input and the oracle's output of the subnormal-tails test.  Channels come in runs of 24 of one kind: Gain(0.5)
    only, the one band only, Gain(0.5) then the band.  The band channels get an impulse of 1.5 * 2^-(100 + c % 24): the response
    decays by 0.5 per frame through the whole subnormal range.  A Gain(0.5) alone only halves its input, and 1.5 * 2^-(101 + 23)
    is still normal, so the Gain-only channels get the same impulse 24 octaves lower, 1.5 * 2^-(124 + c % 24): subnormal inputs
    and subnormal products, the deepest rounded to even.  The impulse sits 40 frames before the end of the first call, so the
    shallower band channels carry a subnormal filter state from one call into the next."""
    kind = (np.arange(n) // 24) % 3
    masks = np.asarray([1, 2, 3], np.uint32)[kind]
    x = np.zeros((2 * NF, n), F)
    x[TAIL_AT] = (1.5 * np.exp2(-(100.0 + np.arange(n) % 24 + 24.0 * (kind == 0)))).astype(F)
    ref = np.empty_like(x)
    for c in range(n):
        ref[:, c] = O.chain_run(S.oracle_nodes(O, int(masks[c]), 0.5, [TAIL_RAW]), x[:, c], 0)
    return kind, masks, x, ref


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("n,tile", STRIP_SHAPES)
def test_strips_subnormal_tails_are_not_flushed(dspfx, torch_cuda, n, tile, K):
    """Modelled on test_subnormal_tails_are_not_flushed: impulses that decay through the subnormal range, link flags 0, 256
    frames in two calls (the state crosses the call subnormal).  Gain-only channels bit for bit, the band channels at the strict
    1 ulp.  Per kind the reference holds at least 20 distinct subnormal samples of magnitude >= 4 x 2^-149 -- a flushed result
    is then at least 4 ulp off, whichever way the flush goes (input, product or output) -- and the last frame is zero."""
    kind, masks, x, ref = tails_case(n)
    for k in range(3):
        vals = ref[:, kind == k]
        deep = is_subnormal(vals) & (np.abs(vals) >= F(4 * TINY))
        assert len(np.unique(vals[deep].view(np.uint32))) >= 20, (k, len(np.unique(vals[deep].view(np.uint32))))
    assert (ref[-1] == 0).all() and is_subnormal(ref[NF]).sum() >= 8
    bank = dspfx.ChannelStrips(n, bands=K, tile_channels=tile, max_frames=NF, link_flags=0)
    for c in range(n):
        if masks[c] & 1:
            bank.set_gain(0.5, c, 1)
        if masks[c] & 2:
            bank.set_band(0, TAIL_RAW, c, 1)
    got = run_blocks(dspfx, torch_cuda, bank, x, n, tile)
    bank.close()
    table = {c: "kind %d" % kind[c] for c in range(n)}
    same_values(got, ref, 1, table, "subnormal tails N=%d tile=%d K=%d" % (n, tile, K))
    same_bits_or_nan(got[:, kind == 0], ref[:, kind == 0], what="Gain-only subnormal tails")


@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("n,tile", STRIP_SHAPES)
def test_strips_edge_sliders(dspfx, torch_cuda, n, tile, K, flags):
    """Slider values at the edges, on plain noise, against the oracle in the strict sense: levels -0.0 (a Gain-only channel: the
    sign of every zero shows), +inf and NaN; raw sliders with a0 = 0 (dspfx_strips_coeffs divides on purpose: +-inf, and NaN where
    the numerator is 0 too); raw sliders that are all subnormal with a0 = 2^-140 (the quotients are an ordinary filter: a host
    that flushes subnormals makes them 0 / 0); and the same with one quotient that overflows.  Every other channel keeps the bits
    of a run with ordinary sliders in those channels."""
    full = (1 << (1 + K)) - 1
    t = 2.0 ** -140
    touched = [5, 6, 7, 9, 10, 13]

    def setup(edge):
        su = StripSetup(n, K, 1200 + 10 * K + flags)
        su.masks[touched] = full
        su.masks[5] = 1
        if edge:
            su.level[5], su.level[6], su.level[7] = -0.0, np.inf, np.nan
            su.raw[0, 9] = [0.0, 1.0, -1.0, 0.0, 2.0, -3.0]
            su.raw[0, 10] = [t, -0.5 * t, 0.25 * t, t, 0.0, 0.0]
            su.raw[K - 1, 13] = [t, -0.5 * t, 0.25 * t, t, 0.0, 1.0]
        return su

    x = S.noise(np.random.default_rng(n + K), 3 * NF, n)
    outs = []
    for edge in (False, True):
        su = setup(edge)
        bank = strips_bank(dspfx, su, tile, flags)
        outs.append(run_blocks(dspfx, torch_cuda, bank, x, n, tile))
        bank.close()
    base, got = outs
    ref = su.oracle(x, flags)
    k9, k10, k13 = S.coeffs(su.raw[0, 9]), S.coeffs(su.raw[0, 10]), S.coeffs(su.raw[K - 1, 13])
    assert np.isinf(k9[[0, 1, 3, 4]]).all() and np.isnan(k9[2]) and is_subnormal(su.raw[0, 10][[0, 1, 2, 3]]).all()
    assert np.array_equal(k10, np.asarray([-0.5, 0.25, 1.0, 0.0, 0.0], F)) and np.isposinf(k13[4]) and np.isfinite(k13[:4]).all()
    table = {5: "level -0.0", 6: "level +inf", 7: "level NaN", 9: "a0 = 0", 10: "a0 = 2^-140", 13: "a0 = 2^-140, b2 / a0 = inf"}
    strict(got, ref, su, table, "edge sliders N=%d tile=%d K=%d lf=%d" % (n, tile, K, flags))
    assert np.isfinite(ref[:, 10]).all() and np.isnan(ref[:, [7, 9, 13]]).all(axis=0).all() and not np.isfinite(ref[:, 6]).any()
    if flags == 0:                                               # (x * -0.0: a zero of either sign, by the sign of the sample)
        assert (ref[:, 5] == 0).all() and 0 < np.signbit(ref[:, 5]).sum() < len(ref)
    others = np.asarray([c for c in range(n) if c not in touched])
    assert np.array_equal(bits(got[:, others]), bits(base[:, others])) and np.isfinite(base).all()


@pytest.mark.parametrize("clearing", ["reset", "band_store"])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n,tile", STRIP_SHAPES)
def test_strips_documented_clearings_remove_the_poison(dspfx, torch_cuda, n, tile, K, clearing):
    """+inf followed by -inf one frame later in one channel (NaN is made inside the filter state) and one NaN in another, during
    block 0, into full strips.  Blocks 0 and 1 follow the oracle; the poison stays.  Then reset(), or a store of band 0 on the
    two channels, each against strips_ref after the same operation: reset() makes the channels finite again; a band store
    clears that band alone -- a one-band bank is finite again, and in a three-band bank bands 1 and 2 still hold NaN until
    they are dropped, after which the output is Gain and band 0 alone and finite: band 0's state is clean.  State that a
    documented clearing leaves NaN (a reset that scales by zero, a store that misses a row of the state) fails here."""
    flags = 3
    su = StripSetup(n, K, 1300 + K)
    su.masks[:] = (1 << (1 + K)) - 1
    x = S.noise(np.random.default_rng(1301), 4 * NF, n)
    a, b = 5, n - 3
    x[10, a], x[11, a], x[20, b] = np.inf, -np.inf, np.nan
    table = {a: "inf_pair", b: "nan"}
    bank = strips_bank(dspfx, su, tile, flags)
    sref = S.Strips(n, K, flags)
    su.store(sref)

    def block(i):
        sl = slice(i * NF, (i + 1) * NF)
        return run_blocks(dspfx, torch_cuda, bank, x[sl], n, tile), sref.run(x[sl]), sl

    for i in range(2):
        got, r, sl = block(i)
        ref = su.oracle(x[sl], flags)
        same_values(got, ref, 1, table, "poisoned block %d" % i)
        same_bits_or_nan(r, ref, table, "strips_ref, poisoned block %d" % i)
    assert np.isnan(ref[:, [a, b]]).all() and np.isfinite(np.delete(ref, [a, b], axis=1)).all()
    if clearing == "reset":
        bank.reset()
        sref.reset()
        got, r, _ = block(2)
        same_values(got, r, 1, table, "after reset()")
        assert np.isfinite(r).all() and np.isfinite(got).all()
    else:
        for c in (a, b):
            bank.set_band(0, su.raw[0, c:c + 1], c)
            sref.set_band(0, su.raw[0, c:c + 1], c)
        got, r, _ = block(2)
        same_values(got, r, 1, table, "after the band-0 store")
        assert np.isfinite(r[:, [a, b]]).all() == (K == 1)
        for band in range(1, K):
            for c in (a, b):
                bank.set_band(band, None, c, 1)
                sref.set_band(band, None, c, 1)
        got, r, _ = block(3)
        same_values(got, r, 1, table, "after the band-0 store, the other bands dropped")
        assert np.isfinite(r).all() and np.isfinite(got).all()
    bank.close()


@pytest.mark.parametrize("K", [2, 3])
def test_strips_misaligned_block_gives_the_same_bits(dspfx, torch_cuda, K):
    """N = 256 frame-major with `in` and `out` one float into a larger tensor: not 16-byte aligned, so the run takes one channel
    a lane although N % 4 == 0.  The edge block gives the bits of the aligned run, and the floats around `out` are untouched."""
    torch = torch_cuda
    n, flags = 256, 3
    su, x, table, ref = strips_case(n, K, flags)
    aligned = strips_bank(dspfx, su, 0, flags)
    base = run_blocks(dspfx, torch, aligned, x, n, 0)
    aligned.close()
    bank = strips_bank(dspfx, su, 0, flags)
    outs = []
    for f0 in range(0, len(x), NF):
        src = torch.zeros(NF * n + 8, dtype=torch.float32, device="cuda")
        dst = torch.full((NF * n + 8,), 7.0, dtype=torch.float32, device="cuda")
        dx, dy = src[1:1 + NF * n], dst[1:1 + NF * n]
        dx.copy_(torch.from_numpy(np.ascontiguousarray(x[f0:f0 + NF]).reshape(-1)))
        assert dx.data_ptr() % 16 == 4 and dy.data_ptr() % 16 == 4
        bank.run(dx, NF, out=dy)
        torch.cuda.synchronize()
        h = dst.cpu().numpy()
        assert h[0] == 7.0 and (h[1 + NF * n:] == 7.0).all()
        outs.append(h[1:1 + NF * n].reshape(NF, n))
    bank.close()
    got = np.concatenate(outs)
    same_bits_or_nan(got, base, table, "misaligned against aligned, K=%d" % K)
    strict(got, ref, su, table, "misaligned K=%d" % K)
    assert {"nan", "+inf", "-inf", "-0", "subnormal"} <= classes_present(ref)


# =================================================================================================================================
# D. mix matrix
# =================================================================================================================================
MM_LAYOUTS = {"frame_major": (T, 0), "tile64": (T64, 64)}


def subnormal_samples(nf, n, seed):
    """integers k in [-512, 512] and the samples k * 2^-149 they stand for"""
    k = np.random.default_rng(seed).integers(-512, 513, (nf, n))
    x = np.ldexp(k.astype(np.float64), -149).astype(F)
    assert is_subnormal(x[x != 0]).all()
    return k, x


def divided(want, mats):
    """fl32(sum / d) in numpy float32 from the exact f32 sums; +0.0 for a row without a wired entry"""
    d, wired = X.divisors(mats, True)
    out = (want / d.astype(F)[None, :]).astype(F)
    out[:, ~wired] = F(0.0)
    return out


def mm_run(dspfx, torch, table, tile, mats, x, normalise, stores=None):
    mm = MMT.bank(dspfx, table, tile, x.shape[0], normalise, mats)
    try:
        if stores:
            stores(mm)
        return MMT.run(dspfx, torch, mm, x, tile)
    finally:
        mm.close()


@pytest.mark.parametrize("layout", ["frame_major", "tile64", "room_of_1024"])
def test_mixmatrix_exact_on_subnormals(dspfx, torch_cuda, layout):
    """Samples k * 2^-149, |k| <= 512, against asymmetric integer matrices in [-3, 3], raw sums: every product and every partial
    sum is an integer below 2^24 times 2^-149, exact in f32, so the output is scaled_int_product bit for bit -- subnormal in the
    rooms of up to 33 members, crossing into the normal range at 1024.  The samples are the MFMA's A operand: a kernel whose
    denormal mode flushes them gives +0.0 everywhere, and one that flushes results loses the small rooms.  Then the division:
    normalise = 1 gives fl32(sum / d) of the exact sum, a correctly rounded division of a subnormal."""
    table, tile = MM_LAYOUTS.get(layout, (BIG, 0))
    k, x = subnormal_samples(MM_FRAMES, table[-1], 91)
    mats = [X.asymmetric(n) for _, n in X.rooms(table)]
    want = X.scaled_int_product(k, table, mats, -149)
    for c0, n in X.rooms(table):
        if n > 1:
            assert (want[:, c0:c0 + n] != 0).mean() > 0.5, (c0, n)
    assert is_subnormal(want).mean() > 0.5
    got = mm_run(dspfx, torch_cuda, table, tile, mats, x, False)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, ("raw", len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    want = divided(want, mats)
    assert is_subnormal(want).mean() > 0.5
    got = mm_run(dspfx, torch_cuda, table, tile, mats, x, True)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, ("normalise", len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("layout", ["frame_major", "tile64"])
def test_mixmatrix_a_subnormal_wire_is_a_wire(dspfx, torch_cuda, layout):
    """The room of 33 holds nothing but subnormal entries, integer multiples of 2^-149: source 9's column stored as 2^-149 for
    everybody through set_cols, then by row stores one listener with a lone entry of 2^-149, one with five, one with three
    entries of +-3 x 2^-149, and one whose row is all -0.0 (silent: +0.0).  Integer samples, normalise = 1: the sum is exact, so
    the output is fl32(exact / link_divisor(w)) bit for bit with w counted as `!= 0` counts it.  A recount that flushes, or that
    compares magnitudes with a threshold, finds w = 0 and writes +0.0; one that counts -0.0 divides the silent row's +0.0 and is
    caught by the count of the others."""
    table, tile = MM_LAYOUTS[layout]
    c0, n = X.rooms(table)[ROOM33]
    k = MMT.integers(MM_FRAMES, table[-1], 92).astype(np.int64)
    ints = [X.asymmetric(m) for _, m in X.rooms(table)]          # what scaled_int_product multiplies
    room = np.zeros((n, n), F)
    room[:, 9] = 1.0                                             # the column store
    lone, five, three, silent = 4, 12, 20, 27
    room[lone, :] = 0.0
    room[lone, 30] = 1.0
    room[five, :] = 0.0
    room[five, [0, 7, 9, 16, 32]] = 1.0
    room[three, :] = 0.0
    room[three, [1, 2, 31]] = [3.0, -3.0, 3.0]
    room[silent, :] = 0.0
    ints[ROOM33] = room
    mats = [m.copy() for m in ints]
    mats[ROOM33] = (room * F(TINY)).astype(F)
    mats[ROOM33][silent, :] = F(-0.0)
    assert is_subnormal(mats[ROOM33][room != 0]).all() and np.signbit(mats[ROOM33][silent]).all()

    def stores(mm):
        mm.fill(ROOM33, dspfx.MIXMATRIX_ZERO)
        mm.set_cols(np.full((1, n), TINY, F), c0 + 9)
        for l in (lone, five, three, silent):
            mm.set_rows(mats[ROOM33][l], c0 + l)

    got = mm_run(dspfx, torch_cuda, table, tile, ints, k.astype(F), True, stores)
    sums = X.scaled_int_product(k, table, ints, 0)
    sums[:, c0:c0 + n] = X.scaled_int_product(k, table, ints, -149)[:, c0:c0 + n]
    d, wired = X.divisors(mats, True)
    w_of = {lone: 1, five: 5, three: 3}
    for l, w in w_of.items():
        assert d[c0 + l] == float(R.link_divisor(w))
    assert not wired[c0 + silent] and (d[c0:c0 + n][np.delete(np.arange(n), [lone, five, three, silent])] == float(R.link_divisor(1))).all()
    want = divided(sums, mats)
    inside = want[:, c0:c0 + n]
    assert (np.delete(inside, silent, axis=1) != 0).mean() > 0.9 and is_subnormal(inside[inside != 0]).all()
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, (len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    assert (bits(got[:, c0 + silent]) == 0).all()


@pytest.mark.parametrize("layout", ["frame_major", "tile64"])
@pytest.mark.parametrize("case", ["nan_source", "inf_pair", "inf_vs_zero"])
def test_mixmatrix_poison_reaches_every_listener_of_its_room_and_no_other(dspfx, torch_cuda, case, layout):
    """"Unwired entries are multiplications by zero, not omissions", the half that had no test: a NaN source makes every wired
    listener of its room NaN; +inf against a 0.0 entry is NaN, against a positive entry +inf, against a negative one -inf; +inf and
    -inf from two sources are NaN.  The NaN / +inf / -inf pattern equals mixmatrix_ref.classify per frame and listener (a kernel
    that skips zero entries gives a finite value or an infinity where this demands NaN); silent rows are +0.0 bitwise with NaN in the
    room; where the class is finite the derived bound holds; every other room has the bits of the clean run."""
    table, tile = MM_LAYOUTS[layout]
    clean, cases = poison_cases(table)
    x, mats, room = cases[case]
    cls = X.classify(x, table, mats, True)
    c0, n = X.rooms(table)[room]
    inside = np.zeros(table[-1], bool)
    inside[c0:c0 + n] = True
    assert (cls[:, ~inside] == "finite").all() and {"nan", "finite"} <= set(np.unique(cls[:, inside]))
    if case != "nan_source":
        assert set(np.unique(cls[:, inside])) == set(X.CLASSES)
    mm = MMT.bank(dspfx, table, tile, MM_FRAMES, True, mats)
    try:
        base = MMT.run(dspfx, torch_cuda, mm, clean, tile)
        got = MMT.run(dspfx, torch_cuda, mm, x, tile)
    finally:
        mm.close()
    assert np.isfinite(base).all()
    for name, fn in (("nan", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        bad = np.argwhere(fn(got) != (cls == name))
        assert len(bad) == 0, (name, len(bad), bad[:5])
    _, wired = X.divisors(mats, True)
    silent = np.flatnonzero(~wired & inside)
    assert len(silent) >= 1 and (bits(got[:, silent]) == 0).all(), "a silent row is +0.0 whatever is in the room"
    with np.errstate(all="ignore"):
        ref, sabs, n_of = X.exact(x, table, mats, True)
        fin = cls == "finite"
        ratio = np.abs(got[fin].astype(np.float64) - ref[fin]) / X.bound(sabs, n_of)[fin]
    print("mixmatrix %s %s: worst err / bound where finite = %.4f" % (case, layout, float(ratio.max())))
    assert (ratio <= 1.0).all()
    assert (bits(got[:, ~inside]) == bits(base[:, ~inside])).all(), "the other rooms: the bits of the clean run"


def test_mixmatrix_edge_entries(dspfx, torch_cuda):
    """Matrix entries of +inf, NaN and 1e30 against finite noise, in the rooms of 33 and 256: a row whose ONLY nonzero entry is
    inf or NaN is wired (`!= 0` is true of both), so its output is +-inf by the sample's sign, or NaN, and not the +0.0 of a silent
    row; the same entries inside ordinary rows; and a 1e30 entry inside the derived bound with the divisor of its wired count."""
    table, tile = T, 0
    x = mm_noise(MM_FRAMES, table[-1], 93)
    mats = X.random_mats(table, 94)
    for r in (ROOM33, ROOM256):
        m = mats[r]
        m[2, :], m[3, :] = 0.0, 0.0
        m[2, 6], m[3, 8] = np.inf, np.nan
        m[4, 10], m[5, 12], m[6, 14] = 1e30, -np.inf, np.nan
    cls = X.classify(x, table, mats, True)
    got = mm_run(dspfx, torch_cuda, table, tile, mats, x, True)
    for name, fn in (("nan", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        bad = np.argwhere(fn(got) != (cls == name))
        assert len(bad) == 0, (name, len(bad), bad[:5])
    d, wired = X.divisors(mats, True)
    for r in (ROOM33, ROOM256):
        c0 = table[r]
        assert wired[c0 + 2] and wired[c0 + 3] and d[c0 + 2] == float(R.link_divisor(1)) == d[c0 + 3]
        assert (np.isposinf(got[:, c0 + 2]) == (x[:, c0 + 6] > 0)).all() and (np.isneginf(got[:, c0 + 2]) == (x[:, c0 + 6] < 0)).all()
        assert np.isnan(got[:, c0 + 3]).all() and np.isnan(got[:, c0 + 6]).all() and np.isinf(got[:, c0 + 5]).all()
    assert set(np.unique(cls)) == set(X.CLASSES)
    with np.errstate(all="ignore"):
        ref, sabs, n_of = X.exact(x, table, mats, True)
        fin = cls == "finite"
        ratio = np.abs(got[fin].astype(np.float64) - ref[fin]) / X.bound(sabs, n_of)[fin]
    print("mixmatrix edge entries: worst err / bound where finite = %.4f" % float(ratio.max()))
    assert (ratio <= 1.0).all() and np.abs(ref[:, [table[ROOM33] + 4, table[ROOM256] + 4]]).max() > 1e27


def test_mixmatrix_zeros_are_plus_zero(dspfx, torch_cuda):
    """A room whose samples are all -0.0 gives +0.0 everywhere (the accumulator starts at +0.0, and +0.0 + -0.0 = +0.0), and so does
    a room whose matrix is all -0.0 (no wired entry).  Only these two cases are asserted: both are free of underflow; the sign of an
    underflowed product depends on fusing."""
    table, tile = T, 0
    x = mm_noise(MM_FRAMES, table[-1], 95)
    mats = X.random_mats(table, 96)
    for r in (ROOM33, ROOM256):
        c0, n = X.rooms(table)[r]
        x[:, c0:c0 + n] = F(-0.0)
    c32, n32 = X.rooms(table)[3]
    mats[3][:] = F(-0.0)
    assert np.signbit(x[:, table[ROOM33]:]).all() and np.signbit(mats[3]).all()
    got = mm_run(dspfx, torch_cuda, table, tile, mats, x, True)
    assert (bits(got[:, table[ROOM33]:]) == 0).all(), "samples of -0.0"
    assert (bits(got[:, c32:c32 + n32]) == 0).all(), "a matrix of -0.0"
    assert (got[:, 3:c32] != 0).mean() > 0.9 and np.isfinite(got).all()


@pytest.mark.parametrize("layout", ["frame_major", "tile64"])
def test_fresh_mixmatrix_and_returns_agree_on_poison(dspfx, torch_cuda, layout):
    """The fresh matrix and MixGroups.returns are documented as the same thing.  In the rooms of 2, 33 and 256 one channel is +inf
    at frame 3 and -inf at frame 20, and another is NaN at frame 10: the infinite channel itself is NaN in both banks (the matrix
    forms 0.0 * inf, returns form inf - inf), its room-mates are +-inf, frame 10 is NaN for the whole room, and both banks give
    the same isnan, isposinf and isneginf arrays -- which are classify's of the mix-minus matrices."""
    torch = torch_cuda
    table, tile = MM_LAYOUTS[layout]
    n_ch = table[-1]
    x = mm_noise(MM_FRAMES, n_ch, 97)
    infs, nans = [], []
    for r in (1, ROOM33, ROOM256):
        c0, n = X.rooms(table)[r]
        infs.append(c0)
        nans.append(c0 + n - 1)
    x[3, infs], x[20, infs], x[10, nans] = np.inf, -np.inf, np.nan
    dx = MMT.device_block(dspfx, torch, x, tile)
    mm = MMT.bank(dspfx, table, tile, MM_FRAMES, True)
    mg = dspfx.MixGroups(n_ch, group_start=table, tile_channels=tile, max_frames=MM_FRAMES)
    try:
        out = MMT.fresh_out(torch, x.size)
        mm.run(dx, MM_FRAMES, out=out)
        ret = mg.returns(dx, MM_FRAMES)
        torch.cuda.synchronize()
        got = MMT.read_out(dspfx, out, MM_FRAMES, n_ch, tile)
        want = dspfx.from_layout(ret.cpu().numpy(), MM_FRAMES, n_ch, tile)
    finally:
        mm.close()
        mg.close()
    cls = X.classify(x, table, X.mix_minus(table), True)
    for name, fn in (("nan", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        assert np.array_equal(fn(got), cls == name), ("matrix", name, np.argwhere(fn(got) != (cls == name))[:5])
        assert np.array_equal(fn(want), cls == name), ("returns", name, np.argwhere(fn(want) != (cls == name))[:5])
    assert np.isnan(got[3, infs]).all() and np.isnan(got[20, infs]).all() and np.isnan(want[3, infs]).all()
    mates = [c + 1 for c in infs]
    assert np.isposinf(got[3, mates]).all() and np.isneginf(got[20, mates]).all() and np.isposinf(want[3, mates]).all()
    assert np.isnan(got[10, nans]).all() and np.isnan(want[10, nans]).all()
    assert set(np.unique(cls)) == set(X.CLASSES)


# =================================================================================================================================
# E. mix groups
# =================================================================================================================================
MG_N, MG_FRAMES = GROUPS[-1], 17


def mg_all(dspfx, torch, x, tile, gain=None, normalise=True, table=GROUPS):
    """-> (buses of run [F][G], buses of returns [F][G], returns [F][N] frame-major), all on the host"""
    nf, n = x.shape
    mg = dspfx.MixGroups(n, group_start=table, tile_channels=tile, max_frames=nf, normalise=normalise)
    try:
        if gain is not None:
            mg.set_gains(gain)
        dx = torch.from_numpy(dspfx.to_layout(x, tile).reshape(-1).copy()).cuda()
        b_run = mg.run(dx, nf, out=torch.full((nf, mg.groups), float("nan"), dtype=torch.float32, device="cuda"))
        b_ret = torch.full((nf, mg.groups), float("nan"), dtype=torch.float32, device="cuda")
        out = mg.returns(dx, nf, out=torch.full_like(dx, float("nan")), buses=b_ret)
        torch.cuda.synchronize()
        return b_run.cpu().numpy(), b_ret.cpu().numpy(), dspfx.from_layout(out.cpu().numpy(), nf, n, tile)
    finally:
        mg.close()


@pytest.mark.parametrize("tile", [0, 256])
def test_mixgroups_exact_on_subnormals(dspfx, torch_cuda, tile):
    """Samples k * 2^-149 with |k| <= 64 under integer faders 1 .. 4, raw sums: every term and every partial sum is an integer
    below 699 * 64 * 4 < 2^24 times 2^-149, exact in f32 in any order, so buses and returns are the integer sums times 2^-149 bit
    for bit.  A multiply, an addition, a lane exchange or a subtraction that flushes subnormals gives zeros instead."""
    rng = np.random.default_rng(101)
    k = rng.integers(-64, 65, (MG_FRAMES, MG_N))
    g = rng.integers(1, 5, MG_N)
    x = np.ldexp(k.astype(np.float64), -149).astype(F)
    t = k * g[None, :]
    gs = GROUPS
    sums = np.stack([t[:, a:b].sum(axis=1) for a, b in zip(gs[:-1], gs[1:])], axis=1)
    assert max(np.abs(t[:, a:b]).sum(axis=1).max() for a, b in zip(gs[:-1], gs[1:])) < 1 << 24
    grp = M.group_of(gs, MG_N)
    others = sums[:, grp] - t
    others[:, np.diff(gs)[grp] == 1] = 0
    want_bus = np.ldexp(sums.astype(np.float64), -149).astype(F)
    want_ret = np.ldexp(others.astype(np.float64), -149).astype(F)
    assert is_subnormal(x[x != 0]).all() and is_subnormal(want_bus).mean() > 0.5 and is_subnormal(want_ret).mean() > 0.9
    b_run, b_ret, ret = mg_all(dspfx, torch_cuda, x, tile, g.astype(F), normalise=False)
    assert (bits(b_run) == bits(want_bus)).all(), np.argwhere(bits(b_run) != bits(want_bus))[:5]
    assert (bits(b_ret) == bits(want_bus)).all(), np.argwhere(bits(b_ret) != bits(want_bus))[:5]
    assert (bits(ret) == bits(want_ret)).all(), np.argwhere(bits(ret) != bits(want_ret))[:5]


ZERO_GROUPS = [0, 2, 4, 5, 6, 8, 10, 11]     # [0,1) one; [2,40), [40,100) and [100,129) inside a span; [129,300) cut by a span boundary;
                                             # [301,1000) 699 channels over three spans; [1023,1024) one; [1024,1500) from a span boundary on


@pytest.mark.parametrize("normalise", [True, False], ids=["normalise", "raw"])
@pytest.mark.parametrize("case", ["minus_zero_samples", "negative_faders"])
@pytest.mark.parametrize("tile", [0, 256])
def test_mixgroups_a_zero_bus_is_plus_zero(dspfx, torch_cuda, tile, case, normalise):
    """The reference's collect_and_average starts from +0.0 and adds pipe by pipe, so a group whose terms are all -0.0 -- samples
    of -0.0, or silence through a fader of -1.0 -- gives a bus of +0.0 (test_edge_banks_cpu shows it, and that a tree gives
    -0.0).  The bank adds in a tree and then adds +0.0 to the finished sum: the bus is +0.0, and so is every return (+0.0 - -0.0).
    Groups of one, inside one span, cut by a span boundary and of more than 256 channels, among noisy neighbours; and a table of
    whole spans, whose sums pass through a reduce level of one piece.  Without the added +0.0 every one of these buses is
    0x80000000."""
    x = np.random.default_rng(102).uniform(-1.0, 1.0, (MG_FRAMES, MG_N)).astype(F)
    gain = np.random.default_rng(103).uniform(0.5, 2.0, MG_N).astype(F)
    zero = np.zeros(MG_N, bool)
    for g in ZERO_GROUPS:
        zero[GROUPS[g]:GROUPS[g + 1]] = True
    if case == "minus_zero_samples":
        x[:, zero] = F(-0.0)
    else:
        x[:, zero] = F(0.0)
        gain[zero] = F(-1.0)
    assert np.signbit(R.terms(x, gain)[:, zero]).all() and (R.terms(x, gain)[:, zero] == 0).all()
    b_run, b_ret, ret = mg_all(dspfx, torch_cuda, x, tile, gain, normalise)
    for name, b in (("run", b_run), ("returns", b_ret)):
        assert (bits(b[:, ZERO_GROUPS]) == 0).all(), (name, np.argwhere(bits(b[:, ZERO_GROUPS]) != 0)[:5])
        noisy = [g for g in range(len(GROUPS) - 1) if g not in ZERO_GROUPS and GROUPS[g + 1] > GROUPS[g]]
        assert (b[:, noisy] != 0).all() and np.isfinite(b).all()
    assert (bits(ret[:, zero]) == 0).all(), np.argwhere(bits(ret[:, zero]) != 0)[:5]
    # whole spans: every group is one span, its sum one piece
    uniform = list(range(0, MG_N + 1, 256))
    if case == "minus_zero_samples":
        ux, ugain = np.full_like(x, F(-0.0)), None
    else:
        ux, ugain = np.zeros_like(x), np.full(MG_N, F(-1.0))
    u_run, u_ret, uret = mg_all(dspfx, torch_cuda, ux, tile, ugain, normalise, uniform)
    assert (bits(u_run) == 0).all() and (bits(u_ret) == 0).all() and (bits(uret) == 0).all()


@pytest.mark.parametrize("group", [4, 6, 8, 11])
@pytest.mark.parametrize("tile", [0, 256])
def test_mixgroups_mixed_infinities(dspfx, torch_cuda, tile, group):
    """One group holds +inf in its first channel and -inf in its last at frame 5, and +inf alone at frame 9: the bus is NaN at
    frame 5 and +inf at frame 9, in run and in returns' buses alike; the returns follow the definition (mixreturns_ref.returns_bits
    from those sums) in isnan, isposinf and isneginf pattern -- at frame 9 the infinite channel hears inf - inf = NaN, the others
    +inf; every other group keeps the bits of the clean run, buses and returns.  Groups inside a span, cut by a span boundary,
    over three spans and from a span boundary on."""
    clean = np.random.default_rng(104).uniform(-1.0, 1.0, (MG_FRAMES, MG_N)).astype(F)
    gain = np.random.default_rng(105).uniform(0.5, 2.0, MG_N).astype(F)
    a, b = GROUPS[group], GROUPS[group + 1]
    x = clean.copy()
    x[5, a], x[5, b - 1], x[9, a] = np.inf, -np.inf, np.inf
    c_run, c_ret, cret = mg_all(dspfx, torch_cuda, clean, tile, gain)
    b_run, b_ret, ret = mg_all(dspfx, torch_cuda, x, tile, gain)
    S_raw, _, _ = mg_all(dspfx, torch_cuda, x, tile, gain, normalise=False)
    for name, bus in (("run", b_run), ("returns", b_ret), ("raw", S_raw)):
        col = bus[:, group]
        assert np.isnan(col[5]) and np.isposinf(col[9]) and np.isfinite(np.delete(col, [5, 9])).all(), (name, col)
    other_groups = [g for g in range(len(GROUPS) - 1) if g != group]
    assert (bits(b_run[:, other_groups]) == bits(c_run[:, other_groups])).all() and np.isfinite(c_run).all()
    assert (bits(b_ret[:, other_groups]) == bits(c_ret[:, other_groups])).all()
    want = M.returns_bits(S_raw, x, GROUPS, gain, True)
    for fn in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(fn(ret), fn(want)), (fn.__name__, np.argwhere(fn(ret) != fn(want))[:5])
    assert np.isnan(ret[5, a:b]).all() and np.isnan(ret[9, a]) and np.isposinf(ret[9, a + 1:b]).all()
    outside = np.r_[0:a, b:MG_N]
    assert (bits(ret[:, outside]) == bits(cret[:, outside])).all() and np.isfinite(cret).all()
    rows = np.delete(np.arange(MG_FRAMES), [5, 9])
    assert (bits(ret[rows]) == bits(cret[rows])).all()
