"""The channel-strip bank without a GPU: dspfx_strips_coeffs (a pure host function) against the oracle's regenerate_filter, the
numpy restatement the GPU tests lean on (strips_ref) against oracle.chain_run bit for bit, the exports, and the argument
checks that need no device."""
import ctypes as C

import numpy as np
import pytest

import numpy_model as NM
import oracle as O
import strips_ref as S

INVALID = -1
NAMES = ("dspfx_strips_create", "dspfx_strips_destroy", "dspfx_strips_last_error", "dspfx_strips_run", "dspfx_strips_set_gain",
         "dspfx_strips_set_band", "dspfx_strips_reset", "dspfx_strips_present", "dspfx_strips_coeffs")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_entry_points_exist(dspfx):
    L = dspfx.lib()
    for name in NAMES:
        assert name in dspfx.EXPORTS and hasattr(L, name), name
    assert dspfx.STRIPS_MAX_BANDS == 8
    for m in ("run", "set_gain", "set_band", "present", "reset", "close"):
        assert hasattr(dspfx.ChannelStrips, m), m


def _raw_cases():
    rng = np.random.default_rng(11)
    cases = [rng.uniform(-10.0, 10.0, 6).astype(np.float32) for _ in range(200)]
    cases.append(np.asarray([1, -0.24, 0, 0.758, 0, 0], np.float32))          # the reference defaults, biquad.rs:18-41
    cases.append(np.asarray([2, -0.24, 0.5, 0.758, 0.1, -0.3], np.float32))   # a0 = 2
    cases.append(np.asarray([-1.5, 0.9, -0.2, 0.3, 0.7, 0.1], np.float32))    # a negative a0
    return cases + list(S.stable_raw6(rng, 20))


def test_coeffs_equal_the_oracles_regenerate_filter(dspfx):
    """The oracle's biquad_regenerate is reachable through a node: O.Node(BIQUAD, raw) runs it.  Its numpy twin
    (numpy_model.Biquad) shows the five coefficients; the C node shows them through what it computes."""
    x = S.noise(np.random.default_rng(3), 6, 1)[:, 0]           # short: a random raw filter may be unstable
    for raw in _raw_cases():
        got = dspfx.strips_coeffs(raw)
        twin = NM.Biquad(*[np.float32(q) for q in raw])
        want = np.asarray([twin.a1, twin.a2, twin.b0, twin.b1, twin.b2], np.float32)
        assert np.array_equal(bits(got), bits(want)), raw
        assert np.array_equal(bits(got), bits(S.coeffs(raw))), raw
        # the C oracle's node, built from the raw sliders, and a filter run on the five coefficients the product makes
        ref = O.chain_run([O.Node(O.BIQUAD, [float(q) for q in raw])], x, 0)
        s = S.Strips(1, 1)
        s.mask[:] = 2
        s.coef[0, :, 0] = got
        assert np.array_equal(bits(s.run(x[:, None])[:, 0]), bits(ref)), raw


def test_coeffs_with_a_zero_a0_are_the_references_infinities(dspfx):
    got = dspfx.strips_coeffs([0, 1, -1, 0, 2, 0])
    assert np.isposinf(got[0]) and np.isneginf(got[1]) and np.isnan(got[2]) and np.isposinf(got[3]) and np.isnan(got[4])
    assert dspfx.lib().dspfx_strips_coeffs(None, None) == INVALID


def _oracle_channel(mask, level, raws, flags, blocks, restore=None):
    """one channel through the oracle, block by block; restore = (block index, band, raw6): the band's node is replaced by a
    fresh one before that block (a slider change: new coefficients, zero state)"""
    nodes = S.oracle_nodes(O, mask, level, raws)
    outs = []
    for i, x in enumerate(blocks):
        if restore is not None and restore[0] == i:
            raws = list(raws)
            raws[restore[1]] = restore[2]
            fresh = S.oracle_nodes(O, mask, level, raws)
            idx = bin(mask & ((1 << (1 + restore[1])) - 1)).count("1")        # the band's place among the present nodes
            nodes[idx] = fresh[idx]
        outs.append(O.chain_run(nodes, x, flags))
    return np.concatenate(outs)


@pytest.mark.parametrize("flags", [0, 1, 3])
def test_restatement_equals_the_oracle_bit_for_bit(flags):
    K, nf, nblocks = 3, 128, 3
    pats = S.patterns(K)
    assert len(pats) == 5
    rng = np.random.default_rng(100 + flags)
    n = 2 * len(pats)                                            # every pattern twice: one channel of each gets the mid-stream store
    masks = np.asarray(pats * 2, np.uint32)
    level = rng.uniform(0.0, 4.0, n).astype(np.float32)
    raw = np.stack([S.stable_raw6(rng, n) for _ in range(K)])    # [band][channel][6]
    x = S.noise(rng, nf * nblocks, n)
    s = S.Strips(n, K, flags)
    for c in range(n):
        if masks[c] & 1:
            s.set_gain(level[c:c + 1], c)
        for b in range(K):
            if masks[c] & (1 << (1 + b)):
                s.set_band(b, raw[b, c:c + 1], c)
    assert np.array_equal(s.mask, masks)
    # before block 2 (index 1): band 1 is stored anew on the second copy of the patterns that carry it
    band, new = 1, S.stable_raw6(rng, n)
    stored = [c for c in range(len(pats), n) if masks[c] & (1 << (1 + band))]
    assert stored
    got = []
    for i in range(nblocks):
        if i == 1:
            for c in stored:
                s.set_band(band, new[c:c + 1], c)
        got.append(s.run(x[i * nf:(i + 1) * nf]))
    got = np.concatenate(got)
    for c in range(n):
        blocks = [x[i * nf:(i + 1) * nf, c] for i in range(nblocks)]
        ref = _oracle_channel(int(masks[c]), level[c], [raw[b, c] for b in range(K)], flags, blocks,
                              (1, band, new[c]) if c in stored else None)
        assert np.array_equal(bits(got[:, c]), bits(ref)), (flags, c, bin(masks[c]))
    assert np.array_equal(bits(got[:, 0]), bits(x[:, 0]))        # no node: the input's bits, hops or not


def test_restatement_drop_and_reset():
    rng = np.random.default_rng(5)
    x = S.noise(rng, 64, 4)
    s = S.Strips(4, 2, 3)
    s.set_gain(2.0)
    s.set_band(1, [1, -0.5, 0.1, 0.3, 0.2, 0.1], first=1, count=2)
    assert list(s.mask) == [1, 5, 5, 1]
    a = s.run(x)
    s.reset()
    assert np.array_equal(bits(s.run(x)), bits(a))
    s.set_band(1, None, first=1, count=1)
    s.set_gain(None, first=3)
    assert list(s.mask) == [1, 1, 5, 0]
    b = s.run(x)
    assert np.array_equal(bits(b[:, 3]), bits(x[:, 3]))


@pytest.mark.parametrize("kw,word", [
    (dict(bands=0), "bands"),
    (dict(bands=9), "bands"),
    (dict(link_flags=4), "link flag"),
    (dict(link_flags=8), "link flag"),
    (dict(tile_channels=48), "power of two"),
    (dict(tile_channels=64), "divides"),
    (dict(channels=0), "n_channels"),
    (dict(max_frames=0), "max_frames"),
])
def test_create_rejects_a_bad_descriptor_before_any_device_work(dspfx, kw, word):
    args = dict(channels=1000, bands=2, tile_channels=0, max_frames=128, link_flags=0)
    args.update(kw)
    with pytest.raises(dspfx.DspfxError) as e:
        dspfx.ChannelStrips(**args)
    assert e.value.status == INVALID and word in str(e.value), str(e.value)


def test_null_arguments_are_invalid(dspfx):
    L = dspfx.lib()
    h = C.c_void_p()
    assert L.dspfx_strips_create(None, C.byref(h)) == INVALID
    assert L.dspfx_strips_last_error(None)
    assert L.dspfx_strips_destroy(None) == INVALID
    assert L.dspfx_strips_run(None, None, None, 128, None) == INVALID
    assert L.dspfx_strips_set_gain(None, None, 0, 0) == INVALID
    assert L.dspfx_strips_set_band(None, 0, None, 0, 0) == INVALID
    assert L.dspfx_strips_reset(None) == INVALID
    assert L.dspfx_strips_present(None, None, 0, 0) == INVALID
