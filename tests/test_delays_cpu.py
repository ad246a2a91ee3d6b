"""The channel-delay bank without a GPU: the numpy restatement the GPU tests lean on (delays_ref) against the oracle's Reverb
(oracle.chain_run) bit for bit, stores in mid-stream included; dspfx_delays_plan (a pure host function) against the formula; the
exports, and the argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

import delays_ref as R
import oracle as O

INVALID = -1
NF = 128
NAMES = ("dspfx_delays_plan", "dspfx_delays_create", "dspfx_delays_destroy", "dspfx_delays_last_error", "dspfx_delays_run",
         "dspfx_delays_set_delay", "dspfx_delays_reset", "dspfx_delays_present", "dspfx_delays_lengths")
DECAYS = [0.5, -1.0, 1.0, np.inf]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def signal(rng, nf, n):
    """noise with runs of -0.0 and +0.0 in it, the first frames of every channel among them (the taps are still zeros there)"""
    x = R.noise(rng, nf, n)
    x[:5] = np.float32(-0.0)
    x[5:8] = np.float32(0.0)
    x[rng.integers(0, nf, 40), rng.integers(0, n, 40)] = np.float32(-0.0)
    return x


def test_the_entry_points_exist(dspfx):
    L = dspfx.lib()
    for name in NAMES:
        assert name in dspfx.EXPORTS and hasattr(L, name), name
    for m in ("run", "set_delay", "present", "lengths", "reset", "close"):
        assert hasattr(dspfx.ChannelDelays, m), m


def test_delay_len_restated():
    for s in (0.0, -1.0, np.nan, np.inf, 0.001, 0.0026, 0.0027, 129.5 / 48000, 0.02, 0.03, 0.25, 0.5, 1.0, 1e5, 1e6):
        for pr in (False, True):
            assert R.delay_len(s, pr) == O.delay_len(s, pr), (s, pr)
    for d in R.PATTERN_LENGTHS[1:]:
        assert O.delay_len(R.seconds_for(d)) == d


@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("page_round,lengths,max_seconds", [(False, [128, 129, 160, 300, 960], 0.02), (True, [1024, 2048], 0.03)])
def test_restatement_equals_the_oracle_bit_for_bit(flags, page_round, lengths, max_seconds):
    """every length under every decay, 12 blocks of 128: every ring wraps, the odd lengths leave the block grid"""
    rng = np.random.default_rng(7 + flags)
    combos = [(d, k) for d in lengths for k in DECAYS]
    n = len(combos) + 1                                          # and one channel without a node
    x = signal(rng, 12 * NF, n)
    ref = R.Delays(n, max_seconds, flags, page_round)
    assert ref.cap == O.delay_len(max_seconds, page_round)
    secs = [(d - 0.5) / 48000.0 if page_round else R.seconds_for(d) for d, _ in combos]
    assert ref.set_delay(np.asarray(secs, np.float32), np.asarray([k for _, k in combos], np.float32))
    assert list(ref.lengths()) == [d for d, _ in combos] + [0]
    got = ref.run_blocks(x)
    for c, (d, k) in enumerate(combos):
        want = O.chain_run([O.Node(O.REVERB, [k, float(np.float32(secs[c]))], mode=int(page_round), delay_len=d)], x[:, c], flags)
        assert np.array_equal(bits(got[:, c]), bits(want)), (flags, d, k)
    assert np.array_equal(bits(got[:, n - 1]), bits(x[:, n - 1])), "no node: the input's bits, hop or not"


@pytest.mark.parametrize("flags", [0, 3])
def test_mid_stream_stores_equal_the_oracles_slider_changes(flags):
    """decay alone (Node.set_param(0, ..)) gives a new zero ring and so cuts the tail; seconds to a shorter and to a longer ring"""
    rng = np.random.default_rng(17 + flags)
    d0 = 300
    cases = [("decay", 0, 0.25, d0), ("shorter", 1, R.seconds_for(160), 160), ("longer", 1, R.seconds_for(960), 960)]
    n = len(cases) + 1                                           # the last channel gets no store: its tail goes on
    x = signal(rng, 8 * NF, n)
    x[4 * NF:] = 0                                               # silence after the store: what comes out is the ring's tail
    ref = R.Delays(n, 0.02, flags)
    assert ref.set_delay(R.seconds_for(d0), 0.9)
    a = ref.run_blocks(x[:4 * NF])
    for c, (name, idx, val, _) in enumerate(cases):
        assert ref.set_delay(seconds=val if idx == 1 else None, decay=val if idx == 0 else None, first_channel=c, count=1)
    assert list(ref.lengths()) == [c[3] for c in cases] + [d0]
    got = np.concatenate([a, ref.run_blocks(x[4 * NF:])])
    for c in range(n):
        node = O.Node(O.REVERB, [0.9, float(R.seconds_for(d0))], delay_len=d0)
        first = O.chain_run([node], x[:4 * NF, c], flags)
        if c < len(cases):
            node.set_param(cases[c][1], float(np.float32(cases[c][2])))
        want = np.concatenate([first, O.chain_run([node], x[4 * NF:, c], flags)])
        assert np.array_equal(bits(got[:, c]), bits(want)), (flags, c)
    assert not got[4 * NF:, :len(cases)].any(), "a store of any slider cuts the tail"
    assert got[4 * NF:, n - 1].any()


def test_restatement_drop_refusal_and_reset():
    rng = np.random.default_rng(5)
    x = R.noise(rng, 2 * NF, 4)
    ref = R.Delays(4, 0.02, 0)
    assert ref.set_delay(0.005, 0.5, first_channel=1, count=2)
    assert list(ref.lengths()) == [0, 240, 240, 0] and list(ref.present()) == [0, 1, 1, 0]
    a = ref.run_blocks(x)
    assert np.array_equal(bits(a[:, [0, 3]]), bits(x[:, [0, 3]]))
    ref.reset()
    assert np.array_equal(bits(ref.run_blocks(x)), bits(a))
    assert not ref.set_delay(0.5, None, first_channel=1, count=1), "24000 frames do not fit a ring of 960"
    assert not ref.set_delay(None, 0.1, first_channel=0, count=1), "an omitted seconds is the default 0.5 on a channel never stored"
    assert not ref.set_delay(0.01, 0.1, first_channel=3, count=2)
    assert list(ref.lengths()) == [0, 240, 240, 0]
    assert ref.set_delay(None, None, first_channel=1, count=1)
    assert list(ref.lengths()) == [0, 0, 240, 0]


def test_plan_is_the_formula(dspfx):
    for n, s, pr in [(1, 0.5, False), (70, 0.02, False), (256, 0.03, True), (1 << 20, 0.02, False), (1 << 20, 0.5, True), (3, 0.0, False),
                     (3, float("nan"), True), (0xFFFFFF00, 1.0, False)]:
        cap, nbytes = dspfx.delays_plan(n, s, pr)
        assert cap == dspfx.delay_len(s, pr) == O.delay_len(s, pr), (n, s, pr)
        assert nbytes == n * cap * 4
    assert dspfx.delays_plan(1 << 20, 0.02) == (960, 3840 << 20)
    assert dspfx.delays_plan(8, (2 ** 31 - 64) / 48000.0)[0] <= 2 ** 31


@pytest.mark.parametrize("args,word", [
    ((8, 1e5), "2^31"),                                          # 4.8e9 frames saturate `as usize` at 2^32 - 1
    ((8, 46000.0), "2^31"),                                      # 2 208 000 000 frames
    ((8, 45000.0, True), "2^31"),                                # 2 160 000 000 frames, page-rounded
    ((0, 0.5), "n_channels"),
    ((1 << 32, 0.5), "n_channels"),
])
def test_plan_refusals(dspfx, args, word):
    with pytest.raises(dspfx.DspfxError) as e:
        dspfx.delays_plan(*args)
    assert e.value.status == INVALID and word in str(e.value) and "delays" in str(e.value), str(e.value)


@pytest.mark.parametrize("kw,word", [
    (dict(max_seconds=46000.0), "2^31"),
    (dict(tile_channels=48), "power of two"),
    (dict(tile_channels=64), "divides"),
    (dict(link_flags=4), "link flag"),
    (dict(channels=0), "n_channels"),
    (dict(max_frames=0), "max_frames"),
])
def test_create_rejects_a_bad_descriptor_before_any_device_work(dspfx, kw, word):
    args = dict(channels=1000, max_seconds=0.02, tile_channels=0, max_frames=128, link_flags=0)
    args.update(kw)
    with pytest.raises(dspfx.DspfxError) as e:
        dspfx.ChannelDelays(**args)
    assert e.value.status == INVALID and word in str(e.value), str(e.value)


def test_null_arguments_are_invalid(dspfx):
    L = dspfx.lib()
    h = C.c_void_p()
    assert L.dspfx_delays_create(None, C.byref(h)) == INVALID
    assert L.dspfx_delays_last_error(None)
    assert L.dspfx_delays_destroy(None) == INVALID
    assert L.dspfx_delays_run(None, None, None, 128, None) == INVALID
    assert L.dspfx_delays_set_delay(None, None, None, 0, 0) == INVALID
    assert L.dspfx_delays_reset(None) == INVALID
    assert L.dspfx_delays_present(None, None, 0, 0) == INVALID
    assert L.dspfx_delays_lengths(None, None, 0, 0) == INVALID
    assert L.dspfx_delays_plan(8, 0.5, 0, None, None) == 0
