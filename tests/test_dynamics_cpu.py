"""The channel-dynamics bank without a GPU: the numpy restatement the GPU tests lean on (dynamics_ref) against the oracle's Envelope
node (oracle.chain_run) bit for bit -- on the key when there is one, and across a slider store in mid-stream -- and against the
oracle's Gain node below the threshold; dspfx_dynamics_gain and dspfx_dynamics_plan (pure host functions) against the restatement
and the formula; the brick-wall bound on the restatement; the exports, and the argument checks that need no device.  A store's
own checks need a bank and so a device: here the restatement refuses them, tests/test_dynamics_gpu.py holds the bank to that."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dynamics_ref as R
import edge_values as E
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dspfx.h")).read()
INVALID = -1
NF = 128
F = np.float32
NAMES = ("dspfx_dynamics_plan", "dspfx_dynamics_gain", "dspfx_dynamics_create", "dspfx_dynamics_destroy", "dspfx_dynamics_last_error",
         "dspfx_dynamics_run", "dspfx_dynamics_set", "dspfx_dynamics_drop", "dspfx_dynamics_reset", "dspfx_dynamics_present",
         "dspfx_dynamics_views")
ATTACKS, RELEASES = [0, 1, 48, 1000], [0, 1, 1000, 24000]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def noise(rng, nf, n):
    return rng.uniform(-1.0, 1.0, (nf, n)).astype(F)


def test_the_entry_points_exist_and_the_abi_version_is_still_2(dspfx):
    L = dspfx.lib()
    for name in NAMES:
        assert name in dspfx.EXPORTS and hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, HDR), name
    for m in ("run", "set", "drop", "reset", "present", "levels", "reductions", "close"):
        assert hasattr(dspfx.ChannelDynamics, m), m
    assert callable(dspfx.dynamics_gain) and callable(dspfx.dynamics_plan)
    assert dspfx.ABI_VERSION == 2 and L.dspfx_abi_version() == 2 and "#define DSPFX_ABI_VERSION 2" in HDR


@pytest.mark.parametrize("keyed", [False, True])
def test_restatement_envelope_equals_the_oracle_bit_for_bit(keyed):
    """every attack under every release, 6 blocks of 128, and after the third a slider store, which keeps env: the oracle's slider
    change sets only the gain.  With a key the envelope is the key's, whatever the block holds"""
    rng = np.random.default_rng(3 + keyed)
    combos = [(a, r) for a in ATTACKS for r in RELEASES]
    n = len(combos)
    x = noise(rng, 6 * NF, n)
    x[NF:NF + 40] *= F(0.01)                                     # a quiet stretch: the release is heard
    x[2 * NF + 5:2 * NF + 9] = F(-0.0)
    x[5 * NF:] = 0
    block = noise(rng, 6 * NF, n) * F(3) if keyed else x         # the detector follows x either way
    ref = R.ChannelDynamics(n)
    assert ref.set(threshold=0.25, makeup=2.0, attack=np.asarray([a for a, _ in combos], F), release=np.asarray([r for _, r in combos], F))
    later = [(combos[(i + 5) % n][0], combos[(i + 3) % n][1]) for i in range(n)]
    envs, outs = [], []
    for b in range(6):
        if b == 3:
            assert ref.set(attack=np.asarray([a for a, _ in later], F), release=np.asarray([r for _, r in later], F))
        sl = slice(b * NF, (b + 1) * NF)
        outs.append(ref.run(block[sl], key=x[sl] if keyed else None))
        envs.append(ref.envs)
        assert np.array_equal(bits(ref.level), bits(ref.envs.max(axis=0))), "the level is the block's largest envelope"
    envs, outs = np.concatenate(envs), np.concatenate(outs)
    for c, (a, r) in enumerate(combos):
        node = O.Node(O.ENVELOPE, [float(a), float(r)])
        first = O.chain_run([node], x[:3 * NF, c], 0)
        node.set_param(0, float(later[c][0]))
        node.set_param(1, float(later[c][1]))
        want = np.concatenate([first, O.chain_run([node], x[3 * NF:, c], 0)])
        assert np.array_equal(bits(envs[:, c]), bits(want)), (a, r)
    # the output is the block times the gain the rule gives for that envelope
    g, q = R.gain(envs, F(0.25), F(2.0))
    assert np.array_equal(bits(outs), bits(block * g)) and (q < 1).any() and (q == 1).any()
    assert np.array_equal(bits(ref.reduction), bits(q[5 * NF:].min(axis=0)))


def test_a_channel_below_its_threshold_equals_the_oracles_gain_node():
    """q is exactly 1.0 there, and in * (mk * 1.0f) is in * mk: the bits of Engine([Gain(mk)]); with mk = 1 a copy"""
    rng = np.random.default_rng(5)
    makeups = [1.0, 0.7, 3.0, 8.0, 0.0]
    n = len(makeups) + 1
    x = noise(rng, 3 * NF, n) * F(0.2)
    x[7, :] = F(-0.0)
    ref = R.ChannelDynamics(n)
    assert ref.set(threshold=0.25, makeup=np.asarray(makeups, F), attack=48.0, release=1000.0, count=len(makeups))
    got = ref.run_blocks(x)
    for c, mk in enumerate(makeups):
        want = O.chain_run([O.Node(O.GAIN, [float(mk)])], x[:, c], 0)
        assert np.array_equal(bits(got[:, c]), bits(want)), mk
    assert np.array_equal(bits(got[:, 0]), bits(x[:, 0])), "makeup 1 below the threshold is a copy"
    assert np.array_equal(bits(got[:, n - 1]), bits(x[:, n - 1])), "no node: a copy"
    assert (ref.reduction == 1).all() and ref.level[n - 1] == 0 and (ref.level[:n - 1] > 0).all()
    assert list(ref.present()) == [1] * len(makeups) + [0]


def specials():
    vals = [v for name, (vs, _) in E.edge_classes(3.0).items() for v in vs if not isinstance(v, tuple)]
    vals += [0.001, 0.0125, 0.1, 0.25, 0.5, 0.98, 1.0, 1.5, 4.0, 1.0 / 3.0, 7.0]
    return np.asarray(vals, F)


def test_dynamics_gain_equals_the_restatement(dspfx):
    """env x threshold over the edge values (NaN, infinities, signed zeros, subnormals, the largest finite) and plain ones, under
    four makeups: the function takes what it is given, the stores are where thresholds are checked"""
    v = specials()
    assert np.isnan(v).any() and np.isinf(v).any() and E.is_subnormal(v).any() and (np.signbit(v) & (v == 0)).any()
    env, thr = np.meshgrid(v, v, indexing="ij")
    for mk in (1.0, 0.7, 3.0, 0.0):
        want_g, want_q = R.gain(env, thr, F(mk))
        got = np.asarray([[dspfx.dynamics_gain(e, t, mk) for t in v] for e in v], F)
        E.same_bits_or_nan(got[:, :, 0], want_g, None, f"gain, makeup {mk}")
        E.same_bits_or_nan(got[:, :, 1], want_q, None, f"q, makeup {mk}")
    assert dspfx.dynamics_gain(1.0, 0.25, 2.0) == (F(0.5), F(0.25)) and dspfx.dynamics_gain(0.25, 0.25, 2.0) == (F(2.0), F(1.0))
    assert dspfx.dynamics_gain(float("nan"), 0.25, 1.0)[1] == 1, "a NaN envelope compares false"
    assert dspfx.lib().dspfx_dynamics_gain(1.0, 0.5, 1.0, None) == 0.5


def test_plan_is_the_formula(dspfx):
    for n in (1, 70, 256, 1 << 20, 0xFFFFFF00):
        assert dspfx.dynamics_plan(n) == 29 * n
    for n in (0, 1 << 32, 0xFFFFFF01):
        with pytest.raises(dspfx.DspfxError) as e:
            dspfx.dynamics_plan(n)
        assert e.value.status == INVALID and "n_channels" in str(e.value) and "dynamics" in str(e.value), str(e.value)


@pytest.mark.parametrize("kw,word", [
    (dict(tile_channels=48), "power of two"),
    (dict(tile_channels=64), "divides"),
    (dict(channels=0), "n_channels"),
    (dict(channels=0xFFFFFF01), "n_channels"),
    (dict(max_frames=0), "max_frames"),
    (dict(max_frames=(1 << 20) + 1), "max_frames"),
])
def test_create_rejects_a_bad_descriptor_before_any_device_work(dspfx, kw, word):
    args = dict(channels=1000, tile_channels=0, max_frames=128)
    args.update(kw)
    with pytest.raises(dspfx.DspfxError) as e:
        dspfx.ChannelDynamics(**args)
    assert e.value.status == INVALID and word in str(e.value) and "dynamics" in str(e.value), str(e.value)


def test_null_arguments_are_invalid(dspfx):
    L = dspfx.lib()
    h = C.c_void_p()
    assert L.dspfx_dynamics_create(None, C.byref(h)) == INVALID
    assert L.dspfx_dynamics_last_error(None)
    assert L.dspfx_dynamics_destroy(None) == INVALID
    assert L.dspfx_dynamics_run(None, None, None, None, 128, None) == INVALID
    assert L.dspfx_dynamics_set(None, None, None, None, None, 0, 0) == INVALID
    assert L.dspfx_dynamics_drop(None, 0, 0) == INVALID
    assert L.dspfx_dynamics_reset(None, 0, 0) == INVALID
    assert L.dspfx_dynamics_present(None, None, 0, 0) == INVALID
    assert L.dspfx_dynamics_views(None, None, None) == INVALID
    assert L.dspfx_dynamics_plan(8, None) == 0


def test_restatement_stores_refusals_drop_and_reset():
    rng = np.random.default_rng(6)
    x = noise(rng, 2 * NF, 4)
    ref = R.ChannelDynamics(4)
    assert ref.set(threshold=0.25, release=1000.0, first_channel=1, count=2)
    assert list(ref.present()) == [0, 1, 1, 0] and list(ref.mk) == [1, 1, 1, 1] and list(ref.ga) == [0, 0, 0, 0]
    a = ref.run_blocks(x)
    assert np.array_equal(bits(a[:, [0, 3]]), bits(x[:, [0, 3]])) and (np.abs(a[:, 1:3]) <= 0.25 * (1 + 2.0 ** -22)).all()
    ref.reset()
    assert np.array_equal(bits(ref.run_blocks(x)), bits(a)), "a reset starts the same stream again"
    before = [t.copy() for t in (ref.thr, ref.mk, ref.ga, ref.gr, ref.on, ref.env)]
    for kw in (dict(threshold=float("nan")), dict(threshold=-0.5), dict(threshold=-0.0), dict(threshold=[0.5, -1.0]),
               dict(makeup=float("nan")), dict(makeup=float("inf")), dict(makeup=-1.0), dict(makeup=-0.0),
               dict(threshold=0.5, first_channel=3, count=2), dict(threshold=0.5, first_channel=5, count=0)):
        assert not ref.set(**kw), kw
    assert not ref.drop(4, 1) and not ref.reset(2, 3)
    assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(before, (ref.thr, ref.mk, ref.ga, ref.gr, ref.on, ref.env)))
    assert ref.set(threshold=float("inf"), first_channel=0, count=1) and ref.set(threshold=0.0, makeup=0.0, first_channel=3, count=1)
    assert ref.set(makeup=2.0, first_channel=1, count=1) and ref.thr[1] == F(0.25) and ref.gr[1] == ref.gr[2], "a partial store keeps the rest"
    assert ref.drop(1, 1) and list(ref.present()) == [1, 0, 1, 1] and ref.env[1] == 0 and ref.env[2] != 0
    assert ref.set(first_channel=1, count=1) and ref.thr[1] == 1 and ref.mk[1] == 1 and ref.gr[1] == 0, "after a drop: the defaults"


GRID = [(amp, thr, mk, rel) for amp in (1e-3, 0.05, 1.0, 4.0) for thr in (0.001, 0.25, 0.5, 1.0) for mk in (0.7, 1.0, 3.0)
        for rel in (0, 1, 48, 1000, 24000)]


def test_brick_wall_bound_on_the_restatement():
    """attack 0, no key, finite input: env >= |x| on every frame, so |out| <= thr * mk * (1 + 2^-24)^3, three roundings (the
    division and the two multiplications).  Every cell of the grid is a channel of its own: noise of four amplitudes x four
    thresholds x three makeups x five releases, 8 blocks of 128"""
    rng = np.random.default_rng(9)
    amp, thr, mk, rel = (np.asarray(col) for col in zip(*GRID))
    n = len(GRID)
    x = (rng.uniform(-1.0, 1.0, (8 * NF, n)) * amp).astype(F)
    ref = R.ChannelDynamics(n)
    assert ref.set(threshold=thr.astype(F), makeup=mk.astype(F), attack=0.0, release=rel.astype(F))
    y, envs = [], []
    for b in range(8):
        y.append(ref.run(x[b * NF:(b + 1) * NF]))
        envs.append(ref.envs)
    y, envs = np.concatenate(y), np.concatenate(envs)
    assert (envs >= np.abs(x)).all(), "with attack 0 the envelope never lies below the sample's magnitude"
    bound = thr.astype(F).astype(np.float64) * mk.astype(F).astype(np.float64) * (1.0 + 2.0 ** -24) ** 3
    worst = (np.abs(y.astype(np.float64)) / bound).max(axis=0)
    print("brick wall: worst |out| / (thr * mk) - 1 = %.3f x 2^-24" % ((worst.max() * (1.0 + 2.0 ** -24) ** 3 - 1) * 2.0 ** 24))
    assert (worst <= 1.0).all(), [GRID[c] for c in np.flatnonzero(worst > 1.0)]
    loud = amp * 0.9 > thr
    assert (np.abs(y[:, loud]).max(axis=0) >= (thr * mk * 0.99)[loud]).all(), "the wall is reached, not undershot"
    # attack above 0: no such bound -- the envelope lags, the first samples overshoot
    lag = R.ChannelDynamics(1)
    assert lag.set(threshold=0.25, attack=48.0, release=24000.0)
    over = np.abs(lag.run(noise(rng, NF, 1))).max() / 0.25
    assert over > 1.5, over
