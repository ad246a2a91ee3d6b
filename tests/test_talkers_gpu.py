"""The talker bank on the GPU (dspfx_talkers_*, through the Python class): per-channel envelopes and levels, every room's loudest,
and the gate.  Everything is compared bit for bit with talkers_ref, which tests/test_talkers_cpu.py holds to the oracle's Envelope
node bit for bit.  One exception, the project's own (tests/edge_values.py): where the reference gives a NaN the bank must give a
NaN, its sign and payload are not compared -- x86 and the GPU make them differently."""
import threading

import numpy as np
import pytest

import edge_values as E
import oracle as O
import talkers_ref as R

pytestmark = pytest.mark.gpu

NF = 128
SHAPES = [(64, 0), (256, 64), (70, 0), (1, 0)]                   # vector lanes; tiled; scalar accesses and a ragged last workgroup; one channel
TWO = [(256, 64), (70, 0)]
ROOM_N, ROOM_TILE = 1280, 256
ROOM_SIZES = [1024, 1, 2, 33, 64, 65, 91]                        # 16 values per lane; one member; a wave's edge on both sides; a ragged tail
ATTACKS, RELEASES = [0, 1, 48, 1000], [0, 1, 1000, 24000]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def table(n):
    """two rooms (one when there is no room for two): a cut that is no multiple of 4"""
    return [0, n // 3, n] if n >= 3 else [0, n]


def device(dspfx, torch, x, tile):
    return torch.from_numpy(dspfx.to_layout(x, tile).reshape(-1).copy()).cuda()


def host(dspfx, t, nf, n, tile):
    return dspfx.from_layout(t.cpu().numpy(), nf, n, tile)


def pair(dspfx, n, tile, gs, top=3, seed=None):
    """a bank and its restatement; seed: every channel's detector drawn from ATTACKS x RELEASES"""
    bank, ref = dspfx.Talkers(n, group_start=gs, top=top, tile_channels=tile, max_frames=NF), R.Talkers(n, gs, top)
    if seed is not None:
        rng = np.random.default_rng(seed)
        a, r = rng.choice(ATTACKS, n).astype(np.float32), rng.choice(RELEASES, n).astype(np.float32)
        both(bank, ref, lambda b: b.set_detector(a, r))
    return bank, ref


def both(bank, ref, call):
    call(bank)
    assert call(ref) is not False


def tables_equal(torch, bank, ref, what):
    torch.cuda.synchronize()
    assert np.array_equal(bits(bank.levels().cpu().numpy()), bits(ref.level)), f"{what}: levels"
    assert np.array_equal(bank.talkers().cpu().numpy(), ref.talkers), f"{what}: talkers\n{bank.talkers().cpu().numpy()}\n{ref.talkers}"
    assert np.array_equal(bits(bank.talker_levels().cpu().numpy()), bits(ref.talker_levels)), f"{what}: talker levels"
    assert np.array_equal(bits(bank.targets().cpu().numpy()), bits(ref.target)), f"{what}: targets"


def step(dspfx, torch, bank, ref, blk, n, tile, what, inplace=False, gate=True):
    """one block through both; the output (NaN judged by isnan) and every table bit for bit"""
    dx = device(dspfx, torch, blk, tile)
    want = ref.run(blk, gate)
    got = None
    if gate:
        dy = bank.run(dx, len(blk), out=dx if inplace else torch.full_like(dx, float("nan")))
        torch.cuda.synchronize()
        got = host(dspfx, dy, len(blk), n, tile)
        E.same_bits_or_nan(got, want, None, f"{what}: output")
    else:
        out = torch.full_like(dx, float("nan"))
        assert bank.run(dx, len(blk), out=out, gate=False) is None
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), f"{what}: gate=False writes no sample"
    tables_equal(torch, bank, ref, what)
    return got


# ---- 1. envelopes, levels and the gate over several blocks -----------------------------------------------------------------
@pytest.mark.parametrize("nf,runs", [(1, 40), (37, 6), (128, 6)])
@pytest.mark.parametrize("n,tile", SHAPES)
def test_levels_tables_and_output_equal_the_restatement(dspfx, torch_cuda, n, tile, nf, runs):
    """every channel its own detector; with one-frame blocks the level is the envelope after every single frame"""
    rng = np.random.default_rng(100 + n + nf)
    bank, ref = pair(dspfx, n, tile, table(n), top=3, seed=n)
    x = R.noise(rng, runs * nf, n) * rng.choice([0.05, 1.0], (runs, 1, n)).astype(np.float32).repeat(nf, 1).reshape(runs * nf, n)
    for b in range(runs):
        got = step(dspfx, torch_cuda, bank, ref, x[b * nf:(b + 1) * nf], n, tile, f"N={n} tile={tile} nf={nf} block {b}")
        if b == 0:
            assert np.array_equal(bits(got), bits(x[:nf])), "a fresh bank's first run is a copy"
    assert n < 8 or (ref.talkers >= 0).sum() == 3 * ref.groups
    bank.close()


# ---- 2. the selection over the room shapes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("top", [1, 3, 8])
def test_selection_over_the_room_shapes(dspfx, torch_cuda, top):
    """rooms of 1024, 1, 2, 33, 64, 65 and 91; ties planted by copying a channel into a lower and a higher channel number; then a
    top per room"""
    torch = torch_cuda
    n, tile = ROOM_N, ROOM_TILE
    gs = np.r_[0, np.cumsum(ROOM_SIZES)]
    rng = np.random.default_rng(200 + top)
    bank, ref = pair(dspfx, n, tile, gs, top=top)
    both(bank, ref, lambda b: b.set_detector(48.0, 1000.0))
    x = R.noise(rng, 3 * NF, n) * np.float32(0.2)
    for src, lo, hi in [(500, 3, 1023), (100, 63, 64), (700, 15, 16), (1150, 1124, 1188), (1250, 1189, 1279), (1040, 1027, 1059)]:
        x[:, src] *= np.float32(4)                               # the loudest of its room, three times over
        x[:, lo] = x[:, hi] = x[:, src]
    for b in range(3):
        step(dspfx, torch, bank, ref, x[b * NF:(b + 1) * NF], n, tile, f"top={top} block {b}")
    t = ref.talkers
    assert t[1, 0] == 1024 and (t[1, 1:] == -1).all() and (t[2, :min(top, 2)] >= 0).all() and (t[2, 2:] == -1).all()
    if top >= 3:
        assert list(t[5, :3]) == [1124, 1150, 1188] and list(t[6, :3]) == [1189, 1250, 1279] and list(t[3, :3]) == [1027, 1040, 1059]
        assert len({float(v) for v in ref.talker_levels[5, :3]}) == 1, "the planted ties are ties"
    tops = np.asarray([8, 1, 2, 5, 1, 3, 7], np.uint8)
    both(bank, ref, lambda b: b.set_top(tops))
    both(bank, ref, lambda b: b.set_top(4, first_room=5, count=1))
    step(dspfx, torch, bank, ref, x[:NF], n, tile, "a top per room")
    assert [(r >= 0).sum() for r in ref.talkers] == [8, 1, 2, 5, 1, 4, 7]
    bank.close()


# ---- 3. the gate across a talker change ------------------------------------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("nf", [1, 37, 128, 4, 8, 9])
@pytest.mark.parametrize("n,tile", TWO)
def test_gate_across_a_talker_change(dspfx, torch_cuda, n, tile, nf, inplace):
    """loud channels move from one set to another: open stays open, shut stays shut, a ramp up, a ramp down"""
    torch = torch_cuda
    rng = np.random.default_rng(300 + n + nf)
    bank, ref = pair(dspfx, n, tile, table(n), top=2)
    quiet = R.noise(rng, 5 * nf, n) * np.float32(0.01)
    xa, xb = quiet.copy(), quiet.copy()
    first, second = [1, n // 3 + 2], [5, n // 3 + 2]             # room 0 changes its loudest, room 1 keeps it
    xa[:, first] = R.noise(rng, 5 * nf, 2)
    xb[:, second] = R.noise(rng, 5 * nf, 2)
    seen = set()
    for b, x in enumerate([xa, xa, xb, xb, xb]):
        seen |= set(zip(ref.gate.tolist(), ref.target.tolist()))
        got = step(dspfx, torch, bank, ref, x[b * nf:(b + 1) * nf], n, tile, f"N={n} nf={nf} block {b}", inplace)
        assert np.array_equal(bits(got[-1]), bits(x[(b + 1) * nf - 1] * ref.gate)), "the last frame is at the target"
    assert seen == {(1.0, 1.0), (0.0, 0.0), (0.0, 1.0), (1.0, 0.0)}
    bank.close()


@pytest.mark.parametrize("n,tile", TWO)
def test_metering_leaves_the_gate_and_writes_no_sample(dspfx, torch_cuda, n, tile):
    torch = torch_cuda
    rng = np.random.default_rng(310 + n)
    bank, ref = pair(dspfx, n, tile, table(n), top=1, seed=7)
    x = R.noise(rng, 4 * NF, n)
    step(dspfx, torch, bank, ref, x[:NF], n, tile, "gated")
    step(dspfx, torch, bank, ref, x[NF:2 * NF], n, tile, "gated again: the losers are shut")
    assert (ref.gate == 0).sum() >= n - 2
    c = 3 if ref.talkers[0, 0] != 3 else 4
    x[2 * NF:3 * NF, c] *= np.float32(50)                        # a new loudest, metered only
    gate = ref.gate.copy()
    step(dspfx, torch, bank, ref, x[2 * NF:3 * NF], n, tile, "metering", gate=False)
    assert np.array_equal(ref.gate, gate) and ref.target[c] == 1 and ref.gate[c] == 0
    got = step(dspfx, torch, bank, ref, x[3 * NF:], n, tile, "the next gated run ramps from the unchanged gate")
    assert got[0, c] != 0 and abs(got[0, c]) < abs(x[3 * NF, c]) and got[-1, c] == x[-1, c]
    bank.close()


# ---- 4. seating ------------------------------------------------------------------------------------------------------------
def test_a_random_assign_of_a_third_of_the_channels(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile, G = ROOM_N, ROOM_TILE, len(ROOM_SIZES)
    gs = np.r_[0, np.cumsum(ROOM_SIZES)]
    rng = np.random.default_rng(400)
    bank, ref = pair(dspfx, n, tile, gs, top=3, seed=40)
    x = R.noise(rng, 4 * NF, n)
    step(dspfx, torch, bank, ref, x[:NF], n, tile, "before the assign")
    ids = rng.integers(0, G, 427).astype(np.uint32)
    ids[rng.random(427) < 0.25] = dspfx.NO_ROOM
    both(bank, ref, lambda b: b.assign(ids, first_channel=400))
    for c in rng.integers(0, n, 20):                             # and single channels anywhere, out of rooms and back in
        g = int(rng.integers(1, G))
        both(bank, ref, lambda b: b.assign([dspfx.NO_ROOM], first_channel=int(c)))
        both(bank, ref, lambda b: b.assign(g, first_channel=int(c)))
    assert np.array_equal(bank.room_of(), ref.room_of()) and np.array_equal(bank.counts(), ref.counts())
    assert (bank.room_of() == dspfx.NO_ROOM).sum() > 50
    for b in range(1, 4):
        step(dspfx, torch, bank, ref, x[b * NF:(b + 1) * NF], n, tile, f"after the assign, block {b}", inplace=b == 2)
    out = ref.room_of() == dspfx.NO_ROOM
    assert not ref.target[out].any() and not np.isin(ref.talkers, np.flatnonzero(out)).any()
    # the seating is a function of room_of alone: a bank seated in one call gives the same tables
    twin = dspfx.Talkers(n, group_start=gs, top=3, tile_channels=tile, max_frames=NF)
    twin.assign(ref.room_of())
    twin.run(device(dspfx, torch, x[:NF], tile), NF, gate=False)
    solo = R.Talkers(n, gs, 3)
    assert solo.assign(ref.room_of())
    solo.run(x[:NF], gate=False)
    tables_equal(torch, twin, solo, "seated in one call")
    twin.close()
    bank.close()


def test_two_full_rooms_swap_a_member_and_a_room_over_1024_is_refused(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile = 2048 + 4, 0
    gs = [0, 1024, 2048, n]
    rng = np.random.default_rng(410)
    bank, ref = pair(dspfx, n, tile, gs, top=2)
    x = R.noise(rng, 3 * NF, n) * np.float32(0.1)
    x[:, 1023], x[:, 1024] = x[:, 1023] * np.float32(9), x[:, 1024] * np.float32(8)
    step(dspfx, torch, bank, ref, x[:NF], n, tile, "before the swap")
    assert ref.talkers[0, 0] == 1023 and ref.talkers[1, 0] == 1024
    both(bank, ref, lambda b: b.assign([1, 0], first_channel=1023))
    assert list(bank.counts()) == [1024, 1024, 4]
    step(dspfx, torch, bank, ref, x[NF:2 * NF], n, tile, "after the swap")
    assert ref.talkers[0, 0] == 1024 and ref.talkers[1, 0] == 1023
    before = bank.room_of()
    for call in (lambda: bank.assign([0], first_channel=2048), lambda: bank.assign([2, 2, 0, 0], first_channel=1025),
                 lambda: bank.assign([3], first_channel=0), lambda: bank.assign([0, 0], first_channel=n - 1),
                 lambda: bank.set_pin([3], first_channel=0), lambda: bank.set_pin([1, 1], first_channel=n - 1),
                 lambda: bank.set_top([0]), lambda: bank.set_top([9]), lambda: bank.set_top([1, 1], first_room=2),
                 lambda: bank.set_detector(1.0, 1.0, first_channel=n - 1, count=2), lambda: bank.reset(n, 1)):
        with pytest.raises(dspfx.DspfxError) as e:
            call()
        assert e.value.status == -1 and "talkers" in str(e.value), str(e.value)
    assert not ref.assign([0], first_channel=2048) and not ref.assign([2, 2, 0, 0], first_channel=1025)
    assert np.array_equal(bank.room_of(), before) and list(bank.counts()) == [1024, 1024, 4]
    step(dspfx, torch, bank, ref, x[2 * NF:], n, tile, "refused calls change nothing")
    bank.close()


# ---- 5. pins and the floor -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", TWO)
def test_pins_and_the_floor(dspfx, torch_cuda, n, tile):
    torch = torch_cuda
    rng = np.random.default_rng(500 + n)
    bank, ref = pair(dspfx, n, tile, table(n), top=2)
    x = R.noise(rng, 6 * NF, n) * np.float32(0.1)
    loud = [2, 4, 6, 8]                                          # room 0's four loudest, in this order
    for k, c in enumerate(loud):
        x[:, c] *= np.float32(9 - k)
    step(dspfx, torch, bank, ref, x[:NF], n, tile, "no pins")
    assert list(ref.talkers[0, :2]) == [2, 4]
    pins = np.zeros(n, np.uint8)
    pins[2], pins[4], pins[n - 1] = dspfx.TALKERS_OPEN, dspfx.TALKERS_SHUT, dspfx.TALKERS_OPEN
    both(bank, ref, lambda b: b.set_pin(pins))
    both(bank, ref, lambda b: b.assign([dspfx.NO_ROOM], first_channel=n - 1))
    step(dspfx, torch, bank, ref, x[NF:2 * NF], n, tile, "pins")
    assert list(ref.talkers[0, :2]) == [6, 8], "an OPEN pin takes no slot, a SHUT pin never appears"
    assert ref.target[2] == 1 and ref.target[4] == 0 and ref.target[n - 1] == 1
    got = step(dspfx, torch, bank, ref, x[2 * NF:3 * NF], n, tile, "pins, heard")
    assert got[-1, 2] == x[3 * NF - 1, 2] and not got[-1, 4] and got[-1, 6] == x[3 * NF - 1, 6]
    both(bank, ref, lambda b: b.set_pin(dspfx.TALKERS_AUTO, first_channel=2, count=3))
    floor = float(np.nextafter(ref.level[4], np.float32(0)))     # the level channel 4 will have again is above it ...
    both(bank, ref, lambda b: b.set_floor(floor))
    step(dspfx, torch, bank, ref, x[2 * NF:3 * NF], n, tile, "a floor under two channels")
    assert list(ref.talkers[0, :2]) == [2, 4]
    both(bank, ref, lambda b: b.set_floor(float(ref.level[4])))  # ... and a level equal to the floor is not
    step(dspfx, torch, bank, ref, x[2 * NF:3 * NF], n, tile, "a floor at a level")
    assert list(ref.talkers[0, :3]) == [2, -1, -1] and (ref.talkers[1] == -1).all()
    bank.close()


# ---- 6. edge values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", TWO)
def test_edge_values(dspfx, torch_cuda, n, tile):
    """NaN, both infinities, signed zeros and subnormals in the samples.  The restatement's envelope is first held to the oracle's
    on this very block (NaN for NaN); the bank's level after every one-frame run is then that envelope wherever it is above zero"""
    torch = torch_cuda
    x, tab = E.edge_block(n, 3 * NF)
    a, r = 48.0, 1000.0
    probe = R.Talkers(n, table(n))
    probe.set_detector(a, r)
    env_ref = []
    for b in range(2):
        probe.run(x[b * NF:(b + 1) * NF], gate=False)
        env_ref.append(probe.envs)
    env_ref = np.concatenate(env_ref)
    for c in tab:
        want = O.chain_run([O.Node(O.ENVELOPE, [a, r])], x[:2 * NF, c], 0)
        E.same_bits_or_nan(env_ref[:, c], want, None, f"envelope of channel {c} ({tab[c]})")
    assert np.isnan(env_ref).any() and E.is_subnormal(env_ref).any()
    # one-frame runs over the second block (the non-finite values sit there), after the first block in one run
    bank, ref = pair(dspfx, n, tile, table(n), top=8)
    both(bank, ref, lambda b: b.set_detector(a, r))
    step(dspfx, torch, bank, ref, x[:NF], n, tile, "the clean block")
    for f in range(NF, 2 * NF):
        step(dspfx, torch, bank, ref, x[f:f + 1], n, tile, f"frame {f}")
        with np.errstate(invalid="ignore"):
            assert np.array_equal(bits(ref.level), bits(np.where(ref.envs[0] > 0, ref.envs[0], np.float32(0))))
    poisoned = np.flatnonzero(np.isnan(ref.env))
    assert len(poisoned) >= 1 and all(tab[c] in ("nan", "inf_pair", "inf") for c in poisoned)
    got = step(dspfx, torch, bank, ref, x[2 * NF:], n, tile, "after the poison")
    assert not np.isin(ref.talkers, poisoned).any() and not ref.level[poisoned].any(), "a NaN envelope is never a talker"
    assert np.isfinite(got[:, [c for c in range(n) if c not in tab]]).all()
    for c in poisoned:
        both(bank, ref, lambda b: b.reset(int(c), 1))
    step(dspfx, torch, bank, ref, x[:NF], n, tile, "after the reset")
    assert np.isfinite(ref.env).all() and (ref.level[poisoned] > 0).all()
    bank.close()


# ---- 7. streams and threads ------------------------------------------------------------------------------------------------
def test_stream_order_across_two_streams(dspfx, torch_cuda):
    torch = torch_cuda
    n, tile = 256, 64
    bank, ref = pair(dspfx, n, tile, table(n), top=3, seed=70)
    x = R.noise(np.random.default_rng(71), 8 * NF, n)
    dxs = [device(dspfx, torch, x[i * NF:(i + 1) * NF], tile) for i in range(8)]
    dys = [torch.empty_like(d) for d in dxs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i in range(8):
        bank.run(dxs[i], NF, out=dys[i], stream=streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    got = np.concatenate([host(dspfx, d, NF, n, tile) for d in dys])
    assert np.array_equal(bits(got), bits(ref.run_blocks(x)))
    tables_equal(torch, bank, ref, "two streams")
    bank.close()


def test_stores_from_a_second_thread(dspfx, torch_cuda):
    """one thread stores detectors, pins and seats while another submits 50 runs.  The block is the same every time and every
    envelope already sits on its sample's magnitude (|x| is constant over the block, attack 0 took it there), so a level is that
    magnitude under any detector and a run's table is a function of the pins and seats alone: it must be the restatement's for
    some prefix of the stores, and the prefixes never go back"""
    torch = torch_cuda
    n, tile, G = 256, 64, 4
    gs = [0, 64, 128, 192, 256]
    rng = np.random.default_rng(80)
    mag = rng.uniform(0.1, 1.0, n).astype(np.float32)
    x = (mag * rng.choice([-1.0, 1.0], (NF, n))).astype(np.float32)
    dx = device(dspfx, torch, x, tile)
    bank, ref = pair(dspfx, n, tile, gs, top=3)
    step(dspfx, torch, bank, ref, x, n, tile, "priming")
    assert np.array_equal(bits(ref.env), bits(mag)) and np.array_equal(bits(ref.level), bits(mag))
    calls, tables = [], [R.select(mag, ref.room, G, ref.top, 0.0, ref.pin)[0]]
    for i in range(150):
        first, count = int(rng.integers(0, n)), int(rng.integers(1, 40))
        count = min(count, n - first)
        kind = i % 3
        if kind == 0:
            arg = (rng.choice(ATTACKS, count).astype(np.float32), rng.choice(RELEASES, count).astype(np.float32))
            assert ref.set_detector(*arg, first_channel=first)
        elif kind == 1:
            arg = rng.integers(0, 3, count).astype(np.uint8)
            assert ref.set_pin(arg, first_channel=first)
        else:
            arg = rng.integers(0, G, count).astype(np.uint32)
            arg[rng.random(count) < 0.2] = dspfx.NO_ROOM
            assert ref.assign(arg, first_channel=first)
        calls.append((kind, arg, first))
        tables.append(R.select(mag, ref.room, G, ref.top, 0.0, ref.pin)[0])
    errors = []

    def storer():
        try:
            for kind, arg, first in calls:
                if kind == 0:
                    bank.set_detector(*arg, first_channel=first)
                elif kind == 1:
                    bank.set_pin(arg, first_channel=first)
                else:
                    bank.assign(arg, first_channel=first)
        except Exception as e:                                   # noqa: BLE001
            errors.append(e)

    t = threading.Thread(target=storer)
    t.start()
    seen = []
    for _ in range(50):
        bank.run(dx, NF, gate=False)
        seen.append(bank.talkers().cpu().numpy().copy())
    t.join()
    assert not errors, errors
    at = 0
    for k, got in enumerate(seen):
        while at < len(tables) and not np.array_equal(got, tables[at]):
            at += 1
        assert at < len(tables), f"run {k}: its table is no prefix's at or after the one before"
    assert np.array_equal(bank.room_of(), ref.room_of()) and np.array_equal(bank.counts(), ref.counts())
    # every store has arrived, the detectors too: from a reset on, other blocks give the restatement's bits
    both(bank, ref, lambda b: b.reset())
    y = R.noise(rng, 3 * NF, n)
    for b in range(3):
        step(dspfx, torch, bank, ref, y[b * NF:(b + 1) * NF], n, tile, f"after the threads, block {b}")
    bank.close()


# ---- 8. full size ----------------------------------------------------------------------------------------------------------
def test_full_size(dspfx, torch_cuda):
    """2^20 channels x 128 frames, tiled 256, 4096 rooms of 256, top 3, attack 48, release 24000, noise in every channel; two
    alternating buffer pairs, device events, median of 20 after 10 warm-ups.  Asserted: the gated run fits the 2.667 ms a 128-frame
    block lasts at 48 kHz, and it takes at most twice Engine([Envelope(48, 24000)]) on the same buffers, measured here -- a guard
    against a spill or an uncoalesced path, not a target.  Printed: the gated and the metering time with their fractions of 8 TB/s
    (two block-units and one), the engine's time, and a flat copy of the gated run's bytes."""
    torch = torch_cuda
    n, nf, tile, room = 1 << 20, 128, 256, 256
    eng = dspfx.Engine(n, nf, link_flags=0, tile_channels=tile)
    eng.set_chain([dspfx.Envelope(48.0, 24000.0)])
    assert eng.kernels_ready()
    xs = [torch.empty(nf * n, dtype=torch.float32, device="cuda") for _ in range(2)]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    for i, x in enumerate(xs):
        eng.fill_noise(x, nf, 1000 * i)

    def timed(fn):
        for i in range(10):
            fn(i)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(21)]
        torch.cuda.synchronize()
        ev[0].record()
        for i in range(20):
            fn(i)
            ev[i + 1].record()
        torch.cuda.synchronize()
        return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(20)]))

    assert dspfx.talkers_plan(n, n // room) == 29 * n + 69 * (n // room) + 4
    bank = dspfx.Talkers(n, group_size=room, top=3, tile_channels=tile, max_frames=nf)
    bank.set_detector(48.0, 24000.0)
    t_gated = timed(lambda i: bank.run(xs[i % 2], nf, out=ys[i % 2]))
    torch.cuda.synchronize()
    talk = bank.talkers().cpu().numpy()
    assert (talk[:, :3] >= 0).all() and (talk[:, 3:] == -1).all() and (talk[:, :3] // room == np.arange(n // room)[:, None]).all()
    assert float(bank.targets().sum()) == 3 * (n // room)
    t_meter = timed(lambda i: bank.run(xs[i % 2], nf, gate=False))
    bank.close()
    t_eng = timed(lambda i: eng.process(xs[i % 2], out=ys[i % 2], n_frames=nf))
    eng.close()
    t_copy = timed(lambda i: ys[i % 2].copy_(xs[i % 2]))
    unit = nf * n * 4
    print(f"full size talkers: gated {t_gated:.4f} ms ({2 * unit / t_gated / 1e9 / 8.0:.3f} of 8 TB/s on {2 * unit / 2**20:.0f} MiB), "
          f"metering {t_meter:.4f} ms ({unit / t_meter / 1e9 / 8.0:.3f} of 8 TB/s on {unit / 2**20:.0f} MiB), "
          f"Engine([Envelope(48, 24000)]) {t_eng:.4f} ms (gated x {t_gated / t_eng:.3f}), flat copy of the gated bytes {t_copy:.4f} ms "
          f"(gated x {t_gated / t_copy:.3f})")
    assert t_gated * 1e-3 <= 128 / 48000, t_gated
    assert t_gated <= 2 * t_eng, (t_gated, t_eng)
