"""Several responses on one convolver bank, on the GPU.  The reference for bit identity is the single-response path: one
Convolver(N, h_r, mode_r, max_taps=...) per response on the same input; channel c of the bank under test, carrying id r, must
be the same bits as channel c of response r's single bank.  The reference for accuracy is convolve_ref.exact (scipy's
fftconvolve in float64) at the FIR row's bar, 1e-6 relative RMS per channel.  Input: white noise, per-channel amplitudes 1e-3
to 1, as in test_convolve_gpu.py."""
import numpy as np
import pytest

import convolve_ref as R

pytestmark = pytest.mark.gpu

B = 128
BAL, AVG = 0, 1
INVALID = -1
# (taps, mode) by id; max_taps; blocks = 2 * slots + 3, so the ring wraps
SMALL = dict(name="small", specs=[(1, BAL), (129, AVG), (300, BAL)], max_taps=640, blocks=2 * 5 + 3)       # P = 1, 2, 3 of 5 slots
LONG = dict(name="long", specs=[(2048, BAL), (2100, AVG), (4200, BAL)], max_taps=4200, blocks=2 * 33 + 3)  # P = 16, 17, 33


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def responses(case):
    return [R.response(T, seed=10 + i) for i, (T, _) in enumerate(case["specs"])]


def pattern(name, N):
    c = np.arange(N)
    if name.startswith("all"):
        return np.full(N, int(name[3:]), np.uint16)
    if name == "ranges":                                                        # boundaries mid-wave (33) and inside a lane pair (33, and 50 is not)
        return ((c >= 33).astype(np.uint16) + (c >= 50).astype(np.uint16)).astype(np.uint16)
    if name == "mod3":
        return (c % 3).astype(np.uint16)
    raise KeyError(name)


def feed(dspfx, torch, bank, x, tile, n_frames=B, in_place=False):
    """x [F][N] (host, frame-major) through `bank`, n_frames per call -> [F][N] (host); one synchronisation at the end"""
    F, N = x.shape
    calls = F // n_frames
    lay = np.stack([dspfx.to_layout(x[i * n_frames:(i + 1) * n_frames], tile).reshape(-1) for i in range(calls)])
    dx = torch.from_numpy(lay).cuda()
    dy = dx if in_place else torch.full_like(dx, float("nan"))
    for i in range(calls):
        bank.run(dx[i], n_frames, out=dy[i])
    torch.cuda.synchronize()
    out = dy.cpu().numpy()
    return np.concatenate([dspfx.from_layout(out[i], n_frames, N, tile) for i in range(calls)])


def make_bank(dspfx, case, N, tile, ids=None):
    hs = responses(case)
    bank = dspfx.Convolver(N, hs[0], mode=case["specs"][0][1], max_taps=case["max_taps"], tile_channels=tile)
    for i in range(1, len(hs)):
        assert bank.add_response(hs[i], mode=case["specs"][i][1]) == i
    assert bank.responses == len(hs)
    if ids is not None:
        bank.assign(ids)
        assert np.array_equal(bank.response_of, ids)
    return bank


_cache = {}


def noise_of(case, N):
    key = ("x", case["name"], N)
    if key not in _cache:
        x = R.noise(case["blocks"] * B, N, seed=21)
        x.setflags(write=False)
        _cache[key] = x
    return _cache[key]


def singles(dspfx, torch, case, N, tile):
    """[response][F][N]: every response's single-response bank on the case's input; computed once, nobody writes into it"""
    key = ("single", case["name"], N, tile)
    if key not in _cache:
        x = noise_of(case, N)
        out = []
        for h, (_, mode) in zip(responses(case), case["specs"]):
            bank = dspfx.Convolver(N, h, mode=mode, max_taps=case["max_taps"], tile_channels=tile)
            out.append(feed(dspfx, torch, bank, x, tile))
            bank.close()
        ref = np.stack(out)
        ref.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def mixed(dspfx, torch, case, N, tile, pat):
    """(ids, output [F][N]) of a bank of the case's responses with the pattern's ids on the case's input; computed once"""
    key = ("mixed", case["name"], N, tile, pat)
    if key not in _cache:
        ids = pattern(pat, N)
        bank = make_bank(dspfx, case, N, tile, ids)
        got = feed(dspfx, torch, bank, noise_of(case, N), tile)
        bank.close()
        got.setflags(write=False)
        _cache[key] = (ids, got)
    return _cache[key]


def expected(ref, ids):
    """[F][N]: channel c from the single bank of ids[c]"""
    return np.take_along_axis(ref, ids[None, None, :].astype(np.int64), axis=0)[0]


def assert_same_bits(got, want, what=""):
    bad = bits(got) != bits(want)
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} samples differ, channels {np.unique(np.nonzero(bad)[1])[:16]}"


# ---- 1, 2: bit identity ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pat", ["all0", "all1", "all2", "ranges", "mod3"])
@pytest.mark.parametrize("N,tile", [(64, 0), (256, 64), (67, 0)], ids=["n64", "n256_tile64", "n67"])
def test_bit_identity_small_partitions(dspfx, torch_cuda, N, tile, pat):
    """P = 1, 2, 3 of 5 slots, 13 blocks: two channels a lane (N even) and one (N = 67); waves of one id and mixed ones."""
    ref = singles(dspfx, torch_cuda, SMALL, N, tile)
    ids, got = mixed(dspfx, torch_cuda, SMALL, N, tile, pat)
    assert np.isfinite(got).all() and got.any()
    assert_same_bits(got, expected(ref, ids), f"N={N} tile={tile} {pat}")


@pytest.mark.parametrize("N", [64, 67])
def test_bit_identity_group_boundaries_inside_a_longer_wave(dspfx, torch_cuda, N):
    """P = 16, 17, 33 and ids c % 3: a short last group of partitions beside a neighbour's full group of 16."""
    ref = singles(dspfx, torch_cuda, LONG, N, 0)
    ids, got = mixed(dspfx, torch_cuda, LONG, N, 0, "mod3")
    assert np.isfinite(got).all() and got.any()
    assert_same_bits(got, expected(ref, ids), f"N={N} mod3")


# ---- 3: accuracy ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,pat", [(SMALL, "ranges"), (SMALL, "mod3"), (LONG, "mod3")], ids=["small-ranges", "small-mod3", "long-mod3"])
def test_accuracy_of_the_mixed_banks(dspfx, torch_cuda, case, pat):
    N = 64
    ids, got = mixed(dspfx, torch_cuda, case, N, 0, pat)
    x = noise_of(case, N)
    worst = 0.0
    for r, (h, (T, mode)) in enumerate(zip(responses(case), case["specs"])):
        ch = np.nonzero(ids == r)[0]
        div = float(np.float32(1.0) / np.float32(T)) if mode == AVG else 1.0
        rr = R.rel_rms(got[:, ch], R.exact(x[:, ch], h, div))
        print(f"{case['name']} {pat}: response {r} (T={T}, P={R.partitions(T)}, {'Average' if mode == AVG else 'Balanced'}, "
              f"{len(ch)} channels): worst rel RMS {rr.max():.3e}")
        worst = max(worst, rr.max())
    assert worst <= R.BAR


# ---- 4: NaN containment and lifetime --------------------------------------------------------------------------------

def test_nan_stays_in_its_channel_for_its_own_partitions(dspfx, torch_cuda):
    """Ids alternate between P = 1 (even channels) and P = 3 (odd).  One NaN in block 3 of channel 10 (P = 1; its lane
    partner 11 has P = 3): channel 10 carries it for P + 1 = 2 blocks, not for the longer response's 4, and is otherwise its
    single bank (fed the same NaN); nobody else sees it."""
    N, blocks, first = 64, 10, 3
    x = noise_of(SMALL, N)[:blocks * B].copy()
    x[first * B + 77, 10] = np.nan
    hs = responses(SMALL)
    ids = np.where(np.arange(N) % 2 == 0, 0, 2).astype(np.uint16)
    bank = make_bank(dspfx, SMALL, N, 0, ids)
    got = feed(dspfx, torch_cuda, bank, x, 0)
    bank.close()
    single0 = dspfx.Convolver(N, hs[0], mode=SMALL["specs"][0][1], max_taps=SMALL["max_taps"])
    ref0 = feed(dspfx, torch_cuda, single0, x, 0)
    single0.close()
    clean = singles(dspfx, torch_cuda, SMALL, N, 0)[:, :blocks * B]
    others = [c for c in range(N) if c != 10]
    assert_same_bits(got[:, others], expected(clean, ids)[:, others], "the other channels")
    bad = np.isnan(got[:, 10]).reshape(blocks, B).any(axis=1)
    assert bad[first] and not bad[:first].any() and not bad[first + 2:].any(), bad
    assert np.array_equal(np.isnan(got[:, 10]), np.isnan(ref0[:, 10]))
    ok = ~np.isnan(ref0[:, 10])                                                 # (a NaN's payload is not part of the contract)
    assert np.array_equal(bits(got[ok, 10]), bits(ref0[ok, 10]))
    assert_same_bits(got[(first + 2) * B:, 10:11], ref0[(first + 2) * B:, 10:11], "channel 10 from the third block on")


# ---- 5: assign keeps the history ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_frames,in_place", [(B, False), (2 * B, True)], ids=["128", "256_in_place"])
def test_assign_keeps_the_history(dspfx, torch_cuda, n_frames, in_place):
    N, cut, blocks = 64, 4, 10
    x = noise_of(SMALL, N)[:blocks * B]
    ref = singles(dspfx, torch_cuda, SMALL, N, 0)[:, :blocks * B]
    moved = [5, 6] + list(range(40, 48))
    bank = make_bank(dspfx, SMALL, N, 0)
    a = feed(dspfx, torch_cuda, bank, x[:cut * B], 0, n_frames, in_place)
    bank.assign(2, first_channel=5)                                             # an int, a list, an array
    bank.assign([2], first_channel=6)
    bank.assign(np.full(8, 2), first_channel=40)
    ids = bank.response_of
    assert sorted(np.nonzero(ids == 2)[0]) == moved and np.count_nonzero(ids) == len(moved)
    b = feed(dspfx, torch_cuda, bank, x[cut * B:], 0, n_frames, in_place)
    bank.close()
    assert_same_bits(a, ref[0, :cut * B], "before the assign: response 0 everywhere")
    assert_same_bits(b, expected(ref, ids)[cut * B:], "from the assign on: response 2's bank on the same ten blocks")


# ---- 6: lifecycle ---------------------------------------------------------------------------------------------------

def test_lifecycle(dspfx, torch_cuda):
    torch = torch_cuda
    N, step = 64, 3
    x = R.noise(8 * step * B, N, seed=33)
    hs = responses(SMALL)
    modes = [m for _, m in SMALL["specs"]]
    ids = pattern("ranges", N)
    bank = make_bank(dspfx, SMALL, N, 0, ids)
    ref = [dspfx.Convolver(N, h, mode=m, max_taps=SMALL["max_taps"]) for h, m in zip(hs, modes)]
    at = [0]

    def advance(what, first=None):
        """the next `step` blocks through the bank and every single bank: each channel is its response's single bank"""
        lo = at[0]
        at[0] += step * B
        seg = x[lo:at[0]] if first is None else np.concatenate([first, x[lo + len(first):at[0]]])
        got = feed(dspfx, torch, bank, seg, 0)
        want = np.stack([feed(dspfx, torch, r, seg, 0) for r in ref])
        assert_same_bits(got, expected(want, bank.response_of), what)
        return got, want

    advance("as created")
    h1b = R.response(200, seed=41)
    bank.set_response(1, h1b, mode=BAL)                                         # only the channels on id 1 change
    ref[1].set_taps(h1b, mode=BAL)
    advance("after set_response(1)")
    h0b = R.response(640, seed=42)
    bank.set_taps(h0b, mode=AVG)                                                # only the channels on id 0 change
    ref[0].set_taps(h0b, mode=AVG)
    assert bank.partitions == 5
    advance("after set_taps")
    h3 = R.response(257, seed=43)
    assert bank.add_response(h3, mode=AVG) == 3 and bank.responses == 4         # nobody carries it yet
    advance("after add_response, before any assign")
    ref.append(dspfx.Convolver(N, h3, mode=AVG, max_taps=SMALL["max_taps"]))
    feed(dspfx, torch, ref[3], x[:at[0]], 0)                                    # the same input history
    bank.assign([3, 3, 3, 3], first_channel=30)                                 # across the boundary at 33
    advance("after assign to the added response")
    before = bank.response_of
    for call in (lambda: bank.assign(bank.responses, first_channel=7),          # an id the bank does not hold
                 lambda: bank.assign([0, 1, 4], first_channel=0),               # ... nothing of it is stored
                 lambda: bank.assign([1, 1], first_channel=N - 1),              # past the channels
                 lambda: bank.assign([1], first_channel=N),
                 lambda: bank.add_response(R.response(641)),                    # longer than max_taps
                 lambda: bank.set_response(2, R.response(641)),
                 lambda: bank.set_response(4, R.response(10))):
        with pytest.raises(dspfx.DspfxError) as ei:
            call()
        assert ei.value.status == INVALID
    assert np.array_equal(bank.response_of, before) and bank.responses == 4
    advance("after the refused calls")
    bank.reset()
    for r in ref:
        r.reset()
    got, _ = advance("after reset", first=np.zeros((B, N), np.float32))
    assert not got[:B].any()                                                    # silence in, silence out: the history is gone
    assert got[B:].any() and np.array_equal(bank.response_of, before) and bank.responses == 4
    for o in ref + [bank]:
        o.close()


# ---- 7: the rooms path ----------------------------------------------------------------------------------------------

def test_rooms_two_halls_master_chain_without_a_host_copy(dspfx, torch_cuda):
    """Engine(256) -> MixGroups(group_size=32) -> a two-hall Convolver over the 8 buses -> master Engine(8), device to device,
    against the same path with one single-response bank per hall, each bus column taken from its hall's bank."""
    torch = torch_cuda
    n, blocks = 256, 12
    chain = [dspfx.BiQuad(1.0, -1.8, 0.81, 0.0025, 0.005, 0.0025), dspfx.Gain(0.5)]
    master = [dspfx.LowPass(0.25), dspfx.Gain(2.0)]
    booth, church = R.response(300, seed=51), R.response(1000, seed=52)
    eng = dspfx.Engine(n, B, link_flags=3, tile_channels=0)
    eng.set_chain(chain)
    mg = dspfx.MixGroups(n, group_size=32, max_frames=B)
    G = mg.groups
    halls = np.array([0, 1, 1, 0, 0, 0, 1, 1], np.uint16)
    assert G == len(halls)
    reverb = dspfx.Convolver(G, booth, max_taps=1000)
    assert reverb.add_response(church, mode=AVG) == 1
    reverb.assign(halls)
    single = [dspfx.Convolver(G, booth, max_taps=1000), dspfx.Convolver(G, church, mode=AVG, max_taps=1000)]
    mengs = []
    for _ in range(2):
        m = dspfx.Engine(G, B, link_flags=3, tile_channels=0)
        m.set_chain(master)
        mengs.append(m)
    in_church = torch.from_numpy(halls.astype(bool)).cuda()
    x = torch.empty(B * n, dtype=torch.float32, device="cuda")
    y = torch.empty_like(x)
    buses = torch.empty((blocks, B, G), dtype=torch.float32, device="cuda")
    wet, wet_ref, out, out_ref = (torch.empty_like(buses) for _ in range(4))
    for b in range(blocks):
        eng.fill_noise(x, B, b * B)
        eng.process(x, out=y, n_frames=B)
        mg.run(y, B, out=buses[b])
        reverb.run(buses[b], B, out=wet[b])
        mengs[0].process(wet[b], out=out[b], n_frames=B)
        w0 = single[0].run(buses[b], B).view(B, G)
        w1 = single[1].run(buses[b], B).view(B, G)
        wet_ref[b] = torch.where(in_church, w1, w0)
        mengs[1].process(wet_ref[b], out=out_ref[b], n_frames=B)
    torch.cuda.synchronize()
    wh, wr, oh, orr = (t.cpu().numpy().reshape(blocks * B, G) for t in (wet, wet_ref, out, out_ref))
    assert wh.any() and oh.any() and np.isfinite(oh).all()
    assert_same_bits(wh, wr, "reverb on the buses")
    assert_same_bits(oh, orr, "after the master chain")
    for o in mengs + single + [reverb, mg, eng]:
        o.close()


# ---- 8: full size ---------------------------------------------------------------------------------------------------

def test_full_size(dspfx, torch_cuda):
    """G = 4096 buses, four responses of 48 000 taps (P = 375), ids in contiguous quarters, one 128-frame block: a run takes
    no longer than the 2.667 ms a block lasts (the project's own budget).  Device events, the median of 20 after P + 5 warm-up
    runs.  Printed beside it: the fraction of 8 TB/s the ring read alone is, the ratio to a single-response bank of the same
    size timed here too, and the same three figures for the interleaved pattern c % 4 (every wave mixed, every lane's pair
    split).  No ratio is asserted: none has been measured."""
    torch = torch_cuda
    N, T, reps, halls = 4096, 48000, 20, 4
    budget = B / 48000 * 1e3
    hs = [R.response(T, seed=60 + i) for i in range(halls)]
    x = torch.from_numpy(R.noise(B, N, seed=11).reshape(-1)).cuda()
    y = torch.empty_like(x)

    def timed(bank):
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            bank.run(x, B, out=y)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    def warm(bank, runs):
        for _ in range(runs):
            bank.run(x, B, out=y)
        torch.cuda.synchronize()

    single = dspfx.Convolver(N, hs[0])
    P = single.partitions
    warm(single, P + 5)
    single_ms = timed(single)
    single.close()
    bank = dspfx.Convolver(N, hs[0])
    for i in range(1, halls):
        assert bank.add_response(hs[i]) == i
    bank.assign(np.repeat(np.arange(halls), N // halls))
    warm(bank, P + 5)
    quarters_ms = timed(bank)
    got = y.cpu().numpy().reshape(B, N)
    bank.assign(np.arange(N) % halls)
    warm(bank, 5)
    inter_ms = timed(bank)
    got_inter = y.cpu().numpy().reshape(B, N)
    bank.close()
    nbytes = P * 1024 * N
    for what, ms in (("contiguous quarters", quarters_ms), ("interleaved c % 4", inter_ms)):
        print(f"full size: N={N} T={T} P={P}, {halls} responses, {what}: {ms:.3f} ms per run (budget {budget:.3f}), the ring read "
              f"alone is {nbytes / (ms * 1e-3) / 8e12:.2f} of the 8 TB/s peak, {ms / single_ms:.2f} x the single-response bank "
              f"({single_ms:.3f} ms)")
    assert np.isfinite(got).all() and got.any() and np.isfinite(got_inter).all() and got_inter.any()
    assert quarters_ms <= budget
