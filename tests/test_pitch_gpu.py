"""The Pitch Detector bank on the GPU (dspfx_pitch_*) against the float64 restatement in pitch_ref.py: parity over sines,
sawtooths, noisy tones, DC, silence and sub-threshold windows in both layouts and at a ragged N; the frame rule and the hold;
split invariance; the slot path; threshold stores, reset and argument errors; an Engine feeding a bank; one window at 2^20
channels."""
import numpy as np
import pytest

import pitch_ref as R

pytestmark = pytest.mark.gpu

B = 128
RATE = 48000.0
# Where the restatement's margin is below this, f32 rounding may flip a decision (pitch_ref.detect): such channels are skipped.
MARGIN = 1e-4
# Bars for the channels that agree.  Measured (f32 FFTs against the float64 restatement, printed by the parity tests): frequency
# <= 1.9e-5 relative, clarity <= 1.4e-5 absolute, the worst at 2^20 channels.  The bars keep about 5x above that: the error grows
# where the parabola through the peak is flattest (the lowest pitches) and with noise.
FREQ_RTOL = 1e-4
CLARITY_ATOL = 1e-4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def signal_set(n, seed=1, frames=R.WINDOW):
    """[frames][n]: a varied mix of the windows the detector meets, cycling over the kinds."""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)[:, None] / RATE
    out = np.zeros((frames, n))
    for c in range(n):
        kind = c % 8
        f = float(np.exp(rng.uniform(np.log(50.0), np.log(4000.0))))
        a = rng.uniform(0.1, 0.9)
        ph = rng.uniform(0, 2 * np.pi)
        tc = t[:, 0]
        if kind in (0, 1):
            x = a * np.sin(2 * np.pi * f * tc + ph)
        elif kind == 2:                                  # sawtooth
            x = a * (2.0 * ((f * tc + ph / (2 * np.pi)) % 1.0) - 1.0)
        elif kind in (3, 4):                             # tone plus noise, SNR 20 / 0 dB
            snr = 20.0 if kind == 3 else 0.0
            x = a * np.sin(2 * np.pi * f * tc + ph)
            x = x + rng.standard_normal(frames) * a / np.sqrt(2) * 10 ** (-snr / 20)
        elif kind == 5:                                  # DC
            x = np.full(frames, a)
        elif kind == 6:                                  # silence
            x = np.zeros(frames)
        else:                                            # sub-threshold: power < 0.5
            x = 0.015 * np.sin(2 * np.pi * f * tc + ph)
        out[:, c] = x
    return out.astype(np.float32)


def _push(dspfx, torch, bank, x, sizes=None):
    """push frame-major numpy x [frames][N] in the bank's layout, in blocks of `sizes` (default: one push)"""
    frames = x.shape[0]
    sizes = sizes or [frames]
    f = 0
    k = 0
    while f < frames:
        n = min(sizes[k % len(sizes)], frames - f)
        blk = dspfx.to_layout(x[f:f + n], bank.tile_channels)
        bank.push(torch.from_numpy(blk).cuda(), n)
        f += n
        k += 1


def _read(torch, bank):
    fr, cl = bank.read()
    torch.cuda.synchronize()
    return fr.cpu().numpy(), cl.cpu().numpy()


def _parity(got_f, got_c, win, P=0.5, C=0.5, K=0.5, prev=None):
    """-> (max freq rel err, max clarity abs err, channels checked)"""
    found, _, fr, cl, margin = R.detect_bank(win.T, P, C, K)
    pf = np.zeros_like(fr) if prev is None else prev[0]
    pc = np.zeros_like(cl) if prev is None else prev[1]
    ok = margin > MARGIN
    exp_f = np.where(found, fr, pf)
    exp_c = np.where(found, cl, pc)
    got_found = got_f != pf
    assert np.array_equal(got_found[ok & found], np.ones(int((ok & found).sum()), bool)), np.nonzero(ok & found & ~got_found)
    assert np.array_equal(got_f[ok & ~found], pf[ok & ~found]), np.nonzero(ok & ~found & got_found)
    sel = ok & found
    # the chosen integer lag: tau + delta with |delta| <= 1/2 around the restatement's
    tau_ref = R.detect_bank(win[:, sel].T, P, C, K)[1]
    assert np.all(np.abs(RATE / got_f[sel].astype(np.float64) - tau_ref) <= 0.5 + 1e-3)
    ferr = np.abs(got_f[sel] / exp_f[sel] - 1.0)
    cerr = np.abs(got_c[sel] - exp_c[sel])
    assert ferr.max(initial=0) <= FREQ_RTOL, (ferr.max(), np.nonzero(sel)[0][np.argmax(ferr)])
    assert cerr.max(initial=0) <= CLARITY_ATOL, (cerr.max(), np.nonzero(sel)[0][np.argmax(cerr)])
    return float(ferr.max(initial=0)), float(cerr.max(initial=0)), int(sel.sum())


@pytest.mark.parametrize("n,tile", [(4096, 0), (4096, 64), (77, 0), (160, 32)])
def test_parity_with_the_restatement(dspfx, torch_cuda, n, tile):
    torch = torch_cuda
    x = signal_set(n, seed=n + tile)
    bank = dspfx.PitchBank(n, tile_channels=tile)
    _push(dspfx, torch, bank, np.concatenate([x, np.zeros((1, n), np.float32)]))
    assert bank.windows == 1
    f, c = _read(torch, bank)
    ferr, cerr, checked = _parity(f, c, x.astype(np.float64))
    print(f"n={n} tile={tile}: {checked} channels checked, freq rel err {ferr:.2e}, clarity abs err {cerr:.2e}")
    assert checked > n // 3


def test_sines_50hz_to_4khz(dspfx, torch_cuda):
    torch = torch_cuda
    freqs = np.geomspace(50.0, 4000.0, 256)
    t = np.arange(R.WINDOW)[:, None] / RATE
    x = (0.5 * np.sin(2 * np.pi * freqs[None, :] * t + 0.3)).astype(np.float32)
    bank = dspfx.PitchBank(len(freqs))
    _push(dspfx, torch, bank, np.concatenate([x, x[:1]]))
    f, c = _read(torch, bank)
    _parity(f, c, x.astype(np.float64))
    hi = freqs > 100.0                     # above the alias band every sine reads as itself
    assert np.all(np.abs(f[hi] / freqs[hi] - 1.0) < 2e-3)


def test_frame_rule_and_hold(dspfx, torch_cuda):
    torch = torch_cuda
    n = 256
    x1 = signal_set(n, seed=5)
    x2 = signal_set(n, seed=6)
    x2[:, ::3] = 0.0                                   # None windows: these channels keep window 0's values
    bank = dspfx.PitchBank(n)
    _push(dspfx, torch, bank, x1)
    f, c = _read(torch, bank)
    assert bank.windows == 0 and not f.any() and not c.any()        # exactly 1024 frames: nothing yet
    _push(dspfx, torch, bank, x2[:1])
    f1, c1 = _read(torch, bank)
    assert bank.windows == 1 and f1.any()
    _parity(f1, c1, x1.astype(np.float64))
    _push(dspfx, torch, bank, x2[1:])
    _push(dspfx, torch, bank, x2[:1])
    f2, c2 = _read(torch, bank)
    assert bank.windows == 2
    _parity(f2, c2, x2.astype(np.float64), prev=(f1, c1))
    assert np.array_equal(f2[::3], f1[::3]) and np.array_equal(c2[::3], c1[::3])


def test_long_push_runs_its_windows_in_order(dspfx, torch_cuda):
    torch = torch_cuda
    n = 192
    x = np.concatenate([signal_set(n, seed=s) for s in (11, 12, 13)])
    x[2048:, 1::2] = 0.0                               # window 2 gives None on odd channels
    one = dspfx.PitchBank(n)
    _push(dspfx, torch, one, x)                        # 3072 frames: windows 0 and 1
    assert one.windows == 2
    f, c = _read(torch, one)
    host = R.HostBank(n)
    host.push(x)
    assert host.windows == 2
    ok = (R.detect_bank(x[:1024].T.astype(np.float64))[4] > MARGIN) & (R.detect_bank(x[1024:2048].T.astype(np.float64))[4] > MARGIN)
    assert np.allclose(f[ok], host.freq[ok], rtol=FREQ_RTOL, atol=0) and np.allclose(c[ok], host.clarity[ok], atol=CLARITY_ATOL)
    _push(dspfx, torch, one, x[:1])                    # window 2
    assert one.windows == 3


def _state(torch, bank):
    f, c = _read(torch, bank)
    return f.view(np.uint32).copy(), c.view(np.uint32).copy(), bank.windows


@pytest.mark.parametrize("tile", [0, 32])
def test_split_invariance(dspfx, torch_cuda, tile):
    torch = torch_cuda
    n = 128
    x = np.concatenate([signal_set(n, seed=s) for s in (21, 22, 23)] + [signal_set(n, seed=24)[:300]])
    states = []
    for sizes in ([128], [1000], [37], [1, 1023, 2048, 128]):
        bank = dspfx.PitchBank(n, tile_channels=tile)
        _push(dspfx, torch, bank, x, sizes)
        states.append(_state(torch, bank))
    for s in states[1:]:
        assert np.array_equal(s[0], states[0][0]) and np.array_equal(s[1], states[0][1]) and s[2] == states[0][2] == 3


@pytest.mark.parametrize("tile", [0, 64])
def test_slot_path_is_bit_identical_to_a_copy(dspfx, torch_cuda, tile):
    torch = torch_cuda
    n = 256
    x = np.concatenate([signal_set(n, seed=31), signal_set(n, seed=32)[:128]])
    a = dspfx.PitchBank(n, tile_channels=tile)
    b = dspfx.PitchBank(n, tile_channels=tile)
    for k in range(x.shape[0] // B):
        blk = torch.from_numpy(dspfx.to_layout(x[k * B:(k + 1) * B], tile)).cuda()
        a.push(blk, B)
        slot = b.slot_tensor()
        assert slot is not None
        slot.copy_(blk.reshape(-1))
        b.push(slot, B)
    assert a.windows == b.windows == 1
    sa, sb = _state(torch, a), _state(torch, b)
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]) and sa[0].any()
    b.push(torch.zeros(5 * n, device="cuda"), 5)
    assert b.slot() is None                            # not on a slot boundary


def test_threshold_stores_and_reset(dspfx, torch_cuda):
    torch = torch_cuda
    n = 128
    x = signal_set(n, seed=41)
    bank = dspfx.PitchBank(n)
    bank.set_param(dspfx.PITCH_POWER, 1e9)             # every window below the power threshold
    _push(dspfx, torch, bank, np.concatenate([x, x[:1]]))
    f, c = _read(torch, bank)
    assert bank.windows == 1 and not f.any() and not c.any()
    for which, v in ((dspfx.PITCH_POWER, 0.2), (dspfx.PITCH_CLARITY, 0.8), (dspfx.PITCH_PICK, 0.9)):
        bank.set_param(which, v)
    bank.reset()
    assert bank.windows == 0
    f, c = _read(torch, bank)
    assert not f.any() and not c.any()
    _push(dspfx, torch, bank, np.concatenate([x, x[:1]]))
    f, c = _read(torch, bank)
    _parity(f, c, x.astype(np.float64), P=0.2, C=0.8, K=0.9)
    assert f.any()


def test_bad_arguments(dspfx, torch_cuda):
    torch = torch_cuda
    L = dspfx.lib()
    INVALID = -1
    import ctypes as C
    bank = dspfx.PitchBank(64)
    blk = torch.zeros(64 * 128, device="cuda")
    assert L.dspfx_pitch_push(bank.h, C.c_void_p(blk.data_ptr()), 0, None) == INVALID
    assert L.dspfx_pitch_push(bank.h, None, 128, None) == INVALID
    assert L.dspfx_pitch_push(None, C.c_void_p(blk.data_ptr()), 128, None) == INVALID
    assert L.dspfx_pitch_push(bank.h, C.c_void_p(bank.slot()), 64, None) == INVALID      # the slot takes whole blocks
    assert L.dspfx_pitch_set_param(bank.h, 3, 0.5) == INVALID
    assert L.dspfx_pitch_set_param(bank.h, -1, 0.5) == INVALID
    assert L.dspfx_pitch_set_param(bank.h, 0, float("nan")) == INVALID
    assert L.dspfx_pitch_read(bank.h, None, None, None) == INVALID
    for ch, tile, abi in ((0, 0, 2), (96, 64, 2), (96, 3, 2), (64, 0, 1)):
        d = dspfx._PitchDesc(abi, 0, ch, tile, 0.5, 0.5, 0.5)
        h = C.c_void_p()
        assert L.dspfx_pitch_create(C.byref(d), C.byref(h)) == INVALID, (ch, tile, abi)
    assert L.dspfx_pitch_create(None, None) == INVALID


def test_engine_output_into_a_bank(dspfx, torch_cuda):
    """Engine.process writes straight into the bank's slot; the bank's result is the restatement's on the chain's output."""
    torch = torch_cuda
    n = 512
    eng = dspfx.Engine(n, B, link_flags=3)
    eng.set_chain([dspfx.Gain(0.8), dspfx.LowPass(0.3)])
    bank = dspfx.PitchBank(n)
    x = signal_set(n, seed=51, frames=9 * B)
    outs = []
    for k in range(9):
        slot = bank.slot_tensor()
        eng.process(torch.from_numpy(x[k * B:(k + 1) * B]).cuda(), out=slot.view(B, n))
        outs.append(slot.view(B, n).cpu().numpy().copy())
        bank.push(slot, B)
    assert bank.windows == 1
    y = np.concatenate(outs)
    f, c = _read(torch, bank)
    _parity(f, c, y[:R.WINDOW].astype(np.float64))


def test_full_size_one_window(dspfx, torch_cuda):
    """2^20 channels (a 4.5 GiB store): one window, checked on a seeded sample of channels."""
    torch = torch_cuda
    n = 1 << 20
    bank = dspfx.PitchBank(n)
    rng = np.random.default_rng(61)
    sample = np.sort(rng.choice(n, 2048, replace=False))
    base = signal_set(256, seed=62)                    # channel c carries base[:, c % 256] scaled by a per-channel gain
    gain = (0.5 + (np.arange(n) % 7) / 7.0).astype(np.float32)
    src = torch.from_numpy(base).cuda()
    g = torch.from_numpy(gain).cuda()
    idx = torch.arange(n, device="cuda") % 256
    for k in range(R.WINDOW // B):
        blk = src[k * B:(k + 1) * B][:, idx] * g[None, :]
        bank.push(blk.contiguous(), B)
    bank.push(torch.zeros(n, device="cuda"), 1)
    assert bank.windows == 1
    f, c = _read(torch, bank)
    win = (base[:, sample % 256] * gain[None, sample]).astype(np.float64)
    ferr, cerr, checked = _parity(f[sample], c[sample], win)
    print(f"2^20 channels: {checked} sampled channels checked, freq rel err {ferr:.2e}, clarity abs err {cerr:.2e}")


def _tap_docs(dspfx):
    """A chain whose Pitch node reads two links (the biquad in the middle of the chain and the gain), and the same document
    with those two links rewired into the Output node instead of the high-pass."""
    import json
    from dsp_stuff_amd import config
    chain = [dspfx.BiQuad(1.0, -1.8, 0.81, 0.0025, 0.005, 0.0025), dspfx.Gain(0.5), dspfx.HighPass(0.2)]
    doc = json.loads(config.dump_dspconfig(chain))
    bq, gain, out = doc["nodes"][1], doc["nodes"][2], doc["nodes"][4]
    srcs = [[bq["id"], bq["cfg"]["outputs"]["out"]], [gain["id"], gain["cfg"]["outputs"]["out"]]]
    rewired = json.loads(json.dumps(doc))
    doc["nodes"].append({"id": 500, "typename": "pitch", "position": [0, 0],
                         "cfg": {"id": 500, "inputs": {"in": 600}, "outputs": {}, "power_thresh": 0.3, "clarity_thresh": 0.6,
                                 "pick_thresh": 0.8}})
    doc["links"] += [{"lhs": s, "rhs": [500, 600]} for s in srcs]
    into_out = [k for k, l in enumerate(rewired["links"]) if l["rhs"][0] == out["id"]]
    port = rewired["links"][into_out[0]]["rhs"]
    rewired["links"] = [l for k, l in enumerate(rewired["links"]) if k not in into_out] + [{"lhs": s, "rhs": port} for s in srcs]
    return json.dumps(doc), json.dumps(rewired)


@pytest.mark.parametrize("plan", ["fused", "regions", "runs"])
def test_graph_pitch_tap_is_the_rewired_output(dspfx, torch_cuda, plan):
    """GraphEngine(pitch=True): the tap is bit-identical to the same links rewired into the Output node, in each plan; the
    Output block itself is unchanged; the bank holds what a PitchBank fed with the rewired output holds."""
    from dsp_stuff_amd.graph import GraphEngine
    torch = torch_cuda
    n = 256
    doc, rewired = _tap_docs(dspfx)
    kw = {"fused": dict(), "regions": dict(regions=True), "runs": dict(fused=False)}[plan]
    ge = GraphEngine(doc, n, **kw, pitch=True)
    plain = GraphEngine(doc, n, **kw)
    rw = GraphEngine(rewired, n, **kw)
    if plan == "fused":
        assert ge.fused is not None and rw.fused is not None
    elif plan == "regions":
        assert ge.regions and rw.regions
    else:
        assert ge.runs and ge.fused is None and not ge.regions
    ref = dspfx.PitchBank(n, power_thresh=0.3, clarity_thresh=0.6, pick_thresh=0.8)
    gen = torch.Generator(device="cuda").manual_seed(71)
    t = torch.arange(B * 9, device="cuda", dtype=torch.float32)[:, None] / RATE
    f0 = 100.0 + 4.0 * torch.arange(n, device="cuda", dtype=torch.float32)[None, :]
    for k in range(9):
        x = (0.8 * torch.sin(2 * torch.pi * f0 * t[k * B:(k + 1) * B]) +
             0.05 * torch.randn((B, n), device="cuda", generator=gen)).contiguous()
        y = ge.process(x).clone()
        y_plain = plain.process(x).clone()
        want = rw.process(x).clone()
        got = ge.pitch_tap(500).clone()
        ref.push(want, B)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (plan, k)
        assert torch.equal(y.view(torch.int32), y_plain.view(torch.int32)), (plan, k)
    assert ge.banks[500].windows == 1
    f, c = ge.pitch(500)
    rf, rc = ref.read()
    torch.cuda.synchronize()
    assert torch.equal(f.view(torch.int32), rf.view(torch.int32)) and torch.equal(c.view(torch.int32), rc.view(torch.int32))
    assert (f > 0).sum().item() > n // 2
    ge.set_pitch_param(500, dspfx.PITCH_POWER, 1e9)
    with pytest.raises(KeyError):
        plain.pitch(500)
    for e in (ge, plain, rw):
        e.close()
