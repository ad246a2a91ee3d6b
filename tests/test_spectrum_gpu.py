"""The Spectrogram bank on the GPU (dspfx_spectrum_*) against the float64 restatement in spectrum_ref.py, through the C ABI like
the other banks: accuracy for the seven sizes in both layouts against a bar taken from a CPU float32 FFT in the same test;
exact structure (impulse, constant, on-bin cosine, the Hann triple); channel independence; the
window / history bookkeeping for any push length; the slot path; the gain table; an Engine writing into a bank; graph
taps in each plan; one column at 2^20 channels, timed.

The measure is e = ||v_gpu - v_ref||_2 / ||v_ref||_2 per channel over a column.  Two conditions on its worst value:
  1. e <= (7 log2 n + 4) 2^-24: what no correct f32 FFT exceeds (spectrum_ref.ceiling);
  2. e <= 4 E_cpu(n), E_cpu(n) = the worst e of scipy.fft.rfft run in float32 on the same windowed inputs (three families,
     N = 512) against the same f64 reference.  The 4 covers the difference in radix and twiddle strategy between two correct
     f32 FFTs and the two extra roundings of the magnitude.
bar(n) below is the smaller of the two."""
import json

import numpy as np
import pytest
import scipy.fft

import spectrum_ref as R

pytestmark = pytest.mark.gpu

B = 128
N_ACC = 512
U = 2.0 ** -24


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _noise(dspfx, torch, frames, n_ch, seed=0x5EED0001):
    """the project's white noise (dspfx_fill_noise), [frames][n_ch] float32 on the host"""
    eng = dspfx.Engine(n_ch, B)
    eng.set_chain([dspfx.Gain(1.0)])
    x = torch.empty((B, n_ch), dtype=torch.float32, device="cuda")
    out = []
    for k in range((frames + B - 1) // B):
        eng.fill_noise(x, B, k * B, seed)
        torch.cuda.synchronize()
        out.append(x.cpu().numpy().copy())
    eng.close()
    return np.concatenate(out)[:frames]


def families(dspfx, torch, n, n_ch=N_ACC):
    """the three input families of the accuracy check, each [n][n_ch] float32"""
    rng = np.random.default_rng(n)
    i = np.arange(n, dtype=np.float64)[:, None]
    white = _noise(dspfx, torch, n, n_ch)
    m = rng.uniform(1.0, n / 2 - 1.0, n_ch)                   # off-bin: a fractional number of cycles per window
    amp = rng.uniform(0.05, 1.0, n_ch)
    ph = rng.uniform(0, 2 * np.pi, n_ch)
    sine = (amp[None, :] * np.sin(2 * np.pi * m[None, :] * i / n + ph[None, :])).astype(np.float32)
    dc = (np.float32(0.9) + np.float32(1e-3) * _noise(dspfx, torch, n, n_ch, seed=0x5EED0002)).astype(np.float32)
    return {"white": white, "sine": sine, "dc": dc}


def cpu_f32_error(x, window=None):
    """the worst e of scipy.fft.rfft in float32 on the windowed input, against the f64 reference"""
    xw = R.windowed(x, window)
    spec = scipy.fft.rfft(xw, axis=0)
    assert spec.dtype == np.complex64
    v = np.abs(spec)[:x.shape[0] // 2]
    return float(R.rel_err(v, R.column(x, window)).max())


_E_CPU = {}


def e_cpu(dspfx, torch, n):
    if n not in _E_CPU:
        _E_CPU[n] = max(cpu_f32_error(x) for x in families(dspfx, torch, n).values())
    return _E_CPU[n]


def bar(dspfx, torch, n):
    return min(R.ceiling(n), 4.0 * e_cpu(dspfx, torch, n))


def push_all(dspfx, torch, bank, x, sizes=None):
    """push frame-major numpy x [frames][N] in the bank's layout, in pushes of `sizes` (cycled; default: 128-frame blocks)"""
    frames, f, k = x.shape[0], 0, 0
    sizes = sizes or [B]
    while f < frames:
        nf = min(sizes[k % len(sizes)], frames - f)
        bank.push(torch.from_numpy(dspfx.to_layout(x[f:f + nf], bank.tile_channels)).cuda(), nf)
        f += nf
        k += 1


def read_column(dspfx, torch, bank, age=0):
    """-> [n/2][N] float32 on the host, or None"""
    col = bank.column(age)
    if col is None:
        return None
    torch.cuda.synchronize()
    return dspfx.from_layout(col.cpu().numpy(), bank.fft_size // 2, bank.channels, bank.tile_channels).copy()


def one_column(dspfx, torch, x, tile=0, **kw):
    bank = dspfx.SpectrumBank(x.shape[1], fft_size=x.shape[0], tile_channels=tile, **kw)
    push_all(dspfx, torch, bank, x)
    assert bank.windows == 1
    v = read_column(dspfx, torch, bank)
    bank.close()
    return v


@pytest.mark.parametrize("tile", [0, 256])
@pytest.mark.parametrize("n", R.SIZES)
def test_accuracy_against_the_f64_restatement(dspfx, torch_cuda, n, tile):
    torch = torch_cuda
    fam = families(dspfx, torch, n)
    ecpu = e_cpu(dspfx, torch, n)
    worst = 0.0
    for name, x in fam.items():
        v = one_column(dspfx, torch, x, tile)
        e = R.rel_err(v, R.column(x))
        print(f"n={n} tile={tile} {name}: worst e = {e.max() / U:.3f} x 2^-24 (channel {int(e.argmax())}), "
              f"CPU f32 rfft {cpu_f32_error(x) / U:.3f} x 2^-24")
        worst = max(worst, float(e.max()))
    print(f"n={n} tile={tile}: GPU worst e = {worst / U:.3f} x 2^-24, E_cpu = {ecpu / U:.3f} x 2^-24, ceiling {R.ceiling(n) / U:.0f} x 2^-24")
    assert worst <= R.ceiling(n)
    assert worst <= 4.0 * ecpu


@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("n", R.SIZES)
def test_exact_structure(dspfx, torch_cuda, n, tile):
    """A permuted, mirrored or mis-scaled output cannot pass these."""
    torch = torch_cuda
    bb = bar(dspfx, torch, n)
    n_ch = 64
    ones = np.ones(n, np.float32)
    i = np.arange(n)
    # impulses at different frames: every bin is 1
    x = np.zeros((n, n_ch), np.float32)
    where = (np.arange(n_ch) * 37 + 1) % n
    x[where, np.arange(n_ch)] = 1.0
    v = one_column(dspfx, torch, x, tile, window=ones)
    e = R.rel_err(v, np.ones((n // 2, n_ch)))
    print(f"n={n} impulse: e = {e.max() / U:.3f} x 2^-24, worst bin off by {np.abs(v - 1.0).max() / U:.3f} x 2^-24")
    assert e.max() <= bb
    # constants c = 1 .. 7 (n c < 2^24: every partial sum is exact)
    c = (1 + np.arange(n_ch) % 7).astype(np.float32)
    v = one_column(dspfx, torch, np.tile(c, (n, 1)), tile, window=ones)
    assert np.all(np.abs(v[0] - n * c) <= bb * n * c)
    assert np.all(v[1:] <= bb * n * c[None, :])
    # a cosine on bin m: n/2 there and nothing elsewhere
    m = 2 + (np.arange(n_ch) * 29) % (n // 2 - 4)              # 2 <= m <= n/2 - 3: the triple m - 1, m, m + 1 is clear of bin 0's mirror
    x = np.cos(2 * np.pi * m[None, :] * i[:, None] / n).astype(np.float32)
    v = one_column(dspfx, torch, x, tile, window=ones)
    peak = v[m, np.arange(n_ch)]
    assert np.all(np.abs(peak - n / 2) <= bb * n / 2), np.abs(peak / (n / 2) - 1).max()
    rest = v.copy()
    rest[m, np.arange(n_ch)] = 0.0
    assert rest.max() <= bb * n / 2, (rest.max(), bb * n / 2)
    assert np.array_equal(v.argmax(axis=0), m)
    # the default window: the Hann triple at m - 1, m, m + 1, as the restatement has it
    v = one_column(dspfx, torch, x, tile)
    ref = R.column(x)
    assert R.rel_err(v, ref).max() <= bb
    assert np.array_equal(v.argmax(axis=0), m)
    top3 = np.sort(np.argsort(v, axis=0)[-3:], axis=0)
    assert np.array_equal(top3, np.stack([m - 1, m, m + 1]))


@pytest.mark.parametrize("n_ch,tile", [(77, 0), (64, 64), (9, 0)])
@pytest.mark.parametrize("n", [128, 512, 4096, 8192])
def test_channel_independence(dspfx, torch_cuda, n, n_ch, tile):
    """Channels 2j and 2j + 1 carry unrelated signals, one 100 times the other: each column is what it is with the partner
    silent.  Every channel has a transform of its own, so this holds bit for bit (and so within the bar); a silent channel's
    column is exactly zero.  Odd N in the frame-major layout, N equal to the tile in the tiled one."""
    torch = torch_cuda
    bb = bar(dspfx, torch, n)
    rng = np.random.default_rng(n + n_ch)
    x = rng.uniform(-1.0, 1.0, (n, n_ch)).astype(np.float32)
    x[:, 1::2] *= np.float32(1e-2)
    x[:, 3::4] = (0.007 * np.sin(2 * np.pi * 11.3 * np.arange(n) / n))[:, None].astype(np.float32)
    both = one_column(dspfx, torch, x, tile)
    even_only, odd_only = x.copy(), x.copy()
    even_only[:, 1::2] = 0.0
    odd_only[:, 0::2] = 0.0
    ve = one_column(dspfx, torch, even_only, tile)
    vo = one_column(dspfx, torch, odd_only, tile)
    ref = R.column(x)
    e = R.rel_err(both, ref)
    print(f"n={n} N={n_ch} tile={tile}: worst e = {e.max() / U:.3f} x 2^-24 (loud {e[0::2].max() / U:.3f}, quiet {e[1::2].max() / U:.3f})")
    assert e.max() <= bb
    assert R.rel_err(ve[:, 0::2], ref[:, 0::2]).max() <= bb and R.rel_err(vo[:, 1::2], ref[:, 1::2]).max() <= bb
    assert np.array_equal(both[:, 0::2].view(np.uint32), ve[:, 0::2].view(np.uint32))
    assert np.array_equal(both[:, 1::2].view(np.uint32), vo[:, 1::2].view(np.uint32))
    assert not ve[:, 1::2].any() and not vo[:, 0::2].any()


@pytest.mark.parametrize("n,tile", [(128, 0), (256, 64), (1024, 0), (1024, 32)])
def test_bookkeeping_for_any_push_length(dspfx, torch_cuda, n, tile):
    torch = torch_cuda
    n_ch = 128
    sizes = [1, 127, 128, 129, n - 1, n, n + 1, 3 * n + 5]
    total = sum(sizes)
    x = np.random.default_rng(n).uniform(-1.0, 1.0, (total, n_ch)).astype(np.float32)
    n_win = total // n
    a = dspfx.SpectrumBank(n_ch, fft_size=n, columns=n_win, tile_channels=tile)
    b = dspfx.SpectrumBank(n_ch, fft_size=n, columns=n_win, tile_channels=tile)
    host = R.HostBank(n_ch, n, columns=n_win)
    assert a.windows == 0 and a.column(0) is None and a.slot() is not None
    f = 0
    for s in sizes:
        before = f // n
        push_all(dspfx, torch, a, x[f:f + s], [s])
        host.push(x[f:f + s])
        f += s
        assert a.windows == f // n == host.windows             # window w appears exactly when n (w + 1) frames are in
        assert (a.slot() is not None) == (f % B == 0)
        assert (a.column(0) is not None) == (f >= n)
        assert a.column(f // n) is None
        if f // n > before:
            got = read_column(dspfx, torch, a)
            assert R.rel_err(got, host.column(0)).max() <= bar(dspfx, torch, n)
    push_all(dspfx, torch, b, x)                               # the same frames, one push per 128-frame block
    assert b.windows == n_win
    for age in range(n_win):
        va, vb = read_column(dspfx, torch, a, age), read_column(dspfx, torch, b, age)
        assert np.array_equal(va.view(np.uint32), vb.view(np.uint32)), age      # the same kernel on the same data
        assert R.rel_err(va, host.column(age)).max() <= bar(dspfx, torch, n)
    assert a.column(n_win) is None


@pytest.mark.parametrize("tile", [0, 64])
def test_history_reset_and_the_slot_path(dspfx, torch_cuda, tile):
    torch = torch_cuda
    n, n_ch, cols = 256, 256, 3
    bb = bar(dspfx, torch, n)
    x = np.random.default_rng(5).uniform(-1.0, 1.0, (5 * n, n_ch)).astype(np.float32)
    a = dspfx.SpectrumBank(n_ch, fft_size=n, columns=cols, tile_channels=tile)
    s = dspfx.SpectrumBank(n_ch, fft_size=n, columns=cols, tile_channels=tile)
    seen = []
    for w in range(5):
        for k in range(n // B):
            blk = torch.from_numpy(dspfx.to_layout(x[w * n + k * B:w * n + (k + 1) * B], tile)).cuda()
            a.push(blk, B)
            slot = s.slot_tensor()                             # the slot path: written in place, nothing copied
            assert slot is not None
            slot.copy_(blk.reshape(-1))
            s.push(slot, B)
        assert a.windows == s.windows == w + 1
        seen.append(a.column(0).data_ptr())
        for age in range(cols + 1):
            va = read_column(dspfx, torch, a, age)
            if age > w or age >= cols:
                assert va is None and s.column(age) is None
                continue
            vs = read_column(dspfx, torch, s, age)
            assert np.array_equal(va.view(np.uint32), vs.view(np.uint32))
            assert R.rel_err(va, R.column(x[(w - age) * n:(w - age + 1) * n])).max() <= bb
    assert seen[3] == seen[0] and seen[4] == seen[1] and len(set(seen[:3])) == 3    # overwritten `columns` windows later
    first = read_column(dspfx, torch, dspfx.SpectrumBank(n_ch, fft_size=n, tile_channels=tile), 0)
    assert first is None
    s.push(torch.zeros(5 * n_ch, device="cuda"), 5)
    assert s.slot() is None and s.slot_tensor() is None        # not on a slot boundary
    import ctypes as C
    L = dspfx.lib()
    assert L.dspfx_spectrum_push(a.h, C.c_void_p(a.slot()), 64, None) == -1     # the slot takes whole blocks
    assert L.dspfx_spectrum_push(a.h, C.c_void_p(a.slot()), 0, None) == -1
    assert L.dspfx_spectrum_push(a.h, None, 128, None) == -1
    # reset: the state after create
    for bank in (a, s):
        bank.reset()
        assert bank.windows == 0 and bank.column(0) is None and bank.slot() is not None
    push_all(dspfx, torch, a, x[:n + 5])
    fresh = dspfx.SpectrumBank(n_ch, fft_size=n, columns=cols, tile_channels=tile)
    push_all(dspfx, torch, fresh, x[:n + 5])
    assert a.windows == 1 and a.column(1) is None
    assert np.array_equal(read_column(dspfx, torch, a).view(np.uint32), read_column(dspfx, torch, fresh).view(np.uint32))
    assert a.column(0).data_ptr() == seen[0]


@pytest.mark.parametrize("n,tile", [(128, 0), (512, 256), (2048, 0), (8192, 256)])
def test_gain_table_is_one_f32_multiply(dspfx, torch_cuda, n, tile):
    torch = torch_cuda
    rng = np.random.default_rng(n)
    x = rng.uniform(-1.0, 1.0, (n, 256)).astype(np.float32)
    gain = rng.uniform(0.25, 4.0, n // 2).astype(np.float32)
    unit = one_column(dspfx, torch, x, tile)
    ones = one_column(dspfx, torch, x, tile, gain=np.ones(n // 2, np.float32))
    scaled = one_column(dspfx, torch, x, tile, gain=gain)
    assert np.array_equal(unit.view(np.uint32), ones.view(np.uint32))
    want = unit * gain[:, None]                                # f32 * f32, rounded once
    assert want.dtype == np.float32
    assert np.array_equal(scaled.view(np.uint32), want.view(np.uint32))
    # and a caller's window table replaces the default
    win = rng.uniform(0.0, 1.0, n).astype(np.float32)
    v = one_column(dspfx, torch, x, tile, window=win)
    assert R.rel_err(v, R.column(x, window=win)).max() <= bar(dspfx, torch, n)


def test_engine_output_into_a_bank(dspfx, torch_cuda):
    """Engine.process writes straight into the bank's slot; the columns are the restatement's on the chain's own output."""
    from dsp_stuff_amd import workloads
    torch = torch_cuda
    n, n_ch = 512, 512
    eng = dspfx.Engine(n_ch, B, link_flags=3)
    eng.set_chain(workloads.chain5(dspfx, delay=300))
    bank = dspfx.SpectrumBank(n_ch, fft_size=n, columns=4)
    x = torch.empty((B, n_ch), dtype=torch.float32, device="cuda")
    outs = []
    for k in range(4 * n // B):
        eng.fill_noise(x, B, k * B)
        slot = bank.slot_tensor()
        eng.process(x, out=slot.view(B, n_ch))
        bank.push(slot, B)
        outs.append(slot.view(B, n_ch).cpu().numpy().copy())
    assert bank.windows == 4
    y = np.concatenate(outs)
    assert np.abs(y).max() > 0.01
    for age in range(4):
        w = 3 - age
        e = R.rel_err(read_column(dspfx, torch, bank, age), R.column(y[w * n:(w + 1) * n]))
        assert e.max() <= bar(dspfx, torch, n), (age, e.max() / U)


def _tap_docs(dspfx, fft_size=256, with_pitch=False):
    """A chain whose Spectrogram node reads two links (the biquad in the middle of the chain and the gain), and the same
    document with those two links rewired into the Output node instead of the high-pass."""
    from dsp_stuff_amd import config
    chain = [dspfx.BiQuad(1.0, -1.8, 0.81, 0.0025, 0.005, 0.0025), dspfx.Gain(0.5), dspfx.HighPass(0.2)]
    doc = json.loads(config.dump_dspconfig(chain))
    bq, gain, out = doc["nodes"][1], doc["nodes"][2], doc["nodes"][4]
    srcs = [[bq["id"], bq["cfg"]["outputs"]["out"]], [gain["id"], gain["cfg"]["outputs"]["out"]]]
    rewired = json.loads(json.dumps(doc))
    doc["nodes"].append({"id": 500, "typename": "spectrogram", "position": [0, 0],
                         "cfg": {"id": 500, "inputs": {"in": 600}, "buffer_size": 100, "fft_size": fft_size, "upper_bound": 20000,
                                 "lower_bound": 20}})
    doc["links"] += [{"lhs": s, "rhs": [500, 600]} for s in srcs]
    if with_pitch:
        doc["nodes"].append({"id": 510, "typename": "pitch", "position": [0, 0],
                             "cfg": {"id": 510, "inputs": {"in": 610}, "outputs": {}, "power_thresh": 0.3, "clarity_thresh": 0.6,
                                     "pick_thresh": 0.8}})
        doc["links"] += [{"lhs": s, "rhs": [510, 610]} for s in srcs]
    into_out = [k for k, l in enumerate(rewired["links"]) if l["rhs"][0] == out["id"]]
    port = rewired["links"][into_out[0]]["rhs"]
    rewired["links"] = [l for k, l in enumerate(rewired["links"]) if k not in into_out] + [{"lhs": s, "rhs": port} for s in srcs]
    return json.dumps(doc), json.dumps(rewired)


def _blocks(torch, n_ch, count, seed=71):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(B * count, device="cuda", dtype=torch.float32)[:, None] / 48000.0
    f0 = 100.0 + 4.0 * torch.arange(n_ch, device="cuda", dtype=torch.float32)[None, :]
    for k in range(count):
        yield (0.8 * torch.sin(2 * torch.pi * f0 * t[k * B:(k + 1) * B]) +
               0.05 * torch.randn((B, n_ch), device="cuda", generator=gen)).contiguous()


@pytest.mark.parametrize("plan", ["fused", "regions", "runs"])
def test_graph_spectrum_tap_is_the_rewired_output(dspfx, torch_cuda, plan):
    """GraphEngine(spectrum=True): the tap is bit-identical to the same links rewired into the Output node, in each plan; the
    Output block itself is unchanged; the bank holds what a SpectrumBank fed with the rewired output holds."""
    from dsp_stuff_amd.graph import GraphEngine
    torch = torch_cuda
    n_ch, n = 256, 256
    doc, rewired = _tap_docs(dspfx, n)
    kw = {"fused": dict(), "regions": dict(regions=True), "runs": dict(fused=False)}[plan]
    ge = GraphEngine(doc, n_ch, **kw, spectrum=True, spectrum_columns=2)
    plain = GraphEngine(doc, n_ch, **kw)
    rw = GraphEngine(rewired, n_ch, **kw)
    if plan == "fused":
        assert ge.fused is not None and rw.fused is not None
    elif plan == "regions":
        assert ge.regions and rw.regions
    else:
        assert ge.runs and ge.fused is None and not ge.regions
    ref = dspfx.SpectrumBank(n_ch, fft_size=n, columns=2)
    assert ge.spectrum(500) is None
    fed = []
    for k, x in enumerate(_blocks(torch, n_ch, 2 * n // B)):
        y = ge.process(x).clone()
        y_plain = plain.process(x).clone()
        want = rw.process(x).clone()
        got = ge.spectrum_tap(500).clone()
        ref.push(want, B)
        torch.cuda.synchronize()
        fed.append(want.view(B, n_ch).cpu().numpy().copy())
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (plan, k)
        assert torch.equal(y.view(torch.int32), y_plain.view(torch.int32)), (plan, k)
    assert ge.spectra[500].windows == 2 and ge.spectra[500].fft_size == n
    fed = np.concatenate(fed)
    for age in (0, 1):
        a, b = ge.spectrum(500, age), ref.column(age)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        w = 1 - age
        assert R.rel_err(a.view(n // 2, n_ch).cpu().numpy(), R.column(fed[w * n:(w + 1) * n])).max() <= bar(dspfx, torch, n)
    assert ge.spectrum(500, 2) is None
    with pytest.raises(KeyError):
        plain.spectrum(500)
    with pytest.raises(KeyError):
        ge.spectrum(1)
    with pytest.raises(KeyError):
        ge.pitch(500)
    for e in (ge, plain, rw):
        e.close()


def test_graph_pitch_and_spectrum_taps_coexist(dspfx, torch_cuda):
    from dsp_stuff_amd import config
    from dsp_stuff_amd.graph import GraphEngine
    torch = torch_cuda
    n_ch, n = 256, 512
    doc, rewired = _tap_docs(dspfx, n, with_pitch=True)
    ge = GraphEngine(doc, n_ch, pitch=True, spectrum=True)
    only_pitch = GraphEngine(doc, n_ch, pitch=True)
    rw = GraphEngine(rewired, n_ch)
    assert ge.fused is not None and ge.tap_ids == [510, 500]
    ref_s = dspfx.SpectrumBank(n_ch, fft_size=n)
    ref_p = dspfx.PitchBank(n_ch, power_thresh=0.3, clarity_thresh=0.6, pick_thresh=0.8)
    for k, x in enumerate(_blocks(torch, n_ch, 9)):
        y = ge.process(x).clone()
        y_p = only_pitch.process(x).clone()
        want = rw.process(x).clone()
        ref_s.push(want, B)
        ref_p.push(want, B)
        torch.cuda.synchronize()
        assert torch.equal(ge.spectrum_tap(500).view(torch.int32), want.view(torch.int32)), k
        assert torch.equal(ge.pitch_tap(510).view(torch.int32), want.view(torch.int32)), k
        assert torch.equal(y.view(torch.int32), y_p.view(torch.int32)), k
    assert ge.banks[510].windows == 1 and ge.spectra[500].windows == 2
    f, c = ge.pitch(510)
    rf, rc = ref_p.read()
    f2, c2 = only_pitch.pitch(510)
    torch.cuda.synchronize()
    assert torch.equal(f.view(torch.int32), rf.view(torch.int32)) and torch.equal(c.view(torch.int32), rc.view(torch.int32))
    assert torch.equal(f.view(torch.int32), f2.view(torch.int32)) and (f > 0).sum().item() > n_ch // 2
    assert torch.equal(ge.spectrum(500).view(torch.int32), ref_s.column(0).view(torch.int32))
    with pytest.raises(KeyError):
        only_pitch.spectrum(500)
    # a saved size the bank does not take: only spectrum=True minds
    odd, _ = _tap_docs(dspfx, 1000)
    GraphEngine(odd, n_ch).close()
    with pytest.raises(config.DspConfigError, match="fft_size 1000"):
        GraphEngine(odd, n_ch, spectrum=True)
    for e in (ge, only_pitch, rw):
        e.close()


def test_full_size_one_column(dspfx, torch_cuda):
    """2^20 channels, fft_size 512, tiled: 64 sampled channels against the restatement, and the time of one column launch
    (HIP events, median of 20 after 5 warm-ups, alternating between two banks' window stores of 2.5 GiB each, so the 256 MiB
    Infinity Cache cannot hold a window between launches).  Correctness is asserted; the time is printed."""
    torch = torch_cuda
    n_ch, n, tile = 1 << 20, 512, 256
    rng = np.random.default_rng(61)
    sample = np.sort(rng.choice(n_ch, 64, replace=False))
    base = rng.uniform(-1.0, 1.0, (2 * n, 256)).astype(np.float32)    # channel c carries base[:, c % 256] times its own gain
    gain = (0.5 + (np.arange(n_ch) % 7) / 7.0).astype(np.float32)
    src = torch.from_numpy(base).cuda()
    g = torch.from_numpy(gain).cuda()
    idx = torch.arange(n_ch, device="cuda") % 256
    banks = [dspfx.SpectrumBank(n_ch, fft_size=n, columns=1, tile_channels=tile) for _ in range(2)]
    for bank in banks:
        for k in range(2 * n // B):                            # two windows: every slot of the store has been written
            blk = src[k * B:(k + 1) * B][:, idx] * g[None, :]                   # [128][N] frame-major
            slot = bank.slot_tensor()
            slot.view(n_ch // tile, B, tile).copy_(blk.view(B, n_ch // tile, tile).permute(1, 0, 2))
            bank.push(slot, B)
            if (k + 1) * B % n == 0:
                w = (k + 1) * B // n - 1
                col = bank.column(0)
                torch.cuda.synchronize()
                got = col.view(n_ch // tile, n // 2, tile).permute(1, 0, 2).reshape(n // 2, n_ch)[:, torch.from_numpy(sample).cuda()]
                x = base[w * n:(w + 1) * n][:, sample % 256] * gain[None, sample]
                e = R.rel_err(got.cpu().numpy(), R.column(x))
                print(f"2^20 channels, window {w}: worst e of 64 sampled channels = {e.max() / U:.3f} x 2^-24")
                assert e.max() <= bar(dspfx, torch, n)
        assert bank.windows == 2
    times = []
    for it in range(25):
        bank = banks[it % 2]
        for k in range(n // B - 1):
            bank.push(bank.slot_tensor(), B)                   # in place: no copy, no launch
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        slot = bank.slot_tensor()
        t0.record()
        bank.push(slot, B)                                     # completes a window: exactly one column launch
        t1.record()
        torch.cuda.synchronize()
        if it >= 5:
            times.append(t0.elapsed_time(t1))
    ms = float(np.median(times))
    floor_bytes = (n * 4 + n // 2 * 4) * n_ch
    print(f"2^20 channels, fft_size 512, tiled {tile}: one column launch {ms:.3f} ms median of {len(times)} "
          f"(min {min(times):.3f}, max {max(times):.3f}); {floor_bytes / ms / 1e9:.2f} TB/s of the {floor_bytes / 2 ** 30:.1f} GiB "
          f"floor; a window lasts {n / B * 128 / 48.0:.3f} ms")
    assert banks[0].windows == 2 + 13 and banks[1].windows == 2 + 12
