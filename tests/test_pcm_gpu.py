"""Device sample formats at the process boundary on the GPU (dspfx_process_pcm / dspfx_process_host_pcm) against the numpy
restatement in pcm_ref.py: exhaustive widening, narrowing edge cases, 2-channel devices, bit-exact parity with the f32 calls
across chains, layouts and paths, the identity format, argument errors."""
import numpy as np
import pytest

from chains import chain3, chain5, fir_taps
from pcm_ref import F32, I16, I32, NP_DTYPE, U16, narrow_np, widen_np

pytestmark = pytest.mark.gpu

B = 128
PAIRS = [(I16, I16), (U16, U16), (I32, I32), (I16, F32)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _dev(torch, a):
    """numpy -> device tensor of the same width (u16 travels as an int16 view; the calls get fmt= for it)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _random_pcm(rng, fmt, shape):
    if fmt == F32:
        return rng.uniform(-1, 1, shape).astype(np.float32)
    info = np.iinfo(NP_DTYPE[fmt])
    return rng.integers(info.min, info.max, shape, endpoint=True, dtype=NP_DTYPE[fmt])


def _pcm_dev(dspfx, torch, eng, x, fmt_in, ch_in, fmt_out, ch_out, side=None, mix=True):
    """one block through dspfx_process_pcm: numpy in, numpy out (+ the f32 bus)"""
    nf = x.shape[0]
    dx = _dev(torch, x)
    ds = _dev(torch, side) if side is not None else None
    dy = torch.empty((nf, eng.channels * ch_out), dtype={F32: torch.float32, I16: torch.int16, U16: torch.int16,
                                                         I32: torch.int32}[fmt_out], device="cuda")
    dm = torch.empty(nf, dtype=torch.float32, device="cuda") if mix else None
    eng.process_pcm(dx, dy, side=ds, mix=dm, in_channels=ch_in, out_channels=ch_out, in_fmt=fmt_in, out_fmt=fmt_out)
    torch.cuda.synchronize()
    return _host(dy, NP_DTYPE[fmt_out]), (dm.cpu().numpy() if mix else None)


def _f32_dev(torch, eng, x, side=None):
    dx = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    ds = torch.from_numpy(np.ascontiguousarray(side, np.float32)).cuda() if side is not None else None
    dy = torch.empty_like(dx)
    dm = torch.empty(x.shape[0], dtype=torch.float32, device="cuda")
    eng.process(dx, out=dy, side=ds, mix=dm)
    torch.cuda.synchronize()
    return dy.cpu().numpy(), dm.cpu().numpy()


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _gain_engine(dspfx, n, frames=1):
    eng = dspfx.Engine(n, frames, link_flags=dspfx.LINK_INTERNAL)     # no hop into the first node rescales
    eng.set_chain([dspfx.Gain(1.0)])
    return eng


def _every_i32_case():
    t = 2 ** 24
    edges = [-2**31, -2**31 + 1, 2**31 - 1, 2**31 - 2, 2**31 - 64, 2**31 - 65, 2**31 - 127, 0, 1, -1]
    ties = [t + k for k in range(-8, 9)] + [-(t + k) for k in range(-8, 9)] + [2 * t + 2, 2 * t + 6, 4 * t + 4, 4 * t + 12]
    spread = np.random.default_rng(5).integers(-2**31, 2**31 - 1, 65536, endpoint=True, dtype=np.int64)
    v = np.concatenate([np.array(edges + ties, np.int64), spread])[:65536]
    return v.astype(np.int32)


def test_exhaustive_widening(dspfx, torch_cuda):
    """Every i16 and every u16 value, one per channel, and a spread of i32 (both extremes, the rounding ties around 2^24)
    through a Gain(1.0) engine to F32 out: v / 32768 (v / 2^31) bit for bit, on the device path and the host path."""
    eng = _gain_engine(dspfx, 65536)
    cases = [(I16, np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)),
             (U16, np.arange(65536, dtype=np.int32).astype(np.uint16)),
             (I32, _every_i32_case())]
    for fmt, v in cases:
        x = v.reshape(1, 65536)
        want = widen_np(x, fmt)
        got, _ = _pcm_dev(dspfx, torch_cuda, eng, x, fmt, 1, F32, 1, mix=False)
        assert np.array_equal(_bits(got), _bits(want)), fmt
        got_h = eng.process_host_pcm(x, out_dtype=np.float32)
        assert np.array_equal(_bits(got_h), _bits(want)), fmt
    # the known answers, on the device
    got, _ = _pcm_dev(dspfx, torch_cuda, eng, np.array([[-32768, 32767] + [0] * 65534], np.int16), I16, 1, F32, 1, mix=False)
    assert got[0, :2].tolist() == [-1.0, 0.999969482421875]


def _narrow_cases():
    f = np.float32
    lsb16, lsb32 = f(1 / 32768), f(2.0 ** -31)
    v = [np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 0.99999, -0.99999, 1.0000001, -1.0000001, 2.0, -2.0, 1e30, -1e30,
         1e-45, -1e-45, 1.17e-38, -1.17e-38, 5.9e-39, -5.9e-39, -1e-5, 1e-5]
    for lsb in (lsb16, lsb32):
        for k in (0.5, 1.5, 2.5, 100.5, 32766.5, 32767.5):
            v += [k * lsb, -k * lsb]
    v += [f(32767.5) * lsb16, f(-32768.5) * lsb16, f(0.5) - lsb32, f(1) - f(2.0 ** -24)]
    x = np.array(v, np.float32)
    rng = np.random.default_rng(11)
    return np.concatenate([x, rng.uniform(-1.5, 1.5, 4096 - len(x)).astype(np.float32)]).reshape(1, 4096)


def test_narrowing_edge_cases(dspfx, torch_cuda):
    """F32 in, I16 / U16 / I32 out: NaN, +-inf, +-0, +-1, 0.99999, 1.0000001, subnormals and values on +-0.5 LSB against
    the restatement, exactly.  (Gain(1.0) hands every value on as it is, or flushes a subnormal, which narrows to 0 either way.)"""
    eng = _gain_engine(dspfx, 4096)
    x = _narrow_cases()
    for fmt in (I16, U16, I32):
        got, _ = _pcm_dev(dspfx, torch_cuda, eng, x, F32, 1, fmt, 1, mix=False)
        assert np.array_equal(got, narrow_np(x, fmt)), fmt
        got_h = eng.process_host_pcm(x, out_dtype=NP_DTYPE[fmt])
        assert np.array_equal(got_h, narrow_np(x, fmt)), fmt


def test_two_channel_devices(dspfx, torch_cuda):
    """2-channel input = a mono run fed to_f32(a) + to_f32(b); 2-channel output = the mono narrowing in both slots."""
    N = 4096 + 3                                  # a ragged width: the rows start off the vector boundary
    rng = np.random.default_rng(3)
    eng = _gain_engine(dspfx, N, 4)
    for fmt in (I16, U16, I32, F32):
        x2 = _random_pcm(rng, fmt, (4, 2 * N))
        got, _ = _pcm_dev(dspfx, torch_cuda, eng, x2, fmt, 2, F32, 1, mix=False)
        mono, _ = _f32_dev(torch_cuda, eng, widen_np(x2, fmt, 2))
        assert np.array_equal(_bits(got), _bits(mono)) and np.array_equal(_bits(got), _bits(widen_np(x2, fmt, 2))), fmt
        xf = rng.uniform(-1.2, 1.2, (4, N)).astype(np.float32)
        got2, _ = _pcm_dev(dspfx, torch_cuda, eng, xf, F32, 1, fmt, 2, mix=False)
        got1, _ = _pcm_dev(dspfx, torch_cuda, eng, xf, F32, 1, fmt, 1, mix=False)
        assert np.array_equal(_bits(got2[:, 0::2]), _bits(got2[:, 1::2])), fmt
        assert np.array_equal(_bits(got2[:, 0::2]), _bits(got1)) and np.array_equal(_bits(got1), _bits(narrow_np(xf, fmt))), fmt


def _chain(dspfx, name):
    if name == "chain5":
        return chain5(dspfx, 512)
    if name == "chain3":
        return chain3(dspfx, 512)
    return [dspfx.BiQuad(), dspfx.Fir(fir_taps(48)), dspfx.Gain(0.7)]        # a FIR stage: the host path's whole-block form


def _engines(dspfx, n, chain, tile, k):
    out = []
    for _ in range(k):
        e = dspfx.Engine(n, B, tile_channels=tile)
        e.set_chain(chain)
        e.kernels_ready()
        out.append(e)
    return out


def _parity(dspfx, torch, chain, N, tile, pinned, seed, blocks):
    """Engine A: dspfx_process on widen_np(x); engine B: the PCM call on x.  `blocks` blocks per format pair, and the state
    carries across blocks and pairs alike: out_B == narrow_np(out_A), mix_B == mix_A, bit for bit."""
    a, b_dev, b_host = _engines(dspfx, N, chain, tile, 3)
    rng = np.random.default_rng(seed)
    bufs = {}
    for fi, fo in PAIRS:
        for ch in (1, 2):
            if pinned:
                key = (fi, fo, ch)
                px = dspfx.PinnedArray((B, N * ch), NP_DTYPE[fi])
                ps = dspfx.PinnedArray((B, N * ch), NP_DTYPE[fi])
                py = dspfx.PinnedArray((B, N * ch), NP_DTYPE[fo])
                bufs[key] = (px, ps, py)
            for blk in range(blocks):
                x = _random_pcm(rng, fi, (B, N * ch))
                side = _random_pcm(rng, fi, (B, N * ch))
                ya, ma = _f32_dev(torch, a, widen_np(x, fi, ch), widen_np(side, fi, ch))
                want = narrow_np(ya, fo, ch)
                where = (fi, fo, ch, blk)
                if pinned:
                    px.array[:], ps.array[:] = x, side
                    yh, mh = b_host.process_host_pcm(px.array, out=py.array, side=ps.array, want_mix=True, in_channels=ch,
                                                     out_channels=ch)
                else:
                    yd, md = _pcm_dev(dspfx, torch, b_dev, x, fi, ch, fo, ch, side=side)
                    assert np.array_equal(_bits(yd), _bits(want)), where
                    assert np.array_equal(_bits(md), _bits(ma)), where
                    yh, mh = b_host.process_host_pcm(x, side=side, want_mix=True, in_channels=ch, out_channels=ch,
                                                     out_dtype=NP_DTYPE[fo])
                assert np.array_equal(_bits(yh), _bits(want)), where
                assert np.array_equal(_bits(mh), _bits(ma)), where
    for e in (a, b_dev, b_host):
        e.close()
    for t in bufs.values():
        for p in t:
            p.close()


@pytest.mark.parametrize("tile", [0, 256])
@pytest.mark.parametrize("name", ["chain5", "chain3", "fir"])
def test_parity_with_the_f32_path(dspfx, torch_cuda, name, tile):
    """device dspfx_process_pcm and dspfx_process_host_pcm from pageable numpy, a few thousand channels"""
    _parity(dspfx, torch_cuda, _chain(dspfx, name), 4096, tile, False, 100 + tile + len(name), 8)


def test_parity_pinned_pipelined(dspfx, torch_cuda):
    """dspfx_process_host_pcm from page-locked buffers at 262144 channels: four channel parts, the pipelined form.  Two blocks
    per format pair (16 in all, the state carried through them): the numpy side of a block of this size is what costs."""
    _parity(dspfx, torch_cuda, _chain(dspfx, "chain5"), 262144, 0, True, 7, 2)


def test_identity_format_is_the_f32_call(dspfx, torch_cuda):
    """{F32, 1, F32, 1} is dspfx_process / dspfx_process_host, bit for bit, state included (4 blocks)."""
    N = 4096 + 64
    chain = chain5(dspfx, 512)
    e_ref, e_pcm, h_ref, h_pcm = _engines(dspfx, N, chain, 0, 4)
    rng = np.random.default_rng(21)
    for _ in range(4):
        x = rng.uniform(-1, 1, (B, N)).astype(np.float32)
        ya, ma = _f32_dev(torch_cuda, e_ref, x)
        yb, mb = _pcm_dev(dspfx, torch_cuda, e_pcm, x, F32, 1, F32, 1)
        assert np.array_equal(_bits(ya), _bits(yb)) and np.array_equal(_bits(ma), _bits(mb))
        yc, mc = h_ref.process_host(x, want_mix=True)
        yd, md = h_pcm.process_host_pcm(x, want_mix=True)
        assert np.array_equal(_bits(yc), _bits(yd)) and np.array_equal(_bits(mc), _bits(md))
        assert np.array_equal(_bits(yc), _bits(ya))


def test_errors_leave_the_engine_working(dspfx, torch_cuda):
    import ctypes as C
    N = 2048
    eng, ref = _engines(dspfx, N, chain3(dspfx, 512), 0, 2)
    L = eng.L
    x = torch_cuda.zeros((B, N), dtype=torch_cuda.int16, device="cuda")
    y = torch_cuda.zeros((B, N), dtype=torch_cuda.int16, device="cuda")
    xp, yp = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())
    hx, hy = np.zeros((B, N), np.int16), np.zeros((B, N), np.int16)
    good = dspfx._PcmIo(I16, 1, I16, 1)
    bad = [dspfx._PcmIo(4, 1, I16, 1), dspfx._PcmIo(I16, 1, -1, 1), dspfx._PcmIo(I16, 3, I16, 1), dspfx._PcmIo(I16, 1, I16, 0)]
    for io in bad + [None]:
        p = C.byref(io) if io is not None else None
        assert L.dspfx_process_pcm(eng.h, p, xp, None, yp, None, B, None) == -1
        assert L.dspfx_process_host_pcm(eng.h, p, hx.ctypes.data, None, hy.ctypes.data, None, B) == -1
        assert L.dspfx_last_error(eng.h).decode()           # the engine's usual error text says why
    assert L.dspfx_process_pcm(eng.h, C.byref(good), xp, None, yp, None, B + 1, None) == -1
    assert L.dspfx_process_host_pcm(eng.h, C.byref(good), hx.ctypes.data, None, hy.ctypes.data, None, B + 1) == -1
    assert L.dspfx_process_pcm(eng.h, C.byref(good), None, None, yp, None, B, None) == -1
    assert L.dspfx_process_pcm(eng.h, C.byref(good), xp, None, None, None, B, None) == -1
    assert L.dspfx_process_host_pcm(eng.h, C.byref(good), None, None, hy.ctypes.data, None, B) == -1
    assert L.dspfx_process_host_pcm(eng.h, C.byref(good), hx.ctypes.data, None, None, None, B) == -1
    rng = np.random.default_rng(9)
    for _ in range(2):
        xi = _random_pcm(rng, I16, (B, N))
        got, gm = _pcm_dev(dspfx, torch_cuda, eng, xi, I16, 1, I16, 1)
        ya, ma = _f32_dev(torch_cuda, ref, widen_np(xi, I16))
        assert np.array_equal(got, narrow_np(ya, I16)) and np.array_equal(_bits(gm), _bits(ma))
