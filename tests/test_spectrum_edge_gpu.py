"""The Spectrogram bank on the GPU at the edges of its input range, against spectrum_ref.py: each channel's own level from 2^-100
to 2^100 beside a neighbour 200 octaves away; subnormal input; NaN and infinities in one window of one channel, with the windows
and the channels around them; the Hann window's two zeros under an infinity; negative zeros.  The blocks, and what the references
do with them, are in test_edge_output_banks_cpu.py.

Sizes 128 (a window is one block), 512 (the node's default) and 8192 (the 128 KiB form, the largest sums); shapes (N, tile) =
(77, 0), ragged, which takes the scalar column stores, and (64, 64), which takes the vector stores.  The measure and the bar are
those of test_spectrum_gpu.py: e = ||v_gpu - v_ref||_2 / ||v_ref||_2 per channel, at most min(ceiling(n), 4 E_cpu) with E_cpu a CPU
float32 FFT on the same inputs."""
import numpy as np
import pytest

import spectrum_ref as R
from test_edge_output_banks_cpu import (FLT_MIN, LEVEL_MAGS, SPEC_SHAPES, SPEC_SIZES, in_level_range, left_out_expected, level_bar,
                                        level_block, spectrum_edge_frames, subnormal_block, window_kinds, zeros_block)
from test_spectrum_gpu import cpu_f32_error, one_column, push_all, read_column

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def columns_of(dspfx, torch, x, n, tile, W):
    """push W windows, keep W columns -> [W][n/2][N], oldest first"""
    bank = dspfx.SpectrumBank(x.shape[1], fft_size=n, columns=W, tile_channels=tile)
    push_all(dspfx, torch, bank, x)
    assert bank.windows == W
    cols = [read_column(dspfx, torch, bank, W - 1 - w) for w in range(W)]
    bank.close()
    return np.stack(cols)


@pytest.mark.parametrize("N,tile", SPEC_SHAPES)
@pytest.mark.parametrize("n", SPEC_SIZES)
def test_own_level_range(dspfx, torch_cuda, n, N, tile):
    """Channel c carries white noise or an off-bin sine scaled exactly by 2^e[c], e through 0, +-40, +-64, +-70, +-100 with
    channels 2j and 2j + 1 at opposite signs: neighbours in one lane group and one LDS row sit up to 200 octaves apart.  Every
    channel is inside the bar against the f64 column of its own scaled window, and its column is, bit for bit, the column of the
    same data at 2^0 times 2^e wherever that product is exact in f32, at every level down to 2^-70 (the reason is at the check).
    (level_block asserts the range conditions: 2 n max|x| < FLT_MAX and a normal peak window product at every level.)"""
    torch = torch_cuda
    base, e, x = level_block(n, N)
    bb = level_bar(n, x)
    got = one_column(dspfx, torch, x, tile)
    err = R.rel_err(got, R.column(x))
    worst = {}
    for m in LEVEL_MAGS:
        for s in ((1, -1) if m else (1,)):
            sel = e == s * m
            worst[s * m] = float(np.nanmax(np.where(np.isnan(err[sel]), np.inf, err[sel])))
    print(f"n={n} N={N} tile={tile}: bar {bb / U:.3f} x 2^-24 (E_cpu {cpu_f32_error(x) / U:.3f}, ceiling {R.ceiling(n) / U:.0f}); worst e "
          "per level, x 2^-24: " + ", ".join(f"2^{lvl:+d}: {w / U:.3g}" for lvl, w in worst.items()))
    bad = np.nonzero(~(err <= bb))[0]
    assert not len(bad), (f"{len(bad)} channels miss the bar of {bb / U:.3f} x 2^-24; the first: channel {bad[0]} at 2^{e[bad[0]]:+d} "
                          f"with e = {err[bad[0]] / U:.4g} x 2^-24; worst per level {({k: round(v / U, 3) for k, v in worst.items()})}")
    # The same bits as at 2^0, times 2^e.  Scaling by a power of two commutes with every f32 operation that neither overflows
    # nor rounds in the subnormals.  Nothing overflows (2 n max|x| < FLT_MAX); a term that underflows changes a bit of a sum
    # only if it lies within that sum's 24 bits.  So the check is made for the channels in which everything down to 2^-48 of
    # the peak window product -- two f32 significands below it -- is still a normal float: every level down to 2^-70.  At
    # 2^-100 terms only 2^-26 below the peak are subnormal, a handful of bins round differently (12 of the 28 672 bins of the
    # seven 2^-100 channels at n = 8192, N = 77; none at 128 and 512), and only the bar above is asked.
    unit = one_column(dspfx, torch, base, tile)
    peak = np.abs(R.windowed(x).astype(np.float64)).max(axis=0)
    scales = peak * 2.0 ** -48 >= FLT_MIN
    assert np.array_equal(scales, e >= -70)
    assert np.array_equal(R.windowed(x)[:, scales].astype(np.float64), np.ldexp(R.windowed(base).astype(np.float64), e[None, :])[:, scales])
    want = np.ldexp(unit.astype(np.float64), e[None, :])
    with np.errstate(over="ignore", under="ignore"):
        exact = np.isfinite(want) & (want.astype(np.float32).astype(np.float64) == want)
    assert exact[:, scales].all()
    same = bits(got) == bits(want.astype(np.float32))
    check = exact & scales[None, :]
    print(f"n={n} N={N} tile={tile}: bit equality with the column at 2^0 times 2^e: {int((same & check).sum())} of {int(check.sum())} bins "
          f"checked; at 2^-100, not checked: {int(same[:, e == -100].sum())} of {int(same[:, e == -100].size)}")
    assert same[check].all(), (int((~same & check).sum()), sorted(set(int(v) for v in e[np.nonzero((~same & check).any(axis=0))[0]])))


@pytest.mark.parametrize("N,tile", SPEC_SHAPES)
@pytest.mark.parametrize("n", SPEC_SIZES)
def test_subnormal_input_is_not_flushed(dspfx, torch_cuda, n, N, tile):
    """window = ones and the constant k 2^-149 per channel, k = 1 + c % 7.  Read through fft_core.hip.h, every step of that chain
    is exact: the window product is 1 * x; the first pass has no twiddles and leaves 4 k 2^-149 (twice, re and im) at every
    fourth point and zeros elsewhere; every later butterfly either adds such multiples under the w^0 twiddle (1, -0), whose
    products are x * 1 and x * 0, or sees zeros only; no sum exceeds 2 n k < 2^24 units.  Bin 0 reaches the magnitude as re =
    2 n k 2^-149, im = 0, and the scaled squares, the root and the scale back are exact for k < 8.  So bin 0 is n k 2^-149
    exactly, and every other bin is below ceiling(n) times that (it is 0)."""
    torch = torch_cuda
    x, k = subnormal_block(n, N)
    got = one_column(dspfx, torch, x, tile, window=np.ones(n, np.float32))
    want = np.ldexp((n * k).astype(np.float64), -149)
    print(f"n={n} N={N} tile={tile}: bin 0 / 2^-149 = {np.unique(got[0].astype(np.float64) * 2.0 ** 149)[:8]}, "
          f"largest other bin / 2^-149 = {float(got[1:].max()) * 2.0 ** 149:.3g}")
    assert (want < FLT_MIN).all()
    assert np.array_equal(got[0].astype(np.float64), want), np.nonzero(got[0] != want)[0][:8]
    assert (got[1:] >= 0).all() and (got[1:] <= R.ceiling(n) * want[None, :]).all()


@pytest.mark.parametrize("N,tile", SPEC_SHAPES)
@pytest.mark.parametrize("n", SPEC_SIZES)
def test_edge_block_neighbours_and_single_windows(dspfx, torch_cuda, n, N, tile):
    """The frames of spectrum_edge_frames: at n >= 256 three windows, the edge block in the first (its non-finite classes sit in
    rows [128, 256)), the same poison once more in the second and plain noise in the third; at n = 128 five windows with the
    poison in the middle one.  Per window and channel, by what the f32 window product holds:
      a NaN        every bin is NaN (at n = 128 the infinities' channels too: the block starts on one, under the window's 0);
      an infinity  every bin is NaN or +inf;
      finite       inside the bar of the f64 column of that window -- zeros and subnormals, the clip points, the switch
                   points -- unless the window is outside the bank's level range: the `large` class wherever the block writes
                   3.4e38, and at n = 128 the zeros / subnormals channel's silent first block; which those are is asserted.
    No bin anywhere is negative or -inf.  Against a run in which the edge channels carried plain noise: every channel outside
    the table, in every window, and every window of an edge channel that holds plain noise (the window after the poison; at
    n = 128 also the one before it) has the same bits."""
    torch = torch_cuda
    x, plain, table, W = spectrum_edge_frames(n, N)
    got = columns_of(dspfx, torch, x, n, tile, W)
    clean = columns_of(dspfx, torch, plain, n, tile, W)
    assert np.isfinite(clean).all()
    kinds, ok = window_kinds(x, n, W), in_level_range(x, n, W)
    with np.errstate(invalid="ignore"):
        assert not (got < 0).any() and not np.isneginf(got).any()
    left_out = set()
    for w in range(W):
        rows = slice(w * n, (w + 1) * n)
        nan, inf, fin = (np.nonzero(kinds[w] == k)[0] for k in ("nan", "inf", "finite"))
        assert np.isnan(got[w][:, nan]).all(), (w, [table.get(c) for c in nan if not np.isnan(got[w][:, c]).all()])
        assert (np.isnan(got[w][:, inf]) | np.isposinf(got[w][:, inf])).all(), w
        left_out |= {(w, int(c)) for c in fin if not ok[w, c]}
        judged = np.asarray([c for c in fin if ok[w, c]])
        bb = min(R.ceiling(n), 4.0 * cpu_f32_error(x[rows][:, judged]))
        err = R.rel_err(got[w][:, judged], R.column(x[rows][:, judged]))
        print(f"n={n} N={N} tile={tile} window {w}: {len(nan)} NaN, {len(inf)} inf, {len(judged)} judged channels, worst e = "
              f"{err.max() / U:.3f} x 2^-24 (channel {judged[int(err.argmax())]}, {table.get(int(judged[int(err.argmax())]), 'noise')}), "
              f"bar {bb / U:.3f}")
        assert (err <= bb).all(), (w, [(int(c), table.get(int(c), "noise")) for c in judged[~(err <= bb)]])
        same_input = (bits(x[rows]) == bits(plain[rows])).all(axis=0)
        assert same_input.sum() >= N - len(table)
        assert np.array_equal(bits(got[w][:, same_input]), bits(clean[w][:, same_input])), w
    assert left_out == left_out_expected(n, table, W)
    nonfinite = [c for c, name in table.items() if name in ("nan", "inf", "inf_pair")]
    for w in ([2] if n >= 256 else [1, 3]):                    # the windows next to the poison: compared just above
        assert (kinds[w, nonfinite] == "finite").all() and (bits(x[w * n:(w + 1) * n][:, nonfinite]) == bits(plain[w * n:(w + 1) * n][:, nonfinite])).all()
    for w in ([0, 1] if n >= 256 else [2]):
        assert (kinds[w, nonfinite] != "finite").all()


@pytest.mark.parametrize("N,tile", SPEC_SHAPES)
@pytest.mark.parametrize("n", SPEC_SIZES)
def test_the_windows_zeros_multiply_and_zeros_stay_plus_zero(dspfx, torch_cuda, n, N, tile):
    """Under the default Hann window, +inf at frame 0 of channel 5 and -inf at frame n - 1 of channel 10: window[0] = window[n - 1]
    = 0, the product is NaN (the restatement's too), and both columns are NaN in every bin; every other channel, the four
    between them included, keeps the bits of the run without the infinities.  A channel of -0.0 samples and one of +0.0 samples
    have columns of +0.0 bits."""
    torch = torch_cuda
    x, clean, a, b = zeros_block(n, N)
    with np.errstate(invalid="ignore"):
        p = R.windowed(x)
    assert np.isnan(p[0, a]) and np.isnan(p[n - 1, b])
    got, base = one_column(dspfx, torch, x, tile), one_column(dspfx, torch, clean, tile)
    assert np.isnan(got[:, [a, b]]).all()
    rest = np.asarray([c for c in range(N) if c not in (a, b)])
    assert np.isfinite(base).all() and np.array_equal(bits(got[:, rest]), bits(base[:, rest]))
    assert np.signbit(x[:, 2]).all() and not bits(got[:, [2, 3]]).any()
    assert R.rel_err(base[:, 4:], R.column(clean[:, 4:])).max() <= min(R.ceiling(n), 4.0 * cpu_f32_error(clean[:, 4:]))
