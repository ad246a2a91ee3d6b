"""Level range and edge values through the restatements of the Spectrogram bank and the output resampler bank, without a GPU:
what lets tests/test_spectrum_edge_gpu.py and tests/test_resample_edge_gpu.py lean on them.  The blocks and streams of the two
GPU files are built here, once, and imported there; the class and count assertions those files rely on are made here on the
restatements alone; a CPU float32 FFT with a range-safe magnitude meets the level-range bar at every level, so the bar asks
nothing of the kernel that the reference side cannot do; and a numpy model of the naive magnitude
0.5f * sqrtf(re * re + im * im) misses it at 2^+-70 and 2^+-100, so the GPU test fails a kernel that has that line."""
import functools

import numpy as np
import pytest

import oracle as O
import pcm_ref
import resample_ref as RR
import spectrum_ref as R
from edge_values import classes_present, edge_block, edge_classes, is_subnormal
from test_spectrum_gpu import cpu_f32_error

F = np.float32
U = 2.0 ** -24
FLT_MAX = float(np.finfo(F).max)
FLT_MIN = 2.0 ** -126                                # the smallest normal float
SEED = 0x5EED0E01                                    # edge_block's
B = 128
F32, I16, U16, I32 = 0, 1, 2, 3

# ---- the Spectrogram bank: shared with the GPU half --------------------------------------------------------------------------------
SPEC_SIZES = (128, 512, 8192)                        # one block per window; the node's default; the 128 KiB form
SPEC_SHAPES = [(77, 0), (64, 64)]                    # ragged: the scalar column stores; a whole tile: the vector stores
LEVEL_MAGS = (0, 40, 64, 70, 100)


def level_exponents(N):
    """e[c]: pair j = c // 2 takes the magnitude LEVEL_MAGS[j % 5]; channels 2j and 2j + 1 get opposite signs, and the sign of the
    even one alternates every ten pairs, so every magnitude meets both signs at both halves of a pair"""
    c = np.arange(N)
    j = c // 2
    mag = np.asarray(LEVEL_MAGS)[j % 5]
    return mag * np.where((j // 10) % 2 == 0, 1, -1) * np.where(c % 2 == 0, 1, -1)


def level_base(n, N):
    """[n][N] f32 at level 2^0, as test_spectrum_gpu.families has them: the project's white noise (the hash of dspfx_fill_noise)
    and off-bin sines with per-channel amplitude and phase, five pairs of the one, five of the other.  The sines are rounded to
    multiples of 2^-23 like the noise, so that 2^-100 times any sample is still a normal float and the scaling is exact."""
    rng = np.random.default_rng(n)
    i = np.arange(n, dtype=np.float64)[:, None]
    white = O.noise(0x5EED0001, np.arange(N), np.arange(n))
    m = rng.uniform(1.0, n / 2 - 1.0, N)
    amp = rng.uniform(0.05, 1.0, N)
    ph = rng.uniform(0, 2 * np.pi, N)
    sine = np.round(amp[None, :] * np.sin(2 * np.pi * m[None, :] * i / n + ph[None, :]) * 2.0 ** 23) * 2.0 ** -23
    kind = ((np.arange(N) // 2) // 5) % 2
    return np.where(kind[None, :] == 0, white, sine.astype(F)).astype(F)


def level_block(n, N):
    """-> (base [n][N], e [N], x = base * 2^e exactly).  The conditions of the bank's level range are asserted here: at every
    level 2 n max|x| < FLT_MAX and the peak window product is a normal float."""
    base, e = level_base(n, N), level_exponents(N)
    x = np.ldexp(base, e[None, :]).astype(F)
    assert np.array_equal(np.ldexp(x.astype(np.float64), -e[None, :]), base.astype(np.float64))       # scaled exactly
    assert (2.0 * n * np.abs(x.astype(np.float64)).max(axis=0) < FLT_MAX).all()
    assert (np.abs(R.windowed(x)).max(axis=0) >= FLT_MIN).all()
    return base, e, x


def level_bar(n, x):
    """the rule of test_spectrum_gpu.py on these inputs: min(ceiling(n), 4 E_cpu), E_cpu = a CPU f32 FFT on the same windows"""
    return min(R.ceiling(n), 4.0 * cpu_f32_error(x))


def _doubled_bins(x, window=None):
    """re, im = 2 X[k], k in [0, n/2), rounded to f32 from an f64 FFT of the f32 window product: what bin_norm is handed"""
    spec = np.fft.rfft(R.windowed(x, window).astype(np.float64), axis=0)[:x.shape[0] // 2]
    return (2.0 * spec.real).astype(F), (2.0 * spec.imag).astype(F)


def naive_column(x, window=None):
    """the magnitude the kernel had: 0.5f * sqrtf(re * re + im * im), every step in f32"""
    re, im = _doubled_bins(x, window)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return (F(0.5) * np.sqrt((re * re + im * im).astype(F))).astype(F)


def scaled_column(x, window=None):
    """the range-safe magnitude: one exact power-of-two scale taken from the larger of |re| and |im| (its exponent, kept inside
    [2, 252]), the squares of the scaled components, the root, the half, and the scale back -- every step in f32"""
    re, im = _doubled_bins(x, window)
    big = np.maximum(np.abs(re), np.abs(im))
    eb = np.clip((big.view(np.uint32) >> 23) & 0xFF, 2, 252).astype(np.uint32)
    down, up = ((254 - eb) << 23).astype(np.uint32).view(F), (eb << 23).astype(np.uint32).view(F)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        sr, si = (re * down).astype(F), (im * down).astype(F)
        return ((F(0.5) * np.sqrt((sr * sr + si * si).astype(F))).astype(F) * up).astype(F)


def subnormal_block(n, N):
    """-> (x [n][N], k [N]): channel c holds the constant k 2^-149, k = 1 + c % 7; the window of that test is all ones"""
    k = 1 + np.arange(N) % 7
    return np.tile(np.ldexp(k.astype(np.float64), -149).astype(F), (n, 1)), k


def spectrum_edge_frames(n, N):
    """-> (x [W n][N], plain [W n][N], table, W): the frames of the edge-block test and the same frames with plain noise in the
    edge channels.
      n >= 256  W = 3.  edge_block(N, 3 n, level=1.0) as it is in window 0 (a non-finite class sits in rows [128, 256) only); the
                edge channels are plain noise in rows [n, 3 n); the non-finite channels get in window 1 what the block puts into
                rows [128, 256) for their class: value k at frame n + 3 + 7 k, a tuple in consecutive frames.
      n = 128   W = 5.  The block in rows [128, 512), plain noise around it: the poison is in window 2 alone."""
    ch = np.arange(N)
    if n >= 256:
        W = 3
        x, table = edge_block(N, 3 * n, level=1.0)
        plain = O.noise(SEED, ch, np.arange(3 * n)).copy()
        edge = sorted(table)
        x[n:, edge] = plain[n:, edge]
        classes = edge_classes(1.0)
        for c, name in table.items():
            vals, finite = classes[name]
            if finite:
                continue
            for k, v in enumerate(vals):
                for j, w in enumerate(v if isinstance(v, tuple) else (v,)):
                    x[n + 3 + 7 * k + j, c] = w
    else:
        W = 5
        blk, table = edge_block(N, 3 * n, level=1.0)
        plain = O.noise(SEED, ch, np.arange(W * n)).copy()
        plain[n:4 * n] = O.noise(SEED, ch, np.arange(3 * n))
        x = plain.copy()
        x[n:4 * n] = blk
    return x, plain, table, W


def window_kinds(x, n, W):
    """[W][N] of "nan" / "inf" / "finite": what the f32 window product of each window of each channel holds under the default
    window (a NaN wins: 0 * inf at the Hann window's two zeros is one)"""
    out = np.empty((W, x.shape[1]), dtype=object)
    for w in range(W):
        with np.errstate(invalid="ignore", over="ignore"):
            p = R.windowed(x[w * n:(w + 1) * n])
        out[w] = np.where(np.isnan(p).any(axis=0), "nan", np.where(np.isinf(p).any(axis=0), "inf", "finite"))
    return out


def in_level_range(x, n, W):
    """[W][N] bool: the window is inside the range the bank states -- finite, the peak window product a normal float, and
    2 n max|window * x| below the largest float"""
    out = np.zeros((W, x.shape[1]), bool)
    for w in range(W):
        with np.errstate(invalid="ignore", over="ignore"):
            p = np.abs(R.windowed(x[w * n:(w + 1) * n]).astype(np.float64))
            peak = p.max(axis=0)
            out[w] = np.isfinite(p).all(axis=0) & (peak >= FLT_MIN) & (2.0 * n * peak < FLT_MAX)
    return out


def left_out_expected(n, table, W):
    """which (window, class) pairs of finite data lie outside the level range, by construction: the `large` class wherever the
    block writes it (3.4e38 times a window entry of a few thousandths and more, times 2 n, overflows), and at n = 128 the
    zeros / subnormals channel in the window that is its silent first block (nothing there but subnormals and 2^-126)"""
    wins = [0] if n >= 256 else [1, 2, 3]
    out = {(w, c) for w in wins for c, name in table.items() if name == "large"}
    if n == 128:
        out |= {(1, c) for c, name in table.items() if name == "zeros_subnormals"}
    return out


def zeros_block(n, N):
    """-> (x, inf_pos, inf_neg, minus_zero): noise; +inf at frame 0 of channel 5, -inf at frame n - 1 of channel 10 (the Hann
    window is 0 at both); channel 2 is all -0.0 and channel 3 all +0.0"""
    x = O.noise(SEED, np.arange(N), np.arange(n)).copy()
    x[:, 2] = -0.0
    x[:, 3] = 0.0
    clean = x.copy()
    x[0, 5] = np.inf
    x[n - 1, 10] = -np.inf
    return x, clean, 5, 10


# ---- the resampler bank: shared with the GPU half ----------------------------------------------------------------------------------
RS_SHAPES = [(96, 32, "1"), (77, 0, "1")]            # (N, tile, DSPFX_RESAMPLE_VEC): four channels a lane; one
RS_RATES = (44100, 96000, 8000)
RS_EDGE_FRAMES = 24 * B
RS_CALLBACKS = 40
RS_MIRROR = 480
POISON_PLACES = ("inside", "carried", "warm")
POISON_INF, POISON_NAN = 1, 2                        # the two poisoned channels: one lane's in the four-channel kernel
SUB_NEG0, SUB_BIG, SUB_DC = 5, 6, 7


def per_of(hz):
    return max(1, int(B * hz / 48000))


def n_outs_of(hz):
    """the callback lengths of test_stream_of_callbacks_is_bit_identical: a 2 * per callback stays inside the four slots"""
    per = per_of(hz)
    return [per, per - 1 if per > 1 else 1, per + 3, 1, 2 * per, per]


def ref_stream(x, hz, n_outs, callbacks, slots=4):
    """The restatement fed as test_resample_gpu.stream feeds a Pair: 128-frame blocks while the FIFO has room, then one callback.
    -> [(want [n_out][N] f32 or None on an underrun, frames consumed, frames waiting before the callback)]"""
    N = x.shape[1]
    ref = RR.Resampler(N, hz)
    fifo = np.zeros((0, N), F)
    f, rows = 0, []
    for cb in range(callbacks):
        while len(fifo) + B <= slots * B and f + B <= len(x):
            fifo = np.concatenate([fifo, x[f:f + B]])
            f += B
        want, consumed = ref.callback(fifo, n_outs[cb % len(n_outs)])
        rows.append((want, consumed, len(fifo)))
        if want is not None:
            fifo = fifo[consumed:]
    return rows


class Replay:
    """stands in for a Pair's restatement: the rows of ref_stream, handed out in order (the same stream, computed once)"""

    def __init__(self, rows):
        self.rows, self.k = rows, 0

    def callback(self, waiting, n_out):
        want, consumed, waiting_len = self.rows[self.k]
        self.k += 1
        assert len(waiting) == waiting_len and (want is None or len(want) == n_out)
        return want, consumed


def outputs_of(rows):
    """every frame the restatement made, underruns left out: [frames][N] f32"""
    return np.concatenate([w for w, _, _ in rows if w is not None])


@functools.lru_cache(maxsize=None)
def resample_edge_case(N, hz):
    """-> (x, plain, table, rows of x, rows of plain): edge_block(N, 24 * 128, level=1.0) through 40 callbacks, and the same stream
    with plain noise in the edge channels.  One addition to the block: which sign an infinity leaves with depends on the sign of
    the coefficient it meets, so on the rate, and at 44100 and 8000 Hz the block alone happens to give +inf and NaN but never
    -inf.  The non-finite samples of rows [128, 256) are therefore repeated NEGATED 480 frames later (480 input frames are a whole
    number of phase periods at all three rates: 1 at 96000, 6 at 8000, 160 at 44100), which turns every +inf of the first
    response into a -inf of the second."""
    x, table = edge_block(N, RS_EDGE_FRAMES, level=1.0)
    first = x[B:2 * B]
    x[B + RS_MIRROR:2 * B + RS_MIRROR] = np.where(np.isfinite(first), x[B + RS_MIRROR:2 * B + RS_MIRROR], -first)
    plain = O.noise(SEED, np.arange(N), np.arange(RS_EDGE_FRAMES)).copy()
    n_outs = n_outs_of(hz)
    return x, plain, table, ref_stream(x, hz, n_outs, RS_CALLBACKS), ref_stream(plain, hz, n_outs, RS_CALLBACKS)


def pulled_before(hz, n_outs, callbacks):
    """[callback][output] -> how many source frames the converter has pulled when it makes that output (the ring then holds the
    16 frames before that count); the scalar state alone, so it holds for every stream that does not underrun"""
    r = RR.Resampler(1, hz)
    total, out = 0, []
    for cb in range(callbacks):
        counts = []
        for adv, _, _ in r.plan(n_outs[cb % len(n_outs)]):
            total += adv
            counts.append(total)
        out.append(np.asarray(counts))
    return out


@functools.lru_cache(maxsize=None)
def poison_case(N, hz, place):
    """Noise with one inf, -inf pair (frames p, p + 1 of channel 1) and one NaN (frame p + 3 of channel 2) inside one callback's
    input; six callbacks of `per` frames.
      inside   p = 40 frames into the third callback's input: the poison has left the ring before that callback ends
      carried  p = 6 frames before the end of what the third callback pulls: the ring saved between the calls carries it
      warm     p = 2: the first callback after create, which the warm-up kernel makes (idx < 8)
    -> (x, clean, rows of x, rows of clean, {channel: (first, last poisoned frame)}, pulled_before)"""
    n_outs, callbacks = [per_of(hz)], 6
    clean = O.noise(SEED, np.arange(N), np.arange(8 * B)).copy()
    rows_clean = ref_stream(clean, hz, n_outs, callbacks)
    assert all(w is not None for w, _, _ in rows_clean)
    pulled = pulled_before(hz, n_outs, callbacks)
    assert [int(p[-1]) for p in pulled] == list(np.cumsum([c for _, c, _ in rows_clean]))
    p = {"inside": int(pulled[1][-1]) + 40, "carried": int(pulled[2][-1]) - 6, "warm": 2}[place]
    x = clean.copy()
    x[p, POISON_INF], x[p + 1, POISON_INF], x[p + 3, POISON_NAN] = np.inf, -np.inf, np.nan
    where = {POISON_INF: (p, p + 1), POISON_NAN: (p + 3, p + 3)}
    return x, clean, ref_stream(x, hz, n_outs, callbacks), rows_clean, where, pulled


@functools.lru_cache(maxsize=None)
def subnormal_case(N, hz):
    """Every channel carries k 2^-149, k a random integer in [-512, 512]; channel 5 is all -0.0; channel 6 alternates +-FLT_MAX;
    channel 7 is FLT_MAX in the first six blocks and -FLT_MAX in the last six.  No coefficient of the windowed sinc exceeds 1, so
    no f64 product of a finite sample rounds to an infinity in f32, and the alternating channel -- a tone at the source's Nyquist
    rate, which the left and right taps cancel -- stays finite (it reaches +-FLT_MAX itself at phase 0).  What overflows is the
    f32 SUM of the constant channel: its two largest terms come first and add up to as much as 1.27 FLT_MAX.
    -> (x, rows): 12 blocks through 10 callbacks"""
    k = np.random.default_rng(91).integers(-512, 513, (12 * B, N))
    x = np.ldexp(k.astype(np.float64), -149).astype(F)
    x[:, SUB_NEG0] = -0.0
    x[:, SUB_BIG] = F(FLT_MAX) * np.where(np.arange(len(x)) % 2 == 0, F(1.0), F(-1.0))
    x[:, SUB_DC] = F(FLT_MAX) * np.where(np.arange(len(x)) < 6 * B, F(1.0), F(-1.0))
    return x, ref_stream(x, hz, n_outs_of(hz), 10)


def f32_layout(dspfx, want, tile):
    """[n_out][N] f32 -> the elements of the device buffer in the bank's layout"""
    return dspfx.to_layout(np.ascontiguousarray(want, F), tile).reshape(-1)


# ---- A. the Spectrogram bank's references ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SPEC_SIZES)
def test_level_block_is_inside_what_a_cpu_f32_fft_does(n):
    """At every level of the level-range test a CPU float32 FFT (scipy's, with numpy's range-safe |z|) stays under ceiling(n), per
    channel; so does an exact FFT followed by the scaled f32 magnitude; the naive f32 magnitude is inside the bar up to 2^+-40; at each of
    2^+-70 and 2^+-100, where re * re leaves f32's range, it misses the bar in some channel, at 2^+-100 in every one."""
    N = 77
    base, e, x = level_block(n, N)
    assert set(np.abs(e)) == set(LEVEL_MAGS) and (e[0:76:2] == -e[1:76:2]).all()
    assert {(int(a), int(b)) for a, b in zip(e[0::2], e[1::2])} >= {(m, -m) for m in LEVEL_MAGS} | {(-m, m) for m in LEVEL_MAGS}
    ecpu = cpu_f32_error(x)
    bb = level_bar(n, x)
    ref = R.column(x)
    print(f"n={n}: E_cpu over all levels {ecpu / U:.3f} x 2^-24, ceiling {R.ceiling(n) / U:.0f}, bar {bb / U:.3f}")
    assert ecpu <= R.ceiling(n)
    safe = R.rel_err(scaled_column(x), ref)
    assert (safe <= bb).all(), (safe.max() / U, int(safe.argmax()))
    with np.errstate(invalid="ignore", over="ignore"):
        naive = R.rel_err(naive_column(x), ref)
    for m in LEVEL_MAGS:
        for s in (1, -1):
            sel = e == s * m
            print(f"n={n} e={s * m:+d}: naive {np.nanmax(naive[sel]) / U:.3g} x 2^-24, scaled {safe[sel].max() / U:.3f} x 2^-24")
    assert (naive[np.abs(e) <= 40] <= bb).all()
    for lvl in (70, -70, 100, -100):                           # some channel of each of these levels misses: the GPU test asks for all
        assert not (naive[e == lvl] <= bb).all(), lvl
    assert not (naive[np.abs(e) == 100] <= bb).any()
    # at the level of every other spectrogram test the scale changes no bit
    ordinary = e == 0
    assert np.array_equal(naive_column(x)[:, ordinary].view(np.uint32), scaled_column(x)[:, ordinary].view(np.uint32))


@pytest.mark.parametrize("n", SPEC_SIZES)
def test_subnormal_constant_has_an_exact_column(n):
    """window = ones, x = k 2^-149: bin 0 of the restatement is n k 2^-149 exactly, every other bin is below ceiling(n) times that;
    the scaled magnitude of the exact bins gives those bits, the naive one gives 0 (re * re underflows)."""
    x, k = subnormal_block(n, 77)
    ones = np.ones(n, F)
    ref = R.column(x, ones)
    want = np.ldexp((n * k).astype(np.float64), -149)
    assert np.array_equal(ref[0], want) and (want < FLT_MIN).all()
    assert (ref[1:] <= R.ceiling(n) * want[None, :]).all()
    got = scaled_column(x, ones)
    assert np.array_equal(got[0].astype(np.float64), want) and (got[1:] <= R.ceiling(n) * want[None, :]).all()
    assert not naive_column(x, ones)[0].any()


@pytest.mark.parametrize("N", [77, 64])
@pytest.mark.parametrize("n", SPEC_SIZES)
def test_spectrum_edge_frames_are_what_the_gpu_test_says(n, N):
    x, plain, table, W = spectrum_edge_frames(n, N)
    assert x.shape == plain.shape == (W * n, N)
    others = np.asarray([c for c in range(N) if c not in table])
    assert np.array_equal(x[:, others].view(np.uint32), plain[:, others].view(np.uint32)) and np.isfinite(plain).all()
    kinds = window_kinds(x, n, W)
    poisoned = [1, 0] if n >= 256 else [2]
    for c, name in table.items():
        want = {"nan": "nan", "inf": "inf", "inf_pair": "inf"}.get(name)
        for w in range(W):
            if want is None or w not in poisoned:
                assert kinds[w, c] == "finite", (w, c, name)
            elif n == 128 and name != "nan":
                assert kinds[w, c] == "nan"                    # frame 0 of the block's second 128 frames holds an infinity: 0 * inf
            else:
                assert kinds[w, c] == want, (w, c, name)
    assert (kinds[:, others] == "finite").all()
    # the window after the poison, and at n = 128 the one before it, are plain noise in the non-finite channels
    nonfinite = [c for c, name in table.items() if name in ("nan", "inf", "inf_pair")]
    for w in ([2] if n >= 256 else [1, 3]):
        rows = slice(w * n, (w + 1) * n)
        assert np.array_equal(x[rows][:, nonfinite].view(np.uint32), plain[rows][:, nonfinite].view(np.uint32))
    ok = in_level_range(x, n, W)
    out = {(w, c) for w in range(W) for c in range(N) if kinds[w, c] == "finite" and not ok[w, c]}
    assert out == left_out_expected(n, table, W), sorted(out ^ left_out_expected(n, table, W))
    # the finite windows that are judged: a CPU f32 FFT is under the ceiling there
    for w in range(W):
        sel = np.nonzero(ok[w])[0]
        assert cpu_f32_error(x[w * n:(w + 1) * n][:, sel]) <= R.ceiling(n), w


@pytest.mark.parametrize("n", SPEC_SIZES)
def test_the_hann_zeros_make_nan_of_an_infinity(n):
    x, clean, a, b = zeros_block(n, 77)
    w = R.hann(n)
    assert w[0] == 0.0 and w[n - 1] == 0.0
    with np.errstate(invalid="ignore"):
        p = R.windowed(x)
        assert np.isnan(p[0, a]) and np.isnan(p[n - 1, b]) and np.isnan(p).sum() == 2 and not np.isinf(p).any()
        col = R.column(x)
    assert np.isnan(col[:, [a, b]]).all()
    rest = [c for c in range(77) if c not in (a, b)]
    assert np.array_equal(col[:, rest], R.column(clean)[:, rest])
    assert not R.column(clean)[:, [2, 3]].any() and np.signbit(x[:, 2]).all()


# ---- B. the resampler bank's restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hz", RS_RATES)
@pytest.mark.parametrize("N", [96, 77])
def test_resample_edge_stream_classes(N, hz):
    """The restatement's f32 output of the edge stream holds NaN, both infinities and subnormals; every integer format holds both
    saturation values; a NaN becomes 0 (I16, I32) or 0x8000 (U16); the channels outside the table are those of the plain stream
    bit for bit (the restatement is elementwise over channels)."""
    x, plain, table, rows, rows_plain = resample_edge_case(N, hz)
    assert sum(w is not None for w, _, _ in rows) >= 12 and [r[1:] for r in rows] == [r[1:] for r in rows_plain]
    out, out_plain = outputs_of(rows), outputs_of(rows_plain)
    assert {"nan", "+inf", "-inf", "subnormal"} <= classes_present(out), classes_present(out)
    assert np.isfinite(out_plain).all()
    others = np.asarray([c for c in range(N) if c not in table])
    assert np.array_equal(out[:, others].view(np.uint32), out_plain[:, others].view(np.uint32))
    nan = np.isnan(out)
    for fmt, lo, hi, zero in ((I16, -32768, 32767, 0), (U16, 0, 65535, 0x8000), (I32, -2 ** 31, 2 ** 31 - 1, 0)):
        dev = pcm_ref.narrow_np(out, fmt, 1)
        assert (dev == lo).any() and (dev == hi).any(), fmt
        assert (dev[nan] == zero).all() and nan.sum() >= 10, fmt
    assert np.array_equal(pcm_ref.narrow_np(out, I16, 2), np.repeat(pcm_ref.narrow_np(out, I16, 1), 2, axis=-1))


@pytest.mark.parametrize("place", POISON_PLACES)
@pytest.mark.parametrize("hz", RS_RATES)
def test_poison_leaves_the_restatement_with_the_ring(hz, place):
    """From the first output whose 16-frame ring no longer holds a poisoned frame the restatement is finite and equals the clean
    stream bit for bit; in steady state every output whose ring holds one is not finite in that channel (all 16 entries are read);
    the two placements are what their names say."""
    N = 77
    x, clean, rows, rows_clean, where, pulled = poison_case(N, hz, place)
    assert [r[1:] for r in rows] == [r[1:] for r in rows_clean]
    out, out_clean = outputs_of(rows), outputs_of(rows_clean)
    P = np.concatenate(pulled)
    cb_of = np.concatenate([np.full(len(p), k) for k, p in enumerate(pulled)])
    last = max(b for _, b in where.values())
    gone = P - RR.TAPS > last
    assert gone.any() and np.isfinite(out[gone]).all()
    assert np.array_equal(out[gone].view(np.uint32), out_clean[gone].view(np.uint32))
    rest = [c for c in range(N) if c not in where]
    assert np.array_equal(out[:, rest].view(np.uint32), out_clean[:, rest].view(np.uint32))
    for c, (a, b) in where.items():
        holds = (P > a) & (P - RR.TAPS <= b)
        steady = holds & (P >= RR.DEPTH)
        assert steady.any() and not np.isfinite(out[steady, c]).any(), c
        before = P <= a
        assert np.array_equal(out[before, c].view(np.uint32), out_clean[before, c].view(np.uint32))
    entered = int(cb_of[np.argmax(P > min(a for a, _ in where.values()))])
    first_gone = int(cb_of[np.argmax(gone)])
    if place == "carried":
        assert first_gone == entered + 1 == 3
    else:
        assert first_gone == entered == (2 if place == "inside" else 0)


@pytest.mark.parametrize("hz", RS_RATES)
@pytest.mark.parametrize("N", [96, 77])
def test_subnormal_stream_through_the_restatement(N, hz):
    x, rows = subnormal_case(N, hz)
    special = [SUB_NEG0, SUB_BIG, SUB_DC]
    assert is_subnormal(np.delete(x, special, axis=1)).mean() > 0.99
    out = outputs_of(rows)
    assert len(out) > 4 * per_of(hz) and not np.isnan(out).any()
    nz = out[out != 0]
    assert is_subnormal(nz).mean() > 0.5, is_subnormal(nz).mean()
    assert (out[:, SUB_NEG0].view(np.uint32) == 0).all()
    assert np.isfinite(out[:, SUB_BIG]).all() and np.abs(out[:, SUB_BIG]).max() > 1e38
    if hz == 8000:                                             # 48000 / 8000 = 6: the phase is always 0, an output is one source frame
        assert np.isfinite(out[:, SUB_DC]).all() and np.abs(out[:, SUB_DC]).max() == FLT_MAX
    else:
        assert np.isposinf(out[:, SUB_DC]).any() and np.isneginf(out[:, SUB_DC]).any()
    rest = np.delete(out, special, axis=1)
    assert (np.abs(rest) < FLT_MIN).all() and (rest != 0).mean() > 0.9


def test_replay_hands_out_the_rows_in_order():
    x, rows = subnormal_case(77, 8000)
    r = Replay(rows)
    want, consumed, waiting = rows[0]
    got = r.callback(np.zeros((waiting, 77), F), len(want))
    assert got[0] is want and got[1] == consumed
    with pytest.raises(AssertionError):
        r.callback(np.zeros((rows[1][2] + 1, 77), F), len(rows[1][0]))
