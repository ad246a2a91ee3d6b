"""The Pitch Detector bank on the GPU: a channel's result depends on its own window alone.  pitch_detect transforms channels 2j
and 2j + 1 as one complex signal, so every test here seats victims (sines and sawtooths the float64 restatement is sure of,
pitch_pairs.victims) on one parity of the channels and a partner that paired arithmetic cannot stand on the other -- non-finite
samples, levels up to the largest float, a full-scale channel beside one 60 dB down -- and asks of every victim what
test_pitch_gpu.py asks (its `_parity` rule and its bars, against pitch_ref.detect on the victim's own window), with no channel
skipped: the victims were chosen by their margin beforehand, on the CPU (test_pitch_pairs_cpu.py shows that they are enough and
that these partners break a pairing that does not keep the channels apart).
Shapes: the smallest that reach each load path of the kernel -- even N (one 8-byte load per pair, a grid of 8: the XCD remap), odd
N (scalar loads; channel 76 has no partner), tiled with a grid of 80, tiled with N equal to the tile."""
import numpy as np
import pytest

import pitch_pairs as PP
import pitch_ref as R
from test_pitch_gpu import CLARITY_ATOL, FREQ_RTOL, MARGIN, RATE, _push, _read, torch_cuda  # noqa: F401  (torch_cuda: a fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(16, 0), (77, 0), (160, 32), (64, 64)]


def _victims(amplitude, P=0.5):
    v = PP.victims(amplitude, P, margin_bar=MARGIN)
    assert 3 * len(v.kept) >= 2 * PP.N_CAND, len(v.kept)
    return v


def _reference(win, P=0.5):
    """the restatement on float32 windows [1024][n] -> (found, tau, freq, clarity)"""
    return R.detect_bank(win.T.astype(np.float64), P)[:4]


def _match(got_f, got_c, ref, prev=None, what=""):
    """test_pitch_gpu._parity's rule on EVERY channel given, against a reference computed beforehand: the found / not found
    decision (a channel without a result keeps `prev`, zeros at first), the chosen integer lag, frequency within FREQ_RTOL and
    clarity within CLARITY_ATOL.  -> (worst frequency error, worst clarity error)"""
    found, tau, freq, clarity = ref
    pf = np.zeros_like(freq) if prev is None else prev[0].astype(np.float64)
    pc = np.zeros_like(clarity) if prev is None else prev[1].astype(np.float64)
    got_found = got_f != pf
    assert np.array_equal(got_found, found), (what, "found differs at", np.nonzero(got_found != found)[0])
    assert np.array_equal(got_f[~found], pf[~found]) and np.array_equal(got_c[~found], pc[~found]), what
    lag = np.abs(RATE / got_f[found].astype(np.float64) - tau[found])
    assert np.all(lag <= 0.5 + 1e-3), (what, "lag off by", lag.max(), "at", np.nonzero(found)[0][np.argmax(lag)])
    ferr = np.abs(got_f[found] / freq[found] - 1.0)
    cerr = np.abs(got_c[found] - clarity[found])
    assert ferr.max(initial=0) <= FREQ_RTOL, (what, "frequency", ferr.max(), "at", np.nonzero(found)[0][np.argmax(ferr)])
    assert cerr.max(initial=0) <= CLARITY_ATOL, (what, "clarity", cerr.max(), "at", np.nonzero(found)[0][np.argmax(cerr)])
    return float(ferr.max(initial=0)), float(cerr.max(initial=0))


def _ref_of(v, pick):
    return v.found[pick], v.tau[pick], v.freq[pick], v.clarity[pick]


def _one_window(dspfx, torch, bank, win):
    """a fresh start, window `win` [1024][N] and the frame that makes it fall due -> freq[N], clarity[N]"""
    bank.reset()
    _push(dspfx, torch, bank, np.concatenate([win, np.zeros((1, win.shape[1]), np.float32)]))
    assert bank.windows == 1
    return _read(torch, bank)


def _beside(dspfx, torch, bank, n, v, partner, what):
    """every kept victim beside partner(channel) on both parities; the victims must match -> the worst errors"""
    worst = (0.0, 0.0)
    for parity in (0, 1):
        for vic, agg, pick in PP.seatings(n, parity, v.kept):
            win = np.empty((R.WINDOW, n), np.float32)
            win[:, vic] = v.win[:, pick]
            for c in agg:
                win[:, c] = partner(int(c))
            f, c = _one_window(dspfx, torch, bank, win)
            worst = np.maximum(worst, _match(f[vic], c[vic], _ref_of(v, pick), what=(what, "victims on parity", parity)))
            yield f[agg], c[agg]
    print(f"{what}: victims' worst freq rel err {worst[0]:.2e}, clarity abs err {worst[1]:.2e}")


@pytest.mark.parametrize("n,tile", SHAPES)
def test_a_non_finite_partner_silences_itself_only(dspfx, torch_cuda, n, tile):
    v = _victims(0.3)
    bank = dspfx.PitchBank(n, tile_channels=tile)
    for kind in PP.NON_FINITE:
        for fa, ca in _beside(dspfx, torch_cuda, bank, n, v, lambda c: PP.non_finite(kind, c), f"n={n} tile={tile} {kind}"):
            assert not fa.any() and not ca.any(), kind                  # the aggressors read (0, 0)


@pytest.mark.parametrize("n,tile", SHAPES)
def test_poison_in_one_window_only(dspfx, torch_cuda, n, tile):
    """Three windows; the aggressors are clean in windows 0 and 2 and non-finite in window 1, where they hold window 0's result.
    Every channel carries a kept victim in every window, another one each time."""
    torch = torch_cuda
    v = _victims(0.3)
    bank = dspfx.PitchBank(n, tile_channels=tile)
    for parity in (0, 1):
        for vic, agg, pick in PP.seatings(n, parity, v.kept):
            at = np.empty((3, n), int)                                   # the candidate on each channel in each window
            for w in range(3):
                at[w, vic] = np.roll(v.kept, -5 * w)[np.searchsorted(v.kept, pick)]
                at[w, agg] = v.kept[(agg + 11 + 13 * w) % len(v.kept)]
            x = np.concatenate([v.win[:, at[w]] for w in range(3)] + [np.zeros((1, n), np.float32)])
            for c in agg:
                kind = PP.NON_FINITE[(c // 2) % len(PP.NON_FINITE)]
                bad = PP.non_finite(kind, int(c))
                x[R.WINDOW:2 * R.WINDOW, c] = np.where(np.isfinite(bad), x[R.WINDOW:2 * R.WINDOW, c], bad)
            bank.reset()
            _push(dspfx, torch, bank, x[:R.WINDOW + 1])
            f0, c0 = _read(torch, bank)
            assert bank.windows == 1
            _match(f0, c0, _ref_of(v, at[0]), what="window 0")
            _push(dspfx, torch, bank, x[R.WINDOW + 1:2 * R.WINDOW + 1])
            f1, c1 = _read(torch, bank)
            assert bank.windows == 2
            _match(f1[vic], c1[vic], _ref_of(v, at[1, vic]), prev=(f0[vic], c0[vic]), what="window 1, victims")
            assert np.array_equal(f1[agg], f0[agg]) and np.array_equal(c1[agg], c0[agg])      # held from window 0
            assert np.all(f1[vic] != f0[vic])
            _push(dspfx, torch, bank, x[2 * R.WINDOW + 1:])
            f2, c2 = _read(torch, bank)
            assert bank.windows == 3
            _match(f2, c2, _ref_of(v, at[2]), prev=(f1, c1), what="window 2")
            assert np.all(f2 != f1)


@pytest.mark.parametrize("n,tile", SHAPES)
def test_a_loud_or_tiny_finite_partner_changes_nothing(dspfx, torch_cuda, n, tile):
    v = _victims(0.3)
    bank = dspfx.PitchBank(n, tile_channels=tile)
    for kind in PP.LOUD:
        for _ in _beside(dspfx, torch_cuda, bank, n, v, lambda c: PP.loud(kind, c), f"n={n} tile={tile} partner {kind}"):
            pass


@pytest.mark.parametrize("n,tile", SHAPES)
def test_a_quiet_channel_beside_a_full_scale_one(dspfx, torch_cuda, n, tile):
    """The case a host can meet: the power threshold lowered to 0, a channel at 1e-3 beside one at 1.0."""
    v = _victims(1e-3, P=0.0)
    bank = dspfx.PitchBank(n, tile_channels=tile)
    bank.set_param(dspfx.PITCH_POWER, 0.0)
    for fa, _ in _beside(dspfx, torch_cuda, bank, n, v, lambda c: PP.loud(1.0, c), f"n={n} tile={tile} 1e-3 beside 1.0"):
        assert fa.all()                                                  # the loud ones do have a pitch


@pytest.mark.parametrize("n,tile", SHAPES)
def test_own_level_range(dspfx, torch_cuda, n, tile):
    """The header's level range: with the power threshold at 0 the result does not depend on the window's level, for every level
    whose max |x| is a normal float.  Every channel is a victim here, scaled by 2^k (exact): all alike, then the two of a pair
    by opposite k; then the far ends (2^+-100, and 3e38 as a level that is no power of two) beside an unscaled partner.  The
    restatement's margin of the SCALED window is not consulted: its only level-dependent part is |power - 0|, and a sum of
    squares cannot round below 0; the victims were kept by the margins that do not depend on the level."""
    torch = torch_cuda
    v = _victims(0.3, P=0.0)
    top = _victims(3e38, P=0.0)
    bank = dspfx.PitchBank(n, tile_channels=tile)
    bank.set_param(dspfx.PITCH_POWER, 0.0)
    ch = np.arange(n)
    worst = (0.0, 0.0)
    for r in range(-(-len(v.kept) // n)):
        pick = v.kept[(r * n + ch) % len(v.kept)]
        for k in (-40, -20, 0, 20, 40):
            for k_odd in (k, -k):
                kk = np.where(ch % 2 == 0, k, k_odd)
                win = np.ldexp(v.win[:, pick], kk[None, :]).astype(np.float32)
                ref = _reference(win, 0.0)
                # the restatement on the scaled window is the unscaled one's answer
                assert np.array_equal(ref[0], v.found[pick]) and np.array_equal(ref[1], v.tau[pick])
                f, c = _one_window(dspfx, torch, bank, win)
                worst = np.maximum(worst, _match(f, c, ref, what=("level", k, k_odd)))
                worst = np.maximum(worst, _match(f, c, _ref_of(v, pick), what=("level, the unscaled answer", k, k_odd)))
    # the far ends: a result there too (every finite normal level), and the partner stays correct
    both = np.intersect1d(v.kept, top.kept)
    assert 3 * len(both) >= 2 * PP.N_CAND
    for parity in (0, 1):
        for vic, agg, pick in PP.seatings(n, parity, both):
            mate = both[(agg // 2 + 7) % len(both)]
            for far in (100, -100, "3e38"):
                win = np.empty((R.WINDOW, n), np.float32)
                win[:, vic] = top.win[:, pick] if far == "3e38" else np.ldexp(v.win[:, pick], far)
                win[:, agg] = v.win[:, mate]
                f, c = _one_window(dspfx, torch, bank, win)
                ref = _ref_of(top, pick) if far == "3e38" else _ref_of(v, pick)
                worst = np.maximum(worst, _match(f[vic], c[vic], ref, what=("far level", far, "parity", parity)))
                worst = np.maximum(worst, _match(f[agg], c[agg], _ref_of(v, mate), what=("partner of far level", far, parity)))
    print(f"n={n} tile={tile}: levels 2^-100 .. 3e38, worst freq rel err {worst[0]:.2e}, clarity abs err {worst[1]:.2e}")
