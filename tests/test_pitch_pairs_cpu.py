"""The pitch bank's pair-partner tests, the part that needs no GPU: the victims that test_pitch_pairs_gpu.py checks are enough and
all clear of a decision the restatement could lose to rounding, and the partners it seats beside them discriminate -- a float32
model of the PAIRED arithmetic (two channels in one complex FFT, pitch_pairs.paired_r_lin, written from include/dspfx.h's
description) loses the victim to them, and the same arithmetic with each channel scaled by its own power of two does not."""
import numpy as np
import pytest

import pitch_pairs as PP
import pitch_ref as R
from test_pitch_gpu import CLARITY_ATOL, FREQ_RTOL, MARGIN

# (amplitude, power threshold) of the victims of the GPU tests: tests 1 to 3, test 4, test 5 and its outer point
VICTIM_SETS = [(0.3, 0.5), (1e-3, 0.0), (0.3, 0.0), (3e38, 0.0)]


@pytest.mark.parametrize("amplitude,P", VICTIM_SETS)
def test_victim_selection(amplitude, P):
    v = PP.victims(amplitude, P)
    print(f"amplitude {amplitude} P {P}: {len(v.kept)} of {PP.N_CAND} kept, smallest kept margin {v.margin[v.kept].min():.2e}")
    assert 3 * len(v.kept) >= 2 * PP.N_CAND
    assert np.all(v.margin[v.kept] > MARGIN)
    assert np.all(v.found[v.kept])                      # every kept victim has a pitch to lose
    assert not v.win.flags.writeable


def test_seatings_cover_every_kept_victim_at_every_shape():
    kept = PP.victims(0.3).kept
    for n in (16, 77, 160, 64):
        for parity in (0, 1):
            rounds = PP.seatings(n, parity, kept)
            seated = np.concatenate([pick for _, _, pick in rounds])
            assert set(seated) == set(kept), (n, parity)
            for vic, agg, pick in rounds:
                assert len(pick) == len(vic) and np.all(vic % 2 == parity) and np.all(agg % 2 == 1 - parity)
                assert sorted(np.concatenate([vic, agg])) == list(range(n))
    vic, agg, _ = PP.seatings(77, 0, kept)[0]
    assert 76 in vic and 75 in agg                      # channel 76 has no partner: a victim here,
    assert 76 in PP.seatings(77, 1, kept)[0][1]         # an aggressor here


def test_the_restatement_does_not_depend_on_the_level():
    """a power of two is exact in float32 and in float64, so with the power threshold at 0 the restatement gives one answer"""
    v = PP.victims(0.3, 0.0)
    for k in (-100, -40, -20, 20, 40, 100):
        found, tau, freq, clarity, _ = R.detect_bank(PP.scaled(v, k).T.astype(np.float64), 0.0)
        assert np.array_equal(found, v.found) and np.array_equal(tau[found], v.tau[found]), k
        assert np.allclose(freq, v.freq, rtol=1e-9, atol=0) and np.allclose(clarity, v.clarity, rtol=0, atol=1e-9), k


def test_model_alone_stays_within_the_bar():
    """the paired arithmetic itself is good enough: with a silent partner every victim's r is within the clarity bar, and the
    pick on that r is the restatement's"""
    v = PP.victims(0.3)
    silent = np.zeros(R.WINDOW, np.float32)
    worst = 0.0
    for i in v.kept:
        worst = max(worst, PP.victim_error(v.win[:, i], silent))
        r = PP.alias(PP.paired_r_lin(v.win[:, i], silent)[0])
        found, tau, freq, clarity, _ = R.detect(v.win[:, i].astype(np.float64), r=r)
        assert found and tau == v.tau[i]
        assert abs(freq / v.freq[i] - 1.0) <= FREQ_RTOL and abs(clarity - v.clarity[i]) <= CLARITY_ATOL
    print(f"victim alone: worst r_lin error / r(0) {worst:.2e}")
    assert worst < CLARITY_ATOL


@pytest.mark.parametrize("kind", PP.NON_FINITE)
def test_model_a_non_finite_partner_poisons_every_lag(kind):
    v = PP.victims(0.3)
    for i in v.kept[::6]:
        with np.errstate(all="ignore"):
            r0, _, _, _ = PP.paired_r_lin(v.win[:, i], PP.non_finite(kind, 1))
            assert not np.any(np.isfinite(r0)), (kind, i)
            assert not R.detect(v.win[:, i].astype(np.float64), r=PP.alias(r0))[0]      # and the victim's pitch is gone
            # each channel on its own scale, a non-finite one as zeros: as if the partner were silent
            assert PP.victim_error(v.win[:, i], PP.non_finite(kind, 1), own_scale=True) < CLARITY_ATOL


# Partner levels at which the unscaled pairing must lose the victim by ten times the bar.  Level 10 beside 0.3 (a ratio of 33)
# is in test 3 as well but not here: the error grows with the square of the ratio and is AT the bar there (about 9e-5, printed
# below), so that case pins the neighbourhood of the bar, not a failure of the parent.
DISCRIMINATING = [k for k in PP.LOUD if k not in (10.0, "subnormal")]


@pytest.mark.parametrize("kind", PP.LOUD)
def test_model_a_loud_partner_costs_the_victim_its_accuracy(kind):
    v = PP.victims(0.3)
    errs, own = [], []
    for i in v.kept[::6]:
        errs.append(PP.victim_error(v.win[:, i], PP.loud(kind, 1)))
        own.append(PP.victim_error(v.win[:, i], PP.loud(kind, 1), own_scale=True))
    print(f"partner {kind}: r_lin error / r(0) unscaled {np.nanmin(errs) if not np.all(np.isnan(errs)) else np.nan:.2e} .. "
          f"(non-finite: {int(np.isnan(errs).sum())} of {len(errs)}), own scale worst {max(own):.2e}")
    if kind in DISCRIMINATING:
        assert all(not (e < 10 * CLARITY_ATOL) for e in errs), errs            # NaN: the squares overflowed
    if kind == "subnormal":
        assert max(errs) < CLARITY_ATOL                                        # a tiny partner costs nothing either way
    assert max(own) < CLARITY_ATOL


def test_model_a_quiet_channel_beside_a_full_scale_one():
    """test 4's pair: 1e-3 beside 1.0"""
    v = PP.victims(1e-3, 0.0)
    errs = [PP.victim_error(v.win[:, i], PP.loud(1.0, 1)) for i in v.kept[::6]]
    own = [PP.victim_error(v.win[:, i], PP.loud(1.0, 1), own_scale=True) for i in v.kept[::6]]
    print(f"1e-3 beside 1.0: r_lin error / r(0) unscaled {min(errs):.2e} .. {max(errs):.2e}, own scale worst {max(own):.2e}")
    assert min(errs) >= 10 * CLARITY_ATOL
    assert max(own) < CLARITY_ATOL
