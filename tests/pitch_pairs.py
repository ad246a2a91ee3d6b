"""Inputs of the pitch bank's pair-partner tests (test_pitch_pairs_cpu.py, test_pitch_pairs_gpu.py), all plain numpy on the CPU:
the victim windows and which of them the restatement's margin keeps, the partners that share a workgroup with them, how the two
are seated on the channels of a bank, and a float32 model of the PAIRED arithmetic (two channels in one complex FFT) that shows
which partners such arithmetic cannot stand.  pitch_kernels.hip puts channels 2j and 2j + 1 into one workgroup."""
import functools
from types import SimpleNamespace

import numpy as np

import pitch_ref as R

N_CAND = 48
NON_FINITE = ("one_nan", "plus_inf", "minus_inf", "inf_pair", "all_nan")
# test 3's partners: an unrelated sine plus noise at these peak levels, the largest float in every frame, subnormals only
LOUD = (10.0, 1e2, 1e4, 1e10, 1e19, 3e38, "flt_max", "subnormal")
F32_MAX = float(np.finfo(np.float32).max)


def candidates(amplitude, frames=R.WINDOW):
    """[frames][48] float32: sines, every third a sawtooth, 100 to 2000 Hz in geometric steps, fixed phases, peak `amplitude`."""
    f = np.geomspace(100.0, 2000.0, N_CAND)[None, :]
    ph = (0.3 + 0.7 * np.arange(N_CAND))[None, :]
    t = np.arange(frames)[:, None] / R.RATE
    x = np.sin(2 * np.pi * f * t + ph)
    saw = 2.0 * ((f * t + ph / (2 * np.pi)) % 1.0) - 1.0
    x[:, 2::3] = saw[:, 2::3]
    return (amplitude * x).astype(np.float32)


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def victims(amplitude, P=0.5, C=0.5, K=0.5, margin_bar=1e-4):
    """The candidates at `amplitude` with the restatement's answer for each (float64, on the float32 window), computed once and
    shared read-only.  `kept`: the candidates whose margin exceeds `margin_bar` -- the restatement alone decides."""
    win = candidates(amplitude)
    found, tau, freq, clarity, margin = R.detect_bank(win.T.astype(np.float64), P, C, K)
    return SimpleNamespace(win=_frozen(win), found=_frozen(found), tau=_frozen(tau), freq=_frozen(freq), clarity=_frozen(clarity),
                           margin=_frozen(margin), kept=_frozen(np.nonzero(margin > margin_bar)[0]), P=P, C=C, K=K)


def scaled(v, k):
    """v.win times 2^k, exact in float32 while nothing leaves the normal range"""
    return np.ldexp(v.win, k).astype(np.float32)


def seatings(n, parity, kept):
    """Victims on the channels of `parity`, partners on the others, in as many rounds as it takes to seat every kept candidate
    once (a round that has seats left over starts the list again).  -> [(victim channels, partner channels, candidate of each
    victim channel)]"""
    vic = np.arange(parity, n, 2)
    agg = np.arange(1 - parity, n, 2)
    rounds = -(-len(kept) // len(vic))
    return [(vic, agg, kept[(r * len(vic) + np.arange(len(vic))) % len(kept)]) for r in range(rounds)]


def _tone(channel, frames=R.WINDOW):
    """a sine unrelated to any candidate, different on every channel, peak 0.85"""
    t = np.arange(frames) / R.RATE
    return 0.85 * np.sin(2 * np.pi * (131.0 + 37.0 * (channel % 41)) * t + 0.11 * channel)


def non_finite(kind, channel):
    """[1024] float32: a clean tone that would give a result, with the non-finite samples of `kind` in it"""
    x = (0.5 * _tone(channel)).astype(np.float32)
    if kind == "one_nan":
        x[500] = np.nan
    elif kind == "plus_inf":
        x[500] = np.inf
    elif kind == "minus_inf":
        x[500] = -np.inf
    elif kind == "inf_pair":
        x[500], x[501] = np.inf, -np.inf
    elif kind == "all_nan":
        x[:] = np.nan
    else:
        raise ValueError(kind)
    return x


def loud(kind, channel):
    """[1024] float32, finite: a tone plus noise of peak level `kind` (|tone + noise| <= 1 before the scaling, so 3e38 stays
    finite), or one of the two named windows"""
    if kind == "flt_max":
        return np.full(R.WINDOW, F32_MAX, np.float32)
    rng = np.random.default_rng(1000 + channel)
    s = _tone(channel) + 0.15 * rng.uniform(-1.0, 1.0, R.WINDOW)
    if kind == "subnormal":
        x = (s * 2.0 ** -130).astype(np.float32)
        assert np.all(np.abs(x) < np.finfo(np.float32).tiny) and x.any()
        return x
    x = (s * float(kind)).astype(np.float32)
    assert np.all(np.isfinite(x))
    return x


# ---- the paired arithmetic, in float32 --------------------------------------------------------------------------------------
def _own_power_of_two(x):
    """x / 2^e with e the exponent of max|x| (exact); zeros for a non-finite window"""
    if not np.all(np.isfinite(x)) or not np.any(x):
        return np.zeros_like(x), 0
    e = int(np.frexp(np.float64(np.abs(x).max()))[1])
    return np.ldexp(x.astype(np.float64), -e).astype(np.float32), e


def paired_r_lin(x0, x1, own_scale=False):
    """Both channels' linear autocorrelations r_lin(0..1023), computed as one complex pair in torch complex64, written from
    include/dspfx.h's description: z = x0 + i x1 zero-padded to 2048; Z = FFT(z); X0 = (Z + conj Z(-k)) / 2,
    X1 = (Z - conj Z(-k)) / 2i; IFFT(|X0|^2 + i |X1|^2) = r_lin0 + i r_lin1.  own_scale: each channel is first divided by its
    own power of two (zeros for a non-finite one) and r_lin comes back in that scale.  -> (r_lin0, r_lin1, e0, e1), float64
    copies of the float32 results."""
    import torch
    x0, x1 = np.asarray(x0, np.float32), np.asarray(x1, np.float32)
    e0 = e1 = 0
    if own_scale:
        x0, e0 = _own_power_of_two(x0)
        x1, e1 = _own_power_of_two(x1)
    z = torch.zeros(2048, dtype=torch.complex64)
    z[:R.SIZE] = torch.complex(torch.from_numpy(x0.copy()), torch.from_numpy(x1.copy()))
    Z = torch.fft.fft(z)
    Zm = torch.conj(torch.roll(torch.flip(Z, [0]), 1))          # conj Z(-k)
    a, b = Z + Zm, Z - Zm                                       # 2 X0, 2i X1
    p = torch.complex(a.real * a.real + a.imag * a.imag, b.real * b.real + b.imag * b.imag)
    r = torch.fft.ifft(p) / 4.0
    return (r.real[:R.SIZE].double().numpy(), r.imag[:R.SIZE].double().numpy(), e0, e1)


def alias(r_lin):
    """r(tau) = r_lin(tau) + r_lin(1536 - tau) for tau > 512, as pitch_ref.autocorr"""
    r = np.array(r_lin, np.float64)
    t = np.arange(R.PADDING + 1, R.SIZE)
    r[t] += r_lin[R.L - t]
    return r


def victim_error(victim, partner, own_scale=False):
    """The worst error of the victim's r_lin in the paired float32 arithmetic, relative to its r(0), against float64 on the
    victim's window alone.  NaN or inf where the model's r is."""
    with np.errstate(all="ignore"):
        got, _, e, _ = paired_r_lin(victim, partner, own_scale)
        x = np.ldexp(np.asarray(victim, np.float64), -e)
        ref = np.correlate(x, x, mode="full")[R.SIZE - 1:]
        return float(np.max(np.abs(got - ref)) / ref[0]) if np.all(np.isfinite(got)) else float("nan")
