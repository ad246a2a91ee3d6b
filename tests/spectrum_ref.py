"""The Spectrogram bank restated in numpy (include/dspfx.h, "spectrogram bank"): what the tests compare dspfx_spectrum_* with.

  vol[k] = |FFT(window * x)[k]| * gain[k],  k in [0, n/2)

The window product is rounded to f32 (as the kernel's), the spectrum is numpy.fft.rfft in FLOAT64 on that product, the
magnitude and the gain product stay in f64: this is the exact value of what the bank computes in f32, so the distance of a
column from it is the bank's own rounding.  HostBank does the window and column bookkeeping for arbitrary push lengths.
"""
import math

import numpy as np

RATE = 48000.0
SIZES = (128, 256, 512, 1024, 2048, 4096, 8192)
SLOT = 128


def hann(n):
    """The default window: 0.5 - 0.5 cos(2 pi i / (n - 1)) in f64 (the C library's cos), rounded once to f32; entries
    n - 1 - i repeat entries i < n/2."""
    w = np.zeros(n, np.float32)
    for i in range(n // 2):
        w[i] = w[n - 1 - i] = np.float32(0.5 - 0.5 * math.cos(2.0 * math.pi * float(i) / float(n - 1)))
    return w


def bin_hz(n):
    """k * 48000 / n for k in [0, n/2): exact in f32 for the seven sizes."""
    return (np.arange(n // 2, dtype=np.float64) * RATE / n).astype(np.float32)


def bins(n, lower_hz, upper_hz):
    """(k_lo, k_hi): lower_hz <= k * 48000 / n <= upper_hz for k_lo <= k < k_hi."""
    ks = [k for k in range(n // 2) if lower_hz <= k * RATE / n <= upper_hz]
    return (ks[0], ks[-1] + 1) if ks else (0, 0)


def windowed(x, window=None):
    """x [n][N] float32 -> window * x rounded to f32, [n][N]"""
    x = np.asarray(x, np.float32)
    w = hann(x.shape[0]) if window is None else np.asarray(window, np.float32)
    return (w[:, None] * x).astype(np.float32)


def column(x, window=None, gain=None):
    """One window x [n][N] float32 -> the column [n/2][N] in float64."""
    n = x.shape[0]
    v = np.abs(np.fft.rfft(windowed(x, window).astype(np.float64), axis=0))[:n // 2]
    if gain is not None:
        v = v * np.asarray(gain, np.float32).astype(np.float64)[:, None]
    return v


def rel_err(got, ref):
    """per channel ||got - ref||_2 / ||ref||_2 over the column ([n/2][N] each) -> [N] float64"""
    got = np.asarray(got, np.float64)
    num = np.sqrt(((got - ref) ** 2).sum(axis=0))
    den = np.sqrt((ref ** 2).sum(axis=0))
    return num / den


def ceiling(n):
    """What no correct f32 FFT exceeds: (7 log2 n + 4) 2^-24 (Higham's bound for radix 2 with correctly rounded twiddles,
    plus the window product, the magnitude and the gain)."""
    return (7.0 * math.log2(n) + 4.0) * 2.0 ** -24


class HostBank:
    """Window and history bookkeeping of the bank for pushes of any length: windows are frames [n w, n (w + 1)), window w is
    computed as soon as n (w + 1) frames are in, the newest `columns` columns are kept."""

    def __init__(self, channels, fft_size=512, columns=1, window=None, gain=None):
        self.N, self.n, self.columns = channels, fft_size, columns
        self.window, self.gain = window, gain
        self.reset()

    def reset(self):
        self.fifo = np.zeros((0, self.N), np.float32)
        self.frames = 0
        self.windows = 0
        self.history = []                       # newest last
        self.due_at = []                        # frames in when each window ran

    def push(self, x):
        x = np.asarray(x, np.float32).reshape(-1, self.N)
        self.fifo = np.concatenate([self.fifo, x])
        self.frames += x.shape[0]
        while self.fifo.shape[0] >= self.n:
            self.history.append(column(self.fifo[:self.n], self.window, self.gain))
            self.history = self.history[-self.columns:]
            self.fifo = self.fifo[self.n:]
            self.windows += 1
            self.due_at.append(self.n * self.windows)

    def slot_free(self):
        return self.frames % SLOT == 0

    def column(self, age=0):
        if age < 0 or age >= self.columns or age >= len(self.history):
            return None
        return self.history[-1 - age]
