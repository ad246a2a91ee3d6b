"""numpy restatement of the output resampler bank's rules (include/dspfx.h, dspfx_resample_*), for the resampler tests.
Written from the three rule blocks of the header -- dasp's Converter, its Sinc over a 16-frame ring, and the output callback
of dsp-stuff/src/devices.rs:394-498 -- not from the product code.  Frames are f32, vectorised over channels and sequential per
frame; the phase and the coefficients are scalars shared by all channels, computed in f64 with the C library (math.sin /
math.cos, not numpy's vector forms, which need not round alike)."""
import math

import numpy as np

import pcm_ref

TAPS = 16
DEPTH = 8


def input_len(n_out, target_hz):
    """(data.len() as f32 * (48_000.0 / rate as f32)) as usize"""
    return int(np.float32(n_out) * (np.float32(48000.0) / np.float32(target_hz)))


def coefficients(x, idx):
    """-> (max_depth, [(ring index, f64 coefficient)] in summation order) for an output at phase x with the index at idx"""
    nl, nr = idx, idx + 1
    max_depth = DEPTH if idx >= DEPTH - 1 else idx + 1
    terms = []
    for n in range(max_depth):
        for phase, k in ((x, nl - n), (1.0 - x, (nr + n) % TAPS)):
            a = math.pi * (phase + n)
            first = 1.0 if a == 0.0 else math.sin(a) / a
            second = 0.5 + 0.5 * math.cos(a / DEPTH)
            terms.append((k, first * second))
    return max_depth, terms


class Resampler:
    """One converter + interpolator per channel (the scalar state is shared), and the callback."""

    def __init__(self, channels, target_hz):
        self.channels, self.target_hz = int(channels), int(target_hz)
        self.ratio = 48000.0 / float(target_hz)
        self.reset()

    def reset(self):
        self.ring = np.zeros((TAPS, self.channels), np.float32)
        self.value = 0.0
        self.idx = 0

    def _pull(self, frame):
        self.ring[:-1] = self.ring[1:]
        self.ring[-1] = frame
        if self.idx < DEPTH:
            self.idx += 1

    def plan(self, n_out):
        """Steps the scalar state only -> rows of (advance, max_depth, terms); for the plan tests."""
        rows = []
        for _ in range(n_out):
            adv = 0
            while self.value >= 1.0:
                adv += 1
                if self.idx < DEPTH:
                    self.idx += 1
                self.value -= 1.0
            depth, terms = coefficients(self.value, self.idx)
            rows.append((adv, depth, terms))
            self.value += self.ratio
        return rows

    def callback(self, waiting, n_out):
        """waiting: [F][C] f32, all the frames in the FIFO.  -> (out [n_out][C] f32 or None on an underrun, frames consumed)"""
        waiting = np.asarray(waiting, np.float32).reshape(-1, self.channels)
        if len(waiting) < input_len(n_out, self.target_hz):
            return None, 0
        out = np.zeros((n_out, self.channels), np.float32)
        zero = np.zeros(self.channels, np.float32)
        index = 0
        for o in range(n_out):
            while self.value >= 1.0:
                if index < len(waiting):                  # CountingSignal::next
                    self._pull(waiting[index])
                    index += 1
                else:
                    self._pull(zero)
                self.value -= 1.0
            _, terms = coefficients(self.value, self.idx)
            v = np.zeros(self.channels, np.float32)
            with np.errstate(over="ignore", invalid="ignore"):
                for k, c in terms:
                    v = v + (c * self.ring[k].astype(np.float64)).astype(np.float32)
            out[o] = v
            self.value += self.ratio
        return out, index


def silence(n_out, channels, fmt, out_channels):
    return pcm_ref.narrow_np(np.zeros((n_out, channels), np.float32), fmt, out_channels)


def to_device(out_f32, fmt, out_channels):
    """[n_out][C] f32 -> [n_out][C * out_channels] in the device format (from_sample; the sample in both slots)"""
    return pcm_ref.narrow_np(out_f32, fmt, out_channels)
