"""References for the convolver bank (include/dspfx.h, dspfx_convolve_*).

exact()        the answer: scipy.signal.fftconvolve in float64 of the f32 input with the f64 taps, cut to the frames run
Partitioned    a float32 restatement of the bank's algorithm (scipy.fft in complex64, 128-frame partitions, partial sums
               over 16 consecutive partitions); it is used ONLY to print its own error beside the GPU's, never as a bar
Signals are [frames, channels]; h is the response in time order."""
import numpy as np
import scipy.fft
import scipy.signal

L = 128
GROUP = 16
SIZES = (1, 127, 128, 129, 1000, 4096)
PARTS = {1: 1, 127: 1, 128: 1, 129: 2, 1000: 8, 48000: 375}
BAR = 1e-6                                   # the FIR row's bar: relative RMS


def partitions(n_taps):
    return (n_taps + L - 1) // L


def response(n_taps, seed=0):
    """noise under an exponential decay (60 dB over the length), f64, unit energy"""
    rng = np.random.default_rng(1000 + seed)
    h = rng.standard_normal(n_taps) * np.exp(-6.9 * np.arange(n_taps) / max(n_taps, 1))
    return h / np.sqrt(np.sum(h * h))


def noise(frames, channels, seed=0):
    """white noise, per-channel amplitudes from 1e-3 to 1"""
    rng = np.random.default_rng(2000 + seed)
    amp = np.logspace(-3.0, 0.0, channels)
    rng.shuffle(amp)
    return (rng.uniform(-1.0, 1.0, (frames, channels)) * amp).astype(np.float32)


def exact(x, h, divisor=1.0):
    """float64: y[n] = sum_j h[j] x[n - j] from silence, for the frames of x"""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    h64 = np.asarray(h, np.float64)
    y = scipy.signal.fftconvolve(x64, h64[:, None], axes=0)[:x64.shape[0]]
    return y * float(divisor)


def table_f64(h):
    """[128, P] complex128: bin k of the 256-point FFT of every zero-padded partition; [0, p] = DC + i Nyquist"""
    h = np.asarray(h, np.float64)
    P = partitions(len(h))
    hp = np.zeros((P, 2 * L))
    for p in range(P):
        seg = h[p * L:(p + 1) * L]
        hp[p, :len(seg)] = seg
    H = np.fft.rfft(hp, axis=1)                                  # [P, 129]
    out = H[:, :L].T.copy()
    out[0] = H[:, 0].real + 1j * H[:, L].real
    return out


def partition_l1(h):
    h = np.abs(np.asarray(h, np.float64))
    return np.array([h[p * L:(p + 1) * L].sum() for p in range(partitions(len(h)))])


class Partitioned:
    """the algorithm in float32 / complex64 on the host; `max_taps` as the bank's: history kept for reloads"""

    def __init__(self, channels, h, divisor=1.0, max_taps=0):
        self.N = channels
        self.slots = partitions(max(max_taps, len(h)))
        self.set_taps(h, divisor)
        self.reset()

    def set_taps(self, h, divisor=1.0):
        h = np.asarray(h, np.float64)
        self.P = partitions(len(h))
        assert self.P <= self.slots
        hp = np.zeros((self.P, 2 * L))
        for p in range(self.P):
            seg = h[p * L:(p + 1) * L]
            hp[p, :len(seg)] = seg
        self.H = np.fft.rfft(hp, axis=1).astype(np.complex64)    # [P, 129], rounded once from f64
        self.divisor = np.float32(divisor)

    def reset(self):
        self.prev = np.zeros((L, self.N), np.float32)
        self.ring = [np.zeros((L + 1, self.N), np.complex64) for _ in range(self.slots)]   # newest first

    def run(self, block):
        block = np.asarray(block, np.float32)
        X = scipy.fft.rfft(np.concatenate([self.prev, block]), axis=0)
        assert X.dtype == np.complex64
        self.prev = block.copy()
        self.ring = [X] + self.ring[:-1]
        total = np.zeros_like(X)
        for g in range(0, self.P, GROUP):
            part = np.zeros_like(X)
            for p in range(g, min(g + GROUP, self.P)):
                part = part + self.H[p][:, None] * self.ring[p]
            total = total + part
        y = scipy.fft.irfft(total, n=2 * L, axis=0)
        assert y.dtype == np.float32
        return y[L:] * self.divisor

    def run_all(self, x):
        return np.concatenate([self.run(x[b:b + L]) for b in range(0, len(x), L)])


def rel_rms(got, want):
    """per channel: RMS of the error over the run / RMS of the answer over the run"""
    e = np.asarray(got, np.float64) - want
    return np.sqrt(np.mean(e * e, axis=0)) / np.sqrt(np.mean(want * want, axis=0))


def block_rms(got, want):
    """per channel: the worst block's error RMS / the channel's RMS over the run"""
    e = np.asarray(got, np.float64) - want
    eb = np.sqrt(np.mean(e.reshape(-1, L, e.shape[1]) ** 2, axis=1))       # [blocks, channels]
    return eb.max(axis=0) / np.sqrt(np.mean(want * want, axis=0))
