"""float64 numpy restatement of the Pitch Detector (dsp-stuff/src/nodes/pitch.rs:120-146), for the pitch tests.

pitch.rs calls `McLeodDetector::new(1024, 512).get_pitch(view, 48_000, power_thresh, clarity_thresh, pick_thresh)` from the
`pitch-detection` crate (magnetophon's fork, the reference's Cargo.lock:3092-3096).  That crate is not vendored: what follows is
restated from the published method (McLeod & Wyvill 2005, "A smarter way to find pitch") with pitch.rs's parameters, UNPINNED
like the envelope detector's and the sinc converter's restatements.  It is written from include/dspfx.h's description, not from
the product code.  A correction to the method lands here and in pitch_kernels.hip.

detect(x, P, C, K) -> (found, tau, freq, clarity, margin).  `margin` is the smallest distance of a quantity that decides the
result from the threshold it is compared with; a GPU result may differ where f32 rounding can flip such a decision.
"""
import numpy as np

SIZE, PADDING, RATE = 1024, 512, 48000
L = SIZE + PADDING
WINDOW = SIZE
BLOCK = 128


def autocorr(x):
    """Circular autocorrelation of x zero-padded to L = 1536 (what the crate's FFT computes), lags [0, 1024):
    r(tau) = r_lin(tau) + r_lin(1536 - tau) for tau > 512."""
    x = np.asarray(x, np.float64)
    r_lin = np.correlate(x, x, mode="full")[SIZE - 1:]          # r_lin(0..1023)
    r = r_lin.copy()
    t = np.arange(PADDING + 1, SIZE)
    r[t] += r_lin[L - t]
    return r


def autocorr_direct(x):
    """O(N^2) circular autocorrelation of the zero-padded window, straight from the definition (for the tests)."""
    x = np.asarray(x, np.float64)
    xp = np.zeros(L)
    xp[:SIZE] = x
    return np.array([sum(xp[j] * xp[(j + t) % L] for j in range(L)) for t in range(SIZE)])


def nsdf(x, r=None):
    """n(tau) = 2 r(tau) / m(tau).  m(0) = 2 r(0), m(tau) = m(tau-1) - x[tau-1]^2 - x[1024-tau]^2 (the energy of the pairs that
    r_lin(tau) multiplies); for tau > 512, where r carries the aliased pairs r_lin(1536 - tau), m carries their energy
    m(1536 - tau) too, so that |n| <= 1.  (Without it the aliased tail reaches n ~ 30 for any periodic window and every pick lands
    there: a 440 Hz sine reads as 47.6 Hz.  With it the alias changes the result below about 94 Hz only.)  Where m(tau) <= 0 (a
    window whose ends are exactly zero) n(tau) is taken as 0.  `r` replaces autocorr(x) (a model of some other arithmetic for
    r(tau), lags [0, 1024)); m(tau) is always the float64 one."""
    x = np.asarray(x, np.float64)
    r_own = autocorr(x)
    r = r_own if r is None else np.asarray(r, np.float64)
    sq = x * x
    m_lin = np.empty(SIZE)
    m_lin[0] = 2.0 * r_own[0]
    m_lin[1:] = m_lin[0] - np.cumsum(sq[:SIZE - 1] + sq[::-1][:SIZE - 1])
    m = m_lin.copy()
    t = np.arange(PADDING + 1, SIZE)
    m[t] += m_lin[L - t]
    n = np.zeros(SIZE)
    ok = m > 0
    n[ok] = 2.0 * r[ok] / m[ok]
    return n


def key_maxima(n):
    """Skip the positive lobe at tau = 0; then one key maximum per maximal run with n > 0: the first tau of the run's largest
    value.  A run still open at tau = 1023 counts.  Returns [(tau, run_start, run_end_exclusive)]."""
    pos = n > 0
    t = 1
    while t < SIZE and pos[t]:
        t += 1
    out = []
    while t < SIZE:
        while t < SIZE and not pos[t]:
            t += 1
        if t >= SIZE:
            break
        s = t
        while t < SIZE and pos[t]:
            t += 1
        out.append((s + int(np.argmax(n[s:t])), s, t))
    return out


def detect(x, P=0.5, C=0.5, K=0.5, r=None):
    x = np.asarray(x, np.float64)
    none = (False, -1, 0.0, 0.0)
    if not np.all(np.isfinite(x)) or not np.any(x):
        return none + (np.inf,)
    power = float(np.sum(x * x))
    margins = [abs(power - P)]
    if power < P:
        return none + (min(margins),)
    n = nsdf(x, r)
    keys = key_maxima(n)
    if not keys:
        return none + (min(margins + [float(np.min(np.abs(n[1:])))]),)
    M = max(n[k] for k, _, _ in keys)
    thr = K * M
    chosen = next(((k, s, e) for k, s, e in keys if n[k] >= thr), None)
    if chosen is None:                                   # K > 1
        return none + (min(margins + [abs(n[k] - thr) for k, _, _ in keys]),)
    k, s, e = chosen
    margins.append(abs(n[k] - thr))
    margins += [thr - n[j] for j, _, _ in keys if j < k]                     # the runners-up before it
    run = np.delete(n[s:e], k - s)
    if run.size:
        margins.append(n[k] - float(np.max(run)))                           # the argmax inside its run
    margins.append(float(np.min(np.abs(n[1:min(e + 1, SIZE)]))))            # the signs that bound the runs up to it
    margins.append(abs(n[k] - C))
    if n[k] < C:
        return none + (min(margins),)
    a, b = n[k - 1], n[k]
    delta = 0.0
    if k < SIZE - 1:
        c = n[k + 1]
        den = 2.0 * (2.0 * b - a - c)
        if den != 0.0:
            delta = (c - a) / den
        y = b + (c - a) * delta / 4.0
    else:
        y = b
    return True, k, RATE / (k + delta), y / n[0], min(margins)


def detect_bank(windows, P=0.5, C=0.5, K=0.5):
    """windows [channels][1024] -> found, tau, freq, clarity, margin arrays."""
    res = [detect(w, P, C, K) for w in windows]
    return tuple(np.array([r[i] for r in res]) for i in range(5))


def windows_due(pushes):
    """The frame rule on the host: window w (samples [1024w, 1024w + 1024)) is detected by the push after which at least
    1024 (w + 1) + 1 frames have been pushed (pitch.rs: detect the oldest 1024 first, then append the call's block; the
    page-rounded circular_buffer(128) of f32 holds at least 1024 samples).  -> [list of windows per push]."""
    out, f = [], 0
    for n in pushes:
        f0, f = f, f + n
        out.append([w for w in range(f) if f0 <= WINDOW * (w + 1) < f])
    return out


class HostBank:
    """pitch.rs's state over a bank: the held (freq, clarity) per channel, 0.0 initially, updated on Some."""

    def __init__(self, channels, P=0.5, C=0.5, K=0.5):
        self.freq = np.zeros(channels)
        self.clarity = np.zeros(channels)
        self.P, self.C, self.K = P, C, K
        self.frames = np.zeros((0, channels))
        self.windows = 0

    def push(self, block):
        """block [n_frames][channels] (frame-major)"""
        f0 = self.frames.shape[0]
        self.frames = np.concatenate([self.frames, np.asarray(block, np.float64)])
        for w in range(self.windows, self.frames.shape[0]):
            if not (f0 <= WINDOW * (w + 1) < self.frames.shape[0]):
                break
            found, _, fr, cl, _ = detect_bank(self.frames[WINDOW * w:WINDOW * (w + 1)].T, self.P, self.C, self.K)
            self.freq[found] = fr[found]
            self.clarity[found] = cl[found]
            self.windows += 1
