"""numpy restatement of the device-sample-format conversions at the process boundary (include/dspfx.h, dspfx_pcm_io), for the
PCM tests.  Written from the rule table of the header -- dasp_sample 0.11.0's to_sample / from_sample as the reference calls
them in dsp-stuff/src/devices.rs:235, 253 (input) and 424, 432, 477, 488 (output) -- not from the product code."""
import numpy as np

F32, I16, U16, I32 = 0, 1, 2, 3
NP_DTYPE = {F32: np.float32, I16: np.int16, U16: np.uint16, I32: np.int32}
_SCALE = {I16: np.float32(32768.0), U16: np.float32(32768.0), I32: np.float32(2147483648.0)}


def widen_np(s, fmt, channels=1):
    """PCM -> f32 per element; 2 device channels: to_f32(a) + to_f32(b), one f32 add (do_read_2, devices.rs:244-258)."""
    s = np.asarray(s)
    if fmt == F32:
        v = s.astype(np.float32)
    elif fmt == U16:   # through i16
        v = (s.astype(np.int32) - 32768).astype(np.float32) / _SCALE[fmt]
    else:              # i16 exact; i32: one round to nearest even in the int -> f32 conversion, the division by 2^31 is exact
        v = s.astype(np.float32) / _SCALE[fmt]
    if channels == 2:
        v = v.reshape(v.shape[:-1] + (v.shape[-1] // 2, 2))
        v = (v[..., 0] + v[..., 1]).astype(np.float32)
    return v


def narrow_np(x, fmt, channels=1):
    """f32 -> PCM per element: Rust `(x * scale) as iN` -- truncated toward zero, saturated, NaN -> 0; u16 = the i16 result
    + 32768.  2 device channels: the sample in both slots (o.fill(x), devices.rs:476-490)."""
    x = np.asarray(x, np.float32)
    if fmt == F32:
        v = x.copy()
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            y = (x * _SCALE[fmt]).astype(np.float64)          # a product by a power of two: exact in f32 (or +-inf)
            lo, hi = (-2147483648.0, 2147483647.0) if fmt == I32 else (-32768.0, 32767.0)
            y = np.where(np.isnan(y), 0.0, y)
            v = np.trunc(np.clip(y, lo, hi)).astype(np.int64)
        v = (v + 32768).astype(np.uint16) if fmt == U16 else v.astype(NP_DTYPE[fmt])
    if channels == 2:
        v = np.repeat(v, 2, axis=-1)
    return v
