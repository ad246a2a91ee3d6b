//! `ChannelCancellers`: per-channel adaptive (NLMS) FIR filters over the channels of a bank (`dspfx_cancel_*`).
//!
//! Channel c may carry one canceller of its own -- T taps (1 .. `max_taps`) that the DEVICE updates every frame, a step size mu, a
//! regulariser eps, a bulk delay (0 .. `max_delay` frames) and the switch adapt.  Two device blocks come in: `mic`, the primary
//! input, and `reference`, the block the channel was sent; the output is the microphone minus the filter's estimate of the echo.
//! All arithmetic is f32 with every operation rounded once (the rule is in include/dspfx.h).  A node exists from the first `set`
//! that names the channel until `drop_nodes`; a fresh bank copies `mic`.  The double-talk decision is the host's: `set_adapt`.
//! The stores never wait for the device: the next `run` applies them in order.
//! NOT compiled in the build container (no rustc).
use super::engine::Error;
use super::ffi::*;
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::ptr;

pub struct ChannelCancellers {
    h: *mut dspfx_cancel,
    channels: u32,
    max_taps: u32,
    max_delay: u32,
}
unsafe impl Send for ChannelCancellers {}
// runs are serialised by the bank's own lock; stores take the store queue's
unsafe impl Sync for ChannelCancellers {}

fn reason(h: *const dspfx_cancel, what: &str) -> String {
    let msg = unsafe { CStr::from_ptr(dspfx_cancel_last_error(h)) }.to_string_lossy().into_owned();
    if msg.is_empty() { what.into() } else { msg }
}

fn opt<T>(v: Option<&[T]>) -> *const T {
    v.map_or(ptr::null(), |s| s.as_ptr())
}

impl ChannelCancellers {
    /// `max_taps`: 1 .. `DSPFX_CANCEL_MAX_TAPS`; `max_delay`: 0 .. `DSPFX_CANCEL_MAX_DELAY` frames; `tile_channels`: 0 (frame-major)
    /// or the engine's W.
    pub fn new(device: i32, channels: u32, max_taps: u32, max_delay: u32, tile_channels: u32, max_frames: u32) -> Result<Self, Error> {
        let desc = dspfx_cancel_desc { abi_version: DSPFX_ABI_VERSION, device, n_channels: channels, max_frames, tile_channels, max_taps, max_delay, general_only: 0 };
        let mut h = ptr::null_mut();
        let rc = unsafe { dspfx_cancel_create(&desc, &mut h) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_cancel_create") });
        }
        Ok(ChannelCancellers { h, channels, max_taps, max_delay })
    }
    fn check(&self, rc: c_int, what: &str) -> Result<(), Error> {
        if rc == DSPFX_OK { Ok(()) } else { Err(Error { status: rc, message: reason(self.h, what) }) }
    }
    pub fn channels(&self) -> u32 { self.channels }
    pub fn max_taps(&self) -> u32 { self.max_taps }
    pub fn max_delay(&self) -> u32 { self.max_delay }
    /// The device bytes of a bank's tables (a pure host function).
    pub fn plan(channels: u64, max_taps: u32, max_delay: u32) -> Result<u64, Error> {
        let mut bytes = 0u64;
        let rc = unsafe { dspfx_cancel_plan(channels, max_taps, max_delay, &mut bytes) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_cancel_plan") });
        }
        Ok(bytes)
    }
    /// DEVICE blocks of `n_frames` frames in the bank's layout: `mic` against `reference` into `out` (`out` may be `mic`: in place;
    /// it may not overlap `reference`).  Asynchronous on `stream`.
    pub unsafe fn run(&self, mic: *const f32, reference: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> Result<(), Error> {
        let rc = dspfx_cancel_run(self.h, mic, reference, out, n_frames, stream);
        self.check(rc, "dspfx_cancel_run")
    }
    /// The node of `count` channels from `first_channel`: each slice is `None` (keep; a new node: `max_taps` taps, mu 0.5, eps 1e-6,
    /// delay 0, adapting) or one value per channel.
    pub fn set(&self, taps: Option<&[u32]>, mu: Option<&[f32]>, eps: Option<&[f32]>, delay: Option<&[u32]>, adapt: Option<&[u32]>, first_channel: u64,
               count: u64) -> Result<(), Error> {
        for n in [taps.map(|s| s.len()), mu.map(|s| s.len()), eps.map(|s| s.len()), delay.map(|s| s.len()), adapt.map(|s| s.len())].into_iter().flatten() {
            if n as u64 != count {
                return Err(Error { status: DSPFX_ERR_INVALID, message: "cancel set: every slice holds `count` values".into() });
            }
        }
        let rc = unsafe { dspfx_cancel_set(self.h, opt(taps), opt(mu), opt(eps), opt(delay), opt(adapt), first_channel, count) };
        self.check(rc, "dspfx_cancel_set")
    }
    /// The host's double-talk decision for a range: `false` freezes (the node filters and does not update).
    pub fn set_adapt(&self, adapt: bool, first_channel: u64, count: u64) -> Result<(), Error> {
        let a = vec![adapt as u32; count as usize];
        self.set(None, None, None, None, Some(&a), first_channel, count)
    }
    /// A warm start: one row of weights for the range, every channel of which carries a node of `row.len()` taps.
    pub fn load(&self, row: &[f32], first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_cancel_load(self.h, row.as_ptr(), row.len() as u32, 0, first_channel, count) };
        self.check(rc, "dspfx_cancel_load")
    }
    /// A row per channel: `rows` is `[count][n_taps]`.
    pub fn load_rows(&self, rows: &[f32], n_taps: u32, first_channel: u64) -> Result<(), Error> {
        if n_taps == 0 || rows.len() % n_taps as usize != 0 {
            return Err(Error { status: DSPFX_ERR_INVALID, message: "cancel load: rows is [count][n_taps]".into() });
        }
        let rc = unsafe { dspfx_cancel_load(self.h, rows.as_ptr(), n_taps, 1, first_channel, (rows.len() / n_taps as usize) as u64) };
        self.check(rc, "dspfx_cancel_load")
    }
    /// Removes the node: a copy again, and a later `set` makes a new node.
    pub fn drop_nodes(&self, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_cancel_drop(self.h, first_channel, count) };
        self.check(rc, "dspfx_cancel_drop")
    }
    /// Weights and history back to +0.0; taps, mu, eps, delay and adapt stay.
    pub fn reset(&self, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_cancel_reset(self.h, first_channel, count) };
        self.check(rc, "dspfx_cancel_reset")
    }
    /// Per channel 1 / 0, as all stores so far left it.
    pub fn present(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_cancel_present(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_cancel_present")?;
        Ok(m)
    }
    /// Per channel the tap count T, 0 without a node.
    pub fn lengths(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_cancel_lengths(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_cancel_lengths")?;
        Ok(m)
    }
    /// Per channel mu and eps, `[channels][2]`.
    pub fn sliders(&self) -> Result<Vec<f32>, Error> {
        let mut m = vec![0f32; 2 * self.channels as usize];
        let rc = unsafe { dspfx_cancel_sliders(self.h, m.as_mut_ptr(), 0, self.channels as u64) };
        self.check(rc, "dspfx_cancel_sliders")?;
        Ok(m)
    }
    /// Per channel the bulk delay in frames.
    pub fn delays(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_cancel_delays(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_cancel_delays")?;
        Ok(m)
    }
    /// Per channel 1 where the node updates its weights.
    pub fn adapting(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_cancel_adapting(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_cancel_adapting")?;
        Ok(m)
    }
    /// The DEVICE pointer of the weights, `[max_taps][channels]` f32, row k = w[k]; valid after a run, on its stream.
    pub fn weights(&self) -> Result<*const f32, Error> {
        let mut p = ptr::null();
        let rc = unsafe { dspfx_cancel_weights_view(self.h, &mut p) };
        self.check(rc, "dspfx_cancel_weights_view")?;
        Ok(p)
    }
    /// The DEVICE pointer of the levels, `[2][channels]` f32: sum d^2 and sum e^2 of the last run.
    pub fn levels(&self) -> Result<*const f32, Error> {
        let mut p = ptr::null();
        let rc = unsafe { dspfx_cancel_levels_view(self.h, &mut p) };
        self.check(rc, "dspfx_cancel_levels_view")?;
        Ok(p)
    }
}

impl Drop for ChannelCancellers {
    fn drop(&mut self) {
        unsafe {
            dspfx_cancel_destroy(self.h);
        }
    }
}
