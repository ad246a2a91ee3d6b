//! `ChannelFirs`: per-channel FIR nodes over the channels of a bank (`dspfx_firs_*`).
//!
//! An engine runs one FIR node (nodes/fir.rs) with one tap table for all its channels; here channel c may carry one FIR node of
//! its own -- its own taps (f64), tap count T (1 .. `max_taps`), mode and deque of past samples -- and its output is bit for bit
//! what the reference's node gives through all its history: the fill phase of its `VecDeque` and the split of the sum at the
//! deque's physical wrap included.  A node exists from the first `set_taps` that names the channel until `drop_nodes`; a fresh
//! bank copies.  `set_taps` on a channel that carries a node is the reference's reload (fir.rs:153-171): the taps are replaced,
//! the deque is kept.  The GUI thread stores through `set_*`, which never wait for the device: the next `run` applies the stores
//! in order.
//! NOT compiled in the build container (no rustc).
use super::engine::Error;
use super::ffi::*;
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::ptr;

pub struct ChannelFirs {
    h: *mut dspfx_firs,
    channels: u32,
    max_taps: u32,
}
unsafe impl Send for ChannelFirs {}
// runs are serialised by the bank's own lock; stores take the store queue's
unsafe impl Sync for ChannelFirs {}

fn reason(h: *const dspfx_firs, what: &str) -> String {
    let msg = unsafe { CStr::from_ptr(dspfx_firs_last_error(h)) }.to_string_lossy().into_owned();
    if msg.is_empty() { what.into() } else { msg }
}

impl ChannelFirs {
    /// `max_taps`: the longest response a channel may carry, 1 .. `DSPFX_FIRS_MAX_TAPS`; `tile_channels`: 0 (frame-major) or the
    /// engine's W.
    pub fn new(device: i32, channels: u32, max_taps: u32, tile_channels: u32, max_frames: u32) -> Result<Self, Error> {
        let desc = dspfx_firs_desc { abi_version: DSPFX_ABI_VERSION, device, n_channels: channels, max_frames, tile_channels, max_taps, general_only: 0 };
        let mut h = ptr::null_mut();
        let rc = unsafe { dspfx_firs_create(&desc, &mut h) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_firs_create") });
        }
        Ok(ChannelFirs { h, channels, max_taps })
    }
    fn check(&self, rc: c_int, what: &str) -> Result<(), Error> {
        if rc == DSPFX_OK { Ok(()) } else { Err(Error { status: rc, message: reason(self.h, what) }) }
    }
    pub fn channels(&self) -> u32 { self.channels }
    pub fn max_taps(&self) -> u32 { self.max_taps }
    /// The device bytes of a bank's tables, `channels * (12 * max_taps + 80)` (a pure host function).
    pub fn plan(channels: u64, max_taps: u32) -> Result<u64, Error> {
        let mut bytes = 0u64;
        let rc = unsafe { dspfx_firs_plan(channels, max_taps, &mut bytes) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_firs_plan") });
        }
        Ok(bytes)
    }
    /// A DEVICE block of `n_frames` frames in the bank's layout through every channel's node into the DEVICE block `out` (`out`
    /// may be `input`: in place).  Asynchronous on `stream`.
    pub unsafe fn run(&self, input: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> Result<(), Error> {
        let rc = dspfx_firs_run(self.h, input, out, n_frames, stream);
        self.check(rc, "dspfx_firs_run")
    }
    /// One response (time order) for `count` channels from `first_channel` (any thread, never waits for the device).  `mode`:
    /// `Some(DSPFX_FIR_BALANCED | DSPFX_FIR_AVERAGE)`, or `None` to keep the node's (a new node: Balanced).
    pub fn set_taps(&self, response: &[f64], mode: Option<u32>, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe {
            dspfx_firs_set_taps(self.h, response.as_ptr(), response.len() as u32, 0, mode.unwrap_or(DSPFX_FIRS_NONE), first_channel, count)
        };
        self.check(rc, "dspfx_firs_set_taps")
    }
    /// A response per channel: `rows` is `[count][n_taps]`, row i for channel `first_channel + i`.
    pub fn set_taps_rows(&self, rows: &[f64], n_taps: u32, mode: Option<u32>, first_channel: u64) -> Result<(), Error> {
        if n_taps == 0 || rows.len() % n_taps as usize != 0 {
            return Err(Error { status: DSPFX_ERR_INVALID, message: "rows is not [count][n_taps]".into() });
        }
        let count = (rows.len() / n_taps as usize) as u64;
        let rc = unsafe { dspfx_firs_set_taps(self.h, rows.as_ptr(), n_taps, 1, mode.unwrap_or(DSPFX_FIRS_NONE), first_channel, count) };
        self.check(rc, "dspfx_firs_set_taps")
    }
    /// The mode of the nodes of `count` channels from `first_channel`; a channel without a node stays without one.
    pub fn set_mode(&self, mode: u32, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_firs_set_mode(self.h, mode, first_channel, count) };
        self.check(rc, "dspfx_firs_set_mode")
    }
    /// Removes the node of `count` channels from `first_channel`: a copy again, and a later `set_taps` makes a new node.
    pub fn drop_nodes(&self, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_firs_drop(self.h, first_channel, count) };
        self.check(rc, "dspfx_firs_drop")
    }
    /// Empties the deque of `count` channels from `first_channel`; taps and mode stay.
    pub fn reset(&self, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_firs_reset(self.h, first_channel, count) };
        self.check(rc, "dspfx_firs_reset")
    }
    /// 1 / 0 per channel: it carries a node, as all stores made so far left it.
    pub fn present(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_firs_present(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_firs_present")?;
        Ok(m)
    }
    /// Per channel the node's tap count, 0 without a node.
    pub fn lengths(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_firs_lengths(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_firs_lengths")?;
        Ok(m)
    }
    /// Per channel `DSPFX_FIR_BALANCED`, `DSPFX_FIR_AVERAGE`, or `DSPFX_FIRS_NONE` without a node.
    pub fn modes(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_firs_modes(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_firs_modes")?;
        Ok(m)
    }
    /// The response of one channel as it was given (time order); empty without a node.
    pub fn taps(&self, channel: u64) -> Result<Vec<f64>, Error> {
        let mut v = vec![0f64; self.max_taps as usize];
        let mut n = 0u32;
        let rc = unsafe { dspfx_firs_taps(self.h, channel, v.as_mut_ptr(), &mut n) };
        self.check(rc, "dspfx_firs_taps")?;
        v.truncate(n as usize);
        Ok(v)
    }
    /// The DEVICE pointer of the deque words, `[3][channels]` i32: len, cap, head after the last run, on its stream.
    pub fn deque(&self) -> Result<*const i32, Error> {
        let mut p = ptr::null();
        let rc = unsafe { dspfx_firs_deque(self.h, &mut p) };
        self.check(rc, "dspfx_firs_deque")?;
        Ok(p)
    }
}

impl Drop for ChannelFirs {
    fn drop(&mut self) {
        unsafe {
            dspfx_firs_destroy(self.h);
        }
    }
}
