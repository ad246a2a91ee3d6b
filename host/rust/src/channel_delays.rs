//! `ChannelDelays`: per-channel Reverb (feedback delay) sliders over the channels of a bank (`dspfx_delays_*`).
//!
//! In the reference every graph owns its Reverb node with its own `seconds` and `decay` sliders and its own ring
//! (reverb.rs:29-41).  A host with one participant per channel binds one `ChannelDelays` over the bank's DEVICE block, where
//! `ChannelStrips` goes: channel c carries its own node from the first store that names it until it is dropped, with a ring of
//! `dspfx_delay_len(seconds, page_round)` frames.  The GUI thread stores sliders through `set_delay`, which never waits for the
//! device: the next `run` applies the stores in order, and every store -- decay alone included -- starts the stored channels again
//! from a zero ring, as `refresh_seconds` does (reverb.rs:55-71).
//! NOT compiled in the build container (no rustc).
use super::engine::Error;
use super::ffi::*;
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::ptr;

pub struct ChannelDelays {
    h: *mut dspfx_delays,
    channels: u32,
}
unsafe impl Send for ChannelDelays {}
// runs are serialised by the bank's own lock; slider stores take the store lock and the store queue's
unsafe impl Sync for ChannelDelays {}

fn reason(h: *const dspfx_delays, what: &str) -> String {
    let msg = unsafe { CStr::from_ptr(dspfx_delays_last_error(h)) }.to_string_lossy().into_owned();
    if msg.is_empty() { what.into() } else { msg }
}

impl ChannelDelays {
    /// `max_seconds` sizes every channel's ring (`plan`); `tile_channels`: 0 (frame-major) or the engine's W; `link_flags` as the engine's.
    pub fn new(device: i32, channels: u32, max_seconds: f32, tile_channels: u32, max_frames: u32, link_flags: u32, page_round: bool) -> Result<Self, Error> {
        let desc = dspfx_delays_desc { abi_version: DSPFX_ABI_VERSION, device, n_channels: channels, max_frames, tile_channels, max_seconds, page_round: page_round as u32, link_flags };
        let mut h = ptr::null_mut();
        let rc = unsafe { dspfx_delays_create(&desc, &mut h) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_delays_create") });
        }
        Ok(ChannelDelays { h, channels })
    }
    fn check(&self, rc: c_int, what: &str) -> Result<(), Error> {
        if rc == DSPFX_OK { Ok(()) } else { Err(Error { status: rc, message: reason(self.h, what) }) }
    }
    pub fn channels(&self) -> u32 { self.channels }
    /// The ring frames per channel and the ring bytes of a bank (a pure host function).
    pub fn plan(channels: u64, max_seconds: f32, page_round: bool) -> Result<(u32, u64), Error> {
        let (mut cap, mut bytes) = (0u32, 0u64);
        let rc = unsafe { dspfx_delays_plan(channels, max_seconds, page_round as c_int, &mut cap, &mut bytes) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_delays_plan") });
        }
        Ok((cap, bytes))
    }
    /// A DEVICE block of `n_frames` frames in the bank's layout through every channel's delay into the DEVICE block `out`
    /// (`out` may be `input`: in place).  Asynchronous on `stream`.
    pub unsafe fn run(&self, input: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> Result<(), Error> {
        let rc = dspfx_delays_run(self.h, input, out, n_frames, stream);
        self.check(rc, "dspfx_delays_run")
    }
    /// Stores the sliders of channels `first_channel ..`, one value per channel; `None` keeps each channel's value (any thread, never
    /// waits for the device).  The stored channels start again from a zero ring.  Refused whole when a channel would need more
    /// than the bank's ring.
    pub fn set_delay(&self, seconds: Option<&[f32]>, decay: Option<&[f32]>, first_channel: u64) -> Result<(), Error> {
        let count = match (seconds, decay) {
            (Some(s), Some(d)) if s.len() != d.len() => return Err(Error { status: DSPFX_ERR_INVALID, message: "seconds and decay name different numbers of channels".into() }),
            (Some(s), _) => s.len(),
            (None, Some(d)) => d.len(),
            (None, None) => return Err(Error { status: DSPFX_ERR_INVALID, message: "no slider given: clear() drops the node".into() }),
        };
        let rc = unsafe { dspfx_delays_set_delay(self.h, seconds.map_or(ptr::null(), |s| s.as_ptr()), decay.map_or(ptr::null(), |d| d.as_ptr()), first_channel, count as u64) };
        self.check(rc, "dspfx_delays_set_delay")
    }
    /// Removes the node of `count` channels from `first_channel`; a later store starts from a zero ring and the default sliders.
    pub fn clear(&self, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_delays_set_delay(self.h, ptr::null(), ptr::null(), first_channel, count) };
        self.check(rc, "dspfx_delays_set_delay")
    }
    /// Every present channel's ring back to zeros; the sliders and the nodes stay.
    pub fn reset(&self) -> Result<(), Error> {
        let rc = unsafe { dspfx_delays_reset(self.h) };
        self.check(rc, "dspfx_delays_reset")
    }
    /// 1 / 0 per channel: it carries a node, as all stores made so far left it.
    pub fn present(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_delays_present(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_delays_present")?;
        Ok(m)
    }
    /// Every channel's ring length in frames, 0 where there is no node.
    pub fn lengths(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_delays_lengths(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_delays_lengths")?;
        Ok(m)
    }
}

impl Drop for ChannelDelays {
    fn drop(&mut self) {
        unsafe {
            dspfx_delays_destroy(self.h);
        }
    }
}
