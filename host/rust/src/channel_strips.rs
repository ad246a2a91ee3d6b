//! `ChannelStrips`: per-channel Gain and BiQuad sliders over the channels of a bank (`dspfx_strips_*`).
//!
//! In the reference every graph has its own node instances and its own `Atomic<f32>` sliders (gain.rs:21-22, biquad.rs:18-41): N
//! channels are N independent sets of settings.  A host with one participant per channel binds one `ChannelStrips` over the bank's
//! DEVICE block, between the chain and `MixGroups::run` / `returns` (or ahead of the chain): channel c goes through its own Gain node
//! and its own BiQuad bands 0 .. K-1, each present from the first store that names it until it is dropped.  The GUI thread stores
//! sliders through `set_gain` / `set_band`, which never wait for the device: the next `run` applies them in order, and a band store
//! zeroes that band's state on the stored channels as `regenerate_filter` does (biquad.rs:62-76).
//! NOT compiled in the build container (no rustc).
use super::engine::Error;
use super::ffi::*;
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::ptr;

pub struct ChannelStrips {
    h: *mut dspfx_strips,
    channels: u32,
    bands: u32,
}
unsafe impl Send for ChannelStrips {}
// runs are serialised by the bank's own lock; slider stores only take the store queue's
unsafe impl Sync for ChannelStrips {}

fn reason(h: *const dspfx_strips, what: &str) -> String {
    let msg = unsafe { CStr::from_ptr(dspfx_strips_last_error(h)) }.to_string_lossy().into_owned();
    if msg.is_empty() { what.into() } else { msg }
}

impl ChannelStrips {
    /// `bands`: 1 ..= `DSPFX_STRIPS_MAX_BANDS`; `tile_channels`: 0 (frame-major) or the engine's W; `link_flags` as the engine's.
    pub fn new(device: i32, channels: u32, bands: u32, tile_channels: u32, max_frames: u32, link_flags: u32) -> Result<Self, Error> {
        let desc = dspfx_strips_desc { abi_version: DSPFX_ABI_VERSION, device, n_channels: channels, max_frames, tile_channels, bands, link_flags };
        let mut h = ptr::null_mut();
        let rc = unsafe { dspfx_strips_create(&desc, &mut h) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_strips_create") });
        }
        Ok(ChannelStrips { h, channels, bands })
    }
    fn check(&self, rc: c_int, what: &str) -> Result<(), Error> {
        if rc == DSPFX_OK { Ok(()) } else { Err(Error { status: rc, message: reason(self.h, what) }) }
    }
    pub fn channels(&self) -> u32 { self.channels }
    pub fn bands(&self) -> u32 { self.bands }
    /// A DEVICE block of `n_frames` frames in the bank's layout through every channel's strip into the DEVICE block `out`
    /// (`out` may be `input`: in place).  Asynchronous on `stream`.
    pub unsafe fn run(&self, input: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> Result<(), Error> {
        let rc = dspfx_strips_run(self.h, input, out, n_frames, stream);
        self.check(rc, "dspfx_strips_run")
    }
    /// Stores the Gain levels of channels `first_channel ..` (any thread, never waits for the device).
    pub fn set_gain(&self, levels: &[f32], first_channel: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_strips_set_gain(self.h, levels.as_ptr(), first_channel, levels.len() as u64) };
        self.check(rc, "dspfx_strips_set_gain")
    }
    /// Removes the Gain node of `count` channels from `first_channel`.
    pub fn clear_gain(&self, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_strips_set_gain(self.h, ptr::null(), first_channel, count) };
        self.check(rc, "dspfx_strips_set_gain")
    }
    /// Stores band `band` of channels `first_channel ..`: six raw sliders a0, a1, a2, b0, b1, b2 per channel.  Zeroes the band's
    /// state on exactly those channels.
    pub fn set_band(&self, band: u32, raw6: &[[f32; 6]], first_channel: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_strips_set_band(self.h, band, raw6.as_ptr() as *const f32, first_channel, raw6.len() as u64) };
        self.check(rc, "dspfx_strips_set_band")
    }
    /// Removes band `band` of `count` channels from `first_channel`; a later store starts it from zero state.
    pub fn clear_band(&self, band: u32, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_strips_set_band(self.h, band, ptr::null(), first_channel, count) };
        self.check(rc, "dspfx_strips_set_band")
    }
    /// Zeroes all state; the sliders and the nodes stay.
    pub fn reset(&self) -> Result<(), Error> {
        let rc = unsafe { dspfx_strips_reset(self.h) };
        self.check(rc, "dspfx_strips_reset")
    }
    /// The node mask of every channel as the next run sees it: bit 0 = Gain, bit 1 + b = band b.
    pub fn present(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_strips_present(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_strips_present")?;
        Ok(m)
    }
    /// The five normalised coefficients a1, a2, b0, b1, b2 exactly as the device gets them (a pure host function).
    pub fn coeffs(raw6: &[f32; 6]) -> [f32; 5] {
        let mut k = [0f32; 5];
        unsafe { dspfx_strips_coeffs(raw6.as_ptr(), k.as_mut_ptr()) };
        k
    }
}

impl Drop for ChannelStrips {
    fn drop(&mut self) {
        unsafe {
            dspfx_strips_destroy(self.h);
        }
    }
}
