//! `ChannelGenerators`: per-channel Signal Generators over the channels of a bank (`dspfx_gens_*`).
//!
//! In the reference every graph owns its own Signal Generator (nodes/signal_gen.rs) with its amplitude and frequency sliders, its
//! mode combo box and its clock; an engine runs one setting for all its channels.  Channel c of this bank carries ONE generator
//! from the first `set` that names it until `drop_nodes`, and its sample is bit for bit what an engine whose chain is that
//! generator writes for the channel over the same sequence of block lengths.  A fresh node is the reference's (0.5, 100 Hz, Sine,
//! clock 0); a node keeps its clock through every later `set`.  The bank is a source that lives on the device: `run` writes the
//! samples, or adds them into a block (a tone into one return slot).  The control blocks are the node's `as_input` slider ports;
//! unlike the reference, a port is connected per call and its first value is NOT latched into the slider.  The GUI thread stores
//! through `set`, which never waits for the device: the next `run` applies the stores in order.
//! NOT compiled in the build container (no rustc).
use super::engine::Error;
use super::ffi::*;
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::ptr;

pub struct ChannelGenerators {
    h: *mut dspfx_gens,
    channels: u32,
}
unsafe impl Send for ChannelGenerators {}
// runs are serialised by the bank's own lock; stores take the store lock and the store queue's
unsafe impl Sync for ChannelGenerators {}

fn reason(h: *const dspfx_gens, what: &str) -> String {
    let msg = unsafe { CStr::from_ptr(dspfx_gens_last_error(h)) }.to_string_lossy().into_owned();
    if msg.is_empty() { what.into() } else { msg }
}

fn same_len(count: u64, lens: &[Option<usize>]) -> Result<(), Error> {
    for n in lens.iter().flatten() {
        if *n as u64 != count {
            return Err(Error { status: DSPFX_ERR_INVALID, message: "a slider slice is not `count` long".into() });
        }
    }
    Ok(())
}

fn fptr(v: Option<&[f32]>) -> *const f32 {
    v.map_or(ptr::null(), |a| a.as_ptr())
}

impl ChannelGenerators {
    /// `tile_channels`: 0 (frame-major) or the engine's W.
    pub fn new(device: i32, channels: u32, tile_channels: u32, max_frames: u32) -> Result<Self, Error> {
        let desc = dspfx_gens_desc { abi_version: DSPFX_ABI_VERSION, device, n_channels: channels, max_frames, tile_channels };
        let mut h = ptr::null_mut();
        let rc = unsafe { dspfx_gens_create(&desc, &mut h) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_gens_create") });
        }
        Ok(ChannelGenerators { h, channels })
    }
    fn check(&self, rc: c_int, what: &str) -> Result<(), Error> {
        if rc == DSPFX_OK { Ok(()) } else { Err(Error { status: rc, message: reason(self.h, what) }) }
    }
    pub fn channels(&self) -> u32 { self.channels }
    /// The device bytes of a bank's tables (a pure host function).
    pub fn plan(channels: u64) -> Result<u64, Error> {
        let mut bytes = 0u64;
        let rc = unsafe { dspfx_gens_plan(channels, &mut bytes) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_gens_plan") });
        }
        Ok(bytes)
    }
    /// `n_frames` frames of every channel's generator into the DEVICE block `out` in the bank's layout.  `add_to`, `amplitude`,
    /// `frequency`: DEVICE blocks of the same shape or null -- the block the samples are added into (`out` may be `add_to`) and
    /// the two control ports.  Asynchronous on `stream`.
    pub unsafe fn run(&self, add_to: *const f32, amplitude: *const f32, frequency: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> Result<(), Error> {
        let rc = dspfx_gens_run(self.h, add_to, amplitude, frequency, out, n_frames, stream);
        self.check(rc, "dspfx_gens_run")
    }
    /// Gives `count` channels from `first_channel` a generator (any thread, never waits for the device): `amplitude`, `frequency`
    /// and `mode` (`DSPFX_SIG_*`), one value per channel each; `None` keeps a node's value.  An unknown mode refuses the whole store.
    pub fn set(&self, amplitude: Option<&[f32]>, frequency: Option<&[f32]>, mode: Option<&[u32]>, first_channel: u64, count: u64) -> Result<(), Error> {
        same_len(count, &[amplitude.map(|a| a.len()), frequency.map(|a| a.len()), mode.map(|a| a.len())])?;
        let m = mode.map_or(ptr::null(), |a| a.as_ptr());
        let rc = unsafe { dspfx_gens_set(self.h, fptr(amplitude), fptr(frequency), m, first_channel, count) };
        self.check(rc, "dspfx_gens_set")
    }
    /// Removes the node of `count` channels from `first_channel`: +0.0 again; a later `set` starts from the defaults at clock 0.
    pub fn drop_nodes(&self, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_gens_drop(self.h, first_channel, count) };
        self.check(rc, "dspfx_gens_drop")
    }
    /// The clocks of the range's nodes back to +0.0; sliders, modes and nodes stay.
    pub fn reset(&self, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_gens_reset(self.h, first_channel, count) };
        self.check(rc, "dspfx_gens_reset")
    }
    /// 1 / 0 per channel: it carries a node, as all stores made so far left it.
    pub fn present(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_gens_present(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_gens_present")?;
        Ok(m)
    }
    /// Per channel the node's `DSPFX_SIG_*` mode, `DSPFX_GENS_NONE` without a node.
    pub fn modes(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_gens_modes(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_gens_modes")?;
        Ok(m)
    }
    /// Amplitude and frequency per channel, 0 without a node.
    pub fn sliders(&self) -> Result<Vec<[f32; 2]>, Error> {
        let mut m = vec![[0f32; 2]; self.channels as usize];
        let rc = unsafe { dspfx_gens_sliders(self.h, m.as_mut_ptr() as *mut f32, 0, m.len() as u64) };
        self.check(rc, "dspfx_gens_sliders")?;
        Ok(m)
    }
    /// The DEVICE pointer of the `channels` clocks (valid after a run, on its stream).
    pub fn clocks(&self) -> Result<*const f32, Error> {
        let mut c = ptr::null();
        let rc = unsafe { dspfx_gens_clocks(self.h, &mut c) };
        self.check(rc, "dspfx_gens_clocks")?;
        Ok(c)
    }
}

impl Drop for ChannelGenerators {
    fn drop(&mut self) {
        unsafe {
            dspfx_gens_destroy(self.h);
        }
    }
}
