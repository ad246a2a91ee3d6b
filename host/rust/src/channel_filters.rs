//! `ChannelFilters`: per-channel one-pole filters and envelope followers over the channels of a bank (`dspfx_filters_*`).
//!
//! The three chain nodes that carry one float of state -- LowPass (nodes/low_pass.rs), HighPass (nodes/high_pass.rs) and Envelope
//! (nodes/envelope.rs, as a node whose output is the envelope) -- per channel: channel c owns `stages` slots (1 .. 4), run in slot
//! order, each empty or one of the three with its own sliders, and its output is bit for bit what an engine whose chain is its
//! present nodes in slot order writes for the channel, however the frames are cut into runs.  A slot's node is new (state +0.0, the
//! reference's defaults for what the call leaves `None`) from the first `set_*` that names it and after a `set_*` of another kind;
//! a `set_*` of the kind it carries keeps what the call leaves `None` and keeps the state.  The GUI thread stores through `set_*`,
//! which never wait for the device: the next `run` applies the stores in order.
//! NOT compiled in the build container (no rustc).
use super::engine::Error;
use super::ffi::*;
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::ptr;

pub struct ChannelFilters {
    h: *mut dspfx_filters,
    channels: u32,
    stages: u32,
}
unsafe impl Send for ChannelFilters {}
// runs are serialised by the bank's own lock; stores take the store lock and the store queue's
unsafe impl Sync for ChannelFilters {}

fn reason(h: *const dspfx_filters, what: &str) -> String {
    let msg = unsafe { CStr::from_ptr(dspfx_filters_last_error(h)) }.to_string_lossy().into_owned();
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

impl ChannelFilters {
    /// `stages`: the slots per channel, 1 .. 4; `tile_channels`: 0 (frame-major) or the engine's W.
    pub fn new(device: i32, channels: u32, stages: u32, tile_channels: u32, max_frames: u32) -> Result<Self, Error> {
        let desc = dspfx_filters_desc { abi_version: DSPFX_ABI_VERSION, device, n_channels: channels, max_frames, tile_channels, stages };
        let mut h = ptr::null_mut();
        let rc = unsafe { dspfx_filters_create(&desc, &mut h) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_filters_create") });
        }
        Ok(ChannelFilters { h, channels, stages })
    }
    fn check(&self, rc: c_int, what: &str) -> Result<(), Error> {
        if rc == DSPFX_OK { Ok(()) } else { Err(Error { status: rc, message: reason(self.h, what) }) }
    }
    pub fn channels(&self) -> u32 { self.channels }
    pub fn stages(&self) -> u32 { self.stages }
    /// The device bytes of a bank's tables (a pure host function).
    pub fn plan(channels: u64, stages: u32) -> Result<u64, Error> {
        let mut bytes = 0u64;
        let rc = unsafe { dspfx_filters_plan(channels, stages, &mut bytes) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_filters_plan") });
        }
        Ok(bytes)
    }
    /// A DEVICE block of `n_frames` frames in the bank's layout through every channel's slots into the DEVICE block `out` (`out`
    /// may be `input`: in place).  Asynchronous on `stream`.
    pub unsafe fn run(&self, input: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> Result<(), Error> {
        let rc = dspfx_filters_run(self.h, input, out, n_frames, stream);
        self.check(rc, "dspfx_filters_run")
    }
    /// Gives slot `stage` of `count` channels from `first_channel` a LowPass node (any thread, never waits for the device):
    /// `ratio`, one value per channel.
    pub fn set_low_pass(&self, stage: u32, ratio: Option<&[f32]>, first_channel: u64, count: u64) -> Result<(), Error> {
        same_len(count, &[ratio.map(|a| a.len())])?;
        let rc = unsafe { dspfx_filters_set_low_pass(self.h, stage, fptr(ratio), first_channel, count) };
        self.check(rc, "dspfx_filters_set_low_pass")
    }
    /// ... a HighPass node.
    pub fn set_high_pass(&self, stage: u32, ratio: Option<&[f32]>, first_channel: u64, count: u64) -> Result<(), Error> {
        same_len(count, &[ratio.map(|a| a.len())])?;
        let rc = unsafe { dspfx_filters_set_high_pass(self.h, stage, fptr(ratio), first_channel, count) };
        self.check(rc, "dspfx_filters_set_high_pass")
    }
    /// ... an Envelope node: attack and release in frames.
    pub fn set_envelope(&self, stage: u32, attack: Option<&[f32]>, release: Option<&[f32]>, first_channel: u64, count: u64) -> Result<(), Error> {
        same_len(count, &[attack.map(|a| a.len()), release.map(|a| a.len())])?;
        let rc = unsafe { dspfx_filters_set_envelope(self.h, stage, fptr(attack), fptr(release), first_channel, count) };
        self.check(rc, "dspfx_filters_set_envelope")
    }
    /// Empties slot `stage` of `count` channels from `first_channel` and zeroes its state: that stage copies again.
    pub fn drop_nodes(&self, stage: u32, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_filters_drop(self.h, stage, first_channel, count) };
        self.check(rc, "dspfx_filters_drop")
    }
    /// The state of slot `stage` (`None`: of every slot) back to +0.0; the nodes and the sliders stay.
    pub fn reset(&self, stage: Option<u32>, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_filters_reset(self.h, stage.unwrap_or(DSPFX_FILTERS_NONE), first_channel, count) };
        self.check(rc, "dspfx_filters_reset")
    }
    /// 1 / 0 per channel: a slot of it carries a node, as all stores made so far left it.
    pub fn present(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_filters_present(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_filters_present")?;
        Ok(m)
    }
    /// Per channel slot `stage`'s `DSPFX_LOW_PASS`, `DSPFX_HIGH_PASS`, `DSPFX_ENVELOPE`, or `DSPFX_FILTERS_NONE` when empty.
    pub fn kinds(&self, stage: u32) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_filters_kinds(self.h, stage, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_filters_kinds")?;
        Ok(m)
    }
    /// Per channel slot `stage`'s two sliders as they were given: ratio, 0 | attack, release (frames); 0, 0 when empty.
    pub fn sliders(&self, stage: u32) -> Result<Vec<[f32; 2]>, Error> {
        let mut m = vec![[0f32; 2]; self.channels as usize];
        let rc = unsafe { dspfx_filters_sliders(self.h, stage, m.as_mut_ptr() as *mut f32, 0, m.len() as u64) };
        self.check(rc, "dspfx_filters_sliders")?;
        Ok(m)
    }
    /// The DEVICE pointer of slot `stage`'s state, `channels` floats: valid after a run, on its stream.
    pub fn state(&self, stage: u32) -> Result<*const f32, Error> {
        let mut p = ptr::null();
        let rc = unsafe { dspfx_filters_state(self.h, stage, &mut p) };
        self.check(rc, "dspfx_filters_state")?;
        Ok(p)
    }
}

impl Drop for ChannelFilters {
    fn drop(&mut self) {
        unsafe {
            dspfx_filters_destroy(self.h);
        }
    }
}
