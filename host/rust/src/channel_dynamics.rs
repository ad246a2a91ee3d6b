//! `ChannelDynamics`: per-channel levellers and limiters over the channels of a bank (`dspfx_dynamics_*`).
//!
//! In the reference every graph owns its Envelope node (nodes/envelope.rs) and may feed slider ports from it: an Envelope into a
//! Gain.  `Talkers` uses that as a gate; this bank is the ordinary use, where the envelope turns the gain DOWN.  Channel c carries
//! its own node from the first `set` that names it until `drop_nodes`: `q = env > threshold ? threshold / env : 1`,
//! `out = in * (makeup * q)`.  A host binds one bank ahead of `Talkers` as a leveller (`threshold = target / max_gain`,
//! `makeup = max_gain`) and one behind `MixGroups` / `MixMatrix` as a limiter (`threshold` = the ceiling, attack 0: a brick wall).
//! The GUI thread stores sliders through `set`, which never waits for the device: the next `run` applies the stores in order.
//! NOT compiled in the build container (no rustc).
use super::engine::Error;
use super::ffi::*;
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::ptr;

pub struct ChannelDynamics {
    h: *mut dspfx_dynamics,
    channels: u32,
}
unsafe impl Send for ChannelDynamics {}
// runs are serialised by the bank's own lock; slider stores take the store lock and the store queue's
unsafe impl Sync for ChannelDynamics {}

/// The device tables of a bank: valid after a run, on its stream.
pub struct DynamicsViews {
    pub level: *const f32,
    pub reduction: *const f32,
}

/// The four sliders of a store, one value per channel each; `None` keeps each channel's value.
#[derive(Default, Clone, Copy)]
pub struct DynamicsSliders<'a> {
    pub threshold: Option<&'a [f32]>,
    pub makeup: Option<&'a [f32]>,
    pub attack: Option<&'a [f32]>,
    pub release: Option<&'a [f32]>,
}

fn reason(h: *const dspfx_dynamics, what: &str) -> String {
    let msg = unsafe { CStr::from_ptr(dspfx_dynamics_last_error(h)) }.to_string_lossy().into_owned();
    if msg.is_empty() { what.into() } else { msg }
}

impl ChannelDynamics {
    /// `tile_channels`: 0 (frame-major) or the engine's W.
    pub fn new(device: i32, channels: u32, tile_channels: u32, max_frames: u32) -> Result<Self, Error> {
        let desc = dspfx_dynamics_desc { abi_version: DSPFX_ABI_VERSION, device, n_channels: channels, max_frames, tile_channels };
        let mut h = ptr::null_mut();
        let rc = unsafe { dspfx_dynamics_create(&desc, &mut h) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_dynamics_create") });
        }
        Ok(ChannelDynamics { h, channels })
    }
    fn check(&self, rc: c_int, what: &str) -> Result<(), Error> {
        if rc == DSPFX_OK { Ok(()) } else { Err(Error { status: rc, message: reason(self.h, what) }) }
    }
    pub fn channels(&self) -> u32 { self.channels }
    /// The device bytes of a bank's tables (a pure host function).
    pub fn plan(channels: u64) -> Result<u64, Error> {
        let mut bytes = 0u64;
        let rc = unsafe { dspfx_dynamics_plan(channels, &mut bytes) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_dynamics_plan") });
        }
        Ok(bytes)
    }
    /// `(makeup * q, q)` for one envelope value: the factor a run multiplies the sample by (a pure host function).
    pub fn gain(env: f32, threshold: f32, makeup: f32) -> (f32, f32) {
        let mut q = 1.0f32;
        let g = unsafe { dspfx_dynamics_gain(env, threshold, makeup, &mut q) };
        (g, q)
    }
    /// A DEVICE block of `n_frames` frames in the bank's layout through every channel's dynamics into the DEVICE block `out`
    /// (`out` may be `input`: in place).  `key`, a DEVICE block of the same shape or null, is what the detector follows instead of
    /// `input`.  Asynchronous on `stream`.
    pub unsafe fn run(&self, input: *const f32, key: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> Result<(), Error> {
        let rc = dspfx_dynamics_run(self.h, input, key, out, n_frames, stream);
        self.check(rc, "dspfx_dynamics_run")
    }
    /// Stores the sliders of `count` channels from `first_channel` and gives each of them its node (any thread, never waits for
    /// the device).  No envelope is touched.  Refused whole on a threshold that is NaN or below +0.0, a makeup that is NaN,
    /// infinite or negative, or slices that are not `count` long.
    pub fn set(&self, s: DynamicsSliders, first_channel: u64, count: u64) -> Result<(), Error> {
        for v in [s.threshold, s.makeup, s.attack, s.release].iter().flatten() {
            if v.len() as u64 != count {
                return Err(Error { status: DSPFX_ERR_INVALID, message: "a slider slice is not `count` long".into() });
            }
        }
        let p = |v: Option<&[f32]>| v.map_or(ptr::null(), |a| a.as_ptr());
        let rc = unsafe { dspfx_dynamics_set(self.h, p(s.threshold), p(s.makeup), p(s.attack), p(s.release), first_channel, count) };
        self.check(rc, "dspfx_dynamics_set")
    }
    /// Removes the node of `count` channels from `first_channel` and clears their envelope; a later store starts from the defaults.
    pub fn drop_nodes(&self, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_dynamics_drop(self.h, first_channel, count) };
        self.check(rc, "dspfx_dynamics_drop")
    }
    /// Envelope and level back to 0 and reduction to 1 on the range; the sliders and the nodes stay; queued like a store.
    pub fn reset(&self, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_dynamics_reset(self.h, first_channel, count) };
        self.check(rc, "dspfx_dynamics_reset")
    }
    /// 1 / 0 per channel: it carries a node, as all stores made so far left it.
    pub fn present(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_dynamics_present(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_dynamics_present")?;
        Ok(m)
    }
    /// The device pointers of level[N] and reduction[N].
    pub fn views(&self) -> Result<DynamicsViews, Error> {
        let mut v = DynamicsViews { level: ptr::null(), reduction: ptr::null() };
        let rc = unsafe { dspfx_dynamics_views(self.h, &mut v.level, &mut v.reduction) };
        self.check(rc, "dspfx_dynamics_views")?;
        Ok(v)
    }
}

impl Drop for ChannelDynamics {
    fn drop(&mut self) {
        unsafe {
            dspfx_dynamics_destroy(self.h);
        }
    }
}
