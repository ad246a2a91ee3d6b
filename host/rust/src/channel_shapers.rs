//! `ChannelShapers`: per-channel waveshapers over the channels of a bank (`dspfx_shapers_*`).
//!
//! In the reference every graph owns its own Distort (nodes/distort.rs), Overdrive (nodes/overdrive.rs) and Chebyshev
//! (nodes/chebyshev.rs) instances, each with its sliders and, for Distort, its mode combo box; an engine runs one setting for all
//! its channels.  Channel c of this bank carries ONE such node from the first `set_*` that names it until `drop_nodes`, and its
//! output is bit for bit what an engine whose chain is that node writes for the channel.  A `set_*` of another family than the
//! channel carries replaces its node, which starts from the reference's defaults for what the call leaves `None`; a `set_*` of the
//! same family keeps what it leaves `None`.  While a channel carries Fuzz, which is block-global over 128 frames, `n_frames` must
//! be a multiple of 128.  The GUI thread stores through `set_*`, which never wait for the device: the next `run` applies the
//! stores in order.  Several shapers per channel are several banks.
//! NOT compiled in the build container (no rustc).
use super::engine::Error;
use super::ffi::*;
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::ptr;

pub struct ChannelShapers {
    h: *mut dspfx_shapers,
    channels: u32,
}
unsafe impl Send for ChannelShapers {}
// runs are serialised by the bank's own lock; stores take the store lock and the store queue's
unsafe impl Sync for ChannelShapers {}

fn reason(h: *const dspfx_shapers, what: &str) -> String {
    let msg = unsafe { CStr::from_ptr(dspfx_shapers_last_error(h)) }.to_string_lossy().into_owned();
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

impl ChannelShapers {
    /// `tile_channels`: 0 (frame-major) or the engine's W.
    pub fn new(device: i32, channels: u32, tile_channels: u32, max_frames: u32) -> Result<Self, Error> {
        let desc = dspfx_shapers_desc { abi_version: DSPFX_ABI_VERSION, device, n_channels: channels, max_frames, tile_channels };
        let mut h = ptr::null_mut();
        let rc = unsafe { dspfx_shapers_create(&desc, &mut h) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_shapers_create") });
        }
        Ok(ChannelShapers { h, channels })
    }
    fn check(&self, rc: c_int, what: &str) -> Result<(), Error> {
        if rc == DSPFX_OK { Ok(()) } else { Err(Error { status: rc, message: reason(self.h, what) }) }
    }
    pub fn channels(&self) -> u32 { self.channels }
    /// The device bytes of a bank's tables (a pure host function).
    pub fn plan(channels: u64) -> Result<u64, Error> {
        let mut bytes = 0u64;
        let rc = unsafe { dspfx_shapers_plan(channels, &mut bytes) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_shapers_plan") });
        }
        Ok(bytes)
    }
    /// A DEVICE block of `n_frames` frames in the bank's layout through every channel's shaper into the DEVICE block `out` (`out`
    /// may be `input`: in place).  Asynchronous on `stream`.
    pub unsafe fn run(&self, input: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> Result<(), Error> {
        let rc = dspfx_shapers_run(self.h, input, out, n_frames, stream);
        self.check(rc, "dspfx_shapers_run")
    }
    /// Gives `count` channels from `first_channel` a Distort node (any thread, never waits for the device): `level` and `mode`
    /// (`DSPFX_DIST_*`), one value per channel each.  An unknown mode refuses the whole store.
    pub fn set_distort(&self, level: Option<&[f32]>, mode: Option<&[u32]>, first_channel: u64, count: u64) -> Result<(), Error> {
        same_len(count, &[level.map(|a| a.len()), mode.map(|a| a.len())])?;
        let m = mode.map_or(ptr::null(), |a| a.as_ptr());
        let rc = unsafe { dspfx_shapers_set_distort(self.h, fptr(level), m, first_channel, count) };
        self.check(rc, "dspfx_shapers_set_distort")
    }
    /// ... an Overdrive node: boost, drive, level.
    pub fn set_overdrive(&self, boost: Option<&[f32]>, drive: Option<&[f32]>, level: Option<&[f32]>, first_channel: u64, count: u64) -> Result<(), Error> {
        same_len(count, &[boost.map(|a| a.len()), drive.map(|a| a.len()), level.map(|a| a.len())])?;
        let rc = unsafe { dspfx_shapers_set_overdrive(self.h, fptr(boost), fptr(drive), fptr(level), first_channel, count) };
        self.check(rc, "dspfx_shapers_set_overdrive")
    }
    /// ... a Chebyshev node: level_pos, level_neg.
    pub fn set_chebyshev(&self, level_pos: Option<&[f32]>, level_neg: Option<&[f32]>, first_channel: u64, count: u64) -> Result<(), Error> {
        same_len(count, &[level_pos.map(|a| a.len()), level_neg.map(|a| a.len())])?;
        let rc = unsafe { dspfx_shapers_set_chebyshev(self.h, fptr(level_pos), fptr(level_neg), first_channel, count) };
        self.check(rc, "dspfx_shapers_set_chebyshev")
    }
    /// Removes the node of `count` channels from `first_channel`: a copy again; a later store starts from the defaults.
    pub fn drop_nodes(&self, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_shapers_drop(self.h, first_channel, count) };
        self.check(rc, "dspfx_shapers_drop")
    }
    /// 1 / 0 per channel: it carries a node, as all stores made so far left it.
    pub fn present(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_shapers_present(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_shapers_present")?;
        Ok(m)
    }
    /// Per channel `DSPFX_DISTORT`, `DSPFX_OVERDRIVE`, `DSPFX_CHEBYSHEV`, or `DSPFX_SHAPERS_NONE` without a node.
    pub fn kinds(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_shapers_kinds(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_shapers_kinds")?;
        Ok(m)
    }
    /// Per channel a Distort node's mode, `DSPFX_SHAPERS_NONE` for every other channel.
    pub fn modes(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_shapers_modes(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_shapers_modes")?;
        Ok(m)
    }
    /// Three sliders per channel in the order of `dspfx_node_desc.params`, 0 where the node has fewer and without a node.
    pub fn sliders(&self) -> Result<Vec<[f32; 3]>, Error> {
        let mut m = vec![[0f32; 3]; self.channels as usize];
        let rc = unsafe { dspfx_shapers_sliders(self.h, m.as_mut_ptr() as *mut f32, 0, m.len() as u64) };
        self.check(rc, "dspfx_shapers_sliders")?;
        Ok(m)
    }
}

impl Drop for ChannelShapers {
    fn drop(&mut self) {
        unsafe {
            dspfx_shapers_destroy(self.h);
        }
    }
}
