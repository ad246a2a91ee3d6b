//! `MixGroups`: one Output bus per contiguous channel range of a bank, with a per-channel fader (`dspfx_mixgroups_*`).
//!
//! The reference allows any number of Output nodes, each averaging the pipes wired to it (nodes/output.rs:215-249 feeding
//! collect_and_average, node.rs:162-194).  A host with R rooms of channels in one `GpuBank` binds one `MixGroups` over the bank's
//! DEVICE output block: `buses[f][g] = (sum over room g of x[f][c] * gain[c]) / f32(0.0001 + n_g)`, `[n_frames][G]` on the
//! device -- the frame-major block of a G-channel `Engine` (the master-bus chain), `Resampler`, `PitchBank` or `SpectrumBank`.
//! The GUI thread stores faders through `set_gains`, which never waits for the device: the next `run` applies them in order.
//! NOT compiled in the build container (no rustc).
use super::engine::Error;
use super::ffi::*;
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::ptr;

pub struct MixGroups {
    h: *mut dspfx_mixgroups,
    channels: u32,
    groups: u32,
}
unsafe impl Send for MixGroups {}
// runs are serialised by the bank's own lock; fader stores only take the store queue's, a seating change its own and then the bank's
unsafe impl Sync for MixGroups {}

fn reason(h: *const dspfx_mixgroups, what: &str) -> String {
    let msg = unsafe { CStr::from_ptr(dspfx_mixgroups_last_error(h)) }.to_string_lossy().into_owned();
    if msg.is_empty() { what.into() } else { msg }
}

impl MixGroups {
    /// `group_start`: G + 1 channel indices, nondecreasing, from 0 to `channels`; `tile_channels`: 0 (frame-major) or the engine's W;
    /// `normalise = false` leaves the raw sums (a group split over ranks).
    pub fn new(device: i32, channels: u32, tile_channels: u32, max_frames: u32, group_start: &[u64], normalise: bool) -> Result<Self, Error> {
        if group_start.len() < 2 {
            return Err(Error { status: DSPFX_ERR_INVALID, message: "MixGroups: group_start holds G + 1 entries".into() });
        }
        let groups = (group_start.len() - 1) as u32;
        let desc = dspfx_mixgroups_desc {
            abi_version: DSPFX_ABI_VERSION,
            device,
            n_channels: channels,
            max_frames,
            tile_channels,
            n_groups: groups,
            normalise: normalise as u32,
            group_start: group_start.as_ptr(),
        };
        let mut h = ptr::null_mut();
        let rc = unsafe { dspfx_mixgroups_create(&desc, &mut h) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_mixgroups_create") });
        }
        Ok(MixGroups { h, channels, groups })
    }
    fn check(&self, rc: c_int, what: &str) -> Result<(), Error> {
        if rc == DSPFX_OK { Ok(()) } else { Err(Error { status: rc, message: reason(self.h, what) }) }
    }
    pub fn channels(&self) -> u32 { self.channels }
    pub fn groups(&self) -> u32 { self.groups }
    /// The buses of a DEVICE block of `n_frames` frames in the bank's layout into the DEVICE array `buses`, `[n_frames][G]`.
    /// Asynchronous on `stream`.
    pub unsafe fn run(&self, block: *const f32, n_frames: u32, buses: *mut f32, stream: *mut c_void) -> Result<(), Error> {
        let rc = dspfx_mixgroups_run(self.h, block, n_frames, buses, stream);
        self.check(rc, "dspfx_mixgroups_run")
    }
    /// Every channel's room minus itself (`dspfx_mixgroups_returns`): the DEVICE block `returns`, in the bank's layout, receives
    /// `(S[f][g] - x[f][c] * gain[c]) / link_divisor(n_g - 1)`, +0.0 in a group of one.  `returns` may be `block` itself (in place);
    /// any other overlap is undefined.  `buses` is null or a DEVICE array `[n_frames][G]` that receives what `run` writes.
    pub unsafe fn returns(&self, block: *const f32, n_frames: u32, buses: *mut f32, returns: *mut f32, stream: *mut c_void) -> Result<(), Error> {
        let rc = dspfx_mixgroups_returns(self.h, block, n_frames, buses, returns, stream);
        self.check(rc, "dspfx_mixgroups_returns")
    }
    /// Stores the faders of channels `first_channel ..` (any thread, never waits for the device); they govern the runs submitted later.
    pub fn set_gains(&self, values: &[f32], first_channel: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_mixgroups_set_gains(self.h, values.as_ptr(), first_channel, values.len() as u64) };
        self.check(rc, "dspfx_mixgroups_set_gains")
    }
    /// Drops the faders of `count` channels from `first_channel`: back to "not multiplied".
    pub fn clear_gains(&self, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_mixgroups_set_gains(self.h, ptr::null(), first_channel, count) };
        self.check(rc, "dspfx_mixgroups_set_gains")
    }
    /// Seats channels `first_channel ..` in the rooms `ids` (each `< groups()` or `DSPFX_MIXGROUPS_NO_ROOM`); a bad id or range
    /// stores nothing.  Any thread, while runs are in flight: it holds for the runs submitted after it returns.  The channels'
    /// faders, and their state in the engine, stay where they are: a participant changes rooms without a click.
    pub fn assign(&self, ids: &[u32], first_channel: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_mixgroups_assign(self.h, ids.as_ptr(), first_channel, ids.len() as u64) };
        self.check(rc, "dspfx_mixgroups_assign")
    }
    /// The room of every channel as the next run sees it.
    pub fn room_of(&self) -> Result<Vec<u32>, Error> {
        let mut ids = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_mixgroups_rooms(self.h, ids.as_mut_ptr(), 0, ids.len() as u64) };
        self.check(rc, "dspfx_mixgroups_rooms")?;
        Ok(ids)
    }
    /// Checks a map (a room id or `DSPFX_MIXGROUPS_NO_ROOM` per channel) and gives, per room, (member count, depth D of its sum
    /// in mapped mode, pieces); a pure host function.
    pub fn room_plan(room_of: &[u32], groups: u32, tile_channels: u32) -> Result<(Vec<u64>, Vec<u32>, Vec<u64>), Error> {
        let g = groups as usize;
        let (mut count, mut depth, mut pieces) = (vec![0u64; g], vec![0u32; g], vec![0u64; g]);
        let rc = unsafe {
            dspfx_mixgroups_room_plan(room_of.as_ptr(), room_of.len() as u64, groups, tile_channels, count.as_mut_ptr(), depth.as_mut_ptr(), pieces.as_mut_ptr())
        };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_mixgroups_room_plan") });
        }
        Ok((count, depth, pieces))
    }
    /// Checks a table and gives, per group, the longest chain of dependent f32 additions in its sum (a pure host function).
    pub fn plan(group_start: &[u64], channels: u64, tile_channels: u32) -> Result<Vec<u32>, Error> {
        if group_start.len() < 2 {
            return Err(Error { status: DSPFX_ERR_INVALID, message: "dspfx_mixgroups_plan".into() });
        }
        let mut depth = vec![0u32; group_start.len() - 1];
        let rc = unsafe { dspfx_mixgroups_plan(group_start.as_ptr(), depth.len() as u32, channels, tile_channels, depth.as_mut_ptr()) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_mixgroups_plan") });
        }
        Ok(depth)
    }
}

impl Drop for MixGroups {
    fn drop(&mut self) {
        unsafe {
            dspfx_mixgroups_destroy(self.h);
        }
    }
}
