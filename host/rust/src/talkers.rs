//! `Talkers`: per-channel levels and each room's loudest, gated live, over the channels of a bank (`dspfx_talkers_*`).
//!
//! In the reference every graph owns its Envelope node (nodes/envelope.rs) and may feed slider ports from it: an Envelope into a
//! Gain.  A host with one participant per channel binds one `Talkers` over the bank's DEVICE block, behind `ChannelStrips` and
//! `ChannelDelays` and ahead of `MixGroups` / `MixMatrix`: every channel has its own attack and release, every room gets its `top`
//! loudest members chosen on the device, and `run` passes those members and ramps the others out.  A run gates with the targets
//! the run before left, then meters, then selects, so a selection is audible one block later.  The GUI thread stores sliders, pins
//! and seats through the setters, which never wait for the device: the next `run` applies them in order.
//! NOT compiled in the build container (no rustc).
use super::engine::Error;
use super::ffi::*;
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::ptr;

pub struct Talkers {
    h: *mut dspfx_talkers,
    channels: u32,
    groups: u32,
}
unsafe impl Send for Talkers {}
// runs are serialised by the bank's own lock; stores take the store lock and the store queue's
unsafe impl Sync for Talkers {}

/// The device tables of a bank: valid after a run, on its stream.
pub struct TalkerViews {
    pub level: *const f32,
    pub target: *const f32,
    pub talkers: *const i32,
    pub talker_levels: *const f32,
}

/// The device tables of the audible list (`Talkers::audible`): `list[N]`, `start[G + 1]`, `count[G]`.
pub struct AudibleViews {
    pub list: *const i32,
    pub start: *const u32,
    pub count: *const u32,
}

fn reason(h: *const dspfx_talkers, what: &str) -> String {
    let msg = unsafe { CStr::from_ptr(dspfx_talkers_last_error(h)) }.to_string_lossy().into_owned();
    if msg.is_empty() { what.into() } else { msg }
}

impl Talkers {
    /// `group_start`: G + 1 channel indices, rooms of 1 ..= `DSPFX_TALKERS_MAX_ROOM` members; `top`: every room's top until `set_top`;
    /// `tile_channels`: 0 (frame-major) or the engine's W.
    pub fn new(device: i32, channels: u32, group_start: &[u64], top: u32, tile_channels: u32, max_frames: u32) -> Result<Self, Error> {
        let groups = group_start.len().saturating_sub(1) as u32;
        let desc = dspfx_talkers_desc { abi_version: DSPFX_ABI_VERSION, device, n_channels: channels, max_frames, tile_channels, n_groups: groups, top, group_start: group_start.as_ptr() };
        let mut h = ptr::null_mut();
        let rc = unsafe { dspfx_talkers_create(&desc, &mut h) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_talkers_create") });
        }
        Ok(Talkers { h, channels, groups })
    }
    fn check(&self, rc: c_int, what: &str) -> Result<(), Error> {
        if rc == DSPFX_OK { Ok(()) } else { Err(Error { status: rc, message: reason(self.h, what) }) }
    }
    pub fn channels(&self) -> u32 { self.channels }
    pub fn groups(&self) -> u32 { self.groups }
    /// Attack or release frames -> the detector's gain (a pure host function).
    pub fn envelope_gain(frames: f32) -> f32 {
        unsafe { dspfx_envelope_gain(frames) }
    }
    /// The device bytes of a bank's tables (a pure host function).
    pub fn plan(channels: u64, groups: u32) -> Result<u64, Error> {
        let mut bytes = 0u64;
        let rc = unsafe { dspfx_talkers_plan(channels, groups, &mut bytes) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_talkers_plan") });
        }
        Ok(bytes)
    }
    /// A DEVICE block of `n_frames` frames in the bank's layout through the gate into the DEVICE block `out` (`out` may be `input`:
    /// in place; null: meter and select only, the gates stay).  Asynchronous on `stream`.
    pub unsafe fn run(&self, input: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> Result<(), Error> {
        let rc = dspfx_talkers_run(self.h, input, out, n_frames, stream);
        self.check(rc, "dspfx_talkers_run")
    }
    /// Seats channels `first_channel ..` in the rooms `ids` (each below `groups()`, or `DSPFX_TALKERS_NO_ROOM`).  Refused whole on a
    /// bad id or a room that would exceed `DSPFX_TALKERS_MAX_ROOM`.  Any thread, never waits for the device.
    pub fn assign(&self, ids: &[u32], first_channel: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_talkers_assign(self.h, ids.as_ptr(), first_channel, ids.len() as u64) };
        self.check(rc, "dspfx_talkers_assign")
    }
    /// Stores attack and release (frames) of channels `first_channel ..`, one value per channel; `None` keeps each channel's value.
    /// No envelope is touched.
    pub fn set_detector(&self, attack: Option<&[f32]>, release: Option<&[f32]>, first_channel: u64) -> Result<(), Error> {
        let count = match (attack, release) {
            (Some(a), Some(r)) if a.len() != r.len() => return Err(Error { status: DSPFX_ERR_INVALID, message: "attack and release name different numbers of channels".into() }),
            (Some(a), _) => a.len(),
            (None, Some(r)) => r.len(),
            (None, None) => 0,
        };
        let rc = unsafe { dspfx_talkers_set_detector(self.h, attack.map_or(ptr::null(), |a| a.as_ptr()), release.map_or(ptr::null(), |r| r.as_ptr()), first_channel, count as u64) };
        self.check(rc, "dspfx_talkers_set_detector")
    }
    /// `DSPFX_TALKERS_AUTO`, `_OPEN` (always passed, never ranked) or `_SHUT` (never passed) per channel from `first_channel`.
    pub fn set_pin(&self, pins: &[u8], first_channel: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_talkers_set_pin(self.h, pins.as_ptr(), first_channel, pins.len() as u64) };
        self.check(rc, "dspfx_talkers_set_pin")
    }
    /// 1 ..= `DSPFX_TALKERS_MAX_TOP` per room from `first_room`.
    pub fn set_top(&self, tops: &[u8], first_room: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_talkers_set_top(self.h, tops.as_ptr(), first_room, tops.len() as u64) };
        self.check(rc, "dspfx_talkers_set_top")
    }
    /// Only a level strictly above the floor makes a candidate.
    pub fn set_floor(&self, floor: f32) -> Result<(), Error> {
        let rc = unsafe { dspfx_talkers_set_floor(self.h, floor) };
        self.check(rc, "dspfx_talkers_set_floor")
    }
    /// Envelope and level back to 0, gate and target to 1 on the range; queued like a store.
    pub fn reset(&self, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_talkers_reset(self.h, first_channel, count) };
        self.check(rc, "dspfx_talkers_reset")
    }
    /// The device pointers of level[N], target[N], talkers[G][8] and talker_levels[G][8].
    pub fn views(&self) -> Result<TalkerViews, Error> {
        let mut v = TalkerViews { level: ptr::null(), target: ptr::null(), talkers: ptr::null(), talker_levels: ptr::null() };
        let rc = unsafe { dspfx_talkers_views(self.h, &mut v.level, &mut v.target, &mut v.talkers, &mut v.talker_levels) };
        self.check(rc, "dspfx_talkers_views")?;
        Ok(v)
    }
    /// The audible list on the device: room r's members whose gate or target was not +-0.0 when the last gated run began, in
    /// ascending channel order, are `list[start[r] .. start[r] + count[r])`.  The first call allocates `list[N]` and `count[G]` and
    /// switches the bank on: every gated run submitted after it also writes them.  The pointers are stable for the life of the
    /// bank; what they hold is valid after a gated run, on its stream.  What `MixMatrix::run_sparse` takes.
    pub fn audible(&self) -> Result<AudibleViews, Error> {
        let mut v = AudibleViews { list: ptr::null(), start: ptr::null(), count: ptr::null() };
        let rc = unsafe { dspfx_talkers_audible_views(self.h, &mut v.list, &mut v.start, &mut v.count) };
        self.check(rc, "dspfx_talkers_audible_views")?;
        Ok(v)
    }
    /// The audible rule on host arrays (a pure host function): `(list[N], start[groups + 1], count[groups])`.
    pub fn audible_of(gate: &[f32], target: &[f32], room_of: &[u32], groups: u32) -> Result<(Vec<i32>, Vec<u32>, Vec<u32>), Error> {
        if gate.len() != target.len() || gate.len() != room_of.len() {
            return Err(Error { status: DSPFX_ERR_INVALID, message: "gate, target and room_of are equally long".into() });
        }
        let (mut list, mut start, mut count) = (vec![-1i32; gate.len()], vec![0u32; groups as usize + 1], vec![0u32; groups as usize]);
        let rc = unsafe {
            dspfx_talkers_audible(gate.as_ptr(), target.as_ptr(), room_of.as_ptr(), gate.len() as u64, groups, list.as_mut_ptr(), start.as_mut_ptr(), count.as_mut_ptr())
        };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_talkers_audible") });
        }
        Ok((list, start, count))
    }
    /// Every channel's room (`DSPFX_TALKERS_NO_ROOM`: none), by every assign made so far.
    pub fn room_of(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_talkers_room_of(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_talkers_room_of")?;
        Ok(m)
    }
    /// Every room's member count.
    pub fn counts(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.groups as usize];
        let rc = unsafe { dspfx_talkers_counts(self.h, m.as_mut_ptr()) };
        self.check(rc, "dspfx_talkers_counts")?;
        Ok(m)
    }
}

impl Drop for Talkers {
    fn drop(&mut self) {
        unsafe {
            dspfx_talkers_destroy(self.h);
        }
    }
}
