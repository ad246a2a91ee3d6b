//! `MixMatrix`: each listener's own mix of their room (`dspfx_mixmatrix_*`).
//!
//! In the reference every participant has an Output node of their own and wires it to whichever of the others they like through
//! Gain nodes of their own (output.rs:215-249, node.rs:162-194, gain.rs:25-38): a gain per (listener, source) pair.  Room r of n_r
//! contiguous channels owns an n_r x n_r matrix `M[l][s]`, and a DEVICE block gives
//! `out[f][c0 + l] = (sum_s M[l][s] * x[f][c0 + s]) / link_divisor(w)`, w = the listener's entries that are not zero.  A fresh bank
//! holds mix-minus, which is `MixGroups::returns` without faders; a host binds it between `ChannelStrips::run` and the listeners'
//! resampler when listeners need mixes of their own.  The GUI thread stores rows and columns, which never wait for the device: the
//! next `run` applies them in order, each whole.  A bank made by `new` has fixed rooms; one made by `with_seats` gives every room a
//! number of seats and follows live moves with `assign`, as `MixGroups::assign` does, without rebuilding a table.
//! NOT compiled in the build container (no rustc).
use super::engine::Error;
use super::ffi::*;
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::ptr;

pub struct MixMatrix {
    h: *mut dspfx_mixmatrix,
    channels: u32,
    rooms: u32,
}
unsafe impl Send for MixMatrix {}
// runs are serialised by the bank's own lock; stores only take the store queue's
unsafe impl Sync for MixMatrix {}

fn reason(h: *const dspfx_mixmatrix, what: &str) -> String {
    let msg = unsafe { CStr::from_ptr(dspfx_mixmatrix_last_error(h)) }.to_string_lossy().into_owned();
    if msg.is_empty() { what.into() } else { msg }
}

/// What `dspfx_mixmatrix_plan` reports: per room its members, the edge of its padded matrix and that matrix's element offset.
pub struct MixMatrixPlan {
    pub count: Vec<u32>,
    pub edge: Vec<u32>,
    pub offset: Vec<u64>,
    pub total_bytes: u64,
}

impl MixMatrix {
    /// `group_start`: G + 1 channel indices from 0 to `channels`, every room 1 ..= `DSPFX_MIXMATRIX_MAX_ROOM` members;
    /// `tile_channels`: 0 (frame-major) or the engine's W.
    pub fn new(device: i32, channels: u32, group_start: &[u64], tile_channels: u32, max_frames: u32, normalise: bool) -> Result<Self, Error> {
        let rooms = group_start.len().saturating_sub(1) as u32;
        let desc = dspfx_mixmatrix_desc {
            abi_version: DSPFX_ABI_VERSION,
            device,
            n_channels: channels,
            max_frames,
            tile_channels,
            n_groups: rooms,
            normalise: normalise as u32,
            group_start: group_start.as_ptr(),
        };
        let mut h = ptr::null_mut();
        let rc = unsafe { dspfx_mixmatrix_create(&desc, &mut h) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_mixmatrix_create") });
        }
        Ok(MixMatrix { h, channels, rooms })
    }
    /// A SEATED bank (`dspfx_mixmatrix_create_seats`): room r owns `seats[r]` seats (at least its members, rounded up to 32, at
    /// most `DSPFX_MIXMATRIX_MAX_ROOM`) and an S_r x S_r table that never moves; `assign` then reseats channels live.
    pub fn with_seats(device: i32, channels: u32, group_start: &[u64], seats: &[u32], tile_channels: u32, max_frames: u32, normalise: bool) -> Result<Self, Error> {
        let rooms = group_start.len().saturating_sub(1) as u32;
        if seats.len() != rooms as usize {
            return Err(Error { status: DSPFX_ERR_INVALID, message: "seats: one count per room".into() });
        }
        let desc = dspfx_mixmatrix_desc {
            abi_version: DSPFX_ABI_VERSION,
            device,
            n_channels: channels,
            max_frames,
            tile_channels,
            n_groups: rooms,
            normalise: normalise as u32,
            group_start: group_start.as_ptr(),
        };
        let mut h = ptr::null_mut();
        let rc = unsafe { dspfx_mixmatrix_create_seats(&desc, seats.as_ptr(), &mut h) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_mixmatrix_create_seats") });
        }
        Ok(MixMatrix { h, channels, rooms })
    }
    /// Seats channels `first_channel ..` in the rooms `ids` (each `< rooms()` or `DSPFX_MIXMATRIX_NO_ROOM`): those whose id is
    /// their room stay as they are, the others leave and then enter in ascending channel order, each into the lowest free seat,
    /// wired by `preset`.  A bad id or range, or a room over capacity, stores nothing.  Any thread; never waits for a run.
    pub fn assign(&self, ids: &[u32], first_channel: u64, preset: u32) -> Result<(), Error> {
        let rc = unsafe { dspfx_mixmatrix_assign(self.h, ids.as_ptr(), first_channel, ids.len() as u64, preset) };
        self.check(rc, "dspfx_mixmatrix_assign")
    }
    /// The room of every channel (`DSPFX_MIXMATRIX_NO_ROOM`: none) by every call made so far.
    pub fn room_of(&self) -> Result<Vec<u32>, Error> {
        let mut v = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_mixmatrix_rooms(self.h, v.as_mut_ptr(), 0, v.len() as u64) };
        self.check(rc, "dspfx_mixmatrix_rooms")?;
        Ok(v)
    }
    /// The seat of every channel in its room (`0xFFFF_FFFF`: in no room).
    pub fn seat_of(&self) -> Result<Vec<u32>, Error> {
        let mut v = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_mixmatrix_seats(self.h, v.as_mut_ptr(), 0, v.len() as u64) };
        self.check(rc, "dspfx_mixmatrix_seats")?;
        Ok(v)
    }
    /// The taken seats of every room.
    pub fn occupancy(&self) -> Result<Vec<u32>, Error> {
        let mut v = vec![0u32; self.rooms as usize];
        let rc = unsafe { dspfx_mixmatrix_occupancy(self.h, v.as_mut_ptr()) };
        self.check(rc, "dspfx_mixmatrix_occupancy")?;
        Ok(v)
    }
    /// `M[listeners[i]][sources[i]] = gains[i]` by channel number, in order; each pair two channels of one room.
    pub fn set_pairs(&self, listeners: &[u32], sources: &[u32], gains: &[f32]) -> Result<(), Error> {
        if listeners.len() != sources.len() || listeners.len() != gains.len() {
            return Err(Error { status: DSPFX_ERR_INVALID, message: "listeners, sources and gains are equally long".into() });
        }
        let rc = unsafe { dspfx_mixmatrix_set_pairs(self.h, listeners.as_ptr(), sources.as_ptr(), gains.as_ptr(), gains.len() as u64) };
        self.check(rc, "dspfx_mixmatrix_set_pairs")
    }
    /// The seating rule on host arrays (a pure host function): what `assign` does to the bank's tables.
    pub fn reseat(room_of: &mut [u32], seat_of: &mut [u32], seats: &[u32], ids: &[u32], first_channel: u64) -> Result<(), Error> {
        if room_of.len() != seat_of.len() {
            return Err(Error { status: DSPFX_ERR_INVALID, message: "room_of and seat_of are equally long".into() });
        }
        let rc = unsafe {
            dspfx_mixmatrix_reseat(room_of.as_mut_ptr(), seat_of.as_mut_ptr(), seats.as_ptr(), seats.len() as u32, room_of.len() as u64,
                                   ids.as_ptr(), first_channel, ids.len() as u64)
        };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_mixmatrix_reseat") });
        }
        Ok(())
    }
    /// A seated bank: the mode of the runs submitted after the call, `DSPFX_MIXMATRIX_DIRECT` or `DSPFX_MIXMATRIX_STAGED`.  Staged
    /// runs transpose the block into a seat-ordered copy, run the same chain over it and transpose back: the direct run's bits at a
    /// cost that does not depend on the seating, and `run` with `out == block` in place.  The first switch allocates
    /// `staging_bytes(..)` of device memory.  Any thread, while runs are in flight.
    pub fn set_staging(&self, mode: u32) -> Result<(), Error> {
        let rc = unsafe { dspfx_mixmatrix_set_staging(self.h, mode) };
        self.check(rc, "dspfx_mixmatrix_set_staging")
    }
    /// The mode of the next run.
    pub fn staging(&self) -> Result<u32, Error> {
        let mut mode = 0u32;
        let rc = unsafe { dspfx_mixmatrix_staging(self.h, &mut mode) };
        self.check(rc, "dspfx_mixmatrix_staging")?;
        Ok(mode)
    }
    /// The bytes `DSPFX_MIXMATRIX_STAGED` adds to the seated bank of this plan (a pure host function).
    pub fn staging_bytes(channels: u64, group_start: &[u64], seats: &[u32], tile_channels: u32, max_frames: u32) -> Result<u64, Error> {
        let g = group_start.len().saturating_sub(1);
        if seats.len() != g {
            return Err(Error { status: DSPFX_ERR_INVALID, message: "seats: one count per room".into() });
        }
        let mut bytes = 0u64;
        let rc = unsafe { dspfx_mixmatrix_staging_bytes(group_start.as_ptr(), g as u32, channels, tile_channels, seats.as_ptr(), max_frames, &mut bytes) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_mixmatrix_staging_bytes") });
        }
        Ok(bytes)
    }
    /// How scattered a seating is (a pure host function): `(chunks, lines)`, the runs of 32 seats that hold anybody and the lines of
    /// 32 adjacent channels they read per frame.  `lines / chunks` near 1: run direct; towards 32: run staged.
    pub fn scatter(room_of: &[u32], seat_of: &[u32], seats: &[u32]) -> Result<(u64, u64), Error> {
        if room_of.len() != seat_of.len() {
            return Err(Error { status: DSPFX_ERR_INVALID, message: "room_of and seat_of are equally long".into() });
        }
        let (mut chunks, mut lines) = (0u64, 0u64);
        let rc = unsafe {
            dspfx_mixmatrix_scatter(room_of.as_ptr(), seat_of.as_ptr(), seats.as_ptr(), seats.len() as u32, room_of.len() as u64, &mut chunks, &mut lines)
        };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_mixmatrix_scatter") });
        }
        Ok((chunks, lines))
    }
    /// `plan` for a seated bank: the edges are the seats rounded up to 32.
    pub fn plan_seats(channels: u64, group_start: &[u64], seats: &[u32], tile_channels: u32) -> Result<MixMatrixPlan, Error> {
        let g = group_start.len().saturating_sub(1);
        if seats.len() != g {
            return Err(Error { status: DSPFX_ERR_INVALID, message: "seats: one count per room".into() });
        }
        let mut p = MixMatrixPlan { count: vec![0; g], edge: vec![0; g], offset: vec![0; g], total_bytes: 0 };
        let rc = unsafe {
            dspfx_mixmatrix_plan_seats(group_start.as_ptr(), g as u32, channels, tile_channels, seats.as_ptr(), p.count.as_mut_ptr(),
                                       p.edge.as_mut_ptr(), p.offset.as_mut_ptr(), &mut p.total_bytes)
        };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_mixmatrix_plan_seats") });
        }
        Ok(p)
    }
    fn check(&self, rc: c_int, what: &str) -> Result<(), Error> {
        if rc == DSPFX_OK { Ok(()) } else { Err(Error { status: rc, message: reason(self.h, what) }) }
    }
    pub fn channels(&self) -> u32 { self.channels }
    pub fn rooms(&self) -> u32 { self.rooms }
    /// A DEVICE block of `n_frames` frames in the bank's layout through every room's matrix into the DEVICE block `out`, which
    /// may not overlap `block` (in `DSPFX_MIXMATRIX_STAGED` it may BE `block`).  Asynchronous on `stream`.
    pub unsafe fn run(&self, block: *const f32, n_frames: u32, out: *mut f32, stream: *mut c_void) -> Result<(), Error> {
        let rc = dspfx_mixmatrix_run(self.h, block, n_frames, out, stream);
        self.check(rc, "dspfx_mixmatrix_run")
    }
    /// The sparse run: room r adds only the sources named in `list[start[r] .. start[r] + count[r])` (DEVICE pointers: `i32` channel
    /// numbers, `start[rooms + 1]`, `count[rooms]`; `Talkers::audible` gives them), in ascending room-local order, and reads no
    /// other.  Where every unlisted source carries +-0.0 it is `run` bit for bit.  Entries that are negative, past the channels,
    /// at or past `list_len`, or of another room are ignored.  The list's producer and this run share a stream.
    pub unsafe fn run_sparse(&self, block: *const f32, n_frames: u32, out: *mut f32, list: *const i32, list_len: u64, start: *const u32, count: *const u32,
                             stream: *mut c_void) -> Result<(), Error> {
        let rc = dspfx_mixmatrix_run_sparse(self.h, block, n_frames, out, list, list_len, start, count, stream);
        self.check(rc, "dspfx_mixmatrix_run_sparse")
    }
    /// What listeners `first_channel ..` of one room hear: `values` is `[count][row_len]`, `row_len` the room's member count.
    pub fn set_rows(&self, values: &[f32], row_len: u32, first_channel: u64) -> Result<(), Error> {
        let count = if row_len == 0 { 0 } else { values.len() as u64 / row_len as u64 };
        let rc = unsafe { dspfx_mixmatrix_set_rows(self.h, values.as_ptr(), row_len, first_channel, count) };
        self.check(rc, "dspfx_mixmatrix_set_rows")
    }
    /// How loud sources `first_channel ..` are for each listener of their room: `values` is `[count][row_len]`.
    pub fn set_cols(&self, values: &[f32], row_len: u32, first_channel: u64) -> Result<(), Error> {
        let count = if row_len == 0 { 0 } else { values.len() as u64 / row_len as u64 };
        let rc = unsafe { dspfx_mixmatrix_set_cols(self.h, values.as_ptr(), row_len, first_channel, count) };
        self.check(rc, "dspfx_mixmatrix_set_cols")
    }
    /// Room `room` (`None`: every room) back to `DSPFX_MIXMATRIX_MIX_MINUS` or `DSPFX_MIXMATRIX_ZERO`.
    pub fn fill(&self, room: Option<u32>, preset: u32) -> Result<(), Error> {
        let rc = unsafe { dspfx_mixmatrix_fill(self.h, room.map_or(-1, |r| r as i64), preset) };
        self.check(rc, "dspfx_mixmatrix_fill")
    }
    /// The fresh state: mix-minus in every room.
    pub fn reset(&self) -> Result<(), Error> {
        let rc = unsafe { dspfx_mixmatrix_reset(self.h) };
        self.check(rc, "dspfx_mixmatrix_reset")
    }
    /// The table's plan without a GPU (a pure host function); `Err` with the reason for a table `new` would refuse.
    pub fn plan(channels: u64, group_start: &[u64], tile_channels: u32) -> Result<MixMatrixPlan, Error> {
        let g = group_start.len().saturating_sub(1);
        let mut p = MixMatrixPlan { count: vec![0; g], edge: vec![0; g], offset: vec![0; g], total_bytes: 0 };
        let rc = unsafe {
            dspfx_mixmatrix_plan(group_start.as_ptr(), g as u32, channels, tile_channels, p.count.as_mut_ptr(), p.edge.as_mut_ptr(),
                                 p.offset.as_mut_ptr(), &mut p.total_bytes)
        };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_mixmatrix_plan") });
        }
        Ok(p)
    }
}

impl Drop for MixMatrix {
    fn drop(&mut self) {
        unsafe {
            dspfx_mixmatrix_destroy(self.h);
        }
    }
}
