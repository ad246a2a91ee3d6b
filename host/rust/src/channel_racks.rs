//! `ChannelRacks`: a per-channel chain of mixed nodes in one pass over the channels of a bank (`dspfx_racks_*`).
//!
//! Channel c owns `slots` slots (1 .. 4), run in slot order, each empty or any one of Gain, BiQuad, LowPass, HighPass, Envelope,
//! Distort (every mode but Fuzz), Overdrive and Chebyshev with its own sliders and state; all slots run between one load and one
//! store of the block.  A channel's output and state are bit for bit what the filters, strips and shapers banks give when they are
//! run slot after slot with the slot's node on that channel.  A `set` of a kind the slot does not carry makes a new node (state
//! +0.0, the reference's defaults for what the call leaves `None`); a `set` of the kind it carries keeps what is `None`, keeps the
//! state of LowPass, HighPass and Envelope and zeroes a BiQuad's.  The GUI thread stores through `set`, which never waits for the
//! device: the next `run` applies the stores in order.
//! NOT compiled in the build container (no rustc).
use super::engine::Error;
use super::ffi::*;
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::ptr;

pub struct ChannelRacks {
    h: *mut dspfx_racks,
    channels: u32,
    slots: u32,
}
unsafe impl Send for ChannelRacks {}
// runs are serialised by the bank's own lock; stores take the store lock and the store queue's
unsafe impl Sync for ChannelRacks {}

fn reason(h: *const dspfx_racks, what: &str) -> String {
    let msg = unsafe { CStr::from_ptr(dspfx_racks_last_error(h)) }.to_string_lossy().into_owned();
    if msg.is_empty() { what.into() } else { msg }
}

impl ChannelRacks {
    /// `slots`: the slots per channel, 1 .. 4; `tile_channels`: 0 (frame-major) or the engine's W.
    pub fn new(device: i32, channels: u32, slots: u32, tile_channels: u32, max_frames: u32) -> Result<Self, Error> {
        let desc = dspfx_racks_desc { abi_version: DSPFX_ABI_VERSION, device, n_channels: channels, max_frames, tile_channels, slots };
        let mut h = ptr::null_mut();
        let rc = unsafe { dspfx_racks_create(&desc, &mut h) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_racks_create") });
        }
        Ok(ChannelRacks { h, channels, slots })
    }
    fn check(&self, rc: c_int, what: &str) -> Result<(), Error> {
        if rc == DSPFX_OK { Ok(()) } else { Err(Error { status: rc, message: reason(self.h, what) }) }
    }
    pub fn channels(&self) -> u32 { self.channels }
    pub fn slots(&self) -> u32 { self.slots }
    /// The device bytes of a bank's tables (a pure host function).
    pub fn plan(channels: u64, slots: u32) -> Result<u64, Error> {
        let mut bytes = 0u64;
        let rc = unsafe { dspfx_racks_plan(channels, slots, &mut bytes) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_racks_plan") });
        }
        Ok(bytes)
    }
    /// A DEVICE block of `n_frames` frames in the bank's layout through every channel's slots into the DEVICE block `out` (`out`
    /// may be `input`: in place).  Asynchronous on `stream`.
    pub unsafe fn run(&self, input: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> Result<(), Error> {
        let rc = dspfx_racks_run(self.h, input, out, n_frames, stream);
        self.check(rc, "dspfx_racks_run")
    }
    /// Gives slot `slot` of `count` channels from `first_channel` a node of `kind` (`DSPFX_GAIN`, `DSPFX_BIQUAD`, `DSPFX_LOW_PASS`,
    /// `DSPFX_HIGH_PASS`, `DSPFX_ENVELOPE`, `DSPFX_DISTORT`, `DSPFX_OVERDRIVE`, `DSPFX_CHEBYSHEV`): `sliders` in the order of the
    /// node's constructor, one value per channel each, `None` to keep or take the default; `modes` for Distort.  Any thread, never
    /// waits for the device.
    pub fn set(&self, slot: u32, kind: u32, sliders: &[Option<&[f32]>], modes: Option<&[u32]>, first_channel: u64, count: u64) -> Result<(), Error> {
        let bad = |message: &str| Err(Error { status: DSPFX_ERR_INVALID, message: message.into() });
        if sliders.len() > 6 {
            return bad("a rack node has at most six sliders");
        }
        let mut six: [*const f32; 6] = [ptr::null(); 6];
        for (t, v) in sliders.iter().enumerate() {
            if let Some(a) = v {
                if a.len() as u64 != count {
                    return bad("a slider slice is not `count` long");
                }
                six[t] = a.as_ptr();
            }
        }
        if modes.map_or(false, |m| m.len() as u64 != count) {
            return bad("the mode slice is not `count` long");
        }
        let rc = unsafe { dspfx_racks_set(self.h, slot, kind, six.as_ptr(), modes.map_or(ptr::null(), |m| m.as_ptr()), first_channel, count) };
        self.check(rc, "dspfx_racks_set")
    }
    /// Empties slot `slot` of `count` channels from `first_channel` and zeroes its state: that slot copies again.
    pub fn drop_nodes(&self, slot: u32, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_racks_drop(self.h, slot, first_channel, count) };
        self.check(rc, "dspfx_racks_drop")
    }
    /// The state of slot `slot` (`None`: of every slot) back to +0.0; the nodes and the sliders stay.
    pub fn reset(&self, slot: Option<u32>, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_racks_reset(self.h, slot.unwrap_or(DSPFX_RACKS_NONE), first_channel, count) };
        self.check(rc, "dspfx_racks_reset")
    }
    /// Per channel a bit per slot: slot t carries a node, as all stores made so far left it.
    pub fn present(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_racks_present(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_racks_present")?;
        Ok(m)
    }
    /// Per channel slot `slot`'s `dspfx_kind`, or `DSPFX_RACKS_NONE` when empty.
    pub fn kinds(&self, slot: u32) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_racks_kinds(self.h, slot, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_racks_kinds")?;
        Ok(m)
    }
    /// Per channel the mode of slot `slot`'s Distort node, `DSPFX_RACKS_NONE` otherwise.
    pub fn modes(&self, slot: u32) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_racks_modes(self.h, slot, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_racks_modes")?;
        Ok(m)
    }
    /// Per channel slot `slot`'s six raw sliders as they were given; 0 behind the kind's slider count and when empty.
    pub fn sliders(&self, slot: u32) -> Result<Vec<[f32; 6]>, Error> {
        let mut m = vec![[0f32; 6]; self.channels as usize];
        let rc = unsafe { dspfx_racks_sliders(self.h, slot, m.as_mut_ptr() as *mut f32, 0, m.len() as u64) };
        self.check(rc, "dspfx_racks_sliders")?;
        Ok(m)
    }
    /// The DEVICE pointer of slot `slot`'s state, four rows of `channels` floats: valid after a run, on its stream.
    pub fn state(&self, slot: u32) -> Result<*const f32, Error> {
        let mut p = ptr::null();
        let rc = unsafe { dspfx_racks_state(self.h, slot, &mut p) };
        self.check(rc, "dspfx_racks_state")?;
        Ok(p)
    }
}

impl Drop for ChannelRacks {
    fn drop(&mut self) {
        unsafe {
            dspfx_racks_destroy(self.h);
        }
    }
}
