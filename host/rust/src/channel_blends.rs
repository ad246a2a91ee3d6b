//! `ChannelBlends`: per-channel Add and Mix nodes over the channels of a bank (`dspfx_blends_*`).
//!
//! In the reference every graph owns its own Add (nodes/add.rs) and Mix (nodes/mix.rs) nodes, a Mix with its own ratio slider, and
//! wires whatever it likes into the node's `b` port, through a Gain node where it wants a send level; an engine runs one ratio and
//! one side block for all its channels.  Channel c of this bank carries ONE such node (none, Add, or Mix with its ratio), an
//! optional send (the Gain node on `b`) and a bus id, and its sample is bit for bit what an engine whose chain is that node writes
//! for the channel from the same inputs.  The second input of a run is an N-channel device block, or a `[n_frames][buses]`
//! frame-major bus block -- what `MixGroups::run`, `Convolver::run` and a frame-major engine write -- that channel c reads at its
//! bus id (+0.0 on `DSPFX_BLENDS_NO_BUS`), or nothing (+0.0, an unconnected port).  The control block is the Mix node's `as_input`
//! ratio port; unlike the reference, it is connected per call and its first value is NOT latched into the slider.  A fresh bank
//! copies `a`.  The GUI thread stores through the `set_*` calls, `assign` and `drop_nodes`, which never wait for the device: the
//! next `run` applies the stores in order.
//! NOT compiled in the build container (no rustc).
use super::engine::Error;
use super::ffi::*;
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::ptr;

pub struct ChannelBlends {
    h: *mut dspfx_blends,
    channels: u32,
    buses: u32,
}
unsafe impl Send for ChannelBlends {}
// runs are serialised by the bank's own lock; stores take the store lock and the store queue's
unsafe impl Sync for ChannelBlends {}

fn reason(h: *const dspfx_blends, what: &str) -> String {
    let msg = unsafe { CStr::from_ptr(dspfx_blends_last_error(h)) }.to_string_lossy().into_owned();
    if msg.is_empty() { what.into() } else { msg }
}

fn same_len(count: u64, v: Option<&[f32]>) -> Result<*const f32, Error> {
    match v {
        Some(a) if a.len() as u64 != count => Err(Error { status: DSPFX_ERR_INVALID, message: "a value slice is not `count` long".into() }),
        Some(a) => Ok(a.as_ptr()),
        None => Ok(ptr::null()),
    }
}

impl ChannelBlends {
    /// `tile_channels`: 0 (frame-major) or the engine's W.  `buses`: the channels of a run's bus block, 0 for a bank that takes none.
    pub fn new(device: i32, channels: u32, buses: u32, tile_channels: u32, max_frames: u32) -> Result<Self, Error> {
        let desc = dspfx_blends_desc { abi_version: DSPFX_ABI_VERSION, device, n_channels: channels, max_frames, tile_channels, n_buses: buses };
        let mut h = ptr::null_mut();
        let rc = unsafe { dspfx_blends_create(&desc, &mut h) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_blends_create") });
        }
        Ok(ChannelBlends { h, channels, buses })
    }
    fn check(&self, rc: c_int, what: &str) -> Result<(), Error> {
        if rc == DSPFX_OK { Ok(()) } else { Err(Error { status: rc, message: reason(self.h, what) }) }
    }
    pub fn channels(&self) -> u32 { self.channels }
    pub fn buses(&self) -> u32 { self.buses }
    /// The device bytes of a bank's tables (a pure host function).
    pub fn plan(channels: u64) -> Result<u64, Error> {
        let mut bytes = 0u64;
        let rc = unsafe { dspfx_blends_plan(channels, &mut bytes) };
        if rc != DSPFX_OK {
            return Err(Error { status: rc, message: reason(ptr::null(), "dspfx_blends_plan") });
        }
        Ok(bytes)
    }
    /// One DEVICE block `a` of `n_frames` frames in the bank's layout into `out` (which may be `a` or `side`).  `side`: a DEVICE
    /// block of the same shape, or `bus`: a DEVICE block `[n_frames][buses]`, or both null (the second input is +0.0); giving both
    /// is refused.  `ratio`: the control block of the Mix nodes' ratio, or null.  Asynchronous on `stream`.
    pub unsafe fn run(&self, a: *const f32, side: *const f32, bus: *const f32, ratio: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> Result<(), Error> {
        let rc = dspfx_blends_run(self.h, a, side, bus, ratio, out, n_frames, stream);
        self.check(rc, "dspfx_blends_run")
    }
    /// Gives `count` channels from `first_channel` a Mix node (any thread, never waits for the device): one ratio per channel;
    /// `None` keeps a Mix node's ratio and is 0.5 where the channel carries none or an Add node.
    pub fn set_mix(&self, ratio: Option<&[f32]>, first_channel: u64, count: u64) -> Result<(), Error> {
        let r = same_len(count, ratio)?;
        let rc = unsafe { dspfx_blends_set_mix(self.h, r, first_channel, count) };
        self.check(rc, "dspfx_blends_set_mix")
    }
    /// Gives `count` channels from `first_channel` an Add node.
    pub fn set_add(&self, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_blends_set_add(self.h, first_channel, count) };
        self.check(rc, "dspfx_blends_set_add")
    }
    /// Gives the channels a send, a Gain node on the second input: one level per channel; `None` removes it.
    pub fn set_send(&self, level: Option<&[f32]>, first_channel: u64, count: u64) -> Result<(), Error> {
        let l = same_len(count, level)?;
        let rc = unsafe { dspfx_blends_set_send(self.h, l, first_channel, count) };
        self.check(rc, "dspfx_blends_set_send")
    }
    /// Channels from `first_channel` read the buses `ids`, each below `buses` or `DSPFX_BLENDS_NO_BUS`; a bad id stores nothing.
    pub fn assign(&self, ids: &[u32], first_channel: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_blends_assign(self.h, ids.as_ptr(), first_channel, ids.len() as u64) };
        self.check(rc, "dspfx_blends_assign")
    }
    /// Removes the node and the send of `count` channels from `first_channel`: a copy of `a` again; the bus id stays.
    pub fn drop_nodes(&self, first_channel: u64, count: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_blends_drop(self.h, first_channel, count) };
        self.check(rc, "dspfx_blends_drop")
    }
    /// Per channel `DSPFX_ADD`, `DSPFX_MIX` or `DSPFX_BLENDS_NONE`, as all stores made so far left it.
    pub fn kinds(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_blends_kinds(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_blends_kinds")?;
        Ok(m)
    }
    /// The Mix node's ratio per channel, 0 for every other channel.
    pub fn ratios(&self) -> Result<Vec<f32>, Error> {
        let mut m = vec![0f32; self.channels as usize];
        let rc = unsafe { dspfx_blends_ratios(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_blends_ratios")?;
        Ok(m)
    }
    /// The send per channel: `Some(level)`, or `None` where the channel has none.
    pub fn sends(&self) -> Result<Vec<Option<f32>>, Error> {
        let mut level = vec![0f32; self.channels as usize];
        let mut present = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_blends_sends(self.h, level.as_mut_ptr(), present.as_mut_ptr(), 0, level.len() as u64) };
        self.check(rc, "dspfx_blends_sends")?;
        Ok(level.iter().zip(&present).map(|(l, p)| if *p != 0 { Some(*l) } else { None }).collect())
    }
    /// The bus id per channel, `DSPFX_BLENDS_NO_BUS` for none.
    pub fn bus_of(&self) -> Result<Vec<u32>, Error> {
        let mut m = vec![0u32; self.channels as usize];
        let rc = unsafe { dspfx_blends_bus_of(self.h, m.as_mut_ptr(), 0, m.len() as u64) };
        self.check(rc, "dspfx_blends_bus_of")?;
        Ok(m)
    }
}

impl Drop for ChannelBlends {
    fn drop(&mut self) {
        unsafe {
            dspfx_blends_destroy(self.h);
        }
    }
}
