//! `Convolver`: one long impulse response over the channels of a bank by partitioned FFT (`dspfx_convolve_*`).
//!
//! The FIR node takes any WAV file as its response (nodes/fir.rs:86-173); past a few thousand taps the direct form is the wrong
//! algorithm.  A host with G room buses (`MixGroups`) binds one `Convolver` of G channels over the DEVICE bus block:
//! `y[n] = (sum over j of h[j] * x[n - j]) * divisor` per 128-frame block, divisor 1 (Balanced) or 1 / T (Average), by a 256-point
//! FFT per block and one read of the channel's spectral history.  Taps are passed time-reversed, exactly as `set_taps` takes them.
//! The history starts as silence; `set_taps` keeps it (the reference's reload), `reset` returns to silence.
//! NOT compiled in the build container (no rustc).
use super::engine::Error;
use super::ffi::*;
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::ptr;

pub struct Convolver {
    h: *mut dspfx_convolve,
    channels: u32,
    partitions: u32,
}
unsafe impl Send for Convolver {}
// every call is serialised by the bank's own lock
unsafe impl Sync for Convolver {}

fn error(rc: c_int, what: &str) -> Error {
    let msg = unsafe { CStr::from_ptr(dspfx_strerror(rc)) }.to_string_lossy().into_owned();
    Error { status: rc, message: format!("{}: {}", what, msg) }
}

impl Convolver {
    /// `taps_reversed`: the response, time-reversed; `mode`: `DSPFX_FIR_BALANCED` or `DSPFX_FIR_AVERAGE`; `max_taps`: history is
    /// reserved for reloads of up to this many taps (0 = this response's length); `tile_channels`: 0 or the engine's W.
    pub fn new(device: i32, channels: u32, tile_channels: u32, taps_reversed: &[f64], mode: i32, max_taps: u32) -> Result<Self, Error> {
        let partitions = Self::plan(taps_reversed)?;
        let desc = dspfx_convolve_desc {
            abi_version: DSPFX_ABI_VERSION,
            device,
            channels,
            tile_channels,
            n_taps: taps_reversed.len() as u32,
            max_taps,
            mode,
            taps_reversed: taps_reversed.as_ptr(),
        };
        let mut h = ptr::null_mut();
        let rc = unsafe { dspfx_convolve_create(&desc, &mut h) };
        if rc != DSPFX_OK {
            return Err(error(rc, "dspfx_convolve_create"));
        }
        Ok(Convolver { h, channels, partitions })
    }
    pub fn channels(&self) -> u32 { self.channels }
    /// The bank's handle, for the calls kept in `convolver_responses.rs`.
    pub(super) fn handle(&self) -> *mut dspfx_convolve { self.h }
    pub(super) fn set_partitions(&mut self, partitions: u32) { self.partitions = partitions; }
    /// P = ceil(T / 128): the spectra of history one block reads per channel.
    pub fn partitions(&self) -> u32 { self.partitions }
    /// A DEVICE block of `n_frames` frames (a multiple of 128) in the bank's layout into the DEVICE block `out` (which may be
    /// `input` itself).  Asynchronous on `stream`.
    pub unsafe fn run(&self, input: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> Result<(), Error> {
        let rc = dspfx_convolve_run(self.h, input, out, n_frames, stream);
        if rc == DSPFX_OK { Ok(()) } else { Err(error(rc, "dspfx_convolve_run")) }
    }
    /// Replaces the response and keeps the history; more than `max_taps` is refused and changes nothing.
    pub fn set_taps(&mut self, taps_reversed: &[f64], mode: i32) -> Result<(), Error> {
        let partitions = Self::plan(taps_reversed)?;
        let rc = unsafe { dspfx_convolve_set_taps(self.h, taps_reversed.as_ptr(), taps_reversed.len() as u32, mode) };
        if rc != DSPFX_OK {
            return Err(error(rc, "dspfx_convolve_set_taps"));
        }
        self.partitions = partitions;
        Ok(())
    }
    /// Back to silence, ahead of the next run.
    pub fn reset(&self) -> Result<(), Error> {
        let rc = unsafe { dspfx_convolve_reset(self.h) };
        if rc == DSPFX_OK { Ok(()) } else { Err(error(rc, "dspfx_convolve_reset")) }
    }
    /// The partitions of a response (a pure host function; it also checks the taps as `new` does).
    pub fn plan(taps_reversed: &[f64]) -> Result<u32, Error> {
        let mut partitions = 0u32;
        let rc = unsafe { dspfx_convolve_plan(taps_reversed.as_ptr(), taps_reversed.len() as u32, &mut partitions, ptr::null_mut()) };
        if rc == DSPFX_OK { Ok(partitions) } else { Err(error(rc, "dspfx_convolve_plan")) }
    }
}

impl Drop for Convolver {
    fn drop(&mut self) {
        unsafe {
            dspfx_convolve_destroy(self.h);
        }
    }
}
