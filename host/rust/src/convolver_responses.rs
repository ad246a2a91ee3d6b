//! Several responses on one `Convolver`, one per channel, switchable live (`dspfx_convolve_response_*`, `dspfx_convolve_assign`).
//!
//! A bank holds up to `DSPFX_CONVOLVE_MAX_RESPONSES` responses -- this room a booth, that one a church -- and a response id for
//! every channel.  Response 0 is the one given to `Convolver::new` (the one `set_taps` replaces) and every channel starts on it.
//! A channel carrying id r gets the bits a `Convolver` of response r alone would give it; `assign` keeps the channel's history,
//! so a room moves from one hall to another without a click.
//! NOT compiled in the build container (no rustc).
use super::convolver::Convolver;
use super::engine::Error;
use super::ffi::*;
use std::ffi::CStr;
use std::os::raw::c_int;

fn error(rc: c_int, what: &str) -> Error {
    let msg = unsafe { CStr::from_ptr(dspfx_strerror(rc)) }.to_string_lossy().into_owned();
    Error { status: rc, message: format!("{}: {}", what, msg) }
}

impl Convolver {
    /// One more response (time-reversed taps, at most the bank's `max_taps`) and its mode; returns its id: 1, 2, ...
    /// No channel carries it until `assign` says so.  A file load: it allocates and waits for the runs already submitted.
    pub fn add_response(&mut self, taps_reversed: &[f64], mode: i32) -> Result<u32, Error> {
        let mut id = 0u32;
        let rc = unsafe { dspfx_convolve_response_add(self.handle(), taps_reversed.as_ptr(), taps_reversed.len() as u32, mode, &mut id) };
        if rc == DSPFX_OK { Ok(id) } else { Err(error(rc, "dspfx_convolve_response_add")) }
    }
    /// Replaces response `id` and leaves the others, the ids and the history alone; `id` 0 is `set_taps`.
    pub fn set_response(&mut self, id: u32, taps_reversed: &[f64], mode: i32) -> Result<(), Error> {
        let partitions = Self::plan(taps_reversed)?;
        let rc = unsafe { dspfx_convolve_response_set(self.handle(), id, taps_reversed.as_ptr(), taps_reversed.len() as u32, mode) };
        if rc != DSPFX_OK {
            return Err(error(rc, "dspfx_convolve_response_set"));
        }
        if id == 0 {
            self.set_partitions(partitions);
        }
        Ok(())
    }
    /// Channels `first_channel ..` carry the responses `ids` from the next run on; their history stays.  An id the bank does
    /// not hold, or a range past the channels, is refused and stores nothing.
    pub fn assign(&self, ids: &[u16], first_channel: u64) -> Result<(), Error> {
        let rc = unsafe { dspfx_convolve_assign(self.handle(), ids.as_ptr(), first_channel, ids.len() as u64) };
        if rc == DSPFX_OK { Ok(()) } else { Err(error(rc, "dspfx_convolve_assign")) }
    }
    /// How many responses the bank holds.
    pub fn responses(&self) -> u32 {
        let n = unsafe { dspfx_convolve_response_count(self.handle()) };
        if n < 0 { 0 } else { n as u32 }
    }
}
