//! `mod gpu;` -- libdspfx binding for the dsp-stuff host (see host/rust/README.md).
pub mod engine;
pub mod ffi;
pub mod gpu_bank;
pub mod gpu_chain;
pub mod mix_groups;
pub mod convolver;
pub mod convolver_responses;
pub mod channel_strips;
pub mod channel_delays;
pub mod talkers;
pub mod channel_dynamics;
pub mod channel_shapers;
pub mod channel_generators;
pub mod channel_blends;
pub mod channel_filters;
pub mod channel_firs;
pub mod mix_matrix;
