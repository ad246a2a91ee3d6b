//! Raw bindings of `include/dspfx.h` (ABI version 1).  Kept in step with the header by
//! `tests/test_rust_shim_sync.py`; NOT compiled in the build container (no rustc there).
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

/// Opaque engine handle (`typedef struct dspfx_engine dspfx_engine`).
#[repr(C)]
pub struct dspfx_engine {
    _private: [u8; 0],
}

/// Opaque pitch detector bank handle (`typedef struct dspfx_pitch dspfx_pitch`).
#[repr(C)]
pub struct dspfx_pitch {
    _private: [u8; 0],
}

/// Opaque communicator handle (`typedef struct dspfx_comm dspfx_comm`).
#[repr(C)]
pub struct dspfx_comm {
    _private: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_engine_desc {
    pub abi_version: u32,
    pub device: i32,
    pub channels: u32,
    pub max_frames: u32,
    pub link_flags: u32,
    pub tile_channels: u32,
    pub channel_offset: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_node_desc {
    pub kind: i32,
    pub mode: i32,
    pub params: [f32; 8],
    pub delay_len: u32,
    pub n_taps: u32,
    pub taps: *const f64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_ctl {
    pub node: i32,
    pub param: i32,
    pub signal: *const f32,
}

/// One link of a graph given to `dspfx_graph_set` (include/dspfx.h).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_graph_link {
    pub src: i32,
    pub dst: i32,
    pub port: i32,
}

/// Where a slider / mode store took effect (`dspfx_param_log`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_param_event {
    pub seq: u64,
    pub frame: u64,
    pub node: i32,
    pub param: i32,
    pub value: f32,
    pub reserved: i32,
}

/// Device sample formats at the process boundary (`dspfx_process_pcm` / `dspfx_process_host_pcm`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_pcm_io {
    pub in_format: i32,
    pub in_channels: i32,
    pub out_format: i32,
    pub out_channels: i32,
}

/// Opaque output resampler bank handle (`typedef struct dspfx_resample dspfx_resample`).
#[repr(C)]
pub struct dspfx_resample {
    _private: [u8; 0],
}

/// The output resampler bank's descriptor (`dspfx_resample_create`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_resample_desc {
    pub abi_version: u32,
    pub device: i32,
    pub channels: u32,
    pub tile_channels: u32,
    pub block_frames: u32,
    pub slots: u32,
    pub target_hz: u32,
    pub out_format: i32,
    pub out_channels: i32,
}

/// Opaque Spectrogram bank handle (`typedef struct dspfx_spectrum dspfx_spectrum`).
#[repr(C)]
pub struct dspfx_spectrum {
    _private: [u8; 0],
}

/// The Spectrogram bank's descriptor (`dspfx_spectrum_create`); `window` / `gain` are host tables read at create, null = default.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_spectrum_desc {
    pub abi_version: u32,
    pub device: i32,
    pub channels: u32,
    pub tile_channels: u32,
    pub fft_size: u32,
    pub columns: u32,
    pub window: *const f32,
    pub gain: *const f32,
}

/// Opaque mix-matrix bank handle (`typedef struct dspfx_mixmatrix dspfx_mixmatrix`).
#[repr(C)]
pub struct dspfx_mixmatrix {
    _private: [u8; 0],
}

/// The mix-matrix bank's descriptor (`dspfx_mixmatrix_create`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_mixmatrix_desc {
    pub abi_version: u32,
    pub device: i32,
    pub n_channels: u32,
    pub max_frames: u32,
    pub tile_channels: u32,
    pub n_groups: u32,
    pub normalise: u32,
    pub group_start: *const u64,
}

/// Opaque channel-strip bank handle (`typedef struct dspfx_strips dspfx_strips`).
#[repr(C)]
pub struct dspfx_strips {
    _private: [u8; 0],
}

/// The channel-strip bank's descriptor (`dspfx_strips_create`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_strips_desc {
    pub abi_version: u32,
    pub device: i32,
    pub n_channels: u32,
    pub max_frames: u32,
    pub tile_channels: u32,
    pub bands: u32,
    pub link_flags: u32,
}

/// Opaque channel-delay bank handle (`typedef struct dspfx_delays dspfx_delays`).
#[repr(C)]
pub struct dspfx_delays {
    _private: [u8; 0],
}

/// The channel-delay bank's descriptor (`dspfx_delays_create`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_delays_desc {
    pub abi_version: u32,
    pub device: i32,
    pub n_channels: u32,
    pub max_frames: u32,
    pub tile_channels: u32,
    pub max_seconds: f32,
    pub page_round: u32,
    pub link_flags: u32,
}

/// Opaque talker bank handle (`typedef struct dspfx_talkers dspfx_talkers`).
#[repr(C)]
pub struct dspfx_talkers {
    _private: [u8; 0],
}

/// The talker bank's descriptor (`dspfx_talkers_create`); `group_start` is a host table of `n_groups + 1` entries read at create.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_talkers_desc {
    pub abi_version: u32,
    pub device: i32,
    pub n_channels: u32,
    pub max_frames: u32,
    pub tile_channels: u32,
    pub n_groups: u32,
    pub top: u32,
    pub group_start: *const u64,
}

/// Opaque channel-dynamics bank handle (`typedef struct dspfx_dynamics dspfx_dynamics`).
#[repr(C)]
pub struct dspfx_dynamics {
    _private: [u8; 0],
}

/// The channel-dynamics bank's descriptor (`dspfx_dynamics_create`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_dynamics_desc {
    pub abi_version: u32,
    pub device: i32,
    pub n_channels: u32,
    pub max_frames: u32,
    pub tile_channels: u32,
}

/// Opaque channel-shaper bank handle (`typedef struct dspfx_shapers dspfx_shapers`).
#[repr(C)]
pub struct dspfx_shapers {
    _private: [u8; 0],
}

/// The channel-shaper bank's descriptor (`dspfx_shapers_create`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_shapers_desc {
    pub abi_version: u32,
    pub device: i32,
    pub n_channels: u32,
    pub max_frames: u32,
    pub tile_channels: u32,
}

/// `dspfx_shapers_kinds`: the channel carries no node; `dspfx_shapers_modes`: it carries no Distort node.
pub const DSPFX_SHAPERS_NONE: u32 = 0xFFFF_FFFF;

/// Opaque channel-generator bank handle (`typedef struct dspfx_gens dspfx_gens`).
#[repr(C)]
pub struct dspfx_gens {
    _private: [u8; 0],
}

/// The channel-generator bank's descriptor (`dspfx_gens_create`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_gens_desc {
    pub abi_version: u32,
    pub device: i32,
    pub n_channels: u32,
    pub max_frames: u32,
    pub tile_channels: u32,
}

/// `dspfx_gens_modes`: the channel carries no node.
pub const DSPFX_GENS_NONE: u32 = 0xFFFF_FFFF;

/// Opaque channel-blend bank handle (`typedef struct dspfx_blends dspfx_blends`).
#[repr(C)]
pub struct dspfx_blends {
    _private: [u8; 0],
}

/// The channel-blend bank's descriptor (`dspfx_blends_create`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_blends_desc {
    pub abi_version: u32,
    pub device: i32,
    pub n_channels: u32,
    pub max_frames: u32,
    pub tile_channels: u32,
    pub n_buses: u32,
}

/// `dspfx_blends_assign`, `dspfx_blends_bus_of`: the channel reads no bus.
pub const DSPFX_BLENDS_NO_BUS: u32 = 0xFFFF_FFFF;
/// `dspfx_blends_kinds`: the channel carries no node.
pub const DSPFX_BLENDS_NONE: u32 = 0xFFFF_FFFF;

/// Opaque channel-filter bank handle (`typedef struct dspfx_filters dspfx_filters`).
#[repr(C)]
pub struct dspfx_filters {
    _private: [u8; 0],
}

/// The channel-filter bank's descriptor (`dspfx_filters_create`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_filters_desc {
    pub abi_version: u32,
    pub device: i32,
    pub n_channels: u32,
    pub max_frames: u32,
    pub tile_channels: u32,
    pub stages: u32,
}

/// `dspfx_filters_kinds`: the slot is empty; `dspfx_filters_reset`: every stage.
pub const DSPFX_FILTERS_NONE: u32 = 0xFFFF_FFFF;

/// Opaque channel-FIR bank handle (`typedef struct dspfx_firs dspfx_firs`).
#[repr(C)]
pub struct dspfx_firs {
    _private: [u8; 0],
}

/// The channel-FIR bank's descriptor (`dspfx_firs_create`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_firs_desc {
    pub abi_version: u32,
    pub device: i32,
    pub n_channels: u32,
    pub max_frames: u32,
    pub tile_channels: u32,
    pub max_taps: u32,
    pub general_only: u32,
}

/// The longest response a channel of a channel-FIR bank may carry.
pub const DSPFX_FIRS_MAX_TAPS: u32 = 1024;
/// `dspfx_firs_modes`: the channel carries no node; `dspfx_firs_set_taps`: keep the node's mode.
pub const DSPFX_FIRS_NONE: u32 = 0xFFFF_FFFF;

/// Opaque channel-canceller bank handle (`typedef struct dspfx_cancel dspfx_cancel`).
#[repr(C)]
pub struct dspfx_cancel {
    _private: [u8; 0],
}

/// The channel-canceller bank's descriptor (`dspfx_cancel_create`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_cancel_desc {
    pub abi_version: u32,
    pub device: i32,
    pub n_channels: u32,
    pub max_frames: u32,
    pub tile_channels: u32,
    pub max_taps: u32,
    pub max_delay: u32,
    pub general_only: u32,
}

/// The longest filter a channel of a channel-canceller bank may carry.
pub const DSPFX_CANCEL_MAX_TAPS: u32 = 1024;
/// The longest bulk delay, in frames, a channel of a channel-canceller bank may carry.
pub const DSPFX_CANCEL_MAX_DELAY: u32 = 65535;

/// Opaque channel-rack bank handle (`typedef struct dspfx_racks dspfx_racks`).
#[repr(C)]
pub struct dspfx_racks {
    _private: [u8; 0],
}

/// The channel-rack bank's descriptor (`dspfx_racks_create`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_racks_desc {
    pub abi_version: u32,
    pub device: i32,
    pub n_channels: u32,
    pub max_frames: u32,
    pub tile_channels: u32,
    pub slots: u32,
}

/// The slots one channel of a channel-rack bank owns at most.
pub const DSPFX_RACKS_MAX_SLOTS: u32 = 4;
/// `dspfx_racks_kinds`: the slot is empty; `dspfx_racks_modes`: it carries no Distort node; `dspfx_racks_reset`: every slot.
pub const DSPFX_RACKS_NONE: u32 = 0xFFFF_FFFF;

/// Opaque mix-group bank handle (`typedef struct dspfx_mixgroups dspfx_mixgroups`).
#[repr(C)]
pub struct dspfx_mixgroups {
    _private: [u8; 0],
}

/// The mix-group bank's descriptor (`dspfx_mixgroups_create`); `group_start` is a host table of `n_groups + 1` entries read at create.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_mixgroups_desc {
    pub abi_version: u32,
    pub device: i32,
    pub n_channels: u32,
    pub max_frames: u32,
    pub tile_channels: u32,
    pub n_groups: u32,
    pub normalise: u32,
    pub group_start: *const u64,
}

/// The Pitch Detector bank's descriptor (`dspfx_pitch_create`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_pitch_desc {
    pub abi_version: u32,
    pub device: i32,
    pub channels: u32,
    pub tile_channels: u32,
    pub power_thresh: f32,
    pub clarity_thresh: f32,
    pub pick_thresh: f32,
}

/// Opaque convolver bank handle (`typedef struct dspfx_convolve dspfx_convolve`).
#[repr(C)]
pub struct dspfx_convolve {
    _private: [u8; 0],
}

/// The convolver bank's descriptor (`dspfx_convolve_create`); `taps_reversed` is a host array of `n_taps` f64 read at create.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct dspfx_convolve_desc {
    pub abi_version: u32,
    pub device: i32,
    pub channels: u32,
    pub tile_channels: u32,
    pub n_taps: u32,
    pub max_taps: u32,
    pub mode: i32,
    pub taps_reversed: *const f64,
}

pub const DSPFX_ABI_VERSION: u32 = 2;
pub const DSPFX_BUF_SIZE: u32 = 128; // dsp-stuff/src/node.rs:257
pub const DSPFX_MAX_NODES: u32 = 32;
pub const DSPFX_COMM_ID_BYTES: usize = 128;

// dspfx_status
pub const DSPFX_OK: c_int = 0;
pub const DSPFX_ERR_INVALID: c_int = -1;
pub const DSPFX_ERR_NO_DEVICE: c_int = -2;
pub const DSPFX_ERR_HIP: c_int = -3;
pub const DSPFX_ERR_OOM: c_int = -4;
pub const DSPFX_ERR_UNSUPPORTED: c_int = -5;
pub const DSPFX_ERR_STATE: c_int = -6;

// dspfx_sample_format (devices.rs:305-350: cpal's SampleFormat, the four the engine converts)
pub const DSPFX_SAMPLE_F32: i32 = 0;
pub const DSPFX_SAMPLE_I16: i32 = 1;
pub const DSPFX_SAMPLE_U16: i32 = 2;
pub const DSPFX_SAMPLE_I32: i32 = 3;

// dspfx_pitch_param (nodes/pitch.rs:47-56 sliders)
pub const DSPFX_PITCH_POWER: i32 = 0;
pub const DSPFX_PITCH_CLARITY: i32 = 1;
pub const DSPFX_PITCH_PICK: i32 = 2;
pub const DSPFX_PITCH_WINDOW: u32 = 1024;
// the Spectrogram node's fft_size slider (spectrogram.rs:142); the bank takes the powers of two in it
pub const DSPFX_SPECTRUM_MIN_FFT: u32 = 128;
pub const DSPFX_SPECTRUM_MAX_FFT: u32 = 8192;
// the most device frames one dspfx_resample_pull makes, and the most frames a FIFO slot holds
pub const DSPFX_RESAMPLE_MAX_FRAMES: u32 = 4096;
// the longest response a convolver bank takes: 4096 partitions of 128 taps
pub const DSPFX_CONVOLVE_MAX_TAPS: u32 = 524288;
// the responses one convolver bank holds
pub const DSPFX_CONVOLVE_MAX_RESPONSES: u32 = 256;
/// the BiQuad bands one channel-strip bank holds per channel
pub const DSPFX_STRIPS_MAX_BANDS: u32 = 8;
pub const DSPFX_MIXMATRIX_MAX_ROOM: u32 = 1024;
pub const DSPFX_MIXMATRIX_MIX_MINUS: u32 = 0;
pub const DSPFX_MIXMATRIX_ZERO: u32 = 1;
pub const DSPFX_MIXMATRIX_DIRECT: u32 = 0;
pub const DSPFX_MIXMATRIX_STAGED: u32 = 1;
/// `DSPFX_MIXGROUPS_NO_ROOM`: the id of a channel that sits in no room.
pub const DSPFX_MIXGROUPS_NO_ROOM: u32 = 0xFFFF_FFFF;
/// `DSPFX_MIXMATRIX_NO_ROOM`: the same, for `dspfx_mixmatrix_assign`.
pub const DSPFX_MIXMATRIX_NO_ROOM: u32 = 0xFFFF_FFFF;
/// the most members a talker bank's room has, and the most talkers it names
pub const DSPFX_TALKERS_MAX_ROOM: u32 = 1024;
pub const DSPFX_TALKERS_MAX_TOP: u32 = 8;
/// a channel's pin (`dspfx_talkers_set_pin`): ranked; always passed and never ranked; never passed
pub const DSPFX_TALKERS_AUTO: u8 = 0;
pub const DSPFX_TALKERS_OPEN: u8 = 1;
pub const DSPFX_TALKERS_SHUT: u8 = 2;
/// `DSPFX_TALKERS_NO_ROOM`: the same, for `dspfx_talkers_assign` and `dspfx_talkers_select`.
pub const DSPFX_TALKERS_NO_ROOM: u32 = 0xFFFF_FFFF;

// link flags
pub const DSPFX_LINK_INTERNAL: u32 = 1;
pub const DSPFX_LINK_INPUT: u32 = 2;
pub const DSPFX_LINK_SIDE_RAW: u32 = 4;
pub const DSPFX_MAX_LINKS: u32 = 16;
pub const DSPFX_GRAPH_MAX_NODES: u32 = 16;
pub const DSPFX_GRAPH_INPUT: i32 = -1;
pub const DSPFX_GRAPH_ZERO: i32 = -2;
pub const DSPFX_GRAPH_INPUT2: i32 = -3;
pub const DSPFX_GRAPH_MAX_IO: u32 = 16;
/// Link source of input block k (`DSPFX_GRAPH_INPUT_N`).
pub const fn dspfx_graph_input_n(k: i32) -> i32 {
    if k == 0 { DSPFX_GRAPH_INPUT } else if k == 1 { DSPFX_GRAPH_INPUT2 } else { -(2 + k) }
}
pub const DSPFX_PORT_MAIN: i32 = 0;
pub const DSPFX_PORT_SIDE: i32 = 1;
pub const DSPFX_PORT_SLIDER: i32 = 2;
pub const DSPFX_PORT_RAW: i32 = 256;

// dspfx_kind
pub const DSPFX_GAIN: c_int = 0;
pub const DSPFX_BIQUAD: c_int = 1;
pub const DSPFX_LOW_PASS: c_int = 2;
pub const DSPFX_HIGH_PASS: c_int = 3;
pub const DSPFX_REVERB: c_int = 4;
pub const DSPFX_DISTORT: c_int = 5;
pub const DSPFX_OVERDRIVE: c_int = 6;
pub const DSPFX_CHEBYSHEV: c_int = 7;
pub const DSPFX_FIR: c_int = 8;
pub const DSPFX_ADD: c_int = 9;
pub const DSPFX_MIX: c_int = 10;
pub const DSPFX_SIGNAL_GEN: c_int = 11;
pub const DSPFX_ENVELOPE: c_int = 12;
pub const DSPFX_N_KINDS: c_int = 13;

// dspfx_distort_mode (nodes/distort.rs:18-28)
pub const DSPFX_DIST_HARD_CLIP: c_int = 0;
pub const DSPFX_DIST_SOFT_CLIP: c_int = 1;
pub const DSPFX_DIST_TANH: c_int = 2;
pub const DSPFX_DIST_RECIP_SOFT_CLIP: c_int = 3;
pub const DSPFX_DIST_FUZZ: c_int = 4;
pub const DSPFX_DIST_SIN: c_int = 5;
pub const DSPFX_DIST_ATAN: c_int = 6;
pub const DSPFX_DIST_SQUARE: c_int = 7;
pub const DSPFX_DIST_CHEBYSHEV4: c_int = 8;

// dspfx_signal_mode (nodes/signal_gen.rs:17-22)
pub const DSPFX_SIG_SINE: c_int = 0;
pub const DSPFX_SIG_TRIANGLE: c_int = 1;
pub const DSPFX_SIG_SQUARE: c_int = 2;
pub const DSPFX_SIG_CONSTANT: c_int = 3;

// dspfx_fir_mode (nodes/fir.rs)
pub const DSPFX_FIR_BALANCED: c_int = 0;
pub const DSPFX_FIR_AVERAGE: c_int = 1;
/// dspfx_fir_precision (dspfx.h): how a FIR node's steady-state sweep multiplies
pub const DSPFX_FIR_PRECISION_DEFAULT: c_int = 0;
pub const DSPFX_FIR_PRECISION_F32: c_int = 1;
pub const DSPFX_FIR_PRECISION_SPLIT: c_int = 2;
pub const DSPFX_FIR_PRECISION_HALF: c_int = 3;

#[link(name = "dspfx")]
extern "C" {
    pub fn dspfx_abi_version() -> u32;
    pub fn dspfx_strerror(status: c_int) -> *const c_char;
    pub fn dspfx_device_count() -> c_int;
    pub fn dspfx_node_defaults(kind: c_int, d: *mut dspfx_node_desc) -> c_int;
    pub fn dspfx_delay_len(seconds: f32, page_round: c_int) -> u32;
    pub fn dspfx_link_divisor(n_connected: u64) -> f32;

    pub fn dspfx_engine_create(desc: *const dspfx_engine_desc, out: *mut *mut dspfx_engine) -> c_int;
    pub fn dspfx_engine_destroy(e: *mut dspfx_engine);
    pub fn dspfx_last_error(e: *const dspfx_engine) -> *const c_char;

    pub fn dspfx_chain_set(e: *mut dspfx_engine, nodes: *const dspfx_node_desc, n_nodes: c_int) -> c_int;
    pub fn dspfx_chain_len(e: *const dspfx_engine) -> c_int;
    pub fn dspfx_kernels_ready(e: *mut dspfx_engine, wait_ms: c_int) -> c_int;
    pub fn dspfx_set_param(e: *mut dspfx_engine, node: c_int, param: c_int, value: f32) -> c_int;
    pub fn dspfx_set_param_seq(e: *mut dspfx_engine, node: c_int, param: c_int, value: f32, seq: *mut u64) -> c_int;
    pub fn dspfx_set_mode(e: *mut dspfx_engine, node: c_int, mode: c_int) -> c_int;
    pub fn dspfx_param_log(e: *mut dspfx_engine, dst: *mut dspfx_param_event, cap: c_int, after_seq: u64) -> c_int;
    pub fn dspfx_frames_submitted(e: *const dspfx_engine) -> u64;
    pub fn dspfx_set_delay_len(e: *mut dspfx_engine, node: c_int, delay_len: u32) -> c_int;
    pub fn dspfx_reserve_delay_len(e: *mut dspfx_engine, node: c_int, delay_len: u32) -> c_int;
    pub fn dspfx_ring_trim(e: *mut dspfx_engine) -> c_int;
    pub fn dspfx_set_taps(e: *mut dspfx_engine, node: c_int, taps_reversed: *const f64, n_taps: u32, mode: c_int) -> c_int;
    pub fn dspfx_set_fir_precision(e: *mut dspfx_engine, node: c_int, precision: c_int) -> c_int;
    pub fn dspfx_reset(e: *mut dspfx_engine) -> c_int;

    pub fn dspfx_tune_placement(e: *mut dspfx_engine, input: *const f32, side: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_process(e: *mut dspfx_engine, input: *const f32, side: *const f32, out: *mut f32, mix: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_process_bus(e: *mut dspfx_engine, input: *const f32, side: *const f32, out: *mut f32, mix: *mut f32, n_frames: u32, n_connected: u64, stream: *mut c_void) -> c_int;
    pub fn dspfx_process_ctl(e: *mut dspfx_engine, input: *const f32, side: *const f32, out: *mut f32, mix: *mut f32, n_frames: u32, ctl: *const dspfx_ctl, n_ctl: c_int, stream: *mut c_void) -> c_int;
    pub fn dspfx_host_alloc(bytes: usize, out: *mut *mut c_void) -> c_int;
    pub fn dspfx_host_free(p: *mut c_void) -> c_int;
    pub fn dspfx_process_host(e: *mut dspfx_engine, input: *const f32, side: *const f32, out: *mut f32, mix: *mut f32, n_frames: u32) -> c_int;
    pub fn dspfx_process_pcm(e: *mut dspfx_engine, io: *const dspfx_pcm_io, input: *const c_void, side: *const c_void, out: *mut c_void, mix: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_process_host_pcm(e: *mut dspfx_engine, io: *const dspfx_pcm_io, input: *const c_void, side: *const c_void, out: *mut c_void, mix: *mut f32, n_frames: u32) -> c_int;
    pub fn dspfx_process_partials(e: *mut dspfx_engine, input: *const f32, side: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_mix_collect(e: *mut dspfx_engine, mix: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_mix_finish(e: *mut dspfx_engine, mix: *mut f32, n_frames: u32, n_connected: u64, stream: *mut c_void) -> c_int;

    // the mix bus across GPUs: one RCCL all-reduce of n_frames floats per block (include/dspfx.h)
    pub fn dspfx_comm_unique_id(id_out: *mut c_void) -> c_int;
    pub fn dspfx_comm_create(device: c_int, n_ranks: c_int, rank: c_int, id: *const c_void, out: *mut *mut dspfx_comm) -> c_int;
    pub fn dspfx_comm_destroy(c: *mut dspfx_comm);
    pub fn dspfx_comm_size(c: *const dspfx_comm) -> c_int;
    pub fn dspfx_comm_rank(c: *const dspfx_comm) -> c_int;
    pub fn dspfx_comm_last_error(c: *const dspfx_comm) -> *const c_char;
    pub fn dspfx_comm_backend(c: *const dspfx_comm) -> *const c_char;
    pub fn dspfx_mix_allreduce(e: *mut dspfx_engine, c: *mut dspfx_comm, mix: *mut f32, n_frames: u32, n_connected: u64, stream: *mut c_void) -> c_int;

    pub fn dspfx_process_mixpipe(e: *mut dspfx_engine, input: *const f32, side: *const f32, out: *mut f32, mix: *mut f32, n_frames: u32, n_connected: u64, stream: *mut c_void) -> c_int;
    pub fn dspfx_mixpipe_flush(e: *mut dspfx_engine, mix_older: *mut f32, mix_newer: *mut f32, n_connected: u64, stream: *mut c_void) -> c_int;
    pub fn dspfx_process_io(e: *mut dspfx_engine, ins: *const *const f32, n_ins: c_int, outs: *const *mut f32, n_outs: c_int, mix: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_graph_set(e: *mut dspfx_engine, nodes: *const dspfx_node_desc, n_nodes: c_int, links: *const dspfx_graph_link, n_links: c_int) -> c_int;
    pub fn dspfx_graph_source(nodes: *const dspfx_node_desc, n_nodes: c_int, links: *const dspfx_graph_link, n_links: c_int, dst: *mut c_char, cap: usize) -> c_int;
    pub fn dspfx_link_average(e: *mut dspfx_engine, srcs: *const *const f32, n_srcs: c_int, dst: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;

    pub fn dspfx_state_size(e: *const dspfx_engine, node: c_int) -> i64;
    pub fn dspfx_state_export(e: *mut dspfx_engine, node: c_int, host_dst: *mut c_void, size: usize) -> c_int;
    pub fn dspfx_state_import(e: *mut dspfx_engine, node: c_int, host_src: *const c_void, size: usize) -> c_int;

    pub fn dspfx_fill_noise(e: *mut dspfx_engine, dst: *mut f32, n_frames: u32, n_abs0: u32, seed: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_sync(e: *mut dspfx_engine, stream: *mut c_void) -> c_int;
    pub fn dspfx_describe(e: *const dspfx_engine, dst: *mut c_char, cap: usize) -> c_int;
    pub fn dspfx_verify_fast_division(device: c_int, c: f32, mismatches: *mut u64) -> c_int;
    pub fn dspfx_verify_libm(device: c_int, func: c_int, mismatches: *mut u64, max_ulp: *mut u32) -> c_int;
    pub fn dspfx_profile_enable(e: *mut dspfx_engine, enable: c_int) -> c_int;
    pub fn dspfx_profile_read(e: *mut dspfx_engine, total_ms: *mut f64, launches: *mut u32, kernel_name: *mut c_char, cap: usize, reset: c_int) -> c_int;
    pub fn dspfx_algorithmic_bytes_per_sample(e: *const dspfx_engine, n_frames: u32) -> f64;

    pub fn dspfx_pitch_create(desc: *const dspfx_pitch_desc, out: *mut *mut dspfx_pitch) -> c_int;
    pub fn dspfx_pitch_destroy(p: *mut dspfx_pitch) -> c_int;
    pub fn dspfx_pitch_push(p: *mut dspfx_pitch, block: *const f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_pitch_slot(p: *mut dspfx_pitch) -> *mut f32;
    pub fn dspfx_pitch_set_param(p: *mut dspfx_pitch, which: c_int, value: f32) -> c_int;
    pub fn dspfx_pitch_read(p: *mut dspfx_pitch, freq: *mut f32, clarity: *mut f32, stream: *mut c_void) -> c_int;
    pub fn dspfx_pitch_reset(p: *mut dspfx_pitch) -> c_int;
    pub fn dspfx_pitch_windows(p: *const dspfx_pitch) -> i64;
    pub fn dspfx_resample_create(desc: *const dspfx_resample_desc, out: *mut *mut dspfx_resample) -> c_int;
    pub fn dspfx_resample_destroy(r: *mut dspfx_resample) -> c_int;
    pub fn dspfx_resample_push(r: *mut dspfx_resample, block: *const f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_resample_slot(r: *mut dspfx_resample) -> *mut f32;
    pub fn dspfx_resample_pull(r: *mut dspfx_resample, out: *mut c_void, n_out: u32, consumed: *mut u32, underrun: *mut i32, stream: *mut c_void) -> c_int;
    pub fn dspfx_resample_available(r: *mut dspfx_resample) -> i64;
    pub fn dspfx_resample_skip(r: *mut dspfx_resample, n_frames: u32) -> c_int;
    pub fn dspfx_resample_reset(r: *mut dspfx_resample) -> c_int;
    pub fn dspfx_resample_plan(target_hz: u32, value: *mut f64, idx: *mut u32, n_out: u32, advance: *mut u32, depth: *mut u32, coeff: *mut f64, input_len: *mut u32, pulled: *mut u32) -> c_int;
    pub fn dspfx_spectrum_create(desc: *const dspfx_spectrum_desc, out: *mut *mut dspfx_spectrum) -> c_int;
    pub fn dspfx_spectrum_destroy(p: *mut dspfx_spectrum) -> c_int;
    pub fn dspfx_spectrum_push(p: *mut dspfx_spectrum, block: *const f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_spectrum_slot(p: *mut dspfx_spectrum) -> *mut f32;
    pub fn dspfx_spectrum_column(p: *mut dspfx_spectrum, age: u32) -> *const f32;
    pub fn dspfx_spectrum_reset(p: *mut dspfx_spectrum) -> c_int;
    pub fn dspfx_spectrum_windows(p: *const dspfx_spectrum) -> i64;
    pub fn dspfx_spectrum_plan(fft_size: u32, window_out: *mut f32, bin_hz_out: *mut f32) -> c_int;
    pub fn dspfx_mixgroups_create(desc: *const dspfx_mixgroups_desc, out: *mut *mut dspfx_mixgroups) -> c_int;
    pub fn dspfx_mixgroups_destroy(m: *mut dspfx_mixgroups) -> c_int;
    pub fn dspfx_mixgroups_last_error(m: *const dspfx_mixgroups) -> *const c_char;
    pub fn dspfx_mixgroups_run(m: *mut dspfx_mixgroups, block: *const f32, n_frames: u32, buses: *mut f32, stream: *mut c_void) -> c_int;
    pub fn dspfx_mixgroups_returns(m: *mut dspfx_mixgroups, block: *const f32, n_frames: u32, buses: *mut f32, returns: *mut f32, stream: *mut c_void) -> c_int;
    pub fn dspfx_mixgroups_set_gains(m: *mut dspfx_mixgroups, host_values: *const f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_mixgroups_plan(group_start: *const u64, n_groups: u32, n_channels: u64, tile_channels: u32, depth_out: *mut u32) -> c_int;
    pub fn dspfx_mixgroups_assign(m: *mut dspfx_mixgroups, host_room_ids: *const u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_mixgroups_rooms(m: *mut dspfx_mixgroups, host_ids_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_mixgroups_room_plan(room_of: *const u32, n_channels: u64, n_groups: u32, tile_channels: u32, count_out: *mut u64, depth_out: *mut u32, pieces_out: *mut u64) -> c_int;
    pub fn dspfx_convolve_create(desc: *const dspfx_convolve_desc, out: *mut *mut dspfx_convolve) -> c_int;
    pub fn dspfx_convolve_destroy(p: *mut dspfx_convolve) -> c_int;
    pub fn dspfx_convolve_reset(p: *mut dspfx_convolve) -> c_int;
    pub fn dspfx_convolve_run(p: *mut dspfx_convolve, input: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_convolve_set_taps(p: *mut dspfx_convolve, taps_reversed: *const f64, n_taps: u32, mode: c_int) -> c_int;
    pub fn dspfx_convolve_plan(taps_reversed: *const f64, n_taps: u32, partitions: *mut u32, table_out: *mut f32) -> c_int;
    pub fn dspfx_convolve_response_add(p: *mut dspfx_convolve, taps_reversed: *const f64, n_taps: u32, mode: c_int, id_out: *mut u32) -> c_int;
    pub fn dspfx_convolve_response_set(p: *mut dspfx_convolve, id: u32, taps_reversed: *const f64, n_taps: u32, mode: c_int) -> c_int;
    pub fn dspfx_convolve_assign(p: *mut dspfx_convolve, host_ids: *const u16, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_convolve_response_count(p: *const dspfx_convolve) -> c_int;
    pub fn dspfx_strips_create(desc: *const dspfx_strips_desc, out: *mut *mut dspfx_strips) -> c_int;
    pub fn dspfx_strips_destroy(s: *mut dspfx_strips) -> c_int;
    pub fn dspfx_strips_last_error(s: *const dspfx_strips) -> *const c_char;
    pub fn dspfx_strips_run(s: *mut dspfx_strips, input: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_strips_set_gain(s: *mut dspfx_strips, host_levels: *const f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_strips_set_band(s: *mut dspfx_strips, band: u32, host_raw6: *const f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_strips_reset(s: *mut dspfx_strips) -> c_int;
    pub fn dspfx_strips_present(s: *mut dspfx_strips, host_masks_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_strips_coeffs(raw6: *const f32, out5: *mut f32) -> c_int;
    pub fn dspfx_delays_plan(channels: u64, max_seconds: f32, page_round: c_int, cap_out: *mut u32, bytes_out: *mut u64) -> c_int;
    pub fn dspfx_delays_create(desc: *const dspfx_delays_desc, out: *mut *mut dspfx_delays) -> c_int;
    pub fn dspfx_delays_destroy(d: *mut dspfx_delays) -> c_int;
    pub fn dspfx_delays_last_error(d: *const dspfx_delays) -> *const c_char;
    pub fn dspfx_delays_run(d: *mut dspfx_delays, input: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_delays_set_delay(d: *mut dspfx_delays, host_seconds: *const f32, host_decay: *const f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_delays_reset(d: *mut dspfx_delays) -> c_int;
    pub fn dspfx_delays_present(d: *mut dspfx_delays, host_present_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_delays_lengths(d: *mut dspfx_delays, host_lengths_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_envelope_gain(frames: f32) -> f32;
    pub fn dspfx_talkers_plan(channels: u64, n_groups: u32, bytes_out: *mut u64) -> c_int;
    pub fn dspfx_talkers_select(levels: *const f32, room_of: *const u32, n_channels: u64, n_groups: u32, top: *const u8, floor: f32, pins: *const u8, talkers_out: *mut i32, levels_out: *mut f32, target_out: *mut f32) -> c_int;
    pub fn dspfx_talkers_create(desc: *const dspfx_talkers_desc, out: *mut *mut dspfx_talkers) -> c_int;
    pub fn dspfx_talkers_destroy(t: *mut dspfx_talkers) -> c_int;
    pub fn dspfx_talkers_last_error(t: *const dspfx_talkers) -> *const c_char;
    pub fn dspfx_talkers_run(t: *mut dspfx_talkers, input: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_talkers_assign(t: *mut dspfx_talkers, host_room_ids: *const u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_talkers_set_detector(t: *mut dspfx_talkers, host_attack: *const f32, host_release: *const f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_talkers_set_pin(t: *mut dspfx_talkers, host_pins: *const u8, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_talkers_set_top(t: *mut dspfx_talkers, host_tops: *const u8, first_room: u64, count: u64) -> c_int;
    pub fn dspfx_talkers_set_floor(t: *mut dspfx_talkers, floor: f32) -> c_int;
    pub fn dspfx_talkers_reset(t: *mut dspfx_talkers, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_talkers_views(t: *mut dspfx_talkers, level_out: *mut *const f32, target_out: *mut *const f32, talkers_out: *mut *const i32, talker_levels_out: *mut *const f32) -> c_int;
    pub fn dspfx_talkers_room_of(t: *mut dspfx_talkers, host_ids_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_talkers_counts(t: *mut dspfx_talkers, host_counts_out: *mut u32) -> c_int;
    pub fn dspfx_talkers_audible(gate: *const f32, target: *const f32, room_of: *const u32, n_channels: u64, n_groups: u32, list_out: *mut i32, start_out: *mut u32, count_out: *mut u32) -> c_int;
    pub fn dspfx_talkers_audible_views(t: *mut dspfx_talkers, list_out: *mut *const i32, start_out: *mut *const u32, count_out: *mut *const u32) -> c_int;

    pub fn dspfx_dynamics_plan(channels: u64, bytes_out: *mut u64) -> c_int;
    pub fn dspfx_dynamics_gain(env: f32, threshold: f32, makeup: f32, q_out: *mut f32) -> f32;
    pub fn dspfx_dynamics_create(desc: *const dspfx_dynamics_desc, out: *mut *mut dspfx_dynamics) -> c_int;
    pub fn dspfx_dynamics_destroy(d: *mut dspfx_dynamics) -> c_int;
    pub fn dspfx_dynamics_last_error(d: *const dspfx_dynamics) -> *const c_char;
    pub fn dspfx_dynamics_run(d: *mut dspfx_dynamics, input: *const f32, key: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_dynamics_set(d: *mut dspfx_dynamics, host_threshold: *const f32, host_makeup: *const f32, host_attack: *const f32, host_release: *const f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_dynamics_drop(d: *mut dspfx_dynamics, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_dynamics_reset(d: *mut dspfx_dynamics, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_dynamics_present(d: *mut dspfx_dynamics, host_present_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_dynamics_views(d: *mut dspfx_dynamics, level_out: *mut *const f32, reduction_out: *mut *const f32) -> c_int;

    pub fn dspfx_shapers_plan(channels: u64, bytes_out: *mut u64) -> c_int;
    pub fn dspfx_shapers_create(desc: *const dspfx_shapers_desc, out: *mut *mut dspfx_shapers) -> c_int;
    pub fn dspfx_shapers_destroy(s: *mut dspfx_shapers) -> c_int;
    pub fn dspfx_shapers_last_error(s: *const dspfx_shapers) -> *const c_char;
    pub fn dspfx_shapers_run(s: *mut dspfx_shapers, input: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_shapers_set_distort(s: *mut dspfx_shapers, host_level: *const f32, host_mode: *const u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_shapers_set_overdrive(s: *mut dspfx_shapers, host_boost: *const f32, host_drive: *const f32, host_level: *const f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_shapers_set_chebyshev(s: *mut dspfx_shapers, host_level_pos: *const f32, host_level_neg: *const f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_shapers_drop(s: *mut dspfx_shapers, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_shapers_present(s: *mut dspfx_shapers, host_present_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_shapers_kinds(s: *mut dspfx_shapers, host_kinds_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_shapers_modes(s: *mut dspfx_shapers, host_modes_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_shapers_sliders(s: *mut dspfx_shapers, host_sliders_out: *mut f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_gens_plan(channels: u64, bytes_out: *mut u64) -> c_int;
    pub fn dspfx_gens_create(desc: *const dspfx_gens_desc, out: *mut *mut dspfx_gens) -> c_int;
    pub fn dspfx_gens_destroy(g: *mut dspfx_gens) -> c_int;
    pub fn dspfx_gens_last_error(g: *const dspfx_gens) -> *const c_char;
    pub fn dspfx_gens_run(g: *mut dspfx_gens, add_to: *const f32, amplitude: *const f32, frequency: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_gens_set(g: *mut dspfx_gens, host_amplitude: *const f32, host_frequency: *const f32, host_mode: *const u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_gens_drop(g: *mut dspfx_gens, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_gens_reset(g: *mut dspfx_gens, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_gens_present(g: *mut dspfx_gens, host_present_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_gens_modes(g: *mut dspfx_gens, host_modes_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_gens_sliders(g: *mut dspfx_gens, host_sliders_out: *mut f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_gens_clocks(g: *mut dspfx_gens, clock_out: *mut *const f32) -> c_int;
    pub fn dspfx_blends_plan(channels: u64, bytes_out: *mut u64) -> c_int;
    pub fn dspfx_blends_create(desc: *const dspfx_blends_desc, out: *mut *mut dspfx_blends) -> c_int;
    pub fn dspfx_blends_destroy(b: *mut dspfx_blends) -> c_int;
    pub fn dspfx_blends_last_error(b: *const dspfx_blends) -> *const c_char;
    pub fn dspfx_blends_run(b: *mut dspfx_blends, a: *const f32, side: *const f32, bus: *const f32, ratio: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_blends_set_mix(b: *mut dspfx_blends, host_ratio: *const f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_blends_set_add(b: *mut dspfx_blends, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_blends_set_send(b: *mut dspfx_blends, host_level: *const f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_blends_assign(b: *mut dspfx_blends, host_ids: *const u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_blends_drop(b: *mut dspfx_blends, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_blends_kinds(b: *mut dspfx_blends, host_kinds_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_blends_ratios(b: *mut dspfx_blends, host_ratios_out: *mut f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_blends_sends(b: *mut dspfx_blends, host_levels_out: *mut f32, host_present_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_blends_bus_of(b: *mut dspfx_blends, host_ids_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_filters_plan(channels: u64, stages: u32, bytes_out: *mut u64) -> c_int;
    pub fn dspfx_filters_create(desc: *const dspfx_filters_desc, out: *mut *mut dspfx_filters) -> c_int;
    pub fn dspfx_filters_destroy(f: *mut dspfx_filters) -> c_int;
    pub fn dspfx_filters_last_error(f: *const dspfx_filters) -> *const c_char;
    pub fn dspfx_filters_run(f: *mut dspfx_filters, input: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_filters_set_low_pass(f: *mut dspfx_filters, stage: u32, host_ratio: *const f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_filters_set_high_pass(f: *mut dspfx_filters, stage: u32, host_ratio: *const f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_filters_set_envelope(f: *mut dspfx_filters, stage: u32, host_attack: *const f32, host_release: *const f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_filters_drop(f: *mut dspfx_filters, stage: u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_filters_reset(f: *mut dspfx_filters, stage: u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_filters_present(f: *mut dspfx_filters, host_present_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_filters_kinds(f: *mut dspfx_filters, stage: u32, host_kinds_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_filters_sliders(f: *mut dspfx_filters, stage: u32, host_sliders_out: *mut f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_filters_state(f: *mut dspfx_filters, stage: u32, state_out: *mut *const f32) -> c_int;
    pub fn dspfx_racks_plan(channels: u64, slots: u32, bytes_out: *mut u64) -> c_int;
    pub fn dspfx_racks_create(desc: *const dspfx_racks_desc, out: *mut *mut dspfx_racks) -> c_int;
    pub fn dspfx_racks_destroy(r: *mut dspfx_racks) -> c_int;
    pub fn dspfx_racks_last_error(r: *const dspfx_racks) -> *const c_char;
    pub fn dspfx_racks_run(r: *mut dspfx_racks, input: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_racks_set(r: *mut dspfx_racks, slot: u32, kind: u32, host_sliders: *const *const f32, host_mode: *const u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_racks_drop(r: *mut dspfx_racks, slot: u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_racks_reset(r: *mut dspfx_racks, slot: u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_racks_present(r: *mut dspfx_racks, host_present_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_racks_kinds(r: *mut dspfx_racks, slot: u32, host_kinds_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_racks_modes(r: *mut dspfx_racks, slot: u32, host_modes_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_racks_sliders(r: *mut dspfx_racks, slot: u32, host_sliders_out: *mut f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_racks_state(r: *mut dspfx_racks, slot: u32, state_out: *mut *const f32) -> c_int;
    pub fn dspfx_firs_plan(channels: u64, max_taps: u32, bytes_out: *mut u64) -> c_int;
    pub fn dspfx_firs_create(desc: *const dspfx_firs_desc, out: *mut *mut dspfx_firs) -> c_int;
    pub fn dspfx_firs_destroy(f: *mut dspfx_firs) -> c_int;
    pub fn dspfx_firs_last_error(f: *const dspfx_firs) -> *const c_char;
    pub fn dspfx_firs_run(f: *mut dspfx_firs, input: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_firs_set_taps(f: *mut dspfx_firs, host_taps: *const f64, n_taps: u32, per_channel: u32, mode: u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_firs_set_mode(f: *mut dspfx_firs, mode: u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_firs_drop(f: *mut dspfx_firs, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_firs_reset(f: *mut dspfx_firs, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_firs_present(f: *mut dspfx_firs, host_present_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_firs_lengths(f: *mut dspfx_firs, host_lengths_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_firs_modes(f: *mut dspfx_firs, host_modes_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_firs_taps(f: *mut dspfx_firs, channel: u64, host_taps_out: *mut f64, n_taps_out: *mut u32) -> c_int;
    pub fn dspfx_firs_deque(f: *mut dspfx_firs, deque_out: *mut *const i32) -> c_int;
    pub fn dspfx_cancel_plan(channels: u64, max_taps: u32, max_delay: u32, bytes_out: *mut u64) -> c_int;
    pub fn dspfx_cancel_create(desc: *const dspfx_cancel_desc, out: *mut *mut dspfx_cancel) -> c_int;
    pub fn dspfx_cancel_destroy(a: *mut dspfx_cancel) -> c_int;
    pub fn dspfx_cancel_last_error(a: *const dspfx_cancel) -> *const c_char;
    pub fn dspfx_cancel_run(a: *mut dspfx_cancel, mic: *const f32, reference: *const f32, out: *mut f32, n_frames: u32, stream: *mut c_void) -> c_int;
    pub fn dspfx_cancel_set(a: *mut dspfx_cancel, host_taps: *const u32, host_mu: *const f32, host_eps: *const f32, host_delay: *const u32, host_adapt: *const u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_cancel_load(a: *mut dspfx_cancel, host_rows: *const f32, n_taps: u32, per_channel: u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_cancel_drop(a: *mut dspfx_cancel, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_cancel_reset(a: *mut dspfx_cancel, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_cancel_present(a: *mut dspfx_cancel, host_present_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_cancel_lengths(a: *mut dspfx_cancel, host_lengths_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_cancel_sliders(a: *mut dspfx_cancel, host_sliders_out: *mut f32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_cancel_delays(a: *mut dspfx_cancel, host_delays_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_cancel_adapting(a: *mut dspfx_cancel, host_adapting_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_cancel_weights_view(a: *mut dspfx_cancel, weights_out: *mut *const f32) -> c_int;
    pub fn dspfx_cancel_levels_view(a: *mut dspfx_cancel, levels_out: *mut *const f32) -> c_int;
    pub fn dspfx_mixmatrix_plan(group_start: *const u64, n_groups: u32, n_channels: u64, tile_channels: u32, count_out: *mut u32, edge_out: *mut u32, offset_out: *mut u64, total_bytes_out: *mut u64) -> c_int;
    pub fn dspfx_mixmatrix_create(desc: *const dspfx_mixmatrix_desc, out: *mut *mut dspfx_mixmatrix) -> c_int;
    pub fn dspfx_mixmatrix_destroy(m: *mut dspfx_mixmatrix) -> c_int;
    pub fn dspfx_mixmatrix_last_error(m: *const dspfx_mixmatrix) -> *const c_char;
    pub fn dspfx_mixmatrix_run(m: *mut dspfx_mixmatrix, block: *const f32, n_frames: u32, out: *mut f32, stream: *mut c_void) -> c_int;
    pub fn dspfx_mixmatrix_set_rows(m: *mut dspfx_mixmatrix, host_values: *const f32, row_len: u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_mixmatrix_set_cols(m: *mut dspfx_mixmatrix, host_values: *const f32, row_len: u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_mixmatrix_fill(m: *mut dspfx_mixmatrix, room: i64, preset: u32) -> c_int;
    pub fn dspfx_mixmatrix_reset(m: *mut dspfx_mixmatrix) -> c_int;
    pub fn dspfx_mixmatrix_set_pairs(m: *mut dspfx_mixmatrix, listeners: *const u32, sources: *const u32, gains: *const f32, count: u64) -> c_int;
    pub fn dspfx_mixmatrix_create_seats(desc: *const dspfx_mixmatrix_desc, seats: *const u32, out: *mut *mut dspfx_mixmatrix) -> c_int;
    pub fn dspfx_mixmatrix_plan_seats(group_start: *const u64, n_groups: u32, n_channels: u64, tile_channels: u32, seats: *const u32, count_out: *mut u32, edge_out: *mut u32, offset_out: *mut u64, total_bytes_out: *mut u64) -> c_int;
    pub fn dspfx_mixmatrix_assign(m: *mut dspfx_mixmatrix, host_room_ids: *const u32, first_channel: u64, count: u64, preset: u32) -> c_int;
    pub fn dspfx_mixmatrix_rooms(m: *mut dspfx_mixmatrix, host_ids_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_mixmatrix_seats(m: *mut dspfx_mixmatrix, host_seats_out: *mut u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_mixmatrix_occupancy(m: *mut dspfx_mixmatrix, host_counts_out: *mut u32) -> c_int;
    pub fn dspfx_mixmatrix_reseat(room_of_io: *mut u32, seat_of_io: *mut u32, seats: *const u32, n_groups: u32, n_channels: u64, room_ids: *const u32, first_channel: u64, count: u64) -> c_int;
    pub fn dspfx_mixmatrix_set_staging(m: *mut dspfx_mixmatrix, mode: u32) -> c_int;
    pub fn dspfx_mixmatrix_staging(m: *mut dspfx_mixmatrix, mode_out: *mut u32) -> c_int;
    pub fn dspfx_mixmatrix_staging_bytes(group_start: *const u64, n_groups: u32, n_channels: u64, tile_channels: u32, seats: *const u32, max_frames: u32, bytes_out: *mut u64) -> c_int;
    pub fn dspfx_mixmatrix_scatter(room_of: *const u32, seat_of: *const u32, seats: *const u32, n_groups: u32, n_channels: u64, chunks_out: *mut u64, lines_out: *mut u64) -> c_int;
    pub fn dspfx_mixmatrix_run_sparse(m: *mut dspfx_mixmatrix, block: *const f32, n_frames: u32, out: *mut f32, list: *const i32, list_len: u64, start: *const u32, count: *const u32, stream: *mut c_void) -> c_int;
}
