"""dsp-stuff_amd -- Python binding of the MI355X-native effect-chain engine.

A thin ctypes layer over the C ABI in include/dspfx.h (csrc/libdspfx.so, hand-written
HIP for gfx950).  Node constructors carry the reference's names, slider fields,
ranges and defaults (dsp-stuff/src/nodes/*.rs) so tests read like the reference's
node definitions.  There is no CPU fallback: importing works anywhere (so the
symbol table can be checked), but creating an Engine without a HIP device raises.

The directory name has a hyphen (it is the repo's package directory, not an
importable identifier): load it with `__graft_entry__.load_package()`.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from dataclasses import dataclass, field
from typing import Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# DSPFX_LIB lets tools/ab.py load an experiment build of the same library side by side
LIB_PATH = os.environ.get("DSPFX_LIB") or os.path.join(_HERE, "csrc", "libdspfx.so")

BUF_SIZE = 128  # dsp-stuff/src/node.rs:257
ABI_VERSION = 2

# dspfx_kind
GAIN, BIQUAD, LOW_PASS, HIGH_PASS, REVERB, DISTORT, OVERDRIVE, CHEBYSHEV, FIR, ADD, MIX, SIGNAL_GEN, ENVELOPE = range(13)
SIG_SINE, SIG_TRIANGLE, SIG_SQUARE, SIG_CONSTANT = range(4)
# dspfx_distort_mode (nodes/distort.rs:18-28)
HARD_CLIP, SOFT_CLIP, TANH, RECIP_SOFT_CLIP, FUZZ, SIN, ATAN, SQUARE, CHEBYSHEV4 = range(9)
DISTORT_MODES = ["HardClip", "SoftClip", "Tanh", "RecipSoftClip", "Fuzz", "Sin", "Atan", "Square", "Chebyshev4"]
FIR_BALANCED, FIR_AVERAGE = 0, 1
FIR_PRECISION_DEFAULT, FIR_PRECISION_F32, FIR_PRECISION_SPLIT, FIR_PRECISION_HALF = 0, 1, 2, 3
LINK_INTERNAL, LINK_INPUT, LINK_SIDE_RAW = 1, 2, 4
MAX_LINKS = 16
GRAPH_MAX_NODES = 16
ERR_UNSUPPORTED = -5
GRAPH_INPUT, GRAPH_ZERO, GRAPH_INPUT2 = -1, -2, -3
GRAPH_MAX_IO = 16
GRAPH_INPUTS = (GRAPH_INPUT, GRAPH_INPUT2) + tuple(-(2 + k) for k in range(2, GRAPH_MAX_IO))     # link source of input block k
PORT_MAIN, PORT_SIDE, PORT_SLIDER = 0, 1, 2
PORT_RAW = 256
# dspfx_sample_format: device sample formats at the boundary (devices.rs:305-350)
SAMPLE_F32, SAMPLE_I16, SAMPLE_U16, SAMPLE_I32 = range(4)
# dspfx_pitch_param: the Pitch Detector's sliders (nodes/pitch.rs:47-56), 0.5 each by default
PITCH_POWER, PITCH_CLARITY, PITCH_PICK = range(3)
PITCH_WINDOW = 1024
SPECTRUM_MIN_FFT, SPECTRUM_MAX_FFT = 128, 8192      # DSPFX_SPECTRUM_*: the Spectrogram node's fft_size slider (spectrogram.rs:142)
SPECTRUM_RATE = 48000.0         # spectrogram.rs:238 sampling_rate: bin k of an n-point window is k * 48000 / n Hz
CONVOLVE_MAX_TAPS = 524288      # DSPFX_CONVOLVE_MAX_TAPS: the longest response a Convolver takes (4096 partitions of 128)
NO_ROOM = 0xFFFFFFFF            # DSPFX_MIXGROUPS_NO_ROOM: MixGroups.assign, the channel sits in no room
CONVOLVE_MAX_RESPONSES = 256    # DSPFX_CONVOLVE_MAX_RESPONSES: the responses one Convolver holds
STRIPS_MAX_BANDS = 8            # DSPFX_STRIPS_MAX_BANDS: the BiQuad bands one ChannelStrips bank holds per channel
MIXMATRIX_MAX_ROOM = 1024       # DSPFX_MIXMATRIX_MAX_ROOM: the most members a MixMatrix room has
MIXMATRIX_MIX_MINUS, MIXMATRIX_ZERO = 0, 1      # DSPFX_MIXMATRIX_*: MixMatrix.fill presets
MIXMATRIX_DIRECT, MIXMATRIX_STAGED = 0, 1       # DSPFX_MIXMATRIX_*: MixMatrix.set_staging modes
TALKERS_MAX_ROOM, TALKERS_MAX_TOP = 1024, 8     # DSPFX_TALKERS_*: the most members a Talkers room has, the most talkers it names
TALKERS_AUTO, TALKERS_OPEN, TALKERS_SHUT = 0, 1, 2      # DSPFX_TALKERS_*: Talkers.set_pin
SHAPERS_NONE = 0xFFFFFFFF       # DSPFX_SHAPERS_NONE: ChannelShapers.kinds() without a node, .modes() without a Distort node
GENS_NONE = 0xFFFFFFFF          # DSPFX_GENS_NONE: ChannelGenerators.modes() without a node
BLENDS_NONE = 0xFFFFFFFF        # DSPFX_BLENDS_NONE: ChannelBlends.kinds() without a node
FILTERS_NONE = 0xFFFFFFFF       # DSPFX_FILTERS_NONE: ChannelFilters.kinds() of an empty slot; reset(stage=None), every stage
RACKS_NONE = 0xFFFFFFFF         # DSPFX_RACKS_NONE: ChannelRacks.kinds() of an empty slot, .modes() without a Distort node
RACKS_MAX_SLOTS = 4             # DSPFX_RACKS_MAX_SLOTS: the slots one ChannelRacks channel owns at most
FIRS_NONE = 0xFFFFFFFF          # DSPFX_FIRS_NONE: ChannelFirs.modes() without a node; set_taps(mode=None), keep the node's mode
FIRS_MAX_TAPS = 1024            # DSPFX_FIRS_MAX_TAPS: the longest response a ChannelFirs channel may carry
CANCEL_MAX_TAPS = 1024          # DSPFX_CANCEL_MAX_TAPS: the longest filter a ChannelCancellers channel may carry
CANCEL_MAX_DELAY = 65535        # DSPFX_CANCEL_MAX_DELAY: the longest bulk delay, in frames
BLENDS_NO_BUS = 0xFFFFFFFF      # DSPFX_BLENDS_NO_BUS: ChannelBlends.assign, the channel reads no bus (the same value as NO_ROOM)
RESAMPLE_MAX_FRAMES = 4096      # DSPFX_RESAMPLE_MAX_FRAMES: the most device frames one pull makes, the most frames a FIFO slot holds

# every symbol include/dspfx.h declares
EXPORTS = [
    "dspfx_abi_version", "dspfx_strerror", "dspfx_device_count", "dspfx_node_defaults", "dspfx_delay_len",
    "dspfx_link_divisor", "dspfx_engine_create", "dspfx_engine_destroy", "dspfx_last_error", "dspfx_chain_set",
    "dspfx_chain_len", "dspfx_set_param", "dspfx_set_mode", "dspfx_set_delay_len", "dspfx_set_taps", "dspfx_set_fir_precision",
    "dspfx_reset", "dspfx_tune_placement", "dspfx_process", "dspfx_process_host", "dspfx_host_alloc", "dspfx_host_free", "dspfx_mix_finish", "dspfx_process_mixpipe", "dspfx_mixpipe_flush", "dspfx_link_average", "dspfx_graph_set", "dspfx_graph_source", "dspfx_state_size",
    "dspfx_state_export", "dspfx_state_import", "dspfx_fill_noise", "dspfx_sync", "dspfx_describe",
    "dspfx_algorithmic_bytes_per_sample", "dspfx_profile_enable", "dspfx_profile_read", "dspfx_verify_fast_division", "dspfx_verify_libm",
    "dspfx_process_partials", "dspfx_mix_collect", "dspfx_process_ctl",
    "dspfx_process_io", "dspfx_comm_unique_id", "dspfx_comm_create", "dspfx_comm_destroy", "dspfx_comm_size", "dspfx_comm_rank",
    "dspfx_comm_last_error", "dspfx_mix_allreduce",
    "dspfx_set_param_seq", "dspfx_param_log", "dspfx_frames_submitted", "dspfx_process_bus", "dspfx_kernels_ready", "dspfx_comm_backend",
    "dspfx_reserve_delay_len", "dspfx_ring_trim", "dspfx_process_pcm", "dspfx_process_host_pcm",
    "dspfx_pitch_create", "dspfx_pitch_destroy", "dspfx_pitch_push", "dspfx_pitch_slot", "dspfx_pitch_set_param", "dspfx_pitch_read",
    "dspfx_pitch_reset", "dspfx_pitch_windows",
    "dspfx_resample_create", "dspfx_resample_destroy", "dspfx_resample_push", "dspfx_resample_slot", "dspfx_resample_pull",
    "dspfx_resample_available", "dspfx_resample_skip", "dspfx_resample_reset", "dspfx_resample_plan",
    "dspfx_spectrum_create", "dspfx_spectrum_destroy", "dspfx_spectrum_push", "dspfx_spectrum_slot", "dspfx_spectrum_column",
    "dspfx_spectrum_reset", "dspfx_spectrum_windows", "dspfx_spectrum_plan",
    "dspfx_mixgroups_create", "dspfx_mixgroups_destroy", "dspfx_mixgroups_last_error", "dspfx_mixgroups_run",
    "dspfx_mixgroups_set_gains", "dspfx_mixgroups_plan", "dspfx_mixgroups_returns",
    "dspfx_mixgroups_assign", "dspfx_mixgroups_rooms", "dspfx_mixgroups_room_plan",
    "dspfx_convolve_create", "dspfx_convolve_destroy", "dspfx_convolve_reset", "dspfx_convolve_run", "dspfx_convolve_set_taps",
    "dspfx_convolve_plan", "dspfx_convolve_response_add", "dspfx_convolve_response_set", "dspfx_convolve_assign",
    "dspfx_convolve_response_count",
    "dspfx_strips_create", "dspfx_strips_destroy", "dspfx_strips_last_error", "dspfx_strips_run", "dspfx_strips_set_gain",
    "dspfx_strips_set_band", "dspfx_strips_reset", "dspfx_strips_present", "dspfx_strips_coeffs",
    "dspfx_delays_plan", "dspfx_delays_create", "dspfx_delays_destroy", "dspfx_delays_last_error", "dspfx_delays_run",
    "dspfx_delays_set_delay", "dspfx_delays_reset", "dspfx_delays_present", "dspfx_delays_lengths",
    "dspfx_mixmatrix_plan", "dspfx_mixmatrix_create", "dspfx_mixmatrix_destroy", "dspfx_mixmatrix_last_error", "dspfx_mixmatrix_run",
    "dspfx_mixmatrix_set_rows", "dspfx_mixmatrix_set_cols", "dspfx_mixmatrix_fill", "dspfx_mixmatrix_reset",
    "dspfx_mixmatrix_set_pairs", "dspfx_mixmatrix_create_seats", "dspfx_mixmatrix_plan_seats", "dspfx_mixmatrix_assign",
    "dspfx_mixmatrix_rooms", "dspfx_mixmatrix_seats", "dspfx_mixmatrix_occupancy", "dspfx_mixmatrix_reseat",
    "dspfx_mixmatrix_set_staging", "dspfx_mixmatrix_staging", "dspfx_mixmatrix_staging_bytes", "dspfx_mixmatrix_scatter",
    "dspfx_envelope_gain", "dspfx_talkers_plan", "dspfx_talkers_select", "dspfx_talkers_create", "dspfx_talkers_destroy",
    "dspfx_talkers_last_error", "dspfx_talkers_run", "dspfx_talkers_assign", "dspfx_talkers_set_detector", "dspfx_talkers_set_pin",
    "dspfx_talkers_set_top", "dspfx_talkers_set_floor", "dspfx_talkers_reset", "dspfx_talkers_views", "dspfx_talkers_room_of",
    "dspfx_talkers_counts", "dspfx_talkers_audible", "dspfx_talkers_audible_views", "dspfx_mixmatrix_run_sparse",
    "dspfx_dynamics_plan", "dspfx_dynamics_gain", "dspfx_dynamics_create", "dspfx_dynamics_destroy", "dspfx_dynamics_last_error",
    "dspfx_dynamics_run", "dspfx_dynamics_set", "dspfx_dynamics_drop", "dspfx_dynamics_reset", "dspfx_dynamics_present",
    "dspfx_dynamics_views",
    "dspfx_shapers_plan", "dspfx_shapers_create", "dspfx_shapers_destroy", "dspfx_shapers_last_error", "dspfx_shapers_run",
    "dspfx_shapers_set_distort", "dspfx_shapers_set_overdrive", "dspfx_shapers_set_chebyshev", "dspfx_shapers_drop",
    "dspfx_shapers_present", "dspfx_shapers_kinds", "dspfx_shapers_modes", "dspfx_shapers_sliders",
    "dspfx_gens_plan", "dspfx_gens_create", "dspfx_gens_destroy", "dspfx_gens_last_error", "dspfx_gens_run", "dspfx_gens_set",
    "dspfx_gens_drop", "dspfx_gens_reset", "dspfx_gens_present", "dspfx_gens_modes", "dspfx_gens_sliders", "dspfx_gens_clocks",
    "dspfx_blends_plan", "dspfx_blends_create", "dspfx_blends_destroy", "dspfx_blends_last_error", "dspfx_blends_run",
    "dspfx_blends_set_mix", "dspfx_blends_set_add", "dspfx_blends_set_send", "dspfx_blends_assign", "dspfx_blends_drop",
    "dspfx_blends_kinds", "dspfx_blends_ratios", "dspfx_blends_sends", "dspfx_blends_bus_of",
    "dspfx_filters_plan", "dspfx_filters_create", "dspfx_filters_destroy", "dspfx_filters_last_error", "dspfx_filters_run",
    "dspfx_filters_set_low_pass", "dspfx_filters_set_high_pass", "dspfx_filters_set_envelope", "dspfx_filters_drop",
    "dspfx_filters_reset", "dspfx_filters_present", "dspfx_filters_kinds", "dspfx_filters_sliders", "dspfx_filters_state",
    "dspfx_firs_plan", "dspfx_firs_create", "dspfx_firs_destroy", "dspfx_firs_last_error", "dspfx_firs_run", "dspfx_firs_set_taps",
    "dspfx_firs_set_mode", "dspfx_firs_drop", "dspfx_firs_reset", "dspfx_firs_present", "dspfx_firs_lengths", "dspfx_firs_modes",
    "dspfx_firs_taps", "dspfx_firs_deque",
    "dspfx_racks_plan", "dspfx_racks_create", "dspfx_racks_destroy", "dspfx_racks_last_error", "dspfx_racks_run", "dspfx_racks_set",
    "dspfx_racks_drop", "dspfx_racks_reset", "dspfx_racks_present", "dspfx_racks_kinds", "dspfx_racks_modes", "dspfx_racks_sliders",
    "dspfx_racks_state",
    "dspfx_cancel_plan", "dspfx_cancel_create", "dspfx_cancel_destroy", "dspfx_cancel_last_error", "dspfx_cancel_run", "dspfx_cancel_set",
    "dspfx_cancel_load", "dspfx_cancel_drop", "dspfx_cancel_reset", "dspfx_cancel_present", "dspfx_cancel_lengths", "dspfx_cancel_sliders",
    "dspfx_cancel_delays", "dspfx_cancel_adapting", "dspfx_cancel_weights_view", "dspfx_cancel_levels_view",
]
COMM_ID_BYTES = 128


class DspfxError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"dspfx error {status}: {msg}")
        self.status = status


class _EngineDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("channels", C.c_uint32),
                ("max_frames", C.c_uint32), ("link_flags", C.c_uint32), ("tile_channels", C.c_uint32),
                ("channel_offset", C.c_uint64)]


class _NodeDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("mode", C.c_int32), ("params", C.c_float * 8),
                ("delay_len", C.c_uint32), ("n_taps", C.c_uint32), ("taps", C.POINTER(C.c_double))]


class _GraphLink(C.Structure):
    _fields_ = [("src", C.c_int32), ("dst", C.c_int32), ("port", C.c_int32)]


class _ParamEvent(C.Structure):
    _fields_ = [("seq", C.c_uint64), ("frame", C.c_uint64), ("node", C.c_int32), ("param", C.c_int32),
                ("value", C.c_float), ("reserved", C.c_int32)]


class _PcmIo(C.Structure):
    _fields_ = [("in_format", C.c_int32), ("in_channels", C.c_int32), ("out_format", C.c_int32), ("out_channels", C.c_int32)]


class _PitchDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("channels", C.c_uint32), ("tile_channels", C.c_uint32),
                ("power_thresh", C.c_float), ("clarity_thresh", C.c_float), ("pick_thresh", C.c_float)]


class _ResampleDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("channels", C.c_uint32), ("tile_channels", C.c_uint32),
                ("block_frames", C.c_uint32), ("slots", C.c_uint32), ("target_hz", C.c_uint32), ("out_format", C.c_int32),
                ("out_channels", C.c_int32)]


class _SpectrumDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("channels", C.c_uint32), ("tile_channels", C.c_uint32),
                ("fft_size", C.c_uint32), ("columns", C.c_uint32), ("window", C.POINTER(C.c_float)), ("gain", C.POINTER(C.c_float))]


class _MixGroupsDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("n_channels", C.c_uint32), ("max_frames", C.c_uint32),
                ("tile_channels", C.c_uint32), ("n_groups", C.c_uint32), ("normalise", C.c_uint32),
                ("group_start", C.POINTER(C.c_uint64))]


class _ConvolveDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("channels", C.c_uint32), ("tile_channels", C.c_uint32),
                ("n_taps", C.c_uint32), ("max_taps", C.c_uint32), ("mode", C.c_int32), ("taps_reversed", C.POINTER(C.c_double))]


class _StripsDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("n_channels", C.c_uint32), ("max_frames", C.c_uint32),
                ("tile_channels", C.c_uint32), ("bands", C.c_uint32), ("link_flags", C.c_uint32)]


class _DelaysDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("n_channels", C.c_uint32), ("max_frames", C.c_uint32),
                ("tile_channels", C.c_uint32), ("max_seconds", C.c_float), ("page_round", C.c_uint32), ("link_flags", C.c_uint32)]


class _MixMatrixDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("n_channels", C.c_uint32), ("max_frames", C.c_uint32),
                ("tile_channels", C.c_uint32), ("n_groups", C.c_uint32), ("normalise", C.c_uint32),
                ("group_start", C.POINTER(C.c_uint64))]


class _TalkersDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("n_channels", C.c_uint32), ("max_frames", C.c_uint32),
                ("tile_channels", C.c_uint32), ("n_groups", C.c_uint32), ("top", C.c_uint32),
                ("group_start", C.POINTER(C.c_uint64))]


class _DynamicsDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("n_channels", C.c_uint32), ("max_frames", C.c_uint32),
                ("tile_channels", C.c_uint32)]


class _ShapersDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("n_channels", C.c_uint32), ("max_frames", C.c_uint32),
                ("tile_channels", C.c_uint32)]


class _GensDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("n_channels", C.c_uint32), ("max_frames", C.c_uint32),
                ("tile_channels", C.c_uint32)]


class _BlendsDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("n_channels", C.c_uint32), ("max_frames", C.c_uint32),
                ("tile_channels", C.c_uint32), ("n_buses", C.c_uint32)]


class _FiltersDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("n_channels", C.c_uint32), ("max_frames", C.c_uint32),
                ("tile_channels", C.c_uint32), ("stages", C.c_uint32)]


class _FirsDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("n_channels", C.c_uint32), ("max_frames", C.c_uint32),
                ("tile_channels", C.c_uint32), ("max_taps", C.c_uint32), ("general_only", C.c_uint32)]


class _CancelDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("n_channels", C.c_uint32), ("max_frames", C.c_uint32),
                ("tile_channels", C.c_uint32), ("max_taps", C.c_uint32), ("max_delay", C.c_uint32), ("general_only", C.c_uint32)]


class _RacksDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("n_channels", C.c_uint32), ("max_frames", C.c_uint32),
                ("tile_channels", C.c_uint32), ("slots", C.c_uint32)]


class _Ctl(C.Structure):
    _fields_ = [("node", C.c_int32), ("param", C.c_int32), ("signal", C.c_void_p)]


_lib = None


def lib():
    """Load csrc/libdspfx.so; fails loudly when the HIP library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C {os.path.dirname(LIB_PATH)}` "
                          "(or __graft_entry__.build()); there is no fallback implementation")
    # One HIP runtime per process: PyTorch ships its own copy of the ROCm libraries, and a process that maps the system's
    # libamdhip64 (through libdspfx.so) BEFORE importing torch ends up with two runtimes, of which only the first to
    # initialise sees the GPU (measured: tools/probe_import_order.py -- either torch or this library reports no device).
    # Importing torch first makes libdspfx.so bind to the copy torch loaded.  Hosts without torch just use the system's.
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(LIB_PATH)
    vp, f32p = C.c_void_p, C.c_void_p
    L.dspfx_abi_version.restype = C.c_uint32
    L.dspfx_strerror.restype = C.c_char_p
    L.dspfx_strerror.argtypes = [C.c_int]
    L.dspfx_device_count.restype = C.c_int
    L.dspfx_node_defaults.argtypes = [C.c_int, C.POINTER(_NodeDesc)]
    L.dspfx_delay_len.restype = C.c_uint32
    L.dspfx_delay_len.argtypes = [C.c_float, C.c_int]
    L.dspfx_link_divisor.restype = C.c_float
    L.dspfx_link_divisor.argtypes = [C.c_uint64]
    L.dspfx_engine_create.argtypes = [C.POINTER(_EngineDesc), C.POINTER(vp)]
    L.dspfx_engine_destroy.argtypes = [vp]
    L.dspfx_engine_destroy.restype = None
    L.dspfx_last_error.restype = C.c_char_p
    L.dspfx_last_error.argtypes = [vp]
    L.dspfx_chain_set.argtypes = [vp, C.POINTER(_NodeDesc), C.c_int]
    L.dspfx_chain_len.argtypes = [vp]
    L.dspfx_kernels_ready.argtypes = [vp, C.c_int]
    L.dspfx_graph_set.argtypes = [vp, C.POINTER(_NodeDesc), C.c_int, C.POINTER(_GraphLink), C.c_int]
    L.dspfx_graph_source.argtypes = [C.POINTER(_NodeDesc), C.c_int, C.POINTER(_GraphLink), C.c_int, C.c_char_p, C.c_size_t]
    L.dspfx_set_param.argtypes = [vp, C.c_int, C.c_int, C.c_float]
    L.dspfx_set_mode.argtypes = [vp, C.c_int, C.c_int]
    L.dspfx_set_param_seq.argtypes = [vp, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_uint64)]
    L.dspfx_param_log.argtypes = [vp, C.POINTER(_ParamEvent), C.c_int, C.c_uint64]
    L.dspfx_frames_submitted.restype = C.c_uint64
    L.dspfx_frames_submitted.argtypes = [vp]
    L.dspfx_set_delay_len.argtypes = [vp, C.c_int, C.c_uint32]
    L.dspfx_reserve_delay_len.argtypes = [vp, C.c_int, C.c_uint32]
    L.dspfx_ring_trim.argtypes = [vp]
    L.dspfx_set_taps.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.c_uint32, C.c_int]
    L.dspfx_set_fir_precision.argtypes = [vp, C.c_int, C.c_int]
    L.dspfx_reset.argtypes = [vp]
    L.dspfx_process.argtypes = [vp, f32p, f32p, f32p, f32p, C.c_uint32, vp]
    L.dspfx_process_host.argtypes = [vp, f32p, f32p, f32p, f32p, C.c_uint32]
    L.dspfx_process_pcm.argtypes = [vp, C.POINTER(_PcmIo), vp, vp, vp, f32p, C.c_uint32, vp]
    L.dspfx_process_host_pcm.argtypes = [vp, C.POINTER(_PcmIo), vp, vp, vp, f32p, C.c_uint32]
    L.dspfx_process_bus.argtypes = [vp, f32p, f32p, f32p, f32p, C.c_uint32, C.c_uint64, vp]
    L.dspfx_mix_finish.argtypes = [vp, f32p, C.c_uint32, C.c_uint64, vp]
    L.dspfx_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    L.dspfx_host_free.argtypes = [C.c_void_p]
    L.dspfx_tune_placement.argtypes = [vp, f32p, f32p, f32p, C.c_uint32, vp]
    L.dspfx_process_mixpipe.argtypes = [vp, f32p, f32p, f32p, f32p, C.c_uint32, C.c_uint64, vp]
    L.dspfx_mixpipe_flush.argtypes = [vp, f32p, f32p, C.c_uint64, vp]
    L.dspfx_link_average.argtypes = [vp, C.POINTER(C.c_void_p), C.c_int, f32p, C.c_uint32, vp]
    L.dspfx_process_ctl.argtypes = [vp, f32p, f32p, f32p, f32p, C.c_uint32, C.POINTER(_Ctl), C.c_int, vp]
    L.dspfx_process_partials.argtypes = [vp, f32p, f32p, f32p, C.c_uint32, vp]
    L.dspfx_mix_collect.argtypes = [vp, f32p, C.c_uint32, vp]
    L.dspfx_state_size.restype = C.c_int64
    L.dspfx_state_size.argtypes = [vp, C.c_int]
    L.dspfx_state_export.argtypes = [vp, C.c_int, vp, C.c_size_t]
    L.dspfx_state_import.argtypes = [vp, C.c_int, vp, C.c_size_t]
    L.dspfx_fill_noise.argtypes = [vp, f32p, C.c_uint32, C.c_uint32, C.c_uint32, vp]
    L.dspfx_sync.argtypes = [vp, vp]
    L.dspfx_describe.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.dspfx_verify_fast_division.argtypes = [C.c_int, C.c_float, C.POINTER(C.c_uint64)]
    L.dspfx_verify_libm.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.dspfx_profile_enable.argtypes = [vp, C.c_int]
    L.dspfx_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t, C.c_int]
    L.dspfx_process_io.argtypes = [vp, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_int, f32p, C.c_uint32, vp]
    L.dspfx_comm_unique_id.argtypes = [vp]
    L.dspfx_comm_create.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.dspfx_comm_destroy.argtypes = [vp]
    L.dspfx_comm_destroy.restype = None
    L.dspfx_comm_size.argtypes = [vp]
    L.dspfx_comm_rank.argtypes = [vp]
    L.dspfx_comm_last_error.argtypes = [vp]
    L.dspfx_comm_last_error.restype = C.c_char_p
    L.dspfx_comm_backend.argtypes = [vp]
    L.dspfx_comm_backend.restype = C.c_char_p
    L.dspfx_mix_allreduce.argtypes = [vp, vp, f32p, C.c_uint32, C.c_uint64, vp]
    L.dspfx_algorithmic_bytes_per_sample.restype = C.c_double
    L.dspfx_algorithmic_bytes_per_sample.argtypes = [vp, C.c_uint32]
    L.dspfx_pitch_create.argtypes = [C.POINTER(_PitchDesc), C.POINTER(C.c_void_p)]
    L.dspfx_pitch_destroy.argtypes = [vp]
    L.dspfx_pitch_push.argtypes = [vp, vp, C.c_uint32, vp]
    L.dspfx_pitch_slot.restype = C.c_void_p
    L.dspfx_pitch_slot.argtypes = [vp]
    L.dspfx_pitch_set_param.argtypes = [vp, C.c_int, C.c_float]
    L.dspfx_pitch_read.argtypes = [vp, vp, vp, vp]
    L.dspfx_pitch_reset.argtypes = [vp]
    L.dspfx_pitch_windows.restype = C.c_int64
    L.dspfx_pitch_windows.argtypes = [vp]
    L.dspfx_resample_create.argtypes = [C.POINTER(_ResampleDesc), C.POINTER(C.c_void_p)]
    L.dspfx_resample_destroy.argtypes = [vp]
    L.dspfx_resample_push.argtypes = [vp, vp, C.c_uint32, vp]
    L.dspfx_resample_slot.restype = C.c_void_p
    L.dspfx_resample_slot.argtypes = [vp]
    L.dspfx_resample_pull.argtypes = [vp, vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), vp]
    L.dspfx_resample_available.restype = C.c_int64
    L.dspfx_resample_available.argtypes = [vp]
    L.dspfx_resample_skip.argtypes = [vp, C.c_uint32]
    L.dspfx_resample_reset.argtypes = [vp]
    L.dspfx_resample_plan.argtypes = [C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.dspfx_spectrum_create.argtypes = [C.POINTER(_SpectrumDesc), C.POINTER(C.c_void_p)]
    L.dspfx_spectrum_destroy.argtypes = [vp]
    L.dspfx_spectrum_push.argtypes = [vp, vp, C.c_uint32, vp]
    L.dspfx_spectrum_slot.restype = C.c_void_p
    L.dspfx_spectrum_slot.argtypes = [vp]
    L.dspfx_spectrum_column.restype = C.c_void_p
    L.dspfx_spectrum_column.argtypes = [vp, C.c_uint32]
    L.dspfx_spectrum_reset.argtypes = [vp]
    L.dspfx_spectrum_windows.restype = C.c_int64
    L.dspfx_spectrum_windows.argtypes = [vp]
    L.dspfx_spectrum_plan.argtypes = [C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.dspfx_mixgroups_create.argtypes = [C.POINTER(_MixGroupsDesc), C.POINTER(C.c_void_p)]
    L.dspfx_mixgroups_destroy.argtypes = [vp]
    L.dspfx_mixgroups_last_error.restype = C.c_char_p
    L.dspfx_mixgroups_last_error.argtypes = [vp]
    L.dspfx_mixgroups_run.argtypes = [vp, f32p, C.c_uint32, f32p, vp]
    L.dspfx_mixgroups_returns.argtypes = [vp, f32p, C.c_uint32, f32p, f32p, vp]
    L.dspfx_mixgroups_set_gains.argtypes = [vp, C.POINTER(C.c_float), C.c_uint64, C.c_uint64]
    L.dspfx_mixgroups_plan.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32)]
    L.dspfx_mixgroups_assign.argtypes = [vp, C.POINTER(C.c_uint32), C.c_uint64, C.c_uint64]
    L.dspfx_mixgroups_rooms.argtypes = [vp, C.POINTER(C.c_uint32), C.c_uint64, C.c_uint64]
    L.dspfx_mixgroups_room_plan.argtypes = [C.POINTER(C.c_uint32), C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.dspfx_convolve_create.argtypes = [C.POINTER(_ConvolveDesc), C.POINTER(C.c_void_p)]
    L.dspfx_convolve_destroy.argtypes = [vp]
    L.dspfx_convolve_reset.argtypes = [vp]
    L.dspfx_convolve_run.argtypes = [vp, f32p, f32p, C.c_uint32, vp]
    L.dspfx_convolve_set_taps.argtypes = [vp, C.POINTER(C.c_double), C.c_uint32, C.c_int]
    L.dspfx_convolve_plan.argtypes = [C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    L.dspfx_convolve_response_add.argtypes = [vp, C.POINTER(C.c_double), C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]
    L.dspfx_convolve_response_set.argtypes = [vp, C.c_uint32, C.POINTER(C.c_double), C.c_uint32, C.c_int]
    L.dspfx_convolve_assign.argtypes = [vp, C.POINTER(C.c_uint16), C.c_uint64, C.c_uint64]
    L.dspfx_convolve_response_count.argtypes = [vp]
    L.dspfx_strips_create.argtypes = [C.POINTER(_StripsDesc), C.POINTER(C.c_void_p)]
    L.dspfx_strips_destroy.argtypes = [vp]
    L.dspfx_strips_last_error.restype = C.c_char_p
    L.dspfx_strips_last_error.argtypes = [vp]
    L.dspfx_strips_run.argtypes = [vp, f32p, f32p, C.c_uint32, vp]
    L.dspfx_strips_set_gain.argtypes = [vp, C.POINTER(C.c_float), C.c_uint64, C.c_uint64]
    L.dspfx_strips_set_band.argtypes = [vp, C.c_uint32, C.POINTER(C.c_float), C.c_uint64, C.c_uint64]
    L.dspfx_strips_reset.argtypes = [vp]
    L.dspfx_strips_present.argtypes = [vp, C.POINTER(C.c_uint32), C.c_uint64, C.c_uint64]
    L.dspfx_strips_coeffs.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.dspfx_delays_plan.argtypes = [C.c_uint64, C.c_float, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.dspfx_delays_create.argtypes = [C.POINTER(_DelaysDesc), C.POINTER(C.c_void_p)]
    L.dspfx_delays_destroy.argtypes = [vp]
    L.dspfx_delays_last_error.restype = C.c_char_p
    L.dspfx_delays_last_error.argtypes = [vp]
    L.dspfx_delays_run.argtypes = [vp, f32p, f32p, C.c_uint32, vp]
    L.dspfx_delays_set_delay.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint64, C.c_uint64]
    L.dspfx_delays_reset.argtypes = [vp]
    L.dspfx_delays_present.argtypes = [vp, C.POINTER(C.c_uint32), C.c_uint64, C.c_uint64]
    L.dspfx_delays_lengths.argtypes = [vp, C.POINTER(C.c_uint32), C.c_uint64, C.c_uint64]
    L.dspfx_mixmatrix_plan.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32),
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.dspfx_mixmatrix_create.argtypes = [C.POINTER(_MixMatrixDesc), C.POINTER(vp)]
    L.dspfx_mixmatrix_destroy.argtypes = [vp]
    L.dspfx_mixmatrix_last_error.restype = C.c_char_p
    L.dspfx_mixmatrix_last_error.argtypes = [vp]
    L.dspfx_mixmatrix_run.argtypes = [vp, f32p, C.c_uint32, f32p, vp]
    L.dspfx_mixmatrix_set_rows.argtypes = [vp, C.POINTER(C.c_float), C.c_uint32, C.c_uint64, C.c_uint64]
    L.dspfx_mixmatrix_set_cols.argtypes = [vp, C.POINTER(C.c_float), C.c_uint32, C.c_uint64, C.c_uint64]
    L.dspfx_mixmatrix_fill.argtypes = [vp, C.c_int64, C.c_uint32]
    L.dspfx_mixmatrix_reset.argtypes = [vp]
    u32p = C.POINTER(C.c_uint32)
    L.dspfx_mixmatrix_set_pairs.argtypes = [vp, u32p, u32p, C.POINTER(C.c_float), C.c_uint64]
    L.dspfx_mixmatrix_create_seats.argtypes = [C.POINTER(_MixMatrixDesc), u32p, C.POINTER(vp)]
    L.dspfx_mixmatrix_plan_seats.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.c_uint64, C.c_uint32, u32p, u32p, u32p,
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.dspfx_mixmatrix_assign.argtypes = [vp, u32p, C.c_uint64, C.c_uint64, C.c_uint32]
    L.dspfx_mixmatrix_rooms.argtypes = [vp, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_mixmatrix_seats.argtypes = [vp, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_mixmatrix_occupancy.argtypes = [vp, u32p]
    L.dspfx_mixmatrix_reseat.argtypes = [u32p, u32p, u32p, C.c_uint32, C.c_uint64, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_mixmatrix_set_staging.argtypes = [vp, C.c_uint32]
    L.dspfx_mixmatrix_staging.argtypes = [vp, u32p]
    L.dspfx_mixmatrix_staging_bytes.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.c_uint64, C.c_uint32, u32p, C.c_uint32, C.POINTER(C.c_uint64)]
    L.dspfx_mixmatrix_scatter.argtypes = [u32p, u32p, u32p, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    u8p, fp = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    L.dspfx_envelope_gain.restype = C.c_float
    L.dspfx_envelope_gain.argtypes = [C.c_float]
    L.dspfx_talkers_plan.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    L.dspfx_talkers_select.argtypes = [fp, u32p, C.c_uint64, C.c_uint32, u8p, C.c_float, u8p, C.POINTER(C.c_int32), fp, fp]
    L.dspfx_talkers_create.argtypes = [C.POINTER(_TalkersDesc), C.POINTER(vp)]
    L.dspfx_talkers_destroy.argtypes = [vp]
    L.dspfx_talkers_last_error.restype = C.c_char_p
    L.dspfx_talkers_last_error.argtypes = [vp]
    L.dspfx_talkers_run.argtypes = [vp, f32p, f32p, C.c_uint32, vp]
    L.dspfx_talkers_assign.argtypes = [vp, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_talkers_set_detector.argtypes = [vp, fp, fp, C.c_uint64, C.c_uint64]
    L.dspfx_talkers_set_pin.argtypes = [vp, u8p, C.c_uint64, C.c_uint64]
    L.dspfx_talkers_set_top.argtypes = [vp, u8p, C.c_uint64, C.c_uint64]
    L.dspfx_talkers_set_floor.argtypes = [vp, C.c_float]
    L.dspfx_talkers_reset.argtypes = [vp, C.c_uint64, C.c_uint64]
    L.dspfx_talkers_views.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.dspfx_talkers_room_of.argtypes = [vp, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_talkers_counts.argtypes = [vp, u32p]
    L.dspfx_talkers_audible.argtypes = [fp, fp, u32p, C.c_uint64, C.c_uint32, C.POINTER(C.c_int32), u32p, u32p]
    L.dspfx_talkers_audible_views.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.dspfx_dynamics_plan.argtypes = [C.c_uint64, C.POINTER(C.c_uint64)]
    L.dspfx_dynamics_gain.restype = C.c_float
    L.dspfx_dynamics_gain.argtypes = [C.c_float, C.c_float, C.c_float, fp]
    L.dspfx_dynamics_create.argtypes = [C.POINTER(_DynamicsDesc), C.POINTER(vp)]
    L.dspfx_dynamics_destroy.argtypes = [vp]
    L.dspfx_dynamics_last_error.restype = C.c_char_p
    L.dspfx_dynamics_last_error.argtypes = [vp]
    L.dspfx_dynamics_run.argtypes = [vp, f32p, f32p, f32p, C.c_uint32, vp]
    L.dspfx_dynamics_set.argtypes = [vp, fp, fp, fp, fp, C.c_uint64, C.c_uint64]
    L.dspfx_dynamics_drop.argtypes = [vp, C.c_uint64, C.c_uint64]
    L.dspfx_dynamics_reset.argtypes = [vp, C.c_uint64, C.c_uint64]
    L.dspfx_dynamics_present.argtypes = [vp, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_dynamics_views.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.dspfx_shapers_plan.argtypes = [C.c_uint64, C.POINTER(C.c_uint64)]
    L.dspfx_shapers_create.argtypes = [C.POINTER(_ShapersDesc), C.POINTER(vp)]
    L.dspfx_shapers_destroy.argtypes = [vp]
    L.dspfx_shapers_last_error.restype = C.c_char_p
    L.dspfx_shapers_last_error.argtypes = [vp]
    L.dspfx_shapers_run.argtypes = [vp, f32p, f32p, C.c_uint32, vp]
    L.dspfx_shapers_set_distort.argtypes = [vp, fp, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_shapers_set_overdrive.argtypes = [vp, fp, fp, fp, C.c_uint64, C.c_uint64]
    L.dspfx_shapers_set_chebyshev.argtypes = [vp, fp, fp, C.c_uint64, C.c_uint64]
    L.dspfx_shapers_drop.argtypes = [vp, C.c_uint64, C.c_uint64]
    for name in ("present", "kinds", "modes"):
        getattr(L, f"dspfx_shapers_{name}").argtypes = [vp, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_shapers_sliders.argtypes = [vp, fp, C.c_uint64, C.c_uint64]
    L.dspfx_gens_plan.argtypes = [C.c_uint64, C.POINTER(C.c_uint64)]
    L.dspfx_gens_create.argtypes = [C.POINTER(_GensDesc), C.POINTER(vp)]
    L.dspfx_gens_destroy.argtypes = [vp]
    L.dspfx_gens_last_error.restype = C.c_char_p
    L.dspfx_gens_last_error.argtypes = [vp]
    L.dspfx_gens_run.argtypes = [vp, f32p, f32p, f32p, f32p, C.c_uint32, vp]
    L.dspfx_gens_set.argtypes = [vp, fp, fp, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_gens_drop.argtypes = [vp, C.c_uint64, C.c_uint64]
    L.dspfx_gens_reset.argtypes = [vp, C.c_uint64, C.c_uint64]
    for name in ("present", "modes"):
        getattr(L, f"dspfx_gens_{name}").argtypes = [vp, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_gens_sliders.argtypes = [vp, fp, C.c_uint64, C.c_uint64]
    L.dspfx_gens_clocks.argtypes = [vp, C.POINTER(vp)]
    L.dspfx_blends_plan.argtypes = [C.c_uint64, C.POINTER(C.c_uint64)]
    L.dspfx_blends_create.argtypes = [C.POINTER(_BlendsDesc), C.POINTER(vp)]
    L.dspfx_blends_destroy.argtypes = [vp]
    L.dspfx_blends_last_error.restype = C.c_char_p
    L.dspfx_blends_last_error.argtypes = [vp]
    L.dspfx_blends_run.argtypes = [vp, f32p, f32p, f32p, f32p, f32p, C.c_uint32, vp]
    L.dspfx_blends_set_mix.argtypes = [vp, fp, C.c_uint64, C.c_uint64]
    L.dspfx_blends_set_add.argtypes = [vp, C.c_uint64, C.c_uint64]
    L.dspfx_blends_set_send.argtypes = [vp, fp, C.c_uint64, C.c_uint64]
    L.dspfx_blends_assign.argtypes = [vp, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_blends_drop.argtypes = [vp, C.c_uint64, C.c_uint64]
    for name in ("kinds", "bus_of"):
        getattr(L, f"dspfx_blends_{name}").argtypes = [vp, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_blends_ratios.argtypes = [vp, fp, C.c_uint64, C.c_uint64]
    L.dspfx_blends_sends.argtypes = [vp, fp, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_filters_plan.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    L.dspfx_filters_create.argtypes = [C.POINTER(_FiltersDesc), C.POINTER(vp)]
    L.dspfx_filters_destroy.argtypes = [vp]
    L.dspfx_filters_last_error.restype = C.c_char_p
    L.dspfx_filters_last_error.argtypes = [vp]
    L.dspfx_filters_run.argtypes = [vp, f32p, f32p, C.c_uint32, vp]
    for name in ("set_low_pass", "set_high_pass"):
        getattr(L, f"dspfx_filters_{name}").argtypes = [vp, C.c_uint32, fp, C.c_uint64, C.c_uint64]
    L.dspfx_filters_set_envelope.argtypes = [vp, C.c_uint32, fp, fp, C.c_uint64, C.c_uint64]
    for name in ("drop", "reset"):
        getattr(L, f"dspfx_filters_{name}").argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64]
    L.dspfx_filters_present.argtypes = [vp, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_filters_kinds.argtypes = [vp, C.c_uint32, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_filters_sliders.argtypes = [vp, C.c_uint32, fp, C.c_uint64, C.c_uint64]
    L.dspfx_filters_state.argtypes = [vp, C.c_uint32, C.POINTER(vp)]
    L.dspfx_firs_plan.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    L.dspfx_firs_create.argtypes = [C.POINTER(_FirsDesc), C.POINTER(vp)]
    L.dspfx_firs_destroy.argtypes = [vp]
    L.dspfx_firs_last_error.restype = C.c_char_p
    L.dspfx_firs_last_error.argtypes = [vp]
    L.dspfx_firs_run.argtypes = [vp, f32p, f32p, C.c_uint32, vp]
    L.dspfx_firs_set_taps.argtypes = [vp, C.POINTER(C.c_double), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]
    L.dspfx_firs_set_mode.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64]
    for name in ("drop", "reset"):
        getattr(L, f"dspfx_firs_{name}").argtypes = [vp, C.c_uint64, C.c_uint64]
    for name in ("present", "lengths", "modes"):
        getattr(L, f"dspfx_firs_{name}").argtypes = [vp, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_firs_taps.argtypes = [vp, C.c_uint64, C.POINTER(C.c_double), u32p]
    L.dspfx_firs_deque.argtypes = [vp, C.POINTER(vp)]
    L.dspfx_racks_plan.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    L.dspfx_racks_create.argtypes = [C.POINTER(_RacksDesc), C.POINTER(vp)]
    L.dspfx_racks_destroy.argtypes = [vp]
    L.dspfx_racks_last_error.restype = C.c_char_p
    L.dspfx_racks_last_error.argtypes = [vp]
    L.dspfx_racks_run.argtypes = [vp, f32p, f32p, C.c_uint32, vp]
    L.dspfx_racks_set.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(fp), u32p, C.c_uint64, C.c_uint64]
    for name in ("drop", "reset"):
        getattr(L, f"dspfx_racks_{name}").argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64]
    L.dspfx_racks_present.argtypes = [vp, u32p, C.c_uint64, C.c_uint64]
    for name in ("kinds", "modes"):
        getattr(L, f"dspfx_racks_{name}").argtypes = [vp, C.c_uint32, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_racks_sliders.argtypes = [vp, C.c_uint32, fp, C.c_uint64, C.c_uint64]
    L.dspfx_racks_state.argtypes = [vp, C.c_uint32, C.POINTER(vp)]
    L.dspfx_cancel_plan.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.dspfx_cancel_create.argtypes = [C.POINTER(_CancelDesc), C.POINTER(vp)]
    L.dspfx_cancel_destroy.argtypes = [vp]
    L.dspfx_cancel_last_error.restype = C.c_char_p
    L.dspfx_cancel_last_error.argtypes = [vp]
    L.dspfx_cancel_run.argtypes = [vp, f32p, f32p, f32p, C.c_uint32, vp]
    L.dspfx_cancel_set.argtypes = [vp, u32p, fp, fp, u32p, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_cancel_load.argtypes = [vp, fp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]
    for name in ("drop", "reset"):
        getattr(L, f"dspfx_cancel_{name}").argtypes = [vp, C.c_uint64, C.c_uint64]
    for name in ("present", "lengths", "delays", "adapting"):
        getattr(L, f"dspfx_cancel_{name}").argtypes = [vp, u32p, C.c_uint64, C.c_uint64]
    L.dspfx_cancel_sliders.argtypes = [vp, fp, C.c_uint64, C.c_uint64]
    for name in ("weights_view", "levels_view"):
        getattr(L, f"dspfx_cancel_{name}").argtypes = [vp, C.POINTER(vp)]
    L.dspfx_mixmatrix_run_sparse.argtypes = [vp, f32p, C.c_uint32, f32p, vp, C.c_uint64, vp, vp, vp]
    _lib = L
    return L


def device_count() -> int:
    return int(lib().dspfx_device_count())


def delay_len(seconds: float, page_round: bool = False) -> int:
    """reverb.rs:58 (and the page-rounded reading of rivulet's ring capacity)."""
    return int(lib().dspfx_delay_len(float(seconds), int(page_round)))


def verify_fast_division(c: float, device: int = 0) -> int:
    """Exhaustive (2^32 inputs) check of the fast constant division for divisor c: mismatch count."""
    n = C.c_uint64()
    rc = lib().dspfx_verify_fast_division(device, float(c), C.byref(n))
    if rc != 0:
        raise DspfxError(rc, lib().dspfx_strerror(rc).decode())
    return int(n.value)


class PinnedArray:
    """A numpy array (float32 unless `dtype` says otherwise) over page-locked host memory from dspfx_host_alloc (`.array`);
    freed on close()/GC."""

    def __init__(self, shape, dtype=np.float32):
        dt = np.dtype(dtype)
        n = int(np.prod(shape))
        self._p = C.c_void_p()
        rc = lib().dspfx_host_alloc(max(1, n * dt.itemsize), C.byref(self._p))
        if rc != 0:
            raise DspfxError(rc, lib().dspfx_strerror(rc).decode())
        self.array = np.frombuffer((C.c_char * (n * dt.itemsize)).from_address(self._p.value), dtype=dt, count=n).reshape(shape)

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            self.array = None
            lib().dspfx_host_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def verify_libm(func: int, device: int = 0):
    """Exhaustive comparison of the engine's f64 tanh (0) / sin (1) / atan (2) with the math library's: (differing inputs, max ulp)."""
    n, u = C.c_uint64(), C.c_uint32()
    rc = lib().dspfx_verify_libm(device, int(func), C.byref(n), C.byref(u))
    if rc != 0:
        raise DspfxError(rc, lib().dspfx_strerror(rc).decode())
    return int(n.value), int(u.value)


def link_divisor(n_connected: int) -> np.float32:
    return np.float32(lib().dspfx_link_divisor(int(n_connected)))


def to_layout(x: np.ndarray, tile_channels: int) -> np.ndarray:
    """[n_frames][N] frame-major -> the engine layout for `tile_channels` (flat view)."""
    if not tile_channels:
        return np.ascontiguousarray(x)
    nf, n = x.shape
    w = tile_channels
    return np.ascontiguousarray(x.reshape(nf, n // w, w).transpose(1, 0, 2))


def from_layout(t: np.ndarray, n_frames: int, channels: int, tile_channels: int) -> np.ndarray:
    """inverse of to_layout: -> [n_frames][N]"""
    if not tile_channels:
        return np.asarray(t).reshape(n_frames, channels)
    w = tile_channels
    return np.ascontiguousarray(np.asarray(t).reshape(channels // w, n_frames, w).transpose(1, 0, 2)).reshape(n_frames, channels)


# --------------------------------------------------------------------------- nodes

@dataclass
class NodeSpec:
    kind: int
    params: Sequence[float] = field(default_factory=list)
    mode: int = 0
    delay_len: int = 0
    taps_reversed: Optional[np.ndarray] = None   # as fir.rs:163,168 stores them

    def oracle_desc(self) -> dict:
        """Same node for the CPU oracle (tests only)."""
        return {"kind": self.kind, "params": list(self.params), "mode": self.mode,
                "delay_len": self.delay_len or None, "taps_reversed": self.taps_reversed}


def Gain(level: float = 1.0) -> NodeSpec:
    """nodes/gain.rs: slider level 0..=10, default 1.0"""
    return NodeSpec(GAIN, [level])


def BiQuad(a0=1.0, a1=-0.24, a2=0.0, b0=0.758, b1=0.0, b2=0.0) -> NodeSpec:
    """nodes/biquad.rs:18-41: raw sliders, each -10..=10; normalised by a0 on the engine."""
    return NodeSpec(BIQUAD, [a0, a1, a2, b0, b1, b2])


def LowPass(ratio: float = 0.5) -> NodeSpec:
    """nodes/low_pass.rs: slider ratio 0..=1, default 0.5"""
    return NodeSpec(LOW_PASS, [ratio])


def HighPass(ratio: float = 0.5) -> NodeSpec:
    """nodes/high_pass.rs"""
    return NodeSpec(HIGH_PASS, [ratio])


def Reverb(seconds: Optional[float] = None, decay: float = 0.5, delay_samples: Optional[int] = None,
           page_round: bool = False) -> NodeSpec:
    """nodes/reverb.rs: feedback delay; params = [decay, seconds], mode bit 0 = page_round.
      Reverb(seconds=s)         a restored node: refresh_seconds has run, the ring is reverb.rs:58's length for s;
      Reverb()                  a node fresh from the menu: make_buffer()'s 128-sample ring (reverb.rs:44-52; 1024 under
                                page_round -- the same rivulet calls as refresh_seconds, so the same reading) under the default
                                0.5 s slider -- its first slider change makes it a 24000-sample delay, like the reference's;
      Reverb(delay_samples=D)   an explicit ring and no seconds slider: a slider change swaps in a zero ring of the same D.
    Any set_param on the node -- decay included -- swaps in a NEW ZERO ring (reverb.rs:19, 55-71; include/dspfx.h)."""
    if delay_samples is None:
        if seconds is None:
            return NodeSpec(REVERB, [decay, 0.5], mode=int(page_round), delay_len=delay_len(0.0, page_round))
        delay_samples = delay_len(seconds, page_round)
    return NodeSpec(REVERB, [decay, 0.0 if seconds is None else float(seconds)], mode=int(page_round), delay_len=int(delay_samples))


def Distort(level: float = 0.0, mode: int = SOFT_CLIP) -> NodeSpec:
    """nodes/distort.rs: slider level 0..=30 default 0.0 (=> bypass), mode default SoftClip"""
    return NodeSpec(DISTORT, [level], mode=mode)


def Overdrive(boost: float = 0.0, drive: float = 0.0, level: float = 0.0) -> NodeSpec:
    """nodes/overdrive.rs:21-28 (field order boost, drive, level)"""
    return NodeSpec(OVERDRIVE, [boost, drive, level])


def Chebyshev(level_pos: float = 0.0, level_neg: float = 0.0) -> NodeSpec:
    """nodes/chebyshev.rs:21-25"""
    return NodeSpec(CHEBYSHEV, [level_pos, level_neg])


def Fir(impulse_response=(1.0,), mode: int = FIR_BALANCED) -> NodeSpec:
    """nodes/fir.rs: `impulse_response` is h[0..T) in natural order (what the WAV holds);
    it is stored time-reversed exactly like fir.rs:163,168."""
    h = np.ascontiguousarray(impulse_response, dtype=np.float64)
    return NodeSpec(FIR, [], mode=mode, taps_reversed=np.ascontiguousarray(h[::-1]))


def Add() -> NodeSpec:
    """nodes/add.rs: out = a + b (b = the engine's side input)"""
    return NodeSpec(ADD)


def Mix(ratio: float = 0.5) -> NodeSpec:
    """nodes/mix.rs: out = b*ratio + a*(1-ratio)"""
    return NodeSpec(MIX, [ratio])


def SignalGen(amplitude: float = 0.5, frequency: float = 100.0, mode: int = SIG_SINE) -> NodeSpec:
    """nodes/signal_gen.rs:41-55: a source -- it has no "in" port, so as a chain node it replaces the
    signal (put it first).  Sliders amplitude -1..=1 and frequency 0.1..=20000 Hz are both `as_input`."""
    return NodeSpec(SIGNAL_GEN, [amplitude, frequency], mode=mode)


def Envelope(attack: float = 0.0, release: float = 0.0) -> NodeSpec:
    """nodes/envelope.rs:27-30: peak envelope follower, attack / release in frames (sliders 0..=1000, default 0)."""
    return NodeSpec(ENVELOPE, [attack, release])


# -------------------------------------------------------------------------- engine

# numpy / torch dtype -> dspfx_sample_format (u16: torch.uint16 where torch has it, else fmt=SAMPLE_U16 over an int16 view)
_NP_FORMATS = {np.dtype(np.float32): SAMPLE_F32, np.dtype(np.int16): SAMPLE_I16, np.dtype(np.uint16): SAMPLE_U16,
               np.dtype(np.int32): SAMPLE_I32}
_FORMAT_NP = {v: k for k, v in _NP_FORMATS.items()}


def _np_format(a, fmt=None):
    if fmt is not None:
        return int(fmt)
    if a.dtype not in _NP_FORMATS:
        raise TypeError(f"no device sample format for dtype {a.dtype}: float32, int16, uint16 or int32")
    return _NP_FORMATS[a.dtype]


def _torch_format(t, fmt=None):
    if fmt is not None:
        return int(fmt)
    import torch
    m = {torch.float32: SAMPLE_F32, torch.int16: SAMPLE_I16, torch.int32: SAMPLE_I32}
    if getattr(torch, "uint16", None) is not None:
        m[torch.uint16] = SAMPLE_U16
    if t.dtype not in m:
        raise TypeError(f"no device sample format for dtype {t.dtype}: float32, int16, uint16 or int32 "
                        "(or pass fmt= with a same-width view)")
    return m[t.dtype]


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "data_ptr"):        # torch tensor on the device
        return C.c_void_p(x.data_ptr())
    raise TypeError(f"expected a device tensor or raw pointer, got {type(x)}")


class Engine:
    """N independent mono channels through one effect chain (include/dspfx.h)."""

    def __init__(self, channels: int, max_frames: int = BUF_SIZE, link_flags: int = LINK_INTERNAL | LINK_INPUT,
                 device: int = 0, channel_offset: int = 0, tile_channels: int = 0):
        self.L = lib()
        self.channels, self.max_frames = int(channels), int(max_frames)
        self.h = C.c_void_p()
        d = _EngineDesc(ABI_VERSION, device, channels, max_frames, link_flags, tile_channels, channel_offset)
        self.tile_channels = int(tile_channels)
        rc = self.L.dspfx_engine_create(C.byref(d), C.byref(self.h))
        if rc != 0:
            self.h = C.c_void_p()
            raise DspfxError(rc, self.L.dspfx_strerror(rc).decode())
        self._keep = []

    def _chk(self, rc):
        if rc != 0:
            raise DspfxError(rc, self.L.dspfx_last_error(self.h).decode() or self.L.dspfx_strerror(rc).decode())

    def close(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            self.L.dspfx_engine_destroy(h)
            h.value = None

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown: module globals may already be gone
            pass

    def set_chain(self, nodes: Sequence[NodeSpec]):
        arr = (_NodeDesc * max(1, len(nodes)))()
        self._keep = []
        for i, n in enumerate(nodes):
            arr[i].kind, arr[i].mode = n.kind, n.mode
            for k, v in enumerate(n.params):
                arr[i].params[k] = float(v)
            arr[i].delay_len = int(n.delay_len)
            if n.taps_reversed is not None:
                t = np.ascontiguousarray(n.taps_reversed, dtype=np.float64)
                self._keep.append(t)
                arr[i].n_taps = len(t)
                arr[i].taps = t.ctypes.data_as(C.POINTER(C.c_double))
        self._chk(self.L.dspfx_chain_set(self.h, arr, len(nodes)))
        self.nodes = list(nodes)

    @staticmethod
    def _graph_arrays(nodes, links):
        arr = (_NodeDesc * max(1, len(nodes)))()
        for i, n in enumerate(nodes):
            arr[i].kind, arr[i].mode = n.kind, n.mode
            for k, v in enumerate(n.params):
                arr[i].params[k] = float(v)
            arr[i].delay_len = int(n.delay_len)
        larr = (_GraphLink * max(1, len(links)))()
        for i, (s, d, p) in enumerate(links):
            larr[i].src, larr[i].dst, larr[i].port = int(s), int(d), int(p)
        return arr, larr

    def set_graph(self, nodes: Sequence[NodeSpec], links: Sequence[Tuple[int, int, int]]):
        """A whole DAG as one generated kernel (include/dspfx.h, dspfx_graph_set).  `nodes` in an order in which every
        link goes forward; links = (src, dst, port): src a node index, GRAPH_INPUT or GRAPH_ZERO; dst a node index or
        len(nodes) for the Output node; port PORT_MAIN, PORT_SIDE or PORT_SLIDER + k.  Raises DspfxError with status
        ERR_UNSUPPORTED when the graph cannot be fused."""
        arr, larr = self._graph_arrays(nodes, links)
        self._chk(self.L.dspfx_graph_set(self.h, arr, len(nodes), larr, len(links)))
        self.nodes = list(nodes)

    def kernels_ready(self, wait_ms: int = 60000) -> bool:
        """Adopt the kernels the background compiler has finished for this engine's chain and wait up to wait_ms for the rest
        (dspfx_kernels_ready): True when nothing is pending any more.  Results never depend on it."""
        rc = self.L.dspfx_kernels_ready(self.h, int(wait_ms))
        if rc < 0:
            self._chk(rc)
        return rc == 1

    def set_param(self, node: int, param: int, value: float):
        self._chk(self.L.dspfx_set_param(self.h, node, param, float(value)))

    def set_mode(self, node: int, mode: int):
        self._chk(self.L.dspfx_set_mode(self.h, node, int(mode)))

    def set_param_seq(self, node: int, param: int, value: float) -> int:
        """set_param that also returns the store's sequence number (safe from any thread: the store is queued and
        applied at the next block boundary, dspfx.h)."""
        seq = C.c_uint64()
        self._chk(self.L.dspfx_set_param_seq(self.h, node, param, float(value), C.byref(seq)))
        return int(seq.value)

    def param_log(self, after_seq: int = 0, cap: int = 4096):
        """The stores applied so far with seq > after_seq: [(seq, frame, node, param, value)], oldest first; `frame` =
        frames submitted when the store took effect (param -1: a mode store)."""
        arr = (_ParamEvent * cap)()
        n = self.L.dspfx_param_log(self.h, arr, cap, int(after_seq))
        if n < 0:
            self._chk(n)
        return [(int(a.seq), int(a.frame), int(a.node), int(a.param), float(a.value)) for a in arr[:n]]

    def frames_submitted(self) -> int:
        return int(self.L.dspfx_frames_submitted(self.h))

    def set_delay_len(self, node: int, d: int):
        self._chk(self.L.dspfx_set_delay_len(self.h, node, int(d)))

    def reserve_delay_len(self, node: int, d: int):
        """Capacity hint (any thread, takes no engine lock): the groups a ring of d samples would need are allocated now."""
        self._chk(self.L.dspfx_reserve_delay_len(self.h, node, int(d)))

    def ring_trim(self):
        self._chk(self.L.dspfx_ring_trim(self.h))

    def set_taps(self, node: int, impulse_response, mode: int = FIR_BALANCED):
        t = np.ascontiguousarray(np.asarray(impulse_response, np.float64)[::-1])
        self._chk(self.L.dspfx_set_taps(self.h, node, t.ctypes.data_as(C.POINTER(C.c_double)), len(t), mode))

    def set_fir_precision(self, node: int, precision: int):
        """FIR_PRECISION_DEFAULT / _F32 / _SPLIT (dspfx_set_fir_precision): how the node's steady-state sweep multiplies."""
        self._chk(self.L.dspfx_set_fir_precision(self.h, node, precision))

    def reset(self):
        self._chk(self.L.dspfx_reset(self.h))

    def process(self, x, out=None, side=None, mix=None, n_frames: Optional[int] = None, stream: int = 0, ctl=None):
        """Device path: x/out/side are [n_frames][channels] f32 device tensors (or raw pointers).
        ctl: {(node, slider): device tensor} = connected `as_input` control ports for this block."""
        if n_frames is None:
            n_frames = x.shape[0]
        if out is None:
            out = x
        st = _stream(stream)
        if ctl:
            arr = (_Ctl * len(ctl))()
            for i, ((node, param), sig) in enumerate(ctl.items()):
                arr[i].node, arr[i].param, arr[i].signal = int(node), int(param), _ptr(sig).value
            self._chk(self.L.dspfx_process_ctl(self.h, _ptr(x), _ptr(side), _ptr(out), _ptr(mix), int(n_frames),
                                               arr, len(ctl), st))
        else:
            self._chk(self.L.dspfx_process(self.h, _ptr(x), _ptr(side), _ptr(out), _ptr(mix), int(n_frames), st))
        return out

    def process_bus(self, x, out, mix, n_frames: int, n_connected: int = 0, side=None, stream: int = 0):
        """One block with the Output node complete (dspfx_process_bus): `mix` = this block's bus, summed inside the chain
        launch and divided by link_divisor(n_connected) when n_connected != 0."""
        self._chk(self.L.dspfx_process_bus(self.h, _ptr(x), _ptr(side), _ptr(out), _ptr(mix), int(n_frames),
                                           int(n_connected), _stream(stream)))

    def process_io(self, ins, outs, n_frames: int, mix=None, stream: int = 0):
        """A graph engine with several input / output blocks (dspfx_process_io): ins[k] = input block k, outs[m] = output
        block m; unused entries may be None."""
        ia = (C.c_void_p * max(1, len(ins)))(*[(_ptr(t).value if t is not None else None) for t in ins])
        oa = (C.c_void_p * max(1, len(outs)))(*[(_ptr(t).value if t is not None else None) for t in outs])
        self._chk(self.L.dspfx_process_io(self.h, ia, len(ins), oa, len(outs), _ptr(mix), int(n_frames),
                                          _stream(stream)))
        return outs[0]

    def process_partials(self, x, out=None, side=None, n_frames: Optional[int] = None, stream: int = 0):
        """Pipelined mix bus, part 1 (stream A): the chain, partial sums stay inside the engine."""
        if n_frames is None:
            n_frames = x.shape[0]
        if out is None:
            out = x
        self._chk(self.L.dspfx_process_partials(self.h, _ptr(x), _ptr(side), _ptr(out), int(n_frames),
                                                _stream(stream)))
        return out

    def mix_collect(self, mix, n_frames: int, stream: int = 0):
        """Pipelined mix bus, part 2 (stream B): wait for the chain kernel, reduce partials -> mix[n_frames]."""
        self._chk(self.L.dspfx_mix_collect(self.h, _ptr(mix), int(n_frames), _stream(stream)))

    def process_host(self, x: np.ndarray, side: Optional[np.ndarray] = None, want_mix: bool = False, out=None):
        """Host path (numpy in / numpy out): H2D, process, D2H.  `out` may be a caller-provided (e.g. pinned) array."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.ndim == 2 and x.shape[1] == self.channels, x.shape
        if out is None:
            out = np.empty_like(x)
        assert out.dtype == np.float32 and out.shape == x.shape and out.flags.c_contiguous
        s = np.ascontiguousarray(side, dtype=np.float32) if side is not None else None
        mix = np.empty(x.shape[0], np.float32) if want_mix else None
        self._chk(self.L.dspfx_process_host(self.h, x.ctypes.data, s.ctypes.data if s is not None else None,
                                            out.ctypes.data, mix.ctypes.data if want_mix else None, x.shape[0]))
        return (out, mix) if want_mix else out

    def process_pcm(self, x, out, side=None, mix=None, in_channels: int = 1, out_channels: int = 1, stream: int = 0,
                    n_frames: Optional[int] = None, in_fmt: Optional[int] = None, out_fmt: Optional[int] = None):
        """Device path in device sample formats (dspfx_process_pcm): x / side / out are device tensors in the engine's sample
        layout, [n_frames][channels * device channels]; the format is read from the dtype (float32, int16, int32, uint16 where
        torch has it) unless in_fmt / out_fmt name it (SAMPLE_U16 over an int16 view).  `mix` stays an f32 device tensor."""
        io = _PcmIo(_torch_format(x, in_fmt), int(in_channels), _torch_format(out, out_fmt), int(out_channels))
        if n_frames is None:
            n_frames = x.shape[0]
        self._chk(self.L.dspfx_process_pcm(self.h, C.byref(io), _ptr(x), _ptr(side), _ptr(out), _ptr(mix), int(n_frames),
                                           _stream(stream)))
        return out

    def process_host_pcm(self, x: np.ndarray, out=None, side: Optional[np.ndarray] = None, want_mix: bool = False,
                         in_channels: int = 1, out_channels: int = 1, out_dtype=None, in_fmt: Optional[int] = None,
                         out_fmt: Optional[int] = None):
        """Host path in device sample formats (dspfx_process_host_pcm): x [n_frames][channels * in_channels] numpy (float32,
        int16, uint16, int32; the format from the dtype).  `out` may be a caller-provided (e.g. pinned) array; without one,
        an array of `out_dtype` (default: x's dtype) is made.  Synchronous."""
        x = np.ascontiguousarray(x)
        assert x.ndim == 2 and x.shape[1] == self.channels * in_channels, x.shape
        if out is None:
            out = np.empty((x.shape[0], self.channels * out_channels), dtype=out_dtype or x.dtype)
        assert out.shape == (x.shape[0], self.channels * out_channels) and out.flags.c_contiguous, out.shape
        s = np.ascontiguousarray(side, dtype=x.dtype) if side is not None else None
        io = _PcmIo(_np_format(x, in_fmt), int(in_channels), _np_format(out, out_fmt), int(out_channels))
        mix = np.empty(x.shape[0], np.float32) if want_mix else None
        self._chk(self.L.dspfx_process_host_pcm(self.h, C.byref(io), x.ctypes.data, s.ctypes.data if s is not None else None,
                                                out.ctypes.data, mix.ctypes.data if want_mix else None, x.shape[0]))
        return (out, mix) if want_mix else out

    def mix_finish(self, mix, n_frames: int, n_connected: int, stream: int = 0):
        self._chk(self.L.dspfx_mix_finish(self.h, _ptr(mix), int(n_frames), int(n_connected),
                                          _stream(stream)))

    def mix_allreduce(self, comm: "Comm", mix, n_frames: int, n_connected: int = 0, stream: int = 0):
        """Sum this rank's un-normalised bus over the communicator's ranks (ONE RCCL all-reduce of n_frames floats, in
        place, asynchronous on `stream`), then the Output hop with the global channel count when n_connected != 0."""
        self._chk(self.L.dspfx_mix_allreduce(self.h, comm.h, _ptr(mix), int(n_frames), int(n_connected),
                                             _stream(stream)))

    def tune_placement(self, x, out, n_frames: int, side=None, stream: int = 0):
        """Re-tune the delay rings' placement with the real chain kernels on the caller's buffers (DSP state is kept)."""
        self._chk(self.L.dspfx_tune_placement(self.h, _ptr(x), _ptr(side), _ptr(out), int(n_frames),
                                              _stream(stream)))

    def process_mixpipe(self, x, out, mix, n_frames: int, n_connected: int = 0, side=None, stream: int = 0):
        """One block with the mix bus pipelined inside the chain kernel: `mix` receives the bus of the block
        submitted two calls earlier (divided by link_divisor(n_connected) when n_connected != 0)."""
        self._chk(self.L.dspfx_process_mixpipe(self.h, _ptr(x), _ptr(side), _ptr(out), _ptr(mix), int(n_frames),
                                               int(n_connected), _stream(stream)))

    def mixpipe_flush(self, mix_older, mix_newer, n_connected: int = 0, stream: int = 0):
        self._chk(self.L.dspfx_mixpipe_flush(self.h, _ptr(mix_older), _ptr(mix_newer), int(n_connected),
                                             _stream(stream)))

    def link_average(self, srcs, dst, n_frames: int, stream: int = 0):
        """collect_and_average (node.rs:162-194) of `srcs` (device buffers, link order) into `dst`."""
        arr = (C.c_void_p * max(1, len(srcs)))(*[_ptr(t).value for t in srcs])
        self._chk(self.L.dspfx_link_average(self.h, arr, len(srcs), _ptr(dst), int(n_frames),
                                            _stream(stream)))

    def state_export(self, node: int) -> np.ndarray:
        n = int(self.L.dspfx_state_size(self.h, node))
        if n < 0:
            self._chk(n)
        buf = np.empty(n, np.uint8)
        if n:
            self._chk(self.L.dspfx_state_export(self.h, node, buf.ctypes.data, n))
        return buf

    def state_import(self, node: int, buf: np.ndarray):
        buf = np.ascontiguousarray(buf).view(np.uint8)
        self._chk(self.L.dspfx_state_import(self.h, node, buf.ctypes.data, buf.size))

    def fill_noise(self, dst, n_frames: int, n_abs0: int, seed: int = 0x5EED0001, stream: int = 0):
        self._chk(self.L.dspfx_fill_noise(self.h, _ptr(dst), int(n_frames), int(n_abs0) & 0xFFFFFFFF, seed,
                                          _stream(stream)))

    def sync(self, stream: int = 0):
        self._chk(self.L.dspfx_sync(self.h, _stream(stream)))

    def describe(self) -> str:
        buf = C.create_string_buffer(1 << 16)
        self._chk(self.L.dspfx_describe(self.h, buf, 1 << 16))
        return buf.value.decode()

    def profile_enable(self, launches: int = 1):
        """0 = off; n > 0 = on, with events for n launches created up front."""
        self._chk(self.L.dspfx_profile_enable(self.h, int(launches)))

    def profile_read(self, reset: bool = True):
        """(total kernel ms, launches, kernel name) of the dominant stage since the last reset."""
        ms, n = C.c_double(), C.c_uint32()
        name = C.create_string_buffer(128)
        self._chk(self.L.dspfx_profile_read(self.h, C.byref(ms), C.byref(n), name, 128, int(reset)))
        return ms.value, n.value, name.value.decode()

    def algorithmic_bytes_per_sample(self, n_frames: int) -> float:
        return float(self.L.dspfx_algorithmic_bytes_per_sample(self.h, int(n_frames)))


def comm_unique_id(backend: Optional[str] = None) -> bytes:
    """The 128-byte id rank 0 creates and hands to every rank (dspfx_comm_unique_id).  backend: None = the library's default
    (DSPFX_COMM_BACKEND, else "mailbox"), or "mailbox" / "rccl" for this id."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    old = os.environ.get("DSPFX_COMM_BACKEND")
    if backend is not None:
        os.environ["DSPFX_COMM_BACKEND"] = backend
    try:
        rc = lib().dspfx_comm_unique_id(buf)
    finally:
        if backend is not None:
            if old is None:
                os.environ.pop("DSPFX_COMM_BACKEND", None)
            else:
                os.environ["DSPFX_COMM_BACKEND"] = old
    if rc != 0:
        raise DspfxError(rc, lib().dspfx_comm_last_error(None).decode() or lib().dspfx_strerror(rc).decode())
    return buf.raw


class Comm:
    """The mix bus' communicator: one per process / GPU (include/dspfx.h, dspfx_comm_create).  `uid` = the bytes of
    comm_unique_id() from rank 0 (may be None for a single rank: then no RCCL communicator is created)."""

    def __init__(self, device: int, n_ranks: int, rank: int, uid: Optional[bytes] = None):
        self.L = lib()
        self.h = C.c_void_p()
        self.n_ranks, self.rank = int(n_ranks), int(rank)
        rc = self.L.dspfx_comm_create(int(device), int(n_ranks), int(rank), uid, C.byref(self.h))
        if rc != 0:
            self.h = C.c_void_p()
            raise DspfxError(rc, self.L.dspfx_comm_last_error(None).decode() or self.L.dspfx_strerror(rc).decode())

    @property
    def backend(self) -> str:
        """"mailbox" (one-shot peer-write all-reduce, the default), "rccl" or "single"."""
        return self.L.dspfx_comm_backend(self.h).decode()

    def close(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            self.L.dspfx_comm_destroy(h)
            h.value = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _raise(L, prefix, rc, h=None):
    """rc != 0 -> DspfxError: the reason dspfx_<prefix>_last_error(h) keeps (prefix None: there is none), else the status's name."""
    if rc != 0:
        why = getattr(L, f"dspfx_{prefix}_last_error")(h).decode() if prefix else ""
        raise DspfxError(rc, why or L.dspfx_strerror(rc).decode())


class _Bank:
    """What the bank classes share: the handle `h` of dspfx_<_C>_create, its status checks and its end."""

    _C = ""             # the bank's name in the C ABI
    _WHY = False        # it has a dspfx_<_C>_last_error

    def _create(self, desc):
        self.h = C.c_void_p()
        rc = getattr(self.L, f"dspfx_{self._C}_create")(C.byref(desc), C.byref(self.h))
        if rc != 0:
            self.h = C.c_void_p()
            _raise(self.L, self._C if self._WHY else None, rc)

    def _chk(self, rc):
        _raise(self.L, self._C if self._WHY else None, rc, self.h)

    def close(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            getattr(self.L, f"dspfx_{self._C}_destroy")(h)
            h.value = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _view(self, addr, shape, typestr="<f4"):
        """Device memory of the bank's as a torch tensor that shares it."""
        import torch

        class _Mem:
            __cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (addr, False), "version": 2}
        return torch.as_tensor(_Mem(), device=torch.device("cuda", self.device))


class _InputBank(_Bank):
    """What the banks that take blocks in share (pitch, spectrum, resample): blocks pushed into a ring of slots of `_slot_frames`
    frames each, and the next slot handed out so that an Engine can write its block there."""

    _slot_frames = BUF_SIZE

    def push(self, block, n_frames: Optional[int] = None, stream: int = 0):
        """Append a device block [n_frames][N] (or the tiled form for n_frames); runs what falls due with it (windows, columns).
        slot_tensor() itself: nothing is copied.  A Resampler's full FIFO raises DspfxError(ERR_STATE) and changes nothing."""
        if n_frames is None:
            n_frames = block.numel() // self.channels
        self._chk(getattr(self.L, f"dspfx_{self._C}_push")(self.h, _ptr(block), int(n_frames), _stream(stream)))

    def slot(self) -> Optional[int]:
        """Device address of the next slot (None unless the frames pushed are a multiple of the slot's frames -- 128, a Resampler's
        block_frames -- and, in a Resampler, a slot is free)."""
        return getattr(self.L, f"dspfx_{self._C}_slot")(self.h)

    def slot_tensor(self):
        """The next slot as a float32 device tensor of slot frames * N elements over the bank's own memory (valid while the bank
        lives; None when there is no slot): an Engine writes its block there, then push(slot, frames) copies nothing."""
        addr = self.slot()
        return None if addr is None else self._view(addr, (self._slot_frames * self.channels,))


class _ChannelBank(_Bank):
    """What the per-channel banks share beyond _Bank: the fields every one of them has, how a store's arguments become a channel
    count and arrays of it, a host table read back, a view of a device table, and the output block a run makes."""

    _WHY = True
    _DESC = None        # the bank's description in ctypes: abi_version, device, n_channels, max_frames, tile_channels, then its own fields

    def __init__(self, channels, tile_channels, max_frames, device, *more):
        """The fields, then the bank on the device; `more`: the description's fields behind the common five."""
        self._fields(channels, tile_channels, max_frames, device)
        self._open(*more)

    def _fields(self, channels, tile_channels, max_frames, device):
        self.L = lib()
        self.channels, self.tile_channels, self.max_frames, self.device = int(channels), int(tile_channels), int(max_frames), int(device)

    def _open(self, *more):
        self._create(self._DESC(ABI_VERSION, self.device, self.channels & 0xFFFFFFFF, self.max_frames & 0xFFFFFFFF, self.tile_channels & 0xFFFFFFFF,
                                *more))

    def _span(self, call, first_channel, count):
        """dspfx_<bank>_<call> over `count` channels from first_channel (default: all from it): a drop, a reset."""
        self._chk(getattr(self.L, f"dspfx_{self._C}_{call}")(self.h, int(first_channel), self._n(first_channel, count)))

    def _n(self, first_channel, count):
        return self.channels - int(first_channel) if count is None else int(count)

    def _range(self, first, count, arrays, why, total=None):
        """The entries a store names: the length its arrays agree on (else DspfxError(why)), or, with scalars only, `count`
        (default: all from `first` up to `total`, the channels)."""
        n = None
        for v in arrays:
            if v is not None and np.ndim(v) != 0:
                m = int(np.size(v))
                if n is not None and m != n:
                    raise DspfxError(-1, why)
                n = m
        if n is None:
            n = (self.channels if total is None else total) - int(first) if count is None else int(count)
        return n

    @staticmethod
    def _f32s(values, n):
        """Each of `values` (None, a scalar or an array) as float32[n] -> (the arrays, to be kept until the call returns, and the
        pointers, None for None)."""
        keep = [None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32).reshape(-1), (max(n, 0),)), np.float32)
                for v in values]
        return keep, [None if a is None else a.ctypes.data_as(C.POINTER(C.c_float)) for a in keep]

    def _u32s(self, modes, n, call, what):
        """`modes` (None, a scalar or an array of non-negative integers) as uint32[n] -> (the array, its pointer)."""
        if modes is None:
            return None, None
        m = np.asarray(modes)
        if m.dtype.kind not in "iu" or (m.size and (m.min() < 0 or m.max() > 0xFFFFFFFF)):
            raise DspfxError(-1, f"{self._C} {call}: a mode is one of the {what} values")
        m = np.ascontiguousarray(np.broadcast_to(m.reshape(-1), (max(n, 0),)), np.uint32)
        return m, m.ctypes.data_as(C.POINTER(C.c_uint32))

    def _table(self, name, first_channel, count, dtype=np.uint32, per=1):
        """dspfx_<bank>_<name>: a host table over `count` channels from first_channel (default: all from it), `per` values each."""
        n = self._n(first_channel, count)
        v = np.zeros((max(n, 0), per) if per > 1 else max(n, 0), dtype)
        ct = C.c_float if dtype == np.float32 else C.c_uint32
        self._chk(getattr(self.L, f"dspfx_{self._C}_{name}")(self.h, v.ctypes.data_as(C.POINTER(ct)), int(first_channel), n))
        return v

    def _frames(self, block, n_frames):
        return block.numel() // self.channels if n_frames is None else n_frames

    def _out(self, n_frames):
        import torch
        return torch.empty(int(n_frames) * self.channels, dtype=torch.float32, device=torch.device("cuda", self.device))


def _stream(stream):
    return C.c_void_p(stream) if stream else None


def _plan_bytes(bank, channels, *more) -> int:
    """dspfx_<bank>_plan(channels, more.., &bytes) -> bytes, of the banks whose plan is one byte count."""
    L = lib()
    n = C.c_uint64()
    rc = getattr(L, f"dspfx_{bank}_plan")(int(channels) & 0xFFFFFFFFFFFFFFFF, *[int(m) & 0xFFFFFFFF for m in more], C.byref(n))
    _raise(L, bank, rc)
    return int(n.value)


class PitchBank(_InputBank):
    """The Pitch Detector node (nodes/pitch.rs) for N channels (include/dspfx.h, dspfx_pitch_*): blocks pushed in the layout
    of `tile_channels` (as Engine's), a McLeod pitch and clarity per channel for every 1024 frames, held until the next
    window that gives one.  Device tensors in, device tensors out; asynchronous on `stream` like Engine.process."""

    _C = "pitch"

    def __init__(self, channels: int, device: int = 0, tile_channels: int = 0, power_thresh: float = 0.5,
                 clarity_thresh: float = 0.5, pick_thresh: float = 0.5):
        self.L = lib()
        self.channels, self.tile_channels, self.device = int(channels), int(tile_channels), int(device)
        d = _PitchDesc(ABI_VERSION, self.device, self.channels, self.tile_channels, power_thresh, clarity_thresh, pick_thresh)
        self._create(d)

    def set_param(self, which: int, value: float):
        self._chk(self.L.dspfx_pitch_set_param(self.h, int(which), float(value)))

    def read(self, freq=None, clarity=None, stream: int = 0):
        """-> (freq, clarity), float32 device tensors [N] (made when not given)."""
        import torch
        dev = torch.device("cuda", self.device)
        if freq is None:
            freq = torch.empty(self.channels, dtype=torch.float32, device=dev)
        if clarity is None:
            clarity = torch.empty(self.channels, dtype=torch.float32, device=dev)
        self._chk(self.L.dspfx_pitch_read(self.h, _ptr(freq), _ptr(clarity), _stream(stream)))
        return freq, clarity

    def reset(self):
        self._chk(self.L.dspfx_pitch_reset(self.h))

    @property
    def windows(self) -> int:
        return int(self.L.dspfx_pitch_windows(self.h))



def resample_plan(target_hz: int, value: float, idx: int, n_out: int):
    """dspfx_resample_plan, a pure host function (no GPU): the plan of the next n_out output frames of the 48 kHz -> target_hz
    converter from the state (value, idx).  -> dict(advance uint32[n_out], depth uint32[n_out], coeff float64[n_out][16],
    value, idx, input_len, pulled); coeff[o][2 n] / [2 n + 1] are the left / right coefficient of tap n."""
    import numpy as np
    L = lib()
    adv = np.zeros(n_out, np.uint32)
    dep = np.zeros(n_out, np.uint32)
    coeff = np.zeros((n_out, 16), np.float64)
    v, i, il, pl = C.c_double(value), C.c_uint32(idx), C.c_uint32(0), C.c_uint32(0)
    rc = L.dspfx_resample_plan(int(target_hz), C.byref(v), C.byref(i), int(n_out), adv.ctypes.data_as(C.POINTER(C.c_uint32)),
                               dep.ctypes.data_as(C.POINTER(C.c_uint32)), coeff.ctypes.data_as(C.POINTER(C.c_double)),
                               C.byref(il), C.byref(pl))
    _raise(L, None, rc)
    return {"advance": adv, "depth": dep, "coeff": coeff, "value": v.value, "idx": i.value, "input_len": il.value,
            "pulled": pl.value}


_PCM_TORCH = {SAMPLE_F32: "float32", SAMPLE_I16: "int16", SAMPLE_U16: "int16", SAMPLE_I32: "int32"}


class Resampler(_InputBank):
    """The output resampler bank (include/dspfx.h, dspfx_resample_*): the reference's output callback (devices.rs:394-498) for
    N channels whose device runs at `target_hz`.  Blocks of engine output (48 kHz, the layout of `tile_channels`, as Engine's)
    are pushed into a FIFO of `slots` slots of `block_frames` frames; pull(n_out) is one callback: n_out device frames of
    every channel through dasp's Converter + 16-frame Sinc, in `out_format` with `out_channels` samples per frame.
    Asynchronous on `stream` like Engine.process; the counters are host values."""

    _C = "resample"

    def __init__(self, channels: int, target_hz: int, device: int = 0, tile_channels: int = 0, block_frames: int = BUF_SIZE,
                 slots: int = 4, out_format: int = SAMPLE_F32, out_channels: int = 1):
        self.L = lib()
        self.channels, self.tile_channels, self.device = int(channels), int(tile_channels), int(device)
        self.block_frames, self.slots, self.target_hz = int(block_frames), int(slots), int(target_hz)
        self.out_format, self.out_channels = int(out_format), int(out_channels)
        d = _ResampleDesc(ABI_VERSION, self.device, self.channels, self.tile_channels, self.block_frames, self.slots,
                          self.target_hz, self.out_format, self.out_channels)
        self._create(d)

    @property
    def _slot_frames(self):
        return self.block_frames

    def pull(self, n_out: int, out=None, stream: int = 0):
        """One output callback -> (out, consumed, underrun).  `out` (made when not given) holds n_out * N device frames of
        out_channels samples in the bank's layout for a block of n_out frames: float32 / int16 / int32 (U16 as int16 bits)."""
        import torch
        if out is None:
            out = torch.empty(int(n_out) * self.channels * self.out_channels, dtype=getattr(torch, _PCM_TORCH[self.out_format]),
                              device=torch.device("cuda", self.device))
        used, under = C.c_uint32(0), C.c_int32(0)
        self._chk(self.L.dspfx_resample_pull(self.h, _ptr(out), int(n_out), C.byref(used), C.byref(under),
                                             _stream(stream)))
        return out, int(used.value), bool(under.value)

    @property
    def available(self) -> int:
        """Frames waiting in the FIFO (a host counter)."""
        n = int(self.L.dspfx_resample_available(self.h))
        if n < 0:
            self._chk(n)
        return n

    def skip(self, n_frames: int):
        """Drop the oldest n_frames waiting frames unseen by the converter (the catch-up of devices.rs:410-432)."""
        self._chk(self.L.dspfx_resample_skip(self.h, int(n_frames)))

    def reset(self):
        self._chk(self.L.dspfx_resample_reset(self.h))



def graph_source(nodes: Sequence[NodeSpec], links: Sequence[Tuple[int, int, int]]) -> str:
    """The translation unit `Engine.set_graph` would compile for this graph (needs no device)."""
    L = lib()
    arr, larr = Engine._graph_arrays(nodes, links)
    buf = C.create_string_buffer(1 << 18)
    rc = L.dspfx_graph_source(arr, len(nodes), larr, len(links), buf, len(buf))
    _raise(L, None, rc)
    return buf.value.decode()


def spectrum_plan(fft_size: int):
    """dspfx_spectrum_plan, a pure host function (no GPU): -> (window float32[n], bin_hz float32[n/2]): the default (Hann)
    window table and the physical frequency k * 48000 / n of every bin."""
    L = lib()
    n = int(fft_size)
    ok = 0 < n <= SPECTRUM_MAX_FFT
    win = np.zeros(n if ok else 1, np.float32)
    hz = np.zeros(max(n // 2, 1) if ok else 1, np.float32)
    rc = L.dspfx_spectrum_plan(n & 0xFFFFFFFF, win.ctypes.data_as(C.POINTER(C.c_float)), hz.ctypes.data_as(C.POINTER(C.c_float)))
    _raise(L, None, rc)
    return win, hz


def spectrum_bins(fft_size: int, lower_hz: float, upper_hz: float):
    """The Spectrogram node's frequency bounds as a bin range: -> (k_lo, k_hi, bin_hz[k_lo:k_hi]) with
    lower_hz <= k * 48000 / n <= upper_hz exactly for k_lo <= k < k_hi (a slice of a column's bins; empty: k_lo == k_hi)."""
    _, hz = spectrum_plan(fft_size)
    inside = np.nonzero((hz >= lower_hz) & (hz <= upper_hz))[0]
    if not len(inside):
        return 0, 0, hz[:0]
    k_lo, k_hi = int(inside[0]), int(inside[-1]) + 1
    return k_lo, k_hi, hz[k_lo:k_hi]


class SpectrumBank(_InputBank):
    """The Spectrogram node (nodes/spectrogram.rs) for N channels (include/dspfx.h, dspfx_spectrum_*): blocks pushed in the
    layout of `tile_channels` (as Engine's); every `fft_size` frames one column vol[k] = |FFT(window * x)[k]| * gain[k],
    k in [0, fft_size/2), per channel, the newest `columns` of them kept on the device.  `window` (float32[fft_size]) and
    `gain` (float32[fft_size/2]) are host tables: None = the Hann window of spectrum_plan / 1.0.  audioviz's volume
    normalisation is not restated: a caller that wants it passes it as `gain`.  Asynchronous on `stream` like Engine.process."""

    _C = "spectrum"

    def __init__(self, channels: int, fft_size: int = 512, columns: int = 1, tile_channels: int = 0, window=None, gain=None,
                 device: int = 0):
        self.L = lib()
        self.channels, self.tile_channels, self.device = int(channels), int(tile_channels), int(device)
        self.fft_size, self.columns = int(fft_size), int(columns)
        fp = C.POINTER(C.c_float)
        tables = []
        for name, tab, length in (("window", window, self.fft_size), ("gain", gain, self.fft_size // 2)):
            if tab is not None:
                tab = np.ascontiguousarray(tab, np.float32)
                if tab.shape != (length,):
                    raise ValueError(f"{name} must hold {length} values, not {tab.shape}")
            tables.append(tab)
        d = _SpectrumDesc(ABI_VERSION, self.device, self.channels, self.tile_channels, self.fft_size & 0xFFFFFFFF,
                          self.columns & 0xFFFFFFFF, *(fp() if tab is None else tab.ctypes.data_as(fp) for tab in tables))
        self._create(d)  # the tables are copied before this returns

    def column(self, age: int = 0):
        """The column `age` windows back (0 = the newest): a float32 device tensor of fft_size/2 * N elements over the bank's
        own memory, no copy -- element (k, c) where frame k of channel c is in a block of fft_size/2 frames (frame-major:
        [k][N]).  None when there is no such column (yet, or age >= columns).  It is overwritten `columns` windows later, and
        a read must be ordered after the push that computed it."""
        if age < 0:
            return None
        addr = self.L.dspfx_spectrum_column(self.h, int(age))
        return None if addr is None else self._view(addr, (self.fft_size // 2 * self.channels,))

    def bins(self, lower_hz: float = 20.0, upper_hz: float = 20000.0):
        """spectrum_bins for this bank's fft_size (the defaults are the node's, spectrogram.rs:200-201)."""
        return spectrum_bins(self.fft_size, lower_hz, upper_hz)

    def reset(self):
        self._chk(self.L.dspfx_spectrum_reset(self.h))

    @property
    def windows(self) -> int:
        return int(self.L.dspfx_spectrum_windows(self.h))



def _group_table(channels: int, group_start=None, group_size=None) -> np.ndarray:
    if (group_start is None) == (group_size is None):
        raise ValueError("give group_start (G + 1 channel indices) or group_size (uniform groups), one of them")
    if group_size is not None:
        if int(group_size) < 1 or channels % int(group_size):
            raise ValueError(f"group_size {group_size} does not divide {channels} channels")
        return np.arange(0, channels + 1, int(group_size), dtype=np.uint64)
    t = np.ascontiguousarray(group_start, dtype=np.uint64)
    if t.ndim != 1 or len(t) < 2:
        raise ValueError("group_start holds G + 1 >= 2 channel indices")
    return t


def mixgroups_plan(channels: int, group_start=None, group_size=None, tile_channels: int = 0) -> np.ndarray:
    """dspfx_mixgroups_plan, a pure host function (no GPU): checks the table (DspfxError with the reason when it is bad) and
    -> depth uint32[G]: per group the longest chain of dependent f32 additions in its sum."""
    L = lib()
    t = _group_table(int(channels), group_start, group_size)
    depth = np.zeros(len(t) - 1, np.uint32)
    rc = L.dspfx_mixgroups_plan(t.ctypes.data_as(C.POINTER(C.c_uint64)), len(t) - 1, int(channels), int(tile_channels),
                                depth.ctypes.data_as(C.POINTER(C.c_uint32)))
    _raise(L, "mixgroups", rc)
    return depth


def _room_ids(ids) -> np.ndarray:
    if hasattr(ids, "detach"):
        ids = ids.detach().cpu().numpy()
    v = np.atleast_1d(np.asarray(ids)).reshape(-1)
    if v.size and (v.dtype.kind not in "iu" or v.min() < 0 or v.max() > NO_ROOM):
        raise DspfxError(-1, "room ids are integers in [0, groups), or NO_ROOM")
    return np.ascontiguousarray(v, np.uint32)


def mixgroups_room_plan(room_of, groups: int, tile_channels: int = 0):
    """dspfx_mixgroups_room_plan, a pure host function (no GPU): checks a map -- a room id in [0, groups) or NO_ROOM per channel
    -- (DspfxError with the reason when it is bad) and -> (count uint64[G], depth uint32[G], pieces uint64[G]): per room its
    members, the longest chain of dependent f32 additions in its sum in mapped mode, and its pieces (one per span it has members
    in; their sum sizes the seating's piece buffer).  A room's depth and pieces depend on its own members alone."""
    L = lib()
    v = _room_ids(room_of)
    G = int(groups)
    count, depth, pieces = np.zeros(max(G, 0), np.uint64), np.zeros(max(G, 0), np.uint32), np.zeros(max(G, 0), np.uint64)
    u64 = C.POINTER(C.c_uint64)
    rc = L.dspfx_mixgroups_room_plan(v.ctypes.data_as(C.POINTER(C.c_uint32)), len(v), G & 0xFFFFFFFF, int(tile_channels),
                                     count.ctypes.data_as(u64), depth.ctypes.data_as(C.POINTER(C.c_uint32)), pieces.ctypes.data_as(u64))
    _raise(L, "mixgroups", rc)
    return count, depth, pieces


class MixGroups(_Bank):
    """One Output bus per contiguous channel range, with a per-channel fader (include/dspfx.h, dspfx_mixgroups_*):
    buses[f][g] = (sum over group g of fl32(x[f][c] * gain[c])) / link_divisor(n_g) for a device block in the layout of
    `tile_channels` (as Engine's).  group_start: G + 1 channel indices, nondecreasing from 0 to N; or group_size for uniform
    groups.  normalise=False leaves the raw sums.  run() returns [n_frames, G] float32 on the device: the frame-major block of a
    G-channel Engine(G, tile_channels=0), Resampler(G, ..), PitchBank(G) or SpectrumBank(G).  Asynchronous on `stream`.
    Every channel starts in the room its range puts it in; `assign` reseats channels live among the G rooms (or in none,
    NO_ROOM): run and returns then read "group g" as the channels whose room is g.  A bank that never calls it runs as before."""

    _C = "mixgroups"
    _WHY = True

    def __init__(self, channels: int, group_start=None, group_size=None, tile_channels: int = 0, max_frames: int = BUF_SIZE,
                 normalise: bool = True, device: int = 0):
        self.L = lib()
        self.channels, self.tile_channels, self.device = int(channels), int(tile_channels), int(device)
        self.max_frames, self.normalise = int(max_frames), bool(normalise)
        self.group_start = _group_table(self.channels, group_start, group_size)
        self.groups = len(self.group_start) - 1
        d = _MixGroupsDesc(ABI_VERSION, self.device, self.channels & 0xFFFFFFFF, self.max_frames & 0xFFFFFFFF, self.tile_channels,
                           self.groups, int(self.normalise), self.group_start.ctypes.data_as(C.POINTER(C.c_uint64)))
        self._create(d)  # the table is copied before this returns

    def run(self, block, n_frames: Optional[int] = None, out=None, stream: int = 0):
        """The buses of one device block -> `out` [n_frames, G] float32 on the device (made when not given)."""
        import torch
        if n_frames is None:
            n_frames = block.numel() // self.channels
        if out is None:
            out = torch.empty((int(n_frames), self.groups), dtype=torch.float32, device=torch.device("cuda", self.device))
        self._chk(self.L.dspfx_mixgroups_run(self.h, _ptr(block), int(n_frames), _ptr(out), _stream(stream)))
        return out

    def returns(self, block, n_frames: Optional[int] = None, out=None, buses=None, stream: int = 0):
        """Every channel's room minus itself: out[f][c] = (S[f][g] - x[f][c] * gain[c]) / link_divisor(n_g - 1), S the group's raw
        sum, +0.0 in a group of one; -> `out`, a device block in the layout of `block` (made when not given; out=block works in
        place).  `buses` [n_frames, G], when given, receives what run() writes: the sums are paid for once."""
        import torch
        if n_frames is None:
            n_frames = block.numel() // self.channels
        if out is None:
            out = torch.empty(int(n_frames) * self.channels, dtype=torch.float32, device=torch.device("cuda", self.device))
        self._chk(self.L.dspfx_mixgroups_returns(self.h, _ptr(block), int(n_frames), _ptr(buses) if buses is not None else None,
                                                 _ptr(out), _stream(stream)))
        return out

    def set_gains(self, values, first_channel: int = 0, count: Optional[int] = None):
        """Store the faders of channels [first_channel, first_channel + len(values)); values=None drops the faders of `count`
        channels (default: all from first_channel) back to "not multiplied".  Any thread; applies to the runs submitted after it."""
        if values is None:
            n = self.channels - int(first_channel) if count is None else int(count)
            self._chk(self.L.dspfx_mixgroups_set_gains(self.h, None, int(first_channel), n))
            return
        v = np.ascontiguousarray(values, np.float32).reshape(-1)
        self._chk(self.L.dspfx_mixgroups_set_gains(self.h, v.ctypes.data_as(C.POINTER(C.c_float)), int(first_channel), len(v)))

    def assign(self, ids, first_channel: int = 0):
        """Seat channels [first_channel, first_channel + len(ids)) in the rooms `ids` (an int for one channel, or any integer
        sequence, numpy array or torch tensor; each in [0, groups) or NO_ROOM).  A bad id, or a range past the channels, stores
        nothing.  Any thread, while runs are in flight: it holds for the runs submitted after it returns.  The channel's fader,
        and its state in the engine, stay where they are."""
        v = _room_ids(ids)
        self._chk(self.L.dspfx_mixgroups_assign(self.h, v.ctypes.data_as(C.POINTER(C.c_uint32)), int(first_channel), len(v)))
        self._mapped = True

    def room_of(self) -> np.ndarray:
        """uint32[channels]: the room of every channel (NO_ROOM: none) as the next run sees it."""
        v = np.zeros(self.channels, np.uint32)
        self._chk(self.L.dspfx_mixgroups_rooms(self.h, v.ctypes.data_as(C.POINTER(C.c_uint32)), 0, len(v)))
        return v

    def counts(self) -> np.ndarray:
        """uint64[G]: the members of every room."""
        r = self.room_of()
        return np.bincount(r[r != NO_ROOM], minlength=self.groups).astype(np.uint64)

    def pieces(self) -> int:
        """The piece rows of the current seating ([pieces][max_frames] f32 on the device); 0 on a bank without a map."""
        if not getattr(self, "_mapped", False):
            return 0
        return int(mixgroups_room_plan(self.room_of(), self.groups, self.tile_channels)[2].sum())

    def depth(self) -> np.ndarray:
        """Per room the longest chain of dependent f32 additions in its sum, for the current seating: mixgroups_plan of the
        table on a bank without a map, mixgroups_room_plan of room_of() once assign has been called."""
        if getattr(self, "_mapped", False):
            return mixgroups_room_plan(self.room_of(), self.groups, self.tile_channels)[1]
        return mixgroups_plan(self.channels, group_start=self.group_start, tile_channels=self.tile_channels)



def _taps_reversed(impulse_response) -> np.ndarray:
    t = np.ascontiguousarray(np.asarray(impulse_response, np.float64).reshape(-1)[::-1])
    if len(t) > CONVOLVE_MAX_TAPS:
        raise DspfxError(-1, f"an impulse response of {len(t)} taps is longer than CONVOLVE_MAX_TAPS = {CONVOLVE_MAX_TAPS}")
    return t


def convolve_plan(impulse_response):
    """dspfx_convolve_plan, a pure host function (no GPU): -> (P, table float32[128, P, 2]): the partitions of the response
    h (in time order) and the f32 response table exactly as the device gets it -- table[k, p] = (re, im) of bin k of the
    256-point FFT of h[128 p : 128 p + 128], zero-padded; table[0, p] = (DC, Nyquist)."""
    L = lib()
    t = _taps_reversed(impulse_response)
    dp = C.POINTER(C.c_double)
    parts = C.c_uint32()
    rc = L.dspfx_convolve_plan(t.ctypes.data_as(dp), len(t), C.byref(parts), None)
    _raise(L, None, rc)
    table = np.zeros((128, int(parts.value), 2), np.float32)
    rc = L.dspfx_convolve_plan(t.ctypes.data_as(dp), len(t), C.byref(parts), table.ctypes.data_as(C.POINTER(C.c_float)))
    _raise(L, None, rc)
    return int(parts.value), table


class Convolver(_Bank):
    """One long impulse response over N channels by partitioned FFT (include/dspfx.h, dspfx_convolve_*): per 128-frame block
    y[n] = fl32(sum_j h[j] x[n - j]) * divisor, divisor 1 (FIR_BALANCED) or 1 / T (FIR_AVERAGE), the FIR node's arithmetic for
    responses too long for its tap table: a convolution reverb on the G buses of a MixGroups.  `impulse_response` is h in
    time order (as Engine.set_taps takes it); `max_taps` reserves history for later set_taps of longer responses (0 = this
    one's length).  Blocks are in the layout of `tile_channels` (as Engine's).  The history starts as silence.  Asynchronous on
    `stream`.
    A bank may hold up to CONVOLVE_MAX_RESPONSES responses and an id per channel: `add_response` / `add_wav` give the next id
    (the one given here is 0, and every channel starts on it), `assign` points channels at an id and keeps their history.
    Each channel gets the bits a Convolver of its response alone would give it."""

    _C = "convolve"

    def __init__(self, channels: int, impulse_response, mode: int = FIR_BALANCED, max_taps: int = 0, tile_channels: int = 0,
                 device: int = 0):
        self.L = lib()
        self.channels, self.tile_channels, self.device = int(channels), int(tile_channels), int(device)
        self.max_taps = int(max_taps)
        t = _taps_reversed(impulse_response)
        d = _ConvolveDesc(ABI_VERSION, self.device, self.channels & 0xFFFFFFFF, self.tile_channels, len(t),
                          self.max_taps & 0xFFFFFFFF, int(mode), t.ctypes.data_as(C.POINTER(C.c_double)))
        self._create(d)  # the taps are copied before this returns
        self.n_taps, self.mode = len(t), int(mode)
        self._responses = [(self.n_taps, self.mode)]                           # (taps, mode) of every response, by id
        self._ids = np.zeros(self.channels, np.uint16)

    @classmethod
    def from_wav(cls, path: str, channels: int, resample: bool = True, **kw):
        """The response from a WAV file exactly as the FIR node loads it (ir.load_impulse_response: channel 0, dasp sinc
        resampling to 48 kHz)."""
        from . import ir
        return cls(channels, ir.load_impulse_response(path, resample=resample), **kw)

    @property
    def partitions(self) -> int:
        """P = ceil(T / 128): the spectra of history one block reads per channel."""
        return (self.n_taps + BUF_SIZE - 1) // BUF_SIZE

    def run(self, block, n_frames: int = BUF_SIZE, out=None, stream: int = 0):
        """One device block of n_frames (a multiple of 128) -> `out`, a device block in the same layout (made when not given;
        out=block works in place)."""
        import torch
        if out is None:
            out = torch.empty(int(n_frames) * self.channels, dtype=torch.float32, device=torch.device("cuda", self.device))
        self._chk(self.L.dspfx_convolve_run(self.h, _ptr(block), _ptr(out), int(n_frames), _stream(stream)))
        return out

    def set_taps(self, impulse_response, mode: Optional[int] = None):
        """Replace the response (at most max_taps long) and keep the history: the reference's reload.  From the next run on."""
        t = _taps_reversed(impulse_response)
        m = self.mode if mode is None else int(mode)
        self._chk(self.L.dspfx_convolve_set_taps(self.h, t.ctypes.data_as(C.POINTER(C.c_double)), len(t), m))
        self.n_taps, self.mode = len(t), m
        self._responses[0] = (len(t), m)

    def add_response(self, impulse_response, mode: int = FIR_BALANCED) -> int:
        """One more response (at most max_taps long, h in time order) -> its id: 1, 2, ...  No channel carries it until `assign`
        says so.  A file load: it allocates the table and waits for the runs already submitted."""
        t = _taps_reversed(impulse_response)
        rid = C.c_uint32()
        self._chk(self.L.dspfx_convolve_response_add(self.h, t.ctypes.data_as(C.POINTER(C.c_double)), len(t), int(mode), C.byref(rid)))
        self._responses.append((len(t), int(mode)))
        return int(rid.value)

    def add_wav(self, path: str, resample: bool = True, mode: int = FIR_BALANCED) -> int:
        """add_response of a WAV file, loaded as from_wav loads it."""
        from . import ir
        return self.add_response(ir.load_impulse_response(path, resample=resample), mode)

    def set_response(self, id: int, impulse_response, mode: Optional[int] = None):
        """Replace response `id` (mode=None keeps its mode) and leave the others, the ids and the history alone; id 0 is set_taps."""
        rid = int(id)
        if not 0 <= rid < len(self._responses):
            raise DspfxError(-1, f"the bank holds {len(self._responses)} responses: no id {rid}")
        t = _taps_reversed(impulse_response)
        m = self._responses[rid][1] if mode is None else int(mode)
        self._chk(self.L.dspfx_convolve_response_set(self.h, rid, t.ctypes.data_as(C.POINTER(C.c_double)), len(t), m))
        self._responses[rid] = (len(t), m)
        if rid == 0:
            self.n_taps, self.mode = len(t), m

    def assign(self, ids, first_channel: int = 0):
        """Point channels [first_channel, first_channel + len(ids)) at the responses `ids` (an int for one channel, or any
        integer sequence, numpy array or torch tensor) and keep their history: from the next run on a channel sounds as if its
        new response had been there all along.  An id the bank does not hold, or a range past the channels, stores nothing."""
        if hasattr(ids, "detach"):
            ids = ids.detach().cpu().numpy()
        v = np.atleast_1d(np.asarray(ids)).reshape(-1)
        if v.size and (v.dtype.kind not in "iu" or v.min() < 0 or v.max() > 0xFFFF):
            raise DspfxError(-1, "response ids are integers in [0, responses)")
        v = np.ascontiguousarray(v, np.uint16)
        self._chk(self.L.dspfx_convolve_assign(self.h, v.ctypes.data_as(C.POINTER(C.c_uint16)), int(first_channel), len(v)))
        self._ids[int(first_channel):int(first_channel) + len(v)] = v

    @property
    def responses(self) -> int:
        """How many responses the bank holds (dspfx_convolve_response_count)."""
        n = self.L.dspfx_convolve_response_count(self.h)
        if n < 0:
            self._chk(n)
        return int(n)

    @property
    def response_of(self) -> np.ndarray:
        """uint16[channels]: the response id of every channel (a host copy)."""
        return self._ids.copy()

    def reset(self):
        """Back to silence (ahead of the next run)."""
        self._chk(self.L.dspfx_convolve_reset(self.h))



def strips_coeffs(raw6) -> np.ndarray:
    """dspfx_strips_coeffs, a pure host function (no GPU): the raw BiQuad sliders a0, a1, a2, b0, b1, b2 -> float32[5] =
    a1, a2, b0, b1, b2 normalised as regenerate_filter does (biquad.rs:66-70), exactly as the device gets them."""
    L = lib()
    r = np.ascontiguousarray(raw6, np.float32).reshape(-1)
    if len(r) != 6:
        raise DspfxError(-1, "a BiQuad band is six raw sliders: a0, a1, a2, b0, b1, b2")
    out = np.zeros(5, np.float32)
    rc = L.dspfx_strips_coeffs(r.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)))
    _raise(L, None, rc)
    return out


class ChannelStrips(_ChannelBank):
    """Per-channel Gain and BiQuad sliders (include/dspfx.h, dspfx_strips_*): the strip of channel c is a chain of up to
    1 + `bands` optional nodes in a fixed order -- a Gain node, then BiQuad bands 0 .. bands-1 -- each with the channel's own
    slider values, over a device block in the layout of `tile_channels` (as Engine's).  A node exists for a channel from the
    first store that names it until it is dropped (None); a fresh bank copies its input.  `link_flags` as Engine's: the
    collect_and_average hops into a channel's first present node (LINK_INPUT) and between its present nodes (LINK_INTERNAL).
    Between eng.process and MixGroups.run / returns, or ahead of the chain.  Asynchronous on `stream`."""

    _C = "strips"
    _DESC = _StripsDesc

    def __init__(self, channels: int, bands: int = 1, tile_channels: int = 0, max_frames: int = BUF_SIZE, link_flags: int = 0,
                 device: int = 0):
        self.bands, self.link_flags = int(bands), int(link_flags)
        super().__init__(channels, tile_channels, max_frames, device, self.bands & 0xFFFFFFFF, self.link_flags & 0xFFFFFFFF)

    def run(self, block, n_frames: Optional[int] = None, out=None, stream: int = 0):
        """One device block through every channel's strip -> `out`, a device block in the same layout (made when not given;
        out=block works in place)."""
        n_frames = self._frames(block, n_frames)
        if out is None:
            out = self._out(n_frames)
        self._chk(self.L.dspfx_strips_run(self.h, _ptr(block), _ptr(out), int(n_frames), _stream(stream)))
        return out

    def set_gain(self, levels, first_channel: int = 0, count: Optional[int] = None):
        """Store the Gain level of channels from first_channel: an array (one level per channel), or a scalar for `count`
        channels (default: all from first_channel); levels=None drops the Gain node of `count` channels.  Any thread; applies
        to the runs submitted after it."""
        first = int(first_channel)
        if levels is None or np.ndim(levels) == 0:
            n = self._n(first, count)
            if levels is None:
                self._chk(self.L.dspfx_strips_set_gain(self.h, None, first, n))
                return
            levels = np.full(max(n, 0), levels, np.float32)
        v = np.ascontiguousarray(levels, np.float32).reshape(-1)
        self._chk(self.L.dspfx_strips_set_gain(self.h, v.ctypes.data_as(C.POINTER(C.c_float)), first, len(v)))

    def set_band(self, band: int, coeffs, first_channel: int = 0, count: Optional[int] = None):
        """Store BiQuad band `band` of channels from first_channel: `coeffs` is [count][6] raw sliders a0, a1, a2, b0, b1, b2
        (one row per channel), or one 6-vector for `count` channels (default: all from first_channel); coeffs=None drops the
        band.  The store zeroes the band's state on exactly those channels, as the reference's slider change does.  Any thread;
        applies to the runs submitted after it."""
        first = int(first_channel)
        if coeffs is None or np.ndim(coeffs) == 1:
            n = self._n(first, count)
            if coeffs is None:
                self._chk(self.L.dspfx_strips_set_band(self.h, int(band) & 0xFFFFFFFF, None, first, n))
                return
            coeffs = np.tile(np.asarray(coeffs, np.float32).reshape(1, -1), (max(n, 0), 1))
        v = np.ascontiguousarray(coeffs, np.float32)
        if v.ndim != 2 or v.shape[1] != 6:
            raise DspfxError(-1, "a BiQuad band is six raw sliders per channel: a0, a1, a2, b0, b1, b2")
        self._chk(self.L.dspfx_strips_set_band(self.h, int(band) & 0xFFFFFFFF, v.ctypes.data_as(C.POINTER(C.c_float)), first, len(v)))

    def present(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: the node mask of every channel as the next run sees it; bit 0 = Gain, bit 1 + b = band b."""
        return self._table("present", first_channel, count)

    def reset(self):
        """Zero all state (on the stream last used); the sliders and the nodes stay."""
        self._chk(self.L.dspfx_strips_reset(self.h))



def delays_plan(channels: int, max_seconds: float = 0.5, page_round: bool = False):
    """dspfx_delays_plan, a pure host function (no GPU): (cap, bytes) of a ChannelDelays bank -- the ring frames per channel,
    delay_len(max_seconds, page_round), and the ring bytes, channels * cap * 4.  Refuses what the bank's create would."""
    L = lib()
    cap, nbytes = C.c_uint32(), C.c_uint64()
    rc = L.dspfx_delays_plan(int(channels) & 0xFFFFFFFFFFFFFFFF, float(max_seconds), int(bool(page_round)), C.byref(cap), C.byref(nbytes))
    _raise(L, "delays", rc)
    return int(cap.value), int(nbytes.value)


class ChannelDelays(_ChannelBank):
    """Per-channel Reverb (feedback delay) sliders (include/dspfx.h, dspfx_delays_*): channel c may carry one Reverb node with
    its own `seconds` and `decay` and its own ring of delay_len(seconds, page_round) frames, over a device block in the layout of
    `tile_channels` (as Engine's).  A node exists for a channel from the first store that names it until it is dropped; a fresh
    bank copies its input.  Every store is the reference's slider change: the stored channels start again from a zero ring.
    `max_seconds` sizes the rings (delays_plan).  `link_flags` as Engine's: LINK_INPUT puts the collect_and_average hop ahead of
    the node.  Where ChannelStrips goes: between eng.process and the room mixes.  Asynchronous on `stream`."""

    _C = "delays"
    _DESC = _DelaysDesc

    def __init__(self, channels: int, max_seconds: float = 0.5, tile_channels: int = 0, max_frames: int = BUF_SIZE, link_flags: int = 0,
                 page_round: bool = False, device: int = 0):
        self.max_seconds, self.link_flags, self.page_round = float(max_seconds), int(link_flags), bool(page_round)
        super().__init__(channels, tile_channels, max_frames, device, self.max_seconds, int(self.page_round), self.link_flags & 0xFFFFFFFF)

    def run(self, block, n_frames: Optional[int] = None, out=None, stream: int = 0):
        """One device block through every channel's delay -> `out`, a device block in the same layout (made when not given;
        out=block works in place)."""
        n_frames = self._frames(block, n_frames)
        if out is None:
            out = self._out(n_frames)
        self._chk(self.L.dspfx_delays_run(self.h, _ptr(block), _ptr(out), int(n_frames), _stream(stream)))
        return out

    def set_delay(self, seconds=None, decay=None, first_channel: int = 0, count: Optional[int] = None):
        """Store the sliders of channels from first_channel: arrays (one value per channel) or scalars for `count` channels
        (default: all from first_channel).  A slider left None keeps each channel's value (0.5 where never stored); both None
        drops the node of `count` channels.  Every stored channel starts again from a zero ring, as the reference's slider
        change does.  Refused whole when a channel would need more than the bank's ring.  Any thread; applies to the runs
        submitted after it."""
        n = self._range(first_channel, count, (seconds, decay), "delays set_delay: seconds and decay name different numbers of channels")
        keep, ptrs = self._f32s((seconds, decay), n)
        self._chk(self.L.dspfx_delays_set_delay(self.h, *ptrs, int(first_channel), n))

    def present(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: 1 where the channel carries a node, as every store made so far left it."""
        return self._table("present", first_channel, count)

    def lengths(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: every channel's ring length D, 0 where there is no node."""
        return self._table("lengths", first_channel, count)

    def reset(self):
        """Every present channel's ring back to zeros (on the stream last used); the sliders and the nodes stay."""
        self._chk(self.L.dspfx_delays_reset(self.h))


def envelope_gain(frames: float) -> np.float32:
    """dspfx_envelope_gain, a pure host function: attack or release frames -> the detector's gain, 0 for 0 frames, else
    powf(e, -1 / frames) -- what Talkers.set_detector stores and what an Engine computes for its Envelope node."""
    return np.float32(lib().dspfx_envelope_gain(float(frames)))


def talkers_plan(channels: int, groups: int) -> int:
    """dspfx_talkers_plan, a pure host function (no GPU): the device bytes of a Talkers bank's tables, 29 per channel and 69 per
    room plus 4 (a bank that hands out Talkers.audible() holds 4 per channel and 4 per room more)."""
    return _plan_bytes("talkers", channels, groups)


def _u8_per(values, n: int, what: str) -> np.ndarray:
    """a scalar or [n] small integers -> uint8[n]"""
    v = np.asarray(values)
    if v.dtype.kind not in "iu" or v.size not in (1, n) or (v.size and (v.min() < 0 or v.max() > 255)):
        raise DspfxError(-1, f"{what}: one small integer, or one per entry")
    return np.ascontiguousarray(np.broadcast_to(v.reshape(-1), (n,)), np.uint8)


def talkers_select(levels, room_of, groups: int, top=3, floor: float = 0.0, pins=None):
    """dspfx_talkers_select, a pure host function (no GPU): the bank's selection rule on host arrays.  levels float32[N] (as the bank
    leaves them: non-negative, no NaN), room_of [N] (a room in [0, groups) or NO_ROOM), top a scalar or [groups] (1 .. 8), pins
    None (all TALKERS_AUTO) or [N] -> (talkers int32[groups, 8], -1 where there is none; talker_levels float32[groups, 8]; target
    float32[N]: 1.0 for a talker or an OPEN pin, 0.0 otherwise).  Per room the candidates are the AUTO members with level > floor,
    ranked by level descending, then channel ascending."""
    L = lib()
    lv = np.ascontiguousarray(levels, np.float32).reshape(-1)
    ro = _room_ids(room_of)
    if len(ro) != len(lv):
        raise DspfxError(-1, "talkers select: levels and room_of name different numbers of channels")
    G = max(int(groups), 0)
    tp = _u8_per(top, G, "talkers select: top")
    pn = None if pins is None else _u8_per(pins, len(lv), "talkers select: pins")
    talk, tl, tg = np.full((G, TALKERS_MAX_TOP), -1, np.int32), np.zeros((G, TALKERS_MAX_TOP), np.float32), np.zeros(len(lv), np.float32)
    u8p, fp = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    rc = L.dspfx_talkers_select(lv.ctypes.data_as(fp), ro.ctypes.data_as(C.POINTER(C.c_uint32)), len(lv), G, tp.ctypes.data_as(u8p), float(floor),
                                pn.ctypes.data_as(u8p) if pn is not None else None, talk.ctypes.data_as(C.POINTER(C.c_int32)),
                                tl.ctypes.data_as(fp), tg.ctypes.data_as(fp))
    _raise(L, "talkers", rc)
    return talk, tl, tg


def talkers_audible(gate, target, room_of, groups: int):
    """dspfx_talkers_audible, a pure host function (no GPU): which members of each room can be non-zero in the block a gated run
    is about to gate.  gate, target float32[N] as that run finds them, room_of [N] (a room in [0, groups) or NO_ROOM) ->
    (list int32[N], start uint32[groups + 1], count uint32[groups]): a channel is audible iff its gate or its target is not
    +-0.0, and room r's audible members, in ascending channel order, are list[start[r] : start[r] + count[r]] (the entries of a
    segment past its count, and those past start[groups], are unspecified).  What Talkers.audible() holds on the device."""
    L = lib()
    g = np.ascontiguousarray(gate, np.float32).reshape(-1)
    t = np.ascontiguousarray(target, np.float32).reshape(-1)
    ro = _room_ids(room_of)
    if not len(g) == len(t) == len(ro):
        raise DspfxError(-1, "talkers audible: gate, target and room_of name different numbers of channels")
    G = max(int(groups), 0)
    lst, start, count = np.full(len(g), -1, np.int32), np.zeros(G + 1, np.uint32), np.zeros(G, np.uint32)
    fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    rc = L.dspfx_talkers_audible(g.ctypes.data_as(fp), t.ctypes.data_as(fp), ro.ctypes.data_as(u32p), len(g), G,
                                 lst.ctypes.data_as(C.POINTER(C.c_int32)), start.ctypes.data_as(u32p), count.ctypes.data_as(u32p))
    _raise(L, "talkers", rc)
    return lst, start, count


class Talkers(_ChannelBank):
    """Per-channel levels and each room's loudest, gated live (include/dspfx.h, dspfx_talkers_*): every channel has its own Envelope
    node (attack and release in frames, `set_detector`), every room -- group_start / group_size as MixGroups takes them, 1 .. 1024
    members, reseated live by `assign` -- gets its `top` loudest members chosen on the device, and run() passes those members and
    ramps the others out, over a device block in the layout of `tile_channels` (as Engine's).  A run first gates with the targets
    the run before left, then meters, then selects: a selection is audible one block later, and a fresh bank copies its first
    block.  Between ChannelStrips / ChannelDelays and the room mixes.  Asynchronous on `stream`."""

    _C = "talkers"
    _DESC = _TalkersDesc
    _ENTRIES = "talkers: the arrays name different numbers of entries"

    def __init__(self, channels: int, group_start=None, group_size=None, top: int = 3, tile_channels: int = 0, max_frames: int = BUF_SIZE,
                 device: int = 0):
        self._fields(channels, tile_channels, max_frames, device)
        self.top = int(top)
        self.group_start = _group_table(self.channels, group_start, group_size)
        self.groups = len(self.group_start) - 1
        self._open(self.groups, self.top & 0xFFFFFFFF, self.group_start.ctypes.data_as(C.POINTER(C.c_uint64)))  # (the table is copied in there)
        ptrs = [C.c_void_p() for _ in range(4)]
        self._chk(self.L.dspfx_talkers_views(self.h, *[C.byref(p) for p in ptrs]))
        self._views = [p.value for p in ptrs]
        self._audible = None                              # the three device addresses of audible(), once it has been asked for

    def run(self, block, n_frames: Optional[int] = None, out=None, gate: bool = True, stream: int = 0):
        """One device block: gate it with the targets of the run before -> `out`, a device block in the same layout (made when not
        given; out=block works in place), then meter it and choose every room's talkers.  gate=False only meters and selects: no
        sample is written, the gates stay, and None is returned."""
        n_frames = self._frames(block, n_frames)
        if not gate:
            out = None
        elif out is None:
            out = self._out(n_frames)
        self._chk(self.L.dspfx_talkers_run(self.h, _ptr(block), _ptr(out) if out is not None else None, int(n_frames), _stream(stream)))
        return out

    def set_detector(self, attack=None, release=None, first_channel: int = 0, count: Optional[int] = None):
        """Store the attack and release sliders (frames) of channels from first_channel: arrays (one value per channel) or scalars
        for `count` channels (default: all from first_channel).  A slider left None keeps each channel's value.  No envelope is
        touched.  Any thread; applies to the runs submitted after it."""
        n = self._range(first_channel, count, (attack, release), self._ENTRIES)
        keep, ptrs = self._f32s((attack, release), n)
        self._chk(self.L.dspfx_talkers_set_detector(self.h, *ptrs, int(first_channel), n))

    def set_pin(self, pins, first_channel: int = 0, count: Optional[int] = None):
        """Store the pins of channels from first_channel (TALKERS_AUTO, TALKERS_OPEN: always passed and never ranked, TALKERS_SHUT:
        never passed): an array, or one value for `count` channels (default: all from first_channel)."""
        n = self._range(first_channel, count, (pins,), self._ENTRIES)
        v = _u8_per(pins, max(n, 0), "talkers set_pin")
        self._chk(self.L.dspfx_talkers_set_pin(self.h, v.ctypes.data_as(C.POINTER(C.c_uint8)), int(first_channel), n))

    def set_top(self, tops, first_room: int = 0, count: Optional[int] = None):
        """Store the top (1 .. 8) of rooms from first_room: an array, or one value for `count` rooms (default: all from first_room)."""
        n = self._range(first_room, count, (tops,), self._ENTRIES, self.groups)
        v = _u8_per(tops, max(n, 0), "talkers set_top")
        self._chk(self.L.dspfx_talkers_set_top(self.h, v.ctypes.data_as(C.POINTER(C.c_uint8)), int(first_room), n))

    def set_floor(self, floor: float):
        """Store the bank's floor: only a level strictly above it makes a candidate."""
        self._chk(self.L.dspfx_talkers_set_floor(self.h, float(floor)))

    def assign(self, ids, first_channel: int = 0):
        """Seat channels [first_channel, first_channel + len(ids)) in the rooms `ids` (an int for one channel, or any integer
        sequence, numpy array or torch tensor; each in [0, groups) or NO_ROOM).  A bad id, a range past the channels, or a room
        that would exceed 1024 members stores nothing.  Any thread, while runs are in flight: it holds for the runs submitted after
        it returns."""
        v = _room_ids(ids)
        self._chk(self.L.dspfx_talkers_assign(self.h, v.ctypes.data_as(C.POINTER(C.c_uint32)), int(first_channel), len(v)))

    def reset(self, first_channel: int = 0, count: Optional[int] = None):
        """Envelope and level back to 0, gate and target to 1 on `count` channels from first_channel (default: all from it); queued
        like a store.  The way out for a channel whose envelope became NaN."""
        self._span("reset", first_channel, count)

    def room_of(self) -> np.ndarray:
        """uint32[channels]: the room of every channel (NO_ROOM: none) by every assign made so far."""
        v = np.zeros(self.channels, np.uint32)
        self._chk(self.L.dspfx_talkers_room_of(self.h, v.ctypes.data_as(C.POINTER(C.c_uint32)), 0, len(v)))
        return v

    def counts(self) -> np.ndarray:
        """uint32[G]: the members of every room."""
        v = np.zeros(self.groups, np.uint32)
        self._chk(self.L.dspfx_talkers_counts(self.h, v.ctypes.data_as(C.POINTER(C.c_uint32))))
        return v

    def audible(self):
        """(list int32[channels], start uint32[groups + 1], count uint32[groups]) on the device: room r's audible members -- those
        whose gate or target was not +-0.0 when the last gated run began, the only ones that can be non-zero in the block it
        gated -- in ascending channel order, are list[start[r] : start[r] + count[r]].  The first call allocates the tables and
        switches the bank on: every gated run submitted after it also writes them (one more kernel, ahead of the gate).  Valid
        after a gated run, on its stream; a metering run leaves them.  What MixMatrix.run(sources=...) takes."""
        if self._audible is None:
            ptrs = [C.c_void_p() for _ in range(3)]
            self._chk(self.L.dspfx_talkers_audible_views(self.h, *[C.byref(p) for p in ptrs]))
            self._audible = [p.value for p in ptrs]
        lst, start, count = self._audible
        return (self._view(lst, (self.channels,), "<i4"), self._view(start, (self.groups + 1,), "<u4"),
                self._view(count, (self.groups,), "<u4"))

    def levels(self):
        """float32[channels] on the device: every channel's largest envelope of the last block (valid after a run, on its stream)."""
        return self._view(self._views[0], (self.channels,), "<f4")

    def targets(self):
        """float32[channels] on the device: 1.0 where the next gated run passes the channel, 0.0 where it ramps it out."""
        return self._view(self._views[1], (self.channels,), "<f4")

    def talkers(self):
        """int32[groups, 8] on the device: every room's talkers, loudest first, -1 where there is none."""
        return self._view(self._views[2], (self.groups, TALKERS_MAX_TOP), "<i4")

    def talker_levels(self):
        """float32[groups, 8] on the device: the talkers' levels, 0.0 where there is none."""
        return self._view(self._views[3], (self.groups, TALKERS_MAX_TOP), "<f4")


def dynamics_plan(channels: int) -> int:
    """dspfx_dynamics_plan, a pure host function (no GPU): the device bytes of a ChannelDynamics bank's tables, 29 per channel."""
    return _plan_bytes("dynamics", channels)


def dynamics_gain(env: float, threshold: float, makeup: float = 1.0):
    """dspfx_dynamics_gain, a pure host function (no GPU): the gain computer on one envelope value -> (makeup * q, q) as float32,
    q = env > threshold ? threshold / env : 1 -- the factor a ChannelDynamics run multiplies the sample by, bit for bit."""
    q = C.c_float()
    g = lib().dspfx_dynamics_gain(float(env), float(threshold), float(makeup), C.byref(q))
    return np.float32(g), np.float32(q.value)


class ChannelDynamics(_ChannelBank):
    """Per-channel levellers and limiters (include/dspfx.h, dspfx_dynamics_*): channel c may carry its own Envelope node (attack and
    release in frames) feeding its own gain computer, q = env > threshold ? threshold / env : 1, out = in * (makeup * q), over a
    device block in the layout of `tile_channels` (as Engine's).  A node exists for a channel from the first `set` that names it
    until `drop`; a fresh bank copies its input.  A limiter: set(threshold=ceiling, release=..) -- attack 0 is a brick wall at
    threshold * makeup.  A leveller towards `target` with at most `max_gain`: set(threshold=target / max_gain, makeup=max_gain,
    ..).  Ahead of Talkers as a leveller, behind the room mixes as a limiter.  Asynchronous on `stream`."""

    _C = "dynamics"
    _DESC = _DynamicsDesc

    def __init__(self, channels: int, tile_channels: int = 0, max_frames: int = BUF_SIZE, device: int = 0):
        super().__init__(channels, tile_channels, max_frames, device)
        ptrs = [C.c_void_p() for _ in range(2)]
        self._chk(self.L.dspfx_dynamics_views(self.h, *[C.byref(p) for p in ptrs]))
        self._views = [p.value for p in ptrs]

    def run(self, block, n_frames: Optional[int] = None, out=None, key=None, stream: int = 0):
        """One device block through every channel's dynamics -> `out`, a device block in the same layout (made when not given;
        out=block works in place).  `key`, a device block of the same shape, is what the detector follows instead of `block`
        (key=block is no key); it must not overlap `out` unless it is `block`."""
        n_frames = self._frames(block, n_frames)
        if out is None:
            out = self._out(n_frames)
        self._chk(self.L.dspfx_dynamics_run(self.h, _ptr(block), _ptr(key) if key is not None else None, _ptr(out), int(n_frames), _stream(stream)))
        return out

    def set(self, threshold=None, makeup=None, attack=None, release=None, first_channel: int = 0, count: Optional[int] = None):
        """Store the sliders of channels from first_channel, and give each of them its node: arrays (one value per channel) or
        scalars for `count` channels (default: all from first_channel).  A slider left None keeps each channel's value (attack 0,
        release 0, threshold 1, makeup 1 where never stored).  No envelope is touched.  Refused whole: a threshold that is NaN or
        below +0.0, a makeup that is NaN, infinite or negative, a range past the channels.  Any thread; applies to the runs
        submitted after it."""
        sliders = (threshold, makeup, attack, release)
        n = self._range(first_channel, count, sliders, "dynamics set: the arrays name different numbers of channels")
        keep, ptrs = self._f32s(sliders, n)
        self._chk(self.L.dspfx_dynamics_set(self.h, *ptrs, int(first_channel), n))

    def drop(self, first_channel: int = 0, count: Optional[int] = None):
        """Remove the node of `count` channels from first_channel (default: all from it) and clear their envelope; queued like a
        store."""
        self._span("drop", first_channel, count)

    def reset(self, first_channel: int = 0, count: Optional[int] = None):
        """Envelope and level back to 0 and reduction to 1 on `count` channels from first_channel (default: all from it); the
        sliders and the nodes stay; queued like a store.  The way out for a channel whose envelope became NaN."""
        self._span("reset", first_channel, count)

    def present(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: 1 where the channel carries a node, as every store made so far left it."""
        return self._table("present", first_channel, count)

    def levels(self):
        """float32[channels] on the device: every channel's largest envelope of the last block, 0.0 without a node (valid after a
        run, on its stream)."""
        return self._view(self._views[0], (self.channels,))

    def reductions(self):
        """float32[channels] on the device: every channel's smallest q of the last block -- 1.0 where it was never turned down."""
        return self._view(self._views[1], (self.channels,))


def shapers_plan(channels: int) -> int:
    """dspfx_shapers_plan, a pure host function (no GPU): the device bytes of a ChannelShapers bank's tables, 13 per channel."""
    return _plan_bytes("shapers", channels)


class ChannelShapers(_ChannelBank):
    """Per-channel waveshapers (include/dspfx.h, dspfx_shapers_*): channel c may carry one node of its own -- Distort with its own
    level and mode, Overdrive or Chebyshev with their own sliders -- over a device block in the layout of `tile_channels` (as
    Engine's).  A node exists for a channel from the first `set_*` that names it until `drop`; a fresh bank copies its input.  A
    channel's output is bit for bit what Engine([that node], link_flags=0) writes for it.  A `set_*` of another family than the
    channel carries replaces its node, which starts from the reference's defaults (every slider 0, mode SOFT_CLIP) for what the
    call leaves None; a `set_*` of the same family keeps what it leaves None.  While a channel carries FUZZ, which is block-global
    over 128 frames, n_frames must be a multiple of 128.  Several shapers per channel are several banks.  Asynchronous on
    `stream`."""

    _C = "shapers"
    _DESC = _ShapersDesc

    def __init__(self, channels: int, tile_channels: int = 0, max_frames: int = BUF_SIZE, device: int = 0):
        super().__init__(channels, tile_channels, max_frames, device)

    def run(self, block, n_frames: Optional[int] = None, out=None, stream: int = 0):
        """One device block through every channel's shaper -> `out`, a device block in the same layout (made when not given;
        out=block works in place)."""
        n_frames = self._frames(block, n_frames)
        if out is None:
            out = self._out(n_frames)
        self._chk(self.L.dspfx_shapers_run(self.h, _ptr(block), _ptr(out), int(n_frames), _stream(stream)))
        return out

    def _store(self, call, values, modes, first_channel, count):
        n = self._range(first_channel, count, tuple(values) + (modes,), f"shapers {call}: the arrays name different numbers of channels")
        keep, args = self._f32s(values, n)
        if call == "set_distort":
            m, mp = self._u32s(modes, n, call, "DSPFX_DIST_*")
            args.append(mp)
        self._chk(getattr(self.L, f"dspfx_shapers_{call}")(self.h, *args, int(first_channel), n))

    def set_distort(self, level=None, mode=None, first_channel: int = 0, count: Optional[int] = None):
        """Give channels from first_channel a Distort node: `level` and `mode` (HARD_CLIP .. CHEBYSHEV4) are arrays (one value per
        channel) or scalars for `count` channels (default: all from first_channel).  None keeps a Distort channel's value and is
        the default (0, SOFT_CLIP) where the channel carries another node or none.  Values are taken as given (no clamp).  An
        unknown mode or a range past the channels refuses the whole store.  Any thread; applies to the runs submitted after it."""
        self._store("set_distort", (level,), mode, first_channel, count)

    def set_overdrive(self, boost=None, drive=None, level=None, first_channel: int = 0, count: Optional[int] = None):
        """... an Overdrive node (sliders boost, drive, level; the defaults are 0).  Rules as set_distort."""
        self._store("set_overdrive", (boost, drive, level), None, first_channel, count)

    def set_chebyshev(self, level_pos=None, level_neg=None, first_channel: int = 0, count: Optional[int] = None):
        """... a Chebyshev node (sliders level_pos, level_neg; the defaults are 0).  Rules as set_distort."""
        self._store("set_chebyshev", (level_pos, level_neg), None, first_channel, count)

    def drop(self, first_channel: int = 0, count: Optional[int] = None):
        """Remove the node of `count` channels from first_channel (default: all from it): a copy again; queued like a store."""
        self._span("drop", first_channel, count)

    def present(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: 1 where the channel carries a node, as every store made so far left it."""
        return self._table("present", first_channel, count)

    def kinds(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: DISTORT, OVERDRIVE, CHEBYSHEV, or SHAPERS_NONE without a node."""
        return self._table("kinds", first_channel, count)

    def modes(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: a Distort node's mode, SHAPERS_NONE for every other channel."""
        return self._table("modes", first_channel, count)

    def sliders(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """float32[count, 3]: the sliders in the order of the node's constructor, 0 where there are fewer and without a node."""
        return self._table("sliders", first_channel, count, np.float32, 3)


def gens_plan(channels: int) -> int:
    """dspfx_gens_plan, a pure host function (no GPU): the device bytes of a ChannelGenerators bank's tables, 13 per channel."""
    return _plan_bytes("gens", channels)


class ChannelGenerators(_ChannelBank):
    """Per-channel Signal Generators (include/dspfx.h, dspfx_gens_*): channel c may carry one generator of its own -- amplitude,
    frequency, mode (SIG_SINE .. SIG_CONSTANT) and clock -- over device blocks in the layout of `tile_channels` (as Engine's).  A
    source that lives on the device: a node exists for a channel from the first `set` that names it until `drop`, starts as the
    reference's (0.5, 100 Hz, Sine, clock 0) and keeps its clock through every later `set`; a fresh bank writes +0.0.  A channel's
    sample is bit for bit what Engine([SignalGen(amplitude, frequency, mode)], link_flags=0) writes for it over the same sequence
    of block lengths.  Unlike the reference, a control block is connected per call and is not latched into the slider.
    Asynchronous on `stream`."""

    _C = "gens"
    _DESC = _GensDesc

    def __init__(self, channels: int, tile_channels: int = 0, max_frames: int = BUF_SIZE, device: int = 0):
        super().__init__(channels, tile_channels, max_frames, device)
        p = C.c_void_p()
        self._chk(self.L.dspfx_gens_clocks(self.h, C.byref(p)))
        self._clock = p.value

    def run(self, n_frames: int, out=None, add_to=None, amplitude=None, frequency=None, stream: Optional[int] = None):
        """`n_frames` frames of every channel's generator -> `out`, a device block in the bank's layout (made when not given); a
        channel without a node gets +0.0.  `add_to`, a device block of the same shape: out = add_to + sample, add_to's own bits
        without a node (out=add_to works in place).  `amplitude`, `frequency`: device blocks of the same shape on the node's control
        ports, mapped per sample from [-1, 1] onto -1 .. 1 and 0.1 .. 20000; the stored sliders are not changed."""
        if out is None:
            out = self._out(n_frames)
        opt = [_ptr(b) if b is not None else None for b in (add_to, amplitude, frequency)]
        self._chk(self.L.dspfx_gens_run(self.h, *opt, _ptr(out), int(n_frames), _stream(stream)))
        return out

    def set(self, amplitude=None, frequency=None, mode=None, first_channel: int = 0, count: Optional[int] = None):
        """Give channels from first_channel a generator: `amplitude`, `frequency` and `mode` (SIG_SINE .. SIG_CONSTANT) are arrays
        (one value per channel) or scalars for `count` channels (default: all from first_channel).  None keeps the value of a
        channel that carries a node and is the default (0.5, 100, SIG_SINE) where it carries none.  Values are taken as given (no
        clamp); a node's clock is kept.  An unknown mode or a range past the channels refuses the whole store.  Any thread; applies
        to the runs submitted after it."""
        n = self._range(first_channel, count, (amplitude, frequency, mode), "gens set: the arrays name different numbers of channels")
        keep, args = self._f32s((amplitude, frequency), n)
        m, mp = self._u32s(mode, n, "set", "DSPFX_SIG_*")
        self._chk(self.L.dspfx_gens_set(self.h, *args, mp, int(first_channel), n))

    def drop(self, first_channel: int = 0, count: Optional[int] = None):
        """Remove the node of `count` channels from first_channel (default: all from it): +0.0 again, and a later `set` starts from
        the defaults at clock 0; queued like a store."""
        self._span("drop", first_channel, count)

    def reset(self, first_channel: int = 0, count: Optional[int] = None):
        """Clock back to +0.0 on the channels of the range that carry a node; sliders, modes and nodes stay; queued like a store."""
        self._span("reset", first_channel, count)

    def present(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: 1 where the channel carries a node, as every store made so far left it."""
        return self._table("present", first_channel, count)

    def modes(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: the node's SIG_* mode, GENS_NONE without a node."""
        return self._table("modes", first_channel, count)

    def sliders(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """float32[count, 2]: amplitude and frequency, 0 without a node."""
        return self._table("sliders", first_channel, count, np.float32, 2)

    def clocks(self):
        """float32[channels] on the device: every channel's clock, the phase carried between blocks; +0.0 without a node (valid
        after a run, on its stream)."""
        return self._view(self._clock, (self.channels,))


def blends_plan(channels: int) -> int:
    """dspfx_blends_plan, a pure host function (no GPU): the device bytes of a ChannelBlends bank's tables, 13 per channel (ratio,
    send level, bus id and a kind / presence byte)."""
    return _plan_bytes("blends", channels)


class ChannelBlends(_ChannelBank):
    """Per-channel Add and Mix nodes (include/dspfx.h, dspfx_blends_*): channel c may carry an Add node or a Mix node with a ratio
    of its own, a send (a Gain node on the node's second input) and a bus id, over device blocks in the layout of `tile_channels`
    (as Engine's).  The second input of a run is an N-channel block `b`, or a [n_frames][buses] frame-major `bus` block that channel
    c reads at bus_of[c] (+0.0 on NO_ROOM), or nothing (+0.0).  A fresh bank copies `a`.  A channel's sample is bit for bit what
    Engine([Mix(ratio)], link_flags=0).process(a, side=b) -- or Engine([Add()]) -- writes for it.  group_size / group_start (as
    MixGroups takes them) make one bus per group and assign every channel its group's.  Unlike the reference, the control block is
    connected per call and is not latched into the slider.  Asynchronous on `stream`."""

    _C = "blends"
    _DESC = _BlendsDesc

    def __init__(self, channels: int, buses: int = 0, tile_channels: int = 0, max_frames: int = BUF_SIZE, device: int = 0,
                 group_size=None, group_start=None):
        self._fields(channels, tile_channels, max_frames, device)
        table = None
        if group_size is not None or group_start is not None:
            table = _group_table(self.channels, group_start, group_size)
            if buses not in (0, len(table) - 1):
                raise ValueError(f"buses {buses} is not the {len(table) - 1} groups of the table")
            buses = len(table) - 1
        self.buses = int(buses)
        self._open(self.buses & 0xFFFFFFFF)
        if table is not None:
            self.assign(np.repeat(np.arange(self.buses, dtype=np.uint32), np.diff(table).astype(np.int64)))

    def run(self, a, n_frames: Optional[int] = None, b=None, bus=None, ratio=None, out=None, stream: Optional[int] = None):
        """One device block `a` -> `out`, a device block in the same layout (made when not given; out=a and out=b work in place).
        `b`: a device block of a's shape, or `bus`: a device block [n_frames][buses]; with neither, the second input is +0.0.
        `ratio`: a device block of a's shape on the Mix nodes' control port, mapped per sample from [-1, 1] onto 0 .. 1; the stored
        ratios are not changed.  Both b and bus, or bus on a bank of buses=0, is refused."""
        n_frames = self._frames(a, n_frames)
        if out is None:
            out = self._out(n_frames)
        opt = [_ptr(t) if t is not None else None for t in (b, bus, ratio)]
        self._chk(self.L.dspfx_blends_run(self.h, _ptr(a), *opt, _ptr(out), int(n_frames), _stream(stream)))
        return out

    def set_mix(self, ratio=None, first_channel: int = 0, count: Optional[int] = None):
        """Give channels from first_channel a Mix node: `ratio` is an array (one value per channel) or a scalar for `count` channels
        (default: all from first_channel).  None keeps the ratio of a channel that carries a Mix node and is 0.5 where it carries
        none or an Add node.  Values are taken as given (no clamp).  A range past the channels refuses the whole store.  Any
        thread; applies to the runs submitted after it."""
        n = self._range(first_channel, count, (ratio,), "blends set_mix: the array names another number of channels")
        keep, args = self._f32s((ratio,), n)
        self._chk(self.L.dspfx_blends_set_mix(self.h, args[0], int(first_channel), n))

    def set_add(self, first_channel: int = 0, count: Optional[int] = None):
        """Give `count` channels from first_channel (default: all from it) an Add node; queued like every store."""
        self._span("set_add", first_channel, count)

    def set_send(self, level, first_channel: int = 0, count: Optional[int] = None):
        """Give channels from first_channel a send, a Gain node on the second input: `level` is an array or a scalar for `count`
        channels.  level=None removes the send."""
        n = self._range(first_channel, count, (level,), "blends set_send: the array names another number of channels")
        keep, args = self._f32s((level,), n)
        self._chk(self.L.dspfx_blends_set_send(self.h, args[0], int(first_channel), n))

    def assign(self, ids, first_channel: int = 0):
        """Channels [first_channel, first_channel + len(ids)) read the buses `ids` (an int for one channel, or any integer sequence,
        numpy array or torch tensor; each in [0, buses) or NO_ROOM).  A bad id or a range past the channels stores nothing.  Any
        thread, while runs are in flight: it holds for the runs submitted after it returns."""
        v = _room_ids(ids)
        self._chk(self.L.dspfx_blends_assign(self.h, v.ctypes.data_as(C.POINTER(C.c_uint32)), int(first_channel), len(v)))

    def drop(self, first_channel: int = 0, count: Optional[int] = None):
        """Remove the node and the send of `count` channels from first_channel (default: all from it): a copy of `a` again; the bus
        id stays; queued like a store."""
        self._span("drop", first_channel, count)

    def kinds(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: ADD, MIX or BLENDS_NONE, as every store made so far left it."""
        return self._table("kinds", first_channel, count)

    def ratios(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """float32[count]: the Mix node's ratio, 0 for every other channel."""
        return self._table("ratios", first_channel, count, np.float32)

    def sends(self, first_channel: int = 0, count: Optional[int] = None):
        """(level float32[count], present uint32[count]): the send's level and whether the channel has one.  A presence array and
        not a NaN: a level is taken as given, NaN included.  An absent send's level reads 0."""
        n = self._n(first_channel, count)
        level, present = np.zeros(max(n, 0), np.float32), np.zeros(max(n, 0), np.uint32)
        self._chk(self.L.dspfx_blends_sends(self.h, level.ctypes.data_as(C.POINTER(C.c_float)), present.ctypes.data_as(C.POINTER(C.c_uint32)),
                                            int(first_channel), n))
        return level, present

    def bus_of(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: the bus of every channel (NO_ROOM: none) by every assign made so far."""
        return self._table("bus_of", first_channel, count)


def filters_plan(channels: int, stages: int = 1) -> int:
    """dspfx_filters_plan, a pure host function (no GPU): the device bytes of a ChannelFilters bank's tables, 13 per channel and
    stage (two sliders, the state, the kind byte)."""
    return _plan_bytes("filters", channels, stages)


class ChannelFilters(_ChannelBank):
    """Per-channel one-pole filters and envelope followers (include/dspfx.h, dspfx_filters_*): channel c owns `stages` slots
    (1 .. 4), run in slot order, each empty or a LowPass, a HighPass or an Envelope node (whose output is the envelope) with its own
    sliders, over a device block in the layout of `tile_channels` (as Engine's).  An empty slot copies; a fresh bank copies its
    input.  A channel's output is bit for bit what Engine([its present nodes in slot order], link_flags=0) writes for it, however
    the frames are cut into runs.  A slot's node is new (state +0.0; ratio 0.5, attack 0, release 0 for what the call leaves None)
    from the first `set_*` that names it and after a `set_*` of another kind; a `set_*` of the kind it carries keeps what the call
    leaves None and keeps the state.  Asynchronous on `stream`."""

    _C = "filters"
    _DESC = _FiltersDesc

    def __init__(self, channels: int, stages: int = 1, tile_channels: int = 0, max_frames: int = BUF_SIZE, device: int = 0):
        self.stages = int(stages)
        super().__init__(channels, tile_channels, max_frames, device, self.stages & 0xFFFFFFFF)

    def run(self, block, n_frames: Optional[int] = None, out=None, stream: int = 0):
        """One device block through every channel's slots -> `out`, a device block in the same layout (made when not given;
        out=block works in place)."""
        n_frames = self._frames(block, n_frames)
        if out is None:
            out = self._out(n_frames)
        self._chk(self.L.dspfx_filters_run(self.h, _ptr(block), _ptr(out), int(n_frames), _stream(stream)))
        return out

    def _store(self, call, stage, values, first_channel, count):
        n = self._range(first_channel, count, values, f"filters {call}: the arrays name different numbers of channels")
        keep, args = self._f32s(values, n)
        self._chk(getattr(self.L, f"dspfx_filters_{call}")(self.h, int(stage) & 0xFFFFFFFF, *args, int(first_channel), n))

    def set_low_pass(self, stage: int, ratio=None, first_channel: int = 0, count: Optional[int] = None):
        """Give slot `stage` of channels from first_channel a LowPass node: `ratio` is an array (one value per channel) or a scalar
        for `count` channels (default: all from first_channel).  None keeps a LowPass slot's ratio and is the default 0.5 where
        the slot carries another node or none.  Values are taken as given (no clamp).  A stage that is not one of the bank's or a
        range past the channels refuses the whole store.  Any thread; applies to the runs submitted after it."""
        self._store("set_low_pass", stage, (ratio,), first_channel, count)

    def set_high_pass(self, stage: int, ratio=None, first_channel: int = 0, count: Optional[int] = None):
        """... a HighPass node.  Rules as set_low_pass."""
        self._store("set_high_pass", stage, (ratio,), first_channel, count)

    def set_envelope(self, stage: int, attack=None, release=None, first_channel: int = 0, count: Optional[int] = None):
        """... an Envelope node (attack and release in frames; the defaults are 0).  Rules as set_low_pass."""
        self._store("set_envelope", stage, (attack, release), first_channel, count)

    def drop(self, stage: int, first_channel: int = 0, count: Optional[int] = None):
        """Empty slot `stage` of `count` channels from first_channel (default: all from it) and zero its state: that stage copies
        again; queued like a store."""
        self._chk(self.L.dspfx_filters_drop(self.h, int(stage) & 0xFFFFFFFF, int(first_channel), self._n(first_channel, count)))

    def reset(self, first_channel: int = 0, count: Optional[int] = None, stage: Optional[int] = None):
        """The state of slot `stage` (None: of every slot) back to +0.0 on `count` channels from first_channel (default: all from
        it); the nodes and the sliders stay; queued like a store.  The way out for a slot whose state became NaN."""
        s = FILTERS_NONE if stage is None else int(stage) & 0xFFFFFFFF
        self._chk(self.L.dspfx_filters_reset(self.h, s, int(first_channel), self._n(first_channel, count)))

    def present(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: 1 where a slot of the channel carries a node, as every store made so far left it."""
        return self._table("present", first_channel, count)

    def _stage_table(self, name, stage, first_channel, count, dtype, per):
        n = self._n(first_channel, count)
        v = np.zeros((max(n, 0), per) if per > 1 else max(n, 0), dtype)
        ct = C.c_float if dtype == np.float32 else C.c_uint32
        self._chk(getattr(self.L, f"dspfx_filters_{name}")(self.h, int(stage) & 0xFFFFFFFF, v.ctypes.data_as(C.POINTER(ct)), int(first_channel), n))
        return v

    def kinds(self, stage: int, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: slot `stage` is LOW_PASS, HIGH_PASS, ENVELOPE, or FILTERS_NONE when empty."""
        return self._stage_table("kinds", stage, first_channel, count, np.uint32, 1)

    def sliders(self, stage: int, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """float32[count, 2]: slot `stage`'s sliders as they were given: ratio, 0 | attack, release (frames); 0, 0 when empty."""
        return self._stage_table("sliders", stage, first_channel, count, np.float32, 2)

    def state(self, stage: int):
        """float32[channels] on the device: slot `stage`'s z or envelope after the last run, +0.0 when empty (valid after a run, on
        its stream)."""
        p = C.c_void_p()
        self._chk(self.L.dspfx_filters_state(self.h, int(stage) & 0xFFFFFFFF, C.byref(p)))
        return self._view(p.value, (self.channels,))


def racks_plan(channels: int, slots: int = 4) -> int:
    """dspfx_racks_plan, a pure host function (no GPU): the device bytes of a ChannelRacks bank's tables, 37 per channel and slot
    (five slider fields, four state floats, the kind byte)."""
    return _plan_bytes("racks", channels, slots)


# the kinds a rack slot may carry and their slider counts; every other kind is refused by the library with a reason
_RACK_SLIDERS = {GAIN: 1, BIQUAD: 6, LOW_PASS: 1, HIGH_PASS: 1, ENVELOPE: 2, DISTORT: 1, OVERDRIVE: 3, CHEBYSHEV: 2}


class ChannelRacks(_ChannelBank):
    """A per-channel chain of mixed nodes in one pass (include/dspfx.h, dspfx_racks_*): channel c owns `slots` slots (1 .. 4), run
    in slot order, each empty or any one of Gain, BiQuad, LowPass, HighPass, Envelope, Distort (every mode but FUZZ), Overdrive and
    Chebyshev with its own sliders and state, over a device block in the layout of `tile_channels` (as Engine's).  All slots run
    between one load and one store of the block.  An empty slot copies; a fresh bank copies its input.  A channel's output and
    state are bit for bit what ChannelFilters(stages=1), ChannelStrips(bands=1) and ChannelShapers give when they are run slot
    after slot with the slot's node on that channel; without a BiQuad that is Engine([its present nodes in slot order],
    link_flags=0).  A `set` of a kind the slot does not carry makes a new node (state +0.0, the reference's defaults for what is
    None); a `set` of the kind it carries keeps what is None, keeps the state of LowPass, HighPass and Envelope and zeroes a
    BiQuad's.  Asynchronous on `stream`."""

    _C = "racks"
    _DESC = _RacksDesc

    def __init__(self, channels: int, slots: int = 4, tile_channels: int = 0, max_frames: int = BUF_SIZE, device: int = 0):
        self.slots = int(slots)
        super().__init__(channels, tile_channels, max_frames, device, self.slots & 0xFFFFFFFF)

    def run(self, block, n_frames: Optional[int] = None, out=None, stream: int = 0):
        """One device block through every channel's slots -> `out`, a device block in the same layout (made when not given;
        out=block works in place)."""
        n_frames = self._frames(block, n_frames)
        if out is None:
            out = self._out(n_frames)
        self._chk(self.L.dspfx_racks_run(self.h, _ptr(block), _ptr(out), int(n_frames), _stream(stream)))
        return out

    def set(self, slot: int, node: NodeSpec, first_channel: int = 0, count: Optional[int] = None):
        """Give slot `slot` of channels from first_channel the node `node`, a NodeSpec of the engine's own constructors (Gain,
        BiQuad, LowPass, HighPass, Envelope, Distort, Overdrive, Chebyshev): every slider, and a Distort's mode, is an array (one
        value per channel, all arrays of one store the same length) or a scalar for `count` channels (default: all from
        first_channel).  A slider given as None keeps its value where the slot carries the kind and is the reference's default
        where it carries another or none.  Values are taken as given (no clamp).  A slot the bank does not have, a range past the
        channels, a kind that is not a rack node, an unknown Distort mode or FUZZ refuse the whole store.  Any thread; applies to
        the runs submitted after it."""
        if not isinstance(node, NodeSpec):
            raise DspfxError(-1, "racks set: the node is a NodeSpec (Gain(..), BiQuad(..), LowPass(..), ..)")
        kind = int(node.kind)
        params = list(node.params)
        if kind in _RACK_SLIDERS and len(params) > _RACK_SLIDERS[kind]:
            raise DspfxError(-1, f"racks set: kind {kind} has {_RACK_SLIDERS[kind]} sliders and {len(params)} are given")
        modes = node.mode if kind == DISTORT else None
        n = self._range(first_channel, count, tuple(params) + (modes,), "racks set: the arrays name different numbers of channels")
        keep, ptrs = self._f32s(params, n)
        six = (C.POINTER(C.c_float) * 6)(*[p if p is not None else C.POINTER(C.c_float)() for p in ptrs])
        m, mp = self._u32s(modes, n, "set", "DSPFX_DIST_*")
        self._chk(self.L.dspfx_racks_set(self.h, int(slot) & 0xFFFFFFFF, kind & 0xFFFFFFFF, six, mp, int(first_channel), n))

    def set_chain(self, nodes: Sequence[NodeSpec], first_channel: int = 0, count: Optional[int] = None):
        """Slots 0 .. len(nodes) - 1 of the range from `nodes`, in order (rules as `set`); the slots behind them are dropped."""
        nodes = list(nodes)
        if len(nodes) > self.slots:
            raise DspfxError(-1, f"racks set_chain: {len(nodes)} nodes, and the bank has {self.slots} slots")
        for node in nodes:
            if not isinstance(node, NodeSpec):
                raise DspfxError(-1, "racks set_chain: every node is a NodeSpec (Gain(..), BiQuad(..), LowPass(..), ..)")
        for t, node in enumerate(nodes):
            self.set(t, node, first_channel, count)
        for t in range(len(nodes), self.slots):
            self.drop(t, first_channel, count)

    def drop(self, slot: int, first_channel: int = 0, count: Optional[int] = None):
        """Empty slot `slot` of `count` channels from first_channel (default: all from it) and zero its state: that slot copies
        again; queued like a store."""
        self._chk(self.L.dspfx_racks_drop(self.h, int(slot) & 0xFFFFFFFF, int(first_channel), self._n(first_channel, count)))

    def reset(self, first_channel: int = 0, count: Optional[int] = None, slot: Optional[int] = None):
        """The state of slot `slot` (None: of every slot) back to +0.0 on `count` channels from first_channel (default: all from
        it); the nodes and the sliders stay; queued like a store.  The way out for a slot whose state became NaN."""
        s = RACKS_NONE if slot is None else int(slot) & 0xFFFFFFFF
        self._chk(self.L.dspfx_racks_reset(self.h, s, int(first_channel), self._n(first_channel, count)))

    def present(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: bit t set where slot t of the channel carries a node, as every store made so far left it."""
        return self._table("present", first_channel, count)

    def _slot_table(self, name, slot, first_channel, count, dtype, per):
        n = self._n(first_channel, count)
        v = np.zeros((max(n, 0), per) if per > 1 else max(n, 0), dtype)
        ct = C.c_float if dtype == np.float32 else C.c_uint32
        self._chk(getattr(self.L, f"dspfx_racks_{name}")(self.h, int(slot) & 0xFFFFFFFF, v.ctypes.data_as(C.POINTER(ct)), int(first_channel), n))
        return v

    def kinds(self, slot: int, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: slot `slot`'s kind (GAIN, BIQUAD, LOW_PASS, HIGH_PASS, ENVELOPE, DISTORT, OVERDRIVE, CHEBYSHEV), or
        RACKS_NONE when empty."""
        return self._slot_table("kinds", slot, first_channel, count, np.uint32, 1)

    def modes(self, slot: int, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: the mode of slot `slot`'s Distort node, RACKS_NONE for every other channel."""
        return self._slot_table("modes", slot, first_channel, count, np.uint32, 1)

    def sliders(self, slot: int, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """float32[count, 6]: slot `slot`'s sliders as they were given, in the order of the node's constructor; 0 where the kind
        has fewer and when empty."""
        return self._slot_table("sliders", slot, first_channel, count, np.float32, 6)

    def state(self, slot: int):
        """float32[4, channels] on the device: slot `slot`'s state after the last run -- row 0 the z of a one-pole or the envelope,
        rows 0 .. 3 a BiQuad's x1, x2, y1, y2, +0.0 everywhere else (valid after a run, on its stream)."""
        p = C.c_void_p()
        self._chk(self.L.dspfx_racks_state(self.h, int(slot) & 0xFFFFFFFF, C.byref(p)))
        return self._view(p.value, (4, self.channels))


def firs_plan(channels: int, max_taps: int = 64) -> int:
    """dspfx_firs_plan, a pure host function (no GPU): the device bytes of a ChannelFirs bank's tables,
    channels * (12 * max_taps + 80): max_taps f64 taps, a ring of max_taps + 16 f32 samples, the node word and the three deque
    words per channel."""
    return _plan_bytes("firs", channels, max_taps)


class ChannelFirs(_ChannelBank):
    """Per-channel FIR nodes (include/dspfx.h, dspfx_firs_*): channel c may carry one FIR node of its own -- its own taps (f64),
    tap count T (1 .. max_taps), mode (FIR_BALANCED, FIR_AVERAGE) and deque of past samples -- over a device block in the layout
    of `tile_channels` (as Engine's).  A node exists from the first `set_taps` that names the channel until `drop`; a fresh bank
    copies its input.  A channel's output is bit for bit what the reference's FIR node gives through all its history (the fill
    phase of its VecDeque and the a / b split of the two sums included), however the frames are cut into runs.  `set_taps` on a
    channel that carries a node is the reference's reload: new taps, the deque is kept.  `general_only` makes every wave take the
    frames one at a time (for timing one body of the kernel against the other).  Asynchronous on `stream`."""

    _C = "firs"
    _DESC = _FirsDesc

    def __init__(self, channels: int, max_taps: int = 64, tile_channels: int = 0, max_frames: int = BUF_SIZE, device: int = 0,
                 general_only: bool = False):
        self.max_taps = int(max_taps)
        super().__init__(channels, tile_channels, max_frames, device, self.max_taps & 0xFFFFFFFF, int(bool(general_only)))
        p = C.c_void_p()
        self._chk(self.L.dspfx_firs_deque(self.h, C.byref(p)))
        self._deque = p.value

    def run(self, block, n_frames: Optional[int] = None, out=None, stream: int = 0):
        """One device block through every channel's node -> `out`, a device block in the same layout (made when not given;
        out=block works in place)."""
        n_frames = self._frames(block, n_frames)
        if out is None:
            out = self._out(n_frames)
        self._chk(self.L.dspfx_firs_run(self.h, _ptr(block), _ptr(out), int(n_frames), _stream(stream)))
        return out

    def set_taps(self, impulse_response, first_channel: int = 0, count: Optional[int] = None, mode: Optional[int] = None):
        """Give channels from first_channel a response, in time order as Fir takes it: a 1-d array [T] for `count` channels
        (default: all from first_channel), or a 2-d array [n][T], one response per channel for n channels (`count`, when given,
        must be n).  mode: FIR_BALANCED or FIR_AVERAGE; None keeps the mode of a channel that carries a node and is FIR_BALANCED
        for a new one.  A channel without a node gets a new one (an empty deque); one that carries a node keeps its deque.  T of 0
        or above max_taps, a range past the channels, an unknown mode or an array of another shape refuses the whole store.  Any
        thread; applies to the runs submitted after it."""
        h = np.ascontiguousarray(impulse_response, dtype=np.float64)
        if h.ndim == 1:
            rows, n = 0, self._n(first_channel, count)
        elif h.ndim == 2 and (count is None or int(count) == h.shape[0]):
            rows, n = 1, h.shape[0]
        else:
            raise DspfxError(-1, "firs set_taps: the response is [T], or [count][T] with one row per channel")
        m = FIRS_NONE if mode is None else int(mode) & 0xFFFFFFFF
        self._chk(self.L.dspfx_firs_set_taps(self.h, h.ctypes.data_as(C.POINTER(C.c_double)), h.shape[-1] & 0xFFFFFFFF, rows, m,
                                             int(first_channel), n))

    def set_mode(self, mode: int, first_channel: int = 0, count: Optional[int] = None):
        """The mode (FIR_BALANCED, FIR_AVERAGE) of the nodes of `count` channels from first_channel (default: all from it); a
        channel without a node stays without one; queued like a store."""
        self._chk(self.L.dspfx_firs_set_mode(self.h, int(mode) & 0xFFFFFFFF, int(first_channel), self._n(first_channel, count)))

    def drop(self, first_channel: int = 0, count: Optional[int] = None):
        """Remove the node of `count` channels from first_channel (default: all from it): a copy again, and a later `set_taps`
        makes a new node; queued like a store."""
        self._span("drop", first_channel, count)

    def reset(self, first_channel: int = 0, count: Optional[int] = None):
        """Empty the deque of `count` channels from first_channel (default: all from it); taps and mode stay; queued like a store."""
        self._span("reset", first_channel, count)

    def present(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: 1 where the channel carries a node, as every store made so far left it."""
        return self._table("present", first_channel, count)

    def lengths(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: the node's tap count T, 0 without a node."""
        return self._table("lengths", first_channel, count)

    def modes(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: FIR_BALANCED, FIR_AVERAGE, or FIRS_NONE without a node."""
        return self._table("modes", first_channel, count)

    def taps(self, channel: int) -> np.ndarray:
        """float64[T]: the response of one channel as it was given (time order); empty without a node."""
        v = np.zeros(max(self.max_taps, 1), np.float64)
        n = C.c_uint32()
        self._chk(self.L.dspfx_firs_taps(self.h, int(channel), v.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)))
        return v[:n.value].copy()

    def deque(self):
        """int32[3, channels] on the device: len, cap and head of every channel's VecDeque after the last run (valid after a run,
        on its stream)."""
        return self._view(self._deque, (3, self.channels), "<i4")


def cancel_plan(channels: int, max_taps: int = 64, max_delay: int = 0) -> int:
    """dspfx_cancel_plan, a pure host function (no GPU): the device bytes of a ChannelCancellers bank's tables,
    channels * (4 * max_taps + 4 * R + 24), R = max_delay + max_taps + 16 rounded up to a multiple of 8: max_taps f32 weights, a
    ring of R f32 reference samples, the node word, the delay, mu, eps and the two levels per channel."""
    return _plan_bytes("cancel", channels, max_taps, max_delay)


class ChannelCancellers(_ChannelBank):
    """Per-channel adaptive (NLMS) FIR filters (include/dspfx.h, dspfx_cancel_*): channel c may carry one canceller of its own --
    T taps (1 .. max_taps) that the device updates every frame, a step size mu, a regulariser eps, a bulk delay (0 .. max_delay
    frames) and the switch adapt -- over two device blocks in the layout of `tile_channels` (as Engine's): `mic`, the primary
    input, and `ref`, the block the channel was sent.  out = mic minus the filter's estimate of ref's path into mic.  A node
    exists from the first `set` that names the channel until `drop`; a fresh bank copies mic and reads no ref.  All arithmetic is
    f32 with every operation rounded once (the rule is in include/dspfx.h), so a channel's output, weights and levels are the
    same bits in either layout, in place or not, on any stream, whatever its neighbours carry and however the frames are cut into
    runs.  1024 taps are 21 ms at 48 kHz: line and handset echo behind a bulk delay, not a room's tail.  `general_only` makes
    every wave take the frames one at a time (for showing that both bodies of the kernel give the same bits).  Asynchronous on
    `stream`."""

    _C = "cancel"
    _DESC = _CancelDesc

    def __init__(self, channels: int, max_taps: int = 64, max_delay: int = 0, tile_channels: int = 0, max_frames: int = BUF_SIZE,
                 device: int = 0, general_only: bool = False):
        self.max_taps, self.max_delay = int(max_taps), int(max_delay)
        super().__init__(channels, tile_channels, max_frames, device, self.max_taps & 0xFFFFFFFF, self.max_delay & 0xFFFFFFFF,
                         int(bool(general_only)))
        w, l = C.c_void_p(), C.c_void_p()
        self._chk(self.L.dspfx_cancel_weights_view(self.h, C.byref(w)))
        self._chk(self.L.dspfx_cancel_levels_view(self.h, C.byref(l)))
        self._weights, self._levels = w.value, l.value

    def run(self, mic, n_frames: Optional[int] = None, ref=None, out=None, stream: int = 0):
        """One device block `mic` against the block `ref` the channels were sent -> `out`, a device block in the same layout
        (made when not given; out=mic works in place).  No ref, or an out that overlaps ref, refuses the run."""
        n_frames = self._frames(mic, n_frames)
        if out is None:
            out = self._out(n_frames)
        self._chk(self.L.dspfx_cancel_run(self.h, _ptr(mic), _ptr(ref), _ptr(out), int(n_frames), _stream(stream)))
        return out

    def set(self, taps=None, mu=None, eps=None, delay=None, adapt=None, first_channel: int = 0, count: Optional[int] = None):
        """The node of channels from first_channel: every argument is None (keep), a scalar for `count` channels (default: all
        from first_channel) or an array with one value per channel (all arrays of one store the same length).  A channel without a
        node gets a new one -- weights and history +0.0 and, for what is None, max_taps taps, mu 0.5, eps 1e-6, delay 0,
        adapting; one that carries a node keeps what is None and keeps its weights and history (a smaller `taps` zeroes the rows
        it leaves, a larger one starts the new rows at +0.0).  adapt=False freezes: the node filters and does not update.  Values
        are taken as given (NaN included).  A `taps` of 0 or above max_taps, a `delay` above max_delay, a range past the channels
        or arrays of different lengths refuse the whole store.  Any thread; applies to the runs submitted after it."""
        if adapt is not None:
            adapt = np.asarray(adapt).astype(bool).astype(np.uint32)
        n = self._range(first_channel, count, (taps, mu, eps, delay, adapt), "cancel set: the arrays name different numbers of channels")
        keep, (pm, pe) = self._f32s((mu, eps), n)
        t, pt = self._counts(taps, n, "taps")
        d, pd = self._counts(delay, n, "delay")
        a, pa = self._counts(adapt, n, "adapt")
        self._chk(self.L.dspfx_cancel_set(self.h, pt, pm, pe, pd, pa, int(first_channel), n))

    @staticmethod
    def _counts(v, n, what):
        """`v` (None, a scalar or an array of non-negative integers) as uint32[n] -> (the array, its pointer)."""
        if v is None:
            return None, None
        m = np.asarray(v)
        if m.dtype.kind not in "iu" or (m.size and (m.min() < 0 or m.max() > 0xFFFFFFFF)):
            raise DspfxError(-1, f"cancel set: {what} is a count of frames, or an array of them")
        m = np.ascontiguousarray(np.broadcast_to(m.reshape(-1), (max(n, 0),)), np.uint32)
        return m, m.ctypes.data_as(C.POINTER(C.c_uint32))

    def load(self, rows, first_channel: int = 0, count: Optional[int] = None):
        """A warm start: the weights of channels from first_channel, a 1-d float32 array [T] for `count` channels (default: all
        from first_channel) or a 2-d array [n][T], one row per channel (`count`, when given, must be n); row[k] is w[k].  Every
        channel of the range carries a node of exactly T taps, else the whole store is refused.  Queued like a store."""
        h = np.ascontiguousarray(rows, dtype=np.float32)
        if h.ndim == 1:
            per, n = 0, self._n(first_channel, count)
        elif h.ndim == 2 and (count is None or int(count) == h.shape[0]):
            per, n = 1, h.shape[0]
        else:
            raise DspfxError(-1, "cancel load: the rows are [T], or [count][T] with one row per channel")
        self._chk(self.L.dspfx_cancel_load(self.h, h.ctypes.data_as(C.POINTER(C.c_float)), h.shape[-1] & 0xFFFFFFFF, per, int(first_channel), n))

    def drop(self, first_channel: int = 0, count: Optional[int] = None):
        """Remove the node of `count` channels from first_channel (default: all from it): a copy again, and a later `set` makes a
        new node; queued like a store."""
        self._span("drop", first_channel, count)

    def reset(self, first_channel: int = 0, count: Optional[int] = None):
        """Weights and history of `count` channels from first_channel (default: all from it) back to +0.0; taps, mu, eps, delay
        and adapt stay; queued like a store.  The way out for a channel whose weights became NaN."""
        self._span("reset", first_channel, count)

    def weights(self):
        """float32[max_taps, channels] on the device, row k = w[k] of every channel, +0.0 in the rows k >= a channel's taps: a
        view of the bank's table, no copy (valid after a run, on its stream)."""
        return self._view(self._weights, (self.max_taps, self.channels))

    def levels(self):
        """float32[2, channels] on the device: sum d^2 and sum e^2 of the last run, +0.0 without a node (a view)."""
        return self._view(self._levels, (2, self.channels))

    def present(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: 1 where the channel carries a node, as every store made so far left it."""
        return self._table("present", first_channel, count)

    def lengths(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: the node's tap count T, 0 without a node."""
        return self._table("lengths", first_channel, count)

    def sliders(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """float32[count, 2]: mu and eps as they were given; 0, 0 without a node."""
        return self._table("sliders", first_channel, count, np.float32, 2)

    def delays(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: the node's bulk delay in frames, 0 without a node."""
        return self._table("delays", first_channel, count)

    def adapting(self, first_channel: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint32[count]: 1 where the node updates its weights, 0 frozen or without a node."""
        return self._table("adapting", first_channel, count)


def _seat_counts(seats, groups: int) -> np.ndarray:
    """a scalar or [G] -> uint32[G]"""
    v = np.asarray(seats)
    if v.dtype.kind not in "iu" or v.size not in (1, groups) or (v.size and (v.min() < 0 or v.max() > 0xFFFFFFFF)):
        raise DspfxError(-1, "seats is one count, or one per room")
    return np.ascontiguousarray(np.broadcast_to(v.reshape(-1), (groups,)), np.uint32)


def mixmatrix_plan(channels: int, group_start=None, group_size=None, tile_channels: int = 0, seats=None):
    """dspfx_mixmatrix_plan, a pure host function (no GPU): checks the room table as MixMatrix does (DspfxError with the reason
    when it is bad: an empty room, one above MIXMATRIX_MAX_ROOM, a table that does not cover the channels) and ->
    (count uint32[G], edge uint32[G], offset uint64[G], total_bytes): per room its members, the edge of its padded table (the
    count rounded up to 32) and the element offset of that table, and the bytes of all the tables.  seats (a scalar or [G]):
    dspfx_mixmatrix_plan_seats, the plan of a seated bank, whose edges are the seats rounded up to 32."""
    L = lib()
    t = _group_table(int(channels), group_start, group_size)
    G = len(t) - 1
    count, edge, offset = np.zeros(G, np.uint32), np.zeros(G, np.uint32), np.zeros(G, np.uint64)
    total = C.c_uint64(0)
    u32 = C.POINTER(C.c_uint32)
    if seats is None:
        rc = L.dspfx_mixmatrix_plan(t.ctypes.data_as(C.POINTER(C.c_uint64)), G, int(channels), int(tile_channels), count.ctypes.data_as(u32),
                                    edge.ctypes.data_as(u32), offset.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(total))
    else:
        s = _seat_counts(seats, G)
        rc = L.dspfx_mixmatrix_plan_seats(t.ctypes.data_as(C.POINTER(C.c_uint64)), G, int(channels), int(tile_channels), s.ctypes.data_as(u32),
                                          count.ctypes.data_as(u32), edge.ctypes.data_as(u32), offset.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          C.byref(total))
    _raise(L, "mixmatrix", rc)
    return count, edge, offset, int(total.value)


def mixmatrix_reseat(room_of, seat_of, seats, ids, first_channel: int = 0):
    """dspfx_mixmatrix_reseat, a pure host function (no GPU): MixMatrix.assign's seating rule on host arrays.  room_of, seat_of:
    uint32[N], a room (NO_ROOM: none) and a seat per channel; seats: a scalar or [G], rounded up to 32.  The channels from
    first_channel whose id is not their room leave, then those that enter a room do so in ascending channel order, each into the
    lowest free seat.  -> (room_of, seat_of) after the call, as new arrays; a bad id, a bad range or a room over capacity is a
    DspfxError with the reason, as assign's."""
    L = lib()
    r, q = np.array(room_of, np.uint32).reshape(-1), np.array(seat_of, np.uint32).reshape(-1)
    s = np.atleast_1d(np.asarray(seats)).reshape(-1)
    if len(r) != len(q) or s.dtype.kind not in "iu" or (s.size and (s.min() < 0 or s.max() > 0xFFFFFFFF)):
        raise DspfxError(-1, "room_of and seat_of are [N], seats is [G]")
    s = np.ascontiguousarray(s, np.uint32)
    v = _room_ids(ids)
    u32 = C.POINTER(C.c_uint32)
    rc = L.dspfx_mixmatrix_reseat(r.ctypes.data_as(u32), q.ctypes.data_as(u32), s.ctypes.data_as(u32), len(s), len(r), v.ctypes.data_as(u32),
                                  int(first_channel), len(v))
    _raise(L, "mixmatrix", rc)
    return r, q


def mixmatrix_staging_bytes(channels: int, seats, group_start=None, group_size=None, tile_channels: int = 0, max_frames: int = BUF_SIZE) -> int:
    """dspfx_mixmatrix_staging_bytes, a pure host function (no GPU): the bytes MIXMATRIX_STAGED adds to the seated bank that
    mixmatrix_plan(..., seats=seats) plans: two seat-ordered copies of (the sum of the seats, each rounded up to 32) x max_frames
    float32, and 4 bytes per channel for the channel -> seat table.  The same checks as the plan's."""
    L = lib()
    t = _group_table(int(channels), group_start, group_size)
    G = len(t) - 1
    s = _seat_counts(seats, G)
    total = C.c_uint64(0)
    rc = L.dspfx_mixmatrix_staging_bytes(t.ctypes.data_as(C.POINTER(C.c_uint64)), G, int(channels), int(tile_channels),
                                         s.ctypes.data_as(C.POINTER(C.c_uint32)), int(max_frames) & 0xFFFFFFFF, C.byref(total))
    _raise(L, "mixmatrix", rc)
    return int(total.value)


def mixmatrix_scatter(room_of, seat_of, seats):
    """dspfx_mixmatrix_scatter, a pure host function (no GPU): how scattered a seating is.  room_of, seat_of: uint32[N] as
    mixmatrix_reseat takes them; seats: [G], one count per room.  -> (chunks, lines): the runs of 32 consecutive seats of a room that hold
    anybody (a chunk of the direct run), and, summed over them, the distinct values of channel // 32 among a run's channels (the
    lines the chunk reads per frame).  lines / chunks is 1 at the seating a fresh bank has when its rooms begin at multiples of
    32, and approaches 32 once everybody has wandered: the figure to decide MixMatrix.set_staging by."""
    L = lib()
    r, q = np.ascontiguousarray(room_of, np.uint32).reshape(-1), np.ascontiguousarray(seat_of, np.uint32).reshape(-1)
    s = np.atleast_1d(np.asarray(seats)).reshape(-1)
    if len(r) != len(q) or s.dtype.kind not in "iu" or (s.size and (s.min() < 0 or s.max() > 0xFFFFFFFF)):
        raise DspfxError(-1, "room_of and seat_of are [N], seats is [G]")
    s = np.ascontiguousarray(s, np.uint32)
    u32 = C.POINTER(C.c_uint32)
    chunks, lines = C.c_uint64(0), C.c_uint64(0)
    rc = L.dspfx_mixmatrix_scatter(r.ctypes.data_as(u32), q.ctypes.data_as(u32), s.ctypes.data_as(u32), len(s), len(r), C.byref(chunks), C.byref(lines))
    _raise(L, "mixmatrix", rc)
    return int(chunks.value), int(lines.value)


class MixMatrix(_Bank):
    """Each listener's own mix of their room (include/dspfx.h, dspfx_mixmatrix_*): room r of n_r contiguous channels owns an
    n_r x n_r float32 matrix M[l][s] (listener, source), and out[f][c0 + l] = (sum_s M[l][s] * x[f][c0 + s]) / link_divisor(w),
    w = the listener's non-zero entries (a row of zeros gives +0.0; normalise=False writes the raw sum), for a device block in the
    layout of `tile_channels` (as Engine's).  Rooms as MixGroups takes them: group_start (G + 1 indices) or group_size; every
    room has 1 .. MIXMATRIX_MAX_ROOM members.  A fresh bank holds mix-minus (1.0 off the diagonal), which is MixGroups.returns
    without faders.  Between ChannelStrips.run and the listeners' Resampler, as an alternative to returns.  Asynchronous on
    `stream`.
    seats=None: the rooms are fixed.  seats (a scalar or [G], each at least the room's members, rounded up to 32, at most
    MIXMATRIX_MAX_ROOM): a SEATED bank (dspfx_mixmatrix_create_seats), whose room r owns seats[r] seats and an S_r x S_r table
    that never moves; a channel holds one seat of one room, or none, and `assign` reseats channels live as MixGroups.assign does:
    no table is rebuilt and those who stay keep their gains.  Rows and columns of a seated bank are S_r long and indexed by seat;
    set_pairs addresses gains by channel number on either kind."""

    _C = "mixmatrix"
    _WHY = True

    def __init__(self, channels: int, group_start=None, group_size=None, tile_channels: int = 0, max_frames: int = BUF_SIZE,
                 normalise: bool = True, device: int = 0, abi_version: int = ABI_VERSION, seats=None):
        self.L = lib()
        self.channels, self.tile_channels, self.device = int(channels), int(tile_channels), int(device)
        self.max_frames, self.normalise = int(max_frames), bool(normalise)
        self.group_start = _group_table(self.channels, group_start, group_size)
        self.groups = len(self.group_start) - 1
        d = _MixMatrixDesc(int(abi_version) & 0xFFFFFFFF, self.device, self.channels & 0xFFFFFFFF, self.max_frames & 0xFFFFFFFF,
                           self.tile_channels & 0xFFFFFFFF, self.groups, int(self.normalise),
                           self.group_start.ctypes.data_as(C.POINTER(C.c_uint64)))
        self.seats = None
        if seats is None:
            self._create(d)  # the table is copied before this returns
            return
        s = _seat_counts(seats, self.groups)
        self.h = C.c_void_p()
        rc = self.L.dspfx_mixmatrix_create_seats(C.byref(d), s.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(self.h))
        if rc != 0:
            self.h = C.c_void_p()
            _raise(self.L, "mixmatrix", rc)
        self.seats = (s + 31) // 32 * 32                  # uint32[G]: S_r

    def assign(self, ids, first_channel: int = 0, preset: int = MIXMATRIX_MIX_MINUS):
        """A seated bank: seat channels [first_channel, first_channel + len(ids)) in the rooms `ids` (an int for one channel, or
        any integer sequence, numpy array or torch tensor; each in [0, groups) or NO_ROOM).  A channel whose id is its room keeps
        its seat and its gains; the others leave (their seat's row and column become +0.0), then enter in ascending channel order,
        each into the lowest free seat of its new room, wired by `preset`: MIXMATRIX_MIX_MINUS (1.0 to and from every other
        taken seat) or MIXMATRIX_ZERO (silent both ways: the host stores its own).  A bad id, a range past the channels or a room
        over capacity stores nothing.  Any thread, while runs are in flight; never waits for a run; holds, whole, for the runs
        submitted after it returns."""
        v = _room_ids(ids)
        self._chk(self.L.dspfx_mixmatrix_assign(self.h, v.ctypes.data_as(C.POINTER(C.c_uint32)), int(first_channel), len(v),
                                                int(preset) & 0xFFFFFFFF))

    def room_of(self) -> np.ndarray:
        """uint32[channels]: the room of every channel (NO_ROOM: none) by every call made so far."""
        v = np.zeros(self.channels, np.uint32)
        self._chk(self.L.dspfx_mixmatrix_rooms(self.h, v.ctypes.data_as(C.POINTER(C.c_uint32)), 0, len(v)))
        return v

    def seat_of(self) -> np.ndarray:
        """uint32[channels]: the seat of every channel in its room (0xFFFFFFFF: in no room) by every call made so far."""
        v = np.zeros(self.channels, np.uint32)
        self._chk(self.L.dspfx_mixmatrix_seats(self.h, v.ctypes.data_as(C.POINTER(C.c_uint32)), 0, len(v)))
        return v

    def occupancy(self) -> np.ndarray:
        """uint32[G]: the taken seats of every room."""
        v = np.zeros(self.groups, np.uint32)
        self._chk(self.L.dspfx_mixmatrix_occupancy(self.h, v.ctypes.data_as(C.POINTER(C.c_uint32))))
        return v

    def set_staging(self, mode: int):
        """A seated bank: the mode of the runs submitted after this returns.  MIXMATRIX_DIRECT: the run gathers every seat's channel
        from the block (fastest while the seating is near the one the bank was made with).  MIXMATRIX_STAGED: the block is
        transposed into a seat-ordered copy, the same chain runs over it and the result is transposed back, so the cost does not
        depend on the seating, the bits are the direct run's, and run(out=block) works in place.  The first switch to STAGED
        allocates mixmatrix_staging_bytes(...) of device memory, kept until the bank goes.  Any thread, while runs are in flight;
        scatter() says when to switch."""
        self._chk(self.L.dspfx_mixmatrix_set_staging(self.h, int(mode) & 0xFFFFFFFF))

    @property
    def staging(self) -> int:
        """MIXMATRIX_DIRECT or MIXMATRIX_STAGED: the mode of the next run."""
        v = C.c_uint32(0)
        self._chk(self.L.dspfx_mixmatrix_staging(self.h, C.byref(v)))
        return int(v.value)

    def scatter(self):
        """A seated bank: mixmatrix_scatter of the seating by every call made so far -> (chunks, lines)."""
        if self.seats is None:
            raise DspfxError(-6, "mixmatrix scatter: the bank has no seats")
        return mixmatrix_scatter(self.room_of(), self.seat_of(), self.seats)

    def set_pairs(self, listeners, sources, gains):
        """M[listeners[i]][sources[i]] = gains[i], by CHANNEL number, in order (a later duplicate wins); gains may be one value for
        all pairs.  Each pair must be two channels of one room, or nothing is stored.  Queued like every other store."""
        u32 = C.POINTER(C.c_uint32)
        l, s = _room_ids(listeners), _room_ids(sources)
        g = np.ascontiguousarray(np.broadcast_to(np.asarray(gains, np.float32).reshape(-1), (len(l),)) if np.size(gains) == 1 else gains,
                                 np.float32).reshape(-1)
        if not len(l) == len(s) == len(g):
            raise DspfxError(-1, "listeners, sources and gains are equally long")
        self._chk(self.L.dspfx_mixmatrix_set_pairs(self.h, l.ctypes.data_as(u32), s.ctypes.data_as(u32), g.ctypes.data_as(C.POINTER(C.c_float)), len(l)))

    def run(self, block, n_frames: Optional[int] = None, out=None, stream: int = 0, sources=None):
        """One device block through every room's matrix -> `out`, a device block in the same layout (made when not given).
        `out` may not overlap `block`: every listener reads every source of its room, so there is no in-place form -- except in
        MIXMATRIX_STAGED, where `out` may be `block` itself.
        sources=(list, start, count), device tensors (int32 channel numbers, uint32[G + 1], uint32[G]; Talkers.audible() gives them):
        the SPARSE run (dspfx_mixmatrix_run_sparse): room r adds only the sources named in list[start[r] : start[r] + count[r]],
        in ascending room-local order, and reads no other.  Where every unlisted source carries +-0.0 it is the dense run bit for
        bit.  Entries that are negative, past the channels or of another room are ignored; the list's producer and this run
        share a stream."""
        import torch
        if n_frames is None:
            n_frames = block.numel() // self.channels
        if out is None:
            out = torch.empty(int(n_frames) * self.channels, dtype=torch.float32, device=torch.device("cuda", self.device))
        s = _stream(stream)
        if sources is None:
            self._chk(self.L.dspfx_mixmatrix_run(self.h, _ptr(block), int(n_frames), _ptr(out), s))
            return out
        lst, start, count = sources
        if start.numel() != self.groups + 1 or count.numel() != self.groups or any(t.element_size() != 4 or t.is_floating_point() for t in sources):
            raise DspfxError(-1, "mixmatrix run: sources is (list, start[groups + 1], count[groups]) of 32-bit integers")
        self._chk(self.L.dspfx_mixmatrix_run_sparse(self.h, _ptr(block), int(n_frames), _ptr(out), _ptr(lst), int(lst.numel()), _ptr(start),
                                                    _ptr(count), s))
        return out

    def _lines(self, fn, values, first_channel, count):
        v = np.ascontiguousarray(values, np.float32)
        if v.ndim == 1:
            v = v.reshape(1, -1)
        if v.ndim != 2 or (count is not None and int(count) != v.shape[0]):
            raise DspfxError(-1, "values is [count][n_r]: one line of the room's member count per channel")
        self._chk(fn(self.h, v.ctypes.data_as(C.POINTER(C.c_float)), v.shape[1] & 0xFFFFFFFF, int(first_channel), v.shape[0]))

    def set_rows(self, values, first_channel: int, count: Optional[int] = None):
        """What listeners first_channel .. hear: values[count][n_r], row i = the gains of listener first_channel + i on the n_r
        sources of its room (one row may be given as a vector).  All listeners must be in one room.  Any thread; never waits for a
        run; applies, whole, to the runs submitted after it.  On a seated bank a row is seats[r] values indexed by SEAT (seat_of()
        tells who sits where), the listeners must share a room by the seating so far, and values at empty seats are stored as +0.0."""
        self._lines(self.L.dspfx_mixmatrix_set_rows, values, first_channel, count)

    def set_cols(self, values, first_channel: int, count: Optional[int] = None):
        """How loud sources first_channel .. are: values[count][n_r], row i = the gain of source first_channel + i for each of the
        n_r listeners of its room (a source fader; zeros mute someone for everybody).  Rules as set_rows."""
        self._lines(self.L.dspfx_mixmatrix_set_cols, values, first_channel, count)

    def fill(self, room: Optional[int] = None, preset: int = MIXMATRIX_MIX_MINUS):
        """Room `room` (None: every room) back to a preset: MIXMATRIX_MIX_MINUS (1.0 off the diagonal) or MIXMATRIX_ZERO."""
        self._chk(self.L.dspfx_mixmatrix_fill(self.h, -1 if room is None else int(room), int(preset) & 0xFFFFFFFF))

    def reset(self):
        """The fresh state: mix-minus in every room (queued like a store)."""
        self._chk(self.L.dspfx_mixmatrix_reset(self.h))
