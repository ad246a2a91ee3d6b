// pcm_kernels.h -- launchers of the device-sample-format conversions at the boundary (pcm_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dspfx.h"

namespace dspfx {

// a dspfx_sample_format / device channel count the conversions take (include/dspfx.h: everything else is DSPFX_ERR_INVALID)
inline bool pcm_format_ok(int32_t fmt) { return fmt >= DSPFX_SAMPLE_F32 && fmt <= DSPFX_SAMPLE_I32; }
inline bool pcm_channels_ok(int32_t ch) { return ch == 1 || ch == 2; }
// bytes of one element of the engine's sample layout in that format: one device frame of `ch` samples
inline size_t pcm_elem_bytes(int32_t fmt, int32_t ch) {
    return (size_t)ch * (fmt == DSPFX_SAMPLE_I16 || fmt == DSPFX_SAMPLE_U16 ? 2 : 4);
}

// The window: rows [0, rows) x elements [c0, c0 + cols) of a buffer whose rows are `pitch` elements apart -- element
// (r, c) at r * pitch + c0 + c in both the PCM and the f32 buffer.  A whole block, in either layout, is rows = n_frames,
// cols = pitch = N, c0 = 0: the conversion is elementwise, so the tiled order needs nothing of its own.
// dst[e] = to_f32(src[e])  (2 device channels: to_f32(a) + to_f32(b)).
hipError_t launch_pcm_widen(int32_t fmt, int32_t ch, const void *src, float *dst, uint32_t rows, uint32_t cols,
                            size_t pitch, size_t c0, hipStream_t s);
// dst[e] = from_f32(src[e])  (2 device channels: the same sample in both slots)
hipError_t launch_pcm_narrow(int32_t fmt, int32_t ch, const float *src, void *dst, uint32_t rows, uint32_t cols,
                             size_t pitch, size_t c0, hipStream_t s);

}  // namespace dspfx
