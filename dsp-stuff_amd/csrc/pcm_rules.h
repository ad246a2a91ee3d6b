// pcm_rules.h -- the device sample format rules (dspfx_sample_format <-> the engine's f32), stated ONCE for every kernel that
// reads or writes a device format: pcm_kernels.hip (widen / narrow) and resample_kernels.hip (the resampler's store).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dspfx.h"

namespace dspfx {
namespace {

template <int FMT> struct PcmType;
template <> struct PcmType<DSPFX_SAMPLE_F32> { using T = float; };
template <> struct PcmType<DSPFX_SAMPLE_I16> { using T = int16_t; };
template <> struct PcmType<DSPFX_SAMPLE_U16> { using T = uint16_t; };
template <> struct PcmType<DSPFX_SAMPLE_I32> { using T = int32_t; };

// ---- the conversion rules: ONE function per direction -------------------------------------------------------------
// dasp_sample 0.11.0 (the reference's Cargo.lock:1267-1269), as called by devices.rs:235, 253 (to f32) and 424, 432, 477,
// 488 (from f32).  Restated AS RECALLED -- the crate is not vendored -- so a correction lands here and nowhere else:
//   I16 -> f32   s / 32768
//   U16 -> f32   through i16: (s - 32768) / 32768
//   I32 -> f32   (f32)s / 2^31: one rounding (to nearest even) in the int -> float conversion, the division is exact
//   f32 -> I16   Rust `(x * 32768.0) as i16`: truncated toward zero, saturated to [-32768, 32767], NaN -> 0
//   f32 -> U16   the i16 result + 32768 (bit pattern ^ 0x8000): NaN -> 32768
//   f32 -> I32   `(x * 2147483648.0) as i32`: truncated, saturated, NaN -> 0
// The products by powers of two are exact in f32 (or overflow to +-inf, which saturates).  C++'s float -> int conversion is
// undefined out of range, so the clamps and the NaN case are written out.
template <int FMT>
__device__ __forceinline__ float to_f32(typename PcmType<FMT>::T s) {
    if constexpr (FMT == DSPFX_SAMPLE_F32) return s;
    else if constexpr (FMT == DSPFX_SAMPLE_I16) return (float)s / 32768.0f;
    else if constexpr (FMT == DSPFX_SAMPLE_U16) return (float)((int32_t)s - 32768) / 32768.0f;
    else return (float)s / 2147483648.0f;
}

template <int FMT>
__device__ __forceinline__ typename PcmType<FMT>::T from_f32(float x) {
    if constexpr (FMT == DSPFX_SAMPLE_F32) {
        return x;
    } else if constexpr (FMT == DSPFX_SAMPLE_I32) {
        const float y = x * 2147483648.0f;
        if (y != y) return 0;
        if (y >= 2147483648.0f) return 2147483647;
        if (y <= -2147483648.0f) return (int32_t)(-2147483647 - 1);
        return (int32_t)y;
    } else {
        const float y = x * 32768.0f;
        int32_t v;
        if (y != y) v = 0;
        else if (y >= 32767.0f) v = 32767;
        else if (y <= -32768.0f) v = -32768;
        else v = (int32_t)y;
        if constexpr (FMT == DSPFX_SAMPLE_U16) return (uint16_t)(v + 32768);
        else return (int16_t)v;
    }
}

}  // namespace
}  // namespace dspfx
