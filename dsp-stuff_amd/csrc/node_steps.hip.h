// node_steps.hip.h -- one sample of the small-state chain nodes that the per-channel banks share (filters, racks, strips, talkers,
// dynamics _kernels.hip), each formula once: scalars in, scalars out.  The loops over rows and channels, the selects and the state
// updates are each bank's own.  Device only, hipcc only.  Not for chain_kernels.hip.h or graph_kernel.hip.h: their text goes to
// hiprtc (kernel_headers.inc), and the engine's apply_node keeps its own.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// a where the mask is all ones, b where it is zero: one v_bfi_b32.  Not `on ? a : b`, which the compiler turns into a divergent
// branch around the arithmetic that makes a -- one branch per frame and channel
__device__ __forceinline__ float pick(uint32_t mask, float a, float b) {
    return __builtin_bit_cast(float, (__builtin_bit_cast(uint32_t, a) & mask) | (__builtin_bit_cast(uint32_t, b) & ~mask));
}

// envelope.rs:34-52 (Detector::next over full_wave): the new envelope from the last one l and the sample x; ga, gr are the attack
// and release gains.  Nothing is contracted
__device__ __forceinline__ float envelope_step(float x, float l, float ga, float gr) {
    const float d = x < 0.0f ? -x : x;
    const float gain = l < d ? ga : gr;
    return __fadd_rn(d, __fmul_rn(__fadd_rn(l, -d), gain));
}

// low_pass.rs:36-39, high_pass.rs:36-39: the new z = x * (1 - r) + r * z from the last one l.  LowPass puts z out, HighPass x - z
__device__ __forceinline__ float one_pole_step(float x, float l, float r, float one_minus_r) {
    return __fadd_rn(__fmul_rn(x, one_minus_r), __fmul_rn(r, l));
}

// biquad.rs:87 -> DirectForm1::run: the plain expression left to right, which -ffp-contract=off leaves as it stands
__device__ __forceinline__ float biquad_step(float x, float a1, float a2, float b0, float b1, float b2, float x1, float x2, float y1, float y2) {
    return b0 * x + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2;
}

}  // namespace
