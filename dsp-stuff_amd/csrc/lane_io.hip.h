// lane_io.hip.h -- how a lane of the per-channel banks (strips, delays, talkers, dynamics, shapers, gens, blends, filters, firs,
// racks, cancel _kernels.hip) reads and writes the channels it owns for a whole block: CPL adjacent channels in one load and one
// store per frame, the frame loop of a bank with one stream in and one out (each_chunk: shapers and talkers), which
// channels a lane's are (lane_channel), and the host's decision whether CPL may be 4.  Device, and one small host part.  hipcc only.
// What the nodes compute per sample is in node_steps.hip.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// CPL adjacent values at p (aligned to CPL values) in one load / one store; NT: nontemporal.  The four-channel form is what load4
// and store4 of bank_common.hip.h do with vec = 1, on the lane's own address
template <int CPL, typename T>
__device__ __forceinline__ void loadv(const T *p, T (&o)[CPL]) {
    typedef T vec __attribute__((ext_vector_type(CPL)));
    if constexpr (CPL == 1) {
        o[0] = *p;
    } else {
        const vec t = *(const vec *)p;
#pragma unroll
        for (int j = 0; j < CPL; ++j) o[j] = t[j];
    }
}

template <int CPL, bool NT>
__device__ __forceinline__ void storev(float *p, const float (&o)[CPL]) {
    typedef float vec __attribute__((ext_vector_type(CPL)));
    if constexpr (CPL == 1) {
        if (NT) __builtin_nontemporal_store(o[0], p);
        else *p = o[0];
    } else {
        vec t;
#pragma unroll
        for (int j = 0; j < CPL; ++j) t[j] = o[j];
        if (NT) __builtin_nontemporal_store(t, (vec *)p);
        else *(vec *)p = t;
    }
}

// R rows from frame f0 of the lane's channels; `lane` is the lane's element of frame 0 (bank_common's lay(0, c, ..)), a frame
// further is `rs` elements on in either layout (rs = W ? W : N), so no row pays lay()'s division.  The stores are nontemporal
template <int CPL, int R>
__device__ __forceinline__ void load_rows(const float *lane, size_t rs, uint32_t f0, float (&v)[R][CPL]) {
#pragma unroll
    for (int i = 0; i < R; ++i) loadv<CPL>(lane + (size_t)(f0 + i) * rs, v[i]);
}

template <int CPL, int R>
__device__ __forceinline__ void store_rows(float *lane, size_t rs, uint32_t f0, const float (&v)[R][CPL]) {
#pragma unroll
    for (int i = 0; i < R; ++i) storev<CPL, true>(lane + (size_t)(f0 + i) * rs, v[i]);
}

// the frame loop of a lane over a block of nf frames: whole chunks of F rows, the next one's loads issued ahead of this one's
// arithmetic; then the rows left, one at a time.  body(v, f0) works on v in place -- float[F][CPL], or float[1][CPL] for a row left --
// whose first frame is f0; it is a generic lambda marked LANE_BODY, so it is inlined into both loops.  STORE = false: the rows are
// loaded and run and no block is written (lout is not used)
#define LANE_BODY __attribute__((always_inline))
template <int CPL, int F, bool STORE = true, class Body>
__device__ __forceinline__ void each_chunk(const float *lin, float *lout, size_t rs, uint32_t nf, Body &&body) {
    const uint32_t nfull = nf / F;
    float cur[F][CPL], nxt[F][CPL];
    if (nfull) load_rows<CPL, F>(lin, rs, 0, cur);
#pragma unroll 1
    for (uint32_t ch = 0; ch < nfull; ++ch) {
        if (ch + 1 < nfull) load_rows<CPL, F>(lin, rs, (ch + 1) * F, nxt);
        body(cur, ch * F);
        if constexpr (STORE) store_rows<CPL, F>(lout, rs, ch * F, cur);
#pragma unroll
        for (int i = 0; i < F; ++i)
#pragma unroll
            for (int j = 0; j < CPL; ++j) cur[i][j] = nxt[i][j];
    }
#pragma unroll 1
    for (uint32_t f = nfull * F; f < nf; ++f) {
        float one[1][CPL];
        load_rows<CPL, 1>(lin, rs, f, one);
        body(one, f);
        if constexpr (STORE) store_rows<CPL, 1>(lout, rs, f, one);
    }
}

// the lane's first channel c in a launch of `wg` lanes per workgroup; false past N: the lane has none (CPL > 1 only with
// N % 4 == 0, so a lane's channels are all inside or all outside)
template <int CPL>
__device__ __forceinline__ bool lane_channel(uint32_t wg, uint32_t N, uint32_t &c) {
    const uint64_t c64 = ((uint64_t)blockIdx.x * wg + threadIdx.x) * CPL;
    c = (uint32_t)c64;
    return c64 < N;
}

// ---- host ------------------------------------------------------------------------------------------------------------
// the workgroups of `wg` lanes that cover N channels at `cpl` channels per lane
inline uint32_t lane_blocks(uint32_t N, uint32_t cpl, uint32_t wg) { return ((N + cpl - 1) / cpl + wg - 1) / wg; }

// vec: a lane may take four channels -- every group of 4 channels from a multiple of 4 is contiguous, 16-byte aligned and inside N
// (the tile divides N).  `ptrs` is the OR of the addresses of the run's blocks; a block that is not given (nullptr) adds nothing
struct LanePlan {
    bool vec;
    uint32_t lanes, blocks;
};

inline LanePlan lane_plan(uint32_t N, uint32_t W, uintptr_t ptrs, uint32_t wg) {
    const bool vec = (W ? W : N) % 4 == 0 && (ptrs & 15u) == 0;
    const uint32_t cpl = vec ? 4 : 1;
    return {vec, (N + cpl - 1) / cpl, lane_blocks(N, cpl, wg)};
}

}  // namespace
