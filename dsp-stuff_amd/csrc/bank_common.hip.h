// bank_common.hip.h -- the stateless helpers the banks share (pitch, resample, spectrum, mixgroups, convolve _kernels.hip):
// the desc's layout, 4-channel loads and stores in it, the slot copy, and small host helpers.  Host and device, hipcc only.
// The FFT is in fft_core.hip.h.  A bank's struct, ring and create / destroy / reset are its own.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/dspfx.h"

// `call` failed: the extern "C" function around it returns DSPFX_ERR_HIP
#define BANK_HIP(call)                                  \
    do {                                                \
        if ((call) != hipSuccess) return DSPFX_ERR_HIP; \
    } while (0)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// element (f, c) of a block of nf frames in the desc's layout (dspfx_engine_desc.tile_channels)
__host__ __device__ inline size_t lay(uint32_t f, uint32_t c, uint32_t nf, uint32_t N, uint32_t W) {
    return W ? ((size_t)(c / W) * nf + f) * W + (c % W) : (size_t)f * N + c;
}

// frame f of 4 channels from c (c a multiple of 4) of a block at `base`; channels outside N read 0.  vec, which the host
// establishes: every group of 4 channels from a multiple of 4 is contiguous, 16-byte aligned and inside N
__device__ __forceinline__ float4 load4(const float *base, uint32_t vec, uint32_t f, uint32_t c, uint32_t nf, uint32_t N, uint32_t W) {
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (vec) {
        if (c < N) v = *(const float4 *)(base + lay(f, c, nf, N, W));
    } else {
        if (c < N) v.x = base[lay(f, c, nf, N, W)];
        if (c + 1 < N) v.y = base[lay(f, c + 1, nf, N, W)];
        if (c + 2 < N) v.z = base[lay(f, c + 2, nf, N, W)];
        if (c + 3 < N) v.w = base[lay(f, c + 3, nf, N, W)];
    }
    return v;
}

// ... and the store; channels outside N are not written.  NT: nontemporal
template <bool NT>
__device__ __forceinline__ void store4(float *base, float4 v, uint32_t vec, uint32_t f, uint32_t c, uint32_t nf, uint32_t N, uint32_t W) {
    if (vec) {
        if (c < N) {
            f32x4 *p = (f32x4 *)(base + lay(f, c, nf, N, W));
            const f32x4 t = {v.x, v.y, v.z, v.w};
            if (NT) __builtin_nontemporal_store(t, p);
            else *p = t;
        }
    } else {
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
            if (c + i < N) {
                float *p = base + lay(f, c + i, nf, N, W);
                if (NT) __builtin_nontemporal_store(e[i], p);
                else *p = e[i];
            }
    }
}

// ---- slot copy: `rows` rows of `len` elements, row r at src + r * spitch / dst + r * dpitch (units of T) -------------
template <typename T>
__global__ void slot_copy(const T *__restrict__ src, T *__restrict__ dst, size_t rows, size_t len, size_t spitch,
                          size_t dpitch) {
    const size_t total = rows * len;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t r = e / len, k = e - r * len;
        dst[r * dpitch + k] = src[r * spitch + k];
    }
}

// (a template only so that a bank that never copies has no copy kernel in its code object)
template <class = void>
hipError_t launch_copy(const float *src, float *dst, size_t rows, size_t len, size_t spitch, size_t dpitch, hipStream_t s) {
    const bool v4 = len % 4 == 0 && spitch % 4 == 0 && dpitch % 4 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0;
    const size_t units = rows * (v4 ? len / 4 : len);
    const unsigned blocks = (unsigned)std::min<size_t>((units + 255) / 256, 1u << 20);
    if (v4)
        slot_copy<float4><<<blocks, 256, 0, s>>>((const float4 *)src, (float4 *)dst, rows, len / 4, spitch / 4, dpitch / 4);
    else
        slot_copy<float><<<blocks, 256, 0, s>>>(src, dst, rows, len, spitch, dpitch);
    return hipGetLastError();
}

// ---- host helpers ---------------------------------------------------------------------------------------------------
bool pow2(uint32_t w) { return w && !(w & (w - 1)); }

// out[t] = exp(-2 pi i t / n), t in [0, n): f64, rounded once to f32
void twiddles(uint32_t n, float2 *out) {
    for (uint32_t t = 0; t < n; ++t) {
        const double ang = -2.0 * M_PI * t / n;
        out[t] = make_float2((float)std::cos(ang), (float)std::sin(ang));
    }
}

// a call on a stream other than the last one the bank used waits (on the device) for that one; Bank has ev, last, used
template <class Bank>
hipError_t order(Bank *p, hipStream_t s) {
    hipError_t err = hipSuccess;
    if (p->used && s != p->last) {
        err = hipEventRecord(p->ev, p->last);
        if (err == hipSuccess) err = hipStreamWaitEvent(s, p->ev, 0);
    }
    p->last = s;
    p->used = true;
    return err;
}

}  // namespace
