// pcm_kernels.hip -- device sample formats <-> the engine's f32 at the process boundary (dspfx_process_pcm,
// dspfx_process_host_pcm).  Two streaming kernel families over a 2-D window (rows x a column range, with a row pitch),
// templated on the format and the device channel count:
//   widen   PCM -> f32   the reference's input side, do_read_1 / do_read_2 (dsp-stuff/src/devices.rs:227-260)
//   narrow  f32 -> PCM   its output side, do_write_1 / do_write_2 (devices.rs:394-498)
// Each lane moves 16 bytes of PCM with one vector load or store (and the matching 8 / 16 / 32 bytes of f32); a row whose
// start is not on a vector boundary, and the last < V elements of a row, go element by element.
#include "pcm_kernels.h"
#include "pcm_rules.h"

#include <algorithm>

namespace dspfx {
namespace {

// (the conversion rules to_f32 / from_f32: pcm_rules.h)
// V elements of f32 at p (p is V * 4 bytes aligned): float4 pieces, or one float2
template <int V>
__device__ __forceinline__ void load_f(const float *p, float (&v)[V]) {
    if constexpr (V % 4 == 0) {
#pragma unroll
        for (int k = 0; k < V / 4; ++k) {
            const float4 q = reinterpret_cast<const float4 *>(p)[k];
            v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
        }
    } else {
        const float2 q = *reinterpret_cast<const float2 *>(p);
        v[0] = q.x; v[1] = q.y;
    }
}
template <int V>
__device__ __forceinline__ void store_f(float *p, const float (&v)[V]) {
    if constexpr (V % 4 == 0) {
#pragma unroll
        for (int k = 0; k < V / 4; ++k)
            reinterpret_cast<float4 *>(p)[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    } else {
        *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[1]);
    }
}

// Per row: elements [0, head) one by one up to the first vector boundary, then nv vectors of V, then the rest one by one.
// Lane t takes vector t and (t < head + rest) one scalar element.  VEC = false (a base pointer off 16 bytes): all scalar.
struct RowSplit {
    uint32_t head, nv, done, nscalar;
};
template <int V, bool VEC>
__device__ __forceinline__ RowSplit split_row(size_t e0, uint32_t cols) {
    RowSplit r;
    if (VEC) {
        r.head = (uint32_t)((V - e0 % V) % V);
        if (r.head > cols) r.head = cols;
        r.nv = (cols - r.head) / V;
    } else {
        r.head = 0;
        r.nv = 0;
    }
    r.done = r.head + r.nv * V;
    r.nscalar = r.head + (cols - r.done);
    return r;
}

constexpr int PCM_WG = 256;

template <int FMT, int CH, bool VEC>
__global__ __launch_bounds__(PCM_WG) void pcm_widen_kernel(const typename PcmType<FMT>::T *__restrict__ src,
                                                           float *__restrict__ dst, uint32_t rows, uint32_t cols,
                                                           size_t pitch, size_t c0) {
    using T = typename PcmType<FMT>::T;
    constexpr int V = 16 / (int)(sizeof(T) * CH);
    const uint32_t t = blockIdx.x * PCM_WG + threadIdx.x;
    for (uint32_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const size_t e0 = (size_t)r * pitch + c0;
        const RowSplit sp = split_row<V, VEC>(e0, cols);
        if (t < sp.nv) {
            const size_t e = e0 + sp.head + (size_t)t * V;
            const uint4 raw = *reinterpret_cast<const uint4 *>(src + e * CH);
            T s[V * CH];
            __builtin_memcpy(s, &raw, sizeof raw);
            float v[V];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                if constexpr (CH == 2) v[k] = to_f32<FMT>(s[2 * k]) + to_f32<FMT>(s[2 * k + 1]);
                else v[k] = to_f32<FMT>(s[k]);
            }
            store_f<V>(dst + e, v);
        }
        if (t < sp.nscalar) {
            const size_t e = e0 + (t < sp.head ? t : sp.done + (t - sp.head));
            const T *p = src + e * CH;
            if constexpr (CH == 2) dst[e] = to_f32<FMT>(p[0]) + to_f32<FMT>(p[1]);
            else dst[e] = to_f32<FMT>(p[0]);
        }
    }
}

template <int FMT, int CH, bool VEC>
__global__ __launch_bounds__(PCM_WG) void pcm_narrow_kernel(const float *__restrict__ src,
                                                            typename PcmType<FMT>::T *__restrict__ dst, uint32_t rows,
                                                            uint32_t cols, size_t pitch, size_t c0) {
    using T = typename PcmType<FMT>::T;
    constexpr int V = 16 / (int)(sizeof(T) * CH);
    const uint32_t t = blockIdx.x * PCM_WG + threadIdx.x;
    for (uint32_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const size_t e0 = (size_t)r * pitch + c0;
        const RowSplit sp = split_row<V, VEC>(e0, cols);
        if (t < sp.nv) {
            const size_t e = e0 + sp.head + (size_t)t * V;
            float v[V];
            load_f<V>(src + e, v);
            T s[V * CH];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const T y = from_f32<FMT>(v[k]);
                s[CH * k] = y;
                if constexpr (CH == 2) s[2 * k + 1] = y;
            }
            uint4 raw;
            __builtin_memcpy(&raw, s, sizeof raw);
            *reinterpret_cast<uint4 *>(dst + e * CH) = raw;
        }
        if (t < sp.nscalar) {
            const size_t e = e0 + (t < sp.head ? t : sp.done + (t - sp.head));
            const T y = from_f32<FMT>(src[e]);
            dst[e * CH] = y;
            if constexpr (CH == 2) dst[e * CH + 1] = y;
        }
    }
}

inline dim3 pcm_grid(uint32_t rows, uint32_t cols, int v, bool vec) {
    // lanes per row: max(vectors, scalar elements) <= cols / V + 2V (vector form), cols (scalar form)
    const size_t lanes = vec ? (size_t)cols / v + 2 * (size_t)v : (size_t)cols;
    return dim3((unsigned)((lanes + PCM_WG - 1) / PCM_WG), std::min<uint32_t>(rows, 65535u));
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

template <int FMT, int CH>
hipError_t widen_as(const void *src, float *dst, uint32_t rows, uint32_t cols, size_t pitch, size_t c0, hipStream_t s) {
    using T = typename PcmType<FMT>::T;
    constexpr int V = 16 / (int)(sizeof(T) * CH);
    const bool vec = aligned16(src) && aligned16(dst);
    const dim3 g = pcm_grid(rows, cols, V, vec);
    if (vec) hipLaunchKernelGGL((pcm_widen_kernel<FMT, CH, true>), g, dim3(PCM_WG), 0, s, (const T *)src, dst, rows, cols, pitch, c0);
    else hipLaunchKernelGGL((pcm_widen_kernel<FMT, CH, false>), g, dim3(PCM_WG), 0, s, (const T *)src, dst, rows, cols, pitch, c0);
    return hipGetLastError();
}

template <int FMT, int CH>
hipError_t narrow_as(const float *src, void *dst, uint32_t rows, uint32_t cols, size_t pitch, size_t c0, hipStream_t s) {
    using T = typename PcmType<FMT>::T;
    constexpr int V = 16 / (int)(sizeof(T) * CH);
    const bool vec = aligned16(src) && aligned16(dst);
    const dim3 g = pcm_grid(rows, cols, V, vec);
    if (vec) hipLaunchKernelGGL((pcm_narrow_kernel<FMT, CH, true>), g, dim3(PCM_WG), 0, s, src, (T *)dst, rows, cols, pitch, c0);
    else hipLaunchKernelGGL((pcm_narrow_kernel<FMT, CH, false>), g, dim3(PCM_WG), 0, s, src, (T *)dst, rows, cols, pitch, c0);
    return hipGetLastError();
}

template <int CH>
hipError_t widen_ch(int32_t fmt, const void *src, float *dst, uint32_t rows, uint32_t cols, size_t pitch, size_t c0, hipStream_t s) {
    switch (fmt) {
    case DSPFX_SAMPLE_F32: return widen_as<DSPFX_SAMPLE_F32, CH>(src, dst, rows, cols, pitch, c0, s);
    case DSPFX_SAMPLE_I16: return widen_as<DSPFX_SAMPLE_I16, CH>(src, dst, rows, cols, pitch, c0, s);
    case DSPFX_SAMPLE_U16: return widen_as<DSPFX_SAMPLE_U16, CH>(src, dst, rows, cols, pitch, c0, s);
    case DSPFX_SAMPLE_I32: return widen_as<DSPFX_SAMPLE_I32, CH>(src, dst, rows, cols, pitch, c0, s);
    default: return hipErrorInvalidValue;
    }
}

template <int CH>
hipError_t narrow_ch(int32_t fmt, const float *src, void *dst, uint32_t rows, uint32_t cols, size_t pitch, size_t c0, hipStream_t s) {
    switch (fmt) {
    case DSPFX_SAMPLE_F32: return narrow_as<DSPFX_SAMPLE_F32, CH>(src, dst, rows, cols, pitch, c0, s);
    case DSPFX_SAMPLE_I16: return narrow_as<DSPFX_SAMPLE_I16, CH>(src, dst, rows, cols, pitch, c0, s);
    case DSPFX_SAMPLE_U16: return narrow_as<DSPFX_SAMPLE_U16, CH>(src, dst, rows, cols, pitch, c0, s);
    case DSPFX_SAMPLE_I32: return narrow_as<DSPFX_SAMPLE_I32, CH>(src, dst, rows, cols, pitch, c0, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_pcm_widen(int32_t fmt, int32_t ch, const void *src, float *dst, uint32_t rows, uint32_t cols,
                            size_t pitch, size_t c0, hipStream_t s) {
    if (rows == 0 || cols == 0) return hipSuccess;
    if (ch == 1) return widen_ch<1>(fmt, src, dst, rows, cols, pitch, c0, s);
    if (ch == 2) return widen_ch<2>(fmt, src, dst, rows, cols, pitch, c0, s);
    return hipErrorInvalidValue;
}

hipError_t launch_pcm_narrow(int32_t fmt, int32_t ch, const float *src, void *dst, uint32_t rows, uint32_t cols,
                             size_t pitch, size_t c0, hipStream_t s) {
    if (rows == 0 || cols == 0) return hipSuccess;
    if (ch == 1) return narrow_ch<1>(fmt, src, dst, rows, cols, pitch, c0, s);
    if (ch == 2) return narrow_ch<2>(fmt, src, dst, rows, cols, pitch, c0, s);
    return hipErrorInvalidValue;
}

}  // namespace dspfx
