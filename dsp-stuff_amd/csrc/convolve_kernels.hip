// convolve_kernels.hip -- the convolver bank (include/dspfx.h, dspfx_convolve_*): one long impulse response over N channels by
// uniformly partitioned overlap-save, partition = the 128-frame block, P = ceil(T / 128) partitions.  Per block and channel:
//   convolve_forward     the real 256-point FFT of (previous block, this block) into slot `head` of the spectral ring
//   convolve_accumulate  Y[k] = sum_{p<P} H[p][k] * X[head - p][k]: the hot path, one read of the channel's spectral history
//   convolve_inverse     the inverse FFT of Y, its last 128 samples times the divisor into `out`
// A spectrum is 128 complex values: bins 1..127, and element 0 = (DC, Nyquist), both real, which multiplies component-wise.
// The real transform of 256 samples is ONE complex transform of 128 points, z[j] = x[2j] + i x[2j + 1] (as spectrum_kernels.hip):
// with Zc = conj Z[128 - k] and w = exp(-2 pi i k / 256)
//       X[k] = ((Z[k] + Zc) - i w (Z[k] - Zc)) / 2            X[0] = Re Z[0] + Im Z[0], X[128] = Re Z[0] - Im Z[0]
// and back, with Yc = conj Y[128 - k]:
//       2 Z[k] = (Y[k] + Yc) + i conj(w) (Y[k] - Yc)          2 Z[0] = (Y[0] + Y[128]) + i (Y[0] - Y[128])
// z = IFFT_128(Z) is done as conj(FFT_128(conj Z)) / 128; the factors 1/2 and 1/128 are one exact multiplication by 2^-8.
// Ring layout [slot][k][N] complex, so in the accumulation consecutive lanes are consecutive channels and H is wave-uniform;
// the response table is [k][P] complex, read with scalar loads through the constant address space.
// The forward and inverse kernels give a workgroup of 256 threads a RUN of 32 adjacent channels (every global access a whole
// segment in both layouts); the 32 transforms are done in place in one LDS buffer A[point][q]: fft_core.hip.h.
// A bank may hold several responses and an id per channel (dspfx_convolve_response_add / _assign).  With one response nothing
// changes: the same kernels, the same launches.  With more, convolve_accumulate_multi reads the ids: a wave whose channels
// all carry one id takes accumulate_wave exactly as above with that response's table and P; a mixed wave runs it once per
// distinct id with the other lanes masked off; convolve_inverse_multi takes the divisor per channel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/dspfx.h"
#include "bank_common.hip.h"
#include "fft_core.hip.h"

namespace {

constexpr uint32_t L = DSPFX_BUF_SIZE;             // partition = block = 128 frames
constexpr int M = 128;                             // complex points of a spectrum
constexpr int Q = 32;                              // channels per workgroup of the forward / inverse kernels
constexpr int ST = 256;                            // their threads
constexpr int GROUP = 16;                          // partitions per partial sum, and loads in flight per lane
constexpr int AW = 4;                              // waves (= values of k) per workgroup of the accumulation

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(4))) float *TablePtr;   // wave-uniform index: scalar loads

// the 128-point transform of the workgroup's 32 channels, radix 4, 4, 4, 2; tw[t] = exp(-2 pi i t / 256)
__device__ __forceinline__ void fft128(float2 *A, const float2 *__restrict__ tw) { fft_all<7, Q, ST, 1>(A, tw); }

struct FftArgs {
    const float *in;             // forward: the caller's block of nf frames
    float *out;                  // inverse: the caller's block of nf frames
    float *prev;                 // [128][N]: the bank's copy of the previous block, frame-major
    float2 *spec;                // forward: the ring slot [128][N]; inverse: the accumulator [128][N]
    const float2 *tw;            // [256] exp(-2 pi i t / 256)
    uint32_t N, W, nf, f0;       // the block is frames [f0, f0 + 128) of nf
    uint32_t vec;                // every group of 4 channels from a multiple of 4 is contiguous, 16-byte aligned and inside N
    float divisor;
};

// the spectrum values of 4 channels at one k: element (k, c + i) of a [128][N] complex array
__device__ __forceinline__ void load_spec4(const float2 *spec, uint32_t vec, uint32_t k, uint32_t c, uint32_t N, float4 &lo, float4 &hi) {
    lo = hi = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float2 *p = spec + (size_t)k * N + c;
    if (vec) {
        if (c < N) {
            lo = *(const float4 *)p;
            hi = *(const float4 *)(p + 2);
        }
    } else {
        if (c < N) { const float2 t = p[0]; lo.x = t.x; lo.y = t.y; }
        if (c + 1 < N) { const float2 t = p[1]; lo.z = t.x; lo.w = t.y; }
        if (c + 2 < N) { const float2 t = p[2]; hi.x = t.x; hi.y = t.y; }
        if (c + 3 < N) { const float2 t = p[3]; hi.z = t.x; hi.w = t.y; }
    }
}

__device__ __forceinline__ void store_spec4(float2 *spec, uint32_t vec, uint32_t k, uint32_t c, uint32_t N, float4 lo, float4 hi) {
    float2 *p = spec + (size_t)k * N + c;
    if (vec) {
        if (c < N) {
            *(float4 *)p = lo;
            *(float4 *)(p + 2) = hi;
        }
    } else {
        if (c < N) p[0] = make_float2(lo.x, lo.y);
        if (c + 1 < N) p[1] = make_float2(lo.z, lo.w);
        if (c + 2 < N) p[2] = make_float2(hi.x, hi.y);
        if (c + 3 < N) p[3] = make_float2(hi.z, hi.w);
    }
}

// X[k] of one channel from Z[k] and Z[(128 - k) & 127]; k = 0 gives the packed (DC, Nyquist).  Not spectrum_kernels.hip's
// bin_norm: here the 0.5 is applied per component, there once after the square root, and the two round differently
__device__ __forceinline__ float2 bin_of(float2 z, float2 zm, float2 w, uint32_t k) {
    if (k == 0) return make_float2(z.x + z.y, z.x - z.y);
    const float ar = z.x + zm.x, ai = z.y - zm.y;
    const float2 t = cmul(w, make_float2(z.x - zm.x, z.y + zm.y));
    return make_float2(0.5f * (ar + t.y), 0.5f * (ai - t.x));
}

// conj(2 Z[k]) of one channel from Y[k] and Y[(128 - k) & 127]; for k = 0 y is the packed (DC, Nyquist)
__device__ __forceinline__ float2 point_of(float2 y, float2 ym, float2 w, uint32_t k) {
    if (k == 0) return make_float2(y.x + y.y, -(y.x - y.y));
    const float er = y.x + ym.x, ei = y.y - ym.y;
    const float2 o = cmul(make_float2(w.x, -w.y), make_float2(y.x - ym.x, y.y + ym.y));
    return make_float2(er - o.y, -(ei + o.x));
}

__global__ __launch_bounds__(ST) void convolve_forward(FftArgs a) {
    __shared__ __attribute__((aligned(16))) float2 A[M * Q];
    float4 *A4 = (float4 *)A;
    const int t = threadIdx.x;
    const uint32_t c0 = blockIdx.x * Q;
    constexpr int UN = M * Q / 4 / ST;                   // units of 4 channels per thread

    // ---- the window: unit u = frames (2j, 2j + 1) of 4 channels = point j of 4 transforms; points 0..63 are the previous block
    float4 xe[UN], xo[UN];
#pragma unroll
    for (int i = 0; i < UN; ++i) {
        const uint32_t u = t + i * ST, j = u / (Q / 4), c = c0 + 4 * (u % (Q / 4));
        if (j < M / 2) {
            xe[i] = load4(a.prev, a.vec, 2 * j, c, L, a.N, 0);
            xo[i] = load4(a.prev, a.vec, 2 * j + 1, c, L, a.N, 0);
        } else {
            xe[i] = load4(a.in, a.vec, a.f0 + 2 * j - L, c, a.nf, a.N, a.W);
            xo[i] = load4(a.in, a.vec, a.f0 + 2 * j - L + 1, c, a.nf, a.N, a.W);
        }
    }
#pragma unroll
    for (int i = 0; i < UN; ++i) {
        const uint32_t u = t + i * ST;
        A4[2 * u] = make_float4(xe[i].x, xo[i].x, xe[i].y, xo[i].y);
        A4[2 * u + 1] = make_float4(xe[i].z, xo[i].z, xe[i].w, xo[i].w);
    }
    __syncthreads();                                     // every read of the previous block is done: this block replaces it
#pragma unroll
    for (int i = 0; i < UN; ++i) {
        const uint32_t u = t + i * ST, j = u / (Q / 4), c = c0 + 4 * (u % (Q / 4));
        if (j >= M / 2) {
            store4<false>(a.prev, xe[i], a.vec, 2 * j - L, c, L, a.N, 0);
            store4<false>(a.prev, xo[i], a.vec, 2 * j - L + 1, c, L, a.N, 0);
        }
    }

    fft128(A, a.tw);

#pragma unroll
    for (int i = 0; i < UN; ++i) {
        const uint32_t u = t + i * ST, k = u / (Q / 4), h = u % (Q / 4), c = c0 + 4 * h;
        const uint32_t km = (M - k) & (M - 1);
        const float4 z0 = A4[(k * (Q / 4) + h) * 2], z1 = A4[(k * (Q / 4) + h) * 2 + 1];
        const float4 y0 = A4[(km * (Q / 4) + h) * 2], y1 = A4[(km * (Q / 4) + h) * 2 + 1];
        const float2 w = a.tw[k];
        const float2 b0 = bin_of(make_float2(z0.x, z0.y), make_float2(y0.x, y0.y), w, k);
        const float2 b1 = bin_of(make_float2(z0.z, z0.w), make_float2(y0.z, y0.w), w, k);
        const float2 b2 = bin_of(make_float2(z1.x, z1.y), make_float2(y1.x, y1.y), w, k);
        const float2 b3 = bin_of(make_float2(z1.z, z1.w), make_float2(y1.z, y1.w), w, k);
        store_spec4(a.spec, a.vec, k, c, a.N, make_float4(b0.x, b0.y, b1.x, b1.y), make_float4(b2.x, b2.y, b3.x, b3.y));
    }
}

// the responses of a bank that holds more than one, as the kernels read them (one device copy per bank)
struct Responses {
    const float2 *table[DSPFX_CONVOLVE_MAX_RESPONSES];   // [128][P] each
    uint32_t P[DSPFX_CONVOLVE_MAX_RESPONSES];
    float divisor[DSPFX_CONVOLVE_MAX_RESPONSES];
};
typedef const __attribute__((address_space(4))) Responses *ResponsesPtr;   // wave-uniform index: scalar loads

// MULTI: the divisor is the one of each channel's response (ids [N], every id below the bank's response count)
template <bool MULTI>
__device__ __forceinline__ void inverse_block(FftArgs a, const uint16_t *ids, const Responses *resp) {
    __shared__ __attribute__((aligned(16))) float2 A[M * Q];
    float4 *A4 = (float4 *)A;
    const int t = threadIdx.x;
    const uint32_t c0 = blockIdx.x * Q;
    constexpr int UN = M * Q / 4 / ST;

#pragma unroll
    for (int i = 0; i < UN; ++i) {
        const uint32_t u = t + i * ST, k = u / (Q / 4), c = c0 + 4 * (u % (Q / 4));
        float4 lo, hi;
        load_spec4(a.spec, a.vec, k, c, a.N, lo, hi);
        A4[2 * u] = lo;
        A4[2 * u + 1] = hi;
    }
    __syncthreads();
    // ---- Y -> conj(2 Z), in place: read both partners, meet, write
    float4 p0[UN], p1[UN];
#pragma unroll
    for (int i = 0; i < UN; ++i) {
        const uint32_t u = t + i * ST, k = u / (Q / 4), h = u % (Q / 4);
        const uint32_t km = (M - k) & (M - 1);
        const float4 z0 = A4[2 * u], z1 = A4[2 * u + 1];
        const float4 y0 = A4[(km * (Q / 4) + h) * 2], y1 = A4[(km * (Q / 4) + h) * 2 + 1];
        const float2 w = a.tw[k];
        const float2 b0 = point_of(make_float2(z0.x, z0.y), make_float2(y0.x, y0.y), w, k);
        const float2 b1 = point_of(make_float2(z0.z, z0.w), make_float2(y0.z, y0.w), w, k);
        const float2 b2 = point_of(make_float2(z1.x, z1.y), make_float2(y1.x, y1.y), w, k);
        const float2 b3 = point_of(make_float2(z1.z, z1.w), make_float2(y1.z, y1.w), w, k);
        p0[i] = make_float4(b0.x, b0.y, b1.x, b1.y);
        p1[i] = make_float4(b2.x, b2.y, b3.x, b3.y);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < UN; ++i) {
        const uint32_t u = t + i * ST;
        A4[2 * u] = p0[i];
        A4[2 * u + 1] = p1[i];
    }
    __syncthreads();

    fft128(A, a.tw);

    // ---- the last 128 samples: point j in [64, 128) holds 256 * (y[2j], -y[2j + 1])
    constexpr float SCALE = 1.0f / 256.0f;
#pragma unroll
    for (int i = 0; i < UN / 2; ++i) {
        const uint32_t u = t + i * ST, j = M / 2 + u / (Q / 4), h = u % (Q / 4), c = c0 + 4 * h;
        const float4 z0 = A4[(j * (Q / 4) + h) * 2], z1 = A4[(j * (Q / 4) + h) * 2 + 1];
        float d0, d1, d2, d3;
        if (MULTI) {                                     // channels outside N are not stored
            d0 = c < a.N ? resp->divisor[ids[c]] : 1.0f;
            d1 = c + 1 < a.N ? resp->divisor[ids[c + 1]] : 1.0f;
            d2 = c + 2 < a.N ? resp->divisor[ids[c + 2]] : 1.0f;
            d3 = c + 3 < a.N ? resp->divisor[ids[c + 3]] : 1.0f;
        } else {
            d0 = d1 = d2 = d3 = a.divisor;
        }
        const float4 e = make_float4(z0.x * SCALE * d0, z0.z * SCALE * d1, z1.x * SCALE * d2, z1.z * SCALE * d3);
        const float4 o = make_float4(-z0.y * SCALE * d0, -z0.w * SCALE * d1, -z1.y * SCALE * d2, -z1.w * SCALE * d3);
        store4<true>(a.out, e, a.vec, a.f0 + 2 * j - L, c, a.nf, a.N, a.W);
        store4<true>(a.out, o, a.vec, a.f0 + 2 * j - L + 1, c, a.nf, a.N, a.W);
    }
}

__global__ __launch_bounds__(ST) void convolve_inverse(FftArgs a) { inverse_block<false>(a, nullptr, nullptr); }

__global__ __launch_bounds__(ST) void convolve_inverse_multi(FftArgs a, const uint16_t *ids, const Responses *resp) {
    inverse_block<true>(a, ids, resp);
}

// ---- the accumulation -----------------------------------------------------------------------------------------------
struct AccArgs {
    const float2 *ring;          // [slots][128][N]
    float2 *acc;                 // [128][N]
    const float2 *table;         // [128][P]
    uint32_t N, P, slots, head;  // head = the slot the forward kernel just wrote: partition p reads slot head - p (mod slots)
};

// V = complex values per lane: 2 (adjacent channels c, c + 1, one 16-byte load; N even) or 1 (8-byte loads)
template <int V> struct Lane;
template <> struct Lane<2> {
    typedef f32x4 T;
    static __device__ __forceinline__ T zero() { return T{0.0f, 0.0f, 0.0f, 0.0f}; }
    // bins 1..127: s += h * x
    static __device__ __forceinline__ void mac(T &s, float2 h, T x) {
        s.x = fmaf(-h.y, x.y, fmaf(h.x, x.x, s.x));
        s.y = fmaf(h.y, x.x, fmaf(h.x, x.y, s.y));
        s.z = fmaf(-h.y, x.w, fmaf(h.x, x.z, s.z));
        s.w = fmaf(h.y, x.z, fmaf(h.x, x.w, s.w));
    }
    // element 0: (DC, Nyquist), component-wise
    static __device__ __forceinline__ void mac0(T &s, float2 h, T x) {
        s.x = fmaf(h.x, x.x, s.x);
        s.y = fmaf(h.y, x.y, s.y);
        s.z = fmaf(h.x, x.z, s.z);
        s.w = fmaf(h.y, x.w, s.w);
    }
};
template <> struct Lane<1> {
    typedef f32x2 T;
    static __device__ __forceinline__ T zero() { return T{0.0f, 0.0f}; }
    static __device__ __forceinline__ void mac(T &s, float2 h, T x) {
        s.x = fmaf(-h.y, x.y, fmaf(h.x, x.x, s.x));
        s.y = fmaf(h.y, x.x, fmaf(h.x, x.y, s.y));
    }
    static __device__ __forceinline__ void mac0(T &s, float2 h, T x) {
        s.x = fmaf(h.x, x.x, s.x);
        s.y = fmaf(h.y, x.y, s.y);
    }
};

// One wave = one k and 64 * V adjacent channels.  The order of additions is a function of P alone: partitions in ascending
// order into a partial sum per 16 consecutive partitions (the last group may be short), the partials added in ascending order.
template <int V, bool DC>
__device__ __forceinline__ void accumulate_wave(const AccArgs &a, uint32_t k, uint32_t c) {
    typedef typename Lane<V>::T T;
    const TablePtr h = (TablePtr)a.table + (size_t)k * a.P * 2;
    const size_t slot_stride = (size_t)M * a.N;          // complex values per slot
    const float2 *x0 = a.ring + (size_t)k * a.N + c;
    T total = Lane<V>::zero();
    uint32_t s = a.head;                                 // the slot of partition p
    uint32_t p = 0;
    for (; p + GROUP <= a.P; p += GROUP) {
        T x[GROUP];
#pragma unroll
        for (int j = 0; j < GROUP; ++j) {
            x[j] = __builtin_nontemporal_load((const T *)(x0 + (size_t)s * slot_stride));
            s = s ? s - 1 : a.slots - 1;
        }
        T part = Lane<V>::zero();
#pragma unroll
        for (int j = 0; j < GROUP; ++j) {
            const float2 hv = make_float2(h[2 * (p + j)], h[2 * (p + j) + 1]);
            if (DC) Lane<V>::mac0(part, hv, x[j]);
            else Lane<V>::mac(part, hv, x[j]);
        }
        total += part;
    }
    if (p < a.P) {                                       // the short last group: the same order, fewer terms
        T part = Lane<V>::zero();
        for (; p < a.P; ++p) {
            const T x = __builtin_nontemporal_load((const T *)(x0 + (size_t)s * slot_stride));
            s = s ? s - 1 : a.slots - 1;
            const float2 hv = make_float2(h[2 * p], h[2 * p + 1]);
            if (DC) Lane<V>::mac0(part, hv, x);
            else Lane<V>::mac(part, hv, x);
        }
        total += part;
    }
    *(T *)(a.acc + (size_t)k * a.N + c) = total;
}

// One wave = one k and 64 * V adjacent channels.  The order of additions is a function of P alone: partitions in ascending
// order into a partial sum per 16 consecutive partitions (the last group may be short), the partials added in ascending order.
template <int V>
__global__ __launch_bounds__(64 * AW) void convolve_accumulate(AccArgs a) {
    const uint32_t k = __builtin_amdgcn_readfirstlane(blockIdx.y * AW + threadIdx.x / 64);
    const uint32_t c = (blockIdx.x * 64 + (threadIdx.x & 63)) * V;
    if (c >= a.N) return;                                // V = 2: N is even, so c + 1 < N as well
    if (k == 0) accumulate_wave<V, true>(a, k, c);
    else accumulate_wave<V, false>(a, k, c);
}

// ---- the accumulation of a bank with more than one response --------------------------------------------------------
struct MultiArgs {
    AccArgs a;                   // table and P are not used: they are the response's
    const uint16_t *ids;         // [N]: the response of every channel, every id below the bank's response count
    const Responses *resp;
};

// accumulate_wave for the active lanes with response r (wave-uniform): its table and its own P, so the order of additions of
// a channel is the one of a single-response bank of that response
template <int V, bool DC>
__device__ __forceinline__ void accumulate_as(const MultiArgs &m, uint32_t r, uint32_t k, uint32_t c) {
    const ResponsesPtr rp = (ResponsesPtr)m.resp;
    AccArgs b = m.a;
    b.table = rp->table[r];
    b.P = rp->P[r];
    accumulate_wave<V, DC>(b, k, c);
}

// the lanes of `todo`, one distinct id at a time: the id of the first lane left, the lanes that carry it, the rest masked off
template <int V, bool DC>
__device__ __forceinline__ void accumulate_by_id(const MultiArgs &m, bool todo, uint32_t id, uint32_t k, uint32_t c) {
    for (uint64_t left = __builtin_amdgcn_ballot_w64(todo); left; left = __builtin_amdgcn_ballot_w64(todo)) {
        const uint32_t r = __builtin_amdgcn_readlane(id, __builtin_ctzll(left));
        if (todo && id == r) {                           // in here id IS r; read it back so that it stays a scalar: the compiler
            accumulate_as<V, DC>(m, __builtin_amdgcn_readfirstlane(id), k, c);   // would put the lane's id in its place
            todo = false;
        }
    }
}

// MIXED = false: the host saw that no wave of this launch carries two ids (wave_span), and only the single bank's path is
// compiled in, at the single bank's registers
template <int V, bool DC, bool MIXED>
__device__ __forceinline__ void accumulate_multi(const MultiArgs &m, uint32_t k, uint32_t c) {
    uint32_t i0, i1;                                     // the ids of the lane's channels (V = 1: one channel)
    if (V == 2) {
        const uint32_t w = *(const uint32_t *)(m.ids + c);   // c is even
        i0 = w & 0xFFFFu;
        i1 = w >> 16;
    } else {
        i0 = i1 = m.ids[c];
    }
    const uint32_t r = __builtin_amdgcn_readfirstlane(i0);
    if (!MIXED || __builtin_amdgcn_ballot_w64(i0 != r || i1 != r) == 0) {   // one response for the whole wave: the single bank's path
        accumulate_as<V, DC>(m, r, k, c);
        return;
    }
    accumulate_by_id<V, DC>(m, i0 == i1, i0, k, c);
    if (V == 2) {                                        // a lane whose two channels differ: one channel at a time
        accumulate_by_id<1, DC>(m, i0 != i1, i0, k, c);
        accumulate_by_id<1, DC>(m, i0 != i1, i1, k, c + 1);
    }
}

template <int V, bool MIXED>
__global__ __launch_bounds__(64 * AW) void convolve_accumulate_multi(MultiArgs m) {
    const uint32_t k = __builtin_amdgcn_readfirstlane(blockIdx.y * AW + threadIdx.x / 64);
    const uint32_t c = (blockIdx.x * 64 + (threadIdx.x & 63)) * V;
    if (c >= m.a.N) return;
    if (k == 0) accumulate_multi<V, true, MIXED>(m, k, c);
    else accumulate_multi<V, false, MIXED>(m, k, c);
}

uint32_t partitions_of(uint32_t n_taps) { return (n_taps + L - 1) / L; }

// DSPFX_OK for a response the bank takes
int check_taps(const double *taps_reversed, uint32_t n_taps) {
    if (!taps_reversed || n_taps == 0 || n_taps > DSPFX_CONVOLVE_MAX_TAPS) return DSPFX_ERR_INVALID;
    for (uint32_t i = 0; i < n_taps; ++i)
        if (!std::isfinite(taps_reversed[i])) return DSPFX_ERR_INVALID;
    return DSPFX_OK;
}

// the table [128][P] complex: H[p] = the 256-point transform of taps h[128 p .. 128 p + 127] (zero-padded), in f64 with the
// twiddle of every term looked up by its exact index (k n mod 256), rounded once to f32; element 0 is (DC, Nyquist)
void make_table(const double *taps_reversed, uint32_t n_taps, float *table) {
    const uint32_t P = partitions_of(n_taps);
    double cs[256], sn[256];
    for (int t = 0; t < 256; ++t) {
        cs[t] = std::cos(2.0 * M_PI * t / 256.0);
        sn[t] = -std::sin(2.0 * M_PI * t / 256.0);
    }
    for (int t = 0; t < 256; t += 64) {                  // the axes exactly
        cs[t] = t == 0 ? 1.0 : t == 128 ? -1.0 : 0.0;
        sn[t] = t == 64 ? -1.0 : t == 192 ? 1.0 : 0.0;
    }
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t n = std::min<uint32_t>(L, n_taps - p * L);
        double hp[L];
        for (uint32_t i = 0; i < n; ++i) hp[i] = taps_reversed[n_taps - 1 - (p * L + i)];
        for (uint32_t k = 0; k <= (uint32_t)M; ++k) {
            double re = 0.0, im = 0.0;
            for (uint32_t i = 0; i < n; ++i) {
                re += hp[i] * cs[(k * i) & 255];
                im += hp[i] * sn[(k * i) & 255];
            }
            if (k == 0) table[((size_t)0 * P + p) * 2] = (float)re;
            else if (k == (uint32_t)M) table[((size_t)0 * P + p) * 2 + 1] = (float)re;
            else {
                table[((size_t)k * P + p) * 2] = (float)re;
                table[((size_t)k * P + p) * 2 + 1] = (float)im;
            }
        }
    }
}

}  // namespace

// a response beyond the first: the first lives in the bank's own fields (P, divisor, table; desc.n_taps, desc.mode)
struct Extra {
    float2 *table = nullptr;                    // room for [128][slots]; in use: [128][P]
    uint32_t P = 0;
    float divisor = 1.0f;
};

struct dspfx_convolve : BankCore<dspfx_convolve_desc> {     // mu: run / set_taps / response_* / assign / reset / destroy are serialised
    uint32_t slots = 0;                        // P_max = partitions of max_taps
    uint32_t P = 0;                             // partitions of the response in use
    float divisor = 1.0f;
    float2 *ring = nullptr;                     // [slots][128][N]
    float *prev = nullptr;                      // [128][N]
    float2 *acc = nullptr;                      // [128][N]
    float2 *table = nullptr;                    // room for [128][slots]; in use: [128][P]
    float2 *tw = nullptr;                       // [256]
    uint64_t blocks = 0;                        // blocks run since create / reset
    bool silence = false;                       // the next run clears the history first
    // more than one response (dspfx_convolve_response_add): made by the first add, absent before it
    std::vector<Extra> extra;                   // responses 1, 2, ...
    std::vector<uint16_t> ids_host;             // [N]: the map as the device has it
    uint16_t *ids = nullptr;                    // [N]
    Responses *resp = nullptr;                  // tables, P and divisors as the kernels read them
    bool mixed = false;                         // some wave of the accumulation carries more than one id
};

namespace {

void release(dspfx_convolve *p) {
    release_plain_by(p, [p] {
        free_device({p->ring, p->prev, p->acc, p->table, p->tw, p->ids, p->resp});
        for (Extra &e : p->extra) free_device({e.table});
    });
}

size_t ring_bytes(const dspfx_convolve *p) { return (size_t)p->slots * M * p->desc.channels * sizeof(float2); }
size_t prev_bytes(const dspfx_convolve *p) { return (size_t)L * p->desc.channels * sizeof(float); }

float divisor_of(int mode, uint32_t n_taps) { return mode == DSPFX_FIR_AVERAGE ? 1.0f / (float)n_taps : 1.0f; }

// the channels of one wave of the accumulation
uint32_t wave_span(uint32_t N) { return N % 2 == 0 ? 128 : 64; }

bool any_mixed_wave(const std::vector<uint16_t> &ids) {
    const size_t span = wave_span((uint32_t)ids.size());
    for (size_t c = 0; c < ids.size(); ++c)
        if (ids[c] != ids[c - c % span]) return true;
    return false;
}

uint32_t response_count(const dspfx_convolve *p) { return 1 + (uint32_t)p->extra.size(); }

// a host array to the device behind the runs already submitted (they are ordered on the last stream used); done on return
hipError_t upload(dspfx_convolve *p, void *dst, const void *src, size_t bytes) {
    const hipStream_t s = p->used ? p->last : nullptr;
    const hipError_t err = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
    return err == hipSuccess ? hipStreamSynchronize(s) : err;
}

// the device's copy of what the kernels read per response, from the host's
hipError_t upload_responses(dspfx_convolve *p) {
    std::vector<Responses> r(1);
    std::memset(r.data(), 0, sizeof(Responses));
    r[0].table[0] = p->table;
    r[0].P[0] = p->P;
    r[0].divisor[0] = p->divisor;
    for (size_t i = 0; i < p->extra.size(); ++i) {
        r[0].table[i + 1] = p->extra[i].table;
        r[0].P[i + 1] = p->extra[i].P;
        r[0].divisor[i + 1] = p->extra[i].divisor;
    }
    return upload(p, p->resp, r.data(), sizeof(Responses));
}

// response `id` of the bank := these taps and this mode (checked by the caller, the lock held); the history stays
int store_response(dspfx_convolve *p, uint32_t id, const double *taps_reversed, uint32_t n_taps, int mode) {
    const uint32_t P = partitions_of(n_taps);
    std::vector<float> table((size_t)M * P * 2);
    make_table(taps_reversed, n_taps, table.data());
    if (hipSetDevice(p->desc.device) != hipSuccess) return DSPFX_ERR_HIP;
    // the runs already submitted read the table in place: they finish first, then it is replaced (a reload is a file load, not
    // a per-block call); the ring holds input spectra, so the history stays
    if (p->used && hipStreamSynchronize(p->last) != hipSuccess) return DSPFX_ERR_HIP;
    float2 *dst = id ? p->extra[id - 1].table : p->table;
    if (hipMemcpy(dst, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return DSPFX_ERR_HIP;
    if (id) {
        p->extra[id - 1].P = P;
        p->extra[id - 1].divisor = divisor_of(mode, n_taps);
    } else {
        p->P = P;
        p->desc.n_taps = n_taps;
        p->desc.mode = mode;
        p->divisor = divisor_of(mode, n_taps);
    }
    if (p->resp && upload_responses(p) != hipSuccess) return DSPFX_ERR_HIP;
    return DSPFX_OK;
}

}  // namespace

extern "C" int dspfx_convolve_plan(const double *taps_reversed, uint32_t n_taps, uint32_t *partitions, float *table_out) {
    const int rc = check_taps(taps_reversed, n_taps);
    if (rc != DSPFX_OK) return rc;
    if (partitions) *partitions = partitions_of(n_taps);
    if (table_out) make_table(taps_reversed, n_taps, table_out);
    return DSPFX_OK;
}

extern "C" int dspfx_convolve_create(const dspfx_convolve_desc *desc, dspfx_convolve **out) {
    uint32_t max_taps = 0;
    const int rc = create_checks_plain(desc, out, [&]() -> int {
        if (desc->mode != DSPFX_FIR_BALANCED && desc->mode != DSPFX_FIR_AVERAGE) return DSPFX_ERR_INVALID;
        const int taps_rc = check_taps(desc->taps_reversed, desc->n_taps);
        if (taps_rc != DSPFX_OK) return taps_rc;
        max_taps = desc->max_taps ? desc->max_taps : desc->n_taps;
        return max_taps < desc->n_taps || max_taps > DSPFX_CONVOLVE_MAX_TAPS ? DSPFX_ERR_INVALID : DSPFX_OK;
    });
    if (rc != DSPFX_OK) return rc;
    const uint32_t N = desc->channels;
    dspfx_convolve *p = new (std::nothrow) dspfx_convolve;
    if (!p) return DSPFX_ERR_OOM;
    p->desc = *desc;
    p->desc.max_taps = max_taps;
    p->desc.taps_reversed = nullptr;            // copied below: the caller's taps are not kept
    p->slots = partitions_of(max_taps);
    p->P = partitions_of(desc->n_taps);
    p->divisor = divisor_of(desc->mode, desc->n_taps);
    std::vector<float> table((size_t)M * p->P * 2);
    make_table(desc->taps_reversed, desc->n_taps, table.data());
    std::vector<float2> tw(256);
    twiddles(256, tw.data());
    tw[0] = make_float2(1.0f, 0.0f);            // the axes exactly: data whose spectrum lies on them goes through bit for bit
    tw[64] = make_float2(0.0f, -1.0f);
    tw[128] = make_float2(-1.0f, 0.0f);
    tw[192] = make_float2(0.0f, 1.0f);           // (this bank's only: its unit-impulse tests are bit-exact; the others are not held to that)
    if (hipMalloc((void **)&p->ring, ring_bytes(p)) != hipSuccess ||
        hipMalloc((void **)&p->prev, prev_bytes(p)) != hipSuccess ||
        hipMalloc((void **)&p->acc, (size_t)M * N * sizeof(float2)) != hipSuccess ||
        hipMalloc((void **)&p->table, (size_t)M * p->slots * sizeof(float2)) != hipSuccess ||
        hipMalloc((void **)&p->tw, 256 * sizeof(float2)) != hipSuccess) {
        (void)hipGetLastError();
        release(p);
        return DSPFX_ERR_OOM;
    }
    if (hipMemset(p->ring, 0, ring_bytes(p)) != hipSuccess || hipMemset(p->prev, 0, prev_bytes(p)) != hipSuccess ||
        hipMemcpy(p->table, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->tw, tw.data(), 256 * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess ||
        hipEventCreateWithFlags(&p->ev, hipEventDisableTiming) != hipSuccess) {
        release(p);
        return DSPFX_ERR_HIP;
    }
    *out = p;
    return DSPFX_OK;
}

extern "C" int dspfx_convolve_destroy(dspfx_convolve *p) { return destroy_bank(p, release); }

extern "C" int dspfx_convolve_reset(dspfx_convolve *p) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    p->blocks = 0;
    p->silence = true;
    return DSPFX_OK;
}

extern "C" int dspfx_convolve_set_taps(dspfx_convolve *p, const double *taps_reversed, uint32_t n_taps, int mode) {
    return dspfx_convolve_response_set(p, 0, taps_reversed, n_taps, mode);
}

extern "C" int dspfx_convolve_response_set(dspfx_convolve *p, uint32_t id, const double *taps_reversed, uint32_t n_taps, int mode) {
    if (!p) return DSPFX_ERR_INVALID;
    if (mode != DSPFX_FIR_BALANCED && mode != DSPFX_FIR_AVERAGE) return DSPFX_ERR_INVALID;
    const int rc = check_taps(taps_reversed, n_taps);
    if (rc != DSPFX_OK) return rc;
    std::lock_guard<std::mutex> lk(p->mu);
    if (n_taps > p->desc.max_taps || id >= response_count(p)) return DSPFX_ERR_INVALID;
    return store_response(p, id, taps_reversed, n_taps, mode);
}

extern "C" int dspfx_convolve_response_add(dspfx_convolve *p, const double *taps_reversed, uint32_t n_taps, int mode,
                                           uint32_t *id_out) {
    if (!p) return DSPFX_ERR_INVALID;
    if (mode != DSPFX_FIR_BALANCED && mode != DSPFX_FIR_AVERAGE) return DSPFX_ERR_INVALID;
    const int rc = check_taps(taps_reversed, n_taps);
    if (rc != DSPFX_OK) return rc;
    std::lock_guard<std::mutex> lk(p->mu);
    if (n_taps > p->desc.max_taps || response_count(p) >= DSPFX_CONVOLVE_MAX_RESPONSES) return DSPFX_ERR_INVALID;
    BANK_HIP(hipSetDevice(p->desc.device));
    const uint32_t N = p->desc.channels;
    if (!p->resp) {                              // the first add: the map (every channel on response 0) and the kernels' view
        uint16_t *ids = nullptr;
        Responses *resp = nullptr;
        if (hipMalloc((void **)&ids, (size_t)N * sizeof(uint16_t)) != hipSuccess ||
            hipMalloc((void **)&resp, sizeof(Responses)) != hipSuccess) {
            (void)hipGetLastError();
            if (ids) (void)hipFree(ids);
            return DSPFX_ERR_OOM;
        }
        if (hipMemset(ids, 0, (size_t)N * sizeof(uint16_t)) != hipSuccess || hipMemset(resp, 0, sizeof(Responses)) != hipSuccess) {
            (void)hipFree(ids);
            (void)hipFree(resp);
            return DSPFX_ERR_HIP;
        }
        p->ids_host.assign(N, 0);
        p->ids = ids;
        p->resp = resp;
    }
    Extra e;
    if (hipMalloc((void **)&e.table, (size_t)M * p->slots * sizeof(float2)) != hipSuccess) {
        (void)hipGetLastError();
        return DSPFX_ERR_OOM;                    // a bank of one response with a map of zeros runs as before
    }
    p->extra.push_back(e);
    const uint32_t id = response_count(p) - 1;
    const int st = store_response(p, id, taps_reversed, n_taps, mode);
    if (st != DSPFX_OK) {
        p->extra.pop_back();
        (void)hipFree(e.table);
        (void)upload_responses(p);
        return st;
    }
    if (id_out) *id_out = id;
    return DSPFX_OK;
}

extern "C" int dspfx_convolve_assign(dspfx_convolve *p, const uint16_t *host_ids, uint64_t first_channel, uint64_t count) {
    if (!p || !host_ids || count == 0) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    const uint64_t N = p->desc.channels;
    if (first_channel >= N || count > N - first_channel) return DSPFX_ERR_INVALID;
    const uint32_t R = response_count(p);
    for (uint64_t i = 0; i < count; ++i)
        if (host_ids[i] >= R) return DSPFX_ERR_INVALID;
    if (!p->ids) return DSPFX_OK;                // one response: every id is 0, which is what a bank without a map runs
    BANK_HIP(hipSetDevice(p->desc.device));
    // in the order of the bank's last stream: behind every run submitted before, ahead of every run submitted after
    BANK_HIP(upload(p, p->ids + first_channel, host_ids, (size_t)count * sizeof(uint16_t)));
    std::copy(host_ids, host_ids + count, p->ids_host.begin() + (size_t)first_channel);
    p->mixed = any_mixed_wave(p->ids_host);
    return DSPFX_OK;
}

extern "C" int dspfx_convolve_response_count(const dspfx_convolve *p) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(const_cast<dspfx_convolve *>(p)->mu);
    return (int)response_count(p);
}

extern "C" int dspfx_convolve_run(dspfx_convolve *p, const float *in, float *out, uint32_t n_frames, void *stream) {
    if (!p || !in || !out || n_frames == 0 || n_frames % L) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    hipStream_t s = (hipStream_t)stream;
    BANK_HIP(hipSetDevice(p->desc.device));
    BANK_HIP(order(p, s));
    if (p->silence) {
        BANK_HIP(hipMemsetAsync(p->ring, 0, ring_bytes(p), s));
        BANK_HIP(hipMemsetAsync(p->prev, 0, prev_bytes(p), s));
        p->silence = false;
    }
    const uint32_t N = p->desc.channels, W = p->desc.tile_channels;
    FftArgs f;
    f.in = in;
    f.out = out;
    f.prev = p->prev;
    f.tw = p->tw;
    f.N = N;
    f.W = W;
    f.nf = n_frames;
    f.vec = (W ? W : N) % 4 == 0;               // the tile divides N; hipMalloc and every row offset are 16-byte aligned then
    f.divisor = p->divisor;
    if (f.vec && ((((uintptr_t)in) | ((uintptr_t)out)) & 15)) f.vec = 0;
    AccArgs a;
    a.ring = p->ring;
    a.acc = p->acc;
    a.table = p->table;
    a.N = N;
    a.P = p->P;
    a.slots = p->slots;
    const unsigned fft_blocks = (N + Q - 1) / Q;
    const bool multi = !p->extra.empty();       // one response: the kernels and launches of a bank that never had more
    for (uint32_t f0 = 0; f0 < n_frames; f0 += L) {
        const uint32_t head = (uint32_t)(p->blocks % p->slots);
        f.f0 = f0;
        f.spec = p->ring + (size_t)head * M * N;
        convolve_forward<<<fft_blocks, ST, 0, s>>>(f);
        BANK_HIP(hipGetLastError());
        p->blocks += 1;                          // the slot is written: a failure further on leaves a consistent history
        a.head = head;
        const dim3 acc_grid(N % 2 == 0 ? (N / 2 + 63) / 64 : (N + 63) / 64, M / AW);
        f.spec = p->acc;
        if (!multi) {
            if (N % 2 == 0) convolve_accumulate<2><<<acc_grid, 64 * AW, 0, s>>>(a);
            else convolve_accumulate<1><<<acc_grid, 64 * AW, 0, s>>>(a);
            BANK_HIP(hipGetLastError());
            convolve_inverse<<<fft_blocks, ST, 0, s>>>(f);
        } else {
            const MultiArgs m{a, p->ids, p->resp};
            if (N % 2 == 0) {
                if (p->mixed) convolve_accumulate_multi<2, true><<<acc_grid, 64 * AW, 0, s>>>(m);
                else convolve_accumulate_multi<2, false><<<acc_grid, 64 * AW, 0, s>>>(m);
            } else {
                if (p->mixed) convolve_accumulate_multi<1, true><<<acc_grid, 64 * AW, 0, s>>>(m);
                else convolve_accumulate_multi<1, false><<<acc_grid, 64 * AW, 0, s>>>(m);
            }
            BANK_HIP(hipGetLastError());
            convolve_inverse_multi<<<fft_blocks, ST, 0, s>>>(f, p->ids, p->resp);
        }
        BANK_HIP(hipGetLastError());
    }
    return DSPFX_OK;
}
