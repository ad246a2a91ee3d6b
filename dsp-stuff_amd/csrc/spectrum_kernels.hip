// spectrum_kernels.hip -- the Spectrogram bank (include/dspfx.h, dspfx_spectrum_*): nodes/spectrogram.rs:225-268 for N channels.
//   slot copy        a pushed block (any frame range of it, either layout) into the 128-frame slots of the window store
//   spectrum_column  one window of every channel: vol[k] = |FFT(window * x)[k]| * gain[k], k in [0, n/2), into the history
// The window store is a ring of n/128 + 1 slots of 128 frames, each slot in the desc's layout for a 128-frame block, so an
// engine can write its output straight into the next slot (dspfx_spectrum_slot).  A window is n/128 consecutive slots and is
// launched with its last frame; the spare slot is the one an engine may already fill while that launch is queued.
//
// spectrum_column, one workgroup of 512 threads per RUN of Q adjacent channels: in both layouts the Q samples of a frame are
// contiguous, so every global read is a whole 4Q-byte segment, and so is every write of a column row.
// A channel's n real samples are ONE complex signal of m = n/2 points, z[j] = x[2j] + i x[2j + 1] (the real-input FFT):
// Z = FFT_m(z); with Zc = conj Z[(m - k) mod m] and w = exp(-2 pi i k / n),
//       X[k] = ((Z[k] + Zc) - i w (Z[k] - Zc)) / 2          k in [0, n/2)
// Every channel is transformed on its own: its rounding error is relative to its own level.  (Packing two CHANNELS into one
// complex FFT costs the same, but each channel then carries the other's rounding error, which fails a quiet channel beside
// a loud one.)  The Q transforms live in ONE LDS buffer A[point][q] (q fastest, as in memory) and are done in place: a pass
// reads all its points into registers, the workgroup meets, then it writes them in Stockham order, so the output is in
// natural order with no second buffer and the run is twice as wide as two buffers would allow.  Radix-4 passes and one
// radix-2 pass when log2 m is odd; twiddles from a table rounded once from f64 (none in the first pass, where they are all 1).
//   n       128   256   512  1024  2048  4096  8192
//   Q       128    64    32    16     8     4     4      channels per workgroup
//   LDS     64 KiB everywhere, 128 KiB at 8192 (one workgroup per CU there, two elsewhere)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/dspfx.h"

namespace {

constexpr uint32_t SLOT = DSPFX_BUF_SIZE;          // frames per slot: one process block
constexpr int ST = 512;                            // threads of spectrum_column
constexpr double RATE = 48000.0;                   // spectrogram.rs:238 sampling_rate

// element (f, c) of a block of nf frames in the desc's layout (dspfx_engine_desc.tile_channels)
__host__ __device__ inline size_t lay(uint32_t f, uint32_t c, uint32_t nf, uint32_t N, uint32_t W) {
    return W ? ((size_t)(c / W) * nf + f) * W + (c % W) : (size_t)f * N + c;
}

// ---- slot copy: `rows` rows of `len` elements, row r at src + r * spitch / dst + r * dpitch (units of T) -------------
template <typename T>
__global__ void spectrum_copy(const T *__restrict__ src, T *__restrict__ dst, size_t rows, size_t len, size_t spitch,
                              size_t dpitch) {
    const size_t total = rows * len;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t r = e / len, k = e - r * len;
        dst[r * dpitch + k] = src[r * spitch + k];
    }
}

hipError_t launch_copy(const float *src, float *dst, size_t rows, size_t len, size_t spitch, size_t dpitch, hipStream_t s) {
    const bool v4 = len % 4 == 0 && spitch % 4 == 0 && dpitch % 4 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0;
    const size_t units = rows * (v4 ? len / 4 : len);
    const unsigned blocks = (unsigned)std::min<size_t>((units + 255) / 256, 1u << 20);
    if (v4)
        spectrum_copy<float4><<<blocks, 256, 0, s>>>((const float4 *)src, (float4 *)dst, rows, len / 4, spitch / 4, dpitch / 4);
    else
        spectrum_copy<float><<<blocks, 256, 0, s>>>(src, dst, rows, len, spitch, dpitch);
    return hipGetLastError();
}

// ---- the column -----------------------------------------------------------------------------------------------------
struct ColArgs {
    const float *ring;           // n/128 + 1 slots of 128 x N
    float *col;                  // [n/2] frames x N, the desc's layout
    const float *win;            // [n]
    const float *gain;           // [n/2]
    const float2 *tw;            // [n] exp(-2 pi i t / n)
    uint32_t N, W;
    uint32_t slot0;              // ring slot of the window's first 128 frames
    uint32_t vec;                // every group of 4 channels from a multiple of 4 is contiguous, 16-byte aligned and inside N
};

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// one in-place Stockham pass of radix R over the Q transforms of m = 2^LOGM points in A[point][q]; NS = the product of the
// radices before it; tw is the table of 2m points, so exp(-2 pi i t / m) = tw[2t]
template <int LOGM, int Q, int R, int NS>
__device__ __forceinline__ void fft_pass(float2 *A, const float2 *__restrict__ tw) {
    constexpr int n = 1 << LOGM, NR = n / R, IT = NR * Q / ST;
    static_assert(NR * Q % ST == 0, "every thread does the same number of butterflies");
    float2 v[IT][R];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int b = threadIdx.x + i * ST, q = b % Q, j = b / Q;
#pragma unroll
        for (int r = 0; r < R; ++r) v[i][r] = A[(j + r * NR) * Q + q];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int b = threadIdx.x + i * ST, q = b % Q, j = b / Q;
        const int k = j & (NS - 1);
        float2 *u = v[i];
        if (NS > 1) {
#pragma unroll
            for (int r = 1; r < R; ++r) u[r] = cmul(u[r], tw[2 * (k * r * (n / (NS * R)))]);
        }
        if (R == 2) {
            const float2 a = u[0];
            u[0] = cadd(a, u[1]);
            u[1] = csub(a, u[1]);
        } else {
            const float2 a0 = cadd(u[0], u[2]), a1 = csub(u[0], u[2]), a2 = cadd(u[1], u[3]), a3 = csub(u[1], u[3]);
            const float2 ja3 = make_float2(a3.y, -a3.x);                                   // -i * a3
            u[0] = cadd(a0, a2);
            u[1] = cadd(a1, ja3);
            u[2] = csub(a0, a2);
            u[3] = csub(a1, ja3);
        }
        const int d = (j - k) * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r) A[(d + r * NS) * Q + q] = u[r];
    }
    __syncthreads();
}

template <int LOGM, int Q, int NS>
__device__ __forceinline__ void fft_all(float2 *A, const float2 *__restrict__ tw) {
    constexpr int m = 1 << LOGM;
    if constexpr (NS * 4 <= m) {
        fft_pass<LOGM, Q, 4, NS>(A, tw);
        fft_all<LOGM, Q, NS * 4>(A, tw);
    } else if constexpr (NS * 2 <= m) {
        fft_pass<LOGM, Q, 2, NS>(A, tw);
    }
}

// frame f of 4 channels from c (c a multiple of 4); channels outside N read 0
__device__ __forceinline__ float4 load4(const ColArgs &a, const float *base, uint32_t f, uint32_t c) {
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a.vec) {
        if (c < a.N) v = *(const float4 *)(base + lay(f, c, SLOT, a.N, a.W));
    } else {
        if (c < a.N) v.x = base[lay(f, c, SLOT, a.N, a.W)];
        if (c + 1 < a.N) v.y = base[lay(f, c + 1, SLOT, a.N, a.W)];
        if (c + 2 < a.N) v.z = base[lay(f, c + 2, SLOT, a.N, a.W)];
        if (c + 3 < a.N) v.w = base[lay(f, c + 3, SLOT, a.N, a.W)];
    }
    return v;
}

// |((z + conj zm) - i w (z - conj zm)) / 2|
__device__ __forceinline__ float bin_norm(float2 z, float2 zm, float2 w) {
    const float ar = z.x + zm.x, ai = z.y - zm.y;
    const float2 t = cmul(w, make_float2(z.x - zm.x, z.y + zm.y));
    const float re = ar + t.y, im = ai - t.x;
    return 0.5f * sqrtf(re * re + im * im);
}

template <int LOGN, int Q>
__global__ __launch_bounds__(ST) void spectrum_column(ColArgs a) {
    constexpr int n = 1 << LOGN, m = n / 2, P = m * Q;   // complex points of the workgroup
    static_assert(Q % 4 == 0 && P % (4 * ST) == 0, "whole units of 4 channels per thread");
    __shared__ __attribute__((aligned(16))) float2 A[P];
    float4 *A4 = (float4 *)A;
    const int t = threadIdx.x;
    // consecutive runs on one XCD (workgroups are dealt round-robin over the 8), so the cache lines they share meet in one L2
    uint32_t blk = blockIdx.x;
    if (gridDim.x % 8 == 0) blk = (blk % 8) * (gridDim.x / 8) + blk / 8;
    const uint32_t c0 = blk * Q;
    const uint32_t RING = n / SLOT + 1;
    constexpr int UN = P / 4 / ST;                       // units of 4 channels per thread, in the load and in the store

    // ---- the window: unit u = frames (2j, 2j + 1) of 4 channels = point j of 4 transforms, A4[2u], A4[2u + 1]
    float4 xe[UN], xo[UN];
#pragma unroll
    for (int i = 0; i < UN; ++i) {
        const uint32_t u = t + i * ST, j = u / (Q / 4), c = c0 + 4 * (u % (Q / 4)), f = 2 * j;
        uint32_t slot = a.slot0 + f / SLOT;
        if (slot >= RING) slot -= RING;
        const float *base = a.ring + (size_t)slot * SLOT * a.N;
        xe[i] = load4(a, base, f % SLOT, c);             // 2j and 2j + 1 are in one slot: a slot holds an even number of frames
        xo[i] = load4(a, base, f % SLOT + 1, c);
    }
#pragma unroll
    for (int i = 0; i < UN; ++i) {
        const uint32_t u = t + i * ST, j = u / (Q / 4);
        const float we = a.win[2 * j], wo = a.win[2 * j + 1];
        A4[2 * u] = make_float4(we * xe[i].x, wo * xo[i].x, we * xe[i].y, wo * xo[i].y);
        A4[2 * u + 1] = make_float4(we * xe[i].z, wo * xo[i].z, we * xe[i].w, wo * xo[i].w);
    }
    __syncthreads();

    fft_all<LOGN - 1, Q, 1>(A, a.tw);

    // ---- the column: bins [0, n/2) of 4 channels per unit, times the gain table
#pragma unroll
    for (int i = 0; i < UN; ++i) {
        const uint32_t u = t + i * ST, k = u / (Q / 4), h = u % (Q / 4), c = c0 + 4 * h;
        const uint32_t km = (m - k) & (m - 1);
        const float4 z0 = A4[(k * (Q / 4) + h) * 2], z1 = A4[(k * (Q / 4) + h) * 2 + 1];
        const float4 y0 = A4[(km * (Q / 4) + h) * 2], y1 = A4[(km * (Q / 4) + h) * 2 + 1];
        const float2 w = a.tw[k];
        const float g = a.gain[k];
        float4 o;
        o.x = bin_norm(make_float2(z0.x, z0.y), make_float2(y0.x, y0.y), w) * g;
        o.y = bin_norm(make_float2(z0.z, z0.w), make_float2(y0.z, y0.w), w) * g;
        o.z = bin_norm(make_float2(z1.x, z1.y), make_float2(y1.x, y1.y), w) * g;
        o.w = bin_norm(make_float2(z1.z, z1.w), make_float2(y1.z, y1.w), w) * g;
        if (a.vec) {
            if (c < a.N) *(float4 *)(a.col + lay(k, c, m, a.N, a.W)) = o;
        } else {
            if (c < a.N) a.col[lay(k, c, m, a.N, a.W)] = o.x;
            if (c + 1 < a.N) a.col[lay(k, c + 1, m, a.N, a.W)] = o.y;
            if (c + 2 < a.N) a.col[lay(k, c + 2, m, a.N, a.W)] = o.z;
            if (c + 3 < a.N) a.col[lay(k, c + 3, m, a.N, a.W)] = o.w;
        }
    }
}

template <int LOGN, int Q>
hipError_t launch_column(const ColArgs &a, hipStream_t s) {
    spectrum_column<LOGN, Q><<<(a.N + Q - 1) / Q, ST, 0, s>>>(a);
    return hipGetLastError();
}

bool pow2(uint32_t w) { return w && !(w & (w - 1)); }

// DSPFX_OK for a size the bank takes
int check_size(uint32_t n) {
    if (n < DSPFX_SPECTRUM_MIN_FFT || n > DSPFX_SPECTRUM_MAX_FFT) return DSPFX_ERR_INVALID;
    return pow2(n) ? DSPFX_OK : DSPFX_ERR_UNSUPPORTED;
}

// the default window: symmetric Hann, f64 rounded once to f32; the second half mirrors the first, so it is symmetric bit for bit
void default_window(uint32_t n, float *w) {
    for (uint32_t i = 0; i < n / 2; ++i) {
        const float v = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)i / (double)(n - 1)));
        w[i] = v;
        w[n - 1 - i] = v;
    }
}

}  // namespace

struct dspfx_spectrum {
    dspfx_spectrum_desc desc{};
    std::mutex mu;                              // push / slot / column / reset / destroy are serialised
    uint32_t ring_slots = 0;                    // n/128 + 1
    float *ring = nullptr;                      // ring_slots slots of 128 x N floats
    float *cols = nullptr;                      // `columns` columns of n/2 x N floats
    float *win = nullptr;                       // [n]
    float *gain = nullptr;                      // [n/2]
    float2 *tw = nullptr;                       // [n]
    hipEvent_t ev = nullptr;
    uint64_t frames = 0;                        // frames pushed since create / reset
    std::atomic<int64_t> windows{0};
    hipStream_t last = nullptr;
    bool used = false;
};

namespace {

void release(dspfx_spectrum *p) {
    (void)hipSetDevice(p->desc.device);
    if (p->ring) (void)hipFree(p->ring);
    if (p->cols) (void)hipFree(p->cols);
    if (p->win) (void)hipFree(p->win);
    if (p->gain) (void)hipFree(p->gain);
    if (p->tw) (void)hipFree(p->tw);
    if (p->ev) (void)hipEventDestroy(p->ev);
    delete p;
}

// a call on a stream other than the last one used waits (on the device) for that one
hipError_t order(dspfx_spectrum *p, hipStream_t s) {
    hipError_t err = hipSuccess;
    if (p->used && s != p->last) {
        err = hipEventRecord(p->ev, p->last);
        if (err == hipSuccess) err = hipStreamWaitEvent(s, p->ev, 0);
    }
    p->last = s;
    p->used = true;
    return err;
}

size_t column_elems(const dspfx_spectrum *p) { return (size_t)(p->desc.fft_size / 2) * p->desc.channels; }

// frames [f, f + nf) of `block` (n_frames long, starting at stream frame f0) into the ring; nf stays within one slot
hipError_t copy_in(dspfx_spectrum *p, const float *block, uint32_t n_frames, uint64_t f0, uint64_t f, uint32_t nf, hipStream_t s) {
    const uint32_t N = p->desc.channels, W = p->desc.tile_channels;
    const uint32_t fa = (uint32_t)(f - f0), g0 = (uint32_t)(f % SLOT);
    float *slot = p->ring + (size_t)((f / SLOT) % p->ring_slots) * SLOT * N;
    if (!W) return launch_copy(block + (size_t)fa * N, slot + (size_t)g0 * N, 1, (size_t)nf * N, 0, 0, s);
    return launch_copy(block + (size_t)fa * W, slot + (size_t)g0 * W, N / W, (size_t)nf * W, (size_t)n_frames * W,
                       (size_t)SLOT * W, s);
}

hipError_t column(dspfx_spectrum *p, uint64_t w, hipStream_t s) {
    const uint32_t n = p->desc.fft_size;
    ColArgs a;
    a.ring = p->ring;
    a.col = p->cols + (size_t)(w % p->desc.columns) * column_elems(p);
    a.win = p->win;
    a.gain = p->gain;
    a.tw = p->tw;
    a.N = p->desc.channels;
    a.W = p->desc.tile_channels;
    a.slot0 = (uint32_t)((w * (n / SLOT)) % p->ring_slots);
    a.vec = (a.W ? a.W : a.N) % 4 == 0;        // the tile divides N; hipMalloc and every slot / column offset are 16-byte aligned then
    switch (n) {
    case 128: return launch_column<7, 128>(a, s);
    case 256: return launch_column<8, 64>(a, s);
    case 512: return launch_column<9, 32>(a, s);
    case 1024: return launch_column<10, 16>(a, s);
    case 2048: return launch_column<11, 8>(a, s);
    case 4096: return launch_column<12, 4>(a, s);
    case 8192: return launch_column<13, 4>(a, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace

#define SPEC_HIP(call)                               \
    do {                                             \
        if ((call) != hipSuccess) return DSPFX_ERR_HIP; \
    } while (0)

extern "C" int dspfx_spectrum_plan(uint32_t fft_size, float *window_out, float *bin_hz_out) {
    const int rc = check_size(fft_size);
    if (rc != DSPFX_OK) return rc;
    if (window_out) default_window(fft_size, window_out);
    if (bin_hz_out)
        for (uint32_t k = 0; k < fft_size / 2; ++k) bin_hz_out[k] = (float)((double)k * RATE / (double)fft_size);
    return DSPFX_OK;
}

extern "C" int dspfx_spectrum_create(const dspfx_spectrum_desc *desc, dspfx_spectrum **out) {
    if (!desc || !out) return DSPFX_ERR_INVALID;
    *out = nullptr;
    if (desc->abi_version != DSPFX_ABI_VERSION || desc->channels == 0 || desc->columns == 0) return DSPFX_ERR_INVALID;
    const uint32_t N = desc->channels, W = desc->tile_channels, n = desc->fft_size;
    if (W && (!pow2(W) || N % W)) return DSPFX_ERR_INVALID;
    const int rc = check_size(n);
    if (rc != DSPFX_OK) return rc;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return DSPFX_ERR_NO_DEVICE;
    if (desc->device < 0 || desc->device >= count) return DSPFX_ERR_INVALID;
    if (hipSetDevice(desc->device) != hipSuccess) return DSPFX_ERR_HIP;
    dspfx_spectrum *p = new (std::nothrow) dspfx_spectrum;
    if (!p) return DSPFX_ERR_OOM;
    p->desc = *desc;
    p->desc.window = nullptr;                   // copied below: the caller's tables are not kept
    p->desc.gain = nullptr;
    p->ring_slots = n / SLOT + 1;
    std::vector<float> win(n), gain(n / 2, 1.0f);
    std::vector<float2> tw(n);
    if (desc->window)
        std::memcpy(win.data(), desc->window, n * sizeof(float));
    else
        default_window(n, win.data());
    if (desc->gain) std::memcpy(gain.data(), desc->gain, (n / 2) * sizeof(float));
    for (uint32_t k = 0; k < n; ++k) {
        const double ang = -2.0 * M_PI * k / n;
        tw[k] = make_float2((float)std::cos(ang), (float)std::sin(ang));
    }
    if (hipMalloc((void **)&p->ring, (size_t)p->ring_slots * SLOT * N * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&p->cols, (size_t)desc->columns * column_elems(p) * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&p->win, n * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&p->gain, (n / 2) * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&p->tw, n * sizeof(float2)) != hipSuccess) {
        (void)hipGetLastError();
        release(p);
        return DSPFX_ERR_OOM;
    }
    if (hipMemcpy(p->win, win.data(), n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->gain, gain.data(), (n / 2) * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->tw, tw.data(), n * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess ||
        hipEventCreateWithFlags(&p->ev, hipEventDisableTiming) != hipSuccess) {
        release(p);
        return DSPFX_ERR_HIP;
    }
    *out = p;
    return DSPFX_OK;
}

extern "C" int dspfx_spectrum_destroy(dspfx_spectrum *p) {
    if (!p) return DSPFX_ERR_INVALID;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        (void)hipSetDevice(p->desc.device);
        if (p->used) (void)hipStreamSynchronize(p->last);   // the bank's work is ordered on the last stream it used
    }
    release(p);
    return DSPFX_OK;
}

extern "C" float *dspfx_spectrum_slot(dspfx_spectrum *p) {
    if (!p) return nullptr;
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->frames % SLOT) return nullptr;
    return p->ring + (size_t)((p->frames / SLOT) % p->ring_slots) * SLOT * p->desc.channels;
}

// spectrogram.rs:225-268 per frame position: window w is frames [n w, n (w + 1)) and runs as soon as the last of them is in
extern "C" int dspfx_spectrum_push(dspfx_spectrum *p, const float *block, uint32_t n_frames, void *stream) {
    if (!p || !block || n_frames == 0) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    const uint32_t N = p->desc.channels, n = p->desc.fft_size;
    const float *slot = p->frames % SLOT ? nullptr : p->ring + (size_t)((p->frames / SLOT) % p->ring_slots) * SLOT * N;
    const bool in_place = block == slot;
    if (in_place && n_frames != SLOT) return DSPFX_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    SPEC_HIP(hipSetDevice(p->desc.device));
    SPEC_HIP(order(p, s));
    const uint64_t f0 = p->frames, f1 = f0 + n_frames;
    for (uint64_t f = f0; f < f1;) {
        const uint64_t end = std::min<uint64_t>(f1, (f / SLOT + 1) * SLOT);
        if (!in_place) SPEC_HIP(copy_in(p, block, n_frames, f0, f, (uint32_t)(end - f), s));
        f = end;
        p->frames = f;                   // what has been launched so far: a failure part-way leaves a consistent state
        if (f % n == 0) {                // a window ends on a slot boundary (n is a multiple of 128)
            SPEC_HIP(column(p, f / n - 1, s));
            p->windows.fetch_add(1);
        }
    }
    return DSPFX_OK;
}

extern "C" const float *dspfx_spectrum_column(dspfx_spectrum *p, uint32_t age) {
    if (!p) return nullptr;
    std::lock_guard<std::mutex> lk(p->mu);
    const int64_t done = p->windows.load();
    if (age >= p->desc.columns || (int64_t)age >= done) return nullptr;
    return p->cols + (size_t)((uint64_t)(done - 1 - age) % p->desc.columns) * column_elems(p);
}

extern "C" int dspfx_spectrum_reset(dspfx_spectrum *p) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    p->frames = 0;
    p->windows = 0;
    return DSPFX_OK;
}

extern "C" int64_t dspfx_spectrum_windows(const dspfx_spectrum *p) {
    if (!p) return DSPFX_ERR_INVALID;
    return p->windows.load();
}
