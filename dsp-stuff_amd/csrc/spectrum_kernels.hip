// spectrum_kernels.hip -- the Spectrogram bank (include/dspfx.h, dspfx_spectrum_*): nodes/spectrogram.rs:225-268 for N channels.
//   slot copy        a pushed block (any frame range of it, either layout) into the 128-frame slots of the window store (bank_common.hip.h)
//   spectrum_column  one window of every channel: vol[k] = |FFT(window * x)[k]| * gain[k], k in [0, n/2), into the history
// The window store is a slot ring (slot_ring.hip.h) of n/128 + 1 slots of 128 frames.  A window is n/128 consecutive slots and is
// launched with its last frame; the spare slot is the one an engine may already fill while that launch is queued.
//
// spectrum_column, one workgroup of 512 threads per RUN of Q adjacent channels: in both layouts the Q samples of a frame are
// contiguous, so every global read is a whole 4Q-byte segment, and so is every write of a column row.
// A channel's n real samples are ONE complex signal of m = n/2 points, z[j] = x[2j] + i x[2j + 1] (the real-input FFT):
// Z = FFT_m(z); with Zc = conj Z[(m - k) mod m] and w = exp(-2 pi i k / n),
//       X[k] = ((Z[k] + Zc) - i w (Z[k] - Zc)) / 2          k in [0, n/2)
// Every channel is transformed on its own: its rounding error is relative to its own level, for every finite window whose
// peak window product is a normal float and whose 2 n max|x| is below FLT_MAX (the sums of the transform stay finite, and
// bin_norm takes the magnitude without squaring out of range); a window with a NaN, or an infinity under a window entry of
// 0, gives a column of NaN, any other infinity a column of NaN and +inf.  (Packing two CHANNELS into one
// complex FFT costs the same, but each channel then carries the other's rounding error, which fails a quiet channel beside
// a loud one.)  The Q transforms are done in place in ONE LDS buffer A[point][q]: fft_core.hip.h.
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
#include "bank_common.hip.h"
#include "fft_core.hip.h"
#include "slot_ring.hip.h"

namespace {

constexpr uint32_t SLOT = DSPFX_BUF_SIZE;          // frames per slot: one process block
constexpr int ST = 512;                            // threads of spectrum_column
constexpr double RATE = 48000.0;                   // spectrogram.rs:238 sampling_rate

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

// |((z + conj zm) - i w (z - conj zm)) / 2|.  Not convolve_kernels.hip's bin_of: there the 0.5 is applied per component, here
// once after the square root, and the two round differently.
// re, im hold 2 X[k].  Their squares leave f32's range long before the magnitude does (from 2^64 up and 2^-63 down), so both
// are first scaled by ONE exact power of two, 2^-E with 2^(E-1) <= max(|re|, |im|) < 2^E (the hardware's frexp exponent, which
// counts a subnormal's leading zeros too; ldexpf is exact here): the larger square lies in [1/4, 1), the smaller one can only
// vanish below half an ulp of it, and the root is scaled back by 2^(E-1), the 0.5 folded in -- exact unless the magnitude
// itself overflows (+inf) or is subnormal (rounded once).  Wherever the plain form 0.5f * sqrtf(re * re + im * im) rounds no
// subnormal square the two give the same bits.  Zero arguments give +0.0 (E = 0, nothing divides); an infinity gives +inf
// or, with a NaN beside it, NaN, whatever E is; fmaxf returns the other argument when one is a NaN, and the NaN then enters
// through its own square
__device__ __forceinline__ float bin_norm(float2 z, float2 zm, float2 w) {
    const float ar = z.x + zm.x, ai = z.y - zm.y;
    const float2 t = cmul(w, make_float2(z.x - zm.x, z.y + zm.y));
    const float re = ar + t.y, im = ai - t.x;
    const int ex = __builtin_amdgcn_frexp_expf(fmaxf(fabsf(re), fabsf(im)));
    const float sr = ldexpf(re, -ex), si = ldexpf(im, -ex);
    return ldexpf(sqrtf(sr * sr + si * si), ex - 1);
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
        // 2j and 2j + 1 are in one slot: a slot holds an even number of frames
        xe[i] = load4(base, a.vec, f % SLOT, c, SLOT, a.N, a.W);
        xo[i] = load4(base, a.vec, f % SLOT + 1, c, SLOT, a.N, a.W);
    }
#pragma unroll
    for (int i = 0; i < UN; ++i) {
        const uint32_t u = t + i * ST, j = u / (Q / 4);
        const float we = a.win[2 * j], wo = a.win[2 * j + 1];
        A4[2 * u] = make_float4(we * xe[i].x, wo * xo[i].x, we * xe[i].y, wo * xo[i].y);
        A4[2 * u + 1] = make_float4(we * xe[i].z, wo * xo[i].z, we * xe[i].w, wo * xo[i].w);
    }
    __syncthreads();

    fft_all<LOGN - 1, Q, ST, 1>(A, a.tw);

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
        // not store4<false> (bank_common.hip.h): its scalar tail is a loop over an array, from which the compiler makes other code
        // for this kernel (fewer instructions, other registers); this form keeps the kernel as it was measured
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

struct dspfx_spectrum : BankCore<dspfx_spectrum_desc> {     // mu: push / slot / column / reset / destroy are serialised
    SlotRing ring;                              // n/128 + 1 slots of 128 x N floats
    float *cols = nullptr;                      // `columns` columns of n/2 x N floats
    float *win = nullptr;                       // [n]
    float *gain = nullptr;                      // [n/2]
    float2 *tw = nullptr;                       // [n]
    uint64_t frames = 0;                        // frames pushed since create / reset
    std::atomic<int64_t> windows{0};
};

namespace {

void release(dspfx_spectrum *p) { release_plain(p, {p->ring.base, p->cols, p->win, p->gain, p->tw}); }

size_t column_elems(const dspfx_spectrum *p) { return (size_t)(p->desc.fft_size / 2) * p->desc.channels; }

// one piece of a push through the slot copy kernel
hipError_t copy_in(const SlotPiece &c, hipStream_t s) { return launch_copy(c.src, c.dst, c.rows, c.len, c.src_pitch, c.dst_pitch, s); }

hipError_t column(dspfx_spectrum *p, uint64_t w, hipStream_t s) {
    const uint32_t n = p->desc.fft_size;
    ColArgs a;
    a.ring = p->ring.base;
    a.col = p->cols + (size_t)(w % p->desc.columns) * column_elems(p);
    a.win = p->win;
    a.gain = p->gain;
    a.tw = p->tw;
    a.N = p->desc.channels;
    a.W = p->desc.tile_channels;
    a.slot0 = (uint32_t)((w * (n / SLOT)) % p->ring.slots);
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

extern "C" int dspfx_spectrum_plan(uint32_t fft_size, float *window_out, float *bin_hz_out) {
    const int rc = check_size(fft_size);
    if (rc != DSPFX_OK) return rc;
    if (window_out) default_window(fft_size, window_out);
    if (bin_hz_out)
        for (uint32_t k = 0; k < fft_size / 2; ++k) bin_hz_out[k] = (float)((double)k * RATE / (double)fft_size);
    return DSPFX_OK;
}

extern "C" int dspfx_spectrum_create(const dspfx_spectrum_desc *desc, dspfx_spectrum **out) {
    const int rc = create_checks_plain(desc, out, [desc] { return desc->columns == 0 ? DSPFX_ERR_INVALID : check_size(desc->fft_size); });
    if (rc != DSPFX_OK) return rc;
    const uint32_t N = desc->channels, n = desc->fft_size;
    dspfx_spectrum *p = new (std::nothrow) dspfx_spectrum;
    if (!p) return DSPFX_ERR_OOM;
    p->desc = *desc;
    p->desc.window = nullptr;                   // copied below: the caller's tables are not kept
    p->desc.gain = nullptr;
    p->ring = {nullptr, n / SLOT + 1, SLOT, N, desc->tile_channels};
    std::vector<float> win(n), gain(n / 2, 1.0f);
    std::vector<float2> tw(n);
    if (desc->window)
        std::memcpy(win.data(), desc->window, n * sizeof(float));
    else
        default_window(n, win.data());
    if (desc->gain) std::memcpy(gain.data(), desc->gain, (n / 2) * sizeof(float));
    twiddles(n, tw.data());
    if (hipMalloc((void **)&p->ring.base, (size_t)p->ring.slots * SLOT * N * sizeof(float)) != hipSuccess ||
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

extern "C" int dspfx_spectrum_destroy(dspfx_spectrum *p) { return destroy_bank(p, release); }

extern "C" float *dspfx_spectrum_slot(dspfx_spectrum *p) {
    if (!p) return nullptr;
    std::lock_guard<std::mutex> lk(p->mu);
    return next_slot(p->ring, p->frames);
}

// spectrogram.rs:225-268 per frame position: window w is frames [n w, n (w + 1)) and runs as soon as the last of them is in
extern "C" int dspfx_spectrum_push(dspfx_spectrum *p, const float *block, uint32_t n_frames, void *stream) {
    if (!p || !block || n_frames == 0) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    const uint32_t n = p->desc.fft_size;
    const bool in_place = block == next_slot(p->ring, p->frames);
    if (in_place && n_frames != SLOT) return DSPFX_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    return push_pieces(p, p->ring, p->frames, n_frames, s, [&](uint64_t f, uint32_t fa, uint32_t nf) -> int {
        if (!in_place) BANK_HIP(copy_in(piece_of(p->ring, block, n_frames, fa, f, nf), s));
        p->frames = f + nf;              // the piece is in, whatever becomes of its window
        if (p->frames % n == 0) {        // a window ends on a slot boundary (n is a multiple of 128)
            BANK_HIP(column(p, p->frames / n - 1, s));
            p->windows.fetch_add(1);
        }
        return DSPFX_OK;
    });
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
