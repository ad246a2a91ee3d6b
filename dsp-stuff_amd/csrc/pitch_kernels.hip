// pitch_kernels.hip -- the Pitch Detector bank (include/dspfx.h, dspfx_pitch_*): nodes/pitch.rs:120-146 for N channels.
//   slot copy     a pushed block (any frame range of it, either layout) into the 128-frame slots of the window store (bank_common.hip.h)
//   pitch_detect  one window of every channel: McLeod pitch and clarity, 8 bytes of result per channel that has one
//   pitch_read    the held results into the caller's freq[N] / clarity[N]
// The window store is a slot ring (slot_ring.hip.h) of 9 slots of 128 frames.  A window is 8 consecutive slots; the ninth is the
// one being filled while the window before it has not been detected yet (it falls due only with its next frame).
//
// pitch_detect, one workgroup of 256 threads per PAIR of channels (c0, c0 + 1): the pair is one complex signal
// z = x0 + i x1, zero-padded to 2048, each channel first scaled by its own power of two (max |x| into [2, 4), exact) and a
// non-finite channel replaced by zeros, so that neither channel's level or poison reaches the other through the shared
// transforms (tests/test_pitch_pairs_gpu.py).  Z = FFT(z); X0 = (Z + conj Z(-k)) / 2, X1 = (Z - conj Z(-k)) / 2i;
// IFFT(|X0|^2 + i |X1|^2) = r_lin0 + i r_lin1, the two linear autocorrelations, exact for every lag < 1024 (2048 >= 2 * 1024 - 1).
// The crate's FFT is 1536 long, so its lags alias: r(tau) = r_lin(tau) + r_lin(1536 - tau) for tau > 512, added here.
// The FFTs are radix-4 (x5) + radix-2 Stockham passes between two LDS buffers, twiddles from a table rounded once from f64.
// (Not fft_core.hip.h's transform: that one is in place over a run of channels, forward only; this one is one transform per
// workgroup between two buffers, forward and inverse.  Only cmul / cadd / csub are shared.)
// m(tau) comes from prefix sums of x^2 (no running subtraction), then n, then the peak pick as six LDS reductions per
// channel: lobe end, largest key maximum M, first tau >= pick * M, end of its run, the run's maximum, its first tau.
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
constexpr uint32_t WIN = DSPFX_PITCH_WINDOW;       // McLeodDetector::new(1024, 512): size
constexpr uint32_t PAD = 512;                      //   padding: the crate's FFT is 1536 long
constexpr uint32_t SLOTS_PER_WIN = WIN / SLOT;
constexpr uint32_t RING = SLOTS_PER_WIN + 1;
constexpr int FFT_N = 2048;
constexpr int DT = 256;                            // threads of pitch_detect
constexpr int CHUNK = WIN / DT;                    // frames each thread loads (both channels)
constexpr int TPC = DT / 2;                        // threads per channel in the peak pick
constexpr int PER = WIN / TPC;                     // lags each of them holds
constexpr float RATE = 48000.0f;                   // pitch.rs:134 get_pitch(view, 48_000, ...)

// ---- detection ---------------------------------------------------------------------------------------------------------
struct DetArgs {
    const float *ring;
    float2 *res;                 // [N] (frequency, clarity), written only where the window gives a result
    const float2 *tw;            // [FFT_N] exp(-2 pi i t / FFT_N)
    uint32_t N, W;
    uint32_t slot0;              // ring slot of the window's first 128 frames
    float P, C, K;               // power_thresh, clarity_thresh, pick_thresh
};

// one ping-pong Stockham pass of radix R over FFT_N points, src -> dst, Ns = the product of the radices before it
template <int R, bool INV>
__device__ __forceinline__ void fft_pass(const float2 *src, float2 *dst, int Ns, const float2 *__restrict__ tw) {
    constexpr int NR = FFT_N / R;
    for (int j = threadIdx.x; j < NR; j += DT) {
        const int k = j & (Ns - 1);
        float2 v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = src[j + r * NR];
#pragma unroll
        for (int r = 1; r < R; ++r) {
            float2 w = tw[k * r * (FFT_N / (Ns * R))];
            if (INV) w.y = -w.y;
            v[r] = cmul(v[r], w);
        }
        if (R == 2) {
            const float2 a = v[0];
            v[0] = cadd(a, v[1]);
            v[1] = csub(a, v[1]);
        } else {
            const float2 a0 = cadd(v[0], v[2]), a1 = csub(v[0], v[2]), a2 = cadd(v[1], v[3]), a3 = csub(v[1], v[3]);
            const float2 ja3 = INV ? make_float2(-a3.y, a3.x) : make_float2(a3.y, -a3.x);   // +-i * a3
            v[0] = cadd(a0, a2);
            v[1] = cadd(a1, ja3);
            v[2] = csub(a0, a2);
            v[3] = csub(a1, ja3);
        }
        const int d = (j - k) * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r) dst[d + r * Ns] = v[r];
    }
}

// 2048 points: in a, out a (six passes, b in between)
template <bool INV>
__device__ void fft2048(float2 *a, float2 *b, const float2 *__restrict__ tw) {
    fft_pass<4, INV>(a, b, 1, tw);
    __syncthreads();
    fft_pass<4, INV>(b, a, 4, tw);
    __syncthreads();
    fft_pass<4, INV>(a, b, 16, tw);
    __syncthreads();
    fft_pass<4, INV>(b, a, 64, tw);
    __syncthreads();
    fft_pass<4, INV>(a, b, 256, tw);
    __syncthreads();
    fft_pass<2, INV>(b, a, 1024, tw);
    __syncthreads();
}

__global__ __launch_bounds__(DT) void pitch_detect(DetArgs a) {
    __shared__ float2 A[FFT_N];
    __shared__ float2 B[FFT_N];
    __shared__ float wsum[2][DT / 64];
    __shared__ uint32_t wmax[2][DT / 64];
    __shared__ int s_lobe[2], s_M[2], s_t1[2], s_end[2], s_bmax[2], s_arg[2];
    const int t = threadIdx.x;
    // consecutive pairs on one XCD (workgroups are dealt round-robin over the 8), so their shared cache lines meet in one L2
    uint32_t blk = blockIdx.x;
    if (gridDim.x % 8 == 0) blk = (blk % 8) * (gridDim.x / 8) + blk / 8;
    const uint32_t c0 = 2 * blk;
    const bool has1 = c0 + 1 < a.N;
    // c0 is even, so (c0, c0 + 1) share a tile when W >= 2, and every row starts 8-byte aligned when N is even
    const bool pair2 = has1 && (a.W ? a.W >= 2 : a.N % 2 == 0);
    if (t < 2) {
        s_lobe[t] = WIN;
        s_M[t] = 0;
        s_t1[t] = WIN;
        s_end[t] = WIN;
        s_bmax[t] = 0;
        s_arg[t] = WIN;
    }

    // ---- the window: frames [CHUNK t, CHUNK t + CHUNK) of both channels, kept in registers to the end
    // mb: the largest bit pattern of |x|, which orders as |x| does and puts inf and every NaN on top
    float x0[CHUNK], x1[CHUNK];
    uint32_t mb0 = 0, mb1 = 0;
#pragma unroll
    for (int i = 0; i < CHUNK; ++i) {
        const uint32_t j = CHUNK * t + i;
        uint32_t slot = a.slot0 + j / SLOT;
        if (slot >= RING) slot -= RING;
        const float *base = a.ring + (size_t)slot * SLOT * a.N;
        const size_t e0 = lay(j % SLOT, c0, SLOT, a.N, a.W);
        if (pair2) {                     // the pair is adjacent and 8-byte aligned: one load
            const float2 v = *(const float2 *)(base + e0);
            x0[i] = v.x;
            x1[i] = v.y;
        } else {
            x0[i] = base[e0];
            x1[i] = has1 ? base[lay(j % SLOT, c0 + 1, SLOT, a.N, a.W)] : 0.0f;
        }
        mb0 = max(mb0, __float_as_uint(x0[i]) & 0x7fffffffu);
        mb1 = max(mb1, __float_as_uint(x1[i]) & 0x7fffffffu);
    }
    const int lane = t & 63, wv = t >> 6;
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        mb0 = max(mb0, (uint32_t)__shfl_xor((int)mb0, d, 64));
        mb1 = max(mb1, (uint32_t)__shfl_xor((int)mb1, d, 64));
    }
    if (lane == 0) {
        wmax[0][wv] = mb0;
        wmax[1][wv] = mb1;
    }
    __syncthreads();
    for (int w = 0; w < DT / 64; ++w) {
        mb0 = max(mb0, wmax[0][w]);
        mb1 = max(mb1, wmax[1][w]);
    }
    // Each channel goes into the pair scaled by its OWN power of two, 2^(128 - E) with E the biased exponent of its max |x|
    // (max |x| lands in [2, 4); a subnormal maximum takes E = 1): exact, and from here on neither channel's level reaches the
    // other's rounding.  A non-finite channel goes in as zeros; it has no result anyway.  n(tau) is a ratio and needs no
    // scaling back; the power does (pw_scale).
    const bool bad0 = mb0 >= 0x7f800000u, bad1 = mb1 >= 0x7f800000u;
    const uint32_t E0 = max(mb0 >> 23, 1u), E1 = max(mb1 >> 23, 1u);
    const float sc0 = bad0 ? 0.0f : __uint_as_float((255u - E0) << 23);
    const float sc1 = bad1 ? 0.0f : __uint_as_float((255u - E1) << 23);
    float q0 = 0.0f, q1 = 0.0f;
#pragma unroll
    for (int i = 0; i < CHUNK; ++i) {
        const uint32_t j = CHUNK * t + i;
        x0[i] = bad0 ? 0.0f : x0[i] * sc0;
        x1[i] = bad1 ? 0.0f : x1[i] * sc1;
        A[j] = make_float2(x0[i], x1[i]);
        A[j + WIN] = make_float2(0.0f, 0.0f);
        q0 += x0[i] * x0[i];
        q1 += x1[i] * x1[i];
    }
    // prefix sums of x^2: P[k] = sum_{j<k} x_j^2 for this thread's k, from a scan of the per-thread sums
    float i0 = q0, i1 = q1;
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        const float u0 = __shfl_up(i0, d, 64), u1 = __shfl_up(i1, d, 64);
        if (lane >= d) {
            i0 += u0;
            i1 += u1;
        }
    }
    if (lane == 63) {
        wsum[0][wv] = i0;
        wsum[1][wv] = i1;
    }
    __syncthreads();
    float e0 = i0 - q0, e1 = i1 - q1, tot0 = 0.0f, tot1 = 0.0f;
    for (int w = 0; w < DT / 64; ++w) {
        if (w < wv) {
            e0 += wsum[0][w];
            e1 += wsum[1][w];
        }
        tot0 += wsum[0][w];
        tot1 += wsum[1][w];
    }
    float pre0[CHUNK], pre1[CHUNK];      // P[CHUNK t + i]
#pragma unroll
    for (int i = 0; i < CHUNK; ++i) {
        pre0[i] = e0;
        pre1[i] = e1;
        e0 += x0[i] * x0[i];
        e1 += x1[i] * x1[i];
    }

    // ---- r_lin of both channels
    const float2 *tw = a.tw;
    fft2048<false>(A, B, tw);
    for (int k = t; k < FFT_N; k += DT) {
        const float2 z = A[k], zm = A[(FFT_N - k) & (FFT_N - 1)];
        const float ar = z.x + zm.x, ai = z.y - zm.y;    // 2 X0
        const float br = z.x - zm.x, bi = z.y + zm.y;    // 2 i X1
        B[k] = make_float2(ar * ar + ai * ai, br * br + bi * bi);
    }
    __syncthreads();
    fft2048<true>(B, A, tw);             // B = 4 * 2048 * (r_lin0 + i r_lin1)

    // P into A (free now): Pf[ch][k], k in [0, 1024]
    float *Pf = (float *)A;
#pragma unroll
    for (int i = 0; i < CHUNK; ++i) {
        Pf[CHUNK * t + i] = pre0[i];
        Pf[(WIN + 1) + CHUNK * t + i] = pre1[i];
    }
    if (t == 0) {
        Pf[WIN] = tot0;
        Pf[(WIN + 1) + WIN] = tot1;
    }
    __syncthreads();

    // ---- n(tau) for this thread's channel and lags
    const int ch = t / TPC, lt = t % TPC;
    const float *P = Pf + ch * (WIN + 1);
    const float tot = P[WIN];
    const float scale = 1.0f / (4.0f * FFT_N);
    float n[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int tau = PER * lt + i;
        const float2 rv = B[tau];
        float r = ch ? rv.y : rv.x;
        // m_lin(u) = sum_{j < 1024-u} x_j^2 + sum_{j >= u} x_j^2
        float m = P[WIN - tau] + (tot - P[tau]);
        if (tau > (int)PAD) {
            const int u = (int)(WIN + PAD) - tau;
            const float2 ra = B[u];
            r += ch ? ra.y : ra.x;
            m += P[WIN - u] + (tot - P[u]);
        }
        r *= scale;
        n[i] = m > 0.0f ? 2.0f * r / m : 0.0f;
    }
    __syncthreads();
    float *nb = (float *)B + ch * WIN;
#pragma unroll
    for (int i = 0; i < PER; ++i) nb[PER * lt + i] = n[i];

    // ---- the peak pick
    int best = WIN;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int tau = PER * lt + i;
        if (tau >= 1 && !(n[i] > 0.0f) && tau < best) best = tau;
    }
    if (best < (int)WIN) atomicMin(&s_lobe[ch], best);
    __syncthreads();
    const int lobe = s_lobe[ch];
    float mx = 0.0f;
#pragma unroll
    for (int i = 0; i < PER; ++i)
        if (PER * lt + i > lobe && n[i] > mx) mx = n[i];
    if (mx > 0.0f) atomicMax(&s_M[ch], __float_as_int(mx));     // positive floats order as their bits
    __syncthreads();
    const float M = __int_as_float(s_M[ch]);
    const float thr = a.K * M;
    best = WIN;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int tau = PER * lt + i;
        if (tau > lobe && n[i] > 0.0f && n[i] >= thr && tau < best) best = tau;
    }
    if (best < (int)WIN) atomicMin(&s_t1[ch], best);
    __syncthreads();
    const int t1 = s_t1[ch];
    best = WIN;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int tau = PER * lt + i;
        if (tau > t1 && !(n[i] > 0.0f) && tau < best) best = tau;
    }
    if (best < (int)WIN) atomicMin(&s_end[ch], best);
    __syncthreads();
    const int e = s_end[ch];
    mx = 0.0f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int tau = PER * lt + i;
        if (tau >= t1 && tau < e && n[i] > mx) mx = n[i];
    }
    if (mx > 0.0f) atomicMax(&s_bmax[ch], __float_as_int(mx));
    __syncthreads();
    const float bmax = __int_as_float(s_bmax[ch]);
    best = WIN;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int tau = PER * lt + i;
        if (tau >= t1 && tau < e && n[i] == bmax && tau < best) best = tau;
    }
    if (best < (int)WIN) atomicMin(&s_arg[ch], best);
    __syncthreads();

    // ---- the result
    if (lt != 0 || (ch == 1 && !has1)) return;
    const uint32_t mb = ch ? mb1 : mb0;
    if (mb >= 0x7f800000u || mb == 0) return;                    // non-finite, all zero
    // the window's own power: tot is that of x 2^(128 - E), so times 2^(2 (E - 128)), in f64 for the range
    const double pw_scale = __longlong_as_double((long long)(2 * (int)(ch ? E1 : E0) - 256 + 1023) << 52);
    if ((double)tot * pw_scale < (double)a.P) return;            // power below the threshold
    const int k = s_arg[ch];
    if (s_M[ch] == 0 || t1 >= (int)WIN || k >= (int)WIN) return;
    const float b = nb[k];
    if (b < a.C) return;
    const float av = nb[k - 1];
    float delta = 0.0f, y = b;
    if (k < (int)WIN - 1) {
        const float c = nb[k + 1];
        const float den = 2.0f * (2.0f * b - av - c);
        if (den != 0.0f) delta = (c - av) / den;
        y = b + (c - av) * delta / 4.0f;
    }
    a.res[c0 + ch] = make_float2(RATE / ((float)k + delta), y / nb[0]);
}

__global__ void pitch_read(const float2 *__restrict__ res, float *__restrict__ freq, float *__restrict__ clarity, uint32_t N) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const float2 v = res[c];
    freq[c] = v.x;
    clarity[c] = v.y;
}

}  // namespace

struct dspfx_pitch : BankCore<dspfx_pitch_desc> {     // mu: push / read / reset / destroy are serialised
    SlotRing ring;                              // RING slots of 128 x N floats
    float2 *res = nullptr;                      // [N]
    float2 *tw = nullptr;                       // [FFT_N]
    uint64_t frames = 0;                        // frames pushed since create / reset
    std::atomic<int64_t> windows{0};
    std::atomic<float> th[3];                   // dspfx_pitch_param
};

namespace {

void release(dspfx_pitch *p) { release_plain(p, {p->ring.base, p->res, p->tw}); }

// one piece of a push through the slot copy kernel
hipError_t copy_in(const SlotPiece &c, hipStream_t s) { return launch_copy(c.src, c.dst, c.rows, c.len, c.src_pitch, c.dst_pitch, s); }

hipError_t detect(dspfx_pitch *p, uint64_t w, hipStream_t s) {
    DetArgs a;
    a.ring = p->ring.base;
    a.res = p->res;
    a.tw = p->tw;
    a.N = p->desc.channels;
    a.W = p->desc.tile_channels;
    a.slot0 = (uint32_t)((w * SLOTS_PER_WIN) % RING);
    a.P = p->th[DSPFX_PITCH_POWER].load();
    a.C = p->th[DSPFX_PITCH_CLARITY].load();
    a.K = p->th[DSPFX_PITCH_PICK].load();
    pitch_detect<<<(a.N + 1) / 2, DT, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace

extern "C" int dspfx_pitch_create(const dspfx_pitch_desc *desc, dspfx_pitch **out) {
    const int rc = create_checks_plain(desc, out, [] { return DSPFX_OK; });
    if (rc != DSPFX_OK) return rc;
    const uint32_t N = desc->channels;
    dspfx_pitch *p = new (std::nothrow) dspfx_pitch;
    if (!p) return DSPFX_ERR_OOM;
    p->desc = *desc;
    p->ring = {nullptr, RING, SLOT, N, desc->tile_channels};
    p->th[DSPFX_PITCH_POWER] = desc->power_thresh;
    p->th[DSPFX_PITCH_CLARITY] = desc->clarity_thresh;
    p->th[DSPFX_PITCH_PICK] = desc->pick_thresh;
    std::vector<float2> tw(FFT_N);
    twiddles(FFT_N, tw.data());
    if (hipMalloc((void **)&p->ring.base, (size_t)RING * SLOT * N * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&p->res, (size_t)N * sizeof(float2)) != hipSuccess ||
        hipMalloc((void **)&p->tw, FFT_N * sizeof(float2)) != hipSuccess) {
        (void)hipGetLastError();
        release(p);
        return DSPFX_ERR_OOM;
    }
    if (hipMemcpy(p->tw, tw.data(), FFT_N * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(p->res, 0, (size_t)N * sizeof(float2)) != hipSuccess ||
        hipEventCreateWithFlags(&p->ev, hipEventDisableTiming) != hipSuccess) {
        release(p);
        return DSPFX_ERR_HIP;
    }
    *out = p;
    return DSPFX_OK;
}

extern "C" int dspfx_pitch_destroy(dspfx_pitch *p) { return destroy_bank(p, release); }

extern "C" float *dspfx_pitch_slot(dspfx_pitch *p) {
    if (!p) return nullptr;
    std::lock_guard<std::mutex> lk(p->mu);
    return next_slot(p->ring, p->frames);
}

// pitch.rs:120-146 per frame position: window w runs once frame 1024 (w + 1) has been pushed too, and before the ring
// slot that frame went to is overwritten (the 9th slot keeps the window whole up to then; see the top of this file)
extern "C" int dspfx_pitch_push(dspfx_pitch *p, const float *block, uint32_t n_frames, void *stream) {
    if (!p || !block || n_frames == 0) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    const bool in_place = block == next_slot(p->ring, p->frames);
    if (in_place && n_frames != SLOT) return DSPFX_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    return push_pieces(p, p->ring, p->frames, n_frames, s, [&](uint64_t f, uint32_t fa, uint32_t nf) -> int {
        // window w falls due with frame 1024 (w + 1): F >= 1024 (w + 1) + 1.  It is launched before that frame is copied:
        // the copy goes to the ring's ninth slot, never into the window.
        if (f > 0 && f % WIN == 0) {
            BANK_HIP(detect(p, f / WIN - 1, s));
            p->windows.fetch_add(1);
        }
        if (!in_place) BANK_HIP(copy_in(piece_of(p->ring, block, n_frames, fa, f, nf), s));
        return DSPFX_OK;
    });
}

extern "C" int dspfx_pitch_set_param(dspfx_pitch *p, int which, float value) {
    if (!p || which < DSPFX_PITCH_POWER || which > DSPFX_PITCH_PICK || !std::isfinite(value)) return DSPFX_ERR_INVALID;
    p->th[which].store(value);
    return DSPFX_OK;
}

extern "C" int dspfx_pitch_read(dspfx_pitch *p, float *freq, float *clarity, void *stream) {
    if (!p || !freq || !clarity) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    hipStream_t s = (hipStream_t)stream;
    BANK_HIP(hipSetDevice(p->desc.device));
    BANK_HIP(order(p, s));
    const uint32_t N = p->desc.channels;
    pitch_read<<<(N + 255) / 256, 256, 0, s>>>(p->res, freq, clarity, N);
    BANK_HIP(hipGetLastError());
    return DSPFX_OK;
}

extern "C" int dspfx_pitch_reset(dspfx_pitch *p) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    BANK_HIP(hipSetDevice(p->desc.device));
    BANK_HIP(hipMemsetAsync(p->res, 0, (size_t)p->desc.channels * sizeof(float2), p->last));
    p->frames = 0;
    p->windows = 0;
    return DSPFX_OK;
}

extern "C" int64_t dspfx_pitch_windows(const dspfx_pitch *p) {
    if (!p) return DSPFX_ERR_INVALID;
    return p->windows.load();
}
