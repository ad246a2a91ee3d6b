// resample_kernels.hip -- the output resampler bank (include/dspfx.h, dspfx_resample_*): the reference's output callback
// (devices.rs:394-498) for N channels that share one device rate, 48 kHz -> target_hz through dasp's Converter + Sinc.
//   resample_pull       one callback in steady state (idx == 8): the 16-frame window of a lane's channels in registers
//   resample_pull_warm  the same while idx < 8 (the first frames after create / reset): the window indexed at run time
//   resample_silence    an underrun: from_f32(0.0) in every output slot
// Who computes what: the phase sequence and the windowed-sinc coefficients depend on the call sequence only, so the host
// makes them in f64 (dspfx_resample_plan) and the kernels read one PlanRow per output frame at a wave-uniform address
// (scalar loads); a lane does, per tap, one f64 multiply, one rounding to f32 and one f32 add, in the reference's order.
// The plan goes host -> device in stream order: a small ring of page-locked tables, copied into one device table.
//
// resample_pull walks the waiting frames once, in order.  The window is `w[16]` with rotating names: the source loop is
// unrolled by 16, in phase h the oldest frame is w[h] and ring[k] = w[(h + k) % 16], and a pull overwrites w[h] -- no moves.
// The window holds the frames as f64 (the widening is exact and done once per frame, not once per tap).  Between two
// pulls the outputs that fall due are made; each is written once, already in the device format (pcm_rules.h from_f32).
// A lane owns V adjacent channels: V = 4 (16-byte loads of the FIFO rows and of the state, 8 / 16 / 2 x 16 byte stores)
// when the layout keeps every row 16-byte aligned and N is at least 262144 (below that one channel a lane fills the chip
// better; DSPFX_RESAMPLE_VEC=0 / 1, read at create, forces V = 1 / V = 4), else V = 1.  Frame-major is the tiled addressing
// with W = N.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/dspfx.h"
#include "bank_common.hip.h"
#include "slot_ring.hip.h"
#include "pcm_kernels.h"
#include "pcm_rules.h"

namespace {

using dspfx::from_f32;
using dspfx::PcmType;

constexpr uint32_t TAPS = 16;                       // Sinc over ring_buffer::Fixed<[f32; 16]>
constexpr uint32_t DEPTH = 8;                       //   its depth: 8 taps to each side
constexpr uint32_t MAX_FRAMES = DSPFX_RESAMPLE_MAX_FRAMES;
constexpr int RS_WG = 256;
constexpr int PLAN_RING = 8;                        // page-locked plan tables in flight

// one output frame of the plan, as the kernels read it
struct PlanRow {
    double c[TAPS];        // c[2 n], c[2 n + 1]: left / right coefficient of tap n
    uint32_t adv;          // source frames pulled before this frame
    uint32_t depth;        // tap pairs summed
    uint32_t nl;           // idx at this frame: the left taps start at ring[nl], the right ones at ring[nl + 1]
    uint32_t pad;
};
// the plan through the constant address space: a wave-uniform index gives scalar loads whatever the stores around them
typedef const __attribute__((address_space(4))) PlanRow *PlanPtr;

struct PullArgs {
    const float *fifo;     // slots x (BF frames in the layout)
    float *state;          // [16][N]: ring[k] of channel c at k * N + c
    const PlanRow *plan;   // [n_out]
    void *out;
    uint32_t N, W;         // W = N for frame-major
    uint32_t BF, slots;
    uint32_t n_out;
    uint32_t slot0, row0;  // where the first waiting frame lies
    uint32_t avail;        // frames waiting (the converter's view); pulls past them feed 0.0
};

// ring index of the t-th term of the steady-state sum (nl = 8): left 8, 7, .., 1 and right 9, .., 15, then 16 % 16 = 0
__device__ __forceinline__ constexpr int tap_k(int t) { return (t & 1) ? (9 + t / 2) % 16 : 8 - t / 2; }

template <int V>
__device__ __forceinline__ void load_v(const float *p, float (&x)[V]) {
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
        x[0] = p[0];
    }
}

// V adjacent elements of the output, each one device frame of CH samples of the format
template <int FMT, int CH, int V>
__device__ __forceinline__ void store_out(void *out, size_t elem, const float (&v)[V]) {
    using T = typename PcmType<FMT>::T;
    T s[V * CH];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const T y = from_f32<FMT>(v[i]);
        s[CH * i] = y;
        if constexpr (CH == 2) s[2 * i + 1] = y;
    }
    T *p = (T *)out + elem * CH;
    constexpr size_t bytes = sizeof(T) * V * CH;
    if constexpr (bytes % 16 == 0) {
        uint4 raw[bytes / 16];
        __builtin_memcpy(raw, s, bytes);
#pragma unroll
        for (size_t i = 0; i < bytes / 16; ++i) reinterpret_cast<uint4 *>(p)[i] = raw[i];
    } else if constexpr (bytes == 8) {
        uint2 raw;
        __builtin_memcpy(&raw, s, 8);
        *reinterpret_cast<uint2 *>(p) = raw;
    } else {
#pragma unroll
        for (int i = 0; i < V * CH; ++i) p[i] = s[i];
    }
}

// the FIFO row of waiting frame j, advanced one frame at a time: scalar arithmetic only
struct Cursor {
    uint32_t j, slot, row;
};

template <int FMT, int CH, int V>
__global__ __launch_bounds__(RS_WG) void resample_pull(const PullArgs a) {
    const uint32_t c = (blockIdx.x * RS_WG + threadIdx.x) * V;
    if (c >= a.N) return;
    const uint32_t tile = c / a.W, cw = c - tile * a.W;
    const float *in = a.fifo + (size_t)tile * a.BF * a.W + cw;
    const size_t slot_elems = (size_t)a.BF * a.N;
    const size_t out0 = (size_t)tile * a.n_out * a.W + cw;
    const PlanPtr plan = (PlanPtr)a.plan;

    double w[TAPS][V];
#pragma unroll
    for (int k = 0; k < (int)TAPS; ++k) {
        float x[V];
        load_v<V>(a.state + (size_t)k * a.N + c, x);
#pragma unroll
        for (int i = 0; i < V; ++i) w[k][i] = (double)x[i];
    }

    // `pre` is waiting frame cur.j, loaded one pull ahead of its use
    Cursor cur{0, a.slot0, a.row0};
    float pre[V];
    auto fetch = [&]() {
        if (cur.j < a.avail) {
            load_v<V>(in + (size_t)cur.slot * slot_elems + (size_t)cur.row * a.W, pre);
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) pre[i] = 0.0f;
        }
        ++cur.j;
        if (++cur.row == a.BF) {
            cur.row = 0;
            if (++cur.slot == a.slots) cur.slot = 0;
        }
    };
    fetch();

    uint32_t o = 0;
    uint32_t need = plan[0].adv;
    for (;;) {
#pragma unroll
        for (int h = 0; h < (int)TAPS; ++h) {
            while (need == 0) {
                float v[V];
#pragma unroll
                for (int i = 0; i < V; ++i) v[i] = 0.0f;
#pragma unroll
                for (int t = 0; t < (int)TAPS; ++t) {
                    const double ct = plan[o].c[t];
#pragma unroll
                    for (int i = 0; i < V; ++i) v[i] = v[i] + (float)(ct * w[(h + tap_k(t)) & 15][i]);
                }
                store_out<FMT, CH, V>(a.out, out0 + (size_t)o * a.W, v);
                if (++o == a.n_out) {
#pragma unroll
                    for (int k = 0; k < (int)TAPS; ++k) {
#pragma unroll
                        for (int i = 0; i < V; ++i) v[i] = (float)w[(h + k) & 15][i];      // exact: they came from f32
                        if constexpr (V == 4) {
                            *reinterpret_cast<float4 *>(a.state + (size_t)k * a.N + c) = make_float4(v[0], v[1], v[2], v[3]);
                        } else {
                            a.state[(size_t)k * a.N + c] = v[0];
                        }
                    }
                    return;
                }
                need = plan[o].adv;
            }
#pragma unroll
            for (int i = 0; i < V; ++i) w[h][i] = (double)pre[i];
            fetch();
            --need;
        }
    }
}

// idx < 8 somewhere in the call: the taps start at ring[nl] with nl below 8 and fewer pairs are summed, so the window is
// indexed at run time.  One lane per channel, the window slid by moves.  It runs for the first frames of a stream only.
template <int FMT, int CH>
__global__ __launch_bounds__(RS_WG) void resample_pull_warm(const PullArgs a) {
    const uint32_t c = blockIdx.x * RS_WG + threadIdx.x;
    if (c >= a.N) return;
    const uint32_t tile = c / a.W, cw = c - tile * a.W;
    const float *in = a.fifo + (size_t)tile * a.BF * a.W + cw;
    const size_t slot_elems = (size_t)a.BF * a.N;
    const size_t out0 = (size_t)tile * a.n_out * a.W + cw;
    const PlanPtr plan = (PlanPtr)a.plan;
    float ring[TAPS];
    for (uint32_t k = 0; k < TAPS; ++k) ring[k] = a.state[(size_t)k * a.N + c];
    Cursor cur{0, a.slot0, a.row0};
    for (uint32_t o = 0; o < a.n_out; ++o) {
        for (uint32_t p = plan[o].adv; p; --p) {
            const float x = cur.j < a.avail ? in[(size_t)cur.slot * slot_elems + (size_t)cur.row * a.W] : 0.0f;
            ++cur.j;
            if (++cur.row == a.BF) {
                cur.row = 0;
                if (++cur.slot == a.slots) cur.slot = 0;
            }
            for (uint32_t k = 0; k + 1 < TAPS; ++k) ring[k] = ring[k + 1];
            ring[TAPS - 1] = x;
        }
        const uint32_t nl = plan[o].nl, depth = plan[o].depth;
        float v = 0.0f;
        for (uint32_t n = 0; n < depth; ++n) {
            v = v + (float)(plan[o].c[2 * n] * (double)ring[(nl - n) & 15]);
            v = v + (float)(plan[o].c[2 * n + 1] * (double)ring[(nl + 1 + n) & 15]);
        }
        const float vv[1] = {v};
        store_out<FMT, CH, 1>(a.out, out0 + (size_t)o * a.W, vv);
    }
    for (uint32_t k = 0; k < TAPS; ++k) a.state[(size_t)k * a.N + c] = ring[k];
}

// an underrun: every slot is from_f32(0.0); `n` samples (elements x device channels), 16 bytes per lane where aligned
template <int FMT>
__global__ __launch_bounds__(RS_WG) void resample_silence(typename PcmType<FMT>::T *__restrict__ out, size_t n, int vec) {
    using T = typename PcmType<FMT>::T;
    constexpr int PER = 16 / (int)sizeof(T);
    const T z = from_f32<FMT>(0.0f);
    const size_t nv = vec ? n / PER : 0;
    const size_t stride = (size_t)gridDim.x * RS_WG;
    T s[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) s[i] = z;
    uint4 raw;
    __builtin_memcpy(&raw, s, 16);
    for (size_t e = (size_t)blockIdx.x * RS_WG + threadIdx.x; e < nv; e += stride) reinterpret_cast<uint4 *>(out)[e] = raw;
    for (size_t e = nv * PER + (size_t)blockIdx.x * RS_WG + threadIdx.x; e < n; e += stride) out[e] = z;
}

enum Path { WARM, FAST1, FAST4 };

template <int FMT, int CH>
hipError_t launch_pull_as(Path path, const PullArgs &a, hipStream_t s) {
    const uint32_t lanes = path == FAST4 ? a.N / 4 : a.N;
    const dim3 g((lanes + RS_WG - 1) / RS_WG), b(RS_WG);
    if (path == FAST4) hipLaunchKernelGGL((resample_pull<FMT, CH, 4>), g, b, 0, s, a);
    else if (path == FAST1) hipLaunchKernelGGL((resample_pull<FMT, CH, 1>), g, b, 0, s, a);
    else hipLaunchKernelGGL((resample_pull_warm<FMT, CH>), g, b, 0, s, a);
    return hipGetLastError();
}

template <int CH>
hipError_t launch_pull_ch(int32_t fmt, Path path, const PullArgs &a, hipStream_t s) {
    switch (fmt) {
    case DSPFX_SAMPLE_F32: return launch_pull_as<DSPFX_SAMPLE_F32, CH>(path, a, s);
    case DSPFX_SAMPLE_I16: return launch_pull_as<DSPFX_SAMPLE_I16, CH>(path, a, s);
    case DSPFX_SAMPLE_U16: return launch_pull_as<DSPFX_SAMPLE_U16, CH>(path, a, s);
    case DSPFX_SAMPLE_I32: return launch_pull_as<DSPFX_SAMPLE_I32, CH>(path, a, s);
    default: return hipErrorInvalidValue;
    }
}

template <int FMT>
hipError_t launch_silence_as(void *out, size_t n, hipStream_t s) {
    using T = typename PcmType<FMT>::T;
    const int vec = ((uintptr_t)out & 15u) == 0;
    const size_t lanes = std::max<size_t>(1, n / (16 / sizeof(T)));
    const unsigned g = (unsigned)std::min<size_t>((lanes + RS_WG - 1) / RS_WG, 8192);
    hipLaunchKernelGGL((resample_silence<FMT>), dim3(g), dim3(RS_WG), 0, s, (T *)out, n, vec);
    return hipGetLastError();
}

hipError_t launch_silence(int32_t fmt, void *out, size_t n, hipStream_t s) {
    switch (fmt) {
    case DSPFX_SAMPLE_F32: return launch_silence_as<DSPFX_SAMPLE_F32>(out, n, s);
    case DSPFX_SAMPLE_I16: return launch_silence_as<DSPFX_SAMPLE_I16>(out, n, s);
    case DSPFX_SAMPLE_U16: return launch_silence_as<DSPFX_SAMPLE_U16>(out, n, s);
    case DSPFX_SAMPLE_I32: return launch_silence_as<DSPFX_SAMPLE_I32>(out, n, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

struct dspfx_resample : BankCore<dspfx_resample_desc> {      // mu: every call but plan is serialised
    SlotRing fifo;                               // slots x block_frames x N
    float *state = nullptr;                      // [16][N]
    PlanRow *dplan = nullptr;                    // [MAX_FRAMES], the table the kernels read
    PlanRow *hplan[PLAN_RING] = {};              // page-locked tables, one per pull in flight
    hipEvent_t hev[PLAN_RING] = {};              //   recorded behind the copy out of it
    bool hbusy[PLAN_RING] = {};
    uint32_t hnext = 0;
    std::vector<uint32_t> adv, depth;            // dspfx_resample_plan's output, before it is packed into rows
    std::vector<double> coeff;
    uint64_t head = 0, tail = 0;                 // frames released / pushed since create or reset
    double value = 0.0;                          // the converter's interpolation_value
    uint32_t idx = 0;                            // the interpolator's idx
    int vec = -1;                                // DSPFX_RESAMPLE_VEC at create: 0 / 1 force the lane width, -1 picks
};

namespace {

void release(dspfx_resample *r) {
    release_plain_by(r, [r] {
        free_device({r->fifo.base, r->state, r->dplan});
        for (int i = 0; i < PLAN_RING; ++i) {
            if (r->hplan[i]) (void)hipHostFree(r->hplan[i]);
            if (r->hev[i]) (void)hipEventDestroy(r->hev[i]);
        }
    });
}

uint64_t capacity(const dspfx_resample *r) { return (uint64_t)r->desc.slots * r->desc.block_frames; }

// devices.rs:401 / 447: (data.len() as f32 * (48_000.0 / rate as f32)) as usize
uint32_t input_len_of(uint32_t n_out, uint32_t target_hz) {
    const float f = (float)n_out * (48000.0f / (float)target_hz);
    return f >= 4294967040.0f ? 0xFFFFFFFFu : (uint32_t)f;
}

// one piece of a push through the copy engine
hipError_t copy_in(const SlotPiece &c, hipStream_t s) {
    if (!c.dst_pitch) return hipMemcpyAsync(c.dst, c.src, c.len * sizeof(float), hipMemcpyDeviceToDevice, s);
    return hipMemcpy2DAsync(c.dst, c.dst_pitch * sizeof(float), c.src, c.src_pitch * sizeof(float), c.len * sizeof(float), c.rows,
                            hipMemcpyDeviceToDevice, s);
}

}  // namespace

extern "C" int dspfx_resample_plan(uint32_t target_hz, double *value, uint32_t *idx, uint32_t n_out, uint32_t *advance,
                                   uint32_t *depth, double *coeff, uint32_t *input_len, uint32_t *pulled) {
    if (target_hz == 0 || !value || !idx || n_out > MAX_FRAMES || *idx > DEPTH || !(*value >= 0.0) || !std::isfinite(*value))
        return DSPFX_ERR_INVALID;
    const double ratio = 48000.0 / (double)target_hz;          // Converter::from_hz_to_hz
    double v = *value;
    uint32_t ix = *idx, total = 0;
    for (uint32_t o = 0; o < n_out; ++o) {
        uint32_t adv = 0;
        while (v >= 1.0) {                                       // Converter::next: advance whole source frames
            ++adv;
            if (ix < DEPTH) ++ix;                                // Sinc::next_source_frame
            v -= 1.0;
        }
        const uint32_t d = ix >= DEPTH - 1 ? DEPTH : ix + 1;     // Sinc::interpolate: the depth clipped at the ring's ends
        if (advance) advance[o] = adv;
        if (depth) depth[o] = d;
        if (coeff) {
            double *c = coeff + (size_t)TAPS * o;
            const double phil = v, phir = 1.0 - v;
            for (uint32_t n = 0; n < DEPTH; ++n) {
                if (n >= d) {
                    c[2 * n] = c[2 * n + 1] = 0.0;
                    continue;
                }
                double a = M_PI * (phil + (double)n);
                double first = a == 0.0 ? 1.0 : std::sin(a) / a;
                double second = 0.5 + 0.5 * std::cos(a / (double)DEPTH);
                c[2 * n] = first * second;
                a = M_PI * (phir + (double)n);
                first = a == 0.0 ? 1.0 : std::sin(a) / a;
                second = 0.5 + 0.5 * std::cos(a / (double)DEPTH);
                c[2 * n + 1] = first * second;
            }
        }
        total += adv;
        v += ratio;
    }
    *value = v;
    *idx = ix;
    if (input_len) *input_len = input_len_of(n_out, target_hz);
    if (pulled) *pulled = total;
    return DSPFX_OK;
}

extern "C" int dspfx_resample_create(const dspfx_resample_desc *desc, dspfx_resample **out) {
    const int rc = create_checks_plain(desc, out, [desc] {
        if (desc->block_frames == 0 || desc->block_frames > MAX_FRAMES || desc->slots < 3 || desc->target_hz == 0) return DSPFX_ERR_INVALID;
        if (!dspfx::pcm_format_ok(desc->out_format) || !dspfx::pcm_channels_ok(desc->out_channels)) return DSPFX_ERR_INVALID;
        return DSPFX_OK;
    });
    if (rc != DSPFX_OK) return rc;
    const uint32_t N = desc->channels;
    dspfx_resample *r = new (std::nothrow) dspfx_resample;
    if (!r) return DSPFX_ERR_OOM;
    r->desc = *desc;
    r->fifo = {nullptr, desc->slots, desc->block_frames, N, desc->tile_channels};
    if (const char *e = std::getenv("DSPFX_RESAMPLE_VEC")) r->vec = std::atoi(e) ? 1 : 0;      // experiments: the lane width
    r->adv.resize(MAX_FRAMES);
    r->depth.resize(MAX_FRAMES);
    r->coeff.resize((size_t)MAX_FRAMES * TAPS);
    if (hipMalloc((void **)&r->fifo.base, (size_t)capacity(r) * N * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&r->state, (size_t)TAPS * N * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&r->dplan, (size_t)MAX_FRAMES * sizeof(PlanRow)) != hipSuccess) {
        (void)hipGetLastError();
        release(r);
        return DSPFX_ERR_OOM;
    }
    for (int i = 0; i < PLAN_RING; ++i) {
        if (hipHostMalloc((void **)&r->hplan[i], (size_t)MAX_FRAMES * sizeof(PlanRow), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            release(r);
            return DSPFX_ERR_OOM;
        }
        if (hipEventCreateWithFlags(&r->hev[i], hipEventDisableTiming) != hipSuccess) {
            release(r);
            return DSPFX_ERR_HIP;
        }
    }
    if (hipMemset(r->state, 0, (size_t)TAPS * N * sizeof(float)) != hipSuccess ||
        hipEventCreateWithFlags(&r->ev, hipEventDisableTiming) != hipSuccess) {
        release(r);
        return DSPFX_ERR_HIP;
    }
    *out = r;
    return DSPFX_OK;
}

extern "C" int dspfx_resample_destroy(dspfx_resample *r) { return destroy_bank(r, release); }

extern "C" float *dspfx_resample_slot(dspfx_resample *r) {
    if (!r) return nullptr;
    std::lock_guard<std::mutex> lk(r->mu);
    if (r->tail - r->head + r->fifo.frames > capacity(r)) return nullptr;       // no slot is free
    return next_slot(r->fifo, r->tail);
}

extern "C" int dspfx_resample_push(dspfx_resample *r, const float *block, uint32_t n_frames, void *stream) {
    if (!r || !block || n_frames == 0) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(r->mu);
    const bool in_place = block == next_slot(r->fifo, r->tail);
    if (in_place && n_frames != r->fifo.frames) return DSPFX_ERR_INVALID;
    if (r->tail - r->head + n_frames > capacity(r)) return DSPFX_ERR_STATE;
    if (in_place) {                      // nothing to launch: the writer and the pulls are stream-ordered by the caller
        r->tail += n_frames;
        return DSPFX_OK;
    }
    hipStream_t s = (hipStream_t)stream;
    return push_pieces(r, r->fifo, r->tail, n_frames, s, [&](uint64_t f, uint32_t fa, uint32_t nf) -> int {
        BANK_HIP(copy_in(piece_of(r->fifo, block, n_frames, fa, f, nf), s));
        return DSPFX_OK;
    });
}

extern "C" int dspfx_resample_pull(dspfx_resample *r, void *out, uint32_t n_out, uint32_t *consumed, int32_t *underrun,
                                   void *stream) {
    if (!r || !out || n_out == 0 || n_out > MAX_FRAMES) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(r->mu);
    const dspfx_resample_desc &d = r->desc;
    hipStream_t s = (hipStream_t)stream;
    BANK_HIP(hipSetDevice(d.device));
    const uint64_t avail = r->tail - r->head;
    if (consumed) *consumed = 0;
    if (underrun) *underrun = 0;
    if (avail < input_len_of(n_out, d.target_hz)) {              // try_grant failed: silence, nothing touched
        BANK_HIP(order(r, s));
        BANK_HIP(launch_silence(d.out_format, out, (size_t)n_out * d.channels * d.out_channels, s));
        if (underrun) *underrun = 1;
        return DSPFX_OK;
    }
    // the plan, on copies of the converter state: it is committed once everything has been queued
    double value = r->value;
    uint32_t idx = r->idx, pulled = 0;
    const uint32_t idx0 = idx;
    if (dspfx_resample_plan(d.target_hz, &value, &idx, n_out, r->adv.data(), r->depth.data(), r->coeff.data(), nullptr, &pulled) != DSPFX_OK)
        return DSPFX_ERR_INVALID;
    const uint32_t h = r->hnext;
    if (r->hbusy[h]) BANK_HIP(hipEventSynchronize(r->hev[h]));     // PLAN_RING pulls ago: long done unless the device is far behind
    PlanRow *rows = r->hplan[h];
    uint32_t nl = idx0;
    for (uint32_t o = 0; o < n_out; ++o) {
        nl = std::min<uint32_t>(DEPTH, nl + r->adv[o]);
        std::memcpy(rows[o].c, r->coeff.data() + (size_t)TAPS * o, sizeof rows[o].c);
        rows[o].adv = r->adv[o];
        rows[o].depth = r->depth[o];
        rows[o].nl = nl;
        rows[o].pad = 0;
    }
    BANK_HIP(order(r, s));
    BANK_HIP(hipMemcpyAsync(r->dplan, rows, (size_t)n_out * sizeof(PlanRow), hipMemcpyHostToDevice, s));
    BANK_HIP(hipEventRecord(r->hev[h], s));
    r->hbusy[h] = true;
    r->hnext = (h + 1) % PLAN_RING;

    PullArgs a;
    a.fifo = r->fifo.base;
    a.state = r->state;
    a.plan = r->dplan;
    a.out = out;
    a.N = d.channels;
    a.W = d.tile_channels ? d.tile_channels : d.channels;
    a.BF = d.block_frames;
    a.slots = d.slots;
    a.n_out = n_out;
    a.slot0 = (uint32_t)((r->head / d.block_frames) % d.slots);
    a.row0 = (uint32_t)(r->head % d.block_frames);
    a.avail = (uint32_t)avail;
    // the register-window kernel needs idx == 8 for every frame; 4 channels per lane need 16-byte rows everywhere
    const bool can4 = a.W % 4 == 0 && ((uintptr_t)out & 15u) == 0;
    // measured (profiles/resample_rate.txt): 4 channels a lane win once there is a workgroup of them for every CU, 1 below that
    const bool want4 = r->vec >= 0 ? r->vec != 0 : a.N / 4 >= 256u * RS_WG;
    const Path path = idx0 < DEPTH ? WARM : (can4 && want4 ? FAST4 : FAST1);
    const hipError_t err = d.out_channels == 2 ? launch_pull_ch<2>(d.out_format, path, a, s) : launch_pull_ch<1>(d.out_format, path, a, s);
    BANK_HIP(err);
    const uint32_t used = (uint32_t)std::min<uint64_t>(pulled, avail);      // CountingSignal: pulls past the view do not count
    r->head += used;
    r->value = value;
    r->idx = idx;
    if (consumed) *consumed = used;
    return DSPFX_OK;
}

extern "C" int64_t dspfx_resample_available(dspfx_resample *r) {
    if (!r) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(r->mu);
    return (int64_t)(r->tail - r->head);
}

extern "C" int dspfx_resample_skip(dspfx_resample *r, uint32_t n_frames) {
    if (!r) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(r->mu);
    if (n_frames > r->tail - r->head) return DSPFX_ERR_INVALID;
    r->head += n_frames;
    return DSPFX_OK;
}

extern "C" int dspfx_resample_reset(dspfx_resample *r) {
    if (!r) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(r->mu);
    BANK_HIP(hipSetDevice(r->desc.device));
    BANK_HIP(hipMemsetAsync(r->state, 0, (size_t)TAPS * r->desc.channels * sizeof(float), r->last));
    r->head = r->tail = 0;
    r->value = 0.0;
    r->idx = 0;
    return DSPFX_OK;
}
