// cancel_kernels.hip -- the channel-canceller bank (include/dspfx.h, dspfx_cancel_*): channel c carries no node or ONE adaptive
// (NLMS) FIR filter of its own: T taps (1 .. max_taps) that the DEVICE updates every frame, a step size mu, a regulariser eps, a
// bulk delay D (0 .. max_delay) and the host's adapt switch.  A channel without a node copies its microphone block.
//
// The arithmetic is defined here (the reference has no such node); all of it is f32, every operation rounded once, as written:
//   u[k]  = ref[n - D - k], k < T                  +0.0 before the node's first frame (its creation or its last reset)
//   dot(a, b) = (s_0 + s_1) + (s_2 + s_3)          four chains from +0.0, chain j takes the k = j (mod 4) in ascending k,
//                                                  s_j = s_j + (a[k] * b[k]); no term k >= T exists
//   y = dot(w, u);  e = d[n] - y;  out[n] = e
//   adapt only:  p = dot(u, u);  g = (mu * e) / (p + eps);  w[k] = w[k] + (g * u[k]), k < T
//   levels: sum d * d and sum e * e over the run, in frame order from +0.0
// The reference samples are in a ring in TIME of R rows, R = max_delay + max_taps + 16 rounded up to a multiple of 8: the sample of
// the bank's frame n is row n mod R for every channel (the host carries the one row counter).  The rows stand in groups of 8,
// [row / 8][N][8] floats (ring_at).  A lane writes a frame's reference sample into the ring
// before it reads any, and a store that makes a node (or resets one) clears the channel's column, so the window before the node's
// first frame is +0.0 without a word per channel or a select in the kernel.  The weights are [tap][N] floats, rows k >= T always
// +0.0 (create clears them, a shorter T, a drop and a reset clear what they leave).
//
// Two bodies in one kernel.  GENERAL (cancel_frame): one frame of one lane, the two dot products and the update as written above
// with loops under the lane's own T, weights and window read from the tables: right for lanes of different T in one wave.
// FAST (cancel_fast<TP, FULL>): a wave whose present lanes share T <= 64 keeps the weights in registers for the whole run and the
// window in a sliding register window, FB = 8 frames per block: per block 8 loads of the microphone, of the reference and of the
// ring's new rows, the weights read once and written once per run.  TP is T's class (8, 16, 32, 64); FULL: T == TP, no term is
// tested; else every term k < TP is under a select on k < T (a select, never a product with a padded zero: an infinity just
// outside the window must not meet a zero).  Both bodies do the same operations in the same order, so they give the same bits; a
// run's frames beyond its last whole block go through the general body.  A wave without a node copies.  Nothing is shared
// between channels: no LDS, no atomics.  The kernel is instantiated per largest class it holds (cancel_run<0 | 8 | 16 | 32 | 64>) and
// the host launches the instance of the longest filter the bank carries: one kernel with every class took the 64-tap window's
// registers (256 VGPRs and AGPRs beside them, 1 wave per SIMD) whatever the bank carried; cancel_run<32> takes 212 VGPRs, 2 waves
// per SIMD, scratch 0.  Measured at 2^20 channels x 128 frames, T = 32, a delay of its own per channel: 1.35 ms,
// the general body forced 57 ms; 16 frames per block 1.35 ms, 4 frames 1.83 ms, the window's squares kept in registers 1.45 ms.
//
// Stores go through the staged-store queue (store_queue.hip.h).  The host keeps every node's T, D, mu, eps and adapt, so a `set`
// stages the resolved words of every channel it names, with what has to be cleared (a new node's column, the rows a shorter T
// leaves); `load` stages the rows of weights.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dspfx.h"
#include "channel_bank.hip.h"
#include "lane_io.hip.h"

namespace {

// the forms of the fast body that were timed against each other: -DCANCEL_FB=16, -DCANCEL_SQ=1, -DCANCEL_WG=128
#ifndef CANCEL_FB
#define CANCEL_FB 8
#endif
#ifndef CANCEL_SQ
#define CANCEL_SQ 0
#endif
#ifndef CANCEL_WG
#define CANCEL_WG 256
#endif
constexpr uint32_t CWG = CANCEL_WG;
constexpr int FB = CANCEL_FB;                    // frames per block of the fast body
constexpr bool SQ = CANCEL_SQ;                   // the window's squares kept beside it: u * u once per sample, not once per frame and tap
constexpr uint32_t RING_PAD = 16;                // the ring has max_delay + max_taps + RING_PAD rows (>= FB)
constexpr uint32_t FAST_MAX_T = 64;              // the largest T the fast body keeps in registers

// the node word of a channel: T in the low 16 bits (0: no node), adapt above
constexpr uint32_t CN_T = 0xFFFFu, CN_ADAPT = 1u << 16;
// a set's fifth staged word: the T the node had in the low 16 bits, `fresh` (a new node: clear the column) above
constexpr uint32_t CW_FRESH = 1u << 16;

struct CancelArgs {
    const float *mic;            // may be `out`: no __restrict__
    const float *ref;
    float *out;
    float *w;                    // [max_taps][N]
    float *ring;                 // [R][N]
    const uint32_t *tn;          // [N]
    const uint32_t *dl;          // [N]
    const float *mu, *eps;       // [N]
    float *lev;                  // [2][N]
    uint32_t N, W, nf, R;
    uint32_t row;                // the ring row of the run's first frame
};

__device__ __forceinline__ float dot_end(const float (&s)[4]) { return __fadd_rn(__fadd_rn(s[0], s[1]), __fadd_rn(s[2], s[3])); }

// ring row r, d rows back (d <= R)
__device__ __forceinline__ uint32_t rows_back(uint32_t r, uint32_t d, uint32_t R) { return r >= d ? r - d : r + R - d; }

__device__ __forceinline__ uint32_t row_next(uint32_t r, uint32_t R) { return r + 1 == R ? 0 : r + 1; }

// the ring's element of row r in a lane's column `col` = ring + 8 * c: the rows stand in groups of RG = 8, [row / 8][N][8], so the 8
// rows a lane writes or reads per block are 32 contiguous bytes of its own and the lanes' groups follow one another; n8 = 8 * N.
// (With plain [row][N] every lane of a wave with a delay of its own reads another row: 64 cache lines per load; measured, DESIGN
// section 8.)
constexpr uint32_t RG = 8;
__host__ __device__ __forceinline__ size_t ring_at(uint32_t r, size_t n8) { return (size_t)(r / RG) * n8 + r % RG; }

// the general body: one frame of one lane whose reference sample is already in the ring.  wc, col: the lane's column of the weights
// and of the ring; r0: the ring row of u[0] (the frame's row, D rows back); d: the microphone sample -> e.  Four terms' loads are
// issued together (a weight past T is read at the last tap's place, a row past the window is a row of the ring; neither is used)
__device__ __forceinline__ float cancel_frame(float *wc, const float *col, size_t N, size_t n8, uint32_t R, uint32_t T, bool adapt, float mu, float eps, uint32_t r0,
                                              float d) {
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f}, p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t r = r0;
    for (uint32_t k = 0; k < T; k += 4) {
        float wv[4], uv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            wv[j] = wc[min(k + j, T - 1) * N];
            uv[j] = col[ring_at(r, n8)];
            r = r ? r - 1 : R - 1;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (k + j < T) {
                s[j] = __fadd_rn(s[j], __fmul_rn(wv[j], uv[j]));
                p[j] = __fadd_rn(p[j], __fmul_rn(uv[j], uv[j]));
            }
    }
    const float e = __fsub_rn(d, dot_end(s));
    if (adapt) {
        const float g = __fdiv_rn(__fmul_rn(mu, e), __fadd_rn(dot_end(p), eps));
        r = r0;
        for (uint32_t k = 0; k < T; k += 4) {
            float wv[4], uv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                wv[j] = wc[min(k + j, T - 1) * N];
                uv[j] = col[ring_at(r, n8)];
                r = r ? r - 1 : R - 1;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (k + j < T) wc[(k + j) * N] = __fadd_rn(wv[j], __fmul_rn(g, uv[j]));
        }
    }
    return e;
}

// the fast body: every whole block of FB frames of the run, for a wave whose present lanes all carry Tw taps, Tw <= TP (FULL:
// Tw == TP).  win[j] is the reference sample of frame f - D - (TP - 1) + j, f the block's first frame: frame i meets tap k at
// win[i + TP - 1 - k].  A lane without a node computes on zeros and keeps its microphone sample.  any_adapt (wave-uniform): a lane
// of the wave adapts; a frozen wave does neither dot(u, u) nor the update.  -> the frames done; row stands behind them
template <int TP, bool FULL>
__device__ __forceinline__ uint32_t cancel_fast(const CancelArgs &a, const float *lmic, const float *lref, float *lout, size_t rs, float *wc, float *col,
                                                uint32_t Tw, bool present, bool adapt, bool any_adapt, float mu, float eps, uint32_t D, uint32_t &row,
                                                float &sd, float &se) {
    const size_t N = a.N, n8 = (size_t)RG * a.N;
    const uint32_t R = a.R;
    float w[TP], win[TP + FB - 1], sq[SQ ? TP + FB - 1 : 1];
#pragma unroll
    for (int k = 0; k < TP; ++k) w[k] = (FULL || (uint32_t)k < Tw) && present ? wc[k * N] : 0.0f;
    uint32_t rd = rows_back(row, D, R);                            // the ring row of the block's first u[0]
#pragma unroll
    for (int j = 0; j < TP - 1; ++j)                               // the history: TP - 1 - j rows behind it, Tw - 1 at the most
        win[j] = (FULL || (uint32_t)j + Tw >= (uint32_t)TP) && present ? col[ring_at(rows_back(rd, TP - 1 - j, R), n8)] : 0.0f;
    if constexpr (SQ) {
#pragma unroll
        for (int j = 0; j < TP - 1; ++j) sq[j] = __fmul_rn(win[j], win[j]);
    }
    uint32_t f = 0;
#pragma unroll 1
    for (; f + FB <= a.nf; f += FB) {
        float d[FB], x[FB], o[FB];
#pragma unroll
        for (int i = 0; i < FB; ++i) {
            d[i] = lmic[(f + i) * rs];
            x[i] = present ? lref[(f + i) * rs] : 0.0f;
        }
        {
            uint32_t r = row;
            if (FB % RG == 0 && row % RG == 0) {                   // (wave-uniform; R is a multiple of RG) whole groups: 16-byte stores
                if (present) {
#pragma unroll
                    for (int i = 0; i < FB; i += 4) {
                        const f32x4 v = {x[i], x[i + 1], x[i + 2], x[i + 3]};
                        *(f32x4 *)(col + ring_at(row + i, n8)) = v;
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < FB; ++i) {
                    if (present) col[ring_at(r, n8)] = x[i];
                    r = row_next(r, R);
                }
            }
            r = rd;
#pragma unroll
            for (int i = 0; i < FB; ++i) {
                win[TP - 1 + i] = present ? col[ring_at(r, n8)] : 0.0f;
                r = row_next(r, R);
            }
            if constexpr (SQ) {
#pragma unroll
                for (int i = 0; i < FB; ++i) sq[TP - 1 + i] = __fmul_rn(win[TP - 1 + i], win[TP - 1 + i]);
            }
            rd = r;
            row += FB;
            if (row >= R) row -= R;
        }
#pragma unroll
        for (int i = 0; i < FB; ++i) {
            float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < TP; ++k) {
                const float sk = __fadd_rn(s[k & 3], __fmul_rn(w[k], win[i + TP - 1 - k]));
                s[k & 3] = FULL || (uint32_t)k < Tw ? sk : s[k & 3];
            }
            const float e = __fsub_rn(d[i], dot_end(s));
            sd = __fadd_rn(sd, __fmul_rn(d[i], d[i]));
            se = __fadd_rn(se, __fmul_rn(e, e));
            o[i] = present ? e : d[i];
            if (any_adapt) {
                float p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int k = 0; k < TP; ++k) {
                    const float u = win[i + TP - 1 - k];
                    const float pk = __fadd_rn(p[k & 3], SQ ? sq[SQ ? i + TP - 1 - k : 0] : __fmul_rn(u, u));
                    p[k & 3] = FULL || (uint32_t)k < Tw ? pk : p[k & 3];
                }
                const float g = __fdiv_rn(__fmul_rn(mu, e), __fadd_rn(dot_end(p), eps));
#pragma unroll
                for (int k = 0; k < TP; ++k) {
                    const float nw = __fadd_rn(w[k], __fmul_rn(g, win[i + TP - 1 - k]));
                    w[k] = adapt && (FULL || (uint32_t)k < Tw) ? nw : w[k];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < FB; ++i) __builtin_nontemporal_store(o[i], lout + (f + i) * rs);
#pragma unroll
        for (int j = 0; j < TP - 1; ++j) win[j] = win[j + FB];
        if constexpr (SQ) {
#pragma unroll
            for (int j = 0; j < TP - 1; ++j) sq[j] = sq[j + FB];
        }
    }
    if (any_adapt && present) {
#pragma unroll
        for (int k = 0; k < TP; ++k)
            if (FULL || (uint32_t)k < Tw) wc[k * N] = w[k];
    }
    return f;
}

// MAXTP: the largest class of the fast body this instance holds (0: none) -- the host launches the instance of the longest filter
// the bank carries, so a bank of short filters does not pay the registers of the 64-tap window
template <int MAXTP>
__global__ __launch_bounds__(CWG) void cancel_run(CancelArgs a) {
    uint32_t c;
    if (!lane_channel<1>(CWG, a.N, c)) return;
    const size_t N = a.N, rs = a.W ? a.W : a.N;
    const size_t lane0 = lay(0, c, a.nf, a.N, a.W);
    const float *lmic = a.mic + lane0;
    float *lout = a.out + lane0;
    const uint32_t tn = a.tn[c], T = tn & CN_T;
    const bool present = T != 0, adapt = present && (tn & CN_ADAPT);
    const unsigned long long nodes = __ballot(present);            // (the lanes that returned above are not asked)
    if (!nodes) {                                                  // a wave without a node: the sample's own bits, levels +0.0
        a.lev[c] = 0.0f;
        a.lev[N + c] = 0.0f;
        if (a.mic == a.out) return;
        uint32_t f = 0;
#pragma unroll 1
        for (; f + 8 <= a.nf; f += 8) {                            // eight loads ahead of their stores
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = lmic[(f + i) * rs];
#pragma unroll
            for (int i = 0; i < 8; ++i) __builtin_nontemporal_store(v[i], lout + (f + i) * rs);
        }
        for (; f < a.nf; ++f) __builtin_nontemporal_store(lmic[f * rs], lout + f * rs);
        return;
    }
    const float *lref = a.ref + lane0;                             // (a lane without a node never reads through it)
    float mu = 0.0f, eps = 0.0f;
    uint32_t D = 0;
    if (present) {
        mu = a.mu[c];
        eps = a.eps[c];
        D = a.dl[c];
    }
    float *wc = a.w + c, *col = a.ring + (size_t)RG * c;
    const size_t n8 = (size_t)RG * a.N;
    const uint32_t R = a.R;
    uint32_t row = a.row, f = 0;
    float sd = 0.0f, se = 0.0f;

    const uint32_t Tw = __builtin_amdgcn_readfirstlane(__shfl(T, (int)__builtin_ctzll(nodes)));    // the T of the wave's first node
    const bool shared = !__ballot(present && T != Tw);
    if (MAXTP > 0 && shared && Tw <= (uint32_t)MAXTP && a.nf >= (uint32_t)FB) {
        const bool any = __ballot(adapt) != 0;
#define CANCEL_FAST(TP)                                                                                                                 \
    f = Tw == TP ? cancel_fast<TP, true>(a, lmic, lref, lout, rs, wc, col, Tw, present, adapt, any, mu, eps, D, row, sd, se) \
                 : cancel_fast<TP, false>(a, lmic, lref, lout, rs, wc, col, Tw, present, adapt, any, mu, eps, D, row, sd, se)
        if constexpr (MAXTP >= 8) {
            if (Tw <= 8) CANCEL_FAST(8);
        }
        if constexpr (MAXTP >= 16) {
            if (Tw > 8 && Tw <= 16) CANCEL_FAST(16);
        }
        if constexpr (MAXTP >= 32) {
            if (Tw > 16 && Tw <= 32) CANCEL_FAST(32);
        }
        if constexpr (MAXTP >= 64) {
            if (Tw > 32) CANCEL_FAST(64);
        }
#undef CANCEL_FAST
    }
    // the general body: one frame at a time
    uint32_t rd = rows_back(row, D, R);
#pragma unroll 1
    for (; f < a.nf; ++f) {
        const float d = lmic[f * rs];
        float y = d;
        if (present) {
            col[ring_at(row, n8)] = lref[f * rs];
            y = cancel_frame(wc, col, N, n8, R, T, adapt, mu, eps, rd, d);
            sd = __fadd_rn(sd, __fmul_rn(d, d));
            se = __fadd_rn(se, __fmul_rn(y, y));
        }
        __builtin_nontemporal_store(y, lout + f * rs);
        row = row_next(row, R);
        rd = row_next(rd, R);
    }
    a.lev[c] = present ? sd : 0.0f;
    a.lev[N + c] = present ? se : 0.0f;
}

enum StoreKind : uint32_t { ST_SET, ST_LOAD, ST_DROP, ST_RESET };

// a set, a drop, a reset over channels [first, first + count), in stream order, one thread per channel (the threads of a wave write
// one row of 64 channels in one access).  SET: vals is five runs of [count] words in page-locked memory -- the node word, the
// delay, mu's and eps' bits, and what to clear: the column of a new node, the rows [T, the T it had) of a node made shorter.
// DROP: no node, the weights +0.0.  RESET: the weights and the column +0.0
__global__ __launch_bounds__(CWG) void cancel_node(float *__restrict__ w, float *__restrict__ ring, uint32_t *__restrict__ tn, uint32_t *__restrict__ dl,
                                                   float *__restrict__ mu, float *__restrict__ eps, const uint32_t *__restrict__ vals, uint32_t N, uint32_t R,
                                                   uint32_t max_taps, uint32_t first, uint32_t count, uint32_t kind) {
    const uint32_t i = blockIdx.x * CWG + threadIdx.x;
    if (i >= count) return;
    const size_t c = (size_t)first + i, n = N;
    uint32_t k0 = 0, k1 = max_taps;
    bool column = kind == ST_RESET;
    if (kind == ST_SET) {
        const uint32_t word = vals[i], clear = vals[4 * (size_t)count + i];
        tn[c] = word;
        dl[c] = vals[(size_t)count + i];
        mu[c] = __uint_as_float(vals[2 * (size_t)count + i]);
        eps[c] = __uint_as_float(vals[3 * (size_t)count + i]);
        k0 = word & CN_T;
        k1 = min(clear & CN_T, max_taps);
        column = clear & CW_FRESH;
    } else if (kind == ST_DROP) {
        tn[c] = 0;
    }
    for (uint32_t k = k0; k < k1; ++k) w[k * n + c] = 0.0f;
    if (column)
        for (uint32_t r = 0; r < R; ++r) ring[RG * c + ring_at(r, RG * n)] = 0.0f;
}

// a load, in stream order: rows[i * stride + k] is weight k of channel first + i (stride 0: one row for the range) -> w[k][c]
__global__ __launch_bounds__(CWG) void cancel_load(float *__restrict__ w, const float *__restrict__ rows, uint32_t N, uint32_t first, uint32_t count,
                                                   uint32_t T, uint32_t stride) {
    const uint64_t total = (uint64_t)count * T;
    for (uint64_t e = (uint64_t)blockIdx.x * CWG + threadIdx.x; e < total; e += (uint64_t)gridDim.x * CWG) {
        uint32_t i, k;
        if (stride) {
            i = (uint32_t)(e / T);
            k = (uint32_t)(e % T);
        } else {
            k = (uint32_t)(e / count);
            i = (uint32_t)(e % count);
        }
        w[(size_t)k * N + first + i] = rows[(size_t)i * stride + k];
    }
}

thread_local std::string g_err;        // the reason of the last failed create or plan on this thread

// a store's vals: SET five runs of [count] words (cancel_node); LOAD T floats (per_channel 0) or count x T; the others carry none
struct StoreFields {
    StoreKind kind = ST_RESET;
    uint32_t first = 0, count = 0;
    uint32_t T = 0, per_channel = 0;
};
typedef StoreQueue<StoreFields> Stores;
typedef Stores::Store Store;

int check_sizes(uint32_t max_taps, uint32_t max_delay, std::string &err) {
    char buf[128];
    if (max_taps < 1 || max_taps > DSPFX_CANCEL_MAX_TAPS) {
        std::snprintf(buf, sizeof buf, "cancel: max_taps is %u, not 1 .. %u", max_taps, (unsigned)DSPFX_CANCEL_MAX_TAPS);
        err = buf;
        return DSPFX_ERR_INVALID;
    }
    if (max_delay > DSPFX_CANCEL_MAX_DELAY) {
        std::snprintf(buf, sizeof buf, "cancel: max_delay is %u, not 0 .. %u", max_delay, (unsigned)DSPFX_CANCEL_MAX_DELAY);
        err = buf;
        return DSPFX_ERR_INVALID;
    }
    return DSPFX_OK;
}

// the class of the fast body a node of T taps runs in (4: none, the general body)
int tap_class(uint32_t T) { return T <= 8 ? 0 : T <= 16 ? 1 : T <= 32 ? 2 : T <= FAST_MAX_T ? 3 : 4; }

uint32_t f32_bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

}  // namespace

struct dspfx_cancel : ChannelBank<dspfx_cancel_desc, StoreFields> {
    static constexpr const char *name = "cancel";
    // the host tables, as every store made so far left them: T (0: no node), the delay, mu, eps, adapt
    std::vector<uint16_t> hT;
    std::vector<uint32_t> hD;
    std::vector<float> hmu, heps;
    std::vector<uint8_t> hadapt;
    uint64_t classes[5] = {0, 0, 0, 0, 0};       // the nodes of T <= 8, <= 16, <= 32, <= 64 and above (the queue's qmu)
    uint32_t row = 0;                            // the ring row of the next run's first frame (mu)
    float *w = nullptr, *ring = nullptr, *dmu = nullptr, *deps = nullptr, *lev = nullptr;
    uint32_t *tn = nullptr, *dl = nullptr;
    static uint32_t ring_rows(const dspfx_cancel_desc &d) { return (d.max_delay + d.max_taps + RING_PAD + RG - 1) / RG * RG; }
    // the fresh state: no node anywhere, every weight +0.0.  The ring is never cleared as a whole: a store that makes a node clears
    // its column
    template <class V>
    static void tables(const dspfx_cancel_desc &d, V v) {
        const uint64_t N = d.n_channels;
        v(4 * N * d.max_taps, 0, &dspfx_cancel::w);
        v(4 * N * ring_rows(d), TABLE_BY_HAND, &dspfx_cancel::ring);
        v(4 * N, 0, &dspfx_cancel::tn);
        v(4 * N, 0, &dspfx_cancel::dl);
        v(4 * N, 0, &dspfx_cancel::dmu);
        v(4 * N, 0, &dspfx_cancel::deps);
        v(8 * N, 0, &dspfx_cancel::lev);
    }
};

namespace {

// one store onto the stream
hipError_t apply_store(dspfx_cancel *p, const Store &st, hipStream_t s) {
    const uint32_t N = p->desc.n_channels;
    const void *vals = nullptr;
    if (st.vals) {
        const hipError_t err = hipHostGetDevicePointer((void **)&vals, st.vals, 0);
        if (err != hipSuccess) return err;
    }
    if (st.kind == ST_LOAD) {
        const uint64_t total = (uint64_t)st.count * st.T;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + CWG - 1) / CWG, 1u << 20);
        cancel_load<<<blocks, CWG, 0, s>>>(p->w, (const float *)vals, N, st.first, st.count, st.T, st.per_channel ? st.T : 0);
    } else {
        cancel_node<<<(st.count + CWG - 1) / CWG, CWG, 0, s>>>(p->w, p->ring, p->tn, p->dl, p->dmu, p->deps, (const uint32_t *)vals, N,
                                                              dspfx_cancel::ring_rows(p->desc), p->desc.max_taps, st.first, st.count, st.kind);
    }
    return hipGetLastError();
}

}  // namespace

extern "C" const char *dspfx_cancel_last_error(const dspfx_cancel *p) { return p ? p->err.c_str() : g_err.c_str(); }

extern "C" int dspfx_cancel_plan(uint64_t channels, uint32_t max_taps, uint32_t max_delay, uint64_t *bytes_out) {
    return plan_bank<dspfx_cancel>(channels, bytes_out, g_err, [=](dspfx_cancel_desc &d, std::string &err) {
        d.max_taps = max_taps;
        d.max_delay = max_delay;
        return check_sizes(max_taps, max_delay, err);
    });
}

extern "C" int dspfx_cancel_create(const dspfx_cancel_desc *desc, dspfx_cancel **out) {
    const int rc = create_checks(desc, out, g_err, [desc](std::string &err) { return check_sizes(desc->max_taps, desc->max_delay, err); });
    if (rc != DSPFX_OK) return rc;
    return create_bank(desc, out, g_err, [](dspfx_cancel *p) {
        const size_t N = p->desc.n_channels;
        p->hT.assign(N, 0);
        p->hD.assign(N, 0);
        p->hmu.assign(N, 0.0f);
        p->heps.assign(N, 0.0f);
        p->hadapt.assign(N, 0);
    });
}

extern "C" int dspfx_cancel_destroy(dspfx_cancel *p) { return destroy_bank(p); }

extern "C" int dspfx_cancel_set(dspfx_cancel *p, const uint32_t *host_taps, const float *host_mu, const float *host_eps, const uint32_t *host_delay,
                                const uint32_t *host_adapt, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_range(p, "set", first_channel, count);
    if (rc != DSPFX_OK) return rc;
    char buf[160];
    for (uint64_t i = 0; i < count; ++i) {
        if (host_taps && (host_taps[i] == 0 || host_taps[i] > p->desc.max_taps)) {
            std::snprintf(buf, sizeof buf, "cancel set: channel %llu is given %u taps, not 1 .. max_taps = %u", (unsigned long long)(first_channel + i),
                          host_taps[i], p->desc.max_taps);
            return p->fail(DSPFX_ERR_INVALID, buf);
        }
        if (host_delay && host_delay[i] > p->desc.max_delay) {
            std::snprintf(buf, sizeof buf, "cancel set: channel %llu is given a delay of %u, above max_delay = %u", (unsigned long long)(first_channel + i),
                          host_delay[i], p->desc.max_delay);
            return p->fail(DSPFX_ERR_INVALID, buf);
        }
    }
    if (count == 0) return DSPFX_OK;
    Store st;
    std::unique_lock<std::mutex> one;
    if (!stage_store(p, st, &one, ST_SET, "set", first_channel, count, 5 * count, "staged node words")) return DSPFX_ERR_OOM;
    uint32_t *word = (uint32_t *)st.vals, *dly = word + count, *mub = dly + count, *epb = mub + count, *clear = epb + count;
    for (uint64_t i = 0; i < count; ++i) {
        const size_t c = first_channel + i;
        const bool fresh = p->hT[c] == 0;                          // a new node: mu 0.5, eps 1e-6, delay 0, adapting, max_taps taps
        const uint32_t T = host_taps ? host_taps[i] : fresh ? p->desc.max_taps : p->hT[c];
        const bool ad = host_adapt ? host_adapt[i] != 0 : fresh ? true : p->hadapt[c] != 0;
        word[i] = T | (ad ? CN_ADAPT : 0u);
        dly[i] = host_delay ? host_delay[i] : fresh ? 0u : p->hD[c];
        mub[i] = f32_bits(host_mu ? host_mu[i] : fresh ? 0.5f : p->hmu[c]);
        epb[i] = f32_bits(host_eps ? host_eps[i] : fresh ? 1e-6f : p->heps[c]);
        clear[i] = p->hT[c] | (fresh ? CW_FRESH : 0u);
    }
    p->stores.push(st, [&] {
        for (uint64_t i = 0; i < count; ++i) {
            const size_t c = first_channel + i;
            if (p->hT[c]) --p->classes[tap_class(p->hT[c])];
            p->hT[c] = (uint16_t)(word[i] & CN_T);
            ++p->classes[tap_class(p->hT[c])];
            p->hadapt[c] = (word[i] & CN_ADAPT) != 0;
            p->hD[c] = dly[i];
            std::memcpy(&p->hmu[c], &mub[i], sizeof(float));
            std::memcpy(&p->heps[c], &epb[i], sizeof(float));
        }
    });
    return DSPFX_OK;
}

extern "C" int dspfx_cancel_load(dspfx_cancel *p, const float *host_rows, uint32_t n_taps, uint32_t per_channel, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    if (!host_rows) return p->fail(DSPFX_ERR_INVALID, "cancel load: no rows");
    const int rc = check_range(p, "load", first_channel, count);
    if (rc != DSPFX_OK) return rc;
    if (count == 0) return DSPFX_OK;
    std::unique_lock<std::mutex> one(p->smu);                      // the nodes' T must not change between the check and the push
    for (uint64_t i = 0; i < count; ++i) {
        const uint32_t T = p->hT[first_channel + i];
        if (T == n_taps && T != 0) continue;
        char buf[160];
        if (T) std::snprintf(buf, sizeof buf, "cancel load: channel %llu carries %u taps and is given %u", (unsigned long long)(first_channel + i), T, n_taps);
        else std::snprintf(buf, sizeof buf, "cancel load: channel %llu carries no node", (unsigned long long)(first_channel + i));
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    const uint64_t n = per_channel ? count * n_taps : n_taps;
    Store st;
    st.T = n_taps;
    st.per_channel = per_channel ? 1 : 0;
    if (!stage_store(p, st, nullptr, ST_LOAD, "load", first_channel, count, n, "staged weights")) return DSPFX_ERR_OOM;
    std::memcpy(st.vals, host_rows, n * sizeof(float));
    p->stores.push(st);
    return DSPFX_OK;
}

extern "C" int dspfx_cancel_drop(dspfx_cancel *p, uint64_t first_channel, uint64_t count) {
    return store_plain(p, ST_DROP, "drop", first_channel, count, [=] {
        for (uint64_t c = first_channel; c < first_channel + count; ++c) {
            if (p->hT[c]) --p->classes[tap_class(p->hT[c])];
            p->hT[c] = 0;
            p->hD[c] = 0;
            p->hmu[c] = p->heps[c] = 0.0f;
            p->hadapt[c] = 0;
        }
    });
}

extern "C" int dspfx_cancel_reset(dspfx_cancel *p, uint64_t first_channel, uint64_t count) { return store_plain(p, ST_RESET, "reset", first_channel, count); }

extern "C" int dspfx_cancel_present(dspfx_cancel *p, uint32_t *host_present_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "present", host_present_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = p->hT[c] != 0; });
}

extern "C" int dspfx_cancel_lengths(dspfx_cancel *p, uint32_t *host_lengths_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "lengths", host_lengths_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = p->hT[c]; });
}

extern "C" int dspfx_cancel_sliders(dspfx_cancel *p, float *host_sliders_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "sliders", host_sliders_out, first_channel, count, [p](float *o, uint64_t i, uint64_t c) {
        o[2 * i] = p->hmu[c];
        o[2 * i + 1] = p->heps[c];
    });
}

extern "C" int dspfx_cancel_delays(dspfx_cancel *p, uint32_t *host_delays_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "delays", host_delays_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = p->hD[c]; });
}

extern "C" int dspfx_cancel_adapting(dspfx_cancel *p, uint32_t *host_adapting_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "adapting", host_adapting_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = p->hadapt[c]; });
}

extern "C" int dspfx_cancel_weights_view(dspfx_cancel *p, const float **weights_out) {
    if (!p) return DSPFX_ERR_INVALID;
    if (weights_out) *weights_out = p->w;
    return DSPFX_OK;
}

extern "C" int dspfx_cancel_levels_view(dspfx_cancel *p, const float **levels_out) {
    if (!p) return DSPFX_ERR_INVALID;
    if (levels_out) *levels_out = p->lev;
    return DSPFX_OK;
}

extern "C" int dspfx_cancel_run(dspfx_cancel *p, const float *mic, const float *ref, float *out, uint32_t n_frames, void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    if (mic && out && !ref) return p->fail(DSPFX_ERR_INVALID, "cancel run: no ref (the block the channel was sent)");
    if (ref && out && n_frames && n_frames <= p->desc.max_frames) {
        const uintptr_t bytes = (uintptr_t)n_frames * p->desc.n_channels * sizeof(float), o = (uintptr_t)out, r = (uintptr_t)ref;
        if (o < r + bytes && r < o + bytes) return p->fail(DSPFX_ERR_INVALID, "cancel run: out overlaps ref (out may be mic, never ref)");
    }
    hipStream_t s = (hipStream_t)stream;
    const int rc = begin_run(p, mic && out, n_frames, s, "cancel run: mic, out or n_frames", "cancel store", apply_store);
    if (rc != DSPFX_OK) return rc;
    CancelArgs a;
    a.mic = mic;
    a.ref = ref;
    a.out = out;
    a.w = p->w;
    a.ring = p->ring;
    a.tn = p->tn;
    a.dl = p->dl;
    a.mu = p->dmu;
    a.eps = p->deps;
    a.lev = p->lev;
    a.N = p->desc.n_channels;
    a.W = p->desc.tile_channels;
    a.nf = n_frames;
    a.R = dspfx_cancel::ring_rows(p->desc);
    a.row = p->row;
    // the instance of the longest filter the bank carries, as the stores made so far left it (a store that joins behind this run's
    // drain can only make the kernel meet a wave whose T is above its class: that wave takes the general body)
    int cls = -1;
    {
        std::lock_guard<std::mutex> qk(p->stores.qmu);
        for (int i = 0; i < 5; ++i)
            if (p->classes[i]) cls = std::min(i, 3);
    }
    if (p->desc.general_only) cls = -1;
    const uint32_t blocks = lane_blocks(a.N, 1, CWG);
    switch (cls) {
    case 0: cancel_run<8><<<blocks, CWG, 0, s>>>(a); break;
    case 1: cancel_run<16><<<blocks, CWG, 0, s>>>(a); break;
    case 2: cancel_run<32><<<blocks, CWG, 0, s>>>(a); break;
    case 3: cancel_run<64><<<blocks, CWG, 0, s>>>(a); break;
    default: cancel_run<0><<<blocks, CWG, 0, s>>>(a); break;
    }
    BANK_HIP_WHY(hipGetLastError(), "cancel_run");
    p->row = (uint32_t)((p->row + (uint64_t)n_frames) % a.R);
    return DSPFX_OK;
}
