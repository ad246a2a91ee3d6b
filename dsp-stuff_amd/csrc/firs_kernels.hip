// firs_kernels.hip -- the channel-FIR bank (include/dspfx.h, dspfx_firs_*): channel c carries no node or ONE FIR node of its own
// (nodes/fir.rs) with its own taps, tap count T (1 .. max_taps), mode and VecDeque.  A channel without a node copies.
//
// The arithmetic is fir.rs:179-225 as fir_exact_kernel (fir_kernels.hip) has it for one shared tap table, here with everything per
// lane (a lane is a channel): per sample push, pop ONE sample when the deque is longer than T, then
//   a = (float) sum_{k < min(n_a, T)} state[k] * taps[k]                        sequential f64, the product rounded before the addition
//   b = (float) sum_{k < min(len - n_a, T - n_a)} state[n_a + k] * taps[n_a + k]       (0 when n_a >= T)
//   out = (a + b) * divisor                                                     divisor 1 or 1.0f / (float)T
// where n_a is the length of the deque's first physical slice.  The three deque words len, cap, head live on the device and the
// kernel steps them per frame (deque_step, as fir_kernels.hip's on the host), so the host keeps no clock per channel.  Only the
// indices of the VecDeque are modelled; the samples are in a ring in TIME, [R][N] floats, R = max_taps + FB rows: the sample of the bank's frame n is row n mod R for every channel (the host carries the one row counter), and the deque
// of a lane is the newest `len` rows.  A lane writes a frame's sample into the ring before it reads any, and reads the block
// only at that frame, so out may be in.
//
// Two bodies in one kernel, chosen by one ballot per block of frames.  GENERAL (fir_frame): one frame, the two sums as written
// above, correct in the fill phase, for a deque longer than its taps and for lanes of different T in one wave (the loops run
// under the lane's own bounds, four terms' loads issued together).  STEADY: a wave whose present lanes ALL stand at len == T < cap
// (no growth and one pop per frame from here on) with the same T takes the next FB = 16 frames at once: the taps are streamed
// once per block in the outer loop (G = 8 of them and the 8 new samples loaded together, ahead of the arithmetic), the samples
// slide through a register window (each widened to f64 once per block) and every frame keeps ONE running f64 sum; where a
// frame's first slice ends (k == n_a) the sum is rounded into the frame's `a` and restarts at +0.0 -- under a wave-uniform
// branch, so a wave pays the selects only at taps where one of its lanes has a slice end.  The sums are the reference's own, in
// its order; no term is replaced by zero.  Measured at 2^20 channels x 128 frames, T = 32: 0.89 ms, the
// general body forced 6.8 ms; blocks of 8 frames took 1.21 ms (the taps and the window are re-read per block: at 8 frames 7.5 KB
// per channel and run cross the caches, at 16 frames 5), two accumulators per frame under per-term selects 1.24 ms, and a tap's
// load waited for at every step 1.51 ms.  A wave without a node copies (in place: does nothing).  Nothing is shared between
// channels: no LDS, no atomics.
//
// Stores go through the staged-store queue (store_queue.hip.h).  The taps are staged as doubles in page-locked memory -- T of them
// for one response over a range, count x T for a response per channel -- and a kernel on the run's stream reads them there and
// writes them REVERSED (fir.rs:163,168) into the table's [tap][N] layout; its thread of tap 0 also makes the node: a channel
// that carried none gets an empty deque (a new node), one that carried one keeps its deque (the reload, fir.rs:153-171).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dspfx.h"
#include "channel_bank.hip.h"
#include "lane_io.hip.h"

namespace {

constexpr uint32_t FWG = 256;
constexpr int FB = 16;                           // frames per block of the steady body; the ring has max_taps + FB rows
constexpr int G = 8;                             // taps whose loads are issued together

// the node word of a channel: T in the low 16 bits (0: no node), the mode above
constexpr uint32_t TN_T = 0xFFFFu, TN_AVERAGE = 1u << 16;

struct FirsArgs {
    const float *in;             // may be `out`: no __restrict__
    float *out;
    const double *taps;          // [max_taps][N], reversed
    float *ring;                 // [R][N]
    const uint32_t *tn;          // [N]
    int32_t *dq;                 // [3][N]: len, cap, head
    uint32_t N, W, nf, R;
    uint32_t row;                // the ring row of the run's first frame
    uint32_t general_only;
};

struct Deque {
    uint32_t len, cap, head;
};

// one push_back and at most one pop_front on the indices of std VecDeque<f64> (fir_kernels.hip, deque_step): -> n_a, the length
// of the first physical slice after the step
__device__ __forceinline__ uint32_t deque_step(Deque &d, uint32_t T) {
    if (d.len == d.cap) {
        const uint32_t old = d.cap, ncap = old ? old * 2 : 4;
        if (d.head > old - d.len) {                                // wrapped (len == old: any head != 0)
            const uint32_t head_len = old - d.head, tail_len = d.len - head_len;
            if (!(head_len > tail_len && ncap - old >= tail_len)) d.head = ncap - head_len;
        }
        d.cap = ncap;
    }
    ++d.len;
    if (d.len > T) {
        d.head = d.head + 1 == d.cap ? 0 : d.head + 1;
        --d.len;
    }
    return min(d.len, d.cap - d.head);
}

// n terms of one slice's sum: samples from ring row r on, taps from k0 on, sequential.  U terms' loads are issued together (a row
// past the slice is a row of the ring and is not used; a tap past it is read at the last tap's place); r moves n rows on
template <int U>
__device__ __forceinline__ double fir_slice(const float *col, const double *tp, size_t N, uint32_t R, uint32_t &r, uint32_t k0, uint32_t n, uint32_t T) {
    double acc = 0.0;
    uint32_t rr = r;
    for (uint32_t k = 0; k < n; k += U) {
        float s[U];
        double t[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            s[j] = col[rr * N];
            rr = rr + 1 == R ? 0 : rr + 1;
            t[j] = tp[min(k0 + k + j, T - 1) * N];
        }
#pragma unroll
        for (int j = 0; j < U; ++j)
            if (k + j < n) acc = __dadd_rn(acc, __dmul_rn((double)s[j], t[j]));
    }
    r += n;
    if (r >= R) r -= R;
    return acc;
}

// the general body: one frame of one lane whose sample is already in ring row `row`.  col, tp: the lane's column of the ring and
// of the taps.  The deque's element k is row (row - (len - 1) + k) mod R; len <= max_taps < R
__device__ __forceinline__ float fir_frame(const float *col, const double *tp, size_t N, uint32_t R, Deque &d, uint32_t T, float div, uint32_t row) {
    const uint32_t na = deque_step(d, T);
    const uint32_t la = min(na, T);
    const uint32_t lb = na < T ? min(d.len - na, T - na) : 0;
    uint32_t r = row + R - d.len + 1;
    if (r >= R) r -= R;
    const float fa = (float)fir_slice<4>(col, tp, N, R, r, 0, la, T);
    const float fb = (float)fir_slice<4>(col, tp, N, R, r, na, lb, T);          // (lb != 0 only with la == na: r stands at element n_a)
    return __fmul_rn(__fadd_rn(fa, fb), div);                      // fir.rs:216,222
}

// one tap of the steady body: frame i of the block meets tap k at the window's sample i + k, kept in w[(i + kk) % F] (kk = k % F).
// S[i] is the running sum of the slice the frame stands in: at k == n_a its first slice ends, the sum is rounded into fa[i] and the
// second slice's sum starts at +0.0.  near (wave-uniform): a lane of the wave has a slice end at this tap in a frame of the block;
// a wave without one does the multiplication and the addition alone
template <int F>
__device__ __forceinline__ void fir_step(const double (&w)[F], int kk, double t, uint32_t k, const uint32_t (&na)[F], bool near, double (&S)[F],
                                         float (&fa)[F]) {
    if (near) {
#pragma unroll
        for (int i = 0; i < F; ++i) {
            const bool cut = k == na[i];
            fa[i] = cut ? (float)S[i] : fa[i];
            S[i] = cut ? 0.0 : S[i];
        }
    }
#pragma unroll
    for (int i = 0; i < F; ++i) S[i] = __dadd_rn(S[i], __dmul_rn(w[(i + kk) % F], t));
}

// 250 VGPRs, no scratch, no LDS: 2 waves per SIMD (gfx950, -O3); with blocks of 8 frames 126 VGPRs and 4 waves, and slower
__global__ __launch_bounds__(FWG) void firs_run(FirsArgs a) {
    uint32_t c;
    if (!lane_channel<1>(FWG, a.N, c)) return;
    const size_t N = a.N, rs = a.W ? a.W : a.N;
    const size_t lane0 = lay(0, c, a.nf, a.N, a.W);
    const float *lin = a.in + lane0;
    float *lout = a.out + lane0;
    const uint32_t tn = a.tn[c], T = tn & TN_T;
    const bool present = T != 0;
    const unsigned long long nodes = __ballot(present);           // (the lanes that returned above are not asked)
    if (!nodes) {                                                  // a wave without a node: the sample's own bits
        if (a.in == a.out) return;
        uint32_t f = 0;
#pragma unroll 1
        for (; f + 8 <= a.nf; f += 8) {                            // eight loads ahead of their stores
            float v[1][8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[0][i] = lin[(f + i) * rs];
#pragma unroll
            for (int i = 0; i < 8; ++i) __builtin_nontemporal_store(v[0][i], lout + (f + i) * rs);
        }
        for (; f < a.nf; ++f) __builtin_nontemporal_store(lin[f * rs], lout + f * rs);
        return;
    }
    Deque d{0, 0, 0};
    if (present) {
        d.len = (uint32_t)a.dq[c];
        d.cap = (uint32_t)a.dq[N + c];
        d.head = (uint32_t)a.dq[2 * N + c];
    }
    const float div = (tn & TN_AVERAGE) ? __fdiv_rn(1.0f, (float)T) : 1.0f;                   // fir.rs:187-190
    float *col = a.ring + c;
    const double *tp = a.taps + c;
    const uint32_t R = a.R;
    uint32_t row = a.row, f = 0;

    const uint32_t Tw = __builtin_amdgcn_readfirstlane(__shfl(T, (int)__builtin_ctzll(nodes)));    // the T of the wave's first node
#pragma unroll 1
    while (f < a.nf) {
        // the steady body, decided block by block (a new node leaves the general body FB frames or fewer after its deque is full):
        // every present lane of the wave at len == T < cap with the same T
        const bool steady = !present || (d.len == T && d.cap > T && T == Tw);
        if (!a.general_only && f + FB <= a.nf && !__ballot(!steady)) {
            Deque e = present ? d : Deque{Tw, Tw + 1, 0};          // (a lane without a node computes on, and keeps its sample)
            float x[FB];
#pragma unroll
            for (int i = 0; i < FB; ++i) x[i] = lin[(f + i) * rs];
            uint32_t na[FB], lo = Tw, hi = 0;                        // the lane's slice ends lie at taps lo .. hi (none: lo > hi)
            {
                uint32_t r = row;
#pragma unroll
                for (int i = 0; i < FB; ++i) {
                    if (present) col[r * N] = x[i];
                    r = r + 1 == R ? 0 : r + 1;
                    e.head = e.head + 1 == e.cap ? 0 : e.head + 1;                             // deque_step at len == T < cap
                    na[i] = min(Tw, e.cap - e.head);
                    lo = min(lo, na[i]);
                    if (na[i] < Tw) hi = max(hi, na[i]);
                }
            }
            // window[j] is the sample of frame f + j - (T - 1): row (row + j - (T - 1)) mod R; frame i meets tap k at window[i + k],
            // kept in w[(i + k) % FB]
            uint32_t r = row + R - Tw + 1;
            if (r >= R) r -= R;
            double w[FB], S[FB];
            float fa[FB];
#pragma unroll
            for (int i = 0; i < FB; ++i) {
                S[i] = 0.0;
                fa[i] = 0.0f;
            }
#pragma unroll
            for (int j = 0; j < FB - 1; ++j) {
                w[j] = (double)col[r * N];
                r = r + 1 == R ? 0 : r + 1;
            }
            // G taps at a time, their loads and the G new samples' issued together ahead of the arithmetic (one tap per step
            // waited for its own load at every step); a last group of fewer than G taps goes one tap at a time
#pragma unroll 1
            for (uint32_t k0 = 0; k0 < Tw; k0 += FB) {
#pragma unroll
                for (int h = 0; h < FB / G; ++h) {
                    const uint32_t kb = k0 + h * G;
                    if (kb >= Tw) break;                            // wave-uniform, as every branch on k
                    if (kb + G <= Tw) {
                        double t[G];
                        float s[G];
#pragma unroll
                        for (int g = 0; g < G; ++g) {
                            s[g] = col[r * N];
                            r = r + 1 == R ? 0 : r + 1;
                            t[g] = tp[(kb + g) * N];
                        }
#pragma unroll
                        for (int g = 0; g < G; ++g) {
                            const int kk = h * G + g;
                            const uint32_t k = kb + g;
                            w[(kk + FB - 1) % FB] = (double)s[g];
                            fir_step<FB>(w, kk, t[g], k, na, __ballot(k >= lo && k <= hi) != 0, S, fa);
                        }
                    } else {
#pragma unroll
                        for (int g = 0; g < G - 1; ++g) {
                            const int kk = h * G + g;
                            const uint32_t k = kb + g;
                            if (k >= Tw) break;
                            w[(kk + FB - 1) % FB] = (double)col[r * N];
                            r = r + 1 == R ? 0 : r + 1;
                            fir_step<FB>(w, kk, tp[k * N], k, na, __ballot(k >= lo && k <= hi) != 0, S, fa);
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < FB; ++i) {
                const float fs = (float)S[i];                       // the second slice's sum where the frame has one (+0.0 else)
                const bool two = na[i] < Tw;
                const float y = __fmul_rn(__fadd_rn(two ? fa[i] : fs, two ? fs : 0.0f), div);
                __builtin_nontemporal_store(present ? y : x[i], lout + (f + i) * rs);
            }
            row += FB;
            if (row >= R) row -= R;
            if (present) d.head = e.head;
            f += FB;
            continue;
        }
        // the general body: one frame
        const float x = lin[f * rs];
        float y = x;
        if (present) {
            col[row * N] = x;
            y = fir_frame(col, tp, N, R, d, T, div, row);
        }
        __builtin_nontemporal_store(y, lout + f * rs);
        row = row + 1 == R ? 0 : row + 1;
        ++f;
    }
    if (present) {
        a.dq[c] = (int32_t)d.len;
        a.dq[N + c] = (int32_t)d.cap;
        a.dq[2 * N + c] = (int32_t)d.head;
    }
}

// a taps store, in stream order: rows[i * stride + j] is tap j (time order) of channel first + i's response (stride 0: one
// response for the range) -> taps[T - 1 - j][c].  With a response per channel consecutive threads read consecutive doubles of the
// page-locked rows; with one response they write consecutive channels.  The thread of j == 0 makes the node: T and the mode
// (DSPFX_FIRS_NONE: the one it carries, Balanced for a new node), and an empty deque where the channel carried none
__global__ __launch_bounds__(FWG) void firs_store(double *__restrict__ taps, uint32_t *__restrict__ tn, int32_t *__restrict__ dq,
                                                  const double *__restrict__ rows, uint32_t N, uint32_t first, uint32_t count, uint32_t T,
                                                  uint32_t stride, uint32_t mode) {
    const uint64_t total = (uint64_t)count * T;
    for (uint64_t e = (uint64_t)blockIdx.x * FWG + threadIdx.x; e < total; e += (uint64_t)gridDim.x * FWG) {
        uint32_t i, j;
        if (stride) {
            i = (uint32_t)(e / T);
            j = (uint32_t)(e % T);
        } else {
            j = (uint32_t)(e / count);
            i = (uint32_t)(e % count);
        }
        const size_t c = (size_t)first + i;
        taps[(size_t)(T - 1 - j) * N + c] = rows[(size_t)i * stride + j];
        if (j) continue;
        const uint32_t old = tn[c];
        const uint32_t m = mode == DSPFX_FIRS_NONE ? ((old & TN_T) ? (old & TN_AVERAGE) : 0u) : mode == DSPFX_FIR_AVERAGE ? TN_AVERAGE : 0u;
        tn[c] = T | m;
        if (!(old & TN_T)) dq[c] = dq[(size_t)N + c] = dq[2 * (size_t)N + c] = 0;
    }
}

enum StoreKind : uint32_t { ST_TAPS, ST_MODE, ST_DROP, ST_RESET };

// a mode, a drop, a reset over channels [first, first + count), in stream order
__global__ __launch_bounds__(FWG) void firs_node(uint32_t *__restrict__ tn, int32_t *__restrict__ dq, uint32_t N, uint32_t first, uint32_t count,
                                                 uint32_t kind, uint32_t mode) {
    const uint32_t i = blockIdx.x * FWG + threadIdx.x;
    if (i >= count) return;
    const size_t c = (size_t)first + i;
    if (kind == ST_MODE) {
        const uint32_t old = tn[c];
        if (old & TN_T) tn[c] = (old & TN_T) | (mode == DSPFX_FIR_AVERAGE ? TN_AVERAGE : 0u);
    } else {
        if (kind == ST_DROP) tn[c] = 0;
        dq[c] = dq[(size_t)N + c] = dq[2 * (size_t)N + c] = 0;     // the deque emptied (fir_reset)
    }
}

thread_local std::string g_err;        // the reason of the last failed create or plan on this thread

// a store's vals: TAPS T doubles (per_channel 0) or count x T doubles, in time order; the others carry none
struct StoreFields {
    StoreKind kind = ST_RESET;
    uint32_t first = 0, count = 0;
    uint32_t T = 0, per_channel = 0, mode = 0;
};
typedef StoreQueue<StoreFields> Stores;
typedef Stores::Store Store;

int check_max_taps(uint32_t max_taps, std::string &err) {
    if (max_taps >= 1 && max_taps <= DSPFX_FIRS_MAX_TAPS) return DSPFX_OK;
    char buf[96];
    std::snprintf(buf, sizeof buf, "firs: max_taps is %u, not 1 .. %u", max_taps, (unsigned)DSPFX_FIRS_MAX_TAPS);
    err = buf;
    return DSPFX_ERR_INVALID;
}

bool mode_ok(uint32_t mode) { return mode == DSPFX_FIR_BALANCED || mode == DSPFX_FIR_AVERAGE; }

}  // namespace

struct dspfx_firs : ChannelBank<dspfx_firs_desc, StoreFields> {
    static constexpr const char *name = "firs";
    // the host tables, as every store made so far left them: T (0: no node), the mode, and the response as it was given -- the
    // values of the store that named the channel last, shared by the channels of that store
    std::vector<uint16_t> hT;
    std::vector<uint8_t> hmode;
    std::vector<std::shared_ptr<const std::vector<double>>> hresp;
    std::vector<uint64_t> hoff;                  // the response starts at (*hresp[c])[hoff[c]]
    uint32_t row = 0;                            // the ring row of the next run's first frame (mu)
    double *taps = nullptr;
    float *ring = nullptr;
    uint32_t *tn = nullptr;
    int32_t *dq = nullptr;
    // the fresh state: no node anywhere, every deque empty.  The taps and the ring are never cleared: a node reads a tap only after
    // the store that wrote it, and a sample only after it pushed it
    template <class V>
    static void tables(const dspfx_firs_desc &d, V v) {
        const uint64_t N = d.n_channels;
        v(8 * N * d.max_taps, TABLE_BY_HAND, &dspfx_firs::taps);
        v(4 * N * (d.max_taps + FB), TABLE_BY_HAND, &dspfx_firs::ring);
        v(4 * N, 0, &dspfx_firs::tn);
        v(12 * N, 0, &dspfx_firs::dq);
    }
};

namespace {

// one store onto the stream
hipError_t apply_store(dspfx_firs *p, const Store &st, hipStream_t s) {
    const uint32_t N = p->desc.n_channels;
    if (st.kind == ST_TAPS) {
        const double *rows = nullptr;
        const hipError_t err = hipHostGetDevicePointer((void **)&rows, st.vals, 0);
        if (err != hipSuccess) return err;
        const uint64_t total = (uint64_t)st.count * st.T;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + FWG - 1) / FWG, 1u << 20);
        firs_store<<<blocks, FWG, 0, s>>>(p->taps, p->tn, p->dq, rows, N, st.first, st.count, st.T, st.per_channel ? st.T : 0, st.mode);
    } else {
        firs_node<<<(st.count + FWG - 1) / FWG, FWG, 0, s>>>(p->tn, p->dq, N, st.first, st.count, st.kind, st.mode);
    }
    return hipGetLastError();
}

}  // namespace

extern "C" const char *dspfx_firs_last_error(const dspfx_firs *p) { return p ? p->err.c_str() : g_err.c_str(); }

extern "C" int dspfx_firs_plan(uint64_t channels, uint32_t max_taps, uint64_t *bytes_out) {
    return plan_bank<dspfx_firs>(channels, bytes_out, g_err, [max_taps](dspfx_firs_desc &d, std::string &err) {
        d.max_taps = max_taps;
        return check_max_taps(max_taps, err);
    });
}

extern "C" int dspfx_firs_create(const dspfx_firs_desc *desc, dspfx_firs **out) {
    const int rc = create_checks(desc, out, g_err, [desc](std::string &err) { return check_max_taps(desc->max_taps, err); });
    if (rc != DSPFX_OK) return rc;
    return create_bank(desc, out, g_err, [](dspfx_firs *p) {
        const size_t N = p->desc.n_channels;
        p->hT.assign(N, 0);
        p->hmode.assign(N, 0);
        p->hresp.assign(N, nullptr);
        p->hoff.assign(N, 0);
    });
}

extern "C" int dspfx_firs_destroy(dspfx_firs *p) { return destroy_bank(p); }

extern "C" int dspfx_firs_set_taps(dspfx_firs *p, const double *host_taps, uint32_t n_taps, uint32_t per_channel, uint32_t mode, uint64_t first_channel,
                                   uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    char buf[160];
    if (!host_taps) return p->fail(DSPFX_ERR_INVALID, "firs set_taps: no taps");
    if (n_taps == 0 || n_taps > p->desc.max_taps) {
        std::snprintf(buf, sizeof buf, "firs set_taps: %u taps, not 1 .. max_taps = %u", n_taps, p->desc.max_taps);
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    if (mode != DSPFX_FIRS_NONE && !mode_ok(mode)) {
        std::snprintf(buf, sizeof buf, "firs set_taps: mode %u is not DSPFX_FIR_BALANCED, DSPFX_FIR_AVERAGE or DSPFX_FIRS_NONE", mode);
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    const int rc = check_range(p, "set_taps", first_channel, count);
    if (rc != DSPFX_OK) return rc;
    if (count == 0) return DSPFX_OK;
    const uint64_t n = per_channel ? count * n_taps : n_taps;
    std::shared_ptr<const std::vector<double>> resp;
    try {
        resp = std::make_shared<const std::vector<double>>(host_taps, host_taps + n);
    } catch (const std::bad_alloc &) {
        return p->fail(DSPFX_ERR_OOM, "firs set_taps: no host memory for the response");
    }
    Store st;
    st.T = n_taps;
    st.per_channel = per_channel ? 1 : 0;
    st.mode = mode;
    if (!stage_store(p, st, nullptr, ST_TAPS, "set_taps", first_channel, count, 2 * n, "staged taps")) return DSPFX_ERR_OOM;
    std::memcpy(st.vals, host_taps, n * sizeof(double));
    p->stores.push(st, [&] {
        for (uint64_t i = 0; i < count; ++i) {
            const size_t c = first_channel + i;
            if (mode != DSPFX_FIRS_NONE) p->hmode[c] = (uint8_t)mode;
            else if (!p->hT[c]) p->hmode[c] = DSPFX_FIR_BALANCED;
            p->hT[c] = (uint16_t)n_taps;
            p->hresp[c] = resp;
            p->hoff[c] = per_channel ? i * n_taps : 0;
        }
    });
    return DSPFX_OK;
}

extern "C" int dspfx_firs_set_mode(dspfx_firs *p, uint32_t mode, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    if (!mode_ok(mode)) {
        char buf[128];
        std::snprintf(buf, sizeof buf, "firs set_mode: mode %u is not DSPFX_FIR_BALANCED or DSPFX_FIR_AVERAGE", mode);
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    return store_plain(
        p, ST_MODE, "set_mode", first_channel, count,
        [=] {
            for (uint64_t c = first_channel; c < first_channel + count; ++c)
                if (p->hT[c]) p->hmode[c] = (uint8_t)mode;
        },
        [=](Store &st) { st.mode = mode; });
}

extern "C" int dspfx_firs_drop(dspfx_firs *p, uint64_t first_channel, uint64_t count) {
    return store_plain(p, ST_DROP, "drop", first_channel, count, [=] {
        for (uint64_t c = first_channel; c < first_channel + count; ++c) {
            p->hT[c] = 0;
            p->hmode[c] = 0;
            p->hresp[c] = nullptr;
            p->hoff[c] = 0;
        }
    });
}

extern "C" int dspfx_firs_reset(dspfx_firs *p, uint64_t first_channel, uint64_t count) { return store_plain(p, ST_RESET, "reset", first_channel, count); }

extern "C" int dspfx_firs_present(dspfx_firs *p, uint32_t *host_present_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "present", host_present_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = p->hT[c] != 0; });
}

extern "C" int dspfx_firs_lengths(dspfx_firs *p, uint32_t *host_lengths_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "lengths", host_lengths_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = p->hT[c]; });
}

extern "C" int dspfx_firs_modes(dspfx_firs *p, uint32_t *host_modes_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "modes", host_modes_out, first_channel, count,
                      [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = p->hT[c] ? (uint32_t)p->hmode[c] : DSPFX_FIRS_NONE; });
}

extern "C" int dspfx_firs_taps(dspfx_firs *p, uint64_t channel, double *host_taps_out, uint32_t *n_taps_out) {
    if (!p) return DSPFX_ERR_INVALID;
    if (!n_taps_out) return p->fail(DSPFX_ERR_INVALID, "firs taps: no count");
    return read_table(p, "taps", host_taps_out, channel, 1, [=](double *o, uint64_t, uint64_t c) {
        *n_taps_out = p->hT[c];
        if (p->hT[c]) std::memcpy(o, p->hresp[c]->data() + p->hoff[c], p->hT[c] * sizeof(double));
    });
}

extern "C" int dspfx_firs_deque(dspfx_firs *p, const int32_t **deque_out) {
    if (!p) return DSPFX_ERR_INVALID;
    if (deque_out) *deque_out = p->dq;
    return DSPFX_OK;
}

extern "C" int dspfx_firs_run(dspfx_firs *p, const float *in, float *out, uint32_t n_frames, void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    hipStream_t s = (hipStream_t)stream;
    const int rc = begin_run(p, in && out, n_frames, s, "firs run: in, out or n_frames", "firs store", apply_store);
    if (rc != DSPFX_OK) return rc;
    FirsArgs a;
    a.in = in;
    a.out = out;
    a.taps = p->taps;
    a.ring = p->ring;
    a.tn = p->tn;
    a.dq = p->dq;
    a.N = p->desc.n_channels;
    a.W = p->desc.tile_channels;
    a.nf = n_frames;
    a.R = p->desc.max_taps + FB;
    a.row = p->row;
    a.general_only = p->desc.general_only;
    firs_run<<<lane_blocks(a.N, 1, FWG), FWG, 0, s>>>(a);
    BANK_HIP_WHY(hipGetLastError(), "firs_run");
    p->row = (uint32_t)((p->row + (uint64_t)n_frames) % a.R);
    return DSPFX_OK;
}
