// racks_kernels.hip -- the channel-rack bank (include/dspfx.h, dspfx_racks_*): every channel owns `slots` slots (1 .. 4), run in
// slot order, and each slot is empty or carries any one of the small-state chain nodes -- Gain (gain.rs:33-37), BiQuad
// (biquad.rs:62-88), LowPass, HighPass, Envelope, Distort (every mode but Fuzz), Overdrive, Chebyshev -- with its own sliders and
// state.  What the strips, filters and shapers banks do in three launches and six block-units of traffic, a rack does in one pass:
// all slots run in registers between one load and one store of the block.
//
// One run is one kernel behind the queued stores, in the shape of filters_run / shapers_run: a lane owns its channels for the whole
// run -- four adjacent channels with one 16-byte load and one nontemporal 16-byte store per frame when the layout allows it and the
// slot count leaves the registers (lane_io.hip.h; CPL below), two or one otherwise.  Frames are taken in chunks of F rows and the
// next chunk's loads are issued ahead of this one's arithmetic.  `slots` is a template parameter: every slot's kind, five slider
// floats and four state floats are registers.  The arithmetic is the merged banks': the one-pole, envelope and biquad steps
// that filters_kernels.hip and strips_kernels.hip call too (node_steps.hip.h), the waveshapers called in chain_kernels.hip.h as
// shapers_kernels.hip calls them, so a channel's bits are those of the existing banks run slot after slot.  The kinds differ per
// lane and per slot: before the frame loop the wave ballots once per slot for the kinds its lanes carry (a Distort or Overdrive
// whose level is below 0.001 is folded into "empty" first, as in shapers), and per chunk and slot it walks the set bits with a
// wave-uniform switch and runs each present kind's templated body on all its values, keeping a result under a per-(lane, channel)
// select.  No lane ever branches on its own kind; a wave whose lanes carry nothing in a slot does no arithmetic for it and reads
// neither its sliders nor its state.  The tables are [slot][field][N]: kinds and sliders are read once per run, the state is read
// once and written once.  A lane rewrites only elements it read, so out may be in.  Nothing is shared between channels: no LDS, no
// atomics.
//
// Stores (nodes, drops, resets) go through the staged-store queue (store_queue.hip.h).  Whether a store makes a slot's node NEW
// (its state back to +0.0; every BiQuad store does, biquad.rs:62-76) is decided on the host, from the host tables, when the store is
// made; it travels as a flag in the kind byte, which racks_fresh takes off again in stream order.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/dspfx.h"
#include "chain_kernels.hip.h"
#include "channel_bank.hip.h"
#include "lane_io.hip.h"
#include "node_steps.hip.h"

namespace {

constexpr uint32_t RWG = 256;
constexpr uint32_t MAX_SLOTS = 4;
constexpr int NFIELD = 5, NSTATE = 4, NRAW = 6;

// a slot's kind code, one byte.  C_NEW rides on a stored code until racks_fresh has zeroed the slot's state
enum Code : uint8_t {
    C_NONE = 0, C_GAIN = 1, C_BIQUAD = 2, C_LP = 3, C_HP = 4, C_ENV = 5, C_DIST = 6 /* + dspfx_distort_mode */,
    C_FUZZ = C_DIST + DSPFX_DIST_FUZZ /* never stored */, C_OVER = 15, C_CHEB = 16, C_COUNT = 17, C_NEW = 0x80
};
constexpr uint32_t bit(int k) { return 1u << k; }
// the kinds that keep state in row 0 / in all four rows; the kinds that read slider field r (a bit per code)
constexpr uint32_t M_STATE = bit(C_BIQUAD) | bit(C_LP) | bit(C_HP) | bit(C_ENV);
constexpr uint32_t field_mask(int r) {
    return r == 0 ? ~bit(C_NONE) : r == 1 ? bit(C_BIQUAD) | bit(C_ENV) | bit(C_OVER) | bit(C_CHEB) : r == 2 ? bit(C_BIQUAD) | bit(C_OVER) : bit(C_BIQUAD);
}
// ... and the kinds that evaluate in f64: the HEAVY instantiation
constexpr uint32_t M_HEAVY = bit(C_DIST + DSPFX_DIST_TANH) | bit(C_DIST + DSPFX_DIST_SIN) | bit(C_DIST + DSPFX_DIST_ATAN) | bit(C_OVER) | bit(C_CHEB);

struct RackArgs {
    const float *in;             // may be `out`: no __restrict__
    float *out;
    const float *field;          // [slots][5][N]: Gain level | BiQuad a1, a2, b0, b1, b2 normalised | ratio | ga, gr | Distort level |
                                 // Overdrive boost, drive, level | Chebyshev level_pos, level_neg
    float *state;                // [slots][4][N]: z or the envelope in row 0 | x1, x2, y1, y2
    const uint8_t *kind;         // [slots][N]
    uint32_t N, W, nf;
    uint32_t slots;              // the bank's: a kernel of more slots reads nothing of the others, which are empty
};

// one slot of the lane over a run.  One-pole: p[1] is 1 - r; Chebyshev: p[2], p[3] are tanh(level_pos), tanh(level_neg)
template <int CPL>
struct Slot {
    float p[NFIELD][CPL], st[NSTATE][CPL];
    uint32_t kind[CPL];          // with the bypasses folded in: C_NONE is a copy
};

// kind K on R rows of one slot: every value is computed, a channel of kind K keeps the result and the new state; every other
// channel keeps its sample's own bits and its state.  Nothing is contracted:
//   Gain      y = x * level                                                  (gain.rs:33-37)
//   BiQuad    y = biquad_step                                                (node_steps.hip.h, as strips_kernels.hip band_rows)
//   LowPass   z = one_pole_step; y = z                                       (node_steps.hip.h, as filters_kernels.hip filt_rows)
//   HighPass  z = one_pole_step; y = x - z
//   Envelope  z = envelope_step; y = z
//   the waveshapers: chain_kernels.hip.h, as shapers_kernels.hip shape_rows calls them
template <int K, int CPL, int R>
__device__ __forceinline__ void rack_rows(float (&v)[R][CPL], Slot<CPL> &s) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const float x = v[i][j];
            const bool mine = s.kind[j] == (uint32_t)K;
            if constexpr (K == C_GAIN) {
                v[i][j] = pick(0u - (uint32_t)mine, x * s.p[0][j], x);
            } else if constexpr (K == C_BIQUAD) {
                const float a1 = s.p[0][j], a2 = s.p[1][j], b0 = s.p[2][j], b1 = s.p[3][j], b2 = s.p[4][j];
                const float y = biquad_step(x, a1, a2, b0, b1, b2, s.st[0][j], s.st[1][j], s.st[2][j], s.st[3][j]);
                const uint32_t m = 0u - (uint32_t)mine;
                s.st[1][j] = pick(m, s.st[0][j], s.st[1][j]);
                s.st[0][j] = pick(m, x, s.st[0][j]);
                s.st[3][j] = pick(m, s.st[2][j], s.st[3][j]);
                s.st[2][j] = pick(m, y, s.st[2][j]);
                v[i][j] = pick(m, y, x);
            } else if constexpr (K == C_LP || K == C_HP || K == C_ENV) {
                const float l = s.st[0][j];
                float nz, y;
                if constexpr (K == C_ENV) {
                    nz = envelope_step(x, l, s.p[0][j], s.p[1][j]);
                    y = nz;
                } else {
                    nz = one_pole_step(x, l, s.p[0][j], s.p[1][j]);
                    y = K == C_HP ? __fsub_rn(x, nz) : nz;
                }
                s.st[0][j] = mine ? nz : l;
                v[i][j] = mine ? y : x;
            } else {
                float y;
                if constexpr (K == C_OVER) y = dspfx::overdrive1(x, s.p[0][j], s.p[1][j], s.p[2][j]);
                else if constexpr (K == C_CHEB) y = dspfx::chebyshev1(x, s.p[0][j], s.p[1][j], s.p[2][j], s.p[3][j]);
                else y = dspfx::distort1<K - C_DIST, false>(x, s.p[0][j], 0.0, 0.0);
                v[i][j] = mine ? y : x;
            }
        }
    }
}

// the kinds in `kinds` (a bit per code, the same in every lane of the wave), one after the other: a channel carries at most one of
// them, so their order does not matter.  HEAVY: the kernel holds the bodies that evaluate in f64 too
template <int CPL, int R, bool HEAVY>
__device__ __forceinline__ void rack_slot(uint32_t kinds, float (&v)[R][CPL], Slot<CPL> &s) {
    while (kinds) {
        const int k = __builtin_ctz(kinds);
        kinds &= kinds - 1;
        switch (k) {
        case C_GAIN: rack_rows<C_GAIN, CPL, R>(v, s); break;
        case C_BIQUAD: rack_rows<C_BIQUAD, CPL, R>(v, s); break;
        case C_LP: rack_rows<C_LP, CPL, R>(v, s); break;
        case C_HP: rack_rows<C_HP, CPL, R>(v, s); break;
        case C_ENV: rack_rows<C_ENV, CPL, R>(v, s); break;
        case C_DIST + DSPFX_DIST_HARD_CLIP: rack_rows<C_DIST + DSPFX_DIST_HARD_CLIP, CPL, R>(v, s); break;
        case C_DIST + DSPFX_DIST_SOFT_CLIP: rack_rows<C_DIST + DSPFX_DIST_SOFT_CLIP, CPL, R>(v, s); break;
        case C_DIST + DSPFX_DIST_TANH: if constexpr (HEAVY) rack_rows<C_DIST + DSPFX_DIST_TANH, CPL, R>(v, s); break;
        case C_DIST + DSPFX_DIST_RECIP_SOFT_CLIP: rack_rows<C_DIST + DSPFX_DIST_RECIP_SOFT_CLIP, CPL, R>(v, s); break;
        case C_DIST + DSPFX_DIST_SIN: if constexpr (HEAVY) rack_rows<C_DIST + DSPFX_DIST_SIN, CPL, R>(v, s); break;
        case C_DIST + DSPFX_DIST_ATAN: if constexpr (HEAVY) rack_rows<C_DIST + DSPFX_DIST_ATAN, CPL, R>(v, s); break;
        case C_DIST + DSPFX_DIST_SQUARE: rack_rows<C_DIST + DSPFX_DIST_SQUARE, CPL, R>(v, s); break;
        case C_DIST + DSPFX_DIST_CHEBYSHEV4: rack_rows<C_DIST + DSPFX_DIST_CHEBYSHEV4, CPL, R>(v, s); break;
        case C_OVER: if constexpr (HEAVY) rack_rows<C_OVER, CPL, R>(v, s); break;
        case C_CHEB: if constexpr (HEAVY) rack_rows<C_CHEB, CPL, R>(v, s); break;
        default: break;
        }
    }
}

// f(integral_constant<int, T>) for T = 0 .. S - 1, the index a constant in every call: `#pragma unroll` gives up on a loop whose
// unrolled body passes its size threshold (the f64 bodies do), and a slot indexed at run time is a slot in scratch
template <int T, int S, class Fn>
__device__ __forceinline__ void each_slot(Fn &&f) {
    if constexpr (T < S) {
        f(std::integral_constant<int, T>{});
        each_slot<T + 1, S>(f);
    }
}
#define RACK_INLINE __attribute__((always_inline))

template <int S>
struct WaveKinds {
    uint32_t k[S];               // bit c: a lane of the wave carries code c in the slot (wave-uniform)
};

template <int S, int CPL, int R, bool HEAVY>
__device__ __forceinline__ void rack_slots(const WaveKinds<S> &w, float (&v)[R][CPL], Slot<CPL> (&s)[S]) {
    each_slot<0, S>([&](auto ti) RACK_INLINE {
        constexpr int t = decltype(ti)::value;
        if (w.k[t]) rack_slot<CPL, R, HEAVY>(w.k[t], v, s[t]);
    });
}

// the channels per lane of the vector path, the frame rows per chunk (two chunks are in registers) and the waves per SIMD the
// register allocation is held to: a slot is 10 registers per channel beside the rows (DESIGN section 8 has the table)
constexpr int rack_cpl(int S) { return S <= 2 ? 4 : 2; }
constexpr int rack_rows_for(int CPL) { return CPL == 4 ? 4 : 8; }

template <int S, int CPL, bool HEAVY>
__global__ __launch_bounds__(RWG) void racks_run(RackArgs a) {
    constexpr int F = rack_rows_for(CPL);
    uint32_t c;
    if (!lane_channel<CPL>(RWG, a.N, c)) return;
    Slot<CPL> s[S];
    WaveKinds<S> w;
    each_slot<0, S>([&](auto ti) RACK_INLINE {
        constexpr int t = decltype(ti)::value;
        uint8_t code[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) code[j] = C_NONE;
        if (t < (int)a.slots) loadv<CPL>(a.kind + (size_t)t * a.N + c, code);      // (N % 4 == 0 with CPL > 1: every slot's row is aligned as the first)
#pragma unroll
        for (int r = 0; r < NFIELD; ++r)
#pragma unroll
            for (int j = 0; j < CPL; ++j) s[t].p[r][j] = 0.0f;
#pragma unroll
        for (int r = 0; r < NSTATE; ++r)
#pragma unroll
            for (int j = 0; j < CPL; ++j) s[t].st[r][j] = 0.0f;
        // what the wave's lanes hold in the table: which sliders and state rows are read at all
        uint32_t held = 0;
#pragma unroll
        for (uint32_t k = C_GAIN; k < C_COUNT; ++k) {
            bool mine = false;
#pragma unroll
            for (int j = 0; j < CPL; ++j) mine |= code[j] == k;
            if (__ballot(mine)) held |= 1u << k;           // (the lanes that returned above are not asked)
        }
        held = __builtin_amdgcn_readfirstlane(held);
        const float *fp = a.field + (size_t)t * NFIELD * a.N + c;
#pragma unroll
        for (int r = 0; r < NFIELD; ++r)
            if (held & field_mask(r)) loadv<CPL>(fp + (size_t)r * a.N, s[t].p[r]);
        const float *sp = a.state + (size_t)t * NSTATE * a.N + c;
        if (held & M_STATE) loadv<CPL>(sp, s[t].st[0]);
        if (held & bit(C_BIQUAD)) {
#pragma unroll
            for (int r = 1; r < NSTATE; ++r) loadv<CPL>(sp + (size_t)r * a.N, s[t].st[r]);
        }
        // the bypasses are the reference's, as in shapers_run: Distort and Overdrive return the sample when level < 0.001, which a
        // NaN level is not; Chebyshev bypasses per branch inside chebyshev1
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            uint32_t k = code[j];
            if (k >= C_DIST && k < C_OVER && s[t].p[0][j] < 0.001f) k = C_NONE;
            if (k == C_OVER && s[t].p[2][j] < 0.001f) k = C_NONE;
            if (k == C_LP || k == C_HP) s[t].p[1][j] = __fsub_rn(1.0f, s[t].p[0][j]);
            s[t].kind[j] = k;
        }
        uint32_t kinds = 0;
#pragma unroll
        for (uint32_t k = C_GAIN; k < C_COUNT; ++k) {
            if (!HEAVY && ((M_HEAVY >> k) & 1u)) continue;
            bool mine = false;
#pragma unroll
            for (int j = 0; j < CPL; ++j) mine |= s[t].kind[j] == k;
            if (__ballot(mine)) kinds |= 1u << k;
        }
        w.k[t] = __builtin_amdgcn_readfirstlane(kinds);
        if (HEAVY && (w.k[t] & bit(C_CHEB))) {             // chebyshev.rs:52-62: the denominators, once per run
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                const float tp = dspfx::tanh_cr(s[t].p[0][j]), tn = dspfx::tanh_cr(s[t].p[1][j]);
                if (s[t].kind[j] == C_CHEB) {
                    s[t].p[2][j] = tp;
                    s[t].p[3][j] = tn;
                }
            }
        }
    });
    const size_t lane0 = lay(0, c, a.nf, a.N, a.W), rs = a.W ? a.W : a.N;
    const float *lin = a.in + lane0;
    float *lout = a.out + lane0;
    // lane_io's each_chunk, written out: with the helper racks_run<4, 2, true> takes 261 registers for 253, one wave per SIMD for two
    const uint32_t nfull = a.nf / F;
    float cur[F][CPL], nxt[F][CPL];
    if (nfull) load_rows<CPL, F>(lin, rs, 0, cur);
#pragma unroll 1
    for (uint32_t ch = 0; ch < nfull; ++ch) {
        if (ch + 1 < nfull) load_rows<CPL, F>(lin, rs, (ch + 1) * F, nxt);
        rack_slots<S, CPL, F, HEAVY>(w, cur, s);
        store_rows<CPL, F>(lout, rs, ch * F, cur);
#pragma unroll
        for (int i = 0; i < F; ++i)
#pragma unroll
            for (int j = 0; j < CPL; ++j) cur[i][j] = nxt[i][j];
    }
#pragma unroll 1
    for (uint32_t f = nfull * F; f < a.nf; ++f) {
        float one[1][CPL];
        load_rows<CPL, 1>(lin, rs, f, one);
        rack_slots<S, CPL, 1, HEAVY>(w, one, s);
        store_rows<CPL, 1>(lout, rs, f, one);
    }
    // a wave without a stateful kind in the slot read nothing and writes nothing; a channel that carries none kept what it read
    each_slot<0, S>([&](auto ti) RACK_INLINE {
        constexpr int t = decltype(ti)::value;
        float *sp = a.state + (size_t)t * NSTATE * a.N + c;
        if (w.k[t] & M_STATE) storev<CPL, false>(sp, s[t].st[0]);
        if (w.k[t] & bit(C_BIQUAD)) {
#pragma unroll
            for (int r = 1; r < NSTATE; ++r) storev<CPL, false>(sp + (size_t)r * a.N, s[t].st[r]);
        }
    });
}

// the device side of a drop, a reset and a new node, in stream order, on channels [first, first + count) of slots
// [slot, slot + gridDim.y): the four state rows back to +0.0.  only_new: only where the stored code carries C_NEW, which is taken off
__global__ __launch_bounds__(RWG) void racks_fresh(float *__restrict__ state, uint8_t *__restrict__ kind, uint32_t N, uint32_t slot, uint32_t first,
                                                   uint32_t count, bool only_new) {
    const uint32_t i = blockIdx.x * RWG + threadIdx.x;
    if (i >= count) return;
    const size_t t = slot + blockIdx.y, at = t * N + first + i;
    if (only_new) {
        const uint8_t k = kind[at];
        if (!(k & C_NEW)) return;
        kind[at] = k & (uint8_t)~C_NEW;
    }
#pragma unroll
    for (int r = 0; r < NSTATE; ++r) state[(t * NSTATE + r) * N + first + i] = 0.0f;
}

thread_local std::string g_err;        // the reason of the last failed create or plan on this thread

enum StoreKind : uint32_t { ST_NODES, ST_DROP, ST_RESET };

// a store's vals: NODES five runs of [count] device fields, six runs of [count] raw sliders (for the host tables), then [count]
// kind codes as bytes; DROP and RESET carry none
struct StoreFields {
    StoreKind kind = ST_RESET;
    uint32_t first = 0, count = 0;
    uint32_t slot = 0, n_slots = 1;              // DROP, RESET: slots [slot, slot + n_slots)
    bool any_new = false;                        // NODES: a code carries C_NEW
};
typedef StoreQueue<StoreFields> Stores;
typedef Stores::Store Store;

bool heavy(uint8_t k) { return k < C_COUNT && ((M_HEAVY >> k) & 1u); }
bool is_dist(uint8_t k) { return k >= C_DIST && k < C_OVER; }
uint32_t code_kind(uint8_t k) {
    switch (k) {
    case C_NONE: return DSPFX_RACKS_NONE;
    case C_GAIN: return DSPFX_GAIN;
    case C_BIQUAD: return DSPFX_BIQUAD;
    case C_LP: return DSPFX_LOW_PASS;
    case C_HP: return DSPFX_HIGH_PASS;
    case C_ENV: return DSPFX_ENVELOPE;
    case C_OVER: return DSPFX_OVERDRIVE;
    case C_CHEB: return DSPFX_CHEBYSHEV;
    default: return DSPFX_DISTORT;
    }
}
uint32_t code_mode(uint8_t k) { return is_dist(k) ? (uint32_t)(k - C_DIST) : DSPFX_RACKS_NONE; }

int check_slots(uint32_t slots, std::string &err) {
    if (slots >= 1 && slots <= MAX_SLOTS) return DSPFX_OK;
    char buf[96];
    std::snprintf(buf, sizeof buf, "racks: slots is %u, not 1 .. %u", slots, MAX_SLOTS);
    err = buf;
    return DSPFX_ERR_INVALID;
}

// the kind a store names: its code (Distort: C_DIST, the mode is added per channel) and its slider count; 0 sliders: refused, and
// `why` names the bank that has the kind
int kind_code(uint32_t kind, uint8_t &code, const char *&why) {
    why = nullptr;
    switch (kind) {
    case DSPFX_GAIN: code = C_GAIN; return 1;
    case DSPFX_BIQUAD: code = C_BIQUAD; return 6;
    case DSPFX_LOW_PASS: code = C_LP; return 1;
    case DSPFX_HIGH_PASS: code = C_HP; return 1;
    case DSPFX_ENVELOPE: code = C_ENV; return 2;
    case DSPFX_DISTORT: code = C_DIST; return 1;
    case DSPFX_OVERDRIVE: code = C_OVER; return 3;
    case DSPFX_CHEBYSHEV: code = C_CHEB; return 2;
    case DSPFX_REVERB: why = "Reverb keeps a ring per channel: the delays bank (dspfx_delays_*) has it"; return 0;
    case DSPFX_FIR: why = "FIR keeps taps and a deque per channel: the firs bank (dspfx_firs_*) has it"; return 0;
    case DSPFX_ADD:
    case DSPFX_MIX: why = "Add and Mix take a second input: the blends bank (dspfx_blends_*) has them"; return 0;
    case DSPFX_SIGNAL_GEN: why = "SignalGen is a source: the gens bank (dspfx_gens_*) has it"; return 0;
    default: why = "no such node kind"; return 0;
    }
}

}  // namespace

struct dspfx_racks : ChannelBank<dspfx_racks_desc, StoreFields> {          // mu: also rcode and run_heavy
    static constexpr const char *name = "racks";
    std::vector<float> hs[NRAW];                 // [slots][N] each: the raw sliders with every store made so far
    std::vector<uint8_t> hcode;                  // [slots][N]: ... and the kind codes
    // what the device tables hold once the stores DRAINED so far have run (shapers_kernels.hip's rcode): which run kernel
    std::vector<uint8_t> rcode;                  // [slots][N]
    uint64_t run_heavy = 0;                      // the slots in rcode of a kind that evaluates in f64
    float *field = nullptr, *state = nullptr;
    uint8_t *kind = nullptr;
    // the fresh state: every slot of every channel empty, every table at rest
    template <class V>
    static void tables(const dspfx_racks_desc &d, V v) {
        const uint64_t cells = (uint64_t)d.slots * d.n_channels;
        v(4 * NFIELD * cells, 0, &dspfx_racks::field);
        v(4 * NSTATE * cells, 0, &dspfx_racks::state);
        v(cells, C_NONE, &dspfx_racks::kind);
    }
};

namespace {

// one store onto the stream (the bank's mu is held): the device tables, and the run-order kind table beside them
hipError_t apply_store(dspfx_racks *p, const Store &st, hipStream_t s) {
    const uint32_t N = p->desc.n_channels;
    const size_t n = st.count, bytes = n * sizeof(float), at = (size_t)st.slot * N + st.first;
    const dim3 grid((st.count + RWG - 1) / RWG, st.n_slots);
    const uint8_t *codes = st.kind == ST_NODES ? (const uint8_t *)(st.vals + (NFIELD + NRAW) * n) : nullptr;
    if (st.kind != ST_RESET)
        for (uint32_t t = 0; t < st.n_slots; ++t)
            for (size_t i = 0; i < n; ++i) {
                uint8_t &r = p->rcode[at + (size_t)t * N + i];
                const uint8_t k = codes ? (uint8_t)(codes[i] & ~C_NEW) : (uint8_t)C_NONE;
                p->run_heavy += (uint64_t)heavy(k) - (uint64_t)heavy(r);
                r = k;
            }
    hipError_t err = hipSuccess;
    switch (st.kind) {
    case ST_NODES:
        for (int r = 0; r < NFIELD && err == hipSuccess; ++r)
            err = hipMemcpyAsync(p->field + ((size_t)st.slot * NFIELD + r) * N + st.first, st.vals + r * n, bytes, hipMemcpyHostToDevice, s);
        if (err == hipSuccess) err = hipMemcpyAsync(p->kind + at, codes, n, hipMemcpyHostToDevice, s);
        if (err != hipSuccess || !st.any_new) return err;
        racks_fresh<<<grid, RWG, 0, s>>>(p->state, p->kind, N, st.slot, st.first, st.count, true);
        return hipGetLastError();
    case ST_DROP:
        for (uint32_t t = 0; t < st.n_slots && err == hipSuccess; ++t) err = hipMemsetAsync(p->kind + at + (size_t)t * N, C_NONE, n, s);
        if (err != hipSuccess) return err;
        [[fallthrough]];
    case ST_RESET:
        racks_fresh<<<grid, RWG, 0, s>>>(p->state, p->kind, N, st.slot, st.first, st.count, false);
        return hipGetLastError();
    }
    return hipSuccess;
}

// `slot` is one of the bank's; the reason is kept
int check_slot(dspfx_racks *p, const char *call, uint32_t slot) {
    if (slot < p->desc.slots) return DSPFX_OK;
    char buf[128];
    std::snprintf(buf, sizeof buf, "racks %s: slot %u is not one of the bank's %u", call, slot, p->desc.slots);
    return p->fail(DSPFX_ERR_INVALID, buf);
}

// channel_bank's store_plain with the slots a drop or a reset names: [slot, slot + n_slots)
template <class Also>
int store_slots(dspfx_racks *p, StoreKind kind, const char *call, uint32_t slot, uint32_t n_slots, uint64_t first, uint64_t count, Also also) {
    return store_plain(p, kind, call, first, count, also, [=](Store &st) {
        st.slot = slot;
        st.n_slots = n_slots;
    });
}

template <int S>
void launch_run(const RackArgs &a, bool vec, bool hv, hipStream_t s) {
    constexpr int CPL = rack_cpl(S);
    const uint32_t cpl = vec ? CPL : 1;
    const uint32_t blocks = lane_blocks(a.N, cpl, RWG);
    if (vec && hv) racks_run<S, CPL, true><<<blocks, RWG, 0, s>>>(a);
    else if (vec) racks_run<S, CPL, false><<<blocks, RWG, 0, s>>>(a);
    else if (hv) racks_run<S, 1, true><<<blocks, RWG, 0, s>>>(a);
    else racks_run<S, 1, false><<<blocks, RWG, 0, s>>>(a);
}

}  // namespace

extern "C" const char *dspfx_racks_last_error(const dspfx_racks *p) { return p ? p->err.c_str() : g_err.c_str(); }

extern "C" int dspfx_racks_plan(uint64_t channels, uint32_t slots, uint64_t *bytes_out) {
    return plan_bank<dspfx_racks>(channels, bytes_out, g_err, [slots](dspfx_racks_desc &d, std::string &err) {
        d.slots = slots;
        return check_slots(slots, err);
    });
}

extern "C" int dspfx_racks_create(const dspfx_racks_desc *desc, dspfx_racks **out) {
    const int rc = create_checks(desc, out, g_err, [desc](std::string &err) { return check_slots(desc->slots, err); });
    if (rc != DSPFX_OK) return rc;
    return create_bank(desc, out, g_err, [](dspfx_racks *p) {
        const size_t cells = (size_t)p->desc.slots * p->desc.n_channels;
        for (auto &h : p->hs) h.assign(cells, 0.0f);
        p->hcode.assign(cells, C_NONE);
        p->rcode.assign(cells, C_NONE);
    });
}

extern "C" int dspfx_racks_destroy(dspfx_racks *p) { return destroy_bank(p); }

extern "C" int dspfx_racks_set(dspfx_racks *p, uint32_t slot, uint32_t kind, const float *const *host_sliders, const uint32_t *host_mode,
                               uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    int rc = check_slot(p, "set", slot);
    if (rc == DSPFX_OK) rc = check_range(p, "set", first_channel, count);
    if (rc != DSPFX_OK) return rc;
    uint8_t code = C_NONE;
    const char *why = nullptr;
    const int n_sliders = kind_code(kind, code, why);
    char buf[224];
    if (n_sliders == 0) {
        std::snprintf(buf, sizeof buf, "racks set: kind %u is not a rack node: %s", kind, why);
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    if (host_mode && code == C_DIST)
        for (uint64_t i = 0; i < count; ++i)
            if (host_mode[i] > DSPFX_DIST_CHEBYSHEV4 || host_mode[i] == DSPFX_DIST_FUZZ) {
                if (host_mode[i] == DSPFX_DIST_FUZZ)
                    std::snprintf(buf, sizeof buf, "racks set: channel %llu is given Fuzz, which is block-global: the shapers bank (dspfx_shapers_*) has it",
                                  (unsigned long long)(first_channel + i));
                else
                    std::snprintf(buf, sizeof buf, "racks set: channel %llu is given mode %u, which is no Distort mode (0 .. %d)",
                                  (unsigned long long)(first_channel + i), host_mode[i], (int)DSPFX_DIST_CHEBYSHEV4);
                return p->fail(DSPFX_ERR_INVALID, buf);
            }
    if (count == 0) return DSPFX_OK;
    dspfx_node_desc def;
    if (dspfx_node_defaults((int)kind, &def) != DSPFX_OK) return p->fail(DSPFX_ERR_INVALID, "racks set: no such node kind");
    Store st;
    st.slot = slot;
    std::unique_lock<std::mutex> one;
    if (!stage_store(p, st, &one, ST_NODES, "set", first_channel, count, (NFIELD + NRAW) * count + (count + 3) / 4, "staged sliders")) return DSPFX_ERR_OOM;
    const size_t at = (size_t)slot * p->desc.n_channels + first_channel;
    float *dev = st.vals, *raw = st.vals + NFIELD * count;
    uint8_t *codes = (uint8_t *)(st.vals + (NFIELD + NRAW) * count);
    for (uint64_t i = 0; i < count; ++i) {
        const uint8_t old = p->hcode[at + i];
        const bool same = code == C_DIST ? is_dist(old) : old == code;      // the kind it carries: what is left out is kept
        float g[NRAW];
        for (int t = 0; t < NRAW; ++t) {
            const float *v = host_sliders ? host_sliders[t] : nullptr;
            g[t] = t >= n_sliders ? 0.0f : v ? v[i] : same ? p->hs[t][at + i] : def.params[t];
            raw[t * count + i] = g[t];
        }
        float d[NFIELD] = {g[0], g[1], g[2], 0.0f, 0.0f};
        if (code == C_BIQUAD) (void)dspfx_strips_coeffs(g, d);              // biquad.rs:66-70, as dspfx_strips_set_band
        else if (code == C_ENV) d[0] = dspfx_envelope_gain(g[0]), d[1] = dspfx_envelope_gain(g[1]);
        for (int r = 0; r < NFIELD; ++r) dev[r * count + i] = d[r];
        uint8_t k = code;
        if (code == C_DIST) k = (uint8_t)(C_DIST + (host_mode ? host_mode[i] : same ? code_mode(old) : (uint32_t)def.mode));
        // a new node starts at rest; a BiQuad store zeroes its state whatever the slot carried (after_settings_change)
        const bool fresh = !same || code == C_BIQUAD;
        codes[i] = fresh ? (uint8_t)(k | C_NEW) : k;
        st.any_new |= fresh;
    }
    p->stores.push(st, [&] {
        for (int t = 0; t < NRAW; ++t) std::memcpy(p->hs[t].data() + at, raw + t * count, count * sizeof(float));
        for (uint64_t i = 0; i < count; ++i) p->hcode[at + i] = codes[i] & (uint8_t)~C_NEW;
    });
    return DSPFX_OK;
}

extern "C" int dspfx_racks_drop(dspfx_racks *p, uint32_t slot, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_slot(p, "drop", slot);
    if (rc != DSPFX_OK) return rc;
    const size_t row = (size_t)slot * p->desc.n_channels;
    return store_slots(p, ST_DROP, "drop", slot, 1, first_channel, count, [=] {
        for (uint64_t c = first_channel; c < first_channel + count; ++c) {     // a later store meets no node: the defaults again
            for (auto &h : p->hs) h[row + c] = 0.0f;
            p->hcode[row + c] = C_NONE;
        }
    });
}

extern "C" int dspfx_racks_reset(dspfx_racks *p, uint32_t slot, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    if (slot == DSPFX_RACKS_NONE) return store_slots(p, ST_RESET, "reset", 0, p->desc.slots, first_channel, count, [] {});
    const int rc = check_slot(p, "reset", slot);
    return rc != DSPFX_OK ? rc : store_slots(p, ST_RESET, "reset", slot, 1, first_channel, count, [] {});
}

extern "C" int dspfx_racks_present(dspfx_racks *p, uint32_t *host_present_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "present", host_present_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) {
        o[i] = 0;
        for (uint32_t t = 0; t < p->desc.slots; ++t) o[i] |= (uint32_t)(p->hcode[(size_t)t * p->desc.n_channels + c] != C_NONE) << t;
    });
}

extern "C" int dspfx_racks_kinds(dspfx_racks *p, uint32_t slot, uint32_t *host_kinds_out, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_slot(p, "kinds", slot);
    if (rc != DSPFX_OK) return rc;
    const size_t row = (size_t)slot * p->desc.n_channels;
    return read_table(p, "kinds", host_kinds_out, first_channel, count, [=](uint32_t *o, uint64_t i, uint64_t c) { o[i] = code_kind(p->hcode[row + c]); });
}

extern "C" int dspfx_racks_modes(dspfx_racks *p, uint32_t slot, uint32_t *host_modes_out, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_slot(p, "modes", slot);
    if (rc != DSPFX_OK) return rc;
    const size_t row = (size_t)slot * p->desc.n_channels;
    return read_table(p, "modes", host_modes_out, first_channel, count, [=](uint32_t *o, uint64_t i, uint64_t c) { o[i] = code_mode(p->hcode[row + c]); });
}

extern "C" int dspfx_racks_sliders(dspfx_racks *p, uint32_t slot, float *host_sliders_out, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_slot(p, "sliders", slot);
    if (rc != DSPFX_OK) return rc;
    const size_t row = (size_t)slot * p->desc.n_channels;
    return read_table(p, "sliders", host_sliders_out, first_channel, count, [=](float *o, uint64_t i, uint64_t c) {
        for (int t = 0; t < NRAW; ++t) o[NRAW * i + t] = p->hs[t][row + c];
    });
}

extern "C" int dspfx_racks_state(dspfx_racks *p, uint32_t slot, const float **state_out) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_slot(p, "state", slot);
    if (rc != DSPFX_OK) return rc;
    if (state_out) *state_out = p->state + (size_t)slot * NSTATE * p->desc.n_channels;
    return DSPFX_OK;
}

extern "C" int dspfx_racks_run(dspfx_racks *p, const float *in, float *out, uint32_t n_frames, void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    hipStream_t s = (hipStream_t)stream;
    const int rc = begin_run(p, in && out, n_frames, s, "racks run: in, out or n_frames", "racks store", apply_store);
    if (rc != DSPFX_OK) return rc;
    RackArgs a;
    a.in = in;
    a.out = out;
    a.field = p->field;
    a.state = p->state;
    a.kind = p->kind;
    a.N = p->desc.n_channels;
    a.W = p->desc.tile_channels;
    a.nf = n_frames;
    a.slots = p->desc.slots;
    const bool vec = lane_plan(a.N, a.W, (uintptr_t)in | (uintptr_t)out, RWG).vec, hv = p->run_heavy != 0;
    switch (p->desc.slots) {                     // a bank of three slots runs the kernel of four, whose last slot is empty
    case 1: launch_run<1>(a, vec, hv, s); break;
    case 2: launch_run<2>(a, vec, hv, s); break;
    default: launch_run<4>(a, vec, hv, s); break;
    }
    BANK_HIP_WHY(hipGetLastError(), "racks_run");
    return DSPFX_OK;
}
