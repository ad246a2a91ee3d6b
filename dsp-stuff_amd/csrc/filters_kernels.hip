// filters_kernels.hip -- the channel-filter bank (include/dspfx.h, dspfx_filters_*): every channel owns `stages` slots (1 .. 4), run
// in slot order, and each slot is empty or carries one of the three chain nodes with one float of state -- LowPass
// (nodes/low_pass.rs:36-39), HighPass (nodes/high_pass.rs:36-39) or Envelope (nodes/envelope.rs:34-52, the node whose OUTPUT is the
// envelope) -- with its own sliders.  An empty slot copies.
//
// One run is one kernel behind the queued stores, in the shape of dynamics_run (dynamics_kernels.hip): time is a serial recurrence
// per channel, so a lane owns its channels for the whole run -- four adjacent channels with one 16-byte load and one nontemporal
// 16-byte store per frame when the layout allows it (lane_io.hip.h), one channel otherwise.  Frames are taken in chunks of F rows
// and the next chunk's loads are issued ahead of this one's arithmetic.  `stages` is a template parameter: every slot's kind, two
// slider floats and state float are registers.  The three recurrences are node_steps.hip.h's, explicit round-to-nearest operations
// in the engine's order (chain_kernels.hip.h, K_LOW_PASS, K_HIGH_PASS, K_ENVELOPE), so a channel's bits are those of an Engine that
// runs its present nodes in slot order.  The kinds differ per lane: before the frame loop the wave ballots once per stage and kind
// (shapers_kernels.hip's scheme), and per chunk and stage it takes one wave-uniform branch.  One kind in the wave (beside empty
// slots): that kind's templated body alone, a result kept under a per-(lane, channel-of-four) select.  Several kinds: one body
// that computes the one-pole and the envelope for every value and selects by the channel's kind -- eight operations where the three
// bodies one after the other are twelve and three pairs of selects (DESIGN section 8 has the times of both pure forms).  A wave
// whose lanes carry no node in a stage does no arithmetic for that stage; no lane ever branches on its own kind.  The tables are [stage][N]: kinds and sliders are read once
// per run, the state is read once and written once.  A lane rewrites only elements it read, so out may be in.  Nothing is shared
// between channels: no LDS, no atomics.
//
// Stores (nodes, drops, resets) go through the staged-store queue (store_queue.hip.h).  Whether a store makes a slot's node NEW
// (its state back to +0.0) is decided on the host, from the host tables, when the store is made; it travels as a flag in the kind
// byte, which filters_fresh takes off again in stream order.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dspfx.h"
#include "channel_bank.hip.h"
#include "lane_io.hip.h"
#include "node_steps.hip.h"

namespace {

constexpr uint32_t FWG = 256;
constexpr uint32_t MAX_STAGES = 4;

// a slot's kind code, one byte.  C_NEW rides on a stored code until filters_fresh has zeroed the slot's state
enum Code : uint8_t { C_NONE = 0, C_LP = 1, C_HP = 2, C_ENV = 3, C_NEW = 0x80 };

struct FiltArgs {
    const float *in;             // may be `out`: no __restrict__
    float *out;
    const float *a, *b;          // [stages][N] each: LowPass, HighPass ratio, - | Envelope attack gain, release gain
    float *z;                    // [stages][N]: the one-pole's z | the envelope
    const uint8_t *kind;         // [stages][N]
    uint32_t N, W, nf;
};

// the lane's slots over a run.  a, b: r and 1 - r of a one-pole, ga and gr of an Envelope
template <int S, int CPL>
struct Lane {
    float z[S][CPL], a[S][CPL], b[S][CPL];
    uint32_t kind[S][CPL];
};

// kind K on R rows of one stage: every value is computed, a channel of kind K keeps the result and the new state; every other
// channel keeps its sample's own bits.  The steps are node_steps.hip.h's:
//   LowPass   z = one_pole_step; y = z
//   HighPass  z = one_pole_step; y = x - z
//   Envelope  z = envelope_step; y = z
template <int K, int CPL, int R>
__device__ __forceinline__ void filt_rows(float (&v)[R][CPL], float (&z)[CPL], const float (&a)[CPL], const float (&b)[CPL], const uint32_t (&kind)[CPL]) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const float x = v[i][j], l = z[j];
            float nz, y;
            if constexpr (K == C_ENV) {
                nz = envelope_step(x, l, a[j], b[j]);
                y = nz;
            } else {
                nz = one_pole_step(x, l, a[j], b[j]);
                y = K == C_HP ? __fsub_rn(x, nz) : nz;
            }
            const bool mine = kind[j] == (uint32_t)K;
            z[j] = mine ? nz : l;
            v[i][j] = mine ? y : x;
        }
    }
}

// ... and all three kinds at once, for a wave whose lanes carry more than one kind in the stage: the one-pole's z and the envelope
// are both computed (five and three operations; a is r or ga, b is 1 - r or gr), and the channel's kind selects
template <int CPL, int R>
__device__ __forceinline__ void filt_rows_any(float (&v)[R][CPL], float (&z)[CPL], const float (&a)[CPL], const float (&b)[CPL], const uint32_t (&kind)[CPL]) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const float x = v[i][j], l = z[j];
            const float e = envelope_step(x, l, a[j], b[j]);
            const float zl = one_pole_step(x, l, a[j], b[j]);
            const float hp = __fsub_rn(x, zl);
            const uint32_t k = kind[j];
            z[j] = k == C_ENV ? e : k == C_NONE ? l : zl;
            v[i][j] = k == C_ENV ? e : k == C_LP ? zl : k == C_HP ? hp : x;
        }
    }
}

// the stages in slot order.  kinds: bit 4 * t + k is set when a lane of the wave carries kind k in stage t (wave-uniform).  One
// kind in the wave: its body alone; several: filt_rows_any; none: nothing
template <int S, int CPL, int R>
__device__ __forceinline__ void filt_stages(uint32_t kinds, float (&v)[R][CPL], Lane<S, CPL> &s) {
#pragma unroll
    for (int t = 0; t < S; ++t) {
        const uint32_t k = (kinds >> (4 * t)) & 0xEu;
        if (k == (1u << C_LP)) filt_rows<C_LP, CPL, R>(v, s.z[t], s.a[t], s.b[t], s.kind[t]);
        else if (k == (1u << C_HP)) filt_rows<C_HP, CPL, R>(v, s.z[t], s.a[t], s.b[t], s.kind[t]);
        else if (k == (1u << C_ENV)) filt_rows<C_ENV, CPL, R>(v, s.z[t], s.a[t], s.b[t], s.kind[t]);
        else if (k) filt_rows_any<CPL, R>(v, s.z[t], s.a[t], s.b[t], s.kind[t]);
    }
}

// F, the frame rows per chunk (two chunks are in registers): 4 with four channels per lane -- 78 / 97 / 117 / 144 VGPRs at
// 1 .. 4 stages, where 8 rows took 138 / 151 / 173 / 202 and ran no faster -- and 8 with one (42 / 54 / 64 / 78 VGPRs).  Scratch is 0 in all eight
template <int S, int CPL>
__global__ __launch_bounds__(FWG) void filters_run(FiltArgs a) {
    constexpr int F = CPL == 4 ? 4 : 8;
    uint32_t c;
    if (!lane_channel<CPL>(FWG, a.N, c)) return;
    Lane<S, CPL> s;
    uint32_t kinds = 0;
#pragma unroll
    for (int t = 0; t < S; ++t) {
        const size_t at = (size_t)t * a.N + c;             // (N % 4 == 0 with CPL = 4: every stage's row is aligned as the first)
        uint8_t code[CPL];
        loadv<CPL>(a.z + at, s.z[t]);
        loadv<CPL>(a.a + at, s.a[t]);
        loadv<CPL>(a.b + at, s.b[t]);
        loadv<CPL>(a.kind + at, code);
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            s.kind[t][j] = code[j];
            if (code[j] == C_LP || code[j] == C_HP) s.b[t][j] = __fsub_rn(1.0f, s.a[t][j]);
        }
#pragma unroll
        for (uint32_t k = C_LP; k <= C_ENV; ++k) {
            bool mine = false;
#pragma unroll
            for (int j = 0; j < CPL; ++j) mine |= s.kind[t][j] == k;
            if (__ballot(mine)) kinds |= 1u << (4 * t + k);        // (the lanes that returned above are not asked)
        }
    }
    kinds = __builtin_amdgcn_readfirstlane(kinds);
    const size_t lane0 = lay(0, c, a.nf, a.N, a.W), rs = a.W ? a.W : a.N;
    const float *lin = a.in + lane0;
    float *lout = a.out + lane0;
    // lane_io's each_chunk, written out: with the helper filters_run<4, 4> kept its 152 registers and measured slower than the
    // spread of five parent runs at 65 536 channels (an empty bank 0.0266 ms for 0.0241, LowPass everywhere 0.0413 for 0.0397)
    const uint32_t nfull = a.nf / F;
    float cur[F][CPL], nxt[F][CPL];
    if (nfull) load_rows<CPL, F>(lin, rs, 0, cur);
#pragma unroll 1
    for (uint32_t ch = 0; ch < nfull; ++ch) {
        if (ch + 1 < nfull) load_rows<CPL, F>(lin, rs, (ch + 1) * F, nxt);
        filt_stages<S, CPL, F>(kinds, cur, s);
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
        filt_stages<S, CPL, 1>(kinds, one, s);
        store_rows<CPL, 1>(lout, rs, f, one);
    }
#pragma unroll
    for (int t = 0; t < S; ++t) storev<CPL, false>(a.z + (size_t)t * a.N + c, s.z[t]);      // (an empty slot: what was read, +0.0)
}

// the device side of a drop, a reset and a kind change, in stream order, on channels [first, first + count) of stages
// [stage, stage + gridDim.y): the state back to +0.0.  only_new: only where the stored code carries C_NEW, which is taken off
__global__ __launch_bounds__(FWG) void filters_fresh(float *__restrict__ z, uint8_t *__restrict__ kind, uint32_t N, uint32_t stage, uint32_t first,
                                                     uint32_t count, bool only_new) {
    const uint32_t i = blockIdx.x * FWG + threadIdx.x;
    if (i >= count) return;
    const size_t at = (size_t)(stage + blockIdx.y) * N + first + i;
    if (only_new) {
        const uint8_t k = kind[at];
        if (!(k & C_NEW)) return;
        kind[at] = k & (uint8_t)~C_NEW;
    }
    z[at] = 0.0f;
}

thread_local std::string g_err;        // the reason of the last failed create or plan on this thread

enum StoreKind : uint32_t { ST_NODES, ST_DROP, ST_RESET };

// a store's vals: NODES four runs of [count]: the device's a and b, the two sliders as they were given (for the host tables), then
// [count] kind codes as bytes; DROP and RESET carry none
struct StoreFields {
    StoreKind kind = ST_RESET;
    uint32_t first = 0, count = 0;
    uint32_t stage = 0, n_stages = 1;            // RESET: stages [stage, stage + n_stages)
    bool any_new = false;                        // NODES: a code carries C_NEW
};
typedef StoreQueue<StoreFields> Stores;
typedef Stores::Store Store;

uint32_t code_kind(uint8_t k) { return k == C_LP ? DSPFX_LOW_PASS : k == C_HP ? DSPFX_HIGH_PASS : k == C_ENV ? DSPFX_ENVELOPE : DSPFX_FILTERS_NONE; }

int check_stages(uint32_t stages, std::string &err) {
    if (stages >= 1 && stages <= MAX_STAGES) return DSPFX_OK;
    char buf[96];
    std::snprintf(buf, sizeof buf, "filters: stages is %u, not 1 .. %u", stages, MAX_STAGES);
    err = buf;
    return DSPFX_ERR_INVALID;
}

}  // namespace

struct dspfx_filters : ChannelBank<dspfx_filters_desc, StoreFields> {
    static constexpr const char *name = "filters";
    std::vector<float> hs[2];                    // [stages][N] each: the sliders as given with every store made so far: ratio, - | attack, release
    std::vector<uint8_t> hkind;                  // [stages][N]: ... and the kind codes
    float *a = nullptr, *b = nullptr, *z = nullptr;
    uint8_t *kind = nullptr;
    // the fresh state: every slot of every channel empty, every table at rest
    template <class V>
    static void tables(const dspfx_filters_desc &d, V v) {
        const uint64_t slots = (uint64_t)d.stages * d.n_channels;
        v(4 * slots, 0, &dspfx_filters::a);
        v(4 * slots, 0, &dspfx_filters::b);
        v(4 * slots, 0, &dspfx_filters::z);
        v(slots, C_NONE, &dspfx_filters::kind);
    }
};

namespace {

// one store onto the stream
hipError_t apply_store(dspfx_filters *p, const Store &st, hipStream_t s) {
    const uint32_t N = p->desc.n_channels;
    const size_t n = st.count, bytes = n * sizeof(float), at = (size_t)st.stage * N + st.first;
    const dim3 grid((st.count + FWG - 1) / FWG, st.n_stages);
    hipError_t err = hipSuccess;
    switch (st.kind) {
    case ST_NODES:
        err = hipMemcpyAsync(p->a + at, st.vals, bytes, hipMemcpyHostToDevice, s);
        if (err == hipSuccess) err = hipMemcpyAsync(p->b + at, st.vals + n, bytes, hipMemcpyHostToDevice, s);
        if (err == hipSuccess) err = hipMemcpyAsync(p->kind + at, st.vals + 4 * n, n, hipMemcpyHostToDevice, s);
        if (err != hipSuccess || !st.any_new) return err;
        filters_fresh<<<grid, FWG, 0, s>>>(p->z, p->kind, N, st.stage, st.first, st.count, true);
        return hipGetLastError();
    case ST_DROP:
        err = hipMemsetAsync(p->kind + at, C_NONE, n, s);
        if (err != hipSuccess) return err;
        [[fallthrough]];
    case ST_RESET:
        filters_fresh<<<grid, FWG, 0, s>>>(p->z, p->kind, N, st.stage, st.first, st.count, false);
        return hipGetLastError();
    }
    return hipSuccess;
}

// `stage` is one of the bank's; the reason is kept
int check_stage(dspfx_filters *p, const char *call, uint32_t stage) {
    if (stage < p->desc.stages) return DSPFX_OK;
    char buf[128];
    std::snprintf(buf, sizeof buf, "filters %s: stage %u is not one of the bank's %u", call, stage, p->desc.stages);
    return p->fail(DSPFX_ERR_INVALID, buf);
}

// a store of one kind into one stage over a range: vals[t] (NULL: keep, or the default where the slot carries another kind or none)
// are the kind's sliders.  The slot's node is NEW where it carried another kind or none, by the host table under smu
int store_nodes(dspfx_filters *p, const char *call, uint8_t code, int n_sliders, const float *const (&vals)[2], const float (&def)[2], uint32_t stage,
                uint64_t first, uint64_t count) {
    int rc = check_stage(p, call, stage);
    if (rc == DSPFX_OK) rc = check_range(p, call, first, count);
    if (rc != DSPFX_OK) return rc;
    if (count == 0) return DSPFX_OK;
    Store st;
    st.stage = stage;
    std::unique_lock<std::mutex> one;
    if (!stage_store(p, st, &one, ST_NODES, call, first, count, 4 * count + (count + 3) / 4, "staged sliders")) return DSPFX_ERR_OOM;
    const size_t at = (size_t)stage * p->desc.n_channels + first;
    float *da = st.vals, *db = da + count, *given[2] = {db + count, db + 2 * count};
    uint8_t *codes = (uint8_t *)(st.vals + 4 * count);
    for (uint64_t i = 0; i < count; ++i) {
        const bool same = p->hkind[at + i] == code;                // the kind it carries: the sliders left out and the state are kept
        for (int t = 0; t < 2; ++t) given[t][i] = t >= n_sliders ? 0.0f : vals[t] ? vals[t][i] : same ? p->hs[t][at + i] : def[t];
        da[i] = code == C_ENV ? dspfx_envelope_gain(given[0][i]) : given[0][i];
        db[i] = code == C_ENV ? dspfx_envelope_gain(given[1][i]) : 0.0f;
        codes[i] = same ? code : (uint8_t)(code | C_NEW);
        st.any_new |= !same;
    }
    p->stores.push(st, [&] {
        for (int t = 0; t < 2; ++t) std::memcpy(p->hs[t].data() + at, given[t], count * sizeof(float));
        std::memset(p->hkind.data() + at, code, count);
    });
    return DSPFX_OK;
}

// channel_bank's store_plain with the stages a drop or a reset names: [stage, stage + n_stages)
template <class Also>
int store_stages(dspfx_filters *p, StoreKind kind, const char *call, uint32_t stage, uint32_t n_stages, uint64_t first, uint64_t count, Also also) {
    return store_plain(p, kind, call, first, count, also, [=](Store &st) {
        st.stage = stage;
        st.n_stages = n_stages;
    });
}

template <int S>
void launch_run(const FiltArgs &a, bool vec, uint32_t blocks, hipStream_t s) {
    if (vec) filters_run<S, 4><<<blocks, FWG, 0, s>>>(a);
    else filters_run<S, 1><<<blocks, FWG, 0, s>>>(a);
}

}  // namespace

extern "C" const char *dspfx_filters_last_error(const dspfx_filters *p) { return p ? p->err.c_str() : g_err.c_str(); }

extern "C" int dspfx_filters_plan(uint64_t channels, uint32_t stages, uint64_t *bytes_out) {
    return plan_bank<dspfx_filters>(channels, bytes_out, g_err, [stages](dspfx_filters_desc &d, std::string &err) {
        d.stages = stages;
        return check_stages(stages, err);
    });
}

extern "C" int dspfx_filters_create(const dspfx_filters_desc *desc, dspfx_filters **out) {
    const int rc = create_checks(desc, out, g_err, [desc](std::string &err) { return check_stages(desc->stages, err); });
    if (rc != DSPFX_OK) return rc;
    return create_bank(desc, out, g_err, [](dspfx_filters *p) {
        const size_t slots = (size_t)p->desc.stages * p->desc.n_channels;
        for (auto &h : p->hs) h.assign(slots, 0.0f);
        p->hkind.assign(slots, C_NONE);
    });
}

extern "C" int dspfx_filters_destroy(dspfx_filters *p) { return destroy_bank(p); }

extern "C" int dspfx_filters_set_low_pass(dspfx_filters *p, uint32_t stage, const float *host_ratio, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const float *const vals[2] = {host_ratio, nullptr};
    return store_nodes(p, "set_low_pass", C_LP, 1, vals, {0.5f, 0.0f}, stage, first_channel, count);
}

extern "C" int dspfx_filters_set_high_pass(dspfx_filters *p, uint32_t stage, const float *host_ratio, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const float *const vals[2] = {host_ratio, nullptr};
    return store_nodes(p, "set_high_pass", C_HP, 1, vals, {0.5f, 0.0f}, stage, first_channel, count);
}

extern "C" int dspfx_filters_set_envelope(dspfx_filters *p, uint32_t stage, const float *host_attack, const float *host_release, uint64_t first_channel,
                                          uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const float *const vals[2] = {host_attack, host_release};
    return store_nodes(p, "set_envelope", C_ENV, 2, vals, {0.0f, 0.0f}, stage, first_channel, count);
}

extern "C" int dspfx_filters_drop(dspfx_filters *p, uint32_t stage, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_stage(p, "drop", stage);
    if (rc != DSPFX_OK) return rc;
    const size_t row = (size_t)stage * p->desc.n_channels;
    return store_stages(p, ST_DROP, "drop", stage, 1, first_channel, count, [=] {
        for (uint64_t c = first_channel; c < first_channel + count; ++c) {     // a later store meets no node: the defaults again
            p->hs[0][row + c] = p->hs[1][row + c] = 0.0f;
            p->hkind[row + c] = C_NONE;
        }
    });
}

extern "C" int dspfx_filters_reset(dspfx_filters *p, uint32_t stage, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    if (stage == DSPFX_FILTERS_NONE) return store_stages(p, ST_RESET, "reset", 0, p->desc.stages, first_channel, count, [] {});
    const int rc = check_stage(p, "reset", stage);
    return rc != DSPFX_OK ? rc : store_stages(p, ST_RESET, "reset", stage, 1, first_channel, count, [] {});
}

extern "C" int dspfx_filters_present(dspfx_filters *p, uint32_t *host_present_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "present", host_present_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) {
        o[i] = 0;
        for (uint32_t t = 0; t < p->desc.stages; ++t) o[i] |= p->hkind[(size_t)t * p->desc.n_channels + c] != C_NONE;
    });
}

extern "C" int dspfx_filters_kinds(dspfx_filters *p, uint32_t stage, uint32_t *host_kinds_out, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_stage(p, "kinds", stage);
    if (rc != DSPFX_OK) return rc;
    const size_t row = (size_t)stage * p->desc.n_channels;
    return read_table(p, "kinds", host_kinds_out, first_channel, count, [=](uint32_t *o, uint64_t i, uint64_t c) { o[i] = code_kind(p->hkind[row + c]); });
}

extern "C" int dspfx_filters_sliders(dspfx_filters *p, uint32_t stage, float *host_sliders_out, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_stage(p, "sliders", stage);
    if (rc != DSPFX_OK) return rc;
    const size_t row = (size_t)stage * p->desc.n_channels;
    return read_table(p, "sliders", host_sliders_out, first_channel, count, [=](float *o, uint64_t i, uint64_t c) {
        for (int t = 0; t < 2; ++t) o[2 * i + t] = p->hs[t][row + c];
    });
}

extern "C" int dspfx_filters_state(dspfx_filters *p, uint32_t stage, const float **state_out) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_stage(p, "state", stage);
    if (rc != DSPFX_OK) return rc;
    if (state_out) *state_out = p->z + (size_t)stage * p->desc.n_channels;
    return DSPFX_OK;
}

extern "C" int dspfx_filters_run(dspfx_filters *p, const float *in, float *out, uint32_t n_frames, void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    hipStream_t s = (hipStream_t)stream;
    const int rc = begin_run(p, in && out, n_frames, s, "filters run: in, out or n_frames", "filters store", apply_store);
    if (rc != DSPFX_OK) return rc;
    FiltArgs a;
    a.in = in;
    a.out = out;
    a.a = p->a;
    a.b = p->b;
    a.z = p->z;
    a.kind = p->kind;
    a.N = p->desc.n_channels;
    a.W = p->desc.tile_channels;
    a.nf = n_frames;
    const auto [vec, lanes, blocks] = lane_plan(a.N, a.W, (uintptr_t)in | (uintptr_t)out, FWG);
    switch (p->desc.stages) {
    case 1: launch_run<1>(a, vec, blocks, s); break;
    case 2: launch_run<2>(a, vec, blocks, s); break;
    case 3: launch_run<3>(a, vec, blocks, s); break;
    default: launch_run<4>(a, vec, blocks, s); break;
    }
    BANK_HIP_WHY(hipGetLastError(), "filters_run");
    return DSPFX_OK;
}
