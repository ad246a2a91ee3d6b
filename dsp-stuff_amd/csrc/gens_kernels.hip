// gens_kernels.hip -- the channel-generator bank (include/dspfx.h, dspfx_gens_*): every channel may carry one Signal Generator node
// of its own (nodes/signal_gen.rs) -- its own amplitude, frequency, mode and clock.  It is the one bank that is a SOURCE: a run reads
// no signal block unless the caller asks for the sample to be added into one (add_to, add.rs) or connects a control port.
//
// One run is one kernel behind the queued stores, in the shape of shapers_run (shapers_kernels.hip): a lane owns four adjacent
// channels with 16-byte loads of add_to and of the control blocks and one nontemporal 16-byte store per frame when the layout allows
// it, one channel otherwise; frames are taken in chunks of F rows and the next chunk's loads are issued ahead of this one's
// arithmetic.  The arithmetic is the engine's own (chain_kernels.hip.h: signal1<MODE>, slider_map, sin_cr), so a channel's bits are
// those of an Engine that runs that one node.  The modes differ per lane: the wave ballots once per run for the mode codes its lanes
// carry (absent is a code of its own) and runs, per chunk, one templated body per mode present, wave-uniformly, keeping a result
// under a per-(lane, channel-of-four) select.  A wave without a Sine channel never enters the f64 sin_cr body; a wave of absent
// channels does no arithmetic.  `total`, the block-local phase advance, is one serial f32 chain per channel: a body walks a channel's
// rows in order from the channel's total and the channel keeps the end of the chain of its own mode.  DIVERGENCE from "step / total
// once for all": signal1 advances the total itself, so in a wave of several modes each body present repeats the chain (one division
// and one addition per sample); a wave of one mode, the common case, pays for it once.
//
// The clock is read once and written once per run; it wraps at every 128-frame block end and at the end of a run that stops inside a
// block, as the engine's does (signal_gen_close_block).  A lane none of whose channels advances a clock (Constant, absent) writes
// nothing.  Stores (sliders and modes, drops, resets) go through the staged-store queue (store_queue.hip.h) as copies and fills: an
// absent channel's clock is +0.0 at all times (create and drop clear it, the kernel never writes it), so a store that creates a node
// finds the clock it must start from.  Nothing is shared between channels: no LDS, no atomics.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dspfx.h"
#include "chain_kernels.hip.h"
#include "channel_bank.hip.h"
#include "lane_io.hip.h"

namespace {

constexpr uint32_t GWG = 256;

// a channel's mode / presence byte: none, or 1 + dspfx_signal_mode
enum Code : uint8_t { C_NONE = 0, C_MODE = 1, C_CONST = C_MODE + DSPFX_SIG_CONSTANT, C_COUNT = 5 };

struct GenArgs {
    const float *add;            // may be `out`: no __restrict__.  nullptr: the sample alone
    const float *cam, *cfr;      // the control blocks of amplitude and frequency, or nullptr
    float *out;
    const float *amp, *freq;     // [N] each: the sliders
    float *clock;                // [N]
    const uint8_t *code;         // [N]
    uint32_t N, W, nf;
};

// the lane's channels over a run
template <int CPL>
struct Lane {
    float amp[CPL], freq[CPL], clock[CPL], total[CPL];
    uint32_t code[CPL];
};

// what a chunk of R rows reads: add_to, and with CTL the two control blocks (mapped to slider values in place)
template <int CPL, int R, bool CTL>
struct Rows {
    float ad[R][CPL];
    float am[CTL ? R : 1][CPL], fr[CTL ? R : 1][CPL];
};

// the lane's pointers to frame 0 of its channels, and which blocks it reads: add for every lane or none, the control blocks only
// where the lane carries a node (an absent channel reads neither)
struct LanePtrs {
    const float *add, *cam, *cfr;
    float *out;
    size_t rs;
};

template <int CPL, int R, bool CTL>
__device__ __forceinline__ void load_chunk(const LanePtrs &l, uint32_t f0, Rows<CPL, R, CTL> &r) {
    if (l.add) load_rows<CPL, R>(l.add, l.rs, f0, r.ad);
    if constexpr (CTL) {
        if (l.cam) load_rows<CPL, R>(l.cam, l.rs, f0, r.am);
        if (l.cfr) load_rows<CPL, R>(l.cfr, l.rs, f0, r.fr);
    }
}

// mode M on R rows: every channel's chain is computed, a channel of mode M keeps the samples and the total
template <int M, int CPL, int R, bool CTL>
__device__ __forceinline__ void gen_rows(float (&v)[R][CPL], Lane<CPL> &s, const Rows<CPL, R, CTL> &r) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const bool mine = s.code[j] == (uint32_t)(C_MODE + M);
        float t = s.total[j];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const float y = dspfx::signal1<M>(s.clock[j], t, CTL ? r.fr[i][j] : s.freq[j], CTL ? r.am[i][j] : s.amp[j]);
            v[i][j] = mine ? y : v[i][j];
        }
        if constexpr (M != dspfx::G_CONSTANT) s.total[j] = mine ? t : s.total[j];
    }
}

// one chunk: the slider values, the body of every mode in `kinds` (a bit per code, the same in every lane of the wave), add_to
template <int CPL, int R, bool CTL>
__device__ __forceinline__ void gen_chunk(uint32_t kinds, Lane<CPL> &s, const LanePtrs &l, Rows<CPL, R, CTL> &r, float (&v)[R][CPL]) {
    if constexpr (CTL) {                                   // dsp-stuff-derive/src/lib.rs:135-153, signal_gen.rs:31-37; no latch
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                r.am[i][j] = l.cam ? dspfx::slider_map(r.am[i][j], -1.0f, 1.0f) : s.amp[j];
                r.fr[i][j] = l.cfr ? dspfx::slider_map(r.fr[i][j], 0.1f, 20000.0f) : s.freq[j];
            }
    }
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < CPL; ++j) v[i][j] = 0.0f;      // an unconnected port (node.rs:162-194)
    while (kinds) {
        const int k = __builtin_ctz(kinds);
        kinds &= kinds - 1;
        switch (k) {
        case C_MODE + DSPFX_SIG_SINE: gen_rows<dspfx::G_SINE, CPL, R, CTL>(v, s, r); break;
        case C_MODE + DSPFX_SIG_TRIANGLE: gen_rows<dspfx::G_TRIANGLE, CPL, R, CTL>(v, s, r); break;
        case C_MODE + DSPFX_SIG_SQUARE: gen_rows<dspfx::G_SQUARE, CPL, R, CTL>(v, s, r); break;
        case C_MODE + DSPFX_SIG_CONSTANT: gen_rows<dspfx::G_CONSTANT, CPL, R, CTL>(v, s, r); break;
        default: break;
        }
    }
    if (l.add) {                                           // add.rs:29-33; without a node the block's own bits
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
            for (int j = 0; j < CPL; ++j) v[i][j] = s.code[j] != C_NONE ? r.ad[i][j] + v[i][j] : r.ad[i][j];
    }
}

// signal_gen.rs:66-67, as the engine closes a block (chain_kernels.hip.h, signal_gen_close_block); Constant leaves the clock alone
template <int CPL>
__device__ __forceinline__ void close_block(Lane<CPL> &s) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const float w = fmodf(s.clock[j] + s.total[j], 1.0f);
        const bool runs = s.code[j] != C_NONE && s.code[j] != C_CONST;
        s.clock[j] = runs ? w : s.clock[j];
        s.total[j] = 0.0f;
    }
}

// CTL: a control block is connected (the host knows); without, the kernel holds no control rows at all
template <int CPL, bool CTL>
__global__ __launch_bounds__(GWG) void gens_run(GenArgs a) {
    constexpr int F = CTL ? 4 : 8;                         // frame rows per chunk (two chunks are in registers); F divides 128
    uint32_t c;
    if (!lane_channel<CPL>(GWG, a.N, c)) return;
    Lane<CPL> s;
    uint8_t code[CPL];
    loadv<CPL>(a.amp + c, s.amp);
    loadv<CPL>(a.freq + c, s.freq);
    loadv<CPL>(a.clock + c, s.clock);
    loadv<CPL>(a.code + c, code);
    bool node = false, runs = false;                       // the lane carries a node; ... one that advances a clock
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        s.code[j] = code[j];
        s.total[j] = 0.0f;
        node |= code[j] != C_NONE;
        runs |= code[j] != C_NONE && code[j] != C_CONST;
    }
    uint32_t kinds = 0;
#pragma unroll
    for (uint32_t k = C_MODE; k < C_COUNT; ++k) {
        bool mine = false;
#pragma unroll
        for (int j = 0; j < CPL; ++j) mine |= s.code[j] == k;
        if (__ballot(mine)) kinds |= 1u << k;              // (the lanes that returned above are not asked)
    }
    kinds = __builtin_amdgcn_readfirstlane(kinds);
    const bool clocked = (kinds & ~(1u << C_CONST)) != 0;  // the wave has a channel whose clock advances
    const size_t lane0 = lay(0, c, a.nf, a.N, a.W);
    LanePtrs l;
    l.rs = a.W ? a.W : a.N;
    l.add = a.add ? a.add + lane0 : nullptr;
    l.cam = CTL && a.cam && node ? a.cam + lane0 : nullptr;
    l.cfr = CTL && a.cfr && node ? a.cfr + lane0 : nullptr;
    l.out = a.out + lane0;
    // lane_io's each_chunk over the bank's own Rows (up to three streams in) and with close_block inside the loop: its own loop
    const uint32_t nfull = a.nf / F;
    Rows<CPL, F, CTL> cur, nxt;
    if (nfull) load_chunk<CPL, F, CTL>(l, 0, cur);
#pragma unroll 1
    for (uint32_t ch = 0; ch < nfull; ++ch) {
        if (ch + 1 < nfull) load_chunk<CPL, F, CTL>(l, (ch + 1) * F, nxt);
        float v[F][CPL];
        gen_chunk<CPL, F, CTL>(kinds, s, l, cur, v);
        store_rows<CPL, F>(l.out, l.rs, ch * F, v);
        if (clocked && (((ch + 1) * F) & 127u) == 0) close_block<CPL>(s);      // a reference block ends with this chunk
        cur = nxt;
    }
#pragma unroll 1
    for (uint32_t f = nfull * F; f < a.nf; ++f) {
        Rows<CPL, 1, CTL> one;
        float v[1][CPL];
        load_chunk<CPL, 1, CTL>(l, f, one);
        gen_chunk<CPL, 1, CTL>(kinds, s, l, one, v);
        store_rows<CPL, 1>(l.out, l.rs, f, v);
    }
    if (clocked && (a.nf & 127u)) close_block<CPL>(s);     // the run stops inside a block
    if (runs) storev<CPL, false>(a.clock + c, s.clock);
}

thread_local std::string g_err;        // the reason of the last failed create or plan on this thread

enum StoreKind : uint32_t { ST_SET, ST_DROP, ST_RESET };

// a store's vals: SET two runs of [count] sliders (amplitude, frequency), then [count] codes as bytes; DROP and RESET carry none
struct StoreFields {
    StoreKind kind = ST_DROP;
    uint32_t first = 0, count = 0;
};
typedef StoreQueue<StoreFields> Stores;
typedef Stores::Store Store;

}  // namespace

struct dspfx_gens : ChannelBank<dspfx_gens_desc, StoreFields> {
    static constexpr const char *name = "gens";
    std::vector<float> hamp, hfreq;              // [N] each: the sliders with every store made so far
    std::vector<uint8_t> hcode;                  // [N]: ... and the mode / presence bytes
    float *amp = nullptr, *freq = nullptr, *clock = nullptr;
    uint8_t *code = nullptr;
    // the fresh state: no node anywhere, every clock +0.0
    template <class V>
    static void tables(const dspfx_gens_desc &d, V v) {
        const uint64_t N = d.n_channels;
        v(4 * N, 0, &dspfx_gens::amp);
        v(4 * N, 0, &dspfx_gens::freq);
        v(4 * N, 0, &dspfx_gens::clock);
        v(N, C_NONE, &dspfx_gens::code);
    }
};

namespace {

// one store onto the stream (the bank's mu is held).  A channel without a node has clock +0.0 at all times, so SET writes no clock
hipError_t apply_store(dspfx_gens *p, const Store &st, hipStream_t s) {
    const size_t n = st.count, bytes = n * sizeof(float);
    hipError_t err = hipSuccess;
    switch (st.kind) {
    case ST_SET:
        err = hipMemcpyAsync(p->amp + st.first, st.vals, bytes, hipMemcpyHostToDevice, s);
        if (err == hipSuccess) err = hipMemcpyAsync(p->freq + st.first, st.vals + n, bytes, hipMemcpyHostToDevice, s);
        if (err == hipSuccess) err = hipMemcpyAsync(p->code + st.first, st.vals + 2 * n, n, hipMemcpyHostToDevice, s);
        break;
    case ST_DROP:
        err = hipMemsetAsync(p->code + st.first, C_NONE, n, s);
        if (err == hipSuccess) err = hipMemsetAsync(p->clock + st.first, 0, bytes, s);
        break;
    case ST_RESET:
        err = hipMemsetAsync(p->clock + st.first, 0, bytes, s);
        break;
    }
    return err;
}

}  // namespace

extern "C" const char *dspfx_gens_last_error(const dspfx_gens *p) { return p ? p->err.c_str() : g_err.c_str(); }

extern "C" int dspfx_gens_plan(uint64_t channels, uint64_t *bytes_out) { return plan_bank<dspfx_gens>(channels, bytes_out, g_err); }

extern "C" int dspfx_gens_create(const dspfx_gens_desc *desc, dspfx_gens **out) {
    const int rc = create_checks(desc, out, g_err);
    if (rc != DSPFX_OK) return rc;
    return create_bank(desc, out, g_err, [](dspfx_gens *p) {
        const uint32_t N = p->desc.n_channels;
        p->hamp.assign(N, 0.0f);
        p->hfreq.assign(N, 0.0f);
        p->hcode.assign(N, C_NONE);
    });
}

extern "C" int dspfx_gens_destroy(dspfx_gens *p) { return destroy_bank(p); }

extern "C" int dspfx_gens_set(dspfx_gens *p, const float *host_amplitude, const float *host_frequency, const uint32_t *host_mode,
                              uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_range(p, "set", first_channel, count);
    if (rc != DSPFX_OK) return rc;
    if (host_mode)
        for (uint64_t i = 0; i < count; ++i)
            if (host_mode[i] > DSPFX_SIG_CONSTANT) {
                char buf[192];
                std::snprintf(buf, sizeof buf, "gens set: channel %llu is given mode %u, which is no Signal Generator mode (0 .. %d)",
                              (unsigned long long)(first_channel + i), host_mode[i], (int)DSPFX_SIG_CONSTANT);
                return p->fail(DSPFX_ERR_INVALID, buf);
            }
    if (count == 0) return DSPFX_OK;
    dspfx_node_desc def;
    if (dspfx_node_defaults(DSPFX_SIGNAL_GEN, &def) != DSPFX_OK) return p->fail(DSPFX_ERR_INVALID, "gens: no such node kind");
    Store st;
    std::unique_lock<std::mutex> one;
    if (!stage_store(p, st, &one, ST_SET, "set", first_channel, count, 2 * count + (count + 3) / 4, "staged sliders")) return DSPFX_ERR_OOM;
    uint8_t *codes = (uint8_t *)(st.vals + 2 * count);
    for (uint64_t i = 0; i < count; ++i) {
        const uint64_t c = first_channel + i;
        const uint8_t old = p->hcode[c];                         // a node it carries keeps what the call leaves out (and its clock)
        st.vals[i] = host_amplitude ? host_amplitude[i] : old ? p->hamp[c] : def.params[0];
        st.vals[count + i] = host_frequency ? host_frequency[i] : old ? p->hfreq[c] : def.params[1];
        codes[i] = host_mode ? (uint8_t)(C_MODE + host_mode[i]) : old ? old : (uint8_t)(C_MODE + def.mode);
    }
    p->stores.push(st, [&] {
        std::memcpy(p->hamp.data() + first_channel, st.vals, count * sizeof(float));
        std::memcpy(p->hfreq.data() + first_channel, st.vals + count, count * sizeof(float));
        std::memcpy(p->hcode.data() + first_channel, codes, count);
    });
    return DSPFX_OK;
}

extern "C" int dspfx_gens_drop(dspfx_gens *p, uint64_t first_channel, uint64_t count) {
    return store_plain(p, ST_DROP, "drop", first_channel, count, [=] {
        for (uint64_t c = first_channel; c < first_channel + count; ++c) {     // a later store meets no node: the defaults again
            p->hamp[c] = p->hfreq[c] = 0.0f;
            p->hcode[c] = C_NONE;
        }
    });
}

extern "C" int dspfx_gens_reset(dspfx_gens *p, uint64_t first_channel, uint64_t count) { return store_plain(p, ST_RESET, "reset", first_channel, count); }

extern "C" int dspfx_gens_present(dspfx_gens *p, uint32_t *host_present_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "present", host_present_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = p->hcode[c] != C_NONE; });
}

extern "C" int dspfx_gens_modes(dspfx_gens *p, uint32_t *host_modes_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "modes", host_modes_out, first_channel, count,
                      [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = p->hcode[c] ? (uint32_t)(p->hcode[c] - C_MODE) : DSPFX_GENS_NONE; });
}

extern "C" int dspfx_gens_sliders(dspfx_gens *p, float *host_sliders_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "sliders", host_sliders_out, first_channel, count, [p](float *o, uint64_t i, uint64_t c) {
        o[2 * i] = p->hamp[c];
        o[2 * i + 1] = p->hfreq[c];
    });
}

extern "C" int dspfx_gens_clocks(dspfx_gens *p, const float **clock_out) {
    if (!p) return DSPFX_ERR_INVALID;
    if (!clock_out) return p->fail(DSPFX_ERR_INVALID, "gens clocks: no pointer");
    *clock_out = p->clock;
    return DSPFX_OK;
}

extern "C" int dspfx_gens_run(dspfx_gens *p, const float *add_to, const float *amplitude, const float *frequency, float *out, uint32_t n_frames,
                              void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    hipStream_t s = (hipStream_t)stream;
    const int rc = begin_run(p, out != nullptr, n_frames, s, "gens run: out or n_frames", "gens store", apply_store);
    if (rc != DSPFX_OK) return rc;
    GenArgs a;
    a.add = add_to;
    a.cam = amplitude;
    a.cfr = frequency;
    a.out = out;
    a.amp = p->amp;
    a.freq = p->freq;
    a.clock = p->clock;
    a.code = p->code;
    a.N = p->desc.n_channels;
    a.W = p->desc.tile_channels;
    a.nf = n_frames;
    const auto [vec, lanes, blocks] = lane_plan(a.N, a.W, (uintptr_t)out | (uintptr_t)add_to | (uintptr_t)amplitude | (uintptr_t)frequency, GWG);
    const bool ctl = amplitude || frequency;
    if (vec && ctl) gens_run<4, true><<<blocks, GWG, 0, s>>>(a);
    else if (vec) gens_run<4, false><<<blocks, GWG, 0, s>>>(a);
    else if (ctl) gens_run<1, true><<<blocks, GWG, 0, s>>>(a);
    else gens_run<1, false><<<blocks, GWG, 0, s>>>(a);
    BANK_HIP_WHY(hipGetLastError(), "gens_run");
    return DSPFX_OK;
}
