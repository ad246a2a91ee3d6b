// blends_kernels.hip -- the channel-blend bank (include/dspfx.h, dspfx_blends_*): every channel may carry one Add node (nodes/add.rs)
// or one Mix node with a ratio of its own (nodes/mix.rs), and a Gain node (gain.rs) on the node's `b` input, the channel's send.  The
// second input is an N-channel block, or a [n_frames][buses] frame-major bus block that a channel reads through its bus id, or
// nothing (an unconnected port, +0.0).
//
// One run is one kernel behind the queued stores, in the shape of gens_run (gens_kernels.hip): a lane owns four adjacent channels
// with 16-byte loads of a, b and the control block and one nontemporal 16-byte store per frame when the layout allows it, one channel
// otherwise; frames are taken in chunks of F rows and the next chunk's loads are issued ahead of this one's arithmetic.  The three
// kinds (none, Add, Mix) are a handful of VALU operations, so every channel computes both and keeps one under a select; the
// expressions are the engine's (chain_kernels.hip.h, apply_node<K_ADD / K_MIX>, slider_map), so a channel's bits are those of an
// Engine that runs that one node.  A lane none of whose channels carries a node reads neither b, the bus nor the control block: it
// copies a.  The kernel is templated on the second input and on whether a control block is connected; a run without either holds no
// rows for them.
//
// Bus mode: each channel gathers bus[f][bus_of[c]] itself.  The bus block is small and stays in L2, and where rooms are whole spans
// of channels the lanes of a wave read one address per frame, which the memory pipeline serves as one request.  A separate path that
// ballots once per run for "the wave shares one bus id" and reads through a wave-uniform address was built and timed at 2^20
// channels x 128 frames, 4096 contiguous rooms of 256: 0.2710 ms against this gather's 0.2181 ms.  It lost and is not here.
// Nothing is shared between channels: no LDS, no atomics.
//
// Stores (set_mix, set_add, set_send, assign, drop) go through the staged-store queue (store_queue.hip.h) as copies and fills.  The
// kind and the send's presence share one byte per channel; a store computes the byte from the host table under the bank's store lock,
// so each store is whole.
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

constexpr uint32_t BWG = 256;

// a channel's byte: the node in the low two bits, the send's presence above them
enum Code : uint8_t { C_NONE = 0, C_ADD = 1, C_MIX = 2, C_KIND = 3, C_SEND = 4 };
// the second input of a run
enum Src : int { S_NONE = 0, S_BLOCK = 1, S_BUS = 2 };

struct BlendArgs {
    const float *a, *b;          // either may be `out`: no __restrict__.  b: S_BLOCK only
    const float *bus;            // [nf][G] frame-major, S_BUS only
    const float *ctl;            // the control block of the ratio, or nullptr
    float *out;
    const float *ratio, *level;  // [N] each
    const uint32_t *bus_of;      // [N]: below G, or DSPFX_BLENDS_NO_BUS
    const uint8_t *code;         // [N]
    uint32_t N, W, nf, G;
};

// the lane's channels over a run
template <int CPL>
struct Lane {
    float ratio[CPL], level[CPL];
    uint32_t code[CPL], bus[CPL];
};

// what a chunk of R rows reads: a, with SRC the second input, with CTL the control block
template <int CPL, int R, int SRC, bool CTL>
struct Rows {
    float a[R][CPL];
    float b[SRC ? R : 1][CPL];
    float ct[CTL ? R : 1][CPL];
};

// the lane's pointers to frame 0 of its channels.  b, bus and ctl are nullptr where the lane carries no node: it reads none of them
struct LanePtrs {
    const float *a, *b, *bus, *ctl;
    float *out;
    size_t rs;
    uint32_t G;
};

template <int CPL, int R, int SRC, bool CTL>
__device__ __forceinline__ void load_chunk(const LanePtrs &l, const Lane<CPL> &s, uint32_t f0, Rows<CPL, R, SRC, CTL> &r) {
    load_rows<CPL, R>(l.a, l.rs, f0, r.a);
    if constexpr (SRC == S_BLOCK) {
        if (l.b) load_rows<CPL, R>(l.b, l.rs, f0, r.b);
    }
    if constexpr (SRC == S_BUS) {
        if (l.bus) {
#pragma unroll
            for (int i = 0; i < R; ++i)
#pragma unroll
                for (int j = 0; j < CPL; ++j) r.b[i][j] = s.bus[j] != DSPFX_BLENDS_NO_BUS ? l.bus[(size_t)(f0 + i) * l.G + s.bus[j]] : 0.0f;
        }
    }
    if constexpr (CTL) {
        if (l.ctl) load_rows<CPL, R>(l.ctl, l.rs, f0, r.ct);
    }
}

// one chunk: gain.rs:33-37 on b where the channel has a send, then add.rs:29-33 and mix.rs:41-46 under the channel's select; without
// a node a's very bits.  Every weight is a multiplication
template <int CPL, int R, int SRC, bool CTL>
__device__ __forceinline__ void blend_chunk(const Lane<CPL> &s, const LanePtrs &l, const Rows<CPL, R, SRC, CTL> &r, float (&v)[R][CPL]) {
    const bool node = SRC == S_BLOCK ? l.b != nullptr : SRC == S_BUS ? l.bus != nullptr : true;
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const uint32_t kind = s.code[j] & C_KIND;
            float bb = SRC != S_NONE && node ? r.b[i][j] : 0.0f;          // an unconnected port (node.rs:288)
            bb = (s.code[j] & C_SEND) ? bb * s.level[j] : bb;
            float ra = s.ratio[j];
            if constexpr (CTL) ra = l.ctl ? dspfx::slider_map(r.ct[i][j], 0.0f, 1.0f) : ra;      // dsp-stuff-derive/src/lib.rs:135-153; no latch
            const float a = r.a[i][j];
            const float add = a + bb;
            const float mix = (bb * ra) + (a * (1.0f - ra));
            v[i][j] = kind == C_ADD ? add : kind == C_MIX ? mix : a;
        }
}

// SRC: the second input; CTL: a control block is connected (the host knows both)
template <int CPL, int SRC, bool CTL>
__global__ __launch_bounds__(BWG) void blends_run(BlendArgs g) {
    constexpr int F = (SRC != S_NONE || CTL) ? 4 : 8;      // frame rows per chunk (two chunks are in registers)
    uint32_t c;
    if (!lane_channel<CPL>(BWG, g.N, c)) return;
    Lane<CPL> s;
    uint8_t code[CPL];
    loadv<CPL>(g.code + c, code);
    bool node = false, mixes = false;                      // the lane carries a node; ... a Mix node
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        s.code[j] = code[j];
        s.ratio[j] = s.level[j] = 0.0f;
        s.bus[j] = DSPFX_BLENDS_NO_BUS;
        node |= (code[j] & C_KIND) != C_NONE;
        mixes |= (code[j] & C_KIND) == C_MIX;
    }
    if (node) {
        loadv<CPL>(g.ratio + c, s.ratio);
        loadv<CPL>(g.level + c, s.level);
        if constexpr (SRC == S_BUS) loadv<CPL>(g.bus_of + c, s.bus);
    }
    const size_t lane0 = lay(0, c, g.nf, g.N, g.W);
    LanePtrs l;
    l.rs = g.W ? g.W : g.N;
    l.G = g.G;
    l.a = g.a + lane0;
    l.out = g.out + lane0;
    l.b = SRC == S_BLOCK && node ? g.b + lane0 : nullptr;
    l.bus = SRC == S_BUS && node ? g.bus : nullptr;
    l.ctl = CTL && mixes ? g.ctl + lane0 : nullptr;
    // lane_io's each_chunk over the bank's own Rows (up to three streams in) and a separate row of results: its own loop
    const uint32_t nfull = g.nf / F;
    Rows<CPL, F, SRC, CTL> cur, nxt;
    if (nfull) load_chunk<CPL, F, SRC, CTL>(l, s, 0, cur);
#pragma unroll 1
    for (uint32_t ch = 0; ch < nfull; ++ch) {
        if (ch + 1 < nfull) load_chunk<CPL, F, SRC, CTL>(l, s, (ch + 1) * F, nxt);
        float v[F][CPL];
        blend_chunk<CPL, F, SRC, CTL>(s, l, cur, v);
        store_rows<CPL, F>(l.out, l.rs, ch * F, v);
        cur = nxt;
    }
#pragma unroll 1
    for (uint32_t f = nfull * F; f < g.nf; ++f) {
        Rows<CPL, 1, SRC, CTL> one;
        float v[1][CPL];
        load_chunk<CPL, 1, SRC, CTL>(l, s, f, one);
        blend_chunk<CPL, 1, SRC, CTL>(s, l, one, v);
        store_rows<CPL, 1>(l.out, l.rs, f, v);
    }
}

thread_local std::string g_err;        // the reason of the last failed create or plan on this thread

// what a store copies: [count] 4-byte values into one table (or none), then [count] code bytes (or none); DROP fills instead
enum StoreKind : uint32_t { ST_COPY, ST_DROP };
enum Table : uint32_t { T_NONE, T_RATIO, T_LEVEL, T_BUS };

struct StoreFields {
    StoreKind kind = ST_DROP;
    Table table = T_NONE;
    bool codes = false;
    uint32_t first = 0, count = 0;
};
typedef StoreQueue<StoreFields> Stores;
typedef Stores::Store Store;

}  // namespace

struct dspfx_blends : ChannelBank<dspfx_blends_desc, StoreFields> {
    static constexpr const char *name = "blends";
    std::vector<float> hratio, hlevel;           // [N] each, with every store made so far; 0 without a Mix node / without a send
    std::vector<uint32_t> hbus;                  // [N]
    std::vector<uint8_t> hcode;                  // [N]
    float *ratio = nullptr, *level = nullptr;
    uint32_t *bus_of = nullptr;
    uint8_t *code = nullptr;
    // the fresh state: no node and no send anywhere, every channel on no bus
    template <class V>
    static void tables(const dspfx_blends_desc &d, V v) {
        const uint64_t N = d.n_channels;
        v(4 * N, 0, &dspfx_blends::ratio);
        v(4 * N, 0, &dspfx_blends::level);
        v(4 * N, 0xFF, &dspfx_blends::bus_of);
        v(N, C_NONE, &dspfx_blends::code);
    }
};

namespace {

// one store onto the stream (the bank's mu is held)
hipError_t apply_store(dspfx_blends *p, const Store &st, hipStream_t s) {
    const size_t n = st.count, bytes = n * sizeof(float);
    if (st.kind == ST_DROP) return hipMemsetAsync(p->code + st.first, C_NONE, n, s);
    hipError_t err = hipSuccess;
    void *dst = st.table == T_RATIO ? (void *)(p->ratio + st.first) : st.table == T_LEVEL ? (void *)(p->level + st.first) : (void *)(p->bus_of + st.first);
    if (st.table != T_NONE) err = hipMemcpyAsync(dst, st.vals, bytes, hipMemcpyHostToDevice, s);
    if (err == hipSuccess && st.codes) err = hipMemcpyAsync(p->code + st.first, st.vals + (st.table != T_NONE ? n : 0), n, hipMemcpyHostToDevice, s);
    return err;
}

// a staged store over a range (the range is checked, count > 0): fill(values, codes) writes what it stages -- either may be absent
// -- reading the host tables; then the host tables take the same values as the store joins the queue
template <class Fill>
int store_copy(dspfx_blends *p, const char *call, Table table, bool codes, uint64_t first, uint64_t count, Fill fill) {
    Store st;
    st.table = table;
    st.codes = codes;
    std::unique_lock<std::mutex> one;
    if (!stage_store(p, st, &one, ST_COPY, call, first, count, (table != T_NONE ? count : 0) + (codes ? (count + 3) / 4 : 0), "staged values"))
        return DSPFX_ERR_OOM;
    float *vals = table != T_NONE ? st.vals : nullptr;
    uint8_t *cs = codes ? (uint8_t *)(st.vals + (table != T_NONE ? count : 0)) : nullptr;
    fill(vals, cs);
    p->stores.push(st, [&] {
        if (table == T_RATIO) std::memcpy(p->hratio.data() + first, vals, count * sizeof(float));
        if (table == T_LEVEL) std::memcpy(p->hlevel.data() + first, vals, count * sizeof(float));
        if (table == T_BUS) std::memcpy(p->hbus.data() + first, vals, count * sizeof(float));
        if (codes) std::memcpy(p->hcode.data() + first, cs, count);
    });
    return DSPFX_OK;
}

}  // namespace

extern "C" const char *dspfx_blends_last_error(const dspfx_blends *p) { return p ? p->err.c_str() : g_err.c_str(); }

extern "C" int dspfx_blends_plan(uint64_t channels, uint64_t *bytes_out) { return plan_bank<dspfx_blends>(channels, bytes_out, g_err); }

extern "C" int dspfx_blends_create(const dspfx_blends_desc *desc, dspfx_blends **out) {
    const int rc = create_checks(desc, out, g_err);
    if (rc != DSPFX_OK) return rc;
    return create_bank(desc, out, g_err, [](dspfx_blends *p) {
        const uint32_t N = p->desc.n_channels;
        p->hratio.assign(N, 0.0f);
        p->hlevel.assign(N, 0.0f);
        p->hbus.assign(N, DSPFX_BLENDS_NO_BUS);
        p->hcode.assign(N, C_NONE);
    });
}

extern "C" int dspfx_blends_destroy(dspfx_blends *p) { return destroy_bank(p); }

extern "C" int dspfx_blends_set_mix(dspfx_blends *p, const float *host_ratio, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_range(p, "set_mix", first_channel, count);
    if (rc != DSPFX_OK || count == 0) return rc;
    dspfx_node_desc def;
    if (dspfx_node_defaults(DSPFX_MIX, &def) != DSPFX_OK) return p->fail(DSPFX_ERR_INVALID, "blends: no such node kind");
    return store_copy(p, "set_mix", T_RATIO, true, first_channel, count, [&](float *vals, uint8_t *cs) {
        for (uint64_t i = 0; i < count; ++i) {
            const uint64_t c = first_channel + i;
            const uint8_t old = p->hcode[c];                         // a Mix node keeps the ratio the call leaves out
            vals[i] = host_ratio ? host_ratio[i] : (old & C_KIND) == C_MIX ? p->hratio[c] : def.params[0];
            cs[i] = (uint8_t)((old & C_SEND) | C_MIX);
        }
    });
}

extern "C" int dspfx_blends_set_add(dspfx_blends *p, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_range(p, "set_add", first_channel, count);
    if (rc != DSPFX_OK || count == 0) return rc;
    return store_copy(p, "set_add", T_RATIO, true, first_channel, count, [&](float *vals, uint8_t *cs) {
        for (uint64_t i = 0; i < count; ++i) {
            vals[i] = 0.0f;                                          // an Add node has no ratio
            cs[i] = (uint8_t)((p->hcode[first_channel + i] & C_SEND) | C_ADD);
        }
    });
}

extern "C" int dspfx_blends_set_send(dspfx_blends *p, const float *host_level, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_range(p, "set_send", first_channel, count);
    if (rc != DSPFX_OK || count == 0) return rc;
    return store_copy(p, "set_send", T_LEVEL, true, first_channel, count, [&](float *vals, uint8_t *cs) {
        for (uint64_t i = 0; i < count; ++i) {
            const uint8_t kind = p->hcode[first_channel + i] & C_KIND;
            vals[i] = host_level ? host_level[i] : 0.0f;
            cs[i] = (uint8_t)(host_level ? kind | C_SEND : kind);    // NULL: the Gain node is gone
        }
    });
}

extern "C" int dspfx_blends_assign(dspfx_blends *p, const uint32_t *host_ids, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    if (!host_ids && count) return p->fail(DSPFX_ERR_INVALID, "blends assign: no ids");
    const int rc = check_range(p, "assign", first_channel, count);
    if (rc != DSPFX_OK) return rc;
    for (uint64_t i = 0; i < count; ++i)
        if (host_ids[i] != DSPFX_BLENDS_NO_BUS && host_ids[i] >= p->desc.n_buses) {
            char buf[192];
            std::snprintf(buf, sizeof buf, "blends assign: channel %llu is given bus %u, which is neither below the bank's %u buses nor DSPFX_BLENDS_NO_BUS",
                          (unsigned long long)(first_channel + i), host_ids[i], p->desc.n_buses);
            return p->fail(DSPFX_ERR_INVALID, buf);
        }
    if (count == 0) return DSPFX_OK;
    return store_copy(p, "assign", T_BUS, false, first_channel, count, [&](float *vals, uint8_t *) { std::memcpy(vals, host_ids, count * sizeof(uint32_t)); });
}

extern "C" int dspfx_blends_drop(dspfx_blends *p, uint64_t first_channel, uint64_t count) {
    return store_plain(p, ST_DROP, "drop", first_channel, count, [=] {
        for (uint64_t c = first_channel; c < first_channel + count; ++c) {     // the bus id stays
            p->hratio[c] = p->hlevel[c] = 0.0f;
            p->hcode[c] = C_NONE;
        }
    });
}

extern "C" int dspfx_blends_kinds(dspfx_blends *p, uint32_t *host_kinds_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "kinds", host_kinds_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) {
        const uint8_t k = p->hcode[c] & C_KIND;
        o[i] = k == C_ADD ? (uint32_t)DSPFX_ADD : k == C_MIX ? (uint32_t)DSPFX_MIX : DSPFX_BLENDS_NONE;
    });
}

extern "C" int dspfx_blends_ratios(dspfx_blends *p, float *host_ratios_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "ratios", host_ratios_out, first_channel, count, [p](float *o, uint64_t i, uint64_t c) { o[i] = p->hratio[c]; });
}

extern "C" int dspfx_blends_sends(dspfx_blends *p, float *host_levels_out, uint32_t *host_present_out, uint64_t first_channel, uint64_t count) {
    if (p && !host_present_out) return p->fail(DSPFX_ERR_INVALID, "blends sends: no array");
    return read_table(p, "sends", host_levels_out, first_channel, count, [p, host_present_out](float *o, uint64_t i, uint64_t c) {
        o[i] = p->hlevel[c];
        host_present_out[i] = (p->hcode[c] & C_SEND) != 0;
    });
}

extern "C" int dspfx_blends_bus_of(dspfx_blends *p, uint32_t *host_ids_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "bus_of", host_ids_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = p->hbus[c]; });
}

namespace {

template <int CPL, int SRC>
void launch(const BlendArgs &g, bool ctl, uint32_t blocks, hipStream_t s) {
    if (ctl) blends_run<CPL, SRC, true><<<blocks, BWG, 0, s>>>(g);
    else blends_run<CPL, SRC, false><<<blocks, BWG, 0, s>>>(g);
}

template <int CPL>
void launch(const BlendArgs &g, int src, bool ctl, uint32_t blocks, hipStream_t s) {
    if (src == S_BLOCK) launch<CPL, S_BLOCK>(g, ctl, blocks, s);
    else if (src == S_BUS) launch<CPL, S_BUS>(g, ctl, blocks, s);
    else launch<CPL, S_NONE>(g, ctl, blocks, s);
}

}  // namespace

extern "C" int dspfx_blends_run(dspfx_blends *p, const float *a, const float *b, const float *bus, const float *ratio, float *out, uint32_t n_frames,
                                void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    if (b && bus) return p->fail(DSPFX_ERR_INVALID, "blends run: both b and bus are given; a run has one second input");
    if (bus && p->desc.n_buses == 0) return p->fail(DSPFX_ERR_INVALID, "blends run: bus is given, but the bank was created with n_buses = 0");
    hipStream_t s = (hipStream_t)stream;
    const int rc = begin_run(p, a != nullptr && out != nullptr, n_frames, s, "blends run: a, out or n_frames", "blends store", apply_store);
    if (rc != DSPFX_OK) return rc;
    BlendArgs g;
    g.a = a;
    g.b = b;
    g.bus = bus;
    g.ctl = ratio;
    g.out = out;
    g.ratio = p->ratio;
    g.level = p->level;
    g.bus_of = p->bus_of;
    g.code = p->code;
    g.N = p->desc.n_channels;
    g.W = p->desc.tile_channels;
    g.nf = n_frames;
    g.G = p->desc.n_buses;
    const auto [vec, lanes, blocks] = lane_plan(g.N, g.W, (uintptr_t)out | (uintptr_t)a | (uintptr_t)b | (uintptr_t)ratio, BWG);
    (void)lanes;
    const int src = b ? S_BLOCK : bus ? S_BUS : S_NONE;
    if (vec) launch<4>(g, src, ratio != nullptr, blocks, s);
    else launch<1>(g, src, ratio != nullptr, blocks, s);
    BANK_HIP_WHY(hipGetLastError(), "blends_run");
    return DSPFX_OK;
}
