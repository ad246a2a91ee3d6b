// strips_kernels.hip -- the channel-strip bank (include/dspfx.h, dspfx_strips_*): every channel has its own chain of up to
// 1 + K optional nodes in a fixed order, a Gain node (gain.rs:25-38) and BiQuad bands 0 .. K-1 (biquad.rs:62-88), each with
// the channel's own slider values.  What the reference has when N graphs each hold their own node instances.
//
// One streaming pass: the block is read once and written once.  Time is a serial recurrence per channel, so a lane owns its
// channels for the whole block: four adjacent channels with one 16-byte load and one nontemporal 16-byte store per frame when
// the layout allows it (lane_io.hip.h), one channel otherwise -- and at K > 4, where the coefficients and the state of four
// channels (9 x 4 x 8 values) no longer fit in registers beside the frames.  A lane's coefficients ([band][5][N]), state
// ([band][4][N]), level ([N]) and node mask ([N]) are read once per block into registers; adjacent lanes read adjacent
// addresses in all of them.  Frames are taken in chunks of F rows; the next chunk's loads are issued before the arithmetic of
// this one.  Over a chunk the nodes are taken in turn: a node that no lane of the wave carries is skipped wave-uniformly
// (ballot), a node that every lane carries runs without selects, one that some carry is computed and each lane keeps its own
// result.  Nothing is shared between channels: no LDS, no atomics, and a channel's bits do not depend on its neighbours.
// A lane rewrites the elements it read, so out may be in.
//
// Slider stores (dspfx_strips_set_gain / _set_band) go through the staged-store queue (store_queue.hip.h): staged in page-locked
// memory, queued, and put on the next run's stream ahead of its kernel; a band store also zeroes the band's state on the stored channels
// (after_settings_change -> regenerate_filter -> reset_state, biquad.rs:62-76).
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

constexpr uint32_t WG = 256;
constexpr uint32_t GAIN_BIT = 1u;                  // node n of a strip is bit n of its mask: the Gain node, then band b at bit 1 + b

struct StripArgs {
    const float *in;             // may be `out`: no __restrict__
    float *out;
    const float *coef;           // [KB][5][N]: a1, a2, b0, b1, b2, normalised
    float *state;                // [KB][4][N]: x1, x2, y1, y2
    const float *level;          // [N]
    const uint32_t *mask;        // [N]
    uint32_t N, W, nf, flags;
    float div;                   // f32(0.0001 + 1.0)
};

// node_steps.hip.h's biquad_step over F frames; SEL: only the channels with mine[j] carry the band (pick: a v_bfi select)
template <int CPL, int F, bool SEL>
__device__ __forceinline__ void band_rows(float (&v)[F][CPL], const float (&k)[5][CPL], float (&st)[4][CPL], const uint32_t (&mine)[CPL]) {
#pragma unroll
    for (int i = 0; i < F; ++i) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const float a1 = k[0][j], a2 = k[1][j], b0 = k[2][j], b1 = k[3][j], b2 = k[4][j];
            const float x = v[i][j];
            const float y = biquad_step(x, a1, a2, b0, b1, b2, st[0][j], st[1][j], st[2][j], st[3][j]);
            if constexpr (SEL) {
                st[1][j] = pick(mine[j], st[0][j], st[1][j]);
                st[0][j] = pick(mine[j], x, st[0][j]);
                st[3][j] = pick(mine[j], st[2][j], st[3][j]);
                st[2][j] = pick(mine[j], y, st[2][j]);
                v[i][j] = pick(mine[j], y, x);
            } else {
                st[1][j] = st[0][j];
                st[0][j] = x;
                st[3][j] = st[2][j];
                st[2][j] = y;
                v[i][j] = y;
            }
        }
    }
}

// node.rs:162-194 with one connected pipe, on the channels whose node n has a hop in front of it
template <int CPL, int F>
__device__ __forceinline__ void hop_rows(float (&v)[F][CPL], const uint32_t (&hop)[CPL], int n, float div) {
#pragma unroll
    for (int i = 0; i < F; ++i)
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const float h = __fdiv_rn(__fadd_rn(0.0f, v[i][j]), div);
            v[i][j] = pick(0u - ((hop[j] >> n) & 1u), h, v[i][j]);
        }
}

// wave-uniform: the nodes some lane carries, the nodes every lane carries, the nodes with a hop in front somewhere
struct Wave {
    uint32_t any, all, hop;
    float div;
};

// F frames of the lane's channels through the strip: the Gain node, then the bands in order
template <int KB, int CPL, int F>
__device__ __forceinline__ void strip_rows(float (&v)[F][CPL], const float (&k)[KB][5][CPL], float (&st)[KB][4][CPL], const uint32_t (&m)[CPL],
                                           const float (&lv)[CPL], const uint32_t (&hop)[CPL], const Wave &w) {
    if (w.any & GAIN_BIT) {                              // gain.rs:33-37
        if (w.hop & GAIN_BIT) hop_rows<CPL, F>(v, hop, 0, w.div);
#pragma unroll
        for (int i = 0; i < F; ++i)
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                const float y = v[i][j] * lv[j];
                v[i][j] = pick(0u - (m[j] & GAIN_BIT), y, v[i][j]);
            }
    }
#pragma unroll
    for (int b = 0; b < KB; ++b) {
        const int n = 1 + b;
        if (!((w.any >> n) & 1u)) continue;
        if ((w.hop >> n) & 1u) hop_rows<CPL, F>(v, hop, n, w.div);
        uint32_t mine[CPL];                              // all ones: the channel carries the band
#pragma unroll
        for (int j = 0; j < CPL; ++j) mine[j] = 0u - ((m[j] >> n) & 1u);
        if ((w.all >> n) & 1u) band_rows<CPL, F, false>(v, k[b], st[b], mine);
        else band_rows<CPL, F, true>(v, k[b], st[b], mine);
    }
}

// frame rows per chunk (two chunks are in registers), and the waves per SIMD the register allocation is held to: beside the
// rows, the coefficients and the state are 9 * KB * CPL registers
constexpr int rows_for(int KB, int CPL) { return CPL == 4 ? 4 : 8; }
constexpr int waves_for(int KB, int CPL) { return KB * CPL <= 4 ? 3 : 2; }

template <int KB, int CPL>
__global__ __launch_bounds__(WG, waves_for(KB, CPL)) void strips_run(StripArgs a) {
    constexpr int F = rows_for(KB, CPL);
    // lane_io's lane_channel, written out: with the helper the register allocation of these kernels comes out otherwise
    const uint64_t c64 = ((uint64_t)blockIdx.x * WG + threadIdx.x) * CPL;
    if (c64 >= a.N) return;                                // (CPL > 1 only with N % 4 == 0: a lane's channels are all inside)
    const uint32_t c = (uint32_t)c64;
    uint32_t m[CPL], hop[CPL];
    float lv[CPL];
    loadv<CPL>(a.mask + c, m);
    loadv<CPL>(a.level + c, lv);
    uint32_t any = 0, all = ~0u, anyhop = 0;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        // the hop in front of node n: LINK_INPUT for the channel's first present node, LINK_INTERNAL for the later ones
        const uint32_t first = m[j] & (0u - m[j]);
        hop[j] = ((a.flags & DSPFX_LINK_INPUT) ? first : 0u) | ((a.flags & DSPFX_LINK_INTERNAL) ? (m[j] & ~first) : 0u);
        any |= m[j];
        all &= m[j];
        anyhop |= hop[j];
    }
    // wave-uniform: the nodes some lane carries, the nodes every lane carries, the nodes with a hop somewhere
    uint32_t w_any = 0, w_all = 0, w_hop = 0;
#pragma unroll
    for (int n = 0; n <= KB; ++n) {
        if (__ballot((any >> n) & 1u)) w_any |= 1u << n;
        if (!__ballot(!((all >> n) & 1u))) w_all |= 1u << n;
        if (__ballot((anyhop >> n) & 1u)) w_hop |= 1u << n;
    }
    float k[KB][5][CPL], st[KB][4][CPL];
#pragma unroll
    for (int b = 0; b < KB; ++b) {
#pragma unroll
        for (int r = 0; r < 5; ++r)
#pragma unroll
            for (int j = 0; j < CPL; ++j) k[b][r][j] = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < CPL; ++j) st[b][r][j] = 0.0f;
        if (!((w_any >> (1 + b)) & 1u)) continue;
#pragma unroll
        for (int r = 0; r < 5; ++r) loadv<CPL>(a.coef + ((size_t)b * 5 + r) * a.N + c, k[b][r]);
#pragma unroll
        for (int r = 0; r < 4; ++r) loadv<CPL>(a.state + ((size_t)b * 4 + r) * a.N + c, st[b][r]);
    }
    const size_t lane0 = lay(0, c, a.nf, a.N, a.W), rs = a.W ? a.W : a.N;
    const float *lin = a.in + lane0;
    float *lout = a.out + lane0;
    const Wave w{w_any, w_all, w_hop, a.div};
    // lane_io's each_chunk, written out: with the helper strips_run<2, 4> takes 202 registers for 198 and measured slower than the
    // spread of five parent runs at 65 536 channels (0.0380 ms for 0.0376)
    const uint32_t nfull = a.nf / F;
    float cur[F][CPL], nxt[F][CPL];
    if (nfull) load_rows<CPL, F>(lin, rs, 0, cur);
#pragma unroll 1
    for (uint32_t ch = 0; ch < nfull; ++ch) {
        if (ch + 1 < nfull) load_rows<CPL, F>(lin, rs, (ch + 1) * F, nxt);
        strip_rows<KB, CPL, F>(cur, k, st, m, lv, hop, w);
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
        strip_rows<KB, CPL, 1>(one, k, st, m, lv, hop, w);
        store_rows<CPL, 1>(lout, rs, f, one);
    }
    // (a channel that does not carry the band kept the values it loaded)
#pragma unroll
    for (int b = 0; b < KB; ++b) {
        if (!((w_any >> (1 + b)) & 1u)) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) storev<CPL, false>(a.state + ((size_t)b * 4 + r) * a.N + c, st[b][r]);
    }
}

// a store's bookkeeping on the device, in stream order: the node bit of channels [first, first + count), and -- a band store --
// the band's four state rows zeroed on exactly those channels
__global__ __launch_bounds__(WG) void strips_store(uint32_t *__restrict__ mask, float *__restrict__ band_state, uint32_t N, uint32_t first,
                                                   uint32_t count, uint32_t set, uint32_t clr) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= count) return;
    const uint32_t c = first + i;
    mask[c] = (mask[c] & ~clr) | set;
    if (band_state) {
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) band_state[(size_t)r * N + c] = 0.0f;
    }
}

thread_local std::string g_err;        // the reason of the last failed create on this thread

// a store's vals: [count] levels or [5][count] coefficients; none: the node is dropped
struct StoreFields {
    int node = 0;                // 0: the Gain node; 1 + b: band b
    uint32_t first = 0, count = 0;
};
typedef StoreQueue<StoreFields> Stores;
typedef Stores::Store Store;

uint32_t bands_built(uint32_t K) { return K <= 1 ? 1u : K <= 2 ? 2u : K <= 4 ? 4u : 8u; }

}  // namespace

struct dspfx_strips : ChannelBank<dspfx_strips_desc, StoreFields> {        // stores.qmu guards hmask too
    static constexpr const char *name = "strips";
    uint32_t KB = 1;                             // the kernel's band count: 1, 2, 4 or 8
    std::vector<uint32_t> hmask;                 // the node masks with every store made so far (stores.qmu): what the next run sees
    float *coef = nullptr, *state = nullptr, *level = nullptr;
    uint32_t *mask = nullptr;
    float div = 1.0f;
    // the fresh state: no node anywhere, every state at rest, every level 1.0
    template <class V>
    static void tables(const dspfx_strips_desc &d, V v) {
        const uint64_t N = d.n_channels, KB = bands_built(d.bands);
        v(KB * 5 * N * 4, 0, &dspfx_strips::coef);
        v(KB * 4 * N * 4, 0, &dspfx_strips::state);
        v(4 * N, 0x3F800000, &dspfx_strips::level);
        v(4 * N, 0, &dspfx_strips::mask);
    }
};

namespace {

// one store onto the stream: its values, then the node bit (and a band's zeroed state) on its channels
hipError_t apply_store(dspfx_strips *p, const Store &st, hipStream_t s) {
    const uint32_t N = p->desc.n_channels;
    const uint32_t bit = 1u << st.node, blocks = (st.count + WG - 1) / WG;
    if (!st.vals) {
        strips_store<<<blocks, WG, 0, s>>>(p->mask, nullptr, N, st.first, st.count, 0u, bit);
        return hipGetLastError();
    }
    hipError_t err = hipSuccess;
    float *band_state = nullptr;
    if (st.node == 0) {
        err = hipMemcpyAsync(p->level + st.first, st.vals, (size_t)st.count * sizeof(float), hipMemcpyHostToDevice, s);
    } else {
        const uint32_t b = (uint32_t)st.node - 1;
        band_state = p->state + (size_t)b * 4 * N;
        for (uint32_t r = 0; r < 5 && err == hipSuccess; ++r)
            err = hipMemcpyAsync(p->coef + ((size_t)b * 5 + r) * N + st.first, st.vals + (size_t)r * st.count,
                                 (size_t)st.count * sizeof(float), hipMemcpyHostToDevice, s);
    }
    if (err != hipSuccess) return err;
    strips_store<<<blocks, WG, 0, s>>>(p->mask, band_state, N, st.first, st.count, bit, 0u);
    return hipGetLastError();
}

// the store joins the queue and the masks the next run will see
void enqueue(dspfx_strips *p, const Store &st) {
    p->stores.push(st, [&] {
        const uint32_t bit = 1u << st.node;
        for (uint32_t i = 0; i < st.count; ++i) {
            uint32_t &m = p->hmask[st.first + i];
            m = st.vals ? (m | bit) : (m & ~bit);
        }
    });
}

// the lane width per band count: four channels while their coefficients and state fit in registers beside the rows, then two, then one
template <int KB, int CPL>
hipError_t launch(const StripArgs &a, hipStream_t s) {
    strips_run<KB, CPL><<<lane_blocks(a.N, CPL, WG), WG, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch(uint32_t KB, bool vec, const StripArgs &a, hipStream_t s) {
    switch (KB) {
    case 1: return vec ? launch<1, 4>(a, s) : launch<1, 1>(a, s);
    case 2: return vec ? launch<2, 4>(a, s) : launch<2, 1>(a, s);
    case 4: return vec ? launch<4, 2>(a, s) : launch<4, 1>(a, s);
    default: return launch<8, 1>(a, s);
    }
}

}  // namespace

extern "C" const char *dspfx_strips_last_error(const dspfx_strips *p) { return p ? p->err.c_str() : g_err.c_str(); }

extern "C" int dspfx_strips_coeffs(const float *raw6, float *out5) {
    if (!raw6 || !out5) return DSPFX_ERR_INVALID;
    const float a0 = raw6[0];                    // biquad.rs:66-70: five f32 divisions, a0 = 0 included
    for (int i = 0; i < 5; ++i) out5[i] = raw6[1 + i] / a0;
    return DSPFX_OK;
}

extern "C" int dspfx_strips_create(const dspfx_strips_desc *desc, dspfx_strips **out) {
    const int rc = create_checks(desc, out, g_err, [desc](std::string &err) -> int {
        char buf[160];
        if (desc->bands < 1 || desc->bands > DSPFX_STRIPS_MAX_BANDS) {
            std::snprintf(buf, sizeof buf, "strips: %u bands, not 1 .. %d", desc->bands, DSPFX_STRIPS_MAX_BANDS);
            err = buf;
            return DSPFX_ERR_INVALID;
        }
        if (desc->link_flags & ~(DSPFX_LINK_INTERNAL | DSPFX_LINK_INPUT)) {
            std::snprintf(buf, sizeof buf, "strips: unknown link flag in 0x%x (DSPFX_LINK_INTERNAL and DSPFX_LINK_INPUT are known)", desc->link_flags);
            err = buf;
            return DSPFX_ERR_INVALID;
        }
        return DSPFX_OK;
    });
    if (rc != DSPFX_OK) return rc;
    return create_bank(
        desc, out, g_err,
        [](dspfx_strips *p) {
            p->KB = bands_built(p->desc.bands);
            p->div = dspfx_link_divisor(1);
            p->hmask.assign(p->desc.n_channels, 0u);
        },
        nullptr, "strips: no device memory for the coefficients, the state, the levels and the masks");
}

extern "C" int dspfx_strips_destroy(dspfx_strips *p) { return destroy_bank(p); }

extern "C" int dspfx_strips_set_gain(dspfx_strips *p, const float *host_levels, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_range(p, "set_gain", first_channel, count);
    if (rc != DSPFX_OK) return rc;
    if (count == 0) return DSPFX_OK;
    Store st;
    st.node = 0;
    if (!stage_store(p, st, nullptr, "set_gain", first_channel, count, host_levels ? count : 0, "staged levels")) return DSPFX_ERR_OOM;
    if (host_levels) std::memcpy(st.vals, host_levels, count * sizeof(float));
    enqueue(p, st);
    return DSPFX_OK;
}

extern "C" int dspfx_strips_set_band(dspfx_strips *p, uint32_t band, const float *host_raw6, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    if (band >= p->desc.bands) {
        char buf[96];
        std::snprintf(buf, sizeof buf, "strips set_band: band %u, and the bank has %u", band, p->desc.bands);
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    const int rc = check_range(p, "set_band", first_channel, count);
    if (rc != DSPFX_OK) return rc;
    if (count == 0) return DSPFX_OK;
    Store st;
    st.node = 1 + (int)band;
    if (!stage_store(p, st, nullptr, "set_band", first_channel, count, host_raw6 ? 5 * count : 0, "staged coefficients")) return DSPFX_ERR_OOM;
    if (host_raw6) {
        for (uint64_t i = 0; i < count; ++i) {           // regenerate_filter per channel, transposed to [5][count]
            float k5[5];
            (void)dspfx_strips_coeffs(host_raw6 + 6 * i, k5);
            for (int r = 0; r < 5; ++r) st.vals[(size_t)r * count + i] = k5[r];
        }
    }
    enqueue(p, st);
    return DSPFX_OK;
}

extern "C" int dspfx_strips_present(dspfx_strips *p, uint32_t *host_masks_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "present", host_masks_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = p->hmask[c]; });
}

extern "C" int dspfx_strips_run(dspfx_strips *p, const float *in, float *out, uint32_t n_frames, void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    hipStream_t s = (hipStream_t)stream;
    const int rc = begin_run(p, in && out, n_frames, s, "strips run: in, out or n_frames", "slider store", apply_store);
    if (rc != DSPFX_OK) return rc;
    StripArgs a;
    a.in = in;
    a.out = out;
    a.coef = p->coef;
    a.state = p->state;
    a.level = p->level;
    a.mask = p->mask;
    a.N = p->desc.n_channels;
    a.W = p->desc.tile_channels;
    a.nf = n_frames;
    a.flags = p->desc.link_flags;
    a.div = p->div;
    BANK_HIP_WHY(launch(p->KB, lane_plan(a.N, a.W, (uintptr_t)in | (uintptr_t)out, WG).vec, a, s), "strips_run");
    return DSPFX_OK;
}

extern "C" int dspfx_strips_reset(dspfx_strips *p) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    if (!p->used) return DSPFX_OK;               // no run yet: the state is as create left it, and a queued band store only zeroes
    BANK_HIP_WHY(hipSetDevice(p->desc.device), "hipSetDevice");
    BANK_HIP_WHY(hipMemsetAsync(p->state, 0, (size_t)p->KB * 4 * p->desc.n_channels * sizeof(float), p->last), "strips reset");
    return DSPFX_OK;
}
