// dynamics_kernels.hip -- the channel-dynamics bank (include/dspfx.h, dspfx_dynamics_*): every channel may carry its own Envelope
// node (nodes/envelope.rs, a peak follower with its own attack and release sliders) feeding its own gain computer: the envelope
// turns the gain DOWN above a threshold, and a makeup gain follows.  One bank object is a leveller ahead of the talker bank or a
// limiter behind the room mixes; the detector may follow another block than the one it turns down (the key).
//
// One run is one kernel behind the queued stores, in the shape of talkers_run (talkers_kernels.hip): time is a serial recurrence
// per channel, so a lane owns its channels for the whole block -- four adjacent channels with one 16-byte load and one nontemporal
// 16-byte store per frame when the layout allows it (lane_io.hip.h), one channel otherwise.  Frames are taken in chunks of F rows and the next chunk's loads are issued ahead of this one's arithmetic,
// so the chain env -> env does not wait for memory; a keyed run holds two such streams and takes chunks half as long, the same
// registers.  Per frame: the envelope as K_ENVELOPE computes it (chain_kernels.hip.h), q = env > thr ? thr / env : 1 with one IEEE
// division, the sample times mk * q, the block's largest envelope into `level` and its smallest q into `reduction`.  The tables are
// read once and env, level and reduction written once.  A lane rewrites the elements it read, so out may be in.  A channel without
// a node keeps its sample's bits and its tables at rest.  Nothing is shared between channels: no LDS, no atomics.
//
// Stores (sliders, drops, resets) go through the staged-store queue (store_queue.hip.h).
#include <hip/hip_runtime.h>

#include <cmath>
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

struct DynArgs {
    const float *in;             // may be `out`: no __restrict__
    const float *key;            // the keyed form only; may be neither `in` (the host takes that for no key) nor overlap `out`
    float *out;
    float *env, *level, *red;    // [N] each
    const float *ga, *gr, *thr, *mk;             // [N] each
    const uint8_t *pres;         // [N]: 1 where the channel carries a node
    uint32_t N, W, nf;
};

// the lane's state over a block
template <int CPL>
struct Chan {
    float env[CPL], ga[CPL], gr[CPL], thr[CPL], mk[CPL], lvl[CPL], red[CPL];
    bool on[CPL];
};

// R rows: node_steps.hip.h's envelope_step per detector sample k, then the gain computer on the sample x.
// v holds x and takes the output; k is v itself when there is no key
template <int CPL, int R>
__device__ __forceinline__ void dyn_rows(float (&v)[R][CPL], const float (&k)[R][CPL], Chan<CPL> &s) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const float x = v[i][j];
            const float e = envelope_step(k[i][j], s.env[j], s.ga[j], s.gr[j]);
            const float q = e > s.thr[j] ? s.thr[j] / e : 1.0f;      // (a NaN envelope compares false)
            const float y = __fmul_rn(x, __fmul_rn(s.mk[j], q));
            if (s.on[j]) {
                s.env[j] = e;
                if (e > s.lvl[j]) s.lvl[j] = e;      // a NaN or a -0.0 never raises it
                if (q < s.red[j]) s.red[j] = q;
                v[i][j] = y;                         // no node: the sample's own bits
            }
        }
    }
}

template <int CPL, bool KEYED>
__global__ __launch_bounds__(WG) void dynamics_run(DynArgs a) {
    constexpr int F = KEYED ? 4 : 8;                       // frame rows per chunk (two chunks of every stream are in registers)
    uint32_t c;
    if (!lane_channel<CPL>(WG, a.N, c)) return;
    Chan<CPL> s;
    uint8_t pres[CPL];
    loadv<CPL>(a.env + c, s.env);
    loadv<CPL>(a.ga + c, s.ga);
    loadv<CPL>(a.gr + c, s.gr);
    loadv<CPL>(a.thr + c, s.thr);
    loadv<CPL>(a.mk + c, s.mk);
    loadv<CPL>(a.pres + c, pres);
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        s.lvl[j] = 0.0f;
        s.red[j] = 1.0f;
        s.on[j] = pres[j] != 0;
    }
    const size_t lane0 = lay(0, c, a.nf, a.N, a.W), rs = a.W ? a.W : a.N;
    const float *lin = a.in + lane0, *lkey = KEYED ? a.key + lane0 : nullptr;
    float *lout = a.out + lane0;
    // lane_io's each_chunk with a second prefetched stream, the key, which the helper does not carry
    const uint32_t nfull = a.nf / F;
    float cur[F][CPL], nxt[F][CPL], kcur[KEYED ? F : 1][CPL], knxt[KEYED ? F : 1][CPL];
    if (nfull) {
        load_rows<CPL, F>(lin, rs, 0, cur);
        if constexpr (KEYED) load_rows<CPL, F>(lkey, rs, 0, kcur);
    }
#pragma unroll 1
    for (uint32_t ch = 0; ch < nfull; ++ch) {
        if (ch + 1 < nfull) {
            load_rows<CPL, F>(lin, rs, (ch + 1) * F, nxt);
            if constexpr (KEYED) load_rows<CPL, F>(lkey, rs, (ch + 1) * F, knxt);
        }
        if constexpr (KEYED) dyn_rows<CPL, F>(cur, kcur, s);
        else dyn_rows<CPL, F>(cur, cur, s);
        store_rows<CPL, F>(lout, rs, ch * F, cur);
#pragma unroll
        for (int i = 0; i < F; ++i)
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                cur[i][j] = nxt[i][j];
                if constexpr (KEYED) kcur[i][j] = knxt[i][j];
            }
    }
#pragma unroll 1
    for (uint32_t f = nfull * F; f < a.nf; ++f) {
        float one[1][CPL], kone[1][CPL];
        load_rows<CPL, 1>(lin, rs, f, one);
        if constexpr (KEYED) {
            load_rows<CPL, 1>(lkey, rs, f, kone);
            dyn_rows<CPL, 1>(one, kone, s);
        } else {
            dyn_rows<CPL, 1>(one, one, s);
        }
        store_rows<CPL, 1>(lout, rs, f, one);
    }
    storev<CPL, false>(a.env + c, s.env);                  // (without a node: what was read, +0.0)
    storev<CPL, false>(a.level + c, s.lvl);
    storev<CPL, false>(a.red + c, s.red);
}

// a reset's and a drop's device side, in stream order, on channels [first, first + count): the state at rest
__global__ __launch_bounds__(WG) void dynamics_fresh(float *__restrict__ env, float *__restrict__ level, float *__restrict__ red, uint32_t first,
                                                     uint32_t count) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= count) return;
    const uint32_t c = first + i;
    env[c] = 0.0f;
    level[c] = 0.0f;
    red[c] = 1.0f;
}

thread_local std::string g_err;        // the reason of the last failed create or plan on this thread

enum StoreKind : uint32_t { ST_SLIDERS, ST_DROP, ST_RESET };

// a store's vals: SLIDERS four runs of [count]: attack gains, release gains, thresholds, makeups; DROP and RESET carry none
struct StoreFields {
    StoreKind kind = ST_RESET;
    uint32_t first = 0, count = 0;
};
typedef StoreQueue<StoreFields> Stores;
typedef Stores::Store Store;

}  // namespace

struct dspfx_dynamics : ChannelBank<dspfx_dynamics_desc, StoreFields> {
    static constexpr const char *name = "dynamics";
    std::vector<float> hga, hgr, hthr, hmk;      // [N]: the sliders with every store made so far (a NULL slider keeps them)
    std::vector<uint8_t> hpres;                  // [N]
    float *env = nullptr, *level = nullptr, *red = nullptr, *ga = nullptr, *gr = nullptr, *thr = nullptr, *mk = nullptr;
    uint8_t *pres = nullptr;
    // the fresh state: no node anywhere.  The state at rest is not one byte over (the reduction is 1.0): create runs dynamics_fresh
    template <class V>
    static void tables(const dspfx_dynamics_desc &d, V v) {
        const uint64_t N = d.n_channels;
        for (auto m : {&dspfx_dynamics::env, &dspfx_dynamics::level, &dspfx_dynamics::red}) v(4 * N, TABLE_BY_HAND, m);
        for (auto m : {&dspfx_dynamics::ga, &dspfx_dynamics::gr, &dspfx_dynamics::thr, &dspfx_dynamics::mk}) v(4 * N, 0, m);
        v(N, 0, &dspfx_dynamics::pres);
    }
};

namespace {

// one store onto the stream
hipError_t apply_store(dspfx_dynamics *p, const Store &st, hipStream_t s) {
    const size_t n = st.count, bytes = n * sizeof(float);
    hipError_t err = hipSuccess;
    switch (st.kind) {
    case ST_SLIDERS: {
        float *const tabs[4] = {p->ga, p->gr, p->thr, p->mk};
        for (int t = 0; t < 4 && err == hipSuccess; ++t) err = hipMemcpyAsync(tabs[t] + st.first, st.vals + t * n, bytes, hipMemcpyHostToDevice, s);
        if (err == hipSuccess) err = hipMemsetAsync(p->pres + st.first, 1, n, s);
        return err;
    }
    case ST_DROP:
        err = hipMemsetAsync(p->pres + st.first, 0, n, s);
        if (err != hipSuccess) return err;
        [[fallthrough]];
    case ST_RESET:
        dynamics_fresh<<<(st.count + WG - 1) / WG, WG, 0, s>>>(p->env, p->level, p->red, st.first, st.count);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace

extern "C" const char *dspfx_dynamics_last_error(const dspfx_dynamics *p) { return p ? p->err.c_str() : g_err.c_str(); }

extern "C" float dspfx_dynamics_gain(float env, float threshold, float makeup, float *q_out) {
    const float q = env > threshold ? threshold / env : 1.0f;
    if (q_out) *q_out = q;
    return makeup * q;
}

extern "C" int dspfx_dynamics_plan(uint64_t channels, uint64_t *bytes_out) { return plan_bank<dspfx_dynamics>(channels, bytes_out, g_err); }

extern "C" int dspfx_dynamics_create(const dspfx_dynamics_desc *desc, dspfx_dynamics **out) {
    const int rc = create_checks(desc, out, g_err);
    if (rc != DSPFX_OK) return rc;
    const uint32_t N = desc->n_channels;
    return create_bank(
        desc, out, g_err,
        [N](dspfx_dynamics *p) {
            p->hga.assign(N, 0.0f);
            p->hgr.assign(N, 0.0f);
            p->hthr.assign(N, 1.0f);
            p->hmk.assign(N, 1.0f);
            p->hpres.assign(N, 0);
        },
        [N](dspfx_dynamics *p) {
            dynamics_fresh<<<(N + WG - 1) / WG, WG>>>(p->env, p->level, p->red, 0u, N);
            return hipGetLastError();
        },
        nullptr);
}

extern "C" int dspfx_dynamics_destroy(dspfx_dynamics *p) { return destroy_bank(p); }

extern "C" int dspfx_dynamics_set(dspfx_dynamics *p, const float *host_threshold, const float *host_makeup, const float *host_attack,
                                  const float *host_release, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_range(p, "set", first_channel, count);
    if (rc != DSPFX_OK) return rc;
    char buf[192];
    for (uint64_t i = 0; i < count; ++i) {
        // (a NaN fails every comparison; -0.0 is below +0.0 here: it would turn the sign of every sample it meets)
        if (host_threshold && (!(host_threshold[i] >= 0.0f) || std::signbit(host_threshold[i]))) {
            std::snprintf(buf, sizeof buf, "dynamics set: channel %llu is given threshold %g (NaN or below +0.0)", (unsigned long long)(first_channel + i),
                          (double)host_threshold[i]);
            return p->fail(DSPFX_ERR_INVALID, buf);
        }
        if (host_makeup && (!(host_makeup[i] >= 0.0f) || std::signbit(host_makeup[i]) || std::isinf(host_makeup[i]))) {
            std::snprintf(buf, sizeof buf, "dynamics set: channel %llu is given makeup %g (NaN, infinite or negative)", (unsigned long long)(first_channel + i),
                          (double)host_makeup[i]);
            return p->fail(DSPFX_ERR_INVALID, buf);
        }
    }
    if (count == 0) return DSPFX_OK;
    Store st;
    std::unique_lock<std::mutex> one;
    if (!stage_store(p, st, &one, ST_SLIDERS, "set", first_channel, count, 4 * count, "staged sliders")) return DSPFX_ERR_OOM;
    float *a = st.vals, *r = a + count, *t = r + count, *m = t + count;
    for (uint64_t i = 0; i < count; ++i) {
        a[i] = host_attack ? dspfx_envelope_gain(host_attack[i]) : p->hga[first_channel + i];
        r[i] = host_release ? dspfx_envelope_gain(host_release[i]) : p->hgr[first_channel + i];
        t[i] = host_threshold ? host_threshold[i] : p->hthr[first_channel + i];
        m[i] = host_makeup ? host_makeup[i] : p->hmk[first_channel + i];
    }
    p->stores.push(st, [&] {
        std::memcpy(p->hga.data() + first_channel, a, count * sizeof(float));
        std::memcpy(p->hgr.data() + first_channel, r, count * sizeof(float));
        std::memcpy(p->hthr.data() + first_channel, t, count * sizeof(float));
        std::memcpy(p->hmk.data() + first_channel, m, count * sizeof(float));
        std::memset(p->hpres.data() + first_channel, 1, count);
    });
    return DSPFX_OK;
}

extern "C" int dspfx_dynamics_drop(dspfx_dynamics *p, uint64_t first_channel, uint64_t count) {
    return store_plain(p, ST_DROP, "drop", first_channel, count, [=] {
        for (uint64_t c = first_channel; c < first_channel + count; ++c) {     // a later store meets the defaults again
            p->hga[c] = p->hgr[c] = 0.0f;
            p->hthr[c] = p->hmk[c] = 1.0f;
            p->hpres[c] = 0;
        }
    });
}

extern "C" int dspfx_dynamics_reset(dspfx_dynamics *p, uint64_t first_channel, uint64_t count) {
    return store_plain(p, ST_RESET, "reset", first_channel, count);
}

extern "C" int dspfx_dynamics_present(dspfx_dynamics *p, uint32_t *host_present_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "present", host_present_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = p->hpres[c]; });
}

extern "C" int dspfx_dynamics_views(dspfx_dynamics *p, const float **level_out, const float **reduction_out) {
    if (!p) return DSPFX_ERR_INVALID;
    if (level_out) *level_out = p->level;
    if (reduction_out) *reduction_out = p->red;
    return DSPFX_OK;
}

extern "C" int dspfx_dynamics_run(dspfx_dynamics *p, const float *in, const float *key, float *out, uint32_t n_frames, void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    hipStream_t s = (hipStream_t)stream;
    const int rc = begin_run(p, in && out, n_frames, s, "dynamics run: in, out or n_frames", "dynamics store", apply_store);
    if (rc != DSPFX_OK) return rc;
    if (key == in) key = nullptr;                // the detector follows the block itself: one stream of loads
    DynArgs a;
    a.in = in;
    a.key = key;
    a.out = out;
    a.env = p->env;
    a.level = p->level;
    a.red = p->red;
    a.ga = p->ga;
    a.gr = p->gr;
    a.thr = p->thr;
    a.mk = p->mk;
    a.pres = p->pres;
    a.N = p->desc.n_channels;
    a.W = p->desc.tile_channels;
    a.nf = n_frames;
    const auto [vec, lanes, blocks] = lane_plan(a.N, a.W, (uintptr_t)in | (uintptr_t)out | (uintptr_t)key, WG);
    if (vec && key) dynamics_run<4, true><<<blocks, WG, 0, s>>>(a);
    else if (vec) dynamics_run<4, false><<<blocks, WG, 0, s>>>(a);
    else if (key) dynamics_run<1, true><<<blocks, WG, 0, s>>>(a);
    else dynamics_run<1, false><<<blocks, WG, 0, s>>>(a);
    BANK_HIP_WHY(hipGetLastError(), "dynamics_run");
    return DSPFX_OK;
}
