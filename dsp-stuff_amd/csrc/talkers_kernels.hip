// talkers_kernels.hip -- the talker bank (include/dspfx.h, dspfx_talkers_*): every channel carries its own Envelope node
// (nodes/envelope.rs, a peak follower with its own attack and release sliders), every room gets its `top` loudest members chosen
// on the device, and a gate passes those members and ramps the others out, so the room mixes downstream add only the talkers.
//
// One run is two kernels behind the queued stores.
//   pass A (talkers_run)   per channel, frames in order.  Time is a serial recurrence per channel, so a lane owns its channels
//            for the whole block, as in strips_kernels.hip: four adjacent channels with one 16-byte load and one nontemporal
//            16-byte store per frame when the layout allows it (lane_io.hip.h), one channel otherwise.  Frames are taken in
//            chunks of F rows and the next chunk's loads are issued ahead of this one's arithmetic, so the chain env -> env does
//            not wait for memory.  Per frame: the envelope as K_ENVELOPE computes it (chain_kernels.hip.h), the block's largest
//            envelope into `level`, and -- the gated form -- the sample times gate + (target - gate) * r[f], r[f] = (f + 1) / nf.
//            The metering form (out == NULL) writes no sample and leaves `gate`.  Either form leaves target[c] at what a channel
//            that is nobody's talker gets: 1.0 under an OPEN pin, +0.0 otherwise; pass B raises the talkers'.  A lane rewrites the
//            elements it read, so out may be in.  Nothing is shared between channels: no LDS, no atomics.
//   pass B (talkers_pick)  one wave per room.  A lane gathers up to 16 members' levels through the member list (sorted by room,
//            then channel, so the kernel does not care how scattered a room is) and builds a u64 key per candidate: the level's
//            bits << 32 | ~channel.  Levels are non-negative and never NaN, so unsigned order is level descending, then channel
//            ascending; 0 is "no candidate" (a channel number is below 2^32 - 256, so no real key is 0).  `top` rounds: the
//            lane's own maximum, a 64-lane __shfl_xor maximum, the winner retired.  Lane 0 writes the room's row of the tables
//            and the winner's target.  No atomics, no LDS, every step in a fixed order.
// A bank that has handed out its audible list (dspfx_talkers_audible_views) launches a third kernel, talkers_audible, ahead of pass A
// of every gated run: per room the members that can be non-zero in the block about to be gated, for dspfx_mixmatrix_run_sparse.
//
// Stores (sliders, pins, tops, the floor, seatings, resets) go through the staged-store queue (store_queue.hip.h).  A seating is
// the member list and room_start[G + 1], built on the host from room_of[N] alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/dspfx.h"
#include "channel_bank.hip.h"
#include "lane_io.hip.h"
#include "node_steps.hip.h"

namespace {

constexpr uint32_t WG = 256;
constexpr uint32_t NONE = DSPFX_TALKERS_NO_ROOM;
constexpr uint32_t MAX_ROOM = DSPFX_TALKERS_MAX_ROOM;
constexpr uint32_t MAX_TOP = DSPFX_TALKERS_MAX_TOP;
constexpr uint32_t PER_LANE = MAX_ROOM / 64;       // pass B: members per lane
constexpr int F = 8;                               // pass A: frame rows per chunk (two chunks are in registers)

struct TalkArgs {
    const float *in;             // may be `out`: no __restrict__
    float *out;                  // the gated form only
    float *env, *gate, *target, *level;          // [N] each
    const float *ga, *gr;        // [N]: the attack and release gains
    const uint8_t *pin;          // [N]
    uint32_t N, W, nf;
};

// the lane's state over a block
template <int CPL>
struct Chan {
    float env[CPL], ga[CPL], gr[CPL], lvl[CPL];
    float g0[CPL], dg[CPL];      // the gated form: the gate, and target - gate
};

// R rows from frame f0: node_steps.hip.h's envelope_step per sample, the block's largest envelope, the gate
template <bool GATED, int CPL, int R>
__device__ __forceinline__ void talk_rows(float (&v)[R][CPL], Chan<CPL> &s, uint32_t f0, float fn) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
        float r = 0.0f;
        if (GATED) r = __fdiv_rn((float)(f0 + i + 1), fn);
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const float x = v[i][j];
            const float e = envelope_step(x, s.env[j], s.ga[j], s.gr[j]);
            s.env[j] = e;
            if (e > s.lvl[j]) s.lvl[j] = e;      // a NaN or a -0.0 never raises it
            if (GATED) v[i][j] = __fmul_rn(x, __fadd_rn(s.g0[j], __fmul_rn(s.dg[j], r)));
        }
    }
}

template <int CPL, bool GATED>
__global__ __launch_bounds__(WG) void talkers_run(TalkArgs a) {
    uint32_t c;
    if (!lane_channel<CPL>(WG, a.N, c)) return;
    Chan<CPL> s;
    uint8_t pin[CPL];
    float tgt[CPL];
    loadv<CPL>(a.env + c, s.env);
    loadv<CPL>(a.ga + c, s.ga);
    loadv<CPL>(a.gr + c, s.gr);
    loadv<CPL>(a.pin + c, pin);
#pragma unroll
    for (int j = 0; j < CPL; ++j) s.lvl[j] = s.g0[j] = s.dg[j] = tgt[j] = 0.0f;
    if (GATED) {
        loadv<CPL>(a.gate + c, s.g0);
        loadv<CPL>(a.target + c, tgt);
#pragma unroll
        for (int j = 0; j < CPL; ++j) s.dg[j] = __fsub_rn(tgt[j], s.g0[j]);
    }
    const size_t lane0 = lay(0, c, a.nf, a.N, a.W), rs = a.W ? a.W : a.N;
    const float *lin = a.in + lane0;
    float *lout = GATED ? a.out + lane0 : nullptr;
    const float fn = (float)a.nf;
    each_chunk<CPL, F, GATED>(lin, lout, rs, a.nf, [&](auto &v, uint32_t f0) LANE_BODY { talk_rows<GATED>(v, s, f0, fn); });
    storev<CPL, false>(a.env + c, s.env);
    storev<CPL, false>(a.level + c, s.lvl);
    if (GATED) storev<CPL, false>(a.gate + c, tgt);        // after the block, gate = target
    float open[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) open[j] = pin[j] == DSPFX_TALKERS_OPEN ? 1.0f : 0.0f;
    storev<CPL, false>(a.target + c, open);                // pass B raises the talkers'
}

// pass B: wave w of the grid takes room w
__global__ __launch_bounds__(WG) void talkers_pick(const float *__restrict__ level, const uint8_t *__restrict__ pin, const uint32_t *__restrict__ members,
                                                   const uint32_t *__restrict__ room_start, const uint8_t *__restrict__ top, float floor,
                                                   float *__restrict__ target, int32_t *__restrict__ talkers, float *__restrict__ tlev, uint32_t G,
                                                   uint32_t N) {
    const uint64_t r64 = (uint64_t)blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
    if (r64 >= G) return;                                  // (wave-uniform)
    const uint32_t r = (uint32_t)r64, lane = threadIdx.x & 63u;
    const uint32_t s0 = room_start[r], n = min(room_start[r + 1] - s0, MAX_ROOM);
    // selects, not branches: the 16 gathers of a lane are independent loads in flight together.  A slot past the room's end reads
    // a valid entry of the list (every entry, listed or stale, is a channel number below N) and gives no key
    unsigned long long key[PER_LANE];
#pragma unroll
    for (uint32_t k = 0; k < PER_LANE; ++k) {
        const uint32_t i = lane + 64 * k;
        const uint32_t c = min(members[min((size_t)s0 + i, (size_t)N - 1)], N - 1u);
        const float lv = level[c];
        const bool cand = i < n && pin[c] == DSPFX_TALKERS_AUTO && lv > floor;
        key[k] = cand ? ((unsigned long long)__float_as_uint(lv) << 32) | (uint32_t)~c : 0ull;
    }
    const uint32_t tp = top[r];
#pragma unroll 1
    for (uint32_t t = 0; t < MAX_TOP; ++t) {
        unsigned long long w = 0ull;
#pragma unroll
        for (uint32_t k = 0; k < PER_LANE; ++k) w = key[k] > w ? key[k] : w;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long o = __shfl_xor(w, m);
            w = o > w ? o : w;
        }
        if (t >= tp) w = 0ull;                             // (the rounds past the room's top: nobody)
        const uint32_t c = ~(uint32_t)w;
        if (lane == 0) {
            talkers[(size_t)r * MAX_TOP + t] = w ? (int32_t)c : -1;
            tlev[(size_t)r * MAX_TOP + t] = w ? __uint_as_float((uint32_t)(w >> 32)) : 0.0f;
            if (w) target[c] = 1.0f;
        }
#pragma unroll
        for (uint32_t k = 0; k < PER_LANE; ++k) key[k] = key[k] == w ? 0ull : key[k];       // (keys are unique: they carry the channel)
    }
}

// the audible list (dspfx_talkers_audible_views): wave w of the grid takes room w, ahead of pass A, which overwrites `gate`.  A member
// is audible iff its gate or its target is not +-0.0: only then can gate + (target - gate) * r[f] be non-zero in the block about to be
// gated.  Member slots are lane + 64 k as in talkers_pick; round k's audible members go behind those of the rounds before, in lane
// order (a ballot and a count of the lanes below), so a room's segment list[room_start[r] ..] comes out in member order, which is
// ascending channel order.  A room writes inside its own segment only.  No atomics, no LDS
__global__ __launch_bounds__(WG) void talkers_audible(const float *__restrict__ gate, const float *__restrict__ target, const uint32_t *__restrict__ members,
                                                      const uint32_t *__restrict__ room_start, int32_t *__restrict__ list, uint32_t *__restrict__ count,
                                                      uint32_t G, uint32_t N) {
    const uint64_t r64 = (uint64_t)blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
    if (r64 >= G) return;                                  // (wave-uniform)
    const uint32_t r = (uint32_t)r64, lane = threadIdx.x & 63u;
    const uint32_t s0 = room_start[r], n = min(room_start[r + 1] - s0, MAX_ROOM);
    // selects, not branches, as in talkers_pick: a slot past the room's end reads a valid entry of the list and is nobody
    uint32_t ch[PER_LANE];
    bool aud[PER_LANE];
#pragma unroll
    for (uint32_t k = 0; k < PER_LANE; ++k) {
        const uint32_t i = lane + 64 * k;
        const uint32_t c = min(members[min((size_t)s0 + i, (size_t)N - 1)], N - 1u);
        ch[k] = c;
        aud[k] = i < n && (gate[c] != 0.0f || target[c] != 0.0f);
    }
    uint32_t at = 0;                                       // the audible members of the rounds before (wave-uniform)
#pragma unroll
    for (uint32_t k = 0; k < PER_LANE; ++k) {
        const unsigned long long b = __ballot(aud[k]);
        if (aud[k]) list[(size_t)s0 + at + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = (int32_t)ch[k];     // (at + below < n)
        at += (uint32_t)__popcll(b);
    }
    if (lane == 0) count[r] = at;
}

// a reset's device side, in stream order, on channels [first, first + count): the fresh state
__global__ __launch_bounds__(WG) void talkers_fresh(float *__restrict__ env, float *__restrict__ level, float *__restrict__ gate, float *__restrict__ target,
                                                    uint32_t first, uint32_t count) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= count) return;
    const uint32_t c = first + i;
    env[c] = 0.0f;
    level[c] = 0.0f;
    gate[c] = 1.0f;
    target[c] = 1.0f;
}

thread_local std::string g_err;        // the reason of the last failed create, plan or select on this thread

enum StoreKind : uint32_t { ST_DETECTOR, ST_PIN, ST_TOP, ST_FLOOR, ST_SEATS, ST_RESET };

// a store's vals: DETECTOR [count] attack gains, then [count] release gains; PIN / TOP count bytes; SEATS [members] channel numbers,
// then room_start[G + 1]; FLOOR and RESET carry none
struct StoreFields {
    StoreKind kind = ST_RESET;
    uint32_t first = 0, count = 0;
    float floor = 0.0f;
};
typedef StoreQueue<StoreFields> Stores;
typedef Stores::Store Store;

size_t bytes_as_floats(uint64_t n) { return (size_t)((n + 3) / 4); }

// ids[count]: each below G, or NONE
int check_ids(const char *call, const uint32_t *ids, uint64_t first, uint64_t count, uint32_t G, std::string &err) {
    for (uint64_t i = 0; i < count; ++i)
        if (ids[i] >= G && ids[i] != NONE) {
            char buf[192];
            std::snprintf(buf, sizeof buf, "talkers %s: channel %llu is given room %u, and there are %u rooms (or DSPFX_TALKERS_NO_ROOM)", call,
                          (unsigned long long)(first + i), ids[i], G);
            err = buf;
            return DSPFX_ERR_INVALID;
        }
    return DSPFX_OK;
}

int check_tops(const char *call, const uint8_t *tops, uint64_t first, uint64_t count, std::string &err) {
    for (uint64_t i = 0; i < count; ++i)
        if (tops[i] < 1 || tops[i] > MAX_TOP) {
            char buf[160];
            std::snprintf(buf, sizeof buf, "talkers %s: room %llu is given a top of %u (1 .. DSPFX_TALKERS_MAX_TOP = %u)", call,
                          (unsigned long long)(first + i), (unsigned)tops[i], MAX_TOP);
            err = buf;
            return DSPFX_ERR_INVALID;
        }
    return DSPFX_OK;
}

int room_too_large(const char *call, uint64_t room, uint64_t n, std::string &err) {
    char buf[192];
    std::snprintf(buf, sizeof buf, "talkers %s: room %llu would have %llu members, above DSPFX_TALKERS_MAX_ROOM = %u", call, (unsigned long long)room,
                  (unsigned long long)n, MAX_ROOM);
    err = buf;
    return DSPFX_ERR_INVALID;
}

// the table bytes of a bank on the device: env, gate, target, level and the two gains (24), the pin (1) and the member list (4)
// per channel; room_start (4), top (1) and the two tables of 8 (64) per room, and room_start's last entry.  By hand, as create's
// allocation and clearing are, not a channel_bank table list: the room tables go by G, the first seating is copied from host
// tables that create builds in between, and the audible list joins the bank later
uint64_t table_bytes(uint64_t N, uint64_t G) { return 29 * N + 69 * G + 4; }

// the seating of room_of[N] (every id below G, or NONE): members sorted by (room, channel) and room_start[G + 1].
// `rs` has G + 1 entries; returns the members listed
template <class RoomOf>
uint32_t build_seating(RoomOf room_of, uint64_t N, uint32_t G, uint32_t *members, uint32_t *rs) {
    std::fill(rs, rs + G + 1, 0u);
    for (uint64_t c = 0; c < N; ++c) {
        const uint32_t r = room_of(c);
        if (r != NONE) ++rs[r + 1];
    }
    for (uint32_t g = 0; g < G; ++g) rs[g + 1] += rs[g];
    const uint32_t total = rs[G];
    // fill in ascending channel order, rs[g] walking; then shift back
    for (uint64_t c = 0; c < N; ++c) {
        const uint32_t r = room_of(c);
        if (r != NONE) members[rs[r]++] = (uint32_t)c;
    }
    for (uint32_t g = G; g > 0; --g) rs[g] = rs[g - 1];
    rs[0] = 0;
    return total;
}

}  // namespace

struct dspfx_talkers : ChannelBank<dspfx_talkers_desc, StoreFields> {
    static constexpr const char *name = "talkers";
    std::vector<uint32_t> room_of;               // [N], with every assign made so far
    std::vector<uint32_t> counts;                // [G]
    std::vector<float> hga, hgr;                 // [N]: the gains, with every store made so far (a NULL slider keeps them)
    float *env = nullptr, *gate = nullptr, *target = nullptr, *level = nullptr, *ga = nullptr, *gr = nullptr, *tlev = nullptr;
    uint8_t *pin = nullptr, *top = nullptr;
    uint32_t *members = nullptr, *room_start = nullptr;
    int32_t *talkers = nullptr;
    // the audible list (dspfx_talkers_audible_views): made by the first call, under mu, and kept until release; while alist is set
    // every gated run launches talkers_audible
    int32_t *alist = nullptr;                    // [N]
    uint32_t *acount = nullptr;                  // [G]
    float floor = 0.0f;                          // as of the stores drained so far (mu)
};

namespace {

void release(dspfx_talkers *p) {
    release_bank(p, {p->env, p->gate, p->target, p->level, p->ga, p->gr, p->tlev, p->pin, p->top, p->members, p->room_start, p->talkers, p->alist,
                     p->acount});
}

// one store onto the stream
hipError_t apply_store(dspfx_talkers *p, const Store &st, hipStream_t s) {
    const uint32_t G = p->desc.n_groups;
    hipError_t err = hipSuccess;
    switch (st.kind) {
    case ST_DETECTOR:
        err = hipMemcpyAsync(p->ga + st.first, st.vals, (size_t)st.count * sizeof(float), hipMemcpyHostToDevice, s);
        if (err == hipSuccess) err = hipMemcpyAsync(p->gr + st.first, st.vals + st.count, (size_t)st.count * sizeof(float), hipMemcpyHostToDevice, s);
        return err;
    case ST_PIN:
        return hipMemcpyAsync(p->pin + st.first, st.vals, st.count, hipMemcpyHostToDevice, s);
    case ST_TOP:
        return hipMemcpyAsync(p->top + st.first, st.vals, st.count, hipMemcpyHostToDevice, s);
    case ST_FLOOR:
        p->floor = st.floor;
        return hipSuccess;
    case ST_SEATS:                               // count: the members listed
        if (st.count) err = hipMemcpyAsync(p->members, st.vals, (size_t)st.count * sizeof(uint32_t), hipMemcpyHostToDevice, s);
        if (err == hipSuccess)
            err = hipMemcpyAsync(p->room_start, st.vals + p->desc.n_channels, ((size_t)G + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s);
        return err;
    case ST_RESET:
        talkers_fresh<<<(st.count + WG - 1) / WG, WG, 0, s>>>(p->env, p->level, p->gate, p->target, st.first, st.count);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace

extern "C" const char *dspfx_talkers_last_error(const dspfx_talkers *p) { return p ? p->err.c_str() : g_err.c_str(); }

extern "C" float dspfx_envelope_gain(float frames) {       // dasp_envelope calc_gain, as dspfx_chain_set computes it
    return frames == 0.0f ? 0.0f : powf(2.71828182845904523536028747135266250f, -1.0f / frames);
}

extern "C" int dspfx_talkers_plan(uint64_t channels, uint32_t n_groups, uint64_t *bytes_out) {
    g_err.clear();
    const int rc = check_shape("talkers", channels, 0, g_err);
    if (rc != DSPFX_OK) return rc;
    if (n_groups == 0) {
        g_err = "talkers: no rooms";
        return DSPFX_ERR_INVALID;
    }
    if (bytes_out) *bytes_out = table_bytes(channels, n_groups);
    return DSPFX_OK;
}

extern "C" int dspfx_talkers_select(const float *levels, const uint32_t *room_of, uint64_t n_channels, uint32_t n_groups, const uint8_t *top, float floor,
                                    const uint8_t *pins, int32_t *talkers_out, float *levels_out, float *target_out) {
    g_err.clear();
    if (!levels || !room_of || !top || n_groups == 0) {
        g_err = "talkers select: levels, room_of, top or n_groups";
        return DSPFX_ERR_INVALID;
    }
    int rc = check_shape("talkers", n_channels, 0, g_err);
    if (rc == DSPFX_OK) rc = check_ids("select", room_of, 0, n_channels, n_groups, g_err);
    if (rc == DSPFX_OK) rc = check_tops("select", top, 0, n_groups, g_err);
    if (rc != DSPFX_OK) return rc;
    std::vector<uint32_t> members, rs;
    try {
        members.resize(n_channels);
        rs.resize((size_t)n_groups + 1);
    } catch (const std::bad_alloc &) {
        return DSPFX_ERR_OOM;
    }
    build_seating([&](uint64_t c) { return room_of[c]; }, n_channels, n_groups, members.data(), rs.data());
    for (uint32_t g = 0; g < n_groups; ++g)
        if (rs[g + 1] - rs[g] > MAX_ROOM) return room_too_large("select", g, rs[g + 1] - rs[g], g_err);
    if (target_out)
        for (uint64_t c = 0; c < n_channels; ++c) target_out[c] = pins && pins[c] == DSPFX_TALKERS_OPEN ? 1.0f : 0.0f;
    std::vector<uint8_t> taken(MAX_ROOM);
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t *m = members.data() + rs[g];
        const uint32_t n = rs[g + 1] - rs[g];
        std::fill(taken.begin(), taken.begin() + n, (uint8_t)0);
        for (uint32_t t = 0; t < MAX_TOP; ++t) {
            uint32_t best = n;
            if (t < top[g])
                for (uint32_t i = 0; i < n; ++i) {         // members ascend by channel: a strict > keeps the lower channel on a tie
                    const uint32_t c = m[i];
                    if (taken[i] || (pins && pins[c] != DSPFX_TALKERS_AUTO) || !(levels[c] > floor)) continue;
                    if (best == n || levels[c] > levels[m[best]]) best = i;
                }
            if (best < n) taken[best] = 1;
            if (talkers_out) talkers_out[(size_t)g * MAX_TOP + t] = best < n ? (int32_t)m[best] : -1;
            if (levels_out) levels_out[(size_t)g * MAX_TOP + t] = best < n ? levels[m[best]] : 0.0f;
            if (target_out && best < n) target_out[m[best]] = 1.0f;
        }
    }
    return DSPFX_OK;
}

extern "C" int dspfx_talkers_audible(const float *gate, const float *target, const uint32_t *room_of, uint64_t n_channels, uint32_t n_groups,
                                     int32_t *list_out, uint32_t *start_out, uint32_t *count_out) {
    g_err.clear();
    if (!gate || !target || !room_of || !list_out || !start_out || !count_out || n_groups == 0) {
        g_err = "talkers audible: gate, target, room_of, list_out, start_out, count_out or n_groups";
        return DSPFX_ERR_INVALID;
    }
    int rc = check_shape("talkers", n_channels, 0, g_err);
    if (rc == DSPFX_OK && n_channels > 0x7FFFFFFFull) {
        g_err = "talkers audible: the list holds int32_t channel numbers, and there are more than 2^31 - 1 channels";
        rc = DSPFX_ERR_INVALID;
    }
    if (rc == DSPFX_OK) rc = check_ids("audible", room_of, 0, n_channels, n_groups, g_err);
    if (rc != DSPFX_OK) return rc;
    // the members, sorted by (room, channel), straight into list_out; then every segment compacted in place, in order
    build_seating([&](uint64_t c) { return room_of[c]; }, n_channels, n_groups, (uint32_t *)list_out, start_out);
    for (uint32_t g = 0; g < n_groups; ++g)
        if (start_out[g + 1] - start_out[g] > MAX_ROOM) return room_too_large("audible", g, start_out[g + 1] - start_out[g], g_err);
    for (uint32_t g = 0; g < n_groups; ++g) {
        int32_t *seg = list_out + start_out[g];
        uint32_t k = 0;
        for (uint32_t i = 0; i < start_out[g + 1] - start_out[g]; ++i) {
            const int32_t c = seg[i];
            if (gate[c] != 0.0f || target[c] != 0.0f) seg[k++] = c;
        }
        count_out[g] = k;
    }
    return DSPFX_OK;
}

extern "C" int dspfx_talkers_create(const dspfx_talkers_desc *desc, dspfx_talkers **out) {
    if (!desc || !out) {
        g_err = "talkers: null argument";
        return DSPFX_ERR_INVALID;
    }
    *out = nullptr;
    g_err.clear();
    if (desc->abi_version != DSPFX_ABI_VERSION || desc->max_frames == 0 || desc->max_frames > (1u << 20)) {
        g_err = "talkers: abi_version or max_frames";
        return DSPFX_ERR_INVALID;
    }
    const uint32_t N = desc->n_channels, G = desc->n_groups;
    int rc = check_table("talkers", desc->group_start, G, N, desc->tile_channels, 0, g_err);
    if (rc != DSPFX_OK) return rc;
    for (uint32_t g = 0; g < G; ++g) {
        const uint64_t n = desc->group_start[g + 1] - desc->group_start[g];
        if (n == 0) {
            char buf[128];
            std::snprintf(buf, sizeof buf, "talkers: room %u is empty (a room has 1 .. %u members)", g, MAX_ROOM);
            g_err = buf;
            return DSPFX_ERR_INVALID;
        }
        if (n > MAX_ROOM) return room_too_large("create", g, n, g_err);
    }
    if (desc->top < 1 || desc->top > MAX_TOP) {
        char buf[128];
        std::snprintf(buf, sizeof buf, "talkers: top is %u (1 .. DSPFX_TALKERS_MAX_TOP = %u)", desc->top, MAX_TOP);
        g_err = buf;
        return DSPFX_ERR_INVALID;
    }
    const uint8_t top0 = (uint8_t)desc->top;
    rc = open_device("talkers", desc->device, &g_err);
    if (rc != DSPFX_OK) return rc;
    dspfx_talkers *p = new (std::nothrow) dspfx_talkers;
    if (!p) return DSPFX_ERR_OOM;
    p->desc = *desc;
    p->desc.group_start = nullptr;               // the caller's table is read here and not kept
    std::vector<uint32_t> hrs;
    try {
        p->room_of.resize(N);
        p->counts.resize(G);
        p->hga.assign(N, 0.0f);
        p->hgr.assign(N, 0.0f);
        hrs.resize((size_t)G + 1);
        for (uint32_t g = 0; g < G; ++g) {
            hrs[g] = (uint32_t)desc->group_start[g];
            p->counts[g] = (uint32_t)(desc->group_start[g + 1] - desc->group_start[g]);
            std::fill(p->room_of.begin() + desc->group_start[g], p->room_of.begin() + desc->group_start[g + 1], g);
        }
        hrs[G] = N;
    } catch (const std::bad_alloc &) {
        delete p;
        return DSPFX_ERR_OOM;
    }
    const size_t tab = (size_t)N * sizeof(float), rows = (size_t)G * MAX_TOP * sizeof(float);
    bool ok = hipMalloc((void **)&p->env, tab) == hipSuccess && hipMalloc((void **)&p->gate, tab) == hipSuccess &&
              hipMalloc((void **)&p->target, tab) == hipSuccess && hipMalloc((void **)&p->level, tab) == hipSuccess &&
              hipMalloc((void **)&p->ga, tab) == hipSuccess && hipMalloc((void **)&p->gr, tab) == hipSuccess &&
              hipMalloc((void **)&p->members, tab) == hipSuccess && hipMalloc((void **)&p->pin, N) == hipSuccess &&
              hipMalloc((void **)&p->room_start, ((size_t)G + 1) * sizeof(uint32_t)) == hipSuccess && hipMalloc((void **)&p->top, G) == hipSuccess &&
              hipMalloc((void **)&p->talkers, rows) == hipSuccess && hipMalloc((void **)&p->tlev, rows) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        release(p);
        char buf[160];
        std::snprintf(buf, sizeof buf, "talkers: no device memory for %llu bytes of tables (%u channels, %u rooms)", (unsigned long long)table_bytes(N, G), N, G);
        g_err = buf;
        return DSPFX_ERR_OOM;
    }
    // the fresh state; the first seating is the create table's: every member list entry is its own channel number
    std::vector<uint32_t> ident;
    try {
        ident.resize(N);
    } catch (const std::bad_alloc &) {
        release(p);
        return DSPFX_ERR_OOM;
    }
    for (uint32_t c = 0; c < N; ++c) ident[c] = c;
    talkers_fresh<<<(N + WG - 1) / WG, WG>>>(p->env, p->level, p->gate, p->target, 0u, N);
    ok = hipGetLastError() == hipSuccess && hipMemset(p->ga, 0, tab) == hipSuccess && hipMemset(p->gr, 0, tab) == hipSuccess &&
         hipMemset(p->pin, DSPFX_TALKERS_AUTO, N) == hipSuccess && hipMemset(p->top, (int)top0, G) == hipSuccess &&
         hipMemset(p->talkers, 0xFF, rows) == hipSuccess && hipMemset(p->tlev, 0, rows) == hipSuccess &&
         hipMemcpy(p->members, ident.data(), tab, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(p->room_start, hrs.data(), ((size_t)G + 1) * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess &&
         hipDeviceSynchronize() == hipSuccess && hipEventCreateWithFlags(&p->ev, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        release(p);
        return DSPFX_ERR_HIP;
    }
    *out = p;
    return DSPFX_OK;
}

extern "C" int dspfx_talkers_destroy(dspfx_talkers *p) { return destroy_bank(p, release); }

extern "C" int dspfx_talkers_set_detector(dspfx_talkers *p, const float *host_attack, const float *host_release, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_range(p, "set_detector", first_channel, count);
    if (rc != DSPFX_OK) return rc;
    if (count == 0 || (!host_attack && !host_release)) return DSPFX_OK;
    Store st;
    std::unique_lock<std::mutex> one;
    if (!stage_store(p, st, &one, ST_DETECTOR, "set_detector", first_channel, count, 2 * count, "staged sliders")) return DSPFX_ERR_OOM;
    float *a = st.vals, *r = st.vals + count;
    for (uint64_t i = 0; i < count; ++i) {
        a[i] = host_attack ? dspfx_envelope_gain(host_attack[i]) : p->hga[first_channel + i];
        r[i] = host_release ? dspfx_envelope_gain(host_release[i]) : p->hgr[first_channel + i];
    }
    p->stores.push(st, [&] {
        std::memcpy(p->hga.data() + first_channel, a, count * sizeof(float));
        std::memcpy(p->hgr.data() + first_channel, r, count * sizeof(float));
    });
    return DSPFX_OK;
}

namespace {

// count bytes for pin[first ..] or top[first ..]
int store_bytes(dspfx_talkers *p, StoreKind kind, const char *call, const uint8_t *host, uint64_t first, uint64_t count) {
    Store st;
    std::unique_lock<std::mutex> one;
    if (!stage_store(p, st, &one, kind, call, first, count, bytes_as_floats(count), "staged values")) return DSPFX_ERR_OOM;
    std::memcpy(st.vals, host, count);
    p->stores.push(st);
    return DSPFX_OK;
}

}  // namespace

extern "C" int dspfx_talkers_set_pin(dspfx_talkers *p, const uint8_t *host_pins, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    if (!host_pins) return p->fail(DSPFX_ERR_INVALID, "talkers set_pin: no array");
    const int rc = check_range(p, "set_pin", first_channel, count);
    if (rc != DSPFX_OK) return rc;
    for (uint64_t i = 0; i < count; ++i)
        if (host_pins[i] > DSPFX_TALKERS_SHUT) {
            char buf[176];
            std::snprintf(buf, sizeof buf, "talkers set_pin: channel %llu is given pin %u (DSPFX_TALKERS_AUTO, _OPEN and _SHUT are known)",
                          (unsigned long long)(first_channel + i), (unsigned)host_pins[i]);
            return p->fail(DSPFX_ERR_INVALID, buf);
        }
    if (count == 0) return DSPFX_OK;
    return store_bytes(p, ST_PIN, "set_pin", host_pins, first_channel, count);
}

extern "C" int dspfx_talkers_set_top(dspfx_talkers *p, const uint8_t *host_tops, uint64_t first_room, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    if (!host_tops) return p->fail(DSPFX_ERR_INVALID, "talkers set_top: no array");
    const uint64_t G = p->desc.n_groups;
    if (first_room > G || count > G - first_room) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "talkers set_top: rooms [%llu, %llu + %llu) are not inside the bank's %llu", (unsigned long long)first_room,
                      (unsigned long long)first_room, (unsigned long long)count, (unsigned long long)G);
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    std::string why;
    if (check_tops("set_top", host_tops, first_room, count, why) != DSPFX_OK) return p->fail(DSPFX_ERR_INVALID, why.c_str());
    if (count == 0) return DSPFX_OK;
    return store_bytes(p, ST_TOP, "set_top", host_tops, first_room, count);
}

extern "C" int dspfx_talkers_set_floor(dspfx_talkers *p, float floor) {
    if (!p) return DSPFX_ERR_INVALID;
    Store st;
    st.kind = ST_FLOOR;
    st.floor = floor;
    std::lock_guard<std::mutex> one(p->smu);
    p->stores.push(st);
    return DSPFX_OK;
}

extern "C" int dspfx_talkers_reset(dspfx_talkers *p, uint64_t first_channel, uint64_t count) {
    return store_plain(p, ST_RESET, "reset", first_channel, count);
}

extern "C" int dspfx_talkers_assign(dspfx_talkers *p, const uint32_t *host_room_ids, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    if (!host_room_ids || count == 0) return p->fail(DSPFX_ERR_INVALID, "talkers assign: no ids");
    const uint64_t N = p->desc.n_channels;
    const uint32_t G = p->desc.n_groups;
    int rc = check_range(p, "assign", first_channel, count);
    if (rc != DSPFX_OK) return rc;
    std::string why;
    if (check_ids("assign", host_room_ids, first_channel, count, G, why) != DSPFX_OK) return p->fail(DSPFX_ERR_INVALID, why.c_str());
    std::lock_guard<std::mutex> one(p->smu);
    // the map so far: only an assign changes it, and this is the only one running
    std::vector<uint32_t> cnt;
    try {
        cnt = p->counts;
    } catch (const std::bad_alloc &) {
        return p->fail(DSPFX_ERR_OOM, "talkers assign: no host memory");
    }
    for (uint64_t i = 0; i < count; ++i) {
        const uint32_t was = p->room_of[first_channel + i], now = host_room_ids[i];
        if (was != NONE) --cnt[was];
        if (now != NONE) ++cnt[now];
    }
    for (uint64_t i = 0; i < count; ++i) {
        const uint32_t now = host_room_ids[i];
        if (now != NONE && cnt[now] > MAX_ROOM) {
            room_too_large("assign", now, cnt[now], why);
            return p->fail(DSPFX_ERR_INVALID, why.c_str());
        }
    }
    Store st;                                    // (smu is held; count: the members listed, below)
    if (!stage_store(p, st, nullptr, ST_SEATS, "assign", 0, 0, (size_t)N + G + 1, "seating's tables")) return DSPFX_ERR_OOM;
    const uint32_t *old = p->room_of.data();
    st.count = build_seating([&](uint64_t c) { return c >= first_channel && c - first_channel < count ? host_room_ids[c - first_channel] : old[c]; }, N, G,
                             (uint32_t *)st.vals, (uint32_t *)st.vals + N);
    p->stores.push(st, [&] {
        std::memcpy(p->room_of.data() + first_channel, host_room_ids, count * sizeof(uint32_t));
        p->counts.swap(cnt);
    });
    return DSPFX_OK;
}

extern "C" int dspfx_talkers_audible_views(dspfx_talkers *p, const int32_t **list_out, const uint32_t **start_out, const uint32_t **count_out) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    if (!p->alist) {
        const size_t N = p->desc.n_channels, G = p->desc.n_groups;
        if (N > 0x7FFFFFFFull) return p->fail(DSPFX_ERR_INVALID, "talkers audible: the list holds int32_t channel numbers, and the bank has more than 2^31 - 1 channels");
        // on the caller's thread, once; count starts at 0 (nobody listed) and the device is idle on it before the first run reads it
        int32_t *list = nullptr;
        uint32_t *count = nullptr;
        const bool ok = hipSetDevice(p->desc.device) == hipSuccess && hipMalloc((void **)&list, N * sizeof(int32_t)) == hipSuccess &&
                        hipMalloc((void **)&count, G * sizeof(uint32_t)) == hipSuccess && hipMemset(list, 0xFF, N * sizeof(int32_t)) == hipSuccess &&
                        hipMemset(count, 0, G * sizeof(uint32_t)) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            if (list) (void)hipFree(list);
            if (count) (void)hipFree(count);
            return p->fail(DSPFX_ERR_OOM, "talkers audible: no device memory for the list (4 bytes per channel and 4 per room)");
        }
        p->acount = count;
        p->alist = list;
    }
    if (list_out) *list_out = p->alist;
    if (start_out) *start_out = p->room_start;
    if (count_out) *count_out = p->acount;
    return DSPFX_OK;
}

extern "C" int dspfx_talkers_room_of(dspfx_talkers *p, uint32_t *host_ids_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "room_of", host_ids_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = p->room_of[c]; });
}

extern "C" int dspfx_talkers_counts(dspfx_talkers *p, uint32_t *host_counts_out) {
    if (!p) return DSPFX_ERR_INVALID;
    if (!host_counts_out) return p->fail(DSPFX_ERR_INVALID, "talkers counts: no array");
    std::lock_guard<std::mutex> lk(p->stores.qmu);
    std::memcpy(host_counts_out, p->counts.data(), p->counts.size() * sizeof(uint32_t));
    return DSPFX_OK;
}

extern "C" int dspfx_talkers_views(dspfx_talkers *p, const float **level_out, const float **target_out, const int32_t **talkers_out,
                                   const float **talker_levels_out) {
    if (!p) return DSPFX_ERR_INVALID;
    if (level_out) *level_out = p->level;
    if (target_out) *target_out = p->target;
    if (talkers_out) *talkers_out = p->talkers;
    if (talker_levels_out) *talker_levels_out = p->tlev;
    return DSPFX_OK;
}

extern "C" int dspfx_talkers_run(dspfx_talkers *p, const float *in, float *out, uint32_t n_frames, void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    hipStream_t s = (hipStream_t)stream;
    const int rc = begin_run(p, in != nullptr, n_frames, s, "talkers run: in or n_frames", "talkers store", apply_store);
    if (rc != DSPFX_OK) return rc;
    TalkArgs a;
    a.in = in;
    a.out = out;
    a.env = p->env;
    a.gate = p->gate;
    a.target = p->target;
    a.level = p->level;
    a.ga = p->ga;
    a.gr = p->gr;
    a.pin = p->pin;
    a.N = p->desc.n_channels;
    a.W = p->desc.tile_channels;
    a.nf = n_frames;
    const auto [vec, lanes, blocks] = lane_plan(a.N, a.W, (uintptr_t)in | (uintptr_t)out, WG);
    const uint32_t G = p->desc.n_groups;
    if (p->alist && out) {                       // behind the stores and ahead of pass A, which overwrites gate
        talkers_audible<<<(G + WG / 64 - 1) / (WG / 64), WG, 0, s>>>(p->gate, p->target, p->members, p->room_start, p->alist, p->acount, G, a.N);
        BANK_HIP_WHY(hipGetLastError(), "talkers_audible");
    }
    if (vec && out) talkers_run<4, true><<<blocks, WG, 0, s>>>(a);
    else if (vec) talkers_run<4, false><<<blocks, WG, 0, s>>>(a);
    else if (out) talkers_run<1, true><<<blocks, WG, 0, s>>>(a);
    else talkers_run<1, false><<<blocks, WG, 0, s>>>(a);
    BANK_HIP_WHY(hipGetLastError(), "talkers_run");
    talkers_pick<<<(G + WG / 64 - 1) / (WG / 64), WG, 0, s>>>(p->level, p->pin, p->members, p->room_start, p->top, p->floor, p->target, p->talkers, p->tlev, G,
                                                            a.N);
    BANK_HIP_WHY(hipGetLastError(), "talkers_pick");
    return DSPFX_OK;
}
