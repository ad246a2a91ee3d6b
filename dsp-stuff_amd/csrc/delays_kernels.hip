// delays_kernels.hip -- the channel-delay bank (include/dspfx.h, dspfx_delays_*): every channel may carry its own Reverb node
// (reverb.rs:55-110, a feedback delay line) with its own `seconds` and `decay` sliders and its own ring.  What the reference has
// when N graphs each hold their own Reverb.
//
// The rings are channel-major, [N][cap]: with one length per channel neighbouring channels read their delayed sample from
// different ring positions, so a [row][N] ring would cost a cache line per sample; here the 128 taps a channel needs for 128 frames
// are 512 contiguous bytes of its own ring (wrapping once at most), and so are the 128 frames it writes back, whatever the lengths
// of its neighbours.  The block has the channel on the lane, the ring has the frame on the lane, so the taps cross LDS:
//   a workgroup takes TC = 64 adjacent channels and walks the block in chunks of FC = 128 frames;
//   gather   each wave takes 16 of the channels in turn: the channel's taps of the chunk, frame on the lane (256 contiguous bytes
//            per wave-instruction, the ring position wave-uniform, eight channels' loads in flight), into the channel's row of the LDS tile; a tap the mask covers
//            (the ring is not zeroed by a store, it reads as +0.0 for D frames) is not loaded;
//   compute  channel on the lane, four adjacent channels per lane: the frame's 16-byte load (bank_common's vec; four 4-byte loads
//            otherwise), the hop, out = in + tap * decay with the tap from the tile, the new sample back into the tile, the
//            16-byte nontemporal store.  A lane rewrites the elements it read, so out may be in;
//   scatter  as the gather, the chunk's new samples from the tile rows to the rings.
// The tile's rows are FC + 1 floats apart: a compute access has (4 q + j) * 129 + f, 16 q and 4 f per wave, on 64 different
// banks, and a gather / scatter access is 64 consecutive floats.  A workgroup none of whose channels carries a node it runs
// (no node, or n_frames above the ring's length: reverb.rs:92-96) moves no ring byte, touches no LDS and meets no barrier: a
// nodeless bank's run is a copy.  Nothing is shared between channels beyond the tile's rows: no atomics, and a channel's bits do
// not depend on its neighbours.  One run touches no ring slot twice (n_frames <= D), so the chunks need no order among them.
//
// Slider stores go through the staged-store queue (store_queue.hip.h); a store's device side is two small copies (lengths, decays)
// and one kernel over the stored channels that puts the ring position to 0 and the count of still-zero taps to D: the reference's
// new zero-filled ring (reverb.rs:60-68) without a memset.
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

constexpr uint32_t WG = 256;
constexpr uint32_t TC = 64;                        // channels of a workgroup
constexpr uint32_t FC = 128;                       // frames of a chunk
constexpr uint32_t PITCH = FC + 1;                 // floats between two channels' rows of the tile
constexpr uint32_t LPR = TC / 4;                   // compute: lanes across the channels (four each) ...
constexpr uint32_t FSTEP = WG / LPR;               // ... so a workgroup covers this many frames at a time
constexpr uint32_t ROWS = FC / FSTEP;              // frames of a chunk per lane
constexpr uint32_t UB = 4;                         // ... taken in batches of UB loads ahead of their arithmetic
constexpr uint32_t CPW = TC / (WG / 64);           // gather / scatter: channels per wave
constexpr uint32_t GB = 8;                         // gather: channels whose loads are in flight together (16 loads a lane)
constexpr uint64_t MAX_CAP = 1ull << 31;

struct DelayArgs {
    const float *in;             // may be `out`: no __restrict__
    float *out;
    float *ring;                 // [N][cap]
    const uint32_t *len;         // [N]: D_c; 0: no node
    uint32_t *pos;               // [N]: the ring slot of the next frame
    uint32_t *zero;              // [N]: the frames whose tap still reads as +0.0
    const float *decay;          // [N]
    uint32_t N, W, nf, flags, cap;
    float div;                   // f32(0.0001 + 1.0)
};

template <bool VEC>
__global__ __launch_bounds__(WG) void delays_run(DelayArgs a) {
    __shared__ float tile[TC * PITCH];
    __shared__ uint32_t s_len[TC], s_live[TC], s_pos[TC], s_zero[TC];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t c0 = blockIdx.x * TC;
    // the span's nodes: a channel is live when it carries a node this run goes through (n_frames <= D)
    uint32_t myD = 0, mypos = 0, myzero = 0, mylive = 0;
    if (t < TC) {
        const uint32_t c = c0 + t;
        if (c < a.N) myD = a.len[c];
        mylive = myD != 0 && a.nf <= myD;
        if (mylive) {
            mypos = a.pos[c];
            myzero = a.zero[c];
        }
        s_len[t] = myD;
        s_live[t] = mylive;
        s_pos[t] = mypos;
        s_zero[t] = myzero;
    }
    const bool any = __syncthreads_or((int)mylive) != 0;

    // compute: the lane's four channels
    const uint32_t lc = (t % LPR) * 4, fr = t / LPR, c = c0 + lc;
    const size_t rs = a.W ? a.W : a.N;
    size_t base[4];
    bool in_n[4], pres[4], live[4];
    float dec[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        in_n[j] = c + j < a.N;
        base[j] = in_n[j] ? lay(0, c + j, a.nf, a.N, a.W) : 0;
        pres[j] = s_len[lc + j] != 0;
        live[j] = s_live[lc + j] != 0;
        dec[j] = live[j] ? a.decay[c + j] : 0.0f;
    }
    const bool hop = (a.flags & DSPFX_LINK_INPUT) != 0;

#pragma unroll 1
    for (uint32_t f0 = 0; f0 < a.nf; f0 += FC) {
        const uint32_t n = min(FC, a.nf - f0);
        if (any) {
            if (f0) __syncthreads();                         // the scatter of the chunk before has read the tile
            // gather: the chunk's taps, a channel at a time, frame on the lane
#pragma unroll 1
            for (uint32_t g = 0; g < CPW; g += GB) {
                float v[GB][2];
#pragma unroll
                for (uint32_t u = 0; u < GB; ++u) {
                    const uint32_t ch = wave * CPW + g + u;
                    const uint32_t D = s_len[ch];
                    const uint32_t start = s_live[ch] ? (s_pos[ch] + f0) % D : 0;
                    const float *row = a.ring + (size_t)(c0 + ch) * a.cap;
#pragma unroll
                    for (uint32_t k = 0; k < 2; ++k) {
                        const uint32_t i = lane + 64 * k;
                        uint32_t r = start + i;
                        if (r >= D) r -= D;
                        v[u][k] = 0.0f;
                        if (s_live[ch] && i < n && f0 + i >= s_zero[ch]) v[u][k] = row[r];
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < GB; ++u) {
                    const uint32_t ch = wave * CPW + g + u;
                    if (s_live[ch]) {
                        tile[ch * PITCH + lane] = v[u][0];
                        tile[ch * PITCH + lane + 64] = v[u][1];
                    }
                }
            }
            __syncthreads();
        }
        // compute: channel on the lane
#pragma unroll 1
        for (uint32_t b = 0; b < ROWS; b += UB) {
            float x[UB][4];
#pragma unroll
            for (uint32_t u = 0; u < UB; ++u) {
                const uint32_t f = fr + (b + u) * FSTEP;
                if (f >= n) continue;
                const size_t off = (size_t)(f0 + f) * rs;
                if (VEC) {
                    if (in_n[0]) {
                        const f32x4 q = *(const f32x4 *)(a.in + base[0] + off);
                        x[u][0] = q.x, x[u][1] = q.y, x[u][2] = q.z, x[u][3] = q.w;
                    }
                } else {
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j)
                        if (in_n[j]) x[u][j] = a.in[base[j] + off];
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < UB; ++u) {
                const uint32_t f = fr + (b + u) * FSTEP;
                if (f >= n) continue;
                const size_t off = (size_t)(f0 + f) * rs;
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    if (!in_n[j] || !pres[j]) continue;      // no node: the input's bits
                    float y = x[u][j];
                    if (hop) y = __fdiv_rn(__fadd_rn(0.0f, y), a.div);         // node.rs:162-194, one connected pipe
                    if (live[j]) {                           // reverb.rs:86-91, 99-103
                        float *slot = &tile[(lc + j) * PITCH + f];
                        y = __fadd_rn(y, __fmul_rn(*slot, dec[j]));
                        *slot = y;
                    }
                    x[u][j] = y;
                }
                if (VEC) {
                    if (in_n[0]) {
                        const f32x4 q = {x[u][0], x[u][1], x[u][2], x[u][3]};
                        __builtin_nontemporal_store(q, (f32x4 *)(a.out + base[0] + off));
                    }
                } else {
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j)
                        if (in_n[j]) __builtin_nontemporal_store(x[u][j], a.out + base[j] + off);
                }
            }
        }
        if (any) {
            __syncthreads();
            // scatter: the chunk's new samples, a channel at a time, frame on the lane
#pragma unroll 1
            for (uint32_t g = 0; g < CPW; ++g) {
                const uint32_t ch = wave * CPW + g;
                if (!s_live[ch]) continue;
                const uint32_t D = s_len[ch];
                const uint32_t start = (s_pos[ch] + f0) % D;
                float *row = a.ring + (size_t)(c0 + ch) * a.cap;
#pragma unroll
                for (uint32_t k = 0; k < 2; ++k) {
                    const uint32_t i = lane + 64 * k;
                    uint32_t r = start + i;
                    if (r >= D) r -= D;
                    if (i < n) row[r] = tile[ch * PITCH + i];
                }
            }
        }
    }
    if (mylive) {                                            // (t < TC)
        a.pos[c0 + t] = (mypos + a.nf) % myD;
        a.zero[c0 + t] = myzero > a.nf ? myzero - a.nf : 0u;
    }
}

// a store's bookkeeping on the device, in stream order, on channels [first, first + count): a new zero ring of the length just
// copied into len (drop: no node)
__global__ __launch_bounds__(WG) void delays_store(uint32_t *__restrict__ len, uint32_t *__restrict__ pos, uint32_t *__restrict__ zero,
                                                   uint32_t first, uint32_t count, uint32_t drop) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= count) return;
    const uint32_t c = first + i;
    if (drop) len[c] = 0u;
    pos[c] = 0u;
    zero[c] = drop ? 0u : len[c];
}

thread_local std::string g_err;        // the reason of the last failed create or plan on this thread

// a store's vals: [count] lengths (as bits), then [count] decays; none: the node is dropped
struct StoreFields {
    uint32_t first = 0, count = 0;
};
typedef StoreQueue<StoreFields> Stores;
typedef Stores::Store Store;

// cap and the ring bytes of a bank, or the reason there is none
int plan(uint64_t N, float max_seconds, int page_round, uint32_t *cap_out, uint64_t *bytes_out, std::string &err) {
    const int rc = check_shape("delays", N, 0, err);
    if (rc != DSPFX_OK) return rc;
    const uint64_t cap = dspfx_delay_len(max_seconds, page_round ? 1 : 0);
    if (cap > MAX_CAP) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "delays: max_seconds %g is a ring of %llu frames, above 2^31", (double)max_seconds, (unsigned long long)cap);
        err = buf;
        return DSPFX_ERR_INVALID;
    }
    if (cap_out) *cap_out = (uint32_t)cap;
    if (bytes_out) *bytes_out = N * cap * sizeof(float);
    return DSPFX_OK;
}

}  // namespace

struct dspfx_delays : ChannelBank<dspfx_delays_desc, StoreFields> {
    static constexpr const char *name = "delays";
    uint32_t cap = 0;
    std::vector<uint32_t> hlen;                  // D_c, 0: no node -- with every store made so far, as hsec and hdec
    std::vector<float> hsec, hdec;               // the sliders; 0.5 for a channel never stored (reverb.rs:29-38)
    float *ring = nullptr, *decay = nullptr;
    uint32_t *len = nullptr, *pos = nullptr, *zero = nullptr;
    float div = 1.0f;
    // the fresh state: no node anywhere.  The rings are not zeroed: a channel's first store says its next D taps read as +0.0
    template <class V>
    static void tables(const dspfx_delays_desc &d, V v) {
        const uint64_t N = d.n_channels;
        v(N * dspfx_delay_len(d.max_seconds, d.page_round ? 1 : 0) * 4, TABLE_BY_HAND, &dspfx_delays::ring);
        v(4 * N, 0, &dspfx_delays::decay);
        v(4 * N, 0, &dspfx_delays::len);
        v(4 * N, 0, &dspfx_delays::pos);
        v(4 * N, 0, &dspfx_delays::zero);
    }
};

namespace {

// one store onto the stream: its lengths and decays, then the new zero ring on its channels
hipError_t apply_store(dspfx_delays *p, const Store &st, hipStream_t s) {
    const uint32_t blocks = (st.count + WG - 1) / WG;
    if (st.vals) {
        hipError_t err = hipMemcpyAsync(p->len + st.first, st.vals, (size_t)st.count * sizeof(uint32_t), hipMemcpyHostToDevice, s);
        if (err == hipSuccess)
            err = hipMemcpyAsync(p->decay + st.first, st.vals + st.count, (size_t)st.count * sizeof(float), hipMemcpyHostToDevice, s);
        if (err != hipSuccess) return err;
    }
    delays_store<<<blocks, WG, 0, s>>>(p->len, p->pos, p->zero, st.first, st.count, st.vals ? 0u : 1u);
    return hipGetLastError();
}

}  // namespace

extern "C" const char *dspfx_delays_last_error(const dspfx_delays *p) { return p ? p->err.c_str() : g_err.c_str(); }

extern "C" int dspfx_delays_plan(uint64_t channels, float max_seconds, int page_round, uint32_t *cap_out, uint64_t *bytes_out) {
    g_err.clear();
    return plan(channels, max_seconds, page_round, cap_out, bytes_out, g_err);
}

extern "C" int dspfx_delays_create(const dspfx_delays_desc *desc, dspfx_delays **out) {
    char buf[192];
    uint32_t cap = 0;
    uint64_t bytes = 0;
    const int rc = create_checks(desc, out, g_err, [&](std::string &err) -> int {
        if (desc->link_flags & ~(DSPFX_LINK_INTERNAL | DSPFX_LINK_INPUT)) {
            std::snprintf(buf, sizeof buf, "delays: unknown link flag in 0x%x (DSPFX_LINK_INTERNAL and DSPFX_LINK_INPUT are known)", desc->link_flags);
            err = buf;
            return DSPFX_ERR_INVALID;
        }
        return plan(desc->n_channels, desc->max_seconds, (int)desc->page_round, &cap, &bytes, err);
    });
    if (rc != DSPFX_OK) return rc;
    const uint32_t N = desc->n_channels;
    std::snprintf(buf, sizeof buf, "delays: no device memory for %llu bytes of rings (%u channels of %u frames) and the tables", (unsigned long long)bytes,
                  N, cap);
    return create_bank(
        desc, out, g_err,
        [N, cap](dspfx_delays *p) {
            p->cap = cap;
            p->div = dspfx_link_divisor(1);
            p->hlen.assign(N, 0u);
            p->hsec.assign(N, 0.5f);
            p->hdec.assign(N, 0.5f);
        },
        nullptr, buf);
}

extern "C" int dspfx_delays_destroy(dspfx_delays *p) { return destroy_bank(p); }

extern "C" int dspfx_delays_set_delay(dspfx_delays *p, const float *host_seconds, const float *host_decay, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_range(p, "set_delay", first_channel, count);
    if (rc != DSPFX_OK) return rc;
    if (count == 0) return DSPFX_OK;
    Store st;
    st.first = (uint32_t)first_channel;
    st.count = (uint32_t)count;
    std::lock_guard<std::mutex> one(p->smu);
    if (!host_seconds && !host_decay) {                      // the node is dropped; a later store meets the defaults again
        p->stores.push(st, [&] {
            for (uint64_t i = 0; i < count; ++i) {
                p->hlen[first_channel + i] = 0u;
                p->hsec[first_channel + i] = p->hdec[first_channel + i] = 0.5f;
            }
        });
        return DSPFX_OK;
    }
    // refresh_seconds (reverb.rs:55-71) from each channel's CURRENT seconds slider: the store is made whole or not at all
    const int pr = p->desc.page_round ? 1 : 0;
    for (uint64_t i = 0; i < count; ++i) {
        const float sec = host_seconds ? host_seconds[i] : p->hsec[first_channel + i];
        const uint32_t D = dspfx_delay_len(sec, pr);
        if (D > p->cap) {
            char buf[192];
            std::snprintf(buf, sizeof buf, "delays set_delay: channel %llu at %g seconds needs a ring of %u frames, and the bank's rings hold %u",
                          (unsigned long long)(first_channel + i), (double)sec, D, p->cap);
            return p->fail(DSPFX_ERR_INVALID, buf);
        }
    }
    if (!stage_store(p, st, nullptr, "set_delay", first_channel, count, 2 * count, "staged sliders")) return DSPFX_ERR_OOM;      // (smu is held)
    uint32_t *lens = (uint32_t *)st.vals;
    float *decs = st.vals + count;
    for (uint64_t i = 0; i < count; ++i) {
        lens[i] = dspfx_delay_len(host_seconds ? host_seconds[i] : p->hsec[first_channel + i], pr);
        decs[i] = host_decay ? host_decay[i] : p->hdec[first_channel + i];
    }
    p->stores.push(st, [&] {
        for (uint64_t i = 0; i < count; ++i) {
            p->hlen[first_channel + i] = lens[i];
            p->hdec[first_channel + i] = decs[i];
            if (host_seconds) p->hsec[first_channel + i] = host_seconds[i];
        }
    });
    return DSPFX_OK;
}

extern "C" int dspfx_delays_present(dspfx_delays *p, uint32_t *host_present_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "present", host_present_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = p->hlen[c] != 0; });
}

extern "C" int dspfx_delays_lengths(dspfx_delays *p, uint32_t *host_lengths_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "lengths", host_lengths_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = p->hlen[c]; });
}

extern "C" int dspfx_delays_run(dspfx_delays *p, const float *in, float *out, uint32_t n_frames, void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    hipStream_t s = (hipStream_t)stream;
    const int rc = begin_run(p, in && out, n_frames, s, "delays run: in, out or n_frames", "slider store", apply_store);
    if (rc != DSPFX_OK) return rc;
    DelayArgs a;
    a.in = in;
    a.out = out;
    a.ring = p->ring;
    a.len = p->len;
    a.pos = p->pos;
    a.zero = p->zero;
    a.decay = p->decay;
    a.N = p->desc.n_channels;
    a.W = p->desc.tile_channels;
    a.nf = n_frames;
    a.flags = p->desc.link_flags;
    a.cap = p->cap;
    a.div = p->div;
    const uint32_t blocks = (a.N + TC - 1) / TC;         // a workgroup takes TC channels; only the lane decision is lane_io's
    if (lane_plan(a.N, a.W, (uintptr_t)in | (uintptr_t)out, WG).vec) delays_run<true><<<blocks, WG, 0, s>>>(a);
    else delays_run<false><<<blocks, WG, 0, s>>>(a);
    BANK_HIP_WHY(hipGetLastError(), "delays_run");
    return DSPFX_OK;
}

// every present channel's ring back to zeros: the store's kernel over all channels, the lengths as they are
extern "C" int dspfx_delays_reset(dspfx_delays *p) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    if (!p->used) return DSPFX_OK;               // no run yet: no store has reached the device, and a queued one starts from zeros
    BANK_HIP_WHY(hipSetDevice(p->desc.device), "hipSetDevice");
    const uint32_t N = p->desc.n_channels;
    delays_store<<<(N + WG - 1) / WG, WG, 0, p->last>>>(p->len, p->pos, p->zero, 0u, N, 0u);
    BANK_HIP_WHY(hipGetLastError(), "delays reset");
    return DSPFX_OK;
}
