// mixgroups_kernels.hip -- the mix-group bank (include/dspfx.h, dspfx_mixgroups_*): one Output bus per contiguous channel range,
// with a per-channel fader.  buses[f][g] = (sum over the channels c of group g of fl32(x[f][c] * gain[c])) / link_divisor(n_g).
//
// The block is read once.  The channel axis is cut into SPANS of 256 channels from channel 0 (a span is what one wave reads of a
// frame with one 16-byte load per lane); a group's sum is put together from PIECES, one per span it touches:
//   partials  one wave per (span, chunk of 16 frames).
//             A span that lies wholly inside one group (host table `slow` = 0): lane l adds its four channels
//             (x0 + x1) + (x2 + x3), then the 64 lanes are added across lane bits 32, 16, 8, 4, 2, 1 (wave_reduce_scatter: the
//             chunk's frames are reduced together and every fourth lane ends up with one frame, so the piece is written as one row).
//             A span with a group boundary (or the end of the channels) inside: four sub-rows of 64 channels, one per lane; in
//             each a segmented Hillis-Steele scan (steps 1, 2, .. 32, a lane adds the value `step` lanes below it while that
//             lane is still in its own group), so the last lane of a group holds the group's sum over the sub-row; a group that
//             goes on into the next sub-row carries that sum over, carry + scan.  A group that ends inside the span it began
//             in is complete: its bus is written from here.  The group that came in from the span before leaves its sum in L[span],
//             the group that goes on into the next span in R[span].  A whole span's piece is L[span] too.
//   reduce    a group's pieces, [R[first span]], L[..], in order; up to 64 of them per workgroup and frame: wave w of four adds
//             pieces w, w + 4, w + 8, .. one after the other, then (w0 + w1) + (w2 + w3); more than 64 pieces take a further
//             level of the same over the results.  The last level divides (IEEE) and writes the bus.
// Which additions make a group's sum follows from the group's own first channel and length (and the layout) alone: no atomics,
// nothing depends on the order waves run in or on the other groups.  dspfx_mixgroups_plan gives the depth of that tree.
//
// Per-channel returns (dspfx_mixgroups_returns): returns[f][c] = fl32(fl32(S[f][g] - t[f][c]) / link_divisor(n_g - 1)), every
// channel hears its room minus itself.  The two kernels above, unchanged, are pointed at divisor tables of 1.0 and at the bank's
// own [max_frames][G] buffer, which so holds the raw sums S; then
//   divide    (only when the caller wants the buses too) buses = S / link_divisor(n_g), what `run` writes, the block not re-read;
//   returns   one streaming pass, one wave per (span, chunk of 16 frames), a lane takes four adjacent channels with one 16-byte
//             load and one 16-byte store per frame.  A span inside one group takes the group from a per-span table (sfirst, built
//             when the first returns call is made) and S[f][g] is one wave-uniform load; a cut span looks its channels' groups up
//             once per wave, between the first group of this span and the first group of the next, and gathers S per frame.
//             A lane rewrites the elements it read, so returns may be the block itself.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/dspfx.h"
#include "bank_common.hip.h"
#include "chain_kernels.hip.h"

namespace {

constexpr uint32_t SPAN = 256;                     // channels per span
constexpr uint32_t SUB = 64;                       // channels per sub-row of a span with boundaries
constexpr uint32_t FAN = 64;                       // pieces one reduce workgroup takes
constexpr uint32_t RW = 4;                         // its waves
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t P1_WG = 256;
constexpr int CHUNK = 16;                          // frames per wave of the partials kernel (64 keep every loaded frame in registers: one wave per SIMD)

struct Task {
    uint32_t src0;       // piece j is row src0 + j of the level's source ...
    uint32_t count;
    uint32_t rslot;      // ... except piece 0 when rslot != NONE: row rslot of R
    uint32_t dst;        // the group (last level) or the row of the next level's source
    float div;
    uint32_t final;
};

struct P1Args {
    const float *x;
    const float *gain;           // [N]
    float *L, *R;                // [nspans][FS]
    float *bus;                  // [nf][G]
    const uint32_t *gstart;      // [G + 1]
    const float *gdiv;           // [G]
    const uint8_t *slow;         // [nspans]
    uint32_t N, Wrow, nf, G, FS, nspans, nchunks;
};

// the offset of channel ch in frame 0 of a block of nf frames; a frame further is Wrow elements on
__device__ __forceinline__ size_t chan_base(uint32_t ch, uint32_t Wrow, uint32_t nf) {
    const uint32_t t = ch / Wrow;
    return (size_t)t * nf * Wrow + (ch - t * Wrow);
}

template <int F, bool GAIN, bool VEC>
__device__ __forceinline__ void whole_span(const P1Args &a, uint32_t k, uint32_t f0, uint32_t lane) {
    const uint32_t ch = k * SPAN + 4 * lane;
    size_t b[4];
    b[0] = chan_base(ch, a.Wrow, a.nf);
    if (!VEC) {
#pragma unroll
        for (int i = 1; i < 4; ++i) b[i] = chan_base(ch + i, a.Wrow, a.nf);
    }
    float4 g = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    if (GAIN) g = *(const float4 *)(a.gain + ch);
    float r[F];
#pragma unroll
    for (int i0 = 0; i0 < F; i0 += 8) {
        float4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t f = f0 + i0 + j;
            v[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (f < a.nf) {
                const size_t o = (size_t)f * a.Wrow;
                if (VEC) {
                    v[j] = *(const float4 *)(a.x + b[0] + o);
                } else {
                    v[j].x = a.x[b[0] + o];
                    v[j].y = a.x[b[1] + o];
                    v[j].z = a.x[b[2] + o];
                    v[j].w = a.x[b[3] + o];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float4 t = v[j];
            if (GAIN) t = make_float4(__fmul_rn(t.x, g.x), __fmul_rn(t.y, g.y), __fmul_rn(t.z, g.z), __fmul_rn(t.w, g.w));
            r[i0 + j] = (t.x + t.y) + (t.z + t.w);
        }
    }
    dspfx::wave_reduce_scatter<F>(r, (int)lane);
    const uint32_t f = f0 + (uint32_t)dspfx::mixbus_frame_of_lane<F>((int)lane);
    if (dspfx::mixbus_lane_writes<F>((int)lane) && f < a.nf) a.L[(size_t)k * a.FS + f] = r[0];
}

template <int F, bool GAIN>
__device__ __forceinline__ void cut_span(const P1Args &a, uint32_t k, uint32_t f0, uint32_t lane) {
    const uint32_t c0 = k * SPAN;
    uint32_t head[4], gi[4];
    bool valid[4], tail[4], joins[4], direct[4];
    float dv[4], gn[4];
    size_t b[4];
    bool goes_on[4];                 // wave-uniform: the group of the sub-row's last channel goes on past the sub-row
    int l_row = -1, l_lane = 0;      // wave-uniform: where the group that came in from the span before ends
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t lo = c0 + SUB * r, ch = lo + lane;
        valid[r] = ch < a.N;
        uint32_t g = 0, gs = 0, ge = 0;
        if (valid[r]) {
            uint32_t i0 = 0, i1 = a.G;                   // the first i in [0, G] with gstart[i] > ch; gstart[G] = N > ch
            while (i0 < i1) {
                const uint32_t m = (i0 + i1) / 2;
                if (a.gstart[m] > ch) i1 = m;
                else i0 = m + 1;
            }
            g = i0 - 1;
            gs = a.gstart[g];
            ge = a.gstart[g + 1];
        }
        gi[r] = g;
        head[r] = valid[r] ? (gs > lo ? gs - lo : 0u) : lane;
        tail[r] = valid[r] && ch == ge - 1;
        joins[r] = valid[r] && gs < lo && r > 0;         // (of the sub-row's first segment) it began in an earlier sub-row
        const bool came_in = valid[r] && gs < c0;
        direct[r] = tail[r] && !came_in;
        dv[r] = valid[r] ? a.gdiv[g] : 1.0f;
        gn[r] = (GAIN && valid[r]) ? a.gain[ch] : 1.0f;
        b[r] = valid[r] ? chan_base(ch, a.Wrow, a.nf) : 0;
        const unsigned long long on = __ballot(lane == 63 && valid[r] && !tail[r]);
        goes_on[r] = on != 0;
        const unsigned long long lm = __ballot(tail[r] && came_in);
        if (lm) {
            l_row = r;
            l_lane = __ffsll((long long)lm) - 1;
        }
    }
    float keep_l = 0.0f, keep_r = 0.0f;
    for (uint32_t i = 0; i < (uint32_t)F; ++i) {
        const uint32_t f = f0 + i;
        if (f >= a.nf) break;
        const size_t o = (size_t)f * a.Wrow;
        float x[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) x[r] = valid[r] ? a.x[b[r] + o] : 0.0f;
        float carry = 0.0f, lval = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = GAIN ? __fmul_rn(x[r], gn[r]) : x[r];
#pragma unroll
            for (uint32_t d = 1; d < 64; d *= 2) {
                const float u = __shfl_up(v, d, 64);
                if (lane >= head[r] + d) v += u;
            }
            if (joins[r] && head[r] == 0) v = carry + v;
            if (direct[r]) a.bus[(size_t)f * a.G + gi[r]] = __fdiv_rn(v, dv[r]);
            if (r == l_row) lval = __shfl(v, l_lane, 64);
            carry = goes_on[r] ? __shfl(v, 63, 64) : 0.0f;
        }
        if (lane == i) {
            keep_l = lval;
            keep_r = carry;
        }
    }
    const uint32_t f = f0 + lane;
    if (lane < (uint32_t)F && f < a.nf) {
        if (l_row >= 0) a.L[(size_t)k * a.FS + f] = keep_l;
        if (goes_on[3]) a.R[(size_t)k * a.FS + f] = keep_r;
    }
}

template <int F, bool GAIN, bool VEC>
__global__ __launch_bounds__(P1_WG) void mixgroups_partials(P1Args a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t item = blockIdx.x * (P1_WG / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= a.nspans * a.nchunks) return;
    const uint32_t k = item / a.nchunks, f0 = (item - k * a.nchunks) * F;
    if (a.slow[k]) cut_span<F, GAIN>(a, k, f0, lane);
    else whole_span<F, GAIN, VEC>(a, k, f0, lane);
}

__global__ __launch_bounds__(RW * 64) void mixgroups_reduce(const Task *__restrict__ tasks, const float *__restrict__ src,
                                                            const float *__restrict__ rsrc, float *__restrict__ next,
                                                            float *__restrict__ bus, uint32_t nf, uint32_t FS, uint32_t G) {
    __shared__ float s[RW][64];
    const Task t = tasks[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t f = blockIdx.y * 64 + lane;
    float acc = 0.0f;
    if (f < nf) {
        for (uint32_t j = w; j < t.count; j += RW) {
            const float p = (j == 0 && t.rslot != NONE) ? rsrc[(size_t)t.rslot * FS + f] : src[(size_t)(t.src0 + j) * FS + f];
            acc = j == w ? p : acc + p;
        }
    }
    s[w][lane] = acc;
    __syncthreads();
    if (w != 0 || f >= nf) return;
    float tot = s[0][lane];
    if (t.count == 2) tot = tot + s[1][lane];
    else if (t.count == 3) tot = (tot + s[1][lane]) + s[2][lane];
    else if (t.count > 3) tot = (tot + s[1][lane]) + (s[2][lane] + s[3][lane]);
    if (t.final) bus[(size_t)f * G + t.dst] = __fdiv_rn(tot, t.div);
    else next[(size_t)t.dst * FS + f] = tot;
}

// ---- per-channel returns ---------------------------------------------------------------------------------------------------
constexpr int RCHUNK = 16;                         // frames per wave of the returns kernel
constexpr int RBATCH = 8;                          // ... of which so many are loaded before the first is written

struct RetArgs {
    const float *x;              // may be `out`: no __restrict__
    float *out;
    const float *gain;           // [N]
    const float *S;              // [nf][G] raw sums
    const uint32_t *gstart;      // [G + 1]
    const float *rdiv;           // [G]: link_divisor(n_g - 1) (1.0 without normalise); 0.0 marks a group of one channel
    const uint32_t *sfirst;      // [nspans + 1]: the group of the span's first channel; [nspans] = G - 1
    const uint8_t *slow;         // [nspans]
    uint32_t N, Wrow, nf, G, nspans, nchunks, norm;
};

// fl32(fl32(S - t) / div); div == 0 marks a group of one: no other pipe, +0.0 whatever the sample is
__device__ __forceinline__ float mix_minus(float S, float x, float g, float div, bool gain, bool norm) {
    const float t = gain ? __fmul_rn(x, g) : x;
    const float d = __fsub_rn(S, t);
    const float q = norm ? __fdiv_rn(d, div) : d;
    return div == 0.0f ? 0.0f : q;
}

template <bool GAIN, bool VEC, bool CUT>
__device__ __forceinline__ void returns_span(const RetArgs &a, uint32_t k, uint32_t f0, uint32_t lane) {
    const uint32_t ch = k * SPAN + 4 * lane;
    if (ch >= a.N) return;
    uint32_t gi[4];
    float dv[4], gn[4];
    bool valid[4];
    size_t b[4];
    uint32_t lo = a.sfirst[k];
    const uint32_t hi = a.sfirst[k + 1];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t c = ch + i;
        valid[i] = c < a.N;
        if (CUT && valid[i]) {
            // the first m in (lo, hi + 1] with gstart[m] > c: gstart[lo] <= c, and gstart[hi + 1] is past this span
            uint32_t i0 = lo + 1, i1 = hi + 1;
            while (i0 < i1) {
                const uint32_t m = (i0 + i1) / 2;
                if (a.gstart[m] > c) i1 = m;
                else i0 = m + 1;
            }
            lo = i0 - 1;
        }
        gi[i] = lo;
        dv[i] = a.rdiv[lo];
        gn[i] = (GAIN && valid[i]) ? a.gain[c] : 1.0f;
        b[i] = (valid[i] && (i == 0 || !VEC)) ? chan_base(c, a.Wrow, a.nf) : 0;
    }
    const bool norm = a.norm != 0;
#pragma unroll
    for (int i0 = 0; i0 < RCHUNK; i0 += RBATCH) {
        float4 v[RBATCH], s[RBATCH];
#pragma unroll
        for (int j = 0; j < RBATCH; ++j) {
            const uint32_t f = f0 + i0 + j;
            v[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            s[j] = v[j];
            if (f < a.nf) {
                const size_t o = (size_t)f * a.Wrow;
                if (VEC) {
                    v[j] = *(const float4 *)(a.x + b[0] + o);
                } else {
                    v[j].x = a.x[b[0] + o];
                    if (valid[1]) v[j].y = a.x[b[1] + o];
                    if (valid[2]) v[j].z = a.x[b[2] + o];
                    if (valid[3]) v[j].w = a.x[b[3] + o];
                }
                const float *row = a.S + (size_t)f * a.G;
                s[j].x = row[gi[0]];
                if (CUT) {
                    s[j].y = row[gi[1]];
                    s[j].z = row[gi[2]];
                    s[j].w = row[gi[3]];
                } else {
                    s[j].y = s[j].z = s[j].w = s[j].x;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < RBATCH; ++j) {
            const uint32_t f = f0 + i0 + j;
            if (f >= a.nf) continue;
            const size_t o = (size_t)f * a.Wrow;
            float4 r;
            r.x = mix_minus(s[j].x, v[j].x, gn[0], dv[0], GAIN, norm);
            r.y = mix_minus(s[j].y, v[j].y, gn[1], dv[1], GAIN, norm);
            r.z = mix_minus(s[j].z, v[j].z, gn[2], dv[2], GAIN, norm);
            r.w = mix_minus(s[j].w, v[j].w, gn[3], dv[3], GAIN, norm);
            if (VEC) {
                *(float4 *)(a.out + b[0] + o) = r;
            } else {
                a.out[b[0] + o] = r.x;
                if (valid[1]) a.out[b[1] + o] = r.y;
                if (valid[2]) a.out[b[2] + o] = r.z;
                if (valid[3]) a.out[b[3] + o] = r.w;
            }
        }
    }
}

template <bool GAIN, bool VEC>
__global__ __launch_bounds__(P1_WG) void mixgroups_returns(RetArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t item = blockIdx.x * (P1_WG / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= a.nspans * a.nchunks) return;
    const uint32_t k = item / a.nchunks, f0 = (item - k * a.nchunks) * RCHUNK;
    if (a.slow[k]) returns_span<GAIN, VEC, true>(a, k, f0, lane);
    else returns_span<GAIN, VEC, false>(a, k, f0, lane);
}

// buses[f][g] = S[f][g] / gdiv[g]: what the last reduce level (or a cut span) of `run` writes, from the raw sums
__global__ __launch_bounds__(256) void mixgroups_divide(const float *__restrict__ S, const float *__restrict__ gdiv,
                                                        float *__restrict__ bus, uint32_t G, uint64_t total) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) bus[i] = __fdiv_rn(S[i], gdiv[i % G]);
}

// ---- the plan: pure host -------------------------------------------------------------------------------------------------
thread_local std::string g_err;        // the reason of the last failed call that had no bank to keep it

uint32_t ceil_log2(uint64_t n) {
    uint32_t b = 0;
    while (((uint64_t)1 << b) < n) ++b;
    return b;
}

// additions one behind the other in one reduce workgroup over `cnt` pieces
uint32_t reduce_depth(uint64_t cnt) { return (uint32_t)((cnt + RW - 1) / RW - (cnt ? 1 : 0)) + (cnt >= 3 ? 2u : cnt == 2 ? 1u : 0u); }

// ... and in the sum of channels [lo, hi) of ONE span that has a boundary inside
uint32_t cut_depth(uint64_t lo, uint64_t hi) { return ceil_log2(std::min<uint64_t>(hi - lo, SUB)) + (uint32_t)((hi - 1) / SUB - lo / SUB); }

struct GroupPieces {
    uint64_t m = 0;              // pieces the reduce levels add (0: the partials kernel writes the bus itself, or the group is empty)
    uint64_t lfirst = 0;         // the first L row
    bool has_r = false;          // piece 0 is R[k0]
    uint64_t k0 = 0;
    uint32_t depth = 0;          // of the deepest piece
};

GroupPieces pieces_of(uint64_t s, uint64_t e) {
    GroupPieces p;
    if (e == s) return p;
    const uint64_t k0 = s / SPAN, k1 = (e - 1) / SPAN;
    p.k0 = k0;
    if (k0 == k1) {
        if (s % SPAN == 0 && e == (k0 + 1) * SPAN) {
            p.m = 1;
            p.lfirst = k0;
            p.depth = 8;
        } else {
            p.depth = cut_depth(s, e);
        }
        return p;
    }
    p.has_r = s % SPAN != 0;
    p.m = k1 - k0 + 1;
    p.lfirst = p.has_r ? k0 + 1 : k0;
    const bool cut_end = e % SPAN != 0;
    const uint64_t whole = p.m - (p.has_r ? 1 : 0) - (cut_end ? 1 : 0);
    if (whole) p.depth = 8;
    if (p.has_r) p.depth = std::max(p.depth, cut_depth(s, (k0 + 1) * SPAN));
    if (cut_end) p.depth = std::max(p.depth, cut_depth(k1 * SPAN, e));
    return p;
}

uint32_t depth_of(const GroupPieces &p) {
    uint32_t d = p.depth;
    for (uint64_t m = p.m; m > 1; m = (m + FAN - 1) / FAN) {
        d += reduce_depth(std::min<uint64_t>(m, FAN));
        if (m <= FAN) break;
    }
    return d;
}

int check_table(const uint64_t *gs, uint32_t G, uint64_t N, uint32_t W, std::string &err) {
    char buf[160];
    if (!gs || G == 0) {
        err = "mixgroups: no group table";
        return DSPFX_ERR_INVALID;
    }
    if (N == 0 || N > 0xFFFFFF00ull) {
        err = "mixgroups: n_channels must be 1 .. 2^32 - 256";
        return DSPFX_ERR_INVALID;
    }
    if (W && (!pow2(W) || N % W)) {
        std::snprintf(buf, sizeof buf, "mixgroups: tile_channels %u is not a power of two that divides n_channels %llu", W, (unsigned long long)N);
        err = buf;
        return DSPFX_ERR_INVALID;
    }
    if (gs[0] != 0) {
        std::snprintf(buf, sizeof buf, "mixgroups: group_start[0] is %llu, not 0", (unsigned long long)gs[0]);
        err = buf;
        return DSPFX_ERR_INVALID;
    }
    for (uint32_t g = 0; g < G; ++g)
        if (gs[g + 1] < gs[g]) {
            std::snprintf(buf, sizeof buf, "mixgroups: group_start decreases at entry %u (%llu after %llu)", g + 1,
                          (unsigned long long)gs[g + 1], (unsigned long long)gs[g]);
            err = buf;
            return DSPFX_ERR_INVALID;
        }
    if (gs[G] != N) {
        std::snprintf(buf, sizeof buf, "mixgroups: group_start[%u] is %llu, not n_channels %llu", G, (unsigned long long)gs[G], (unsigned long long)N);
        err = buf;
        return DSPFX_ERR_INVALID;
    }
    return DSPFX_OK;
}

struct Level {
    std::vector<Task> tasks;
    uint32_t rows = 0;           // rows of partial sums it leaves for the next level
    Task *dtasks = nullptr;
    Task *dtasks_raw = nullptr;  // the same tasks with div = 1.0 (returns; made at the first returns call of a normalising bank)
    float *out = nullptr;
};

struct Store {
    float *vals = nullptr;       // page-locked; nullptr: back to 1.0 ("no multiply")
    size_t cap = 0;
    uint64_t first = 0, count = 0;
    hipEvent_t ev = nullptr;
};

}  // namespace

struct dspfx_mixgroups {
    dspfx_mixgroups_desc desc{};
    std::mutex mu;                               // run / destroy
    std::mutex qmu;                              // the store queue and the free staging buffers
    std::deque<Store> queue;                     // stores not yet handed to a stream
    std::vector<Store> spare;                    // staging buffers free for the next store
    std::vector<Store> flying;                   // copies queued on a stream (mu)
    std::vector<hipEvent_t> events;              // spare events (mu)
    std::vector<uint8_t> faded;                  // per channel: a fader value is stored (mu)
    uint64_t n_faded = 0;
    uint32_t nspans = 0, FS = 0;
    float *gain = nullptr, *L = nullptr, *R = nullptr, *gdiv = nullptr;
    uint32_t *gstart = nullptr;
    uint8_t *slow = nullptr;
    std::vector<Level> levels;
    std::vector<uint32_t> hstart;                // the table, host copy (for the returns tables)
    // per-channel returns: made at the first dspfx_mixgroups_returns call (mu)
    bool ret_ready = false;
    float *S = nullptr;                          // [max_frames][G] raw sums
    float *gdiv_raw = nullptr;                   // [G] of 1.0 (a bank with normalise = 0 uses gdiv itself)
    float *rdiv = nullptr;                       // [G]
    uint32_t *sfirst = nullptr;                  // [nspans + 1]
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;
    bool used = false;
    std::string err;
};

namespace {

void release(dspfx_mixgroups *p) {
    (void)hipSetDevice(p->desc.device);
    for (void *d : {(void *)p->gain, (void *)p->L, (void *)p->R, (void *)p->gdiv, (void *)p->gstart, (void *)p->slow, (void *)p->S,
                    (void *)p->gdiv_raw, (void *)p->rdiv, (void *)p->sfirst})
        if (d) (void)hipFree(d);
    for (Level &l : p->levels) {
        if (l.dtasks) (void)hipFree(l.dtasks);
        if (l.dtasks_raw) (void)hipFree(l.dtasks_raw);
        if (l.out) (void)hipFree(l.out);
    }
    for (Store &s : p->queue)
        if (s.vals) (void)hipHostFree(s.vals);
    for (Store &s : p->spare)
        if (s.vals) (void)hipHostFree(s.vals);
    for (Store &s : p->flying) {
        if (s.vals) (void)hipHostFree(s.vals);
        if (s.ev) (void)hipEventDestroy(s.ev);
    }
    for (hipEvent_t e : p->events) (void)hipEventDestroy(e);
    if (p->ev) (void)hipEventDestroy(p->ev);
    delete p;
}

int fail(dspfx_mixgroups *p, int rc, const char *what) {
    p->err = what;
    return rc;
}

// the stores made so far, in order, onto the stream ahead of the run; staging buffers whose copy is done go back
hipError_t apply_stores(dspfx_mixgroups *p, hipStream_t s) {
    std::vector<Store> done;
    for (size_t i = 0; i < p->flying.size();) {
        if (hipEventQuery(p->flying[i].ev) == hipSuccess) {
            p->events.push_back(p->flying[i].ev);
            p->flying[i].ev = nullptr;
            done.push_back(p->flying[i]);
            p->flying[i] = p->flying.back();
            p->flying.pop_back();
        } else {
            (void)hipGetLastError();
            ++i;
        }
    }
    std::deque<Store> q;
    {
        std::lock_guard<std::mutex> lk(p->qmu);
        for (Store &d : done) p->spare.push_back(d);
        q.swap(p->queue);
    }
    hipError_t err = hipSuccess;
    while (!q.empty()) {
        Store st = q.front();
        q.pop_front();
        if (err != hipSuccess) {                 // a failed call drops the stores behind it; their buffers are still freed
            if (st.vals) (void)hipHostFree(st.vals);
            continue;
        }
        uint8_t *fl = p->faded.data() + st.first;
        const uint8_t to = st.vals ? 1 : 0;
        for (uint64_t i = 0; i < st.count; ++i) {
            p->n_faded += (uint64_t)to - fl[i];
            fl[i] = to;
        }
        if (!st.vals) {
            err = hipMemsetD32Async((hipDeviceptr_t)(p->gain + st.first), 0x3F800000, st.count, s);
            continue;
        }
        err = hipMemcpyAsync(p->gain + st.first, st.vals, st.count * sizeof(float), hipMemcpyHostToDevice, s);
        if (err == hipSuccess) {
            if (p->events.empty()) {
                err = hipEventCreateWithFlags(&st.ev, hipEventDisableTiming);
            } else {
                st.ev = p->events.back();
                p->events.pop_back();
            }
        }
        if (err == hipSuccess) err = hipEventRecord(st.ev, s);
        p->flying.push_back(st);                 // (with or without an event: destroy frees it after the device is idle)
    }
    return err;
}

template <int F>
hipError_t launch_partials(const P1Args &a, bool gain, bool vec, hipStream_t s) {
    const uint32_t items = a.nspans * a.nchunks, blocks = (items + P1_WG / 64 - 1) / (P1_WG / 64);
    if (gain) {
        if (vec) mixgroups_partials<F, true, true><<<blocks, P1_WG, 0, s>>>(a);
        else mixgroups_partials<F, true, false><<<blocks, P1_WG, 0, s>>>(a);
    } else {
        if (vec) mixgroups_partials<F, false, true><<<blocks, P1_WG, 0, s>>>(a);
        else mixgroups_partials<F, false, false><<<blocks, P1_WG, 0, s>>>(a);
    }
    return hipGetLastError();
}

}  // namespace

// (not BANK_HIP: this bank keeps the reason of a failure for dspfx_mixgroups_last_error)
#define MG_HIP(call, what)                                         \
    do {                                                           \
        if ((call) != hipSuccess) return fail(p, DSPFX_ERR_HIP, what); \
    } while (0)

extern "C" const char *dspfx_mixgroups_last_error(const dspfx_mixgroups *p) { return p ? p->err.c_str() : g_err.c_str(); }

extern "C" int dspfx_mixgroups_plan(const uint64_t *group_start, uint32_t n_groups, uint64_t n_channels, uint32_t tile_channels,
                                    uint32_t *depth_out) {
    g_err.clear();
    const int rc = check_table(group_start, n_groups, n_channels, tile_channels, g_err);
    if (rc != DSPFX_OK) return rc;
    if (depth_out)
        for (uint32_t g = 0; g < n_groups; ++g) depth_out[g] = depth_of(pieces_of(group_start[g], group_start[g + 1]));
    return DSPFX_OK;
}

extern "C" int dspfx_mixgroups_create(const dspfx_mixgroups_desc *desc, dspfx_mixgroups **out) {
    if (!desc || !out) {
        g_err = "mixgroups: null argument";
        return DSPFX_ERR_INVALID;
    }
    *out = nullptr;
    g_err.clear();
    if (desc->abi_version != DSPFX_ABI_VERSION || desc->max_frames == 0 || desc->max_frames > (1u << 20)) {
        g_err = "mixgroups: abi_version or max_frames";
        return DSPFX_ERR_INVALID;
    }
    int rc = check_table(desc->group_start, desc->n_groups, desc->n_channels, desc->tile_channels, g_err);
    if (rc != DSPFX_OK) return rc;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return DSPFX_ERR_NO_DEVICE;
    if (desc->device < 0 || desc->device >= count) {
        g_err = "mixgroups: no such device";
        return DSPFX_ERR_INVALID;
    }
    if (hipSetDevice(desc->device) != hipSuccess) return DSPFX_ERR_HIP;
    dspfx_mixgroups *p = new (std::nothrow) dspfx_mixgroups;
    if (!p) return DSPFX_ERR_OOM;
    p->desc = *desc;
    p->desc.group_start = nullptr;               // copied below: the caller's table is not kept
    const uint32_t N = desc->n_channels, G = desc->n_groups;
    const uint64_t *gs = desc->group_start;
    p->nspans = (N + SPAN - 1) / SPAN;
    p->FS = (desc->max_frames + 63u) / 64u * 64u;
    if ((uint64_t)p->nspans * (p->FS / CHUNK) >= (1ull << 31)) {      // one wave per span and chunk
        g_err = "mixgroups: n_channels x max_frames is too large";
        delete p;
        return DSPFX_ERR_INVALID;
    }
    p->faded.assign(N, 0);

    // the tables: group starts and divisors, the spans with a boundary inside, the reduce levels
    std::vector<uint32_t> gstart(G + 1);
    std::vector<float> gdiv(G, 1.0f);
    std::vector<uint8_t> slow(p->nspans, 0);
    struct Pending {
        uint32_t g, src0, m, rslot;
        float div;
    };
    std::vector<Pending> cur;
    uint64_t last_n = ~0ull;
    float last_div = 1.0f;
    for (uint32_t g = 0; g <= G; ++g) {
        gstart[g] = (uint32_t)gs[g];
        if (gs[g] % SPAN) slow[gs[g] / SPAN] = 1;        // a boundary strictly inside a span (N itself included)
    }
    for (uint32_t g = 0; g < G; ++g) {
        const uint64_t n = gs[g + 1] - gs[g];
        if (desc->normalise) {
            if (n != last_n) {
                last_n = n;
                last_div = dspfx_link_divisor(n);
            }
            gdiv[g] = last_div;
        }
        const GroupPieces pc = pieces_of(gs[g], gs[g + 1]);
        if (n == 0 || pc.m) cur.push_back({g, (uint32_t)(pc.has_r ? pc.lfirst - 1 : pc.lfirst), (uint32_t)pc.m,
                                           pc.has_r ? (uint32_t)pc.k0 : NONE, gdiv[g]});
    }
    while (!cur.empty()) {
        Level lv;
        std::vector<Pending> next;
        for (const Pending &q : cur) {
            if (q.m <= FAN) {
                lv.tasks.push_back({q.src0, q.m, q.rslot, q.g, q.div, 1u});
                continue;
            }
            const uint32_t nch = (q.m + FAN - 1) / FAN, base = lv.rows;
            for (uint32_t c = 0; c < nch; ++c)
                lv.tasks.push_back({q.src0 + c * FAN, std::min(FAN, q.m - c * FAN), c == 0 ? q.rslot : NONE, lv.rows++, 1.0f, 0u});
            next.push_back({q.g, base, nch, NONE, q.div});
        }
        p->levels.push_back(std::move(lv));
        cur.swap(next);
    }

    const size_t prow = (size_t)p->nspans * p->FS * sizeof(float);
    bool ok = hipMalloc((void **)&p->gain, (size_t)N * sizeof(float)) == hipSuccess && hipMalloc((void **)&p->L, prow) == hipSuccess &&
              hipMalloc((void **)&p->R, prow) == hipSuccess && hipMalloc((void **)&p->gdiv, (size_t)G * sizeof(float)) == hipSuccess &&
              hipMalloc((void **)&p->gstart, (size_t)(G + 1) * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc((void **)&p->slow, p->nspans) == hipSuccess;
    for (Level &l : p->levels) {
        ok = ok && hipMalloc((void **)&l.dtasks, l.tasks.size() * sizeof(Task)) == hipSuccess;
        if (l.rows) ok = ok && hipMalloc((void **)&l.out, (size_t)l.rows * p->FS * sizeof(float)) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        release(p);
        return DSPFX_ERR_OOM;
    }
    ok = hipMemsetD32((hipDeviceptr_t)p->gain, 0x3F800000, N) == hipSuccess &&
         hipMemcpy(p->gdiv, gdiv.data(), (size_t)G * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(p->gstart, gstart.data(), (size_t)(G + 1) * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(p->slow, slow.data(), p->nspans, hipMemcpyHostToDevice) == hipSuccess &&
         hipEventCreateWithFlags(&p->ev, hipEventDisableTiming) == hipSuccess;
    for (Level &l : p->levels)
        ok = ok && hipMemcpy(l.dtasks, l.tasks.data(), l.tasks.size() * sizeof(Task), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        release(p);
        return DSPFX_ERR_HIP;
    }
    p->hstart = std::move(gstart);
    *out = p;
    return DSPFX_OK;
}

extern "C" int dspfx_mixgroups_destroy(dspfx_mixgroups *p) {
    if (!p) return DSPFX_ERR_INVALID;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        (void)hipSetDevice(p->desc.device);
        if (p->used) (void)hipStreamSynchronize(p->last);    // the bank's work is ordered on the last stream it used
    }
    release(p);
    return DSPFX_OK;
}

extern "C" int dspfx_mixgroups_set_gains(dspfx_mixgroups *p, const float *host_values, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    if (first_channel > p->desc.n_channels || count > p->desc.n_channels - first_channel) return DSPFX_ERR_INVALID;
    if (count == 0) return DSPFX_OK;
    Store st;
    st.first = first_channel;
    st.count = count;
    if (host_values) {
        {
            std::lock_guard<std::mutex> lk(p->qmu);
            for (size_t i = 0; i < p->spare.size(); ++i)
                if (p->spare[i].cap >= count) {
                    st.vals = p->spare[i].vals;
                    st.cap = p->spare[i].cap;
                    p->spare[i] = p->spare.back();
                    p->spare.pop_back();
                    break;
                }
        }
        if (!st.vals) {
            if (hipSetDevice(p->desc.device) != hipSuccess) return DSPFX_ERR_HIP;
            if (hipHostMalloc((void **)&st.vals, count * sizeof(float), hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                return DSPFX_ERR_OOM;
            }
            st.cap = count;
        }
        std::memcpy(st.vals, host_values, count * sizeof(float));
    }
    std::lock_guard<std::mutex> lk(p->qmu);
    p->queue.push_back(st);
    return DSPFX_OK;
}

extern "C" int dspfx_mixgroups_run(dspfx_mixgroups *p, const float *block, uint32_t n_frames, float *buses, void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    if (!block || !buses || n_frames == 0 || n_frames > p->desc.max_frames) return fail(p, DSPFX_ERR_INVALID, "mixgroups run: block, buses or n_frames");
    hipStream_t s = (hipStream_t)stream;
    MG_HIP(hipSetDevice(p->desc.device), "hipSetDevice");
    MG_HIP(order(p, s), "stream order");
    MG_HIP(apply_stores(p, s), "fader store");
    P1Args a;
    a.x = block;
    a.gain = p->gain;
    a.L = p->L;
    a.R = p->R;
    a.bus = buses;
    a.gstart = p->gstart;
    a.gdiv = p->gdiv;
    a.slow = p->slow;
    a.N = p->desc.n_channels;
    a.Wrow = p->desc.tile_channels ? p->desc.tile_channels : a.N;
    a.nf = n_frames;
    a.G = p->desc.n_groups;
    a.FS = p->FS;
    a.nspans = p->nspans;
    const bool gain = p->n_faded != 0;
    const bool vec = a.Wrow % 4 == 0 && ((uintptr_t)block & 15u) == 0;
    a.nchunks = (n_frames + CHUNK - 1) / CHUNK;
    MG_HIP(launch_partials<CHUNK>(a, gain, vec, s), "mixgroups_partials");
    const float *src = p->L;
    for (Level &l : p->levels) {
        const dim3 grid((unsigned)l.tasks.size(), (n_frames + 63) / 64);
        mixgroups_reduce<<<grid, RW * 64, 0, s>>>(l.dtasks, src, p->R, l.out, buses, n_frames, p->FS, a.G);
        MG_HIP(hipGetLastError(), "mixgroups_reduce");
        src = l.out;
    }
    return DSPFX_OK;
}

namespace {

// The returns' buffers and tables, at the first call that asks for returns: a bank that never does keeps its footprint.
int prepare_returns(dspfx_mixgroups *p) {
    if (p->ret_ready) return DSPFX_OK;
    const uint32_t G = p->desc.n_groups, N = p->desc.n_channels;
    const std::vector<uint32_t> &gs = p->hstart;
    std::vector<float> rdiv(G, 1.0f);
    uint64_t last_n = ~0ull;
    float last_div = 1.0f;
    for (uint32_t g = 0; g < G; ++g) {
        const uint64_t n = gs[g + 1] - gs[g];
        if (n == 1) {
            rdiv[g] = 0.0f;                      // no other pipe: the kernel writes +0.0
        } else if (p->desc.normalise && n >= 2) {
            if (n != last_n) {
                last_n = n;
                last_div = dspfx_link_divisor(n - 1);
            }
            rdiv[g] = last_div;
        }
    }
    std::vector<uint32_t> sfirst(p->nspans + 1, G - 1);
    uint32_t g = 0;
    for (uint32_t k = 0; k < p->nspans; ++k) {
        while (gs[g + 1] <= (uint64_t)k * SPAN) ++g;     // gs[G] = N > k * SPAN
        sfirst[k] = g;
    }
    const bool raw = p->desc.normalise != 0;
    bool ok = hipMalloc((void **)&p->S, (size_t)p->desc.max_frames * G * sizeof(float)) == hipSuccess &&
              hipMalloc((void **)&p->rdiv, (size_t)G * sizeof(float)) == hipSuccess &&
              hipMalloc((void **)&p->sfirst, sfirst.size() * sizeof(uint32_t)) == hipSuccess;
    if (raw) {
        ok = ok && hipMalloc((void **)&p->gdiv_raw, (size_t)G * sizeof(float)) == hipSuccess;
        for (Level &l : p->levels) ok = ok && hipMalloc((void **)&l.dtasks_raw, l.tasks.size() * sizeof(Task)) == hipSuccess;
    }
    int rc = DSPFX_OK;
    if (!ok) {
        (void)hipGetLastError();
        rc = fail(p, DSPFX_ERR_OOM, "mixgroups returns: no device memory for the raw sums [max_frames][G] and the returns tables");
    } else {
        ok = hipMemcpy(p->rdiv, rdiv.data(), (size_t)G * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(p->sfirst, sfirst.data(), sfirst.size() * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
        if (raw) {
            ok = ok && hipMemsetD32((hipDeviceptr_t)p->gdiv_raw, 0x3F800000, G) == hipSuccess;
            for (Level &l : p->levels) {
                std::vector<Task> t = l.tasks;
                for (Task &q : t) q.div = 1.0f;
                ok = ok && hipMemcpy(l.dtasks_raw, t.data(), t.size() * sizeof(Task), hipMemcpyHostToDevice) == hipSuccess;
            }
        }
        if (!ok) rc = fail(p, DSPFX_ERR_HIP, "mixgroups returns: copying the returns tables");
    }
    if (rc != DSPFX_OK) {                        // all or nothing: the next call tries again
        for (void **d : {(void **)&p->S, (void **)&p->rdiv, (void **)&p->sfirst, (void **)&p->gdiv_raw})
            if (*d) {
                (void)hipFree(*d);
                *d = nullptr;
            }
        for (Level &l : p->levels)
            if (l.dtasks_raw) {
                (void)hipFree(l.dtasks_raw);
                l.dtasks_raw = nullptr;
            }
        return rc;
    }
    p->ret_ready = true;
    return DSPFX_OK;
}

hipError_t launch_returns(const RetArgs &a, bool gain, bool vec, hipStream_t s) {
    const uint32_t items = a.nspans * a.nchunks, blocks = (items + P1_WG / 64 - 1) / (P1_WG / 64);
    if (gain) {
        if (vec) mixgroups_returns<true, true><<<blocks, P1_WG, 0, s>>>(a);
        else mixgroups_returns<true, false><<<blocks, P1_WG, 0, s>>>(a);
    } else {
        if (vec) mixgroups_returns<false, true><<<blocks, P1_WG, 0, s>>>(a);
        else mixgroups_returns<false, false><<<blocks, P1_WG, 0, s>>>(a);
    }
    return hipGetLastError();
}

}  // namespace

extern "C" int dspfx_mixgroups_returns(dspfx_mixgroups *p, const float *block, uint32_t n_frames, float *buses, float *returns,
                                       void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    if (!block || !returns || n_frames == 0 || n_frames > p->desc.max_frames)
        return fail(p, DSPFX_ERR_INVALID, "mixgroups returns: block, returns or n_frames");
    hipStream_t s = (hipStream_t)stream;
    MG_HIP(hipSetDevice(p->desc.device), "hipSetDevice");
    const int rc = prepare_returns(p);
    if (rc != DSPFX_OK) return rc;
    MG_HIP(order(p, s), "stream order");
    MG_HIP(apply_stores(p, s), "fader store");       // once: the sums and the subtraction see the same table
    const bool raw = p->desc.normalise != 0;
    P1Args a;
    a.x = block;
    a.gain = p->gain;
    a.L = p->L;
    a.R = p->R;
    a.bus = p->S;
    a.gstart = p->gstart;
    a.gdiv = raw ? p->gdiv_raw : p->gdiv;
    a.slow = p->slow;
    a.N = p->desc.n_channels;
    a.Wrow = p->desc.tile_channels ? p->desc.tile_channels : a.N;
    a.nf = n_frames;
    a.G = p->desc.n_groups;
    a.FS = p->FS;
    a.nspans = p->nspans;
    const bool gain = p->n_faded != 0;
    a.nchunks = (n_frames + CHUNK - 1) / CHUNK;
    MG_HIP(launch_partials<CHUNK>(a, gain, a.Wrow % 4 == 0 && ((uintptr_t)block & 15u) == 0, s), "mixgroups_partials");
    const float *src = p->L;
    for (Level &l : p->levels) {
        const dim3 grid((unsigned)l.tasks.size(), (n_frames + 63) / 64);
        mixgroups_reduce<<<grid, RW * 64, 0, s>>>(raw ? l.dtasks_raw : l.dtasks, src, p->R, l.out, p->S, n_frames, p->FS, a.G);
        MG_HIP(hipGetLastError(), "mixgroups_reduce");
        src = l.out;
    }
    if (buses) {
        const uint64_t total = (uint64_t)n_frames * a.G;
        mixgroups_divide<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(p->S, p->gdiv, buses, a.G, total);
        MG_HIP(hipGetLastError(), "mixgroups_divide");
    }
    RetArgs r;
    r.x = block;
    r.out = returns;
    r.gain = p->gain;
    r.S = p->S;
    r.gstart = p->gstart;
    r.rdiv = p->rdiv;
    r.sfirst = p->sfirst;
    r.slow = p->slow;
    r.N = a.N;
    r.Wrow = a.Wrow;
    r.nf = n_frames;
    r.G = a.G;
    r.nspans = p->nspans;
    r.nchunks = (n_frames + RCHUNK - 1) / RCHUNK;
    r.norm = raw ? 1u : 0u;
    const bool vec = a.Wrow % 4 == 0 && (((uintptr_t)block | (uintptr_t)returns) & 15u) == 0;
    MG_HIP(launch_returns(r, gain, vec, s), "mixgroups_returns");
    return DSPFX_OK;
}
