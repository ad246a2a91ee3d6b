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
// The sign of a zero bus: the reference's collect_and_average starts from +0.0 and adds pipe by pipe, so terms that are all -0.0
// (silence through a negative fader) give +0.0, where a tree gives (-0) + (-0) = -0.  Wherever a finished sum becomes a bus -- the
// last reduce level, and a group complete inside its span -- it is written as +0.0 + sum, before the division: that is the sum
// itself for every value but -0.0.  The raw sums that returns read go through the same two places.
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
//
// Fader stores (dspfx_mixgroups_set_gains) go through the staged-store queue (store_queue.hip.h): staged in page-locked memory, queued,
// and put on the next run's stream ahead of its kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/dspfx.h"
#include "bank_common.hip.h"
#include "store_queue.hip.h"
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

// (A: P1Args or MapArgs; the piece is row `row` of a.L: the span itself without a map)
template <int F, bool GAIN, bool VEC, class A>
__device__ __forceinline__ void whole_span(const A &a, uint32_t k, uint32_t row, uint32_t f0, uint32_t lane) {
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
    if (dspfx::mixbus_lane_writes<F>((int)lane) && f < a.nf) a.L[(size_t)row * a.FS + f] = r[0];
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
            if (direct[r]) a.bus[(size_t)f * a.G + gi[r]] = __fdiv_rn(__fadd_rn(0.0f, v), dv[r]);   // (+0.0 + sum: see the head)
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
    else whole_span<F, GAIN, VEC>(a, k, k, f0, lane);
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
    if (t.final) bus[(size_t)f * G + t.dst] = __fdiv_rn(__fadd_rn(0.0f, tot), t.div);    // (+0.0 + sum: see the head)
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

// the frames [f0, f0 + RCHUNK) of a lane's four channels; CUT: the four may be in different groups
template <bool GAIN, bool VEC, bool CUT>
__device__ __forceinline__ void returns_rows(const float *x, float *out, const float *S, uint32_t Wrow, uint32_t nf, uint32_t G,
                                             bool norm, uint32_t f0, const uint32_t (&gi)[4], const float (&dv)[4],
                                             const float (&gn)[4], const bool (&valid)[4], const size_t (&b)[4]) {
#pragma unroll
    for (int i0 = 0; i0 < RCHUNK; i0 += RBATCH) {
        float4 v[RBATCH], s[RBATCH];
#pragma unroll
        for (int j = 0; j < RBATCH; ++j) {
            const uint32_t f = f0 + i0 + j;
            v[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            s[j] = v[j];
            if (f < nf) {
                const size_t o = (size_t)f * Wrow;
                if (VEC) {
                    v[j] = *(const float4 *)(x + b[0] + o);
                } else {
                    v[j].x = x[b[0] + o];
                    if (valid[1]) v[j].y = x[b[1] + o];
                    if (valid[2]) v[j].z = x[b[2] + o];
                    if (valid[3]) v[j].w = x[b[3] + o];
                }
                const float *row = S + (size_t)f * G;
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
            if (f >= nf) continue;
            const size_t o = (size_t)f * Wrow;
            float4 r;
            r.x = mix_minus(s[j].x, v[j].x, gn[0], dv[0], GAIN, norm);
            r.y = mix_minus(s[j].y, v[j].y, gn[1], dv[1], GAIN, norm);
            r.z = mix_minus(s[j].z, v[j].z, gn[2], dv[2], GAIN, norm);
            r.w = mix_minus(s[j].w, v[j].w, gn[3], dv[3], GAIN, norm);
            if (VEC) {
                *(float4 *)(out + b[0] + o) = r;
            } else {
                out[b[0] + o] = r.x;
                if (valid[1]) out[b[1] + o] = r.y;
                if (valid[2]) out[b[2] + o] = r.z;
                if (valid[3]) out[b[3] + o] = r.w;
            }
        }
    }
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
    returns_rows<GAIN, VEC, CUT>(a.x, a.out, a.S, a.Wrow, a.nf, a.G, a.norm != 0, f0, gi, dv, gn, valid, b);
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

// ---- mapped mode: a room id per channel (dspfx_mixgroups_assign) ----------------------------------------------------------------
// A room's members may lie anywhere.  Per span the host sorts the channels by (room, channel): a room's members of the span
// become one SEGMENT of adjacent sorted positions, and every segment of a seated room has a piece row; one room's pieces are
// adjacent rows, in ascending span order, so the reduce kernel above adds them as it adds a range's.
//   partials  one wave per (span, chunk of 16 frames), the same single 16-byte load per lane and frame.
//             A span whose 256 channels all sit in one room: whole_span, unchanged, into the room's piece row.
//             Any other span: the terms go through LDS into sorted order (four frames at a time; a row of 256 is padded by one
//             word per 64 so that neither the scattered write of a near-identity order nor the read conflicts), lane l then
//             holds sorted positions 4 l .. 4 l + 3, and a Hillis-Steele scan with steps 1, 2, .. 128 runs over the 256
//             positions in which the element of rank r IN ITS OWN SEGMENT adds the element `step` below it when r >= step.
//             The last element of a segment of n members then holds their sum, put together by a tree that n alone decides:
//             where the segment lies in the span, and what lies around it, changes nothing.  Unseated channels (and the
//             channels past N of the last span) sort last as a segment of their own that is written nowhere: left out, not
//             multiplied by zero.
//   returns   the streaming pass above with the room of each of a lane's four channels from the map, S gathered per frame;
//             an unseated channel and a room of one carry the divisor 0.0, which writes +0.0.
constexpr uint32_t SKIP = 0xFFFFFFFEu;             // swhole: nobody of the span is seated
constexpr int MB = 4;                              // frames that go through LDS together
constexpr uint32_t MROW = SPAN + SPAN / 64;        // floats of one frame's row in LDS: position p at p + p / 64

struct MapArgs {
    const float *x;
    const float *gain;           // [N]
    float *L;                    // [pieces][FS]
    const uint8_t *pos;          // [nspans * SPAN]: the sorted position of a channel in its span
    const uint8_t *rank;         // [nspans * SPAN], by sorted position: the rank in its segment
    const uint32_t *slot;        // [nspans * SPAN], by sorted position: the piece row, at the last element of a seated room's segment; else NONE
    const uint32_t *swhole;      // [nspans]: the piece row of a span that one room holds wholly; SKIP; NONE: sorted and scanned
    uint32_t N, Wrow, nf, FS, nspans, nchunks;
};

// the wave's own LDS writes before its reads, and its reads before the next writes (one wave: the LDS takes them in order)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the value the lane below holds (DPP wave_shr:1, no LDS round trip); lane 0 gets 0.0
__device__ __forceinline__ float lane_below(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}

template <int F, bool GAIN, bool VEC>
__device__ __forceinline__ void mapped_span(const MapArgs &a, float *lds, uint32_t k, uint32_t f0, uint32_t lane) {
    const uint32_t c0 = k * SPAN, ch = c0 + 4 * lane;
    const uint32_t pp = *(const uint32_t *)(a.pos + ch);         // the tables are padded to whole spans
    const uint32_t rr = *(const uint32_t *)(a.rank + ch);
    const uint4 ss = *(const uint4 *)(a.slot + ch);
    const uint32_t sl[4] = {ss.x, ss.y, ss.z, ss.w};
    bool valid[4];
    size_t b[4];
    float gn[4];
    uint32_t ph[4], rk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t c = ch + i, p = (pp >> (8 * i)) & 255u;
        valid[i] = c < a.N;
        ph[i] = p + (p >> 6);
        gn[i] = (GAIN && valid[i]) ? a.gain[c] : 1.0f;
        b[i] = (valid[i] && (i == 0 || !VEC)) ? chan_base(c, a.Wrow, a.nf) : 0;
        rk[i] = (rr >> (8 * i)) & 255u;
    }
    const uint32_t rd = 4 * lane + (lane >> 4);                  // where sorted position 4 * lane lies in a row
#pragma unroll
    for (int i0 = 0; i0 < F; i0 += 8) {
        float4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t f = f0 + i0 + j;
            v[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (f < a.nf && valid[0]) {
                const size_t o = (size_t)f * a.Wrow;
                if (VEC) {
                    v[j] = *(const float4 *)(a.x + b[0] + o);
                } else {
                    v[j].x = a.x[b[0] + o];
                    if (valid[1]) v[j].y = a.x[b[1] + o];
                    if (valid[2]) v[j].z = a.x[b[2] + o];
                    if (valid[3]) v[j].w = a.x[b[3] + o];
                }
            }
        }
#pragma unroll
        for (int h = 0; h < 8; h += MB) {
            if (f0 + i0 + h >= a.nf) break;                      // wave-uniform
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                float4 t = v[h + m];
                if (GAIN) t = make_float4(__fmul_rn(t.x, gn[0]), __fmul_rn(t.y, gn[1]), __fmul_rn(t.z, gn[2]), __fmul_rn(t.w, gn[3]));
                float *row = lds + m * MROW;
                row[ph[0]] = t.x;
                row[ph[1]] = t.y;
                row[ph[2]] = t.z;
                row[ph[3]] = t.w;
            }
            wave_lds_sync();
            float s[MB][4];
#pragma unroll
            for (int m = 0; m < MB; ++m)
#pragma unroll
                for (int j = 0; j < 4; ++j) s[m][j] = lds[m * MROW + rd + j];
            wave_lds_sync();
            // sorted position 4 * lane + j is s[.][j]: steps 1 and 2 stay inside the lane but for the lane below's last elements,
            // a step of 4 k takes the same register k lanes below.  A position below `step` has a rank below it: no lane reads
            // past lane 0
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                float (&e)[4] = s[m];
                const float u3 = lane_below(e[3]);
                if (rk[3] >= 1u) e[3] = e[3] + e[2];
                if (rk[2] >= 1u) e[2] = e[2] + e[1];
                if (rk[1] >= 1u) e[1] = e[1] + e[0];
                if (rk[0] >= 1u) e[0] = e[0] + u3;
                const float w2 = lane_below(e[2]), w3 = lane_below(e[3]);
                if (rk[3] >= 2u) e[3] = e[3] + e[1];
                if (rk[2] >= 2u) e[2] = e[2] + e[0];
                if (rk[1] >= 2u) e[1] = e[1] + w3;
                if (rk[0] >= 2u) e[0] = e[0] + w2;
            }
#pragma unroll
            for (uint32_t k = 1; k < 64; k *= 2) {
                const int from = (int)((lane - k) & 63u);
#pragma unroll
                for (int m = 0; m < MB; ++m)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float u = k == 1 ? lane_below(s[m][j]) : __shfl(s[m][j], from, 64);
                        if (rk[j] >= 4 * k) s[m][j] = s[m][j] + u;
                    }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (sl[j] == NONE) continue;
                float *dst = a.L + (size_t)sl[j] * a.FS + f0 + i0 + h;
#pragma unroll
                for (int m = 0; m < MB; ++m)
                    if (f0 + i0 + h + m < a.nf) dst[m] = s[m][j];
            }
        }
    }
}

template <bool GAIN, bool VEC>
__global__ __launch_bounds__(P1_WG) void mixrooms_partials(MapArgs a) {
    __shared__ float lds[P1_WG / 64][MB * MROW];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t item = blockIdx.x * (P1_WG / 64) + wave;
    if (item >= a.nspans * a.nchunks) return;
    const uint32_t k = item / a.nchunks, f0 = (item - k * a.nchunks) * CHUNK;
    const uint32_t sw = a.swhole[k];
    if (sw == SKIP) return;
    if (sw != NONE) whole_span<CHUNK, GAIN, VEC>(a, k, sw, f0, lane);
    else mapped_span<CHUNK, GAIN, VEC>(a, lds[wave], k, f0, lane);
}

struct RetMapArgs {
    const float *x;              // may be `out`: no __restrict__
    float *out;
    const float *gain;           // [N]
    const float *S;              // [nf][G] raw sums
    const uint32_t *room;        // [nspans * SPAN]; NONE: unseated
    const float *rdiv;           // [G], as RetArgs::rdiv for the room's member count
    uint32_t N, Wrow, nf, G, nspans, nchunks, norm;
};

template <bool GAIN, bool VEC>
__global__ __launch_bounds__(P1_WG) void mixrooms_returns(RetMapArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t item = blockIdx.x * (P1_WG / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= a.nspans * a.nchunks) return;
    const uint32_t k = item / a.nchunks, f0 = (item - k * a.nchunks) * RCHUNK;
    const uint32_t ch = k * SPAN + 4 * lane;
    if (ch >= a.N) return;
    const uint4 rm = *(const uint4 *)(a.room + ch);
    const uint32_t r4[4] = {rm.x, rm.y, rm.z, rm.w};
    uint32_t gi[4];
    float dv[4], gn[4];
    bool valid[4];
    size_t b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t c = ch + i;
        valid[i] = c < a.N;
        const bool seated = r4[i] != NONE;
        gi[i] = seated ? r4[i] : 0u;                 // (a row of S always has room 0)
        dv[i] = seated ? a.rdiv[gi[i]] : 0.0f;
        gn[i] = (GAIN && valid[i]) ? a.gain[c] : 1.0f;
        b[i] = (valid[i] && (i == 0 || !VEC)) ? chan_base(c, a.Wrow, a.nf) : 0;
    }
    returns_rows<GAIN, VEC, true>(a.x, a.out, a.S, a.Wrow, a.nf, a.G, a.norm != 0, f0, gi, dv, gn, valid, b);
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

struct Level {
    std::vector<Task> tasks;
    uint32_t rows = 0;           // rows of partial sums it leaves for the next level
    Task *dtasks = nullptr;
    Task *dtasks_raw = nullptr;  // the same tasks with div = 1.0 (returns; made at the first returns call of a normalising bank)
    float *out = nullptr;
};

// a fader store's vals: [count]; none: back to 1.0 ("no multiply")
struct StoreFields {
    uint64_t first = 0, count = 0;
};
typedef StoreQueue<StoreFields> Stores;
typedef Stores::Store Store;

// ---- a seating (mapped mode): pure host ---------------------------------------------------------------------------------
struct RoomPlan {
    std::vector<uint64_t> count;         // [G] members
    std::vector<uint64_t> npieces;       // [G]
    std::vector<uint64_t> first;         // [G] the room's first piece row; its pieces follow in ascending span order
    std::vector<uint32_t> pdepth;        // [G] the deepest piece
    uint64_t pieces = 0;
    std::vector<uint8_t> pos, rank;      // MapArgs
    std::vector<uint32_t> slot, swhole, room;    // room: padded to whole spans with NONE
};

uint32_t room_depth(const RoomPlan &pl, uint32_t g) {
    GroupPieces gp;
    gp.m = pl.npieces[g];
    gp.depth = pl.pdepth[g];
    return depth_of(gp);
}

// room_of[N], every id < G or NONE (checked by the caller); tables: the kernels' tables too
void plan_rooms(const uint32_t *room_of, uint64_t N, uint32_t G, bool tables, RoomPlan &pl) {
    const uint64_t nspans = (N + SPAN - 1) / SPAN;
    pl.count.assign(G, 0);
    pl.npieces.assign(G, 0);
    pl.first.assign(G, 0);
    pl.pdepth.assign(G, 0);
    std::vector<uint8_t> ord((size_t)nspans * SPAN);             // the channel (of its span) at a sorted position
    std::vector<uint8_t> whole(nspans, 0);                       // 1: one room holds the span; 2: nobody is seated in it
    uint32_t key[SPAN];
    uint16_t idx[SPAN];
    for (uint64_t k = 0; k < nspans; ++k) {
        const uint64_t c0 = k * SPAN;
        bool sorted = true;
        for (uint32_t i = 0; i < SPAN; ++i) {
            key[i] = c0 + i < N ? room_of[c0 + i] : NONE;
            idx[i] = (uint16_t)i;
            if (i && key[i] < key[i - 1]) sorted = false;
        }
        if (!sorted) std::stable_sort(idx, idx + SPAN, [&](uint16_t x, uint16_t y) { return key[x] < key[y]; });
        uint8_t *o = ord.data() + c0;
        for (uint32_t i = 0; i < SPAN; ++i) o[i] = (uint8_t)idx[i];
        if (key[idx[0]] == NONE) whole[k] = 2;
        else if (key[idx[0]] == key[idx[SPAN - 1]]) whole[k] = 1;    // 256 members: the span is full
        for (uint32_t i = 0; i < SPAN;) {                        // the segments
            const uint32_t g = key[idx[i]];
            uint32_t e = i + 1;
            while (e < SPAN && key[idx[e]] == g) ++e;
            if (g != NONE) {
                pl.count[g] += e - i;
                pl.npieces[g] += 1;
                pl.pdepth[g] = std::max(pl.pdepth[g], whole[k] == 1 ? 8u : ceil_log2(e - i));
            }
            i = e;
        }
    }
    pl.pieces = 0;
    for (uint32_t g = 0; g < G; ++g) {
        pl.first[g] = pl.pieces;
        pl.pieces += pl.npieces[g];
    }
    if (!tables) return;
    pl.pos.assign((size_t)nspans * SPAN, 0);
    pl.rank.assign((size_t)nspans * SPAN, 0);
    pl.slot.assign((size_t)nspans * SPAN, NONE);
    pl.swhole.assign(nspans, NONE);
    pl.room.assign((size_t)nspans * SPAN, NONE);
    std::copy(room_of, room_of + N, pl.room.begin());
    std::vector<uint64_t> next = pl.first;
    for (uint64_t k = 0; k < nspans; ++k) {
        const uint64_t c0 = k * SPAN;
        const uint8_t *o = ord.data() + c0;
        if (whole[k] == 2) pl.swhole[k] = SKIP;
        for (uint32_t i = 0; i < SPAN;) {
            const uint32_t g = pl.room[c0 + o[i]];
            uint32_t e = i;
            for (; e < SPAN && pl.room[c0 + o[e]] == g; ++e) {
                pl.pos[c0 + o[e]] = (uint8_t)e;
                pl.rank[c0 + e] = (uint8_t)(e - i);
            }
            if (g != NONE) {
                const uint32_t row = (uint32_t)next[g]++;
                pl.slot[c0 + e - 1] = row;
                if (whole[k] == 1) pl.swhole[k] = row;
            }
            i = e;
        }
    }
}

int check_rooms(const uint32_t *room_of, uint64_t first, uint64_t count, uint32_t G, std::string &err) {
    char buf[160];
    for (uint64_t i = 0; i < count; ++i)
        if (room_of[i] >= G && room_of[i] != NONE) {
            std::snprintf(buf, sizeof buf, "mixgroups: channel %llu is given room %u, and there are %u rooms (or DSPFX_MIXGROUPS_NO_ROOM)",
                          (unsigned long long)(first + i), room_of[i], G);
            err = buf;
            return DSPFX_ERR_INVALID;
        }
    return DSPFX_OK;
}

struct Seating {
    std::vector<uint32_t> room;          // [N], host
    uint64_t pieces = 0;
    uint8_t *pos = nullptr, *rank = nullptr;
    uint32_t *slot = nullptr, *swhole = nullptr, *droom = nullptr;
    float *gdiv = nullptr, *rdiv = nullptr;      // [G]
    float *P = nullptr;                  // [pieces][FS]
    std::vector<Level> levels;           // (dtasks_raw with the seating, in a normalising bank)
    hipEvent_t ev = nullptr;             // of a retired seating: behind the last run that was given it
};

void free_seating(Seating *t) {
    if (!t) return;
    for (void *d : {(void *)t->pos, (void *)t->rank, (void *)t->slot, (void *)t->swhole, (void *)t->droom, (void *)t->gdiv,
                    (void *)t->rdiv, (void *)t->P})
        if (d) (void)hipFree(d);
    for (Level &l : t->levels) {
        if (l.dtasks) (void)hipFree(l.dtasks);
        if (l.dtasks_raw) (void)hipFree(l.dtasks_raw);
        if (l.out) (void)hipFree(l.out);
    }
    if (t->ev) (void)hipEventDestroy(t->ev);
    delete t;
}

struct Pending {
    uint32_t g, src0, m, rslot;
    float div;
};

// the reduce levels over every group's pieces: up to FAN pieces a task, further levels over the tasks' results
std::vector<Level> build_levels(std::vector<Pending> cur) {
    std::vector<Level> levels;
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
        levels.push_back(std::move(lv));
        cur.swap(next);
    }
    return levels;
}
}  // namespace

struct dspfx_mixgroups : BankError {
    dspfx_mixgroups_desc desc{};
    std::mutex mu;                               // run / destroy
    Stores stores;                               // the fader stores (store_queue.hip.h)
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
    // mapped mode (dspfx_mixgroups_assign): nullptr until the first assign
    std::mutex amu;                              // one assign at a time; taken before mu
    Seating *seat = nullptr;                     // written under amu and mu
    std::vector<Seating *> retired;              // replaced seatings that a run in flight may still read (mu)
    hipStream_t astream = nullptr;               // the table copies of an assign (amu)
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;
    bool used = false;
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
    p->stores.free_all();
    if (p->ev) (void)hipEventDestroy(p->ev);
    free_seating(p->seat);
    for (Seating *t : p->retired) free_seating(t);
    if (p->astream) (void)hipStreamDestroy(p->astream);
    delete p;
}

// one fader store onto the stream, and into the count of faded channels (mu)
hipError_t apply_store(dspfx_mixgroups *p, const Store &st, hipStream_t s) {
    uint8_t *fl = p->faded.data() + st.first;
    const uint8_t to = st.vals ? 1 : 0;
    for (uint64_t i = 0; i < st.count; ++i) {
        p->n_faded += (uint64_t)to - fl[i];
        fl[i] = to;
    }
    if (!st.vals) return hipMemsetD32Async((hipDeviceptr_t)(p->gain + st.first), 0x3F800000, st.count, s);
    return hipMemcpyAsync(p->gain + st.first, st.vals, st.count * sizeof(float), hipMemcpyHostToDevice, s);
}

// the stores made so far, in order, onto the stream ahead of the run
hipError_t apply_stores(dspfx_mixgroups *p, hipStream_t s) {
    return p->stores.drain(s, [p](const Store &st, hipStream_t on) { return apply_store(p, st, on); });
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

extern "C" const char *dspfx_mixgroups_last_error(const dspfx_mixgroups *p) { return p ? p->err.c_str() : g_err.c_str(); }

extern "C" int dspfx_mixgroups_plan(const uint64_t *group_start, uint32_t n_groups, uint64_t n_channels, uint32_t tile_channels,
                                    uint32_t *depth_out) {
    g_err.clear();
    const int rc = check_table("mixgroups", group_start, n_groups, n_channels, tile_channels, 0, g_err);
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
    int rc = check_table("mixgroups", desc->group_start, desc->n_groups, desc->n_channels, desc->tile_channels, 0, g_err);
    if (rc != DSPFX_OK) return rc;
    rc = open_device("mixgroups", desc->device, &g_err);
    if (rc != DSPFX_OK) return rc;
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
    p->levels = build_levels(std::move(cur));

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

extern "C" int dspfx_mixgroups_destroy(dspfx_mixgroups *p) { return destroy_bank(p, release); }

extern "C" int dspfx_mixgroups_set_gains(dspfx_mixgroups *p, const float *host_values, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    std::string why;
    if (check_range("mixgroups", "set_gains", first_channel, count, p->desc.n_channels, why) != DSPFX_OK) return p->fail(DSPFX_ERR_INVALID, why.c_str());
    if (count == 0) return DSPFX_OK;
    Store st;
    st.first = first_channel;
    st.count = count;
    if (host_values) {
        if (!p->stores.staging(p->desc.device, count, st)) {
            const bool dev = hipSetDevice(p->desc.device) == hipSuccess;     // which of staging's two calls it was
            return dev ? p->fail(DSPFX_ERR_OOM, "mixgroups set_gains: no page-locked memory for the staged values")
                       : p->fail(DSPFX_ERR_HIP, "hipSetDevice");
        }
        std::memcpy(st.vals, host_values, count * sizeof(float));
    }
    p->stores.push(st);
    return DSPFX_OK;
}

namespace {

// the sums of a mapped bank: the pieces, then the reduce levels into dst ([nf][G]; raw: undivided)
int mapped_sums(dspfx_mixgroups *p, const Seating &t, const float *block, uint32_t n_frames, float *dst, bool raw, bool gain, hipStream_t s) {
    MapArgs a;
    a.x = block;
    a.gain = p->gain;
    a.L = t.P;
    a.pos = t.pos;
    a.rank = t.rank;
    a.slot = t.slot;
    a.swhole = t.swhole;
    a.N = p->desc.n_channels;
    a.Wrow = p->desc.tile_channels ? p->desc.tile_channels : a.N;
    a.nf = n_frames;
    a.FS = p->FS;
    a.nspans = p->nspans;
    a.nchunks = (n_frames + CHUNK - 1) / CHUNK;
    const bool vec = a.Wrow % 4 == 0 && ((uintptr_t)block & 15u) == 0;
    const uint32_t items = a.nspans * a.nchunks, blocks = (items + P1_WG / 64 - 1) / (P1_WG / 64);
    if (gain) {
        if (vec) mixrooms_partials<true, true><<<blocks, P1_WG, 0, s>>>(a);
        else mixrooms_partials<true, false><<<blocks, P1_WG, 0, s>>>(a);
    } else {
        if (vec) mixrooms_partials<false, true><<<blocks, P1_WG, 0, s>>>(a);
        else mixrooms_partials<false, false><<<blocks, P1_WG, 0, s>>>(a);
    }
    if (hipGetLastError() != hipSuccess) return p->fail(DSPFX_ERR_HIP, "mixrooms_partials");
    const float *src = t.P;
    for (const Level &l : t.levels) {
        const dim3 grid((unsigned)l.tasks.size(), (n_frames + 63) / 64);
        mixgroups_reduce<<<grid, RW * 64, 0, s>>>(raw ? l.dtasks_raw : l.dtasks, src, t.P, l.out, dst, n_frames, p->FS, p->desc.n_groups);
        if (hipGetLastError() != hipSuccess) return p->fail(DSPFX_ERR_HIP, "mixgroups_reduce");
        src = l.out;
    }
    return DSPFX_OK;
}

}  // namespace

extern "C" int dspfx_mixgroups_run(dspfx_mixgroups *p, const float *block, uint32_t n_frames, float *buses, void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    if (!block || !buses || n_frames == 0 || n_frames > p->desc.max_frames) return p->fail(DSPFX_ERR_INVALID, "mixgroups run: block, buses or n_frames");
    hipStream_t s = (hipStream_t)stream;
    BANK_HIP_WHY(hipSetDevice(p->desc.device), "hipSetDevice");
    BANK_HIP_WHY(order(p, s), "stream order");
    BANK_HIP_WHY(apply_stores(p, s), "fader store");
    if (p->seat) return mapped_sums(p, *p->seat, block, n_frames, buses, false, p->n_faded != 0, s);
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
    BANK_HIP_WHY(launch_partials<CHUNK>(a, gain, vec, s), "mixgroups_partials");
    const float *src = p->L;
    for (Level &l : p->levels) {
        const dim3 grid((unsigned)l.tasks.size(), (n_frames + 63) / 64);
        mixgroups_reduce<<<grid, RW * 64, 0, s>>>(l.dtasks, src, p->R, l.out, buses, n_frames, p->FS, a.G);
        BANK_HIP_WHY(hipGetLastError(), "mixgroups_reduce");
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
        rc = p->fail(DSPFX_ERR_OOM, "mixgroups returns: no device memory for the raw sums [max_frames][G] and the returns tables");
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
        if (!ok) rc = p->fail(DSPFX_ERR_HIP, "mixgroups returns: copying the returns tables");
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
        return p->fail(DSPFX_ERR_INVALID, "mixgroups returns: block, returns or n_frames");
    hipStream_t s = (hipStream_t)stream;
    BANK_HIP_WHY(hipSetDevice(p->desc.device), "hipSetDevice");
    const int rc = prepare_returns(p);
    if (rc != DSPFX_OK) return rc;
    BANK_HIP_WHY(order(p, s), "stream order");
    BANK_HIP_WHY(apply_stores(p, s), "fader store");       // once: the sums and the subtraction see the same table
    const bool raw = p->desc.normalise != 0;
    if (p->seat) {
        const Seating &t = *p->seat;
        const bool gain = p->n_faded != 0;
        const int st = mapped_sums(p, t, block, n_frames, p->S, raw, gain, s);
        if (st != DSPFX_OK) return st;
        const uint32_t G = p->desc.n_groups;
        if (buses) {
            const uint64_t total = (uint64_t)n_frames * G;
            mixgroups_divide<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(p->S, t.gdiv, buses, G, total);
            BANK_HIP_WHY(hipGetLastError(), "mixgroups_divide");
        }
        RetMapArgs r;
        r.x = block;
        r.out = returns;
        r.gain = p->gain;
        r.S = p->S;
        r.room = t.droom;
        r.rdiv = t.rdiv;
        r.N = p->desc.n_channels;
        r.Wrow = p->desc.tile_channels ? p->desc.tile_channels : r.N;
        r.nf = n_frames;
        r.G = G;
        r.nspans = p->nspans;
        r.nchunks = (n_frames + RCHUNK - 1) / RCHUNK;
        r.norm = raw ? 1u : 0u;
        const bool vec = r.Wrow % 4 == 0 && (((uintptr_t)block | (uintptr_t)returns) & 15u) == 0;
        const uint32_t items = r.nspans * r.nchunks, blocks = (items + P1_WG / 64 - 1) / (P1_WG / 64);
        if (gain) {
            if (vec) mixrooms_returns<true, true><<<blocks, P1_WG, 0, s>>>(r);
            else mixrooms_returns<true, false><<<blocks, P1_WG, 0, s>>>(r);
        } else {
            if (vec) mixrooms_returns<false, true><<<blocks, P1_WG, 0, s>>>(r);
            else mixrooms_returns<false, false><<<blocks, P1_WG, 0, s>>>(r);
        }
        BANK_HIP_WHY(hipGetLastError(), "mixrooms_returns");
        return DSPFX_OK;
    }
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
    BANK_HIP_WHY(launch_partials<CHUNK>(a, gain, a.Wrow % 4 == 0 && ((uintptr_t)block & 15u) == 0, s), "mixgroups_partials");
    const float *src = p->L;
    for (Level &l : p->levels) {
        const dim3 grid((unsigned)l.tasks.size(), (n_frames + 63) / 64);
        mixgroups_reduce<<<grid, RW * 64, 0, s>>>(raw ? l.dtasks_raw : l.dtasks, src, p->R, l.out, p->S, n_frames, p->FS, a.G);
        BANK_HIP_WHY(hipGetLastError(), "mixgroups_reduce");
        src = l.out;
    }
    if (buses) {
        const uint64_t total = (uint64_t)n_frames * a.G;
        mixgroups_divide<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(p->S, p->gdiv, buses, a.G, total);
        BANK_HIP_WHY(hipGetLastError(), "mixgroups_divide");
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
    BANK_HIP_WHY(launch_returns(r, gain, vec, s), "mixgroups_returns");
    return DSPFX_OK;
}

// ---- seating: a room id per channel ------------------------------------------------------------------------------------------
namespace {

// the tables of a seating, on the device before this returns (copied on the bank's own stream: no run is waited for)
int make_seating(dspfx_mixgroups *p, std::vector<uint32_t> &&room, Seating **out, const char **why) {
    const uint32_t G = p->desc.n_groups;
    RoomPlan pl;
    plan_rooms(room.data(), p->desc.n_channels, G, true, pl);
    Seating *t = new (std::nothrow) Seating;
    if (!t) {
        *why = "mixgroups assign: no host memory";
        return DSPFX_ERR_OOM;
    }
    t->room = std::move(room);
    t->pieces = pl.pieces;
    std::vector<float> gdiv(G, 1.0f), rdiv(G, 1.0f);
    std::vector<Pending> cur;
    cur.reserve(G);
    for (uint32_t g = 0; g < G; ++g) {
        const uint64_t n = pl.count[g];
        if (p->desc.normalise) gdiv[g] = dspfx_link_divisor(n);
        if (n == 1) rdiv[g] = 0.0f;                  // no other pipe: the kernel writes +0.0
        else if (p->desc.normalise && n >= 2) rdiv[g] = dspfx_link_divisor(n - 1);
        cur.push_back({g, (uint32_t)pl.first[g], (uint32_t)pl.npieces[g], NONE, gdiv[g]});
    }
    t->levels = build_levels(std::move(cur));
    const bool raw = p->desc.normalise != 0;
    const size_t cells = (size_t)p->nspans * SPAN;
    bool ok = hipMalloc((void **)&t->pos, cells) == hipSuccess && hipMalloc((void **)&t->rank, cells) == hipSuccess &&
              hipMalloc((void **)&t->slot, cells * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc((void **)&t->swhole, (size_t)p->nspans * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc((void **)&t->droom, cells * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc((void **)&t->gdiv, (size_t)G * sizeof(float)) == hipSuccess &&
              hipMalloc((void **)&t->rdiv, (size_t)G * sizeof(float)) == hipSuccess &&
              hipMalloc((void **)&t->P, (size_t)std::max<uint64_t>(pl.pieces, 1) * p->FS * sizeof(float)) == hipSuccess;
    for (Level &l : t->levels) {
        ok = ok && hipMalloc((void **)&l.dtasks, l.tasks.size() * sizeof(Task)) == hipSuccess;
        if (raw) ok = ok && hipMalloc((void **)&l.dtasks_raw, l.tasks.size() * sizeof(Task)) == hipSuccess;
        if (l.rows) ok = ok && hipMalloc((void **)&l.out, (size_t)l.rows * p->FS * sizeof(float)) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        free_seating(t);
        *why = "mixgroups assign: no device memory for the seating's tables and its pieces [pieces][max_frames]";
        return DSPFX_ERR_OOM;
    }
    hipStream_t s = p->astream;
    std::vector<std::vector<Task>> rawtasks;         // alive until the copies are done
    ok = hipMemcpyAsync(t->pos, pl.pos.data(), cells, hipMemcpyHostToDevice, s) == hipSuccess &&
         hipMemcpyAsync(t->rank, pl.rank.data(), cells, hipMemcpyHostToDevice, s) == hipSuccess &&
         hipMemcpyAsync(t->slot, pl.slot.data(), cells * sizeof(uint32_t), hipMemcpyHostToDevice, s) == hipSuccess &&
         hipMemcpyAsync(t->swhole, pl.swhole.data(), (size_t)p->nspans * sizeof(uint32_t), hipMemcpyHostToDevice, s) == hipSuccess &&
         hipMemcpyAsync(t->droom, pl.room.data(), cells * sizeof(uint32_t), hipMemcpyHostToDevice, s) == hipSuccess &&
         hipMemcpyAsync(t->gdiv, gdiv.data(), (size_t)G * sizeof(float), hipMemcpyHostToDevice, s) == hipSuccess &&
         hipMemcpyAsync(t->rdiv, rdiv.data(), (size_t)G * sizeof(float), hipMemcpyHostToDevice, s) == hipSuccess;
    for (Level &l : t->levels) {
        ok = ok && hipMemcpyAsync(l.dtasks, l.tasks.data(), l.tasks.size() * sizeof(Task), hipMemcpyHostToDevice, s) == hipSuccess;
        if (raw) {
            rawtasks.push_back(l.tasks);
            for (Task &q : rawtasks.back()) q.div = 1.0f;
            ok = ok && hipMemcpyAsync(l.dtasks_raw, rawtasks.back().data(), l.tasks.size() * sizeof(Task), hipMemcpyHostToDevice, s) == hipSuccess;
        }
    }
    const bool done = hipStreamSynchronize(s) == hipSuccess;     // (also after a failed copy: the host arrays go away)
    if (!ok || !done) {
        (void)hipGetLastError();
        free_seating(t);
        *why = "mixgroups assign: copying the seating's tables";
        return DSPFX_ERR_HIP;
    }
    *out = t;
    return DSPFX_OK;
}

int assign_fail(dspfx_mixgroups *p, int rc, const std::string &what) { return p->fail(rc, what.c_str()); }

void rooms_of_table(const std::vector<uint32_t> &gs, std::vector<uint32_t> &room) {
    for (size_t g = 0; g + 1 < gs.size(); ++g) std::fill(room.begin() + gs[g], room.begin() + gs[g + 1], (uint32_t)g);
}

}  // namespace

extern "C" int dspfx_mixgroups_assign(dspfx_mixgroups *p, const uint32_t *host_room_ids, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> alk(p->amu);
    const uint64_t N = p->desc.n_channels;
    if (!host_room_ids || count == 0) return assign_fail(p, DSPFX_ERR_INVALID, "mixgroups assign: no ids");
    if (first_channel >= N || count > N - first_channel) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "mixgroups assign: channels [%llu, %llu + %llu) are not inside the bank's %llu",
                      (unsigned long long)first_channel, (unsigned long long)first_channel, (unsigned long long)count, (unsigned long long)N);
        return assign_fail(p, DSPFX_ERR_INVALID, buf);
    }
    std::string why;
    if (check_rooms(host_room_ids, first_channel, count, p->desc.n_groups, why) != DSPFX_OK) return assign_fail(p, DSPFX_ERR_INVALID, why);
    // the map so far: only an assign changes it, and this is the only one running
    std::vector<uint32_t> room;
    try {
        if (p->seat) {
            room = p->seat->room;
        } else {
            room.assign(N, NONE);
            rooms_of_table(p->hstart, room);
        }
    } catch (const std::bad_alloc &) {
        return assign_fail(p, DSPFX_ERR_OOM, "mixgroups assign: no host memory");
    }
    std::copy(host_room_ids, host_room_ids + count, room.begin() + (size_t)first_channel);
    if (hipSetDevice(p->desc.device) != hipSuccess) return assign_fail(p, DSPFX_ERR_HIP, "hipSetDevice");
    if (!p->astream && hipStreamCreateWithFlags(&p->astream, hipStreamNonBlocking) != hipSuccess) {
        p->astream = nullptr;
        return assign_fail(p, DSPFX_ERR_HIP, "mixgroups assign: no stream for the table copies");
    }
    Seating *t = nullptr;
    const char *what = "";
    int rc;
    try {
        rc = make_seating(p, std::move(room), &t, &what);
    } catch (const std::bad_alloc &) {
        rc = DSPFX_ERR_OOM;
        what = "mixgroups assign: no host memory";
    }
    if (rc != DSPFX_OK) return assign_fail(p, rc, what);
    // the switch: every run submitted from here on is given the new seating; the old one stays until the last run given it is done
    std::lock_guard<std::mutex> lk(p->mu);
    for (size_t i = 0; i < p->retired.size();) {
        if (hipEventQuery(p->retired[i]->ev) == hipSuccess) {
            free_seating(p->retired[i]);
            p->retired[i] = p->retired.back();
            p->retired.pop_back();
        } else {
            (void)hipGetLastError();
            ++i;
        }
    }
    Seating *old = p->seat;
    p->seat = t;
    if (old) {
        if (p->used && hipEventCreateWithFlags(&old->ev, hipEventDisableTiming) == hipSuccess && hipEventRecord(old->ev, p->last) == hipSuccess) {
            p->retired.push_back(old);
        } else {
            if (p->used) (void)hipStreamSynchronize(p->last);    // no event to be had: wait instead
            free_seating(old);
        }
    }
    return DSPFX_OK;
}

extern "C" int dspfx_mixgroups_rooms(dspfx_mixgroups *p, uint32_t *host_ids_out, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    const uint64_t N = p->desc.n_channels;
    if (!host_ids_out || first_channel > N || count > N - first_channel) return p->fail(DSPFX_ERR_INVALID, "mixgroups rooms: the array or the range");
    if (p->seat) {
        std::copy(p->seat->room.begin() + (size_t)first_channel, p->seat->room.begin() + (size_t)(first_channel + count), host_ids_out);
        return DSPFX_OK;
    }
    uint32_t g = 0;
    for (uint64_t c = first_channel; c < first_channel + count; ++c) {
        while (p->hstart[g + 1] <= c) ++g;
        host_ids_out[c - first_channel] = g;
    }
    return DSPFX_OK;
}

extern "C" int dspfx_mixgroups_room_plan(const uint32_t *room_of, uint64_t n_channels, uint32_t n_groups, uint32_t tile_channels,
                                         uint64_t *count_out, uint32_t *depth_out, uint64_t *pieces_out) {
    g_err.clear();
    if (!room_of || n_groups == 0) {
        g_err = "mixgroups: no room ids, or no rooms";
        return DSPFX_ERR_INVALID;
    }
    int rc = check_shape("mixgroups", n_channels, tile_channels, g_err);
    if (rc != DSPFX_OK) return rc;
    rc = check_rooms(room_of, 0, n_channels, n_groups, g_err);
    if (rc != DSPFX_OK) return rc;
    RoomPlan pl;
    try {
        plan_rooms(room_of, n_channels, n_groups, false, pl);
    } catch (const std::bad_alloc &) {
        g_err = "mixgroups: no host memory";
        return DSPFX_ERR_OOM;
    }
    for (uint32_t g = 0; g < n_groups; ++g) {
        if (count_out) count_out[g] = pl.count[g];
        if (depth_out) depth_out[g] = room_depth(pl, g);
        if (pieces_out) pieces_out[g] = pl.npieces[g];
    }
    return DSPFX_OK;
}
