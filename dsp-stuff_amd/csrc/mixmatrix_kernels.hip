// mixmatrix_kernels.hip -- the mix-matrix bank (include/dspfx.h, dspfx_mixmatrix_*): every participant of a room has an Output node
// of their own, wired to whichever of the others they like through Gain nodes of their own (nodes/output.rs:215-249, node.rs:162-194,
// gain.rs:25-38): a gain per (listener, source) pair.  Rooms are contiguous channel ranges of 1 .. 1024 members; room r owns an
// n_r x n_r f32 matrix M_r[l][s] and a block gives
//       out[f][c0 + l] = (sum over s in [0, n_r) of M_r[l][s] * x[f][c0 + s]) / d[c0 + l]
// d = dspfx_link_divisor(w), w = the WIRED entries of the listener's row (those that are not +-0.0); a row without a wired entry
// gives +0.0; normalise = 0 writes the raw sum.  KNOWN DIFFERENCE from the reference: a wire through a Gain node of level 0 counts in
// the reference's divisor and not here (a caller who needs that uses normalise = 0 and scales the rows).  Unwired entries are
// multiplications by zero, not omissions: a NaN or an infinity in a source reaches every listener of its own room, and no other.
//
// The product is D[f][l] = sum_s A[f][s] B[s][l] on v_mfma_f32_32x32x2_f32 (A = the samples, B = the matrix): the C/D column -- the
// lane -- is the listener, so a frame row is stored as adjacent channels.  32x32x2 and not 16x16x4: per byte of operand it does twice
// the arithmetic (one A and one B register feed 2048 multiply-adds instead of 1024), so the LDS reads and the matrix loads per flop
// halve, and four independent 32x32 accumulators per wave already keep the pipe busy.  Both forms are bit for bit a k-ordered fmaf
// chain, so the choice does not touch the numerics.
//   - M is kept source-major, Mt[s][l], rows padded to P = n rounded up to 32 and the padding zero: the B operand of a k step is two
//     rows of 32 adjacent floats, one coalesced load, and the matrix never goes through LDS.
//   - A workgroup of four waves owns 128 listeners of one room (a wave 32 of them) and 128 frames -- all frames of the usual
//     block: four accumulators per wave, and the room's matrix is read from memory once per 128 frames.
//   - x is staged through LDS in chunks of 32 sources x 128 frames, read along channels; the next chunk's global loads (and the next
//     chunk's matrix rows) are issued into registers ahead of this chunk's MFMAs.
//   - A listener's sources are summed in ascending room-local order into ONE accumulator chain, zero-padded up to P: the order is a
//     function of n_r alone, so a room's bits do not depend on the layout, the frame count, its neighbours or the run.
//   - Sources past n_r and frames past n_frames are not loaded (they are +0.0 in LDS): the neighbouring room's samples never meet
//     the matrix's zero padding.  Padding listeners and padding frames are never stored.  No atomics, no scratch.
// out may not overlap the block: a room's inputs are all needed after its first outputs exist (every listener reads every source),
// so in place cannot work; the run refuses it.
//
// Stores (dspfx_mixmatrix_set_rows / _set_cols / _fill / _reset) go through the staged-store queue (store_queue.hip.h): validated,
// staged in page-locked memory, queued under the queue's own lock, and put on the next run's stream ahead of its kernel in the order they
// were made: a copy, a scatter into the source-major table, and a recount of w and d for the listeners touched -- d is computed on the
// device with dspfx_link_divisor's own f32 expression, so no store waits for the device.
//
// Seated banks (dspfx_mixmatrix_create_seats): a room owns S_r seats and an S_r x S_r table that never moves, a channel holds one
// seat of one room or none, and dspfx_mixmatrix_assign reseats channels live through the same queue: one row and one column per
// mover, never the table.  The seating rule is reseat() below, once, for the bank and for dspfx_mixmatrix_reseat.  The two kinds of
// bank share every kernel and every host path: what a room-local index means -- a member, or a seat -- is a template argument of the
// run, fill, store and recount kernels ("the two seatings" below) and data on the host.  A bank made by dspfx_mixmatrix_create runs
// the instantiation that is, instruction for instruction, what it always ran.
//
// The staged run of a seated bank (dspfx_mixmatrix_set_staging): the direct run gathers x[f][seat_chan[s]], one lane per seat, and a
// channel's frames are a whole row apart, so once participants have wandered a chunk of 32 seats reads up to 32 lines per frame
// for 32 words, per listener tile, and stores the same way.  In DSPFX_MIXMATRIX_STAGED a run is three kernels on the stream, behind
// the drained stores: mixmatrix_stage_in (the block, read once and coalesced, into a seat-ordered copy), mixmatrix_run<true, true>
// (the same chain over the copy, reading and writing along frames) and mixmatrix_stage_out (the result back, +0.0 for the channels
// in no room).  Every read of the block is over before the first write of out, so out == block is allowed in this mode.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/dspfx.h"
#include "bank_common.hip.h"
#include "store_queue.hip.h"

namespace {

constexpr uint32_t WG = 256;
constexpr uint32_t KC = 32;              // sources per LDS chunk
constexpr uint32_t FT = 128;             // frames per pass: four 32-row tiles, one accumulator each
constexpr uint32_t LT = 128;             // listeners per workgroup: 32 per wave
constexpr uint32_t XS = KC + 1;          // LDS row stride (floats): odd, so 32 frames of one source fall in 32 banks
constexpr uint32_t MAXN = DSPFX_MIXMATRIX_MAX_ROOM;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Room {
    uint64_t off;                // element offset of the room's table Mt[P][P]
    uint32_t c0, n;              // first channel, members
};
struct Item {
    uint32_t room, l0;           // a workgroup's listeners: [l0, l0 + LT) of the room
};

__host__ __device__ inline uint32_t edge(uint32_t n) { return (n + 31u) & ~31u; }

constexpr uint32_t NONE = DSPFX_MIXMATRIX_NO_ROOM;

// ---- the two seatings -----------------------------------------------------------------------------------------------------------
// What a room-local index i means.  SEATED = false (dspfx_mixmatrix_create): member i of the room, channel c0 + i; the table's edge is
// n rounded up to 32 and the indices from n on are its padding, which nobody holds.  SEATED = true (dspfx_mixmatrix_create_seats):
// seat i of S_r = Room.n seats (a multiple of 32, so the table has no padding), and Room.c0 is the room's first entry of seat_chan,
// which holds the channel in every seat (NONE: the seat is empty).  The row and the column of an index nobody holds are +0.0 in the
// table -- every store keeps that -- so a seated room computes what an unseated one computes for S_r contiguous members of which
// the absent ones carry +0.0: the same chain, term for term.
template <bool SEATED>
__device__ inline uint32_t table_edge(const Room &rm) {
    return SEATED ? rm.n : edge(rm.n);
}
// the channel at index i (below the table's edge) of the room; NONE: nobody
template <bool SEATED>
__device__ inline uint32_t chan_of(const Room &rm, const uint32_t *__restrict__ seat_chan, uint32_t i) {
    if (SEATED) return seat_chan[rm.c0 + i];
    return i < rm.n ? rm.c0 + i : NONE;
}
template <bool SEATED>
__device__ inline bool taken(const Room &rm, const uint32_t *__restrict__ seat_chan, uint32_t i) {
    return chan_of<SEATED>(rm, seat_chan, i) != NONE;
}

struct RunArgs {
    const float *__restrict__ in;
    float *__restrict__ out;
    const float *__restrict__ tab;
    const float *__restrict__ div;       // [N]: the listener's divisor; 0.0: no wired entry, the output is +0.0
    const Room *__restrict__ rooms;
    const Item *__restrict__ items;
    uint32_t N, W, nf, normalise;
    const uint32_t *__restrict__ seat_chan;      // a seated bank's; the other's kernel never reads it
    // the staged mode's (only its instantiation reads them): the seat-ordered copy of the block and of the result, [seat][MF], a
    // seat's row being its entry of seat_chan
    const float *__restrict__ sin;
    float *__restrict__ sout;
    uint32_t MF;
};

// The seatings differ in the table's edge and in two addresses (written out here, not through chan_of: each instantiation keeps the
// instruction stream it had as a kernel of its own): the source at index s is x[..][c0 + s], or x[..][seat_chan[s]], and listener
// l's row goes to out[..][c0 + l], or out[..][seat_chan[l]].  An index nobody holds is not loaded (+0.0 in LDS) and not stored.  The
// seat entry of a chunk is fetched one chunk ahead of the chunk's own loads, so the samples' addresses never wait for it
//
// STAGED (a seated bank in DSPFX_MIXMATRIX_STAGED): the same chain over the seat-ordered copy.  The source at seat s is row c0 + s of
// a.sin and listener l's result goes to row c0 + l of a.sout, both read and written ALONG FRAMES: a wave's load is 64 consecutive
// frames of one seat (two whole lines wherever the row starts), and a lane's four consecutive accumulator rows are 16 contiguous
// bytes of its listener's row.  seat_chan still decides who is loaded and who is stored: the row of an empty seat holds whatever its
// last occupant left there and is never read.  The chunk lands in LDS in the same [frame][source] image, so the MFMA loop is the
// direct kernel's, term for term
template <bool SEATED, bool STAGED = false>
__global__ __launch_bounds__(WG, 3) void mixmatrix_run(RunArgs a) {
    static_assert(SEATED || !STAGED, "only a seated bank has a staged run");
    __shared__ float xs[FT * XS];                        // [frame][source of the chunk]
    const Item it = a.items[blockIdx.x];
    const Room rm = a.rooms[it.room];
    const uint32_t n = rm.n, P = SEATED ? n : edge(n), c0 = rm.c0;
    const uint32_t *sc = a.seat_chan + c0;               // (SEATED)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t r = lane & 31u, h = lane >> 5;        // MFMA operand maps: A[i = r][k = h], B[k = h][j = r]
    const uint32_t lt = it.l0 + (uint32_t)__builtin_amdgcn_readfirstlane((int)wave) * 32u;     // the wave's listener tile (uniform)
    const bool active = lt < P;                          // wave-uniform; an idle wave still stages its share of x
    const uint32_t ss = tid & 31u, sf = tid >> 5;        // staging: source ss of the chunk, frames sf + 8 i
    const uint32_t fl = tid & 127u, sh = tid >> 7;       // (STAGED) staging: frame fl of the pass, sources sh + 2 i (wave-uniform)
    const size_t rs = a.W ? a.W : a.N;                   // a frame further is rs elements on in either layout

    // (the frame pass is a grid dimension and not a loop here: a loop would have the compiler keep every row's offset live across it)
    const uint32_t f0 = blockIdx.y * FT;
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
    float st[16], bn[KC / 2];
    // the chunk from source k0 into registers: samples outside the room or the block are +0.0 and are not read
    // the frames of the pass this thread stages: sf + 8 i for i < nst (a running pointer and one count: no offset per row is kept)
    const uint32_t left = a.nf - f0, nst = left > sf ? (left - sf + 7u) / 8u : 0u;
    const float *tabr = a.tab + rm.off;                  // uniform; the table has P * P <= 2^20 elements: 32-bit offsets
    const uint32_t bcol = (active ? lt + r : 0u) + h * P;
    uint32_t cn = 0;                                     // SEATED: who sits in this thread's seat of the next chunk to load (P >= 32)
    if constexpr (SEATED) cn = sc[ss];
    auto gload = [&](uint32_t k0) {
        if constexpr (STAGED) {
            // bit q: seat k0 + q is taken (lanes 0 .. 31 hold the chunk's 32 seats; the upper half repeats them)
            const uint32_t held = (uint32_t)__ballot(cn != NONE);
            if (k0 + KC < P) cn = sc[k0 + KC + ss];
            const bool inside = f0 + fl < a.nf;
            const float *p = a.sin + (size_t)(c0 + k0 + sh) * a.MF + f0 + fl;
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) {
                st[i] = (inside && (held >> (sh + 2u * i) & 1u)) ? *p : 0.0f;
                p += 2u * (size_t)a.MF;
            }
            if (active) {
                const uint32_t o = k0 * P + bcol;
#pragma unroll
                for (uint32_t j = 0; j < KC / 2; ++j) bn[j] = tabr[o + 2u * j * P];
            }
            return;
        }
        bool held;
        uint32_t ch;                                     // the channel whose samples p walks; nobody's index: any valid one, unread
        if constexpr (SEATED) {
            ch = cn;
            if (k0 + KC < P) cn = sc[k0 + KC + ss];
            held = ch != NONE;
            if (!held) ch = 0u;
        } else {
            const uint32_t s = k0 + ss;
            held = s < n;
            ch = c0 + (held ? s : 0u);
        }
        const float *p = a.in + lay(0, ch, a.nf, a.N, a.W) + (size_t)(f0 + sf) * rs;
        const uint32_t cnt = held ? nst : 0u;
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) {
            st[i] = i < cnt ? *p : 0.0f;
            p += 8u * rs;
        }
        if (active) {
            const uint32_t o = k0 * P + bcol;
#pragma unroll
            for (uint32_t j = 0; j < KC / 2; ++j) bn[j] = tabr[o + 2u * j * P];
        }
    };
    gload(0);
#pragma unroll 1
    for (uint32_t k0 = 0; k0 < P; k0 += KC) {
        __syncthreads();                                 // the chunk before is read
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) {
            if constexpr (STAGED) xs[fl * XS + sh + 2u * i] = st[i];   // (33 fl: a half-wave's 32 frames fall in 32 banks)
            else xs[(sf + 8u * i) * XS + ss] = st[i];
        }
        float b[KC / 2];
#pragma unroll
        for (uint32_t j = 0; j < KC / 2; ++j) b[j] = bn[j];
        __syncthreads();
        if (k0 + KC < P) gload(k0 + KC);
        if (active) {
            // the A values of k step j + 1 are read from LDS ahead of the MFMAs of step j; the fence keeps the compiler from
            // hoisting all 64 reads of the chunk (and their registers) in front of the first MFMA
            const float *xr = xs + r * XS + h;
            float an[4], ac[4];
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t) an[t] = xr[t * 32u * XS];
#pragma unroll
            for (uint32_t j = 0; j < KC / 2; ++j) {
#pragma unroll
                for (uint32_t t = 0; t < 4; ++t) ac[t] = an[t];
                if (j + 1 < KC / 2) {
#pragma unroll
                    for (uint32_t t = 0; t < 4; ++t) an[t] = xr[t * 32u * XS + 2u * (j + 1)];
                }
#pragma unroll
                for (uint32_t t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[t], b[j], acc[t], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    // C/D: column = r (the listener), row = (reg & 3) + 8 (reg >> 2) + 4 h (the frame of the tile)
    bool heard;
    uint32_t c;
    if constexpr (SEATED) {
        c = active ? sc[lt + r] : NONE;
        heard = c != NONE;
    } else {
        const uint32_t l = lt + r;
        heard = active && l < n;
        c = c0 + l;
    }
    if constexpr (STAGED) {
        if (heard) {
            const float d = a.div[c];
            float *po = a.sout + (size_t)(c0 + lt + r) * a.MF + f0;
            const bool vec = (a.MF & 3u) == 0u;          // every row starts on 16 bytes (f0 and the tile's rows are multiples of 4)
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t)
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) {
                    const uint32_t fb = t * 32u + 8u * q + 4u * h;     // accumulator rows 4 q .. 4 q + 3: frames fb .. fb + 3
                    float v[4];
#pragma unroll
                    for (uint32_t i = 0; i < 4; ++i) {
                        v[i] = acc[t][4u * q + i];
                        if (d == 0.0f) v[i] = 0.0f;
                        else if (a.normalise) v[i] = __fdiv_rn(v[i], d);
                    }
                    if (vec && f0 + fb + 4u <= a.nf) {
                        *(f32x4 *)(po + fb) = f32x4{v[0], v[1], v[2], v[3]};
                    } else {
#pragma unroll
                        for (uint32_t i = 0; i < 4; ++i)
                            if (f0 + fb + i < a.nf) po[fb + i] = v[i];
                    }
                }
        }
        return;
    }
    if (heard) {
        const float d = a.div[c];
        float *po = a.out + lay(0, c, a.nf, a.N, a.W);
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t)
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) {
                const uint32_t f = f0 + t * 32u + (i & 3u) + 8u * (i >> 2) + 4u * h;
                if (f < a.nf) {
                    float v = acc[t][i];
                    if (d == 0.0f) v = 0.0f;
                    else if (a.normalise) v = __fdiv_rn(v, d);
                    __builtin_nontemporal_store(v, po + (size_t)f * rs);
                }
                if ((i & 3u) == 3u) __builtin_amdgcn_sched_barrier(0);   // (four rows' addresses at a time, not sixty-four)
            }
    }
}

// ---- the sparse run (dspfx_mixmatrix_run_sparse) ----------------------------------------------------------------------------------
// The same chain over a LISTED set of sources per room: A_r = the room-local indices held by the channels of
// list[start[r] .. start[r] + min(count[r], MAXN)), e.g. the talker bank's audible list.  A source outside A_r is not read.
//
// Why the bits are the dense run's when every unlisted source carries +-0.0 and the room's table is finite.  The dense chain of a
// listener is acc = fmaf(x[s], Mt[s][l], acc) over ascending s from acc = +0.0.  (1) fmaf(m, +-0.0, acc) == acc for finite m unless
// acc is -0.0: the product is an exact zero and adding a zero of either sign changes neither a non-zero acc nor +0.0.  (2) The
// chain starts at +0.0.  (3) An exact cancellation gives +0.0 under round-to-nearest.  So acc is never -0.0 -- unless a non-zero
// product has underflowed to -0.0 on the way, the one excepted case, which can change the sign of a zero result -- every unlisted
// step is the identity, and what is left is the chain over the listed sources in ascending order: this kernel's.  With everybody
// listed it is the dense chain on any block.  The MFMA places listed source number k at k step k instead of s; the chain does not
// care where a term sits, only in which order the terms come.
//
//   1. a 1024-bit mask in LDS: the threads stride over the room's segment of the list and set the bit of every entry that names a
//      channel of this room (LDS atomicOr: order-free, so deterministic; duplicates count once, any order of the list gives the
//      same set).  An entry that is negative, >= N, past list_len or of another room sets nothing.
//   2. one wave turns the mask into idx[K], ascending, by a popcount prefix over its 32 words.
//   3. the dense kernel's chunk loop over the K listed sources: x[f][chan(idx[k])] into the same [frame][source] LDS image,
//      the B operand of a k step from rows Mt[idx[k]] (32 adjacent listeners: one coalesced load), K padded up to the k step with
//      +0.0 * +0.0 terms that are not loaded, the k loop of the last chunk trimmed to ceil(K / 2) steps.  The same epilogue.
// STAGED here means the epilogue only: the few listed sources are read straight from the block (no mixmatrix_stage_in), the result
// goes to the seat-ordered sout rows along frames, and mixmatrix_stage_out carries it to out in whole lines.
struct SparseArgs {
    RunArgs r;
    const int32_t *__restrict__ list;            // device: channel numbers
    const uint32_t *__restrict__ start;          // device, [G + 1]
    const uint32_t *__restrict__ count;          // device, [G]
    uint64_t list_len;
    const uint32_t *__restrict__ room_of;        // a seated bank's: the channel's room, and its entry of seat_chan
    const uint32_t *__restrict__ slot_of;
};

template <bool SEATED, bool STAGED = false>
__global__ __launch_bounds__(WG, 3) void mixmatrix_run_sparse(SparseArgs sa) {
    static_assert(SEATED || !STAGED, "only a seated bank has a staged run");
    const RunArgs &a = sa.r;
    __shared__ float xs[FT * XS];                        // [frame][listed source of the chunk]
    __shared__ uint32_t idx[MAXN];                       // the listed indices, ascending
    __shared__ uint32_t mask[MAXN / 32];
    __shared__ uint32_t listed;                          // K
    const Item it = a.items[blockIdx.x];
    const Room rm = a.rooms[it.room];
    const uint32_t n = rm.n, P = SEATED ? n : edge(n), c0 = rm.c0;
    const uint32_t *sc = a.seat_chan + c0;               // (SEATED)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t r = lane & 31u, h = lane >> 5;        // MFMA operand maps: A[i = r][k = h], B[k = h][j = r]
    const uint32_t lt = it.l0 + (uint32_t)__builtin_amdgcn_readfirstlane((int)wave) * 32u;     // the wave's listener tile (uniform)
    const bool active = lt < P;                          // wave-uniform; an idle wave still stages its share of x
    const uint32_t ss = tid & 31u, sf = tid >> 5;        // staging: listed source ss of the chunk, frames sf + 8 i
    const size_t rs = a.W ? a.W : a.N;                   // a frame further is rs elements on in either layout
    const uint32_t f0 = blockIdx.y * FT;

    // 1. the mask
    if (tid < MAXN / 32) mask[tid] = 0u;
    __syncthreads();
    {
        const uint64_t s0 = sa.start[it.room];
        const uint32_t cnt = min(sa.count[it.room], MAXN);
        for (uint32_t i = tid; i < cnt; i += WG) {
            const uint64_t e = s0 + i;
            if (e >= sa.list_len) break;
            const int32_t c = sa.list[e];
            if (c < 0 || (uint32_t)c >= a.N) continue;
            uint32_t l;
            if constexpr (SEATED) {
                if (sa.room_of[c] != it.room) continue;
                l = sa.slot_of[c] - c0;                  // the channel's seat (its entry of seat_chan, less the room's first)
            } else {
                l = (uint32_t)c - c0;
            }
            if (l < n) atomicOr(&mask[l >> 5], 1u << (l & 31u));
        }
    }
    __syncthreads();
    // 2. the list: lane w < 32 of wave 0 owns word w, and writes its bits behind those of the words below
    if (wave == 0) {
        uint32_t w = lane < MAXN / 32 ? mask[lane] : 0u;
        uint32_t incl = (uint32_t)__popc(w);
#pragma unroll
        for (uint32_t q = 0; q < 5; ++q) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, 1u << q);
            if (lane >= (1u << q)) incl += o;
        }
        uint32_t at = incl - (uint32_t)__popc(w);
        while (w) {
            idx[at++] = lane * 32u + (uint32_t)__ffs((int)w) - 1u;       // (at < K <= n <= MAXN)
            w &= w - 1u;
        }
        if (lane == 31) listed = incl;
    }
    __syncthreads();
    const uint32_t K = listed;

    // 3. the chain over the K listed sources
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
    float st[16], bn[KC / 2];
    const uint32_t left = a.nf - f0, nst = left > sf ? (left - sf + 7u) / 8u : 0u;
    const float *tabr = a.tab + rm.off;                  // uniform; the table has P * P <= 2^20 elements: 32-bit offsets
    const uint32_t bcol = active ? lt + r : 0u;
    // the chunk from listed source k0 into registers: a position past K is a +0.0 * +0.0 term and is not read
    auto gload = [&](uint32_t k0) {
        bool held = k0 + ss < K;
        const uint32_t s = held ? idx[k0 + ss] : 0u;
        uint32_t ch;                                     // the channel whose samples p walks; nobody's: any valid one, unread
        if constexpr (SEATED) {
            ch = sc[s];
            held = held && ch != NONE;
            if (!held) ch = 0u;
        } else {
            ch = c0 + s;                                 // (s < n)
        }
        const float *p = a.in + lay(0, ch, a.nf, a.N, a.W) + (size_t)(f0 + sf) * rs;
        const uint32_t cnt = held ? nst : 0u;
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) {
            st[i] = i < cnt ? *p : 0.0f;
            p += 8u * rs;
        }
        if (active) {
#pragma unroll
            for (uint32_t j = 0; j < KC / 2; ++j) {
                const uint32_t k = k0 + 2u * j + h;
                bn[j] = k < K ? tabr[idx[k < K ? k : 0u] * P + bcol] : 0.0f;
            }
        }
    };
    if (K) gload(0);
#pragma unroll 1
    for (uint32_t k0 = 0; k0 < K; k0 += KC) {
        __syncthreads();                                 // the chunk before is read
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) xs[(sf + 8u * i) * XS + ss] = st[i];
        float b[KC / 2];
#pragma unroll
        for (uint32_t j = 0; j < KC / 2; ++j) b[j] = bn[j];
        __syncthreads();
        if (k0 + KC < K) gload(k0 + KC);
        if (active) {
            const uint32_t steps = (min(K - k0, KC) + 1u) / 2u;          // (uniform) the last chunk: ceil of what is left / 2
            const float *xr = xs + r * XS + h;
            float an[4], ac[4];
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t) an[t] = xr[t * 32u * XS];
#pragma unroll
            for (uint32_t j = 0; j < KC / 2; ++j) {
                if (j < steps) {                         // (a uniform branch per step; no break: the loop unrolls, b[j] stays a register)
#pragma unroll
                    for (uint32_t t = 0; t < 4; ++t) ac[t] = an[t];
                    if (j + 1 < KC / 2) {
#pragma unroll
                        for (uint32_t t = 0; t < 4; ++t) an[t] = xr[t * 32u * XS + 2u * (j + 1)];
                    }
#pragma unroll
                    for (uint32_t t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[t], b[j], acc[t], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
    // the dense kernel's epilogue.  C/D: column = r (the listener), row = (reg & 3) + 8 (reg >> 2) + 4 h (the frame of the tile)
    bool heard;
    uint32_t c;
    if constexpr (SEATED) {
        c = active ? sc[lt + r] : NONE;
        heard = c != NONE;
    } else {
        const uint32_t l = lt + r;
        heard = active && l < n;
        c = c0 + l;
    }
    if (!heard) return;
    const float d = a.div[c];
    if constexpr (STAGED) {
        float *po = a.sout + (size_t)(c0 + lt + r) * a.MF + f0;
        const bool vec = (a.MF & 3u) == 0u;              // every row starts on 16 bytes (f0 and the tile's rows are multiples of 4)
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t)
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t fb = t * 32u + 8u * q + 4u * h;         // accumulator rows 4 q .. 4 q + 3: frames fb .. fb + 3
                float v[4];
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i) {
                    v[i] = acc[t][4u * q + i];
                    if (d == 0.0f) v[i] = 0.0f;
                    else if (a.normalise) v[i] = __fdiv_rn(v[i], d);
                }
                if (vec && f0 + fb + 4u <= a.nf) {
                    *(f32x4 *)(po + fb) = f32x4{v[0], v[1], v[2], v[3]};
                } else {
#pragma unroll
                    for (uint32_t i = 0; i < 4; ++i)
                        if (f0 + fb + i < a.nf) po[fb + i] = v[i];
                }
            }
    } else {
        float *po = a.out + lay(0, c, a.nf, a.N, a.W);
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t)
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) {
                const uint32_t f = f0 + t * 32u + (i & 3u) + 8u * (i >> 2) + 4u * h;
                if (f < a.nf) {
                    float v = acc[t][i];
                    if (d == 0.0f) v = 0.0f;
                    else if (a.normalise) v = __fdiv_rn(v, d);
                    __builtin_nontemporal_store(v, po + (size_t)f * rs);
                }
                if ((i & 3u) == 3u) __builtin_amdgcn_sched_barrier(0);   // (four rows' addresses at a time, not sixty-four)
            }
    }
}

// the channels in no room read +0.0 in every frame; launched ahead of a seated bank's mixmatrix_run while the bank has any
__global__ __launch_bounds__(WG) void mixmatrix_zero_roomless(float *__restrict__ out, const uint32_t *__restrict__ room_of, uint32_t N, uint32_t W, uint32_t nf) {
    const uint32_t c = blockIdx.x * WG + threadIdx.x;
    if (c >= N || room_of[c] != NONE) return;
    float *po = out + lay(0, c, nf, N, W);
    const size_t rs = W ? W : N;
    for (uint32_t f = 0; f < nf; ++f) po[(size_t)f * rs] = 0.0f;
}

// ---- the staged mode's transposes ---------------------------------------------------------------------------------------------
// Between the block (a frame's channels adjacent, a channel's frames a whole row apart) and the seat-ordered copies (a seat's frames
// adjacent).  A workgroup owns SG adjacent channels and the FT frames of one pass, and goes through an LDS tile [frame][channel]
// of stride SG + 1: on the block's side a wave's lanes are 64 adjacent channels of one frame, on the copy's side 64 consecutive
// frames of one channel, and both sides of the tile meet 32 banks per half-wave (lane = channel: consecutive words; lane = frame: a
// stride of 65 words).  slot_of[c] is channel c's entry of seat_chan -- its row of the copies -- or NONE
constexpr uint32_t SG = 64;
constexpr uint32_t TS = SG + 1;

// block -> sin: every seated channel's frames, contiguous, into its seat's row.  A channel in no room is not read
__global__ __launch_bounds__(WG) void mixmatrix_stage_in(const float *__restrict__ in, float *__restrict__ sin, const uint32_t *__restrict__ slot_of,
                                                         uint32_t N, uint32_t W, uint32_t nf, uint32_t MF) {
    __shared__ float ts[FT * TS];
    __shared__ uint32_t slot[SG];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t g0 = blockIdx.x * SG, f0 = blockIdx.y * FT, left = min(nf - f0, FT), c = g0 + lane;
    const size_t rs = W ? W : N;
    const uint32_t mine = c < N ? slot_of[c] : NONE;
    if (wave == 0) slot[lane] = mine;
    if (mine != NONE) {
        const float *p = in + lay(0, c, nf, N, W) + (size_t)(f0 + wave) * rs;
#pragma unroll 8
        for (uint32_t f = wave; f < left; f += WG / 64u) {
            ts[f * TS + lane] = *p;
            p += (WG / 64u) * rs;
        }
    }
    __syncthreads();
    for (uint32_t j = wave; j < SG; j += WG / 64u) {     // (j and the slot are wave-uniform)
        const uint32_t sl = slot[j];
        if (sl == NONE) continue;
        float *q = sin + (size_t)sl * MF + f0;
        for (uint32_t f = lane; f < left; f += 64u) q[f] = ts[f * TS + j];
    }
}

// sout -> out: the inverse.  A channel in no room reads +0.0 in every frame (so a staged run launches no mixmatrix_zero_roomless)
__global__ __launch_bounds__(WG) void mixmatrix_stage_out(const float *__restrict__ sout, float *__restrict__ out, const uint32_t *__restrict__ slot_of,
                                                          uint32_t N, uint32_t W, uint32_t nf, uint32_t MF) {
    __shared__ float ts[FT * TS];
    __shared__ uint32_t slot[SG];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t g0 = blockIdx.x * SG, f0 = blockIdx.y * FT, left = min(nf - f0, FT), c = g0 + lane;
    const size_t rs = W ? W : N;
    if (wave == 0) slot[lane] = c < N ? slot_of[c] : NONE;       // (a channel past N: zeros in the tile, never stored)
    __syncthreads();
    // a wave takes channels wave, wave + 4, ..: four rows' loads (two halves of FT frames each) are issued before the first of them
    // is needed, so a wave does not wait out one row's latency after the other
    constexpr uint32_t NW = WG / 64u, UN = 4;
#pragma unroll
    for (uint32_t jb = 0; jb < SG / NW; jb += UN) {
        float v[UN][FT / 64u];
#pragma unroll
        for (uint32_t u = 0; u < UN; ++u) {
            const uint32_t sl = slot[wave + NW * (jb + u)];
            const float *q = sout + (size_t)(sl != NONE ? sl : 0u) * MF + f0;
#pragma unroll
            for (uint32_t hh = 0; hh < FT / 64u; ++hh) {
                const uint32_t f = lane + 64u * hh;
                v[u][hh] = (sl != NONE && f < left) ? q[f] : 0.0f;
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < UN; ++u)
#pragma unroll
            for (uint32_t hh = 0; hh < FT / 64u; ++hh) ts[(lane + 64u * hh) * TS + wave + NW * (jb + u)] = v[u][hh];
    }
    __syncthreads();
    if (c < N) {
        float *p = out + lay(0, c, nf, N, W) + (size_t)(f0 + wave) * rs;
#pragma unroll 8
        for (uint32_t f = wave; f < left; f += WG / 64u) {
            __builtin_nontemporal_store(ts[f * TS + lane], p);
            p += (WG / 64u) * rs;
        }
    }
}

// a preset into the tables of rooms [first_room, first_room + gridDim.x): one workgroup per room.  Mix-minus is 1.0 between two
// different TAKEN indices; everything else, the padding with it, is +0.0
template <bool SEATED>
__global__ __launch_bounds__(WG) void mixmatrix_fill(float *__restrict__ tab, const Room *__restrict__ rooms, const uint32_t *__restrict__ seat_chan,
                                                     uint32_t first_room, uint32_t preset) {
    const Room rm = rooms[first_room + blockIdx.x];
    const uint32_t P = table_edge<SEATED>(rm);
    float *t = tab + rm.off;
    for (uint32_t e = threadIdx.x; e < P * P; e += WG) {
        const uint32_t s = e / P, l = e - s * P;
        t[e] = (preset == DSPFX_MIXMATRIX_MIX_MINUS && s != l && taken<SEATED>(rm, seat_chan, s) && taken<SEATED>(rm, seat_chan, l)) ? 1.0f : 0.0f;
    }
}

// staged lines into the room's source-major table: words = [count] room-local indices, then [count][Room.n] values (a line is as long
// as the room has members, or seats).  Line i belongs to index q = words[i].  cols = 0: it is what listener q hears, vals[i][s] ->
// Mt[s][q]; cols = 1: it is how loud source q is for each listener, vals[i][l] -> Mt[q][l].  A value at an empty seat is stored as +0.0
template <bool SEATED>
__global__ __launch_bounds__(WG) void mixmatrix_store(float *__restrict__ tab, const uint32_t *__restrict__ words, const uint32_t *__restrict__ seat_chan,
                                                      Room rm, uint32_t count, uint32_t cols) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x, n = rm.n, P = table_edge<SEATED>(rm);
    if (e >= count * n) return;
    const uint32_t i = e / n, j = e - i * n, q = words[i];
    const float v = taken<SEATED>(rm, seat_chan, j) ? __uint_as_float(words[count + e]) : 0.0f;
    float *t = tab + rm.off;
    if (cols) t[(size_t)q * P + j] = v;
    else t[(size_t)j * P + q] = v;
}

// words = [n] (channel, room or NONE) pairs: the movers of an assign.  Every mover leaves its row of the staged copies here;
// mixmatrix_seat_set, behind it, gives those who sit down again their new one (so a swap between two full rooms comes out right)
__global__ __launch_bounds__(WG) void mixmatrix_chan_set(uint32_t *__restrict__ room_of, uint32_t *__restrict__ slot_of, const uint32_t *__restrict__ words,
                                                         uint32_t n) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    room_of[words[2u * i]] = words[2u * i + 1u];
    slot_of[words[2u * i]] = NONE;
}

// words = [n] (seat_chan index, channel or NONE) pairs: the seats an assign changed, each with who sits there after the call (a
// seat can be named twice, with the same occupant)
__global__ __launch_bounds__(WG) void mixmatrix_seat_set(uint32_t *__restrict__ seat_chan, uint32_t *__restrict__ slot_of, const uint32_t *__restrict__ words,
                                                         uint32_t n) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const uint32_t at = words[2u * i], c = words[2u * i + 1u];
    seat_chan[at] = c;
    if (c != NONE) slot_of[c] = at;
}

// words = [gridDim.x] (room, seat | preset << 31) pairs: the seats an assign emptied (preset bit clear) or gave to a newcomer.  The
// seat's row and column: mix-minus (bit set) is 1.0 towards every other taken seat by the seating AFTER the call (seat_chan already
// holds it), everything else +0.0.  Two changed seats of one room write the entries between them twice, with the same value
__global__ __launch_bounds__(WG) void mixmatrix_seat_lines(float *__restrict__ tab, const Room *__restrict__ rooms, const uint32_t *__restrict__ seat_chan,
                                                           const uint32_t *__restrict__ words) {
    const Room rm = rooms[words[2u * blockIdx.x]];
    const uint32_t w = words[2u * blockIdx.x + 1u], q = w & 0x7FFFFFFFu, S = rm.n;
    float *t = tab + rm.off;
    for (uint32_t j = threadIdx.x; j < S; j += WG) {
        const float v = ((w >> 31) && j != q && seat_chan[rm.c0 + j] != NONE) ? 1.0f : 0.0f;
        t[q * S + j] = v;
        t[j * S + q] = v;
    }
}

// words = [n] (room, listener index << 16 | source index, gain) triples into the source-major tables (indices are seats in a seated
// bank and room-local members otherwise); the host has dropped all but the last of equal pairs
__global__ __launch_bounds__(WG) void mixmatrix_pairs(float *__restrict__ tab, const Room *__restrict__ rooms, const uint32_t *__restrict__ words, uint32_t n) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const Room rm = rooms[words[3u * i]];
    const uint32_t ls = words[3u * i + 1u], P = edge(rm.n);
    tab[rm.off + (size_t)(ls & 0xFFFFu) * P + (ls >> 16)] = __uint_as_float(words[3u * i + 2u]);
}

// w and d of the listeners at indices [i0, i0 + count) -- those that exist and are taken -- of the rooms list[blockIdx.x] (list =
// nullptr: first_room + blockIdx.x): w = the entries of the listener's row that are not +-0.0 (the padding never is); d =
// dspfx_link_divisor(w) by its own f32 expression (node.rs:166,179: sequential f32 increments from 0.0001), 0.0 for a row without a
// wired entry
template <bool SEATED>
__global__ __launch_bounds__(WG) void mixmatrix_recount(const float *__restrict__ tab, const Room *__restrict__ rooms, const uint32_t *__restrict__ seat_chan,
                                                        float *__restrict__ div, const uint32_t *__restrict__ list, uint32_t first_room, uint32_t i0,
                                                        uint32_t count) {
    const Room rm = rooms[list ? list[blockIdx.x] : first_room + blockIdx.x];
    const uint32_t P = table_edge<SEATED>(rm), at = blockIdx.y * WG + threadIdx.x, l = i0 + at;
    if (at >= count || l >= P) return;
    const uint32_t c = chan_of<SEATED>(rm, seat_chan, l);
    if (c == NONE) return;
    const float *t = tab + rm.off + l;
    uint32_t w = 0;
    for (uint32_t s = 0; s < P; ++s) w += t[(size_t)s * P] != 0.0f;
    float d = 0.0f;
    if (w) {
        d = 0.0001f;
        for (uint32_t k = 0; k < w; ++k) d = d + 1.0f;   // (w <= 1024: never saturates)
    }
    div[c] = d;
}

thread_local std::string g_err;        // the reason of the last failed create or plan on this thread

// a store's vals (the buffer is 4-byte words: integers travel as their bits).  Rows or columns: [count] room-local indices (members,
// or seats), then [count][Room.n] values; a fill has none.  An assign's words: [n_seats] (seat_chan index, channel) pairs, [n_chans]
// (channel, room) pairs, [n_lines] (room, seat | preset << 31) pairs, [n_rooms] rooms to recount.  Pairs: [n_lines] (room,
// listener << 16 | source, gain) triples, [n_rooms] rooms
enum Kind { ROWS, COLS, FILL, ASSIGN, PAIRS };
struct StoreFields {
    Kind kind = ROWS;
    uint32_t room = 0, l0 = 0, count = 0;        // rows / columns: room-local first index and count; fill: rooms [room, room + count)
    uint32_t preset = 0;
    size_t n_seats = 0, n_chans = 0, n_lines = 0, n_rooms = 0;
    uint64_t roomless = 0;       // an assign: the channels in no room once it is applied
};
typedef StoreQueue<StoreFields> Stores;
typedef Stores::Store Store;

// one channel of an assign that changes rooms: from seat q0 of room r0 to seat q1 of room r1 (NONE: no room, no seat)
struct Move {
    uint32_t c, r0, q0, r1, q1;
};

// host tables of a seating: who sits where.  S[g] = the seats of room g (a multiple of 32), off[g] = its first entry of seat_chan
struct Seats {
    uint32_t *room_of, *seat_of, *seat_chan, *occ;
    const uint32_t *S, *off;
    uint32_t G;
    uint64_t N;
};

// THE SEATING RULE (include/dspfx.h, dspfx_mixmatrix_assign), for the bank and for dspfx_mixmatrix_reseat.  The range, every id and
// every room's capacity are checked before anything changes.  Then the named channels whose id is not their room leave (their seat
// is free), and those that enter a room do so in ascending channel order, each into the lowest free seat.  -> the moves made.
// O(count + the seats of the rooms entered)
int reseat(const Seats &t, const uint32_t *ids, uint64_t first, uint64_t count, std::string &why, std::vector<Move> &moves) {
    char buf[192];
    if (!ids || count == 0) {
        why = "mixmatrix assign: no ids";
        return DSPFX_ERR_INVALID;
    }
    if (first >= t.N || count > t.N - first) {
        std::snprintf(buf, sizeof buf, "mixmatrix assign: channels [%llu, %llu + %llu) are not inside the bank's %llu", (unsigned long long)first,
                      (unsigned long long)first, (unsigned long long)count, (unsigned long long)t.N);
        why = buf;
        return DSPFX_ERR_INVALID;
    }
    std::unordered_map<uint32_t, int64_t> delta;         // per room touched: enters - leaves
    size_t n_moves = 0;
    for (uint64_t i = 0; i < count; ++i) {
        const uint32_t g = ids[i], was = t.room_of[first + i];
        if (g != NONE && g >= t.G) {
            std::snprintf(buf, sizeof buf, "mixmatrix assign: channel %llu is given room %u, and there are %u rooms (or DSPFX_MIXMATRIX_NO_ROOM)",
                          (unsigned long long)(first + i), g, t.G);
            why = buf;
            return DSPFX_ERR_INVALID;
        }
        if (g == was) continue;
        ++n_moves;
        if (was != NONE) --delta[was];
        if (g != NONE) ++delta[g];
    }
    uint32_t full = NONE;                                // the lowest room that would overflow
    for (const auto &d : delta)
        if ((int64_t)t.occ[d.first] + d.second > (int64_t)t.S[d.first] && d.first < full) full = d.first;
    if (full != NONE) {
        std::snprintf(buf, sizeof buf, "mixmatrix assign: room %u would hold %lld participants, and has %u seats (capacity)", full,
                      (long long)((int64_t)t.occ[full] + delta[full]), t.S[full]);
        why = buf;
        return DSPFX_ERR_INVALID;
    }
    moves.clear();
    moves.reserve(n_moves);
    for (uint64_t i = 0; i < count; ++i) {               // the leaves
        const uint32_t c = (uint32_t)(first + i), was = t.room_of[c];
        if (ids[i] == was) continue;
        moves.push_back(Move{c, was, t.seat_of[c], ids[i], NONE});
        if (was != NONE) {
            t.seat_chan[t.off[was] + t.seat_of[c]] = NONE;
            --t.occ[was];
        }
        t.room_of[c] = NONE;
        t.seat_of[c] = NONE;
    }
    std::unordered_map<uint32_t, uint32_t> from;         // per room entered: no seat below this one is free
    for (Move &m : moves) {                              // the enters, in ascending channel order
        if (m.r1 == NONE) continue;
        uint32_t &q = from[m.r1];
        while (t.seat_chan[t.off[m.r1] + q] != NONE) ++q;        // (the capacity check has shown there is one)
        m.q1 = q;
        t.seat_chan[t.off[m.r1] + q] = m.c;
        ++t.occ[m.r1];
        t.room_of[m.c] = m.r1;
        t.seat_of[m.c] = q;
    }
    return DSPFX_OK;
}

// takes the moves back, for an assign that could not be queued
void unseat(const Seats &t, const std::vector<Move> &moves) {
    for (const Move &m : moves)
        if (m.r1 != NONE) {
            t.seat_chan[t.off[m.r1] + m.q1] = NONE;
            --t.occ[m.r1];
        }
    for (const Move &m : moves) {
        if (m.r0 != NONE) {
            t.seat_chan[t.off[m.r0] + m.q0] = m.c;
            ++t.occ[m.r0];
        }
        t.room_of[m.c] = m.r0;
        t.seat_of[m.c] = m.q0;
    }
}

// seats[g] rounded up to 32 into S and the rooms' first seat_chan entries into off; members = nullptr: no lower limit
int check_seats(const char *what, const uint32_t *seats, const uint32_t *members, uint32_t G, std::vector<uint32_t> &S, std::vector<uint32_t> &off,
                std::string &why) {
    char buf[192];
    if (!seats) {
        why = std::string(what) + ": no seats";
        return DSPFX_ERR_INVALID;
    }
    S.resize(G);
    off.resize(G);
    uint64_t total = 0;
    for (uint32_t g = 0; g < G; ++g) {
        const uint32_t n = members ? members[g] : 1u;
        if (seats[g] < n || seats[g] > MAXN) {
            std::snprintf(buf, sizeof buf, "%s: room %u is given %u seats, and it has %u members (a room has at most DSPFX_MIXMATRIX_MAX_ROOM = %u seats)",
                          what, g, seats[g], members ? n : 0u, MAXN);
            why = buf;
            return DSPFX_ERR_INVALID;
        }
        S[g] = edge(seats[g]);
        off[g] = (uint32_t)total;
        total += S[g];
        if (total > 0xFFFFFF00ull) {
            why = std::string(what) + ": more than 2^32 - 256 seats";
            return DSPFX_ERR_INVALID;
        }
    }
    return DSPFX_OK;
}

}  // namespace

struct dspfx_mixmatrix : BankError {
    dspfx_mixmatrix_desc desc{};
    std::vector<uint64_t> gs;                    // the table, [G + 1]
    std::vector<Room> hrooms;
    std::mutex mu;                               // run / destroy
    Stores stores;                               // the matrix stores
    float *tab = nullptr, *div = nullptr, *stage = nullptr;      // stage: [maxn][maxn + 1], where a drained store's words land
    Room *rooms = nullptr;
    Item *items = nullptr;
    uint32_t n_items = 0, maxn = 0;
    size_t stage_words = 0;                      // the size of `stage`; longer word lists go through it in slices
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;
    bool used = false;
    // a seated bank (dspfx_mixmatrix_create_seats): Room.n is the room's seats and Room.c0 its first entry of seat_chan.  The host
    // tables hold the seating after every assign made so far; the device ones (room_of, seat_chan) what the runs drained so far see
    bool seated = false;
    std::mutex smu;                              // the host tables, held from a store's checks to its push (smu, then the queue's lock)
    std::vector<uint32_t> hroom_of, hseat_of, hseat_chan, hS, hoff;
    std::vector<uint32_t> occ;                   // participants per room (either kind of bank: the members, where nobody moves)
    uint64_t hroomless = 0;                      // channels in no room (smu)
    uint64_t roomless = 0;                       // ... by the assigns drained so far (mu)
    uint32_t *room_of = nullptr, *seat_chan = nullptr;
    uint32_t *slot_of = nullptr;                 // [N]: the channel's entry of seat_chan (NONE: in no room), kept by every assign
    // the staged mode (dspfx_mixmatrix_set_staging).  `mode` is read once by a run, so a run is wholly one mode; sbuf is written once,
    // under gmu, before the first store of STAGED into mode, and kept until release
    std::atomic<uint32_t> mode{DSPFX_MIXMATRIX_DIRECT};
    std::mutex gmu;                              // set_staging
    float *sbuf = nullptr;                       // the two seat-ordered copies, [2][n_slots][max_frames]; never zeroed
    uint64_t n_slots = 0;                        // the sum of S_r: the entries of seat_chan
    Seats seats() { return Seats{hroom_of.data(), hseat_of.data(), hseat_chan.data(), occ.data(), hS.data(), hoff.data(), desc.n_groups, desc.n_channels}; }
};

namespace {

void release(dspfx_mixmatrix *p) { release_bank(p, {p->tab, p->div, p->stage, p->rooms, p->items, p->room_of, p->seat_chan, p->slot_of, p->sbuf}); }

// the room and the room-local index (the seat, in a seated bank) of channel c; smu is held on a seated bank
void place_of(dspfx_mixmatrix *p, uint32_t c, uint32_t &room, uint32_t &index) {
    if (p->seated) {
        room = p->hroom_of[c];
        index = p->hseat_of[c];
    } else {
        room = (uint32_t)(std::upper_bound(p->gs.begin(), p->gs.end(), (uint64_t)c) - p->gs.begin()) - 1;
        index = c - (uint32_t)p->gs[room];
    }
}

// the divisors of the listeners at indices [i0, i0 + count) of rooms [first_room, first_room + n_rooms), or of the n_rooms listed at
// `list` (device); a range past a room's edge ends there, so count = maxn means whole rooms
hipError_t recount(dspfx_mixmatrix *p, const uint32_t *list, uint32_t first_room, uint32_t n_rooms, uint32_t i0, uint32_t count, hipStream_t s) {
    const auto kernel = p->seated ? mixmatrix_recount<true> : mixmatrix_recount<false>;
    kernel<<<dim3(n_rooms, (count + WG - 1) / WG), WG, 0, s>>>(p->tab, p->rooms, p->seat_chan, p->div, list, first_room, i0, count);
    return hipGetLastError();
}

// n records of `rec` words at src (page-locked) through `stage`, a slice at a time: launch(the slice on the device, its records)
template <class F>
hipError_t sliced(dspfx_mixmatrix *p, const uint32_t *src, size_t n, uint32_t rec, hipStream_t s, F launch) {
    const size_t per = p->stage_words / rec;
    for (size_t i = 0; i < n; i += per) {
        const size_t k = std::min(per, n - i);
        hipError_t err = hipMemcpyAsync(p->stage, src + i * rec, k * rec * sizeof(uint32_t), hipMemcpyHostToDevice, s);
        if (err != hipSuccess) return err;
        err = launch((const uint32_t *)p->stage, (uint32_t)k);
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

// the divisors of every listener of the n rooms listed at src (page-locked)
hipError_t recount_rooms(dspfx_mixmatrix *p, const uint32_t *src, size_t n, hipStream_t s) {
    return sliced(p, src, n, 1, s, [&](const uint32_t *w, uint32_t k) { return recount(p, w, 0, k, 0, p->maxn, s); });
}

hipError_t fill_rooms(dspfx_mixmatrix *p, uint32_t first_room, uint32_t count, uint32_t preset, hipStream_t s) {
    const auto kernel = p->seated ? mixmatrix_fill<true> : mixmatrix_fill<false>;
    kernel<<<count, WG, 0, s>>>(p->tab, p->rooms, p->seat_chan, first_room, preset);
    const hipError_t err = hipGetLastError();
    return err != hipSuccess ? err : recount(p, nullptr, first_room, count, 0, p->maxn, s);
}

// one store onto the stream: a fill, or the values into `stage`, the scatter into the table and the recount
hipError_t apply_store(dspfx_mixmatrix *p, const Store &st, hipStream_t s) {
    if (st.kind == FILL) return fill_rooms(p, st.room, st.count, st.preset, s);
    const uint32_t *words = (const uint32_t *)st.vals;
    if (st.kind == ASSIGN) {                     // the rooms of the channels, the seats, the lines, the divisors -- in that order
        hipError_t err = sliced(p, words + 2 * st.n_seats, st.n_chans, 2, s, [&](const uint32_t *w, uint32_t k) {
            mixmatrix_chan_set<<<(k + WG - 1) / WG, WG, 0, s>>>(p->room_of, p->slot_of, w, k);
            return hipGetLastError();
        });
        if (err != hipSuccess) return err;
        err = sliced(p, words, st.n_seats, 2, s, [&](const uint32_t *w, uint32_t k) {
            mixmatrix_seat_set<<<(k + WG - 1) / WG, WG, 0, s>>>(p->seat_chan, p->slot_of, w, k);
            return hipGetLastError();
        });
        if (err != hipSuccess) return err;
        words += 2 * st.n_seats + 2 * st.n_chans;
        err = sliced(p, words, st.n_lines, 2, s, [&](const uint32_t *w, uint32_t k) {
            mixmatrix_seat_lines<<<k, WG, 0, s>>>(p->tab, p->rooms, p->seat_chan, w);
            return hipGetLastError();
        });
        if (err != hipSuccess) return err;
        p->roomless = st.roomless;
        return recount_rooms(p, words + 2 * st.n_lines, st.n_rooms, s);
    }
    if (st.kind == PAIRS) {
        const hipError_t err = sliced(p, words, st.n_lines, 3, s, [&](const uint32_t *w, uint32_t k) {
            mixmatrix_pairs<<<(k + WG - 1) / WG, WG, 0, s>>>(p->tab, p->rooms, w, k);
            return hipGetLastError();
        });
        return err != hipSuccess ? err : recount_rooms(p, words + 3 * st.n_lines, st.n_rooms, s);
    }
    const Room &rm = p->hrooms[st.room];
    hipError_t err = hipMemcpyAsync(p->stage, st.vals, (size_t)st.count * (rm.n + 1) * sizeof(float), hipMemcpyHostToDevice, s);
    if (err != hipSuccess) return err;
    const auto kernel = p->seated ? mixmatrix_store<true> : mixmatrix_store<false>;
    kernel<<<(st.count * rm.n + WG - 1) / WG, WG, 0, s>>>(p->tab, (const uint32_t *)p->stage, p->seat_chan, rm, st.count, (uint32_t)(st.kind == COLS));
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    // a row store changes the wired count of its listeners -- adjacent members, or seats anywhere in the room -- and a column store
    // that of every listener of the room
    const bool own = st.kind == ROWS && !p->seated;
    return recount(p, nullptr, st.room, 1, own ? st.l0 : 0u, own ? st.count : rm.n, s);
}

// rows or columns [first, first + count) of one room, row_len values each
int store_lines(dspfx_mixmatrix *p, Kind kind, const float *vals, uint32_t row_len, uint64_t first, uint64_t count) {
    const char *what = kind == COLS ? "set_cols" : "set_rows";
    char buf[224];
    if (!vals) {
        std::snprintf(buf, sizeof buf, "mixmatrix %s: no values", what);
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    std::string why;                             // (a range that begins at N is in no room: not even an empty one is inside)
    if (check_range("mixmatrix", what, first, count, p->desc.n_channels, why, false) != DSPFX_OK) return p->fail(DSPFX_ERR_INVALID, why.c_str());
    std::lock_guard<std::mutex> lk(p->smu);
    uint32_t room, l0;
    place_of(p, (uint32_t)first, room, l0);
    if (p->seated) {
        // lines by seat: the channels must share a room by the seating so far (any seats of it)
        for (uint64_t c = first; c < first + count || c == first; ++c)
            if (p->hroom_of[c] != room || room == NONE) {
                std::snprintf(buf, sizeof buf, "mixmatrix %s: channels [%llu, %llu + %llu) are not in one room by the seating (channel %llu is not in the room of the first)",
                              what, (unsigned long long)first, (unsigned long long)first, (unsigned long long)count, (unsigned long long)c);
                return p->fail(DSPFX_ERR_INVALID, buf);
            }
    } else if (first + count > p->gs[room + 1]) {
        std::snprintf(buf, sizeof buf, "mixmatrix %s: channels [%llu, %llu + %llu) are not in one room (room %u is [%u, %u))", what,
                      (unsigned long long)first, (unsigned long long)first, (unsigned long long)count, room, (uint32_t)p->gs[room], (uint32_t)p->gs[room + 1]);
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    const uint32_t len = p->hrooms[room].n;      // a line is as long as the room has members, or seats
    if (row_len != len) {
        std::snprintf(buf, sizeof buf, "mixmatrix %s: a row of %u values, and room %u has %u %s", what, row_len, room, len, p->seated ? "seats" : "members");
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    if (count == 0) return DSPFX_OK;
    Store st;
    st.kind = kind;
    st.room = room;
    st.l0 = l0;
    st.count = (uint32_t)count;
    const size_t cells = (size_t)count * len;
    if (!p->stores.staging(p->desc.device, count + cells, st)) {
        std::snprintf(buf, sizeof buf, "mixmatrix %s: no page-locked memory for the staged values", what);
        return p->fail(DSPFX_ERR_OOM, buf);
    }
    uint32_t *index = (uint32_t *)st.vals;
    for (uint64_t i = 0; i < count; ++i) index[i] = p->seated ? p->hseat_of[first + i] : l0 + (uint32_t)i;
    std::memcpy(st.vals + count, vals, cells * sizeof(float));
    p->stores.push(st);
    return DSPFX_OK;
}

// counts, table edges, table offsets and the total of a bank's rooms.  The edge of a room is its seats rounded up to 32 in a seated
// bank (seats: [n_groups]) and its members rounded up to 32 otherwise
int plan(const uint64_t *group_start, uint32_t n_groups, uint64_t n_channels, uint32_t tile_channels, const uint32_t *seats, bool seated,
         uint32_t *count_out, uint32_t *edge_out, uint64_t *offset_out, uint64_t *total_bytes_out) {
    g_err.clear();
    const int rc = check_table("mixmatrix", group_start, n_groups, n_channels, tile_channels, MAXN, g_err);
    if (rc != DSPFX_OK) return rc;
    try {
        std::vector<uint32_t> S, off;
        if (seated) {
            std::vector<uint32_t> cnt(n_groups);
            for (uint32_t g = 0; g < n_groups; ++g) cnt[g] = (uint32_t)(group_start[g + 1] - group_start[g]);
            const int src = check_seats("mixmatrix", seats, cnt.data(), n_groups, S, off, g_err);
            if (src != DSPFX_OK) return src;
        }
        uint64_t at = 0;
        for (uint32_t g = 0; g < n_groups; ++g) {
            const uint32_t n = (uint32_t)(group_start[g + 1] - group_start[g]), P = seated ? S[g] : edge(n);
            if (count_out) count_out[g] = n;
            if (edge_out) edge_out[g] = P;
            if (offset_out) offset_out[g] = at;
            at += (uint64_t)P * P;
        }
        if (total_bytes_out) *total_bytes_out = at * sizeof(float);
    } catch (const std::bad_alloc &) {
        g_err = "mixmatrix: no host memory for the room tables";
        return DSPFX_ERR_OOM;
    }
    return DSPFX_OK;
}

}  // namespace

extern "C" const char *dspfx_mixmatrix_last_error(const dspfx_mixmatrix *p) { return p ? p->err.c_str() : g_err.c_str(); }

extern "C" int dspfx_mixmatrix_plan(const uint64_t *group_start, uint32_t n_groups, uint64_t n_channels, uint32_t tile_channels,
                                    uint32_t *count_out, uint32_t *edge_out, uint64_t *offset_out, uint64_t *total_bytes_out) {
    return plan(group_start, n_groups, n_channels, tile_channels, nullptr, false, count_out, edge_out, offset_out, total_bytes_out);
}

extern "C" int dspfx_mixmatrix_plan_seats(const uint64_t *group_start, uint32_t n_groups, uint64_t n_channels, uint32_t tile_channels, const uint32_t *seats,
                                          uint32_t *count_out, uint32_t *edge_out, uint64_t *offset_out, uint64_t *total_bytes_out) {
    return plan(group_start, n_groups, n_channels, tile_channels, seats, true, count_out, edge_out, offset_out, total_bytes_out);
}

namespace {

// seats: a seated bank's seats per room (host, [n_groups])
int create_bank(const dspfx_mixmatrix_desc *desc, const uint32_t *seats, bool seated, dspfx_mixmatrix **out) {
    if (!desc || !out) {
        g_err = "mixmatrix: null argument";
        return DSPFX_ERR_INVALID;
    }
    *out = nullptr;
    g_err.clear();
    if (desc->abi_version != DSPFX_ABI_VERSION) {
        char buf[96];
        std::snprintf(buf, sizeof buf, "mixmatrix: abi_version %u, and the library's is %u", desc->abi_version, (unsigned)DSPFX_ABI_VERSION);
        g_err = buf;
        return DSPFX_ERR_INVALID;
    }
    if (desc->max_frames == 0 || desc->max_frames > (1u << 20)) {
        g_err = "mixmatrix: max_frames must be 1 .. 2^20";
        return DSPFX_ERR_INVALID;
    }
    const uint32_t G = desc->n_groups, N = desc->n_channels;
    uint64_t total_bytes = 0;
    std::vector<uint32_t> cnt, edges;
    std::vector<uint64_t> offs;
    std::vector<Item> items;
    std::vector<uint32_t> slots;                         // a seated bank's first slot_of
    dspfx_mixmatrix *p = nullptr;
    try {
        cnt.resize(G ? G : 1);
        offs.resize(G ? G : 1);
        edges.resize(G ? G : 1);
        const int rc = plan(desc->group_start, G, N, desc->tile_channels, seats, seated, cnt.data(), edges.data(), offs.data(), &total_bytes);
        if (rc != DSPFX_OK) return rc;
        if ((uint64_t)N * desc->max_frames > (1ull << 40)) {
            g_err = "mixmatrix: n_channels x max_frames is too large";
            return DSPFX_ERR_INVALID;
        }
        const int dev_rc = open_device("mixmatrix", desc->device, &g_err);
        if (dev_rc != DSPFX_OK) return dev_rc;
        p = new dspfx_mixmatrix;
        p->desc = *desc;
        p->gs.assign(desc->group_start, desc->group_start + G + 1);
        p->desc.group_start = nullptr;
        p->hrooms.resize(G);
        p->seated = seated;
        p->occ = cnt;
        uint32_t seat0 = 0;
        for (uint32_t g = 0; g < G; ++g) {
            p->hrooms[g] = seated ? Room{offs[g], seat0, edges[g]} : Room{offs[g], (uint32_t)p->gs[g], cnt[g]};
            p->maxn = std::max(p->maxn, p->hrooms[g].n);
            for (uint32_t l0 = 0; l0 < edges[g]; l0 += LT) items.push_back(Item{g, l0});
            seat0 += seated ? edges[g] : 0u;
        }
        if (seated) {                                    // channel c0 + i of a room sits in its seat i
            p->hroom_of.resize(N);
            p->hseat_of.resize(N);
            p->hseat_chan.assign(seat0, NONE);
            p->hS = edges;
            p->hoff.resize(G);
            for (uint32_t g = 0; g < G; ++g) {
                p->hoff[g] = p->hrooms[g].c0;
                std::fill(p->hroom_of.begin() + p->gs[g], p->hroom_of.begin() + p->gs[g + 1], g);
                for (uint32_t i = 0; i < cnt[g]; ++i) {
                    p->hseat_of[p->gs[g] + i] = i;
                    p->hseat_chan[p->hoff[g] + i] = (uint32_t)p->gs[g] + i;
                }
            }
            p->n_slots = seat0;
            slots.resize(N);
            for (uint32_t c = 0; c < N; ++c) slots[c] = p->hoff[p->hroom_of[c]] + p->hseat_of[c];
        }
        // `stage` takes a room's lines (and their indices) at once, and at least a page of an assign's or a pair store's words
        p->stage_words = std::max<size_t>((size_t)p->maxn * p->maxn + p->maxn, 4096);
    } catch (const std::bad_alloc &) {
        delete p;
        g_err = "mixmatrix: no host memory for the room tables";
        return DSPFX_ERR_OOM;
    }
    if (items.size() > 0x7FFFFFFFull) {
        delete p;
        g_err = "mixmatrix: too many listener tiles for one launch";
        return DSPFX_ERR_INVALID;
    }
    p->n_items = (uint32_t)items.size();
    bool ok = hipMalloc((void **)&p->tab, total_bytes) == hipSuccess && hipMalloc((void **)&p->div, (size_t)N * sizeof(float)) == hipSuccess &&
              hipMalloc((void **)&p->stage, p->stage_words * sizeof(float)) == hipSuccess &&
              (!seated || hipMalloc((void **)&p->seat_chan, p->hseat_chan.size() * sizeof(uint32_t)) == hipSuccess) &&
              hipMalloc((void **)&p->rooms, (size_t)G * sizeof(Room)) == hipSuccess &&
              hipMalloc((void **)&p->items, items.size() * sizeof(Item)) == hipSuccess &&
              (!seated || hipMalloc((void **)&p->room_of, (size_t)N * sizeof(uint32_t)) == hipSuccess) &&
              (!seated || hipMalloc((void **)&p->slot_of, (size_t)N * sizeof(uint32_t)) == hipSuccess);
    if (!ok) {
        (void)hipGetLastError();
        release(p);
        g_err = "mixmatrix: no device memory for the matrices, the divisors and the room tables";
        return DSPFX_ERR_OOM;
    }
    ok = hipMemcpy(p->rooms, p->hrooms.data(), (size_t)G * sizeof(Room), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(p->items, items.data(), items.size() * sizeof(Item), hipMemcpyHostToDevice) == hipSuccess &&
         (!seated || hipMemcpy(p->room_of, p->hroom_of.data(), (size_t)N * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess) &&
         (!seated || hipMemcpy(p->seat_chan, p->hseat_chan.data(), p->hseat_chan.size() * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess) &&
         (!seated || hipMemcpy(p->slot_of, slots.data(), (size_t)N * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess) &&
         fill_rooms(p, 0, G, DSPFX_MIXMATRIX_MIX_MINUS, nullptr) == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
         hipEventCreateWithFlags(&p->ev, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        release(p);
        return DSPFX_ERR_HIP;
    }
    *out = p;
    return DSPFX_OK;
}

}  // namespace

extern "C" int dspfx_mixmatrix_create(const dspfx_mixmatrix_desc *desc, dspfx_mixmatrix **out) { return create_bank(desc, nullptr, false, out); }

extern "C" int dspfx_mixmatrix_create_seats(const dspfx_mixmatrix_desc *desc, const uint32_t *seats, dspfx_mixmatrix **out) {
    return create_bank(desc, seats, true, out);
}

extern "C" int dspfx_mixmatrix_reseat(uint32_t *room_of_io, uint32_t *seat_of_io, const uint32_t *seats, uint32_t n_groups, uint64_t n_channels,
                                      const uint32_t *room_ids, uint64_t first_channel, uint64_t count) {
    g_err.clear();
    if (!room_of_io || !seat_of_io || n_groups == 0 || n_channels == 0 || n_channels > 0xFFFFFF00ull) {
        g_err = "mixmatrix reseat: no tables, no rooms or no channels";
        return DSPFX_ERR_INVALID;
    }
    try {
        std::vector<uint32_t> S, off, chan, occ(n_groups, 0);
        const int rc = check_seats("mixmatrix reseat", seats, nullptr, n_groups, S, off, g_err);
        if (rc != DSPFX_OK) return rc;
        chan.assign((size_t)off[n_groups - 1] + S[n_groups - 1], NONE);
        for (uint64_t c = 0; c < n_channels; ++c) {
            const uint32_t g = room_of_io[c], q = seat_of_io[c];
            if (g == NONE) continue;
            if (g >= n_groups || q >= S[g] || chan[off[g] + q] != NONE) {
                char buf[160];
                std::snprintf(buf, sizeof buf, "mixmatrix reseat: channel %llu is in seat %u of room %u, which does not exist or is held twice", (unsigned long long)c, q, g);
                g_err = buf;
                return DSPFX_ERR_INVALID;
            }
            chan[off[g] + q] = (uint32_t)c;
            ++occ[g];
        }
        std::vector<Move> moves;
        return reseat(Seats{room_of_io, seat_of_io, chan.data(), occ.data(), S.data(), off.data(), n_groups, n_channels}, room_ids, first_channel, count, g_err, moves);
    } catch (const std::bad_alloc &) {
        g_err = "mixmatrix reseat: no host memory";
        return DSPFX_ERR_OOM;
    }
}

extern "C" int dspfx_mixmatrix_scatter(const uint32_t *room_of, const uint32_t *seat_of, const uint32_t *seats, uint32_t n_groups, uint64_t n_channels,
                                       uint64_t *chunks_out, uint64_t *lines_out) {
    g_err.clear();
    if (!room_of || !seat_of || n_groups == 0 || n_channels == 0 || n_channels > 0xFFFFFF00ull) {
        g_err = "mixmatrix scatter: no tables, no rooms or no channels";
        return DSPFX_ERR_INVALID;
    }
    try {
        std::vector<uint32_t> S, off, chan;
        const int rc = check_seats("mixmatrix scatter", seats, nullptr, n_groups, S, off, g_err);
        if (rc != DSPFX_OK) return rc;
        chan.assign((size_t)off[n_groups - 1] + S[n_groups - 1], NONE);
        for (uint64_t c = 0; c < n_channels; ++c) {
            const uint32_t g = room_of[c], q = seat_of[c];
            if (g == NONE) continue;
            if (g >= n_groups || q >= S[g] || chan[off[g] + q] != NONE) {
                char buf[160];
                std::snprintf(buf, sizeof buf, "mixmatrix scatter: channel %llu is in seat %u of room %u, which does not exist or is held twice", (unsigned long long)c, q, g);
                g_err = buf;
                return DSPFX_ERR_INVALID;
            }
            chan[off[g] + q] = (uint32_t)c;
        }
        // (every S_r is a multiple of 32, so a run of 32 entries of `chan` from a multiple of 32 is a run of 32 seats of one room:
        // a chunk of the direct run)
        uint64_t chunks = 0, lines = 0;
        uint32_t line[KC];
        for (size_t k0 = 0; k0 < chan.size(); k0 += KC) {
            uint32_t n = 0;
            for (uint32_t i = 0; i < KC; ++i)
                if (chan[k0 + i] != NONE) line[n++] = chan[k0 + i] / 32u;
            if (n == 0) continue;
            std::sort(line, line + n);
            ++chunks;
            lines += (uint64_t)(std::unique(line, line + n) - line);
        }
        if (chunks_out) *chunks_out = chunks;
        if (lines_out) *lines_out = lines;
    } catch (const std::bad_alloc &) {
        g_err = "mixmatrix scatter: no host memory";
        return DSPFX_ERR_OOM;
    }
    return DSPFX_OK;
}

extern "C" int dspfx_mixmatrix_staging_bytes(const uint64_t *group_start, uint32_t n_groups, uint64_t n_channels, uint32_t tile_channels, const uint32_t *seats,
                                             uint32_t max_frames, uint64_t *bytes_out) {
    uint64_t tables = 0;
    std::vector<uint32_t> edges;
    try {
        edges.resize(n_groups ? n_groups : 1);
    } catch (const std::bad_alloc &) {
        g_err = "mixmatrix: no host memory for the room tables";
        return DSPFX_ERR_OOM;
    }
    const int rc = plan(group_start, n_groups, n_channels, tile_channels, seats, true, nullptr, edges.data(), nullptr, &tables);
    if (rc != DSPFX_OK) return rc;
    if (max_frames == 0 || max_frames > (1u << 20)) {
        g_err = "mixmatrix: max_frames must be 1 .. 2^20";
        return DSPFX_ERR_INVALID;
    }
    uint64_t slots = 0;
    for (uint32_t g = 0; g < n_groups; ++g) slots += edges[g];
    if (bytes_out) *bytes_out = 2u * slots * max_frames * sizeof(float) + n_channels * sizeof(uint32_t);
    return DSPFX_OK;
}

extern "C" int dspfx_mixmatrix_set_staging(dspfx_mixmatrix *p, uint32_t mode) {
    if (!p) return DSPFX_ERR_INVALID;
    if (!p->seated) return p->fail(DSPFX_ERR_STATE, "mixmatrix set_staging: the bank has no seats (it was not made by dspfx_mixmatrix_create_seats)");
    if (mode != DSPFX_MIXMATRIX_DIRECT && mode != DSPFX_MIXMATRIX_STAGED)
        return p->fail(DSPFX_ERR_INVALID, "mixmatrix set_staging: the mode (DSPFX_MIXMATRIX_DIRECT and DSPFX_MIXMATRIX_STAGED are known)");
    std::lock_guard<std::mutex> lk(p->gmu);
    if (mode == DSPFX_MIXMATRIX_STAGED && !p->sbuf) {
        // on the caller's thread, as a slider store allocates a longer delay ring; kept until destroy, so no toggle frees what a run
        // in flight reads.  Not zeroed: a run reads only what its own stage_in and run kernels wrote
        if (hipSetDevice(p->desc.device) != hipSuccess ||
            hipMalloc((void **)&p->sbuf, 2u * (size_t)p->n_slots * p->desc.max_frames * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            p->sbuf = nullptr;
            return p->fail(DSPFX_ERR_OOM, "mixmatrix set_staging: no device memory for the seat-ordered copies (dspfx_mixmatrix_staging_bytes)");
        }
    }
    p->mode.store(mode, std::memory_order_release);
    return DSPFX_OK;
}

extern "C" int dspfx_mixmatrix_staging(dspfx_mixmatrix *p, uint32_t *mode_out) {
    if (!p) return DSPFX_ERR_INVALID;
    if (!mode_out) return p->fail(DSPFX_ERR_INVALID, "mixmatrix staging: no mode_out");
    *mode_out = p->mode.load(std::memory_order_acquire);
    return DSPFX_OK;
}

extern "C" int dspfx_mixmatrix_assign(dspfx_mixmatrix *p, const uint32_t *host_room_ids, uint64_t first_channel, uint64_t count, uint32_t preset) {
    if (!p) return DSPFX_ERR_INVALID;
    if (!p->seated) return p->fail(DSPFX_ERR_STATE, "mixmatrix assign: the bank has no seats (it was not made by dspfx_mixmatrix_create_seats)");
    if (preset != DSPFX_MIXMATRIX_MIX_MINUS && preset != DSPFX_MIXMATRIX_ZERO)
        return p->fail(DSPFX_ERR_INVALID, "mixmatrix assign: the preset (DSPFX_MIXMATRIX_MIX_MINUS and DSPFX_MIXMATRIX_ZERO are known)");
    std::lock_guard<std::mutex> lk(p->smu);
    const Seats t = p->seats();
    std::vector<Move> moves;
    std::string why;
    try {
        const int rc = reseat(t, host_room_ids, first_channel, count, why, moves);
        if (rc != DSPFX_OK) return p->fail(rc, why.c_str());
        if (moves.empty()) return DSPFX_OK;
        // what the device needs, by the seating after the call: who sits in every seat touched, the room of every mover, the seats
        // whose row and column change (emptied: +0.0; a newcomer's: the preset), and the rooms whose divisors change
        std::vector<uint32_t> w_seats, w_chans, w_lines, w_rooms;
        std::unordered_set<uint32_t> seen;
        const uint32_t bit = preset == DSPFX_MIXMATRIX_MIX_MINUS ? 0x80000000u : 0u;
        for (const Move &m : moves) {
            w_chans.insert(w_chans.end(), {m.c, m.r1});
            if (m.r0 != NONE) {
                const uint32_t at = t.off[m.r0] + m.q0;
                w_seats.insert(w_seats.end(), {at, t.seat_chan[at]});
                if (t.seat_chan[at] == NONE) w_lines.insert(w_lines.end(), {m.r0, m.q0});       // (taken again: the newcomer's line covers it)
                if (seen.insert(m.r0).second) w_rooms.push_back(m.r0);
            }
            if (m.r1 != NONE) {
                w_seats.insert(w_seats.end(), {t.off[m.r1] + m.q1, m.c});
                w_lines.insert(w_lines.end(), {m.r1, m.q1 | bit});
                if (seen.insert(m.r1).second) w_rooms.push_back(m.r1);
            }
        }
        int64_t gone = 0;
        for (const Move &m : moves) gone += (m.r1 == NONE) - (m.r0 == NONE);
        Store st;
        st.kind = ASSIGN;
        st.preset = preset;
        st.n_seats = w_seats.size() / 2;
        st.n_chans = w_chans.size() / 2;
        st.n_lines = w_lines.size() / 2;
        st.n_rooms = w_rooms.size();
        st.roomless = (uint64_t)((int64_t)p->hroomless + gone);
        const size_t words = w_seats.size() + w_chans.size() + w_lines.size() + w_rooms.size();
        if (!p->stores.staging(p->desc.device, words, st)) {
            unseat(t, moves);
            return p->fail(DSPFX_ERR_OOM, "mixmatrix assign: no page-locked memory for the staged seats");
        }
        uint32_t *w = (uint32_t *)st.vals;
        for (const std::vector<uint32_t> *v : {&w_seats, &w_chans, &w_lines, &w_rooms}) {
            std::memcpy(w, v->data(), v->size() * sizeof(uint32_t));
            w += v->size();
        }
        p->hroomless = st.roomless;
        p->stores.push(st);
    } catch (const std::bad_alloc &) {
        if (!moves.empty()) unseat(t, moves);
        return p->fail(DSPFX_ERR_OOM, "mixmatrix assign: no host memory");
    }
    return DSPFX_OK;
}

extern "C" int dspfx_mixmatrix_set_pairs(dspfx_mixmatrix *p, const uint32_t *listeners, const uint32_t *sources, const float *gains, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    if (!listeners || !sources || !gains) return p->fail(DSPFX_ERR_INVALID, "mixmatrix set_pairs: no listeners, sources or gains");
    if (count == 0) return DSPFX_OK;
    char buf[192];
    std::lock_guard<std::mutex> lk(p->smu);
    try {
        std::vector<uint32_t> words, rooms;
        std::unordered_map<uint64_t, size_t> at;         // (room, listener, source) -> its triple: a later duplicate takes its place
        std::unordered_set<uint32_t> seen;
        const uint32_t N = p->desc.n_channels;
        for (uint64_t i = 0; i < count; ++i) {
            uint32_t rl = NONE, rs = NONE, il = 0, is = 0;
            if (listeners[i] < N) place_of(p, listeners[i], rl, il);
            if (sources[i] < N) place_of(p, sources[i], rs, is);
            if (rl == NONE || rl != rs) {
                std::snprintf(buf, sizeof buf, "mixmatrix set_pairs: pair %llu: listener %u and source %u are not two channels of one room",
                              (unsigned long long)i, listeners[i], sources[i]);
                return p->fail(DSPFX_ERR_INVALID, buf);
            }
            uint32_t g;
            std::memcpy(&g, &gains[i], sizeof g);
            const auto ins = at.emplace((uint64_t)rl << 20 | (uint64_t)il << 10 | is, words.size());
            if (ins.second) words.insert(words.end(), {rl, il << 16 | is, g});
            else words[ins.first->second + 2] = g;
            if (seen.insert(rl).second) rooms.push_back(rl);
        }
        Store st;
        st.kind = PAIRS;
        st.n_lines = words.size() / 3;
        st.n_rooms = rooms.size();
        if (!p->stores.staging(p->desc.device, words.size() + rooms.size(), st))
            return p->fail(DSPFX_ERR_OOM, "mixmatrix set_pairs: no page-locked memory for the staged values");
        std::memcpy(st.vals, words.data(), words.size() * sizeof(uint32_t));
        std::memcpy(st.vals + words.size(), rooms.data(), rooms.size() * sizeof(uint32_t));
        p->stores.push(st);
    } catch (const std::bad_alloc &) {
        return p->fail(DSPFX_ERR_OOM, "mixmatrix set_pairs: no host memory");
    }
    return DSPFX_OK;
}

extern "C" int dspfx_mixmatrix_rooms(dspfx_mixmatrix *p, uint32_t *host_ids_out, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const uint64_t N = p->desc.n_channels;
    if (!host_ids_out || first_channel > N || count > N - first_channel) return p->fail(DSPFX_ERR_INVALID, "mixmatrix rooms: the array or the range");
    std::lock_guard<std::mutex> lk(p->smu);
    for (uint64_t i = 0; i < count; ++i) {
        uint32_t index;
        place_of(p, (uint32_t)(first_channel + i), host_ids_out[i], index);
    }
    return DSPFX_OK;
}

extern "C" int dspfx_mixmatrix_seats(dspfx_mixmatrix *p, uint32_t *host_seats_out, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const uint64_t N = p->desc.n_channels;
    if (!host_seats_out || first_channel > N || count > N - first_channel) return p->fail(DSPFX_ERR_INVALID, "mixmatrix seats: the array or the range");
    std::lock_guard<std::mutex> lk(p->smu);
    for (uint64_t i = 0; i < count; ++i) {
        uint32_t room;
        place_of(p, (uint32_t)(first_channel + i), room, host_seats_out[i]);
    }
    return DSPFX_OK;
}

extern "C" int dspfx_mixmatrix_occupancy(dspfx_mixmatrix *p, uint32_t *host_counts_out) {
    if (!p) return DSPFX_ERR_INVALID;
    if (!host_counts_out) return p->fail(DSPFX_ERR_INVALID, "mixmatrix occupancy: no array");
    std::lock_guard<std::mutex> lk(p->smu);
    for (uint32_t g = 0; g < p->desc.n_groups; ++g) host_counts_out[g] = p->occ[g];
    return DSPFX_OK;
}

extern "C" int dspfx_mixmatrix_destroy(dspfx_mixmatrix *p) { return destroy_bank(p, release); }

extern "C" int dspfx_mixmatrix_set_rows(dspfx_mixmatrix *p, const float *host_values, uint32_t row_len, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    return store_lines(p, ROWS, host_values, row_len, first_channel, count);
}

extern "C" int dspfx_mixmatrix_set_cols(dspfx_mixmatrix *p, const float *host_values, uint32_t row_len, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    return store_lines(p, COLS, host_values, row_len, first_channel, count);
}

extern "C" int dspfx_mixmatrix_fill(dspfx_mixmatrix *p, int64_t room, uint32_t preset) {
    if (!p) return DSPFX_ERR_INVALID;
    char buf[128];
    const uint32_t G = p->desc.n_groups;
    if (preset != DSPFX_MIXMATRIX_MIX_MINUS && preset != DSPFX_MIXMATRIX_ZERO) {
        std::snprintf(buf, sizeof buf, "mixmatrix fill: preset %u (DSPFX_MIXMATRIX_MIX_MINUS and DSPFX_MIXMATRIX_ZERO are known)", preset);
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    if (room < -1 || room >= (int64_t)G) {
        std::snprintf(buf, sizeof buf, "mixmatrix fill: room %lld, and the bank has %u (-1: every room)", (long long)room, G);
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    Store st;
    st.kind = FILL;
    st.room = room < 0 ? 0u : (uint32_t)room;
    st.count = room < 0 ? G : 1u;
    st.preset = preset;
    p->stores.push(st);
    return DSPFX_OK;
}

extern "C" int dspfx_mixmatrix_reset(dspfx_mixmatrix *p) { return dspfx_mixmatrix_fill(p, -1, DSPFX_MIXMATRIX_MIX_MINUS); }

namespace {

// what the two runs share, under mu: the argument checks (`what`: "run" or "run_sparse"), the stream order, the queued stores onto
// the stream, and the kernels' arguments.  The mode is read once: a run is wholly one mode, the one of the last set_staging that
// returned before it
int begin_run(dspfx_mixmatrix *p, const char *what, const float *block, uint32_t n_frames, float *out, hipStream_t s, bool &staged, RunArgs &a) {
    const std::string pre = std::string("mixmatrix ") + what + ": ";
    if (!block || !out || n_frames == 0 || n_frames > p->desc.max_frames) return p->fail(DSPFX_ERR_INVALID, (pre + "block, out or n_frames").c_str());
    const uintptr_t bytes = (uintptr_t)p->desc.n_channels * n_frames * sizeof(float), b0 = (uintptr_t)block, o0 = (uintptr_t)out;
    staged = p->mode.load(std::memory_order_acquire) == DSPFX_MIXMATRIX_STAGED;
    if (b0 < o0 + bytes && o0 < b0 + bytes) {
        if (!staged)
            return p->fail(DSPFX_ERR_INVALID, (pre + "out overlaps the block (every listener reads every source of its room: no in-place form)").c_str());
        // staged: every read of the block is over before stage_out writes the first sample, so out == block is in place
        if (b0 != o0) return p->fail(DSPFX_ERR_INVALID, (pre + "out overlaps the block in part (a staged run takes out == block, or no overlap)").c_str());
    }
    BANK_HIP_WHY(hipSetDevice(p->desc.device), "hipSetDevice");
    BANK_HIP_WHY(order(p, s), "stream order");
    BANK_HIP_WHY(p->stores.drain(s, [p](const Store &st, hipStream_t on) { return apply_store(p, st, on); }), "matrix store");
    a.in = block;
    a.out = out;
    a.tab = p->tab;
    a.div = p->div;
    a.rooms = p->rooms;
    a.items = p->items;
    a.N = p->desc.n_channels;
    a.W = p->desc.tile_channels;
    a.nf = n_frames;
    a.normalise = p->desc.normalise;
    a.seat_chan = p->seat_chan;
    a.sin = p->sbuf;
    a.sout = p->sbuf ? p->sbuf + (size_t)p->n_slots * p->desc.max_frames : nullptr;
    a.MF = p->desc.max_frames;
    return DSPFX_OK;
}

}  // namespace

extern "C" int dspfx_mixmatrix_run_sparse(dspfx_mixmatrix *p, const float *block, uint32_t n_frames, float *out, const int32_t *list, uint64_t list_len,
                                          const uint32_t *start, const uint32_t *count, void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    if (!list || !start || !count) return p->fail(DSPFX_ERR_INVALID, "mixmatrix run_sparse: list, start or count");
    if (list_len > 0xFFFFFFFFull) return p->fail(DSPFX_ERR_INVALID, "mixmatrix run_sparse: list_len is above 2^32 - 1");
    hipStream_t s = (hipStream_t)stream;
    bool staged = false;
    SparseArgs sa;
    const int rc = begin_run(p, "run_sparse", block, n_frames, out, s, staged, sa.r);
    if (rc != DSPFX_OK) return rc;
    sa.list = list;
    sa.start = start;
    sa.count = count;
    sa.list_len = list_len;
    sa.room_of = p->room_of;
    sa.slot_of = p->slot_of;
    const dim3 grid(p->n_items, (n_frames + FT - 1) / FT);
    if (staged) {                                // the listed sources straight from the block, the seat-ordered result, sout -> out
        mixmatrix_run_sparse<true, true><<<grid, WG, 0, s>>>(sa);
        BANK_HIP_WHY(hipGetLastError(), "mixmatrix_run_sparse_staged");
        mixmatrix_stage_out<<<dim3((sa.r.N + SG - 1) / SG, grid.y), WG, 0, s>>>(sa.r.sout, out, p->slot_of, sa.r.N, sa.r.W, n_frames, sa.r.MF);
        BANK_HIP_WHY(hipGetLastError(), "mixmatrix_stage_out");
        return DSPFX_OK;
    }
    if (p->roomless) {
        mixmatrix_zero_roomless<<<(sa.r.N + WG - 1) / WG, WG, 0, s>>>(out, p->room_of, sa.r.N, sa.r.W, n_frames);
        BANK_HIP_WHY(hipGetLastError(), "mixmatrix_zero_roomless");
    }
    const auto kernel = p->seated ? mixmatrix_run_sparse<true> : mixmatrix_run_sparse<false>;
    kernel<<<grid, WG, 0, s>>>(sa);
    BANK_HIP_WHY(hipGetLastError(), p->seated ? "mixmatrix_run_sparse_seated" : "mixmatrix_run_sparse");
    return DSPFX_OK;
}

extern "C" int dspfx_mixmatrix_run(dspfx_mixmatrix *p, const float *block, uint32_t n_frames, float *out, void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    hipStream_t s = (hipStream_t)stream;
    bool staged = false;
    RunArgs a;
    const int rc = begin_run(p, "run", block, n_frames, out, s, staged, a);
    if (rc != DSPFX_OK) return rc;
    if (staged) {                               // block -> sin, the chain over the seats, sout -> out: all three behind the stores
        const dim3 tg((a.N + SG - 1) / SG, (n_frames + FT - 1) / FT);
        mixmatrix_stage_in<<<tg, WG, 0, s>>>(block, p->sbuf, p->slot_of, a.N, a.W, n_frames, a.MF);
        BANK_HIP_WHY(hipGetLastError(), "mixmatrix_stage_in");
        mixmatrix_run<true, true><<<dim3(p->n_items, tg.y), WG, 0, s>>>(a);
        BANK_HIP_WHY(hipGetLastError(), "mixmatrix_run_staged");
        mixmatrix_stage_out<<<tg, WG, 0, s>>>(a.sout, out, p->slot_of, a.N, a.W, n_frames, a.MF);
        BANK_HIP_WHY(hipGetLastError(), "mixmatrix_stage_out");
        return DSPFX_OK;
    }
    if (p->roomless) {                           // (a seated bank's: the other has nobody without a room)
        mixmatrix_zero_roomless<<<(a.N + WG - 1) / WG, WG, 0, s>>>(out, p->room_of, a.N, a.W, n_frames);
        BANK_HIP_WHY(hipGetLastError(), "mixmatrix_zero_roomless");
    }
    const auto kernel = p->seated ? mixmatrix_run<true> : mixmatrix_run<false>;
    kernel<<<dim3(p->n_items, (n_frames + FT - 1) / FT), WG, 0, s>>>(a);
    BANK_HIP_WHY(hipGetLastError(), p->seated ? "mixmatrix_run_seated" : "mixmatrix_run");
    return DSPFX_OK;
}
