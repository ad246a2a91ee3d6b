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
// Stores (dspfx_mixmatrix_set_rows / _set_cols / _fill / _reset) follow the mix-group bank's fader stores: validated, staged in
// page-locked memory, queued under the queue's own lock, and put on the next run's stream ahead of its kernel in the order they were
// made: a copy, a scatter into the source-major table, and a recount of w and d for the listeners touched -- d is computed on the
// device with dspfx_link_divisor's own f32 expression, so no store waits for the device.
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

struct RunArgs {
    const float *__restrict__ in;
    float *__restrict__ out;
    const float *__restrict__ tab;
    const float *__restrict__ div;       // [N]: the listener's divisor; 0.0: no wired entry, the output is +0.0
    const Room *__restrict__ rooms;
    const Item *__restrict__ items;
    uint32_t N, W, nf, normalise;
};

__global__ __launch_bounds__(WG, 3) void mixmatrix_run(RunArgs a) {
    __shared__ float xs[FT * XS];                        // [frame][source of the chunk]
    const Item it = a.items[blockIdx.x];
    const Room rm = a.rooms[it.room];
    const uint32_t n = rm.n, P = edge(n), c0 = rm.c0;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t r = lane & 31u, h = lane >> 5;        // MFMA operand maps: A[i = r][k = h], B[k = h][j = r]
    const uint32_t lt = it.l0 + (uint32_t)__builtin_amdgcn_readfirstlane((int)wave) * 32u;     // the wave's listener tile (uniform)
    const bool active = lt < P;                          // wave-uniform; an idle wave still stages its share of x
    const uint32_t ss = tid & 31u, sf = tid >> 5;        // staging: source ss of the chunk, frames sf + 8 i
    const size_t rs = a.W ? a.W : a.N;                   // a frame further is rs elements on in either layout

    // (the frame pass is a grid dimension and not a loop here: a loop would have the compiler keep every row's offset live across it)
    const uint32_t f0 = blockIdx.y * FT;
    {
        f32x16 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
        float st[16], bn[KC / 2];
        // the chunk from source k0 into registers: samples outside the room or the block are +0.0 and are not read
        // the frames of the pass this thread stages: sf + 8 i for i < nst (a running pointer and one count: no offset per row is kept)
        const uint32_t left = a.nf - f0, nst = left > sf ? (left - sf + 7u) / 8u : 0u;
        const float *tabr = a.tab + rm.off;              // uniform; the table has P * P <= 2^20 elements: 32-bit offsets
        const uint32_t bcol = (active ? lt + r : 0u) + h * P;
        auto gload = [&](uint32_t k0) {
            const uint32_t s = k0 + ss;
            const float *p = a.in + lay(0, c0 + (s < n ? s : 0u), a.nf, a.N, a.W) + (size_t)(f0 + sf) * rs;
            const uint32_t cnt = s < n ? nst : 0u;
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
            __syncthreads();                             // the chunk before is read
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) xs[(sf + 8u * i) * XS + ss] = st[i];
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
        const uint32_t l = lt + r;
        if (active && l < n) {
            const uint32_t c = c0 + l;
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
}

// a preset into the tables of rooms [first_room, first_room + gridDim.x): one workgroup per room, the padding zero
__global__ __launch_bounds__(WG) void mixmatrix_fill(float *__restrict__ tab, const Room *__restrict__ rooms, uint32_t first_room, uint32_t preset) {
    const Room rm = rooms[first_room + blockIdx.x];
    const uint32_t n = rm.n, P = edge(n);
    float *t = tab + rm.off;
    for (uint32_t e = threadIdx.x; e < P * P; e += WG) {
        const uint32_t s = e / P, l = e - s * P;
        t[e] = (preset == DSPFX_MIXMATRIX_MIX_MINUS && s < n && l < n && s != l) ? 1.0f : 0.0f;
    }
}

// staged values [count][n] into the room's source-major table: cols = 0: row i is what listener l0 + i hears, vals[i][s] -> Mt[s][l0 + i];
// cols = 1: row i is how loud source l0 + i is for each listener, vals[i][l] -> Mt[l0 + i][l]
__global__ __launch_bounds__(WG) void mixmatrix_store(float *__restrict__ tab, const float *__restrict__ vals, uint64_t off, uint32_t n, uint32_t l0,
                                                      uint32_t count, uint32_t cols) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    if (e >= count * n) return;
    const uint32_t i = e / n, j = e - i * n, P = edge(n);
    float *t = tab + off;
    if (cols) t[(size_t)(l0 + i) * P + j] = vals[e];
    else t[(size_t)j * P + l0 + i] = vals[e];
}

// w and d of listeners [first, first + count): w = the entries of the listener's row that are not +-0.0; d = dspfx_link_divisor(w) by
// its own f32 expression (node.rs:166,179: sequential f32 increments from 0.0001), 0.0 for a row without a wired entry
__global__ __launch_bounds__(WG) void mixmatrix_recount(const float *__restrict__ tab, const Room *__restrict__ rooms, const uint32_t *__restrict__ room_of,
                                                        float *__restrict__ div, uint32_t first, uint32_t count) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= count) return;
    const uint32_t c = first + i;
    const Room rm = rooms[room_of[c]];
    const uint32_t n = rm.n, P = edge(n), l = c - rm.c0;
    const float *t = tab + rm.off + l;
    uint32_t w = 0;
    for (uint32_t s = 0; s < n; ++s) w += t[(size_t)s * P] != 0.0f;
    float d = 0.0f;
    if (w) {
        d = 0.0001f;
        for (uint32_t k = 0; k < w; ++k) d = d + 1.0f;   // (w <= 1024: never saturates)
    }
    div[c] = d;
}

thread_local std::string g_err;        // the reason of the last failed create or plan on this thread

struct Store {
    int kind = 0;                // 0: rows, 1: columns, 2: fill
    float *vals = nullptr;       // page-locked, [count][n]; fill: none
    size_t cap = 0;              // floats
    uint32_t room = 0, l0 = 0, count = 0;        // rows / columns: room-local first index and count; fill: rooms [room, room + count)
    uint32_t preset = 0;
    hipEvent_t ev = nullptr;
};

int check_table(const uint64_t *gs, uint32_t G, uint64_t N, uint32_t W, std::string &err) {
    char buf[192];
    if (!gs || G == 0) {
        err = "mixmatrix: no group table";
        return DSPFX_ERR_INVALID;
    }
    if (N == 0 || N > 0xFFFFFF00ull) {
        err = "mixmatrix: n_channels must be 1 .. 2^32 - 256";
        return DSPFX_ERR_INVALID;
    }
    if (W && (!pow2(W) || N % W)) {
        std::snprintf(buf, sizeof buf, "mixmatrix: tile_channels %u is not a power of two that divides n_channels %llu", W, (unsigned long long)N);
        err = buf;
        return DSPFX_ERR_INVALID;
    }
    if (gs[0] != 0) {
        std::snprintf(buf, sizeof buf, "mixmatrix: group_start[0] is %llu, not 0", (unsigned long long)gs[0]);
        err = buf;
        return DSPFX_ERR_INVALID;
    }
    for (uint32_t g = 0; g < G; ++g) {
        if (gs[g + 1] < gs[g]) {
            std::snprintf(buf, sizeof buf, "mixmatrix: group_start decreases at entry %u (%llu after %llu)", g + 1, (unsigned long long)gs[g + 1],
                          (unsigned long long)gs[g]);
            err = buf;
            return DSPFX_ERR_INVALID;
        }
        const uint64_t n = gs[g + 1] - gs[g];
        if (n == 0) {
            std::snprintf(buf, sizeof buf, "mixmatrix: room %u is empty (a room has 1 .. %u members)", g, MAXN);
            err = buf;
            return DSPFX_ERR_INVALID;
        }
        if (n > MAXN) {
            std::snprintf(buf, sizeof buf, "mixmatrix: room %u has %llu members, above DSPFX_MIXMATRIX_MAX_ROOM = %u", g, (unsigned long long)n, MAXN);
            err = buf;
            return DSPFX_ERR_INVALID;
        }
    }
    if (gs[G] != N) {
        std::snprintf(buf, sizeof buf, "mixmatrix: group_start[%u] is %llu, not n_channels %llu", G, (unsigned long long)gs[G], (unsigned long long)N);
        err = buf;
        return DSPFX_ERR_INVALID;
    }
    return DSPFX_OK;
}

}  // namespace

struct dspfx_mixmatrix {
    dspfx_mixmatrix_desc desc{};
    std::vector<uint64_t> gs;                    // the table, [G + 1]
    std::vector<Room> hrooms;
    std::mutex mu;                               // run / destroy
    std::mutex qmu;                              // the store queue, the free staging buffers
    std::mutex emu;                              // err
    std::deque<Store> queue;                     // stores not yet handed to a stream
    std::vector<Store> spare;                    // staging buffers free for the next store
    std::vector<Store> flying;                   // copies queued on a stream (mu)
    std::vector<hipEvent_t> events;              // spare events (mu)
    float *tab = nullptr, *div = nullptr, *stage = nullptr;      // stage: [maxn][maxn], where a drained store's values land
    Room *rooms = nullptr;
    Item *items = nullptr;
    uint32_t *room_of = nullptr;
    uint32_t n_items = 0, maxn = 0;
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;
    bool used = false;
    std::string err;
};

namespace {

void release(dspfx_mixmatrix *p) {
    (void)hipSetDevice(p->desc.device);
    for (void *d : {(void *)p->tab, (void *)p->div, (void *)p->stage, (void *)p->rooms, (void *)p->items, (void *)p->room_of})
        if (d) (void)hipFree(d);
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

int fail(dspfx_mixmatrix *p, int rc, const char *what) {
    std::lock_guard<std::mutex> lk(p->emu);
    p->err = what;
    return rc;
}

hipError_t recount(dspfx_mixmatrix *p, uint32_t first, uint32_t count, hipStream_t s) {
    mixmatrix_recount<<<(count + WG - 1) / WG, WG, 0, s>>>(p->tab, p->rooms, p->room_of, p->div, first, count);
    return hipGetLastError();
}

hipError_t fill_rooms(dspfx_mixmatrix *p, uint32_t first_room, uint32_t count, uint32_t preset, hipStream_t s) {
    mixmatrix_fill<<<count, WG, 0, s>>>(p->tab, p->rooms, first_room, preset);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const uint32_t c0 = (uint32_t)p->gs[first_room], c1 = (uint32_t)p->gs[first_room + count];
    return recount(p, c0, c1 - c0, s);
}

// the stores made so far, in order, onto the stream ahead of the run; staging buffers whose copy is done go back
hipError_t apply_stores(dspfx_mixmatrix *p, hipStream_t s) {
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
        if (st.kind == 2) {
            err = fill_rooms(p, st.room, st.count, st.preset, s);
            continue;
        }
        const Room &rm = p->hrooms[st.room];
        const uint32_t cells = st.count * rm.n;
        err = hipMemcpyAsync(p->stage, st.vals, (size_t)cells * sizeof(float), hipMemcpyHostToDevice, s);
        if (err == hipSuccess) {
            mixmatrix_store<<<(cells + WG - 1) / WG, WG, 0, s>>>(p->tab, p->stage, rm.off, rm.n, st.l0, st.count, (uint32_t)st.kind);
            err = hipGetLastError();
        }
        // a row store changes the wired count of its listeners, a column store that of every listener of the room
        if (err == hipSuccess) err = st.kind == 0 ? recount(p, rm.c0 + st.l0, st.count, s) : recount(p, rm.c0, rm.n, s);
        if (err == hipSuccess) {
            if (p->events.empty()) {
                err = hipEventCreateWithFlags(&st.ev, hipEventDisableTiming);
            } else {
                st.ev = p->events.back();
                p->events.pop_back();
            }
        }
        if (err == hipSuccess) err = hipEventRecord(st.ev, s);
        if (st.ev) {
            p->flying.push_back(st);
        } else {                                 // no event to tell when the copy is done: wait, then the buffer is free
            (void)hipStreamSynchronize(s);
            (void)hipHostFree(st.vals);
        }
    }
    return err;
}

// a staging buffer of at least `floats`, from the spare ones or new; nullptr: none to be had
float *staging(dspfx_mixmatrix *p, size_t floats, size_t *cap) {
    {
        std::lock_guard<std::mutex> lk(p->qmu);
        for (size_t i = 0; i < p->spare.size(); ++i)
            if (p->spare[i].cap >= floats) {
                float *v = p->spare[i].vals;
                *cap = p->spare[i].cap;
                p->spare[i] = p->spare.back();
                p->spare.pop_back();
                return v;
            }
    }
    float *v = nullptr;
    if (hipSetDevice(p->desc.device) != hipSuccess) return nullptr;
    if (hipHostMalloc((void **)&v, floats * sizeof(float), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    *cap = floats;
    return v;
}

// rows or columns [first, first + count) of one room, row_len values each
int store_lines(dspfx_mixmatrix *p, int kind, const float *vals, uint32_t row_len, uint64_t first, uint64_t count) {
    const char *what = kind ? "set_cols" : "set_rows";
    char buf[224];
    const uint64_t N = p->desc.n_channels;
    if (!vals) {
        std::snprintf(buf, sizeof buf, "mixmatrix %s: no values", what);
        return fail(p, DSPFX_ERR_INVALID, buf);
    }
    if (first >= N || count > N - first) {
        std::snprintf(buf, sizeof buf, "mixmatrix %s: channels [%llu, %llu + %llu) are not inside the bank's %llu", what, (unsigned long long)first,
                      (unsigned long long)first, (unsigned long long)count, (unsigned long long)N);
        return fail(p, DSPFX_ERR_INVALID, buf);
    }
    const uint32_t room = (uint32_t)(std::upper_bound(p->gs.begin(), p->gs.end(), first) - p->gs.begin()) - 1;
    const Room &rm = p->hrooms[room];
    if (first + count > (uint64_t)rm.c0 + rm.n) {
        std::snprintf(buf, sizeof buf, "mixmatrix %s: channels [%llu, %llu + %llu) are not in one room (room %u is [%u, %u))", what,
                      (unsigned long long)first, (unsigned long long)first, (unsigned long long)count, room, rm.c0, rm.c0 + rm.n);
        return fail(p, DSPFX_ERR_INVALID, buf);
    }
    if (row_len != rm.n) {
        std::snprintf(buf, sizeof buf, "mixmatrix %s: a row of %u values, and room %u has %u members", what, row_len, room, rm.n);
        return fail(p, DSPFX_ERR_INVALID, buf);
    }
    if (count == 0) return DSPFX_OK;
    Store st;
    st.kind = kind;
    st.room = room;
    st.l0 = (uint32_t)first - rm.c0;
    st.count = (uint32_t)count;
    const size_t cells = (size_t)count * rm.n;
    st.vals = staging(p, cells, &st.cap);
    if (!st.vals) {
        std::snprintf(buf, sizeof buf, "mixmatrix %s: no page-locked memory for the staged values", what);
        return fail(p, DSPFX_ERR_OOM, buf);
    }
    std::memcpy(st.vals, vals, cells * sizeof(float));
    std::lock_guard<std::mutex> lk(p->qmu);
    p->queue.push_back(st);
    return DSPFX_OK;
}

}  // namespace

#define MM_HIP(call, what)                                             \
    do {                                                               \
        if ((call) != hipSuccess) return fail(p, DSPFX_ERR_HIP, what); \
    } while (0)

extern "C" const char *dspfx_mixmatrix_last_error(const dspfx_mixmatrix *p) { return p ? p->err.c_str() : g_err.c_str(); }

extern "C" int dspfx_mixmatrix_plan(const uint64_t *group_start, uint32_t n_groups, uint64_t n_channels, uint32_t tile_channels,
                                    uint32_t *count_out, uint32_t *edge_out, uint64_t *offset_out, uint64_t *total_bytes_out) {
    g_err.clear();
    const int rc = check_table(group_start, n_groups, n_channels, tile_channels, g_err);
    if (rc != DSPFX_OK) return rc;
    uint64_t off = 0;
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t n = (uint32_t)(group_start[g + 1] - group_start[g]), P = edge(n);
        if (count_out) count_out[g] = n;
        if (edge_out) edge_out[g] = P;
        if (offset_out) offset_out[g] = off;
        off += (uint64_t)P * P;
    }
    if (total_bytes_out) *total_bytes_out = off * sizeof(float);
    return DSPFX_OK;
}

extern "C" int dspfx_mixmatrix_create(const dspfx_mixmatrix_desc *desc, dspfx_mixmatrix **out) {
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
    std::vector<uint32_t> cnt, room_of;
    std::vector<uint64_t> offs;
    std::vector<Item> items;
    dspfx_mixmatrix *p = nullptr;
    try {
        cnt.resize(G ? G : 1);
        offs.resize(G ? G : 1);
        const int rc = dspfx_mixmatrix_plan(desc->group_start, G, N, desc->tile_channels, cnt.data(), nullptr, offs.data(), &total_bytes);
        if (rc != DSPFX_OK) return rc;
        if ((uint64_t)N * desc->max_frames > (1ull << 40)) {
            g_err = "mixmatrix: n_channels x max_frames is too large";
            return DSPFX_ERR_INVALID;
        }
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return DSPFX_ERR_NO_DEVICE;
        if (desc->device < 0 || desc->device >= count) {
            g_err = "mixmatrix: no such device";
            return DSPFX_ERR_INVALID;
        }
        if (hipSetDevice(desc->device) != hipSuccess) return DSPFX_ERR_HIP;
        p = new dspfx_mixmatrix;
        p->desc = *desc;
        p->gs.assign(desc->group_start, desc->group_start + G + 1);
        p->desc.group_start = nullptr;
        p->hrooms.resize(G);
        room_of.resize(N);
        for (uint32_t g = 0; g < G; ++g) {
            p->hrooms[g] = Room{offs[g], (uint32_t)p->gs[g], cnt[g]};
            p->maxn = std::max(p->maxn, cnt[g]);
            for (uint32_t l0 = 0; l0 < edge(cnt[g]); l0 += LT) items.push_back(Item{g, l0});
            std::fill(room_of.begin() + p->gs[g], room_of.begin() + p->gs[g + 1], g);
        }
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
              hipMalloc((void **)&p->stage, (size_t)p->maxn * p->maxn * sizeof(float)) == hipSuccess &&
              hipMalloc((void **)&p->rooms, (size_t)G * sizeof(Room)) == hipSuccess &&
              hipMalloc((void **)&p->items, items.size() * sizeof(Item)) == hipSuccess &&
              hipMalloc((void **)&p->room_of, (size_t)N * sizeof(uint32_t)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        release(p);
        g_err = "mixmatrix: no device memory for the matrices, the divisors and the room tables";
        return DSPFX_ERR_OOM;
    }
    ok = hipMemcpy(p->rooms, p->hrooms.data(), (size_t)G * sizeof(Room), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(p->items, items.data(), items.size() * sizeof(Item), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(p->room_of, room_of.data(), (size_t)N * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess &&
         fill_rooms(p, 0, G, DSPFX_MIXMATRIX_MIX_MINUS, nullptr) == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
         hipEventCreateWithFlags(&p->ev, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        release(p);
        return DSPFX_ERR_HIP;
    }
    *out = p;
    return DSPFX_OK;
}

extern "C" int dspfx_mixmatrix_destroy(dspfx_mixmatrix *p) {
    if (!p) return DSPFX_ERR_INVALID;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        (void)hipSetDevice(p->desc.device);
        if (p->used) (void)hipStreamSynchronize(p->last);    // the bank's work is ordered on the last stream it used
    }
    release(p);
    return DSPFX_OK;
}

extern "C" int dspfx_mixmatrix_set_rows(dspfx_mixmatrix *p, const float *host_values, uint32_t row_len, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    return store_lines(p, 0, host_values, row_len, first_channel, count);
}

extern "C" int dspfx_mixmatrix_set_cols(dspfx_mixmatrix *p, const float *host_values, uint32_t row_len, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    return store_lines(p, 1, host_values, row_len, first_channel, count);
}

extern "C" int dspfx_mixmatrix_fill(dspfx_mixmatrix *p, int64_t room, uint32_t preset) {
    if (!p) return DSPFX_ERR_INVALID;
    char buf[128];
    const uint32_t G = p->desc.n_groups;
    if (preset != DSPFX_MIXMATRIX_MIX_MINUS && preset != DSPFX_MIXMATRIX_ZERO) {
        std::snprintf(buf, sizeof buf, "mixmatrix fill: preset %u (DSPFX_MIXMATRIX_MIX_MINUS and DSPFX_MIXMATRIX_ZERO are known)", preset);
        return fail(p, DSPFX_ERR_INVALID, buf);
    }
    if (room < -1 || room >= (int64_t)G) {
        std::snprintf(buf, sizeof buf, "mixmatrix fill: room %lld, and the bank has %u (-1: every room)", (long long)room, G);
        return fail(p, DSPFX_ERR_INVALID, buf);
    }
    Store st;
    st.kind = 2;
    st.room = room < 0 ? 0u : (uint32_t)room;
    st.count = room < 0 ? G : 1u;
    st.preset = preset;
    std::lock_guard<std::mutex> lk(p->qmu);
    p->queue.push_back(st);
    return DSPFX_OK;
}

extern "C" int dspfx_mixmatrix_reset(dspfx_mixmatrix *p) { return dspfx_mixmatrix_fill(p, -1, DSPFX_MIXMATRIX_MIX_MINUS); }

extern "C" int dspfx_mixmatrix_run(dspfx_mixmatrix *p, const float *block, uint32_t n_frames, float *out, void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    if (!block || !out || n_frames == 0 || n_frames > p->desc.max_frames) return fail(p, DSPFX_ERR_INVALID, "mixmatrix run: block, out or n_frames");
    const uintptr_t bytes = (uintptr_t)p->desc.n_channels * n_frames * sizeof(float), b0 = (uintptr_t)block, o0 = (uintptr_t)out;
    if (b0 < o0 + bytes && o0 < b0 + bytes)
        return fail(p, DSPFX_ERR_INVALID, "mixmatrix run: out overlaps the block (every listener reads every source of its room: no in-place form)");
    hipStream_t s = (hipStream_t)stream;
    MM_HIP(hipSetDevice(p->desc.device), "hipSetDevice");
    MM_HIP(order(p, s), "stream order");
    MM_HIP(apply_stores(p, s), "matrix store");
    RunArgs a;
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
    mixmatrix_run<<<dim3(p->n_items, (n_frames + FT - 1) / FT), WG, 0, s>>>(a);
    MM_HIP(hipGetLastError(), "mixmatrix_run");
    return DSPFX_OK;
}
