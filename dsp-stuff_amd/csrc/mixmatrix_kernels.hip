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

// a store's vals: [count][n]; a fill has none
struct StoreFields {
    int kind = 0;                // 0: rows, 1: columns, 2: fill
    uint32_t room = 0, l0 = 0, count = 0;        // rows / columns: room-local first index and count; fill: rooms [room, room + count)
    uint32_t preset = 0;
};
typedef StoreQueue<StoreFields> Stores;
typedef Stores::Store Store;

}  // namespace

struct dspfx_mixmatrix : BankError {
    dspfx_mixmatrix_desc desc{};
    std::vector<uint64_t> gs;                    // the table, [G + 1]
    std::vector<Room> hrooms;
    std::mutex mu;                               // run / destroy
    Stores stores;                               // the matrix stores
    float *tab = nullptr, *div = nullptr, *stage = nullptr;      // stage: [maxn][maxn], where a drained store's values land
    Room *rooms = nullptr;
    Item *items = nullptr;
    uint32_t *room_of = nullptr;
    uint32_t n_items = 0, maxn = 0;
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;
    bool used = false;
};

namespace {

void release(dspfx_mixmatrix *p) {
    (void)hipSetDevice(p->desc.device);
    for (void *d : {(void *)p->tab, (void *)p->div, (void *)p->stage, (void *)p->rooms, (void *)p->items, (void *)p->room_of})
        if (d) (void)hipFree(d);
    p->stores.free_all();
    if (p->ev) (void)hipEventDestroy(p->ev);
    delete p;
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

// one store onto the stream: a fill, or the values into `stage`, the scatter into the table and the recount
hipError_t apply_store(dspfx_mixmatrix *p, const Store &st, hipStream_t s) {
    if (st.kind == 2) return fill_rooms(p, st.room, st.count, st.preset, s);
    const Room &rm = p->hrooms[st.room];
    const uint32_t cells = st.count * rm.n;
    hipError_t err = hipMemcpyAsync(p->stage, st.vals, (size_t)cells * sizeof(float), hipMemcpyHostToDevice, s);
    if (err != hipSuccess) return err;
    mixmatrix_store<<<(cells + WG - 1) / WG, WG, 0, s>>>(p->tab, p->stage, rm.off, rm.n, st.l0, st.count, (uint32_t)st.kind);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    // a row store changes the wired count of its listeners, a column store that of every listener of the room
    return st.kind == 0 ? recount(p, rm.c0 + st.l0, st.count, s) : recount(p, rm.c0, rm.n, s);
}

// rows or columns [first, first + count) of one room, row_len values each
int store_lines(dspfx_mixmatrix *p, int kind, const float *vals, uint32_t row_len, uint64_t first, uint64_t count) {
    const char *what = kind ? "set_cols" : "set_rows";
    char buf[224];
    if (!vals) {
        std::snprintf(buf, sizeof buf, "mixmatrix %s: no values", what);
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    std::string why;                             // (a range that begins at N is in no room: not even an empty one is inside)
    if (check_range("mixmatrix", what, first, count, p->desc.n_channels, why, false) != DSPFX_OK) return p->fail(DSPFX_ERR_INVALID, why.c_str());
    const uint32_t room = (uint32_t)(std::upper_bound(p->gs.begin(), p->gs.end(), first) - p->gs.begin()) - 1;
    const Room &rm = p->hrooms[room];
    if (first + count > (uint64_t)rm.c0 + rm.n) {
        std::snprintf(buf, sizeof buf, "mixmatrix %s: channels [%llu, %llu + %llu) are not in one room (room %u is [%u, %u))", what,
                      (unsigned long long)first, (unsigned long long)first, (unsigned long long)count, room, rm.c0, rm.c0 + rm.n);
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    if (row_len != rm.n) {
        std::snprintf(buf, sizeof buf, "mixmatrix %s: a row of %u values, and room %u has %u members", what, row_len, room, rm.n);
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    if (count == 0) return DSPFX_OK;
    Store st;
    st.kind = kind;
    st.room = room;
    st.l0 = (uint32_t)first - rm.c0;
    st.count = (uint32_t)count;
    const size_t cells = (size_t)count * rm.n;
    if (!p->stores.staging(p->desc.device, cells, st)) {
        std::snprintf(buf, sizeof buf, "mixmatrix %s: no page-locked memory for the staged values", what);
        return p->fail(DSPFX_ERR_OOM, buf);
    }
    std::memcpy(st.vals, vals, cells * sizeof(float));
    p->stores.push(st);
    return DSPFX_OK;
}

}  // namespace

extern "C" const char *dspfx_mixmatrix_last_error(const dspfx_mixmatrix *p) { return p ? p->err.c_str() : g_err.c_str(); }

extern "C" int dspfx_mixmatrix_plan(const uint64_t *group_start, uint32_t n_groups, uint64_t n_channels, uint32_t tile_channels,
                                    uint32_t *count_out, uint32_t *edge_out, uint64_t *offset_out, uint64_t *total_bytes_out) {
    g_err.clear();
    const int rc = check_table("mixmatrix", group_start, n_groups, n_channels, tile_channels, MAXN, g_err);
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
        const int dev_rc = open_device("mixmatrix", desc->device, &g_err);
        if (dev_rc != DSPFX_OK) return dev_rc;
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
    close_bank(p, release);
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
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    if (room < -1 || room >= (int64_t)G) {
        std::snprintf(buf, sizeof buf, "mixmatrix fill: room %lld, and the bank has %u (-1: every room)", (long long)room, G);
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    Store st;
    st.kind = 2;
    st.room = room < 0 ? 0u : (uint32_t)room;
    st.count = room < 0 ? G : 1u;
    st.preset = preset;
    p->stores.push(st);
    return DSPFX_OK;
}

extern "C" int dspfx_mixmatrix_reset(dspfx_mixmatrix *p) { return dspfx_mixmatrix_fill(p, -1, DSPFX_MIXMATRIX_MIX_MINUS); }

extern "C" int dspfx_mixmatrix_run(dspfx_mixmatrix *p, const float *block, uint32_t n_frames, float *out, void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    if (!block || !out || n_frames == 0 || n_frames > p->desc.max_frames) return p->fail(DSPFX_ERR_INVALID, "mixmatrix run: block, out or n_frames");
    const uintptr_t bytes = (uintptr_t)p->desc.n_channels * n_frames * sizeof(float), b0 = (uintptr_t)block, o0 = (uintptr_t)out;
    if (b0 < o0 + bytes && o0 < b0 + bytes)
        return p->fail(DSPFX_ERR_INVALID, "mixmatrix run: out overlaps the block (every listener reads every source of its room: no in-place form)");
    hipStream_t s = (hipStream_t)stream;
    BANK_HIP_WHY(hipSetDevice(p->desc.device), "hipSetDevice");
    BANK_HIP_WHY(order(p, s), "stream order");
    BANK_HIP_WHY(p->stores.drain(s, [p](const Store &st, hipStream_t on) { return apply_store(p, st, on); }), "matrix store");
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
    BANK_HIP_WHY(hipGetLastError(), "mixmatrix_run");
    return DSPFX_OK;
}
