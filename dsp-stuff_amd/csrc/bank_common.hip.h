// bank_common.hip.h -- what the banks share (pitch, resample, spectrum, convolve, mixgroups, mixmatrix and the per-channel banks
// strips, delays, talkers, dynamics, shapers, gens, blends, filters _kernels.hip): the desc's layout, 4-channel loads and stores in it, the slot copy,
// and small host helpers -- all stateless --, BankCore, the members a bank's struct starts from, and the scaffold around it: the
// error holder of the banks that take live stores, the shape / range / table checks of their arguments, create_checks_plain,
// open_device, close_bank, release_plain / release_bank and destroy_bank.  Host and device, hipcc only.
// The FFT is in fft_core.hip.h, the staged stores in store_queue.hip.h, a lane's loads and stores of its own channels in
// lane_io.hip.h, what the per-channel banks share beyond this in channel_bank.hip.h, the ring of block slots of the banks that take
// blocks in (pitch, spectrum, resample) in slot_ring.hip.h.  The rest of a bank's struct and of create / reset are its own.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <mutex>
#include <string>

#include "../../include/dspfx.h"

// `call` failed: the extern "C" function around it returns DSPFX_ERR_HIP
#define BANK_HIP(call)                                  \
    do {                                                \
        if ((call) != hipSuccess) return DSPFX_ERR_HIP; \
    } while (0)

// ... of a bank that keeps the reason (BankError): the function returns p->fail(DSPFX_ERR_HIP, what)
#define BANK_HIP_WHY(call, what)                                        \
    do {                                                                \
        if ((call) != hipSuccess) return p->fail(DSPFX_ERR_HIP, what); \
    } while (0)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// element (f, c) of a block of nf frames in the desc's layout (dspfx_engine_desc.tile_channels)
__host__ __device__ inline size_t lay(uint32_t f, uint32_t c, uint32_t nf, uint32_t N, uint32_t W) {
    return W ? ((size_t)(c / W) * nf + f) * W + (c % W) : (size_t)f * N + c;
}

// frame f of 4 channels from c (c a multiple of 4) of a block at `base`; channels outside N read 0.  vec, which the host
// establishes: every group of 4 channels from a multiple of 4 is contiguous, 16-byte aligned and inside N
__device__ __forceinline__ float4 load4(const float *base, uint32_t vec, uint32_t f, uint32_t c, uint32_t nf, uint32_t N, uint32_t W) {
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (vec) {
        if (c < N) v = *(const float4 *)(base + lay(f, c, nf, N, W));
    } else {
        if (c < N) v.x = base[lay(f, c, nf, N, W)];
        if (c + 1 < N) v.y = base[lay(f, c + 1, nf, N, W)];
        if (c + 2 < N) v.z = base[lay(f, c + 2, nf, N, W)];
        if (c + 3 < N) v.w = base[lay(f, c + 3, nf, N, W)];
    }
    return v;
}

// ... and the store; channels outside N are not written.  NT: nontemporal
template <bool NT>
__device__ __forceinline__ void store4(float *base, float4 v, uint32_t vec, uint32_t f, uint32_t c, uint32_t nf, uint32_t N, uint32_t W) {
    if (vec) {
        if (c < N) {
            f32x4 *p = (f32x4 *)(base + lay(f, c, nf, N, W));
            const f32x4 t = {v.x, v.y, v.z, v.w};
            if (NT) __builtin_nontemporal_store(t, p);
            else *p = t;
        }
    } else {
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
            if (c + i < N) {
                float *p = base + lay(f, c + i, nf, N, W);
                if (NT) __builtin_nontemporal_store(e[i], p);
                else *p = e[i];
            }
    }
}

// ---- slot copy: `rows` rows of `len` elements, row r at src + r * spitch / dst + r * dpitch (units of T) -------------
template <typename T>
__global__ void slot_copy(const T *__restrict__ src, T *__restrict__ dst, size_t rows, size_t len, size_t spitch,
                          size_t dpitch) {
    const size_t total = rows * len;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t r = e / len, k = e - r * len;
        dst[r * dpitch + k] = src[r * spitch + k];
    }
}

// (a template only so that a bank that never copies has no copy kernel in its code object)
template <class = void>
hipError_t launch_copy(const float *src, float *dst, size_t rows, size_t len, size_t spitch, size_t dpitch, hipStream_t s) {
    const bool v4 = len % 4 == 0 && spitch % 4 == 0 && dpitch % 4 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0;
    const size_t units = rows * (v4 ? len / 4 : len);
    const unsigned blocks = (unsigned)std::min<size_t>((units + 255) / 256, 1u << 20);
    if (v4)
        slot_copy<float4><<<blocks, 256, 0, s>>>((const float4 *)src, (float4 *)dst, rows, len / 4, spitch / 4, dpitch / 4);
    else
        slot_copy<float><<<blocks, 256, 0, s>>>(src, dst, rows, len, spitch, dpitch);
    return hipGetLastError();
}

// ---- host helpers ---------------------------------------------------------------------------------------------------
bool pow2(uint32_t w) { return w && !(w & (w - 1)); }

// out[t] = exp(-2 pi i t / n), t in [0, n): f64, rounded once to f32
void twiddles(uint32_t n, float2 *out) {
    for (uint32_t t = 0; t < n; ++t) {
        const double ang = -2.0 * M_PI * t / n;
        out[t] = make_float2((float)std::cos(ang), (float)std::sin(ang));
    }
}

// what every bank has: its desc, the lock of its calls, and the stream order's event and state
template <class Desc>
struct BankCore {
    Desc desc{};
    std::mutex mu;               // the bank's calls are serialised
    hipEvent_t ev = nullptr;     // order()
    hipStream_t last = nullptr;
    bool used = false;
};

// a call on a stream other than the last one the bank used waits (on the device) for that one
template <class Bank>
hipError_t order(Bank *p, hipStream_t s) {
    hipError_t err = hipSuccess;
    if (p->used && s != p->last) {
        err = hipEventRecord(p->ev, p->last);
        if (err == hipSuccess) err = hipStreamWaitEvent(s, p->ev, 0);
    }
    p->last = s;
    p->used = true;
    return err;
}

// ---- the scaffold of the banks with stores -------------------------------------------------------------------------------------------
// the reason of a bank's last failed call, for its *_last_error; a bank derives from it
struct BankError {
    std::mutex emu;              // err: stores fail on any thread
    std::string err;
    int fail(int rc, const char *what) {
        std::lock_guard<std::mutex> lk(emu);
        err = what;
        return rc;
    }
};

// n_channels and tile_channels of a desc or a plan; `name` is the bank's, the prefix of every reason
int check_shape(const char *name, uint64_t N, uint32_t W, std::string &err) {
    char buf[192];
    if (N == 0 || N > 0xFFFFFF00ull) {
        err = std::string(name) + ": n_channels must be 1 .. 2^32 - 256";
        return DSPFX_ERR_INVALID;
    }
    if (W && (!pow2(W) || N % W)) {
        std::snprintf(buf, sizeof buf, "%s: tile_channels %u is not a power of two that divides n_channels %llu", name, W, (unsigned long long)N);
        err = buf;
        return DSPFX_ERR_INVALID;
    }
    return DSPFX_OK;
}

// channels [first, first + count) of a call lie inside the bank's N; end_ok: an empty range at N itself does
int check_range(const char *name, const char *call, uint64_t first, uint64_t count, uint64_t N, std::string &err, bool end_ok = true) {
    if (first > N || count > N - first || (!end_ok && first == N)) {
        char buf[192];
        std::snprintf(buf, sizeof buf, "%s %s: channels [%llu, %llu + %llu) are not inside the bank's %llu", name, call, (unsigned long long)first,
                      (unsigned long long)first, (unsigned long long)count, (unsigned long long)N);
        err = buf;
        return DSPFX_ERR_INVALID;
    }
    return DSPFX_OK;
}

// a group table gs[G + 1] over N channels: starts at 0, never decreases, ends at N.  max_room = 0: a group may be empty and as long
// as it likes; otherwise every group is a room of 1 .. max_room members
int check_table(const char *name, const uint64_t *gs, uint32_t G, uint64_t N, uint32_t W, uint32_t max_room, std::string &err) {
    char buf[192];
    if (!gs || G == 0) {
        err = std::string(name) + ": no group table";
        return DSPFX_ERR_INVALID;
    }
    const int rc = check_shape(name, N, W, err);
    if (rc != DSPFX_OK) return rc;
    if (gs[0] != 0) {
        std::snprintf(buf, sizeof buf, "%s: group_start[0] is %llu, not 0", name, (unsigned long long)gs[0]);
        err = buf;
        return DSPFX_ERR_INVALID;
    }
    for (uint32_t g = 0; g < G; ++g) {
        if (gs[g + 1] < gs[g]) {
            std::snprintf(buf, sizeof buf, "%s: group_start decreases at entry %u (%llu after %llu)", name, g + 1, (unsigned long long)gs[g + 1],
                          (unsigned long long)gs[g]);
            err = buf;
            return DSPFX_ERR_INVALID;
        }
        const uint64_t n = gs[g + 1] - gs[g];
        if (max_room && n == 0) {
            std::snprintf(buf, sizeof buf, "%s: room %u is empty (a room has 1 .. %u members)", name, g, max_room);
            err = buf;
            return DSPFX_ERR_INVALID;
        }
        if (max_room && n > max_room) {
            std::snprintf(buf, sizeof buf, "%s: room %u has %llu members, above DSPFX_MIXMATRIX_MAX_ROOM = %u", name, g, (unsigned long long)n, max_room);
            err = buf;
            return DSPFX_ERR_INVALID;
        }
    }
    if (gs[G] != N) {
        std::snprintf(buf, sizeof buf, "%s: group_start[%u] is %llu, not n_channels %llu", name, G, (unsigned long long)gs[G], (unsigned long long)N);
        err = buf;
        return DSPFX_ERR_INVALID;
    }
    return DSPFX_OK;
}

// create's device lines: the device exists and is the thread's current one.  err may be null (a bank that keeps no reason)
int open_device(const char *name, int device, std::string *err) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return DSPFX_ERR_NO_DEVICE;
    if (device < 0 || device >= count) {
        if (err) *err = std::string(name) + ": no such device";
        return DSPFX_ERR_INVALID;
    }
    if (hipSetDevice(device) != hipSuccess) return DSPFX_ERR_HIP;
    return DSPFX_OK;
}

// create's first lines in the banks that keep no reason (pitch, spectrum, resample, convolve): the arguments, abi_version, the
// shape, more() -- the bank's own checks of its desc -- and the device.  *out is cleared
template <class Desc, class Bank, class More>
int create_checks_plain(const Desc *desc, Bank **out, More more) {
    if (!desc || !out) return DSPFX_ERR_INVALID;
    *out = nullptr;
    if (desc->abi_version != DSPFX_ABI_VERSION || desc->channels == 0) return DSPFX_ERR_INVALID;
    const uint32_t N = desc->channels, W = desc->tile_channels;
    if (W && (!pow2(W) || N % W)) return DSPFX_ERR_INVALID;
    const int rc = more();
    return rc != DSPFX_OK ? rc : open_device(nullptr, desc->device, nullptr);
}

// destroy: no run is inside the bank, its work on the device is done, then `release` frees it
template <class Bank>
void close_bank(Bank *p, void (*release)(Bank *)) {
    {
        std::lock_guard<std::mutex> lk(p->mu);
        (void)hipSetDevice(p->desc.device);
        if (p->used) (void)hipStreamSynchronize(p->last);    // the bank's work is ordered on the last stream it used
    }
    release(p);
}

// a bank's `release`, where there is no more to it: free_tables() frees its device memory (the device is set), then the bank's
// event, the bank
template <class Bank, class FreeTables>
void release_plain_by(Bank *p, FreeTables free_tables) {
    (void)hipSetDevice(p->desc.device);
    free_tables();
    if (p->ev) (void)hipEventDestroy(p->ev);
    delete p;
}

// ... of a bank with staged stores (store_queue.hip.h): their buffers and events go behind the tables
template <class Bank, class FreeTables>
void release_bank_by(Bank *p, FreeTables free_tables) {
    release_plain_by(p, [&] {
        free_tables();
        p->stores.free_all();
    });
}

// the device pointers in `dev` (nullptr: never allocated)
inline void free_device(std::initializer_list<void *> dev) {
    for (void *d : dev)
        if (d) (void)hipFree(d);
}

// ... the tables being the device pointers in `dev`
template <class Bank>
void release_plain(Bank *p, std::initializer_list<void *> dev) {
    release_plain_by(p, [&] { free_device(dev); });
}

template <class Bank>
void release_bank(Bank *p, std::initializer_list<void *> dev) {
    release_bank_by(p, [&] { free_device(dev); });
}

// the body of dspfx_<bank>_destroy
template <class Bank>
int destroy_bank(Bank *p, void (*release)(Bank *)) {
    if (!p) return DSPFX_ERR_INVALID;
    close_bank(p, release);
    return DSPFX_OK;
}

}  // namespace
