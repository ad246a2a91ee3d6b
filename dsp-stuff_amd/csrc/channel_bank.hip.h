// channel_bank.hip.h -- the scaffold of the per-channel banks (strips, delays, talkers, dynamics, shapers, gens, blends, filters,
// firs, racks, cancel _kernels.hip): the members they all have, and the host glue around BankError (bank_common.hip.h) and StoreQueue
// (store_queue.hip.h) that is the same in each -- the range check, create's checks and its tail, the device tables' bytes,
// allocation, clearing and freeing from the bank's one list of them, a run's first lines, a staged store's first lines, a store
// without values, a host table read back.  A bank keeps what its stores mean (apply_store, its host tables, its validation), its
// kernels and its launch.  Host only.
//
// A bank's struct derives from ChannelBank and names itself: static constexpr const char *name, the prefix of its reasons.  It lists
// its device tables once, in a static member that needs no bank (plan runs without a GPU):
//     template <class V> static void tables(const Desc &d, V v) { v(bytes, fill, &Bank::member); v(bytes, fill, &Bank::array, i); .. }
// in the order they are allocated, cleared and freed; fill is the byte a fresh bank holds in the table (above 0xFF: a 32-bit
// pattern for a table of words), or TABLE_BY_HAND for a table that create's memsets leave alone.  The reasons of a failed create
// go to the thread-local g_err of the bank's own file, so dspfx_<bank>_last_error(NULL) keeps its meaning.
#pragma once

#include <cstddef>
#include <cstdio>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>

#include "bank_common.hip.h"
#include "store_queue.hip.h"

namespace {

// Desc: the bank's dspfx_<bank>_desc (abi_version, device, n_channels, max_frames, tile_channels, ..); Fields: what a store of its holds
template <class Desc, class Fields>
struct ChannelBank : BankError, BankCore<Desc> {      // mu: run / reset / destroy
    typedef StoreQueue<Fields> Stores;
    typedef typename Stores::Store Store;
    std::mutex smu;              // one store at a time, where a store reads the host tables before it queues (strips': never taken)
    Stores stores;               // its qmu guards the host tables' writes and their readers
};

// channels [first, first + count) of `call` lie inside the bank; the reason is kept
template <class Bank>
int check_range(Bank *p, const char *call, uint64_t first, uint64_t count) {
    std::string why;
    const int rc = check_range(Bank::name, call, first, count, p->desc.n_channels, why);
    return rc == DSPFX_OK ? rc : p->fail(rc, why.c_str());
}

// create's first lines, up to the device: the arguments, abi_version and max_frames, the shape, `more(err)` -- the bank's own checks
// of its desc -- and open_device.  *out is cleared; the reason goes to err
template <class Bank, class Desc, class More>
int create_checks(const Desc *desc, Bank **out, std::string &err, More more) {
    if (!desc || !out) {
        err = std::string(Bank::name) + ": null argument";
        return DSPFX_ERR_INVALID;
    }
    *out = nullptr;
    err.clear();
    if (desc->abi_version != DSPFX_ABI_VERSION || desc->max_frames == 0 || desc->max_frames > (1u << 20)) {
        err = std::string(Bank::name) + ": abi_version or max_frames";
        return DSPFX_ERR_INVALID;
    }
    int rc = check_shape(Bank::name, desc->n_channels, desc->tile_channels, err);
    if (rc == DSPFX_OK) rc = more(err);
    if (rc == DSPFX_OK) rc = open_device(Bank::name, desc->device, &err);
    return rc;
}

template <class Bank, class Desc>
int create_checks(const Desc *desc, Bank **out, std::string &err) {
    return create_checks(desc, out, err, [](std::string &) -> int { return DSPFX_OK; });
}

// create found no device memory for the bank's tables
inline int no_table_memory(const char *name, uint64_t bytes, uint32_t N, std::string &err) {
    char buf[160];
    std::snprintf(buf, sizeof buf, "%s: no device memory for %llu bytes of tables (%u channels)", name, (unsigned long long)bytes, N);
    err = buf;
    return DSPFX_ERR_OOM;
}

// ---- the bank's list of device tables (Bank::tables, above) -------------------------------------------------------------------------
constexpr int64_t TABLE_BY_HAND = -1;

// where the bank keeps the table's device pointer
template <class Bank, class T>
void **table_slot(Bank *p, T *Bank::*m) {
    return (void **)&(p->*m);
}
template <class Bank, class T, size_t K>
void **table_slot(Bank *p, T *(Bank::*m)[K], int i) {
    return (void **)&(p->*m)[i];
}

// the bytes of a bank of this desc on the device
template <class Bank, class Desc>
uint64_t table_bytes(const Desc &d) {
    uint64_t sum = 0;
    Bank::tables(d, [&](uint64_t bytes, int64_t, auto...) { sum += bytes; });
    return sum;
}

// the body of dspfx_<bank>_plan: more(d, err) puts what else fixes the sizes into the desc and checks it
template <class Bank, class More>
int plan_bank(uint64_t channels, uint64_t *bytes_out, std::string &err, More more) {
    err.clear();
    decltype(Bank::desc) d{};
    int rc = check_shape(Bank::name, channels, 0, err);
    if (rc == DSPFX_OK) {
        d.n_channels = (uint32_t)channels;
        rc = more(d, err);
    }
    if (rc != DSPFX_OK) return rc;
    if (bytes_out) *bytes_out = table_bytes<Bank>(d);
    return DSPFX_OK;
}

template <class Bank>
int plan_bank(uint64_t channels, uint64_t *bytes_out, std::string &err) {
    return plan_bank<Bank>(channels, bytes_out, err, [](decltype(Bank::desc) &, std::string &) -> int { return DSPFX_OK; });
}

// a bank's release and the body of dspfx_<bank>_destroy (bank_common.hip.h), the device tables being the listed ones
template <class Bank>
void release_tables(Bank *p) {
    release_bank_by(p, [p] {
        Bank::tables(p->desc, [p](uint64_t, int64_t, auto... m) {
            if (void *d = *table_slot(p, m...)) (void)hipFree(d);
        });
    });
}

template <class Bank>
int destroy_bank(Bank *p) {
    return destroy_bank(p, release_tables<Bank>);
}

// create behind create_checks: the bank with its desc; init(p), its host tables and whatever else the desc fixes (bad_alloc is
// caught here); the listed tables allocated -- no_memory is the reason where there is no room, nullptr: no_table_memory's --;
// fresh(p) -> hipError_t, the clearing that is not a memset (nullptr: none); the tables' fill, the device idle, the bank's event
template <class Bank, class Desc, class Init, class Fresh>
int create_bank(const Desc *desc, Bank **out, std::string &err, Init init, Fresh fresh, const char *no_memory) {
    Bank *p = new (std::nothrow) Bank;
    if (!p) return DSPFX_ERR_OOM;
    p->desc = *desc;
    try {
        init(p);
    } catch (const std::bad_alloc &) {
        delete p;
        return DSPFX_ERR_OOM;
    }
    bool ok = true;
    Bank::tables(p->desc, [&](uint64_t bytes, int64_t, auto... m) { ok = ok && hipMalloc(table_slot(p, m...), (size_t)bytes) == hipSuccess; });
    if (!ok) {
        (void)hipGetLastError();
        release_tables(p);
        if (!no_memory) return no_table_memory(Bank::name, table_bytes<Bank>(*desc), desc->n_channels, err);
        err = no_memory;
        return DSPFX_ERR_OOM;
    }
    if constexpr (!std::is_same<Fresh, std::nullptr_t>::value) ok = fresh(p) == hipSuccess;
    Bank::tables(p->desc, [&](uint64_t bytes, int64_t fill, auto... m) {
        void *d = *table_slot(p, m...);
        if (fill == TABLE_BY_HAND || !ok) return;
        ok = (fill > 0xFF ? hipMemsetD32((hipDeviceptr_t)d, (int)fill, (size_t)bytes / 4) : hipMemset(d, (int)fill, (size_t)bytes)) == hipSuccess;
    });
    ok = ok && hipDeviceSynchronize() == hipSuccess && hipEventCreateWithFlags(&p->ev, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        release_tables(p);
        return DSPFX_ERR_HIP;
    }
    *out = p;
    return DSPFX_OK;
}

template <class Bank, class Desc, class Init>
int create_bank(const Desc *desc, Bank **out, std::string &err, Init init) {
    return create_bank(desc, out, err, init, nullptr, nullptr);
}

// a run's first lines (the bank's mu is held): the arguments -- args_ok is the bank's test of its own pointers, `bad` the reason that
// names them -- the device, the stream order, then the stores made so far onto the stream through the bank's apply(p, store, s)
template <class Bank, class Apply>
int begin_run(Bank *p, bool args_ok, uint32_t n_frames, hipStream_t s, const char *bad, const char *store_what, Apply apply) {
    if (!args_ok || n_frames == 0 || n_frames > p->desc.max_frames) return p->fail(DSPFX_ERR_INVALID, bad);
    BANK_HIP_WHY(hipSetDevice(p->desc.device), "hipSetDevice");
    BANK_HIP_WHY(order(p, s), "stream order");
    BANK_HIP_WHY(p->stores.drain(s, [p, apply](const typename Bank::Store &st, hipStream_t on) { return apply(p, st, on); }), store_what);
    return DSPFX_OK;
}

// a staged store's first lines: its range, the bank's smu -- through `one`, which the caller keeps until the store has joined the
// queue; nullptr: not taken here -- and `floats` of page-locked staging (0: a store without values).  false: there is none, the
// call returns DSPFX_ERR_OOM; `what` ends the reason
template <class Bank>
bool stage_store(Bank *p, typename Bank::Store &st, std::unique_lock<std::mutex> *one, const char *call, uint64_t first, uint64_t count, size_t floats,
                const char *what) {
    st.first = (uint32_t)first;
    st.count = (uint32_t)count;
    if (one) *one = std::unique_lock<std::mutex>(p->smu);
    if (floats == 0 || p->stores.staging(p->desc.device, floats, st)) return true;
    p->fail(DSPFX_ERR_OOM, (std::string(Bank::name) + " " + call + ": no page-locked memory for the " + what).c_str());
    return false;
}

// ... of a bank whose stores have a kind
template <class Bank, class Kind>
bool stage_store(Bank *p, typename Bank::Store &st, std::unique_lock<std::mutex> *one, Kind kind, const char *call, uint64_t first, uint64_t count,
                size_t floats, const char *what) {
    st.kind = kind;
    return stage_store(p, st, one, call, first, count, floats, what);
}

// a store of `kind` without values over a range; fields(st) sets what else the bank's store holds, `also` runs under the queue's
// lock as the store joins (StoreQueue::push)
template <class Bank, class Kind, class Also, class Fields>
int store_plain(Bank *p, Kind kind, const char *call, uint64_t first, uint64_t count, Also also, Fields fields) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_range(p, call, first, count);
    if (rc != DSPFX_OK) return rc;
    if (count == 0) return DSPFX_OK;
    typename Bank::Store st;
    std::unique_lock<std::mutex> one;
    fields(st);
    (void)stage_store(p, st, &one, kind, call, first, count, 0, "");
    p->stores.push(st, also);
    return DSPFX_OK;
}

template <class Bank, class Kind, class Also>
int store_plain(Bank *p, Kind kind, const char *call, uint64_t first, uint64_t count, Also also) {
    return store_plain(p, kind, call, first, count, also, [](typename Bank::Store &) {});
}

template <class Bank, class Kind>
int store_plain(Bank *p, Kind kind, const char *call, uint64_t first, uint64_t count) {
    return store_plain(p, kind, call, first, count, [] {});
}

// a host table over a range, as every store made so far left it: get(out, i, channel) writes entry i
template <class Bank, class T, class Get>
int read_table(Bank *p, const char *call, T *out, uint64_t first, uint64_t count, Get get) {
    if (!p) return DSPFX_ERR_INVALID;
    if (!out) return p->fail(DSPFX_ERR_INVALID, (std::string(Bank::name) + " " + call + ": no array").c_str());
    const int rc = check_range(p, call, first, count);
    if (rc != DSPFX_OK) return rc;
    std::lock_guard<std::mutex> lk(p->stores.qmu);
    for (uint64_t i = 0; i < count; ++i) get(out, i, first + i);
    return DSPFX_OK;
}

}  // namespace
