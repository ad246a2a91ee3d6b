// channel_bank.hip.h -- the scaffold of the per-channel banks (strips, delays, talkers, dynamics, shapers, gens, blends _kernels.hip): the
// members they all have, and the host glue around BankError (bank_common.hip.h) and StoreQueue (store_queue.hip.h) that is the
// same in each -- the range check, create's first lines, a run's first lines, a store without values, a host table read back.
// A bank keeps what its stores mean (apply_store, its host tables, its validation), its kernels and its launch.  Host only.
//
// A bank's struct derives from ChannelBank and names itself: static constexpr const char *name, the prefix of its reasons.  The
// reasons of a failed create go to the thread-local g_err of the bank's own file, so dspfx_<bank>_last_error(NULL) keeps its meaning.
#pragma once

#include <cstdio>
#include <mutex>
#include <string>

#include "bank_common.hip.h"
#include "store_queue.hip.h"

namespace {

// Desc: the bank's dspfx_<bank>_desc (abi_version, device, n_channels, max_frames, tile_channels, ..); Fields: what a store of its holds
template <class Desc, class Fields>
struct ChannelBank : BankError {
    typedef StoreQueue<Fields> Stores;
    typedef typename Stores::Store Store;
    Desc desc{};
    std::mutex mu;               // run / reset / destroy
    std::mutex smu;              // one store at a time, where a store reads the host tables before it queues (strips': never taken)
    Stores stores;               // its qmu guards the host tables' writes and their readers
    hipEvent_t ev = nullptr;     // order()
    hipStream_t last = nullptr;
    bool used = false;
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

// a store of `kind` without values over a range; `also` runs under the queue's lock as the store joins (StoreQueue::push)
template <class Bank, class Kind, class Also>
int store_plain(Bank *p, Kind kind, const char *call, uint64_t first, uint64_t count, Also also) {
    if (!p) return DSPFX_ERR_INVALID;
    const int rc = check_range(p, call, first, count);
    if (rc != DSPFX_OK) return rc;
    if (count == 0) return DSPFX_OK;
    typename Bank::Store st;
    st.kind = kind;
    st.first = (uint32_t)first;
    st.count = (uint32_t)count;
    std::lock_guard<std::mutex> one(p->smu);
    p->stores.push(st, also);
    return DSPFX_OK;
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
