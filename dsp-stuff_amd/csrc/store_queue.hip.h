// store_queue.hip.h -- the staged-store queue of the banks that take live stores (mixgroups, mixmatrix and the per-channel banks
// strips, delays, talkers, dynamics, shapers, gens, blends, filters, firs, racks, cancel _kernels.hip; the latter through channel_bank.hip.h).
// A store is made on any thread at any time: its values are copied into a page-locked staging buffer and it joins the queue.  The
// next run drains the queue onto its own stream ahead of its kernel, in the order the stores were made, so a store between two runs
// changes exactly the second.  A staging buffer is reused once the event recorded behind its copy has passed.  Host only.
//
// The bank keeps what a store means: P holds its fields (which channels, which node, ..), and the `apply` it hands to drain() issues
// its copies and kernels.  The queue owns the buffers, the events and the order.
#pragma once

#include <hip/hip_runtime.h>

#include <deque>
#include <mutex>
#include <vector>

namespace {

template <class P>
struct StoreQueue {
    struct Store : P {
        float *vals = nullptr;       // page-locked, from staging(); nullptr: a store without values (a fill, a drop)
        size_t cap = 0;              // floats
        hipEvent_t ev = nullptr;     // recorded behind the store's copies while it is in `flying`
    };

    std::mutex qmu;                  // queue, spare, and whatever the bank changes together with a push
    std::deque<Store> queue;         // stores not yet handed to a stream (qmu)
    std::vector<Store> spare;        // staging buffers free for the next store (qmu)
    std::vector<Store> flying;       // copies queued on a stream (the bank's mu)
    std::vector<hipEvent_t> events;  // spare events (the bank's mu)

    // a staging buffer of at least `floats` for st, from the spare ones or new; nullptr: none to be had
    float *staging(int device, size_t floats, Store &st) {
        {
            std::lock_guard<std::mutex> lk(qmu);
            for (size_t i = 0; i < spare.size(); ++i)
                if (spare[i].cap >= floats) {
                    st.vals = spare[i].vals;
                    st.cap = spare[i].cap;
                    spare[i] = spare.back();
                    spare.pop_back();
                    return st.vals;
                }
        }
        if (hipSetDevice(device) != hipSuccess) return nullptr;
        if (hipHostMalloc((void **)&st.vals, floats * sizeof(float), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            st.vals = nullptr;
            return nullptr;
        }
        st.cap = floats;
        return st.vals;
    }

    // the store joins the queue; `also` runs under the same lock, before it does
    template <class F>
    void push(const Store &st, F also) {
        std::lock_guard<std::mutex> lk(qmu);
        also();
        queue.push_back(st);
    }
    void push(const Store &st) {
        push(st, [] {});
    }

    // (the bank's mu is held) the stores made so far, in order, onto the stream: apply(store, s) -> hipError_t issues one store's
    // copies and kernels.  Staging buffers whose copies are done go back to `spare` first.  A failed call drops the stores behind it
    template <class Apply>
    hipError_t drain(hipStream_t s, Apply apply) {
        std::vector<Store> done;
        for (size_t i = 0; i < flying.size();) {
            if (hipEventQuery(flying[i].ev) == hipSuccess) {
                events.push_back(flying[i].ev);
                flying[i].ev = nullptr;
                done.push_back(flying[i]);
                flying[i] = flying.back();
                flying.pop_back();
            } else {
                (void)hipGetLastError();
                ++i;
            }
        }
        std::deque<Store> q;
        {
            std::lock_guard<std::mutex> lk(qmu);
            for (Store &d : done) spare.push_back(d);
            q.swap(queue);
        }
        hipError_t err = hipSuccess;
        for (Store &st : q) {
            if (err != hipSuccess) {                 // dropped; its buffer is still freed
                if (st.vals) (void)hipHostFree(st.vals);
                continue;
            }
            err = apply(st, s);
            if (!st.vals) continue;
            if (err == hipSuccess) {
                if (events.empty()) {
                    err = hipEventCreateWithFlags(&st.ev, hipEventDisableTiming);
                } else {
                    st.ev = events.back();
                    events.pop_back();
                }
            }
            if (err == hipSuccess) err = hipEventRecord(st.ev, s);
            if (st.ev) {
                flying.push_back(st);
            } else {                                 // no event to tell when the copies are done: wait, then the buffer is free
                (void)hipStreamSynchronize(s);
                (void)hipHostFree(st.vals);
            }
        }
        return err;
    }

    // for the bank's release(): the device is set and idle
    void free_all() {
        for (Store &st : queue)
            if (st.vals) (void)hipHostFree(st.vals);
        for (Store &st : spare)
            if (st.vals) (void)hipHostFree(st.vals);
        for (Store &st : flying) {
            if (st.vals) (void)hipHostFree(st.vals);
            if (st.ev) (void)hipEventDestroy(st.ev);
        }
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
    }
};

}  // namespace
