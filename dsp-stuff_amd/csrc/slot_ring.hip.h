// slot_ring.hip.h -- the ring of block slots of the banks that take blocks in (pitch, spectrum, resample _kernels.hip): a ring of
// `slots` slots of `frames` frames, each slot in the desc's layout (lay, bank_common.hip.h) for a block of `frames` frames, so an engine
// can write its output straight into the next slot.  Stream frame f lies in slot (f / frames) % slots, at frame f % frames of it.
// The first part is plain C++ with no HIP in it (tests/cpp/test_slot_ring.cpp builds it with a host compiler): where a frame lies,
// the copy geometry of one piece of a push, and the loop that cuts a push at the slot boundaries.  The second part, under hipcc only,
// is the device side of a push.  The copy itself stays in the bank: the slot copy kernel (pitch, spectrum) or the copy engine (resample).
#pragma once

#include <cstddef>
#include <cstdint>

namespace {

struct SlotRing {
    float *base = nullptr;       // slots x frames x N floats
    uint32_t slots = 0;
    uint32_t frames = 0;         // per slot
    uint32_t N = 0, W = 0;       // the desc's channels and tile_channels
};

// the slot that stream frame f lies in
inline float *slot_of(const SlotRing &r, uint64_t f) { return r.base + (size_t)((f / r.frames) % r.slots) * r.frames * r.N; }

// the next whole slot for a producer after `pushed` frames: null unless they end on a slot boundary
inline float *next_slot(const SlotRing &r, uint64_t pushed) { return pushed % r.frames ? nullptr : slot_of(r, pushed); }

// one piece of a push: `rows` rows of `len` floats, row i at src + i * src_pitch -> dst + i * dst_pitch (pitches 0: one row)
struct SlotPiece {
    float *dst;
    const float *src;
    size_t rows, len, src_pitch, dst_pitch;
};

// frames [f, f + nf) of the ring (inside one slot) <- frames [fa, fa + nf) of `block`, a block of n_frames in the layout
inline SlotPiece piece_of(const SlotRing &r, const float *block, uint32_t n_frames, uint32_t fa, uint64_t f, uint32_t nf) {
    const uint32_t g0 = (uint32_t)(f % r.frames);
    float *slot = slot_of(r, f);
    if (!r.W) return {slot + (size_t)g0 * r.N, block + (size_t)fa * r.N, 1, (size_t)nf * r.N, 0, 0};
    return {slot + (size_t)g0 * r.W, block + (size_t)fa * r.W, r.N / r.W, (size_t)nf * r.W, (size_t)n_frames * r.W, (size_t)r.frames * r.W};
}

// a push of n_frames from frame `counter` on, cut at the slot boundaries: body(f, fa, nf) -> int (0: done) launches frames
// [f, f + nf) of the ring, frames [fa, fa + nf) of the block, and whatever falls due with them.  `counter` advances behind each
// piece that succeeded -- what has been launched so far: a failure part-way leaves a consistent state -- and the first failure
// is returned
template <class Body>
int for_slot_pieces(const SlotRing &r, uint64_t &counter, uint32_t n_frames, Body body) {
    const uint64_t f0 = counter, f1 = f0 + n_frames;
    for (uint64_t f = f0; f < f1;) {
        const uint64_t next = (f / r.frames + 1) * r.frames, end = f1 < next ? f1 : next;
        const int rc = body(f, (uint32_t)(f - f0), (uint32_t)(end - f));
        if (rc != 0) return rc;
        counter = f = end;
    }
    return 0;
}

}  // namespace

#ifdef __HIPCC__
#include "bank_common.hip.h"

namespace {

// the device side of a push (the bank's mu is held, its own conditions are met): the device, the stream order, the pieces
template <class Bank, class Body>
int push_pieces(Bank *p, const SlotRing &r, uint64_t &counter, uint32_t n_frames, hipStream_t s, Body body) {
    BANK_HIP(hipSetDevice(p->desc.device));
    BANK_HIP(order(p, s));
    return for_slot_pieces(r, counter, n_frames, body);
}

}  // namespace
#endif
