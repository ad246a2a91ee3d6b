// The plain part of csrc/slot_ring.hip.h with a host compiler, no GPU: every piece of every push of the shapes below, element by
// element against the layout rule, and the loop's bookkeeping.  Prints the number of checks and exits 0, or says what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../dsp-stuff_amd/csrc/slot_ring.hip.h"

// the layout rule of bank_common.hip.h, restated: element (f, c) of a block of nf frames
static size_t lay(uint32_t f, uint32_t c, uint32_t nf, uint32_t N, uint32_t W) {
    return W ? ((size_t)(c / W) * nf + f) * W + (c % W) : (size_t)f * N + c;
}

static long checks = 0;

#define CHECK(cond, ...)                      \
    do {                                      \
        ++checks;                             \
        if (!(cond)) {                        \
            std::printf("FAILED %s: ", #cond); \
            std::printf(__VA_ARGS__);         \
            std::printf("\n");                \
            std::exit(1);                     \
        }                                     \
    } while (0)

struct Piece {
    uint64_t f;
    uint32_t fa, nf;
};

int main() {
    const uint32_t N = 12, SLOT = 8, SLOTS = 3;
    const uint32_t tiles[] = {0, 4}, lengths[] = {1, 7, 8, 9, 20};
    std::vector<float> store((size_t)SLOTS * SLOT * N);
    for (uint32_t W : tiles) {
        const SlotRing ring{store.data(), SLOTS, SLOT, N, W};
        const uint32_t Wd = W ? W : N;
        for (uint32_t n_frames : lengths) {
            std::vector<float> block((size_t)n_frames * N);
            for (uint64_t f0 = 0; f0 < 2 * SLOTS * SLOT; ++f0) {
                // the next slot: null exactly when the count is no multiple of the slot length
                const float *next = next_slot(ring, f0);
                CHECK((next == nullptr) == (f0 % SLOT != 0), "f0 %llu", (unsigned long long)f0);
                if (next) CHECK(next == store.data() + (size_t)((f0 / SLOT) % SLOTS) * SLOT * N && next == slot_of(ring, f0), "f0 %llu", (unsigned long long)f0);

                // the pieces: in order, each inside one slot, together [f0, f0 + n_frames) once; the counter follows them
                std::vector<Piece> pieces;
                uint64_t counter = f0, expect = f0;
                const int rc = for_slot_pieces(ring, counter, n_frames, [&](uint64_t f, uint32_t fa, uint32_t nf) -> int {
                    CHECK(counter == expect && f == expect && fa == f - f0 && nf > 0, "W %u n %u f0 %llu f %llu", W, n_frames, (unsigned long long)f0,
                          (unsigned long long)f);
                    CHECK(f / SLOT == (f + nf - 1) / SLOT, "a piece crosses a slot boundary: f %llu nf %u", (unsigned long long)f, nf);
                    CHECK(f + nf == f0 + n_frames || (f + nf) % SLOT == 0, "a piece ends early: f %llu nf %u", (unsigned long long)f, nf);
                    pieces.push_back({f, fa, nf});
                    expect = f + nf;
                    return 0;
                });
                CHECK(rc == 0 && counter == f0 + n_frames && expect == counter, "W %u n %u f0 %llu", W, n_frames, (unsigned long long)f0);

                // the geometry of every piece against the layout rule
                for (const Piece &pc : pieces) {
                    const SlotPiece c = piece_of(ring, block.data(), n_frames, pc.fa, pc.f, pc.nf);
                    const size_t slot0 = (size_t)((pc.f / SLOT) % SLOTS) * SLOT * N;
                    CHECK(c.rows == N / Wd && c.len == (size_t)pc.nf * Wd, "rows %zu len %zu", c.rows, c.len);
                    if (W) CHECK(c.src_pitch == (size_t)n_frames * W && c.dst_pitch == (size_t)SLOT * W, "pitches %zu %zu", c.src_pitch, c.dst_pitch);
                    else CHECK(c.src_pitch == 0 && c.dst_pitch == 0, "pitches %zu %zu", c.src_pitch, c.dst_pitch);
                    for (size_t r = 0; r < c.rows; ++r)
                        for (size_t k = 0; k < c.len; ++k) {
                            const uint32_t df = (uint32_t)(k / Wd), ch = (uint32_t)(r * Wd + k % Wd);
                            const size_t d = (size_t)(c.dst - store.data()) + r * c.dst_pitch + k, s = (size_t)(c.src - block.data()) + r * c.src_pitch + k;
                            CHECK(d == slot0 + lay((uint32_t)(pc.f % SLOT) + df, ch, SLOT, N, W), "dst: W %u n %u f %llu r %zu k %zu", W, n_frames,
                                  (unsigned long long)pc.f, r, k);
                            CHECK(s == lay(pc.fa + df, ch, n_frames, N, W), "src: W %u n %u f %llu r %zu k %zu", W, n_frames, (unsigned long long)pc.f, r, k);
                            CHECK(d < store.size() && s < block.size(), "out of bounds: d %zu s %zu", d, s);
                        }
                }

                // a body that fails at piece i: its code comes back, the counter stays at the end of piece i - 1
                for (size_t i = 0; i < pieces.size(); ++i) {
                    uint64_t c2 = f0;
                    size_t at = 0;
                    const int rc2 = for_slot_pieces(ring, c2, n_frames, [&](uint64_t, uint32_t, uint32_t) -> int { return at++ == i ? -3 : 0; });
                    CHECK(rc2 == -3 && at == i + 1 && c2 == pieces[i].f, "fail at %zu: rc %d counter %llu", i, rc2, (unsigned long long)c2);
                }
            }
        }
    }
    std::printf("%ld checks\n", checks);
    return 0;
}
