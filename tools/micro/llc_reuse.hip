// What the 256 MiB Infinity Cache does for lines that come back, with and without the nontemporal hint (aux 2) the chain kernels
// put on their sample and ring streams.  Flat 8-byte-per-lane buffer accesses like load_row / store_row: a 256-lane workgroup
// owns one 128 KiB tile and walks its 64 rows of 2 KiB; tiles are walked front to back or back to front.  HIP events around the
// timed launch(es), median of REPS repetitions after warm-up; every repetition rebuilds the cache state it measures.
//   hipcc --offload-arch=gfx950 -O3 -o tools/micro/llc_reuse tools/micro/llc_reuse.hip && tools/micro/llc_reuse
// (profiles/llc_reuse.txt, section 1, holds one run and what it was read as.)
// `llc_reuse zones` runs the second part alone: the output stores' policy by dispatch-order zone (profiles/llc_zones.txt).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
constexpr unsigned WG = 256, ROW_BYTES = WG * 8, ROWS = 64, TILE_BYTES = ROW_BYTES * ROWS;   // 128 KiB
constexpr size_t MiB = 1 << 20;
constexpr int REPS = 21, WARM = 3;

#define CHECK(x)                                                                             \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } \
    } while (0)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const char *base, unsigned tile) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(base + (size_t)tile * TILE_BYTES), 0, (int)TILE_BYTES, 0x00020000);
}
__device__ __forceinline__ unsigned tile_of(int rev) { return rev ? gridDim.x - 1 - blockIdx.x : blockIdx.x; }

// grid = tiles of the buffer; never true: sink keeps the loads alive
template <int AUX>
__global__ void __launch_bounds__(WG) rd(const char *buf, int rev, unsigned *sink) {
    const __amdgpu_buffer_rsrc_t r = tile_rsrc(buf, tile_of(rev));
    unsigned acc = 0;
#pragma unroll 8
    for (unsigned row = 0; row < ROWS; ++row) {
        const u32x2 t = __builtin_amdgcn_raw_buffer_load_b64(r, (int)(threadIdx.x * 8), (int)(row * ROW_BYTES), AUX);
        acc ^= t.x ^ t.y;
    }
    if (acc == 0x9e3779b9u) *sink = acc;
}
template <int AUX>
__global__ void __launch_bounds__(WG) wr(char *buf, int rev, unsigned val) {
    const __amdgpu_buffer_rsrc_t r = tile_rsrc(buf, tile_of(rev));
    u32x2 t;
    t.x = val;
    t.y = threadIdx.x;
#pragma unroll 8
    for (unsigned row = 0; row < ROWS; ++row) __builtin_amdgcn_raw_buffer_store_b64(t, r, (int)(threadIdx.x * 8), (int)(row * ROW_BYTES), AUX);
}
// the chain's four streams over one tile walk: samples in (nt), ring rows read then written (nt), output written with AUX_OUT
template <int AUX_OUT>
__global__ void __launch_bounds__(WG) chainpat(const char *in, char *ring, char *out, int rev) {
    const unsigned tile = tile_of(rev);
    const __amdgpu_buffer_rsrc_t ri = tile_rsrc(in, tile), rr = tile_rsrc(ring, tile), ro = tile_rsrc(out, tile);
    for (unsigned row0 = 0; row0 < ROWS; row0 += 8) {
        u32x2 x[8], y[8];
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) {
            x[k] = __builtin_amdgcn_raw_buffer_load_b64(ri, (int)(threadIdx.x * 8), (int)((row0 + k) * ROW_BYTES), 2);
            y[k] = __builtin_amdgcn_raw_buffer_load_b64(rr, (int)(threadIdx.x * 8), (int)((row0 + k) * ROW_BYTES), 2);
        }
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) {
            __builtin_amdgcn_raw_buffer_store_b64(x[k], rr, (int)(threadIdx.x * 8), (int)((row0 + k) * ROW_BYTES), 2);
            __builtin_amdgcn_raw_buffer_store_b64(x[k] + y[k], ro, (int)(threadIdx.x * 8), (int)((row0 + k) * ROW_BYTES), AUX_OUT);
        }
    }
}

// chainpat with the output stores' policy chosen per workgroup, by its place in DISPATCH order (blockIdx, whichever way the
// tiles are walked): the first `head` workgroups rewrite what the launch before left, the last `tail` leave theirs for the
// next launch, the middle streams.  Where the zones meet or overlap every workgroup is a tail-zone workgroup.
// aux bits: 1 = sc0, 2 = nt, 16 = sc1.  state: a 32 MiB stream of 8 KiB per tile, read at the tile's start and written at its
// end (the chain kernels' state rows): 0 = none, 1 = default policy everywhere, 2 = nt outside the zones.
struct Zones {
    unsigned head, tail;        // workgroups
    int aux_head, aux_mid, aux_tail, state;
};
constexpr unsigned ST_ROWS = 4;                                                                 // 8 KiB of state per tile
template <int AUX_OUT, int AUX_ST>
__device__ __forceinline__ void zone_tile(const char *in, char *ring, char *out, char *state, unsigned tile, bool with_state) {
    const __amdgpu_buffer_rsrc_t ri = tile_rsrc(in, tile), rr = tile_rsrc(ring, tile), ro = tile_rsrc(out, tile);
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(state + (size_t)tile * (ST_ROWS * ROW_BYTES), 0, (int)(ST_ROWS * ROW_BYTES), 0x00020000);
    u32x2 s[ST_ROWS];
    if (with_state)
#pragma unroll
        for (unsigned k = 0; k < ST_ROWS; ++k) s[k] = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(threadIdx.x * 8), (int)(k * ROW_BYTES), AUX_ST);
    for (unsigned row0 = 0; row0 < ROWS; row0 += 8) {
        u32x2 x[8], y[8];
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) {
            x[k] = __builtin_amdgcn_raw_buffer_load_b64(ri, (int)(threadIdx.x * 8), (int)((row0 + k) * ROW_BYTES), 2);
            y[k] = __builtin_amdgcn_raw_buffer_load_b64(rr, (int)(threadIdx.x * 8), (int)((row0 + k) * ROW_BYTES), 2);
        }
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) {
            __builtin_amdgcn_raw_buffer_store_b64(x[k], rr, (int)(threadIdx.x * 8), (int)((row0 + k) * ROW_BYTES), 2);
            __builtin_amdgcn_raw_buffer_store_b64(x[k] + y[k], ro, (int)(threadIdx.x * 8), (int)((row0 + k) * ROW_BYTES), AUX_OUT);
        }
    }
    if (with_state)
#pragma unroll
        for (unsigned k = 0; k < ST_ROWS; ++k) __builtin_amdgcn_raw_buffer_store_b64(s[k] + 1u, rs, (int)(threadIdx.x * 8), (int)(k * ROW_BYTES), AUX_ST);
}
__global__ void __launch_bounds__(WG) zonepat(const char *in, char *ring, char *out, char *state, int rev, Zones z) {
    const unsigned tile = tile_of(rev);
    const bool in_tail = blockIdx.x + z.tail >= gridDim.x, in_head = !in_tail && blockIdx.x < z.head;
    const int aux = in_tail ? z.aux_tail : in_head ? z.aux_head : z.aux_mid;
    const bool st_nt = z.state == 2 && !in_tail && !in_head;
#define ZONE_CASE(A)                                                                 \
    case A:                                                                          \
        if (st_nt) zone_tile<A, 2>(in, ring, out, state, tile, true);                \
        else zone_tile<A, 0>(in, ring, out, state, tile, z.state != 0);              \
        break;
    switch (aux) {
        ZONE_CASE(0)
        ZONE_CASE(2)
        ZONE_CASE(16)
        ZONE_CASE(17)
        ZONE_CASE(18)
    }
#undef ZONE_CASE
}

static unsigned *g_sink;
static void read_buf(const char *b, size_t bytes, int aux, int rev = 0) {
    const unsigned tiles = (unsigned)(bytes / TILE_BYTES);
    if (aux) hipLaunchKernelGGL(rd<2>, dim3(tiles), dim3(WG), 0, 0, b, rev, g_sink);
    else hipLaunchKernelGGL(rd<0>, dim3(tiles), dim3(WG), 0, 0, b, rev, g_sink);
}
static void write_buf(char *b, size_t bytes, int aux, int rev = 0) {
    static unsigned val = 1;
    const unsigned tiles = (unsigned)(bytes / TILE_BYTES);
    if (aux) hipLaunchKernelGGL(wr<2>, dim3(tiles), dim3(WG), 0, 0, b, rev, ++val);
    else hipLaunchKernelGGL(wr<0>, dim3(tiles), dim3(WG), 0, 0, b, rev, ++val);
}
static void chain_pat(const char *in, char *ring, char *out, size_t bytes, int aux_out, int rev) {
    const unsigned tiles = (unsigned)(bytes / TILE_BYTES);
    if (aux_out) hipLaunchKernelGGL(chainpat<2>, dim3(tiles), dim3(WG), 0, 0, in, ring, out, rev);
    else hipLaunchKernelGGL(chainpat<0>, dim3(tiles), dim3(WG), 0, 0, in, ring, out, rev);
}

static hipEvent_t e0, e1;
template <class PRE, class TIMED>
static float median_us(PRE pre, TIMED timed) {
    std::vector<float> v;
    for (int r = 0; r < WARM + REPS; ++r) {
        pre();
        CHECK(hipEventRecord(e0, 0));
        timed();
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        float ms;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= WARM) v.push_back(ms * 1000.0f);
    }
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

// Section 2 (profiles/llc_zones.txt): the alternating chain pattern with a head zone, a middle and a tail zone, steady state
// (8 alternating launches after 2), microseconds per launch.  `state` is a 32 MiB buffer, the others 512 MiB.
static void zones_section(const char *in, char *ring, char *out, char *state, size_t bytes) {
    const unsigned tiles = (unsigned)(bytes / TILE_BYTES);
    const unsigned per_mib = (unsigned)(MiB / TILE_BYTES);
    struct Pol { int aux; const char *name; };
    const Pol heads[] = {{0, "default"}, {2, "nt"}, {16, "sc1"}, {17, "sc0 sc1"}, {18, "nt sc1"}};
    const Pol tails[] = {{0, "default"}, {16, "sc1"}, {17, "sc0 sc1"}};
    const unsigned zs[] = {64, 96, 128, 160, 192, 224};
    const char *states[] = {"no state stream", "32 MiB state stream beside it, default policy", "32 MiB state stream beside it, nt outside the zones"};
    auto steady = [&](Zones z) {
        auto go = [&](int n) { for (int k = 0; k < n; ++k) hipLaunchKernelGGL(zonepat, dim3(tiles), dim3(WG), 0, 0, in, ring, out, state, k & 1, z); };
        return median_us([&] { go(2); }, [&] { go(8); }) / 8.0f;
    };
    printf("\n## zones: alternating chain pattern, output stores by dispatch-order zone (head | middle nt | tail), us per launch\n");
    for (int st = 0; st < 3; ++st) {
        printf("### %s\n", states[st]);
        printf("no zones (all nt)                %8.2f\n", steady(Zones{0, 0, 2, 2, 2, st}));
        for (const Pol &t : tails) {
            printf("# tail %-8s   head \\ Z MiB", t.name);
            for (unsigned z : zs) printf(" %8u", z);
            printf("\n");
            for (const Pol &h : heads) {
                printf("tail %-8s head %-8s     ", t.name, h.name);
                for (unsigned z : zs) printf(" %8.2f", steady(Zones{z * per_mib, z * per_mib, h.aux, 2, t.aux, st}));
                printf("\n");
                fflush(stdout);
            }
        }
    }
    printf("### no state stream, tail default: head zone HALF the tail zone (columns: tail Z MiB)\n");
    const unsigned zt[] = {128, 192, 224};
    for (const Pol &h : heads) {
        printf("tail default  head %-8s     ", h.name);
        for (unsigned z : zt) printf(" %8.2f", steady(Zones{z / 2 * per_mib, z * per_mib, h.aux, 2, 0, 0}));
        printf("\n");
    }
    // head nt is the middle's policy, i.e. NO head zone: the tail zone alone may then grow past half the buffer
    printf("### tail zone alone (head = middle = nt), tail default (columns: tail Z MiB; 512 = every output store on the default policy)\n");
    const unsigned zl[] = {192, 224, 256, 288, 320, 384, 512};
    printf("#                                ");
    for (unsigned z : zl) printf(" %8u", z);
    printf("\n");
    for (int st = 0; st < 3; ++st) {
        printf("state mode %d                     ", st);
        for (unsigned z : zl) printf(" %8.2f", steady(Zones{0, z * per_mib, 2, 2, 0, st}));
        printf("\n");
    }
    // what one figure above is good for: the write-through candidates against today's pair, three interleaved passes
    printf("### repeatability: three interleaved passes (columns: Z 96 / Z 128 without, Z 96 / Z 128 with the default-policy state stream)\n");
    const int cand[][2] = {{0, 0}, {16, 0}, {17, 0}, {0, 16}, {16, 16}};       // {head aux, tail aux}
    for (int pass = 0; pass < 3; ++pass)
        for (const auto &c : cand) {
            printf("pass %d  head aux %2d  tail aux %2d    ", pass, c[0], c[1]);
            for (int st = 0; st < 2; ++st)
                for (unsigned z : {96u, 128u}) printf(" %8.2f", steady(Zones{z * per_mib, z * per_mib, c[0], 2, c[1], st}));
            printf("\n");
        }
}

int main(int argc, char **argv) {
    const bool zones_only = argc > 1 && !strcmp(argv[1], "zones");      // `llc_reuse zones`: section 2 alone
    const size_t S = 32 * MiB, L = 512 * MiB;
    char *small, *ta, *tb, *big[4];
    CHECK(hipMalloc(&small, S));
    CHECK(hipMalloc(&ta, S));
    CHECK(hipMalloc(&tb, S));
    for (auto &p : big) { CHECK(hipMalloc(&p, L)); CHECK(hipMemset(p, 0, L)); }
    CHECK(hipMalloc(&g_sink, 4));
    CHECK(hipMemset(small, 0, S));
    CHECK(hipMemset(ta, 0, S));
    CHECK(hipMemset(tb, 0, S));
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    // displaces whatever the cache holds: 512 MiB read and 512 MiB written on the default policy
    auto flush = [&] { read_buf(big[2], L, 0); write_buf(big[3], L, 0); };
    // 64 MiB of other traffic: 32 MiB read, 32 MiB written
    auto traffic64 = [&](int aux) { read_buf(ta, S, aux); write_buf(tb, S, aux); };

    if (zones_only) {
        printf("# llc_reuse zones: median of %d repetitions, microseconds (HIP events around the timed launches)\n", REPS);
        zones_section(big[1], big[2], big[0], small, L);
        CHECK(hipDeviceSynchronize());
        return 0;
    }
    printf("# llc_reuse: median of %d repetitions, microseconds (HIP events around the timed launch)\n", REPS);
    const float t_empty = median_us([] {}, [&] { read_buf(small, TILE_BYTES, 0); });
    printf("one-tile launch (event overhead)        %8.2f\n", t_empty);

    printf("\n## re-read: read 32 MiB, 64 MiB of other traffic, read the 32 MiB again (timed)\n");
    printf("# first/timed read aux, traffic aux -> us   (GB/s)\n");
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            const float t = median_us([&] { flush(); read_buf(small, S, a * 2); traffic64(b * 2); }, [&] { read_buf(small, S, a * 2); });
            printf("read aux %d, traffic aux %d               %8.2f   %7.0f\n", a * 2, b * 2, t, S / (t * 1e-6) / 1e9);
        }
    for (int a = 0; a < 2; ++a) {
        const float t = median_us([&] { read_buf(small, S, a * 2); flush(); }, [&] { read_buf(small, S, a * 2); });
        printf("read aux %d, cold (behind 1 GiB)          %8.2f   %7.0f\n", a * 2, t, S / (t * 1e-6) / 1e9);
    }

    printf("\n## rewrite: write 32 MiB, 64 MiB of other traffic, write the 32 MiB again (timed)\n");
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            const float t = median_us([&] { flush(); write_buf(small, S, a * 2); traffic64(b * 2); }, [&] { write_buf(small, S, a * 2); });
            printf("write aux %d, traffic aux %d              %8.2f   %7.0f\n", a * 2, b * 2, t, S / (t * 1e-6) / 1e9);
        }
    for (int a = 0; a < 2; ++a) {
        const float t = median_us([&] { write_buf(small, S, a * 2); flush(); }, [&] { write_buf(small, S, a * 2); });
        printf("write aux %d, cold (behind 1 GiB)         %8.2f   %7.0f\n", a * 2, t, S / (t * 1e-6) / 1e9);
    }
    // back-to-back launches queue behind each other: a 32 MiB store launch returns before its lines have drained, so also
    // time FOUR rewrites in a row (the steady state of an output block rewritten every call) against four cold buffers
    for (int a = 0; a < 2; ++a) {
        const float hot = median_us([&] { flush(); write_buf(small, S, a * 2); }, [&] { for (int k = 0; k < 4; ++k) write_buf(small, S, a * 2); });
        const float cold = median_us([&] { flush(); }, [&] { for (int k = 0; k < 4; ++k) write_buf(big[0] + (size_t)k * 64 * MiB, S, a * 2); });
        printf("write aux %d, 4 x same 32 MiB / 4 x fresh %8.2f / %8.2f\n", a * 2, hot, cold);
    }

    printf("\n## large walk: 512 MiB written twice; the second launch is timed\n");
    for (int a = 0; a < 2; ++a)
        for (int rev = 0; rev < 2; ++rev) {
            const float t = median_us([&] { flush(); write_buf(big[0], L, a * 2, 0); }, [&] { write_buf(big[0], L, a * 2, rev); });
            printf("write aux %d alone, forward then %s   %8.2f   %7.0f\n", a * 2, rev ? "backward" : "forward ", t, L / (t * 1e-6) / 1e9);
        }
    printf("# with the chain's other streams beside it (512 MiB read nt, 512 MiB read-then-written nt): 2 GiB per launch\n");
    for (int a = 0; a < 2; ++a)
        for (int rev = 0; rev < 2; ++rev) {
            const float t = median_us([&] { flush(); chain_pat(big[1], big[2], big[0], L, a * 2, 0); }, [&] { chain_pat(big[1], big[2], big[0], L, a * 2, rev); });
            printf("out aux %d in chain, forward then %s  %8.2f   %7.0f\n", a * 2, rev ? "backward" : "forward ", t, 4.0 * L / (t * 1e-6) / 1e9);
        }
    printf("# steady state, 8 launches in a row after 2 of the same pattern: us per launch\n");
    for (int a = 0; a < 2; ++a)
        for (int alt = 0; alt < 2; ++alt) {
            const float t = median_us([&] { for (int k = 0; k < 2; ++k) chain_pat(big[1], big[2], big[0], L, a * 2, alt ? k & 1 : 0); },
                                      [&] { for (int k = 0; k < 8; ++k) chain_pat(big[1], big[2], big[0], L, a * 2, alt ? k & 1 : 0); }) / 8.0f;
            printf("out aux %d in chain, %s         %8.2f   %7.0f\n", a * 2, alt ? "alternating " : "all forward ", t, 4.0 * L / (t * 1e-6) / 1e9);
        }
    zones_section(big[1], big[2], big[0], small, L);
    CHECK(hipDeviceSynchronize());
    return 0;
}
