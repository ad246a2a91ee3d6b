// What the 256 MiB Infinity Cache does for lines that come back, with and without the nontemporal hint (aux 2) the chain kernels
// put on their sample and ring streams.  Flat 8-byte-per-lane buffer accesses like load_row / store_row: a 256-lane workgroup
// owns one 128 KiB tile and walks its 64 rows of 2 KiB; tiles are walked front to back or back to front.  HIP events around the
// timed launch(es), median of REPS repetitions after warm-up; every repetition rebuilds the cache state it measures.
//   hipcc --offload-arch=gfx950 -O3 -o tools/micro/llc_reuse tools/micro/llc_reuse.hip && tools/micro/llc_reuse
// (profiles/llc_reuse.txt, section 1, holds one run and what it was read as.)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
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

int main() {
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
    CHECK(hipDeviceSynchronize());
    return 0;
}
