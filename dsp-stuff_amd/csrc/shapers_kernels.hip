// shapers_kernels.hip -- the channel-shaper bank (include/dspfx.h, dspfx_shapers_*): every channel may carry one waveshaper node of
// its own -- Distort (nodes/distort.rs, nine modes), Overdrive (nodes/overdrive.rs) or Chebyshev (nodes/chebyshev.rs) -- with its own
// sliders.  The other slider banks differ per channel only in values; here the code path differs per lane, across twelve kinds.
//
// One run is one kernel behind the queued stores, in the shape of dynamics_run (dynamics_kernels.hip): a lane owns four adjacent
// channels with one 16-byte load and one nontemporal 16-byte store per frame when the layout allows it, one channel otherwise;
// frames are taken in chunks of F rows and the next chunk's loads are issued ahead of this one's arithmetic.  The arithmetic is the
// engine's own (chain_kernels.hip.h: distort1<MODE, false>, overdrive1, chebyshev1, tanh_cr), so a channel's bits are those of an
// Engine that runs that one node.  DIVERGENCE: before the frame loop every lane folds the bypasses into its kind codes (a Distort
// or Overdrive whose level is below 0.001 is a copy, as is a channel without a node, as is -- in this pass -- a Fuzz channel) and
// the wave ballots once per kind: a bit set for every kind one of its lanes carries.  Per chunk the wave walks the set bits with a
// wave-uniform switch and runs each present kind's templated body on all its values, keeping a result under a per-(lane,
// channel-of-four) select.  A wave whose 256 channels share a kind pays for one body, a wave that carries all of them for their
// sum, a wave of copies for none; no lane ever branches on its own kind.  Chebyshev's two tanh(level) denominators are computed per
// channel once per run, where the wave has such a channel.
//
// Fuzz (distort.rs:146-172) is block-global over reference blocks of 128 frames: three maxima over a channel's block.  It is a
// second kernel, launched only when the tables the run has drained hold a Fuzz channel, in place on `out` behind the first (which
// copied those channels): fuzz_kernel's decomposition (aux_kernels.hip) -- 64 channels per workgroup, four waves of 32 frames each,
// the three maxima combined through LDS -- with a level per channel and a predicate per channel.  A workgroup whose 64 kind bytes
// hold no Fuzz returns at once (all four waves read the same bytes: no barrier is needed for the decision); lanes without Fuzz
// take part in the barriers, load nothing, and store nothing.
//
// Stores (sliders, drops) go through the staged-store queue (store_queue.hip.h).  Nothing is shared between channels in the first
// kernel: no LDS, no atomics.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dspfx.h"
#include "chain_kernels.hip.h"
#include "channel_bank.hip.h"
#include "lane_io.hip.h"

namespace {

constexpr uint32_t SWG = 256;

// a channel's kind code, one byte: none, Distort by mode, Overdrive, Chebyshev
enum Code : uint8_t { C_NONE = 0, C_DIST = 1 /* + dspfx_distort_mode */, C_FUZZ = C_DIST + DSPFX_DIST_FUZZ, C_OVER = 10, C_CHEB = 11, C_COUNT = 12 };

struct ShapeArgs {
    const float *in;             // may be `out`: no __restrict__
    float *out;
    const float *p0, *p1, *p2;   // [N] each: Distort level | Overdrive boost, drive, level | Chebyshev level_pos, level_neg
    const uint8_t *code;         // [N]
    uint32_t N, W, nf;
};

// the lane's channels over a run.  code: the kind with the bypasses folded in (C_NONE: a copy in this kernel).  Chebyshev keeps
// tanh(level_pos) in p2 and tanh(level_neg) in p3
template <int CPL>
struct Lane {
    float p0[CPL], p1[CPL], p2[CPL], p3[CPL];
    uint32_t code[CPL];
};

// kind K on R rows: every value is computed, a channel of kind K keeps the result
template <int K, int CPL, int R>
__device__ __forceinline__ void shape_rows(float (&v)[R][CPL], const Lane<CPL> &s) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const float x = v[i][j];
            float y;
            if constexpr (K == C_OVER) y = dspfx::overdrive1(x, s.p0[j], s.p1[j], s.p2[j]);
            else if constexpr (K == C_CHEB) y = dspfx::chebyshev1(x, s.p0[j], s.p1[j], s.p2[j], s.p3[j]);
            else y = dspfx::distort1<K - C_DIST, false>(x, s.p0[j], 0.0, 0.0);
            v[i][j] = s.code[j] == (uint32_t)K ? y : x;
        }
    }
}

// the kinds in `kinds` (a bit per code, the same in every lane of the wave), one after the other.  HEAVY: the kernel holds the
// bodies that evaluate in f64 (Tanh, Sin, Atan, Overdrive, Chebyshev) too
template <bool HEAVY, int CPL, int R>
__device__ __forceinline__ void shape_kinds(uint32_t kinds, float (&v)[R][CPL], const Lane<CPL> &s) {
    while (kinds) {
        const int k = __builtin_ctz(kinds);
        kinds &= kinds - 1;
        switch (k) {
        case C_DIST + DSPFX_DIST_HARD_CLIP: shape_rows<C_DIST + DSPFX_DIST_HARD_CLIP, CPL, R>(v, s); break;
        case C_DIST + DSPFX_DIST_SOFT_CLIP: shape_rows<C_DIST + DSPFX_DIST_SOFT_CLIP, CPL, R>(v, s); break;
        case C_DIST + DSPFX_DIST_TANH: if constexpr (HEAVY) shape_rows<C_DIST + DSPFX_DIST_TANH, CPL, R>(v, s); break;
        case C_DIST + DSPFX_DIST_RECIP_SOFT_CLIP: shape_rows<C_DIST + DSPFX_DIST_RECIP_SOFT_CLIP, CPL, R>(v, s); break;
        case C_DIST + DSPFX_DIST_SIN: if constexpr (HEAVY) shape_rows<C_DIST + DSPFX_DIST_SIN, CPL, R>(v, s); break;
        case C_DIST + DSPFX_DIST_ATAN: if constexpr (HEAVY) shape_rows<C_DIST + DSPFX_DIST_ATAN, CPL, R>(v, s); break;
        case C_DIST + DSPFX_DIST_SQUARE: shape_rows<C_DIST + DSPFX_DIST_SQUARE, CPL, R>(v, s); break;
        case C_DIST + DSPFX_DIST_CHEBYSHEV4: shape_rows<C_DIST + DSPFX_DIST_CHEBYSHEV4, CPL, R>(v, s); break;
        case C_OVER: if constexpr (HEAVY) shape_rows<C_OVER, CPL, R>(v, s); break;
        case C_CHEB: if constexpr (HEAVY) shape_rows<C_CHEB, CPL, R>(v, s); break;
        default: break;
        }
    }
}

// HEAVY = false: for tables without a kind that evaluates in f64 (the host knows); those bodies' constants and temporaries cost
// 85 VGPRs, which a bank of arithmetic kinds does not pay
template <int CPL, bool HEAVY>
__global__ __launch_bounds__(SWG) void shapers_run(ShapeArgs a) {
    constexpr int F = 8;                                   // frame rows per chunk (two chunks are in registers)
    uint32_t c;
    if (!lane_channel<CPL>(SWG, a.N, c)) return;
    Lane<CPL> s;
    uint8_t code[CPL];
    loadv<CPL>(a.p0 + c, s.p0);
    loadv<CPL>(a.p1 + c, s.p1);
    loadv<CPL>(a.p2 + c, s.p2);
    loadv<CPL>(a.code + c, code);
    // the bypasses are the reference's: Distort (every mode but Fuzz) and Overdrive return the sample when level < 0.001, which a
    // NaN level is not; Chebyshev bypasses per branch inside chebyshev1.  Fuzz has the second kernel
    uint32_t kinds = 0;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        uint32_t k = code[j];
        if (k >= C_DIST && k < C_OVER && (k == C_FUZZ || s.p0[j] < 0.001f)) k = C_NONE;
        if (k == C_OVER && s.p2[j] < 0.001f) k = C_NONE;
        s.code[j] = k;
        s.p3[j] = 0.0f;
    }
#pragma unroll
    for (uint32_t k = C_DIST; k < C_COUNT; ++k) {
        bool mine = false;
#pragma unroll
        for (int j = 0; j < CPL; ++j) mine |= s.code[j] == k;
        if (__ballot(mine)) kinds |= 1u << k;              // (the lanes that returned above are not asked)
    }
    kinds = __builtin_amdgcn_readfirstlane(kinds);
    if (HEAVY && (kinds & (1u << C_CHEB))) {               // chebyshev.rs:52-62: the denominators, once per run (the engine: per chunk)
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const float tp = dspfx::tanh_cr(s.p0[j]), tn = dspfx::tanh_cr(s.p1[j]);
            if (s.code[j] == C_CHEB) {
                s.p2[j] = tp;
                s.p3[j] = tn;
            }
        }
    }
    const size_t lane0 = lay(0, c, a.nf, a.N, a.W), rs = a.W ? a.W : a.N;
    const float *lin = a.in + lane0;
    float *lout = a.out + lane0;
    each_chunk<CPL, F>(lin, lout, rs, a.nf, [&](auto &v, uint32_t) LANE_BODY { shape_kinds<HEAVY>(kinds, v, s); });
}

// ---- Fuzz ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }

// distort.rs:146-172 with fuzz_kernel's arithmetic and order (aux_kernels.hip), no link hop and no control port: wave q holds frames
// [32q, 32q + 32) of 64 channels (lane = channel).  In place on `out`; nf % 128 == 0 (the host refuses anything else)
constexpr int FZ_CH = 64, FZ_Q = SWG / FZ_CH, FZ_F = 128 / FZ_Q;
__global__ __launch_bounds__(SWG) void shapers_fuzz(float *out, const float *level, const uint8_t *code, uint32_t N, uint32_t W, uint32_t nf) {
    __shared__ unsigned smax[3][FZ_Q][FZ_CH];
    const int lane = threadIdx.x & (FZ_CH - 1), q = __builtin_amdgcn_readfirstlane(threadIdx.x / FZ_CH);
    const uint64_t c64 = (uint64_t)blockIdx.x * FZ_CH + lane;
    const bool fz = c64 < N && code[c64] == C_FUZZ;
    if (!__ballot(fz)) return;                             // the same 64 bytes in all four waves: they all leave, or none does
    const uint32_t c = fz ? (uint32_t)c64 : 0;
    float *p = out + lay(0, c, nf, N, W);
    const size_t rs = W ? W : N;
    const float lv = fz ? level[c] : 0.0f;
    auto wg_max = [&](int which, unsigned mine) {          // max of the four waves' partial maxima, per channel
        smax[which][q][lane] = mine;
        __syncthreads();
        unsigned m = smax[which][0][lane];
#pragma unroll
        for (int k = 1; k < FZ_Q; ++k) m = smax[which][k][lane] >= m ? smax[which][k][lane] : m;
        return m;
    };
    for (uint32_t b0 = 0; b0 < nf; b0 += 128) {
        float x[FZ_F];
        const uint32_t f0 = b0 + q * FZ_F;
        unsigned m = 0;
#pragma unroll
        for (int f = 0; f < FZ_F; ++f) {
            x[f] = fz ? __builtin_nontemporal_load(p + (size_t)(f0 + f) * rs) : 0.0f;
            const unsigned bts = abs_bits(x[f]);           // max_by(total_cmp) over |x| == integer max of the bits
            m = bts >= m ? bts : m;
        }
        const float mx = __uint_as_float(wg_max(0, m));
        const double rmx = 1.0 / (double)mx;
        unsigned mzb = 0;
#pragma unroll
        for (int f = 0; f < FZ_F; ++f) {
            const float qv = dspfx::div_lane(dspfx::clip1(x[f] * lv), mx, rmx);      // 158
            const float e = dspfx::exp_cr(-fabsf(qv));                               // q.copysign(-1.0).exp()
            const float z = -fabsf(1.0f - e);                                        // (1.0 - e).copysign(-1.0)
            x[f] = z;
            const unsigned bts = abs_bits(z);
            mzb = bts >= mzb ? bts : mzb;
        }
        const float mz = __uint_as_float(wg_max(1, mzb));
        const double rmz = 1.0 / (double)mz;
        unsigned myb = 0;
#pragma unroll
        for (int f = 0; f < FZ_F; ++f) {
            const float y = dspfx::div_lane(dspfx::clip1(x[f] * mx), mz, rmz);       // 167
            x[f] = y;
            const unsigned bts = abs_bits(y);
            myb = bts >= myb ? bts : myb;
        }
        const float my = __uint_as_float(wg_max(2, myb));
        const double rmy = 1.0 / (double)my;
        if (fz) {
#pragma unroll
            for (int f = 0; f < FZ_F; ++f) __builtin_nontemporal_store(dspfx::div_lane(x[f] * mx, my, rmy), p + (size_t)(f0 + f) * rs);   // 171
        }
        __syncthreads();                                   // smax is reused by the next 128-frame block
    }
}

thread_local std::string g_err;        // the reason of the last failed create or plan on this thread

enum StoreKind : uint32_t { ST_NODES, ST_DROP };

// a store's vals: NODES three runs of [count] sliders (p0, p1, p2), then [count] kind codes as bytes; DROP carries none
struct StoreFields {
    StoreKind kind = ST_DROP;
    uint32_t first = 0, count = 0;
};
typedef StoreQueue<StoreFields> Stores;
typedef Stores::Store Store;

bool heavy(uint8_t k) { return k == C_DIST + DSPFX_DIST_TANH || k == C_DIST + DSPFX_DIST_SIN || k == C_DIST + DSPFX_DIST_ATAN || k == C_OVER || k == C_CHEB; }
uint32_t code_kind(uint8_t k) { return k == C_NONE ? DSPFX_SHAPERS_NONE : k == C_OVER ? DSPFX_OVERDRIVE : k == C_CHEB ? DSPFX_CHEBYSHEV : DSPFX_DISTORT; }
uint32_t code_mode(uint8_t k) { return k >= C_DIST && k < C_OVER ? (uint32_t)(k - C_DIST) : DSPFX_SHAPERS_NONE; }

}  // namespace

struct dspfx_shapers : ChannelBank<dspfx_shapers_desc, StoreFields> {        // mu: also rcode, run_fuzz and run_heavy
    static constexpr const char *name = "shapers";
    std::vector<float> hp[3];                    // [N] each: the sliders with every store made so far
    std::vector<uint8_t> hcode;                  // [N]: ... and the kind codes
    // what the device tables hold once the stores DRAINED so far have run -- not the stores made so far: the second launch and
    // the n_frames % 128 refusal of a run go by these, so a drop queued behind the run's drain cannot cancel its Fuzz pass
    std::vector<uint8_t> rcode;                  // [N]
    uint64_t run_fuzz = 0;                       // the Fuzz channels in rcode
    uint64_t run_heavy = 0;                      // ... and those of a kind that evaluates in f64: which run kernel
    float *p[3] = {nullptr, nullptr, nullptr};
    uint8_t *code = nullptr;
    // the fresh state: no node anywhere
    template <class V>
    static void tables(const dspfx_shapers_desc &d, V v) {
        for (int t = 0; t < 3; ++t) v(4 * (uint64_t)d.n_channels, 0, &dspfx_shapers::p, t);
        v(d.n_channels, C_NONE, &dspfx_shapers::code);
    }
};

namespace {

// one store onto the stream (the bank's mu is held): the device tables, and the run-order kind table beside them
hipError_t apply_store(dspfx_shapers *p, const Store &st, hipStream_t s) {
    const size_t n = st.count, bytes = n * sizeof(float);
    const uint8_t *codes = st.kind == ST_NODES ? (const uint8_t *)(st.vals + 3 * n) : nullptr;
    for (size_t i = 0; i < n; ++i) {
        uint8_t &r = p->rcode[st.first + i];
        const uint8_t k = codes ? codes[i] : (uint8_t)C_NONE;
        p->run_fuzz += (uint64_t)(k == C_FUZZ) - (uint64_t)(r == C_FUZZ);
        p->run_heavy += (uint64_t)heavy(k) - (uint64_t)heavy(r);
        r = k;
    }
    if (st.kind == ST_DROP) return hipMemsetAsync(p->code + st.first, C_NONE, n, s);
    hipError_t err = hipSuccess;
    for (int t = 0; t < 3 && err == hipSuccess; ++t) err = hipMemcpyAsync(p->p[t] + st.first, st.vals + t * n, bytes, hipMemcpyHostToDevice, s);
    if (err == hipSuccess) err = hipMemcpyAsync(p->code + st.first, codes, n, hipMemcpyHostToDevice, s);
    return err;
}

// a store of one family over a range: vals[t] (NULL: keep, or the default where the channel carries another family or none) are the
// family's sliders, modes (Distort only, NULL: keep or the default) its modes
int store_nodes(dspfx_shapers *p, const char *call, int kind, int n_sliders, const float *const (&vals)[3], const uint32_t *modes, uint64_t first,
                uint64_t count) {
    const int rc = check_range(p, call, first, count);
    if (rc != DSPFX_OK) return rc;
    if (modes)
        for (uint64_t i = 0; i < count; ++i)
            if (modes[i] > DSPFX_DIST_CHEBYSHEV4) {
                char buf[192];
                std::snprintf(buf, sizeof buf, "shapers %s: channel %llu is given mode %u, which is no Distort mode (0 .. %d)", call,
                              (unsigned long long)(first + i), modes[i], (int)DSPFX_DIST_CHEBYSHEV4);
                return p->fail(DSPFX_ERR_INVALID, buf);
            }
    if (count == 0) return DSPFX_OK;
    dspfx_node_desc def;
    if (dspfx_node_defaults(kind, &def) != DSPFX_OK) return p->fail(DSPFX_ERR_INVALID, "shapers: no such node kind");
    Store st;
    std::unique_lock<std::mutex> one;
    if (!stage_store(p, st, &one, ST_NODES, call, first, count, 3 * count + (count + 3) / 4, "staged sliders")) return DSPFX_ERR_OOM;
    uint8_t *codes = (uint8_t *)(st.vals + 3 * count);
    for (uint64_t i = 0; i < count; ++i) {
        const uint64_t c = first + i;
        const uint8_t old = p->hcode[c];
        const bool same = code_kind(old) == (uint32_t)kind;      // the family it carries: the sliders left out are kept
        for (int t = 0; t < 3; ++t)
            st.vals[t * count + i] = t >= n_sliders ? 0.0f : vals[t] ? vals[t][i] : same ? p->hp[t][c] : def.params[t];
        if (kind == DSPFX_DISTORT) codes[i] = (uint8_t)(C_DIST + (modes ? modes[i] : same ? code_mode(old) : (uint32_t)def.mode));
        else codes[i] = kind == DSPFX_OVERDRIVE ? C_OVER : C_CHEB;
    }
    p->stores.push(st, [&] {
        for (int t = 0; t < 3; ++t) std::memcpy(p->hp[t].data() + first, st.vals + t * count, count * sizeof(float));
        std::memcpy(p->hcode.data() + first, codes, count);
    });
    return DSPFX_OK;
}

}  // namespace

extern "C" const char *dspfx_shapers_last_error(const dspfx_shapers *p) { return p ? p->err.c_str() : g_err.c_str(); }

extern "C" int dspfx_shapers_plan(uint64_t channels, uint64_t *bytes_out) { return plan_bank<dspfx_shapers>(channels, bytes_out, g_err); }

extern "C" int dspfx_shapers_create(const dspfx_shapers_desc *desc, dspfx_shapers **out) {
    const int rc = create_checks(desc, out, g_err);
    if (rc != DSPFX_OK) return rc;
    return create_bank(desc, out, g_err, [](dspfx_shapers *p) {
        const uint32_t N = p->desc.n_channels;
        for (auto &h : p->hp) h.assign(N, 0.0f);
        p->hcode.assign(N, C_NONE);
        p->rcode.assign(N, C_NONE);
    });
}

extern "C" int dspfx_shapers_destroy(dspfx_shapers *p) { return destroy_bank(p); }

extern "C" int dspfx_shapers_set_distort(dspfx_shapers *p, const float *host_level, const uint32_t *host_mode, uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const float *const vals[3] = {host_level, nullptr, nullptr};
    return store_nodes(p, "set_distort", DSPFX_DISTORT, 1, vals, host_mode, first_channel, count);
}

extern "C" int dspfx_shapers_set_overdrive(dspfx_shapers *p, const float *host_boost, const float *host_drive, const float *host_level,
                                           uint64_t first_channel, uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const float *const vals[3] = {host_boost, host_drive, host_level};
    return store_nodes(p, "set_overdrive", DSPFX_OVERDRIVE, 3, vals, nullptr, first_channel, count);
}

extern "C" int dspfx_shapers_set_chebyshev(dspfx_shapers *p, const float *host_level_pos, const float *host_level_neg, uint64_t first_channel,
                                           uint64_t count) {
    if (!p) return DSPFX_ERR_INVALID;
    const float *const vals[3] = {host_level_pos, host_level_neg, nullptr};
    return store_nodes(p, "set_chebyshev", DSPFX_CHEBYSHEV, 2, vals, nullptr, first_channel, count);
}

extern "C" int dspfx_shapers_drop(dspfx_shapers *p, uint64_t first_channel, uint64_t count) {
    return store_plain(p, ST_DROP, "drop", first_channel, count, [=] {
        for (uint64_t c = first_channel; c < first_channel + count; ++c) {     // a later store meets no node: the defaults again
            p->hp[0][c] = p->hp[1][c] = p->hp[2][c] = 0.0f;
            p->hcode[c] = C_NONE;
        }
    });
}

extern "C" int dspfx_shapers_present(dspfx_shapers *p, uint32_t *host_present_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "present", host_present_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = p->hcode[c] != C_NONE; });
}

extern "C" int dspfx_shapers_kinds(dspfx_shapers *p, uint32_t *host_kinds_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "kinds", host_kinds_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = code_kind(p->hcode[c]); });
}

extern "C" int dspfx_shapers_modes(dspfx_shapers *p, uint32_t *host_modes_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "modes", host_modes_out, first_channel, count, [p](uint32_t *o, uint64_t i, uint64_t c) { o[i] = code_mode(p->hcode[c]); });
}

extern "C" int dspfx_shapers_sliders(dspfx_shapers *p, float *host_sliders_out, uint64_t first_channel, uint64_t count) {
    return read_table(p, "sliders", host_sliders_out, first_channel, count, [p](float *o, uint64_t i, uint64_t c) {
        for (int t = 0; t < 3; ++t) o[3 * i + t] = p->hp[t][c];
    });
}

extern "C" int dspfx_shapers_run(dspfx_shapers *p, const float *in, float *out, uint32_t n_frames, void *stream) {
    if (!p) return DSPFX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    hipStream_t s = (hipStream_t)stream;
    const int rc = begin_run(p, in && out, n_frames, s, "shapers run: in, out or n_frames", "shapers store", apply_store);
    if (rc != DSPFX_OK) return rc;
    // by the tables this run has drained (run_fuzz), not by the stores made so far
    if (p->run_fuzz && n_frames % DSPFX_BUF_SIZE) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "shapers run: Fuzz is block-global over 128 frames and %llu channels carry it: n_frames %u %% 128 != 0",
                      (unsigned long long)p->run_fuzz, n_frames);
        return p->fail(DSPFX_ERR_INVALID, buf);
    }
    ShapeArgs a;
    a.in = in;
    a.out = out;
    a.p0 = p->p[0];
    a.p1 = p->p[1];
    a.p2 = p->p[2];
    a.code = p->code;
    a.N = p->desc.n_channels;
    a.W = p->desc.tile_channels;
    a.nf = n_frames;
    const auto [vec, lanes, blocks] = lane_plan(a.N, a.W, (uintptr_t)in | (uintptr_t)out, SWG);
    if (vec && p->run_heavy) shapers_run<4, true><<<blocks, SWG, 0, s>>>(a);
    else if (vec) shapers_run<4, false><<<blocks, SWG, 0, s>>>(a);
    else if (p->run_heavy) shapers_run<1, true><<<blocks, SWG, 0, s>>>(a);
    else shapers_run<1, false><<<blocks, SWG, 0, s>>>(a);
    BANK_HIP_WHY(hipGetLastError(), "shapers_run");
    if (p->run_fuzz) {
        shapers_fuzz<<<(a.N + FZ_CH - 1) / FZ_CH, SWG, 0, s>>>(out, p->p[0], p->code, a.N, a.W, n_frames);
        BANK_HIP_WHY(hipGetLastError(), "shapers_fuzz");
    }
    return DSPFX_OK;
}
