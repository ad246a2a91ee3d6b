// host_pipe.hip -- the host-buffer form of the process call (dspfx_process_host, and dspfx_process_host_pcm in device sample
// formats: pinned staging, upload / kernel / download of channel windows overlapped) and its allocator.  See engine.h for the split.
#include "engine.h"

using namespace dspfx;
using namespace dspfx_host;


extern "C" int dspfx_host_alloc(size_t bytes, void **out) {
    if (!out || bytes == 0) return DSPFX_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return DSPFX_ERR_NO_DEVICE;
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        *out = nullptr;
        return DSPFX_ERR_OOM;
    }
    return DSPFX_OK;
}

extern "C" int dspfx_host_free(void *p) {
    if (!p) return DSPFX_OK;
    return hipHostFree(p) == hipSuccess ? DSPFX_OK : DSPFX_ERR_HIP;
}

namespace dspfx_host {
bool is_pinned_host(const void *p) {
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeHost;
}
}  // namespace dspfx_host

// PCM staging on the device (dspfx_process_host_pcm): grown to max_frames x N elements of the widest format asked for.  Only the
// host calls use it, and they return with the device idle, so a buffer that is too small is simply replaced.
static int stage_grow(dspfx_engine *e, void **p, size_t *cap, size_t want) {
    if (*cap >= want) return DSPFX_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    HIPCHK(e, hipMalloc(p, want));
    *cap = want;
    return DSPFX_OK;
}

// One block from host buffers, in the formats of `io` ({F32, 1, F32, 1}: dspfx_process_host).  An f32 mono side of the block
// goes through the f32 staging as it always has; any other format crosses the bus as it is and is widened / narrowed on the
// device, next to the f32 staging.  Called with api_mu held and the arguments checked.
static int host_block(dspfx_engine *e, const dspfx_pcm_io &io, const void *in, const void *side, void *out, float *mix,
                      uint32_t n_frames) {
    const size_t cap = (size_t)e->desc.max_frames * e->desc.channels * sizeof(float);
    const bool plain_in = io.in_format == DSPFX_SAMPLE_F32 && io.in_channels == 1;
    const bool plain_out = io.out_format == DSPFX_SAMPLE_F32 && io.out_channels == 1;
    const size_t in_es = pcm_elem_bytes(io.in_format, io.in_channels), out_es = pcm_elem_bytes(io.out_format, io.out_channels);
    if (!e->h_in) HIPCHK(e, hipMalloc((void **)&e->h_in, cap));
    if (!e->h_out) HIPCHK(e, hipMalloc((void **)&e->h_out, cap));
    if (side && !e->h_side) HIPCHK(e, hipMalloc((void **)&e->h_side, cap));
    if (mix && !e->h_mix) HIPCHK(e, hipMalloc((void **)&e->h_mix, e->desc.max_frames * sizeof(float)));
    if (!plain_in) {
        const size_t want = (size_t)e->desc.max_frames * e->desc.channels * in_es;
        if (const int rc = stage_grow(e, &e->p_in, &e->p_in_cap, want)) return rc;
        if (side)
            if (const int rc = stage_grow(e, &e->p_side, &e->p_side_cap, want)) return rc;
    }
    if (!plain_out)
        if (const int rc = stage_grow(e, &e->p_out, &e->p_out_cap, (size_t)e->desc.max_frames * e->desc.channels * out_es)) return rc;
    // where each direction crosses the bus on the device: the f32 staging itself, or the PCM staging beside it
    void *d_in = plain_in ? (void *)e->h_in : e->p_in, *d_side = plain_in ? (void *)e->h_side : e->p_side;
    void *d_out = plain_out ? (void *)e->h_out : e->p_out;
    // Pipelined form: the block is cut into channel parts; while part p runs, part p+1 is uploaded and part p-1
    // downloaded (both directions of the bus busy).  Needs a single fused stage per part (no FIR / Fuzz / mix bus),
    // the frame-major layout and a block that is not split at a short delay line.
    bool fused_only = !e->desc.tile_channels && n_frames <= e->min_delay && !e->has_siggen && !e->collect_due && !e->mp_count;
    for (const Stage &st : e->stages) fused_only = fused_only && st.type == ST_FUSED;
    const uint32_t N = e->desc.channels;
    const uint32_t part = e->env.host_part > 0 ? (uint32_t)e->env.host_part : 65536u;   // channels per part (multiple of 1024); 32k 15.5, 64k 13.7, 128k 14.1, 256k 15.1 ms
    const bool pipe_off = e->env.host_pipeline == 0;
    // page-locked buffers only (dspfx_host_alloc): copies from pageable memory are staged by the runtime and do not overlap
    if (fused_only && !pipe_off && N >= 2 * part && is_pinned_host(in) && is_pinned_host(out) && (!side || is_pinned_host(side))) {
        if (!e->hs_in) {
            HIPCHK(e, hipStreamCreateWithFlags(&e->hs_in, hipStreamNonBlocking));
            HIPCHK(e, hipStreamCreateWithFlags(&e->hs_out, hipStreamNonBlocking));
            HIPCHK(e, hipStreamCreateWithFlags(&e->hs_run, hipStreamNonBlocking));
        }
        {   // the parts run on the engine's own stream: order it behind whatever used the state last -- and the uploads too:
            // dspfx_process_pcm may still be reading the staging on the stream it was given
            const bool elsewhere = e->cur_stream_set && e->cur_stream != e->hs_run;
            const int brc = bind_stream(e, e->hs_run);
            if (brc) return brc;
            if (elsewhere && e->ev_order) HIPCHK(e, hipStreamWaitEvent(e->hs_in, e->ev_order, 0));
        }
        const uint32_t n_parts = (N + part - 1) / part;
        while (e->hev.size() < 2 * (size_t)n_parts) {
            hipEvent_t ev = nullptr;
            HIPCHK(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            e->hev.push_back(ev);
        }
        const size_t in_pitch = (size_t)N * in_es, out_pitch = (size_t)N * out_es;
        const char *h_in = (const char *)in, *h_side = (const char *)side;
        char *h_out = (char *)out;
        int rc = DSPFX_OK;
        for (uint32_t p = 0; p < n_parts && rc == DSPFX_OK; ++p) {
            const uint32_t c0 = p * part, cn = std::min(part, N - c0);
            HIPCHK(e, hipMemcpy2DAsync((char *)d_in + c0 * in_es, in_pitch, h_in + c0 * in_es, in_pitch, cn * in_es, n_frames, hipMemcpyHostToDevice, e->hs_in));
            if (side) HIPCHK(e, hipMemcpy2DAsync((char *)d_side + c0 * in_es, in_pitch, h_side + c0 * in_es, in_pitch, cn * in_es, n_frames, hipMemcpyHostToDevice, e->hs_in));
            HIPCHK(e, hipEventRecord(e->hev[2 * p], e->hs_in));
            HIPCHK(e, hipStreamWaitEvent(e->hs_run, e->hev[2 * p], 0));
            if (!plain_in) {
                HIPCHK(e, launch_pcm_widen(io.in_format, io.in_channels, d_in, e->h_in, n_frames, cn, N, c0, e->hs_run));
                if (side) HIPCHK(e, launch_pcm_widen(io.in_format, io.in_channels, d_side, e->h_side, n_frames, cn, N, c0, e->hs_run));
            }
            BlockCall c(e->h_in, side ? e->h_side : nullptr, e->h_out, nullptr, n_frames, e->hs_run);
            c.window_c0 = c0;
            c.window_n = cn;
            c.window_last = p + 1 == n_parts;
            if (mix) {   // every part leaves its waves' partial sums; reduced once below
                c.bus = BUS_DEFERRED;
                c.partials = e->mixpart;
            }
            rc = run_subblock(e, c);
            if (rc) break;
            if (!plain_out) HIPCHK(e, launch_pcm_narrow(io.out_format, io.out_channels, e->h_out, d_out, n_frames, cn, N, c0, e->hs_run));
            HIPCHK(e, hipEventRecord(e->hev[2 * p + 1], e->hs_run));
            HIPCHK(e, hipStreamWaitEvent(e->hs_out, e->hev[2 * p + 1], 0));
            HIPCHK(e, hipMemcpy2DAsync(h_out + c0 * out_es, out_pitch, (const char *)d_out + c0 * out_es, out_pitch, cn * out_es, n_frames, hipMemcpyDeviceToHost, e->hs_out));
        }
        if (rc == DSPFX_OK && mix) {
            launch_mix_reduce(e->mixpart, e->mixpart_b, e->h_mix, n_frames, e->part_stride[e->flip], e->hs_run);
            HIPCHK(e, hipMemcpyAsync(mix, e->h_mix, n_frames * sizeof(float), hipMemcpyDeviceToHost, e->hs_run));
        }
        (void)hipStreamSynchronize(e->hs_in);
        (void)hipStreamSynchronize(e->hs_run);
        HIPCHK(e, hipStreamSynchronize(e->hs_out));
        if (rc == DSPFX_OK) e->frames_submitted += n_frames;
        return rc;
    }
    // whole block: the uploads below are synchronous copies on the null stream, so the staging must be free there first
    if (const int brc = bind_stream(e, nullptr)) return brc;
    HIPCHK(e, hipMemcpy(d_in, in, (size_t)n_frames * N * in_es, hipMemcpyHostToDevice));
    if (side) HIPCHK(e, hipMemcpy(d_side, side, (size_t)n_frames * N * in_es, hipMemcpyHostToDevice));
    const int rc = dspfx_process_pcm(e, &io, d_in, side ? d_side : nullptr, d_out, mix ? e->h_mix : nullptr, n_frames, nullptr);
    if (rc) return rc;
    HIPCHK(e, hipStreamSynchronize(nullptr));
    HIPCHK(e, hipMemcpy(out, d_out, (size_t)n_frames * N * out_es, hipMemcpyDeviceToHost));
    if (mix) HIPCHK(e, hipMemcpy(mix, e->h_mix, n_frames * sizeof(float), hipMemcpyDeviceToHost));
    return DSPFX_OK;
}

extern "C" int dspfx_process_host(dspfx_engine *e, const float *in, const float *side, float *out, float *mix,
                                  uint32_t n_frames) {
    if (!e) return DSPFX_ERR_INVALID;
    ApiScope api(e);
    if (api.rc) return api.rc;
    if (const int rc = check_block(e, in, out, n_frames)) return rc;
    const dspfx_pcm_io f32{DSPFX_SAMPLE_F32, 1, DSPFX_SAMPLE_F32, 1};
    return host_block(e, f32, in, side, out, mix, n_frames);
}

extern "C" int dspfx_process_host_pcm(dspfx_engine *e, const dspfx_pcm_io *io, const void *in, const void *side, void *out,
                                      float *mix, uint32_t n_frames) {
    if (!e) return DSPFX_ERR_INVALID;
    ApiScope api(e);
    if (api.rc) return api.rc;
    if (const int rc = check_pcm_io(e, io)) return rc;
    if (const int rc = check_block(e, in, out, n_frames)) return rc;
    return host_block(e, *io, in, side, out, mix, n_frames);
}
