// dspfx.hpp -- C++17 host-side mirror of the reference's operator interface over the C ABI (dspfx.h).
//
// The reference is Rust; its toolchain is absent from the build image, so the host layer above the
// C ABI is written in C++ (and mirrored in Python for the tests).  Names, slider fields, ranges and
// defaults follow dsp-stuff/src/nodes/*.rs; `GpuChain::process` has the shape of
// `SimpleNode::process` (dsp-stuff/src/node.rs:135-146): borrowed input slice(s) in, output slice out,
// node-owned parameters and state.  Errors that the reference turns into panics
// (node.rs:173,271,280) become dspfx::Error exceptions here; nothing falls back to the CPU.
#pragma once
#include <cstddef>
#include <array>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "dspfx.h"

namespace dspfx {

struct Error : std::runtime_error {
    int status;
    Error(int st, const std::string &msg) : std::runtime_error("dspfx error " + std::to_string(st) + ": " + msg), status(st) {}
};

constexpr std::size_t BUF_SIZE = DSPFX_BUF_SIZE;   // node.rs:257
constexpr std::uint32_t NO_ROOM = DSPFX_MIXGROUPS_NO_ROOM;                         // MixGroups::assign: the channel sits in no room
constexpr std::uint32_t CONVOLVE_MAX_RESPONSES = DSPFX_CONVOLVE_MAX_RESPONSES;   // the responses one Convolver holds

// nodes/distort.rs:18-28
enum class Mode : int { HardClip = 0, SoftClip, Tanh, RecipSoftClip, Fuzz, Sin, Atan, Square, Chebyshev4 };
// nodes/fir.rs Mode
enum class FirMode : int { Balanced = 0, Average = 1 };

// One node of a chain: the reference node's saved fields.
struct Node {
    dspfx_node_desc d{};
    std::vector<double> taps;   // Fir: time-reversed, as fir.rs:163,168 stores them
};

inline Node make(int kind) {
    Node n;
    if (dspfx_node_defaults(kind, &n.d) != DSPFX_OK) throw Error(DSPFX_ERR_INVALID, "unknown node kind");
    return n;
}
// nodes/gain.rs: slider level 0..=10, default 1.0
inline Node Gain(float level = 1.0f) { Node n = make(DSPFX_GAIN); n.d.params[0] = level; return n; }
// nodes/biquad.rs:18-41: raw sliders -10..=10, normalised by a0 on the engine (biquad.rs:62-76)
inline Node BiQuad(float a0 = 1.0f, float a1 = -0.24f, float a2 = 0.0f, float b0 = 0.758f, float b1 = 0.0f, float b2 = 0.0f) {
    Node n = make(DSPFX_BIQUAD);
    const float p[6] = {a0, a1, a2, b0, b1, b2};
    for (int i = 0; i < 6; ++i) n.d.params[i] = p[i];
    return n;
}
inline Node LowPass(float ratio = 0.5f) { Node n = make(DSPFX_LOW_PASS); n.d.params[0] = ratio; return n; }
inline Node HighPass(float ratio = 0.5f) { Node n = make(DSPFX_HIGH_PASS); n.d.params[0] = ratio; return n; }
// nodes/reverb.rs: a RESTORED node -- refresh_seconds has run (dsp-stuff-derive/src/lib.rs:319-337), the ring has
// reverb.rs:58's length for `seconds`; the seconds slider travels with the node (params[1]) so that a later slider store --
// which swaps in a new zero ring, decay included (reverb.rs:19, 55-71) -- refreshes to the same length
inline Node Reverb(float seconds = 0.5f, float decay = 0.5f, bool page_round = false) {
    Node n = make(DSPFX_REVERB);
    n.d.params[0] = decay;
    n.d.params[1] = seconds;
    n.d.mode = page_round ? 1 : 0;
    n.d.delay_len = dspfx_delay_len(seconds, page_round ? 1 : 0);
    return n;
}
// a node fresh from the menu: make_buffer()'s ring under the 0.5 s slider (reverb.rs:44-52) = dspfx_node_defaults: 128 samples,
// or 1024 under the page-rounded reading of rivulet (make_buffer() is refresh_seconds' three calls with 128 for num_samples)
inline Node ReverbFresh(bool page_round = false) {
    Node n = make(DSPFX_REVERB);
    n.d.mode = page_round ? 1 : 0;
    n.d.delay_len = dspfx_delay_len(0.0f, page_round ? 1 : 0);
    return n;
}
// an explicit ring and no seconds slider: a slider store swaps in a zero ring of the same length
inline Node ReverbSamples(std::uint32_t delay_len, float decay = 0.5f) {
    Node n = make(DSPFX_REVERB);
    n.d.params[0] = decay;
    n.d.params[1] = 0.0f;
    n.d.delay_len = delay_len;
    return n;
}
// nodes/distort.rs: level 0..=30 default 0 (bypass), mode default SoftClip
inline Node Distort(float level = 0.0f, Mode mode = Mode::SoftClip) {
    Node n = make(DSPFX_DISTORT);
    n.d.params[0] = level;
    n.d.mode = static_cast<int>(mode);
    return n;
}
inline Node Overdrive(float boost = 0.0f, float drive = 0.0f, float level = 0.0f) {
    Node n = make(DSPFX_OVERDRIVE);
    n.d.params[0] = boost; n.d.params[1] = drive; n.d.params[2] = level;
    return n;
}
inline Node Chebyshev(float level_pos = 0.0f, float level_neg = 0.0f) {
    Node n = make(DSPFX_CHEBYSHEV);
    n.d.params[0] = level_pos; n.d.params[1] = level_neg;
    return n;
}
// nodes/fir.rs: impulse response h[0..T) in natural order; stored reversed like fir.rs:163,168
inline Node Fir(const std::vector<double> &impulse_response, FirMode mode = FirMode::Balanced) {
    Node n = make(DSPFX_FIR);
    n.taps.assign(impulse_response.rbegin(), impulse_response.rend());
    n.d.mode = static_cast<int>(mode);
    return n;
}
inline Node Add() { return make(DSPFX_ADD); }
inline Node Mix(float ratio = 0.5f) { Node n = make(DSPFX_MIX); n.d.params[0] = ratio; return n; }
// nodes/envelope.rs:27-30: peak envelope follower, attack / release in frames
inline Node Envelope(float attack = 0.0f, float release = 0.0f) {
    Node n = make(DSPFX_ENVELOPE);
    n.d.params[0] = attack; n.d.params[1] = release;
    return n;
}
// nodes/signal_gen.rs:41-55: a source (no "in" port) -- as a chain node it replaces the signal
enum class SignalMode : int { Sine = DSPFX_SIG_SINE, Triangle = DSPFX_SIG_TRIANGLE, Square = DSPFX_SIG_SQUARE, Constant = DSPFX_SIG_CONSTANT };
inline Node SignalGen(float amplitude = 0.5f, float frequency = 100.0f, SignalMode mode = SignalMode::Sine) {
    Node n = make(DSPFX_SIGNAL_GEN);
    n.d.params[0] = amplitude; n.d.params[1] = frequency;
    n.d.mode = static_cast<int>(mode);
    return n;
}

// The translation unit Engine::set_graph would compile for this graph (dspfx.h: dspfx_graph_source); needs no device.
inline std::string graph_source(const std::vector<Node> &nodes, const std::vector<dspfx_graph_link> &links) {
    std::vector<dspfx_node_desc> d;
    for (const Node &n : nodes) d.push_back(n.d);
    std::string out(std::size_t{1} << 18, '\0');
    const int rc = dspfx_graph_source(d.data(), static_cast<int>(d.size()), links.data(), static_cast<int>(links.size()),
                                      out.data(), out.size());
    if (rc != DSPFX_OK) throw Error(rc, dspfx_strerror(rc));
    out.resize(std::strlen(out.c_str()));
    return out;
}

// N independent mono channels through one chain.
class Engine {
  public:
    Engine(std::uint32_t channels, std::uint32_t max_frames = DSPFX_BUF_SIZE,
           std::uint32_t link_flags = DSPFX_LINK_INTERNAL | DSPFX_LINK_INPUT, int device = 0,
           std::uint32_t tile_channels = 0, std::uint64_t channel_offset = 0)
        : channels_(channels) {
        dspfx_engine_desc d{DSPFX_ABI_VERSION, device, channels, max_frames, link_flags, tile_channels, channel_offset};
        const int rc = dspfx_engine_create(&d, &e_);
        if (rc != DSPFX_OK) throw Error(rc, dspfx_strerror(rc));
    }
    ~Engine() { dspfx_engine_destroy(e_); }
    Engine(const Engine &) = delete;
    Engine &operator=(const Engine &) = delete;
    Engine(Engine &&o) noexcept : e_(std::exchange(o.e_, nullptr)), channels_(o.channels_) {}

    void set_chain(const std::vector<Node> &nodes) {
        std::vector<dspfx_node_desc> d;
        for (const Node &n : nodes) {
            d.push_back(n.d);
            if (n.d.kind == DSPFX_FIR) {
                d.back().taps = n.taps.data();
                d.back().n_taps = static_cast<std::uint32_t>(n.taps.size());
            }
        }
        chk(dspfx_chain_set(e_, d.data(), static_cast<int>(d.size())));
    }
    // specialised kernels are compiled in the background and adopted at a block boundary: wait for them (dspfx.h)
    bool kernels_ready(int wait_ms = 60000) {
        const int rc = dspfx_kernels_ready(e_, wait_ms);
        if (rc < 0) chk(rc);
        return rc == 1;
    }
    // a whole DAG as one generated kernel (dspfx.h, dspfx_graph_set); Error::status == DSPFX_ERR_UNSUPPORTED when it cannot be fused
    void set_graph(const std::vector<Node> &nodes, const std::vector<dspfx_graph_link> &links) {
        std::vector<dspfx_node_desc> d;
        for (const Node &n : nodes) d.push_back(n.d);
        chk(dspfx_graph_set(e_, d.data(), static_cast<int>(d.size()), links.data(), static_cast<int>(links.size())));
    }
    // Slider / mode stores are safe from another thread while this one is inside process(): queued, applied at the next
    // block boundary in order (dspfx.h, "threads").  set_param_seq returns the store's sequence number, param_log where
    // the stores took effect.
    void set_param(int node, int param, float v) { chk(dspfx_set_param(e_, node, param, v)); }
    std::uint64_t set_param_seq(int node, int param, float v) {
        std::uint64_t seq = 0;
        chk(dspfx_set_param_seq(e_, node, param, v, &seq));
        return seq;
    }
    void set_mode(int node, Mode m) { chk(dspfx_set_mode(e_, node, static_cast<int>(m))); }
    std::vector<dspfx_param_event> param_log(std::uint64_t after_seq = 0) {
        std::vector<dspfx_param_event> ev(4096);
        const int n = dspfx_param_log(e_, ev.data(), static_cast<int>(ev.size()), after_seq);
        if (n < 0) chk(n);
        ev.resize(static_cast<std::size_t>(n));
        return ev;
    }
    std::uint64_t frames_submitted() const { return dspfx_frames_submitted(e_); }
    void set_delay_len(int node, std::uint32_t d) { chk(dspfx_set_delay_len(e_, node, d)); }
    void reserve_delay_len(int node, std::uint32_t d) { chk(dspfx_reserve_delay_len(e_, node, d)); }   // capacity hint (any thread)
    void ring_trim() { chk(dspfx_ring_trim(e_)); }
    /// DSPFX_FIR_PRECISION_DEFAULT / _F32 / _SPLIT / _HALF: how a FIR node's steady-state sweep multiplies (dspfx.h)
    void set_fir_precision(int node, dspfx_fir_precision p) { chk(dspfx_set_fir_precision(e_, node, static_cast<int>(p))); }
    void reset() { chk(dspfx_reset(e_)); }
    // device buffers, asynchronous on `stream`
    void process(const float *in, float *out, std::uint32_t n_frames, const float *side = nullptr,
                 float *mix = nullptr, void *stream = nullptr) {
        chk(dspfx_process(e_, in, side, out, mix, n_frames, stream));
    }
    // the Output node in the same launch: mix = this block's bus / link_divisor(n_connected) (0: the un-normalised sum)
    void process_bus(const float *in, float *out, float *mix, std::uint32_t n_frames, std::uint64_t n_connected,
                     const float *side = nullptr, void *stream = nullptr) {
        chk(dspfx_process_bus(e_, in, side, out, mix, n_frames, n_connected, stream));
    }
    // host buffers ([n_frames][channels]), synchronous
    void process_host(const float *in, float *out, std::uint32_t n_frames, const float *side = nullptr,
                      float *mix = nullptr) {
        chk(dspfx_process_host(e_, in, side, out, mix, n_frames));
    }
    // device sample formats at the boundary (dspfx.h: dspfx_pcm_io); `mix` stays f32.  Device buffers, asynchronous on `stream`
    void process_pcm(const dspfx_pcm_io &io, const void *in, void *out, std::uint32_t n_frames, const void *side = nullptr,
                     float *mix = nullptr, void *stream = nullptr) {
        chk(dspfx_process_pcm(e_, &io, in, side, out, mix, n_frames, stream));
    }
    // ... host buffers, synchronous
    void process_host_pcm(const dspfx_pcm_io &io, const void *in, void *out, std::uint32_t n_frames, const void *side = nullptr,
                          float *mix = nullptr) {
        chk(dspfx_process_host_pcm(e_, &io, in, side, out, mix, n_frames));
    }
    void mix_finish(float *mix, std::uint32_t n_frames, std::uint64_t n_connected, void *stream = nullptr) {
        chk(dspfx_mix_finish(e_, mix, n_frames, n_connected, stream));
    }
    // the mix bus across GPUs: sum this rank's un-normalised bus over the communicator's ranks (ONE RCCL all-reduce of
    // n_frames floats, in place, asynchronous on `stream`), then the Output hop with the GLOBAL channel count
    void mix_allreduce(dspfx_comm *comm, float *mix, std::uint32_t n_frames, std::uint64_t n_connected, void *stream = nullptr) {
        chk(dspfx_mix_allreduce(e_, comm, mix, n_frames, n_connected, stream));
    }
    // re-tune the delay rings' placement against the buffers the host will keep using (DSP state is kept)
    void tune_placement(const float *in, float *out, std::uint32_t n_frames, const float *side = nullptr, void *stream = nullptr) {
        chk(dspfx_tune_placement(e_, in, side, out, n_frames, stream));
    }
    // collect_and_average over several pipes (node.rs:162-194): dst = (0 + srcs...) / f32(0.0001 + n)
    void link_average(const std::vector<const float *> &srcs, float *dst, std::uint32_t n_frames, void *stream = nullptr) {
        chk(dspfx_link_average(e_, srcs.data(), static_cast<int>(srcs.size()), dst, n_frames, stream));
    }
    std::uint32_t channels() const { return channels_; }
    dspfx_engine *raw() { return e_; }

  private:
    void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, dspfx_last_error(e_));
    }
    dspfx_engine *e_ = nullptr;
    std::uint32_t channels_;
};

// The mix bus' communicator: one per process / GPU (include/dspfx.h).  Rank 0 calls Comm::unique_id() and hands the
// bytes to every rank over the host's own channel; every rank then constructs its Comm (collective).
class Comm {
  public:
    using Id = std::array<unsigned char, DSPFX_COMM_ID_BYTES>;
    static Id unique_id() {
        Id id{};
        const int rc = dspfx_comm_unique_id(id.data());
        if (rc != DSPFX_OK) throw Error(rc, dspfx_comm_last_error(nullptr));
        return id;
    }
    Comm(int device, int n_ranks, int rank, const Id *id = nullptr) {
        const int rc = dspfx_comm_create(device, n_ranks, rank, id ? id->data() : nullptr, &c_);
        if (rc != DSPFX_OK) throw Error(rc, dspfx_comm_last_error(nullptr));
    }
    ~Comm() { dspfx_comm_destroy(c_); }
    Comm(const Comm &) = delete;
    Comm &operator=(const Comm &) = delete;
    int size() const { return dspfx_comm_size(c_); }
    int rank() const { return dspfx_comm_rank(c_); }
    dspfx_comm *raw() { return c_; }

  private:
    dspfx_comm *c_ = nullptr;
};

// Reference-shaped node: what a `GpuChain: SimpleNode` in the Rust host does per block.
// process(input, output) takes one 128-frame block per channel bank laid out [frame][channel]
// (channels == 1 reproduces the reference's mono node exactly); the host's Perform wrapper has
// already averaged the input pipes (node.rs:290-299), so only the hops BETWEEN the fused nodes are
// applied here (DSPFX_LINK_INTERNAL).
class GpuChain {
  public:
    GpuChain(std::vector<Node> chain, std::uint32_t channels = 1, int device = 0)
        : eng_(channels, DSPFX_BUF_SIZE, DSPFX_LINK_INTERNAL, device) {
        eng_.set_chain(chain);
    }
    static const char *title() { return "GPU chain"; }
    static const char *cfg_name() { return "gpu_chain"; }
    void process(const float *input, float *output, std::size_t n_frames = BUF_SIZE) {
        eng_.process_host(input, output, static_cast<std::uint32_t>(n_frames));
    }
    Engine &engine() { return eng_; }

  private:
    Engine eng_;
};

// The Pitch Detector node (nodes/pitch.rs) for N channels (include/dspfx.h, dspfx_pitch_*): device blocks in the layout of
// tile_channels, a McLeod pitch and clarity per channel for every 1024 frames, held until the next window that gives one.
class PitchBank {
  public:
    enum Param : int { Power = DSPFX_PITCH_POWER, Clarity = DSPFX_PITCH_CLARITY, Pick = DSPFX_PITCH_PICK };
    explicit PitchBank(std::uint32_t channels, int device = 0, std::uint32_t tile_channels = 0, float power_thresh = 0.5f,
                       float clarity_thresh = 0.5f, float pick_thresh = 0.5f) {
        const dspfx_pitch_desc d{DSPFX_ABI_VERSION, device, channels, tile_channels, power_thresh, clarity_thresh, pick_thresh};
        chk(dspfx_pitch_create(&d, &p_));
    }
    ~PitchBank() { dspfx_pitch_destroy(p_); }
    PitchBank(const PitchBank &) = delete;
    PitchBank &operator=(const PitchBank &) = delete;
    // device block of n_frames; asynchronous on `stream`.  push(slot(), 128) copies nothing.
    void push(const float *block, std::uint32_t n_frames, void *stream = nullptr) { chk(dspfx_pitch_push(p_, block, n_frames, stream)); }
    float *slot() { return dspfx_pitch_slot(p_); }
    void set_param(Param which, float value) { chk(dspfx_pitch_set_param(p_, which, value)); }
    // device arrays freq[N], clarity[N]
    void read(float *freq, float *clarity, void *stream = nullptr) { chk(dspfx_pitch_read(p_, freq, clarity, stream)); }
    void reset() { chk(dspfx_pitch_reset(p_)); }
    std::int64_t windows() const { return dspfx_pitch_windows(p_); }
    dspfx_pitch *raw() { return p_; }

  private:
    static void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, dspfx_strerror(rc));
    }
    dspfx_pitch *p_ = nullptr;
};

// The output resampler bank (include/dspfx.h, dspfx_resample_*): the reference's output callback (devices.rs:394-498) for N
// channels whose device runs at target_hz.  Engine output goes into a FIFO of block_frames-frame slots; pull() is one callback.
class Resampler {
  public:
    struct Pulled {
        std::uint32_t consumed;   // frames released from the FIFO
        bool underrun;            // fewer than input_len frames were waiting: `out` is silence, nothing was consumed
    };
    Resampler(std::uint32_t channels, std::uint32_t target_hz, int device = 0, std::uint32_t tile_channels = 0,
              std::uint32_t block_frames = DSPFX_BUF_SIZE, std::uint32_t slots = 4, int out_format = DSPFX_SAMPLE_F32,
              int out_channels = 1) {
        const dspfx_resample_desc d{DSPFX_ABI_VERSION, device, channels, tile_channels, block_frames, slots, target_hz, out_format, out_channels};
        chk(dspfx_resample_create(&d, &r_));
    }
    ~Resampler() { dspfx_resample_destroy(r_); }
    Resampler(const Resampler &) = delete;
    Resampler &operator=(const Resampler &) = delete;
    // device block of n_frames; asynchronous on `stream`.  push(slot(), block_frames) copies nothing.  A full FIFO throws (DSPFX_ERR_STATE).
    void push(const float *block, std::uint32_t n_frames, void *stream = nullptr) { chk(dspfx_resample_push(r_, block, n_frames, stream)); }
    float *slot() { return dspfx_resample_slot(r_); }
    // n_out device frames of every channel into the device buffer `out`, in the bank's layout and format
    Pulled pull(void *out, std::uint32_t n_out, void *stream = nullptr) {
        std::uint32_t consumed = 0;
        std::int32_t underrun = 0;
        chk(dspfx_resample_pull(r_, out, n_out, &consumed, &underrun, stream));
        return Pulled{consumed, underrun != 0};
    }
    std::int64_t available() { return dspfx_resample_available(r_); }
    void skip(std::uint32_t n_frames) { chk(dspfx_resample_skip(r_, n_frames)); }
    void reset() { chk(dspfx_resample_reset(r_)); }
    dspfx_resample *raw() { return r_; }

  private:
    static void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, dspfx_strerror(rc));
    }
    dspfx_resample *r_ = nullptr;
};

// The Spectrogram node (nodes/spectrogram.rs) for N channels (include/dspfx.h, dspfx_spectrum_*): device blocks in the layout of
// tile_channels; every fft_size frames one column vol[k] = |FFT(window * x)[k]| * gain[k], k < fft_size / 2, per channel, the
// newest `columns` kept on the device.  window / gain: host tables copied at construction, nullptr = Hann / 1.0.
class SpectrumBank {
  public:
    explicit SpectrumBank(std::uint32_t channels, std::uint32_t fft_size = 512, std::uint32_t columns = 1, int device = 0,
                          std::uint32_t tile_channels = 0, const float *window = nullptr, const float *gain = nullptr) {
        const dspfx_spectrum_desc d{DSPFX_ABI_VERSION, device, channels, tile_channels, fft_size, columns, window, gain};
        chk(dspfx_spectrum_create(&d, &p_));
    }
    ~SpectrumBank() { dspfx_spectrum_destroy(p_); }
    SpectrumBank(const SpectrumBank &) = delete;
    SpectrumBank &operator=(const SpectrumBank &) = delete;
    // device block of n_frames; asynchronous on `stream`.  push(slot(), 128) copies nothing.
    void push(const float *block, std::uint32_t n_frames, void *stream = nullptr) { chk(dspfx_spectrum_push(p_, block, n_frames, stream)); }
    float *slot() { return dspfx_spectrum_slot(p_); }
    // the device column `age` windows back (fft_size / 2 frames of N channels in the bank's layout), nullptr when there is none
    const float *column(std::uint32_t age = 0) { return dspfx_spectrum_column(p_, age); }
    void reset() { chk(dspfx_spectrum_reset(p_)); }
    std::int64_t windows() const { return dspfx_spectrum_windows(p_); }
    dspfx_spectrum *raw() { return p_; }

  private:
    static void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, dspfx_strerror(rc));
    }
    dspfx_spectrum *p_ = nullptr;
};

// The default window table and the bin frequencies k * 48000 / fft_size (dspfx_spectrum_plan: a pure host function, no GPU).
struct SpectrumPlan {
    std::vector<float> window;                    // [fft_size]
    std::vector<float> bin_hz;                    // [fft_size / 2]
};
inline SpectrumPlan spectrum_plan(std::uint32_t fft_size) {
    SpectrumPlan p;
    if (fft_size <= DSPFX_SPECTRUM_MAX_FFT) {
        p.window.resize(fft_size);
        p.bin_hz.resize(fft_size / 2);
    }
    const int rc = dspfx_spectrum_plan(fft_size, p.window.data(), p.bin_hz.data());
    if (rc != DSPFX_OK) throw Error(rc, dspfx_strerror(rc));
    return p;
}

// The converter's plan for the next n_out output frames (dspfx_resample_plan: a pure host function, no GPU).
struct ResamplePlan {
    std::vector<std::uint32_t> advance, depth;
    std::vector<double> coeff;                    // [n_out][16]
    std::uint32_t input_len = 0, pulled = 0;
};
inline ResamplePlan resample_plan(std::uint32_t target_hz, double &value, std::uint32_t &idx, std::uint32_t n_out) {
    ResamplePlan p;
    p.advance.resize(n_out);
    p.depth.resize(n_out);
    p.coeff.resize((std::size_t)n_out * 16);
    const int rc = dspfx_resample_plan(target_hz, &value, &idx, n_out, p.advance.data(), p.depth.data(), p.coeff.data(), &p.input_len, &p.pulled);
    if (rc != DSPFX_OK) throw Error(rc, dspfx_strerror(rc));
    return p;
}

// One Output bus per contiguous channel range, with a per-channel fader (include/dspfx.h, dspfx_mixgroups_*):
// buses[f][g] = (sum over group g of fl32(x[f][c] * gain[c])) / link_divisor(n_g) for a device block in the layout of
// tile_channels.  group_start: G + 1 channel indices, nondecreasing from 0 to N (copied).  The buses, [n_frames][G] on the device,
// are the frame-major block of a G-channel Engine, Resampler, PitchBank or SpectrumBank.
class MixGroups {
  public:
    MixGroups(std::uint32_t channels, const std::vector<std::uint64_t> &group_start, std::uint32_t tile_channels = 0,
              std::uint32_t max_frames = DSPFX_BUF_SIZE, bool normalise = true, int device = 0)
        : groups_(group_start.empty() ? 0 : (std::uint32_t)group_start.size() - 1) {
        const dspfx_mixgroups_desc d{DSPFX_ABI_VERSION, device, channels, max_frames, tile_channels, groups_, normalise ? 1u : 0u,
                                     group_start.data()};
        const int rc = dspfx_mixgroups_create(&d, &p_);
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_mixgroups_last_error(nullptr) ? dspfx_mixgroups_last_error(nullptr) : dspfx_strerror(rc));
    }
    ~MixGroups() { dspfx_mixgroups_destroy(p_); }
    MixGroups(const MixGroups &) = delete;
    MixGroups &operator=(const MixGroups &) = delete;
    std::uint32_t groups() const { return groups_; }
    // device block of n_frames -> device buses [n_frames][G]; asynchronous on `stream`
    void run(const float *block, std::uint32_t n_frames, float *buses, void *stream = nullptr) { chk(dspfx_mixgroups_run(p_, block, n_frames, buses, stream)); }
    // every channel's room minus itself: returns[f][c] = (S[f][g] - t[f][c]) / link_divisor(n_g - 1), in the block's layout
    // (returns == block: in place); buses may be nullptr, else it receives what run() writes (dspfx_mixgroups_returns)
    void returns(const float *block, std::uint32_t n_frames, float *buses, float *returns, void *stream = nullptr) {
        chk(dspfx_mixgroups_returns(p_, block, n_frames, buses, returns, stream));
    }
    // faders of channels [first_channel, first_channel + count) from a host array; nullptr drops them.  Any thread; never waits.
    void set_gains(const float *host_values, std::uint64_t first_channel, std::uint64_t count) {
        chk(dspfx_mixgroups_set_gains(p_, host_values, first_channel, count));
    }
    // seating (dspfx_mixgroups_assign): the rooms of channels [first_channel, first_channel + ids.size()), each < groups() or
    // NO_ROOM; a bad id or range stores nothing.  Any thread; holds for the runs submitted after it returns, and the channels'
    // faders (and their state in the engine) stay where they are
    void assign(const std::vector<std::uint32_t> &ids, std::uint64_t first_channel = 0) {
        chk(dspfx_mixgroups_assign(p_, ids.data(), first_channel, ids.size()));
    }
    void assign(std::uint32_t id, std::uint64_t first_channel) { chk(dspfx_mixgroups_assign(p_, &id, first_channel, 1)); }
    // the room of each of `count` channels from first_channel, as the next run sees them
    std::vector<std::uint32_t> room_of(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> ids(count);
        chk(dspfx_mixgroups_rooms(p_, ids.data(), first_channel, count));
        return ids;
    }
    dspfx_mixgroups *raw() { return p_; }

  private:
    void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_mixgroups_last_error(p_) ? dspfx_mixgroups_last_error(p_) : dspfx_strerror(rc));
    }
    dspfx_mixgroups *p_ = nullptr;
    std::uint32_t groups_;
};

// Checks a group table and gives, per group, the longest chain of dependent f32 additions in its sum (dspfx_mixgroups_plan: a
// pure host function, no GPU).
inline std::vector<std::uint32_t> mixgroups_plan(const std::vector<std::uint64_t> &group_start, std::uint64_t channels,
                                                 std::uint32_t tile_channels = 0) {
    std::vector<std::uint32_t> depth(group_start.empty() ? 0 : group_start.size() - 1);
    const int rc = dspfx_mixgroups_plan(group_start.data(), (std::uint32_t)depth.size(), channels, tile_channels, depth.data());
    if (rc != DSPFX_OK) throw Error(rc, dspfx_mixgroups_last_error(nullptr));
    return depth;
}

// Checks a map (a room id or NO_ROOM per channel) and gives, per room, its member count, the depth D of its sum in mapped mode
// and its pieces (dspfx_mixgroups_room_plan: a pure host function, no GPU).
struct RoomPlan {
    std::vector<std::uint64_t> count;
    std::vector<std::uint32_t> depth;
    std::vector<std::uint64_t> pieces;
};
inline RoomPlan mixgroups_room_plan(const std::vector<std::uint32_t> &room_of, std::uint32_t groups, std::uint32_t tile_channels = 0) {
    RoomPlan r{std::vector<std::uint64_t>(groups), std::vector<std::uint32_t>(groups), std::vector<std::uint64_t>(groups)};
    const int rc = dspfx_mixgroups_room_plan(room_of.data(), room_of.size(), groups, tile_channels, r.count.data(), r.depth.data(), r.pieces.data());
    if (rc != DSPFX_OK) throw Error(rc, dspfx_mixgroups_last_error(nullptr));
    return r;
}

// Per-channel Gain and BiQuad sliders (include/dspfx.h, dspfx_strips_*): the strip of channel c is a chain of up to 1 + bands
// optional nodes in a fixed order -- a Gain node, then BiQuad bands 0 .. bands-1 -- each with the channel's own slider values,
// over a device block in the layout of tile_channels.  A node exists for a channel from the first store that names it until it
// is dropped (nullptr); a fresh bank copies its input.  Between Engine::process and MixGroups::run / returns, or ahead of the chain.
class ChannelStrips {
  public:
    ChannelStrips(std::uint32_t channels, std::uint32_t bands = 1, std::uint32_t tile_channels = 0,
                  std::uint32_t max_frames = DSPFX_BUF_SIZE, std::uint32_t link_flags = 0, int device = 0)
        : bands_(bands) {
        const dspfx_strips_desc d{DSPFX_ABI_VERSION, device, channels, max_frames, tile_channels, bands, link_flags};
        const int rc = dspfx_strips_create(&d, &p_);
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_strips_last_error(nullptr) ? dspfx_strips_last_error(nullptr) : dspfx_strerror(rc));
    }
    ~ChannelStrips() { dspfx_strips_destroy(p_); }
    ChannelStrips(const ChannelStrips &) = delete;
    ChannelStrips &operator=(const ChannelStrips &) = delete;
    std::uint32_t bands() const { return bands_; }
    // device block of n_frames -> device block in the same layout (out == in: in place); asynchronous on `stream`
    void run(const float *in, float *out, std::uint32_t n_frames, void *stream = nullptr) { chk(dspfx_strips_run(p_, in, out, n_frames, stream)); }
    // Gain levels of channels [first_channel, first_channel + count) from a host array; nullptr drops the node.  Any thread; never waits.
    void set_gain(const float *host_levels, std::uint64_t first_channel, std::uint64_t count) {
        chk(dspfx_strips_set_gain(p_, host_levels, first_channel, count));
    }
    // band `band` of those channels from [count][6] raw sliders a0, a1, a2, b0, b1, b2; nullptr drops the band.  The store zeroes the
    // band's state on exactly those channels (the reference's after_settings_change).  Any thread; never waits.
    void set_band(std::uint32_t band, const float *host_raw6, std::uint64_t first_channel, std::uint64_t count) {
        chk(dspfx_strips_set_band(p_, band, host_raw6, first_channel, count));
    }
    // zero all state, keep the sliders and the nodes
    void reset() { chk(dspfx_strips_reset(p_)); }
    // the node mask of each of `count` channels from first_channel, as the next run sees it: bit 0 = Gain, bit 1 + b = band b
    std::vector<std::uint32_t> present(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_strips_present(p_, m.data(), first_channel, count));
        return m;
    }
    dspfx_strips *raw() { return p_; }

  private:
    void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_strips_last_error(p_) ? dspfx_strips_last_error(p_) : dspfx_strerror(rc));
    }
    dspfx_strips *p_ = nullptr;
    std::uint32_t bands_;
};

// The five normalised coefficients a1, a2, b0, b1, b2 of six raw BiQuad sliders exactly as the device gets them
// (dspfx_strips_coeffs: a pure host function, no GPU).
inline std::vector<float> strips_coeffs(const float (&raw6)[6]) {
    std::vector<float> k(5);
    const int rc = dspfx_strips_coeffs(raw6, k.data());
    if (rc != DSPFX_OK) throw Error(rc, dspfx_strerror(rc));
    return k;
}

// Per-channel Reverb (feedback delay) sliders (include/dspfx.h, dspfx_delays_*): channel c may carry one Reverb node with its own
// seconds and decay and its own ring of dspfx_delay_len(seconds, page_round) frames, over a device block in the layout of
// tile_channels.  A node exists for a channel from the first store that names it until it is dropped; a fresh bank copies its
// input.  Every store is the reference's slider change: the stored channels start again from a zero ring.  max_seconds sizes the
// rings (delays_plan).  Where ChannelStrips goes: between Engine::process and the room mixes.
class ChannelDelays {
  public:
    ChannelDelays(std::uint32_t channels, float max_seconds = 0.5f, std::uint32_t tile_channels = 0, std::uint32_t max_frames = DSPFX_BUF_SIZE,
                  std::uint32_t link_flags = 0, bool page_round = false, int device = 0) {
        const dspfx_delays_desc d{DSPFX_ABI_VERSION, device, channels, max_frames, tile_channels, max_seconds, page_round ? 1u : 0u, link_flags};
        const int rc = dspfx_delays_create(&d, &p_);
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_delays_last_error(nullptr) ? dspfx_delays_last_error(nullptr) : dspfx_strerror(rc));
    }
    ~ChannelDelays() { dspfx_delays_destroy(p_); }
    ChannelDelays(const ChannelDelays &) = delete;
    ChannelDelays &operator=(const ChannelDelays &) = delete;
    // device block of n_frames -> device block in the same layout (out == in: in place); asynchronous on `stream`
    void run(const float *in, float *out, std::uint32_t n_frames, void *stream = nullptr) { chk(dspfx_delays_run(p_, in, out, n_frames, stream)); }
    // the sliders of channels [first_channel, first_channel + count) from host arrays; a nullptr slider keeps each channel's value, both
    // nullptr drop the node.  Refused whole when a channel would need more than the bank's ring.  Any thread; never waits.
    void set_delay(const float *host_seconds, const float *host_decay, std::uint64_t first_channel, std::uint64_t count) {
        chk(dspfx_delays_set_delay(p_, host_seconds, host_decay, first_channel, count));
    }
    // every present channel's ring back to zeros, the sliders and the nodes kept
    void reset() { chk(dspfx_delays_reset(p_)); }
    // 1 / 0 per channel: it carries a node; and each channel's ring length, 0 where there is none -- as all stores so far left them
    std::vector<std::uint32_t> present(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_delays_present(p_, m.data(), first_channel, count));
        return m;
    }
    std::vector<std::uint32_t> lengths(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_delays_lengths(p_, m.data(), first_channel, count));
        return m;
    }
    dspfx_delays *raw() { return p_; }

  private:
    void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_delays_last_error(p_) ? dspfx_delays_last_error(p_) : dspfx_strerror(rc));
    }
    dspfx_delays *p_ = nullptr;
};

// The ring frames per channel and the ring bytes of a ChannelDelays bank (dspfx_delays_plan: a pure host function, no GPU).
struct DelaysPlan {
    std::uint32_t cap;
    std::uint64_t bytes;
};
inline DelaysPlan delays_plan(std::uint64_t channels, float max_seconds = 0.5f, bool page_round = false) {
    DelaysPlan r{0, 0};
    const int rc = dspfx_delays_plan(channels, max_seconds, page_round ? 1 : 0, &r.cap, &r.bytes);
    if (rc != DSPFX_OK) throw Error(rc, dspfx_delays_last_error(nullptr));
    return r;
}

// Per-channel levels and each room's loudest, gated live (include/dspfx.h, dspfx_talkers_*): every channel has its own Envelope node
// (attack and release in frames), every room -- rooms as MixGroups takes them, 1 .. DSPFX_TALKERS_MAX_ROOM members, reseated live by
// assign() -- gets its `top` loudest members chosen on the device, and run() passes those members and ramps the others out.  A run
// gates with the targets the run before left, then meters, then selects: a selection is audible one block later, and a fresh bank
// copies its first block.  Between ChannelStrips / ChannelDelays and the room mixes.
class Talkers {
  public:
    struct Views {
        const float *level;            // [N]
        const float *target;           // [N]
        const std::int32_t *talkers;   // [G][8], -1 where there is none
        const float *talker_levels;    // [G][8]
    };
    Talkers(std::uint32_t channels, const std::vector<std::uint64_t> &group_start, std::uint32_t top = 3, std::uint32_t tile_channels = 0,
            std::uint32_t max_frames = DSPFX_BUF_SIZE, int device = 0)
        : groups_((std::uint32_t)(group_start.empty() ? 0 : group_start.size() - 1)) {
        const dspfx_talkers_desc d{DSPFX_ABI_VERSION, device, channels, max_frames, tile_channels, groups_, top, group_start.data()};
        const int rc = dspfx_talkers_create(&d, &p_);
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_talkers_last_error(nullptr) ? dspfx_talkers_last_error(nullptr) : dspfx_strerror(rc));
    }
    ~Talkers() { dspfx_talkers_destroy(p_); }
    Talkers(const Talkers &) = delete;
    Talkers &operator=(const Talkers &) = delete;
    // device block of n_frames -> device block in the same layout (out == in: in place; out == nullptr: meter and select only, the
    // gates stay); asynchronous on `stream`
    void run(const float *in, float *out, std::uint32_t n_frames, void *stream = nullptr) { chk(dspfx_talkers_run(p_, in, out, n_frames, stream)); }
    // the rooms of channels [first_channel, first_channel + ids.size()): each below the bank's rooms, or DSPFX_TALKERS_NO_ROOM.  Refused
    // whole on a bad id or a room that would exceed DSPFX_TALKERS_MAX_ROOM.  Any thread; never waits.
    void assign(const std::vector<std::uint32_t> &ids, std::uint64_t first_channel) { chk(dspfx_talkers_assign(p_, ids.data(), first_channel, ids.size())); }
    // attack and release (frames) from host arrays; a nullptr slider keeps each channel's value.  No envelope is touched
    void set_detector(const float *host_attack, const float *host_release, std::uint64_t first_channel, std::uint64_t count) {
        chk(dspfx_talkers_set_detector(p_, host_attack, host_release, first_channel, count));
    }
    // DSPFX_TALKERS_AUTO, _OPEN (always passed, never ranked) or _SHUT (never passed) per channel
    void set_pin(const std::vector<std::uint8_t> &pins, std::uint64_t first_channel) { chk(dspfx_talkers_set_pin(p_, pins.data(), first_channel, pins.size())); }
    // 1 .. DSPFX_TALKERS_MAX_TOP per room
    void set_top(const std::vector<std::uint8_t> &tops, std::uint64_t first_room) { chk(dspfx_talkers_set_top(p_, tops.data(), first_room, tops.size())); }
    void set_floor(float floor) { chk(dspfx_talkers_set_floor(p_, floor)); }
    // envelope and level back to 0, gate and target to 1 on the range; queued like a store
    void reset(std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_talkers_reset(p_, first_channel, count)); }
    // the device tables: valid after a run, on its stream
    Views views() {
        Views v{nullptr, nullptr, nullptr, nullptr};
        chk(dspfx_talkers_views(p_, &v.level, &v.target, &v.talkers, &v.talker_levels));
        return v;
    }
    // the audible list on the device: room r's members whose gate or target was not +-0.0 when the last gated run began -- the only
    // ones that can be non-zero in the block it gated -- in ascending channel order, are list[start[r] .. start[r] + count[r]).  The
    // first call allocates list and count and switches the bank on: every gated run submitted after it also writes them.  Stable
    // pointers; valid after a gated run, on its stream.  What MixMatrix::run_sparse takes
    struct Audible {
        const std::int32_t *list;      // [N]
        const std::uint32_t *start;    // [G + 1]
        const std::uint32_t *count;    // [G]
    };
    Audible audible() {
        Audible v{nullptr, nullptr, nullptr};
        chk(dspfx_talkers_audible_views(p_, &v.list, &v.start, &v.count));
        return v;
    }
    // every channel's room and every room's member count, by every assign made so far
    std::vector<std::uint32_t> room_of(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_talkers_room_of(p_, m.data(), first_channel, count));
        return m;
    }
    std::vector<std::uint32_t> counts() {
        std::vector<std::uint32_t> m(groups_);
        chk(dspfx_talkers_counts(p_, m.data()));
        return m;
    }
    dspfx_talkers *raw() { return p_; }

  private:
    void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_talkers_last_error(p_) ? dspfx_talkers_last_error(p_) : dspfx_strerror(rc));
    }
    dspfx_talkers *p_ = nullptr;
    std::uint32_t groups_ = 0;
};

// The device bytes of a Talkers bank's tables (dspfx_talkers_plan: a pure host function, no GPU).
inline std::uint64_t talkers_plan(std::uint64_t channels, std::uint32_t groups) {
    std::uint64_t bytes = 0;
    const int rc = dspfx_talkers_plan(channels, groups, &bytes);
    if (rc != DSPFX_OK) throw Error(rc, dspfx_talkers_last_error(nullptr));
    return bytes;
}

// Per-channel levellers and limiters (include/dspfx.h, dspfx_dynamics_*): channel c may carry its own Envelope node (attack and
// release in frames) feeding its own gain computer, q = env > threshold ? threshold / env : 1, out = in * (makeup * q), over a
// device block in the layout of tile_channels.  A node exists for a channel from the first set() that names it until drop(); a
// fresh bank copies its input.  A limiter: threshold = the ceiling, makeup 1, attack 0 (a brick wall).  A leveller towards `target`
// with at most `max_gain`: threshold = target / max_gain, makeup = max_gain.  Ahead of Talkers as a leveller, behind the room mixes
// as a limiter.
class ChannelDynamics {
  public:
    struct Views {
        const float *level;            // [N]: the block's largest envelope, 0 without a node
        const float *reduction;        // [N]: the block's smallest q, 1 where the channel was never turned down
    };
    ChannelDynamics(std::uint32_t channels, std::uint32_t tile_channels = 0, std::uint32_t max_frames = DSPFX_BUF_SIZE, int device = 0) {
        const dspfx_dynamics_desc d{DSPFX_ABI_VERSION, device, channels, max_frames, tile_channels};
        const int rc = dspfx_dynamics_create(&d, &p_);
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_dynamics_last_error(nullptr) ? dspfx_dynamics_last_error(nullptr) : dspfx_strerror(rc));
    }
    ~ChannelDynamics() { dspfx_dynamics_destroy(p_); }
    ChannelDynamics(const ChannelDynamics &) = delete;
    ChannelDynamics &operator=(const ChannelDynamics &) = delete;
    // device block of n_frames -> device block in the same layout (out == in: in place); key, a device block of the same shape or
    // nullptr, is what the detector follows instead of `in`; asynchronous on `stream`
    void run(const float *in, float *out, std::uint32_t n_frames, const float *key = nullptr, void *stream = nullptr) {
        chk(dspfx_dynamics_run(p_, in, key, out, n_frames, stream));
    }
    // the sliders of channels [first_channel, first_channel + count) from host arrays, and a node for each of them; a nullptr slider
    // keeps each channel's value.  No envelope is touched.  Refused whole on a threshold that is NaN or below +0.0 or a makeup that is
    // NaN, infinite or negative.  Any thread; never waits
    void set(const float *host_threshold, const float *host_makeup, const float *host_attack, const float *host_release, std::uint64_t first_channel,
             std::uint64_t count) {
        chk(dspfx_dynamics_set(p_, host_threshold, host_makeup, host_attack, host_release, first_channel, count));
    }
    // the node removed and its envelope cleared; queued like a store
    void drop(std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_dynamics_drop(p_, first_channel, count)); }
    // envelope and level back to 0 and reduction to 1 on the range, the sliders and the nodes kept; queued like a store
    void reset(std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_dynamics_reset(p_, first_channel, count)); }
    // 1 / 0 per channel: it carries a node, as all stores so far left it
    std::vector<std::uint32_t> present(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_dynamics_present(p_, m.data(), first_channel, count));
        return m;
    }
    // the device tables: valid after a run, on its stream
    Views views() {
        Views v{nullptr, nullptr};
        chk(dspfx_dynamics_views(p_, &v.level, &v.reduction));
        return v;
    }
    dspfx_dynamics *raw() { return p_; }

  private:
    void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_dynamics_last_error(p_) ? dspfx_dynamics_last_error(p_) : dspfx_strerror(rc));
    }
    dspfx_dynamics *p_ = nullptr;
};

// The device bytes of a ChannelDynamics bank's tables (dspfx_dynamics_plan: a pure host function, no GPU).
inline std::uint64_t dynamics_plan(std::uint64_t channels) {
    std::uint64_t bytes = 0;
    const int rc = dspfx_dynamics_plan(channels, &bytes);
    if (rc != DSPFX_OK) throw Error(rc, dspfx_dynamics_last_error(nullptr));
    return bytes;
}

// makeup * q, the factor a ChannelDynamics run multiplies the sample by for this envelope value (dspfx_dynamics_gain: a pure host function).
inline float dynamics_gain(float env, float threshold, float makeup = 1.0f, float *q_out = nullptr) {
    return dspfx_dynamics_gain(env, threshold, makeup, q_out);
}

// Per-channel waveshapers (include/dspfx.h, dspfx_shapers_*): channel c may carry one node of its own -- Distort with its own level
// and mode (Fuzz included), Overdrive or Chebyshev with their own sliders -- over a device block in the layout of tile_channels; its
// output is bit for bit what an engine whose chain is that node writes for it.  A node exists for a channel from the first set_*()
// that names it until drop(); a fresh bank copies its input.  A set_*() of another family than the channel carries replaces its
// node from the reference's defaults; one of the same family keeps the sliders passed as nullptr.  While a channel carries Fuzz,
// n_frames must be a multiple of DSPFX_BUF_SIZE.  Several shapers per channel are several banks.
class ChannelShapers {
  public:
    ChannelShapers(std::uint32_t channels, std::uint32_t tile_channels = 0, std::uint32_t max_frames = DSPFX_BUF_SIZE, int device = 0) {
        const dspfx_shapers_desc d{DSPFX_ABI_VERSION, device, channels, max_frames, tile_channels};
        const int rc = dspfx_shapers_create(&d, &p_);
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_shapers_last_error(nullptr) ? dspfx_shapers_last_error(nullptr) : dspfx_strerror(rc));
    }
    ~ChannelShapers() { dspfx_shapers_destroy(p_); }
    ChannelShapers(const ChannelShapers &) = delete;
    ChannelShapers &operator=(const ChannelShapers &) = delete;
    // device block of n_frames -> device block in the same layout (out == in: in place); asynchronous on `stream`
    void run(const float *in, float *out, std::uint32_t n_frames, void *stream = nullptr) { chk(dspfx_shapers_run(p_, in, out, n_frames, stream)); }
    // a node for each of channels [first_channel, first_channel + count) from host arrays; an unknown mode refuses the whole store.
    // Any thread; never waits
    void set_distort(const float *host_level, const std::uint32_t *host_mode, std::uint64_t first_channel, std::uint64_t count) {
        chk(dspfx_shapers_set_distort(p_, host_level, host_mode, first_channel, count));
    }
    void set_overdrive(const float *host_boost, const float *host_drive, const float *host_level, std::uint64_t first_channel, std::uint64_t count) {
        chk(dspfx_shapers_set_overdrive(p_, host_boost, host_drive, host_level, first_channel, count));
    }
    void set_chebyshev(const float *host_level_pos, const float *host_level_neg, std::uint64_t first_channel, std::uint64_t count) {
        chk(dspfx_shapers_set_chebyshev(p_, host_level_pos, host_level_neg, first_channel, count));
    }
    // the node removed: a copy again; queued like a store
    void drop(std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_shapers_drop(p_, first_channel, count)); }
    // the host tables, as all stores so far left them: 1 / 0; DSPFX_DISTORT .. or DSPFX_SHAPERS_NONE; a Distort node's mode or
    // DSPFX_SHAPERS_NONE; [count][3] sliders
    std::vector<std::uint32_t> present(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_shapers_present(p_, m.data(), first_channel, count));
        return m;
    }
    std::vector<std::uint32_t> kinds(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_shapers_kinds(p_, m.data(), first_channel, count));
        return m;
    }
    std::vector<std::uint32_t> modes(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_shapers_modes(p_, m.data(), first_channel, count));
        return m;
    }
    std::vector<float> sliders(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<float> m(3 * count);
        chk(dspfx_shapers_sliders(p_, m.data(), first_channel, count));
        return m;
    }
    dspfx_shapers *raw() { return p_; }

  private:
    void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_shapers_last_error(p_) ? dspfx_shapers_last_error(p_) : dspfx_strerror(rc));
    }
    dspfx_shapers *p_ = nullptr;
};

// The device bytes of a ChannelShapers bank's tables (dspfx_shapers_plan: a pure host function, no GPU).
inline std::uint64_t shapers_plan(std::uint64_t channels) {
    std::uint64_t bytes = 0;
    const int rc = dspfx_shapers_plan(channels, &bytes);
    if (rc != DSPFX_OK) throw Error(rc, dspfx_shapers_last_error(nullptr));
    return bytes;
}

// Per-channel one-pole filters and envelope followers (include/dspfx.h, dspfx_filters_*): channel c owns `stages` slots (1 .. 4),
// run in slot order, each empty or a LowPass, a HighPass or an Envelope node (whose output is the envelope) with its own sliders,
// over a device block in the layout of tile_channels; its output is bit for bit what an engine whose chain is its present nodes in
// slot order writes for it, however the frames are cut into runs.  A slot's node is new (state +0.0; ratio 0.5, attack 0, release 0
// for a slider passed as nullptr) from the first set_*() that names it and after a set_*() of another kind; a set_*() of the kind
// it carries keeps the sliders passed as nullptr and keeps the state.  A fresh bank copies its input.
class ChannelFilters {
  public:
    ChannelFilters(std::uint32_t channels, std::uint32_t stages = 1, std::uint32_t tile_channels = 0, std::uint32_t max_frames = DSPFX_BUF_SIZE,
                   int device = 0) {
        const dspfx_filters_desc d{DSPFX_ABI_VERSION, device, channels, max_frames, tile_channels, stages};
        const int rc = dspfx_filters_create(&d, &p_);
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_filters_last_error(nullptr) ? dspfx_filters_last_error(nullptr) : dspfx_strerror(rc));
    }
    ~ChannelFilters() { dspfx_filters_destroy(p_); }
    ChannelFilters(const ChannelFilters &) = delete;
    ChannelFilters &operator=(const ChannelFilters &) = delete;
    // device block of n_frames -> device block in the same layout (out == in: in place); asynchronous on `stream`
    void run(const float *in, float *out, std::uint32_t n_frames, void *stream = nullptr) { chk(dspfx_filters_run(p_, in, out, n_frames, stream)); }
    // a node in slot `stage` of channels [first_channel, first_channel + count) from host arrays; a stage that is not one of the
    // bank's refuses the whole store.  Any thread; never waits
    void set_low_pass(std::uint32_t stage, const float *host_ratio, std::uint64_t first_channel, std::uint64_t count) {
        chk(dspfx_filters_set_low_pass(p_, stage, host_ratio, first_channel, count));
    }
    void set_high_pass(std::uint32_t stage, const float *host_ratio, std::uint64_t first_channel, std::uint64_t count) {
        chk(dspfx_filters_set_high_pass(p_, stage, host_ratio, first_channel, count));
    }
    void set_envelope(std::uint32_t stage, const float *host_attack, const float *host_release, std::uint64_t first_channel, std::uint64_t count) {
        chk(dspfx_filters_set_envelope(p_, stage, host_attack, host_release, first_channel, count));
    }
    // the slot emptied and its state zeroed: that stage copies again; queued like a store
    void drop(std::uint32_t stage, std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_filters_drop(p_, stage, first_channel, count)); }
    // the state of slot `stage` (DSPFX_FILTERS_NONE: of every slot) back to +0.0; nodes and sliders stay; queued like a store
    void reset(std::uint64_t first_channel, std::uint64_t count, std::uint32_t stage = DSPFX_FILTERS_NONE) {
        chk(dspfx_filters_reset(p_, stage, first_channel, count));
    }
    // the host tables, as all stores so far left them: 1 / 0 (a slot of the channel carries a node); slot `stage`'s DSPFX_LOW_PASS ..
    // or DSPFX_FILTERS_NONE; its [count][2] sliders as given (ratio, 0 | attack, release)
    std::vector<std::uint32_t> present(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_filters_present(p_, m.data(), first_channel, count));
        return m;
    }
    std::vector<std::uint32_t> kinds(std::uint32_t stage, std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_filters_kinds(p_, stage, m.data(), first_channel, count));
        return m;
    }
    std::vector<float> sliders(std::uint32_t stage, std::uint64_t first_channel, std::uint64_t count) {
        std::vector<float> m(2 * count);
        chk(dspfx_filters_sliders(p_, stage, m.data(), first_channel, count));
        return m;
    }
    // slot `stage`'s state[channels] on the device: z or the envelope after the last run, on its stream
    const float *state(std::uint32_t stage) {
        const float *z = nullptr;
        chk(dspfx_filters_state(p_, stage, &z));
        return z;
    }
    dspfx_filters *raw() { return p_; }

  private:
    void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_filters_last_error(p_) ? dspfx_filters_last_error(p_) : dspfx_strerror(rc));
    }
    dspfx_filters *p_ = nullptr;
};

// The device bytes of a ChannelFilters bank's tables (dspfx_filters_plan: a pure host function, no GPU).
inline std::uint64_t filters_plan(std::uint64_t channels, std::uint32_t stages) {
    std::uint64_t bytes = 0;
    const int rc = dspfx_filters_plan(channels, stages, &bytes);
    if (rc != DSPFX_OK) throw Error(rc, dspfx_filters_last_error(nullptr));
    return bytes;
}

// A per-channel chain of mixed nodes in one pass (include/dspfx.h, dspfx_racks_*): channel c owns `slots` slots (1 .. 4), run in slot
// order, each empty or any one of Gain, BiQuad, LowPass, HighPass, Envelope, Distort (every mode but Fuzz), Overdrive and Chebyshev
// with its own sliders and state, over a device block in the layout of tile_channels; all slots run between one load and one store
// of the block.  Its output and state are bit for bit what ChannelFilters(1 stage), ChannelStrips(1 band) and ChannelShapers give
// when they are run slot after slot with the slot's node on that channel.  A set() of a kind the slot does not carry makes a new
// node (state +0.0, dspfx_node_defaults for a slider passed as nullptr); a set() of the kind it carries keeps what is nullptr,
// keeps the state of LowPass, HighPass and Envelope and zeroes a BiQuad's.  A fresh bank copies its input.
class ChannelRacks {
  public:
    ChannelRacks(std::uint32_t channels, std::uint32_t slots = DSPFX_RACKS_MAX_SLOTS, std::uint32_t tile_channels = 0,
                 std::uint32_t max_frames = DSPFX_BUF_SIZE, int device = 0) {
        const dspfx_racks_desc d{DSPFX_ABI_VERSION, device, channels, max_frames, tile_channels, slots};
        const int rc = dspfx_racks_create(&d, &p_);
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_racks_last_error(nullptr) ? dspfx_racks_last_error(nullptr) : dspfx_strerror(rc));
    }
    ~ChannelRacks() { dspfx_racks_destroy(p_); }
    ChannelRacks(const ChannelRacks &) = delete;
    ChannelRacks &operator=(const ChannelRacks &) = delete;
    // device block of n_frames -> device block in the same layout (out == in: in place); asynchronous on `stream`
    void run(const float *in, float *out, std::uint32_t n_frames, void *stream = nullptr) { chk(dspfx_racks_run(p_, in, out, n_frames, stream)); }
    // a node of `kind` (a dspfx_kind) in slot `slot` of channels [first_channel, first_channel + count): host_sliders is nullptr or six
    // pointers in the order of dspfx_node_desc.params, each nullptr or `count` values; host_mode is nullptr or `count` DSPFX_DIST_*
    // values (Distort).  A slot that is not one of the bank's, a kind that is no rack node, an unknown mode or Fuzz refuses the
    // whole store.  Any thread; never waits
    void set(std::uint32_t slot, std::uint32_t kind, const float *const *host_sliders, const std::uint32_t *host_mode, std::uint64_t first_channel,
             std::uint64_t count) {
        chk(dspfx_racks_set(p_, slot, kind, host_sliders, host_mode, first_channel, count));
    }
    // the slot emptied and its state zeroed: that slot copies again; queued like a store
    void drop(std::uint32_t slot, std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_racks_drop(p_, slot, first_channel, count)); }
    // the state of slot `slot` (DSPFX_RACKS_NONE: of every slot) back to +0.0; nodes and sliders stay; queued like a store
    void reset(std::uint64_t first_channel, std::uint64_t count, std::uint32_t slot = DSPFX_RACKS_NONE) {
        chk(dspfx_racks_reset(p_, slot, first_channel, count));
    }
    // the host tables, as all stores so far left them: a bit per slot that carries a node; slot `slot`'s dspfx_kind or
    // DSPFX_RACKS_NONE; its Distort mode or DSPFX_RACKS_NONE; its [count][6] raw sliders as given
    std::vector<std::uint32_t> present(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_racks_present(p_, m.data(), first_channel, count));
        return m;
    }
    std::vector<std::uint32_t> kinds(std::uint32_t slot, std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_racks_kinds(p_, slot, m.data(), first_channel, count));
        return m;
    }
    std::vector<std::uint32_t> modes(std::uint32_t slot, std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_racks_modes(p_, slot, m.data(), first_channel, count));
        return m;
    }
    std::vector<float> sliders(std::uint32_t slot, std::uint64_t first_channel, std::uint64_t count) {
        std::vector<float> m(6 * count);
        chk(dspfx_racks_sliders(p_, slot, m.data(), first_channel, count));
        return m;
    }
    // slot `slot`'s state[4][channels] on the device after the last run, on its stream: row 0 z or the envelope, rows 0 .. 3 a
    // BiQuad's x1, x2, y1, y2
    const float *state(std::uint32_t slot) {
        const float *z = nullptr;
        chk(dspfx_racks_state(p_, slot, &z));
        return z;
    }
    dspfx_racks *raw() { return p_; }

  private:
    void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_racks_last_error(p_) ? dspfx_racks_last_error(p_) : dspfx_strerror(rc));
    }
    dspfx_racks *p_ = nullptr;
};

// The device bytes of a ChannelRacks bank's tables (dspfx_racks_plan: a pure host function, no GPU).
inline std::uint64_t racks_plan(std::uint64_t channels, std::uint32_t slots) {
    std::uint64_t bytes = 0;
    const int rc = dspfx_racks_plan(channels, slots, &bytes);
    if (rc != DSPFX_OK) throw Error(rc, dspfx_racks_last_error(nullptr));
    return bytes;
}

// Per-channel FIR nodes (include/dspfx.h, dspfx_firs_*): channel c may carry one FIR node of its own -- its own taps (f64), tap
// count T (1 .. max_taps), mode and deque of past samples -- over a device block in the layout of tile_channels; its output is bit
// for bit what the reference's node gives through all its history.  A node exists from the first set_taps() that names the channel
// until drop(); set_taps() on a channel that carries a node is the reference's reload: new taps, the deque is kept.  A fresh bank
// copies its input.
class ChannelFirs {
  public:
    ChannelFirs(std::uint32_t channels, std::uint32_t max_taps = 64, std::uint32_t tile_channels = 0, std::uint32_t max_frames = DSPFX_BUF_SIZE,
                int device = 0, bool general_only = false) : max_taps_(max_taps) {
        const dspfx_firs_desc d{DSPFX_ABI_VERSION, device, channels, max_frames, tile_channels, max_taps, general_only ? 1u : 0u};
        const int rc = dspfx_firs_create(&d, &p_);
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_firs_last_error(nullptr) ? dspfx_firs_last_error(nullptr) : dspfx_strerror(rc));
    }
    ~ChannelFirs() { dspfx_firs_destroy(p_); }
    ChannelFirs(const ChannelFirs &) = delete;
    ChannelFirs &operator=(const ChannelFirs &) = delete;
    // device block of n_frames -> device block in the same layout (out == in: in place); asynchronous on `stream`
    void run(const float *in, float *out, std::uint32_t n_frames, void *stream = nullptr) { chk(dspfx_firs_run(p_, in, out, n_frames, stream)); }
    // one response (time order) for channels [first_channel, first_channel + count); mode DSPFX_FIR_BALANCED, DSPFX_FIR_AVERAGE, or
    // DSPFX_FIRS_NONE to keep the node's.  Any thread; never waits
    void set_taps(const std::vector<double> &response, std::uint64_t first_channel, std::uint64_t count, std::uint32_t mode = DSPFX_FIRS_NONE) {
        chk(dspfx_firs_set_taps(p_, response.data(), (std::uint32_t)response.size(), 0, mode, first_channel, count));
    }
    // a response per channel: host_rows is [count][n_taps]
    void set_taps_rows(const double *host_rows, std::uint32_t n_taps, std::uint64_t first_channel, std::uint64_t count,
                       std::uint32_t mode = DSPFX_FIRS_NONE) {
        chk(dspfx_firs_set_taps(p_, host_rows, n_taps, 1, mode, first_channel, count));
    }
    void set_mode(std::uint32_t mode, std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_firs_set_mode(p_, mode, first_channel, count)); }
    // the node removed: a copy again, a later set_taps() makes a new node; queued like a store
    void drop(std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_firs_drop(p_, first_channel, count)); }
    // the deque emptied; taps and mode stay; queued like a store
    void reset(std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_firs_reset(p_, first_channel, count)); }
    // the host tables, as all stores so far left them: 1 / 0; T (0 without a node); the mode or DSPFX_FIRS_NONE
    std::vector<std::uint32_t> present(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_firs_present(p_, m.data(), first_channel, count));
        return m;
    }
    std::vector<std::uint32_t> lengths(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_firs_lengths(p_, m.data(), first_channel, count));
        return m;
    }
    std::vector<std::uint32_t> modes(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_firs_modes(p_, m.data(), first_channel, count));
        return m;
    }
    // the response of one channel as it was given (time order); empty without a node
    std::vector<double> taps(std::uint64_t channel) {
        std::vector<double> v(max_taps_ ? max_taps_ : 1);
        std::uint32_t n = 0;
        chk(dspfx_firs_taps(p_, channel, v.data(), &n));
        v.resize(n);
        return v;
    }
    // int32 [3][channels] on the device: len, cap, head of every channel's deque after the last run, on its stream
    const std::int32_t *deque() {
        const std::int32_t *d = nullptr;
        chk(dspfx_firs_deque(p_, &d));
        return d;
    }
    dspfx_firs *raw() { return p_; }

  private:
    void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_firs_last_error(p_) ? dspfx_firs_last_error(p_) : dspfx_strerror(rc));
    }
    dspfx_firs *p_ = nullptr;
    std::uint32_t max_taps_;
};

// The device bytes of a ChannelFirs bank's tables (dspfx_firs_plan: a pure host function, no GPU).
inline std::uint64_t firs_plan(std::uint64_t channels, std::uint32_t max_taps) {
    std::uint64_t bytes = 0;
    const int rc = dspfx_firs_plan(channels, max_taps, &bytes);
    if (rc != DSPFX_OK) throw Error(rc, dspfx_firs_last_error(nullptr));
    return bytes;
}

// Per-channel adaptive (NLMS) FIR filters (include/dspfx.h, dspfx_cancel_*): channel c may carry one canceller of its own -- T taps
// (1 .. max_taps) that the device updates every frame, mu, eps, a bulk delay and the switch adapt -- over two device blocks in the
// layout of tile_channels: mic, the primary input, and ref, the block the channel was sent; out = mic minus the filter's estimate
// of ref's path into mic.  A node exists from the first set() that names the channel until drop(); a fresh bank copies mic.  In
// set() a null pointer keeps the node's value (a new node: max_taps taps, mu 0.5, eps 1e-6, delay 0, adapting).
class ChannelCancellers {
  public:
    ChannelCancellers(std::uint32_t channels, std::uint32_t max_taps = 64, std::uint32_t max_delay = 0, std::uint32_t tile_channels = 0,
                      std::uint32_t max_frames = DSPFX_BUF_SIZE, int device = 0, bool general_only = false) {
        const dspfx_cancel_desc d{DSPFX_ABI_VERSION, device, channels, max_frames, tile_channels, max_taps, max_delay, general_only ? 1u : 0u};
        const int rc = dspfx_cancel_create(&d, &p_);
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_cancel_last_error(nullptr) ? dspfx_cancel_last_error(nullptr) : dspfx_strerror(rc));
    }
    ~ChannelCancellers() { dspfx_cancel_destroy(p_); }
    ChannelCancellers(const ChannelCancellers &) = delete;
    ChannelCancellers &operator=(const ChannelCancellers &) = delete;
    // device blocks of n_frames -> device block in the same layout (out == mic: in place; out may not overlap ref); asynchronous on `stream`
    void run(const float *mic, const float *ref, float *out, std::uint32_t n_frames, void *stream = nullptr) {
        chk(dspfx_cancel_run(p_, mic, ref, out, n_frames, stream));
    }
    // the node of channels [first_channel, first_channel + count): each array null (keep) or `count` values.  Any thread; never waits
    void set(const std::uint32_t *taps, const float *mu, const float *eps, const std::uint32_t *delay, const std::uint32_t *adapt,
             std::uint64_t first_channel, std::uint64_t count) {
        chk(dspfx_cancel_set(p_, taps, mu, eps, delay, adapt, first_channel, count));
    }
    // the host's double-talk decision for a range: false freezes (the node filters and does not update)
    void set_adapt(bool adapt, std::uint64_t first_channel, std::uint64_t count) {
        const std::vector<std::uint32_t> a(count, adapt ? 1u : 0u);
        chk(dspfx_cancel_set(p_, nullptr, nullptr, nullptr, nullptr, a.data(), first_channel, count));
    }
    // a warm start: one row of weights for the range, every channel of which carries a node of row.size() taps
    void load(const std::vector<float> &row, std::uint64_t first_channel, std::uint64_t count) {
        chk(dspfx_cancel_load(p_, row.data(), (std::uint32_t)row.size(), 0, first_channel, count));
    }
    // a row per channel: host_rows is [count][n_taps]
    void load_rows(const float *host_rows, std::uint32_t n_taps, std::uint64_t first_channel, std::uint64_t count) {
        chk(dspfx_cancel_load(p_, host_rows, n_taps, 1, first_channel, count));
    }
    // the node removed: a copy again, a later set() makes a new node; queued like a store
    void drop(std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_cancel_drop(p_, first_channel, count)); }
    // weights and history back to +0.0; taps, mu, eps, delay and adapt stay; queued like a store
    void reset(std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_cancel_reset(p_, first_channel, count)); }
    // the host tables, as all stores so far left them: 1 / 0; T (0 without a node); the delay; 1 / 0
    std::vector<std::uint32_t> present(std::uint64_t first_channel, std::uint64_t count) { return table(dspfx_cancel_present, first_channel, count); }
    std::vector<std::uint32_t> lengths(std::uint64_t first_channel, std::uint64_t count) { return table(dspfx_cancel_lengths, first_channel, count); }
    std::vector<std::uint32_t> delays(std::uint64_t first_channel, std::uint64_t count) { return table(dspfx_cancel_delays, first_channel, count); }
    std::vector<std::uint32_t> adapting(std::uint64_t first_channel, std::uint64_t count) { return table(dspfx_cancel_adapting, first_channel, count); }
    // [count][2]: mu and eps as they were given
    std::vector<float> sliders(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<float> v(2 * count);
        chk(dspfx_cancel_sliders(p_, v.data(), first_channel, count));
        return v;
    }
    // float [max_taps][channels] on the device, row k = w[k], +0.0 in the rows k >= a channel's T; valid after a run, on its stream
    const float *weights() {
        const float *w = nullptr;
        chk(dspfx_cancel_weights_view(p_, &w));
        return w;
    }
    // float [2][channels] on the device: sum d * d and sum e * e of the last run
    const float *levels() {
        const float *l = nullptr;
        chk(dspfx_cancel_levels_view(p_, &l));
        return l;
    }
    dspfx_cancel *raw() { return p_; }

  private:
    void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_cancel_last_error(p_) ? dspfx_cancel_last_error(p_) : dspfx_strerror(rc));
    }
    std::vector<std::uint32_t> table(int (*get)(dspfx_cancel *, std::uint32_t *, std::uint64_t, std::uint64_t), std::uint64_t first_channel,
                                     std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(get(p_, m.data(), first_channel, count));
        return m;
    }
    dspfx_cancel *p_ = nullptr;
};

// The device bytes of a ChannelCancellers bank's tables (dspfx_cancel_plan: a pure host function, no GPU).
inline std::uint64_t cancel_plan(std::uint64_t channels, std::uint32_t max_taps, std::uint32_t max_delay) {
    std::uint64_t bytes = 0;
    const int rc = dspfx_cancel_plan(channels, max_taps, max_delay, &bytes);
    if (rc != DSPFX_OK) throw Error(rc, dspfx_cancel_last_error(nullptr));
    return bytes;
}

// Per-channel Signal Generators (include/dspfx.h, dspfx_gens_*), a source that lives on the device: channel c may carry one
// generator of its own -- amplitude, frequency, mode (DSPFX_SIG_*) and clock -- over device blocks in the layout of tile_channels; its
// sample is bit for bit what an engine whose chain is that one Signal Generator writes for it over the same block lengths.  A node
// exists for a channel from the first set() that names it until drop(), starts as the reference's (0.5, 100, Sine, clock +0.0) and
// keeps its clock through every later set(); a fresh bank writes +0.0.  Unlike the reference, a control block is connected per run
// and is not latched into the slider.
class ChannelGenerators {
  public:
    ChannelGenerators(std::uint32_t channels, std::uint32_t tile_channels = 0, std::uint32_t max_frames = DSPFX_BUF_SIZE, int device = 0) {
        const dspfx_gens_desc d{DSPFX_ABI_VERSION, device, channels, max_frames, tile_channels};
        const int rc = dspfx_gens_create(&d, &p_);
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_gens_last_error(nullptr) ? dspfx_gens_last_error(nullptr) : dspfx_strerror(rc));
    }
    ~ChannelGenerators() { dspfx_gens_destroy(p_); }
    ChannelGenerators(const ChannelGenerators &) = delete;
    ChannelGenerators &operator=(const ChannelGenerators &) = delete;
    // n_frames of every channel's generator -> the device block out; add_to (out = add_to + sample; may be out), amplitude and
    // frequency (control blocks, mapped per sample onto -1 .. 1 and 0.1 .. 20000) are device blocks of the same shape or nullptr;
    // asynchronous on `stream`
    void run(float *out, std::uint32_t n_frames, const float *add_to = nullptr, const float *amplitude = nullptr, const float *frequency = nullptr,
             void *stream = nullptr) {
        chk(dspfx_gens_run(p_, add_to, amplitude, frequency, out, n_frames, stream));
    }
    // a generator for each of channels [first_channel, first_channel + count) from host arrays (nullptr: kept, or the default where
    // there is no node); an unknown mode refuses the whole store.  Any thread; never waits
    void set(const float *host_amplitude, const float *host_frequency, const std::uint32_t *host_mode, std::uint64_t first_channel, std::uint64_t count) {
        chk(dspfx_gens_set(p_, host_amplitude, host_frequency, host_mode, first_channel, count));
    }
    // the node removed: +0.0 again; queued like a store
    void drop(std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_gens_drop(p_, first_channel, count)); }
    // the clocks of the range's nodes back to +0.0; queued like a store
    void reset(std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_gens_reset(p_, first_channel, count)); }
    // the host tables, as all stores so far left them: 1 / 0; the DSPFX_SIG_* mode or DSPFX_GENS_NONE; [count][2] amplitude, frequency
    std::vector<std::uint32_t> present(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_gens_present(p_, m.data(), first_channel, count));
        return m;
    }
    std::vector<std::uint32_t> modes(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_gens_modes(p_, m.data(), first_channel, count));
        return m;
    }
    std::vector<float> sliders(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<float> m(2 * count);
        chk(dspfx_gens_sliders(p_, m.data(), first_channel, count));
        return m;
    }
    // clock[N] on the device (valid after a run, on its stream)
    const float *clocks() {
        const float *c = nullptr;
        chk(dspfx_gens_clocks(p_, &c));
        return c;
    }
    dspfx_gens *raw() { return p_; }

  private:
    void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_gens_last_error(p_) ? dspfx_gens_last_error(p_) : dspfx_strerror(rc));
    }
    dspfx_gens *p_ = nullptr;
};

// The device bytes of a ChannelGenerators bank's tables (dspfx_gens_plan: a pure host function, no GPU).
inline std::uint64_t gens_plan(std::uint64_t channels) {
    std::uint64_t bytes = 0;
    const int rc = dspfx_gens_plan(channels, &bytes);
    if (rc != DSPFX_OK) throw Error(rc, dspfx_gens_last_error(nullptr));
    return bytes;
}

// Per-channel Add and Mix nodes (include/dspfx.h, dspfx_blends_*): channel c may carry an Add node or a Mix node with a ratio of its
// own, a send (a Gain node on the node's second input) and a bus id, over device blocks in the layout of tile_channels; its sample
// is bit for bit what an engine whose chain is that one node writes for it from the same inputs.  The second input of a run is an
// N-channel block, a [n_frames][buses] frame-major bus block read through the bus ids (+0.0 on DSPFX_BLENDS_NO_BUS), or nothing
// (+0.0).  A fresh bank copies a.  Unlike the reference, the control block is connected per run and is not latched into the slider.
class ChannelBlends {
  public:
    ChannelBlends(std::uint32_t channels, std::uint32_t buses = 0, std::uint32_t tile_channels = 0, std::uint32_t max_frames = DSPFX_BUF_SIZE,
                  int device = 0) {
        const dspfx_blends_desc d{DSPFX_ABI_VERSION, device, channels, max_frames, tile_channels, buses};
        const int rc = dspfx_blends_create(&d, &p_);
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_blends_last_error(nullptr) ? dspfx_blends_last_error(nullptr) : dspfx_strerror(rc));
    }
    ~ChannelBlends() { dspfx_blends_destroy(p_); }
    ChannelBlends(const ChannelBlends &) = delete;
    ChannelBlends &operator=(const ChannelBlends &) = delete;
    // the device block a -> out (may be a or side); side (a block of a's shape) or bus ([n_frames][buses]) is the second input, both
    // nullptr: +0.0, both given: refused; ratio: the control block of the Mix nodes' ratio or nullptr; asynchronous on `stream`
    void run(const float *a, float *out, std::uint32_t n_frames, const float *side = nullptr, const float *bus = nullptr, const float *ratio = nullptr,
             void *stream = nullptr) {
        chk(dspfx_blends_run(p_, a, side, bus, ratio, out, n_frames, stream));
    }
    // a Mix node for each of channels [first_channel, first_channel + count) from a host array of ratios (nullptr: kept on a Mix
    // node, else 0.5).  Any thread; never waits
    void set_mix(const float *host_ratio, std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_blends_set_mix(p_, host_ratio, first_channel, count)); }
    // ... an Add node
    void set_add(std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_blends_set_add(p_, first_channel, count)); }
    // a send, the Gain node on the second input, from a host array of levels; nullptr removes it
    void set_send(const float *host_level, std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_blends_set_send(p_, host_level, first_channel, count)); }
    // the bus ids, each below buses or DSPFX_BLENDS_NO_BUS; a bad id refuses the whole store
    void assign(const std::uint32_t *host_ids, std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_blends_assign(p_, host_ids, first_channel, count)); }
    // the node and the send removed: a copy again; the bus id stays; queued like a store
    void drop(std::uint64_t first_channel, std::uint64_t count) { chk(dspfx_blends_drop(p_, first_channel, count)); }
    // the host tables, as all stores so far left them: DSPFX_ADD, DSPFX_MIX or DSPFX_BLENDS_NONE; the Mix ratio (0 elsewhere); the
    // send's level and, in `present`, 1 / 0; the bus id or DSPFX_BLENDS_NO_BUS
    std::vector<std::uint32_t> kinds(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_blends_kinds(p_, m.data(), first_channel, count));
        return m;
    }
    std::vector<float> ratios(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<float> m(count);
        chk(dspfx_blends_ratios(p_, m.data(), first_channel, count));
        return m;
    }
    std::vector<float> sends(std::uint64_t first_channel, std::uint64_t count, std::vector<std::uint32_t> &present) {
        std::vector<float> m(count);
        present.assign(count, 0);
        chk(dspfx_blends_sends(p_, m.data(), present.data(), first_channel, count));
        return m;
    }
    std::vector<std::uint32_t> bus_of(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> m(count);
        chk(dspfx_blends_bus_of(p_, m.data(), first_channel, count));
        return m;
    }
    dspfx_blends *raw() { return p_; }

  private:
    void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_blends_last_error(p_) ? dspfx_blends_last_error(p_) : dspfx_strerror(rc));
    }
    dspfx_blends *p_ = nullptr;
};

// The device bytes of a ChannelBlends bank's tables (dspfx_blends_plan: a pure host function, no GPU).
inline std::uint64_t blends_plan(std::uint64_t channels) {
    std::uint64_t bytes = 0;
    const int rc = dspfx_blends_plan(channels, &bytes);
    if (rc != DSPFX_OK) throw Error(rc, dspfx_blends_last_error(nullptr));
    return bytes;
}

// Each listener's own mix of their room (include/dspfx.h, dspfx_mixmatrix_*): room r of n_r contiguous channels owns an n_r x n_r
// matrix M[l][s] (listener, source), out[f][c0 + l] = (sum_s M[l][s] x[f][c0 + s]) / link_divisor(wired entries of row l).  Rooms as
// MixGroups takes them, 1 .. DSPFX_MIXMATRIX_MAX_ROOM members each; a fresh bank holds mix-minus, which is MixGroups::returns without
// faders.  Between ChannelStrips::run and the listeners' Resampler, as an alternative to returns.  The rooms are fixed, unless
// the bank is made with seats (the second constructor): then assign() reseats channels live, as MixGroups::assign does.
class MixMatrix {
  public:
    MixMatrix(std::uint32_t channels, const std::vector<std::uint64_t> &group_start, std::uint32_t tile_channels = 0,
              std::uint32_t max_frames = DSPFX_BUF_SIZE, bool normalise = true, int device = 0) {
        const dspfx_mixmatrix_desc d{DSPFX_ABI_VERSION, device, channels, max_frames, tile_channels,
                                     (std::uint32_t)(group_start.empty() ? 0 : group_start.size() - 1), normalise ? 1u : 0u, group_start.data()};
        const int rc = dspfx_mixmatrix_create(&d, &p_);
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_mixmatrix_last_error(nullptr) ? dspfx_mixmatrix_last_error(nullptr) : dspfx_strerror(rc));
    }
    ~MixMatrix() { dspfx_mixmatrix_destroy(p_); }
    MixMatrix(const MixMatrix &) = delete;
    MixMatrix &operator=(const MixMatrix &) = delete;
    // device block of n_frames -> device block in the same layout; out may not overlap block (no in-place form, except out == block
    // in DSPFX_MIXMATRIX_STAGED); asynchronous on `stream`
    void run(const float *block, std::uint32_t n_frames, float *out, void *stream = nullptr) { chk(dspfx_mixmatrix_run(p_, block, n_frames, out, stream)); }
    // the sparse run: room r adds only the sources named in list[start[r] .. start[r] + count[r]) (device pointers: channel numbers,
    // start[G + 1], count[G]; Talkers::audible gives them), in ascending room-local order, and reads no other.  Where every unlisted
    // source carries +-0.0 it is run() bit for bit.  Bad entries are ignored.  The list's producer and this run share a stream
    void run_sparse(const float *block, std::uint32_t n_frames, float *out, const std::int32_t *list, std::uint64_t list_len, const std::uint32_t *start,
                    const std::uint32_t *count, void *stream = nullptr) {
        chk(dspfx_mixmatrix_run_sparse(p_, block, n_frames, out, list, list_len, start, count, stream));
    }
    // what listeners [first_channel, first_channel + count) of ONE room hear: host_values[count][row_len], row_len = the room's members.
    // Any thread; never waits; applies, whole, to the runs submitted after it.
    void set_rows(const float *host_values, std::uint32_t row_len, std::uint64_t first_channel, std::uint64_t count) {
        chk(dspfx_mixmatrix_set_rows(p_, host_values, row_len, first_channel, count));
    }
    // how loud sources [first_channel, first_channel + count) are for each listener of their room: host_values[count][row_len]
    void set_cols(const float *host_values, std::uint32_t row_len, std::uint64_t first_channel, std::uint64_t count) {
        chk(dspfx_mixmatrix_set_cols(p_, host_values, row_len, first_channel, count));
    }
    // room `room` (-1: every room) back to DSPFX_MIXMATRIX_MIX_MINUS or DSPFX_MIXMATRIX_ZERO
    void fill(std::int64_t room = -1, std::uint32_t preset = DSPFX_MIXMATRIX_MIX_MINUS) { chk(dspfx_mixmatrix_fill(p_, room, preset)); }
    // the fresh state: mix-minus in every room
    void reset() { chk(dspfx_mixmatrix_reset(p_)); }
    // a SEATED bank (dspfx_mixmatrix_create_seats): room r owns seats[r] seats (>= its members, rounded up to 32, <= the limit) and a
    // table that never moves; assign() then reseats channels live.  Rows and columns are S_r long and indexed by seat
    MixMatrix(std::uint32_t channels, const std::vector<std::uint64_t> &group_start, const std::vector<std::uint32_t> &seats,
              std::uint32_t tile_channels = 0, std::uint32_t max_frames = DSPFX_BUF_SIZE, bool normalise = true, int device = 0) {
        const std::uint32_t G = (std::uint32_t)(group_start.empty() ? 0 : group_start.size() - 1);
        if (seats.size() != G) throw Error(DSPFX_ERR_INVALID, "seats: one count per room");
        const dspfx_mixmatrix_desc d{DSPFX_ABI_VERSION, device, channels, max_frames, tile_channels, G, normalise ? 1u : 0u, group_start.data()};
        const int rc = dspfx_mixmatrix_create_seats(&d, seats.data(), &p_);
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_mixmatrix_last_error(nullptr) ? dspfx_mixmatrix_last_error(nullptr) : dspfx_strerror(rc));
    }
    // seating (dspfx_mixmatrix_assign): the rooms of channels [first_channel, first_channel + ids.size()), each < the rooms or NO_ROOM.
    // Those whose id is their room stay as they are; the others leave, then enter in ascending channel order, each into the lowest
    // free seat, wired by `preset`.  A bad id or range, or a room over capacity, stores nothing.  Any thread; never waits for a run
    void assign(const std::vector<std::uint32_t> &ids, std::uint64_t first_channel = 0, std::uint32_t preset = DSPFX_MIXMATRIX_MIX_MINUS) {
        chk(dspfx_mixmatrix_assign(p_, ids.data(), first_channel, ids.size(), preset));
    }
    void assign(std::uint32_t id, std::uint64_t first_channel, std::uint32_t preset = DSPFX_MIXMATRIX_MIX_MINUS) {
        chk(dspfx_mixmatrix_assign(p_, &id, first_channel, 1, preset));
    }
    // the room (NO_ROOM: none) and the seat (0xFFFFFFFF: none) of channels [first_channel, first_channel + count), and the taken seats
    // of each of `rooms` rooms, by every call made so far
    std::vector<std::uint32_t> room_of(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> v(count);
        chk(dspfx_mixmatrix_rooms(p_, v.data(), first_channel, count));
        return v;
    }
    std::vector<std::uint32_t> seat_of(std::uint64_t first_channel, std::uint64_t count) {
        std::vector<std::uint32_t> v(count);
        chk(dspfx_mixmatrix_seats(p_, v.data(), first_channel, count));
        return v;
    }
    std::vector<std::uint32_t> occupancy(std::uint32_t rooms) {
        std::vector<std::uint32_t> v(rooms);
        chk(dspfx_mixmatrix_occupancy(p_, v.data()));
        return v;
    }
    // a seated bank: the mode of the runs submitted after the call (dspfx_mixmatrix_set_staging).  DSPFX_MIXMATRIX_STAGED transposes the
    // block into a seat-ordered copy, runs the same chain over it and transposes back: the direct run's bits at a cost that does not
    // depend on the seating, and run(block, n, block) in place.  The first switch allocates mixmatrix_staging_bytes(...).  Any thread
    void set_staging(std::uint32_t mode) { chk(dspfx_mixmatrix_set_staging(p_, mode)); }
    std::uint32_t staging() {
        std::uint32_t mode = 0;
        chk(dspfx_mixmatrix_staging(p_, &mode));
        return mode;
    }
    // M[listeners[i]][sources[i]] = gains[i] by channel number, in order; each pair two channels of one room
    void set_pairs(const std::vector<std::uint32_t> &listeners, const std::vector<std::uint32_t> &sources, const std::vector<float> &gains) {
        if (listeners.size() != sources.size() || listeners.size() != gains.size()) throw Error(DSPFX_ERR_INVALID, "listeners, sources and gains are equally long");
        chk(dspfx_mixmatrix_set_pairs(p_, listeners.data(), sources.data(), gains.data(), gains.size()));
    }
    dspfx_mixmatrix *raw() { return p_; }

  private:
    void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, *dspfx_mixmatrix_last_error(p_) ? dspfx_mixmatrix_last_error(p_) : dspfx_strerror(rc));
    }
    dspfx_mixmatrix *p_ = nullptr;
};

// Per room of a table: its members, the edge of its padded matrix and the element offset of that matrix, and the bytes of all of
// them (dspfx_mixmatrix_plan: a pure host function, no GPU; throws with the reason for a table MixMatrix would refuse).
struct MixMatrixPlan {
    std::vector<std::uint32_t> count, edge;
    std::vector<std::uint64_t> offset;
    std::uint64_t total_bytes = 0;
};
inline MixMatrixPlan mixmatrix_plan(std::uint64_t channels, const std::vector<std::uint64_t> &group_start, std::uint32_t tile_channels = 0) {
    const std::uint32_t G = (std::uint32_t)(group_start.empty() ? 0 : group_start.size() - 1);
    MixMatrixPlan r;
    r.count.resize(G);
    r.edge.resize(G);
    r.offset.resize(G);
    const int rc = dspfx_mixmatrix_plan(group_start.data(), G, channels, tile_channels, r.count.data(), r.edge.data(), r.offset.data(), &r.total_bytes);
    if (rc != DSPFX_OK) throw Error(rc, dspfx_mixmatrix_last_error(nullptr));
    return r;
}
// ... of a seated bank (dspfx_mixmatrix_plan_seats): the edges are the seats rounded up to 32
inline MixMatrixPlan mixmatrix_plan(std::uint64_t channels, const std::vector<std::uint64_t> &group_start, const std::vector<std::uint32_t> &seats,
                                    std::uint32_t tile_channels = 0) {
    const std::uint32_t G = (std::uint32_t)(group_start.empty() ? 0 : group_start.size() - 1);
    if (seats.size() != G) throw Error(DSPFX_ERR_INVALID, "seats: one count per room");
    MixMatrixPlan r;
    r.count.resize(G);
    r.edge.resize(G);
    r.offset.resize(G);
    const int rc = dspfx_mixmatrix_plan_seats(group_start.data(), G, channels, tile_channels, seats.data(), r.count.data(), r.edge.data(), r.offset.data(),
                                              &r.total_bytes);
    if (rc != DSPFX_OK) throw Error(rc, dspfx_mixmatrix_last_error(nullptr));
    return r;
}
// The seating rule on host arrays (dspfx_mixmatrix_reseat: a pure host function): what MixMatrix::assign does to the bank's tables
inline void mixmatrix_reseat(std::vector<std::uint32_t> &room_of, std::vector<std::uint32_t> &seat_of, const std::vector<std::uint32_t> &seats,
                             const std::vector<std::uint32_t> &ids, std::uint64_t first_channel = 0) {
    if (room_of.size() != seat_of.size()) throw Error(DSPFX_ERR_INVALID, "room_of and seat_of are equally long");
    const int rc = dspfx_mixmatrix_reseat(room_of.data(), seat_of.data(), seats.data(), (std::uint32_t)seats.size(), room_of.size(), ids.data(), first_channel,
                                          ids.size());
    if (rc != DSPFX_OK) throw Error(rc, dspfx_mixmatrix_last_error(nullptr));
}

// The bytes DSPFX_MIXMATRIX_STAGED adds to the seated bank of this plan (dspfx_mixmatrix_staging_bytes: a pure host function)
inline std::uint64_t mixmatrix_staging_bytes(std::uint64_t channels, const std::vector<std::uint64_t> &group_start, const std::vector<std::uint32_t> &seats,
                                             std::uint32_t max_frames = DSPFX_BUF_SIZE, std::uint32_t tile_channels = 0) {
    const std::uint32_t G = (std::uint32_t)(group_start.empty() ? 0 : group_start.size() - 1);
    if (seats.size() != G) throw Error(DSPFX_ERR_INVALID, "seats: one count per room");
    std::uint64_t bytes = 0;
    const int rc = dspfx_mixmatrix_staging_bytes(group_start.data(), G, channels, tile_channels, seats.data(), max_frames, &bytes);
    if (rc != DSPFX_OK) throw Error(rc, dspfx_mixmatrix_last_error(nullptr));
    return bytes;
}
// How scattered a seating is (dspfx_mixmatrix_scatter: a pure host function): the chunks of 32 seats that hold anybody, and the lines
// of 32 adjacent channels they read per frame.  lines / chunks near 1: the direct run is the cheaper; towards 32: the staged one
struct MixMatrixScatter {
    std::uint64_t chunks = 0, lines = 0;
};
inline MixMatrixScatter mixmatrix_scatter(const std::vector<std::uint32_t> &room_of, const std::vector<std::uint32_t> &seat_of,
                                          const std::vector<std::uint32_t> &seats) {
    if (room_of.size() != seat_of.size()) throw Error(DSPFX_ERR_INVALID, "room_of and seat_of are equally long");
    MixMatrixScatter r;
    const int rc = dspfx_mixmatrix_scatter(room_of.data(), seat_of.data(), seats.data(), (std::uint32_t)seats.size(), room_of.size(), &r.chunks, &r.lines);
    if (rc != DSPFX_OK) throw Error(rc, dspfx_mixmatrix_last_error(nullptr));
    return r;
}

// One long impulse response over N channels by partitioned FFT (dspfx_convolve_*): the FIR node's arithmetic for responses too
// long for its tap table, e.g. a convolution reverb on the G buses of a MixGroups.  `taps_reversed` as dspfx_set_taps takes them.
class Convolver {
  public:
    Convolver(std::uint32_t channels, const std::vector<double> &taps_reversed, int mode = DSPFX_FIR_BALANCED,
              std::uint32_t max_taps = 0, std::uint32_t tile_channels = 0, int device = 0) {
        const dspfx_convolve_desc d{DSPFX_ABI_VERSION, device, channels, tile_channels, (std::uint32_t)taps_reversed.size(), max_taps,
                                    mode, taps_reversed.data()};
        const int rc = dspfx_convolve_create(&d, &p_);
        if (rc != DSPFX_OK) throw Error(rc, dspfx_strerror(rc));
        partitions_ = partitions_of(taps_reversed);
    }
    ~Convolver() { dspfx_convolve_destroy(p_); }
    Convolver(const Convolver &) = delete;
    Convolver &operator=(const Convolver &) = delete;
    // P = ceil(T / 128): the spectra of history one block reads per channel
    std::uint32_t partitions() const { return partitions_; }
    // device block of n_frames (a multiple of 128) -> device block `out` in the same layout (out == in: in place); asynchronous
    void run(const float *in, float *out, std::uint32_t n_frames = DSPFX_BUF_SIZE, void *stream = nullptr) {
        chk(dspfx_convolve_run(p_, in, out, n_frames, stream));
    }
    // replaces the response (at most max_taps long) and keeps the history; from the next run on
    void set_taps(const std::vector<double> &taps_reversed, int mode = DSPFX_FIR_BALANCED) {
        chk(dspfx_convolve_set_taps(p_, taps_reversed.data(), (std::uint32_t)taps_reversed.size(), mode));
        partitions_ = partitions_of(taps_reversed);
    }
    void reset() { chk(dspfx_convolve_reset(p_)); }
    // one more response (at most max_taps long) -> its id: 1, 2, ...; no channel carries it until assign says so
    std::uint32_t add_response(const std::vector<double> &taps_reversed, int mode = DSPFX_FIR_BALANCED) {
        std::uint32_t id = 0;
        chk(dspfx_convolve_response_add(p_, taps_reversed.data(), (std::uint32_t)taps_reversed.size(), mode, &id));
        return id;
    }
    // replaces response `id` and leaves the others, the ids and the history alone; id 0 is set_taps
    void set_response(std::uint32_t id, const std::vector<double> &taps_reversed, int mode = DSPFX_FIR_BALANCED) {
        chk(dspfx_convolve_response_set(p_, id, taps_reversed.data(), (std::uint32_t)taps_reversed.size(), mode));
        if (id == 0) partitions_ = partitions_of(taps_reversed);
    }
    // channels [first_channel, first_channel + ids.size()) carry these responses from the next run on; the history stays
    void assign(const std::vector<std::uint16_t> &ids, std::uint64_t first_channel = 0) {
        chk(dspfx_convolve_assign(p_, ids.data(), first_channel, ids.size()));
    }
    void assign(std::uint16_t id, std::uint64_t first_channel) { chk(dspfx_convolve_assign(p_, &id, first_channel, 1)); }
    // how many responses the bank holds (at most CONVOLVE_MAX_RESPONSES)
    std::uint32_t responses() const {
        const int n = dspfx_convolve_response_count(p_);
        if (n < 0) throw Error(n, dspfx_strerror(n));
        return (std::uint32_t)n;
    }
    dspfx_convolve *raw() { return p_; }

  private:
    static std::uint32_t partitions_of(const std::vector<double> &taps_reversed) {
        std::uint32_t parts = 0;
        const int rc = dspfx_convolve_plan(taps_reversed.data(), (std::uint32_t)taps_reversed.size(), &parts, nullptr);
        if (rc != DSPFX_OK) throw Error(rc, dspfx_strerror(rc));
        return parts;
    }
    void chk(int rc) {
        if (rc != DSPFX_OK) throw Error(rc, dspfx_strerror(rc));
    }
    dspfx_convolve *p_ = nullptr;
    std::uint32_t partitions_ = 0;
};

}  // namespace dspfx
