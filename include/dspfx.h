/*
 * dspfx.h -- C ABI of the MI355X-native effect-chain engine.
 *
 * The drop-in boundary for simmsb/dsp-stuff's per-block effect-node evaluation
 * loop: everything `SimpleNode::process` (dsp-stuff/src/node.rs:135-146) and the
 * blanket `Perform` wrapper (node.rs:267-352) compute for one mono channel and one
 * 128-frame block, evaluated here for N independent channels per launch by
 * hand-written HIP kernels (gfx950).  The reference has no FFI of its own
 * (SURVEY.md 8b); this header is the ABI its Rust host would bind (see
 * INTEGRATION.md for the `extern "C"` block and the `GpuChain: SimpleNode` shim).
 *
 * Conventions
 *   - plain C types only; every call returns 0 (DSPFX_OK) or a negative
 *     dspfx_status; nothing aborts or throws across the boundary (the reference
 *     panics instead: node.rs:173,271,280).
 *   - the caller owns sample buffers; the engine owns parameters, coefficients
 *     and all DSP state (biquad history, one-pole z, delay rings, FIR history)
 *     in HBM -- the same ownership split as node.rs:271-288 vs biquad.rs:43-44,
 *     reverb.rs:40-41, fir.rs:64-65.
 *   - sample layout is frame-major f32 by default: buf[frame * channels + channel]
 *     ("[B][N]"): for every frame the N channels are contiguous, so one
 *     wavefront reads 64 consecutive channels as one coalesced burst
 *     (dspfx_engine_desc.tile_channels selects the channel-tiled form).
 *   - threads: every entry point may be called from any thread; calls on one engine are
 *     serialised by the engine (distinct engines are independent).  The reference's split is
 *     kept: ONE thread drives the process calls (one node task, runtime.rs:718-728) while
 *     another -- the GUI -- stores sliders and modes (dsp-stuff-derive/src/lib.rs:487-492,
 *     biquad.rs:62-76).  dspfx_set_param / dspfx_set_mode NEVER wait for a process call in
 *     progress: the store is queued and takes effect at the next block boundary (at once when
 *     the engine is idle), in the order the stores were made.
 *   - streams: the process calls are asynchronous on the caller's stream.  Everything that
 *     writes DSP state outside a block (a biquad's reset on a coefficient store, dspfx_reset)
 *     is queued on the stream the state was last used on, so it is ordered behind the blocks
 *     in flight and ahead of the next one -- with any kind of stream (torch's and most hosts'
 *     streams are non-blocking: the null stream orders nothing against them).  A process call
 *     on a DIFFERENT stream first waits (on the device) for the previous stream.  Calls that
 *     free or re-allocate state (dspfx_chain_set, dspfx_graph_set, dspfx_set_taps, dspfx_ring_trim,
 *     dspfx_state_import / _export) wait for the device first.  A delay-ring length change does NOT (dspfx_set_param).
 *   - there is NO CPU fallback: without a HIP device every entry point that
 *     needs one fails with DSPFX_ERR_NO_DEVICE.
 *   - kernels: which kernel serves a chain is the engine's business and never changes a sample
 *     (dspfx_describe names it).  Kernels specialised for a chain's shape are taken from the
 *     on-disk cache or compiled by the library's background thread while an interpreting kernel
 *     serves, and adopted at a block boundary (dspfx_kernels_ready).  N need not be a multiple of 64.
 */
#ifndef DSPFX_H
#define DSPFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): REVERB carries its `seconds` slider (params[1]) and every slider store on a REVERB node swaps in a new zero
 *    ring like the reference's after_settings_change; the FIR state blob is {32-byte header, held samples} (round 3);
 *    DSPFX_FIR_PRECISION_DEFAULT means the split bf16 sweep (round 3).  Engines refuse a descriptor of another version. */
#define DSPFX_ABI_VERSION 2
/* dsp-stuff/src/node.rs:257 `pub const BUF_SIZE: usize = 128;` */
#define DSPFX_BUF_SIZE 128
/* longest chain one engine accepts */
#define DSPFX_MAX_NODES 32

typedef struct dspfx_engine dspfx_engine;

typedef enum dspfx_status {
    DSPFX_OK = 0,
    DSPFX_ERR_INVALID = -1,    /* bad argument / descriptor */
    DSPFX_ERR_NO_DEVICE = -2,  /* no usable HIP device (there is no CPU fallback) */
    DSPFX_ERR_HIP = -3,        /* a HIP runtime call failed; see dspfx_last_error */
    DSPFX_ERR_OOM = -4,        /* device allocation failed */
    DSPFX_ERR_UNSUPPORTED = -5,
    DSPFX_ERR_STATE = -6       /* call not valid in the engine's current state */
} dspfx_status;

/* Node kinds = the effect variants of `enum Nodes` (nodes/mod.rs:38-63) that
 * are on the hot path. */
typedef enum dspfx_kind {
    DSPFX_GAIN = 0,      /* nodes/gain.rs:25-38 */
    DSPFX_BIQUAD = 1,    /* nodes/biquad.rs:48-88 (+ biquad 0.4.2 DirectForm1<f32>) */
    DSPFX_LOW_PASS = 2,  /* nodes/low_pass.rs:26-42 */
    DSPFX_HIGH_PASS = 3, /* nodes/high_pass.rs:26-42 */
    DSPFX_REVERB = 4,    /* nodes/reverb.rs:44-111: feedback delay line */
    DSPFX_DISTORT = 5,   /* nodes/distort.rs:53-195 */
    DSPFX_OVERDRIVE = 6, /* nodes/overdrive.rs:31-72 */
    DSPFX_CHEBYSHEV = 7, /* nodes/chebyshev.rs:28-62 */
    DSPFX_FIR = 8,       /* nodes/fir.rs:179-225 */
    DSPFX_ADD = 9,       /* nodes/add.rs:24-34  (port "b" = the side input) */
    DSPFX_MIX = 10,      /* nodes/mix.rs:31-47  (port "b" = the side input) */
    DSPFX_SIGNAL_GEN = 11, /* nodes/signal_gen.rs:55-129: a SOURCE (no "in" port): replaces the signal */
    DSPFX_ENVELOPE = 12, /* nodes/envelope.rs:34-52: dasp_envelope 0.11.0 peak detector (full-wave) */
    DSPFX_N_KINDS = 13
} dspfx_kind;

/* nodes/signal_gen.rs:17-22 `enum Mode` */
typedef enum dspfx_signal_mode { DSPFX_SIG_SINE = 0, DSPFX_SIG_TRIANGLE = 1, DSPFX_SIG_SQUARE = 2, DSPFX_SIG_CONSTANT = 3 } dspfx_signal_mode;

/* nodes/distort.rs:18-28 `enum Mode`, declaration order (repr(u8)) */
typedef enum dspfx_distort_mode {
    DSPFX_DIST_HARD_CLIP = 0,
    DSPFX_DIST_SOFT_CLIP = 1,
    DSPFX_DIST_TANH = 2,
    DSPFX_DIST_RECIP_SOFT_CLIP = 3,
    DSPFX_DIST_FUZZ = 4,
    DSPFX_DIST_SIN = 5,
    DSPFX_DIST_ATAN = 6,
    DSPFX_DIST_SQUARE = 7,
    DSPFX_DIST_CHEBYSHEV4 = 8
} dspfx_distort_mode;

/* nodes/fir.rs `enum Mode` (fir.rs:187-190) */
typedef enum dspfx_fir_mode { DSPFX_FIR_BALANCED = 0, DSPFX_FIR_AVERAGE = 1 } dspfx_fir_mode;

/* Which hops of the chain reproduce `collect_and_average` with one connected
 * pipe (node.rs:162-194: value = (0.0 + x) / f32(0.0001 + 1.0)).
 *   INTERNAL: the hops between consecutive nodes of the chain (what disappears
 *             when k reference nodes are fused into one GpuChain node);
 *   INPUT   : also the hop into the first node (whole-graph semantics: the
 *             engine is fed by the Input node, nodes/input.rs:213-240).        */
#define DSPFX_LINK_INTERNAL 1u
#define DSPFX_LINK_INPUT 2u
/*   SIDE_RAW: the side input (port "b" of ADD/MIX) is taken as given: it was already averaged
 *             over several links by dspfx_link_average (graphs with fan-in on that port).  */
#define DSPFX_LINK_SIDE_RAW 4u
/* most links into one port that dspfx_link_average accepts */
#define DSPFX_MAX_LINKS 16

typedef struct dspfx_engine_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t channels;        /* N: independent mono channels held by this engine */
    uint32_t max_frames;      /* largest n_frames a process call will pass (>=1) */
    uint32_t link_flags;      /* DSPFX_LINK_* */
    uint32_t tile_channels;   /* sample layout: 0 = frame-major [n_frames][N];
                                 W (power of two, N % W == 0) = channel-tiled [N/W][n_frames][W]:
                                 element (f, c) at ((c / W) * n_frames + f) * W + c % W, so the
                                 block of every W-channel group is one contiguous HBM extent */
    uint64_t channel_offset;  /* global index of local channel 0 (multi-GPU shards, noise) */
} dspfx_engine_desc;

/* One node of the chain: the reference node's slider fields, in field order.
 *   GAIN       params[0]=level (0..=10, default 1)                    gain.rs:21-22
 *   BIQUAD     params[0..5]=a0,a1,a2,b0,b1,b2 (raw sliders -10..=10)  biquad.rs:18-41
 *   LOW_PASS   params[0]=ratio (0..=1, default 0.5)                   low_pass.rs:20-21
 *   HIGH_PASS  params[0]=ratio                                        high_pass.rs:20-21
 *   REVERB     params[0]=decay (0..=1, default .5), params[1]=seconds (0..=1, default .5; 0 = not given);
 *              delay_len=D, the ring the node STARTS with (restored: dspfx_delay_len(seconds, r); fresh from the menu:
 *              dspfx_delay_len(0, r) -- make_buffer); mode bit 0 = r: the page-rounded reading of seconds -> samples
 *              (see dspfx_set_param for what a slider store does to the ring)   reverb.rs:29-38, 44-71
 *   DISTORT    params[0]=level (0..=30, default 0); mode              distort.rs:46-50
 *   OVERDRIVE  params[0]=boost, [1]=drive, [2]=level                  overdrive.rs:21-28
 *   CHEBYSHEV  params[0]=level_pos, [1]=level_neg                     chebyshev.rs:21-25
 *   FIR        taps/n_taps (time-REVERSED, as fir.rs:163,168 stores them); mode
 *   ADD        -
 *   MIX        params[0]=ratio (0..=1, default .5)                    mix.rs:22-28
 *   SIGNAL_GEN params[0]=amplitude (-1..=1, default .5), [1]=frequency (0.1..=20000 Hz, default 100); mode
 *              (dspfx_signal_mode); per-channel phase clock, wrapped at every 128-frame block end  signal_gen.rs:41-55
 *   ENVELOPE   params[0]=attack, [1]=release, both in frames (0..=1000, default 0); per-channel envelope
 *              env = d + (env - d)*g, d = |x|, g = env < d ? e^(-1/attack) : e^(-1/release), g = 0 for 0 frames
 *              (dasp_envelope 0.11.0 Detector::next, restated as recalled: see oracle/dspfx_oracle.h)  envelope.rs:27-30
 * delay_len is explicit because rivulet's capacity rounding is not in the
 * reference tree; dspfx_delay_len() gives both readings.    */
typedef struct dspfx_node_desc {
    int32_t kind;        /* dspfx_kind */
    int32_t mode;        /* dspfx_distort_mode / dspfx_fir_mode / dspfx_signal_mode */
    float params[8];
    uint32_t delay_len;  /* REVERB: D >= 128 */
    uint32_t n_taps;     /* FIR */
    const double *taps;  /* FIR: n_taps f64 values, host memory, copied */
} dspfx_node_desc;

/* ---- library ----------------------------------------------------------- */
uint32_t dspfx_abi_version(void);
const char *dspfx_strerror(int status);
/* Number of visible HIP devices (0 when there is none). */
int dspfx_device_count(void);
/* Fill `d` with the reference's defaults for `kind` (derive `default=`, lib.rs:196-210). */
int dspfx_node_defaults(int kind, dspfx_node_desc *d);
/* reverb.rs:58 `((seconds * 48000.0) as usize).max(128)`; page_round != 0 rounds up to whole 4 KiB pages (1024 f32).
 * Two readings of ONE fact that the reference tree does not contain (rivulet is a git dependency, Cargo.toml:42): both
 * refresh_seconds (reverb.rs:60-68) and make_buffer (reverb.rs:44-49) call circular_buffer::<f32>(n), try_grant(n) and then
 * release(view().len()) zeros -- the delay is however long the granted view is.
 *   page_round = 0  the view is exactly the n asked for: the delay is n samples (what the slider's "s" suffix promises);
 *   page_round = 1  the view is all the free space of a buffer whose capacity is whole pages: n rounded up to 1024 f32.
 * Evidence, as far as it goes: rivulet's circular buffer is a virtual-memory mirror (page-granular capacity) and its `grant`
 * contract is "at least count" -- both favour 1; the label "Delay ... s" and the 0.5 s default say what the author MEANT -- 0.
 * Neither can be pinned here, so the reading is the caller's choice (mode bit 0 of a REVERB node) and it is applied to BOTH
 * call sites alike: a node fresh from the menu sits on dspfx_delay_len(0, page_round) = 128 or 1024 samples. */
uint32_t dspfx_delay_len(float seconds, int page_round);
/* node.rs:166,179: f32 0.0001 incremented by 1.0 per connected pipe. */
float dspfx_link_divisor(uint64_t n_connected);

/* ---- engine lifecycle -------------------------------------------------- */
int dspfx_engine_create(const dspfx_engine_desc *desc, dspfx_engine **out);
/* Waits for the device (blocks in flight still read the engine's state), then frees everything.  Takes no lock: call it
 * when no other thread is inside an entry point of this engine or still holds a reference to it. */
void dspfx_engine_destroy(dspfx_engine *e);
const char *dspfx_last_error(const dspfx_engine *e);

/* Replace the chain (NodeStatic::new for every node, node.rs:125-133): allocates
 * and zeroes all DSP state.  Nodes are evaluated in order, node i feeding i+1
 * (a linear graph of runtime.rs LinkInstances). */
int dspfx_chain_set(dspfx_engine *e, const dspfx_node_desc *nodes, int n_nodes);
int dspfx_chain_len(const dspfx_engine *e);
/* Kernels specialised for a chain's shape come from this process' table or the on-disk cache of code objects
 * ($DSPFX_CACHE_DIR, else $XDG_CACHE_HOME/dspfx, else ~/.cache/dspfx; DSPFX_DISK_CACHE=0: none) in milliseconds; a shape seen
 * for the first time is compiled by ONE background thread while the engine serves its blocks on the interpreting kernel, and
 * adopted at a block boundary: dspfx_chain_set, dspfx_set_mode and the first connected control port never wait for the
 * compiler (the reference re-creates nodes on every graph edit, runtime.rs:319-362).  Samples are the same bit for bit, and so
 * is the bus (the interpreter runs with the coming kernel's rows of partial sums).  This call is for a host -- or a benchmark --
 * that wants the specialised kernels BEFORE its first block: it adopts what is finished and waits up to wait_ms milliseconds
 * for the rest.  Returns 1: nothing is pending (dspfx_describe names the kernels that are live), 0: still compiling, < 0: error.
 * It does not hold the engine while it waits.  DSPFX_JIT=0: no run-time kernels; DSPFX_JIT=1 / DSPFX_JIT_ASYNC=0: compiled inside
 * dspfx_chain_set (about a second per new shape), as in rounds 1-3.  A whole-graph kernel (dspfx_graph_set) has no interpreter to
 * stand in for it: compiled in the call when neither cache has it. */
int dspfx_kernels_ready(dspfx_engine *e, int wait_ms);

/* Slider store + `after_settings_change` (dsp-stuff-derive/src/lib.rs:487-497, 560-568: the generated render() runs the
 * node's hook when ANY of its widgets changed):
 *   BIQUAD renormalises by a0 and ZEROES its state (biquad.rs:15, 62-76);
 *   REVERB -- ANY slider, `decay` included -- swaps in a NEW ZERO-FILLED ring (reverb.rs:19, 55-71: refresh_seconds): the echo
 *          tail is cut.  Its length is what the seconds slider says, max((seconds * 48000) as usize, 128) (mode bit 0: rounded up
 *          to whole 4 KiB pages), when the node was given one (params[1] > 0) -- so a node fresh from the menu (dspfx_node_defaults:
 *          make_buffer's 128-sample ring -- 1024 page-rounded -- under a 0.5 s slider, reverb.rs:44-52) becomes a 24000-sample delay at its first slider
 *          change, like the reference's -- and the ring's current length otherwise.  The swap costs NOTHING on the thread
 *          that drives the blocks, whatever the two lengths: no wait for the device, no memset, no re-allocation, placement
 *          kept.  The ring is a table of separately allocated 128-row groups of which a ring of D samples uses the first
 *          ceil(D / 128); the swap sets D, restarts the position and makes the next D frames read their taps as +0.0 (a per-node
 *          frame counter in the kernel arguments), in order with the blocks in flight, which carry their own copies.  Groups a
 *          LONGER ring needs are allocated -- not zeroed: every row is written before it is read unmasked -- by the thread
 *          that MAKES the store, before the store is queued (the reference's GUI thread allocates the new ring too,
 *          reverb.rs:55-71); dspfx_chain_set reserves them up front for a menu-fresh node when that is cheap (at most 1/16 of the
 *          device's free memory; DSPFX_MENU_RING_RESERVE=0 never, =1 whenever it fits -- dspfx_reserve_delay_len is the explicit
 *          form and dspfx_ring_trim gives unused reservations back); a shorter ring keeps the surplus
 *          as capacity (dspfx_ring_trim returns it).  DSPFX_ERR_OOM: the store was NOT made, the node keeps ring and slider.
 *          params[1] outside 0..=1 (the slider's range, reverb.rs:34-37) is DSPFX_ERR_INVALID; a STORED 0.0 is a value like any other
 *          (a 128-sample ring, reverb.rs:58) -- only in a node DESCRIPTOR does params[1] = 0 mean "no seconds slider: keep delay_len";
 *   other kinds just take the value from the next block on.  Nothing is launched or compiled by a slider store (the
 * exactness of a DISTORT level as a constant divisor is decided on the host; only a level that is an even integer
 * other than a power of two runs the 2 ms device check, once per value and process).
 * Safe from a second thread while another one is inside a process call (the reference's GUI thread does exactly
 * that): the store is validated, queued and returns; it is applied -- with its stores before it, in order -- by the
 * next entry point that holds the engine: immediately when the engine is idle, else at the next block boundary.  The
 * biquad reset is queued on the stream of the blocks in flight, behind them.  dspfx_set_param_seq also returns the
 * store's sequence number; dspfx_param_log tells where each store took effect. */
int dspfx_set_param(dspfx_engine *e, int node, int param, float value);
int dspfx_set_param_seq(dspfx_engine *e, int node, int param, float value, uint64_t *seq);
/* Mode store (the `mode` atomics of distort.rs:46-50, fir.rs, signal_gen.rs): queued like a slider store. */
int dspfx_set_mode(dspfx_engine *e, int node, int mode);
/* Where the stores took effect.  `frame` = frames the engine had been handed (dspfx_frames_submitted) when the store
 * was applied: the store governs every frame from that one on -- always a boundary between two process calls.
 * Copies the applied stores with seq > after_seq, oldest first, into dst[cap]; returns how many (the engine keeps the
 * most recent 4096). */
typedef struct dspfx_param_event {
    uint64_t seq;     /* 1, 2, ... in the order the stores were made on this engine */
    uint64_t frame;
    int32_t node;
    int32_t param;    /* -1: a mode store (value = the mode) */
    float value;
    int32_t reserved;
} dspfx_param_event;
int dspfx_param_log(dspfx_engine *e, dspfx_param_event *dst, int cap, uint64_t after_seq);
/* Frames handed to the process calls since the engine was created (all sub-blocks counted). */
uint64_t dspfx_frames_submitted(const dspfx_engine *e);
/* Reverb::refresh_seconds (reverb.rs:55-71) with D explicit: a NEW zero ring, the same O(1) swap as a slider store (no wait
 * for the device).  A ring longer than the node's capacity has its missing groups allocated inside the call, on the calling
 * thread (DSPFX_ERR_OOM leaves the ring as it was); dspfx_reserve_delay_len beforehand, from any thread, moves that cost off
 * the thread that drives the blocks.  The node's seconds slider (params[1]) is left as it is. */
int dspfx_set_delay_len(dspfx_engine *e, int node, uint32_t delay_len);
/* Capacity hint -- the allocation half of Reverb::refresh_seconds (reverb.rs:60: `circular_buffer::<f32>(num_samples)`) made ahead of
 * the swap half (reverb.rs:70): allocate (not zero, not yet use) the 128-row groups a ring of delay_len samples at `node` would need beyond
 * what the node already has -- e.g. dspfx_delay_len(1.0f, page_round) once after dspfx_chain_set, and no seconds store can
 * allocate again.  Callable from any thread while blocks are running; takes no engine lock, launches nothing. */
int dspfx_reserve_delay_len(dspfx_engine *e, int node, uint32_t delay_len);
/* Give back delay-ring capacity beyond the rings' current lengths (and reservations not yet used) -- what dropping the old ring does in
 * the reference (reverb.rs:70: the previous (source, sink) pair is freed when `*guard` is overwritten), made explicit because here a
 * shorter ring keeps its groups.  Waits for the device. */
int dspfx_ring_trim(dspfx_engine *e);
/* Fir tap reload (fir.rs:153-171).  Like the reference it replaces the taps ONLY: the history is kept (`state`,
 * fir.rs:64-65, is never cleared), and because at most one sample is popped per step (fir.rs:193-197) a history longer
 * than the new tap count STAYS longer -- its oldest samples pair with the taps, i.e. the output is the new convolution
 * delayed by (old length - new length) samples -- while a shorter one goes on filling front-aligned like the warm-up.
 * dspfx_reset (or a new dspfx_chain_set) starts from an empty history. */
int dspfx_set_taps(dspfx_engine *e, int node, const double *taps_reversed, uint32_t n_taps, int mode);
/* How the FIR node's steady-state sweep multiplies (the reference accumulates in f64, fir.rs:201-216; every form below meets
 * the stated 1e-6 relative RMS bar and is bit-exact on data whose products and sums are exact in its operand width):
 *   DSPFX_FIR_PRECISION_HALF     every f32 operand as f16 hi + f16 lo (samples x 2^14, taps x a power of two: 22 significant
 *                                bits), THREE f16 products per term on the matrix pipe, f32 accumulation: 3e-7 relative RMS at
 *                                4096 taps like the others, and the fastest (the sweep becomes HBM-bound).  f16's range is
 *                                narrow: the sweep tracks every channel's peak over the window it swept and lists the tiles with
 *                                a channel at 3.998 or above, or below 2^-13 (-78 dBFS) without being silent; the SPLIT sweep,
 *                                launched right behind it over the listed tiles only (usually none), redoes those.  Whole
 *                                128-frame slices while the tap tables fit the LDS (<= ~5000 taps);
 *   DSPFX_FIR_PRECISION_SPLIT    every f32 operand split exactly into three bf16 parts, six bf16 products per term: any f32
 *                                range (bf16 has f32's exponent), 1.5 x faster than F32, 1.5 x slower than HALF;
 *   DSPFX_FIR_PRECISION_F32      f32 products on the f32 matrix pipe (v_mfma_f32_32x32x2_f32), always;
 *   DSPFX_FIR_PRECISION_DEFAULT  HALF (round 4; DSPFX_FIR_HALF=0 in the environment makes it SPLIT, DSPFX_FIR_SPLIT=0 F32).
 * Takes effect from the next block; history and taps are untouched. */
typedef enum dspfx_fir_precision {
    DSPFX_FIR_PRECISION_DEFAULT = 0,
    DSPFX_FIR_PRECISION_F32 = 1,
    DSPFX_FIR_PRECISION_SPLIT = 2,
    DSPFX_FIR_PRECISION_HALF = 3
} dspfx_fir_precision;
int dspfx_set_fir_precision(dspfx_engine *e, int node, int precision);
/* Zero every node's DSP state (fresh nodes); parameters are kept.  Asynchronous: the clears are queued on the stream
 * the engine was last driven on, behind the blocks in flight there (delay rings are not rewritten at all: their next D
 * frames read zeros, see dspfx_set_param). */
int dspfx_reset(dspfx_engine *e);

/* ---- the hot path ------------------------------------------------------ */
/* One block through the whole chain for all N channels == what N reference
 * graphs do in `Perform::perform` x chain length (node.rs:267-352).
 *   in    : device ptr, [n_frames][N] f32
 *   side  : device ptr or NULL, [n_frames][N]: port "b" of ADD/MIX nodes
 *           (NULL = unconnected port = zeros, node.rs:288)
 *   out   : device ptr, [n_frames][N] (may alias `in`)
 *   mix   : device ptr or NULL, [n_frames] f32: receives sum over this
 *           engine's channels of `out` per frame (the un-normalised mix bus,
 *           node.rs:181-183 before the division; deterministic order)
 *   stream: hipStream_t as void* (NULL = default stream); the call is
 *           asynchronous on that stream.
 * n_frames <= max_frames; DISTORT/Fuzz needs n_frames % 128 == 0 (it is
 * block-global over BUF_SIZE, distort.rs:146-172). */
int dspfx_process(dspfx_engine *e, const float *in, const float *side, float *out, float *mix,
                  uint32_t n_frames, void *stream);
/* dspfx_process with the Output node complete: mix[f] = (sum over this engine's channels of out[f][c]) /
 * dspfx_link_divisor(n_connected) -- nodes/output.rs:215-249 feeding collect_and_average (node.rs:162-194); n_connected
 * = 0 leaves the un-normalised sum (what a rank hands to dspfx_mix_allreduce).  The bus of THIS block, ready when the
 * block's samples are: the chain launch itself finishes the sum in its last workgroups (the workgroup that completes a
 * slice of partial sums reduces it, the one that completes the last slice writes the bus), no further kernel runs.
 * Fixed summation order: bit-identical from run to run and to every other form of the bus in this header. */
int dspfx_process_bus(dspfx_engine *e, const float *in, const float *side, float *out, float *mix, uint32_t n_frames,
                      uint64_t n_connected, void *stream);
/* One connected control port (`as_input` slider, dsp-stuff-derive/src/lib.rs:122-161): `param` is
 * the slider's index in dspfx_node_desc.params (GAIN level 0; DISTORT level 0; OVERDRIVE boost 0,
 * drive 1, level 2; MIX ratio 0; SIGNAL_GEN amplitude 0, frequency 1); `signal` is a device buffer in the sample layout.  Per sample the
 * slider takes lo + (hi-lo)*clamp((x+1)/2, 0, 1) over its reference range; the first value of each
 * 128-frame block is latched per channel and keeps applying once the port is disconnected
 * (lib.rs:148-151) until dspfx_set_param overwrites it.  Every DISTORT mode takes the port, Fuzz included
 * (distort.rs:176-180 maps it before the mode switch; fuzz zips it per sample, 154-160). */
typedef struct dspfx_ctl {
    int32_t node;
    int32_t param;
    const float *signal;
} dspfx_ctl;
int dspfx_process_ctl(dspfx_engine *e, const float *in, const float *side, float *out, float *mix,
                      uint32_t n_frames, const dspfx_ctl *ctl, int n_ctl, void *stream);
/* Placement tuning against the caller's own buffers.  Large delay rings are tables of separately allocated
 * 128-row groups, and how fast a group streams depends on where it landed physically RELATIVE to the sample
 * buffers it is streamed with (placement).  dspfx_chain_set already keeps the fastest of up to 2x
 * candidate groups, judged with scratch buffers; this call repeats that with the real chain kernels reading
 * `in` and writing `out` -- the buffers the host will keep using -- and keeps the fastest groups again.
 * `in` / `out` are laid out like a block of max_frames frames; n_frames <= 128 of it are streamed per probe (`out` is
 * overwritten).  About 3 s at 94 GiB.  DSP state is PRESERVED -- filter state is snapshotted and restored, every ring
 * group's rows are parked while it is probed and end up at the same ring position, the rows the probe blocks overwrite
 * in every OTHER delay ring and in FIR histories are parked and put back -- so a live host can call it again after it
 * re-allocated its buffers (flush the mix pipeline first).  Results never change, only speed. */
int dspfx_tune_placement(dspfx_engine *e, const float *in, const float *side, float *out, uint32_t n_frames,
                         void *stream);
/* Page-locked host memory for the blocks handed to dspfx_process_host.  From ordinary (pageable) buffers the two
 * copies of a block run one after the other; from these buffers dspfx_process_host cuts the block into channel
 * parts and overlaps upload, kernel and download (both directions of the bus busy; DESIGN.md, host buffers).  A host
 * that gathers its pipes into one block anyway should gather into these. */
int dspfx_host_alloc(size_t bytes, void **out);
int dspfx_host_free(void *p);
/* Same with HOST buffers (what a Rust `process(&[f32], &mut [f32])` holds):
 * H2D copy, process, D2H copy, synchronous. */
int dspfx_process_host(dspfx_engine *e, const float *in, const float *side, float *out, float *mix,
                       uint32_t n_frames);
/* ---- device sample formats at the boundary -------------------------------------------------------------
 * The reference's device boundary takes whatever sample type the sound card speaks (cpal's SampleFormat,
 * devices.rs:305-350) and converts it at the edge with dasp_sample 0.11.0 (Cargo.lock:1267-1269):
 *   input   do_read_1 / do_read_2 (devices.rs:227-260): to_sample into f32 (devices.rs:235, 253); a 2-channel device
 *           is folded to mono as to_f32(a) + to_f32(b) -- one f32 add, no halving;
 *   output  do_write_1 / do_write_2 (devices.rs:394-498): from_sample of each f32 (devices.rs:424, 432, 477, 488); a
 *           2-channel device gets the same sample in both slots (o.fill(x), devices.rs:476-490).
 * The rules, AS RECALLED (the crate is not vendored; they are restated once, in pcm_rules.h to_f32 / from_f32):
 *   I16  to f32: s / 32768.0f                    from f32: x * 32768.0f, truncated toward zero, saturated, NaN -> 0
 *   U16  to f32: (s - 32768) / 32768.0f          from f32: the I16 result + 32768 (bit pattern ^ 0x8000)
 *   I32  to f32: (float)s / 2147483648.0f        from f32: x * 2147483648.0f, truncated toward zero, saturated, NaN -> 0
 *   F32  identity                                identity
 * (the float -> int rule is Rust's `as`: no dither, no rounding).
 * Layout: every PCM buffer follows the engine's sample layout element by element (frame-major, or channel-tiled
 * under tile_channels); with 2 device channels each element is an adjacent pair (a, b).  `mix` stays f32 and means
 * what it means in dspfx_process: the Output node's f32 sum.  Any other format or channel count is DSPFX_ERR_INVALID.
 * {F32, 1, F32, 1} gives the same bits as dspfx_process / dspfx_process_host. */
typedef enum dspfx_sample_format {
    DSPFX_SAMPLE_F32 = 0,
    DSPFX_SAMPLE_I16 = 1,
    DSPFX_SAMPLE_U16 = 2,
    DSPFX_SAMPLE_I32 = 3
} dspfx_sample_format;
typedef struct dspfx_pcm_io {
    int32_t in_format;     /* dspfx_sample_format of `in` AND `side` */
    int32_t in_channels;   /* 1, or 2: interleaved device frames (a, b) -> to_f32(a) + to_f32(b)   devices.rs:244-258 */
    int32_t out_format;    /* dspfx_sample_format of `out` */
    int32_t out_channels;  /* 1, or 2: each output sample written to both slots                  devices.rs:476-490 */
} dspfx_pcm_io;
/* dspfx_process with device buffers in device sample formats; asynchronous on `stream`.  Widens `in` (and `side`)
 * into engine-owned f32 scratch, runs the block as dspfx_process does, narrows into `out` (may alias `in`: the three
 * steps are in stream order).  The scratch is shared with dspfx_process_host: calls on different streams are ordered
 * like every other call on the engine (see "Threads and streams" above). */
int dspfx_process_pcm(dspfx_engine *e, const dspfx_pcm_io *io, const void *in, const void *side, void *out,
                      float *mix, uint32_t n_frames, void *stream);
/* dspfx_process_host with host buffers in device sample formats; synchronous.  From page-locked buffers the block is
 * pipelined in channel parts exactly when dspfx_process_host's would be; each part crosses the bus in its device format
 * and is widened / narrowed on the GPU. */
int dspfx_process_host_pcm(dspfx_engine *e, const dspfx_pcm_io *io, const void *in, const void *side, void *out,
                           float *mix, uint32_t n_frames);
/* Pipelined mix bus.  dspfx_process(mix != NULL) / dspfx_process_bus finish the bus inside the chain launch (a few
 * microseconds at its tail; a chain that ends in a FIR node, an odd block length or DSPFX_MIX_TAIL=0 take two small
 * kernels behind it instead).  The forms below move even that off the block's own launch, at the price of delivering
 * the bus late:
 *   dspfx_process_partials(stream A): the chain, leaving per-wavefront partial sums in one of two
 *       engine-owned buffers (n_frames must not exceed the shortest delay line);
 *   dspfx_mix_collect(stream B): B waits for that chain kernel, reduces the partials into
 *       mix[n_frames] in fixed order.  The next block's chain kernel on A does not wait for it
 *       (it only waits, two blocks later, before reusing the same partial buffer).
 * Every dspfx_process_partials must be followed by exactly one dspfx_mix_collect. */
int dspfx_process_partials(dspfx_engine *e, const float *in, const float *side, float *out,
                           uint32_t n_frames, void *stream);
int dspfx_mix_collect(dspfx_engine *e, float *mix, uint32_t n_frames, void *stream);
/* Mix bus pipelined INSIDE the chain kernel: no second stream, no events, no extra launches.  The launch of
 * block k also runs, in its first 65 workgroups, the slice reduction of block k-1's partials and the final
 * reduction (+ the Output hop when n_connected != 0) of block k-2, so `mix` receives the bus of the block
 * submitted TWO calls earlier (it is not written by the first two calls after a flush / reset; it may be NULL
 * there).  Same reduction tree as dspfx_process(mix) and dspfx_mix_collect: bit-identical sums.  n_frames must
 * stay the same between flushes and must not exceed the shortest delay line.
 * dspfx_mixpipe_flush drains the pipeline with stand-alone kernels: mix_older <- the block before the last one
 * (may be NULL when only one block is in flight), mix_newer <- the last block. */
int dspfx_process_mixpipe(dspfx_engine *e, const float *in, const float *side, float *out, float *mix,
                          uint32_t n_frames, uint64_t n_connected, void *stream);
int dspfx_mixpipe_flush(dspfx_engine *e, float *mix_older, float *mix_newer, uint64_t n_connected, void *stream);
/* Output-node hop of the mix bus (node.rs:189-191): mix[f] /= link_divisor(n_connected),
 * in place on the device; call after the cross-GPU all-reduce with the GLOBAL channel count. */
int dspfx_mix_finish(dspfx_engine *e, float *mix, uint32_t n_frames, uint64_t n_connected, void *stream);

/* ---- the mix bus across GPUs ------------------------------------------------------------------------
 * Channels shard over the GPUs of a node with no data-path exchange; the one collective of the path is the mix bus:
 * the Output node's sum over ALL channels (nodes/output.rs:215-249 feeding node.rs:162-194).  Each rank owns one
 * engine; its un-normalised bus (dspfx_process_bus / dspfx_process(mix) / dspfx_process_mixpipe with n_connected = 0) is summed
 * over the ranks by ONE exchange of n_frames floats, then divided by f32(0.0001 + N_total).
 *
 * One process per GPU (several ranks may also share one device).  Rank 0 calls dspfx_comm_unique_id and hands the
 * DSPFX_COMM_ID_BYTES bytes to the other ranks over whatever channel the host already has (the Rust host's control socket, a
 * file, MPI); every rank then calls dspfx_comm_create(device, n_ranks, rank, id) -- collectively, it blocks until all ranks
 * have joined (DSPFX_COMM_TIMEOUT_MS, default 60 s).  Two backends, chosen by the rank that makes the id (DSPFX_COMM_BACKEND):
 *   mailbox (default)  a one-shot all-reduce by direct peer writes: every rank owns a mailbox in its device memory, opened by
 *                      its peers through hipIpc handles (exchanged via a shared-memory file named by the id: one node, which
 *                      is all xGMI spans); an exchange is ONE kernel of one workgroup per rank that writes its n_frames
 *                      {value, sequence} granules into every peer's mailbox over xGMI, then adds the n_ranks vectors of its
 *                      own mailbox IN RANK ORDER, ((0 + x_0) + x_1) + ..., and applies the Output hop.  The sum is the same
 *                      bits on every rank and from run to run by construction; latency is one peer write + one poll (a few
 *                      microseconds), what the 512-byte, latency-bound exchange wants (a ring or tree only adds hops).  Every
 *                      wait is bounded: a peer that never arrives gives NaNs and an error from the next call, not a hang.
 *                      Up to 16 ranks, n_frames <= 2048.
 *   rccl               ONE ncclAllReduce(sum, float, n_frames) in place + the Output hop.  RCCL is loaded at run time (the copy
 *                      already mapped into the process, else librccl.so.1): a host that never asks for it needs no RCCL.
 *                      Deterministic for a given rank count only as far as RCCL's topology search is.
 * n_ranks = 1 is allowed (id may be NULL: no exchange runs, the calls still divide).
 * dspfx_mix_allreduce is asynchronous on `stream`, in place on `mix` (device, n_frames f32), and applies the Output hop when
 * n_connected != 0: mix[f] = (sum over ranks of mix[f]) / dspfx_link_divisor(n_connected).  Calls on one communicator must be
 * made in the same order by every rank (they are counted). */
typedef struct dspfx_comm dspfx_comm;
#define DSPFX_COMM_ID_BYTES 128
int dspfx_comm_unique_id(void *id_out);
int dspfx_comm_create(int device, int n_ranks, int rank, const void *id, dspfx_comm **out);
void dspfx_comm_destroy(dspfx_comm *c);
int dspfx_comm_size(const dspfx_comm *c);
int dspfx_comm_rank(const dspfx_comm *c);
const char *dspfx_comm_last_error(const dspfx_comm *c);
/* "mailbox", "rccl" or "single" (one rank without an id). */
const char *dspfx_comm_backend(const dspfx_comm *c);
int dspfx_mix_allreduce(dspfx_engine *e, dspfx_comm *c, float *mix, uint32_t n_frames, uint64_t n_connected,
                        void *stream);

/* collect_and_average for a port with n_srcs connected pipes (node.rs:162-194), element-wise on whole
 * blocks: dst = (0 + srcs[0] + srcs[1] + ...) / f32(0.0001 + n_srcs), added in the order given.
 * n_srcs = 0 gives zeros (an unconnected port); n_srcs = 1 is the plain hop.  Device buffers in the
 * engine's sample layout; dst may alias one of the sources.  This is the only piece a graph with
 * fan-in needs besides the chain engines (dsp-stuff_amd/graph.py). */
int dspfx_link_average(dspfx_engine *e, const float *const *srcs, int n_srcs, float *dst, uint32_t n_frames,
                       void *stream);

/* ---- a whole graph in one kernel ------------------------------------------------------------------
 * The reference evaluates a saved graph (DSPConfig) node by node, every link a pipe through memory
 * (node.rs:267-352).  For a DAG of at most DSPFX_GRAPH_MAX_NODES fusable nodes (every kind except FIR and
 * Distort/Fuzz) the engine instead compiles ONE kernel for the graph at run time: node outputs live in
 * registers, every port's collect_and_average (node.rs:162-194) is arithmetic on them, and a block costs one
 * read of the Input node's buffer and one write of the Output node's, whatever the wiring.
 *
 * `nodes` are given in an order in which every link goes forward (src < dst).  A link connects the output of
 * node `src` (or DSPFX_GRAPH_INPUT: the block passed as `in`; DSPFX_GRAPH_INPUT2: the block passed as `side`;
 * DSPFX_GRAPH_ZERO: a connected pipe that carries zeros, the unselected output of a demux) to port `port` of node `dst` (dst == n_nodes: the Output
 * node, whose only port is MAIN; its value is the block written to `out`).  A port with k links averages
 * them in the order given, (0 + x1 + ... + xk) / f32(0.0001 + k); a port without links reads zeros (main,
 * "b") or keeps its slider value (slider ports).  Ports: DSPFX_PORT_MAIN, DSPFX_PORT_SIDE (port "b" of
 * ADD / MIX), DSPFX_PORT_SLIDER + k (the `as_input` port of slider k, dsp-stuff-derive/src/lib.rs:135-153).
 * The engine's link_flags do not apply (every hop is explicit), `side` of the process calls is DSPFX_GRAPH_INPUT2 and
 * control ports cannot be passed to dspfx_process_ctl.  Needs channels % 64 == 0 (whole waves).
 * DSPFX_ERR_UNSUPPORTED: the graph cannot be fused (too many nodes, a FIR / Fuzz node, channel count) or the
 * run-time compiler is unavailable: cut it into a series of such kernels (DSPFX_PORT_RAW, DSPFX_GRAPH_INPUT2: segment_plan in
 * dsp-stuff_amd/graph.py and include/dspfx_graph.hpp) or evaluate it run by run (graph.py).
 * dspfx_chain_set returns the engine to chain mode.  (dspfx_chain_set itself uses the same generated kernel for a
 * run of 9..16 fusable nodes without Add / Mix on engines above 131072 channels: one launch instead of two.) */
#define DSPFX_GRAPH_MAX_NODES 16
#define DSPFX_GRAPH_INPUT (-1)
#define DSPFX_GRAPH_ZERO (-2)
/* a second block from memory: the buffer passed as `side` to the process calls (must then be non-null).  Lets a graph
 * that was cut into consecutive kernels carry a signal AROUND a node that has a kernel of its own -- the dry path
 * beside a FIR cabinet: the kernel after the FIR node reads the FIR output as its Input and the dry signal here. */
#define DSPFX_GRAPH_INPUT2 (-3)
/* Regions of a graph that was cut into several kernels exchange more than two signals: a generated kernel may read up to
 * DSPFX_GRAPH_MAX_IO blocks and write up to DSPFX_GRAPH_MAX_IO blocks.  Inputs: DSPFX_GRAPH_INPUT (block 0),
 * DSPFX_GRAPH_INPUT2 (block 1), DSPFX_GRAPH_INPUT_N(k) for block k (= -(2 + k) from block 2 on); a link into an Add / Mix "b" port or a slider
 * port from one of them is a side input / control signal read from memory.  Outputs: dst == n_nodes is output block 0
 * (the Output node: `out`), dst == n_nodes + m output block m -- averaged like any port, or DSPFX_PORT_RAW to hand one
 * signal over untouched.  Blocks beyond `in` / `side` / `out` are passed with dspfx_process_io. */
#define DSPFX_GRAPH_MAX_IO 16
#define DSPFX_GRAPH_INPUT_N(k) ((k) == 0 ? DSPFX_GRAPH_INPUT : (k) == 1 ? DSPFX_GRAPH_INPUT2 : -(2 + (k)))   /* link source of input block k */
#define DSPFX_PORT_MAIN 0
#define DSPFX_PORT_SIDE 1
#define DSPFX_PORT_SLIDER 2
/* OR into `port`: the port's only link, taken as it is (no averaging, no division).  For cutting a large graph into
 * consecutive kernels at a point where a single signal crosses: the first kernel's Output link is RAW, the next
 * engine reads that buffer as its Input (dsp-stuff_amd/graph.py, segment_plan). */
#define DSPFX_PORT_RAW 256
typedef struct dspfx_graph_link {
    int32_t src;    /* producing node index, DSPFX_GRAPH_INPUT, DSPFX_GRAPH_INPUT2 or DSPFX_GRAPH_ZERO */
    int32_t dst;    /* consuming node index, or n_nodes for the Output node */
    int32_t port;   /* DSPFX_PORT_* of the consumer (| DSPFX_PORT_RAW) */
} dspfx_graph_link;
int dspfx_graph_set(dspfx_engine *e, const dspfx_node_desc *nodes, int n_nodes, const dspfx_graph_link *links,
                    int n_links);
/* dspfx_process for a graph engine with several input / output blocks: ins[k] = input block k (ins[0] = `in`, ins[1] =
 * `side`), outs[m] = output block m (outs[0] = `out`).  Entries the graph does not use may be NULL; n_ins, n_outs <=
 * DSPFX_GRAPH_MAX_IO.  `mix` sums output block 0. */
int dspfx_process_io(dspfx_engine *e, const float *const *ins, int n_ins, float *const *outs, int n_outs, float *mix,
                     uint32_t n_frames, void *stream);
/* The translation unit dspfx_graph_set would compile for this graph (the generated `struct Prog`; it includes
 * csrc/graph_kernel.hip.h), NUL-terminated into dst[cap].  Needs no engine and no device: for inspection and for
 * checking the generator where there is no GPU (without one every division is written in its IEEE form, since the
 * exact-division check runs on the device).  DSPFX_ERR_INVALID: bad graph or cap too small. */
int dspfx_graph_source(const dspfx_node_desc *nodes, int n_nodes, const dspfx_graph_link *links, int n_links,
                       char *dst, size_t cap);

/* ---- DSP state (parity tests; the reference never saves it) --- */
/* Size in bytes of node `node`'s exported state:
 *   BIQUAD 4*N f32 [x1|x2|y1|y2][N]; LOW/HIGH_PASS N f32; REVERB D*N f32
 *   [D][N] oldest sample first; others 0;
 *   FIR: the reference's `state: VecDeque<f64>` (fir.rs:64-65) as it stands -- a 32-byte header {u64 samples pushed
 *   since empty, u64 held = the deque's length, u32 VecDeque capacity, u32 VecDeque head, u32 n_taps, u32 0} followed
 *   by the held samples [held][N] f32, oldest first.  held < n_taps while the deque fills, == n_taps in steady state,
 *   > n_taps after a reload with a shorter impulse response: the size changes with the node's history, so ask right
 *   before exporting.  dspfx_state_import takes such a blob of any length (the size must match the blob's own header). */
int64_t dspfx_state_size(const dspfx_engine *e, int node);
int dspfx_state_export(dspfx_engine *e, int node, void *host_dst, size_t size);
int dspfx_state_import(dspfx_engine *e, int node, const void *host_src, size_t size);

/* ---- utilities --------------------------------------------------------- */
/* Synthetic white noise, identical integer hash on CPU and GPU:
 * dst[f][c] = noise(seed, channel_offset + c, n_abs0 + f), dst device [n_frames][N]. */
int dspfx_fill_noise(dspfx_engine *e, float *dst, uint32_t n_frames, uint32_t n_abs0, uint32_t seed,
                     void *stream);
/* Block until everything queued by this engine on `stream` has finished. */
int dspfx_sync(dspfx_engine *e, void *stream);
/* Human-readable plan of the current chain (stages, kernels, bytes/sample). */
int dspfx_describe(const dspfx_engine *e, char *dst, size_t cap);
/* Division by a wave-uniform constant c (the link divisor, SoftClip's 3.0, a clip level)
 * is evaluated as (float)((double)x * (1.0/c)) when that is bit-identical to IEEE f32
 * x / c for EVERY one of the 2^32 possible x.  That holds for every c that is not an even
 * integer (only those have exact ties among their subnormal quotients: csrc/chain_kernels.hip.h,
 * div_c); the engine takes it for granted there and runs this exhaustive check for even
 * integers.  The call runs the check on the device for ANY c and returns the number of
 * mismatching inputs (0 => the fast form is exact for c), so the rule itself is testable. */
int dspfx_verify_fast_division(int device, float c, uint64_t *mismatches);
/* The Tanh / Sin / Atan modes (distort.rs:109,117,125; overdrive.rs:38; chebyshev.rs:34,40; signal_gen.rs:64)
 * evaluate in f64 and round once.  The engine's own f64 tanh (func 0) / sin (func 1) / atan (func 2) are cheaper than the math library's; this compares the two
 * over all 2^32 inputs on the device: *mismatches = inputs whose f32 results differ, *max_ulp = the largest
 * distance among them (a handful of near-tie inputs, 1 ulp).  func 3: the f64 exp of Fuzz (distort.rs:159).
 * func 4..64: Fuzz's per-lane divisions (distort.rs:158,167,171) as f64 products with an IEEE fallback for
 * subnormal quotients, against IEEE division on 2^32 (numerator, hashed divisor) pairs; must report 0. */
int dspfx_verify_libm(int device, int func, uint64_t *mismatches, uint32_t *max_ulp);
/* Kernel timing for the roofline report: when enabled, every stage's main kernel
 * launch is bracketed by HIP events on the stream it is launched on.  read()
 * synchronises those events and returns, for the stage with the largest total,
 * the summed kernel time and the number of launches (and optionally resets). */
int dspfx_profile_enable(dspfx_engine *e, int enable /* 0 = off; n > 0 = on, pre-creating events for n launches */);
int dspfx_profile_read(dspfx_engine *e, double *total_ms, uint32_t *launches, char *kernel_name, size_t cap,
                       int reset);
/* Algorithmic HBM bytes per channel-sample of the current chain at n_frames. */
double dspfx_algorithmic_bytes_per_sample(const dspfx_engine *e, uint32_t n_frames);

/* ---- pitch detector bank ---------------------------------------------------------------------------------
 * The Pitch Detector node (nodes/pitch.rs:120-146) for N independent channels: a McLeod pitch and clarity per
 * channel.  A separate object, fed with blocks of samples; it is not a node kind of the chain.
 * Per channel, pitch.rs keeps a FIFO of samples; at the start of every process call, if it holds 1024 samples, it
 * runs McLeodDetector::new(1024, 512).get_pitch(oldest 1024, 48000, power, clarity, pick) on them and stores the
 * result when there is one, then drops those 1024 samples, and then appends the call's block.  So the windows are
 * samples [1024 w, 1024 w + 1024), consecutive, and window w has been detected once frames [0, F) have been pushed
 * with F >= 1024 (w + 1) + 1.  (This holds for any FIFO capacity of at least 1024 samples; rivulet's page-rounded
 * circular_buffer(128) of f32 holds 1024.)  A push of any length runs the windows that fall due, in order.
 * The detector (the pitch-detection crate, magnetophon's fork, Cargo.lock:3092-3096: not vendored, restated from
 * McLeod & Wyvill 2005 with pitch.rs's parameters, UNPINNED), for one window x[0..1024):
 *   power = sum x^2; power < power_thresh, a non-finite or an all-zero window: no result;
 *   r(tau), tau in [0, 1024): the circular autocorrelation of x zero-padded to 1536 (the crate's FFT length):
 *       r_lin(tau) + r_lin(1536 - tau) for tau > 512;
 *   m(tau): the energy of the same pairs, m_lin(tau) = sum_{j < 1024-tau} x_j^2 + sum_{j >= tau} x_j^2, plus
 *       m_lin(1536 - tau) for tau > 512; n(tau) = 2 r(tau) / m(tau) (0 where m <= 0);
 *   key maxima: after the positive lobe at tau = 0, the first largest n of every run with n > 0 (an open run counts);
 *   pick: the first key maximum with n >= pick_thresh * (largest key maximum); none, or its n < clarity_thresh:
 *       no result;
 *   parabola through its neighbours a, b, c: delta = (c - a) / (2 (2b - a - c)) (0 if that is 0/0 or tau = 1023),
 *       frequency = 48000 / (tau + delta), clarity = (b + (c - a) delta / 4) / n(0).
 * The result is held per channel (0, 0 initially) and replaced only when a window gives one.
 * Independence: a channel's result depends on its own window alone, whatever any other channel carries -- non-finite
 * samples, the largest float in every frame, or a level 2^200 away from its own.  (The kernel transforms two channels
 * at a time; each enters that pair scaled by its own power of two, and a non-finite channel enters it as zeros.)
 * Level: the result is the restatement's (within the f32 accuracy the tests state) for every finite window whose
 * max |x| is a normal float, 2^-126 <= max |x| <= FLT_MAX: frequency and clarity do not depend on the level, only
 * the power test does, and `power` is compared with power_thresh without overflow or underflow (in f64).  Outside
 * that range: a window with a NaN or an infinity gives no result, as above; a window whose max |x| is subnormal
 * (or 0) has power < 2^-242 and gives no result at any power_thresh > 0; at power_thresh <= 0 it is scaled by
 * 2^127 and detected like any other window, from the few significant bits its samples have (all zero: no result).
 * Layout: every block pushed is in the layout of the desc, exactly as dspfx_engine_desc's channels / tile_channels
 * (the tiled form for a block of n_frames).  The bank stores the samples in 128-frame slots, each in that layout. */
typedef struct dspfx_pitch dspfx_pitch;
typedef struct dspfx_pitch_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t channels;        /* N */
    uint32_t tile_channels;   /* 0 = frame-major; W = channel-tiled, as dspfx_engine_desc */
    float power_thresh;       /* pitch.rs sliders, default 0.5 each */
    float clarity_thresh;
    float pick_thresh;
} dspfx_pitch_desc;
/* which threshold dspfx_pitch_set_param stores */
typedef enum dspfx_pitch_param {
    DSPFX_PITCH_POWER = 0,
    DSPFX_PITCH_CLARITY = 1,
    DSPFX_PITCH_PICK = 2
} dspfx_pitch_param;
/* Samples per window (a slot holds DSPFX_BUF_SIZE = 128 frames; a window is 8 slots). */
#define DSPFX_PITCH_WINDOW 1024
int dspfx_pitch_create(const dspfx_pitch_desc *desc, dspfx_pitch **out);
int dspfx_pitch_destroy(dspfx_pitch *p);
/* Appends n_frames >= 1 frames (a device buffer in the desc's layout) and runs every detection that falls due, in
 * order; asynchronous on `stream`, stream-ordered like the process calls.  When `block` is dspfx_pitch_slot(p) and
 * n_frames is 128, the samples are already in place and nothing is copied. */
int dspfx_pitch_push(dspfx_pitch *p, const float *block, uint32_t n_frames, void *stream);
/* The device address where the next 128 frames belong (a 128-frame block in the desc's layout), so that an engine can
 * write its output there and push it without a copy; NULL while the frames pushed are not a multiple of 128.
 * The slot may still be read by the detection the previous push launched: a write into it must be stream-ordered
 * after the previous dspfx_pitch_push (the same stream, or one that waits for it). */
float *dspfx_pitch_slot(dspfx_pitch *p);
/* Stores a threshold (dspfx_pitch_param); it applies to every detection a later push launches.  Any thread. */
int dspfx_pitch_set_param(dspfx_pitch *p, int which, float value);
/* Writes the held results into device arrays freq[N], clarity[N]; asynchronous on `stream`. */
int dspfx_pitch_read(dspfx_pitch *p, float *freq, float *clarity, void *stream);
/* Back to the state after create: no samples, results 0 (queued on the stream last used); the thresholds stay. */
int dspfx_pitch_reset(dspfx_pitch *p);
/* Windows detected so far (since create or reset). */
int64_t dspfx_pitch_windows(const dspfx_pitch *p);

/* ---- output resampler bank -----------------------------------------------------------------------------
 * The reference's output stream runs at whatever rate the device offers closest to 48 kHz (devices.rs:513-527) and
 * resamples every output callback from 48 kHz to it (devices.rs:394-498, 549-555) with dasp's Converter over a
 * 16-frame Sinc.  This bank does that for N channels that share one device rate: blocks of engine output are pushed
 * into a FIFO, and each pull is one output callback.  A separate object like the pitch bank; input streams are opened
 * at 48 kHz by the reference and are never resampled, so there is no input direction.
 * The rules (dasp_signal 0.11.0 interpolate::Converter, dasp_interpolate 0.11.0 sinc::Sinc over
 * ring_buffer::Fixed<[f32; 16]>: not vendored, restated AS RECALLED, UNPINNED; include/dspfx_ir.hpp resample_dasp_sinc is
 * the same state machine over f64 frames), per channel:
 *   converter    ratio = 48000.0 / target_hz (f64); value = 0.0 at the start.  One output frame: while value >= 1.0
 *                { pull one source frame into the interpolator; value -= 1.0 }; interpolate at value; value += ratio.
 *   interpolator a ring of 16 frames, 0.0 at the start; a pulled frame enters at the back (ring[15]) and ring[0] drops
 *                out; idx climbs by one per pulled frame up to 8.  At phase x: nl = idx, nr = idx + 1; depth = 8 once
 *                idx >= 7, idx + 1 before.  v = 0.0f; for n in 0 .. depth, left tap then right tap:
 *                    a = PI * (phase + n)            phase = x on the left, 1 - x on the right
 *                    coeff = (a == 0 ? 1 : sin(a) / a) * (0.5 + 0.5 * cos(a / 8))                       (f64)
 *                    v = v + (f32)(coeff * (f64)ring[k])      k = nl - n on the left, (nr + n) % 16 on the right
 *                one f64 product rounded once to f32, f32 adds in that order, nothing contracted.  The % 16 is the
 *                ring indexing modulo its length: in steady state the last right tap reads ring[0], the OLDEST frame.
 *   callback     for n_out device frames: input_len = (size_t)((f32)n_out * (48000.0f / (f32)target_hz)), in f32.
 *                Fewer than input_len frames waiting: every output slot is from_sample(0.0), nothing is consumed and the
 *                converter is not touched (an underrun).  Otherwise the converter sees ALL waiting frames, makes
 *                exactly n_out frames and pulls what its state needs (input_len - 1, input_len or input_len + 1 occur);
 *                a pull past the last waiting frame yields 0.0 and is not counted (CountingSignal, devices.rs:376-388);
 *                the frames pulled from the FIFO are released.  Each f32 goes through from_sample (the rules of the
 *                "device sample formats" section); a 2-channel device gets it in both slots.
 * The phases and coefficients depend on the call sequence only, never on samples: the host computes them
 * (dspfx_resample_plan, f64, the C library's sin / cos) and the kernel multiplies and adds.
 * Layout: the FIFO is `slots` slots of `block_frames` frames, each slot in the desc's layout for a block of block_frames
 * frames (channels / tile_channels as dspfx_engine_desc), so an engine can write its output into dspfx_resample_slot
 * and the push copies nothing.  A pull's `out` is in the same layout for a block of n_out frames, in the device format:
 * element (f, c) is one device frame of out_channels samples. */
typedef struct dspfx_resample dspfx_resample;
typedef struct dspfx_resample_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t channels;        /* N */
    uint32_t tile_channels;   /* 0 = frame-major; W = channel-tiled, as dspfx_engine_desc */
    uint32_t block_frames;    /* frames per FIFO slot, 1 ..= DSPFX_RESAMPLE_MAX_FRAMES (an engine's block: 128) */
    uint32_t slots;           /* FIFO capacity = slots * block_frames frames; at least 3 */
    uint32_t target_hz;       /* the device's rate, > 0; 48000 is NOT a bypass (the reference resamples then too) */
    int32_t out_format;       /* dspfx_sample_format of a pull's `out` */
    int32_t out_channels;     /* 1, or 2: each output sample written to both slots   devices.rs:476-490 */
} dspfx_resample_desc;
/* The most device frames one pull makes, and the most frames a slot holds. */
#define DSPFX_RESAMPLE_MAX_FRAMES 4096
/* A bad descriptor (no channels, a tile that is not a power of two dividing N, block_frames out of range, slots < 3,
 * target_hz 0, an unknown format, a channel count other than 1 or 2) is DSPFX_ERR_INVALID. */
int dspfx_resample_create(const dspfx_resample_desc *desc, dspfx_resample **out);
int dspfx_resample_destroy(dspfx_resample *r);
/* Appends n_frames >= 1 frames (a device buffer in the desc's layout for a block of n_frames); asynchronous on
 * `stream`.  When `block` is dspfx_resample_slot(r), n_frames must be block_frames: the samples are in place and nothing
 * is copied.  More frames than the FIFO has room for: DSPFX_ERR_STATE, nothing changed. */
int dspfx_resample_push(dspfx_resample *r, const float *block, uint32_t n_frames, void *stream);
/* The device address where the next block_frames frames belong, so that an engine can write its output there and push
 * it without a copy; NULL while the frames pushed are not a multiple of block_frames, or the FIFO has no whole slot
 * free.  A write into it must be stream-ordered after the pulls issued so far (the same stream, or one that waits). */
float *dspfx_resample_slot(dspfx_resample *r);
/* One output callback: n_out (1 ..= DSPFX_RESAMPLE_MAX_FRAMES) device frames of every channel into `out`;
 * asynchronous on `stream`, stream-ordered.  *consumed = the frames released from the FIFO and *underrun = 1 when the
 * callback found fewer than input_len frames (then *consumed = 0 and `out` is silence in the device format: 0x8000
 * for U16); both are host values, known when the call returns (they depend on the counters only). */
int dspfx_resample_pull(dspfx_resample *r, void *out, uint32_t n_out, uint32_t *consumed, int32_t *underrun,
                        void *stream);
/* Frames waiting in the FIFO (a host counter: no device wait); negative: a dspfx_status. */
int64_t dspfx_resample_available(dspfx_resample *r);
/* Drops the oldest n_frames waiting frames unseen by the converter (the catch-up of devices.rs:410-432 is
 * `skip(available - input_len)` before a pull; when to do it is the host's policy).  More than are waiting:
 * DSPFX_ERR_INVALID, nothing changed. */
int dspfx_resample_skip(dspfx_resample *r, uint32_t n_frames);
/* Back to the state after create: ring 0.0 (queued on the stream last used), value = 0, idx = 0, FIFO empty. */
int dspfx_resample_reset(dspfx_resample *r);
/* PURE HOST function (no GPU, no bank): the plan of the next n_out output frames from the converter state (*value,
 * *idx), which it updates.  For output frame o: advance[o] = source frames pulled first, depth[o] = the tap pairs
 * summed, coeff[16 * o + 2 n] / [16 * o + 2 n + 1] = the left / right coefficient of tap n (0.0 from 2 * depth[o] on).
 * advance, depth and coeff may be NULL (only the state is stepped).  *input_len = the callback's f32 figure above,
 * *pulled = the sum of advance (what the converter asks for; a view shorter than that feeds 0.0).  Either may be NULL.
 * dspfx_resample_pull runs exactly this plan. */
int dspfx_resample_plan(uint32_t target_hz, double *value, uint32_t *idx, uint32_t n_out, uint32_t *advance,
                        uint32_t *depth, double *coeff, uint32_t *input_len, uint32_t *pulled);

/* ---- spectrogram bank ------------------------------------------------------------------------------------
 * The Spectrogram node (nodes/spectrogram.rs:225-268) for N independent channels: one column of per-bin volumes per
 * channel for every fft_size frames.  A separate object like the pitch and resampler banks; it is not a node kind.
 * Per call, spectrogram.rs gathers exactly fft_size frames of its "in" port (collect_and_average), hands them to
 * audioviz's Processor::compute_all(), pushes the column onto a queue that keeps the newest buffer_size columns, and
 * releases fft_size frames.  So the windows are frames [n w, n (w + 1)), back to back, no overlap, and window w is due
 * as soon as n (w + 1) frames have been pushed (the Pitch node needs one frame more; this node does not).
 * What compute_all() does (audioviz 0.6.0 with apodize 1.0.0 and rustfft 6.2.0, Cargo.lock:465-474: not vendored, restated
 * AS RECALLED, UNPINNED): a window function over the buffer, a forward complex FFT, the norm of the first n/2 outputs, a
 * per-bin volume normalisation, a frequency label per bin and a bound on those labels.  The only sample-dependent step is
 * |FFT(window * x)[k]|, k in [0, n/2); everything else is a factor or a label that depends on the bin index alone.  So the
 * GPU computes
 *       vol[k] = |FFT(window * x)[k]| * gain[k]        k in [0, n/2)
 * in f32 (window product rounded once; magnitude sqrtf(re * re + im * im) of the two components scaled by one exact power of
 * two, so that the squares stay inside f32's range; then the gain product), and window[n] and
 * gain[n/2] are TABLES THE HOST SUPPLIES: what is not pinned is confined to them, and a maintainer who has the crates can
 * replace them without a new kernel.
 * Independence: a channel's column depends on its own window alone, whatever any other channel carries -- non-finite
 * samples, or a level 2^200 away from its own.  (Every channel has a transform of its own.)
 * Level: the column is the restatement's (within the f32 accuracy the tests state, relative to the channel's own level) for
 * every finite window whose peak window product max |window[i] * x[i]| is a normal float, >= 2^-126, and whose samples keep
 * 2 n max |x| below FLT_MAX, so that no sum of the transform overflows; at ordinary levels the scale changes no bit.
 * Outside that range: a window product that is NaN -- a NaN sample, or an infinity under a window entry of 0, as the default
 * window's first and last -- makes every bin of the column NaN; any other infinity makes every bin NaN or +inf; no bin is
 * ever negative or -inf; a finite window above the range gives +inf or NaN in some bins; a window whose products are all
 * subnormal is transformed as it is, nothing flushed (a constant k * 2^-149 under a window of ones gives n k 2^-149 in
 * bin 0 exactly), but its accuracy relative to its own level is not stated; an all-zero window, of either sign, gives +0.0
 * in every bin.
 * The defaults:
 *   window = NULL   the symmetric Hann window 0.5 - 0.5 cos(2 pi i / (n - 1)), f64 rounded once to f32 (apodize's
 *                   hanning_iter as recalled); entries n - 1 - i repeat entries i < n/2, so it is symmetric bit for bit
 *   gain = NULL     1.0 for every bin.  audioviz's VolumeNormalisation::Mixture curve is not restated here: a caller
 *                   that wants it passes it as `gain`.
 * Frequency bounds (lower_bound ..= upper_bound) are not the bank's business: a column always holds all n/2 bins, and
 * the host maps a bound to a bin range with the physical bin frequency k * 48000 / n (dspfx_spectrum_plan).
 * Layout: every block pushed is in the layout of the desc (channels / tile_channels as dspfx_engine_desc, the tiled form
 * for a block of n_frames).  The window store is fft_size / 128 + 1 slots of 128 frames, each in that layout.  A column
 * is a block of fft_size / 2 "frames" in the same layout: element (k, c), bin k of channel c, is frame k of channel c
 * (frame-major: [k][N]).
 * Memory: the bank allocates columns * (fft_size / 2) * channels * 4 bytes of history plus
 * (fft_size / 128 + 1) * 128 * channels * 4 bytes of window store (250 columns of 256 bins at 2^20 channels are 268 GB:
 * the caller chooses `columns`).  An allocation that fails is DSPFX_ERR_OOM, never an abort. */
typedef struct dspfx_spectrum dspfx_spectrum;
typedef struct dspfx_spectrum_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t channels;        /* N */
    uint32_t tile_channels;   /* 0 = frame-major; W = channel-tiled, as dspfx_engine_desc */
    uint32_t fft_size;        /* n: a power of two, DSPFX_SPECTRUM_MIN_FFT ..= DSPFX_SPECTRUM_MAX_FFT (the node's default: 512) */
    uint32_t columns;         /* history depth >= 1: the node's buffer_size (its default: 250) */
    const float *window;      /* host, [fft_size], read at create and copied; NULL = the Hann window above */
    const float *gain;        /* host, [fft_size / 2], read at create and copied; NULL = 1.0 */
} dspfx_spectrum_desc;
/* The node's slider range for fft_size (spectrogram.rs:142). */
#define DSPFX_SPECTRUM_MIN_FFT 128
#define DSPFX_SPECTRUM_MAX_FFT 8192
/* fft_size outside the slider range, columns 0, no channels, a tile that is not a power of two dividing N: DSPFX_ERR_INVALID.
 * fft_size inside the range but not a power of two: DSPFX_ERR_UNSUPPORTED (rustfft takes any length; this bank does
 * not).  All of that is checked before any device work. */
int dspfx_spectrum_create(const dspfx_spectrum_desc *desc, dspfx_spectrum **out);
int dspfx_spectrum_destroy(dspfx_spectrum *p);
/* Appends n_frames >= 1 frames (a device buffer in the desc's layout) and computes the column of every window that
 * falls due, in order; asynchronous on `stream`, stream-ordered like the process calls.  When `block` is
 * dspfx_spectrum_slot(p) and n_frames is 128, the samples are already in place and nothing is copied. */
int dspfx_spectrum_push(dspfx_spectrum *p, const float *block, uint32_t n_frames, void *stream);
/* The device address where the next 128 frames belong (a 128-frame block in the desc's layout), so that an engine can
 * write its output there and push it without a copy; NULL while the frames pushed are not a multiple of 128.
 * The slot may still be read by the column the previous push launched: a write into it must be stream-ordered after
 * the previous dspfx_spectrum_push (the same stream, or one that waits for it). */
float *dspfx_spectrum_slot(dspfx_spectrum *p);
/* The device address of the column `age` windows back (0 = the newest), fft_size / 2 * channels floats in the layout
 * above; NULL when that column does not exist yet or age >= columns.  The column of window w is overwritten by the push
 * that completes window w + columns; a read must be stream-ordered after the push that launched it (the same stream,
 * or one that waits for it) and done before that later push. */
const float *dspfx_spectrum_column(dspfx_spectrum *p, uint32_t age);
/* Back to the state after create: no samples, no columns; the tables stay. */
int dspfx_spectrum_reset(dspfx_spectrum *p);
/* Windows computed so far (since create or reset). */
int64_t dspfx_spectrum_windows(const dspfx_spectrum *p);
/* PURE HOST function (no GPU, no bank): the default window table, window_out[fft_size], and the physical frequency of
 * every bin, bin_hz_out[fft_size / 2] = k * 48000 / fft_size (exact in f32).  Either may be NULL.  The same size rules
 * as dspfx_spectrum_create.  A host that wants a scaled Hann window scales this table and passes it as `window`. */
int dspfx_spectrum_plan(uint32_t fft_size, float *window_out, float *bin_hz_out);

/* ---- mix groups: one Output bus per channel range ---------------------------------------------------------
 * The reference allows any number of Output nodes, each averaging only the pipes wired to it (nodes/output.rs:215-249
 * feeding collect_and_average, node.rs:162-194); the engine's own mix bus is ONE sum over all its channels.  This bank
 * gives a host with many rooms of channels one bus per room, and every channel its own level in its room's mix: a table of
 * G contiguous channel ranges ("groups") and an optional per-channel fader, over a device block in the engine's sample
 * layout (channels / tile_channels as dspfx_engine_desc, the tiled form for a block of n_frames):
 *       buses[f][g] = (sum over the channels c of group g of fl32(x[f][c] * gain[c])) / dspfx_link_divisor(n_g)
 * n_g = the group's channel count.  The product is one f32 multiply, never contracted into the add: a Gain node in front
 * of the Output node, x * level (gain.rs:25-38); a channel without a stored fader is not multiplied.  The division is an
 * IEEE f32 division; normalise = 0 leaves the raw sums (a host that splits a group over ranks exchanges those and divides
 * itself).  An empty group gives +0.0.  A separate object like the other banks; it reads the block once and changes nothing.
 * `buses` is [n_frames][G] f32 on the device: the frame-major layout of a G-channel engine, so it can go straight into a second
 * engine of G channels (tile_channels = 0) as a master-bus chain, or into a resampler, pitch or spectrogram bank of G channels.
 * Summation order: fixed, and for one group a function of the group's first channel and length (and the layout) alone -- the
 * bus of a group is the same bits whatever the rest of the table looks like, from run to run and on any stream; no atomics.
 * Channels are cut into spans of 256 from channel 0.  A span wholly inside the group: a lane adds four adjacent channels
 * (x0 + x1) + (x2 + x3), the 64 lanes are added pairwise across lane bits 32, 16, 8, 4, 2, 1.  A span the group shares: per
 * 64 channels a segmented scan with steps 1, 2, .. 32, carried from one 64 to the next.  The spans' sums are added 64 at a
 * time: four rows of up to 16 one after the other, then (r0 + r1) + (r2 + r3); more than 64 take further rounds of the same.
 * The longest chain of dependent additions D(n) this makes for a group of n channels is at most 64 + ceil(log2(max(n, 1)))
 * (47 at 2^24 channels); dspfx_mixgroups_plan reports it per group.  Not the reference's order (sequential): within
 * (D + 1) 2^-24 sum|terms| / divisor of the exact sum. */
typedef struct dspfx_mixgroups dspfx_mixgroups;
typedef struct dspfx_mixgroups_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t n_channels;      /* N */
    uint32_t max_frames;      /* largest n_frames a run will pass (>= 1) */
    uint32_t tile_channels;   /* 0 = frame-major; W = channel-tiled, as dspfx_engine_desc */
    uint32_t n_groups;        /* G >= 1 */
    uint32_t normalise;       /* 1: divide by the link divisor of the group's channel count; 0: the raw sums */
    const uint64_t *group_start; /* host, [n_groups + 1], read at create and copied: group g is channels [group_start[g],
                                 group_start[g + 1]); nondecreasing, [0] = 0, [G] = N; boundaries need not align with anything */
} dspfx_mixgroups_desc;
/* A bad descriptor or table is DSPFX_ERR_INVALID with the reason in dspfx_mixgroups_last_error of a NULL bank (kept per
 * thread); all of that is checked before any device work. */
int dspfx_mixgroups_create(const dspfx_mixgroups_desc *desc, dspfx_mixgroups **out);
int dspfx_mixgroups_destroy(dspfx_mixgroups *m);
/* The reason of the bank's last failed call; of a NULL bank: of this thread's last failed create or plan. */
const char *dspfx_mixgroups_last_error(const dspfx_mixgroups *m);
/* block: device, n_frames frames in the desc's layout (1 <= n_frames <= max_frames); buses: device, [n_frames][G] f32.
 * Asynchronous on `stream`; a run on another stream than the one before first waits (on the device) for that one, since the
 * partial sums are the bank's.
 * The sign of a zero bus is the reference's: collect_and_average (node.rs:162-194) starts from +0.0 and adds pipe by pipe, so a
 * group whose terms are all -0.0 (samples of -0.0, or silence through a negative fader: +0.0 * -1.0) gives +0.0, not the -0.0 a
 * tree of additions gives.  The bank writes +0.0 + sum wherever a finished sum becomes a bus, ahead of the division; that changes
 * no other value.  The raw sums that dspfx_mixgroups_returns subtracts from are the same, so such a group's returns are +0.0 too. */
int dspfx_mixgroups_run(dspfx_mixgroups *m, const float *block, uint32_t n_frames, float *buses, void *stream);
/* Per-channel returns: every participant of a room has an Output node of their own, wired to the OTHER n_g - 1 channels of
 * the room, so that nobody hears themself.  With t[f][c] = fl32(x[f][c] * gain[c]) (x[f][c] itself for a channel without a
 * stored fader: the terms dspfx_mixgroups_run sums), for channel c of group g:
 *       returns[f][c] = fl32( fl32(S[f][g] - t[f][c]) / dspfx_link_divisor(n_g - 1) )      n_g >= 2
 *       returns[f][c] = +0.0                                                               n_g == 1
 * S[f][g] is the group's RAW sum exactly as this bank computes it: the bits a bank with the same table, layout and
 * normalise = 0 writes as its bus.  One f32 subtraction, then one IEEE f32 division by the f32 divisor of n_g - 1 connected
 * pipes (node.rs:166,179); nothing is contracted.  A group of one channel has no other pipe: the reference's unconnected
 * port stays zeroed (node.rs:288), so the return is +0.0 whatever the sample is, NaN included.  normalise = 0 leaves the
 * division out: returns = fl32(S - t).  Otherwise edge values are what that arithmetic gives: a channel carrying +inf gets
 * inf - inf = NaN in its own return and +inf in the others', a NaN channel makes every return of its room NaN.
 * Not the reference's order (which adds the other n_g - 1 pipes one after the other): within
 *       (D + 2) 2^-24 (sum over the WHOLE group of |t|) / divisor + 2^-24 |ref| + 2^-149
 * of the exact sum of the others, D = the group's depth from dspfx_mixgroups_plan; one rounding more than the bus, for the
 * subtraction.  The bound is absolute and taken over the whole group's terms: a channel that dominates its room gets a
 * return with a poor relative error, because of cancellation.  That is the known price of mix-minus, and it is what makes
 * the cost O(n) instead of O(n^2).
 * block, returns: device, n_frames frames in the desc's layout (1 <= n_frames <= max_frames).  returns == block works in
 * place (a thread rewrites the elements it read, after the sums in stream order); any other overlap is the caller's error.
 * buses: NULL, or device [n_frames][G]: receives exactly what dspfx_mixgroups_run would have written, the same bits, and the
 * sums are paid for once.  Stream rules as dspfx_mixgroups_run; queued fader stores are drained once, ahead of the first
 * kernel, so the sums and the subtraction see the same table.  The first call allocates a [max_frames][G] f32 buffer for the
 * raw sums (a bank that never asks for returns keeps its footprint); if that fails: DSPFX_ERR_OOM, the reason in
 * dspfx_mixgroups_last_error, and a later call tries again.  NULL returns or block, n_frames of 0 or above max_frames:
 * DSPFX_ERR_INVALID before any device work. */
int dspfx_mixgroups_returns(dspfx_mixgroups *m, const float *block, uint32_t n_frames, float *buses, float *returns, void *stream);
/* Stores the faders of channels [first_channel, first_channel + count) from a host array; host_values = NULL drops them for
 * that range: back to "not multiplied".  Callable from any thread while runs are in flight, and never waits for the device or
 * for a run: the values are copied into a page-locked staging buffer and queued; the next run puts the queued stores on its
 * stream ahead of its kernels, in the order they were made.  So a run submitted after the call returns sees the new values,
 * and the runs submitted before it see the old ones. */
int dspfx_mixgroups_set_gains(dspfx_mixgroups *m, const float *host_values, uint64_t first_channel, uint64_t count);
/* PURE HOST function (no GPU, no bank): checks a table as create does (DSPFX_ERR_INVALID and the reason for a table that
 * decreases, does not start at 0 or end at n_channels, or a tile that is not a power of two dividing n_channels) and gives,
 * per group, depth_out[g] = D: the longest chain of dependent f32 additions in the group's sum (an upper bound that counts
 * every addition the kernels make on the path).  depth_out may be NULL. */
int dspfx_mixgroups_plan(const uint64_t *group_start, uint32_t n_groups, uint64_t n_channels, uint32_t tile_channels,
                         uint32_t *depth_out);
/* Seating: a room id per channel, reseated live.  A channel is a participant -- its biquad state, delay ring and FIR history
 * live at its index in the engine -- so a participant who changes rooms keeps the index and changes the id.  A bank has the G
 * rooms of its create table and every channel starts in the room its range puts it in; dspfx_mixgroups_assign moves channels
 * between those G rooms, or out of all of them (DSPFX_MIXGROUPS_NO_ROOM).  A bank on which assign is never called has no map
 * and launches the kernels above with the arguments above.  MAPPED MODE starts with the first assign, whatever it stores; from
 * then on a room that is still a contiguous range may differ from the unmapped bits, within the documented bound (the order
 * below is another one).
 * Arithmetic: dspfx_mixgroups_run and _returns as stated above with "group g" read as {c : room[c] == g} and n_g as its member
 * count: the same terms t[f][c], one IEEE division by dspfx_link_divisor(n_g) (normalise = 0: the raw sums), an empty room
 * gives +0.0, a return is fl32(fl32(S - t) / dspfx_link_divisor(n_g - 1)), +0.0 in a room of one; nothing is contracted.  A
 * channel carrying +inf gets NaN in its own return and +inf in the others', a NaN channel makes every return of its room NaN.
 * Faders belong to the channel and move with it.  An UNSEATED channel is in no sum and its return is +0.0 whatever it carries:
 * it is left out, not multiplied by zero, so its NaN or inf reaches no bus and no return.
 * Summation order: fixed, no atomics, and for one room a function of the room's MEMBER SET (and the layout) alone: the bus is
 * the same bits whatever the other channels' seating is, whatever the room's own id is, whatever sequence of assigns produced
 * the map, from run to run and on any stream.  Channels are cut into spans of 256 from channel 0.  A span whose 256 channels
 * are all the room's: as above, (x0 + x1) + (x2 + x3) per lane and the lane tree.  Any other span: the room's members in the
 * span, in ascending channel order, are summed by a Hillis-Steele scan over their RANKS (member r adds member r - step when
 * r >= step, steps 1, 2, .. 128): the tree is decided by how many members the span holds, not by where they sit.  The spans'
 * sums, in ascending span order, are added 64 at a time as above.  D, the longest chain of dependent additions, is at most
 * 8 + the reduce rounds' and stays under 64 + ceil(log2(max(n, 1))); dspfx_mixgroups_room_plan reports it per room, and the
 * error bounds of run and returns hold with this D.
 * Memory: a seating holds 10 bytes per channel of tables and its pieces, [pieces][max_frames rounded up to 64] f32 with
 * pieces = the sum over the spans of the rooms seated in the span: N / 256 for rooms that are whole spans, up to N -- one
 * block, [max_frames][N] f32 -- when every channel of a span sits in another room.  While runs given the old seating are in
 * flight, the old and the new one exist side by side. */
#define DSPFX_MIXGROUPS_NO_ROOM 0xFFFFFFFFu
/* Stores the room ids of channels [first_channel, first_channel + count) from a host array.  Every id (< G, or
 * DSPFX_MIXGROUPS_NO_ROOM) and the range are checked before anything is stored: otherwise DSPFX_ERR_INVALID, the reason in
 * dspfx_mixgroups_last_error, nothing changed.  It holds for every run submitted after it returns and for none submitted
 * before: blocks in flight keep the old seating.  Callable from any thread while runs are in flight, and the caller need not
 * idle the device: a seating change, not a per-block call -- O(N) host work, device memory for the new seating allocated on the
 * calling thread (DSPFX_ERR_OOM: the seating is unchanged, a later call may try again), and the call waits for its own table
 * copy, which travels on a stream of the bank's own. */
int dspfx_mixgroups_assign(dspfx_mixgroups *m, const uint32_t *host_room_ids, uint64_t first_channel, uint64_t count);
/* The room ids of channels [first_channel, first_channel + count) as the next run will see them (the create table's, on a bank
 * without a map). */
int dspfx_mixgroups_rooms(dspfx_mixgroups *m, uint32_t *host_ids_out, uint64_t first_channel, uint64_t count);
/* PURE HOST function (no GPU, no bank): checks a map room_of[n_channels] as assign does (an id that is neither < n_groups nor
 * DSPFX_MIXGROUPS_NO_ROOM, or a tile that is not a power of two dividing n_channels: DSPFX_ERR_INVALID and the reason) and
 * gives, per room, count_out[g] = n_g, depth_out[g] = D in mapped mode, and pieces_out[g] = the room's pieces (their sum is the
 * seating's piece count).  Each of the three may be NULL.  A room's D and pieces depend on its own members alone. */
int dspfx_mixgroups_room_plan(const uint32_t *room_of, uint64_t n_channels, uint32_t n_groups, uint32_t tile_channels,
                              uint64_t *count_out, uint32_t *depth_out, uint64_t *pieces_out);

/* ---- convolver bank: one long impulse response by partitioned FFT ----------------------------------------------
 * The FIR node takes any WAV file as its impulse response (nodes/fir.rs:86-173); the engine restates that arithmetic in the
 * direct form, which is the wrong algorithm for a room response of 24 000 to 144 000 taps.  This bank is the same node for N
 * channels and ONE response of T taps by uniformly partitioned overlap-save: per channel and 128-frame block
 *       y[n] = fl32(sum_{j<T} h[j] x[n - j]) * divisor          h[j] = taps_reversed[T - 1 - j]
 * taps arrive time-reversed in f64 exactly as dspfx_set_taps takes them (fir.rs:163,168); divisor is 1.0f for
 * DSPFX_FIR_BALANCED and 1.0f / (float)T for DSPFX_FIR_AVERAGE (fir.rs:187-190,222), one f32 multiplication after the sum.
 * The sum is NOT the reference's order of operations (no order is restated: the kernels use fmaf): it is a 256-point real FFT
 * of (previous block, this block) per block, kept in a ring of P_max spectra, Y[k] = sum_{p<P} H[p][k] X[head - p][k] over the
 * P = ceil(T / 128) partitions of the response, and the last 128 samples of the inverse FFT.  Relative RMS error against the
 * exact convolution is about 2e-7 at any length; the additions are in a fixed order that depends on P
 * alone (a partial sum per 16 consecutive partitions, the partials in ascending order; no atomics), so the output is the
 * same bits from run to run, on any stream, in either layout, and whatever the other channels carry.
 * History: starts as silence, and dspfx_convolve_reset returns to silence -- the reference node after T samples of silence.
 * The reference's FILL PHASE (while its deque is shorter than the taps it pairs the oldest held sample with taps[0]) is
 * deliberately NOT restated.  The ring holds input spectra, not products: dspfx_convolve_set_taps replaces the response and
 * keeps the history, which is the reference's reload behaviour.
 * A spectrum is 128 complex f32: bins 1..127, and element 0 = (DC, Nyquist), both real, which multiplies component-wise.
 * The response table H[p] = the 256-point FFT of taps h[128 p .. 128 p + 127], zero-padded, is computed on the host in f64 and
 * rounded once to f32 (dspfx_convolve_plan gives it exactly as the device gets it).
 * Memory: (P_max + 1) * 1024 * channels bytes of ring and accumulator plus 512 * channels of previous block -- under
 * (P_max + 2) * 1024 * channels bytes -- plus P_max * 1024 of table, P_max = ceil(max_taps / 128): 375 KiB per channel at
 * 48 000 taps, so a tool for G buses, not for 2^20 channels.  An allocation that fails is DSPFX_ERR_OOM, never an abort. */
typedef struct dspfx_convolve dspfx_convolve;
typedef struct dspfx_convolve_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t channels;        /* N */
    uint32_t tile_channels;   /* 0 = frame-major; W = channel-tiled, as dspfx_engine_desc */
    uint32_t n_taps;          /* T: 1 ..= DSPFX_CONVOLVE_MAX_TAPS */
    uint32_t max_taps;        /* ring slots are reserved for reloads of up to this many taps; 0 = n_taps */
    int32_t mode;             /* dspfx_fir_mode */
    const double *taps_reversed; /* host, [n_taps], read at create and copied; every tap finite */
} dspfx_convolve_desc;
/* The longest response the bank takes (10.9 s at 48 kHz, 4096 partitions). */
#define DSPFX_CONVOLVE_MAX_TAPS 524288
/* n_taps 0 or above DSPFX_CONVOLVE_MAX_TAPS, max_taps below n_taps or above the maximum, NULL or non-finite taps, an unknown
 * mode, no channels, a tile that is not a power of two dividing N, another ABI version: DSPFX_ERR_INVALID.  All of that is
 * checked before any device work. */
int dspfx_convolve_create(const dspfx_convolve_desc *desc, dspfx_convolve **out);
int dspfx_convolve_destroy(dspfx_convolve *p);
/* Back to silence; takes effect ahead of the next run, in that run's stream order.  The response stays. */
int dspfx_convolve_reset(dspfx_convolve *p);
/* in, out: device blocks of n_frames frames in the desc's layout (the tiled form for a block of n_frames); n_frames is a
 * multiple of 128 and is taken 128 frames at a time (anything else: DSPFX_ERR_INVALID before any device work).  out == in
 * works in place; any other overlap is the caller's error.  Asynchronous on `stream`; a run on another stream than the one
 * before first waits (on the device) for that one, since the history is the bank's (the rules of dspfx_mixgroups_run). */
int dspfx_convolve_run(dspfx_convolve *p, const float *in, float *out, uint32_t n_frames, void *stream);
/* Replaces the response (and the mode) and keeps the history; takes effect from the next run in stream order: the call waits
 * for the runs already submitted, which read the table in place -- a reload is a file load, not a per-block call.  More
 * than max_taps, or anything dspfx_convolve_create refuses in a response: DSPFX_ERR_INVALID, nothing changed. */
int dspfx_convolve_set_taps(dspfx_convolve *p, const double *taps_reversed, uint32_t n_taps, int mode);
/* PURE HOST function (no GPU, no bank): *partitions = P = ceil(n_taps / 128), and table_out (NULL, or room for
 * 128 * P * 2 floats) = the f32 response table exactly as the device gets it: element (k, p) at table_out[(k * P + p) * 2]
 * (re) and + 1 (im), k in [0, 128), with (DC, Nyquist) of partition p at k = 0.  The same rules for the taps as create. */
int dspfx_convolve_plan(const double *taps_reversed, uint32_t n_taps, uint32_t *partitions, float *table_out);
/* Several responses, one per channel.  A bank holds up to DSPFX_CONVOLVE_MAX_RESPONSES responses and a response id for every
 * channel: response 0 is the one given at create (the one dspfx_convolve_set_taps replaces) and every channel starts on it, so
 * a bank on which none of the calls below is made runs, launches and costs what it did without them.  The use is a small set
 * of halls shared by many buses -- this room a booth, that one a church -- not a table per channel.
 * Contract: channel c carrying id r gets THE SAME BITS as the same channel of a bank created with response r alone (its taps,
 * its mode) and fed the same input since the last reset -- in either layout, in place, 128 or 256 frames a call, after a reset,
 * and whatever ids and data its neighbours carry.  The partitions read for c are the response's own P_r = ceil(n_taps_r / 128)
 * (no padding to the longest response), so the order of additions stays a function of P_r alone and a NaN sample leaves the
 * channel after P_r + 1 blocks; the Average divisor is the response's own 1.0f / (float)n_taps_r.  The ring holds input
 * spectra, so pointing a channel at another response keeps its history: from the next run on its output is what a bank of the
 * new response alone would give on the same input history.  The ids are a uint16_t per channel (256 halls fit four times
 * over; the value is the cap on what one bank allocates).
 * Memory: each response beyond the first adds P_max * 1024 bytes of table (375 KiB at 48 000 taps, 94 MiB for 256 of them),
 * and the first one added 2 * channels + 4096 bytes of ids and per-response parameters. */
#define DSPFX_CONVOLVE_MAX_RESPONSES 256
/* Adds a response under dspfx_convolve_set_taps's rules (finite taps, 1 <= n_taps <= the bank's max_taps, a known mode) and
 * gives its id -- 1, 2, ... -- in *id_out (which may be NULL).  No channel carries it until dspfx_convolve_assign says so.
 * DSPFX_ERR_INVALID once the bank holds DSPFX_CONVOLVE_MAX_RESPONSES; DSPFX_ERR_OOM when the table cannot be allocated; either
 * way nothing changed.  Allocates on the calling thread and waits for the runs already submitted: a file load, not a
 * per-block call. */
int dspfx_convolve_response_add(dspfx_convolve *p, const double *taps_reversed, uint32_t n_taps, int mode, uint32_t *id_out);
/* Replaces response `id` (and its mode) and leaves the other responses, the ids and the history alone; id 0 is
 * dspfx_convolve_set_taps, the same operation.  An id the bank does not hold: DSPFX_ERR_INVALID, nothing changed. */
int dspfx_convolve_response_set(dspfx_convolve *p, uint32_t id, const double *taps_reversed, uint32_t n_taps, int mode);
/* Stores the ids of channels [first_channel, first_channel + count) from a host array.  An id at or above
 * dspfx_convolve_response_count, or a range past the bank's channels: DSPFX_ERR_INVALID and NOTHING is stored.  Serialised
 * with dspfx_convolve_run under the bank's lock: it holds for every run submitted after it returns and for none submitted
 * before (the copy travels in the order of the bank's last stream, and the call waits for it).  The history stays. */
int dspfx_convolve_assign(dspfx_convolve *p, const uint16_t *host_ids, uint64_t first_channel, uint64_t count);
/* The responses the bank holds (1 after create), or DSPFX_ERR_INVALID for a NULL bank. */
int dspfx_convolve_response_count(const dspfx_convolve *p);
/* In all four, the checks that need no device -- a NULL bank, NULL taps or ids, count == 0, the mode, the rules for the taps
 * -- come first and return DSPFX_ERR_INVALID with or without a GPU. */

/* ---- channel strips: per-channel Gain and BiQuad sliders ---------------------------------------------------------
 * An engine runs one chain for all its channels with ONE set of slider values.  In the reference every graph has its own node
 * instances and its own Atomic<f32> sliders (gain.rs:21-22, biquad.rs:18-41): N channels are N independent sets of settings.
 * This bank is that for the two node kinds where a participant's own settings matter most -- an input trim and a high-pass or
 * EQ ahead of the room.  It sits between the N-channel chain and dspfx_mixgroups_run / _returns, or ahead of the chain.
 * The strip of channel c is a chain of up to 1 + K optional nodes in a fixed order:
 *       a Gain node                 out = in * level[c]                                           gain.rs:25-38
 *       BiQuad bands 0 .. K-1       y = b0*x + b1*x1 + b2*x2 - a1*y1 - a2*y2, then the DF1 shift  biquad.rs:62-88
 * A node EXISTS for a channel from the first store that names it until it is dropped; a fresh bank has no node anywhere and
 * run copies in to out bit for bit.  A channel's output is what the reference gives a graph made of exactly that channel's
 * present nodes with that channel's slider values.  The level is taken as given, as a restored config's is (no clamp to the
 * slider range 0..=10).  The biquad step is evaluated left to right in f32 with nothing contracted -- the engine's BIQUAD
 * expression -- on four f32 of state per band and channel (x1, x2, y1, y2), kept between runs, zero after create and reset.
 * link_flags has the meaning of dspfx_engine_desc.link_flags: DSPFX_LINK_INPUT puts one collect_and_average hop,
 * (0.0f + v) / f32(0.0001 + 1.0) (node.rs:162-194, an IEEE division), ahead of a channel's first present node,
 * DSPFX_LINK_INTERNAL one between consecutive present nodes; a channel without a node gets no hop.
 * A channel's output is the same bits in either layout, in place or not, in one call of 256 frames or two of 128, on any
 * stream, and whatever its neighbours carry (a NaN channel changes no other channel). */
#define DSPFX_STRIPS_MAX_BANDS 8
typedef struct dspfx_strips dspfx_strips;
typedef struct dspfx_strips_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t n_channels;      /* N */
    uint32_t max_frames;      /* largest n_frames a run will pass (>= 1) */
    uint32_t tile_channels;   /* 0 = frame-major; W = channel-tiled, as dspfx_engine_desc */
    uint32_t bands;           /* K: 1 ..= DSPFX_STRIPS_MAX_BANDS */
    uint32_t link_flags;      /* DSPFX_LINK_INTERNAL | DSPFX_LINK_INPUT; any other bit: DSPFX_ERR_INVALID */
} dspfx_strips_desc;
/* A bad descriptor is DSPFX_ERR_INVALID with the reason in dspfx_strips_last_error of a NULL bank (kept per thread); all of
 * that is checked before any device work.  Memory: (9 K' + 2) * 4 bytes per channel, K' = K rounded up to 1, 2, 4 or 8. */
int dspfx_strips_create(const dspfx_strips_desc *desc, dspfx_strips **out);
int dspfx_strips_destroy(dspfx_strips *s);
/* The reason of the bank's last failed call; of a NULL bank: of this thread's last failed create. */
const char *dspfx_strips_last_error(const dspfx_strips *s);
/* in, out: device blocks of n_frames frames in the desc's layout (1 <= n_frames <= max_frames).  out == in works in place
 * (a thread rewrites the elements it read); any other overlap is the caller's error.  Asynchronous on `stream`; a run on
 * another stream than the one before first waits (on the device) for that one, since the state is the bank's (the rules of
 * dspfx_mixgroups_run).  Queued slider stores go onto the stream ahead of the kernel, in the order they were made. */
int dspfx_strips_run(dspfx_strips *s, const float *in, float *out, uint32_t n_frames, void *stream);
/* Stores the Gain level of channels [first_channel, first_channel + count) from a host array; host_levels = NULL removes the
 * Gain node for that range.  The contract of dspfx_mixgroups_set_gains: callable from any thread while runs are in flight,
 * never waits for the device or for a run; the values are copied into a page-locked staging buffer and queued, and the next
 * run applies the queued stores in order: a run submitted after the call returns sees the new values, the runs submitted
 * before it the old ones.  A range past the bank's channels stores nothing: DSPFX_ERR_INVALID, the reason in
 * dspfx_strips_last_error. */
int dspfx_strips_set_gain(dspfx_strips *s, const float *host_levels, uint64_t first_channel, uint64_t count);
/* Stores band `band` of channels [first_channel, first_channel + count): host_raw6 is [count][6] raw sliders in the reference's
 * field order a0, a1, a2, b0, b1, b2 (biquad.rs:18-41).  The host normalises as regenerate_filter does (biquad.rs:66-70: five
 * f32 divisions by a0; a0 = 0 gives the infinities or NaNs the reference would get, no check is made), and the store zeroes
 * the four state values of exactly the stored channels' band (reset_state, biquad.rs:74) and touches nothing else: the
 * reference's after_settings_change.  host_raw6 = NULL removes the band for the range; a later store starts it from zero
 * state.  Threading and ordering as dspfx_strips_set_gain.  band >= K or a range past the channels: DSPFX_ERR_INVALID and the
 * reason, nothing stored. */
int dspfx_strips_set_band(dspfx_strips *s, uint32_t band, const float *host_raw6, uint64_t first_channel, uint64_t count);
/* Zeroes all state and keeps the sliders and the nodes; queued on the stream last used. */
int dspfx_strips_reset(dspfx_strips *s);
/* The node mask of channels [first_channel, first_channel + count) as the next run will see it: bit 0 = the Gain node,
 * bit 1 + b = band b. */
int dspfx_strips_present(dspfx_strips *s, uint32_t *host_masks_out, uint64_t first_channel, uint64_t count);
/* PURE HOST function (no GPU, no bank): out5 = a1, a2, b0, b1, b2, the five normalised coefficients of the raw sliders raw6
 * exactly as the device gets them. */
int dspfx_strips_coeffs(const float *raw6, float *out5);

/* ---- channel delays: per-channel Reverb (feedback delay) sliders ---------------------------------------------------
 * An engine runs one Reverb(seconds, decay) for all its channels.  In the reference every graph owns its Reverb node with its
 * own `seconds` and `decay` sliders and its own ring (nodes/reverb.rs:29-41).  This bank is that: channel c may carry one Reverb
 * node with its own ring of D_c frames.  It goes where the channel strips go, between the N-channel chain and the room mixes.
 * A node EXISTS for a channel from the first store that names it until it is dropped; a fresh bank has no node anywhere and run
 * copies in to out bit for bit.  Per channel the bank keeps D_c, decay_c, seconds_c, a ring position and the count of frames
 * whose tap still reads as zero.
 * A store to a channel is the reference's slider change: ANY slider of the node, decay included, fires refresh_seconds
 * (reverb.rs:19, 55-71), so the channel gets a NEW ZERO ring of D_c = dspfx_delay_len(seconds_c, page_round) frames at position 0
 * and every echo in the old one is gone.  The values are taken as given: no clamp, NaN seconds is 128 frames as dspfx_delay_len says.
 * One run of n_frames, per channel that carries a node (reverb.rs:76-110):
 *       n_frames <= D_c    for i in order   tap = ring[(pos + i) % D_c]  (+0.0f while the new ring is still zeros)
 *                                           out[i] = in[i] + tap * decay_c     one f32 multiply, one f32 add, nothing contracted
 *                                           ring[(pos + i) % D_c] = out[i]
 *                          then pos = (pos + n_frames) % D_c.  The arithmetic is done on the zero taps too: -0.0 + (+0.0 * -1.0) and
 *                          +0.0 * inf come out as the reference gives them.
 *       n_frames > D_c     out = in, ring and position untouched: "Reverb buffer is empty", reverb.rs:92-96 (only with
 *                          max_frames above 128)
 * link_flags has the meaning of dspfx_engine_desc.link_flags: DSPFX_LINK_INPUT puts one collect_and_average hop,
 * (0.0f + v) / f32(0.0001 + 1.0) (node.rs:162-194, an IEEE division), ahead of the node on the channels that carry one (in
 * either branch above); DSPFX_LINK_INTERNAL has nothing to act on.
 * Memory: cap = dspfx_delay_len(max_seconds, page_round) frames of ring per channel, n_channels * cap * 4 bytes, allocated by
 * create and NEVER zeroed: a store says that the channel's next D_c taps read as +0.0, so it costs one small kernel over the
 * stored channels, never a memset.  Plus 16 bytes of tables per channel.
 * A channel's output is the same bits in either layout, in place or not, on any stream, and whatever its neighbours carry. */
typedef struct dspfx_delays dspfx_delays;
typedef struct dspfx_delays_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t n_channels;      /* N */
    uint32_t max_frames;      /* largest n_frames a run will pass (>= 1) */
    uint32_t tile_channels;   /* 0 = frame-major; W = channel-tiled, as dspfx_engine_desc */
    float max_seconds;        /* the longest delay a store may ask for: cap = dspfx_delay_len(max_seconds, page_round) */
    uint32_t page_round;      /* 0 / 1: the reading of seconds -> frames, as dspfx_delay_len's */
    uint32_t link_flags;      /* DSPFX_LINK_INTERNAL | DSPFX_LINK_INPUT; any other bit: DSPFX_ERR_INVALID */
} dspfx_delays_desc;
/* PURE HOST function (no GPU, no bank): the ring frames per channel and the ring bytes of a bank of `channels` channels.
 * channels of 0 or above 2^32 - 256, or a cap above 2^31 frames: DSPFX_ERR_INVALID, the reason in dspfx_delays_last_error(NULL). */
int dspfx_delays_plan(uint64_t channels, float max_seconds, int page_round, uint32_t *cap_out, uint64_t *bytes_out);
/* A bad descriptor (what dspfx_delays_plan refuses, a tile that is not a power of two dividing n_channels, an unknown link flag,
 * another ABI version, max_frames of 0) is DSPFX_ERR_INVALID with the reason in dspfx_delays_last_error of a NULL bank (kept per
 * thread); all of that is checked before any device work.  Rings that do not fit the device: DSPFX_ERR_OOM and the reason. */
int dspfx_delays_create(const dspfx_delays_desc *desc, dspfx_delays **out);
int dspfx_delays_destroy(dspfx_delays *d);
/* The reason of the bank's last failed call; of a NULL bank: of this thread's last failed create or plan. */
const char *dspfx_delays_last_error(const dspfx_delays *d);
/* in, out: device blocks of n_frames frames in the desc's layout (1 <= n_frames <= max_frames).  out == in works in place
 * (a thread rewrites the elements it read); any other overlap is the caller's error.  Asynchronous on `stream`; a run on
 * another stream than the one before first waits (on the device) for that one, since the rings are the bank's (the rules of
 * dspfx_strips_run).  Queued slider stores go onto the stream ahead of the kernel, in the order they were made. */
int dspfx_delays_run(dspfx_delays *d, const float *in, float *out, uint32_t n_frames, void *stream);
/* Stores the sliders of channels [first_channel, first_channel + count) from host arrays of `count` values each.  host_seconds
 * or host_decay may be NULL: that slider keeps each channel's value (0.5 for a channel never stored, or dropped since: the
 * reference's defaults, reverb.rs:29-38), and the store still gives every channel of the range its new zero ring.  BOTH NULL
 * removes the node for the range; a later store starts from a zero ring.  A store that needs D_c > cap on any of its channels,
 * or whose range lies outside the bank's channels, is refused WHOLE: DSPFX_ERR_INVALID, the reason in dspfx_delays_last_error,
 * nothing changed.  The contract of dspfx_strips_set_gain otherwise: callable from any thread while runs are in flight, never
 * waits for the device or for a run; the values are staged in page-locked memory and queued, and a run submitted after the call
 * returns sees the store, whole, the runs submitted before it do not. */
int dspfx_delays_set_delay(dspfx_delays *d, const float *host_seconds, const float *host_decay, uint64_t first_channel, uint64_t count);
/* Every present channel's ring back to zeros at position 0; the sliders and the nodes stay.  Queued on the stream last used. */
int dspfx_delays_reset(dspfx_delays *d);
/* 1 / 0 per channel of [first_channel, first_channel + count): it carries a node, as all stores made so far left it (host tables). */
int dspfx_delays_present(dspfx_delays *d, uint32_t *host_present_out, uint64_t first_channel, uint64_t count);
/* D_c per channel of the range, 0 where there is no node, from the same host tables. */
int dspfx_delays_lengths(dspfx_delays *d, uint32_t *host_lengths_out, uint64_t first_channel, uint64_t count);

/* ---- talker bank: per-channel levels and each room's K loudest, gated live ------------------------------------------
 * An engine's Envelope node (nodes/envelope.rs, a peak follower) has one (attack, release) pair for all N channels and replaces
 * the signal with its envelope.  In the reference every graph owns its Envelope node and feeds slider ports from it: an Envelope
 * into a Gain.  At the scale of a room that is a gate driven by the room's ranking.  This bank is both halves over N channels in
 * the desc's layout (tile_channels as dspfx_engine_desc): every channel has its own Envelope node, every room gets its `top`
 * loudest members chosen on the device, and a gate passes those members and ramps the others out, so dspfx_mixgroups_run /
 * _returns and dspfx_mixmatrix_run downstream add only the talkers.  It sits behind the channel strips and delays, ahead of the
 * room mixes.
 * ROOMS.  Create takes contiguous rooms as dspfx_mixgroups_create does (group_start, G + 1 indices), each of 1 ..
 * DSPFX_TALKERS_MAX_ROOM members; dspfx_talkers_assign moves channels as dspfx_mixgroups_assign does.  The host keeps room_of[N];
 * the device gets a member list sorted by (room, channel) and room_start[G + 1], so a seating is a function of room_of alone, not
 * of the calls that led to it, and the selection does not care how scattered a room's members are.
 * PER CHANNEL.  State: env (f32, starts +0.0), gate and target (f32, start 1.0).  Sliders: attack and release in frames, taken
 * as given (no clamp), 0 and 0 by default as the node's; the host converts them with dspfx_envelope_gain.  A pin, one uint8_t:
 * DSPFX_TALKERS_AUTO (the default), DSPFX_TALKERS_OPEN (always passed, never ranked, takes no slot) or DSPFX_TALKERS_SHUT (never
 * passed, never ranked).
 * PER ROOM: top, 1 .. DSPFX_TALKERS_MAX_TOP, the desc's value until dspfx_talkers_set_top stores another.  BANK-WIDE: floor, f32,
 * 0.0 by default.
 * ONE RUN does three things, in this order.
 *   1. Queued stores go onto the stream, in the order they were made.
 *   2. Pass A, per channel, frames in order.  The envelope as the engine's Envelope node computes it:
 *            d = x < 0 ? -x : x        gain = env < d ? ga : gr        env = d + (env + (-d)) * gain       nothing contracted
 *      so env after every frame is what the reference's node writes, bit for bit (a NaN where it has a NaN).  level[c] starts at
 *      +0.0 and takes each frame's env whenever env > level: the block's largest env.  A NaN or a -0.0 envelope never raises it, so
 *      a level is always a non-negative, non-NaN f32.  With out not NULL:
 *            out[f][c] = in[f][c] * (gate + (target - gate) * r[f])            r[f] = f32(f + 1) / f32(n_frames)
 *      one IEEE division, one f32 subtraction, multiply and add for the ramp, one multiply for the sample, nothing contracted.
 *      With gate and target in {0, 1}: exactly 1.0; exactly +0.0; a ramp up; a ramp down; the last frame is exactly at the
 *      target.  These are multiplications, not omissions: a NaN sample in a closed channel stays a NaN (as dspfx_mixmatrix_run
 *      documents for unwired entries).  After the block gate = target.  out == in works in place.  out == NULL meters and selects
 *      only: no sample is written and gate stays as it is.
 *   3. Pass B, per room, with the tables as of this run.  The candidates are the members with pin AUTO and level > floor,
 *      strictly; ranked by level descending, then channel number ascending; the first min(top_r, candidates) are the room's
 *      talkers.  It writes talkers[G][8] (int32_t channel numbers, -1 where there is none), talker_levels[G][8] (f32, +0.0 where
 *      there is none) and target[c] for EVERY channel: 1.0 for a talker and for an OPEN pin (in a room or not), +0.0 for everybody
 *      else, SHUT pins and AUTO channels in no room included.
 * So a selection is audible in the run after the one that measured it, and a store governs the selection at the end of the first
 * run submitted after it: one rule and no second read of the block, at the cost of at most one block plus the one-block ramp
 * before a new talker is fully open.  A fresh bank passes its first block bit for bit: every gate is at 1.0.
 * A channel's output and a room's tables are the same bits in either layout, in place or not, on any stream, and whatever the
 * other rooms carry.  No atomics; every step in a fixed order.
 * Memory: 29 bytes per channel and 69 per room of tables on the device (dspfx_talkers_plan), 12 per channel on the host. */
#define DSPFX_TALKERS_MAX_ROOM 1024
#define DSPFX_TALKERS_MAX_TOP 8
#define DSPFX_TALKERS_AUTO 0
#define DSPFX_TALKERS_OPEN 1
#define DSPFX_TALKERS_SHUT 2
/* dspfx_talkers_assign, dspfx_talkers_select: the channel sits in no room */
#define DSPFX_TALKERS_NO_ROOM 0xFFFFFFFFu
typedef struct dspfx_talkers dspfx_talkers;
typedef struct dspfx_talkers_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t n_channels;      /* N */
    uint32_t max_frames;      /* largest n_frames a run will pass (>= 1) */
    uint32_t tile_channels;   /* 0 = frame-major; W = channel-tiled, as dspfx_engine_desc */
    uint32_t n_groups;        /* G >= 1 rooms */
    uint32_t top;             /* every room's top until dspfx_talkers_set_top: 1 ..= DSPFX_TALKERS_MAX_TOP */
    const uint64_t *group_start; /* host, [n_groups + 1], read at create and copied: room g is channels [group_start[g],
                                 group_start[g + 1]); increasing, [0] = 0, [G] = N; every room has 1 .. 1024 members */
} dspfx_talkers_desc;
/* PURE HOST function (no GPU, no bank): frames -> the gain the detector multiplies by, frames == 0 ? 0 : powf(e, -1 / frames)
 * (dasp_envelope's calc_gain, with the host's libm as the reference calls it): what dspfx_talkers_set_detector stores and what
 * dspfx_chain_set computes for an Envelope node. */
float dspfx_envelope_gain(float frames);
/* PURE HOST function: *bytes_out = the device bytes of a bank's tables, 29 * channels + 69 * n_groups + 4.  channels of 0 or above
 * 2^32 - 256, or no rooms: DSPFX_ERR_INVALID, the reason in dspfx_talkers_last_error(NULL).  A bank that asks for its audible list
 * (dspfx_talkers_audible_views) holds 4 * channels + 4 * n_groups more, which this figure leaves out. */
int dspfx_talkers_plan(uint64_t channels, uint32_t n_groups, uint64_t *bytes_out);
/* PURE HOST function: pass B's rule on host arrays.  levels[n_channels] (as the bank leaves them: non-negative, no NaN),
 * room_of[n_channels] (each below n_groups, or DSPFX_TALKERS_NO_ROOM), top[n_groups] (1 .. 8 each), pins[n_channels] or NULL for
 * all AUTO -> talkers_out[n_groups][8], levels_out[n_groups][8], target_out[n_channels]; each of the three may be NULL.  A bad
 * id, a bad top, or a room above DSPFX_TALKERS_MAX_ROOM: DSPFX_ERR_INVALID, the reason in dspfx_talkers_last_error(NULL). */
int dspfx_talkers_select(const float *levels, const uint32_t *room_of, uint64_t n_channels, uint32_t n_groups, const uint8_t *top, float floor,
                         const uint8_t *pins, int32_t *talkers_out, float *levels_out, float *target_out);
/* A bad descriptor (a table that decreases, does not start at 0 or end at n_channels, an empty room or one above
 * DSPFX_TALKERS_MAX_ROOM, a top of 0 or above DSPFX_TALKERS_MAX_TOP, a tile that is not a power of two dividing n_channels, another
 * ABI version, max_frames of 0) is DSPFX_ERR_INVALID with the reason in dspfx_talkers_last_error of a NULL bank (kept per thread);
 * all of that is checked before any device work. */
int dspfx_talkers_create(const dspfx_talkers_desc *desc, dspfx_talkers **out);
int dspfx_talkers_destroy(dspfx_talkers *t);
/* The reason of the bank's last failed call; of a NULL bank: of this thread's last failed create, plan or select. */
const char *dspfx_talkers_last_error(const dspfx_talkers *t);
/* in, out: device blocks of n_frames frames in the desc's layout (1 <= n_frames <= max_frames); out may be in, or NULL (meter and
 * select only); any other overlap is the caller's error.  Asynchronous on `stream`; a run on another stream than the one before
 * first waits (on the device) for that one, since the state is the bank's (the rules of dspfx_strips_run). */
int dspfx_talkers_run(dspfx_talkers *t, const float *in, float *out, uint32_t n_frames, void *stream);
/* Seats channels [first_channel, first_channel + count) in the rooms host_room_ids (each below n_groups, or
 * DSPFX_TALKERS_NO_ROOM).  The range, every id and every room's size after the call (at most DSPFX_TALKERS_MAX_ROOM) are checked
 * before anything is stored: otherwise DSPFX_ERR_INVALID, the reason in dspfx_talkers_last_error, nothing changed.  Callable from
 * any thread while runs are in flight, never waits for the device or for a run, and holds, whole, for every run submitted after it
 * returns and for none submitted before.  A seating change, not a per-block call: O(N + G) host work and a staged copy of the
 * member list.  A channel's envelope, gate and pin stay with the channel. */
int dspfx_talkers_assign(dspfx_talkers *t, const uint32_t *host_room_ids, uint64_t first_channel, uint64_t count);
/* Stores the attack and release sliders (frames) of channels [first_channel, first_channel + count) from host arrays of `count`
 * values each; either may be NULL, which keeps each channel's value.  The store touches no envelope: the reference's slider
 * change sets only the gain.  The contract of dspfx_strips_set_gain: any thread, never waits, staged and queued, whole for the runs
 * submitted after it returns.  A range past the channels: DSPFX_ERR_INVALID and the reason, nothing stored. */
int dspfx_talkers_set_detector(dspfx_talkers *t, const float *host_attack, const float *host_release, uint64_t first_channel, uint64_t count);
/* Stores the pins of channels [first_channel, first_channel + count); a value above DSPFX_TALKERS_SHUT or a range past the
 * channels: DSPFX_ERR_INVALID and the reason, nothing stored.  Threading and ordering as dspfx_talkers_set_detector. */
int dspfx_talkers_set_pin(dspfx_talkers *t, const uint8_t *host_pins, uint64_t first_channel, uint64_t count);
/* Stores the top of rooms [first_room, first_room + count); a value of 0 or above DSPFX_TALKERS_MAX_TOP, or a range past the
 * rooms: DSPFX_ERR_INVALID and the reason, nothing stored.  Threading and ordering as dspfx_talkers_set_detector. */
int dspfx_talkers_set_top(dspfx_talkers *t, const uint8_t *host_tops, uint64_t first_room, uint64_t count);
/* Stores the floor (taken as given; under a NaN floor nobody is a candidate).  Queued like the other stores. */
int dspfx_talkers_set_floor(dspfx_talkers *t, float floor);
/* env and level back to +0.0, gate and target to 1.0 on channels [first_channel, first_channel + count); the sliders, pins and
 * seats stay.  Queued like a store.  Also the way out for a channel whose envelope became NaN and, as in the reference, stays
 * NaN. */
int dspfx_talkers_reset(dspfx_talkers *t, uint64_t first_channel, uint64_t count);
/* The device pointers of level[N], target[N], talkers[G][8] and talker_levels[G][8] (each out pointer may be NULL).  The pointers
 * never change; what they hold is valid after a run, on its stream. */
int dspfx_talkers_views(dspfx_talkers *t, const float **level_out, const float **target_out, const int32_t **talkers_out,
                        const float **talker_levels_out);
/* The room ids of channels [first_channel, first_channel + count), and every room's member count ([n_groups]), by every assign made
 * so far (host tables). */
int dspfx_talkers_room_of(dspfx_talkers *t, uint32_t *host_ids_out, uint64_t first_channel, uint64_t count);
int dspfx_talkers_counts(dspfx_talkers *t, uint32_t *host_counts_out);
/* ---- the audible list: which members of each room can be non-zero in the block a run has just gated -------------------------
 * talkers[G][8] is not that list: the gate ramps over one block, so in the block after a talker change the members fading out
 * are still non-zero, and OPEN pins pass without taking a talker slot (a fresh or reset bank passes everybody).
 * THE RULE.  A channel is AUDIBLE in a gated run iff its gate or its target, as the run finds them after the queued stores have
 * been applied, is not +-0.0.  These are exactly the channels whose factor gate + (target - gate) * r[f] can be non-zero; every
 * other channel's gated sample is x * 0, exactly zero for finite input.  From the third gated block after a fresh state a room
 * lists at most 2 * top_r members (those fading in or held, those fading out) plus its OPEN pins.
 * PURE HOST function: the rule on host arrays.  gate[n_channels], target[n_channels], room_of[n_channels] (each below n_groups, or
 * DSPFX_TALKERS_NO_ROOM) -> start_out[n_groups + 1], the members' prefix table (room r has start[r + 1] - start[r] members: the
 * room_start a bank makes from room_of); list_out[n_channels]: room r's audible members, in ascending channel order, are
 * list_out[start[r] .. start[r] + count[r]), the entries of a segment past count[r] and the entries past start[n_groups] are
 * unspecified; count_out[n_groups].  A bad id, a room above DSPFX_TALKERS_MAX_ROOM, more than 2^31 - 1 channels or a NULL pointer:
 * DSPFX_ERR_INVALID, the reason in dspfx_talkers_last_error(NULL). */
int dspfx_talkers_audible(const float *gate, const float *target, const uint32_t *room_of, uint64_t n_channels, uint32_t n_groups,
                          int32_t *list_out, uint32_t *start_out, uint32_t *count_out);
/* The device form.  The first call allocates list[N] (int32_t) and count[G] (4 bytes per channel and 4 per room beside
 * dspfx_talkers_plan's figure; DSPFX_ERR_OOM if that fails, DSPFX_ERR_INVALID on a bank above 2^31 - 1 channels) and switches the
 * bank on: every GATED run submitted after it launches one more kernel, talkers_audible, behind the drained stores and ahead of
 * pass A (which overwrites gate): one wave per room gathers gate and target through the member list and compacts by ballot, in
 * member order.  No atomics.  A metering run (out == NULL) gates nothing and leaves the tables as they were.  -> the device
 * pointers of list, start (the bank's own room_start[G + 1], which dspfx_talkers_assign rewrites in stream order) and count; each
 * out pointer may be NULL.  The pointers are stable for the life of the bank; what they hold is valid after a gated run, on its
 * stream (before the first one: nobody is listed).  A bank that never calls this launches what it always launched.  The list is
 * what dspfx_mixmatrix_run_sparse takes. */
int dspfx_talkers_audible_views(dspfx_talkers *t, const int32_t **list_out, const uint32_t **start_out, const uint32_t **count_out);

/* ---- channel dynamics: a bank of per-channel levellers and limiters --------------------------------------------------
 * The talker bank uses the reference's "an Envelope into a Gain" as a gate.  This bank is the ordinary use, where the envelope
 * turns the gain DOWN: channel c may carry its own Envelope node (nodes/envelope.rs) feeding its own gain computer, over N
 * channels in the desc's layout (tile_channels as dspfx_engine_desc).  One bank object serves two places of the room pipeline: a
 * LEVELLER ahead of dspfx_talkers_run, so that the ranking is not by microphone gain, and a LIMITER behind the room mixes, ahead of
 * the resampler and the PCM conversion, which hard-clip.
 * A node EXISTS for a channel from the first dspfx_dynamics_set that names it until dspfx_dynamics_drop; a fresh bank has no node
 * anywhere and run copies in to out bit for bit.
 * PER CHANNEL.  State: env (f32, starts +0.0).  Sliders: attack and release in frames, taken as given (no clamp) and converted on
 * the host by dspfx_envelope_gain into ga and gr; threshold thr and makeup mk.  A slider the first store leaves out starts at 0,
 * 0, 1.0 and 1.0.
 * ONE RUN: queued stores go onto the stream in the order they were made, then per channel that carries a node, frames in order,
 * nothing contracted:
 *       k   = key ? key[f][c] : in[f][c]
 *       d   = k < 0 ? -k : k
 *       g   = env < d ? ga : gr
 *       env = d + (env + (-d)) * g                 the engine's Envelope node, bit for bit (a NaN where it has a NaN)
 *       q   = env > thr ? thr / env : 1.0f         one IEEE f32 division
 *       out[f][c] = in[f][c] * (mk * q)            two f32 multiplications
 *       level[c]     = env > level ? env : level   starts +0.0 every run: never NaN, never negative
 *       reduction[c] = q < reduction ? q : reduction     starts 1.0 every run
 * One curve covers both uses.  A limiter is mk = 1, thr = the ceiling, attack 0.  A leveller that brings everybody towards
 * `target` with a gain of at most `max_gain` is thr = target / max_gain, mk = max_gain.  A ratio or a knee needs powf on the
 * device, whose bits nothing pins: there is none.
 * WHAT FOLLOWS.
 *   - A channel without a node is copied bit for bit; its level is +0.0 and its reduction 1.0.
 *   - A channel that never exceeds its threshold gets in * (mk * 1.0f): the bits of the engine's Gain(mk) node; with mk = 1 a copy.
 *   - The gain is a multiplication, not an omission: a NaN sample stays a NaN.
 *   - A NaN envelope compares false, so q = 1; as in the reference it stays NaN until dspfx_dynamics_reset.
 *   - BRICK WALL: with attack 0 (ga = 0), no key, finite input, release >= 0 and thr * mk in the normal range, env >= |in| on every
 *     frame (env is |in| exactly when it rises, and a release step rounds a value between |in| and the old env, monotonically),
 *     so |out| <= thr * mk * (1 + 2^-24)^3: three roundings, the division and the two multiplications.  On a numpy model over noise
 *     of amplitude 1e-3 .. 4, thresholds 0.001 .. 1, makeups 0.7 .. 3 and releases 0 .. 24000 the worst excess over thr * mk was
 *     1.95 x 2^-24.  With attack ABOVE 0 there is NO such bound: the envelope lags the signal, and the model overshoots 4-fold on
 *     the first samples at attack 48.  With a key there is none either: the envelope is the key's.
 * THE KEY.  key, a block of the same shape, is what the detector follows while the gain is applied to in: the reference's Envelope
 * of one signal into the Gain slider of another, turned downward (music ducked under an announcer; a detector ahead of an EQ).
 * key == in gives the bits of no key (and is run as no key); key == NULL is no key.
 * A channel's output and tables are the same bits in either layout, in place or not, on any stream, and whatever its neighbours
 * carry.  No atomics, no LDS.
 * Memory: 29 bytes per channel of tables on the device (ga, gr, thr, mk, env, level, reduction and the presence byte;
 * dspfx_dynamics_plan), 17 per channel on the host. */
typedef struct dspfx_dynamics dspfx_dynamics;
typedef struct dspfx_dynamics_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t n_channels;      /* N */
    uint32_t max_frames;      /* largest n_frames a run will pass (>= 1) */
    uint32_t tile_channels;   /* 0 = frame-major; W = channel-tiled, as dspfx_engine_desc */
} dspfx_dynamics_desc;
/* PURE HOST function (no GPU, no bank): *bytes_out = the device bytes of a bank's tables, 29 * channels.  channels of 0 or above
 * 2^32 - 256: DSPFX_ERR_INVALID, the reason in dspfx_dynamics_last_error(NULL). */
int dspfx_dynamics_plan(uint64_t channels, uint64_t *bytes_out);
/* PURE HOST function: the gain computer's rule on one envelope value.  q = env > threshold ? threshold / env : 1.0f goes to *q_out
 * (which may be NULL) and makeup * q is returned: the factor the device multiplies the sample by, bit for bit.  No check is made. */
float dspfx_dynamics_gain(float env, float threshold, float makeup, float *q_out);
/* A bad descriptor (channels of 0 or above 2^32 - 256, a tile that is not a power of two dividing n_channels, another ABI version,
 * max_frames of 0) is DSPFX_ERR_INVALID with the reason in dspfx_dynamics_last_error of a NULL bank (kept per thread); all of that
 * is checked before any device work. */
int dspfx_dynamics_create(const dspfx_dynamics_desc *desc, dspfx_dynamics **out);
int dspfx_dynamics_destroy(dspfx_dynamics *d);
/* The reason of the bank's last failed call; of a NULL bank: of this thread's last failed create or plan. */
const char *dspfx_dynamics_last_error(const dspfx_dynamics *d);
/* in, key, out: device blocks of n_frames frames in the desc's layout (1 <= n_frames <= max_frames); key may be NULL.  out == in
 * works in place, with or without a key (a thread rewrites the elements it read); key overlapping out while key != in, and any
 * other overlap, is the caller's error.  Asynchronous on `stream`; a run on another stream than the one before first waits (on the
 * device) for that one, since the state is the bank's (the rules of dspfx_strips_run).  Queued stores go onto the stream ahead of
 * the kernel, in the order they were made. */
int dspfx_dynamics_run(dspfx_dynamics *d, const float *in, const float *key, float *out, uint32_t n_frames, void *stream);
/* Stores the sliders of channels [first_channel, first_channel + count) from host arrays of `count` values each, and gives every
 * channel of the range its node.  Any of the four may be NULL, which keeps each channel's value (the defaults for a channel never
 * stored, or dropped since); all four NULL only makes the nodes.  The store touches no envelope: the reference's slider change sets
 * only the gain.  Refused WHOLE, DSPFX_ERR_INVALID with the reason in dspfx_dynamics_last_error and nothing stored: a threshold
 * that is NaN or below +0.0 (-0.0 included: it would turn the sign of every sample above it), a makeup that is NaN, infinite or
 * negative (-0.0 included), a range past the channels.  A threshold of +infinity is a channel that is never turned down.  The
 * contract of dspfx_strips_set_gain otherwise: callable from any thread while runs are in flight, never waits for the device or for
 * a run; the values are staged in page-locked memory and queued, and a run submitted after the call returns sees the store, whole,
 * the runs submitted before it do not. */
int dspfx_dynamics_set(dspfx_dynamics *d, const float *host_threshold, const float *host_makeup, const float *host_attack,
                       const float *host_release, uint64_t first_channel, uint64_t count);
/* Removes the node of channels [first_channel, first_channel + count) and clears their envelope; a later store starts from the
 * default sliders and a zero envelope.  Queued like a store.  A range past the channels: DSPFX_ERR_INVALID and the reason. */
int dspfx_dynamics_drop(dspfx_dynamics *d, uint64_t first_channel, uint64_t count);
/* env and level back to +0.0 and reduction to 1.0 on the range; the sliders and the nodes stay.  Queued like a store.  Also the way
 * out for a channel whose envelope became NaN. */
int dspfx_dynamics_reset(dspfx_dynamics *d, uint64_t first_channel, uint64_t count);
/* 1 / 0 per channel of [first_channel, first_channel + count): it carries a node, as all stores made so far left it (host tables). */
int dspfx_dynamics_present(dspfx_dynamics *d, uint32_t *host_present_out, uint64_t first_channel, uint64_t count);
/* The device pointers of level[N] and reduction[N] (each out pointer may be NULL).  The pointers never change; what they hold is
 * valid after a run, on its stream. */
int dspfx_dynamics_views(dspfx_dynamics *d, const float **level_out, const float **reduction_out);

/* ---- channel shapers: a bank of per-channel Distort, Overdrive and Chebyshev -----------------------------------------
 * An engine runs one chain with one set of slider values for all N channels; in the reference every graph owns its own node
 * instances, sliders and mode combo box.  This bank is that for the waveshapers: channel c may carry ONE waveshaper node of its
 * own -- Distort with its nine modes (nodes/distort.rs), Overdrive (nodes/overdrive.rs) or Chebyshev (nodes/chebyshev.rs) -- over N
 * channels in the desc's layout (tile_channels as dspfx_engine_desc).  Several shapers per channel are several banks.
 * A node EXISTS for a channel from the first store that names it until dspfx_shapers_drop; a fresh bank has no node anywhere and
 * run copies in to out bit for bit.  The shapers have no state, so there is no reset.
 * PER CHANNEL.  A kind (DSPFX_DISTORT, DSPFX_OVERDRIVE, DSPFX_CHEBYSHEV, or none), a mode (a DSPFX_DIST_* value, Distort only)
 * and up to three sliders in the order of dspfx_node_desc.params: Distort level | Overdrive boost, drive, level | Chebyshev
 * level_pos, level_neg.  Values are taken as given, as dspfx_set_param takes them: no clamp, NaN included.
 * STORES.  A dspfx_shapers_set_* of a family the channel does not carry REPLACES its node: the sliders (and the mode) the call
 * leaves out start from the reference's defaults (dspfx_node_defaults: every slider 0, mode SoftClip).  A set_* of the family it
 * already carries keeps the sliders (and the mode) left out.  An unknown mode or a range past the channels refuses the WHOLE
 * store: DSPFX_ERR_INVALID, the reason in dspfx_shapers_last_error, nothing stored.
 * ONE RUN: queued stores go onto the stream in the order they were made, then per channel:
 *   - out[f][c] is bit for bit what an engine whose chain is that one node, with link_flags = 0, writes for the channel.  The
 *     bank calls the engine's own device functions; where the engine divides by a slider through its fast constant division,
 *     which is exact wherever the engine uses it, the bank divides per lane in IEEE f32: the same bits.
 *   - The bypasses are the reference's: Distort (every mode but Fuzz) and Overdrive give the sample's own bits when level < 0.001
 *     (which a NaN level is not); Chebyshev bypasses per branch (level_pos < 0.001 for samples >= 0, level_neg < 0.001 for the
 *     others, a NaN sample among them).  Its two tanh(level) denominators are computed per channel on the device, once per run.
 *   - A channel without a node keeps its sample's bits.
 * FUZZ (distort.rs:146-172) is block-global over the reference's blocks of 128 frames: three maxima over the channel's block, no
 * bypass, an all-zero block gives NaN.  It runs as a second kernel, in place on out behind the first, launched only when a
 * channel carries Fuzz, with the arithmetic and the order of the engine's Fuzz kernel.  While any channel carries Fuzz a run whose
 * n_frames is not a multiple of DSPFX_BUF_SIZE is refused, as the engine refuses it (DSPFX_ERR_INVALID, the reason; the queued
 * stores have gone onto the stream, nothing else is launched); a bank with no Fuzz channel takes any n_frames up to max_frames.
 * Both decisions go by the stores the run has drained, not by the stores made so far: a drop made on another thread while a run
 * is being submitted cannot take the Fuzz pass away from a run whose tables still hold Fuzz.
 * The first kernel has the shape of the dynamics bank's: a lane owns four adjacent channels (one when the layout or the alignment
 * forbids it), frames go in chunks with the next chunk's loads issued ahead of the arithmetic, stores are nontemporal.  The kinds
 * differ per lane, so a wave ballots once per run for the kinds its lanes carry and runs, per chunk, the body of each kind that
 * is present, wave-uniformly, keeping each result under a select: a wave of 256 channels of one kind pays for one body, a wave
 * that carries all of them for their sum, a wave of copies for none.  The kernel exists twice: without the bodies that evaluate
 * in f64 (Tanh, Sin, Atan, Overdrive, Chebyshev), whose constants cost 85 registers, for tables that hold no such kind, and with.
 * A channel's output is the same bits in either layout, in place or not, on any stream, and whatever its neighbours carry.  No
 * atomics; LDS only in the Fuzz kernel (3 KiB).
 * Not here: control-port modulation of the sliders and link hops, which stay with the engine.
 * Memory: 13 bytes per channel of tables on the device (three sliders and a kind byte; dspfx_shapers_plan), 14 on the host. */
/* dspfx_shapers_kinds: the channel carries no node; dspfx_shapers_modes: it carries no Distort node */
#define DSPFX_SHAPERS_NONE 0xFFFFFFFFu
typedef struct dspfx_shapers dspfx_shapers;
typedef struct dspfx_shapers_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t n_channels;      /* N */
    uint32_t max_frames;      /* largest n_frames a run will pass (>= 1) */
    uint32_t tile_channels;   /* 0 = frame-major; W = channel-tiled, as dspfx_engine_desc */
} dspfx_shapers_desc;
/* PURE HOST function (no GPU, no bank): *bytes_out = the device bytes of a bank's tables, 13 * channels.  channels of 0 or above
 * 2^32 - 256: DSPFX_ERR_INVALID, the reason in dspfx_shapers_last_error(NULL). */
int dspfx_shapers_plan(uint64_t channels, uint64_t *bytes_out);
/* A bad descriptor (channels of 0 or above 2^32 - 256, a tile that is not a power of two dividing n_channels, another ABI version,
 * max_frames of 0) is DSPFX_ERR_INVALID with the reason in dspfx_shapers_last_error of a NULL bank (kept per thread); all of that
 * is checked before any device work. */
int dspfx_shapers_create(const dspfx_shapers_desc *desc, dspfx_shapers **out);
int dspfx_shapers_destroy(dspfx_shapers *s);
/* The reason of the bank's last failed call; of a NULL bank: of this thread's last failed create or plan. */
const char *dspfx_shapers_last_error(const dspfx_shapers *s);
/* in, out: device blocks of n_frames frames in the desc's layout (1 <= n_frames <= max_frames, a multiple of DSPFX_BUF_SIZE while
 * a channel carries Fuzz).  out == in works in place (a thread rewrites the elements it read); any other overlap is the caller's
 * error.  Asynchronous on `stream`; a run on another stream than the one before first waits (on the device) for that one (the
 * rules of dspfx_strips_run).  Queued stores go onto the stream ahead of the kernels, in the order they were made. */
int dspfx_shapers_run(dspfx_shapers *s, const float *in, float *out, uint32_t n_frames, void *stream);
/* Gives channels [first_channel, first_channel + count) a Distort node, from host arrays of `count` values each: the level
 * sliders and the modes (DSPFX_DIST_*).  Either may be NULL: kept where the channel carries a Distort node, the default (level 0,
 * SoftClip) where it carries another node or none.  The contract of dspfx_dynamics_set: callable from any thread while runs are in
 * flight, never waits for the device or for a run; the values are staged in page-locked memory and queued, each store is whole,
 * and a run submitted after the call returns sees it, the runs submitted before it do not. */
int dspfx_shapers_set_distort(dspfx_shapers *s, const float *host_level, const uint32_t *host_mode, uint64_t first_channel, uint64_t count);
/* ... an Overdrive node: boost, drive, level (each may be NULL; the defaults are 0).  Rules as dspfx_shapers_set_distort. */
int dspfx_shapers_set_overdrive(dspfx_shapers *s, const float *host_boost, const float *host_drive, const float *host_level, uint64_t first_channel,
                                uint64_t count);
/* ... a Chebyshev node: level_pos, level_neg (each may be NULL; the defaults are 0).  Rules as dspfx_shapers_set_distort. */
int dspfx_shapers_set_chebyshev(dspfx_shapers *s, const float *host_level_pos, const float *host_level_neg, uint64_t first_channel, uint64_t count);
/* Removes the node of channels [first_channel, first_channel + count): a copy again, and a later store starts from the defaults.
 * Queued like a store.  A range past the channels: DSPFX_ERR_INVALID and the reason. */
int dspfx_shapers_drop(dspfx_shapers *s, uint64_t first_channel, uint64_t count);
/* The host tables over [first_channel, first_channel + count), as all stores made so far left them: present 1 / 0 (the channel
 * carries a node); kinds DSPFX_DISTORT, DSPFX_OVERDRIVE, DSPFX_CHEBYSHEV or DSPFX_SHAPERS_NONE; modes the DSPFX_DIST_* value of a
 * Distort node, DSPFX_SHAPERS_NONE for every other channel; sliders [count][3] in the order of dspfx_node_desc.params, 0 where the
 * node has fewer than three and where there is no node. */
int dspfx_shapers_present(dspfx_shapers *s, uint32_t *host_present_out, uint64_t first_channel, uint64_t count);
int dspfx_shapers_kinds(dspfx_shapers *s, uint32_t *host_kinds_out, uint64_t first_channel, uint64_t count);
int dspfx_shapers_modes(dspfx_shapers *s, uint32_t *host_modes_out, uint64_t first_channel, uint64_t count);
int dspfx_shapers_sliders(dspfx_shapers *s, float *host_sliders_out, uint64_t first_channel, uint64_t count);

/* ---- channel filters: a bank of per-channel LowPass, HighPass and Envelope -------------------------------------------
 * The three chain nodes that carry exactly one float of state, per channel: LowPass (nodes/low_pass.rs:36-39), HighPass
 * (nodes/high_pass.rs:36-39) and Envelope (nodes/envelope.rs:34-52) as a node whose OUTPUT is the envelope -- the dynamics and
 * talker banks keep theirs as a hidden detector.  A rumble and a hiss filter of each participant's own (HighPass then LowPass),
 * a de-zipper on a per-channel control block ahead of an engine's control port, an envelope follower per channel with a smoothing
 * LowPass behind it in the same launch.  Over N channels in the desc's layout (tile_channels as dspfx_engine_desc).
 * PER CHANNEL.  `stages` SLOTS (1 .. 4), run in slot order 0 .. stages - 1.  A slot is empty, LowPass, HighPass or Envelope, with
 * one float of state (z, or the envelope; starts +0.0) and its sliders: ratio r | attack and release in frames, converted on the
 * host by dspfx_envelope_gain into ga and gr (as dspfx_talkers_set_detector and dspfx_dynamics_set do).  Values are taken as given,
 * as dspfx_set_param takes them: no clamp, NaN, infinities and values outside the slider's range included.  A fresh bank has
 * every slot of every channel empty: run copies in to out bit for bit and leaves every table at rest.
 * STORES.  A slot's node is NEW from the first dspfx_filters_set_* that names it, and after a set_* of another kind than it
 * carries: state +0.0, and the reference's defaults for the sliders the call leaves out (ratio 0.5, attack 0, release 0).  A set_*
 * of the kind the slot already carries keeps the sliders left out AND THE STATE: none of the three nodes has an
 * after_settings_change (low_pass.rs, high_pass.rs, envelope.rs; only reverb.rs:19 and biquad.rs:15 do), which is also what
 * dspfx_set_param does for them.  Whether a store meets the same kind is decided when the store is made, from the host tables,
 * whatever is in flight.  dspfx_filters_drop empties a slot and zeroes its state; dspfx_filters_reset zeroes state and keeps nodes
 * and sliders.  A stage >= stages or a range past the channels refuses the WHOLE store: DSPFX_ERR_INVALID, the reason in
 * dspfx_filters_last_error, nothing stored.
 * ONE RUN: queued stores go onto the stream in the order they were made, then per channel, frames in order, slots in order,
 * nothing contracted, every operation one IEEE f32 round-to-nearest:
 *       LowPass    y = x * (1 - r) + r * z;   z = y                        (chain_kernels.hip.h K_LOW_PASS)
 *       HighPass   z = x * (1 - r) + r * z;   y = x - z                    (K_HIGH_PASS)
 *       Envelope   d = x < 0 ? -x : x;   g = z < d ? ga : gr;   z = d + (z + (-d)) * g;   y = z       (K_ENVELOPE)
 *       empty      y = x: the sample's own bits, not a multiplication by one
 * So out[f][c] is bit for bit what an engine whose chain is the channel's present nodes in slot order, with link_flags = 0,
 * writes for the channel, in either layout, in place or not, on any stream, whatever its neighbours carry and however the frames
 * are cut into runs (the recurrences carry no block structure); the state tables equal the engine's exported node state.
 * The kernel has the shape of the dynamics bank's: a lane owns four adjacent channels (one when the layout or the alignment
 * forbids it), frames go in chunks with the next chunk's loads issued ahead of the arithmetic, stores are nontemporal; `stages`
 * is a template parameter and every slot lives in registers.  The kinds differ per lane: a wave ballots once per run, stage and
 * kind, and takes per chunk and stage one wave-uniform branch: the body of the one kind its lanes carry, or, where they carry
 * several, one body that computes the one-pole and the envelope for every value and selects by the channel's kind.
 * A wave none of whose lanes carries a node in a stage does no arithmetic for that stage.  No atomics, no LDS.
 * Not here: link hops, control-port modulation of the sliders (none of the three is a control input in the reference) and graph
 * wiring, which stay with the engine.
 * Memory: 13 bytes per channel and stage of tables on the device (two sliders, the state and a kind byte; dspfx_filters_plan),
 * 9 on the host. */
/* dspfx_filters_kinds: the slot is empty; dspfx_filters_reset: every stage */
#define DSPFX_FILTERS_NONE 0xFFFFFFFFu
typedef struct dspfx_filters dspfx_filters;
typedef struct dspfx_filters_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t n_channels;      /* N */
    uint32_t max_frames;      /* largest n_frames a run will pass (>= 1) */
    uint32_t tile_channels;   /* 0 = frame-major; W = channel-tiled, as dspfx_engine_desc */
    uint32_t stages;          /* slots per channel, 1 .. 4 */
} dspfx_filters_desc;
/* PURE HOST function (no GPU, no bank): *bytes_out = the device bytes of a bank's tables, 13 * stages * channels.  channels of 0
 * or above 2^32 - 256, stages outside 1 .. 4: DSPFX_ERR_INVALID, the reason in dspfx_filters_last_error(NULL). */
int dspfx_filters_plan(uint64_t channels, uint32_t stages, uint64_t *bytes_out);
/* A bad descriptor (channels of 0 or above 2^32 - 256, a tile that is not a power of two dividing n_channels, another ABI version,
 * max_frames of 0, stages outside 1 .. 4) is DSPFX_ERR_INVALID with the reason in dspfx_filters_last_error of a NULL bank (kept
 * per thread); all of that is checked before any device work. */
int dspfx_filters_create(const dspfx_filters_desc *desc, dspfx_filters **out);
int dspfx_filters_destroy(dspfx_filters *f);
/* The reason of the bank's last failed call; of a NULL bank: of this thread's last failed create or plan. */
const char *dspfx_filters_last_error(const dspfx_filters *f);
/* in, out: device blocks of n_frames frames in the desc's layout (1 <= n_frames <= max_frames).  out == in works in place (a
 * thread rewrites the elements it read); any other overlap is the caller's error.  Asynchronous on `stream`; a run on another
 * stream than the one before first waits (on the device) for that one, since the state is the bank's (the rules of
 * dspfx_strips_run).  Queued stores go onto the stream ahead of the kernel, in the order they were made. */
int dspfx_filters_run(dspfx_filters *f, const float *in, float *out, uint32_t n_frames, void *stream);
/* Gives slot `stage` of channels [first_channel, first_channel + count) a LowPass node, from a host array of `count` ratios.
 * NULL: kept where the slot carries a LowPass node, the default 0.5 where it carries another node or none.  The contract of
 * dspfx_dynamics_set: callable from any thread while runs are in flight, never waits for the device or for a run; the values are
 * staged in page-locked memory and queued, each store is whole, and a run submitted after the call returns sees it, the runs
 * submitted before it do not. */
int dspfx_filters_set_low_pass(dspfx_filters *f, uint32_t stage, const float *host_ratio, uint64_t first_channel, uint64_t count);
/* ... a HighPass node.  Rules as dspfx_filters_set_low_pass (a LowPass slot that becomes HighPass is a new node). */
int dspfx_filters_set_high_pass(dspfx_filters *f, uint32_t stage, const float *host_ratio, uint64_t first_channel, uint64_t count);
/* ... an Envelope node: attack and release in frames (each may be NULL; the defaults are 0).  Rules as dspfx_filters_set_low_pass. */
int dspfx_filters_set_envelope(dspfx_filters *f, uint32_t stage, const float *host_attack, const float *host_release, uint64_t first_channel,
                               uint64_t count);
/* Empties slot `stage` of channels [first_channel, first_channel + count) and zeroes its state: that stage copies again, and a
 * later store starts from the defaults.  Queued like a store. */
int dspfx_filters_drop(dspfx_filters *f, uint32_t stage, uint64_t first_channel, uint64_t count);
/* The state of slot `stage` (DSPFX_FILTERS_NONE: of every slot) back to +0.0 on the range; the nodes and the sliders stay.
 * Queued like a store.  Also the way out for a slot whose state became NaN. */
int dspfx_filters_reset(dspfx_filters *f, uint32_t stage, uint64_t first_channel, uint64_t count);
/* The host tables over [first_channel, first_channel + count), as all stores made so far left them: present 1 / 0 (a slot of
 * the channel carries a node); kinds of slot `stage` DSPFX_LOW_PASS, DSPFX_HIGH_PASS, DSPFX_ENVELOPE or DSPFX_FILTERS_NONE; sliders
 * of slot `stage` [count][2] as they were given: ratio, 0 | attack, release (frames); 0, 0 for an empty slot. */
int dspfx_filters_present(dspfx_filters *f, uint32_t *host_present_out, uint64_t first_channel, uint64_t count);
int dspfx_filters_kinds(dspfx_filters *f, uint32_t stage, uint32_t *host_kinds_out, uint64_t first_channel, uint64_t count);
int dspfx_filters_sliders(dspfx_filters *f, uint32_t stage, float *host_sliders_out, uint64_t first_channel, uint64_t count);
/* The device pointer of slot `stage`'s state[N]: z of a one-pole, the envelope of an Envelope, +0.0 of an empty slot.  The pointer
 * never changes; what it holds is valid after a run, on its stream. */
int dspfx_filters_state(dspfx_filters *f, uint32_t stage, const float **state_out);

/* ---- channel FIRs: a bank of per-channel FIR nodes, each with its own taps --------------------------------------------
 * An engine runs one FIR node (nodes/fir.rs) with one tap table for all N channels, and the Convolver bank shares at most 256
 * long responses.  This bank gives channel c ONE FIR node of its own: its own taps (f64), tap count T (1 .. max_taps), mode and
 * VecDeque of past samples, over N channels in the desc's layout (tile_channels as dspfx_engine_desc).  A linear-phase EQ, a
 * fractional delay for time alignment, a short cabinet or handset model, the taps of an adaptive echo canceller: short filters
 * that are different numbers on every channel.
 * A node EXISTS for a channel from the first dspfx_firs_set_taps that names it until dspfx_firs_drop; a fresh bank has no node
 * anywhere: run copies in to out bit for bit.
 * PER CHANNEL, per sample, what fir.rs:179-225 does: push; pop ONE sample when the deque is longer than T; then
 *       a = (float) sum_{k < min(n_a, T)} state[k] * taps[k]                              sequential f64, nothing fused
 *       b = (float) sum_{k < min(len - n_a, T - n_a)} state[n_a + k] * taps[n_a + k]     (+0.0 when n_a >= T)
 *       out = (a + b) * divisor               divisor 1.0f (DSPFX_FIR_BALANCED) or 1.0f / (float)T (DSPFX_FIR_AVERAGE)
 * with taps the response REVERSED (fir.rs:163,168) and n_a the length of the first physical slice of the reference's VecDeque
 * (capacity 0, then 4, then doubling).  NaN, infinities and signed zeros go through the arithmetic as they are.  So out[f][c] is
 * bit for bit what the reference's node gives through all its history, in either layout, in place or not, on any stream,
 * whatever the channel's neighbours carry and however the frames are cut into runs.
 * STORES.  dspfx_firs_set_taps on a channel without a node makes a NEW node: an empty deque, mode DSPFX_FIR_BALANCED unless the
 * call names one.  On a channel that carries a node it is the reference's reload (fir.rs:153-171): the taps are replaced, the
 * deque and (with mode DSPFX_FIRS_NONE) the mode are kept -- a deque longer than a shorter new response stays longer, a pure extra
 * delay.  dspfx_firs_drop removes the node, so the next set_taps makes a new one; dspfx_firs_reset empties the deque and keeps
 * taps and mode.  n_taps of 0 or above max_taps, a range past the channels, an unknown mode or no array refuses the WHOLE store:
 * DSPFX_ERR_INVALID, the reason in dspfx_firs_last_error, nothing stored.
 * ON THE DEVICE, per channel: the taps table, max_taps doubles laid out [tap][N] so the lanes of a wave (a lane is a channel)
 * read one tap of 64 channels in one access; a ring of max_taps + 16 float samples in time, [row][N]; one word of T and mode; the
 * three deque words len, cap, head, which the kernel steps itself per frame.  dspfx_firs_plan:
 *       bytes = channels * (8 * max_taps + 4 * (max_taps + 16) + 4 + 12) = channels * (12 * max_taps + 80)
 * Only the node words and the deque words are cleared at create.  On the host: 31 bytes per channel and one copy of every
 * response a channel still carries.
 * ONE RUN is one kernel behind the queued stores, one lane per channel.  A wave whose present lanes all stand at len == T < cap
 * with the same T takes the next sixteen frames at once: the taps are read once per sixteen frames, the samples slide through a
 * register window, and every frame keeps one running f64 sum that is rounded and restarted at +0.0 where its first slice ends.
 * Otherwise the wave takes one frame with the two sums as written above (the fill phase, a deque longer than its taps, lanes of
 * different T) and decides again, so a new node leaves that slower body at most sixteen frames after its deque is full.  A wave
 * without a node copies.  No atomics, no LDS.
 * Not here: link hops, control ports and graph wiring, which stay with the engine; T above DSPFX_FIRS_MAX_TAPS, the Convolver's. */
#define DSPFX_FIRS_MAX_TAPS 1024u
/* dspfx_firs_modes: the channel carries no node; dspfx_firs_set_taps: keep the node's mode (a new node: DSPFX_FIR_BALANCED) */
#define DSPFX_FIRS_NONE 0xFFFFFFFFu
typedef struct dspfx_firs dspfx_firs;
typedef struct dspfx_firs_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t n_channels;      /* N */
    uint32_t max_frames;      /* largest n_frames a run will pass (>= 1) */
    uint32_t tile_channels;   /* 0 = frame-major; W = channel-tiled, as dspfx_engine_desc */
    uint32_t max_taps;        /* the longest response a channel may carry, 1 .. DSPFX_FIRS_MAX_TAPS */
    uint32_t general_only;    /* 0; 1: every wave takes the frames one at a time (for timing one body against the other) */
} dspfx_firs_desc;
/* PURE HOST function (no GPU, no bank): *bytes_out = the device bytes of a bank's tables, channels * (12 * max_taps + 80).
 * channels of 0 or above 2^32 - 256, max_taps outside 1 .. 1024: DSPFX_ERR_INVALID, the reason in dspfx_firs_last_error(NULL). */
int dspfx_firs_plan(uint64_t channels, uint32_t max_taps, uint64_t *bytes_out);
/* A bad descriptor (channels of 0 or above 2^32 - 256, a tile that is not a power of two dividing n_channels, another ABI version,
 * max_frames of 0, max_taps outside 1 .. 1024) is DSPFX_ERR_INVALID with the reason in dspfx_firs_last_error of a NULL bank (kept
 * per thread); all of that is checked before any device work. */
int dspfx_firs_create(const dspfx_firs_desc *desc, dspfx_firs **out);
int dspfx_firs_destroy(dspfx_firs *f);
/* The reason of the bank's last failed call; of a NULL bank: of this thread's last failed create or plan. */
const char *dspfx_firs_last_error(const dspfx_firs *f);
/* in, out: device blocks of n_frames frames in the desc's layout (1 <= n_frames <= max_frames).  out == in works in place (a
 * thread rewrites the elements it read); any other overlap is the caller's error.  Asynchronous on `stream`; a run on another
 * stream than the one before first waits (on the device) for that one, since the state is the bank's (the rules of
 * dspfx_strips_run).  Queued stores go onto the stream ahead of the kernel, in the order they were made. */
int dspfx_firs_run(dspfx_firs *f, const float *in, float *out, uint32_t n_frames, void *stream);
/* Gives channels [first_channel, first_channel + count) a response of n_taps taps in TIME order (h[0] meets the newest sample; the
 * bank reverses them): per_channel 0: host_taps is [n_taps], one response for the range; 1: [count][n_taps], a response per
 * channel.  mode: DSPFX_FIR_BALANCED, DSPFX_FIR_AVERAGE, or DSPFX_FIRS_NONE to keep the node's.  The contract of dspfx_dynamics_set:
 * callable from any thread while runs are in flight, never waits for the device or for a run; the values are staged in page-locked
 * memory and queued, each store is whole, and a run submitted after the call returns sees it, the runs submitted before it do not. */
int dspfx_firs_set_taps(dspfx_firs *f, const double *host_taps, uint32_t n_taps, uint32_t per_channel, uint32_t mode, uint64_t first_channel,
                        uint64_t count);
/* The mode of the nodes on the range (a channel without a node stays without one).  Queued like a store. */
int dspfx_firs_set_mode(dspfx_firs *f, uint32_t mode, uint64_t first_channel, uint64_t count);
/* Removes the node of the channels of the range: a copy again, and a later set_taps makes a new node.  Queued like a store. */
int dspfx_firs_drop(dspfx_firs *f, uint64_t first_channel, uint64_t count);
/* Empties the deque of the channels of the range (what dspfx_reset does for the engine's FIR node); taps and mode stay.  Queued
 * like a store. */
int dspfx_firs_reset(dspfx_firs *f, uint64_t first_channel, uint64_t count);
/* The host tables over [first_channel, first_channel + count), as all stores made so far left them: present 1 / 0; lengths T, 0
 * without a node; modes DSPFX_FIR_BALANCED, DSPFX_FIR_AVERAGE, or DSPFX_FIRS_NONE without a node. */
int dspfx_firs_present(dspfx_firs *f, uint32_t *host_present_out, uint64_t first_channel, uint64_t count);
int dspfx_firs_lengths(dspfx_firs *f, uint32_t *host_lengths_out, uint64_t first_channel, uint64_t count);
int dspfx_firs_modes(dspfx_firs *f, uint32_t *host_modes_out, uint64_t first_channel, uint64_t count);
/* The response of ONE channel as it was given (time order): *n_taps_out = T (0 without a node), host_taps_out[0 .. T); the array
 * has room for max_taps doubles. */
int dspfx_firs_taps(dspfx_firs *f, uint64_t channel, double *host_taps_out, uint32_t *n_taps_out);
/* The device pointer of the deque words, int32 [3][N]: len, cap, head of every channel's VecDeque after the last run (0, 0, 0
 * without a node or before the first sample).  The pointer never changes; what it holds is valid after a run, on its stream. */
int dspfx_firs_deque(dspfx_firs *f, const int32_t **deque_out);

/* ---- channel racks: a per-channel chain of mixed nodes in one pass ----------------------------------------------------
 * The strips, filters and shapers banks give every channel its own sliders, but the ORDER of the nodes is the order of the host's
 * run calls, the same for all N channels, and every bank is a launch with one read and one write of the block.  A rack gives
 * channel c a chain of its own: `slots` SLOTS (1 .. 4), run in slot order 0 .. slots - 1, each empty or carrying ANY ONE of the
 * small-state chain nodes with its own sliders and state, all slots between one load and one store of the block.  Over N channels
 * in the desc's layout (tile_channels as dspfx_engine_desc).  A fresh bank has every slot empty: run copies in to out bit for bit.
 * PER SLOT AND CHANNEL.  A kind (a dspfx_kind, or none), a mode (Distort only) and up to six sliders in the order of
 * dspfx_node_desc.params, four floats of state:
 *       kind               sliders                          state            arithmetic
 *       DSPFX_GAIN         level                            -                x * level                      (gain.rs:33-37)
 *       DSPFX_BIQUAD       raw a0, a1, a2, b0, b1, b2       x1, x2, y1, y2   normalised by dspfx_strips_coeffs; the strips bank's row,
 *                                                                            b0 * x + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2 in that order
 *       DSPFX_LOW_PASS     ratio                            z                the filters bank's bodies, every operation one IEEE f32
 *       DSPFX_HIGH_PASS    ratio                            z                round-to-nearest
 *       DSPFX_ENVELOPE     attack, release (frames)         env              the filters bank's; the gains by dspfx_envelope_gain
 *       DSPFX_DISTORT      level; mode: the eight DSPFX_DIST_* other than Fuzz    -    the engine's distort1, the shapers bank's bypass
 *                                                                            (level < 0.001, which a NaN level is not)
 *       DSPFX_OVERDRIVE    boost, drive, level              -                the engine's overdrive1, the shapers bank's bypass
 *       DSPFX_CHEBYSHEV    level_pos, level_neg             -                the engine's chebyshev1; the two tanh denominators once per run
 *   An empty slot keeps the sample's own bits.  Values are taken as given: no clamp, NaN and out-of-range values included.
 *   NOT HERE, refused as kinds with a reason that names the bank that has them: DSPFX_REVERB (delays), DSPFX_FIR (firs), DSPFX_ADD
 *   and DSPFX_MIX (blends), DSPFX_SIGNAL_GEN (gens); Fuzz, which is block-global, stays with the shapers bank.  Link hops, control
 *   ports and graph wiring stay with the engine.  More than four slots are two racks in a row.
 * THE CONTRACT.  For any table of kinds and sliders and any sequence of stores and run lengths a channel's output is BIT FOR BIT
 * what the existing banks give when they are run slot after slot on the same stream -- for slot t a dspfx_filters bank of one
 * stage, then a dspfx_strips bank of one band with link_flags 0, then a dspfx_shapers bank, each persistent across runs and each
 * carrying slot t's node on exactly the channels whose slot t holds a kind of its family -- and the slot's state is theirs.  So a
 * channel without a BiQuad equals an engine whose chain is its present nodes in slot order with link_flags = 0 bit for bit, and a
 * BiQuad slot is within 1 ulp of the engine's BiQuad, as the strips bank is.  A channel's bits are the same in either layout, in
 * place or not, on any stream, however the frames are cut into runs and whatever its neighbours carry.
 * STORES.  dspfx_racks_set of a kind the slot does not carry makes a NEW node: state +0.0, and the values of dspfx_node_defaults
 * for what the call leaves NULL.  A set of the kind the slot carries keeps what is NULL; it KEEPS THE STATE for LowPass, HighPass
 * and Envelope (none has an after_settings_change) and ZEROES it for BiQuad on the stored channels (biquad.rs:62-76, as
 * dspfx_strips_set_band).  dspfx_racks_drop empties a slot and zeroes its state; dspfx_racks_reset zeroes state and keeps nodes and
 * sliders.  A slot the bank does not have, a range past the channels, a kind outside the table, an unknown Distort mode or Fuzz
 * refuse the WHOLE store: DSPFX_ERR_INVALID, the reason in dspfx_racks_last_error, nothing stored.  All stores go through the
 * staged-store queue: from any thread, never waiting for the device, governing the runs submitted after they return.
 * ONE RUN is one kernel behind the drained stores: a lane owns its channels for the whole run (four adjacent channels per 16-byte
 * access at one or two slots, two at four slots, one when the layout or the alignment forbids vectors), frames go in chunks with
 * the next chunk's loads issued ahead of the arithmetic, stores are nontemporal, `slots` is a template parameter (a bank of three
 * runs the kernel of four) and every slot lives in registers.  The kinds differ per lane and slot: a wave ballots once per run
 * and slot, and per chunk and slot runs each present kind's body wave-uniformly under a per-channel select; a wave whose lanes
 * carry nothing in a slot does no arithmetic for it and reads neither its sliders nor its state.  A bank whose drained tables hold
 * no kind that evaluates in f64 (Tanh, Sin, Atan, Overdrive, Chebyshev) runs an instantiation without those bodies.  No atomics,
 * no LDS.
 * Memory: 37 bytes per channel and slot of tables on the device (five slider fields, four state floats and a kind byte;
 * dspfx_racks_plan), 26 on the host. */
/* dspfx_racks_kinds: the slot is empty; dspfx_racks_modes: it carries no Distort node; dspfx_racks_reset: every slot */
#define DSPFX_RACKS_NONE 0xFFFFFFFFu
#define DSPFX_RACKS_MAX_SLOTS 4
typedef struct dspfx_racks dspfx_racks;
typedef struct dspfx_racks_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t n_channels;      /* N */
    uint32_t max_frames;      /* largest n_frames a run will pass (>= 1) */
    uint32_t tile_channels;   /* 0 = frame-major; W = channel-tiled, as dspfx_engine_desc */
    uint32_t slots;           /* slots per channel, 1 .. DSPFX_RACKS_MAX_SLOTS */
} dspfx_racks_desc;
/* PURE HOST function (no GPU, no bank): *bytes_out = the device bytes of a bank's tables, 37 * slots * channels.  channels of 0 or
 * above 2^32 - 256, slots outside 1 .. 4: DSPFX_ERR_INVALID, the reason in dspfx_racks_last_error(NULL). */
int dspfx_racks_plan(uint64_t channels, uint32_t slots, uint64_t *bytes_out);
/* A bad descriptor (channels of 0 or above 2^32 - 256, a tile that is not a power of two dividing n_channels, another ABI version,
 * max_frames of 0, slots outside 1 .. 4) is DSPFX_ERR_INVALID with the reason in dspfx_racks_last_error of a NULL bank (kept per
 * thread); all of that is checked before any device work. */
int dspfx_racks_create(const dspfx_racks_desc *desc, dspfx_racks **out);
int dspfx_racks_destroy(dspfx_racks *r);
/* The reason of the bank's last failed call; of a NULL bank: of this thread's last failed create or plan. */
const char *dspfx_racks_last_error(const dspfx_racks *r);
/* in, out: device blocks of n_frames frames in the desc's layout (1 <= n_frames <= max_frames).  out == in works in place (a
 * thread rewrites the elements it read); any other overlap is the caller's error.  Asynchronous on `stream`; a run on another
 * stream than the one before first waits (on the device) for that one, since the state is the bank's (the rules of
 * dspfx_strips_run).  Queued stores go onto the stream ahead of the kernel, in the order they were made. */
int dspfx_racks_run(dspfx_racks *r, const float *in, float *out, uint32_t n_frames, void *stream);
/* Gives slot `slot` of channels [first_channel, first_channel + count) a node of `kind` (a dspfx_kind of the table above).
 * host_sliders: NULL or six pointers in the order of dspfx_node_desc.params, each NULL or a host array of `count` values; those
 * behind the kind's slider count are not read.  host_mode: NULL or `count` DSPFX_DIST_* values, read for DSPFX_DISTORT only.  What
 * is NULL is kept where the slot carries the kind and is the default of dspfx_node_defaults where it carries another or none.  The
 * contract of dspfx_dynamics_set: callable from any thread while runs are in flight, never waits for the device or for a run; the
 * values are staged in page-locked memory and queued, each store is whole, and a run submitted after the call returns sees it,
 * the runs submitted before it do not. */
int dspfx_racks_set(dspfx_racks *r, uint32_t slot, uint32_t kind, const float *const *host_sliders, const uint32_t *host_mode, uint64_t first_channel,
                    uint64_t count);
/* Empties slot `slot` of channels [first_channel, first_channel + count) and zeroes its state: that slot copies again, and a
 * later store starts from the defaults.  Queued like a store. */
int dspfx_racks_drop(dspfx_racks *r, uint32_t slot, uint64_t first_channel, uint64_t count);
/* The state of slot `slot` (DSPFX_RACKS_NONE: of every slot) back to +0.0 on the range; the nodes and the sliders stay.  Queued
 * like a store.  Also the way out for a slot whose state became NaN. */
int dspfx_racks_reset(dspfx_racks *r, uint32_t slot, uint64_t first_channel, uint64_t count);
/* The host tables over [first_channel, first_channel + count), as all stores made so far left them: present, bit t set where slot
 * t carries a node; kinds of slot `slot`, a dspfx_kind or DSPFX_RACKS_NONE; modes of slot `slot`, the DSPFX_DIST_* value of a
 * Distort node, DSPFX_RACKS_NONE otherwise; sliders of slot `slot` [count][6] raw, as they were given, 0 behind the kind's slider
 * count and for an empty slot. */
int dspfx_racks_present(dspfx_racks *r, uint32_t *host_present_out, uint64_t first_channel, uint64_t count);
int dspfx_racks_kinds(dspfx_racks *r, uint32_t slot, uint32_t *host_kinds_out, uint64_t first_channel, uint64_t count);
int dspfx_racks_modes(dspfx_racks *r, uint32_t slot, uint32_t *host_modes_out, uint64_t first_channel, uint64_t count);
int dspfx_racks_sliders(dspfx_racks *r, uint32_t slot, float *host_sliders_out, uint64_t first_channel, uint64_t count);
/* The device pointer of slot `slot`'s state, float [4][N]: row 0 is z of a one-pole or the envelope, rows 0 .. 3 are x1, x2, y1, y2
 * of a BiQuad, +0.0 everywhere else.  The pointer never changes; what it holds is valid after a run, on its stream. */
int dspfx_racks_state(dspfx_racks *r, uint32_t slot, const float **state_out);

/* ---- channel cancellers: a bank of per-channel adaptive (NLMS) FIR filters ---------------------------------------------
 * The FIR bank's taps come from the host.  This bank gives channel c ONE adaptive filter of its own whose taps the DEVICE updates
 * every frame: the stage that removes a participant's own return from their microphone (an echo canceller), adaptive noise
 * cancelling against a reference pick-up, feedback suppression, live identification of a channel's path.  Two blocks come in, in
 * the desc's layout (tile_channels as dspfx_engine_desc): mic, the primary input d, and ref, the block the channel was sent.
 * A node EXISTS for a channel from the first dspfx_cancel_set that names it until dspfx_cancel_drop; a fresh bank has no node
 * anywhere: run copies mic to out bit for bit and reads no ref.
 * PER CHANNEL: T taps (1 .. max_taps), weights w[0 .. T), a step size mu, a regulariser eps, a bulk delay D (0 .. max_delay), the
 * switch adapt.  All arithmetic is f32, every operation rounded once, as written, nothing fused or reassociated.  For frame n of
 * the bank's own frame count:
 *       u[k] = ref[n - D - k], k < T            +0.0 where that frame lies before the node's first frame (its creation or its
 *                                               last reset); the history runs across runs
 *       dot(a, b) = (s_0 + s_1) + (s_2 + s_3)   four chains from +0.0; chain j takes the k = j (mod 4) in ascending k,
 *                                               s_j = s_j + (a[k] * b[k]); every k < T is a product as written, no term k >= T exists
 *       y = dot(w, u);  e = d[n] - y;  out[n] = e
 *       adapt only:  p = dot(u, u);  g = (mu * e) / (p + eps), one IEEE division;  w[k] = w[k] + (g * u[k]) for every k < T
 *       levels: sum d * d and sum e * e over the run, in frame order, from +0.0
 * Values are taken as given, NaN included: a NaN or an infinity that reaches a channel's weights stays in that channel until
 * dspfx_cancel_reset and never reaches a neighbour.  So a channel's out, weights and levels are the same bits in either layout, in
 * place or not, on any stream, whatever its neighbours carry and however the frames are cut into runs (the levels are per run).
 * STORES.  dspfx_cancel_set on a channel without a node makes a NEW node: weights and history +0.0, and for what the call leaves
 * NULL: max_taps taps, mu 0.5, eps 1e-6, delay 0, adapting.  On a channel that carries a node it keeps what it leaves NULL and
 * keeps the weights and the history: a smaller T zeroes the rows k >= T, a larger T starts the new rows at +0.0 (the weights
 * table holds +0.0 in every row k >= the node's T, always); a new delay only moves the window.  dspfx_cancel_load replaces the
 * weights (a warm start).  dspfx_cancel_drop removes the node; dspfx_cancel_reset puts weights and history back to +0.0 and
 * keeps T, mu, eps, delay and adapt.  A T of 0 or above max_taps, a delay above max_delay, a range past the channels, a load on a
 * channel without a node or with another T refuses the WHOLE store: DSPFX_ERR_INVALID, the reason in dspfx_cancel_last_error,
 * nothing stored.
 * ON THE DEVICE, per channel: max_taps float weights laid out [tap][N], so the lanes of a wave (a lane is a channel) read one tap
 * of 64 channels in one access; a ring in time of R float reference samples, R = max_delay + max_taps + 16 rounded up to a multiple
 * of 8, the rows in groups of eight, [row / 8][N][8], so the eight rows a lane writes and reads per block are 32 bytes of its own
 * whatever its delay; the node word (T and adapt), the delay, mu, eps; two levels.  dspfx_cancel_plan:
 *       bytes = channels * (4 * max_taps + 4 * R + 16 + 8)
 * ONE RUN is one kernel behind the queued stores, one lane per channel.  A wave whose present lanes share one T <= 64 keeps the
 * weights in registers for the whole run and the window in a sliding register window, eight frames per block; otherwise (lanes
 * of different T, T above 64, the frames behind a run's last whole block) a lane takes one frame at a time from the tables under
 * its own bounds.  Both do the same operations in the same order.  A wave without a node copies.  No atomics, no LDS.
 * 1024 taps are 21 ms at 48 kHz: line and handset echo behind a bulk delay, not a room's tail.
 * Not here: a frequency-domain form for long tails, a double-talk detector (adapt is the host's), leakage, step-size control, a
 * residual suppressor, link hops and graph wiring. */
#define DSPFX_CANCEL_MAX_TAPS 1024u
#define DSPFX_CANCEL_MAX_DELAY 65535u
typedef struct dspfx_cancel dspfx_cancel;
typedef struct dspfx_cancel_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t n_channels;      /* N */
    uint32_t max_frames;      /* largest n_frames a run will pass (>= 1) */
    uint32_t tile_channels;   /* 0 = frame-major; W = channel-tiled, as dspfx_engine_desc */
    uint32_t max_taps;        /* the longest filter a channel may carry, 1 .. DSPFX_CANCEL_MAX_TAPS */
    uint32_t max_delay;       /* the longest bulk delay a channel may carry, 0 .. DSPFX_CANCEL_MAX_DELAY frames */
    uint32_t general_only;    /* 0; 1: every wave takes the frames one at a time (for showing that both bodies give the same bits) */
} dspfx_cancel_desc;
/* PURE HOST function (no GPU, no bank): *bytes_out = the device bytes of a bank's tables, channels * (4 * max_taps + 4 * R + 24), R =
 * max_delay + max_taps + 16 rounded up to a multiple of 8.  channels of 0 or above 2^32 - 256, max_taps outside 1 .. 1024, max_delay above 65535: DSPFX_ERR_INVALID, the reason in
 * dspfx_cancel_last_error(NULL). */
int dspfx_cancel_plan(uint64_t channels, uint32_t max_taps, uint32_t max_delay, uint64_t *bytes_out);
/* A bad descriptor (channels of 0 or above 2^32 - 256, a tile that is not a power of two dividing n_channels, another ABI version,
 * max_frames of 0, max_taps outside 1 .. 1024, max_delay above 65535) is DSPFX_ERR_INVALID with the reason in
 * dspfx_cancel_last_error of a NULL bank (kept per thread); all of that is checked before any device work. */
int dspfx_cancel_create(const dspfx_cancel_desc *desc, dspfx_cancel **out);
int dspfx_cancel_destroy(dspfx_cancel *a);
/* The reason of the bank's last failed call; of a NULL bank: of this thread's last failed create or plan. */
const char *dspfx_cancel_last_error(const dspfx_cancel *a);
/* mic, ref, out: device blocks of n_frames frames in the desc's layout (1 <= n_frames <= max_frames).  out == mic works in place (a
 * thread rewrites the elements it read).  No ref, or an out that overlaps ref, refuses the run: DSPFX_ERR_INVALID.  Asynchronous
 * on `stream`; a run on another stream than the one before first waits (on the device) for that one, since the state is the
 * bank's (the rules of dspfx_strips_run).  Queued stores go onto the stream ahead of the kernel, in the order they were made. */
int dspfx_cancel_run(dspfx_cancel *a, const float *mic, const float *ref, float *out, uint32_t n_frames, void *stream);
/* The node of channels [first_channel, first_channel + count): each array is NULL (keep; a new node: the default) or `count`
 * values -- host_taps T, host_mu, host_eps, host_delay D, host_adapt 0 / not 0.  The contract of dspfx_dynamics_set: callable from
 * any thread while runs are in flight, never waits for the device or for a run; the values are staged in page-locked memory and
 * queued, each store is whole, and a run submitted after the call returns sees it, the runs submitted before it do not. */
int dspfx_cancel_set(dspfx_cancel *a, const uint32_t *host_taps, const float *host_mu, const float *host_eps, const uint32_t *host_delay,
                     const uint32_t *host_adapt, uint64_t first_channel, uint64_t count);
/* Replaces the weights of the channels of the range, every one of which carries a node of n_taps taps: per_channel 0: host_rows is
 * [n_taps], one row for the range; 1: [count][n_taps], a row per channel; row[k] is w[k].  Queued like a store. */
int dspfx_cancel_load(dspfx_cancel *a, const float *host_rows, uint32_t n_taps, uint32_t per_channel, uint64_t first_channel, uint64_t count);
/* Removes the node of the channels of the range: a copy again, and a later set makes a new node.  Queued like a store. */
int dspfx_cancel_drop(dspfx_cancel *a, uint64_t first_channel, uint64_t count);
/* Weights and history of the channels of the range back to +0.0; T, mu, eps, delay and adapt stay.  Queued like a store.  Also the
 * way out for a channel whose weights became NaN. */
int dspfx_cancel_reset(dspfx_cancel *a, uint64_t first_channel, uint64_t count);
/* The host tables over [first_channel, first_channel + count), as all stores made so far left them: present 1 / 0; lengths T, 0
 * without a node; sliders [count][2], mu and eps (0, 0 without a node); delays D; adapting 1 / 0. */
int dspfx_cancel_present(dspfx_cancel *a, uint32_t *host_present_out, uint64_t first_channel, uint64_t count);
int dspfx_cancel_lengths(dspfx_cancel *a, uint32_t *host_lengths_out, uint64_t first_channel, uint64_t count);
int dspfx_cancel_sliders(dspfx_cancel *a, float *host_sliders_out, uint64_t first_channel, uint64_t count);
int dspfx_cancel_delays(dspfx_cancel *a, uint32_t *host_delays_out, uint64_t first_channel, uint64_t count);
int dspfx_cancel_adapting(dspfx_cancel *a, uint32_t *host_adapting_out, uint64_t first_channel, uint64_t count);
/* The device pointer of the weights, float [max_taps][N], row k = w[k] of every channel, +0.0 in the rows k >= a channel's T.  The
 * pointer never changes; what it holds is valid after a run, on its stream. */
int dspfx_cancel_weights_view(dspfx_cancel *a, const float **weights_out);
/* The device pointer of the levels, float [2][N]: sum d * d and sum e * e of the last run, +0.0 without a node. */
int dspfx_cancel_levels_view(dspfx_cancel *a, const float **levels_out);

/* ---- channel generators: a bank of per-channel Signal Generators -------------------------------------------------------
 * An engine runs one Signal Generator (nodes/signal_gen.rs) with one amplitude, frequency and mode for all N channels.  This bank
 * gives channel c ONE generator of its own, with its own sliders, mode and clock, over N channels in the desc's layout
 * (tile_channels as dspfx_engine_desc).  It is a SOURCE that lives on the device: a run reads no signal block unless the caller has
 * the sample added into one.  A line-check tone for one participant, a join beep in one listener's return, a hold tone for the
 * channels in no room, an LFO of its own rate per channel feeding an engine's control port.
 * A node EXISTS for a channel from the first dspfx_gens_set that names it until dspfx_gens_drop; a fresh bank has no node anywhere.
 * A fresh node is the reference's (signal_gen.rs:40-52): amplitude 0.5, frequency 100, mode Sine, clock +0.0.
 * PER CHANNEL.  Amplitude, frequency, a mode (DSPFX_SIG_*) and the clock, the phase carried between blocks.  Values are taken as
 * given, as dspfx_set_param takes them: no clamp, NaN, infinities and values outside the slider's range included.
 * STORES.  dspfx_gens_set keeps the sliders and the mode it leaves out where the channel carries a node, and starts from the
 * defaults where it carries none.  A channel that carries a node keeps its CLOCK through any set (the reference has no
 * after_settings_change here); a channel that carried none, or was dropped, starts at clock +0.0.  A mode outside DSPFX_SIG_SINE ..
 * DSPFX_SIG_CONSTANT or a range past the channels refuses the WHOLE store: DSPFX_ERR_INVALID, the reason in dspfx_gens_last_error,
 * nothing stored.
 * ONE RUN: queued stores go onto the stream in the order they were made, then per channel:
 *   - The sample is bit for bit what an engine whose chain is that one Signal Generator, with link_flags = 0, writes for the
 *     channel over the same sequence of block lengths: the bank calls the engine's own device functions.  Square compares the
 *     block-local total, not the phase, with 0.5, as the reference does.
 *   - Without add_to, out[f][c] is the sample; a channel without a node gets +0.0 (an unconnected port, node.rs:162-194).
 *   - With add_to, a block in the bank's layout, out[f][c] = add_to[f][c] + sample by one f32 addition (add.rs); a channel without
 *     a node gets add_to's very bits.  out may be add_to.
 *   - BLOCKS.  The run's frames are cut into the reference's blocks of DSPFX_BUF_SIZE frames from frame 0.  At every block end, and
 *     at the end of a run that stops inside a block, clock = fmodf(clock + total, 1) and total = 0, as the engine does.  Constant
 *     leaves the clock alone (signal_gen.rs:106-108).
 *   - CONTROL PORTS.  amplitude and frequency are optional device blocks in the bank's layout, the reference's `as_input` slider
 *     ports (dsp-stuff-derive/src/lib.rs:135-153): where one is given, a channel's slider value for sample f is the block's value
 *     mapped from [-1, 1] onto the slider's range, -1 .. 1 for the amplitude and 0.1 .. 20000 for the frequency, per sample.
 *     Channels without a node read neither block.
 *     KNOWN DIFFERENCE from the reference: the bank does NOT latch a block's first value into the slider.  A port here is
 *     connected per call, not wired: a later run without the block uses what the stores left.
 *   - No link hops: the bank is link_flags = 0.
 * The kernel has the shape of the shaper bank's: a lane owns four adjacent channels (one when the layout or the alignment forbids
 * it), frames go in chunks with the next chunk's loads of add_to and the control blocks issued ahead of the arithmetic, stores are
 * nontemporal.  The modes differ per lane, so a wave ballots once per run for the modes its lanes carry and runs, per chunk, the
 * body of each mode that is present, wave-uniformly, keeping each result under a select: a wave of one mode pays for one body, a
 * wave without a Sine channel never evaluates the f64 sine, a wave without a node does no arithmetic.  The clocks are read once and
 * written once per run.  A channel's output is the same bits in either layout, with add_to in place or not, on any stream, and
 * whatever its neighbours carry.  No atomics, no LDS.
 * Memory: 13 bytes per channel of tables on the device (amplitude, frequency, clock and a mode / presence byte; dspfx_gens_plan),
 * 9 on the host. */
/* dspfx_gens_modes: the channel carries no node */
#define DSPFX_GENS_NONE 0xFFFFFFFFu
typedef struct dspfx_gens dspfx_gens;
typedef struct dspfx_gens_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t n_channels;      /* N */
    uint32_t max_frames;      /* largest n_frames a run will pass (>= 1) */
    uint32_t tile_channels;   /* 0 = frame-major; W = channel-tiled, as dspfx_engine_desc */
} dspfx_gens_desc;
/* PURE HOST function (no GPU, no bank): *bytes_out = the device bytes of a bank's tables, 13 * channels.  channels of 0 or above
 * 2^32 - 256: DSPFX_ERR_INVALID, the reason in dspfx_gens_last_error(NULL). */
int dspfx_gens_plan(uint64_t channels, uint64_t *bytes_out);
/* A bad descriptor (channels of 0 or above 2^32 - 256, a tile that is not a power of two dividing n_channels, another ABI version,
 * max_frames of 0) is DSPFX_ERR_INVALID with the reason in dspfx_gens_last_error of a NULL bank (kept per thread); all of that is
 * checked before any device work. */
int dspfx_gens_create(const dspfx_gens_desc *desc, dspfx_gens **out);
int dspfx_gens_destroy(dspfx_gens *g);
/* The reason of the bank's last failed call; of a NULL bank: of this thread's last failed create or plan. */
const char *dspfx_gens_last_error(const dspfx_gens *g);
/* out: a device block of n_frames frames in the desc's layout (1 <= n_frames <= max_frames).  add_to, amplitude, frequency: device
 * blocks of the same shape, each may be NULL (see ONE RUN).  out == add_to works in place (a thread rewrites the elements it read);
 * any other overlap is the caller's error.  Asynchronous on `stream`; a run on another stream than the one before first waits (on
 * the device) for that one (the rules of dspfx_strips_run).  Queued stores go onto the stream ahead of the kernel, in the order they
 * were made. */
int dspfx_gens_run(dspfx_gens *g, const float *add_to, const float *amplitude, const float *frequency, float *out, uint32_t n_frames,
                   void *stream);
/* Gives channels [first_channel, first_channel + count) a generator, from host arrays of `count` values each: the amplitudes, the
 * frequencies and the modes (DSPFX_SIG_*).  Each may be NULL: kept where the channel carries a node, the default (0.5, 100, Sine)
 * where it carries none.  The contract of dspfx_dynamics_set: callable from any thread while runs are in flight, never waits for the
 * device or for a run; the values are staged in page-locked memory and queued, each store is whole, and a run submitted after the
 * call returns sees it, the runs submitted before it do not. */
int dspfx_gens_set(dspfx_gens *g, const float *host_amplitude, const float *host_frequency, const uint32_t *host_mode, uint64_t first_channel,
                   uint64_t count);
/* Removes the node of channels [first_channel, first_channel + count): +0.0 (or add_to's bits) again, and a later set starts from
 * the defaults and from clock +0.0.  Queued like a store.  A range past the channels: DSPFX_ERR_INVALID and the reason. */
int dspfx_gens_drop(dspfx_gens *g, uint64_t first_channel, uint64_t count);
/* Sets the clocks of the channels of the range that carry a node to +0.0; sliders, modes and nodes stay.  Queued like a store. */
int dspfx_gens_reset(dspfx_gens *g, uint64_t first_channel, uint64_t count);
/* The host tables over [first_channel, first_channel + count), as all stores made so far left them: present 1 / 0 (the channel
 * carries a node); modes the DSPFX_SIG_* value, DSPFX_GENS_NONE without a node; sliders [count][2], amplitude then frequency, 0
 * without a node. */
int dspfx_gens_present(dspfx_gens *g, uint32_t *host_present_out, uint64_t first_channel, uint64_t count);
int dspfx_gens_modes(dspfx_gens *g, uint32_t *host_modes_out, uint64_t first_channel, uint64_t count);
int dspfx_gens_sliders(dspfx_gens *g, float *host_sliders_out, uint64_t first_channel, uint64_t count);
/* The device pointer of clock[N], f32: +0.0 for a channel without a node.  The pointer never changes; what it holds is valid after
 * a run, on its stream. */
int dspfx_gens_clocks(dspfx_gens *g, const float **clock_out);

/* ---- channel blends: a bank of per-channel Add and Mix nodes, and buses back into channels -----------------------------
 * An engine runs an Add (nodes/add.rs) or a Mix node (nodes/mix.rs) with one ratio for all N channels and one N-channel side
 * block.  This bank gives channel c ONE two-input node of its own -- none, Add, or Mix with its own ratio -- over N channels in the
 * desc's layout (tile_channels as dspfx_engine_desc), and an optional Gain node (gain.rs) on the node's `b` input: the channel's
 * SEND level, as the reference would wire b -> Gain -> Add.  Per-participant wet/dry after an echo, a shaper or the convolver; each
 * room's reverberated bus added back into its members' returns; an announcement bus (n_buses = 1) into everybody's; a crossfade of
 * a channel between two sources by a control block.
 * PER CHANNEL.  A node (none / Add / Mix), the Mix node's ratio, the send (absent, or a level) and a bus id in [0, n_buses) or
 * DSPFX_BLENDS_NO_BUS.  A fresh bank has no node, no send and DSPFX_BLENDS_NO_BUS everywhere: it copies a.  A new Mix node's ratio
 * is dspfx_node_defaults' 0.5.  Values are taken as given, as dspfx_set_param takes them: no clamp, NaN, infinities and values
 * outside the slider's range included.  The send EXISTS from the first dspfx_blends_set_send that names the channel until a
 * set_send without levels or dspfx_blends_drop; a send on a channel without a node is kept and does nothing.
 * ONE RUN: queued stores go onto the stream in the order they were made, then per channel c and frame f
 *   - THE SECOND INPUT.  b, an N-channel block in the bank's layout: b[f][c].  Or bus, a [n_frames][n_buses] frame-major block (what
 *     dspfx_mixgroups_run, dspfx_convolve_run and a frame-major engine of n_buses channels write): bus[f][bus_of[c]], +0.0 for a
 *     channel on DSPFX_BLENDS_NO_BUS.  With neither, +0.0: an unconnected port (node.rs:288), as an engine's Add or Mix without a
 *     side block.
 *   - bb = the second input, times the send's level by one f32 multiplication where the channel has a send.
 *   - Add: out = a + bb.  Mix: out = (bb * r) + (a * (1.0f - r)), in this order and never fused (mix.rs:45).  No node: a's very
 *     bits, NaN payloads included.  Every weight is a multiplication, never an omission: Mix at r = 0 with b = inf gives NaN.
 *     A channel's sample is bit for bit what an engine whose chain is that one node, with link_flags = 0, writes for it from the
 *     same a and side block: the bank uses the engine's expressions.
 *   - THE CONTROL PORT.  ratio is an optional device block in the bank's layout, the Mix node's `as_input` port
 *     (dsp-stuff-derive/src/lib.rs:135-153): where given, a Mix channel's r for sample f is the block's value mapped from [-1, 1]
 *     onto 0 .. 1, per sample.  Add channels and channels without a node do not read it.
 *     KNOWN DIFFERENCE from the reference, as dspfx_gens_run's: the bank does NOT latch the block's first value into the slider.  A
 *     later run without the block uses the stored ratio.
 *   - No link hops: the bank is link_flags = 0.
 * The kernel has the shape of the generator bank's: a lane owns four adjacent channels (one when the layout or the alignment forbids
 * it), frames go in chunks with the next chunk's loads issued ahead of the arithmetic, stores are nontemporal.  The kinds run under
 * per-channel selects.  A lane none of whose channels carries a node reads neither b, the bus nor the control block.  In bus mode every
 * channel gathers its own bus[f][bus_of[c]] from the small bus block, which stays in L2.  A channel's output is the same bits in either layout, in place or not, on any stream, and whatever its
 * neighbours carry.  No atomics, no LDS.
 * Memory: 13 bytes per channel of tables on the device (ratio, send level, bus id and a kind / presence byte;
 * dspfx_blends_plan), 13 on the host. */
/* dspfx_blends_assign, dspfx_blends_bus_of: the channel reads no bus */
#define DSPFX_BLENDS_NO_BUS 0xFFFFFFFFu
/* dspfx_blends_kinds: the channel carries no node */
#define DSPFX_BLENDS_NONE 0xFFFFFFFFu
typedef struct dspfx_blends dspfx_blends;
typedef struct dspfx_blends_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t n_channels;      /* N */
    uint32_t max_frames;      /* largest n_frames a run will pass (>= 1) */
    uint32_t tile_channels;   /* 0 = frame-major; W = channel-tiled, as dspfx_engine_desc */
    uint32_t n_buses;         /* G: the channels of a run's bus block; 0: the bank takes none */
} dspfx_blends_desc;
/* PURE HOST function (no GPU, no bank): *bytes_out = the device bytes of a bank's tables, 13 * channels.  channels of 0 or above
 * 2^32 - 256: DSPFX_ERR_INVALID, the reason in dspfx_blends_last_error(NULL). */
int dspfx_blends_plan(uint64_t channels, uint64_t *bytes_out);
/* A bad descriptor (channels of 0 or above 2^32 - 256, a tile that is not a power of two dividing n_channels, another ABI version,
 * max_frames of 0) is DSPFX_ERR_INVALID with the reason in dspfx_blends_last_error of a NULL bank (kept per thread); all of that is
 * checked before any device work. */
int dspfx_blends_create(const dspfx_blends_desc *desc, dspfx_blends **out);
int dspfx_blends_destroy(dspfx_blends *b);
/* The reason of the bank's last failed call; of a NULL bank: of this thread's last failed create or plan. */
const char *dspfx_blends_last_error(const dspfx_blends *b);
/* a, out: device blocks of n_frames frames in the desc's layout (1 <= n_frames <= max_frames).  side: a block of the same shape, or
 * NULL; bus: a device block [n_frames][n_buses], or NULL; ratio: a block of a's shape, or NULL (see ONE RUN).  Both side and bus,
 * bus on a bank of n_buses = 0, or n_frames of 0 or above max_frames: DSPFX_ERR_INVALID and the reason, before any device work and
 * with the queued stores still queued.  out == a and out == side work in place (a thread rewrites the elements it read); any other
 * overlap is the caller's error.  Asynchronous on `stream`; a run on another stream than the one before first waits (on the device)
 * for that one (the rules of dspfx_strips_run).  Queued stores go onto the stream ahead of the kernel, in the order they were
 * made. */
int dspfx_blends_run(dspfx_blends *b, const float *a, const float *side, const float *bus, const float *ratio, float *out, uint32_t n_frames,
                     void *stream);
/* Gives channels [first_channel, first_channel + count) a Mix node, from a host array of `count` ratios.  NULL: the ratio is kept
 * where the channel carries a Mix node, and is the default 0.5 where it carries none or an Add node.  The send and the bus id
 * stay.  The contract of dspfx_gens_set: callable from any thread while runs are in flight, never waits for the device or for a
 * run; the values are staged in page-locked memory and queued, each store is whole, and a run submitted after the call returns sees
 * it, the runs submitted before it do not.  A range past the channels refuses the WHOLE store: DSPFX_ERR_INVALID, the reason in
 * dspfx_blends_last_error, nothing stored.  The same holds for every store below. */
int dspfx_blends_set_mix(dspfx_blends *b, const float *host_ratio, uint64_t first_channel, uint64_t count);
/* ... an Add node.  The send and the bus id stay. */
int dspfx_blends_set_add(dspfx_blends *b, uint64_t first_channel, uint64_t count);
/* Gives the channels a send, a Gain node on the node's second input, from a host array of `count` levels; NULL removes it. */
int dspfx_blends_set_send(dspfx_blends *b, const float *host_level, uint64_t first_channel, uint64_t count);
/* Stores the bus ids of the channels from a host array of `count` ids, each below n_buses or DSPFX_BLENDS_NO_BUS; any other id
 * refuses the whole store. */
int dspfx_blends_assign(dspfx_blends *b, const uint32_t *host_ids, uint64_t first_channel, uint64_t count);
/* Removes the node and the send of the channels: a copy of a again, and a later set_mix starts from the default.  The bus id
 * stays.  Queued like a store. */
int dspfx_blends_drop(dspfx_blends *b, uint64_t first_channel, uint64_t count);
/* The host tables over [first_channel, first_channel + count), as all stores made so far left them: kinds DSPFX_ADD, DSPFX_MIX or
 * DSPFX_BLENDS_NONE; ratios the Mix node's, 0 for every other channel; sends the level and, in a presence array of its own, 1 / 0
 * (a level may be any value, NaN included, so no value can stand for "absent"; the level of an absent send reads 0); bus_of the id
 * or DSPFX_BLENDS_NO_BUS. */
int dspfx_blends_kinds(dspfx_blends *b, uint32_t *host_kinds_out, uint64_t first_channel, uint64_t count);
int dspfx_blends_ratios(dspfx_blends *b, float *host_ratios_out, uint64_t first_channel, uint64_t count);
int dspfx_blends_sends(dspfx_blends *b, float *host_levels_out, uint32_t *host_present_out, uint64_t first_channel, uint64_t count);
int dspfx_blends_bus_of(dspfx_blends *b, uint32_t *host_ids_out, uint64_t first_channel, uint64_t count);

/* ---- mix matrix: each listener's own mix of their room ---------------------------------------------------------------
 * dspfx_mixgroups_returns gives every listener of a room the same mix of the others, with one fader per SOURCE.  In the
 * reference every participant has an Output node of their own and wires it to whichever of the others they like through Gain
 * nodes of their own (nodes/output.rs:215-249, node.rs:162-194, gain.rs:25-38): "A mutes B for themself only", "C turns D up"
 * and "nearer people are louder" are all a gain per (listener, source) pair.  This bank holds that pair table.
 * Rooms are contiguous channel ranges given as dspfx_mixgroups_create takes them (group_start, G + 1 indices); room r has
 * 1 <= n_r <= DSPFX_MIXMATRIX_MAX_ROOM members and owns an n_r x n_r f32 matrix M_r[l][s] (listener l, source s, room-local
 * indices).  For a device block x of n_frames frames in the desc's layout (tile_channels as dspfx_engine_desc):
 *       out[f][c0 + l] = (sum over s in [0, n_r) of M_r[l][s] * x[f][c0 + s]) / d[c0 + l]
 * normalise = 1: d = dspfx_link_divisor(w), w = the WIRED entries of the listener's row, an entry being wired when it is not
 * +-0.0; one IEEE f32 division.  A row without a wired entry gives +0.0 whatever the samples are, as dspfx_mixgroups_returns
 * does in a room of one.  normalise = 0 writes the raw sum (and still +0.0 for a row without a wired entry).  A fresh bank
 * holds mix-minus in every room -- 1.0 off the diagonal, +0.0 on it -- so it is dspfx_mixgroups_returns of a bank without
 * faders, up to the order of summation.
 * KNOWN DIFFERENCE from the reference: a wire through a Gain node of level 0 counts in the reference's divisor and not here.  A
 * caller who needs that uses normalise = 0 and scales the rows.
 * Non-finite samples: unwired entries are multiplications by zero, not omissions, so a NaN or an infinity in a source reaches
 * every listener OF ITS OWN ROOM (0 * inf = NaN), and no listener of another room: sources outside the room are never read.
 * Arithmetic: v_mfma_f32_32x32x2_f32, which is bit for bit an f32 fmaf chain: a listener's sources are added in ascending
 * room-local order into one chain (then zero terms up to n_r rounded up to 32), so the result is within
 *       (n_r + 2) 2^-24 (sum over s of |M[l][s] x[s]|) / d + 2^-149
 * of the exact value, and a room's output bits are a function of its own matrix, its own samples and n_r alone: the same from
 * run to run, on any stream, in either layout, for any n_frames, and whatever the other rooms hold.  No atomics.
 * Memory: the matrices are kept source-major with edges padded to a multiple of 32: 4 * sum over the rooms of
 * (n_r rounded up to 32)^2 bytes (dspfx_mixmatrix_plan gives it; 1 GiB for 4096 rooms of 256), 8 bytes per channel beside it.
 * A bank made by dspfx_mixmatrix_create has fixed rooms.  A host that reseats participants live (dspfx_mixgroups_assign) makes
 * the bank with dspfx_mixmatrix_create_seats and follows every move with dspfx_mixmatrix_assign (below): no table is rebuilt and
 * the gains of those who stay are kept.  Rooms above the limit, sparse tables and reduced precision are not offered. */
#define DSPFX_MIXMATRIX_MAX_ROOM 1024
/* dspfx_mixmatrix_assign: the channel sits in no room */
#define DSPFX_MIXMATRIX_NO_ROOM 0xFFFFFFFFu
/* dspfx_mixmatrix_fill presets: 1.0 off the diagonal and +0.0 on it; all +0.0 */
#define DSPFX_MIXMATRIX_MIX_MINUS 0
#define DSPFX_MIXMATRIX_ZERO 1
typedef struct dspfx_mixmatrix dspfx_mixmatrix;
typedef struct dspfx_mixmatrix_desc {
    uint32_t abi_version;     /* DSPFX_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    uint32_t n_channels;      /* N */
    uint32_t max_frames;      /* largest n_frames a run will pass (>= 1) */
    uint32_t tile_channels;   /* 0 = frame-major; W = channel-tiled, as dspfx_engine_desc */
    uint32_t n_groups;        /* G >= 1 rooms */
    uint32_t normalise;       /* 1: divide by the link divisor of the listener's wired count; 0: the raw sums */
    const uint64_t *group_start; /* host, [n_groups + 1], read at create and copied: room g is channels [group_start[g],
                                 group_start[g + 1]); increasing, [0] = 0, [G] = N; every room has 1 .. 1024 members */
} dspfx_mixmatrix_desc;
/* PURE HOST function (no GPU, no bank): checks a table as create does and gives, per room, count_out[g] = n_g, edge_out[g] =
 * n_g rounded up to 32 (the edge of its padded table) and offset_out[g] = the element offset of its table, and
 * *total_bytes_out = the bytes of all tables.  Each of the four may be NULL.  A table that decreases, does not start at 0 or end
 * at n_channels, an empty room, a room above DSPFX_MIXMATRIX_MAX_ROOM, or a tile that is not a power of two dividing
 * n_channels: DSPFX_ERR_INVALID, the reason in dspfx_mixmatrix_last_error(NULL). */
int dspfx_mixmatrix_plan(const uint64_t *group_start, uint32_t n_groups, uint64_t n_channels, uint32_t tile_channels,
                         uint32_t *count_out, uint32_t *edge_out, uint64_t *offset_out, uint64_t *total_bytes_out);
/* A bad descriptor (what dspfx_mixmatrix_plan refuses, another ABI version, max_frames of 0) is DSPFX_ERR_INVALID with the
 * reason in dspfx_mixmatrix_last_error of a NULL bank (kept per thread); all of that is checked before any device work. */
int dspfx_mixmatrix_create(const dspfx_mixmatrix_desc *desc, dspfx_mixmatrix **out);
int dspfx_mixmatrix_destroy(dspfx_mixmatrix *m);
/* The reason of the bank's last failed call; of a NULL bank: of this thread's last failed create or plan. */
const char *dspfx_mixmatrix_last_error(const dspfx_mixmatrix *m);
/* block, out: device blocks of n_frames frames in the desc's layout (1 <= n_frames <= max_frames).  out may NOT overlap block:
 * a room's inputs are all needed after its first outputs exist, so there is no in-place form; an overlap is DSPFX_ERR_INVALID
 * and nothing is launched (a seated bank in DSPFX_MIXMATRIX_STAGED, below, takes out == block).  Asynchronous on `stream`; a run on another stream than the one before first waits (on the device)
 * for that one (the rules of dspfx_mixgroups_run).  Queued stores go onto the stream ahead of the kernel, in the order they
 * were made. */
int dspfx_mixmatrix_run(dspfx_mixmatrix *m, const float *block, uint32_t n_frames, float *out, void *stream);
/* What listeners [first_channel, first_channel + count) hear: host_values is [count][row_len], row i = M[l][0 .. n_r) of
 * listener first_channel + i.  All listeners must be in ONE room and row_len must be that room's n_r; otherwise, or with a range
 * past the channels, DSPFX_ERR_INVALID, the reason in dspfx_mixmatrix_last_error, nothing stored.  The contract of
 * dspfx_mixgroups_set_gains: callable from any thread while runs are in flight, never waits for the device or for a run; the
 * values are copied into a page-locked staging buffer and queued, and the next run applies the queued stores in order, each
 * whole: a run submitted after the call returns sees the new values, the runs submitted before it the old ones.  The wired
 * counts and divisors of the listeners touched are recomputed on the device behind the store. */
int dspfx_mixmatrix_set_rows(dspfx_mixmatrix *m, const float *host_values, uint32_t row_len, uint64_t first_channel, uint64_t count);
/* How loud sources [first_channel, first_channel + count) are: host_values is [count][row_len], row i = M[0 .. n_r)[s] of
 * source first_channel + i, one value per listener of its room (a source fader, or muting someone for everybody).  Rules,
 * threading and ordering as dspfx_mixmatrix_set_rows. */
int dspfx_mixmatrix_set_cols(dspfx_mixmatrix *m, const float *host_values, uint32_t row_len, uint64_t first_channel, uint64_t count);
/* Room `room` (-1: every room) back to a preset, DSPFX_MIXMATRIX_MIX_MINUS or DSPFX_MIXMATRIX_ZERO; queued like a store. */
int dspfx_mixmatrix_fill(dspfx_mixmatrix *m, int64_t room, uint32_t preset);
/* The fresh state: mix-minus in every room; queued like a store. */
int dspfx_mixmatrix_reset(dspfx_mixmatrix *m);
/* Gains by channel number, for both kinds of bank: M[listeners[i]][sources[i]] = gains[i] for i in [0, count), in that order, so
 * a later duplicate wins ("A mutes B" needs no seat lookup).  Each pair must be two channels of ONE room (by the seating so far);
 * otherwise DSPFX_ERR_INVALID, the reason, nothing stored.  Queued like every other store; the divisors of the rooms touched are
 * recounted behind it. */
int dspfx_mixmatrix_set_pairs(dspfx_mixmatrix *m, const uint32_t *listeners, const uint32_t *sources, const float *gains, uint64_t count);

/* ---- seated banks: participants change rooms live -----------------------------------------------------------------------
 * dspfx_mixmatrix_create_seats makes a bank whose room r owns S_r SEATS: seats[r] rounded up to 32, n_r <= S_r <=
 * DSPFX_MIXMATRIX_MAX_ROOM (a value below n_r or above the limit is DSPFX_ERR_INVALID with the reason in
 * dspfx_mixmatrix_last_error(NULL), before any device work).  The room's table is S_r x S_r and its memory never changes after
 * create; a channel holds one seat of one room, or none.  At first channel c0 + i of room r sits in seat i and the table holds
 * mix-minus among the taken seats; every entry in the row or the column of an empty seat is +0.0, and every store keeps it so.
 * For a channel c in seat l of room r, with chan_r(s) the channel in seat s:
 *       out[f][c] = (sum over the taken seats s of M_r[l][s] * x[f][chan_r(s)]) / d[c]
 * d, w and normalise as above.  A channel in no room reads +0.0 in every frame whatever it carries; its samples are never read.
 * The sources are added in ascending SEAT order into one fmaf chain with a +0.0 * +0.0 term at every empty seat: the chain of
 * a dspfx_mixmatrix_create room of S_r contiguous members whose absent members carry +0.0 samples and zero rows and columns, bit
 * for bit.  A room's bits are a function of its table, its samples and its seat arrangement alone; the error bound is the one
 * above with n = the taken seats (zero terms are exact).
 * Memory: 4 * sum of S_r^2 bytes of tables (dspfx_mixmatrix_plan_seats), 4 bytes per seat and 12 per channel on the device (the
 * last 4 are the channel -> seat table of the staged run, below), and 4 bytes per seat and 8 per channel on the host.
 * Stores on a seated bank: set_rows / set_cols take lines of row_len = S_r values indexed by SEAT; the channels named must all
 * sit in one room by the seating so far (in any seats of it); a value given for an empty seat is stored as +0.0.
 * dspfx_mixmatrix_fill with DSPFX_MIXMATRIX_MIX_MINUS means 1.0 between two different taken seats. */
int dspfx_mixmatrix_create_seats(const dspfx_mixmatrix_desc *desc, const uint32_t *seats /* host, [n_groups] */, dspfx_mixmatrix **out);
/* PURE HOST function: dspfx_mixmatrix_plan for a seated bank: edge_out[g] = S_g, the offsets and the bytes of S_g x S_g tables. */
int dspfx_mixmatrix_plan_seats(const uint64_t *group_start, uint32_t n_groups, uint64_t n_channels, uint32_t tile_channels, const uint32_t *seats,
                               uint32_t *count_out, uint32_t *edge_out, uint64_t *offset_out, uint64_t *total_bytes_out);
/* Seats channels [first_channel, first_channel + count) in the rooms host_room_ids (each < n_groups, or
 * DSPFX_MIXMATRIX_NO_ROOM).  DSPFX_ERR_STATE on a bank not made by dspfx_mixmatrix_create_seats.  The contract of
 * dspfx_mixgroups_assign: the range, every id and every room's capacity are checked before anything is stored
 * (DSPFX_ERR_INVALID, the reason, nothing changed); callable from any thread while runs are in flight; never waits for the device
 * or for a run; holds, whole, for every run submitted after it returns and for none submitted before.  Queued in order with the
 * other stores.
 * THE SEATING RULE.  A channel whose id is its current room is untouched: it keeps its seat and its gains.  All other named
 * channels first LEAVE: their seat is free, its row and column in the old room's table become +0.0.  Then the channels that
 * enter a room do so in ascending channel order, each into the LOWEST FREE SEAT of its new room (so two participants can swap
 * between two full rooms in one call, and somebody who comes back gets the lowest free seat, not the old one).
 * The newcomer's wiring, by the seating after the whole call: DSPFX_MIXMATRIX_MIX_MINUS: 1.0 in the newcomer's row at every
 * other taken seat and in their column for every other seated listener, +0.0 on the diagonal; DSPFX_MIXMATRIX_ZERO: row and
 * column +0.0 (the host then stores its own).  Entries between two participants who both stayed are never touched.  The
 * divisors of every listener of a room somebody left or entered are recounted on the device.
 * Cost: O(count + the seats of the rooms entered) on the host, one row and one column per mover on the device. */
int dspfx_mixmatrix_assign(dspfx_mixmatrix *m, const uint32_t *host_room_ids, uint64_t first_channel, uint64_t count, uint32_t preset);
/* The room (DSPFX_MIXMATRIX_NO_ROOM: none) and the seat (0xFFFFFFFF: none) of channels [first_channel, first_channel + count), and
 * the taken seats of every room ([n_groups]), by every call made so far.  A bank without seats answers by its table. */
int dspfx_mixmatrix_rooms(dspfx_mixmatrix *m, uint32_t *host_ids_out, uint64_t first_channel, uint64_t count);
int dspfx_mixmatrix_seats(dspfx_mixmatrix *m, uint32_t *host_seats_out, uint64_t first_channel, uint64_t count);
int dspfx_mixmatrix_occupancy(dspfx_mixmatrix *m, uint32_t *host_counts_out);
/* PURE HOST function: the seating rule on host arrays.  room_of_io[n_channels] and seat_of_io[n_channels] hold a seating of rooms
 * with seats[g] seats (rounded up to 32) and are changed as dspfx_mixmatrix_assign changes the bank's; the same checks, the reason
 * in dspfx_mixmatrix_last_error(NULL), nothing changed on a refusal.  dspfx_mixmatrix_assign uses the same code. */
int dspfx_mixmatrix_reseat(uint32_t *room_of_io, uint32_t *seat_of_io, const uint32_t *seats, uint32_t n_groups, uint64_t n_channels,
                           const uint32_t *room_ids, uint64_t first_channel, uint64_t count);

/* ---- seated banks: the staged run, whose cost does not depend on the seating -----------------------------------------------
 * The direct run gathers: it reads x[f][chan_r(s)] for 32 seats at a time, one lane per seat, and in either layout a channel's
 * consecutive frames are a whole row apart, so the only locality it can have is between seats whose CHANNEL NUMBERS are
 * adjacent.  At the seating create gives, a chunk of 32 seats is one line per frame; once participants have wandered it is up
 * to 32 lines per frame for 32 useful words, read again by every listener tile and paid again by the stores.  Ordering a room's
 * seats by channel would not help: what counts is whether the members are neighbouring channels, not the order they sit in
 * (and a new order would change the room's summation order, and so its bits).
 * DSPFX_MIXMATRIX_STAGED runs three kernels instead: mixmatrix_stage_in reads the block once, coalesced, and writes every seated
 * channel's frames contiguously into its seat's row of a seat-ordered copy; the same MFMA chain runs over that copy, reading
 * and writing along frames; mixmatrix_stage_out transposes the result back and writes +0.0 for the channels in no room.  Every
 * pass moves whole lines whatever the seating, and the accumulator chain is the direct run's term for term -- ascending seat
 * order, +0.0 at empty seats, whose stale rows are never read -- so a room's bits are the same in both modes.  The mode costs
 * four more passes over the block; dspfx_mixmatrix_scatter says when that is the cheaper way (DESIGN.md §8 has the figures).
 * Memory: two copies of (sum of S_r) x max_frames f32, allocated by the first switch to STAGED and kept until destroy
 * (dspfx_mixmatrix_staging_bytes; 1 GiB + 4 MiB for 4096 rooms of 256 seats and 128 frames).  The channel -> seat table the
 * transposes go by (4 bytes per channel) is kept by every seated bank from create on, in order with the assigns. */
#define DSPFX_MIXMATRIX_DIRECT 0
#define DSPFX_MIXMATRIX_STAGED 1
/* The mode of the runs submitted after the call returns; a run is wholly one mode.  Any thread, while runs are in flight; never
 * waits for the device or for a run.  DSPFX_ERR_STATE on a bank not made by dspfx_mixmatrix_create_seats; an unknown mode is
 * DSPFX_ERR_INVALID and changes nothing.  The first switch to DSPFX_MIXMATRIX_STAGED allocates the copies on the calling thread;
 * if that fails the call is DSPFX_ERR_OOM and the mode is unchanged.  The memory is never zeroed and never freed before
 * destroy.
 * dspfx_mixmatrix_run in staged mode: the same contract, except that out == block (the very same pointer) is allowed: every
 * read of the block is finished before the first write of out.  A partial overlap is still refused, and so is any overlap in
 * direct mode. */
int dspfx_mixmatrix_set_staging(dspfx_mixmatrix *m, uint32_t mode);
int dspfx_mixmatrix_staging(dspfx_mixmatrix *m, uint32_t *mode_out);
/* PURE HOST function: the bytes DSPFX_MIXMATRIX_STAGED adds to a seated bank of this plan (checked as dspfx_mixmatrix_plan_seats
 * checks it): 2 * (sum of S_r) * max_frames * 4 for the two copies, and 4 * n_channels for the channel -> seat table. */
int dspfx_mixmatrix_staging_bytes(const uint64_t *group_start, uint32_t n_groups, uint64_t n_channels, uint32_t tile_channels, const uint32_t *seats,
                                  uint32_t max_frames, uint64_t *bytes_out);
/* PURE HOST function: how scattered a seating is -- "is it time to turn staging on?".  room_of[n_channels], seat_of[n_channels]
 * and seats[n_groups] as dspfx_mixmatrix_reseat takes them (the same checks).  Every run of 32 consecutive seats of a room that
 * holds at least one channel is a CHUNK of the direct run, and the distinct values of channel / 32 among its channels are the
 * LINES the chunk reads per frame in a layout whose rows are 128-byte aligned: *chunks_out and *lines_out are the totals (either
 * may be NULL).  With rooms that begin at multiples of 32 the seating of create gives lines == chunks; a shuffled seating
 * approaches 32 lines per chunk. */
int dspfx_mixmatrix_scatter(const uint32_t *room_of, const uint32_t *seat_of, const uint32_t *seats, uint32_t n_groups, uint64_t n_channels,
                            uint64_t *chunks_out, uint64_t *lines_out);

/* ---- the sparse run: only a listed set of sources per room --------------------------------------------------------------
 * Behind a talker bank nearly every term of dspfx_mixmatrix_run is a multiplication by an exact zero.  This run reads only the
 * sources a list names.  list (int32_t channel numbers), start[G + 1] and count[G] are DEVICE pointers, G the bank's room count:
 * what dspfx_talkers_audible_views gives, or anything of that shape.
 * CONTRACT.  For room r let A_r be the set of room-local indices held by the channels in
 *       list[start[r] .. start[r] + min(count[r], DSPFX_MIXMATRIX_MAX_ROOM))
 * a room-local index being a member index c - c0 in a bank made by dspfx_mixmatrix_create and a seat in a seated one.  An entry
 * is IGNORED if it is negative, if it is >= N, if it lies at or past list_len, or if it names a channel that does not sit in room r;
 * duplicates count once; the order of a segment does not matter.  Then for every taken index l of the room
 *       out[f][chan(l)] = (fmaf chain from +0.0 over s in A_r, ascending s, of x[f][chan(s)] * Mt[s][l]) / d[chan(l)]
 * d, normalise, "a row without a wired entry gives +0.0", the channels in no room (+0.0) and the layouts are those of
 * dspfx_mixmatrix_run, and d still counts the WHOLE row's wired entries, listed or not.  A source outside A_r is NOT READ, whatever
 * it carries: the documented difference from the dense run, where an unlisted NaN still reaches its room.  An empty A_r gives +0.0
 * to every listener of the room.
 * BITS.  If every source of the room outside A_r carries +-0.0 and the room's matrix is finite, the result is the dense run's bit
 * for bit: fmaf(m, +-0.0, acc) == acc for finite m unless acc is -0.0; the chain starts at +0.0; an exact cancellation gives
 * +0.0; so the dense chain's unlisted steps are all the identity.  The one exception is the sign of a zero result when a non-zero
 * product has underflowed to -0.0 on the way.  With everybody listed it is the dense run on any block.  The error bound is the
 * dense run's with n = the listed sources.
 * MODES.  In DSPFX_MIXMATRIX_DIRECT out is written as the dense direct run writes it, out may not overlap the block, and the
 * channels in no room are zeroed as there.  In DSPFX_MIXMATRIX_STAGED the few listed sources are read straight from the block
 * (no mixmatrix_stage_in), the result goes to the seat-ordered copy and mixmatrix_stage_out writes out in whole lines whatever
 * the seating; out == block is allowed.  Queued stores drain first, as in dspfx_mixmatrix_run.  The caller orders the list's
 * producer and this run on one stream, or by an event, as for any device block.
 * The host checks the pointers, n_frames, the overlap and list_len (at most 2^32 - 1): DSPFX_ERR_INVALID, the reason, nothing
 * launched.  What the list holds is validated on the device, which never reads outside list[0 .. list_len), start[0 .. G] and
 * count[0 .. G): a bad list yields ignored entries, not an error.  LDS atomics only (an order-free OR); no global atomics. */
int dspfx_mixmatrix_run_sparse(dspfx_mixmatrix *m, const float *block, uint32_t n_frames, float *out, const int32_t *list, uint64_t list_len,
                               const uint32_t *start, const uint32_t *count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DSPFX_H */
