"""Edge-value parity on the GPU: NaN, infinities, signed zeros, subnormals, the clip points and the fast f64 functions'
switch points (tests/edge_values.py) through every chain-kernel family, the BASELINE chains' two kernels, a generated graph
kernel, control ports and the documented state clearings, against the CPU oracle through the strict comparison
`same_values` (NaN pattern, signed infinities, the sign of every zero, then the project's existing ulp bars).  Every test
asserts, through `classes_present` on the oracle's output, that the classes it is about were really compared."""
import numpy as np
import pytest

import graph_eval
import graphs
import oracle as O
from chains import chain3, chain5, ulp_diff
from edge_values import classes_present, edge_block, is_subnormal, same_bits_or_nan, same_values
from test_gpu_parity import LIBM_COMPOSITE_ULP, LIBM_ULP, _every_node, noise_block, run_gpu, run_oracle, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
B = 128
BLOCKS = 3
LEVEL = 3.0          # _every_node's distort level: the clip and switch-point classes are placed for it
SPECIAL = {"nan", "+inf", "-inf", "-0"}


def node_bar(dspfx, node):
    """The project's existing bars: 0 for Gain / Add / Reverb / Envelope (bit-exact today), LIBM_ULP for the three
    math-library distort modes, LIBM_COMPOSITE_ULP where a math-library result feeds further f32 operations, else 1."""
    if node.kind in (dspfx.GAIN, dspfx.ADD, dspfx.REVERB, dspfx.ENVELOPE):
        return 0
    if node.kind == dspfx.DISTORT and node.mode in LIBM_ULP:
        return LIBM_ULP[node.mode]
    if node.kind in (dspfx.OVERDRIVE, dspfx.CHEBYSHEV) or (node.kind == dspfx.SIGNAL_GEN and node.mode == dspfx.SIG_SINE):
        return LIBM_COMPOSITE_ULP
    return 1


def stage_lines(dspfx, N, chain, lf=3, tile=0):
    eng = dspfx.Engine(N, B, link_flags=lf, tile_channels=tile)
    eng.set_chain(chain)
    lines = [l for l in eng.describe().splitlines() if l.startswith("stage")]
    eng.close()
    return lines


_blocks, _refs, _interp = {}, {}, {}


def blocks_for(N):
    """The edge block and the side-input edge block (another seed) for N channels, made once."""
    if N not in _blocks:
        x, table = edge_block(N, B * BLOCKS, LEVEL)
        side, _ = edge_block(N, B * BLOCKS, LEVEL, seed=0x5EED0E02)
        _blocks[N] = (x, side, table)
    return _blocks[N]


def oracle_for(nodes, k, N, lf):
    """The oracle's output for node k alone, computed once per (node, N, link flags) and left unchanged."""
    if (k, N, lf) not in _refs:
        x, side, _ = blocks_for(N)
        ref = run_oracle([nodes[k]], x, lf, side)
        ref.setflags(write=False)
        _refs[(k, N, lf)] = ref
    return _refs[(k, N, lf)]


# name -> (environment, N, tile, what the stage line must / must not contain)
FAMILIES = {
    "interpreter": ({"DSPFX_JIT": "0"}, 100, 0, ["fused kernel dyn", "CPL=1"], ["jit_"]),
    "interpreter_tiled": ({"DSPFX_JIT": "0"}, 128, 64, ["fused kernel dyn", "CPL=1"], ["jit_"]),
    "dyn_f8_c1": ({"DSPFX_VARIANT": "static=0,f=8,cpl=1"}, 100, 0, ["fused kernel dyn", "F=8, CPL=1"], ["jit_"]),
    "dyn_f8_c2": ({"DSPFX_VARIANT": "static=0,f=8,cpl=2"}, 418, 0, ["fused kernel dyn", "_c2", "F=8, CPL=2"], ["jit_"]),
    # no compiled-in specialisation of a one-node chain exists: static=1 falls back to the two-channel interpreter for the
    # single nodes; the compiled-in kernels themselves (s3h / s5h / s3n / s5n) run the BASELINE chains below
    "static_f8_c2": ({"DSPFX_VARIANT": "static=1,f=8,cpl=2"}, 418, 0, ["_c2", "F=8, CPL=2"], ["jit_"]),
    "jit": ({"DSPFX_JIT": "1"}, 418, 0, ["fused kernel jit_"], []),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_node_in_every_kernel_family(dspfx, torch_cuda, monkeypatch, family):
    """Each node of `_every_node` alone on the edge block (side input: an edge block of another seed, so Add / Mix see
    NaN + finite and inf + -inf), link flags 0 (the sign of a zero lives to the output) and 3 (the `0.0 + x` hop turns -0.0
    into +0.0), through one kernel family: parity with the oracle at the node's existing bar through `same_values`, and
    the interpreter's bits (NaN by isnan).  100 channels = 64 in the main launch + 36 in the guarded tail; 418 = 384 + 34 for
    two channels per lane; 128 with 64-channel tiles for the tiled layout.  The edge channels sit at both ends."""
    env, N, tile, must, must_not = FAMILIES[family]
    exact, libm = _every_node(dspfx)
    nodes = exact + libm
    x, side, table = blocks_for(N)
    seen = {}
    for k, node in enumerate(nodes):
        for lf in (0, 3):
            ref = oracle_for(nodes, k, N, lf)
            what = "%s kind %d mode %d lf %d" % (family, node.kind, node.mode, lf)
            if (k, N, tile, lf) not in _interp:
                for name in ("DSPFX_VARIANT", "DSPFX_JIT"):
                    monkeypatch.delenv(name, raising=False)
                monkeypatch.setenv("DSPFX_JIT", "0")
                assert "fused kernel dyn" in stage_lines(dspfx, N, [node], lf, tile)[0]
                _interp[(k, N, tile, lf)] = run_gpu(dspfx, torch_cuda, [node], x, lf, side=side, tile=tile)
            base = _interp[(k, N, tile, lf)]
            monkeypatch.delenv("DSPFX_JIT", raising=False)
            for name, value in env.items():
                monkeypatch.setenv(name, value)
            line = stage_lines(dspfx, N, [node], lf, tile)[0]
            assert all(m in line for m in must) and not any(m in line for m in must_not), (what, line)
            got = run_gpu(dspfx, torch_cuda, [node], x, lf, side=side, tile=tile)
            for name in env:
                monkeypatch.delenv(name, raising=False)
            same_values(got, ref, node_bar(dspfx, node), table, what)
            same_bits_or_nan(got, base, table, what + " against the interpreter")
            seen.setdefault((node.kind, node.mode), set()).update(classes_present(ref))
    everything = set().union(*seen.values())
    assert SPECIAL <= everything, everything
    for key in ((dspfx.GAIN, 0), (dspfx.LOW_PASS, 0), (dspfx.DISTORT, dspfx.HARD_CLIP)):
        assert "subnormal" in seen[key], (key, seen[key])


@pytest.mark.parametrize("which", ["chain3", "chain5"])
def test_compiled_in_kernels_on_the_edge_block(dspfx, torch_cuda, monkeypatch, which):
    """The compiled-in specialisations exist for the BASELINE chains only: `static=1,f=8,cpl=2` with the time-sliced kernel
    switched off runs s3?_f8_c2 / s5?_f8_c2 itself (418 channels: 384 + 34 in the guarded tail), for both link-flag
    settings, against the oracle and the interpreter's bits."""
    N = 418
    x, _, table = blocks_for(N)
    chain = chain3(dspfx, 128) if which == "chain3" else chain5(dspfx, 128)
    seen = set()
    for lf in (0, 3):
        monkeypatch.setenv("DSPFX_VARIANT", "static=0,ts=0")      # the interpreter: no compiled-in kernel, no time slices
        monkeypatch.setenv("DSPFX_TS_TAIL", "0")
        line = stage_lines(dspfx, N, chain, lf)[0]
        assert "fused kernel dyn" in line and "time-sliced" not in line and "left over" not in line, line
        base = run_gpu(dspfx, torch_cuda, chain, x, lf)
        monkeypatch.delenv("DSPFX_TS_TAIL")
        monkeypatch.setenv("DSPFX_VARIANT", "static=1,f=8,cpl=2,ts=0")
        line = stage_lines(dspfx, N, chain, lf)[0]
        name = ("s3" if which == "chain3" else "s5") + ("h" if lf else "n") + "_f8_c2"
        assert "fused kernel " + name in line and "time-sliced" not in line, line
        got = run_gpu(dspfx, torch_cuda, chain, x, lf)
        monkeypatch.delenv("DSPFX_VARIANT")
        ref = run_oracle(chain, x, lf)
        same_values(got, ref, 1, table, "%s %s" % (name, which))
        same_bits_or_nan(got, base, table, name + " against the interpreter")
        seen |= classes_present(ref)
    # (chain5's SoftClip sends NaN down its last arm, to -2/3: the first biquad's NaN state never shows at the output)
    assert ({"nan", "+inf", "subnormal"} if which == "chain3" else {"subnormal"}) <= seen, seen


@pytest.mark.parametrize("N,tile", [(64 * 5 + 5, 0), (256, 64)])
@pytest.mark.parametrize("which", ["chain3", "chain5"])
def test_time_sliced_and_standard_kernel_on_the_edge_block(dspfx, torch_cuda, monkeypatch, which, N, tile):
    """The BASELINE chains with a short delay on the time-sliced kernel (carried state crosses waves through LDS: a NaN or
    inf state must travel like any other bits) and on the standard one: the two agree bit for bit, both match the oracle
    within 1 ulp in the strict sense."""
    x, _, table = blocks_for(N)
    chain = chain3(dspfx, 128) if which == "chain3" else chain5(dspfx, 128)
    ref = run_oracle(chain, x, 3)
    outs = {}
    for ts in ("1", "0"):
        monkeypatch.setenv("DSPFX_VARIANT", "ts=" + ts)
        line = stage_lines(dspfx, N, chain, 3, tile)[0]
        assert ("time-sliced" in line) == (ts == "1"), line
        outs[ts] = run_gpu(dspfx, torch_cuda, chain, x, 3, tile=tile)
        monkeypatch.delenv("DSPFX_VARIANT")
        same_values(outs[ts], ref, 1, table, "%s ts=%s N=%d tile=%d" % (which, ts, N, tile))
    same_bits_or_nan(outs["1"], outs["0"], table, "time-sliced against standard")
    # (chain5's SoftClip sends NaN down its last arm, to -2/3: the first biquad's NaN state never shows at the output)
    assert ({"nan", "+inf", "subnormal"} if which == "chain3" else {"subnormal"}) <= classes_present(ref), classes_present(ref)


def test_generated_graph_kernel_on_the_edge_block(dspfx, torch_cuda):
    """The diamond (fan-out, a two-link fan-in into the distort, a two-link fan-in into the Output node) fed the edge block:
    the generated whole-graph kernel and the run-by-run evaluation against the reference-semantics evaluation on the
    oracle, within the graph tests' 1 ulp in the strict sense, and bit for bit against each other.  The fan-in averages see
    inf + -inf and NaN + finite."""
    from dsp_stuff_amd import graph as G
    N = 128
    x, _, table = blocks_for(N)
    outs = {}
    for fused in (True, False):
        ge = G.GraphEngine(graphs.diamond(), N, B, fused=fused)
        assert ("jit_graph" in ge.describe()) == fused, ge.describe()
        got = np.empty_like(x)
        for f0 in range(0, len(x), B):
            y = ge.process(torch_cuda.from_numpy(x[f0:f0 + B]).cuda(), B)
            torch_cuda.cuda.synchronize()
            got[f0:f0 + B] = y.cpu().numpy().reshape(B, N)
        if fused:
            ref = graph_eval.run_graph(ge.g, x)
        ge.close()
        outs[fused] = got
        same_values(got, ref, 1, table, "diamond, fused=%s" % fused)
    same_bits_or_nan(outs[True], outs[False], table, "one kernel against run by run")
    assert {"nan", "-0", "subnormal"} <= classes_present(ref), classes_present(ref)     # (inf + -inf and inf through a biquad: NaN)


def test_fuzz_on_the_edge_block(dspfx, torch_cuda):
    """Fuzz's three block-global maxima restate max_by(f32::total_cmp): one NaN or one infinity in a 128-frame block of a
    channel makes that whole block NaN, and only that one (so does a peak of 3.4e38, whose products overflow).  The NaN pattern per channel and block is exact; where the
    reference is finite, test_fuzz's bar applies per channel and block (4e-6 x the block's peak)."""
    N = 100
    x, _, table = blocks_for(N)
    chain = [dspfx.Distort(LEVEL, dspfx.FUZZ)]
    for lf in (0, 3):
        got, ref = run_gpu(dspfx, torch_cuda, chain, x, lf), run_oracle(chain, x, lf)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan), (lf, np.argwhere(np.isnan(got) != nan)[:4])
        for b in range(BLOCKS):
            sl = slice(b * B, (b + 1) * B)
            assert np.array_equal(nan[sl].all(axis=0), nan[sl].any(axis=0))                  # whole blocks of a channel, or none
            poisoned = {c for c in range(N) if nan[sl, c].all()}
            nonfinite = {c for c, n in table.items() if n in ("inf", "inf_pair", "nan")}      # (written into block 1 only)
            assert poisoned <= set(table) and (nonfinite <= poisoned if b == 1 else not (nonfinite & poisoned)), (b, poisoned)
            for c in range(N):
                if c in poisoned:
                    continue
                err, peak = np.abs(got[sl, c].astype(np.float64) - ref[sl, c]).max(), np.abs(ref[sl, c]).max()
                assert np.isfinite(got[sl, c]).all() and err <= 4e-6 * peak, (lf, b, c, table.get(c, "noise"), err, peak)
        assert "nan" in classes_present(ref)


def test_libm_modes_at_the_switch_points_against_correct_rounding(dspfx, torch_cuda):
    """Tanh / Sin / Atan on the edge block (the tanh clamp at 20, the hand-over to the library sin at 2^22, huge arguments),
    GPU and glibc each against the correctly rounded value (numpy's float64 function of the f32 argument, rounded once).
    Bounds: the GPU evaluates in f64 and rounds once, so it can miss the correctly rounded f32 only where the f64 error
    crosses a rounding boundary: <= 1 ulp; glibc's f32 routines are within LIBM_ULP of it (DESIGN.md's libm table).  The
    distances are printed per mode and class before they are asserted."""
    N = 100
    x, _, table = blocks_for(N)
    f64 = {dspfx.TANH: np.tanh, dspfx.SIN: np.sin, dspfx.ATAN: np.arctan}
    for mode, fn in f64.items():
        chain = [dspfx.Distort(LEVEL, mode)]
        got, ref = run_gpu(dspfx, torch_cuda, chain, x, 0), run_oracle(chain, x, 0)
        with np.errstate(all="ignore"):
            arg = (x * F(LEVEL)).astype(F)
            cr = fn(arg.astype(np.float64)).astype(F)
        worst = {}
        for c in range(N):
            name = table.get(c, "noise")
            fin = np.isfinite(cr[:, c])
            g, r = ulp_diff(got[fin, c], cr[fin, c]).max(), ulp_diff(ref[fin, c], cr[fin, c]).max()
            w = worst.setdefault(name, [0, 0])
            w[0], w[1] = max(w[0], int(g)), max(w[1], int(r))
        print("libm distances to correct rounding, mode %d: {class: [gpu, glibc]} = %r" % (mode, worst))
        same_values(got, cr, 1, table, "GPU against correct rounding, mode %d" % mode)
        same_values(ref, cr, LIBM_ULP[mode], table, "glibc against correct rounding, mode %d" % mode)
        assert {"tanh_clamp_20", "sin_handover_2p22", "large"} <= set(worst)


# ---------------------------------------------------------------- containment and recovery

def _poisoned_input(N, blocks):
    x = noise_block(N, B * blocks, seed=0x5EED0E03)
    xp = x.copy()
    xp[10, 5], xp[11, 5] = np.inf, -np.inf          # a channel of the main launch
    xp[20, 80] = np.nan                             # a channel of the guarded tail
    return x, xp, [5, 80]


def _containment_chain(dspfx):
    return [dspfx.BiQuad(), dspfx.Reverb(delay_samples=128, decay=0.5), dspfx.LowPass(0.3), dspfx.Envelope(12.0, 300.0)]


@pytest.mark.parametrize("mix_tail", [None, "0", "1"])
def test_poison_stays_in_its_channel_and_on_the_mix_bus(dspfx, torch_cuda, monkeypatch, mix_tail):
    """+inf followed by -inf, and one NaN, injected in block 0 into two channels (one of them in the guarded tail), six
    blocks: every other channel equals, bit for bit, a run without the poison; the poisoned channels follow the oracle's
    NaN pattern frame by frame (the biquad state stays NaN, the ring hands it back every 128 frames); the mix bus of the
    same call is NaN exactly in the frames where the oracle's f64 channel sum is, and keeps test_ragged_channel_counts'
    bar elsewhere -- with DSPFX_MIX_TAIL unset, 0 and 1."""
    if mix_tail is not None:
        monkeypatch.setenv("DSPFX_MIX_TAIL", mix_tail)
    N, blocks = 100, 6
    x, xp, bad = _poisoned_input(N, blocks)
    chain = _containment_chain(dspfx)
    clean, _ = run_gpu(dspfx, torch_cuda, chain, x, want_mix=True)
    got, mix = run_gpu(dspfx, torch_cuda, chain, xp, want_mix=True)
    ref = run_oracle(chain, xp)
    others = [c for c in range(N) if c not in bad]
    assert np.array_equal(got[:, others].view(np.uint32), clean[:, others].view(np.uint32))
    assert np.isfinite(got[:, others]).all()
    same_values(got, ref, 1, {5: "inf_pair", 80: "nan"}, "containment")
    assert np.isnan(ref[B * 5:, bad]).all() and not np.isnan(ref[:10, bad]).any()           # the poison really stays for good
    want = ref.astype(np.float64).sum(axis=1)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(mix), nan), np.flatnonzero(np.isnan(mix) != nan)[:8]
    assert 0 < nan.sum() < len(nan)
    assert np.allclose(mix[~nan], want[~nan], rtol=1e-5, atol=1e-4)


def _drive(dspfx, torch, eng, x, b):
    dx = torch.from_numpy(x[b * B:(b + 1) * B]).cuda()
    dy = torch.empty_like(dx)
    eng.process(dx, out=dy, n_frames=B)
    torch.cuda.synchronize()
    return dy.cpu().numpy()


@pytest.mark.parametrize("clearing", ["reset", "biquad_store", "reverb_store"])
def test_documented_clearings_remove_the_poison(dspfx, torch_cuda, clearing):
    """eng.reset(), a biquad coefficient store (zeroes the filter state) and a Reverb slider store (swaps in a zero ring)
    after two poisoned blocks: the next blocks equal the oracle's after the same operation.  reset() clears the whole
    chain, so the poisoned channels are finite again; a store clears its own node, shown finite on that node alone.
    State that still holds NaN after a documented clearing is a bug (a reset that scales state by zero keeps NaN)."""
    N = 100
    x, xp, bad = _poisoned_input(N, 4)
    if clearing == "reset":
        chains = [_containment_chain(dspfx)]
    elif clearing == "biquad_store":
        chains = [_containment_chain(dspfx), [dspfx.BiQuad()]]
    else:
        chains = [_containment_chain(dspfx), [dspfx.Reverb(delay_samples=128, decay=0.5)]]
    for chain in chains:
        eng = dspfx.Engine(N, B)
        eng.set_chain(chain)
        descs = [n.oracle_desc() for n in chain]
        nodes = []
        for b in range(2):
            got = _drive(dspfx, torch_cuda, eng, xp, b)
            ref = O.run_channels(descs, xp[b * B:(b + 1) * B], 3, nodes_out=nodes)
            same_values(got, ref, 1, what="%s before, block %d" % (clearing, b))
        assert np.isnan(ref[:, bad]).any()
        k = 0 if clearing != "reverb_store" or len(chain) == 1 else 1
        if clearing == "reset":
            eng.reset()
            for chn in nodes:
                for n in chn:
                    n.reset()
        elif clearing == "biquad_store":
            eng.set_param(k, 3, 0.758)
            for chn in nodes:
                chn[k].set_param(3, 0.758)
        else:
            eng.set_param(k, 0, 0.4)
            for chn in nodes:
                chn[k].set_param(0, 0.4)
        for b in range(2, 4):
            got = _drive(dspfx, torch_cuda, eng, xp, b)
            ref = O.run_channels(descs, xp[b * B:(b + 1) * B], 3, nodes_out=nodes)
            same_values(got, ref, 1, {5: "inf_pair", 80: "nan"}, "%s after, block %d, %d nodes" % (clearing, b, len(chain)))
            if clearing == "reset" or len(chain) == 1:
                assert np.isfinite(ref).all() and np.isfinite(got).all(), (clearing, b)
        eng.close()


def test_poisoned_state_survives_export_and_import(dspfx, torch_cuda):
    """state_export of every node of the poisoned chain, imported into a fresh engine: both continue identically (NaN
    state is state like any other)."""
    N = 100
    x, xp, bad = _poisoned_input(N, 4)
    chain = _containment_chain(dspfx)
    a, b = dspfx.Engine(N, B), dspfx.Engine(N, B)
    a.set_chain(chain)
    b.set_chain(chain)
    for k in range(2):
        _drive(dspfx, torch_cuda, a, xp, k)
    assert np.isnan(a.state_export(0).view(np.float32)).any()
    for k in range(len(chain)):
        b.state_import(k, a.state_export(k))
    for k in range(2, 4):
        ya, yb = _drive(dspfx, torch_cuda, a, xp, k), _drive(dspfx, torch_cuda, b, xp, k)
        assert np.isnan(ya[:, bad]).any()
        same_bits_or_nan(yb, ya, what="imported state, block %d" % k)
    a.close()
    b.close()


# ---------------------------------------------------------------- control ports

def test_control_ports_fed_edge_values(dspfx, torch_cuda):
    """test_control_ports' chain A with control signals that are edge blocks scaled by 1.5 (NaN, +-inf, values outside
    [-1, 1], +-0): the mapped slider (`f32::clamp(0.0, 1.0)`: NaN stays NaN) and the per-channel latch of each block's first
    value match the oracle in the strict sense -- a NaN latch keeps applying after the port is disconnected, until a slider
    store overwrites it."""
    N, blocks = 96, 6
    x, side = noise_block(N, B * blocks), noise_block(N, B * blocks, seed=5)
    sigs = []
    for s in range(4):
        c, table = edge_block(N, B * blocks, LEVEL, seed=0x5EED0E10 + s)
        sigs.append((c * F(1.5)).astype(F))
    chain = [dspfx.Gain(1.0), dspfx.Distort(3.0, dspfx.HARD_CLIP), dspfx.Mix(0.5), dspfx.BiQuad(), dspfx.Distort(2.0, dspfx.SOFT_CLIP)]
    ctl_all = {(0, 0): sigs[0], (1, 0): sigs[1], (2, 0): sigs[2], (4, 0): sigs[3]}
    keys = list(ctl_all)
    eng = dspfx.Engine(N, B, link_flags=3)
    eng.set_chain(chain)
    descs = [n.oracle_desc() for n in chain]
    nodes = []
    dev = {k: torch_cuda.from_numpy(v).cuda() for k, v in ctl_all.items()}
    dx, ds = torch_cuda.from_numpy(x).cuda(), torch_cuda.from_numpy(side).cuda()
    dy = torch_cuda.empty_like(dx)
    ref = np.empty_like(x)

    def run(b, ks):
        sl = slice(b * B, (b + 1) * B)
        eng.process(dx[sl], out=dy[sl], side=ds[sl], n_frames=B, ctl={k: dev[k][sl] for k in ks} or None)
        ref[sl] = O.run_channels(descs, x[sl], 3, side[sl], ctl={k: ctl_all[k][sl] for k in ks} or None, nodes_out=nodes)

    run(0, keys)
    run(1, keys)                                # block 1 starts with an edge value in every edge channel: that is latched
    run(2, keys[1:2])                           # the others disconnected: their latched per-channel values apply
    run(3, [])
    nan_latched = np.isnan(ref[3 * B:4 * B]).all(axis=0)
    eng.set_param(0, 0, 0.7)                    # a slider store overwrites the latch
    for chn in nodes:
        chn[0].set_param(0, 0.7)
    run(4, [])
    run(5, keys[-1:])
    torch_cuda.cuda.synchronize()
    same_values(dy.cpu().numpy(), ref, 1, table, "control ports")
    assert nan_latched.any() and not nan_latched.all()                                   # a NaN latch kept applying ...
    assert {"nan"} <= classes_present(ref[:4 * B]) and np.isnan(ref[B:2 * B]).any()
    gain_nan = np.isnan(sigs[0][B])                                                       # ... in the channels whose gain port latched NaN
    assert gain_nan.any() and nan_latched[gain_nan].all()


def test_fuzz_level_port_fed_edge_values(dspfx, torch_cuda):
    """test_fuzz_level_control_port's pattern, frame-major layout, with an edge block scaled by 1.5 on the level port: the
    NaN pattern is exact, the finite part keeps that test's bar."""
    N, blocks = 96, 5
    x = noise_block(N, B * blocks)
    sig, table = edge_block(N, B * blocks, LEVEL, seed=0x5EED0E20)
    sig = (sig * F(1.5)).astype(F)
    chain = [dspfx.Gain(0.9), dspfx.Distort(3.0, dspfx.FUZZ), dspfx.BiQuad()]
    eng = dspfx.Engine(N, B, link_flags=3)
    eng.set_chain(chain)
    descs = [n.oracle_desc() for n in chain]
    nodes = []
    got, ref = np.empty_like(x), np.empty_like(x)

    def run(b, connected):
        sl = slice(b * B, (b + 1) * B)
        dx, dc = torch_cuda.from_numpy(x[sl]).cuda(), torch_cuda.from_numpy(sig[sl]).cuda()
        dy = torch_cuda.empty_like(dx)
        eng.process(dx, out=dy, n_frames=B, ctl={(1, 0): dc} if connected else None)
        torch_cuda.cuda.synchronize()
        got[sl] = dy.cpu().numpy()
        ref[sl] = O.run_channels(descs, x[sl], 3, ctl={(1, 0): sig[sl]} if connected else None, nodes_out=nodes)

    run(0, True)
    run(1, True)
    run(2, False)
    eng.set_param(1, 0, 2.5)
    for chn in nodes:
        chn[1].set_param(0, 2.5)
    run(3, False)
    run(4, True)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), np.argwhere(np.isnan(got) != nan)[:4]
    assert 0 < nan.mean() < 0.5
    fin = ~nan
    assert np.abs(got[fin] - ref[fin]).max() <= 4e-6 * np.abs(ref[fin]).max(), np.abs(got[fin] - ref[fin]).max()


# ---------------------------------------------------------------- subnormal tails

def test_subnormal_tails_are_not_flushed(dspfx, torch_cuda):
    """An impulse decaying through the subnormal range, bit-exact against the oracle, link flags 0: a kernel compiled to
    flush denormals fails here and nowhere else in the suite.  LowPass(0.5) and HighPass(0.5) answer a unit impulse with
    0.5^n: 23 subnormal samples per channel before zero.  BiQuad()'s defaults decay by 0.24 per frame -- eleven frames
    across the subnormal range -- and Gain(0.5) eight times over only scales by 2^-8, so a unit impulse gives those two
    fewer than twenty subnormal samples (none for the gains): their impulse is 1.5 x 2^-(100 + c) in channel c, which puts
    the tails of the channels at different depths.  Each case asserts at least 20 distinct nonzero subnormal samples in the
    reference output."""
    N, nf = 64, 256
    unit = np.zeros((nf, N), F)
    unit[0] = 1.0
    scaled = np.zeros((nf, N), F)
    scaled[0] = F(1.5) * np.exp2(-(100.0 + np.arange(N))).astype(F)
    for name, chain, x in (("low_pass", [dspfx.LowPass(0.5)], unit), ("high_pass", [dspfx.HighPass(0.5)], unit),
                           ("biquad", [dspfx.BiQuad()], scaled), ("gain x 8", [dspfx.Gain(0.5)] * 8, scaled)):
        got, ref = run_gpu(dspfx, torch_cuda, chain, x, 0), run_oracle(chain, x, 0)
        sub = is_subnormal(ref)
        n_distinct = len(np.unique(ref[sub].view(np.uint32)))
        if x is unit:
            assert sub[:, 0].sum() >= 20, (name, int(sub[:, 0].sum()))
        assert n_distinct >= 20, (name, n_distinct)
        assert (ref[-1] == 0).all(), name                                               # ... before it reaches zero
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (name, np.argwhere(got.view(np.uint32) != ref.view(np.uint32))[:4])
