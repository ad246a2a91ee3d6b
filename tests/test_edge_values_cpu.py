"""Edge values on the CPU: known answers read off the reference's own lines (nodes/distort.rs:53-172 and Rust's documented
signum / copysign / powi / total_cmp) against the C oracle, and the two restatements of the reference -- the C oracle and
the numpy model -- against each other on the edge block of tests/edge_values.py, sign of zero and NaN pattern included."""
import numpy as np
import pytest

import numpy_model as M
import oracle as O
from edge_values import CLASS_NAMES, classes_present, edge_block, edge_channels, same_values

F = np.float32
INF, NAN = F(np.inf), F(np.nan)
TINY = F(2.0 ** -149)


def bits(v):
    return np.asarray(v, F).view(np.uint32)


def distort(mode, values, level=2.0):
    return O.Node(O.DISTORT, [level], mode).process(np.asarray(values, F))


def check(got, want):
    """Bit for bit; NaN by isnan."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (got, want)
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), (got, want, bits(got), bits(want))


# ---------------------------------------------------------------- the helper itself

def test_the_comparator_sees_what_ulp_diff_does_not():
    from chains import ulp_diff
    a = np.array([[0.0, 1.0, np.inf, np.nan]], F)
    assert same_values(a, a.copy(), 0)
    assert ulp_diff(np.array([-0.0], F), np.array([0.0], F)).max() == 0            # the hole this comparator closes
    for k, v, why in ((0, -0.0, "sign of zero"), (2, -np.inf, "infinity"), (2, 3.4e38, "infinity"), (3, 1.0, "NaN pattern"),
                      (1, np.nan, "NaN pattern"), (1, np.nextafter(F(1), F(2)), "1 ulp")):
        b = a.copy()
        b[0, k] = v
        with pytest.raises(AssertionError, match=why):
            same_values(b, a, 0, table={0: "x", 1: "x", 2: "x", 3: "x"})
    b = a.copy()
    b[0, 1] = np.nextafter(F(1), F(2))
    assert same_values(b, a, 1)
    nan_other = a.copy()
    nan_other.view(np.uint32)[0, 3] = 0xFFC12345                                   # payload and sign of a NaN are not compared
    assert same_values(nan_other, a, 0)
    assert classes_present(np.array([0.0, 1.0], F)) == set()
    assert classes_present(np.array([-0.0, np.nan, np.inf, -np.inf, 1e-40], F)) == {"-0", "nan", "+inf", "-inf", "subnormal"}


def test_edge_block_layout():
    for N in (100, 418, 128, 24):
        x, table = edge_block(N, 384, 3.0)
        assert set(table.values()) == set(CLASS_NAMES)
        plain = O.noise(0x5EED0E01, np.arange(N), np.arange(384))
        for c in range(N):
            if c not in table:
                assert np.array_equal(x[:, c], plain[:, c])                         # the innocent neighbours
        if N >= 100:
            assert max(table) >= 64 and any(c % 2 == 0 for c in table) and any(c % 2 == 1 for c in table)
            for name in CLASS_NAMES:                                                # each class in both halves of a lane pair
                assert {c % 2 for c, n in table.items() if n == name} == {0, 1}, name
        nonfinite = {c for c in range(N) if not np.isfinite(x[:, c]).all()}
        assert nonfinite == {c for c, n in table.items() if n in ("inf", "inf_pair", "nan")}
        assert classes_present(x) == {"nan", "+inf", "-inf", "-0", "subnormal"}
    x, table = edge_block(100, 384, 3.0)
    assert edge_channels(100)[99] == table[99]
    c = [c for c, n in table.items() if n == "inf_pair"][0]
    f = np.flatnonzero(np.isposinf(x[:, c]))
    assert len(f) and np.isneginf(x[f[-1] + 1, c])                                  # +inf followed by -inf in the next frame
    c = [c for c, n in table.items() if n == "clip_level"][0]
    assert (np.abs(x[:, c]) * F(3.0) > 1).any() and ((np.abs(x[:, c]) * F(3.0) <= 1) & (np.abs(x[:, c]) > 0.33)).any()


# ---------------------------------------------------------------- (a) known answers, level 2.0 (every division exact)

def test_hard_clip_known_answers():
    got = distort(O.HARD_CLIP, [NAN, INF, -INF, 3.4e38, -0.0, TINY, -TINY])
    check(got, [NAN, 0.5, -0.5, 0.5, -0.0, TINY, -TINY])                            # a flushed subnormal would show as 0


def test_soft_clip_known_answers():
    two_thirds = F(2.0) / F(3.0)
    got = distort(O.SOFT_CLIP, [NAN, INF, -INF, -0.0, 0.0])
    # NaN fails `> 1.0` and `(-1.0..=1.0).contains` alike: the last arm, -2/3 (distort.rs:77-83); s - s^3/3 at -0 is (-0) - (-0) = +0
    check(got, [-two_thirds / F(2), two_thirds / F(2), -two_thirds / F(2), 0.0, 0.0])
    assert np.isfinite(got).all()


def test_recip_soft_clip_known_answers():
    check(distort(O.RECIP_SOFT_CLIP, [-0.0, 0.0, INF, -INF, NAN]), [-0.0, 0.0, 1.0, -1.0, NAN])


def test_square_known_answers():
    check(distort(O.SQUARE, [-0.0, 0.0, -TINY, TINY, -INF, INF, NAN]), [-0.0, 0.0, -0.0, 0.0, -INF, INF, NAN])


def test_chebyshev4_known_answers():
    check(distort(O.CHEBYSHEV4, [0.0, -0.0, INF, -INF, 3.4e38, F(1e15) / F(2)]), [1.0, 1.0, NAN, NAN, NAN, INF])


def test_libm_modes_at_infinity():
    from test_gpu_parity import LIBM_ULP
    from chains import ulp_diff
    check(distort(O.TANH, [INF, -INF]), [1.0, -1.0])
    assert np.isnan(distort(O.SIN, [INF, -INF])).all()
    got = distort(O.ATAN, [INF, -INF])
    assert ulp_diff(got, np.array([np.pi / 2, -np.pi / 2], F)).max() <= LIBM_ULP[O.ATAN] and got[0] > 0 > got[1]


@pytest.mark.parametrize("mode", [O.HARD_CLIP, O.SOFT_CLIP, O.TANH, O.RECIP_SOFT_CLIP, O.SIN, O.ATAN, O.SQUARE, O.CHEBYSHEV4])
def test_bypass_hands_every_edge_value_on(mode):
    """level < 0.001: `return sample` in every per-sample mode (Fuzz has no bypass)."""
    x, table = edge_block(len(CLASS_NAMES), 256, 3.0)
    for level in (0.0, 0.0009):
        for c in range(x.shape[1]):
            got = O.chain_run([O.Node(O.DISTORT, [level], mode)], x[:, c], 0)
            nan = np.isnan(x[:, c])
            assert np.array_equal(np.isnan(got), nan), (mode, table[c])
            assert np.array_equal(bits(got)[~nan], bits(x[:, c])[~nan]), (mode, table[c])


def test_fuzz_known_answers():
    """distort.rs:146-172: abs, then max_by(total_cmp) -- a NaN is the block's maximum, so one NaN sample makes the whole
    block NaN; one infinity makes mx = inf, every q = +-0, every z = -0, mz = 0 and y = clip(-0 * inf) / 0 = NaN; a silent
    block is 0 / 0."""
    base = O.noise(3, np.array([0]), np.arange(128))[:, 0]
    for poison in (NAN, np.array(0xFFC00001, np.uint32).view(F), INF, -INF):
        x = base.copy()
        x[77] = poison
        fz = O.Node(O.DISTORT, [3.0], O.FUZZ)
        assert np.isnan(fz.process(x)).all(), poison
        assert np.isfinite(fz.process(base)).all()                                  # Fuzz keeps no state: the next block is clean
    for zero in (0.0, -0.0):
        assert np.isnan(O.Node(O.DISTORT, [3.0], O.FUZZ).process(np.full(128, zero, F))).all()


# ---------------------------------------------------------------- (b) the two restatements agree on the edge block

def _nodes(dspfx):
    from test_gpu_parity import _every_node
    exact, libm = _every_node(dspfx)
    return exact, libm


def _platform_libm():
    """The platform's own f32 routines (what Rust's f32::tanh etc. and the C oracle call), vectorised for the numpy model."""
    import ctypes as C
    import ctypes.util
    lib = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")

    def unary(name):
        f = getattr(lib, name)
        f.restype, f.argtypes = C.c_float, [C.c_float]
        vec = np.frompyfunc(lambda v: f(float(v)), 1, 1)
        return lambda a: np.asarray(vec(np.asarray(a, F)), dtype=F)

    powf = lib.powf
    powf.restype, powf.argtypes = C.c_float, [C.c_float, C.c_float]
    return {"tanh": unary("tanhf"), "sin": unary("sinf"), "atan": unary("atanf"), "exp": unary("expf"), "sin_cr": unary("sinf"),
            "powf": lambda base, x: F(powf(float(F(base)), float(F(x))))}


def test_both_restatements_agree_on_the_edge_block(dspfx, monkeypatch):
    """The C oracle against the numpy model on the edge block, both link-flag settings, side input an edge block of another
    seed: the same values in the strict sense, bar 0.  Compared: every node of the GPU tests' `_every_node` -- Gain, BiQuad,
    LowPass, HighPass, Reverb, Add, Mix, the five arithmetic distort modes, SignalGen triangle / square / constant / sine,
    three Envelopes, distort Tanh / Sin / Atan, Overdrive, Chebyshev -- and Fuzz.  Not compared: FIR (it has its own
    non-finite tests).  The numpy model's math-library calls are pointed at the platform's f32 routines for this (the
    reference calls the platform's; numpy's own float32 tanh is 2 ulp from glibc's at some switch points), so for the
    math-library nodes what is compared is every line AROUND those calls.  That includes SignalGen's sine and the
    Envelope's powf, which the model by default takes correctly rounded: here they are glibc's sinf / powf."""
    monkeypatch.setattr(M, "LIBM", _platform_libm())
    N, nf = 2 * len(CLASS_NAMES) + 2, 384
    x, table = edge_block(N, nf, 3.0)
    side, _ = edge_block(N, nf, 3.0, seed=0x5EED0E02)
    exact, libm = _nodes(dspfx)
    seen = {}
    for node in exact + libm + [dspfx.Distort(3.0, dspfx.FUZZ)]:
        d = node.oracle_desc()
        for lf in (0, 3):
            ref = O.run_channels([d], x, lf, side)
            got = np.empty_like(ref)
            for c in range(N):
                got[:, c] = M.chain_run([M.make_node(d)], x[:, c], lf, side[:, c])
            same_values(got, ref, 0, table, what="numpy model against C oracle, kind %d mode %r lf %d" % (d["kind"], d.get("mode"), lf))
            seen.setdefault((d["kind"], d.get("mode") or 0), set()).update(classes_present(ref))
    everything = set().union(*seen.values())
    assert {"nan", "+inf", "-inf", "-0"} <= everything, everything
    for key in ((O.GAIN, 0), (O.LOW_PASS, 0), (O.DISTORT, O.HARD_CLIP)):
        assert "subnormal" in seen[key], (key, seen[key])
