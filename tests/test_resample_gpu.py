"""The output resampler bank on the GPU (dspfx_resample_*) against the numpy restatement in resample_ref.py.  Every comparison
is of raw bytes: the plan is shared (test_resample_cpu.py), and the device work is an f64 multiply, one rounding to f32, f32 adds
in a fixed order and the exact from_f32 rules -- none of it leaves room for a tolerance."""
import threading
import time

import numpy as np
import pytest

import resample_ref as R

pytestmark = pytest.mark.gpu

B = 128
F32, I16, U16, I32 = 0, 1, 2, 3
RATES = (8000, 22050, 44100, 48000, 96000, 192000)
NP_OUT = {F32: np.float32, I16: np.int16, U16: np.uint16, I32: np.int32}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def signal(frames, n, seed):
    """[frames][n] f32: uniform noise in [-1, 1]; channel 0 zeros, 1 and 2 full-scale DC, 3 one impulse, 4 past +-1.0"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (frames, n)).astype(np.float32)
    if n >= 5:
        x[:, 0] = 0.0
        x[:, 1] = 1.0
        x[:, 2] = -1.0
        x[:, 3] = 0.0
        x[min(200, frames - 1), 3] = 1.0
        x[:, 4] *= 3.0
    return x


def expected_bytes(dspfx, out_f32, tile, fmt, ch):
    """[n_out][N] f32 -> the bytes of the device buffer: the layout for n_out frames, each element `ch` samples of the format"""
    dev = R.to_device(out_f32, fmt, 1)
    flat = dspfx.to_layout(np.ascontiguousarray(dev), tile).reshape(-1)
    return np.repeat(flat, ch).view(np.uint8)


def got_bytes(torch, out):
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(-1).view(np.uint8)


class Pair:
    """a bank and its restatement, fed alike"""

    def __init__(self, dspfx, torch, n, hz, tile=0, fmt=F32, ch=1, slots=4, compare=None):
        """compare(pair, got bytes, want [n_out][N] f32), when given, takes the place of the byte comparison in pull"""
        self.dspfx, self.torch, self.n, self.tile, self.fmt, self.ch = dspfx, torch, n, tile, fmt, ch
        self.compare = compare
        self.bank = dspfx.Resampler(n, hz, tile_channels=tile, slots=slots, out_format=fmt, out_channels=ch)
        self.ref = R.Resampler(n, hz)
        self.fifo = np.zeros((0, n), np.float32)
        self.pulls = 0

    def push(self, x, via_slot=False):
        torch = self.torch
        blk = torch.from_numpy(self.dspfx.to_layout(x, self.tile).reshape(-1).copy()).cuda()
        if via_slot:
            slot = self.bank.slot_tensor()
            assert slot is not None and len(x) == B
            slot.copy_(blk)
            self.bank.push(slot, B)
        else:
            self.bank.push(blk, len(x))
        self.fifo = np.concatenate([self.fifo, x])

    def pull(self, n_out):
        out, used, under = self.bank.pull(n_out)
        want, consumed = self.ref.callback(self.fifo, n_out)
        if want is None:
            assert under and used == 0
            want = np.zeros((n_out, self.n), np.float32)
        else:
            assert not under and used == consumed, (used, consumed)
            self.fifo = self.fifo[consumed:]
        assert self.bank.available == len(self.fifo)
        got = got_bytes(self.torch, out)
        exp = expected_bytes(self.dspfx, want, self.tile, self.fmt, self.ch)
        assert got.shape == exp.shape
        if self.compare is not None:
            self.compare(self, got, want)
        elif not np.array_equal(got, exp):
            bad = np.nonzero(got != exp)[0]
            raise AssertionError(f"pull {self.pulls} (n_out {n_out}): {len(bad)} bytes differ, first at {bad[0]}")
        self.pulls += 1
        return used, under


def stream(p, x, n_outs, callbacks):
    """push 128-frame blocks of x while there is room (the slot path every other block), pull with the lengths of n_outs"""
    f, k = 0, 0
    cap = p.bank.slots * B
    for cb in range(callbacks):
        while p.bank.available + B <= cap and f + B <= len(x):
            p.push(x[f:f + B], via_slot=(k % 2 == 1))
            f += B
            k += 1
        p.pull(n_outs[cb % len(n_outs)])
    return f


@pytest.mark.parametrize("hz", RATES)
@pytest.mark.parametrize("n,tile", [(512, 0), (512, 256), (96, 32), (77, 0)])
def test_stream_of_callbacks_is_bit_identical(dspfx, torch_cuda, monkeypatch, hz, n, tile):
    """40 callbacks of varying length: warm-up from the first frame, pulls that start mid-slot, cross slots and wrap the FIFO,
    an underrun now and then (a long callback against a short FIFO), in frame-major and tiled layouts and at a ragged N"""
    monkeypatch.setenv("DSPFX_RESAMPLE_VEC", "1")            # 4 channels a lane wherever the layout allows (N = 77 cannot)
    per = max(1, int(B * hz / 48000))
    n_outs = [per, per - 1 if per > 1 else 1, per + 3, 1, 2 * per, per]
    x = signal(64 * B, n, seed=hz + n + tile)
    p = Pair(dspfx, torch_cuda, n, hz, tile)
    pushed = stream(p, x, n_outs, 40)
    assert p.pulls == 40 and pushed > 4 * 4 * B              # the FIFO (4 slots) wrapped several times


@pytest.mark.parametrize("fmt", [F32, I16, U16, I32])
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("n,tile,vec", [(512, 256, "1"), (512, 256, "0"), (512, 0, "1"), (77, 0, "1")])
def test_formats_and_device_channels(dspfx, torch_cuda, monkeypatch, fmt, ch, n, tile, vec):
    """every format and device channel count through both steady-state kernels: DSPFX_RESAMPLE_VEC (read at create) picks 4
    channels a lane or 1, which the bank otherwise chooses by N; a ragged N runs 1 a lane whatever it says"""
    monkeypatch.setenv("DSPFX_RESAMPLE_VEC", vec)
    x = signal(48 * B, n, seed=7 * fmt + ch)
    p = Pair(dspfx, torch_cuda, n, 44100, tile, fmt, ch)
    stream(p, x, [118, 117, 59, 200], 40)


def test_underrun_is_silence_and_changes_nothing(dspfx, torch_cuda):
    torch = torch_cuda
    n = 256
    x = signal(8 * B, n, seed=3)
    for fmt, ch in ((U16, 1), (U16, 2), (I16, 2), (F32, 1), (I32, 1)):
        p = Pair(dspfx, torch, n, 44100, 0, fmt, ch)
        used, under = p.pull(118)                             # nothing pushed yet
        assert under and used == 0
        if fmt == U16:
            out, _, _ = p.bank.pull(5)
            torch.cuda.synchronize()
            assert np.all(out.cpu().numpy().view(np.uint16) == 0x8000)
        p.push(x[:B])
        assert p.pull(118)[1] is False                        # input_len 128 == waiting 128
        p.push(x[B:B + 100])
        assert p.pull(118)[1] is True                         # short: silence, nothing consumed
        assert p.bank.available == len(p.fifo)
        p.push(x[B + 100:2 * B + 100])
        assert p.pull(118)[1] is False                        # ... and the later output is what it would have been


def test_exactly_short_view_feeds_one_zero(dspfx, torch_cuda):
    """44.1 kHz, 118 frames: the third callback wants 129 frames; with exactly input_len = 128 waiting, the last pull is 0.0
    and is not counted"""
    n = 64
    x = signal(3 * B, n, seed=5)
    p = Pair(dspfx, torch_cuda, n, 44100)
    p.push(x[:B])
    assert p.pull(118) == (127, False)
    p.push(x[B:2 * B - 1])                                    # 1 + 127 = 128 waiting
    assert p.pull(118) == (128, False)
    p.push(x[2 * B - 1:3 * B - 1])                            # exactly 128 waiting
    assert p.bank.available == 128
    assert p.pull(118) == (128, False)                        # the converter asked for 129
    assert p.bank.available == 0


def test_skip_reset_and_full_fifo(dspfx, torch_cuda):
    torch = torch_cuda
    n = 128
    x = signal(12 * B, n, seed=9)
    p = Pair(dspfx, torch, n, 44100, 32, I16, 2, slots=3)
    for k in range(3):
        p.push(x[k * B:(k + 1) * B])
    assert p.bank.slot() is None
    with pytest.raises(dspfx.DspfxError) as ei:               # full: DSPFX_ERR_STATE, nothing changed
        p.bank.push(torch.zeros(n, device="cuda"), 1)
    assert ei.value.status == -6 and p.bank.available == 3 * B
    first_used, _ = p.pull(118)
    with pytest.raises(dspfx.DspfxError):
        p.bank.skip(p.bank.available + 1)
    p.bank.skip(100)                                          # the catch-up primitive: the converter never sees them
    p.fifo = p.fifo[100:]
    p.pull(118)
    # reset reproduces the first callback
    p.bank.reset()
    p.ref.reset()
    p.fifo = p.fifo[:0]
    assert p.bank.available == 0
    for k in range(3):
        p.push(x[k * B:(k + 1) * B], via_slot=True)
    assert p.pull(118)[0] == first_used


def test_slot_and_copy_paths_agree(dspfx, torch_cuda):
    torch = torch_cuda
    n, hz = 512, 96000
    x = signal(8 * B, n, seed=11)
    outs = []
    for via_slot in (False, True):
        p = Pair(dspfx, torch, n, hz, 256)
        res = []
        for k in range(8):
            p.push(x[k * B:(k + 1) * B], via_slot=via_slot)
            out, used, under = p.bank.pull(256)
            res.append((got_bytes(torch, out).copy(), used, under))
        outs.append(res)
    for a, b in zip(*outs):
        assert a[1:] == b[1:] and np.array_equal(a[0], b[0])


@pytest.mark.parametrize("n,tile", [(96, 32), (77, 0)])
def test_pushes_that_straddle_slots_are_bit_identical(dspfx, torch_cuda, n, tile):
    """pushes of 1, 127, 128, 129, 5 and 250 frames: pieces that end inside a slot, start inside one, cross one and two slot
    boundaries and wrap the FIFO (tiled: rows of the block at a pitch of its own length into rows of the slot).  Every pull
    equals the restatement, and the pulls equal those of a second bank fed the same frames in whole 128-frame blocks"""
    lengths = (1, 127, 128, 129, 5, 250)
    x = signal(sum(lengths), n, seed=13 + n)
    cap = 4 * B

    def keep(pair, got, want):
        assert np.array_equal(got, expected_bytes(dspfx, want, pair.tile, pair.fmt, pair.ch)), pair.pulls
        pair.last = got.copy()

    def feed(pieces):
        p = Pair(dspfx, torch_cuda, n, 44100, tile, compare=keep)
        outs, f = [], 0

        def pull():
            used, under = p.pull(118)
            if not under:
                outs.append((p.last, used))
            return under

        for m in pieces:
            while p.bank.available + m > cap:
                assert not pull()
            p.push(x[f:f + m])
            f += m
        while not pull():
            pass
        assert f == len(x) and p.bank.available == len(p.fifo) < B
        return outs

    ragged = feed(lengths)
    whole = feed([B] * (len(x) // B))
    assert len(ragged) == len(whole) >= 4
    for k, (a, b) in enumerate(zip(ragged, whole)):
        assert a[1] == b[1] and np.array_equal(a[0], b[0]), k


def test_engine_chain5_into_the_slot(dspfx, torch_cuda):
    """an engine writes chain5 output straight into the slot; the pulls equal dspfx_process output fed to the restatement"""
    torch = torch_cuda
    from dsp_stuff_amd import workloads
    n, tile = 1024, 256
    engines = [dspfx.Engine(n, B, link_flags=3, tile_channels=tile) for _ in range(2)]
    for e in engines:
        e.set_chain(workloads.chain5(dspfx, delay=300))
    p = Pair(dspfx, torch, n, 44100, tile, I16, 2)
    x = torch.empty(B * n, dtype=torch.float32, device="cuda")
    y = torch.empty_like(x)
    for k in range(12):
        engines[0].fill_noise(x, B, k * B)
        slot = p.bank.slot_tensor()
        engines[0].process(x, out=slot, n_frames=B)
        p.bank.push(slot, B)
        engines[1].process(x, out=y, n_frames=B)               # the same block through dspfx_process, for the restatement
        torch.cuda.synchronize()
        p.fifo = np.concatenate([p.fifo, dspfx.from_layout(y.cpu().numpy(), B, n, tile)])
        p.pull(118)


def test_bad_descriptors_and_arguments(dspfx, torch_cuda):
    ok = dict(channels=64, target_hz=44100)
    for bad in (dict(target_hz=0), dict(out_format=4), dict(out_format=-1), dict(out_channels=0), dict(out_channels=3),
                dict(slots=2), dict(block_frames=0), dict(block_frames=4097), dict(channels=0), dict(tile_channels=48),
                dict(channels=96, tile_channels=64)):
        with pytest.raises(dspfx.DspfxError) as ei:
            dspfx.Resampler(**{**ok, **bad})
        assert ei.value.status == -1, bad
    r = dspfx.Resampler(64, 44100)
    for n_out in (0, 4097):
        with pytest.raises(dspfx.DspfxError) as ei:
            r.pull(n_out, out=torch_cuda.zeros(64, device="cuda"))
        assert ei.value.status == -1
    out, used, under = r.pull(4096)                            # the cap itself is allowed (an underrun here)
    assert under and used == 0


def test_pulls_from_a_second_thread_keep_the_counters(dspfx, torch_cuda):
    """pushes on this thread, pulls on another, each on its own stream, for about two seconds: frames pushed = frames consumed
    + frames waiting, and no call fails other than a push into a full FIFO"""
    torch = torch_cuda
    n = 256
    bank = dspfx.Resampler(n, 44100, slots=8)
    blk = torch.zeros(B * n, device="cuda")
    state = {"consumed": 0, "pulls": 0, "under": 0, "err": None}
    stop = threading.Event()

    def puller():
        try:
            s = torch.cuda.Stream()
            out = torch.empty(118 * n, device="cuda")
            while not stop.is_set():
                _, used, under = bank.pull(118, out=out, stream=s.cuda_stream)
                state["consumed"] += used
                state["pulls"] += 1
                state["under"] += under
            s.synchronize()
        except Exception as e:                                 # noqa: BLE001
            state["err"] = e

    t = threading.Thread(target=puller)
    t.start()
    pushed, full = 0, 0
    end = time.time() + 2.0
    while time.time() < end:
        try:
            bank.push(blk, B)
            pushed += B
        except dspfx.DspfxError as e:
            assert e.status == -6
            full += 1
    stop.set()
    t.join(30)
    assert not t.is_alive() and state["err"] is None, state["err"]
    torch.cuda.synchronize()
    assert pushed == state["consumed"] + bank.available
    assert state["pulls"] > state["under"] and pushed > 0


def test_large_bank_on_a_sample_of_channels(dspfx, torch_cuda):
    """2^18 channels, where the bank itself picks 4 channels a lane: 6 callbacks, checked on a seeded sample of channels"""
    torch = torch_cuda
    n, tile, hz = 1 << 18, 256, 44100
    bank = dspfx.Resampler(n, hz, tile_channels=tile, out_format=I16, out_channels=2)
    rng = np.random.default_rng(21)
    sample = np.sort(rng.choice(n, 512, replace=False))
    ref = R.Resampler(len(sample), hz)
    fifo = np.zeros((0, len(sample)), np.float32)
    g = torch.Generator(device="cuda").manual_seed(5)
    for k in range(7):
        slot = bank.slot_tensor()
        slot.copy_(torch.rand(B * n, device="cuda", generator=g) * 2.0 - 1.0)
        bank.push(slot, B)
        blk = dspfx.from_layout(slot.cpu().numpy(), B, n, tile)
        fifo = np.concatenate([fifo, blk[:, sample]])
        if k == 0:
            continue
        out, used, under = bank.pull(118)
        want, consumed = ref.callback(fifo, 118)
        assert not under and used == consumed
        fifo = fifo[consumed:]
        torch.cuda.synchronize()
        got = dspfx.from_layout(out.cpu().numpy().view(np.int32), 118, n, tile)[:, sample]      # a stereo pair = one int32
        exp = R.to_device(want, I16, 2).view(np.int32)
        assert np.array_equal(got, exp), k
