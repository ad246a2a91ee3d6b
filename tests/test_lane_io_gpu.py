"""The lane decision the per-channel banks share (csrc/lane_io.hip.h, lane_plan): a run takes four channels per lane with 16-byte
accesses only when every block it is given is 16-byte aligned, and one channel per lane otherwise.  The other bank tests reach the
one-channel kernels only through N = 70; here the shapes allow four channels and one pointer at a time does not.  For ChannelStrips
(one band), Talkers (gated), ChannelDynamics (plain and keyed), ChannelShapers (SoftClip) and ChannelGenerators (with add_to, and
with the control blocks too): two consecutive blocks from aligned device tensors, then -- a fresh bank, the same stores, the same
data -- with one block argument a view that starts one float into a larger tensor.  The outputs and the banks' device tables must
be the same bits.  The aligned run is made once per bank form and shape and shared.  Outputs start as NaN, so every sample is shown
to be written."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
NF = 37                                  # four whole chunks of 8 rows and 5 single rows; nine chunks of 4 and one row where a run holds two streams
BLOCKS = 2                               # the second block starts from the state, the gates and the clocks the first one left
SHAPES = [(64, 0), (256, 64)]            # flat; tiled, more than one tile
# a bank form -> the block arguments of its run, in the order they are shifted
FORMS = {
    "strips": ("in", "out"),
    "talkers": ("in", "out"),
    "dynamics": ("in", "out"),
    "dynamics_keyed": ("in", "key", "out"),
    "shapers": ("in", "out"),
    "gens": ("add_to", "out"),
    "gens_ctl": ("add_to", "amplitude", "frequency", "out"),
}
TABLES = {"talkers": ("levels", "targets", "talkers", "talker_levels"), "dynamics": ("levels", "reductions"),
          "dynamics_keyed": ("levels", "reductions"), "gens": ("clocks",), "gens_ctl": ("clocks",)}
CASES = [(form, arg) for form, args in FORMS.items() for arg in args]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


_REF = {}


@pytest.fixture(scope="module", autouse=True)
def references():
    yield
    _REF.clear()


def make(dspfx, form, n, tile, rng):
    """a fresh bank of the form; every channel carries a node with its own sliders"""
    if form == "strips":
        bank = dspfx.ChannelStrips(n, bands=1, tile_channels=tile)
        bank.set_gain(rng.uniform(0.25, 2.0, n).astype(F))
        raw = np.tile(np.array([1.0, -1.8, 0.81, 0.0025, 0.005, 0.0025], F), (n, 1))
        raw[:, 1] += rng.uniform(0.0, 0.2, n).astype(F)
        bank.set_band(0, raw)
    elif form == "talkers":
        bank = dspfx.Talkers(n, group_size=32, top=3, tile_channels=tile)
        bank.set_detector(rng.choice([0, 1, 48], n).astype(F), rng.choice([0, 1, 1000], n).astype(F))
    elif form.startswith("dynamics"):
        bank = dspfx.ChannelDynamics(n, tile_channels=tile)
        bank.set(threshold=rng.choice([0.0125, 0.1, 0.25, 0.5], n).astype(F), makeup=rng.choice([1.0, 0.7, 3.0], n).astype(F),
                 attack=rng.choice([0, 1, 48], n).astype(F), release=rng.choice([0, 1, 1000], n).astype(F))
    elif form == "shapers":
        bank = dspfx.ChannelShapers(n, tile_channels=tile)
        bank.set_distort(level=rng.uniform(0.5, 4.0, n).astype(F), mode=dspfx.SOFT_CLIP)
    else:
        bank = dspfx.ChannelGenerators(n, tile_channels=tile)
        bank.set(amplitude=rng.uniform(-1.0, 1.0, n).astype(F), frequency=rng.uniform(50.0, 12000.0, n).astype(F),
                 mode=rng.integers(dspfx.SIG_SINE, dspfx.SIG_CONSTANT + 1, n).astype(np.uint32))
    return bank


def place(torch, data, shifted):
    """`data` on the device: at the start of a tensor of its own, or one float into one"""
    buf = torch.full((data.numel() + 4,), float("nan"), dtype=torch.float32, device="cuda:0")
    v = buf[1:1 + data.numel()] if shifted else buf[:data.numel()]
    v.copy_(data)
    assert v.data_ptr() % 16 == (4 if shifted else 0)
    return v


def run(dspfx, torch, form, n, tile, shifted=()):
    """BLOCKS runs of a fresh bank -> {name: int32 bits on the host} of every output block and every device table"""
    rng = np.random.default_rng(20)
    bank = make(dspfx, form, n, tile, rng)
    try:
        res = {}
        for b in range(BLOCKS):
            blk = {a: place(torch, torch.from_numpy(rng.uniform(-1.0, 1.0, NF * n).astype(F)), a in shifted) for a in FORMS[form] if a != "out"}
            out = place(torch, torch.full((NF * n,), float("nan")), "out" in shifted)
            if form.startswith("gens"):
                bank.run(NF, out=out, add_to=blk["add_to"], amplitude=blk.get("amplitude"), frequency=blk.get("frequency"))
            elif form.startswith("dynamics"):
                bank.run(blk["in"], NF, out=out, key=blk.get("key"))
            else:
                bank.run(blk["in"], NF, out=out)
            res[f"out{b}"] = out
        torch.cuda.synchronize()
        for name in TABLES.get(form, ()):
            res[name] = getattr(bank, name)()
        return {k: v.contiguous().view(torch.int32).cpu() for k, v in res.items()}
    finally:
        bank.close()


def reference(dspfx, torch, form, n, tile):
    key = (form, n, tile)
    if key not in _REF:
        ref = run(dspfx, torch, form, n, tile)
        for b in range(BLOCKS):
            assert not torch.isnan(ref[f"out{b}"].view(torch.float32)).any(), "the aligned run left samples unwritten"
        _REF[key] = ref
    return _REF[key]


@pytest.mark.parametrize("form,arg", CASES)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_one_misaligned_block_changes_no_bit(dspfx, torch_cuda, n, tile, form, arg):
    torch = torch_cuda
    ref = reference(dspfx, torch, form, n, tile)
    got = run(dspfx, torch, form, n, tile, shifted=(arg,))
    assert sorted(got) == sorted(ref)
    for name in ref:
        assert torch.equal(got[name], ref[name]), f"{form} with `{arg}` one float off 16 bytes: {name} differs from the aligned run"
