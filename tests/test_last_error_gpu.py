"""dspfx_last_error keeps a copy of the message per calling thread.  The copy is keyed by the engine it belongs to, and that key
must not be the engine's address: an engine created after another was destroyed may be allocated where that one was, and a fresh
engine has no message."""
import pytest

pytestmark = pytest.mark.gpu


def test_a_fresh_engine_shows_no_message_of_a_destroyed_one(dspfx):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    same_address = 0
    for _ in range(8):
        a = dspfx.Engine(64, 128, link_flags=0)
        a.set_chain([dspfx.Gain(1.0)])
        addr = a.h.value
        with pytest.raises(dspfx.DspfxError):
            a.set_param(5, 0, 1.0)                               # no such node: this thread fails on this engine
        assert a.L.dspfx_last_error(a.h).decode() != ""
        a.close()
        b = dspfx.Engine(64, 128, link_flags=0)
        same_address += b.h.value == addr
        assert b.L.dspfx_last_error(b.h).decode() == "", "a fresh engine has no message"
        b.close()
    print(f"{same_address} of 8 engines were allocated at the address of the one destroyed before them")
