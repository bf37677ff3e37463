"""Every row of the option table (datago_amd/csrc/host/options.cpp) reaches a
live context through dg_ctx_set_option, and what the keys do beyond storing a
value (locks, the cache starting over, streams made again) still runs: the
context decodes bit-exactly afterwards, and again after its slots' streams were
rebuilt behind batches.  The values each key takes are checked without a GPU
(test_options_cpu.py)."""
import numpy as np
import pytest

from datago_amd import synth
from oracle import oracle as O
from test_options_cpu import option_defaults

pytestmark = pytest.mark.gpu


def test_every_option_reaches_a_context_and_it_still_decodes():
    from datago_amd import _lib as L
    names, defaults = option_defaults()
    ctx = L.Context(0)
    for key in names:  # each key with its default: nothing changes, every step around the store runs
        value = defaults.get(key, 1)  # reset_host_us has no value of its own
        assert L.load().dg_ctx_set_option(ctx._h, key.encode(), value) == L.DG_OK, (key, value, L.last_error())
    assert defaults["debug_flags"] == defaults["dec_dbg"] == defaults["max_device_mb"] == 0
    jpg, png = synth.make_jpeg(41, 48, 40, 90, "4:2:0"), synth.make_png(42, 17, 9, "RGBA")
    want = [O.jpeg_decode(jpg)[1], O.png_decode(png)[1]]

    def check():
        res = ctx.decode_batch([jpg, png])
        for (st, arr, _), ref in zip(res, want):
            assert st == 0, L.last_error()
            assert arr.shape == ref.shape and np.array_equal(arr, ref)

    check()
    ctx.set_option("slot_queue", 0)  # the baseline slots finish, their streams are made again
    ctx.set_option("side_queue", -1)
    check()
    ctx.close()
