"""Option sync_chain on the GPU: k_huff_sync's state-only decodes with up to
1, 2 and 3 chained multi entries per step (multi_chain, dg_entropy.h) give the
bytes, the statuses and the resync work of the unchained kernel, in both decode
semantics, on the small images tests/test_entropy_chain.py checks state by
state on the CPU (every sampling, flat blocks, blocks without EOB, optimised
tables, restart intervals of one MCU and of one MCU row)."""
import numpy as np
import pytest

from oracle import oracle as O
from test_entropy_chain import CASES

pytestmark = pytest.mark.gpu

NAMES = ["420_q75", "422_q75", "444_q75", "gray_q75", "420_q10", "444_q95", "gray_q10", "flat", "noise_q100",
         "optimized", "rst_mcu", "rst_row"]


def _lib():
    from datago_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def batch():
    datas = [CASES[n][0]() for n in NAMES]
    refs = {}
    for sem in (0, 1):
        with O.semantics(sem):
            dec = [O.jpeg_decode(d) for d in datas]
        assert all(st == 0 for st, _ in dec)
        refs[sem] = [a for _, a in dec]
    return datas, refs


@pytest.mark.parametrize("sem", [0, 1], ids=["libjpeg", "zune"])
@pytest.mark.parametrize("sub_bits,lead", [(256, 0), (256, -1), (2048, 0), (2048, -1)])
def test_sync_chain_bit_exact(batch, sem, sub_bits, lead):
    L = _lib()
    datas, refs = batch
    outs, work = {}, {}
    for chain in range(4):
        ctx = L.Context(0, decode_semantics=sem)
        ctx.set_option("sync_chain", chain)
        assert ctx.stat("sync_chain") == chain
        ctx.set_option("sub_bits", sub_bits)
        if lead >= 0:
            ctx.set_option("lead_bits", lead)
        outs[chain] = ctx.decode_batch(datas)
        assert ctx.stat("write_mismatch") == 0, chain
        work[chain] = (ctx.stat("resync_rounds"), ctx.stat("fix_workgroups"))
        ctx.close()
    for chain in range(4):
        assert work[chain] == work[0], (chain, work)
        for i, ((st, a, _), (st0, a0, _)) in enumerate(zip(outs[chain], outs[0])):
            assert st == 0 and st0 == 0, (chain, NAMES[i], L.last_error())
            assert a.tobytes() == a0.tobytes(), (chain, NAMES[i])
            ref = refs[sem][i]
            assert np.array_equal(a.reshape(ref.shape), ref), (chain, NAMES[i])


@pytest.mark.parametrize("value", [-1, 4])
def test_sync_chain_rejected_value_names_itself(value):
    L = _lib()
    ctx = L.Context(0)
    assert L.load().dg_ctx_set_option(ctx._h, b"sync_chain", value) == L.DG_ERR_INVALID
    msg = L.last_error()
    assert "sync_chain" in msg and str(value) in msg and "valid unless" in msg, msg
    ctx.close()
