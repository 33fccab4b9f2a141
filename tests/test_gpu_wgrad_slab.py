"""The weight-gradient family on the GPU, bit for bit against the parent commit of csrc/lwg_wgrad_slab.h.

Every kernel of the family is deterministic (slabs are added in slab order, no float atomics), so sharing the slab arithmetic, the un-packing map and the
split plan must not move one bit.  tests/golden/wgrad_slab_parent.json holds, per case of tests/wgrad_slab_cases.py, the sha256 of the dw and db bytes
the PARENT commit's library wrote on the MI355X (``python -m tests.wgrad_slab_cases gpu`` in an export of that commit, once) and the kernel forms the
case reaches: the direct kernel <SMALLC, BN> in its four combinations, the bf16 kernel's two widths, every reduction kernel (unpack<1 / 4 / 16>, unpack4,
unpack4g<4 / 8>, the plain reductions through the packed entry and through the column sums, the Winograd engine's three), with and without db, the
transposed layout with a parity launch's quarter of a pre-filled tensor, two inputs, ragged M, cin < cin_pad, nout < n_pad.  dw and db are pre-filled
with seeded values, so the positions a launch must leave alone are part of the hash."""
import faulthandler
import json
import os
import sys

import pytest

from tests import wgrad_slab_cases as wsc

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_slab_parent.json")))
FORMS = ("wgrad<1, 64>", "wgrad<1, 128>", "wgrad<0, 64>", "wgrad<0, 128>", "wgrad_bf16<64>", "wgrad_bf16<128>", "unpack<1>", "unpack<4>", "unpack<16>", "unpack4",
         "unpack4g<4>", "unpack4g<8>", "wgrad_reduce", "slab_reduce_g<4>", "slab_reduce_g<16>", "wgw_reduce<1>", "wgw_reduce<4>", "wgw_reduce<16>",
         "colsum_partial4", "colsum_partial ")


@pytest.fixture(autouse=True)
def _own_timeout():
    """A launch that hangs ends the run after a minute (each case takes milliseconds) instead of holding the device."""
    faulthandler.dump_traceback_later(60, exit=True, file=sys.stderr)
    yield
    faulthandler.cancel_dump_traceback_later()


def test_the_cases_reach_every_form():
    assert sorted(GOLD) == sorted(wsc.GPU_CASES)
    forms = [GOLD[name]["form"] for name in GOLD]
    for f in FORMS:
        assert any(f in g for g in forms), f
    for entry, red in (("lwg_conv2d_wgrad_nhwc_f32", ("wgrad_reduce", "slab_reduce_g<4>", "slab_reduce_g<16>")), ("lwg_colsum_nhwc_f32", ("wgrad_reduce", "slab_reduce_g<4>", "slab_reduce_g<16>"))):
        got = {GOLD[n]["form"].split(" + ")[1] for n, (e, _) in wsc.GPU_CASES.items() if e == entry}
        assert got == set(red), (entry, got)
    assert any("db" in GOLD[n] and "dw" in GOLD[n] for n in GOLD) and any("db" not in GOLD[n] for n in GOLD)


@pytest.mark.parametrize("name", sorted(wsc.GPU_CASES))
def test_bits_are_the_parents(name):
    got = wsc.run_case(name)
    print(name, got)
    assert got == GOLD[name]
