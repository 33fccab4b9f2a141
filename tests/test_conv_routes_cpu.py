"""ops.conv2d / ops.conv_transpose2d ask the library exactly what the commit before the route record asked, launch by launch, and
ops.conv2d_route / ops.conv_transpose2d_route name what the call then does (no GPU).

tests/golden/conv_routes_parent.json was written ONCE, by tests/conv_route_cases.py run in an export of the parent commit (the last one whose
ops.conv2d was the if-chain).  It is never regenerated from the tree under test: a trace that differs is a behaviour change of the tree, and the
fix is in ipercore_amd/ops.py.  A new case is added by running the new case list on that same parent commit."""
import os

import pytest

from ipercore_amd import ops
from tests import conv_route_cases as crc

GOLDEN = crc.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routes_parent.json"))


def test_golden_covers_the_case_list():
    assert set(GOLDEN) == {c["id"] for c in crc.CASES} and len(crc.CASES) >= 300
    kinds = {h["kind"] for r in GOLDEN.values() for h in r["hooks"]}
    assert kinds == {"direct", "winograd", "winograd4", "split", "bf16", "bf16_winograd", "bf16op", "up4", "winograd_up4"}
    assert sum(1 for r in GOLDEN.values() if r["raises"]) >= 10
    # both answers of lwg_conv_transpose4_is_one_grid, and after a refusal both forms of the parity-group rule of "bf16_operands"
    asked = [r["calls"] for r in GOLDEN.values() if "lwg_conv_transpose4_is_one_grid" in r["calls"]]
    refused = [c for c in asked if "lwg_conv_transpose4_nhwc_f32" not in c]
    assert len(asked) - len(refused) >= 10 and len(refused) >= 10
    assert any(c[:2] == ["lwg_conv_transpose4_is_one_grid", "lwg_conv2d_bf16op_ws_floats"] and c.count("lwg_conv_transpose4_is_one_grid") == 1 for c in asked)
    assert any(c.count("lwg_conv_transpose4_is_one_grid") == 1 and c.count("lwg_conv2d_bf16op_ws_floats") == 4 for c in refused)


def check_route(c, rec, args, kw):
    """The route functions, asked after the call with the call's own arguments (under the same modes and switches), name what the trace shows."""
    sw = {c["sw"]: 1 if c["sw"] == "SPADE_SKIP_Q8_MIN" else False} if c["sw"] else {}
    stubs = {} if args[0].device.type != "cpu" else dict(_stream=lambda: None, _ptr=lambda t, dt=None: 0 if t is None else t.data_ptr())
    with crc.patched(ops, **sw, **stubs), ops.conv_precision(c["mode"]), ops.train_conv_tiles(c["tiles"]):
        if rec["raises"] and rec["raises"].startswith("ValueError") and c["lists"] != "badcal":
            with pytest.raises(ValueError) as e:
                ops.conv2d_route(*args, **kw)
            assert rec["raises"] == f"ValueError: {e.value}"
            return
        if rec["raises"]:
            return                                  # conv_args' own assertions, the list tensors' check: not the route's
        r = (ops.conv_transpose2d_route if c["op"] == "convt" else ops.conv2d_route)(*args, **kw)
    launches = [n for n in rec["calls"] if not crc.is_host(n) and not n.startswith("panel:")]
    assert isinstance(r, ops.ConvRoute) and r.form in ("plain", "ws", "lists")
    if r.entry is None:                             # four parity conv2d calls, each with a route of its own
        assert c["op"] == "convt" and len(launches) == 4 and len(rec["hook_end"]) == 4 and r.kind == "parity4"
        return
    assert launches == [r.entry] and rec["hook_end"] == [[r.kind, r.sliced, r.extra]] and rec["hooks"][0]["kind"] == r.kind
    assert (r.form == "ws") == (r.nws > 0) == r.entry.endswith("_ws")
    assert (r.form == "lists") == ("_list" in r.entry or r.entry.endswith(("_fine_f32", "_q8_f32"))) and (r.form != "lists" or c["lists"] is not None)
    assert [n for n in rec["calls"] if n.startswith("panel:")] == (["panel:" + r.panel] if r.panel in ("_wwino", "_wwino4") else [])
    assert r.panel is None or callable(getattr(ops, r.panel))


@pytest.mark.parametrize("c", crc.CASES, ids=lambda c: c["id"])
def test_trace_is_the_parents_and_the_route_names_it(c):
    rec, args, kw = crc.run_case(c)
    assert rec == GOLDEN[c["id"]]
    check_route(c, rec, args, kw)


def test_route_asks_what_the_call_asks():
    """conv2d_route makes conv2d's host queries in conv2d's order (with and without the caller's argument block), and a second identical
    call hands back the same record."""
    for mode, tiles in (("winograd", "4x4"), ("bf16_operands", "2x2"), ("fp32", "2x2")):
        cid = f"epi=none-mode={mode}-shape=1x32x32x256x256-splitk=True-tiles={tiles}"
        c = next(d for d in crc.CASES if d["id"] == cid)
        rec, args, kw = crc.run_case(c)
        queries = [n for n in rec["calls"] if crc.is_host(n) and n != "lwg_conv_slice_count"]
        lib = crc.Recorder(ops._lib.lib())
        with crc.patched(ops._lib, lib=lambda: lib), crc.patched(ops, _stream=lambda: None, _ptr=lambda t, dt=None: 0 if t is None else t.data_ptr()), \
                ops.conv_precision(c["mode"]), ops.train_conv_tiles(c["tiles"]):
            r1 = ops.conv2d_route(*args, **kw)
            r2 = ops.conv2d_route(*args, a=ops.conv_args(*args, **{k: v for k, v in kw.items() if k not in ("splitk", "lists")}), **kw)
        assert lib.calls == queries * 2 and r1 == r2 and r1.nws > 0, cid


def test_launch_modes_is_every_frozen_switch():
    assert ops.launch_modes() == ("fp32", True, "direct", "2x2")
    with ops.conv_precision("winograd2x2"), ops.wgrad_mode("bf16"), ops.train_conv_tiles("4x4"):
        assert ops.launch_modes() == ("winograd", False, "bf16", "4x4")
    assert ops.launch_modes() == (ops.CONV_PRECISION, ops._MODE_WINO4, ops.WGRAD_PRECISION, ops.TRAIN_CONV_TILES)
