"""A fixed list of ops.conv2d / ops.conv_transpose2d launches and one recorder of what each of them asks of the library (shared by
tests/test_conv_routes_cpu.py and tests/test_gpu_conv_routes.py).

The recorder stands in for ``_lib.lib()``: the host-only queries (``*_plan``, ``*_ws_floats``, ``*_applies``, ``*_is_one_grid``, ``lwg_conv_slice_count``)
go to the real library - they read the launch description and never a pointer's target -, every other call is recorded by name and returns 0
(``forward=True``, the GPU test: it runs).  ``ops._wwino`` / ``ops._wwino4`` are recorded as ``panel:<name>``.  Per case the record is the ordered
list of library and panel calls, every closing CONV_HOOK info dict, what ``ops._hook_end`` was handed (kind, sliced, extra) and the exception, if
the call raised.  Nothing here reads ``ops.conv2d_route``: the module runs unchanged on a tree that does not have it, which is how
tests/golden/conv_routes_parent.json was written (``python -m tests.conv_route_cases OUT.json`` in an export of the parent commit with this file
copied in)."""
import contextlib
import json
import sys

import torch

from ipercore_amd import _lib, ops
from ipercore_amd.networks import packing

HOST_SUFFIXES = ("_plan", "_ws_floats", "_applies", "_is_one_grid")
HOST_NAMES = ("lwg_conv_slice_count",)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
EPIS = {"none": (ops.EPI_NONE, ops.ACT_NONE), "relu": (ops.EPI_NONE, ops.ACT_RELU), "res": (ops.EPI_RESIDUAL, ops.ACT_NONE),
        "resmask": (ops.EPI_RESIDUAL, ops.ACT_RELU_MASK), "spade": (ops.EPI_SPADE, ops.ACT_NONE)}
MODES = ("fp32", "bf16", "bf16_winograd", "split", "winograd", "winograd2x2", "bf16_operands")
SMALL, MID, BIG = (1, 8, 8, 64, 64), (1, 32, 32, 256, 256), (2, 64, 64, 256, 256)


def is_host(name):
    return name.endswith(HOST_SUFFIXES) or name in HOST_NAMES


class Recorder:
    def __init__(self, real, forward=False):
        self.real, self.forward, self.calls, self.muted = real, forward, [], 0

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*args):
            if not self.muted:
                self.calls.append(name)
            return fn(*args) if self.forward or is_host(name) else 0
        return call


class _Cuda(torch.Tensor):
    """A CPU tensor that says it lives on the device: the transposed convolution's routing asks."""
    @property
    def is_cuda(self):
        return True


@contextlib.contextmanager
def patched(obj, **attrs):
    old = {k: getattr(obj, k) for k in attrs}
    for k, v in attrs.items():
        setattr(obj, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(obj, k, v)


_DEFAULTS = dict(op="conv2d", mode="fp32", tiles="2x2", shape=SMALL, k="k3", splitk=False, epi="none", c1=0, yc=None, ycoff=0, q4=False, out_hw=False,
                 xdt="f32", ydt=None, lists=None, sw=None, cuda=False, gpu=False)
CASES = []


def _case(**kw):
    assert set(kw) <= set(_DEFAULTS), kw
    c = dict(_DEFAULTS, **kw)
    c["id"] = "-".join(f"{k}={'x'.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in sorted(kw.items()) if k != "gpu") or "default"
    assert c["id"] not in {d["id"] for d in CASES}, c["id"]
    CASES.append(c)


def _build_cases():
    # every precision mode x tiles x split-K x epilogue on fp32 tensors (the small and the middle shape; the large one plain)
    for mode in MODES:
        for tiles in ("2x2", "4x4"):
            for splitk in (False, True):
                for shape in (SMALL, MID):
                    for epi in ("none", "res", "resmask", "spade"):
                        _case(mode=mode, tiles=tiles, splitk=splitk, shape=shape, epi=epi)
                _case(mode=mode, tiles=tiles, splitk=splitk, shape=BIG)
    for mode in ("fp32", "split", "winograd", "winograd2x2", "bf16_operands"):
        for splitk in (False, True):
            _case(mode=mode, splitk=splitk, shape=MID, c1=128)                                  # a skip concatenation
            _case(mode=mode, splitk=splitk, shape=MID, c1=8)                                    # ... one the bf16-operand kernel refuses (C0 % 32)
            _case(mode=mode, splitk=splitk, shape=(1, 32, 32, 32, 64))                          # Cin < WINO4_MIN_CIN
            _case(mode=mode, splitk=splitk, shape=(1, 16, 16, 64, 128), yc=256, ycoff=128)      # a slice of a wider output
            _case(mode=mode, splitk=splitk, shape=(1, 16, 16, 64, 64), yc=128, ycoff=2)         # ... at an offset no Winograd / bf16-operand launch takes
            _case(mode=mode, splitk=splitk, shape=MID, k="k1")
            _case(mode=mode, splitk=splitk, shape=MID, k="k4s2")
            _case(mode=mode, splitk=splitk, shape=(1, 16, 16, 8, 64), k="c8")                   # a small-Cin first layer
            for out_hw in (False, True):                                                        # one parity launch of a transposed convolution
                _case(mode=mode, splitk=splitk, shape=MID, k="parity", out_hw=out_hw)
            _case(mode=mode, splitk=splitk, shape=(1, 19, 18, 128, 64), c1=56, tiles="4x4")      # ragged, the inputs' boundary off the 32-channel grid
    # channel-quad planes, and the guard that refuses them
    for mode in MODES:
        _case(mode=mode, q4=True, shape=MID)
    _case(mode="winograd", q4=True, splitk=True)
    _case(mode="fp32", q4=True, xdt="bf16", ydt="f32")
    # bf16 tensors: dispatch is by dtype in every mode; hr / pw / v2 / c8 / bf16 Winograd
    for mode in ("fp32", "bf16", "bf16_winograd", "winograd"):
        for shape in (SMALL, (1, 16, 16, 128, 128)):
            for epi in ("none", "relu", "res", "spade"):
                _case(mode=mode, xdt="bf16", shape=shape, epi=epi)
        _case(mode=mode, xdt="bf16", shape=(1, 16, 16, 128, 128), c1=64)
        _case(mode=mode, xdt="bf16", shape=(1, 16, 16, 128, 128), k="k1")                       # the pointwise form
        _case(mode=mode, xdt="bf16", shape=(1, 16, 16, 64, 128), k="k1")                        # 1x1 but not C -> C
        _case(mode=mode, xdt="bf16", shape=(1, 16, 16, 64, 64), k="k4s2")
        _case(mode=mode, xdt="bf16", shape=(1, 16, 16, 64, 64), k="parity")
        _case(mode=mode, xdt="bf16", shape=(1, 16, 16, 64, 128), yc=256, ycoff=64)
        _case(mode=mode, xdt="f32", ydt="bf16", shape=(1, 16, 16, 8, 64), k="c8")               # the first layer of a bf16 network
        _case(mode=mode, xdt="f32", ydt="bf16", shape=(1, 16, 16, 64, 64))
    _case(mode="bf16", xdt="bf16", ydt="f32")                                                   # raises
    _case(mode="bf16", xdt="bf16", shape=(1, 8, 8, 32, 64))                                     # raises
    for name in ("BF16_HR", "BF16_PW", "BF16_C8"):
        _case(mode="bf16", xdt="bf16", sw=name)
        _case(mode="bf16", xdt="bf16", shape=(1, 16, 16, 128, 128), k="k1", sw=name)
        _case(mode="bf16", xdt="f32", ydt="bf16", shape=(1, 16, 16, 8, 64), k="c8", sw=name)
    _case(mode="bf16_winograd", xdt="bf16", sw="BF16_HR")                                       # the switch does not reach this mode
    # lists: every accepted shape, the silent ignores, the guard
    for lists in ("block", "skip", "skip8", "skipnofine"):
        for epi in ("none", "spade"):
            _case(mode="winograd", shape=(1, 32, 32, 128, 128), epi=epi, lists=lists)
            _case(mode="winograd", shape=(1, 32, 32, 128, 128), epi=epi, lists=lists, sw="SPADE_SKIP_Q8_MIN")      # the 8 x 8 lists in reach
            _case(mode="bf16", xdt="bf16", shape=(1, 16, 16, 128, 128), epi=epi, lists=lists)
        _case(mode="winograd", shape=(1, 32, 32, 128, 128), lists=lists, sw="SPADE_SKIP_FINE")
    for mode in MODES:
        _case(mode=mode, lists="block")
        _case(mode=mode, lists="skip", xdt="bf16")
    _case(mode="winograd", lists="block", splitk=True)                                          # raises: training launches keep F(2x2) ...
    _case(mode="winograd", lists="block", splitk=True, tiles="4x4")                             # ... admitted, then refused by the plan: lists ignored
    _case(mode="winograd", lists="block", splitk=True, tiles="4x4", shape=BIG)                  # ... taken split by the plan: the list form wins
    _case(mode="winograd", lists="block", k="k1")                                               # admitted on Cin alone, not eligible: lists ignored
    _case(mode="winograd", lists="block", shape=(1, 8, 8, 32, 64))
    _case(mode="winograd", lists="skip", sw="WINO4")
    _case(mode="bf16", xdt="bf16", lists="block", c1=32, shape=(1, 8, 8, 128, 64))
    _case(mode="bf16", xdt="bf16", lists="block", k="k1")
    _case(mode="bf16", xdt="bf16", lists="badcal")
    _case(mode="bf16", xdt="bf16", lists="skip", sw="BF16_HR")
    # lab switches of the "winograd" mode, each off once per plan it changes
    for name in ("WINO4", "WINO_SPLITK", "WINO4_TRAIN_WHOLE", "WINO4_TRAIN_SPLITK"):
        for tiles in ("2x2", "4x4"):
            for splitk in (False, True):
                for shape in (MID, BIG, (1, 128, 128, 128, 256)):
                    _case(mode="winograd", tiles=tiles, splitk=splitk, shape=shape, sw=name)
    for tiles in ("2x2", "4x4"):
        _case(mode="winograd", tiles=tiles, splitk=True, shape=(1, 128, 128, 128, 256))
        _case(mode="winograd", tiles=tiles, splitk=True, shape=(1, 28, 28, 512, 512))
    # transposed convolutions: device / host tensors, both sides of WINO_UP4_24_MIN_HW, the parity-group rule's shapes (every one of these is ONE grid by the library's rule: the groups it refuses are further down)
    up = ((1, 8, 8, 64, 64), (1, 32, 32, 32, 32), (1, 64, 64, 32, 32), (1, 64, 64, 256, 128), (1, 128, 128, 128, 64), (1, 128, 128, 256, 128))
    for mode in MODES:
        for splitk in (False, True):
            for shape in up:
                _case(op="convt", mode=mode, splitk=splitk, shape=shape, cuda=True)
            _case(op="convt", mode=mode, splitk=splitk, cuda=True, out_hw=True)
            _case(op="convt", mode=mode, splitk=splitk, cuda=True, out_hw=True, shape=(1, 64, 64, 256, 128))
            _case(op="convt", mode=mode, splitk=splitk, cuda=False)
            _case(op="convt", mode=mode, splitk=splitk, cuda=True, xdt="bf16")
            _case(op="convt", mode=mode, splitk=splitk, cuda=True, xdt="bf16", shape=(1, 8, 8, 256, 64))        # Cin > 128: four launches
        _case(op="convt", mode=mode, cuda=True, q4=True)
    for name in ("WINO_UP4", "WINO_UP4_24", "F32_UP4", "BF16_UP4", "BF16_HR"):
        for mode in ("fp32", "winograd", "bf16_operands", "bf16"):
            _case(op="convt", mode=mode, cuda=True, sw=name, shape=(1, 64, 64, 32, 32))
            _case(op="convt", mode=mode, cuda=True, sw=name, shape=(1, 64, 64, 256, 128), splitk=True)
            _case(op="convt", mode=mode, cuda=True, sw=name, xdt="bf16")
    # groups lwg_conv_transpose4_is_one_grid REFUSES (300 tiles of 128 x 128 or more per parity): asked, then four parity conv2d calls - and in
    # "bf16_operands" with split-K the parity-group rule stops at the refusal (lwg_conv2d_bf16op_ws_floats is asked by the four calls only)
    for shape in ((1, 256, 256, 64, 64), (4, 128, 128, 128, 64), (2, 256, 256, 32, 32), (8, 64, 64, 256, 128)):
        for mode in ("fp32", "winograd", "bf16_operands"):
            for splitk in (False, True):
                _case(op="convt", mode=mode, splitk=splitk, shape=shape, cuda=True)
    for mode in ("fp32", "winograd", "bf16_operands"):
        _case(op="convt", mode=mode, splitk=True, shape=(1, 256, 256, 64, 64), cuda=True, out_hw=True)
    # the GPU test's cases: one per route at the smallest shape that takes it, plain epilogue (real tensors: "cuda" is not read)
    for mode, kw in (("fp32", {}), ("fp32", dict(splitk=True, shape=(1, 16, 16, 512, 512))), ("split", {}), ("winograd", dict(shape=(1, 8, 8, 32, 64))),
                     ("winograd", {}), ("winograd", dict(splitk=True, shape=MID)), ("winograd", dict(splitk=True, shape=BIG, tiles="4x4")),
                     ("bf16_operands", {}), ("bf16_operands", dict(splitk=True, shape=(1, 16, 16, 512, 512))), ("bf16", dict(xdt="bf16")),
                     ("bf16", dict(xdt="bf16", k="k1")), ("bf16", dict(xdt="bf16", k="k4s2")), ("bf16_winograd", dict(xdt="bf16")),
                     ("bf16", dict(xdt="f32", ydt="bf16", k="c8", shape=(1, 8, 8, 8, 64)))):
        _case(mode=mode, gpu=True, epi="relu", **kw)
    for mode, kw in (("bf16", dict(xdt="bf16")), ("winograd", dict(shape=(1, 8, 8, 32, 64))), ("winograd", dict(shape=(1, 64, 64, 32, 64))),
                     ("fp32", dict(shape=(1, 8, 8, 32, 64))), ("fp32", dict(shape=(1, 8, 8, 32, 64), sw="F32_UP4")), ("bf16_operands", {}),
                     ("fp32", dict(shape=(1, 256, 256, 64, 64)))):                             # ... and one group the one-grid rule refuses
        _case(op="convt", mode=mode, gpu=True, epi="relu", cuda=True, **kw)


_build_cases()
_SPECS = {}


def _specs(c, device):
    """The case's spec (conv2d) or four parity specs (conv_transpose2d), packed once per (kernel, channels, device) on the host from zero weights."""
    _, _, _, C, N = c["shape"]
    key = (c["op"], c["k"], C, N, str(device))
    if key not in _SPECS:
        bias = torch.zeros(N)
        if c["op"] == "convt" or c["k"] == "parity":
            s = packing.pack_conv_transpose(torch.zeros(C, N, 4, 4), bias)
        elif c["k"] == "c8":
            s = [packing.pack_conv(torch.zeros(N, 3, 3, 3), bias, cin_pad=8)]
        else:
            kh = {"k3": 3, "k1": 1, "k4s2": 4}[c["k"]]
            s = [packing.pack_conv(torch.zeros(N, C, kh, kh), bias, stride=2 if c["k"] == "k4s2" else 1, pad=1 if c["k"] == "k4s2" else None)]
        _SPECS[key] = [packing.spec_to(sp, device) for sp in s] if device is not None else s
    s = _SPECS[key]
    return s if c["op"] == "convt" else s[1] if c["k"] == "parity" else s[0]


def _lists(c, x0, y, spec, zeros):
    kind, (B, H, W, _, N) = c["lists"], c["shape"]
    n = B * H * W
    trip = lambda: tuple(zeros((m,), torch.int32) for m in (n, n, 2))      # noqa: E731
    if c["xdt"] == "bf16":
        cal = zeros((H * W * (N if c["epi"] == "spade" else y.shape[3]) + (kind == "badcal"),), torch.float32 if c["epi"] == "spade" else torch.bfloat16)
    else:
        cal = zeros((H * W * N,), torch.float32)
    if kind in ("block", "badcal"):
        return trip() + (cal,)
    sl = ops.SkipLists(trip())
    sl.fine = None if kind == "skipnofine" else trip()
    sl.fine8 = trip() if kind == "skip8" else None
    return sl, cal


def run_case(c, device=None):
    """Run one case under a recorder (device=None: host tensors, nothing launched; a device: the real launches) -> its record."""
    dev = "cpu" if device is None else device
    xdt, ydt = DTYPES[c["xdt"]], DTYPES[c["ydt"] or c["xdt"]]
    B, H, W, C, N = c["shape"]
    epi, act = EPIS[c["epi"]]

    def zeros(shape, dtype):
        t = torch.zeros(shape, dtype=dtype, device=dev)
        return t.as_subclass(_Cuda) if c["cuda"] and device is None else t

    spec = _specs(c, device)
    rec = Recorder(_lib.lib(), forward=device is not None)
    hooks, ends = [], []
    real_end, real_panels = ops._hook_end, {"_wwino": ops._wwino, "_wwino4": ops._wwino4}

    def hook_end(a, sp, e, kind, slices=True, extra=0):
        ends.append([kind, bool(slices), int(extra)])
        return real_end(a, sp, e, kind, slices, extra)

    def panel(name):
        def build(sp):
            rec.calls.append("panel:" + name)
            if device is None:
                return sp.w
            rec.muted += 1                         # the panel's own launch is not part of the conv call's trace: recorded as panel:<name>
            try:
                return real_panels[name](sp)
            finally:
                rec.muted -= 1
        return build

    patches = dict(_hook_end=hook_end, _wwino=panel("_wwino"), _wwino4=panel("_wwino4"),
                   CONV_HOOK=lambda begin, M, sp, e, info: None if begin else hooks.append(dict(info)))
    if device is None:
        patches.update(_stream=lambda: None, _ptr=lambda t, dt=None: 0 if t is None else t.data_ptr())
    if c["sw"]:
        patches[c["sw"]] = 1 if c["sw"] == "SPADE_SKIP_Q8_MIN" else False
    ops._PARITY4_PLAN.clear()
    ops._LISTS_APPLY.clear()
    raised = None
    with patched(_lib, lib=lambda: rec), patched(ops, **patches), ops.conv_precision(c["mode"]), ops.train_conv_tiles(c["tiles"]):
        try:
            if c["op"] == "convt":
                x = zeros((B, H, W, C), xdt)
                y = zeros((B, N // 4, 2 * H, 2 * W, 4) if c["q4"] else (B, 2 * H, 2 * W, N), ydt)
                args = (x, spec, y)
                kw = dict(act=act, splitk=c["splitk"], out_hw=(lambda s: (H, W)) if c["out_hw"] else None, q4=c["q4"])
                ops.conv_transpose2d(*args, **kw)
            else:
                c1 = c["c1"]
                x0, x1 = zeros((B, H, W, C - c1), xdt), zeros((B, H, W, c1), xdt) if c1 else None
                OH, OW = (H // 2, W // 2) if c["k"] == "k4s2" else (2 * H, 2 * W) if c["k"] == "parity" else (H, W)
                yc = c["yc"] or (N // 2 if c["epi"] == "spade" else N)
                y = zeros((B, yc // 4, OH, OW, 4) if c["q4"] else (B, OH, OW, yc), ydt)
                kw = dict(x1=x1, epi=epi, act=act, out_hw=(H, W) if c["out_hw"] else None, ycoff=c["ycoff"], splitk=c["splitk"], q4=c["q4"])
                if epi == ops.EPI_RESIDUAL:
                    kw["res"] = zeros(tuple(y.shape), ydt)
                if epi == ops.EPI_SPADE:
                    kw.update(xn=zeros((B, OH, OW, N // 2), ydt), mean=zeros((B, N // 2), torch.float32), rstd=zeros((B, N // 2), torch.float32))
                if c["lists"]:
                    kw["lists"] = _lists(c, x0, y, spec, zeros)
                args = (x0, spec, y)
                ops.conv2d(*args, **kw)
        except (ValueError, AssertionError, TypeError) as e:
            raised = f"{type(e).__name__}: {e}"
    return {"calls": rec.calls, "hooks": hooks, "hook_end": ends, "raises": raised}, args, kw


def load(path):
    """{case id: record} of a file ``main`` wrote (the distinct records once, the cases by index)."""
    with open(path) as fp:
        doc = json.load(fp)
    return {cid: doc["records"][i] for cid, i in doc["cases"].items()}


def main(out):
    records, cases = [], {}
    for c in CASES:
        r = run_case(c)[0]
        if r not in records:
            records.append(r)
        cases[c["id"]] = records.index(r)
    with open(out, "w") as fp:
        fp.write('{"records": [\n' + ",\n".join(json.dumps(r, sort_keys=True) for r in records) + '],\n"cases": {\n')
        fp.write(",\n".join(f"{json.dumps(cid)}: {i}" for cid, i in cases.items()) + "}}\n")
    print(len(CASES), "cases,", len(records), "distinct records ->", out)


if __name__ == "__main__":
    main(sys.argv[1])
