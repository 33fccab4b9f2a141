"""The opt-in F(4x4, 3x3) Winograd forward / data gradient of the training step (TrainOpts.conv_tiles = "4x4", ops.train_conv_tiles; csrc/conv_winograd4.hip's
split-K form) - the parts that need no GPU: the switch, the new exports and their host contracts, the split plan's arithmetic through
lwg_conv2d_winograd4_plan (256 compute units without a device), the F(4x4) half of ops.PanelCache and the library calls behind ops.conv2d in
either mode."""
import ctypes

import pytest
import torch

from ipercore_amd import _lib, ops
from ipercore_amd.trainers import TrainOpts
from tests import emu_ops

NEW = ("lwg_conv2d_winograd4_f32_ws", "lwg_conv2d_winograd4_plan", "lwg_conv2d_winograd4_ws_floats", "lwg_winograd4_panels_f32")
BAD = 0xdead0000
REAL_CONV2D = ops.conv2d        # (emu_ops.install replaces ops.conv2d: the launch tests below are about the real one's library calls)


def test_switch_defaults_and_context_manager():
    assert ops.TRAIN_CONV_TILES == "2x2"
    assert TrainOpts().conv_tiles == "2x2"
    with ops.train_conv_tiles("4x4"):
        assert ops.TRAIN_CONV_TILES == "4x4"
        with ops.train_conv_tiles("2x2"):
            assert ops.TRAIN_CONV_TILES == "2x2"
        assert ops.TRAIN_CONV_TILES == "4x4"
    assert ops.TRAIN_CONV_TILES == "2x2"
    with pytest.raises(ZeroDivisionError):
        with ops.train_conv_tiles("4x4"):
            1 / 0
    assert ops.TRAIN_CONV_TILES == "2x2"
    with pytest.raises(AssertionError):
        ops.train_conv_tiles("6x6")
    with pytest.raises(AssertionError):
        ops.conv_precision("winograd4x4")          # not a precision mode: the set of those is unchanged


def test_new_symbols_at_abi_10():
    syms = _lib.header_symbols()
    for name in NEW:
        assert name in syms and name in _lib._SIGS
    with open(_lib.HEADER_PATH) as fp:
        assert "#define LWG_ABI_VERSION 10" in fp.read()
    assert _lib.lib().lwg_abi_version() == 10


def _args(B=1, H=16, W=32, C0=128, C1=0, N=64, **kw):
    a = _lib.LwgConvArgs()
    a.x0, a.w, a.y = BAD, BAD, BAD
    a.x1 = BAD if C1 else None
    a.B, a.H, a.W, a.C0, a.C1, a.OH, a.OW, a.M, a.N, a.YH, a.YW, a.YC = B, H, W, C0, C1, H, W, B * H * W, N, H, W, N
    a.ntaps, a.stride, a.omul = 9, 1, 1
    for t in range(9):
        a.dy[t], a.dx[t] = t // 3 - 1, t % 3 - 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _plan(a, with_ws=1):
    blocks, slices, nbv, wgs = ctypes.c_longlong(-1), ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    e = _lib.lib().lwg_conv2d_winograd4_plan(a, with_ws, ctypes.byref(blocks), ctypes.byref(slices), ctypes.byref(nbv), ctypes.byref(wgs))
    return e, blocks.value, slices.value, nbv.value, wgs.value


def test_host_contract_rejects_before_any_launch():
    """The four new entry points validate on the host and return 1 (ws_floats: 0) before any launch: no pointer is dereferenced, no GPU touched."""
    L = _lib.lib()
    assert L.lwg_conv2d_winograd4_f32_ws(None, BAD, None) == 1
    assert L.lwg_conv2d_winograd4_plan(None, 1, None, None, None, None) == 1
    assert L.lwg_conv2d_winograd4_ws_floats(None) == 0
    assert L.lwg_winograd4_panels_f32(None, 1, 1, None) == 1
    assert L.lwg_winograd4_panels_f32(BAD, 0, 1, None) == 1
    assert L.lwg_winograd4_panels_f32(BAD, 1, 0, None) == 1
    a = _args()
    assert _plan(a)[0] == 0 and L.lwg_conv2d_winograd4_ws_floats(a) == 2 * a.M * a.N          # the base case is inside the contract, and split
    assert L.lwg_conv2d_winograd4_plan(a, 1, None, None, None, None) == 0                      # every out pointer may be NULL

    def rejected(**kw):
        b = _args(**kw)
        return L.lwg_conv2d_winograd4_f32_ws(b, BAD, None) == 1 and L.lwg_conv2d_winograd4_f32_ws(b, None, None) == 1 and _plan(b)[0] == 1 and \
            L.lwg_conv2d_winograd4_ws_floats(b) == 0

    assert rejected(x0=None)
    assert rejected(w=None)
    assert rejected(y=None)
    assert rejected(N=32, YC=32)                   # N % 64
    assert rejected(N=96, YC=96)
    assert rejected(C0=72)                         # Cin % 16
    assert rejected(C0=64, C1=64, x1=None)         # a second input without its pointer
    assert rejected(stride=2)
    assert rejected(ntaps=4)
    assert rejected(OH=8, M=8 * 32)
    assert rejected(xdt=_lib.DT_BF16)
    assert rejected(act=_lib.ACT_RELU_MASK)        # the mask without its source


def test_split_plan_refuses_what_the_finishing_kernel_does_not_finish():
    L = _lib.lib()
    a = _args()
    assert _plan(a)[2] == 2
    spade = _args(N=128, YC=64, epi=_lib.EPI_SPADE, xn=BAD, mean=BAD, rstd=BAD, bias=BAD)
    assert _plan(spade)[0] == 0 and _plan(spade)[2] == 0 and L.lwg_conv2d_winograd4_ws_floats(spade) == 0
    res = _args(epi=_lib.EPI_RESIDUAL, res=BAD)                                                # a plain residual: whole
    assert _plan(res)[2] == 0 and L.lwg_conv2d_winograd4_ws_floats(res) == 0
    mask = _args(epi=_lib.EPI_RESIDUAL, res=BAD, act=_lib.ACT_RELU_MASK)                       # the ReLU-mask data gradient: split
    assert _plan(mask)[2] == 2 and L.lwg_conv2d_winograd4_ws_floats(mask) == 2 * mask.M * mask.N
    assert _plan(a, with_ws=0)[2] == 0                                                         # no workspace: whole


MIN_STAGES = 8      # lwg_conv_wino.h CW4_SPLIT_MIN_STAGES: K stages (8 input channels each) of a slice, but for a ragged last one


@pytest.mark.parametrize("shape", [(1, 16, 32, 128, 0, 64), (1, 17, 31, 160, 0, 128), (1, 1, 33, 96, 0, 64), (2, 8, 8, 256, 0, 256), (1, 32, 32, 64, 64, 64),
                                   (1, 19, 18, 72, 56, 64), (2, 21, 19, 256, 0, 64), (1, 64, 64, 512, 0, 128), (1, 32, 32, 512, 0, 512),
                                   (1, 28, 28, 512, 0, 512), (1, 128, 128, 256, 0, 256), (1, 64, 64, 64, 0, 64), (4, 128, 128, 128, 0, 128)])
def test_split_plan_arithmetic(shape):
    """Slices are contiguous, cover all K stages and are each an even number of stages; ws_floats = slices M N; the workgroups are the 4-wave blocks
    times the slices; a launch whose 4-wave blocks cover more than half of the 256 compute units is never split."""
    B, H, W, C0, C1, N = shape
    a = _args(B, H, W, C0, C1, N)
    e, blocks, slices, nbv, wgs = _plan(a)
    assert e == 0
    nst = (C0 + C1) // 8
    blocks32 = B * ((W + 31) // 32) * ((H + 15) // 16) * (N // 32)
    ws = _lib.lib().lwg_conv2d_winograd4_ws_floats(a)
    assert ws == slices * a.M * N
    if 2 * blocks32 > 256:
        assert slices == 0
    if slices == 0:
        whole = _plan(a, with_ws=0)
        assert (blocks, nbv, wgs) == whole[1:2] + whole[3:]
        assert nbv == (32 if blocks32 <= 256 else 64) and blocks == blocks32 * 32 // nbv and wgs == min(blocks, 256)
        return
    assert 2 <= slices <= 8 and nbv == 32 and blocks == blocks32 * slices == wgs
    # the slices the kernel derives from the stage count per slice (cw4_slice_begin / _end): sps = the smallest even count >= 8 that leaves `slices`
    sps = [s for s in range(MIN_STAGES, nst + 1, 2) if (nst + s - 1) // s == slices]
    assert sps, (nst, slices)
    want = min(8, 256 // blocks32)
    s0 = max(MIN_STAGES, (nst + want - 1) // want)
    s0 += s0 & 1
    assert s0 in sps
    bounds = [(z * s0, min((z + 1) * s0, nst)) for z in range(slices)]
    assert bounds[0][0] == 0 and bounds[-1][1] == nst and all(b[1] == c[0] for b, c in zip(bounds, bounds[1:]))
    assert all((e_ - b_) % 2 == 0 and e_ > b_ for b_, e_ in bounds) and all(e_ - b_ >= MIN_STAGES for b_, e_ in bounds[:-1])


def test_gpu_test_matrix_is_split():
    """The shapes tests/test_gpu_train_conv_tiles.py runs as split launches are split by the plan (on 256 compute units)."""
    for shape in [(1, 16, 32, 128, 0, 64), (1, 17, 31, 160, 0, 128), (1, 1, 33, 96, 0, 64), (2, 8, 8, 256, 0, 256), (1, 32, 32, 64, 64, 64),
                  (1, 19, 18, 72, 56, 64), (2, 21, 19, 256, 0, 64)]:
        assert _plan(_args(*shape))[2] >= 2, shape
    assert _plan(_args(1, 17, 31, 160, 0, 128))[2] == 3                      # 20 stages: 8 + 8 + 4, a ragged last slice
    assert _plan(_args(1, 32, 32, 64, 64, 64))[2] == 2                       # 8 + 8: the boundary is the inputs' boundary
    assert _plan(_args(1, 19, 18, 72, 56, 64))[2] == 2                       # 8 + 8: the boundary lies inside the first input (72 channels)


class _Recorder:
    """A library whose launches are recorded and not run; the host-only planners are the real library's."""
    HOST = ("lwg_conv2d_winograd_plan", "lwg_conv2d_winograd4_plan", "lwg_conv2d_ws_floats", "lwg_conv_slice_count", "lwg_conv2d_winograd_ws_floats",
            "lwg_conv2d_winograd4_ws_floats")

    def __init__(self, real, missing=()):
        self.real, self.calls, self.missing = real, [], missing

    def __getattr__(self, name):
        if name in self.missing:
            raise AttributeError(name)             # the emulated ABI of the CPU suites does not have it

        def call(*args):
            self.calls.append(name)
            return getattr(self.real, name)(*args) if name in self.HOST else 0
        return call


def _launch(monkeypatch, tiles, shape=(1, 32, 32, 256, 256), splitk=True, missing=(), **kw):
    from ipercore_amd.networks import packing
    rec = _Recorder(_lib.lib(), missing)
    emu_ops.install(monkeypatch)
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_ptr", lambda t, dt=None: 0 if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "_wwino", lambda spec: rec.calls.append("panel2x2") or spec.w)
    monkeypatch.setattr(ops, "_wwino4", lambda spec: rec.calls.append("panel4x4") or spec.w)
    B, H, W, C, N = shape
    spec = packing.pack_conv(torch.zeros(N, C, 3, 3))
    x, y = torch.zeros(B, H, W, C), torch.zeros(B, H, W, N)
    hook = []
    monkeypatch.setattr(ops, "CONV_HOOK", lambda begin, M, s, epi, info: hook.append(info))
    with ops.conv_precision("winograd"), ops.train_conv_tiles(tiles):
        REAL_CONV2D(x, spec, y, splitk=splitk, **kw)
    return rec.calls, hook[-1]


def test_switch_off_calls_what_the_parent_calls(monkeypatch):
    """With conv_tiles = "2x2" a training launch asks the F(2x2) plan and runs the F(2x2) split form - the calls of the code before the switch existed -
    on a library that does not have the new functions at all."""
    calls, info = _launch(monkeypatch, "2x2", missing=NEW)
    assert calls == ["lwg_conv2d_winograd_plan", "panel2x2", "lwg_conv2d_winograd_f32_ws"]
    assert info == {"kernels": 2, "kind": "winograd"}
    assert not set(calls) & set(NEW)


def test_switch_off_synthesis_and_small_launches(monkeypatch):
    calls, info = _launch(monkeypatch, "2x2", splitk=False, missing=NEW)                        # the synthesis path: F(4x4) whole, as ever
    assert calls == ["panel4x4", "lwg_conv2d_winograd4_f32"] and info == {"kernels": 1, "kind": "winograd4"}
    calls, info = _launch(monkeypatch, "2x2", shape=(1, 8, 8, 64, 64), missing=NEW)             # too small for the Winograd kernels: direct
    assert calls == ["lwg_conv2d_winograd_plan", "lwg_conv2d_ws_floats", "lwg_conv2d_nhwc_f32_ws", "lwg_conv_slice_count"] and info["kind"] == "direct"
    assert not set(calls) & set(NEW)


def test_switch_on_routes_through_the_f44_plan(monkeypatch):
    """ops._wino4_plan takes the library's split form where every slice keeps >= 128 input channels, its whole form on launches of more than 128
    units, and hands every other launch to the parent's plan unchanged."""
    calls, info = _launch(monkeypatch, "4x4", shape=(2, 64, 64, 256, 256))                      # 128 blocks of 32 channels, 2 slices of 128 channels
    assert calls == ["lwg_conv2d_winograd4_plan", "panel4x4", "lwg_conv2d_winograd4_f32_ws"] and info == {"kernels": 2, "kind": "winograd4"}
    calls, info = _launch(monkeypatch, "4x4", shape=(1, 128, 128, 128, 256))                    # 256 blocks of 32 channels: whole
    assert calls == ["lwg_conv2d_winograd4_plan", "panel4x4", "lwg_conv2d_winograd4_f32"] and info == {"kernels": 1, "kind": "winograd4"}
    calls, info = _launch(monkeypatch, "4x4", splitk=False)                                     # the synthesis path does not read the switch
    assert calls == ["panel4x4", "lwg_conv2d_winograd4_f32"] and info == {"kernels": 1, "kind": "winograd4"}
    calls, info = _launch(monkeypatch, "4x4", shape=(1, 32, 32, 32, 64))                        # Cin < WINO4_MIN_CIN: the parent's choice
    assert "lwg_conv2d_winograd4_plan" not in calls and calls[0] == "lwg_conv2d_winograd_plan"
    parent = ["lwg_conv2d_winograd_plan", "panel2x2", "lwg_conv2d_winograd_f32_ws"]
    calls, info = _launch(monkeypatch, "4x4")                                                   # 4 slices of 64 channels: declined, the parent's choice
    assert calls == ["lwg_conv2d_winograd4_plan"] + parent and info == {"kernels": 2, "kind": "winograd"}
    monkeypatch.setattr(ops, "WINO4_TRAIN_MIN_SLICE_CIN", 0)
    monkeypatch.setattr(ops, "WINO4_TRAIN_MIN_GRID", 0)
    calls, info = _launch(monkeypatch, "4x4")                                                   # (the thresholds off: the same launch split)
    assert calls == ["lwg_conv2d_winograd4_plan", "panel4x4", "lwg_conv2d_winograd4_f32_ws"] and info == {"kernels": 2, "kind": "winograd4"}
    monkeypatch.setattr(ops, "WINO4_TRAIN_SPLITK", False)
    assert _launch(monkeypatch, "4x4")[0] == ["lwg_conv2d_winograd4_plan"] + parent


def test_panel_cache_f44_half(monkeypatch):
    """PanelCache.winograd4: a fragment panel once per (GEMM panel, tap order), registered for the per-step refresh only when the source weight
    trains; refresh() hands lwg_winograd4_panels_f32 one LwgWinoDesc per registered panel, blocks of 64 columns x 4 input channels, behind the
    F(2x2) launch; a frozen weight written in place is re-derived; invalidate() forgets everything."""
    flat = torch.zeros(64 * 64 * 9, requires_grad=True)
    w = flat.detach().view(64, 64, 3, 3)
    frozen = torch.zeros(128, 64, 3, 3)
    cache = ops.PanelCache([flat, frozen])
    calls = []

    class _Stub:
        def __getattr__(self, name):
            def call(*args):
                calls.append((name,) + tuple(a for a in args if isinstance(a, int)))
                return 0
            return call
    monkeypatch.setattr(_lib, "lib", lambda: _Stub())
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_ptr", lambda t, dt=None: 0 if t is None else t.data_ptr())
    pa, _ = cache.get(w, False, tuple(range(9)), 64, 64, 64, 64)
    pt, _ = cache.get(w, True, tuple(reversed(range(9))), 64, 64, 64, 64)
    pf, _ = cache.get(frozen, False, tuple(range(9)), 64, 64, 128, 128)

    class _Spec:
        def __init__(self, panel, cin):
            self.w, self.Cin = panel, cin
    taps, rtaps = list(range(9)), list(reversed(range(9)))
    ua = cache.winograd4(_Spec(pa, 64), taps)
    assert cache.winograd4(_Spec(pa, 64), taps) is ua and ua.shape == (4, 8, 4, 2, 9 * 64)
    ut = cache.winograd4(_Spec(pt, 64), rtaps)
    uf = cache.winograd4(_Spec(pf, 64), taps)
    assert uf.shape == (4, 8, 4, 2, 9 * 128) and cache.winograd4(_Spec(torch.zeros(144, 64, 4), 64), taps) is None
    assert [c[0] for c in calls] == ["lwg_winograd4_panel_f32"] * 3
    assert len(cache.wino4_rows) == 2 and not cache.wino_rows
    u2 = cache.winograd(_Spec(pa, 64), taps)                                                    # the F(2x2) panel of the same weight, side by side
    assert u2.shape == (16, 8, 2, 64, 4) and len(cache.wino_rows) == 1
    calls.clear()
    cache.refresh()
    cache.refresh()
    assert [c[0] for c in calls] == ["lwg_pack_panels_f32", "lwg_winograd_panels_f32", "lwg_winograd4_panels_f32"] * 2
    per = ((64 + 63) // 64) * ((64 + 3) // 4)
    assert calls[2][-2:] == (2, 2 * per) and calls[2] == calls[5]                               # the table is built once
    descs = (_lib.LwgWinoDesc * 2).from_buffer_copy(bytes(cache.wino4_table.numpy().tobytes()))
    assert [d.first_block for d in descs] == [0, per]
    assert descs[0].wpanel == pa.data_ptr() and descs[0].upk == ua.data_ptr() and descs[1].upk == ut.data_ptr() and list(descs[1].tap9) == rtaps
    assert (descs[0].Cin, descs[0].N) == (64, 64)
    calls.clear()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    frozen.add_(1.0)                                                                            # an in-place load_state_dict of a loss network
    cache.refresh()
    assert [c[0] for c in calls][:2] == ["lwg_pack_panel_f32", "lwg_winograd4_panel_f32"]
    cache.invalidate()
    assert not cache.wino4 and not cache.wino4_rows and cache.wino4_table is None and cache.wino4_blocks == 0
