"""The opt-in bf16-operand forward / data-gradient convolution (csrc/conv_igemm_bf16op.hip) - the parts that need no GPU: its
definition and the two derived error bounds (tests/convbf16op_emu.py) on the GPU test's matrix, the host contract of the three C entry points, the
split plan's answers, the mode switch, the Python eligibility rule and the documentation of the trainer option."""
import os
import re
import types

import pytest
import torch

from ipercore_amd import _lib, ops
from ipercore_amd.trainers import TrainOpts
from tests import convbf16op_emu as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ids(v):
    return "x".join(map(str, v[0])) + "_k%ds%d" % v[1][:2] if isinstance(v, tuple) and isinstance(v[0], tuple) else str(v)


def _check_emulation(x, w, bias, geom, tag, act=emu.ACT_NONE, res=None):
    k, stride, pad = geom
    kw = dict(k=k, stride=stride, pad=pad, act=act, res=res)
    got = emu.emulate(x, w, bias, **kw)
    ref, rref = emu.reference(x, w, bias, **kw), emu.rounded_reference(x, w, bias, **kw)
    bnds = emu.bounds(x, w, bias, k, stride, pad, res=None if act == emu.ACT_RELU_MASK else res)
    where = None if act != emu.ACT_RELU_MASK else (res > 0)
    ok, fa, fr = emu.inside(got, ref, rref, bnds, where)
    print(f"conv_bf16op emulation {tag}: err / accumulation bound {fa:.3e}, err / rounding bound {fr:.3e}, "
          f"rel L2 vs fp64 {float((got.double() - ref).norm() / ref.norm()):.3e}")
    assert torch.isfinite(got).all() and ok, (tag, fa, fr)
    if where is not None:
        assert bool((got[~where] == 0).all())


@pytest.mark.parametrize("case", emu.MATRIX + emu.SPLITK, ids=_ids)
def test_emulation_meets_both_bounds(case):
    shape, geom, _ = case
    x, w, bias, _ = emu.case(shape, geom)
    small = shape[1] * shape[2] <= 1024
    for b in ((bias, None) if small else (bias,)):
        for act in ((emu.ACT_NONE, emu.ACT_RELU) if small else (emu.ACT_RELU,)):
            _check_emulation(x, w, b, geom, f"{case} bias={b is not None} act={act}", act)


@pytest.mark.parametrize("kind", emu.KINDS)
def test_emulation_meets_both_bounds_on_the_operand_kinds(kind):
    shape, geom, _ = emu.KINDS_SHAPE
    x, w, bias, _ = emu.case(shape, geom, kind)
    _check_emulation(x, w, bias, geom, kind)


def test_emulation_of_the_relu_mask_and_the_residual():
    shape, geom, _ = emu.MASK_SHAPE
    x, w, bias, res = emu.case(shape, geom)
    _check_emulation(x, w, None, geom, "relu mask", emu.ACT_RELU_MASK, res)
    _check_emulation(x, w, bias, geom, "residual", emu.ACT_NONE, res)


def test_emulation_of_the_parity_forms():
    g = torch.Generator().manual_seed(77)
    for name, x, w, op in (("conv_transpose (1,8,8,64)", torch.randn(1, 8, 8, 64, generator=g), 0.05 * torch.randn(64, 64, 4, 4, generator=g), 0),
                           ("dgrad 4x4 s2, H = W = 9", torch.randn(2, 4, 4, 64, generator=g), 0.05 * torch.randn(64, 64, 4, 4, generator=g), 1)):
        got = emu._convt(emu.rounded(x), emu.rounded(w), torch.float32, op)
        ok, fa, fr = emu.inside(got, emu.convt_reference(x, w, op), emu.convt_rounded_reference(x, w, op), emu.convt_bounds(x, w, op))
        print(f"conv_bf16op emulation {name}: err / accumulation bound {fa:.3e}, err / rounding bound {fr:.3e}")
        assert ok and got.shape[1] == 2 * x.shape[1] + op, (name, fa, fr)


def test_rounded_reference_is_the_reference_of_bf16_operands():
    x, w, bias, _ = emu.case((2, 9, 7, 32, 0, 64), (3, 1, 1))
    xr, wr = emu.rounded(x), emu.rounded(w)
    assert not torch.equal(xr, x) and torch.equal(emu.rounded(xr), xr)
    assert torch.equal(emu.rounded_reference(xr, wr, bias), emu.reference(xr, wr, bias))
    assert not torch.equal(emu.rounded_reference(x, w, bias), emu.reference(x, w, bias))
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20])      # ties go to the even neighbour
    assert emu.rounded(t).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]


NAMES = ("lwg_conv2d_nhwc_f32_bf16op", "lwg_conv2d_bf16op_ws_floats", "lwg_conv2d_nhwc_f32_bf16op_ws")


def test_symbols_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "lwg_hip.h")) as f:
        h = f.read()
    assert "#define LWG_ABI_VERSION 10" in h
    assert "int lwg_conv2d_nhwc_f32_bf16op(const LwgConvArgs* args, lwg_stream_t stream);" in h
    assert "size_t lwg_conv2d_bf16op_ws_floats(const LwgConvArgs* args);" in h
    assert "int lwg_conv2d_nhwc_f32_bf16op_ws(const LwgConvArgs* args, float* ws, lwg_stream_t stream);" in h
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib._SIGS and getattr(L, n) is not None, n


BAD = 0xdead0000                         # a non-NULL pointer that is never dereferenced


def _valid_args(**kw):
    """3x3 / stride 1 / pad 1, (1, 8, 8, 64) -> 64: inside the contract."""
    a = _lib.LwgConvArgs()
    a.x0 = a.w = a.y = BAD
    a.B, a.H, a.W, a.C0, a.C1, a.OH, a.OW, a.M, a.N, a.YH, a.YW, a.YC = 1, 8, 8, 64, 0, 8, 8, 64, 64, 8, 8, 64
    a.ntaps, a.stride, a.omul = 9, 1, 1
    for t in range(9):
        a.dy[t], a.dx[t] = t // 3 - 1, t % 3 - 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_host_contract_rejects_before_any_launch():
    """Every contract violation is hipErrorInvalidValue (1) from the host checks - the pointers are never dereferenced, no GPU is touched - through
    both launching entry points."""
    L = _lib.lib()
    assert L.lwg_conv2d_nhwc_f32_bf16op(None, None) == 1 and L.lwg_conv2d_nhwc_f32_bf16op_ws(None, BAD, None) == 1

    def rejected(**kw):
        a = _valid_args(**kw)
        return L.lwg_conv2d_nhwc_f32_bf16op(a, None) == 1 and L.lwg_conv2d_nhwc_f32_bf16op_ws(a, BAD, None) == 1

    assert rejected(x0=None) and rejected(w=None) and rejected(y=None)              # NULL pointers
    assert rejected(N=32, YC=32) and rejected(N=96, YC=96)                          # N % 64
    assert rejected(C0=48) and rejected(C0=8)                                       # Cin % 32 (the small-Cin first layers keep the fp32 kernel)
    assert rejected(C0=32, C1=32)                                                   # a second input without its pointer
    assert rejected(C0=48, C1=16, x1=BAD)                                           # C0 % 32
    assert rejected(xdt=_lib.DT_BF16) and rejected(ydt=_lib.DT_BF16)                # bf16 tensors
    assert rejected(epi=_lib.EPI_SPADE, N=128, xn=BAD, mean=BAD, rstd=BAD, bias=BAD)      # SPADE (a complete SPADE description)
    assert rejected(ydt=_lib.DT_F32_Q4)                                             # channel-quad planes
    assert rejected(ntaps=53) and rejected(ntaps=0)                                 # ntaps > LWG_MAX_TAPS (52)
    assert rejected(epi=_lib.EPI_RESIDUAL)                                          # a residual without its tensor
    assert rejected(act=_lib.ACT_RELU_MASK)                                         # the ReLU mask without a residual
    assert rejected(M=0) and rejected(YC=66) and rejected(ycoff=2, YC=128)
    assert rejected(H=1 << 14, W=1 << 14, OH=1 << 14, OW=1 << 14, YH=1 << 14, YW=1 << 14, M=1 << 28)     # one frame beyond 32-bit buffer offsets


def _launch(B, H, W, Cin, N, ntaps=9, **kw):
    a = _valid_args(B=B, H=H, W=W, C0=Cin, OH=H, OW=W, YH=H, YW=W, M=B * H * W, N=N, YC=N, **kw)
    a.ntaps = ntaps
    return a


def test_split_plan_answers():
    L = _lib.lib()
    f = L.lwg_conv2d_bf16op_ws_floats
    assert f(None) == 0
    one = _launch(1, 16, 16, 512, 512)
    assert f(_launch(1, 16, 16, 512, 512, epi=_lib.EPI_RESIDUAL, res=BAD)) == 0                 # a fused residual runs whole
    assert f(_launch(1, 16, 16, 512, 512, epi=_lib.EPI_RESIDUAL, res=BAD, act=_lib.ACT_RELU_MASK)) == f(one) > 0       # ... the ReLU mask splits
    assert f(_launch(4, 128, 128, 128, 128)) == 0                                               # 512 tiles of 128 x 128: fills the chip
    assert f(_launch(1, 16, 16, 32, 64)) == 0                                                   # one chunk: nothing to split
    for B, H, W, Cin, N in ((1, 16, 16, 512, 512), (1, 64, 64, 256, 256)):                      # the one-sample shapes of the GPU test
        n = f(_launch(B, H, W, Cin, N))
        mn = B * H * W * N
        assert n > mn and n % mn == 0 and n // mn <= 8, (B, H, W, Cin, N, n)
        assert n // mn <= Cin // 32                                                            # whole 32-channel chunks


def test_mode_enters_and_restores():
    assert ops.CONV_PRECISION == "fp32"
    with ops.conv_precision("winograd"):
        with ops.conv_precision("bf16_operands"):
            assert ops.CONV_PRECISION == "bf16_operands"
        assert ops.CONV_PRECISION == "winograd"
    with pytest.raises(ZeroDivisionError):
        with ops.conv_precision("bf16_operands"):
            1 / 0
    assert ops.CONV_PRECISION == "fp32" and ops._MODE_WINO4
    with pytest.raises(AssertionError):
        ops.conv_precision("bf16_operand")


def _spec(cin, n, ntaps=9, stride=1, omul=1):
    return types.SimpleNamespace(Cin=cin, N=n, ntaps=ntaps, stride=stride, omul=omul, ooy=0, oox=0)


def test_eligibility_rule():
    f32, bf = torch.float32, torch.bfloat16
    t = lambda *s, dt=f32: torch.empty(*s, dtype=dt)        # noqa: E731
    use = ops._bf16op_use
    assert use(_spec(64, 64), t(1, 8, 8, 64), t(1, 8, 8, 64))
    assert use(_spec(64, 128, 16, stride=2), t(1, 16, 16, 64), t(1, 8, 8, 128))                                 # 4x4 / stride 2
    assert use(_spec(96, 64, 1), t(2, 8, 8, 96), t(2, 8, 8, 64))                                                # 1x1
    assert use(_spec(64, 64, 4, omul=2), t(1, 8, 8, 64), t(1, 16, 16, 64))                                      # a parity launch
    assert use(_spec(128, 64), t(1, 8, 8, 32), t(1, 8, 8, 64), t(1, 8, 8, 96))                                  # two inputs, 32-granular
    assert use(_spec(64, 64), t(1, 8, 8, 64), t(1, 8, 8, 128), ycoff=64)                                        # a slice of a wider output
    assert use(_spec(64, 64), t(1, 8, 8, 64), t(1, 8, 8, 64), epi=ops.EPI_RESIDUAL, act=ops.ACT_RELU_MASK)
    assert use(_spec(64, 64), t(1, 8, 8, 64), t(1, 8, 8, 64), epi=ops.EPI_RESIDUAL, act=ops.ACT_RELU)
    assert not use(_spec(8, 64), t(1, 8, 8, 8), t(1, 8, 8, 64))                                                 # Cin 8
    assert not use(_spec(48, 64), t(1, 8, 8, 48), t(1, 8, 8, 64))
    assert not use(_spec(64, 32), t(1, 8, 8, 64), t(1, 8, 8, 32))                                               # N % 64
    assert not use(_spec(64, 128), t(1, 8, 8, 64), t(1, 8, 8, 64), epi=ops.EPI_SPADE)
    assert not use(_spec(64, 64), t(1, 8, 8, 64), t(1, 16, 8, 8, 4), q4=True)
    assert not use(_spec(64, 64), t(1, 8, 8, 64), t(1, 8, 8, 64), act=ops.ACT_RELU_MASK)                        # the mask without a residual
    assert not use(_spec(64, 64), t(1, 8, 8, 64, dt=bf), t(1, 8, 8, 64, dt=bf))
    assert not use(_spec(64, 64), t(1, 8, 8, 64), t(1, 8, 8, 64, dt=bf))
    assert not use(_spec(64, 64), t(1, 8, 8, 48), t(1, 8, 8, 64), t(1, 8, 8, 16))                               # C0 % 32
    assert not use(_spec(64, 64), t(1, 8, 8, 64), t(1, 8, 8, 128), ycoff=2)
    # a rule on the launch description: the batch and the image size have no say
    assert use(_spec(64, 64), t(7, 3, 5, 64), t(7, 3, 5, 64)) and use(_spec(64, 64), t(1, 128, 128, 64), t(1, 128, 128, 64))


def test_parity_group_rule():
    """ops._bf16op_use_parity4: a group that "fp32" runs as one grid AND whose parity launches the plan splits keeps the "fp32" form - asked of the
    library through the same two host functions; everything else the launch rule admits stays in the mode."""
    L = _lib.lib()

    def lib_says(B, H, W, Cin, N):
        a = _launch(B, H, W, Cin, N, ntaps=4)
        return bool(L.lwg_conv_transpose4_is_one_grid(a)) and L.lwg_conv2d_bf16op_ws_floats(a) > 0

    assert lib_says(1, 64, 64, 256, 128) and lib_says(1, 32, 32, 512, 256) and lib_says(1, 128, 128, 128, 64)        # three of the step's seven losers
    assert not lib_says(1, 128, 128, 256, 128) and not lib_says(2, 64, 64, 256, 256)      # one grid, run whole: gains (0.57, 0.56)
    assert not lib_says(1, 256, 256, 128, 64)                                             # four direct launches in the default mode
    # the Python side without a device: a group the launch rule refuses is refused; without splitk the plan is not consulted
    specs = [types.SimpleNamespace(Cin=64, N=64, ntaps=4, stride=1, omul=2, ooy=i >> 1, oox=i & 1) for i in range(4)]
    x, y = torch.empty(1, 8, 8, 64), torch.empty(1, 16, 16, 64)
    assert ops._bf16op_use_parity4(specs, x, y) and ops._bf16op_use_parity4(specs, x, y, splitk=True)      # (CPU tensors: never the one-grid form)
    assert not ops._bf16op_use_parity4(specs, x, torch.empty(1, 16, 16, 16, 4), q4=True)
    import inspect
    assert "1.07 - 1.41" in inspect.getdoc(ops._bf16op_use_parity4)


def test_trainer_drops_the_panel_cache_on_a_precision_switch():
    """LWGTrainer._sync_modes on a bare trainer: a change of conv_precision or conv_tiles empties the panel cache exactly once and drops the
    captured graphs, a change of wgrad_precision drops the graphs and leaves the cache, an unchanged step does neither."""
    from ipercore_amd.trainers import LWGTrainer

    class _Cache:
        n = 0

        def invalidate(self):
            self.n += 1
    tr = LWGTrainer.__new__(LWGTrainer)
    tr.opts, tr._panel_cache, graphs = TrainOpts(), _Cache(), {"A": object()}

    def step(**changes):
        for k, v in changes.items():
            assert getattr(tr.opts, k) != v
            setattr(tr.opts, k, v)
        tr._graphs, before = graphs, tr._panel_cache.n
        tr._sync_modes()
        return tr._panel_cache.n - before, tr._graphs is None

    assert step() == (0, False) and step() == (0, False)                    # the first step has nothing to compare with; an unchanged one
    assert step(conv_precision="bf16_operands") == (1, True)
    assert step() == (0, False)
    assert step(conv_tiles="4x4") == (1, True)
    assert step(wgrad_precision="bf16") == (0, True)
    assert step(wgrad_precision="winograd") == (0, True)
    assert step() == (0, False)
    assert step(conv_precision="winograd", conv_tiles="2x2") == (1, True)   # both at once: still one invalidation
    assert step(conv_precision="fp32", wgrad_precision="direct") == (1, True)
    assert step() == (0, False)
    tr._panel_cache = None                                                  # no panel cache (use_panel_cache off): the graphs still go
    assert tr.opts.conv_tiles == "2x2"
    tr.opts.conv_tiles, tr._graphs = "4x4", graphs
    tr._sync_modes()
    assert tr._graphs is None


def test_trainopts_documents_the_value():
    import inspect
    src = inspect.getsource(TrainOpts)
    assert TrainOpts().conv_precision == "winograd"
    doc = src[:src.index('conv_precision = "winograd"')]
    assert '"bf16_operands"' in doc and "opt-in" in doc and "wgrad_precision" in doc and "conv_tiles" in doc and "re-captures" in doc


def test_source_uses_the_shared_header():
    with open(os.path.join(ROOT, "ipercore_amd", "csrc", "conv_igemm_bf16op.hip")) as f:
        k = f.read()
    assert '#include "lwg_conv_direct.h"' in k and '#include "lwg_conv_epilogue.h"' in k
    assert not re.search(r"0xc0000000|3221225472", k, re.I)            # no buffer-range constant of its own
    assert "LWG_BUF_RANGE" in k and k.count("cd_sliced(a, ") == 1 and "cd_contract_ok(a, " in k and "cd_epilogue_ok(a, " in k
    assert "lwg_splitk_finish_launch(" in k and "atomicAdd" not in k
    with open(os.path.join(ROOT, "ipercore_amd", "csrc", "Makefile")) as f:
        assert "conv_igemm_bf16op.hip" in f.read()
