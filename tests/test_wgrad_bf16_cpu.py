"""The opt-in bf16-operand weight gradient (csrc/conv_wgrad_bf16.hip) - the parts that need no GPU: its definition and the two derived
error bounds (tests/wgradbf16_emu.py) on the GPU test's matrix, the host contract of the two C entry points, the switch, and the agreement of the
Python predicate with the library's."""
import ctypes
import types

import pytest
import torch

from ipercore_amd import _lib, ops
from ipercore_amd.trainers import TrainOpts
from tests import wgradbf16_emu as emu


def _ids(v):
    return "x".join(map(str, v[0])) + "_k%ds%d" % v[1][:2] if isinstance(v, tuple) and isinstance(v[0], tuple) else str(v)


def _check_emulation(x, dy, geom, tag):
    got = emu.emulate(x, dy, *geom).double()
    acc, rnd = emu.bounds(x, dy, *geom)
    ea, er = (got - emu.rounded_reference(x, dy, *geom)).abs(), (got - emu.reference(x, dy, *geom)).abs()
    ref = emu.reference(x, dy, *geom)
    print(f"wgrad_bf16 emulation {tag}: err / accumulation bound {float((ea / acc).max()):.3e}, err / rounding bound {float((er / rnd).max()):.3e}, "
          f"rel L2 vs fp64 {float((got - ref).norm() / ref.norm()):.3e}")
    assert torch.isfinite(got).all()
    assert bool((ea <= acc).all()) and bool((er <= rnd).all()), tag


@pytest.mark.parametrize("case", emu.MATRIX, ids=_ids)
def test_emulation_meets_both_bounds(case):
    shape, geom, drop = case
    x, dy, cin, nout = emu.case(shape, geom, drop)
    _check_emulation(x[..., :cin], dy[..., :nout], geom, str(case))


@pytest.mark.parametrize("kind", emu.KINDS)
def test_emulation_meets_both_bounds_on_the_operand_kinds(kind):
    shape, geom, _ = emu.KINDS_SHAPE
    x, dy, _, _ = emu.case(shape, geom, None, kind)
    _check_emulation(x, dy, geom, kind)


def test_rounded_reference_is_the_reference_of_bf16_operands():
    """Operands that are bf16-representable are their own rounding: the two references coincide exactly, and the rounding is idempotent."""
    x, dy, _, _ = emu.case((2, 9, 7, 32, 0, 64), (3, 1, 1))
    xr, dyr = emu.rounded(x), emu.rounded(dy)
    assert not torch.equal(xr, x) and torch.equal(emu.rounded(xr), xr)
    assert torch.equal(emu.rounded_reference(xr, dyr), emu.reference(xr, dyr))
    assert not torch.equal(emu.rounded_reference(x, dy), emu.reference(x, dy))
    # round to nearest even on a tie: 1 + 2^-8 lies halfway between the bf16 neighbours 1 and 1 + 2^-7 -> the even one, 1; 1 + 3 * 2^-8 -> 1 + 2^-6
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20])
    assert emu.rounded(t).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]


BAD = 0xdead0000                         # a non-NULL pointer that is never dereferenced


def _valid_args(**kw):
    """3x3 / stride 1 / pad 1, (1, 8, 8, 64) -> 64: inside the contract."""
    a = _lib.LwgConvArgs()
    a.x0 = BAD
    a.B, a.H, a.W, a.C0, a.C1, a.OH, a.OW, a.M, a.N, a.YH, a.YW, a.YC = 1, 8, 8, 64, 0, 8, 8, 64, 64, 8, 8, 64
    a.ntaps, a.stride, a.omul = 9, 1, 1
    for t in range(9):
        a.dy[t], a.dx[t] = t // 3 - 1, t % 3 - 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _call(a, dy=BAD, ws=BAD, dw=BAD, D0=64, D1=64, KH=3, KW=3, transposed=0, kidx=tuple(range(9)), cin=64, nout=64, db=None):
    arr = None if kidx is None else (ctypes.c_int * len(kidx))(*kidx)
    return _lib.lib().lwg_conv2d_wgrad_bf16_f32(a, dy, ws, dw, D0, D1, KH, KW, transposed, arr, cin, nout, db, None)


def test_host_contract_rejects_before_any_launch():
    """Both entry points validate on the host: 0 floats / hipErrorInvalidValue (1) before any launch - the pointers are never dereferenced and no
    GPU is touched.  (Fails on a library without the symbols.)"""
    L = _lib.lib()
    assert L.lwg_conv2d_wgrad_bf16_ws_floats(None) == 0
    assert _call(None) == 1
    a = _valid_args()
    n = L.lwg_conv2d_wgrad_bf16_ws_floats(a)
    assert n > 0 and n % ((9 * 64 + 1) * 64) == 0             # whole slabs: Ktot weight rows + the bias row
    assert _call(a, dy=None) == 1
    assert _call(a, ws=None) == 1
    assert _call(a, dw=None) == 1
    assert _call(a, kidx=None) == 1
    assert _call(a, cin=65) == 1                              # cin > C0 + C1
    assert _call(a, cin=0) == 1
    assert _call(a, nout=0) == 1
    assert _call(a, nout=65) == 1                             # nout > N
    assert _call(a, D0=63) == 1                               # nout > D0
    assert _call(a, D1=63) == 1                               # cin > D1
    assert _call(a, kidx=(0, 1, 2, 3, 4, 5, 6, 7, 9)) == 1    # a position outside KH KW

    def rejected(**kw):
        b = _valid_args(**kw)
        return _call(b, cin=32, nout=32) == 1 and L.lwg_conv2d_wgrad_bf16_ws_floats(b) == 0

    assert rejected(x0=None)
    assert rejected(C0=48)                                    # C0 % 32
    assert rejected(C0=8)                                     # the small-Cin first layers stay on the direct kernel
    assert rejected(C1=32)                                    # a second input without its pointer
    assert rejected(C1=16, x1=BAD)                            # C1 % 32
    assert rejected(N=32, YC=32)                              # N % 64
    assert rejected(ntaps=0)
    assert rejected(ntaps=53)
    assert rejected(stride=0)
    assert rejected(omul=2)                                   # a transposed convolution's parity launch
    assert rejected(ooy=1)
    assert rejected(YH=16)                                    # dy is not dense
    assert rejected(M=32)                                     # M != B OH OW
    assert rejected(xdt=_lib.DT_BF16)
    assert rejected(ydt=_lib.DT_BF16)
    assert rejected(YC=32)                                    # ycoff + N > YC
    assert rejected(YC=66)                                    # YC % 4
    assert rejected(B=1 << 12, H=1 << 10, W=1 << 10, OH=1 << 10, OW=1 << 10, YH=1 << 10, YW=1 << 10, M=1 << 30)     # beyond 32-bit buffer offsets
    # ... and the clauses the contract leaves free are accepted: any taps, stride 2, a second 32-granular input, a slice of a wider dy
    for kw in (dict(stride=2, OH=4, OW=4, YH=4, YW=4, M=16), dict(ntaps=1), dict(ntaps=16), dict(C0=32, C1=96, x1=BAD), dict(YC=128, ycoff=64)):
        assert L.lwg_conv2d_wgrad_bf16_ws_floats(_valid_args(**kw)) > 0, kw


def test_switch_nests_and_restores():
    assert ops.WGRAD_PRECISION == "direct" and TrainOpts().wgrad_precision == "direct"
    with ops.wgrad_mode("bf16"):
        assert ops.WGRAD_PRECISION == "bf16"
        with ops.wgrad_precision("winograd"):
            assert ops.WGRAD_PRECISION == "winograd"
            with ops.wgrad_precision("direct"):
                assert ops.WGRAD_PRECISION == "direct"
            assert ops.WGRAD_PRECISION == "winograd"
        assert ops.WGRAD_PRECISION == "bf16"
    assert ops.WGRAD_PRECISION == "direct"
    with pytest.raises(ZeroDivisionError):
        with ops.wgrad_mode("bf16"):
            1 / 0
    assert ops.WGRAD_PRECISION == "direct"
    with pytest.raises(AssertionError):
        ops.wgrad_mode("fp16")
    with pytest.raises(AssertionError):
        ops.wgrad_precision("bf16")                  # the older switch keeps its two names; wgrad_mode is the one that knows the third


def _spec(cin, n, taps, stride=1, omul=1, ooy=0, oox=0):
    return types.SimpleNamespace(Cin=cin, N=n, ntaps=len(taps), stride=stride, omul=omul, ooy=ooy, oox=oox, cshift=0,
                                 dy=[t[0] for t in taps], dx=[t[1] for t in taps])


def _args_of(xs, spec, dys, x1s):
    """The launch description ops.conv_args builds for tensors of these shapes (fp32, ycoff 0)."""
    a = _lib.LwgConvArgs()
    a.x0, a.x1 = BAD, (BAD if x1s is not None else None)
    a.B, a.H, a.W, a.C0 = xs
    a.C1 = 0 if x1s is None else x1s[3]
    a.YH, a.YW, a.YC = dys[1:]
    a.OH, a.OW = a.YH // spec.omul, a.YW // spec.omul
    a.M, a.N = a.B * a.OH * a.OW, spec.N
    a.stride, a.ntaps, a.omul, a.ooy, a.oox = spec.stride, spec.ntaps, spec.omul, spec.ooy, spec.oox
    for i in range(spec.ntaps):
        a.dy[i], a.dx[i] = spec.dy[i], spec.dx[i]
    return a


T3 = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
T4 = [(dy, dx) for dy in (-1, 0, 1, 2) for dx in (-1, 0, 1, 2)]
LAUNCHES = [  # (x0 shape, spec, dy shape, x1 shape or None, inside the contract)
    ((1, 8, 8, 64), _spec(64, 64, T3), (1, 8, 8, 64), None, True),
    ((2, 9, 7, 32), _spec(128, 64, T3), (2, 9, 7, 64), (2, 9, 7, 96), True),           # two inputs, 32-granular
    ((1, 8, 8, 48), _spec(48, 64, T3), (1, 8, 8, 64), None, False),                    # C0 % 32
    ((1, 8, 8, 64), _spec(80, 64, T3), (1, 8, 8, 64), (1, 8, 8, 16), False),           # C1 % 32
    ((1, 8, 8, 64), _spec(64, 32, T3), (1, 8, 8, 32), None, False),                    # N % 64
    ((1, 8, 8, 64), _spec(64, 96, T3), (1, 8, 8, 96), None, False),
    ((2, 9, 9, 64), _spec(64, 64, T3, stride=2), (2, 5, 5, 64), None, True),           # stride 2
    ((1, 16, 16, 64), _spec(64, 128, T4, stride=2), (1, 8, 8, 128), None, True),       # 4x4 / stride 2
    ((2, 8, 8, 96), _spec(96, 64, [(0, 0)]), (2, 8, 8, 64), None, True),               # 1x1
    ((1, 8, 8, 64), _spec(64, 64, [(0, 0), (0, -1), (-1, 0), (-1, -1)], omul=2), (1, 16, 16, 64), None, False),    # a parity launch of a transposed conv
    ((1, 8, 8, 8), _spec(8, 64, T3), (1, 8, 8, 64), None, False),                      # small Cin
    ((1, 16, 16, 64), _spec(64, 64, T4, stride=2), (1, 8, 8, 64), None, True),         # a transposed convolution's adjoint form: 16 taps, stride 2
    ((4096, 1024, 1024, 64), _spec(64, 64, T3), (4096, 1024, 1024, 64), None, False),  # beyond 32-bit buffer offsets
    ((1, 1024, 1024, 32), _spec(32, 1024, T3), (1, 1024, 1024, 1024), None, False),    # ... dy alone beyond them
]


def test_python_predicate_agrees_with_the_library():
    """ops._wgrad_bf16_use's shape clauses (the device / dtype clauses need tensors) against lwg_conv2d_wgrad_bf16_ws_floats != 0, launch by launch."""
    L = _lib.lib()
    for xs, spec, dys, x1s, want in LAUNCHES:
        py = ops._wgrad_bf16_shapes_ok(xs, spec, dys, x1s)
        c = L.lwg_conv2d_wgrad_bf16_ws_floats(_args_of(xs, spec, dys, x1s)) != 0
        assert py == c == want, (xs, dys, x1s, py, c, want)


def test_cpu_tensors_are_never_eligible():
    """The predicate requires device tensors: the host-logic tests over the emulated ABI keep the direct two-step form in every mode."""
    from ipercore_amd.networks import packing
    spec = packing.pack_conv(torch.randn(64, 64, 3, 3))
    x, dy = torch.randn(1, 8, 8, 64), torch.randn(1, 8, 8, 64)
    assert ops._wgrad_bf16_shapes_ok(tuple(x.shape), spec, tuple(dy.shape)) and not ops._wgrad_bf16_use(x, spec, dy, None)
