"""The opt-in F(2x2, 3x3) Winograd weight gradient (csrc/conv_wgrad_winograd.hip) - the parts that need no GPU: the identity the kernel
implements, the host contract of its C entry point and the defaults of its switches."""
import pytest
import torch

from ipercore_amd import _lib, ops
from ipercore_amd.trainers import TrainOpts
from tests import wgradwino_emu as emu


@pytest.mark.parametrize("shape", [(3, 9, 7, 5, 6), (2, 8, 8, 4, 3), (1, 3, 5, 2, 2), (1, 1, 1, 3, 2), (2, 6, 11, 3, 4)])
def test_emulation_equals_conv2d_weight_in_fp64(shape):
    """dw = G^T (sum_t (B^T d_t B) (A dy_t A^T)) G is torch.nn.grad.conv2d_weight of a 3x3 / stride 1 / pad 1 convolution: pins the three matrices,
    the halo and the zero padding of ragged (odd H / W) tiles.  fp64: 1e-12 relative L2 (the identity is exact; measured 3e-16 - 5e-16)."""
    B, H, W, C, N = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    dy = torch.randn(B, H, W, N, generator=g, dtype=torch.float64)
    ref = emu.reference(x, dy)
    for chunk in (None, 8):
        got = emu.wgrad(x, dy, chunk=chunk)
        assert got.shape == (N, C, 3, 3)
        assert float((got - ref).norm() / ref.norm()) <= 1e-12


def _valid_args(bad):
    a = _lib.LwgConvArgs()
    a.x0 = bad
    a.B, a.H, a.W, a.C0, a.C1, a.OH, a.OW, a.M, a.N, a.YH, a.YW, a.YC = 1, 8, 8, 64, 0, 8, 8, 64, 64, 8, 8, 64
    a.ntaps, a.stride, a.omul = 9, 1, 1
    for t in range(9):
        a.dy[t], a.dx[t] = t // 3 - 1, t % 3 - 1
    return a


def test_host_contract_rejects_before_any_launch():
    """lwg_conv2d_wgrad_winograd_f32 validates on the host and returns hipErrorInvalidValue (1) before any launch: the pointers are never
    dereferenced and no GPU is touched.  (Fails on a library without the symbol.)"""
    L = _lib.lib()
    bad = 0xdead0000
    assert L.lwg_conv2d_wgrad_winograd_ws_floats(None) == 0
    assert L.lwg_conv2d_wgrad_winograd_f32(None, bad, bad, bad, 64, 64, None) == 1
    a = _valid_args(bad)
    assert L.lwg_conv2d_wgrad_winograd_ws_floats(a) % (16 * 64 * 64) == 0 and L.lwg_conv2d_wgrad_winograd_ws_floats(a) > 0    # the base case is inside the contract
    assert L.lwg_conv2d_wgrad_winograd_f32(a, None, bad, bad, 64, 64, None) == 1       # NULL dy
    assert L.lwg_conv2d_wgrad_winograd_f32(a, bad, None, bad, 64, 64, None) == 1       # NULL ws
    assert L.lwg_conv2d_wgrad_winograd_f32(a, bad, bad, None, 64, 64, None) == 1       # NULL dw
    assert L.lwg_conv2d_wgrad_winograd_f32(a, bad, bad, bad, 65, 64, None) == 1        # cin > C0 + C1
    assert L.lwg_conv2d_wgrad_winograd_f32(a, bad, bad, bad, 64, 0, None) == 1         # nout < 1

    def rejected(**kw):
        b = _valid_args(bad)
        for k, v in kw.items():
            setattr(b, k, v)
        return L.lwg_conv2d_wgrad_winograd_f32(b, bad, bad, bad, 64, 32, None) == 1 and L.lwg_conv2d_wgrad_winograd_ws_floats(b) == 0

    assert rejected(x0=None)
    assert rejected(C0=96)
    assert rejected(N=32, YC=32)
    assert rejected(stride=2)
    assert rejected(ntaps=4)
    assert rejected(OH=4, M=32)                    # OH != H
    assert rejected(C1=64)                         # a second input without its pointer
    assert rejected(C1=32, x1=bad)                 # C1 % 64
    assert rejected(omul=2)
    assert rejected(xdt=_lib.DT_BF16)
    assert rejected(YC=32)                         # ycoff + N > YC
    assert rejected(B=1 << 12, H=1 << 10, W=1 << 10, OH=1 << 10, OW=1 << 10, YH=1 << 10, YW=1 << 10, M=1 << 30)     # beyond 32-bit buffer offsets
    b = _valid_args(bad)
    b.dy[0], b.dy[8] = 1, -1                       # the nine taps, but not in ascending (dy, dx) order
    assert L.lwg_conv2d_wgrad_winograd_f32(b, bad, bad, bad, 64, 64, None) == 1


def test_switch_defaults_and_context_manager():
    assert ops.WGRAD_PRECISION == "direct"
    assert TrainOpts().wgrad_precision == "direct"
    with ops.wgrad_precision("winograd"):
        assert ops.WGRAD_PRECISION == "winograd"
        with ops.wgrad_precision("direct"):
            assert ops.WGRAD_PRECISION == "direct"
        assert ops.WGRAD_PRECISION == "winograd"
    assert ops.WGRAD_PRECISION == "direct"
    with pytest.raises(ZeroDivisionError):
        with ops.wgrad_precision("winograd"):
            1 / 0
    assert ops.WGRAD_PRECISION == "direct"
    with pytest.raises(AssertionError):
        ops.wgrad_precision("bf16")


def test_cpu_tensors_are_never_eligible():
    """The predicate requires device tensors: the host-logic tests over the emulated ABI keep the direct two-step form in either mode."""
    from ipercore_amd.networks import packing
    w = torch.randn(64, 64, 3, 3)
    spec = packing.pack_conv(w)
    x, dy = torch.randn(1, 8, 8, 64), torch.randn(1, 8, 8, 64)
    assert not ops._wgrad_wino_use(x, spec, dy, None)
    with ops.wgrad_precision("winograd"):
        assert not packing.wgrad_conv_is_winograd(x, spec, dy, None, 3, 3)
