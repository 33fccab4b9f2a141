"""lwg_norm_fwd_nhwc_f32 / lwg_norm_bwd_nhwc_f32 (csrc/train_ops.hip) called directly with an explicit nsplit, against torch autograd in
float64 on the CPU, at the tolerances of check_train_ops (y 2e-5, dx 2e-4, dgamma / dbeta 2e-5 through _cmp).

The geometries reach what NormAct at 16x16 / 8x8 / 7x9 never does: 24 lanes per pixel with 16 idle threads and an empty last split, one
lane per pixel, a second channel block that is a quarter full, fold lanes that add several records, and nsplit > HW (empty splits whose
records the fold still reads: the workspace is NaN-filled, so a record nobody wrote poisons dx).  dy is N(0,1) in one run and, in another,
0 except 64.0 at one probe pixel per channel (tests/instnorm_emu.probe_pixels): a dropped pixel then removes the channel's whole sum."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ipercore_amd import _lib, ops
from tests import instnorm_emu as emu
from tests.gpu_checks import DEV, _cmp

pytestmark = pytest.mark.gpu

# (B, HW, C, nsplit of the backward's reduction pass)
GEOMETRIES = ((2, 35, 96, 8), (1, 63, 4, 64), (2, 1000, 320, 9), (1, 1000, 512, 24), (3, 576, 256, 7), (2, 300, 128, 512))
FUSED_GEOMETRIES = ((2, 35, 96, 8), (3, 150, 64, 7))        # C = 64: 16 lanes per pixel, 16 pixel groups, last split 18 of 22 pixels
ACTS = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU}
KINK = 1e-4     # no pre-activation closer to 0 than this: the kernels' fp32 z differs from the reference's by ~1e-6, and a ReLU whose mask flips is another function


def _randn(shape, *seed):
    return torch.from_numpy(np.random.default_rng(list(seed)).standard_normal(shape, dtype=np.float32))


def _z64(x, gm, bt):
    xh = F.instance_norm(x.double().permute(0, 2, 1), eps=1e-5).permute(0, 2, 1)
    return xh if gm is None else xh * (1 + gm.double()) + bt.double()


def _inputs(B, HW, C, spade):
    """x = 1.5 N(0,1) + 0.7 as in check_train_ops, gamma / beta = 0.5 N(0,1); then every element whose float64 pre-activation lies within
    KINK of 0 is moved away from it (beta where there is one, else x), so that ReLU / LeakyReLU are differentiable at every input."""
    x = _randn((B, HW, C), 900, B, HW, C) * 1.5 + 0.7
    gm, bt = (_randn((B, HW, C), 901, B, HW, C) * 0.5, _randn((B, HW, C), 902, B, HW, C) * 0.5) if spade else (None, None)
    for _ in range(20):
        z = _z64(x, gm, bt)
        near = z.abs() < KINK
        if not near.any():
            break
        (bt if spade else x)[near] += 0.01
    assert not (_z64(x, gm, bt).abs() < KINK).any()
    return x, gm, bt


def _dy(kind, B, HW, C, nsplit):
    if kind == "n01":
        return _randn((B, HW, C), 903, B, HW, C)
    lpp = min(C // 4, 64)
    probes = emu.probe_pixels(HW, nsplit, 256 // lpp)
    dy = torch.zeros(B, HW, C)
    for b in range(B):
        for c in range(C):
            dy[b, probes[(b * C + c) % len(probes)], c] = 64.0
    return dy


def _reference(x, gm, bt, act, dy):
    xr = x.double().requires_grad_(True)
    gr, br = (gm.double().requires_grad_(True), bt.double().requires_grad_(True)) if gm is not None else (None, None)
    xh = F.instance_norm(xr.permute(0, 2, 1), eps=1e-5).permute(0, 2, 1)
    z = xh if gm is None else xh * (1 + gr) + br
    y = {ops.ACT_NONE: lambda t: t, ops.ACT_RELU: F.relu, ops.ACT_LRELU: lambda t: F.leaky_relu(t, 0.2)}[act](z)
    (y * dy.double()).sum().backward()
    return y.detach(), xr.grad, (gr.grad if gm is not None else None), (br.grad if gm is not None else None)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _run(x, gm, bt, fused, act, dy, nsplit):
    """Statistics, forward and backward entry points with NaN-filled outputs and workspace -> y, dx, dgamma, dbeta (None without gamma)."""
    B, HW, C = x.shape
    L = _lib.lib()
    xd, dyd = x.to(DEV), dy.to(DEV)
    mean, rstd = _nan(B, C), _nan(B, C)
    ops.instnorm_stats(xd.view(B, 1, HW, C), mean, rstd, _nan(B * C * 64 * 3))
    y, dx, ws = _nan(B, HW, C), _nan(B, HW, C), _nan(B * (nsplit + 1) * C * 2)
    gp = bp = dgp = dbp = None
    gs = 0
    if gm is not None and fused:
        gb, dgb = torch.cat([gm, bt], dim=2).contiguous().to(DEV), _nan(B, HW, 2 * C)
        gp, bp, dgp, dbp, gs = gb.data_ptr(), gb.data_ptr() + 4 * C, dgb.data_ptr(), dgb.data_ptr() + 4 * C, 2 * C
    elif gm is not None:
        gd, bd, dg, db = gm.to(DEV), bt.to(DEV), _nan(B, HW, C), _nan(B, HW, C)
        gp, bp, dgp, dbp = gd.data_ptr(), bd.data_ptr(), dg.data_ptr(), db.data_ptr()
    _lib.check(L.lwg_norm_fwd_nhwc_f32(xd.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gp, bp, gs, B, HW, C, act, y.data_ptr(), ops._stream()),
               "lwg_norm_fwd_nhwc_f32")
    _lib.check(L.lwg_norm_bwd_nhwc_f32(dyd.data_ptr(), y.data_ptr(), xd.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gp, gs, B, HW, C, act, nsplit,
                                       dx.data_ptr(), dgp, dbp, ws.data_ptr(), ops._stream()), "lwg_norm_bwd_nhwc_f32")
    torch.cuda.synchronize()
    if gm is None:
        return y, dx, None, None
    return (y, dx, dgb[..., :C], dgb[..., C:]) if fused else (y, dx, dg, db)


def _check(got, want, what):
    for g, w, tol, name in zip(got, want, (2e-5, 2e-4, 2e-5, 2e-5), ("y", "dx", "dgamma", "dbeta")):
        assert (g is None) == (w is None)
        if g is not None:
            _cmp(g, w.float(), tol, f"{what} {name}")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("spade", (False, True), ids=("plain", "gamma_beta"))
@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "B%d_HW%d_C%d_ns%d" % g)
def test_norm_fwd_bwd_against_float64_autograd(geom, spade, act):
    B, HW, C, nsplit = geom
    x, gm, bt = _inputs(B, HW, C, spade)
    for kind in ("n01", "spike"):
        dy = _dy(kind, B, HW, C, nsplit)
        _check(_run(x, gm, bt, False, ACTS[act], dy, nsplit), _reference(x, gm, bt, ACTS[act], dy), f"{geom} {act} dy={kind}")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("geom", FUSED_GEOMETRIES, ids=lambda g: "B%d_HW%d_C%d_ns%d" % g)
def test_fused_gamma_beta_is_bitwise_the_two_tensor_form(geom, act):
    """gamma | beta as ONE (B, HW, 2C) tensor (gstride = 2C, dbeta = dgamma + C): against float64, and bit for bit what two dense tensors give."""
    B, HW, C, nsplit = geom
    x, gm, bt = _inputs(B, HW, C, True)
    for kind in ("n01", "spike"):
        dy = _dy(kind, B, HW, C, nsplit)
        fused, dense = _run(x, gm, bt, True, ACTS[act], dy, nsplit), _run(x, gm, bt, False, ACTS[act], dy, nsplit)
        _check(fused, _reference(x, gm, bt, ACTS[act], dy), f"fused {geom} {act} dy={kind}")
        for f, d, name in zip(fused, dense, ("y", "dx", "dgamma", "dbeta")):
            assert torch.equal(f, d), f"fused gamma | beta {geom} {act} dy={kind}: {name} differs from the two-tensor form"
