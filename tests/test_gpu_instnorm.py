"""The InstanceNorm kernels of csrc/norm.hip called directly, on ragged splits and ill-conditioned data: statistics (the three vector
widths, the generic-C kernel, bf16) against float64 statistics of the same values under the bounds of tests/instnorm_emu.py, batch
invariance bit for bit, the host-side refusals, and the apply kernel against float64 evaluated with the kernel's own mean / rstd.

The geometries reach what the shapes of check_instnorm never do: splits shorter than a pixel group, a partly filled last group, the tail
loop after the four-in-flight iterations, empty trailing splits, B > 1 with nsplit > 1, and nsplit > 64 (the serial pre-merge)."""
import functools

import numpy as np
import pytest
import torch

from ipercore_amd import _lib, ops
from tests import instnorm_emu as emu
from tests.gpu_checks import DEV, _cmp

pytestmark = pytest.mark.gpu

EPS = 1e-5
U = emu.U
# (kernel, C, PG): PG = pixel groups of a workgroup (vector fp32: 256 / (C/4); generic: four waves stride the pixels; bf16: 256 / (C/8))
WIDTHS = (("vec", 64, 16), ("vec", 128, 8), ("vec", 256, 4), ("generic", 4, 4), ("generic", 96, 4), ("generic", 320, 4), ("generic", 512, 4),
          ("bf16", 64, 32), ("bf16", 128, 16), ("bf16", 256, 8))
STATS_CASES = [(g, k, C, PG) for g in emu.GEOMETRIES for (k, C, PG) in WIDTHS if not (k == "bf16" and g[2] > 64)]


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _stats_call(xd, B, HW, C, nsplit, bf16):
    """The entry point itself with NaN-filled workspace and outputs -> (hipError_t, mean, rstd)."""
    mean, rstd, ws = _nan(B, C), _nan(B, C), _nan(max(1, B * C * max(nsplit, 1) * 3))
    fn = _lib.lib().lwg_instnorm_stats_nhwc_bf16 if bf16 else _lib.lib().lwg_instnorm_stats_nhwc_f32
    err = fn(xd.data_ptr(), B, HW, C, EPS, mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(), nsplit, ops._stream())
    torch.cuda.synchronize()
    return err, mean, rstd


@functools.lru_cache(maxsize=2)
def _data(B, HW, C, nsplit, PG, bf16):
    """The families of instnorm_emu.make_data; for bf16 rounded to bf16 first, and the reference takes the rounded values."""
    x, fam, _ = emu.make_data(B, HW, C, nsplit, PG, seed=11)
    xt = torch.from_numpy(x)
    if bf16:
        xt = xt.to(torch.bfloat16)
        x = xt.float().numpy()
    return x, xt, fam, emu.reference(x, nsplit, PG, EPS)


@pytest.mark.parametrize("geom,kind,C,PG", STATS_CASES, ids=lambda v: "B%d_HW%d_ns%d" % v if isinstance(v, tuple) else str(v))
def test_stats_within_bounds_and_batch_invariant(geom, kind, C, PG):
    B, HW, nsplit = geom
    bf16 = kind == "bf16"
    x, xt, fam, ref = _data(B, HW, C, nsplit, PG, bf16)
    xd = xt.to(DEV)
    err, mean, rstd = _stats_call(xd, B, HW, C, nsplit, bf16)
    assert err == 0
    m, r = mean.cpu().numpy(), rstd.cpu().numpy()
    for fname, (a, b) in emu.worst_by_family(m, r, ref, fam).items():
        print(f"RATIO {kind} C{C} B{B}_HW{HW}_ns{nsplit} {fname} {a:.4f} {b:.4f}")
    emu.assert_bounds(m, r, ref, EPS, fam, f"{kind} C={C} {geom}")
    for b in range(B if B > 1 else 0):                          # the (b * nsplit + split) * C record index: an image never sees its batch
        err, m1, r1 = _stats_call(xd[b:b + 1].contiguous(), 1, HW, C, nsplit, bf16)
        assert err == 0 and torch.equal(m1[0], mean[b]) and torch.equal(r1[0], rstd[b]), f"image {b} of {B} depends on its batch"


def test_refusals_leave_the_outputs_untouched():
    x32, x16 = torch.ones(1, 64, 96, device=DEV), torch.ones(1, 64, 96, device=DEV, dtype=torch.bfloat16)
    for what, (xd, C, nsplit, bf16) in {"bf16 nsplit 65": (x16, 64, 65, True), "bf16 C 96": (x16, 96, 4, True), "bf16 nsplit 0": (x16, 64, 0, True),
                                        "fp32 nsplit 0": (x32, 96, 0, False), "fp32 nsplit 0 C 64": (x32, 64, 0, False)}.items():
        err, mean, rstd = _stats_call(xd, 1, 64 * 96 // C, C, nsplit, bf16)
        assert err != 0, f"{what}: accepted"
        assert torch.isnan(mean).all() and torch.isnan(rstd).all(), f"{what}: refused, but wrote"


def test_outlier_shift_limitation():
    """x[0] = 1e4 in N(0,1), HW 4096: with ONE split every d^2 is ~1e8 and rstd loses ~1e-3 relative (inside the bound: its kappa term);
    with the product's 64 splits only the first is hit.  The figures are in DESIGN.md 3.2."""
    out = {}
    for nsplit in (1, 64):
        x, xt, fam, ref = _data(1, 4096, 64, nsplit, 16, False)
        err, mean, rstd = _stats_call(xt.to(DEV), 1, 4096, 64, nsplit, False)
        assert err == 0
        m, r = mean.cpu().numpy(), rstd.cpu().numpy()
        emu.assert_bounds(m, r, ref, EPS, fam, f"outlier shift nsplit {nsplit}")
        sel = fam == emu.FAMILIES.index("outlier_shift")
        out[nsplit] = float(np.abs(r.astype(np.float64) / ref["rho"] - 1)[sel].max())
    print("OUTLIER", out)
    assert out[64] < out[1], out


# ---------------------------------------------------------------------------------------------------------------- apply
def _apply_call(xd, mean, rstd, res, B, HW, C, act):
    y = _nan(B, HW, C)
    err = _lib.lib().lwg_instnorm_apply_nhwc_f32(xd.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None if res is None else res.data_ptr(),
                                                 y.data_ptr(), B, HW, C, act, ops._stream())
    torch.cuda.synchronize()
    assert err == 0
    return y


def _apply_check(y, x, mean, rstd, res, act, what):
    """y (n, HW, C) of the kernel against float64 with the SAME fp32 mean / rstd: the subtraction, the product and the residual's addition
    round once each, so ACT_NONE / ACT_RELU stay within 4 u (|t| + |res|), t = (x - mean) rstd; tanh / sigmoid keep the suite's 2e-5."""
    t = (x.double() - mean.double()[:, None, :]) * rstd.double()[:, None, :]
    r = torch.zeros_like(t) if res is None else res.double()
    if act in (ops.ACT_NONE, ops.ACT_RELU):
        want = (t.clamp_min(0) if act == ops.ACT_RELU else t) + r
        over = (y.double() - want).abs() - 4 * U * (t.abs() + r.abs())
        assert torch.isfinite(y).all() and over.max().item() <= 0, f"{what}: {int((over > 0).sum())} elements over 4u(|t|+|res|), worst by {over.max().item():.3e}"
    else:
        _cmp(y, ((torch.tanh(t) if act == ops.ACT_TANH else torch.sigmoid(t)) + r).float(), 2e-5, what)


@pytest.mark.parametrize("C", (4, 96, 256))
@pytest.mark.parametrize("B,HW,nsplit", ((2, 35, 8), (3, 1000, 3)))
def test_apply_every_activation_with_and_without_residual(B, HW, nsplit, C):
    x, xt, fam, _ = _data(B, HW, C, nsplit, 4, False)
    xd = xt.to(DEV)
    err, mean, rstd = _stats_call(xd, B, HW, C, nsplit, False)
    assert err == 0
    res = torch.from_numpy(np.random.default_rng([12, B, HW, C]).standard_normal((B, HW, C), dtype=np.float32))
    for with_res in (False, True):
        for act in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_TANH, ops.ACT_SIGMOID):
            y = _apply_call(xd, mean, rstd, res.to(DEV) if with_res else None, B, HW, C, act)
            _apply_check(y.cpu(), xt, mean.cpu(), rstd.cpu(), res if with_res else None, act, f"apply C={C} HW={HW} act={act} res={with_res}")


def test_apply_grid_stride_loop_wraps():
    """(5, 96x96, 96) is 1,105,920 float4 against the launch's 4096 x 256 = 1,048,576 threads: the last 57,344 come from a second trip of
    the grid-stride loop.  First and last image compared in full, and nothing in between left unwritten."""
    B, HW, C, nsplit = 5, 96 * 96, 96, 64
    x, xt, fam, _ = _data(B, HW, C, nsplit, 4, False)
    xd = xt.to(DEV)
    err, mean, rstd = _stats_call(xd, B, HW, C, nsplit, False)
    assert err == 0
    res = torch.from_numpy(np.random.default_rng([13]).standard_normal((B, HW, C), dtype=np.float32))
    y = _apply_call(xd, mean, rstd, res.to(DEV), B, HW, C, ops.ACT_RELU)
    assert not torch.isnan(y).any()
    for b in (0, B - 1):
        s = slice(b, b + 1)
        _apply_check(y[s].cpu(), xt[s], mean[s].cpu(), rstd[s].cpu(), res[s], ops.ACT_RELU, f"apply wrap image {b}")
