"""tests/attn_flows.py checked on the CPU: the flow families do what their names say, the torch references agree with an independent
numpy loop, each deliberately wrong variant of the block fails the GPU test's bound by more than 10x on at least one family, and the
fp32 CPU evaluation of every case of tests/test_gpu_lwb_attention_flows.py stays inside the bound that test uses (so a GPU failure
is the kernel's, not the reference's)."""
import functools

import numpy as np
import pytest
import torch

from tests import attn_flows as af
from tests import emu_ops

C_F32 = (32, 64, 128, 256)


# ------------------------------------------------------------------------------------------------ family properties
@pytest.mark.parametrize("family", af.FAMILIES)
def test_fields_are_finite_fp32_and_reproducible(family):
    for (B, ns, S, h, w) in af.GEOMETRIES:
        for (H, W, size) in ((S, S, (h, w)), (h, w, None)):
            T = af.flows(family, B, ns, H, W, seed=3, size=size)
            assert T.dtype == torch.float32 and tuple(T.shape) == (B, ns, H, W, 2) and torch.isfinite(T).all()
            assert torch.isfinite((T + 1) * float(max(h, w))).all(), "(g + 1) * size overflows"
            assert torch.equal(T, af.flows(family, B, ns, H, W, seed=3, size=size))
            assert family == "collapse" or family == "identity" or not torch.equal(T, af.flows(family, B, ns, H, W, seed=4, size=size))


@pytest.mark.parametrize("size", [8, 16, 64])
def test_lattice_and_half_are_exact_in_fp32(size):
    """Power-of-two sizes: the fp32 flow evaluated in FP32 with the kernel's expression gives the integer / half-integer exactly."""
    for family, frac, lo, hi in (("lattice", 0.0, -2, size + 1), ("half", 0.5, -2, size)):
        T = af.flows(family, 2, 3, size, size, seed=1)
        pix = ((T + 1.0) * float(size) - 1.0) * 0.5                  # fp32 arithmetic
        assert pix.dtype == torch.float32
        fl = torch.floor(pix)
        assert torch.equal(pix - fl, torch.full_like(pix, frac))
        assert fl.min().item() == lo and fl.max().item() == hi, (fl.min().item(), fl.max().item())
    T = af.flows("lattice", 2, 3, size, size, seed=1)
    ix, iy = af.pixel_coords(T, size, size)
    for v in (-2, -1, 0, size - 1, size, size + 1):                  # first / last in-image tap and fully outside, on both axes
        assert (ix == v).any() and (iy == v).any(), v


def test_border_has_every_in_out_pattern():
    """Per axis the two taps (floor, floor + 1) are in / out of the image in all four ways: (out, out), (out, in), (in, in), (in, out)."""
    for (h, w) in ((16, 16), (9, 13), (13, 13)):
        T = af.flows("border", 2, 3, h, w, seed=1)
        for coord, size in zip(af.pixel_coords(T, h, w), (w, h)):
            f0 = coord.floor()
            in0, in1 = (f0 >= 0) & (f0 < size), (f0 + 1 >= 0) & (f0 + 1 < size)
            seen = {(bool(a), bool(b)) for a, b in zip(in0.flatten().tolist(), in1.flatten().tolist())}
            assert seen == {(False, False), (False, True), (True, True), (True, False)}, seen
            assert ((coord - coord.round()).abs() <= 0.02 + 1e-6).all()


@pytest.mark.parametrize("hw", [(8, 8), (13, 13), (9, 13), (7, 5), (1, 7), (64, 64)])
def test_one_per_tile_has_one_foreground_pixel_per_tile_source_and_frame(hw):
    h, w = hw
    T = af.flows("one_per_tile", 3, 2, h, w, seed=5)
    fg = (T != -2.0).any(dim=-1)
    assert ((T == -2.0).all(dim=-1) | ((T >= -1) & (T <= 1)).all(dim=-1)).all()
    for ty in range(0, h, 8):
        for tx in range(0, w, 8):
            assert (fg[:, :, ty:ty + 8, tx:tx + 8].sum(dim=(2, 3)) == 1).all(), (ty, tx)
    assert len({int(i) for i in fg.reshape(6, -1).float().argmax(dim=1)}) > 1 or h * w < 8


def test_checker_collapse_identity_wild():
    T = af.flows("checker", 2, 3, 13, 13, seed=1)
    bg = (T == -2.0).all(dim=-1)
    y, x, s = torch.meshgrid(torch.arange(13), torch.arange(13), torch.arange(3), indexing="ij")
    assert torch.equal(bg[0], ((y + x + s) % 2 == 0).permute(2, 0, 1)) and torch.equal(bg[0], bg[1])
    T = af.flows("collapse", 2, 3, 9, 13, seed=1)
    assert (T == T[0, 0, 0, 0]).all()
    ix, iy = af.pixel_coords(T, 9, 13)
    assert 0 < ix[0, 0, 0, 0] < 12 and 0 < iy[0, 0, 0, 0] < 8 and abs(ix[0, 0, 0, 0].item() - 6.2) < 1e-5
    for (H, W, size) in ((9, 13, None), (40, 40, (9, 13))):         # also through the resize: linear fields survive it
        T = af.flows("identity", 1, 2, H, W, seed=1, size=size)
        ix, iy = af.pixel_coords(T if size is None else af.ref_flow_resize(T, 9, 13), 9, 13)
        assert (ix - torch.arange(13.0, dtype=torch.float64)).abs().max() < 1e-5
        assert (iy - torch.arange(9.0, dtype=torch.float64)[:, None]).abs().max() < 1e-5
    T = af.flows("wild", 2, 3, 16, 16, seed=1)
    odd = (T.abs() > 1).any(dim=-1).float().mean().item()
    assert 0.3 < odd < 0.7 and T.abs().max().item() == np.float32(1e30)
    assert set(T[T.abs() > 1].tolist()) == {float(np.float32(v)) for v in af.WILD_VALUES}


def test_wild_only_without_resize():
    table = af.forward_table()
    assert all(not af.uses_resize(g) for f, g in table if f == "wild") and any(f == "wild" for f, g in table)
    assert {g for f, g in table} == set(af.GEOMETRIES) and {f for f, g in table} == set(af.FAMILIES)


# ------------------------------------------------------------------------------------------------ independent reference
@pytest.mark.parametrize("family", af.FAMILIES)
def test_numpy_loop_agrees_with_emulation(family):
    """One small case per family, with and without the resize: the numpy loop against emu_ops.lwb_attention in fp64, 1e-12."""
    for geom in ((2, 2, 7, 7, 7), (2, 3, 11, 4, 6)):
        if not af.family_allowed(family, geom):
            continue
        B, ns, S, h, w = geom
        T = af.flows(family, B, ns, S, S, seed=2, size=(h, w))
        ops_ = af.qkv_operands(af.rs(9, S), B, ns, h, w, 8, True)
        ref = af.ref_attention(*ops_, T, True)
        got = af.attention_loops(*[t.numpy() for t in ops_], T.numpy(), True)
        assert np.abs(got - ref.numpy()).max() <= 1e-12 * max(1.0, ref.abs().max().item()), (family, geom)
        assert torch.equal(af.variant_attention(*ops_, T, True, None), ref)


# ------------------------------------------------------------------------------------------------ discriminating power
@pytest.mark.parametrize("variant", af.VARIANTS)
def test_wrong_variant_fails_the_gpu_bound_by_10x(variant):
    """For each deliberate mistake at least one family's fp64 result is more than 10x the GPU test's bound away from the reference."""
    worst = {}
    geom = (2, 3, 40, 9, 13) if variant == "resize_no_align_corners" else (3, 3, 13, 13, 13)
    for family in af.FAMILIES:
        if not af.family_allowed(family, geom):
            continue
        ops_, T, ref, err32 = af.forward_case(family, geom, 32, True, False)
        emax, emean, ref_max = af.fwd_errors(af.variant_attention(*ops_, T, True, variant), ref)
        bmax, bmean = af.fwd_bound("f32", ref_max, err32)
        worst[family] = max(emax / bmax, emean / bmean)
    print("variant", variant, {k: f"{v:.3g}" for k, v in worst.items()})
    assert max(worst.values()) > 10.0, worst
    if variant == "padding_border":
        assert worst["border"] > 10.0 and worst["identity"] < 1.0       # only flows that leave the image tell the two paddings apart


def test_wrong_resize_fails_the_flow_resize_bound_by_10x():
    B, ns, S, h, w = 2, 3, 40, 9, 13
    T = af.flows("border", B, ns, S, S, seed=0, size=(h, w))
    wrong = torch.nn.functional.interpolate(T.double().reshape(B * ns, S, S, 2).permute(0, 3, 1, 2), size=(h, w), mode="bilinear",
                                            align_corners=False).permute(0, 2, 3, 1).reshape(B, ns, h, w, 2)
    err = (wrong - af.ref_flow_resize(T, h, w)).abs().max().item()
    assert err > 10 * af.RESIZE_TOL * S * max(1.0, T.abs().max().item()), err


# ------------------------------------------------------------------------------------------------ the reference alone stays inside the bound
@functools.lru_cache(maxsize=None)
def _forward_figures(family, geom):
    rows = []
    for dt, Cs in (("f32", C_F32), ("bf16", C_F32[1:])):
        for C in Cs:
            for batched in (False, True):
                for peaked in (False, True):
                    ops_, T, ref, err32 = af.forward_case(family, geom, C, batched, peaked, dt)
                    got = af.ref_attention(*ops_, T, batched, dtype=torch.float32)
                    if dt == "bf16":
                        got = got.to(torch.bfloat16)
                    rows.append(((dt, C, batched, peaked), af.fwd_errors(got, ref), err32))
    return rows


@pytest.mark.parametrize("family,geom", af.forward_table(), ids=[f"{f}-{af.geom_id(g)}" for f, g in af.forward_table()])
def test_fp32_forward_reference_stays_inside_the_bound(family, geom):
    """The q / K / V forward of every case the GPU test runs, evaluated with emu_ops in float32 (bf16: on the bf16-rounded operands, the
    result rounded to bf16).  Resized cases: 4 * err32 <= 2e-3 * max(1, ref_max), so the per-case bound cannot grow silently."""
    bad = []
    for key, (emax, emean, ref_max), err32 in _forward_figures(family, geom):
        bmax, bmean = af.fwd_bound(key[0], ref_max, err32)
        if err32 is not None:
            print(f"ERR32 {family} {af.geom_id(geom)} {key[0]} C{key[1]} b{int(key[2])} p{int(key[3])} max {err32[0]:.2e} mean {err32[1]:.2e} ref_max {ref_max:.2f}")
            if not af.ERR32_FACTOR * err32[0] <= af.ERR32_CAP * max(1.0, ref_max):
                bad.append((key, "4 * err32 over its cap", err32, ref_max))
        if not (emax <= bmax and emean <= bmean):
            bad.append((key, emax, emean, bmax, bmean))
    assert not bad, bad


@pytest.mark.parametrize("family,geom", af.forward_table(), ids=[f"{f}-{af.geom_id(g)}" for f, g in af.forward_table()])
def test_fp32_backward_reference_stays_inside_the_bound(family, geom):
    """fp32 CPU autograd of the case the GPU backward test runs (src_batched, B >= 2) against fp64 autograd: <= 5e-4."""
    B, ns, S, h, w = geom
    B = max(B, 2)
    T = af.flows(family, B, ns, S, S, seed=0, size=(h, w))
    for C in (32, 256):
        r = af.rs(1, C, B, ns, h, w)
        ops_ = af.qkv_operands(r, B, ns, h, w, C, True)
        dout = af._n(r, (B, h, w, C))
        ref = af.ref_attention_bwd(*ops_, T, dout, True)
        got = emu_ops.lwb_attention_bwd(*ops_, T, dout, src_batched=True)
        errs = af.bwd_errors(got, ref)
        assert max(errs) <= af.BWD_TOL, (C, errs)
        # the texels the GPU test requires to stay exactly zero: zero in fp64, and zero in fp32 too (a coordinate that fp32 rounds across a
        # pixel edge moves a tap by one pixel at the most - also from just outside the image to its first row)
        far = ~af.touched(T, h, w, B * ns, True)
        for t in (ref[1], ref[2], got[1], got[2]):
            assert (t[far] == 0).all(), C


@pytest.mark.parametrize("family", af.FAMILIES)
def test_fp32_x_form_reference_stays_inside_the_bound(family):
    for (B, ns, S, h, w) in af.GEOMETRIES:
        T = af.flows(family, B, ns, h, w, seed=0)
        for C in (32, 256):
            for peaked in (False, True):
                ops_ = af.x_operands(af.rs(2, C, B, ns, h, w), B, ns, h, w, C, False, peaked)
                ref = af.ref_attention_x(*ops_, T, False)
                emax, emean, ref_max = af.fwd_errors(af.ref_attention_x(*ops_, T, False, dtype=torch.float32), ref)
                bmax, bmean = af.fwd_bound("f32", ref_max)
                assert emax <= bmax and emean <= bmean, (family, h, w, C, peaked, emax, emean)
