"""The output-head kernels one by one on the cases of tests/head_cases.py: lwg_head_compose_f32 (both tile forms), lwg_head_compose_q4_f32 (both),
lwg_head_compose_bf16 (with its frame-slicing recursion), the head phase of lwg_up4_head_compose_bf16, lwg_thin_conv_f32 (ks 5 and 7, both tile
forms), the two layout kernels and lwg_frames_to_u8.  References, bounds and their derivations live in tests/head_cases.py;
tests/test_head_cases_cpu.py shows on the CPU that the exact family is exact, that an fp32 restatement of every form meets every bound with slack and
that the planted indexing faults do not.

The sharp instrument is the exact family (pre-activations exact in any summation order: what is left is the transcendental and the compositing, a few
ulp) at every size on either side of every form's tile seams; on top of it every form is checked for output selection, for frames that cannot see
their NaN neighbours, for writes outside its output planes (C ABI on views inside NaN-filled allocations; the ops.* wrapper must return the same
bits), and on random data for magnitude.  Every test prints its metrics - the worst |error| / bound of each comparison - as one JSON line."""
import functools
import json
import time

import numpy as np
import pytest
import torch

from ipercore_amd import _lib, ops
from ipercore_amd.networks import packing
from tests import head_cases as hc
from tests.gpu_checks import DEV, _spec_dev

pytestmark = pytest.mark.gpu

SENT = 0x7FC0DEAD                                    # a quiet NaN with a payload no computation produces
SENT16 = 0x7FDA                                      # ... the same in bf16
ENTRY = {"f32": "lwg_head_compose_f32", "q4": "lwg_head_compose_q4_f32", "bf16": "lwg_head_compose_bf16"}
SUBSETS = [(p, m, i) for p in (True, False) for m in (True, False) for i in (True, False) if p or m or i]
INVALID = 1                                          # hipErrorInvalidValue


def _report(what, metrics):
    print("head_kernels " + json.dumps({what: metrics}))


def _np(outs):
    return [None if o is None else o.cpu().numpy() for o in outs]


def _same(a, b):
    return all((x is None and y is None) or torch.equal(hc.bits(x), hc.bits(y)) for x, y in zip(a, b))


def _operands(kind, case):
    """(x, packed head weights) on the device in the layout and type form ``kind`` takes - the case's values, rounded to nothing on the exact family."""
    x, w = case["x"], case["w"]
    if kind == "q4":
        B, S, _, C = x.shape
        return x.view(B, S, S, C // 4, 4).permute(0, 3, 1, 2, 4).contiguous().to(DEV), packing.pack_head(w[:3], w[3:]).to(DEV)
    if kind == "bf16":
        return x.to(torch.bfloat16).to(DEV), packing.pack_head_bf16(w[:3], w[3:]).to(DEV)
    return x.to(DEV), packing.pack_head(w[:3], w[3:]).to(DEV)


def _run(kind, xd, wd, bg, sel=(True, True, True)):
    return ops.head_compose(xd, wd, bg, want_pred=sel[0], want_mask=sel[1], want_img=sel[2], q4=kind == "q4")


def _head(kind, case, sel=(True, True, True)):
    xd, wd = _operands(kind, case)
    out = _run(kind, xd, wd, case["bg"].to(DEV), sel)
    torch.cuda.synchronize()
    return out


def _assert_ratios(r, what):
    assert max(r.values()) <= 1.0, "%s: worst |error| / bound %s" % (what, r)


# ------------------------------------------------------------------------------------------------------------------------------ the exact family
@pytest.mark.parametrize("S", hc.SIZES)
@pytest.mark.parametrize("kind", hc.FORMS)
def test_exact_family(kind, S):
    """unsat / sat / cancel at every channel count of the form, B = 1, 2, 3 in turn with a per-frame background, against float64 within the
    transcendental-and-compositing bound."""
    worst = {}
    for C in hc.CHANNELS[kind]:
        for variant in hc.VARIANTS:
            case = hc.exact_case(variant, hc.batch_of(S), S, C)
            r = hc.ratios(_np(_head(kind, case)), hc.reference(case))
            worst[case["name"]] = r
    _report("exact_%s_S%d" % (kind, S), worst)
    for name, r in worst.items():
        _assert_ratios(r, "%s %s" % (kind, name))


@pytest.mark.parametrize("S", hc.SIZES)
def test_thin_conv_exact_family(S):
    """No transcendental: the outputs are float64's bit for bit, the columns behind the N real outputs exactly 0."""
    n = 0
    for ks, N in hc.THIN:
        for C in hc.CHANNELS["thin"]:
            case = hc.exact_case("unsat", hc.batch_of(S), S, C, ks=ks, N=N)
            got = ops.thin_conv(case["x"].to(DEV), packing.pack_thin(case["w"]).to(DEV), ks).cpu()
            want = hc.preact(case["x"].numpy(), case["w"].numpy())
            assert np.array_equal(got[..., :N].double().numpy(), want), "thin conv %s differs from float64" % case["name"]
            assert N == 4 or not got[..., N:].any(), "thin conv %s: a column behind the outputs is not 0" % case["name"]
            n += 1
    _report("thin_exact_S%d" % S, {"cases": n, "worst_error_over_bound": 0.0, "bitwise": True})


@pytest.mark.parametrize("pas", ["tap", "chan"])
@pytest.mark.parametrize("kind", hc.FORMS)
def test_coded_impulse(kind, pas):
    """One impulse per frame at corners, edges and both sides of every tile seam, in channels 0, 3/4, 7/8, 31/32 and C - 1: every output is the
    transcendental of exactly one coded weight."""
    worst = {}
    for S in hc.IMPULSE_S[kind]:
        C = hc.CHANNELS[kind][-1] if S == 65 else hc.CHANNELS[kind][0]
        case = hc.impulse_case(kind, pas, S, C)
        worst[case["name"]] = hc.ratios(_np(_head(kind, case)), hc.reference(case))
    _report("impulse_%s_%s" % (kind, pas), worst)
    for name, r in worst.items():
        _assert_ratios(r, "%s %s" % (kind, name))


@pytest.mark.parametrize("S", hc.LARGE_S)
@pytest.mark.parametrize("kind", ["f32", "q4", "thin"])
def test_large_tile_forms(kind, S):
    """The frame-batch forms (<4>, <2, 4>, thin J = 4) at the smallest batch that reaches them: frames 0, the middle one and the last against float64,
    and every frame bitwise its one-frame launch, which takes the small form."""
    C = hc.CHANNELS[kind][0]
    B = hc.large_form_batch(kind, S)
    assert hc.head_form(kind, B, S)[0] in ("J4", "NX2_RY4") and hc.head_form(kind, 1, S)[0] in ("J2", "NX1_RY2")
    frames = [0, B // 2, B - 1]
    if kind == "thin":
        worst = {}
        for ks, N in ((5, 4), (7, 3)):
            case = hc.exact_case("unsat", B, S, C, ks=ks, N=N)
            xd, wd = case["x"].to(DEV), packing.pack_thin(case["w"]).to(DEV)
            got = ops.thin_conv(xd, wd, ks)
            want = hc.preact(case["x"][frames].numpy(), case["w"].numpy())
            assert np.array_equal(got[frames][..., :N].cpu().double().numpy(), want), "thin conv J = 4, %s" % case["name"]
            assert N == 4 or not got[..., N:].any()
            for f in range(B):
                assert torch.equal(hc.bits(ops.thin_conv(xd[f:f + 1], wd, ks)[0]), hc.bits(got[f])), "thin conv %s: frame %d depends on its batch" % (case["name"], f)
            worst[case["name"]] = 0.0
        _report("large_form_thin_S%d" % S, {"B": B, "worst_error_over_bound": worst, "frames_bitwise_one_frame_launch": True})
        return
    case = hc.exact_case("unsat", B, S, C)
    xd, wd = _operands(kind, case)
    bg = case["bg"].to(DEV)
    out = _run(kind, xd, wd, bg)
    torch.cuda.synchronize()
    sub = {"x": case["x"][frames], "w": case["w"], "bg": case["bg"][frames]}
    r = hc.ratios(_np([o[frames] for o in out]), hc.reference(sub))
    _report("large_form_%s_S%d" % (kind, S), {"B": B, "worst_error_over_bound": r})
    _assert_ratios(r, "%s large form S = %d" % (kind, S))
    for f in range(B):
        one = _run(kind, xd[f:f + 1], wd, bg[f:f + 1])
        assert _same(one, [o[f:f + 1] for o in out]), "%s S = %d: frame %d of %d differs from its one-frame launch" % (kind, S, f, B)


# ------------------------------------------------------------------------------------------------------------------------------ the fused up-sampling head
@functools.lru_cache(maxsize=None)
def _up4_weights(name, case_fn, *args):
    case = case_fn(*args)
    specs = [_spec_dev(s) for s in packing.pack_conv_transpose(case["wup"], case["bias"])]
    return case, specs, packing.pack_head_bf16(case["w"][:3], case["w"][3:]).to(DEV)


def _up4(case, specs, head16, sel=(True, True, True), bg="case", x=None):
    xd = case["x"].to(torch.bfloat16).to(DEV) if x is None else x
    assert ops.up4_head_eligible(xd, specs, ops.ACT_RELU)
    bgd = case["bg"].to(DEV) if isinstance(bg, str) else bg
    out = ops.up4_head_compose_bf16(xd, specs, head16, bgd, want_pred=sel[0], want_mask=sel[1], want_img=sel[2])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("H,W", hc.UP4_HW)
def test_up4_head_exact_family(H, W):
    """(1, 1), (1, 7), the exact tile (6, 14), one over (7, 15) and the two non-square shapes: the three variants on an exact intermediate, then the coded
    impulse in the intermediate (both passes)."""
    worst = {}
    todo = [(hc.up4_case, (v, 1 + (H + W) % 3, H, W)) for v in hc.VARIANTS] + [(hc.up4_impulse_case, (p, H, W)) for p in ("tap", "chan")]
    for fn, args in todo:
        case, specs, head16 = _up4_weights(fn.__name__, fn, *args)
        worst[case["name"]] = hc.ratios(_np(_up4(case, specs, head16)), hc.reference(case))
    _report("up4_exact_%dx%d" % (H, W), worst)
    for name, r in worst.items():
        _assert_ratios(r, name)


def test_up4_head_many_tiles_per_workgroup():
    """5 x 96 x 96: 560 tiles, more than one per CU - persistent workgroups walk several tiles, and prefetch the next one's halo under the head phase."""
    B, H, W = hc.UP4_MANY
    case, specs, head16 = _up4_weights("many", hc.up4_case, "unsat", B, H, W, False)
    r = hc.ratios(_np(_up4(case, specs, head16)), hc.reference(case))
    _report("up4_many_tiles", {"tiles": B * -(-2 * H // 12) * -(-2 * W // 28), "worst_error_over_bound": r})
    _assert_ratios(r, case["name"])


# ------------------------------------------------------------------------------------------------------------------------------ properties of every form
KINDS = ("f32", "q4", "bf16", "up4")


def _property_cases(kind):
    """[(case, run(sel, bg tensor or None, frames or None) -> (pred, mask, img))] at two or three small sizes, B = 3."""
    out = []
    if kind == "up4":
        for H, W in ((7, 15), (5, 23)):
            case, specs, head16 = _up4_weights("prop", hc.up4_case, "unsat", 3, H, W)
            xd = case["x"].to(torch.bfloat16).to(DEV)

            def run(sel, bg, frames=None, xd=xd, case=case, specs=specs, head16=head16, x=None):
                xs = xd if x is None else x
                return _up4(case, specs, head16, sel, bg, xs if frames is None else xs[frames].contiguous())
            out.append((case, run))
        return out
    for S in hc.PROPERTY_S:
        case = hc.exact_case("unsat", 3, S, hc.CHANNELS[kind][0])
        xd, wd = _operands(kind, case)

        def run(sel, bg, frames=None, xd=xd, wd=wd, x=None):
            xs = xd if x is None else x
            o = _run(kind, xs if frames is None else xs[frames].contiguous(), wd, bg, sel)
            torch.cuda.synchronize()
            return o
        out.append((case, run))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_output_selection(kind):
    """Each of the seven non-empty subsets of (pred, mask, img) gives the bits of the full call, with a shared (stride 0) and a per-frame background;
    the outputs not asked for are not returned; pred without a background is refused before any launch."""
    n = 0
    for case, run in _property_cases(kind):
        for bg in (case["bg"].to(DEV), case["bg"][1:2].contiguous().to(DEV)):
            full = run((True, True, True), bg)
            assert all(bool(torch.isfinite(o).all()) for o in full)
            for sel in SUBSETS:
                got = run(sel, bg if sel[0] else None)
                assert all((g is None) == (not s) for g, s in zip(got, sel)), (case["name"], sel)
                assert _same(got, [o if s else None for o, s in zip(full, sel)]), "%s %s: selecting %s changes the values" % (kind, case["name"], sel)
                n += 1
    x = torch.zeros(1, 8, 8, 64, device=DEV)
    p = torch.zeros(1, 3, 8, 8, device=DEV)
    for k, xx in (("f32", x), ("q4", x), ("bf16", x.to(torch.bfloat16))):
        assert getattr(_lib.lib(), ENTRY[k])(xx.data_ptr(), x.data_ptr(), None, 0, 1, 8, 64, p.data_ptr(), None, None, ops._stream()) == INVALID, k
        assert getattr(_lib.lib(), ENTRY[k])(xx.data_ptr(), x.data_ptr(), None, 0, 1, 8, 64, None, None, None, ops._stream()) == INVALID, k
    _report("output_selection_" + kind, {"subsets_bitwise_equal_to_full_call": n})


@pytest.mark.parametrize("kind", KINDS + ("thin",))
def test_poisoned_neighbours(kind):
    """B = 3 with frames 0 and 2 all NaN, in x and in their per-frame backgrounds: frame 1 is finite and bitwise its one-frame launch - a halo that
    reached into a neighbouring frame (frames are adjacent in memory: a missed gy >= 0 reads valid memory) would show."""
    n = 0
    if kind == "thin":
        for S in hc.PROPERTY_S:
            for ks, N in ((5, 4), (7, 3)):
                case = hc.exact_case("unsat", 3, S, 8, ks=ks, N=N)
                xd, wd = case["x"].to(DEV), packing.pack_thin(case["w"]).to(DEV)
                xd[0], xd[2] = float("nan"), float("nan")
                got, one = ops.thin_conv(xd, wd, ks), ops.thin_conv(xd[1:2].contiguous(), wd, ks)
                assert bool(torch.isfinite(got[1]).all()) and torch.equal(hc.bits(got[1]), hc.bits(one[0])), case["name"]
                assert np.array_equal(got[1, ..., :N].cpu().double().numpy(), hc.preact(case["x"][1:2].numpy(), case["w"].numpy())[0]), case["name"]
                n += 1
    else:
        for case, run in _property_cases(kind):
            xd = (case["x"].to(torch.bfloat16) if kind in ("bf16", "up4") else case["x"]).clone()
            xd[0], xd[2] = float("nan"), float("nan")
            xd = _operands(kind, {"x": xd, "w": case["w"]})[0] if kind != "up4" else xd.to(DEV)
            bg = case["bg"].clone().to(DEV)
            bg[0], bg[2] = float("nan"), float("nan")
            got = run((True, True, True), bg, x=xd)
            one = run((True, True, True), bg[1:2].contiguous(), frames=slice(1, 2), x=xd)
            assert all(bool(torch.isfinite(g[1]).all()) for g in got), "%s %s: frame 1 picked up a neighbour's NaN" % (kind, case["name"])
            assert _same([g[1:2] for g in got], one), "%s %s: frame 1 differs from its one-frame launch" % (kind, case["name"])
            n += 1
    _report("poisoned_neighbours_" + kind, {"cases": n, "frame_1_finite_and_bitwise_one_frame_launch": True})


def _guard_len(row):
    return -(-(2 * row + 64) // 64) * 64                  # at least two image rows, a multiple of 64 elements (16-byte alignment and more)


def _guarded(t, row, fill=False):
    """t's values (or, fill=True, the sentinel) as a contiguous view in the middle of a sentinel-NaN allocation -> (view, check())."""
    g, n = _guard_len(row), t.numel()
    wide = {torch.float32: (torch.int32, SENT), torch.bfloat16: (torch.int16, SENT16)}[t.dtype]
    raw = torch.full((g + n + g,), wide[1], dtype=wide[0], device=DEV)
    buf = raw.view(t.dtype)
    view = buf[g:g + n].view(t.shape)
    if not fill:
        view.copy_(t)

    def check(what):
        assert bool((raw[:g] == wide[1]).all()) and bool((raw[g + n:] == wide[1]).all()), what + ": a guard band was written"
        assert not bool(torch.isnan(view.float()).any()), what + ": an element inside was not written"
    assert view.data_ptr() % 16 == 0
    return view, check


@pytest.mark.parametrize("kind", KINDS + ("thin",))
def test_guard_bands(kind):
    """Inputs and outputs are views in the middle of NaN-filled allocations (guards of at least two image rows on each side): after the launch through
    the C ABI the guards hold their bits, the outputs hold no NaN - so nothing read a guard, nothing was written outside the planes, nothing inside was
    left unwritten - and the ops.* wrapper returns the same bits."""
    lib, n = _lib.lib(), 0
    if kind == "thin":
        for S in hc.PROPERTY_S:
            for ks, N in ((5, 4), (7, 3)):
                case = hc.exact_case("unsat", 3, S, 8, ks=ks, N=N)
                x, cx = _guarded(case["x"], S * 8)
                w, cw = _guarded(packing.pack_thin(case["w"]), 32)
                y, cy = _guarded(torch.empty(3, S, S, 4), S * 4, fill=True)
                assert lib.lwg_thin_conv_f32(x.data_ptr(), w.data_ptr(), 3, S, 8, ks, y.data_ptr(), ops._stream()) == 0
                torch.cuda.synchronize()
                for c, what in ((cx, "x"), (cw, "w"), (cy, "y")):
                    c("thin conv %s %s" % (case["name"], what))
                assert torch.equal(hc.bits(ops.thin_conv(x, w, ks)), hc.bits(y)), case["name"]
                n += 1
        _report("guard_bands_thin", {"cases": n})
        return
    for case, run in _property_cases(kind):
        B, H2, W2 = case["bg"].shape[0], case["bg"].shape[2], case["bg"].shape[3]
        if kind == "up4":
            _, specs, head16 = _up4_weights("prop", hc.up4_case, "unsat", 3, case["x"].shape[1], case["x"].shape[2])
            x, cx = _guarded(case["x"].to(torch.bfloat16), case["x"].shape[2] * 128)
        else:
            xd, wd = _operands(kind, case)
            x, cx = _guarded(xd, W2 * 4 if kind == "q4" else W2 * xd.shape[-1])
            w, cw = _guarded(wd, 64)
        for shared in (False, True):
            bg, cb = _guarded(case["bg"][:1] if shared else case["bg"], W2)
            outs = [_guarded(torch.empty(B, c, H2, W2), W2, fill=True) for c in (3, 1, 3)]
            ptrs = [o.data_ptr() for o, _ in outs]
            bstride = 0 if shared else 3 * H2 * W2
            if kind == "up4":
                H, W = case["x"].shape[1], case["x"].shape[2]
                a = ops.conv_args(x, specs[0], torch.empty(0, H2, W2, 64, device=DEV, dtype=torch.bfloat16), act=ops.ACT_RELU, out_hw=(H, W))
                a.w = ops._ptr(ops._w16up(specs), torch.bfloat16)
                e = lib.lwg_up4_head_compose_bf16(a, head16.data_ptr(), bg.data_ptr(), bstride, *ptrs, ops._stream())
                torch.cuda.synchronize()
                want = _up4(case, specs, head16, bg=bg, x=x)
            else:
                e = getattr(lib, ENTRY[kind])(x.data_ptr(), w.data_ptr(), bg.data_ptr(), bstride, B, H2, case["x"].shape[3], *ptrs, ops._stream())
                torch.cuda.synchronize()
                want = run((True, True, True), bg, x=x)
                cw("%s %s weights" % (kind, case["name"]))
            assert e == 0, (kind, case["name"], e)
            cx("%s %s x" % (kind, case["name"]))
            cb("%s %s bg" % (kind, case["name"]))
            for (o, c), what in zip(outs, ("pred", "mask", "img")):
                c("%s %s %s" % (kind, case["name"], what))
            assert _same([o for o, _ in outs], want), "%s %s: the wrapper and the C ABI differ" % (kind, case["name"])
            if not shared:
                r = hc.ratios(_np([o for o, _ in outs]), hc.reference(case))
                _assert_ratios(r, "%s %s inside guards" % (kind, case["name"]))
            n += 1
    _report("guard_bands_" + kind, {"cases": n, "guards_intact": True})


@pytest.mark.parametrize("scale", [0.03, 0.3])
@pytest.mark.parametrize("kind", KINDS)
def test_random_family(kind, scale):
    """x ~ N(0, 1), weights at 0.03 and 0.3, C = 64: magnitude and conditioning.  float64 from the same (bf16-rounded where the form takes bf16)
    operands; gamma(25 C + 8) sum |x||w| through the Lipschitz constants on top of the exact-family bound (the fused form: 2e-2, see the cases module)."""
    if kind == "up4":
        case, specs, head16 = _up4_weights("rand", hc.up4_random_case, scale, 2, 23, 23)
        r = hc.ratios(_np(_up4(case, specs, head16)), hc.up4_random_reference(case))
    else:
        case = hc.random_case(scale, 2, 33, 64, kind == "bf16")
        r = hc.ratios(_np(_head(kind, case)), hc.reference(case, e_s=True))
    _report("random_%s_%g" % (kind, scale), {"worst_error_over_bound": r})
    _assert_ratios(r, "%s %s" % (kind, case["name"]))


# ------------------------------------------------------------------------------------------------------------------------------ bf16 head slicing
def test_bf16_head_frame_slicing():
    """256 x 256 frames (8 MiB of bf16 each) in batches one frame under and exactly at the 32-bit buffer range (0xC0000000 bytes): B = n - 1 is one
    launch, B = n runs in slices and its last slice is one frame.  The recursion re-bases x, bg, pred, mask and img: with a per-frame and with a shared
    background every frame next to the slice boundary, the first and the last are bitwise their one-frame launches."""
    t0 = time.time()
    S = 256
    per = S * S * 128
    n = 0xC0000000 // per
    assert n * per == 0xC0000000 and n == 384
    g = torch.Generator(device=DEV)
    g.manual_seed(20261021)
    x = torch.empty(n, S, S, 64, device=DEV, dtype=torch.bfloat16)
    for f in range(0, n, 32):
        x[f:f + 32] = torch.randn(32, S, S, 64, generator=g, device=DEV)
    bgs = torch.rand(n, 3, S, S, generator=g, device=DEV) - 0.5
    w = torch.randn(4, 64, 5, 5, generator=g, device=DEV).cpu() * 0.05
    wd = packing.pack_head_bf16(w[:3], w[3:]).to(DEV)
    checked = 0
    for B in (n - 1, n):
        first_slice = (0xC0000000 - 1) // per if B * per >= 0xC0000000 else B
        assert first_slice == (B if B < n else n - 1)
        frames = sorted({0, B // 2, first_slice - 2, first_slice - 1, min(first_slice, B - 1), B - 1})
        for bg in (bgs[:B], bgs[5:6]):
            out = ops.head_compose(x[:B], wd, bg, want_pred=True, want_mask=True, want_img=True)
            for f in frames:
                one = ops.head_compose(x[f:f + 1], wd, bg if bg.shape[0] == 1 else bg[f:f + 1], want_pred=True, want_mask=True, want_img=True)
                assert _same(one, [o[f:f + 1] for o in out]), "bf16 head: frame %d of %d differs from its one-frame launch" % (f, B)
                checked += 1
            assert bool(torch.isfinite(out[0][-1]).all())
            del out
    torch.cuda.synchronize()
    del x, bgs
    torch.cuda.empty_cache()
    _report("bf16_head_slicing", {"frames_per_range": n, "frames_checked_bitwise": checked, "seconds": round(time.time() - t0, 2)})


# ------------------------------------------------------------------------------------------------------------------------------ layout kernels
@pytest.mark.parametrize("B", hc.LAYOUT_B)
def test_layout_kernels(B):
    """Every element names its position (arange); the destination is a NaN-filled view between guards: padding channels exactly 0, nothing unwritten,
    nothing outside; and back, taking the first C of Cs channels.  The wrappers return the same bits."""
    lib, n = _lib.lib(), 0
    for P in hc.LAYOUT_P:
        for C in hc.LAYOUT_C:
            src = hc.layout_src(B, C, P)
            for Cp in hc.layout_pads(C):
                want = hc.nchw_to_nhwc_ref(src, Cp)
                s, cs = _guarded(src, P)
                d, cd = _guarded(torch.empty(B, P, Cp), Cp, fill=True)
                assert lib.lwg_nchw_to_nhwc_f32(s.data_ptr(), d.data_ptr(), B, C, Cp, P, ops._stream()) == 0
                torch.cuda.synchronize()
                cs("nchw_to_nhwc src"), cd("nchw_to_nhwc B%d C%d Cp%d P%d" % (B, C, Cp, P))
                assert torch.equal(hc.bits(d.cpu()), hc.bits(want)), "nchw_to_nhwc B%d C%d Cp%d P%d" % (B, C, Cp, P)
                assert torch.equal(hc.bits(ops.nchw_to_nhwc(s.view(B, C, 1, P), c_pad=Cp).view(B, P, Cp)), hc.bits(d))
                back, cb = _guarded(torch.empty(B, C, P), P, fill=True)                 # channels C < Cs whenever Cp > C
                assert lib.lwg_nhwc_to_nchw_f32(d.data_ptr(), back.data_ptr(), B, C, Cp, P, ops._stream()) == 0
                torch.cuda.synchronize()
                cd("nhwc_to_nchw src"), cb("nhwc_to_nchw B%d C%d Cs%d P%d" % (B, C, Cp, P))
                assert torch.equal(hc.bits(back.cpu()), hc.bits(src)), "nhwc_to_nchw B%d C%d Cs%d P%d" % (B, C, Cp, P)
                assert torch.equal(hc.bits(ops.nhwc_to_nchw(d.view(B, 1, P, Cp), channels=C).view(B, C, P)), hc.bits(back))
                n += 1
    _report("layout_B%d" % B, {"shapes": n, "bitwise": True})


# ------------------------------------------------------------------------------------------------------------------------------ frames_to_u8
@pytest.mark.parametrize("bgr", [False, True])
def test_frames_to_u8_thresholds(bgr):
    """On the documented domain [-1, 1]: for every k in 1 .. 255 the fp32 neighbours of the value where the output steps to k, +-1, +-0 and the smallest
    normals, against numpy's fp32 sequence - exact by contract."""
    fr = hc.u8_threshold_frames()
    S = fr.shape[-1]
    want = torch.tensor(hc.u8_ref(fr.numpy())).permute(0, 2, 3, 1)
    want = want.flip(-1) if bgr else want
    out = torch.full((S * 3 + 64 + S * S * 3 + S * 3 + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    g = S * 3 + 64
    g -= g % 16
    frd = fr.to(DEV)
    assert _lib.lib().lwg_frames_to_u8(frd.data_ptr(), 1, S, 1 if bgr else 0, out[g:].data_ptr(), ops._stream()) == 0
    torch.cuda.synchronize()
    got = out[g:g + S * S * 3].view(1, S, S, 3).cpu()
    bad = int((got != want).sum())
    _report("frames_to_u8_thresholds_%s" % ("bgr" if bgr else "rgb"), {"values": int(hc.u8_threshold_values().size), "wrong_bytes": bad})
    assert bad == 0, "frames_to_u8: %d bytes differ from numpy's fp32 sequence" % bad
    assert bool((out[:g] == 0xA5).all()) and bool((out[g + S * S * 3:] == 0xA5).all()), "frames_to_u8 wrote outside its output"
    assert torch.equal(ops.frames_to_u8(frd, bgr=bgr).cpu(), want)


def test_frames_to_u8_grid_stride():
    """B S^2 = 9 * 512^2 > 8192 * 256 pixels: the grid-stride loop runs a second pass.  Every output byte names its position."""
    x, k = hc.u8_position_coded(9, 512)
    assert x.shape[0] * 512 * 512 > 8192 * 256
    for bgr in (False, True):
        got = ops.frames_to_u8(x.to(DEV), bgr=bgr).cpu()
        want = k.permute(0, 2, 3, 1)
        assert torch.equal(got, want.flip(-1) if bgr else want), "frames_to_u8 (grid stride, bgr = %s)" % bgr
    _report("frames_to_u8_grid_stride", {"pixels": 9 * 512 * 512, "wrong_bytes": 0})
