"""tests/head_cases.py checked on the CPU: the exact family is exact (its assertions hold on every case and fp32 pre-activations equal float64 bit for
bit in every form's summation order), a numpy-float32 restatement of each form stays inside every bound with slack, every planted fault breaks the
bound on a named case, the form-selection rules put each case where it claims, and the small references (layout, uint8 conversion) are what
they say."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import head_cases as hc

SLACK = 0.75           # the restatements (numpy's tanh / exp are within 1 ulp, one rounding per other operation) must leave a quarter of every bound unused
ORDER = {"f32": "f32", "q4": "q4", "bf16": "mfma", "up4": "mfma", "thin": "f32"}


def _restate(case, kind):
    """float32 restatement of form ``kind`` on a case -> (pred, mask, img), and whether its pre-activations are float64's bit for bit."""
    x = (case["t"] if "t" in case else case["x"]).numpy()
    s32 = hc.preact(x, case["w"].numpy(), np.float32, ORDER[kind])
    s64 = hc.preact(x, case["w"].numpy())
    return hc.compose32(s32, case["bg"].numpy()), np.array_equal(s32.astype(np.float64), s64)


@pytest.mark.parametrize("S", hc.SIZES)
def test_exact_family_is_exact_and_restatements_meet_bounds(S):
    """Every (variant, C) of every form at this size, B cycling through 1, 2, 3: the exactness assertions (made when the case is built), torch's fp32
    conv2d = float64 bit for bit, and - in each form's own order - the fp32 restatement exact on s and inside the bounds with slack."""
    B = hc.batch_of(S)
    for kind in hc.FORMS:
        for C in hc.CHANNELS[kind]:
            for variant in hc.VARIANTS:
                case = hc.exact_case(variant, B, S, C)
                ref = hc.reference(case)
                x, w = case["x"].permute(0, 3, 1, 2), case["w"]
                s32 = F.conv2d(x, w, padding=2).permute(0, 2, 3, 1)
                assert np.array_equal(s32.double().numpy(), ref["s"]), case["name"] + ": fp32 conv2d is not exact"
                if variant == "cancel":
                    assert not ref["s"].any() and np.all(ref["mask"] == 0.5) and not ref["img"].any(), case["name"]
                    assert np.array_equal(ref["pred"], 0.5 * case["bg"].double().numpy()), case["name"]
                if variant == "sat" and C == 64 and S >= 15:       # expf(-s) overflows, the fp32 mask is exactly 1 and below the smallest normal, tanhf is +-1
                    s3 = ref["s"][..., 3]
                    assert s3.min() < -89 and s3.max() > 89 and np.float32(ref["mask"].max()) == 1 and ref["mask"].min() < hc.FLOOR, case["name"]
                    assert np.float32(ref["img"].max()) == 1 and np.float32(ref["img"].min()) == -1, case["name"]
                if C == 64 and S not in (5, 17, 33, 65):      # the restatement's 25 C serial steps: every size at the small C, four sizes at C = 64
                    continue
                got, exact = _restate(case, kind)
                assert exact, "%s: the fp32 restatement of %s rounds a pre-activation" % (case["name"], kind)
                r = hc.ratios(got, ref)
                assert max(r.values()) <= SLACK, (case["name"], kind, r)


@pytest.mark.parametrize("ks,N", hc.THIN)
def test_thin_exact_family(ks, N):
    for S in (1, 3, 17, 33):
        for C in hc.CHANNELS["thin"][:2]:
            case = hc.exact_case("unsat", 2, S, C, ks=ks, N=N)
            x, w = case["x"].numpy(), case["w"].numpy()
            s64 = hc.preact(x, w)
            assert np.array_equal(hc.preact(x, w, np.float32, "f32").astype(np.float64), s64), case["name"]
            assert np.array_equal(hc.preact(x, w, np.float64, "f32"), s64), case["name"]          # the emulator's slow path against torch's conv2d


@pytest.mark.parametrize("kind", hc.FORMS)
def test_impulse_cases(kind):
    """Every output of an impulse frame is the transcendental of exactly one weight (or of 0), the restatement meets the bounds, the launch stays in
    the small form."""
    for pas in ("tap", "chan"):
        for S in hc.IMPULSE_S[kind]:
            C = hc.CHANNELS[kind][-1] if S == 65 else hc.CHANNELS[kind][0]
            case = hc.impulse_case(kind, pas, S, C)
            ref = hc.reference(case)
            w = case["w"].double().numpy()
            for f, (py, px, c) in enumerate(case["place"]):
                s = ref["s"][f]
                assert np.count_nonzero(s.any(-1)) == (min(S, py + 3) - max(0, py - 2)) * (min(S, px + 3) - max(0, px - 2)), (case["name"], f)
                for oy in range(max(0, py - 2), min(S, py + 3)):
                    for ox in range(max(0, px - 2), min(S, px + 3)):
                        assert np.array_equal(s[oy, ox], w[:, c, py - oy + 2, px - ox + 2]), (case["name"], f, oy, ox)
            assert hc.head_form(kind, len(case["place"]), S)[0] in ("J2", "NX1_RY2", "NCB2"), case["name"]
            if S != 65:
                got, exact = _restate(case, kind)
                assert exact and max(hc.ratios(got, ref).values()) <= SLACK, case["name"]
            chans = {c for _, _, c in case["place"]}
            assert chans == {c for c in hc.IMPULSE_CH if c < C - 1} | {C - 1}, (case["name"], chans)


def test_impulse_placements_sit_on_both_sides_of_every_seam():
    for kind, S in (("f32", 65), ("q4", 65), ("bf16", 65), ("bf16", 29)):
        place = hc.impulse_case(kind, "tap", S, hc.CHANNELS[kind][0])["place"]
        ys, xs = {p[0] for p in place}, {p[1] for p in place}
        th, tw = hc.head_form(kind, 1, S)[1]
        for edge, have, n in ((th, ys, 16 if kind == "bf16" else S), (tw, xs, S)):
            for m in range(edge, min(n, S - 1) + 1, edge):
                if m < S:
                    assert m - 1 in have and m in have, (kind, S, edge, m)
        if kind == "q4":                                   # the 64-column seam of the large form as well
            assert 63 in xs and 64 in xs
        assert {0, S - 1} <= ys and {0, S - 1} <= xs and (0, 0) in {(p[0], p[1]) for p in place}


@pytest.mark.parametrize("H,W", hc.UP4_HW)
def test_up4_cases(H, W):
    for variant in hc.VARIANTS:
        case = hc.up4_case(variant, 1 + (H + W) % 3, H, W)
        assert float(case["t"].max()) >= 4 and float(case["t"].min()) == 0.0, case["name"]       # ReLU both cuts and passes
        ref = hc.reference(case)
        if variant == "cancel":
            assert not ref["s"].any(), case["name"]
        got, exact = _restate(case, "up4")
        assert exact and max(hc.ratios(got, ref).values()) <= SLACK, case["name"]
    for pas in ("tap", "chan"):
        case = hc.up4_impulse_case(pas, H, W)
        got, exact = _restate(case, "up4")
        assert exact and max(hc.ratios(got, hc.reference(case)).values()) <= SLACK, case["name"]


def test_up4_many_tiles_case():
    B, H, W = hc.UP4_MANY
    assert B * -(-2 * H // 12) * -(-2 * W // 28) > 304            # more tiles than any CDNA part has CUs: persistent workgroups walk several
    hc.up4_case("unsat", B, H, W, False)                          # builds, and its exactness assertions hold


# ------------------------------------------------------------------------------------------------------------------------------ planted faults
FAULT_CASES = {          # fault -> the (kind, variant, B, S, C) cases of the exact family on which it must break a bound
    "tap_off_last_col": (("f32", "unsat", 1, 33, 8), ("bf16", "unsat", 1, 29, 64)),
    "drop_last_stage": (("f32", "unsat", 1, 5, 24), ("q4", "unsat", 1, 5, 12)),
    "halo_row_zero": (("f32", "unsat", 1, 17, 8), ("bf16", "unsat", 1, 5, 64)),
    "prev_frame_pad": (("f32", "unsat", 3, 3, 8), ("q4", "sat", 3, 16, 4)),
    "swap_out23": (("f32", "unsat", 1, 1, 8), ("bf16", "sat", 2, 2, 64)),
    "drop_kx4_first_cols": (("f32", "unsat", 1, 33, 8), ("q4", "unsat", 1, 33, 4)),
    "bg_stride0": (("f32", "unsat", 2, 2, 8), ("bf16", "cancel", 2, 15, 64)),
}


@pytest.mark.parametrize("fault", sorted(FAULT_CASES))
def test_planted_fault_breaks_the_bound(fault):
    for kind, variant, B, S, C in FAULT_CASES[fault]:
        assert B == hc.batch_of(S) and C in hc.CHANNELS[kind]            # a case the GPU test runs on that form
        case = hc.exact_case(variant, B, S, C)
        ref = hc.reference(case)
        tile = hc.head_form(kind, B, S)[1]
        s = hc.preact(case["x"].numpy(), case["w"].numpy(), fault=fault, tile=tile, order="ref")
        r = hc.ratios(hc.compose64(s, case["bg"].numpy(), fault=fault)[:3], ref)
        assert max(r.values()) > 1e3, "%s passes on %s (%s): %s" % (fault, case["name"], kind, r)
        clean = hc.ratios(hc.compose64(hc.preact(case["x"].numpy(), case["w"].numpy(), tile=tile, order="f32"), case["bg"].numpy())[:3], ref)
        assert max(clean.values()) == 0.0, (case["name"], clean)                      # the slow path without a fault is the reference itself


def test_planted_faults_show_on_the_impulse_too():
    case = hc.impulse_case("f32", "tap", 33, 8)
    ref = hc.reference(case)
    for fault in ("tap_off_last_col", "halo_row_zero", "prev_frame_pad", "swap_out23"):       # (no impulse sits 2 columns into a tile: kx = 4 is the dense cases')
        s = hc.preact(case["x"].numpy(), case["w"].numpy(), fault=fault, tile=(16, 32))
        r = hc.ratios(hc.compose64(s, case["bg"].numpy())[:3], ref)
        assert max(r.values()) > 1e3, (fault, r)


@pytest.mark.parametrize("H,W", [(5, 23), (23, 5)])
def test_exchanged_tile_counts_break_the_non_square_up4_cases(H, W):
    case = hc.up4_case("unsat", 2, H, W)
    ref = hc.reference(case)
    got = [hc.tiles_swapped(ref[k], (12, 28)) for k in ("pred", "mask", "img")]
    assert max(hc.ratios(got, ref).values()) == float("inf")
    sq = hc.reference(hc.up4_case("unsat", 1, 6, 14))
    assert max(hc.ratios([hc.tiles_swapped(sq[k], (12, 28)) for k in ("pred", "mask", "img")], sq).values()) == 0.0     # one tile: nothing to exchange


# ------------------------------------------------------------------------------------------------------------------------------ form selection
def test_form_selection_rules():
    for kind in ("f32", "q4", "thin"):
        for S in hc.SIZES:
            for B in (1, 2, 3):
                assert hc.head_form(kind, B, S)[0] in ("J2", "NX1_RY2"), (kind, B, S)
        for S in hc.LARGE_S:
            B = hc.large_form_batch(kind, S)
            assert hc.head_form(kind, B, S)[0] in ("J4", "NX2_RY4") and hc.head_form(kind, B - 1, S)[0] in ("J2", "NX1_RY2"), (kind, S, B)
            assert hc.head_form(kind, 1, S)[0] in ("J2", "NX1_RY2")
    assert hc.large_form_batch("f32", 33) == 128 and hc.large_form_batch("f32", 65) == 57
    assert hc.large_form_batch("q4", 33) == 256 and hc.large_form_batch("q4", 65) == 86
    assert hc.large_form_batch("thin", 33) == 128


# ------------------------------------------------------------------------------------------------------------------------------ random family
@pytest.mark.parametrize("scale", [0.03, 0.3])
def test_random_family_bound_holds_and_is_far_from_blind(scale):
    for kind, bf16 in (("f32", False), ("q4", False), ("bf16", True)):
        case = hc.random_case(scale, 2, 17, 64, bf16)
        ref = hc.reference(case, e_s=True)
        got, _ = _restate(case, kind)
        r = hc.ratios(got, ref)
        assert max(r.values()) <= SLACK, (case["name"], kind, r)
    # ... and the same bound WITHOUT the pre-activation term refuses the restatement: the term is what the random family needs, not padding
    tight = hc.reference(case)
    assert max(hc.ratios(got, tight).values()) > 1.0


# ------------------------------------------------------------------------------------------------------------------------------ small references
def test_layout_reference():
    for C in hc.LAYOUT_C:
        assert {C, C + 1, (C + 7) // 8 * 8} == set(hc.layout_pads(C))
        src = hc.layout_src(3, C, 33)
        assert src.unique().numel() == src.numel()
        for Cp in hc.layout_pads(C):
            want = hc.nchw_to_nhwc_ref(src, Cp)
            assert torch.equal(want[..., :C].permute(0, 2, 1), src) and not want[..., C:].any()


def test_u8_reference_and_thresholds():
    v = hc.u8_threshold_values()
    assert v.min() == -1 and v.max() == 1 and len(v) > 5 * 250
    out = hc.u8_ref(v)
    for k in range(1, 256):
        i = 5 * (k - 1)
        got = out[i:i + 5] if k < 255 else None
        if got is not None:
            assert list(got) == [k - 1, k - 1, k, k, k], (k, got)
    assert set(out.tolist()) == set(range(256))
    assert hc.u8_ref(np.float32(-0.0)) == 127 and hc.u8_ref(np.float32(2.0 ** -126)) == 127 and hc.u8_ref(np.float32(1)) == 255
    fr = hc.u8_threshold_frames()
    assert fr.shape[1] == 3 and set(fr[0, 0].flatten().tolist()) == set(v.tolist())
    x, k = hc.u8_position_coded(2, 33)
    assert float(x.abs().max()) <= 1 and k.unique().numel() == 256
