"""tests/bf16conv_cases.py checked on the CPU: the exact family is exact on every case (bf16-exact operands and references, float32 = float64 bit for
bit, the integer bounds), the plain restatement of the convolution equals torch's, every planted fault changes every case that claims to expose it,
what the Gaussian 1.2e-2 criterion of gpu_checks._bf16_kernel_case makes of the same faults, the coded impulses name their weight, and
``bf16_form`` is the text of the launch rules and puts every case on the kernel form its section is about."""
import os
import re

import pytest
import torch

from ipercore_amd import ops
from tests import bf16conv_cases as bc
from tests import emu_ops
from tests import test_gpu_bf16_conv_exact as gx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ipercore_amd", "csrc")
CUS = 256                   # the MI355X; the CU-dependent shapes are built for the device's own count on the GPU and for two counts here

GROUPS = {
    "hr2_cross_64": lambda: bc.hr2_cross(64),
    "hr2_cross_128": lambda: bc.hr2_cross(128),
    "hr2_axes": bc.hr2_axes,
    "hr2_parity": bc.hr2_parity,
    "hr2_acc": bc.hr2_acc,
    "up4": bc.up4_cases,
    "general_small": bc.general_small,
    "general_lds_route": bc.general_lds_route,
    "general_big": lambda: bc.general_big(CUS),
    "pw_small": bc.pw_small,
    "pw_persistent": lambda: [bc.pw_persistent(CUS, C) for C in bc.PW_BM],
    "c8_small": bc.c8_small,
    "c8_second_pass": bc.c8_second_pass,
    "wino_cross": bc.wino_cross,
    "wino_axes": bc.wino_axes,
    "ties": bc.tie_cases,
    "impulses": bc.impulse_cases,
}
BIG = ("general_big", "pw_persistent", "c8_second_pass")


def _code(name):
    """csrc/<name> without its comments."""
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def test_case_names_are_unique():
    names = [c.name for g in GROUPS.values() for c in g()]
    assert len(names) == len(set(names)) and len(names) > 400


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_family_conditions_and_restatement(group):
    """Every case of the group: the family's conditions (bc.assert_family) and, on the small cases, restated(case) == torch's convolution."""
    for case in GROUPS[group]():
        bc.assert_family(case)
        if group not in BIG:
            assert torch.equal(bc.restated(case), bc.reference(case)), case.name
        bc.reference.cache_clear()
        bc.operands.cache_clear()


@pytest.mark.parametrize("group", ("hr2_axes", "hr2_parity", "up4", "general_small", "general_lds_route", "pw_small", "c8_small", "wino_axes", "ties", "impulses"))
def test_packed_cases_compute_the_reference_under_the_emulation(group):
    """What the GPU test hands to the library - the packed specs (the hand-built 10-tap one among them), the framed residual, the SPADE operands,
    the channel slice - run through the CPU emulation of the conv contract (tests/emu_ops.py, fp32: exact on these families) gives the reference."""
    for case in GROUPS[group]()[::3]:
        o = bc.operands(case)
        sp = gx._specs(case, o, "cpu")
        oh, ow = bc.out_hw(case)
        n = bc.out_channels(case)
        y = torch.full((case.B, oh, ow, n + case.pad), float("nan"))
        ycoff = 8 if case.pad else 0
        if case.kind == "convT":
            for s in sp:
                emu_ops.conv2d(o["x0"], s, y, act=gx.ACT[case.act], ycoff=ycoff)
        else:
            kw = dict(x1=o["x1"], epi=gx.EPI[case.epi], act=gx.ACT[case.act], ycoff=ycoff)
            if case.epi == "res":
                kw["res"] = gx._framed(case, o["res"], torch.float32, "cpu")
            if case.epi == "spade":
                kw.update(xn=o["xn"], mean=o["mean"], rstd=o["rstd"])
            emu_ops.conv2d(o["x0"], sp, y, **kw)
        assert torch.equal(y[..., ycoff:ycoff + n], bc.reference(case, torch.float32)), case.name
        assert not case.pad or bool(torch.isnan(y[..., :8]).all() and torch.isnan(y[..., 8 + n:]).all())
        bc.reference.cache_clear()
        bc.operands.cache_clear()
    assert ops.BF16_HR and ops.BF16_PW and ops.BF16_C8 and ops.BF16_UP4


def test_worst_sums_stay_inside_bf16():
    """The largest K of the lists: Cin = 384 (the 128 + 256 concat), 3 x 3, at the largest image - the family's margin to 256."""
    worst = max((c for c in bc.hr2_axes() if c.C0 + c.C1 == 384 and (c.H, c.W) == (17, 33)), key=lambda c: c.N)
    m = float(bc.reference(worst).abs().max())
    assert 100 <= m <= 256, m


@pytest.mark.parametrize("group", sorted(set(GROUPS) - {"hr2_acc", "wino_cross", "wino_axes", "ties", "impulses", "general_big", "c8_second_pass"}))
def test_planted_faults_change_every_case_that_claims_them(group):
    seen = set()
    for case in GROUPS[group]():
        ref = bc.reference(case)
        for fault in sorted(bc.covers(case, CUS)):
            assert fault in bc.FAULTS
            got = bc.restated(case, fault, CUS)
            assert not torch.equal(got, ref), (case.name, fault)
            seen.add(fault)
        bc.reference.cache_clear()
        bc.operands.cache_clear()
    want = {"hr2_cross_64": {"drop_tap_row", "drop_tap_col", "halo_neighbour", "skip_last_odd_chunk", "bias_next_tile"},
            "hr2_axes": {"drop_tap_row", "drop_tap_col", "halo_neighbour", "skip_last_odd_chunk", "swap_concat", "bias_next_tile"},
            "hr2_parity": {"drop_tap_row", "drop_tap_col", "halo_neighbour", "skip_last_odd_chunk", "parity_swap", "bias_next_tile"},
            "up4": {"drop_tap_row", "drop_tap_col", "halo_neighbour", "skip_last_odd_chunk", "parity_swap", "bias_next_tile"},
            "general_small": {"drop_tap_row", "drop_tap_col", "swap_concat", "skip_last_odd_chunk", "bias_next_tile"},
            "pw_persistent": {"pw_stale_tile", "bias_next_tile"}}.get(group, {"drop_tap_row", "bias_next_tile"})
    assert want <= seen, (group, want - seen)


def test_covers_is_honest_about_what_it_leaves_out():
    """A fault a case does not claim is one the case cannot show: the restatement with it equals the reference (spot checks of each rule)."""
    c = bc.hr2_cross(64)
    one = next(k for k in c if (k.H, k.W) == (9, 15))
    assert {"drop_tap_col", "halo_neighbour"}.isdisjoint(bc.covers(one))
    for fault in ("drop_tap_col", "halo_neighbour", "swap_concat", "parity_swap"):
        assert torch.equal(bc.restated(one, fault), bc.reference(one)), fault
    two = next(k for k in bc.hr2_axes() if k.name == "hr2_chunks2_9x17")
    assert "skip_last_odd_chunk" not in bc.covers(two) and torch.equal(bc.restated(two, "skip_last_odd_chunk"), bc.reference(two))
    small = next(k for k in bc.pw_small() if k.name == "pw_C128_M259")
    assert "pw_stale_tile" not in bc.covers(small) and torch.equal(bc.restated(small, "pw_stale_tile"), bc.reference(small))
    for C in bc.PW_BM:
        f = bc.bf16_form(bc.pw_persistent(CUS, C), CUS)
        assert f.info["walk"] == 3 and f.info["tiles"] == 2 * f.info["slots"] + 2 and bc.rows(bc.pw_persistent(CUS, C)) % f.tile[0] == 5


def test_what_the_gaussian_criterion_makes_of_the_faults():
    """gpu_checks._bf16_kernel_case's data and criterion (max |d| <= 1.2e-2 of the reference's maximum after rounding to bf16) on the planted faults,
    the drop faults at width = 1: ONE product lost per output along a block seam.
    Figures (printed): the maximum over a whole seam does rise above the criterion - 0.067 / 0.064 (64 -> 128, row / column seam) and 0.031 / 0.030
    (256 -> 256) of the reference's maximum against 0.012 -, because among the thousands of outputs on a seam some lose a product from the tail of
    |x w|; bias from the next 32-column tile gives 0.09 - 0.10 (the biases are 0.1 N(0, 1): two of them differ by 0.14 on average).  So the Gaussian
    check sees these faults only through the largest few of the products it happens to draw: 84 - 95 % of the CHANGED outputs sit inside the
    criterion, and a fault confined to a few dozen outputs (one block corner, one column quad of one pixel row) passes it whole.
    Asserted, from the distributions and not from these figures: the sound restatement passes; more than half of the outputs a dropped product
    changes are inside the criterion (x ~ N(0, 1), w ~ N(0, 1 / 9 Cin), reference maximum >= 3 sigma of a unit-variance output: the criterion hides
    |x w| sqrt(9 Cin) <= 0.036 sqrt(9 Cin) >= 0.86, and the median of a product of two standard normals is 0.46); on the exact family the same
    fault moves every output it touches by a whole integer."""
    for case in bc.gaussian_cases():
        ref = bc.reference(case)
        wmax = float(ref.abs().max())
        assert wmax >= 3.0
        assert bc.gauss_rel(case, bc.restated(case)) <= bc.GAUSS_TOL, case.name
        for fault in ("drop_tap_row", "drop_tap_col", "bias_next_tile", "halo_neighbour"):
            got = bc.restated(case, fault, width=1)
            d = (got.float().to(torch.bfloat16).double() - ref).abs()
            changed = got != ref
            hidden = float(((d <= bc.GAUSS_TOL * wmax) & changed).sum()) / max(1.0, float(changed.sum()))
            print("%s %-15s rel %.4f  changed outputs %d  of them within the criterion %.1f %%" % (case.name, fault, bc.gauss_rel(case, got), int(changed.sum()), 100 * hidden))
            if fault in ("drop_tap_row", "drop_tap_col"):
                assert int(changed.sum()) > 1000 and hidden > 0.5, (case.name, fault, hidden)
    exact = next(k for k in bc.hr2_axes() if k.name == "hr2_chunks4_17x33")
    for fault in ("drop_tap_row", "drop_tap_col"):
        d = (bc.restated(exact, fault, width=1) - bc.reference(exact)).abs()
        assert int((d != 0).sum()) > 500 and set(d.unique().tolist()) == {0.0, 1.0}, fault


def test_impulse_outputs_name_their_weight():
    for case in bc.impulse_cases():
        bc.assert_family(case)
        ref, w = bc.reference(case), bc.operands(case)["w"]
        assert len({p[:2] for p in case.extra}) == 4 and {p[2] for p in case.extra} >= {0, case.C0 - 1}, case.name
        for b, (py, px, c) in enumerate(case.extra):
            nz = ref[b].abs().sum(-1) > 0
            assert int(nz.sum()) >= 1, (case.name, b)
            oy, ox = (int(v[0]) for v in torch.nonzero(nz)[0].split(1))
            hits = bc.impulse_decode(case, ref[b, oy, ox, 3].item())
            cdim = 0 if case.kind == "convT" else 1
            assert hits and all(h[cdim] == c or w.numel() > 65024 for h in hits) and any(h[cdim] == c and h[1 - cdim] == 3 for h in hits), (case.name, b, hits)
    code = bc.impulse_code(65024)
    assert len(set(code.tolist())) == 65024 and bc.bf16_exact(code) and bool(torch.isfinite(code).all()) and float(code.abs().min()) >= 2.0 ** -126


def test_winograd_transforms_of_the_family_are_bf16_exact():
    """U = G w G^T of ternary weights: multiples of 1/4 of magnitude <= 9/4; V = B^T d B of ternary inputs: integers of magnitude <= 4."""
    G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)
    Bt = torch.tensor([[1.0, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
    case = bc.wino_axes()[0]
    o = bc.operands(case)
    U = torch.einsum("ar,ncrs,bs->ncab", G, o["w"].double(), G)
    assert bc.bf16_exact(U) and float(U.abs().max()) <= 2.25 and torch.equal(4 * U, (4 * U).round())
    worst = torch.einsum("ar,rs,bs->ab", G, torch.ones(3, 3, dtype=torch.float64), G)
    assert float(worst.abs().max()) == 2.25
    d = torch.tensor([[1.0, 0, -1, 0], [0, 1, 1, 0], [-1, 1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
    V = Bt @ d @ Bt.t()
    assert float((Bt.abs() @ torch.ones(4, 4, dtype=torch.float64) @ Bt.abs().t()).max()) == 4.0 and bc.bf16_exact(V)


# ------------------------------------------------------------------------------------------------------------------------------ bf16_form
def test_bf16_form_is_the_text_of_the_launch_rules():
    k = _code("conv_igemm_bf16.hip")
    h = _code("lwg_common.h")
    for define in ("#define LWG_BF16_PW_TM 2", "#define LWG_BF16_DMA_A 1", "#define LWG_BF16_TILE64 0", "#define LWG_BF16_BIG 1"):
        assert define in h, define
    for rule in (
            # launch_epi_bf16: 256 x 256, then "small", then 128 x 128 | 128 x 64
            "if (LWG_BF16_BIG && dma_a && a.N % 256 == 0 && (long)((a.M + 255) / 256) * (a.N / 256) >= (long)cus) return launch_cfg_bf16<2, 4, 4, 2, EPI, true>(a, stream);",
            "const long tiles128 = (long)((a.M + 127) / 128) * (a.N / 128);",
            "const bool small = a.N % 128 == 0 && tiles128 < 2L * cus;",
            "if (EPI == LWG_EPI_SPADE || (a.N % 128 == 0 && LWG_BF16_TILE64 != 1 && !(small && LWG_BF16_TILE64 == 0)))\n        return launch_cfg_bf16<2, 2, 2, 2, EPI, dma_a>(a, stream);\n    return launch_cfg_bf16<4, 1, 1, 2, EPI, dma_a>(a, stream);",
            "return cd_epi_dispatch(a, 128, true, [&](auto epi) { return launch_epi_bf16<decltype(epi)::value>(a, stream); });",
            # launch_epi_bf16_hr
            "if (lwg_bf16_tap_grid(a, 3, 3)) return a.N % 128 == 0 ? launch_cfg_bf16_hr2<3, 3, EPI, 1>(a, stream) : launch_cfg_bf16_hr2<3, 3, EPI, 2>(a, stream);",
            "if (lwg_bf16_tap_grid(a, 2, 2)) return a.N % 128 == 0 ? launch_cfg_bf16_hr2<2, 2, EPI, 1>(a, stream) : launch_cfg_bf16_hr2<2, 2, EPI, 2>(a, stream);",
            "const long tiles = (long)a.B * ((a.OH + 7) / 8) * ((a.OW + 15) / 16) * (a.N / (128 / WAVES_M));",
            # the pointwise kernel
            "if (a.N == 64) return (int)launch_cfg_bf16_pw<1, 2>(a, stream);", "if (a.N == 128) return (int)launch_cfg_bf16_pw<2, 4>(a, stream);",
            "return (int)launch_cfg_bf16_pw<4, 8>(a, stream);", "return launch_cfg_bf16_pw_tm<NCH, WAVES_N, LWG_BF16_PW_TM>(a, stream);",
            "constexpr int BM = (8 / WAVES_N) * TM * 32;", "const int ntiles = (a.M + BM - 1) / BM;", "const int slots = lwg_device_cus() * (TM == 4 ? 1 : 2);",
            "dim3((unsigned)(ntiles < slots ? ntiles : slots))",
            "(a.N == 64 || a.N == 128 || a.N == 256) && a.H == a.OH && a.W == a.OW;",
            # the fused transposed convolution
            "if (a.N % 128 == 0) return (int)(a.C0 == 64 ? launch_cfg_bf16_up4<1, 1>(a, stream) : launch_cfg_bf16_up4<2, 1>(a, stream));",
            "return (int)(a.C0 == 64 ? launch_cfg_bf16_up4<1, 2>(a, stream) : launch_cfg_bf16_up4<2, 2>(a, stream));",
            # the first layer
            "const int ngroups4 = (a.M + 255) / 256;", "dim3((unsigned)(ngroups4 < 2048 ? ngroups4 : 2048)), dim3(256), 0, stream, a, (a.ntaps + 1) / 2);",
            "for (int g = blockIdx.x * 4 + wid; g < ngroups; g += gridDim.x * 4) {",
            # the accumulator frame
            "hipLaunchKernelGGL((lwg_conv_bf16_hr2_kernel<3, 3, LWG_EPI_NONE, 1, HR2_ACC>)"):
        assert rule in k, rule
    hl = _code("lwg_bf16_hr_list.h")
    assert "CW_FN int hrl_acc_column(int khalf, int r) { return 8 * (r >> 2) + 4 * khalf + (r & 3); }" in hl
    assert "{ return ((size_t)oy * W + ox) * (size_t)N + (size_t)(ncol + 16 * khalf); }" in hl
    cols = bc.acc_frame_columns(128).tolist()
    assert sorted(cols) == list(range(128)) and all(cols[32 * t + 16 * kh + r] == 32 * t + 8 * (r >> 2) + 4 * kh + (r & 3)
                                                    for t in range(4) for kh in range(2) for r in range(16))
    for n, (nch, wn) in {64: (1, 2), 128: (2, 4), 256: (4, 8)}.items():
        assert bc.PW_BM[n] == (8 // wn) * 2 * 32 and nch == n // 64 and wn == n // 32
    o = re.sub(r"#[^\n]*", "", open(os.path.join(ROOT, "ipercore_amd", "ops.py")).read())
    for rule in (
            "if not BF16_HR or spec.stride != 1 or spec.ntaps not in (9, 4) or spec.N % 64 != 0 or spec.Cin % 64 != 0:",
            "if not BF16_PW or spec.ntaps != 1 or spec.stride != 1 or spec.omul != 1 or x1 is not None or epi != EPI_NONE:",
            "if spec.dy[0] != 0 or spec.dx[0] != 0 or spec.N != spec.Cin or spec.N not in (64, 128, 256):",
            "if BF16_C8 and spec.Cin == 8 and spec.N == 64 and spec.ntaps <= 10 and x1 is None and epi == EPI_NONE and spec.omul == 1:",
            "if (BF16_UP4 and BF16_HR and x.dtype == torch.bfloat16 and y.dtype == torch.bfloat16 and len(specs) == 4 and s0.Cin in (64, 128)",
            "if mode == \"bf16_winograd\" and _bf16_wino_eligible(spec, x0, y, x1, epi, act, out_hw, ycoff):",
            "if hr or _pw_eligible(spec, x0, y, x1, epi, out_hw):"):
        assert rule in o, rule


KERNEL_OF = {
    "hr2_cross_64": {"lwg_conv_bf16_hr2_kernel<3,3,2>"}, "hr2_cross_128": {"lwg_conv_bf16_hr2_kernel<3,3,1>"},
    "hr2_axes": {"lwg_conv_bf16_hr2_kernel<3,3,1>", "lwg_conv_bf16_hr2_kernel<3,3,2>"},
    "hr2_parity": {"lwg_conv_bf16_hr2_kernel<2,2,1>", "lwg_conv_bf16_hr2_kernel<2,2,2>"},
    "hr2_acc": {"lwg_conv_bf16_hr2_kernel<3,3,1,ACC>"},
    "up4": {"lwg_conv_bf16_up4_kernel<%d,%d>" % (n, w) for n in (1, 2) for w in (1, 2)},
    "general_small": {"lwg_conv_bf16_kernel<4,1,1,2>", "lwg_conv_bf16_kernel<2,2,2,2>"},
    "general_lds_route": {"lwg_conv_bf16_kernel<4,1,1,2>", "lwg_conv_bf16_kernel<2,2,2,2>"},
    "general_big": {"lwg_conv_bf16_kernel<2,4,4,2>", "lwg_conv_bf16_kernel<2,2,2,2>"},
    "pw_small": {"lwg_conv_bf16_pw_kernel<1,2,2>", "lwg_conv_bf16_pw_kernel<2,4,2>", "lwg_conv_bf16_pw_kernel<4,8,2>"},
    "pw_persistent": {"lwg_conv_bf16_pw_kernel<1,2,2>", "lwg_conv_bf16_pw_kernel<2,4,2>", "lwg_conv_bf16_pw_kernel<4,8,2>"},
    "c8_small": {"lwg_conv_c8_bf16_kernel"}, "c8_second_pass": {"lwg_conv_c8_bf16_kernel"},
    "wino_cross": {"lwg_conv_winograd_bf16_kernel"}, "wino_axes": {"lwg_conv_winograd_bf16_kernel"},
}


@pytest.mark.parametrize("cus", (256, 304, 64))
def test_every_section_reaches_the_forms_it_is_about(cus):
    groups = dict(GROUPS, general_big=lambda: bc.general_big(cus), pw_persistent=lambda: [bc.pw_persistent(cus, C) for C in bc.PW_BM])
    for group, kernels in KERNEL_OF.items():
        got = {bc.bf16_form(c, cus).kernel for c in groups[group]()}
        assert got == kernels, (group, got)
    big = {c.name.split("_cus")[0]: bc.bf16_form(c, cus) for c in bc.general_big(cus)}
    assert big["big256_1x1"].kernel == big["big256_s2"].kernel == "lwg_conv_bf16_kernel<2,4,4,2>" and big["big256_1x1"].info["tiles_m"] == cus + 1
    assert big["big128_1x1"].kernel == "lwg_conv_bf16_kernel<2,2,2,2>" and big["big128_1x1"].info["tiles_m"] == 2 * cus + 1
    for c in bc.general_big(cus)[:2]:                              # one row fewer than a tile per CU: the launch would fall back to the 4-wave forms
        M = bc.rows(c)
        assert M % 256 == 37 and (M - 37) // 256 == cus
    for C in bc.PW_BM:
        f = bc.bf16_form(bc.pw_persistent(cus, C), cus)
        assert f.info["walk"] == 3 and f.info["slots"] == 2 * cus
    assert all(bc.bf16_form(c, cus).info["walk"] == 1 for c in bc.pw_small())
    assert all(bc.bf16_form(c, cus).info == {"grid": 2048, "passes": 2} for c in bc.c8_second_pass())
    assert [bc.rows(c) for c in bc.c8_second_pass()] == [2048 * 256 + 257, 727 * 727]
    assert {bc.bf16_form(c, cus).info["passes"] for c in bc.c8_small()} == {1}
    small = {bc.bf16_form(c, cus).kernel for c in bc.general_small() if c.epi != "spade"}
    assert small == {"lwg_conv_bf16_kernel<4,1,1,2>"}
    assert {bc.bf16_form(c, cus).kernel for c in bc.general_small() if c.epi == "spade"} == {"lwg_conv_bf16_kernel<2,2,2,2>"}
    assert {bc.bf16_form(c, cus).info["chunks"] for c in bc.hr2_axes()} == {1, 2, 3, 4, 5, 6}
    assert {bc.bf16_form(c, cus).info["chunks"] for c in bc.hr2_parity()} == {3, 4}
    lds = {c.name: bc.bf16_form(c, cus) for c in bc.general_lds_route()}
    assert all(f.entry == "lwg_conv2d_nhwc_bf16" for f in lds.values()) and lds["lds_3x3_spade"].kernel == "lwg_conv_bf16_kernel<2,2,2,2>"
    ties = {c.name: bc.bf16_form(c, cus).kernel for c in bc.tie_cases()}
    assert ties == {"tie_hr2_plain": "lwg_conv_bf16_hr2_kernel<3,3,2>", "tie_hr2_spade": "lwg_conv_bf16_hr2_kernel<3,3,1>", "tie_lds_plain": "lwg_conv_bf16_kernel<4,1,1,2>",
                    "tie_lds_spade": "lwg_conv_bf16_kernel<2,2,2,2>", "tie_c8": "lwg_conv_c8_bf16_kernel"}
    imp = {bc.bf16_form(c, cus).kernel.split("<")[0] for c in bc.impulse_cases()}
    assert imp == {"lwg_conv_bf16_hr2_kernel", "lwg_conv_bf16_up4_kernel", "lwg_conv_bf16_kernel", "lwg_conv_bf16_pw_kernel", "lwg_conv_c8_bf16_kernel"}


def test_size_lists_sit_on_both_sides_of_every_seam():
    for edge, sizes in ((8, bc.HS), (16, bc.WS)):
        assert {1, edge - 1, edge, edge + 1, 2 * edge - 1, 2 * edge, 2 * edge + 1} == set(sizes)
    assert {(min(bc.HS), min(bc.WS)), (min(bc.HS), max(bc.WS)), (max(bc.HS), min(bc.WS)), (max(bc.HS), max(bc.WS)), (9, 17)} == set(bc.REDUCED)
    ms = sorted(2 * a * b for a, b in bc.GENERAL_OHW)
    assert {254, 256, 258} <= set(ms) and 510 in ms and 512 in ms
    assert {c.B for c in bc.hr2_cross(64)} == {1, 2, 3}
    for C, bm in bc.PW_BM.items():
        assert {bc.rows(c) for c in bc.pw_small() if c.C0 == C and not c.pad} == {1, bm - 1, bm, bm + 1, 2 * bm + 3}
    assert {63, 64, 65, 255, 257} <= {bc.rows(c) for c in bc.c8_small()}
