"""tests/lbs_cases.py held against itself, on the CPU: every stage bound against the numpy-float32 restatement of the skinning kernels on every
case, the end-to-end bounds against the fp32 oracle (tests/emu_ops.smpl_lbs), and against eight planted errors, each of which the assertions of
tests/test_gpu_lbs_kernels.py must refuse on a named case.  The same planted errors are then run through the check the suite had before
(gpu_checks.check_lbs: the synthetic SMPL-H dict, natural poses, 1e-5) and what that check lets through is printed - the gap on record in
DESIGN.md section 3.6.  Also here: the workspace layout the GPU test reads, pinned on the text of csrc/lbs.hip, and the host glue of bodynets.py
(_offsets_rows, _links_2d) through the emulated ABI."""
import json
import os
import re

import numpy as np
import pytest
import torch

from ipercore_amd import synthetic
from ipercore_amd.bodynets import SMPLH
from oracle import lwg_oracle as orc
from tests import emu_ops
from tests import lbs_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _code(name):
    with open(os.path.join(ROOT, "ipercore_amd", "csrc", name)) as fp:
        return fp.read()


def _oracle(case, links=None):
    verts, j3d, j2d = emu_ops.smpl_lbs(case["model"], case["pose"], case["beta"], case["cam"], case["offsets"], links)
    return {"verts": verts, "j3d": j3d, "j2d": j2d}


# ------------------------------------------------------------------------------------------------------------------- the cases themselves
def test_models_are_sparse_small_and_spread():
    assert len(lc.MODELS) < 12 and {m[1] for m in lc.MODELS} == {2, 24, 52, 64} and {m[2] for m in lc.MODELS} == {1, 63, 257}
    assert ("chain", 64, 257) in lc.MODELS and ("star", 64, 257) in lc.MODELS
    for kind, nj, nv in lc.MODELS:
        m = lc.make_model(kind, nj, nv)
        W, Jr, par = m["lbs_weights"], m["J_regressor"], m["parents"].tolist()
        nnz = (W != 0).sum(dim=1)
        assert W.shape == (nv, nj) and int(nnz.max()) <= 4 and int(nnz.min()) >= 1 and (nnz[0::3] == 1).all() and (W >= 0).all()
        assert (W.double().sum(dim=1) - 1).abs().max() <= 2 * lc.U * 4
        jn = (Jr != 0).sum(dim=1)
        assert Jr.shape == (nj, nv) and int(jn.max()) <= 4 and int(jn.min()) >= 1 and (Jr.double().sum(dim=1) - 1).abs().max() <= 2 * lc.U * 4
        assert par[0] == -1 and all(0 <= par[j] < j for j in range(1, nj))
        if kind == "chain":
            assert par[1:] == list(range(nj - 1))
        elif kind == "star":
            assert not any(par[1:])
        else:
            assert all(par[j] >= max(0, j - 4) for j in range(1, nj))
        assert m["v_template"].abs().max() <= 1 and m["posedirs"].shape == (9 * (nj - 1), 3 * nv) and m["shapedirs"].shape == (nv, 3, lc.NBETA)
        if nv >= nj >= 24:                  # joints O(1) apart (the synthetic dicts: within 1e-2 of one point), every joint moves a vertex
            J = (Jr.double() @ m["v_template"].double())
            d = (J[:, None] - J[None]).norm(dim=-1)
            assert float(d.median()) > 0.5 and (W != 0).any(dim=0).all()


def test_cases_cover_every_pose_kind_batch_and_offset_form():
    kinds_at_b1, forms = set(), set()
    for c in lc.CASES:
        case = lc.make_case(*c)
        B = case["pose"].shape[0]
        assert B == c[1] and len(case["kinds"]) == B and case["beta"].shape == (B, lc.NBETA) and case["cam"].shape == (B, 3)
        assert not lc.pose_excluded(case["pose"])
        if B == 1:
            kinds_at_b1.add(case["kinds"][0])
        if B > 1:
            assert len({tuple(r) for r in case["beta"].tolist()}) == B                # a different beta per frame
            if case["offsets"] is not None and case["offsets"].dim() == 3:
                assert not torch.equal(case["offsets"][0], case["offsets"][1])       # batched offsets really differ per frame
        forms.add((B, c[2]))
    assert kinds_at_b1 == set(lc.POSE_KINDS)
    assert forms == {(B, o) for B in (1, 8, 9, 17) for o in ("none", "shared", "batched")}
    nj = 24
    r = lc._rng(99)
    ang = {k: torch.from_numpy(lc.pose_row(k, nj, r)).view(nj, 3).double().norm(dim=1) for k in lc.POSE_KINDS}
    assert float(ang["zero"].max()) == 0 and abs(float(ang["tiny6"].mean()) - 1e-6) < 1e-9 and abs(float(ang["tiny4"].mean()) - 1e-4) < 1e-7
    for k in ("pi_x", "pi_y", "pi_z"):
        assert (ang[k] == lc.PI32).all()
    assert (ang["pi_rand"] - np.pi).abs().max() < 1e-6 and float(ang["wide"].max()) > 2 * np.pi and float(ang["wide"].min()) < np.pi
    assert int((ang["one_3pi2"] > 0).sum()) == 1 and abs(float(ang["one_3pi2"].max()) - 1.5 * np.pi) < 1e-6
    assert abs(float(ang["natural"][0]) - np.pi) < 0.5 and float(ang["natural"][1:].max()) < 1.5


def test_the_nan_input_is_excluded_and_is_nan_in_the_reference():
    nj = 4
    pose = torch.zeros(2, 3 * nj)
    assert not lc.pose_excluded(pose)
    pose[1, 6:9] = float(np.float32(-1e-8))
    assert lc.pose_excluded(pose)
    assert torch.isnan(orc.rotvec_to_rotmat(pose.view(-1, 3))).any()                  # the reference gives NaN there too
    pose[1, 8] = 0.0                                                                  # two coordinates vanish, the third does not: fine
    assert not lc.pose_excluded(pose) and torch.isfinite(orc.rotvec_to_rotmat(pose.view(-1, 3))).all()


def test_links_hold_both_chains_and_no_duplicate_target():
    assert lc.link_pairs(1) is None
    for nv in (63, 257):
        ln = lc.link_pairs(nv)
        to, frm = ln[:, 0].tolist(), ln[:, 1].tolist()
        assert len(set(to)) == len(to) and min(to + frm) >= 0 and max(to + frm) < nv
        assert to[1] == frm[0] and to[2] == frm[1]                                    # reader first
        assert to[3] == frm[4] and to[4] == frm[5]                                    # writer first
        verts = torch.arange(nv * 3, dtype=torch.float32).view(1, nv, 3)
        assert torch.equal(lc.link64(verts, ln), orc.link(verts, ln.long()))


def test_reference_agrees_with_the_oracle_in_float64():
    """ref64 is smplx's lbs: the oracle's formulas run in float64 (its fp32 constants aside) give the same vertices and joints to 1e-6 - far above
    float64 rounding, far below any error in the formulas."""
    for c in (lc.CASES[2], lc.CASES[19], lc.CASES[40], lc.CASES[-1]):
        case = lc.make_case(*c)
        ref, got = lc.case_ref64(case), _oracle(case)
        for k, r in (("verts", ref["verts"]), ("j3d", ref["G_t"]), ("j2d", ref["j2d"])):
            assert (got[k].double() - r).abs().max() < 1e-4, (case["id"], k)
        assert ref["verts"].dtype == torch.float64 and ref["G_R"].dtype == torch.float64 and ref["E_verts"].dtype == torch.float64
        GR = ref["G_R"]
        assert (GR @ GR.transpose(-1, -2) - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-12


# ------------------------------------------------------------------------------------------------ bounds against the restatement and oracle
def test_restatement_stays_within_every_stage_bound_on_every_case():
    worst = {}
    for c in lc.CASES:
        case = lc.make_case(*c)
        r = lc.stage_ratios(case, lc.lbs_f32(case))
        assert set(r) == set(lc.STAGES), (case["id"], sorted(r))
        for k, v in r.items():
            assert v <= 1.0, f"{case['id']}: the fp32 restatement misses the {k} bound: |error| / bound = {v}"
            worst[k] = max(worst.get(k, 0.0), v)
    print("lbs_cases restatement " + json.dumps({"worst_ratio": worst, "cases": len(lc.CASES)}))


def test_fp32_oracle_stays_within_the_end_to_end_bounds_on_every_case():
    """The fp32 oracle sums in other orders than the kernels (einsum, matmul), so only the end-to-end bounds apply to it - and hold only if the
    propagated counts are right.  Worst ratios per tree kind are printed (and recorded in DESIGN.md section 3.6)."""
    worst = {k: {"verts": 0.0, "j3d": 0.0, "j2d": 0.0} for k in lc.TREES}
    for c in lc.CASES:
        case = lc.make_case(*c)
        r = lc.stage_ratios(case, _oracle(case))
        assert set(r) == {"verts", "j3d", "j2d"}
        for k, v in r.items():
            assert v <= 1.0, f"{case['id']}: the fp32 oracle misses the end-to-end {k} bound: |error| / bound = {v}"
            w = worst[case["model"]["kind"]]
            w[k] = max(w[k], v)
    print("lbs_cases oracle " + json.dumps({"worst_ratio_by_tree": worst}))


def test_chain_bound_grows_with_depth():
    """What a fixed tolerance cannot do: the 64-chain's j3d bound exceeds the 64-star's by more than the depth ratio's square root, and both stay
    far below the errors the planted faults make (O(0.1))."""
    chain = lc.case_ref64(lc.make_case(lc.MODELS.index(("chain", 64, 257)), 17, "batched"))
    star = lc.case_ref64(lc.make_case(lc.MODELS.index(("star", 64, 257)), 17, "batched"))
    assert float(chain["E_t"][:, -1].min()) > 8 * float(star["E_t"][:, -1].max())
    assert float(chain["E_t"].max()) < 2e-2 and float(chain["E_verts"].max()) < 5e-2 and float(star["E_verts"].max()) < 1e-3


# --------------------------------------------------------------------------------------------------------------------------- planted errors
PLANT_CASES = tuple((mi, 17, "batched") for mi in range(len(lc.MODELS)))


def _caught(case, got, links):
    """The GPU test's assertions on a result: the stages over their bound, and the link faults."""
    over = [k for k, v in lc.stage_ratios(case, dict(got, verts=got["verts_raw"])).items() if not v <= 1.0]
    if links is not None:
        over += ["link: " + f for f in lc.link_faults(got["verts"], got["verts_raw"], links)]
    return over


@pytest.mark.parametrize("plant", lc.PLANTS)
def test_planted_error_is_refused_on_a_named_case(plant):
    caught = {}
    for c in PLANT_CASES:
        case = lc.make_case(*c)
        links = lc.link_pairs(case["model"]["lbs_weights"].shape[0])
        assert _caught(case, lc.lbs_f32(case, links=links), links) == [], case["id"]          # the unplanted restatement passes the same assertions
        over = _caught(case, lc.lbs_f32(case, links=links, plant=plant), links)
        if over:
            caught[case["id"]] = over
    print("lbs_cases planted " + json.dumps({plant: {"what": lc.PLANT_TEXT[plant], "caught_on": caught}}))
    assert caught, f"planted error '{lc.PLANT_TEXT[plant]}' passes every case"


def _synthetic_case():
    """check_lbs's inputs: the synthetic SMPL-H dict, 11 natural frames, one shared offset table, 40 random link pairs."""
    md = synthetic.smplh_model_dict(seed=0)
    body = SMPLH(md)
    theta = torch.tensor(synthetic.smpl_sequence(11, seed=1, pose_dim=72))
    offsets = torch.tensor((0.005 * synthetic._rs(3, "offsets").standard_normal((6890, 3))).astype(np.float32))
    r = synthetic._rs(4, "links")
    links = torch.tensor(np.stack([r.randint(0, 6890, size=40), r.randint(0, 6890, size=40)], axis=1).astype(np.int32))
    model = dict(body._device_model(), kind="rand")
    return {"id": "synthetic_smplh", "model": model, "pose": body._full_pose(theta[:, 3:-10].contiguous()), "beta": theta[:, -10:].contiguous(),
            "cam": theta[:, 0:3].contiguous(), "offsets": offsets, "kinds": ["natural"] * 11}, links


def test_report_what_the_old_check_lets_through():
    """Not an assertion on the plants: the record of which of them check_lbs's comparison (1e-5 max(1, max |ref|) on verts / j3d / j2d against the
    fp32 oracle, exact link gathers) would have passed.  The unplanted restatement must pass it."""
    case, links = _synthetic_case()
    want = _oracle(case, links)
    to, frm = links[:, 0].long(), links[:, 1].long()

    def old_check(got):
        fails = []
        for k in ("verts", "j3d", "j2d"):
            err = float((got[k] - want[k]).abs().max())
            if not err <= 1e-5 * max(1.0, float(want[k].abs().max())):
                fails.append(f"{k} {err:.1e}")
        if not torch.equal(got["verts"][:, to], got["verts_raw"][:, frm]):
            fails.append("link gather")
        return fails

    assert old_check(lc.lbs_f32(case, links=links)) == []
    report = {}
    for plant in lc.PLANTS:
        fails = old_check(lc.lbs_f32(case, links=links, plant=plant))
        report[plant] = "passes the old check" if not fails else "refused: " + ", ".join(fails)
    print("lbs_cases old_check " + json.dumps(report))


# ------------------------------------------------------------------------------------------------------------------------ workspace layout
def test_workspace_layout_is_the_one_the_gpu_test_reads():
    src = _code("lbs.hip")
    for line in ("float* v_shaped = ws;", "float* vraw = v_shaped + (size_t)B * nv3;", "float* J = vraw + (size_t)B * nv3;",
                 "float* pf = J + (size_t)B * nj * 3;", "float* A = pf + (size_t)B * npf;", "const int nv3 = nv * 3, npf = (nj - 1) * 9;",
                 "return (size_t)B * nv * 3 * 2 + (size_t)B * nj * 3 + (size_t)B * (nj - 1) * 9 + (size_t)B * nj * 12 + 64;",
                 "float* skin_out = (links && nlinks > 0) ? vraw : verts;", "float* v_posed = (links && nlinks > 0) ? verts : vraw;",
                 "#define LWG_MAX_JOINTS 64", "#define LWG_LBS_FB %d" % lc.FB, "B > 65535"):
        assert line in src, line
    # each buffer is written by the kernel the stage names: shape -> v_shaped, joints -> J, pose -> (pf, A, j3d, j2d), posed -> v_posed
    assert re.search(r"lwg_lbs_shape_kernel,[^;]*nv3, v_shaped\);", src) and re.search(r"lwg_lbs_joints_kernel,[^;]*nv, nj, J\);", src)
    assert re.search(r"lwg_lbs_pose_kernel,[^;]*parents, nj, pf, A,\s*j3d, j2d\);", src)
    assert re.search(r"lwg_lbs_posed_kernel,[^;]*v_shaped, posedirs, pf, npf, nv3, B, v_posed\);", src)
    assert re.search(r"lwg_lbs_blend_kernel,[^;]*v_posed, lbs_weights, A, nj, nv, skin_out\);", src)
    for B, nv, nj in ((1, 1, 2), (17, 257, 64), (9, 63, 24)):
        parts = lc.ws_split(torch.zeros(lc.ws_floats(B, nv, nj)), B, nv, nj)
        assert list(parts) == ["v_shaped", "vraw", "J", "pose_feature", "A"]
        assert sum(p.numel() for p in parts.values()) + 64 == lc.ws_floats(B, nv, nj)
        assert parts["A"].shape == (B, nj, 12) and parts["pose_feature"].shape == (B, 9 * (nj - 1))


# ------------------------------------------------------------------------------------------------------------- host glue of bodynets.py
def _body_and_case(monkeypatch, B):
    emu_ops.install(monkeypatch)
    mi = lc.MODELS.index(("rand", 52, 63))
    case = lc.make_case(mi, B, "none")
    return SMPLH(lc.model_pickle_dict(case["model"])), case


def test_offsets_rows_through_the_emulated_abi(monkeypatch):
    """(1, nv, 3): the dataset's collated table, shared by every frame.  (bs, nv, 3) with B = bs ns skinned rows: row i serves frames
    i ns .. (i + 1) ns - 1, which is what the reference's broadcast (bs, 1, nv, 3) + (bs, ns, nv, 3) does - stated with the oracle sample by sample."""
    body, case = _body_and_case(monkeypatch, 8)
    nv = 63
    om = orc.SMPLHModel(lc.model_pickle_dict(case["model"]))
    theta = lc.theta_buffer(case)
    off1 = torch.from_numpy((0.05 * lc._rng(7).standard_normal((1, nv, 3))).astype(np.float32))
    got = body.get_details(theta, offsets=off1)
    want = orc.smplh_get_details(om, theta, off1[0])
    assert torch.equal(got["verts"], want["verts"]) and torch.equal(got["j2d"], want["j2d"]) and torch.equal(got["j3d"], want["j3d"])
    assert SMPLH._offsets_rows(off1, 8, "cpu").shape == (nv, 3) and SMPLH._offsets_rows(0, 8, "cpu") is None
    bs, ns = 4, 2
    offb = torch.from_numpy((0.05 * lc._rng(8).standard_normal((bs, nv, 3))).astype(np.float32))
    rows = SMPLH._offsets_rows(offb, bs * ns, "cpu")
    assert rows.shape == (bs * ns, nv, 3) and all(torch.equal(rows[b], offb[b // ns]) for b in range(bs * ns))
    got = body.get_details(theta, offsets=offb)
    broadcast = (torch.zeros(bs, ns, nv, 3) + offb[:, None]).reshape(bs * ns, nv, 3)            # (bs, 1, nv, 3) against (bs, ns, nv, 3)
    want = orc.smplh_get_details(om, theta, broadcast)
    assert torch.equal(got["verts"], want["verts"]) and torch.equal(got["j3d"], want["j3d"])
    for i in range(bs):                                                               # and sample by sample (another batch: BLAS may sum otherwise)
        alone = orc.smplh_get_details(om, theta[i * ns:(i + 1) * ns], offb[i])["verts"]
        assert (got["verts"][i * ns:(i + 1) * ns] - alone).abs().max() <= 1e-5
    assert not torch.equal(got["verts"], body.get_details(theta, offsets=offb[0:1])["verts"])
    with pytest.raises(ValueError):
        SMPLH._offsets_rows(offb[:3], 8, "cpu")


def test_links_2d_forms_through_the_emulated_abi(monkeypatch):
    """(n, 2); (n, 3) with flags - a 2-D table is applied whole, flags or not (base_smpl.py:44-45); an expanded identical (B, n, 3), reduced to its
    flagged rows; a genuinely per-sample (B, n, 3), skinned row by row.  Each against orc.link on the un-linked vertices."""
    B = 8
    body, case = _body_and_case(monkeypatch, B)
    theta = lc.theta_buffer(case)
    raw = body.get_details(theta)["verts"]
    pairs = lc.link_pairs(63).long()
    n = pairs.shape[0]
    got = body.get_details(theta, links_ids=pairs)["verts"]
    assert torch.equal(got, orc.link(raw, pairs)) and not torch.equal(got, raw)
    flags = torch.tensor([1, 0] * n)[:n]
    l3 = torch.cat([pairs, flags[:, None]], dim=1)
    assert torch.equal(body.get_details(theta, links_ids=l3)["verts"], orc.link(raw, l3))
    assert torch.equal(orc.link(raw, l3), orc.link(raw, pairs))                       # 2-D: every row applied
    expanded = l3[None].expand(B, n, 3)
    assert body._links_2d(expanded, "cpu").shape == (int(flags.sum()), 2)
    got = body.get_details(theta, links_ids=expanded)["verts"]
    assert torch.equal(got, orc.link(raw, expanded)) and not torch.equal(got, orc.link(raw, pairs))
    per = expanded.clone()
    per[1::2, :, 2] = 1 - per[1::2, :, 2]                                             # odd frames flag the other half
    assert body._links_2d(per, "cpu") is None
    got = body.get_details(theta, links_ids=per)
    rows = torch.cat([body.get_details(theta[b:b + 1])["verts"] for b in range(B)])   # the emulation's BLAS sums a 1-row batch in another order
    assert (rows - raw).abs().max() <= 1e-5
    assert torch.equal(got["verts"], orc.link(rows, per)) and torch.equal(body.link(raw, per), orc.link(raw, per))
    assert not torch.equal(orc.link(rows, per), orc.link(rows, expanded)) and got["j2d"].shape == (B, 52, 2)
    # column 0 is the destination, column 1 the source
    one = torch.tensor([[5, 9]])
    got = body.get_details(theta, links_ids=one)["verts"]
    assert torch.equal(got[:, 5], raw[:, 9]) and torch.equal(got[:, 9], raw[:, 9])
