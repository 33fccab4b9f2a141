"""The SMPL skinning kernels (csrc/lbs.hip) stage by stage on the bodies, poses and batches of tests/lbs_cases.py: lwg_smpl_lbs_f32 is called
through the C ABI with a workspace the test owns, the five intermediates (v_shaped, J, pose_feature, v_posed, A) are read back from it and every
stage is held against its float64 evaluation and its rounding-count bound; the end results against float64 from the inputs with the propagated
bounds.  References, bounds and their derivations live in tests/lbs_cases.py; tests/test_lbs_cases_cpu.py shows on the CPU that every bound holds
for an fp32 restatement of the kernels and refuses the planted errors.  The argument forms of the ABI (links, strided views into a theta buffer,
no camera) and the independence of a frame from its batch are bitwise comparisons.  Every buffer the library writes starts NaN-filled: an element
nobody wrote shows up.  Every test prints its metrics - for the toleranced comparisons the worst |error| / bound per stage - as one JSON line."""
import functools
import json

import pytest
import torch

from ipercore_amd import _lib, ops, synthetic
from tests import lbs_cases as lc
from tests.gpu_checks import DEV, _smplh_dev

pytestmark = pytest.mark.gpu

INVALID_VALUE = 1                      # hipErrorInvalidValue
MODEL_KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "parents", "lbs_weights")


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _report(what, metrics):
    print("lbs_kernels " + json.dumps({what: metrics}))


@functools.lru_cache(maxsize=None)
def _dev_model(kind, nj, nv):
    m = lc.make_model(kind, nj, nv)
    return {k: m[k].to(DEV).contiguous() for k in MODEL_KEYS}


def _call(md, pose, beta, cam, offsets=None, links=None, strided=False, want_j2d=True, check=True, override=None, B=None):
    """One lwg_smpl_lbs_f32 call on device tensors into NaN-filled outputs and a NaN-filled workspace.  ``strided``: pose and cam travel as views
    into one (B, 3 + 3 nj + 10) buffer.  ``override``: ABI arguments replaced by name (the contract test).
    -> (hipError_t, dict of device tensors: verts, j3d, j2d, ws)."""
    L = _lib.lib()
    nv, nj = md["lbs_weights"].shape
    B = pose.shape[0] if B is None else B
    nbeta = beta.shape[1]
    n_ws = L.lwg_smpl_lbs_ws_floats(B, nv, nj)
    assert n_ws == lc.ws_floats(B, nv, nj)
    out = {"verts": _nan(B, nv, 3), "j3d": _nan(B, nj, 3), "j2d": _nan(B, nj, 2), "ws": _nan(n_ws)}
    keep = []
    if strided:
        theta = torch.cat([cam, pose, beta], dim=1).contiguous()
        keep.append(theta)
        pose_ptr, cam_ptr, pose_stride, cam_stride = theta.data_ptr() + 3 * 4, theta.data_ptr(), theta.shape[1], theta.shape[1]
    else:
        pose_ptr, pose_stride = pose.data_ptr(), pose.shape[1]
        cam_ptr, cam_stride = (None, 0) if cam is None else (cam.data_ptr(), cam.shape[1])
    a = {"pose": pose_ptr, "pose_stride": pose_stride, "beta": beta.data_ptr(), "beta_stride": nbeta, "nbeta": nbeta, "cam": cam_ptr,
         "cam_stride": cam_stride, "v_template": md["v_template"].data_ptr(), "offsets": None if offsets is None else offsets.data_ptr(),
         "off_batched": 1 if offsets is not None and offsets.dim() == 3 else 0, "shapedirs": md["shapedirs"].data_ptr(),
         "posedirs": md["posedirs"].data_ptr(), "J_regressor": md["J_regressor"].data_ptr(), "parents": md["parents"].data_ptr(),
         "lbs_weights": md["lbs_weights"].data_ptr(), "links": None if links is None else links.data_ptr(),
         "nlinks": 0 if links is None else links.shape[0], "B": B, "nv": nv, "nj": nj, "verts": out["verts"].data_ptr(), "j3d": out["j3d"].data_ptr(),
         "j2d": out["j2d"].data_ptr() if want_j2d else None, "ws": out["ws"].data_ptr()}
    a.update(override or {})
    err = L.lwg_smpl_lbs_f32(*a.values(), ops._stream())
    torch.cuda.synchronize()
    if check:
        _lib.check(err, "lwg_smpl_lbs_f32")
    return err, out


def _skin(case, links=None, strided=False, camera=True):
    """A case of lbs_cases through the library -> dict of CPU tensors: verts, j3d, j2d and the workspace's five parts (ws_split's names)."""
    md = _dev_model(*[m for m in lc.MODELS if lc.make_model(*m) is case["model"]][0])
    nv, nj = md["lbs_weights"].shape
    dev = lambda t: None if t is None else t.to(DEV).contiguous()                       # noqa: E731
    _, out = _call(md, dev(case["pose"]), dev(case["beta"]), dev(case["cam"]) if camera else None, dev(case["offsets"]), dev(links), strided=strided,
                   want_j2d=camera)
    got = {k: out[k].cpu() for k in ("verts", "j3d", "j2d")}
    got.update(lc.ws_split(out["ws"].cpu(), case["pose"].shape[0], nv, nj))
    return got


def _stage_inputs(got):
    """The un-linked call's results under the names stage_ratios reads (vraw holds v_posed when no links are given)."""
    return {"verts": got["verts"], "j3d": got["j3d"], "j2d": got["j2d"], "v_shaped": got["v_shaped"], "J": got["J"], "pose_feature": got["pose_feature"],
            "v_posed": got["vraw"], "A": got["A"]}


def _same_bits(a, b):
    return torch.equal(lc.bits(a), lc.bits(b))


WRITTEN = ("verts", "j3d", "j2d", "v_shaped", "vraw", "J", "pose_feature", "A")


# ---------------------------------------------------------------------------------------------------------------------- stage by stage
@pytest.mark.parametrize("mi", range(len(lc.MODELS)), ids=[lc.model_id(m) for m in lc.MODELS])
def test_every_stage_within_its_bound(mi):
    """Every case of the model (B in 1, 8, 9, 17; offsets absent, shared, batched; the ten pose kinds cycled over the frames), no links: the five
    intermediates from the workspace and the three outputs, each stage against its bound."""
    worst = {}
    for c in lc.CASES:
        if c[0] != mi:
            continue
        case = lc.make_case(*c)
        got = _skin(case)
        for k in WRITTEN:
            assert not torch.isnan(got[k]).any(), f"{case['id']}: {int(torch.isnan(got[k]).sum())} elements of {k} are NaN or were never written"
        r = lc.stage_ratios(case, _stage_inputs(got))
        assert set(r) == set(lc.STAGES)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
        bad = {k: v for k, v in r.items() if not v <= 1.0}
        assert not bad, f"{case['id']} (pose kinds {case['kinds']}): |error| / bound {bad}"
    _report(lc.model_id(lc.MODELS[mi]), {"worst_ratio": worst})


# ----------------------------------------------------------------------------------------------------------------------- argument forms
LINK_MODELS = [i for i, m in enumerate(lc.MODELS) if m[2] >= 8]


@pytest.mark.parametrize("mi", LINK_MODELS, ids=[lc.model_id(lc.MODELS[i]) for i in LINK_MODELS])
def test_links_are_exact_gathers_of_the_unlinked_vertices(mi):
    """Pairs that chain (the ``to`` of one is the ``from`` of another, in both orders): every linked row holds the bits of the UN-linked source
    row, every other row its own; the un-linked vertices stay readable in the workspace; joints do not change."""
    for B, off in ((9, "shared"), (1, "batched")):
        case = lc.make_case(mi, B, off)
        links = lc.link_pairs(lc.MODELS[mi][2])
        raw, linked = _skin(case), _skin(case, links=links)
        assert lc.link_faults(linked["verts"], raw["verts"], links) == [], case["id"]
        assert _same_bits(linked["vraw"], raw["verts"]), f"{case['id']}: the workspace's un-linked vertices differ from the un-linked call's"
        for k in ("j3d", "j2d", "v_shaped", "J", "pose_feature", "A"):
            assert _same_bits(linked[k], raw[k]), f"{case['id']}: {k} differs with links"
        assert not _same_bits(linked["verts"], raw["verts"])


def test_views_into_a_theta_buffer_equal_the_contiguous_call():
    """pose_stride = cam_stride = 3 + 3 nj + 10, pointers 3 floats and 0 floats into the buffer: every output and intermediate bit for bit."""
    for mi, B, off in ((0, 9, "batched"), (3, 17, "shared"), (6, 8, "none"), (8, 9, "none"), (7, 1, "shared")):
        case = lc.make_case(mi, B, off)
        a, b = _skin(case), _skin(case, strided=True)
        for k in WRITTEN:
            assert _same_bits(a[k], b[k]), f"{case['id']}: {k} differs between the strided and the contiguous form"


def test_without_a_camera_vertices_and_joints_are_the_same_bits():
    """cam = NULL with j2d = NULL: verts, j3d and the intermediates as with a camera.  cam = NULL with a j2d buffer: j2d is not written."""
    for mi, B, off in ((2, 9, "shared"), (9, 17, "batched"), (7, 8, "none")):
        case = lc.make_case(mi, B, off)
        a, b = _skin(case), _skin(case, camera=False)
        for k in WRITTEN:
            if k != "j2d":
                assert _same_bits(a[k], b[k]), f"{case['id']}: {k} differs without a camera"
        assert torch.isnan(b["j2d"]).all()
    md = _dev_model(*lc.MODELS[7])
    _, out = _call(md, case["pose"].to(DEV), case["beta"].to(DEV), None, None, want_j2d=True)
    assert torch.isnan(out["j2d"]).all() and _same_bits(out["verts"].cpu(), a["verts"])


# ------------------------------------------------------------------------------------------------------------------- batch independence
ALONE = (0, 7, 8, 16)


def test_a_frame_does_not_depend_on_its_batch():
    """B = 17 (groups of 8, 8 and 1 frames), a different pose, beta and offset table per frame: frames 0, 7, 8 and 16 skinned alone (slot 0 of a
    one-frame group) are the bits of their rows in the batch - the three outputs and the five intermediates.  lwg_lbs_posed_kernel's explicit
    fmaf is what holds this: left to contraction, the compiler packed some frame slots and fused others."""
    for mi in range(len(lc.MODELS)):
        case = lc.make_case(mi, 17, "batched")
        batch = _skin(case)
        for b in ALONE:
            alone = _skin(lc.frame_of(case, b))
            for k in WRITTEN:
                assert _same_bits(alone[k][0], batch[k][b]), f"{case['id']}: {k} of frame {b} skinned alone differs from its row in the batch"


def test_a_frame_does_not_depend_on_its_batch_at_full_size():
    """The same at the real size (the synthetic SMPL-H dict: nv = 6890, nj = 52, natural poses), where the packed-math difference once appeared."""
    body = _smplh_dev(synthetic.smplh_model_dict(seed=0))
    md = {k: v.contiguous() for k, v in body._device_model().items()}
    theta = torch.tensor(synthetic.smpl_sequence(17, seed=1, pose_dim=72), device=DEV)
    pose, beta, cam = body._full_pose(theta[:, 3:-10].contiguous()), theta[:, -10:].contiguous(), theta[:, 0:3].contiguous()
    nv, nj = md["lbs_weights"].shape
    assert (nv, nj) == (6890, 52)
    _, out = _call(md, pose, beta, cam)
    batch = dict({k: out[k] for k in ("verts", "j3d", "j2d")}, **lc.ws_split(out["ws"], 17, nv, nj))
    for k in WRITTEN:
        assert not torch.isnan(batch[k]).any(), k
    for b in ALONE:
        _, o1 = _call(md, pose[b:b + 1].contiguous(), beta[b:b + 1].contiguous(), cam[b:b + 1].contiguous())
        alone = dict({k: o1[k] for k in ("verts", "j3d", "j2d")}, **lc.ws_split(o1["ws"], 1, nv, nj))
        for k in WRITTEN:
            assert _same_bits(alone[k][0], batch[k][b]), f"synthetic SMPL-H: {k} of frame {b} skinned alone differs from its row in the batch"


# ----------------------------------------------------------------------------------------------------------------------------- contract
def _untouched(out):
    return all(bool(torch.isnan(out[k]).all()) for k in ("verts", "j3d", "j2d", "ws"))


def test_invalid_arguments_are_refused_before_anything_is_written():
    """nj of 1 and of 65, beta_stride != nbeta, each required pointer NULL, B <= 0 and B = 65536 (one past what grid.y takes; nv = 1): invalid-value,
    and the NaN-filled outputs and workspace keep every NaN.  The buffers are sized for the call as if it were valid."""
    md = _dev_model("rand", 24, 63)
    case = lc.make_case(lc.MODELS.index(("rand", 24, 63)), 8, "none")
    pose, beta, cam = (case[k].to(DEV) for k in ("pose", "beta", "cam"))
    err, out = _call(md, pose, beta, cam)
    assert err == 0 and not _untouched(out)
    bad = [{"nj": 1}, {"nj": 65}, {"beta_stride": 11}, {"B": 0}, {"B": -1}, {"nv": 0}]
    bad += [{k: None} for k in ("pose", "beta", "v_template", "shapedirs", "posedirs", "J_regressor", "parents", "lbs_weights", "verts", "j3d", "ws")]
    for o in bad:
        err, out = _call(md, pose, beta, cam, check=False, override=o)
        assert err == INVALID_VALUE, f"{o}: returned {err}"
        assert _untouched(out), f"{o}: something was written"
    B = 65536
    md1 = _dev_model("rand", 2, 1)
    err, out = _call(md1, torch.zeros(B, 6, device=DEV), torch.zeros(B, lc.NBETA, device=DEV), torch.ones(B, 3, device=DEV), check=False)
    assert err == INVALID_VALUE, f"B = 65536: returned {err}"
    assert _untouched(out), "B = 65536: something was written"
    err, out = _call(md1, torch.zeros(B - 1, 6, device=DEV), torch.zeros(B - 1, lc.NBETA, device=DEV), torch.ones(B - 1, 3, device=DEV))
    assert err == 0 and not torch.isnan(out["verts"]).any() and not torch.isnan(out["j2d"]).any()            # 65535 is the largest batch
    assert torch.equal(out["verts"][0], out["verts"][-1]) and torch.equal(out["j3d"][0], out["j3d"][-1])
