"""INTEGRATION.md's levels against what the reference's own code produced on this package, recorded in
tests/golden/golden_integration_v1.npz by tests/golden/make_golden_integration.py (run where the reference checkout is importable).
The C ABI is emulated on CPU tensors (tests/emu_ops.py), as it was when the record was made, so what is exercised here is the BINDING:
names, argument conventions and return types the reference's callers rely on.

Level 2 - with ``sys.modules["neural_renderer"] = ipercore_amd.nr`` the reference's unmodified ``SMPLRenderer``
(iPERCore/tools/human_digitalizer/renders/nmr.py:128-225, 243-296, 298-358, 390-401, 639-681, 713-757) ran on our module; its outputs
must equal those of ``ipercore_amd.renders.SMPLRenderer`` on the same inputs (exact maps by sha256, the rest within the old bounds).
Level 1 - the reference's unmodified runner function ``call_imitator_inference`` (iPERCore/services/run_imitator.py:19-84, with
``base_runner.add_bullet_time_effect / add_special_effect / add_hands_params_to_smpl`` :33-151) drove ``ipercore_amd.imitator.Imitator``:
its calls to ``Imitator.inference`` are replayed here, and the file names, frame count and the frames themselves are checked against
what the runner returned and against the oracle.
"""
import os

import numpy as np
import pytest
import torch

from tests import emu_ops
from tests import parity_utils as pu
from tests.golden.make_golden_integration import S, sha

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_integration_v1.npz")


@pytest.fixture(scope="module")
def recorded():
    return np.load(GOLDEN, allow_pickle=False)


def test_level2_reference_smplrenderer_on_our_neural_renderer(recorded, monkeypatch):
    from ipercore_amd import synthetic
    from ipercore_amd.renders import SMPLRenderer
    from tests.test_oracle_golden import _details72
    g = recorded
    emu_ops.install(monkeypatch)
    ours = SMPLRenderer(image_size=S, has_front=True, top_k=3)
    d = _details72()
    cam, verts = d["cam"][0:2].clone(), d["verts"][0:2].clone()
    # nmr.py:319-342 (look_at + vertices_to_faces + rasterize_face_index_map_and_weight_map of OUR module inside THEIR wrapper)
    for smpl_faces in (True, False):
        of, ofim, owim = ours.render_fim_wim(cam, verts, smpl_faces=smpl_faces)
        assert ofim.dtype == torch.int32 and owim.shape == (2, S, S, 3)
        key = f"l2/render_fim_wim/{int(smpl_faces)}"
        assert sha(of) == g[f"{key}/f2pts_sha"] and sha(ofim) == g[f"{key}/fim_sha"] and sha(owim) == g[f"{key}/wim_sha"]
        assert int((ofim >= 0).sum()) > 100
    assert sha(ours.render_fim(cam, verts, smpl_faces=True)) == g["l2/render_fim_sha"]
    # nmr.py:344-358 UV atlas
    ouf, ouw = ours.render_uv_fim_wim(2)
    assert sha(ouf) == g["l2/uv_fim_sha"] and sha(ouw) == g["l2/uv_wim_sha"]
    # consumers of the maps: their torch code on their maps vs our kernels' contract on ours (the maps themselves are equal, above)
    f2pts, fim, wim = ours.render_fim_wim(cam, verts, smpl_faces=True)
    enc_o, _ = ours.encode_fim(fim=fim, transpose=True)
    assert sha(enc_o) == g["l2/encode_fim_sha"]
    T_o = ours.cal_bc_transform(f2pts.flip(0).contiguous(), fim, wim)
    assert np.abs(T_o.numpy() - g["l2/T_src"]).max() <= 1e-6 and bool((T_o == -2).any()) and bool((g["l2/T_src"] == -2).any())
    Tuv_o = ours.cal_bc_transform(ours.get_f_uvs2img(2), fim, wim)
    assert np.abs(Tuv_o.numpy() - g["l2/T_uv"]).max() <= 1e-6
    assert sha(ours.get_vis_f2pts(f2pts, fim)) == g["l2/vis_f2pts_sha"]
    # the textured renderer's calls (nr.lighting / nr.rasterize, nmr.py:243-296): signature-compatible and the same image through either
    # wrapper (the values themselves are parity-unpinned: the package is not vendored); the texture is recorded as a seeded sample (within
    # the old bound, which locates a difference) and as the sha256 of the whole tensor
    uv_img = torch.tensor(synthetic.uniform_image((2, 3, S, S), 11, "integration/uv_img"))
    ours.set_ambient_light()
    img_o, tex_o = ours.forward(cam, verts, uv_img, dynamic=True)
    assert img_o.shape == (2, 3, S, S) and torch.isfinite(img_o).all()
    assert tuple(tex_o.shape) == tuple(g["l2/tex_shape"])
    assert np.abs(tex_o.reshape(-1).numpy()[g["l2/tex_index"]] - g["l2/tex_sample"]).max() <= 1e-5
    assert sha(tex_o) == g["l2/tex_sha"]
    assert np.abs(img_o.numpy() - g["l2/img"]).max() <= 1e-4


def _frames_of(paths):
    from PIL import Image
    return np.stack([np.asarray(Image.open(p))[:, :, ::-1] for p in paths])          # PNGs hold BGR (cv2.imwrite of the reference)


def _replay(im, g, tag, out_dir):
    """The runner's calls to Imitator.inference, in its order, with its arguments -> the outputs zipped per frame, as it returns them."""
    outs = []
    for i in range(int(g[f"l1/{tag}/n_calls"])):
        kw = {k: g[f"l1/{tag}/call{i}/{k}"].item() for k in ("cam_strategy", "prefix", "verbose", "use_selected_f2pts")}
        outs.append(im.inference(tgt_smpls=g[f"l1/{tag}/call{i}/tgt_smpls"], output_dir=out_dir, visualizer=None, **kw))
    return list(zip(*outs))


def _oracle_u8(smpls):
    from oracle import lwg_oracle as orc
    case = pu.build_case(image_size=S, num_filters=[64, 64, 128], n_res=2, bg_filters=[64, 64, 128], n_frames=4, ns=2)
    case.tgt_smpls = smpls.astype(np.float32)
    return np.stack([orc.to_uint8_bgr(w.numpy()) for w in pu.run_oracle(case)])


def test_level1_reference_runner_drives_our_imitator(recorded, monkeypatch, tmp_path):
    from ipercore_amd.imitator import add_hands_params_to_smpl
    g = recorded
    emu_ops.install(monkeypatch)
    case = pu.build_case(image_size=S, num_filters=[64, 64, 128], n_res=2, bg_filters=[64, 64, 128], n_frames=4, ns=2)
    im = pu.make_imitator(case, frame_batch=3, device="cpu")
    ref_paths = [f"frame_{i:08d}.png" for i in range(4)]
    hands = im.body_rec.np_hands_mean

    # (a) no multi-view: bullet-time effect at frame 1 (2 novel-view frames inserted), hands appended -> (6,169) rows (cam 3 + pose 156 + shape 10), prefix "pred_"
    smpls = g["l1/plain/call0/tgt_smpls"]
    assert int(g["l1/plain/n_calls"]) == 1 and smpls.shape == (6, 3 + 156 + 10)
    assert list(g["l1/plain/ref_imgs_paths"]) == ref_paths[:2] + [ref_paths[1]] * 2 + ref_paths[2:]
    # our restatement of add_hands_params_to_smpl forms the runner's rows: [cam, body pose[:66], hands, shape]
    rows85 = np.concatenate([smpls[:, :69], np.zeros((6, 6), smpls.dtype), smpls[:, -10:]], axis=1)
    assert np.array_equal(add_hands_params_to_smpl(rows85, hands), smpls)
    res = _replay(im, g, "plain", str(tmp_path / "plain"))
    outs = [o[0] for o in res]
    assert [[os.path.basename(p) for p in o] for o in res] == g["l1/plain/outputs"].tolist()
    assert [os.path.basename(p) for p in outs] == [f"pred_{t:0>8}.png" for t in range(6)]          # imitator.py:369
    want_u8, got_u8 = _oracle_u8(smpls), _frames_of(outs)
    assert np.abs(got_u8.astype(int) - want_u8.astype(int)).max() <= 1 and (got_u8 != want_u8).mean() < 1e-3

    # (b) multi-view outputs (run_imitator.py:62-75): one inference per view, prefix "pred_{i}_{view}_", outputs zipped per frame
    im.first_cam = None
    assert int(g["l1/views/n_calls"]) == 2 and list(g["l1/views/ref_imgs_paths"]) == ref_paths
    res = _replay(im, g, "views", str(tmp_path / "views"))
    assert len(res) == 4 and all(len(o) == 2 for o in res)
    assert [[os.path.basename(p) for p in o] for o in res] == g["l1/views/outputs"].tolist()
    assert os.path.basename(res[2][1]) == "pred_1_90_00000002.png"
    # the reference's add_view_effect rotates ref_smpls IN PLACE (base_runner.py:72-75): view 1 acted on the rows view 0 returned
    want_u8, got_u8 = _oracle_u8(g["l1/views/call1/tgt_smpls"]), _frames_of([o[1] for o in res])
    assert np.abs(got_u8.astype(int) - want_u8.astype(int)).max() <= 1 and (got_u8 != want_u8).mean() < 1e-3
