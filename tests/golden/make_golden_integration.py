#!/usr/bin/env python3
"""Generate tests/golden/golden_integration_v1.npz from the REFERENCE's own code (its checkout named by LWG_REFERENCE), for
tests/test_reference_integration.py.  The C ABI is emulated on CPU tensors (tests/emu_ops.py), as in that test.

Level 2 - ``sys.modules["neural_renderer"] = ipercore_amd.nr``, then the reference's unmodified ``SMPLRenderer``
(iPERCore/tools/human_digitalizer/renders/nmr.py) runs on it: its outputs for the seeded inputs are recorded (exact arrays as sha256
digests, the ones compared with a tolerance as arrays or a seeded sample of them).
Level 1 - the reference's unmodified runner function ``call_imitator_inference`` (iPERCore/services/run_imitator.py) drives
``ipercore_amd.imitator.Imitator``: every call it makes to ``Imitator.inference`` (arguments, SMPL rows) and the result it returns
(output file names per frame, reference image paths) are recorded.

    LWG_REFERENCE=<reference checkout> python tests/golden/make_golden_integration.py
"""
import hashlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("LWG_REFERENCE", "")
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import emu_ops  # noqa: E402
from tests import parity_utils as pu  # noqa: E402

S = 64
OUT = os.path.join(ROOT, "tests", "golden", "golden_integration_v1.npz")
TEX_SAMPLE = 20000          # seeded sample of the textured renderer's (2, F, 3, 3, 3, 3) texture tensor (the whole of it: by sha256)


def sha(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


class _Stub(types.ModuleType):
    """An absent third-party module the reference imports at module scope but never calls on these paths."""

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        m = _Stub(self.__name__ + "." + k)
        setattr(self, k, m)
        return m

    def __call__(self, *a, **k):
        return None


class _Patch:
    def setattr(self, obj, name, value, raising=True):
        setattr(obj, name, value)


def install():
    import ipercore_amd.nr as our_nr
    emu_ops.install(_Patch())
    np.int, np.float = int, float               # removed in NumPy >= 1.24, used by the reference's mesh.py
    for name in ("cv2", "toml", "torchvision", "torchvision.transforms", "torchvision.transforms.functional", "tensorboardX"):
        sys.modules.setdefault(name, _Stub(name))
    sys.modules["neural_renderer"] = our_nr
    sys.path.insert(0, REF)
    return our_nr


def level2(our_nr):
    import iPERCore.tools.human_digitalizer.renders.nmr as ref_nmr
    from ipercore_amd import synthetic
    from iPERCore.tools.human_digitalizer.renders.nmr import SMPLRenderer
    from tests.test_oracle_golden import _details72
    assert ref_nmr.nr is our_nr, "the reference's `import neural_renderer as nr` did not bind ipercore_amd.nr"
    cfgdir = os.path.join(REF, "assets/configs/pose3d")
    tmp = synthetic.tmp_asset_dir()
    ref = SMPLRenderer(face_path=synthetic.write_smpl_faces_npy(os.path.join(tmp, "smpl_faces.npy")),
                       fim_enc_path=os.path.join(cfgdir, "mapper_fim_enc.txt"), uv_map_path=os.path.join(cfgdir, "mapper_uv.txt"),
                       part_path=os.path.join(cfgdir, "smpl_part_info.json"), front_path=os.path.join(cfgdir, "front_body.json"),
                       head_path=os.path.join(cfgdir, "head.json"), facial_path=os.path.join(cfgdir, "front_facial.json"),
                       map_name="uv_seg", tex_size=3, image_size=S, fill_back=False, anti_aliasing=True,
                       background_color=(0, 0, 0), has_front=True, top_k=3)
    d = _details72()
    cam, verts = d["cam"][0:2].clone(), d["verts"][0:2].clone()
    g = {}
    for smpl_faces in (True, False):
        f2pts, fim, wim = ref.render_fim_wim(cam, verts, smpl_faces=smpl_faces)
        for k, v in (("f2pts", f2pts), ("fim", fim), ("wim", wim)):
            g[f"l2/render_fim_wim/{int(smpl_faces)}/{k}_sha"] = sha(v)
    g["l2/render_fim_sha"] = sha(ref.render_fim(cam, verts, smpl_faces=True))
    uf, uw = ref.render_uv_fim_wim(2)
    g["l2/uv_fim_sha"], g["l2/uv_wim_sha"] = sha(uf), sha(uw)
    f2pts, fim, wim = ref.render_fim_wim(cam, verts, smpl_faces=True)
    enc, _ = ref.encode_fim(fim=fim, transpose=True)
    g["l2/encode_fim_sha"] = sha(enc)
    g["l2/T_src"] = ref.cal_bc_transform(f2pts.flip(0).contiguous(), fim, wim).numpy()
    g["l2/T_uv"] = ref.cal_bc_transform(ref.get_f_uvs2img(2), fim, wim).numpy()
    g["l2/vis_f2pts_sha"] = sha(ref.get_vis_f2pts(f2pts, fim))
    uv_img = torch.tensor(synthetic.uniform_image((2, 3, S, S), 11, "integration/uv_img"))
    ref.set_ambient_light()
    img, tex = ref.forward(cam, verts, uv_img, dynamic=True)
    g["l2/img"] = img.numpy()
    g["l2/tex_shape"] = np.array(tex.shape)
    g["l2/tex_sha"] = sha(tex)
    tex = tex.reshape(-1).numpy()
    g["l2/tex_index"] = np.sort(np.random.RandomState(0).choice(tex.size, TEX_SAMPLE, replace=False))
    g["l2/tex_sample"] = tex[g["l2/tex_index"]]
    return g


class _Meta:
    def __init__(self, out_img_dir, view, bt):
        self.out_img_dir, self.effect_info, self.pose_fc, self.cam_fc = out_img_dir, {"View": view, "BT": bt}, 300, 100


def level1(tmp):
    from iPERCore.services import run_imitator as ref_runner
    case = pu.build_case(image_size=S, num_filters=[64, 64, 128], n_res=2, bg_filters=[64, 64, 128], n_frames=4, ns=2)
    im = pu.make_imitator(case, frame_batch=3, device="cpu")
    opt = pu.AttrDict(cam_strategy="smooth")
    ref_paths = [f"frame_{i:08d}.png" for i in range(4)]
    calls = []
    inference = im.inference

    def recording(**kw):
        calls.append({k: v for k, v in kw.items() if k not in ("output_dir", "visualizer")})
        return inference(**kw)
    im.inference = recording
    g = {}
    for tag, view, bt in (("plain", [], [(1, 2)]), ("views", [0, 90], [])):
        im.first_cam = None
        del calls[:]
        res = ref_runner.call_imitator_inference(opt, im, _Meta(os.path.join(tmp, tag), view, bt), ref_paths, case.tgt_smpls.copy(),
                                                 visualizer=None)
        g[f"l1/{tag}/ref_imgs_paths"] = np.array(res["ref_imgs_paths"])
        g[f"l1/{tag}/outputs"] = np.array([[os.path.basename(p) for p in o] for o in res["outputs"]])
        g[f"l1/{tag}/n_calls"] = np.array(len(calls))
        for i, kw in enumerate(calls):
            g[f"l1/{tag}/call{i}/tgt_smpls"] = np.asarray(kw.pop("tgt_smpls"))
            for k, v in kw.items():
                g[f"l1/{tag}/call{i}/{k}"] = np.array(v)
    return g


def main():
    import tempfile
    assert os.path.isdir(os.path.join(REF, "iPERCore")), "LWG_REFERENCE must name the reference checkout"
    our_nr = install()
    g = level2(our_nr)
    with tempfile.TemporaryDirectory() as tmp:
        g.update(level1(tmp))
    g = {k: (np.array(v) if isinstance(v, str) else v) for k, v in g.items()}
    np.savez_compressed(OUT, **g)
    print(OUT, os.path.getsize(OUT), "bytes,", len(g), "arrays")


if __name__ == "__main__":
    main()
