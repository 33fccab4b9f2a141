#!/usr/bin/env python3
"""Generate tests/golden/golden_morph_v1.npz: ``morph`` (erode / dilate) and ``soft_dilate`` of the REFERENCE's own
tools/utils/morphology/morph_ops.py, loaded from the reference checkout in the authoring container (the file needs only torch, so it is
loaded by path: the package around it imports cv2), on small seeded NON-SQUARE masks that touch the image border.

    python tests/golden/make_golden_morph.py

Stored: the masks as uint8 numerators k of k/8 (binary masks are 0 / 8), the kernel sizes, and per mode one uint8 array
(n_masks, n_ks, H, W).  Every sum is a multiple of 1/8 far below 2^24, so the results do not depend on the summation order of the
host's conv2d."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("LWG_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)

import torch  # noqa: E402

H, W = 40, 56
KS = (1, 3, 5, 13, 21, 51)           # 51 is larger than the image
NAMES = ("disc_corner", "noise50", "sparse2", "dense98", "zeros", "ones", "eighths")


def masks_eighths(H=H, W=W, seed=41):
    """(7, H, W) uint8 numerators of k/8: a disc cut by the corner, 50 % noise, 2 % and 98 % density, all 0, all 1, random k/8."""
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    disc = ((yy - 4) ** 2 + (xx - (W - 7)) ** 2 <= 15 ** 2)
    u = r.uniform(size=(3, H, W))
    m = [disc, u[0] < 0.5, u[1] < 0.02, u[2] < 0.98, np.zeros((H, W), bool), np.ones((H, W), bool)]
    return np.stack([a.astype(np.uint8) * 8 for a in m] + [r.randint(0, 9, size=(H, W)).astype(np.uint8)])


def main():
    spec = importlib.util.spec_from_file_location("ref_morph_ops", os.path.join(REF, "iPERCore/tools/utils/morphology/morph_ops.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    m8 = masks_eighths()
    x = torch.tensor(m8.astype(np.float32) / 8.0).unsqueeze(1)
    out = {"masks8": m8, "ks": np.array(KS, dtype=np.int32), "names": np.array(NAMES)}
    with torch.no_grad():
        for mode, fn in (("erode", lambda t, k: ref.morph(t, k, mode="erode")), ("dilate", lambda t, k: ref.morph(t, k, mode="dilate")),
                         ("soft_dilate", lambda t, k: ref.soft_dilate(t, k))):
            out[mode] = np.stack([fn(x, k)[:, 0].numpy().astype(np.uint8) for k in KS], axis=1)
            assert set(np.unique(out[mode])) <= {0, 1}
    dst = os.path.join(HERE, "golden_morph_v1.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes;", {k: v.shape for k, v in out.items()})
    print({mode: out[mode].reshape(len(NAMES), len(KS), -1).mean(-1).round(2).tolist() for mode in ("erode", "dilate", "soft_dilate")})


if __name__ == "__main__":
    main()
