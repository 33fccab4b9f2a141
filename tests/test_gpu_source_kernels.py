"""The once-per-source image kernels of csrc/source.hip called directly, on small NON-SQUARE inputs that touch the image border: morph (erode /
dilate / soft dilate), Canny, the boundary fill, grid_sample, the UV merges and the input packing - each against the oracle (pinned to the
reference by tests/golden/golden_morph_v1.npz and golden_source_v1.npz where a fixture exists) or a plain fp64 restatement of its formula."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ipercore_amd import morphology, ops
from tests.gpu_checks import DEV, _cmp
from tests.test_oracle_golden import golden_morph

pytestmark = pytest.mark.gpu

H, W = 72, 96
KS = (1, 3, 5, 13, 21, 51)


def _rs(seed):
    return np.random.RandomState(seed)


def _t(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32))


def _disc(h, w, cy, cx, r):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.float32)


def _rot_rect(h, w, cy, cx, a, b, deg):
    yy, xx = np.mgrid[0:h, 0:w]
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    u, v = (xx - cx) * c + (yy - cy) * s, -(xx - cx) * s + (yy - cy) * c
    return ((np.abs(u) <= a) & (np.abs(v) <= b)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ morph
@functools.lru_cache(maxsize=None)
def _morph_masks():
    """(2, 3, 1, H, W): two batches of three DIFFERENT masks - disc cut by the corner / 50 % noise / values k/8, then 2 % / 98 % / all ones."""
    r = _rs(11)
    a = np.stack([_disc(H, W, 6, W - 9, 30), (r.uniform(size=(H, W)) < 0.5), r.randint(0, 9, size=(H, W)) / 8.0])
    b = np.stack([(r.uniform(size=(H, W)) < 0.02), (r.uniform(size=(H, W)) < 0.98), np.ones((H, W))])
    return _t(np.stack([a, b])[:, :, None])


@pytest.mark.parametrize("ks", KS)
def test_morph_equals_reference_fixture_and_oracle(ks):
    """Exact: the sums are integers or multiples of 1/8 far below 2^24, so no summation order can change a threshold decision.  ks = 51 is
    larger than both images; masks touch the border (pad value 1 for erode, 0 for the dilations); H != W."""
    from oracle import lwg_oracle as orc
    masks, ks_list, want = golden_morph()                     # the reference's own morph / soft_dilate on (7,1,40,56)
    j = ks_list.index(ks)
    md = masks.to(DEV)
    got = {"erode": morphology.morph(md, ks, mode="erode"), "dilate": morphology.morph(md, ks, mode="dilate"), "soft_dilate": morphology.soft_dilate(md, ks)}
    for mode, g in got.items():
        assert tuple(g.shape) == (7, 1, 40, 56)
        assert np.array_equal(g[:, 0].cpu().numpy().astype(np.uint8), want[mode][:, j]), f"{mode} ks={ks} differs from the reference's"
        assert torch.equal(g[2:5], ops.morph(md[2:5].contiguous(), ks, mode)), f"{mode} ks={ks}: an image depends on its batch"
    for batch in _morph_masks():                              # n = 3 different masks of (72, 96), not in the fixture
        for mode in ("erode", "dilate", "soft_dilate"):
            w = orc.soft_dilate(batch, ks) if mode == "soft_dilate" else orc.morph(batch, ks, mode)
            g = ops.morph(batch.to(DEV), ks, mode).cpu()
            assert torch.equal(g, w), f"{mode} ks={ks}: {int((g != w).sum())} pixels differ from the oracle's"


# ------------------------------------------------------------------------------------------------------------------ Canny
def _canny_inputs():
    """(8, 1, H, W): disc, disc cut by the border, rotated rectangle, one-pixel line, diagonal band, full, empty, 50 % noise."""
    yy, xx = np.mgrid[0:H, 0:W]
    line = np.zeros((H, W), dtype=np.float32)
    line[H // 3, 5:W - 9] = 1
    band = (np.abs((xx - yy) - 10) <= 6).astype(np.float32)
    return _t(np.stack([_disc(H, W, 34, 50, 22), _disc(H, W, 3, 4, 25), _rot_rect(H, W, 36, 44, 30, 12, 27), line, band,
                        np.ones((H, W)), np.zeros((H, W)), _rs(12).uniform(size=(H, W)) < 0.5])[:, None])


_CANNY_NAMES = ("disc", "disc_on_border", "rotated_rectangle", "line", "diagonal_band", "full", "empty", "noise50")


@pytest.mark.parametrize("pair", [0, 1, 2, 3])
def test_canny_equals_oracle(pair):
    """edge_mismatch == 0 (the bound of the source stage), n = 2 images of 72 x 96 per launch."""
    from oracle import lwg_oracle as orc
    x = _canny_inputs()[2 * pair:2 * pair + 2]
    want = orc.canny(x, 0.1, 0.9)
    got = morphology.CannyFilter()(x.to(DEV), 0.1, 0.9, True).cpu()
    for i in range(2):
        name = _CANNY_NAMES[2 * pair + i]
        bad = int((got[i] != want[i]).sum())
        print(name, "edges", int(want[i].sum()), "mismatch", bad)
        assert bad == 0, f"{name}: {bad} edge pixels differ from the oracle's ({int(want[i].sum())} edges)"
        if name not in ("empty", "line"):                      # (the reference's filter finds no edge on a one-pixel line; a full image has
            assert want[i].sum() > 0, name                     # edges along the zero-padded border)


# ------------------------------------------------------------------------------------------------------------------ boundary fill
@functools.lru_cache(maxsize=None)
def _fill_case():
    """A 50 % noise confidant mask of 72 x 96 (about 2200 Canny edges), its 5 x 5 dilation as the outer mask, a random source image, and the
    edge map trimmed by hand (row-major prefix) to exact counts on both sides of the kernel's 1024-point LDS chunk."""
    from oracle import lwg_oracle as orc
    r = _rs(15)
    conf = _t(r.uniform(size=(1, 1, H, W)) < 0.5)
    outpad = orc.morph(conf, 5, "dilate")
    src = _t(r.uniform(-1, 1, size=(1, 3, H, W)))
    full = orc.canny(conf, 0.1, 0.9)
    nfull = int(full.sum())
    assert nfull > 2048, nfull
    order = full.reshape(-1).nonzero()[:, 0]
    edges = {}
    for k in (0, 2, 3, 700, 1024, 1025, nfull):
        e = torch.zeros(H * W)
        e[order[:k]] = 1
        edges[k] = e.view(1, 1, H, W)
    return conf, outpad, src, edges, nfull


def _fill_want(src, conf, outpad, edges):
    from oracle import lwg_oracle as orc
    img, _, _ = orc.make_morph_image(src, conf, outpad, thin=edges)
    top3 = torch.full((src.shape[0], 3, H, W), -1, dtype=torch.int64)
    for i in range(src.shape[0]):
        u = (outpad * (1 - conf))[i, 0].nonzero(as_tuple=False)
        _, _, vals = orc.top_k_nearest(u, edges[i, 0].nonzero(as_tuple=False), 3)
        top3[i][:, u[:, 0], u[:, 1]] = vals.permute(1, 0)
    return img, top3


@pytest.mark.parametrize("counts", [(3, 1024, "full"), (1025, 700, 1024)])
def test_boundary_fill_equals_oracle(counts):
    """n = 3 images with different boundary counts in one launch: 3 (the minimum), below / exactly / one above the 1024-point chunk, and more
    than two chunks.  top3 (squared distances) exact; colours at the source stage's 1e-5 on ALL pixels - both sides break distance ties to the
    lowest boundary index, so tie pixels are not excluded."""
    conf, outpad, src, edges, nfull = _fill_case()
    counts = [nfull if c == "full" else c for c in counts]
    r = _rs(14)
    srcs = torch.cat([src, _t(r.uniform(-1, 1, size=(2, 3, H, W)))])
    confs, outs = conf.expand(3, -1, -1, -1).contiguous(), outpad.expand(3, -1, -1, -1).contiguous()
    e = torch.cat([edges[c] for c in counts])
    want_img, want_top3 = _fill_want(srcs, confs, outs, e)
    img, cnt, top3 = ops.boundary_fill(srcs.to(DEV), confs.to(DEV), outs.to(DEV), e.to(DEV), want_top3=True)
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == counts
    assert torch.equal(top3.cpu().long(), want_top3), "top-3 squared distances differ"
    assert int((want_top3[:, 0] >= 0).sum()) > 3 * 1000
    _cmp(img, want_img, 1e-5, "boundary fill colours")
    one, _, one3 = ops.boundary_fill(srcs[1:2].to(DEV), confs[1:2].to(DEV), outs[1:2].to(DEV), e[1:2].to(DEV), want_top3=True)
    assert torch.equal(one, img[1:2]) and torch.equal(one3, top3[1:2]), "an image depends on its batch"


def test_boundary_fill_without_a_band_and_with_too_few_points():
    """An empty uncertain band (outer mask = confidant mask) with a full edge list, and fewer than three boundary pixels (0 and 2) with a full
    band.  For the latter the reference raises (topk of 3 out of fewer); the kernel's code states src * confidant with top3 = -1 - only that is
    asserted here."""
    conf, outpad, src, edges, nfull = _fill_case()
    srcs = src.expand(3, -1, -1, -1).contiguous()
    confs = conf.expand(3, -1, -1, -1).contiguous()
    outs = torch.cat([conf, outpad, outpad])
    e = torch.cat([edges[nfull], edges[0], edges[2]])
    img, cnt, top3 = ops.boundary_fill(srcs.to(DEV), confs.to(DEV), outs.to(DEV), e.to(DEV), want_top3=True)
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [nfull, 0, 2]
    assert torch.equal(img.cpu(), srcs * confs) and (top3 == -1).all()
    from oracle import lwg_oracle as orc
    want, _, _ = orc.make_morph_image(srcs[:1], confs[:1], outs[:1], thin=e[:1])      # the oracle agrees on the empty band
    assert torch.equal(img[:1].cpu(), want)


# ------------------------------------------------------------------------------------------------------------------ grid_sample
def _grid(n, Ho, Wo, Hi, Wi, seed):
    """Uniform in [-1.3, 1.3] with planted values: exact texel centres, +-1, just outside, -2 (the flows' background sentinel), +-1e9."""
    r = _rs(seed)
    g = r.uniform(-1.3, 1.3, size=(n, Ho, Wo, 2)).astype(np.float32)
    k = r.randint(0, 1 << 30, size=(n, Ho, Wo))
    cx, cy = (2.0 * (k % Wi) + 1) / Wi - 1, (2.0 * (k % Hi) + 1) / Hi - 1
    sel = k % 6 == 0
    g[sel] = np.stack([cx, cy], axis=-1)[sel]
    for m, v in ((1, 1.0), (2, -1.0), (3, 1.0 + 2.0 ** -20), (4, -1.0 - 2.0 ** -20), (5, -2.0), (7, 1e9), (8, -1e9)):
        sel = k % 37 == m
        which = (k // 37) % 3                                   # x only, y only, both
        g[..., 0][sel & (which != 1)] = v
        g[..., 1][sel & (which != 0)] = v
    return torch.tensor(g)


@pytest.mark.parametrize("C", [1, 3, 4])
def test_grid_sample_equals_fp64(C):
    """F.grid_sample (bilinear, zeros, align_corners=False) evaluated in fp64 on the same fp32 grid, 1e-5 by _cmp (extract_tex's bound); the
    function is continuous, so no pixel is excluded.  H != W, Ho != Wo, per-image inputs and one image broadcast over n = 3."""
    Hi, Wi, Ho, Wo, n = 24, 40, 36, 52, 3
    img = _t(_rs(20 + C).uniform(-1, 1, size=(n, C, Hi, Wi)))
    grid = _grid(n, Ho, Wo, Hi, Wi, 30 + C)
    for src in (img, img[:1]):
        want = F.grid_sample(src.double().expand(n, -1, -1, -1), grid.double(), mode="bilinear", padding_mode="zeros", align_corners=False)
        got = ops.grid_sample(src.to(DEV), grid.to(DEV))
        torch.cuda.synchronize()
        assert tuple(got.shape) == (n, C, Ho, Wo)
        m = _cmp(got, want, 1e-5, f"grid_sample C={C} images={src.shape[0]}")
        print("grid_sample", C, src.shape[0], m)
        far = (grid.abs() > 1.0 + 2.0 / Hi).any(-1)              # wholly outside: exactly zero
        assert far.any() and (got.cpu().permute(0, 2, 3, 1)[far] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ UV merges, packing
def _vis(shape, seed):
    return _t(np.array([0.0, 0.25, 0.5, 1.0])[_rs(seed).randint(0, 4, size=shape)])


@pytest.mark.parametrize("ns", [1, 2, 4])
def test_uv_merges_equal_fp64(ns):
    """fp64 restatements of models/flowcomposition.py:123-130 (uv_merge) and :816-856 (uv_merge_parts) at input_G_bg's 1e-6 by _cmp.
    Visibilities come from {0, 0.25, 0.5, 1}: their sums are exact, so vis_sum >= 1 is decided alike on both sides."""
    warp, vis = _t(_rs(40 + ns).uniform(-1, 1, size=(ns, 3, H, W))), _vis((ns, 1, H, W), 50 + ns)
    w, v = warp.double(), vis.double()
    vis_sum = v[1:].sum(dim=0)
    temp = (w[1:] * v[1:]).sum(dim=0) / (vis_sum + 1e-5)
    front_invisible = (1 - v[0]) * (vis_sum >= 1).double()
    want = w[0] * (1 - front_invisible) + temp * front_invisible
    if ns > 1:
        assert 0.1 < float((front_invisible > 0).double().mean()) < 0.9
    _cmp(ops.uv_merge(warp.to(DEV), vis.to(DEV)), want, 1e-6, f"uv_merge ns={ns}")
    norm = v / (v.sum(dim=0, keepdim=True) + 1e-7)
    _cmp(ops.uv_merge_parts(warp.to(DEV), vis.to(DEV)), (w * norm).sum(dim=0, keepdim=True), 1e-6, f"uv_merge_parts n={ns}")


@pytest.mark.parametrize("Cp", [4, 8])
def test_pack_inputs_is_an_exact_gather(Cp):
    """cat[a * mask, b] (NCHW) -> NHWC padded to Cp channels with zeros: with and without a mask, with and without b (Cb = 0)."""
    n = 2
    a, b, mask = _t(_rs(60).uniform(-1, 1, size=(n, 3, H, W))), _t(_rs(61).uniform(-1, 1, size=(n, Cp - 3, H, W))), _vis((n, 1, H, W), 62)
    for bb in (b, None):
        for mm in (mask, None):
            want = torch.zeros(n, H, W, Cp)
            want[..., :3] = (a * mm if mm is not None else a).permute(0, 2, 3, 1)
            if bb is not None:
                want[..., 3:] = bb.permute(0, 2, 3, 1)
            got = ops.pack_inputs(a.to(DEV), None if bb is None else bb.to(DEV), None if mm is None else mm.to(DEV), Cp)
            assert torch.equal(got.cpu(), want), (Cp, bb is not None, mm is not None)
