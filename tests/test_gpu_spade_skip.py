"""The list-driven SPADE convolutions (ops.SPADE_SKIP; csrc/spade_skip.hip, lwg_conv2d_winograd4_list_f32) on the GPU: every
comparison is bitwise (torch.equal) against the path without lists.

  * predicate: wherever the classifier calls a block light at d = 1, lwb_attention_x's output over the block's window IS the all-background frame's;
  * kernel: the list entry point against lwg_conv2d_winograd4_f32, both epilogues the engine uses, on inputs that differ from the calibration frame
    exactly where the flows say foreground - single pixels at distance 1, 2, 5, 6 from a block's edge and corner separate d = 1, 2 and 5;
  * generator: run_tsf with the switch on and off; batches of the 4-wave form, where the switch must be a no-op;
  * calibration frames: built once per packed weight version and size."""
import functools

import pytest
import torch

from ipercore_amd import ops
from ipercore_amd.networks import generator, packing
from tests import parity_utils as pu
from tests.gpu_checks import DEV, _rand, _spec_dev

pytestmark = pytest.mark.gpu


def _tiles(h, w):
    return (w + 31) // 32, (h + 15) // 16


def _heavy_set(flow, d):
    """The classifier's heavy tiles of a flow batch as a set of tile ids (and both lists checked: ascending, disjoint, complete)."""
    B, _, h, w, _ = flow.shape
    heavy, light, counts = ops.spade_skip_lists(flow, d)
    nh, nl = (int(v) for v in counts.cpu())
    bx, by = _tiles(h, w)
    hv, lt = heavy[:nh].cpu().tolist(), light[:nl].cpu().tolist()
    assert nh + nl == B * bx * by and hv == sorted(hv) and lt == sorted(lt) and sorted(hv + lt) == list(range(B * bx * by))
    return set(hv), (heavy, light, counts)


def _window(t, h, w, d):
    bx, by = _tiles(h, w)
    b, r = divmod(t, bx * by)
    x0, y0 = (r % bx) * 32, (r // bx) * 16
    return b, max(x0 - d, 0), max(y0 - d, 0), min(x0 + 32 + d, w), min(y0 + 16 + d, h)


def _g(ix, size):
    """The flow value whose pixel coordinate is ix: ix = ((g + 1) size - 1) / 2."""
    return (2.0 * ix + 1.0) / size - 1.0


@pytest.mark.parametrize("h,w", [(16, 16), (24, 40)])
def test_light_blocks_see_the_all_background_attention(h, w):
    B, ns, C = 3, 2, 64
    T = torch.full((B, ns, h, w, 2), -2.0)
    # frame 0: background, with values just OUTSIDE the in-image boundary (tx0 = -2, tx0 = w; ty0 = -2, ty0 = h) everywhere in its right part
    T[0, 0, :, w - 8:, 0] = _g(-1.5, w)
    T[0, 1, :, w - 8:, 0] = _g(w + 0.5, w)
    T[0, 0, :, w - 8:, 1] = _g(h + 0.25, h)
    T[0, 1, :, w - 8:, 1] = _g(-1.25, h)
    # frame 1: background but for values just INSIDE the boundary (tx0 = -1 | w - 1) at single pixels of the top-left block
    T[1, 0, 3, 2] = torch.tensor([_g(-0.5, w), 0.1])
    T[1, 1, 5, 6] = torch.tensor([_g(w - 0.5, w), _g(h - 0.5, h)])
    if w > 32:                                                 # ... the rest of frame 1: exact boundary coordinates on the outside (ix = -1 - 1/64, w + 1/64)
        T[1, 0, :, 34:, 0] = _g(-1.015625, w)
        T[1, 1, :, 34:, 0] = _g(w + 0.015625, w)
    # frame 2: random flows
    T[2] = _rand((ns, h, w, 2), 11, 0.7)
    T = T.to(DEV)
    x, Kq, Vs, kap, bv = (_rand(s, 20 + i).to(DEV) for i, s in enumerate(((B, h, w, C), (ns, h, w, C), (ns, h, w, C), (ns, h, w), (C,))))
    att = ops.lwb_attention_x(x, Kq, kap, Vs, bv, T, torch.empty_like(x))
    Tc = torch.full((1, ns, h, w, 2), -2.0, device=DEV)
    att_cal = ops.lwb_attention_x(x[:1].contiguous(), Kq, kap, Vs, bv, Tc, torch.empty(1, h, w, C, device=DEV))
    heavy, _ = _heavy_set(T, 1)
    bx, by = _tiles(h, w)
    nlight = 0
    for t in range(B * bx * by):
        if t in heavy:
            continue
        b, xa, ya, xb, yb = _window(t, h, w, 1)
        assert torch.equal(att[b, ya:yb, xa:xb], att_cal[0, ya:yb, xa:xb]), (t, "a light block's window is not the all-background attention")
        nlight += 1
    # heavy: frame 1's top-left block (the values just inside the boundary) and every block of frame 2; everything else holds background or
    # out-of-image values only
    per = bx * by
    expect = {per} | {2 * per + i for i in range(per)}
    assert heavy == expect and nlight == B * per - len(expect), (sorted(heavy), nlight)


# ---- kernel level ----

def _flows(pattern, B, H, W):
    """(B, 2, H, W, 2) flows: -2 = background, in-image values = foreground."""
    T = torch.full((B, 2, H, W, 2), -2.0)
    fg = _rand((B, 2, H, W, 2), 31, 0.5).clamp(-0.9, 0.9)
    if pattern == "all_fg":
        return fg
    if pattern in ("singles", "mixed"):
        # frame k: ONE foreground pixel at distance dist from the left edge (x = 32) of block (1, 1) - straight (frames 0-3) and diagonally from its
        # top-left corner (32, 16) (frames 4-7)
        for k, dist in enumerate((1, 2, 5, 6)):
            if 16 - dist >= 0 and B > 4 + k:
                T[k, k % 2, 20, 32 - dist] = fg[k, 0, 20, 32 - dist]
                T[4 + k, k % 2, 16 - dist, 32 - dist] = fg[4 + k, 0, 16 - dist, 32 - dist]
    if pattern == "mixed":
        T[8] = fg[8]                                          # a frame that is all foreground
        T[9, 0, 5:30, 10:50] = fg[9, 0, 5:30, 10:50]          # a body-sized rectangle
        T[10, 1, H - 3:, W - 2:] = fg[10, 1, H - 3:, W - 2:]  # the bottom-right corner
        T[11, 0, 0, 0] = fg[11, 0, 0, 0]                      # the top-left pixel
    return T


@functools.lru_cache(maxsize=None)
def _conv_case(H, W, B, spade):
    """Weights, the calibration input frame (random per pixel: a block's result may depend on its place) and the calibration outputs - once per shape."""
    Cin, N = 64, 128
    if spade:
        C = N // 2
        sp = _spec_dev(packing.pack_spade_gamma_beta(_rand((C, Cin, 3, 3), 41, 0.04), _rand((C,), 42, 0.1), _rand((C, Cin, 3, 3), 43, 0.04), _rand((C,), 44, 0.1)))
    else:
        sp = _spec_dev(packing.pack_conv(_rand((N, Cin, 3, 3), 45, 0.04), _rand((N,), 46, 0.1), stride=1, pad=1))
    xcal = _rand((1, H, W, Cin), 47).to(DEV)
    cal = torch.empty(1, H, W, N, device=DEV)
    with ops.conv_precision("winograd"):
        ops.conv2d(xcal, sp, cal, act=ops.ACT_NONE if spade else ops.ACT_RELU)       # SPADE: gamma | beta columns, no epilogue, no activation
    xn = (_rand((B, H, W, N // 2), 48, 2.0) + 0.5).to(DEV)
    mean = xn.reshape(B, -1, N // 2).mean(1).contiguous()
    rstd = (1 / torch.sqrt(xn.reshape(B, -1, N // 2).var(1, unbiased=False) + 1e-5)).contiguous()
    return sp, xcal, cal, xn, mean, rstd


@pytest.mark.parametrize("H,W,B", [(64, 64, 20), (40, 72, 12)])
@pytest.mark.parametrize("spade", [False, True], ids=["relu", "spade"])
@pytest.mark.parametrize("pattern", ["all_bg", "all_fg", "singles", "mixed"])
def test_list_kernel_is_bitwise_the_plain_kernel(H, W, B, spade, pattern):
    sp, xcal, cal, xn, mean, rstd = _conv_case(H, W, B, spade)
    d = 5 if spade else 1
    r = d - 1                                                  # the input differs from the calibration frame within r pixels of a foreground pixel
    T = _flows(pattern, B, H, W)
    fgpix = (T > -1.5).any(dim=4).any(dim=1).float().view(B, 1, H, W)                  # the in-image values of _flows
    near = torch.nn.functional.max_pool2d(fgpix, 2 * r + 1, stride=1, padding=r).view(B, H, W, 1) > 0
    x = torch.where(near.to(DEV), _rand((B, H, W, 64), 49).to(DEV), xcal.expand(B, H, W, 64)).contiguous()
    heavy, lists = _heavy_set(T.to(DEV), d)
    bx, by = _tiles(H, W)
    if pattern == "all_bg":
        assert not heavy
    elif pattern == "all_fg":
        assert len(heavy) == B * bx * by
    else:
        # block (1, 1) of frame k (straight) and 4 + k (diagonal): heavy exactly while the pixel's distance is within d
        t11 = bx + 1
        for k, dist in enumerate((1, 2, 5, 6)):
            for f in (k, 4 + k):
                assert (f * bx * by + t11 in heavy) == (dist <= d), (f, dist, d)
                assert f * bx * by + (bx if f == k else 0) in heavy            # the block that holds the pixel
    kw = dict(epi=ops.EPI_SPADE, xn=xn, mean=mean, rstd=rstd, act=ops.ACT_RELU) if spade else dict(act=ops.ACT_RELU)
    YC = 64 if spade else 128
    want, got = torch.zeros(B, H, W, YC, device=DEV), torch.zeros(B, H, W, YC, device=DEV)
    with ops.conv_precision("winograd"):
        assert ops.conv2d_lists_apply(x, sp, got, **kw)
        ops.conv2d(x, sp, want, **kw)
        ops.conv2d(x, sp, got, lists=lists + (cal,), **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert torch.equal(got, want), (pattern, float((got - want).abs().max()), int((got != want).sum()))


# ---- generator level ----

@functools.lru_cache(maxsize=None)
def _gen_case():
    case = pu.build_case(image_size=128, n_res=2, bg_filters=[64, 64, 128], n_frames=20, ns=2)
    im = pu.make_imitator(case, 20)
    tgt = im.prepare_sequence(case.tgt_smpls, "smooth")
    tsf8, Tst = im.make_inputs_for_tsf(im.src_info, tgt, "smooth", t=0)[:2]
    return im, tsf8, Tst


def _run(im, tsf8, Tst, skip):
    calls = []
    real = ops.spade_skip_lists
    prev, ops.SPADE_SKIP = ops.SPADE_SKIP, skip
    ops.spade_skip_lists = lambda flow, d: (calls.append((flow.shape[2], d)), real(flow, d))[1]
    try:
        out = im.generator.run_tsf(tsf8, im.src_info["feats_nhwc"], Tst, bg=im.src_info["bg"], want_pred=True, want_mask=True, want_img=True)
        torch.cuda.synchronize()
    finally:
        ops.SPADE_SKIP, ops.spade_skip_lists = prev, real
    return out, calls


@pytest.mark.parametrize("B", [4, 1, 20])
def test_generator_frames_do_not_depend_on_the_switch(B):
    """S = 128: B = 4 and B = 1 launch every SPADE convolution in the 4-wave form - the switch is a no-op, no list is built; B = 20 takes the list-driven
    form for both convolutions of the 64^2 site and the gamma | beta convolutions of the others (256 CUs).  pred, mask and img are bitwise equal either way."""
    im, tsf8, Tst = _gen_case()
    a, b = tsf8[:B].contiguous(), Tst[:B].contiguous()
    off, calls_off = _run(im, a, b, False)
    on, calls_on = _run(im, a, b, True)
    assert not calls_off
    assert bool(calls_on) == (B == 20), calls_on
    if B == 20:                                                # one list per frame batch, feature size and d (three sites share the 16^2 one)
        assert sorted(calls_on) == [(16, 5), (32, 5), (64, 1), (64, 5)], calls_on
    for name, p, q in zip(("pred", "mask", "img"), on, off):
        assert p is not None and torch.isfinite(p).all()
        assert torch.equal(p, q), (name, B)


def test_calibration_frames_follow_the_packed_weights():
    im, _, _ = _gen_case()
    gen = im.generator
    x = torch.zeros(1, 64, 64, gen.num_filters[0], device=DEV)
    with ops.conv_precision("winograd"):
        st = gen.packed().enc_sites[0]
        c1 = generator.spade_calibration(st, x)
        c2 = generator.spade_calibration(gen.packed().enc_sites[0], x)
        assert c1[0] is c2[0] and c1[1] is c2[1]                                      # unchanged weights: built once
        w = dict(gen.named_parameters())["enc_attlwbs.0.spade.mlp_shared.0.weight"]
        try:
            with torch.no_grad():
                w.mul_(1.5)
            st2 = gen.packed().enc_sites[0]
            assert st2 is not st
            c3 = generator.spade_calibration(st2, x)
            torch.cuda.synchronize()
            assert c3[0].shape == c1[0].shape and not torch.equal(c3[0], c1[0]) and not torch.equal(c3[1], c1[1])
        finally:
            with torch.no_grad():
                w.div_(1.5)


# ---- the classifier's three entry points ----

@pytest.mark.parametrize("B,h,w", [(2, 40, 72), (1, 1, 8)])
@pytest.mark.parametrize("d", [1, 5])
def test_three_classifier_entry_points_agree(B, h, w, d):
    """lwg_spade_skip_lists_f32 (blocks), _fine_lists_f32 (and 16 x 8) and _q8_lists_f32 (and 8 x 8) run one classifier and one scan: what they share
    is bitwise the same - the block marks, lists and counts of all three, the 16 x 8 ones of the latter two.  Frame 0: a body in the middle of a
    background frame, the last frame all background; 40 x 72 has ragged blocks and sub-tiles wholly outside the image (class-2 marks)."""
    ns, i32 = 2, torch.int32
    T = torch.full((B, ns, h, w, 2), -2.0)
    ys, xs = slice(h // 4, max(3 * h // 4, 1)), slice(w // 4, 3 * w // 4)
    T[0, 0, ys, xs] = _rand((B, ns, h, w, 2), 31, 0.5).clamp(-0.9, 0.9)[0, 0, ys, xs]
    T = T.to(DEV)
    tiles = B * ((h + 15) // 16) * ((w + 31) // 32)

    def level(per):                                           # marks, heavy, light (poisoned: the lists' tails are compared too), counts
        return [torch.full((per * tiles,), -7, device=DEV, dtype=i32) for _ in range(3)] + [torch.full((2,), -7, device=DEV, dtype=i32)]

    def run(name, pers):
        out = [level(p) for p in pers]
        ops._lib.check(getattr(ops._lib.lib(), name)(ops._ptr(T), B, ns, h, w, d, *[ops._ptr(t, i32) for lv in out for t in lv], ops._stream()), name)
        return out

    blk, fine, q8 = run("lwg_spade_skip_lists_f32", (1,)), run("lwg_spade_skip_fine_lists_f32", (1, 4)), run("lwg_spade_skip_q8_lists_f32", (1, 4, 8))
    torch.cuda.synchronize()
    for other in (fine, q8):
        for a, b in zip(blk[0], other[0]):
            assert torch.equal(a, b)
    for a, b in zip(fine[1], q8[1]):
        assert torch.equal(a, b)
    marks, _, _, counts = blk[0]
    fmarks, fcounts = fine[1][0], fine[1][3]
    assert int(counts.sum()) == tiles and set(marks.tolist()) <= {0, 1} and int(counts[0]) == int(marks.sum()) and 0 < int(counts[0]) <= tiles // B
    assert int(fcounts.sum()) == B * ((h + 7) // 8) * ((w + 15) // 16) and ((fmarks == 2).any().item() == (h % 16 in range(1, 9) or w % 32 in range(1, 17)))
