"""The sub-tile form of the list-driven SPADE convolutions (csrc/spade_skip.hip lwg_spade_skip_fine_lists_f32, lwg_conv2d_winograd4_fine_f32;
DESIGN.md 3.12e) on the GPU: every comparison is bitwise (torch.equal) against the plain entry point.

  * classifier: the heavy sub-tiles are exactly those whose window (the 16 x 8 sub-tile grown by d) holds a foreground pixel - single pixels at distance
    1, 2, 5, 6 from a sub-tile edge (x = 16) and corner (16, 8) INSIDE a 32 x 16 block, where the block rule and the sub-tile rule disagree; lists
    ascending, disjoint, complete over the in-image sub-tiles; a block's mark = the OR of its sub-tiles' marks;
  * kernel: groups of heavy sub-tiles from different frames, rows and columns with a count that is no multiple of four, all background, all
    foreground (the fallback order), image corners, a ragged image (40 x 72), four column blocks (N = 256);
  * generator: run_tsf with the switch on and off, and the sub-tile entry point is the one that ran."""
import functools

import pytest
import torch

from ipercore_amd import _lib, ops
from ipercore_amd.networks import packing
from tests.gpu_checks import DEV, _rand, _spec_dev

pytestmark = pytest.mark.gpu


def _sub_id(f, y, x, h, w):
    bx, by = (w + 31) // 32, (h + 15) // 16
    return 4 * (f * bx * by + (y // 16) * bx + x // 32) + 2 * ((y % 16) // 8) + (x % 32) // 16


def _expected_heavy(T, d):
    """The definition on the CPU: sub-tile ids whose window holds a pixel with an in-image flow value (``_flows`` writes background as -2)."""
    B, _, h, w, _ = T.shape
    fg = (T > -1.5).any(dim=4).any(dim=1).float().view(B, 1, h, w)
    dil = torch.nn.functional.max_pool2d(fg, 2 * d + 1, stride=1, padding=d) if d else fg
    cell = torch.nn.functional.max_pool2d(dil, (8, 16), stride=(8, 16), ceil_mode=True).view(B, (h + 7) // 8, (w + 15) // 16)
    return {_sub_id(f, 8 * sy, 16 * sx, h, w) for f, sy, sx in cell.nonzero().tolist()}


def _all_subs(B, h, w):
    return {_sub_id(f, y, x, h, w) for f in range(B) for y in range(0, h, 8) for x in range(0, w, 16)}


def _classify(T, d):
    """The classifier's lists of a flow batch, checked against the definition; -> (heavy sub-tile set, the SkipLists)."""
    B, _, h, w, _ = T.shape
    lists = ops.spade_skip_lists(T.to(DEV), d)
    heavy, light, counts = lists                               # the block-level contract
    fh, fl, fc = lists.fine
    assert counts.numel() == 2 and fc.numel() == 2
    nh, nl = (int(v) for v in fc.cpu())
    hv, lt = fh[:nh].cpu().tolist(), fl[:nl].cpu().tolist()
    assert hv == sorted(hv) and lt == sorted(lt) and not set(hv) & set(lt)
    assert set(hv) | set(lt) == _all_subs(B, h, w), "the lists hold every in-image sub-tile, and no other"
    assert set(hv) == _expected_heavy(T, d)
    nbh = int(counts[0])
    assert set(heavy[:nbh].cpu().tolist()) == {u // 4 for u in hv}, "a block's mark is the OR of its sub-tiles' marks"
    return set(hv), lists


def _flows(pattern, B, H, W):
    """(B, 2, H, W, 2) flows: -2 = background, in-image values = foreground."""
    T = torch.full((B, 2, H, W, 2), -2.0)
    fg = _rand((B, 2, H, W, 2), 31, 0.5).clamp(-0.9, 0.9)
    if pattern == "all_fg":
        return fg
    if pattern in ("singles", "mixed"):
        # block (1, 1) = pixels (32.., 16..): its inner edge x = 48 and inner corner (48, 24).  Frame k: ONE foreground pixel at distance dist left of
        # the edge in the bottom-left sub-tile (frames 0-3), diagonally from the corner in the top-left sub-tile (frames 4-7)
        for k, dist in enumerate((1, 2, 5, 6)):
            T[k, k % 2, 28, 48 - dist] = fg[k, 0, 28, 48 - dist]
            T[4 + k, k % 2, 24 - dist, 48 - dist] = fg[4 + k, 0, 24 - dist, 48 - dist]
    if pattern == "mixed":
        T[8] = fg[8]                                          # a frame that is all foreground
        T[9, 0, 5:30, 10:50] = fg[9, 0, 5:30, 10:50]          # a body-sized rectangle
        T[10, 1, H - 3:, W - 2:] = fg[10, 1, H - 3:, W - 2:]  # the bottom-right corner
        T[11, 0, 0, 0] = fg[11, 0, 0, 0]                      # the top-left pixel, one next to a sub-tile edge of the bottom row, the bottom-right pixel
        T[11, 1, H - 1, 15] = fg[11, 1, H - 1, 15]
        T[11, 1, H - 1, W - 1] = fg[11, 1, H - 1, W - 1]
    if pattern == "corners":
        T[0, 0, 0, 0] = fg[0, 0, 0, 0]
        T[1, 1, H - 1, W - 1] = fg[1, 1, H - 1, W - 1]
        T[B - 1, 0, H - 1, 0] = fg[B - 1, 0, H - 1, 0]
    return T


@functools.lru_cache(maxsize=None)
def _conv_case(H, W, B, spade, N):
    """Weights, the calibration input frame (random per pixel: a result may depend on its place) and the calibration outputs - once per shape."""
    Cin = 64
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
    xfg = _rand((B, H, W, Cin), 49).to(DEV)
    return sp, xcal, cal, xn, mean, rstd, xfg


def _count_fine_calls():
    """Wrap the ctypes binding of the sub-tile entry point; -> (calls list, restore)."""
    lib = _lib.lib()
    real, calls = lib.lwg_conv2d_winograd4_fine_f32, []

    def counted(*args):
        calls.append(1)
        return real(*args)
    lib.lwg_conv2d_winograd4_fine_f32 = counted

    def restore():
        lib.lwg_conv2d_winograd4_fine_f32 = real
    return calls, restore


def _check_kernel(H, W, B, spade, pattern, N=128, T=None):
    sp, xcal, cal, xn, mean, rstd, xfg = _conv_case(H, W, B, spade, N)
    d = 5 if spade else 1
    r = d - 1                                                  # the input differs from the calibration frame within r pixels of a foreground pixel
    T = _flows(pattern, B, H, W) if T is None else T
    fgpix = (T > -1.5).any(dim=4).any(dim=1).float().view(B, 1, H, W)
    near = torch.nn.functional.max_pool2d(fgpix, 2 * r + 1, stride=1, padding=r).view(B, H, W, 1) > 0
    x = torch.where(near.to(DEV), xfg, xcal.expand(B, H, W, 64)).contiguous()
    heavy, lists = _classify(T, d)
    if pattern == "all_bg":
        assert not heavy
    elif pattern == "all_fg":
        assert heavy == _all_subs(B, H, W)
    elif pattern in ("singles", "mixed"):
        for k, dist in enumerate((1, 2, 5, 6)):
            # straight: the pixel's sub-tile (bottom-left of block (1, 1)) is heavy, its right neighbour exactly while dist <= d
            assert _sub_id(k, 28, 48 - dist, H, W) in heavy
            assert (_sub_id(k, 28, 48, H, W) in heavy) == (dist <= d), (k, dist, d)
            # diagonal: the pixel's sub-tile (top-left) is heavy, the bottom-right one of the SAME block exactly while dist <= d
            assert _sub_id(4 + k, 24 - dist, 48 - dist, H, W) in heavy
            assert (_sub_id(4 + k, 24, 48, H, W) in heavy) == (dist <= d), (4 + k, dist, d)
            assert _sub_id(k, 28, 48, H, W) // 4 == _sub_id(k, 28, 48 - dist, H, W) // 4        # (one block: the block rule calls all of it heavy)
        if pattern == "mixed":
            assert len(heavy) % 4 != 0 and len({u // 4 for u in heavy}) > 8, len(heavy)
    kw = dict(epi=ops.EPI_SPADE, xn=xn, mean=mean, rstd=rstd, act=ops.ACT_RELU) if spade else dict(act=ops.ACT_RELU)
    YC = N // 2 if spade else N
    want, got = torch.zeros(B, H, W, YC, device=DEV), torch.zeros(B, H, W, YC, device=DEV)
    calls, restore = _count_fine_calls()
    try:
        with ops.conv_precision("winograd"):
            assert ops.conv2d_lists_apply(x, sp, got, **kw)
            ops.conv2d(x, sp, want, **kw)
            assert not calls
            ops.conv2d(x, sp, got, lists=(lists, cal), **kw)
            assert len(calls) == 1
        torch.cuda.synchronize()
    finally:
        restore()
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert torch.equal(got, want), (pattern, float((got - want).abs().max()), int((got != want).sum()))


@pytest.mark.parametrize("H,W,B", [(64, 64, 20), (40, 72, 12)])
@pytest.mark.parametrize("spade", [False, True], ids=["relu", "spade"])
@pytest.mark.parametrize("pattern", ["all_bg", "all_fg", "singles", "mixed", "corners"])
def test_subtile_kernel_is_bitwise_the_plain_kernel(H, W, B, spade, pattern):
    _check_kernel(H, W, B, spade, pattern)


@pytest.mark.parametrize("spade", [False, True], ids=["relu", "spade"])
def test_four_column_blocks(spade):
    """N = 256 at 32 x 32: two blocks per frame x four column blocks; B = 20 launches the 8-wave form (2 * 160 blocks > 256 CUs)."""
    T = torch.full((20, 2, 32, 32, 2), -2.0)
    fg = _rand((20, 2, 32, 32, 2), 33, 0.5).clamp(-0.9, 0.9)
    for f, (y, x) in enumerate(((3, 3), (12, 20), (20, 9), (29, 30), (8, 16), (15, 15), (0, 31))):
        T[2 * f, f % 2, y, x] = fg[2 * f, 0, y, x]
    T[17] = fg[17]
    _check_kernel(32, 32, 20, spade, "custom", N=256, T=T)


# ---- generator level ----

def test_generator_takes_the_subtile_route_and_frames_do_not_depend_on_it():
    """S = 128, B = 20: both convolutions of the 64^2 site and the gamma | beta convolutions of the others run list-driven - through the sub-tile entry
    point; pred, mask and img are bitwise those of the switch turned off."""
    from tests import test_gpu_spade_skip as base
    im, tsf8, Tst = base._gen_case()
    a, b = tsf8[:20].contiguous(), Tst[:20].contiguous()
    calls, restore = _count_fine_calls()
    try:
        off, lists_off = base._run(im, a, b, False)
        assert not calls and not lists_off
        on, lists_on = base._run(im, a, b, True)
        n_on = len(calls)
        prev, ops.SPADE_SKIP_FINE = ops.SPADE_SKIP_FINE, False
        try:
            blk, _ = base._run(im, a, b, True)                 # the block lists: the sub-tile entry point must not run
        finally:
            ops.SPADE_SKIP_FINE = prev
        assert len(calls) == n_on
    finally:
        restore()
    assert sorted(lists_on) == [(16, 5), (32, 5), (64, 1), (64, 5)], lists_on
    assert n_on >= 4, n_on
    for name, p, q, r in zip(("pred", "mask", "img"), on, off, blk):
        assert p is not None and torch.isfinite(p).all()
        assert torch.equal(p, q) and torch.equal(r, q), name
