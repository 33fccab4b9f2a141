"""The 8 x 8 sub-tile form of the list-driven SPADE convolutions (csrc/spade_skip.hip lwg_spade_skip_q8_lists_f32, csrc/conv_winograd4.hip
lwg_conv2d_winograd4_q8_f32) on the GPU: every comparison is bitwise (torch.equal) against the plain entry point.

  * classifier: the heavy 8 x 8 sub-tiles are exactly those whose window (the sub-tile grown by d) holds a foreground pixel - a torch restatement of
    the definition on the flow patterns of tests/test_gpu_spade_skip_fine.py (single pixels at distance 1, 2, 5, 6 from a sub-tile edge, x = 48, and
    corner, (48, 24)); lists ascending, disjoint, complete over the in-image sub-tiles; the 16 x 8 and the block lists that come out of the same two
    launches are those of the 16 x 8 classifier, a 16 x 8 mark = the OR of its two halves, a block's = the OR of its eight;
  * kernel: the new entry point called directly (the size rule of ``ops.conv2d`` does not hide it) on groups of heavy sub-tiles from different
    frames, rows and columns with a count that is no multiple of eight, all background (nothing but light entries), all foreground (the companion
    kernel runs the plain body), image corners, a ragged image (40 x 72), four column blocks (N = 256);
  * generator: run_tsf with the switch off, the block lists, the 16 x 8 lists and - the threshold forced low - the 8 x 8 lists: pred, mask and img
    bitwise equal, the new entry point ran; with the default threshold it does not run at S = 128, B = 20."""
import ctypes

import pytest
import torch

from ipercore_amd import _lib, ops
from tests import test_gpu_spade_skip_fine as fine
from tests.gpu_checks import DEV, _rand

pytestmark = pytest.mark.gpu


def _sub8_id(f, y, x, h, w):
    bx, by = (w + 31) // 32, (h + 15) // 16
    return 8 * (f * bx * by + (y // 16) * bx + x // 32) + 4 * ((y % 16) // 8) + (x % 32) // 8


def _expected_heavy8(T, d):
    B, _, h, w, _ = T.shape
    fg = (T > -1.5).any(dim=4).any(dim=1).float().view(B, 1, h, w)
    dil = torch.nn.functional.max_pool2d(fg, 2 * d + 1, stride=1, padding=d) if d else fg
    cell = torch.nn.functional.max_pool2d(dil, 8, stride=8, ceil_mode=True).view(B, (h + 7) // 8, (w + 7) // 8)
    return {_sub8_id(f, 8 * sy, 8 * sx, h, w) for f, sy, sx in cell.nonzero().tolist()}


def _all_subs8(B, h, w):
    return {_sub8_id(f, y, x, h, w) for f in range(B) for y in range(0, h, 8) for x in range(0, w, 8)}


class _low_threshold:
    """``ops.SPADE_SKIP_Q8_MIN`` forced to 1 (every list-driven launch is 'large'), or to another value."""

    def __init__(self, value=1):
        self.value = value

    def __enter__(self):
        self.prev, ops.SPADE_SKIP_Q8_MIN = ops.SPADE_SKIP_Q8_MIN, self.value

    def __exit__(self, *exc):
        ops.SPADE_SKIP_Q8_MIN = self.prev


def _classify8(T, d):
    """The 8 x 8 lists of a flow batch against the definition, the coarser lists against the 16 x 8 classifier; -> (heavy set, the SkipLists)."""
    B, _, h, w, _ = T.shape
    with ops.conv_precision("winograd"):
        with _low_threshold(1 << 30):
            ref = ops.spade_skip_lists(T.to(DEV), d)           # nothing is large: lwg_spade_skip_fine_lists_f32
        assert ref.fine8 is None
        with _low_threshold():
            lists = ops.spade_skip_lists(T.to(DEV), d)
    assert lists.fine8 is not None
    qh, ql, qc = lists.fine8
    assert qc.numel() == 2
    nh, nl = (int(v) for v in qc.cpu())
    hv, lt = qh[:nh].cpu().tolist(), ql[:nl].cpu().tolist()
    assert hv == sorted(hv) and lt == sorted(lt) and not set(hv) & set(lt)
    assert set(hv) | set(lt) == _all_subs8(B, h, w), "the lists hold every in-image sub-tile, and no other"
    assert set(hv) == _expected_heavy8(T, d)
    for got, want in ((tuple(lists), tuple(ref)), (lists.fine, ref.fine)):
        cg, cw = got[2].cpu().tolist(), want[2].cpu().tolist()
        assert cg == cw
        assert torch.equal(got[0][:cg[0]], want[0][:cw[0]]) and torch.equal(got[1][:cg[1]], want[1][:cw[1]])
    fh = lists.fine[0][:int(lists.fine[2][0])].cpu().tolist()
    assert set(fh) == {4 * (u // 8) + 2 * ((u % 8) // 4) + (u % 4) // 2 for u in hv}, "a 16 x 8 mark is the OR of its two halves"
    assert set(lists[0][:int(lists[2][0])].cpu().tolist()) == {u // 8 for u in hv}, "a block's mark is the OR of its eight"
    return hv, lists


@pytest.mark.parametrize("H,W,B", [(64, 64, 20), (40, 72, 12)])
@pytest.mark.parametrize("d", [1, 5])
@pytest.mark.parametrize("pattern", ["all_bg", "all_fg", "singles", "mixed", "corners"])
def test_classifier_against_the_definition(H, W, B, d, pattern):
    T = fine._flows(pattern, B, H, W)
    hv, _ = _classify8(T, d)
    heavy = set(hv)
    if pattern == "all_bg":
        assert not heavy
    elif pattern == "all_fg":
        assert heavy == _all_subs8(B, H, W)
    elif pattern in ("singles", "mixed"):
        for k, dist in enumerate((1, 2, 5, 6)):
            # straight: the pixel's sub-tile is heavy, its right neighbour (x = 48 ..) exactly while dist <= d
            assert _sub8_id(k, 28, 48 - dist, H, W) in heavy
            assert (_sub8_id(k, 28, 48, H, W) in heavy) == (dist <= d), (k, dist, d)
            # diagonal: the pixel's sub-tile is heavy, the one across the corner (48, 24) exactly while dist <= d
            assert _sub8_id(4 + k, 24 - dist, 48 - dist, H, W) in heavy
            assert (_sub8_id(4 + k, 24, 48, H, W) in heavy) == (dist <= d), (4 + k, dist, d)


def _q8_direct(x, sp, y, lists8, cal, **kw):
    """lwg_conv2d_winograd4_q8_f32 itself, as ``ops.conv2d`` calls it."""
    a = ops.conv_args(x, sp, y, None, kw.get("epi", ops.EPI_NONE), kw.get("act", ops.ACT_NONE), None, kw.get("xn"), kw.get("mean"), kw.get("rstd"))
    a.w = ops._ptr(ops._wwino4(sp))
    i32 = torch.int32
    ld = _lib.LwgConvLists(ops._ptr(lists8[0], i32), ops._ptr(lists8[1], i32), ops._ptr(lists8[2], i32), ops._ptr(cal))
    _lib.check(_lib.lib().lwg_conv2d_winograd4_q8_f32(a, ctypes.byref(ld), ops._stream()), "lwg_conv2d_winograd4_q8_f32")


def _check_kernel(H, W, B, spade, pattern, N=128, T=None):
    sp, xcal, cal, xn, mean, rstd, xfg = fine._conv_case(H, W, B, spade, N)
    d = 5 if spade else 1
    r = d - 1                                                  # the input differs from the calibration frame within r pixels of a foreground pixel
    T = fine._flows(pattern, B, H, W) if T is None else T
    fgpix = (T > -1.5).any(dim=4).any(dim=1).float().view(B, 1, H, W)
    near = torch.nn.functional.max_pool2d(fgpix, 2 * r + 1, stride=1, padding=r).view(B, H, W, 1) > 0
    x = torch.where(near.to(DEV), xfg, xcal.expand(B, H, W, 64)).contiguous()
    hv, lists = _classify8(T, d)
    per = (H + 15) // 16 * ((W + 31) // 32) * 8                # sub-tile ids per frame
    if pattern == "all_bg":
        assert not hv
    elif pattern == "all_fg":
        assert len(hv) == len(_all_subs8(B, H, W))            # the companion kernel's case
    elif pattern == "custom" or (pattern == "mixed" and H == 40):
        assert len(hv) % 8 != 0, len(hv)                      # a last group with empty slots (86 | 133 and 30 | 49 heavy sub-tiles)
    if pattern in ("singles", "mixed", "custom"):
        assert any(hv[i] // per != hv[i + 7] // per for i in range(0, len(hv) - 7, 8)), "a group spans frames"
    kw = dict(epi=ops.EPI_SPADE, xn=xn, mean=mean, rstd=rstd, act=ops.ACT_RELU) if spade else dict(act=ops.ACT_RELU)
    YC = N // 2 if spade else N
    want, got = torch.zeros(B, H, W, YC, device=DEV), torch.zeros(B, H, W, YC, device=DEV)
    with ops.conv_precision("winograd"):
        assert ops.conv2d_lists_apply(x, sp, got, **kw)
        ops.conv2d(x, sp, want, **kw)
        _q8_direct(x, sp, got, lists.fine8, cal, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert torch.equal(got, want), (pattern, float((got - want).abs().max()), int((got != want).sum()))


@pytest.mark.parametrize("H,W,B", [(64, 64, 20), (40, 72, 12)])
@pytest.mark.parametrize("spade", [False, True], ids=["relu", "spade"])
@pytest.mark.parametrize("pattern", ["all_bg", "all_fg", "singles", "mixed", "corners"])
def test_q8_kernel_is_bitwise_the_plain_kernel(H, W, B, spade, pattern):
    _check_kernel(H, W, B, spade, pattern)


@pytest.mark.parametrize("spade", [False, True], ids=["relu", "spade"])
def test_q8_four_column_blocks(spade):
    """N = 256 at 32 x 32: two blocks per frame x four column blocks; B = 20 launches the 8-wave form (2 * 160 blocks > 256 CUs)."""
    T = torch.full((20, 2, 32, 32, 2), -2.0)
    fg = _rand((20, 2, 32, 32, 2), 33, 0.5).clamp(-0.9, 0.9)
    for f, (y, x) in enumerate(((3, 3), (12, 20), (20, 9), (29, 30), (8, 16), (15, 15), (0, 31))):
        T[2 * f, f % 2, y, x] = fg[2 * f, 0, y, x]
    T[17] = fg[17]
    T[19, 0, 9, 9] = fg[19, 0, 9, 9]
    _check_kernel(32, 32, 20, spade, "custom", N=256, T=T)


# ---- generator level ----

def _count_q8_calls():
    lib = _lib.lib()
    real, calls = lib.lwg_conv2d_winograd4_q8_f32, []

    def counted(*args):
        calls.append(1)
        return real(*args)
    lib.lwg_conv2d_winograd4_q8_f32 = counted

    def restore():
        lib.lwg_conv2d_winograd4_q8_f32 = real
    return calls, restore


def test_generator_routes_and_frames_do_not_depend_on_them():
    """S = 128, B = 20: switch off, block lists, 16 x 8 lists (the default route of these small launches - the new entry point must not run) and, the
    threshold forced low, 8 x 8 lists (it must run): pred, mask and img are bitwise equal."""
    from tests import test_gpu_spade_skip as base
    im, tsf8, Tst = base._gen_case()
    a, b = tsf8[:20].contiguous(), Tst[:20].contiguous()
    calls, restore = _count_q8_calls()
    fcalls, frestore = fine._count_fine_calls()
    try:
        off, _ = base._run(im, a, b, False)
        sub, lists_on = base._run(im, a, b, True)              # default threshold: 16 x 8
        assert not calls and len(fcalls) >= 4
        n16 = len(fcalls)
        with _low_threshold():
            q8, lists_q8 = base._run(im, a, b, True)
        assert len(calls) == n16 and len(fcalls) == n16, (len(calls), len(fcalls), n16)
        prev, ops.SPADE_SKIP_Q8 = ops.SPADE_SKIP_Q8, False
        try:
            with _low_threshold():
                base._run(im, a, b, True)                      # the switch off: 16 x 8 whatever the threshold
            assert len(calls) == n16 and len(fcalls) == 2 * n16
        finally:
            ops.SPADE_SKIP_Q8 = prev
        prev, ops.SPADE_SKIP_FINE = ops.SPADE_SKIP_FINE, False
        try:
            blk, _ = base._run(im, a, b, True)
        finally:
            ops.SPADE_SKIP_FINE = prev
        assert len(calls) == n16 and len(fcalls) == 2 * n16
    finally:
        restore()
        frestore()
    assert sorted(lists_on) == sorted(lists_q8) == [(16, 5), (32, 5), (64, 1), (64, 5)]
    for name, p, q, r, s in zip(("pred", "mask", "img"), q8, off, sub, blk):
        assert p is not None and torch.isfinite(p).all()
        assert torch.equal(p, q) and torch.equal(r, q) and torch.equal(s, q), name
