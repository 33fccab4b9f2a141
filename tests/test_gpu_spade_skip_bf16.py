"""The list-driven SPADE convolutions of the bf16 engine (lwg_conv2d_nhwc_bf16_hr_list, lwg_conv2d_nhwc_bf16_hr_acc; ops.SPADE_SKIP_BF16; DESIGN.md
3.12f) on the GPU.  Every comparison is bitwise (torch.equal) against the plain lwg_conv2d_nhwc_bf16_hr launch on the same inputs.

  * kernel: 3 distinct frames at 40 x 48 (sub-tiles outside the image on both edges) and 16 x 16; Cin 64 (one chunk: no barrier inside the K loop) and
    128; N 128 and 256 (one and two column tiles of the WAVES_M = 1 instantiation - the only one a SPADE launch of the shipped generators reaches:
    `shared` has N = 128, gamma | beta N = 2 C with C in {64, 128, 256}); LWG_EPI_NONE + ReLU with d = 1 and LWG_EPI_SPADE with d = 2 and real xn /
    mean / rstd; flows all -2 except single foreground pixels at distance d and d + 1 from a sub-tile's edge and corner; an all-background and an
    all-foreground batch; the lists are checked against the definition, and that both kinds of entry occurred where expected;
  * generator: the tiny AttLWB-SPADE configuration at S = 64 in "bf16": frames with the switch on = frames with it off, a frame in a batch of 1 = the
    same frame in a batch of 3, the list launches ran, the calibration is built once per weight version and again after a parameter update;
  * rules: conv2d_lists_apply per mode and switch; the entry points refuse NULL and invalid arguments before any launch."""
import ctypes
import functools

import pytest
import torch

from ipercore_amd import _lib, ops, synthetic
from ipercore_amd.networks import NetworksFactory, generator_param_shapes, packing
from tests import lwbfuse_bf16_emu as emu16
from tests import parity_utils as pu
from tests.gpu_checks import DEV, _rand, _spec_dev
from tests.test_gpu_spade_skip_fine import _all_subs, _expected_heavy, _sub_id

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(autouse=True)
def _switch_on():
    prev = ops.SPADE_SKIP, ops.SPADE_SKIP_BF16
    ops.SPADE_SKIP = ops.SPADE_SKIP_BF16 = True
    yield
    ops.SPADE_SKIP, ops.SPADE_SKIP_BF16 = prev


def _count(name):
    """Wrap one ctypes entry point; -> (calls list, restore)."""
    lib = _lib.lib()
    real, calls = getattr(lib, name), []

    def counted(*args):
        calls.append(1)
        return real(*args)
    setattr(lib, name, counted)
    return calls, lambda: setattr(lib, name, real)


def _classify(T, d):
    """The sub-tile lists of a flow batch against the definition; -> (heavy sub-tile set, the SkipLists)."""
    B, _, h, w, _ = T.shape
    lists = ops.spade_skip_lists(T.to(DEV), d)
    fh, fl, fc = lists.fine
    nh, nl = (int(v) for v in fc.cpu())
    hv, lt = fh[:nh].cpu().tolist(), fl[:nl].cpu().tolist()
    assert hv == sorted(hv) and lt == sorted(lt) and not set(hv) & set(lt)
    assert set(hv) | set(lt) == _all_subs(B, h, w) and set(hv) == _expected_heavy(T, d)
    return set(hv), lists


def _flows(pattern, H, W, d):
    """(3, 2, H, W, 2) flows: -2 = background, in-image values = foreground."""
    T = torch.full((3, 2, H, W, 2), -2.0)
    fg = _rand((3, 2, H, W, 2), 31, 0.5).clamp(-0.9, 0.9)
    if pattern == "all_fg":
        return fg
    if pattern == "singles":
        def put(f, s, y, x):
            T[f, s, y, x] = fg[f, s, y, x]
        if W >= 32:
            # the edge x = 16 between sub-tiles (0, 0) and (0, 16): a pixel d left of it reaches the right one's window, d + 1 does not
            put(0, 0, 4, 16 - d)
            put(1, 1, 4, 16 - d - 1)
            # the corner (32, 24) of sub-tile (24, 32): diagonally d / d + 1 away, inside sub-tile (16, 16)
            put(1, 0, 24 - d, 32 - d)
            put(0, 1, 24 - d - 1, 32 - d - 1)
            put(2, 0, H - 1, W - 1)                            # the ragged bottom-right sub-tile alone
        else:
            # 16 x 16: two sub-tiles, the edge y = 8
            put(0, 0, 8 - d, 5)
            put(1, 1, 8 - d - 1, 5)
    return T                                                   # (frame 2 of the small image, and "all_bg": nothing)


@functools.lru_cache(maxsize=None)
def _conv_case(H, W, spade, Cin, N):
    """Weights, the calibration input frame (random per pixel: a result may depend on its place), the calibration frame the kernel takes, the SPADE
    operands and the foreground input - once per shape."""
    B = 3
    if spade:
        C = N // 2
        sp = _spec_dev(packing.pack_spade_gamma_beta(_rand((C, Cin, 3, 3), 41, 0.04), _rand((C,), 42, 0.1), _rand((C, Cin, 3, 3), 43, 0.04), _rand((C,), 44, 0.1)))
    else:
        sp = _spec_dev(packing.pack_conv(_rand((N, Cin, 3, 3), 45, 0.04), _rand((N,), 46, 0.1), stride=1, pad=1))
    xcal = _rand((1, H, W, Cin), 47).to(BF).to(DEV)
    with ops.conv_precision("bf16"):
        if spade:
            cal = ops.conv2d_acc_frame(xcal, sp)               # fp32 accumulators, the kernel's column order
            assert cal.dtype == torch.float32 and tuple(cal.shape) == (1, H, W, N)
        else:
            cal = ops.conv2d(xcal, sp, torch.empty(1, H, W, N, device=DEV, dtype=BF), act=ops.ACT_RELU)
    xn32 = _rand((B, H, W, N // 2), 48, 2.0) + 0.5
    xn = xn32.to(BF).to(DEV)
    mean = xn32.reshape(B, -1, N // 2).mean(1).contiguous().to(DEV)
    rstd = (1 / torch.sqrt(xn32.reshape(B, -1, N // 2).var(1, unbiased=False) + 1e-5)).contiguous().to(DEV)
    xfg = _rand((B, H, W, Cin), 49).to(BF).to(DEV)
    return sp, xcal, cal, xn, mean, rstd, xfg


def _check_kernel(H, W, spade, Cin, N, pattern):
    B = 3
    sp, xcal, cal, xn, mean, rstd, xfg = _conv_case(H, W, spade, Cin, N)
    d = ops.SPADE_SKIP_D_BF16[1 if spade else 0]
    r = d - 1                                                  # the input differs from the calibration frame within r pixels of a foreground pixel
    T = _flows(pattern, H, W, d)
    fgpix = (T > -1.5).any(dim=4).any(dim=1).float().view(B, 1, H, W)
    near = torch.nn.functional.max_pool2d(fgpix, 2 * r + 1, stride=1, padding=r).view(B, H, W, 1) > 0
    x = torch.where(near.to(DEV), xfg, xcal.expand(B, H, W, Cin)).contiguous()
    heavy, lists = _classify(T, d)
    every = _all_subs(B, H, W)
    if pattern == "all_bg":
        assert not heavy
    elif pattern == "all_fg":
        assert heavy == every
    elif W >= 32:
        assert _sub_id(0, 4, 16, H, W) in heavy and _sub_id(1, 4, 16, H, W) not in heavy          # the edge: d reaches, d + 1 does not
        assert _sub_id(1, 24, 32, H, W) in heavy and _sub_id(0, 24, 32, H, W) not in heavy        # the corner
        assert heavy and every - heavy and _sub_id(2, H - 1, W - 1, H, W) in heavy
    else:
        assert _sub_id(0, 8, 0, H, W) in heavy and _sub_id(1, 8, 0, H, W) not in heavy and len(heavy) == 3
    kw = dict(epi=ops.EPI_SPADE, xn=xn, mean=mean, rstd=rstd, act=ops.ACT_RELU) if spade else dict(act=ops.ACT_RELU)
    YC = N // 2 if spade else N
    n = B * H * W * YC
    bw, bg = torch.full((n + 4096,), -7.0, device=DEV, dtype=BF), torch.full((n + 4096,), -7.0, device=DEV, dtype=BF)
    want, got = bw[:n].view(B, H, W, YC), bg[:n].view(B, H, W, YC)
    calls, restore = _count("lwg_conv2d_nhwc_bf16_hr_list")
    try:
        with ops.conv_precision("bf16"):
            assert ops.conv2d_lists_apply(x, sp, got, **kw)
            ops.conv2d(x, sp, want, **kw)
            assert not calls
            ops.conv2d(x, sp, got, lists=(lists, cal), **kw)
            assert len(calls) == 1
        torch.cuda.synchronize()
    finally:
        restore()
    assert torch.isfinite(want.float()).all() and float(want.float().abs().max()) > 0
    assert (bg[n:] == -7.0).all(), "the list launch wrote past its output"
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (pattern, int((got.view(torch.int16) != want.view(torch.int16)).sum()))
    if pattern == "singles":
        # the list launch did fill light sub-tiles from the calibration frame: with a foreign frame in its place the result changes there, and only there
        other = torch.full((n,), -7.0, device=DEV, dtype=BF).view(B, H, W, YC)
        with ops.conv_precision("bf16"):
            ops.conv2d(x, sp, other, lists=(lists, torch.zeros_like(cal)), **kw)
        torch.cuda.synchronize()
        diff = (other.view(torch.int16) != want.view(torch.int16)).any(dim=3).cpu()
        assert diff.any()
        for f, y, xx in diff.nonzero().tolist():
            assert _sub_id(f, y, xx, H, W) not in heavy


@pytest.mark.parametrize("H,W", [(40, 48), (16, 16)])
@pytest.mark.parametrize("Cin,N", [(64, 128), (128, 256)])
@pytest.mark.parametrize("spade", [False, True], ids=["relu_d1", "spade_d2"])
@pytest.mark.parametrize("pattern", ["singles", "all_bg", "all_fg"])
def test_list_kernel_is_bitwise_the_plain_kernel(H, W, Cin, N, spade, pattern):
    _check_kernel(H, W, spade, Cin, N, pattern)


# ---- generator level ----

@functools.lru_cache(maxsize=None)
def _gen_case():
    nf, nres, bgf = emu16.CONFIGS["tiny"]
    G = NetworksFactory.get_by_name("AttLWB-SPADE", cfg=pu.gen_cfg(nf, nres, bgf), temporal=False).eval()
    sdn = synthetic.fill_state_dict(generator_param_shapes(nf, nres, bgf), seed=7)
    G.load_state_dict({k: torch.tensor(v) for k, v in sdn.items()}, strict=True)
    G.to(DEV)
    G.conv_precision = "bf16"
    src_inputs, tsf_inputs, Tst = emu16.generator_inputs()
    S, ns = emu16.S, emu16.NS
    src8 = ops.nchw_to_nhwc(src_inputs.reshape(ns, 6, S, S).contiguous().float().to(DEV), c_pad=8)
    feats = G.encode_sources(src8, batched=False, ns=ns)
    # three distinct frames: the rendered flows; the same with the sources swapped; a small patch of them on background
    T = torch.cat([Tst, Tst.flip(1), torch.full_like(Tst, -2.0)], dim=0).float()
    ys, xs = (Tst[0] > -1.5).any(dim=3).any(dim=0).nonzero()[0].tolist()
    y0, x0 = max(min(ys, S - 12), 0), max(min(xs - 6, S - 12), 0)
    T[2, :, y0:y0 + 12, x0:x0 + 12] = Tst[0, :, y0:y0 + 12, x0:x0 + 12]
    tsf = torch.cat([tsf_inputs, tsf_inputs * -0.7, tsf_inputs.flip(3)], dim=0)
    tsf8 = ops.nchw_to_nhwc(tsf.contiguous().float().to(DEV), c_pad=8)
    return G, feats, tsf8, T.contiguous().to(DEV)


def _run(G, feats, tsf8, T, skip):
    """-> ((mask, img), the list launches' (h, d), the classifier's (h, d, heavy, light) counts)."""
    launches, counts = [], []
    real_conv, real_lists = ops.conv2d, ops.spade_skip_lists

    def conv2d(x0, spec, y, *a, **k):
        if k.get("lists") is not None:
            launches.append((x0.shape[1], x0.dtype, k.get("epi", ops.EPI_NONE)))
        return real_conv(x0, spec, y, *a, **k)

    def lists(flow, d):
        out = real_lists(flow, d)
        counts.append((flow.shape[2], d) + tuple(int(v) for v in out.fine[2].cpu()))
        return out
    prev, ops.SPADE_SKIP = ops.SPADE_SKIP, skip
    ops.conv2d, ops.spade_skip_lists = conv2d, lists
    try:
        _, mask, img = G.run_tsf(tsf8, feats, T, bg=None, want_pred=False, want_mask=True, want_img=True)
        torch.cuda.synchronize()
    finally:
        ops.SPADE_SKIP, ops.conv2d, ops.spade_skip_lists = prev, real_conv, real_lists
    return (mask, img), launches, counts


def test_generator_frames_do_not_depend_on_the_switch_or_the_batch():
    G, feats, tsf8, T = _gen_case()
    nf, nres, _ = emu16.CONFIGS["tiny"]
    off, launches_off, _ = _run(G, feats, tsf8, T, False)
    assert not launches_off
    calls, restore = _count("lwg_conv2d_nhwc_bf16_hr_list")
    try:
        on, launches, counts = _run(G, feats, tsf8, T, True)
        ncalls = len(calls)
    finally:
        restore()
    # both convolutions of every attention site ran list-driven, on bf16 tensors, through the new entry point
    assert len(launches) == 2 * (len(nf) + nres) == ncalls, (launches, ncalls)
    assert all(dt == BF for _, dt, _ in launches) and sorted({e for _, _, e in launches}) == [ops.EPI_NONE, ops.EPI_SPADE]
    # one classification per feature size and d; both kinds of sub-tile occurred at the 32^2 site for both reaches
    assert sorted(c[:2] for c in counts) == [(8, 1), (8, 2), (16, 1), (16, 2), (32, 1), (32, 2)], counts
    for h, d, nh, nl in counts:
        assert nh + nl == 3 * ((h + 7) // 8) * ((h + 15) // 16)
        if h == 32:
            assert nh > 0 and nl > 0, counts
    for name, p, q in zip(("mask", "img"), on, off):
        assert torch.isfinite(p).all() and torch.equal(p, q), name
    for f in range(3):
        one, launches1, _ = _run(G, feats, tsf8[f:f + 1].contiguous(), T[f:f + 1].contiguous(), True)
        assert len(launches1) == len(launches)
        for name, p, q in zip(("mask", "img"), one, on):
            assert torch.equal(p[0], q[f]), (name, f)


def test_calibration_is_built_once_per_weight_version():
    G, feats, tsf8, T = _gen_case()
    nf, nres, _ = emu16.CONFIGS["tiny"]
    nsites = len(nf) + nres
    real, built = ops.conv2d_acc_frame, []
    ops.conv2d_acc_frame = lambda *a, **k: (built.append(1), real(*a, **k))[1]
    w = dict(G.named_parameters())["enc_attlwbs.0.spade.mlp_shared.0.weight"]
    w0 = w.detach().clone()
    try:
        G._packed = None                                       # a fresh packed version: no calibration frame yet
        first, _, _ = _run(G, feats, tsf8, T, True)
        assert len(built) == nsites, len(built)
        st = G.packed().enc_sites[0]
        (key, (actv_cal, gb_cal)), = st["cal"].items()
        assert actv_cal.dtype == BF and gb_cal.dtype == torch.float32 and tuple(gb_cal.shape) == (1, 32, 32, st["gb"].N), key
        again, _, _ = _run(G, feats, tsf8, T, True)
        assert len(built) == nsites and G.packed().enc_sites[0] is st
        assert torch.equal(again[1], first[1])
        with torch.no_grad():
            w.mul_(1.5)
        upd, _, _ = _run(G, feats, tsf8, T, True)              # a parameter update: repacked, every site calibrated again
        assert len(built) == 2 * nsites and G.packed().enc_sites[0] is not st
        ref, _, _ = _run(G, feats, tsf8, T, False)
        assert torch.equal(upd[1], ref[1]) and torch.equal(upd[0], ref[0]) and not torch.equal(upd[1], first[1])
    finally:
        ops.conv2d_acc_frame = real
        with torch.no_grad():
            w.copy_(w0)
        G._packed = None


# ---- rules ----

def test_rules_and_refusals():
    H = W = 16
    sp, xcal, cal, xn, mean, rstd, xfg = _conv_case(H, W, True, 64, 128)
    y = torch.full((3, H, W, 64), -7.0, device=DEV, dtype=BF)
    kw = dict(epi=ops.EPI_SPADE, xn=xn, mean=mean, rstd=rstd, act=ops.ACT_RELU)
    with ops.conv_precision("bf16"):
        assert ops.conv2d_lists_apply(xfg, sp, y, **kw)
        for name in ("SPADE_SKIP", "SPADE_SKIP_BF16"):
            setattr(ops, name, False)
            try:
                assert not ops.conv2d_lists_apply(xfg, sp, y, **kw), name
            finally:
                setattr(ops, name, True)
        assert not ops.conv2d_lists_apply(xfg.float(), sp, y.float(), **kw)                      # fp32 tensors: the "winograd" mode's rule
        sp64 = _spec_dev(packing.pack_conv(_rand((64, 64, 3, 3), 45, 0.04), _rand((64,), 46, 0.1), stride=1, pad=1))
        assert not ops.conv2d_lists_apply(xfg, sp64, y, act=ops.ACT_RELU)                        # N = 64: the WAVES_M = 2 form has no list kernel
    with ops.conv_precision("bf16_winograd"):
        assert not ops.conv2d_lists_apply(xfg, sp, y, **kw)
        lists = ops.spade_skip_lists(torch.full((3, 2, H, W, 2), -2.0, device=DEV), 2)
        with pytest.raises(ValueError):
            ops.conv2d(xfg, sp, y, lists=(lists, cal), **kw)
    with ops.conv_precision("winograd"):
        assert not ops.conv2d_lists_apply(xfg, sp, y, **kw)
    # the C entry points: NULL and invalid arguments are refused on the host, nothing is launched (the output keeps its fill)
    lib = _lib.lib()
    assert lib.lwg_conv2d_nhwc_bf16_hr_list_applies(None) == 0
    assert lib.lwg_conv2d_nhwc_bf16_hr_list(None, None, None) == 1 and lib.lwg_conv2d_nhwc_bf16_hr_acc(None, None) == 1
    a = ops._hr_args(ops.conv_args(xfg, sp, y, None, ops.EPI_SPADE, ops.ACT_RELU, None, xn, mean, rstd), sp, ops.EPI_SPADE)
    assert lib.lwg_conv2d_nhwc_bf16_hr_list_applies(a) == 1
    i32 = torch.int32
    fh, fl, fc = lists.fine
    good = (ops._ptr(fh, i32), ops._ptr(fl, i32), ops._ptr(fc, i32), ops._ptr(cal))
    stream = ops._stream()
    assert lib.lwg_conv2d_nhwc_bf16_hr_list(a, None, stream) == 1
    for k in range(4):
        ld = _lib.LwgConvLists(*[None if j == k else p for j, p in enumerate(good)])
        assert lib.lwg_conv2d_nhwc_bf16_hr_list(a, ctypes.byref(ld), stream) == 1, k
    ld = _lib.LwgConvLists(*good)
    for field, value in (("xn", None), ("mean", None), ("x0", None), ("y", None), ("w", None), ("N", 64), ("C1", 64), ("stride", 2), ("ntaps", 4), ("xdt", _lib.DT_F32),
                         ("epi", ops.EPI_RESIDUAL), ("YC", 128), ("M", 5), ("H", 1 << 20)):
        b = ops._hr_args(ops.conv_args(xfg, sp, y, None, ops.EPI_SPADE, ops.ACT_RELU, None, xn, mean, rstd), sp, ops.EPI_SPADE)
        setattr(b, field, value)
        assert lib.lwg_conv2d_nhwc_bf16_hr_list(b, ctypes.byref(ld), stream) == 1, field
        if field not in ("xn", "mean", "x0", "y", "w"):
            assert lib.lwg_conv2d_nhwc_bf16_hr_list_applies(b) == 0, field
    b = ops.conv_args(xcal, sp, cal)
    ops._hr_args(b, sp, ops.EPI_SPADE)
    for field, value in (("ydt", _lib.DT_BF16), ("act", ops.ACT_RELU), ("epi", ops.EPI_SPADE), ("N", 64), ("y", None)):
        c = ops._hr_args(ops.conv_args(xcal, sp, cal), sp, ops.EPI_SPADE)
        setattr(c, field, value)
        assert lib.lwg_conv2d_nhwc_bf16_hr_acc(c, stream) == 1, field
    torch.cuda.synchronize()
    assert (y == -7.0).all()
    assert lib.lwg_conv2d_nhwc_bf16_hr_list(a, ctypes.byref(ld), stream) == 0                    # ... and the valid call runs
    torch.cuda.synchronize()
    assert not (y == -7.0).any()
