"""Host logic of the bf16 convolution family (no GPU): the operand panels ops.py builds for csrc/conv_igemm_bf16.hip must hold, at the
index the kernel reads, the weight the reference convolution applies (attlwb_spade_resunet.py:14-25 conv / :331-340 ConvTranspose2d).
The kernels' own arithmetic is checked on the GPU (tests/gpu_checks.py check_bf16_conv_kernels)."""
import itertools

import numpy as np
import pytest
import torch

from ipercore_amd import ops
from ipercore_amd.networks import packing


def _w(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def test_register_streamed_panel_3x3():
    """[step = chunk * ntaps + tap'][ks][n][e] = W[n][64 chunk + 16 ks + e][tap], taps ascending in (dy, dx)."""
    N, Cin = 128, 192
    w = _w((N, Cin, 3, 3), 1)
    spec = packing.pack_conv(w, None, stride=1)
    panel, bias = ops._w16hr(spec, False)
    assert panel.shape == (Cin // 64 * 9, 4, N, 16) and panel.dtype == torch.bfloat16 and bias is None
    order = ops._hr_tap_order(spec)
    assert order == list(range(9))                                      # a Conv2d's taps are already an ascending grid
    p = panel.float().numpy()
    wq = w.to(torch.bfloat16).float().numpy()
    for chunk, t, ks, e, n in itertools.product(range(3), range(9), range(4), (0, 7, 15), (0, 31, 127)):
        assert p[chunk * 9 + t, ks, n, e] == wq[n, 64 * chunk + 16 * ks + e, t // 3, t % 3]


def test_register_streamed_panel_transposed_parities_sorted():
    """The four parity launches of ConvTranspose2d(4, 2, 1): taps re-ordered ascending (the row-renaming kernel's grid), panel rows
    following; parity (py, px) must use dy in {py-1, py}, dx in {px-1, px} - what the fused launch assumes."""
    Cin, N = 128, 64
    w = _w((Cin, N, 4, 4), 2)
    specs = packing.pack_conv_transpose(w, None)
    wq = w.to(torch.bfloat16).float().numpy()
    # out[2a + p] = sum over (kernel index k, input offset d) of _CT_TAPS[p]:  x[a + d] w[k]
    ct = {0: {0: 1, -1: 3}, 1: {1: 0, 0: 2}}
    for i, spec in enumerate(specs):
        py, px = i >> 1, i & 1
        assert (spec.ooy, spec.oox, spec.omul) == (py, px, 2)
        order = ops._hr_tap_order(spec)
        taps = [(spec.dy[t], spec.dx[t]) for t in order]
        assert taps == [(py - 1, px - 1), (py - 1, px), (py, px - 1), (py, px)]
        panel = ops._w16hr(spec, False)[0].float().numpy()
        assert panel.shape == (Cin // 64 * 4, 4, N, 16)
        for chunk, (ti, (dy, dx)), ks, e, n in itertools.product(range(2), enumerate(taps), range(4), (0, 9), (0, 63)):
            assert panel[chunk * 4 + ti, ks, n, e] == wq[64 * chunk + 16 * ks + e, n, ct[py][dy], ct[px][dx]]


def test_spade_panel_interleaves_gamma_beta_in_blocks_of_16():
    C, Cin = 64, 128
    wg, wb = _w((C, Cin, 3, 3), 3), _w((C, Cin, 3, 3), 4)
    bg, bb = _w((C,), 5), _w((C,), 6)
    spec = packing.pack_spade_gamma_beta(wg, bg, wb, bb)
    panel, bias = ops._w16hr(spec, True)
    p = panel.float().numpy()
    g16, b16 = wg.to(torch.bfloat16).float().numpy(), wb.to(torch.bfloat16).float().numpy()
    for col in (0, 15, 16, 31, 32, 47, 100, 127):
        q, r = col // 32, col % 32
        ch, src, sb = 16 * q + r % 16, (g16 if r < 16 else b16), (bg if r < 16 else bb)
        assert float(bias[col]) == float(sb[ch])
        for t, ks, e in ((0, 0, 0), (4, 2, 5), (8, 3, 15)):
            assert p[1 * 9 + t, ks, col, e] == src[ch, 64 + 16 * ks + e, t // 3, t % 3]


def test_first_layer_panel():
    """lwg_conv2d_nhwc_c8_bf16: [ceil(ntaps / 2)][64][16], k = 8 tap + c, zero past the taps and for the padded channels 6, 7."""
    w = _w((64, 6, 3, 3), 7)
    spec = packing.pack_conv(w, None, stride=2, cin_pad=8)
    panel = ops._w16c8(spec).float().numpy()
    assert panel.shape == (5, 64, 16)
    wq = w.to(torch.bfloat16).float().numpy()
    for ks, n, e in itertools.product(range(5), (0, 17, 63), range(16)):
        tap, c = (16 * ks + e) // 8, (16 * ks + e) % 8
        want = wq[n, c, tap // 3, tap % 3] if (tap < 9 and c < 6) else 0.0
        assert panel[ks, n, e] == want


def test_lds_dma_panel_swizzle():
    """lwg_conv2d_nhwc_bf16: [step][n][64], the eight 16-byte k-octets of row n stored at slot octet ^ ((n >> 1) & 7)."""
    N, Cin = 64, 64
    w = _w((N, Cin, 3, 3), 8)
    spec = packing.pack_conv(w, None)
    panel = ops._w16v2(spec).float().numpy()
    assert panel.shape == (9, N, 64)
    wq = w.to(torch.bfloat16).float().numpy()
    for t, n, octet, e in itertools.product((0, 5, 8), (0, 1, 2, 37, 63), range(8), (0, 7)):
        slot = octet ^ ((n >> 1) & 7)
        assert panel[t, n, 8 * slot + e] == wq[n, 8 * octet + e, t // 3, t % 3]


def test_head_panel_bf16():
    """csrc/bf16_ops.hip lwg_head_bf16_kernel operand: [ky][pass][channel half][lane][8], MFMA row = 4 * tap + output."""
    w_img, w_att = _w((3, 64, 5, 5), 9), _w((1, 64, 5, 5), 10)
    pk = packing.pack_head_bf16(w_img, w_att).float().numpy()
    assert pk.shape == (5, 2, 2, 64, 8)
    w4 = torch.cat([w_img, w_att]).to(torch.bfloat16).float().numpy()
    for ky, half, lane, e in itertools.product(range(5), range(2), (0, 5, 16, 47, 63), (0, 3, 7)):
        row, koct = lane % 16, lane // 16
        tap, o, c = row // 4, row % 4, half * 32 + koct * 8 + e
        assert pk[ky, 0, half, lane, e] == w4[o, c, ky, tap]
        assert pk[ky, 1, half, lane, e] == (w4[o, c, ky, 4] if tap == 0 else 0.0)


def test_panel_cache_bookkeeping(monkeypatch):
    """ops.PanelCache (the one-launch-per-step re-packing of the training step): only tensors living in parameter storage are cached,
    a panel is registered once per (storage address, packing arguments), and refresh() hands the library one descriptor per panel
    with consecutive block ranges."""
    import ctypes

    from ipercore_amd import _lib
    flat = torch.zeros(64 * 32 * 9 + 32 * 64 * 16, requires_grad=True)   # a flat parameter buffer (it trains) with two weight views
    w1 = flat.detach()[:64 * 32 * 9].view(64, 32, 3, 3)
    w2 = flat.detach()[64 * 32 * 9:].view(32, 64, 4, 4)
    frozen = torch.zeros(64, 32, 3, 3)                                   # a loss network's weight: cached, packed once by its caller, never re-packed
    cache = ops.PanelCache([flat, frozen])
    f, fresh_f = cache.get(frozen, False, tuple(range(9)), 32, 32, 64, 64)
    f2, fresh_f2 = cache.get(frozen, False, tuple(range(9)), 32, 32, 64, 64)
    assert fresh_f and not fresh_f2 and f2 is f and cache.cacheable(frozen) and not cache.rows
    assert cache.cacheable(w1) and cache.cacheable(w2) and not cache.cacheable(torch.cat([w1, w1]))
    a, fresh_a = cache.get(w1, False, tuple(range(9)), 32, 32, 64, 64)
    b, fresh_b = cache.get(w1, False, tuple(range(9)), 32, 32, 64, 64)
    c, fresh_c = cache.get(w1, True, tuple(range(9)), 64, 64, 32, 64)   # the data-gradient panel of the same weight
    d, fresh_d = cache.get(w2, True, (5, 7, 13, 15), 32, 32, 64, 64)
    assert fresh_a and not fresh_b and fresh_c and fresh_d and a is b and a is not c
    assert a.shape == (9 * 32 // 4, 64, 4) and c.shape == (9 * 64 // 4, 64, 4) and d.shape == (4 * 32 // 4, 64, 4)
    calls = []

    class _Stub:
        def lwg_pack_panels_f32(self, table, n, blocks, stream):
            calls.append((table, n, blocks))
            return 0
    monkeypatch.setattr(_lib, "lib", lambda: _Stub())
    monkeypatch.setattr(ops, "_stream", lambda: None)
    cache.refresh()
    cache.refresh()
    assert len(calls) == 2 and calls[0][1] == 3 and calls[0] == calls[1]            # the table is built once
    descs = (_lib.LwgPackDesc * 3).from_buffer_copy(bytes(cache.table.numpy().tobytes()))
    firsts = [d_.first_block for d_ in descs]
    sizes = [((d_.Kp // 4) * d_.n_pad + 255) // 256 for d_ in descs]
    assert firsts == [0, sizes[0], sizes[0] + sizes[1]] and calls[0][2] == sum(sizes)
    assert descs[0].w == w1.data_ptr() and descs[2].w == w2.data_ptr() and descs[1].transposed == 1 and list(descs[2].kidx[:4]) == [5, 7, 13, 15]
    assert ctypes.sizeof(_lib.LwgPackDesc) == 264


def test_winograd_panel_cache_and_launch_plan(monkeypatch):
    """Host logic around the Winograd engine in the training step (no GPU): PanelCache.winograd builds a fragment panel once per (GEMM panel, tap
    order), registers it for the per-step refresh only when the source weight trains, and refresh() hands the library one LwgWinoDesc per registered
    panel with consecutive block ranges; ops._wino_plan: the synthesis path (splitk=False) always runs the kernel whole, a training launch takes the
    split form when the library plans one and its slices fill >= WINO_MIN_GRID workgroups, stays whole when the grid is large enough, and is handed
    to the direct kernel (None) otherwise."""
    from ipercore_amd import _lib
    flat = torch.zeros(64 * 64 * 9, requires_grad=True)
    w = flat.detach().view(64, 64, 3, 3)
    frozen = torch.zeros(128, 64, 3, 3)
    cache = ops.PanelCache([flat, frozen])
    calls = []

    class _Stub:
        plan, asked = (0, 0, 64), []

        def lwg_winograd_panel_f32(self, wp, up, cin, n, taps, stream):
            calls.append(("one", cin, n, list(taps)))
            return 0

        def lwg_pack_panels_f32(self, table, n, blocks, stream):
            calls.append(("pack", n, blocks))
            return 0

        def lwg_winograd_panels_f32(self, table, n, blocks, stream):
            calls.append(("all", n, blocks))
            return 0

        def lwg_conv2d_winograd_plan(self, a, with_ws, blocks, slices, nbv, workgroups):
            # the library's answer, stubbed: (64-patch blocks x K slices, slices, channels per block); with_ws = 0: never sliced
            self.asked.append(int(with_ws))
            b, sl, v = self.plan if with_ws else (self.plan[0] // max(1, self.plan[1]), 0, self.plan[2])
            blocks._obj.value, slices._obj.value, nbv._obj.value = b, sl, v
            return 0
    stub = _Stub()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_ptr", lambda t, dt=None: 0 if t is None else t.data_ptr())
    pa, _ = cache.get(w, False, tuple(range(9)), 64, 64, 64, 64)
    pt, _ = cache.get(w, True, tuple(reversed(range(9))), 64, 64, 64, 64)
    pf, _ = cache.get(frozen, False, tuple(range(9)), 64, 64, 128, 128)

    class _Spec:
        def __init__(self, panel, cin):
            self.w, self.Cin = panel, cin
    taps, rtaps = list(range(9)), list(reversed(range(9)))
    ua = cache.winograd(_Spec(pa, 64), taps)
    assert cache.winograd(_Spec(pa, 64), taps) is ua and ua.shape == (16, 8, 2, 64, 4)          # once per (panel, tap order)
    ut = cache.winograd(_Spec(pt, 64), rtaps)
    uf = cache.winograd(_Spec(pf, 64), taps)
    assert uf.shape == (16, 8, 2, 128, 4) and cache.winograd(_Spec(torch.zeros(144, 64, 4), 64), taps) is None      # a per-call temporary: not cached
    assert [c[0] for c in calls] == ["one", "one", "one"] and calls[1][3] == rtaps
    assert len(cache.rows) == 2 and len(cache.wino_rows) == 2                                     # the frozen weight's panels are not re-derived
    calls.clear()
    cache.refresh()
    cache.refresh()
    assert [c[0] for c in calls] == ["pack", "all", "pack", "all"] and calls[1] == calls[3] and calls[1][1] == 2
    descs = (_lib.LwgWinoDesc * 2).from_buffer_copy(bytes(cache.wino_table.numpy().tobytes()))
    per = ((64 + 63) // 64) * ((64 + 15) // 16)
    assert [d_.first_block for d_ in descs] == [0, per] and calls[1][2] == 2 * per
    assert descs[0].wpanel == pa.data_ptr() and descs[0].upk == ua.data_ptr() and descs[1].upk == ut.data_ptr() and list(descs[1].tap9) == rtaps
    # the launch plan
    a = _lib.LwgConvArgs()

    class _S2:
        N = 256
    y_small, y_mid, y_big = torch.zeros(1, 28, 28, 256), torch.zeros(1, 64, 64, 256), torch.zeros(2, 128, 128, 256)
    a.M = 28 * 28
    assert ops._wino_plan(a, _S2, y_small, False) == 0 and ops._wino_plan(a, _S2, y_big, False) == 0     # synthesis path: whole, always (the library is not asked)
    assert stub.asked == []
    stub.plan = (4 * 8, 0, 32)
    assert ops._wino_plan(a, _S2, y_small, True) is None                                                   # 4 tiles x 8 blocks of 32 channels = 32 units, no slices: direct split-K
    a.M = 64 * 64
    stub.plan = (16 * 4, 0, 64)
    assert ops._wino_plan(a, _S2, y_mid, True) == 0                                                        # 16 tiles x 4 blocks of 64 channels = 128 units: whole
    a.M = 28 * 28
    stub.plan = (4 * 8 * 4, 4, 32)
    assert ops._wino_plan(a, _S2, y_small, True) == 4 * a.M * 256                                          # 32 x 4 slices = 128 units: the split form, its workspace
    stub.plan = (4 * 8 * 2, 2, 32)
    assert ops._wino_plan(a, _S2, y_small, True) is None                                                   # 64 units even when split
    monkeypatch.setattr(ops, "WINO_SPLITK", False)
    stub.plan, stub.asked = (4 * 8 * 4, 4, 32), []
    assert ops._wino_plan(a, _S2, y_small, True) is None and stub.asked == [0]                             # the lab switch: the library is asked for the whole-launch plan


def test_winograd_transpose_panel_and_algorithm_cpu():
    """The F(2x2, 2x2) Winograd form of ConvTranspose2d(4, 2, 1) (csrc/convt_winograd.hip) restated on the CPU around the REAL panel builder
    (ops._wwino_t, from the four parity GEMM panels): 25 transformed values per 4 x 4 input patch and channel (row / column forms r0-r1, r1, r2-r1, r2,
    r3-r2), product (xi, nu) of parity (py, px) = form (2 py + xi, 2 px + nu) x panel element 3 xi + nu (the sign of a shared form lives in the panel),
    Y[a][b] = the sum of the four products around (a, b) - equal to torch's transposed convolution on a ragged size; panel layout
    [4][Cin/8][4][2][9 N] ([N][4] products 0-3, [N][4] products 4-7, [N] product 8: every load of the kernel reads contiguous memory)."""
    torch.manual_seed(0)
    B, H, W, Cin, N = 1, 6, 5, 32, 64
    w, b, x = torch.randn(Cin, N, 4, 4) * 0.1, torch.randn(N) * 0.1, torch.randn(B, H, W, Cin)
    want = torch.nn.functional.conv_transpose2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=2, padding=1).permute(0, 2, 3, 1)
    specs = packing.pack_conv_transpose(w, b)
    assert ops._parity_specs_ok(specs) and not ops._parity_specs_ok(specs[::-1])
    U = ops._wwino_t(specs)
    assert U.shape == (4, Cin // 8, 4, 2, 9 * N) and U.dtype == torch.float32 and ops._wwino_t(specs) is U
    Uf = U.double().reshape(4, Cin, 9 * N)                                                  # [parity][c = 8 s + 2 kk + kh][ [N][4] | [N][4] | [N] ]
    Uc = torch.cat([Uf[..., :4 * N].reshape(4, Cin, N, 4).permute(0, 1, 3, 2), Uf[..., 4 * N:8 * N].reshape(4, Cin, N, 4).permute(0, 1, 3, 2),
                    Uf[..., 8 * N:].reshape(4, Cin, 1, N)], dim=2)                          # [parity][c][product 0..8][n]
    xp = torch.zeros(H + 4, W + 4, Cin, dtype=torch.float64)
    xp[1:H + 1, 1:W + 1] = x[0].double()                                                    # xp[r] = x[r - 1]: the patch of input rows i - 1 .. i + 2 is xp[i : i + 4]
    y = torch.zeros(2 * H, 2 * W, N, dtype=torch.float64)
    for i in range(0, H + 1, 2):
        for j in range(0, W + 1, 2):
            d = xp[i:i + 4, j:j + 4]
            t = torch.stack([d[0] - d[1], d[1], d[2] - d[1], d[2], d[3] - d[2]])
            V = torch.stack([t[:, 0] - t[:, 1], t[:, 1], t[:, 2] - t[:, 1], t[:, 2], t[:, 3] - t[:, 2]], dim=1)      # (5, 5, Cin)
            for par in range(4):
                py, px = par >> 1, par & 1
                M = torch.stack([torch.stack([V[2 * py + xi, 2 * px + nu] @ Uc[par, :, 3 * xi + nu] for nu in range(3)]) for xi in range(3)])
                for a_ in range(2):
                    for b_ in range(2):
                        if i + a_ < H and j + b_ < W:
                            y[2 * (i + a_) + py, 2 * (j + b_) + px] = M[a_, b_] + M[a_, b_ + 1] + M[a_ + 1, b_] + M[a_ + 1, b_ + 1] + b.double()
    assert (y - want[0]).abs().max().item() <= 1e-6 * max(1.0, want.abs().max().item())


def test_fused_transpose_dispatch_and_flow_cache(monkeypatch):
    """Host logic around two round-2 kernels (no GPU): ops.conv_transpose2d picks the one-launch form only for bf16 tensors with
    Cin <= 128 and the four parity specs in order, and hands the accounting hook ONE pseudo-spec for the whole transposed
    convolution; generator._Scratch.flow resizes the flows once per resolution and passes same-size fields through."""
    from ipercore_amd import _lib
    from ipercore_amd.networks import generator
    calls = []

    class _Stub:
        def lwg_conv_transpose4_nhwc_bf16(self, a, stream):
            calls.append(("fused", a.contents.ntaps if hasattr(a, "contents") else a.ntaps))
            return 0

        def lwg_conv_slice_count(self, a):
            return 1
    monkeypatch.setattr(_lib, "lib", lambda: _Stub())
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_ptr", lambda t, dt=None: 0 if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "conv2d", lambda x, s, y, act=0, **kw: calls.append(("parity", s.ooy, s.oox)))
    hooked = []
    infos = []
    monkeypatch.setattr(ops, "CONV_HOOK", lambda begin, M, spec, epi=0, info=None: (hooked.append((begin, M, spec.N, spec.ntaps, spec.algo_kn)), infos.append(info)))

    specs128 = packing.pack_conv_transpose(_w((128, 64, 4, 4), 20), torch.zeros(64))
    x = torch.zeros(1, 8, 16, 128, dtype=torch.bfloat16)
    y = torch.zeros(1, 16, 32, 64, dtype=torch.bfloat16)
    ops.conv_transpose2d(x, specs128, y, act=ops.ACT_RELU)
    assert calls == [("fused", 4)]
    assert hooked == [(True, 128, 256, 16, 4 * specs128[0].algo_kn), (False, 128, 256, 16, 4 * specs128[0].algo_kn)]
    assert infos == [None, {"kernels": 1, "kind": "up4"}]          # the closing call says what ran: launches behind the call, kernel family
    assert ops._w16up(specs128).shape == (4, 2 * 4, 4, 64, 16)                   # [parity][Cin/64 * taps][ks][N][16]

    calls.clear()
    specs256 = packing.pack_conv_transpose(_w((256, 128, 4, 4), 21), torch.zeros(128))
    ops.conv_transpose2d(torch.zeros(1, 8, 16, 256, dtype=torch.bfloat16), specs256, torch.zeros(1, 16, 32, 128, dtype=torch.bfloat16))
    assert calls == [("parity", 0, 0), ("parity", 0, 1), ("parity", 1, 0), ("parity", 1, 1)]      # Cin = 256: four launches
    calls.clear()
    ops.conv_transpose2d(torch.zeros(1, 8, 16, 128), specs128, torch.zeros(1, 16, 32, 64))         # fp32 tensors: four launches
    assert [c[0] for c in calls] == ["parity"] * 4

    resized = []
    monkeypatch.setattr(ops, "flow_resize", lambda T, h, w: resized.append((h, w)) or torch.zeros(T.shape[0], T.shape[1], h, w, 2))
    sc = generator._Scratch()
    T = torch.zeros(2, 2, 64, 64, 2)
    a = sc.flow(T, 16, 16)
    b = sc.flow(T, 16, 16)
    c = sc.flow(T, 32, 32)
    assert a is b and a.shape == (2, 2, 16, 16, 2) and c.shape == (2, 2, 32, 32, 2) and resized == [(16, 16), (32, 32)]
    assert sc.flow(T, 64, 64) is T and sc.flow(T, 16, 32) is T                # same size / non-square: passed through


@pytest.mark.parametrize("name,cin,n", [("_wwino_t", 32, 32), ("_wwino_t24", 32, 32), ("_w16up", 64, 64), ("_w32up", 64, 64)])
def test_parity_panels_follow_all_four_sources(name, cin, n):
    """A panel built from the four parity specs is cached on specs[0] but valid only while EVERY spec's ``w`` is the tensor it was built from:
    replacing specs[2].w gives a new panel, equal to the one fresh specs with those weights give; packing.spec_to leaves a correct panel."""
    build = getattr(ops, name)
    w, w2, b = _w((cin, n, 4, 4), 30), _w((cin, n, 4, 4), 31), _w((n,), 32)
    specs = packing.pack_conv_transpose(w, b)
    U = build(specs)
    assert build(specs) is U
    specs[2].w = packing.pack_conv_transpose(w2, b)[2].w
    assert specs[2].w.shape == specs[0].w.shape
    U2 = build(specs)
    fresh = packing.pack_conv_transpose(w, b)
    fresh[2] = packing.pack_conv_transpose(w2, b)[2]
    assert U2 is not U and not torch.equal(U2, U) and torch.equal(U2, build(fresh))
    assert build(specs) is U2
    for s in specs:
        packing.spec_to(s, s.w.device)
    assert torch.equal(build(specs), build(fresh))


def test_precision_mode_leaves_the_lab_switch_alone():
    """conv_precision selects the engine through its own flag: "winograd" inside "winograd2x2" runs the F(4x4, 3x3) kernel again, and the lab
    switch ops.WINO4 is neither written by a context nor restored by one."""
    spec64 = packing.pack_conv(torch.zeros(64, 64, 3, 3), None, stride=1, pad=1)
    prev = ops.WINO4
    try:
        assert ops.WINO4 and ops._wino4_use(spec64, False)
        with ops.conv_precision("winograd2x2"):
            assert ops.CONV_PRECISION == "winograd" and ops.WINO4 and not ops._wino4_use(spec64, False)
            with ops.conv_precision("winograd"):
                assert ops._wino4_use(spec64, False)
            assert not ops._wino4_use(spec64, False)
        assert ops._wino4_use(spec64, False)
        ops.WINO4 = False
        with ops.conv_precision("winograd"):
            assert not ops._wino4_use(spec64, False)
        assert ops.WINO4 is False
        with ops.conv_precision("winograd"):
            ops.WINO4 = True                             # a lab setting made inside a context survives the exit
        assert ops.WINO4 is True
        with ops.conv_precision("winograd2x2"):
            ops.WINO4 = False
        assert ops.WINO4 is False
    finally:
        ops.WINO4 = prev


def test_winograd_panel_and_eligibility():
    """ops._wwino: the fragment panel of lwg_conv2d_winograd_f32 holds U = G w G^T of every (input, output) channel pair at
    [xi * 4 + nu][c // 8][c % 2][n][(c % 8) // 2]; F(2x2, 3x3) evaluated with it in torch equals the convolution.  ops._wino_eligible: which
    launches the mode takes."""
    import torch.nn.functional as F
    from ipercore_amd import ops
    from ipercore_amd.networks import packing
    g = torch.Generator().manual_seed(3)
    N, Cin = 64, 32
    w, b = torch.randn(N, Cin, 3, 3, generator=g) * 0.1, torch.randn(N, generator=g)
    spec = packing.pack_conv(w, b, stride=1, pad=1)
    from tests import emu_ops
    Upk = emu_ops.winograd_panel(spec)               # the contract of lwg_winograd_panel_f32 (the GPU suite holds the kernel against it)
    assert tuple(Upk.shape) == (16, Cin // 8, 2, N, 4) and Upk.dtype == torch.float32
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops._wwino(spec)
    U = Upk.permute(0, 1, 4, 2, 3).reshape(16, Cin, N)                       # [p][c = 8 s + 2 kk + kh][n]
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
    assert torch.allclose(U, torch.einsum("ij,ncjk,lk->ilcn", G, w, G).reshape(16, Cin, N), atol=1e-7)
    # the whole algorithm with this U on one image: V = B^T d B, M = sum_c U V, Y = A^T M A
    BT = torch.tensor([[1., 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]])
    AT = torch.tensor([[1., 1, 1, 0], [0, 1, -1, -1]])
    x = torch.randn(1, 10, 14, Cin, generator=g)
    t = F.pad(x.permute(0, 3, 1, 2), [1, 1, 1, 1]).unfold(2, 4, 2).unfold(3, 4, 2)            # (1,C,th,tw,4,4)
    V = torch.einsum("ij,ncthjk,lk->ncthil", BT, t, BT)
    M = torch.einsum("ilco,ncthil->nothil", U.view(4, 4, Cin, N), V)
    Y = torch.einsum("pi,nothil,ql->nothpq", AT, M, AT)
    y = Y.permute(0, 1, 2, 4, 3, 5).reshape(1, N, 10, 14) + b.view(1, -1, 1, 1)
    want = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1)
    assert torch.allclose(y, want, atol=2e-5), float((y - want).abs().max())
    # eligibility
    x0, yy = torch.zeros(1, 8, 8, Cin), torch.zeros(1, 8, 8, N)
    ok = lambda **k: ops._wino_eligible(k.get("spec", spec), k.get("x0", x0), k.get("y", yy), k.get("x1"), k.get("epi", ops.EPI_NONE),
                                        k.get("act", ops.ACT_RELU), k.get("out_hw"), k.get("q4", False), k.get("ycoff", 0))
    assert ok() and ok(epi=ops.EPI_RESIDUAL) and not ok(q4=True) and not ok(act=ops.ACT_RELU_MASK)
    assert not ok(spec=packing.pack_conv(w, b, stride=2, pad=1)) and not ok(spec=packing.pack_conv(w[:, :, 1:2, 1:2].contiguous(), b, stride=1, pad=0))
    assert not ok(y=torch.zeros(1, 8, 8, N, dtype=torch.bfloat16))
    sp2 = packing.pack_conv(torch.randn(N, 96, 3, 3, generator=g), b, stride=1, pad=1)
    assert ok(spec=sp2, x0=torch.zeros(1, 8, 8, 64), x1=torch.zeros(1, 8, 8, 32))
    assert ok(spec=spec, y=torch.zeros(1, 8, 8, N // 2), epi=ops.EPI_SPADE) and not ok(spec=spec, epi=ops.EPI_SPADE)


def test_winograd4_panel_algorithm_and_rule():
    """csrc/conv_winograd4.hip (F(4x4, 3x3)) on the CPU: the fragment panel's contract (tests/emu_ops.winograd4_panel: U = G w G^T, products dealt to the four
    wave sets as (row q) + (three products of row 4 + q // 2), nine floats per (column, block) in three contiguous parts), the algorithm restated around that panel
    exactly as the kernel folds it (whole rows, half rows as three partial sums, the bias as the start value of product (1, 1)) equals the convolution on
    ragged sizes, and ops._wino4_use is a rule on the LAYER only (never on the batch: batch invariance)."""
    import torch.nn.functional as F
    from ipercore_amd import ops
    from ipercore_amd.networks import packing
    from tests import emu_ops
    g = torch.Generator().manual_seed(5)
    N, Cin = 64, 32
    w, b = torch.randn(N, Cin, 3, 3, generator=g) * 0.1, torch.randn(N, generator=g)
    spec = packing.pack_conv(w, b, stride=1, pad=1)
    Upk = emu_ops.winograd4_panel(spec)
    assert tuple(Upk.shape) == (4, Cin // 8, 4, 2, 9 * N) and Upk.dtype == torch.float32
    prod = emu_ops.winograd4_panel_products(Upk)                               # [q][j][c][n]
    G = torch.tensor(emu_ops.W4_G, dtype=torch.float64)
    U = torch.einsum("ij,ncjk,lk->ilcn", G, w.double(), G)                    # [xi][nu][c][n]
    seen = set()
    for q in range(4):
        for j in range(9):
            xi, nu = emu_ops.winograd4_product(q, j)
            seen.add((xi, nu))
            assert torch.allclose(prod[q, j].double(), U[xi, nu], atol=1e-7), (q, j)
            blk = Upk[q, 1, 2, 1]                                                 # the block of input channel c = 8 + 4 + 1: [N][4] | [N][4] | [N]
            where = blk[(j // 4) * 4 * N + (j % 4):(j // 4 + 1) * 4 * N:4] if j < 8 else blk[8 * N:]
            assert torch.equal(where, prod[q, j, 13]), (q, j)
    assert len(seen) == 36                                                    # every product of the 6 x 6 patch exactly once
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops._wwino4(spec)
    for (B, H, W) in ((1, 10, 14), (2, 5, 33), (1, 1, 7)):
        x = torch.randn(B, H, W, Cin, generator=g)
        y = emu_ops.winograd4_conv(x, Upk, b)
        want = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
        assert tuple(y.shape) == tuple(want.shape)
        assert float((y - want).abs().max()) <= 2e-5, float((y - want).abs().max())      # (the panel is rounded to fp32 once)
    # the rule: the layer's Cin, never the batch; training launches (splitk) keep the F(2x2, 3x3) kernel and its split plan
    assert ops.WINO4 and ops._wino4_use(packing.pack_conv(torch.zeros(64, ops.WINO4_MIN_CIN, 3, 3), None, stride=1, pad=1), False)
    assert not ops._wino4_use(spec, True)
    if ops.WINO4_MIN_CIN > 32:
        assert not ops._wino4_use(spec, False)


def test_convt_exchange_slots():
    """csrc/convt_winograd.hip ctw_slot: the pixel-slot permutation of the transposed Winograd kernel's exchange buffer (rows of 32 slots x 36 floats) is a
    bijection; the eight consecutive lanes of a ds_write_b128 (patches etx = 0..7, pixel 4 etx + r) hit eight distinct bank quads (banks mod 32), and the
    sixteen lanes of either ds_read_b128 lane group of the channel-quad-plane reader (32 consecutive pixels, banks mod 64; MI355X_MICROARCH.md, LDS)
    sixteen distinct ones.  The same enumeration for the epilogue reader map of csrc/conv_winograd4.hip (LWG_W4_RDMAP: rows of 68 floats)."""
    slot = lambda lx: 8 * (lx & 3) + (((lx >> 2) + 2 * (lx & 3)) & 7)      # noqa: E731
    assert sorted(slot(lx) for lx in range(32)) == list(range(32))
    orow = 36
    for r in range(4):
        for qd in range(8):                                   # a lane's 16-byte piece: channel quad qd of its pixel
            quads = {((slot(4 * etx + r) * orow + 4 * qd) // 4) % 8 for etx in range(8)}
            assert len(quads) == 8, (r, qd, quads)
            lin = {(((4 * etx + r) * orow + 4 * qd) // 4) % 8 for etx in range(8)}
            assert len(lin) == 2                              # what the linear order did: four-way conflicts
    groups = ([0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31])
    for grp in groups:
        for cq in range(8):
            quads = {((slot(lx) * orow + 4 * cq) // 4) % 16 for lx in grp}
            assert len(quads) == 16, (cq, quads)
    # conv_winograd4.hip: reader lane -> (patch, quad) through the lane groups; a slot of the 68-float rows lies in bank quad (17 patch + quad) % 16
    amask = 0x0FF0F00F
    for half in range(2):
        for first in (True, False):
            lanes = [l for l in range(32) if bool((amask >> l) & 1) == first]
            seen = set()
            for l5 in lanes:
                gm = amask if first else (~amask & 0xFFFFFFFF)
                gidx = bin(gm & ((1 << l5) - 1)).count("1")
                patch = 2 * half + (0 if first else 1) + 8 * (gidx >> 3)
                quad = gidx & 7
                seen.add((17 * patch + quad) % 16)
            assert len(seen) == 16, (half, first, seen)
