"""The "bf16_winograd" precision mode without a GPU: the algorithm at its documented rounding points (a torch emulation against fp64, beside the
direct bf16 form), the fragment panel ops._wwino16 builds (every element read back through the documented index formula), and the mode plumbing."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ipercore_amd import _lib, ops
from ipercore_amd.networks import packing
from tests.bf16wino_emu import G, RATIO_BOUND, adversarial_ratios, emulate_winograd, r16


def test_emulation_is_a_convolution():
    """The emulation computes the convolution: on small-integer operands every intermediate is exact, so it must equal fp64 bit for bit."""
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-3, 4, (2, 5, 7, 64), generator=g).float()
    w = torch.randint(-2, 3, (64, 64, 3, 3), generator=g).float() * 4            # G w G^T of multiples of 4 is integral
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1)
    got = emulate_winograd(x, w)
    assert torch.equal(got.double(), r16(ref.float()).double())


def test_algorithm_and_rounding_points():
    ratios = adversarial_ratios()
    for case, (ew, ed, ratio) in ratios.items():
        print(f"{case}: winograd {ew:.3e} direct {ed:.3e} ratio {ratio:.2f}")
    worst = max(ratios.items(), key=lambda kv: kv[1][2])
    assert all(np.isfinite(v[0]) and v[1] > 0 for v in ratios.values())
    assert worst[1][2] <= RATIO_BOUND, worst


def _spec(cin, n, seed, spade=False):
    g = torch.Generator().manual_seed(seed)
    if spade:
        c = n // 2
        wg, wb = torch.randn(c, cin, 3, 3, generator=g), torch.randn(c, cin, 3, 3, generator=g)
        bg, bb = torch.randn(c, generator=g), torch.randn(c, generator=g)
        return packing.pack_spade_gamma_beta(wg, bg, wb, bb), (wg, bg, wb, bb)
    w, b = torch.randn(n, cin, 3, 3, generator=g), torch.randn(n, generator=g)
    return packing.pack_conv(w, b, stride=1), (w, b)


@pytest.mark.parametrize("cin,n", [(64, 64), (128, 256), (384, 64), (64, 256)])
def test_panel_layout(cin, n):
    spec, (w, b) = _spec(cin, n, 7 + cin + n)
    panel, bias = ops._wwino16(spec, False)
    assert panel.dtype == torch.bfloat16 and tuple(panel.shape) == (cin // 16, 16, n, 16) and panel.is_contiguous()
    assert torch.equal(bias, b)
    want = torch.einsum("ar,ncrs,bs->abcn", G, w.double(), G).to(torch.bfloat16)                 # (xi, nu, c, n)
    flat = panel.reshape(-1)
    ks, p, nn, e = torch.meshgrid(torch.arange(cin // 16), torch.arange(16), torch.arange(n), torch.arange(16), indexing="ij")
    got = flat[ops.wwino16_index(ks, p, nn, e, n)]                                               # EVERY element through the documented formula
    assert torch.equal(got, want[p // 4, p % 4, 16 * ks + e, nn])
    assert ops._wwino16(spec, False)[0] is panel                                                 # cached
    assert set(spec._panels) == {("wwino16", False)}                                             # this panel and no other engine's


def test_panel_spade_interleave():
    cin, n = 128, 128
    spec, (wg, bg, wb, bb) = _spec(cin, n, 99, spade=True)
    panel, bias = ops._wwino16(spec, True)
    ug = torch.einsum("ar,ncrs,bs->abcn", G, wg.double(), G).to(torch.bfloat16)
    ub = torch.einsum("ar,ncrs,bs->abcn", G, wb.double(), G).to(torch.bfloat16)
    for j in range(n):
        ch, beta = ops.wwino16_spade_column(j)
        assert (ch, beta) == (4 * (j // 8) + j % 4, (j % 8) // 4)
        src = ub if beta else ug
        col = panel[:, :, j, :]                                                                  # (ks, p, e)
        want = src[:, :, :, ch].reshape(16, cin // 16, 16).permute(1, 0, 2)
        assert torch.equal(col, want), j
        assert bias[j] == (bb if beta else bg)[ch]
    assert ops._wwino16(spec, True)[0] is panel
    plain, _ = ops._wwino16(spec, False)                                                         # the other key: its own panel
    assert plain is not panel and not torch.equal(plain, panel)
    assert ops._wwino16(spec, True)[0] is panel and ops._wwino16(spec, False)[0] is plain        # the variants coexist on the spec
    hr, hr_bias = ops._w16hr(spec, True)
    hr_plain, _ = ops._w16hr(spec, False)
    assert hr_plain is not hr and not torch.equal(hr_plain, hr)
    assert ops._w16hr(spec, True)[0] is hr and ops._w16hr(spec, True)[1] is hr_bias and ops._w16hr(spec, False)[0] is hr_plain


def test_mode_plumbing():
    prev = ops.CONV_PRECISION
    with ops.conv_precision("bf16_winograd"):
        assert ops.CONV_PRECISION == "bf16_winograd"
    assert ops.CONV_PRECISION == prev
    with pytest.raises(AssertionError):
        ops.conv_precision("bf16_winograd4")

    class _G:
        conv_precision = "bf16_winograd"
    from ipercore_amd.networks import generator
    cls = [c for c in vars(generator).values() if isinstance(c, type) and hasattr(c, "_act_dtype")]
    assert cls
    for c in cls:
        assert c._act_dtype(_G()) is torch.bfloat16
        _G.conv_precision = "bf16"
        assert c._act_dtype(_G()) is torch.bfloat16
        _G.conv_precision = "winograd"
        assert c._act_dtype(_G()) is torch.float32
        _G.conv_precision = "bf16_winograd"
    assert "lwg_conv2d_winograd_bf16" in _lib.header_symbols()
    assert "lwg_conv2d_winograd_bf16" in _lib._SIGS
    with open(_lib.HEADER_PATH) as fp:
        assert "#define LWG_ABI_VERSION 10" in fp.read()
    if os.path.exists(_lib.LIB_PATH):
        handle = ctypes.CDLL(_lib.LIB_PATH)
        assert hasattr(handle, "lwg_conv2d_winograd_bf16")
        handle.lwg_abi_version.restype = ctypes.c_int
        assert handle.lwg_abi_version() == 10


def test_eligibility_is_a_layer_rule():
    """_bf16_wino_eligible looks at the layer (taps, Cin, N, epilogue) and never at the batch."""
    spec, _ = _spec(64, 64, 3)
    for b in (1, 7):
        x = torch.empty(b, 9, 11, 64, dtype=torch.bfloat16)
        y = torch.empty(b, 9, 11, 64, dtype=torch.bfloat16)
        assert ops._bf16_wino_eligible(spec, x, y, None, ops.EPI_NONE, ops.ACT_RELU, None)
        assert not ops._bf16_wino_eligible(spec, x, y, None, ops.EPI_NONE, ops.ACT_LRELU, None)
    prev = ops.BF16_WINO_MIN_CIN
    try:
        ops.BF16_WINO_MIN_CIN = 128
        assert not ops._bf16_wino_eligible(spec, x, y, None, ops.EPI_NONE, ops.ACT_RELU, None)
    finally:
        ops.BF16_WINO_MIN_CIN = prev
    s2 = packing.pack_conv(torch.randn(64, 64, 3, 3), None, stride=2)
    assert not ops._bf16_wino_eligible(s2, x, torch.empty(7, 5, 6, 64, dtype=torch.bfloat16), None, ops.EPI_NONE, ops.ACT_NONE, None)
    s1 = packing.pack_conv(torch.randn(64, 64, 1, 1), None, stride=1)
    assert not ops._bf16_wino_eligible(s1, x, y, None, ops.EPI_NONE, ops.ACT_NONE, None)
