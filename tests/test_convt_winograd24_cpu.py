"""CPU checks of the F(2x4, 2x2) transposed-convolution kernel (csrc/convt_winograd24.hip): the algorithm restated around the real panel builder
(ops._wwino_t24) against torch, the product -> wave map, the exchange-buffer slot map, and the host dispatch (no GPU)."""
import torch

from ipercore_amd import ops
from ipercore_amd.networks import packing


def _cols(c):
    """The kernel's nine column forms of six staged columns (ctw24_cols: B^T on c0..c4 and c1..c5, C4 shared)."""
    return torch.stack([c[0] - 2 * c[1] - c[2] + 2 * c[3], -c[1] + c[2] + 2 * c[3], c[1] - 3 * c[2] + 2 * c[3], c[3] - c[1],
                        c[1] - 2 * c[2] - c[3] + 2 * c[4], -c[2] + c[3] + 2 * c[4], c[2] - 3 * c[3] + 2 * c[4], c[4] - c[2],
                        c[2] - 2 * c[3] - c[4] + 2 * c[5]])


def _panel_products(U, Cin, N):
    """Upk[4][Cin/8][4][2][15 N] -> [parity][c][product 0..14][n] (layout of include/lwg_hip.h)."""
    Uf = U.double().reshape(4, Cin, 15 * N)
    q4 = lambda lo: Uf[..., lo * N:(lo + 4) * N].reshape(4, Cin, N, 4).permute(0, 1, 3, 2)      # noqa: E731
    return torch.cat([q4(0), q4(4), Uf[..., 8 * N:9 * N].reshape(4, Cin, 1, N), q4(9), Uf[..., 13 * N:15 * N].reshape(4, Cin, 2, N)], dim=2)


def _product(xi, nu):
    """Panel index of product (xi, nu): h = 0 owns nu = 0..2 (3 xi + nu), h = 1 owns nu = 3, 4 (9 + 2 xi + nu - 3)."""
    return 3 * xi + nu if nu < 3 else 9 + 2 * xi + nu - 3


def _restated(x, specs, bias):
    B, H, W, Cin = x.shape
    N = specs[0].N
    U = ops._wwino_t24(specs)
    assert U.shape == (4, Cin // 8, 4, 2, 15 * N) and U.dtype == torch.float32 and ops._wwino_t24(specs) is U
    Uc = _panel_products(U, Cin, N)
    y = torch.zeros(B, 2 * H, 2 * W, N, dtype=torch.float64)
    for bb in range(B):
        xp = torch.zeros(H + 4, W + 6, Cin, dtype=torch.float64)
        xp[1:H + 1, 1:W + 1] = x[bb].double()                      # xp[r] = x[r - 1]: the patch at (i, j) stages xp[i : i + 4, j : j + 6]
        for i in range(0, H, 2):
            for j in range(0, W, 4):
                d = xp[i:i + 4, j:j + 6]
                R = torch.stack([d[0] - d[1], d[1], d[2] - d[1], d[2], d[3] - d[2]])          # (5, 6, Cin)
                V = torch.stack([_cols(R[f].unbind(0)) for f in range(5)])                    # (5, 9, Cin): 45 values per channel
                for par in range(4):
                    py, px = par >> 1, par & 1
                    M = [[V[2 * py + xi, 4 * px + nu] @ Uc[par, :, _product(xi, nu)] for nu in range(5)] for xi in range(3)]
                    for ia in range(2):
                        S = [M[ia][nu] + M[ia + 1][nu] for nu in range(5)]
                        p0 = [S[0] + S[1] + S[2], S[1] - S[2], S[1] + S[2], S[1] - S[2]]      # h = 0's partials
                        p1 = [S[3], S[3] / 2, S[3] / 4, S[3] / 8 + S[4]]                      # h = 1's (through the exchange buffer)
                        for ib in range(4):
                            if i + ia < H and j + ib < W:
                                y[bb, 2 * (i + ia) + py, 2 * (j + ib) + px] = p0[ib] + p1[ib] + bias.double()
    return y


def test_winograd24_panel_and_algorithm_cpu():
    """F(2x4, 2x2): 45 transformed values per 2 x 4 input patch and channel serve 60 products; restated in fp64 around the real fp32 panel it is
    torch's transposed convolution on ragged, odd and tiny sizes, both parities of each dimension, several images."""
    torch.manual_seed(0)
    for (B, H, W, Cin, N) in ((1, 6, 5, 32, 32), (2, 3, 7, 32, 64), (1, 1, 1, 32, 32), (1, 4, 8, 64, 32)):
        w, b, x = torch.randn(Cin, N, 4, 4) * 0.1, torch.randn(N) * 0.1, torch.randn(B, H, W, Cin)
        want = torch.nn.functional.conv_transpose2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=2, padding=1).permute(0, 2, 3, 1)
        specs = packing.pack_conv_transpose(w, b)
        y = _restated(x, specs, b)
        assert (y - want).abs().max().item() <= 2e-6 * max(1.0, want.abs().max().item()), (B, H, W, Cin, N)


def test_winograd24_transforms_exact():
    """The transform matrices: A^T [(G_x g) * (B^T d)] is the 2-tap correlation of 5 inputs for any d, g (fp64, exact up to rounding)."""
    Gx = torch.tensor(ops._G_X24, dtype=torch.float64)
    AT = torch.tensor([[1, 1, 1, 1, 0], [0, 1, -1, 0.5, 0], [0, 1, 1, 0.25, 0], [0, 1, -1, 0.125, 1]], dtype=torch.float64)
    torch.manual_seed(1)
    for _ in range(4):
        d, g = torch.randn(6, dtype=torch.float64), torch.randn(2, dtype=torch.float64)
        V = _cols(d.unbind(0))
        for px in range(2):
            want = torch.stack([d[px + i] * g[0] + d[px + i + 1] * g[1] for i in range(4)])
            got = AT @ ((Gx @ g) * V[4 * px:4 * px + 5])
            assert (got - want).abs().max().item() < 1e-12


def test_winograd24_product_wave_map():
    """Wave w: parity w % 4, half w / 4; h = 0 owns (xi, nu < 3), h = 1 (xi, nu >= 3).  Every product of every parity is owned exactly once, each
    SIMD (waves p and p + 4) executes 15 per k-pair, and a wave's fragment forms (2 py + xi, 4 px + nu) lie inside the 5 x 9 forms."""
    seen = {}
    for w in range(8):
        par, h = w % 4, w // 4
        py, px = par >> 1, par & 1
        nus = (0, 1, 2) if h == 0 else (3, 4)
        for q in range(9 if h == 0 else 6):                   # the kernel's local product index: xi = q / NU, nu' = q % NU
            nu_l = 3 if h == 0 else 2
            xi, nu = q // nu_l, nus[q % nu_l]
            assert _product(xi, nu) == (q if h == 0 else 9 + q)
            form = 9 * (2 * py + xi) + 4 * px + 3 * h + q % nu_l
            assert 0 <= form < 45 and form == 9 * (2 * py + xi) + 4 * px + nu
            seen[(par, xi, nu)] = seen.get((par, xi, nu), 0) + 1
    assert len(seen) == 60 and set(seen.values()) == {1}
    for simd in range(4):
        assert sum(1 for (par, _, _) in seen if par == simd) == 15


def _slot(ly, lx):
    return ((lx & 7) * 4 + (lx >> 3)) ^ (((ly >> 2) & 1) << 2)


def test_winograd24_formulas_are_the_kernels():
    """The index formulas the two tests below enumerate, read out of csrc/convt_winograd24.hip itself (so that they check the HIP source, not only
    a Python copy): the slot map, the fragment offsets (form 9 (2 py + xi) + 4 px + 3 h + nu') and the panel products of a wave (3 / 2 per row)."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ipercore_amd", "csrc", "convt_winograd24.hip")).read()
    body = re.search(r"int ctw24_slot\(int ly, int lx\) \{\s*return (.*?);\s*\}", src, re.S).group(1)
    for ly in range(32):
        for lx in range(32):
            assert eval(body, {"ly": ly, "lx": lx}) == _slot(ly, lx)
    assert "(18 * py + 4 * px + 3 * hh) * KS * VSTR + (lane >> 5) * VSTR + (lane & 31)" in src
    assert "smem[fbs[buf] + ((9 * (q / NU) + q % NU) * KS + 2 * kk) * VSTR]" in src
    assert "constexpr int NU = HV ? 2 : 3;" in src and "constexpr int NP = HV ? 6 : 9;" in src


def test_winograd24_exchange_slots():
    """ctw24_slot: a bijection of the 32 pixel slots of every row; the eight consecutive lanes of an epilogue ds_write_b128 (patches etx = 0..3 of
    patch rows 2 m, 2 m + 1) hit eight distinct bank quads (banks mod 32); the sixteen lanes of either ds_read_b128 lane group of the
    channel-quad-plane reader sixteen distinct ones (banks mod 64) - the enumeration of tests/test_bf16_panels.py::test_convt_exchange_slots."""
    orow = 36
    for ly in range(32):
        assert sorted(_slot(ly, lx) for lx in range(32)) == list(range(32))
    for ia in range(2):
        for py in range(2):
            for r in range(8):                                # r = 2 ib + px
                for m in range(4):
                    for chq in range(8):
                        quads = set()
                        for lane in range(8 * m, 8 * m + 8):
                            ety, etx = lane >> 2, lane & 3
                            ly, lx = 4 * ety + 2 * ia + py, 8 * etx + r
                            quads.add(((ly * 32 + _slot(ly, lx)) * orow + 4 * chq) // 4 % 8)
                        assert len(quads) == 8, (ia, py, r, m, quads)
    groups = ([0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31])
    for ly in range(32):
        for grp in groups:
            for cq in range(8):
                quads = {((ly * 32 + _slot(ly, lx)) * orow + 4 * cq) // 4 % 16 for lx in grp}
                assert len(quads) == 16, (ly, cq, quads)


def test_winograd24_dispatch(monkeypatch):
    """The "winograd" mode's synthesis path: images of >= WINO_UP4_24_MIN_HW input pixels take lwg_conv_transpose4_winograd24_f32 with the 15 N
    panel, smaller ones lwg_conv_transpose4_winograd_f32 with the 9 N panel; the lab switch turns the new kernel off; the hook kind stays
    "winograd_up4"; training callers (splitk=True) never reach either."""
    from ipercore_amd import _lib
    calls = []

    class _Stub:
        def lwg_conv_transpose4_winograd24_f32(self, a, stream):
            calls.append("f24")
            return 0

        def lwg_conv_transpose4_winograd_f32(self, a, stream):
            calls.append("f22")
            return 0
    monkeypatch.setattr(_lib, "lib", lambda: _Stub())
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_ptr", lambda t, dt=None: 0 if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "conv_args", lambda x, s, y, **kw: type("A", (), {"M": x.shape[0] * x.shape[1] * x.shape[2]})())

    class _Cuda(torch.Tensor):
        @property
        def is_cuda(self):
            return True
    torch.manual_seed(2)
    specs = packing.pack_conv_transpose(torch.randn(32, 32, 4, 4) * 0.1, torch.zeros(32))
    kinds = []
    monkeypatch.setattr(ops, "CONV_HOOK", lambda begin, M, spec, epi=0, info=None: kinds.append(info["kind"]) if not begin else None)
    monkeypatch.setattr(ops, "_hook_end", lambda a, whole, epi, kind, *r: ops.CONV_HOOK(False, a.M, whole, epi, {"kind": kind}))
    with ops.conv_precision("winograd"):
        for hw, want in ((64, "f24"), (32, "f22")):
            x = torch.zeros(1, hw, hw, 32).as_subclass(_Cuda)
            y = torch.zeros(1, 2 * hw, 2 * hw, 32)
            ops.conv_transpose2d(x, specs, y)
            assert calls[-1] == want and kinds[-1] == "winograd_up4", (hw, calls, kinds)
        monkeypatch.setattr(ops, "WINO_UP4_24", False)
        ops.conv_transpose2d(torch.zeros(1, 64, 64, 32).as_subclass(_Cuda), specs, torch.zeros(1, 128, 128, 32))
        assert calls[-1] == "f22"
    assert ops._wwino_t24(specs).shape == (4, 4, 4, 2, 15 * 32) and ops._wwino_t(specs).shape == (4, 4, 4, 2, 9 * 32)
