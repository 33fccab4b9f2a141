"""Lab: wave -> SIMD placement and per-phase cycles of the two fp32 transposed-convolution Winograd kernels on the decoder's three layer shapes.
Every wave of a workgroup's second block stamps its hardware id and s_memtime (a -DLWG_CTW24_TS build of csrc/convt_winograd24.hip, a -DLWG_CTW_TS
build of csrc/convt_winograd.hip, both from tools/labbuild.sh):
    tools/labbuild.sh convt_winograd24.hip ct24ts -DLWG_CTW24_TS && tools/labbuild.sh convt_winograd.hip ct22ts -DLWG_CTW_TS
    python tools/up4ts24.py tools/lab/ct24ts.so tools/lab/ct22ts.so"""
import collections
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from ipercore_amd import _lib, ops  # noqa: E402
from ipercore_amd.networks import packing  # noqa: E402

dev = "cuda:0"
l24, l22 = ctypes.CDLL(os.path.abspath(sys.argv[1])), ctypes.CDLL(os.path.abspath(sys.argv[2]))
for f in (l24.lwg_conv_transpose4_winograd24_f32, l22.lwg_conv_transpose4_winograd_f32):
    f.argtypes, f.restype = [ctypes.POINTER(_lib.LwgConvArgs), ctypes.c_void_p], ctypes.c_int
cus = torch.cuda.get_device_properties(0).multi_processor_count
g = torch.Generator().manual_seed(7)
for name, B, H, Cin, N in (("up0", 16, 64, 256, 256), ("up1", 4, 128, 256, 128), ("up2", 2, 256, 128, 64)):
    w = torch.randn(Cin, N, 4, 4, generator=g) * (Cin * 4) ** -0.5
    specs = [packing.spec_to(s, dev) for s in packing.pack_conv_transpose(w, 0.1 * torch.randn(N, generator=g))]
    x = torch.randn(B, H, H, Cin, generator=g).to(dev)
    y = torch.empty(B, 2 * H, 2 * H, N, device=dev)
    nst = Cin // 8
    for tag, lib, fn, panel, words, st in (("F(2x4,2x2)", l24, "lwg_conv_transpose4_winograd24_f32", ops._wwino_t24(specs), 8, (1, 2, 3, 4)),
                                            ("F(2x2,2x2)", l22, "lwg_conv_transpose4_winograd_f32", ops._wwino_t(specs), 16, (4, 5, 6, 13))):
        a = ops.conv_args(x, specs[0], y, act=ops.ACT_RELU)
        a.w = ops._ptr(panel)
        ts = torch.zeros(cus * 8 * words, dtype=torch.int64, device=dev)
        a.res = ts.data_ptr()
        for _ in range(3):
            assert getattr(lib, fn)(ctypes.byref(a), None) == 0
        torch.cuda.synchronize()
        t = ts.cpu().numpy().reshape(cus, 8, words).astype(np.float64)
        ok = t[:, :, st[0]] > 0
        kl = (t[:, :, st[1]] - t[:, :, st[0]])[ok] / nst
        ep = (t[:, :, st[3]] - t[:, :, st[1]])[ok]
        line = f"{name} {tag}: K loop {np.median(kl):7.0f} cycles per stage (p90 {np.percentile(kl, 90):7.0f}), block after the K loop {np.median(ep):7.0f}"
        if words == 8:
            hw = ts.cpu().numpy().reshape(cus, 8, words)[:, :, 0]
            simd = (hw >> 4) & 3
            pats = collections.Counter(tuple(int(v) for v in simd[i]) for i in range(cus) if ok[i].all())
            xc = (t[:, :, 3] - t[:, :, 2])[ok]
            line += f" (partial exchange {np.median(xc):6.0f});  SIMD of waves 0..7: " + ", ".join(f"{k} x{v}" for k, v in pats.most_common(4))
        print(line, flush=True)
