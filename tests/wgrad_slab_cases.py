"""Fixed cases of the weight-gradient family (csrc/lwg_wgrad_slab.h) and the two recorders of what the library makes of them, shared by
tests/test_wgrad_slab_cpu.py and tests/test_gpu_wgrad_slab.py.

``plans()``: the split plans of a fixed shape grid through the library's host-only queries (lwg_conv2d_wgrad_ws_floats, _bf16_ws_floats,
_winograd_ws_floats: they read the launch description, never a pointer's target, and need no GPU; without one the CU count falls back to 256,
the MI355X's).  ``gpu()``: seeded inputs through the five entry points, per case a sha256 of the dw bytes and of the db bytes plus the kernel
forms the case reaches.  The module calls the C ABI directly and knows nothing of the header, so it runs unchanged on a tree that does not have it:
    python -m tests.wgrad_slab_cases plans tests/golden/wgrad_plans_parent.json
    python -m tests.wgrad_slab_cases gpu   tests/golden/wgrad_slab_parent.json
in an export of the parent commit with this file copied in is how the two goldens were written, once."""
import ctypes
import hashlib
import json
import sys

from ipercore_amd import _lib

T3 = [(t // 3 - 1, t % 3 - 1) for t in range(9)]
CT_TAPS = {0: [(1, 0), (3, -1)], 1: [(0, 1), (2, 0)]}                # networks.packing._CT_TAPS: output parity -> [(kernel index, input offset)]
PARITY_TAPS = [(dy, dx) for _, dy in CT_TAPS[1] for _, dx in CT_TAPS[0]]                 # the (py, px) = (1, 0) launch of a ConvTranspose2d(4, 2, 1)
PARITY_KIDX = [ky * 4 + kx for ky, _ in CT_TAPS[1] for kx, _ in CT_TAPS[0]]
ADJ = [((py - 2 * ey, px - 2 * ex), ky * 4 + kx) for py in (0, 1) for px in (0, 1) for ky, ey in CT_TAPS[py] for kx, ex in CT_TAPS[px]]
ADJ_TAPS, ADJ_KIDX = [t for t, _ in ADJ], [i for _, i in ADJ]      # pack_dgrad_conv_transpose's 16-tap order


def taps_of(k):
    return [(t // k - k // 2, t % k - k // 2) for t in range(k * k)]


def conv_args(B, H, W, C0, C1, N, taps, stride=1, OH=None, OW=None, omul=1, ooy=0, oox=0, x0=1, x1=None, YC=None):
    """The launch description of one weight gradient; pointers are integers (1 = a stand-in for the host-only queries)."""
    OH, OW = OH or H, OW or W
    a = _lib.LwgConvArgs()
    a.x0, a.x1 = x0, (x1 if C1 else None)
    a.C0, a.C1, a.B, a.H, a.W = C0, C1, B, H, W
    a.OH, a.OW, a.M = OH, OW, B * OH * OW
    Cin = C0 + C1
    a.stride, a.ntaps, a.cshift = stride, len(taps), (0 if Cin % 32 == 0 else (Cin // 4).bit_length() - 1)
    a.N, a.YH, a.YW, a.YC, a.ycoff = N, OH * omul, OW * omul, YC or N, 0
    a.omul, a.ooy, a.oox = omul, ooy, oox
    a.xdt = a.ydt = _lib.DT_F32
    for t, (dy, dx) in enumerate(taps):
        a.dy[t], a.dx[t] = dy, dx
    return a


# ---------------------------------------------------------------------------------------------------------------- the split plans
def plan_grid():
    """(S, div, B, ntaps, Cin, N): the weight gradients of a step at S x S - resolutions S / div, 1 - 3 images per launch, the 1x1 / parity / 3x3 /
    4x4 / 5x5 / 7x7 tap counts, the small-Cin first layers up to the 512-channel concatenations and discriminator layers."""
    return [(S, div, B, nt, C, N) for S in (256, 512) for div in (1, 2, 4, 8, 16, 32) for B in (1, 2, 3) for nt in (1, 4, 9, 16, 25, 49)
            for C in (4, 8, 64, 128, 256, 512) for N in (4, 64, 128, 192, 256, 512)]


def plans():
    """-> {"grid": [...], "direct": [splits], "bf16": [splits or -1 outside its contract], "winograd": [...]}; splits = ws_floats / slab floats."""
    L = _lib.lib()
    out = {"direct": [], "bf16": [], "winograd": []}
    for S, div, B, nt, C, N in plan_grid():
        H = S // div
        Ktot, M = nt * C, B * H * H
        ws = L.lwg_conv2d_wgrad_ws_floats(Ktot, N, M)
        assert ws % ((Ktot + 1) * N) == 0
        out["direct"].append(ws // ((Ktot + 1) * N))
        k = {1: 1, 9: 3, 25: 5, 49: 7}.get(nt)
        taps = taps_of(k) if k else (ADJ_TAPS if nt == 16 else PARITY_TAPS)
        a = conv_args(B, H, H, C, 0, N, taps)
        ws = L.lwg_conv2d_wgrad_bf16_ws_floats(ctypes.byref(a))
        assert ws % ((Ktot + 1) * N) == 0 and (ws > 0) == (C % 32 == 0 and N % 64 == 0)
        out["bf16"].append(ws // ((Ktot + 1) * N) if ws else -1)
        ws = L.lwg_conv2d_wgrad_winograd_ws_floats(ctypes.byref(a))
        assert ws % (16 * C * N) == 0 and (ws > 0) == (nt == 9 and C % 64 == 0 and N % 64 == 0)
        out["winograd"].append(ws // (16 * C * N) if ws else -1)
    return out


# ---------------------------------------------------------------------------------------------------------------- the GPU cases
# name -> (entry, geometry); geometry = dict(B, H, W, C0, C1, N, taps, ...) + un-packing (transposed, kidx, D (the dw shape), cin, nout, db)
def _conv(B, H, W, C0, N, k=3, C1=0, cin=None, nout=None, db=False, **kw):
    cin, nout = cin or C0 + C1, nout or N
    return dict(B=B, H=H, W=W, C0=C0, C1=C1, N=N, taps=taps_of(k), transposed=0, kidx=list(range(k * k)), D=(nout, cin, k, k), cin=cin, nout=nout, db=db, **kw)


UNPACKED = "lwg_conv2d_wgrad_unpacked_f32"
GPU_CASES = {
    # direct kernel <SMALLC, BN> x reduction kernel
    "d_c4_n64_ragged": (UNPACKED, _conv(3, 9, 7, 4, 64, cin=3, nout=4, db=True)),                    # <1, 64>, M = 189, cin < cin_pad, nout < n_pad (odd: scalar map)
    "d_c8_n128": (UNPACKED, _conv(1, 64, 64, 8, 128, cin=6, db=True)),                              # <1, 128>, 32 slabs
    "d_c8_n64_many": (UNPACKED, _conv(1, 96, 96, 8, 64, k=1)),                                      # <1, 64>, 72 slabs
    "d_1x1_n64_many": (UNPACKED, _conv(1, 96, 96, 64, 64, k=1, db=True)),                           # <0, 64>, 72 slabs
    "d_n192": (UNPACKED, _conv(1, 96, 96, 32, 192)),                                                # <0, 64> (192 % 128 = 64), 48 slabs
    "d_two_inputs_many": (UNPACKED, _conv(1, 128, 128, 32, 128, C1=32, db=True)),                   # <0, 128>, C1 > 0, 86 slabs of 73728 weights
    "d_n128_32": (UNPACKED, _conv(1, 64, 64, 64, 128, db=True)),                                    # 32 slabs
    "d_n128_8": (UNPACKED, _conv(1, 32, 32, 64, 128, cin=60, nout=124, db=True)),                   # 8 slabs, cin < cin_pad, nout < n_pad (quads)
    "d_n128_ragged": (UNPACKED, _conv(3, 9, 7, 64, 128)),                                           # M = 189: one slab
    "d_stride2": (UNPACKED, _conv(2, 17, 13, 32, 64, stride=2, OH=9, OW=7, db=True)),
    "d_parity": (UNPACKED, dict(B=1, H=16, W=16, C0=64, C1=0, N=64, taps=PARITY_TAPS, omul=2, ooy=1, oox=0, transposed=1, kidx=PARITY_KIDX,
                                D=(64, 64, 4, 4), cin=64, nout=64, db=False)),                      # a quarter of a pre-filled (Cin, N, 4, 4)
    "d_parity_quads": (UNPACKED, dict(B=1, H=16, W=16, C0=128, C1=0, N=128, taps=PARITY_TAPS, omul=2, ooy=1, oox=0, transposed=1, kidx=PARITY_KIDX,
                                      D=(128, 128, 4, 4), cin=128, nout=128, db=False)),
    "d_adjoint16": (UNPACKED, dict(B=1, H=32, W=32, C0=64, C1=0, N=64, taps=ADJ_TAPS, stride=2, OH=16, OW=16, transposed=0, kidx=ADJ_KIDX,
                                   D=(64, 64, 4, 4), cin=64, nout=64, db=False)),
    # the packed form: the plain reductions
    "p_1x1_many": ("lwg_conv2d_wgrad_nhwc_f32", _conv(1, 96, 96, 64, 64, k=1)),                      # 72 slabs of 4096
    "p_c8_32": ("lwg_conv2d_wgrad_nhwc_f32", _conv(1, 64, 64, 8, 128)),                              # 32 slabs of 9216
    "p_n128_8": ("lwg_conv2d_wgrad_nhwc_f32", _conv(1, 32, 32, 64, 128)),                            # 8 slabs of 73728
    # bf16 operands
    "b_n64": ("lwg_conv2d_wgrad_bf16_f32", _conv(1, 96, 96, 64, 64, k=1, db=True)),
    "b_n192_two_inputs": ("lwg_conv2d_wgrad_bf16_f32", _conv(1, 64, 64, 32, 192, C1=32, cin=60, nout=188)),
    "b_n128": ("lwg_conv2d_wgrad_bf16_f32", _conv(1, 64, 64, 64, 128, db=True)),
    "b_ragged": ("lwg_conv2d_wgrad_bf16_f32", _conv(3, 9, 7, 32, 128, db=True)),
    "b_adjoint16": ("lwg_conv2d_wgrad_bf16_f32", dict(B=1, H=32, W=32, C0=64, C1=0, N=64, taps=ADJ_TAPS, stride=2, OH=16, OW=16, transposed=0, kidx=ADJ_KIDX,
                                                      D=(64, 64, 4, 4), cin=64, nout=64, db=False)),
    # Winograd: its three reductions
    "w_many": ("lwg_conv2d_wgrad_winograd_f32", _conv(1, 96, 96, 64, 64)),
    "w_8": ("lwg_conv2d_wgrad_winograd_f32", _conv(1, 32, 32, 64, 128, C1=64, cin=120, nout=100)),
    "w_ragged": ("lwg_conv2d_wgrad_winograd_f32", _conv(3, 9, 7, 64, 64)),
    # column sums: (rows, C)
    "c_many": ("lwg_colsum_nhwc_f32", dict(rows=9216, C=64)),                                         # 144 row blocks
    "c_32": ("lwg_colsum_nhwc_f32", dict(rows=2000, C=128)),
    "c_3": ("lwg_colsum_nhwc_f32", dict(rows=189, C=64)),
    "c_odd": ("lwg_colsum_nhwc_f32", dict(rows=5000, C=6)),                                           # C % 4 != 0: the scalar first pass, 64 row blocks
}


def _reduce_form(total, nsplit):
    return "slab_reduce_g<16>" if total < 65536 and nsplit >= 64 else "slab_reduce_g<4>" if total < 65536 and nsplit >= 16 else "wgrad_reduce"


def _unpack_form(g, nsplit):
    """lwg_wgrad_reduce_unpack's choice, restated from its thresholds."""
    weights = len(g["taps"]) * g["cin"] * g["nout"]
    total = weights + (g["nout"] if g["db"] else 0)
    slab = (len(g["taps"]) * (g["C0"] + g["C1"]) + 1) * g["N"]
    if weights >= 65536 and g["nout"] % 4 == 0 and g["N"] % 4 == 0 and slab % 4 == 0:
        if total // 4 < 65536 and nsplit >= 32:
            return "unpack4g<8>" if nsplit >= 64 else "unpack4g<4>"
        return "unpack4"
    return "unpack<16>" if weights < 65536 and nsplit >= 64 else "unpack<4>" if weights < 65536 and nsplit >= 16 else "unpack<1>"


def _bn(N):
    return 64 if N % 128 != 0 and N % 128 <= 64 else 128


def form_of(name):
    """The kernels a case reaches, from the host-only workspace queries, the slab size and the launchers' thresholds."""
    L = _lib.lib()
    entry, g = GPU_CASES[name]
    if entry == "lwg_colsum_nhwc_f32":
        rows, C = g["rows"], g["C"]
        if C % 4 == 0 and C <= 1024 and 256 % min(C // 4, 256) == 0:
            nblk = 512 if rows >= 512 * 64 else (rows + 63) // 64
            return "colsum_partial4 x%d + %s" % (nblk, _reduce_form(C, nblk))
        nblk = 64 if rows >= 64 * 64 else (rows + 63) // 64
        return "colsum_partial x%d + %s" % (nblk, _reduce_form(C, nblk))
    a = _args(g)
    Cin, nt = g["C0"] + g["C1"], len(g["taps"])
    Ktot = nt * Cin
    if entry == "lwg_conv2d_wgrad_winograd_f32":
        n = L.lwg_conv2d_wgrad_winograd_ws_floats(ctypes.byref(a)) // (16 * Cin * g["N"])
        total = g["cin"] * g["nout"]
        return "wgrad_winograd x%d + wgw_reduce<%d>" % (n, 16 if total < 65536 and n >= 32 else 4 if total < 262144 and n >= 8 else 1)
    if entry == "lwg_conv2d_wgrad_bf16_f32":
        n = L.lwg_conv2d_wgrad_bf16_ws_floats(ctypes.byref(a)) // ((Ktot + 1) * g["N"])
        return "wgrad_bf16<%d> x%d + %s" % (_bn(g["N"]), n, _unpack_form(g, n))
    n = L.lwg_conv2d_wgrad_ws_floats(Ktot, g["N"], a.M) // ((Ktot + 1) * g["N"])
    kern = "wgrad<%d, %d> x%d" % (Cin % 32 != 0, _bn(g["N"]), n)
    return kern + " + " + (_reduce_form(Ktot * g["N"], n) if entry == "lwg_conv2d_wgrad_nhwc_f32" else _unpack_form(g, n))


def _args(g, x0=1, x1=1):
    return conv_args(g["B"], g["H"], g["W"], g["C0"], g["C1"], g["N"], g["taps"], stride=g.get("stride", 1), OH=g.get("OH"), OW=g.get("OW"),
                     omul=g.get("omul", 1), ooy=g.get("ooy", 0), oox=g.get("oox", 0), x0=x0, x1=x1)


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_case(name):
    """One case on the device -> {"form", "dw", "db" (absent without a bias gradient)}.  dw and db are pre-filled with seeded values, so
    whatever the launch leaves untouched is part of the hash."""
    import torch
    L = _lib.lib()
    entry, g = GPU_CASES[name]
    gen = torch.Generator().manual_seed(sum(name.encode()) * 7919 + len(name))
    rnd = lambda *s: torch.randn(*s, generator=gen).cuda()                   # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    out = {"form": form_of(name)}
    if entry == "lwg_colsum_nhwc_f32":
        x, o, ws = rnd(g["rows"], g["C"]), rnd(g["C"]), torch.empty(512 * g["C"]).cuda()
        _lib.check(L.lwg_colsum_nhwc_f32(x.data_ptr(), g["rows"], g["C"], o.data_ptr(), ws.data_ptr(), stream), entry)
        torch.cuda.synchronize()
        out["db"] = _sha(o)
        return out
    x0 = rnd(g["B"], g["H"], g["W"], g["C0"])
    x1 = rnd(g["B"], g["H"], g["W"], g["C1"]) if g["C1"] else None
    a = _args(g, x0.data_ptr(), x1.data_ptr() if g["C1"] else None)
    dy = rnd(g["B"], a.YH, a.YW, g["N"])
    Ktot = len(g["taps"]) * (g["C0"] + g["C1"])
    kidx = (ctypes.c_int * len(g["kidx"]))(*g["kidx"])
    D = g["D"]
    db = rnd(g["nout"]) if g["db"] else None
    dbp = db.data_ptr() if g["db"] else None
    if entry == "lwg_conv2d_wgrad_nhwc_f32":
        dw = rnd(Ktot, g["N"])
        ws = torch.empty(L.lwg_conv2d_wgrad_ws_floats(Ktot, g["N"], a.M)).cuda()
        _lib.check(L.lwg_conv2d_wgrad_nhwc_f32(ctypes.byref(a), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), stream), entry)
    elif entry == "lwg_conv2d_wgrad_winograd_f32":
        dw = rnd(g["nout"], g["cin"], 3, 3)
        ws = torch.empty(L.lwg_conv2d_wgrad_winograd_ws_floats(ctypes.byref(a))).cuda()
        assert ws.numel() > 0
        _lib.check(L.lwg_conv2d_wgrad_winograd_f32(ctypes.byref(a), dy.data_ptr(), ws.data_ptr(), dw.data_ptr(), g["cin"], g["nout"], stream), entry)
    else:
        dw = rnd(*D)
        n = L.lwg_conv2d_wgrad_bf16_ws_floats(ctypes.byref(a)) if entry == "lwg_conv2d_wgrad_bf16_f32" else L.lwg_conv2d_wgrad_ws_floats(Ktot, g["N"], a.M)
        assert n > 0
        ws = torch.empty(n).cuda()
        _lib.check(getattr(L, entry)(ctypes.byref(a), dy.data_ptr(), ws.data_ptr(), dw.data_ptr(), D[0], D[1], D[2], D[3], g["transposed"], kidx,
                                     g["cin"], g["nout"], dbp, stream), entry)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dw).all())
    out["dw"] = _sha(dw)
    if db is not None:
        out["db"] = _sha(db)
    return out


def gpu():
    return {name: run_case(name) for name in GPU_CASES}


if __name__ == "__main__":
    what, path = sys.argv[1:3]
    res = {"plans": plans, "gpu": gpu}[what]()
    with open(path, "w") as f:
        json.dump(res, f, indent=None if what == "plans" else 1, separators=(",", ":") if what == "plans" else None, sort_keys=True)
        f.write("\n")
    print("%s: %d entries -> %s" % (what, len(res["direct"]) if what == "plans" else len(res), path))
