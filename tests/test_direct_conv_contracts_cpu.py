"""CPU checks of the host contracts of the direct (implicit-GEMM) convolution entry points, clause by clause.

test_decision_table calls every entry point in a child process that sees no GPU (checked) on fake pointers: a small base description (8 x 8 pixels,
64 channels) that passes every host check - so the call gets as far as the launch, which fails with another code than 1 where no device is visible -
and one single-field mutation per clause of the entry point's checks, which must return 1 (hipErrorInvalidValue) before any launch.  Cases marked
``ok`` are accepted descriptions (variants of the base, and the oddities of the contracts): they must return neither 0 nor 1.

The clauses, per entry point (tick them off against the code; "common" = N = 96, YC = 66, RESIDUAL without res, SPADE without xn, epi = 7):
  lwg_conv2d_nhwc_f32 / _f32_ws: common; x0 / w / y null; ntaps 0 and LWG_MAX_TAPS + 1; M = 0; Cin % 4; ycoff % 4; xdt bf16; ydt unknown; ydt bf16 with
    an epilogue; (ws) ydt bf16 / planes with a workspace; ydt planes with the ReLU mask; small Cin: a second input, Cin > 16, Cin not a power of two, a wrong
    cshift, SPADE, RESIDUAL; two inputs: C0 % 32, x1 null; SPADE: mean / rstd / bias null, N % 128, N != 2 YC; plain epilogue with the ReLU mask; one frame of
    3 GiB; a sliced batch with M != B OH OW; (ws) a sliced batch with a workspace.  ok: ydt bf16 / planes plain; small Cin; two inputs; SPADE; SPADE with ycoff = 4
    (not checked here); RESIDUAL (with the ReLU mask too); M != B OH OW unsliced (slicing comes before the field checks, which never compare M); a batch over
    3 GiB (sliced).
  lwg_conv2d_nhwc_f32_split: common; x0 / w / y null; ntaps; M; Cin % 32; ycoff % 4; two inputs: C0 % 32, x1 null; the panel of 6 bytes per (k, n) at 3 GiB;
    xdt / ydt bf16; SPADE: mean / rstd / bias null, N % 128, N != 2 YC; one frame of 3 GiB.  ok: SPADE with ycoff = 4; RESIDUAL; the panel just under 3 GiB.
  lwg_conv2d_nhwc_bf16: common; x0 / w / y null; ntaps; M; xdt / ydt fp32; Cin % 64; YC % 8; ycoff % 8; two inputs: C0 % 64, x1 null; the panel of 2 bytes per
    (k, n) at 3 GiB; SPADE: mean / rstd / bias null, N % 128, N != 2 YC, ycoff != 0; one frame of 3 GiB.  ok: SPADE; RESIDUAL; two inputs; the panel just under.
  lwg_conv2d_nhwc_bf16_hr, 3 x 3 and 2 x 2: common; x0 / w / y null; M; ntaps = 5; xdt / ydt fp32; stride; OH != H; OW != W; Cin % 64; YC % 8; ycoff % 8; two
    inputs: C0 % 64, x1 null; a tap outside [-1, 1]; taps that are no ascending grid; the panel at 3 GiB; SPADE: mean / rstd / bias null, N != 2 YC, ycoff != 0;
    one frame of 3 GiB.  ok: SPADE with N = 64 (no N % 128 rule here); RESIDUAL; the 2 x 2 grid.
    pointwise: common (N = 96 breaks N = C0); a tap off the centre; a second input; N != C0; N = C0 = 192; an epilogue; YC % 8; ycoff % 8; M C0 2 bytes at 3 GiB.
    ok: C = 128 and 256; M C0 2 just under 3 GiB.
  lwg_conv2d_nhwc_c8_bf16: common; x0 / w / y null; M; ntaps 0 and 11; xdt bf16; ydt fp32; C0 = 16; a second input; N = 128; ycoff % 8; stride 0; one frame
    of 3 GiB.  ok: stride 2; 10 taps.
  lwg_conv_transpose4_nhwc_f32: common; x0 / w / y null; M; ntaps; stride; omul; ooy; oox; a second input; xdt bf16; ydt bf16; C0 % 32; ycoff % 4; OH; OW; YH;
    YW; dy / dx outside {-1, 0}; one frame of 3 GiB.  ok: ydt planes.
  lwg_conv_transpose4_nhwc_bf16: common; x0 / w / y null; M; ntaps; a second input; C0 = 192; xdt / ydt fp32; stride; H != OH; W != OW; omul; YH; YW; ycoff % 8;
    one frame of 3 GiB.  ok: C0 = 64; N = 128; taps of any value (ignored).
  lwg_up4_head_compose_bf16: x0 / w / bias / whead null; pred without bg; no output; B, H, W = 0; C0 = 64; a second input; N = 128; ntaps; stride; omul; OH;
    OW; xdt fp32; an epilogue; act != ReLU; one frame of 3 GiB.  ok: mask only; pred with bg; a batch over 3 GiB (sliced).

test_fit_helpers_by_inclusion compiles part 1 of csrc/lwg_conv_direct.h into a host program with signed-overflow traps and holds the buffer-range
predicates and the frames-per-slice rule to a restatement on both sides of every size limit.  test_direct_family_uses_the_shared_header is the converse
text check: the direct family's sources spell no limit, opt-in state or slicing loop of their own."""
import json
import os
import re
import subprocess
import sys
import tempfile

from tests.test_conv_offsets_cpu import CSRC, OOB, ROOT, _code, _compiler

MAX_TAPS = 52
NONE, RESIDUAL, SPADE = 0, 1, 2
F32, BF16, Q4 = 0, 1, 2
RELU, MASK = 1, 5
T3 = [(t // 3 - 1, t % 3 - 1) for t in range(9)]
T2 = [(-1, -1), (-1, 0), (0, -1), (0, 0)]

_CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, ROOT)
hip = ctypes.CDLL("libamdhip64.so")
n = ctypes.c_int(0)
e = hip.hipGetDeviceCount(ctypes.byref(n))
if e == 0 and n.value > 0:
    print(json.dumps({"error": "a device is visible"}))
    sys.exit(0)
from ipercore_amd import _lib
L = _lib.lib()
bad = 0xdead0000
PTRS = ("x0", "x1", "w", "y", "bias", "res", "xn", "mean", "rstd")
def call(fn, d):
    a = _lib.LwgConvArgs()
    for k, v in d.items():
        if k in PTRS:
            setattr(a, k, bad if v else None)
        elif k == "taps":
            for t, (dy, dx) in enumerate(v):
                a.dy[t], a.dx[t] = dy, dx
        elif not k.startswith("_"):
            setattr(a, k, v)
    p = lambda k: bad if d.get(k) else None
    if fn == "lwg_up4_head_compose_bf16":
        return L.lwg_up4_head_compose_bf16(ctypes.byref(a), p("_whead"), p("_bg"), 0, p("_pred"), p("_mask"), p("_img"), None)
    if fn.endswith("_ws"):
        return L.lwg_conv2d_nhwc_f32_ws(ctypes.byref(a), p("_ws"), None)
    return getattr(L, fn)(ctypes.byref(a), None)
print(json.dumps([call(fn, d) for _, fn, d, _ in CASES]))
"""


def _base(**kw):
    """8 x 8 pixels, 64 -> 64 channels, 3 x 3, fp32, plain epilogue; every pointer of the plain launch given."""
    d = dict(x0=1, x1=0, w=1, y=1, bias=1, res=0, xn=0, mean=0, rstd=0, B=1, H=8, W=8, C0=64, C1=0, N=64, OH=8, OW=8, M=64, YH=8, YW=8, YC=64, ycoff=0,
             stride=1, ntaps=9, cshift=0, omul=1, ooy=0, oox=0, epi=NONE, act=0, xdt=F32, ydt=F32, taps=T3)
    d.update(kw)
    return d


def _spade(d, **kw):
    d = dict(d, **kw)
    return dict(d, epi=SPADE, xn=1, mean=1, rstd=1, N=2 * d["YC"])


def _frame(d, ebytes, C=None, up=1):
    """One frame of exactly 3 GiB in a batch of two (a row of pixels)."""
    w = OOB // ((C or d["C0"]) * ebytes)
    return dict(d, B=2, H=1, W=w, OH=1, OW=w, M=2 * w, YH=up, YW=up * w)


def _cases():
    """(label, entry point, description, the result is 1)."""
    out = []

    def add(fn, base, refused, accepted=()):
        out.append(("%s base" % fn, fn, base, False))
        out.extend(("%s refuses %s" % (fn, k), fn, dict(base, **m) if isinstance(m, dict) else m, True) for k, m in refused)
        out.extend(("%s accepts %s" % (fn, k), fn, dict(base, **m) if isinstance(m, dict) else m, False) for k, m in accepted)

    def common(b):
        return [("N = 96", dict(N=96)), ("YC = 66", dict(YC=66)), ("RESIDUAL without res", dict(epi=RESIDUAL)),
                ("SPADE without xn", dict(_spade(b), xn=0)), ("epi = 7", dict(epi=7))]

    def nulls(*names):
        return [("%s null" % k, {k: 0}) for k in names]

    def two(b, mult):
        return [("two inputs: C0 %% %d" % mult, dict(C0=mult + mult // 2, C1=mult // 2, x1=1)), ("two inputs: x1 null", dict(C0=mult, C1=mult))]

    def spade_rules(b, n128=True, ycoff0=False):
        s = _spade(b, YC=64)
        r = [("SPADE: %s null" % k, dict(s, **{k: 0})) for k in ("mean", "rstd", "bias")] + [("SPADE: N != 2 YC", dict(s, YC=32))]
        if n128:
            r.append(("SPADE: N % 128", _spade(b, YC=32)))
        if ycoff0:
            r.append(("SPADE: ycoff != 0", dict(s, ycoff=8)))
        return r

    sliced = dict(B=3, H=1024, W=1024, OH=1024, OW=1024, YH=1024, YW=1024, C0=256, YC=64, M=3 * 1024 * 1024)       # fp32: 1 GiB per frame -> slices of two
    # ---- fp32
    b = _base()
    small = dict(C0=8, cshift=1)
    for fn in ("lwg_conv2d_nhwc_f32", "lwg_conv2d_nhwc_f32_ws"):
        ws = fn.endswith("_ws")
        refused = common(b) + nulls("x0", "w", "y") + [
            ("ntaps = 0", dict(ntaps=0)), ("ntaps over the maximum", dict(ntaps=MAX_TAPS + 1)), ("M = 0", dict(M=0)), ("Cin % 4", dict(C0=62)), ("ycoff % 4", dict(ycoff=2)),
            ("xdt bf16", dict(xdt=BF16)), ("ydt unknown", dict(ydt=7)), ("ydt bf16 with an epilogue", dict(ydt=BF16, epi=RESIDUAL, res=1)),
            ("ydt planes with the ReLU mask", dict(ydt=Q4, act=MASK)), ("small Cin: a second input", dict(C0=8, C1=8, x1=1, cshift=2)),
            ("small Cin: over 16", dict(C0=24, cshift=2)), ("small Cin: no power of two", dict(C0=12, cshift=1)), ("small Cin: cshift", dict(C0=8, cshift=2)),
            ("small Cin: SPADE", _spade(b, YC=64, **small)), ("small Cin: RESIDUAL", dict(small, epi=RESIDUAL, res=1))] + two(b, 32) + spade_rules(b) + [
            ("the ReLU mask without RESIDUAL", dict(act=MASK)), ("one frame of 3 GiB", _frame(b, 4)), ("a sliced batch with M != B OH OW", dict(sliced, M=64))]
        if ws:
            refused += [("ydt bf16 with a workspace", dict(ydt=BF16, _ws=1)), ("ydt planes with a workspace", dict(ydt=Q4, _ws=1)),
                        ("a sliced batch with a workspace", dict(sliced, _ws=1))]
        accepted = [("ydt bf16", dict(ydt=BF16)), ("ydt planes", dict(ydt=Q4)), ("small Cin", small), ("two inputs", dict(C0=32, C1=32, x1=1)), ("SPADE", _spade(b, YC=64)),
                    ("SPADE with ycoff = 4", _spade(b, YC=64, ycoff=4)), ("RESIDUAL", dict(epi=RESIDUAL, res=1)), ("RESIDUAL with the ReLU mask", dict(epi=RESIDUAL, res=1, act=MASK)),
                    ("M != B OH OW", dict(M=63)), ("a batch over 3 GiB", sliced)]
        if ws:
            accepted += [("a workspace", dict(_ws=1)), ("the ReLU mask with a workspace", dict(epi=RESIDUAL, res=1, act=MASK, _ws=1, C0=2048, M=64))]
        add(fn, b, refused, accepted)
    # ---- three-plane bf16 split of fp32: a 6-byte panel entry per (k, n)
    assert 9 * 8192 * 7232 * 6 < OOB <= 9 * 8192 * 7296 * 6
    add("lwg_conv2d_nhwc_f32_split", b, common(b) + nulls("x0", "w", "y") + [
        ("ntaps = 0", dict(ntaps=0)), ("ntaps over the maximum", dict(ntaps=MAX_TAPS + 1)), ("M = 0", dict(M=0)), ("Cin % 32", dict(C0=48)), ("ycoff % 4", dict(ycoff=2))] +
        two(b, 32) + [("the panel at 3 GiB", dict(C0=8192, N=7296)), ("xdt bf16", dict(xdt=BF16)), ("ydt bf16", dict(ydt=BF16))] + spade_rules(b) +
        [("one frame of 3 GiB", _frame(b, 4))],
        [("SPADE with ycoff = 4", _spade(b, YC=64, ycoff=4)), ("RESIDUAL", dict(epi=RESIDUAL, res=1)), ("the panel just under 3 GiB", dict(C0=8192, N=7232))])
    # ---- bf16: 2 bytes per (k, n)
    b = _base(xdt=BF16, ydt=BF16)
    assert 9 * 16384 * 10880 * 2 < OOB <= 9 * 16384 * 10944 * 2
    add("lwg_conv2d_nhwc_bf16", b, common(b) + nulls("x0", "w", "y") + [
        ("ntaps = 0", dict(ntaps=0)), ("ntaps over the maximum", dict(ntaps=MAX_TAPS + 1)), ("M = 0", dict(M=0)), ("xdt fp32", dict(xdt=F32)), ("ydt fp32", dict(ydt=F32)),
        ("Cin % 64", dict(C0=32)), ("YC % 8", dict(YC=68)), ("ycoff % 8", dict(ycoff=4))] + two(b, 64) + [("the panel at 3 GiB", dict(C0=16384, N=10944))] +
        spade_rules(b, ycoff0=True) + [("one frame of 3 GiB", _frame(b, 2))],
        [("SPADE", _spade(b, YC=64)), ("RESIDUAL", dict(epi=RESIDUAL, res=1)), ("two inputs", dict(C0=64, C1=64, x1=1)), ("the panel just under 3 GiB", dict(C0=16384, N=10880))])
    fn = "lwg_conv2d_nhwc_bf16_hr"
    t_out = [(-2, -1)] + T3[1:]
    t_nogrid = [T3[1], T3[0]] + T3[2:]
    add(fn, b, common(b) + nulls("x0", "w", "y") + [
        ("M = 0", dict(M=0)), ("ntaps = 5", dict(ntaps=5)), ("xdt fp32", dict(xdt=F32)), ("ydt fp32", dict(ydt=F32)), ("stride 2", dict(stride=2)), ("OH != H", dict(OH=4)),
        ("OW != W", dict(OW=4)), ("Cin % 64", dict(C0=32)), ("YC % 8", dict(YC=68)), ("ycoff % 8", dict(ycoff=4))] + two(b, 64) + [
        ("a tap outside [-1, 1]", dict(taps=t_out)), ("taps that are no grid", dict(taps=t_nogrid)), ("the panel at 3 GiB", dict(C0=16384, N=10944))] +
        spade_rules(b, n128=False, ycoff0=True) + [("one frame of 3 GiB", _frame(b, 2))],
        [("SPADE with N = 64", _spade(b, YC=32)), ("RESIDUAL", dict(epi=RESIDUAL, res=1)), ("two inputs", dict(C0=64, C1=64, x1=1))])
    b2 = dict(b, ntaps=4, taps=T2)
    out.append(("%s 2 x 2 base" % fn, fn, b2, False))
    out.extend(("%s 2 x 2 refuses %s" % (fn, k), fn, dict(b2, **m), True) for k, m in common(b2) + [("taps that are no grid", dict(taps=T2[:3] + [(0, 1)]))])
    bp = dict(b, ntaps=1, taps=[(0, 0)])
    m_lim = OOB // (64 * 2)
    out.append(("%s pointwise base" % fn, fn, bp, False))
    out.extend(("%s pointwise refuses %s" % (fn, k), fn, dict(bp, **m), True) for k, m in common(bp) + [
        ("a tap off the centre", dict(taps=[(0, 1)])), ("a second input", dict(C1=64, x1=1)), ("N != C0", dict(N=128, YC=128)), ("N = C0 = 192", dict(C0=192, N=192, YC=192)),
        ("an epilogue", dict(epi=RESIDUAL, res=1)), ("YC % 8", dict(YC=68)), ("ycoff % 8", dict(ycoff=4)), ("M C0 2 bytes at 3 GiB", dict(M=m_lim))])
    out.extend(("%s pointwise accepts %s" % (fn, k), fn, dict(bp, **m), False) for k, m in [
        ("C = 128", dict(C0=128, N=128, YC=128)), ("C = 256", dict(C0=256, N=256, YC=256)), ("M C0 2 bytes just under 3 GiB", dict(M=m_lim - 1))])
    # ---- the bf16 first layer: fp32 NHWC-8 in, bf16 out
    b = _base(C0=8, ydt=BF16)
    add("lwg_conv2d_nhwc_c8_bf16", b, common(b) + nulls("x0", "w", "y") + [
        ("M = 0", dict(M=0)), ("ntaps = 0", dict(ntaps=0)), ("ntaps = 11", dict(ntaps=11)), ("xdt bf16", dict(xdt=BF16)), ("ydt fp32", dict(ydt=F32)), ("C0 = 16", dict(C0=16)),
        ("a second input", dict(C1=8, x1=1)), ("N = 128", dict(N=128, YC=128)), ("ycoff % 8", dict(ycoff=4)), ("stride 0", dict(stride=0)), ("one frame of 3 GiB", _frame(b, 4))],
        [("stride 2", dict(stride=2, OH=4, OW=4, M=16, YH=4, YW=4)), ("10 taps", dict(ntaps=10))])
    # ---- the transposed forms
    b = _base(ntaps=4, taps=T2, omul=2, YH=16, YW=16)
    add("lwg_conv_transpose4_nhwc_f32", b, common(b) + nulls("x0", "w", "y") + [
        ("M = 0", dict(M=0)), ("ntaps = 9", dict(ntaps=9)), ("stride 2", dict(stride=2)), ("omul 1", dict(omul=1)), ("ooy", dict(ooy=1)), ("oox", dict(oox=1)),
        ("a second input", dict(C0=32, C1=32, x1=1)), ("xdt bf16", dict(xdt=BF16)), ("ydt bf16", dict(ydt=BF16)), ("C0 % 32", dict(C0=48)), ("ycoff % 4", dict(ycoff=2)),
        ("OH != H", dict(OH=4)), ("OW != W", dict(OW=4)), ("YH != 2 H", dict(YH=8)), ("YW != 2 W", dict(YW=8)), ("dy = 1", dict(taps=T2[:3] + [(1, 0)])),
        ("dy = -2", dict(taps=[(-2, -1)] + T2[1:])), ("dx = 1", dict(taps=T2[:3] + [(0, 1)])), ("dx = -2", dict(taps=[(-1, -2)] + T2[1:])),
        ("one frame of 3 GiB", _frame(b, 4, up=2))], [("ydt planes", dict(ydt=Q4))])
    b = dict(b, C0=128, xdt=BF16, ydt=BF16)
    add("lwg_conv_transpose4_nhwc_bf16", b, common(b) + nulls("x0", "w", "y") + [
        ("M = 0", dict(M=0)), ("ntaps = 9", dict(ntaps=9)), ("a second input", dict(C0=64, C1=64, x1=1)), ("C0 = 192", dict(C0=192)), ("xdt fp32", dict(xdt=F32)),
        ("ydt fp32", dict(ydt=F32)), ("stride 2", dict(stride=2)), ("H != OH", dict(OH=4, YH=8)), ("W != OW", dict(OW=4, YW=8)), ("omul 1", dict(omul=1)),
        ("YH != 2 OH", dict(YH=8)), ("YW != 2 OW", dict(YW=8)), ("ycoff % 8", dict(ycoff=4)), ("one frame of 3 GiB", _frame(b, 2, up=2))],
        [("C0 = 64", dict(C0=64)), ("N = 128", dict(N=128, YC=128)), ("taps of any value", dict(taps=[(5, 5)] * 4))])
    # ---- the fused last up-sampling layer + head
    b = dict(b, act=RELU, _whead=1, _mask=1)
    half = dict(B=3, H=2048, W=2048, OH=2048, OW=2048)             # 1 GiB per frame
    add("lwg_up4_head_compose_bf16", b, nulls("x0", "w", "bias", "_whead") + [
        ("pred without bg", dict(_pred=1)), ("no output", dict(_mask=0)), ("B = 0", dict(B=0)), ("H = 0", dict(H=0, OH=0)), ("W = 0", dict(W=0, OW=0)), ("C0 = 64", dict(C0=64)),
        ("a second input", dict(C1=64, x1=1)), ("N = 128", dict(N=128)), ("ntaps = 9", dict(ntaps=9)), ("stride 2", dict(stride=2)), ("omul 1", dict(omul=1)),
        ("OH != H", dict(OH=4)), ("OW != W", dict(OW=4)), ("xdt fp32", dict(xdt=F32)), ("an epilogue", dict(epi=RESIDUAL, res=1)), ("act none", dict(act=0)),
        ("one frame of 3 GiB", _frame(b, 2))], [("pred with bg", dict(_pred=1, _bg=1)), ("img only", dict(_mask=0, _img=1)), ("a batch over 3 GiB", half)])
    return out


def test_decision_table():
    """Every clause of every direct conv entry point refuses its mutation with 1 before any launch; the bases and the accepted variants - the contracts'
    oddities among them - pass every host check (the module docstring lists the clauses)."""
    cases = _cases()
    assert len({k for k, _, _, _ in cases}) == len(cases)
    code = "ROOT = %r\nCASES = %r\n" % (ROOT, cases) + _CHILD
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-"], input=code, capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)      # (too long for a command line)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert isinstance(got, list), got
    assert len(got) == len(cases)
    wrong = {k: v for (k, _, _, refused), v in zip(cases, got) if (v != 1 if refused else v in (0, 1))}
    assert not wrong, wrong
    for fn in ("lwg_conv2d_nhwc_f32", "lwg_conv2d_nhwc_f32_ws", "lwg_conv2d_nhwc_f32_split", "lwg_conv2d_nhwc_bf16", "lwg_conv2d_nhwc_bf16_hr", "lwg_conv2d_nhwc_c8_bf16",
               "lwg_conv_transpose4_nhwc_f32", "lwg_conv_transpose4_nhwc_bf16", "lwg_up4_head_compose_bf16"):
        assert sum(1 for _, f, _, refused in cases if f == fn and refused) >= 15, fn


# ---- part 1 of the shared header, by inclusion ----

_AUDIT = r"""
#include <cstdio>
#include "lwg_conv_direct.h"
struct Fit { int B, H, W, C0, C1, e; };
struct Sl { int B; unsigned long long per; };
static const Fit fits[] = { FITS };
static const Sl sls[] = { SLS };
int main() {
    std::printf("range %llu\n", (unsigned long long)LWG_BUF_RANGE);
    int i = 0;
    for (const Fit& f : fits) {
        LwgConvArgs a = {};
        a.B = f.B, a.H = f.H, a.W = f.W, a.C0 = f.C0, a.C1 = f.C1, a.ntaps = f.H, a.N = f.W, a.xdt = f.e == 2 ? LWG_DT_BF16 : LWG_DT_F32;
        const unsigned long long bytes = (unsigned long long)f.B * f.H * f.W * (unsigned long long)(f.C0 > f.C1 ? f.C0 : f.C1) * f.e;
        std::printf("fit %d %d%d%d %d\n", i++, (int)lwg_buf_fits(bytes), (int)cd_inputs_fit(a, f.e), (int)cd_panel_fits(a, f.B * f.e), lwg_conv_slice_frames(a));
    }
    i = 0;
    for (const Sl& s : sls) std::printf("slice %d %d\n", i++, lwg_slice_frames(s.B, s.per));
    return 0;
}
"""


def _slice_frames(B, per):
    if per == 0 or B * per < OOB:
        return 0
    n = (OOB - 1) // per
    return n if n >= 1 else -1


def test_fit_helpers_by_inclusion():
    """lwg_buf_fits, cd_inputs_fit, cd_panel_fits, lwg_slice_frames and lwg_conv_slice_frames as the entry points compile them, against their restatement:
    a tensor fits a raw buffer iff its bytes < 0xC0000000; a batch is cut into slices of (0xC0000000 - 1) / per frames iff B per >= 0xC0000000, and a frame
    of that size or more is refused.  Evaluated at B per == 0xC0000000 exactly and one element to either side, for both element sizes, one and two inputs."""
    fits = []
    for e in (2, 4):
        for C0, C1 in ((64, 0), (64, 256), (1024, 32)):
            C = max(C0, C1)
            for B, H in ((1, 1), (1, 384), (3, 128), (24, 16), (1536, 1)):
                W = OOB // (B * H * C * e)
                assert B * H * W * C * e == OOB
                fits += [(B, H, W + d, C0, C1, e) for d in (-1, 0, 1)]
    fits += [(0, 8, 8, 64, 0, 4), (4, 0, 8, 64, 0, 2), (2, 8, 8, 0, 0, 4), (65535, 1024, 1024, 64, 64, 4)]
    sls = [(B, per + d) for B, per in ((1, OOB), (2, OOB // 2), (3, OOB // 3), (48, OOB // 48), (3, 1 << 30), (2, OOB - 1), (1, 256), (7, 1 << 29)) for d in (-1, 0, 1)]
    sls += [(5, 0), (1, OOB - 1), (OOB // 256 + 1, 256), (OOB // 256, 256), (OOB // 256 - 1, 256), (2, 1 << 40)]
    src = _AUDIT.replace("FITS", ", ".join("{%d, %d, %d, %d, %d, %d}" % f for f in fits)).replace("SLS", ", ".join("{%d, %dull}" % s for s in sls))
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "audit.cpp"), os.path.join(tmp, "audit")
        open(cpp, "w").write(src)
        flags = ["-std=c++17", "-O1", "-fsanitize=signed-integer-overflow", "-fsanitize-trap=signed-integer-overflow", "-Wno-unused-variable", "-Wno-unused-function"]
        r = subprocess.run([_compiler(), *flags, "-I", CSRC, cpp, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:])
    assert int(re.search(r"^range (\d+)$", r.stdout, re.M).group(1)) == OOB
    got = dict((int(i), (v, int(n))) for i, v, n in re.findall(r"^fit (\d+) (\d\d\d) (-?\d+)$", r.stdout, re.M))
    assert len(got) == len(fits)
    for j, (B, H, W, C0, C1, e) in enumerate(fits):
        ok = B * H * W * max(C0, C1) * e < OOB
        panel = H * (C0 + C1) * W * B * e < OOB             # (the audit program's stand-in: ntaps = H, N = W, B e bytes per (k, n))
        assert got[j] == ("%d%d%d" % (ok, ok, panel), _slice_frames(B, H * W * max(C0, C1) * e)), (fits[j], got[j])
    assert 0 < sum(v[0] == "1" for v, _ in got.values()) < len(fits) and {n for _, n in got.values()} >= {-1, 0, 2, 23}
    got = dict((int(i), int(v)) for i, v in re.findall(r"^slice (\d+) (-?\d+)$", r.stdout, re.M))
    assert len(got) == len(sls)
    for j, (B, per) in enumerate(sls):
        assert got[j] == _slice_frames(B, per), (sls[j], got[j])
    assert {-1, 0, 1, 2, 47} <= set(got.values())


DIRECT_SOURCES = ("conv_igemm.hip", "conv_igemm_split.hip", "conv_igemm_bf16.hip", "up4_head_bf16.hip", "bf16_ops.hip", "conv_wgrad.hip")
DIRECT_HEADER = "lwg_conv_direct.h"


def test_direct_family_uses_the_shared_header():
    """The converse of the audit: the direct family spells no buffer-range limit, dynamic-LDS opt-in state, CU cache or slicing loop of its own, and
    every sliced entry point runs the one preamble."""
    h = _code(DIRECT_HEADER)
    assert h.count("0xC0000000ull") == 1 and "static inline bool lwg_buf_fits(unsigned long long bytes) { return bytes < LWG_BUF_RANGE; }" in h
    for name in DIRECT_SOURCES + ("conv_wgrad_winograd.hip", "lwb_attn.hip", "lwb_attn_x.hip"):
        k = _code(name)
        own = name.startswith("lwb_attn")             # (the attention kernels keep their own launch macro)
        for word in ("0xC0000000ull", "static unsigned long long attr_done", "lwg_conv_run_sliced(", "lwg_allow_dynamic_lds", "hipDeviceAttributeMultiprocessorCount")[:1 if own else 5]:
            assert word not in k, (name, word)
    for name in DIRECT_SOURCES:
        assert '#include "%s"' % DIRECT_HEADER in _code(name), name
    sliced = {"conv_igemm.hip": ("lwg_conv2d_nhwc_f32_ws(&s, nullptr, stream_)", "lwg_conv_transpose4_nhwc_f32(&s, stream_)"),
              "conv_igemm_split.hip": ("lwg_conv2d_nhwc_f32_split(&s, stream_)",),
              "conv_igemm_bf16.hip": ("lwg_conv_transpose4_nhwc_bf16(&s, stream_)", "lwg_conv2d_nhwc_c8_bf16(&s, stream_)", "lwg_conv2d_nhwc_bf16_hr(&s, stream_)",
                                      "lwg_conv2d_nhwc_bf16(&s, stream_)")}
    for name, selves in sliced.items():
        k = _code(name)
        assert k.count("cd_sliced(a, ") == len(selves), name
        for s in selves:
            assert re.search(r"cd_sliced\(a, \[&\]\(const LwgConvArgs& s\) \{ return [^;]*" + re.escape(s), k), (name, s)
    for name, n in (("conv_igemm.hip", 1), ("conv_igemm_split.hip", 1), ("conv_igemm_bf16.hip", 2)):
        assert _code(name).count("cd_epi_dispatch(a, ") == n, name
    assert "lwg_slice_frames(a.B, per)" in _code("up4_head_bf16.hip") and "lwg_slice_frames(B, per)" in _code("bf16_ops.hip")
