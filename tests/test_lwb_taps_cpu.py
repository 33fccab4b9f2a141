"""Host audit of csrc/lwg_lwb_taps.h: the flow resize (indices, weights, four-texel blend), the bilinear taps of a flow value, the per-tap
zero-padding predicate and the linear pixel decode of the Liquid Warping Block kernels (csrc/lwb_attn.hip, csrc/bf16_ops.hip,
csrc/lwb_attn_x.hip, csrc/spade_skip.hip).  No GPU.

A small C++ program INCLUDES the header - the functions the kernels compile - and is built with -ffp-contract=off and with traps on signed
integer overflow and on float -> int conversions that do not fit (the clamp before the int conversion is what keeps +-1e30 flows legal).
It evaluates, for every flow family of tests/attn_flows.py (``wild`` included) on the geometries of attn_flows.GEOMETRIES plus the
upsampling shape (S = 5, 9 x 13), per pixel and source: the linear pixel decode, the resize struct, the resized flow, the top-left tap, the
four weights, the four per-tap pixels and in-image bits and the "touches the image" predicate - once through the resize from the S x S field
(the attention / fusion kernels) and once on a field stored at (h, w) (the x-form and the SPADE skip classifier).  Everything is compared
with the fp32 torch evaluation of the same expressions: unfused elementwise fp32 is what -ffp-contract=off compiles, so integers, bits,
weights and flows must agree exactly.

The kernels that resize the flow field themselves (lwb_attn.hip, bf16_ops.hip) keep their own copy of the blend and of the coordinate /
clamp / weight expressions, four of them also of the index arithmetic (through the header's functions the compiler
contracts the blend differently and their results leave the recorded bits); test_kernel_copies_are_the_header_text holds every copy to
the header's expression text."""
import os
import re
import subprocess
import tempfile

import numpy as np
import torch

from tests import attn_flows as af
from tests.test_conv_offsets_cpu import CSRC, _code, _compiler

HEADER = "lwg_lwb_taps.h"
FAMILY_SOURCES = ("lwb_attn.hip", "bf16_ops.hip", "lwb_attn_x.hip", "spade_skip.hip")
SHAPES = tuple(g[1:] for g in af.GEOMETRIES) + ((2, 5, 9, 13),)          # (ns, S, h, w); one frame each
NI, NF = 19, 10                                                             # int and float words per (source, pixel) record

_PROGRAM = r"""
#include "lwg_lwb_taps.h"
#include <cstdio>
#include <vector>
// in:  int32 ncases, then per case int32 {n, S, h, w, direct} and n * (direct ? h * w : S * S) float2
// out: per case, field and pixel 19 int32 {tx0, ty0, bits, tx[4], ty[4], f, y, x, y0, x0, y1, x1, same} + 10 float {wt[4], ly0, ly1, lx0, lx1, gx, gy}
int main(int argc, char** argv) {
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    int ncases = 0;
    if (!in || !out || fread(&ncases, 4, 1, in) != 1) return 2;
    for (int c = 0; c < ncases; ++c) {
        int hd[5];
        if (fread(hd, 4, 5, in) != 5) return 2;
        const int n = hd[0], S = hd[1], h = hd[2], w = hd[3], direct = hd[4];
        const size_t per = direct ? (size_t)h * w : (size_t)S * S;
        std::vector<float2> T(n * per);
        if (fread(T.data(), sizeof(float2), T.size(), in) != T.size()) return 2;
        for (long gp = 0; gp < (long)n * h * w; ++gp) {
            int iw[19] = {0};
            float fw[10] = {0.f};
            lwb_pixel_of(gp, h, w, iw[11], iw[12], iw[13]);
            const int f = iw[11], y = iw[12], x = iw[13];
            float2 g;
            if (direct) {
                g = T[gp];
            } else {
                const LwbResize r = lwb_resize_of(y, x, h, w, S);
                iw[14] = r.y0; iw[15] = r.x0; iw[16] = r.y1; iw[17] = r.x1; iw[18] = r.same;
                fw[4] = r.ly0; fw[5] = r.ly1; fw[6] = r.lx0; fw[7] = r.lx1;
                g.x = g.y = 0.f;
                // (indices outside the field are reported, not dereferenced)
                if (r.y0 >= 0 && r.y0 <= r.y1 && r.y1 < S && r.x0 >= 0 && r.x0 <= r.x1 && r.x1 < S) g = lwb_flow_at(T.data() + (size_t)f * per, r, y, x, S);
            }
            fw[8] = g.x; fw[9] = g.y;
            lwb_taps_of(g, w, h, *reinterpret_cast<float (*)[4]>(fw), iw[0], iw[1]);
            for (int t = 0; t < 4; ++t)
                if (lwb_tap(t, iw[0], iw[1], w, h, iw[3 + t], iw[7 + t])) iw[2] |= 1 << t;
            if (lwb_tap_in_image(iw[0], iw[1], w, h)) iw[2] |= 16;
            fwrite(iw, 4, 19, out);
            fwrite(fw, 4, 10, out);
        }
    }
    fclose(out);
    return 0;
}
"""


def _cases():
    """(family, ns, S, h, w, direct, field): every family through the resize from S x S (direct 0) and stored at (h, w) (direct 1)."""
    out = []
    for ns, S, h, w in SHAPES:
        for fam in af.FAMILIES:
            out.append((fam, ns, S, h, w, 0, af.flows(fam, 1, ns, S, S, seed=0, size=(h, w))[0]))
            out.append((fam, ns, S, h, w, 1, af.flows(fam, 1, ns, h, w, seed=0)[0]))
    return out


def _run(cases):
    with tempfile.TemporaryDirectory() as d:
        cpp, exe, fin, fout = (os.path.join(d, n) for n in ("audit.cpp", "audit", "in.bin", "out.bin"))
        open(cpp, "w").write(_PROGRAM)
        with open(fin, "wb") as fp:
            fp.write(np.int32(len(cases)).tobytes())
            for _, ns, S, h, w, direct, T in cases:
                fp.write(np.array([ns, S, h, w, direct], dtype=np.int32).tobytes())
                fp.write(T.numpy().astype(np.float32).tobytes())
        checks = "signed-integer-overflow,float-cast-overflow"
        flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=" + checks, "-fsanitize-trap=" + checks]
        r = subprocess.run([_compiler(), *flags, "-I", CSRC, cpp, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
        assert r.returncode >= 0, "an int conversion or an index expression of lwg_lwb_taps.h overflowed (trapped)"
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:])
        words = np.fromfile(fout, dtype=np.int32)
    out, pos = [], 0
    for _, ns, S, h, w, direct, T in cases:
        n = ns * h * w
        rec = words[pos:pos + n * (NI + NF)].reshape(ns, h, w, NI + NF)
        pos += n * (NI + NF)
        out.append((torch.from_numpy(rec[..., :NI].copy()), torch.from_numpy(rec[..., NI:].copy().view(np.float32))))
    assert pos == words.size
    return out


def _f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def _torch_resize(T, S, h, w):
    """lwb_resize_of and lwb_flow_at in unfused fp32 torch arithmetic: T (ns,S,S,2) -> the struct's fields (h,w) and the flow (ns,h,w,2)."""
    sc_y = _f32(S - 1) / _f32(h - 1) if h > 1 else _f32(0)
    sc_x = _f32(S - 1) / _f32(w - 1) if w > 1 else _f32(0)
    sy = (sc_y * torch.arange(h, dtype=torch.float32)).view(h, 1).expand(h, w)
    sx = (sc_x * torch.arange(w, dtype=torch.float32)).view(1, w).expand(h, w)
    y0, x0 = sy.to(torch.int32), sx.to(torch.int32)
    y1, x1 = y0 + (y0 < S - 1).to(torch.int32), x0 + (x0 < S - 1).to(torch.int32)
    ly1, lx1 = sy - y0.float(), sx - x0.float()
    ly0, lx0 = 1.0 - ly1, 1.0 - lx1
    same = h == S and w == S
    if same:
        g = T.clone()
    else:
        yc0, yc1, xc0, xc1 = (v.long().clamp(0, S - 1) for v in (y0, y1, x0, x1))       # (a wrong index fails its own assertion)
        t00, t01, t10, t11 = T[:, yc0, xc0], T[:, yc0, xc1], T[:, yc1, xc0], T[:, yc1, xc1]
        e = lambda v: v.unsqueeze(-1)        # noqa: E731
        g = e(ly0) * (e(lx0) * t00 + e(lx1) * t01) + e(ly1) * (e(lx0) * t10 + e(lx1) * t11)
    return (y0, x0, y1, x1, ly0, ly1, lx0, lx1, same), g


def _torch_taps(g, h, w):
    """lwb_taps_of / lwb_tap / lwb_tap_in_image in unfused fp32 torch arithmetic on a flow g (..., 2)."""
    ix = ((g[..., 0] + 1.0) * float(w) - 1.0) * 0.5
    iy = ((g[..., 1] + 1.0) * float(h) - 1.0) * 0.5
    fx0, fy0 = ix.floor(), iy.floor()
    wx1, wy1, wx0, wy0 = ix - fx0, iy - fy0, (fx0 + 1.0) - ix, (fy0 + 1.0) - iy
    tx0 = torch.minimum(torch.maximum(fx0, _f32(-2)), _f32(w) + 1.0).to(torch.int32)
    ty0 = torch.minimum(torch.maximum(fy0, _f32(-2)), _f32(h) + 1.0).to(torch.int32)
    wt = torch.stack([wy0 * wx0, wy0 * wx1, wy1 * wx0, wy1 * wx1], dim=-1)
    tx = torch.stack([tx0 + (t & 1) for t in range(4)], dim=-1)
    ty = torch.stack([ty0 + (t >> 1) for t in range(4)], dim=-1)
    inside = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
    return tx0, ty0, wt, tx, ty, inside


def _bits(a):
    return a.contiguous().view(torch.int32)


def test_header_agrees_with_fp32_torch_on_every_flow_family():
    """The program ends without a trap, and every value it wrote equals the fp32 torch evaluation: the pixel decode, the resize struct's
    indices, tx0 / ty0, the tap pixels and the in-image bits exactly, the resize weights, the resized flow and the tap weights bitwise;
    lwb_tap_in_image is the OR of the four per-tap bits; 0 <= y0 <= y1 <= S - 1 and the same in x (h = 1 and S < h included); the resized
    flow is within RESIZE_TOL * S * max(1, max |T|) of the fp64 reference and is the field itself where S == h == w."""
    cases = _cases()
    assert {c[0] for c in cases} == set(af.FAMILIES) and any(c[3] == 1 for c in cases) and any(c[2] < c[3] for c in cases)
    seen_out, seen_in, seen_wild, seen_held = 0, 0, 0, 0
    for (fam, ns, S, h, w, direct, T), (iw, fw) in zip(cases, _run(cases)):
        key = (fam, ns, S, h, w, direct)
        f_, y_, x_ = torch.meshgrid(torch.arange(ns), torch.arange(h), torch.arange(w), indexing="ij")
        assert torch.equal(iw[..., 11:14], torch.stack([f_, y_, x_], dim=-1).to(torch.int32)), ("pixel decode", key)
        if direct:
            g = T
        else:
            (y0, x0, y1, x1, ly0, ly1, lx0, lx1, same), g = _torch_resize(T, S, h, w)
            assert (0 <= iw[..., 14]).all() and (iw[..., 14] <= iw[..., 16]).all() and (iw[..., 16] <= S - 1).all(), ("0 <= y0 <= y1 <= S - 1", key)
            assert (0 <= iw[..., 15]).all() and (iw[..., 15] <= iw[..., 17]).all() and (iw[..., 17] <= S - 1).all(), ("0 <= x0 <= x1 <= S - 1", key)
            for nm, col, want in (("y0", 14, y0), ("x0", 15, x0), ("y1", 16, y1), ("x1", 17, x1)):
                assert torch.equal(iw[..., col], want.expand(ns, h, w)), (nm, key)
            assert (iw[..., 18] == int(same)).all(), ("same", key)
            for nm, col, want in (("ly0", 4, ly0), ("ly1", 5, ly1), ("lx0", 6, lx0), ("lx1", 7, lx1)):
                assert torch.equal(_bits(fw[..., col]), _bits(want.expand(ns, h, w))), (nm, key)
            err = (fw[..., 8:10].double() - af.ref_flow_resize(T.unsqueeze(0), h, w)[0]).abs().max().item()
            assert err <= af.RESIZE_TOL * S * max(1.0, T.abs().max().item()), ("flow against fp64", key, err)
            if same:
                assert torch.equal(_bits(fw[..., 8:10]), _bits(T)), ("the S == h == w flow is the field itself", key)
            seen_held += int(((iw[..., 14] == S - 1) & (iw[..., 16] == S - 1)).sum())
        assert torch.equal(_bits(fw[..., 8:10]), _bits(g)), ("flow", key)
        tx0, ty0, wt, tx, ty, inside = _torch_taps(g, h, w)
        assert torch.equal(iw[..., 0], tx0) and torch.equal(iw[..., 1], ty0), ("tx0 / ty0", key)
        assert torch.equal(_bits(fw[..., 0:4]), _bits(wt)), ("weights", key)
        assert torch.equal(iw[..., 3:7], tx) and torch.equal(iw[..., 7:11], ty), ("tap pixels", key)
        got_in = torch.stack([(iw[..., 2] >> t) & 1 for t in range(4)], dim=-1).bool()
        assert torch.equal(got_in, inside), ("per-tap in-image bits", key)
        assert torch.equal(((iw[..., 2] >> 4) & 1).bool(), got_in.any(dim=-1)), ("lwb_tap_in_image is the OR of the four taps", key)
        seen_out += int((~inside).sum())
        seen_in += int(inside.sum())
        seen_wild += int((g.abs() > 1e20).sum())
    # the cases reach both sides of the padding rule, the clamp, and the last row of the field (y1 held at S - 1)
    assert seen_out > 1000 and seen_in > 1000 and seen_wild > 100 and seen_held > 100


# the header's expressions as the in-kernel copies spell them (the copies name the flow value gx / gy, the header t.x / t.y)
_COPY_TEXT = ("const float ix = ((gx + 1.f) * (float)w - 1.f) * 0.5f, iy = ((gy + 1.f) * (float)h - 1.f) * 0.5f;",
              "const float fx0 = floorf(ix), fy0 = floorf(iy);",
              "(int)fminf(fmaxf(fx0, -2.f), (float)w + 1.f)", "(int)fminf(fmaxf(fy0, -2.f), (float)h + 1.f)",
              "ix - fx0", "iy - fy0", "(fx0 + 1.f) - ix", "(fy0 + 1.f) - iy")
_COPIES = {"lwb_attn.hip": 3, "bf16_ops.hip": 1}          # attention forward, attention backward, lwg_fuse_taps | the position lambda
_PREDICATE = "ty >= 0 && ty < h && tx >= 0 && tx < w"
# the resize: index / weight arithmetic (the header writes into its struct r) and the blend (lwg_flow_resize_kernel and lwg_fuse_taps read a struct r too)
_RESIZE_TEXT = ("sc_y = h > 1 ? (float)(S - 1) / (float)(h - 1) : 0.f;", "sc_x = w > 1 ? (float)(S - 1) / (float)(w - 1) : 0.f;",
                "sy = sc_y * (float)y, sx = sc_x * (float)x;", "(int)sy", "(int)sx", "y0 + (y0 < S - 1 ? 1 : 0)", "x0 + (x0 < S - 1 ? 1 : 0)",
                "sy - (float)y0", "sx - (float)x0", "1.f - ly1", "1.f - lx1")
_BLEND_TEXT = ("Tp[(size_t)y0 * S + x0], t01 = Tp[(size_t)y0 * S + x1];", "Tp[(size_t)y1 * S + x0], t11 = Tp[(size_t)y1 * S + x1];",
               "= ly0 * (lx0 * t00.x + lx1 * t01.x) + ly1 * (lx0 * t10.x + lx1 * t11.x);", "= ly0 * (lx0 * t00.y + lx1 * t01.y) + ly1 * (lx0 * t10.y + lx1 * t11.y);")
_RESIZE_COPIES = {"lwb_attn.hip": 3, "bf16_ops.hip": 1}    # attention forward, lwg_flow_resize_kernel, attention backward (the fusion kernels: lwb_resize_of) | bf16 attention
_BLEND_COPIES = {"lwb_attn.hip": 4, "bf16_ops.hip": 1}     # ... and lwg_fuse_taps


def test_kernel_copies_are_the_header_text():
    """The header holds the family's expressions; the kernels of lwb_attn_x.hip and spade_skip.hip call it for everything, those of
    lwb_attn.hip and bf16_ops.hip for the pixel decode and the per-tap predicate of their pointer and scatter loops.  Their coordinate /
    clamp / weight copies (three and one), their copies of the resize index arithmetic (three and one; the fusion kernels call
    lwb_resize_of) and of the four-texel blend (four and one) carry the header's expression text verbatim, nothing else in them floors or
    clamps a coordinate or scales by S - 1, and the predicate is spelled out only in the two buffer-load loops (kept inline: see there)."""
    h = _code(HEADER)
    for fn in ("lwb_taps_of(const float2 t, int w, int h, float (&wt)[4], int& tx0, int& ty0)", "lwb_tap_in_image(int tx0, int ty0, int w, int h)",
               "lwb_tap(int t, int tx0, int ty0, int w, int h, int& tx, int& ty)", "lwb_pixel_of(long gp, int h, int w, int& b, int& y, int& x)",
               "LwbResize lwb_resize_of(int y, int x, int h, int w, int S)", "float2 lwb_flow_at(const float2* __restrict__ Tp, const LwbResize& r, int y, int x, int S)"):
        assert fn in h, fn
    for word in ("__shfl", "threadIdx", "__builtin_amdgcn", "hipLaunch"):
        assert word not in h, word
    hx = h.replace("t.x", "gx").replace("t.y", "gy")
    for text in _COPY_TEXT + (_PREDICATE,):
        assert hx.count(text) == 1, text
    unstruct = lambda code: re.sub(r"\br\.", "", code)        # noqa: E731
    for text in _RESIZE_TEXT + _BLEND_TEXT:
        assert unstruct(h).count(text) == 1, text
    for name in FAMILY_SOURCES:
        k = _code(name)
        assert '#include "%s"' % HEADER in k, name
        for word in ("rem / w", "lwg_pack_bf16x2", "lwg_fuse_widen8", "lwg_pack2", "lwg_unpack8", "lwg_fuse_uintx4"):
            assert word not in k, (name, word)
        n = _COPIES.get(name, 0)
        for text in _COPY_TEXT:
            assert k.count(text) == n, (name, text, k.count(text))
        assert k.count("floorf(i") == 2 * n and k.count("fmaxf(f") == 2 * n, name
        assert k.count(_PREDICATE) == (1 if n else 0), name
        for text in _RESIZE_TEXT:
            assert unstruct(k).count(text) == _RESIZE_COPIES.get(name, 0), (name, text, unstruct(k).count(text))
        for text in _BLEND_TEXT:
            assert unstruct(k).count(text) == _BLEND_COPIES.get(name, 0), (name, text, unstruct(k).count(text))
        assert k.count("(S - 1)") == 2 * _RESIZE_COPIES.get(name, 0) and k.count("lx0 *") == 4 * _BLEND_COPIES.get(name, 0), name
        for word in ("LwgFuseResize", "lwg_fuse_resize"):
            assert word not in k, (name, word)
    assert _code("lwb_attn.hip").count("lwb_resize_of(y, x, h, w, S)") == 3
    for name in _COPIES:
        k = _code(name)
        assert "lwb_tap(t, " in k and "lwg_lpp_dispatch<" in k and "switch (C)" not in k and "_LAUNCH(" not in k, name
