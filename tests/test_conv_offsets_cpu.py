"""CPU checks of the 32-bit buffer offsets of the fp32 Winograd convolutions at the edges of their host contracts.

The kernels address an image as ONE raw buffer: a byte offset is 32 bits, and an access that must not happen (a padding tap, a pixel right of or below
the image) gets the marker 0xC0000000 - at or beyond any image's size, so the hardware drops the store / returns zeros for the load.  That holds only
while every offset the kernel forms - the marker plus a per-pass or per-stage increment included - stays within 32 bits, and while the C++
expressions that form the offsets do not overflow their own types.

The audit below compiles the kernels' own offset arithmetic into a host program with signed-overflow traps - the transposed kernels' by INCLUDING
csrc/lwg_convt_wino.h, whose integer functions are what both kernels compile; the 3 x 3 kernels' expressions cut VERBATIM out of their sources -
and evaluates it for the corner shapes the host contracts accept: the widest output rows at the
fewest rows, the tallest images at one or two pixels of width, images just under the size limits, widths and heights that are not multiples of the
tile.  Every kept access must land at its own pixel and channel; every dropped one at or beyond the buffer's size modulo 2^32.

The host-limit test checks, per entry point, that the smallest shape over each size limit returns 1 before any launch."""
import os
import re
import shutil
import subprocess
import sys
import tempfile
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ipercore_amd", "csrc")
OOB = 0xC0000000


def _src(name):
    text = open(os.path.join(CSRC, name)).read()
    return re.sub(r"//[^\n]*", "", text)                    # comments out: statements are cut at ';' on paren depth 0


def _stmts(text):
    """The statements of a piece of C++ (split at ';' outside parentheses), whitespace-normalised."""
    out, depth, cur = [], 0, []
    for ch in text:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == ";" and depth == 0:
            out.append(" ".join("".join(cur).split()))
            cur = []
        else:
            cur.append(ch)
    return [s.lstrip("{} ").strip() for s in out]


def _call_args(text, fname):
    """Argument texts of the first call of fname in text."""
    i = text.index(fname + "(") + len(fname) + 1
    depth, cur, args = 0, [], []
    while True:
        ch = text[i]
        i += 1
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            if depth == 0:
                args.append(" ".join("".join(cur).split()))
                return args
            depth -= 1
        if ch == "," and depth == 0:
            args.append(" ".join("".join(cur).split()))
            cur = []
        else:
            cur.append(ch)


def _code(name):
    """csrc/<name> without its comments."""
    return _src(name)


CONVT_KERNELS = ("convt_winograd.hip", "convt_winograd24.hip")
CONVT_HEADER = "lwg_convt_wino.h"


def _w4_exprs():
    s = _src("conv_winograd4.hip")
    vo = re.search(r"vo\[hp\]\[i\] = (.*?);", s, re.S).group(1)
    st = _call_args(s[s.index("__builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(w4_u4, o[i])"):], "__builtin_amdgcn_raw_buffer_store_b128")
    ld = _call_args(s[s.index("ext[h][i] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(re"):], "__builtin_amdgcn_raw_buffer_load_b128")
    return " ".join(vo.split()), st[2], st[3], ld[1], ld[2]


def _halo_exprs():
    """(kernel, input 0 / 1, offset expression) of the 3 x 3 Winograd kernels' halo loads (the transposed kernels': ctw_halo_voff of the header)."""
    out = []
    for name, var in (("conv_winograd.hip", "q"), ("conv_winograd4.hip", "k")):
        s = _src(name)
        for inp in ("0", "1"):
            m = re.search(r"voff%s\[%s\] = (in \?.*?);" % (inp, var), s, re.S)
            if m:
                out.append((name, inp, " ".join(m.group(1).split())))
    return out


def _halo_soffsets():
    """The stage's channel offset of every halo load: the scalar offset argument, as written in each kernel."""
    got = {}
    for name in ("conv_winograd.hip", "conv_winograd4.hip"):
        s = _src(name)
        r = s[s.index("auto rld1"):]
        fn = re.search(r"(\w+_buf_load\w*)\(rx0, voff0\[\w\], ", r).group(1)
        got[name] = _call_args(r, fn)[2]
    return got


def test_offset_expressions_are_found():
    """The audit below reads what it checks out of the kernels: the expressions it cuts out must be there, in the forms it knows how to drive.  The
    transposed kernels are audited through the shared header, so the converse is checked here: neither kernel forms a store or halo offset of its
    own, and both run the header's block walk, halo staging and store phase."""
    h = _code(CONVT_HEADER)
    st = _call_args(h, "__builtin_amdgcn_raw_buffer_store_b128")
    assert st[2].startswith("(int)ctw_store_voff(") and "pass" in st[2] and st[3] == "0", st       # pass offsets in the VECTOR offset (test_no_wide_buffer_store_with_register_soffset)
    assert "ctw_store_thread(q4, tide, ex0, ey0, a.ycoff, en0, a.YH, a.YW, a.YC)" in h
    assert "ctw_buf_load(rx0, voff0[q], ctw_halo_soff(st))" in h and "voff0[q] = ctw_halo_voff(tid + WG_THREADS * q, x0, y0, a.H, a.W, a.C0)" in h
    assert "ctw_has_block(o, id)" in h and "!ctw_contract_ok(*pa, pair_bytes, panel_limit)" in h
    for name in CONVT_KERNELS:
        k = _code(name)
        for word in ("raw_buffer_store", "make_buffer_rsrc(a.y", "make_buffer_rsrc(const_cast<float*>(a.x0", "WINO_OOB", "auto has_block", "hipLaunchKernelGGL"):
            assert word not in k, (name, word)
        assert '#include "%s"' % CONVT_HEADER in k, name
        for call in ("CtwBlock<", "bk.setup(a, tid, id)", "bk.has_block(nblk)", "bk.rld1(", "bk.rst1(raw0, ", "ctw_store_block<", "return ctw_launch("):
            assert call in k, (name, call)
    vo, st_off, st_soff, ld_off, ld_soff = _w4_exprs()
    assert "W4_OOB" in vo and st_soff == "0" and ld_soff == "0"
    assert len(_halo_exprs()) == 4                                       # two inputs in each of the two 3 x 3 kernels
    so = _halo_soffsets()
    assert so == {"conv_winograd.hip": "(unsigned)c * 4u", "conv_winograd4.hip": "(unsigned)c * 4u"}, so
    assert "CTW_FN unsigned ctw_halo_soff(int st) { return (unsigned)(st * KS) * 4u; }" in h


# ---- host contracts (restated from the entry points; test_host_limits_at_the_boundary checks them against the library) ----

def _convt_ok(H, W, C0, YC):
    return H * W * C0 * 4 < OOB and (2 * H) * (2 * W) * YC * 4 + 32 * (2 * W) * YC * 4 < OOB


def _w4_ok(H, W, C, YC):
    return H * W * C * 4 < OOB and H * W * YC * 4 + 256 < OOB


def _wmax(ok, H, *rest):
    """Largest W the contract ok accepts at height H."""
    lo, hi = 1, 1 << 31
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(H, mid, *rest) else (lo, mid)
    return lo


def _hmax(ok, W, *rest):
    lo, hi = 1, 1 << 31
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid, W, *rest) else (lo, mid)
    return lo


def _convt_shapes():
    """(H, W, Cin, N, YC, ycoff) the transposed kernels' contract accepts, at its corners."""
    out = [(4, 150001, 16, 32, 64, 32)]                                 # 0.57 GiB: the pass offsets of dropped stores reach 1 GiB
    for YC, N in ((32, 32), (64, 32), (64, 64), (256, 64)):
        for H in (1, 2, 3, 4):
            W = _wmax(_convt_ok, H, 16, YC)
            out += [(H, W, 16, N, YC, YC - N), (H, W - (W - 1) % 16, 16, N, YC, 0)]
        for W in (1, 2, 3):
            H = _hmax(_convt_ok, W, 16, YC)
            out += [(H, W, 16, N, YC, YC - N), (H - 5, W, 16, N, YC, 0)]
    for H in (1000, 1201, 1917):                                        # square-ish images just under the limit (> 2 GiB of output)
        W = _wmax(_convt_ok, H, 64, 64)
        out += [(H, W, 64, 64, 64, 0), (H, W - 7, 64, 32, 64, 32)]
    for sh in out:
        assert _convt_ok(sh[0], sh[1], sh[2], sh[4]) and sh[3] + sh[5] <= sh[4], sh
    return out


def _w4_shapes():
    """(H, W, C, N, YC, ycoff) of the F(4x4, 3x3) kernel's contract, at its corners."""
    out = []
    for YC, N in ((64, 64), (128, 64), (256, 256)):
        for H in (1, 2, 5):
            W = _wmax(_w4_ok, H, 64, YC)
            out += [(H, W, 64, N, YC, YC - N), (H, W - (W - 1) % 16, 64, N, YC, 0)]
        for W in (1, 3):
            out.append((_hmax(_w4_ok, W, 64, YC), W, 64, N, YC, YC - N))
        W = 3001
        out.append((_hmax(_w4_ok, W, 64, YC), W, 64, N, YC, 0))
    return out


# the transposed kernels through csrc/lwg_convt_wino.h: the store phase of a block (32 x 32 output pixels x 32 channels; 512 threads x 16 passes), its
# halo (512 threads x 2 elements x every stage), the block walk of a launch, the host contract
_CONVT = r"""
#include "lwg_convt_wino.h"
#include <vector>
template <bool Q4>
static void convt_store(const Args& a, int ex0, int ey0, int en0) {
    const int oy0 = 2 * ey0, ox0 = 2 * ex0;
    const size_t plane = (size_t)a.YH * a.YW;
    const u64 size = (u64)plane * a.YC * 4ull;
    static unsigned char seen[32 * 32 * 8];
    for (unsigned char& v : seen) v = 0;
    for (int tide = 0; tide < 512; ++tide) {
        const CtwStore s = ctw_store_thread(Q4, tide, ex0, ey0, a.ycoff, en0, a.YH, a.YW, a.YC);
        for (int pass = 0; pass < 16; ++pass) {
            const int ly = s.lyh + 2 * pass;
            if (ly < 0 || ly >= 32 || s.lx < 0 || s.lx >= 32 || s.cq < 0 || s.cq >= 8 || seen[(ly * 32 + s.lx) * 8 + s.cq]++) {       // every output of the block once
                if (bad++ < 8) printf("BAD %s tide=%d pass=%d: pixel (%d, %d) quad %d out of the block or stored twice\n", where, tide, pass, s.lx, ly, s.cq);
                continue;
            }
            const int row = oy0 + ly, col = ox0 + s.lx, ch = a.ycoff + en0 + 4 * s.cq;
            const bool keep = row < a.YH && col < a.YW;
            const u64 want = Q4 ? (((u64)(ch / 4) * plane + (u64)row * a.YW + col) * 16ull) : (((u64)row * a.YW + col) * a.YC + ch) * 4ull;
            check(keep, ctw_store_voff(Q4, s, pass, ey0, a.YH), 0u, want, size, col, row, ch);       // (scalar offset: the constant 0 of ctw_store_block)
        }
    }
}

static void convt_halo(const Args& a, int x0, int y0, int) {
    const u64 size = (u64)a.H * a.W * a.C0 * 4ull;
    for (int i = 0; i < 2 * WG_THREADS; ++i) {
        const unsigned v = ctw_halo_voff(i, x0, y0, a.H, a.W, a.C0);
        const int half = i % 2, gy = y0 - 1 + (i / 2) / 18, gx = x0 - 1 + (i / 2) % 18;
        const bool in = i < 2 * 18 * 18 && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
        for (int st = 0; st < a.C0 / 8; ++st) {
            const u64 want = in ? (((u64)gy * a.W + gx) * a.C0 + 4 * half + 8 * st) * 4ull : 0ull;
            check(in, v, ctw_halo_soff(st), want, size, gx, gy, 8 * st + 4 * half);
        }
        // LDS: the element's four channels at slot + k PLANE inside raw[u]; the threads without one at their own dump slot
        const int slot = ctw_halo_slot(i, 1 << 20);
        if (i < 2 * 18 * 18 ? slot != 4 * half * 324 + (i / 2) || slot + 3 * 324 >= RAW_FLOATS : slot != 1 << 20)
            if (bad++ < 8) printf("BAD %s halo slot of element %d: %d\n", where, i, slot);
    }
}

// every workgroup's walk over a launch of nwg workgroups: each (column block, tile) exactly once, inside the grid; no block behind the last one
static void convt_walk(int B, int H, int W, int N, unsigned nwg, bool xcd_on) {
    const CtwGrid g = ctw_grid(B, H, W, N);
    if ((long)nwg > ctw_total_blocks(B, H, W, N)) nwg = (unsigned)g.total;             // (the launch: min(blocks, CUs) workgroups)
    std::vector<int> seen((size_t)g.total, 0);
    u64 fails = 0;
    for (unsigned wg = 0; wg < nwg; ++wg) {
        const CtwOrder o = ctw_order(xcd_on, nwg, wg, N, g);
        if (o.xcd != (xcd_on && ctw_xcd_applies(nwg, N / 32, g.tiles, g.total))) ++fails;
        int id = (int)wg;
        do {                                                                           // (the first block is taken unconditionally, as the kernels do)
            const int cb = ctw_col_block(o, id), t = ctw_tile(o, id, cb), b = ctw_image(g, t);
            int x0, y0, n0;
            ctw_corner(g, t - b * g.bx * g.by, cb, x0, y0, n0);
            if (cb < 0 || cb >= N / 32 || t < 0 || t >= g.tiles || b < 0 || b >= B || x0 < 0 || x0 >= W || y0 < 0 || y0 >= H || x0 % 16 || y0 % 16 || n0 != 32 * cb) ++fails;
            else ++seen[(size_t)cb * g.tiles + t];
            ++walked;
            id += (int)nwg;
        } while (ctw_has_block(o, id));
        for (int k = 1; k < 4; ++k) if (ctw_has_block(o, id + k * (int)nwg)) ++fails;
    }
    for (int v : seen) if (v != 1) ++fails;
    if (fails) { bad += fails; printf("BAD walk B=%d H=%d W=%d N=%d nwg=%u xcd=%d: %llu\n", B, H, W, N, nwg, (int)xcd_on, fails); }
}

static int convt_contract(int B, int H, int W, int C0, int N, int YC, int ydt, u64 pair_bytes, u64 panel_limit) {
    static float dummy;
    LwgConvArgs a = {};
    a.x0 = a.w = &dummy; a.y = &dummy;
    a.B = B; a.H = a.OH = H; a.W = a.OW = W; a.C0 = C0; a.N = N; a.M = B * H * W;
    a.YH = 2 * H; a.YW = 2 * W; a.YC = YC; a.ntaps = 4; a.stride = 1; a.omul = 2; a.ydt = ydt;
    return (int)ctw_contract_ok(a, pair_bytes, panel_limit);
}
"""

_HARNESS = r"""
#include <cstdio>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#define W4_OOB 0xC0000000u
#define W4_KS 8
struct Args { int H, W, C0, C1, N, YH, YW, YC, ycoff; };
typedef unsigned long long u64;
static u64 kept = 0, dropped = 0, bad = 0, walked = 0;
static const char* where = "";
// every access: kept ones at want (inside the image); dropped ones at or beyond the buffer's size modulo 2^32
static void check(bool keep, unsigned voff, unsigned soff, u64 want, u64 size, int x, int y, int c) {
    const unsigned off = voff + soff;
    bool ok;
    if (keep) { ok = want < size && (u64)off == want; ++kept; }
    else { ok = (u64)off >= size && (u64)voff >= size; ++dropped; }
    if (!ok && bad++ < 8)
        printf("BAD %s keep=%d x=%d y=%d c=%d off=%u want=%llu size=%llu\n", where, (int)keep, x, y, c, off, (unsigned long long)want, size);
}

@CONVT@

// the F(4x4, 3x3) kernel's output pixels (stores; residual / SPADE epilogue loads): one pixel (ox, oyb + i), channel group chan (+ 32 h)
template <int EPI, bool SM>
static void w4_pixel(const Args& a, int ox, int oyb, int chan) {
    constexpr int NVP = 1;
    const int W = a.W, H = a.H;
    const u64 size = (u64)H * W * a.YC * 4ull;
    for (int i = 0; i < 4; ++i) {
        unsigned vo[NVP][4];
        for (int hp = 0; hp < NVP; ++hp) vo[hp][i] = @VO@;
        for (int h = 0; h < 2; ++h) {
            const bool keep = ox < W && oyb + i < H;
            const int ch = chan + (EPI == LWG_EPI_SPADE || SM ? 0 : 32 * h);
            const u64 want = (((u64)(oyb + i) * W + ox) * a.YC + ch) * 4ull;
            check(keep, (unsigned)(@ST_OFF@), (unsigned)(@ST_SOFF@), want, size, ox, oyb + i, ch);
            if (EPI != LWG_EPI_SPADE) {
                const int chl = chan + (SM ? 0 : 32 * h);
                const u64 wl = (((u64)(oyb + i) * W + ox) * a.YC + chl) * 4ull;
                check(keep, (unsigned)(@LD_OFF@), (unsigned)(@LD_SOFF@), wl, size, ox, oyb + i, chl);
            }
        }
    }
}

// halo loads: the element (gx, gy, channel quad half) of an input with C channels, the stage's channels c .. c + 7 through the scalar offset
@HALO@

static void run_convt(void (*fn)(const Args&, int, int, int), const char* name, Args a) {
    const int bx = (a.W + 15) / 16, by = (a.H + 15) / 16;
    const u64 rowb = (u64)a.YW * a.YC * 4ull;
    int ycross = (int)(((1ull << 31) + rowb - 1) / rowb / 2 / 16) * 16;            // the block whose rows cross 2^31 bytes
    int ys[4] = {0, (by - 1) * 16, ycross < by * 16 ? ycross : 0, ycross >= 16 && ycross - 16 < by * 16 ? ycross - 16 : 0};
    int xs[3] = {0, (bx - 1) * 16, bx > 2 ? (bx / 2) * 16 : 0};
    int ns[2] = {0, a.N - 32};
    where = name;
    printf("%s\n", name);
    fflush(stdout);
    for (int y : ys) for (int x : xs) for (int n : ns) fn(a, x, y, n);
}

static void run_w4(const Args& a) {
    where = "conv_winograd4 out";
    const int rows[] = {0, 1, 2, 3, a.H - 4, a.H - 3, a.H - 2, a.H - 1, a.H, a.H + 1, a.H + 7, a.H + 15};
    for (int oyb : rows) {
        if (oyb < 0) continue;
        for (int ox : {0, 1, a.W - 2, a.W - 1, a.W, a.W + 1, a.W + 31})
            for (int k = 0; 4 * k + 32 < a.N || k == 0; k += 3) {
                if (ox < 0) continue;
                const int chan = a.ycoff + 4 * k;
                w4_pixel<LWG_EPI_NONE, false>(a, ox, oyb, chan);
                w4_pixel<LWG_EPI_RESIDUAL, false>(a, ox, oyb, chan);
                w4_pixel<LWG_EPI_NONE, true>(a, ox, oyb, chan);
                w4_pixel<LWG_EPI_SPADE, false>(a, ox, oyb, chan);
            }
    }
    // the rows where the image's bytes cross 2^31
    const u64 rowb = (u64)a.W * a.YC * 4ull;
    const int yc = (int)((1ull << 31) / rowb);
    if (yc < a.H)
        for (int oyb = yc - 3; oyb <= yc; ++oyb)
            if (oyb >= 0) for (int ox : {0, a.W - 1, a.W}) w4_pixel<LWG_EPI_RESIDUAL, false>(a, ox, oyb, a.ycoff);
}

int main() {
@MAIN@
    printf("kept %llu dropped %llu bad %llu walked %llu\n", kept, dropped, bad, walked);
    return bad != 0;
}
"""


# block walks: the decoder's three up-sampling layers at 512 x 512 (B, H = W, N) for the benchmark's frame batches on 256 CUs, and ragged launches -
# grids that are no multiple of 8, 1 / 2 / 4 / 8 column blocks, fewer tiles than workgroups per column block, fewer blocks than workgroups
def _walk_cases():
    out = [(B, S, S, N, 256) for S, N in ((64, 256), (128, 128), (256, 64)) for B in (300, 32, 2, 1)]
    out += [(1, 40, 56, 32 * ncb, nwg) for ncb in (1, 2, 4, 8) for nwg in (8, 24, 64, 250, 256, 304)]
    out += [(3, 17, 100, 32 * ncb, nwg) for ncb in (2, 3, 8) for nwg in (16, 40, 63)]
    out += [(1, 16, 16 * 9, 256, 64), (1, 16, 16 * 8, 256, 64), (1, 16, 16 * 7, 256, 64), (5, 1, 1, 64, 8)]       # tiles = 9, 8, 7 against grid / ncb = 8
    return out


def _contract_cases():
    """(entry point, B, H, W, C0, N, YC, ydt) of _limit_cases()'s transposed Winograd shapes, over and under each limit, and of _convt_shapes()."""
    out = []
    for _, fn, over, under in _limit_cases():
        if "transpose4_winograd" in fn:
            out += [(fn, kw["B"], kw["H"], kw["W"], kw["C0"], kw["N"], kw["YC"], kw.get("ydt", 0)) for kw in (over, under)]
    for H, W, Cin, N, YC, _ in _convt_shapes():
        out += [(fn, 1, H, W, Cin, N, YC, 0) for fn in ("lwg_conv_transpose4_winograd_f32", "lwg_conv_transpose4_winograd24_f32")]
    return out


_PANELS = {"lwg_conv_transpose4_winograd_f32": (144, 0xffffffff), "lwg_conv_transpose4_winograd24_f32": (240, 0x7fffffff)}      # bytes per (Cin, N) pair, size limit


def _harness():
    vo, st_off, st_soff, ld_off, ld_soff = _w4_exprs()
    halo, hcalls = [], []
    soffs = _halo_soffsets()
    for j, (name, inp, expr) in enumerate(_halo_exprs()):
        cvar = "a.C" + inp if "a.C" + inp in expr else "Cin"
        so = soffs[name]
        halo.append(textwrap.dedent("""
        static void halo_%d(const Args& a, int gx, int gy) {
            const int W = a.W, H = a.H, Cin = %s;
            const u64 size = (u64)H * W * Cin * 4ull;
            for (int half = 0; half < 2; ++half) {
                const int hq = half;
                const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
                const unsigned v = %s;
                for (int c = 0; c < Cin; c += 8) {
                    const u64 want = in ? (((u64)gy * W + gx) * Cin + 4 * half + c) * 4ull : 0ull;
                    check(in, v, %s, want, size, gx, gy, c + 4 * half);
                }
            }
        }""") % (j, cvar, expr.replace("a.C0", "Cin").replace("a.C1", "Cin"), so))
        hcalls.append((name, j))
    main = []
    who = "%s (%s)" % (CONVT_HEADER, ", ".join(CONVT_KERNELS))
    for sh in _convt_shapes():
        H, W, Cin, N, YC, ycoff = sh
        a = "Args{%d, %d, %d, 0, %d, %d, %d, %d, %d}" % (H, W, Cin, N, 2 * H, 2 * W, YC, ycoff)
        for lay, fn in (("q4", "convt_store<true>"), ("nhwc", "convt_store<false>"), ("halo", "convt_halo")):
            main.append('    run_convt(%s, "%s %s H=%d W=%d YC=%d ycoff=%d", %s);' % (fn, who, lay, H, W, YC, ycoff, a))
    for c in _walk_cases():
        main.append("    convt_walk(%d, %d, %d, %d, %du, true); convt_walk(%d, %d, %d, %d, %du, false);" % (c + c))
    for j, (fn, B, H, W, C0, N, YC, ydt) in enumerate(_contract_cases()):
        main.append('    printf("contract %d %%d\\n", convt_contract(%d, %d, %d, %d, %d, %d, %d, %dull, %dull));' % ((j, B, H, W, C0, N, YC, ydt) + _PANELS[fn]))
    for sh in _w4_shapes():
        H, W, C, N, YC, ycoff = sh
        a = "Args{%d, %d, %d, %d, %d, %d, %d, %d, %d}" % (H, W, C, C, N, H, W, YC, ycoff)
        main.append("    run_w4(%s);" % a)
        for name, j in hcalls:
            main.append('    where = "%s halo H=%d W=%d"; for (int gy : {-1, 0, %d, %d}) for (int gx : {-1, 0, %d, %d}) halo_%d(%s, gx, gy);'
                        % (name, H, W, H - 1, H, W - 1, W, j, a))
    return (_HARNESS.replace("@CONVT@", _CONVT).replace("@VO@", vo).replace("@ST_OFF@", st_off).replace("@ST_SOFF@", st_soff)
            .replace("@LD_OFF@", ld_off).replace("@LD_SOFF@", ld_soff).replace("@HALO@", "\n".join(halo)).replace("@MAIN@", "\n".join(main)))


def _compiler():
    for c in (shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", shutil.which("g++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no host C++ compiler")


def test_buffer_offsets_stay_in_32_bits_at_the_contract_edges():
    """Every buffer access of the fp32 Winograd kernels whose offset can be the out-of-range marker plus an increment, at the corner shapes their host
    contracts accept: the stores of F(4x4, 3x3), convT F(2x2, 2x2) and convT F(2x4, 2x2) (NHWC and channel-quad planes), the residual / SPADE
    epilogue loads of F(4x4, 3x3), the halo loads of all four.  Kept accesses land on their own pixel and channel, dropped ones at or beyond the
    buffer's size modulo 2^32, and no expression that forms an offset overflows its C++ type (signed overflow traps)."""
    src = _harness()
    with tempfile.TemporaryDirectory() as d:
        cpp, exe = os.path.join(d, "audit.cpp"), os.path.join(d, "audit")
        open(cpp, "w").write(src)
        flags = ["-std=c++17", "-O1", "-fsanitize=signed-integer-overflow", "-fsanitize-trap=signed-integer-overflow", "-Wno-unused-variable"]
        r = subprocess.run([_compiler(), *flags, "-I", CSRC, cpp, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    out = "\n".join(ln for ln in r.stdout.splitlines() if not ln.startswith(("conv", "lwg_convt", "contract")))
    assert r.returncode >= 0, "signed overflow in an offset expression (trapped) at: " + r.stdout.strip().splitlines()[-1:].__repr__()
    assert r.returncode == 0, out[-3000:]
    kept, dropped = (int(v) for v in re.search(r"kept (\d+) dropped (\d+)", r.stdout).groups())
    assert kept > 10 ** 6 and dropped > 10 ** 6, r.stdout
    # the block walks ran (every workgroup of every launch of _walk_cases(), XCD order on and off; their findings count as bad above)
    assert int(re.search(r"walked (\d+)", r.stdout).group(1)) > 10 ** 5, r.stdout
    # the entry points' contract (ctw_contract_ok with each kernel's panel) agrees with its restatement on both sides of every size limit
    got = dict((int(i), int(v)) for i, v in re.findall(r"^contract (\d+) (\d)$", r.stdout, re.M))
    cases = _contract_cases()
    assert len(got) == len(cases)
    for j, (fn, B, H, W, C0, N, YC, ydt) in enumerate(cases):
        assert got[j] == int(_convt_ok(H, W, C0, YC)), (fn, B, H, W, C0, N, YC, ydt, got[j])
    assert 0 < sum(got.values()) < len(cases)


# ---- host limits ----

_LIMITS = r"""
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
out = {}
bad = 0xdead0000
def args(B, H, W, C0, N, YH, YW, YC, ycoff=0, ntaps=4, omul=2, xdt=0, ydt=0, C1=0, act=0, stride=1):
    a = _lib.LwgConvArgs()
    a.x0, a.w, a.y, a.bias = bad, bad, bad, bad
    a.x1 = bad if C1 else None
    a.B, a.H, a.W, a.C0, a.C1, a.N = B, H, W, C0, C1, N
    a.OH, a.OW, a.M = H, W, B * H * W
    a.YH, a.YW, a.YC, a.ycoff = YH, YW, YC, ycoff
    a.ntaps, a.stride, a.omul, a.xdt, a.ydt, a.act = ntaps, stride, omul, xdt, ydt, act
    if stride != 1:
        a.OH, a.OW, a.M = YH, YW, B * YH * YW
    if ntaps == 4:
        for t, (dy, dx) in enumerate(((-1, -1), (-1, 0), (0, -1), (0, 0))):
            a.dy[t], a.dx[t] = dy, dx
    else:
        for t in range(9):
            a.dy[t], a.dx[t] = t // 3 - 1, t % 3 - 1
    return a
def call(fn, kw):
    a = ctypes.byref(args(**kw))
    if fn == "lwg_up4_head_compose_bf16":
        return L.lwg_up4_head_compose_bf16(a, bad, None, 0, None, bad, None, None)
    if fn.endswith("_ws"):
        return getattr(L, fn)(a, bad, None)
    return getattr(L, fn)(a, None)
for key, fn, over, under in CASES:
    out[key] = [call(fn, over), call(fn, under)]
out["slice_count"] = [L.lwg_conv_slice_count(ctypes.byref(args(**kw))) for kw in SLICE]
print(json.dumps(out))
"""


def _limit_cases():
    """(key, entry point, args just over ONE size limit, the same args just under it).  Over: 1 (hipErrorInvalidValue) before any launch.  Under: every
    host check passes, so the call gets as far as the launch - which fails with another code where no device is visible: the pair shows that this very
    limit is what refuses the first shape (no other check of the entry point does)."""
    cases = []
    d = dict
    # transposed Winograd kernels: output image + 32 rows of slack < 3 GiB (a 16-channel input: far under its own limit)
    for YC in (32, 64):
        W = _wmax(_convt_ok, 1, 16, YC)
        assert not _convt_ok(1, W + 1, 16, YC) and (W + 1) * 16 * 4 < OOB
        for fn in ("lwg_conv_transpose4_winograd_f32", "lwg_conv_transpose4_winograd24_f32"):
            for ydt in (0, 2):
                kw = lambda w: d(B=1, H=1, W=w, C0=16, N=32, YH=2, YW=2 * w, YC=YC, ydt=ydt)      # noqa: E731
                cases.append(("%s out YC=%d ydt=%d" % (fn, YC, ydt), fn, kw(W + 1), kw(W)))
    # ... input image < 3 GiB: 1024 input channels, a 32-channel output of 0.4 GiB
    H, W = 384, OOB // (384 * 1024 * 4)
    assert H * W * 1024 * 4 == OOB and _convt_ok(H, W - 1, 1024, 32) and (2 * H + 32) * 2 * W * 32 * 4 < OOB
    for fn in ("lwg_conv_transpose4_winograd_f32", "lwg_conv_transpose4_winograd24_f32"):
        kw = lambda w: d(B=1, H=H, W=w, C0=1024, N=32, YH=2 * H, YW=2 * w, YC=32)          # noqa: E731
        cases.append(("%s in" % fn, fn, kw(W), kw(W - 1)))
    # F(4x4, 3x3): output image + 256 bytes < 3 GiB (64 input channels: half the input limit)
    W = _wmax(_w4_ok, 1, 64, 128)
    assert not _w4_ok(1, W + 1, 64, 128) and (W + 1) * 64 * 4 < OOB
    kw = lambda w: d(B=1, H=1, W=w, C0=64, N=64, YH=1, YW=w, YC=128, ntaps=9, omul=1)              # noqa: E731
    cases.append(("lwg_conv2d_winograd4_f32 out", "lwg_conv2d_winograd4_f32", kw(W + 1), kw(W)))
    # F(4x4, 3x3) and F(2x2, 3x3) (plain and workspace form): each input image < 3 GiB - 512 channels in, a 64-channel output of 0.4 GiB
    W = OOB // (512 * 4)
    assert W * 512 * 4 == OOB and W * 64 * 4 + 256 < OOB
    for fn in ("lwg_conv2d_winograd4_f32", "lwg_conv2d_winograd_f32", "lwg_conv2d_winograd_f32_ws"):
        kw = lambda w: d(B=1, H=1, W=w, C0=512, N=64, YH=1, YW=w, YC=64, ntaps=9, omul=1)          # noqa: E731
        cases.append(("%s in" % fn, fn, kw(W), kw(W - 1)))
        kw = lambda w: d(B=1, H=1, W=w, C0=16, C1=512, N=64, YH=1, YW=w, YC=64, ntaps=9, omul=1)   # noqa: E731
        cases.append(("%s in x1" % fn, fn, kw(W), kw(W - 1)))
    # the sliced entry points: ONE frame over the 32-bit input range (under it, two frames run as two one-frame slices)
    for fn, xdt, C0 in (("lwg_conv2d_nhwc_f32", 0, 64), ("lwg_conv2d_nhwc_f32_split", 0, 64), ("lwg_conv2d_nhwc_bf16", 1, 64),
                        ("lwg_conv2d_nhwc_bf16_hr", 1, 64)):
        W = OOB // (C0 * (2 if xdt else 4))
        kw = lambda w: d(B=2, H=1, W=w, C0=C0, N=64, YH=1, YW=w, YC=64, ntaps=9, omul=1, xdt=xdt, ydt=xdt)      # noqa: E731
        cases.append(("%s one frame" % fn, fn, kw(W), kw(W - 1)))
    W = OOB // (2 * 8 * 4)                                                  # fp32 8-channel input of the bf16 first layer, two rows; stride 2
    kw = lambda w: d(B=2, H=2, W=w, C0=8, N=64, YH=1, YW=(w + 1) // 2, YC=64, ntaps=9, omul=1, xdt=0, ydt=1, stride=2)      # noqa: E731
    cases.append(("lwg_conv2d_nhwc_c8_bf16 one frame", "lwg_conv2d_nhwc_c8_bf16", kw(W), kw(W - 1)))
    W = OOB // (128 * 2)
    kw = lambda w: d(B=2, H=1, W=w, C0=128, N=64, YH=2, YW=2 * w, YC=64, xdt=1, ydt=1)          # noqa: E731
    cases.append(("lwg_conv_transpose4_nhwc_bf16 one frame", "lwg_conv_transpose4_nhwc_bf16", kw(W), kw(W - 1)))
    kw = lambda w: d(B=2, H=1, W=w, C0=128, N=64, YH=2, YW=2 * w, YC=64, xdt=1, ydt=1, act=1)   # noqa: E731
    cases.append(("lwg_up4_head_compose_bf16 one frame", "lwg_up4_head_compose_bf16", kw(W), kw(W - 1)))
    W = OOB // (64 * 4)
    kw = lambda w: d(B=2, H=1, W=w, C0=64, N=64, YH=2, YW=2 * w, YC=64)                          # noqa: E731
    cases.append(("lwg_conv_transpose4_nhwc_f32 one frame", "lwg_conv_transpose4_nhwc_f32", kw(W), kw(W - 1)))
    return cases


def test_host_limits_at_the_boundary():
    """The smallest shape over each size limit of a conv entry point returns 1 before any launch, and the shape just under that limit (the same in
    every other respect) passes the host checks; for the batch-slicing entry points a single frame that cannot fit is refused, and lwg_conv_slice_count
    reports 0 for it, 1 for a batch just under the range and 2 for one just over.  Runs in a child process that sees no GPU (checked), so that the
    calls that pass the host checks - and a missing check - can never launch a kernel on the test's fake pointers."""
    import json
    cases = _limit_cases()
    per = 1 * 1024 * 64 * 4
    n = OOB // per
    slice_shapes = [dict(B=1, H=1, W=OOB // 256, C0=64, N=64, YH=1, YW=OOB // 256, YC=64, ntaps=9, omul=1),        # one frame of exactly 3 GiB
                    dict(B=n - 1, H=1, W=1024, C0=64, N=64, YH=1, YW=1024, YC=64, ntaps=9, omul=1),            # B per < 0xC0000000: one launch
                    dict(B=n, H=1, W=1024, C0=64, N=64, YH=1, YW=1024, YC=64, ntaps=9, omul=1)]           # B per == 0xC0000000: two slices
    code = "ROOT = %r\nCASES = %r\nSLICE = %r\n" % (ROOT, cases, slice_shapes) + _LIMITS
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert "error" not in got, got
    assert got.pop("slice_count") == [0, 1, 2]
    assert set(got) == {k for k, _, _, _ in cases}
    wrong = {k: v for k, v in got.items() if v[0] != 1}
    assert not wrong, ("not refused", wrong)
    wrong = {k: v for k, v in got.items() if v[1] in (0, 1)}
    assert not wrong, ("refused (or launched) just under the limit", wrong)
