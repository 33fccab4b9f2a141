"""CPU checks of the 32-bit buffer offsets of the fp32 Winograd convolutions at the edges of their host contracts.

The kernels address an image as ONE raw buffer: a byte offset is 32 bits, and an access that must not happen (a padding tap, a pixel right of or below
the image) gets the marker 0xC0000000 - at or beyond any image's size, so the hardware drops the store / returns zeros for the load.  That holds only
while every offset the kernel forms - the marker plus a per-pass or per-stage increment included - stays within 32 bits, and while the C++
expressions that form the offsets do not overflow their own types.

The audit below compiles the kernels' own offset arithmetic into a host program with signed-overflow traps by INCLUDING csrc/lwg_convt_wino.h (the
two transposed kernels) and csrc/lwg_conv_wino.h (the three 3 x 3 kernels), whose integer functions are what the kernels compile, and evaluates
it - offsets, block walks, host contracts - for the corner shapes the host contracts accept: the widest output rows at the
fewest rows, the tallest images at one or two pixels of width, images just under the size limits, widths and heights that are not multiples of the
tile.  Every kept access must land at its own pixel and channel; every dropped one at or beyond the buffer's size modulo 2^32.

The host-limit test checks, per entry point, that the smallest shape over each size limit returns 1 before any launch."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ipercore_amd", "csrc")
OOB = 0xC0000000


def _code(name):
    """csrc/<name> without its comments."""
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


CONVT_KERNELS = ("convt_winograd.hip", "convt_winograd24.hip")
CONVT_HEADER = "lwg_convt_wino.h"


CONV3_KERNELS = ("conv_winograd.hip", "conv_winograd4.hip", "conv_winograd_bf16.hip")
CONV3_HEADER = "lwg_conv_wino.h"


def test_offset_expressions_are_found():
    """The kernels are audited through the shared headers, so the converse is checked here: no kernel forms a store or halo offset, an input
    descriptor, a marker or a contract of its own, and each runs the header's block walk, halo offsets and (transposed kernels) store phase."""
    h = _code(CONVT_HEADER)
    assert "(v, ry, (int)ctw_store_voff(q4, s, pass, ey0, a.YH), 0, NT)" in h      # pass offsets in the VECTOR offset (test_no_wide_buffer_store_with_register_soffset)
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
    assert "CTW_FN unsigned ctw_halo_soff(int st) { return (unsigned)(st * KS) * 4u; }" in h
    # the 3 x 3 kernels: csrc/lwg_conv_wino.h
    h = _code(CONV3_HEADER)
    for call in ("voff0[k] = cw_halo_voff(tid + nth * k, hw, nel, 1, x0, y0, a.H, a.W, a.C0, 4)", "voff1[k] = cw_halo_voff(tid + nth * k, hw, nel, 1, x0, y0, a.H, a.W, a.C1, 4)",
                 "cw_buf_load<POLICY>(rx0, voff0[k], cw_stage_soff(c, a.C0, false, 4))", "cw_buf_load<POLICY>(r, v, cw_stage_soff(c, a.C0, true, 4))",
                 "const bool second = cw_stage_second(c, a.C0, true)", "rx0 = cw_image_rsrc(a.x0, b, a.H, a.W, a.C0, 4u)", "rx1 = cw_image_rsrc(a.x1, b, a.H, a.W, a.C1, 4u)"):
        assert call in h, call
    calls = {
        "conv_winograd.hip": ("cw_grid(a.B, H, W, N, 2 * TPB, 2 * TPB, NBV)", "cw_order(CW_COLMAJOR, gridDim.x, blockIdx.x, N / NBV, g)", "CwBlock<2, TWO> bk", "cw_block(o, id, cb, t)",
                              "bk.locate(a, g, t, 2 * TPB, 2 * TPB, cw_n0(cb, NBV))", "bk.halo(a, tid, WG_THREADS, HALO, PLANE * 2)", "bk.rld1(a, (st + sbeg) * KS, q)",
                              "cw_rst1(raw0 + ", "cw_has_block(o, nblk)", "cw_contract_ok(a, 64ull, CW_NO_OUT_BUFFER)", "cw_launch<", "cw_panel_args_ok(",
                              "#define TPB 8", "#define HALO 18", "#define KS 8"),
        "conv_winograd4.hip": ("cw_grid(a.B, H, W, N, 4 * W4_PBX, 4 * W4_PBY, NBV)", "cw_order(cw4_order_kind(LWG_W4_XCD, LWG_W4_CHUNK, SM, gridDim.x, N / NBV, Cin, N, g.tiles, g.total), gridDim.x, blockIdx.x, N / NBV, g)",
                               "CwBlock<NQ, TWO> bk", "cw_block(o, id, cb, t)", "bk.locate(a, g, t, 4 * W4_PBX, 4 * W4_PBY, SMS ? cw4_n0_spade_small(cb) : cw_n0(cb, NBV))",
                               "bk.halo(a, tids, NTH, W4_HW, W4_NEL)", "bk.template rld1<W4_NT_LD>(a, c, k)", "const int c = st * W4_KS;", "cw_rst1(raw0 + ", "cw_has_block(o, nblk)",
                               "vo[hp][i] = cw4_out_voff(ox, oyb + i, H, W, a.YC, chan)",
                               "re, (int)cw4_out_group(vo[NVP == 2 ? h : 0][i], h, !SM), 0, W4_NT_RES)",                       # (scalar offsets: the constant 0)
                               "ry, (int)cw4_out_group(vo[NVP == 2 ? h : 0][i], h, EPI != LWG_EPI_SPADE && !SM), 0, W4_NT_ST)",
                               "cw_contract_ok(*pa, 144ull, 256ll)", "cw_launch<", "cw_panel_args_ok(", "#define W4_PBX 8", "#define W4_PBY 4", "#define W4_HW 34", "#define W4_HH 18",
                               "#define W4_NEL (W4_HW * W4_HH * 2)", "#define W4_NQ 3", "NQ = SM ? 5 : W4_NQ", "NTH = SM ? 256 : W4_THREADS", "#define W4_KS 8"),
        "conv_winograd_bf16.hip": ("cw_grid(a.B, H, W, N, 16, 16, 64)", "cw_image(g, t)", "cw_corner(g, t - b * g.bx * g.by, 16, 16, x0, y0)", "cw_n0(cb, 64)",
                                   "cw_image_rsrc(a.x0, b, H, W, a.C0, 2u)", "cw_image_rsrc(a.x1, b, H, W, a.C1, 2u)",
                                   "hlin[q] = cw_halo_pixel(tid + WB_THREADS * q, WB_HALO, 4 * WB_HALO_PIX, 2, x0, y0, H, W)",
                                   "cw_halo_pixel_voff(hlin[q], tid + WB_THREADS * q, 2, use1 ? a.C1 : a.C0, 2)", "use1 = cw_stage_second(cc, a.C0, TWO)",
                                   "soff = cw_stage_soff(cc, a.C0, TWO, 2)", "cwb_contract_ok(*pa)", "cw_launch<", "#define WB_HALO 18", "#define WB_HALO_LOADS 3", "#define WB_KS 32"),
    }
    for name in CONV3_KERNELS:
        k = _code(name)
        assert '#include "%s"' % CONV3_HEADER in k, name
        for word in ("0xC0000000", "_OOB", "gy * W + gx", "a.M !=", "a.ntaps !=", "a.stride !=", "hipLaunchKernelGGL((lwg_conv", "lwg_allow_dynamic_lds", "done["):
            assert word not in k, (name, word)
        assert not re.search(r"make_buffer_rsrc\([^;]*a\.x[01]", k), name
        for call in calls[name]:
            assert call in k, (name, call)


# ---- host contracts (restated from the entry points; test_host_limits_at_the_boundary checks them against the library) ----

def _convt_ok(H, W, C0, YC):
    return H * W * C0 * 4 < OOB and (2 * H) * (2 * W) * YC * 4 + 32 * (2 * W) * YC * 4 < OOB


def _w4_ok(H, W, C, YC):
    return H * W * C * 4 < OOB and H * W * YC * 4 + 256 < OOB


def _w2_ok(H, W, C):
    return H * W * C * 4 < OOB


def _wb_ok(H, W, C):
    return H * W * C * 2 < OOB


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


def _wb_shapes():
    """(H, W, C) of the bf16 F(2x2, 3x3) kernel's contract, at its corners: the widest rows at the fewest rows, the tallest images at the fewest columns."""
    out = [(H, _wmax(_wb_ok, H, 64), 64) for H in (1, 2, 3)] + [(_hmax(_wb_ok, W, 64), W, 64) for W in (1, 2, 3)]
    out += [(H, W - (W - 1) % 16, C) for H, W, C in out[:3]] + [(1201, _wmax(_wb_ok, 1201, 64), 64)]
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

# the 3 x 3 kernels through csrc/lwg_conv_wino.h: F(4x4)'s output pixels, every kernel's halo by element index (every thread x every piece x every
# stage of both inputs), the block walks of the fp32 kernels in every order, the three host contracts
_CONV3 = r"""
#include "lwg_conv_wino.h"
// the F(4x4, 3x3) kernel's output pixels (stores; residual / SPADE epilogue loads): one pixel (ox, oyb + i), channel group chan (+ 32 h)
template <int EPI, bool SM>
static void w4_pixel(const Args& a, int ox, int oyb, int chan) {
    const int W = a.W, H = a.H;
    const u64 size = (u64)H * W * a.YC * 4ull;
    for (int i = 0; i < 4; ++i) {
        const unsigned vo = cw4_out_voff(ox, oyb + i, H, W, a.YC, chan);
        for (int h = 0; h < 2; ++h) {
            const bool keep = ox < W && oyb + i < H;
            const int ch = chan + (EPI == LWG_EPI_SPADE || SM ? 0 : 32 * h);
            const u64 want = (((u64)(oyb + i) * W + ox) * a.YC + ch) * 4ull;
            check(keep, cw4_out_group(vo, h, EPI != LWG_EPI_SPADE && !SM), 0u, want, size, ox, oyb + i, ch);      // (scalar offsets: the constant 0 of the kernel)
            if (EPI != LWG_EPI_SPADE) {
                const int chl = chan + (SM ? 0 : 32 * h);
                const u64 wl = (((u64)(oyb + i) * W + ox) * a.YC + chl) * 4ull;
                check(keep, cw4_out_group(vo, h, !SM), 0u, wl, size, ox, oyb + i, chl);
            }
        }
    }
}

// a kernel's halo staging: nth threads x nq elements of a hw x hh halo in 2^lgp 16-byte pieces per pixel, stages of ks channels of ebytes bytes
struct HaloForm { const char* name; int nth, nq, hw, hh, lgp, ebytes, ks, ex, ey; };
static const HaloForm F22 = {"conv_winograd", 512, 2, 18, 18, 1, 4, 8, 16, 16}, F44 = {"conv_winograd4", 512, 3, 34, 18, 1, 4, 8, 32, 16},
                      F44S = {"conv_winograd4 4-wave", 256, 5, 34, 18, 1, 4, 8, 32, 16}, FB16 = {"conv_winograd_bf16", 512, 3, 18, 18, 2, 2, 32, 16, 16};

static void conv_halo(const HaloForm& f, const Args& a, int x0, int y0) {
    const int nel = (f.hw * f.hh) << f.lgp, per = 16 / f.ebytes;
    for (int inp = 0; inp < 2; ++inp) {
        const int C = inp ? a.C1 : a.C0, cbeg = inp ? a.C0 : 0;
        const u64 size = (u64)a.H * a.W * C * f.ebytes;
        for (int i = 0; i < f.nth * f.nq; ++i) {
            const unsigned v = cw_halo_voff(i, f.hw, nel, f.lgp, x0, y0, a.H, a.W, C, f.ebytes);
            const int lin = cw_halo_pixel(i, f.hw, nel, f.lgp, x0, y0, a.H, a.W);
            const int pix = i >> f.lgp, piece = i & ((1 << f.lgp) - 1), gy = y0 - 1 + pix / f.hw, gx = x0 - 1 + pix % f.hw;
            const bool in = i < nel && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            if (v != cw_halo_pixel_voff(lin, i, f.lgp, C, f.ebytes) || (lin >= 0) != in || (in && (u64)lin != (u64)gy * a.W + gx))
                if (bad++ < 8) printf("BAD %s element %d at (%d, %d): pixel %d, offset %u\n", where, i, x0, y0, lin, v);
            for (int c = cbeg; c < cbeg + C; c += f.ks) {                         // the stages of this input (channels in concatenated order)
                const u64 want = in ? (((u64)gy * a.W + gx) * C + per * piece + (c - cbeg)) * f.ebytes : 0ull;
                check(in, v, cw_stage_soff(c, a.C0, true, f.ebytes), want, size, gx, gy, c - cbeg + per * piece);
                if (cw_stage_second(c, a.C0, true) != (inp == 1) || cw_stage_second(c, a.C0, false) ||
                    (!inp && cw_stage_soff(c, a.C0, false, f.ebytes) != cw_stage_soff(c, a.C0, true, f.ebytes)))       // (the one-input form: the same offset)
                    if (bad++ < 8) printf("BAD %s stage at channel %d: input / one-input offset\n", where, c);
            }
        }
    }
}

// ... at the block corners first, last and middle in x and y, and at the block where an input's bytes cross 2^31
static void run_halo(const HaloForm& f, const Args& a) {
    static char name[160];
    snprintf(name, sizeof name, "%s halo H=%d W=%d C=%d+%d", f.name, a.H, a.W, a.C0, a.C1);
    where = name;
    const int bx = (a.W + f.ex - 1) / f.ex, by = (a.H + f.ey - 1) / f.ey;
    for (int y : {0, (by - 1) * f.ey, (by / 2) * f.ey}) for (int x : {0, (bx - 1) * f.ex, (bx / 2) * f.ex}) conv_halo(f, a, x, y);
    const u64 p = (1ull << 31) / ((u64)(a.C0 > a.C1 ? a.C0 : a.C1) * f.ebytes);                 // the first pixel beyond 2^31 bytes
    if (p / a.W < (u64)a.H) conv_halo(f, a, (int)(p % a.W) / f.ex * f.ex, (int)(p / a.W) / f.ey * f.ey);
}

// every workgroup's walk over a launch of nwg workgroups: each (column block, tile) exactly once, inside the grid, no block behind the last one; the
// order is the one the restated rule expects; spade: the 4-wave SPADE form's column map - the columns n0 .. + 15 and n0 + 32 .. + 47 of all
// blocks tile N once (per tile)
static void conv_walk(bool f4, int B, int H, int W, int N, int Cin, int nbv, unsigned nwg, int xcd_sw, int chunk_sw, int want_kind, bool spade) {
    const int ex = f4 ? 32 : 16, ey = 16, ncb = N / nbv;
    const CwGrid g = cw_grid(B, H, W, N, ex, ey, nbv);
    if ((long long)nwg > cw_total_blocks(B, H, W, N, ex, ey, nbv)) nwg = (unsigned)g.total;          // (the launch: min(blocks, CUs) workgroups)
    const int kind = f4 ? cw4_order_kind(xcd_sw, chunk_sw, nbv == 32, nwg, ncb, Cin, N, g.tiles, g.total) : CW_COLMAJOR;
    u64 fails = kind != want_kind;
    std::vector<int> seen((size_t)g.total, 0), cols((size_t)N, 0);
    for (unsigned wg = 0; wg < nwg; ++wg) {
        const CwOrder o = cw_order(kind, nwg, wg, ncb, g);
        int id = (int)wg;
        do {                                                                           // (the first block is taken unconditionally, as the kernels do)
            int cb, t, x0 = -1, y0 = -1;
            cw_block(o, id, cb, t);
            const int b = t >= 0 && t < g.tiles ? cw_image(g, t) : -1, n0 = spade ? cw4_n0_spade_small(cb) : cw_n0(cb, nbv);
            if (b >= 0) cw_corner(g, t - b * g.bx * g.by, ex, ey, x0, y0);
            if (cb < 0 || cb >= ncb || b < 0 || b >= B || x0 < 0 || x0 >= W || y0 < 0 || y0 >= H || x0 % ex || y0 % ey || n0 < 0 || n0 + (spade ? 48 : nbv) > N) ++fails;
            else {
                ++seen[(size_t)cb * g.tiles + t];
                if (t == 0) for (int k = 0; k < (spade ? 16 : nbv); ++k) { ++cols[n0 + k]; if (spade) ++cols[n0 + 32 + k]; }
            }
            ++walked;
            id += (int)nwg;
        } while (cw_has_block(o, id));
        for (int k = 1; k < 4; ++k) if (cw_has_block(o, id + k * (int)nwg)) ++fails;
    }
    for (int v : seen) if (v != 1) ++fails;
    for (int v : cols) if (v != 1) ++fails;
    if (fails) { bad += fails; printf("BAD walk f4=%d B=%d H=%d W=%d N=%d Cin=%d nbv=%d nwg=%u xcd=%d chunk=%d kind=%d (want %d): %llu\n", (int)f4, B, H, W, N, Cin, nbv, nwg, xcd_sw, chunk_sw, kind, want_kind, fails); }
}

// which: 0 lwg_conv2d_winograd_f32 (_ws), 1 lwg_conv2d_winograd4_f32, 2 lwg_conv2d_winograd_bf16
static int conv_contract(int which, int B, int H, int W, int C0, int C1, int N, int YC, int ycoff, int epi, int act, int M) {
    static float dummy;
    LwgConvArgs a = {};
    a.x0 = a.w = a.bias = a.res = a.xn = a.mean = a.rstd = &dummy; a.y = &dummy;
    if (C1) a.x1 = &dummy;
    a.B = B; a.H = a.OH = a.YH = H; a.W = a.OW = a.YW = W; a.C0 = C0; a.C1 = C1; a.N = N; a.M = M;
    a.YC = YC; a.ycoff = ycoff; a.ntaps = 9; a.stride = 1; a.omul = 1; a.epi = epi; a.act = act; a.xdt = a.ydt = which == 2 ? LWG_DT_BF16 : LWG_DT_F32;
    for (int t = 0; t < 9; ++t) { a.dy[t] = t / 3 - 1; a.dx[t] = t % 3 - 1; }
    return (int)(which == 2 ? cwb_contract_ok(a) : cw_contract_ok(a, which ? 144ull : 64ull, which ? 256ll : CW_NO_OUT_BUFFER));
}
"""

_HARNESS = r"""
#include <cstdio>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
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

@CONV3@

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


# the generator's 3 x 3 layer shapes at 512 x 512 (H = W, Cin, N): residual blocks and SPADE gamma | beta pairs at 128^2, the decoder's (skip) convolutions
_GEN512 = ((128, 256, 256), (128, 256, 512), (256, 128, 128), (256, 256, 128), (256, 128, 256), (512, 64, 64), (512, 128, 64))


def _w4_kind(nwg, ncb, Cin, N, tiles, sm, xcd_sw, chunk_sw):
    """The F(4x4, 3x3) kernel's block order, restated: 2 XCD-aware, 1 chunked, 0 column-block-major."""
    nwg = min(nwg, tiles * ncb)
    if xcd_sw and not sm and nwg % 8 == 0 and (ncb in (4, 8) or (ncb == 2 and (Cin >= 192 or xcd_sw == 2))) and nwg < tiles * ncb and tiles >= nwg // ncb:
        return 2
    return 1 if chunk_sw == 2 or (chunk_sw == 1 and 144 * Cin * N <= 5 << 20) else 0


def _walk3_cases():
    """(f4, B, H, W, N, Cin, nbv, nwg, xcd switch, chunk switch, order expected, SPADE column map) for conv_walk: the generator's layers at the benchmark's
    frame batches on 256 workgroups and ragged launches (_walk_cases()' style; N = 128 with Cin on both sides of 192 and of the 5 MiB panel rule), F(2x2)
    at 64 and 32 channels per block, F(4x4) in its 8-wave and 4-wave forms under the product's switches and with each order forced."""
    shapes = [(B, S, S, N, Cin, 256) for S, Cin, N in _GEN512 for B in (300, 32, 2, 1)]
    shapes += [(1, 40, 56, 64 * ncb, 64, nwg) for ncb in (1, 2, 4, 8) for nwg in (8, 24, 64, 250, 256, 304)]
    shapes += [(3, 17, 100, 64 * ncb, 256, nwg) for ncb in (2, 3, 8) for nwg in (16, 40, 63)]
    shapes += [(1, 16, 32 * t, 512, 64, 64) for t in (9, 8, 7)] + [(5, 1, 1, 128, 64, 8)]          # tiles = 9, 8, 7 against grid / ncb = 8
    shapes += [(B, 100, 130, 128, Cin, nwg) for Cin in (128, 176, 192, 208, 272, 288) for B, nwg in ((9, 256), (9, 250), (1, 16))]
    out = []
    for B, H, W, N, Cin, nwg in shapes:
        for nbv in (64, 32):
            out.append((0, B, H, W, N, Cin, nbv, nwg, 0, 0, 0, 0))
            tiles = B * ((H + 15) // 16) * ((W + 31) // 32)
            for xs, cs in ((1, 1), (2, 1), (0, 2), (0, 0)):
                out.append((1, B, H, W, N, Cin, nbv, nwg, xs, cs, _w4_kind(nwg, N // nbv, Cin, N, tiles, nbv == 32, xs, cs), 0))
            out.append((1, B, H, W, N, Cin, 32, nwg, 1, 1, _w4_kind(nwg, N // 32, Cin, N, tiles, True, 1, 1), 1))
    assert {c[10] for c in out if c[0] and c[6] == 64 and (c[8], c[9]) == (1, 1)} == {0, 1, 2}       # the product's rule picks each order somewhere
    return out


def _fp32_ok(pair, slack, B, H, W, C0, C1, N, YC, ycoff, epi, act, M):
    """cw_contract_ok restated for the fields the cases vary (pair: panel bytes per (Cin, N); slack: None = the output is no buffer)."""
    if M <= 0 or C0 <= 0 or C0 % 8 or C1 < 0 or C1 % 8 or (C0 + C1) % 16 or N <= 0 or N % 64 or M != B * H * W or ycoff < 0 or ycoff % 4 or YC % 4:
        return False
    if (act == 5 and epi != 1) or (epi == 2 and (YC * 2 != N or ycoff)) or (epi != 2 and (ycoff + N > YC or epi not in (0, 1))):
        return False
    return _w2_ok(H, W, max(C0, C1)) and pair * (C0 + C1) * N < 0xffffffff and (slack is None or H * W * YC * 4 + slack < OOB)


def _bf16_ok(B, H, W, C0, C1, N, YC, ycoff, epi, act, M):
    """cwb_contract_ok restated for the same fields."""
    if min(B, H, W, C0, N) <= 0 or C1 < 0 or M != B * H * W or N % 64 or (C0 + C1) % 64 or YC % 8 or ycoff % 8 or ycoff < 0 or (C1 and C0 % 64):
        return False
    if act not in (0, 1, 2, 3) or not _wb_ok(H, W, max(C0, C1)) or 32 * (C0 + C1) * N >= OOB or B * ((H + 15) // 16) * ((W + 15) // 16) * (N // 64) >= 0x7fffffff:
        return False
    return (YC * 2 == N and ycoff == 0) if epi == 2 else (ycoff + N <= YC and epi in (0, 1))


def _contract3_cases():
    """(B, H, W, C0, C1, N, YC, ycoff, epi, act, M) for the three 3 x 3 entry points' predicates: _limit_cases()'s shapes over and under each limit,
    the corner shapes of the audit, and one case on either side of every other size term.  M is what a caller computes in an int."""
    rows = []
    for _, fn, over, under in _limit_cases():
        if fn in ("lwg_conv2d_winograd4_f32", "lwg_conv2d_winograd_f32", "lwg_conv2d_winograd_f32_ws"):
            rows += [(kw["B"], kw["H"], kw["W"], kw["C0"], kw.get("C1", 0), kw["N"], kw["YC"], 0, 0, 0) for kw in (over, under)]
    rows += [(1, H, W, C, C, N, YC, ycoff, 0, 0) for H, W, C, N, YC, ycoff in _w4_shapes()]
    rows += [(1, H, W + d, C, C, 64, 64, 0, 0, 0) for H, W, C in _wb_shapes()[:6] for d in (0, 1)]                   # bf16: the input image on either side of 3 GiB
    rows += [(1, 8, 8, 4096, 0, N, N, 0, 0, 0) for N in (7232, 7296, 16320, 16384, 24512, 24576)]                 # the panel limits: 144, 64 and 32 bytes per pair
    rows += [((1 << 27) - d, 1, 1, 64, 0, 1024, 1024, 0, 0, 0) for d in (0, 1)]                                     # bf16: 2^31 blocks | 16 fewer
    rows += [(65537, 1, 65536, 64, 0, 64, 64, 0, 0, 0)]                                                             # B H W = 2^32 + 65536: an int M wraps to 65536
    rows += [(2, 20, 24, 64, 64, 128, 64, 0, 2, 1), (2, 20, 24, 64, 64, 128, 128, 0, 2, 1), (2, 20, 24, 64, 0, 64, 128, 64, 1, 5),
             (2, 20, 24, 64, 0, 64, 128, 64, 0, 5), (2, 20, 24, 64, 0, 64, 128, 68, 1, 2), (2, 20, 24, 72, 56, 64, 68, 4, 0, 3), (2, 20, 24, 64, 0, 64, 64, 0, 3, 0)]
    wrap = lambda m: (m + (1 << 31)) % (1 << 32) - (1 << 31)      # noqa: E731
    return [r + (wrap(r[0] * r[1] * r[2]),) for r in rows]


def _harness():
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
        main.append("    run_w4(%s); run_halo(F22, %s); run_halo(F44, %s); run_halo(F44S, %s);" % (a, a, a, a))
    for H, W, C in _wb_shapes():
        main.append("    run_halo(FB16, Args{%d, %d, %d, %d, 64, %d, %d, 64, 0});" % (H, W, C, C, H, W))
    for c in _walk3_cases():
        main.append("    conv_walk(%d, %d, %d, %d, %d, %d, %d, %du, %d, %d, %d, %d);" % c)
    for j, c in enumerate(_contract3_cases()):
        main.append('    printf("contract3 %d %%d%%d%%d\\n", %s);' % (j, ", ".join("conv_contract(%d, %s)" % (w, ", ".join(str(v) for v in c)) for w in (0, 1, 2))))
    return _HARNESS.replace("@CONVT@", _CONVT).replace("@CONV3@", _CONV3).replace("@MAIN@", "\n".join(main))


def _compiler():
    for c in (shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", shutil.which("g++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no host C++ compiler")


def test_buffer_offsets_stay_in_32_bits_at_the_contract_edges():
    """Every buffer access of the Winograd kernels whose offset can be the out-of-range marker plus an increment, at the corner shapes their host
    contracts accept: the stores of F(4x4, 3x3), convT F(2x2, 2x2) and convT F(2x4, 2x2) (NHWC and channel-quad planes), the residual / SPADE
    epilogue loads of F(4x4, 3x3), the halo loads of all five (the bf16 F(2x2, 3x3) kernel's included) by element index.  Kept accesses land on
    their own pixel and channel, dropped ones at or beyond the buffer's size modulo 2^32, and no expression that forms an offset overflows its C++
    type (signed overflow traps).  The block walks visit every block once in the order the restated rules expect, and the host contracts agree
    with their restatements on both sides of every size limit."""
    src = _harness()
    with tempfile.TemporaryDirectory() as d:
        cpp, exe = os.path.join(d, "audit.cpp"), os.path.join(d, "audit")
        open(cpp, "w").write(src)
        flags = ["-std=c++17", "-O1", "-fsanitize=signed-integer-overflow", "-fsanitize-trap=signed-integer-overflow", "-Wno-unused-variable"]
        r = subprocess.run([_compiler(), *flags, "-I", CSRC, cpp, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    out = "\n".join(ln for ln in r.stdout.splitlines() if not ln.startswith(("lwg_convt", "contract")))
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
    # ... and the 3 x 3 entry points' (cw_contract_ok with each fp32 kernel's panel and output slack, cwb_contract_ok)
    got = dict((int(i), v) for i, v in re.findall(r"^contract3 (\d+) (\d\d\d)$", r.stdout, re.M))
    cases = _contract3_cases()
    assert len(got) == len(cases)
    for j, c in enumerate(cases):
        want = "%d%d%d" % (_fp32_ok(64, None, *c), _fp32_ok(144, 256, *c), _bf16_ok(*c))
        assert got[j] == want, (c, got[j], want)
    for w in range(3):
        assert 0 < sum(int(v[w]) for v in got.values()) < len(cases)


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
