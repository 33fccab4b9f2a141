"""CPU checks of the list-driven form of the bf16 row-renaming convolution kernel (lwg_conv2d_nhwc_bf16_hr_list; csrc/lwg_bf16_hr_list.h; DESIGN.md
3.12f) - the id arithmetic the kernel compiles, built into a stand-alone host program with signed-overflow traps as tests/test_spade_skip_fine_cpu.py does.

  * the walk: on ragged images (40 x 72, 40 x 48, 8 x 16) with heavy counts 0, 1, all and mixed and 1, 2 and 4 column tiles every in-image (sub-tile,
    column tile) is visited exactly once, heavy ones by heavy entries and before every light one in dispatch order; workgroups beyond the counts exit,
    counts that the memory could not hold by rights (negative, larger than the grid) never reach a list slot past the launch's entries;
  * the light lanes' offsets: over the workgroups of a launch the fp32 accumulator frame's floats (pixel, column) and the bf16 frame's channels are
    each touched exactly once, inside the frame on ragged edges, in 16-byte pieces;
  * the window reach: a numpy model of "3 x 3 direct convolution, ReLU, 3 x 3 convolution" on integer-valued background / foreground frames shows
    that d = (1, 2) is sufficient - every light sub-tile equals the calibration frame's - and that (0, 1) is not."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ipercore_amd", "csrc")

_SRC = r"""
#include <cstdio>
#include <vector>
#include <set>
#include "lwg_bf16_hr_list.h"
typedef unsigned long long u64;
static u64 bad = 0, walked = 0, exited = 0, elems = 0;
#define FAIL(...) do { if (bad++ < 12) { printf("BAD " __VA_ARGS__); printf("\n"); } } while (0)

// the in-image sub-tile ids of a launch in ascending order (the classifier's numbering: 4 * block + 2 * sub-tile row + sub-tile column)
static std::vector<int> in_image(int B, int H, int W) {
    const CwGrid g = cw_grid(B, H, W, CW_NB, 32, 16, CW_NB);
    std::vector<int> ids;
    for (int u = 0; u < g.tiles * Cw4F::NS; ++u) {
        int b, x0, y0;
        Cw4F::corner(g, u, b, x0, y0);
        if (Cw4F::in_image(x0, y0, H, W)) ids.push_back(u);
    }
    return ids;
}

// heavy_mode: 0 none, 1 one (the middle id), 2 all, 3 every third + the last; c0 / c1: what the kernel finds in counts[] (-1: the true counts)
static void walk_case(int B, int H, int W, int tiles_n, int heavy_mode, int c0, int c1) {
    const std::vector<int> ids = in_image(B, H, W);
    const int total = (int)ids.size();
    if (total != Cw4F::in_image_total(B, H, W)) FAIL("total %d != %d", total, Cw4F::in_image_total(B, H, W));
    std::vector<int> heavy, light;
    for (int k = 0; k < total; ++k) {
        const bool h = heavy_mode == 2 || (heavy_mode == 1 && k == total / 2) || (heavy_mode == 3 && (k % 3 == 0 || k == total - 1));
        (h ? heavy : light).push_back(ids[k]);
    }
    const bool honest = c0 < 0;
    if (honest) c0 = (int)heavy.size(), c1 = (int)light.size();
    const long long grid = hrl_grid(B, H, W, tiles_n);
    if (grid != (long long)total * tiles_n) FAIL("grid");
    const int tx = (W + 15) / 16, ty = (H + 7) / 8;
    std::vector<int> seen((size_t)B * ty * tx * tiles_n, 0);
    int last_heavy = -1, first_light = (int)grid;
    for (int lid = 0; lid < (int)grid; ++lid) {
        int e, tile_n, nh, nl, idx;
        hrl_entry(lid, tiles_n, e, tile_n);
        if (e != lid / tiles_n || tile_n != lid % tiles_n || tile_n < 0 || tile_n >= tiles_n) FAIL("entry");
        hrl_counts(c0, c1, total, nh, nl);
        if (nh < 0 || nl < 0 || nh + nl > total) FAIL("counts %d %d of %d", nh, nl, total);
        const int kind = hrl_kind(e, nh, nl, idx);
        if (kind == HRL_EXIT) { ++exited; continue; }
        // a list slot the honest lists do not have is never read
        if (idx < 0 || idx >= total) { FAIL("slot %d of %d", idx, total); continue; }
        if (!honest) continue;
        int b, x0, y0;
        if (nh >= total) {
            hrl_plain_corner(e, H, W, b, x0, y0);
            if (kind != HRL_HEAVY) FAIL("plain order but light");
            if (e != (b * ty + y0 / 8) * tx + x0 / 16) FAIL("plain corner");
        } else {
            if (idx >= (int)(kind == HRL_HEAVY ? heavy.size() : light.size())) { FAIL("slot past the list"); continue; }
            const int u = kind == HRL_HEAVY ? heavy[idx] : light[idx];
            if (!hrl_locate(u, B, H, W, b, x0, y0)) { FAIL("locate %d", u); continue; }
        }
        if (b < 0 || b >= B || x0 < 0 || x0 >= W || y0 < 0 || y0 >= H || x0 % 16 || y0 % 8) { FAIL("corner %d %d %d", b, x0, y0); continue; }
        // the sub-tile's class by the lists = the kind of the entry that visits it
        const int u_here = Cw4F::NS * ((b * ((H + 15) / 16) + y0 / 16) * ((W + 31) / 32) + x0 / 32) + 2 * ((y0 % 16) / 8) + (x0 % 32) / 16;
        bool is_heavy = false;
        for (int v : heavy) is_heavy |= v == u_here;
        if (is_heavy != (kind == HRL_HEAVY)) FAIL("kind of sub-tile %d", u_here);
        if (kind == HRL_HEAVY) last_heavy = lid; else if (lid < first_light) first_light = lid;
        ++seen[((size_t)(b * ty + y0 / 8) * tx + x0 / 16) * tiles_n + tile_n];
        ++walked;
    }
    if (!honest) return;
    if (last_heavy > first_light) FAIL("a light entry before a heavy one");
    for (int v : seen) if (v != 1) FAIL("(sub-tile, column tile) visited %d times (B=%d H=%d W=%d tn=%d mode=%d)", v, B, H, W, tiles_n, heavy_mode);
    // ids that are no sub-tile of the launch
    int b, x0, y0;
    const CwGrid g = cw_grid(B, H, W, CW_NB, 32, 16, CW_NB);
    if (hrl_locate(-1, B, H, W, b, x0, y0) || hrl_locate(g.tiles * Cw4F::NS, B, H, W, b, x0, y0) || hrl_locate(0x7fffffff, B, H, W, b, x0, y0)) FAIL("locate took a foreign id");
    for (int u = 0; u < g.tiles * Cw4F::NS; ++u) {
        bool in = false;
        for (int v : ids) in |= v == u;
        if (hrl_locate(u, B, H, W, b, x0, y0) != in) FAIL("locate(%d)", u);
    }
}

// every workgroup of a launch as a LIGHT one: the floats of the accumulator frame (1, H, W, N) / the channels [ycoff, ycoff + N) of the bf16 frame (1, H, W, YC)
static void light_case(int H, int W, int N, int YC, int ycoff) {
    std::vector<int> facc((size_t)H * W * N, 0), fcpy((size_t)H * W * YC, 0);
    for (int y0 = 0; y0 < H; y0 += 8)
        for (int x0 = 0; x0 < W; x0 += 16)
            for (int tile_n = 0; tile_n < N / HRL_BN; ++tile_n) {
                std::vector<int> sub((size_t)Cw4F::SX * Cw4F::SY * HRL_BN, 0);
                for (int wn = 0; wn < 4; ++wn)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int i = 0; i < HRL_TM; ++i) {
                            int py, px;
                            hrl_lane_pixel(lane, i, py, px);
                            if (py < 0 || py >= Cw4F::SY || px < 0 || px >= Cw4F::SX) { FAIL("lane pixel"); continue; }
                            const int oy = y0 + py, ox = x0 + px, khalf = lane >> 5, ncol = tile_n * HRL_BN + wn * 32;
                            if (oy >= H || ox >= W) continue;                    // a dead lane: nothing read beyond offset 0, nothing stored
                            const size_t o = hrl_acc_offset(oy, ox, W, N, ncol, khalf);
                            if (o % 4 != 0) FAIL("accumulator offset not a 16-byte piece");
                            for (int r = 0; r < 16; ++r) {
                                const int col = ncol + hrl_acc_column(khalf, r);
                                if (o + r >= facc.size()) { FAIL("accumulator offset outside the frame"); continue; }
                                ++facc[o + r];
                                ++sub[(size_t)(py * Cw4F::SX + px) * HRL_BN + col - tile_n * HRL_BN];
                                // the frame is the panel's columns per pixel: a 32-column tile is stored [khalf][r]
                                if (o + r != ((size_t)oy * W + ox) * N + (size_t)(ncol + 16 * khalf + r)) FAIL("accumulator layout");
                                ++elems;
                            }
                            const size_t c = hrl_copy_offset(oy, ox, W, YC, ycoff + ncol, khalf);
                            if (c % 8 != 0) FAIL("copy offset not a 16-byte piece");
                            for (int j = 0; j < 16; ++j) {
                                if (c + j >= fcpy.size()) { FAIL("copy offset outside the frame"); continue; }
                                if (c + j != ((size_t)oy * W + ox) * YC + (size_t)(ycoff + ncol + 16 * khalf + j)) FAIL("copy layout");
                                ++fcpy[c + j];
                            }
                        }
                for (int py = 0; py < Cw4F::SY; ++py)
                    for (int px = 0; px < Cw4F::SX; ++px)
                        for (int c = 0; c < HRL_BN; ++c)
                            if (sub[(size_t)(py * Cw4F::SX + px) * HRL_BN + c] != (y0 + py < H && x0 + px < W ? 1 : 0)) FAIL("(pixel, column) of a sub-tile");
            }
    for (int v : facc) if (v != 1) FAIL("accumulator float touched %d times (H=%d W=%d N=%d)", v, H, W, N);
    for (size_t k = 0; k < fcpy.size(); ++k) {
        const int ch = (int)(k % YC);
        if (fcpy[k] != (ch >= ycoff && ch < ycoff + N ? 1 : 0)) FAIL("bf16 channel %d touched %d times", ch, fcpy[k]);
    }
    // every register is one column of the tile, once
    for (int khalf = 0; khalf < 2; ++khalf) {
        std::set<int> cols;
        for (int r = 0; r < 16; ++r) cols.insert(hrl_acc_column(khalf, r));
        if (cols.size() != 16) FAIL("acc columns");
    }
}

static void contract_case() {
    LwgConvArgs a = {};
    a.B = 180, a.H = a.W = a.OH = a.OW = a.YH = a.YW = 512, a.C0 = 64, a.N = 128, a.YC = 128, a.M = 180 * 512 * 512, a.stride = 1, a.ntaps = 9, a.omul = 1;
    a.xdt = a.ydt = LWG_DT_BF16, a.epi = LWG_EPI_NONE;
    for (int t = 0; t < 9; ++t) a.dy[t] = (signed char)(t / 3 - 1), a.dx[t] = (signed char)(t % 3 - 1);
    if (!hrl_contract_ok(a)) FAIL("the 1024^2 site (180 frames, 6 GB of input) must pass: per-image descriptors");
    LwgConvArgs b = a;
    b.N = 64, b.YC = 64;
    if (hrl_contract_ok(b)) FAIL("N = 64");
    b = a, b.C1 = 64;
    if (hrl_contract_ok(b)) FAIL("two inputs");
    b = a, b.dy[0] = 1;
    if (hrl_contract_ok(b)) FAIL("tap order");
    b = a, b.epi = LWG_EPI_RESIDUAL;
    if (hrl_contract_ok(b)) FAIL("residual");
    b = a, b.epi = LWG_EPI_SPADE;
    if (hrl_contract_ok(b)) FAIL("SPADE with N != 2 YC");
    b.YC = 64;
    if (!hrl_contract_ok(b)) FAIL("SPADE");
    b = a, b.B = 1, b.H = b.OH = b.YH = 40000, b.W = b.OW = b.YW = 1024, b.M = 40000 * 1024;     // one image of 5.2 GB
    if (hrl_contract_ok(b)) FAIL("an image beyond the buffer range");
    b = a, b.xdt = LWG_DT_F32;
    if (hrl_contract_ok(b)) FAIL("fp32 input");
}

int main() {
    if (HRL_BN != 128 || HRL_TM != 4 || Cw4F::SX != 16 || Cw4F::SY != 8) FAIL("constants");
@MAIN@
    contract_case();
    printf("walked %llu exited %llu elems %llu bad %llu\n", walked, exited, elems, bad);
    return bad != 0;
}
"""


def _main():
    out = []
    for B, H, W in ((3, 40, 72), (3, 40, 48), (2, 8, 16), (1, 16, 16)):
        for tn in (1, 2, 4):
            for mode in (0, 1, 2, 3):
                out.append("    walk_case(%d, %d, %d, %d, %d, -1, -1);" % (B, H, W, tn, mode))
            # counts the classifier never writes: short of the grid (the rest exits), beyond it, negative
            for c0, c1 in ((2, 3), (1 << 30, 1 << 30), (-5, 7), (0, 1 << 30), (7, -1)):
                out.append("    walk_case(%d, %d, %d, %d, 3, %d, %d);" % (B, H, W, tn, c0, c1))
    for H, W in ((40, 72), (40, 48), (8, 16), (5, 7), (17, 33)):
        out.append("    light_case(%d, %d, 128, 128, 0);" % (H, W))
        out.append("    light_case(%d, %d, 256, 264, 8);" % (H, W))
    return "\n".join(out)


def _compiler():
    for c in (shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", shutil.which("g++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no host C++ compiler")


def test_walk_and_light_offsets():
    assert os.path.exists(os.path.join(CSRC, "lwg_bf16_hr_list.h"))
    with tempfile.TemporaryDirectory() as d:
        cpp, exe = os.path.join(d, "hrl.cpp"), os.path.join(d, "hrl")
        open(cpp, "w").write(_SRC.replace("@MAIN@", _main()))
        flags = ["-std=c++17", "-O1", "-fsanitize=signed-integer-overflow", "-fsanitize-trap=signed-integer-overflow", "-Wno-unused-variable", "-Wno-unused-function"]
        r = subprocess.run([_compiler(), *flags, "-I", CSRC, "-I", os.path.join(ROOT, "include"), cpp, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode >= 0, "signed overflow (trapped): " + r.stdout[-500:]
    assert r.returncode == 0, r.stdout[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert int(last[1]) > 3000 and int(last[3]) > 100 and int(last[5]) > 10 ** 5 and int(last[7]) == 0, r.stdout[-500:]


def test_kernel_goes_through_the_shared_functions():
    """The kernel, its light path and the entry points use the functions audited above; the sub-tile constants stay those of lwg_conv_wino.h."""
    k = open(os.path.join(CSRC, "conv_igemm_bf16.hip")).read()
    for call in ("hrl_entry(lid, tiles_n, e, tile_n)", "hrl_counts(", "hrl_kind(e, nh, nl, idx)", "hrl_plain_corner(e, a.OH, a.OW, tb, x0, y0)",
                 "hrl_locate(u, a.B, a.OH, a.OW, tb, x0, y0)", "hrl_lane_pixel(lane, i, py, px)", "hrl_acc_offset(", "hrl_copy_offset(", "hrl_contract_ok(",
                 "hrl_grid(a.B, a.OH, a.OW, a.N / HRL_BN)"):
        assert call in k, call
    h = open(os.path.join(CSRC, "lwg_bf16_hr_list.h")).read()
    for own in ("Cw4Sub<", "struct Cw4", "#define SX", "int SX ="):
        assert own not in h and own not in k, own
    assert '#include "lwg_conv_wino.h"' in h and "Cw4F::SX" in h


# ---- the window reach d: a numpy model of the two SPADE convolutions as the direct kernel computes them ----

def _conv3(x, w):
    """3 x 3 / stride 1 / zero padding 1, integers: x (H, W, C), w (3, 3, C, N)."""
    H, W, _ = x.shape
    xp = np.zeros((H + 2, W + 2, x.shape[2]), dtype=np.int64)
    xp[1:-1, 1:-1] = x
    return sum(np.tensordot(xp[r:r + H, s:s + W], w[r, s], axes=1) for r in range(3) for s in range(3))


def _light(fg, d):
    """The classifier's rule on a foreground mask (H, W): sub-tile (sy, sx) is light when its window - the 16 x 8 sub-tile grown by d - holds no foreground."""
    H, W = fg.shape
    out = {}
    for y0 in range(0, H, 8):
        for x0 in range(0, W, 16):
            out[(y0, x0)] = not fg[max(y0 - d, 0):y0 + 8 + d, max(x0 - d, 0):x0 + 16 + d].any()
    return out


def _violations(d1, d2, fg_pixels, H=40, W=48):
    """Light sub-tiles (by d1 for `shared`, by d2 for the convolution behind it) whose result differs from the calibration frame's, over single
    foreground pixels.  The second convolution reads the first one's list-driven output (light sub-tiles filled from the calibration)."""
    rng = np.random.RandomState(5)
    C = 3
    w1 = rng.randint(1, 4, size=(3, 3, C, C)).astype(np.int64)       # positive: no difference cancels
    w2 = rng.randint(1, 4, size=(3, 3, C, C)).astype(np.int64)
    bg = np.array([1, 2, 3], dtype=np.int64)                         # att = one vector wherever no source has a tap
    cal_att = np.broadcast_to(bg, (H, W, C)).copy()
    cal_actv = np.maximum(_conv3(cal_att, w1) - 20, 0)               # (a bias, so that the ReLU is live somewhere and not everywhere)
    cal_gb = _conv3(cal_actv, w2)
    bad1 = bad2 = n_light = 0
    for (fy, fx) in fg_pixels:
        fg = np.zeros((H, W), dtype=bool)
        fg[fy, fx] = True
        att = cal_att.copy()
        att[fy, fx] = bg + 100
        actv_true = np.maximum(_conv3(att, w1) - 20, 0)
        gb_true = _conv3(actv_true, w2)
        l1, l2 = _light(fg, d1), _light(fg, d2)
        actv = actv_true.copy()
        for (y0, x0), lt in l1.items():
            if lt:
                n_light += 1
                bad1 += not np.array_equal(actv_true[y0:y0 + 8, x0:x0 + 16], cal_actv[y0:y0 + 8, x0:x0 + 16])
                actv[y0:y0 + 8, x0:x0 + 16] = cal_actv[y0:y0 + 8, x0:x0 + 16]
        gb = _conv3(actv, w2)
        for (y0, x0), lt in l2.items():
            if lt:
                gb[y0:y0 + 8, x0:x0 + 16] = cal_gb[y0:y0 + 8, x0:x0 + 16]
        bad2 += not np.array_equal(gb, gb_true)
    assert n_light > 0
    return bad1, bad2


# single foreground pixels at distance 1, 2, 3 from a sub-tile's edge (x = 16, y = 8) and corner (16, 8), at the image's corners and on the ragged edge
_FG = [(4, 15), (4, 14), (4, 13), (7, 20), (6, 20), (5, 20), (7, 15), (6, 14), (5, 13), (8, 16), (9, 17), (0, 0), (39, 47), (39, 0), (20, 31), (23, 32), (24, 32)]


def test_d_1_2_is_sufficient_and_0_1_is_not():
    from ipercore_amd import ops
    assert ops.SPADE_SKIP_D_BF16 == (1, 2)
    assert _violations(1, 2, _FG) == (0, 0)
    b1, _ = _violations(0, 2, _FG)
    assert b1 > 0, "d = 0 for `shared` must leave a light sub-tile that differs: a pixel next to the sub-tile's edge reads it"
    _, b2 = _violations(1, 1, _FG)
    assert b2 > 0, "d = 1 for the gamma | beta convolution must leave a light sub-tile that differs: it reads actv one pixel further"
    b1, b2 = _violations(0, 1, _FG)
    assert b1 > 0 and b2 > 0
    # ... and nothing larger is needed: one more pixel of reach only turns light sub-tiles heavy
    assert _violations(2, 3, _FG) == (0, 0)
