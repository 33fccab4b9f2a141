"""CPU checks of the integer arithmetic behind the sub-tile form of the list-driven F(4x4, 3x3) convolution (csrc/lwg_conv_wino.h part 1: Cw4F =
Cw4Sub<16, 8> - corner, reached, slot_of_patch, slot_index, halo_voff, light_pixel - and cw4_halo_elem) - the very functions the kernels
compile, built into a host program with signed-overflow traps as tests/test_spade_skip_cpu.py does.

  * sub-tile numbering and windows: sub-tile 4 t + s of block t, its corner, its window against the definition pixel by pixel, which sub-tiles lie in
    the image - on ragged images (40 x 72: the lower sub-tiles of the last block row and the right ones of the last block column are outside);
  * the classifier's one-pass rule: bit s of Cw4F::reached = "the pixel lies in sub-tile s's window", and on random foreground masks the block's mark is
    the OR of its in-image sub-tiles' marks;
  * the group walk of every workgroup for heavy counts 0, 1, 3, 4, 5 and 4 k + 2 and 2, 4, 8 column blocks: every (sub-tile, column block) exactly
    once, empty slots only in the last group; the light entries behind them exactly once;
  * the slot-to-patch mapping: a group that is one whole block has the plain block's patch numbering;
  * the halo staging: the 1 536 staged elements are the four slots' 360 halo elements exactly once, a wave round belongs to one slot, offsets against
    their definition; a light sub-tile's elements: every (pixel, channel quad) exactly once."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ipercore_amd", "csrc")

_SRC = r"""
#include <cstdio>
#include <vector>
#include "lwg_conv_wino.h"
typedef unsigned long long u64;
static u64 bad = 0, subs = 0, walked = 0, elems = 0, masks = 0;
static unsigned rng = 12345u;
static unsigned rnd() { rng = rng * 1664525u + 1013904223u; return rng >> 8; }
#define FAIL(...) do { if (bad++ < 12) { printf("BAD " __VA_ARGS__); printf("\n"); } } while (0)

static void numbering_case(int B, int H, int W, int d) {
    const CwGrid g = cw_grid(B, H, W, 64, 32, 16, 64);
    int inside = 0;
    for (int t = 0; t < g.tiles; ++t) {
        const int b = cw_image(g, t);
        int bx0, by0;
        cw_corner(g, t - b * g.bx * g.by, 32, 16, bx0, by0);
        const CwWindow bw = cw_block_window(bx0, by0, 32, 16, d, H, W);
        for (int s = 0; s < Cw4F::NS; ++s) {
            int ub, x0, y0;
            Cw4F::corner(g, Cw4F::NS * t + s, ub, x0, y0);
            if (ub != b || x0 != bx0 + (s & 1) * 16 || y0 != by0 + (s >> 1) * 8) FAIL("corner t=%d s=%d: %d %d %d", t, s, ub, x0, y0);
            const bool in = Cw4F::in_image(x0, y0, H, W);
            if (in != (x0 < W && y0 < H)) FAIL("in_image");
            inside += in;
            ++subs;
        }
        // every image pixel: bit s of Cw4F::reached <=> inside sub-tile s's window; the block's window = the union of the in-image sub-tiles' windows
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const unsigned m = Cw4F::reached(x, y, bx0, by0, d);
                bool any_in = false;
                for (int s = 0; s < Cw4F::NS; ++s) {
                    const int x0 = bx0 + (s & 1) * 16, y0 = by0 + (s >> 1) * 8;
                    const CwWindow w = cw_block_window(x0, y0, Cw4F::SX, Cw4F::SY, d, H, W);
                    const bool want = x >= w.x0 && x < w.x1 && y >= w.y0 && y < w.y1;
                    const bool def = x >= x0 - d && x < x0 + 16 + d && y >= y0 - d && y < y0 + 8 + d;
                    if (want != def || want != (((m >> s) & 1u) != 0)) FAIL("reached H=%d W=%d d=%d t=%d s=%d (%d, %d)", H, W, d, t, s, x, y);
                    any_in |= want && Cw4F::in_image(x0, y0, H, W);
                }
                const bool inb = x >= bw.x0 && x < bw.x1 && y >= bw.y0 && y < bw.y1;
                if (inb != any_in) FAIL("union H=%d W=%d d=%d t=%d (%d, %d)", H, W, d, t, x, y);
            }
    }
    if (inside != Cw4F::in_image_total(B, H, W)) FAIL("in-image total H=%d W=%d: %d != %d", H, W, inside, Cw4F::in_image_total(B, H, W));
}

// random foreground masks: marks as the classifier forms them (one pass over the block's window, Cw4F::reached) against the definition; block = OR
static void mask_case(int H, int W, int d, int permille) {
    const CwGrid g = cw_grid(1, H, W, 64, 32, 16, 64);
    std::vector<char> fg((size_t)H * W);
    for (auto& v : fg) v = (int)(rnd() % 1000u) < permille;
    for (int t = 0; t < g.tiles; ++t) {
        int bx0, by0;
        cw_corner(g, t, 32, 16, bx0, by0);
        const CwWindow bw = cw_block_window(bx0, by0, 32, 16, d, H, W);
        unsigned all = 0;
        bool blk = false;
        for (int y = bw.y0; y < bw.y1; ++y)
            for (int x = bw.x0; x < bw.x1; ++x)
                if (fg[(size_t)y * W + x]) blk = true, all |= Cw4F::reached(x, y, bx0, by0, d);
        bool orr = false;
        for (int s = 0; s < Cw4F::NS; ++s) {
            const int x0 = bx0 + (s & 1) * 16, y0 = by0 + (s >> 1) * 8;
            const CwWindow w = cw_block_window(x0, y0, Cw4F::SX, Cw4F::SY, d, H, W);
            bool want = false;
            for (int y = w.y0; y < w.y1; ++y)
                for (int x = w.x0; x < w.x1; ++x) want |= fg[(size_t)y * W + x] != 0;
            if (!Cw4F::in_image(x0, y0, H, W)) continue;
            if (want != (((all >> s) & 1u) != 0)) FAIL("mark H=%d W=%d d=%d t=%d s=%d", H, W, d, t, s);
            orr |= want;
        }
        if (orr != blk) FAIL("block mark != OR H=%d W=%d d=%d t=%d", H, W, d, t);
        ++masks;
    }
}

// nh heavy and nl light sub-tiles (ids: heavy 3 i + 1, light 3 i + 2), ncb column blocks, nwg workgroups
static void walk_case(int nh, int nl, int ncb, int nwg) {
    const int ngrp = Cw4F::groups(nh), nhe = ngrp * ncb, nle = nl * ncb;
    std::vector<int> hseen((size_t)nh * ncb, 0), lseen((size_t)nl * ncb, 0);
    for (int wg = 0; wg < nwg; ++wg) {
        int id = wg;
        for (; id < nhe; id += nwg) {
            int grp, cb;
            cw_list_entry(id, ncb, grp, cb);
            if (grp < 0 || grp >= ngrp || cb < 0 || cb >= ncb) { FAIL("entry"); continue; }
            int empty = 0;
            for (int k = 0; k < Cw4F::NS; ++k) {
                const int ix = Cw4F::slot_index(grp, k, nh);
                if (ix < 0) { ++empty; continue; }
                if (ix != grp * Cw4F::NS + k || ix >= nh || empty) { FAIL("slot index nh=%d grp=%d k=%d", nh, grp, k); continue; }      // (empty slots: trailing only)
                ++hseen[(size_t)ix * ncb + cb];
            }
            if (empty && grp != ngrp - 1) FAIL("empty slot in group %d of %d (nh=%d)", grp, ngrp, nh);
            if (empty != (grp == ngrp - 1 ? ngrp * Cw4F::NS - nh : 0)) FAIL("empty count nh=%d grp=%d", nh, grp);
            ++walked;
        }
        if (cw_list_first_light(wg, nwg, nhe) != id) FAIL("first light");
        for (; id < nhe + nle; id += nwg) {
            int slot, cb;
            cw_list_entry(id - nhe, ncb, slot, cb);
            if (slot < 0 || slot >= nl || cb < 0 || cb >= ncb) { FAIL("light entry"); continue; }
            ++lseen[(size_t)slot * ncb + cb];
            ++walked;
        }
    }
    for (int v : hseen) if (v != 1) FAIL("heavy sub-tile visited %d times (nh=%d ncb=%d nwg=%d)", v, nh, ncb, nwg);
    for (int v : lseen) if (v != 1) FAIL("light sub-tile visited %d times (nl=%d ncb=%d nwg=%d)", v, nl, ncb, nwg);
}

static void patch_case(int B, int H, int W) {
    const CwGrid g = cw_grid(B, H, W, 64, 32, 16, 64);
    for (int t = 0; t < g.tiles; ++t) {
        const int b = cw_image(g, t);
        int bx0, by0;
        cw_corner(g, t - b * g.bx * g.by, 32, 16, bx0, by0);
        for (int pty = 0; pty < 4; ++pty)
            for (int ptx = 0; ptx < 8; ++ptx) {
                const int s = Cw4F::slot_of_patch(pty, ptx);
                int ly, lx, ub, x0, y0;
                Cw4F::patch_in_slot(pty, ptx, ly, lx);
                Cw4F::corner(g, Cw4F::NS * t + s, ub, x0, y0);
                if (s != (pty >> 1) * 2 + (ptx >> 2) || ub != b || x0 + 4 * lx != bx0 + 4 * ptx || y0 + 4 * ly != by0 + 4 * pty) FAIL("patch t=%d (%d, %d)", t, pty, ptx);
                // the epilogue's reader: pass ph of the wave pair wid / 4 reads patches of ONE slot
                ++elems;
            }
    }
}

static void halo_case(int H, int W, int C, int x0, int y0) {
    std::vector<int> seen((size_t)Cw4F::NS * Cw4F::NEL, 0);
    for (int i = 0; i < 3 * 512; ++i) {
        int s, j, s0, j0;
        cw4_halo_elem(Cw4F{}, i, s, j);
        cw4_halo_elem(Cw4F{}, i & ~63, s0, j0);
        if (s != s0 || s < 0 || s >= Cw4F::NS || j < 0) { FAIL("halo elem %d", i); continue; }       // a wave round: one slot
        if (j >= Cw4F::NEL) {
            if (Cw4F::halo_voff(true, j, x0, y0, H, W, C) != CW_OOB) FAIL("halo: no element but an offset");
            continue;
        }
        ++seen[(size_t)s * Cw4F::NEL + j];
        int hy, hx, hq;
        Cw4F::halo_place(j, hy, hx, hq);
        if (hy < 0 || hy >= Cw4F::HH || hx < 0 || hx >= Cw4F::HW || hq < 0 || hq > 1 || (hy * Cw4F::HW + hx) * 2 + hq != j) FAIL("halo place %d", j);
        const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const unsigned want = in ? (unsigned)(((long long)gy * W + gx) * C + 4 * hq) * 4u : CW_OOB;
        if (Cw4F::halo_voff(true, j, x0, y0, H, W, C) != want) FAIL("halo voff (%d, %d) j=%d", x0, y0, j);
        if (Cw4F::halo_voff(false, j, x0, y0, H, W, C) != CW_OOB) FAIL("halo voff of an empty slot");
        ++elems;
    }
    for (int v : seen) if (v != 1) FAIL("halo element staged %d times", v);
}

static void light_case(int nq) {
    const int npass = Cw4F::SX * Cw4F::SY * nq / 512;
    std::vector<int> seen((size_t)Cw4F::SX * Cw4F::SY * nq, 0);
    for (int tid = 0; tid < 512; ++tid) {
        int q0 = -1;
        for (int it = 0; it < npass; ++it) {
            int px, py, q4;
            cw4_light_elem(tid, it, 512, nq, px, py, q4);
            Cw4F::light_pixel(px, py);
            if (px < 0 || px >= Cw4F::SX || py < 0 || py >= Cw4F::SY || q4 < 0 || q4 >= nq) { FAIL("light elem"); continue; }
            if (it == 0) q0 = q4;
            if (q4 != q0) FAIL("light quad");
            ++seen[(size_t)(py * Cw4F::SX + px) * nq + q4];
            ++elems;
        }
    }
    for (int v : seen) if (v != 1) FAIL("light element %d times (nq=%d)", v, nq);
}

int main() {
    if (Cw4F::NS != 4 || Cw4F::SX * Cw4F::NSX != 32 || Cw4F::SY * (Cw4F::NS / Cw4F::NSX) != 16 || Cw4F::NS * Cw4F::ROUNDS * 64 != 3 * 512 || Cw4F::NEL != 360) FAIL("constants");
@MAIN@
    printf("subs %llu masks %llu walked %llu elems %llu bad %llu\n", subs, masks, walked, elems, bad);
    return bad != 0;
}
"""


def _main():
    out = []
    for H, W in ((40, 72), (64, 64), (16, 32), (1, 1), (17, 33), (9, 17), (8, 16), (32, 32)):
        for d in (0, 1, 5, 6):
            out.append("    numbering_case(2, %d, %d, %d);" % (H, W, d))
        for d in (1, 5):
            for pm in (1, 5, 30):
                out.append("    mask_case(%d, %d, %d, %d);" % (H, W, d, pm))
        out.append("    patch_case(3, %d, %d);" % (H, W))
    for nh in (0, 1, 3, 4, 5, 4 * 7 + 2, 4 * 300 + 2, 4 * 64):
        for ncb in (2, 4, 8):
            for nwg in (256, 8, 5):
                for nl in (0, 3, 700):
                    out.append("    walk_case(%d, %d, %d, %d);" % (nh, nl, ncb, nwg))
    for H, W, x0, y0 in ((40, 72, 0, 0), (40, 72, 64, 32), (40, 72, 64, 40), (64, 64, 48, 56), (64, 64, 16, 8), (5, 7, 0, 0)):
        out.append("    halo_case(%d, %d, 64, %d, %d);" % (H, W, x0, y0))
    out += ["    light_case(8);", "    light_case(16);"]
    return "\n".join(out)


def _compiler():
    for c in (shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", shutil.which("g++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no host C++ compiler")


def test_subtiles_groups_slots_and_halo():
    with tempfile.TemporaryDirectory() as d:
        cpp, exe = os.path.join(d, "fine.cpp"), os.path.join(d, "fine")
        open(cpp, "w").write(_SRC.replace("@MAIN@", _main()))
        flags = ["-std=c++17", "-O1", "-fsanitize=signed-integer-overflow", "-fsanitize-trap=signed-integer-overflow", "-Wno-unused-variable", "-Wno-unused-function"]
        r = subprocess.run([_compiler(), *flags, "-I", CSRC, cpp, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode >= 0, "signed overflow (trapped): " + r.stdout[-500:]
    assert r.returncode == 0, r.stdout[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert int(last[1]) > 500 and int(last[3]) > 100 and int(last[5]) > 10 ** 4 and int(last[7]) > 10 ** 4 and int(last[9]) == 0, r.stdout[-500:]


def test_kernels_use_the_shared_functions():
    """The sub-tile kernel and the classifier go through the functions audited above - by the geometry parameter G, which the 16 x 8 entry points
    instantiate with Cw4F - and there is ONE definition of the sub-tile geometry."""
    rd = lambda n: open(os.path.join(CSRC, n)).read()      # noqa: E731
    k = rd("conv_winograd4.hip")
    for call in ("G::slot_index(slot, k, nht)", "cw4_halo_elem(G{}, tids + NTH * k, s, j)", "G::halo_voff(u >= 0, j, x0, y0, H, W, a.C0)", "G::slot_of_patch(pty, ptx)",
                 "G::patch_in_slot(pty, ptx, pby, pbx)", "G::light_pixel(px, py)", "G::in_image_total(a.B, H, W)", "G::groups(nht)",
                 "lwg_wino4_lists_go<Cw4F>(pa, pl, stream_)"):
        assert call in k, call
    c = rd("spade_skip.hip")
    assert "GS::reached(x, y, x0, y0, d)" in c and "G::in_image(" in c and "sk_lists<Cw4F>(" in c
    for own in ("struct Cw4Sub", "Cw4Sub<", "#define SX", "int SX ="):
        assert own not in k and own not in c, own
    h = rd("lwg_conv_wino.h")
    assert h.count("struct Cw4Sub") == 1 and h.count("using Cw4F = Cw4Sub<16, 8>;") == 1 and h.count("Cw4Sub<") == 2
