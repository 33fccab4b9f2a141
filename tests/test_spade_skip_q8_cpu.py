"""CPU checks of the integer arithmetic behind the 8 x 8 sub-tile form of the list-driven F(4x4, 3x3) convolution (csrc/lwg_conv_wino.h part 1:
Cw4Q = Cw4Sub<8, 8>, cw4_halo_elem, Cw4QLds, cw4_reader8, cw4_marks16_of8) - the very functions the kernels compile, built into a host program with signed-overflow traps as tests/test_spade_skip_fine_cpu.py
does for the 16 x 8 form.

  * numbering, corners and windows: sub-tile 8 t + 4 r + c of block t on ragged images (40 x 72, 8 x 8, one row), which sub-tiles lie in the image;
  * Cw4Q::reached against the definition pixel by pixel for d in {0, 1, 5, 6}; on random foreground masks the block's mark is the OR of the eight and
    a 16 x 8 mark (Cw4F::reached's) the OR of its two halves (cw4_marks16_of8);
  * the group walk of every workgroup for heavy counts 0, 1, 7, 8, 9, 8 k + 3 and 2, 4, 8 column blocks: every (sub-tile, column block) exactly once,
    empty slots only at the end of the last group; the light entries behind them exactly once;
  * slot <-> patch: the 32 patches are the eight slots' 2 x 2 exactly once, a group that is one whole block has the plain block's patch positions;
  * the halo staging: the 2 048 staged elements hold the eight slots' 200 halo elements exactly once, a wave stages one slot, offsets against their
    definition, every element's place inside the channel plane in range and distinct;
  * bank quads: the sixteen patches of either ds_read_b128 lane group of the input transform start in sixteen distinct bank quads, for every one
    of the six rows read; the epilogue reader's patches of a wave and pass are the 2 x 2 of ONE slot (4 pass + wave / 2), its (output column, patch)
    pairs cover the block once, and a lane group reads the eight channel quads of patches a and a + 8;
  * a light sub-tile's elements: every (pixel, channel quad) of the 64 pixels exactly once."""
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
#include <set>
#include "lwg_conv_wino.h"
typedef unsigned long long u64;
static u64 bad = 0, subs = 0, walked = 0, elems = 0, masks = 0;
static unsigned rng = 4711u;
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
        for (int s = 0; s < Cw4Q::NS; ++s) {
            int ub, x0, y0;
            Cw4Q::corner(g, Cw4Q::NS * t + s, ub, x0, y0);
            if (ub != b || x0 != bx0 + (s & 3) * 8 || y0 != by0 + (s >> 2) * 8) FAIL("corner t=%d s=%d: %d %d %d", t, s, ub, x0, y0);
            const bool in = Cw4Q::in_image(x0, y0, H, W);
            if (in != (x0 < W && y0 < H)) FAIL("in_image");
            inside += in;
            ++subs;
        }
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const unsigned m = Cw4Q::reached(x, y, bx0, by0, d);
                bool any_in = false;
                for (int s = 0; s < Cw4Q::NS; ++s) {
                    const int x0 = bx0 + (s & 3) * 8, y0 = by0 + (s >> 2) * 8;
                    const CwWindow w = cw_block_window(x0, y0, Cw4Q::SX, Cw4Q::SY, d, H, W);
                    const bool want = x >= w.x0 && x < w.x1 && y >= w.y0 && y < w.y1;
                    const bool def = x >= x0 - d && x < x0 + 8 + d && y >= y0 - d && y < y0 + 8 + d;
                    if (want != def || want != (((m >> s) & 1u) != 0)) FAIL("reached H=%d W=%d d=%d t=%d s=%d (%d, %d)", H, W, d, t, s, x, y);
                    any_in |= want && Cw4Q::in_image(x0, y0, H, W);
                }
                const bool inb = x >= bw.x0 && x < bw.x1 && y >= bw.y0 && y < bw.y1;
                if (inb != any_in) FAIL("union H=%d W=%d d=%d t=%d (%d, %d)", H, W, d, t, x, y);
                if (cw4_marks16_of8(m) != Cw4F::reached(x, y, bx0, by0, d)) FAIL("16 x 8 bits H=%d W=%d d=%d t=%d (%d, %d)", H, W, d, t, x, y);
            }
    }
    if (inside != Cw4Q::in_image_total(B, H, W)) FAIL("in-image total H=%d W=%d: %d != %d", H, W, inside, Cw4Q::in_image_total(B, H, W));
}

// random foreground masks: the marks as the classifier forms them (one pass over the block's window) against the definition; block = OR of the
// eight, 16 x 8 sub-tile = OR of its two
static void mask_case(int H, int W, int d, int permille) {
    const CwGrid g = cw_grid(1, H, W, 64, 32, 16, 64);
    std::vector<char> fg((size_t)H * W);
    for (auto& v : fg) v = (int)(rnd() % 1000u) < permille;
    for (int t = 0; t < g.tiles; ++t) {
        int bx0, by0;
        cw_corner(g, t, 32, 16, bx0, by0);
        const CwWindow bw = cw_block_window(bx0, by0, 32, 16, d, H, W);
        unsigned all = 0, all16 = 0;
        bool blk = false;
        for (int y = bw.y0; y < bw.y1; ++y)
            for (int x = bw.x0; x < bw.x1; ++x)
                if (fg[(size_t)y * W + x]) blk = true, all |= Cw4Q::reached(x, y, bx0, by0, d), all16 |= Cw4F::reached(x, y, bx0, by0, d);
        bool orr = false;
        unsigned want8 = 0;
        for (int s = 0; s < Cw4Q::NS; ++s) {
            const int x0 = bx0 + (s & 3) * 8, y0 = by0 + (s >> 2) * 8;
            const CwWindow w = cw_block_window(x0, y0, Cw4Q::SX, Cw4Q::SY, d, H, W);
            bool want = false;
            for (int y = w.y0; y < w.y1; ++y)
                for (int x = w.x0; x < w.x1; ++x) want |= fg[(size_t)y * W + x] != 0;
            want8 |= (want ? 1u : 0u) << s;
            if (!Cw4Q::in_image(x0, y0, H, W)) continue;
            if (want != (((all >> s) & 1u) != 0)) FAIL("mark H=%d W=%d d=%d t=%d s=%d", H, W, d, t, s);
            orr |= want;
        }
        if (orr != blk) FAIL("block mark != OR H=%d W=%d d=%d t=%d", H, W, d, t);
        for (int f = 0; f < Cw4F::NS; ++f) {
            const int a = 4 * (f >> 1) + 2 * (f & 1);
            const bool two = ((want8 >> a) & 1u) || ((want8 >> (a + 1)) & 1u);
            if (two != (((all16 >> f) & 1u) != 0) || two != (((cw4_marks16_of8(all) >> f) & 1u) != 0)) FAIL("16 x 8 mark != OR of its two H=%d W=%d d=%d t=%d f=%d", H, W, d, t, f);
        }
        ++masks;
    }
}

static void walk_case(int nh, int nl, int ncb, int nwg) {
    const int ngrp = Cw4Q::groups(nh), nhe = ngrp * ncb, nle = nl * ncb;
    std::vector<int> hseen((size_t)nh * ncb, 0), lseen((size_t)nl * ncb, 0);
    for (int wg = 0; wg < nwg; ++wg) {
        int id = wg;
        for (; id < nhe; id += nwg) {
            int grp, cb;
            cw_list_entry(id, ncb, grp, cb);
            if (grp < 0 || grp >= ngrp || cb < 0 || cb >= ncb) { FAIL("entry"); continue; }
            int empty = 0;
            for (int k = 0; k < Cw4Q::NS; ++k) {
                const int ix = Cw4Q::slot_index(grp, k, nh);
                if (ix < 0) { ++empty; continue; }
                if (ix != grp * Cw4Q::NS + k || ix >= nh || empty) { FAIL("slot index nh=%d grp=%d k=%d", nh, grp, k); continue; }
                ++hseen[(size_t)ix * ncb + cb];
            }
            if (empty != (grp == ngrp - 1 ? ngrp * Cw4Q::NS - nh : 0)) FAIL("empty count nh=%d grp=%d", nh, grp);
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
        int per[Cw4Q::NS][2][2] = {};
        for (int pty = 0; pty < 4; ++pty)
            for (int ptx = 0; ptx < 8; ++ptx) {
                const int s = Cw4Q::slot_of_patch(pty, ptx);
                int ly, lx, ub, x0, y0;
                Cw4Q::patch_in_slot(pty, ptx, ly, lx);
                Cw4Q::corner(g, Cw4Q::NS * t + s, ub, x0, y0);
                if (s != 4 * (pty / 2) + ptx / 2 || ly < 0 || ly > 1 || lx < 0 || lx > 1 || ub != b || x0 + 4 * lx != bx0 + 4 * ptx || y0 + 4 * ly != by0 + 4 * pty) { FAIL("patch t=%d (%d, %d)", t, pty, ptx); continue; }
                ++per[s][ly][lx];
                ++elems;
            }
        for (int s = 0; s < Cw4Q::NS; ++s)
            for (int i = 0; i < 4; ++i) if (per[s][i >> 1][i & 1] != 1) FAIL("slot %d patch %d: %d times", s, i, per[s][i >> 1][i & 1]);
    }
}

static void halo_case(int H, int W, int C, int x0, int y0) {
    std::vector<int> seen((size_t)Cw4Q::NS * Cw4Q::NEL, 0);
    std::set<int> places;
    for (int i = 0; i < Cw4Q::ROUNDS * 512; ++i) {
        int s, j;
        cw4_halo_elem(Cw4Q{}, i, s, j);
        if (s != ((i >> 6) & 7) || j < 0 || j >= Cw4Q::ROUNDS * 64) { FAIL("halo elem %d", i); continue; }       // a wave: one slot
        if (j >= Cw4Q::NEL) {
            if (Cw4Q::halo_voff(true, j, x0, y0, H, W, C) != CW_OOB) FAIL("halo: no element but an offset");
            continue;
        }
        ++seen[(size_t)s * Cw4Q::NEL + j];
        int hy, hx, hq;
        Cw4Q::halo_place(j, hy, hx, hq);
        if (hy < 0 || hy >= Cw4Q::HH || hx < 0 || hx >= Cw4Q::HW || hq < 0 || hq > 1 || (hy * Cw4Q::HW + hx) * 2 + hq != j) FAIL("halo place %d", j);
        const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const unsigned want = in ? (unsigned)(((long long)gy * W + gx) * C + 4 * hq) * 4u : CW_OOB;
        if (Cw4Q::halo_voff(true, j, x0, y0, H, W, C) != want) FAIL("halo voff (%d, %d) j=%d", x0, y0, j);
        if (Cw4Q::halo_voff(false, j, x0, y0, H, W, C) != CW_OOB) FAIL("halo voff of an empty slot");
        // its place in the LDS buffer: the kernel's expression - four channel planes from 4 hq PLANE on
        for (int k = 0; k < 4; ++k) {
            const int at = (4 * hq + k) * Cw4QLds::PLN + Cw4QLds::slot(s) + hy * Cw4QLds::RS + hx;
            if (at < 0 || at >= 8 * Cw4QLds::PLN || Cw4QLds::slot(s) + hy * Cw4QLds::RS + hx >= Cw4QLds::PLN || !places.insert(at).second) FAIL("LDS place slot %d j=%d", s, j);
        }
        ++elems;
    }
    for (int v : seen) if (v != 1) FAIL("halo element staged %d times", v);
    // the transform reads rows of 6 floats (16 + 8 bytes) of the patch's 6 x 6 window: inside its slot's sub-plane, 16-byte aligned
    for (int pty = 0; pty < 4; ++pty)
        for (int ptx = 0; ptx < 8; ++ptx) {
            int ly, lx;
            Cw4Q::patch_in_slot(pty, ptx, ly, lx);
            const int base = Cw4QLds::patch(pty, ptx), slot = Cw4QLds::slot(Cw4Q::slot_of_patch(pty, ptx));
            if ((base & 3) || (Cw4QLds::RS & 3) || (Cw4QLds::PLN & 3) || base != slot + 4 * ly * Cw4QLds::RS + 4 * lx) FAIL("patch base (%d, %d)", pty, ptx);
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c < 6; ++c)
                    if (!places.count(base + r * Cw4QLds::RS + c)) FAIL("patch (%d, %d) reads (%d, %d) outside the staged halo", pty, ptx, r, c);
        }
}

// ds_read_b128: a half wave is served in the lane groups {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}; a 16-byte access lies in bank quad (float
// offset / 4) % 16.  The transform's thread: patch = lane % 32 (pty = patch / 8, ptx = patch % 8), the half waves 8 channel planes apart.
static void bank_case() {
    const unsigned G0 = 0x0FF0F00Fu;
    for (int grp = 0; grp < 2; ++grp)
        for (int r = 0; r < 6; ++r) {
            unsigned used = 0;
            int n = 0;
            for (int l = 0; l < 32; ++l) {
                if ((((G0 >> l) & 1u) != 0) != (grp == 0)) continue;
                const int off = Cw4QLds::patch(l >> 3, l & 7) + r * Cw4QLds::RS;
                used |= 1u << ((off >> 2) & 15);
                ++n;
            }
            if (n != 16 || used != 0xFFFFu) FAIL("transform row %d, lane group %d: bank quads %04x", r, grp, used);
            ++elems;
        }
    if ((4 * Cw4QLds::PLN) % 32 != 16) FAIL("the two channel quads of a pixel share a bank");
    // the epilogue's reader
    int cover[2][16][4] = {};
    for (int wid = 0; wid < 8; ++wid)
        for (int ph = 0; ph < 2; ++ph) {
            for (int lane = 0; lane < 64; ++lane) {
                int rb, p16;
                cw4_reader8(wid, lane, rb, p16);
                if (rb < 0 || rb > 3 || p16 < 0 || p16 > 15) { FAIL("reader wid=%d lane=%d", wid, lane); continue; }
                int rb0, p0;
                cw4_reader8(wid, lane & 32, rb0, p0);
                if (rb != rb0) FAIL("reader: a half wave has two output columns");
                const int p = 16 * ph + p16;
                if (Cw4Q::slot_of_patch(p >> 3, p & 7) != 4 * ph + wid / 2) FAIL("reader wid=%d pass %d lane=%d: slot %d", wid, ph, lane, Cw4Q::slot_of_patch(p >> 3, p & 7));
                ++cover[ph][p16][rb];
            }
            // a lane group: the eight channel quads (exchange rows of 68 floats: bank quad (patch + quad) % 16) of patches a and a + 8
            for (int half = 0; half < 2; ++half)
                for (int grp = 0; grp < 2; ++grp) {
                    unsigned used = 0;
                    for (int l = 0; l < 32; ++l) {
                        if ((((G0 >> l) & 1u) != 0) != (grp == 0)) continue;
                        int rb, p16;
                        cw4_reader8(wid, 32 * half + l, rb, p16);
                        const unsigned l5 = (unsigned)l, gsel = (G0 >> l5) & 1u;
                        const int gidx = __builtin_popcount((gsel ? G0 : ~G0) & ((1u << l5) - 1u));
                        used |= 1u << ((p16 * 17 + (gidx & 7)) & 15);       // 68 floats = 17 quads per patch row
                    }
                    if (used != 0xFFFFu) FAIL("reader wid=%d half %d group %d: bank quads %04x", wid, half, grp, used);
                    ++elems;
                }
        }
    for (int ph = 0; ph < 2; ++ph)
        for (int p = 0; p < 16; ++p)
            for (int rb = 0; rb < 4; ++rb)
                if (cover[ph][p][rb] != 8) FAIL("reader: (patch %d, column %d) of pass %d read by %d lanes, not its 8 channel quads", p, rb, ph, cover[ph][p][rb]);
}

static void light_case(int nq) {
    const int npass = Cw4Q::SX * Cw4Q::SY * nq / 512;
    if (npass < 1 || npass * 512 != Cw4Q::SX * Cw4Q::SY * nq) FAIL("light passes");
    std::vector<int> seen((size_t)Cw4Q::SX * Cw4Q::SY * nq, 0);
    for (int tid = 0; tid < 512; ++tid) {
        int q0 = -1;
        for (int it = 0; it < npass; ++it) {
            int px, py, q4;
            cw4_light_elem(tid, it, 512, nq, px, py, q4);
            Cw4Q::light_pixel(px, py);
            if (px < 0 || px >= Cw4Q::SX || py < 0 || py >= Cw4Q::SY || q4 < 0 || q4 >= nq) { FAIL("light elem"); continue; }
            if (it == 0) q0 = q4;
            if (q4 != q0) FAIL("light quad");
            ++seen[(size_t)(py * Cw4Q::SX + px) * nq + q4];
            ++elems;
        }
    }
    for (int v : seen) if (v != 1) FAIL("light element %d times (nq=%d)", v, nq);
}

int main() {
    if (Cw4Q::NS != 8 || Cw4Q::SX * Cw4Q::NSX != 32 || Cw4Q::SY * (Cw4Q::NS / Cw4Q::NSX) != 16 || Cw4Q::ROUNDS != 4 || Cw4Q::NEL != 200 || Cw4F::NS != 4) FAIL("constants");
@MAIN@
    printf("subs %llu masks %llu walked %llu elems %llu bad %llu\n", subs, masks, walked, elems, bad);
    return bad != 0;
}
"""


def _main():
    out = []
    for H, W in ((40, 72), (64, 64), (8, 8), (1, 40), (1, 1), (17, 33), (9, 17), (16, 32)):
        for d in (0, 1, 5, 6):
            out.append("    numbering_case(2, %d, %d, %d);" % (H, W, d))
        for d in (1, 5):
            for pm in (1, 5, 30):
                out.append("    mask_case(%d, %d, %d, %d);" % (H, W, d, pm))
        out.append("    patch_case(3, %d, %d);" % (H, W))
    for nh in (0, 1, 7, 8, 9, 8 * 7 + 3, 8 * 300 + 3, 8 * 64):
        for ncb in (2, 4, 8):
            for nwg in (256, 8, 5):
                for nl in (0, 3, 700):
                    out.append("    walk_case(%d, %d, %d, %d);" % (nh, nl, ncb, nwg))
    for H, W, x0, y0 in ((40, 72, 0, 0), (40, 72, 64, 32), (40, 72, 64, 40), (64, 64, 56, 56), (64, 64, 8, 8), (5, 7, 0, 0), (1, 40, 32, 0)):
        out.append("    halo_case(%d, %d, 64, %d, %d);" % (H, W, x0, y0))
    out += ["    bank_case();", "    light_case(8);", "    light_case(16);"]
    return "\n".join(out)


def _compiler():
    for c in (shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", shutil.which("g++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no host C++ compiler")


def test_q8_subtiles_groups_slots_halo_and_banks():
    with tempfile.TemporaryDirectory() as d:
        cpp, exe = os.path.join(d, "q8.cpp"), os.path.join(d, "q8")
        open(cpp, "w").write(_SRC.replace("@MAIN@", _main()))
        flags = ["-std=c++17", "-O1", "-fsanitize=signed-integer-overflow", "-fsanitize-trap=signed-integer-overflow", "-Wno-unused-variable", "-Wno-unused-function"]
        r = subprocess.run([_compiler(), *flags, "-I", CSRC, cpp, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode >= 0, "signed overflow (trapped): " + r.stdout[-500:]
    assert r.returncode == 0, r.stdout[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert int(last[1]) > 500 and int(last[3]) > 100 and int(last[5]) > 10 ** 4 and int(last[7]) > 10 ** 3 and int(last[9]) == 0, r.stdout[-500:]


def test_q8_kernels_use_the_shared_functions():
    """The 8 x 8 kernel form and its classifier go through the functions audited above: the geometry parameter G, instantiated with Cw4Q by the 8 x 8
    entry points, and what only this form has (its LDS placement, its reader, the 16 x 8 marks from its own)."""
    rd = lambda n: open(os.path.join(CSRC, n)).read()      # noqa: E731
    k = rd("conv_winograd4.hip")
    for call in ("G::slot_index(slot, k, nht)", "cw4_halo_elem(G{}, tids + NTH * k, s, j)", "G::halo_voff(u >= 0, j, x0, y0, H, W, a.C0)", "L::patch(pty, ptx)",
                 "L::slot(s)", "cw4_reader8(wid, lanee, rb, p16q)", "G::light_pixel(px, py)", "G::in_image_total(a.B, H, W)", "G::groups(nht)",
                 "L::PLN", "L::RS", "struct W4Lds<Cw4Q> : Cw4QLds {}", "lwg_wino4_lists_go<Cw4Q>(pa, pl, stream_)"):
        assert call in k, call
    c = rd("spade_skip.hip")
    assert "GS::reached(x, y, x0, y0, d)" in c and "G::in_image(" in c and "cw4_marks16_of8(m)" in c and "sk_lists<Cw4Q>(" in c
    for own in ("struct Cw4Sub", "Cw4Sub<", "struct Cw4QLds", "#define SX", "int SX ="):
        assert own not in k and own not in c, own
    h = rd("lwg_conv_wino.h")
    assert h.count("using Cw4Q = Cw4Sub<8, 8>;") == 1 and h.count("struct Cw4QLds") == 1
