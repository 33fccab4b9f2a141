"""CPU checks of the integer arithmetic behind the list-driven F(4x4, 3x3) convolution (csrc/lwg_conv_wino.h part 1: cw_block_window, cw_list_entry,
cw_list_first_light, cw4_light_elem) - the very functions the kernels compile, built into a host program with signed-overflow traps as
tests/test_conv_offsets_cpu.py does.

  * a block's window (the block grown by d pixels, clipped to the image) against its definition pixel by pixel, at the image's corners and on sizes that
    are no multiple of the block;
  * the walk of every workgroup of a persistent grid over the heavy and the light entries: every (tile, column block) exactly once - heavy tiles in the
    K-loop phase, light tiles in the streaming phase -, for an empty heavy list, an empty light list and mixed ones, grids larger and smaller than the
    lists;
  * a light block's elements: every (pixel, channel quad) of the 32 x 16 block exactly once, a thread keeping its quad through the passes."""
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
static u64 bad = 0, windows = 0, walked = 0, elems = 0;

static void window_case(int H, int W, int d) {
    const CwGrid g = cw_grid(1, H, W, 64, 32, 16, 64);
    for (int t = 0; t < g.tiles; ++t) {
        int x0, y0;
        cw_corner(g, t, 32, 16, x0, y0);
        const CwWindow w = cw_block_window(x0, y0, 32, 16, d, H, W);
        u64 fails = 0;
        for (int y = -d - 1; y <= H + d; ++y)
            for (int x = -d - 1; x <= W + d; ++x) {
                const bool want = x >= 0 && x < W && y >= 0 && y < H && x >= x0 - d && x < x0 + 32 + d && y >= y0 - d && y < y0 + 16 + d;
                const bool got = x >= w.x0 && x < w.x1 && y >= w.y0 && y < w.y1;
                fails += want != got;
            }
        if (w.x0 < 0 || w.y0 < 0 || w.x1 > W || w.y1 > H || w.x0 >= w.x1 || w.y0 >= w.y1) ++fails;      // never empty: a block's corner is inside the image
        if (fails && bad++ < 8) printf("BAD window H=%d W=%d d=%d tile %d: [%d, %d) x [%d, %d)\n", H, W, d, t, w.x0, w.x1, w.y0, w.y1);
        bad += fails ? fails - 1 : 0;
        ++windows;
    }
}

// tiles tiles of which every tile with (t * 7 + 3) % mod < cut is heavy (mod = 0: none; cut >= mod: all); ncb column blocks; nwg workgroups
static void walk_case(int tiles, int ncb, int nwg_in, int mod, int cut) {
    std::vector<int> heavy, light;
    for (int t = 0; t < tiles; ++t) (mod && (t * 7 + 3) % mod < cut ? heavy : light).push_back(t);
    const int nhe = (int)heavy.size() * ncb, nle = (int)light.size() * ncb, total = tiles * ncb;
    const int nwg = nwg_in < total ? nwg_in : total;                        // (the launch: min(blocks, CUs) workgroups)
    std::vector<int> seen((size_t)total, 0);
    u64 fails = 0;
    for (int wg = 0; wg < nwg; ++wg) {
        int id = wg, last = -1;
        for (; id < nhe; id += nwg) {                                       // the K-loop phase
            int slot, cb;
            cw_list_entry(id, ncb, slot, cb);
            if (slot < 0 || slot >= (int)heavy.size() || cb < 0 || cb >= ncb) { ++fails; continue; }
            if (heavy[slot] < last) ++fails;                                // ascending tiles per workgroup
            last = heavy[slot];
            seen[(size_t)heavy[slot] * ncb + cb] += 1;
            ++walked;
        }
        if (cw_list_first_light(wg, nwg, nhe) != id) ++fails;               // the streaming phase starts at the workgroup's first id behind the heavy ones
        for (id = cw_list_first_light(wg, nwg, nhe); id < nhe + nle; id += nwg) {
            int slot, cb;
            cw_list_entry(id - nhe, ncb, slot, cb);
            if (slot < 0 || slot >= (int)light.size() || cb < 0 || cb >= ncb) { ++fails; continue; }
            seen[(size_t)light[slot] * ncb + cb] += 16;
            ++walked;
        }
    }
    for (int t = 0; t < tiles; ++t)
        for (int cb = 0; cb < ncb; ++cb) {
            const bool hv = mod && (t * 7 + 3) % mod < cut;
            if (seen[(size_t)t * ncb + cb] != (hv ? 1 : 16)) ++fails;
        }
    if (fails) { bad += fails; printf("BAD walk tiles=%d ncb=%d nwg=%d mod=%d cut=%d: %llu\n", tiles, ncb, nwg, mod, cut, fails); }
}

static void light_case(int nq) {
    std::vector<int> seen((size_t)512 * nq, 0);
    u64 fails = 0;
    for (int tid = 0; tid < 512; ++tid) {
        int q0 = -1;
        for (int it = 0; it < nq; ++it) {
            int px, py, q4;
            cw4_light_elem(tid, it, 512, nq, px, py, q4);
            if (px < 0 || px >= 32 || py < 0 || py >= 16 || q4 < 0 || q4 >= nq) { ++fails; continue; }
            if (it == 0) q0 = q4;
            if (q4 != q0) ++fails;
            ++seen[(size_t)(py * 32 + px) * nq + q4];
            ++elems;
        }
    }
    for (int v : seen) fails += v != 1;
    if (fails) { bad += fails; printf("BAD light elements nq=%d: %llu\n", nq, fails); }
}

int main() {
@MAIN@
    printf("windows %llu walked %llu elems %llu bad %llu\n", windows, walked, elems, bad);
    return bad != 0;
}
"""


def _main():
    out = []
    for H, W in ((16, 32), (1, 1), (17, 33), (40, 72), (64, 64), (15, 31), (128, 128), (5, 200), (200, 5)):
        for d in (0, 1, 2, 5, 6, 40):
            out.append("    window_case(%d, %d, %d);" % (H, W, d))
    # (tiles, ncb, workgroups): the generator's SPADE launches at a 300-frame batch (256^2: 128 tiles per frame, 2 / 4 column blocks) cut down to 20
    # frames, the GPU test's launches, ragged ones; heavy pattern (mod, cut): none, all, a few, most, alternating
    for tiles, ncb, nwg in ((2560, 2, 256), (640, 4, 256), (160, 8, 256), (160, 2, 256), (36, 2, 256), (36, 4, 256), (7, 3, 5), (1, 1, 8), (33, 8, 24), (300, 1, 256)):
        for mod, cut in ((0, 0), (1, 1), (13, 1), (13, 12), (2, 1), (5, 2)):
            out.append("    walk_case(%d, %d, %d, %d, %d);" % (tiles, ncb, nwg, mod, cut))
    out += ["    light_case(8);", "    light_case(16);"]
    return "\n".join(out)


def _compiler():
    for c in (shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", shutil.which("g++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no host C++ compiler")


def test_windows_list_walk_and_light_elements():
    with tempfile.TemporaryDirectory() as d:
        cpp, exe = os.path.join(d, "skip.cpp"), os.path.join(d, "skip")
        open(cpp, "w").write(_SRC.replace("@MAIN@", _main()))
        flags = ["-std=c++17", "-O1", "-fsanitize=signed-integer-overflow", "-fsanitize-trap=signed-integer-overflow", "-Wno-unused-variable", "-Wno-unused-function"]
        r = subprocess.run([_compiler(), *flags, "-I", CSRC, cpp, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode >= 0, "signed overflow (trapped): " + r.stdout[-500:]
    assert r.returncode == 0, r.stdout[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert int(last[1]) > 400 and int(last[3]) > 10 ** 4 and int(last[5]) == 512 * 24 and int(last[7]) == 0, r.stdout[-500:]


def test_kernels_use_the_shared_functions():
    """The list-driven kernel and the classifier go through the functions audited above, and both the attention kernel and the classifier take the
    in-image predicate from ONE header."""
    rd = lambda n: open(os.path.join(CSRC, n)).read()      # noqa: E731
    k = rd("conv_winograd4.hip")
    for call in ("cw_list_entry(id, N / NBV, slot, cb)", "cw_list_entry(id - nhe, ncb, slot, cb)", "cw_list_first_light((int)blockIdx.x, (int)gridDim.x, nhe)",
                 "cw4_light_elem(tid, it + i, W4_THREADS, NQD, px, py, q4)", "w4_spade_mod(", "w4_act16(a.act, o)"):
        assert call in k, call
    assert k.count("w4_spade_mod(") == 3 and k.count("w4_act16(a.act, o)") == 2        # the definition; the epilogue and the light loop
    c = rd("spade_skip.hip")
    assert "cw_block_window(x0, y0, SK_EX, SK_EY, d, h, w)" in c and "lwb_tap_in_image(tx0, ty0, w, h)" in c and "lwb_taps_of(" in c
    assert "atomic" not in c
    a = rd("lwb_attn_x.hip")
    assert a.count("lwb_tap_in_image(tx0, ty0, w, h)") == 2 and "lwb_taps_of(t, w, h, wt, tx0, ty0)" in a and "tx0 >= -1" not in a
