"""The fused source | reference | output video without a GPU: tests/fusecanvas_emu.py - the definition of the panel and the
canvas - against the reference's own concatenations (tests/golden/golden_fuse_video_v1.npz), the 8-bit round trip of the source pixels,
csrc/lwg_fuse_geom.h walked byte by byte on the host under overflow traps, the argument checks of the C entry points (the library loads
without a GPU) and the host code around them (output.FuseSpec / RefFrames / FrameWriter(fuse=...), the AVI of emulator-coded canvases).

Grid of the header audit (the GPU tests' canvas grid): S in (4, 8, 20, 36) x ns in (1, 2, 8) x pad in (0, 1, 2, 3, 10) x reference yes / no x
n_out in (1, 2, 4); the panel cells for ns = 1 .. 9 at S in (4, 8, 20, 64)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from ipercore_amd import _lib, output
from tests import fusecanvas_emu as emu
from tests import jpegdev_emu
from tests.test_conv_offsets_cpu import CSRC, _compiler
from tests.test_jpeg_device_cpu import decode, riff_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lwg_fuse_sources_u8", "lwg_fuse_canvas_u8", "lwg_fuse_panel_width", "lwg_fuse_canvas_width")
CANVAS_S, CANVAS_NS, PADS, N_OUTS = (4, 8, 20, 36), (1, 2, 8), (0, 1, 2, 3, 10), (1, 2, 4)
PANEL_S = (4, 8, 20, 64)


def panel_ok(ns, S):
    return ns == 1 or (ns <= 7 and S % 2 == 0) or (ns >= 8 and S % 4 == 0)


def canvas_cases():
    return [(S, ns, pad, ref, n_out) for S in CANVAS_S for ns in CANVAS_NS for pad in PADS for ref in (1, 0) for n_out in N_OUTS]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "golden_fuse_video_v1.npz")))


def as_source(u8_hwc):
    """imitator.load_images' arithmetic on 8-bit RGB images (n,S,S,3) -> (n,3,S,S) fp32 in [-1, 1]."""
    a = np.asarray(u8_hwc, dtype=np.float32) / 255.0
    return np.ascontiguousarray((a * 2 - 1).transpose(0, 3, 1, 2))


# ---- the definition against the reference's concatenations ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", range(1, 10))
def test_panel_equals_the_references_fuse_source(golden, ns):
    want = golden["panel_ns%d" % ns][:, :, ::-1]                      # BGR -> RGB
    got = emu.panel(as_source(golden["src"][:ns]))
    assert got.shape == want.shape and np.array_equal(got, want)
    if ns == 9:
        assert np.array_equal(got, emu.panel(as_source(golden["src"][:8])))


@pytest.mark.parametrize("ns", (1, 2, 8))
@pytest.mark.parametrize("pad,pad_val", ((10, 0), (3, 255)))
def test_canvas_equals_the_references_merges(golden, ns, pad, pad_val):
    pan = emu.panel(as_source(golden["src"][:ns]))
    ref, outs = golden["ref"][None], [golden["outs"][k][None] for k in range(3)]
    tag = "_ns%d_pad%d" % (ns, pad)
    for name, r, o in (("row_merge", ref, outs[:1]), ("row_src_out", None, outs[:1]), ("row_multi", ref, outs)):
        want = golden[name + tag][:, :, ::-1]
        got = emu.canvas(pan, r, o, pad, pad_val)
        assert got.shape == (1,) + want.shape and np.array_equal(got[0], want), name + tag
        assert got.shape[2] == emu.canvas_width(pan.shape[1], 16, pad, r is not None, len(o))


def test_every_8_bit_level_survives_rint_and_not_truncation():
    levels = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, axis=3)
    x = as_source(levels)
    assert np.array_equal(emu.src_u8(x).transpose(0, 2, 3, 1), levels)
    lost = int((emu.frames_u8(x) != levels).any(axis=(0, 3)).sum())
    assert lost == 63, lost                                           # what lwg_frames_to_u8's truncation would do to a source image
    odd = np.array([np.nan, -1.5, 1.5, np.inf, -np.inf, 0.5 / 127.5 - 1, 1.5 / 127.5 - 1, 2.5 / 127.5 - 1], dtype=np.float32)
    assert emu.src_u8(odd).tolist()[:5] == [0, 0, 255, 255, 0]


def test_layout_refuses_what_the_rules_refuse():
    for ns, S in ((0, 8), (2, 5), (7, 9), (8, 6), (9, 10), (1, 0)):
        with pytest.raises(ValueError):
            emu.layout(ns, S)
    assert emu.layout(7, 8) == emu.layout(4, 8) and emu.layout(3, 8)[1][3][0] == -1
    assert [c[0] for c in emu.layout(12, 8)[1]] == [0, 1, 4, 5]


# ---- the library without a GPU ----------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    hdr = _lib.header_symbols()
    for name in NEW:
        assert name in hdr and name in _lib._SIGS, name
    assert set(_lib._SIGS) == set(hdr)
    assert _lib.lib().lwg_abi_version() == 10
    assert "#define LWG_ABI_VERSION 10" in open(_lib.HEADER_PATH).read()


def test_helper_widths_are_the_emulators():
    lib = _lib.lib()
    for S in sorted(set(CANVAS_S + PANEL_S + (5, 6, 512))):
        for ns in range(1, 10):
            if not panel_ok(ns, S):
                assert lib.lwg_fuse_panel_width(ns, S) == 0 and lib.lwg_fuse_canvas_width(ns, S, 10, 1, 1) == 0
                continue
            Wp = emu.layout(ns, S)[0]
            assert lib.lwg_fuse_panel_width(ns, S) == Wp
            for pad in PADS:
                for ref in (0, 1):
                    for n_out in N_OUTS:
                        assert lib.lwg_fuse_canvas_width(ns, S, pad, ref, n_out) == emu.canvas_width(Wp, S, pad, ref, n_out)
    assert lib.lwg_fuse_canvas_width(1, 512, 10, 1, 1) == 1556
    for bad in ((0, 8, 10, 1, 1), (-1, 8, 10, 1, 1), (1, 0, 10, 1, 1), (1, 8, -1, 1, 1), (1, 8, 10, 1, 0), (1, 8, 10, 1, 5),
                (1, 13378, 0, 0, 1),       # 12 S^2 = 2 147 650 608 bytes: an fp32 frame beyond int32
                (1, 12000, 0, 0, 4),       # 3 S Wc = 2 160 000 000 bytes: a canvas frame beyond int32
                (2, 8, 30000, 1, 4)):      # a row of 450 492 bytes: more than a workgroup holds
        assert lib.lwg_fuse_canvas_width(*bad) == 0, bad
    assert lib.lwg_fuse_panel_width(1, 13378) == 0 and lib.lwg_fuse_panel_width(0, 8) == 0 and lib.lwg_fuse_panel_width(1, -4) == 0


def test_bad_arguments_are_refused_before_any_launch():
    import ctypes
    lib = _lib.lib()
    ok = dict(panel=16, Wp=8, ref=16, outs=(16,), n_out=1, B=1, S=8, pad=10, pad_val=0, canvas=16)

    def call(**kw):
        a = dict(ok, **kw)
        outs = None if a["outs"] is None else (ctypes.c_void_p * max(len(a["outs"]), 1))(*a["outs"])
        return lib.lwg_fuse_canvas_u8(a["panel"], a["Wp"], a["ref"], outs, a["n_out"], a["B"], a["S"], a["pad"], a["pad_val"], a["canvas"], None)
    for bad in (dict(panel=None), dict(outs=None), dict(canvas=None), dict(outs=(None,)), dict(outs=(16, None), n_out=2),
                dict(panel=18), dict(ref=17), dict(canvas=19), dict(outs=(18,)),            # not 4-byte aligned
                dict(B=0), dict(B=-1), dict(S=0), dict(S=-8), dict(n_out=0), dict(n_out=5), dict(pad=-1), dict(pad_val=-1), dict(pad_val=256),
                dict(Wp=3), dict(Wp=0), dict(Wp=16), dict(S=6, Wp=2),                       # no panel width of S
                dict(S=13378, Wp=13378, pad=0, ref=None, outs=(16,) * 4, n_out=4),          # frames of 2^31 bytes and more
                dict(pad=30000)):                                                           # a row no workgroup holds
        assert call(**bad) == 1, bad
    for bad in ((None, 1, 8, 16), (16, 1, 8, None), (18, 1, 8, 16), (16, 1, 8, 18), (16, 0, 8, 16), (16, 2, 7, 16), (16, 8, 10, 16), (16, 1, 0, 16),
                (16, 1, 13378, 16)):
        assert lib.lwg_fuse_sources_u8(bad[0], bad[1], bad[2], bad[3], None) == 1, bad


def test_frame_writer_fuse_has_no_cpu_fallback():
    import torch
    from ipercore_amd import ops
    panel = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with tempfile.TemporaryDirectory() as d:
        for enc in ("host", "device", "jpeg", "mjpeg"):
            w = output.FrameWriter(d, encoder=enc, fuse=output.FuseSpec(panel, with_ref=False), video_name="fused.avi")
            try:
                with pytest.raises(RuntimeError):
                    w.submit(torch.zeros(1, 3, 8, 8), 0)
            finally:
                assert w.close() == []
        with pytest.raises(TypeError):
            output.FrameWriter(d, fuse=panel)
        w = output.FrameWriter(d)                                     # without fuse the writer is what it was: CPU frames are taken ...
        try:
            with pytest.raises(ValueError):                           # ... and there is nothing to put a reference into
                w.submit(_FakeDevice(), 0, ref=np.zeros((1, 8, 8, 3), np.uint8))
        finally:
            w.close()
    for bad in (dict(pad=-1), dict(pad_val=256), dict(pad_val=-1)):
        with pytest.raises(ValueError):
            output.FuseSpec(panel, **bad)
    with pytest.raises(RuntimeError):
        ops.fuse_source_panel(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError):
        ops.fuse_canvas(panel, None, torch.zeros(1, 3, 8, 8))


class _FakeDevice(object):
    """A frame batch that says it is on the device and is never looked at further: FrameWriter.submit refuses ``ref`` before any launch."""
    is_cuda, shape = True, (1, 3, 8, 8)

    def contiguous(self):
        return self


def test_ref_frames_feed():
    from PIL import Image
    import torch
    r = np.random.RandomState(3)
    frames = r.randint(0, 256, size=(5, 8, 8, 3)).astype(np.uint8)
    batches = [(0, 2), (2, 2), (4, 1)]
    for kind in ("array", "tensor"):
        src = frames if kind == "array" else torch.from_numpy(frames)
        feed = output.RefFrames(src, 5, 8, batches)
        for k, (s, n) in enumerate(batches):
            assert np.array_equal(np.asarray(feed.get(k)), frames[s:s + n])
            feed.done(k)
        feed.close()
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for t in range(5):
            paths.append(os.path.join(d, "ref_%d.png" % t))
            Image.fromarray(frames[t], mode="RGB").save(paths[t])
        big = os.path.join(d, "big.png")                              # not S x S: resized as load_images resizes
        Image.fromarray(np.kron(frames[4], np.ones((2, 2, 1), np.uint8)), mode="RGB").save(big)
        feed = output.RefFrames(paths[:4] + [big], 5, 8, batches)
        try:
            for k, (s, n) in enumerate(batches):
                got = np.asarray(feed.get(k)).copy()
                if k < 2:
                    assert np.array_equal(got, frames[s:s + n])
                else:
                    want = np.asarray(Image.open(big).convert("RGB").resize((8, 8), Image.BILINEAR))
                    assert got.shape == (1, 8, 8, 3) and np.array_equal(got[0], want)
                feed.done(k)
        finally:
            feed.close()
        with pytest.raises(ValueError):
            output.RefFrames(paths, 6, 8, batches)                    # the reference asserts the same
    with pytest.raises(ValueError):
        output.RefFrames(frames, 4, 8, batches)
    with pytest.raises(ValueError):
        output.RefFrames(frames.astype(np.float32), 5, 8, batches)
    with pytest.raises(ValueError):
        output.RefFrames(frames, 5, 16, batches)


# ---- the container around emulator-coded canvases ---------------------------------------------------------------------------------------------
def test_avi_of_emulator_coded_canvases(golden):
    pan = emu.panel(as_source(golden["src"][:2]))
    refs = np.stack([golden["ref"], golden["ref"][::-1]])
    outs = [np.stack([golden["outs"][0], golden["outs"][1]])]
    can = emu.canvas(pan, refs, outs, 10, 0)
    B, S, Wc, _ = can.shape
    assert (S, Wc) == (16, 8 + 2 * 26)
    ri = min((Wc + 7) // 8, 64)
    files = [jpegdev_emu.file(can[t], 90, ri) for t in range(B)]
    with tempfile.TemporaryDirectory() as d:
        w = output.MjpegAviWriter(os.path.join(d, "pred_fused.avi"), Wc, S, fps=25)
        for t in (1, 0):
            w.add(t, files[t])
        path, = w.close()
        with open(path, "rb") as fp:
            info = riff_frames(fp.read())
    assert info["frames"] == files and (info["width"], info["height"], info["total"]) == (Wc, S, B)
    for t in range(B):
        assert decode(info["frames"][t], Wc, S).shape == (S, Wc, 3)


# ---- csrc/lwg_fuse_geom.h on the host ---------------------------------------------------------------------------------------------------------
_PROGRAM = r"""
#include "lwg_fuse_geom.h"
#include <cstdio>
// in:  int32 npanel, per panel case {ns, S}; int32 ncanvas, per canvas case {S, ns, pad, has_ref, n_out}
// out: per panel case int32 {Wp, ncells, 4 x {src, top, left, size}}, then per panel pixel of a valid case the number of cells that hold it;
//      per canvas case int32 {ok, Wc, row3}, then per byte of a row {region, off}
int main(int argc, char** argv) {
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    int n = 0;
    if (!in || !out || fread(&n, 4, 1, in) != 1) return 2;
    for (int c = 0; c < n; ++c) {
        int hd[2];
        if (fread(hd, 4, 2, in) != 2) return 2;
        LwgFuseCell cells[LWG_FUSE_MAX_CELLS] = {};
        int rec[2 + 4 * LWG_FUSE_MAX_CELLS] = {0};
        const int Wp = lwg_fuse_panel_cells(hd[0], hd[1], cells, rec[1]);
        rec[0] = Wp;
        for (int k = 0; k < rec[1]; ++k) { rec[2 + 4 * k] = cells[k].src; rec[3 + 4 * k] = cells[k].top; rec[4 + 4 * k] = cells[k].left; rec[5 + 4 * k] = cells[k].size; }
        fwrite(rec, 4, 2 + 4 * LWG_FUSE_MAX_CELLS, out);
        for (int y = 0; Wp > 0 && y < hd[1]; ++y)
            for (int x = 0; x < Wp; ++x) {
                int hits = 0;
                for (int k = 0; k < rec[1]; ++k)
                    hits += y >= cells[k].top && y < cells[k].top + cells[k].size && x >= cells[k].left && x < cells[k].left + cells[k].size;
                fwrite(&hits, 4, 1, out);
            }
    }
    if (fread(&n, 4, 1, in) != 1) return 2;
    for (int c = 0; c < n; ++c) {
        int hd[5];
        if (fread(hd, 4, 5, in) != 5) return 2;
        LwgFuseCell cells[LWG_FUSE_MAX_CELLS] = {};
        int ncells = 0;
        const int Wp = lwg_fuse_panel_cells(hd[1], hd[0], cells, ncells);
        LwgFuseGeom g = {};
        int rec[3] = {0, 0, 0};
        rec[0] = Wp > 0 && lwg_fuse_geom_of(hd[0], Wp, hd[2], hd[3], hd[4], g);
        rec[1] = g.Wc; rec[2] = g.row3;
        fwrite(rec, 4, 3, out);
        for (int xb = 0; rec[0] && xb < g.row3; ++xb) {
            int ro[2];
            lwg_fuse_locate(g, xb, ro[0], ro[1]);
            fwrite(ro, 4, 2, out);
        }
    }
    // the taps of the three factors
    for (int f = 1; f <= 4; f *= 2)
        for (int i = 0; i < 5; ++i) {
            int t[2];
            t[0] = lwg_fuse_tap0(i, f, t[1]);
            fwrite(t, 4, 2, out);
        }
    // sizes at the edge of the contract: the width arithmetic must not overflow on the way to refusing them
    const int edge[6][5] = {{13377, 13377, 0, 0, 1}, {13378, 13378, 0, 0, 4}, {2147483647, 2147483647, 2147483647, 1, 4}, {4, 4, 2147483647, 1, 4},
                            {8192, 2048, 10, 1, 4}, {13376, 3344, 0, 0, 1}};
    for (int e = 0; e < 6; ++e) {
        LwgFuseGeom g = {};
        const int ok = lwg_fuse_geom_of(edge[e][0], edge[e][1], edge[e][2], edge[e][3], edge[e][4], g);
        fwrite(&ok, 4, 1, out);
    }
    fclose(out);
    return 0;
}
"""


def test_header_walk_equals_the_emulator_on_every_canvas_byte():
    """The program ends without a trap (no index expression of lwg_fuse_geom.h overflows), the cells are the emulator's and tile the panel
    exactly once, and every byte of every canvas row of the grid has the emulator's (region, offset) - hence exactly one source."""
    panels = [(ns, S) for S in PANEL_S + (5, 6) for ns in range(0, 10)]
    cases = canvas_cases()
    with tempfile.TemporaryDirectory() as d:
        cpp, exe, fin, fout = (os.path.join(d, n) for n in ("audit.cpp", "audit", "in.bin", "out.bin"))
        open(cpp, "w").write(_PROGRAM)
        with open(fin, "wb") as fp:
            fp.write(np.int32(len(panels)).tobytes() + np.array(panels, dtype=np.int32).tobytes())
            fp.write(np.int32(len(cases)).tobytes() + np.array(cases, dtype=np.int32).tobytes())
        checks = "signed-integer-overflow"
        flags = ["-std=c++17", "-O1", "-fsanitize=" + checks, "-fsanitize-trap=" + checks]
        r = subprocess.run([_compiler(), *flags, "-I", CSRC, cpp, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
        assert r.returncode >= 0, "an index expression of lwg_fuse_geom.h overflowed (trapped)"
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:])
        words = np.fromfile(fout, dtype=np.int32)
    pos = 0
    for ns, S in panels:
        rec = words[pos:pos + 18]
        pos += 18
        if ns < 1 or not panel_ok(ns, S):
            assert rec[0] == 0, (ns, S)
            continue
        Wp, cells = emu.layout(ns, S)
        assert rec[0] == Wp and rec[1] == len(cells) and [tuple(rec[2 + 4 * k:6 + 4 * k]) for k in range(len(cells))] == cells, (ns, S)
        assert (words[pos:pos + S * Wp] == 1).all(), (ns, S)
        pos += S * Wp
    seen_ragged = False
    for S, ns, pad, ref, n_out in cases:
        ok, Wc, row3 = words[pos:pos + 3]
        pos += 3
        if not panel_ok(ns, S):
            assert ok == 0
            continue
        Wp = emu.layout(ns, S)[0]
        region, off = emu.row_map(Wp, S, pad, ref, n_out)
        assert ok == 1 and Wc == emu.canvas_width(Wp, S, pad, ref, n_out) and row3 == 3 * Wc == region.size
        got = words[pos:pos + 2 * row3].reshape(row3, 2)
        pos += 2 * row3
        assert np.array_equal(got[:, 0], region) and np.array_equal(got[:, 1], off), (S, ns, pad, ref, n_out)
        # exactly one source per byte: within a region the offsets are 0 .. n - 1, each once
        for rg in np.unique(region):
            o = off[region == rg]
            n = {emu.PANEL: 3 * Wp, emu.PAD: 3 * pad}.get(int(rg), 3 * S)
            counts = np.bincount(o, minlength=n)
            assert o.max() < n and (counts == (ref + n_out if rg == emu.PAD else 1)).all()
        seen_ragged = seen_ragged or row3 % 4 != 0
    assert seen_ragged and 3 * emu.canvas_width(4, 4, 1, 0, 1) == 27
    taps = words[pos:pos + 30].reshape(3, 5, 2)
    pos += 30
    assert taps[0].tolist() == [[i, 0] for i in range(5)] and taps[1].tolist() == [[2 * i, 1] for i in range(5)] \
        and taps[2].tolist() == [[4 * i + 1, 1] for i in range(5)]
    assert words[pos:pos + 6].tolist() == [1, 0, 0, 0, 1, 1] and pos + 6 == words.size
