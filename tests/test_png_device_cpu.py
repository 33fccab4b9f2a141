"""The device PNG encoder (csrc/png_deflate.hip) without a GPU: the stream's definition (tests/pngdev_emu.py) decodes, the code
construction does what it says on the edge cases, and the integer rules the kernels compile (csrc/lwg_png_code.h) equal the definition.

  * emulator streams round-trip through zlib.decompress to the raw scanlines and through output.png_from_stream + PIL to the pixels:
    constant, smooth, smooth + noise, uniform noise and equal-frequency frames at ragged sizes and several segment heights;
  * a segment of zeros gives the two-symbol code (lengths 1 and 1);
  * the 17 Fibonacci literals + end of block: unlimited Huffman depth 17, limited to 15 with Kraft sum exactly 1, and it decodes;
  * uniform noise: every segment is stored and n + 5 bytes long; a frame never exceeds the capacity;
  * lwg_png_stream_capacity equals the emulator's bound; the entry points return hipErrorInvalidValue (1) / 0 on bad arguments; the new
    symbols are declared in the header and bound in _lib._SIGS;
  * csrc/lwg_png_code.h compiled for the host under AddressSanitizer + UBSan: raw bytes, histogram -> code lengths and canonical codes, sizes,
    stored bytes and the Adler-32 combination against the emulator / zlib, and the kernels call those functions."""
import io
import os
import shutil
import struct
import subprocess
import tempfile
import zlib
from fractions import Fraction

import numpy as np
import pytest

from ipercore_amd import _lib, output
from tests import pngdev_emu as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ipercore_amd", "csrc")
NEW = ("lwg_png_deflate_u8", "lwg_png_stream_capacity", "lwg_png_deflate_ws_bytes")


def _decode_png(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("H,W,rows", [(5, 5, 16), (20, 20, 8), (37, 53, 16), (33, 70, 7), (1, 1, 1), (64, 48, 64)])
@pytest.mark.parametrize("kind", emu.KINDS)
def test_emulator_streams_decode(kind, H, W, rows):
    img = emu.frame(kind, H, W, rows)
    raw = emu.paeth_filter(img)
    z = emu.stream(img, rows)
    assert z[:2] == b"\x78\x01" and len(z) <= emu.capacity(H, W, rows)
    assert zlib.decompress(z) == raw.tobytes()
    assert np.array_equal(_decode_png(output.png_from_stream(z, W, H)), img)
    assert np.array_equal(_decode_png(output.png_from_stream(np.frombuffer(z, np.uint8), W, H)), img)
    if kind == "noise" and min(rows, H) * (1 + 3 * W) > 200:
        segs = emu.segment_list(raw, rows)
        assert all(emu.is_stored(s) for s in segs)
        assert [len(s) for s in segs] == [nr * (1 + 3 * W) + 5 for _, nr in emu.segments_of(H, rows)]
        assert len(z) == emu.capacity(H, W, rows)


def test_filter_inverse():
    res = np.random.default_rng(3).integers(0, 256, (9, 3 * 11), dtype=np.uint8)
    assert np.array_equal(emu.paeth_filter(emu.paeth_unfilter(res))[:, 1:], res)


def test_zero_segment_has_the_two_symbol_code():
    raw = bytes(5000)
    lengths = emu.code_lengths(emu.segment_hist(raw))
    assert lengths[0] == 1 and lengths[256] == 1 and sum(lengths) == 2
    seg = emu.segment(raw)
    assert not emu.is_stored(seg) and len(seg) == (emu.HEADER_BITS + 5001 + 3 + 7) // 8 + 4
    assert zlib.decompress(b"\x78\x01" + seg + b"\x01\x00\x00\xff\xff" + struct.pack(">I", zlib.adler32(raw))) == raw


def test_fibonacci_histogram_forces_the_length_limit():
    res = emu.fib_residuals(sum(emu.FIB_COUNTS), 0)
    assert res.size == 6763
    hist = emu.segment_hist(res.tobytes())
    assert sorted(int(c) for c in hist if c) == sorted((1,) + emu.FIB_COUNTS)
    assert max(emu.huffman_depths(hist)) == 17
    lengths = emu.code_lengths(hist)
    assert max(lengths) == 15 and sum(Fraction(1, 2 ** l) for l in lengths if l) == 1
    assert all((l > 0) == (c > 0) for l, c in zip(lengths, hist))
    seg = emu.segment(res.tobytes())
    assert not emu.is_stored(seg)
    assert zlib.decompress(b"\x78\x01" + seg + b"\x01\x00\x00\xff\xff" + struct.pack(">I", zlib.adler32(res.tobytes()))) == res.tobytes()
    # the GPU test's frame carries the same chain, one literal longer, in its second segment
    raw = emu.paeth_filter(emu.fib_frame())
    h1 = emu.segment_hist(raw[32:].tobytes())
    assert max(emu.huffman_depths(h1)) == 18 and max(emu.code_lengths(h1)) == 15
    segs = emu.segment_list(raw, 32)
    assert emu.is_stored(segs[0]) and not emu.is_stored(segs[1])


def test_stored_rule_is_exact():
    """dyn > n + 5 -> stored, dyn == n + 5 -> dynamic: 256 equally frequent literals cost 8 bits each, so the dynamic form always loses there;
    a two-literal segment wins as soon as the header is paid for."""
    for n in (1, 100, 139, 160, 200):
        raw = bytes([1, 2] * n)[:n]
        hist = emu.segment_hist(raw)
        dyn = emu.dynamic_size(hist, emu.code_lengths(hist))
        seg = emu.segment(raw)
        assert emu.is_stored(seg) == (dyn > n + 5) and len(seg) == min(dyn, n + 5)
        assert zlib.decompress(b"\x78\x01" + seg + b"\x01\x00\x00\xff\xff" + struct.pack(">I", zlib.adler32(raw))) == raw


def test_new_symbols_are_declared_and_bound():
    hdr = _lib.header_symbols()
    for name in NEW:
        assert name in hdr and name in _lib._SIGS, name
    assert _lib.lib().lwg_abi_version() == 10


def test_capacity_is_the_emulators_bound():
    lib = _lib.lib()
    for H, W, rows in ((5, 5, 16), (20, 20, 8), (37, 53, 16), (128, 128, 16), (64, 160, 32), (512, 512, 16), (1024, 1024, 16), (1, 21844, 1), (7, 3, 100)):
        assert lib.lwg_png_stream_capacity(H, W, rows) == emu.capacity(H, W, min(rows, H)), (H, W, rows)
        assert lib.lwg_png_deflate_ws_bytes(3, H, W, rows) >= 3 * (emu.capacity(H, W, min(rows, H)) - 11)


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.lib()
    ok = dict(u8=16, B=1, H=8, W=8, rows=4, ws=16, streams=16, nbytes=16)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.lwg_png_deflate_u8(a["u8"], a["B"], a["H"], a["W"], a["rows"], a["ws"], a["streams"], a["nbytes"], None)
    for bad in (dict(u8=None), dict(ws=None), dict(streams=None), dict(nbytes=None), dict(B=0), dict(H=0), dict(W=-1), dict(rows=0), dict(B=-3),
                dict(H=64, W=1024, rows=32),        # 32 x 3 073 = 98 336 raw bytes in a segment
                dict(H=1, W=21845, rows=1),         # 65 536
                dict(ws=24)):                       # not 16-byte aligned
        assert call(**bad) == 1, bad
    for H, W, rows in ((0, 8, 4), (8, 0, 4), (8, 8, 0), (64, 1024, 32), (1, 21845, 1)):
        assert lib.lwg_png_stream_capacity(H, W, rows) == 0
        assert lib.lwg_png_deflate_ws_bytes(1, H, W, rows) == 0
    assert lib.lwg_png_deflate_ws_bytes(0, 8, 8, 4) == 0
    assert lib.lwg_png_stream_capacity(1, 21844, 1) == 65533 + 5 + 11       # the largest segment: 65 533 raw bytes


def test_frame_writer_device_encoder_has_no_cpu_fallback():
    import torch
    with tempfile.TemporaryDirectory() as d:
        with pytest.raises(ValueError):
            output.FrameWriter(d, encoder="gpu")
        w = output.FrameWriter(d, encoder="device")
        try:
            assert w.workers == output.FrameWriter.DEVICE_WORKERS
            with pytest.raises(RuntimeError):
                w.submit(torch.zeros(1, 3, 8, 8), 0)
        finally:
            assert w.close() == []
        w = output.FrameWriter(d)                       # the default is the host encoder, and it still takes CPU frames
        assert w.encoder == "host"
        w.submit(torch.zeros(2, 3, 8, 8), 0)
        assert [os.path.basename(p) for p in w.close()] == ["pred_00000000.png", "pred_00000001.png"]


def test_ops_png_deflate_raises_on_cpu_tensors():
    import torch
    from ipercore_amd import ops
    with pytest.raises(RuntimeError):
        ops.png_deflate(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))


# ---- csrc/lwg_png_code.h on the host: a serial walk through launch 1's data flow with the very functions the kernel calls
_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lwg_png_code.h"
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    int hdr[3];
    if (!f || fread(hdr, 4, 3, f) != 3) return 2;
    const int H = hdr[0], W = hdr[1], rows = hdr[2];
    std::vector<unsigned char> img((size_t)H * W * 3);
    if (fread(img.data(), 1, img.size(), f) != img.size()) return 2;
    fclose(f);
    PngGeom g;
    if (!png_geom(1, H, W, rows, g)) return 3;
    printf("geom %d %d %u %u %u %zu %u %u\n", g.rows, g.nseg, g.rowlen, g.nfull, g.slot, g.cap, png_lds_raw(g), png_out_words(g));
    unsigned A = 1, Bs = 0;
    for (int seg = 0; seg < g.nseg; ++seg) {
        const int r0 = seg * g.rows, nr = g.rows < H - r0 ? g.rows : H - r0;
        const unsigned n = (unsigned)nr * g.rowlen;
        std::vector<unsigned char> raw(n);                               // exactly n: ASan sees a read past the segment
        unsigned hist[PNG_NSYM] = {};
        unsigned long long s1 = 0, s2 = 0;
        for (unsigned i = 0; i < n; ++i) {
            const unsigned v = png_raw_byte(img.data(), g.rowlen, r0, i);
            raw[i] = (unsigned char)v;
            ++hist[v];
            s1 += v;
            s2 += (unsigned long long)(n - i) * v;
        }
        hist[256] = 1;
        unsigned m = 0;
        for (int s = 0; s < PNG_NSYM; ++s) m += hist[s] != 0;
        std::vector<unsigned> weight(2 * m - 1);                         // exactly the nodes png_code_build may touch
        std::vector<unsigned short> parent(2 * m - 1), depth(2 * m - 1), rank2(PNG_NSYM);
        for (int s = 0; s < PNG_NSYM; ++s) {
            unsigned r1 = 0, r2 = 0;
            for (int q = 0; q < PNG_NSYM; ++q) r1 += png_before_asc(hist[q], q, hist[s], s), r2 += png_before_desc(hist[q], q, hist[s], s);
            if (hist[s]) weight.at(r1) = hist[s], rank2[s] = (unsigned short)r2;
        }
        unsigned cum[16], nxt[16], lens[PNG_NSYM], payload = 0;
        png_code_build(weight.data(), parent.data(), depth.data(), m, cum, nxt);
        for (int s = 0; s < PNG_NSYM; ++s) lens[s] = hist[s] ? png_len_of_rank(cum, rank2[s]) : 0u, payload += hist[s] * lens[s];
        const unsigned dyn = png_dyn_bytes(payload);
        printf("seg %u %u %u", n, payload, dyn);
        for (int s = 0; s < PNG_NSYM; ++s) {
            unsigned idx = 0;
            for (int q = 0; q < s; ++q) idx += lens[q] == lens[s];
            printf(" %u:%u", lens[s], lens[s] ? png_rev(nxt[lens[s]] + idx, lens[s]) : 0u);
        }
        printf("\nraw");
        for (unsigned i = 0; i < n; ++i) printf(" %u", raw[i]);
        printf("\nstored");
        for (unsigned k = 0; k < ((n + 5u + 3u) / 4u) * 4u; ++k) printf(" %u", png_stored_byte(raw.data(), n, k));
        printf("\n");
        png_adler_step(A, Bs, n, (unsigned)(s1 % PNG_ADLER), (unsigned)(s2 % PNG_ADLER));
    }
    printf("adler %u\n", (Bs << 16) | A);
    return 0;
}
"""


def _compiler():
    for c in (shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", shutil.which("g++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no host C++ compiler")


@pytest.fixture(scope="module")
def host_program():
    d = tempfile.mkdtemp(prefix="lwg_pngcode_")
    cpp, exe = os.path.join(d, "pngcode.cpp"), os.path.join(d, "pngcode")
    with open(cpp, "w") as fp:
        fp.write(_SRC)
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([_compiler(), *flags, "-I", CSRC, cpp, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    yield exe
    shutil.rmtree(d, ignore_errors=True)


def _host_case(exe, img, rows):
    H, W, _ = img.shape
    with tempfile.NamedTemporaryFile(suffix=".bin") as fp:
        fp.write(struct.pack("<iii", H, W, rows) + img.tobytes())
        fp.flush()
        r = subprocess.run([exe, fp.name], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    raw = emu.paeth_filter(img)
    geom = [int(v) for v in lines[0].split()[1:]]
    assert geom[0] == min(rows, H) and geom[1] == len(emu.segments_of(H, rows)) and geom[2] == 1 + 3 * W and geom[3] == min(rows, H) * (1 + 3 * W)
    assert geom[4] % 16 == 0 and geom[4] >= geom[3] + 5 + 16 and geom[5] == emu.capacity(H, W, rows)
    assert geom[6] % 16 == 0 and geom[6] >= geom[3] and 4 * geom[7] >= geom[3] + 5 + 8
    for k, (r0, nr) in enumerate(emu.segments_of(H, rows)):
        seg, rawl, stl = (lines[1 + 3 * k + j].split() for j in range(3))
        want = raw[r0:r0 + nr].tobytes()
        hist = emu.segment_hist(want)
        lengths = emu.code_lengths(hist)
        codes = emu.canonical_codes(lengths)
        assert [int(v) for v in seg[1:4]] == [len(want), sum(int(h) * l for h, l in zip(hist, lengths)), emu.dynamic_size(hist, lengths)]
        assert seg[4:] == ["%d:%d" % (l, c) for l, c in zip(lengths, codes)]
        assert bytes(int(v) for v in rawl[1:]) == want
        st = bytes(int(v) for v in stl[1:])
        assert st[:len(want) + 5] == emu.segment_stored(want) and not any(st[len(want) + 5:])
    assert int(lines[-1].split()[1]) == zlib.adler32(raw.tobytes()) & 0xFFFFFFFF


@pytest.mark.parametrize("kind", emu.KINDS)
def test_kernel_rules_on_the_host_equal_the_emulator(host_program, kind):
    for H, W, rows in ((5, 5, 16), (20, 20, 8), (37, 53, 16)):
        _host_case(host_program, emu.frame(kind, H, W, rows), rows)


def test_kernel_rules_on_the_host_length_limit_and_largest_segment(host_program):
    _host_case(host_program, emu.fib_frame(), 32)
    img = np.random.default_rng(5).integers(0, 256, (2, 21844, 3), dtype=np.uint8)        # two segments of 65 533 bytes: the Adler sums at their largest
    img[1] = 255
    _host_case(host_program, img, 1)


def test_kernels_call_the_shared_rules():
    k = open(os.path.join(CSRC, "png_deflate.hip")).read()
    for call in ("png_raw_byte(img, g.rowlen, r0, i)", "png_before_asc(cq, q, c, s)", "png_before_desc(cq, q, c, s)",
                 "png_code_build(t.weight, t.parent, t.depth, t.m, t.cum, t.nxt)", "png_len_of_rank(t.cum, t.rank2[s])", "png_rev(t.nxt[l] + idx, l)",
                 "png_dyn_bytes(payload)", "png_stored_byte(raw, n, 4u * w + h)", "png_adler_step(A, Bs, mt.n, mt.s1, mt.s2)", "png_geom(B, H, W, rows_per_segment, g)",
                 "png_lds_raw(g)", "png_out_words(g)"):
        assert call in k, call
    for own in ("PNG_FN", "struct PngGeom", "bool png_geom"):
        assert own not in k, own
