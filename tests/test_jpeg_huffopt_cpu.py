"""The device JPEG encoder's per-frame Huffman tables without a GPU: tests/jpeghuff_emu.py - the definition - on adversarial
histograms against a second restatement of the rule that builds the tree explicitly, its files against a real decoder and against the
fixed-table files of the same frames, the host code around the scan (output.jpeg_headers / jpeg_from_scan / FrameWriter / Imitator's option)
and the argument checks of the new C entry points (the library loads without a GPU).

Grids: those of tests/test_jpeg_device_cpu.py (4:4:4) and tests/test_jpeg420_cpu.py (4:2:0) - their sizes, qualities, the five contents and
their restart intervals.

Measured with this file at quality 90, one MCU row per segment, 128 x 128, 4:4:4 (scan bytes fixed -> saved): noise 30 628 -> 3 697,
smooth_noise 4 181 -> 451, smooth 2 382 -> 594, checker 9 006 -> 5 152, constant 542 -> 272; the four DHT segments shrink from 432 bytes to
91 .. 151.  No grid point of either format gives a larger file than the fixed tables."""
import tempfile

import numpy as np
import pytest

from ipercore_amd import _lib, output
from tests import jpeg420_emu as emu420
from tests import jpegdev_emu as emu444
from tests import jpeghuff_emu as emu
from tests import test_jpeg420_cpu as grid420
from tests import test_jpeg_device_cpu as grid444
from tests.test_jpeg_device_cpu import decode

GRIDS = {"444": grid444, "420": grid420}
FIXED = {"444": emu444, "420": emu420}
NEW = ("lwg_jpeg_scan_opt_u8", "lwg_jpeg_scan_opt_capacity", "lwg_jpeg_scan_opt_ws_bytes", "lwg_jpeg420_scan_opt_u8", "lwg_jpeg420_scan_opt_capacity",
       "lwg_jpeg420_scan_opt_ws_bytes", "lwg_jpeg_hist_u8", "lwg_jpeg420_hist_u8", "lwg_jpeg_huff_tables")


def _padded(counts):
    return list(counts) + [0] * (256 - len(counts))


def adversarial_histograms():
    """name -> 256 counts: the inputs of the table checks, here and on the GPU."""
    fib = [1, 1]
    while len(fib) < 42:
        fib.append(fib[-1] + fib[-2])
    h = {
        "empty": [0] * 256,
        "one symbol": _padded([0, 0, 0, 7]),
        "one symbol, the last": [0] * 255 + [1],
        "two symbols": _padded([5, 0, 0, 0, 0, 0, 0, 0, 0, 9]),
        "two equal symbols": _padded([3, 3]),
        "256 equal": [5] * 256,
        "256 ones": [1] * 256,
        "powers of two": _padded([1] + [1 << i for i in range(29)]),
        "powers of two, descending": _padded([1 << i for i in range(28, -1, -1)] + [1]),
        "fibonacci": _padded(fib),
        "fibonacci, scattered": [0] * 256,
        "all 2^32 - 1": [0xFFFFFFFF] * 256,
        "some 2^32 - 1": _padded([0xFFFFFFFF, 1, 0xFFFFFFFF, 2, 0xFFFFFFFE, 0xFFFFFFFF]),
    }
    for k, v in enumerate(fib):
        h["fibonacci, scattered"][(k * 37 + 11) % 256] = v
    h["fibonacci from 1, 2"] = _padded(fib[1:] + [fib[-1] + fib[-2], fib[-1] * 2 + fib[-2]])      # a chain: lengths above libjpeg's cap of 32
    for seed in range(6):
        rng = np.random.default_rng(seed)
        c = np.zeros(256, np.int64)
        at = rng.choice(256, int(rng.integers(3, 200)), replace=False)
        c[at] = rng.integers(1, 4, at.size)                # many ties
        h["sparse %d" % seed] = [int(v) for v in c]
    return h


def tree_table(counts):
    """A second statement of the rule with an explicit tree: every merge makes a node above its two parts, a symbol's length is its depth.  The
    node takes the place (the index) of c1 among the candidates."""
    nodes = {i: (int(c), ("leaf", i)) for i, c in enumerate(list(counts) + [1]) if c}
    while len(nodes) > 1:
        order = sorted(nodes, key=lambda i: (nodes[i][0], -i))
        c1, c2 = order[0], order[1]
        nodes[c1] = (nodes[c1][0] + nodes[c2][0], ("node", nodes[c1][1], nodes[c2][1]))
        del nodes[c2]
    depth = {}
    stack = [(next(iter(nodes.values()))[1], 0)]
    while stack:
        t, d = stack.pop()
        if t[0] == "leaf":
            depth[t[1]] = d
        else:
            stack += [(t[1], d + 1), (t[2], d + 1)]
    real = sorted((s for s in depth if s < 256), key=lambda s: (depth[s], s))
    if not real:
        return [0] * 16, [], depth
    bits = [0] * (max(depth.values()) + 2)
    for d in depth.values():
        bits[d] += 1
    for i in range(len(bits) - 1, 16, -1):
        while bits[i]:
            j = max(k for k in range(i - 1) if bits[k])
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    bits = (bits + [0] * 17)[:17]
    bits[max(k for k in range(17) if bits[k])] -= 1
    return bits[1:], real, depth


# ---- the tables -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(adversarial_histograms()))
def test_table_on_adversarial_histograms(name):
    counts = adversarial_histograms()[name]
    bits, symbols = emu.table(counts)
    assert len(bits) == 16 and all(0 <= b <= 255 for b in bits)                       # every length is <= 16
    kraft = sum(b << (16 - l) for l, b in enumerate(bits, 1))
    assert kraft <= 65535, kraft                                                      # no code is all 1-bits
    assert sorted(symbols) == [s for s in range(256) if counts[s]]                    # every counted symbol has a code, no other has
    assert sum(bits) == len(symbols)
    want_bits, want_symbols, depth = tree_table(counts)
    assert (bits, symbols) == (want_bits, want_symbols)
    assert symbols == sorted(symbols, key=lambda s: (depth[s], s))
    code, length = emu444._huff((bits, symbols))
    assert all(length[s] > 0 for s in symbols) and (length > 0).sum() == len(symbols)
    if symbols:
        assert int(max(code[s] for s in symbols)) < (1 << 16) - 1


def test_adversarial_histograms_reach_what_they_are_for():
    h = adversarial_histograms()
    assert max(emu.code_lengths(h["fibonacci"])) == 22                                # far above 16: the limiting step runs
    assert max(emu.code_lengths(h["powers of two"])) >= 29 and max(emu.code_lengths(h["256 ones"])) == 9
    for name in ("fibonacci", "powers of two", "powers of two, descending", "fibonacci, scattered"):
        bits, _ = emu.table(h[name])
        assert sum(b << (16 - l) for l, b in enumerate(bits, 1)) == 65535, name
    assert emu.table(h["256 equal"])[0] == [0] * 7 + [255, 1] + [0] * 7 == emu.table(h["all 2^32 - 1"])[0]
    assert emu.table(h["empty"]) == ([0] * 16, [])
    assert emu.table(h["one symbol"]) == ([1] + [0] * 15, [3])
    assert emu.table(h["two symbols"]) == ([1, 1] + [0] * 14, [9, 0])
    deep = h["fibonacci from 1, 2"]
    assert max(deep) < 1 << 32 and max(emu.code_lengths(deep)) == 43 > 32


def test_dht_and_coder_forms():
    specs = [emu.table(h) for h in (adversarial_histograms()[n] for n in ("fibonacci", "256 equal", "one symbol", "empty"))]
    d = emu.dht(specs)
    assert d.shape == (4, 272) and d.dtype == np.uint8
    for k, (bits, symbols) in enumerate(specs):
        assert list(d[k, :16]) == bits and list(d[k, 16:16 + len(symbols)]) == symbols and not d[k, 16 + len(symbols):].any()
    w = emu.coder_words([specs[2], specs[1], specs[3], specs[0]])
    assert w.shape == (544,) and w.dtype == np.uint32
    assert w[3] == (1 << 16) and not w[:3].any() and not w[4:32].any()                # DC luminance: symbol 3, the code 0 of one bit
    assert (w[32:288] >> 16).tolist().count(8) == 255 and (w[32:288] >> 16).max() == 9


# ---- the files ------------------------------------------------------------------------------------------------------------------------------------
def _cases():
    for sub in ("444", "420"):
        for H, W in GRIDS[sub].SIZES:
            for quality in GRIDS[sub].QUALITIES:
                yield sub, quality, H, W


@pytest.mark.parametrize("sub,quality,H,W", list(_cases()))
def test_files_decode_to_the_fixed_table_pixels_and_are_not_larger(sub, quality, H, W):
    larger = []
    for kind in emu.KINDS:
        img = emu.frame(kind, H, W)
        for ri in GRIDS[sub].intervals(H, W):
            own, fixed = emu.file(img, quality, ri, sub), FIXED[sub].file(img, quality, ri)
            scan = emu.scan(img, quality, ri, sub)
            assert 0 < len(scan) <= emu.capacity(H, W, ri, sub)
            GRIDS[sub].check_scan(scan, H, W, ri)
            assert (decode(own, W, H) == decode(fixed, W, H)).all(), (kind, ri)
            specs = emu.frame_tables(img, quality, ri, sub)
            assert own == output.jpeg_from_scan(scan, W, H, quality, ri, sub, emu.dht(specs)), "output.jpeg_from_scan differs from the emulator's file"
            h = emu.histogram(img, quality, ri, sub)
            assert h.shape == (4, 256) and not h[0, 12:].any() and not h[2, 12:].any()
            blocks = 3 if sub == "444" else 6
            my, mx, _ = FIXED[sub].geometry(H, W, ri)
            assert h[0].sum() + h[2].sum() == my * mx * blocks                        # one DC symbol per block
            print("%s %s %d x %d q %d interval %d: %d bytes, fixed %d" % (sub, kind, H, W, quality, ri, len(own), len(fixed)))
            if len(own) > len(fixed):
                larger.append((kind, ri, len(own), len(fixed)))
    assert not larger, larger


def test_capacity_follows_the_212_byte_block():
    lib = _lib.lib()
    for sub, prefix in (("444", "lwg_jpeg"), ("420", "lwg_jpeg420")):
        most = getattr(lib, prefix + "_max_mcus_per_segment")()
        for H, W in GRIDS[sub].SIZES + ((512, 512), (1024, 1024)):
            for ri in GRIDS[sub].intervals(H, W) + [most]:
                cap = emu.capacity(H, W, ri, sub)
                _, _, nseg = FIXED[sub].geometry(H, W, ri)
                assert getattr(lib, prefix + "_scan_opt_capacity")(H, W, ri) == cap > FIXED[sub].capacity(H, W, ri)
                assert getattr(lib, prefix + "_scan_opt_ws_bytes")(3, H, W, ri) >= 3 * (cap - 2 * (nseg - 1)) + 3 * (nseg + 1) * 544 * 4
    assert emu.BLOCK_BYTES == 212 and emu.BLOCK_BYTES % 4 == 0 and emu.BLOCK_BYTES >= (16 + 11 + 63 * 26 + 7) // 8 == 209
    assert emu.capacity(512, 512, 64) == 64 * 64 * 3 * 212 * 2 + 2 * 63


# ---- the host side --------------------------------------------------------------------------------------------------------------------------------
def test_headers_with_default_arguments_are_todays():
    for sub in ("444", "420"):
        for (W, H, q, ri) in ((1, 1, 50, 1), (23, 17, 90, 2), (512, 512, 90, 32), (65535, 9, 100, 64)):
            base = FIXED[sub].headers(W, H, emu.quant_tables(q), ri)
            assert output.jpeg_headers(W, H, q, ri, sub) == base == output.jpeg_headers(W, H, q, ri, sub, None)
            assert output.jpeg_headers(W, H, q, ri, subsampling=sub, tables=None) == base
            assert output.jpeg_from_scan(b"\x12", W, H, q, ri, sub) == base + b"\x12\xff\xd9" == output.jpeg_from_scan(b"\x12", W, H, q, ri, sub, None)
            specs = [emu.table(h) for h in emu.histogram(emu.frame("smooth_noise", 24, 40), q, 2, sub)]
            own = output.jpeg_headers(W, H, q, ri, sub, emu.dht(specs))
            assert own == emu.headers(W, H, emu.quant_tables(q), ri, specs, sub) and len(own) < len(base)
    assert output.jpeg_headers(8, 8, 90, 1) == emu444.headers(8, 8, emu444.tables(90), 1)
    for bad in (np.zeros((4, 271), np.uint8), np.zeros((3, 272), np.uint8), np.zeros((4, 272), np.int32)):
        with pytest.raises(ValueError):
            output.jpeg_headers(8, 8, 90, 1, "444", bad)


def test_new_symbols_are_declared_and_bound():
    hdr = _lib.header_symbols()
    for name in NEW:
        assert name in hdr and name in _lib._SIGS, name
        assert getattr(_lib.lib(), name) is not None
    assert _lib.lib().lwg_abi_version() == 10


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.lib()
    good = bytes([1] * 128)
    for prefix in ("lwg_jpeg", "lwg_jpeg420"):
        R = getattr(lib, prefix + "_max_mcus_per_segment")()
        ok = dict(u8=16, B=1, H=8, W=8, q=good, ri=1, ws=16, scans=16, nbytes=16, tables=16, hist=16)

        def scan(**kw):
            a = dict(ok, **kw)
            return getattr(lib, prefix + "_scan_opt_u8")(a["u8"], a["B"], a["H"], a["W"], a["q"], a["ri"], a["ws"], a["scans"], a["nbytes"], a["tables"], None)

        def hist(**kw):
            a = dict(ok, **kw)
            return getattr(lib, prefix + "_hist_u8")(a["u8"], a["B"], a["H"], a["W"], a["q"], a["ri"], a["ws"], a["hist"], None)
        shared = (dict(u8=None), dict(q=None), dict(ws=None), dict(B=0), dict(B=-3), dict(H=0), dict(W=-1), dict(H=65536), dict(W=65536), dict(ri=0),
                  dict(ri=-1), dict(ri=R + 1), dict(ri=65536), dict(q=bytes([1] * 127 + [0])), dict(q=bytes([0] + [1] * 127)),
                  dict(H=16384, W=16384, ri=R), dict(ws=24))
        for bad in shared + (dict(scans=None), dict(nbytes=None), dict(tables=None), dict(tables=18)):
            assert scan(**bad) == 1, bad
        for bad in shared + (dict(hist=None), dict(hist=18)):
            assert hist(**bad) == 1, bad
        for H, W, ri in ((0, 8, 1), (8, 0, 1), (8, 8, 0), (8, 8, R + 1), (8, 8, 65536), (16384, 16384, R), (65536, 8, 1)):
            assert getattr(lib, prefix + "_scan_opt_capacity")(H, W, ri) == 0
            assert getattr(lib, prefix + "_scan_opt_ws_bytes")(1, H, W, ri) == 0
        assert getattr(lib, prefix + "_scan_opt_ws_bytes")(0, 8, 8, 1) == 0
    for bad in ((None, 1, 16, 16), (16, 1, None, 16), (16, 1, 16, None), (16, 0, 16, 16), (16, -1, 16, 16), (18, 1, 16, 16), (16, 1, 18, 16), (16, 1, 16, 18)):
        assert lib.lwg_jpeg_huff_tables(*bad, None) == 1, bad


def test_bad_huffman_raises_and_there_is_no_cpu_fallback():
    import torch
    from ipercore_amd import ops
    from ipercore_amd.imitator import Imitator
    with tempfile.TemporaryDirectory() as d:
        for enc in ("jpeg", "mjpeg", "host"):
            w = output.FrameWriter(d, encoder=enc, huffman="optimized")
            try:
                assert w.huffman == "optimized" and w.subsampling == "444"
                if enc != "host":
                    with pytest.raises(RuntimeError):
                        w.submit(torch.zeros(1, 3, 8, 8), 0)
            finally:
                assert w.close() == []
        w = output.FrameWriter(d, encoder="jpeg")
        assert w.huffman == "fixed" and w.close() == []
        for bad in ("optimised", "adaptive", True, None, ""):
            with pytest.raises(ValueError):
                output.FrameWriter(d, encoder="jpeg", huffman=bad)
    frames = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ops.jpeg_scan(frames, huffman="optimized")
    with pytest.raises(RuntimeError):
        ops.jpeg_symbol_histogram(frames)
    with pytest.raises(RuntimeError):
        ops.jpeg_huffman_tables(torch.zeros(1, 4, 256, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.jpeg_scan(frames, 90, None, "444", "optimised")
    for bad in ("optimised", "per-frame", 1):
        with pytest.raises(ValueError, match="jpeg_huffman"):
            Imitator({"jpeg_huffman": bad}, device=torch.device("cpu"))
