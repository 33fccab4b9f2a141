"""CPU checks of csrc/lwg_wgrad_slab.h - the slab format, the split plan and the tile width of the weight-gradient family - by inclusion.

Part 1 of the header is compiled into a stand-alone host program with signed-overflow traps (the pattern of
tests/test_direct_conv_contracts_cpu.py::test_fit_helpers_by_inclusion) that prints, for small un-packing cases, (src, dst, bias) of every output
element through lwg_unpack_map and through the quad decode of the unpack4 kernels, the verdicts of lwg_wgrad_unpack_map_make and a list of split
plans; the tests hold them to a numpy / Python restatement written from the format's description, not from the header's text.
tests/golden/wgrad_plans_parent.json is what the three engines' workspace queries answered on the parent commit, where each engine had its own copy
of the split function (tests/wgrad_slab_cases.py wrote it, once): the tree must reproduce every value, and so must the restatement.  The source
audit is the converse: the K order, the parameter layout and the split rule are spelled in the header and nowhere else in csrc/."""
import glob
import json
import os
import re
import subprocess
import tempfile

import numpy as np

from tests import wgrad_slab_cases as wsc
from tests.test_conv_offsets_cpu import CSRC, ROOT, _code, _compiler

HEADER = "lwg_wgrad_slab.h"
ENGINES = ("conv_wgrad.hip", "conv_wgrad_bf16.hip", "conv_wgrad_winograd.hip")
MAX_TAPS = 52
T9, T16 = list(range(9)), list(range(16))

# name -> ntaps, cin, cin_pad, nout, n_pad, transposed, (D0, D1, KH, KW), kidx
MAPS = {
    "chunked 24 of 32, 4 of 64": (9, 24, 32, 4, 64, 0, (4, 24, 3, 3), T9),
    "chunked 64, two chunks, transposed": (9, 40, 64, 8, 8, 1, (40, 8, 3, 3), T9),
    "parity 4 of 16, transposed": (4, 64, 64, 8, 64, 1, (64, 8, 4, 4), wsc.PARITY_KIDX),
    "small 6 of 8, 4 of 64": (9, 6, 8, 4, 64, 0, (4, 6, 3, 3), T9),
    "small 8, transposed, odd nout": (4, 8, 8, 5, 8, 1, (9, 7, 2, 2), [3, 0, 2, 1]),
    "adjoint 16 taps": (16, 20, 32, 8, 8, 0, (8, 20, 4, 4), wsc.ADJ_KIDX),
    "roomy tensor": (9, 24, 32, 12, 64, 0, (13, 30, 3, 3), T9[::-1]),
    "one tap, cin_pad 4": (1, 3, 4, 4, 4, 0, (4, 3, 1, 1), [0]),
}
# label -> mutation of the base call of lwg_wgrad_unpack_map_make (9 taps, 32 -> 64 channels, cin 24, nout 60, (60, 24, 3, 3))
MAKE_BASE = dict(pa=1, kidx=1, ntaps=9, C0=16, C1=16, N=64, D0=60, D1=24, KH=3, KW=3, tr=0, cin=24, nout=60, k0=0)
MAKES = [("base", {}, True), ("transposed base", dict(tr=1, D0=24, D1=60), True), ("cin = cin_pad, nout = N", dict(cin=32, nout=64, D0=64, D1=32), True),
         ("pa null", dict(pa=0), False), ("kidx null", dict(kidx=0), False), ("cin 0", dict(cin=0), False), ("cin over C0 + C1", dict(cin=33, D1=40), False),
         ("nout 0", dict(nout=0), False), ("nout over N", dict(nout=65, D0=70), False), ("kidx negative", dict(k0=-1), False), ("kidx = KH KW", dict(k0=9), False),
         ("D0 under nout", dict(D0=59), False), ("D1 under cin", dict(D1=23), False), ("transposed: D0 under cin", dict(tr=1, D0=23, D1=60), False),
         ("transposed: D1 under nout", dict(tr=1, D0=24, D1=59), False), ("ntaps 0", dict(ntaps=0), False), ("ntaps over the maximum", dict(ntaps=MAX_TAPS + 1), False),
         ("kidx = KH KW - 1", dict(k0=8), True)]
CAP48, CAP64 = 48 << 20, 64 << 20
# (blocks, nchunks, workgroups, slab bytes, cap bytes): the clamps one by one, then the contract's extremes - 52 taps, Cin = N = 1024 (3328 tiles, a 218 MB
# slab), M at the end of the buffer range of a 4-channel fp32 input (0xC0000000 / 16 rows)
PLANS = [(36, 128, 512, 2305 * 256 * 4, CAP48), (784, 9999, 512, 25089 * 512 * 4, CAP48), (144, 8192, 512, 4609 * 512 * 4, CAP48), (1, 7, 512, 4096, CAP48),
         (1, 2, 512, 4096, CAP48), (1, 1 << 20, 512, 260, CAP48), (8, 288, 256, 64 * 64 * 64, CAP64), (3328, 6291456, 512, 53249 * 1024 * 4, CAP48),
         (1, 6291456, 512, 5 * 4 * 4, CAP48), (3328, 3145728, 512, 53249 * 1024 * 4, CAP48), (256, 50331648, 256, 64 * 1024 * 1024, CAP64), (1, 1 << 20, 512, 1 << 20, CAP48),
         (1, 2147483647 // 32, 2147483647, 4, CAP48)]
SHAPES = [(1, 4), (36, 64), (288, 192), (576, 128), (53248, 1024), (9 * 512, 512), (72, 320), (8, 65)]          # (Ktot, N): tile width, tiles, slab floats

_AUDIT = r"""
#include <cstdio>
#include "lwg_wgrad_slab.h"
struct Map { int ntaps, cin, cin_pad, nout, n_pad, tr, D0, D1, KH, KW; int kidx[LWG_MAX_TAPS]; };
struct Make { int pa, kidx, ntaps, C0, C1, N, D0, D1, KH, KW, tr, cin, nout, k0; };
struct Plan { int blocks, nchunks, wg; long long slab, cap; };
struct Shape { int Ktot, N; };
static const Map maps[] = { MAPS };
static const Make makes[] = { MAKES };
static const Plan plans[] = { PLANS };
static const Shape shapes[] = { SHAPES };
int main() {
    int ci = 0;
    for (const Map& m : maps) {
        LwgConvArgs a = {};
        a.C0 = m.cin_pad, a.N = m.n_pad, a.ntaps = m.ntaps;
        LwgUnpackMap u;
        if (!lwg_wgrad_unpack_map_make(&a, m.D0, m.D1, m.KH, m.KW, m.tr, m.kidx, m.cin, m.nout, &u)) return 2;
        std::printf("case %d %zu %zu %d\n", ci, lwg_unpack_weights(u), lwg_unpack_slab_floats(u), lwg_unpack_bias_row(u));
        const size_t total = lwg_unpack_weights(u) + m.nout;
        for (size_t i = 0; i < total; ++i) {
            size_t src, dst;
            bool bias;
            lwg_unpack_map(u, i, src, dst, bias);
            std::printf("m %d %zu %zu %zu %d\n", ci, i, src, dst, (int)bias);
        }
        if (m.nout % 4 == 0)
            for (size_t i4 = 0; i4 < total / 4; ++i4) {
                const LwgUnpackQuad q = lwg_unpack_quad(u, i4);
                for (int j = 0; j < 4; ++j)
                    std::printf("q %d %zu %zu %zu %d\n", ci, i4 * 4 + j, q.src + j, q.bias ? (size_t)(q.n + j) : lwg_unpack_dst(u, q.tap, q.c, q.n + j), (int)q.bias);
            }
        for (int tap = 0; tap < m.ntaps; ++tap)
            for (int c = 0; c < m.cin_pad; ++c) {
                int t2, c2;
                lwg_korder_decode(lwg_unpack_k(u, tap, c), m.ntaps, m.cin_pad, t2, c2);
                if (t2 != tap || c2 != c) return 3;
            }
        ++ci;
    }
    ci = 0;
    for (const Make& k : makes) {
        LwgConvArgs a = {};
        a.C0 = k.C0, a.C1 = k.C1, a.N = k.N, a.ntaps = k.ntaps;
        int kidx[LWG_MAX_TAPS + 1] = {};
        kidx[0] = k.k0;
        for (int i = 1; i < LWG_MAX_TAPS + 1; ++i) kidx[i] = i % (k.KH * k.KW);
        LwgUnpackMap u;
        std::printf("mk %d %d\n", ci++, (int)lwg_wgrad_unpack_map_make(k.pa ? &a : nullptr, k.D0, k.D1, k.KH, k.KW, k.tr, k.kidx ? kidx : nullptr, k.cin, k.nout, &u));
    }
    ci = 0;
    for (const Plan& p : plans) {
        const LwgSplitPlan r = lwg_wgrad_split_plan(p.blocks, p.nchunks, p.wg, p.slab, p.cap);
        std::printf("pl %d %d %d\n", ci++, r.splits, r.cps);
    }
    ci = 0;
    for (const Shape& s : shapes) std::printf("sh %d %d %d %zu\n", ci++, lwg_wgrad_bn(s.N), lwg_wgrad_tiles(s.Ktot, s.N), lwg_wgrad_slab_floats(s.Ktot, s.N));
    std::printf("maxtaps %d\n", LWG_MAX_TAPS);
    return 0;
}
"""


def _run_audit():
    maps = ", ".join("{%d, %d, %d, %d, %d, %d, %d, %d, %d, %d, {%s}}" % (m[:6] + m[6] + (", ".join(map(str, m[7])),)) for m in MAPS.values())
    keys = ("pa", "kidx", "ntaps", "C0", "C1", "N", "D0", "D1", "KH", "KW", "tr", "cin", "nout", "k0")
    makes = ", ".join("{%s}" % ", ".join(str(dict(MAKE_BASE, **mut)[k]) for k in keys) for _, mut, _ in MAKES)
    plans = ", ".join("{%d, %d, %d, %dll, %dll}" % p for p in PLANS)
    src = _AUDIT.replace(" MAPS ", " %s " % maps).replace(" MAKES ", " %s " % makes).replace(" PLANS ", " %s " % plans)
    src = src.replace(" SHAPES ", " %s " % ", ".join("{%d, %d}" % s for s in SHAPES))
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "audit.cpp"), os.path.join(tmp, "audit")
        open(cpp, "w").write(src)
        flags = ["-std=c++17", "-O1", "-fsanitize=signed-integer-overflow", "-fsanitize-trap=signed-integer-overflow", "-Wno-unused-variable", "-Wno-unused-function"]
        r = subprocess.run([_compiler(), *flags, "-I", CSRC, cpp, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-500:])
    return r.stdout


_OUT = []


def _audit():
    """The audit program's output, compiled and run once per session."""
    if not _OUT:
        _OUT.append(_run_audit())
    return _OUT[0]


def _rows(tag, n):
    return [tuple(int(v) for v in m) for m in re.findall(r"^%s %s$" % (tag, " ".join([r"(-?\d+)"] * n)), _audit(), re.M)]


def _restated_map(ntaps, cin, cin_pad, nout, n_pad, transposed, D, kidx):
    """(src, dst, bias) of every output element i in [0, ntaps cin nout + nout): i = (tap, c, n) with n fastest, then the nout bias elements.  The slab
    row of (tap, c) is chunk-major / tap-minor for whole 32-channel chunks, tap-major otherwise; row ntaps cin_pad is the bias gradient."""
    i = np.arange(ntaps * cin * nout + nout, dtype=np.int64)
    n, r = i % nout, i // nout
    bias = r >= ntaps * cin
    tap, c = np.where(bias, 0, r // cin), r % cin
    k = (c // 32 * ntaps + tap) * 32 + c % 32 if cin_pad % 32 == 0 else tap * cin_pad + c
    k = np.where(bias, ntaps * cin_pad, k)
    d0, d1 = (c, n) if transposed else (n, c)
    dst = (d0 * D[1] + d1) * (D[2] * D[3]) + np.asarray(kidx, dtype=np.int64)[tap]
    return k * n_pad + n, np.where(bias, n, dst), bias


def test_unpack_map_by_inclusion():
    """lwg_unpack_map as the reduction kernels compile it against the restatement, for both K orders (cin_pad 32 and 64 against 8 and 4), cin < cin_pad,
    nout < n_pad, both parameter layouts, a parity launch's 4 of 16 kernel positions and pack_dgrad_conv_transpose's 16-tap order; dst is injective over
    the weight elements and inside the tensor, src inside one slab, the bias elements in row ntaps cin_pad; lwg_korder_decode inverts lwg_korder_k
    (the program returns 3 otherwise)."""
    heads, rows = _rows("case", 4), _rows("m", 5)
    assert len(heads) == len(MAPS)
    assert sorted(set(wsc.ADJ_KIDX)) == T16 and len(set(wsc.PARITY_KIDX)) == 4
    for ci, (name, (ntaps, cin, cin_pad, nout, n_pad, tr, D, kidx)) in enumerate(MAPS.items()):
        src, dst, bias = _restated_map(ntaps, cin, cin_pad, nout, n_pad, tr, D, kidx)
        got = np.array([r[1:] for r in rows if r[0] == ci], dtype=np.int64)
        weights, slab = ntaps * cin * nout, (ntaps * cin_pad + 1) * n_pad
        assert heads[ci] == (ci, weights, slab, ntaps * cin_pad), (name, heads[ci])
        assert got.shape == (weights + nout, 4) and (got[:, 0] == np.arange(weights + nout)).all(), name
        assert (got[:, 1] == src).all() and (got[:, 2] == dst).all() and (got[:, 3] == bias).all(), name
        w = got[:weights]
        assert not w[:, 3].any() and got[weights:, 3].all(), name
        assert len(set(w[:, 2].tolist())) == weights and w[:, 2].min() >= 0 and w[:, 2].max() < D[0] * D[1] * D[2] * D[3], name
        assert got[:, 1].min() >= 0 and got[:, 1].max() < slab and len(set(got[:, 1].tolist())) == weights + nout, name
        assert (w[:, 1] // n_pad < ntaps * cin_pad).all(), name
        assert (got[weights:, 1] // n_pad == ntaps * cin_pad).all() and (got[weights:, 2] == np.arange(nout)).all(), name
        assert set((w[:, 2] % (D[2] * D[3])).tolist()) == set(kidx), name                    # only the launch's kernel positions are written


def test_quad_decode_gives_the_scalar_map():
    """For nout % 4 == 0 the quad decode of the unpack4 kernels gives, for each of its four lanes, exactly lwg_unpack_map's (src, dst, bias)."""
    scalar, quad = _rows("m", 5), _rows("q", 5)
    done = 0
    for ci, (name, m) in enumerate(MAPS.items()):
        s, q = [r for r in scalar if r[0] == ci], [r for r in quad if r[0] == ci]
        if m[3] % 4:
            assert not q, name
            continue
        assert q == s and len(q) == m[0] * m[1] * m[3] + m[3], name
        done += 1
    assert done >= 6


def test_unpack_map_make_clauses():
    """lwg_wgrad_unpack_map_make refuses each clause it refused as conv_wgrad.hip's function and accepts the base calls."""
    got = dict(_rows("mk", 2))
    assert len(got) == len(MAKES) and int(re.search(r"^maxtaps (\d+)$", _audit(), re.M).group(1)) == MAX_TAPS
    wrong = {label: got[j] for j, (label, _, ok) in enumerate(MAKES) if got[j] != int(ok)}
    assert not wrong, wrong
    assert sum(not ok for _, _, ok in MAKES) >= 12


def _restated_plan(blocks, nchunks, workgroups, slab_bytes, cap_bytes):
    """-> (splits, chunks per split, the clamps that bound): fill the workgroup budget, stay under the byte cap, at least four chunks per workgroup, at
    least one split; then drop the splits that would get no chunk."""
    hit = set()
    s = workgroups // blocks
    if s * slab_bytes > cap_bytes:
        s, _ = cap_bytes // slab_bytes, hit.add("cap")
    if s > nchunks // 4:
        s, _ = nchunks // 4, hit.add("chunks")
    if s < 1:
        s, _ = 1, hit.add("one")
    cps = -(-nchunks // s)
    kept = -(-nchunks // cps) if cps else 0
    if kept < s:
        hit.add("dropped")
    return kept, cps, hit


def test_split_plan_by_inclusion():
    """lwg_wgrad_split_plan under the overflow traps: each clamp, the direct kernel's 128 chunks over 14 splits -> 13, and the contract's extremes; cps is
    what the launchers used to derive again from the returned splits; the tile width and the slab size."""
    got = _rows("pl", 3)
    assert len(got) == len(PLANS)
    seen = set()
    for (j, splits, cps), p in zip(got, PLANS):
        want = _restated_plan(*p)
        assert (splits, cps) == want[:2] and cps == -(-p[1] // splits) and splits >= 1 and splits * cps >= p[1] > (splits - 1) * cps, (p, splits, cps, want)
        seen |= want[2]
    assert got[0][1:] == (13, 10) and seen == {"cap", "chunks", "one", "dropped"}
    sh = _rows("sh", 4)
    for (j, bn, tiles, floats), (Ktot, N) in zip(sh, SHAPES):
        wbn = 64 if 1 <= N % 128 <= 64 else 128
        assert (bn, tiles, floats) == (wbn, -(-Ktot // 128) * -(-N // wbn), (Ktot + 1) * N), (Ktot, N)
    assert len(sh) == len(SHAPES) and {r[1] for r in sh} == {64, 128}


def _engine_plans(S, div, B, nt, C, N):
    """The three engines' parameters of the split plan for one grid entry (256 CUs) -> {engine: restated plan or None outside its contract}."""
    H = S // div
    Ktot, M = nt * C, B * H * H
    bn = 64 if 1 <= N % 128 <= 64 else 128
    tiles, slab = -(-Ktot // 128) * -(-N // bn), (Ktot + 1) * N * 4
    out = {"direct": _restated_plan(tiles, -(-M // 32), 512, slab, CAP48), "bf16": None, "winograd": None}
    if C % 32 == 0 and N % 64 == 0:
        out["bf16"] = _restated_plan(tiles, -(-M // 64), 2 * 256, slab, CAP48)
    if nt == 9 and C % 64 == 0 and N % 64 == 0:
        out["winograd"] = _restated_plan((C // 64) * (N // 64), -(-(B * ((H + 1) // 2) ** 2) // 8), 256, 64 * C * N, CAP64)
    return out


def test_split_plans_are_the_parents():
    """Every value of tests/golden/wgrad_plans_parent.json - the three workspace queries over wgrad_slab_cases.plan_grid(), recorded on the parent
    commit - from the tree's library, and from the restatement with each engine's constants; the grid reaches every clamp in every engine."""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "wgrad_plans_parent.json")))
    grid = wsc.plan_grid()
    assert all(len(gold[e]) == len(grid) for e in ("direct", "bf16", "winograd"))
    assert wsc.plans() == gold
    seen = {e: set() for e in gold}
    for j, g in enumerate(grid):
        for e, p in _engine_plans(*g).items():
            assert gold[e][j] == (p[0] if p else -1), (e, g, gold[e][j], p)
            if p:
                seen[e] |= p[2]
    # On 256 CUs the byte cap binds in no engine, K = 9 x 512 with N = 512 included: a full budget of 128 x 128 tiles is 512 x 64 KB = 32 MB of slabs
    # under the cap of 48, and 256 Winograd blocks of 64 x 64 x 16 are the cap's 64 MB exactly.  The cap is there for devices with more CUs;
    # test_split_plan_by_inclusion drives it.
    assert all(v == {"chunks", "one", "dropped"} for v in seen.values()), seen
    at = lambda *g: gold["direct"][grid.index(g)]                                    # noqa: E731
    assert at(256, 4, 1, 9, 256, 256) == 13                                          # 128 chunks over 14 splits: 10 each
    assert at(512, 1, 1, 49, 512, 512) == 1                                          # 784 tiles: the budget gives 0
    assert at(512, 1, 1, 9, 512, 512) == 3                                           # 144 tiles, 3 x 9.4 MB
    assert at(256, 32, 1, 9, 64, 64) == 1                                            # 2 chunks


def test_the_family_spells_the_format_once():
    """The converse of the audits: the three engines include the header; the K-order expression, the parameter-tensor offset and the split rule occur in
    the header and in no other file of csrc/."""
    files = sorted(os.path.basename(p) for ext in ("*.hip", "*.h") for p in glob.glob(os.path.join(CSRC, ext)))
    assert HEADER in files and "lwg_wgrad_reduce.h" not in files
    for pat in (r"& 31\) == 0 \?", r"\? c\w*[^:;?]*: n\w*[^:;?]*\) \* [\w.>-]*D1", r"\? n\w*[^:;?]*: c\w*[^:;?]*\)\) \* [\w.>-]*KHW", r"splits > nchunks / 4"):
        assert [f for f in files if re.search(pat, _code(f))] == [HEADER], pat
    for name in ENGINES:
        assert '#include "%s"' % HEADER in _code(name), name
