"""The conditions that make tests/test_gpu_raster_scenes.py meaningful, pinned on the oracle alone (CPU): each scene of tests/raster_scenes.py
does reach the code path it was built for.  Counts are totals per tile / per pixel: the order of a bin's face list is not defined."""
import numpy as np
import pytest

from oracle import lwg_oracle as orc
from tests import raster_scenes as rs
from tests.test_raster_property import _fp64_rasterize

LWG_RPAIRS, LWG_RCHUNK = 12288, 256          # csrc/raster.hip


def _oracle(f, S, near=0.1, far=100.0):
    fim, wim = orc.rasterize_fim_wim(f[None], S, near, far)
    return fim[0].numpy(), wim[0].numpy()


def _winner_from_restatement(f, S, near=0.1, far=100.0):
    """argmin over (depth, id) of the numpy restatement: must be the oracle's map (this pins the restatement the counts below rely on)."""
    hit, zp = rs.cover_and_depth(f, S, near, far)
    best = zp.argmin(axis=0)                                    # the first (lowest id) of equal minima
    return np.where(np.isfinite(zp.min(axis=0)), best, -1), hit, zp


def _assert_inside_boxes(f, S, fim):
    """Every pixel the oracle gives to a face lies inside the box the kernel's setup gives that face (so culling cannot drop a winner)."""
    box = rs.kernel_boxes(f, S)
    rr, cc = np.nonzero(fim >= 0)
    b = box[fim[rr, cc]]
    y = S - 1 - rr
    assert ((b[:, 0] <= cc) & (cc <= b[:, 1]) & (b[:, 2] <= y) & (y <= b[:, 3])).all()


@pytest.mark.parametrize("name", ["full96", "half96"])
def test_stacks_overflow_the_hit_list_within_one_chunk(name):
    f = rs.full_stack(96) if name == "full96" else rs.half_stack(96)
    S = 32
    assert f.shape[0] <= LWG_RCHUNK and f.shape == (96, 3, 3) and f.dtype == np.float32
    want, hit, _ = _winner_from_restatement(f, S)
    fim, _ = _oracle(f, S)
    assert np.array_equal(want, fim) and ((fim >= 0).all() if name == "full96" else (fim >= 0).mean() > 0.8)
    per_tile = hit.reshape(96, 2, 16, 2, 16).sum(axis=(0, 2, 4))
    print(name, "hits per tile", per_tile.tolist())
    assert (per_tile > LWG_RPAIRS).all()                        # one chunk, more hits than the list holds: only flushing gets this right
    if name == "half96":
        frac = hit.reshape(96, 2, 16, 2, 16).mean(axis=(2, 4))
        assert frac.min() >= 0.35 and frac.max() <= 0.65        # no group of 32 candidates fills 256 * 32 entries by itself
    _assert_inside_boxes(f, S, fim)


def test_full_stack_600_spans_chunks_and_the_winner_is_not_in_the_first():
    f = rs.full_stack(600)
    assert f.shape[0] > 2 * LWG_RCHUNK
    fim, _ = _oracle(f, 32)
    assert (fim == 307).all() and 307 >= LWG_RCHUNK
    hit, _ = rs.cover_and_depth(f, 32)
    assert hit.all()


def test_ties_go_to_the_lowest_id():
    f = rs.ties()
    S = 32
    for g in rs.TIE_GROUPS:
        for i in g[1:]:
            assert np.array_equal(f[i], f[g[0]])
    want, _, zp = _winner_from_restatement(f, S)
    fim, _ = _oracle(f, S)
    assert np.array_equal(want, fim)
    two = np.sort(zp, axis=0)[:2]
    tie = np.isfinite(two[0]) & (two[0].view(np.int32) == two[1].view(np.int32))
    print("tie pixels", int(tie.sum()), "winners", sorted(set(fim[tie].tolist())))
    assert tie.sum() >= 100
    lowest = {min(g) for g in rs.TIE_GROUPS}
    assert set(fim[tie].tolist()) == lowest                     # every group wins pixels, always under its lowest id
    for g in rs.TIE_GROUPS:
        assert not np.isin(fim, [i for i in g if i != min(g)]).any()
    assert max(rs.TIE_GROUPS[3]) // LWG_RCHUNK != min(rs.TIE_GROUPS[3]) // LWG_RCHUNK
    _assert_inside_boxes(f, S, fim)


@pytest.mark.parametrize("S", [32, 48])
@pytest.mark.parametrize("z", ["const", "vertex"])
def test_lattice_has_no_holes(S, z):
    f, (lo, hi) = rs.lattice(S, z=z)
    assert (rs.signed_area2(f) > 0).all()
    fim, wim = _oracle(f, S)
    inner = fim[S - 1 - hi:S - lo, lo:hi + 1]
    assert (inner >= 0).all()                                   # edges and vertices on pixel centres leave no hole
    assert set(np.unique(inner).tolist()) == set(range(f.shape[0]))          # and every face keeps its interior pixel
    outside = np.ones((S, S), dtype=bool)
    outside[S - 1 - hi:S - lo, lo:hi + 1] = False
    assert (fim[outside] == -1).all()
    on = wim[fim >= 0]
    assert ((on == 0).any(axis=1)).sum() > 0.3 * len(on)        # pixel centres on edges: a weight of exactly 0
    assert ((on == 1).any(axis=1)).sum() >= (f.shape[0] // 2) // 2               # and on vertices: a weight of exactly 1
    f2, _ = rs.lattice(S, z=z, layers=2)
    fim2, _ = _oracle(f2, S)
    assert np.array_equal(fim2[S - 1 - hi:S - lo, lo:hi + 1], inner)             # the second layer is hidden behind the first ...
    assert (fim2[outside] >= f.shape[0]).sum() > 0                               # ... and shows beyond its rim
    _assert_inside_boxes(f2, S, fim2)


def _drawn(f, S, near=0.1, far=100.0):
    fim, _ = _oracle(f, S, near, far)
    return set(np.unique(fim[fim >= 0]).tolist()), fim


def test_degenerate_faces_draw_what_is_recorded():
    S = 32
    f = rs.degenerate(S)
    names = rs.DEGENERATE_NAMES
    alone = tuple(n for i, n in enumerate(names) if _drawn(f[i:i + 1], S)[0])
    ids, fim = _drawn(f, S)
    together = tuple(names[i] for i in sorted(ids))
    print("alone", alone, "together", together)
    assert alone == rs.DEGENERATE_DRAWN_ALONE
    assert together == rs.DEGENERATE_DRAWN_TOGETHER
    want, _, _ = _winner_from_restatement(f, S)
    assert np.array_equal(want, fim)
    for S2, near, far in ((32, 0.1, 25.0), (32, 1.0, 5.0), (100, 0.1, 100.0), (100, 1.0, 5.0)):
        f2 = rs.degenerate(S2)
        _assert_inside_boxes(f2, S2, _drawn(f2, S2, near, far)[1])


@pytest.mark.parametrize("n,S", [(500, 72), (3000, 100)])
def test_soup_agrees_with_the_independent_fp64_rasterizer(n, S):
    """tests/test_raster_property.py's bounds on random triangle soups (its scenes are the body mesh only)."""
    f = rs.soup(n)
    culled = float((rs.signed_area2(f) < 0).mean())
    assert 0.4 < culled < 0.6
    fim32, _ = _oracle(f, S)
    fim64, _, margin = _fp64_rasterize(f.astype(np.float64), S)
    clear = margin > 1e-6
    agree = float((fim32[clear] == fim64[clear]).mean())
    print(n, S, "clear", float(clear.mean()), "agree on clear", agree, "cover", float((fim64 >= 0).mean()))
    assert clear.mean() > 0.95
    assert agree >= 0.999
    assert ((fim32 >= 0) == (fim64 >= 0))[clear].all()
    assert 0.05 < (fim64 >= 0).mean() < 0.98
    _assert_inside_boxes(f, S, fim32)


@pytest.mark.parametrize("S", [48, 100])
def test_snapped_soup_has_edge_hits_and_ties(S):
    f = rs.snapped_soup(3000, S)
    fim, wim = _oracle(f, S)
    if S == 48:
        want, _, zp = _winner_from_restatement(f, S)
        assert np.array_equal(want, fim)
        two = np.sort(zp, axis=0)[:2]
        tie = np.isfinite(two[0]) & (two[0].view(np.int32) == two[1].view(np.int32))
        print("snapped soup tie pixels", int(tie.sum()))
        assert tie.sum() >= 20
    on = wim[fim >= 0]
    assert (on == 0).any(axis=1).sum() >= 50                    # centres exactly on edges
    assert (rs.signed_area2(f) == 0).sum() >= 20                # faces collapsed to segments / points
    _assert_inside_boxes(f, S, fim)
