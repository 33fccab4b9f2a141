"""lwg_raster_tiles_kernel (csrc/raster.hip) and the consumers of its maps (csrc/flow.hip, lwg_texture_sample_kernel) on the synthetic scenes of
tests/raster_scenes.py: the hit list's flushes, exact depth ties, pixel centres on edges and vertices, faces that are no triangles, depth planes,
batches of different frames, a dirty workspace.  fim and wim must equal oracle/raster_oracle.c bit for bit (check_raster's bound: the same
arithmetic in the same order on both sides).  tests/test_raster_scenes_cpu.py pins that each scene meets the condition it was built for."""
import functools

import numpy as np
import pytest
import torch

from ipercore_amd import _lib, ops
from tests import emu_ops
from tests import raster_scenes as rs
from tests.gpu_checks import DEV, _cmp

pytestmark = pytest.mark.gpu

_BUILD = {
    "full96": lambda S: rs.full_stack(96), "full600": lambda S: rs.full_stack(600), "half96": lambda S: rs.half_stack(96),
    "ties": lambda S: rs.ties(),
    "lattice_const": lambda S: rs.lattice(S, z="const")[0], "lattice_vertex": lambda S: rs.lattice(S, z="vertex")[0],
    "lattice2_const": lambda S: rs.lattice(S, z="const", layers=2)[0], "lattice2_vertex": lambda S: rs.lattice(S, z="vertex", layers=2)[0],
    "degenerate": rs.degenerate, "soup500": lambda S: rs.soup(500), "soup3000": lambda S: rs.soup(3000),
    "snapped3000": lambda S: rs.snapped_soup(3000, S),
}


@functools.lru_cache(maxsize=None)
def _scene(name, S):
    f = _BUILD[name](S)
    assert f.dtype == np.float32 and f.shape[1:] == (3, 3) and f.shape[0] <= 4000 and S <= 128
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _want(name, S, near=0.1, far=100.0):
    """The oracle's maps of one scene, computed once and shared (never modified)."""
    from oracle import lwg_oracle as orc
    fim, wim = orc.rasterize_fim_wim(_scene(name, S)[None], S, near, far)
    return fim[0], wim[0]


def _gpu(faces, S, near=0.1, far=100.0):
    """faces (nf,3,3) or (B,nf,3,3) numpy -> fim, wim on the CPU."""
    fv = torch.tensor(np.ascontiguousarray(faces if faces.ndim == 4 else faces[None]), device=DEV)
    fim, wim = ops.rasterize_fim_wim(fv, S, near, far)
    torch.cuda.synchronize()
    return (fim.cpu(), wim.cpu()) if faces.ndim == 4 else (fim[0].cpu(), wim[0].cpu())


def _same(got, want, what):
    fim, wim = got
    nd = int((fim != want[0]).sum())
    assert torch.equal(fim, want[0]), f"{what}: {nd} face ids differ from the oracle's"
    assert torch.equal(wim, want[1]), f"{what}: weights differ from the oracle's, max |d| {(wim - want[1]).abs().max().item():.3e}"


# the smallest S at which each scene meets its condition (S = 32: one bin, full tiles), and sizes with partial tiles (72, 100) and partial
# bins (48, 72, 100)
_CASES = [("full96", 32), ("full96", 72), ("full600", 32), ("full600", 100), ("half96", 32), ("half96", 48), ("ties", 32), ("ties", 100),
          ("lattice_const", 32), ("lattice_const", 72), ("lattice_vertex", 32), ("lattice_vertex", 48), ("lattice_vertex", 100),
          ("lattice2_const", 48), ("lattice2_vertex", 72), ("degenerate", 32), ("degenerate", 48), ("degenerate", 72), ("degenerate", 100),
          ("soup500", 48), ("soup500", 72), ("soup3000", 32), ("soup3000", 100), ("snapped3000", 48), ("snapped3000", 72), ("snapped3000", 100)]


@pytest.mark.parametrize("name,S", _CASES)
def test_scene_equals_oracle(name, S):
    want = _want(name, S)
    _same(_gpu(_scene(name, S), S), want, f"{name} S={S}")
    if name == "full600":
        assert (want[0] == 307).all()
    if name == "ties":
        on = set(np.unique(want[0].numpy()).tolist())
        assert {min(g) for g in rs.TIE_GROUPS} <= on and not on & {i for g in rs.TIE_GROUPS for i in g if i != min(g)}
    if name == "degenerate" and S == 32:
        drawn = tuple(rs.DEGENERATE_NAMES[i] for i in np.unique(want[0].numpy()) if i >= 0)
        assert drawn == rs.DEGENERATE_DRAWN_TOGETHER, drawn


@pytest.mark.parametrize("near,far", [(0.1, 25.0), (1.0, 5.0)])
@pytest.mark.parametrize("name,S", [("degenerate", 32), ("degenerate", 100), ("soup500", 72), ("soup3000", 100), ("snapped3000", 48)])
def test_depth_planes(name, S, near, far):
    """far = 25 is what the renderer passes; (1, 5) cuts through the soups' z in [0.6, 6] and the degenerate scene's faces."""
    want = _want(name, S, near, far)
    _same(_gpu(_scene(name, S), S, near, far), want, f"{name} S={S} near={near} far={far}")
    if (near, far) == (1.0, 5.0) and name != "degenerate":
        assert not torch.equal(want[0], _want(name, S)[0]), "the planes cut nothing"


def test_degenerate_faces_alone():
    """Each face of the degenerate scene as a scene of its own (nf = 1), all of them in one batch: what draws is what the oracle draws."""
    S = 32
    f = _scene("degenerate", S)
    from oracle import lwg_oracle as orc
    want = orc.rasterize_fim_wim(f[:, None], S)
    _same(_gpu(f[:, None], S), want, "degenerate faces alone")
    drawn = tuple(n for i, n in enumerate(rs.DEGENERATE_NAMES) if (want[0][i] >= 0).any())
    assert drawn == rs.DEGENERATE_DRAWN_ALONE, drawn


@pytest.mark.parametrize("nf,S,names", [(768, 48, ("full96", "ties", "soup500")), (977, 72, ("half96", "ties", "lattice_vertex")),
                                         (3001, 100, ("snapped3000", "full600", "degenerate")), (1, 48, None)])
def test_batch_independence(nf, S, names):
    """B = 3 different frames in one launch = each frame launched alone, bit for bit (and = the oracle): nf a multiple of the 256-face setup block,
    not a multiple, and a single face."""
    if names is None:
        faces = [rs.full_stack(96)[55:56], rs.BACK_FACE[None], rs.ties()[5:6]]      # the whole image, nothing, one quadrant
    else:
        faces = [rs.pad_back(_scene(n, S), nf) for n in names]
    batch = np.stack(faces)
    assert batch.shape == (3, nf, 3, 3)
    fim, wim = _gpu(batch, S)
    assert len({fim[b].numpy().tobytes() for b in range(3)}) == 3, "the frames of the batch do not differ"
    from oracle import lwg_oracle as orc
    for b in range(3):
        one = _gpu(faces[b], S)
        assert torch.equal(fim[b], one[0]) and torch.equal(wim[b], one[1]), f"frame {b} depends on its batch"
        want = _want(names[b], S) if names is not None else tuple(t[0] for t in orc.rasterize_fim_wim(faces[b][None], S))
        _same((fim[b], wim[b]), want, f"batched frame {b}")


def _raster_ws(faces, S, ws, near=0.1, far=100.0):
    fv = torch.tensor(np.ascontiguousarray(faces[None]), device=DEV)
    nf = fv.shape[1]
    assert ws.numel() >= _lib.lib().lwg_rasterize_ws_bytes(1, nf, S)
    fim = torch.full((1, S, S), -7, device=DEV, dtype=torch.int32)
    wim = torch.full((1, S, S, 3), float("nan"), device=DEV)
    _lib.check(_lib.lib().lwg_rasterize_fim_wim_f32(ops._ptr(fv), 1, nf, S, near, far, ops._ptr(fim, torch.int32), ops._ptr(wim), ws.data_ptr(),
                                                    ops._stream()), "lwg_rasterize_fim_wim_f32")
    torch.cuda.synchronize()
    return fim[0].cpu(), wim[0].cpu()


def test_stale_workspace():
    """A caller's workspace full of 0xFF bytes (bin counts of -1, face ids of -1), then the same workspace straight after a dense scene, for a
    scene of the same nf (the same layout: stale lists in place) and for a smaller one (another layout over the old bytes)."""
    S = 72
    dense, sparse, small = rs.pad_back(_scene("full600", S), 3000), _scene("soup3000", S), _scene("soup500", S)
    ws = torch.full((int(_lib.lib().lwg_rasterize_ws_bytes(1, 3000, S)),), 0xFF, device=DEV, dtype=torch.uint8)
    _same(_raster_ws(sparse, S, ws), _want("soup3000", S), "soup3000 on a workspace of 0xFF bytes")
    _same(_raster_ws(dense, S, ws), _want("full600", S), "full600")
    _same(_raster_ws(sparse, S, ws), _want("soup3000", S), "soup3000 after a dense scene")
    _same(_raster_ws(dense, S, ws), _want("full600", S), "full600 again")
    _same(_raster_ws(small, S, ws), _want("soup500", S), "soup500 after a dense scene of another nf")


def test_stack_determinism():
    """One comparison, not a stress loop: each stack scene launched twice gives the same bits."""
    for name, S in (("full96", 32), ("full600", 100), ("half96", 32)):
        a, b = _gpu(_scene(name, S), S), _gpu(_scene(name, S), S)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name


# ------------------------------------------------------------------------------------------------------------------ consumers of the maps
def _tables(nf, ns, Hu, Wu, seed):
    """Synthetic tables sized to the scene.  f_uvs2img / src_f2pts rows: random in [-1, 1]; every 7th face constant on a texel BORDER of the
    Hu x Wu image, every 11th constant on a texel centre, every 13th at +-1 exactly, every 17th outside [-1, 1]."""
    r = np.random.RandomState(seed)
    map_fn = r.uniform(0, 1, size=(nf + 1, 3)).astype(np.float32)
    map_fn[nf] = (0.25, 0.5, 0.75)                                     # the background row, next to face nf - 1
    t = r.uniform(-1, 1, size=(ns + 1, nf, 3, 2))
    k = np.arange(nf)
    border = np.stack([(2.0 * (k % Wu) + 2) / Wu - 1, (2.0 * (k % Hu) + 2) / Hu - 1], axis=1)
    centre = np.stack([(2.0 * (k % Wu) + 1) / Wu - 1, (2.0 * (k % Hu) + 1) / Hu - 1], axis=1)
    for tab in t:
        tab[k % 7 == 0] = border[k % 7 == 0][:, None, :]
        tab[k % 11 == 0] = centre[k % 11 == 0][:, None, :]
        tab[k % 13 == 0] = np.where(r.uniform(size=(nf, 3, 2)) < 0.5, -1.0, 1.0)[k % 13 == 0]
        tab[k % 17 == 0] = r.uniform(1.0, 1.6, size=(nf, 3, 2))[k % 17 == 0] * np.where(r.uniform(size=(nf, 1, 1)) < 0.5, -1.0, 1.0)[k % 17 == 0]
    uv4 = np.zeros((Hu, Wu, 4), dtype=np.float32)
    uv4[..., :3] = r.uniform(-1, 1, size=(Hu, Wu, 3))
    return torch.tensor(map_fn), torch.tensor(t[0].astype(np.float32)), torch.tensor(t[1:].astype(np.float32)), torch.tensor(uv4)


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("name,S", [("lattice_vertex", 48), ("soup3000", 100), ("ties", 32)])
def test_flow_consumers_on_scene_maps(name, S, ns):
    """ops.flow_compose / bc_transform / encode_fim against tests/emu_ops on the oracle's maps of the scenes, with tables sized to the scene
    (nf != 13776, Hu != Wu, the last face id next to the background row): check_flows' bounds - flows 1e-6, tsf 1e-4, cond an exact gather, the
    -2 sentinel at the same pixels."""
    fim, wim = _want(name, S)
    fim2, wim2 = _want(name, S, 1.0, 5.0)
    fim, wim = torch.stack([fim, fim2]), torch.stack([wim, wim2])       # B = 2 frames that differ
    nf = _scene(name, S).shape[0]
    if name == "lattice_vertex":
        assert int(fim.max()) == nf - 1 and int(fim.min()) == -1         # the last face sits next to the background row
        assert ((wim == 1).any(-1) & (fim >= 0)).sum() > 50              # weights of exactly 1: flows exactly on the table's texel borders
    Hu, Wu = 24, 40
    map_fn, fu, src, uv4 = _tables(nf, ns, Hu, Wu, 70 + ns)
    w_tsf, w_T, w_cond, w_tuv = emu_ops.flow_compose(fim, wim, map_fn, fu, uv4, src, True, True)
    fd, wd = fim.to(DEV), wim.to(DEV)
    g_tsf, g_T, g_cond, g_tuv = ops.flow_compose(fd, wd, map_fn.to(DEV), fu.to(DEV), uv4.to(DEV), src.to(DEV), True, True)
    torch.cuda.synchronize()
    assert tuple(g_T.shape) == (2, ns, S, S, 2)
    _cmp(g_T, w_T, 1e-6, "Tst")
    _cmp(g_tuv, w_tuv, 1e-6, "Tuv")
    _cmp(g_tsf, w_tsf, 1e-4, "tsf_inputs")
    assert torch.equal(g_cond.cpu(), w_cond), "cond (encode_fim) must be an exact gather"
    assert torch.equal(g_tsf[..., 3:6].cpu(), w_tsf[..., 3:6]) and (g_tsf[..., 6:] == 0).all()
    assert torch.equal(g_T.cpu() == -2, w_T == -2) and torch.equal(g_tuv.cpu() == -2, w_tuv == -2), "background sentinel positions differ"
    assert float(w_T[w_T != -2].abs().max()) > 1.0 and (w_T == -2).any()      # flows outside [-1, 1] and the sentinel both occur
    f2 = torch.stack([src[0], fu])                                       # per-frame tables for the generic transform
    _cmp(ops.bc_transform(f2.to(DEV), fd, wd), emu_ops.bc_transform(f2, fim, wim), 1e-6, "bc_transform")
    assert torch.equal(ops.encode_fim(fd, map_fn.to(DEV)).cpu(), emu_ops.encode_fim(fim, map_fn))
    wide = torch.tensor(np.random.RandomState(5).uniform(size=(nf + 1, 5)).astype(np.float32))      # D != 3
    assert torch.equal(ops.encode_fim(fd, wide.to(DEV)).cpu(), emu_ops.encode_fim(fim, wide))


@pytest.mark.parametrize("T", [1, 2, 4, 6])
def test_texture_sample_on_scene_maps(T):
    """ops.texture_sample against tests/emu_ops at check_textured_render's 2e-5: texture sizes other than 3, textures per frame and shared, a
    non-zero background colour, on the maps of the lattice (weights of exactly 0 and 1) and soup scenes."""
    S = 48
    nf = 500
    faces = np.stack([rs.pad_back(_scene("lattice_vertex", S), nf), _scene("soup500", S)])
    assert _scene("lattice_vertex", S).shape[0] <= nf
    fim = torch.stack([_want("lattice_vertex", S)[0], _want("soup500", S)[0]])
    wim = torch.stack([_want("lattice_vertex", S)[1], _want("soup500", S)[1]])
    assert ((wim[0] == 1).any(-1)).sum() > 50 and ((wim[0] == 0).any(-1) & (fim[0] >= 0)).sum() > 200
    fv = torch.tensor(faces)
    bg = (0.25, -0.5, 1.0)
    for shared in (False, True):
        tex = torch.tensor(np.random.RandomState(90 + T).uniform(-1, 1, size=(1 if shared else 2, nf, T, T, T, 3)).astype(np.float32))
        want = emu_ops.texture_sample(fim, wim, fv, tex, 1e-3, bg)
        got = ops.texture_sample(fim.to(DEV), wim.to(DEV), fv.to(DEV), tex.to(DEV), 1e-3, bg)
        torch.cuda.synchronize()
        _cmp(got, want, 2e-5, f"texture_sample T={T} shared={shared}")
        off = fim < 0
        assert off.any() and torch.equal(got.cpu()[off], torch.tensor(bg).expand(int(off.sum()), 3))
