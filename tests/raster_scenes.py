"""Seeded synthetic scenes for the rasterizer (csrc/raster.hip against oracle/raster_oracle.c), numpy only.  Every builder returns (nf, 3, 3)
fp32 faces, per vertex (x, y, z) in the rasterizer's input space (y up), in their final winding: what the oracle's rule
(y2 - y0)(x1 - x0) >= (y1 - y0)(x2 - x0) keeps is meant to be drawn, what it culls is meant to be culled.  The scenes aim at what the body
mesh never does: tens of faces over one pixel (the hit list's flushes), bit-equal depths (the tie rule), pixel centres exactly on edges and
vertices, faces that are no triangles at all, and faces across the image border and the depth planes.

Shared by tests/test_raster_scenes_cpu.py (which pins, on the oracle alone, the condition each scene is built for) and
tests/test_gpu_raster_scenes.py (kernel == oracle, bit for bit).  `cover_and_depth` restates the oracle's per-face arithmetic in numpy fp32
(one rounding per operation, as the C file built with contraction off) so the CPU test can count hits and depth ties per pixel."""
import numpy as np

BACK_FACE = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 1.0], [1.0, 0.0, 1.0]], dtype=np.float32)      # culled by the oracle's rule: padding


def centre(c, S):
    """NDC coordinate of pixel-centre index c (fractions allowed) with the kernel's own expression, evaluated in fp64."""
    return (2.0 * np.asarray(c, dtype=np.float64) + 1 - S) / S


def signed_area2(f):
    """(y2 - y0)(x1 - x0) - (y1 - y0)(x2 - x0) in fp64: > 0 is front-facing."""
    f = np.asarray(f, dtype=np.float64)
    return (f[..., 2, 1] - f[..., 0, 1]) * (f[..., 1, 0] - f[..., 0, 0]) - (f[..., 1, 1] - f[..., 0, 1]) * (f[..., 2, 0] - f[..., 0, 0])


def _front(f):
    """Swap v1 and v2 of the faces whose winding the oracle would cull."""
    f = np.array(f, dtype=np.float64)
    back = signed_area2(f) < 0
    f[back] = f[back][:, [0, 2, 1]]
    return f


def pad_back(faces, nf):
    """The scene padded to nf faces with back-facing ones (for batches of scenes of different sizes)."""
    assert faces.shape[0] <= nf
    return np.concatenate([faces, np.broadcast_to(BACK_FACE, (nf - faces.shape[0], 3, 3))]).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ stacks
def full_stack(n, seed=0):
    """n triangles that each cover the whole image, at distinct depths 1 + 0.01 k in shuffled order; the nearest one sits at id n // 2 + 7."""
    r = np.random.RandomState(1000 + seed)
    base = np.array([[-4.0, -2.0], [4.0, -2.0], [0.0, 4.0]])
    order = r.permutation(n)
    w, at = int(np.nonzero(order == 0)[0][0]), n // 2 + 7
    order[w], order[at] = order[at], order[w]
    f = np.zeros((n, 3, 3))
    f[:, :, :2] = base[None] + r.uniform(-0.3, 0.3, size=(n, 3, 2))
    f[:, :, 2] = 1.0 + 0.01 * order[:, None] + r.uniform(-0.002, 0.002, size=(n, 3))
    return _front(f).astype(np.float32)


def _coverage_per_tile(f, S=32):
    """Fraction of each 16 x 16 tile's pixel centres inside the triangle f (3,3) (fp64, inclusive edges)."""
    c = centre(np.arange(S), S)
    px, py = np.meshgrid(c, c[::-1])
    inside = np.ones((S, S), dtype=bool)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        inside &= ~((py - f[a, 1]) * (f[b, 0] - f[a, 0]) < (px - f[a, 0]) * (f[b, 1] - f[a, 1]))
    t = S // 16
    return inside.reshape(t, 16, t, 16).mean(axis=(1, 3))


def half_stack(n=96, seed=0):
    """n rotated triangles around the image centre, each covering 35-65 % of every 16 x 16 tile at S = 32 (rejection-sampled), depths as in
    full_stack: a group of 32 candidates adds about half of 256 * 32 hits, so the list crosses its threshold only every second group or so."""
    r = np.random.RandomState(2000 + seed)
    out = []
    while len(out) < n:
        ang = r.uniform(0, 2 * np.pi) + np.array([0.0, 2 * np.pi / 3, 4 * np.pi / 3]) + r.uniform(-0.25, 0.25, size=3)
        rad = r.uniform(1.1, 1.9, size=3)
        xy = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1) + r.uniform(-0.15, 0.15, size=2)
        f = _front(np.concatenate([xy, np.ones((3, 1))], axis=1)[None])[0]
        cov = _coverage_per_tile(f)
        if cov.min() >= 0.35 and cov.max() <= 0.65:
            out.append(f)
    f = np.stack(out)
    order = r.permutation(n)
    f[:, :, 2] = 1.0 + 0.01 * order[:, None] + r.uniform(-0.002, 0.002, size=(n, 3))
    return f.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ soups
def soup(n, seed=0, centre_range=1.2):
    """n random triangles: size log-uniform in [0.006, 0.3] NDC, centres in +-1.2 (faces straddle every image edge), random winding (half are
    culled), one in five a near-sliver (third vertex almost on the line of the other two), per-vertex z in [0.6, 6] (both sides of the planes (1, 5))."""
    r = np.random.RandomState(3000 + seed)
    size = np.exp(r.uniform(np.log(0.006), np.log(0.3), size=n))
    c = r.uniform(-centre_range, centre_range, size=(n, 2))
    ang = r.uniform(0, 2 * np.pi, size=(n, 1)) + np.sort(r.uniform(0, 2 * np.pi, size=(n, 3)), axis=1)
    xy = c[:, None, :] + size[:, None, None] * r.uniform(0.3, 1.0, size=(n, 3, 1)) * np.stack([np.cos(ang), np.sin(ang)], axis=2)
    sl = r.uniform(size=n) < 0.2
    t = r.uniform(0.1, 0.9, size=(n, 1))
    on_line = xy[:, 0] + t * (xy[:, 1] - xy[:, 0])
    xy[sl, 2] = on_line[sl] + (xy[sl, 2] - on_line[sl]) * 0.01
    flip = r.uniform(size=n) < 0.5
    xy[flip] = xy[flip][:, [0, 2, 1]]
    f = np.concatenate([xy, r.uniform(0.6, 6.0, size=(n, 3, 1))], axis=2)
    return f.astype(np.float32)


def snapped_soup(n, S, seed=0):
    """The soup with vertices snapped to the half-pixel lattice of an S x S image (pixel centres and pixel corners) and one depth per face out of
    four values: edges and vertices through pixel centres, faces collapsed to segments and points, and equal depths, all at once."""
    r = np.random.RandomState(4000 + seed)
    f = soup(n, seed).astype(np.float64)
    pix = (f[:, :, :2] * S + S - 1) / 2
    f[:, :, :2] = centre(np.round(pix * 2) / 2, S)
    f[:, :, 2] = np.array([1.0, 1.5, 2.0, 3.0])[r.randint(0, 4, size=n)][:, None]
    return f.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ ties
TIE_GROUPS = ((5, 6), (300, 290), (100, 101, 450), (3, 700))      # ids that hold the same nine floats; the lowest id must win


def ties(seed=0):
    """720 filler triangles at z in [2, 3] and, nearer, four large triangles (one per image quadrant, per-vertex z in [1, 1.4]) each stored under
    the ids of one TIE_GROUP: adjacent ids, the copy below its original, a three-way tie, and ids 3 and 700 that fall into different
    256-candidate chunks."""
    r = np.random.RandomState(5000 + seed)
    f = _front(soup(720, 77 + seed, centre_range=1.0).astype(np.float64))
    f[:, :, 2] = r.uniform(2.0, 3.0, size=(720, 3))
    for g, (qx, qy) in zip(TIE_GROUPS, ((-0.5, 0.5), (0.5, 0.5), (-0.5, -0.5), (0.5, -0.5))):
        xy = np.array([qx, qy]) + np.array([[-0.42, -0.40], [0.44, -0.33], [-0.05, 0.43]]) + r.uniform(-0.03, 0.03, size=(3, 2))
        tri = _front(np.concatenate([xy, r.uniform(1.0, 1.4, size=(3, 1))], axis=1)[None])[0]
        for i in g:
            f[i] = tri
    return f.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ lattice
def lattice(S, cell=3, z="const", layers=1, seed=0):
    """A triangulated grid whose vertices are the pixel centres 1, 1 + cell, ... of an S x S image: the axis-parallel edges, the diagonals and
    the vertices all pass exactly through pixel centres.  z: "const" (1.5 everywhere) or "vertex" (one random depth in [1, 1.6] per grid vertex,
    shared by the triangles around it).  layers = 2 adds the same grid shifted by half a cell (vertices on pixel corners when cell is odd)
    0.7 behind.  Returns (faces, (lo, hi)): the front layer covers the pixel centres lo..hi inclusive in both directions."""
    r = np.random.RandomState(6000 + seed)
    nc = (S - 4) // cell
    idx = 1 + cell * np.arange(nc + 1)
    zz = np.full((nc + 1, nc + 1), 1.5) if z == "const" else r.uniform(1.0, 1.6, size=(nc + 1, nc + 1))
    out = []
    for layer in range(layers):
        sh, dz = 0.5 * cell * layer, 0.7 * layer
        c = centre(idx + sh, S)
        v = lambda i, j: (c[i], c[j], zz[j, i] + dz)      # noqa: E731  (column i -> x, row j -> y)
        for j in range(nc):
            for i in range(nc):
                if (i + j) % 2 == 0:      # alternate the diagonal so both directions occur
                    out += [[v(i, j), v(i + 1, j), v(i + 1, j + 1)], [v(i, j), v(i + 1, j + 1), v(i, j + 1)]]
                else:
                    out += [[v(i, j), v(i + 1, j), v(i, j + 1)], [v(i + 1, j), v(i + 1, j + 1), v(i, j + 1)]]
    return _front(np.array(out)).astype(np.float32), (int(idx[0]), int(idx[-1]))


# ------------------------------------------------------------------------------------------------------------------ degenerate
DEGENERATE_NAMES = ("backdrop", "point", "collinear_row", "collinear_diagonal", "v0_eq_v1", "v1_eq_v2", "v0_eq_v2", "nan_vertex", "inf_vertex",
                    "needle", "huge_1e6", "nearer_than_near", "beyond_far", "z_zero", "one_z_zero", "z_negative", "straddles_planes", "plain")


def degenerate(S):
    """A backdrop (id 0, the whole image at z = 3) and in front of it one face per DEGENERATE_NAMES entry, each in a slot of its own of a 4 x 4
    layout (pixel-centre aligned for image size S where the name says so).  "plain" is an ordinary triangle: the scene must draw something
    besides the backdrop.  The depth faces use near = 0.1 / far = 100 and stay outside (1, 5) and (0.1, 25) as well."""
    def slot(k):                                   # centre pixel of slot k, snapped to a pixel centre
        sx, sy = k % 4, k // 4
        return np.array([round((sx + 0.5) * S / 4 - 0.5), round((sy + 0.5) * S / 4 - 0.5)], dtype=np.float64)

    def tri(k, offs, z):                           # offsets in pixels around the slot centre
        p = slot(k)[None] + np.asarray(offs, dtype=np.float64)
        return np.concatenate([centre(p, S), np.broadcast_to(np.asarray(z, dtype=np.float64).reshape(-1, 1), (3, 1))], axis=1)

    h = max(2, S // 10)                            # half-size of an ordinary face in pixels
    ordinary = [[-h, -h + 0.3], [h + 0.4, -h], [-0.2, h + 0.3]]
    nan, inf = float("nan"), float("inf")
    f = [np.array([[-4.0, -2.0, 3.0], [4.0, -2.0, 3.0], [0.0, 4.0, 3.0]]),
         tri(0, [[0, 0], [0, 0], [0, 0]], 1.2),
         tri(1, [[-h, 0], [0, 0], [h, 0]], 1.2),
         tri(2, [[-h, -h], [0, 0], [h, h]], 1.2),
         tri(3, [ordinary[0], ordinary[0], ordinary[2]], 1.2),
         tri(4, [ordinary[0], ordinary[1], ordinary[1]], 1.2),
         tri(5, [ordinary[0], ordinary[1], ordinary[0]], 1.2),
         tri(6, ordinary, 1.2), tri(7, ordinary, 1.2),
         tri(8, [[-h, -h], [h, h + 0.02], [h, h]], [1.1, 1.3, 1.2]),
         np.array([[-1e6, -1e6, 2.5], [1e6, 1e6 + 0.5, 2.5], [-1e6, 1e6, 2.5]]),
         tri(9, ordinary, 0.05), tri(10, ordinary, 150.0), tri(11, ordinary, 0.0), tri(12, ordinary, [0.0, 1.2, 1.3]),
         tri(13, ordinary, -1.0), tri(14, ordinary, [0.05, 2.0, 150.0]), tri(15, ordinary, [1.1, 1.25, 1.4])]
    f = _front(np.stack(f))
    f[7, 1, 0] = nan
    f[8, 2, 1] = inf
    assert len(f) == len(DEGENERATE_NAMES)
    return f.astype(np.float32)


# faces of degenerate(32) that own at least one pixel of the oracle's map at near = 0.1, far = 100: each face alone in the scene / all together
# (tests/test_raster_scenes_cpu.py asserts both against the oracle; the GPU test inherits them)
DEGENERATE_DRAWN_ALONE = ("backdrop", "needle", "huge_1e6", "straddles_planes", "plain")
DEGENERATE_DRAWN_TOGETHER = ("backdrop", "needle", "huge_1e6", "straddles_planes", "plain")


# ------------------------------------------------------------------------------------------------------------------ the oracle's arithmetic in numpy
def cover_and_depth(faces, S, near=0.1, far=100.0):
    """faces (nf,3,3) fp32 -> hit (nf,S,S) bool: kept by the back-face rule and the pixel centre passes the three edge tests (what the kernel
    appends to its hit list); zp (nf,S,S) fp32: the oracle's depth there, +inf where the face is not selectable (no hit, NaN, or outside
    (near, far)).  Row 0 is the top of the image.  The oracle's expressions in the oracle's order, one fp32 rounding per operation."""
    f = np.asarray(faces, dtype=np.float32)
    nf = f.shape[0]
    F32 = np.float32
    with np.errstate(all="ignore"):
        keep = ~((f[:, 2, 1] - f[:, 0, 1]) * (f[:, 1, 0] - f[:, 0, 0]) < (f[:, 1, 1] - f[:, 0, 1]) * (f[:, 2, 0] - f[:, 0, 0]))
        xi = np.arange(S)
        yi = S - 1 - np.arange(S)
        xp = ((2.0 * xi + 1 - S) / S).astype(F32)[None, None, :]
        yp = ((2.0 * yi + 1 - S) / S).astype(F32)[None, :, None]
        c = lambda n, d: f[:, n, d][:, None, None]      # noqa: E731
        hit = keep[:, None, None] & np.ones((nf, S, S), dtype=bool)
        for a, b in ((0, 1), (1, 2), (2, 0)):
            hit &= ~((yp - c(a, 1)) * (c(b, 0) - c(a, 0)) < (xp - c(a, 0)) * (c(b, 1) - c(a, 1)))
        p = F32(0.5) * (f[:, :, :2] * F32(S) + F32(S) - F32(1.0))
        P = lambda n, d: p[:, n, d]      # noqa: E731
        den = P(2, 0) * (P(0, 1) - P(1, 1)) + P(0, 0) * (P(1, 1) - P(2, 1)) + P(1, 0) * (P(2, 1) - P(0, 1))
        m = np.stack([P(1, 1) - P(2, 1), P(2, 0) - P(1, 0), P(1, 0) * P(2, 1) - P(2, 0) * P(1, 1),
                      P(2, 1) - P(0, 1), P(0, 0) - P(2, 0), P(2, 0) * P(0, 1) - P(0, 0) * P(2, 1),
                      P(0, 1) - P(1, 1), P(1, 0) - P(0, 0), P(0, 0) * P(1, 1) - P(1, 0) * P(0, 1)], axis=1) / den[:, None]
        fx, fy = xi.astype(F32)[None, None, :], yi.astype(F32)[None, :, None]
        w = []
        for k in range(3):
            wk = m[:, 3 * k, None, None] * fx + m[:, 3 * k + 1, None, None] * fy + m[:, 3 * k + 2, None, None]
            w.append(np.where(wk < 0, F32(0), np.where(wk > 1, F32(1), wk)))      # clamp01 keeps NaN
        ws = w[0] + w[1] + w[2]
        w = [wk / ws for wk in w]
        zp = F32(1.0) / (w[0] / c(0, 2) + w[1] / c(1, 2) + w[2] / c(2, 2))
        ok = hit & ~((zp <= F32(near)) | (F32(far) <= zp)) & (zp < F32(far))
    return hit, np.where(ok, zp, F32(np.inf)).astype(F32)


def kernel_boxes(faces, S):
    """The conservative pixel box lwg_raster_setup_kernel gives each face, restated in numpy fp32: (nf, 4) ints x0, x1, y0, y1 in the kernel's
    y-up pixel coordinates, an empty box (x0 > x1) for a culled face.  The CPU test holds every pixel the oracle gives a face against it."""
    f = np.asarray(faces, dtype=np.float32)
    F32 = np.float32
    with np.errstate(all="ignore"):
        front = ~((f[:, 2, 1] - f[:, 0, 1]) * (f[:, 1, 0] - f[:, 0, 0]) < (f[:, 1, 1] - f[:, 0, 1]) * (f[:, 2, 0] - f[:, 0, 0]))
        p = F32(0.5) * (f[:, :, :2] * F32(S) + F32(S) - F32(1.0))
        fmin = lambda a: np.fmin(np.fmin(a[:, 0], a[:, 1]), a[:, 2])      # noqa: E731  (fminf / fmaxf ignore a NaN operand)
        fmax = lambda a: np.fmax(np.fmax(a[:, 0], a[:, 1]), a[:, 2])      # noqa: E731
        xmin, xmax, ymin, ymax = fmin(p[:, :, 0]), fmax(p[:, :, 0]), fmin(p[:, :, 1]), fmax(p[:, :, 1])
        lim = F32(S) + F32(1)
        ok = front & ~np.isnan(xmin) & ~np.isnan(ymin) & (xmax >= -2) & (ymax >= -2) & (xmin <= lim) & (ymin <= lim)
        x0, x1 = np.fmax(np.floor(xmin) - 1, -1), np.fmin(np.ceil(xmax) + 1, lim)
        y0, y1 = np.fmax(np.floor(ymin) - 1, -1), np.fmin(np.ceil(ymax) + 1, lim)
    box = np.stack([np.where(ok, x0, 1), np.where(ok, x1, 0), np.where(ok, y0, 1), np.where(ok, y1, 0)], axis=1)
    return np.nan_to_num(box, nan=0.0).astype(np.int64)
