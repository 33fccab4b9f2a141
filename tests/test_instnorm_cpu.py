"""The error bounds of the InstanceNorm statistics tests (tests/instnorm_emu.py) on the CPU: the float32 emulation of the documented
algorithm meets them on every geometry, pixel-group width and data family of tests/test_gpu_instnorm.py with a wide margin, and two broken
variants - the one-pass E[x^2] - E[x]^2 form, and a tail loop that stops one pixel short - violate them: the bounds bite."""
import numpy as np
import pytest

from tests import instnorm_emu as emu

EPS = 1e-5
C = 200                     # 20 channels per family and image: every probe pixel of the spike family is used
PGS = (4, 8, 16, 32)        # generic fp32 / fp32 C = 256, bf16 C = 256 / fp32 C = 128, bf16 C = 128 / fp32 C = 64 / bf16 C = 64


def _case(geom, PG):
    B, HW, nsplit = geom
    x, fam, probe = emu.make_data(B, HW, C, nsplit, PG, seed=7)
    return x, fam, probe, emu.reference(x, nsplit, PG, EPS)


@pytest.mark.parametrize("PG", PGS)
@pytest.mark.parametrize("geom", emu.GEOMETRIES, ids=lambda g: "B%d_HW%d_ns%d" % g)
def test_emulation_meets_the_bounds(geom, PG):
    """The algorithm alone stays inside half of every bound on every family, so the kernels' fused multiply-adds have room (the worst is the
    mean of relu(N - 2) at HW 1000, nsplit 3, PG 4: 0.23, a split whose shift pixel is one of the few non-zero ones)."""
    x, fam, _, ref = _case(geom, PG)
    mean, rstd = emu.stats_emu(x, geom[2], PG, EPS)
    emu.assert_bounds(mean, rstd, ref, EPS, fam, f"emulation {geom} PG {PG}")
    worst = emu.worst_by_family(mean, rstd, ref, fam)
    print("EMU", geom, PG, {k: (round(a, 4), round(b, 4)) for k, (a, b) in worst.items()})
    assert max(max(v) for v in worst.values()) <= 0.5, worst


@pytest.mark.parametrize("PG", PGS)
@pytest.mark.parametrize("geom", [g for g in emu.GEOMETRIES if -(-g[1] // g[2]) > 1], ids=lambda g: "B%d_HW%d_ns%d" % g)
def test_one_pass_variance_violates_the_bounds(geom, PG):
    """Without the shift, sum x^2 - (sum x)^2 / n cancels: wherever a split holds more than one pixel, channels of 1000 + N(0,1) and of
    100 + 0.01 N(0,1) leave the bounds (with one pixel per split both forms are exact and Chan's merge does the rest)."""
    x, fam, _, ref = _case(geom, PG)
    mean, rstd = emu.stats_emu(x, geom[2], PG, EPS, variant="onepass")
    bad = emu.violations(mean, rstd, ref, EPS)
    for name in ("1000+n", "100+0.01n"):
        assert bad[fam == emu.FAMILIES.index(name)].any(), f"one-pass variance passes on {name} at {geom} PG {PG}"


@pytest.mark.parametrize("PG", PGS)
@pytest.mark.parametrize("geom", emu.GEOMETRIES, ids=lambda g: "B%d_HW%d_ns%d" % g)
def test_dropped_tail_pixel_violates_the_bounds(geom, PG):
    """A tail loop that stops one pixel early loses the spike at p1 - 1 of every probed split whose length is no multiple of 4 PG (where it
    is one, the tail loop has nothing to do and the variant is the algorithm)."""
    B, HW, nsplit = geom
    x, fam, probe, ref = _case(geom, PG)
    mean, rstd = emu.stats_emu(x, nsplit, PG, EPS, variant="drop_tail")
    bad = emu.violations(mean, rstd, ref, EPS)
    _, rng = emu.split_ranges(HW, nsplit)
    full = [r for r in rng if r[0] < r[1]]
    hit = [p1 - 1 for p0, p1 in (full[0], full[len(full) // 2], full[-1]) if (p1 - p0) % (4 * PG)]
    if not hit:
        assert not bad.any()
        return
    for p in hit:
        sel = (fam == emu.SPIKE) & (probe == p)
        assert sel.any() and bad[sel].all(), f"a dropped pixel {p} passes at {geom} PG {PG}"


def test_outlier_shift_limitation():
    """With the shift pixel an outlier (x[0] = 1e4 in N(0,1)) and ONE split, every d^2 is ~1e8 and the variance's few units drown in the
    roundings of a 4096-term sum of them: up to ~1e-3 relative in rstd, which the kappa term of the bound allows.  At the product's
    nsplit = 64 only the first split is hit and the loss is ~1e-5.  Documented in DESIGN.md 3.2; the shift stays the first pixel."""
    out = {}
    for nsplit in (1, 64):
        x, fam, _ = emu.make_data(1, 4096, C, nsplit, 16, seed=7)
        ref = emu.reference(x, nsplit, 16, EPS)
        mean, rstd = emu.stats_emu(x, nsplit, 16, EPS)
        emu.assert_bounds(mean, rstd, ref, EPS, fam, f"outlier shift nsplit {nsplit}")
        sel = fam == emu.FAMILIES.index("outlier_shift")
        out[nsplit] = float(np.abs(rstd.astype(np.float64) / ref["rho"] - 1)[sel].max())
    print("OUTLIER", out)
    assert out[64] < out[1], out                             # measured: 9.6e-4 with one split, 8.0e-6 with 64
