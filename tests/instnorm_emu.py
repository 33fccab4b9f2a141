"""InstanceNorm statistics (csrc/norm.hip) restated in numpy with every operation rounded to float32, the ill-conditioned data families
the statistics are tested on, and the error bounds both the emulation (tests/test_instnorm_cpu.py) and the kernels
(tests/test_gpu_instnorm.py) have to meet against float64 statistics of the same float32 values.

The algorithm: an image's HW pixels are cut into nsplit splits of per = ceil(HW / nsplit) pixels (the last ones may be short or empty).
Per split and channel, shift = the split's first pixel; PG thread groups each sum d = x - shift and d^2 over the pixels p0 + pg,
p0 + pg + PG, ...; the PG partials are added in index order; the record is (n, shift + t1 / n, max(t2 - t1^2 / n, 0)).  Lane s % 64 of
the final wave merges its records serially (Chan's update), then a six-round shuffle tree merges the 64 lanes.

Bounds, per (image, channel), with u = 2^-24, A = max |x|, rho = 1 / sqrt(var + eps), T = ceil(per / PG) + PG + ceil(nsplit / 64) + 6 (the
longest chain of dependent additions) and kappa = max over the non-empty splits of (x[p0_s] - mean_s)^2 / (var_s + eps):
    |mean - mu|      <= 16 u A
    |rstd / rho - 1| <= 2 u (8 + |mu| / sqrt(var + eps) + T (1 + kappa))
(final roundings; record means stored in float32 at magnitude |mu|; a sum of n terms of size var + delta^2, delta = the distance from
the shift to the split's mean).  A constant channel must give its mean exactly and rstd within 4 u of 1 / sqrt(eps)."""
import numpy as np

U = 2.0 ** -24
F32 = np.float32
FAMILIES = ("n01", "1000+n", "100+0.01n", "1e-3n", "1e3n", "zero", "const1000.25", "relu(n-2)", "outlier_shift", "spike")
SPIKE = FAMILIES.index("spike")
# (B, HW, nsplit) of the statistics tests; (1, 640, 130) runs the serial pre-merge of the final pass and is fp32 only (bf16 takes <= 64 splits)
GEOMETRIES = ((2, 35, 8), (2, 63, 64), (1, 1, 1), (3, 1000, 3), (2, 4160, 64), (1, 16384, 64), (1, 640, 130), (2, 9216, 64))


def split_ranges(HW, nsplit):
    per = -(-HW // nsplit)
    return per, [(s * per, min(HW, s * per + per)) for s in range(nsplit)]


def chain_length(HW, nsplit, PG):
    per = -(-HW // nsplit)
    return -(-per // PG) + PG + -(-nsplit // 64) + 6


def probe_pixels(HW, nsplit, PG):
    """Where a dropped or doubled pixel of the partial pass would hide: both ends of the first, a middle and the last non-empty split, the
    last pixel of the first pixel group and the first of the second, the same around the four-iterations-in-flight boundary, and the image's ends."""
    _, rng = split_ranges(HW, nsplit)
    full = [r for r in rng if r[0] < r[1]]
    out = []
    for p0, p1 in (full[0], full[len(full) // 2], full[-1]):
        out += [p for p in (p0, p1 - 1, p0 + PG - 1, p0 + PG, p0 + 4 * PG - 1, p0 + 4 * PG) if p0 <= p < p1]
    out += [0, HW - 1]
    return list(dict.fromkeys(out))


def family_of(b, C):
    """Family index of every channel of image b: the families cycle over the channels, starting 4 further per image (so that C = 4 meets 8)."""
    return (np.arange(C) + 4 * b) % len(FAMILIES)


def make_data(B, HW, C, nsplit, PG, seed):
    """(B, HW, C) float32, one family per channel, another seed per image -> (x, fam (B, C), probe (B, C): the spike's pixel or -1)."""
    x = np.empty((B, HW, C), dtype=F32)
    fam = np.stack([family_of(b, C) for b in range(B)])
    probe = np.full((B, C), -1, dtype=np.int64)
    probes = probe_pixels(HW, nsplit, PG)
    k = 0
    for b in range(B):
        g = np.random.default_rng([seed, b, HW, C]).standard_normal((HW, C), dtype=F32).astype(np.float64)
        f = fam[b][None, :]
        v = np.select([f == 0, f == 1, f == 2, f == 3, f == 4, f == 5, f == 6, f == 7, f == 8],
                      [g, 1000 + g, 100 + 0.01 * g, 1e-3 * g, 1e3 * g, 0 * g, 0 * g + 1000.25, np.maximum(g - 2, 0), g], 0.0)
        v[0, fam[b] == 8] = 1e4                                  # the shift pixel of the first split is an outlier
        for c in np.nonzero(fam[b] == SPIKE)[0]:
            probe[b, c] = probes[k % len(probes)]
            v[probe[b, c], c] = 64.0
            k += 1
        x[b] = v.astype(F32)
    return x, fam, probe


# ---------------------------------------------------------------------------------------------------------------- emulation
def partial_emu(x, nsplit, PG, variant=None):
    """x (HW, C) float32 -> the records (n (nsplit,), mean (nsplit, C), M2 (nsplit, C)) of pass 1, float32 throughout.
    variant: None = the documented algorithm; "onepass" = no shift (M2 = sum x^2 - (sum x)^2 / n, the cancellation the shift avoids);
    "drop_tail" = the loop after the four-in-flight iterations stops one pixel short of the split's end."""
    assert x.dtype == F32 and variant in (None, "onepass", "drop_tail")
    HW, C = x.shape
    per, rng = split_ranges(HW, nsplit)
    p0, p1 = np.array([r[0] for r in rng]), np.array([r[1] for r in rng])
    full = p0 < p1
    shift = np.zeros((nsplit, C), dtype=F32)
    if variant != "onepass":
        shift[full] = x[p0[full]]
    s1, s2 = np.zeros((nsplit, PG, C), dtype=F32), np.zeros((nsplit, PG, C), dtype=F32)
    n = np.zeros((nsplit, PG), dtype=np.int64)
    pg = np.arange(PG)
    for k in range(-(-per // PG)):
        p = p0[:, None] + pg[None, :] + k * PG
        valid = p < p1[:, None]
        if variant == "drop_tail":
            in_flight = p0[:, None] + pg[None, :] + (k // 4) * 4 * PG + 3 * PG < p1[:, None]
            valid = np.where(in_flight, valid, p < p1[:, None] - 1)
        d = x[np.minimum(p, HW - 1)] - shift[:, None, :]
        s1 = np.where(valid[..., None], s1 + d, s1)
        s2 = np.where(valid[..., None], s2 + d * d, s2)
        n += valid
    t1, t2 = np.zeros((nsplit, C), dtype=F32), np.zeros((nsplit, C), dtype=F32)
    for g in range(PG):                                          # the PG partials, added in index order
        t1, t2 = t1 + s1[:, g], t2 + s2[:, g]
    tn = n.sum(1).astype(F32)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(tn > 0, shift + t1 / tn, shift)
        m2 = np.where(tn > 0, t2 - t1 * t1 / tn, F32(0))
    return tn[:, 0], mean.astype(F32), np.maximum(m2, F32(0)).astype(F32)


def _chan(n, mu, m2, nb, mub, m2b):
    """Chan's update of (n, mu, m2) by the record (nb, mub, m2b) where nb > 0, operation by operation as lwg_in_stats_final writes it."""
    with np.errstate(divide="ignore", invalid="ignore"):
        tot = n + nb
        delta = mub - mu
        r = nb / tot
        mu2 = mu + delta * r
        m22 = m2 + (m2b + delta * delta * (n * r))
    on = nb > 0
    return np.where(on, tot, n), np.where(on, mu2, mu), np.where(on, m22, m2)


def final_emu(rn, rmean, rm2, eps):
    """Pass 2: lane s % 64 merges its records serially, then the six-round shuffle tree (lane i takes lane i + off) -> mean, rstd (C,)."""
    nsplit, C = rmean.shape
    n, mu, m2 = (np.zeros((64, C), dtype=F32) for _ in range(3))
    for j in range(-(-nsplit // 64)):
        m = min(64, nsplit - 64 * j)
        nb, mub, m2b = (np.zeros((64, C), dtype=F32) for _ in range(3))
        nb[:m], mub[:m], m2b[:m] = rn[64 * j:64 * j + m, None], rmean[64 * j:64 * j + m], rm2[64 * j:64 * j + m]
        n, mu, m2 = _chan(n, mu, m2, nb, mub, m2b)
    off = 32
    while off >= 1:
        n[:off], mu[:off], m2[:off] = _chan(n[:off], mu[:off], m2[:off], n[off:2 * off], mu[off:2 * off], m2[off:2 * off])
        off //= 2
    with np.errstate(divide="ignore", invalid="ignore"):        # n = 0 only in a broken variant that drops every pixel: NaN, as on the device
        return mu[0].astype(F32), (F32(1) / np.sqrt(m2[0] / n[0] + F32(eps))).astype(F32)


def stats_emu(x, nsplit, PG, eps, variant=None):
    """x (B, HW, C) float32 -> mean, rstd (B, C) float32 as the kernels of csrc/norm.hip compute them (up to fused multiply-adds)."""
    out = [final_emu(*partial_emu(xb, nsplit, PG, variant), eps) for xb in x]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---------------------------------------------------------------------------------------------------------------- reference and bounds
def reference(x, nsplit, PG, eps):
    """float64 statistics of the float32 (or bf16-rounded) values x (B, HW, C) and the bounds of the module docstring, all (B, C)."""
    B, HW, C = x.shape
    x64 = x.astype(np.float64)
    mu, var, A = x64.mean(1), x64.var(1), np.abs(x64).max(1)
    _, rng = split_ranges(HW, nsplit)
    kappa = np.zeros((B, C))
    for p0, p1 in rng:
        if p0 < p1:
            xs = x64[:, p0:p1]
            kappa = np.maximum(kappa, (xs[:, 0] - xs.mean(1)) ** 2 / (xs.var(1) + eps))
    T = chain_length(HW, nsplit, PG)
    return {"mu": mu, "rho": 1 / np.sqrt(var + eps), "const": x64.min(1) == x64.max(1), "mean_bound": 16 * U * A,
            "rstd_bound": 2 * U * (8 + np.abs(mu) / np.sqrt(var + eps) + T * (1 + kappa))}


def ratios(mean, rstd, ref):
    """error / bound per (image, channel) for the mean and rstd (0 / 0 = 0: an exact mean under a zero bound)."""
    em, er = np.abs(mean.astype(np.float64) - ref["mu"]), np.abs(rstd.astype(np.float64) / ref["rho"] - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rm = np.where(em == 0, 0.0, em / ref["mean_bound"])
    return rm, er / ref["rstd_bound"]


def violations(mean, rstd, ref, eps):
    """The (image, channel) pairs that break a bound: over the mean's, over rstd's, non-finite, or a constant channel that is not exact."""
    rm, rr = ratios(mean, rstd, ref)
    bad = ~np.isfinite(mean) | ~np.isfinite(rstd) | ~(rm <= 1) | ~(rr <= 1)
    c = ref["const"]
    bad |= c & ((mean.astype(np.float64) != ref["mu"]) | ~(np.abs(rstd.astype(np.float64) * np.sqrt(eps) - 1) <= 4 * U))
    return bad


def assert_bounds(mean, rstd, ref, eps, fam, what):
    bad = violations(mean, rstd, ref, eps)
    if bad.any():
        rm, rr = ratios(mean, rstd, ref)
        b, c = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} (image, channel) pairs out of bounds, first image {b} channel {c} ({FAMILIES[fam[b, c]]}): "
                             f"mean {mean[b, c]!r} against {ref['mu'][b, c]!r} (error / bound {rm[b, c]:.3g}), "
                             f"rstd {rstd[b, c]!r} against {ref['rho'][b, c]!r} (error / bound {rr[b, c]:.3g})")


def worst_by_family(mean, rstd, ref, fam):
    """{family: (worst mean error / bound, worst rstd error / bound)} over the channels of each family present."""
    rm, rr = ratios(mean, rstd, ref)
    return {FAMILIES[f]: (float(rm[fam == f].max()), float(rr[fam == f].max())) for f in np.unique(fam)}
