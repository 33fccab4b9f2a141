"""The attention-warp kernels on adversarial flows and ragged shapes (flow families, operands and references: tests/attn_flows.py;
tests/test_attn_flows_cpu.py shows that the references alone stay inside the bounds used here and that wrong variants do not).

Every kernel is compared with tests/emu_ops.py evaluated in float64 on the values the kernel is handed (bf16: the rounded operands).
Outputs are NaN-filled before each launch, so a pixel the kernel does not write fails.  Failures are collected over the inner loops
(C, src_batched, plain / peaked operands) and asserted once per (family, geometry); the worst error of each kernel is printed.

Which case closes which gap of the old coverage (gpu_checks.check_lwb_attention, check_lwb_attention_x, check_attention_backward):
  backward with src_batched=True and B > 1 (sidx = b * ns + s)       test_backward[*]: always src_batched, B in {2, 3}
  backward's !live tail (gp = total - 1)                              test_backward[*-B2_ns3_S40_9x13] (234 pixels), [*-B2_ns2_S20_7x5], [*-B1_ns2_S6_1x7]
  backward at ns = 8 = MAXS                                           test_backward[*-B1_ns8_S12_12x12]
  lwb_attention_f32 / _kv_f32 on ragged tiles, live lanes next to
  dead ones in the shuffles                                           test_forward[*-B3_ns3_S13_13x13], [*-B2_ns3_S40_9x13], [*-B2_ns2_S20_7x5], [*-B1_ns2_S6_1x7]
  h != w                                                              test_forward / test_backward / test_x_form [*-B2_ns3_S40_9x13], [*-B2_ns2_S20_7x5]
  batch independence of lwb_attention_f32 / _kv_f32                   test_forward[*]: every frame alone is bitwise the frame in its batch
  lwg_lwb_attention_bf16 at kernel level                              test_forward[*]: the "bf16" rows
  x-form wave-uniform skip with one foreground lane / one source      test_x_form[one_per_tile-*], [checker-*], and both at B9_ns2_64x64 (four-wave against sixteen-wave)
  pixel centres, half pixels, the +-1 pixel border band               families lattice, half, border in every test
  all pixels at one texel (the backward's atomics)                    test_backward[collapse-*]
  very large finite flows (the clamp before the int conversion)       [wild-*] (no resize only)
  softmax far from uniform (corr = exp(mrun - mnew))                  the peaked operands of test_forward and test_x_form
  flow resize with h != w, h = 1, upsampling, identity                test_flow_resize[*-B2_ns3_S40_9x13], [*-B1_ns2_S6_1x7], [*-B2_ns2_S5_9x13], the S == h == w shapes"""
import pytest
import torch

from ipercore_amd import _lib, ops
from tests import attn_flows as af
from tests.gpu_checks import DEV, _cmp

pytestmark = pytest.mark.gpu

C_F32, C_BF16 = (32, 64, 128, 256), (64, 128, 256)
TABLE = af.forward_table()
TABLE_IDS = [f"{f}-{af.geom_id(g)}" for f, g in TABLE]
X_TABLE = [(f, g) for g in af.GEOMETRIES for f in af.FAMILIES] + [(f, af.LARGE_X) for f in af.LARGE_X_FAMILIES]
X_IDS = [f"{f}-B{g[0]}_ns{g[1]}_{g[3]}x{g[4]}" for f, g in X_TABLE]
RESIZE_SHAPES = af.GEOMETRIES + ((2, 2, 5, 9, 13),)             # + one upsampling case
RESIZE_TABLE = [(f, g) for g in RESIZE_SHAPES for f in af.FAMILIES if f != "wild"]
BF = torch.bfloat16


def _nan(shape, dtype=torch.float32):
    return torch.full(tuple(shape), float("nan"), device=DEV, dtype=dtype)


def _dev(ts):
    return [t.to(DEV) for t in ts]


class _Worst:
    """Worst error over bound per kernel within one (family, geometry), and the failing cases."""

    def __init__(self, family, gid):
        self.family, self.gid, self.worst, self.bad = family, gid, {}, []

    def add(self, kernel, key, figures):
        """figures: [(name, error, bound)]"""
        ratio = max(e / b if b > 0 else (0.0 if e == 0 else float("inf")) for _, e, b in figures)
        if not ratio <= self.worst.get(kernel, (-1.0,))[0]:
            self.worst[kernel] = (ratio, key, figures)
        if not ratio <= 1.0:
            self.bad.append((kernel, key, [(n, f"{e:.3e}", f"{b:.3e}") for n, e, b in figures]))

    def fail(self, kernel, key, what):
        self.bad.append((kernel, key, what))

    def done(self):
        for kernel, (ratio, key, figures) in sorted(self.worst.items()):
            print(f"ATTNFLOW {kernel} {self.family} {self.gid} worst_at {key} " + " ".join(f"{n} {e:.3e} / {b:.3e}" for n, e, b in figures))
        assert not self.bad, self.bad


def _fwd_figures(got, ref, dt, err32):
    assert got.shape == ref.shape
    emax, emean, ref_max = af.fwd_errors(got.float(), ref)
    bmax, bmean = af.fwd_bound(dt, ref_max, err32)
    return [("max_abs", emax if emax == emax else float("inf"), bmax), ("mean_abs", emean if emean == emean else float("inf"), bmean)]


# ------------------------------------------------------------------------------------------------ q / K / V forward kernels
@pytest.mark.parametrize("family,geom", TABLE, ids=TABLE_IDS)
def test_forward(family, geom):
    """lwg_lwb_attention_f32, lwg_lwb_attention_kv_f32 (C in {32, 64, 128, 256}) and lwg_lwb_attention_bf16 (C in {64, 128, 256}), both
    src_batched settings, plain and peaked operands, against fp64: max_abs <= 1e-4 max(1, ref_max) and mean_abs <= 5e-6 (bf16: 3e-2,
    2e-3), with the in-kernel resize max(that, 4 err32).  Two identical launches and every frame launched alone give the batch's bits."""
    B, ns, S, h, w = geom
    W = _Worst(family, af.geom_id(geom))
    for dt, Cs in (("f32", C_F32), ("bf16", C_BF16)):
        adt = BF if dt == "bf16" else torch.float32
        for C in Cs:
            for batched in (False, True):
                for peaked in (False, True):
                    key = f"C{C}_b{int(batched)}_p{int(peaked)}"
                    (q, Ks, Vs, bk, bv), T, ref, err32 = af.forward_case(family, geom, C, batched, peaked, dt)
                    qd, Kd, Vd, bkd, bvd, Td = _dev((q, Ks, Vs, bk, bv, T))
                    forms = [("attn_" + dt, lambda q_, K_, V_, T_, o_: ops.lwb_attention(q_, K_, V_, bkd, bvd, T_, o_, src_batched=batched))]
                    if dt == "f32":
                        forms.append(("attn_kv_f32", lambda q_, K_, V_, T_, o_: ops.lwb_attention_kv(q_, torch.cat([K_, V_], dim=3), bkd, bvd, T_, o_,
                                                                                                   src_batched=batched)))
                    for kernel, run in forms:
                        got = run(qd, Kd, Vd, Td, _nan((B, h, w, C), adt))
                        again = run(qd, Kd, Vd, Td, _nan((B, h, w, C), adt))
                        torch.cuda.synchronize()
                        W.add(kernel, key, _fwd_figures(got, ref, dt, err32))
                        if not torch.equal(got, again):
                            W.fail(kernel, key, "two identical launches differ")
                        for b in range(B):
                            sl = slice(b * ns, (b + 1) * ns) if batched else slice(None)
                            one = run(qd[b:b + 1], Kd[sl], Vd[sl], Td[b:b + 1].contiguous(), _nan((1, h, w, C), adt))
                            if not torch.equal(one[0], got[b]):
                                W.fail(kernel, key, f"frame {b} alone differs from the frame in its batch")
    W.done()


# ------------------------------------------------------------------------------------------------ x-form
def _x_launch(xd, Kq, kap, Vs, bvd, Td, batched, stats):
    B, h, w, C = xd.shape
    nrec = ops.attn_records(h, w, C, xd.dtype)
    ws = _nan((ops.instnorm_finalize_ws(B, C, nrec),)) if stats else None
    out = ops.lwb_attention_x(xd, Kq, kap, Vs, bvd, Td, _nan((B, h, w, C), xd.dtype), stats=ws, src_batched=batched)
    if not stats:
        return out, None, None
    mean, rstd = _nan((B, C)), _nan((B, C))
    ops.instnorm_finalize(ws, B, C, nrec, mean, rstd)
    return out, mean, rstd


@pytest.mark.parametrize("family,geom", X_TABLE, ids=X_IDS)
def test_x_form(family, geom):
    """lwg_lwb_attention_x_f32 / _bf16 on the (h, w) fields of the geometries (+ 9 frames of 64 x 64 at C = 128: four waves per tile in the
    batch, sixteen for a frame alone) against emu_ops.lwb_attention_x in fp64 under check_lwb_attention_x's bounds; its equalities:
    statistics on / off give the same bits, a frame alone is bitwise the frame in its batch, statistics included; the statistics within
    mean 2e-6, rstd relative 2e-6 of torch's."""
    B, ns, _, h, w = geom
    large = geom == af.LARGE_X
    W = _Worst(family, f"B{B}_ns{ns}_{h}x{w}")
    T = af.flows(family, B, ns, h, w, seed=0)
    Td = T.to(DEV)
    for dt, Cs in (("f32", (128,) if large else C_F32), ("bf16", (128,) if large else C_BF16)):
        for C in Cs:
            for batched in ((False,) if large else (False, True)):
                for peaked in ((False,) if large else (False, True)):
                    key = f"C{C}_b{int(batched)}_p{int(peaked)}"
                    x, Kq, kap, Vs, bv = af.x_operands(af.rs(2, C, B, ns, h, w, int(batched)), B, ns, h, w, C, batched, peaked)
                    x, Kq, Vs = af.store(x, dt), af.store(Kq, dt), af.store(Vs, dt)
                    ref = af.ref_attention_x(x, Kq, kap, Vs, bv, T, batched)
                    xd, Kd, kd, Vd, bvd = _dev((x, Kq, kap, Vs, bv))
                    got, mean, rstd = _x_launch(xd, Kd, kd, Vd, bvd, Td, batched, True)
                    plain, _, _ = _x_launch(xd, Kd, kd, Vd, bvd, Td, batched, False)
                    torch.cuda.synchronize()
                    W.add("attn_x_" + dt, key, _fwd_figures(got, ref, dt, None))
                    v = x.float().reshape(B, h * w, C).double()
                    m_err = (mean.cpu().double() - v.mean(dim=1)).abs().max().item()
                    r_err = ((rstd.cpu().double() * torch.sqrt(v.var(dim=1, unbiased=False) + 1e-5)) - 1).abs().max().item()
                    W.add("attn_x_stats_" + dt, key, [("mean", m_err if m_err == m_err else float("inf"), af.STATS_TOL[0]),
                                                      ("rstd_rel", r_err if r_err == r_err else float("inf"), af.STATS_TOL[1])])
                    if not torch.equal(got, plain):
                        W.fail("attn_x_" + dt, key, "the statistics form changes the output")
                    for b in range(B):
                        sl = slice(b * ns, (b + 1) * ns) if batched else slice(None)
                        one, m1, r1 = _x_launch(xd[b:b + 1], Kd[sl], kd[sl], Vd[sl], bvd, Td[b:b + 1], batched, True)
                        if not (torch.equal(one[0], got[b]) and torch.equal(m1[0], mean[b]) and torch.equal(r1[0], rstd[b])):
                            W.fail("attn_x_" + dt, key, f"frame {b} alone differs from the frame in its batch (output or statistics)")
    W.done()


# ------------------------------------------------------------------------------------------------ backward
def _bwd_launch(q, Ks, Vs, bk, bv, T, dout):
    """lwg_lwb_attention_bwd_f32 itself with a NaN-filled dq (ops.lwb_attention_bwd allocates its own) -> dq, dKs, dVs."""
    B, h, w, C = q.shape
    dq, dK, dV = _nan(q.shape), torch.zeros_like(Ks), torch.zeros_like(Vs)
    _lib.check(_lib.lib().lwg_lwb_attention_bwd_f32(q.data_ptr(), Ks.data_ptr(), Vs.data_ptr(), bk.data_ptr(), bv.data_ptr(), T.data_ptr(), dout.data_ptr(),
                                                     dq.data_ptr(), dK.data_ptr(), dV.data_ptr(), B, T.shape[1], h, w, C, T.shape[2], 1, ops._stream()),
               "lwg_lwb_attention_bwd_f32")
    return dq, dK, dV


def _kv_bwd_launch(q, kv, bk, bv, T, dout):
    B, h, w, C = q.shape
    dq, dkv = _nan(q.shape), torch.zeros_like(kv)
    _lib.check(_lib.lib().lwg_lwb_attention_kv_bwd_f32(q.data_ptr(), kv.data_ptr(), bk.data_ptr(), bv.data_ptr(), T.data_ptr(), dout.data_ptr(), dq.data_ptr(),
                                                        dkv.data_ptr(), B, T.shape[1], h, w, C, T.shape[2], 1, ops._stream()), "lwg_lwb_attention_kv_bwd_f32")
    return dq, dkv


@pytest.mark.parametrize("family,geom", TABLE, ids=TABLE_IDS)
def test_backward(family, geom):
    """lwg_lwb_attention_bwd_f32 and lwg_lwb_attention_kv_bwd_f32 with src_batched=True and B in {2, 3} (a geometry's B = 1 becomes 2),
    every C, against fp64 autograd under check_attention_backward's 5e-4; the K | V form's halves against the two-tensor form under its
    1e-5 rule; dKs / dVs exactly zero on every texel further than one pixel from any tap (the reference is exactly zero there too)."""
    B, ns, S, h, w = geom
    B = max(B, 2)
    W = _Worst(family, af.geom_id((B, ns, S, h, w)))
    T = af.flows(family, B, ns, S, S, seed=0, size=(h, w))
    far = ~af.touched(T, h, w, B * ns, True)
    for C in C_F32:
        key = f"C{C}"
        r = af.rs(1, C, B, ns, h, w)
        q, Ks, Vs, bk, bv = af.qkv_operands(r, B, ns, h, w, C, True)
        dout = af._n(r, (B, h, w, C))
        ref = af.ref_attention_bwd(q, Ks, Vs, bk, bv, T, dout, True)
        assert (ref[1][far] == 0).all() and (ref[2][far] == 0).all()
        qd, Kd, Vd, bkd, bvd, Td, gd = _dev((q, Ks, Vs, bk, bv, T, dout))
        dq, dK, dV = _bwd_launch(qd, Kd, Vd, bkd, bvd, Td, gd)
        dq2, dkv = _kv_bwd_launch(qd, torch.cat([Kd, Vd], dim=3), bkd, bvd, Td, gd)
        via_ops = ops.lwb_attention_bwd(qd, Kd, Vd, bkd, bvd, Td, gd, src_batched=True)
        torch.cuda.synchronize()
        got = [t.cpu() for t in (dq, dK, dV)]
        got_kv = [dq2.cpu(), dkv[..., :C].cpu(), dkv[..., C:].cpu()]
        for kernel, g_ in (("attn_bwd", got), ("attn_kv_bwd", got_kv)):
            errs = af.bwd_errors(g_, ref)
            W.add(kernel, key, [(n, e if e == e else float("inf"), af.BWD_TOL) for n, e in zip(("dq", "dKs", "dVs"), errs)])
            if not ((g_[1][far] == 0).all() and (g_[2][far] == 0).all()):
                W.fail(kernel, key, "a texel no tap touches received a gradient")
        sc = max(got[1].abs().max().item(), got[2].abs().max().item())
        W.add("attn_kv_bwd_vs_bwd", key, [(n, (a_ - b_).abs().max().item(), af.KV_TOL * max(sc, b_.abs().max().item()))
                                          for n, a_, b_ in zip(("dq", "dKs", "dVs"), got_kv, got)])
        W.add("attn_bwd_ops_vs_abi", key, [(n, (a_.cpu() - b_).abs().max().item(), af.KV_TOL * max(sc, b_.abs().max().item()))
                                           for n, a_, b_ in zip(("dq", "dKs", "dVs"), via_ops, got)])
    W.done()


# ------------------------------------------------------------------------------------------------ flow resize
@pytest.mark.parametrize("family,geom", RESIZE_TABLE, ids=[f"{f}-B{g[0]}_ns{g[1]}_S{g[2]}_{g[3]}x{g[4]}" for f, g in RESIZE_TABLE])
def test_flow_resize(family, geom):
    """lwg_flow_resize_f32 against emu_ops.flow_resize in fp64: <= 4e-6 S max(1, max |T|) (check_lwb_attention's bound, scaled by the
    field's magnitude); S == h == w returns the input bitwise."""
    B, ns, S, h, w = geom
    T = af.flows(family, B, ns, S, S, seed=0, size=(h, w))
    Td = T.to(DEV)
    out = _nan((B, ns, h, w, 2))
    _lib.check(_lib.lib().lwg_flow_resize_f32(Td.data_ptr(), B * ns, S, h, w, out.data_ptr(), ops._stream()), "lwg_flow_resize_f32")
    via_ops = ops.flow_resize(Td, h, w)
    torch.cuda.synchronize()
    assert torch.equal(via_ops, out)
    err = (out.cpu().double() - af.ref_flow_resize(T, h, w)).abs().max().item()
    bound = af.RESIZE_TOL * S * max(1.0, T.abs().max().item())
    print(f"ATTNFLOW flow_resize {family} {af.geom_id(geom)} worst_at - max_abs {err:.3e} / {bound:.3e}")
    assert err <= bound, (err, bound)
    if S == h and S == w:
        assert torch.equal(out.cpu(), T), "the identity resize changed the field"


def test_peaked_operands_are_peaked():
    """The peaked operands put nearly all of a pixel's softmax weight on one source (the online rescaling sees logit gaps of order 40),
    the plain ones do not - on the values the kernels above are handed."""
    geom = (3, 3, 13, 13, 13)
    for peaked, lo, hi in ((False, 0.0, 0.8), (True, 0.95, 1.0)):
        (q, Ks, Vs, bk, bv), T, ref, _ = af.forward_case("identity", geom, 64, True, peaked)
        Kw = Ks.double().view(3, 3, 13, 13, 64) + bk.double()
        a = torch.softmax((Kw * q.double().unsqueeze(1)).sum(-1) / 8.0, dim=1)
        assert lo <= a.max(dim=1).values.median().item() <= hi, (peaked, a.max(dim=1).values.median().item())
        got = ops.lwb_attention(*_dev((q, Ks, Vs, bk, bv, T)), _nan((3, 13, 13, 64)), src_batched=True)
        _cmp(got, ref.float(), 1e-4, "identity forward")
