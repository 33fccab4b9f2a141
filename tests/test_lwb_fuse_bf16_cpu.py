"""The bf16 engine of the AddLWB / AvgLWB / SoftGateAddLWB / SoftGateAvgLWB generators on the CPU: ``lwg_lwb_fuse_bf16`` is declared and
exported, its host-side rejections, the contract restatement (tests/lwbfuse_bf16_emu.py) against torch's eager fp64 chain, and the
yardstick of the GPU tests' 40 dB bound - what bf16 storage alone costs these generators in the oracle."""
import ctypes

import pytest
import torch

from ipercore_amd import _lib
from tests import lwbfuse_bf16_emu as emu16
from tests.gpu_checks import _rand
from tests.test_gpu_lwb_fuse_backward import CASES
from tests.test_lwb_fuse_backward_cpu import adversarial_flows


def test_fuse_bf16_is_declared_and_exported():
    """include/lwg_hip.h declares it, the library exports it, the binding resolves it; the addition leaves the ABI version at 10."""
    assert "lwg_lwb_fuse_bf16" in _lib.header_symbols()
    assert "lwg_lwb_fuse_bf16" in _lib._SIGS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "lwg_lwb_fuse_bf16")
    L = _lib.lib()
    assert L.lwg_lwb_fuse_bf16 is not None and L.lwg_abi_version() == 10


def test_fuse_bf16_host_rejections():
    """Every host-side rejection of lwg_lwb_fuse_bf16 returns 1 before any launch (no GPU is touched)."""
    L = _lib.lib()
    buf = (ctypes.c_float * 4)()
    bad = ctypes.cast(buf, ctypes.c_void_p)
    f = L.lwg_lwb_fuse_bf16
    ok = dict(tsf_x=bad, src_x=bad, gate=None, T=bad, out=bad, B=1, ns=2, h=8, w=8, C=64, S=8)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["tsf_x"], a["src_x"], a["gate"], a["T"], a["out"], a["B"], a["ns"], a["h"], a["w"], a["C"], a["S"], 0, 1.0, 1.0, None)
    for name in ("tsf_x", "src_x", "T", "out"):
        assert call(**{name: None}) == 1, name
        assert call(**{name: None}, gate=bad) == 1, name
    for name in ("B", "ns", "h", "w", "S"):
        assert call(**{name: 0}) == 1 and call(**{name: -3}) == 1, name
    for C in (48, 512, 0, 16, 96):
        assert call(C=C) == 1, C


def test_ops_lwb_fuse_checks_dtypes_before_any_launch():
    """ops.lwb_fuse dispatches on tsf_x.dtype: src_x, gate and out must share it and the flows are fp32 (asserted before a pointer is taken);
    matching CPU tensors of either storage type still meet the no-CPU-fallback refusal."""
    from ipercore_amd import ops
    bf = torch.bfloat16
    mk = lambda dt: (torch.zeros(1, 4, 4, 32, dtype=dt), torch.zeros(2, 4, 4, 32, dtype=dt), torch.zeros(1, 2, 4, 4, 2), torch.zeros(1, 4, 4, 32, dtype=dt))  # noqa: E731
    for dt, other in ((bf, torch.float32), (torch.float32, bf)):
        tsf, src, T, out = mk(dt)
        with pytest.raises(AssertionError):
            ops.lwb_fuse(tsf, src.to(other), T, out)
        with pytest.raises(AssertionError):
            ops.lwb_fuse(tsf, src, T, out.to(other))
        with pytest.raises(AssertionError):
            ops.lwb_fuse(tsf, src, T, out, gate=tsf.to(other))
        with pytest.raises(AssertionError):
            ops.lwb_fuse(tsf, src, T.double(), out)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.lwb_fuse(tsf, src, T, out, gate=tsf)


@pytest.mark.parametrize("C,B,ns,h,w,S_,gated,batched,sw,so", CASES, ids=[f"c{c[0]}_b{c[1]}_ns{c[2]}_{c[3]}x{c[4]}_S{c[5]}" for c in CASES])
def test_emulation_matches_eager_fp64_chain(C, B, ns, h, w, S_, gated, batched, sw, so):
    """The tap-by-tap contract in fp64 against F.interpolate(align_corners=True) -> F.grid_sample(zeros, align_corners=False) -> fuse in fp64,
    on the bf16 operands and adversarial flows of the GPU kernel cases: 1e-12."""
    tsf, src, gate = emu16.kernel_case(C, B, ns, h, w, S_, gated, batched, _rand)
    T = adversarial_flows(B, ns, S_, seed=7 + C + h, dtype=torch.float32)
    got = emu16.lwb_fuse(tsf, src, T, gate, sw, so, bool(batched), dtype=torch.float64)
    want = emu16.eager_chain(tsf, src, T, gate, sw, so, bool(batched), dtype=torch.float64)
    assert got.dtype == torch.float64 and (got - want).abs().max().item() <= 1e-12
    # bf16-valued fp32 operands are the same operands: widening is exact
    up = emu16.lwb_fuse(tsf.float(), src.float(), T, None if gate is None else gate.float(), sw, so, bool(batched), dtype=torch.float64)
    assert torch.equal(up, got)


@pytest.mark.parametrize("tag", ["tiny", "full"])
@pytest.mark.parametrize("kind", list(emu16.KINDS))
def test_bf16_storage_yardstick(monkeypatch, kind, tag):
    """bf16 storage alone (weights and every layer output rounded to bf16 in the oracle, fp32 arithmetic) keeps tsf_img >= 60 dB from the
    fp32 oracle for every kind, reduced and full width, on the case and seed the GPU tests use (measured with this emulation: 67.5 .. 79.4 dB, worst
    AddLWB full; tsf_mask at peak-to-peak 1: 73.9 .. 86.7 dB).  The GPU tests' 40 dB bound therefore has > 25 dB of headroom: a failure
    there points at a kernel, not at the yardstick."""
    _, sdn = emu16.build_generator(kind, tag)
    src_inputs, tsf_inputs, Tst = emu16.generator_inputs()
    img, mask = emu16.oracle_tsf(sdn, kind, tag, src_inputs, tsf_inputs, Tst)
    with monkeypatch.context() as mp:
        emu16.install_bf16_storage(mp)
        img16, mask16 = emu16.oracle_tsf(sdn, kind, tag, src_inputs, tsf_inputs, Tst)
    p_img, p_mask = emu16.psnr(img16, img, 2.0), emu16.psnr(mask16, mask, 1.0)
    print("bf16 storage yardstick", kind, tag, f"img {p_img:.1f} dB mask {p_mask:.1f} dB")
    assert (img16 - img).abs().max().item() > 0, "the storage emulation changed nothing"
    assert torch.isfinite(img16).all() and p_img >= 60.0, (kind, tag, p_img)
