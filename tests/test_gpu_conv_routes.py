"""One launch per route of ops.conv2d / ops.conv_transpose2d on the device, through a recorder that forwards every call to the real library:
the traces are those of tests/golden/conv_routes_parent.json - so the host stubs and the 256-CU host plans of tests/test_conv_routes_cpu.py
describe what happens with device tensors - and the route functions name the launch that ran.  The list-driven forms are left to
tests/test_gpu_spade_skip*.py, which run them on real lists."""
import pytest
import torch

from tests import conv_route_cases as crc
from tests.test_conv_routes_cpu import GOLDEN, check_route

pytestmark = pytest.mark.gpu
GPU_CASES = [c for c in crc.CASES if c["gpu"]]


def test_one_case_per_route():
    launches = {n for c in GPU_CASES for n in GOLDEN[c["id"]]["calls"] if not crc.is_host(n) and not n.startswith("panel:")}
    assert len(GPU_CASES) == 21 and len(launches) >= 17, sorted(launches)


@pytest.mark.parametrize("c", GPU_CASES, ids=lambda c: c["id"])
def test_device_trace_is_the_recorded_one(c):
    rec, args, kw = crc.run_case(c, device="cuda")
    torch.cuda.synchronize()
    y = args[2]
    assert bool(torch.isfinite(y.float()).all()) and float(y.float().abs().max()) == 0.0        # zero weights, zero bias, ReLU
    assert rec == GOLDEN[c["id"]]
    check_route(c, rec, args, kw)
