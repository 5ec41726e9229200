"""Co-runner guard of the LiDAR trunk's own kernels, in the manner of tests/test_gpu_corunner.py: the sum kernel and the entry
transposition, 20 times each on fixed inputs beside split-f16 layers of a second stream, give the bits they give alone."""
import pytest
import torch

from co_occ_amd import core, lidar_trunk as lt

from util_second3d import bits_equal

pytestmark = pytest.mark.gpu
N_CALLS = 20


@pytest.mark.parametrize("corunner", ["h2p", "wino"])
@pytest.mark.parametrize("stage", ["fpn_sum", "zyx_to_rows"])
def test_trunk_kernels_are_bit_stable_beside_matrix_core_work(dev, stage, corunner):
    g = torch.Generator().manual_seed(11)
    xb = core.to_rows(torch.randn(1, 128, 100, 100, 8, generator=g).to(dev))
    pc = (core.PackedConv((torch.randn(128, 128, 1, 1, 1, generator=g) * 0.05).to(dev), ksize=1, pad=0) if corunner == "h2p" else
          core.PackedConv((torch.randn(128, 128, 3, 3, 3, generator=g) * 0.02).to(dev), ksize=3, pad=1))
    B, X, Y, Z = 1, 100, 100, 8
    ups = [core.Rows(torch.randn(B * (X // s) * (Y // s) * Z, s * s * 128, generator=g).to(dev), B, X // s, Y // s, Z, s * s * 128)
           for s in (1, 2, 4)]
    vol = torch.randn(1, 128, Z, Y, X, generator=g).to(dev)
    fn = (lambda: lt.fpn_sum(ups, [1, 2, 4], 128).t) if stage == "fpn_sum" else (lambda: lt.bczyx_to_rows(vol).t)
    s0, s1 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    with torch.no_grad():
        core.conv_rows(xb, pc, relu=False)
        torch.cuda.synchronize()
        with torch.cuda.stream(s0):
            ref = fn().clone()
        torch.cuda.synchronize()
        got = []
        for _ in range(N_CALLS):
            with torch.cuda.stream(s1):
                for _ in range(4):
                    core.conv_rows(xb, pc, relu=False)
            with torch.cuda.stream(s0):
                got.append(fn().clone())
        torch.cuda.synchronize()
    core.check_h2_overflow()
    bad = sum(int(not bits_equal(ref, t)) for t in got)
    assert bad == 0, "%s beside %s: %d of %d calls differ from the run alone" % (stage, corunner, bad, N_CALLS)
