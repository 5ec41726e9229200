"""Generate tests/golden/depthnet.npz from the reference's own DepthNet wiring (development machine only: it needs the reference
checkout that ``oracle.refshim`` loads by path).

The reference file builds DepthNet from two library classes that are not installed anywhere we run: mmdet 2.14's ``BasicBlock``
and mmcv 1.4.0's DCN (``build_conv_layer(dict(type='DCN', ...))``).  This script puts its own torch restatements of the two under
those names into the loaded module, instantiates the reference's ``DepthNet`` and runs the reference's ``forward`` in float64.
What it pins is therefore the module's wiring, its ASPP / Mlp / SELayer classes and its state_dict keys -- not the DCN against
mmcv.

Fixture: mid = 32, context = 16, depth = 24, BN = 2 cameras, map 12 x 20; non-trivial BN running statistics; ``conv_offset`` given
random weights so the offsets are about a pixel.  Weights and inputs are float32 values (stored as float32, run as float64), the
outputs float64: the state dict, x, mlp_input, the module's output and the ASPP block's input and output alone.

    python tools/gen_depthnet_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IN, MID, CONTEXT, DEPTH, BN, H, W = 32, 32, 16, 24, 2, 12, 20
OUT = os.path.join(ROOT, "tests", "golden", "depthnet.npz")


class BasicBlock(nn.Module):
    """mmdet 2.14 ResNet BasicBlock(inplanes, planes) with its defaults: stride 1, no downsample, BN."""

    def __init__(self, inplanes, planes):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + x)


class DeformConv2dPack(nn.Module):
    """mmcv 1.4.0 DeformConv2dPack(cin, cout, 3, padding=1, groups, deform_groups=1, bias=False): offsets from ``conv_offset``
    (zero-initialised Conv2d(cin, 18, 3, padding=1)), channel 2t / 2t + 1 = row / column offset of tap t = 3i + j, bilinear
    sampling with zeros outside, all channels share the offset field."""

    def __init__(self, in_channels, out_channels, kernel_size, padding, groups, im2col_step=128):
        super().__init__()
        assert kernel_size == 3 and padding == 1
        self.groups = groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, 3, 3))
        nn.init.kaiming_uniform_(self.weight, nonlinearity="relu")
        self.conv_offset = nn.Conv2d(in_channels, 18, 3, padding=1, bias=True)
        nn.init.zeros_(self.conv_offset.weight)
        nn.init.zeros_(self.conv_offset.bias)

    def forward(self, x):
        off = self.conv_offset(x)
        B, C, Hh, Ww = x.shape
        ys = torch.arange(Hh, dtype=x.dtype).view(1, Hh, 1)
        xs = torch.arange(Ww, dtype=x.dtype).view(1, 1, Ww)
        co, cg = self.weight.shape[0] // self.groups, C // self.groups
        out = x.new_zeros(B, self.groups, co, Hh, Ww)
        for t in range(9):
            py, px = ys - 1 + t // 3 + off[:, 2 * t], xs - 1 + t % 3 + off[:, 2 * t + 1]
            grid = torch.stack([2 * px / (Ww - 1) - 1, 2 * py / (Hh - 1) - 1], -1)
            s = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True).view(B, self.groups, cg, Hh, Ww)
            out = out + torch.einsum("goc,bgchw->bgohw", self.weight.view(self.groups, co, cg, 9)[..., t], s)
        return out.view(B, self.groups * co, Hh, Ww)


def build_conv_layer(cfg, *args, **kwargs):
    cfg = dict(cfg)
    assert cfg.pop("type") == "DCN"
    return DeformConv2dPack(*args, **kwargs, **cfg)


def main():
    from oracle import refshim
    mod = refshim.install()["lss_bevdepth"]
    mod.BasicBlock, mod.build_conv_layer = BasicBlock, build_conv_layer
    torch.manual_seed(20)
    net = mod.DepthNet(IN, MID, CONTEXT, DEPTH)
    g = torch.Generator().manual_seed(21)
    for m in net.modules():
        if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) * 0.6 + 0.7)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.2)
    x = torch.randn(BN, IN, H, W, generator=g)
    mlp_input = torch.randn(1, BN, 27, generator=g)
    net = net.double().eval()
    co = net.depth_conv[4].conv_offset
    with torch.no_grad():
        # offsets of about a pixel: scale random weights by the ASPP output they will see
        co.weight.copy_(torch.randn(co.weight.shape, generator=g).double())
        co.bias.copy_(torch.randn(18, generator=g).double() * 0.3)
        seen = {}
        hk = net.depth_conv[3].register_forward_hook(lambda m, i, o: seen.update(a=o))
        net(x.double(), mlp_input.double())
        hk.remove()
        co.weight.mul_(1.0 / float(co(seen["a"]).std()))
    sd = {k: (v.float() if v.is_floating_point() else v) for k, v in net.state_dict().items()}        # float32 values ...
    net.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()})     # ... run as float64
    taps = {}
    hk = net.depth_conv[3].register_forward_hook(lambda m, i, o: taps.update(aspp_in=i[0].clone(), aspp_out=o.clone()))
    with torch.no_grad():
        out = net(x.double(), mlp_input.double())
        off = co(taps["aspp_out"])
    hk.remove()
    assert len(sd) == 107 and tuple(out.shape) == (BN, DEPTH + CONTEXT, H, W)
    arrays = {"sd/" + k: v.numpy() for k, v in sd.items()}
    arrays.update(x=x.numpy(), mlp_input=mlp_input.numpy(), out=out.numpy(), aspp_in=taps["aspp_in"].numpy(),
                  aspp_out=taps["aspp_out"].numpy())
    np.savez(OUT, **arrays)
    print("wrote %s: %d state_dict entries, %d bytes; offsets std %.2f px, max %.2f px" % (
        OUT, len(sd), os.path.getsize(OUT), float(off.std()), float(off.abs().max())))


if __name__ == "__main__":
    main()
