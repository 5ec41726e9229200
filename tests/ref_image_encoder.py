"""Torch restatements of the image encoder's eval-mode arithmetic, on state dicts with the reference's keys and in the dtype of
their tensors (float64 = the judge, float32 = the fp32 noise floor): mmdet 2.14's ``ResNet`` (depth 50 / 101, the torchvision
Bottleneck layout, ``style='pytorch'``) and mmdet3d's ``SECONDFPN`` (mmdet3d/models/necks/second_fpn.py; pinned against the
reference file's own float64 run by tests/golden/image_neck.npz).  The two ``nn.Module`` classes below are plain torch modules with
the same keys: what a user without this package's encoder would inject (tools/bench_image_encoder.py times them)."""
import torch
import torch.nn.functional as F
from torch import nn

ARCH = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}
NECK_EPS = 1e-3


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def bn(x, sd, pre, eps=1e-5):
    s = sd[pre + ".weight"] / torch.sqrt(sd[pre + ".running_var"] + eps)
    return (x - sd[pre + ".running_mean"].view(1, -1, 1, 1)) * s.view(1, -1, 1, 1) + sd[pre + ".bias"].view(1, -1, 1, 1)


# ------------------------------------------------------------------ functional restatements (state dict in, tensors out)
def stem(x, sd, relu=True, pool=True):
    y = bn(F.conv2d(x, sd["conv1.weight"], None, stride=2, padding=3), sd, "bn1")
    if relu:
        y = torch.relu(y)
    return F.max_pool2d(y, 3, 2, 1) if pool else y


def bottleneck(x, sd, pre, stride):
    y = torch.relu(bn(F.conv2d(x, sd[pre + ".conv1.weight"]), sd, pre + ".bn1"))
    y = torch.relu(bn(F.conv2d(y, sd[pre + ".conv2.weight"], None, stride=stride, padding=1), sd, pre + ".bn2"))
    y = bn(F.conv2d(y, sd[pre + ".conv3.weight"]), sd, pre + ".bn3")
    if pre + ".downsample.0.weight" in sd:
        x = bn(F.conv2d(x, sd[pre + ".downsample.0.weight"], None, stride=stride), sd, pre + ".downsample.1")
    return torch.relu(y + x)


def resnet(x, sd, depth, strides=(1, 2, 2, 2), out_indices=(0, 1, 2, 3)):
    """x [BN,3,H,W] -> tuple of stage outputs, in the dtype of x / sd."""
    h = stem(x, sd)
    outs = []
    for i, n in enumerate(ARCH[depth]):
        for j in range(n):
            h = bottleneck(h, sd, "layer%d.%d" % (i + 1, j), strides[i] if j == 0 else 1)
        if i in out_indices:
            outs.append(h)
    return tuple(outs)


def second_fpn(xs, sd, upsample_strides, use_conv_for_no_stride=False, eps=NECK_EPS):
    ups = []
    for i, (x, s) in enumerate(zip(xs, upsample_strides)):
        w = sd["deblocks.%d.0.weight" % i]
        b = sd.get("deblocks.%d.0.bias" % i)
        if s > 1 or (s == 1 and not use_conv_for_no_stride):
            y = F.conv_transpose2d(x, w, b, stride=int(s))
        else:
            y = F.conv2d(x, w, b, stride=int(round(1.0 / s)))
        ups.append(torch.relu(bn(y, sd, "deblocks.%d.1" % i, eps)))
    return [torch.cat(ups, 1) if len(ups) > 1 else ups[0]]


# ------------------------------------------------------------------ plain torch modules with the reference's keys
class Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = downsample

    def forward(self, x):
        y = torch.relu(self.bn1(self.conv1(x)))
        y = torch.relu(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        return torch.relu(y + (x if self.downsample is None else self.downsample(x)))


class TorchResNet(nn.Module):
    def __init__(self, depth, base_channels=64, stem_channels=64, strides=(1, 2, 2, 2)):
        super().__init__()
        self.conv1 = nn.Conv2d(3, stem_channels, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(stem_channels)
        inplanes = stem_channels
        for i, n in enumerate(ARCH[depth]):
            planes, blocks = base_channels * 2 ** i, []
            for j in range(n):
                s = strides[i] if j == 0 else 1
                down = None
                if j == 0 and (s != 1 or inplanes != planes * 4):
                    down = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=s, bias=False), nn.BatchNorm2d(planes * 4))
                blocks.append(Bottleneck(inplanes, planes, s, down))
                inplanes = planes * 4
            setattr(self, "layer%d" % (i + 1), nn.Sequential(*blocks))

    def forward(self, x):
        h = F.max_pool2d(torch.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        outs = []
        for i in range(4):
            h = getattr(self, "layer%d" % (i + 1))(h)
            outs.append(h)
        return tuple(outs)


class TorchSECONDFPN(nn.Module):
    def __init__(self, in_channels, out_channels, upsample_strides, use_conv_for_no_stride=False):
        super().__init__()
        blocks = []
        for ci, co, s in zip(in_channels, out_channels, upsample_strides):
            if s > 1 or (s == 1 and not use_conv_for_no_stride):
                up = nn.ConvTranspose2d(ci, co, int(s), stride=int(s), bias=False)
            else:
                k = int(round(1.0 / s))
                up = nn.Conv2d(ci, co, k, stride=k, bias=False)
            blocks.append(nn.Sequential(up, nn.BatchNorm2d(co, eps=NECK_EPS, momentum=0.01), nn.ReLU(inplace=True)))
        self.deblocks = nn.ModuleList(blocks)

    def forward(self, xs):
        ups = [blk(x) for blk, x in zip(self.deblocks, xs)]
        return [torch.cat(ups, 1) if len(ups) > 1 else ups[0]]


# ------------------------------------------------------------------ the fixture recipe
def transposed_keys(upsample_strides, use_conv_for_no_stride=False):
    """The neck's ConvTranspose2d weight keys."""
    return {"deblocks.%d.0.weight" % i for i, s in enumerate(upsample_strides) if s > 1 or (s == 1 and not use_conv_for_no_stride)}


def fixture_state_dict(sd, seed, transposed=()):
    """Random float32 values for a state dict with the encoder's keys: conv weights N(0, 2 / fan_in), BN weight U(0.5, 1.5) (x 0.3
    for every bn3, which keeps the residual sums of 33 blocks inside a few hundred), BN bias and running mean 0.2 N(0, 1), running
    variance U(0.5, 1.5).  ``transposed``: the keys of ConvTranspose2d weights."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            out[k] = torch.zeros_like(v)
        elif k.endswith("running_var"):
            out[k] = torch.rand(v.shape, generator=g) + 0.5
        elif k.endswith("running_mean"):
            out[k] = 0.2 * torch.randn(v.shape, generator=g)
        elif v.dim() == 4:
            fan_in = v.shape[0] if k in transposed else v[0].numel()        # a ConvTranspose2d weight is [Cin,Cout,s,s], kernel = stride
            out[k] = torch.randn(v.shape, generator=g) * (2.0 / fan_in) ** 0.5
        elif k.endswith("bias"):
            out[k] = 0.2 * torch.randn(v.shape, generator=g)
        else:                                   # a BN weight
            w = torch.rand(v.shape, generator=g) + 0.5
            out[k] = w * 0.3 if ".bn3." in k else w
    return out


def fixture_images(BN, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(BN, 3, H, W, generator=g)
    if BN > 1:
        x[1] *= 2.5
    return x
