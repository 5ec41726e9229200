"""Plain torch restatement of the dense LiDAR trunk, runnable in fp32 and fp64 on the CPU: the oracle of
co_occ_amd/lidar_trunk.py.  Same ``state_dict`` keys and shapes as the reference modules
(P/coocc/backbones/second3d.py, P/coocc/necks/second3d_fpn.py); tools/gen_golden_second3d.py checks it against the unmodified
reference files and writes tests/golden/second3d.npz."""
import torch
from torch import nn


def _bn(norm_cfg, c):
    cfg = dict(norm_cfg)
    assert cfg.pop("type") in ("BN3d", "BN"), "BN3d only"
    cfg.pop("requires_grad", None)
    return nn.BatchNorm3d(c, **cfg)


class RefSECOND3D(nn.Module):
    """P/coocc/backbones/second3d.py:24-114 for the 'Conv3d' kernel type."""

    def __init__(self, in_channels=128, out_channels=(128, 128, 256), layer_nums=(3, 5, 5), layer_strides=(2, 2, 2), is_cascade=True,
                 norm_cfg=dict(type='BN3d', eps=1e-3, momentum=0.01), conv_cfg=dict(type='Conv3d', bias=False), **_):
        super().__init__()
        conv_cfg = dict(conv_cfg)
        assert conv_cfg.pop("type") == "Conv3d"
        in_filters = list(in_channels) if isinstance(in_channels, (list, tuple)) else [in_channels, *out_channels[:-1]]   # :39-42
        kernel = tuple(conv_cfg.pop("kernel", (1, 3, 3)))                                                      # :48-51
        padding = tuple((k - 1) // 2 for k in kernel)                                                          # :52
        self.is_cascade = is_cascade
        blocks = []
        for i, n in enumerate(layer_nums):                                                                    # :53-77
            s = layer_strides[i]
            block = [nn.Conv3d(in_filters[i], out_channels[i], kernel, stride=(1, s, s), padding=padding, **conv_cfg),
                     _bn(norm_cfg, out_channels[i]), nn.ReLU(inplace=True)]
            for _j in range(n):
                block += [nn.Conv3d(out_channels[i], out_channels[i], kernel, padding=padding, **conv_cfg),
                          _bn(norm_cfg, out_channels[i]), nn.ReLU(inplace=True)]
            blocks.append(nn.Sequential(*block))
        self.blocks = nn.ModuleList(blocks)

    def forward(self, x):                                                                                     # :91-114
        outs = []
        for blk in self.blocks:
            if self.is_cascade:
                x = blk(x)
                outs.append(x)
            else:
                outs.append(blk(x))
        return tuple(outs)


class RefSECOND3DFPN(nn.Module):
    """P/coocc/necks/second3d_fpn.py:27-143 for 'deconv3d' upsampling, integer strides, no sep_kernel, no distillation."""

    def __init__(self, in_channels=(128, 128, 256), out_channels=(256, 256, 256), upsample_strides=(1, 2, 4),
                 norm_cfg=dict(type='BN3d', eps=1e-3, momentum=0.01), upsample_cfg=dict(type='deconv3d', bias=False),
                 conv_cfg=dict(type='Conv3d', bias=False), extra_conv=None, use_conv_for_no_stride=False, **_):
        super().__init__()
        up_cfg, conv_cfg = dict(upsample_cfg), dict(conv_cfg)
        assert up_cfg.pop("type") == "deconv3d" and conv_cfg.pop("type") == "Conv3d"
        self.in_channels = list(in_channels)
        deblocks = []
        for i, oc in enumerate(out_channels):                                                                 # :47-69
            s = upsample_strides[i]
            if s > 1 or (s == 1 and not use_conv_for_no_stride):
                up = nn.ConvTranspose3d(in_channels[i], oc, (1, s, s), stride=(1, s, s), **up_cfg)
            else:
                up = nn.Conv3d(in_channels[i], oc, (1, 1, 1), stride=(1, 1, 1), **conv_cfg)
            deblocks.append(nn.Sequential(up, _bn(norm_cfg, oc), nn.ReLU(inplace=True)))
        self.deblocks = nn.ModuleList(deblocks)
        self.extra = extra_conv is not None
        if self.extra:                                                                                        # :72-104
            ec = dict(extra_conv)
            assert ec.pop("type") == "Conv3d"
            n = ec.pop("num_conv")
            kernel = tuple(ec.pop("kernel", (3, 3, 3)))
            padding = tuple((k - 1) // 2 for k in kernel)
            extra = []
            for _j in range(n):
                extra += [nn.Conv3d(out_channels[-1], out_channels[-1], kernel, padding=padding, **ec),
                          _bn(norm_cfg, out_channels[-1]), nn.ReLU(inplace=True)]
            self.extra_blocks = nn.Sequential(*extra)

    def forward(self, x):                                                                                     # :108-143
        assert len(x) == len(self.in_channels)
        ups = [d(x[i]) for i, d in enumerate(self.deblocks)]
        out = sum(ups) if len(ups) > 1 else ups[0]
        return self.extra_blocks(out) if self.extra else out


def build(backbone_cfg, neck_cfg, sd_backbone=None, sd_neck=None, dtype=torch.float32):
    """Both modules from config dicts (``type`` ignored), optionally loaded, in eval mode and ``dtype``."""
    b = RefSECOND3D(**{k: v for k, v in backbone_cfg.items() if k != "type"})
    n = RefSECOND3DFPN(**{k: v for k, v in neck_cfg.items() if k != "type"})
    if sd_backbone is not None:
        b.load_state_dict(sd_backbone)
    if sd_neck is not None:
        n.load_state_dict(sd_neck)
    return b.to(dtype).eval(), n.to(dtype).eval()


def run(backbone, neck, x):
    """(backbone outputs, neck output) of ``x`` [B,C,Z,Y,X] in the modules' dtype."""
    dt = next(backbone.parameters()).dtype
    with torch.no_grad():
        feats = backbone(x.to(dt))
        return feats, neck(list(feats))
