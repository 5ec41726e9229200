"""Generate tests/golden/image_neck.npz from the reference's own SECONDFPN (development machine only: it needs the reference
checkout, found where ``oracle.refshim`` looks for it).

The reference file (mmdetection3d/mmdet3d/models/necks/second_fpn.py) is loaded by path, unmodified.  It imports three mmcv
builders, mmcv's ``BaseModule`` / ``auto_fp16`` and mmdet's ``NECKS`` registry, none of which is installed anywhere we run: this
script installs stubs of its own under those names (plain torch layers behind the builders, a pass-through decorator, a dict-backed
registry), instantiates the reference's class and runs the reference's ``forward`` in float64.  What it pins is the neck's wiring --
which levels are strided convolutions and which transposed ones, the BN eps, the concatenation order, the state_dict keys.  The
backbone (mmdet's ResNet) has no source in the reference checkout and stays a restatement.

Fixture: in [32, 64, 128, 256] -> out 32 each, strides [0.25, 0.5, 1, 2], 2 cameras, level maps 8x16, 4x8, 2x4, 1x2; weights and
inputs are float32 values (stored as float32, run as float64), the output float64.

    python tools/gen_image_encoder_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

IN, OUT_C, STRIDES, BN = [32, 64, 128, 256], [32, 32, 32, 32], [0.25, 0.5, 1, 2], 2
MAPS = [(8, 16), (4, 8), (2, 4), (1, 2)]
OUT = os.path.join(ROOT, "tests", "golden", "image_neck.npz")


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    m.__path__ = []
    sys.modules[name] = m
    return m


def install_stubs():
    def build_conv_layer(cfg, *args, **kwargs):
        cfg = dict(cfg)
        assert cfg.pop("type") == "Conv2d"
        return nn.Conv2d(*args, **kwargs, **cfg)

    def build_upsample_layer(cfg, *args, **kwargs):
        cfg = dict(cfg)
        assert cfg.pop("type") == "deconv"
        return nn.ConvTranspose2d(*args, **kwargs, **cfg)

    def build_norm_layer(cfg, num_features):
        cfg = dict(cfg)
        assert cfg.pop("type") == "BN"
        return "bn", nn.BatchNorm2d(num_features, **cfg)

    class BaseModule(nn.Module):
        def __init__(self, init_cfg=None):
            super().__init__()
            self.init_cfg = init_cfg

    def auto_fp16(*a, **k):
        return lambda f: f

    class Registry:
        def register_module(self):
            return lambda cls: cls
    _module("mmcv")
    _module("mmcv.cnn", build_conv_layer=build_conv_layer, build_norm_layer=build_norm_layer, build_upsample_layer=build_upsample_layer)
    _module("mmcv.runner", BaseModule=BaseModule, auto_fp16=auto_fp16)
    _module("mmdet")
    _module("mmdet.models", NECKS=Registry())


def main():
    from oracle import refshim
    import ref_image_encoder as R
    install_stubs()
    path = os.path.join(refshim.REF, "mmdetection3d", "mmdet3d", "models", "necks", "second_fpn.py")
    spec = importlib.util.spec_from_file_location("_ref_second_fpn", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net = mod.SECONDFPN(in_channels=IN, upsample_strides=STRIDES, out_channels=OUT_C).eval()
    sd = R.fixture_state_dict(net.state_dict(), 31, R.transposed_keys(STRIDES))
    assert len(sd) == 24
    g = torch.Generator().manual_seed(32)
    xs = [torch.randn(BN, c, h, w, generator=g) for c, (h, w) in zip(IN, MAPS)]
    for x in xs:
        x[1] *= 2.5
    net.load_state_dict(R.cast(sd, torch.float64))
    net = net.double()
    with torch.no_grad():
        out = net([x.double() for x in xs])
    assert isinstance(out, list) and len(out) == 1 and tuple(out[0].shape) == (BN, sum(OUT_C), 2, 4)
    arrays = {"sd/" + k: v.numpy() for k, v in sd.items()}
    arrays.update({"x%d" % i: x.numpy() for i, x in enumerate(xs)})
    arrays.update(out=out[0].numpy(), strides=np.asarray(STRIDES, np.float64))
    np.savez(OUT, **arrays)
    print("wrote %s: %d state_dict entries, %d bytes" % (OUT, len(sd), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
