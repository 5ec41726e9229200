"""Generate tests/golden/second3d.npz by running the UNMODIFIED reference trunk (P/coocc/backbones/second3d.py,
P/coocc/necks/second3d_fpn.py, imported by path through oracle/refshim.py) in eval mode on seeded inputs.  Runs only where the
reference checkout is present:

    python tools/gen_golden_second3d.py

Three things the shim does not provide are supplied here before the files are loaded: ``mmcv.cnn.build_upsample_layer``
('deconv3d' -> nn.ConvTranspose3d), a stand-in module ``symbol`` with an ``import_from`` attribute (second3d.py:2 imports it and
never uses it; the module left the standard library in Python 3.10), and config dicts with attribute access
(``conv_cfg.type``, second3d.py:46).

Both modules are built from the values of projects/configs/coocc_nusc/coocc_lidar.py (``co_occ_amd.synth.second3d_cfg``) for the
cases of ``synth.SECOND3D_CASES`` that are stored ("small": reduced layer counts on [1,128,2,8,8]; "config": the config's [5,5,5]
on [1,128,2,16,16]).  Inputs and weights (Kaiming-normal, BN weight / variance U(0.5, 1.5), mean / bias N(0, 0.1)) are re-created
from seeds by ``synth``; only the three backbone outputs, the neck output and the state_dict key -> shape maps are stored.  The
restatement tests/ref_second3d.py is run on the same inputs in fp32 and its largest |delta| against the reference is printed and
stored (``<case>_restatement_delta``; expected 0: same torch ops in the same order) -- and in fp64, to check the condition the
GPU test relies on (the fp32 evaluation within TOL / 4 of the fp64 one).  Fixed zip timestamps: running this again gives the same
bytes."""
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refshim  # noqa: E402
from co_occ_amd import synth  # noqa: E402  (host-side module: numpy + torch only)
import ref_second3d  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "second3d.npz")
STORED = ("small", "config")


class Cfg(dict):
    __getattr__ = dict.get


def _build_upsample_layer(cfg, *args, **kwargs):
    cfg = dict(cfg)
    t = cfg.pop("type")
    assert t == "deconv3d", t
    return nn.ConvTranspose3d(*args, **kwargs, **cfg)


def load_reference():
    refshim.install()
    sys.modules["mmcv.cnn"].build_upsample_layer = _build_upsample_layer
    sys.modules.setdefault("symbol", types.ModuleType("symbol")).import_from = None
    cooc = os.path.join(refshim.PLUGIN, "coocc")
    b = refshim._load("projects.mmdet3d_plugin.coocc.backbones.second3d", os.path.join(cooc, "backbones", "second3d.py"))
    n = refshim._load("projects.mmdet3d_plugin.coocc.necks.second3d_fpn", os.path.join(cooc, "necks", "second3d_fpn.py"))
    return b.SECOND3D, n.SECOND3DFPN


def attr_cfg(cfg):
    return {k: (Cfg(v) if isinstance(v, dict) else v) for k, v in cfg.items() if k != "type"}


def main():
    torch.set_num_threads(1)
    RB, RN = load_reference()
    out = {}
    for name in STORED:
        c = synth.SECOND3D_CASES[name]
        bcfg, ncfg = synth.second3d_cfg(c["layer_nums"])
        rb, rn = RB(**attr_cfg(bcfg)).eval(), RN(**attr_cfg(ncfg)).eval()
        sdb, sdn = synth.second3d_weights(rb, rn, c["seed"])
        rb.load_state_dict(sdb)
        rn.load_state_dict(sdn)
        x = synth.second3d_input(c["grid_zyx"], seed=c["seed"])
        with torch.no_grad():
            feats = rb(x)
            y = rn(list(feats))
        b32, n32 = ref_second3d.build(bcfg, ncfg, sdb, sdn)
        f32, y32 = ref_second3d.run(b32, n32, x)
        b64, n64 = ref_second3d.build(bcfg, ncfg, sdb, sdn, torch.float64)
        f64, y64 = ref_second3d.run(b64, n64, x)
        delta = max(float((a - b).abs().max()) for a, b in zip(list(feats) + [y], list(f32) + [y32]))
        rel = [float((a.double() - b).abs().max() / max(1.0, float(b.abs().max()))) for a, b in zip(list(feats) + [y], list(f64) + [y64])]
        print("%s: restatement |delta| %g; fp32 vs fp64 (scale-relative) %s; max|ref| %s" % (
            name, delta, ["%.1e" % r for r in rel], ["%.1f" % float(t.abs().max()) for t in list(feats) + [y]]))
        assert max(rel) <= 1e-4 / 4, "the fp32 evaluation is not within TOL / 4 of fp64 on this fixture: choose other weights"
        for i, t in enumerate(feats):
            out["%s_feat%d" % (name, i)] = t.numpy()
        out[name + "_neck"] = y.numpy()
        out[name + "_restatement_delta"] = np.float64(delta)
        for tag, m in (("backbone", rb), ("neck", rn)):
            sd = m.state_dict()
            out["%s_%s_keys" % (name, tag)] = np.array(list(sd.keys()))
            out["%s_%s_shapes" % (name, tag)] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            b = io.BytesIO()
            np.save(b, np.asarray(out[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(2026, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, b.getvalue())
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print("wrote %s (%d bytes)" % (OUT, len(buf.getvalue())))


if __name__ == "__main__":
    main()
