"""Generate tests/golden/render_eval.npz: the render-evaluation numbers of the reference on seeded synthetic maps.  Runs only where
the reference checkout is present (oracle/refshim.py finds it):

    python tools/gen_golden_render_eval.py

What runs:
  compute_psnr of the UNMODIFIED P/utils/save_rendered_img.py (:10-20), loaded by path.  The file imports cv2, imageio, skimage
      and tqdm at its top; whichever of them does not import here is replaced by an empty stub module while the file loads
      (compute_psnr uses none of them).
  The panel expression of COOCC_Ray.simple_test (P/coocc/detectors/coocc_ray.py:629-637), written here in our own words, the
      reference's lines cited at each step: that code sits in the middle of simple_test and cannot be called on its own.
  The squared depth error of save_rendered_img (:58), summed in float64 over the pixels with gt_depth > 0.

Maps: N = 3 views of 32 x 48.  Colours and images reach outside [0, 1] (the clip); view 1 has a constant depth map (dmax == dmin:
the 1e-8 path), view 2 has negative depths; a third of gt_depth is 0 (invalid).  Values are multiples of 1/1024 so the fixture
compresses.  The file is written with fixed zip timestamps: running this again gives the same bytes."""
import importlib
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import refshim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "render_eval.npz")
N, H, W = 3, 32, 48


def load_reference_module():
    stubbed = []
    for name in ("cv2", "imageio", "skimage", "skimage.metrics", "tqdm"):
        try:
            importlib.import_module(name)
        except Exception:
            m = types.ModuleType(name)
            if name == "skimage.metrics":
                m.structural_similarity = None
                sys.modules["skimage"].metrics = m
            if name == "tqdm":
                m.tqdm = None
            sys.modules[name] = m
            stubbed.append(name)
    path = os.path.join(refshim.PLUGIN, "utils", "save_rendered_img.py")
    spec = importlib.util.spec_from_file_location("projects.mmdet3d_plugin.utils.save_rendered_img", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name in stubbed:
        sys.modules.pop(name, None)
    return mod, stubbed


def q(a):
    return (np.round(a * 1024.0) / 1024.0).astype(np.float32)


def make_maps(seed=20):
    rs = np.random.RandomState(seed)
    rgbs = q(-0.2 + 1.4 * rs.rand(N, H, W, 3))
    gt_img = q(-0.3 + 1.6 * rs.rand(N, 3, H, W))
    gt_img[0] = q(np.clip(rgbs[0].transpose(2, 0, 1) + 0.05 * rs.randn(3, H, W), -0.3, 1.3))     # a view that is close: high PSNR
    depths = q(2.0 + 56.0 * rs.rand(N, H, W))
    depths[1] = 7.25
    depths[2] = q(-3.0 + 9.0 * rs.rand(H, W))
    gt_depth = q(1.0 + 58.0 * rs.rand(N, H, W))
    gt_depth[rs.rand(N, H, W) < 1.0 / 3.0] = 0.0
    return rgbs, depths, gt_img, gt_depth


def main():
    assert refshim.available(), "the reference checkout is not present"
    ref, stubbed = load_reference_module()
    rgbs_np, depths_np, gt_np, gtd_np = make_maps()
    rgbs, depths, gt_img = torch.from_numpy(rgbs_np), torch.from_numpy(depths_np), torch.from_numpy(gt_np)
    panels, psnrs = [], []
    psnr_total = 0                                                        # :609
    for v in range(rgbs.shape[0]):                                        # :629
        span = depths[v].max() - depths[v].min() + 1e-8                   # :630, the denominator
        depth_ = ((depths[v] - depths[v].min()) / span).unsqueeze(-1).repeat(1, 1, 3)            # :630
        panel = torch.cat([rgbs[v], gt_img[v].permute(1, 2, 0), depth_], dim=1).clip(0, 1)       # :631
        panels.append(np.uint8(panel.cpu().numpy() * 255.0))             # :632
        psnr = ref.compute_psnr(rgbs[v], gt_img[v].permute(1, 2, 0), mask=None)                 # :633, the reference's function
        psnr_total += psnr                                                # :634
        psnrs.append(psnr)
    psnr_mean = psnr_total / rgbs.shape[0]                                # :636, the value upstream prints
    assert all(p.dtype == np.float32 for p in psnrs) and np.asarray(psnr_mean).dtype == np.float32
    # float64 evaluations of the same quantities (the judge of the fp32 numbers)
    d64 = rgbs_np.astype(np.float64) - gt_np.transpose(0, 2, 3, 1).astype(np.float64)
    sq_rgb = (d64 ** 2).reshape(N, -1).sum(1)
    psnr64 = -10.0 * np.log(sq_rgb / (3.0 * H * W)) / np.log(10.0)
    valid = gtd_np > 0
    e64 = (depths_np.astype(np.float64) - gtd_np.astype(np.float64)) ** 2              # save_rendered_img.py:58, per pixel
    arrays = dict(rgbs=rgbs_np, depths=depths_np, gt_img=gt_np, gt_depth=gtd_np,
                  panels=np.stack(panels), psnr=np.asarray(psnrs, np.float32), psnr_mean=np.float32(psnr_mean),
                  psnr64=psnr64, sq_rgb64=sq_rgb,
                  depth_min=depths_np.reshape(N, -1).min(1), depth_max=depths_np.reshape(N, -1).max(1),
                  depth_sq_err64=(e64 * valid).reshape(N, -1).sum(1), depth_valid=valid.reshape(N, -1).sum(1).astype(np.int64))
    assert arrays["depth_min"][1] == arrays["depth_max"][1] and (rgbs_np > 1).any() and (rgbs_np < 0).any() and (gt_np > 1).any()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with zipfile.ZipFile(OUT, "w") as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, np.asarray(arrays[k]))
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print("stubbed while loading the reference file:", stubbed or "nothing")
    print("psnr", arrays["psnr"], "mean", arrays["psnr_mean"], "psnr64", psnr64)
    print("wrote %s (%.0f kB)" % (OUT, os.path.getsize(OUT) / 1e3))


if __name__ == "__main__":
    main()
