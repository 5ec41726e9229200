"""tests/golden/depth_maps.npz: what the installed torch makes of a small cloud through the reference's CreateDepthFromLiDAR
(broadcast fp32 matmuls on the CPU, sort by depth, indexed assignment): two cameras of the synthetic rig, 24 x 40 maps, 4096 points
FILTERED so that no pixel is hit twice -- where several valid points round to one pixel the reference's assignment has no defined
order, and the file must not record an accident.  Stored: the points, the five matrices, torch's valid mask [P, 2], its (u, v, d) at
the valid pairs, its maps, and the torch version.

    python tools/gen_golden_depth_maps.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_map_refs as D  # noqa: E402


def main():
    H, W = D.SMALL['input_size']
    mats = D.rig(D.SMALL, cams=D.GOLDEN_CAMS)
    pts = D.cloud(8 * D.GOLDEN_POINTS, seed=77)
    u, v, d = D.torch_projection(pts, *mats)
    _, ok = D.torch_maps(u, v, d, H, W)
    # keep a point unless one of its landings is a pixel an earlier kept point landed in
    taken, keep = set(), []
    for i in range(pts.shape[0]):
        cells = [(n, int(v[i, n].round()), int(u[i, n].round())) for n in range(len(D.GOLDEN_CAMS)) if ok[i, n]]
        if any(c in taken for c in cells):
            continue
        taken.update(cells)
        keep.append(i)
        if len(keep) == D.GOLDEN_POINTS:
            break
    assert len(keep) == D.GOLDEN_POINTS
    pts = pts[keep]
    u, v, d = D.torch_projection(pts, *mats)
    maps, ok = D.torch_maps(u, v, d, H, W)
    assert int(ok.sum()) == int((maps != 0).sum()) > 100, "a pixel is hit twice, or hardly any"
    out = dict(torch_version=np.array(torch.__version__), points=pts, valid=ok.numpy(),
               uvd=torch.stack([u[ok], v[ok], d[ok]], 1).numpy(), maps=maps.numpy())
    for k, m in zip(("rots", "trans", "intrins", "post_rots", "post_trans"), mats):
        out[k] = m.numpy()
    path = os.path.join(ROOT, "tests", "golden", "depth_maps.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, torch", torch.__version__, "valid pairs", int(ok.sum()))


if __name__ == "__main__":
    main()
