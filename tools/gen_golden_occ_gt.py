"""tests/golden/occ_gt.npz: what the installed torch and numpy make of a small occupancy sample through the reference's three
loaders on the CPU -- grid 8 x 6 x 4 over [-4, -3, -5, 4, 3, 3], flips (dx, dz), 230 annotation rows (every voxel once, then repeats), a 700-point cloud with lidarseg
bytes, two cameras of the synthetic rig at 24 x 40.  Stored: the inputs, torch's project_points (u, v, d) of the row centres, the
visible flags of the sequential z-buffer, and the volumes of the sequential vote (forms A, B, C, the camera and LiDAR masks), aabb.

    python tools/gen_golden_occ_gt.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_map_refs as D  # noqa: E402
import occ_gt_refs as G  # noqa: E402

FLIP = (True, False, True)


def main():
    H, W = G.SMALL['input_size']
    mats = G.small_rig()
    np_mats = [m.numpy() for m in mats]
    bda = G.bda(0.0, *FLIP)
    occ = G.distinct_rows(G.GOLDEN_ROWS, G.GRID, seed=3)
    occ_a = G.rows(G.GOLDEN_ROWS, 4, G.GRID, seed=4, label_col=3)
    cloud = np.concatenate([G.grid_cloud(700 - len(G.border_points()), seed=5), np.pad(G.border_points(), ((0, 0), (0, 2)))]).astype(np.float32)
    seg = G.seg_bytes(cloud.shape[0], G.LEARNING_MAP, seed=6)
    pose = G.pose_fields(1)
    centres, _, _ = G.occupancy2_rows(occ, G.GRID, G.PC_RANGE, bda)
    u, v, d = D.torch_projection(torch.Tensor(centres), *mats)          # live torch, as project_points
    vol_c, pocc = G.nusc_annotations(cloud, seg, G.LEARNING_MAP, bda, G.GRID, G.PC_RANGE, 17)
    out = dict(torch_version=np.array(torch.__version__), numpy_version=np.array(np.__version__), flip=np.array(FLIP), bda=bda,
               occ=occ.astype(np.int16), occ_a=occ_a.astype(np.int16), cloud=cloud, seg=seg, uvd=torch.stack([u, v, d], -1).numpy(),
               visible=G.visible_rows(centres, np_mats, H, W), gt_a=G.load_occupancy(occ_a, G.GRID).astype(np.uint8),
               gt_b=G.load_occupancy2(occ, G.GRID, G.PC_RANGE, bda, 0),
               img_mask=G.img_visible_mask(occ, G.GRID, G.PC_RANGE, bda, np_mats, H, W),
               lidar_mask=G.lidar_visible_mask(cloud, G.GRID, G.PC_RANGE), gt_c=vol_c, points_occ=pocc, aabb=G.aabb(cloud, pose),
               pose=np.concatenate([np.asarray(pose[k], np.float64) for k in sorted(pose)]), pose_keys=np.array(sorted(pose)))
    for k, m in zip(("rots", "trans", "intrins", "post_rots", "post_trans"), np_mats):
        out[k] = m
    assert 20 < int(out["visible"].sum()) < G.GOLDEN_ROWS and int(out["img_mask"].sum()) > 5 and int(out["lidar_mask"].sum()) > 50
    path = os.path.join(ROOT, "tests", "golden", "occ_gt.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, torch", torch.__version__, "numpy", np.__version__, "visible rows", int(out["visible"].sum()),
          "img voxels", int(out["img_mask"].sum()), "lidar voxels", int(out["lidar_mask"].sum()))


if __name__ == "__main__":
    main()
