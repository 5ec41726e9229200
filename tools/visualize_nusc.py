"""Pictures of saved predictions: step 2 of the reference's predict-and-visualize workflow (its
projects/mmdet3d_plugin/visualize/visualize_nusc.py PRED_DIR SAVE_PATH), rendered on the device without mayavi.

    python tools/visualize_nusc.py PRED_DIR SAVE_PATH [--occ-size 200 200 16] [--pc-range -51.2 -51.2 -5.0 51.2 51.2 3.0]

PRED_DIR holds the ``<token>.pkl`` files of the test loop's ``--pred-save`` (``co_occ_amd.apis.save_output_nuscenes``: ``pred_voxels``,
``cam2lidar``, ``img_canvas``).  Per sample SAVE_PATH receives ``<token>_assets/<VIEW>.png`` for the six cameras, DRIVING_VIEW and
BIRD_EYE_VIEW, and ``<token>_cat_vis.png``; samples whose picture exists are skipped.  The defaults are the reference's hard-coded
nuScenes grid."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from co_occ_amd import visualize as VZ  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("pred_dir")
    ap.add_argument("save_path")
    ap.add_argument("--occ-size", type=int, nargs=3, default=VZ.NUSC_OCC_SIZE)
    ap.add_argument("--pc-range", type=float, nargs=6, default=VZ.NUSC_PC_RANGE)
    a = ap.parse_args()
    done = VZ.visualize_saved(a.pred_dir, a.save_path, a.occ_size, a.pc_range)
    print("wrote %d pictures into %s" % (len(done), a.save_path))


if __name__ == "__main__":
    main()
