"""Worker of test_gpu_render_kernels.test_two_phase_in_kernel_geometry_form: a fresh process whose environment holds
COOCC_RENDER_GEO_LDS=1 (the library reads the knob once per process), so that ``coocc_render_nearest_cams`` launches the two-phase
form k_render_nearest<.., .., true> instead of the LDS-free k_render_rays_geo.  Runs every camera case of tests/render_refs.py with
raw and activated tables and saves the maps to the .npz file named on the command line; the parent judges them."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(path):
    import numpy as np
    import torch
    import render_refs as R
    assert os.environ.get("COOCC_RENDER_GEO_LDS") == "1", "the parent sets COOCC_RENDER_GEO_LDS=1"
    dev = torch.device("cuda:0")
    out = {}
    for H, W, D, b in R.CAM_CASES:
        for act in (0, 1):
            out["%s_a%d" % (R.cam_name(H, W, D, b), act)] = R.run_cams(dev, H, W, D, b, act).numpy()
    torch.cuda.synchronize()
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
