"""Generate tests/golden/occ_views_ref.npz: what the UNMODIFIED reference P/visualize/visualize_nusc.py hands to mayavi for a small
seeded volume.  Runs only where the reference checkout is present (oracle/refshim.py finds it):

    python tools/gen_golden_occ_views.py

The reference file is loaded by path with stub ``mayavi`` / ``mayavi.mlab`` modules in ``sys.modules`` (and a stub ``tqdm`` where it
does not import): mayavi needs VTK and an OpenGL context.  The stubs draw nothing, they RECORD:
  points3d      the three coordinate arrays and the scalars it receives, ``scale_factor``, ``vmin`` / ``vmax``
  the figure    its size and background, and the table written into the scalar LUT
  savefig       the camera fields set at that moment -- position, focal_point, view_angle, view_up, clipping_range -- per view
and the eighth ``savefig`` ends the call (what follows reads the PNG files mayavi would have written).

Input: the 16 x 16 x 16 labels of case ``grid16`` of tests/occ_view_refs.py (every class, 0, 17 and 255 among them), its rig as
``cam2lidar``, voxels of 0.5 m -- powers of two, so the reference's fp32 ``index * size + size / 2 + origin`` and the package's
``origin + (index + 0.5) * size`` are the same numbers.  The file holds arrays only, written with fixed zip timestamps."""
import importlib
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refshim  # noqa: E402
import occ_view_refs as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "occ_views_ref.npz")
CAMERA_FIELDS = ("position", "focal_point", "view_angle", "view_up", "clipping_range")


class Done(Exception):
    pass


class Bag:
    """An object that accepts any attribute, and makes nested ones on first read."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        b = Bag()
        object.__setattr__(self, name, b)
        return b


def make_stubs(rec):
    mlab = types.ModuleType("mayavi.mlab")
    mlab.options = Bag()
    state = {}

    def figure(size=None, bgcolor=None, **kw):
        rec["figure_size"], rec["figure_bgcolor"] = np.asarray(size), np.asarray(bgcolor, np.float64)
        fig = Bag()
        fig.scene.camera.compute_view_plane_normal = lambda: None
        fig.scene.render = lambda: None
        state["fig"] = fig
        return fig

    def points3d(x, y, z, s, **kw):
        rec["points_x"], rec["points_y"], rec["points_z"], rec["points_s"] = [np.array(a) for a in (x, y, z, s)]
        rec["scale_factor"], rec["vmin"], rec["vmax"] = np.float64(kw["scale_factor"]), np.float64(kw["vmin"]), np.float64(kw["vmax"])
        assert kw["mode"] == "cube" and kw["opacity"] == 1.0
        state["plot"] = Bag()
        return state["plot"]

    def savefig(path, **kw):
        cam = state["fig"].scene.camera
        for f in CAMERA_FIELDS:
            rec.setdefault("camera_" + f, []).append(np.asarray(getattr(cam, f), np.float64))
        rec.setdefault("saved", []).append(os.path.basename(path))
        if len(rec["saved"]) == 8:
            rec["lut_table"] = np.array(state["plot"].module_manager.scalar_lut_manager.lut.table)
            raise Done

    mlab.figure, mlab.points3d, mlab.savefig, mlab.close = figure, points3d, savefig, lambda *a, **k: None
    mayavi = types.ModuleType("mayavi")
    mayavi.mlab = mlab
    return {"mayavi": mayavi, "mayavi.mlab": mlab}


def load_reference_module(stubs):
    try:
        importlib.import_module("tqdm")
    except Exception:
        stubs["tqdm"] = types.ModuleType("tqdm")
        stubs["tqdm"].tqdm = None
    sys.modules.update(stubs)
    path = os.path.join(refshim.PLUGIN, "visualize", "visualize_nusc.py")
    spec = importlib.util.spec_from_file_location("projects.mmdet3d_plugin.visualize.visualize_nusc", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import tempfile
    assert refshim.available(), "the reference checkout is not present"
    rec = {}
    stubs = make_stubs(rec)
    ref = load_reference_module(stubs)
    c = R.case("grid16")
    labels, origin, vs, cam2lidar = c["labels"], c["origin"], c["voxel_size"], R.rig()
    assert set(range(18)) <= set(labels.reshape(-1).tolist()) and (labels == 255).any()
    # the reference's __main__, its lines 258-261
    cam_positions = (cam2lidar @ np.array([0., 0., 0., 1.]))[:, :3]
    focal_positions = (cam2lidar @ np.array([0., 0., 0.0055, 1.]))[:, :3]
    with tempfile.TemporaryDirectory() as tmp:
        try:
            ref.draw_nusc_occupancy(input_imgs=[], voxels=labels, vox_origin=np.array(origin), voxel_size=np.array(vs),
                                    grid=np.array(labels.shape), pred_lidarseg=None, target_lidarseg=None,
                                    save_folder=os.path.join(tmp, "assets"), cat_save_file=os.path.join(tmp, "cat.png"),
                                    cam_positions=cam_positions, focal_positions=focal_positions)
            raise AssertionError("the reference did not stop at the eighth savefig")
        except Done:
            pass
    for k in stubs:
        sys.modules.pop(k, None)
    assert rec.pop("saved") == [k + ".png" for k in R.VIEW_KEYS]
    arrays = dict(labels=labels, vox_origin=np.asarray(origin, np.float64), voxel_size=np.asarray(vs, np.float64), cam2lidar=cam2lidar,
                  palette=np.array(ref.colors))
    for k, v in rec.items():
        arrays[k] = np.stack(v) if isinstance(v, list) else np.asarray(v)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with zipfile.ZipFile(OUT, "w") as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, np.asarray(arrays[k]))
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print({k: (v.shape, str(v.dtype)) for k, v in arrays.items()})
    print("wrote %s (%.0f kB)" % (OUT, os.path.getsize(OUT) / 1e3))


if __name__ == "__main__":
    main()
