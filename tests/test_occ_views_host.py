"""Occupancy pictures, the parts that need no GPU: the restatement (tests/occ_view_refs.py) and the package's host code
(co_occ_amd/visualize.py) against what the unmodified reference hands to mayavi (tests/golden/occ_views_ref.npz,
tools/gen_golden_occ_views.py); the palette rule, the layout, the refusals; and the fp32 cast against its float64 anchor."""
import ctypes

import numpy as np
import pytest

import occ_view_refs as R
from co_occ_amd import _lib
from co_occ_amd import visualize as VZ

CAMERA_FIELDS = ("position", "focal_point", "view_angle", "view_up", "clipping_range")


@pytest.fixture(scope="module")
def gold(golden):
    return golden("occ_views_ref")


def test_cube_list_and_colours_equal_the_reference(gold):
    """The drawn voxels in linear order, their centres (fp32), their scalars, the cube edge and the colour mapping are what
    points3d receives from the reference."""
    labels, origin, vs = gold["labels"], gold["vox_origin"], gold["voxel_size"]
    assert set(range(18)) <= set(labels.reshape(-1).tolist()) and (labels == 255).any()
    draw = R.draw_volume(labels)
    lin = np.flatnonzero((draw.reshape(-1) > 0) & (draw.reshape(-1) < 20))
    ijk = np.unravel_index(lin, draw.shape)
    ctr = [(origin[a] + (ijk[a] + 0.5) * vs[a]).astype(np.float32) for a in range(3)]
    for a, key in enumerate(("points_x", "points_y", "points_z")):
        assert gold[key].dtype == np.float32 and np.array_equal(ctr[a], gold[key]), key
    assert np.array_equal(draw.reshape(-1)[lin].astype(np.float32), gold["points_s"])
    assert 2.0 * R.cube_half(vs) == float(gold["scale_factor"]) == 2.0 * VZ.cube_half(vs)
    # VTK maps vmin .. vmax linearly onto the table's rows: 1 .. 19 onto 19 rows is row v - 1
    assert float(gold["vmin"]) == 1.0 and float(gold["vmax"]) == 19.0 and gold["lut_table"].shape == (19, 4)
    assert np.array_equal(VZ.PALETTE, gold["lut_table"]) and np.array_equal(VZ.PALETTE, gold["palette"])
    assert np.array_equal(gold["figure_bgcolor"], [1.0, 1.0, 1.0])             # the background byte 255
    assert int(gold["figure_size"][0]) * 9 == int(gold["figure_size"][1]) * 16  # 16 : 9


def test_cameras_equal_the_reference(gold):
    for cams in (R.cameras(gold["cam2lidar"]), VZ.view_cameras(gold["cam2lidar"])):
        assert len(cams) == 8
        for f in CAMERA_FIELDS:
            got = np.stack([np.asarray(c[f], np.float64) for c in cams])
            assert np.array_equal(got, gold["camera_" + f]), f
    pos, foc = VZ.camera_positions(gold["cam2lidar"])
    assert np.array_equal(VZ.view_cameras(cam_positions=pos, focal_positions=foc)[2]["position"], gold["camera_position"][2])


def test_view_rows_match_the_restatement_and_the_birds_eye_axis_is_exact(gold):
    cams = VZ.view_cameras(gold["cam2lidar"])
    rows = VZ.view_rows(cams, 7)
    assert rows.dtype == np.float32 and np.array_equal(rows, R.view_rows(R.cameras(gold["cam2lidar"]), 7))
    assert np.array_equal(rows[7, 3:6], [0, 0, -1]) and rows[7, 7] == 0 and rows[7, 8] == 0 and rows[7, 9] == 0 and rows[7, 11] == 0
    # tan_x = tan_y * 16 / 9, the view angle is the vertical one
    assert abs(float(rows[7, 10]) - np.tan(np.radians(20.0))) < 1e-7 and abs(float(rows[7, 6]) - np.tan(np.radians(20.0)) * 16 / 9) < 1e-7
    with pytest.raises(ValueError):
        VZ.view_rows([dict(cams[0], focal_point=cams[0]["position"])])
    with pytest.raises(ValueError):
        VZ.view_rows([dict(cams[7], view_up=[0., 0., 1.])])


def test_palette_index_rule():
    draw = R.draw_volume(np.full((12, 12, 16), 17, np.uint8))
    assert set(draw.reshape(-1).tolist()) == {17, 18, 19, 20}                  # the relabelled 17 outside the block, the car inside
    assert [VZ.palette_index(v) for v in (0, 1, 16, 17, 19, 20, 255)] == [None, 0, 15, 16, 18, None, None]
    assert VZ.PALETTE.shape == (19, 4) and VZ.PALETTE.dtype == np.uint8 and tuple(VZ.SHADE) == tuple(R.SHADE)
    # the ego-car block: 8 x 8 x 6 voxels, labels banded along y and z, constant along x
    blk = draw[0:8, 0:8, 3:9]
    assert (blk == blk[:1]).all() and blk[0, 0, 0] == 17 and blk[0, 3, 0] == 18 and blk[0, 6, 0] == 19 and blk[0, 0, 2] == 18


def test_layout_boxes():
    want = {"input0": (0, 0), "input1": (490, 0), "input2": (980, 0), "input3": (0, 280), "input4": (490, 280), "input5": (980, 280),
            "CAM_FRONT_LEFT": (1470, 0), "CAM_FRONT": (1960, 0), "CAM_FRONT_RIGHT": (2450, 0), "CAM_BACK_LEFT": (1470, 280),
            "CAM_BACK": (1960, 280), "CAM_BACK_RIGHT": (2450, 280)}
    boxes = VZ.layout()
    assert boxes == R.layout() and VZ.CANVAS_SIZE == (2930, 1640) == (R.CANVAS_W, R.CANVAS_H)
    for k, (x, y) in want.items():
        assert boxes[k] == (x, y, 480, 270), k
    assert boxes["DRIVING_VIEW"] == (0, 560, 1920, 1080) and boxes["BIRD_EYE_VIEW"] == (1930, 560, 1000, 1080)
    assert VZ.BEV_WINDOW == (460, 1460) and len(boxes) == 14
    # compose: black canvas, every panel in its box, a missing input stays black
    panels = {k: np.full((boxes[k][3], boxes[k][2], 3), 10 + i, np.uint8) for i, k in enumerate(VZ.VIEW_KEYS)}
    inputs = [np.full((270, 480, 3), 100 + i, np.uint8) for i in range(6)]
    inputs[4] = None
    canvas = VZ.compose(inputs, panels)
    assert canvas.shape == (1640, 2930, 3) and canvas.dtype == np.uint8
    seen = np.zeros(canvas.shape[:2], bool)
    for i, k in enumerate(["input%d" % j for j in range(6)] + VZ.VIEW_KEYS):
        x, y, w, h = boxes[k]
        val = (100 + i) if i < 6 else 10 + i - 6
        assert (canvas[y:y + h, x:x + w] == (0 if k == "input4" else val)).all(), k
        seen[y:y + h, x:x + w] = True
    assert (canvas[~seen] == 0).all()
    assert (VZ.compose(None, {})) .max() == 0


def test_written_files_hold_rgb_whichever_library_writes(tmp_path, monkeypatch):
    """A palette colour written through visualize's writer and decoded with zlib alone is the same R, G, B -- with PIL, and with
    cv2, whose imwrite takes B, G, R (a stand-in with that contract where cv2 does not import)."""
    import sys
    import types
    pic = np.zeros((5, 7, 3), np.uint8)
    pic[:] = VZ.PALETTE[3, :3]                                                 # car: (0, 150, 245)
    pic[0, 0] = VZ.PALETTE[0, :3]                                              # barrier: (255, 120, 50)
    writers = []
    try:
        import cv2  # noqa: F401
        writers.append("cv2")
    except ImportError:
        from PIL import Image
        fake = types.ModuleType("cv2")
        fake.imwrite = lambda f, a: Image.fromarray(np.ascontiguousarray(a[..., ::-1])).save(f) or True      # B, G, R in, as cv2
        writers.append(fake)
    writers.append(None)                                                        # PIL itself
    for i, w in enumerate(writers):
        if w is None:
            monkeypatch.setitem(sys.modules, "cv2", None)                       # import cv2 fails: the PIL branch
        elif w != "cv2":
            monkeypatch.setitem(sys.modules, "cv2", w)
        writer, ext = VZ._image_writer("test")
        path = str(tmp_path / ("pic%d%s" % (i, ext)))
        writer(path, pic)
        assert ext == ".png" and np.array_equal(R.read_png(path), pic), i
        assert tuple(R.read_png(path)[2, 3]) == (0, 150, 245) and tuple(R.read_png(path)[0, 0]) == (255, 120, 50)


def test_a_cube_that_leaves_its_cell_is_refused():
    with pytest.raises(ValueError, match="cube edge"):
        VZ.cube_half([0.5, 0.5, 0.25])
    with pytest.raises(ValueError):
        VZ.cube_half([0.5, -0.5, 0.5])
    assert VZ.cube_half(0.5) == 0.5 * (0.5 - 0.05 * 0.5) and VZ.cube_half(VZ.grid_of()[1]) > 0
    origin, vs = VZ.grid_of()
    assert np.array_equal(origin, [-51.2, -51.2, -5.0]) and np.array_equal(vs, [102.4 / 200, 102.4 / 200, 0.5])


def test_entries_validate_before_launching():
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    assert lib.coocc_occ_view_prepare(None, 0, 200, 200, 16, None, None, 0, None) == 80000 + 640
    assert lib.coocc_occ_view_prepare(None, 0, 20, 20, 11, None, None, 0, None) == 800 + 16
    assert lib.coocc_occ_view_prepare(None, 0, 8, 200, 16, None, None, 0, None) == -1 and b"occ_view_prepare" in lib.coocc_last_error()
    assert lib.coocc_occ_view_prepare(one, 0, 16, 16, 16, one, one, 8, None) == -3
    grid = (ctypes.c_float * 7)(-4, -4, -4, 0.5, 0.5, 0.5, 0.2375)
    rows = R.view_rows(R.cameras(R.rig()))
    pal = np.ascontiguousarray(VZ.PALETTE[:, :3])
    args = lambda V=8, S=1, W=64, FW=64, g=grid, r=rows, ids=None: (one, one, 16, 16, 16, g, r.ctypes.data, V, 36, W, S, FW, 36, pal.ctypes.data, 0,
                                                                      one, ids, None, None, None, None)
    for bad in (args(V=9), args(S=9), args(W=65), args(ids=one), args(g=(ctypes.c_float * 7)(-4, -4, -4, 0.5, 0.5, 0.25, 0.2375))):
        assert lib.coocc_occ_view_cast(*bad) == -1 and b"occ_view_cast" in lib.coocc_last_error()
    r2 = rows.copy()
    r2[0, 14] = 1                                                               # the window would leave the frame
    assert lib.coocc_occ_view_cast(*args(r=r2)) == -1 and b"window" in lib.coocc_last_error()
    r2 = rows.copy()
    r2[3, 12] = 0.0                                                             # near must be positive
    assert lib.coocc_occ_view_cast(*args(r=r2)) == -1 and b"near" in lib.coocc_last_error()


def test_cpu_labels_are_refused():
    import torch
    with pytest.raises(_lib.CooccError):
        VZ.draw_volume(torch.zeros(16, 16, 16, dtype=torch.uint8))


@pytest.mark.parametrize("name", R.CASES)
def test_fp32_cast_against_the_float64_anchor(name):
    """At most 0.1 % of a case's samples may see another (voxel, face) in fp32 than in float64: the condition under which the
    exact comparison of the kernel with the fp32 restatement says something about the picture."""
    c, draw, rows, ids, faces, t = R.reference(name)
    ids64, faces64, t64 = R.cast(draw, c["origin"], c["voxel_size"], rows, c["H"], c["W"], c["S"], c["FW"], c["FH"], np.float64)
    differ = int(((ids != ids64) | (faces != faces64)).sum())
    hit = ids >= 0
    print("%s: %d of %d samples differ, %.1f %% hit, %d drawn cubes" % (name, differ, ids.size, 100.0 * hit.mean(),
                                                                        int(((draw > 0) & (draw < 20)).sum())))
    assert differ <= 0.001 * ids.size
    both = hit & (ids == ids64) & (faces == faces64)           # t is compared where both casts see the same face of the same cube
    assert np.abs(t[both] - t64[both]).max() <= 1e-4 * max(1.0, float(t64[both].max()))
    assert 0 < hit.sum() and (name == "eye_inside" or hit.sum() < ids.size)   # every case hits something and, the inside eye aside, misses


def test_cases_hold_what_they_are_for():
    c, draw, rows, ids, faces, t = R.reference("bev_odd")
    d = R.view_rows(c["cams"])[0]
    assert c["W"] % 2 == 1 and c["H"] % 2 == 1 and np.array_equal(d[3:6], [0, 0, -1])          # the centre sample: u = v = 0
    assert ids[0, c["H"] // 2, c["W"] // 2] >= 0 and faces[0, c["H"] // 2, c["W"] // 2] == 4     # it sees a top face
    c, draw, rows, ids, faces, t = R.reference("eye_inside")
    own = np.ravel_multi_index((16 // 2 - 3, 16 // 2 - 3, 16 // 2 - 3), draw.shape)
    assert (ids == own).all() and set(np.unique(faces)) <= {0, 1, 2, 3, 4, 5}                    # the exit faces of the eye's own cube
    c, draw, rows, ids, faces, t = R.reference("near_far")
    for v in range(2):
        h = ids[v] >= 0
        assert h.any() and t[v][h].min() >= rows[v, 12] and t[v][h].max() <= rows[v, 13]
    c, draw, rows, ids, faces, t = R.reference("far_eye")
    assert (ids[2] < 0).all() and (ids[0] >= 0).any() and (ids[1] < 0).any()
    c, draw, rows, ids, faces, t = R.reference("empty")
    assert set(np.unique(draw)) == {0, 17, 18, 19}
    c, draw, rows, ids, faces, t = R.reference("window")
    assert rows[0, 14] == 20 and c["W"] == 32 and c["FW"] == 64
