"""Occupancy pictures on the device (csrc/occ_views.hip through co_occ_amd/visualize.py): the draw volume, the masks, and per sample
the voxel, the face, t and the picture's bytes EQUAL the fp32 brute-force restatement of tests/occ_view_refs.py -- every cube asked
there, only the cubes the grid walk reaches here.  The cases and their references are shared with tests/test_occ_views_host.py,
which bounds the restatement against float64."""
import os

import numpy as np
import pytest
import torch

import occ_view_refs as R
from co_occ_amd import apis
from co_occ_amd import visualize as VZ

pytestmark = pytest.mark.gpu


def run_case(name, dev, lds_budget=None, details=True, labels=None):
    c = R.reference(name)[0]
    lab = torch.from_numpy(c["labels"] if labels is None else labels).to(dev)
    draw, masks = VZ.prepare(lab)
    out = VZ.cast_views(draw, masks, R.reference(name)[2], c["origin"], c["voxel_size"], (c["W"], c["H"]), c["S"], (c["FW"], c["FH"]), details,
                        c["lds_budget"] if lds_budget is None else lds_budget)
    return draw, masks, out, out.cell_bits if details else None


def read_image(path):
    """A written picture back as an array through PIL, which hands out R, G, B whatever library wrote the file."""
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def split_masks(masks, shape):
    """The two defined parts of the mask buffer (the bytes that pad each part to 16 are not written)."""
    X, Y, Z = shape
    zw = (Z + 15) // 16
    ncol, nbrick = X * Y * zw, ((X + 7) // 8) * ((Y + 7) // 8) * zw
    mb = masks.cpu().numpy()
    return mb[:ncol * 2].view(np.uint16), mb[(ncol * 2 + 15) // 16 * 16:][:nbrick]


def masks_of(draw):
    """The column words and brick flags of a draw volume, restated."""
    X, Y, Z = draw.shape
    zw = (Z + 15) // 16
    bits = np.zeros((X, Y, zw * 16), np.uint32)
    bits[:, :, :Z] = (draw > 0) & (draw < 20)
    col = (bits.reshape(X, Y, zw, 16) << np.arange(16, dtype=np.uint32)).sum(3).astype(np.uint16)
    bx, by = (X + 7) // 8, (Y + 7) // 8
    pad = np.zeros((bx * 8, by * 8, zw), np.uint16)
    pad[:X, :Y] = col
    brick = (pad.reshape(bx, 8, by, 8, zw) != 0).any((1, 3)).astype(np.uint8)
    return col, brick


@pytest.mark.parametrize("name", R.CASES)
def test_kernel_equals_the_fp32_restatement(name, dev):
    c, draw, rows, ids, faces, t = R.reference(name)
    d, m, (rgb, gi, gf, gt, reads, path), _ = run_case(name, dev)
    assert np.array_equal(d.cpu().numpy(), draw)
    col, brick = masks_of(draw)
    gcol, gbrick = split_masks(m, draw.shape)
    assert np.array_equal(gcol, col.reshape(-1)) and np.array_equal(gbrick, brick.reshape(-1))
    assert path == c["cell_bits"]
    gi, gf, gt = gi.cpu().numpy(), gf.cpu().numpy(), gt.cpu().numpy()
    print("%s: ids differ %d, faces %d, t %d of %d samples" % (name, (gi != ids).sum(), (gf != faces).sum(), (gt != t).sum(), ids.size))
    assert np.array_equal(gi, ids) and np.array_equal(gf, faces) and np.array_equal(gt, t)
    want = R.shade(draw, VZ.PALETTE, ids, faces, c["S"])
    assert np.array_equal(rgb.cpu().numpy(), want)
    # the read counters: a walk that tested a cube read its column word, and a word is read only behind a set brick flag
    reads = reads.cpu().numpy()
    assert (reads[..., 1] <= reads[..., 0]).all() and (reads[..., 1][ids >= 0] >= 1).all() and reads[..., 0].max() <= 4 * sum(draw.shape) + 64
    # without the per-sample outputs: the same picture
    assert np.array_equal(run_case(name, dev, details=False)[2].cpu().numpy(), want)


def test_global_bits_path_equals_the_lds_path(dev):
    _, _, a, pa = run_case("global_bits", dev)
    _, _, b, pb = run_case("global_bits", dev, lds_budget=0)
    assert (pa, pb) == ("global", "lds")
    for x, y in zip(a[:5], b[:5]):                              # the picture, ids, faces, t and the read counts
        assert torch.equal(x, y)
    # masks above the default budget of 16 KiB: from memory by default, in the 80 KiB form on request
    _, _, a, pa = run_case("lds80k", dev)
    _, _, b, pb = run_case("lds80k", dev, lds_budget=0)
    assert (pa, pb) == ("lds", "global") and all(torch.equal(x, y) for x, y in zip(a[:5], b[:5]))
    for name in ("grid20x11", "deep40"):
        _, _, c, pc = run_case(name, dev, lds_budget=16)
        assert pc == "global" and all(torch.equal(x, y) for x, y in zip(c[:5], run_case(name, dev)[2][:5])), name


def test_int64_labels_and_two_runs_give_the_same_bytes(dev):
    c = R.reference("grid16")[0]
    wide = c["labels"].astype(np.int64)
    wide[c["labels"] == 255] = 255 + 256 * 3                   # only the low byte counts
    d8, m8, a, _ = run_case("grid16", dev)
    d64, m64, b, _ = run_case("grid16", dev, labels=wide)
    assert torch.equal(d8, d64) and all(np.array_equal(x, y) for x, y in zip(split_masks(m8, d8.shape), split_masks(m64, d8.shape)))
    for x, y in zip(a[:5], b[:5]):
        assert torch.equal(x, y)
    assert torch.equal(VZ.draw_volume(torch.from_numpy(c["labels"]).to(dev)[None]), d8) and torch.equal(VZ.draw_volume(c["labels"], dev), d8)


def test_render_views_picks_cameras_sizes_and_the_window(dev):
    c, draw, rows, ids, faces, t = R.reference("window")
    cam2lidar = R.rig()
    rgb = VZ.render_views(c["labels"], cam2lidar, c["origin"], c["voxel_size"], views=[6, 7], size=(64, 36), samples=2, window=(20, 52),
                          device=dev)
    assert rgb.shape == (2, 36, 32, 3) and np.array_equal(rgb.cpu().numpy(), R.shade(draw, VZ.PALETTE, ids, faces, 2))
    full = VZ.render_views(c["labels"], cam2lidar, c["origin"], c["voxel_size"], views=[6, 7], size=(64, 36), samples=2, device=dev)
    assert torch.equal(full[:, :, 20:52], rgb)                  # the window is a crop of the frame, not another camera
    nine = VZ.render_views(c["labels"], None, c["origin"], c["voxel_size"], cameras=R.cameras(cam2lidar) + R.cameras(cam2lidar)[6:7],
                           size=(64, 36), samples=2, device=dev)
    assert nine.shape[0] == 9 and torch.equal(nine[8], nine[6]) and torch.equal(nine[6:8], full)
    with pytest.raises(ValueError):
        VZ.render_views(c["labels"], cam2lidar, c["origin"], [0.5, 0.5, 0.25], device=dev)


@pytest.fixture(scope="module")
def composed(dev, golden, tmp_path_factory):
    """draw_nusc_occupancy once at 16 x 16 x 16 (the golden's labels, grid and rig), files written."""
    g = golden("occ_views_ref")
    out = tmp_path_factory.mktemp("occ_views")
    inputs = [np.full((270, 480, 3), 40 + 30 * i, np.uint8) for i in range(6)]
    inputs[2] = None
    pos, foc = VZ.camera_positions(g["cam2lidar"])
    canvas = VZ.draw_nusc_occupancy(inputs, g["labels"], g["vox_origin"], g["voxel_size"], grid=np.array(g["labels"].shape),
                                    save_folder=str(out / "tok_assets"), cat_save_file=str(out / "tok_cat_vis.png"), cam_positions=pos,
                                    focal_positions=foc)
    return g, inputs, canvas, out


def test_composed_canvas_equals_the_restatement(composed):
    """End to end against the restated canvas.  Restating all 25 M samples by brute force takes hours; the canvas is restated at
    496 seeded pixels of each of the eight views, on the whole last pixel row and the whole last pixel column of each (the tails
    of the tile grid: 270 and 1080 rows and 1000 columns are no multiples of 16) -- 4 x 4 or 2 x 2 samples each --
    and, exactly, everywhere outside the views."""
    g, inputs, canvas, out = composed
    boxes = R.layout()
    assert canvas.shape == (R.CANVAS_H, R.CANVAS_W, 3)
    draw = R.draw_volume(g["labels"])
    cams = R.cameras(g["cam2lidar"])
    rng = np.random.default_rng(0)
    seen = np.zeros(canvas.shape[:2], bool)
    for v, name in enumerate(R.VIEW_KEYS):
        x0, y0, w, h = boxes[name]
        S, FW, FH, c0 = (4, R.CAM_W, R.CAM_H, 0) if v < 6 else (2, R.PRED_W, R.PRED_H, R.BEV_WINDOW[0] if v == 7 else 0)
        seen[y0:y0 + h, x0:x0 + w] = True
        px = np.concatenate([rng.integers(0, w, 492), [0, w - 1, 0, w - 1], np.arange(w), np.full(h, w - 1)])
        py = np.concatenate([rng.integers(0, h, 492), [0, 0, h - 1, h - 1], np.full(w, h - 1), np.arange(h)])
        n = px.size
        sy, sx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
        gx = ((c0 + px)[:, None] * S + sx.reshape(-1)[None]).reshape(-1)
        gy = (py[:, None] * S + sy.reshape(-1)[None]).reshape(-1)
        ids, faces, _ = R.cast_samples(draw, g["vox_origin"], g["voxel_size"], R.view_rows(cams[v:v + 1])[0], gx, gy, S, FW, FH)
        # one row of n pixels, S*S samples each, in shade's layout [V, H*S, W*S] with H = 1 and S rows of samples
        ids = ids.reshape(n, S, S).transpose(1, 0, 2).reshape(1, S, n * S)
        faces = faces.reshape(n, S, S).transpose(1, 0, 2).reshape(1, S, n * S)
        want = R.shade(draw, VZ.PALETTE, ids, faces, S)[0, 0]
        got = canvas[y0 + py, x0 + px]
        assert np.array_equal(got, want), "%s: %d of %d pixels differ" % (name, (got != want).any(1).sum(), n)
        assert (ids >= 0).any() and (name == "CAM_FRONT" or (ids < 0).any()), name       # cubes and, the front camera aside, sky
    for i in range(6):
        x0, y0, w, h = boxes["input%d" % i]
        seen[y0:y0 + h, x0:x0 + w] = True
        assert (canvas[y0:y0 + h, x0:x0 + w] == (0 if inputs[i] is None else inputs[i])).all()
    assert (canvas[~seen] == 0).all()


def test_composed_files_and_the_saved_loop(composed, dev):
    g, inputs, canvas, out = composed
    boxes = R.layout()
    assert np.array_equal(read_image(out / "tok_cat_vis.png"), canvas)
    for name in R.VIEW_KEYS:
        x0, y0, w, h = boxes[name]
        # two of the files byte by byte without an imaging library (pure Python: the small ones), the others through PIL
        got = R.read_png(str(out / "tok_assets" / (name + ".png"))) if name in ("CAM_FRONT_LEFT", "CAM_BACK") else read_image(
            out / "tok_assets" / (name + ".png"))
        assert np.array_equal(got, canvas[y0:y0 + h, x0:x0 + w]), name
    # the files hold R, G, B: the ego car's top faces keep the table's bytes (0, 255, 127) in the bird's-eye picture; no
    # row of the table reads (127, 255, 0), so swapped channels could not show it
    x0, y0, w, h = boxes["BIRD_EYE_VIEW"]
    colours = {tuple(p) for p in read_image(out / "tok_assets" / "BIRD_EYE_VIEW.png").reshape(-1, 3).tolist()}
    assert (0, 255, 127) in colours
    # apis.visualize_result: the same picture from a result's tensors, no pickle; missing img_canvas leaves the boxes black
    rots = torch.from_numpy(g["cam2lidar"][None, :, :3, :3]).float().to(dev)
    trans = torch.from_numpy(g["cam2lidar"][None, :, :3, 3]).float().to(dev)
    vox = torch.from_numpy(g["labels"]).to(dev)[None].long()
    again = apis.visualize_result((None, rots, trans), vox, None, str(out / "direct.png"), vox_origin=g["vox_origin"],
                                  voxel_size=g["voxel_size"])
    x0, y0, w, h = boxes["DRIVING_VIEW"]
    assert np.array_equal(again[y0:], canvas[y0:]) and (again[:y0, :boxes["CAM_FRONT_LEFT"][0]] == 0).all()
    assert os.path.exists(out / "direct.png")
    # visualize_saved: the loop over the pickles of save_output_nuscenes skips finished samples
    pred = out / "pred"
    apis.save_output_nuscenes((None, rots, trans), vox, str(pred), "scene", "tok", None, 0, None)
    # the default grid is nuScenes' 200 x 200 x 16 range: the 16^3 volume is drawn with --occ-size / --pc-range
    pc_range = list(g["vox_origin"]) + list(g["vox_origin"] + 16 * g["voxel_size"])
    done = VZ.visualize_saved(str(pred), str(out / "vis"), occ_size=[16, 16, 16], pc_range=pc_range)
    assert [os.path.basename(p) for p in done] == ["tok_cat_vis.png"]
    # float32 rots / trans round the rig: the saved picture is compared where rounding cannot show, the bird's-eye view
    x0, y0, w, h = boxes["BIRD_EYE_VIEW"]
    assert np.array_equal(read_image(done[0])[y0:y0 + h, x0:x0 + w], canvas[y0:y0 + h, x0:x0 + w])
    assert VZ.visualize_saved(str(pred), str(out / "vis"), occ_size=[16, 16, 16], pc_range=pc_range) == []
