"""The LiDAR depth maps on the host (no GPU): the numpy float32 restatement (tests/depth_map_refs.py) the GPU tests are judged
against is held here against LIVE torch on the CPU -- the reference's broadcast matmuls -- and against the torch-made golden file;
plus the host halves of co_occ_amd/depth_maps.py and the C entry point's argument validation.  If torch's CPU bmm on some host ever
contracts its multiply-adds, this file shows it."""
import inspect
import os

import numpy as np
import pytest
import torch

import depth_map_refs as D
import image_input_refs as R
from conftest import GOLDEN
from co_occ_amd import _lib, depth_maps as DM, image_inputs as II, staging
from co_occ_amd._lib import CooccError

SIZES = {"R50": R.R50, "R101": R.R101}
_LIVE = {}


def same(a, b):
    """numeric equality, NaN equal to NaN (signed zeros are not observable in the maps)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def live(name):
    """Torch's and the restatement's (u, v, d) of 35 000 Gaussian points in the six cameras of the synthetic rig: once per size."""
    if name not in _LIVE:
        mats = D.rig(SIZES[name])
        pts = D.cloud(35000, seed=1)
        tu, tv, td = (t.numpy() for t in D.torch_projection(pts, *mats))
        nu, nv, nd = D.project(pts, D.inverse(mats[0]), *[m.numpy() for m in mats[1:]])
        _LIVE[name] = (mats, pts, (tu, tv, td), (nu, nv, nd))
    return _LIVE[name]


@pytest.mark.parametrize("name", list(SIZES))
def test_restatement_equals_live_torch_projection(name):
    _, _, t, n = live(name)
    assert t[0].shape == (35000, 6)
    for what, a, b in zip("uvd", t, n):
        assert same(a, b), "%s differs at %d of %d pairs" % (what, int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum()), a.size)


@pytest.mark.parametrize("name", list(SIZES))
def test_every_pixel_against_live_torch_fill(name):
    """Where exactly one valid point lands the restatement's map has torch's bits; where several land it holds their minimum and
    torch's value is one of theirs; where none lands both hold 0.  No pixel is exempt."""
    H, W = SIZES[name]['input_size']
    _, _, t, n = live(name)
    tmaps, tok = D.torch_maps(*[torch.from_numpy(x) for x in t], H, W)
    tmaps, tok = tmaps.numpy(), tok.numpy()
    ok = D.valid_mask(*n, H, W)
    assert np.array_equal(ok, tok)
    maps = D.min_maps(*n, ok, H, W)
    count = np.zeros((6, H, W), np.int64)
    for c in range(6):
        y, x = D.pixels(n[0][ok[:, c], c], n[1][ok[:, c], c])
        np.add.at(count[c], (y, x), 1)
    assert int((count == 1).sum()) > 1000
    assert np.array_equal(bits(maps[count <= 1]), bits(tmaps[count <= 1]))
    assert not maps[count == 0].any()
    for c, y, x in zip(*np.nonzero(count > 1)):
        m = ok[:, c]
        py, px = D.pixels(n[0][m, c], n[1][m, c])
        theirs = n[2][m, c][(py == y) & (px == x)]
        assert len(theirs) == count[c, y, x] and maps[c, y, x] == theirs.min() and tmaps[c, y, x] in theirs


def test_golden_file_equals_the_restatement():
    g = np.load(os.path.join(GOLDEN, "depth_maps.npz"))
    H, W = D.SMALL['input_size']
    assert g["points"].shape == (D.GOLDEN_POINTS, 3) and g["maps"].shape == (2, H, W) and str(g["torch_version"])
    u, v, d = D.project(g["points"], D.inverse(g["rots"]), g["trans"], g["intrins"], g["post_rots"], g["post_trans"])
    ok = D.valid_mask(u, v, d, H, W)
    assert np.array_equal(ok, g["valid"]) and int(ok.sum()) > 100
    assert np.array_equal(bits(np.stack([u[ok], v[ok], d[ok]], 1)), bits(g["uvd"]))
    maps = D.min_maps(u, v, d, ok, H, W)
    assert np.array_equal(bits(maps), bits(g["maps"]))
    assert int((maps != 0).sum()) == int(ok.sum())          # no pixel hit twice: the file records no accident of the assignment
    assert np.array_equal(bits(D.restatement(g["points"], g["rots"], g["trans"], g["intrins"], g["post_rots"], g["post_trans"], (H, W))),
                          bits(g["maps"]))
    # the rig the file was made from is the one the tests build
    for k, m in zip(("rots", "trans", "intrins", "post_rots", "post_trans"), D.rig(D.SMALL, cams=D.GOLDEN_CAMS)):
        assert np.array_equal(bits(m.numpy()), bits(g[k])), k


def test_edge_points_expectation_is_the_restatement():
    pts, want = D.edge_points()
    got = D.restatement(pts, *[m.numpy() for m in D.identity_rig()], (5, 7))
    assert np.array_equal(bits(got[0]), bits(want))
    assert want[0, 0] == np.nextafter(np.float32(0), np.float32(1)) and want[3, 6] == 0.5 and want[2, 2] == 32 and want[3, 2] == 64


def test_camera_table_layout_and_inverse_bits():
    mats = D.rig(R.R50)
    table = DM.camera_table(*mats)
    assert table.dtype == torch.float32 and tuple(table.shape) == (6, DM.CAM_FLOATS) and table.is_contiguous()
    t = table.numpy()
    assert np.array_equal(bits(t[:, :9]), bits(mats[0].inverse().numpy().reshape(6, 9)))
    assert np.array_equal(bits(t[:, 9:12]), bits(mats[1].numpy())) and np.array_equal(bits(t[:, 12:21]), bits(mats[2].numpy().reshape(6, 9)))
    assert np.array_equal(bits(t[:, 21:25]), bits(mats[3][:, :2, :2].numpy().reshape(6, 4)))
    assert np.array_equal(bits(t[:, 25:27]), bits(mats[4][:, :2].numpy())) and not t[:, 27].any()
    # the table alone reproduces the restatement on the matrices
    pts = D.cloud(2000, seed=3)
    assert np.array_equal(bits(D.from_table(pts, t, (256, 704))), bits(D.restatement(pts, *mats, (256, 704))))
    # 2 x 2 / length-2 post matrices are taken too
    assert torch.equal(DM.camera_table(mats[0], mats[1], mats[2], mats[3][:, :2, :2], mats[4][:, :2]), table)


def test_camera_table_refusals():
    rots, trans, intrins, post_rots, post_trans = D.rig(R.R50)
    k4 = torch.eye(4)[None].repeat(6, 1, 1)
    with pytest.raises(NotImplementedError, match="4 x 4"):
        DM.camera_table(rots, trans, k4, post_rots, post_trans)
    with pytest.raises(ValueError, match="float32"):
        DM.camera_table(rots.double(), trans, intrins, post_rots, post_trans)
    with pytest.raises(ValueError, match="float32"):
        DM.camera_table(rots.numpy(), trans, intrins, post_rots, post_trans)
    with pytest.raises(ValueError, match="rots"):
        DM.camera_table(rots[0], trans, intrins, post_rots, post_trans)
    with pytest.raises(ValueError, match="trans"):
        DM.camera_table(rots, trans[:5], intrins, post_rots, post_trans)
    with pytest.raises(ValueError, match="post_rots"):
        DM.camera_table(rots, trans, intrins, post_rots[:5], post_trans)


def test_lidar_only_matrices_have_the_reference_bits():
    """The no-image branch for the coocc_lidar data_config (896 x 1600, no augmentation): a blank image of the input size itself, so
    resize 1.0 and a crop at the origin; every matrix with the reference's float32 operations."""
    cfg = R.R101
    infos, l2c = R.synthetic_calibration()
    make = DM.CreateDepthFromLiDAR(cfg, is_train=True, rng=np.random.RandomState(4))
    got, size = make.lidar_only_matrices(infos, l2c)
    assert size == (896, 1600) and set(got) == {"rots", "trans", "intrins", "post_rots", "post_trans", "sensor2sensors"}
    for i, name in enumerate(cfg['cams']):
        s2l = torch.tensor(np.asarray(l2c[name], np.float64)).inverse().float()
        rot2, tran2 = torch.eye(2), torch.zeros(2)
        rot2 *= 1600. / 1600.
        tran2 -= torch.Tensor([0, 0])
        turn = torch.Tensor([[np.cos(0.0), np.sin(0.0)], [-np.sin(0.0), np.cos(0.0)]])
        half = torch.Tensor([1600, 896]) / 2
        rot2, tran2 = turn.matmul(rot2), turn.matmul(tran2) + (turn.matmul(-half) + half)
        post_rot, post_tran = torch.eye(3), torch.zeros(3)
        post_rot[:2, :2], post_tran[:2] = rot2, tran2
        for k, w in (("rots", s2l[:3, :3]), ("trans", s2l[:3, 3]), ("intrins", torch.Tensor(infos[name]['cam_intrinsic'])),
                     ("post_rots", post_rot), ("post_trans", post_tran), ("sensor2sensors", s2l)):
            assert got[k].dtype == torch.float32 and np.array_equal(bits(got[k][i].numpy()), bits(w.numpy())), (name, k)
    # a training config draws per camera from the generator, in the reference's order: resize, crop height, crop width, flip
    train = dict(R.TRAIN, input_size=(24, 40))
    a = DM.CreateDepthFromLiDAR(train, is_train=True, rng=np.random.RandomState(9))
    got, size = a.lidar_only_matrices(infos, l2c)
    rng = np.random.RandomState(9)
    names = rng.choice(train['cams'], train['Ncams'], replace=False)
    assert size == (24, 40) and got["rots"].shape[0] == 5
    for i, name in enumerate(names):
        resize = 40. / 40. + rng.uniform(*train['resize'])
        newW, newH = int(40 * resize), int(24 * resize)
        y0 = int((1 - rng.uniform(*train['crop_h'])) * newH) - 24
        x0 = int(rng.uniform(0, max(0, newW - 40)))
        flip = train['flip'] and rng.choice([0, 1])
        rng.uniform(*train['rot'])
        rot, tran = R.post_matrices(resize, (x0, y0, x0 + 40, y0 + 24), flip)
        assert np.array_equal(bits(got["post_rots"][i].numpy()), bits(rot.numpy())), name
        assert np.array_equal(bits(got["post_trans"][i].numpy()), bits(tran.numpy())), name
        s2l = torch.tensor(np.asarray(l2c[name], np.float64)).inverse().float()
        assert np.array_equal(bits(got["rots"][i].numpy()), bits(s2l[:3, :3].numpy()))


def test_lidar_gt_depths_is_the_tuple_the_detector_reads():
    from co_occ_amd.detector import COOCC_Ray_L
    nine = (torch.zeros(2, 4, 6), torch.rand(2, 3, 3), torch.rand(2, 3), torch.rand(2, 3, 3), torch.rand(2, 3, 3), torch.rand(2, 3),
            torch.rand(2, 4, 4), torch.rand(2, 4, 6), torch.Size([4, 6]))
    flat = DM.lidar_gt_depths(nine, batch=False)
    assert len(flat) == 8 and flat[COOCC_Ray_L.DEPTH_GT_INDEX] is nine[7] and flat[0] is nine[1] and torch.equal(flat[5], torch.eye(3))
    assert flat[-1] == (4, 6)
    b = DM.lidar_gt_depths(nine, bda_rot=2 * torch.eye(3))
    assert tuple(b[COOCC_Ray_L.DEPTH_GT_INDEX].shape) == (1, 2, 4, 6) and tuple(b[5].shape) == (1, 3, 3) and float(b[5][0, 0, 0]) == 2
    assert [int(s) for s in b[-1]] == [4, 6] and all(tuple(b[i].shape) == (1,) + tuple(nine[i + 1].shape) for i in range(5))


def test_entry_point_validates_before_launching():
    """COOCC_EINVAL and a message naming the entry point, before any launch: needs no GPU."""
    lib = _lib.load()
    one = _lib.c_void_p(16)
    ok = dict(points=one, P=8, stride=3, cams=one, N=1, H=4, W=4, maps=one)
    bad = [dict(points=None), dict(cams=None), dict(maps=None), dict(N=0), dict(H=0), dict(W=0), dict(P=-1), dict(stride=2), dict(N=-3)]
    for change in bad:
        a = dict(ok, **change)
        rc = lib.coocc_points_to_depth_maps(a["points"], a["P"], a["stride"], a["cams"], a["N"], a["H"], a["W"], a["maps"], None)
        assert rc == -1 and b"points_to_depth_maps" in lib.coocc_last_error(), change


def test_python_refusals_without_a_gpu():
    pts, table = torch.zeros(4, 3), torch.zeros(1, DM.CAM_FLOATS)
    with pytest.raises(CooccError, match="GPU only"):
        DM.points_to_depth_maps(pts, table, (4, 4))
    with pytest.raises(ValueError, match="tensor"):
        DM.points_to_depth_maps(pts.numpy(), table, (4, 4))
    stage = staging.PointStage("cuda")
    with pytest.raises(ValueError, match="float32"):
        stage(np.zeros((4, 3), np.float64))
    with pytest.raises(ValueError, match="C >= 3"):
        stage(np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError, match="data_config"):
        DM.CreateDepthFromLiDAR().lidar_only_matrices({}, {})
    with pytest.raises(ValueError, match="12-tuple"):
        DM.CreateDepthFromLiDAR()(pts, (None,) * 9)


def test_loader_without_points_is_unchanged():
    """``points`` is the last, optional argument of the loader's call and defaults to None: every earlier call means what it meant
    (the [N,1] zeros of the depth slot are asserted on the device by test_gpu_image_inputs and test_gpu_depth_maps); no
    point staging buffer exists until points are given."""
    params = list(inspect.signature(II.LoadMultiViewFrames.__call__).parameters.values())
    assert [p.name for p in params] == ["self", "frames", "cam_infos", "lidar2cam_dic", "flip", "scale", "points"]
    assert params[-1].default is None
    load = II.LoadMultiViewFrames(dict(R.R50, input_size=(8, 16)))
    assert load._point_stage is None
