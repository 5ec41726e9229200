"""LiDAR depth maps on the device (co_occ_amd/depth_maps.py, csrc/depth_maps.hip): everything bit for bit against the numpy float32
restatement run on the CPU (tests/depth_map_refs.py) and the torch-made golden file -- never against live torch (that comparison is
test_depth_maps_host.py's).  The kernel gives a thread one point, 256 threads a block; a pixel holds the minimum valid depth."""
import os

import numpy as np
import pytest
import torch

import depth_map_refs as D
import image_input_refs as R
from conftest import GOLDEN
from co_occ_amd import depth_maps as DM, image_inputs as II
from co_occ_amd._lib import CooccError

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def np_mats(mats):
    return [m.numpy() if isinstance(m, torch.Tensor) else m for m in mats]


def device_maps(dev, pts, mats, size, **kw):
    table = DM.camera_table(*mats).to(dev)
    p = pts if isinstance(pts, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pts))
    got = DM.points_to_depth_maps(p.to(dev), table, size, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (table.shape[0],) + tuple(size) and got.is_contiguous()
    return got.cpu().numpy()


def check(dev, pts, mats, size):
    got = device_maps(dev, pts, mats, size)
    want = D.restatement(np.asarray(pts)[:, :3], *np_mats(mats), size)
    assert same_bits(got, want), "%d of %d pixels differ" % (int((bits(got) != bits(want)).sum()), got.size)
    return got


def shifted_rig(N):
    """N identity cameras that differ in post_tran (and the last in a mirror), so that every camera's map is its own."""
    rots, trans, intrins, post_rots, post_trans = D.identity_rig(N)
    for n in range(N):
        post_trans[n, 0], post_trans[n, 1] = 1.5 * n, -0.75 * n
    if N > 1:
        post_rots[N - 1, 0, 0] = -1.0
        post_trans[N - 1, 0] = 30.0
    return rots, trans, intrins, post_rots, post_trans


_FULL = {}


def full_reference(name):
    """35 000 points in the six cameras of the synthetic rig at a config's size: made once, shared, never changed."""
    if name not in _FULL:
        cfg = getattr(R, name)
        mats, pts = D.rig(cfg), D.cloud(35000, seed=1)
        want = D.restatement(pts, *np_mats(mats), cfg['input_size'])
        want.setflags(write=False)
        _FULL[name] = (mats, pts, want)
    return _FULL[name]


# ------------------------------------------------------------------ the identity camera, hand-placed points
def test_hand_placed_points(dev):
    """u and v at 0, at W-1 / H-1 and one ulp past; halves to even; -0.0; d = 0, negative and the smallest denormal; NaN and
    infinities; two and three points in a pixel in both memory orders; equal depths."""
    pts, want = D.edge_points()
    got = check(dev, pts, D.identity_rig(), (5, 7))
    assert same_bits(got[0], want)
    # every point alone: what is dropped writes nothing, what lands lands where the restatement says
    for i in range(len(pts)):
        check(dev, pts[i:i + 1], D.identity_rig(), (5, 7))
    back = check(dev, pts[::-1].copy(), D.identity_rig(), (5, 7))
    assert same_bits(back, got)


@pytest.mark.parametrize("P", D.P_CASES)
def test_point_counts(dev, P):
    got = check(dev, D.front_cloud(P, 24, 40, seed=2), shifted_rig(2), (24, 40))
    assert got.any() == (P > 0)


@pytest.mark.parametrize("C", [3, 4, 5])
def test_point_stride(dev, C):
    pts = D.front_cloud(300, 24, 40, seed=3)
    wide = D.cloud(300, seed=4, C=C)
    wide[:, :3] = pts
    got = check(dev, wide, shifted_rig(2), (24, 40))
    assert same_bits(got, D.restatement(pts, *np_mats(shifted_rig(2)), (24, 40))) and got.any()


def test_non_contiguous_column_slice(dev):
    wide = D.cloud(300, seed=5, C=6)
    wide[:, 1:4] = D.front_cloud(300, 24, 40, seed=6)
    sl = torch.from_numpy(wide).to(dev)[:, 1:5]
    assert not sl.is_contiguous()
    got = DM.points_to_depth_maps(sl, DM.camera_table(*shifted_rig(2)).to(dev), (24, 40)).cpu().numpy()
    assert same_bits(got, D.restatement(wide[:, 1:4], *np_mats(shifted_rig(2)), (24, 40))) and got.any()


@pytest.mark.parametrize("N", D.N_CASES)
def test_camera_counts(dev, N):
    got = check(dev, D.front_cloud(500, 24, 40, seed=7), shifted_rig(N), (24, 40))
    assert all(got[n].any() for n in range(N)) and (N == 1 or not same_bits(got[0], got[N - 1]))


@pytest.mark.parametrize("size", D.SIZE_CASES)
def test_map_sizes(dev, size):
    assert check(dev, D.front_cloud(700, size[0], size[1], seed=8), shifted_rig(2), size).any()


# ------------------------------------------------------------------ contention
def test_one_pixel_takes_4096_points(dev):
    z = (1.0 + np.random.default_rng(9).permutation(4096) / 4096.0).astype(np.float32)          # distinct, z / z = 1 exactly
    pts = np.stack([z, z, z], 1)
    got = check(dev, pts, D.identity_rig(), (2, 2))
    assert got[0, 1, 1] == z.min() == 1.0 and np.count_nonzero(got) == 1


def test_100000_points_over_nine_pixels(dev):
    pts = D.front_cloud(100000, 3, 3, seed=10)
    got = check(dev, pts, D.identity_rig(), (3, 3))
    assert np.count_nonzero(got) == 9


# ------------------------------------------------------------------ out=, determinism
def test_out_is_overwritten_everywhere(dev):
    mats, pts = shifted_rig(2), D.front_cloud(50, 24, 40, seed=11)
    out = torch.full((2, 24, 40), 77.0, device=dev)
    table = DM.camera_table(*mats).to(dev)
    got = DM.points_to_depth_maps(torch.from_numpy(pts).to(dev), table, (24, 40), out=out)
    assert got is out
    want = D.restatement(pts, *np_mats(mats), (24, 40))
    assert same_bits(out.cpu().numpy(), want) and (want == 0).sum() > 1500
    none = DM.points_to_depth_maps(torch.empty((0, 3), device=dev), table, (24, 40), out=out)          # P == 0: the fill alone
    assert none is out and not out.any()
    with pytest.raises(ValueError, match="out must be"):
        DM.points_to_depth_maps(torch.from_numpy(pts).to(dev), table, (24, 40), out=torch.empty((2, 24, 41), device=dev))


def test_two_runs_and_a_permutation_give_the_same_bits(dev):
    mats, pts, want = full_reference("R50")
    a = device_maps(dev, pts, mats, (256, 704))
    b = device_maps(dev, pts, mats, (256, 704))
    c = device_maps(dev, pts[np.random.default_rng(12).permutation(len(pts))], mats, (256, 704))
    assert same_bits(a, b) and same_bits(a, c) and same_bits(a, want)


# ------------------------------------------------------------------ full size, the golden case
@pytest.mark.parametrize("name", ["R50", "R101"])
def test_full_size(dev, name):
    mats, pts, want = full_reference(name)
    got = device_maps(dev, pts, mats, getattr(R, name)['input_size'])
    assert same_bits(got, want) and np.count_nonzero(want) > 1000


def test_golden_case(dev):
    g = np.load(os.path.join(GOLDEN, "depth_maps.npz"))
    mats = [torch.from_numpy(g[k]) for k in ("rots", "trans", "intrins", "post_rots", "post_trans")]
    got = device_maps(dev, g["points"], mats, D.SMALL['input_size'])
    assert same_bits(got, g["maps"]) and np.count_nonzero(got) == int(g["valid"].sum())


def test_captured_graph_replays_on_new_points(dev):
    mats = shifted_rig(2)
    table = DM.camera_table(*mats).to(dev)
    a, b = D.front_cloud(257, 24, 40, seed=13), D.front_cloud(257, 24, 40, seed=14)
    static = torch.from_numpy(a).to(dev)
    out = torch.empty((2, 24, 40), device=dev)
    DM.points_to_depth_maps(static, table, (24, 40), out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        DM.points_to_depth_maps(static, table, (24, 40), out=out)
    static.copy_(torch.from_numpy(b))
    g.replay()
    torch.cuda.synchronize()
    eager = DM.points_to_depth_maps(torch.from_numpy(b).to(dev), table, (24, 40))
    assert same_bits(out.cpu().numpy(), eager.cpu().numpy()) and same_bits(out.cpu().numpy(), D.restatement(b, *np_mats(mats), (24, 40)))
    assert not same_bits(out.cpu().numpy(), D.restatement(a, *np_mats(mats), (24, 40)))


@pytest.mark.parametrize("corunner", ["h2p", "wino"])
def test_bit_stable_beside_matrix_core_work(dev, corunner):
    import test_gpu_corunner as C
    S = C._scene(dev)
    mats, pts, want = full_reference("R50")
    table, p = DM.camera_table(*mats).to(dev), torch.from_numpy(pts).to(dev)
    ref, got = C._run_beside(S, lambda: [DM.points_to_depth_maps(p, table, (256, 704))], n=20, corunner=corunner)
    assert len(got) == 20 and C._count_differing(ref, got) == 0 and same_bits(ref[0].cpu().numpy(), want)


# ------------------------------------------------------------------ the loader and the pipeline step
def test_loader_fills_the_depth_slot(dev):
    import test_gpu_image_inputs as T
    frames = np.stack([R.frame(900, 1600, "random", seed=40 + i) for i in range(6)])
    want14, _, infos, l2c = T.full_reference("R50", frames)
    pts = D.cloud(35000, seed=1, C=5)                                  # a nuScenes [P,5] cloud from the host, unsliced
    load = II.LoadMultiViewFrames(R.R50, device=dev)
    twelve, extras = load(list(frames), infos, l2c, points=pts)
    assert len(twelve) == 12 and twelve[6].is_cuda and tuple(twelve[6].shape) == (6, 256, 704)
    want = D.restatement(pts, *np_mats(want14[1:6]), (256, 704))
    assert same_bits(twelve[6].cpu().numpy(), want) and np.count_nonzero(want) > 1000
    assert same_bits(extras["depth_table"].cpu().numpy(), DM.camera_table(*want14[1:6]).numpy())
    fourteen = II.with_bda(twelve)
    assert tuple(fourteen[7].shape) == (1, 6, 256, 704) and same_bits(fourteen[0][0].cpu().numpy(), want14[0].numpy())
    # device points, and the same loader without points: the reference loader's [N,1] zeros, no table
    again, _ = load(torch.from_numpy(frames).to(dev), infos, l2c, points=torch.from_numpy(pts).to(dev))
    assert same_bits(again[6].cpu().numpy(), want)
    plain, plain_extras = load(torch.from_numpy(frames).to(dev), infos, l2c)
    assert tuple(plain[6].shape) == (6, 1) and not plain[6].any() and "depth_table" not in plain_extras
    # CreateDepthFromLiDAR's camera form on that tuple (its matrices live on the device) gives the same maps
    step = DM.CreateDepthFromLiDAR(device=dev)(pts, plain)
    assert len(step) == 12 and same_bits(step[6].cpu().numpy(), want) and all(step[i] is plain[i] for i in (0, 1, 5, 7, 11))


def test_loader_training_draws(dev):
    """Training mode with a seeded generator (five of six cameras, per-camera resize, crop and flip): the restatement on the
    parameters the loader reports."""
    cfg = dict(R.TRAIN, input_size=(96, 160))
    frames = {c: R.frame(225, 400, "random", seed=80 + i) for i, c in enumerate(R.CAMS)}
    infos, l2c = R.synthetic_calibration()
    pts = D.cloud(35000, seed=15, C=4, sigma=(20.0, 20.0, 20.0))
    load = II.LoadMultiViewFrames(cfg, is_train=True, device=dev, rng=np.random.RandomState(3))
    twelve, extras = load(frames, infos, l2c, points=pts)
    names, params = list(extras["cam_names"]), extras["params"]
    assert len(names) == 5 and any(p["flip"] for p in params) and not all(p["flip"] for p in params)
    cols = [[] for _ in range(5)]
    for c, p in zip(names, params):
        s2l = torch.tensor(np.asarray(l2c[c], np.float64)).inverse().float()
        rot, tran = R.post_matrices(p["resize"], p["crop"], bool(p["flip"]))
        for lst, m in zip(cols, (s2l[:3, :3], s2l[:3, 3], torch.Tensor(infos[c]['cam_intrinsic']), rot, tran)):
            lst.append(m)
    want = D.restatement(pts, *[torch.stack(c).numpy() for c in cols], (96, 160))
    assert same_bits(twelve[6].cpu().numpy(), want) and all(want[n].any() for n in range(5))


def test_lidar_only_form(dev):
    cfg = dict(R.R50, input_size=(96, 160))
    infos, l2c = R.synthetic_calibration()
    pts = D.cloud(35000, seed=16, C=5, sigma=(20.0, 20.0, 20.0))
    make = DM.CreateDepthFromLiDAR(cfg, is_train=True, device=dev)
    nine = make.lidar_only(pts, infos, l2c)
    host, size = make.lidar_only_matrices(infos, l2c)
    assert len(nine) == 9 and size == (96, 160) and tuple(nine[8]) == (96, 160)
    assert tuple(nine[0].shape) == (6, 96, 160) and not nine[0].any() and all(t.is_cuda for t in nine[:8])
    for i, k in enumerate(("rots", "trans", "intrins", "post_rots", "post_trans", "sensor2sensors"), start=1):
        assert same_bits(nine[i].cpu().numpy(), host[k].numpy()), k
    want = D.restatement(pts, *[host[k].numpy() for k in ("rots", "trans", "intrins", "post_rots", "post_trans")], (96, 160))
    assert same_bits(nine[7].cpu().numpy(), want) and want.any()
    from co_occ_amd.detector import COOCC_Ray_L
    g = DM.lidar_gt_depths(nine)
    assert len(g) == 8 and g[COOCC_Ray_L.DEPTH_GT_INDEX][0].data_ptr() == nine[7].data_ptr()


# ------------------------------------------------------------------ consumers
def test_depth_loss_reads_the_device_made_maps(dev):
    from co_occ_amd import losses
    # depths inside the bins of dbound = [2, 10, 1]: the nearest point of a 16 x 16 block is its label
    mats, pts = shifted_rig(2), D.front_cloud(200, 32, 48, seed=17, zlo=4.0, zhi=9.5)
    made = DM.points_to_depth_maps(torch.from_numpy(pts).to(dev), DM.camera_table(*mats).to(dev), (32, 48))[None]
    uploaded = torch.from_numpy(D.restatement(pts, *np_mats(mats), (32, 48))).to(dev)[None]
    preds = torch.softmax(torch.randn(2, 8, 2, 3, generator=torch.Generator().manual_seed(18)), 1).to(dev)
    out = []
    for maps in (made, uploaded):
        x = preds.clone().requires_grad_(True)
        loss = losses.depth_loss_device(x, maps, 16, [2.0, 10.0, 1.0], 8, 3.0)
        loss.backward()
        out.append((loss.detach().cpu().numpy(), x.grad.cpu().numpy()))
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1]) and float(out[0][0]) > 0


def test_render_eval_accepts_the_maps(dev):
    from co_occ_amd import evaluation as E
    mats, pts = shifted_rig(2), D.front_cloud(3000, 32, 48, seed=19)
    made = DM.points_to_depth_maps(torch.from_numpy(pts).to(dev), DM.camera_table(*mats).to(dev), (32, 48))
    want = D.restatement(pts, *np_mats(mats), (32, 48))
    depths = (torch.rand(2, 32, 48, generator=torch.Generator().manual_seed(20)) * 40).to(dev)
    a = E.render_eval(None, depths, None, gt_depth=made)
    b = E.render_eval(None, depths, None, gt_depth=torch.from_numpy(want).to(dev))
    assert a["depth_valid"].cpu().tolist() == [int((want[n] > 0).sum()) for n in range(2)]
    assert torch.equal(a["depth_sq_err"].cpu(), b["depth_sq_err"].cpu()) and float(a["depth_sq_err"].sum()) > 0


# ------------------------------------------------------------------ refusals
def test_refusals(dev):
    mats = shifted_rig(2)
    table = DM.camera_table(*mats).to(dev)
    pts = torch.from_numpy(D.front_cloud(10, 24, 40)).to(dev)
    with pytest.raises(CooccError, match="GPU only"):
        DM.points_to_depth_maps(pts.cpu(), table, (24, 40))
    with pytest.raises(CooccError, match="GPU only"):
        DM.points_to_depth_maps(pts, table.cpu(), (24, 40))
    with pytest.raises(ValueError, match="float32"):
        DM.points_to_depth_maps(pts.double(), table, (24, 40))
    with pytest.raises(ValueError, match="float32"):
        DM.points_to_depth_maps(pts, table.half(), (24, 40))
    with pytest.raises(ValueError, match=r"C >= 3"):
        DM.points_to_depth_maps(pts[:, :2], table, (24, 40))
    with pytest.raises(ValueError, match=r"C >= 3"):
        DM.points_to_depth_maps(pts.reshape(-1), table, (24, 40))
    with pytest.raises(ValueError, match="table must be"):
        DM.points_to_depth_maps(pts, table[:, :27], (24, 40))
    with pytest.raises(ValueError, match="size must be"):
        DM.points_to_depth_maps(pts, table, (0, 40))
    with pytest.raises(NotImplementedError, match="4 x 4"):
        DM.camera_table(mats[0], mats[1], torch.eye(4)[None].repeat(2, 1, 1), mats[3], mats[4])
    with pytest.raises(ValueError, match="float32"):
        II.LoadMultiViewFrames(dict(R.R50, input_size=(12, 16)), device=dev)(
            [R.frame(37, 53, "random", 1)] * 6, *R.synthetic_calibration(), points=np.zeros((4, 3), np.float64))
