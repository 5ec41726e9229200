"""The occupancy ground truth on the device (co_occ_amd/occ_gt.py, csrc/occ_gt.hip): every volume, mask and flag by exact integer
equality against the numpy restatements of the reference's three loaders run on the CPU (tests/occ_gt_refs.py) and against the
golden file; aabb within one fp32 step of numpy's float64 matmul (BLAS sums are not pinned) and bit-equal to the left-to-right form.
Kernels give a thread one row, 256 threads a block: the row counts straddle a wave and a block."""
import numpy as np
import pytest
import torch

import depth_map_refs as D
import image_input_refs as R
import occ_gt_refs as G
from conftest import GOLDEN
from co_occ_amd import depth_maps as DM, image_inputs as II, occ_gt as OG

pytestmark = pytest.mark.gpu

BIG_GRID, BIG_RANGE = (512, 512, 40), [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
CONF = dict(rot_lim=(0, 0), scale_lim=(0.95, 1.05), flip_dx_ratio=0.5, flip_dy_ratio=0.5, flip_dz_ratio=0.5)


class Draws:
    """an rng whose five draws give the wanted flips"""

    def __init__(self, flip):
        self.flip = flip

    def uniform(self, *a):
        self.n = getattr(self, "n", -1) + 1
        return (0.0, 1.0)[self.n % 5] if self.n % 5 < 2 else (0.25 if self.flip[self.n % 5 - 2] else 0.75)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN + "/occ_gt.npz")


def up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def rows_dev(dev, occ, label_col, grid=None):
    return up(dev, OG.pack_rows(occ, label_col, grid).view(np.int16))


def form_b(dev, occ, bda, grid=G.GRID, pc_range=G.PC_RANGE, unoccupied=0):
    vox, labels, centres = OG.rows_to_voxels(rows_dev(dev, occ, -1), grid, pc_range, bda)
    vol = OG.vote_labels(vox, labels, grid, fill=unoccupied)
    assert vol.dtype == torch.uint8 and tuple(vol.shape) == tuple(grid) and vol.is_contiguous()
    return vol.cpu().numpy(), vox, centres


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got, want), "%d of %d values differ" % (int((got != want).sum()), want.size)


# ------------------------------------------------------------------ form B and the vote
@pytest.mark.parametrize("flip", G.FLIPS)
def test_form_b_every_flip_row_count_and_stride(dev, flip):
    bda = G.bda(0.0, *flip)
    for C in (4, 7):
        for N in G.ROW_COUNTS:
            occ = G.rows(N, C, seed=21)
            got, _, _ = form_b(dev, occ, bda, unoccupied=3)
            same(got, G.load_occupancy2(occ, G.GRID, G.PC_RANGE, bda, 3))


def test_hand_made_votes(dev):
    grid = (2, 2, 2)
    pairs = np.concatenate([np.array([[0, 0, 0, 9], [0, 0, 0, 4], [0, 0, 0, 9], [0, 0, 0, 4]]),          # a tie: the lowest label
                            np.array([[0, 1, 0, 255]] * 3 + [[0, 1, 0, 7]] * 2),                          # 255 against a smaller count
                            np.array([[1, 1, 1, 3]] * 65536 + [[1, 1, 1, 5]] * 2),                        # 65 536 wrap to 0: 5 wins
                            np.array([[1, 0, 1, 3]] * 65536)])                                            # nothing left: argmax gives 0
    g = np.random.default_rng(0)
    want = G.vote_sorted(np.full(grid, 17, np.uint8), pairs)
    assert (want[0, 0, 0], want[0, 1, 0], want[1, 1, 1], want[1, 0, 1], want[0, 0, 1]) == (4, 255, 5, 0, 17)
    for order in (np.arange(len(pairs)), np.arange(len(pairs))[::-1], g.permutation(len(pairs))):
        p = pairs[order]
        lin = np.ravel_multi_index((p[:, 0], p[:, 1], p[:, 2]), grid)
        got = OG.vote_labels(up(dev, lin.astype(np.int32)), up(dev, p[:, 3].astype(np.uint8)), grid, fill=17)
        same(got.cpu().numpy(), want)
    # rows that name no voxel do not vote, wherever they stand
    lin = np.array([-1, 3, 8, 3, -5, 2 ** 31 - 1, 3], np.int32)
    got = OG.vote_labels(up(dev, lin), up(dev, np.array([9, 6, 9, 6, 9, 9, 2], np.uint8)), grid, fill=1).cpu().numpy().reshape(-1)
    assert got.tolist() == [1, 1, 1, 6, 1, 1, 1, 1]
    form_c = OG.vote_labels(up(dev, np.array([0, 1, 2], np.int32)), up(dev, np.array([0, 17, 5], np.uint8)), grid, fill=0, post_empty=17)
    assert form_c.cpu().numpy().reshape(-1).tolist() == [255, 0, 5, 0, 0, 0, 0, 0]


def test_row_order_does_not_change_a_byte(dev):
    occ = G.rows(5000, 4, seed=22)
    bda = G.bda(0.0, True, False, True)
    want = G.load_occupancy2(occ, G.GRID, G.PC_RANGE, bda, 0)
    g = np.random.default_rng(1)
    for order in (slice(None), slice(None, None, -1), g.permutation(5000), g.permutation(5000)):
        same(form_b(dev, occ[order], bda)[0], want)
    a, b = form_b(dev, occ, bda)[0], form_b(dev, occ, bda)[0]
    same(a, b)


# ------------------------------------------------------------------ form A
def test_form_a_last_row_wins(dev):
    hi = G.GRID
    for C in (4, 7):
        for N in G.ROW_COUNTS:
            occ = G.rows(N, C, hi, seed=23, label_col=3)
            for o in (occ, occ[::-1]):
                for sem in (True, False):
                    got = OG.scatter_labels(rows_dev(dev, o, 3, hi), hi, use_semantic=sem)
                    assert got.dtype == torch.uint8
                    same(got.cpu().numpy(), G.load_occupancy(o, hi, sem).astype(np.uint8))
    occ = np.array([[1, 2, 3, 5], [1, 2, 3, 9], [0, 0, 0, 0], [1, 2, 3, 4], [7, 5, 3, 0], [7, 5, 3, 6], [7, 5, 3, 0]])
    vol = OG.scatter_labels(rows_dev(dev, occ, 3, hi), hi).cpu().numpy()
    assert (vol[1, 2, 3], vol[0, 0, 0], vol[7, 5, 3], vol[2, 2, 2]) == (4, 255, 255, 0)
    vol = OG.scatter_labels(rows_dev(dev, occ[::-1], 3, hi), hi, use_semantic=False).cpu().numpy()
    assert (vol[1, 2, 3], vol[0, 0, 0], vol[7, 5, 3], int(vol.sum())) == (1, 0, 1, 2)


def test_form_a_200_x_200_x_16(dev):
    grid, pr = (200, 200, 16), [-50.0, -50.0, -5.0, 50.0, 50.0, 3.0]
    occ = G.rows(60000, 4, grid, seed=24, label_col=3)
    pts, pose = D.cloud(35000, seed=2, C=5), G.pose_fields(2)
    ld = OG.LoadOccupancy(grid_size=list(grid), pc_range=pr, is_train=True, bda_aug_conf=CONF, device=dev, rng=Draws((True, True, False)))
    out = ld(occ, pts, pose, dtype=torch.float64)
    want = G.load_occupancy(occ, grid)
    assert out["gt_occ"].dtype == torch.float64
    same(out["gt_occ"].cpu().numpy(), want)          # not transformed by bda_rot: the reference's quirk
    same(out["bda_rot"].cpu().numpy(), G.bda(0.0, True, True, False))
    assert G.ulps(out["aabb"].cpu().numpy(), G.aabb(pts, pose)).max() <= 1
    assert ld(occ, pts, pose)["gt_occ"].dtype == torch.uint8


# ------------------------------------------------------------------ form C
@pytest.mark.parametrize("flip", [(False, False, False), (True, False, True), (False, True, False)])
def test_form_c_borders_holes_and_non_finite_points(dev, flip):
    lm = G.LEARNING_MAP_HOLES
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    odd = np.array([[nan, 0, 0], [0, inf, 0], [0, 0, -inf], [nan, nan, nan]], np.float32)
    xyz = np.concatenate([G.border_points(), G.grid_cloud(257, seed=31)[:, :3], odd])
    pts = np.concatenate([xyz, np.zeros((xyz.shape[0], 2), np.float32)], 1)
    seg, pose = G.seg_bytes(pts.shape[0], lm, seed=32), G.pose_fields(3)
    ld = OG.LoadNuscOccupancyAnnotations(is_train=True, grid_size=list(G.GRID), point_cloud_range=G.PC_RANGE, bda_aug_conf=CONF,
                                         unoccupied_id=17, learning_map=lm, device=dev, rng=Draws(flip))
    out = ld(pts, seg, pose, dtype=torch.long)
    bda = G.bda(0.0, *flip)
    vol, pocc = G.nusc_annotations(pts, seg, lm, bda, G.GRID, G.PC_RANGE, 17)
    assert out["gt_occ"].dtype == torch.long
    same(out["gt_occ"].cpu().numpy(), vol)
    got = out["points_occ"].cpu().numpy()
    assert got.dtype == np.float32 and got.shape == pocc.shape
    assert bool(np.all((got == pocc) | (np.isnan(got) & np.isnan(pocc))))          # as numbers: the sign of a zero is not pinned
    same(out["bda_rot"].cpu().numpy(), bda)
    for N in G.ROW_COUNTS[:6]:
        p, s = G.grid_cloud(N, seed=33), G.seg_bytes(N, lm, seed=34)
        vox, labels, _ = OG.points_to_voxels(up(dev, p), "annotation", G.GRID, G.PC_RANGE, bda, up(dev, s), up(dev, ld.table))
        same(OG.vote_labels(vox, labels, G.GRID, fill=0, post_empty=17).cpu().numpy(),
             G.nusc_annotations(p, s, lm, bda, G.GRID, G.PC_RANGE, 17)[0])
    sub = OG.LoadNuscOccupancyAnnotations(is_test_submit=True, grid_size=list(G.GRID), point_cloud_range=G.PC_RANGE, device=dev)
    eight = tuple(torch.zeros(2, 3, device=dev) for _ in range(8))
    res = sub(pts[:200], None, None, img_inputs=eight)
    assert len(res["img_inputs"]) == 9 and torch.equal(res["img_inputs"][6].cpu(), torch.eye(3))
    same(res["points_occ"].cpu().numpy(), G.points_occ(pts[:200], None, None, np.eye(3)).astype(np.float32))


# ------------------------------------------------------------------ the visibility masks
def zbuffer_centres():
    """Centres for two identity cameras at 24 x 40 (u = x / z, v = y / z, d = z; the second shifted by post_tran)."""
    F = np.float32
    rows = []

    def at(u, v, z):
        rows.append((F(u) * F(z), F(v) * F(z), F(z)))
    for (u, v), zs in (((4, 1), (2.0, 4.0)), ((5, 1), (4.0, 2.0)), ((4, 2), (8.0, 2.0, 4.0)), ((5, 2), (2.0, 8.0, 4.0)), ((6, 3), (4.0, 4.0)),
                       ((7, 3), (4.0, 4.03125, 4.0625)),      # unequal depths, equal d*10 truncated: the lowest row
                       ((8, 3), (4.09375, 4.0)),              # 40 against 40
                       ((9, 3), (4.125, 4.0))):               # 41 against 40
        for z in zs:
            at(u, v, z)
    at(10.25, 4.0, 2.0)                                        # two that differ before truncation, one pixel
    at(10.75, 4.5, 2.0)
    at(12, 5, 204.75)                                          # d*10 = 2047.5 -> 2047: wins an empty pixel
    at(13, 5, 204.8)                                           # d*10 rounds to 2048: never wins
    at(14, 5, 3276.8)                                          # d*10 >= 32 768
    at(15, 5, 0.0)                                             # d = 0: 0 / 0
    rows.append((F(3.0), F(3.0), F(0.0)))                      # d = 0: inf
    at(39, 6, 1.0)                                             # u = W-1
    rows.append((np.nextafter(F(39), F(np.inf)), F(6.0), F(1.0)))          # one step past W-1: still column 39, a later equal
    rows.append((F(40.0), F(6.0), F(1.0)))                     # u = W: out
    at(2, 23, 1.0)                                             # v = H-1
    rows.append((F(2.0), F(24.0), F(1.0)))                     # v = H: out
    rows.append((F(-0.0), F(7.0), F(1.0)))                     # u = -0.0: column 0
    rows.append((F(-0.5), F(7.0), F(1.0)))                     # truncates to column 0, but u < 0: out
    rows.append((F(2.0), F(2.0), F(-1.0)))                     # behind
    return np.array(rows, F)


def test_zbuffer_hand_cases_in_both_memory_orders(dev):
    H, W = 24, 40
    mats = D.identity_rig(2)
    mats[4][1, 0], mats[4][1, 1] = 1.5, 0.25
    np_mats = [m.numpy() for m in mats]
    table = DM.camera_table(*mats).to(dev)
    cen = zbuffer_centres()
    g = np.random.default_rng(4)
    for order in (np.arange(len(cen)), np.arange(len(cen))[::-1], g.permutation(len(cen))):
        c = cen[order]
        want = G.visible_rows(c.astype(np.float64), np_mats, H, W)
        assert 10 < want.sum() < len(cen)
        got = OG.visible_rows(up(dev, c), table, (H, W))
        same(got.cpu().numpy().astype(bool), want)
    first = OG.visible_rows(up(dev, cen), up(dev, DM.camera_table(*D.identity_rig(1)).numpy()), (H, W)).cpu().numpy()
    assert first[:5].tolist() == [1, 0, 0, 1, 0] and first[12:15].tolist() == [1, 0, 0]          # near wins; the lowest row among equal d*10


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 257, 5000])
def test_camera_mask_on_the_synthetic_rig(dev, N):
    H, W = G.SMALL['input_size']
    mats = G.small_rig()
    np_mats = [m.numpy() for m in mats]
    occ = G.distinct_rows(N, G.GRID, seed=41)
    bda = G.bda(0.0, False, True, True)
    _, vox, centres = form_b(dev, occ, bda)
    masks = OG.visible_masks(centres, vox, G.GRID, DM.camera_table(*mats).to(dev), (H, W))
    want = G.img_visible_mask(occ, G.GRID, G.PC_RANGE, bda, np_mats, H, W) if N else np.zeros(G.GRID, np.uint8)
    same(masks["img_visible_mask"].cpu().numpy(), want)
    same(masks["visible_mask"].cpu().numpy(), want)
    if N == 257:          # every voxel once and 65 repeats: a lone visible row carries its voxel (at 5000 a voxel's 26 rows outvote the one winner)
        assert want.sum() > 5


def test_lidar_mask_on_and_inside_the_borders(dev):
    pts = np.concatenate([G.border_points(), G.grid_cloud(5000, seed=42)[:, :3], np.array([[np.nan, 0, 0], [0, np.inf, 0]], np.float32)])
    want = G.lidar_visible_mask(pts, G.GRID, G.PC_RANGE)
    vox, labels, _ = OG.points_to_voxels(up(dev, pts), "lidar_mask", G.GRID, G.PC_RANGE)
    same(OG.vote_labels(vox, labels, G.GRID, fill=0).cpu().numpy(), want)
    assert want[0, 0, 0] == 1 and 0 < want.sum()
    many = np.repeat(np.array([[0.5, 0.5, 0.5]], np.float32), 65536, 0)          # the reference's counter wraps here too
    vox, labels, _ = OG.points_to_voxels(up(dev, many), "lidar_mask", G.GRID, G.PC_RANGE)
    same(OG.vote_labels(vox, labels, G.GRID, fill=0).cpu().numpy(), G.lidar_visible_mask(many, G.GRID, G.PC_RANGE, G.vote_sorted))


# ------------------------------------------------------------------ aabb
@pytest.mark.parametrize("P", [1, 64, 35000])
def test_aabb_within_one_step_of_numpy(dev, P):
    unequal = 0
    for seed in range(3):
        pts, pose = D.cloud(P, seed=50 + seed, C=5), G.pose_fields(10 + seed)
        got = OG.cloud_aabb(up(dev, pts), pose).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (2, 3)
        same(got.view(np.uint32), G.aabb_ordered(pts, pose).view(np.uint32))          # the same operations in the same order
        off = G.ulps(got, G.aabb(pts, pose))
        assert off.max() <= 1, off
        unequal += int((off != 0).sum())
    print("aabb P = %d: %d of 18 fp32 values differ from numpy's matmul" % (P, unequal))
    assert unequal == 0, "%d of 18 fp32 values are one step from numpy's matmul: its float64 sums are no longer left to right" % unequal


def test_aabb_of_a_cloud_with_a_nan_is_numpy_s(dev):
    """numpy's min / max give NaN where any value is NaN; a NaN coordinate reaches every axis its rotation row touches."""
    pts, pose = D.cloud(300, seed=53, C=5), G.pose_fields(13)
    pts[17, 1] = np.nan
    with np.errstate(invalid="ignore"):
        want = G.aabb(pts, pose)
    got = OG.cloud_aabb(up(dev, pts), pose).cpu().numpy()
    assert np.isnan(want).all() and np.isnan(got).all()          # 0 * NaN is NaN in the matrix product: every axis
    pts[17, 1] = np.inf                                          # an infinity is a value: inf - inf on some axis, +-inf on others
    with np.errstate(invalid="ignore"):
        want = G.aabb_ordered(pts, pose)
    got = OG.cloud_aabb(up(dev, pts), pose).cpu().numpy()
    assert np.array_equal(got, want, equal_nan=True)


# ------------------------------------------------------------------ the golden file
def test_golden_sample_through_the_loaders(dev, gold):
    H, W = G.SMALL['input_size']
    flip = tuple(bool(f) for f in gold["flip"])
    mats = [torch.from_numpy(gold[k]) for k in ("rots", "trans", "intrins", "post_rots", "post_trans")]
    imgs = torch.zeros(2, 3, H, W)
    twelve = tuple(t.to(dev) for t in (imgs, *mats, torch.zeros(2, H, W), torch.zeros(2, 4, 4), imgs, torch.zeros(2, 3, 3), torch.zeros(2, 4, 4)))
    twelve = twelve + (imgs.shape[-2:],)
    pose = G.golden_pose(gold)
    ld = OG.LoadOccupancy2(grid_size=list(G.GRID), pc_range=G.PC_RANGE, cal_visible=True, is_train=True, bda_aug_conf=CONF,
                           learning_map=G.LEARNING_MAP, device=dev, rng=Draws(flip))
    out = ld(gold["occ"], gold["cloud"], gold["seg"], pose, img_inputs=twelve, lidar_points=gold["cloud"])
    same(out["gt_occ"].cpu().numpy(), gold["gt_b"])
    same(out["img_visible_mask"].cpu().numpy(), gold["img_mask"])
    same(out["lidar_visible_mask"].cpu().numpy(), gold["lidar_mask"])
    same(out["visible_mask"].cpu().numpy(), gold["img_mask"] | gold["lidar_mask"])
    same(out["points_occ"].cpu().numpy(), gold["points_occ"])
    same(out["bda_rot"].cpu().numpy(), gold["bda"])
    assert G.ulps(out["aabb"].cpu().numpy(), gold["aabb"]).max() <= 1
    assert len(out["img_inputs"]) == 14 and out["img_inputs"][6] is out["bda_rot"] and out["img_inputs"][10] is out["aabb"]
    assert len(out["gt_depths"]) == 7 and out["gt_depths"][5] is out["bda_rot"]
    _, vox, centres = form_b(dev, gold["occ"].astype(np.int64), gold["bda"])
    flags = OG.visible_rows(centres, DM.camera_table(*mats).to(dev), (H, W))
    same(flags.cpu().numpy().astype(bool), gold["visible"])
    same(OG.scatter_labels(rows_dev(dev, gold["occ_a"], 3, G.GRID), G.GRID).cpu().numpy(), gold["gt_a"])
    c = OG.LoadNuscOccupancyAnnotations(is_train=True, grid_size=list(G.GRID), point_cloud_range=G.PC_RANGE, bda_aug_conf=CONF,
                                        learning_map=G.LEARNING_MAP, device=dev, rng=Draws(flip))(gold["cloud"], gold["seg"], pose)
    same(c["gt_occ"].cpu().numpy(), gold["gt_c"])
    assert c["gt_occ"].dtype == torch.uint8


# ------------------------------------------------------------------ the full size
def test_openoccupancy_size_with_masks(dev):
    """512 x 512 x 40, 300 000 rows, six cameras at 896 x 1600, cal_visible: against the vectorised restatement."""
    H, W = R.R101['input_size']
    mats = D.rig(R.R101)
    np_mats = [m.numpy() for m in mats]
    occ = np.concatenate([G.distinct_rows(240000, BIG_GRID, seed=61), G.rows(60000, 4, (40, 512, 512), seed=62)])
    occ = occ[np.random.default_rng(63).permutation(len(occ))]
    pts, pose = D.cloud(34720, seed=64, C=5), G.pose_fields(20)
    seg = G.seg_bytes(len(pts), G.LEARNING_MAP, seed=65)
    flip = (True, False, True)
    bda = G.bda(0.0, *flip)
    imgs = torch.zeros(6, 3, H, W, device=dev)
    twelve = (imgs,) + tuple(m.to(dev) for m in mats) + (None, None, None, None, None, imgs.shape[-2:])
    ld = OG.LoadOccupancy2(grid_size=list(BIG_GRID), pc_range=BIG_RANGE, cal_visible=True, is_train=True, bda_aug_conf=CONF,
                           learning_map=G.LEARNING_MAP, device=dev, rng=Draws(flip))
    out = ld(occ, pts, seg, pose, img_inputs=twelve, lidar_points=pts)
    same(out["gt_occ"].cpu().numpy(), G.load_occupancy2(occ, BIG_GRID, BIG_RANGE, bda, 0, G.vote_sorted))
    want_img = G.img_visible_mask(occ, BIG_GRID, BIG_RANGE, bda, np_mats, H, W, G.vote_sorted, G.zbuffer_sorted)
    want_pts = G.lidar_visible_mask(pts, BIG_GRID, BIG_RANGE, G.vote_sorted)
    assert want_img.sum() > 1000 and want_pts.sum() > 1000
    same(out["img_visible_mask"].cpu().numpy(), want_img)
    same(out["lidar_visible_mask"].cpu().numpy(), want_pts)
    same(out["visible_mask"].cpu().numpy(), want_img | want_pts)
    assert ld._stage.last_bytes < 4 << 20          # rows as 8-byte records, the cloud, the tables: under the 10.5 MB volume
    assert OG.release_scratch() >= 6 * H * W * 8 and OG.release_scratch() == 0          # the canvas and the sort storage go; nothing is left
    again = ld(occ[:1000], pts, seg, pose, img_inputs=twelve, lidar_points=pts)            # and come back on the next call
    same(again["gt_occ"].cpu().numpy(), G.load_occupancy2(occ[:1000], BIG_GRID, BIG_RANGE, bda, 0, G.vote_sorted))


# ------------------------------------------------------------------ end to end
def test_forward_train_reads_the_device_ground_truth(dev):
    """with_bda(img_inputs, bda_rot, aabb) and the device gt_occ through forward_train(device_occ_losses=True) give the loss values
    of the same labels built on the host and uploaded.  The labels are asserted equal byte for byte; the losses are then the same
    computation twice, held to the 2e-5 max(1, |v|) that tests/test_gpu_occ_losses.py allows two runs of one step."""
    import test_gpu_boundary as TB
    model = TB._full_model(dev)
    model.train()
    model.device_occ_losses = model.pts_bbox_head.device_losses = True
    img_inputs, points, gt = TB._sample(dev)
    grid = (200, 200, 16)
    occ = G.rows(60000, 4, grid, seed=71, labels=17, label_col=3)
    pose = G.pose_fields(30)
    host_gt = G.load_occupancy(occ, grid).astype(np.uint8)
    ld = OG.LoadOccupancy(grid_size=list(grid), pc_range=[-50, -50, -5, 50, 50, 3], device=dev)
    imgs, rots, trans, intrins, post_rots, post_trans, _, depth, size = img_inputs
    twelve = (imgs[0], rots[0], trans[0], intrins[0], post_rots[0], post_trans[0], depth[0], None, None, None, None, size)
    out = ld(occ, points[0], pose, img_inputs=twelve)
    same(out["gt_occ"].cpu().numpy(), host_gt)
    fourteen = II.with_bda(twelve, out["bda_rot"], out["aabb"])
    assert len(fourteen) == 14 and torch.equal(fourteen[6][0].cpu(), torch.eye(3)) and tuple(fourteen[10].shape) == (1, 2, 3)
    runs = []
    for inputs, labels in ((fourteen, out["gt_occ"][None]), (img_inputs, torch.from_numpy(host_gt)[None].to(dev))):
        losses = model(return_loss=True, points=points, img_metas=None, img_inputs=inputs, gt_occ=labels,
                       generator=torch.Generator(device=dev).manual_seed(0))
        runs.append({k: float(v.detach()) for k, v in losses.items()})
    assert set(runs[0]) == set(runs[1]) and len(runs[0]) >= 4
    for k, v in runs[1].items():
        assert np.isfinite(v) and abs(runs[0][k] - v) <= 2e-5 * max(1.0, abs(v)), (k, runs[0][k], v)
