"""The occupancy ground truth on the host (no GPU): the numpy restatements the GPU tests are judged against (tests/occ_gt_refs.py)
are held here against each other (the literal sequential loops against their sorted twins), against LIVE torch on the CPU (the
projection and the fp32 bda product) and against the golden file; plus the host halves of co_occ_amd/occ_gt.py -- the draws, the
matrix, the row packing, the refusals -- and the C entry points' argument validation."""
import ctypes

import numpy as np
import pytest
import torch

import depth_map_refs as D
import occ_gt_refs as G
from conftest import GOLDEN
from co_occ_amd import _lib, occ_gt as OG
from co_occ_amd._lib import CooccError

BIG_GRID, BIG_RANGE = (512, 512, 40), [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN + "/occ_gt.npz")


# ------------------------------------------------------------------ the restatements against each other
@pytest.mark.parametrize("N", [1, 65, 5000])
@pytest.mark.parametrize("flip", [(False, False, False), (True, False, True), (True, True, True)])
def test_sequential_vote_equals_the_sorted_vote(N, flip):
    occ = G.rows(N, 7, seed=11)
    a = G.load_occupancy2(occ, G.GRID, G.PC_RANGE, G.bda(0.0, *flip), 3, vote=G.vote_loop)
    b = G.load_occupancy2(occ, G.GRID, G.PC_RANGE, G.bda(0.0, *flip), 3, vote=G.vote_sorted)
    assert a.dtype == b.dtype == np.uint8 and np.array_equal(a, b)
    if N == 5000:
        assert len(np.unique(a)) > 5 and (a == 255).any()


def test_votes_wrap_at_65536_and_ties_take_the_lowest_label():
    grid = (2, 2, 2)
    tie = np.array([[0, 0, 0, 9], [0, 0, 0, 4], [0, 0, 0, 9], [0, 0, 0, 4]])
    wrap = np.array([[1, 1, 1, 3]] * 65536 + [[1, 1, 1, 5]] * 2)
    alone = np.array([[1, 0, 1, 3]] * 65536)
    big = np.array([[0, 1, 0, 255]] * 3 + [[0, 1, 0, 7]] * 2)
    pairs = np.concatenate([tie, wrap, alone, big])
    pairs = pairs[np.lexsort((pairs[:, 0], pairs[:, 1], pairs[:, 2]))]
    for vote in (G.vote_loop, G.vote_sorted):
        vol = vote(np.full(grid, 17, np.uint8), pairs)
        assert (vol[0, 0, 0], vol[1, 1, 1], vol[1, 0, 1], vol[0, 1, 0], vol[0, 0, 1]) == (4, 5, 0, 255, 17), vote.__name__


def test_zbuffer_loop_equals_the_sorted_zbuffer():
    g = np.random.default_rng(5)
    pix = np.stack([g.integers(0, 7, 900), g.integers(0, 5, 900), g.integers(0, 2300, 900)], 1).astype(np.int16)
    a, b = G.zbuffer_loop(pix, 5, 7), G.zbuffer_sorted(pix, 5, 7)
    assert np.array_equal(a, b) and 0 < a.sum() <= 35
    same = np.array([[1, 1, 30], [1, 1, 30], [1, 1, 2048], [2, 2, 2048], [3, 3, 2047]], np.int16)
    for z in (G.zbuffer_loop, G.zbuffer_sorted):
        assert z(same, 5, 7).tolist() == [True, False, False, False, True]          # the lowest row among equals; 2048 never wins


def test_rotation_fragments_the_reference_vote():
    """Why rotate_bda != 0 is refused: the reference sorts form B's rows by FLOAT coordinates, so with a rotation the rows of one
    voxel are not adjacent and its loop writes the voxel once per fragment -- the last fragment's winner stays.  With flips the
    coordinates of a voxel's rows are equal floats, the rows stay adjacent, and the loop is the order-independent vote."""
    g = np.random.default_rng(8)
    occ = np.stack([g.integers(15, 25, 20000), g.integers(200, 300, 20000), g.integers(200, 300, 20000), g.integers(1, 17, 20000)], 1)
    diff = {}
    for name, m in (("flip", G.bda(0.0, True, True, False)), ("rotate", G.bda(10.0))):
        _, coords, label = G.occupancy2_rows(occ, BIG_GRID, BIG_RANGE, m)
        pairs = G.sort_pairs(coords, label)
        loop = G.vote_loop(np.zeros(BIG_GRID, np.uint8), pairs)
        diff[name] = int((loop != G.vote_sorted(np.zeros(BIG_GRID, np.uint8), pairs)).sum())
    print("voxels where the sequential loop differs from the vote:", diff)
    assert diff["flip"] == 0 and diff["rotate"] > 0


# ------------------------------------------------------------------ against live torch and the golden file
def test_projection_and_bda_product_restate_live_torch(gold):
    mats = G.small_rig()
    occ = G.distinct_rows(G.GOLDEN_ROWS, G.GRID, seed=3)
    assert np.array_equal(occ, gold["occ"])
    centres, _, _ = G.occupancy2_rows(occ, G.GRID, G.PC_RANGE, gold["bda"])
    tu, tv, td = (t.numpy() for t in D.torch_projection(torch.Tensor(centres), *mats))
    nu, nv, nd = G.projected(centres, [m.numpy() for m in mats])
    for t, n, k in ((tu, nu, 0), (tv, nv, 1), (td, nd, 2)):
        assert np.array_equal(t.view(np.uint32), n.view(np.uint32)) and np.array_equal(t, gold["uvd"][..., k])
    g = np.random.default_rng(3)
    m = torch.from_numpy(g.standard_normal((3, 3)).astype(np.float32))
    p = g.standard_normal((4000, 3)) * 30
    want = (m @ torch.from_numpy(p).unsqueeze(-1).float()).squeeze(-1).numpy()
    assert np.array_equal(G.rotate32(m.numpy(), p.astype(np.float32)).view(np.uint32), want.view(np.uint32))


def test_restatements_give_the_golden_volumes(gold):
    H, W = G.SMALL['input_size']
    mats = [gold[k] for k in ("rots", "trans", "intrins", "post_rots", "post_trans")]
    occ, bda = gold["occ"].astype(np.int64), gold["bda"]
    assert np.array_equal(bda, np.diag([-1.0, 1.0, -1.0]).astype(np.float32))
    for vote, zb in ((G.vote_loop, G.zbuffer_loop), (G.vote_sorted, G.zbuffer_sorted)):
        assert np.array_equal(G.load_occupancy2(occ, G.GRID, G.PC_RANGE, bda, 0, vote), gold["gt_b"])
        assert np.array_equal(G.img_visible_mask(occ, G.GRID, G.PC_RANGE, bda, mats, H, W, vote, zb), gold["img_mask"])
        assert np.array_equal(G.lidar_visible_mask(gold["cloud"], G.GRID, G.PC_RANGE, vote), gold["lidar_mask"])
        vol, pocc = G.nusc_annotations(gold["cloud"], gold["seg"], G.LEARNING_MAP, bda, G.GRID, G.PC_RANGE, 17, vote)
        assert np.array_equal(vol, gold["gt_c"]) and np.array_equal(pocc, gold["points_occ"])
    assert np.array_equal(G.load_occupancy(gold["occ_a"], G.GRID).astype(np.uint8), gold["gt_a"])
    pose = G.golden_pose(gold)
    assert np.array_equal(G.aabb(gold["cloud"], pose), gold["aabb"])
    off = G.ulps(G.aabb_ordered(gold["cloud"], pose), gold["aabb"])
    print("aabb: left-to-right float64 against numpy's matmul, fp32 steps apart:", off.reshape(-1).tolist())
    assert off.max() <= 1
    assert int((off != 0).sum()) == 0, "numpy's float64 matmul no longer sums left to right on this host: %s" % off.reshape(-1).tolist()


# ------------------------------------------------------------------ the host halves of the module
def test_bda_matrix_is_the_flip_diagonal():
    for flip in G.FLIPS:
        m = OG.bda_matrix(0.0, 1.3, *flip)
        assert m.dtype == torch.float32 and tuple(m.shape) == (3, 3)
        assert np.array_equal(m.numpy(), np.diag([-1.0 if f else 1.0 for f in flip]).astype(np.float32))
        assert np.array_equal(m.numpy(), G.bda(0.0, *flip))
    assert np.array_equal(OG.bda_matrix(10.0, 1.0, True, False, False).numpy(), G.bda(10.0, True, False, False))


def test_the_five_draws_come_in_the_reference_order():
    class Recorder:
        def __init__(self):
            self.calls, self.values = [], iter([0.0, 1.02, 0.4, 0.6, 0.1])

        def uniform(self, *a):
            self.calls.append(a)
            return next(self.values)

    rng = Recorder()
    conf = dict(rot_lim=(0, 0), scale_lim=(0.95, 1.05), flip_dx_ratio=0.5, flip_dy_ratio=0.5, flip_dz_ratio=0.5)
    assert OG.sample_3d_augmentation(conf, rng) == (0.0, 1.02, True, False, True)
    assert rng.calls == [(0, 0), (0.95, 1.05), (), (), ()]
    conf.pop("flip_dz_ratio")
    assert not OG.sample_3d_augmentation(conf, Recorder())[4]          # no flip_dz_ratio: 0.0, still drawn
    state = np.random.RandomState(4)
    want = (state.uniform(0, 0), state.uniform(0.95, 1.05), state.uniform() < 0.5, state.uniform() < 0.5, state.uniform() < 0.0)
    assert OG.sample_3d_augmentation(conf, np.random.RandomState(4)) == want


def test_pack_rows_reads_the_reference_columns():
    occ = G.rows(50, 7, seed=2)
    occ[:, 3] = np.arange(50) % 5
    b, a = OG.pack_rows(occ, -1), OG.pack_rows(occ, 3, (4, 6, 8))
    assert a.dtype == b.dtype == np.uint16 and a.shape == b.shape == (50, 4)
    assert np.array_equal(b[:, :3], occ[:, :3]) and np.array_equal(b[:, 3], occ[:, 6]) and np.array_equal(a[:, 3], occ[:, 3])
    assert np.array_equal(OG.pack_rows(occ.astype(np.float32) + np.float32(0.25), 3)[:, :3], occ[:, :3])          # truncated
    assert OG.pack_rows(np.zeros((0, 4), np.uint8)).shape == (0, 4)
    # form A rounds the rows to float32 before it truncates them (occ.astype(np.float32)): a float64 index of 4 - 1e-12 is 4 there
    near = np.array([[4 - 1e-12, 2 - 1e-12, 3 + 1e-12, 5 - 1e-12], [1.75, 0.5, 2.25, 7.0]])
    assert OG.pack_rows(near, 3, (8, 6, 4), to_float32=True).tolist() == [[4, 2, 3, 5], [1, 0, 2, 7]]
    assert OG.pack_rows(near, 3, (8, 6, 4)).tolist() == [[3, 1, 3, 4], [1, 0, 2, 7]]
    assert G.load_occupancy(near, G.GRID)[4, 2, 3] == 5 and G.load_occupancy(near, G.GRID)[1, 0, 2] == 7
    with pytest.raises(ValueError, match="outside"):
        OG.pack_rows(np.array([[8 - 1e-12, 0, 0, 1]]), 3, (8, 6, 4), to_float32=True)          # 8.0 after the rounding: outside


def test_refusals():
    occ = G.rows(20, 4, seed=1)
    for bad in (dict(col=3, val=256), dict(col=3, val=-1)):
        o = occ.copy()
        o[3, bad["col"]] = bad["val"]
        with pytest.raises(ValueError, match="labels"):
            OG.pack_rows(o, 3)
    o = occ.copy()
    o[5, 1] = 6
    with pytest.raises(ValueError, match="outside"):
        OG.pack_rows(o, 3, (4, 6, 8))
    o = occ.copy()
    o[7, 0] = -1
    with pytest.raises(ValueError, match="outside"):
        OG.pack_rows(o, -1)
    with pytest.raises(ValueError):
        OG.pack_rows(occ[:, :3])
    for cls in (OG.LoadOccupancy, OG.LoadOccupancy2):
        with pytest.raises(NotImplementedError, match="use_vel"):
            cls(use_vel=True, learning_map=G.LEARNING_MAP)
    with pytest.raises(ValueError, match="2\\^24"):
        OG.LoadOccupancy(grid_size=[512, 512, 80])
    conf = dict(rot_lim=(10, 10), scale_lim=(1, 1), flip_dx_ratio=0.5, flip_dy_ratio=0.5)
    for ld in (OG.LoadOccupancy(is_train=True, bda_aug_conf=conf), OG.LoadOccupancy2(is_train=True, bda_aug_conf=conf, learning_map=G.LEARNING_MAP),
               OG.LoadNuscOccupancyAnnotations(is_train=True, bda_aug_conf=conf, grid_size=G.GRID, point_cloud_range=G.PC_RANGE,
                                               learning_map=G.LEARNING_MAP)):
        with pytest.raises(NotImplementedError, match="rotate_bda"):
            ld._bda()
    ld = OG.LoadNuscOccupancyAnnotations(grid_size=G.GRID, point_cloud_range=G.PC_RANGE, learning_map=G.LEARNING_MAP_HOLES)
    with pytest.raises(ValueError, match="learning_map"):
        ld._seg_bytes(np.array([1, 2, 10], np.uint8), 3)
    assert ld._seg_bytes(np.array([1, 2, 200], np.uint8), 3).tolist() == [1, 2, 200]
    with pytest.raises(ValueError):
        ld._seg_bytes(np.array([1, 2], np.int32), 2)
    with pytest.raises(ValueError, match="0 .. 255"):
        OG.LoadNuscOccupancyAnnotations(grid_size=G.GRID, point_cloud_range=G.PC_RANGE, learning_map={1: 300})
    # CPU tensors handed to a kernel
    rows = torch.zeros((3, 4), dtype=torch.int16)
    with pytest.raises(CooccError):
        OG.scatter_labels(rows, G.GRID)
    with pytest.raises(CooccError):
        OG.vote_labels(torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.uint8), G.GRID)
    with pytest.raises(CooccError):
        OG.visible_rows(torch.zeros((3, 3)), torch.zeros((1, 28)), (4, 4))
    with pytest.raises(CooccError):
        OG.cloud_aabb(torch.zeros((3, 3)), G.pose_fields())
    with pytest.raises(CooccError):
        OG.points_to_voxels(torch.zeros((3, 3)), "annotation", G.GRID, G.PC_RANGE)
    with pytest.raises(CooccError):
        OG.rows_to_voxels(rows, G.GRID, G.PC_RANGE)
    with pytest.raises(ValueError):
        OG.scatter_labels(np.zeros((3, 4), np.int16), G.GRID)


def test_entry_points_validate_before_launching():
    lib = _lib.load()
    one = ctypes.c_void_p(256)          # validation never dereferences device pointers
    grid = (ctypes.c_double * 9)(-4, -3, -5, 4, 3, 3, 1, 1, 2)
    err = lambda: lib.coocc_last_error()
    assert lib.coocc_occ_scatter_labels(one, 5, 512, 512, 80, 1, one, one, None) == -1 and b"occ_scatter_labels" in err()
    assert lib.coocc_occ_scatter_labels(None, 5, 8, 6, 4, 1, one, one, None) == -1 and b"null" in err()
    assert lib.coocc_occ_scatter_labels(one, 1 << 24, 8, 6, 4, 1, one, one, None) == -1 and b"rows" in err()
    assert lib.coocc_occ_rows_to_voxels(one, 5, None, None, 8, 6, 4, one, one, None, None) == -1 and b"grid" in err()
    assert lib.coocc_occ_rows_to_voxels(one, 5, grid, None, 8, 0, 4, one, one, None, None) == -1
    assert lib.coocc_occ_points_to_voxels(one, 5, 2, None, None, None, grid, 8, 6, 4, 1, one, one, None, None) == -1 and b"floats" in err()
    assert lib.coocc_occ_points_to_voxels(one, 5, 3, one, None, None, grid, 8, 6, 4, 1, one, one, None, None) == -1 and b"table" in err()
    assert lib.coocc_occ_points_to_voxels(one, 5, 3, None, None, None, grid, 8, 6, 4, 3, one, one, None, None) == -1 and b"mode" in err()
    assert lib.coocc_occ_vote_labels(one, one, 5, (1 << 24) + 1, 0, -1, one, one, 1 << 20, None) == -1 and b"2^24" in err()
    assert lib.coocc_occ_vote_labels(one, one, 5, 192, 256, -1, one, one, 1 << 20, None) == -1 and b"fill" in err()
    assert lib.coocc_occ_visible_rows(one, 5, one, 2, 40000, 40, one, one, None) == -1 and b"int16" in err()
    assert lib.coocc_occ_visible_rows(one, 5, one, 0, 24, 40, one, one, None) == -1 and b"cameras" in err()
    assert lib.coocc_occ_cloud_aabb(one, 0, 5, grid, one, one, None) == -1 and b"empty" in err()
    assert lib.coocc_occ_cloud_aabb(one, 5, 5, None, one, one, None) == -1 and b"null" in err()
    assert lib.coocc_occ_vote_ws(0) == 256
