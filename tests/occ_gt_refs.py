"""References of the occupancy ground-truth tests (test_occ_gt_host.py, test_gpu_occ_gt.py), written apart from co_occ_amd/occ_gt.py:
numpy restatements of what the reference's three occupancy loaders compute, step by step in their order --
  - the majority vote as the literal sequential loop over sorted rows with a uint16 counter per label (``vote_loop``) and a
    vectorised twin for large cases (``vote_sorted``: one sort, counts modulo 65 536, the lowest label among the maxima);
  - form A (indexed assignment, the last row wins), form B (float64 centre -> fp32 -> bda -> float64 index, clip, truncate),
    form C (clip, floor) and the camera / LiDAR visibility masks (the sequential z-buffer and a sorted twin);
  - aabb in numpy float64 matmuls, as the reference computes it;
  - the grids, rows, clouds and cases both test files share.
numba and pyquaternion are not needed; nothing here imports the package."""
import numpy as np
import torch

import depth_map_refs as D
import image_input_refs as R

F = np.float32
GRID = (8, 6, 4)
PC_RANGE = [-4.0, -3.0, -5.0, 4.0, 3.0, 3.0]          # non-cubic cells, z not symmetric: flip_dz shifts and clips, it does not mirror
FLIPS = [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)]
ROW_COUNTS = [0, 1, 63, 64, 65, 257, 5000]
LEARNING_MAP = {k: (k * 7) % 17 for k in range(0, 32)}
LEARNING_MAP_HOLES = {k: (k * 5) % 17 for k in list(range(0, 9)) + list(range(12, 20)) + [31, 200]}


def voxel_size(grid, pc_range):
    r = np.array(pc_range)
    return (r[3:] - r[:3]) / np.array(grid)


# ------------------------------------------------------------------ the vote
def vote_loop(volume, pairs):
    """The reference's nb_process_label: ``pairs`` int64 [M, 4] (i, j, k, label) SORTED so that a voxel's rows are adjacent; a 256-bin
    uint16 counter per voxel, np.argmax when the voxel changes.  Writes into ``volume`` and returns it."""
    if pairs.shape[0] == 0:
        return volume
    counter = np.zeros(256, np.uint16)
    counter[pairs[0, 3]] = 1
    cur = pairs[0, :3]
    with np.errstate(over="ignore"):
        for i in range(1, pairs.shape[0]):
            ind = pairs[i, :3]
            if not np.all(np.equal(ind, cur)):
                volume[cur[0], cur[1], cur[2]] = np.argmax(counter)
                counter = np.zeros(256, np.uint16)
                cur = ind
            counter[pairs[i, 3]] = np.uint16((int(counter[pairs[i, 3]]) + 1) & 0xFFFF)
    volume[cur[0], cur[1], cur[2]] = np.argmax(counter)
    return volume


def sort_pairs(coords, labels):
    """[coords | labels] sorted by np.lexsort((c0, c1, c2)) and truncated to int64, as the loaders do before the loop"""
    pairs = np.concatenate([coords, np.asarray(labels).reshape(-1, 1)], axis=-1)
    pairs = pairs[np.lexsort((coords[:, 0], coords[:, 1], coords[:, 2])), :]
    return pairs.astype(np.int64)


def vote_sorted(volume, pairs):
    """The same volume from int64 pairs in ANY order: counts per (voxel, label) modulo 65 536, the lowest label among the maxima."""
    if pairs.shape[0] == 0:
        return volume
    lin = np.ravel_multi_index((pairs[:, 0], pairs[:, 1], pairs[:, 2]), volume.shape)
    keys, counts = np.unique(lin * 256 + pairs[:, 3], return_counts=True)
    vox, lab, counts = keys >> 8, keys & 255, counts & 0xFFFF
    starts = np.flatnonzero(np.r_[True, vox[1:] != vox[:-1]])
    best = np.maximum.reduceat(counts * 256 + (255 - lab), starts)
    win = np.where(best >> 8 == 0, 0, 255 - (best & 255))          # every count wrapped to 0: argmax of a zero counter
    volume.reshape(-1)[vox[starts]] = win
    return volume


# ------------------------------------------------------------------ the augmentation matrix
def bda(rotate=0.0, flip_dx=False, flip_dy=False, flip_dz=False):
    """voxel_transform(None, ...)'s fp32 matrix with torch, as the reference makes it"""
    a = torch.tensor(rotate / 180 * np.pi)
    s, c = torch.sin(a), torch.cos(a)
    rot = torch.Tensor([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    flip = torch.eye(4)
    if flip_dx:
        flip = flip @ torch.Tensor([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    if flip_dy:
        flip = flip @ torch.Tensor([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    if flip_dz:
        flip = flip @ torch.Tensor([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]])
    return (flip @ rot)[:3, :3].numpy()


def rotate32(m, p):
    """m @ p per row in numpy float32: products rounded, sums left to right (ATen's CPU bmm of a 3 x 3 with a 3 x 1)"""
    m, p = np.asarray(m, F), np.asarray(p, F)
    return np.stack([(m[i, 0] * p[:, 0] + m[i, 1] * p[:, 1]) + m[i, 2] * p[:, 2] for i in range(3)], 1)


# ------------------------------------------------------------------ form A
def load_occupancy(occ, grid, use_semantic=True):
    occ = np.asarray(occ).astype(F)
    if use_semantic:
        occ[..., 3][occ[..., 3] == 0] = 255
    else:
        occ = occ[occ[..., 3] > 0]
        occ[..., 3] = 1
    voxel = np.zeros(grid)
    voxel[occ[:, 0].astype(int), occ[:, 1].astype(int), occ[:, 2].astype(int)] = occ[:, 3]
    return voxel


# ------------------------------------------------------------------ form B
def occupancy2_rows(occ, grid, pc_range, bda_rot):
    """(centres float64 [N,3] untransformed, voxel coordinates float64 [N,3] transformed and clipped, labels [N,1])"""
    r, vs = np.array(pc_range), voxel_size(grid, pc_range)
    pcd = np.array(occ)
    label = pcd[..., -1:]
    label[label == 0] = 255
    centres = (pcd[..., [2, 1, 0]] + 0.5) * vs[None, :] + r[:3][None, :]
    moved = rotate32(bda_rot, centres.astype(F))
    coords = (moved - r[:3][None, :]) / vs[None, :]
    coords = np.clip(coords, np.array([0, 0, 0]), np.array(grid) - 1)
    return centres, coords, label


def load_occupancy2(occ, grid, pc_range, bda_rot, unoccupied=0, vote=vote_loop):
    _, coords, label = occupancy2_rows(occ, grid, pc_range, bda_rot)
    return vote(np.ones(grid, dtype=np.uint8) * np.uint8(unoccupied), sort_pairs(coords, label))


def zbuffer_loop(pix, H, W):
    """nb_process_img_points: pix int16 [M, 3] (u, v, d10) in row order -> bool [M]"""
    canvas = np.ones((H, W), dtype=np.uint16) * 2048
    owner = -np.ones((H, W), dtype=np.int64)
    ok = np.zeros(pix.shape[0], dtype=bool)
    for i in range(pix.shape[0]):
        u, v, d = int(pix[i, 0]), int(pix[i, 1]), int(pix[i, 2])
        if d < canvas[v, u]:
            if owner[v, u] != -1:
                ok[owner[v, u]] = False
            owner[v, u] = i
            canvas[v, u] = d
            ok[i] = True
    return ok


def zbuffer_sorted(pix, H, W):
    """the same flags by one sort: per pixel the first row with the smallest d10 below 2048"""
    ok = np.zeros(pix.shape[0], dtype=bool)
    rows = np.flatnonzero(pix[:, 2] < 2048)
    if rows.size == 0:
        return ok
    p = pix[rows].astype(np.int64)
    cell = p[:, 1] * W + p[:, 0]
    order = np.lexsort((rows, p[:, 2], cell))
    first = np.r_[True, cell[order][1:] != cell[order][:-1]]
    ok[rows[order[first]]] = True
    return ok


def projected(centres, mats):
    """(u, v, d) float32 [N, n_cam] of project_points on float64 centres: torch.Tensor(centres) rounds to fp32 first"""
    rots, trans, intrins, post_rots, post_trans = [np.asarray(m, F) for m in mats]
    return D.project(np.asarray(centres).astype(F), D.inverse(rots), trans, intrins, post_rots, post_trans)


def visible_rows(centres, mats, H, W, zbuffer=zbuffer_loop):
    """bool [N]: the centre wins a pixel in any camera (loading.py:301-321)"""
    u, v, d = projected(centres, mats)
    seen = np.zeros((u.shape[0], u.shape[1]))
    for cam in range(u.shape[1]):
        with np.errstate(invalid="ignore"):
            mask = (u[:, cam] >= 0) & (u[:, cam] < F(W)) & (v[:, cam] >= 0) & (v[:, cam] < F(H)) & (d[:, cam] >= 0)
            t = d[mask, cam] * F(10)
            keep = t < F(32768)          # the int16 cast beyond is undefined; such a depth can never win (2048 <= it)
        pix = np.stack([u[mask, cam][keep], v[mask, cam][keep], t[keep]], 1).astype(np.int16)
        flags = np.zeros(int(mask.sum()), dtype=bool)
        flags[keep] = zbuffer(pix, H, W)
        seen[mask, cam] = flags
    return seen.sum(1) > 0


def img_visible_mask(occ, grid, pc_range, bda_rot, mats, H, W, vote=vote_loop, zbuffer=zbuffer_loop):
    centres, coords, label = occupancy2_rows(occ, grid, pc_range, bda_rot)
    flags = visible_rows(centres, mats, H, W, zbuffer).reshape(-1, 1).astype(label.dtype)
    return vote(np.zeros(grid, dtype=np.uint8), sort_pairs(coords, flags))


def lidar_visible_mask(points, grid, pc_range, vote=vote_loop):
    r, vs = np.array(pc_range), voxel_size(grid, pc_range)
    pts = np.asarray(points)[:, :3]
    with np.errstate(invalid="ignore"):
        pts = pts[((pts >= r[:3]) & (pts < r[3:])).sum(1) == 3]
    pts = (pts - r[:3]) / vs
    return vote(np.zeros(grid, dtype=np.uint8), sort_pairs(pts, np.ones((pts.shape[0], 1)).astype(pts.dtype)))


# ------------------------------------------------------------------ form C and points_occ
def mapped_labels(seg, learning_map):
    return np.vectorize(learning_map.__getitem__, otypes=[np.int64])(np.asarray(seg, np.uint8).reshape(-1, 1))


def points_occ(points, seg, learning_map, bda_rot):
    """the reference's lidarseg array as float32 [P, 4]; a zero label column without seg (is_test_submit)"""
    pts = np.asarray(points)[:, :3]
    label = mapped_labels(seg, learning_map) if seg is not None else np.zeros((pts.shape[0], 1))
    lidarseg = np.concatenate([pts, label], axis=-1)
    with np.errstate(invalid="ignore"):
        lidarseg[:, :3] = pts @ np.asarray(bda_rot, F).T
    return lidarseg


def nusc_annotations(points, seg, learning_map, bda_rot, grid, pc_range, unoccupied_id=17, vote=vote_loop):
    """(gt_occ uint8, points_occ float32): non-finite points are left out of the vote (the reference's cast of them is undefined)"""
    r, vs = np.array(pc_range), voxel_size(grid, pc_range)
    lidarseg = points_occ(points, seg, learning_map, bda_rot)
    fin = lidarseg[np.isfinite(lidarseg[:, :3]).all(1)]
    ind = np.floor((np.clip(fin[:, :3], r[:3], r[3:] - 1e-5) - r[:3]) / vs).astype(int)
    vol = vote(np.ones(grid, dtype=np.uint8) * np.uint8(unoccupied_id), sort_pairs(ind, fin[:, -1:]))
    vol[vol == 0] = 255
    vol[vol == unoccupied_id] = 0
    return vol, lidarseg.astype(F)


# ------------------------------------------------------------------ aabb
def pose_fields(seed=0):
    g = np.random.default_rng([77, seed])
    q1, q2 = g.standard_normal(4), g.standard_normal(4)
    return dict(lidar2ego_rotation=list(q1 / np.linalg.norm(q1)), lidar2ego_translation=list(g.uniform(-2, 2, 3)),
                ego2global_rotation=list(q2 / np.linalg.norm(q2) * 1.0000001), ego2global_translation=list(g.uniform(-900, 900, 3)))


def aabb(points, results):
    """float32 [2, 3] with numpy's float64 matmuls (BLAS), as the reference; ``aabb_ordered`` is the left-to-right form"""
    pT = np.asarray(points)[:, :3].copy().T
    pT = R.quat_matrix(results['lidar2ego_rotation']) @ pT
    pT = pT + np.array(results['lidar2ego_translation'])[:, np.newaxis]
    pT = R.quat_matrix(results['ego2global_rotation']) @ pT
    pT = (pT + np.array(results['ego2global_translation'])[:, np.newaxis]).T
    return torch.stack([torch.Tensor([pT[:, 0].min(), pT[:, 1].min(), pT[:, 2].min()]),
                        torch.Tensor([pT[:, 0].max(), pT[:, 1].max(), pT[:, 2].max()])]).numpy()


def aabb_ordered(points, results):
    p = np.asarray(points)[:, :3].astype(np.float64)
    for q, t in ((results['lidar2ego_rotation'], results['lidar2ego_translation']),
                 (results['ego2global_rotation'], results['ego2global_translation'])):
        m, t = R.quat_matrix(q), np.asarray(t, np.float64)
        p = np.stack([((m[i, 0] * p[:, 0] + m[i, 1] * p[:, 1]) + m[i, 2] * p[:, 2]) + t[i] for i in range(3)], 1)
    return np.stack([p.min(0), p.max(0)]).astype(F)


def ulps(a, b):
    """distance in float32 steps, elementwise (finite values of one sign pattern order as their bits)"""
    a, b = np.asarray(a, F).view(np.int32).astype(np.int64), np.asarray(b, F).view(np.int32).astype(np.int64)
    a, b = np.where(a < 0, -(a & 0x7FFFFFFF), a), np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


# ------------------------------------------------------------------ cases
def rows(N, C=4, hi=(GRID[2], GRID[1], GRID[0]), seed=0, labels=18, dtype=np.int64, label_col=-1):
    """annotation rows [N, C]: column i below hi[i] for the three indices, a label below ``labels`` in ``label_col``, small noise in
    the others (the velocity columns of the 7-wide files)"""
    g = np.random.default_rng([seed, N, C])
    out = g.integers(0, 6, (N, C))
    for i in range(3):
        out[:, i] = g.integers(0, hi[i], N)
    out[:, label_col] = g.integers(0, labels, N)
    return out.astype(dtype)


def grid_cloud(P, pc_range=PC_RANGE, seed=0, C=5, spill=0.15):
    """float32 [P, C] points about the range, a share of them outside on every side"""
    g = np.random.default_rng([seed, P, 9])
    r = np.asarray(pc_range)
    span = r[3:] - r[:3]
    pts = g.uniform(0, 31, (P, C)).astype(F)
    pts[:, :3] = (r[:3] - spill * span + g.random((P, 3)) * (1 + 2 * spill) * span).astype(F)
    return pts


def seg_bytes(P, learning_map, seed=0):
    g = np.random.default_rng([seed, P, 3])
    return np.asarray(sorted(learning_map), np.uint8)[g.integers(0, len(learning_map), P)]


def border_points(pc_range=PC_RANGE):
    """form C's borders: exactly on lo, on hi, at hi - 1e-5, one float below / above, far outside on each side"""
    r = np.asarray(pc_range)
    lo, hi = r[:3].astype(F), r[3:].astype(F)
    mid = ((r[:3] + r[3:]) / 2).astype(F)
    out = [lo, hi, (r[3:] - 1e-5).astype(F), np.nextafter(lo, F(-np.inf)), np.nextafter(lo, F(np.inf)), np.nextafter(hi, F(-np.inf)),
           np.nextafter(hi, F(np.inf)), lo - F(100), hi + F(100)]
    for a in range(3):
        for v in (lo[a], hi[a], np.nextafter(hi[a], F(-np.inf)), lo[a] - F(7), hi[a] + F(7)):
            p = mid.copy()
            p[a] = v
            out.append(p)
    return np.stack(out).astype(F)


SMALL = D.SMALL                      # two cameras of the synthetic rig at 24 x 40
GOLDEN_CAMS = D.GOLDEN_CAMS
GOLDEN_ROWS = 230


def small_rig():
    return D.rig(SMALL, cams=GOLDEN_CAMS)


def distinct_rows(N, grid, seed=0, labels=18):
    """[N, 4] rows (z, y, x, label) as the annotation files have them: every voxel once, in random order, before any repeats -- a
    voxel with one row takes that row's visible flag, one with more votes"""
    g = np.random.default_rng([seed, N, 5])
    V = grid[0] * grid[1] * grid[2]
    lin = np.r_[g.permutation(V), g.integers(0, V, max(N - V, 0))][:N]
    x, y, z = np.unravel_index(lin, grid)
    return np.stack([z, y, x, g.integers(0, labels, N)], 1).astype(np.int64)


def golden_pose(gold):
    """the pose fields dict of tests/golden/occ_gt.npz"""
    sizes = dict(ego2global_rotation=4, ego2global_translation=3, lidar2ego_rotation=4, lidar2ego_translation=3)
    out, at = {}, 0
    for k in [str(s) for s in gold["pose_keys"]]:
        out[k] = list(gold["pose"][at:at + sizes[k]])
        at += sizes[k]
    return out
