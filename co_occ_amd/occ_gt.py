"""Occupancy ground truth from the annotation rows.

The reference's LoadOccupancy, LoadOccupancy2 (P/datasets/pipelines/loading.py:59-134, 217-353) and LoadNuscOccupancyAnnotations
(loading_nusc_occ.py:61-137) build ``gt_occ`` -- and ``bda_rot``, ``aabb``, ``points_occ``, the visibility masks -- on one host core
and send the dense volume to the device (10.5 MB at 512 x 512 x 40).  Here the rows go up as narrow integers (8 bytes a row) with the
cloud, through ONE pinned staging buffer and one copy, and csrc/occ_gt.hip writes the volume: the reference's integers, bit for bit.

The rules:
  * form A (LoadOccupancy): an indexed assignment, **the last row of a voxel wins**; the volume starts at 0 and is NOT transformed by
    ``bda_rot`` (the reference's quirk, kept).
  * forms B and C and the masks: **a voxel holds the label with the largest row count modulo 65 536, the lowest label among equals**
    (the reference's uint16 counter and ``np.argmax``), independent of the row order.
  * the camera mask: a pixel's winner is the lexicographic minimum of ``(int(d * 10), row)`` among depths below 2048.
  * ``rotate_bda != 0`` is refused: the reference sorts form B's rows by their FLOAT coordinates, a voxel's rows are then not
    adjacent, and its loop writes the voxel once per fragment -- an accident of the sort.  Every config has ``rot_lim = (0, 0)``.

mmdet ``PIPELINES`` run in DataLoader worker processes, which must not open the GPU: the workers read the files (``np.load``,
``np.fromfile``) and the three classes are called in the main process on the arrays, as ``image_inputs.LoadMultiViewFrames`` is.
"""
import ctypes

import numpy as np
import torch

from . import _lib, core, depth_maps
from . import image_inputs as II
from ._lib import ptr
from .staging import HostStage, check_points, device_points, device_tensor

MAX_VOXELS = 1 << 24         # keys voxel * 256 + label in 32 bits


# ------------------------------------------------------------------ the augmentation
def sample_3d_augmentation(conf, rng=np.random):
    """``(rotate_bda, scale_bda, flip_dx, flip_dy, flip_dz)``: the reference's five draws in its order."""
    rotate_bda = rng.uniform(*conf['rot_lim'])
    scale_bda = rng.uniform(*conf['scale_lim'])
    flip_dx = rng.uniform() < conf['flip_dx_ratio']
    flip_dy = rng.uniform() < conf['flip_dy_ratio']
    flip_dz = rng.uniform() < conf.get('flip_dz_ratio', 0.0)
    return rotate_bda, scale_bda, flip_dx, flip_dy, flip_dz


def bda_matrix(rotate_bda=0.0, scale_bda=1.0, flip_dx=False, flip_dy=False, flip_dz=False):
    """``voxel_transform(None, ...)``'s fp32 ``[3,3]`` matrix (loading_nusc_occ.py:157-194), on the CPU: the flips times the BEV
    rotation; ``scale_bda`` is ignored, as upstream ignores it."""
    angle = torch.tensor(rotate_bda / 180 * np.pi)
    s, c = torch.sin(angle), torch.cos(angle)
    rot = torch.Tensor([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    flip = torch.eye(4)
    for on, axis in ((flip_dx, 0), (flip_dy, 1), (flip_dz, 2)):
        if on:
            m = torch.eye(4)
            m[axis, axis] = -1
            flip = flip @ m
    return (flip @ rot)[:3, :3]


# ------------------------------------------------------------------ checks
def _grid(grid_size):
    g = tuple(int(v) for v in np.asarray(grid_size).reshape(-1))
    if len(g) != 3 or min(g) < 1 or max(g) > 65535:
        raise ValueError("grid_size must be three extents of 1 .. 65535, got %s" % (grid_size,))
    if g[0] * g[1] * g[2] > MAX_VOXELS:
        raise ValueError("a grid of %d x %d x %d has more than 2^24 voxels: the vote's keys are voxel * 256 + label in 32 bits" % g)
    return g


def _range(pc_range, grid):
    r = np.asarray(pc_range, np.float64).reshape(-1)
    if r.shape != (6,) or not np.all(np.isfinite(r)) or not np.all(r[3:] > r[:3]):
        raise ValueError("pc_range must be six finite numbers lo < hi, got %s" % (pc_range,))
    return r, (r[3:] - r[:3]) / np.asarray(grid)          # voxel_size in float64, as the reference makes it


def _doubles(vals):
    v = [float(x) for x in vals]
    return (ctypes.c_double * len(v))(*v)


def _bda_host(bda):
    """host fp32 [9] of a bda matrix (None: NULL, the identity)"""
    if bda is None:
        return None
    m = bda.detach().cpu().numpy() if isinstance(bda, torch.Tensor) else np.asarray(bda)
    if m.shape != (3, 3):
        raise ValueError("bda_rot must be [3,3], got %s" % (m.shape,))
    return _lib.host_f32(np.asarray(m, np.float32).reshape(-1))


def pack_rows(occ, label_col=3, grid_size=None, to_float32=False):
    """uint16 ``[N,4]`` (the three index columns, the label) of annotation rows ``[N, >=4]`` as ``np.load`` returns them; the indices
    are truncated as ``astype(int)`` truncates them.  ``to_float32`` (form A): the rows are rounded to float32 first, as
    ``occ.astype(np.float32)`` rounds them there -- a float64 index of 4 - 1e-12 is 4.  ``ValueError``: labels outside 0 .. 255,
    indices outside 0 .. 65535 (outside ``grid_size`` when given: form A's indexed assignment would raise or wrap there)."""
    occ = np.asarray(occ)
    if occ.ndim != 2 or occ.shape[1] < 4 or occ.dtype.kind not in "iuf":
        raise ValueError("annotation rows must be a numeric [N, >= 4] array, got %s %s" % (occ.dtype, occ.shape))
    idx, lab = occ[:, :3], occ[:, label_col]
    if to_float32 and occ.dtype.kind == "f":          # integers inside a grid (below 2^24) are float32 numbers already
        idx, lab = idx.astype(np.float32), lab.astype(np.float32)
    if idx.dtype.kind == "f":
        if not (np.all(np.isfinite(idx)) and np.all(np.isfinite(lab))):
            raise ValueError("annotation rows hold non-finite values")
        idx, lab = np.trunc(idx), np.trunc(lab)
    if occ.shape[0]:
        if lab.min() < 0 or lab.max() > 255:
            raise ValueError("labels must lie in 0 .. 255, got %s .. %s" % (lab.min(), lab.max()))
        hi = np.asarray(grid_size if grid_size is not None else (65536,) * 3)
        if idx.min() < 0 or np.any(idx.max(0) >= hi):
            raise ValueError("row indices %s .. %s lie outside %s" % (idx.min(0), idx.max(0), "the grid %s" % (tuple(hi),) if grid_size is not None
                                                                        else "0 .. 65535"))
    out = np.empty((occ.shape[0], 4), np.uint16)
    out[:, :3] = idx
    out[:, 3] = lab
    return out


SCRATCH_KINDS = ("occ_gt_win", "occ_gt_vote", "occ_gt_canvas", "occ_gt_aabb")


def release_scratch():
    """Drop this module's per-stream scratch buffers from the registry (``core.stream_buffer``): at 512 x 512 x 40 with six
    896 x 1600 cameras they are 42 MB (form A's uint32 winners), 69 MB (the z-buffer canvas) and a few MB of sort storage per
    stream, kept for the life of the process otherwise.  The next call allocates them again.  Returns the bytes let go."""
    gone = [k for k in core._stream_bufs if k[2] in SCRATCH_KINDS]
    return sum(t.numel() * t.element_size() for t in (core._stream_bufs.pop(k) for k in gone))


# ------------------------------------------------------------------ the kernels alone
def scatter_labels(rows, grid_size, use_semantic=True, out=None):
    """Form A: uint8 ``[G0,G1,G2]`` with ``vol[i0,i1,i2] = label`` for every row of ``rows`` (device int16 ``[N,4]`` holding
    ``pack_rows``' uint16 bits), 0 elsewhere; the last row of a voxel wins.  ``use_semantic``: label 0 is written as 255; without it
    rows of label 0 are dropped and the rest write 1."""
    g = _grid(grid_size)
    rows = device_tensor("rows", rows, torch.int16, 4)
    if rows.shape[0] >= (1 << 24) - 1:
        raise ValueError("scatter_labels takes fewer than 2^24 - 1 rows, got %d" % rows.shape[0])
    V = g[0] * g[1] * g[2]
    if out is None:
        out = torch.empty(g, dtype=torch.uint8, device=rows.device)
    elif tuple(out.shape) != g or out.dtype != torch.uint8:
        raise ValueError("out must be uint8 %s, got %s %s" % (g, out.dtype, tuple(out.shape)))
    win = core.stream_buffer(rows.device, "occ_gt_win", V, torch.int32)
    _lib.call("coocc_occ_scatter_labels", ptr(rows) if rows.shape[0] else ptr(None), rows.shape[0], g[0], g[1], g[2], int(bool(use_semantic)),
              ptr(win), ptr(out, torch.uint8))
    return out


def rows_to_voxels(rows, grid_size, pc_range, bda_rot=None, centres=True):
    """Form B's row arithmetic: ``(vox int32 [N], labels uint8 [N], centres fp32 [N,3] or None)`` -- the linear voxel of every row
    after ``bda_rot`` (fp32 ``[3,3]``, host or device; None: identity) and the clip, its label with 0 as 255, and the untransformed
    fp32 centres the camera mask projects."""
    g = _grid(grid_size)
    r, vs = _range(pc_range, g)
    rows = device_tensor("rows", rows, torch.int16, 4)
    N = rows.shape[0]
    vox = torch.empty(N, dtype=torch.int32, device=rows.device)
    labels = torch.empty(N, dtype=torch.uint8, device=rows.device)
    cen = torch.empty((N, 3), dtype=torch.float32, device=rows.device) if centres else None
    if N:
        _lib.call("coocc_occ_rows_to_voxels", ptr(rows), N, _doubles(list(r[:3]) + list(vs)), _bda_host(bda_rot), g[0], g[1], g[2],
                  ptr(vox), ptr(labels), ptr(cen))
    return vox, labels, cen


def points_to_voxels(points, mode, grid_size=None, pc_range=None, bda_rot=None, lidarseg=None, table=None, points_occ=False):
    """One pass over the cloud (device fp32 ``[P, C >= 3]``).  ``mode`` "none" | "annotation" (form C: clip to ``[lo, hi - 1e-5]``,
    floor; non-finite points do not vote) | "lidar_mask" (form B's LiDAR branch: points inside ``[lo, hi)``, truncation, label 1).
    ``lidarseg``: device uint8 ``[P]`` mapped through ``table`` (device uint8 ``[256]``).  Returns ``(vox, labels, points_occ)`` with
    None for what was not asked; ``points_occ`` is fp32 ``[P,4]``: ``xyz @ bda_rot^T`` and the mapped label (0 without lidarseg)."""
    m = {"none": 0, "annotation": 1, "lidar_mask": 2}.get(mode)
    if m is None:
        raise ValueError("mode must be 'none', 'annotation' or 'lidar_mask', got %r" % (mode,))
    points = device_points(points)
    P, dev = points.shape[0], points.device
    g, grid = (1, 1, 1), None
    if m:
        g = _grid(grid_size)
        r, vs = _range(pc_range, g)
        grid = _doubles(list(r[:3]) + list(r[3:] - 1e-5 if m == 1 else r[3:]) + list(vs))
    if lidarseg is not None:
        lidarseg, table = device_tensor("lidarseg", lidarseg, torch.uint8, dim=1), device_tensor("table", table, torch.uint8, 256, dim=1)
        if lidarseg.shape[0] != P:
            raise ValueError("%d lidarseg bytes for %d points" % (lidarseg.shape[0], P))
    if m == 0 and not points_occ:
        raise ValueError("mode 'none' makes points_occ only")
    vox = torch.empty(P, dtype=torch.int32, device=dev) if m else None
    labels = torch.empty(P, dtype=torch.uint8, device=dev) if m else None
    pocc = torch.empty((P, 4), dtype=torch.float32, device=dev) if points_occ else None
    if P:
        _lib.call("coocc_occ_points_to_voxels", ptr(points, torch.float32), P, points.shape[1], ptr(lidarseg), ptr(table), _bda_host(bda_rot), grid,
                  g[0], g[1], g[2], m, ptr(vox), ptr(labels), ptr(pocc))
    return vox, labels, pocc


def vote_labels(vox, labels, grid_size, fill=0, post_empty=None, out=None):
    """The majority vote (the reference's ``nb_process_label``): uint8 ``[G0,G1,G2]`` = ``fill``, and for every voxel named in ``vox``
    (device int32 ``[N]``, linear; negative or too large: no vote) the label of ``labels`` (device uint8 ``[N]``) with the largest
    count modulo 65 536, the lowest among equals.  ``post_empty`` (form C): a written 0 becomes 255, then ``post_empty`` becomes 0 --
    ``fill`` is written as given.  One radix sort and one run-length pass; the same bytes for every order of the rows."""
    g = _grid(grid_size)
    vox, labels = device_tensor("vox", vox, torch.int32, dim=1), device_tensor("labels", labels, torch.uint8, dim=1)
    N = vox.shape[0]
    if labels.shape[0] != N or labels.device != vox.device:
        raise ValueError("vox [%d] on %s, labels [%d] on %s" % (N, vox.device, labels.shape[0], labels.device))
    if not 0 <= int(fill) <= 255 or (post_empty is not None and not 0 <= int(post_empty) <= 255):
        raise ValueError("fill and post_empty are labels 0 .. 255, got %s, %s" % (fill, post_empty))
    if out is None:
        out = torch.empty(g, dtype=torch.uint8, device=vox.device)
    elif tuple(out.shape) != g or out.dtype != torch.uint8:
        raise ValueError("out must be uint8 %s, got %s %s" % (g, out.dtype, tuple(out.shape)))
    need = _lib.load().coocc_occ_vote_ws(N)
    ws = core.stream_buffer(vox.device, "occ_gt_vote", need, torch.uint8)
    _lib.call("coocc_occ_vote_labels", ptr(vox) if N else ptr(None), ptr(labels) if N else ptr(None), N, g[0] * g[1] * g[2], int(fill),
              -1 if post_empty is None else int(post_empty), ptr(out, torch.uint8), ptr(ws), ws.numel())
    return out


def visible_rows(centres, table, size):
    """uint8 ``[N]``: 1 where the centre (device fp32 ``[N,3]``) wins a pixel of any camera of ``table`` (device fp32 ``[n,28]``,
    ``depth_maps.camera_table``) at ``size = (H, W)`` -- the reference's per-camera z-buffer ``nb_process_img_points``."""
    centres = device_tensor("centres", centres, torch.float32, 3)
    table = device_tensor("table", table, torch.float32, depth_maps.CAM_FLOATS)
    H, W = int(size[0]), int(size[1])
    if not (1 <= H <= 32767 and 1 <= W <= 32767) or table.shape[0] < 1:
        raise ValueError("size (H, W) within 1 .. 32767 and one camera at least; got %s, %d cameras" % ((H, W), table.shape[0]))
    N = centres.shape[0]
    flags = torch.empty(N, dtype=torch.uint8, device=centres.device)
    if N:
        canvas = core.stream_buffer(centres.device, "occ_gt_canvas", table.shape[0] * H * W, torch.int64)
        _lib.call("coocc_occ_visible_rows", ptr(centres), N, ptr(table), table.shape[0], H, W, ptr(canvas), ptr(flags))
    return flags


def visible_masks(centres, vox, grid_size, table=None, size=None, lidar_points=None, pc_range=None):
    """Form B's ``cal_visible`` volumes (loading.py:296-346) as a dict: ``img_visible_mask`` when ``table`` is given (the vote of the
    rows' visible flags at their voxels ``vox``), ``lidar_visible_mask`` when ``lidar_points`` is (device fp32 ``[P, C >= 3]``), and
    ``visible_mask``, their union."""
    g = _grid(grid_size)
    out = {}
    if table is not None:
        out["img_visible_mask"] = vote_labels(vox, visible_rows(centres, table, size), g, fill=0)
    if lidar_points is not None:
        lv, ll, _ = points_to_voxels(lidar_points, "lidar_mask", g, pc_range)
        out["lidar_visible_mask"] = vote_labels(lv, ll, g, fill=0)
    masks = list(out.values())
    out["visible_mask"] = (masks[0] | masks[1] if len(masks) == 2 else masks[0].clone() if masks
                           else torch.zeros(g, dtype=torch.uint8, device=vox.device))
    return out


def pose_doubles(results):
    """host doubles r1[9] t1[3] r2[9] t2[3] of ``results``' lidar2ego and ego2global fields (scalar-first quaternions)"""
    r1 = II.quaternion_rotation_matrix(results['lidar2ego_rotation'])
    r2 = II.quaternion_rotation_matrix(results['ego2global_rotation'])
    t1 = np.asarray(results['lidar2ego_translation'], np.float64).reshape(3)
    t2 = np.asarray(results['ego2global_translation'], np.float64).reshape(3)
    return np.concatenate([r1.reshape(-1), t1, r2.reshape(-1), t2])


def cloud_aabb(points, results):
    """fp32 ``[2,3]``: the min / max of the cloud (device fp32 ``[P >= 1, C >= 3]``) in the global frame -- lidar to ego, ego to global,
    in float64 on the device, rounded once.  A NaN coordinate makes the axes it reaches NaN, as numpy's min / max do."""
    points = device_points(points, min_rows=1)
    aabb = torch.empty((2, 3), dtype=torch.float32, device=points.device)
    slots = core.stream_buffer(points.device, "occ_gt_aabb", 6, torch.int64)
    _lib.call("coocc_occ_cloud_aabb", ptr(points, torch.float32), points.shape[0], points.shape[1], _doubles(pose_doubles(results)), ptr(slots),
              ptr(aabb))
    return aabb


# ------------------------------------------------------------------ the three loaders
def _learning_map(cls_metas, learning_map):
    if learning_map is None:
        import yaml
        with open(cls_metas, 'r') as stream:
            learning_map = yaml.safe_load(stream)['learning_map']
    table, known = np.zeros(256, np.uint8), np.zeros(256, bool)
    for k, v in learning_map.items():
        if not (0 <= int(k) <= 255 and 0 <= int(v) <= 255):
            raise ValueError("learning_map entry %s -> %s lies outside 0 .. 255" % (k, v))
        table[int(k)], known[int(k)] = int(v), True
    return table, known


class _Loader:
    form = None

    def _init(self, grid_size, pc_range, is_train, is_test_submit, bda_aug_conf, cls_metas, learning_map, device, rng, need_map):
        self.grid_size = np.array(grid_size)
        self.grid = _grid(grid_size)
        self.pc_range, self.voxel_size = _range(pc_range, self.grid)
        self.is_train, self.is_test_submit, self.bda_aug_conf = is_train, is_test_submit, bda_aug_conf
        self.cls_metas, self.device, self.rng = cls_metas, torch.device(device), rng
        self.table = self.known = self._table_dev = None
        if need_map or learning_map is not None:
            self.table, self.known = _learning_map(cls_metas, learning_map)
        self._stage = HostStage(self.device)

    def sample_3d_augmentation(self):
        return sample_3d_augmentation(self.bda_aug_conf, self.rng)

    def _bda(self):
        """the sample's fp32 [3,3] bda matrix on the CPU (identity in eval)"""
        if not self.is_train:
            return torch.eye(3).float()
        rotate_bda, scale_bda, fx, fy, fz = self.sample_3d_augmentation()
        if rotate_bda != 0:
            raise NotImplementedError("rotate_bda = %s: the reference's vote over rows sorted by float coordinates writes a voxel once per "
                                      "fragment (DESIGN.md 16); every config has rot_lim = (0, 0)" % rotate_bda)
        return bda_matrix(rotate_bda, scale_bda, fx, fy, fz)

    def _cloud(self, points):
        return check_points(points if isinstance(points, torch.Tensor) else np.asarray(points))

    def _seg_bytes(self, lidarseg, P):
        seg = lidarseg.numpy() if isinstance(lidarseg, torch.Tensor) else np.asarray(lidarseg)
        if seg.dtype != np.uint8 or seg.size != P:
            raise ValueError("lidarseg must be %d uint8 bytes, got %s %s" % (P, seg.dtype, seg.shape))
        seg = seg.reshape(-1)
        missing = np.flatnonzero(np.bincount(seg, minlength=256).astype(bool) & ~self.known)
        if missing.size:
            raise ValueError("lidarseg bytes %s are not in learning_map" % missing.tolist())
        return seg

    def _table(self):
        if self._table_dev is None:
            self._table_dev = torch.from_numpy(self.table).to(self.device)
        return self._table_dev

    def _tuples(self, out, img_inputs, gt_depths, bda_dev, aabb, with_size):
        if img_inputs is not None:
            if len(img_inputs) != 12:
                raise ValueError("img_inputs must be the loader's 12-tuple, got %d elements" % len(img_inputs))
            out["img_inputs"] = II.with_bda(img_inputs, bda_dev, aabb, batch=False)
            if self.form != "A":
                t = out["img_inputs"]
                out["gt_depths"] = tuple(t[1:8]) + ((t[13],) if with_size else ())
        elif gt_depths is not None:
            if len(gt_depths) != 9:
                raise ValueError("gt_depths must be the LiDAR-only 9-tuple, got %d elements" % len(gt_depths))
            out["gt_depths"] = depth_maps.lidar_gt_depths(gt_depths, bda_dev, batch=False)

    def _test_submit(self, points, img_inputs):
        """the is_test_submit form: the 9-tuple with the identity at index 6, points_occ with label 0"""
        out = {}
        d = self._stage.named(dict(points=self._cloud(points), bda=np.eye(3, dtype=np.float32)))
        if img_inputs is not None:
            if len(img_inputs) != 8:
                raise ValueError("is_test_submit reads the 8-tuple (imgs, rots, trans, intrins, post_rots, post_trans, gt_depths, "
                                 "sensor2sensors), got %d elements" % len(img_inputs))
            out["img_inputs"] = tuple(img_inputs[:6]) + (d["bda"],) + tuple(img_inputs[6:])
        out["points_occ"] = points_to_voxels(d["points"], "none", points_occ=True)[2]
        return out

    def _cast(self, vol, dtype):
        return vol if dtype in (None, torch.uint8) else vol.to(dtype)


class LoadOccupancy(_Loader):
    """The reference's LoadOccupancy on the device (form A).  ``loader(occ, points, results, img_inputs=... | gt_depths=...)`` with
    ``occ`` the rows ``[N, >= 4]`` of the sample's ``.npy`` (indices in columns 0 .. 2, the label in column 3), ``points`` the key-frame
    cloud fp32 ``[P, C >= 3]`` and ``results`` the dict with the four pose fields; returns a dict with ``gt_occ`` (uint8;
    ``dtype=torch.float64`` gives the reference's), ``bda_rot``, ``aabb`` and the ``img_inputs`` 14-tuple or the ``gt_depths`` 8-tuple.
    ``gt_occ`` is not transformed by ``bda_rot``: the reference's quirk."""
    form = "A"

    def __init__(self, to_float32=True, use_semantic=True, occ_path=None, grid_size=[512, 512, 40], unoccupied=0,
                 pc_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], gt_resize_ratio=1, cal_visible=False, use_vel=False, data_root='data/nuscenes',
                 is_train=False, is_test_submit=False, bda_aug_conf=None, cls_metas='nuscenes.yaml', learning_map=None, device="cuda",
                 rng=np.random):
        if use_vel:
            raise NotImplementedError("use_vel=True (gt_vel) is not restated")
        self.to_float32, self.use_semantic, self.occ_path, self.unoccupied = to_float32, use_semantic, occ_path, unoccupied
        self.gt_resize_ratio, self.cal_visible, self.use_vel, self.data_root = gt_resize_ratio, cal_visible, use_vel, data_root
        self._init(grid_size, pc_range, is_train, is_test_submit, bda_aug_conf, cls_metas, learning_map, device, rng, need_map=False)

    def __call__(self, occ, points, results, img_inputs=None, gt_depths=None, dtype=None):
        if self.is_test_submit:
            return self._test_submit(points, img_inputs)
        bda = self._bda()
        d = self._stage.named(dict(rows=pack_rows(occ, 3, self.grid, to_float32=True), points=self._cloud(points), bda=bda.numpy()))
        out = dict(bda_rot=d["bda"], aabb=cloud_aabb(d["points"], results))
        out["gt_occ"] = self._cast(scatter_labels(d["rows"], self.grid, self.use_semantic), dtype)
        self._tuples(out, img_inputs, gt_depths, d["bda"], out["aabb"], True)
        return out


class LoadOccupancy2(_Loader):
    """The reference's LoadOccupancy2 on the device (form B): ``loader(occ, points, lidarseg, results, img_inputs, lidar_points=None)``.
    ``occ``: integer rows ``[N, >= 4]`` (z y x ... label last); ``lidarseg``: the cloud's uint8 label bytes; ``lidar_points``: what the
    reference reads from ``results['points']`` for the LiDAR mask.  Returns ``gt_occ`` (uint8), ``points_occ``, ``bda_rot``, ``aabb``,
    the ``img_inputs`` 14-tuple, ``gt_depths`` and, with ``cal_visible``, the three masks."""
    form = "B"

    def __init__(self, to_float32=True, use_semantic=False, occ_path=None, grid_size=[512, 512, 40], unoccupied=0,
                 pc_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], gt_resize_ratio=1, cal_visible=False, use_vel=False, data_root='data/nuscenes',
                 is_train=False, is_test_submit=False, bda_aug_conf=None, cls_metas='nuscenes.yaml', learning_map=None, device="cuda",
                 rng=np.random):
        if use_vel:
            raise NotImplementedError("use_vel=True (gt_vel) is not restated")
        if not 0 <= int(unoccupied) <= 255:
            raise ValueError("unoccupied must be a label 0 .. 255, got %s" % (unoccupied,))
        self.to_float32, self.use_semantic, self.occ_path, self.unoccupied = to_float32, use_semantic, occ_path, unoccupied
        self.gt_resize_ratio, self.cal_visible, self.use_vel, self.data_root = gt_resize_ratio, cal_visible, use_vel, data_root
        self._init(grid_size, pc_range, is_train, is_test_submit, bda_aug_conf, cls_metas, learning_map, device, rng, need_map=not is_test_submit)

    def __call__(self, occ, points, lidarseg, results, img_inputs=None, gt_depths=None, lidar_points=None, table=None, dtype=None):
        if self.is_test_submit:
            return self._test_submit(points, img_inputs)
        occ = np.asarray(occ)
        if occ.dtype.kind not in "iu" and occ.dtype != np.float64:
            raise ValueError("form B reads integer (or float64) rows: (idx + 0.5) is float64 arithmetic in the reference; got %s" % occ.dtype)
        if occ.dtype.kind == "f" and occ.size and not np.array_equal(occ[:, :3], np.trunc(occ[:, :3])):
            raise ValueError("form B's row indices must be whole numbers")
        bda = self._bda()
        pts = self._cloud(points)
        host = dict(rows=pack_rows(occ, -1), points=pts, bda=bda.numpy(), seg=self._seg_bytes(lidarseg, pts.shape[0]))
        if lidar_points is not None and self.cal_visible:
            host["lidar_points"] = self._cloud(lidar_points)
        if self.cal_visible and img_inputs is not None and table is None:
            small = [t.cpu() for t in img_inputs[1:6]]
            host["cams"] = depth_maps.camera_table(*small).numpy()
        d = self._stage.named(host)
        out = dict(bda_rot=d["bda"], aabb=cloud_aabb(d["points"], results))
        out["points_occ"] = points_to_voxels(d["points"], "none", bda_rot=bda, lidarseg=d["seg"], table=self._table(), points_occ=True)[2]
        vox, labels, centres = rows_to_voxels(d["rows"], self.grid, self.pc_range, bda, centres=self.cal_visible)
        out["gt_occ"] = self._cast(vote_labels(vox, labels, self.grid, fill=self.unoccupied), dtype)
        if self.cal_visible:
            cams = table if table is not None else d.get("cams")
            out.update(visible_masks(centres, vox, self.grid, cams, img_inputs[0].shape[-2:] if cams is not None else None,
                                     d.get("lidar_points"), self.pc_range))
        self._tuples(out, img_inputs, gt_depths, d["bda"], out["aabb"], False)
        return out


class LoadNuscOccupancyAnnotations(_Loader):
    """The reference's LoadNuscOccupancyAnnotations on the device (form C): ``loader(points, lidarseg, results, img_inputs)``; the
    volume is voted from the labelled cloud itself.  ``gt_occ`` is uint8 (``dtype=torch.long`` gives the reference's)."""
    form = "C"

    def __init__(self, data_root='data/nuscenes', is_train=False, is_test_submit=False, grid_size=None, point_cloud_range=None,
                 bda_aug_conf=None, unoccupied_id=17, cls_metas='nuscenes.yaml', learning_map=None, device="cuda", rng=np.random):
        if not 0 <= int(unoccupied_id) <= 255:
            raise ValueError("unoccupied_id must be a label 0 .. 255, got %s" % (unoccupied_id,))
        self.data_root, self.unoccupied_id = data_root, unoccupied_id
        self._init(grid_size, point_cloud_range, is_train, is_test_submit, bda_aug_conf, cls_metas, learning_map, device, rng,
                   need_map=not is_test_submit)
        self.point_cloud_range = self.pc_range
        self.transform_center = (self.pc_range[:3] + self.pc_range[3:]) / 2

    def __call__(self, points, lidarseg, results, img_inputs=None, gt_depths=None, dtype=None):
        if self.is_test_submit:
            return self._test_submit(points, img_inputs)
        bda = self._bda()
        pts = self._cloud(points)
        d = self._stage.named(dict(points=pts, bda=bda.numpy(), seg=self._seg_bytes(lidarseg, pts.shape[0])))
        out = dict(bda_rot=d["bda"], aabb=cloud_aabb(d["points"], results))
        vox, labels, out["points_occ"] = points_to_voxels(d["points"], "annotation", self.grid, self.pc_range, bda, d["seg"], self._table(),
                                                          points_occ=True)
        empty = int(self.unoccupied_id)
        fill = 255 if empty == 0 else 0          # the two rewrites applied to the unoccupied id itself: 0 -> 255, then empty -> 0
        out["gt_occ"] = self._cast(vote_labels(vox, labels, self.grid, fill=fill, post_empty=empty), dtype)
        self._tuples(out, img_inputs, gt_depths, d["bda"], out["aabb"], True)
        return out
