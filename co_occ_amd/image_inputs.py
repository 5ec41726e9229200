"""Camera ``img_inputs`` from decoded uint8 frames.

The reference's LoadMultiViewImageFromFiles_OccFormer (P/datasets/pipelines/loading_nusc_imgs.py:25-221) resizes every frame with
Pillow, crops, flips, converts to fp32 / 255 on the host and describes that with the small matrices of the tuple.  Here the frames go
to the device as bytes, ONE kernel (csrc/image_inputs.hip) makes ``imgs`` and ``canvas`` with Pillow's bits, and the matrices are made
on the host with the reference's float32 torch operations in the reference's order.

Pillow's 8-bit resize is integer arithmetic once its coefficient tables exist (``pillow_coeffs``): float64 coefficients, rounded to
22-bit fixed point, accumulation from 2^21, arithmetic shift, clamp to 0..255; horizontal pass first and stored as uint8, then the
vertical pass; a pass whose size does not change is skipped.

No mmcv, mmdet or pyquaternion is needed.  mmdet ``PIPELINES`` run in DataLoader worker processes, which must not open the GPU:
``LoadMultiViewFrames`` is called in the main process on frames the workers decoded.
"""
import collections
import ctypes
import functools
import math

import numpy as np
import torch

from . import _lib
from ._lib import CooccError, ptr, require_gpu
from .staging import HostStage, PointStage, device_points, device_tensor, pinned_upload

PRECISION_BITS = 22          # Pillow's 32 - 8 - 2
MAX_TAPS = 33                # csrc/image_inputs.hip II_KMAX: bicubic (support 2) at a downscale ratio of 8
MAX_RATIO = 8
CAM_INTS = 12                # per-camera header of coocc_frames_to_imgs
CAM_FLOATS = 28              # csrc/lidar_project.h LIDAR_CAM_FLOATS: inv_rot[9] tran[3] intrin[9] post_rot 2x2 [4] post_tran[2] pad


# ------------------------------------------------------------------ Pillow's coefficient tables
def _bicubic(x):
    """Pillow's bicubic kernel (a = -0.5), float64, in its operation order."""
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def tap_count(in_size, out_size):
    """Taps Pillow allots per output index: ceil(support * max(in / out, 1)) * 2 + 1 with the bicubic support of 2."""
    scale = float(in_size) / out_size
    return int(math.ceil(2.0 * max(scale, 1.0))) * 2 + 1


@functools.lru_cache(maxsize=64)
def pillow_coeffs(in_size, out_size):
    """(bounds int32 [out, 2] = (first source index, tap count), taps int32 [out, ksize]) of ``Image.resize`` along one axis from
    ``in_size`` to ``out_size`` samples: Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter over the whole
    axis.  Computed once per (in, out) and cached; the arrays are read-only."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("pillow_coeffs: sizes %d -> %d" % (in_size, out_size))
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # C's (int) truncates; negative values clamp to 0 anyway
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    w = _bicubic(((x + xmin[:, None]) - center[:, None] + 0.5) * ss)
    w = np.where(x < xmax[:, None], w, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]          # the sequential sum of the C loop (adding the masked zeros changes nothing)
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    taps = np.trunc(np.where(w < 0, -0.5, 0.5) + w * float(1 << PRECISION_BITS)).astype(np.int32)
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    bounds.setflags(write=False)
    taps.setflags(write=False)
    return bounds, taps


# ------------------------------------------------------------------ augmentation parameters and the matrices (host, reference bits)
def sample_augmentation(data_config, H, W, is_train, flip=None, scale=None, rng=np.random):
    """loading_nusc_imgs.py:87-111 -> (resize, resize_dims, crop, flip, rotate) with its Python arithmetic (``int()`` truncations
    included).  Training draws come from ``rng`` in the reference's order -- resize, crop height, crop width, flip, rotation -- and
    ``rng.choice`` is drawn only when ``data_config['flip']`` is true, so a seeded generator gives the reference's parameters."""
    fH, fW = data_config['input_size']
    resize = float(fW) / float(W)
    if is_train:
        resize += rng.uniform(*data_config['resize'])
    else:
        resize += data_config.get('resize_test', 0.0)
        if scale is not None:
            resize = scale
    newW, newH = int(W * resize), int(H * resize)
    if is_train:
        kept = 1 - rng.uniform(*data_config['crop_h'])
        x0 = int(rng.uniform(0, max(0, newW - fW)))
        flip = data_config['flip'] and rng.choice([0, 1])
        rotate = rng.uniform(*data_config['rot'])
    else:
        kept = 1 - np.mean(data_config['crop_h'])
        x0 = int(max(0, newW - fW) / 2)
        flip = False if flip is None else flip
        rotate = 0
    y0 = int(kept * newH) - fH
    return resize, (newW, newH), (x0, y0, x0 + fW, y0 + fH), flip, rotate


def post_transform(resize, crop, flip, rotate):
    """(post_rot [3,3], post_tran [3]) of loading_nusc_imgs.py:49-68 and 175-178: the same float32 torch CPU operations in the same
    order -- scale, minus the crop origin, the mirror about the crop width, the turn about the crop centre -- so the reference's
    bits."""
    x0, y0, x1, y1 = crop
    rot2, tran2 = torch.eye(2), torch.zeros(2)
    rot2 *= resize
    tran2 -= torch.Tensor([x0, y0])
    if flip:
        mirror = torch.Tensor([[-1, 0], [0, 1]])
        rot2 = mirror.matmul(rot2)
        tran2 = mirror.matmul(tran2) + torch.Tensor([x1 - x0, 0])
    h = rotate / 180 * np.pi
    turn = torch.Tensor([[np.cos(h), np.sin(h)], [-np.sin(h), np.cos(h)]])
    half = torch.Tensor([x1 - x0, y1 - y0]) / 2
    shift = turn.matmul(-half) + half
    rot2 = turn.matmul(rot2)
    tran2 = turn.matmul(tran2) + shift
    post_rot, post_tran = torch.eye(3), torch.zeros(3)
    post_rot[:2, :2] = rot2
    post_tran[:2] = tran2
    return post_rot, post_tran


def intrin_nerf(cam_intrinsic, resize, crop):
    """loading_nusc_imgs.py:143, 180-182: the intrinsics of the resized and cropped image."""
    k = torch.Tensor(np.asarray(cam_intrinsic))
    k[:2] = k[:2] * resize
    k[0, 2] -= crop[0]
    k[1, 2] -= crop[1]
    return k


def quaternion_rotation_matrix(q):
    """Rotation matrix [3,3] (float64) of the scalar-first quaternion (w, x, y, z), normalised first when it is not a unit
    quaternion -- what the reference reads from ``pyquaternion.Quaternion(q).rotation_matrix``: the lower right 3 x 3 block of the
    product of the left- and the conjugated right-multiplication matrices."""
    q = np.asarray(q, dtype=np.float64).reshape(4)
    ss = np.dot(q, q)
    if not abs(1.0 - ss) < 1e-14:
        n = math.sqrt(ss)
        if n > 0:
            q = q / n
    w, x, y, z = q
    left = np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])
    right = np.array([[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]])
    return np.dot(left, right.conj().transpose())[1:][:, 1:]


def pose_matrix(quat, translation):
    """4 x 4 float64 pose from a scalar-first quaternion and a translation."""
    m = np.eye(4)
    m[:3, :3] = quaternion_rotation_matrix(quat)
    m[:3, 3] = translation
    return m


def calibration(cam_data, lidar2cam):
    """The per-camera calibration tensors of loading_nusc_imgs.py:142-159 (CPU, float32): ``intrin``; ``cam2world`` = the float64
    product ego_pose @ cam_pose, then float32; ``sensor2lidar`` = inverse(lidar2cam) in float64, then ``.float()``; ``rot`` / ``tran``
    its blocks."""
    intrin = torch.Tensor(np.asarray(cam_data['cam_intrinsic']))
    cam_pose = pose_matrix(cam_data['sensor2ego_rotation'], cam_data['sensor2ego_translation'])
    ego_pose = pose_matrix(cam_data['ego2global_rotation'], cam_data['ego2global_translation'])
    cam2world = torch.Tensor(ego_pose @ cam_pose)
    sensor2lidar = torch.tensor(np.asarray(lidar2cam, dtype=np.float64)).inverse().float()
    return dict(intrin=intrin, cam2world=cam2world, sensor2lidar=sensor2lidar, rot=sensor2lidar[:3, :3], tran=sensor2lidar[:3, 3])


def choose_cams(data_config, is_train, rng=np.random):
    """The cameras of a sample: ``Ncams`` drawn from ``cams`` without replacement in training, else all of them."""
    if is_train and data_config['Ncams'] < len(data_config['cams']):
        return rng.choice(data_config['cams'], data_config['Ncams'], replace=False)
    return data_config['cams']


def require_calibration(cam_names, cam_infos, lidar2cam_dic):
    missing = [c for c in cam_names if c not in cam_infos or c not in lidar2cam_dic]
    if missing:
        raise ValueError("no calibration for cameras %s" % missing)


# ------------------------------------------------------------------ the LiDAR depth slot (the loaders are in depth_maps)
def camera_table(rots, trans, intrins, post_rots, post_trans):
    """The ``[N,28]`` host table of ``coocc_points_to_depth_maps`` from CPU fp32 tensors ``rots`` [N,3,3], ``trans`` [N,3],
    ``intrins`` [N,3,3], ``post_rots`` [N,3,3] (or [N,2,2]) and ``post_trans`` [N,3] (or [N,2]).  ``rots.inverse()`` is taken here, on
    the CPU and batched, as the reference calls it."""
    ts = dict(rots=rots, trans=trans, intrins=intrins, post_rots=post_rots, post_trans=post_trans)
    for k, t in ts.items():
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError("camera_table: %s must be a float32 tensor, got %s" % (k, getattr(t, "dtype", type(t).__name__)))
        if t.is_cuda:
            raise ValueError("camera_table: %s is on %s; the table is made on the host (rots.inverse() with the reference's bits)" % (k, t.device))
    if intrins.dim() == 3 and tuple(intrins.shape[-2:]) == (4, 4):
        raise NotImplementedError("camera_table: 4 x 4 intrinsics (the reference's KITTI form) are not restated; nuScenes' are 3 x 3")
    N = rots.shape[0] if rots.dim() == 3 else -1
    if N < 1 or tuple(rots.shape) != (N, 3, 3) or tuple(trans.shape) != (N, 3) or tuple(intrins.shape) != (N, 3, 3):
        raise ValueError("camera_table: rots [N,3,3], trans [N,3], intrins [N,3,3]; got %s, %s, %s"
                         % (tuple(rots.shape), tuple(trans.shape), tuple(intrins.shape)))
    if tuple(post_rots.shape) not in ((N, 3, 3), (N, 2, 2)) or tuple(post_trans.shape) not in ((N, 3), (N, 2)):
        raise ValueError("camera_table: post_rots [N,3,3] and post_trans [N,3] for N = %d; got %s, %s"
                         % (N, tuple(post_rots.shape), tuple(post_trans.shape)))
    return torch.cat([rots.inverse().reshape(N, 9), trans, intrins.reshape(N, 9), post_rots[:, :2, :2].reshape(N, 4),
                      post_trans[:, :2], torch.zeros(N, 1)], 1).contiguous()


def points_to_depth_maps(points, table, size, out=None):
    """fp32 ``[N,H,W]`` depth maps of ``points`` (device fp32 ``[P,C>=3]``, x y z first; made contiguous when it is not) for the cameras
    of ``table`` (device fp32 ``[N,28]``, ``camera_table``), ``size = (H, W)``.  Runs on the current stream: a zero fill and one launch,
    no host read; capturable into a graph with no parallel branches.  ``out``: written in place (entirely) when given."""
    points, table = device_points(points), device_tensor("table", table, torch.float32, CAM_FLOATS)
    if table.shape[0] < 1:
        raise ValueError("table must be [N >= 1, %d], got %s" % (CAM_FLOATS, tuple(table.shape)))
    if table.device != points.device:
        raise CooccError("points on %s, table on %s" % (points.device, table.device))
    H, W = int(size[0]), int(size[1])
    if H < 1 or W < 1:
        raise ValueError("size must be (H >= 1, W >= 1), got %s" % ((H, W),))
    N = table.shape[0]
    if out is None:
        out = torch.empty((N, H, W), dtype=torch.float32, device=points.device)
    elif tuple(out.shape) != (N, H, W):
        raise ValueError("out must be [%d, %d, %d], got %s" % (N, H, W, tuple(out.shape)))
    _lib.call("coocc_points_to_depth_maps", ptr(points, torch.float32), points.shape[0], points.shape[1], ptr(table, torch.float32), N, H, W,
              ptr(out, torch.float32))
    return out


# ------------------------------------------------------------------ the plan: per-camera parameters and tables, resident on the device
class ResizePlan:
    """What ``coocc_frames_to_imgs`` needs beside the frames: per camera ``resize_dims`` (newW, newH), ``crop`` (x0, y0, x1, y1) and
    ``flip``, and the two coefficient tables.  ``cams``: one ``(resize_dims, crop, flip)`` per camera; the cameras of one call may
    differ (training draws per camera), the output size ``out_size = (fH, fW)`` is common and every crop box has it.

    Tables are computed once per distinct (in size, out size) (``pillow_coeffs`` caches them) and stored once per plan.  ``resident``
    uploads header and tables with ONE asynchronous copy from pinned memory and keeps them on the device: a fixed rig in eval mode
    uploads nothing per sample."""

    def __init__(self, Hs, Ws, cams, out_size, device=None):
        self.Hs, self.Ws = int(Hs), int(Ws)
        self.fH, self.fW = int(out_size[0]), int(out_size[1])
        self.cams = [((int(d[0]), int(d[1])), tuple(int(v) for v in c), bool(f)) for d, c, f in cams]
        self.N = len(self.cams)
        if self.N < 1:
            raise ValueError("ResizePlan: no cameras")
        header = np.zeros((self.N, CAM_INTS), np.int32)
        chunks, offsets, at = [], {}, 0

        def table(in_size, out_size_):
            nonlocal at
            if in_size == out_size_:
                return -1, 0
            ratio = float(in_size) / out_size_
            k = tap_count(in_size, out_size_)
            if k > MAX_TAPS:
                raise ValueError("ResizePlan: downscale ratio %d / %d = %.3f needs %d taps; the kernel takes ratios up to %d (%d taps)"
                                 % (in_size, out_size_, ratio, k, MAX_RATIO, MAX_TAPS))
            key = (in_size, out_size_)
            if key not in offsets:
                bounds, taps = pillow_coeffs(in_size, out_size_)
                offsets[key] = at
                chunks.extend([bounds.reshape(-1), taps.reshape(-1)])
                at += bounds.size + taps.size
            return offsets[key], k

        for i, ((newW, newH), crop, flip) in enumerate(self.cams):
            if newW < 1 or newH < 1:
                raise ValueError("ResizePlan: camera %d resize_dims %s" % (i, (newW, newH)))
            if crop[2] - crop[0] != self.fW or crop[3] - crop[1] != self.fH:
                raise ValueError("ResizePlan: camera %d crop %s is not the common output size %d x %d" % (i, crop, self.fH, self.fW))
            htab, hk = table(self.Ws, newW)
            vtab, vk = table(self.Hs, newH)
            header[i, :9] = (newW, newH, crop[0], crop[1], int(flip), htab, hk, vtab, vk)
        self.header = header
        self.table_ints = at
        self.host = np.concatenate([header.reshape(-1)] + chunks + [np.zeros(4, np.int32)])          # never an empty table buffer
        self._dev = {}
        if device is not None:
            self.resident(device)

    def key(self):
        return (self.Hs, self.Ws, self.fH, self.fW, tuple(self.cams))

    def resident(self, device):
        """(params, tables, pinned host copy) on ``device``; the first call per device uploads, on the current stream."""
        device = torch.device(device)
        require_gpu(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        got = self._dev.get(device)
        if got is None:
            dev, pinned = pinned_upload(torch.from_numpy(self.host), device)
            n = self.N * CAM_INTS
            got = self._dev[device] = (dev[:n], dev[n:], pinned)
        return got


def _check_frames(frames):
    """-> (list of tensors or one 4-D tensor, N, Hs, Ws); ValueError for what is not uint8 [.., Hs, Ws, 3] of one size."""
    if isinstance(frames, torch.Tensor):
        if frames.dtype != torch.uint8:
            raise ValueError("frames must be uint8, got %s" % frames.dtype)
        if frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError("frames must be [N, Hs, Ws, 3], got %s" % (tuple(frames.shape),))
        return frames, frames.shape[0], frames.shape[1], frames.shape[2]
    frames = list(frames)
    if not frames:
        raise ValueError("no frames")
    for f in frames:
        if not isinstance(f, torch.Tensor):
            raise ValueError("frames must be uint8 tensors, got %s" % type(f).__name__)
        if f.dtype != torch.uint8:
            raise ValueError("frames must be uint8, got %s" % f.dtype)
        if f.dim() != 3 or f.shape[-1] != 3:
            raise ValueError("a frame must be [Hs, Ws, 3], got %s" % (tuple(f.shape),))
        if f.shape != frames[0].shape:
            raise ValueError("frames of mixed sizes: %s and %s" % (tuple(frames[0].shape), tuple(f.shape)))
    return frames, len(frames), frames[0].shape[0], frames[0].shape[1]


def frames_to_imgs(frames, plan, out=None, canvas=None):
    """``imgs`` fp32 [N,3,fH,fW] from ``frames``: uint8 [N,Hs,Ws,3] on the device, or a list of N device tensors [Hs,Ws,3] of one size
    (their addresses then travel in one small asynchronous copy).  Runs on the current stream; one launch when the plan's tables are
    resident; capturable into a graph with no parallel branches.  ``out``: written in place when given (a serving slot's static
    tensor).  ``canvas``: optional uint8 [N,fH,fW,3] that receives the bytes ``imgs`` was divided from."""
    frames, N, Hs, Ws = _check_frames(frames)
    if N != plan.N:
        raise ValueError("%d frames for a plan of %d cameras" % (N, plan.N))
    if (Hs, Ws) != (plan.Hs, plan.Ws):
        raise ValueError("frames are %d x %d, the plan was made for %d x %d" % (Hs, Ws, plan.Hs, plan.Ws))
    first = frames if isinstance(frames, torch.Tensor) else frames[0]
    require_gpu(first)
    device = first.device
    params, tables, pinned = plan.resident(device)
    if out is None:
        out = torch.empty((N, 3, plan.fH, plan.fW), dtype=torch.float32, device=device)
    elif tuple(out.shape) != (N, 3, plan.fH, plan.fW):
        raise ValueError("out must be [%d, 3, %d, %d], got %s" % (N, plan.fH, plan.fW, tuple(out.shape)))
    if canvas is not None and tuple(canvas.shape) != (N, plan.fH, plan.fW, 3):
        raise ValueError("canvas must be [%d, %d, %d, 3], got %s" % (N, plan.fH, plan.fW, tuple(canvas.shape)))
    if isinstance(frames, torch.Tensor):
        fptr, pptr, keep = ptr(frames, torch.uint8), ptr(None), None
    else:
        for f in frames:
            ptr(f, torch.uint8)                                  # device, dtype, contiguity
            if f.device != device:
                raise CooccError("frames on different devices: %s and %s" % (device, f.device))
        keep = pinned_upload(torch.tensor([f.data_ptr() for f in frames], dtype=torch.int64), device)[0]
        fptr, pptr = ptr(None), ptr(keep)
    _lib.call("coocc_frames_to_imgs", fptr, pptr, N, Hs, Ws, ptr(params, torch.int32), ctypes.c_void_p(pinned.data_ptr()),
              ptr(tables, torch.int32), plan.table_ints, plan.fH, plan.fW, ptr(out, torch.float32), ptr(canvas, torch.uint8))
    return out


# ------------------------------------------------------------------ the loader
class LoadMultiViewFrames:
    """The reference's LoadMultiViewImageFromFiles_OccFormer on decoded frames: ``__call__`` returns its 12-tuple with every tensor on
    ``device``.  Call it in the main process (it opens the GPU), on frames the DataLoader workers decoded.

    ``data_config``: the config's dict (``input_size``, ``cams``, ``Ncams``, ``resize``, ``crop_h``, ``flip``, ``rot``,
    ``resize_test``).  ``rng``: where training draws come from, ``np.random`` as in the reference."""

    PLAN_CACHE = 32

    def __init__(self, data_config, is_train=False, device="cuda", rng=np.random):
        self.data_config, self.is_train, self.device, self.rng = data_config, is_train, torch.device(device), rng
        self._plans = collections.OrderedDict()
        self._stage, self._small_stage = HostStage(self.device, threaded_fill=True), HostStage(self.device)          # frames | matrices
        self._point_stage = None

    def choose_cams(self):
        return choose_cams(self.data_config, self.is_train, self.rng)

    def _plan(self, Hs, Ws, cams):
        fH, fW = self.data_config['input_size']
        key = (Hs, Ws, fH, fW, tuple(cams))
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = ResizePlan(Hs, Ws, cams, (fH, fW), device=self.device)
            while len(self._plans) > self.PLAN_CACHE:
                self._plans.popitem(last=False)
        else:
            self._plans.move_to_end(key)
        return plan

    def _upload(self, frames):
        """Host frames (numpy arrays or CPU tensors, uint8 [Hs,Ws,3]) -> one device tensor [N,Hs,Ws,3]: the bytes go back to back
        through one pinned staging buffer and one asynchronous copy (a ``HostStage`` group)."""
        ts = [torch.from_numpy(np.ascontiguousarray(f)) if isinstance(f, np.ndarray) else f for f in frames]
        ts, N, Hs, Ws = _check_frames(ts)
        if all(t.is_cuda for t in ts):
            return ts
        return self._stage([tuple(t.numpy() for t in ts)])[0].view(N, Hs, Ws, 3)

    def __call__(self, frames, cam_infos, lidar2cam_dic, flip=None, scale=None, points=None):
        """``frames``: the decoded frames of the chosen cameras in the order of ``cam_names`` (a sequence, a [N,Hs,Ws,3] tensor, or a
        dict by camera name), uint8 with the channel order of the decoder -- channel k of ``imgs`` is byte k.  ``cam_infos``: the
        sample's ``['curr']['cams']`` dict; ``lidar2cam_dic``: 4 x 4 per camera name.  Returns ``(img_inputs, extras)``;
        ``denorm_imgs`` (index 8) has the values of ``imgs`` and SHARES its storage.

        ``points``: the cloud (key frame, or the merged sweeps), fp32 [P,C>=3] (a device tensor, or a numpy array / CPU tensor that is uploaded).  With it
        ``gt_depths`` (index 6) is the [N,fH,fW] LiDAR depth maps of the reference's CreateDepthFromLiDAR, made on the device
        (``depth_maps``); the camera table rides in the one small upload and is ``extras['depth_table']``.  Without it
        the slot holds the reference loader's [N,1] zeros."""
        cam_names = self.choose_cams()
        if isinstance(frames, dict):
            frames = [frames[c] for c in cam_names]
        n_frames = frames.shape[0] if isinstance(frames, torch.Tensor) and frames.dim() == 4 else len(frames)
        if n_frames != len(cam_names):
            raise ValueError("%d frames for the %d cameras %s" % (n_frames, len(cam_names), list(cam_names)))
        require_calibration(cam_names, cam_infos, lidar2cam_dic)
        if isinstance(frames, torch.Tensor):
            dev_frames = _check_frames(frames)[0]
            if not dev_frames.is_cuda:
                dev_frames = self._upload(list(frames))
        else:
            dev_frames = self._upload(frames)
        first = dev_frames if isinstance(dev_frames, torch.Tensor) else dev_frames[0]
        Hs, Ws = int(first.shape[-3]), int(first.shape[-2])
        cams, drawn, cols = [], [], collections.defaultdict(list)
        for name in cam_names:
            cal = calibration(cam_infos[name], lidar2cam_dic[name])
            resize, resize_dims, crop, flip, rotate = sample_augmentation(self.data_config, Hs, Ws, self.is_train, flip, scale, self.rng)
            if rotate != 0:
                raise NotImplementedError("rotate = %r: every coocc_nusc config has 'rot': (0, 0), and Pillow's nearest-neighbour affine "
                                          "(Image.rotate) is not restated" % (rotate,))
            post_rot, post_tran = post_transform(resize, crop, flip, rotate)
            cams.append((resize_dims, crop, bool(flip)))
            drawn.append(dict(resize=resize, resize_dims=resize_dims, crop=crop, flip=flip, rotate=rotate))
            for k, v in (("rots", cal["rot"]), ("trans", cal["tran"]), ("intrins", cal["intrin"]), ("post_rots", post_rot),
                         ("post_trans", post_tran), ("gt_depths", torch.zeros(1)), ("sensor2sensors", cal["sensor2lidar"]),
                         ("intrin_nerf", intrin_nerf(cam_infos[name]['cam_intrinsic'], resize, crop)), ("c2ws", cal["cam2world"])):
                cols[k].append(v)
        plan = self._plan(Hs, Ws, cams)
        N = len(cams)
        canvas = torch.empty((N, plan.fH, plan.fW, 3), dtype=torch.uint8, device=self.device)
        imgs = frames_to_imgs(dev_frames, plan, canvas=canvas)
        # the small tensors: stacked on the host, one upload, views of it
        stacked = {k: torch.stack(v) for k, v in cols.items()}
        if points is not None:
            stacked["depth_table"] = camera_table(*[stacked[k] for k in ("rots", "trans", "intrins", "post_rots", "post_trans")])
        m = self._small_stage.named(stacked)
        extras = dict(canvas=canvas, cam_names=cam_names, params=drawn, plan=plan)
        gt_depths = m["gt_depths"]
        if points is not None:
            if self._point_stage is None:
                self._point_stage = PointStage(self.device)
            gt_depths = points_to_depth_maps(self._point_stage(points), m["depth_table"], (plan.fH, plan.fW))
            extras["depth_table"] = m["depth_table"]
        img_inputs = (imgs, m["rots"], m["trans"], m["intrins"], m["post_rots"], m["post_trans"], gt_depths, m["sensor2sensors"],
                      imgs, m["intrin_nerf"], m["c2ws"], imgs.shape[-2:])
        return img_inputs, extras


def with_bda(img_inputs, bda_rot=None, aabb=None, batch=True):
    """The 14-tuple the reference's occupancy loader (P/datasets/pipelines/loading.py:129) turns the 12-tuple into: ``bda_rot``
    (identity when None) at index 6, ``aabb`` at index 10.  ``batch=True`` adds the leading batch dimension of 1 the DataLoader's
    collate adds (the image size becomes ``(tensor([H]), tensor([W]))``): the form ``simple_test(img=...)``, ``serving_frame`` and
    ``apis.pipelined_test`` read (``img[1:7]``)."""
    (imgs, rots, trans, intrins, post_rots, post_trans, gt_depths, sensor2sensors, denorm_imgs, intrin_nerf_, c2ws, size) = img_inputs
    if bda_rot is None:
        bda_rot = torch.eye(3, device=imgs.device).float()
    out = (imgs, rots, trans, intrins, post_rots, post_trans, bda_rot, gt_depths, sensor2sensors, denorm_imgs, aabb, intrin_nerf_, c2ws,
           size)
    if not batch:
        return out
    b = lambda t: t[None] if isinstance(t, torch.Tensor) else t
    return tuple(b(t) for t in out[:13]) + ((torch.tensor([int(size[0])]), torch.tensor([int(size[1])])),)
