"""LiDAR depth maps from the raw point cloud.

The reference's CreateDepthFromLiDAR (P/datasets/pipelines/lidar2depth.py) projects the cloud (key frame, or the merged sweeps) into every camera with
broadcast fp32 matmuls on the CPU, sorts per camera and fills ``[N,fH,fW]`` maps with an indexed assignment; the maps then travel to
the device (34 MB at 6 x 896 x 1600).  Here the cloud goes up (0.4 - 0.7 MB) and ONE kernel (csrc/depth_maps.hip) writes the maps: the
reference's fp32 operations in the reference's order, so a point lands in the pixel it lands in on the CPU.

Where several valid points round to one pixel the reference is not defined (an indexed assignment with repeated indices has no
guaranteed order); its sort shows the intent.  **A pixel holds the minimum depth over the valid points that round to it, 0 where
there is none.**

mmdet ``PIPELINES`` run in DataLoader worker processes, which must not open the GPU: ``CreateDepthFromLiDAR`` is called in the main
process, as ``image_inputs.LoadMultiViewFrames`` is.
"""
import numpy as np
import torch

from . import _lib
from . import image_inputs as II
from ._lib import CooccError, ptr

CAM_FLOATS = 28              # csrc/depth_maps.hip DM_CAM_FLOATS: inv_rot[9] tran[3] intrin[9] post_rot 2x2 [4] post_tran[2] pad


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
    for name, t in (("points", points), ("table", table)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be a tensor, got %s" % (name, type(t).__name__))
        if not t.is_cuda:
            raise CooccError("co_occ_amd ops run on the GPU only; got a %s tensor (no CPU fallback)" % t.device)
        if t.dtype != torch.float32:
            raise ValueError("%s must be float32, got %s" % (name, t.dtype))
    if points.dim() != 2 or points.shape[1] < 3:
        raise ValueError("points must be [P, C >= 3], got %s" % (tuple(points.shape),))
    if table.dim() != 2 or table.shape[1] != CAM_FLOATS or table.shape[0] < 1:
        raise ValueError("table must be [N, %d], got %s" % (CAM_FLOATS, tuple(table.shape)))
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
    points, table = points.contiguous(), table.contiguous()
    _lib.call("coocc_points_to_depth_maps", ptr(points, torch.float32), points.shape[0], points.shape[1], ptr(table, torch.float32), N, H, W,
              ptr(out, torch.float32))
    return out


class HostStage:
    """Several host arrays (numpy, contiguous or made so, any dtype) -> the device through ONE pinned staging buffer and one
    asynchronous copy: they are laid into the buffer at 256-byte offsets and the device tensors returned are views of that one
    upload (uint16 arrays come back as int16 views of the same bits: torch has no uint16 views).  The buffer grows to the largest
    sample seen and is reused once the previous copy has read it.  ``last_bytes``: the bytes of the last upload.

    An entry of ``arrays`` may be a tuple of arrays of one dtype: they are laid BACK TO BACK, with no padding between them, and come
    back as one flat device tensor (``sweeps.LoadPointsFromMultiSweeps``: the raw clouds as one buffer of rows)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._stage, self._done, self.last_bytes = None, None, 0

    def __call__(self, arrays):
        if self.device.type != "cuda":
            raise CooccError("co_occ_amd ops run on the GPU only; got device %s (no CPU fallback)" % self.device)
        groups = [[np.ascontiguousarray(p) for p in a] if isinstance(a, tuple) else None for a in arrays]
        arrays = [np.ascontiguousarray(a) if g is None else np.empty(sum(p.size for p in g), g[0].dtype if g else np.uint8)
                  for a, g in zip(arrays, groups)]          # a group's stand-in is read for its size, dtype and shape only
        offs, at = [], 0
        for a in arrays:
            offs.append(at)
            at += (a.nbytes + 255) & ~255
        self.last_bytes = at
        dtypes = [torch.int16 if a.dtype == np.uint16 else torch.from_numpy(np.empty(0, a.dtype)).dtype for a in arrays]
        if at == 0:
            return [torch.empty(a.shape, dtype=dt, device=self.device) for a, dt in zip(arrays, dtypes)]
        if self._stage is None or self._stage.numel() < at:
            self._stage = torch.empty(at, dtype=torch.uint8).pin_memory()
        elif self._done is not None:
            self._done.synchronize()                             # the previous sample's copy has read the buffer
        host = self._stage.numpy()
        for a, g, o in zip(arrays, groups, offs):
            for p in ([a] if g is None else g):
                host[o:o + p.nbytes] = p.reshape(-1).view(np.uint8)
                o += p.nbytes
        dev = self._stage[:at].to(self.device, non_blocking=True)
        self._done = torch.cuda.Event()
        self._done.record()
        return [dev[o:o + a.nbytes].view(dt).view(a.shape) for a, o, dt in zip(arrays, offs, dtypes)]


class PointStage:
    """Host points (a numpy array or a CPU tensor, fp32 ``[P,C]``) -> the device through one pinned staging buffer and one asynchronous
    copy, as the loader uploads frames; device points pass through.  The buffer grows to the largest cloud seen and is reused once the
    previous copy has read it (``HostStage`` with one array)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._host = HostStage(device)

    def __call__(self, points):
        if isinstance(points, np.ndarray):
            points = torch.from_numpy(np.ascontiguousarray(points))
        if not isinstance(points, torch.Tensor):
            raise ValueError("points must be a tensor or a numpy array, got %s" % type(points).__name__)
        if points.dtype != torch.float32:
            raise ValueError("points must be float32, got %s" % points.dtype)
        if points.dim() != 2 or points.shape[1] < 3:
            raise ValueError("points must be [P, C >= 3], got %s" % (tuple(points.shape),))
        if points.is_cuda:
            return points
        if self.device.type != "cuda":
            raise CooccError("co_occ_amd ops run on the GPU only; got device %s (no CPU fallback)" % self.device)
        if points.numel() == 0:
            return torch.empty(tuple(points.shape), dtype=torch.float32, device=self.device)
        return self._host([points.detach().contiguous().numpy()])[0]


def lidar_gt_depths(nine, bda_rot=None, batch=True):
    """What the reference's occupancy loader (P/datasets/pipelines/loading.py:130-132) turns the LiDAR-only 9-tuple into:
    ``(rots, trans, intrins, post_rots, post_trans, bda_rot, gt_depths, size)`` -- ``bda_rot`` the identity when None.  ``batch=True``
    adds the leading batch dimension of 1 the DataLoader's collate adds (the size becomes ``(tensor([H]), tensor([W]))``): the form
    ``forward_train(gt_depths=...)`` reads (``get_frustum`` on its first six and last element, the map at ``DEPTH_GT_INDEX``)."""
    imgs, rots, trans, intrins, post_rots, post_trans, sensor2sensors, gt_depths, size = nine
    if bda_rot is None:
        bda_rot = torch.eye(3, device=rots.device).float()
    out = (rots, trans, intrins, post_rots, post_trans, bda_rot, gt_depths)
    if not batch:
        return out + (size,)
    return tuple(t[None] for t in out) + ((torch.tensor([int(size[0])]), torch.tensor([int(size[1])])),)


class CreateDepthFromLiDAR:
    """The reference's CreateDepthFromLiDAR on the device, in its two forms.  Call it in the main process (it opens the GPU).

    ``data_config``: the config's dict; only the LiDAR-only form reads it (``input_size``, ``cams``, ``Ncams``, ``resize``, ``crop_h``,
    ``flip``, ``rot``, ``resize_test``).  ``rng``: where its training draws come from, ``np.random`` as in the reference."""

    def __init__(self, data_config=None, is_train=False, device="cuda", rng=np.random):
        self.data_config, self.is_train, self.device, self.rng = data_config, is_train, torch.device(device), rng
        self._points = PointStage(self.device)

    def _table(self, host_table):
        return (host_table.pin_memory() if self.device.type == "cuda" else host_table).to(self.device, non_blocking=True)

    def __call__(self, points, img_inputs):
        """The camera form (lidar2depth.py:57-88): ``img_inputs`` is the loader's 12-tuple; returns it with element 6 replaced by the
        ``[N,fH,fW]`` maps of ``points`` (fp32 ``[P,C>=3]``: a device tensor, or a numpy array / CPU tensor that is uploaded).  The five
        small matrices may live on the device: they are brought to the host once, for the table."""
        if len(img_inputs) != 12:
            raise ValueError("img_inputs must be the loader's 12-tuple, got %d elements" % len(img_inputs))
        imgs, small = img_inputs[0], list(img_inputs[1:6])
        if any(t.is_cuda for t in small):
            flat = torch.cat([t.reshape(-1).float() for t in small]).cpu()          # one read
            at, host = 0, []
            for t in small:
                host.append(flat[at:at + t.numel()].view(t.shape))
                at += t.numel()
            small = host
        table = self._table(camera_table(*small))
        maps = points_to_depth_maps(self._points(points), table, tuple(imgs.shape[-2:]))
        return tuple(img_inputs[:6]) + (maps,) + tuple(img_inputs[7:])

    def choose_cams(self):
        cfg = self.data_config
        if self.is_train and cfg['Ncams'] < len(cfg['cams']):
            return self.rng.choice(cfg['cams'], cfg['Ncams'], replace=False)
        return cfg['cams']

    def lidar_only_matrices(self, cam_infos, lidar2cam_dic):
        """The host half of ``lidar_only`` (lidar2depth.py:91-149): ``(dict of stacked CPU fp32 tensors rots, trans, intrins, post_rots,
        post_trans, sensor2sensors, (fH, fW))`` with the reference's float32 torch operations in its order.  Opens no GPU."""
        if self.data_config is None:
            raise ValueError("CreateDepthFromLiDAR.lidar_only needs data_config")
        fH, fW = self.data_config['input_size']
        cam_names = self.choose_cams()
        missing = [c for c in cam_names if c not in cam_infos or c not in lidar2cam_dic]
        if missing:
            raise ValueError("no calibration for cameras %s" % missing)
        cols = dict(rots=[], trans=[], intrins=[], post_rots=[], post_trans=[], sensor2sensors=[])
        for name in cam_names:
            cal = II.calibration(cam_infos[name], lidar2cam_dic[name])
            resize, _, crop, flip, rotate = II.sample_augmentation(self.data_config, fH, fW, self.is_train, None, None, self.rng)
            post_rot, post_tran = II.post_transform(resize, crop, flip, rotate)
            for k, v in (("rots", cal["rot"]), ("trans", cal["tran"]), ("intrins", cal["intrin"]), ("post_rots", post_rot),
                         ("post_trans", post_tran), ("sensor2sensors", cal["sensor2lidar"])):
                cols[k].append(v)
        return {k: torch.stack(v) for k, v in cols.items()}, (crop[3] - crop[1], crop[2] - crop[0])

    def lidar_only(self, points, cam_infos, lidar2cam_dic):
        """The no-image form (lidar2depth.py:90-178), which coocc_lidar.py trains with: calibration and ``post_rot`` / ``post_tran``
        for a blank image of ``data_config['input_size']`` (so ``H, W`` of the augmentation are the input size itself), then the maps.
        Returns the reference's 9-tuple ``(imgs, rots, trans, intrins, post_rots, post_trans, sensor2sensors, gt_depths, size)`` with
        every tensor on the device; ``imgs`` is zeros ``[N,fH,fW]``.  ``lidar_gt_depths`` makes the tuple ``forward_train`` reads."""
        stacked, (fH, fW) = self.lidar_only_matrices(cam_infos, lidar2cam_dic)
        stacked["table"] = camera_table(*[stacked[k] for k in ("rots", "trans", "intrins", "post_rots", "post_trans")])
        flat = self._table(torch.cat([t.reshape(-1) for t in stacked.values()]))          # one upload, views of it
        m, at = {}, 0
        for k, t in stacked.items():
            m[k] = flat[at:at + t.numel()].view(t.shape)
            at += t.numel()
        imgs = torch.zeros((stacked["rots"].shape[0], fH, fW), dtype=torch.float32, device=self.device)
        maps = points_to_depth_maps(self._points(points), m["table"], (fH, fW))
        return (imgs, m["rots"], m["trans"], m["intrins"], m["post_rots"], m["post_trans"], m["sensor2sensors"], maps, imgs.shape[-2:])
