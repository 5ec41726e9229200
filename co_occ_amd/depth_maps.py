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

from . import image_inputs as II
from .image_inputs import CAM_FLOATS, camera_table, points_to_depth_maps          # the op itself sits below both loaders
from .staging import HostStage, PointStage, pinned_upload


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
        self._points, self._small_stage = PointStage(self.device), HostStage(self.device)

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
        table = pinned_upload(camera_table(*small), self.device)[0]
        maps = points_to_depth_maps(self._points(points), table, tuple(imgs.shape[-2:]))
        return tuple(img_inputs[:6]) + (maps,) + tuple(img_inputs[7:])

    def choose_cams(self):
        return II.choose_cams(self.data_config, self.is_train, self.rng)

    def lidar_only_matrices(self, cam_infos, lidar2cam_dic):
        """The host half of ``lidar_only`` (lidar2depth.py:91-149): ``(dict of stacked CPU fp32 tensors rots, trans, intrins, post_rots,
        post_trans, sensor2sensors, (fH, fW))`` with the reference's float32 torch operations in its order.  Opens no GPU."""
        if self.data_config is None:
            raise ValueError("CreateDepthFromLiDAR.lidar_only needs data_config")
        fH, fW = self.data_config['input_size']
        cam_names = self.choose_cams()
        II.require_calibration(cam_names, cam_infos, lidar2cam_dic)
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
        m = self._small_stage.named(stacked)          # one upload, views of it
        imgs = torch.zeros((stacked["rots"].shape[0], fH, fW), dtype=torch.float32, device=self.device)
        maps = points_to_depth_maps(self._points(points), m["table"], (fH, fW))
        return (imgs, m["rots"], m["trans"], m["intrins"], m["post_rots"], m["post_trans"], m["sensor2sensors"], maps, imgs.shape[-2:])
