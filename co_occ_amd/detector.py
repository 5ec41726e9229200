"""``COOCC_Ray`` / ``COOCC_Ray_L`` -- the detector surface of P/coocc/detectors/coocc_ray.py (and coocc_ray_lidar.py)
with the reference's call signatures, so that an unchanged ``tools/test.py`` / ``tools/train.py`` run reaches the HIP
path through ``forward(return_loss=...)`` (M/models/detectors/base.py:46-58):

    extract_feat:  [image encoder -> DepthNet]* -> fused lift (x) splat -> | occ_fuser (BiFuser_N)
                   [LiDAR points] -> voxelise -> VFE -> sparse encoder  -> |
    -> semantic_encoder (CustomResNet3D) -> semantic_neck (FPN3D) -> pts_bbox_head (OccHead)
    -> inline volume-render block (sigma_head / rgb_head) -> metrics / losses

Child modules are built from the same config dicts through the registries (coocc_ray.py:80-83, bevdepth.py:21-34) and
keep the reference attribute names, so a reference checkpoint's ``occ_fuser.* / semantic_encoder.* / semantic_neck.* /
pts_bbox_head.* / sigma_head.* / rgb_head.*`` entries load unchanged.

[*] The 2D image encoder (``img_backbone`` / ``img_neck``: mmdet ResNet + SECONDFPN) and DepthNet (DCN, ASPP) are
UPSTREAM of the hot path (out of scope) and are NOT re-implemented: they are built through the real
mmdet / mmdet3d registries when those packages are importable, may be injected as ``nn.Module`` instances, and
otherwise construction fails (``external_encoders=True`` defers the failure to the first call that needs them, for
callers that feed ``precomputed=`` features or attach the encoders afterwards).  Opt-in exceptions: ``hip_image_encoder=True``
builds ResNet / SECONDFPN config dicts from ``image_encoder`` (HIP engine; ``train_image_encoder=True`` also trains them there under
``train()``), ``depth_net='hip'`` on the view
transformer builds ``depth_net.DepthNet``.
"""
import numpy as np
import torch
from torch import nn

from . import registry
from .core import to_rows
from .registry import DETECTORS
from .render import MLP, render_block, render_losses
from .view_transformer import get_frustum


def _build_upstream(kind, cfg, external, hip_image=False):
    """``img_backbone`` / ``img_neck`` / ``pts_backbone`` / ``pts_neck``: modules upstream of the hot path.  Resolution
    order: an injected nn.Module -> (``hip_image``: the image encoder's own registries, for a config dict of type ResNet /
    SECONDFPN) -> our registries (a type we do implement) -> the real mmdet3d builder -> error."""
    if cfg is None or isinstance(cfg, nn.Module):
        return cfg
    if hip_image:
        from . import image_encoder
        mine = {"backbone": (image_encoder.IMAGE_BACKBONES, "ResNet"), "neck": (image_encoder.IMAGE_NECKS, "SECONDFPN")}[kind]
        if cfg.get("type") == mine[1]:
            return mine[0].build(cfg)
    ours = {"backbone": registry.BACKBONES, "neck": registry.NECKS}[kind]
    if cfg.get("type") in ours:
        return ours.build(cfg)
    try:
        from mmdet3d.models import builder as m3b
    except Exception as e:
        if external:
            return None
        raise ImportError("COOCC_Ray: config entry %s=%r is upstream of the MI355X hot path and is built through mmdet3d's "
                          "registries, which are not importable here (%s).  Install mmdet/mmdet3d, pass the module "
                          "instance instead of the config, or build with external_encoders=True and feed "
                          "precomputed= features." % (kind, cfg.get("type"), e))
    return getattr(m3b, "build_" + kind)(cfg)


def _no_detector():
    return None


class _FusedReaders:
    """The layers that read the fuser's output: the encoder's ``input_proj`` and the first layer of each render MLP (callable
    handed to ``BiFuser_N.output_readers``; holds the detector weakly so the module tree stays a tree)."""

    def __init__(self, det):
        import weakref
        self._det = weakref.ref(det)

    def __getstate__(self):
        return {}                     # the weak reference does not pickle; COOCC_Ray.__setstate__ wires a fresh one

    def __setstate__(self, state):
        self._det = _no_detector

    def __call__(self):
        det = self._det()
        if det is None:
            return ()
        out = []
        enc = getattr(det, "semantic_encoder", None)
        if enc is not None and hasattr(enc, "_packed") and not enc.training:
            out.append(enc._packed()["proj"])
        for name in ("sigma_head", "rgb_head"):
            h = getattr(det, name, None)
            if h is not None and det.use_rendering:
                out.append(h._packed()[0])
        return out


def _drop_captured_pipeline(module, incompatible_keys):
    """``load_state_dict`` post-hook (module level, so the detector stays picklable: ``torch.save(model)``, spawn)."""
    module._pipe1 = None


@DETECTORS.register_module()
class COOCC_Ray(nn.Module):
    WITH_RGB_HEAD = True          # COOCC_Ray_L has the sigma head only (coocc_ray_lidar.py:111-112)
    # SparseEncoderHD returns the dense [B,C,Z,Y,X] tensor SECOND3D takes; the fusion detector's extract_pts_feat reads the dict
    # (x, pts_feats) of the 8x / 4x encoders (coocc_ray.py:215-234), upstream as here: only COOCC_Ray_L can run it
    TAKES_SPARSE_ENCODER_HD = False

    def __init__(self, voxel_size=None, n_voxels=None, loss_cfg=None, aabb=None, near_far_range=None,
                 N_samples=40, N_rand=4096, depth_supervise=False, use_nerf_mask=True, nerf_sample_view=3,
                 nerf_mode='volume', squeeze_scale=4, rgb_supervise=True, nerf_density=False,
                 rendering_test=False, disable_loss_depth=False, empty_idx=0, scale=16, white_bkgd=True,
                 occ_fuser=None, occ_encoder_backbone=None, occ_encoder_neck=None, density_encoder=None,
                 color_encoder=None, semantic_encoder=None, density_neck=None, color_neck=None,
                 semantic_neck=None, loss_norm=False, use_rendering=False, loss_voxel_ce_weight=1.0,
                 loss_voxel_sem_scal_weight=1.0, loss_voxel_geo_scal_weight=1.0, loss_voxel_lovasz_weight=1.0,
                 test_rendering=False, img_view_transformer=None, pts_bbox_head=None, pts_voxel_layer=None,
                 pts_voxel_encoder=None, pts_middle_encoder=None, img_backbone=None, img_neck=None,
                 pts_backbone=None, pts_neck=None, external_encoders=False, render_eval=False, sparse_encoder_hd=False,
                 train_lidar_trunk=False, train_sparse_encoder_hd=False, device_occ_losses=False, render_ssim=False, hip_image_encoder=False,
                 train_image_encoder=False, device_depth_loss=False, **kwargs):
        super().__init__()
        self.ignored_cfg_keys = sorted(kwargs)      # train_cfg / test_cfg / pretrained / img_bev_encoder_* ...
        self.external_encoders = external_encoders
        # LiDAR-side producer (coocc_ray.py:215-234; bevdepth.py builds these three from the config)
        from . import lidar
        self.pts_voxel_layer = lidar.Voxelization(**pts_voxel_layer) if pts_voxel_layer else None
        self.pts_voxel_encoder = lidar.VOXEL_ENCODERS.build(pts_voxel_encoder) if pts_voxel_encoder else None
        self.pts_middle_encoder = None
        # opt-in: a ``pts_middle_encoder`` of type SparseEncoderHD (coocc_lidar.py) is built from ``lidar_hd`` -- the HIP sparse
        # engine -- instead of staying upstream (spconv v1, which does not build on ROCm)
        self.sparse_encoder_hd = bool(sparse_encoder_hd)
        # opt-in (COOCC_Ray_L): under train() the dense LiDAR trunk SECOND3D + SECOND3DFPN runs its differentiable form
        # (lidar_trunk.run_trunk_train) and forward_train takes pts_middle_feats / raw points; detectors without that trunk ignore it
        self.train_lidar_trunk = bool(train_lidar_trunk)
        # opt-in (COOCC_Ray_L with sparse_encoder_hd=True): ``SparseEncoderHD`` runs its differentiable forward under train()
        # (lidar_hd ``train_enabled``: batch-statistics BN1d, gradients through the rule books); detectors without it ignore the key
        self.train_sparse_encoder_hd = bool(train_sparse_encoder_hd)
        if pts_middle_encoder:
            if self.sparse_encoder_hd and pts_middle_encoder.get("type") == "SparseEncoderHD":
                if not self.TAKES_SPARSE_ENCODER_HD:
                    raise NotImplementedError("%s: sparse_encoder_hd=True with pts_middle_encoder type 'SparseEncoderHD' -- that encoder "
                                              "returns the dense [B,C,Z,Y,X] volume of the LiDAR-only trunk, which this detector's "
                                              "extract_pts_feat does not take (upstream's neither); use COOCC_Ray_L" % type(self).__name__)
                from . import lidar_hd
                self.pts_middle_encoder = lidar_hd.MIDDLE_ENCODERS_HD.build(pts_middle_encoder)
                self.pts_middle_encoder.train_enabled = self.train_sparse_encoder_hd
            elif pts_middle_encoder.get("type") in lidar.MIDDLE_ENCODERS:
                # trains like upstream (sparse_lidar_enc.py:125-176; batch-statistics BN1d, gradients through the rule books:
                # co_occ_amd/lidar.py ``SparseConvFn``); ``freeze_lidar_encoder()`` restores the round-2..4 behaviour
                self.pts_middle_encoder = lidar.MIDDLE_ENCODERS.build(pts_middle_encoder)
            elif not external_encoders:
                raise NotImplementedError("COOCC_Ray: pts_middle_encoder type %r is not on the MI355X path (SparseLiDAREnc8x / "
                                          "SparseLiDAREnc4x are); pass external_encoders=True to attach it yourself"
                                          % pts_middle_encoder.get("type"))
        # opt-in: ``img_backbone`` / ``img_neck`` config dicts of type ResNet / SECONDFPN are built from ``image_encoder`` -- the HIP
        # engine -- instead of staying upstream (mmdet / mmdet3d); module instances are taken as they are.  ``train_image_encoder=True``
        # on top of it: both modules' ``train_enabled`` is set, so under train() ``image_encoder()`` trains them on the HIP engine
        # (frozen_stages / norm_eval as in mmdet); without it their train() forward raises
        self.hip_image_encoder = bool(hip_image_encoder)
        self.train_image_encoder = bool(train_image_encoder)
        self.img_backbone = _build_upstream("backbone", img_backbone, external_encoders, self.hip_image_encoder)
        self.img_neck = _build_upstream("neck", img_neck, external_encoders, self.hip_image_encoder)
        if self.hip_image_encoder:
            from . import image_encoder
            if isinstance(self.img_backbone, image_encoder.ResNet) and isinstance(self.img_neck, image_encoder.SECONDFPN):
                self.img_backbone.output_readers = image_encoder.NeckReaders(self.img_neck)
        if self.train_image_encoder:
            from . import image_encoder
            if not (self.hip_image_encoder and isinstance(self.img_backbone, image_encoder.ResNet)
                    and isinstance(self.img_neck, image_encoder.SECONDFPN)):
                raise ValueError("%s: train_image_encoder=True trains this package's ResNet / SECONDFPN; pass hip_image_encoder=True "
                                 "with img_backbone / img_neck config dicts of those types" % type(self).__name__)
            for m in (self.img_backbone, self.img_neck):
                m.train_enabled = True
                m.train(m.training)
        self.pts_backbone = _build_upstream("backbone", pts_backbone, external_encoders)
        self.pts_neck = _build_upstream("neck", pts_neck, external_encoders)
        self.empty_idx, self.scale = empty_idx, scale
        self.voxel_size, self.n_voxels, self.aabb = voxel_size, n_voxels, aabb
        self.near_far_range, self.N_samples, self.N_rand = near_far_range, N_samples, N_rand
        self.white_bkgd, self.loss_norm = white_bkgd, loss_norm
        self.loss_cfg, self.disable_loss_depth = loss_cfg, disable_loss_depth
        self.use_rendering, self.test_rendering = use_rendering, test_rendering
        self.metrics_on_device = False              # True: SC/SSC histograms stay int64 device tensors (no sync)
        # opt-in: simple_test also judges its rendered maps (coocc_ray.py:626-637: PSNR against the camera images; the squared
        # depth error of save_rendered_img.py:39-79 when gt_depths carries a map) on the device.  Upstream runs that branch
        # unconditionally, prints, and writes ./img_<v>.png; here nothing is printed or written (apis.save_rendered_panels does)
        self.render_eval = bool(render_eval)
        # opt-in, on top of ``render_eval``: the SSIM of the rendered colour maps too (the second member of save_rendered_img's
        # triple, save_rendered_img.py:22-37), on the device.  Detectors that render no colour (COOCC_Ray_L) never report it
        self.render_ssim = bool(render_ssim)
        # eval-mode ``simple_test`` runs its dense stage as ONE captured hipGraph launch (co_occ_amd.serving, one slot, results
        # identical to the eager path); COOCC_SIMPLE_TEST_GRAPH=0 or ``model.graph_simple_test = False`` keeps every launch eager
        self.graph_simple_test = __import__("os").environ.get("COOCC_SIMPLE_TEST_GRAPH", "1") != "0"
        self._pipe1 = None                          # (shape key, ServingPipeline) of simple_test
        self.graph_unavailable = None               # why simple_test fell back to the eager path, if it did
        self.img_view_transformer = registry.build_neck(img_view_transformer) if img_view_transformer else None
        self.pts_bbox_head = registry.build_head(pts_bbox_head) if pts_bbox_head else None
        # opt-in: OccHead.loss computes its eight voxel / fine-point terms and their gradient on the device (losses.occ_loss_terms_device:
        # no host read, bitwise reproducible) instead of eager torch
        self.device_occ_losses = bool(device_occ_losses)
        if self.pts_bbox_head is not None:
            self.pts_bbox_head.device_losses = self.device_occ_losses
        # opt-in: the view transformer's get_depth_loss (``loss_depth``) computes its labels, the BCE and the gradient on the device
        # (losses.depth_loss_device: no host read, bitwise reproducible) instead of eager torch.  On, it switches the module's own
        # ``device_depth_loss`` on; off, the module keeps what its config set.  Detectors without a view transformer ignore it
        self.device_depth_loss = bool(device_depth_loss)
        if self.img_view_transformer is not None and self.device_depth_loss:
            self.img_view_transformer.device_depth_loss = True
        self.occ_fuser = registry.build_fusion_layer(occ_fuser) if occ_fuser is not None else None
        self.semantic_encoder = registry.build_backbone(semantic_encoder)
        self.semantic_neck = registry.build_neck(semantic_neck)
        if use_rendering:                                      # coocc_ray.py:111-113
            self.sigma_head = MLP(input_dim=128, output_dim=1, net_depth=1, skip_layer=None)
            if self.WITH_RGB_HEAD:
                self.rgb_head = MLP(input_dim=128, output_dim=3, net_depth=3, skip_layer=None)
        if self.occ_fuser is not None and hasattr(self.occ_fuser, "output_readers"):
            self.occ_fuser.output_readers = _FusedReaders(self)
        self.register_load_state_dict_post_hook(_drop_captured_pipeline)

    def __getstate__(self):
        # torch.save(model) / multiprocessing spawn: the captured pipeline (streams, hipGraphs) belongs to this process
        state = dict(self.__dict__)
        state["_pipe1"] = None
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        if self.occ_fuser is not None and hasattr(self.occ_fuser, "output_readers"):
            self.occ_fuser.output_readers = _FusedReaders(self)

    # ------------------------------------------------------------------ encoders (coocc_ray.py:120-256)
    @property
    def with_img_neck(self):
        return self.img_neck is not None

    def image_encoder(self, img):
        """coocc_ray.py:120-135: the 2D backbone (+ neck) over the B*N views -- upstream torch modules."""
        if self.img_backbone is None:
            raise NotImplementedError("COOCC_Ray.image_encoder: no img_backbone attached (built with external_encoders=True); "
                                      "assign model.img_backbone / model.img_neck or pass precomputed= features")
        B, N, C, imH, imW = img.shape
        x = self.img_backbone(img.view(B * N, C, imH, imW))
        if self.with_img_neck:
            x = self.img_neck(x)
        if type(x) in [list, tuple]:
            x = x[0]
        x = x.view(B, N, *x.shape[1:])
        return {'x': x, 'img_feats': [x.clone()]}

    def extract_img_feat(self, img, img_metas):
        """coocc_ray.py:163-197 -> (img_voxel_feats [B,C,X,Y,Z], depth [B*N,D,fH,fW], img_feats, geom)."""
        enc = self.image_encoder(img[0])
        rots, trans, intrins, post_rots, post_trans, bda = img[1:7]
        vt = self.img_view_transformer
        mlp_input = vt.get_mlp_input(rots, trans, intrins, post_rots, post_trans, bda)
        x, depth, geom, _ = vt([enc['x'], rots, trans, intrins, post_rots, post_trans, bda, mlp_input])
        return x, depth, enc['img_feats'], geom

    def extract_pts_feat(self, pts):
        """coocc_ray.py:215-234 (batch size 1): points [N,F] (or a one-element list) -> (pts_voxel_feats [1,C,X,Y,Z],
        [sparse features])."""
        if self.pts_middle_encoder is None:
            raise NotImplementedError("COOCC_Ray was built without pts_voxel_layer / pts_voxel_encoder / pts_middle_encoder")
        if isinstance(pts, (list, tuple)):
            assert len(pts) == 1, "batch size 1 (hard-coded upstream)"
            pts = pts[0]
        voxels, coors, num_points = self.pts_voxel_layer(pts)
        feats = self.pts_voxel_encoder(voxels, num_points, coors)
        enc = self.pts_middle_encoder(feats, coors, 1)
        if self.pts_backbone is not None:                    # coocc_ray.py:223-226 (no coocc_nusc fusion config sets them)
            enc['x'] = self.pts_backbone(enc['x'])
        if self.pts_neck is not None:
            enc['x'] = self.pts_neck(enc['x'])
        return enc['x'], enc['pts_feats']

    def extract_feat(self, points, img, img_metas, search=None):
        """coocc_ray.py:237-266 -> (voxel_feats, img_feats, pts_feats, depth, geom, img_voxel_feats)."""
        img_voxel_feats = pts_voxel_feats = pts_feats = depth = img_feats = geom = None
        if img is not None:
            img_voxel_feats, depth, img_feats, geom = self.extract_img_feat(img, img_metas)
        if points is not None:
            pts_voxel_feats, pts_feats = self.extract_pts_feat(points)
        voxel_feats = self.fuse(img_voxel_feats, pts_voxel_feats, search)
        return voxel_feats, img_feats, pts_feats, depth, geom, img_voxel_feats

    def freeze_lidar_encoder(self, frozen=True):
        """Optional (fine-tuning with a fixed LiDAR branch): the sparse encoder keeps its eval-mode path (folded BN1d running
        statistics, split-f16 rule-book GEMMs) under ``train()`` and its parameters take no gradient."""
        self._lidar_frozen = bool(frozen)
        if self.pts_middle_encoder is not None:
            for prm in self.pts_middle_encoder.parameters():
                prm.requires_grad_(not frozen)
            if frozen:
                self.pts_middle_encoder.eval()
        return self

    def train(self, mode=True):
        """``nn.Module.train`` (an unchanged tools/train.py calls ``model.train()`` on the whole detector); a LiDAR encoder
        frozen with ``freeze_lidar_encoder()`` stays in eval mode."""
        super().train(mode)
        if mode:
            self._pipe1 = None          # the captured eval-mode graph holds the CURRENT weight packs; training rewrites them
        if mode and getattr(self, "_lidar_frozen", False) and getattr(self, "pts_middle_encoder", None) is not None:
            self.pts_middle_encoder.eval()
        return self

    def fuse(self, img_voxel_feats, pts_voxel_feats, search=None):
        """coocc_ray.py:252-256."""
        if self.occ_fuser is not None:
            return self.occ_fuser(img_voxel_feats, pts_voxel_feats, search=search)
        assert (img_voxel_feats is None) or (pts_voxel_feats is None)
        return img_voxel_feats if pts_voxel_feats is None else pts_voxel_feats

    def search(self, img_voxel_feats, pts_voxel_feats):
        """Index-search stage of the fuser for one sample (``BiFuser_N.search``): may be issued for sample i+1 on
        another stream / host thread while sample i runs ``forward_hot_path(..., search=...)``."""
        return self.occ_fuser.search(img_voxel_feats, pts_voxel_feats)

    def forward_hot_path(self, img_voxel_feats, pts_voxel_feats, gemo=None, img_feats=None, transform=None,
                         render=None, dense_fine=True, search=None):
        """simple_test (coocc_ray.py:520-627) minus encoders and metrics.

        img_voxel_feats / pts_voxel_feats: [1,C,X,Y,Z]; gemo: [1,N,D,fH,fW,3] (get_geometry);
        img_feats: [[1,N,512,fH,fW]]; transform: img_inputs[1:] (rots, trans, intrins, post_rots,
        post_trans, bda, ..., (H_img, W_img))."""
        voxel_feats = self.fuse(img_voxel_feats, pts_voxel_feats, search)
        return self.decode(voxel_feats, gemo, img_feats, transform, render, dense_fine)

    def decode(self, voxel_feats, gemo=None, img_feats=None, transform=None, render=None, dense_fine=True,
               depth_only=False, fine_size=None, after_encoder=None, static=False, cam_geo=None):
        """Everything after ``extract_feat`` and before the metrics (coocc_ray.py:525-627).  ``after_encoder``: callback run
        once the encoder's launches are enqueued (a serving loop with two samples in flight staggers them there).
        ``static``: no host read anywhere (the fine branch keeps its count on the device and returns capacity-sized
        tensors + ``fine_count``): the form ``co_occ_amd.graph`` captures into a hipGraph."""
        from . import core
        neck, head = self.semantic_neck, self.pts_bbox_head
        do_render = (self.use_rendering and self.test_rendering) if render is None else render
        rbranch = rendered = None
        if do_render:
            # the render block reads the fused features only: forked beside the encoder / neck / head chain (core.Fork), joined below
            rbranch = core.Fork(0, voxel_feats.t.device if isinstance(voxel_feats, core.Rows) else voxel_feats.device)
            with rbranch:
                rendered = render_block(self.sigma_head, getattr(self, "rgb_head", None), to_rows(voxel_feats), gemo, 16,
                                        depth_only=depth_only or not hasattr(self, "rgb_head"), cam_geo=cam_geo)
        ibranch = head.fork_image_branch(img_feats, transform, to_rows(voxel_feats)) if hasattr(head, "fork_image_branch") else None
        mid = self.semantic_encoder.forward_rows(voxel_feats, readers=neck.lateral_packs() if hasattr(neck, "lateral_packs") else None)
        if after_encoder is not None:
            after_encoder()
        sem = neck.forward_rows(mid, readers=head.level_readers() if hasattr(head, "level_readers") else None)
        kw = dict(image_branch=ibranch) if ibranch is not None else {}
        output = self.pts_bbox_head(voxel_feats=sem, img_feats=img_feats, transform=transform, static=static, **kw)
        res = dict(voxel_feats=voxel_feats, pred_c=output['output_voxels'][0], pred_f=None,
                   output_voxels_fine=output['output_voxels_fine'], output_coords_fine=output['output_coords_fine'])
        if output['output_voxels_fine'] is not None and dense_fine:
            cf = self.pts_bbox_head.cascade_ratio
            pc = res['pred_c']
            size = fine_size or [pc.shape[2] * cf, pc.shape[3] * cf, pc.shape[4] * cf]     # == gt_occ size (coocc_ray.py:549)
            res['pred_f'] = self.pts_bbox_head.scatter_fine(output['output_voxels_fine'][0],
                                                            output['output_coords_fine'][0], list(size),
                                                            count_dev=output.get('fine_count'))
            res['fine_count'] = output.get('fine_count')
        if do_render:
            rgbs, depths, maps = rendered
            rbranch.join(rgbs, depths, maps)
            res.update(rgbs=rgbs, depths=depths, render_maps=maps)
        return res

    def forward_train_hot_path(self, img_voxel_feats, pts_voxel_feats, gemo=None, img_feats=None, transform=None,
                               coarse_lin=None, render=True, generator=None, depth_only=False, search=None):
        """Differentiable counterpart of ``forward_hot_path``: K1-K5 run as in inference (indices are not differentiated, as
        upstream), everything after them is an autograd Function over the HIP kernels; every BatchNorm follows its own
        ``training`` flag (batch / SyncBN statistics under model.train(), folded running statistics in eval mode).
        Returns rows / tensors with ``grad_fn``: ``voxel_rows`` [V,C] (con_enc output), ``levels`` [(rows, geom)],
        ``out_voxel_rows`` [V,128], ``logit_rows`` [V,ncls], ``fine_logits`` [8n,ncls] + ``fine_xyz`` [3,8n], ``rgbs`` /
        ``depths`` of the render block.  ``coarse_lin``: int32 rows of the coarse voxels whose children the fine branch
        evaluates; default: ``OccHead.draw_fine_voxels`` -- the foreground voxels (argmax != empty), randomly thinned to
        ``fine_topk`` whole coarse voxels when there are more, as the reference does (coordinate_transform.py:17-21 permutes the
        COARSE columns and keeps the first ``topk``, each with all of its ratio^3 children).
        ``search``: a ``BiFuser_N.search`` result of THIS sample issued earlier (the indices depend on the inputs only, not on the
        weights, so a training loop may run the search of batch i+1 on a side stream under the backward pass of batch i -- 2 ms of
        dependent FPS steps off the critical path; ``bench.py --train`` does)."""
        from . import autograd as ag
        one = img_voxel_feats if img_voxel_feats is not None else pts_voxel_feats
        B, C, X, Y, Z = one.shape
        assert B == 1, "batch size 1 per GPU (coocc_ray.py:365)"
        V = X * Y * Z
        rows = lambda t: t.float().permute(0, 2, 3, 4, 1).reshape(V, t.shape[1])
        if self.occ_fuser is not None:
            sr = search
            if sr is None:
                with torch.no_grad():
                    sr = self.occ_fuser.search(img_voxel_feats.detach(), pts_voxel_feats.detach())
            self.occ_fuser.finish_bookkeeping(sr)              # the img->pts direction (or all of it) ran on another stream
            cat4 = ag.fuser_fuse_train(self.occ_fuser, rows(img_voxel_feats).contiguous(), rows(pts_voxel_feats).contiguous(), sr)
            vf, geom = ag.con_enc_train(self.occ_fuser.con_enc, cat4, (1, X, Y, Z))
        else:                                                  # coocc_ray.py:255-256: single-modality models
            assert (img_voxel_feats is None) or (pts_voxel_feats is None)
            vf, geom = rows(one).contiguous(), (1, X, Y, Z)
        levels = ag.trunk_forward_train(None, self.semantic_encoder, self.semantic_neck, vf, geom)
        head = self.pts_bbox_head
        out_rows, logit_rows = ag.occhead_coarse_train(head, levels)
        res = dict(voxel_rows=vf, levels=levels, out_voxel_rows=out_rows, logit_rows=logit_rows)
        if head.cascade_ratio != 1 and (head.sample_from_img or head.sample_from_voxel):
            if coarse_lin is None:
                coarse_lin = head.draw_fine_voxels(logit_rows.detach(), generator)
            if coarse_lin.numel():
                res["fine_logits"], res["fine_xyz"] = ag.fine_branch_train(head, out_rows, (1, X, Y, Z), coarse_lin.contiguous(),
                                                                           img_feats, transform)
        if render and self.use_rendering:
            rgb_head = None if (depth_only or not hasattr(self, "rgb_head")) else self.rgb_head
            res["rgbs"], res["depths"] = ag.render_block_train(self.sigma_head, rgb_head, vf, (X, Y, Z), gemo)
        return res

    def render_losses(self, rgbs, depths, rgb_gt, depth_gt, D):
        """coocc_ray.py:423-433."""
        return render_losses(rgbs, depths, rgb_gt, depth_gt, D)

    def _metrics_launch(self, out, gt_occ, visible_mask):
        """coocc_ray.py:539-554 on the device: SC / SSC (/ visible-only SSC) confusion matrices of pred_c and pred_f, one kernel
        per prediction on the CURRENT stream -> int64 device tensor [1 or 2, 4 + 2*C*C].  No synchronisation."""
        from .evaluation import semantic_histograms
        hc = semantic_histograms(out["pred_c"], gt_occ, visible_mask, self.empty_idx)
        hf = semantic_histograms(out["pred_f"], gt_occ, visible_mask, self.empty_idx) if out.get("pred_f") is not None else None
        return torch.stack([hc, hf]) if hf is not None else hc[None]

    def _metrics_finish(self, both, C, visible):
        """``both``: what ``_metrics_launch`` produced -- a numpy array (already on the host: the upstream dict of numpy arrays
        that ``collect_results_cpu`` pickles) or the device tensor (``metrics_on_device``)."""
        from .evaluation import split_histograms
        if torch.is_tensor(both):
            split = lambda h: split_histograms(h, C)
        else:
            split = lambda h: (h[:4].reshape(2, 2), h[4:4 + C * C].reshape(C, C), h[4 + C * C:].reshape(C, C))
        sc, ssc, occ = split(both[0])
        res = dict(SC_metric=sc, SSC_metric=ssc)
        if visible:
            res["SSC_occ_metric"] = occ
        if both.shape[0] > 1:
            sc, ssc, occ = split(both[1])
            res.update(SC_metric=sc, SSC_metric_fine=ssc)                    # coocc_ray.py:553-554 overwrites SC_metric
            if visible:
                res["SSC_occ_metric_fine"] = occ
        return res

    def _metrics(self, out, gt_occ, visible_mask):
        """coocc_ray.py:539-554: by default one device->host read of the 4 + 2*17*17 counters per prediction so the dict holds
        numpy arrays like upstream; ``metrics_on_device`` keeps int64 device tensors instead (no synchronisation)."""
        both = self._metrics_launch(out, gt_occ, visible_mask)
        if not self.metrics_on_device:
            both = both.cpu().numpy()
        return self._metrics_finish(both, out["pred_c"].shape[1], visible_mask is not None)

    # ------------------------------------------------------------------ serving (co_occ_amd.serving)
    def serving(self, example, **kw):
        """A ``ServingPipeline`` over this detector: ``submit(frame) -> Ticket`` with several frames in flight (the dense stage
        of each is one captured hipGraph launch).  ``example``: a frame dict that fixes the shapes (``serving_frame``)."""
        from .serving import ServingPipeline
        return ServingPipeline(self, example, **kw)

    def serving_frame(self, img=None, points=None, img_metas=None, precomputed=None):
        """The ``frame`` dict ``ServingPipeline.submit`` takes, from ``simple_test``'s arguments: runs what is UPSTREAM of the hot
        path (2-D image encoder + DepthNet, the LiDAR producer) eagerly and stops before Lift (x) Splat.  ``precomputed`` may
        carry ``depth`` + ``ctx`` (the lifted pair) or ``img_voxel_feats`` (already pooled), ``pts_voxel_feats``, ``img_feats``,
        ``gemo`` / ``cams``, ``transform``."""
        pc = precomputed or {}
        fr = dict(depth=pc.get("depth"), ctx=pc.get("ctx"), img_voxel_feats=pc.get("img_voxel_feats"), pts=pc.get("pts_voxel_feats"),
                  img_feats=pc.get("img_feats"), gemo=pc.get("gemo"), cams=pc.get("cams"),
                  transform=(img[1:] if img is not None else pc.get("transform")))
        if precomputed is None and img is not None:
            enc = self.image_encoder(img[0])
            rots, trans, intrins, post_rots, post_trans, bda = img[1:7]
            vt = self.img_view_transformer
            mlp_input = vt.get_mlp_input(rots, trans, intrins, post_rots, post_trans, bda)
            fr["depth"], fr["ctx"] = vt.lift([enc['x'], rots, trans, intrins, post_rots, post_trans, bda, mlp_input])
            fr["img_feats"] = enc['img_feats']
        if precomputed is None and points is not None:
            fr["pts"] = self.extract_pts_feat(points)[0]
        if fr["cams"] is None and fr["gemo"] is None and fr["transform"] is not None:
            fr["cams"] = tuple(fr["transform"][:6])
        return fr

    def _simple_test_graph(self, fr, fine_size):
        """The dense stage of one frame through a one-slot ``ServingPipeline`` (built on first use, rebuilt when the shapes
        change).  Returns the output dict, or None when this configuration / frame cannot take the captured form."""
        from . import _lib
        camera = fr["depth"] is not None or fr["img_voxel_feats"] is not None
        if self.occ_fuser is not None:
            if fr["pts"] is None or fr["img_feats"] is None or fr["transform"] is None or not camera:
                return None
        elif camera == (fr["pts"] is not None):               # single modality: the camera volume or the LiDAR volume, not both
            return None
        if fr["depth"] is not None and (fr["cams"] is None or self.img_view_transformer is None):
            return None
        do_render = bool(self.use_rendering and self.test_rendering)
        if do_render and not camera:
            return None                                       # the LiDAR-only captured stage has no render block
        one = next(fr[k] for k in ("pts", "depth", "img_voxel_feats") if fr[k] is not None)
        key = tuple((k, tuple(v.shape), v.dtype) for k, v in sorted(fr.items()) if torch.is_tensor(v)) + \
            (tuple(fr["img_feats"][0].shape) if fr["img_feats"] is not None else None, do_render, str(one.device))
        if self._pipe1 is None or self._pipe1[0] != key:
            if self.graph_unavailable is not None and self.graph_unavailable[0] == key:
                return None
            self._pipe1 = None                                # frees the old slot + graph before the new capture
            try:
                self._pipe1 = (key, self.serving(fr, slots=1, dense_streams=1, render=do_render))
            except _lib.CooccError as e:
                # the range guard (results not trustworthy) and HIP runtime / launch failures are bug reports, not fallbacks;
                # a call the library REFUSED before launching (COOCC_EINVAL / COOCC_ENOMEM: a shape the static form does not
                # take, a workspace that is too small) leaves the eager launches as the route, as before
                if not isinstance(e, _lib.CooccArgError):
                    raise
                import warnings
                why = "%s: %s" % (type(e).__name__, e)
                warnings.warn("COOCC_Ray.simple_test: the captured (hipGraph) dense stage is unavailable for this input "
                              "signature, running eager launches instead (about half the throughput); not retried for this "
                              "signature -- %s" % why)
                self.graph_unavailable = (key, why)
                return None
            except (NotImplementedError, AssertionError, RuntimeError) as e:
                import warnings
                why = "%s: %s" % (type(e).__name__, e)
                transient = isinstance(e, torch.cuda.OutOfMemoryError) or "out of memory" in str(e).lower()
                warnings.warn("COOCC_Ray.simple_test: the captured (hipGraph) dense stage is unavailable for this input "
                              "signature, running eager launches instead (about half the throughput)%s -- %s"
                              % ("" if transient else "; not retried for this signature", why))
                if not transient:                             # out-of-memory during warm-up + capture may not repeat: try again
                    self.graph_unavailable = (key, why)
                return None
        pipe = self._pipe1[1]
        X, Y, Z = pipe.grid
        cf = self.pts_bbox_head.cascade_ratio
        if fine_size is not None and self.pts_bbox_head.has_fine_branch and list(fine_size) != [X * cf, Y * cf, Z * cf]:
            return None                                       # the captured scatter writes the default fine grid
        t = pipe.submit(fr, copy=True)
        out = dict(t.result(wait=True))
        res = pipe.graphs[0].out if not t.fallback else None
        if res is not None and res.get("output_voxels_fine") is not None and out.get("fine_count") is not None:
            # capacity-sized fine outputs of the captured form -> the exact-size tensors the eager path returns
            n = int(out["fine_count"].item()) * cf ** 3
            out["output_voxels_fine"] = [res["output_voxels_fine"][0][:n].clone()]
            xyz = res["output_coords_fine"][0]                # the device-count kernels pack [3][n] at the start of the buffer
            out["output_coords_fine"] = [xyz.reshape(-1)[:3 * n].view(3, n).clone()]
        return out

    def simple_test(self, img_metas=None, img=None, gt_depths=None, points=None, rescale=False, points_occ=None,
                    gt_occ=None, visible_mask=None, precomputed=None):
        """Reference signature and result dict (coocc_ray.py:520-656).  ``img`` = img_inputs (imgs, rots, trans, intrins,
        post_rots, post_trans, bda, ...); ``points`` = [points [N,5]].  ``precomputed=dict(img_voxel_feats= | depth= + ctx=,
        pts_voxel_feats=, gemo=, img_feats=)`` (an extension) bypasses the upstream encoders.
        In eval mode the dense stage runs as one captured hipGraph launch (``graph_simple_test``; same bits as the eager
        launches, which remain the fallback for configurations / frames the captured form does not cover).  So do the models
        without a fuser -- the camera-only ``COOCC_Ray`` and ``COOCC_Ray_L`` (one ``graph.VoxelSlot`` instead of the search
        slot; ``COOCC_Ray_L`` with ``test_rendering`` keeps the eager launches: its captured stage has no render block).  One
        configuration is NOT bit-equal between the two routes: a voxel-only fine head (``sample_from_voxel=True,
        sample_from_img=False``, cascade 2).  Its captured form (csrc/fine_vox.hip) applies ``fine_mlp[0]`` before the trilinear
        interpolation, the eager form after it as the reference does; ``pred_f`` and the fine logits agree to fp32 rounding
        (tests/test_gpu_fine_vox.py judges both against float64), ``pred_c`` and the fine coordinates bit for bit.
        ``points_occ`` ([points [N,>=4]], label in column 3; ``gt_occ`` may be None, the test-submission case) adds the lidarseg
        keys of coocc_ray.py:556-560, 648-651: ``output_points`` (int64 labels 1..16 on the device), ``target_points`` and
        ``evaluation_semantic`` (16x16 int64; a device tensor under ``metrics_on_device``)."""
        fine_size = list(gt_occ.shape[1:]) if gt_occ is not None else None
        out = None
        lifted = precomputed is not None and precomputed.get("depth") is not None
        # the frame route: fused models with a view transformer, and single-modality models (no fuser: the camera-only COOCC_Ray,
        # COOCC_Ray_L) -- those only when the captured form or a lifted pair asks for it, so that with graph_simple_test off their
        # eager calls stay the launches they always were
        framed = self.img_view_transformer is not None if self.occ_fuser is not None else True
        if (self.graph_simple_test or lifted) and not self.training and framed:
            fr = self.serving_frame(img, points, img_metas, precomputed)
            out = self._simple_test_graph(fr, fine_size) if self.graph_simple_test else None
            if out is None:                                   # eager path from the frame that was just built
                if fr["img_voxel_feats"] is None and fr["depth"] is not None:
                    fr["img_voxel_feats"] = self.img_view_transformer.lift_splat(fr["depth"], fr["ctx"], cams=fr["cams"])
                gemo = fr["gemo"]
                if gemo is None and fr["cams"] is not None and self.use_rendering and self.test_rendering:
                    gemo = self.img_view_transformer.get_geometry(*fr["cams"])
                voxel_feats = self.fuse(fr["img_voxel_feats"], fr["pts"], (precomputed or {}).get("search"))
                out = self.decode(voxel_feats, gemo, fr["img_feats"], fr["transform"], fine_size=fine_size)
        elif precomputed is not None:
            voxel_feats = self.fuse(precomputed.get("img_voxel_feats"), precomputed.get("pts_voxel_feats"), precomputed.get("search"))
            img_feats, gemo = precomputed.get("img_feats"), precomputed.get("gemo")
            transform = img[1:] if img is not None else precomputed.get("transform")
            out = self.decode(voxel_feats, gemo, img_feats, transform, fine_size=fine_size)
        else:
            voxel_feats, img_feats, _, _, gemo, _ = self.extract_feat(points, img=img, img_metas=img_metas)
            transform = img[1:] if img is not None else None
            out = self.decode(voxel_feats, gemo, img_feats, transform, fine_size=fine_size)
        return self.finish_test_result(out, gt_occ, visible_mask, points_occ=points_occ, img_metas=img_metas,
                                       gt_img=self.render_gt_img(img, precomputed), gt_depths=gt_depths)

    @staticmethod
    def render_gt_img(img, precomputed=None):
        """The images the rendered maps are compared with: ``img[0][0]`` [N,3,H,W] (coocc_ray.py:627), or ``precomputed['gt_img']``
        when the image encoder was bypassed."""
        if img is not None and img[0] is not None:
            return img[0][0]
        return (precomputed or {}).get("gt_img")

    def finish_test_result(self, out, gt_occ=None, visible_mask=None, points_occ=None, img_metas=None, gt_img=None, gt_depths=None):
        """The tail of ``simple_test`` (coocc_ray.py:539-560, 629-656) on a decoded sample: the reference's result keys and,
        with ground truth, the SC / SSC confusion matrices; with ``points_occ``, the lidarseg keys; with ``render_eval`` set, rendered
        maps and ``gt_img``, the render keys ``psnr`` [N] / ``psnr_mean`` (+ ``depth_sq_err`` / ``depth_valid`` [N] when ``gt_depths``
        gives a map of the maps' size; + ``ssim`` [N] / ``ssim_mean`` with ``render_ssim`` and colour maps) -- numpy like the other
        metrics, device tensors under ``metrics_on_device``."""
        out = dict(out)
        out.update(output_voxels=out["pred_c"], target_voxels=gt_occ)
        lseg = self._lidarseg_launch(out, points_occ, img_metas) if points_occ else None
        reval = self._render_eval_launch(out, gt_img, gt_depths)
        rssim = self._render_ssim_launch(out, gt_img)
        if reval is not None:
            out.update(self._render_eval_finish(reval[0] if self.metrics_on_device else reval[0].cpu().numpy(), *reval[1:]))
        if rssim is not None:
            out.update(self._render_ssim_finish(rssim if self.metrics_on_device else rssim.cpu().numpy()))
        if gt_occ is not None:
            out.update(self._metrics(out, gt_occ, visible_mask))
        if lseg is not None:
            labels, hist = lseg
            out.update(self._lidarseg_finish(labels, hist if self.metrics_on_device else hist.cpu().numpy(), points_occ))
        if (gt_occ is not None or lseg is not None or reval is not None or rssim is not None) and not self.metrics_on_device:
            from . import core
            core.check_h2_overflow()          # the metrics were read back: the whole sample has finished on this stream
        return out

    def _render_gt_depth(self, gt_depths, depths):
        """The depth ground truth of the rendered maps, if ``gt_depths`` holds one of their size: a tensor, or the dataset's
        tuple with the map at ``DEPTH_GT_INDEX`` (as ``forward_train`` reads it); leading batch dimensions of 1 are dropped."""
        g = gt_depths
        if isinstance(g, (list, tuple)):
            i = self.DEPTH_GT_INDEX
            g = g[i] if -len(g) <= i < len(g) else None
        if not torch.is_tensor(g):
            return None
        while g.dim() > depths.dim() and g.shape[0] == 1:
            g = g[0]
        return g if g.shape == depths.shape and g.device == depths.device else None

    def _render_eval_launch(self, out, gt_img, gt_depths):
        """coocc_ray.py:626-637 on the device: the stats block of the sample's rendered maps (``coocc_render_eval_stats``) on the
        CURRENT stream -> (float64 [N,8], PSNR present, depth error present), or None when ``render_eval`` is off, nothing was
        rendered or the ground truth is missing.  The depth-only variant has no colour maps: depth keys only.  No synchronisation."""
        if not self.render_eval or out.get("depths") is None:
            return None
        rgbs, depths = out.get("rgbs"), out["depths"]
        gd = self._render_gt_depth(gt_depths, depths)
        if rgbs is None:
            gt_img = None
            if gd is None:
                return None
        elif gt_img is None:
            return None
        from .evaluation import render_eval_stats
        return render_eval_stats(rgbs, depths, gt_img, gd), rgbs is not None, gd is not None

    @staticmethod
    def _render_eval_finish(block, with_rgb, with_depth):
        """The render keys of a stats block: the host copy (numpy) or the device tensor (``metrics_on_device``)."""
        from .evaluation import render_eval_keys
        return render_eval_keys(block, with_rgb, with_depth, extrema=False)

    def _render_ssim_launch(self, out, gt_img):
        """The SSIM block of the sample's rendered colour maps (``coocc_render_eval_ssim``) on the CURRENT stream, right behind
        the stats launch -> float64 [N,8], or None unless ``render_eval`` and ``render_ssim`` are both set, colour maps were
        rendered and ``gt_img`` is there.  No synchronisation."""
        if not (self.render_eval and self.render_ssim) or out.get("rgbs") is None or gt_img is None:
            return None
        from .evaluation import render_ssim
        return render_ssim(out["rgbs"], gt_img)

    @staticmethod
    def _render_ssim_finish(block):
        """``ssim`` / ``ssim_mean`` of an SSIM block: the host copy (numpy) or the device tensor (``metrics_on_device``)."""
        from .evaluation import render_ssim_keys
        keys = render_ssim_keys(block)
        return dict(ssim=keys["ssim"], ssim_mean=keys["ssim_mean"])

    def _lidarseg_launch(self, out, points_occ, img_metas=None):
        """coocc_ray.py:556-560 on the device: the eval labels of ``forward_lidarseg`` (argmax of the softmax over classes
        1..16, + 1) and the 16x16 ``simple_evaluation_semantic`` matrix of pred_c at the points, one kernel per batch element on
        the CURRENT stream -> (int64 [N], int64 [16,16]).  No synchronisation."""
        return self.pts_bbox_head.lidarseg_labels(out["pred_c"], points_occ, img_metas)

    @staticmethod
    def _lidarseg_finish(labels, hist, points_occ):
        """The result keys of coocc_ray.py:648-651; ``hist``: the host matrix (numpy) or the device tensor (``metrics_on_device``)."""
        return dict(output_points=labels, target_points=torch.cat(list(points_occ), dim=0),
                    evaluation_semantic=hist.reshape(16, 16))

    def evaluation_semantic(self, pred, gt, eval_type, visible_mask=None):
        """coocc_ray.py:659-684 on the device (no .cpu().numpy())."""
        from .evaluation import evaluation_semantic
        return evaluation_semantic(pred, gt, eval_type, visible_mask, self.empty_idx)

    # ------------------------------------------------------------------ training (coocc_ray.py:313-518)
    def forward_train(self, points=None, img_metas=None, img_inputs=None, gt_occ=None, points_occ=None, visible_mask=None,
                      gt_depths=None, precomputed=None, generator=None, **kwargs):
        """Reference signature; returns the reference's loss dict: ``loss_depth`` (DepthNet BCE: upstream torch, or with
        ``device_depth_loss`` the HIP kernels of ``losses.depth_loss_device`` -- no host read, bitwise reproducible),
        the OccHead losses ``loss_voxel_{ce,sem_scal,geo_scal,lovasz}_{c_0,fine}`` (co_occ_amd.losses), ``loss_norm``
        rescaling, and the render regulariser ``loss_depth_render`` / ``loss_rgb`` (camera branch :358-434) or
        ``loss_depth_render`` alone through ``get_frustum`` (LiDAR-only branch :436-496).  Everything between the
        encoders and the losses is an autograd Function over the HIP kernels (``forward_train_hot_path``).  ``points_occ``
        ([points [N,>=4]], label in the last column) adds ``point_mean_iou`` (OccHead.loss, occ_head.py:333-335): a float64
        device tensor, no host read."""
        depth = None
        if precomputed is not None:
            img_voxel_feats, pts_voxel_feats = precomputed.get("img_voxel_feats"), precomputed.get("pts_voxel_feats")
            img_feats, gemo, depth = precomputed.get("img_feats"), precomputed.get("gemo"), precomputed.get("depth")
        else:
            img_voxel_feats = pts_voxel_feats = img_feats = gemo = None
            if img_inputs is not None:
                img_voxel_feats, depth, img_feats, gemo = self.extract_img_feat(img_inputs, img_metas)
            if points is not None:
                pts_voxel_feats, _ = self.extract_pts_feat(points)
        transform = img_inputs[1:] if img_inputs is not None else None
        losses = dict()
        if not self.disable_loss_depth and depth is not None:
            losses['loss_depth'] = self.img_view_transformer.get_depth_loss(img_inputs[7], depth)
        depth_only = img_feats is None
        if self.use_rendering and depth_only:                  # :436-437
            g = gt_depths
            gemo = get_frustum(g[0], g[1], g[2], g[3], g[4], g[5], g[-1], 16)
        res = self.forward_train_hot_path(img_voxel_feats, pts_voxel_feats, gemo, img_feats, transform,
                                          render=self.use_rendering, generator=generator, depth_only=depth_only)
        head = self.pts_bbox_head
        B, _, X, Y, Z = (img_voxel_feats if img_voxel_feats is not None else pts_voxel_feats).shape
        logits = res["logit_rows"].view(B, X, Y, Z, -1).permute(0, 4, 1, 2, 3)
        fine = [res["fine_logits"]] if "fine_logits" in res else None
        coords = [res["fine_xyz"]] if "fine_xyz" in res else None
        losses.update(head.loss(output_voxels=[logits], output_voxels_fine=fine, output_coords_fine=coords,
                                target_voxels=gt_occ, target_points=points_occ, img_metas=img_metas, visible_mask=visible_mask))
        if self.loss_norm:                                     # :351-354
            for k in list(losses):
                if k.startswith('loss'):
                    losses[k] = losses[k] / (losses[k].detach() + 1e-9)
        if self.use_rendering:
            D = gemo.shape[2]
            if not depth_only:                                 # :423-433
                rl = self.render_losses_train(res["rgbs"], res["depths"], img_inputs[0][0].permute(0, 2, 3, 1), img_inputs[7][0], D)
                losses.update(rl)
            else:                                              # :486-496 (gt_depths[6] there, gt_depths[-2] in coocc_ray_lidar.py)
                dg = gt_depths[self.DEPTH_GT_INDEX][0]
                rl = self.render_losses_train(None, res["depths"], None, dg, D)
                losses["loss_depth_render"] = rl["loss_depth_render"]
        return losses

    DEPTH_GT_INDEX = 6

    @staticmethod
    def render_losses_train(rgbs, depths, rgb_gt, depth_gt, D):
        from . import autograd as ag
        if rgbs is None:                                       # depth-only: the colour term does not exist
            rgbs = torch.zeros(*depths.shape, 3, device=depths.device)
            rgb_gt = rgbs
        return ag.render_losses(rgbs, depths, rgb_gt.float().contiguous(), depth_gt.float().contiguous(), D)

    def forward_test(self, img_metas=None, img_inputs=None, **kwargs):
        return self.simple_test(img_metas, img_inputs, **kwargs)

    def forward(self, return_loss=True, **kwargs):
        """M/models/detectors/base.py:46-58."""
        if return_loss:
            return self.forward_train(**kwargs)
        return self.forward_test(**kwargs)


@DETECTORS.register_module()
class COOCC_Ray_L(COOCC_Ray):
    """LiDAR-only variant (P/coocc/detectors/coocc_ray_lidar.py): same decoder and depth-only render regulariser (no
    rgb head, :111-112; depth ground truth at gt_depths[-2], :507).  Its dense trunk ``pts_backbone`` / ``pts_neck`` (SECOND3D /
    SECOND3DFPN, projects/configs/coocc_nusc/coocc_lidar.py) is built from the unchanged config through this package's
    registries and runs on the HIP engine (``lidar_trunk``).  The ``SparseEncoderHD`` middle encoder in front of it is built from
    ``lidar_hd`` (the HIP sparse engine) under ``sparse_encoder_hd=True`` -- the model then runs from a raw point cloud: eager
    voxelise -> VFE -> encoder -> trunk, then the decoder; by default it is left to the caller as before (an injected module, or
    ``external_encoders``); ``precomputed=dict(pts_middle_feats=...)`` (its dense [B,C,Z,Y,X] output) runs the trunk without it.
    ``train_lidar_trunk=True``: under ``train()`` the trunk runs ``lidar_trunk.run_trunk_train`` (batch-statistics BN, gradients to
    every trunk parameter) and ``forward_train`` takes ``pts_middle_feats``, or raw ``points``: with the sparse middle encoder frozen
    (``freeze_lidar_encoder()``: it stays in eval mode and takes no gradient), or -- ``train_sparse_encoder_hd=True`` -- with
    ``SparseEncoderHD`` training too (``lidar_hd``: batch-statistics BN1d, gradients through the per-axis rule books), so that a
    step from a raw cloud reaches every ``pts_middle_encoder`` / ``pts_backbone`` / ``pts_neck`` parameter."""
    WITH_RGB_HEAD = False
    DEPTH_GT_INDEX = -2
    TAKES_SPARSE_ENCODER_HD = True

    def trunk_from_middle(self, x):
        """SparseEncoderHD's dense output [B,C,Z,Y,X] (a tensor, Rows, or a view that remembers them) -> (pts_voxel_feats
        [1,C,X,Y,Z], [trunk output [B,C,Z,Y,X]]) (coocc_ray_lidar.py:249-256).  With both trunk modules of this package the whole
        trunk stays on channels-last rows: one entry transposition at most, no conversion towards the fuser / encoder."""
        from . import lidar_trunk as lt
        if isinstance(self.pts_backbone, lt.SECOND3D) and isinstance(self.pts_neck, lt.SECOND3DFPN):
            if self.train_lidar_trunk and self.training:
                # training (opt-in): the differentiable trunk; the views below keep the graph (view + permute of rows with a grad_fn).
                # A view that remembers its rows (SparseEncoderHD's output, with or without a grad_fn) hands them over as they are
                r = lt.rows_of_bczyx(x) if torch.is_tensor(x) else None
                rows = lt.run_trunk_train(self.pts_backbone, self.pts_neck, r if r is not None else x)
                return rows.as_ncdhw(), [lt.rows_as_bczyx(rows)]
            rows = lt.run_trunk(self.pts_backbone, self.pts_neck, x)
            return rows.as_ncdhw(), [lt.rows_as_bczyx(rows)]
        if self.pts_backbone is not None:
            x = self.pts_backbone(x)
        if self.pts_neck is not None:
            x = self.pts_neck(x)
        rows = lt.rows_of_bczyx(x) if torch.is_tensor(x) else None
        return (rows.as_ncdhw() if rows is not None else x.permute(0, 1, 4, 3, 2)), [x]

    def extract_pts_feat(self, pts):
        """coocc_ray_lidar.py:236-256: the dense LiDAR trunk returns [B,C,Z,Y,X]; the detector permutes to [B,C,X,Y,Z]."""
        if self.pts_backbone is None and self.pts_neck is None:
            raise NotImplementedError("COOCC_Ray_L was built without pts_backbone / pts_neck (SECOND3D / SECOND3DFPN)")
        if self.pts_middle_encoder is None:
            raise NotImplementedError("COOCC_Ray_L: the sparse middle encoder (SparseEncoderHD, spconv) is upstream of the hot path "
                                      "and was not attached; assign model.pts_middle_encoder, or feed its dense output as "
                                      "precomputed=dict(pts_middle_feats=...) (or the trunk's as pts_voxel_feats=...)")
        if isinstance(pts, (list, tuple)):
            assert len(pts) == 1, "batch size 1 (hard-coded upstream)"
            pts = pts[0]
        voxels, coors, num_points = self.pts_voxel_layer(pts)
        feats = self.pts_voxel_encoder(voxels, num_points, coors)
        return self.trunk_from_middle(self.pts_middle_encoder(feats, coors, 1))

    def _with_trunk(self, precomputed):
        """``precomputed`` with ``pts_middle_feats`` (the middle encoder's dense output) run through the trunk into ``pts_voxel_feats``."""
        if precomputed is not None and precomputed.get("pts_middle_feats") is not None and precomputed.get("pts_voxel_feats") is None:
            precomputed = dict(precomputed)
            precomputed["pts_voxel_feats"] = self.trunk_from_middle(precomputed.pop("pts_middle_feats"))[0]
        return precomputed

    def serving_frame(self, img=None, points=None, img_metas=None, precomputed=None):
        if precomputed is None and img is None and points is not None:
            # LiDAR-only from the cloud (no image branch to run): the LiDAR producer eagerly, as the base class does for a full frame
            precomputed = dict(pts_voxel_feats=self.extract_pts_feat(points)[0])
        return super().serving_frame(img, points, img_metas, self._with_trunk(precomputed))

    def forward_train(self, points=None, img_metas=None, img_inputs=None, gt_occ=None, points_occ=None, visible_mask=None,
                      gt_depths=None, precomputed=None, generator=None, **kwargs):
        if precomputed is not None and precomputed.get("pts_middle_feats") is not None:
            if not self.train_lidar_trunk:
                raise NotImplementedError("COOCC_Ray_L.forward_train: precomputed pts_middle_feats would run SECOND3D / SECOND3DFPN in "
                                          "training mode, which this detector was not built for (train_lidar_trunk=True); feed "
                                          "pts_voxel_feats")
            precomputed = self._with_trunk(precomputed)
        return super().forward_train(points, img_metas, img_inputs, gt_occ, points_occ, visible_mask, gt_depths, precomputed,
                                     generator, **kwargs)

    def simple_test(self, img_metas=None, img=None, gt_depths=None, points=None, rescale=False, points_occ=None,
                    gt_occ=None, visible_mask=None, precomputed=None):
        return super().simple_test(img_metas, img, gt_depths, points, rescale, points_occ, gt_occ, visible_mask,
                                   self._with_trunk(precomputed))
