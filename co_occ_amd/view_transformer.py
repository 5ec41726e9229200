"""``ViewTransformerLiftSplatShootVoxel`` -- P/coocc/image2bev/ViewTransformerLSSVoxel.py /
ViewTransformerLSSBEVDepth.py: geometry (P1), voxel pooling (P2), and ``forward`` with the reference signature where
Lift (x) Splat is ONE fused HIP pass (the [B,N,D,H,W,C] volume is never materialised).
DepthNet (DCN + ASPP, the image branch upstream of the path): ``depth_net='hip'`` builds this package's
``depth_net.DepthNet`` (HIP engine; ``train_depth_net=True`` also builds its training path); otherwise ``depth_net`` is an injected nn.Module, else the reference's own class
when the plugin and mmcv's DCN are importable.
"""
import torch
from torch import nn

from ._lib import call, host_f32, ptr
from .ops import _pool_workspace, pool_ws_clean, pool_ws_done
from .registry import NECKS

_F32 = torch.float32


def gen_dx_bx(xbound, ybound, zbound):
    """ViewTransformerLSSBEVDepth.py:21-25."""
    dx = torch.Tensor([row[2] for row in [xbound, ybound, zbound]])
    bx = torch.Tensor([row[0] + row[2] / 2.0 for row in [xbound, ybound, zbound]])
    nx = torch.Tensor([(row[1] - row[0]) / row[2] for row in [xbound, ybound, zbound]])
    return dx, bx, nx


def camera_mats(rots, trans, intrins, post_rots, post_trans, bda):
    """[B*N, COOCC_CAM_FLOATS] constants of the frustum -> ego chain (get_geometry / get_frustum): inv(post_rots),
    post_trans, rots @ inv(intrins[:3,:3]), trans, bda[:3,:3], the KITTI shift intrins[:3,3] (3x4 / 4x4 intrinsics,
    else 0) and the translation of a 4x4 bda (else 0).  One device kernel (coocc_camera_mats): torch.inverse would
    synchronise with the host."""
    B, N, _ = trans.shape
    f = lambda t: t.float().contiguous()
    kd, bd = int(intrins.shape[-1]), int(bda.shape[-1])
    if intrins.shape[-2] != kd:                      # 3x4 KITTI intrinsics: pad to 4x4 rows (only [:3,:] is read)
        intrins = torch.cat([intrins, intrins.new_zeros(B, N, kd - intrins.shape[-2], kd)], -2)
    mats = torch.empty(B * N, 39, device=trans.device, dtype=_F32)
    call("coocc_camera_mats", ptr(f(rots)), ptr(f(trans)), ptr(f(intrins)), ptr(f(post_rots)), ptr(f(post_trans)), ptr(f(bda)),
         B, N, kd, bd, ptr(mats))
    return mats


def frustum_axes(input_size, downsample, dbound, device):
    """The three axes of create_frustum (ViewTransformerLSSBEVDepth.py:104-115) for an ``input_size // downsample`` map."""
    ogfH, ogfW = int(input_size[0]), int(input_size[1])
    fH, fW = ogfH // downsample, ogfW // downsample
    ds = torch.arange(*dbound, dtype=torch.float)
    xs = torch.linspace(0, ogfW - 1, fW, dtype=torch.float)
    ys = torch.linspace(0, ogfH - 1, fH, dtype=torch.float)
    return xs.to(device), ys.to(device), ds.to(device)


def geometry_from_mats(mats, xs, ys, ds, B, N):
    D, fH, fW = ds.numel(), ys.numel(), xs.numel()
    geom = torch.empty(B, N, D, fH, fW, 3, device=mats.device, dtype=_F32)
    call("coocc_get_geometry", ptr(mats), ptr(xs), ptr(ys), ptr(ds), B * N, D, fH, fW, ptr(geom))
    return geom


def get_frustum(rots, trans, intrins, post_rots, post_trans, bda, input_size, scale):
    """Module-level ``get_frustum`` of the detector (P/coocc/detectors/coocc_ray.py:732-776): ego-frame sample points
    [B,N,D,H//scale,W//scale,3] of the 112 depth bins (2.0 .. 58.0 step 0.5, hard-coded upstream) for the LiDAR-only
    depth-render branch (:436-484).  input_size = (H, W) tensors / numbers; KITTI 3x4 intrinsics and 4x4 bda handled."""
    H = input_size[0].item() if torch.is_tensor(input_size[0]) else input_size[0]
    W = input_size[1].item() if torch.is_tensor(input_size[1]) else input_size[1]
    xs, ys, ds = frustum_axes((H, W), scale, (2.0, 58.0, 0.5), trans.device)
    mats = camera_mats(rots, trans, intrins, post_rots, post_trans, bda)
    return geometry_from_mats(mats, xs, ys, ds, trans.shape[0], trans.shape[1])


@NECKS.register_module()
class ViewTransformerLiftSplatShootVoxel(nn.Module):
    def __init__(self, loss_depth_weight=1.0, scale=16, point_cloud_range=None, loss_depth_type='bce',
                 grid_config=None, data_config=None, numC_input=512, numC_Trans=64, downsample=16,
                 accelerate=False, use_bev_pool=True, vp_megvii=False, vp_stero=False, cam_channels=27,
                 loss_depth_reg_weight=0.0, use_voxel_net=False, depth_net=None, train_depth_net=False, device_depth_loss=False,
                 **kwargs):
        super().__init__()
        # opt-in: get_depth_loss computes the depth labels, the BCE and its gradient on the device (losses.depth_loss_device: no host
        # read, bitwise reproducible) instead of eager torch
        self.device_depth_loss = bool(device_depth_loss)
        if use_voxel_net:
            raise NotImplementedError("DepthAggregation (use_voxel_net) is not used by the coocc_nusc configs")
        if grid_config is None:
            grid_config = {'xbound': [-51.2, 51.2, 0.8], 'ybound': [-51.2, 51.2, 0.8],
                           'zbound': [-10.0, 10.0, 20.0], 'dbound': [1.0, 60.0, 1.0]}
        if vp_megvii:
            raise NotImplementedError("vp_megvii pooling is not used by the coocc_nusc configs")
        self.grid_config = grid_config
        dx, bx, nx = gen_dx_bx(grid_config['xbound'], grid_config['ybound'], grid_config['zbound'])
        self.dx = nn.Parameter(dx, requires_grad=False)
        self.bx = nn.Parameter(bx, requires_grad=False)
        self.nx = nn.Parameter(nx, requires_grad=False)
        self.data_config = data_config or {'input_size': (256, 704)}
        self.downsample, self.scale = downsample, scale
        self.numC_input, self.numC_Trans = numC_input, numC_Trans
        self.loss_depth_weight, self.loss_depth_type = loss_depth_weight, loss_depth_type
        self.cam_depth_range = grid_config['dbound']
        self.point_cloud_range = point_cloud_range
        self.frustum = self.create_frustum()
        self.D = self.frustum.shape[0]
        self.cam_channels = cam_channels
        if isinstance(depth_net, nn.Module):
            self.depth_net = depth_net
        elif isinstance(depth_net, str) and depth_net == 'hip':
            # opt-in: DepthNet(numC_input, numC_input, numC_Trans, D, cam_channels) of ViewTransformerLSSBEVDepth.py:616-617 on the HIP engine
            from .depth_net import DepthNet
            self.depth_net = DepthNet(self.numC_input, self.numC_input, self.numC_Trans, self.D, cam_channels=self.cam_channels)
            # opt-in: under train() DepthNet runs its differentiable forward on the HIP engine (off: train() raises)
            self.depth_net.train_enabled = bool(train_depth_net)
        else:
            self.depth_net = self._reference_depth_net()
        if train_depth_net and not (isinstance(depth_net, str) and depth_net == 'hip'):
            raise ValueError("ViewTransformerLiftSplatShootVoxel: train_depth_net=True trains this package's DepthNet; pass depth_net='hip'")

    def _reference_depth_net(self):
        """DepthNet(numC_input, numC_input, numC_Trans, D, cam_channels) of ViewTransformerLSSBEVDepth.py:616-617 -- the
        reference's class (it needs mmcv's DCN), or None when the plugin / mmcv are not importable (forward then raises)."""
        try:
            from projects.mmdet3d_plugin.coocc.image2bev.ViewTransformerLSSBEVDepth import DepthNet
            return DepthNet(self.numC_input, self.numC_input, self.numC_Trans, self.D, cam_channels=self.cam_channels)
        except Exception:
            return None

    def get_depth_dist(self, x):
        return x.softmax(dim=1)

    def create_frustum(self):
        """ViewTransformerLSSBEVDepth.py:104-115 (kept as the reference's [D,fH,fW,3] Parameter)."""
        ogfH, ogfW = self.data_config['input_size']
        fH, fW = ogfH // self.downsample, ogfW // self.downsample
        ds = torch.arange(*self.grid_config['dbound'], dtype=torch.float).view(-1, 1, 1).expand(-1, fH, fW)
        D = ds.shape[0]
        xs = torch.linspace(0, ogfW - 1, fW, dtype=torch.float).view(1, 1, fW).expand(D, fH, fW)
        ys = torch.linspace(0, ogfH - 1, fH, dtype=torch.float).view(1, fH, 1).expand(D, fH, fW)
        return nn.Parameter(torch.stack((xs, ys, ds), -1), requires_grad=False)

    def _camera_mats(self, rots, trans, intrins, post_rots, post_trans, bda):
        """Per-camera constants of the geometry chain (COOCC_CAM_FLOATS each) + the frustum axes."""
        # the three axes depend on the frustum parameter only: kept (three copy launches per sample otherwise, inside every captured graph)
        key = (self.frustum._version, self.frustum.data_ptr(), trans.device)
        ax = getattr(self, "_axes_cache", None)
        if ax is None or ax[0] != key:
            fr = self.frustum.detach().to(trans.device)
            ax = (key, fr[0, 0, :, 0].contiguous(), fr[0, :, 0, 1].contiguous(), fr[:, 0, 0, 2].contiguous())
            self._axes_cache = ax
        return camera_mats(rots, trans, intrins, post_rots, post_trans, bda), ax[1], ax[2], ax[3]

    def get_geometry(self, rots, trans, intrins, post_rots, post_trans, bda):
        """ViewTransformerLSSBEVDepth.py:117-150 -> [B,N,D,fH,fW,3].  The 3x3 inverses and the
        rots @ inv(intrins) product are host-side torch (6 tiny matrices); the per-point chain
        runs in one HIP kernel."""
        mats, xs, ys, ds = self._camera_mats(rots, trans, intrins, post_rots, post_trans, bda)
        return geometry_from_mats(mats, xs, ys, ds, trans.shape[0], trans.shape[1])

    def get_frustum(self, rots, trans, intrins, post_rots, post_trans, bda, scale):
        """ViewTransformerLSSBEVDepth.py:152-195: the same chain on a frustum of ``input_size // scale`` pixels."""
        xs, ys, ds = frustum_axes(self.data_config['input_size'], scale, self.grid_config['dbound'], trans.device)
        mats = camera_mats(rots, trans, intrins, post_rots, post_trans, bda)
        return geometry_from_mats(mats, xs, ys, ds, trans.shape[0], trans.shape[1])

    def get_mlp_input(self, rot, tran, intrin, post_rot, post_tran, bda=None):
        """ViewTransformerLSSBEVDepth.py:636-691: the camera-parameter vector DepthNet's SE branches consume
        (27 numbers per camera for 3x3 intrinsics and bda; KITTI 3x4 intrinsics add 3, a 4x4 bda adds 3)."""
        B, N = rot.shape[:2]
        if bda is None:
            bda = torch.eye(3).to(rot).view(1, 3, 3).repeat(B, 1, 1)
        bda = bda.view(B, 1, *bda.shape[-2:]).repeat(1, N, 1, 1)
        pick = lambda m, ij: [m[:, :, i, j] for i, j in ij]
        kitti = intrin.shape[-1] == 4
        cols = pick(intrin, [(0, 0), (1, 1), (0, 2), (1, 2)] + ([(0, 3), (1, 3), (2, 3)] if kitti else []))
        cols += pick(post_rot, [(0, 0), (0, 1)]) + [post_tran[:, :, 0]] + pick(post_rot, [(1, 0), (1, 1)]) + [post_tran[:, :, 1]]
        cols += pick(bda, [(0, 0), (0, 1), (1, 0), (1, 1), (2, 2)])
        mlp_input = torch.stack(cols, dim=-1)
        if kitti and bda.shape[-1] == 4:
            mlp_input = torch.cat((mlp_input, bda[:, :, :3, -1]), dim=2)
        sensor2ego = torch.cat([rot, tran.reshape(B, N, 3, 1)], dim=-1).reshape(B, N, -1)
        return torch.cat([mlp_input, sensor2ego], dim=-1)

    def _grid_host(self):
        """(X, Y, Z) and [lo(3), dx(3)] of the pooling grid as host numbers.  nx / bx / dx are Parameters as upstream, so they
        live on the device after ``.to()``: reading them per call would be three device->host synchronisations per sample;
        the host copy is refreshed whenever one of them is written (``load_state_dict`` bumps ``_version``)."""
        key = (self.nx._version, self.bx._version, self.dx._version, self.nx.data_ptr())
        if getattr(self, "_grid_host_key", None) != key:
            nx = tuple(int(v) for v in self.nx.tolist())
            lo = (self.bx - self.dx / 2.).tolist() + self.dx.tolist()
            self._grid_host_val, self._grid_host_key = (nx, lo), key
        return self._grid_host_val

    def voxel_pooling(self, geom_feats, x):
        """ViewTransformerLSSVoxel.py:100-123: geom [B,N,D,H,W,3], x [B,N,D,H,W,C] -> [B,C,X,Y,Z]
        (a channels-last view).  Truncate-then-filter quantisation and the pooling run in the
        library without argsort / boolean-mask compaction."""
        B, N, D, H, W, C = x.shape
        Nprime = B * N * D * H * W
        (X, Y, Z), lo = self._grid_host()
        xf = x.reshape(Nprime, C).float().contiguous()
        g = geom_feats.reshape(Nprime, 3).float().contiguous()
        out = torch.empty(B * X * Y * Z, C, device=x.device, dtype=_F32)
        ws = _pool_workspace(x.device, Nprime, B * X * Y * Z)
        call("coocc_voxel_pool", ptr(xf), ptr(g), Nprime, Nprime // B, C, host_f32(lo), B, X, Y, Z,
             ptr(out), C, ptr(ws), ws.numel(), pool_ws_clean(ws, Nprime, B * X * Y * Z))
        pool_ws_done(ws, Nprime, B * X * Y * Z)
        return out.view(B, X, Y, Z, C).permute(0, 4, 1, 2, 3)

    def lift_splat(self, depth_prob, img_feat, geom_feats=None, cams=None, out=None):
        """Fused Lift + Splat (ViewTransformerLSSVoxel.py:135-145 without the [B,N,D,H,W,C] volume):
        depth_prob [B*N,D,H,W], img_feat [B*N,C,H,W] -> [B,C,X,Y,Z].  Geometry is either the tensor
        get_geometry returned ([B,N,D,H,W,3]) or, with cams=(rots, trans, intrins, post_rots, post_trans,
        bda), computed inside the key kernel so it never exists in HBM.  ``out``: Rows to write into (e.g. slot 0 of the
        fuser's concat buffer, ``BiFuser_N.concat_buffer``) instead of a fresh [V,C] tensor."""
        BN, C, H, W = img_feat.shape
        D = depth_prob.shape[1]
        assert tuple(depth_prob.shape) == (BN, D, H, W) and (geom_feats is None) != (cams is None)
        B = geom_feats.shape[0] if cams is None else cams[1].shape[0]
        (X, Y, Z), lo = self._grid_host()
        lo = host_f32(lo)
        dev = img_feat.device
        feat = torch.empty(BN * H * W, C, device=dev, dtype=_F32)
        call("coocc_ncdhw_to_ndhwc", ptr(img_feat.float().contiguous()), ptr(feat), BN, C, H * W, C, 0)
        npts = BN * D * H * W
        if out is None:
            out_t, out_stride, out_ptr = torch.empty(B * X * Y * Z, C, device=dev, dtype=_F32), C, None
        else:
            assert (out.B, out.X, out.Y, out.Z, out.C) == (B, X, Y, Z, C) and out.t.is_contiguous()
            out_t, out_stride, out_ptr = out.t, out.stride, out.data()
        if out_ptr is None:
            out_ptr = ptr(out_t)
        ws = _pool_workspace(dev, npts, B * X * Y * Z)
        dp = depth_prob.float().contiguous()
        if getattr(self, "accelerate", False) and not self.training:
            # fixed camera rig (the reference's ``accelerate`` flag, ViewTransformerLSSBEVDepth.py:67,242-300 -- the CALLER asserts
            # that rots / trans / intrins / post_* / bda do not change between frames, exactly as upstream; training-time bda
            # augmentation changes them every step, so the cache is bypassed under ``train()``; ``invalidate_geometry_cache()``
            # after a rig change): the voxel binning of the first call is kept in a private workspace and every later call only
            # runs the per-voxel sums.  The binning was built on ONE stream: its completion event is waited for by any other
            # stream that reuses it (per-slot prefetch streams).
            key = (dev.index, npts, B * X * Y * Z)
            cache = getattr(self, "_geometry_cache", None)
            if cache is not None and cache[0] == key:
                cur = torch.cuda.current_stream(dev)
                if cache[3] != cur.cuda_stream:
                    cur.wait_event(cache[2])
                call("coocc_lift_splat_reuse", ptr(dp), ptr(feat), BN, D, H, W, C, B, X, Y, Z, out_ptr, out_stride, ptr(cache[1]),
                     cache[1].numel())
                if out is not None:
                    v = out.as_ncdhw()
                    v._coocc_keep = out.t
                    return v
                return out_t.view(B, X, Y, Z, C).permute(0, 4, 1, 2, 3)
            ws = torch.empty_like(ws)
            self._geometry_cache_pending = (key, ws)
        from ._lib import TIMER
        # algorithmic HBM bytes of the fused form: depth + context rows read, pooled rows written
        with TIMER.region("k_lift_splat", 4.0 * npts + 4.0 * BN * H * W * C + 4.0 * B * X * Y * Z * C):
            if cams is None:
                assert geom_feats.numel() == npts * 3
                g = geom_feats.reshape(-1, 3).float().contiguous()
                call("coocc_lift_splat", ptr(dp), ptr(feat), ptr(g), BN, D, H, W, C, npts // B, lo, B, X, Y, Z, out_ptr, out_stride,
                     ptr(ws), ws.numel(), pool_ws_clean(ws, npts, B * X * Y * Z))
            else:
                mats, xs, ys, ds = self._camera_mats(*cams)
                assert (ds.numel(), ys.numel(), xs.numel()) == (D, H, W)
                call("coocc_lift_splat_cams", ptr(dp), ptr(feat), ptr(mats), ptr(xs), ptr(ys), ptr(ds), BN, D, H, W, C,
                     npts // B, lo, B, X, Y, Z, out_ptr, out_stride, ptr(ws), ws.numel(), pool_ws_clean(ws, npts, B * X * Y * Z))
            pool_ws_done(ws, npts, B * X * Y * Z)
        pend = getattr(self, "_geometry_cache_pending", None)
        if pend is not None and pend[1] is ws:
            ev = torch.cuda.Event()
            ev.record()
            self._geometry_cache = (pend[0], ws, ev, torch.cuda.current_stream(dev).cuda_stream)
            self._geometry_cache_pending = None
        if out is not None:
            v = out.as_ncdhw()
            v._coocc_keep = out.t            # the buffer object BiFuser_N.concat_buffer registered stays alive with the view
            return v
        return out_t.view(B, X, Y, Z, C).permute(0, 4, 1, 2, 3)

    def lift(self, input):
        """The Lift half alone (ViewTransformerLSSVoxel.py:125-134): (x [B,N,C,H,W], rots, ..., bda, mlp_input) ->
        (depth_prob [B*N,D,H,W], img_feat [B*N,C,H,W]) -- what ``lift_splat`` / ``serving.ServingPipeline`` consume."""
        x = input[0]
        if self.depth_net is None:
            raise NotImplementedError("ViewTransformerLiftSplatShootVoxel.lift: DepthNet is upstream of the hot path and "
                                      "could not be built here (needs the reference plugin + mmcv DCN); pass depth_net='hip' or depth_net=<module>")
        B, N, C, H, W = x.shape
        y = self.depth_net(x.view(B * N, C, H, W), input[7])
        return self.get_depth_dist(y[:, :self.D, ...]), y[:, self.D:self.D + self.numC_Trans, ...]

    def invalidate_geometry_cache(self):
        """Drop the cached voxel binning of ``accelerate`` (call after the camera rig changed)."""
        self._geometry_cache = self._geometry_cache_pending = None

    def forward(self, input):
        """ViewTransformerLSSVoxel.py:125-145, reference signature:
        (x [B,N,C,H,W], rots, trans, intrins, post_rots, post_trans, bda, mlp_input) ->
        (bev_feat [B,C,X,Y,Z], depth_prob [B*N,D,H,W], geom [B,N,D,H,W,3], sum_d volume [B*N,H,W,C]).
        DepthNet is upstream torch; Lift (x) Splat is one fused HIP pass with the geometry computed in the key kernel
        (inference) or through ``autograd.lift_splat`` (when gradients are needed).
        A 6-D first element is taken as an already-lifted volume [B,N,D,H,W,C] -> (bev_feat, geom) (the Splat half alone)."""
        x, rots, trans, intrins, post_rots, post_trans, bda = input[:7]
        if x.dim() == 6:
            geom = self.get_geometry(rots, trans, intrins, post_rots, post_trans, bda)
            return self.voxel_pooling(geom, x), geom
        if self.depth_net is None:
            raise NotImplementedError("ViewTransformerLiftSplatShootVoxel.forward: DepthNet is upstream of the hot path and "
                                      "could not be built here (needs the reference plugin + mmcv DCN); pass depth_net='hip' or depth_net=<module>")
        B, N, C, H, W = x.shape
        y = self.depth_net(x.view(B * N, C, H, W), input[7])
        depth_prob = self.get_depth_dist(y[:, :self.D, ...])
        img_feat = y[:, self.D:self.D + self.numC_Trans, ...]
        geom = self.get_geometry(rots, trans, intrins, post_rots, post_trans, bda)
        if torch.is_grad_enabled() and (depth_prob.requires_grad or img_feat.requires_grad):
            from . import autograd as ag
            bev_feat = ag.lift_splat(self, depth_prob, img_feat, geom)
        else:
            bev_feat = self.lift_splat(depth_prob, img_feat, cams=(rots, trans, intrins, post_rots, post_trans, bda))
        vol_sum = (img_feat * depth_prob.sum(1, keepdim=True)).permute(0, 2, 3, 1)      # == volume.sum over D (:145)
        return bev_feat, depth_prob, geom, vol_sum

    # ------------------------------------------------------------------ DepthNet supervision (upstream torch, eager; with
    # ``device_depth_loss`` get_depth_loss runs csrc/depth_loss.hip instead)
    def get_downsampled_gt_depth(self, gt_depths):
        """ViewTransformerLSSVoxel.py:30-56: [B,N,H,W] metric depth -> (bin values [B*N,h,w], one-hot [B*N*h*w, D]) with the
        nearest non-zero depth of every downsample x downsample patch."""
        B, N, H, W = gt_depths.shape
        ds = self.downsample
        g = gt_depths.view(B * N, H // ds, ds, W // ds, ds).permute(0, 1, 3, 2, 4).reshape(-1, ds * ds)
        g = torch.where(g == 0.0, torch.full_like(g, 1e5), g).min(dim=-1).values.view(B * N, H // ds, W // ds)
        db = self.grid_config['dbound']
        g = (g - (db[0] - db[2] / 2)) / db[2]
        vals = g.clone()
        g = torch.where((g < self.D + 1) & (g >= 0.0), g, torch.zeros_like(g))
        onehot = torch.nn.functional.one_hot(g.long(), num_classes=self.D + 1).view(-1, self.D + 1)[:, 1:]
        return vals, onehot.float()

    def get_depth_loss(self, depth_labels, depth_preds):
        """ViewTransformerLSSVoxel.py:58-98, 'bce' type (what the coocc_nusc configs set).  ``device_depth_loss``: the same number and
        its gradient from ``losses.depth_loss_device`` (HIP kernels, no host read)."""
        if self.loss_depth_type != 'bce':
            raise NotImplementedError("loss_depth_type %r: only 'bce' is used by the coocc_nusc configs" % self.loss_depth_type)
        if self.device_depth_loss:
            from .losses import depth_loss_device
            return depth_loss_device(depth_preds, depth_labels, self.downsample, self.grid_config['dbound'], self.D, self.loss_depth_weight)
        _, labels = self.get_downsampled_gt_depth(depth_labels)
        preds = depth_preds.permute(0, 2, 3, 1).contiguous().view(-1, self.D)
        fg = labels.max(dim=1).values > 0.0
        loss = torch.nn.functional.binary_cross_entropy(preds[fg].float(), labels[fg], reduction='none').sum() / max(1.0, float(fg.sum()))
        return self.loss_depth_weight * loss
