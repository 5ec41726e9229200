"""Registry surface of the reference (mmcv ``Registry`` name lookup).

``dict(type='BiFuser_N', ...)`` configs resolve through ``FUSION_LAYERS.build(cfg)`` exactly as
``mmdet3d.models.builder`` does (M/models/builder.py:10-24,97-99).  When mmdet / mmdet3d are
importable, :func:`register_into_mmdet` additionally registers the classes into the real
registries (``force=True``), which is what makes ``projects/configs/coocc_nusc/*`` build our
modules unchanged.
"""


class Registry:
    def __init__(self, name):
        self.name = name
        self._module_dict = {}

    @property
    def module_dict(self):
        return self._module_dict

    def get(self, key):
        return self._module_dict.get(key)

    def __contains__(self, key):
        return key in self._module_dict

    def register_module(self, name=None, force=False, module=None):
        def _register(cls):
            key = name or cls.__name__
            if key in self._module_dict and not force:
                raise KeyError("%s is already registered in %s" % (key, self.name))
            self._module_dict[key] = cls
            return cls
        return _register(module) if module is not None else _register

    def build(self, cfg, default_args=None):
        if not isinstance(cfg, dict) or "type" not in cfg:
            raise TypeError("cfg must be a dict with a 'type' key, got %r" % (cfg,))
        args = dict(cfg)
        for k, v in (default_args or {}).items():
            args.setdefault(k, v)
        t = args.pop("type")
        cls = self.get(t) if isinstance(t, str) else t
        if cls is None:
            raise KeyError("%s is not in the %s registry" % (t, self.name))
        return cls(**args)


DETECTORS = Registry("detector")
BACKBONES = Registry("backbone")
NECKS = Registry("neck")
HEADS = Registry("head")
FUSION_LAYERS = Registry("fusion_layer")


def build_fusion_layer(cfg):
    return FUSION_LAYERS.build(cfg)


def build_backbone(cfg):
    return BACKBONES.build(cfg)


def build_neck(cfg):
    return NECKS.build(cfg)


def build_head(cfg, **kw):
    return HEADS.build(cfg)


def build_detector(cfg, train_cfg=None, test_cfg=None, **overrides):
    """``overrides`` are merged into the config (e.g. ``external_encoders=True``, ``img_backbone=<module>``)."""
    return DETECTORS.build(dict(cfg, **overrides))


def register_into_mmdet(detectors=False, sparse_encoder_hd=False, train_lidar_trunk=False, train_sparse_encoder_hd=False,
                        device_occ_losses=False, hip_depth_net=False, train_depth_net=False, hip_image_encoder=False,
                        train_image_encoder=False, device_depth_loss=False):
    """Register our classes under the reference names into the real mmdet / mmdet3d registries (``force=True``).

    Default: the hot-path MODULES only (BiFuser_N, CustomResNet3D, FPN3D, OccHead, ViewTransformerLiftSplatShootVoxel and
    the LiDAR producer) -- the reference's own ``COOCC_Ray`` then builds them from its unchanged configs and keeps its
    encoders, losses and metrics.  ``detectors=True`` additionally replaces ``COOCC_Ray`` / ``COOCC_Ray_L`` with ours (HIP
    render block, on-device metrics; its image encoder is built back through these same registries).
    ``sparse_encoder_hd=True`` additionally replaces mmdet3d's ``SparseEncoderHD`` middle encoder (spconv v1) with
    ``lidar_hd.SparseEncoderHD``.  ``train_lidar_trunk=True`` (with ``detectors=True``: the option is the detector's) registers
    ``COOCC_Ray_L`` with its ``train_lidar_trunk`` option on by default, so an unchanged coocc_lidar.py config trains SECOND3D /
    SECOND3DFPN on the HIP engine.  ``train_sparse_encoder_hd=True`` (with ``sparse_encoder_hd=True``) registers a
    ``SparseEncoderHD`` whose ``train_enabled`` is on, so the reference's own detector trains it under ``train()``; with
    ``detectors=True`` our ``COOCC_Ray_L`` is registered with the option on by default as well.  ``device_occ_losses=True`` (with
    ``detectors=True``) registers ``COOCC_Ray`` and ``COOCC_Ray_L`` with their ``device_occ_losses`` option on by default: OccHead's
    loss terms and their gradient are computed on the device.  ``hip_depth_net=True`` registers a
    ``ViewTransformerLiftSplatShootVoxel`` whose ``depth_net`` option defaults to ``'hip'``: an unchanged config then runs DepthNet on
    the HIP engine (``depth_net.DepthNet``) instead of the reference's class and mmcv's DCN; ``train_depth_net=True`` (with
    ``hip_depth_net=True``) registers it with its ``train_depth_net`` option on by default as well, so the module also trains on the
    HIP engine under ``train()``.  ``hip_image_encoder=True`` registers ``image_encoder.ResNet`` / ``image_encoder.SECONDFPN`` (the 2-D
    image backbone and neck on the HIP engine) under the reference names ``ResNet`` / ``SECONDFPN``, so an unchanged config builds
    them as ``img_backbone`` / ``img_neck``; ``train_image_encoder=True`` (with ``hip_image_encoder=True``) registers them with their
    ``train_enabled`` option on, so the reference's own detector trains them on the HIP engine under ``train()`` (``frozen_stages`` /
    ``norm_eval`` as in mmdet).  ``device_depth_loss=True`` registers a ``ViewTransformerLiftSplatShootVoxel`` whose
    ``device_depth_loss`` option is on by default (a subclass of whatever ``hip_depth_net`` / ``train_depth_net`` produced): the
    reference's own detector calls its ``get_depth_loss``, which then computes the depth labels, the BCE and its gradient on the device
    without a host read; with ``detectors=True`` ``COOCC_Ray`` and ``COOCC_Ray_L`` are registered with the option on by default as well
    (on top of the ``device_occ_losses`` and trunk-training wrappers).  Returns False when mmdet / mmdet3d are not importable."""
    if train_image_encoder and not hip_image_encoder:
        raise ValueError("register_into_mmdet: train_image_encoder=True trains this package's ResNet / SECONDFPN; pass "
                         "hip_image_encoder=True")
    if train_depth_net and not hip_depth_net:
        raise ValueError("register_into_mmdet: train_depth_net=True trains this package's DepthNet; pass hip_depth_net=True")
    if device_occ_losses and not detectors:
        raise ValueError("register_into_mmdet: device_occ_losses=True is an option of this package's detectors; pass detectors=True")
    if train_lidar_trunk and not detectors:
        raise ValueError("register_into_mmdet: train_lidar_trunk=True is an option of this package's COOCC_Ray_L; pass detectors=True")
    if train_sparse_encoder_hd and not sparse_encoder_hd:
        raise ValueError("register_into_mmdet: train_sparse_encoder_hd=True trains this package's SparseEncoderHD; pass "
                         "sparse_encoder_hd=True")
    try:
        from mmdet.models import builder as mb
        from mmdet3d.models import builder as m3b
    except Exception:
        return False
    pairs = [(BACKBONES, m3b.BACKBONES), (NECKS, m3b.NECKS), (HEADS, m3b.HEADS), (FUSION_LAYERS, m3b.FUSION_LAYERS)]
    if detectors:
        pairs.append((DETECTORS, mb.DETECTORS))
    from . import lidar
    pairs += [(lidar.VOXEL_ENCODERS, m3b.VOXEL_ENCODERS), (lidar.MIDDLE_ENCODERS, m3b.MIDDLE_ENCODERS)]
    if sparse_encoder_hd:
        from . import lidar_hd
        pairs.append((lidar_hd.MIDDLE_ENCODERS_HD, m3b.MIDDLE_ENCODERS))
    for ours, theirs in pairs:
        for k, cls in ours.module_dict.items():
            theirs.register_module(name=k, force=True, module=cls)
    if train_sparse_encoder_hd:
        m3b.MIDDLE_ENCODERS.register_module(name="SparseEncoderHD", force=True, module=training_sparse_encoder_hd())
    if hip_depth_net:
        m3b.NECKS.register_module(name="ViewTransformerLiftSplatShootVoxel", force=True, module=hip_depth_net_view_transformer(train_depth_net))
    if hip_image_encoder:
        from . import image_encoder
        bb, nk = training_image_encoder() if train_image_encoder else (image_encoder.ResNet, image_encoder.SECONDFPN)
        m3b.BACKBONES.register_module(name="ResNet", force=True, module=bb)
        m3b.NECKS.register_module(name="SECONDFPN", force=True, module=nk)
    if detectors and (train_lidar_trunk or train_sparse_encoder_hd):
        mb.DETECTORS.register_module(name="COOCC_Ray_L", force=True,
                                     module=trunk_training_detector(train_lidar_trunk, train_sparse_encoder_hd))
    if detectors and device_occ_losses:
        for name in ("COOCC_Ray", "COOCC_Ray_L"):
            mb.DETECTORS.register_module(name=name, force=True, module=device_occ_losses_detector(mb.DETECTORS.module_dict[name]))
    if device_depth_loss:
        name = "ViewTransformerLiftSplatShootVoxel"
        m3b.NECKS.register_module(name=name, force=True, module=device_depth_loss_view_transformer(m3b.NECKS.module_dict[name]))
        if detectors:
            for name in ("COOCC_Ray", "COOCC_Ray_L"):
                mb.DETECTORS.register_module(name=name, force=True, module=device_depth_loss_detector(mb.DETECTORS.module_dict[name]))
    return True


def device_depth_loss_view_transformer(base=None):
    """``base`` (``ViewTransformerLiftSplatShootVoxel``, possibly already a ``hip_depth_net_view_transformer``) whose
    ``device_depth_loss`` option is on by default (what ``register_into_mmdet(device_depth_loss=True)`` puts into mmdet3d's registry
    under the reference name)."""
    if base is None:
        base = NECKS.get("ViewTransformerLiftSplatShootVoxel")

    class _VT(base):
        def __init__(self, *args, device_depth_loss=True, **kwargs):
            super().__init__(*args, device_depth_loss=device_depth_loss, **kwargs)
    _VT.__name__ = _VT.__qualname__ = base.__name__
    return _VT


def device_depth_loss_detector(base):
    """``base`` (``COOCC_Ray`` / ``COOCC_Ray_L``, possibly already a ``device_occ_losses_detector`` / ``trunk_training_detector``)
    whose ``device_depth_loss`` option is on by default (``register_into_mmdet(detectors=True, device_depth_loss=True)``)."""
    if isinstance(base, str):
        base = DETECTORS.get(base)

    class _Det(base):
        def __init__(self, *args, device_depth_loss=True, **kwargs):
            super().__init__(*args, device_depth_loss=device_depth_loss, **kwargs)
    _Det.__name__ = _Det.__qualname__ = base.__name__
    return _Det


def device_occ_losses_detector(base):
    """``base`` (``COOCC_Ray`` / ``COOCC_Ray_L``, possibly already a ``trunk_training_detector``) whose ``device_occ_losses`` option is
    on by default (what ``register_into_mmdet(detectors=True, device_occ_losses=True)`` puts into mmdet's registry)."""
    if isinstance(base, str):
        base = DETECTORS.get(base)

    class _Det(base):
        def __init__(self, *args, device_occ_losses=True, **kwargs):
            super().__init__(*args, device_occ_losses=device_occ_losses, **kwargs)
    _Det.__name__ = _Det.__qualname__ = base.__name__
    return _Det


def trunk_training_detector(train_lidar_trunk=True, train_sparse_encoder_hd=False):
    """``COOCC_Ray_L`` whose ``train_lidar_trunk`` / ``train_sparse_encoder_hd`` options default to the given values (what
    ``register_into_mmdet(train_lidar_trunk=True)`` puts into mmdet's registry under the reference name)."""
    base = DETECTORS.get("COOCC_Ray_L")
    trunk_default, hd_default = bool(train_lidar_trunk), bool(train_sparse_encoder_hd)

    class COOCC_Ray_L(base):
        def __init__(self, *args, train_lidar_trunk=trunk_default, train_sparse_encoder_hd=hd_default, **kwargs):
            super().__init__(*args, train_lidar_trunk=train_lidar_trunk, train_sparse_encoder_hd=train_sparse_encoder_hd, **kwargs)
    COOCC_Ray_L.__qualname__ = "COOCC_Ray_L"
    return COOCC_Ray_L


def hip_depth_net_view_transformer(train_depth_net=False):
    """``ViewTransformerLiftSplatShootVoxel`` whose ``depth_net`` option defaults to ``'hip'`` and whose ``train_depth_net`` option
    defaults to the given value (what ``register_into_mmdet(hip_depth_net=True)`` puts into mmdet3d's registry under the reference
    name)."""
    base = NECKS.get("ViewTransformerLiftSplatShootVoxel")
    train_default = bool(train_depth_net)

    class ViewTransformerLiftSplatShootVoxel(base):
        def __init__(self, *args, depth_net='hip', train_depth_net=train_default, **kwargs):
            super().__init__(*args, depth_net=depth_net, train_depth_net=train_depth_net, **kwargs)
    ViewTransformerLiftSplatShootVoxel.__qualname__ = "ViewTransformerLiftSplatShootVoxel"
    return ViewTransformerLiftSplatShootVoxel


def training_image_encoder():
    """(``image_encoder.ResNet``, ``image_encoder.SECONDFPN``) with ``train_enabled`` on (what
    ``register_into_mmdet(hip_image_encoder=True, train_image_encoder=True)`` puts into mmdet3d's registries: upstream's constructor
    signatures, the differentiable forward and mmdet's stage freezing under ``train()``)."""
    from . import image_encoder

    def enabled(base):
        class _Enabled(base):
            def __init__(self, *args, **kwargs):
                super().__init__(*args, **kwargs)
                self.train_enabled = True
                self.train(self.training)
        _Enabled.__name__ = _Enabled.__qualname__ = base.__name__
        return _Enabled
    return enabled(image_encoder.ResNet), enabled(image_encoder.SECONDFPN)


def training_sparse_encoder_hd():
    """``lidar_hd.SparseEncoderHD`` with ``train_enabled`` on (what ``register_into_mmdet(train_sparse_encoder_hd=True)`` puts into
    mmdet3d's registry: upstream's constructor signature, the differentiable forward under ``train()``)."""
    from . import lidar_hd

    class SparseEncoderHD(lidar_hd.SparseEncoderHD):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            self.train_enabled = True
    SparseEncoderHD.__qualname__ = "SparseEncoderHD"
    return SparseEncoderHD
