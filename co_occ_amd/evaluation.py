"""On-device evaluation -- mirror of ``COOCC_Ray.evaluation_semantic`` (P/coocc/detectors/coocc_ray.py:659-684),
``fast_hist`` (:726-730) and ``cm_to_ious`` (P/utils/formating.py:4-14).

The reference resamples the logits to the ground-truth size, takes the argmax, copies prediction and
label to the host and runs ``np.bincount`` three times per prediction.  Here one kernel produces the
SC, SSC and visible-only SSC confusion matrices on the device; ``SemanticEvaluator`` accumulates them
over a whole validation set and reads them back once.

The lidarseg metrics (``points_occ``: OccHead.forward_lidarseg, occ_head.py:339-383, and simple_evaluation_semantic,
coocc_ray.py:693-700) take the same route: ``lidarseg_points`` samples the logits at the points, labels them and builds the
16x16 ``fast_hist_crop`` matrix in one kernel; ``LidarSegEvaluator`` accumulates it over a dataset.

The rendered maps of ``test_rendering`` (coocc_ray.py:626-637, P/utils/save_rendered_img.py) are judged the same way:
``render_eval`` gives the per-view PSNR, the depth error and the comparison panels from two kernels and, on request, the SSIM of
the colour maps (``render_ssim``, skimage's ``structural_similarity`` as save_rendered_img.py:22-37 calls it); ``RenderEvaluator``
accumulates them over a dataset."""
import contextlib
import warnings

import numpy as np
import torch

from ._lib import call, check, host_f32, load, ptr

NOISE = 255


def _as_u8(t):
    if t.dtype != torch.uint8:
        t = t.to(torch.uint8)   # labels 0..C-1 and 255 survive the narrowing (astype(np.int) upstream)
    return t.contiguous()


def semantic_histograms(pred, gt, visible_mask=None, empty_idx=0, out=None, accumulate=False):
    """pred [1,C,h,w,d] float logits (any strides), gt [1,H,W,D] labels, visible_mask [1,H,W,D] or None
    -> int64 device tensor [4 + 2*C*C] = SC 2x2 | SSC CxC | OCC CxC, each [label][pred]."""
    if not pred.is_cuda:
        raise RuntimeError("co_occ_amd.evaluation runs on the HIP device only")
    assert pred.dim() == 5 and pred.shape[0] == 1 and gt.dim() == 4 and gt.shape[0] == 1, "batch size 1 (coocc_ray.py:662)"
    pred = pred.float()
    C, h, w, d = pred.shape[1:]
    H, W, D = gt.shape[1:]
    g = _as_u8(gt[0])
    v = _as_u8(visible_mask[0] != 0) if visible_mask is not None else None
    if out is None:
        out = torch.empty(4 + 2 * C * C, dtype=torch.int64, device=pred.device)
        accumulate = False
    sc, sx, sy, sz = pred.stride()[1:]
    call("coocc_eval_semantic", ptr(pred, strided=True), sc, sx, sy, sz, C, h, w, d, ptr(g), ptr(v) if v is not None else None,
         H, W, D, int(empty_idx), 1 if accumulate else 0, ptr(out))
    return out


def split_histograms(hist, C):
    return hist[:4].view(2, 2), hist[4:4 + C * C].view(C, C), hist[4 + C * C:].view(C, C)


def evaluation_semantic(pred, gt, eval_type, visible_mask=None, empty_idx=0):
    """Signature and return convention of coocc_ray.py:659: 'SC' -> (hist 2x2, None); 'SSC' -> (hist CxC,
    hist_occ CxC or None).  Histograms are int64 device tensors (``.cpu().numpy()`` gives the upstream arrays)."""
    C = pred.shape[1]
    sc, ssc, occ = split_histograms(semantic_histograms(pred, gt, visible_mask, empty_idx), C)
    if eval_type == 'SC':
        return sc, None
    if eval_type == 'SSC':
        return ssc, (occ if visible_mask is not None else None)
    raise ValueError("eval_type must be 'SC' or 'SSC'")


def cm_to_ious(cm):
    """formating.py:4-14: per-class tp / (pred + gt - tp) of a [label][pred] confusion matrix."""
    cm = np.asarray(cm, dtype=np.float64)
    tp = np.diag(cm)
    with np.errstate(divide="ignore", invalid="ignore"):
        return list(tp / (cm.sum(0) + cm.sum(1) - tp))


class SemanticEvaluator:
    """Whole-dataset accumulation on the device: ``update`` enqueues one kernel and never synchronises;
    ``compute`` does the single device->host copy."""

    def __init__(self, num_classes=17, empty_idx=0, device="cuda"):
        self.C, self.empty_idx = num_classes, empty_idx
        self.hist = torch.zeros(4 + 2 * num_classes * num_classes, dtype=torch.int64, device=device)

    def update(self, pred, gt, visible_mask=None):
        assert pred.shape[1] == self.C
        semantic_histograms(pred, gt, visible_mask, self.empty_idx, out=self.hist, accumulate=True)

    def compute(self):
        sc, ssc, occ = (t.cpu().numpy() for t in split_histograms(self.hist, self.C))
        ious = cm_to_ious(ssc)
        return dict(SC_metric=sc, SSC_metric=ssc, SSC_occ_metric=occ, SC_IoU=cm_to_ious(sc)[1],
                    SSC_mIoU=float(np.nanmean(ious[1:])), class_ious=ious)


# ---------------------------------------------------------------- LiDAR segmentation (points_occ)
LIDARSEG_CLASSES = 16           # fast_hist_crop(..., unique_label=np.arange(16)): nuScenes lidarseg classes 1..16
_PADDING = {'zeros': 0, 'border': 1}


def fast_hist_crop(output, target, unique_label):
    """P/utils/metric_util.py:8-23: bincount of ``n * label + pred`` over 0 <= label < n (n = max(unique_label) + 2),
    cropped to rows / columns ``unique_label + 1``; numpy in, int64 numpy out."""
    output, target = np.asarray(output).flatten(), np.asarray(target).flatten()
    n = int(np.max(unique_label)) + 2
    k = (target >= 0) & (target < n)
    hist = np.bincount(n * target[k].astype(int) + output[k], minlength=n ** 2)[:n ** 2].reshape(n, n)
    idx = np.asarray(unique_label) + 1
    return hist[idx, :][:, idx]


def per_class_iu(hist):
    """metric_util.py:14-15: diag / (row sums + column sums - diag), NaN for classes absent from both."""
    hist = np.asarray(hist)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.diag(hist) / (hist.sum(1) + hist.sum(0) - np.diag(hist))


def point_mean_iou(hist):
    """``np.nanmean(per_class_iu(hist))`` of occ_head.py:376-379 with torch ops on the device (no host read): float64 0-dim."""
    h = hist.to(torch.float64)
    d = torch.diagonal(h)
    return torch.nanmean(d / (h.sum(1) + h.sum(0) - d))


def lidarseg_points(logits, points, pc_range, padding_mode='border', train=False, probs=None, labels=None, hist=None,
                    accumulate=False, label_col=None):
    """One ``coocc_lidarseg_points`` launch on the current stream: the points of ONE batch element against its logits.

    logits [C,X,Y,Z] (or [1,C,X,Y,Z]) fp32 with any strides (the channels-last ``Rows`` view of pred_c or NCDHW); points
    [N,>=4] device tensor, xyz first; pc_range: 6 numbers (xyz min, xyz max), rounded to fp32 as the reference's
    ``torch.tensor(...).type_as(...)``.  Writes whichever of ``probs`` [N,C] fp32 (eval only), ``labels`` [N] int64 and
    ``hist`` int64 [16*16] (``fast_hist_crop`` of labels against ``points[:, label_col]``; default column 3 in eval, the last
    column in train, as upstream) are given."""
    if padding_mode not in _PADDING:
        raise NotImplementedError("forward_lidarseg: padding_mode %r (border and zeros are implemented)" % (padding_mode,))
    if not logits.is_cuda:
        raise RuntimeError("co_occ_amd.evaluation runs on the HIP device only")
    if logits.dim() == 5:
        assert logits.shape[0] == 1, "one batch element per launch"
        logits = logits[0]
    assert logits.dim() == 4 and logits.dtype == torch.float32, "logits [C,X,Y,Z] fp32"
    assert points.dim() == 2 and points.shape[1] >= 4, "points [N,>=4]"
    if points.dtype != torch.float32 or points.device != logits.device or points.stride(1) != 1:
        points = points.to(device=logits.device, dtype=torch.float32).contiguous()
    C, X, Y, Z = logits.shape
    n, F = points.shape
    if label_col is None:
        label_col = F - 1 if train else 3
    rng = np.asarray(pc_range, dtype=np.float32).reshape(6)
    sc, sx, sy, sz = logits.stride()
    call("coocc_lidarseg_points", ptr(logits, strided=True), sc, sx, sy, sz, C, X, Y, Z, ptr(points, strided=True), n,
         max(points.stride(0), F) if n > 1 else F, F, int(label_col), host_f32(rng.tolist()), _PADDING[padding_mode], 1 if train else 0,
         ptr(probs, torch.float32), ptr(labels, torch.int64), 1 if accumulate else 0, ptr(hist, torch.int64))


class LidarSegEvaluator:
    """Whole-dataset lidarseg confusion matrix on the device (the sum of the per-sample ``evaluation_semantic`` matrices of
    ``COOCC_Ray.simple_test``): ``update`` enqueues one kernel and never synchronises; ``compute`` reads it back once."""

    def __init__(self, device="cuda", padding_mode='border'):
        self.padding_mode = padding_mode
        self.hist = torch.zeros(LIDARSEG_CLASSES * LIDARSEG_CLASSES, dtype=torch.int64, device=device)

    def update(self, logits, points, pc_range):
        """logits [1,17,X,Y,Z] (pred_c), points [N,>=4] with the target label in column 3."""
        lidarseg_points(logits, points, pc_range, self.padding_mode, hist=self.hist, accumulate=True)

    def add(self, hist):
        """Add a 16x16 matrix already computed (``simple_test``'s ``evaluation_semantic``, a device tensor or numpy)."""
        self.hist += torch.as_tensor(np.asarray(hist) if not torch.is_tensor(hist) else hist).reshape(-1).to(self.hist)

    def compute(self):
        return lidarseg_metrics(self.hist.cpu().numpy().reshape(LIDARSEG_CLASSES, LIDARSEG_CLASSES))


def lidarseg_metrics(hist):
    """The host half of ``LidarSegEvaluator.compute``: 16x16 matrix -> hist, per-class IoU, mIoU (nanmean)."""
    hist = np.asarray(hist, dtype=np.int64).reshape(LIDARSEG_CLASSES, LIDARSEG_CLASSES)
    ious = per_class_iu(hist)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)         # nanmean of all-NaN IoUs (an empty matrix) is NaN
        miou = float(np.nanmean(ious))
    return dict(hist=hist, class_ious=ious, mIoU=miou)


# ---------------------------------------------------------------- rendered maps (test_rendering)
# The tail of COOCC_Ray.simple_test under ``use_rendering and test_rendering`` (coocc_ray.py:626-637): PSNR of every rendered colour
# map against the camera image (compute_psnr, P/utils/save_rendered_img.py:10-20), the [rgb | gt | depth_] uint8 panels, and the
# squared depth error of save_rendered_img (:39-79) -- on the device.  Columns of the [N, 8] float64 stats block
# (include/coocc_hip.h, coocc_render_eval_stats):
RE_SQ_RGB, RE_DMIN, RE_DMAX, RE_SQ_DEPTH, RE_NVALID, RE_PSNR, RE_PSNR_MEAN = range(7)
RENDER_EVAL_SLOTS = 8


def _check_maps(rgbs, depths, gt_img, gt_depth):
    for name, t in (("rgbs", rgbs), ("depths", depths), ("gt_img", gt_img), ("gt_depth", gt_depth)):
        if t is not None and not torch.is_tensor(t):
            raise TypeError("render_eval: %s is a %s, not a tensor" % (name, type(t).__name__))
    if depths.dim() != 3:
        raise ValueError("render_eval: depths %s is not [N, H, W]" % (tuple(depths.shape),))
    N, H, W = depths.shape
    if (rgbs is None) != (gt_img is None):
        raise ValueError("render_eval: rgbs and gt_img come together (both, or neither for the depth-only variant)")
    if rgbs is not None:
        if tuple(rgbs.shape) != (N, H, W, 3):
            raise ValueError("render_eval: rgbs %s does not match depths %s ([N, H, W, 3] expected)"
                             % (tuple(rgbs.shape), tuple(depths.shape)))
        if tuple(gt_img.shape) != (N, 3, H, W):
            raise ValueError("render_eval: gt_img %s does not match the rendered maps %s: the maps are 16 fH x 16 fW and must equal "
                             "the image size ([N, 3, H, W] = %s expected)" % (tuple(gt_img.shape), tuple(rgbs.shape), (N, 3, H, W)))
    if gt_depth is not None and tuple(gt_depth.shape) != (N, H, W):
        raise ValueError("render_eval: gt_depth %s does not match depths %s" % (tuple(gt_depth.shape), tuple(depths.shape)))
    for name, t in (("rgbs", rgbs), ("depths", depths), ("gt_img", gt_img), ("gt_depth", gt_depth)):
        if t is not None and not t.is_cuda:
            raise RuntimeError("co_occ_amd.evaluation runs on the HIP device only (%s is a %s tensor; there is no CPU fallback)"
                               % (name, t.device))
    return N, H, W


def _f32c(t):
    return None if t is None else t.float().contiguous()


def render_eval_stats(rgbs, depths, gt_img, gt_depth=None, out=None):
    """``coocc_render_eval_stats`` on the current stream -> the float64 [N, 8] device block (columns RE_*).  rgbs [N,H,W,3] /
    depths [N,H,W] (the render block's maps), gt_img [N,3,H,W] (``img[0][0]``), gt_depth [N,H,W] or None; ``rgbs = gt_img = None``:
    the depth-only variant (no PSNR).  No synchronisation, no host read."""
    N, H, W = _check_maps(rgbs, depths, gt_img, gt_depth)
    rgbs, depths, gt_img, gt_depth = _f32c(rgbs), _f32c(depths), _f32c(gt_img), _f32c(gt_depth)
    if out is None:
        out = torch.empty(N, RENDER_EVAL_SLOTS, dtype=torch.float64, device=depths.device)
    need = int(load().coocc_render_eval_stats(None, None, None, None, N, H, W, None, None, 0, None))
    if need < 0:
        check(need)
    ws = torch.empty(need // 8, dtype=torch.float64, device=depths.device)
    call("coocc_render_eval_stats", ptr(rgbs), ptr(depths), ptr(gt_img), ptr(gt_depth), N, H, W, ptr(out, torch.float64), ptr(ws),
         need)
    return out


def render_panels(rgbs, depths, gt_img, block):
    """``coocc_render_panels`` -> uint8 [N, H, 3W, 3] on the device: [rgb | gt | normalised depth] per view (coocc_ray.py:629-633).
    ``block``: the stats block of the same maps (its depth extrema are read on the device)."""
    N, H, W = _check_maps(rgbs, depths, gt_img, None)
    if rgbs is None:
        raise ValueError("render_panels: the panels need rgbs and gt_img (the depth-only variant has no colour maps)")
    if block is None or tuple(block.shape) != (N, RENDER_EVAL_SLOTS):
        raise ValueError("render_panels: the stats block of render_eval_stats ([%d, 8] float64) is required" % N)
    panels = torch.empty(N, H, 3 * W, 3, dtype=torch.uint8, device=depths.device)
    call("coocc_render_panels", ptr(_f32c(rgbs)), ptr(_f32c(depths)), ptr(_f32c(gt_img)), ptr(block, torch.float64), N, H, W,
         ptr(panels))
    return panels


def render_eval_keys(block, with_rgb=True, with_depth=False, extrema=True):
    """The result keys held by a stats block -- a device tensor (the keys stay device tensors: nothing synchronises) or its
    host copy as a numpy array."""
    if torch.is_tensor(block):
        f32, i64 = (lambda a: a.to(torch.float32)), (lambda a: a.to(torch.int64))
    else:
        block = np.asarray(block, dtype=np.float64).reshape(-1, RENDER_EVAL_SLOTS)
        f32, i64 = (lambda a: a.astype(np.float32)), (lambda a: a.astype(np.int64))
    res = {}
    if with_rgb:
        res.update(psnr=f32(block[:, RE_PSNR]), psnr_mean=f32(block[0, RE_PSNR_MEAN]))
    if extrema:
        res.update(depth_min=f32(block[:, RE_DMIN]), depth_max=f32(block[:, RE_DMAX]))
    if with_depth:
        res.update(depth_sq_err=block[:, RE_SQ_DEPTH], depth_valid=i64(block[:, RE_NVALID]))
    return res


# SSIM of the colour maps, the second member of the triple save_rendered_img returns (save_rendered_img.py:22-37, 39-79).  Columns
# of the [N, 8] float64 block (include/coocc_hip.h, coocc_render_eval_ssim): the three channel means, the view's value, the mean
# over the views, the window count (H-6)(W-6), data_range:
RS_C0, RS_C1, RS_C2, RS_SSIM, RS_SSIM_MEAN, RS_COUNT, RS_RANGE = range(7)
RENDER_SSIM_SLOTS = 8
SSIM_WINDOW = 7


def _check_colour_maps(rgbs, gt_img):
    for name, t in (("rgbs", rgbs), ("gt_img", gt_img)):
        if not torch.is_tensor(t):
            raise TypeError("render_ssim: %s is a %s, not a tensor" % (name, type(t).__name__))
    if rgbs.dim() != 4 or rgbs.shape[3] != 3:
        raise ValueError("render_ssim: rgbs %s is not [N, H, W, 3]" % (tuple(rgbs.shape),))
    N, H, W = rgbs.shape[:3]
    if tuple(gt_img.shape) != (N, 3, H, W):
        raise ValueError("render_ssim: gt_img %s does not match the rendered maps %s: the maps are 16 fH x 16 fW and must equal "
                         "the image size ([N, 3, H, W] = %s expected)" % (tuple(gt_img.shape), tuple(rgbs.shape), (N, 3, H, W)))
    if H < SSIM_WINDOW or W < SSIM_WINDOW:
        raise ValueError("render_ssim: maps %s are smaller than the 7 x 7 window" % (tuple(rgbs.shape),))
    for name, t in (("rgbs", rgbs), ("gt_img", gt_img)):
        if not t.is_cuda:
            raise RuntimeError("co_occ_amd.evaluation runs on the HIP device only (%s is a %s tensor; there is no CPU fallback)"
                               % (name, t.device))
    return N, H, W


def render_ssim(rgbs, gt_img, data_range=2.0, out=None):
    """``coocc_render_eval_ssim`` on the current stream -> the float64 [N, 8] device block (columns RS_*): the SSIM of every
    rendered colour map rgbs [N,H,W,3] against gt_img [N,3,H,W] as ``skimage.metrics.structural_similarity(pred, target,
    channel_axis=-1)`` of scikit-image 0.19.3 defines it (7 x 7 uniform window, sample covariance, mean over the windows that lie
    inside the image, then over the channels).  ``data_range`` defaults to 2.0: upstream passes none, and skimage 0.19.3 then takes
    the span of the float dtype's nominal range (-1, 1) whatever the images hold, so 2.0 is what upstream's numbers are computed
    with; pass 1.0 for images in [0, 1] judged by their own range.  No synchronisation, no host read."""
    N, H, W = _check_colour_maps(rgbs, gt_img)
    data_range = float(data_range)
    if not (0.0 < data_range < float("inf")):
        raise ValueError("render_ssim: data_range %r must be positive and finite" % (data_range,))
    rgbs, gt_img = _f32c(rgbs), _f32c(gt_img)
    if out is None:
        out = torch.empty(N, RENDER_SSIM_SLOTS, dtype=torch.float64, device=rgbs.device)
    need = int(load().coocc_render_eval_ssim(None, None, N, H, W, data_range, None, None, 0, None))
    if need < 0:
        check(need)
    ws = torch.empty(need // 8, dtype=torch.float64, device=rgbs.device)
    call("coocc_render_eval_ssim", ptr(rgbs), ptr(gt_img), N, H, W, data_range, ptr(out, torch.float64), ptr(ws), need)
    return out


def render_ssim_keys(block):
    """The result keys held by an SSIM block -- a device tensor (the keys stay device tensors: nothing synchronises) or its host
    copy as a numpy array: ``ssim`` [N] fp32, ``ssim_mean`` fp32 scalar (the mean upstream returns), ``ssim_channels`` [N,3] fp64."""
    if torch.is_tensor(block):
        f32 = lambda a: a.to(torch.float32)
    else:
        block = np.asarray(block, dtype=np.float64).reshape(-1, RENDER_SSIM_SLOTS)
        f32 = lambda a: a.astype(np.float32)
    return dict(ssim=f32(block[:, RS_SSIM]), ssim_mean=f32(block[0, RS_SSIM_MEAN]), ssim_channels=block[:, RS_C0:RS_C2 + 1])


def render_eval(rgbs, depths, gt_img, gt_depth=None, panels=False, stream=None, ssim=False, data_range=2.0):
    """PSNR / depth error / comparison panels of rendered maps on the device (``stream``: a torch stream, default the current one).
    Returns device tensors: ``psnr`` [N] fp32, ``psnr_mean`` (the scalar upstream prints), ``depth_min`` / ``depth_max`` [N]; with
    ``gt_depth``: ``depth_sq_err`` [N] fp64 = sum (depth - gt_depth)^2 and ``depth_valid`` [N] int64, over gt_depth > 0; with
    ``panels=True``: ``panels`` uint8 [N,H,3W,3]; with ``ssim=True`` (colour maps required): ``ssim`` [N] fp32, ``ssim_mean`` and
    ``ssim_stats``, the raw block of ``render_ssim(rgbs, gt_img, data_range)``; always ``stats``, the raw [N, 8] block."""
    if ssim and rgbs is None:
        raise ValueError("render_eval: ssim needs rgbs and gt_img (the depth-only variant has no colour maps)")
    _check_maps(rgbs, depths, gt_img, gt_depth)
    if panels and rgbs is None:
        raise ValueError("render_eval: panels need rgbs and gt_img")
    ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    with ctx:
        block = render_eval_stats(rgbs, depths, gt_img, gt_depth)
        res = render_eval_keys(block, rgbs is not None, gt_depth is not None)
        res["stats"] = block
        if ssim:
            sblock = render_ssim(rgbs, gt_img, data_range)
            keys = render_ssim_keys(sblock)
            res.update(ssim=keys["ssim"], ssim_mean=keys["ssim_mean"], ssim_stats=sblock)
        if panels:
            res["panels"] = render_panels(rgbs, depths, gt_img, block)
    return res


class RenderEvaluator:
    """Whole-dataset accumulation of the render metrics on the device: ``update`` / ``add`` enqueue a few tiny device operations
    and never synchronise; ``summary`` reads back once.  Sums: psnr over the views, the view count, the squared depth error and
    its pixel count; once an SSIM block has been added, the per-view SSIM and its view count too."""

    def __init__(self, device="cuda"):
        self.acc = torch.zeros(4, dtype=torch.float64, device=device)       # sum psnr | views | sum sq_depth | sum n_valid
        self.acc_ssim = None                                                # sum ssim | views, from the first SSIM block on

    def add(self, block, with_rgb=True):
        """Add a stats block already computed (``render_eval(...)['stats']``; a device tensor or numpy)."""
        b = torch.as_tensor(np.asarray(block) if not torch.is_tensor(block) else block).reshape(-1, RENDER_EVAL_SLOTS).to(self.acc)
        n = float(b.shape[0])
        psnr = b[:, RE_PSNR].sum() if with_rgb else b.new_zeros(())
        self.acc += torch.stack([psnr, b.new_tensor(n if with_rgb else 0.0), b[:, RE_SQ_DEPTH].sum(), b[:, RE_NVALID].sum()])

    def add_ssim(self, block):
        """Add an SSIM block already computed (``render_ssim(...)`` / ``render_eval(..., ssim=True)['ssim_stats']``; a device
        tensor or numpy)."""
        b = torch.as_tensor(np.asarray(block) if not torch.is_tensor(block) else block).reshape(-1, RENDER_SSIM_SLOTS).to(self.acc)
        if self.acc_ssim is None:
            self.acc_ssim = torch.zeros(2, dtype=torch.float64, device=self.acc.device)
        self.acc_ssim += torch.stack([b[:, RS_SSIM].sum(), b.new_tensor(float(b.shape[0]))])

    def update(self, rgbs, depths, gt_img, gt_depth=None, ssim=False, data_range=2.0):
        self.add(render_eval_stats(rgbs, depths, gt_img, gt_depth), with_rgb=rgbs is not None)
        if ssim:
            if rgbs is None:
                raise ValueError("RenderEvaluator.update: ssim needs rgbs and gt_img")
            self.add_ssim(render_ssim(rgbs, gt_img, data_range))

    def summary(self):
        psnr, views, sq, nv = self.acc.cpu().tolist()
        res = dict(psnr_mean=psnr / views if views else float("nan"), views=int(views), depth_sq_err=sq, depth_valid=int(nv),
                   depth_mse=sq / nv if nv else float("nan"), depth_rmse=(sq / nv) ** 0.5 if nv else float("nan"))
        if self.acc_ssim is not None:
            total, n = self.acc_ssim.cpu().tolist()
            res["ssim_mean"] = total / n if n else float("nan")
        return res
