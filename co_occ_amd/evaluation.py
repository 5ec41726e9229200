"""On-device evaluation -- mirror of ``COOCC_Ray.evaluation_semantic`` (P/coocc/detectors/coocc_ray.py:659-684),
``fast_hist`` (:726-730) and ``cm_to_ious`` (P/utils/formating.py:4-14).

The reference resamples the logits to the ground-truth size, takes the argmax, copies prediction and
label to the host and runs ``np.bincount`` three times per prediction.  Here one kernel produces the
SC, SSC and visible-only SSC confusion matrices on the device; ``SemanticEvaluator`` accumulates them
over a whole validation set and reads them back once.

The lidarseg metrics (``points_occ``: OccHead.forward_lidarseg, occ_head.py:339-383, and simple_evaluation_semantic,
coocc_ray.py:693-700) take the same route: ``lidarseg_points`` samples the logits at the points, labels them and builds the
16x16 ``fast_hist_crop`` matrix in one kernel; ``LidarSegEvaluator`` accumulates it over a dataset."""
import warnings

import numpy as np
import torch

from ._lib import call, host_f32, ptr

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
