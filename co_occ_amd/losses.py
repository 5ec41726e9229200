"""Occupancy losses of ``OccHead.loss`` (P/coocc/dense_heads/occ_head.py:265-337): class-weighted cross-entropy, the
semantic / geometric scene-class affinity losses (P/utils/semkitti.py:65-149) and Lovasz-softmax
(P/coocc/dense_heads/lovasz_softmax.py:156-203), plus the majority-vote label pooling of ``loss_voxel`` (:269-281).

The functions below are host-side eager torch on the logits the HIP path produced, exactly as upstream; ``occ_loss_terms_device`` /
``pool_labels_device`` at the end of the file compute the same numbers and their gradient in HIP kernels (csrc/occ_loss.hip, opt-in
through ``OccHead.device_losses``); ``depth_labels_device`` / ``depth_loss_device`` after them are the device form of the view
transformer's DepthNet supervision (csrc/depth_loss.hip, opt-in through its ``device_depth_loss``).  (The losses are a few reductions over
80 k coarse voxels / <= 8 x fine_topk fine points; they are downstream of the hot path)  Restated in
vectorised form -- one softmax, one one-hot matmul for all per-class sums, one column-wise sort for all present classes
-- instead of the reference's per-class Python loops; the arithmetic (sums, ratios, -log clamped at 100) is the same, so
values agree to float rounding (tests/golden/losses.npz, generated from the unmodified reference functions)."""
import numpy as np
import torch
import torch.nn.functional as F

# voxel counts per nuScenes-Occupancy class (data: P/utils/nusc_param.py:10-12), class_weights = 1 / log(freq + 1e-3)
NUSC_CLASS_FREQUENCIES = np.array([2242961742295, 25985376, 1561108, 28862014, 196106643, 15920504, 2158753, 26539491, 4004729,
                                   34838681, 75173306, 2255027978, 50959399, 646022466, 869055679, 1446141335, 1724391378])


def nusc_class_weights():
    return torch.from_numpy(1 / np.log(NUSC_CLASS_FREQUENCIES + 0.001))


def _bce_to_one(x):
    """F.binary_cross_entropy(x, ones) = -log(x) with torch's clamp of the log at -100.  Written with a substituted
    argument so that x == 0 gives the value 100 and a ZERO gradient (0 * inf would be NaN; torch's own backward clamps the
    denominator at 1e-12 instead -- a degenerate case, e.g. a present class that receives no probability mass at all)."""
    ok = x > 1e-43
    return torch.where(ok, -torch.log(torch.where(ok, x, torch.ones_like(x))), torch.full_like(x, 100.0))


def _flat(pred, target):
    """[B,C,...] logits + [B,...] labels -> ([P,C], [P])."""
    C = pred.shape[1]
    return pred.reshape(pred.shape[0], C, -1).permute(0, 2, 1).reshape(-1, C), target.reshape(-1)


def ce_ssc_loss(pred, target, class_weights=None, ignore_index=255):
    """semkitti.py:140-149."""
    return F.cross_entropy(pred, target.long(), weight=class_weights, ignore_index=ignore_index, reduction="mean")


def geo_scal_loss(pred, ssc_target, ignore_index=255, non_empty_idx=0):
    """semkitti.py:65-90: precision / recall / specificity of the occupied-vs-empty split, each through BCE against 1."""
    logits, t = _flat(pred, ssc_target)
    p = F.softmax(logits, dim=1)
    valid = t != ignore_index
    empty = p[:, non_empty_idx][valid]
    nonempty = 1 - empty
    tgt = (t != non_empty_idx)[valid].float()
    eps = 1e-5
    inter = (tgt * nonempty).sum()
    precision = inter / (nonempty.sum() + eps)
    recall = inter / (tgt.sum() + eps)
    spec = ((1 - tgt) * empty).sum() / ((1 - tgt).sum() + eps)
    return _bce_to_one(precision) + _bce_to_one(recall) + _bce_to_one(spec)


def sem_scal_loss(pred, ssc_target, ignore_index=255):
    """semkitti.py:93-137: for every class present in the target, -log precision (if any probability mass), -log recall,
    -log specificity (if any negative), averaged over the present classes."""
    logits, t = _flat(pred, ssc_target)
    valid = t != ignore_index
    p = F.softmax(logits, dim=1)[valid]                       # [P,C]
    t = t[valid].long()
    C = p.shape[1]
    onehot = F.one_hot(t.clamp(max=C - 1), C).to(p.dtype) * (t < C).unsqueeze(1)
    n_t = onehot.sum(0)                                       # voxels of class i
    nom = (p * onehot).sum(0)
    sum_p = p.sum(0)
    neg = p.shape[0] - n_t                                    # sum(1 - completion_target)
    spec_num = ((1 - p) * (1 - onehot)).sum(0)
    present = n_t > 0
    zero = torch.zeros_like(nom)
    l_prec = torch.where(sum_p > 0, _bce_to_one(nom / sum_p.clamp(min=1e-38)), zero)
    l_rec = _bce_to_one(nom / n_t.clamp(min=1))
    l_spec = torch.where(neg > 0, _bce_to_one(spec_num / neg.clamp(min=1)), zero)
    per_class = torch.where(present, l_prec + l_rec + l_spec, zero)
    return per_class.sum() / present.sum()


def lovasz_softmax(probas, labels, ignore=None):
    """lovasz_softmax.py:156-203 with classes='present', per_image=False: mean over present classes of
    <sorted errors, Lovasz gradient>; all present classes are sorted in one column-wise sort."""
    if probas.dim() > 2:
        probas, labels = _flat(probas, labels)
    if ignore is not None:
        valid = labels != ignore
        probas, labels = probas[valid], labels[valid]
    if probas.numel() == 0:
        return probas.sum() * 0.
    C = probas.shape[1]
    labels = labels.long()
    present = torch.bincount(labels.clamp(max=C), minlength=C + 1)[:C] > 0
    cls = torch.nonzero(present).flatten()
    fg = (labels.unsqueeze(1) == cls.unsqueeze(0)).to(probas.dtype)          # [P, Cp]
    errors = (fg - probas[:, cls]).abs()
    errors_sorted, perm = torch.sort(errors, 0, descending=True)
    fg_sorted = torch.gather(fg, 0, perm)
    gts = fg_sorted.sum(0, keepdim=True)
    inter = gts - fg_sorted.cumsum(0)
    union = gts + (1 - fg_sorted).cumsum(0)
    jac = 1. - inter / union
    jac = torch.cat([jac[:1], jac[1:] - jac[:-1]], 0)                        # lovasz_grad (:21-33)
    return (errors_sorted * jac).sum(0).mean()


def pool_labels(target_voxels, H, W, D, empty_idx=0, num_cls=17):
    """Label volume [B,rH,rW,rD] -> [B,H,W,D] by the majority vote of ``loss_voxel`` (occ_head.py:269-281): a cell whose
    children are all empty stays empty; otherwise the most frequent NON-empty label wins (smallest label on ties); when no
    non-empty label occurs twice the upstream trick (empty children get unique negative ids, torch.mode returns the
    smallest mode) yields 255 as soon as one child is empty and the smallest label otherwise."""
    B = target_voxels.shape[0]
    ratio = target_voxels.shape[1] // H
    if ratio == 1:
        return target_voxels.long()
    t = target_voxels.reshape(B, H, ratio, W, ratio, D, ratio).permute(0, 1, 3, 5, 2, 4, 6).reshape(B, H, W, D, ratio ** 3).long()
    # labels are 0 .. num_cls-1 and 255 (ignore): 255 takes the extra bin num_cls, which keeps it the LARGEST label in the
    # "smallest label on ties" order (a [.., 256] histogram was 82 MB per step at 100x100x8)
    nlab = num_cls + 1
    counts = torch.zeros(B, H, W, D, nlab, dtype=torch.int32, device=t.device)
    counts.scatter_add_(-1, torch.where(t == 255, torch.full_like(t, num_cls), t.clamp(0, num_cls - 1)), torch.ones_like(t, dtype=torch.int32))
    n_empty = counts[..., empty_idx].clone()
    all_empty = t.sum(-1) == empty_idx
    counts[..., empty_idx] = 0
    m, arg = counts.max(-1)                                   # first (= smallest label) maximum
    arg = torch.where(arg == num_cls, torch.full_like(arg, 255), arg)
    out = torch.where((m == 1) & (n_empty > 0), torch.full_like(arg, 255), arg)
    return torch.where(all_empty, torch.full_like(arg, empty_idx), out).long()


# ----------------------------------------------------------------------------- the same terms on the device (csrc/occ_loss.hip)
def logit_rows(logits):
    """[B,C,...] or [P,C] logits -> the [P,C] float32 rows the kernels read IN PLACE: unit column stride, row stride ld >= C.  The
    NCDHW tensor ``forward_train`` hands to ``OccHead.loss`` is a permuted view of exactly such rows and comes back as a view (no
    copy); any other layout goes through ``.contiguous()``."""
    C = logits.shape[1]
    rows = logits.movedim(1, -1).reshape(-1, C) if logits.dim() > 2 else logits
    if rows.dtype != torch.float32:
        rows = rows.float()
    if (C > 1 and rows.stride(1) != 1) or (rows.shape[0] > 1 and rows.stride(0) < C):
        rows = rows.contiguous()
    return rows


def _device_only(name, *tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            from ._lib import CooccError
            raise CooccError("%s runs on the GPU only; got a %s tensor (the eager functions of co_occ_amd.losses take CPU tensors)"
                             % (name, t.device))


def _labels_u8(t):
    return (t if t.dtype == torch.uint8 else t.to(torch.uint8)).contiguous()


def occ_loss_terms_device(logits, target, class_weights=None, empty_idx=0, ignore_index=255, coords=None):
    """The four unweighted terms (ce_ssc_loss, sem_scal_loss, geo_scal_loss, lovasz_softmax of the softmax) of ``logits`` ([B,C,...] or
    [P,C]) against ``target`` ([B,...] or [P] labels, ``ignore_index`` = ignore) as ONE differentiable [4] tensor: HIP kernels forward
    and backward, no host read, bitwise reproducible.  ``coords`` ([3,P] int64): ``target`` is the label volume [B,X,Y,Z] and row i is
    judged against ``target[0, coords[0,i], coords[1,i], coords[2,i]]`` (OccHead.loss_point's gather, done in the kernel)."""
    _device_only("occ_loss_terms_device", logits, target, class_weights, coords)
    if ignore_index != 255:
        raise ValueError("occ_loss_terms_device: ignore_index is 255 (uint8 labels), got %r" % (ignore_index,))
    from .autograd import OccLossFn
    rows = logit_rows(logits)
    if class_weights is not None:
        class_weights = class_weights.float().contiguous()
        if class_weights.numel() != rows.shape[1]:
            raise ValueError("occ_loss_terms_device: %d class weights for %d classes" % (class_weights.numel(), rows.shape[1]))
    if coords is not None:
        labels, coords = _labels_u8(target[0]), coords.long().contiguous()
        if coords.shape != (3, rows.shape[0]):
            raise ValueError("occ_loss_terms_device: coords %s for %d rows" % (tuple(coords.shape), rows.shape[0]))
    else:
        labels = _labels_u8(target.reshape(-1))
        if labels.numel() != rows.shape[0]:
            raise ValueError("occ_loss_terms_device: %d labels for %d rows" % (labels.numel(), rows.shape[0]))
    return OccLossFn.apply(rows, labels, coords, class_weights, empty_idx)


def pool_labels_device(target_voxels, H, W, D, empty_idx=0, num_cls=17, dtype=torch.long):
    """``pool_labels`` as one HIP kernel (a thread per coarse cell): the same integers.  Ratios 1, 2 and 4."""
    _device_only("pool_labels_device", target_voxels)
    from ._lib import call, ptr
    B = target_voxels.shape[0]
    ratio = target_voxels.shape[1] // H
    vol = _labels_u8(target_voxels)
    if tuple(vol.shape) != (B, H * ratio, W * ratio, D * ratio):
        raise ValueError("pool_labels_device: volume %s is not %d x the grid (%d, %d, %d)" % (tuple(vol.shape), ratio, H, W, D))
    out = torch.empty(B, H, W, D, device=vol.device, dtype=torch.uint8)
    call("coocc_pool_labels", ptr(vol), B, H, W, D, ratio, int(empty_idx), int(num_cls), ptr(out))
    return out if dtype == torch.uint8 else out.to(dtype)


# ----------------------------------------------------------------------------- the DepthNet depth loss on the device (csrc/depth_loss.hip)
def _depth_maps(name, gt_depths, downsample):
    """[B,N,H,W] (or [B*N,H,W]) depth maps -> the contiguous float32 [B*N,H,W] tensor the label kernel reads."""
    if gt_depths.dim() not in (3, 4):
        raise ValueError("%s: gt_depths %s is not [B,N,H,W]" % (name, tuple(gt_depths.shape)))
    H, W = gt_depths.shape[-2:]
    if H % downsample or W % downsample:
        raise ValueError("%s: depth maps %d x %d are not a multiple of downsample = %d" % (name, H, W, downsample))
    return gt_depths.reshape(-1, H, W).float().contiguous()


def depth_labels_device(gt_depths, downsample, dbound, D):
    """``ViewTransformerLiftSplatShootVoxel.get_downsampled_gt_depth`` as one HIP kernel: [B,N,H,W] metric depth -> (``vals`` [B*N,h,w]
    float32, the eager function's bits; ``labels`` [B*N,h,w] int32: 0 = no foreground, 1..D = the one-hot's column + 1).  ``dbound`` =
    ``grid_config['dbound']``; ``downsample``: a power of two from 1 to 32."""
    _device_only("depth_labels_device", gt_depths)
    from ._lib import call, ptr
    ds = int(downsample)
    g = _depth_maps("depth_labels_device", gt_depths, ds)
    BN, H, W = g.shape
    vals = torch.empty(BN, H // ds, W // ds, device=g.device, dtype=torch.float32)
    labels = torch.empty(BN, H // ds, W // ds, device=g.device, dtype=torch.int32)
    # the eager expression subtracts the Python (double) number dbound[0] - dbound[2] / 2 and divides by dbound[2], each as a float32
    call("coocc_depth_labels", ptr(g), BN, H, W, ds, float(dbound[0] - dbound[2] / 2), float(dbound[2]), int(D), ptr(vals), ptr(labels))
    return vals, labels


def depth_loss_device(depth_preds, gt_depths, downsample, dbound, D, weight):
    """``get_depth_loss`` ('bce') of ``depth_preds`` [B*N,D,h,w] against the depth maps ``gt_depths`` [B,N,H,W] as ONE differentiable
    0-dim float32 tensor: HIP kernels forward (3 launches) and backward (1), no host read, bitwise reproducible.  Non-contiguous
    ``depth_preds`` and non-float32 ``gt_depths`` are converted; the gradient has ``depth_preds``' shape."""
    _device_only("depth_loss_device", depth_preds, gt_depths)
    from .autograd import DepthLossFn
    _, labels = depth_labels_device(gt_depths, downsample, dbound, D)
    if depth_preds.dim() != 4 or tuple(depth_preds.shape) != (labels.shape[0], int(D), labels.shape[1], labels.shape[2]):
        raise ValueError("depth_loss_device: depth_preds %s for labels %s and D = %d" % (tuple(depth_preds.shape), tuple(labels.shape), D))
    return DepthLossFn.apply(depth_preds, labels, float(weight))
