"""Float64 yardstick of the DepthNet depth loss (``ViewTransformerLiftSplatShootVoxel.get_downsampled_gt_depth`` + ``get_depth_loss``,
'bce') on the CPU, and the named fixtures tests/test_depth_loss_host.py and tests/test_gpu_depth_loss.py share.

Labels are DECIDED in float32, operation by operation as the eager code decides them (a patch minimum with exact zeros read as 1e5,
one float32 subtraction, one float32 division, a truncation): a float64 label would disagree on bin edges.  The BCE and its
gradient are evaluated in the asked dtype with the -100 clamp of ``F.binary_cross_entropy`` and the 1e-12 clamp of its backward."""
import functools

import numpy as np
import torch

GOUTS = (1.0, 0.7310586)            # upstream gradients of the loss: plain, and what loss_norm's v / (v + 1e-9) rescaling hands down


# ----------------------------------------------------------------------------- the restatement
def labels_fp32(gt, ds, dbound, D):
    """gt [B,N,H,W] -> (vals [B*N,h,w] float32, labels [B*N,h,w] int64: 0 = no foreground, 1..D = bin 0..D-1)."""
    g = gt.detach().cpu().numpy().astype(np.float32)
    B, N, H, W = g.shape
    g = g.reshape(B * N, H // ds, ds, W // ds, ds).transpose(0, 1, 3, 2, 4).reshape(B * N, H // ds, W // ds, ds * ds)
    m = np.where(g == 0.0, np.float32(1e5), g).min(-1)
    c0, step = np.float32(dbound[0] - dbound[2] / 2), np.float32(dbound[2])
    vals = ((m - c0) / step).astype(np.float32)
    lab = np.where((vals < np.float32(D + 1)) & (vals >= np.float32(0.0)), vals, np.float32(0.0)).astype(np.int64)
    return torch.from_numpy(vals), torch.from_numpy(lab)


def evaluate(preds, labels, D, weight, dtype, gouts=GOUTS):
    """-> (value, [gradient [B*N,D,h,w] per upstream scalar in ``gouts``]) as numpy float64, computed in ``dtype``."""
    p = preds.detach().cpu().to(dtype)
    fg = (labels > 0)
    y = torch.nn.functional.one_hot(labels, D + 1)[..., 1:].permute(0, 3, 1, 2).to(dtype)
    lp, l1 = torch.log(p).clamp(min=-100.0), torch.log1p(-p).clamp(min=-100.0)
    terms = -(y * lp + (1 - y) * l1) * fg[:, None].to(dtype)
    n = max(1.0, float(fg.sum()))
    value = weight * (terms.sum() / n)
    core = (p - y) / ((1 - p) * p).clamp(min=1e-12) * fg[:, None].to(dtype)
    grads = [(core * torch.tensor(g * weight, dtype=dtype) / n).double().numpy() for g in gouts]
    return float(value), grads


def module(f):
    """The eager view transformer of a fixture (CPU)."""
    from co_occ_amd.view_transformer import ViewTransformerLiftSplatShootVoxel
    H, W = f["gt"].shape[-2:]
    vt = ViewTransformerLiftSplatShootVoxel(grid_config=dict(xbound=[-8, 8, 1.0], ybound=[-8, 8, 1.0], zbound=[-2, 2, 1.0], dbound=list(f["dbound"])),
                                            data_config=dict(input_size=(H, W)), downsample=f["ds"], loss_depth_weight=f["weight"],
                                            depth_net=torch.nn.Identity())
    assert vt.D == f["D"], (vt.D, f["D"])
    return vt


def eager(f, gouts=GOUTS):
    """Today's eager ``get_depth_loss`` in float32 on the CPU -> (value, gradients) as numpy float64."""
    vt = module(f)
    leaf = f["preds"].detach().clone().requires_grad_(True)
    loss = vt.get_depth_loss(f["gt"], leaf)
    grads = [torch.autograd.grad(loss * g, leaf, retain_graph=True)[0].double().numpy() for g in gouts]
    return float(loss.detach().double()), grads


def eager_labels(f):
    """``get_downsampled_gt_depth`` on the CPU -> (vals float32 [B*N,h,w], labels int64 [B*N,h,w] = argmax + 1 where a one-hot row is
    non-zero, else 0)."""
    vals, onehot = module(f).get_downsampled_gt_depth(f["gt"])
    lab = torch.where(onehot.max(1).values > 0, onehot.argmax(1) + 1, torch.zeros((), dtype=torch.long))
    return vals, lab.view(vals.shape)


# ----------------------------------------------------------------------------- fixtures
def _probs(g, BN, D, h, w):
    return torch.from_numpy(g.normal(0.0, 2.0, (BN, D, h, w)).astype(np.float32)).softmax(1)


def _sweep(g, BN, H, W, keep, far):
    d = g.uniform(0.5, far, (1, BN, H, W)) * (g.random((1, BN, H, W)) < keep)
    return torch.from_numpy(d.astype(np.float32))


EDGE_DBOUND = (2.0, 58.0, 0.5)
# hand-placed patches of ``edges``: (image, patch row, patch column) -> (what it holds, the label it must get)
EDGE_PATCHES = {
    (0, 0, 0): ("all zero", 0),
    (0, 0, 1): ("one depth of 10.0 at its last row and column", 16),
    (0, 0, 2): ("minimum 1.8: v in [0, 1)", 0),
    (0, 1, 0): ("-1.0 beside positive depths", 0),
    (0, 1, 1): ("4.25 = 1.75 + 0.5 * 5, a bin edge", 5),
    (0, 1, 2): ("57.75, the last bin's lower edge", 112),
    (1, 0, 0): ("58.25: v = D + 1, out of range", 0),
    (1, 0, 1): ("70.0", 0),
    (1, 0, 2): ("1.75: v = 0 exactly", 0),
    (1, 1, 0): ("2.25, the first bin's lower edge", 1),
    (1, 1, 1): ("30.25 = 1.75 + 0.5 * 57 under larger depths", 57),
    (1, 1, 2): ("30.249, just below the bin edge 30.25", 56),
}


def _edges():
    g = np.random.default_rng(3)
    gt = np.zeros((1, 2, 32, 48), np.float32)
    P = lambda b, i, j: gt[0, b, 16 * i:16 * i + 16, 16 * j:16 * j + 16]
    P(0, 0, 1)[15, 15] = 10.0
    P(0, 0, 2)[...] = g.uniform(5.0, 40.0, (16, 16)) * (g.random((16, 16)) < 0.3)
    P(0, 0, 2)[7, 3] = 1.8
    P(0, 1, 0)[...] = g.uniform(5.0, 40.0, (16, 16)) * (g.random((16, 16)) < 0.3)
    P(0, 1, 0)[2, 9] = -1.0
    P(0, 1, 1)[0, 0] = 4.25
    P(0, 1, 2)[4, 12] = 57.75
    P(1, 0, 0)[9, 1] = 58.25
    P(1, 0, 1)[3, 3] = 70.0
    P(1, 0, 2)[15, 0] = 1.75
    P(1, 1, 0)[0, 15] = 2.25
    P(1, 1, 1)[...] = g.uniform(31.0, 56.0, (16, 16))
    P(1, 1, 1)[8, 8] = 30.25
    P(1, 1, 2)[5, 5] = 30.249
    P(1, 1, 2)[5, 6] = 44.0
    return dict(gt=torch.from_numpy(gt), preds=_probs(g, 2, 112, 2, 3), ds=16, dbound=EDGE_DBOUND, D=112, weight=1.0)


def _empty():
    g = np.random.default_rng(4)
    return dict(gt=torch.zeros(1, 2, 32, 32), preds=_probs(g, 2, 112, 2, 2), ds=16, dbound=EDGE_DBOUND, D=112, weight=1.0)


def _ragged_63():
    g = np.random.default_rng(5)
    return dict(gt=_sweep(g, 3, 48, 112, 0.01, 50.0), preds=_probs(g, 3, 110, 3, 7), ds=16, dbound=(1.0, 45.0, 0.4), D=110, weight=3.0)


def _ragged_264():
    g = np.random.default_rng(6)
    return dict(gt=_sweep(g, 6, 64, 176, 0.008, 9.5), preds=_probs(g, 6, 7, 4, 11), ds=16, dbound=(1.0, 8.0, 1.0), D=7, weight=0.5)


def _ds1():
    g = np.random.default_rng(7)
    return dict(gt=_sweep(g, 2, 5, 9, 0.6, 9.5), preds=_probs(g, 2, 7, 5, 9), ds=1, dbound=(1.0, 8.0, 1.0), D=7, weight=1.0)


def _ds4():
    g = np.random.default_rng(8)
    return dict(gt=_sweep(g, 2, 12, 20, 0.15, 13.0), preds=_probs(g, 2, 20, 3, 5), ds=4, dbound=(2.0, 12.0, 0.5), D=20, weight=1.0)


def _saturated():
    """Probabilities of exactly 0.0 at the label's bin and exactly 1.0 at another bin of every foreground pixel: two elements of
    100 each in the sum, gradients at the 1e-12 clamp (magnitude 1e12 x the scale)."""
    g = np.random.default_rng(9)
    f = dict(gt=_sweep(g, 1, 8, 12, 0.3, 8.5), preds=_probs(g, 1, 7, 2, 3), ds=4, dbound=(1.0, 8.0, 1.0), D=7, weight=1.0)
    _, lab = labels_fp32(f["gt"], 4, f["dbound"], 7)
    for (b, i, j) in np.argwhere(lab.numpy() > 0):
        l = int(lab[b, i, j])
        f["preds"][b, l - 1, i, j] = 0.0
        f["preds"][b, l % 7, i, j] = 1.0
    return f


def _strided():
    g = np.random.default_rng(10)
    p = torch.from_numpy(g.normal(0.0, 2.0, (2, 3, 5, 20)).astype(np.float32)).softmax(-1)        # [B*N,h,w,D] in memory
    return dict(gt=_sweep(g, 2, 12, 20, 0.15, 13.0), preds=p.permute(0, 3, 1, 2), ds=4, dbound=(2.0, 12.0, 0.5), D=20, weight=1.0)


FIXTURES = {"edges": _edges, "empty": _empty, "ragged_63px_D110": _ragged_63, "ragged_264px_D7": _ragged_264, "ragged_ds1": _ds1,
            "ragged_ds4": _ds4, "saturated": _saturated, "strided": _strided}
# label-only cases for the downsample factors no loss fixture has (each takes its own path through the label kernel's dispatch)
LABEL_ONLY = {"ds2": (2, 6, 10), "ds8": (8, 24, 40), "ds32": (32, 64, 96)}


def label_case(name):
    ds, H, W = LABEL_ONLY[name]
    g = np.random.default_rng(ds)
    return dict(gt=_sweep(g, 3, H, W, 2.0 / (ds * ds), 9.5), ds=ds, dbound=(1.0, 8.0, 1.0), D=7, weight=1.0,
                preds=torch.zeros(3, 7, H // ds, W // ds))


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fixture with its float32 labels, the float64 yardstick (v64, g64), the restatement in float32 (v32, g32) and today's eager
    float32 result on the CPU (ve, ge).  Computed once; callers do not modify it."""
    f = FIXTURES[name]()
    assert not name == "strided" or not f["preds"].is_contiguous()
    f["vals"], f["labels"] = labels_fp32(f["gt"], f["ds"], f["dbound"], f["D"])
    f["v64"], f["g64"] = evaluate(f["preds"], f["labels"], f["D"], f["weight"], torch.float64)
    f["v32"], f["g32"] = evaluate(f["preds"], f["labels"], f["D"], f["weight"], torch.float32)
    f["ve"], f["ge"] = eager(f)
    return f
