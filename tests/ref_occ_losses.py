"""The yardstick of the device OccHead losses: ``co_occ_amd/losses.py`` itself (pinned to the unmodified reference functions by
tests/golden/losses.npz), evaluated on the CPU at a chosen dtype with autograd -- float64 is the reference, float32 is the eager
path whose own error sets the tolerance.  Plus the fixtures tests/test_gpu_occ_losses.py runs and tests/test_occ_losses_host.py
vets, and the Lovasz exclusion rule (elements whose rank is not decided at fp32 precision)."""
import numpy as np
import torch

from co_occ_amd import losses as L

TERMS = ("ce", "sem_scal", "geo_scal", "lovasz")
TIE = 1e-5                     # opposite-status errors closer than this may legitimately swap ranks at fp32 precision
MAX_EXCLUDED_SHARE = 1e-3      # of the gradient tensor


def terms(logits, target, class_weights=None, empty_idx=0, dtype=torch.float64):
    """-> (leaf logits at ``dtype``, [4] values) by losses.py on the CPU.  logits [B,C,...] or [P,C], target [B,...] or [P]."""
    lg = logits.detach().cpu().to(dtype).clone().requires_grad_(True)
    t = target.detach().cpu().long()
    w = None if class_weights is None else class_weights.detach().cpu().float().to(dtype)
    vals = torch.stack([L.ce_ssc_loss(lg, t, w, ignore_index=255), L.sem_scal_loss(lg, t, ignore_index=255),
                        L.geo_scal_loss(lg, t, ignore_index=255, non_empty_idx=empty_idx),
                        L.lovasz_softmax(torch.softmax(lg, dim=1), t, ignore=255)])
    return lg, vals


def evaluate(logits, target, class_weights, empty_idx, dtype, gouts):
    """-> (values [4] float64 numpy, [one gradient per upstream vector in ``gouts``] float64 numpy in the logits' shape)."""
    lg, vals = terms(logits, target, class_weights, empty_idx, dtype)
    grads = [torch.autograd.grad((vals * g.to(dtype)).sum(), lg, retain_graph=True)[0].double().numpy() for g in gouts]
    return vals.detach().double().numpy(), grads


def head_loss(logits, gt, fine, coord, dtype=torch.float64):
    """The eight entries of ``OccHead.loss`` (unit loss weights, nuScenes class weights, empty_idx 0) restated with losses.py at ``dtype``."""
    H, W, D = logits.shape[2:]
    pooled = L.pool_labels(gt, H, W, D, 0, num_cls=logits.shape[1])
    out = {}
    _, v = terms(logits, pooled, L.nusc_class_weights(), 0, dtype)
    out.update({"loss_voxel_%s_c_0" % n: float(v[i].detach()) for i, n in enumerate(TERMS)})
    _, v = terms(fine, gt[:, coord[0], coord[1], coord[2]].long()[0], None, 0, dtype)
    out.update({"loss_voxel_%s_fine" % n: float(v[i].detach()) for i, n in enumerate(TERMS)})
    return out, pooled


def lovasz_exclusions(rows, labels):
    """bool [P,C]: the (row, class) elements of the Lovasz term whose float64 error has a neighbour of the OPPOSITE foreground status
    within ``TIE`` in the sorted order of its class (valid rows, present classes)."""
    p = torch.softmax(rows.detach().cpu().double(), 1).numpy()
    lab = labels.detach().cpu().long().numpy().reshape(-1)
    P, C = p.shape
    ex = np.zeros((P, C), bool)
    vi = np.nonzero(lab != 255)[0]
    for c in range(C):
        fg = lab[vi] == c
        if not fg.any() or fg.all():
            continue
        err = np.abs(fg - p[vi, c])
        for a, b in ((fg, ~fg), (~fg, fg)):
            other = np.sort(err[b])
            k = np.searchsorted(other, err[a])
            near = np.minimum(np.abs(other[np.clip(k, 0, len(other) - 1)] - err[a]), np.abs(other[np.clip(k - 1, 0, len(other) - 1)] - err[a]))
            ex[vi[a][near < TIE], c] = True
    return ex


# ----------------------------------------------------------------------------- fixtures (the cases.loss_inputs distribution)
PASS1_ROWS = 256                   # rows of a pass-1 tile = sorted elements of a pass-2 tile (csrc/occ_loss.hip OL_TILE)


def make(P, C, seed, mode="", empty_idx=0):
    """logits [P,C] = normal x 2; labels: classes 1..C-1, 60 % empty (0), 4 % ignore (255)."""
    g = np.random.default_rng(seed)
    logits = torch.from_numpy(g.standard_normal((P, C), dtype=np.float32) * 2)
    lab = g.integers(1, C, P).astype(np.int64)
    lab[g.random(P) < 0.6] = 0
    lab[g.random(P) < 0.04] = 255
    if P == 1:
        lab[:] = min(3, C - 1)
    if mode == "absent":               # class 3 never occurs
        lab[lab == 3] = 4
    elif mode == "single":             # one class only (plus ignored rows)
        lab[lab != 255] = 5
    elif mode == "noempty":
        lab[lab == 0] = 2
    elif mode == "onlyempty":
        lab[lab != 255] = 0
    weights = torch.from_numpy(g.random(C, dtype=np.float32) + 0.5)
    return logits, torch.from_numpy(lab), weights


# name -> dict(P, C, seed, layout in {"rows", "ld", "ncdhw", "coords"}, weights, mode).  C = 2 stays at small P: with two classes the
# errors of a column are dense in [0, 1] and 9 % of 6000 x 2 elements have an opposite-status neighbour within TIE.
FIXTURES = {}
for _P in (1, 65, PASS1_ROWS - 1, PASS1_ROWS + 1, 6000):
    FIXTURES["P%d_C17_w" % _P] = dict(P=_P, C=17, seed=1, layout="rows", weights=True, mode="")
FIXTURES.update({
    "P257_C2_ld": dict(P=PASS1_ROWS + 1, C=2, seed=2, layout="ld", weights=False, mode=""),
    "P257_C32_ld": dict(P=PASS1_ROWS + 1, C=32, seed=3, layout="ld", weights=True, mode=""),
    "P6000_C32": dict(P=6000, C=32, seed=2, layout="rows", weights=False, mode=""),
    "P65_C17_ld": dict(P=65, C=17, seed=4, layout="ld", weights=False, mode=""),
    "ncdhw_C17_w": dict(P=2 * 5 * 4 * 3, C=17, seed=5, layout="ncdhw", weights=True, mode="", grid=(2, 5, 4, 3)),
    "coords_C17": dict(P=300, C=17, seed=6, layout="coords", weights=False, mode="", volume=(6, 5, 4)),
    "absent_C17_w": dict(P=300, C=17, seed=7, layout="rows", weights=True, mode="absent"),
    "single_C17": dict(P=300, C=17, seed=8, layout="rows", weights=False, mode="single"),
    "noempty_C17_w": dict(P=300, C=17, seed=9, layout="rows", weights=True, mode="noempty"),
    "onlyempty_C17": dict(P=300, C=17, seed=10, layout="rows", weights=False, mode="onlyempty"),
})


def fixture(name):
    """-> dict(rows [P,C] logits, labels [P], weights or None, and for "coords": volume [1,X,Y,Z], coords [3,P])."""
    f = FIXTURES[name]
    logits, lab, w = make(f["P"], f["C"], f["seed"], f["mode"])
    out = dict(f, rows=logits, labels=lab, class_weights=w if f["weights"] else None)
    if f["layout"] == "coords":        # labels are read through repeated coordinates of a small volume (120 cells, 300 points)
        g = np.random.default_rng(f["seed"] + 100)
        X, Y, Z = f["volume"]
        vol = torch.from_numpy(g.integers(1, f["C"], (1, X, Y, Z)).astype(np.int64))
        vol[torch.from_numpy(g.random((1, X, Y, Z)) < 0.6)] = 0
        vol[torch.from_numpy(g.random((1, X, Y, Z)) < 0.04)] = 255
        coords = torch.from_numpy(np.stack([g.integers(0, X, f["P"]), g.integers(0, Y, f["P"]), g.integers(0, Z, f["P"])]))
        out.update(volume=vol, coords=coords, labels=vol[0, coords[0], coords[1], coords[2]])
    return out


_cache = {}


def reference(name):
    """Computed once per session and shared: dict(gouts [5,4] = the unit vectors and one random positive vector, v64 / v32 values,
    g64 / g32 gradient lists, ex = excluded rows x classes of the Lovasz term)."""
    if name not in _cache:
        f = fixture(name)
        g = np.random.default_rng(1000 + f["seed"])
        gouts = torch.cat([torch.eye(4, dtype=torch.float64), torch.from_numpy(g.random((1, 4)) + 0.5)], 0)
        v64, g64 = evaluate(f["rows"], f["labels"], f["class_weights"], 0, torch.float64, gouts)
        v32, g32 = evaluate(f["rows"], f["labels"], f["class_weights"], 0, torch.float32, gouts)
        _cache[name] = dict(f, gouts=gouts, v64=v64, g64=g64, v32=v32, g32=g32, ex=lovasz_exclusions(f["rows"], f["labels"]))
    return _cache[name]
