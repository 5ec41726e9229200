"""Generate tests/golden/lidarseg.npz by running the UNMODIFIED reference lidarseg code (imported by path through
oracle/refshim.py) on seeded inputs.  Runs only where the reference checkout is present:

    python tools/gen_golden_lidarseg.py

Reference functions run, unmodified:
  OccHead.forward_lidarseg (P/coocc/dense_heads/occ_head.py:339-383), eval mode -> softmax [N,C], and train mode ->
      point_mean_iou (its ``.cuda()`` is patched to the identity while it runs);
  COOCC_Ray.simple_evaluation_semantic (P/coocc/detectors/coocc_ray.py:693-700) on the eval labels
      ``argmax(probs[:, 1:]) + 1`` (:557), with ``np.int`` restored for numpy 2 as oracle/gen_golden.py does;
  fast_hist_crop / per_class_iu (P/utils/metric_util.py), loaded by path into the names the two files import.  In train mode the
      hist and labels the reference builds internally are recorded at its fast_hist_crop call.

Cases: (a) a 20x20x4 grid, C = 17, about 5 000 points (about 10 % outside each face, some exactly on the faces and corners, labels
including 0, 17, 255, -1 and fractions), border padding; (b) the same points and logits, padding_mode='zeros'; (c) a batch of two
([2,17,20,20,4] logits, two point lists of 5 columns whose last one is the label), train mode.  Points whose top two probabilities
(eval) or logits (train) over classes 1..16 are closer than 1e-4 are dropped and the reference is run again on the rest, so every
label in the fixture is unambiguous; the one exception kept is an exact tie of all-zero logits (a point none of whose corners is
in bounds under zeros padding), which every implementation resolves to class 1.  Logits are multiples of 1/16 and coordinates
multiples of 1/64 m, so the fixture stays small; case (b) stores only the probability rows that differ from case (a)
(``b_probs_rows``, ``b_probs_at_rows``: points whose zeros padding drops a corner of non-zero weight).  The file is written with fixed zip timestamps:
running this again gives the same bytes."""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import refshim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lidarseg.npz")
GRID = (20, 20, 4)
C = 17
PC_RANGE = [-40.0, -40.0, -1.0, 40.0, 40.0, 5.4]
MARGIN = 1e-4


def _metric_util():
    path = os.path.join(refshim.PLUGIN, "utils", "metric_util.py")
    spec = importlib.util.spec_from_file_location("projects.mmdet3d_plugin.utils.metric_util", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def make_points(n, seed, cols=4):
    """xyz uniform over the range widened by 12.5 % of its length on each side (-> about 10 % of the points beyond each face),
    5 % of the points snapped to the faces / edges / corners; label column(s) with fractions and out-of-range values."""
    rs = np.random.RandomState(seed)
    lo, hi = np.array(PC_RANGE[:3], np.float32), np.array(PC_RANGE[3:], np.float32)
    span = hi - lo
    xyz = (lo - 0.125 * span + rs.rand(n, 3) * 1.25 * span).astype(np.float32)
    xyz = (np.round(xyz * 64.0) / 64.0).astype(np.float32)    # 1/64 m steps: exact in fp32 and compressible
    snap = rs.rand(n) < 0.05
    for k in range(3):                                  # each coordinate of a snapped point: min, max or left as is
        pick = rs.randint(0, 3, n)
        xyz[snap & (pick == 0), k] = lo[k]
        xyz[snap & (pick == 1), k] = hi[k]
    lab = rs.randint(0, 17, n).astype(np.float32)
    special = rs.rand(n)
    lab[special < 0.04] = 255.0
    lab[(special >= 0.04) & (special < 0.07)] = -1.0
    lab[(special >= 0.07) & (special < 0.10)] = 17.0
    lab[(special >= 0.10) & (special < 0.14)] += 0.6     # 3.6 -> 3, as astype(int) / .long() truncate
    lab[(special >= 0.14) & (special < 0.16)] = -0.5     # -> 0
    cols_out = [xyz, rs.rand(n, 1).astype(np.float32) * 100.0] if cols == 5 else [xyz]
    return np.concatenate(cols_out + [lab[:, None]], axis=1)


def _logits(batch, g):
    """[batch,17,20,20,4] logits with standard deviation 3 in steps of 1/16 (exact in fp32, and they compress)."""
    return torch.round(torch.randn(batch, C, *GRID, generator=g) * 48.0) / 16.0


def top2_margin(v):
    s = np.sort(v[:, 1:], axis=1)
    return s[:, -1] - s[:, -2]


def main():
    torch.set_num_threads(1)
    R = refshim.install()
    oh, cr = R["occ_head"], R["coocc_ray"]
    mu = _metric_util()
    rec = {}

    def recording_hist(output, target, unique_label):
        rec["labels"], rec["target"] = np.array(output), np.array(target)
        rec["hist"] = mu.fast_hist_crop(output, target, unique_label)
        return rec["hist"]

    oh.fast_hist_crop, oh.per_class_iu = recording_hist, mu.per_class_iu
    cr.fast_hist_crop, cr.per_class_iu = mu.fast_hist_crop, mu.per_class_iu
    if not hasattr(np, "int"):
        np.int = int
    metas = [dict(pc_range=list(PC_RANGE))]
    g = torch.Generator().manual_seed(20261015)
    out = dict(pc_range=np.array(PC_RANGE, np.float64))

    def head(padding_mode, training):
        return types.SimpleNamespace(padding_mode=padding_mode, align_corners=True, training=training)

    def run_eval(logits, pts, padding_mode):
        probs = oh.OccHead.forward_lidarseg(head(padding_mode, False), logits, [torch.from_numpy(pts)], metas)
        labels = torch.argmax(probs[:, 1:], dim=1) + 1                                    # coocc_ray.py:557
        hist = cr.COOCC_Ray.simple_evaluation_semantic(None, labels, torch.from_numpy(pts), metas)
        return probs.numpy(), labels.numpy(), hist

    def run_train(logits, pts_list):
        cuda = torch.Tensor.cuda
        torch.Tensor.cuda = lambda self, *a, **k: self
        try:
            res = oh.OccHead.forward_lidarseg(head('border', True), logits, [torch.from_numpy(p) for p in pts_list], metas)
        finally:
            torch.Tensor.cuda = cuda
        return res["point_mean_iou"], rec["labels"], rec["hist"]

    def sampled_logits(logits, pts_list, padding_mode):
        """grid_sample of the reference's own normalisation, to find near-ties in train mode (not stored)."""
        rng = torch.tensor(PC_RANGE).float()
        outs = []
        for b, p in enumerate(pts_list):
            q = ((torch.from_numpy(p)[:, :3] - rng[:3]) / (rng[3:] - rng[:3])) * 2 - 1
            q = q[:, [2, 1, 0]].view(1, 1, 1, -1, 3)
            outs.append(torch.nn.functional.grid_sample(logits[b:b + 1], q, mode='bilinear', padding_mode=padding_mode,
                                                        align_corners=True).squeeze().t().numpy())
        return outs

    # (a) + (b): one logits grid, one point set, both padding modes
    logits = _logits(1, g)
    pts = make_points(5200, 1)
    keep = np.ones(len(pts), bool)
    for mode in ("border", "zeros"):
        probs, _, _ = run_eval(logits, pts, mode)
        m = top2_margin(probs)
        zero_tie = (sampled_logits(logits, [pts], mode)[0] == 0).all(1)
        keep &= (m > MARGIN) | zero_tie
    pts = pts[keep]
    for tag, mode in (("a", "border"), ("b", "zeros")):
        probs, labels, hist = run_eval(logits, pts, mode)
        zero_tie = (sampled_logits(logits, [pts], mode)[0] == 0).all(1)
        assert ((top2_margin(probs) > MARGIN) | zero_tie).all(), tag
        out.update({tag + "_labels": labels.astype(np.int64), tag + "_hist": hist.astype(np.int64)})
        if tag == "a":
            out["a_probs"] = probs
        else:
            # zeros padding changes only the points with an out-of-bounds corner of non-zero weight: store those rows
            rows = np.nonzero((probs.view(np.int32) != out["a_probs"].view(np.int32)).any(1))[0]
            out.update(b_probs_rows=rows.astype(np.int32), b_probs_at_rows=probs[rows])
            b = out["a_probs"].copy()
            b[rows] = probs[rows]
            assert np.array_equal(b.view(np.int32), probs.view(np.int32))
        print("case (%s) %-6s %d points (%d with all corners out of bounds), %d counted in the 16x16 histogram"
              % (tag, mode, len(pts), int(zero_tie.sum()), int(hist.sum())))
    out.update(a_logits=logits.numpy(), a_points=pts)

    # (c): batch of two, train mode, 5-column points (label last)
    logits_c = _logits(2, g)
    pc = [make_points(3100, 2, cols=5), make_points(2100, 3, cols=5)]
    pc = [p[top2_margin(s) > MARGIN] for p, s in zip(pc, sampled_logits(logits_c, pc, "border"))]
    miou, labels, hist = run_train(logits_c, pc)
    assert (np.concatenate([top2_margin(s) for s in sampled_logits(logits_c, pc, "border")]) > MARGIN).all()
    out.update(c_logits=logits_c.numpy(), c_points0=pc[0], c_points1=pc[1], c_labels=np.asarray(labels, np.int64),
               c_hist=np.asarray(hist, np.int64), c_point_mean_iou=np.asarray(miou.item(), np.float64))
    print("case (c) train  %d + %d points, point_mean_iou %.12f" % (len(pc[0]), len(pc[1]), miou.item()))

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with zipfile.ZipFile(OUT, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.require(out[k], requirements="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print("wrote %s (%.0f kB)" % (OUT, os.path.getsize(OUT) / 1e3))


if __name__ == "__main__":
    main()
