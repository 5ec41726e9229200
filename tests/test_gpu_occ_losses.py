"""The OccHead losses on the device (csrc/occ_loss.hip, ``losses.occ_loss_terms_device`` / ``pool_labels_device``,
``OccHead.device_losses``) on the GPU, judged against ``co_occ_amd/losses.py`` evaluated on the CPU in float64
(tests/ref_occ_losses.py) in the project's form: err(device, fp64) <= max(3 x err(eager fp32 losses.py, fp64), floor), floor =
2e-5 max(1, |ref|) for a value and 2e-5 max|ref grad| for a gradient tensor.  For the Lovasz term and the total, elements whose rank
is not decided at fp32 precision are excluded on both sides (``ref_occ_losses.lovasz_exclusions``; the host test bounds their share).
Set COOCC_OCC_PARITY_OUT to a path to get the measured errors of both sides appended there (profiles/occ_losses_parity.txt)."""
import os

import numpy as np
import pytest
import torch

import co_occ_amd as pkg
from co_occ_amd import core, losses as L
from oracle import cases

import ref_occ_losses as R

pytestmark = pytest.mark.gpu


def record(line):
    path = os.environ.get("COOCC_OCC_PARITY_OUT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def within(what, err_dev, err_eager, floor):
    record("%-44s device %.3e  eager fp32 %.3e  floor %.3e" % (what, err_dev, err_eager, floor))
    assert err_dev <= max(3.0 * err_eager, floor), "%s: device error %.3e > max(3 x eager %.3e, floor %.3e)" % (what, err_dev, err_eager, floor)


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def _head(c, dev, device_losses):
    head = pkg.build_head(dict(type='OccHead', in_channels=[32] * 2, out_channel=c["ncls"], num_level=2, soft_weights=True,
                               norm_cfg=dict(type='BN3d', requires_grad=True), cascade_ratio=c["ratio"], sample_from_voxel=True,
                               sample_from_img=True, final_occ_size=[v * c["ratio"] for v in c["coarse"]], empty_idx=0))
    head.device_losses = device_losses
    return head


# ----------------------------------------------------------------------------- 1. the head against the reference golden
def test_head_with_device_losses_matches_the_reference_golden(dev, golden):
    g = golden("losses")
    c = cases.LOSS_CASE
    logits, gt, fine, coord = cases.loss_inputs(c)
    head = _head(c, dev, True)
    h, w, d = c["coarse"]
    pooled = L.pool_labels_device(gt.to(dev), h, w, d)
    assert pooled.dtype == torch.long and np.array_equal(pooled.cpu().numpy(), g["pooled_target"])
    out = head.loss(output_voxels=[logits.to(dev)], output_coords_fine=[coord.to(dev)], output_voxels_fine=[fine.to(dev)],
                    target_voxels=gt.to(dev))
    keys = [k for k in g.files if k.startswith("loss_")]
    assert set(out) == set(keys) and len(keys) == 8
    for k in keys:
        assert abs(float(out[k]) - float(g[k])) <= 2e-5 * max(1.0, abs(float(g[k]))), (k, float(out[k]), float(g[k]))


# ----------------------------------------------------------------------------- 2. label pooling
def test_pool_labels_hand_cells(dev):
    def cell(vals):
        return int(L.pool_labels_device(torch.tensor(vals).view(1, 2, 2, 2).to(dev), 1, 1, 1)[0, 0, 0, 0])
    assert cell([0] * 8) == 0
    assert cell([3, 3, 0, 0, 0, 0, 0, 5]) == 3
    assert cell([4, 4, 2, 2, 0, 0, 0, 0]) == 2
    assert cell([4, 2, 7, 0, 0, 0, 0, 0]) == 255
    assert cell([8, 7, 6, 5, 4, 3, 2, 1]) == 1
    assert cell([255, 255, 3, 0, 0, 0, 0, 0]) == 255


@pytest.mark.parametrize("ratio", [1, 2, 4])
def test_pool_labels_bit_equal_to_the_eager_pooling(dev, ratio):
    H, W, D = 6, 5, 3
    for seed, p_empty, p_ign, hi in [(0, 0.6, 0.04, 17), (1, 0.9, 0.02, 17), (2, 0.2, 0.3, 4), (3, 0.0, 0.0, 17)]:
        g = np.random.default_rng(seed)
        vol = g.integers(1, hi, (2, H * ratio, W * ratio, D * ratio)).astype(np.int64)
        vol[g.random(vol.shape) < p_empty] = 0
        vol[g.random(vol.shape) < p_ign] = 255
        vol[0, :ratio, :ratio] = 0                                   # all-empty cells
        vol = torch.from_numpy(vol)
        want = L.pool_labels(vol, H, W, D)
        got = L.pool_labels_device(vol.to(dev), H, W, D)
        assert got.dtype == want.dtype and torch.equal(got.cpu(), want), (ratio, seed)
        assert torch.equal(L.pool_labels_device(vol.to(torch.uint8).to(dev), H, W, D, dtype=torch.uint8).cpu().long(), want)
    with pytest.raises(pkg._lib.CooccArgError, match="pool_labels"):
        L.pool_labels_device(torch.zeros(1, 18, 15, 9, dtype=torch.uint8, device=dev), 6, 5, 3)      # ratio 3


# ----------------------------------------------------------------------------- 3. values and gradients against float64
def run_device(f, dev, gouts):
    """-> (values [4] float64 numpy, [gradient [P,C] float64 numpy per upstream vector], rows labelled 255 as a bool array)."""
    P, C = f["P"], f["C"]
    cw = None if f["class_weights"] is None else f["class_weights"].to(dev)
    kw, target = {}, f["labels"].to(dev)
    if f["layout"] == "ld":                                         # rows inside a wider buffer; the padding must never be read
        leaf = torch.full((P, C + 3), float("nan"), device=dev)
        leaf[:, :C] = f["rows"].to(dev)
        leaf.requires_grad_(True)
        arg = leaf[:, :C]
        assert L.logit_rows(arg).data_ptr() == leaf.data_ptr() and L.logit_rows(arg).stride(0) == C + 3
    elif f["layout"] == "ncdhw":                                    # what forward_train hands to head.loss: a permuted view of rows
        B, H, W, D = f["grid"]
        leaf = f["rows"].to(dev).requires_grad_(True)
        arg = leaf.view(B, H, W, D, C).permute(0, 4, 1, 2, 3)
        assert not arg.is_contiguous() and L.logit_rows(arg).data_ptr() == leaf.data_ptr(), "the NCDHW view was copied"
        target = target.view(B, H, W, D)
    else:
        leaf = arg = f["rows"].to(dev).requires_grad_(True)
        if f["layout"] == "coords":
            target, kw = f["volume"].to(dev), dict(coords=f["coords"].to(dev))
    out = L.occ_loss_terms_device(arg, target, cw, 0, **kw)
    assert out.shape == (4,) and out.dtype == torch.float32
    grads = []
    for g in gouts:
        d, = torch.autograd.grad((out * g.to(dev).float()).sum(), leaf, retain_graph=True)
        if f["layout"] == "ld":
            assert float(d[:, C:].abs().sum()) == 0.0
            d = d[:, :C]
        grads.append(d.double().cpu().numpy().reshape(P, C))
    return out.detach().double().cpu().numpy(), grads


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_values_and_gradients_against_float64(dev, name):
    r = R.reference(name)
    vals, grads = run_device(r, dev, r["gouts"])
    for i, t in enumerate(R.TERMS):
        within("%s value %s" % (name, t), abs(vals[i] - r["v64"][i]), abs(r["v32"][i] - r["v64"][i]), 2e-5 * max(1.0, abs(r["v64"][i])))
    ignored = r["labels"].numpy().reshape(-1) == 255
    for k, what in enumerate(R.TERMS + ("total",)):
        keep = ~r["ex"] if what in ("lovasz", "total") else np.ones_like(r["ex"])
        g64, g32 = r["g64"][k].reshape(r["P"], r["C"]), r["g32"][k].reshape(r["P"], r["C"])
        assert np.isfinite(grads[k]).all()
        assert not grads[k][ignored].any(), "rows labelled 255 must get exactly 0"
        within("%s grad %s" % (name, what), np.abs(grads[k] - g64)[keep].max(), np.abs(g32 - g64)[keep].max(), 2e-5 * np.abs(g64).max())


# ----------------------------------------------------------------------------- 4. saturation
def test_saturated_logits_take_the_clamps(dev):
    """Logits of +-200: class 5 is present but its own rows give it no probability at all (recall and precision ratios of exactly 0 ->
    the value 100 with a zero gradient), while other rows do (sum_p > 0).  The errors tie at exactly 0 and 1, so gradients are only
    checked for being finite; the values do not depend on the order inside a tie."""
    g = np.random.default_rng(21)
    P, C = 300, 17
    lab = g.integers(0, 8, P).astype(np.int64)
    lab[g.random(P) < 0.05] = 255
    hot = np.where(lab == 5, 6, np.where(g.random(P) < 0.7, np.minimum(lab, 16), g.integers(0, 8, P)))
    hot[lab == 255] = 3
    assert (hot[lab == 5] != 5).all() and (hot == 5).any()
    rows = torch.full((P, C), -200.0)
    rows[torch.arange(P), torch.from_numpy(hot)] = 200.0
    lab_t = torch.from_numpy(lab)
    gouts = torch.cat([torch.eye(4, dtype=torch.float64), torch.tensor([[0.7, 1.3, 0.9, 1.1]], dtype=torch.float64)])
    v64, _ = R.evaluate(rows, lab_t, None, 0, torch.float64, gouts[:1])
    v32, _ = R.evaluate(rows, lab_t, None, 0, torch.float32, gouts[:1])
    assert v64[1] > 100.0 / 8                                       # a clamp at 100 is in the mean over at most 8 present classes
    f = dict(P=P, C=C, layout="rows", rows=rows, labels=lab_t, class_weights=None)
    vals, grads = run_device(f, dev, gouts)
    for i, t in enumerate(R.TERMS):
        within("saturated value %s" % t, abs(vals[i] - v64[i]), abs(v32[i] - v64[i]), 2e-5 * max(1.0, abs(v64[i])))
    assert all(np.isfinite(d).all() for d in grads)
    assert not any(d[lab == 255].any() for d in grads)


# ----------------------------------------------------------------------------- 5. ignored rows
def test_all_ignored_target(dev):
    rows, _, _ = R.make(300, 17, 31)
    lab = torch.full((300,), 255, dtype=torch.long)
    leaf = rows.to(dev).requires_grad_(True)
    out = L.occ_loss_terms_device(leaf, lab.to(dev))
    got = out.detach().double().cpu().numpy()
    _, want = R.terms(rows, lab, None, 0, torch.float32)
    want = want.detach().double().numpy()
    assert got[3] == 0.0 and want[3] == 0.0
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    assert np.isnan(got[0]) and np.isnan(got[1]) and got[2] == want[2] == 300.0
    d, = torch.autograd.grad(out[2] + out[3], leaf)
    assert float(d.abs().sum()) == 0.0


# ----------------------------------------------------------------------------- 6. run-to-run bits
def _terms_and_grad(rows, lab, cw, gout):
    leaf = rows.clone().requires_grad_(True)
    out = L.occ_loss_terms_device(leaf, lab, cw)
    d, = torch.autograd.grad((out * gout).sum(), leaf)
    return out.detach(), d


def test_two_calls_give_the_same_bits(dev):
    r = R.reference("P6000_C17_w")
    rows, lab, cw = r["rows"].to(dev), r["labels"].to(dev), r["class_weights"].to(dev)
    gout = r["gouts"][4].float().to(dev)
    a, b = _terms_and_grad(rows, lab, cw, gout), _terms_and_grad(rows, lab, cw, gout)
    assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1])


N_CALLS = 8


def test_bit_stable_beside_split_f16_gemms(dev):
    """In the manner of tests/test_gpu_sparse_wgrad_h2t.py: calls on one stream beside split-f16 pointwise layers of a second stream
    give the bits of the run alone."""
    g = torch.Generator().manual_seed(11)
    xb = core.to_rows(torch.randn(1, 128, 100, 100, 8, generator=g).to(dev))
    pc = core.PackedConv((torch.randn(128, 128, 1, 1, 1, generator=g) * 0.05).to(dev), ksize=1, pad=0)
    r = R.reference("P6000_C17_w")
    rows, lab, cw = r["rows"].to(dev), r["labels"].to(dev), r["class_weights"].to(dev)
    gout = r["gouts"][4].float().to(dev)
    s0, s1 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    with torch.no_grad():
        core.conv_rows(xb, pc, relu=False)
    torch.cuda.synchronize()
    with torch.cuda.stream(s0):
        ref = _terms_and_grad(rows, lab, cw, gout)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ref[1]).all()) and float(ref[1].abs().max()) > 0.0
    got = []
    for _ in range(N_CALLS):
        with torch.cuda.stream(s1), torch.no_grad():
            for _ in range(4):
                core.conv_rows(xb, pc, relu=False)
        with torch.cuda.stream(s0):
            got.append(_terms_and_grad(rows, lab, cw, gout))
    torch.cuda.synchronize()
    core.check_h2_overflow()
    bad = sum(int(not (bits_equal(ref[0], t[0]) and bits_equal(ref[1], t[1]))) for t in got)
    assert bad == 0, "device losses beside split-f16 GEMMs: %d of %d calls differ from the run alone" % (bad, N_CALLS)


# ----------------------------------------------------------------------------- 7. no host read
def _head_step(head, logits, gt, fine, coord):
    lg, fn = logits.clone().requires_grad_(True), fine.clone().requires_grad_(True)
    out = head.loss(output_voxels=[lg], output_coords_fine=[coord], output_voxels_fine=[fn], target_voxels=gt)
    total = None
    for k in sorted(out):
        total = out[k] if total is None else total + out[k]
    total.backward()
    return lg.grad, fn.grad


def test_forward_and_backward_never_synchronise(dev):
    c = cases.LOSS_CASE
    logits, gt, fine, coord = [t.to(dev) for t in cases.loss_inputs(c)]
    on, off = _head(c, dev, True), _head(c, dev, False)
    _head_step(on, logits, gt, fine, coord)                         # first call: per-stream buffers, the class weights' upload
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        g1, g2 = _head_step(on, logits, gt, fine, coord)
        with pytest.raises(RuntimeError):                           # the eager path reads p[valid], nonzero(present), ... back
            _head_step(off, logits, gt, fine, coord)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert bool(torch.isfinite(g1).all()) and bool(torch.isfinite(g2).all()) and float(g1.abs().sum()) > 0 and float(g2.abs().sum()) > 0


# ----------------------------------------------------------------------------- 8. detector level
def test_forward_train_with_device_occ_losses(dev):
    """The COOCC_Ray fixture tests/test_gpu_boundary.py trains, ``loss_norm`` on, ``device_occ_losses`` off and on from the same weights:
    the same keys, the eight un-normalised terms within the criterion of this file against float64 (losses.py on the CPU on the logits
    the step produced), and the first fuser convolution's weight gradient within 2e-5 max|grad| of the eager step's."""
    import test_gpu_boundary as TB
    model = TB._full_model(dev)
    model.loss_norm = True
    model.train()
    img_inputs, points, gt = TB._sample(dev)
    head = model.pts_bbox_head
    seen, orig = {}, head.loss

    def spy(**kw):
        out = orig(**kw)
        seen["args"], seen["terms"] = kw, {k: v.detach().double().cpu() for k, v in out.items()}
        return out
    head.loss = spy
    runs = {}
    for on in (False, True):
        model.device_occ_losses = head.device_losses = on
        model.zero_grad(set_to_none=True)
        losses = model(return_loss=True, points=points, img_metas=None, img_inputs=img_inputs, gt_occ=gt,
                       generator=torch.Generator(device=dev).manual_seed(0))
        sum(losses.values()).backward()
        w = model.occ_fuser.con_enc[0].weight
        runs[on] = dict(losses={k: float(v) for k, v in losses.items()}, terms=seen["terms"], grad=w.grad.detach().double().cpu().clone(),
                        args=seen["args"])
    assert set(runs[True]["losses"]) == set(runs[False]["losses"]) and len(runs[True]["terms"]) == 8
    for k, v in runs[True]["losses"].items():                       # loss_norm: every normalised term is v / (v + 1e-9)
        assert abs(v - runs[False]["losses"][k]) <= 2e-5 * max(1.0, abs(runs[False]["losses"][k])), (k, v, runs[False]["losses"][k])
    a = runs[False]["args"]
    want, _ = R.head_loss(a["output_voxels"][0].detach().cpu(), gt.cpu().long(), a["output_voxels_fine"][0].detach().cpu(),
                          a["output_coords_fine"][0].cpu(), torch.float64)
    for k in sorted(want):
        within("forward_train %s" % k, abs(float(runs[True]["terms"][k]) - want[k]), abs(float(runs[False]["terms"][k]) - want[k]),
               2e-5 * max(1.0, abs(want[k])))
    ge, gd = runs[False]["grad"], runs[True]["grad"]
    err, floor = float((gd - ge).abs().max()), 2e-5 * float(ge.abs().max())
    record("forward_train con_enc[0].weight grad: device vs eager %.3e  floor %.3e  max|grad| %.3e" % (err, floor, float(ge.abs().max())))
    assert float(ge.abs().max()) > 0 and err <= floor, (err, floor)
