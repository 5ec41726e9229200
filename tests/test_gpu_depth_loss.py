"""The DepthNet depth loss on the device (csrc/depth_loss.hip, ``losses.depth_labels_device`` / ``depth_loss_device``, the view
transformer's ``device_depth_loss``) on the GPU.  Labels and bin values are the eager function's bits; values and gradients are judged
against the float64 restatement (tests/ref_depth_loss.py) in the project's form: err(device, fp64) <= max(3 x err(eager fp32 on the
CPU, fp64), floor), floor = 2e-5 max(1, |ref|) for the value and 2e-5 max|ref grad| for the gradient tensor, no element left out.
Set COOCC_DEPTH_PARITY_OUT to a path to get the measured errors of both sides appended there (profiles/depth_loss_parity.txt)."""
import os

import numpy as np
import pytest
import torch

from co_occ_amd import core, losses as L

import ref_depth_loss as R

pytestmark = pytest.mark.gpu


def record(line):
    path = os.environ.get("COOCC_DEPTH_PARITY_OUT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def within(what, err_dev, err_eager, floor):
    record("%-44s device %.3e  eager fp32 %.3e  floor %.3e" % (what, err_dev, err_eager, floor))
    assert err_dev <= max(3.0 * err_eager, floor), "%s: device error %.3e > max(3 x eager %.3e, floor %.3e)" % (what, err_dev, err_eager, floor)


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


# ----------------------------------------------------------------------------- 1. labels
@pytest.mark.parametrize("name", list(R.FIXTURES) + list(R.LABEL_ONLY))
def test_labels_and_bin_values_are_the_eager_bits(dev, name):
    f = R.reference(name) if name in R.FIXTURES else R.label_case(name)
    evals, elab = R.eager_labels(f)
    vals, lab = L.depth_labels_device(f["gt"].to(dev), f["ds"], f["dbound"], f["D"])
    assert vals.dtype == torch.float32 and lab.dtype == torch.int32 and vals.shape == lab.shape == evals.shape
    assert bits_equal(vals.cpu(), evals), "vals differ from get_downsampled_gt_depth's"
    assert torch.equal(lab.cpu().long(), elab)
    # float64 depth maps are converted; a view that starts 4 bytes into its storage takes the kernel's unaligned route
    v2, l2 = L.depth_labels_device(f["gt"].double().to(dev), f["ds"], f["dbound"], f["D"])
    assert bits_equal(v2, vals) and torch.equal(l2, lab)
    flat = torch.empty(f["gt"].numel() + 1, device=dev)
    flat[1:] = f["gt"].to(dev).reshape(-1)
    v3, l3 = L.depth_labels_device(flat[1:].view(f["gt"].shape), f["ds"], f["dbound"], f["D"])
    assert bits_equal(v3, vals) and torch.equal(l3, lab)


# ----------------------------------------------------------------------------- 2. values and gradients against float64
def run_device(f, dev, gouts=R.GOUTS):
    leaf = f["preds"].to(dev).requires_grad_(True)                      # ``strided`` keeps its permuted strides through .to()
    assert leaf.is_contiguous() == f["preds"].is_contiguous()
    out = L.depth_loss_device(leaf, f["gt"].to(dev), f["ds"], f["dbound"], f["D"], f["weight"])
    assert out.shape == () and out.dtype == torch.float32 and out.grad_fn is not None
    grads = []
    for g in gouts:
        d, = torch.autograd.grad(out * g, leaf, retain_graph=True)
        assert d.shape == leaf.shape and d.dtype == torch.float32
        grads.append(d.double().cpu().numpy())
    return float(out.detach().double()), grads


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_values_and_gradients_against_float64(dev, name):
    f = R.reference(name)
    val, grads = run_device(f, dev)
    within("%s value" % name, abs(val - f["v64"]), abs(f["ve"] - f["v64"]), 2e-5 * max(1.0, abs(f["v64"])))
    bg = np.broadcast_to((f["labels"].numpy() == 0)[:, None], grads[0].shape)
    for k, g in enumerate(R.GOUTS):
        assert np.isfinite(grads[k]).all()
        assert not grads[k][bg].any(), "elements of non-foreground pixels must be exactly 0"
        within("%s grad gout=%g" % (name, g), np.abs(grads[k] - f["g64"][k]).max(), np.abs(f["ge"][k] - f["g64"][k]).max(),
               2e-5 * np.abs(f["g64"][k]).max())
    if name == "empty":
        assert val == 0.0 and not any(g.any() for g in grads)
    if name == "saturated":
        n_fg = int((f["labels"] > 0).sum())
        assert val >= 200.0 - 1e-3 and np.abs(grads[0]).max() == pytest.approx(1e12 / n_fg, rel=1e-6)


# ----------------------------------------------------------------------------- 3. run-to-run bits
def _loss_and_grad(f, preds, gt, gout):
    leaf = preds.clone().requires_grad_(True)
    out = L.depth_loss_device(leaf, gt, f["ds"], f["dbound"], f["D"], f["weight"])
    d, = torch.autograd.grad(out * gout, leaf)
    return out.detach().reshape(1), d


def test_two_calls_give_the_same_bits(dev):
    f = R.reference("ragged_264px_D7")
    preds, gt = f["preds"].to(dev), f["gt"].to(dev)
    a, b = _loss_and_grad(f, preds, gt, R.GOUTS[1]), _loss_and_grad(f, preds, gt, R.GOUTS[1])
    assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1]) and float(a[1].abs().max()) > 0.0


N_CALLS = 8


def test_bit_stable_beside_split_f16_gemms(dev):
    """In the manner of tests/test_gpu_occ_losses.py: calls on one stream beside split-f16 pointwise layers of a second stream give
    the bits of the run alone."""
    g = torch.Generator().manual_seed(11)
    xb = core.to_rows(torch.randn(1, 128, 100, 100, 8, generator=g).to(dev))
    pc = core.PackedConv((torch.randn(128, 128, 1, 1, 1, generator=g) * 0.05).to(dev), ksize=1, pad=0)
    f = R.reference("ragged_63px_D110")
    preds, gt = f["preds"].to(dev), f["gt"].to(dev)
    s0, s1 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    with torch.no_grad():
        core.conv_rows(xb, pc, relu=False)
    torch.cuda.synchronize()
    with torch.cuda.stream(s0):
        ref = _loss_and_grad(f, preds, gt, R.GOUTS[1])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ref[1]).all()) and float(ref[1].abs().max()) > 0.0
    got = []
    for _ in range(N_CALLS):
        with torch.cuda.stream(s1), torch.no_grad():
            for _ in range(4):
                core.conv_rows(xb, pc, relu=False)
        with torch.cuda.stream(s0):
            got.append(_loss_and_grad(f, preds, gt, R.GOUTS[1]))
    torch.cuda.synchronize()
    core.check_h2_overflow()
    bad = sum(int(not (bits_equal(ref[0], t[0]) and bits_equal(ref[1], t[1]))) for t in got)
    assert bad == 0, "device depth loss beside split-f16 GEMMs: %d of %d calls differ from the run alone" % (bad, N_CALLS)


# ----------------------------------------------------------------------------- 4. no host read
def _module_step(vt, gt, preds):
    leaf = preds.clone().requires_grad_(True)
    vt.get_depth_loss(gt, leaf).backward()
    return leaf.grad


def test_forward_and_backward_never_synchronise(dev):
    f = R.reference("ragged_264px_D7")
    vt = R.module(f).to(dev)
    preds, gt = f["preds"].to(dev), f["gt"].to(dev)
    vt.device_depth_loss = True
    _module_step(vt, gt, preds)                                         # first call: the per-stream workspace
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        g1 = _module_step(vt, gt, preds)
        vt.device_depth_loss = False
        with pytest.raises(RuntimeError):                               # the eager path reads preds[fg] and float(fg.sum()) back
            _module_step(vt, gt, preds)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().sum()) > 0


# ----------------------------------------------------------------------------- 5. detector level
def test_forward_train_with_device_depth_loss(dev):
    """The COOCC_Ray fixture tests/test_gpu_boundary.py trains, ``device_depth_loss`` off and on from the same weights: the same keys,
    ``loss_depth`` within the criterion of this file against the float64 restatement on the ``depth`` tensor the step produced, and --
    backpropagating ``loss_depth`` alone -- DepthNet's convolution weight gradient within 2e-5 max|grad| of the eager step's."""
    import test_gpu_boundary as TB
    model = TB._full_model(dev)
    model.train()
    img_inputs, points, gt = TB._sample(dev)
    vt = model.img_view_transformer
    seen, orig = {}, vt.get_depth_loss

    def spy(depth_labels, depth_preds):
        seen["gt"], seen["depth"] = depth_labels.detach().cpu(), depth_preds.detach().cpu()
        return orig(depth_labels, depth_preds)
    vt.get_depth_loss = spy
    runs = {}
    for on in (False, True):
        model.device_depth_loss = vt.device_depth_loss = on
        model.zero_grad(set_to_none=True)
        losses = model(return_loss=True, points=points, img_metas=None, img_inputs=img_inputs, gt_occ=gt,
                       generator=torch.Generator(device=dev).manual_seed(0))
        losses["loss_depth"].backward()
        w = vt.depth_net.conv.weight
        runs[on] = dict(keys=set(losses), loss=float(losses["loss_depth"].detach().double()), depth=seen["depth"], gt=seen["gt"],
                        grad=w.grad.detach().double().cpu().clone())
    assert runs[True]["keys"] == runs[False]["keys"] and "loss_depth" in runs[True]["keys"]
    _, lab = R.labels_fp32(runs[True]["gt"], vt.downsample, vt.grid_config['dbound'], vt.D)
    assert int((lab > 0).sum()) > 0
    want = {on: R.evaluate(runs[on]["depth"], lab, vt.D, vt.loss_depth_weight, torch.float64, ())[0] for on in (False, True)}   # each step's own tensor
    within("forward_train loss_depth", abs(runs[True]["loss"] - want[True]), abs(runs[False]["loss"] - want[False]),
           2e-5 * max(1.0, abs(want[True])))
    ge, gd = runs[False]["grad"], runs[True]["grad"]
    err, floor = float((gd - ge).abs().max()), 2e-5 * float(ge.abs().max())
    record("forward_train depth_net.conv.weight grad: device vs eager %.3e  floor %.3e  max|grad| %.3e" % (err, floor, float(ge.abs().max())))
    assert float(ge.abs().max()) > 0 and err <= floor, (err, floor)
