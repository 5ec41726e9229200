"""Training-mode restatement of upstream's ``SparseEncoderHD`` for the tests of ``lidar_hd``'s differentiable forward.  TEST
INFRASTRUCTURE ONLY.

The layer plan, the masked dense convolutions and the dense scatter are those of tests/ref_sparse_hd.py; what changes is the norm:
nn.BatchNorm1d under ``train()`` on the [N, C] rows of the ACTIVE voxels -- batch mean and BIASED variance for the normalisation,
the UNBIASED variance (n / (n - 1)) in the running update, ``running = (1 - momentum) * running + momentum * batch``,
``num_batches_tracked += 1`` (torch/nn/modules/batchnorm.py, torch.nn.functional.batch_norm).  Everything is plain differentiable
torch, so autograd in float64 gives ``dfeats`` and every parameter's gradient; the same code in float32 gives the fp32 noise floor
of a fixture (``evaluate``)."""
import torch
import torch.nn.functional as F

from ref_sparse_hd import DEFAULTS, conv_layer, layer_plan, to_dense


def norm_cfg_of(cfg):
    return dict(DEFAULTS["norm_cfg"], **cfg.get("norm_cfg", {}))


def bn_rows_train(x, mask, sd, prefix, eps, momentum, new_stats, counts):
    """nn.BatchNorm1d.train() on the active rows of the dense volume x [1,C,Z,Y,X]; records the updated running statistics."""
    v = lambda k: sd["%s.%s" % (prefix, k)].view(1, -1, 1, 1, 1)
    m = mask.to(x.dtype)
    n = int(mask.sum())
    counts[prefix] = n
    if n == 0:                                   # no active row: nothing to normalise (torch itself refuses an empty batch)
        return x * m + (v("weight").sum() + v("bias").sum()) * 0
    dims = (0, 2, 3, 4)
    mean = (x * m).sum(dims, keepdim=True) / n
    var = (((x - mean) ** 2) * m).sum(dims, keepdim=True) / n
    with torch.no_grad():
        unbiased = var * (n / max(n - 1, 1))
        new_stats[prefix + ".running_mean"] = (1 - momentum) * sd[prefix + ".running_mean"] + momentum * mean.flatten()
        new_stats[prefix + ".running_var"] = (1 - momentum) * sd[prefix + ".running_var"] + momentum * unbiased.flatten()
        new_stats[prefix + ".num_batches_tracked"] = sd[prefix + ".num_batches_tracked"] + 1
    return ((x - mean) / torch.sqrt(var + eps) * v("weight") + v("bias")) * m


def encoder_forward_train(sd, cfg, feats, coors, momentum=None):
    """``ref_sparse_hd.encoder_forward`` under train(): sd = tensors of one dtype (leaves with requires_grad to differentiate),
    feats [M, Cin] -> (dense [1,C,Z,Y,X], final mask, updated running statistics {key: tensor}, {norm prefix: active rows})."""
    nc = norm_cfg_of(cfg)
    eps, momentum = nc.get("eps", 1e-5), nc.get("momentum", 0.1) if momentum is None else momentum
    c = torch.as_tensor(coors).long().reshape(-1, 3)
    x = _scatter(feats, c, cfg["sparse_shape"])
    _, mask = to_dense(feats.detach(), coors, cfg["sparse_shape"])
    new_stats, counts = {}, {}
    for kind, pre, cin, cout, k, s, p in layer_plan(cfg):
        if kind == "block":
            h, _ = conv_layer(x, mask, sd[pre + ".conv1.weight"], k, s, p, True)
            h = F.relu(bn_rows_train(h, mask, sd, pre + ".bn1", eps, momentum, new_stats, counts))
            h, _ = conv_layer(h, mask, sd[pre + ".conv2.weight"], k, s, p, True)
            x = F.relu(bn_rows_train(h, mask, sd, pre + ".bn2", eps, momentum, new_stats, counts) + x) * mask
        else:
            x, mask = conv_layer(x, mask, sd[pre + ".0.weight"], k, s, p, kind == "subm")
            x = F.relu(bn_rows_train(x, mask, sd, pre + ".1", eps, momentum, new_stats, counts))
    return x, mask, new_stats, counts


def _scatter(feats, c, shape):
    """Differentiable ``to_dense``: feats [M, C] at (z, y, x) = c -> [1, C, D, H, W]."""
    D, H, W = shape
    flat = feats.new_zeros(D * H * W, feats.shape[1])
    flat = flat.index_put(((c[:, 0] * H + c[:, 1]) * W + c[:, 2],), feats)
    return flat.view(D, H, W, -1).permute(3, 0, 1, 2).unsqueeze(0)


def evaluate(sd, cfg, feats, coors, gout, dtype, momentum=None):
    """One training step's quantities in ``dtype``: dict(y, mask, dfeats, '<param key>.grad' ..., running statistics, counts) for
    the loss sum(y * gout)."""
    leaves = {k: (v.detach().to(dtype).clone().requires_grad_(not k.endswith(("running_mean", "running_var"))) if v.is_floating_point()
                  else v.clone()) for k, v in sd.items()}
    f = torch.as_tensor(feats).detach().to(dtype).clone().requires_grad_()
    y, mask, stats, counts = encoder_forward_train(leaves, cfg, f, coors, momentum)
    (y * gout.to(dtype)).sum().backward()
    out = dict(y=y.detach(), mask=mask, dfeats=f.grad, counts=counts)
    for k, v in leaves.items():
        if v.is_floating_point() and v.requires_grad:
            out[k + ".grad"] = v.grad if v.grad is not None else torch.zeros_like(v)
    out.update(stats)
    return out
