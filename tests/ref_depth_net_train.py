"""Train-mode restatement of DepthNet (the reference's ViewTransformerLSSBEVDepth.py:351-549 under ``train()``), built on the
functions of tests/ref_depth_net.py: every BatchNorm normalises with batch statistics (biased variance) and reports the running
statistics torch would leave behind (momentum, unbiased variance), the pooled ASPP branch is the broadcast map, ASPP's dropout takes
an optional given mask.  Runs under torch autograd in the dtype of its tensors: float64 is the judge, float32 the noise floor.  The
deformable convolution is the GATHER form (floor-based four corners): its offset gradient is the right derivative at integer
positions, which is what the engine's sampler backward computes (``grid_sample``'s differs there)."""
import torch
import torch.nn.functional as F

import ref_depth_net as R

SEED, ARGS, BN_CAMS, MAP = 31, (32, 32, 16, 24), 2, (8, 10)
GOLDEN_BNS = ("bn", "depth_conv.3.bn1", "depth_conv.3.global_avg_pool.2")
GOLDEN_GRADS = ("reduce_conv.0.weight", "depth_mlp.fc1.weight", "depth_conv.1.bn2.weight", "depth_conv.3.aspp4.atrous_conv.weight",
                "depth_conv.4.conv_offset.weight", "depth_conv.4.weight")


def seeded_state_dict(shapes, seed=SEED):
    """The seed rule of the train-mode fixture and tests: ``synth.random_state_dict`` over a DepthNet state_dict (only its keys and
    shapes are read) -- float32 values, so that nothing but the seed has to be stored."""
    from co_occ_amd import synth
    return {k: v.clone() for k, v in synth.random_state_dict(shapes, seed=seed).items()}


def seeded_inputs(args=ARGS, BN=BN_CAMS, H=MAP[0], W=MAP[1], seed=SEED):
    """(x [BN,Cin,H,W], mlp_input [1,BN,27], r [BN, depth + context, H, W]) as float32: the inputs and the weights of the loss
    sum(out * r)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(BN, args[0], H, W, generator=g)
    mlp = torch.randn(1, BN, 27, generator=g)
    r = torch.randn(BN, args[3] + args[2], H, W, generator=g)
    return x, mlp, r


def bn(x, sd, pre, stats=None, eps=1e-5, momentum=0.1):
    """Training-mode BatchNorm over every axis but 1; ``stats[pre]`` = (running_mean, running_var) after this step."""
    dims = [0] + list(range(2, x.dim()))
    n = x.numel() // x.shape[1]
    if n < 2:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
    mean, var = x.mean(dims), x.var(dims, unbiased=False)
    if stats is not None:
        with torch.no_grad():
            stats[pre] = (sd[pre + ".running_mean"] * (1 - momentum) + momentum * mean,
                          sd[pre + ".running_var"] * (1 - momentum) + momentum * var * (n / (n - 1)))
    shape = [1, -1] + [1] * (x.dim() - 2)
    return (x - mean.view(shape)) / torch.sqrt(var.view(shape) + eps) * sd[pre + ".weight"].view(shape) + sd[pre + ".bias"].view(shape)


def basic_block(x, sd, pre, stats):
    h = torch.relu(bn(R.conv(x, sd, pre + ".conv1", padding=1), sd, pre + ".bn1", stats))
    return torch.relu(bn(R.conv(h, sd, pre + ".conv2", padding=1), sd, pre + ".bn2", stats) + x)


def aspp(x, sd, pre, stats=None, mask=None, p=0.0):
    """``mask``: [BN, mid, H, W] of 0 / 1 (the kept elements), applied as y * mask / (1 - p)."""
    outs = [torch.relu(bn(R.conv(x, sd, pre + ".aspp1.atrous_conv"), sd, pre + ".aspp1.bn", stats))]
    for k, d in enumerate(R.DILATIONS):
        q = "%s.aspp%d" % (pre, k + 2)
        outs.append(torch.relu(bn(R.conv(x, sd, q + ".atrous_conv", padding=d, dilation=d), sd, q + ".bn", stats)))
    g = x.mean((2, 3), keepdim=True)
    g = torch.relu(bn(R.conv(g, sd, pre + ".global_avg_pool.1"), sd, pre + ".global_avg_pool.2", stats))
    outs.append(g.expand(-1, -1, x.shape[2], x.shape[3]))
    y = torch.relu(bn(R.conv(torch.cat(outs, 1), sd, pre + ".conv1"), sd, pre + ".bn1", stats))
    if mask is not None:
        y = y * mask.to(y.dtype) * (1.0 / (1.0 - p))
    return y


def depth_net(sd, x, mlp_input, stats=None, mask=None, p=0.0):
    """The train() forward in the dtype of ``x`` -> [BN, depth + context, H, W]; ``sd`` in that dtype (its tensors may require a
    gradient)."""
    v = bn(mlp_input.reshape(-1, mlp_input.shape[-1]).to(x.dtype), sd, "bn", stats)
    x = torch.relu(bn(R.conv(x, sd, "reduce_conv.0", padding=1), sd, "reduce_conv.1", stats))
    context = R.conv(x * R.gate(v, sd, "context_mlp", "context_se"), sd, "context_conv")
    h = x * R.gate(v, sd, "depth_mlp", "depth_se")
    for i in range(3):
        h = basic_block(h, sd, "depth_conv.%d" % i, stats)
    a = aspp(h, sd, "depth_conv.3", stats, mask, p)
    off = R.conv(a, sd, "depth_conv.4.conv_offset", padding=1)
    d = R.dcn(a, off, sd["depth_conv.4.weight"], form="gather")
    return torch.cat([R.conv(d, sd, "depth_conv.5"), context], 1)


def run(sd32, x, mlp_input, r, dtype, mask=None, p=0.0):
    """One training step's numbers in ``dtype``: dict(out, stats {bn: (running_mean, running_var)}, grads {key: d loss / d sd[key]},
    dx) for the loss sum(out * r)."""
    sd = {k: (v.to(dtype).clone().requires_grad_(not k.split(".")[-1].startswith(("running", "num")))
              if v.is_floating_point() else v) for k, v in sd32.items()}
    xx = x.to(dtype).clone().requires_grad_(True)
    stats = {}
    out = depth_net(sd, xx, mlp_input.to(dtype), stats, mask, p)
    (out * r.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in sd.items() if v.is_floating_point() and v.requires_grad}
    return dict(out=out.detach(), stats=stats, grads=grads, dx=xx.grad)
