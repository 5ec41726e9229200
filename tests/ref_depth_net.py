"""Torch restatement of DepthNet's eval-mode arithmetic (the reference's ViewTransformerLSSBEVDepth.py:351-549; mmdet 2.14's
BasicBlock; mmcv 1.4.0's DeformConv2dPack as DESIGN.md 10 defines it), on a state dict with the reference's keys and in the
dtype of its tensors (float64 = the judge, float32 = the fp32 noise floor).  The deformable convolution is written twice,
independently: through ``grid_sample`` at pixel coordinates and as an explicit four-corner gather with the <= -1 / >= H cut."""
import torch
import torch.nn.functional as F

DILATIONS = (6, 12, 18)
GROUPS = 4


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def bn(x, sd, pre, eps=1e-5):
    shape = [1, -1] + [1] * (x.dim() - 2)
    s = sd[pre + ".weight"] / torch.sqrt(sd[pre + ".running_var"] + eps)
    return (x - sd[pre + ".running_mean"].view(shape)) * s.view(shape) + sd[pre + ".bias"].view(shape)


def conv(x, sd, pre, **kw):
    return F.conv2d(x, sd[pre + ".weight"], sd.get(pre + ".bias"), **kw)


def tap_positions(off):
    """off [BN,18,H,W] -> (py, px) [BN,9,H,W]: tap t = 3i + j samples (y - 1 + i + off[2t], x - 1 + j + off[2t + 1])."""
    BN, _, H, W = off.shape
    ys = torch.arange(H, dtype=off.dtype).view(1, 1, H, 1)
    xs = torch.arange(W, dtype=off.dtype).view(1, 1, 1, W)
    ti = torch.arange(9).div(3, rounding_mode="floor").to(off.dtype).view(1, 9, 1, 1)
    tj = (torch.arange(9) % 3).to(off.dtype).view(1, 9, 1, 1)
    return (ys - 1 + ti) + off[:, 0::2], (xs - 1 + tj) + off[:, 1::2]


def dcn_cols_grid_sample(x, off):
    """Sampled columns [BN,C,9,H,W] through grid_sample(align_corners=True, zeros padding) at pixel coordinates."""
    BN, C, H, W = x.shape
    py, px = tap_positions(off)
    grid = torch.stack([2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1], -1)              # [BN,9,H,W,2] (x, y)
    out = F.grid_sample(x, grid.reshape(BN, 9 * H, W, 2), mode="bilinear", padding_mode="zeros", align_corners=True)
    return out.view(BN, C, 9, H, W)


def dcn_cols_gather(x, off):
    """Sampled columns [BN,C,9,H,W] as an explicit four-corner gather: 0 when the position is <= -1 or >= H (W), a corner outside
    the image contributes 0."""
    BN, C, H, W = x.shape
    py, px = tap_positions(off)
    inside = (py > -1) & (py < H) & (px > -1) & (px < W)
    y0, x0 = torch.floor(py), torch.floor(px)
    ly, lx = py - y0, px - x0
    flat = x.reshape(BN, C, H * W)
    out = torch.zeros(BN, C, 9, H, W, dtype=x.dtype)
    for dy, wy in ((0, 1 - ly), (1, ly)):
        for dx, wx in ((0, 1 - lx), (1, lx)):
            yy, xx = y0 + dy, x0 + dx
            ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long().view(BN, 1, -1).expand(BN, C, -1)
            v = torch.gather(flat, 2, idx).view(BN, C, 9, H, W)
            out = out + v * (wy * wx * ok.to(x.dtype)).unsqueeze(1)
    return out


def dcn_from_cols(cols, w, groups=GROUPS):
    """cols [BN,C,9,H,W], w [Cout, C/groups, 3, 3] -> [BN,Cout,H,W]: output channels of group g read input channels of group g."""
    BN, C, _, H, W = cols.shape
    co, cg = w.shape[0] // groups, C // groups
    wg = w.reshape(groups, co, cg, 9)
    return torch.einsum("goct,bgcthw->bgohw", wg, cols.view(BN, groups, cg, 9, H, W)).reshape(BN, groups * co, H, W)


def dcn(x, off, w, groups=GROUPS, form="gather"):
    return dcn_from_cols((dcn_cols_gather if form == "gather" else dcn_cols_grid_sample)(x, off), w, groups)


def cols_as_rows(cols, groups=GROUPS):
    """[BN,C,9,H,W] -> [groups, BN*H*W, 9 * C/groups], column t * C/groups + c: the layout of the engine's column matrices."""
    BN, C, _, H, W = cols.shape
    cg = C // groups
    return cols.view(BN, groups, cg, 9, H, W).permute(1, 0, 4, 5, 3, 2).reshape(groups, BN * H * W, 9 * cg)


def basic_block(x, sd, pre):
    h = torch.relu(bn(conv(x, sd, pre + ".conv1", padding=1), sd, pre + ".bn1"))
    return torch.relu(bn(conv(h, sd, pre + ".conv2", padding=1), sd, pre + ".bn2") + x)


def aspp(x, sd, pre):
    outs = [torch.relu(bn(conv(x, sd, pre + ".aspp1.atrous_conv"), sd, pre + ".aspp1.bn"))]
    for k, d in enumerate(DILATIONS):
        p = "%s.aspp%d" % (pre, k + 2)
        outs.append(torch.relu(bn(conv(x, sd, p + ".atrous_conv", padding=d, dilation=d), sd, p + ".bn")))
    g = x.mean((2, 3), keepdim=True)
    g = torch.relu(bn(conv(g, sd, pre + ".global_avg_pool.1"), sd, pre + ".global_avg_pool.2"))
    outs.append(g.expand(-1, -1, x.shape[2], x.shape[3]))                     # bilinear upsampling of a 1x1 map is a broadcast
    return torch.relu(bn(conv(torch.cat(outs, 1), sd, pre + ".conv1"), sd, pre + ".bn1"))


def gate(v, sd, mlp, se):
    v = F.linear(torch.relu(F.linear(v, sd[mlp + ".fc1.weight"], sd[mlp + ".fc1.bias"])), sd[mlp + ".fc2.weight"], sd[mlp + ".fc2.bias"])
    v = v[..., None, None]
    return torch.sigmoid(conv(torch.relu(conv(v, sd, se + ".conv_reduce")), sd, se + ".conv_expand"))


def depth_conv(x, sd, pre="depth_conv", form="gather"):
    for i in range(3):
        x = basic_block(x, sd, "%s.%d" % (pre, i))
    x = aspp(x, sd, pre + ".3")
    off = conv(x, sd, pre + ".4.conv_offset", padding=1)
    x = dcn(x, off, sd[pre + ".4.weight"], form=form)
    return conv(x, sd, pre + ".5")


def depth_net(sd, x, mlp_input, form="gather"):
    """forward of :540-549 in the dtype of ``x`` -> [BN, depth + context, H, W]."""
    sd = cast(sd, x.dtype)
    v = bn(mlp_input.reshape(-1, mlp_input.shape[-1]).to(x.dtype), sd, "bn")
    x = torch.relu(bn(conv(x, sd, "reduce_conv.0", padding=1), sd, "reduce_conv.1"))
    context = conv(x * gate(v, sd, "context_mlp", "context_se"), sd, "context_conv")
    depth = depth_conv(x * gate(v, sd, "depth_mlp", "depth_se"), sd, form=form)
    return torch.cat([depth, context], 1)
