"""Restatement of upstream's ``SparseEncoderHD`` (P/coocc/voxel_encoder/sparse_encoder_hd.py) as masked dense torch convolutions,
evaluated in float64, and the rule-book forms it is checked against.  TEST INFRASTRUCTURE ONLY.

spconv v1 (mmdetection3d/mmdet3d/ops/spconv) cannot be built here -- its tensorview.h includes CUDA headers even for the CPU
functors (oracle/ref_lidar.py) -- so no fixture comes from the unmodified module.  The layer semantics are restated from:
  * sparse_encoder_hd.py:32-100, 136-210   the layer plan (``layer_plan``) and the state_dict keys;
  * sparse_block.py:103-121, 124-186       SparseBasicBlock / make_sparse_convmodule (bias-free conv, BN1d, ReLU);
  * spconv/conv.py:68-77, 98-99, 126-145   per-axis kernel / stride / padding lists, weight [kd,kh,kw,Cin,Cout], the 1x1x1 GEMM;
  * spconv/ops.py:20-31                     get_conv_output_size per axis;
  * spconv/include/spconv/spconv_ops.h:76-79  SubMConv3d: stride 1, padding k // 2 whatever the layer was given;
  * spconv/include/spconv/geometry.h:25-86  getValidOutPos (``valid_out_pos``), :144-192 an output is active iff an input reaches it.
Masked-dense form: active set of a SparseConv3d = ``max_pool3d`` of the mask with the same per-axis geometry; BN1d in eval mode
acts on the active rows, so the dense result is multiplied by the mask after it."""
import itertools

import numpy as np
import torch
import torch.nn.functional as F


def triple(v):
    return tuple(int(a) for a in v) if isinstance(v, (list, tuple)) else (int(v),) * 3


def out_size(shape, k, s, p):
    """ops.py:20-31 (dilation 1)."""
    return tuple((n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip(shape, k, s, p))


DEFAULTS = dict(order=('conv', 'norm', 'act'), norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01), base_channels=16, output_channels=128,
                encoder_channels=((16, ), (32, 32, 32), (64, 64, 64), (64, 64, 64)),
                encoder_paddings=((1, ), (1, 1, 1), (1, 1, 1), ((0, 1, 1), 1, 1)), encoder_strides=(2, 2, 2, 1),
                block_type='conv_module')               # sparse_encoder_hd.py:32-46


def layer_plan(cfg):
    """[(kind, key prefix, cin, cout, kernel, stride, padding)], kind in subm | down | block | out (sparse_encoder_hd.py:66-100,
    159-209).  A block's prefix carries conv1 / bn1 / conv2 / bn2, a conv module's 0 (conv) / 1 (norm)."""
    c = dict(DEFAULTS, **{k: v for k, v in cfg.items() if k != "type"})
    one = (1, 1, 1)
    plan = [("subm", "conv_input", c["in_channels"], c["base_channels"], (3, 3, 3), one, one)]
    cin = c["base_channels"]
    chans = c["encoder_channels"]
    for i, blocks in enumerate(chans):
        for j, cout in enumerate(tuple(blocks)):
            pad = tuple(c["encoder_paddings"][i])[j]
            pre = "encoder_layers.encoder_layer%d.%d" % (i + 1, j)
            if i != 0 and j == 0 and c["block_type"] == 'conv_module':
                plan.append(("down", pre, cin, cout, (3, 3, 3), triple(c["encoder_strides"][i]), triple(pad)))
            elif c["block_type"] == 'basicblock':
                if j == len(blocks) - 1 and i != len(chans) - 1:
                    plan.append(("down", pre, cin, cout, (3, 3, 3), triple(c["encoder_strides"][i]), triple(pad)))
                else:
                    plan.append(("block", pre, cout, cout, (3, 3, 3), one, one))
            else:
                plan.append(("subm", pre, cin, cout, (3, 3, 3), one, one))
            cin = cout
    plan.append(("out", "conv_out", cin, c["output_channels"], one, one, (0, 0, 0)))
    return plan


def expected_state_dict_shapes(cfg):
    """key -> shape of upstream's module built from ``cfg``: conv weights [kd,kh,kw,Cin,Cout] without bias (conv.py:98-103),
    nn.BatchNorm1d's five entries per norm."""
    out = {}

    def bn(prefix, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            out["%s.%s" % (prefix, k)] = (c,)
        out[prefix + ".num_batches_tracked"] = ()
    for kind, pre, cin, cout, k, s, p in layer_plan(cfg):
        if kind == "block":
            for n in ("1", "2"):
                out["%s.conv%s.weight" % (pre, n)] = (3, 3, 3, cout, cout)
                bn("%s.bn%s" % (pre, n), cout)
        else:
            out[pre + ".0.weight"] = tuple(k) + (cin, cout)
            bn(pre + ".1", cout)
    return out


# ----------------------------------------------------------------------------- masked dense layers
def to_dense(feats, coors, shape):
    D, H, W = shape
    feats = torch.as_tensor(feats)
    vol = torch.zeros(1, feats.shape[1], D, H, W, dtype=feats.dtype)
    mask = torch.zeros(1, 1, D, H, W, dtype=torch.bool)
    c = torch.as_tensor(np.asarray(coors)).long().reshape(-1, 3)
    vol[0, :, c[:, 0], c[:, 1], c[:, 2]] = feats.t()
    mask[0, 0, c[:, 0], c[:, 1], c[:, 2]] = True
    return vol, mask


def conv_layer(x, mask, w_v1, k, s, p, subm):
    """One spconv v1 convolution on the dense volume: weight [kd,kh,kw,Cin,Cout] -> (y, mask of the outputs)."""
    w = w_v1.to(x.dtype).permute(4, 3, 0, 1, 2).contiguous()
    if subm:
        return F.conv3d(x, w, padding=tuple(kk // 2 for kk in k)) * mask, mask
    if tuple(k) == (1, 1, 1):                                     # conv.py:134-145: the same indices
        return F.conv3d(x, w) * mask, mask
    newmask = F.max_pool3d(mask.to(x.dtype), tuple(k), tuple(s), tuple(p)) > 0
    return F.conv3d(x, w, stride=tuple(s), padding=tuple(p)) * newmask, newmask


def bn_rows(x, mask, sd, prefix, eps):
    """nn.BatchNorm1d.eval() on the [N, C] rows of the active voxels."""
    v = lambda k: sd["%s.%s" % (prefix, k)].to(x.dtype).view(1, -1, 1, 1, 1)
    return ((x - v("running_mean")) / torch.sqrt(v("running_var") + eps) * v("weight") + v("bias")) * mask


def encoder_forward(sd, cfg, feats, coors, dtype=torch.float64):
    """-> (dense [1, C, Z, Y, X] = out.dense() (sparse_encoder_hd.py:128-129), final active mask [1,1,Z,Y,X])."""
    eps = dict(DEFAULTS["norm_cfg"], **cfg.get("norm_cfg", {})).get("eps", 1e-5)
    sd = {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}
    x, mask = to_dense(torch.as_tensor(feats).to(dtype), coors, cfg["sparse_shape"])
    for kind, pre, cin, cout, k, s, p in layer_plan(cfg):
        if kind == "block":                                                           # sparse_block.py:103-121
            h, _ = conv_layer(x, mask, sd[pre + ".conv1.weight"], k, s, p, True)
            h = F.relu(bn_rows(h, mask, sd, pre + ".bn1", eps))
            h, _ = conv_layer(h, mask, sd[pre + ".conv2.weight"], k, s, p, True)
            x = F.relu(bn_rows(h, mask, sd, pre + ".bn2", eps) + x) * mask
        else:
            x, mask = conv_layer(x, mask, sd[pre + ".0.weight"], k, s, p, kind == "subm")
            x = F.relu(bn_rows(x, mask, sd, pre + ".1", eps))
    return x, mask


# ----------------------------------------------------------------------------- rule books
def brute_book(coors, shape, k, s, p):
    """From the definition: output o reads input i = o*s - p + t per axis through tap t = (kd*ky + kh)*kx + kw; o is active iff
    some active i is reached.  -> (out coors [Mo,3] ascending (z,y,x), table [taps, Mo] of input rows or -1, out shape).  A plain
    loop over every output site: small grids only."""
    idx = {tuple(int(v) for v in c): j for j, c in enumerate(np.asarray(coors).reshape(-1, 3))}
    osz = out_size(shape, k, s, p)
    outs, cols = [], []
    for o in itertools.product(*(range(n) for n in osz)):
        col = [idx.get(tuple(o[a] * s[a] - p[a] + t[a] for a in range(3)), -1) for t in itertools.product(*(range(kk) for kk in k))]
        if any(r >= 0 for r in col):
            outs.append(o)
            cols.append(col)
    taps = k[0] * k[1] * k[2]
    return (np.asarray(outs, np.int64).reshape(-1, 3), np.asarray(cols, np.int64).reshape(-1, taps).T.copy(), osz)


def valid_out_pos(pos, k, s, p, osz):
    """geometry.h:25-86 (getValidOutPos, dilation 1) with per-axis kernel / stride / padding, for one input position:
    [(out position, kernel offset)], offset = (kz*ky + ky_)*kx + kx_ accumulated from the last axis as upstream does."""
    rng = []
    for a in range(3):
        lo = (pos[a] - (k[a] - 1) - 1 + s[a] + p[a]) // s[a]
        hi = (pos[a] + p[a]) // s[a]
        rng.append(range(lo, hi + 1))
    res = []
    for o in itertools.product(*rng):
        if any(v < 0 or v > osz[a] - 1 for a, v in enumerate(o)):
            continue
        off, m = 0, 1
        for a in (2, 1, 0):
            off += m * (pos[a] - o[a] * s[a] + p[a])
            m *= k[a]
        res.append((o, off))
    return res


def scatter_book(coors, shape, k, s, p):
    """The rule book the way spconv builds it (geometry.h:144-192): every input scatters to its valid outputs.  Same return
    as ``brute_book`` (outputs sorted, which the library's hash order does not promise and no consumer observes)."""
    osz = out_size(shape, k, s, p)
    pairs = {}
    for j, c in enumerate(np.asarray(coors).reshape(-1, 3)):
        for o, off in valid_out_pos(tuple(int(v) for v in c), k, s, p, osz):
            pairs.setdefault(o, {})[off] = j
    outs = sorted(pairs)
    taps = k[0] * k[1] * k[2]
    table = np.full((taps, len(outs)), -1, np.int64)
    for n, o in enumerate(outs):
        for off, j in pairs[o].items():
            table[off, n] = j
    return np.asarray(outs, np.int64).reshape(-1, 3), table, osz


def active_outputs(coors, shape, k, s, p):
    """Vectorised active set of SparseConv3d (any size): sorted unique linear ids (z*Ho + y)*Wo + x of the outputs
    o = (i + p - t) / s that are whole and in range, over every active input i and tap t."""
    c = np.asarray(coors, np.int64).reshape(-1, 3)
    osz = out_size(shape, k, s, p)
    ids = []
    for t in itertools.product(*(range(kk) for kk in k)):
        num = c + np.asarray(p) - np.asarray(t)
        o = num // np.asarray(s)
        ok = ((num % np.asarray(s)) == 0).all(1) & (num >= 0).all(1) & (o < np.asarray(osz)).all(1)
        o = o[ok]
        ids.append((o[:, 0] * osz[1] + o[:, 1]) * osz[2] + o[:, 2])
    return np.unique(np.concatenate(ids)) if ids else np.zeros(0, np.int64)


def rulebook_conv(feats, coors, shape, w_v1, k, s, p, book=brute_book):
    """out[o] = sum_t feats[table[t][o]] @ W[t] over a rule book (float64) -> (rows [Mo, Cout], out coors, out shape)."""
    outs, table, osz = book(coors, shape, k, s, p)
    f = torch.as_tensor(feats).double()
    W = w_v1.double().reshape(-1, w_v1.shape[3], w_v1.shape[4])
    y = torch.zeros(len(outs), W.shape[2], dtype=torch.float64)
    for t in range(table.shape[0]):
        m = torch.from_numpy(table[t] >= 0)
        if m.any():
            y[m] += f[torch.from_numpy(table[t])[m]] @ W[t]
    return y, outs, osz


# ----------------------------------------------------------------------------- inputs
def edge_voxels(shape, block_at=None):
    """Voxels on all six faces and in the eight corners, one isolated voxel, and a solid 4^3 block: [M,3] (z,y,x), unique."""
    D, H, W = shape
    pts = set(itertools.product((0, D - 1), (0, H - 1), (0, W - 1)))
    pts |= {(0, H // 2, W // 3), (D - 1, H // 3, W // 2), (D // 2, 0, W // 2), (D // 3, H - 1, W // 2), (D // 2, H // 2, 0), (D // 3, H // 3, W - 1)}
    pts.add((D // 2, H // 4, (3 * W) // 4))                          # nothing within two cells of it
    b = block_at or (min(D // 2 + 2, D - 4), min(H // 2 + 1, H - 4), max(W // 2 - 5, 0))
    pts |= {(b[0] + a, b[1] + c, b[2] + e) for a, c, e in itertools.product(range(4), repeat=3)}
    assert all(0 <= z < D and 0 <= y < H and 0 <= x < W for z, y, x in pts)
    return np.asarray(sorted(pts), np.int32)


def random_voxels(shape, n, seed):
    rs = np.random.RandomState(seed)
    D, H, W = shape
    lin = rs.choice(D * H * W, size=n, replace=False)
    return np.stack([lin // (H * W), (lin // W) % H, lin % W], 1).astype(np.int32)
