"""References of the camera img_inputs tests (test_image_inputs_host.py, test_gpu_image_inputs.py), written apart from
co_occ_amd/image_inputs.py:
  - the numpy integer restatement of Pillow's 8-bit bicubic resize (coeffs, resize), crop, flip and to_imgs;
  - the host restatement of the augmentation parameters, the matrices and the calibration;
  - the case lists both test files share.
Nothing here imports the package."""
import math

import numpy as np
import torch

BITS = 22
CAMS = ['CAM_FRONT_LEFT', 'CAM_FRONT', 'CAM_FRONT_RIGHT', 'CAM_BACK_LEFT', 'CAM_BACK', 'CAM_BACK_RIGHT']
# the data_config of the two coocc_nusc camera configs, and one with the ranges a training draw needs
R50 = dict(cams=CAMS, Ncams=6, input_size=(256, 704), src_size=(900, 1600), resize=(0, 0), rot=(0, 0), flip=False,
           crop_h=(0.0, 0.0), resize_test=0.00)
R101 = dict(cams=CAMS, Ncams=6, input_size=(896, 1600), src_size=(900, 1600), resize=(0, 0), rot=(0, 0), flip=False,
            crop_h=(0.0, 0.0), resize_test=0.00)
TRAIN = dict(cams=CAMS, Ncams=5, input_size=(256, 704), src_size=(900, 1600), resize=(-0.06, 0.11), rot=(0, 0), flip=True,
             crop_h=(0.0, 0.1), resize_test=0.00)

# (Hs, Ws) -> (newH, newW): the pairs the restatement is held against live Pillow at
SIZE_PAIRS = [((37, 53), (16, 23)), ((37, 53), (37, 23)), ((37, 53), (16, 53)), ((20, 31), (47, 64)), ((64, 64), (7, 9)),
              ((9, 7), (64, 64)), ((13, 200), (13, 17)), ((5, 5), (1, 1))]
FULL_PAIRS = [((900, 1600), (396, 704)), ((900, 1600), (900, 1600))]
PATTERNS = ["random", "checker", "stripes"]

# name -> (Hs, Ws, resize_dims (newW, newH), crop (x0, y0, x1, y1), flip): the small cases of the fixture and of the GPU tests.
# The GPU kernel's output tile is 16 rows x 64 columns: widths 63 / 64 / 65 / 129 and heights 15 / 16 / 17 / 33 are in.  The unresized
# form takes four pixels per thread when the width is a multiple of 4 (w32 / w28 / w36: mirrored, odd origin, leaving on the right).
CASES = {
    "both_passes": (37, 53, (23, 16), (3, 2, 19, 14), False),
    "horizontal_only": (37, 53, (23, 37), (3, 2, 19, 14), False),
    "vertical_only": (37, 53, (53, 16), (3, 2, 19, 14), False),
    "up_20x31": (20, 31, (64, 47), (0, 0, 64, 47), False),
    "up_9x7": (9, 7, (64, 64), (0, 0, 64, 64), False),
    "down_strong": (64, 64, (11, 9), (0, 0, 11, 9), False),
    "one_pixel": (5, 5, (1, 1), (0, 0, 1, 1), False),
    "r101_form": (20, 32, (32, 20), (0, 4, 32, 20), False),
    "out_left": (37, 53, (23, 16), (-5, 2, 11, 12), False),
    "out_top": (37, 53, (23, 16), (3, -4, 19, 8), False),
    "out_right": (37, 53, (23, 16), (12, 2, 30, 12), False),
    "out_bottom": (37, 53, (23, 16), (3, 9, 19, 21), False),
    "out_wholly": (37, 53, (23, 16), (40, 30, 56, 40), False),
    "flip_odd": (37, 53, (23, 16), (2, 1, 19, 14), True),
    "flip_out": (37, 53, (23, 16), (-5, -3, 12, 12), True),
    "ws64": (40, 64, (29, 18), (1, 1, 28, 17), False),
    "tile_65x17": (40, 150, (70, 19), (2, 1, 67, 18), False),
    "tile_63x15": (40, 150, (70, 19), (3, 2, 66, 17), True),
    "tile_129x33": (50, 200, (140, 40), (5, 3, 134, 36), False),
    "r101_flip_out": (20, 32, (32, 20), (-3, 4, 30, 23), True),
    "r101_flip_out_w32": (20, 32, (32, 20), (-3, 4, 29, 23), True),
    "r101_odd_origin_w28": (20, 32, (32, 20), (1, 2, 29, 18), False),
    "r101_out_right_w36": (20, 32, (32, 20), (4, -2, 40, 22), False),
}
FIXTURE_CASES = ["both_passes", "horizontal_only", "vertical_only", "up_20x31", "up_9x7", "down_strong", "one_pixel", "r101_form",
                 "out_left", "flip_odd", "flip_out", "tile_65x17"]
# six cameras of one 37 x 53 call with six parameter sets (common output 14 x 17)
SIX = [((23, 16), (3, 1, 20, 15), False), ((23, 37), (2, 20, 19, 34), True), ((53, 16), (30, 1, 47, 15), False),
       ((53, 37), (-2, 30, 15, 44), True), ((64, 47), (40, 30, 57, 44), False), ((9, 7), (-4, -3, 13, 11), True)]


def frame(Hs, Ws, pattern, seed=0):
    """uint8 [Hs, Ws, 3]: random bytes, a 0/255 checkerboard, or 0/255 stripes of 3 columns (both ends of the clamp)."""
    if pattern == "random":
        return np.random.default_rng([seed, Hs, Ws]).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    y, x = np.mgrid[0:Hs, 0:Ws]
    m = ((x + y) % 2) if pattern == "checker" else ((x // 3 + seed) % 2)
    f = (m * 255).astype(np.uint8)
    return np.stack([f, 255 - f, f], -1)


# ------------------------------------------------------------------ Pillow's resize as integers
def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size):
    """[(xmin, [taps as int])] per output index: Pillow's precompute_coeffs and normalize_coeffs_8bpc, a loop at a time."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        out.append((xmin, [int(-0.5 + w * (1 << BITS)) if w < 0 else int(0.5 + w * (1 << BITS)) for w in k]))
    return out


def _pass(img, table, axis):
    img = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(table),) + img.shape[1:], np.uint8)
    for i, (xmin, taps) in enumerate(table):
        acc = np.full(img.shape[1:], 1 << (BITS - 1), np.int64)
        for k, t in enumerate(taps):
            acc += img[xmin + k] * t
        out[i] = np.clip(acc >> BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, resize_dims):
    """Image.resize(resize_dims) of a uint8 [H, W, 3] array: horizontal pass, uint8, vertical pass; an unchanged axis is skipped."""
    newW, newH = resize_dims
    H, W = img.shape[:2]
    if newW != W:
        img = _pass(img, coeffs(W, newW), 1)
    if newH != H:
        img = _pass(img, coeffs(H, newH), 0)
    return np.ascontiguousarray(img)


def crop(img, box):
    """Image.crop(box): zeros where the box leaves the image."""
    x0, y0, x1, y1 = box
    H, W = img.shape[:2]
    out = np.zeros((y1 - y0, x1 - x0, 3), np.uint8)
    ya, yb, xa, xb = max(y0, 0), min(y1, H), max(x0, 0), min(x1, W)
    if ya < yb and xa < xb:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = img[ya:yb, xa:xb]
    return out


def flip(img):
    return np.ascontiguousarray(img[:, ::-1])


def canvas(frame_, resize_dims, box, do_flip):
    out = crop(resize(frame_, resize_dims), box)
    return flip(out) if do_flip else out


def to_imgs(canvas_):
    """[N, fH, fW, 3] bytes -> the reference's fp32 [N, 3, fH, fW]: torch on the CPU, a true division."""
    t = torch.from_numpy(np.ascontiguousarray(canvas_))
    return (t.float().permute(0, 3, 1, 2).contiguous() / 255.)


# ------------------------------------------------------------------ the host side, restated
def augmentation_eval(cfg, H, W, flip_=None, scale=None):
    fH, fW = cfg['input_size']
    r = float(fW) / float(W) + cfg.get('resize_test', 0.0)
    if scale is not None:
        r = scale
    newW, newH = int(W * r), int(H * r)
    ch = int((1 - np.mean(cfg['crop_h'])) * newH) - fH
    cw = int(max(0, newW - fW) / 2)
    return r, (newW, newH), (cw, ch, cw + fW, ch + fH), (False if flip_ is None else flip_), 0


def post_matrices(resize_, box, do_flip):
    """post_rot [3,3], post_tran [3] for rotate = 0, with the reference's float32 operations."""
    rot = torch.eye(2) * resize_
    tran = torch.zeros(2) - torch.Tensor(box[:2])
    if do_flip:
        A = torch.Tensor([[-1, 0], [0, 1]])
        rot = A.matmul(rot)
        tran = A.matmul(tran) + torch.Tensor([box[2] - box[0], 0])
    A = torch.Tensor([[np.cos(0.0), np.sin(0.0)], [-np.sin(0.0), np.cos(0.0)]])
    b = torch.Tensor([box[2] - box[0], box[3] - box[1]]) / 2
    b = A.matmul(-b) + b
    rot = A.matmul(rot)
    tran = A.matmul(tran) + b
    R, T = torch.eye(3), torch.zeros(3)
    R[:2, :2] = rot
    T[:2] = tran
    return R, T


def nerf_intrinsics(K, resize_, box):
    k = torch.Tensor(np.asarray(K))
    k[:2] = k[:2] * resize_
    k[0, 2] -= box[0]
    k[1, 2] -= box[1]
    return k


def quat_matrix(q):
    q = np.asarray(q, np.float64)
    n2 = float(np.dot(q, q))
    if not abs(1.0 - n2) < 1e-14:
        q = q / math.sqrt(n2)
    w, x, y, z = q
    L = np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])
    Rm = np.array([[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]])
    return np.dot(L, Rm.T)[1:, 1:]


def pose(q, t):
    p = np.eye(4)
    p[:3, :3] = quat_matrix(q)
    p[:3, 3] = t
    return p


def synthetic_calibration(seed=5):
    """(cam_infos, lidar2cam_dic) of a six-camera rig: random unit-ish quaternions, translations, intrinsics, rigid lidar2cam."""
    g = np.random.default_rng(seed)
    infos, l2c = {}, {}
    for i, name in enumerate(CAMS):
        q1, q2 = g.standard_normal(4), g.standard_normal(4)
        q1, q2 = q1 / np.linalg.norm(q1), q2 / np.linalg.norm(q2)
        infos[name] = dict(cam_intrinsic=[[1266.4 + i, 0.0, 816.2 - i], [0.0, 1266.4 + i, 491.5 + i], [0.0, 0.0, 1.0]],
                           sensor2ego_rotation=list(q1), sensor2ego_translation=list(g.uniform(-2, 2, 3)),
                           ego2global_rotation=list(q2 * 1.0000001), ego2global_translation=list(g.uniform(-900, 900, 3)))
        m = np.eye(4)
        m[:3, :3] = quat_matrix(g.standard_normal(4))
        m[:3, 3] = g.uniform(-2, 2, 3)
        l2c[name] = m
    return infos, l2c


def img_inputs14(cfg, frames, infos, l2c, flip_=None, scale=None):
    """The reference's 14-tuple (no batch dimension) on the CPU from uint8 frames [N, Hs, Ws, 3], eval mode."""
    cols = [[] for _ in range(10)]
    cv = []
    for name, f in zip(cfg['cams'], frames):
        r, dims, box, fl, _ = augmentation_eval(cfg, f.shape[0], f.shape[1], flip_, scale)
        R, T = post_matrices(r, box, fl)
        s2l = torch.tensor(np.asarray(l2c[name], np.float64)).inverse().float()
        d = infos[name]
        c2w = torch.Tensor(pose(d['ego2global_rotation'], d['ego2global_translation']) @
                           pose(d['sensor2ego_rotation'], d['sensor2ego_translation']))
        cv.append(canvas(f, dims, box, fl))
        for lst, v in zip(cols, (s2l[:3, :3], s2l[:3, 3], torch.Tensor(d['cam_intrinsic']), R, T, torch.zeros(1), s2l,
                                 nerf_intrinsics(d['cam_intrinsic'], r, box), c2w)):
            lst.append(v)
    cv = np.stack(cv)
    imgs = to_imgs(cv)
    rots, trans, intrins, post_rots, post_trans, gt_depths, s2s, nerf, c2ws = [torch.stack(c) for c in cols[:9]]
    return (imgs, rots, trans, intrins, post_rots, post_trans, torch.eye(3), gt_depths, s2s, imgs.clone(), None, nerf, c2ws,
            imgs.shape[-2:]), cv
