"""Restatements of the reference's SSIM, kept in the test tree: ``save_rendered_img`` (P/utils/save_rendered_img.py:22-37, 39-79)
calls ``skimage.metrics.structural_similarity(pred, target, channel_axis=-1)`` of scikit-image 0.19.3 on float32 [H,W,3] images with
no other argument.  scikit-image is not a dependency of this project, so no fixture comes from the library itself; the judge of the
HIP kernel is ``ssim64``, the definition written directly in float64, and tests/test_render_ssim_host.py checks it against a second,
independent float64 form (``scipy.ndimage.uniform_filter``).

With skimage's defaults: 7 x 7 uniform window (NP = 49), sample covariance (NP / (NP - 1)), data_range R = 2.0 for float images (the
span of ``dtype_range``), C1 = (0.01 R)^2, C2 = (0.03 R)^2, S averaged over the pixels whose whole window lies inside the image (a
crop of 3 per side), then over the three channels; ``save_rendered_img`` adds the views one by one in fp32 and divides by N."""
import numpy as np
import torch

WIN = 7
NP = WIN * WIN
COV = NP / (NP - 1.0)


def _s_map(ux, uy, uxx, uyy, uxy, R):
    vx, vy, vxy = COV * (uxx - ux * ux), COV * (uyy - uy * uy), COV * (uxy - ux * uy)
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def _box(a):
    """The 49-term mean of every whole 7 x 7 window of a float64 [H,W] array -> [H-6, W-6]."""
    return np.lib.stride_tricks.sliding_window_view(a, (WIN, WIN)).mean(axis=(-2, -1))


def _channel64(args):
    x, y, R = args
    return _s_map(_box(x), _box(y), _box(x * x), _box(y * y), _box(x * y), R).mean()


def ssim64(rgbs, gt_img, R=2.0):
    """rgbs [N,H,W,3], gt_img [N,3,H,W] (numpy or CPU tensors, fp32) -> float64 [N,3]: per view and channel the mean of S over
    the (H-6)(W-6) whole windows; every box mean is the plain 49-term mean of a ``sliding_window_view``.  The 3N channels are
    independent and go to a few threads (numpy's reductions release the interpreter lock): the r101 size takes seconds, not a
    minute."""
    from concurrent.futures import ThreadPoolExecutor
    rgbs, gt_img = np.asarray(rgbs, dtype=np.float64), np.asarray(gt_img, dtype=np.float64)
    N = rgbs.shape[0]
    jobs = [(np.ascontiguousarray(rgbs[v, :, :, c]), gt_img[v, c], float(R)) for v in range(N) for c in range(3)]
    with ThreadPoolExecutor(max_workers=8) as ex:
        vals = list(ex.map(_channel64, jobs))
    return np.asarray(vals, dtype=np.float64).reshape(N, 3)


def ssim64_filter(rgbs, gt_img, R=2.0):
    """The same quantity through ``scipy.ndimage.uniform_filter`` in float64 and a crop of 3: the second form ``ssim64`` is checked
    against."""
    from scipy.ndimage import uniform_filter
    rgbs, gt_img = np.asarray(rgbs, dtype=np.float64), np.asarray(gt_img, dtype=np.float64)
    f = lambda a: uniform_filter(a, size=WIN)[3:-3, 3:-3]
    out = np.empty((rgbs.shape[0], 3))
    for v in range(rgbs.shape[0]):
        for c in range(3):
            x, y = rgbs[v, :, :, c], gt_img[v, c]
            out[v, c] = _s_map(f(x), f(y), f(x * x), f(y * y), f(x * y), float(R)).mean()
    return out


def view_ssim(channels):
    """float64 [N,3] channel values -> the view's value as the kernel's block holds it: (c0 + c1 + c2) / 3 rounded once to fp32."""
    channels = np.asarray(channels, dtype=np.float64)
    return ((channels[:, 0] + channels[:, 1] + channels[:, 2]) / 3).astype(np.float32)


def ssim32(rgbs, gt_img, R=2.0):
    """skimage 0.19.3's own chain on float32 images: ``uniform_filter(size=7)`` in fp32, the pointwise chain in fp32, crop 3,
    ``mean(dtype=float64)`` per channel, the fp32 mean of the channel values, and save_rendered_img's sequential fp32 sum over the
    views / N -> (ssim [N] fp32, mean fp32)."""
    from scipy.ndimage import uniform_filter
    rgbs, gt_img = np.asarray(rgbs, dtype=np.float32), np.asarray(gt_img, dtype=np.float32)
    f = lambda a: uniform_filter(a, size=WIN)
    cov, R = np.float32(COV), float(R)
    C1, C2 = np.float32((0.01 * R) ** 2), np.float32((0.03 * R) ** 2)
    vals = []
    for v in range(rgbs.shape[0]):
        ch = np.empty(3, dtype=np.float32)       # skimage: mssim = np.empty(nch, dtype=float_type); mssim[ch] = ...; mssim.mean()
        for c in range(3):
            x, y = rgbs[v, :, :, c], gt_img[v, c]
            ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
            vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
            A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
            S = (A1 * A2) / (B1 * B2)
            assert S.dtype == np.float32
            ch[c] = S[3:-3, 3:-3].mean(dtype=np.float64)
        vals.append(ch.mean())
    total = np.float32(0)
    for s in vals:
        total = np.float32(total + s)
    return np.asarray(vals, dtype=np.float32), np.float32(total / np.float32(len(vals)))


def ssim_torch(rgbs, gt_img, R=2.0):
    """The torch form on whichever device the inputs live on -- the yardstick the HIP kernels are timed against: per view five
    ``avg_pool2d(7, stride=1)`` passes over the three channels plus the pointwise chain -> (ssim [N] fp32, mean fp32)."""
    import torch.nn.functional as F
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    pool = lambda a: F.avg_pool2d(a, WIN, stride=1)
    vals = []
    for v in range(rgbs.shape[0]):
        x, y = rgbs[v].permute(2, 0, 1).unsqueeze(0), gt_img[v].unsqueeze(0)          # [1,3,H,W]
        ux, uy, uxx, uyy, uxy = pool(x), pool(y), pool(x * x), pool(y * y), pool(x * y)
        vx, vy, vxy = COV * (uxx - ux * ux), COV * (uyy - uy * uy), COV * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        vals.append(S.flatten(2).mean(2).mean())
    total = torch.zeros((), dtype=torch.float32, device=rgbs.device)
    for s in vals:
        total = total + s
    return torch.stack(vals), total / rgbs.shape[0]
