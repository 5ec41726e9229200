"""Torch restatement of the reference's render evaluation, kept in the test tree: the judge of the HIP kernels at sizes the golden
fixture (tests/golden/render_eval.npz, made by the unmodified reference: tools/gen_golden_render_eval.py) cannot cover.
tests/test_render_eval_host.py pins it to that fixture on the CPU; it runs on whichever device its inputs live on, so the same lines
are also the torch-on-GPU yardstick the kernels are timed against."""
import numpy as np
import torch


def psnr(rgbs, gt_img):
    """compute_psnr (P/utils/save_rendered_img.py:10-20) per view as COOCC_Ray.simple_test calls it (coocc_ray.py:633-636):
    rgbs [N,H,W,3], gt_img [N,3,H,W] -> (psnr [N] fp32, their mean accumulated one by one in fp32)."""
    vals = []
    for v in range(rgbs.shape[0]):
        mse = ((rgbs[v] - gt_img[v].permute(1, 2, 0)) ** 2).mean()
        vals.append(-10.0 * torch.log(mse) / np.log(10.0))
    total = torch.zeros((), dtype=torch.float32, device=rgbs.device)
    for p in vals:
        total = total + p
    return torch.stack(vals), total / rgbs.shape[0]


def psnr64(rgbs, gt_img):
    """The same quantity in float64 from the fp32 inputs."""
    d = rgbs.double() - gt_img.double().permute(0, 2, 3, 1)
    return -10.0 * torch.log((d ** 2).flatten(1).mean(1)) / np.log(10.0)


def panels(rgbs, depths, gt_img):
    """coocc_ray.py:629-632: uint8 [N,H,3W,3] = [rgb | gt | normalised depth], clipped to [0, 1], times 255, truncated."""
    out = []
    for v in range(rgbs.shape[0]):
        dmin, dmax = depths[v].min(), depths[v].max()
        depth_ = ((depths[v] - dmin) / (dmax - dmin + 1e-8)).unsqueeze(-1).repeat(1, 1, 3)
        panel = torch.cat([rgbs[v], gt_img[v].permute(1, 2, 0), depth_], dim=1).clip(0, 1)
        out.append((panel * 255.0).to(torch.uint8))
    return torch.stack(out)


def depth_error(depths, gt_depth):
    """save_rendered_img.py:58 summed per view over the pixels with gt_depth > 0, in float64 -> (sum [N] fp64, count [N] int64)."""
    valid = gt_depth > 0
    e = (depths.double() - gt_depth.double()) ** 2
    return (e * valid).flatten(1).sum(1), valid.flatten(1).sum(1)


def ulps(a, b):
    """Distance in fp32 units in the last place between two fp32 arrays of finite values of one sign."""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())
