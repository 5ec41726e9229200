"""Prediction dump of the nuScenes test loop -- mirror of ``save_output_nuscenes`` (P/coocc/apis/utils.py:54-110), of the lidarseg
submission writer ``save_nuscenes_lidarseg_submission`` (:112-133) and of the
label preparation in ``custom_single_gpu_test`` (P/coocc/apis/test.py:67-68,197-201).

Upstream resamples the logits to the ground-truth grid with ``F.interpolate``, takes ``argmax`` on the device, copies an
int64 volume to the host and narrows it to uint8 there.  ``predict_labels`` produces the uint8 volume on the device in one
kernel (no resampled [1,C,H,W,D] temporary: 174 MB at 17 x 200 x 200 x 16 fp32); the pickle written by
``save_output_nuscenes`` has the upstream keys (``pred_voxels``, ``cam2lidar``, ``img_canvas``)."""
import json
import os
import pickle

import numpy as np
import torch

from ._lib import call, ptr

CAMERA_NAMES = ['CAM_FRONT_LEFT', 'CAM_FRONT', 'CAM_FRONT_RIGHT', 'CAM_BACK_LEFT', 'CAM_BACK', 'CAM_BACK_RIGHT']


def predict_labels(pred, size=None):
    """pred [1,C,h,w,d] float logits (any strides) -> uint8 device tensor [1,H,W,D] = argmax over classes of the logits
    trilinearly resampled to ``size`` (default: the logits' own grid)."""
    if not pred.is_cuda:
        raise RuntimeError("co_occ_amd.apis.predict_labels runs on the HIP device only")
    assert pred.dim() == 5 and pred.shape[0] == 1, "batch size 1 (test.py:59)"
    pred = pred.float()
    C, h, w, d = pred.shape[1:]
    H, W, D = [int(v) for v in (size if size is not None else (h, w, d))]
    out = torch.empty(1, H, W, D, dtype=torch.uint8, device=pred.device)
    sc, sx, sy, sz = pred.stride()[1:]
    call("coocc_predict_labels", ptr(pred, strided=True), sc, sx, sy, sz, C, h, w, d, H, W, D, ptr(out))
    return out


def save_output_nuscenes(img_inputs, output_voxels, save_path, scene_token, sample_token, img_filenames, timestamp,
                         scene_name):
    """Same arguments and file as upstream.  ``output_voxels``: [1,X,Y,Z] labels (``predict_labels`` output, or the
    upstream int64 argmax).  ``img_filenames``: {camera name: path} or None (then ``img_canvas`` is an empty list)."""
    rots, trans = img_inputs[1:3]
    num_img = rots.shape[1]
    cam2lidar = np.repeat(np.eye(4)[np.newaxis], repeats=num_img, axis=0)
    cam2lidar[:, :3, :3] = rots[0].detach().cpu().numpy()
    cam2lidar[:, :3, -1] = trans[0].detach().cpu().numpy()
    labels = output_voxels[0].detach().cpu().numpy().astype(np.uint8)
    canvas = []
    if img_filenames:
        from PIL import Image
        for name in CAMERA_NAMES:
            canvas.append(Image.open(img_filenames[name]).resize([480, 270], Image.BILINEAR))
    out_dict = dict(pred_voxels=labels, cam2lidar=cam2lidar, img_canvas=canvas)
    if scene_name is not None:
        save_path = os.path.join(save_path, scene_name)
        filepath = os.path.join(save_path, str(timestamp) + '.pkl')
    else:
        filepath = os.path.join(save_path, sample_token + '.pkl')
    os.makedirs(save_path, exist_ok=True)
    with open(filepath, "wb") as handle:
        pickle.dump(out_dict, handle)
    return filepath


def save_nuscenes_lidarseg_submission(output_points, save_path, img_metas):
    """P/coocc/apis/utils.py:112-133: ``<save_path>/test/submission.json`` (the upstream ``meta`` dict, written once) and
    ``<save_path>/lidarseg/test/<lidar_token>_lidarseg.bin``, the point labels as uint8.  ``output_points``: ``simple_test``'s
    int64 labels (device or host).  Returns the path of the .bin file."""
    meta_file = os.path.join(save_path, 'test', 'submission.json')
    if not os.path.exists(meta_file):
        os.makedirs(os.path.join(save_path, 'test'), exist_ok=True)
        meta = dict(meta=dict(use_lidar=False, use_camera=True, use_radar=False, use_map=False, use_external=False))
        with open(meta_file, 'w') as f:
            json.dump(meta, f)
    save_path = os.path.join(save_path, 'lidarseg', 'test')
    os.makedirs(save_path, exist_ok=True)
    save_file = os.path.join(save_path, '{}_lidarseg.bin'.format(img_metas['lidar_token']))
    labels = output_points.detach().cpu().numpy() if torch.is_tensor(output_points) else np.asarray(output_points)
    labels.astype(np.uint8).tofile(save_file)
    return save_file


def save_rendered_panels(result_or_maps, out_dir, gt_img=None, prefix="view_"):
    """The comparison images upstream writes from ``simple_test`` (coocc_ray.py:629-636, ``./img_<v>.png``) and from
    ``save_rendered_img`` (P/utils/save_rendered_img.py:59-77), without ``cv2.putText``: one ``[rgb | gt | normalised depth]`` uint8
    panel per view, composed on the device (``coocc_render_panels``) and copied to the host once.

    ``result_or_maps``: ``simple_test``'s result (its ``rgbs`` / ``depths``) or a ``(rgbs, depths)`` pair; ``gt_img`` [N,3,H,W]
    (``img[0][0]``; a result dict may carry it as ``gt_img``).  Writes ``<out_dir>/<prefix><v>.png`` through cv2 or PIL, whichever
    imports; with neither, ``.npy`` arrays (and a warning that says so).  Returns (paths, panels uint8 numpy [N,H,3W,3]); the
    channel order of the files is the arrays' (upstream hands the same RGB-ordered array to ``cv2.imwrite``)."""
    from . import evaluation as E
    if isinstance(result_or_maps, dict):
        rgbs, depths = result_or_maps.get("rgbs"), result_or_maps.get("depths")
        gt_img = gt_img if gt_img is not None else result_or_maps.get("gt_img")
    else:
        rgbs, depths = result_or_maps[:2]
    if rgbs is None or depths is None or gt_img is None:
        raise ValueError("save_rendered_panels: rgbs, depths (a rendered result) and gt_img are needed")
    panels = E.render_eval(rgbs, depths, gt_img, panels=True)["panels"].cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    writer, ext = None, ".npy"
    try:
        import cv2
        writer, ext = (lambda f, a: cv2.imwrite(f, a)), ".png"
    except ImportError:
        try:
            from PIL import Image
            writer, ext = (lambda f, a: Image.fromarray(a).save(f)), ".png"
        except ImportError:
            import warnings
            warnings.warn("save_rendered_panels: neither cv2 nor PIL imports; writing the panels as .npy arrays")
            writer = lambda f, a: np.save(f, a)
    paths = []
    for v in range(panels.shape[0]):
        paths.append(os.path.join(out_dir, "%s%d%s" % (prefix, v, ext)))
        writer(paths[-1], panels[v])
    return paths, panels


def visualize_result(img_inputs, output_voxels, img_canvas=None, cat_save_file=None, save_folder=None, vox_origin=None, voxel_size=None):
    """The picture of ``visualize_nusc.py`` straight from a ``simple_test`` / ``pipelined_test`` result, without the pickle of
    ``save_output_nuscenes``: ``img_inputs`` gives ``cam2lidar`` as there (``rots``, ``trans`` of its entries 1 and 2),
    ``output_voxels`` is any label volume [1,X,Y,Z] or [X,Y,Z] -- ``predict_labels``' uint8, upstream's int64 argmax, or a ground-truth
    volume of ``occ_gt`` -- and stays on the device.  ``img_canvas``: the six 480 x 270 input frames (PIL images or uint8 arrays);
    without it their boxes stay black.  ``vox_origin`` / ``voxel_size`` default to the reference's nuScenes range divided by the
    volume's own shape.  Returns the canvas (uint8 [1640,2930,3]); writes ``cat_save_file`` and, into ``save_folder``, the eight
    views when given (``visualize.draw_nusc_occupancy``)."""
    from . import visualize as VZ
    rots, trans = img_inputs[1:3]
    cam2lidar = np.repeat(np.eye(4)[np.newaxis], repeats=rots.shape[1], axis=0)
    cam2lidar[:, :3, :3] = rots[0].detach().cpu().numpy()
    cam2lidar[:, :3, -1] = trans[0].detach().cpu().numpy()
    vol = output_voxels[0] if output_voxels.ndim == 4 else output_voxels
    if vox_origin is None or voxel_size is None:
        o, v = VZ.grid_of(list(vol.shape))
        vox_origin, voxel_size = (o if vox_origin is None else vox_origin), (v if voxel_size is None else voxel_size)
    return VZ.draw_nusc_occupancy(img_canvas, vol, vox_origin, voxel_size, grid=np.array(vol.shape), save_folder=save_folder,
                                  cat_save_file=cat_save_file, cam2lidar=cam2lidar)


def pipelined_test(model, data_iter, slots=6, dense_streams=3, ahead=0, stats=None):
    """The loop of ``custom_single_gpu_test`` (P/coocc/apis/test.py:43-45: ``result = model(return_loss=False, **data)`` once per
    sample) with ``slots`` samples in flight (``co_occ_amd.serving``): a generator of ``(data, result)`` in sample order, ``result``
    = what ``COOCC_Ray.simple_test`` returns for that sample (same tensors, same metrics, fine outputs trimmed to their exact
    size).  ``data``: the keyword arguments of ``simple_test`` (``img_inputs`` / ``img``, ``points``, ``gt_occ``,
    ``visible_mask``, ``points_occ``, ``img_metas``, ``gt_depths``, ``precomputed``).  With ``model.render_eval`` the render keys
    (``psnr``, ``psnr_mean``, ``depth_sq_err``, ``depth_valid``) are computed the same way (``coocc_render_eval_stats``), and with
    ``model.render_ssim`` on top of it ``ssim`` / ``ssim_mean`` (``coocc_render_eval_ssim``).

    Nothing in the loop waits for the sample that was just issued: the encoders upstream of the hot path run eagerly at submit
    time; pooling + index search of the next ``ahead`` samples are prefetched under the dense stages (one captured hipGraph
    launch per sample) of the current ones; a sample's SC / SSC confusion matrices (``coocc_eval_semantic``), its lidarseg labels
    and 16x16 matrix (``coocc_lidarseg_points``, when it carries ``points_occ``) and its fine-point count are computed on ITS dense stream right behind the replay and copied to pinned host memory asynchronously; the sample
    is yielded ``dense_streams`` issues later, when that copy has normally long finished.  A sample whose ``gt_occ`` is not the
    captured fine grid (cascade_ratio x the coarse grid) takes ``model.simple_test`` (eager decode) in its turn -- when the head
    has a fine branch; without one nothing is scattered and the metrics kernel resamples ``pred_c`` to any ground-truth grid.
    Models without a fuser (camera-only ``COOCC_Ray``, ``COOCC_Ray_L``) run the same loop: their prefetch stage is the copy-in
    and the slot fill (pooling, or the volume's layout kernel), with no index search.  Result tensors
    of a sample stay valid until ``slots`` more samples have been submitted: consume (or clone) them inside the loop body, as
    the upstream loop does.  ``stats`` (optional dict) receives ``fallbacks`` / ``recaptures`` / ``eager_samples``."""
    import collections
    model.eval()
    pipe = None
    submitted = collections.deque()        # (data, ticket | None, eager result | None): search dispatched, dense not issued
    issued = collections.deque()           # (data, ticket, pinned host buffer, event): dense stage + metrics enqueued
    ncls_of = lambda out: out["pred_c"].shape[1]
    eager = 0

    def issue(item):
        """Dense stage of the oldest submitted sample onto its stream (no host wait) + metrics + the async host copy."""
        data, t, res = item
        if t is None:
            return (data, None, res, None)
        out = t.result(wait=False)
        ds = pipe.dense_streams[t.slot % pipe.ndense]
        gt, vm, po = data.get("gt_occ"), data.get("visible_mask"), data.get("points_occ")
        with torch.cuda.stream(ds):
            parts = []
            if gt is not None:
                gt.record_stream(ds)
                if vm is not None:
                    vm.record_stream(ds)
                both = model._metrics_launch(out, gt, vm)
                parts.append(both.reshape(-1))
            lseg = None
            if po:
                # the lidarseg labels + 16x16 matrix read the slot's pred_c: here, before the slot can be reused
                for p in po:
                    if p.is_cuda:
                        p.record_stream(ds)
                lseg = model._lidarseg_launch(out, po, data.get("img_metas"))
                if not model.metrics_on_device:
                    parts.append(lseg[1].reshape(-1))
            if out.get("fine_count") is not None:
                parts.append(out["fine_count"].reshape(-1).to(torch.int64))
            reval = rssim = None
            if model.render_eval:
                # the render stats read the slot's maps: here, before the slot can be reused; the float64 block rides in the
                # same pinned-host copy, bit for bit (viewed as int64)
                img = data.get("img_inputs", data.get("img"))
                gi, gdep = model.render_gt_img(img, data.get("precomputed")), data.get("gt_depths")
                for g in (gi, gdep):
                    if torch.is_tensor(g) and g.is_cuda:
                        g.record_stream(ds)
                reval = model._render_eval_launch(out, gi, gdep)
                # the SSIM block likewise, right behind the stats launch; in the host buffer it sits IN FRONT of the render stats
                rssim = model._render_ssim_launch(out, gi)
                if rssim is not None and not model.metrics_on_device:
                    parts.append(rssim.view(torch.int64).reshape(-1))
                if reval is not None and not model.metrics_on_device:
                    parts.append(reval[0].view(torch.int64).reshape(-1))
            host = ev = None
            if parts and not (model.metrics_on_device and gt is not None and len(parts) == 1):
                dev_buf = torch.cat(parts) if len(parts) > 1 else parts[0]
                host = torch.empty(dev_buf.shape, dtype=torch.int64, pin_memory=True)
                host.copy_(dev_buf, non_blocking=True)
            from . import streams as cstreams
            ev = cstreams.new_event()           # fires after the pinned-host copy above: a copy command, complete when it does
            ev.record(ds)
        return (data, t, (out, host, both if gt is not None else None, lseg, reval, rssim), ev)

    def finish(item):
        data, t, payload, ev = item
        if t is None:
            return data, payload
        out, host, both, lseg, reval, rssim = payload
        ev.synchronize()
        from . import core
        core.check_h2_overflow()
        out = dict(out)
        gt, vm = data.get("gt_occ"), data.get("visible_mask")
        C = ncls_of(out)
        nm = nl = 0                               # host buffer: [ metrics (nm) | lidarseg matrix (nl) | fine count | ssim block | render stats ]
        if gt is not None:
            nm = both.numel()
        if lseg is not None and not model.metrics_on_device:
            nl = lseg[1].numel()
        if out.get("fine_count") is not None and out.get("output_voxels_fine") is not None and not t.fallback:
            cf = model.pts_bbox_head.cascade_ratio
            n = int(host[nm + nl]) * cf ** 3
            # capacity-sized fine outputs of the captured form -> the exact-size tensors simple_test returns (views of the
            # slot's static buffers: no copy; the device-count kernels pack [3][n] at the start of the coords buffer)
            out["output_voxels_fine"] = [out["output_voxels_fine"][0][:n]]
            out["output_coords_fine"] = [out["output_coords_fine"][0].reshape(-1)[:3 * n].view(3, n)]
        out.update(output_voxels=out["pred_c"], target_voxels=gt)
        if gt is not None:
            m = both if model.metrics_on_device else host[:nm].numpy().reshape(both.shape).copy()
            out.update(model._metrics_finish(m, C, vm is not None))
        if lseg is not None:
            hist = lseg[1] if model.metrics_on_device else host[nm:nm + nl].numpy().copy()
            out.update(model._lidarseg_finish(lseg[0], hist, data["points_occ"]))
        nr = 0                                    # int64 words of the render stats at the end of the host buffer
        if reval is not None:
            block = reval[0]
            if not model.metrics_on_device:
                nr = block.numel()
                block = host[host.numel() - nr:].view(torch.float64).numpy().reshape(block.shape).copy()
            out.update(model._render_eval_finish(block, *reval[1:]))
        if rssim is not None:
            block = rssim
            if not model.metrics_on_device:
                end = host.numel() - nr
                block = host[end - block.numel():end].view(torch.float64).numpy().reshape(block.shape).copy()
            out.update(model._render_ssim_finish(block))
        return data, out

    try:
        with torch.no_grad():
            for data in data_iter:
                img = data.get("img_inputs", data.get("img"))
                fr = model.serving_frame(img=img, points=data.get("points"), img_metas=data.get("img_metas"),
                                         precomputed=data.get("precomputed"))
                if pipe is None:
                    pipe = model.serving(fr, slots=slots, dense_streams=dense_streams, ahead=ahead,
                                         render=bool(model.use_rendering and model.test_rendering))
                gt = data.get("gt_occ")
                X, Y, Z = pipe.grid
                cf = model.pts_bbox_head.cascade_ratio
                if gt is not None and model.pts_bbox_head.has_fine_branch and list(gt.shape[1:]) != [X * cf, Y * cf, Z * cf]:
                    # the captured scatter writes the default fine grid: this sample goes through simple_test's eager decode (a head
                    # without a fine branch scatters nothing: the metrics kernel resamples pred_c to any gt grid)
                    keep, model.graph_simple_test = model.graph_simple_test, False
                    try:
                        res = model.simple_test(**{("img" if k == "img_inputs" else k): v for k, v in data.items()})
                    finally:
                        model.graph_simple_test = keep
                    eager += 1
                    submitted.append((data, None, res))
                else:
                    submitted.append((data, pipe.submit(fr), None))
                while len(submitted) > pipe.ahead:
                    issued.append(issue(submitted.popleft()))
                while len(issued) > pipe.ndense:
                    yield finish(issued.popleft())
            while submitted:
                issued.append(issue(submitted.popleft()))
                while len(issued) > pipe.ndense:
                    yield finish(issued.popleft())
            while issued:
                yield finish(issued.popleft())
    finally:
        if pipe is not None:
            if stats is not None:
                stats.update(fallbacks=pipe.fallbacks, recaptures=pipe.recaptures, eager_samples=eager)
            pipe.drain()
            pipe.close()
