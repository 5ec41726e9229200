"""Pictures of saved occupancy predictions -- step 2 of the reference's predict-and-visualize workflow
(P/visualize/visualize_nusc.py: ``draw_nusc_occupancy`` and its ``__main__`` loop) -- rendered on the device, without mayavi, VTK
or an OpenGL context.

The reference draws every voxel with ``0 < label < 20`` (after relabelling 17 to 20 and writing the ego-car block over the centre)
as a cube of 95 % of the mean voxel size, coloured by a 19-row table, photographs the scene from eight cameras (the six of the
sample, a driving view, a bird's-eye view) and pastes the photographs beside the six input frames.  Here the draw volume and its bit
masks come from one kernel (``coocc_occ_view_prepare``) and the photographs from a ray caster (``coocc_occ_view_cast``,
csrc/occ_views.hip): per sample the nearest cube face inside the clipping range, flat-shaded by the face's direction, S x S samples a
pixel.  Mayavi's lighting and its anti-aliasing are NOT reproduced (a face here has one of four fixed shades, an edge is the mean
of its samples); the geometry -- which cubes, where, which colour row, which cameras, which layout -- is the reference's, and
tests/golden/occ_views_ref.npz holds what the unmodified reference hands to mayavi for it.  DESIGN.md 19.

Cube of voxel (i, j, k): centre ``origin + (index + 0.5) * voxel_size`` per axis, half edge ``0.5 * 0.95 * mean(voxel_size)``.
That is the reference's geometry for grids with X == Y and equal x / y voxel sizes and origins (nuScenes, OpenOccupancy): its
``meshgrid`` pairs the x coordinates with the second index and swaps them back when plotting, which is the identity only there; for
other grids this definition holds."""
import collections
import os
import pickle
import warnings

import numpy as np
import torch

from . import _lib
from ._lib import call, check, load, ptr

CAMERA_NAMES = ['CAM_FRONT_LEFT', 'CAM_FRONT', 'CAM_FRONT_RIGHT', 'CAM_BACK_LEFT', 'CAM_BACK', 'CAM_BACK_RIGHT']
VIEW_KEYS = CAMERA_NAMES + ['DRIVING_VIEW', 'BIRD_EYE_VIEW']
# the colour table: row v - 1 for draw value v (VTK maps vmin = 1 .. vmax = 19 onto the 19 rows)
PALETTE = np.array([
    [255, 120, 50, 255],        # barrier
    [255, 192, 203, 255],       # bicycle
    [255, 255, 0, 255],         # bus
    [0, 150, 245, 255],         # car
    [0, 255, 255, 255],         # construction_vehicle
    [255, 127, 0, 255],         # motorcycle
    [255, 0, 0, 255],           # pedestrian
    [255, 240, 150, 255],       # traffic_cone
    [135, 60, 0, 255],          # trailer
    [160, 32, 240, 255],        # truck
    [255, 0, 255, 255],         # driveable_surface
    [139, 137, 137, 255],       # other_flat
    [75, 0, 75, 255],           # sidewalk
    [150, 240, 80, 255],        # terrain
    [230, 230, 250, 255],       # manmade
    [0, 175, 0, 255],           # vegetation
    [0, 255, 127, 255],         # ego car
    [255, 99, 71, 255],         # ego car
    [0, 191, 255, 255],         # ego car
], np.uint8)
SHADE = (208, 208, 168, 168, 256, 128)        # faces +x -x +y -y +z -z, / 256
CONSTANT_F = 0.0055
ASPECT = 16.0 / 9.0
# the reference's hard-coded nuScenes grid
NUSC_PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
NUSC_OCC_SIZE = [200, 200, 16]
# the composed picture
CAM_IMG_SIZE, PRED_IMG_SIZE, SPACING = (480, 270), (1920, 1080), 10
BEV_WINDOW = (460, 1460)
CANVAS_SIZE = (CAM_IMG_SIZE[0] * 6 + 5 * SPACING, CAM_IMG_SIZE[1] * 2 + PRED_IMG_SIZE[1] + 2 * SPACING)      # 2930 x 1640


def palette_index(label):
    """Colour row of a draw value, None when it is not drawn."""
    return int(label) - 1 if 0 < int(label) < 20 else None


def layout():
    """name -> (left, top, width, height) on the canvas: ``input0`` .. ``input5`` and the eight view names."""
    (cw, ch), (pw, ph), sp = CAM_IMG_SIZE, PRED_IMG_SIZE, SPACING
    boxes = {}
    for i in range(6):
        x, y = (i % 3) * (cw + sp), (i // 3) * (ch + sp)
        boxes["input%d" % i] = (x, y, cw, ch)
        boxes[VIEW_KEYS[i]] = (x + 3 * (cw + sp), y, cw, ch)
    boxes["DRIVING_VIEW"] = (0, 2 * ch + 2 * sp, pw, ph)
    boxes["BIRD_EYE_VIEW"] = (pw + sp, 2 * ch + 2 * sp, BEV_WINDOW[1] - BEV_WINDOW[0], ph)
    return boxes


def cube_half(voxel_size):
    """Half the cube edge (float64): the reference's ``scale_factor`` -- the mean voxel size less 5 % -- halved.  ValueError when
    the edge exceeds the smallest voxel side: a cube must fit inside its own cell (the walk through the grid relies on it)."""
    vs = np.asarray(voxel_size, np.float64).reshape(-1)
    if vs.size == 1:
        vs = np.repeat(vs, 3)
    if vs.size != 3 or not np.all(np.isfinite(vs)) or np.any(vs <= 0):
        raise ValueError("visualize: voxel_size %r is not one or three positive sizes" % (voxel_size,))
    m = sum(vs) / 3
    edge = m - 0.05 * m
    if vs.min() < edge:
        raise ValueError("visualize: the cube edge %.6g (95 %% of the mean voxel size) exceeds the smallest voxel side %.6g: "
                         "the cube of a voxel would reach into its neighbours' cells" % (edge, vs.min()))
    return 0.5 * edge


def camera_positions(cam2lidar, constant_f=CONSTANT_F):
    """``cam_positions``, ``focal_positions`` [6,3] of the reference's ``__main__`` from the pickle's ``cam2lidar`` [6,4,4]."""
    cam2lidar = np.asarray(cam2lidar, np.float64)
    pos = (cam2lidar @ np.array([0., 0., 0., 1.]))[:, :3]
    foc = (cam2lidar @ np.array([0., 0., constant_f, 1.]))[:, :3]
    return pos, foc


def view_cameras(cam2lidar=None, cam_positions=None, focal_positions=None):
    """The eight cameras of ``draw_nusc_occupancy`` in VIEW_KEYS order: dicts of ``position``, ``focal_point``, ``view_angle`` (the
    vertical field of view, degrees), ``view_up``, ``clipping_range`` (along the view axis) -- the fields the reference sets."""
    if cam_positions is None:
        cam_positions, focal_positions = camera_positions(cam2lidar)
    cam_positions, focal_positions = np.asarray(cam_positions, np.float64), np.asarray(focal_positions, np.float64)
    cams = []
    for i in range(8):
        if i < 6:
            c = dict(position=cam_positions[i] - np.array([0.7, 1.3, 0.]), focal_point=focal_positions[i] - np.array([0.7, 1.3, 0.]),
                     view_angle=35 if i != 3 else 60, view_up=[0.0, 0.0, 1.0], clipping_range=[0.01, 300.])
        elif i == 6:
            c = dict(position=[0.75131739, -35.08337438, 16.71378558], focal_point=[0.75131739, -34.21734897, 16.21378558],
                     view_angle=40.0, view_up=[0.0, 0.0, 1.0], clipping_range=[0.01, 300.])
        else:
            c = dict(position=[0.75131739, 0.78265103, 93.21378558], focal_point=[0.75131739, 0.78265103, 92.21378558],
                     view_angle=40.0, view_up=[0., 1., 0.], clipping_range=[0.01, 400.])
        cams.append({k: np.asarray(v, np.float64) for k, v in c.items()})
    return cams


def view_rows(cameras, col0=0):
    """Camera dicts -> the fp32 [V,16] rows ``coocc_occ_view_cast`` reads: eye, fwd, right * tan_x, up * tan_y, near, far, col0, 0.
    The basis is made in float64 and rounded once; tan_x = tan_y * 16 / 9."""
    rows = np.zeros((len(cameras), 16), np.float32)
    for v, c in enumerate(cameras):
        pos, up0 = np.asarray(c["position"], np.float64), np.asarray(c["view_up"], np.float64)
        fwd = np.asarray(c["focal_point"], np.float64) - pos
        n = np.sqrt((fwd * fwd).sum())
        if not n > 0:
            raise ValueError("visualize: view %d: position and focal point coincide" % v)
        fwd = fwd / n
        right = np.cross(fwd, up0)
        n = np.sqrt((right * right).sum())
        if not n > 0:
            raise ValueError("visualize: view %d: view_up is parallel to the view axis" % v)
        right = right / n
        up = np.cross(right, fwd)
        tan_y = np.tan(np.radians(float(c["view_angle"])) / 2)
        rows[v, 0:3], rows[v, 3:6], rows[v, 6:9], rows[v, 9:12] = pos, fwd, right * (tan_y * ASPECT), up * tan_y
        rows[v, 12:14] = np.asarray(c["clipping_range"], np.float64)
        rows[v, 14] = col0
    return rows


def _labels_on_device(labels, device=None):
    if isinstance(labels, np.ndarray):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        labels = torch.from_numpy(np.ascontiguousarray(labels)).to(device)
    _lib.require_gpu(labels, "labels")
    if labels.dim() == 4 and labels.shape[0] == 1:
        labels = labels[0]
    if labels.dim() != 3:
        raise ValueError("visualize: labels %s is not an [X, Y, Z] volume" % (tuple(labels.shape),))
    if labels.dtype not in (torch.uint8, torch.int64):
        labels = labels.to(torch.int64)
    return labels.contiguous()


def _call(name, *args):
    """``_lib.call`` for an entry whose non-negative return value is information (``call`` raises on any non-zero value)."""
    fn = getattr(load(), name)
    dev = _lib._device_of(args)
    with torch.cuda.device(dev):
        rc = int(fn(*args, _lib.stream(dev)))
    if rc < 0:
        check(rc)
    return rc


def prepare(labels, device=None):
    """labels [X,Y,Z] (uint8 or int64, device tensor or numpy) -> (draw uint8 [X,Y,Z], masks uint8 [n]) on the device, one launch."""
    labels = _labels_on_device(labels, device)
    X, Y, Z = labels.shape
    need = int(load().coocc_occ_view_prepare(None, 0, X, Y, Z, None, None, 0, None))
    if need < 0:
        check(need)
    draw = torch.empty((X, Y, Z), dtype=torch.uint8, device=labels.device)
    masks = torch.empty(need, dtype=torch.uint8, device=labels.device)
    call("coocc_occ_view_prepare", ptr(labels), int(labels.dtype == torch.int64), X, Y, Z, ptr(draw), ptr(masks), need)
    return draw, masks


def draw_volume(labels, device=None):
    """The volume the reference plots: label 17 -> 20, the ego-car block (17 / 18 / 19) over the centre; drawn iff 0 < v < 20."""
    return prepare(labels, device)[0]


Views = collections.namedtuple("Views", "rgb ids faces t reads cell_bits")


def cast_views(draw, masks, rows, vox_origin, voxel_size, size, samples=1, frame=None, details=False, lds_budget_bytes=0):
    """``coocc_occ_view_cast`` on a prepared volume: ``rows`` fp32 [V,16] (``view_rows``), ``size`` = (W, H) pixels written per
    view, ``frame`` = (FW, FH) the full frame the rays are laid out on (default: ``size``).  -> rgb uint8 [V,H,W,3] on the device.
    With ``details`` a ``Views`` tuple: rgb; per sample, [V, H*S, W*S], ids int32 (the voxel's linear index, -1: none), faces uint8
    (0 +x, 1 -x, 2 +y, 3 -y, 4 +z, 5 -z; 255) and t fp32 (the depth along the view axis, +inf); reads uint32 [V, H*S, W*S, 2], the
    brick flags and column words the sample's walk read; cell_bits, where the column words were read: 'lds' or 'global' (the
    brick flags are always in LDS)."""
    X, Y, Z = draw.shape
    (W, H), S = [int(v) for v in size], int(samples)
    FW, FH = [int(v) for v in (frame if frame is not None else size)]
    vs = np.asarray(voxel_size, np.float64).reshape(-1)
    vs = np.repeat(vs, 3) if vs.size == 1 else vs
    grid = np.concatenate([np.asarray(vox_origin, np.float64).reshape(3), vs, [cube_half(vs)]]).astype(np.float32)
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 16)
    pal = np.ascontiguousarray(PALETTE[:, :3])
    V, dev = rows.shape[0], draw.device
    rgb = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev)
    ids = faces = t = reads = None
    if details:
        ids = torch.empty((V, H * S, W * S), dtype=torch.int32, device=dev)
        faces = torch.empty((V, H * S, W * S), dtype=torch.uint8, device=dev)
        t = torch.empty((V, H * S, W * S), dtype=torch.float32, device=dev)
        reads = torch.empty((V, H * S, W * S, 2), dtype=torch.int32, device=dev)          # the entry's uint32, never above 2^31
    rc = _call("coocc_occ_view_cast", ptr(draw, torch.uint8), ptr(masks, torch.uint8), X, Y, Z, grid.ctypes.data, rows.ctypes.data, V, H, W, S,
               FW, FH, pal.ctypes.data, int(lds_budget_bytes), ptr(rgb), ptr(ids), ptr(faces), ptr(t), ptr(reads))
    return Views(rgb, ids, faces, t, reads, "global" if rc == 1 else "lds") if details else rgb


def render_views(labels, cam2lidar, vox_origin, voxel_size, views=None, size=CAM_IMG_SIZE, samples=None, window=None, cameras=None,
                 details=False, lds_budget_bytes=0, device=None):
    """Photographs of a label volume.  ``views``: indices into VIEW_KEYS (default all eight) of the cameras made from ``cam2lidar``
    [6,4,4], or pass ``cameras`` (dicts as ``view_cameras`` returns) and leave ``cam2lidar`` None.  ``size`` = (W, H) of the full
    frame, ``samples`` S x S per pixel (default 4 up to 480 x 270, else 2), ``window`` = (c0, c1): only the frame's columns c0 .. c1 - 1
    are rendered.  -> device uint8 [V, H, c1 - c0, 3], or with ``details`` a ``Views`` tuple as ``cast_views`` returns."""
    if cameras is None:
        cams = view_cameras(cam2lidar)
        cameras = [cams[i] for i in (range(8) if views is None else views)]
    W, H = [int(v) for v in size]
    S = int(samples) if samples is not None else (4 if W * H <= CAM_IMG_SIZE[0] * CAM_IMG_SIZE[1] else 2)
    c0, c1 = (0, W) if window is None else [int(v) for v in window]
    draw, masks = prepare(labels, device)
    outs = []
    for v0 in range(0, len(cameras), 8):                   # the entry takes eight views a launch
        outs.append(cast_views(draw, masks, view_rows(cameras[v0:v0 + 8], c0), vox_origin, voxel_size, (c1 - c0, H), S, (W, H), details,
                               lds_budget_bytes))
    if len(outs) == 1:
        return outs[0]
    return Views(*[torch.cat(o) for o in zip(*[o[:5] for o in outs])], outs[0].cell_bits) if details else torch.cat(outs)


def _image_writer(what):
    try:
        import cv2
        return (lambda f, a: cv2.imwrite(f, np.ascontiguousarray(a[..., ::-1]))), ".png"          # cv2 takes BGR; the files are RGB
    except ImportError:
        try:
            from PIL import Image
            return (lambda f, a: Image.fromarray(a).save(f)), ".png"
        except ImportError:
            warnings.warn("%s: neither cv2 nor PIL imports; writing the pictures as .npy arrays" % what)
            return (lambda f, a: np.save(f, a)), ".npy"


def compose(input_imgs, panels):
    """The reference's canvas: black 2930 x 1640, the six inputs (PIL images or uint8 [270,480,3] arrays; missing ones stay black)
    left of the six camera photographs in the two top rows, the driving view and the bird's-eye window below.  ``panels``: name ->
    uint8 [h,w,3] array.  -> uint8 [1640, 2930, 3]."""
    canvas = np.zeros((CANVAS_SIZE[1], CANVAS_SIZE[0], 3), np.uint8)
    boxes = layout()

    def paste(name, img):
        x, y, w, h = boxes[name]
        a = np.asarray(img)
        if a.ndim == 2:
            a = np.repeat(a[..., None], 3, 2)
        h, w = min(h, a.shape[0]), min(w, a.shape[1])        # PIL's paste clips at the canvas; an input never leaves its box here
        canvas[y:y + h, x:x + w] = a[:h, :w, :3]
    for i, img in enumerate(list(input_imgs or [])[:6]):
        if img is not None:
            paste("input%d" % i, img)
    for name, a in panels.items():
        paste(name, a)
    return canvas


def draw_nusc_occupancy(input_imgs, voxels, vox_origin, voxel_size=0.5, grid=None, pred_lidarseg=None, target_lidarseg=None,
                        save_folder=None, cat_save_file=None, cam_positions=None, focal_positions=None, cam2lidar=None,
                        lds_budget_bytes=0):
    """The reference's function with its arguments (``grid``, ``pred_lidarseg`` and ``target_lidarseg`` are as unused as there), plus
    ``cam2lidar`` as an alternative to the two position arrays.  Renders the six camera views at 480 x 270 (4 x 4 samples a pixel),
    the driving view at 1920 x 1080 and columns 460:1460 of the bird's-eye view (2 x 2), composes the canvas and returns it (uint8
    [1640,2930,3]).  With ``save_folder`` the eight ``<VIEW>.png`` are written there, with ``cat_save_file`` the canvas -- through
    cv2 or PIL, whichever imports, else as ``.npy`` with a warning; the files hold RGB, as the reference's do."""
    cams = view_cameras(cam2lidar, cam_positions, focal_positions)
    draw, masks = prepare(voxels)
    (cw, ch), (pw, ph) = CAM_IMG_SIZE, PRED_IMG_SIZE
    small = cast_views(draw, masks, view_rows(cams[:6]), vox_origin, voxel_size, (cw, ch), 4, None, False, lds_budget_bytes)
    drive = cast_views(draw, masks, view_rows(cams[6:7]), vox_origin, voxel_size, (pw, ph), 2, None, False, lds_budget_bytes)
    bev = cast_views(draw, masks, view_rows(cams[7:8], BEV_WINDOW[0]), vox_origin, voxel_size, (BEV_WINDOW[1] - BEV_WINDOW[0], ph), 2,
                     (pw, ph), False, lds_budget_bytes)
    small, drive, bev = small.cpu().numpy(), drive.cpu().numpy(), bev.cpu().numpy()
    panels = {VIEW_KEYS[i]: small[i] for i in range(6)}
    panels["DRIVING_VIEW"], panels["BIRD_EYE_VIEW"] = drive[0], bev[0]
    canvas = compose(input_imgs, panels)
    if save_folder is not None or cat_save_file is not None:
        writer, ext = _image_writer("draw_nusc_occupancy")
        if save_folder is not None:
            os.makedirs(save_folder, exist_ok=True)
            for name in VIEW_KEYS:
                writer(os.path.join(save_folder, name + ext), panels[name])
        if cat_save_file is not None:
            os.makedirs(os.path.dirname(os.path.abspath(cat_save_file)), exist_ok=True)
            writer(cat_save_file if ext == ".png" else os.path.splitext(cat_save_file)[0] + ext, canvas)
    return canvas


def grid_of(occ_size=None, pc_range=None):
    """(vox_origin, voxel_size) float64 of a grid: the reference's ``__main__`` arithmetic."""
    occ_size = NUSC_OCC_SIZE if occ_size is None else occ_size
    r = NUSC_PC_RANGE if pc_range is None else pc_range
    return np.array(r[:3], np.float64), np.array([(r[3 + a] - r[a]) / occ_size[a] for a in range(3)])


def visualize_saved(pred_dir, save_path, occ_size=None, pc_range=None):
    """The reference's loop: every ``<token>.pkl`` of ``pred_dir`` (``apis.save_output_nuscenes``) -> ``<save_path>/<token>_assets/``
    and ``<save_path>/<token>_cat_vis.png``; samples whose picture exists are skipped.  Returns the pictures written."""
    origin, vs = grid_of(occ_size, pc_range)
    done = []
    for sample_file in sorted(os.listdir(pred_dir)):
        if not sample_file[-3:] == 'pkl':
            continue
        token = sample_file.split('.')[0]
        cat_save_file = os.path.join(save_path, '{}_cat_vis.png'.format(token))
        if os.path.exists(cat_save_file):
            continue
        with open(os.path.join(pred_dir, sample_file), 'rb') as f:
            data = pickle.load(f)
        draw_nusc_occupancy(data['img_canvas'], data['pred_voxels'], origin, vs, grid=np.array(NUSC_OCC_SIZE if occ_size is None else occ_size),
                            save_folder=os.path.join(save_path, '{}_assets'.format(token)), cat_save_file=cat_save_file,
                            cam2lidar=data['cam2lidar'])
        done.append(cat_save_file)
    return done
