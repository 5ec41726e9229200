"""The occupancy pictures (co_occ_amd/visualize.py, csrc/occ_views.hip) restated in numpy, independent of the package: the draw
volume and the cameras of the reference's draw_nusc_occupancy, then a BRUTE-FORCE cast -- every sample against every drawn cube, no
grid walk -- in fp32 with the operation order include/coocc_hip.h states for coocc_occ_view_cast, and the same cast in float64 as
the anchor.  The kernel's ids, faces, t and bytes must equal the fp32 cast exactly (tests/test_gpu_occ_views.py); the fp32 cast may
differ from the float64 one in (voxel, face) on at most 0.1 % of a case's samples (tests/test_occ_views_host.py).

CASES is the case list of both files; a case's reference is computed once (reference(name)) and shared."""
import functools

import numpy as np

VIEW_KEYS = ['CAM_FRONT_LEFT', 'CAM_FRONT', 'CAM_FRONT_RIGHT', 'CAM_BACK_LEFT', 'CAM_BACK', 'CAM_BACK_RIGHT', 'DRIVING_VIEW',
             'BIRD_EYE_VIEW']
SHADE = np.array([208, 208, 168, 168, 256, 128], np.int64)      # faces +x -x +y -y +z -z
PARALLEL = 1e-30
ASPECT = 16.0 / 9.0


def draw_volume(labels):
    """labels [X,Y,Z] -> uint8 draw volume: 17 -> 20, then the ego-car block, by the reference's own index arithmetic."""
    w, h, z = labels.shape
    flat = labels.astype(np.uint8).reshape(-1).copy()
    flat[flat == 17] = 20
    car_x = np.arange(w // 2 - 2 - 4, w // 2 - 2 + 4)
    car_y = np.arange(h // 2 - 2 - 4, h // 2 - 2 + 4)
    car_z = np.arange(z // 2 - 2 - 3, z // 2 - 2 + 3)
    xx, yy, zz = np.meshgrid(car_x, car_y, car_z)
    lab = np.zeros([8, 8, 6], np.uint8)
    lab[:3, :, :2], lab[3:6, :, :2], lab[6:, :, :2] = 17, 18, 19
    lab[:3, :, 2:4], lab[3:6, :, 2:4], lab[6:, :, 2:4] = 18, 19, 17
    lab[:3, :, 4:], lab[3:6, :, 4:], lab[6:, :, 4:] = 19, 17, 18
    flat[xx.flatten() * h * z + yy.flatten() * z + zz.flatten()] = lab.flatten()
    return flat.reshape(w, h, z)


def cube_half(voxel_size):
    """Half the cube edge: the reference's scale_factor (mean voxel size less 5 %) halved, in float64."""
    m = sum(np.asarray(voxel_size, np.float64)) / 3
    return 0.5 * (m - 0.05 * m)


def cameras(cam2lidar, constant_f=0.0055):
    """The eight cameras of draw_nusc_occupancy from the [6,4,4] cam2lidar of the pickle: dicts of position, focal_point,
    view_angle, view_up, clipping_range."""
    pos = (cam2lidar @ np.array([0., 0., 0., 1.]))[:, :3]
    foc = (cam2lidar @ np.array([0., 0., constant_f, 1.]))[:, :3]
    out = []
    for i in range(8):
        if i < 6:
            c = dict(position=pos[i] - np.array([0.7, 1.3, 0.]), focal_point=foc[i] - np.array([0.7, 1.3, 0.]),
                     view_angle=35 if i != 3 else 60, view_up=[0.0, 0.0, 1.0], clipping_range=[0.01, 300.])
        elif i == 6:
            c = dict(position=[0.75131739, -35.08337438, 16.71378558], focal_point=[0.75131739, -34.21734897, 16.21378558],
                     view_angle=40.0, view_up=[0.0, 0.0, 1.0], clipping_range=[0.01, 300.])
        else:
            c = dict(position=[0.75131739, 0.78265103, 93.21378558], focal_point=[0.75131739, 0.78265103, 92.21378558],
                     view_angle=40.0, view_up=[0., 1., 0.], clipping_range=[0.01, 400.])
        out.append({k: np.asarray(v, np.float64) for k, v in c.items()})
    return out


def view_rows(cams, col0=0):
    """fp32 [V,16] rows of coocc_occ_view_cast from camera dicts: the basis in float64, rounded once."""
    rows = np.zeros((len(cams), 16), np.float32)
    for v, c in enumerate(cams):
        fwd = c["focal_point"] - c["position"]
        fwd = fwd / np.sqrt((fwd * fwd).sum())
        right = np.cross(fwd, c["view_up"])
        right = right / np.sqrt((right * right).sum())
        up = np.cross(right, fwd)
        tan_y = np.tan(np.radians(float(c["view_angle"])) / 2)
        rows[v, 0:3], rows[v, 3:6], rows[v, 6:9], rows[v, 9:12] = c["position"], fwd, right * (tan_y * ASPECT), up * tan_y
        rows[v, 12:14] = c["clipping_range"]
        rows[v, 14] = col0
    return rows


def cast_samples(draw, origin, voxel_size, row, gx, gy, S, FW, FH, dt=np.float32, chunk=2048):
    """Samples (gx[n], gy[n]) of the FW*S x FH*S sample frame of ONE view (``row`` fp32 [16]) against every drawn cube.
    -> ids int32 [n] (-1), faces uint8 [n] (255), t [n] (+inf), in ``dt`` arithmetic: fp32 is the kernel's definition, float64 the
    anchor (same fp32 inputs, exact products)."""
    lin = np.flatnonzero((draw.reshape(-1) > 0) & (draw.reshape(-1) < 20))
    ijk = np.stack(np.unravel_index(lin, draw.shape), 0)
    org, vs = np.asarray(origin, np.float32).astype(dt), np.asarray(voxel_size, np.float32).astype(dt)
    half = dt(np.float32(cube_half(voxel_size)))
    ctr = [org[a] + (ijk[a].astype(dt) + dt(0.5)) * vs[a] for a in range(3)]
    lo, hi = [c - half for c in ctr], [c + half for c in ctr]
    rw = dt(np.float32(1.0 / (FW * S))) if dt is np.float32 else 1.0 / (FW * S)
    rh = dt(np.float32(1.0 / (FH * S))) if dt is np.float32 else 1.0 / (FH * S)
    gx, gy = np.asarray(gx, np.int64), np.asarray(gy, np.int64)
    ids, faces, ts = np.full(gx.size, -1, np.int32), np.full(gx.size, 255, np.uint8), np.full(gx.size, np.inf, dt)
    r = np.asarray(row, np.float32).astype(dt)
    e, fwd, R, U, near, far = r[0:3], r[3:6], r[6:9], r[9:12], r[12], r[13]
    u = (2 * gx + 1 - FW * S).astype(dt) * rw
    w = (FH * S - 2 * gy - 1).astype(dt) * rh
    d = [(fwd[a] + u * R[a]) + w * U[a] for a in range(3)]
    for s in range(0, u.size if lin.size else 0, chunk):
        n = min(chunk, u.size - s)
        ten = np.full((n, lin.size), -np.inf, dt)
        tex = np.full((n, lin.size), np.inf, dt)
        aen, aex = np.zeros((n, lin.size), np.int8), np.zeros((n, lin.size), np.int8)
        miss = np.zeros((n, lin.size), bool)
        for a in range(3):
            da = d[a][s:s + n]
            par = np.abs(da) < dt(PARALLEL)
            inv = (dt(1.0) / np.where(par, dt(1.0), da))[:, None]
            ta, tb = (lo[a][None, :] - e[a]) * inv, (hi[a][None, :] - e[a]) * inv
            tn, tf = np.minimum(ta, tb), np.maximum(ta, tb)
            outside = ((e[a] < lo[a]) | (e[a] > hi[a]))[None, :]
            miss |= par[:, None] & outside
            live = ~par[:, None]
            g = live & (tn > ten)                                              # strictly: the lowest axis among equals stays
            ten[g], aen[g] = tn[g], a
            g = live & (tf < tex)
            tex[g], aex[g] = tf[g], a
        hit = ~miss & (ten <= tex)
        front = ten >= near
        t = np.where(front, ten, tex)
        hit &= (front | (tex >= near)) & (t <= far)
        ax = np.where(front, aen, aex)
        dpos = np.stack([dd[s:s + n] for dd in d], 0) > 0                      # [3, n]
        pos = np.take_along_axis(dpos, ax.astype(np.int64).T, 0).T            # d[ax] > 0 per (sample, cube)
        face = 2 * ax + np.where(front, pos, ~pos)
        t = np.where(hit, t, np.inf).astype(dt)
        best = np.argmin(t, 1)                                                 # the first minimum: the lowest linear index
        rr = np.arange(n)
        ok = hit[rr, best]
        ids[s:s + n] = np.where(ok, lin[best], -1)
        faces[s:s + n] = np.where(ok, face[rr, best], 255)
        ts[s:s + n] = np.where(ok, t[rr, best], np.inf)
    return ids, faces, ts


def cast(draw, origin, voxel_size, rows, H, W, S, FW, FH, dt=np.float32):
    """Every sample of every view: ids, faces, t [V, H*S, W*S]; view v writes the frame's columns col0 .. col0 + W - 1."""
    out = []
    for v in range(rows.shape[0]):
        gx, gy = np.meshgrid(int(rows[v, 14]) * S + np.arange(W * S), np.arange(H * S))
        out.append([a.reshape(H * S, W * S) for a in cast_samples(draw, origin, voxel_size, rows[v], gx.reshape(-1), gy.reshape(-1), S,
                                                                  FW, FH, dt)])
    return tuple(np.stack(a) for a in zip(*out))


def shade(draw, palette, ids, faces, S):
    """Sample colours -> uint8 pixels [V,H,W,3]: (palette * shade + 128) >> 8, 255 without a hit, rounded mean of S x S samples."""
    V, HS, WS = ids.shape
    hit = ids >= 0
    cls = draw.reshape(-1)[np.where(hit, ids, 0)].astype(np.int64) - 1
    col = (np.asarray(palette, np.int64)[cls, :3] * SHADE[np.where(hit, faces, 0)][..., None] + 128) >> 8
    col = np.where(hit[..., None], col, 255)
    sums = col.reshape(V, HS // S, S, WS // S, S, 3).sum((2, 4))
    return ((sums + (S * S) // 2) // (S * S)).astype(np.uint8)


# the layout of the composed picture: name -> (left, top, width, height) on the 2930 x 1640 canvas
CAM_W, CAM_H, PRED_W, PRED_H, SPACING = 480, 270, 1920, 1080, 10
CANVAS_W, CANVAS_H = CAM_W * 6 + 5 * SPACING, CAM_H * 2 + PRED_H + 2 * SPACING
BEV_WINDOW = (460, 1460)


def layout():
    boxes = {}
    for i in range(6):
        x, y = (i % 3) * (CAM_W + SPACING), (i // 3) * (CAM_H + SPACING)
        boxes["input%d" % i] = (x, y, CAM_W, CAM_H)
        boxes[VIEW_KEYS[i]] = (x + 3 * (CAM_W + SPACING), y, CAM_W, CAM_H)
    boxes["DRIVING_VIEW"] = (0, 2 * CAM_H + 2 * SPACING, PRED_W, PRED_H)
    boxes["BIRD_EYE_VIEW"] = (PRED_W + SPACING, 2 * CAM_H + 2 * SPACING, BEV_WINDOW[1] - BEV_WINDOW[0], PRED_H)
    return boxes


# ---------------------------------------------------------------------------------------------------------------- the cases
def rig(radius=1.0, height=2.2):
    """A six-camera rig like nuScenes': cameras on a circle looking outwards (camera z forward, y down), [6,4,4] float64."""
    out = np.repeat(np.eye(4)[None], 6, 0)
    for i, yaw in enumerate(np.radians([55.0, 0.0, -55.0, 110.0, 180.0, -110.0])):
        f = np.array([np.cos(yaw), np.sin(yaw), 0.0])                  # lidar x forward, y left
        down = np.array([0.0, 0.0, -1.0])
        out[i, :3, 0], out[i, :3, 1], out[i, :3, 2] = np.cross(down, f), down, f
        out[i, :3, 3] = radius * f + np.array([0.0, 0.0, height])
    return out


def labels_random(shape, fill, seed):
    """Seeded labels with every class, 0, 17 and 255 present; ``fill``: the share of non-zero voxels."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(1, 18, size=shape).astype(np.uint8)
    lab[rng.random(shape) >= fill] = 0
    flat = lab.reshape(-1)
    flat[rng.choice(flat.size, flat.size // 50, replace=False)] = 255
    flat[:18] = np.arange(18)
    flat[18] = 255
    return lab


def _cam(position, focal_point, view_angle=40.0, view_up=(0., 0., 1.), clipping_range=(0.01, 300.)):
    return {k: np.asarray(v, np.float64) for k, v in dict(position=position, focal_point=focal_point, view_angle=view_angle,
                                                         view_up=view_up, clipping_range=clipping_range).items()}


def _grid(shape, vs=(0.5, 0.5, 0.5)):
    vs = np.asarray(vs, np.float64)
    return -0.5 * np.asarray(shape) * vs + np.array([0.0, 0.0, 1.0]), vs


def _ego_eye(shape, origin, vs):
    """A point inside the cube of an ego-car voxel, off its centre."""
    idx = np.array([shape[0] // 2 - 3, shape[1] // 2 - 3, shape[2] // 2 - 3])
    return origin + (idx + 0.5) * vs + np.array([0.07, -0.05, 0.03])


def case(name):
    """-> dict(labels, origin, voxel_size, cams, H, W, S, FW, FH, col0, lds_budget, cell_bits: where the column words are read)."""
    c = dict(H=36, W=64, S=1, FW=None, FH=None, col0=0, lds_budget=0, cell_bits="lds")
    g16 = _grid((16, 16, 16))
    if name == "grid12":            # the smallest grid the ego car fits
        shape = (12, 12, 16)
        o, v = _grid(shape)
        c.update(labels=labels_random(shape, 0.3, 1), origin=o, voxel_size=v, cams=cameras(rig())[1:8:3], S=2)
    elif name == "grid16":          # the golden's grid and all eight of its cameras
        c.update(labels=labels_random((16, 16, 16), 0.3, 2), origin=g16[0], voxel_size=g16[1], cams=cameras(rig()))
    elif name == "grid20x11":       # 4400 cell bits: no multiple of 64; 11 of the 16 bits of a column word
        shape = (20, 20, 11)
        o, v = _grid(shape, (0.512, 0.512, 0.5))
        c.update(labels=labels_random(shape, 0.3, 3), origin=o, voxel_size=v, cams=cameras(rig())[0:8:2], H=37, W=70, S=2)
    elif name == "odd70x37":        # no tile multiple, one sample a pixel
        c.update(labels=labels_random((16, 16, 16), 0.3, 4), origin=g16[0], voxel_size=g16[1], cams=cameras(rig())[2:8:2], H=37, W=70)
    elif name == "bev_odd":         # odd frame: the centre sample's ray is exactly (0, 0, -1); the eye over a cube's centre line
        o, v = g16
        eye = o + (np.array([5, 9, 0]) + 0.5) * v
        c.update(labels=labels_random((16, 16, 16), 0.5, 5), origin=o, voxel_size=v, H=37, W=65,
                 cams=[_cam([eye[0], eye[1], 30.0], [eye[0], eye[1], 29.0], view_up=(0., 1., 0.), clipping_range=(0.01, 400.))])
    elif name == "window":          # columns 20 .. 51 of a 64-wide frame
        c.update(labels=labels_random((16, 16, 16), 0.3, 6), origin=g16[0], voxel_size=g16[1], cams=cameras(rig())[6:8], W=32, FW=64, col0=20,
                 S=2)
    elif name == "eye_inside":      # the eye inside an ego-car cube: its samples see that cube's exit faces
        o, v = g16
        eye = _ego_eye((16, 16, 16), o, v)
        c.update(labels=labels_random((16, 16, 16), 0.3, 7), origin=o, voxel_size=v,
                 cams=[_cam(eye, eye + np.array([1.0, 0.3, 0.1])), _cam(eye, eye + np.array([-0.2, -1.0, 0.4]), 60.0)])
    elif name == "far_eye":         # far outside the grid; the wide view's border rays miss it altogether
        o, v = g16
        c.update(labels=labels_random((16, 16, 16), 0.3, 8), origin=o, voxel_size=v,
                 cams=[_cam([60.0, 45.0, 30.0], [0.0, 0.0, 1.0], 12.0), _cam([-50.0, 3.0, 2.0], [0.0, 0.0, 1.0], 100.0),
                       _cam([0.0, 0.0, 40.0], [0.0, 30.0, 40.0], 30.0)])
    elif name == "empty":           # the ego car alone
        c.update(labels=np.zeros((16, 16, 16), np.uint8), origin=g16[0], voxel_size=g16[1], cams=cameras(rig())[0:8:3], S=2)
    elif name == "full":            # every voxel drawn (label 17 and the unknowns aside)
        lab = labels_random((16, 16, 16), 1.0, 9)
        c.update(labels=lab, origin=g16[0], voxel_size=g16[1], cams=cameras(rig())[5:8])
    elif name == "near_far":        # near cuts cubes in front of the eye open, far drops the back of the scene
        c.update(labels=labels_random((16, 16, 16), 0.4, 10), origin=g16[0], voxel_size=g16[1],
                 cams=[_cam([-6.0, -5.0, 2.0], [0.0, 0.0, 1.0], clipping_range=(4.3, 8.1)),
                       _cam([0.3, 0.2, 9.0], [0.3, 0.2, 8.0], view_up=(0., 1., 0.), clipping_range=(6.2, 7.4))])
    elif name == "global_bits":     # 32 x 32 x 16 with a 64-byte LDS budget: the column words stay in memory
        shape = (32, 32, 16)
        o, v = _grid(shape)
        c.update(labels=labels_random(shape, 0.1, 11), origin=o, voxel_size=v, cams=cameras(rig())[1:8:2], lds_budget=64, cell_bits="global")
    elif name == "deep40":          # 40 cells deep: three words a column, the walk crosses from word to word
        shape = (24, 20, 40)
        o, v = _grid(shape, (0.4, 0.4, 0.4))
        lab = labels_random(shape, 0.06, 12)
        lab[:, :, 16:32][np.random.default_rng(13).random((24, 20, 16)) < 0.9] = 0          # a nearly empty middle word
        c.update(labels=lab, origin=o, voxel_size=v, H=37, W=70,
                 cams=cameras(rig(1.0, 4.0))[0:6:5] + [_cam([9.0, -7.0, 11.0], [0.0, 0.0, 1.0]),
                                                        _cam([0.3, 0.2, 14.0], [0.3, 0.2, 13.0], view_up=(0., 1., 0.)),
                                                        _cam([1.0, 0.5, -9.5], [0.2, 0.1, 1.0], 50.0)])
    elif name == "lds80k":          # 18 KiB of column words: above the default budget; staged in the 80 KiB form on request
        shape = (96, 96, 16)
        o, v = _grid(shape)
        c.update(labels=labels_random(shape, 0.04, 14), origin=o, voxel_size=v, cams=cameras(rig())[4:8:3], lds_budget=81920)
    else:
        raise KeyError(name)
    c["FW"], c["FH"] = c["FW"] or c["W"], c["FH"] or c["H"]
    return c


CASES = ["grid12", "grid16", "grid20x11", "odd70x37", "bev_odd", "window", "eye_inside", "far_eye", "empty", "full", "near_far",
         "global_bits", "deep40", "lds80k"]


@functools.lru_cache(maxsize=None)
def reference(name, dt=np.float32):
    """(case, draw, rows, ids, faces, t) of a case, computed once; the arrays are read-only."""
    c = case(name)
    draw = draw_volume(c["labels"])
    rows = view_rows(c["cams"], c["col0"])
    out = cast(draw, c["origin"], c["voxel_size"], rows, c["H"], c["W"], c["S"], c["FW"], c["FH"], dt)
    for a in (draw, rows) + out:
        a.setflags(write=False)
    return (c, draw, rows) + out


def read_png(path):
    """An 8-bit RGB / RGBA / grey PNG decoded with zlib alone -- no imaging library, so what a writer put into the file shows as it
    is -> uint8 [h, w, channels]."""
    import struct
    import zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head = 8, [], None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        pos += 12 + n
    w, h, depth, colour, _, _, interlace = head
    assert depth == 8 and interlace == 0 and colour in (0, 2, 6)
    ch = {0: 1, 2: 3, 6: 4}[colour]
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(h, 1 + w * ch)
    out = np.zeros((h, w * ch), np.uint8)
    prev = np.zeros(w * ch, np.int64)
    for y in range(h):
        f, line = int(raw[y, 0]), raw[y, 1:].astype(np.int64)
        if f == 0:
            cur = line
        elif f == 2:
            cur = (line + prev) & 255
        elif f == 1:                                  # sub: a running sum per channel
            cur = (np.cumsum(line.reshape(w, ch), 0) & 255).reshape(-1)
        else:                                         # average, Paeth: byte by byte
            cur = np.zeros(w * ch, np.int64)
            pl, ll = prev.tolist(), line.tolist()
            cl = [0] * (w * ch)
            for i in range(w * ch):
                a = cl[i - ch] if i >= ch else 0
                b = pl[i]
                if f == 3:
                    pred = (a + b) >> 1
                else:
                    c = pl[i - ch] if i >= ch else 0
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cl[i] = (ll[i] + pred) & 255
            cur = np.asarray(cl, np.int64)
        out[y] = cur
        prev = cur
    return out.reshape(h, w, ch)
