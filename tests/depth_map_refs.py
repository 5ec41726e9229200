"""References of the LiDAR depth map tests (test_depth_maps_host.py, test_gpu_depth_maps.py), written apart from
co_occ_amd/depth_maps.py:
  - the numpy float32 restatement of the reference's projection (every product rounded, sums left to right, IEEE division) and of the
    map definition: a pixel holds the minimum depth of the valid points that round to it, 0 where there is none;
  - an eager-torch form of the reference's projection and fill (the host test holds the restatement against it, live);
  - the rigs, clouds and cases both test files share.
Nothing here imports the package."""
import numpy as np
import torch

import image_input_refs as R

F = np.float32


# ------------------------------------------------------------------ the restatement
def project(points, inv_rots, trans, intrins, post_rots, post_trans):
    """(u, v, d) float32 [P, N] of points [P, >=3] in N cameras.  numpy float32 arithmetic: `a * b` rounds the product, `+` rounds
    the sum, `/` is IEEE -- the order is ATen's small-matrix bmm, (a0*x0 + a1*x1) + a2*x2."""
    p = np.asarray(points, F)[:, None, :3]
    A, t, K, Rp, tp = (np.asarray(m, F) for m in (inv_rots, trans, intrins, post_rots, post_trans))
    with np.errstate(all="ignore"):
        q = [p[..., i] - t[None, :, i] for i in range(3)]
        c = [(A[None, :, i, 0] * q[0] + A[None, :, i, 1] * q[1]) + A[None, :, i, 2] * q[2] for i in range(3)]
        k = [(K[None, :, i, 0] * c[0] + K[None, :, i, 1] * c[1]) + K[None, :, i, 2] * c[2] for i in range(3)]
        d = k[2]
        u0, v0 = k[0] / d, k[1] / d
        u = (Rp[None, :, 0, 0] * u0 + Rp[None, :, 0, 1] * v0) + tp[None, :, 0]
        v = (Rp[None, :, 1, 0] * u0 + Rp[None, :, 1, 1] * v0) + tp[None, :, 1]
    assert u.dtype == v.dtype == d.dtype == F
    return u, v, d


def valid_mask(u, v, d, H, W):
    with np.errstate(invalid="ignore"):
        return (u >= 0) & (v >= 0) & (u <= F(W - 1)) & (v <= F(H - 1)) & (d > 0)


def pixels(u, v):
    """(row, column) of unrounded (u, v): half to even."""
    with np.errstate(invalid="ignore"):
        return np.rint(v).astype(np.int64), np.rint(u).astype(np.int64)


def min_maps(u, v, d, valid, H, W):
    """float32 [N, H, W]: the minimum d per pixel over the valid pairs, 0 where none lands."""
    N = u.shape[1]
    maps = np.zeros((N, H, W), F)
    hit = np.zeros((N, H, W), bool)
    far = np.full((H, W), np.inf, F)
    for n in range(N):
        m = valid[:, n]
        y, x = pixels(u[m, n], v[m, n])
        near = far.copy()
        np.minimum.at(near, (y, x), d[m, n])
        hit[n][y, x] = True
        maps[n][hit[n]] = near[hit[n]]          # a valid depth of +inf is a depth: only pixels nothing lands in stay 0
    return maps


def inverse(rots):
    return torch.as_tensor(np.asarray(rots, F)).inverse().numpy()


def restatement(points, rots, trans, intrins, post_rots, post_trans, size):
    """The maps [N, H, W] from the tuple's matrices (numpy or CPU tensors); the inverse is torch's batched CPU inverse."""
    mats = [np.asarray(m, F) for m in (rots, trans, intrins, post_rots, post_trans)]
    u, v, d = project(points, inverse(mats[0]), *mats[1:])
    return min_maps(u, v, d, valid_mask(u, v, d, size[0], size[1]), size[0], size[1])


def from_table(points, table, size):
    """The maps from a [N, 28] camera table (its inverse as it stands)."""
    t = np.asarray(table, F)
    N = t.shape[0]
    Rp = np.zeros((N, 2, 2), F)
    Rp[:] = t[:, 21:25].reshape(N, 2, 2)
    u, v, d = project(points, t[:, :9].reshape(N, 3, 3), t[:, 9:12], t[:, 12:21].reshape(N, 3, 3), Rp, t[:, 25:27])
    return min_maps(u, v, d, valid_mask(u, v, d, size[0], size[1]), size[0], size[1])


# ------------------------------------------------------------------ eager torch, as the reference's pipeline step computes it
def torch_projection(points, rots, trans, intrins, post_rots, post_trans):
    """(u, v, d) tensors [P, N]: lidar -> camera -> image plane -> augmented image, broadcast fp32 matmuls on the CPU."""
    pts = torch.as_tensor(points)[:, :3].reshape(-1, 1, 3) - trans.reshape(1, -1, 3)
    cam = torch.matmul(rots.inverse()[None], pts[..., None])
    img = torch.matmul(intrins[None], cam)[..., 0]
    depth = img[..., 2:3]
    uv = img[..., :2] / depth
    uv = torch.matmul(post_rots[:, :2, :2][None], uv[..., None])[..., 0] + post_trans[:, :2][None]
    return uv[..., 0], uv[..., 1], depth[..., 0]


def torch_maps(u, v, d, H, W):
    """The reference's fill: per camera the valid points sorted by depth, far first, then ONE indexed assignment."""
    ok = (u >= 0) & (v >= 0) & (u <= W - 1) & (v <= H - 1) & (d > 0)
    out = []
    for n in range(u.shape[1]):
        un, vn, dn = u[ok[:, n], n], v[ok[:, n], n], d[ok[:, n], n]
        order = torch.argsort(dn, descending=True)
        m = torch.zeros((H, W))
        m[vn[order].round().long(), un[order].round().long()] = dn[order]
        out.append(m)
    return torch.stack(out), ok


# ------------------------------------------------------------------ rigs, clouds, cases
def rig(cfg, Hs=900, Ws=1600, cams=None, seed=5):
    """(rots, trans, intrins, post_rots, post_trans) CPU tensors of image_input_refs.synthetic_calibration() for ``cfg`` in eval mode:
    the matrices img_inputs14 makes, without the frames."""
    infos, l2c = R.synthetic_calibration(seed)
    r, _, box, fl, _ = R.augmentation_eval(cfg, Hs, Ws)
    cols = [[] for _ in range(5)]
    for name in (cams or cfg['cams']):
        s2l = torch.tensor(np.asarray(l2c[name], np.float64)).inverse().float()
        Rp, Tp = R.post_matrices(r, box, fl)
        for lst, m in zip(cols, (s2l[:3, :3], s2l[:3, 3], torch.Tensor(infos[name]['cam_intrinsic']), Rp, Tp)):
            lst.append(m)
    return tuple(torch.stack(c) for c in cols)


def identity_rig(N=1):
    """rot = I, tran = 0, intrin = I, post_rot = I, post_tran = 0: u = x / z and v = y / z exactly, d = z."""
    eye = torch.eye(3)[None].repeat(N, 1, 1)
    return eye.clone(), torch.zeros(N, 3), eye.clone(), eye.clone(), torch.zeros(N, 3)


def cloud(P, seed=0, C=3, sigma=(20.0, 20.0, 3.0)):
    """float32 [P, C]: Gaussian x y z about the sensor (columns past the third: uniform noise, as intensity and ring index)."""
    g = np.random.default_rng([seed, P])
    pts = g.uniform(0, 31, (P, C)).astype(F)
    pts[:, :3] = (g.standard_normal((P, 3)) * np.asarray(sigma)).astype(F)
    return pts


def front_cloud(P, H, W, seed=0, zlo=1.0, zhi=40.0):
    """float32 [P, 3] for the identity camera of an H x W map: most points land inside, some outside on each side and behind."""
    g = np.random.default_rng([seed, P, H, W])
    z = g.uniform(zlo, zhi, P)
    z[g.random(P) < 0.05] *= -1
    return np.stack([g.uniform(-0.2 * W, 1.2 * W, P) * z, g.uniform(-0.2 * H, 1.2 * H, P) * z, z], 1).astype(F)


P_CASES = [0, 1, 63, 64, 65, 255, 256, 257]
SIZE_CASES = [(5, 7), (24, 40), (33, 129)]
N_CASES = [1, 6, 7]
SMALL = dict(R.R50, input_size=(24, 40))          # the golden case's config: two cameras of the rig, 24 x 40
GOLDEN_CAMS = R.CAMS[:2]
GOLDEN_POINTS = 4096


def edge_points(H=5, W=7):
    """Hand-placed points for the identity camera of a 5 x 7 map (z = 1 unless said, so u = x and v = y exactly) and what the map
    must hold: (points float32 [P, 3], expected float32 [H, W]).  Depths are distinct per landing so that a wrong pixel shows."""
    up, tiny, nan, inf = np.nextafter(F(W - 1), F(np.inf)), np.nextafter(F(0), F(1)), F(np.nan), F(np.inf)
    vup = np.nextafter(F(H - 1), F(np.inf))
    rows, want = [], np.zeros((H, W), F)

    def at(u, v, z=1.0, lands=None):          # a point that projects to exactly (u, v) at depth z (z a power of two keeps x / z exact)
        rows.append((F(u) * F(z), F(v) * F(z), F(z)))
        if lands is not None:
            y, x = lands
            want[y, x] = F(z) if want[y, x] == 0 else min(want[y, x], F(z))

    at(0.0, 0.0, 2.0, (0, 0))                          # u = 0, v = 0
    at(W - 1, 1.0, 4.0, (1, W - 1))                    # u = W-1
    rows.append((up, F(1.0), F(1.0)))                  # u just past W-1: dropped
    at(1.0, H - 1, 8.0, (H - 1, 1))                    # v = H-1
    rows.append((F(1.0), vup, F(1.0)))                 # v just past H-1: dropped
    at(0.5, 2.0, 16.0, (2, 0))                         # halves, to even: 0.5 -> 0
    at(1.5, 2.0, 32.0, (2, 2))                         # 1.5 -> 2
    at(2.5, 3.0, 64.0, (3, 2))                         # 2.5 -> 2
    at(W - 1.5, 3.0, 0.5, (3, W - 1 if (W - 1) % 2 == 0 else W - 2))          # W-1.5 = 5.5 -> 6
    at(3.0, 0.5, 0.25, (0, 3))                         # v = 0.5 -> 0
    at(3.0, 1.5, 0.125, (2, 3))                        # v = 1.5 -> 2
    rows.append((F(-0.0), F(4.0), F(1.0)))             # u = -0.0: valid, column 0
    want[4, 0] = 1.0
    rows.append((F(4.0), F(-0.0), F(1.0)))             # v = -0.0: valid, row 0
    want[0, 4] = 1.0
    rows.append((F(2.0), F(2.0), F(0.0)))              # d = 0: dropped (u, v = inf)
    rows.append((F(0.0), F(0.0), F(0.0)))              # 0 / 0: NaN, dropped
    rows.append((F(-2.0), F(-2.0), F(-1.0)))           # d < 0 with u, v inside: dropped
    rows.append((F(0.0), F(0.0), tiny))                # the smallest positive denormal depth at (0, 0): nearer than the 2.0 above
    want[0, 0] = tiny
    for bad in (nan, inf, -inf):
        rows.append((bad, F(1.0), F(1.0)))
        rows.append((F(1.0), bad, F(1.0)))
        rows.append((F(1.0), F(1.0), bad))
    rows.append((F(-1.0), F(1.0), F(1.0)))             # left of the image
    rows.append((F(1.0), F(-0.25), F(1.0)))            # above it, though it would round to row 0
    # several points in one pixel: near first, far first, three, equal depths
    for (u, v), zs in (((4.0, 1.0), (2.0, 4.0)), ((5.0, 1.0), (4.0, 2.0)), ((4.0, 2.0), (8.0, 2.0, 4.0)), ((5.0, 2.0), (2.0, 8.0, 4.0)),
                       ((4.0, 3.0), (4.0, 8.0, 2.0)), ((5.0, 3.0), (4.0, 4.0))):
        for z in zs:
            at(u, v, z, (int(v), int(u)))
    at(3.75, 3.75, 2.0, (4, 4))                        # two that differ before rounding, one pixel
    at(4.25, 4.0, 1.0, (4, 4))
    return np.array(rows, F), want
