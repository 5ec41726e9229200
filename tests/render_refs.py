"""Plain restatements, input generators and the judging rules for the volume-rendering kernels: csrc/render.hip
(``coocc_render_nearest``, ``coocc_render_nearest_cams``, ``coocc_render_activate_table``, ``coocc_volume_sampling``,
``coocc_raw2outputs``, ``coocc_render_losses``), csrc/interp.hip ``coocc_upsample_maps`` and csrc/backward.hip
(``coocc_render_nearest_bwd``, ``coocc_render_losses_bwd``).  Used by tests/test_render_refs_host.py (no GPU),
tests/test_gpu_render_kernels.py and tests/render_geo_lds_worker.py.

Every operation is written once as a function of a dtype, from the formulas in the kernels' comments and oracle/ref_cpu.py:
float64 is the reference, float32 the anchor of ``util.assert_precise`` (C_MAX = 4, C_RMS = 2, unchanged).

The discrete parts are not judged with a tolerance, they are reproduced: the voxel index of a sample (``sample_index``), the depth
bin and the foreground test of the losses, the in-box mask of the library sampler.  Each is a handful of single IEEE fp32
operations, which numpy evaluates to the same bits as the device, so the float64 references take them as inputs.

The ray kernels evaluate exp, the sigmoid's reciprocal and the step's square root with the hardware instructions (v_exp_f32,
v_rcp_f32, v_sqrt_f32: 1 ulp each by the ISA manual), exp(x) as exp2(x log2 e).  A plain fp32 restatement (torch's correctly
rounded-ish libm, sequential sums) is therefore quieter than any correct kernel of this design can be; ``composite(..., hw=True)``
is a second fp32 form that models exactly those three instructions from their stated accuracy (a seeded relative perturbation of
up to 1 ulp = 2^-23 after each, and the rounded product x log2 e before the exp2).  It never sees a kernel's output.  The anchor of
the ray kernels is the worse of the two forms' errors (``ray_anchor``)."""
import numpy as np
import torch

import util
from adjoint_refs import atomics_anchor, exact_ref, lin_src, maps_fwd     # noqa: F401  (shared rules, some used through this module)
from norm_refs import assert_exact, bits_equal, gen, no_subnormals          # noqa: F401

F32, F64 = torch.float32, torch.float64
NAN = float("nan")
ULP = 2.0 ** -23
LOG2E = float(np.float32(1.4426950408889634))


# ----------------------------------------------------------------------------- the index rule (discrete, bit-exact)
def bounds_consts(bounds):
    """(lo [3], n [3], step [3]) in numpy float32 from the nine floats xbound, ybound, zbound = (lo, hi, step), with the host code's
    own operations (render_nearest_impl): b = lo + step / 2, lo' = b - step / 2, n = (hi - lo) / step."""
    b = np.asarray(bounds, dtype=np.float32).reshape(3, 3)
    two = np.float32(2.0)
    step = b[:, 2]
    centre = b[:, 0] + step / two
    return centre - step / two, (b[:, 1] - b[:, 0]) / step, step


def sample_coords(geom, bounds):
    """g [..., 3] float32 (numpy): the voxel coordinate of every sample position, (p - lo) when all steps are 1, else
    (p - lo) / step -- one or two IEEE fp32 operations per axis."""
    lo, n, step = bounds_consts(bounds)
    p = geom.detach().cpu().numpy().astype(np.float32)
    g = p - lo
    if not bool((step == np.float32(1.0)).all()):
        g = g / step
    assert g.dtype == np.float32
    return g


def sample_index(geom, bounds):
    """(idx int64 [..., 3], inside bool [...]) of float32 positions ``geom`` [..., 3]: inside = 0 <= g < n on all three axes, the
    index trunc(g) inside and (0, 0, 0) outside."""
    _, n, _ = bounds_consts(bounds)
    g = sample_coords(geom, bounds)
    inside = ((g >= np.float32(0.0)) & (g < n)).all(-1)
    idx = np.where(inside[..., None], np.trunc(g), np.float32(0.0)).astype(np.int64)
    return torch.from_numpy(idx), torch.from_numpy(inside)


# ----------------------------------------------------------------------------- compositing
class _Hw:
    """The three hardware transcendentals as the ISA manual states them, on float32 tensors; ``on=False``: torch's own."""

    def __init__(self, on, seed):
        self.on, self.g = on, gen(seed)

    def _jitter(self, v):
        u = torch.rand(v.shape, generator=self.g, dtype=F64) * 2 - 1
        return (v.to(F64) * (1 + u * ULP)).to(F32)

    def exp(self, x):
        if not self.on:
            return torch.exp(x)
        y = x * torch.tensor(LOG2E, dtype=F32)                  # the rounded fp32 product, then v_exp_f32
        e = self._jitter(torch.exp2(y.to(F64)).to(F32))
        # 2^0 is taken as exactly 1: a step of length 0 or an empty voxel has alpha = 0 on the device too (the all-empty ray of the
        # GPU test must render exact zeros), and most samples of the long-ray cases are such steps -- jitter there would only
        # inflate the anchor (by 2x at D = 33 to 10x at D = 256 on the depth channel)
        return torch.where(y == 0, torch.ones_like(e), e)

    def rcp(self, x):
        return self._jitter((1.0 / x.to(F64)).to(F32)) if self.on else 1.0 / x

    def sqrt(self, x):
        return self._jitter(torch.sqrt(x.to(F64)).to(F32)) if self.on else torch.sqrt(x)


def rays_of(t):
    """[N, D, H, W, ...] -> [N H W, D, ...]: one row per ray, samples in depth order."""
    lead = t.shape[0] * t.shape[2] * t.shape[3]
    return t.permute(0, 2, 3, 1, *range(4, t.dim())).reshape(lead, t.shape[1], *t.shape[4:])


def lanes_ch(D):
    """Samples per lane of the ray kernels: 32 lanes per ray."""
    return (D + 31) // 32


def _ray_terms(table, dims, idx, inside, dtype, hw=False, seed=0, mutate=None, coords=None):
    """Per ray and sample: (lin [R, D] voxel rows, sigma_raw, dist, alpha, colour [R, D, 3], factor = 1 - alpha + 1e-10, T exclusive).
    ``idx`` [R, D, 3], ``inside`` [R, D].  ``mutate``: one of the wrong forms of the host test."""
    X, Y, Z = dims
    R, D = inside.shape
    h = _Hw(hw and dtype == F32, seed)
    lin = (idx[..., 0] * Y + idx[..., 1]) * Z + idx[..., 2]
    t = table.to(dtype)[lin]                                   # [R, D, 4]
    sraw = t[..., 0]
    sigma = torch.relu(sraw)
    pos = idx.to(dtype)
    if mutate == "untruncated":                               # steps between the positions themselves, not their voxels
        pos = torch.where(inside[..., None], torch.as_tensor(coords).to(dtype), torch.zeros_like(pos))
    nxt = pos[:, 1:]
    if mutate == "wrong_lane" and D > 1:                      # a lane's last sample takes its "next" from the lane after the next
        CH = lanes_ch(D)
        d = torch.arange(D - 1)
        src = torch.where((d + 1) % CH == 0, torch.clamp(d + 1 + CH, max=D - 1), d + 1)
        nxt = pos[:, src]
    diff = nxt - pos[:, :-1]
    dist = h.sqrt((diff * diff).sum(-1)) if dtype == F32 else torch.sqrt((diff * diff).sum(-1))
    last = dist[:, -1:].clone() if (mutate == "last_step" and D > 1) else torch.full((R, 1), 1e10, dtype=dtype)
    if mutate == "last_step" and D == 1:
        last = torch.ones(R, 1, dtype=dtype)
    dist = torch.cat([dist, last], 1)
    e = h.exp(-torch.relu(sigma * dist)) if dtype == F32 else torch.exp(-torch.relu(sigma * dist))
    alpha = 1 - e
    if dtype == F32:
        sig = h.rcp(1 + h.exp(-t[..., 1:]))
    else:
        sig = 1 / (1 + torch.exp(-t[..., 1:]))
    out_colour = sig if mutate == "oob_sigmoid" else torch.full_like(sig, 0.5)
    colour = torch.where(inside[..., None], sig, out_colour)
    factor = 1 - alpha if mutate == "no_eps" else 1 - alpha + torch.tensor(1e-10, dtype=dtype)
    ones = torch.ones(R, 1, dtype=dtype)
    if mutate == "restart16" and D > 16 * lanes_ch(D):         # the scan starts again at lane 16
        k = 16 * lanes_ch(D)
        T = torch.cat([torch.cat([ones, torch.cumprod(factor[:, :k], 1)[:, :-1]], 1),
                       torch.cat([ones, torch.cumprod(factor[:, k:], 1)[:, :-1]], 1)], 1)
    else:
        T = torch.cat([ones, torch.cumprod(factor, 1)[:, :-1]], 1)
    if mutate == "inclusive":
        T = torch.cumprod(factor, 1)
    return lin, sraw, dist, alpha, colour, factor, T


def composite(table, dims, idx, inside, zvals, dtype, hw=False, seed=0, mutate=None, coords=None):
    """maps [N, H, W, 4] (r, g, b, depth) of table [V, 4] (sigma, rgb logits) over the samples idx [N, D, H, W, 3], inside
    [N, D, H, W]:  sigma = relu(t.s), dist_k = |idx_{k+1} - idx_k| (the last 1e10), alpha = 1 - exp(-relu(sigma dist)),
    c = inside ? sigmoid(t.rgb) : 0.5, T = exclusive product of (1 - alpha + 1e-10), w = alpha T, rgb = sum w c, depth = sum w z.
    float32 sums sample after sample; ``hw``: the float32 form with the modelled hardware transcendentals."""
    N, D, H, W = inside.shape
    ri, rin = rays_of(idx), rays_of(inside)
    rc = None if coords is None else rays_of(torch.as_tensor(coords))
    _, _, _, alpha, colour, _, T = _ray_terms(table, dims, ri, rin, dtype, hw, seed, mutate, rc)
    w = alpha * T
    z = zvals.to(dtype)
    rgb, depth = torch.zeros(N * H * W, 3, dtype=dtype), torch.zeros(N * H * W, dtype=dtype)
    for k in range(D):                                        # the sequential sum (float64: the order does not matter)
        rgb = rgb + w[:, k:k + 1] * colour[:, k]
        depth = depth + w[:, k] * z[k]
    return torch.cat([rgb, depth[:, None]], 1).view(N, H, W, 4)


def ray_refs(c, mutate=None):
    """(ref64, (plain fp32, hardware-modelled fp32)) of a ray case."""
    a = (c["table"], c["dims"], c["idx"], c["inside"], c["zvals"])
    return composite(*a, F64), (composite(*a, F32), composite(*a, F32, hw=True, seed=c["seed"]))


def ray_anchor(ref64, forms, chan):
    """The worse (e_max, e_rms) of the float32 forms on the channels ``chan`` (a slice of the last axis)."""
    errs = [util.errors(f[..., chan], ref64[..., chan]) for f in forms]
    return max(e[0] for e in errs), max(e[1] for e in errs)


RGB, DEPTH = slice(0, 3), slice(3, 4)


def judge_maps(out, ref64, forms, what, judge=util.assert_precise):
    """rgb and depth judged apart (their scales differ), each against float64 with the worse float32 form as the anchor."""
    return [judge(out[..., ch], ref64[..., ch], anchor=ray_anchor(ref64, forms, ch), what="%s %s" % (what, nm))
            for nm, ch in (("rgb", RGB), ("depth", DEPTH))]


def maps_rejected(out, ref64, forms):
    """True when ``judge_maps`` would turn ``out`` down on either part."""
    return any(not st["ok"] for st in judge_maps(out, ref64, forms, "(host) a wrong result", judge=util.precision))


# ----------------------------------------------------------------------------- backward of the compositing
def _lane_scans(factor, qw_of, CH):
    """(T [R, D], S [R, D]) in the order the backward kernel documents: 64 lanes with CH consecutive samples each; a lane's product
    of its factors, an up-scan over the lanes (steps 1, 2, ... 32), the exclusive prefix handed on inside the lane; the lane's sum
    of q w, a down-scan over the lanes, the exclusive suffix handed back inside the lane.  ``qw_of(T)`` gives q w from T."""
    R, D = factor.shape
    pad = 64 * CH - D
    f = torch.cat([factor, torch.ones(R, pad, dtype=factor.dtype)], 1).view(R, 64, CH)
    prod = torch.ones(R, 64, dtype=factor.dtype)
    for j in range(CH):
        prod = prod * f[:, :, j]
    inc, o = prod, 1
    while o < 64:
        inc = torch.cat([inc[:, :o], inc[:, o:] * inc[:, :-o]], 1)
        o *= 2
    t = torch.cat([torch.ones(R, 1, dtype=factor.dtype), inc[:, :-1]], 1)
    Ts = []
    for j in range(CH):
        Ts.append(t)
        t = t * f[:, :, j]
    T = torch.stack(Ts, 2).reshape(R, 64 * CH)[:, :D]
    qw = torch.cat([qw_of(T), torch.zeros(R, pad, dtype=factor.dtype)], 1).view(R, 64, CH)
    tot = torch.zeros(R, 64, dtype=factor.dtype)
    for j in range(CH):
        tot = tot + qw[:, :, j]
    suf, o = tot, 1
    while o < 64:
        suf = torch.cat([suf[:, :-o] + suf[:, o:], suf[:, -o:]], 1)
        o *= 2
    sv = torch.cat([suf[:, 1:], torch.zeros(R, 1, dtype=factor.dtype)], 1)
    Ss = [None] * CH
    for j in range(CH - 1, -1, -1):
        Ss[j] = sv
        sv = sv + qw[:, :, j]
    return T, torch.stack(Ss, 2).reshape(R, 64 * CH)[:, :D]


def render_adj(c, dmaps, dtype, order=None, mutate=None, scan=False):
    """dtable [V, 4] of ``composite`` with respect to the table, by the formulas above k_render_nearest_bwd: with
    q_k = <g_rgb, c_k> + g_depth z_k and S_k = sum_{j > k} q_j w_j:  dL/da_k = q_k T_k - S_k / (1 - a_k + 1e-10),
    da_k/ds_k = exp(-sigma_k dist_k) dist_k [s_k > 0],  dL/d logit_k = w_k g_rgb c_k (1 - c_k) for inside samples.
    The contributions are added sample after sample, or (``order``: a seed) in a seeded permutation: the kernel's atomics land in an
    order that changes from run to run.  ``scan``: T and S in the kernel's documented scan order over 64 lanes instead of sample
    after sample (another honest float32 evaluation of the same two recurrences).  ``mutate``: the wrong forms of the host test."""
    X, Y, Z = c["dims"]
    ri, rin = rays_of(c["idx"]), rays_of(c["inside"])
    lin, sraw, dist, alpha, colour, factor, T = _ray_terms(c["table"], c["dims"], ri, rin, dtype)
    R, D = lin.shape
    g = dmaps.to(dtype).reshape(R, 4)
    z = c["zvals"].to(dtype)
    q = (colour * g[:, None, :3]).sum(-1) + g[:, 3:4] * z[None]
    if scan:                                                               # the kernel's own order of the two scans
        T, S = _lane_scans(factor, lambda Tk: q * (alpha * Tk), (D + 63) // 64)
    w = alpha * T
    qw = q * w
    incl = torch.flip(torch.cumsum(torch.flip(qw, [1]), 1), [1])          # sum_{j >= k}
    if not scan:
        S = incl if mutate == "suffix_inclusive" else torch.cat([incl[:, 1:], torch.zeros(R, 1, dtype=dtype)], 1)
    da = q * T - S / factor
    x = torch.relu(sraw) * dist
    gate = torch.ones_like(x, dtype=torch.bool) if mutate == "no_gate" else ((sraw > 0) & (x > 0))
    ds = torch.where(gate, da * torch.exp(-x) * dist, torch.zeros_like(da))
    dc = torch.where(rin[..., None], w[..., None] * g[:, None, :3] * colour * (1 - colour), torch.zeros_like(colour))
    contrib = torch.cat([ds[..., None], dc], -1).reshape(-1, 4)
    rows = lin.reshape(-1)
    if order is not None:
        perm = torch.randperm(rows.numel(), generator=gen(order))
        rows, contrib = rows[perm], contrib[perm]
    return torch.zeros(X * Y * Z, 4, dtype=dtype).index_add_(0, rows, contrib)


def bwd_forms(c, dmaps, seeds=(1, 2, 3)):
    """The float32 evaluations whose worst error is the anchor of the backward: the two recurrences sample after sample and in the
    kernel's scan order, each with its contributions added in three seeded orders."""
    return [render_adj(c, dmaps, F32, order=s, scan=sc) for sc in (False, True) for s in seeds]


def bwd_anchor(c, dmaps, ref64, col):
    """(e_max, e_rms) on the columns ``col``: adjoint_refs.atomics_anchor (the worst of three seeded orders) of either scan order."""
    a = [atomics_anchor(lambda order: render_adj(c, dmaps, F32, order=order, scan=sc)[:, col], ref64[:, col]) for sc in (False, True)]
    return max(a[0][0], a[1][0]), max(a[0][1], a[1][1])


SIGMA, LOGITS = slice(0, 1), slice(1, 4)


def touched(c):
    """bool [V]: the voxels some sample of the case reads (every other row of dtable must stay exactly 0)."""
    X, Y, Z = c["dims"]
    idx = c["idx"]
    m = torch.zeros(X * Y * Z, dtype=torch.bool)
    m[((idx[..., 0] * Y + idx[..., 1]) * Z + idx[..., 2]).reshape(-1)] = True
    return m


# ----------------------------------------------------------------------------- the ray cases
UNIT_SMALL = ([-6., 6., 1.], [-5., 5., 1.], [-3., 3., 1.])              # (12, 10, 6)
BOUNDS = {
    "unit": ((12, 10, 6), UNIT_SMALL),
    "half": ((12, 10, 6), ([-3., 3., .5], [-2.5, 2.5, .5], [-1.5, 1.5, .5])),
    "y04": ((12, 10, 6), ([-6., 6., 1.], [-2., 2., .4], [-1.5, 1.5, .5])),    # 0.4: not a power of two; n = 10 in fp32
    "small_box": ((12, 10, 6), ([-4., 4., 1.], [-3., 4., 1.], [-2., 2., 1.])),  # the render box (8, 7, 4) inside the volume
    "wide": ((40, 30, 6), ([-20., 20., 1.], [-15., 15., 1.], [-3., 3., 1.])),  # room for the long rays
    "wide_half": ((40, 30, 6), ([-10., 10., .5], [-7.5, 7.5, .5], [-1.5, 1.5, .5])),
    "x1024": ((1024, 1, 2), ([0., 1024., 1.], [0., 1., 1.], [0., 2., 1.])),
    "y1024": ((2, 1024, 1), ([0., 2., 1.], [0., 1024., 1.], [0., 1., 1.])),
    "z1024": ((1, 2, 1024), ([0., 1., 1.], [0., 2., 1.], [0., 1024., 1.])),
}
RENDER_D = [1, 2, 31, 32, 33, 64, 65, 112, 128, 129, 255, 256]          # with W = 5
RENDER_W = [1, 8, 9, 31, 32, 33, 40]                                     # with D = 33
RENDER_BOUNDS_AT = [("half", 33), ("y04", 33), ("small_box", 33), ("wide_half", 129), ("half", 256)]
PACKING = ["x1024", "y1024", "z1024"]
BWD_D = [1, 24, 63, 64, 65, 128, 129, 192, 193, 256]
BWD_RAYS = {1: (1, 1, 1), 3: (1, 3, 1), 4: (2, 1, 2), 5: (1, 1, 5), 30: (2, 3, 5)}    # N H W -> (N, H, W)
ACT_V = [1, 255, 256, 257]


def bounds_for(D, half=False):
    return ("wide_half" if half else "wide") if D > 64 else ("half" if half else "unit")


def render_edge_cases():
    """(bounds name, N, D, H, W, opaque_first) of every forward edge shape: the depths, the widths, the bounds, the packing limit
    and the two cases whose rays survive an opaque first sample through the 1e-10 alone."""
    out = [(bounds_for(D), 2, D, 3, 5, False) for D in RENDER_D]
    out += [("unit", 2, 33, 3, W, False) for W in RENDER_W]
    out += [(b, 2, D, 3, 5, False) for b, D in RENDER_BOUNDS_AT]
    out += [(b, 2, 33, 3, 5, False) for b in PACKING]
    return out + [("unit", 2, 33, 3, 5, True), ("wide", 2, 129, 3, 5, True)]


def case_id(v):
    return "%s-N%d-D%d-H%d-W%d%s" % (v[0], v[1], v[2], v[3], v[4], "-opaque" if v[5] else "")


def bwd_edge_cases():
    """(bounds name, N, D, H, W) of the backward: every depth at 30 rays, every other ray count at D = 65, both steps."""
    out = [(bounds_for(D, half), 2, D, 3, 5) for D in BWD_D for half in (False, True)]
    return out + [(bounds_for(65, half),) + (BWD_RAYS[r][0], 65) + BWD_RAYS[r][1:] for r in BWD_RAYS if r != 30 for half in (False, True)]


def flat9(bounds):
    return [float(v) for b in bounds for v in b]


def ray_case(bname, N, D, H, W, seed=0, opaque_first=False):
    """Table [V, 4] (N(0, 1) rgb logits, 0.3 N(0, 1) sigma: about half of the voxels empty, rays alive to the end), zvals =
    linspace(0, D, D) and positions [N, D, H, W, 3] that start inside the render box and march out of it (every generic ray has
    inside and outside samples; steps of half a voxel and less give repeated voxels, i.e. steps of length 0).  Rays, in (n, h, w)
    order, as far as the case has them:
      0  planted samples: exactly on lo (voxel 0), exactly on lo + n step (outside), just below lo (outside); then on from that corner
      1  entirely outside            2  entirely inside one voxel (all steps 0 but the last)
      3  inside for all D samples, through voxels whose sigma is made <= 0: its map is exactly 0
    Voxel (0, 0, 0), which every outside sample reads, gets sigma 0.8, so the out-of-bounds colour carries weight.
    ``opaque_first``: every ray's first voxel gets sigma 50 and its second sample lies in another voxel: alpha_0 = 1, the rest of
    the ray survives only through the 1e-10 (and z_0 = 0: the depth map is of the order 1e-10 D)."""
    dims, bounds = BOUNDS[bname]
    X, Y, Z = dims
    g = gen(7919 * D + 131 * W + 17 * N + H + 1000003 * seed + sum(map(ord, bname)))
    lo, n, step = (torch.from_numpy(a.astype(np.float64)) for a in bounds_consts(flat9(bounds)))
    R = N * H * W
    table = no_subnormals(torch.randn(X * Y * Z, 4, generator=g))
    table[:, 0] *= 0.3
    table[0, 0] = 0.8
    start = torch.rand(R, 3, generator=g, dtype=F64) * (n - 0.02) + 0.01
    direction = torch.randn(R, 3, generator=g, dtype=F64)
    long_axis = int(torch.argmax(n))
    if float(n.max()) >= 1024:                                # the packing cases: along the long axis, over all of it
        even = torch.arange(R) % 2 == 0                       # every second ray runs down from the far end
        direction[:, long_axis] = torch.where(even, 40.0, -40.0).to(F64)
        start[:, long_axis] = torch.where(even, 0.3, float(n.max()) - 0.3).to(F64)
    else:                                                       # ray 0 marches on from the corner voxel its planted samples sit at
        start[0], direction[0] = 0.6, direction[0].abs() + 0.2
    direction = direction / direction.norm(dim=1, keepdim=True)
    reach = float(n.max()) * 1.2                                # generic rays: a box length and a fifth over the D samples
    k = torch.arange(D, dtype=F64)
    gpos = start[:, None] + direction[:, None] * (k[None, :, None] * (reach / max(D, 2)))
    if opaque_first and D > 1:                                  # the second sample one whole voxel further along x (or back)
        gpos[:, 0] = torch.floor(gpos[:, 0]) + 0.5
        shift = torch.where(gpos[:, 0, 0] + 1 < n[0], 1.0, -1.0)
        gpos[:, 1] = gpos[:, 0]
        gpos[:, 1, 0] += shift
    if R > 1 and not opaque_first:
        gpos[1] = -3.0 - torch.rand(D, 3, generator=g, dtype=F64)
    if R > 2 and not opaque_first:
        gpos[2] = (torch.floor(n / 2) + 0.1)[None] + 0.8 * torch.rand(D, 3, generator=g, dtype=F64)
    empty_ray = R > 3 and not opaque_first
    if empty_ray:
        a, b = torch.tensor([0.3, 0.4, 0.2], dtype=F64) * n + 1e-3, torch.tensor([0.8, 0.7, 0.9], dtype=F64) * n
        gpos[3] = a[None] + (b - a)[None] * (k[:, None] / max(D - 1, 1))
    geom = (gpos * step + lo).to(F32)
    if not opaque_first:                                        # the planted samples of ray 0, as exact fp32 values
        lo32 = bounds_consts(flat9(bounds))[0]
        hi32 = np.asarray(bounds, dtype=np.float32)[:, 1]
        planted = [lo32, hi32, np.nextafter(lo32, np.float32(-np.inf))]
        for d, p in enumerate(planted[:D]):
            geom[0, d] = torch.from_numpy(p.astype(np.float32))
    geom = geom.view(N, H, W, D, 3).permute(0, 3, 1, 2, 4).contiguous()          # [N, D, H, W, 3]
    idx, inside = sample_index(geom, flat9(bounds))
    if float(n.max()) >= 1024:                                # two samples that hit index 1023 and index 0 of the long axis
        far = gpos[0, 0].clone()
        far[long_axis] = 1023.5
        near = far.clone()
        near[long_axis] = 0.25
        r = R - 1
        nn_, hh, ww = r // (H * W), (r // W) % H, r % W
        geom[nn_, 0, hh, ww] = (far * step + lo).to(F32)
        if D > 1:
            geom[nn_, 1, hh, ww] = (near * step + lo).to(F32)
        idx, inside = sample_index(geom, flat9(bounds))
    lin = (idx[..., 0] * Y + idx[..., 1]) * Z + idx[..., 2]
    if empty_ray:
        rows = rays_of(lin)[3]
        assert bool(rays_of(inside)[3].all()), "the empty ray must stay inside"
        table[rows, 0] = -table[rows, 0].abs()
        assert not bool((rows == 0).any())
    if opaque_first and D > 1:
        first = rays_of(lin)[:, 0]
        assert bool(rays_of(inside)[:, :2].all()) and bool((rays_of(lin)[:, 1] != first).all())
        table[first, 0] = 50.0
    zvals = torch.linspace(0, D, D, dtype=F32)
    return dict(name=bname, dims=dims, bounds=flat9(bounds), table=table.contiguous(), geom=geom, idx=idx, inside=inside,
                coords=sample_coords(geom, flat9(bounds)), zvals=zvals, N=N, D=D, H=H, W=W, seed=1 + seed, empty_ray=empty_ray)


# ----------------------------------------------------------------------------- coocc_render_activate_table
def activate_ref(table, dtype, hw=False, seed=0):
    """sigmoid on the columns 1..3 of the [V, 4] table; column 0 passes."""
    h = _Hw(hw and dtype == F32, seed)
    t = table.to(dtype).clone()
    t[:, 1:] = h.rcp(1 + h.exp(-t[:, 1:])) if dtype == F32 else 1 / (1 + torch.exp(-t[:, 1:]))
    return t


# ----------------------------------------------------------------------------- the camera cases (in-kernel geometry)
CAM_FRUSTA = [(3, 5), (2, 9), (1, 33)]
CAM_D = [31, 33, 112, 129, 256]
CAM_GRID = (100, 100, 8)
CAM_BOUNDS = {"unit": ([-50., 50., 1.], [-50., 50., 1.], [-5., 3., 1.]), "half": ([-25., 25., .5], [-25., 25., .5], [-2., 2., .5])}
CAM_CASES = [(H, W, D, "unit") for H, W in CAM_FRUSTA for D in CAM_D] + [(3, 5, 33, "half"), (2, 9, 129, "half"), (1, 33, 256, "half")]


def cam_table(seed):
    g = gen(4000 + seed)
    X, Y, Z = CAM_GRID
    t = no_subnormals(torch.randn(X * Y * Z, 4, generator=g))
    t[:, 0] *= 0.3
    t[0, 0] = 0.8
    return t.contiguous()


def cam_dbound(D):
    """Depth axis of D bins from 2 m to at least 58 m in power-of-two steps (2 m for 31 and 33 bins, 0.5 m for 112 and 129, 0.25 m for
    256): the rays of every frustum, the nearly level ones of the one-row frustum too, leave the 100 m volume."""
    import math
    step = 2.0 ** math.ceil(math.log2(56.0 / D))
    return [2.0, 2.0 + step * D, step]


def cam_name(H, W, D, b):
    return "%dx%d_D%d_%s" % (H, W, D, b)


# ----------------------------------------------------------------------------- coocc_raw2outputs
RAW_R, RAW_S = [1, 3, 4, 5, 48], [1, 16, 63, 64, 65, 130]


def raw_case(R, S):
    """raw [R, S, 4] (rgb in [0, 1], sigma |N(0, 1)|), z [R, S] ascending from 0.5.  With R >= 3 ray 1 has all-zero sigma (weights
    exactly 0, depth = zmin) and ray 2 sigma 50 at its first sample (all weight on sample 0)."""
    g = gen(100 * R + S)
    raw = torch.rand(R, S, 4, generator=g)
    raw[..., 3] = no_subnormals(torch.randn(R, S, generator=g)).abs()
    z = (0.5 + torch.cumsum(torch.rand(R, S, generator=g) * 0.2 + 0.05, 1)).to(F32)
    if R >= 3:
        raw[1, :, 3] = 0.0
        raw[2, 0, 3] = 50.0
    return dict(raw=raw.contiguous(), z=z.contiguous(), zmin=float(z.min()), zmax=float(z.max()))


def raw2outputs_ref(raw, z, white_bkgd, zmin, zmax, dtype):
    """(rgb [R, 3], depth [R], weights [R, S]): alpha = 1 - exp(-sigma), T the exclusive product of (1 - alpha + 1e-10), w = alpha T,
    rgb = sum w c (+ 1 - sum w on a white background), depth = clamp(sum w z / (sum w + 1e-8), zmin, zmax)."""
    raw, z = raw.to(dtype), z.to(dtype)
    R, S, _ = raw.shape
    alpha = 1 - torch.exp(-raw[..., 3])
    f = 1 - alpha + torch.tensor(1e-10, dtype=dtype)
    T = torch.cat([torch.ones(R, 1, dtype=dtype), torch.cumprod(f, 1)[:, :-1]], 1)
    w = alpha * T
    rgb, ad, aw = torch.zeros(R, 3, dtype=dtype), torch.zeros(R, dtype=dtype), torch.zeros(R, dtype=dtype)
    for k in range(S):
        rgb = rgb + w[:, k:k + 1] * raw[:, k, :3]
        ad = ad + w[:, k] * z[:, k]
        aw = aw + w[:, k]
    if white_bkgd:
        rgb = rgb + (1 - aw)[:, None]
    depth = torch.clamp(ad / (aw + torch.tensor(1e-8, dtype=dtype)), torch.tensor(zmin, dtype=F32).to(dtype), torch.tensor(zmax, dtype=F32).to(dtype))
    return rgb, depth, w


# ----------------------------------------------------------------------------- coocc_volume_sampling
VS_VOLS, VS_C, VS_N = [(2, 2, 2), (5, 3, 4), (1, 4, 3)], [1, 8, 64, 65, 130], [1, 63, 257]
VS_AABB = {"generic": [-12., -10., -2., 12., 10., 3.], "pow2": [-4., -2., -1., 4., 2., 1.]}


def vs_scale(aabb):
    """The host's three factors 1 / size * 2 in fp32."""
    a = np.asarray(aabb, dtype=np.float32)
    return np.float32(1.0) / (a[3:] - a[:3]) * np.float32(2.0)


def vs_norm32(pts, aabb):
    """(p - a) s - 1 in fp32, the product rounded before the subtraction."""
    a = np.asarray(aabb, dtype=np.float32)
    return (pts.numpy().astype(np.float32) - a[:3]) * vs_scale(aabb) - np.float32(1.0)


def vs_case(vol, C, n, kind):
    """Volume rows [d0 d1 d2, C] of N(0, 1) and n points.  "generic": inside and up to half a box outside, none closer than 1e-3
    (normalised) to a face -- a fused multiply-subtract cannot move the mask.  "pow2": a box with power-of-two sides, where the
    normalisation is exact; a third of the points then sit exactly on faces (and edges and corners)."""
    d0, d1, d2 = vol
    g = gen(1000 * C + n + d0 * 7 + d1 * 3 + d2 + len(kind))
    aabb = VS_AABB[kind]
    a = torch.tensor(aabb, dtype=F64)
    u = torch.rand(n, 3, generator=g, dtype=F64) * 3 - 1.5                     # normalised coordinates in [-1.5, 1.5]
    pts = ((u + 1) / 2 * (a[3:] - a[:3]) + a[:3]).to(F32)
    if kind == "pow2":
        face = torch.randint(0, 2, (n, 3), generator=g).to(F64) * 2 - 1         # -1 or 1
        pick = (torch.rand(n, 3, generator=g) < 0.5) & (torch.arange(n) % 3 == 0)[:, None]
        pick[0] = torch.tensor([True, True, True])
        on = ((face + 1) / 2 * (a[3:] - a[:3]) + a[:3]).to(F32)
        pts = torch.where(pick, on, pts)
    nrm = vs_norm32(pts, aabb)
    if kind == "generic":
        near = np.abs(np.abs(nrm.astype(np.float64)) - 1) < 1e-3
        pts = torch.where(torch.from_numpy(near), torch.zeros_like(pts) + a[:3].to(F32) + 0.25 * (a[3:] - a[:3]).to(F32), pts)
        assert not bool((np.abs(np.abs(vs_norm32(pts, aabb).astype(np.float64)) - 1) < 1e-3).any())
    rows = no_subnormals(torch.randn(d0 * d1 * d2, C, generator=g))
    return dict(rows=rows.contiguous(), pts=pts.contiguous(), aabb=aabb, vol=vol, C=C, n=n)


def volume_sampling_ref(rows, vol, pts, aabb, dtype):
    """(feat [n, C] in ``dtype``, mask bool [n] in fp32): trilinear, align_corners=True, border clamp; point x indexes the LAST
    volume axis.  mask: (p - a) s - 1 strictly inside (-1, 1) on all axes."""
    d0, d1, d2 = vol
    nrm = vs_norm32(pts, aabb)
    mask = torch.from_numpy(((nrm < 1) & (nrm > -1)).all(-1))
    if dtype == F32:
        g = torch.from_numpy(nrm)
    else:
        a = torch.tensor(aabb, dtype=F32).to(F64)
        g = (pts.to(F64) - a[:3]) * (2 / (a[3:] - a[:3])) - 1
    fr, i0, i1 = [], [], []
    for axis, size in ((0, d2), (1, d1), (2, d0)):
        f = torch.clamp((g[:, axis] + 1) / 2 * (size - 1), 0, size - 1)
        lo = torch.floor(f)
        fr.append(f - lo)
        i0.append(lo.to(torch.int64))
        i1.append(torch.clamp(lo.to(torch.int64) + 1, max=size - 1))
    r = rows.to(dtype)
    out = torch.zeros(pts.shape[0], rows.shape[1], dtype=dtype)
    for cz in range(2):
        for cy in range(2):
            for cx in range(2):
                zi, yi, xi = (i1 if cz else i0)[2], (i1 if cy else i0)[1], (i1 if cx else i0)[0]
                wgt = (fr[0] if cx else 1 - fr[0]) * (fr[1] if cy else 1 - fr[1]) * (fr[2] if cz else 1 - fr[2])
                out = out + r[(zi * d1 + yi) * d2 + xi] * wgt[:, None]
    return out, mask


# ----------------------------------------------------------------------------- the render losses
LOSS_NPIX, LOSS_D = [1, 255, 1024, 1025, 70000], [16, 112]


def loss_case(npix, D, foreground=True):
    """Rendered and ground-truth maps of ``npix`` pixels.  depth_gt: a third zeros (background), a sixth below 1.75 (bin 0:
    background), a sixth far beyond the last bin (clipped to D), the rest inside the bins.  ``foreground=False``: none at all."""
    g = gen(3 * npix + D)
    rgbs, rgb_gt = torch.rand(npix, 3, generator=g), torch.rand(npix, 3, generator=g)
    depths = (torch.rand(npix, generator=g) * D).to(F32)
    gt = (1.75 + torch.rand(npix, generator=g) * 0.5 * D).to(F32)
    kind = torch.arange(npix) % 6
    gt[(kind == 1) | (kind == 4)] = 0.0
    gt[kind == 2] = (torch.rand(npix, generator=g) * 1.75)[kind == 2]
    gt[kind == 3] = 1.75 + 0.5 * D + 40.0
    if not foreground:
        gt = torch.where(torch.arange(npix) % 2 == 0, torch.zeros(npix), torch.rand(npix, generator=g) * 1.75)
    return dict(rgbs=rgbs.contiguous(), depths=depths.contiguous(), rgb_gt=rgb_gt.contiguous(), depth_gt=gt.to(F32).contiguous())


def depth_bins(depth_gt, D):
    """(bin float32, foreground bool): clip((gt - 1.75) / 0.5, 0, D) and bin > 0, in fp32 as the kernel computes them."""
    g = torch.clamp((depth_gt.to(F32) - torch.tensor(1.75, dtype=F32)) / torch.tensor(0.5, dtype=F32), 0, float(D))
    return g, g > 0


def render_losses_ref(c, D, dtype):
    """(loss_depth, loss_rgb, nfg): mean over the foreground of (depth / D - bin / D)^2, mean of (rgb - rgb_gt)^2.  float32: the
    pixel terms in fp32, their squares and sums in fp64, the two totals rounded to fp32 -- the kernel's own split."""
    g, fg = depth_bins(c["depth_gt"], D)
    nfg = int(fg.sum())
    Dt = torch.tensor(float(D), dtype=dtype)
    e = (c["depths"].to(dtype) / Dt - g.to(dtype) / Dt)[fg].to(F64)
    ec = (c["rgbs"].to(dtype) - c["rgb_gt"].to(dtype)).to(F64)
    ld = (e * e).sum() / nfg if nfg else torch.tensor(NAN, dtype=F64)
    lc = (ec * ec).sum() / (3.0 * c["rgbs"].shape[0])
    if dtype == F32:
        ld, lc = ld.to(F32), lc.to(F32)
    return ld.reshape(1), lc.reshape(1), nfg


def render_losses_adj(c, D, gl, nfg, dtype):
    """(drgbs [npix, 3], ddepths [npix]) for the upstream gradients gl = (d loss_depth, d loss_rgb), in the kernel's own order:
    ddepth = gl0 2 (depth / D - bin / D) / (D nfg) on the foreground, drgb = (gl1 2 / (3 npix)) (rgb - rgb_gt)."""
    g, fg = depth_bins(c["depth_gt"], D)
    npix = c["rgbs"].shape[0]
    t = lambda v: torch.tensor(float(v), dtype=F32).to(dtype)
    Dt = t(D)
    e = c["depths"].to(dtype) / Dt - g.to(dtype) / Dt
    dd = torch.where(fg, t(gl[0]) * 2 * e / (Dt * t(nfg)), torch.zeros_like(e)) if nfg else torch.zeros_like(e)
    k = t(gl[1]) * 2 / (3 * t(npix))
    return k * (c["rgbs"].to(dtype) - c["rgb_gt"].to(dtype)), dd


# ----------------------------------------------------------------------------- coocc_upsample_maps
UPSAMPLE = [(1, 1, 1, 16), (2, 3, 5, 16), (1, 2, 3, 4), (1, 3, 4, 3), (1, 2, 2, 2), (3, 2, 4, 1), (1, 5, 7, 8), (1, 1, 33, 12)]


def quad_shares_columns(W, scale):
    """True when every aligned quad of output pixels of a row has one pair of source columns (the kernel's 4-tap branch)."""
    i0, i1, _, _ = lin_src(W, W * scale, F32)
    q0, q3 = torch.arange(0, W * scale, 4), torch.arange(3, W * scale, 4)
    return bool(((i0[q0] == i0[q3]) & (i1[q0] == i1[q3])).all())


# ----------------------------------------------------------------------------- device buffers (the conventions of test_gpu_adjoints.py)
GUARD, SENT = 64, 12345.0


def on_dev(dev, t):
    """A contiguous, 16-byte aligned device copy."""
    t = t.to(dev).contiguous()
    assert t.data_ptr() % 16 == 0
    return t


def guarded(dev, numel, dtype=F32, fill=NAN, sent=SENT):
    """A flat buffer of ``numel`` elements of ``fill`` followed by GUARD sentinels."""
    buf = torch.full((numel + GUARD,), fill, device=dev, dtype=dtype)
    buf[numel:] = sent
    assert buf.data_ptr() % 16 == 0
    return buf


def finish(buf, numel, what, sent=SENT):
    assert bool((buf[numel:] == sent).all()), what + ": wrote behind its output"
    return buf[:numel].clone()


# ----------------------------------------------------------------------------- the camera cases on the device
def cam_setup(dev, H, W, D):
    """(mats [2, 39], xs, ys, ds) of a two-camera rig over an (H, W) frustum with D depth bins, all on ``dev``."""
    import co_occ_amd.synth as synth
    from co_occ_amd.view_transformer import camera_mats, frustum_axes
    size = (H * 64, W * 64)
    rig = synth.camera_rig(2, size, seed=7)
    mats = camera_mats(*[rig[k].to(dev) for k in ("rots", "trans", "intrins", "post_rots", "post_trans", "bda")]).reshape(-1, 39)
    xs, ys, ds = frustum_axes(size, 64, cam_dbound(D), dev)
    assert (ys.numel(), xs.numel(), ds.numel()) == (H, W, D)
    return mats.contiguous(), xs, ys, ds


def run_cams(dev, H, W, D, bname, activated, table=None):
    """maps [2, H, W, 4] (on the CPU) of coocc_render_nearest_cams alone; ``table``: the device table to use (activated = 1: the
    one coocc_render_activate_table has already been through)."""
    from co_occ_amd._lib import call, host_f32, ptr
    X, Y, Z = CAM_GRID
    mats, xs, ys, ds = cam_setup(dev, H, W, D)
    t = on_dev(dev, cam_table(D)) if table is None else table
    if table is None and activated:
        call("coocc_render_activate_table", ptr(t), X * Y * Z)
    zvals = on_dev(dev, torch.linspace(0, D, D, dtype=F32))
    what = "render_nearest_cams " + cam_name(H, W, D, bname)
    buf = guarded(dev, 2 * H * W * 4)
    call("coocc_render_nearest_cams", ptr(t), X, Y, Z, ptr(mats), ptr(xs), ptr(ys), ptr(ds), ptr(zvals), 2, D, H, W,
         host_f32(flat9(CAM_BOUNDS[bname])), activated, ptr(buf))
    return finish(buf, 2 * H * W * 4, what).view(2, H, W, 4).cpu()
