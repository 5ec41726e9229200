"""The volume-rendering kernels on the GPU, each entry alone through the C ABI against float64 at its edge shapes
(tests/render_refs.py: the restatements, the cases and the judging rules; tests/test_render_refs_host.py proves on the CPU that these
rules turn down subtly wrong renderers): ``coocc_render_nearest``, ``coocc_render_nearest_cams`` (both of its forms),
``coocc_render_activate_table``, ``coocc_render_nearest_bwd``, ``coocc_upsample_maps``, ``coocc_raw2outputs``,
``coocc_volume_sampling``, ``coocc_render_losses`` and ``coocc_render_losses_bwd``.

Every buffer a kernel writes starts as NaN and is followed by 64 guard elements that must keep their sentinel; inputs are contiguous
and 16-byte aligned; a kernel without atomics runs twice and must give the same bits.  The discrete parts (voxel indices, masks,
depth bins, the foreground count) are reproduced on the CPU in fp32 and must be equal; the rest is judged by
``util.assert_precise`` against float64 with C_MAX = 4, C_RMS = 2 and a float32 restatement as the anchor -- for the ray kernels the
worse of the plain and the hardware-modelled one.  No verdict compares a kernel with itself.

Which instantiation a parameter reaches (every entry is called by name here, and a TIMER region of a C-ABI call carries nothing but
that name, so ``util.kernels()`` could not tell the template arguments apart; they follow from the dispatch in render_nearest_impl):
  coocc_render_nearest         k_render_nearest<act, D <= 128 ? 4 : 8, false>: D = 129, 255, 256 run CHT = 8 (CH = 5, 8, 8 samples per
                               lane), every other D runs CHT = 4 with CH = ceil(D / 32); W <= 32 is one tile of W rays, W = 33 and 40
                               are a full tile and a tail of 1 and 8
  coocc_render_nearest_cams    k_render_rays_geo<act, 4 or 8> by the same rule on D in a process without COOCC_RENDER_GEO_LDS (this
                               one: the test asserts the variable is not set), (W + 7) / 8 workgroups per row: W = 5 is a partial
                               workgroup, 9 and 33 have a tail of one ray; k_render_nearest<act, 4 or 8, true> in the worker process,
                               which starts with COOCC_RENDER_GEO_LDS=1
  coocc_render_nearest_bwd     one kernel, CH = ceil(D / 64): D <= 64 -> 1, 65 and 128 -> 2, 129 and 192 -> 3, 193 and 256 -> 4
  unit bounds take the subtraction-only branch of the index rule in the forward kernels, every other bounds set the __fdiv_rn one."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from co_occ_amd._lib import call, host_f32, ptr

import render_refs as R
import util

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
D_, guarded, finish = R.on_dev, R.guarded, R.finish


def precise(out, ref64, ref32, what, anchor=None):
    assert not bool(torch.isnan(out).any()), what + ": NaN in the result"
    return util.assert_precise(out.cpu(), ref64, ref32, anchor=anchor, what=what)


def clean(out, what):
    assert not bool(torch.isnan(out).any()), what + ": NaN (the fill value) in the result"


# ============================================================================= coocc_render_activate_table
def activate(dev, table, what="render_activate_table"):
    V = table.shape[0]
    buf = guarded(dev, V * 4)
    buf[:V * 4] = table.to(dev).flatten()
    call("coocc_render_activate_table", ptr(buf), V)
    return finish(buf, V * 4, what).view(V, 4)


@pytest.mark.parametrize("V", R.ACT_V)
def test_render_activate_table(dev, V):
    """One thread per voxel in blocks of 256: V = 1, a last thread, a full block, one voxel into the second block."""
    what = "render_activate_table V=%d" % V
    table = R.no_subnormals(torch.randn(V, 4, generator=R.gen(V)) * 2)
    out = activate(dev, table, what).cpu()
    ref64 = R.activate_ref(table, F64)
    forms = (R.activate_ref(table, F32), R.activate_ref(table, F32, hw=True, seed=V))
    errs = [util.errors(f[:, 1:], ref64[:, 1:]) for f in forms]
    precise(out[:, 1:], ref64[:, 1:], None, what, anchor=(max(e[0] for e in errs), max(e[1] for e in errs)))
    R.assert_exact(out[:, 0], table[:, 0], what + ": sigma passes")
    R.assert_exact(activate(dev, table).cpu(), out, what + ", second call")


# ============================================================================= coocc_render_nearest
@functools.lru_cache(maxsize=None)
def fwd_case(case):
    c = R.ray_case(*case[:5], opaque_first=case[5])
    return c, R.ray_refs(c)


def render_nearest(dev, c, activated, what, geom=None, table=None):
    X, Y, Z = c["dims"]
    N, Dd, H, W = c["N"], c["D"], c["H"], c["W"]
    t = D_(dev, c["table"]).clone() if table is None else table
    if activated and table is None:
        t = activate(dev, c["table"])
    buf = guarded(dev, N * H * W * 4)
    call("coocc_render_nearest", ptr(t), X, Y, Z, ptr(D_(dev, c["geom"] if geom is None else geom)), ptr(D_(dev, c["zvals"])),
         N, Dd, H, W, host_f32(c["bounds"]), activated, ptr(buf))
    return finish(buf, N * H * W * 4, what).view(N, H, W, 4).cpu()


@pytest.mark.parametrize("activated", [0, 1])
@pytest.mark.parametrize("case", R.render_edge_cases(), ids=R.case_id)
def test_render_nearest(dev, case, activated):
    """The geometry-tensor form at every edge shape (render_refs.render_edge_cases: the depths at W = 5, the widths at D = 33, the
    four non-unit bounds, the 10-bit packing limit on each axis, the opaque first sample), with raw logits and with the table that
    coocc_render_activate_table has been through.  Both are judged against the float64 compositing of the raw table."""
    c, (ref64, forms) = fwd_case(case)
    what = "render_nearest %s act=%d" % (R.case_id(case), activated)
    out = render_nearest(dev, c, activated, what)
    clean(out, what)
    R.judge_maps(out, ref64, forms, what)
    flat = out.reshape(-1, 4)
    if c["D"] == 1:
        assert bool((flat[:, 3] == 0).all()), what + ": z = [0], the depth is exactly 0"
    if c["empty_ray"]:
        assert bool((ref64.reshape(-1, 4)[3] == 0).all()) and bool((flat[3] == 0).all()), what + ": the ray through empty voxels"
    if case[0] in R.PACKING:
        axis = R.PACKING.index(case[0])
        assert int(c["idx"][..., axis].max()) == 1023 and int(c["idx"][..., axis][c["inside"]].min()) == 0
    R.assert_exact(render_nearest(dev, c, activated, what), out, what + ", second call")


def test_render_nearest_refuses_more_than_256_samples(dev):
    """D = 257 is beyond the 8 samples per lane of the widest instantiation: the entry says so instead of launching."""
    from co_occ_amd._lib import CooccArgError
    c = R.ray_case("unit", 1, 2, 1, 1)
    buf = guarded(dev, 4)
    with pytest.raises(CooccArgError):
        call("coocc_render_nearest", ptr(D_(dev, c["table"])), 12, 10, 6, ptr(D_(dev, torch.zeros(1, 257, 1, 1, 3))),
             ptr(D_(dev, torch.zeros(257))), 1, 257, 1, 1, host_f32(c["bounds"]), 0, ptr(buf))
    assert bool(torch.isnan(finish(buf, 4, "refused call")).all())


# ============================================================================= coocc_render_nearest_cams
def cam_geometry(dev, H, W, D):
    """[2, D, H, W, 3] of the device's own coocc_get_geometry for the case's constants."""
    from co_occ_amd.view_transformer import geometry_from_mats
    mats, xs, ys, ds = R.cam_setup(dev, H, W, D)
    return geometry_from_mats(mats, xs, ys, ds, 1, 2)[0].contiguous()


@pytest.fixture(scope="module")
def cam_results(dev):
    """Per camera case and table form: the maps of the in-kernel-geometry entry in this process (the LDS-free form), and per case the
    references over the device's own geometry tensor."""
    assert "COOCC_RENDER_GEO_LDS" not in os.environ, "this process must run the LDS-free form"
    res = {}
    for H, W, Dd, b in R.CAM_CASES:
        geom = cam_geometry(dev, H, W, Dd)
        bounds = R.flat9(R.CAM_BOUNDS[b])
        idx, inside = R.sample_index(geom.cpu(), bounds)
        c = dict(dims=R.CAM_GRID, bounds=bounds, table=R.cam_table(Dd), geom=geom, idx=idx, inside=inside,
                 zvals=torch.linspace(0, Dd, Dd, dtype=F32), N=2, D=Dd, H=H, W=W, seed=Dd)
        ref64, forms = R.ray_refs(c)
        res[R.cam_name(H, W, Dd, b)] = dict(c=c, ref64=ref64, forms=forms, maps={a: R.run_cams(dev, H, W, Dd, b, a) for a in (0, 1)})
    return res


@pytest.mark.parametrize("activated", [0, 1])
@pytest.mark.parametrize("H,W,Dd,b", R.CAM_CASES, ids=lambda v: str(v))
def test_render_nearest_cams(dev, cam_results, H, W, Dd, b, activated):
    """The LDS-free in-kernel-geometry form: judged against float64 over the positions the device's own coocc_get_geometry gives for
    the same constants, and bit-equal to coocc_render_nearest on that tensor."""
    r = cam_results[R.cam_name(H, W, Dd, b)]
    c, what = r["c"], "render_nearest_cams %s act=%d" % (R.cam_name(H, W, Dd, b), activated)
    out = r["maps"][activated]
    clean(out, what)
    assert bool(c["inside"].any()) and not bool(c["inside"].all()), what + ": samples inside and outside"
    R.judge_maps(out, r["ref64"], r["forms"], what)
    R.assert_exact(render_nearest(dev, c, activated, what), out, what + " vs the geometry-tensor form")
    R.assert_exact(R.run_cams(dev, H, W, Dd, b, activated), out, what + ", second call")


def test_two_phase_in_kernel_geometry_form(dev, cam_results, tmp_path):
    """COOCC_RENDER_GEO_LDS=1 (read once per process) selects k_render_nearest<.., .., true>: a fresh child process runs every camera
    case with it; its maps are judged by the same rules and must have the bits of this process's LDS-free results.  W = 5 and 9 are
    one tile of W rays (the phase-2 loop over 8 rays per step with a tail), W = 33 a full 32-ray tile and a tile of one ray."""
    path = str(tmp_path / "geo_lds.npz")
    env = dict(os.environ, COOCC_RENDER_GEO_LDS="1")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "render_geo_lds_worker.py")
    p = subprocess.run([sys.executable, worker, path], env=env, timeout=120, capture_output=True, text=True)
    assert p.returncode == 0, "the worker failed (%d):\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    got = np.load(path)
    for H, W, Dd, b in R.CAM_CASES:
        r = cam_results[R.cam_name(H, W, Dd, b)]
        for a in (0, 1):
            what = "render_nearest_cams two-phase %s act=%d" % (R.cam_name(H, W, Dd, b), a)
            out = torch.from_numpy(got["%s_a%d" % (R.cam_name(H, W, Dd, b), a)])
            clean(out, what)
            R.judge_maps(out, r["ref64"], r["forms"], what)
            R.assert_exact(out, r["maps"][a], what + " vs the LDS-free form")


# ============================================================================= coocc_render_nearest_bwd
def render_bwd(dev, c, dmaps, what, buf=None):
    X, Y, Z = c["dims"]
    n = X * Y * Z * 4
    buf = guarded(dev, n) if buf is None else buf
    call("coocc_render_nearest_bwd", ptr(D_(dev, c["table"])), X, Y, Z, ptr(D_(dev, c["geom"])), ptr(D_(dev, c["zvals"])),
         c["N"], c["D"], c["H"], c["W"], host_f32(c["bounds"]), ptr(D_(dev, dmaps)), ptr(buf))
    return finish(buf, n, what).view(-1, 4).cpu(), buf


BWD_CASES = [v + ("all",) for v in R.bwd_edge_cases()] + [("wide", 2, 129, 3, 5, "depth"), ("wide", 2, 129, 3, 5, "rgb"),
                                                           ("half", 2, 24, 3, 5, "depth"), ("half", 2, 24, 3, 5, "rgb")]


@pytest.mark.parametrize("case", BWD_CASES, ids=lambda v: "%s-N%d-D%d-H%d-W%d-%s" % v)
def test_render_nearest_bwd(dev, case):
    """dtable against the analytic float64 gradient (render_refs.render_adj, tied to autograd by the host test).  The anchor is the
    worst of the float32 evaluations of render_refs.bwd_anchor: three seeded orders of the contributions (the atomics), each with the
    two recurrences sample after sample and in the kernel's own scan order -- the sigma column of these small cases hangs on one or
    two large entries, whose rounding differs by a factor of 3 between the two orders.  The sigma column and the three
    logit columns are judged apart.
    ``depth`` / ``rgb``: only that part of dmaps is non-zero."""
    c = R.ray_case(*case[:5])
    what = "render_nearest_bwd %s-N%d-D%d-H%d-W%d-%s" % case
    dmaps = R.no_subnormals(torch.randn(c["N"], c["H"], c["W"], 4, generator=R.gen(case[2] + 7)))
    if case[5] == "depth":
        dmaps[..., :3] = 0
    if case[5] == "rgb":
        dmaps[..., 3] = 0
    out, buf = render_bwd(dev, c, dmaps, what)
    clean(out, what)
    ref64 = R.render_adj(c, dmaps, F64)
    for nm, col in (("sigma", R.SIGMA), ("logits", R.LOGITS)):
        precise(out[:, col], ref64[:, col], None, what + " " + nm, anchor=R.bwd_anchor(c, dmaps, ref64, col))
    assert bool((out[~R.touched(c)] == 0).all()), what + ": a voxel no sample touches"
    again, _ = render_bwd(dev, c, dmaps, what + ", second call", buf)          # the entry clears the table itself
    assert torch.equal(again != 0, out != 0), what + ": the second call on the same buffer has other non-zero voxels"


# ============================================================================= coocc_upsample_maps
def upsample(dev, maps, scale, what, with_rgb=True):
    N, H, W, _ = maps.shape
    npx = N * H * scale * W * scale
    rb, db = guarded(dev, npx * 3), guarded(dev, npx)
    call("coocc_upsample_maps", ptr(D_(dev, maps)), N, H, W, scale, ptr(rb if with_rgb else None), ptr(db))
    rgbs = finish(rb, npx * 3, what + " rgbs").view(N, H * scale, W * scale, 3).cpu()
    return rgbs, finish(db, npx, what + " depths").view(N, H * scale, W * scale).cpu()


@pytest.mark.parametrize("N,H,W,scale", R.UPSAMPLE)
def test_upsample_maps(dev, N, H, W, scale):
    """Scales 16 and 8 take the 4-tap branch (a quad of output pixels shares its source columns), 1, 2, 3, 4 and 12 reach the
    per-pixel one (the host test checks which); the totals are 64 quads (one full wave), 24, 27, 4 and 6 (one partial wave), 1920 (a last
    half block), 560 and 1188 (a last partial wave)."""
    what = "upsample_maps %dx%dx%d x%d" % (N, H, W, scale)
    g = R.gen(N + 10 * H + 100 * W + scale)
    maps = R.no_subnormals(torch.randn(N, H, W, 4, generator=g))
    rgbs, depths = upsample(dev, maps, scale, what)
    (r64, d64), (r32, d32) = R.maps_fwd(maps, scale, F64), R.maps_fwd(maps, scale, F32)
    precise(rgbs, r64, r32, what + " rgbs")
    precise(depths, d64, d32, what + " depths")
    r2, d2 = upsample(dev, maps, scale, what)
    R.assert_exact(r2, rgbs, what + ", second call")
    R.assert_exact(d2, depths, what + ", second call")
    nan_rgb, d3 = upsample(dev, maps, scale, what + " depth-only", with_rgb=False)
    R.assert_exact(d3, depths, what + ": the depth-only form")
    assert bool(torch.isnan(nan_rgb).all()), what + ": the depth-only form wrote colours"
    if scale & (scale - 1) == 0:                  # power-of-two scale: weights k / (2 scale), integer maps: every term exact
        imaps = torch.randint(-4, 5, (N, H, W, 4), generator=g).to(F32)
        ri, di = upsample(dev, imaps, scale, what + " exact")
        (r64, d64), (r32, d32) = R.maps_fwd(imaps, scale, F64), R.maps_fwd(imaps, scale, F32)
        R.assert_exact(ri + 0.0, R.exact_ref(r64, r32), what + " exact rgbs")
        R.assert_exact(di + 0.0, R.exact_ref(d64, d32), what + " exact depths")


# ============================================================================= coocc_raw2outputs
def raw2outputs(dev, c, R_, S, white, with_weights, what):
    rb, db, wb = guarded(dev, R_ * 3), guarded(dev, R_), guarded(dev, R_ * S)
    call("coocc_raw2outputs", ptr(D_(dev, c["raw"])), ptr(D_(dev, c["z"])), R_, S, white, c["zmin"], c["zmax"], ptr(rb), ptr(db),
         ptr(wb if with_weights else None))
    return (finish(rb, R_ * 3, what).view(R_, 3).cpu(), finish(db, R_, what).cpu(), finish(wb, R_ * S, what).view(R_, S).cpu())


@pytest.mark.parametrize("S", R.RAW_S)
@pytest.mark.parametrize("R_", R.RAW_R)
def test_raw2outputs(dev, R_, S):
    """One wave per ray, CH = ceil(S / 64) samples per lane: S = 1, 16, 63 leave lanes without a sample, 64 fills the wave, 65 and
    130 run CH = 2 and 3 with a partial last lane; R = 1, 3, 5 leave waves of the last workgroup without a ray."""
    c = R.raw_case(R_, S)
    zmin, zmax = (float(torch.tensor(v, dtype=F32)) for v in (c["zmin"], c["zmax"]))
    for white in (0, 1):
        what = "raw2outputs R=%d S=%d white=%d" % (R_, S, white)
        rgb, depth, w = raw2outputs(dev, c, R_, S, white, True, what)
        r64, d64, w64 = R.raw2outputs_ref(c["raw"], c["z"], white, zmin, zmax, F64)
        r32, d32, w32 = R.raw2outputs_ref(c["raw"], c["z"], white, zmin, zmax, F32)
        precise(rgb, r64, r32, what + " rgb")
        precise(w, w64, w32, what + " weights")
        heavy = w64.sum(1) >= 0.1                 # below that the division by sum w + 1e-8 amplifies the rounding of the sums
        if bool(heavy.any()):
            precise(depth[heavy], d64[heavy], d32[heavy], what + " depth")
        clean(depth, what)
        assert bool(((depth >= zmin) & (depth <= zmax)).all()), what + ": depth outside [zmin, zmax]"
        if R_ >= 3:
            assert bool((w[1] == 0).all()) and float(depth[1]) == zmin and bool((rgb[1] == float(white)).all()), what + ": empty ray"
            assert float(w[2, 0]) == 1.0 and float(w[2, 1:].abs().max() if S > 1 else 0.0) <= 1e-9, what + ": opaque first sample"
        rgb2, depth2, w2 = raw2outputs(dev, c, R_, S, white, True, what)
        for a, b in ((rgb2, rgb), (depth2, depth), (w2, w)):
            R.assert_exact(a, b, what + ", second call")
        rgb3, depth3, w3 = raw2outputs(dev, c, R_, S, white, False, what + " weights=NULL")
        R.assert_exact(rgb3, rgb, what + " weights=NULL")
        R.assert_exact(depth3, depth, what + " weights=NULL")
        assert bool(torch.isnan(w3).all())


# ============================================================================= coocc_volume_sampling
def volume_sampling(dev, c, what):
    n, C = c["n"], c["C"]
    fb, mb = guarded(dev, n * C), guarded(dev, n, dtype=torch.uint8, fill=7, sent=99)
    call("coocc_volume_sampling", ptr(D_(dev, c["rows"])), C, *c["vol"], ptr(D_(dev, c["pts"])), n, host_f32(c["aabb"]), ptr(fb), ptr(mb))
    return finish(fb, n * C, what).view(n, C).cpu(), finish(mb, n, what, sent=99).cpu()


@pytest.mark.parametrize("n", R.VS_N)
@pytest.mark.parametrize("C", R.VS_C)
@pytest.mark.parametrize("vol", R.VS_VOLS, ids=lambda v: "%dx%dx%d" % v)
def test_volume_sampling(dev, vol, C, n):
    """One wave per point, lanes over the channels: C = 1 and 8 leave lanes idle, 64 fills the wave, 65 and 130 loop with a partial
    last pass; n = 1, 63 and 257 leave waves of the last workgroup without a point.  A volume axis of 1 has both taps on index 0.
    Points inside, outside (clamped to the border) and, in the power-of-two box, exactly on faces, edges and corners."""
    for kind in ("generic", "pow2"):
        c = R.vs_case(vol, C, n, kind)
        what = "volume_sampling %dx%dx%d C=%d n=%d %s" % (vol + (C, n, kind))
        feat, mask = volume_sampling(dev, c, what)
        f64, m = R.volume_sampling_ref(c["rows"], vol, c["pts"], c["aabb"], F64)
        f32, _ = R.volume_sampling_ref(c["rows"], vol, c["pts"], c["aabb"], F32)
        precise(feat, f64, f32, what)
        assert torch.equal(mask, m.to(torch.uint8)), what + ": the in-box mask"
        if n > 1:
            assert bool(m.any()) and not bool(m.all())
        feat2, mask2 = volume_sampling(dev, c, what)
        R.assert_exact(feat2, feat, what + ", second call")
        assert torch.equal(mask2, mask)


# ============================================================================= coocc_render_losses / _bwd
def render_losses(dev, c, Dd, what):
    npix = c["depths"].numel()
    ob = guarded(dev, 3)
    ws = torch.zeros(3 * 1024, device=dev, dtype=F64)
    a = [D_(dev, c[k]) for k in ("rgbs", "depths", "rgb_gt", "depth_gt")]
    call("coocc_render_losses", *[ptr(t) for t in a], npix, Dd, ptr(ob), ptr(ws), ws.numel() * 8)
    out = finish(ob, 3, what)
    gl = (0.7, -1.3)
    rb, db = guarded(dev, npix * 3), guarded(dev, npix)
    call("coocc_render_losses_bwd", *[ptr(t) for t in a], npix, Dd, ptr(out), ptr(D_(dev, torch.tensor(gl, dtype=F32))), ptr(rb), ptr(db))
    return out.cpu(), finish(rb, npix * 3, what + " drgbs").view(npix, 3).cpu(), finish(db, npix, what + " ddepths").cpu(), gl


@pytest.mark.parametrize("Dd", R.LOSS_D)
@pytest.mark.parametrize("npix", R.LOSS_NPIX)
def test_render_losses_and_their_gradients(dev, npix, Dd):
    """npix = 1 and 255 are one partial block, 1024 one block's full slice, 1025 two blocks, 70000 69 blocks of the grid-stride loop.
    The sums are fp64 on the device: the anchor is the float32 rounding of the terms and of the result."""
    c = R.loss_case(npix, Dd)
    what = "render_losses npix=%d D=%d" % (npix, Dd)
    out, drgbs, ddepths, gl = render_losses(dev, c, Dd, what)
    ld64, lc64, nfg = R.render_losses_ref(c, Dd, F64)
    ld32, lc32, _ = R.render_losses_ref(c, Dd, F32)
    assert float(out[2]) == nfg > 0, what + ": foreground count %r vs %d" % (float(out[2]), nfg)
    precise(out[0:1], ld64, ld32, what + " loss_depth")
    precise(out[1:2], lc64, lc32, what + " loss_rgb")
    (r64, d64), (r32, d32) = R.render_losses_adj(c, Dd, gl, nfg, F64), R.render_losses_adj(c, Dd, gl, nfg, F32)
    precise(drgbs, r64, r32, what + " drgbs")
    precise(ddepths, d64, d32, what + " ddepths")
    _, fg = R.depth_bins(c["depth_gt"], Dd)
    assert bool((ddepths[~fg] == 0).all()), what + ": a background pixel has a depth gradient"
    out2, drgbs2, ddepths2, _ = render_losses(dev, c, Dd, what)
    for a, b in ((out2, out), (drgbs2, drgbs), (ddepths2, ddepths)):
        R.assert_exact(a, b, what + ", second call")


def test_render_losses_without_foreground(dev):
    """No foreground pixel: the depth loss is 0 / 0 = NaN like torch's mean of an empty selection, the count 0, no depth gradient."""
    c = R.loss_case(255, 16, foreground=False)
    out, drgbs, ddepths, gl = render_losses(dev, c, 16, "render_losses without foreground")
    _, lc64, nfg = R.render_losses_ref(c, 16, F64)
    assert nfg == 0 and bool(torch.isnan(out[0])) and float(out[2]) == 0.0
    precise(out[1:2], lc64, R.render_losses_ref(c, 16, F32)[1], "render_losses without foreground loss_rgb")
    assert bool((ddepths == 0).all())
    precise(drgbs, R.render_losses_adj(c, 16, gl, 0, F64)[0], R.render_losses_adj(c, 16, gl, 0, F32)[0], "render_losses without foreground drgbs")
