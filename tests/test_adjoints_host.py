"""The linear adjoint entries of csrc/backward.hip without a GPU: (1) the restatements of tests/adjoint_refs.py agree with torch in
float64, forward and autograd, at every shape tests/test_gpu_adjoints.py uses; (2) the inputs have the properties the GPU tests
rely on (exact cases agree bit for bit between float32 and float64, the camera rig keeps its margin to every mask branch, the pooling
geometry fills the truncation band); (3) each judging rule rejects wrong adjoints made on the CPU and passes a correct fp32 one;
(4) every entry refuses bad arguments with COOCC_EINVAL and a message naming it, before any launch."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from co_occ_amd import _lib

import adjoint_refs as R
import util

F32, F64 = torch.float32, torch.float64
ONE = ctypes.c_void_p(16)       # a non-null dummy address: validation never dereferences device pointers
REL = 1e-12


def close(a, b, what):
    a, b = a.to(F64), b.to(F64)
    assert a.shape == b.shape, "%s: shape %s vs %s" % (what, tuple(a.shape), tuple(b.shape))
    scale = max(float(b.abs().max()), 1e-300) if b.numel() else 1.0
    err = float((a - b).abs().max()) / scale if b.numel() else 0.0
    assert err <= REL, "%s: %.3e relative to the reference's scale" % (what, err)


def ncdhw(t):
    return t.permute(0, 4, 1, 2, 3).contiguous()


def last(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


# ----------------------------------------------------------------------------- 1. the restatements against torch in float64
TRI_ALL = R.TRI_EXACT + R.TRI_PRECISE + [R.TRI_COPY]


@pytest.mark.parametrize("B,C,coarse,fine", TRI_ALL)
def test_trilinear_restatement_agrees_with_torch(B, C, coarse, fine):
    g = R.gen(1)
    x = torch.randn((B,) + coarse + (C,), generator=g, dtype=F64)
    dy = torch.randn((B,) + fine + (C,), generator=g, dtype=F64)
    xa = ncdhw(x).requires_grad_(True)
    y = F.interpolate(xa, size=fine, mode="trilinear", align_corners=False)
    y.backward(ncdhw(dy))
    close(R.trilinear_fwd(x, fine, F64), last(y.detach()), "trilinear forward")
    close(R.trilinear_adj(dy, coarse, F64), last(xa.grad), "trilinear adjoint")
    close(R.trilinear_adj_fused(dy, coarse, F64), last(xa.grad), "trilinear adjoint, fused weights")


@pytest.mark.parametrize("N,H,W,scale", R.MAPS_EXACT + R.MAPS_PRECISE + [R.MAPS_COPY])
def test_maps_restatement_agrees_with_torch(N, H, W, scale):
    g = R.gen(2)
    maps = torch.randn(N, H, W, 4, generator=g, dtype=F64)
    dr = torch.randn(N, H * scale, W * scale, 3, generator=g, dtype=F64)
    dd = torch.randn(N, H * scale, W * scale, generator=g, dtype=F64)
    ma = maps.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    up = F.interpolate(ma, size=(H * scale, W * scale), mode="bilinear", align_corners=False)
    rgbs, depths = R.maps_fwd(maps, scale, F64)
    close(rgbs, up[:, :3].permute(0, 2, 3, 1).detach(), "maps forward rgb")
    close(depths, up[:, 3].detach(), "maps forward depth")
    up.backward(torch.cat([dr.permute(0, 3, 1, 2), dd[:, None]], 1))
    close(R.maps_adj(dr, dd, N, H, W, scale, F64), ma.grad.permute(0, 2, 3, 1), "maps adjoint")


@pytest.mark.parametrize("name", list(R.MIX))
def test_mix_restatement_agrees_with_torch(name):
    c = R.mix_case(name)
    B, C, dims = c["B"], c["C"], c["dims"]
    X0, Y0, Z0 = dims[0]
    lv = [ncdhw(p.to(F64)).requires_grad_(True) for p in c["levels"]]
    V0, L = B * X0 * Y0 * Z0, len(dims)
    wl = (torch.zeros(V0, L, dtype=F64) if c["wlogit"] is None else c["wlogit"].to(F64)).requires_grad_(True)
    ups = [F.interpolate(p, size=dims[0], mode="trilinear", align_corners=False) if tuple(p.shape[2:]) != dims[0] else p for p in lv]
    w = torch.softmax(wl, 1)
    out = sum(w[:, l:l + 1] * last(ups[l]).reshape(V0, C) for l in range(L))
    out.backward(c["dout"].to(F64))
    close(R.mix_fwd(c["levels"], c["wlogit"], F64), out.detach(), "mix forward")
    gl, dwl = R.mix_adj(c["levels"], c["wlogit"], c["dout"], F64)
    close(dwl, wl.grad, "mix dwlogit")
    for l, d in enumerate(R.mix_level_grads(c["levels"], gl, F64)):
        close(d, last(lv[l].grad), "mix gradient of level %d" % l)


def vox_lists():
    full = R.fine_children(R.vox_coarse_list().long(), R.VOX_DIMS)
    return {"children": full, "repeats": R.vox_repeat_list(), "corners": R.vox_corner_list(), "one": full[:, 5:6].contiguous()}


@pytest.mark.parametrize("C", R.VOX_C)
@pytest.mark.parametrize("which", ["children", "repeats", "corners", "one"])
def test_voxel_sampler_restatement_agrees_with_torch(C, which):
    xyz = vox_lists()[which]
    X, Y, Z = R.VOX_DIMS
    g = R.gen(3)
    vol = torch.randn(X, Y, Z, C, generator=g, dtype=F64)
    df = torch.randn(xyz.shape[1], C, generator=g, dtype=F64)
    va = vol.permute(3, 0, 1, 2)[None].contiguous().requires_grad_(True)
    gn = torch.stack([(xyz[a].to(F64) / (R.VOX_FINAL[a] - 1) - 0.5) * 2 for a in (2, 1, 0)], 1)      # grid x walks the last axis
    y = F.grid_sample(va, gn[None, None, None], mode="bilinear", padding_mode="zeros", align_corners=False)[0, :, 0, 0].t()
    y.backward(df)
    close(R.sample_voxel_fwd(vol, xyz, R.VOX_FINAL, F64), y.detach(), "voxel sampler forward")
    close(R.sample_voxel_adj(df, xyz, R.VOX_FINAL, R.VOX_DIMS, F64), va.grad[0].permute(1, 2, 3, 0), "voxel sampler adjoint")


def test_fine_children_cover_every_corner_of_the_final_grid():
    full = vox_lists()["children"]
    have = {tuple(p) for p in full.t().tolist()}
    fx, fy, fz = (f - 1 for f in R.VOX_FINAL)
    assert all((x, y, z) in have for x in (0, fx) for y in (0, fy) for z in (0, fz))
    _, _, ok = R.voxel_taps(R.vox_corner_list()[:, :8], R.VOX_FINAL, R.VOX_DIMS, F64)
    assert bool((ok.sum(1) == 1).all()), "a corner of the final grid keeps exactly one of its eight taps"
    assert len(have) == full.shape[1]
    rep = R.vox_repeat_list()
    assert torch.equal(rep[:, :full.shape[1]], full) and bool((rep[:, full.shape[1]:] == torch.tensor([[5], [7], [3]])).all())
    assert rep.shape[1] == full.shape[1] + 50
    assert R.vox_corner_list().shape[1] == 58


def test_atomics_anchor_is_the_worst_of_three_seeded_orders():
    """Permuting the contributions leaves the float64 sum where it is (to 1e-12) and moves the fp32 one; the anchor is the worst of
    the three and a correct fp32 result in a fourth order passes rule 2 under it."""
    xyz = R.vox_repeat_list()
    df = R.normal((xyz.shape[1], 4), R.gen(11))
    adj = lambda dtype: (lambda order=None: R.sample_voxel_adj(df, xyz, R.VOX_FINAL, R.VOX_DIMS, dtype, order))
    ref64 = adj(F64)()
    close(adj(F64)(order=2), ref64, "float64 in a permuted order")
    errs = [util.errors(adj(F32)(order=s), ref64) for s in (1, 2, 3)]
    assert len(set(errs)) == 3, "the seeded orders give one fp32 result"
    anchor = R.atomics_anchor(adj(F32), ref64)
    assert anchor == (max(e[0] for e in errs), max(e[1] for e in errs))
    assert util.precision(adj(F32)(order=4), ref64, anchor=anchor, what="(host) a fourth order")["ok"]
    prm, grid = R.camera_rig()
    di = R.normal((grid.shape[1], 4), R.gen(12))
    close(R.sample_img_adj(di, prm, grid, 2, 6, 8, F64, order=3), R.sample_img_adj(di, prm, grid, 2, 6, 8, F64), "image sampler, permuted")


@pytest.mark.parametrize("Ci", R.IMG_C)
@pytest.mark.parametrize("Hf,Wf", R.IMG_MAPS)
@pytest.mark.parametrize("post_rot", [False, True])
def test_image_sampler_restatement_agrees_with_torch(Ci, Hf, Wf, post_rot):
    prm, xyz = R.camera_rig(post_rot)
    g = R.gen(4)
    img = torch.randn(2, Hf, Wf, Ci, generator=g, dtype=F64)
    df = torch.randn(xyz.shape[1], Ci, generator=g, dtype=F64)
    ia = img.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = 0
    for cam, (u2, v2, _, m, _) in enumerate(R.project(prm, xyz, 2, F64)):
        grid = torch.stack([u2, v2], 1)[None, None]
        s = F.grid_sample(ia[cam:cam + 1], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, 0].t()
        y = y + s * m[:, None].to(F64)
    y.backward(df)
    close(R.sample_img_fwd(img, prm, xyz, F64), y.detach(), "image sampler forward")
    close(R.sample_img_adj(df, prm, xyz, 2, Hf, Wf, F64), ia.grad.permute(0, 2, 3, 1), "image sampler adjoint")


@pytest.mark.parametrize("gname", list(R.POOL_GRIDS))
@pytest.mark.parametrize("N,D,H,W,C,B,grid", R.POOL)
def test_pooling_restatements_agree_with_torch(N, D, H, W, C, B, grid, gname):
    c = R.pool_case(N, D, H, W, C, B, grid, gname, exact=False)
    keys, kept = c["keys"], c["keys"] >= 0
    depth, feat = c["depth"].to(F64).requires_grad_(True), c["feat"].to(F64).requires_grad_(True)
    pix = R._pix(N, D, H * W)
    vol = depth.reshape(-1, 1) * feat[pix]
    vol.retain_grad()
    out = torch.zeros(c["nvox"], C, dtype=F64).index_add(0, keys[kept], vol[kept])
    out.backward(c["dout"].to(F64))
    close(R.lift_splat_fwd(c["depth"], c["feat"], keys, c["nvox"], F64), out.detach(), "lift-splat forward")
    dd, dfe = R.lift_splat_adj(c["dout"], c["depth"], c["feat"], keys, F64)
    close(dd, depth.grad, "lift-splat d_depth")
    close(dfe, feat.grad, "lift-splat d_feat")
    close(R.voxel_pool_adj(c["dout"], keys, F64), vol.grad, "voxel pooling adjoint")


@pytest.mark.parametrize("n,C,rows,ss,ds", R.SCATTER)
def test_scatter_restatement_agrees_with_torch(n, C, rows, ss, ds):
    c = R.scatter_case(n, C, rows, exact=False)
    ref = c["dst"].to(F64).clone()
    for r in range(n):
        if int(c["idx"][r]) >= 0:
            ref[int(c["idx"][r])] += c["src"][r].to(F64)
    close(R.scatter_add(c["dst"], c["src"], c["idx"], F64), ref, "scatter_add_rows")
    assert bool((c["idx"] == -1).any())


# ----------------------------------------------------------------------------- 2. the inputs have the properties the GPU tests rely on
@pytest.mark.parametrize("B,C,coarse,fine", R.TRI_EXACT)
def test_exact_trilinear_cases_are_exact(B, C, coarse, fine):
    c = R.tri_case(B, C, coarse, fine, exact=True)
    R.exact_ref(R.trilinear_adj(c["dfine"], coarse, F64), R.trilinear_adj(c["dfine"], coarse, F32))
    R.exact_ref(R.trilinear_adj(c["dfine"], coarse, F64), R.trilinear_adj_fused(c["dfine"], coarse, F32))
    assert float(c["dfine"].abs().max()) <= 4


@pytest.mark.parametrize("N,H,W,scale", R.MAPS_EXACT)
def test_exact_maps_cases_are_exact(N, H, W, scale):
    g = R.gen(N + H + W + scale)
    dr, dd = R.ints((N, H * scale, W * scale, 3), g, -4, 4), R.ints((N, H * scale, W * scale), g, -4, 4)
    R.exact_ref(R.maps_adj(dr, dd, N, H, W, scale, F64), R.maps_adj(dr, dd, N, H, W, scale, F32))


@pytest.mark.parametrize("name", R.MIX_EXACT)
def test_exact_mix_cases_are_exact(name):
    c = R.mix_case(name, exact=True)
    g64, d64 = R.mix_adj(c["levels"], c["wlogit"], c["dout"], F64)
    g32, d32 = R.mix_adj(c["levels"], c["wlogit"], c["dout"], F32)
    for a, b in zip(g64, g32):
        R.exact_ref(a, b)
    R.exact_ref(d64, d32)
    for a, b in zip(R.mix_level_grads(c["levels"], g64, F64), R.mix_level_grads(c["levels"], g32, F32)):
        R.exact_ref(a, b)
    if name == "L1":
        assert bool((d64 == 0).all()) and R.bits_equal(g32[0], c["dout"])


def test_exact_sampler_and_pooling_cases_are_exact():
    xyz = R.vox_corner_list()
    df = R.ints((xyz.shape[1], 4), R.gen(6), -4, 4)
    R.exact_ref(R.sample_voxel_adj(df, xyz, R.VOX_FINAL, R.VOX_DIMS, F64), R.sample_voxel_adj(df, xyz, R.VOX_FINAL, R.VOX_DIMS, F32))
    prm, grid = R.camera_rig()
    di = R.ints((grid.shape[1], 4), R.gen(7), -4, 4)
    R.exact_ref(R.sample_img_adj(di, prm, grid, 2, 1, 1, F64), R.sample_img_adj(di, prm, grid, 2, 1, 1, F32))
    for shape in R.POOL:
        c = R.pool_case(*shape, "offset", exact=True)
        a, b = R.lift_splat_adj(c["dout"], c["depth"], c["feat"], c["keys"], F64), R.lift_splat_adj(c["dout"], c["depth"], c["feat"], c["keys"], F32)
        R.exact_ref(a[0], b[0])
        R.exact_ref(a[1], b[1])
        R.exact_ref(R.lift_splat_fwd(c["depth"], c["feat"], c["keys"], c["nvox"], F64))


@pytest.mark.parametrize("post_rot", [False, True])
def test_camera_rig_keeps_its_margin_to_every_mask_branch(post_rot):
    prm, grid = R.camera_rig(post_rot)
    p64, p32 = R.project(prm, grid, 2, F64), R.project(prm, grid, 2, F32)
    for cam in range(2):
        assert float(p64[cam][4].min()) >= 1e-3, "camera %d: a point is %.2e from a mask branch" % (cam, float(p64[cam][4].min()))
        assert torch.equal(p64[cam][3], p32[cam][3]), "camera %d: the fp32 mask differs from the float64 one" % cam
    assert bool(p64[0][3].all()), "camera 0 sees every point"
    vis, behind = float(p64[1][3].double().mean()), float((p64[1][2] <= 0).double().mean())
    assert 0.4 <= vis <= 0.6 and 0.2 <= behind <= 0.3, "camera 1 sees %.2f of the points, %.2f are behind it" % (vis, behind)


@pytest.mark.parametrize("gname", list(R.POOL_GRIDS))
@pytest.mark.parametrize("N,D,H,W,C,B,grid", R.POOL[1:])             # (the first shape is a single point)
def test_pooling_geometry_fills_the_truncation_band(N, D, H, W, C, B, grid, gname):
    c = R.pool_case(N, D, H, W, C, B, grid, gname, exact=True)
    l = torch.tensor(c["lo_dx"], dtype=F32)
    gq = (c["geom"] - l[:3]) / l[3:]
    band = ((gq > -1) & (gq < 0)).any(1).double().mean()
    kept = (c["keys"] >= 0).double().mean()
    assert float(band) >= 0.05 and float(1 - kept) >= 0.10 and float(kept) >= 0.50, "band %.3f, outside %.3f, kept %.3f" % (band, 1 - kept, kept)
    in_band_kept = (((gq > -1) & (gq < 0)).any(1) & (c["keys"] >= 0)).double().mean()
    assert float(in_band_kept) >= 0.05, "points of the band (-1, 0) that truncation keeps: %.3f" % in_band_kept
    if B > 1:
        assert len({int(k) // (c["nvox"] // B) for k in c["keys"].tolist() if k >= 0}) == B
    pix_last = c["keys"].reshape(N, D, H * W)[N - 1, :, H * W - 1]
    assert bool((pix_last < 0).all()), "the last pixel's whole ray is outside"


# ----------------------------------------------------------------------------- 3. the judging rules bite
def judged(wrong32, ref64, ref32, exact64=None, wrong_exact=None, what=""):
    """A wrong fp32 adjoint is turned down by rule 2 (and, when an exact case is given, by rule 1), a correct one passes both."""
    assert R.rejects(wrong32, ref64, ref32), what + ": rule 2 lets the wrong adjoint through"
    assert not R.rejects(ref32, ref64, ref32)
    if exact64 is not None:
        assert not R.bits_equal(wrong_exact, R.exact_ref(exact64)), what + ": rule 1 lets the wrong adjoint through"


@pytest.mark.parametrize("mutate", ["drop_last", "shift", "align_corners"])
def test_rules_reject_wrong_resampling_adjoints(mutate):
    for (B, C, coarse, fine), (eB, eC, ecoarse, efine) in zip(R.TRI_PRECISE[:2], R.TRI_EXACT[1:3]):
        c, e = R.tri_case(B, C, coarse, fine, False), R.tri_case(eB, eC, ecoarse, efine, True)
        ref64, ref32 = R.trilinear_adj(c["dfine"], coarse, F64), R.trilinear_adj(c["dfine"], coarse, F32)
        for axis in range(3):
            if coarse[axis] == fine[axis] or ecoarse[axis] == efine[axis] or ecoarse[axis] == 1:
                continue
            if torch.equal(R.axis_matrix(coarse[axis], fine[axis], F64, mutate), R.axis_matrix(coarse[axis], fine[axis], F64)):
                continue          # 2 -> 3 samples: both conventions give the taps 0, 1/2, 1
            m = tuple(mutate if a == axis else None for a in range(3))
            judged(R.trilinear_adj(c["dfine"], coarse, F32, m), ref64, ref32, R.trilinear_adj(e["dfine"], ecoarse, F64),
                   R.trilinear_adj(e["dfine"], ecoarse, F32, m), "trilinear %s on axis %d" % (mutate, axis))
        # another correct fp32 order passes
        assert not R.rejects(R.trilinear_adj_fused(c["dfine"], coarse, F32), ref64, ref32)
    N, H, W, scale = R.MAPS_PRECISE[0]
    g = R.gen(8)
    dr, dd = R.normal((N, H * scale, W * scale, 3), g), R.normal((N, H * scale, W * scale), g)
    er, ed = R.ints((N, H * scale, W * scale, 3), g, -4, 4), R.ints((N, H * scale, W * scale), g, -4, 4)
    judged(R.maps_adj(dr, dd, N, H, W, scale, F32, mutate), R.maps_adj(dr, dd, N, H, W, scale, F64), R.maps_adj(dr, dd, N, H, W, scale, F32),
           R.maps_adj(er, ed, N, H, W, scale, F64), R.maps_adj(er, ed, N, H, W, scale, F32, mutate), "maps " + mutate)


@pytest.mark.parametrize("wrong", ["batch_zero", "floor"])
def test_rules_reject_wrong_voxel_keys(wrong):
    N, D, H, W, C, B, grid = R.POOL[1]
    for gname in R.POOL_GRIDS:
        c, e = R.pool_case(N, D, H, W, C, B, grid, gname, False), R.pool_case(N, D, H, W, C, B, grid, gname, True)
        bad = R.voxel_keys(c["geom"], c["lo_dx"], c["ppb"], grid, **{wrong: True})
        bad_e = R.voxel_keys(e["geom"], e["lo_dx"], e["ppb"], grid, **{wrong: True})
        r64, r32 = R.lift_splat_adj(c["dout"], c["depth"], c["feat"], c["keys"], F64), R.lift_splat_adj(c["dout"], c["depth"], c["feat"], c["keys"], F32)
        w32 = R.lift_splat_adj(c["dout"], c["depth"], c["feat"], bad, F32)
        e64, we = R.lift_splat_adj(e["dout"], e["depth"], e["feat"], e["keys"], F64), R.lift_splat_adj(e["dout"], e["depth"], e["feat"], bad_e, F32)
        for k in range(2):
            judged(w32[k], r64[k], r32[k], e64[k], we[k], "lift-splat output %d with %s keys" % (k, wrong))
        # the gather is judged by bit equality alone
        assert not R.bits_equal(R.voxel_pool_adj(c["dout"], bad, F32), R.voxel_pool_adj(c["dout"], c["keys"], F64).to(F32))
        # ... and the adjoint identity against a forward with the right keys breaks as integers
        fwd = R.lift_splat_fwd(e["depth"], e["feat"], e["keys"], e["nvox"], F64)
        assert float((e["dout"].to(F64) * fwd).sum()) == float((e64[0] * e["depth"].to(F64)).sum()) == float((e64[1] * e["feat"].to(F64)).sum())
        assert float((e["dout"].to(F64) * fwd).sum()) != float((we[0].to(F64) * e["depth"].to(F64)).sum())


def test_rules_reject_an_ignored_camera_mask():
    prm, grid = R.camera_rig()
    g = R.gen(9)
    for Hf, Wf in R.IMG_MAPS:
        df, di = R.normal((grid.shape[1], 4), g), R.ints((grid.shape[1], 4), g, -4, 4)
        args = (prm, grid, 2, Hf, Wf)
        exact = (R.sample_img_adj(di, *args, F64), R.sample_img_adj(di, *args, F32, ignore_mask=1)) if (Hf, Wf) == (1, 1) else (None, None)
        judged(R.sample_img_adj(df, *args, F32, ignore_mask=1), R.sample_img_adj(df, *args, F64), R.sample_img_adj(df, *args, F32), *exact,
               what="image sampler %dx%d with camera 1's mask ignored" % (Hf, Wf))
    # the 1 x 1 map's N(0, 1) sums are held to rule 3 (weights exactly 1, one sum per camera and channel)
    idx = torch.cat([torch.where(m, cam, -1) for cam, (_, _, _, m, _) in enumerate(R.project(prm, grid, 2, F64))]).to(torch.int32)
    src, zero = torch.cat([df, df]), torch.zeros(2, 4)
    assert R.scatter_ratio(R.sample_img_adj(df, *args, F32, order=2).view(2, 4), zero, src, idx) <= 1.0
    assert R.scatter_ratio(R.sample_img_adj(df, *args, F32, ignore_mask=1).view(2, 4), zero, src, idx) > 1.0


def test_rules_reject_a_permuted_softmax_weight():
    for name in ("L4", "L3_c260", "peak"):
        c = R.mix_case(name)
        L = len(c["dims"])
        perm = list(range(1, L)) + [0]
        g64, d64 = R.mix_adj(c["levels"], c["wlogit"], c["dout"], F64)
        g32, d32 = R.mix_adj(c["levels"], c["wlogit"], c["dout"], F32)
        gw, dw = R.mix_adj(c["levels"], c["wlogit"], c["dout"], F32, perm=perm)
        for l in range(L):
            judged(gw[l], g64[l], g32[l], what="%s g[%d] with permuted weights" % (name, l))
        judged(dw, d64, d32, what=name + " dwlogit with permuted weights")


def test_scatter_rule_rejects_a_lost_and_a_doubled_row():
    n, C, rows, _, _ = R.SCATTER[0]
    c = R.scatter_case(n, C, rows, exact=False)
    ok = R.scatter_add(c["dst"], c["src"], c["idx"], F32)
    assert R.scatter_ratio(ok, c["dst"], c["src"], c["idx"]) <= 1.0
    r = int((c["idx"] >= 0).nonzero()[0])
    for sign in (-1.0, 1.0):
        bad = ok.clone()
        bad[int(c["idx"][r])] += sign * c["src"][r]
        assert R.scatter_ratio(bad, c["dst"], c["src"], c["idx"]) > 1.0
    # sequential fp32 additions in three seeded orders stay inside the bound
    for seed in (1, 2, 3):
        perm = torch.randperm(n, generator=R.gen(seed))
        out = c["dst"].clone()
        for i in perm.tolist():
            if int(c["idx"][i]) >= 0:
                out[int(c["idx"][i])] += c["src"][i]
        assert R.scatter_ratio(out, c["dst"], c["src"], c["idx"]) <= 1.0


# ----------------------------------------------------------------------------- 4. bad arguments are refused before any launch
def _refused(lib, rc, name, what):
    assert rc == -1, "%s: %s returned %d, not COOCC_EINVAL" % (name, what, rc)
    assert name.encode() in lib.coocc_last_error(), "%s: %s: the message %r does not name the entry" % (name, what, lib.coocc_last_error())


def test_pooling_and_scatter_entries_validate_before_launching():
    lib = _lib.load()
    lo = _lib.host_f32([0, 0, 0, 1, 1, 1])

    def scatter(src=ONE, ss=8, idx=ONE, n=10, C=8, dst=ONE, ds=8):
        return lib.coocc_scatter_add_rows(src, ss, idx, n, C, dst, ds, None)
    for what, kw in [("a source stride below C", dict(ss=7)), ("a destination stride below C", dict(ds=4)), ("C = 0", dict(C=0, ss=0, ds=0)),
                     ("n < 0", dict(n=-1)), ("a null source", dict(src=None)), ("a null index", dict(idx=None)), ("a null destination", dict(dst=None))]:
        _refused(lib, scatter(**kw), "scatter_add_rows", what)

    def pool(dout=ONE, stride=8, npts=40, ppb=20, C=8, B=2, grid=(2, 2, 2), dx=ONE):
        return lib.coocc_voxel_pool_bwd(dout, stride, ONE, npts, ppb, C, lo, B, *grid, dx, None)

    def lift(stride=8, N=2, D=5, H=2, W=2, C=8, ppb=20, B=2, grid=(2, 2, 2), dd=ONE):
        return lib.coocc_lift_splat_bwd(ONE, stride, ONE, ONE, ONE, N, D, H, W, C, ppb, lo, B, *grid, dd, ONE, None)
    for what, kw in [("dout_stride < C", dict(stride=4)), ("B = 0", dict(B=0)), ("an empty grid", dict(grid=(2, 0, 2))),
                     ("a negative grid", dict(grid=(2, 2, -1))), ("more points than B * pts_per_batch", dict(ppb=19)),
                     ("one batch too few", dict(B=1)), ("C % 4 != 0", dict(C=6)), ("pts_per_batch = 0", dict(ppb=0))]:
        _refused(lib, pool(**kw), "voxel_pool_bwd", what)
        _refused(lib, lift(**kw), "lift_splat_bwd", what)
    _refused(lib, pool(npts=0), "voxel_pool_bwd", "no points")
    _refused(lib, pool(dx=None), "voxel_pool_bwd", "a null dx")
    _refused(lib, lift(D=0), "lift_splat_bwd", "D = 0")
    _refused(lib, lift(dd=None), "lift_splat_bwd", "a null d_depth")


def test_resampling_and_mix_entries_validate_before_launching():
    lib = _lib.load()

    def tri(dfine=ONE, B=1, C=4, coarse=(2, 2, 2), fine=(4, 4, 4)):
        return lib.coocc_upsample_trilinear_bwd(dfine, ONE, B, C, *coarse, *fine, 0, None)
    for what, kw in [("an empty coarse axis", dict(coarse=(2, 0, 2), fine=(4, 0, 4))), ("a negative coarse axis", dict(coarse=(-1, 2, 2), fine=(-1, 4, 4))),
                     ("B = 0", dict(B=0)), ("C = 0", dict(C=0)), ("C % 4 != 0", dict(C=6)), ("a factor above 8", dict(fine=(17, 4, 4))),
                     ("downsampling", dict(fine=(1, 4, 4))), ("a null dfine", dict(dfine=None))]:
        _refused(lib, tri(**kw), "upsample_trilinear_bwd", what)

    def maps(dr=ONE, dd=ONE, N=1, H=2, W=2, scale=2, out=ONE):
        return lib.coocc_upsample_maps_bwd(dr, dd, N, H, W, scale, out, None)
    for what, kw in [("both gradients null", dict(dr=None, dd=None)), ("N = 0", dict(N=0)), ("H = 0", dict(H=0)), ("W < 0", dict(W=-2)),
                     ("scale = 0", dict(scale=0)), ("a null dmaps", dict(out=None))]:
        _refused(lib, maps(**kw), "upsample_maps_bwd", what)

    def mix(levels=(16, 16), grads=(16, 16), dims=(4, 4, 2, 2, 2, 1), L=2, B=1, C=8, dout=ONE):
        lv = (ctypes.c_void_p * len(levels))(*levels)
        gr = (ctypes.c_void_p * len(grads))(*grads)
        return lib.coocc_occhead_mix_bwd(lv, _lib.host_i32(dims), L, ONE, dout, gr, ONE, B, C, None)
    for what, kw in [("a null level pointer", dict(levels=(16, None))), ("a null gradient pointer", dict(grads=(None, 16))),
                     ("an empty level", dict(dims=(4, 4, 2, 2, 0, 1))), ("a negative level-0 axis", dict(dims=(4, -4, 2, 2, 2, 1))),
                     ("B = 0", dict(B=0)), ("C = 0", dict(C=0)), ("C % 4 != 0", dict(C=6)), ("L = 0", dict(L=0)),
                     ("L = 5", dict(L=5, levels=(16,) * 5, grads=(16,) * 5, dims=(2,) * 15)), ("a null dout", dict(dout=None))]:
        _refused(lib, mix(**kw), "occhead_mix_bwd", what)


def test_sampler_entries_validate_before_launching():
    lib = _lib.load()

    def vox(stride=8, C=8, dims=(3, 3, 3), nfine=5, final=(6, 6, 6), dvol=ONE):
        return lib.coocc_fine_sample_voxel_bwd(ONE, stride, C, *dims, ONE, nfine, _lib.host_i32(final), dvol, None)
    for what, kw in [("dfeat_stride < C", dict(stride=7)), ("an empty volume", dict(dims=(3, 0, 3))), ("a negative volume axis", dict(dims=(3, 3, -3))),
                     ("final_size 1 on x", dict(final=(1, 6, 6))), ("final_size 0 on z", dict(final=(6, 6, 0))), ("C = 0", dict(C=0, stride=0)),
                     ("nfine < 0", dict(nfine=-1)), ("a null dvol", dict(dvol=None))]:
        _refused(lib, vox(**kw), "fine_sample_voxel_bwd", what)

    def img(stride=8, ncam=2, Ci=8, Hf=3, Wf=4, nfine=5, dimg=ONE):
        return lib.coocc_fine_sample_img_bwd(ONE, stride, ncam, Ci, Hf, Wf, ONE, ONE, nfine, dimg, None)
    for what, kw in [("dfeat_stride < Ci", dict(stride=6)), ("Hf = 0", dict(Hf=0)), ("Wf < 0", dict(Wf=-1)), ("no camera", dict(ncam=0)),
                     ("Ci = 0", dict(Ci=0, stride=0)), ("nfine < 0", dict(nfine=-1)), ("a null dimg", dict(dimg=None))]:
        _refused(lib, img(**kw), "fine_sample_img_bwd", what)
