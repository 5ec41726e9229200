"""``coocc_fine_vox`` (csrc/fine_vox.hip): the voxel-only fine branch of OccHead at cascade ratio 2 in one launch with the foreground
count on the device -- alone, inside the head (eager static form == graph replay), through ``apis.pipelined_test`` of a LiDAR-only
model with ``sample_from_voxel=True``, and beside split-f16 GEMMs of another stream.

The judge is ``util.assert_precise`` against a float64 restatement of the reference's chain (occ_head.py:212-220, 237): normalised
coordinates -> ``F.grid_sample`` of the 128-channel features -> Linear 128 -> 64 + bias -> GroupNorm(16) -> ReLU -> Linear 64 -> ncls.
Its anchors are restated here too: the same chain in fp32 on the CPU, and -- where Q came from the engine's own GEMM -- the chain
with the first Linear applied before the interpolation on operands split the engine's way.  The kernel applies that Linear before
the interpolation (they commute), so it is fp32-accurate against the chain, not bit-equal to the eager three-launch form."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import util
from co_occ_amd import _lib, core, graph
from co_occ_amd._lib import call, host_i32, ptr

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0


# ------------------------------------------------------------------ the restated chain
def fine_coords(lin, grid):
    """coordinate_transform.py:3-18 at ratio 2 for the coarse voxels ``lin`` (row = (x Y + y) Z + z): int64 [3, 8 n], point
    o n + i = child o = (a 2 + b) 2 + c of voxel i."""
    X, Y, Z = grid
    lin = lin.long().cpu()
    coarse = torch.stack([lin // (Y * Z), (lin // Z) % Y, lin % Z])                         # [3, n]
    value = torch.stack(torch.meshgrid([torch.arange(2)] * 3, indexing="ij"), dim=3).reshape(-1, 3)
    return (coarse[None] * 2 + value[:, :, None]).permute(1, 0, 2).reshape(3, -1)


def sample(rows, grid, xyz, final, dtype):
    """occ_head.py:213-220: rows [V, C] on the coarse grid -> [8 n, C] at the fine coordinates ``xyz``."""
    X, Y, Z = grid
    vol = util._f64(rows).to(dtype).view(1, X, Y, Z, -1).permute(0, 4, 1, 2, 3)
    g = xyz.to(dtype)
    g = torch.stack([(g[k] / (final[k] - 1) - 0.5) * 2 for k in range(3)])
    g = g[None, None, None].permute(0, 4, 1, 2, 3)
    out = F.grid_sample(vol.permute(0, 1, 4, 3, 2), g, mode="bilinear", padding_mode="zeros", align_corners=False)
    return out[0, :, :, 0, 0].permute(1, 0)


def tail(y, prm, dtype):
    """fine_mlp[1:] on the pre-activation ``y`` [n, 64] (bias included): GroupNorm(16, 64), ReLU, Linear 64 -> ncls."""
    t = lambda k: util._f64(prm[k]).to(dtype)
    v = y.reshape(y.shape[0], 16, -1)
    m = v.mean(-1, keepdim=True)
    var = (v - m).pow(2).mean(-1, keepdim=True)
    h = torch.relu(((v - m) / torch.sqrt(var + prm["eps"])).reshape(y.shape) * t("gamma") + t("beta"))
    return h @ t("w3").t() + t("b3")


def chain(x, grid, xyz, final, prm, dtype):
    """The reference's order: sample the 128-channel rows, then fine_mlp."""
    t = lambda k: util._f64(prm[k]).to(dtype)
    return tail(sample(x, grid, xyz, final, dtype) @ t("w0").t() + t("b0"), prm, dtype)


def chain_split(x, grid, xyz, final, prm):
    """The engine's order with its operand split: Q = W0 x by ``util.split_mm`` rounded to fp32, then the rest in float64, the
    result rounded to fp32."""
    q = util.split_mm(util._f64(x).float(), util._f64(prm["w0"]).float().t()).float()
    return tail(sample(q, grid, xyz, final, torch.float64) + util._f64(prm["b0"]), prm, torch.float64).float()


def params_of(head):
    l0, g0, l3 = head.fine_mlp[0], head.fine_mlp[1], head.fine_mlp[3]
    return dict(w0=l0.weight.detach(), b0=l0.bias.detach(), gamma=g0.weight.detach(), beta=g0.bias.detach(), eps=float(g0.eps),
                w3=l3.weight.detach(), b3=l3.bias.detach())


def random_params(ncls, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(w0=r(64, 128) * 0.125, b0=r(64) * 0.1, gamma=torch.rand(64, generator=g) + 0.5, beta=r(64) * 0.1, eps=1e-5,
                w3=r(ncls, 64) * 0.18, b3=r(ncls) * 0.1)


def launch(dev, q, grid, lin, n_cap, cnt, prm, ncls, cap_rows):
    """One ``coocc_fine_vox`` call into sentinel-filled, capacity-sized outputs."""
    X, Y, Z = grid
    xyz = torch.full((3 * 8 * cap_rows,), int(SENTINEL), device=dev, dtype=torch.int64)
    out = torch.full((8 * cap_rows, ncls), SENTINEL, device=dev)
    d = lambda k: ptr(prm[k].to(dev).contiguous())
    call("coocc_fine_vox", ptr(q), X, Y, Z, ptr(lin), int(n_cap), ptr(cnt) if cnt is not None else None, host_i32([2 * X, 2 * Y, 2 * Z]),
         d("b0"), d("gamma"), d("beta"), float(prm["eps"]), d("w3"), d("b3"), ncls, ptr(xyz), ptr(out))
    torch.cuda.synchronize()
    return xyz.cpu(), out.cpu()


GRID = (8, 8, 2)
_ALONE = {}


def _alone_inputs():
    """The coarse rows, Q and one foreground permutation, shared by every case (made once, never written)."""
    if not _ALONE:
        X, Y, Z = GRID
        g = torch.Generator().manual_seed(77)
        x = torch.randn(X * Y * Z, 128, generator=g)
        row = lambda a, b, c: (a * Y + b) * Z + c
        # the two corners and a voxel on each face first, then every other voxel in a seeded order: any count >= 8 holds them
        first = [row(0, 0, 0), row(7, 7, 1), row(0, 3, 1), row(7, 4, 0), row(2, 0, 0), row(5, 7, 1), row(3, 3, 0), row(4, 2, 1)]
        rest = [v for v in torch.randperm(X * Y * Z, generator=g).tolist() if v not in first]
        _ALONE.update(x=x, order=torch.tensor(first + rest, dtype=torch.int32))
    return _ALONE


@pytest.mark.parametrize("ncls", [17, 32])
@pytest.mark.parametrize("count", [0, 1, 37, 128])
def test_kernel_alone_against_the_float64_chain(dev, count, ncls):
    S = _alone_inputs()
    X, Y, Z = GRID
    V, final = X * Y * Z, (2 * X, 2 * Y, 2 * Z)
    prm = random_params(ncls, 5)
    # Q as the head makes it, here with the best rounding there is: the float64 product rounded to fp32 once
    q = (S["x"].double() @ prm["w0"].double().t()).float().to(dev)
    lin_host = S["order"][:count] if count != 1 else S["order"][1:2]          # count 1: the far corner (7, 7, 1)
    lin = torch.zeros(V, dtype=torch.int32)
    lin[:count] = lin_host
    lin = lin.to(dev)
    cnt = torch.tensor([count], dtype=torch.int32, device=dev)
    xyz_d, out_d = launch(dev, q, GRID, lin, V, cnt, prm, ncls, V)             # capacity V, count on the device
    nf = 8 * count
    assert bool((out_d[nf:] == SENTINEL).all()) and bool((xyz_d[3 * nf:] == int(SENTINEL)).all()), "rows past the count were written"
    if count == 0:
        return
    xyz_h, out_h = launch(dev, q, GRID, lin, count, None, prm, ncls, V)         # the host-count form: n_dev null
    assert torch.equal(xyz_d, xyz_h) and torch.equal(out_d.view(torch.int32), out_h.view(torch.int32)), "n_dev and host-count forms differ"
    want = fine_coords(lin_host, GRID)
    assert torch.equal(xyz_d[:3 * nf].view(3, nf), want)
    ref64 = chain(S["x"], GRID, want, final, prm, torch.float64)
    ref32 = chain(S["x"], GRID, want, final, prm, torch.float32)
    util.assert_precise(out_d[:nf], ref64, ref32, what="fine_vox alone n=%d ncls=%d" % (count, ncls))


def test_kernel_refuses_what_it_does_not_take(dev):
    prm = random_params(17, 5)
    q = torch.zeros(128, 64, device=dev)
    lin = torch.zeros(128, dtype=torch.int32, device=dev)
    xyz, out = torch.zeros(3 * 8 * 128, dtype=torch.int64, device=dev), torch.zeros(8 * 128, 40, device=dev)
    d = lambda k: ptr(prm[k].to(dev).contiguous())
    args = lambda final, ncls, n: (ptr(q), 8, 8, 2, ptr(lin), n, None, host_i32(final), d("b0"), d("gamma"), d("beta"), 1e-5,
                                   ptr(torch.zeros(40, 64, device=dev)), ptr(torch.zeros(40, device=dev)), ncls, ptr(xyz), ptr(out))
    for final, ncls, n in (((32, 32, 8), 17, 4), ((16, 16, 4), 33, 4), ((16, 16, 4), 17, 129)):
        with pytest.raises(_lib.CooccArgError, match="fine_vox"):
            call("coocc_fine_vox", *args(final, ncls, n))


# ------------------------------------------------------------------ the head and the models
def lidar_model(dev, final, ratio=2):
    from test_gpu_single_modality_serving import _build
    from co_occ_amd import synth
    cfg = synth.model_cfg_lidar()
    cfg.update(external_encoders=True)
    cfg["pts_bbox_head"].update(final_occ_size=list(final), sample_from_voxel=True, cascade_ratio=ratio)
    return _build(cfg, dev, 9)


def judge_fine(head, grid, pred_c, xyz, logits, what):
    """Fine outputs (exact size) of one sample against the restated chain on the head's own coarse features of that sample."""
    X, Y, Z = grid
    rows = head.last_out_voxel_feats
    x = rows.t[:, rows.coff:rows.coff + rows.C].detach().cpu()
    lin = torch.nonzero(pred_c[0].argmax(0).reshape(-1) != head.empty_idx).flatten().cpu()
    want = fine_coords(lin, grid)
    assert lin.numel() > 0 and torch.equal(xyz.cpu().reshape(3, -1), want), "%s: fine coordinates" % what
    final, prm = tuple(int(v) for v in head.final_occ_size), params_of(head)
    util.assert_precise(logits.cpu(), chain(x, grid, want, final, prm, torch.float64), chain(x, grid, want, final, prm, torch.float32),
                        chain_split(x, grid, want, final, prm), what=what)
    return want


def test_head_static_form_equals_its_graph_replay_and_both_forms_meet_the_chain(dev):
    from co_occ_amd import synth
    grid = (10, 10, 4)
    model = lidar_model(dev, (20, 20, 8))
    head = model.pts_bbox_head
    pts = synth.voxel_inputs(grid, C=128, seed=91, p_pts=0.4)[1].to(dev)
    slot = graph.make_slot(model, grid, dev, example=dict(pts=pts))
    assert isinstance(slot, graph.VoxelSlot)
    stream = torch.cuda.Stream(device=dev)
    dg = graph.DenseGraph(model, slot, {}, stream, render=False)
    with torch.no_grad():
        eager = model.forward_hot_path(None, pts)                      # the eager ``_fine``: samples first, Linear afterwards
        judge_fine(head, grid, eager["pred_c"], eager["output_coords_fine"][0], eager["output_voxels_fine"][0], "eager _fine")
        with torch.cuda.stream(stream):
            graph.fill_volume(slot, pts)
            with util.kernels() as names:
                issued = dg._run()                                     # decode(static=True), launch by launch
            n = int(issued["fine_count"].item())
            keep = {k: issued[k].clone() for k in ("pred_c", "pred_f")}
            keep["fine"], keep["xyz"] = issued["output_voxels_fine"][0].clone(), issued["output_coords_fine"][0].clone()
        assert names.get("k_fine_vox", 0) >= 1, names
        out = dg.capture().replay()
        stream.synchronize()
    assert n > 0 and torch.equal(keep["pred_c"], eager["pred_c"])
    for k, v in (("pred_c", out["pred_c"]), ("pred_f", out["pred_f"]), ("fine", out["output_voxels_fine"][0][:8 * n]),
                 ("xyz", out["output_coords_fine"][0][:24 * n])):
        ref = keep[k] if k in ("pred_c", "pred_f") else keep[k][:v.shape[0]]
        assert torch.equal(ref.view(torch.int32) if ref.is_floating_point() else ref, v.view(torch.int32) if v.is_floating_point() else v), k
    want = judge_fine(head, grid, out["pred_c"], out["output_coords_fine"][0][:24 * n].view(3, -1), out["output_voxels_fine"][0][:8 * n],
                      "static _fine (coocc_fine_vox)")
    # pred_f: the fine logits at their voxels, the empty value elsewhere
    pf = out["pred_f"][0].cpu()
    assert torch.equal(pf[:, want[0], want[1], want[2]].t(), out["output_voxels_fine"][0][:8 * n].cpu())
    mask = torch.ones(pf.shape[1:], dtype=torch.bool)
    mask[want[0], want[1], want[2]] = False
    assert bool((pf[:, mask] == float(head.empty_idx)).all())
    # a ratio-4 voxel-only head has no device-count kernel: refused before anything is launched
    head.cascade_ratio, head.final_occ_size = 4, [40, 40, 16]
    with torch.no_grad(), torch.cuda.stream(stream), pytest.raises(_lib.CooccArgError, match="static fine branch"):
        dg._run()
    stream.synchronize()


def test_lidar_only_with_the_voxel_cascade_through_pipelined_test(dev):
    from co_occ_amd import apis, synth
    grid = (50, 50, 4)
    model = lidar_model(dev, (100, 100, 8))
    head = model.pts_bbox_head
    vols = [synth.voxel_inputs(grid, C=128, seed=70 + i, p_pts=0.3)[1].to(dev) for i in range(3)]
    data = [dict(precomputed=dict(pts_voxel_feats=v)) for v in vols]
    ref = []
    with torch.no_grad():
        model.graph_simple_test = False
        for d in data:
            r = model.simple_test(**d)
            rows = head.last_out_voxel_feats
            ref.append((r["pred_c"].clone(), rows.t[:, rows.coff:rows.coff + rows.C].detach().cpu()))
        model.graph_simple_test = True
    stats, n = {}, 0
    final, prm = (100, 100, 8), params_of(head)
    for i, (d, res) in enumerate(apis.pipelined_test(model, iter(data), slots=2, dense_streams=1, stats=stats)):
        pred_c, x = ref[i]
        assert torch.equal(res["pred_c"], pred_c), "sample %d: pred_c" % i
        lin = torch.nonzero(pred_c[0].argmax(0).reshape(-1) != head.empty_idx).flatten().cpu()
        want = fine_coords(lin, grid)
        assert torch.equal(res["output_coords_fine"][0].cpu(), want)
        got = res["pred_f"][0].cpu()[:, want[0], want[1], want[2]].t()
        util.assert_precise(got, chain(x, grid, want, final, prm, torch.float64), chain(x, grid, want, final, prm, torch.float32),
                            chain_split(x, grid, want, final, prm), what="pipelined pred_f sample %d" % i)
        n += 1
    assert n == 3 and stats["fallbacks"] == 0 and stats["eager_samples"] == 0, stats


@pytest.mark.parametrize("corunner", ["h2p", "wino"])
def test_fine_vox_is_bit_stable_beside_split_f16_gemms(dev, corunner):
    import test_gpu_corunner as CR
    gb = torch.Generator().manual_seed(11)
    xb = core.to_rows(torch.randn(1, 128, 100, 100, 8, generator=gb).to(dev))
    S = dict(xb=xb, pc1=core.PackedConv((torch.randn(128, 128, 1, 1, 1, generator=gb) * 0.05).to(dev), ksize=1, pad=0),
             pc3=core.PackedConv((torch.randn(128, 128, 3, 3, 3, generator=gb) * 0.02).to(dev), ksize=3, pad=1),
             s0=torch.cuda.Stream(device=dev), s1=torch.cuda.Stream(device=dev))
    with torch.no_grad():
        core.conv_rows(xb, S["pc1"], relu=False)
        core.conv_rows(xb, S["pc3"], relu=False)
    grid = (100, 100, 8)
    V, ncls = 80000, 17
    prm = {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in random_params(ncls, 6).items()}
    q = torch.randn(V, 64, generator=gb).to(dev)
    lin = torch.sort(torch.randperm(V, generator=gb)[:12000])[0].int().to(dev)          # 15 % foreground
    cnt = torch.tensor([lin.numel()], dtype=torch.int32, device=dev)

    def fn():
        xyz = torch.empty(3 * 8 * lin.numel(), device=dev, dtype=torch.int64)
        out = torch.empty(8 * lin.numel(), ncls, device=dev)
        call("coocc_fine_vox", ptr(q), 100, 100, 8, ptr(lin), lin.numel(), ptr(cnt), host_i32([200, 200, 16]), ptr(prm["b0"]),
             ptr(prm["gamma"]), ptr(prm["beta"]), 1e-5, ptr(prm["w3"]), ptr(prm["b3"]), ncls, ptr(xyz), ptr(out))
        return [xyz, out]
    torch.cuda.synchronize()
    ref, got = CR._run_beside(S, fn, corunner=corunner)
    bad = CR._count_differing(ref, got)
    assert bad == 0, "coocc_fine_vox beside %s: %d of %d calls differ from the run alone" % (corunner, bad, len(got))
