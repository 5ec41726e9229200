"""The captured dense stage (co_occ_amd.graph.DenseGraph: one hipGraphLaunch per sample, every data-dependent count read on
the device) against the eager path on the same samples, bit for bit."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _eager(model, s, dev):
    import bench
    with torch.no_grad():
        img = bench.pool(model, s)
        sr = model.search(img, s["pts"])
        out = model.forward_hot_path(img, s["pts"], s["gemo"], s["img_feats"], s["transform"], render=True, search=sr)
    torch.cuda.synchronize()
    return {k: out[k].clone() for k in ("pred_c", "pred_f", "rgbs", "depths")}, sr.counts


def test_dense_graph_replay_equals_eager(dev):
    import bench
    from co_occ_amd import graph as cg
    bench.CFGNAME[0] = "r50"
    model, _ = bench.build_model("r50", dev)
    a = bench.make_inputs("r50", 1234, dev, model)
    b = bench.make_inputs("r50", 99, dev, model)
    # the graph binds the per-sample tensors it reads besides the slot: give sample b the rig of sample a
    for k in ("gemo", "img_feats", "transform", "cams"):
        b[k] = a[k]
    want_a, counts_a = _eager(model, a, dev)
    want_b, counts_b = _eager(model, b, dev)
    assert counts_a != counts_b
    X, Y, Z = a["pts"].shape[2:]
    slot = cg.make_slot(model, (X, Y, Z), dev)
    stream = torch.cuda.Stream(device=dev)
    cur = torch.cuda.current_stream(dev)

    def search(s):
        with torch.no_grad():
            sr = cg.search_into_slot(model, slot, s["depth"], s["ctx"], s["cams"], s["pts"])
        sr.done_main.wait(stream)
        sr.done_side.wait(stream)
        return sr

    sr = search(a)
    g = cg.DenseGraph(model, slot, a, stream).capture()
    assert g.fits(sr.counts)
    for s, want, counts in ((a, want_a, counts_a), (b, want_b, counts_b), (a, want_a, counts_a)):
        cur.wait_stream(stream)          # the slot is rewritten only after the previous replay has finished with it
        sr = search(s)
        assert sr.counts == counts and g.fits(sr.counts)
        with torch.cuda.stream(stream):
            out = g.replay()
        stream.synchronize()
        n = int(out["fine_count"].item())
        assert n > 0
        for k in ("pred_c", "pred_f", "rgbs", "depths"):
            assert torch.equal(out[k], want[k]), "%s differs between the graph replay and the eager path" % k


def test_native_search_equals_python_search(dev):
    """coocc_fuser_search (the whole index-search stage issued from C++, csrc/search.hip) against BiFuser_N.search: voxel lists,
    counts, neighbour ordinals and row tables bit for bit, concat rows included."""
    import bench
    from co_occ_amd import graph as cg
    bench.CFGNAME[0] = "r50"
    model, _ = bench.build_model("r50", dev)
    s = bench.make_inputs("r50", 4321, dev, model)
    X, Y, Z = s["pts"].shape[2:]
    f = model.occ_fuser
    with torch.no_grad():
        a, b = cg.make_slot(model, (X, Y, Z), dev), cg.make_slot(model, (X, Y, Z), dev)
        for slot in (a, b):
            model.img_view_transformer.lift_splat(s["depth"], s["ctx"], cams=s["cams"], out=slot.img_rows())
        sa = f.search(a.img_rows().as_ncdhw(), s["pts"], slot=a)
        sb = f.search_native(s["pts"], b)
    torch.cuda.synchronize()
    assert sa.counts == sb.counts and min(sa.counts) > 2048
    assert torch.equal(sa.lin_img, sb.lin_img) and torch.equal(sa.lin_pts, sb.lin_pts)
    assert torch.equal(sa.near_img, sb.near_img) and torch.equal(sa.near_pts, sb.near_pts)
    assert torch.equal(sa.rows, sb.rows) and torch.equal(sa.rows_p, sb.rows_p)
    C = f.in_channels
    assert torch.equal(a.cat4[:, :2 * C], b.cat4[:, :2 * C])
    assert torch.equal(a.counts, b.counts)


def test_stream_scratch_holds_every_per_stream_buffer(dev):
    """The contract a captured graph relies on (core.stream_buffer / core.stream_scratch): every per-stream device buffer of the
    package is listed for its stream; a buffer that has to grow is REPLACED, the new one is listed and a list taken earlier still
    holds the old one; a zeroed kind comes back as fresh zeros.  Allocates and compares, launches only the FPS / voxelisation
    calls whose workspaces are taken inside them (torch hands stream handles out of a pool, so nothing here assumes the
    stream starts out empty)."""
    from co_occ_amd import _lib, autograd, core, fuser, lidar, ops
    from oracle import cases
    lib = _lib.load()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))

    def listed(t, tensors=None):
        return any(t is u for u in (core.stream_scratch(dev, s) if tensors is None else tensors))

    with torch.cuda.stream(s), torch.no_grad():
        got = dict(workspace=core.workspace(dev), scratch=core.scratch(dev, "registry_test", 1000), tile_sem=core.tile_sem(dev),
                   wino=core._wino_buffer(dev, "V", 1000), bf16=core.stream_buffer(dev, "bf16", 1000, torch.bfloat16),
                   amax=autograd._amax_word(dev), pool=ops._pool_workspace(dev, 5000, 300))
        assert got["workspace"].numel() == 64 << 20 and got["tile_sem"].numel() == 4096 and got["amax"].numel() == 2048
        assert got["tile_sem"].dtype == got["amax"].dtype == torch.int32 and got["bf16"].dtype == torch.bfloat16
        assert got["pool"].numel() >= int(lib.coocc_voxel_pool_ws(5000, 300)) and got["pool"].dtype == torch.uint8
        # FPS and voxelisation take their workspaces inside the call: run each once, then ask the registry what it holds
        X, Y, Z = 7, 5, 3
        fuser._fps_voxels_on_current(torch.arange(X * Y * Z, dtype=torch.int32, device=dev), (X, Y, Z), 20)
        got["fps"] = core.stream_buffer(dev, "fps", 0, torch.uint8)
        assert got["fps"].numel() >= int(lib.coocc_fps_voxels_ws(X, Y, Z)) > 0
        c = cases.LIDAR_CASE
        pts = torch.from_numpy(cases.lidar_points(c)).to(dev)
        vox = lidar.Voxelization(c["voxel_size"], c["point_cloud_range"], c["max_points"], (c["max_voxels"],) * 2).eval()
        vox(pts)
        got["voxelize"] = core.stream_buffer(dev, "voxelize", 0, torch.uint8)
        assert got["voxelize"].numel() >= int(lib.coocc_voxelize_ws(pts.shape[0])) > 0
        assert not hasattr(vox, "_ws")                                          # the module itself holds no workspace
        for name, t in got.items():
            assert listed(t), "%s is not in stream_scratch" % name              # (i)
        # the same request again is the same tensor; another stream has its own
        assert core.scratch(dev, "registry_test", 1000) is got["scratch"] and core.workspace(dev) is got["workspace"]
    mine = core.scratch(dev, "registry_test", 1000)                              # the current stream is not s
    assert mine is not got["scratch"] and listed(mine, core.stream_scratch(dev, torch.cuda.current_stream(dev))) and not listed(mine)
    with torch.cuda.stream(s):
        before = core.stream_scratch(dev, s)
        big = core.scratch(dev, "registry_test", got["scratch"].numel() + 1)     # (ii)
        assert big is not got["scratch"] and big.numel() > got["scratch"].numel()
        assert listed(big) and not listed(got["scratch"]) and listed(got["scratch"], before) and not listed(big, before)
        z = core._wino_buffer(dev, "registry_test_z", 64)                        # (iii)
        assert int(z.count_nonzero()) == 0
        z.fill_(1.0)
        z2 = core._wino_buffer(dev, "registry_test_z", 4 * z.numel())
        assert z2 is not z and int(z2.count_nonzero()) == 0 and int(z.count_nonzero()) == z.numel()
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
