"""DepthNet on the HIP engine (co_occ_amd/depth_net.py, csrc/depthnet.hip) against float64.

Single kernels are judged at their own precision (``util.assert_precise``: the fp32 CPU evaluation of the same operation and the
split-f16 emulation as anchors); module-level outputs by ``util.assert_close`` (TOL), under the condition that the fp32 restatement
(tests/ref_depth_net.py) is itself within TOL / 4 of float64 on that input.  The deformable convolution takes its offsets as an
input tensor in the kernel tests, so no offset error is amplified."""
import pytest
import torch
import torch.nn.functional as F

import co_occ_amd as pkg
import ref_depth_net as R
from co_occ_amd import core, depth_net as dn, synth
from co_occ_amd.core import Rows
from util import TOL, assert_close, assert_precise, gemm_refs, rel_err, split_mm

pytestmark = pytest.mark.gpu


def rows_of(x):
    """[BN,C,H,W] -> channels-last rows [BN*H*W, C]."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def as_rows(x, dev):
    BN, C, H, W = x.shape
    return Rows(rows_of(x).float().to(dev), BN, H, W, 1, C)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------ 1. dilated convolutions over the neighbour table
@pytest.mark.parametrize("H,W", [(5, 7), (16, 44), (19, 37)])
def test_dilated_table_conv(dev, H, W):
    C, BN = 64, 2
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(BN, C, H, W, generator=g) * torch.tensor([1.0, 3.0]).view(2, 1, 1, 1)        # the cameras differ
    xr = as_rows(x, dev)
    for d in dn.ASPP_DILATIONS:
        w = torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5)
        table = dn.neighbour_table(BN, H, W, d, dev)
        tb = table.cpu()
        m = torch.arange(BN * H * W)
        assert torch.equal(tb[4].long(), m)                                                     # the centre tap is the pixel itself
        live = tb >= 0
        assert bool((tb[live].long() // (H * W) == m.expand(9, -1)[live] // (H * W)).all())     # never another camera's row
        for t in range(9):
            i, j = t // 3 - 1, t % 3 - 1
            dead = (i != 0 and d >= H) or (j != 0 and d >= W)
            assert bool(live[t].any()) != dead, "tap %d of dilation %d on %dx%d" % (t, d, H, W)
        assert dn.live_taps(H, W, d) == tuple(t for t in range(9) if live[t].any())
        all_dead = d >= max(H, W)            # 5x7 at dilations 12 and 18 (at 6 the horizontal taps still join columns 0 and 6)
        if all_dead:
            assert int(live.sum()) == BN * H * W                     # every non-centre tap is dead: the centre-tap 1x1
        if (H, W) == (16, 44) and d == 18:
            assert not live[[0, 1, 2, 6, 7, 8]].any() and live[3].any() and live[5].any()
        out = dn.dilated_conv_rows(xr, dn.table_pack(w.to(dev)), d, table=table, relu=False)
        xp = F.pad(x.double(), (d, d, d, d))
        pairs = [(rows_of(xp[:, :, i * d:i * d + H, j * d:j * d + W]), w[:, :, i, j].double().t()) for i in range(3) for j in range(3)]
        r64, r32, rs = gemm_refs(pairs)
        want = rows_of(F.conv2d(x.double(), w.double(), dilation=d, padding=d))
        assert float((r64 - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert_precise(out.cpu(), want, r32, rs, what="dilated %dx%d d=%d" % (H, W, d))
        if all_dead:
            c64, c32, cs = gemm_refs([pairs[4]])
            assert_precise(out.cpu(), c64, c32, cs, what="dilated %dx%d d=%d vs the centre-tap 1x1" % (H, W, d))
        assert (H, W) != (5, 7) or all_dead == (d > 6)
    core.check_h2_overflow()


# ------------------------------------------------------------------ 2. the deformable convolution, offsets given
def _dcn_inputs(H, W, seed):
    C, BN = 128, 2
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(BN, C, H, W, generator=g)
    w = torch.randn(C, C // 4, 3, 3, generator=g) / (3 * (C // 4) ** 0.5)
    w = w * torch.tensor([1.0, 2.0, 0.5, 4.0]).repeat_interleave(C // 4).view(C, 1, 1, 1)           # the groups differ visibly
    return x, w, g


def _hand_placed(H, W):
    """Positions exactly at -1, H-1 and H and just inside -1 (rows: taps 0-3; columns: taps 4-7), every one exact in fp32."""
    off = torch.zeros(2, 18, H, W)
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    eps = 2.0 ** -10
    off[:, 0] = -1 - (ys - 1)               # tap 0 (i = 0): row position -1     -> 0
    off[:, 2] = (H - 1) - (ys - 1)          # tap 1 (i = 0): row position H - 1  -> the last row, its lower neighbour outside
    off[:, 4] = H - (ys - 1)                # tap 2 (i = 0): row position H      -> 0
    off[:, 6] = (-1 + eps) - ys             # tap 3 (i = 1): row position -1 + eps: eps of row 0
    off[:, 9] = -1 - xs                     # tap 4 (j = 1): column position -1  -> 0
    off[:, 11] = (W - 1) - (xs + 1)         # tap 5 (j = 2): column position W - 1
    off[:, 13] = W - (xs - 1)               # tap 6 (j = 0): column position W   -> 0
    off[:, 15] = (-1 + eps) - xs            # tap 7 (j = 1): column position -1 + eps
    return off


def _judge_dcn(dev, x, w, off, what, zero_taps=None):
    """Sampler columns and the grouped GEMM's output against float64; returns (columns, output) of the device."""
    BN, C, H, W = x.shape
    xr = as_rows(x, dev)
    offr = rows_of(off).float().to(dev)
    M = BN * H * W
    c64 = R.cols_as_rows(R.dcn_cols_gather(x.double(), off.double()))
    c32 = R.cols_as_rows(R.dcn_cols_gather(x.float(), off.float()))
    cols = dn.dcn_columns(xr, offr, 0, M).cpu()
    assert_precise(cols, c64, c32, what="dcn columns " + what)
    py, px = R.tap_positions(off.double())
    outside = rows_of((py <= -1) | (py >= H) | (px <= -1) | (px >= W))                            # [M, 9]
    cg = C // 4
    cv = cols.view(4, M, 9, cg)
    assert float(cv.permute(1, 2, 0, 3)[outside].abs().max() if outside.any() else 0.0) == 0.0, "a tap outside the map is exactly 0"
    if zero_taps is not None:
        for t in range(9):
            assert (float(cv[:, :, t].abs().max()) == 0.0) == (t in zero_taps), "tap %d" % t
    out = dn.dcn_rows(xr, offr, dn.dcn_group_packs(w.to(dev))).cpu()
    wg = w.double().reshape(4, cg, cg, 9).permute(0, 3, 2, 1).reshape(4, 9 * cg, cg)              # [g][t * cg + c][o]
    r64 = torch.cat([c64[g] @ wg[g] for g in range(4)], 1)
    r32 = torch.cat([c32[g] @ wg[g].float() for g in range(4)], 1)
    rs = torch.cat([split_mm(c32[g], wg[g].float()).float() for g in range(4)], 1)
    want = rows_of(R.dcn(x.double(), off.double(), w.double(), form="grid"))
    assert float((r64 - want).abs().max()) <= 1e-11 * float(want.abs().max())                     # the second form agrees
    assert_precise(out, r64, r32, rs, what="dcn " + what)
    return cols, out, outside


@pytest.mark.parametrize("H,W", [(7, 11), (16, 44)])
def test_dcn_offsets_as_input(dev, H, W):
    x, w, g = _dcn_inputs(H, W, 7 * H + W)
    zero = torch.zeros(2, 18, H, W)
    _, out, _ = _judge_dcn(dev, x, w, zero, "%dx%d zero offsets" % (H, W))
    conv = rows_of(F.conv2d(x.double(), w.double(), padding=1, groups=4))
    r32 = rows_of(F.conv2d(x, w, padding=1, groups=4))
    cols0 = R.cols_as_rows(R.dcn_cols_gather(x.float(), zero))
    wg = w.reshape(4, 32, 32, 9).permute(0, 3, 2, 1).reshape(4, 288, 32)
    rs = torch.cat([split_mm(cols0[k], wg[k]).float() for k in range(4)], 1)
    assert_precise(out, conv, r32, rs, what="dcn %dx%d zero offsets vs conv2d(groups=4)" % (H, W))
    _judge_dcn(dev, x, w, (torch.randn(2, 18, H, W, generator=g) * 3).round(), "%dx%d integer offsets" % (H, W))
    _judge_dcn(dev, x, w, torch.randn(2, 18, H, W, generator=g) * 3, "%dx%d sigma 3" % (H, W))
    _, _, outside = _judge_dcn(dev, x, w, torch.randn(2, 18, H, W, generator=g) * 20, "%dx%d sigma 20" % (H, W))
    assert 0.0 < float(outside.double().mean()) < 1.0
    _judge_dcn(dev, x, w, _hand_placed(H, W), "%dx%d hand-placed" % (H, W), zero_taps=(0, 2, 4, 6))
    core.check_h2_overflow()


def test_dcn_in_chunks(dev, monkeypatch):
    H, W = 7, 11
    x, w, g = _dcn_inputs(H, W, 5)
    off = torch.randn(2, 18, H, W, generator=g) * 3
    _, whole, _ = _judge_dcn(dev, x, w, off, "7x11 one chunk")
    monkeypatch.setattr(dn, "DCN_CHUNK_ROWS", 60)                    # 154 rows: chunks of 60, 60, 34
    _, parts, _ = _judge_dcn(dev, x, w, off, "7x11 chunks of 60")
    assert bits_equal(whole, parts)


# ------------------------------------------------------------------ 3. SE gates, pooled branch, ASPP
@pytest.mark.parametrize("H,W", [(5, 7), (16, 44)])
def test_gates_and_camera_means(dev, H, W):
    C, BN = 64, 2
    g = torch.Generator().manual_seed(H + W)
    x = torch.randn(BN, C, H, W, generator=g)
    ga, gb = torch.randn(BN, C, generator=g) * 2, torch.randn(BN, C, generator=g) * 2
    xr = as_rows(x, dev)
    a, b = dn.se_gate2(xr, ga.to(dev), gb.to(dev))
    for got, gate, nm in ((a, ga, "a"), (b, gb, "b")):
        want = rows_of(x.double() * torch.sigmoid(gate.double())[:, :, None, None])              # each camera's rows, its own gate
        assert_precise(got.t.cpu(), want, rows_of(x * torch.sigmoid(gate)[:, :, None, None]), what="se gate %s %dx%d" % (nm, H, W))
    mean = dn.camera_means(xr).cpu()
    assert_precise(mean, x.double().mean((2, 3)), x.mean((2, 3)), what="camera means %dx%d" % (H, W))
    swapped = dn.camera_means(as_rows(x.flip(0), dev)).cpu()
    assert bits_equal(swapped, mean.flip(0))


def _aspp(dev, mid, seed):
    torch.manual_seed(seed)
    m = dn.ASPP(mid, mid)
    sd = synth.random_state_dict(m.state_dict(), seed=seed)
    m.load_state_dict(sd)
    return m.to(dev).eval(), {("a." + k): v for k, v in sd.items()}


@pytest.mark.parametrize("H,W", [(5, 7), (16, 44)])
def test_aspp_block_and_camera_swap(dev, H, W):
    mid, BN = 64, 2
    m, sd = _aspp(dev, mid, 11)
    g = torch.Generator().manual_seed(H * W)
    x = torch.randn(BN, mid, H, W, generator=g) * torch.tensor([1.0, 2.0]).view(2, 1, 1, 1)
    want = rows_of(R.aspp(x.double(), R.cast(sd, torch.float64), "a"))
    w32 = rows_of(R.aspp(x, R.cast(sd, torch.float32), "a"))
    assert rel_err(w32, want) <= TOL / 4
    packs = dn.aspp_packs(m)
    tables = [dn.neighbour_table(BN, H, W, d, dev) for d in dn.ASPP_DILATIONS]
    out = dn.aspp_rows(as_rows(x, dev), packs, tables).t.cpu()
    assert_close(out, want, what="aspp %dx%d" % (H, W))
    # each camera's rows use that camera's mean: swapping the cameras' inputs swaps their outputs
    out_sw = dn.aspp_rows(as_rows(x.flip(0), dev), packs, tables).t.cpu()
    assert bits_equal(out_sw.view(2, H * W, mid).flip(0), out.view(2, H * W, mid))
    assert not bits_equal(out.view(2, H * W, mid)[0], out.view(2, H * W, mid)[1])
    core.check_h2_overflow()


@pytest.fixture(scope="module")
def fix(golden):
    z = golden("depthnet")
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    return sd, {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("sd/")}


@pytest.fixture(scope="module")
def fix_net(fix, dev):
    net = dn.DepthNet(32, 32, 16, 24)
    net.load_state_dict(fix[0], strict=True)
    return net.to(dev).eval()


def test_aspp_block_reproduces_the_fixture(dev, fix, fix_net):
    sd, t = fix
    x = t["aspp_in"]
    BN, mid, H, W = x.shape
    w32 = R.aspp(x.float(), R.cast({k: v for k, v in sd.items()}, torch.float32), "depth_conv.3")
    assert rel_err(w32, t["aspp_out"]) <= TOL / 4
    tables, taps = fix_net._aspp_tables(BN, H, W, dev)
    assert [len(k) for k in taps] == [9, 3, 3] and [tb.shape[0] for tb in tables] == [9, 3, 3]      # 12 x 20: vertical taps dead at 12, 18
    out = dn.aspp_rows(as_rows(x, dev), fix_net._packed()["aspp"], tables, taps).t.cpu()
    assert_close(out, rows_of(t["aspp_out"]), what="aspp fixture")
    full = [dn.neighbour_table(BN, H, W, d, dev) for d in dn.ASPP_DILATIONS]
    assert bits_equal(dn.aspp_rows(as_rows(x, dev), fix_net._packed()["aspp"], full).t.cpu(), out)      # leaving dead taps out is exact


# ------------------------------------------------------------------ 4. / 5. the whole module
def test_module_reproduces_the_fixture(dev, fix, fix_net):
    sd, t = fix
    assert rel_err(R.depth_net(sd, t["x"].float(), t["mlp_input"].float()), t["out"]) <= TOL / 4
    with torch.no_grad():
        out = fix_net(t["x"].to(dev), t["mlp_input"].to(dev))
    assert tuple(out.shape) == tuple(t["out"].shape)
    assert_close(out.cpu(), t["out"], what="DepthNet fixture: depth logits | context")
    assert_close(out[:, :24].cpu(), t["out"][:, :24], what="DepthNet fixture: depth logits")
    assert_close(out[:, 24:].cpu(), t["out"][:, 24:], what="DepthNet fixture: context")
    core.check_h2_overflow()


def _seeded(args, seed, offset_std=0.0):
    torch.manual_seed(seed)
    net = dn.DepthNet(*args)
    if offset_std:
        with torch.no_grad():
            net.depth_conv[4].conv_offset.weight.normal_(0.0, offset_std)
    return net.eval()


@pytest.mark.parametrize("args,BN,H,W,offset_std", [((512, 512, 128, 112), 1, 4, 6, 0.0), ((128, 128, 128, 112), 2, 16, 44, 0.01)])
def test_module_against_the_restatement(dev, args, BN, H, W, offset_std):
    net = _seeded(args, 3, offset_std)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(BN + H)
    x = torch.randn(BN, args[0], H, W, generator=g)
    mlp = torch.randn(1, BN, 27, generator=g)
    want = R.depth_net(sd, x.double(), mlp.double())
    assert rel_err(R.depth_net(sd, x, mlp), want) <= TOL / 4
    with torch.no_grad():
        out = net.to(dev)(x.to(dev), mlp.to(dev))
    assert_close(out.cpu(), want, what="DepthNet%s BN=%d %dx%d" % (args, BN, H, W))
    core.check_h2_overflow()


# ------------------------------------------------------------------ 6. the view transformer lifts by itself
def test_view_transformer_with_the_hip_depth_net(dev):
    torch.manual_seed(5)
    vt = pkg.ViewTransformerLiftSplatShootVoxel(
        grid_config={'xbound': [-8., 8., 2.], 'ybound': [-8., 8., 2.], 'zbound': [-2., 2., 2.], 'dbound': [2.0, 10.0, 1.0]},
        data_config={'input_size': (64, 96)}, numC_input=32, numC_Trans=16, downsample=16, depth_net='hip')
    with torch.no_grad():
        vt.depth_net.depth_conv[4].conv_offset.weight.normal_(0.0, 0.02)
    sd = {k: v.detach().clone() for k, v in vt.depth_net.state_dict().items()}
    vt = vt.to(dev).eval()
    D = vt.D
    assert D == 8
    rig = synth.camera_rig(ncam=2, input_size=(64, 96))
    cams = tuple(rig[k].to(dev) for k in ("rots", "trans", "intrins", "post_rots", "post_trans", "bda"))
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 2, 32, 4, 6, generator=g)
    mlp = torch.randn(1, 2, 27, generator=g)
    inp = (x.to(dev),) + cams + (mlp.to(dev),)
    want = R.depth_net(sd, x.view(2, 32, 4, 6).double(), mlp.double())
    assert rel_err(R.depth_net(sd, x.view(2, 32, 4, 6), mlp), want) <= TOL / 4
    with torch.no_grad():
        dp, feat = vt.lift(inp)
        assert tuple(dp.shape) == (2, D, 4, 6) and tuple(feat.shape) == (2, 16, 4, 6)
        assert float((dp.sum(1) - 1).abs().max()) <= 1e-5
        assert_close(dp.cpu(), want[:, :D].softmax(1), what="lift: depth_prob")
        assert_close(feat.cpu(), want[:, D:], what="lift: img_feat")
        bev, dp2, geom, vol = vt.forward(inp)
        assert bits_equal(dp2, dp)
        again = vt.lift_splat(dp, feat, cams=cams)
    assert tuple(bev.shape) == (1, 16, 8, 8, 2) and float(bev.abs().sum()) > 0
    assert bits_equal(bev, again)
    core.check_h2_overflow()


# ------------------------------------------------------------------ 7. one captured graph
def test_forward_in_one_captured_graph_equals_eager(dev):
    net = _seeded((64, 64, 32, 16), 9, 0.02).to(dev)
    g = torch.Generator().manual_seed(10)
    xa, xb = (torch.randn(2, 64, 16, 44, generator=g).to(dev) for _ in range(2))
    mlp = torch.randn(1, 2, 27, generator=g).to(dev)
    with torch.no_grad():
        want_a = net(xa, mlp).clone()
        want_b = net(xb, mlp).clone()
        static = xa.clone()
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            net(static, mlp)                                  # warm-up on the capture stream: packs, tables, scratch buffers
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                out = net(static, mlp)
        torch.cuda.current_stream(dev).wait_stream(s)
        keep = core.stream_scratch(dev, s)
        graph.replay()
        torch.cuda.synchronize()
        assert bits_equal(out, want_a)
        static.copy_(xb)
        graph.replay()
        torch.cuda.synchronize()
        assert bits_equal(out, want_b) and not bits_equal(want_a, want_b)
    assert keep is not None
    core.check_h2_overflow()
