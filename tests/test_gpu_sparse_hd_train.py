"""Training of ``SparseEncoderHD`` on the GPU (``lidar_hd``'s differentiable forward, csrc/sparse_train.hip): the transposed rule
books against the brute-force book (exactly), ``coocc_bn_apply_ex`` against ``coocc_bn_apply`` / ``coocc_rows_to_h2`` (bit for bit),
one down-convolution layer and the whole module against the float64 training-mode restatement (tests/ref_sparse_hd_train.py), the
LiDAR-only detector trained from a raw cloud, the co-runner guard of the new kernels, an empty cloud.

The bound of the float64 comparisons is the project's: scale-relative error <= ``util.TOL``, under the condition -- asserted per
tensor -- that the float32 torch evaluation of the same fixture is within TOL / 4 of float64 (``_cmp`` of
tests/test_gpu_trunk_train.py)."""
import numpy as np
import pytest
import torch

import co_occ_amd as pkg
import co_occ_amd.synth as synth
from co_occ_amd import autograd as ag, core, lidar_hd, lidar_trunk as lt
from co_occ_amd._lib import call, ptr
from co_occ_amd.lidar_hd import SparseEncoderHD, SparseLevel

import ref_sparse_hd as R
import ref_sparse_hd_train as RT
import test_gpu_sparse_hd as T
import util

pytestmark = pytest.mark.gpu

K3, S1, S2, P1, P011 = T.K3, T.S1, T.S2, T.P1, T.P011


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _cmp(got, r64, r32, what, tol=util.TOL):
    """``util.TOL`` scale-relative, under the condition that the fp32 torch evaluation is within a quarter of it."""
    e32 = util.rel_err(r32, r64)
    assert e32 <= tol / 4, "%s: the fp32 torch evaluation is %.3e from float64: TOL does not judge this fixture" % (what, e32)
    e = util.rel_err(got, r64)
    print("[sparse_hd train] %-58s scale-relative %.3e (fp32 torch %.3e)" % (what, e, e32))
    assert e <= tol, "%s: %.3e from float64" % (what, e)
    return e


@pytest.fixture
def engine(request):
    """core.CONV_ENGINE = the parameter's engine for the test body ("h2_narrow": the split-f16 engine with ``wide16 = False``)."""
    old = core.CONV_ENGINE
    core.CONV_ENGINE = request.param.split("_")[0]
    yield request.param
    core.CONV_ENGINE = old


# ----------------------------------------------------------------------------- a. transposed books
def _transpose(table, n_in):
    """[taps, Mo] forward book -> [taps, n_in]: the output row that reads input i through tap t, or -1."""
    inv = np.full((table.shape[0], n_in), -1, np.int64)
    t, o = np.nonzero(table >= 0)
    inv[t, table[t, o]] = o
    return inv


def _check_transposed(dev, level, coors_np, k, s, p):
    outs, table, osz = R.brute_book(coors_np, level.shape, k, s, p)
    nxt, tb = level.downsample(k, s, p)
    assert nxt.shape == tuple(osz) and np.array_equal(tb.cpu().numpy(), table)
    bwd, cls, classes = lidar_hd.dgrad_books(level, nxt, k, s, p, by_class=True)
    want = _transpose(table, len(coors_np))
    assert np.array_equal(bwd.cpu().numpy(), want), "transposed book of %r / %r / %r on %r" % (k, s, p, level.shape)
    c = coors_np.astype(np.int64)
    want_cls = (((c[:, 0] + p[0]) % s[0]) * s[1] + (c[:, 1] + p[1]) % s[1]) * s[2] + (c[:, 2] + p[2]) % s[2]
    assert np.array_equal(cls.cpu().numpy(), want_cls), "residue classes"
    taps = k[0] * k[1] * k[2]
    for cid in range(s[0] * s[1] * s[2]):                 # the live taps of a class cover every entry of its rows
        dead = sorted(set(range(taps)) - set(lidar_hd.class_taps(cid, k, s)))
        assert (want[dead][:, want_cls == cid] < 0).all(), "class %d reaches an output through a tap outside its live set" % cid
    if s == S1:
        assert classes is None
    else:
        seen = np.zeros(len(coors_np), bool)
        for rows, t_idx, sub in classes:
            rows, t_idx = rows.cpu().numpy(), t_idx.cpu().numpy()
            cid = want_cls[rows[0]]
            assert (want_cls[rows] == cid).all() and list(t_idx) == lidar_hd.class_taps(int(cid), k, s) and (np.diff(rows) > 0).all()
            assert np.array_equal(sub.cpu().numpy(), want[t_idx][:, rows])
            seen[rows] = True
        assert (want[:, ~seen] < 0).all(), "a row outside every class list is read by an output"
        if len(outs):
            assert seen.sum() == sum((want_cls == cid).sum() for cid in range(8) if lidar_hd.class_taps(cid, k, s))
    return nxt, outs.astype(np.int32)


@pytest.mark.parametrize("case", list(T.BOOK_CASES))
def test_transposed_books_equal_the_brute_force_book(dev, case):
    shape, chain = T.BOOK_CASES[case]
    coors_np = R.edge_voxels(shape)
    level = SparseLevel(torch.from_numpy(coors_np).to(dev), shape)
    for k, s, p in chain:
        level, coors_np = _check_transposed(dev, level, coors_np, k, s, p)
    if case == "21x21x27":
        assert level.shape == (2, 3, 4)


@pytest.mark.parametrize("voxel,shape,reaches", [((0, 0, 0), (6, 7, 7), True), ((5, 6, 6), (6, 7, 7), False), ((20, 20, 26), (21, 21, 27), True)])
def test_transposed_book_of_a_single_voxel(dev, voxel, shape, reaches):
    """A voxel in a corner, and an input set none of whose voxels reaches an output ((0,1,1) padding on an even extent: z = 5 of
    6): the book is all -1 there and no class is listed."""
    coors_np = np.asarray([voxel], np.int32)
    level = SparseLevel(torch.from_numpy(coors_np).to(dev), shape)
    nxt, _ = _check_transposed(dev, level, coors_np, K3, S2, P011)
    assert (nxt.M > 0) == reaches
    bwd, cls, classes = lidar_hd.dgrad_books(level, nxt, K3, S2, P011, by_class=True)
    assert tuple(bwd.shape) == (27, 1) and (bool((bwd >= 0).any()) == reaches) and (len(classes) > 0) == reaches


# ----------------------------------------------------------------------------- b. coocc_bn_apply_ex
@pytest.mark.parametrize("C", [32, 64, 128])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 257])
def test_bn_apply_ex_is_bn_apply_and_its_twin_is_rows_to_h2(dev, M, C):
    g = torch.Generator().manual_seed(100 * M + C)
    x = (torch.randn(M, C, generator=g) * 3 + 0.5).to(dev)
    res = torch.randn(M, C, generator=g).to(dev)
    mean, var = torch.randn(C, generator=g).to(dev), (torch.rand(C, generator=g) + 0.1).to(dev)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev)
    for r in (None, res):
        for relu in (0, 1):
            want = torch.empty_like(x)
            call("coocc_bn_apply", ptr(x), M, C, ptr(mean), ptr(var), ptr(gamma), ptr(beta), 1e-3, ptr(r), relu, ptr(want))
            want_h2 = torch.empty_like(x)
            call("coocc_rows_to_h2", ptr(want), C, M, C, 1.0, ptr(want_h2))
            y, y2, twin = torch.empty_like(x), torch.empty_like(x), torch.full_like(x, float("nan"))
            call("coocc_bn_apply_ex", ptr(x), M, C, ptr(mean), ptr(var), ptr(gamma), ptr(beta), 1e-3, ptr(r), relu, ptr(y), ptr(twin))
            call("coocc_bn_apply_ex", ptr(x), M, C, ptr(mean), ptr(var), ptr(gamma), ptr(beta), 1e-3, ptr(r), relu, ptr(y2), None)
            what = "M %d C %d res %s relu %d" % (M, C, r is not None, relu)
            assert bits_equal(y, want) and bits_equal(y2, want), "fp32 output, " + what
            assert bits_equal(twin, want_h2), "split-f16 twin, " + what
    core.check_h2_overflow()


# ----------------------------------------------------------------------------- c. one layer
def _layer_refs(w, bn_sd, feats, coors, shape, k, s, p, subm, gout_rows):
    """conv (spconv v1 weight) + BN1d (train) + ReLU on the dense grid in float64 and float32: rows of the outputs (SparseConv3d:
    ascending (z,y,x) order; SubMConv3d: the inputs' order), dx, dW, dgamma, dbeta, the updated running statistics."""
    refs = {}
    for dt in (torch.float64, torch.float32):
        wl = w.to(dt).clone().requires_grad_()
        sd = {"n." + kk: (v.to(dt).clone() if v.is_floating_point() else v.clone()) for kk, v in bn_sd.items()}
        sd["n.weight"].requires_grad_(), sd["n.bias"].requires_grad_()
        f = feats.to(dt).clone().requires_grad_()
        x = RT._scatter(f, torch.as_tensor(coors).long(), shape)
        _, mask = R.to_dense(feats, coors, shape)
        y, omask = R.conv_layer(x, mask, wl, k, s, p, subm)
        stats, counts = {}, {}
        y = torch.relu(RT.bn_rows_train(y, omask, sd, "n", 1e-3, 0.01, stats, counts))
        oc = torch.as_tensor(coors).long() if subm else torch.nonzero(omask[0, 0])          # (nonzero: ascending (z, y, x))
        rows = y[0][:, oc[:, 0], oc[:, 1], oc[:, 2]].t()
        (rows * gout_rows.to(dt)).sum().backward()
        refs[dt] = dict(y=rows.detach(), dx=f.grad, dw=wl.grad, dgamma=sd["n.weight"].grad, dbeta=sd["n.bias"].grad,
                        rm=stats["n.running_mean"], rv=stats["n.running_var"], n=counts["n"])
    return refs


def _layer_case(kind):
    shape = (9, 9, 12)
    if kind == "down":
        cin, cout, k, s, p, subm = 32, 64, K3, S2, P011, False
    else:
        cin, cout, k, s, p, subm = 16, 16, K3, S1, P1, True
    g = torch.Generator().manual_seed(31 + cin)
    coors = R.random_voxels(shape, 150, 7)
    feats = torch.randn(150, cin, generator=g)
    conv = lidar_hd.SparseConvV1(cin, cout, 3, stride=s, padding=p, subm=subm)
    w = (torch.randn(3, 3, 3, cin, cout, generator=g) * (2.0 / (27 * cin)) ** 0.5)
    bn = torch.nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01)
    bn_sd = synth.random_state_dict(bn.state_dict(), seed=32)
    n_out = len(R.active_outputs(coors, shape, k, s, p)) if not subm else 150
    gout = torch.randn(n_out, cout, generator=g)
    return dict(shape=shape, k=k, s=s, p=p, subm=subm, coors=coors, feats=feats, conv=conv, w=w, bn=bn, bn_sd=bn_sd, gout=gout,
                refs=_layer_refs(w, bn_sd, feats, coors, shape, k, s, p, subm, gout))


_LAYER = {}


def _run_layer(dev, c, by_class):
    conv, bn = c["conv"], c["bn"]
    with torch.no_grad():
        conv.weight.copy_(c["w"])
    bn.load_state_dict(c["bn_sd"])
    conv, bn = conv.to(dev), bn.to(dev).train()
    for prm in list(conv.parameters()) + list(bn.parameters()):
        prm.grad = None
    level = SparseLevel(torch.from_numpy(c["coors"]).to(dev), c["shape"])
    x = c["feats"].to(dev).requires_grad_()
    if c["subm"]:
        tb = level.table(c["k"])
        bwd = tb.flip(0).contiguous()
    else:
        nxt, tb = level.downsample(c["k"], c["s"], c["p"])
        table, _, classes = lidar_hd.dgrad_books(level, nxt, c["k"], c["s"], c["p"], by_class=by_class)
        assert (classes is not None) == by_class
        bwd = classes if by_class else table
    with util.kernels() as names:
        y, yh = lidar_hd.conv_bn_train(x, None, conv, bn, tb, bwd)
        (y * c["gout"].to(dev)).sum().backward()
    core.check_h2_overflow()
    return dict(y=y.detach(), dx=x.grad, dw=conv.weight.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, rm=bn.running_mean,
                rv=bn.running_var, nb=int(bn.num_batches_tracked), yh=yh), names


@pytest.mark.parametrize("engine", ["h2", "f32"], indirect=True)
@pytest.mark.parametrize("kind", ["down", "subm16"])
def test_one_layer_under_train_matches_float64(dev, kind, engine):
    """SparseConv3d(3, 2, (0,1,1)) 32 -> 64 (and SubMConv3d 16 -> 16, the width below the split-f16 engine's 32) + BN1d (train) +
    ReLU on a (9,9,12) grid with 150 voxels: output, dx, dW, dgamma, dbeta against float64; the strided dgrad per residue class and
    as one 27-tap launch, each against float64 and against each other to the same bound."""
    if kind not in _LAYER:
        _LAYER[kind] = _layer_case(kind)
    c = _LAYER[kind]
    r64, r32 = c["refs"][torch.float64], c["refs"][torch.float32]
    got = {}
    for by_class in ((True, False) if kind == "down" else (False,)):
        g, names = _run_layer(dev, c, by_class)
        got[by_class] = g
        assert tuple(g["dw"].shape) == tuple(c["w"].shape), "dW comes back in the v1 layout"
        for key in ("y", "dx", "dw", "dgamma", "dbeta"):
            _cmp(g[key].cpu(), r64[key], r32[key], "%s %s classes=%d %s" % (kind, engine, by_class, key))
        assert g["nb"] == 1
        for key in ("rm", "rv"):
            e = float((g[key].cpu().double() - r64[key]).abs().max())
            assert e <= 1e-5, "running statistic %s: %.3e" % (key, e)
        h2_fwd = engine == "h2" and c["feats"].shape[1] % 32 == 0
        assert any(n.startswith("k_gemm_h2 sparse_hd_fwd") for n in names) == h2_fwd, names
        assert any(n.startswith("k_gemm_h2 sparse_hd_dgrad") for n in names) == (engine == "h2" and c["w"].shape[4] % 32 == 0), names
        assert (g["yh"] is not None) == (engine == "h2" and c["w"].shape[4] % 32 == 0)
        if kind == "down":
            nd = sum(v for n, v in names.items() if "sparse_hd_dgrad" in n)
            assert nd == (8 if by_class else 1), names
    if kind == "down":
        e = util.rel_err(got[True]["dx"], got[False]["dx"])
        print("[sparse_hd train] down %s: dgrad per class vs one launch %.3e" % (engine, e))
        assert e <= util.TOL
        assert bits_equal(got[True]["y"], got[False]["y"]) and bits_equal(got[True]["dw"], got[False]["dw"])


# ----------------------------------------------------------------------------- d. the whole module
_REF = {}


def _module_case(kind):
    if kind not in _REF:
        c = dict(T._module_case(kind))
        cfg = c["cfg"]
        oshape = SparseEncoderHD(**cfg).out_shape()
        gout = torch.randn(1, 128, *oshape, generator=torch.Generator().manual_seed(73))
        c["gout"] = gout
        c["refs"] = {dt: RT.evaluate(c["sd"], cfg, c["feats"], c["coors"].numpy(), gout, dt) for dt in (torch.float64, torch.float32)}
        _REF[kind] = c
    return _REF[kind]


@pytest.mark.parametrize("engine", ["h2", "h2_narrow", "f32"], indirect=True)
@pytest.mark.parametrize("kind", list(T.MODULE_CFGS))
def test_module_under_train_matches_the_float64_restatement(dev, kind, engine):
    """Both configurations on the [21,21,27] fixture of the inference test under train(): the dense output, dfeats and every
    parameter's gradient within ``util.TOL`` of the float64 training-mode restatement (fp32 torch within TOL / 4, asserted per
    tensor; checked on the CPU when the fixture was written: 2.9e-6 at worst), exact zeros off the active set, and torch's
    running-statistics update to 1e-5 absolute -- with momentum 0.01 a biased variance in the update would be 0.01 / (n - 1) off,
    above 1e-4 for the n <= 100 rows of the last level, which the test asserts."""
    c = _module_case(kind)
    r64, r32 = c["refs"][torch.float64], c["refs"][torch.float32]
    m = SparseEncoderHD(**c["cfg"])
    m.load_state_dict(c["sd"], strict=True)
    m = m.to(dev).train()
    m.train_enabled = True
    m.wide16 = engine == "h2"
    f = c["feats"].to(dev).requires_grad_()
    y = m(f, c["coors"].to(dev), 1)
    assert y.grad_fn is not None and tuple(y.shape) == tuple(r64["y"].shape) == (1, 128) + m.out_shape()
    r = lt.rows_of_bczyx(y)
    assert r is not None and r.t.grad_fn is not None and r.t.data_ptr() == y.data_ptr()          # channels-last rows, remembered
    (y * c["gout"].to(dev)).sum().backward()
    core.check_h2_overflow()
    tag = "%s %s " % (kind, engine)
    _cmp(y.detach().cpu(), r64["y"], r32["y"], tag + "y")
    mask = r64["mask"]
    assert bool((~mask).any()) and bool(mask.any()) and int(mask.sum()) == m.last_active
    assert float(y.detach().cpu()[(~mask).expand_as(r64["y"])].abs().max()) == 0.0, "the dense output is exactly zero off the active set"
    _cmp(f.grad.cpu(), r64["dfeats"], r32["dfeats"], tag + "dfeats")
    worst = 0.0
    for k, p in m.named_parameters():
        assert p.grad is not None and tuple(p.grad.shape) == tuple(p.shape), k
        worst = max(worst, _cmp(p.grad.cpu(), r64[k + ".grad"], r32[k + ".grad"], tag + k + ".grad"))
    n_last = r64["counts"]["conv_out.1"]
    assert 2 <= n_last <= 100 and 0.01 / (n_last - 1) > 1e-4, "the last level's %d rows do not expose a biased running variance" % n_last
    for k, v in m.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1 == int(r64[k]), k
        else:
            e = float((v.cpu().double() - r64[k]).abs().max())
            assert e <= 1e-5, "%s: %.3e from torch's update" % (k, e)
    print("[sparse_hd train] %s worst parameter gradient %.3e, %d rows at the last level" % (tag, worst, n_last))


# ----------------------------------------------------------------------------- e. the detector
def test_detector_trains_its_sparse_encoder_from_a_raw_cloud(dev):
    cfg = T._small_detector_cfg()
    det = pkg.build_detector(cfg, sparse_encoder_hd=True, train_sparse_encoder_hd=True, train_lidar_trunk=True)
    sd = synth.random_state_dict(det.state_dict(), seed=9, gain=0.5)
    det.load_state_dict(sd)
    det = det.to(dev)
    det.graph_simple_test = False                         # eager launches: nothing here is about the captured graph
    g = torch.Generator().manual_seed(10)
    pts = torch.cat([(torch.rand(3000, 3, generator=g) - 0.5) * torch.tensor([7.9, 7.9, 3.9]), torch.rand(3000, 2, generator=g)], 1).to(dev)
    gt = torch.randint(0, 17, (1, 16, 16, 8), generator=g).to(dev)
    gen = lambda: torch.Generator(device=dev).manual_seed(0)
    conversions = ("coocc_zyx_to_rows", "coocc_ncdhw_to_ndhwc", "coocc_ndhwc_to_ncdhw")
    enc = [(k, p) for k, p in det.named_parameters() if k.startswith("pts_middle_encoder.")]
    trunk = [(k, p) for k, p in det.named_parameters() if k.startswith(("pts_backbone.", "pts_neck."))]
    assert len(enc) > 40 and len(trunk) > 60

    # frozen: today's path -- the encoder in eval mode, no gradient to it, and the same losses as a detector built without the option
    old = pkg.build_detector(cfg, sparse_encoder_hd=True, train_lidar_trunk=True)
    old.load_state_dict(sd)
    old = old.to(dev).freeze_lidar_encoder().train()
    want = old.forward_train(points=[pts], gt_occ=gt, gt_depths=None, generator=gen())
    det.freeze_lidar_encoder().train()
    assert not det.pts_middle_encoder.training
    losses = det.forward_train(points=[pts], gt_occ=gt, gt_depths=None, generator=gen())
    assert set(losses) == set(want)
    for k in want:
        assert bits_equal(losses[k].detach(), want[k].detach()), "frozen encoder, %s: not the losses of today's frozen path" % k
    sum(v for k, v in losses.items() if k.startswith("loss")).backward()
    assert all(p.grad is None for _, p in enc) and all(p.grad is not None for _, p in trunk)
    del old, want

    # unfrozen: every encoder and trunk parameter takes a finite, non-zero gradient; no layout conversion in the step
    det.load_state_dict(sd)
    det.freeze_lidar_encoder(False).train()
    det.zero_grad(set_to_none=True)
    assert det.pts_middle_encoder.training
    with torch.no_grad():
        det.eval()
        before = det.simple_test(points=[pts])
        det.train()
    rm0 = det.pts_middle_encoder.conv_input[1].running_mean.clone()
    core.TIMER.enabled, core.TIMER.only = 2, None         # level 2: every C-ABI call is recorded
    core.TIMER.reset()
    losses = det.forward_train(points=[pts], gt_occ=gt, gt_depths=None, generator=gen())
    assert all(v.requires_grad for k, v in losses.items() if k.startswith("loss"))
    sum(v for k, v in losses.items() if k.startswith("loss")).backward()
    names = util.kernels_stop()
    core.check_h2_overflow()
    assert names.get("coocc_sparse_dgrad_table3", 0) == 3 and names.get("coocc_bn_apply_ex", 0) + names.get("coocc_bn_apply", 0) > 20, names
    assert not any(k in names for k in conversions), "a layout conversion between encoder, trunk and decoder: %s" % names
    for k, p in enc + trunk:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, k
    assert not torch.equal(det.pts_middle_encoder.conv_input[1].running_mean, rm0), "a training-mode BN1d updates its running mean"

    # after an SGD step, eval() runs on the stepped weights (PackCache) and is bit-stable.  The losses of this randomly initialised
    # model are not normalised, so the step is sized by the largest gradient: no parameter moves by more than 1e-3
    gmax = max(float(p.grad.abs().max()) for _, p in enc + trunk)
    print("[sparse_hd train] detector: largest parameter gradient %.3e" % gmax)
    torch.optim.SGD([p for _, p in enc + trunk], lr=1e-3 / gmax).step()
    det.eval()
    with torch.no_grad():
        a = det.simple_test(points=[pts])
        b = det.simple_test(points=[pts])
    core.check_h2_overflow()
    assert bits_equal(a["voxel_feats"], b["voxel_feats"]) and bits_equal(a["pred_c"], b["pred_c"]), "run to run"
    assert not bits_equal(a["voxel_feats"], before["voxel_feats"]), "eval() after the step still runs the weights from before it"


# ----------------------------------------------------------------------------- f. co-runner guard
N_CALLS = 20


def test_new_kernels_are_bit_stable_beside_split_f16_gemms(dev):
    """In the manner of tests/test_gpu_trunk_train.py: 20 calls of each new kernel on fixed inputs beside split-f16 layers of a
    second stream give the bits they give alone."""
    g = torch.Generator().manual_seed(11)
    xb = core.to_rows(torch.randn(1, 128, 100, 100, 8, generator=g).to(dev))
    pc = core.PackedConv((torch.randn(128, 128, 1, 1, 1, generator=g) * 0.05).to(dev), ksize=1, pad=0)
    M, C = 60000, 64
    x, res = torch.randn(M, C, generator=g).to(dev), torch.randn(M, C, generator=g).to(dev)
    mean, var = torch.randn(C, generator=g).to(dev), (torch.rand(C, generator=g) + 0.1).to(dev)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev)
    shape = (17, 200, 200)
    level = SparseLevel(torch.from_numpy(R.random_voxels(shape, 40000, 4)).to(dev), shape)
    nxt, _ = level.downsample(K3, S2, P011)
    omap = nxt.index_map().clone()

    def fn():
        y, twin = torch.empty_like(x), torch.empty_like(x)
        call("coocc_bn_apply_ex", ptr(x), M, C, ptr(mean), ptr(var), ptr(gamma), ptr(beta), 1e-3, ptr(res), 1, ptr(y), ptr(twin))
        tb = torch.empty(27, level.M, device=dev, dtype=torch.int32)
        cls = torch.empty(level.M, device=dev, dtype=torch.int32)
        call("coocc_sparse_dgrad_table3", ptr(level.coors), level.M, *shape, *K3, *S2, *P011, *nxt.shape, ptr(omap), ptr(tb), ptr(cls))
        return y, twin, tb.view(torch.float32), cls.view(torch.float32)
    s0, s1 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    with torch.no_grad():
        core.conv_rows(xb, pc, relu=False)
        torch.cuda.synchronize()
        with torch.cuda.stream(s0):
            ref = fn()
        torch.cuda.synchronize()
        want = torch.empty_like(x)
        call("coocc_bn_apply", ptr(x), M, C, ptr(mean), ptr(var), ptr(gamma), ptr(beta), 1e-3, ptr(res), 1, ptr(want))
        assert bits_equal(ref[0], want) and int((ref[2].view(torch.int32) >= 0).sum()) > 0
        got = []
        for _ in range(N_CALLS):
            with torch.cuda.stream(s1):
                for _ in range(4):
                    core.conv_rows(xb, pc, relu=False)
            with torch.cuda.stream(s0):
                got.append(fn())
        torch.cuda.synchronize()
    core.check_h2_overflow()
    bad = sum(int(not all(bits_equal(a, b) for a, b in zip(ref, t))) for t in got)
    assert bad == 0, "the new kernels beside split-f16 GEMMs: %d of %d calls differ from the run alone" % (bad, N_CALLS)


# ----------------------------------------------------------------------------- g. an empty cloud
def test_module_under_train_on_an_empty_cloud(dev):
    m = SparseEncoderHD(**T.MODULE_CFGS["basicblock"]).to(dev).train()
    m.train_enabled = True
    rm = m.conv_input[1].running_mean.clone()
    f = torch.zeros(0, 4, device=dev, requires_grad=True)
    y = m(f, torch.zeros(0, 3, dtype=torch.int32, device=dev), 1)
    assert tuple(y.shape) == (1, 128, 2, 3, 4) and float(y.detach().abs().max()) == 0.0 and y.grad_fn is not None
    y.sum().backward()
    assert tuple(f.grad.shape) == (0, 4)
    for k, p in m.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0, k
    assert torch.equal(m.conv_input[1].running_mean, rm) and int(m.conv_input[1].num_batches_tracked) == 0
