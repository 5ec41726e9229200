"""``SparseEncoderHD`` on the HIP sparse engine, GPU half: the per-axis rule books against the brute-force book (exactly), the module
against its float64 restatement (tests/ref_sparse_hd.py; the project's scale-relative bound ``util.TOL``), the LiDAR-only detector
from a raw cloud, one full-size run.  spconv v1 cannot be built here, so no fixture comes from the unmodified module: the
restatement is checked against two independent forms in tests/test_sparse_hd_host.py."""
import contextlib
import signal

import numpy as np
import pytest
import torch

import co_occ_amd as pkg
import co_occ_amd.synth as synth
from co_occ_amd import core, lidar_hd, lidar_trunk as lt
from co_occ_amd.lidar_hd import SparseEncoderHD, SparseLevel

import ref_sparse_hd as R
import util

pytestmark = pytest.mark.gpu

K3, S1, S2, P1, P011 = (3, 3, 3), (1, 1, 1), (2, 2, 2), (1, 1, 1), (0, 1, 1)
CHAIN = [(K3, S2, P1), (K3, S2, P1), (K3, S2, P011)]
BOOK_CASES = {"21x21x27": ((21, 21, 27), CHAIN), "17x24x24": ((17, 24, 24), CHAIN), "s1_p011": ((21, 21, 27), [(K3, S1, P011)])}


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_level(level, coors_np):
    """SubM k3 and the 1x1x1 book of one level against the brute-force book on the same coordinates."""
    for k in (K3, (1, 1, 1)):
        outs, table, _ = R.brute_book(coors_np, level.shape, k, S1, tuple(v // 2 for v in k))
        # SubM keeps the input rows: the brute-force outputs (every site an input reaches) restricted to the active set
        lut = {tuple(c): j for j, c in enumerate(outs.tolist())}
        cols = [lut[tuple(c)] for c in coors_np.tolist()]
        assert np.array_equal(level.table(k).cpu().numpy(), table[:, cols]), "SubM table, kernel %r" % (k,)


@pytest.mark.parametrize("case", list(BOOK_CASES))
def test_rule_books_equal_the_brute_force_book(dev, case):
    shape, chain = BOOK_CASES[case]
    coors_np = R.edge_voxels(shape)
    level = SparseLevel(torch.from_numpy(coors_np).to(dev), shape)
    _check_level(level, coors_np)
    dropped = False
    for k, s, p in chain:
        outs, table, osz = R.brute_book(coors_np, level.shape, k, s, p)
        if p == P011 and s == S2:
            reached = set(np.unique(table[table >= 0]).tolist())
            dropped = dropped or len(reached) < len(coors_np)
            if case == "21x21x27":
                assert level.shape[0] == 6 and (coors_np[:, 0] == 5).any(), "the case holds a level-3 voxel at z = 5 that reaches no output"
                assert all(j not in reached for j in np.nonzero(coors_np[:, 0] == 5)[0])
        nxt, tb = level.downsample(k, s, p)
        assert nxt.shape == tuple(osz)
        assert np.array_equal(nxt.coors.cpu().numpy(), outs), "active set of %r / %r / %r on %r" % (k, s, p, level.shape)
        assert np.array_equal(tb.cpu().numpy(), table), "rule book of %r / %r / %r on %r" % (k, s, p, level.shape)
        D, H, W = osz
        assert np.array_equal(nxt.dense_rows().cpu().numpy(), (outs[:, 2] * H + outs[:, 1]) * D + outs[:, 0])
        level, coors_np = nxt, outs.astype(np.int32)
        _check_level(level, coors_np)
    if case == "21x21x27":
        assert level.shape == (2, 3, 4) and dropped


def test_rule_books_of_an_empty_set(dev):
    level = SparseLevel(torch.zeros(0, 3, dtype=torch.int32, device=dev), (21, 21, 27))
    assert tuple(level.table().shape) == (27, 0)
    nxt, tb = level.downsample(K3, S2, P011)
    assert nxt.shape == (10, 11, 14) and nxt.M == 0 and tuple(tb.shape) == (27, 0)
    # and a non-empty set none of whose voxels reaches an output
    one = SparseLevel(torch.tensor([[5, 3, 3]], dtype=torch.int32, device=dev), (6, 7, 7))
    nxt, tb = one.downsample(K3, S2, P011)
    assert nxt.shape == (2, 4, 4) and nxt.M == 0 and tuple(tb.shape) == (27, 0)


# ----------------------------------------------------------------------------- the module
SHAPE = [21, 21, 27]
MODULE_CFGS = {
    "basicblock": dict({k: v for k, v in synth.model_cfg_lidar()["pts_middle_encoder"].items() if k != "type"}, sparse_shape=SHAPE),
    "conv_module": dict(in_channels=4, sparse_shape=SHAPE),                 # the constructor defaults, (0,1,1) padding included
}
_REF = {}


def _module_case(kind):
    if kind not in _REF:
        cfg = MODULE_CFGS[kind]
        m = SparseEncoderHD(**cfg)
        sd = synth.random_state_dict(m.state_dict(), seed=71)
        # a cluster in one corner region + single voxels: the final grid (2 x 3 x 4 / 4 x 6 x 7) keeps inactive sites
        coors = np.unique(np.concatenate([R.random_voxels((9, 9, 12), 400, 5), np.asarray([[0, 20, 0], [12, 3, 26], [20, 8, 13]], np.int32)]), axis=0)
        g = torch.Generator().manual_seed(72)
        feats = torch.randn(len(coors), 4, generator=g)
        want, mask = R.encoder_forward(sd, cfg, feats, coors)
        _REF[kind] = dict(cfg=cfg, sd=sd, coors=torch.from_numpy(coors), feats=feats, want=want, mask=mask)
    return _REF[kind]


@pytest.fixture
def engine(request):
    """core.CONV_ENGINE = the parameter's engine for the test body; "h2_narrow" = the split-f16 engine with the 16-wide first stage
    kept on 16-wide fp32-MFMA rows (``wide16 = False``, the COOCC_HD_WIDE16=0 form)."""
    old = core.CONV_ENGINE
    core.CONV_ENGINE = request.param.split("_")[0]
    yield request.param
    core.CONV_ENGINE = old


@pytest.mark.parametrize("engine", ["h2", "h2_narrow", "f32"], indirect=True)
@pytest.mark.parametrize("kind", list(MODULE_CFGS))
def test_module_matches_the_float64_restatement(dev, kind, engine):
    c = _module_case(kind)
    m = SparseEncoderHD(**c["cfg"])
    m.load_state_dict(c["sd"], strict=True)
    m = m.to(dev).eval()
    m.wide16 = engine == "h2"
    with torch.no_grad():
        y = m(c["feats"].to(dev), c["coors"].to(dev), 1)
        y2 = m(c["feats"].to(dev), torch.cat([torch.zeros(len(c["coors"]), 1, dtype=torch.int32), c["coors"]], 1).to(dev), 1)
    core.check_h2_overflow()
    want, mask = c["want"], c["mask"]
    assert tuple(y.shape) == tuple(want.shape) == (1, 128) + m.out_shape()
    e = util.rel_err(y, want)
    print("[sparse_hd] %s %s: scale-relative error %.3e against float64 (max|ref| %.2f, %d active outputs)"
          % (kind, engine, e, float(want.abs().max()), int(mask.sum())))
    assert e <= util.TOL, "%s (%s engine): %.3e from the float64 restatement" % (kind, engine, e)
    assert bool((~mask).any()) and bool(mask.any())
    off = (~mask).expand_as(want)
    assert float(y.cpu()[off].abs().max()) == 0.0, "the dense output is exactly zero off the active set"
    assert int(mask.sum()) == m.last_active and bits_equal(y, y2)
    r = lt.rows_of_bczyx(y)
    assert r is not None and lt.bczyx_to_rows(y) is r and r.t.data_ptr() == y.data_ptr()      # channels-last rows, remembered


def test_coordinates_outside_the_grid_are_refused(dev):
    m = SparseEncoderHD(**MODULE_CFGS["basicblock"]).to(dev).eval()
    f = torch.zeros(2, 4, device=dev)
    for bad in ([[0, 0, 0], [21, 0, 0]], [[0, 0, 27], [1, 1, 1]], [[0, -1, 0], [1, 1, 1]]):
        with pytest.raises(ValueError, match="outside sparse_shape"):
            m(f, torch.tensor(bad, dtype=torch.int32, device=dev), 1)


def test_module_on_an_empty_cloud_gives_zeros(dev):
    m = SparseEncoderHD(**MODULE_CFGS["basicblock"]).to(dev).eval()
    with torch.no_grad():
        y = m(torch.zeros(0, 4, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev), 1)
    assert tuple(y.shape) == (1, 128, 2, 3, 4) and float(y.abs().max()) == 0.0


# ----------------------------------------------------------------------------- the detector from a raw cloud
def _small_detector_cfg():
    rng = [-4.0, -4.0, -2.0, 4.0, 4.0, 2.0]
    cfg = synth.model_cfg_lidar()
    cfg["pts_voxel_layer"] = dict(max_num_points=10, point_cloud_range=rng, voxel_size=[0.125] * 3, max_voxels=(4000, 4000))
    cfg["pts_middle_encoder"] = dict(cfg["pts_middle_encoder"], in_channels=5, sparse_shape=[33, 64, 64])
    cfg["pts_bbox_head"] = dict(cfg["pts_bbox_head"], final_occ_size=[16, 16, 8], fine_topk=100, point_cloud_range=rng)
    return cfg


def test_detector_runs_from_a_raw_cloud(dev):
    det = pkg.build_detector(_small_detector_cfg(), sparse_encoder_hd=True)
    det.load_state_dict(synth.random_state_dict(det.state_dict(), seed=9, gain=0.5))
    det = det.to(dev).eval()
    g = torch.Generator().manual_seed(10)
    pts = torch.cat([(torch.rand(3000, 3, generator=g) - 0.5) * torch.tensor([7.9, 7.9, 3.9]), torch.rand(3000, 2, generator=g)], 1).to(dev)
    conversions = ("coocc_zyx_to_rows", "coocc_ncdhw_to_ndhwc", "coocc_ndhwc_to_ncdhw")
    with torch.no_grad():
        voxels, coors, num = det.pts_voxel_layer(pts)
        feats = det.pts_voxel_encoder(voxels, num, coors)
        mid = det.pts_middle_encoder(feats, coors, 1)
        assert tuple(mid.shape) == (1, 128, 4, 8, 8)
        r = lt.rows_of_bczyx(mid)
        assert r is not None and lt.bczyx_to_rows(mid) is r and r.t.data_ptr() == mid.data_ptr()
        core.TIMER.enabled, core.TIMER.only = 2, None         # level 2: every C-ABI call is recorded
        core.TIMER.reset()
        a = det.simple_test(points=[pts])
        names = util.kernels_stop()
        assert names.get("coocc_voxelize_hard") == 1 and names.get("coocc_sparse_conv_table3", 0) >= 4, names
        assert not any(k in names for k in conversions), "a layout conversion between encoder, trunk and decoder: %s" % names
        b = det.simple_test(precomputed=dict(pts_middle_feats=mid))
        a2 = det.simple_test(points=[pts])
        c = det.forward(return_loss=False, points=[pts])
        fr = det.serving_frame(points=[pts])
    core.check_h2_overflow()
    assert a["voxel_feats"] is not None and a["pred_c"] is not None
    for key in ("voxel_feats", "pred_c", "pred_f"):
        if a[key] is None:
            assert b[key] is None and c[key] is None, key
            continue
        assert bool(torch.isfinite(a[key]).all()), key
        assert bits_equal(a[key], b[key]), "%s: from the cloud vs from the module's output" % key
        assert bits_equal(a[key], a2[key]), "%s: run to run" % key
        assert bits_equal(a[key], c[key]), "%s: forward(return_loss=False)" % key
    assert bits_equal(core.to_rows(fr["pts"]).t, core.to_rows(a["voxel_feats"]).t)
    with pytest.raises(ValueError, match=r"5 channels.*in_channels = 4"):
        bad = pkg.build_detector(dict(_small_detector_cfg(), pts_middle_encoder=dict(_small_detector_cfg()["pts_middle_encoder"], in_channels=4)),
                                 sparse_encoder_hd=True).to(dev).eval()
        bad.extract_pts_feat([pts])


# ----------------------------------------------------------------------------- the config's own size
@contextlib.contextmanager
def _time_limit(seconds):
    """The test's own time limit: SIGALRM ends it instead of letting a slow run hold the suite."""
    def on_alarm(signum, frame):
        raise TimeoutError("the full-size run took more than %d s" % seconds)
    old = signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def test_full_size_run_fills_the_voxel_cap(dev):
    with _time_limit(120):
        _full_size_run(dev)


def _full_size_run(dev):
    """[65, 800, 800], a synthetic cloud that fills the 120 000-voxel cap: shape, finiteness, active count = the brute-force count
    computed on the host from the coordinates, no range-guard flag."""
    cfg = synth.model_cfg_lidar()
    vl = pkg.Voxelization(**cfg["pts_voxel_layer"]).eval()
    mcfg = {k: v for k, v in cfg["pts_middle_encoder"].items() if k != "type"}
    m = SparseEncoderHD(**mcfg)
    m.load_state_dict(synth.random_state_dict(m.state_dict(), seed=12))
    m = m.to(dev).eval()
    pts = synth.lidar_points(400000, seed=3).to(dev)
    with torch.no_grad():
        voxels, coors, num = vl(pts)
        assert coors.shape[0] == 120000, "the cloud fills the cap"
        feats = pkg.HardSimpleVFE(num_features=4)(voxels, num, coors)
        y = m(feats, coors, 1)
    core.check_h2_overflow()                                             # raises if the range guard fired
    assert tuple(y.shape) == (1, 128, 8, 100, 100) and bool(torch.isfinite(y).all())
    c, shape = coors.cpu().numpy(), (65, 800, 800)
    for k, s, p in CHAIN:
        lin = R.active_outputs(c, shape, k, s, p)
        shape = R.out_size(shape, k, s, p)
        c = np.stack([lin // (shape[1] * shape[2]), (lin // shape[2]) % shape[1], lin % shape[2]], 1)
    assert shape == (8, 100, 100) and m.last_active == len(c)
    expected = np.zeros(8 * 100 * 100, bool)
    expected[(c[:, 0] * 100 + c[:, 1]) * 100 + c[:, 2]] = True
    nonzero = (y[0] != 0).any(0).cpu().numpy().reshape(-1)              # [Z, Y, X]
    assert not nonzero[~expected].any(), "a value outside the brute-force active set"
