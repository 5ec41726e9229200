"""The multi-sweep LiDAR cloud on the device (co_occ_amd/sweeps.py, csrc/sweeps.hip, coocc_sweeps_merge): everything bit for bit
(uint32 views) against the numpy restatement run on the CPU (tests/sweep_refs.py); where the restatement has a NaN the device must
have one.  Every randomised sample is one of sweep_refs.SAMPLES, whose seeds tests/test_sweeps_host.py holds to tie_free on all rows.
A tile of the kernels is 256 output rows, a wave 64."""
import numpy as np
import pytest
import torch

import sweep_refs as S
from co_occ_amd import sweeps as SW

pytestmark = pytest.mark.gpu
F = np.float32


def device_merge(dev, points, sweeps, ts, choices, use_dim=(0, 1, 2, 4), radius=1.0, out=None, count=None, **kw):
    """merge_sweeps on the raw buffer (the key frame, then the chosen sweeps): (the written rows on the host, the padded device buffer,
    the device count or None, the table)."""
    choices = list(choices)
    padded = kw.get("pad_empty_sweeps", False) and len(sweeps) == 0
    raw = np.concatenate([points] + ([] if padded else [sweeps[i]['points'] for i in choices]))
    table = SW.sweep_table(len(points), sweeps, ts, choices, **kw)
    buf, cnt = SW.merge_sweeps(torch.from_numpy(raw).to(dev), table, use_dim, radius, out=out, count=count)
    assert buf.dtype == torch.float32 and tuple(buf.shape) == (table.total, len(S.columns(use_dim))) and buf.is_contiguous()
    assert (cnt is not None) or not table.filtering
    n = int(cnt.item()) if cnt is not None else table.total
    return buf[:n].cpu().numpy(), buf, cnt, table


def check(dev, points, sweeps, ts, choices, use_dim=(0, 1, 2, 4), radius=1.0, **kw):
    got, _, cnt, table = device_merge(dev, points, sweeps, ts, choices, use_dim, radius, **kw)
    want, rows = S.restatement(points, sweeps, ts, choices, use_dim, radius=radius, **kw)
    assert len(got) == len(want), "the device kept %d rows, the restatement %d" % (len(got), len(want))
    assert S.same(got, want), "%d of %d values differ" % (int((got.view(np.uint32) != want.view(np.uint32)).sum()), got.size)
    assert rows[0] == len(points)
    if S.columns(use_dim)[:3] == [0, 1, 2]:                                  # the key frame: first, whole, its coordinates untouched
        assert np.array_equal(got[:len(points), :3].view(np.uint32), points[:, :3].view(np.uint32))
    return got, want, rows


def hand_sweep(rows, R=None, t=None, lag=0.25, ts=S.TS):
    rows = np.asarray(rows, F)
    full = np.zeros((len(rows), 5), F)
    full[:, :rows.shape[1]] = rows
    full[:, 3], full[:, 4] = np.arange(len(rows)) + 1, 9
    return S.sweep_entry(full, np.eye(3) if R is None else R, np.zeros(3) if t is None else t, lag, ts)


KEY = S.cloud(3, seed=90)


# ------------------------------------------------------------------ segment sizes, the choice rules
def test_segment_sizes_in_one_call(dev):
    """A key frame of 1 row; sweeps of 0, 1, 63, 64, 65, 255, 256 and 257 rows."""
    points, sweeps, ts = S.make("sizes")
    for rc in (True, False):
        got, want, rows = check(dev, points, sweeps, ts, range(8), remove_close=rc)
        assert rows[0] == 1 and (rows[1:] == [0, 1, 63, 64, 65, 255, 256, 257]) == (not rc)
    lags = [F(ts - sw['timestamp'] / 1e6) for sw in sweeps]
    assert got[0, 3] == 0 and got[1:, 3].tolist() == np.repeat(lags, rows[1:]).tolist() and len(set(lags)) == 8          # column 4


def test_no_sweeps_at_all(dev):
    points, sweeps, ts = S.make("none")
    for rc in (False, True):
        got, want, rows = check(dev, points, sweeps, ts, [], remove_close=rc)
        assert rows == [300] and not got[:, 3].any() and points[:, 4].any()
    got, _, _, _ = device_merge(dev, points[:0], sweeps, ts, [])
    assert got.shape == (0, 4)


def test_twelve_sweeps_take_ten(dev):
    points, sweeps, ts = S.make("twelve")
    first = SW.choose_sweeps(12, 10, test_mode=True)
    drawn = SW.choose_sweeps(12, 10, rng=np.random.RandomState(5))
    assert first.tolist() == list(range(10)) and drawn.tolist() == np.random.RandomState(5).choice(12, 10, replace=False).tolist()
    a, _, rows_a = check(dev, points, sweeps, ts, first)
    b, _, rows_b = check(dev, points, sweeps, ts, drawn, remove_close=True)
    assert rows_a[1:] == [30 + 7 * k for k in first] and len(rows_b) == 11 and drawn.tolist() != sorted(drawn.tolist())
    # the loader draws the same ten from a generator in the same state
    cloud, extras = SW.LoadPointsFromMultiSweeps(remove_close=True, device=dev, rng=np.random.RandomState(5))(points, sweeps, ts)
    assert extras["choices"].tolist() == drawn.tolist() and S.same(cloud.cpu().numpy(), b)
    cloud, extras = SW.LoadPointsFromMultiSweeps(test_mode=True, device=dev)(points, sweeps, ts)
    assert extras["choices"].tolist() == first.tolist() and S.same(cloud.cpu().numpy(), a) and extras["rows"] == rows_a


# ------------------------------------------------------------------ hand-placed rows
def test_hand_placed_rows(dev):
    tiny, big = 2.0 ** -149, float(np.finfo(F).max)
    swap = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 2]])                     # small integers: exact in every order
    sweeps = [
        hand_sweep([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, -0.0, 3], [-0.0, 5, -0.0], [-3, -0.0, 0.0]], swap, [0.0, 0.0, 0.0]),
        hand_sweep([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [-4, 2, -0.0], [4, -2, 8]], swap, [4.0, -2.0, -16.0]),      # sums that cancel to 0
        hand_sweep([[tiny, 0, 0], [0, -tiny, 0], [tiny, tiny, -tiny], [3 * tiny, 0, 2.0 ** -126]]),                  # denormals in and out
        hand_sweep([[2.0 ** -148, 0, 0], [2.0 ** -126, 2.0 ** -127, 6 * tiny]], np.eye(3) * 0.5),                    # denormals made
        hand_sweep([[big, 0, 0], [-big, 1, 2], [big, big, 0], [2.0 ** 127, 0, 0]], np.eye(3) * 2.0),                 # past FLT_MAX: inf
        hand_sweep([[big, 0, 0], [0, -big, 0]], None, [big, -big, 0.0]),                                             # ... by the second rounding
        hand_sweep([[np.nan, 1, 2], [1, np.nan, 2], [np.inf, 1, 2], [1, -np.inf, 2], [np.inf, -np.inf, np.nan], [1, 2, np.inf]], swap,
                   [1.0, 2.0, 4.0]),
        hand_sweep([[1, 1, 0]], np.array([[1.0, 2.0 ** -24, 0], [0, 1, 0], [0, 0, 1]]), [2.0 ** -24, 0.0, 0.0]),     # two roundings, not one
    ]
    got, want, rows = check(dev, KEY, sweeps, S.TS, range(len(sweeps)))
    at = np.cumsum([0] + rows)
    seg = [got[at[k + 1]:at[k + 2]] for k in range(len(sweeps))]
    assert np.array_equal(np.signbit(seg[0][:, :3]), np.signbit(want[at[1]:at[2], :3])) and not seg[0][0, :3].any()
    assert seg[2][0, 0] == F(tiny) and seg[2][1, 1] == -F(tiny) and seg[3][0, 0] == F(tiny) and seg[3][1, 2] == F(3 * tiny)
    assert np.isinf(seg[4][:, 0]).all() and np.isinf(seg[5][0, 0]) and np.isinf(seg[5][1, 1]) and seg[5][1, 1] < 0
    assert np.isnan(seg[6][0, 1]) and np.isnan(seg[6][1, 0]) and np.isnan(seg[6][4, :3]).all() and np.isinf(seg[6][5, 2])
    assert seg[7][0, 0] == F(1.0)
    assert (got[at[1]:, 3] == F(S.TS - sweeps[0]['timestamp'] / 1e6)).all() and not got[:3, 3].any()


def test_identity_returns_the_input_bits(dev):
    pts = S.cloud(777, seed=91)
    pts[:5, :3] = [[2.0 ** -149, 2.0 ** -140, -2.0 ** -130], [1e-38, -1e-39, 1e-45], [3.4e38, -3.4e38, 1], [1e-20, 1e20, -1], [7, -7, 0.1]]
    assert (pts[:, :3] != 0).all()
    got, want, rows = check(dev, KEY, [S.sweep_entry(pts, np.eye(3), np.zeros(3), 0.5)], S.TS, [0], use_dim=5)
    assert np.array_equal(got[3:, :4].view(np.uint32), pts[:, :4].view(np.uint32)) and (got[3:, 4] == F(0.5)).all()


def test_a_lag_fp32_does_not_hold(dev):
    ts, stamp = 0.3, 0.2 * 1e6
    lag = ts - stamp / 1e6
    assert float(F(lag)) != lag
    sw = dict(hand_sweep([[1, 2, 3], [4, 5, 6]]), timestamp=stamp)
    got, _, _ = check(dev, KEY, [sw], ts, [0])
    assert (got[3:, 3] == F(lag)).all()


# ------------------------------------------------------------------ remove_close
def test_remove_close_edges(dev):
    below, above = np.nextafter(F(1), F(0)), np.nextafter(F(1), F(2))
    rows = [[1.0, 0, 0], [-1.0, 0, 1], [0, 1.0, 2], [0.5, -1.0, 3],                   # |x| == r or |y| == r exactly: kept
            [below, 0.5, 4], [-below, -below, 5], [0.0, -0.0, 6], [2.0 ** -149, 0, 7],  # just inside: dropped
            [0.5, 2, 8], [-0.25, above, 9], [3, 0.5, 10], [above, 0, 11],             # one of the two not close: kept
            [np.nan, 0, 12], [0, np.nan, 13], [np.nan, np.nan, 14], [np.inf, 0, 15]]  # a NaN is never close
    keep = [True] * 4 + [False] * 4 + [True] * 8
    rot = np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]])
    got, want, n = check(dev, KEY, [hand_sweep(rows, rot, [64.0, 32.0, 0.0])], S.TS, [0], use_dim=5, remove_close=True)
    assert n == [3, 12] and got[3:, 3].tolist() == [i + 1.0 for i, k in enumerate(keep) if k]              # by the row tags in column 3
    # the filter reads the untransformed coordinates: with the transform's output it would keep everything here
    assert S.not_close(want[3:]).all()
    # the key frame is never filtered
    near = np.zeros((5, 5), F)
    got, _, n = check(dev, near, [hand_sweep(rows)], S.TS, [0], remove_close=True)
    assert n == [5, 12]


@pytest.mark.parametrize("radius", [0.1, 0.7, 2.5])
def test_radius_is_compared_in_fp32(dev, radius):
    """float32(0.1) lies above 0.1 and float32(0.7) below 0.7: a comparison with the double would drop |x| == float32(0.7)."""
    r = F(radius)
    rows = [[r, 0, 0], [np.nextafter(r, F(0)), 0, 1], [np.nextafter(r, F(9)), 0, 2], [0, -r, 3], [0, -np.nextafter(r, F(0)), 4],
            [np.nextafter(r, F(0)), np.nextafter(r, F(0)), 5]]
    got, _, n = check(dev, KEY, [hand_sweep(rows)], S.TS, [0], use_dim=5, radius=radius, remove_close=True)
    assert n == [3, 3] and got[3:, 3].tolist() == [1.0, 3.0, 4.0]


def _tagged(n, close):
    """n rows tagged 0 .. n-1 in column 3, row i within the radius where close[i]."""
    p = S.cloud(n, seed=92, near=0.0)
    close = np.asarray(close, bool)
    p[:, 0] = np.where(close, 0.25, 40.0 + np.arange(n) % 7)
    p[:, 1] = np.where(close, -0.5, p[:, 1])
    p[:, 3] = np.arange(n)
    return p


def test_tiles_and_waves(dev):
    """Everything dropped, nothing dropped, a whole tile dropped between two kept ones, keep / drop alternating across wave and tile
    borders -- with the key frame a whole tile (the sweeps' tiles are the kernel's) and one row (they straddle)."""
    rng = np.random.default_rng(93)
    eye, zero = np.eye(3), np.zeros(3)
    i = np.arange(1100)
    patterns = {"all": np.ones(600, bool), "none": np.zeros(600, bool), "tile": (i[:768] >= 256) & (i[:768] < 512),
                "alternate": i % 2 == 0, "runs": (i // 3) % 2 == 1, "waves": (i // 64) % 2 == 0, "random": rng.random(1100) < 0.5,
                "edges": np.isin(i % 256, [0, 63, 64, 255])}
    names = ["tile", "waves", "all", "none", "alternate", "runs", "random", "edges"]          # P0 = 256: "tile" and "waves" start on a tile
    sweeps = [S.sweep_entry(_tagged(len(patterns[k]), patterns[k]), eye, zero, 0.05 * (j + 1)) for j, k in enumerate(names)]
    for P0 in (256, 1):
        points = S.cloud(P0, seed=94)
        got, want, rows = check(dev, points, sweeps, S.TS, range(len(names)), use_dim=5, remove_close=True)
        assert rows[1:] == [int((~patterns[k]).sum()) for k in names] and rows[1 + names.index("all")] == 0
        at = np.cumsum([0] + rows)
        for j, k in enumerate(names):                                                   # the row order is preserved
            assert got[at[j + 1]:at[j + 2], 3].tolist() == np.flatnonzero(~patterns[k]).astype(F).tolist(), k
        _, buf, cnt, table = device_merge(dev, points, sweeps, S.TS, range(len(names)), use_dim=5, remove_close=True)
        assert int(cnt.item()) == sum(rows) == len(want) and table.total == P0 + sum(len(p) for p in patterns.values())


def test_random_filtering(dev):
    points, sweeps, ts = S.make("filter")
    got, want, rows = check(dev, points, sweeps, ts, [2, 0, 1], remove_close=True)
    assert rows[0] == 256 and rows[2] < 900 and rows[1] < 700 and rows[3] == 0
    plain, _, prow = check(dev, points, sweeps, ts, [2, 0, 1])
    assert prow == [256, 700, 900, 0] and len(plain) > len(got)


# ------------------------------------------------------------------ pad_empty_sweeps, use_dim
@pytest.mark.parametrize("remove_close", [False, True])
def test_pad_empty_sweeps(dev, remove_close):
    points, sweeps, ts = S.make("pad")
    got, want, rows = check(dev, points, sweeps, ts, [], sweeps_num=3, pad_empty_sweeps=True, remove_close=remove_close)
    kept = int(S.not_close(points).sum())
    assert 0 < kept < 517 and rows == [517] + [kept if remove_close else 517] * 3 and not got[:, 3].any()
    assert np.array_equal(got[517:517 + rows[1], :3].view(np.uint32), points[S.not_close(points) | (not remove_close), :3].view(np.uint32))
    cloud, extras = SW.LoadPointsFromMultiSweeps(sweeps_num=3, pad_empty_sweeps=True, remove_close=remove_close, device=dev)(points, sweeps, ts)
    assert S.same(cloud.cpu().numpy(), want) and extras["rows"] == [517] * 4 and int(extras["count"].item()) == len(want)
    assert len(extras["choices"]) == 0 and extras["upload_bytes"] < 517 * 20 + 256 + 4 * 128 + 256             # the key frame goes up once


@pytest.mark.parametrize("name", ["dims5", "dims6"])
@pytest.mark.parametrize("use_dim", [[0, 1, 2, 4], 5, [0, 1, 2, 3, 4], [4, 2, 0], "all"])
def test_use_dim(dev, name, use_dim):
    points, sweeps, ts = S.make(name)
    C = points.shape[1]
    use_dim = list(range(C)) if use_dim == "all" else use_dim
    for rc in (False, True):
        got, want, rows = check(dev, points, sweeps, ts, [1, 0], use_dim=use_dim, remove_close=rc)
        assert got.shape[1] == len(S.columns(use_dim))
        load = SW.LoadPointsFromMultiSweeps(load_dim=C, use_dim=use_dim, remove_close=rc, device=dev)
        cloud, extras = load(points, list(reversed(sweeps)), ts)
        assert S.same(cloud.cpu().numpy(), want) and cloud.is_cuda and int(extras["count"].item()) == len(want)
    if C == 6 and use_dim == list(range(6)):                               # a column past 4 is copied bit for bit
        assert np.array_equal(got[:70, 5].view(np.uint32), points[:, 5].view(np.uint32))


# ------------------------------------------------------------------ out=, count=, determinism, a captured graph
def test_out_and_count_are_written_in_place(dev):
    points, sweeps, ts = S.make("filter")
    total = 256 + 900 + 700
    for rc in (False, True):
        out = torch.full((total, 4), 77.0, device=dev)
        count = torch.full((1,), -5, dtype=torch.int32, device=dev)
        got, buf, cnt, table = device_merge(dev, points, sweeps, ts, [0, 1, 2], out=out, count=count, remove_close=rc)
        want, _ = S.restatement(points, sweeps, ts, [0, 1, 2], remove_close=rc)
        assert buf is out and cnt is count and int(count.item()) == len(want) and S.same(got, want)
        assert (len(want) == total) == (not rc)
        assert (out[len(want):] == 77.0).all()                             # the rows past the count are not written
        again, _, _, _ = device_merge(dev, points, sweeps, ts, [0, 1, 2], remove_close=rc)
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32))          # two runs, the same bits
    with pytest.raises(ValueError, match="out must be"):
        device_merge(dev, points, sweeps, ts, [0, 1, 2], out=torch.empty((total, 5), device=dev))
    with pytest.raises(ValueError, match="count must be"):
        device_merge(dev, points, sweeps, ts, [0, 1, 2], count=torch.empty(1, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="raw must be"):
        SW.merge_sweeps(torch.zeros((5, 5), device=dev), SW.sweep_table(len(points), sweeps, ts, [0]))
    # an output that is not 16-byte aligned takes the store-per-element path
    odd = torch.empty(total * 4 + 1, device=dev)[1:].view(total, 4)
    assert odd.data_ptr() % 16 == 4
    got, _, _, _ = device_merge(dev, points, sweeps, ts, [0, 1, 2], out=odd)
    assert S.same(got, S.restatement(points, sweeps, ts, [0, 1, 2])[0])


def test_captured_graph_replays_on_new_clouds(dev):
    a, b = S.make("graph_a"), S.make("graph_b")
    raw_a, raw_b = (np.concatenate([s[0]] + [sw['points'] for sw in s[1]]) for s in (a, b))
    table = SW.sweep_table(257, a[1], a[2], [0, 1]).to(dev)
    static = torch.from_numpy(raw_a).to(dev)
    out = torch.empty((table.total, 4), device=dev)
    SW.merge_sweeps(static, table, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        SW.merge_sweeps(static, table, out=out)
    static.copy_(torch.from_numpy(raw_b))
    g.replay()
    torch.cuda.synchronize()
    moved = [dict(sb, sensor2lidar_rotation=sa['sensor2lidar_rotation'], sensor2lidar_translation=sa['sensor2lidar_translation'])
             for sa, sb in zip(a[1], b[1])]                                # the captured table holds a's calibration
    assert all(S.tie_free(s['points'][:, :3], s['sensor2lidar_rotation'], s['sensor2lidar_translation']) for s in moved)
    want = S.restatement(b[0], moved, b[2], [0, 1])[0]
    eager = SW.merge_sweeps(torch.from_numpy(raw_b).to(dev), table)[0]
    assert S.same(out.cpu().numpy(), want) and S.same(eager.cpu().numpy(), want)
    assert not S.same(out.cpu().numpy(), S.restatement(a[0], a[1], a[2], [0, 1])[0])


# ------------------------------------------------------------------ the workload's size, the pipeline
_WORK = {}


def workload_reference(rc):
    if rc not in _WORK:
        points, sweeps, ts = S.make("workload")
        want, rows = S.restatement(points, sweeps, ts, range(10), remove_close=rc)
        want.setflags(write=False)
        _WORK[rc] = (want, rows)
    return _WORK[rc]


@pytest.mark.parametrize("remove_close", [False, True])
def test_workload_size(dev, remove_close):
    """11 x 34 720 rows through the loader: raw clouds from the host, one upload."""
    points, sweeps, ts = S.make("workload")
    want, rows = workload_reference(remove_close)
    load = SW.LoadPointsFromMultiSweeps(remove_close=remove_close, device=dev)
    cloud, extras = load(points, sweeps, ts)
    assert cloud.is_cuda and cloud.dtype == torch.float32 and tuple(cloud.shape) == want.shape
    assert S.same(cloud.cpu().numpy(), want) and int(extras["count"].item()) == len(want) == sum(rows)
    assert extras["rows"] == [34720] * 11 and extras["choices"].tolist() == list(range(10))
    assert 11 * 34720 * 20 <= extras["upload_bytes"] <= 11 * 34720 * 20 + 256 + 11 * 128 + 256
    assert (len(want) == 11 * 34720) == (not remove_close)
    again, _ = load(points, sweeps, ts)                                      # the staging buffer is reused
    assert S.same(again.cpu().numpy(), want)


def test_loader_reads_paths_and_bytes(dev, tmp_path):
    points, sweeps, ts = S.make("dims5")
    want = S.restatement(points, sweeps, ts, [0, 1])[0]
    listed = []
    for k, s in enumerate(sweeps):
        e = {key: v for key, v in s.items() if key != 'points'}
        e['data_path'] = str(tmp_path / ("sweep%d.bin" % k))
        s['points'].tofile(e['data_path'])
        listed.append(e)
    load = SW.LoadPointsFromMultiSweeps(device=dev)
    for key in (points.tobytes(), torch.from_numpy(points.copy()), points):
        cloud, _ = load(key, listed, ts)
        assert S.same(cloud.cpu().numpy(), want)


def test_chained_with_voxelisation_and_depth_maps(dev):
    """Voxelization and points_to_depth_maps on the loader's cloud and on the uploaded restatement cloud give identical outputs."""
    import depth_map_refs as D
    import image_input_refs as R
    from co_occ_amd import depth_maps as DM
    from co_occ_amd.lidar import Voxelization
    points, sweeps, ts = S.make("chain")
    for rc in (False, True):
        cloud, _ = SW.LoadPointsFromMultiSweeps(remove_close=rc, device=dev)(points, sweeps, ts)
        want = S.restatement(points, sweeps, ts, [0, 1], remove_close=rc)[0]
        uploaded = torch.from_numpy(want).to(dev)
        vox = Voxelization([0.5, 0.5, 0.5], [-50.0, -50.0, -5.0, 50.0, 50.0, 3.0], 10, 20000).to(dev).eval()
        a, b = vox(cloud), vox(uploaded)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[0].shape[0] > 1000 and int(a[2].max()) > 1
        table = DM.camera_table(*D.rig(R.R50)).to(dev)
        ma, mb = DM.points_to_depth_maps(cloud, table, (256, 704)), DM.points_to_depth_maps(uploaded, table, (256, 704))
        assert torch.equal(ma, mb) and int((ma > 0).sum()) > 1000
