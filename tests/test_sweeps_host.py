"""The multi-sweep loader's host side (co_occ_amd/sweeps.py) and the references the GPU tests lean on (tests/sweep_refs.py): the
restatement against the literal numpy expressions, tie_free against exact rational arithmetic, the table's layout, the choice rules,
every refusal.  No GPU."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import sweep_refs as S
from co_occ_amd import _lib, sweeps as SW
from co_occ_amd._lib import CooccError

F = np.float32


# ------------------------------------------------------------------ the references
@pytest.mark.parametrize("name", sorted(S.SAMPLES))
def test_every_randomised_sample_is_tie_free(name):
    assert S.sample_tie_free(S.make(name))


@pytest.mark.parametrize("name", [n for n in sorted(S.SAMPLES) if n != "workload"])
@pytest.mark.parametrize("remove_close", [False, True])
def test_restatement_is_the_literal_expressions(name, remove_close):
    points, sweeps, ts = S.make(name)
    C = points.shape[1]
    for choices in (np.arange(len(sweeps)), np.arange(len(sweeps))[::-1]):
        for use_dim in ([0, 1, 2, 4], C):
            kw = dict(use_dim=use_dim, remove_close=remove_close, pad_empty_sweeps=name == "pad", sweeps_num=3)
            want = S.literal(points, sweeps, ts, choices, **kw)
            got, rows = S.restatement(points, sweeps, ts, choices, **kw)
            assert want.dtype == F and S.same(got, want) and sum(rows) == len(got)
    assert points[:, 4].any()                                       # the inputs were not written


def test_restatement_is_the_literal_expressions_at_the_workload():
    points, sweeps, ts = S.make("workload")
    choices = np.arange(10)
    for rc in (False, True):
        got, rows = S.restatement(points, sweeps, ts, choices, remove_close=rc)
        assert S.same(got, S.literal(points, sweeps, ts, choices, remove_close=rc))
        assert (sum(rows) == 11 * 34720) == (not rc) and rows[0] == 34720


def test_hand_placed_values_of_the_restatement():
    tiny, big = F(2.0 ** -149), np.finfo(F).max
    R, t = np.eye(3), np.zeros(3)
    assert S.transform(np.array([[tiny, 0, 0]], F), R, t)[0, 0] == tiny                      # a denormal in and out
    assert S.transform(np.array([[2.0 ** -148, 0, 0]], F), R * 0.5, t)[0, 0] == tiny         # a denormal made
    assert np.isinf(S.transform(np.array([[big, 0, 0]], F), R * 2.0, t)[0, 0])               # past FLT_MAX
    out = S.transform(np.array([[np.inf, 1, 2]], F), R, t)[0]
    assert np.isinf(out[0]) and np.isnan(out[1]) and np.isnan(out[2])                        # inf * 0
    # two roundings, not one: 1 + 2^-24 rounds to 1 (even), then + 2^-24 rounds to 1 again; one rounding of 1 + 2^-23 gives 1 + 2^-23
    R2 = np.array([[1.0, 2.0 ** -24, 0], [0, 1, 0], [0, 0, 1]])
    assert S.transform(np.array([[1, 1, 0]], F), R2, np.array([2.0 ** -24, 0, 0]))[0, 0] == F(1.0)
    rows = np.array([[1.0, 0, 0, 0, 0], [np.nextafter(F(1), F(0)), 0.5, 0, 0, 0], [0.5, 2, 0, 0, 0], [np.nan, 0, 0, 0, 0], [-1.0, -1.0, 0, 0, 0],
                     [-0.5, 0.25, 0, 0, 0]], F)
    assert S.not_close(rows).tolist() == [True, False, True, True, True, False]
    r7 = np.array([[F(0.7), 0, 0, 0, 0], [np.nextafter(F(0.7), F(0)), 0, 0, 0, 0]], F)
    assert S.not_close(r7, 0.7).tolist() == [True, False] and float(F(0.7)) < 0.7            # float32(radius), not the double


def exact_margins(xyz_row, R, t):
    """(exact distance of the exactly summed value to the nearest fp32 boundary, the float64-evaluated value's error) per rounding."""
    def boundary(v):                          # exact distance of a Fraction to the nearest fp32 rounding boundary
        a = abs(v)
        e = -126
        if a != 0:
            e = max(-126, a.numerator.bit_length() - a.denominator.bit_length() - 1)
            while Fraction(2) ** (e + 1) <= a:
                e += 1
            while e > -126 and Fraction(2) ** e > a:
                e -= 1
        s = Fraction(2) ** (e - 23)
        w = a / s
        return abs((w - (w.numerator // w.denominator)) - Fraction(1, 2)) * s
    out = []
    x = [Fraction(float(v)) for v in xyz_row]
    for j in range(3):
        v = sum(x[k] * Fraction(float(R[j, k])) for k in range(3))
        out.append((boundary(v), v))
        xf = xyz_row.astype(np.float64)
        rot = F((xf[0] * R[j, 0] + xf[1] * R[j, 1]) + xf[2] * R[j, 2])
        v2 = Fraction(float(rot)) + Fraction(float(t[j]))
        out.append((boundary(v2), v2))
    return out


def test_tie_free_against_exact_arithmetic():
    rng = np.random.default_rng(21)
    xyz = S.cloud(50, seed=22)[:, :3]
    xyz[:4] = [[1, 2, 3], [0, 0, 0], [2.0 ** -149, 0, 0], [1e-30, -1e-30, 5.0]]
    R, t = S.rotation(rng), rng.normal(size=3) * 3.0
    dist, need = S.tie_margins(xyz, R, t)
    for i in range(len(xyz)):
        for c, (exact_dist, exact_v) in enumerate(exact_margins(xyz[i], R, t)):
            # With u one ulp of the largest term (need = 4 u): the float64 value is the exact one plus three product roundings
            # (u / 2 each), the rounding of a sum below 4 terms' size (u) and of one below 8 (2 u): 4.5 u at most
            assert abs(Fraction(float(dist[i, c])) - exact_dist) <= Fraction(float(need[i, c])) * Fraction(9, 8)
    assert S.tie_free(xyz, R, t) == bool((dist > need).all())
    # exact ties and near ties are refused: 1 + 2^-24 is the midpoint of 1 and 1 + 2^-23
    eye, zero = np.eye(3), np.zeros(3)
    R_tie = np.array([[1.0, 2.0 ** -24, 0], [0, 1, 0], [0, 0, 1]])
    assert not S.tie_free(np.array([[1, 1, 0]], F), R_tie, zero)
    assert not S.tie_free(np.array([[1, 1, 0]], F), np.array([[1.0, 2.0 ** -24 + 2.0 ** -52, 0], [0, 1, 0], [0, 0, 1]]), zero)
    assert not S.tie_free(np.array([[1, 0, 0]], F), eye, np.array([2.0 ** -24, 0, 0]))           # the second rounding
    assert S.tie_free(np.array([[1, 1, 0]], F), np.array([[1.0, 2.0 ** -24 + 2.0 ** -40, 0], [0, 1, 0], [0, 0, 1]]), zero)
    assert S.tie_free(np.array([[1, 2, 3], [4, -8, 0.5]], F), eye, np.array([1.0, 2.0, -4.0]))    # small integers: exact in every order
    assert not S.tie_free(np.array([[np.nan, 0, 0]], F), eye, zero) and not S.tie_free(np.array([[np.inf, 0, 0]], F), eye, zero)
    assert S.boundary_distance(np.array([1.0 + 2.0 ** -24]))[0] == 0 and S.boundary_distance(np.array([1.0]))[0] == 2.0 ** -24
    assert S.boundary_distance(np.array([2.0 ** -150]))[0] == 0 and S.boundary_distance(np.array([0.0]))[0] == 2.0 ** -150


# ------------------------------------------------------------------ sweep_table
def test_table_layout():
    points, sweeps, ts = S.make("twelve")
    assert SW.SEG_DTYPE.itemsize == 128 and [SW.SEG_DTYPE.fields[k][1] for k in ("in_row0", "n_rows", "out_row0", "R", "t", "dt", "flags")] == \
        [0, 8, 16, 24, 96, 120, 124]
    choices = [5, 0, 11]
    t = SW.sweep_table(len(points), sweeps, ts, choices, remove_close=True)
    rows = [len(sweeps[c]['points']) for c in choices]
    assert t.rows == [40] + rows and t.total == 40 + sum(rows) == t.in_rows and t.sources == [-1] + choices and t.filtering
    assert t.segs["in_row0"].tolist() == [0, 40, 40 + rows[0], 40 + rows[0] + rows[1]] == t.segs["out_row0"].tolist()
    assert t.segs["flags"].tolist() == [0, 3, 3, 3] and t.segs["dt"][0] == 0 and not t.segs["R"][0].any()
    for k, c in enumerate(choices, start=1):
        assert np.array_equal(t.segs["R"][k].reshape(3, 3), sweeps[c]['sensor2lidar_rotation'])
        assert np.array_equal(t.segs["t"][k], sweeps[c]['sensor2lidar_translation'])
        want = F(ts - sweeps[c]['timestamp'] / 1e6)
        assert t.segs["dt"][k] == want and 0.04 < want < 0.7
    # a lag that fp32 does not hold: the float64 difference, rounded once
    odd = SW.sweep_table(1, [S.sweep_entry(points[:2], np.eye(3), np.zeros(3), 0.1, ts=0.3)], 0.3, [0])
    assert odd.segs["dt"][1] == F(0.3 - (0.3 - 0.1) * 1e6 / 1e6) and float(odd.segs["dt"][1]) != 0.3 - (0.3 - 0.1) * 1e6 / 1e6
    plain = SW.sweep_table(len(points), sweeps, ts, choices)
    assert plain.segs["flags"].tolist() == [0, 1, 1, 1] and not plain.filtering
    # rows given instead of read from 'points'; a transposed (non-contiguous) rotation is laid out row-major
    bare = [dict(s) for s in sweeps]
    for s in bare:
        del s['points']
        s['sensor2lidar_rotation'] = np.asfortranarray(s['sensor2lidar_rotation'])
    again = SW.sweep_table(len(points), bare, ts, choices, sweep_rows=rows, remove_close=True)
    assert again.segs.tobytes() == t.segs.tobytes()
    # pad_empty_sweeps: sweeps_num records that all name the key frame; filtered only with remove_close
    pad = SW.sweep_table(7, [], ts, [], sweeps_num=4, pad_empty_sweeps=True, remove_close=True)
    assert pad.rows == [7] * 5 and pad.in_rows == 7 and pad.total == 35 and pad.segs["in_row0"].tolist() == [0] * 5
    assert pad.segs["out_row0"].tolist() == [0, 7, 14, 21, 28] and pad.segs["flags"].tolist() == [0, 2, 2, 2, 2] and pad.filtering
    pad = SW.sweep_table(7, [], ts, [], sweeps_num=4, pad_empty_sweeps=True)
    assert pad.segs["flags"].tolist() == [0] * 5 and not pad.filtering
    none = SW.sweep_table(7, [], ts, [], remove_close=True)
    assert none.rows == [7] and not none.filtering                     # the key frame alone is never filtered
    some = SW.sweep_table(7, sweeps, ts, [1], pad_empty_sweeps=True)     # sweeps present: pad_empty_sweeps does nothing
    assert some.rows == [7, len(sweeps[1]['points'])]


# ------------------------------------------------------------------ the choice rules
def test_choice_rules():
    assert SW.choose_sweeps(7, 10).tolist() == list(range(7)) and SW.choose_sweeps(10, 10).tolist() == list(range(10))
    assert SW.choose_sweeps(0, 10).tolist() == []
    assert SW.choose_sweeps(12, 10, test_mode=True).tolist() == list(range(10))
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    got, want = SW.choose_sweeps(12, 10, rng=a), b.choice(12, 10, replace=False)
    assert got.tolist() == want.tolist() and got.tolist() != sorted(got.tolist())          # the order drawn is kept
    assert a.randint(1 << 30) == b.randint(1 << 30)                                        # consumed exactly as np.random.choice consumes it
    a = np.random.RandomState(6)
    SW.choose_sweeps(10, 10, rng=a), SW.choose_sweeps(12, 10, test_mode=True, rng=a)       # no draw where none is made
    assert a.randint(1 << 30) == np.random.RandomState(6).randint(1 << 30)
    np.random.seed(7)
    got = SW.choose_sweeps(12, 10)                                                         # the default is np.random itself
    np.random.seed(7)
    assert got.tolist() == np.random.choice(12, 10, replace=False).tolist()
    for n, k, tm in ((12, 10, False), (12, 10, True), (3, 10, False)):
        assert SW.choose_sweeps(n, k, tm, np.random.RandomState(8)).tolist() == S.choose(n, k, tm, np.random.RandomState(8)).tolist()


def test_read_points(tmp_path):
    pts = S.cloud(9, seed=30)
    path = tmp_path / "sweep.bin"
    pts.tofile(path)
    for src in (pts, torch.from_numpy(pts), str(path), path, pts.tobytes(), pts.reshape(-1)):
        got = SW.read_points(src, 5)
        assert got.dtype == F and got.shape == (9, 5) and np.array_equal(got, pts)
    assert SW.read_points(S.cloud(4, seed=31, C=6).tobytes(), 6).shape == (4, 6)


# ------------------------------------------------------------------ refusals
def test_refusals():
    points, sweeps, ts = S.make("dims5")
    with pytest.raises(ValueError, match="load_dim must be 5"):
        SW.LoadPointsFromMultiSweeps(load_dim=4, use_dim=[0, 1, 2])
    with pytest.raises(ValueError, match="outside load_dim = 5"):
        SW.LoadPointsFromMultiSweeps(use_dim=[0, 1, 2, 5])
    with pytest.raises(ValueError, match="outside load_dim = 5"):
        SW.LoadPointsFromMultiSweeps(use_dim=6)
    with pytest.raises(ValueError, match="sweeps_num"):
        SW.LoadPointsFromMultiSweeps(sweeps_num=65)
    for key, bad in (("sensor2lidar_rotation", np.eye(3, dtype=F)), ("sensor2lidar_translation", np.zeros(3, F)),
                     ("sensor2lidar_rotation", np.eye(3).tolist()), ("sensor2lidar_translation", np.zeros(3, np.int64))):
        broken = [dict(s) for s in sweeps]
        broken[1][key] = bad
        with pytest.raises(ValueError, match="sweep 1: %s must be a float64" % key):
            SW.sweep_table(len(points), broken, ts, [0, 1])
        SW.sweep_table(len(points), broken, ts, [0])                       # a sweep that is not chosen is not read
    broken = [dict(s) for s in sweeps]
    broken[0]['sensor2lidar_rotation'] = np.eye(4)
    with pytest.raises(ValueError, match=r"must be \(3, 3\)"):
        SW.sweep_table(len(points), broken, ts, [0])
    with pytest.raises(ValueError, match="outside the 2 sweeps"):
        SW.sweep_table(len(points), sweeps, ts, [2])
    with pytest.raises(ValueError, match="sweep_rows has"):
        SW.sweep_table(len(points), sweeps, ts, [0, 1], sweep_rows=[3])
    with pytest.raises(ValueError, match="2\\^31"):
        SW.sweep_table(1 << 30, sweeps, ts, [0, 1], sweep_rows=[1 << 29, 1 << 29])
    for bad in (points.astype(np.float64), points.astype(np.float16), torch.from_numpy(points.copy()).double()):
        with pytest.raises(ValueError, match="points must be float32"):
            SW.read_points(bad, 5)
    with pytest.raises(ValueError, match=r"sweep 3 must be \[P, 5\]"):
        SW.read_points(np.zeros((4, 6), F), 5, "sweep 3")
    with pytest.raises(ValueError, match=r"must be \[P, 5\]"):
        SW.read_points(np.zeros(7, F).tobytes(), 5)
    # no CPU fallback: the loader, the op and the table's upload
    with pytest.raises(CooccError, match="GPU only"):
        SW.LoadPointsFromMultiSweeps(device="cpu")(points, sweeps, ts)
    table = SW.sweep_table(len(points), sweeps, ts, [0, 1])
    raw = torch.from_numpy(np.concatenate([points] + [s['points'] for s in sweeps]))
    with pytest.raises(CooccError, match="GPU only"):
        SW.merge_sweeps(raw, table)
    with pytest.raises(CooccError, match="GPU only"):
        table.to("cpu")
    with pytest.raises(ValueError, match="raw must be a tensor"):
        SW.merge_sweeps(raw.numpy(), table)


def test_entry_point_refuses_before_launching():
    """The C entry checks the host copy of the table before anything is launched, so this needs no GPU; a total of 2^31 rows is
    refused with COOCC_EINVAL."""
    lib = _lib.load()
    one = ctypes.c_void_p(256)                # a non-null dummy address: validation never dereferences device pointers
    use = (ctypes.c_int * 4)(0, 1, 2, 4)

    def call(segs, in_rows, load_dim=5, use=use, n_use=4, out_rows=1 << 40, count=one, nseg=None, radius=1.0):
        return lib.coocc_sweeps_merge(one, in_rows, load_dim, one, ctypes.c_void_p(segs.ctypes.data), len(segs) if nseg is None else nseg, use, n_use,
                                      radius, one, out_rows, count, one, 1 << 40, None)
    segs = np.zeros(3, SW.SEG_DTYPE)
    segs["n_rows"], segs["out_row0"] = 1 << 30, [0, 1 << 30, 1 << 31]
    assert call(segs, 1 << 30) == -1 and b"2^31" in lib.coocc_last_error()
    assert call(segs[:1], 1 << 31) == -1 and b"in_rows" in lib.coocc_last_error()
    ok = np.zeros(2, SW.SEG_DTYPE)
    ok["n_rows"], ok["in_row0"], ok["out_row0"] = [5, 7], [0, 5], [0, 5]
    for field, value, word in (("in_row0", 6, b"names rows"), ("n_rows", 8, b"names rows"), ("n_rows", -1, b"names rows"),
                               ("out_row0", 4, b"starts at output row"), ("flags", 4, b"flags")):
        bad = ok.copy()
        bad[field][1] = value
        assert call(bad, 12) == -1 and word in lib.coocc_last_error(), field
    assert call(ok, 12, load_dim=4) == -1 and b"load_dim" in lib.coocc_last_error()
    assert call(ok, 12, use=(ctypes.c_int * 4)(0, 1, 2, 5)) == -1 and b"use_dim[3]" in lib.coocc_last_error()
    assert call(ok, 12, n_use=17) == -1 and b"output columns" in lib.coocc_last_error()
    assert call(ok, 12, out_rows=11) == -1 and b"out holds" in lib.coocc_last_error()
    assert call(ok, 12, nseg=66) == -1 and b"nseg" in lib.coocc_last_error()
    assert call(ok, 12, radius=float("nan")) == -1 and b"radius" in lib.coocc_last_error()
    flt = ok.copy()
    flt["flags"][1] = 3
    assert call(flt, 12, count=None) == -1 and b"needs count" in lib.coocc_last_error()
    assert lib.coocc_sweeps_merge_ws(0) == 256 and lib.coocc_sweeps_merge_ws(257) >= 2 * 2 * 4 and \
        lib.coocc_sweeps_merge_ws(11 * 34720) >= 2 * 4 * ((11 * 34720 + 255) // 256)
