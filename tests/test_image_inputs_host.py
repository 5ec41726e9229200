"""Camera img_inputs, the host side (co_occ_amd/image_inputs.py; no GPU): the integer restatement of Pillow's resize against the
fixture and against the installed Pillow, the coefficient tables, the augmentation parameters and matrices, the C ABI's validation."""
import ctypes
import os

import numpy as np
import pytest
import torch

import image_input_refs as R
from conftest import GOLDEN
from co_occ_amd import _lib
from co_occ_amd import image_inputs as II


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLDEN, "image_inputs.npz"))


# ------------------------------------------------------------------ the restatement
def test_restatement_reproduces_the_fixture(fix):
    assert str(fix["pillow_version"])
    names = [str(n) for n in fix["cases"]]
    assert names == R.FIXTURE_CASES and len(names) >= 10
    for name in names:
        Hs, Ws, dims, crop, flip = R.CASES[name]
        assert fix["params_" + name].tolist() == [Hs, Ws, dims[0], dims[1], *crop, int(flip)]
        got = R.canvas(fix["frame_" + name], dims, crop, flip)
        assert np.array_equal(got, fix["canvas_" + name]), name


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("pair", R.SIZE_PAIRS, ids=lambda p: "%dx%d-%dx%d" % (p[0] + p[1]))
def test_restatement_equals_live_pillow(pair, pattern):
    Image = pytest.importorskip("PIL.Image")
    (Hs, Ws), (newH, newW) = pair
    f = R.frame(Hs, Ws, pattern, seed=3)
    assert np.array_equal(R.resize(f, (newW, newH)), np.array(Image.fromarray(f).resize((newW, newH))))


@pytest.mark.parametrize("pair", R.FULL_PAIRS, ids=lambda p: "%dx%d-%dx%d" % (p[0] + p[1]))
def test_restatement_equals_live_pillow_full_size(pair):
    Image = pytest.importorskip("PIL.Image")
    (Hs, Ws), (newH, newW) = pair
    f = R.frame(Hs, Ws, "random", seed=4)
    assert np.array_equal(R.resize(f, (newW, newH)), np.array(Image.fromarray(f).resize((newW, newH))))


def test_crop_and_flip_equal_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    f = R.frame(16, 23, "random", seed=5)
    im = Image.fromarray(f)
    for box in [(3, 2, 19, 14), (-5, 2, 11, 12), (3, -4, 19, 8), (12, 2, 30, 12), (3, 9, 19, 21), (40, 30, 56, 40)]:
        assert np.array_equal(R.crop(f, box), np.array(im.crop(box))), box
    assert not R.crop(f, (40, 30, 56, 40)).any()
    assert np.array_equal(R.flip(f), np.array(im.transpose(method=Image.FLIP_LEFT_RIGHT)))
    assert np.array_equal(f, np.array(im.rotate(0)))


def test_to_imgs_is_a_true_division():
    b = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, 3)
    got = R.to_imgs(b)
    assert got.shape == (1, 3, 16, 16) and got.dtype == torch.float32
    want = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)          # one rounding of the exact quotient
    assert np.array_equal(got[0, 0].reshape(-1).numpy(), want)
    assert not np.array_equal(want, np.arange(256, dtype=np.float32) * np.float32(1.0 / 255.0))      # a reciprocal gives other bits


# ------------------------------------------------------------------ the coefficient tables
AXES = sorted({(a, b) for (hs, ws), (nh, nw) in R.SIZE_PAIRS + R.FULL_PAIRS + [((64, 64), (9, 11))] for a, b in ((hs, nh), (ws, nw))})


@pytest.mark.parametrize("axis", AXES, ids=lambda a: "%d-%d" % a)
def test_coefficient_tables(axis):
    """The package's vectorised tables are the loop restatement's; the taps of every output index sum to 2^22 within the rounding of
    their count (each tap is rounded by at most 1/2); 255 * sum |taps| + 2^21 stays under 2^31, so 32-bit accumulation never wraps;
    first indices and ends never decrease, which is what lets a tile take its source span from its first and last index."""
    a, b = axis
    bounds, taps = II.pillow_coeffs(a, b)
    ref = R.coeffs(a, b)
    assert bounds.shape == (b, 2) and taps.shape == (b, II.tap_count(a, b)) and taps.dtype == np.int32
    for i, (xmin, t) in enumerate(ref):
        assert (int(bounds[i, 0]), int(bounds[i, 1])) == (xmin, len(t))
        assert taps[i, :len(t)].tolist() == t and not taps[i, len(t):].any()
        assert abs(sum(t) - (1 << 22)) <= len(t) / 2.0
        assert 255 * sum(abs(v) for v in t) + (1 << 21) < (1 << 31)
        assert sum(abs(v) for v in t) < 2 << 22
        assert 0 <= xmin and xmin + len(t) <= a and len(t) >= 1
    assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()
    assert II.pillow_coeffs(a, b)[1] is taps          # cached
    with pytest.raises(ValueError):
        taps[0, 0] = 0                                # and read-only


def test_patterns_reach_both_ends_of_the_clamp():
    """The unclamped value of a pass leaves 0..255 on both sides (bicubic's negative lobes) on the 0/255 stripes at the 2.3 downscale
    and on both 0/255 patterns at the upscales: the cases of both test files exercise the clamp, not only the shift.  (The
    checkerboard averages to grey under a downscale and does not.)"""
    for (Hs, Ws), new, patterns in [((37, 53), 23, ["stripes"]), ((20, 31), 64, ["checker", "stripes"]), ((9, 7), 64, ["checker", "stripes"])]:
        for pattern in patterns:
            f = R.frame(Hs, Ws, pattern, seed=20).astype(np.int64)
            raw = np.array([[((1 << 21) + sum(int(f[0, xmin + k, c]) * t for k, t in enumerate(taps))) >> 22
                             for xmin, taps in R.coeffs(Ws, new)] for c in range(2)])
            assert raw.min() < 0 and raw.max() > 255, (Hs, Ws, new, pattern)


def test_tile_spans_fit_the_kernels_lds_at_the_limit():
    """csrc/image_inputs.hip: 16 output rows span at most 160 source rows, 64 output columns at most 544 source columns, at any
    ratio the tap limit admits."""
    for a, b in [(64, 8), (1600, 200), (900, 113), (1600, 704), (900, 396), (7, 64), (257, 33)]:
        assert II.tap_count(a, b) <= II.MAX_TAPS
        bounds = II.pillow_coeffs(a, b)[0].astype(np.int64)
        end = bounds.sum(1)
        for n, cap in ((16, 160), (64, 544)):
            span = [end[min(i + n, b) - 1] - bounds[i, 0] for i in range(b)]
            assert max(span) <= cap
    # the launcher sizes the LDS from the ratio alone: n outputs span less than (n - 1) * scale + 2 * support + 1
    for a, b in AXES + [(64, 8), (1600, 200), (900, 113), (257, 33), (1600, 1543), (900, 1000)]:
        if II.tap_count(a, b) > II.MAX_TAPS:
            continue
        bounds = II.pillow_coeffs(a, b)[0].astype(np.int64)
        end, scale = bounds.sum(1), float(a) / b
        for n in (16, 64):
            span = max(end[min(i + n, b) - 1] - bounds[i, 0] for i in range(b))
            assert span < (n - 1) * scale + 4.0 * max(scale, 1.0) + 1.0
    assert II.tap_count(64, 8) == 33 and II.tap_count(64, 7) > II.MAX_TAPS and II.tap_count(7, 64) == 5


def test_plan_headers_and_refusals():
    plan = II.ResizePlan(37, 53, R.SIX, (14, 17))
    assert plan.N == 6 and plan.header.shape == (6, II.CAM_INTS)
    h = plan.header
    assert h[0, :5].tolist() == [23, 16, 3, 1, 0] and h[1, :5].tolist() == [23, 37, 2, 20, 1]
    assert h[0, 5] == h[1, 5] >= 0 and h[1, 7] == -1 and h[2, 5] == -1 and h[0, 7] == h[2, 7] >= 0          # tables shared per (in, out)
    assert h[3, 5] == -1 and h[3, 7] == -1
    assert h[0, 6] == II.tap_count(53, 23) and h[0, 8] == II.tap_count(37, 16)
    # the table the header points to is the one pillow_coeffs makes
    bounds, taps = II.pillow_coeffs(53, 23)
    t = plan.host[6 * II.CAM_INTS:]
    at = int(h[0, 5])
    assert np.array_equal(t[at:at + 46].reshape(23, 2), bounds) and np.array_equal(t[at + 46:at + 46 + taps.size].reshape(taps.shape), taps)
    with pytest.raises(ValueError, match=r"ratio 64 / 7 = 9\.143"):
        II.ResizePlan(64, 64, [((9, 7), (0, 0, 9, 7), False)], (7, 9))
    with pytest.raises(ValueError, match="output size"):
        II.ResizePlan(37, 53, [((23, 16), (0, 0, 10, 10), False)], (14, 17))
    with pytest.raises(_lib.CooccError):
        plan.resident("cpu")


# ------------------------------------------------------------------ augmentation parameters and matrices
def test_sample_augmentation_anchors():
    assert II.sample_augmentation(R.R50, 900, 1600, False) == (0.44, (704, 396), (0, 140, 704, 396), False, 0)
    assert II.sample_augmentation(R.R101, 900, 1600, False) == (1.0, (1600, 900), (0, 4, 1600, 900), False, 0)
    assert II.sample_augmentation(R.R50, 900, 1600, False, flip=True, scale=0.5) == (0.5, (800, 450), (48, 194, 752, 450), True, 0)
    for cfg in (R.R50, R.R101):
        assert II.sample_augmentation(cfg, 900, 1600, False) == R.augmentation_eval(cfg, 900, 1600)


def test_seeded_training_draw():
    """The draws in the reference's order: resize, crop_h, crop_w, flip (only when data_config['flip']), rotate."""
    for cfg in (R.TRAIN, dict(R.TRAIN, flip=False)):
        rng, hand = np.random.RandomState(7), np.random.RandomState(7)
        for _ in range(3):
            got = II.sample_augmentation(cfg, 900, 1600, True, rng=rng)
            fH, fW = cfg['input_size']
            resize = float(fW) / float(1600) + hand.uniform(*cfg['resize'])
            newW, newH = int(1600 * resize), int(900 * resize)
            crop_h = int((1 - hand.uniform(*cfg['crop_h'])) * newH) - fH
            crop_w = int(hand.uniform(0, max(0, newW - fW)))
            flip = cfg['flip'] and hand.choice([0, 1])
            rotate = hand.uniform(*cfg['rot'])
            assert got == (resize, (newW, newH), (crop_w, crop_h, crop_w + fW, crop_h + fH), flip, rotate)
        assert rng.uniform() == hand.uniform()          # the same number of draws was made


def test_post_transform_and_intrin_nerf():
    rot, tran = II.post_transform(0.44, (0, 140, 704, 396), False, 0)
    assert rot.dtype == torch.float32 and torch.equal(rot, torch.diag(torch.tensor([0.44, 0.44, 1.0])))
    assert torch.equal(tran, torch.tensor([0.0, -140.0, 0.0]))
    rot, tran = II.post_transform(1.0, (0, 4, 1600, 900), False, 0)
    assert torch.equal(rot, torch.eye(3)) and torch.equal(tran, torch.tensor([0.0, -4.0, 0.0]))
    rot, tran = II.post_transform(0.5, (48, 194, 752, 450), True, 0)
    assert torch.equal(rot, torch.diag(torch.tensor([-0.5, 0.5, 1.0]))) and torch.equal(tran, torch.tensor([48.0 + 704.0, -194.0, 0.0]))
    for args in [(0.44, (0, 140, 704, 396), False), (0.5, (48, 194, 752, 450), True), (0.473, (13, 150, 717, 406), True)]:
        got, want = II.post_transform(*args, 0), R.post_matrices(*args)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    K = [[1266.4, 0.0, 816.2], [0.0, 1266.4, 491.5], [0.0, 0.0, 1.0]]
    k = II.intrin_nerf(K, 0.44, (0, 140, 704, 396))
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    assert torch.equal(k[0], torch.stack([f32(1266.4) * 0.44, f32(0.0), f32(816.2) * 0.44]))
    assert torch.equal(k[1], torch.stack([f32(0.0), f32(1266.4) * 0.44, f32(491.5) * 0.44 - 140]))
    assert torch.equal(k[2], f32([0.0, 0.0, 1.0]))
    assert torch.equal(II.intrin_nerf(K, 1.0, (0, 4, 1600, 900)), f32([[1266.4, 0.0, 816.2], [0.0, 1266.4, 487.5], [0.0, 0.0, 1.0]]))


def test_calibration_against_the_restatement():
    infos, l2c = R.synthetic_calibration()
    for name in R.CAMS:
        cal = II.calibration(infos[name], l2c[name])
        d = infos[name]
        c2w = torch.Tensor(R.pose(d['ego2global_rotation'], d['ego2global_translation']) @
                           R.pose(d['sensor2ego_rotation'], d['sensor2ego_translation']))
        s2l = torch.tensor(np.asarray(l2c[name], np.float64)).inverse().float()
        assert torch.equal(cal["cam2world"], c2w) and torch.equal(cal["sensor2lidar"], s2l)
        assert torch.equal(cal["rot"], s2l[:3, :3]) and torch.equal(cal["tran"], s2l[:3, 3])
        assert torch.equal(cal["intrin"], torch.Tensor(d['cam_intrinsic']))
    # a rotation about z by 90 degrees, and a quaternion that is not unit
    m = II.quaternion_rotation_matrix([np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)])
    assert np.allclose(m, [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    assert np.allclose(II.quaternion_rotation_matrix([2.0, 0.0, 0.0, 2.0]), m, atol=1e-15)
    m = II.quaternion_rotation_matrix(infos[R.CAMS[0]]['sensor2ego_rotation'])
    assert np.allclose(m @ m.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(m) - 1) < 1e-14


def test_quaternion_matrix_equals_pyquaternion():
    pyquaternion = pytest.importorskip("pyquaternion")
    g = np.random.default_rng(11)
    for _ in range(20):
        q = g.standard_normal(4)
        q = q / np.linalg.norm(q) * g.choice([1.0, 1.0000001, 3.0])
        assert np.allclose(II.quaternion_rotation_matrix(q), pyquaternion.Quaternion(q).rotation_matrix, rtol=0, atol=1e-15)


def test_with_bda_layout():
    t = lambda *s: torch.zeros(*s)
    imgs = t(6, 3, 4, 5)
    twelve = (imgs, t(6, 3, 3), t(6, 3), t(6, 3, 3), t(6, 3, 3), t(6, 3), t(6, 1), t(6, 4, 4), imgs, t(6, 3, 3), t(6, 4, 4), imgs.shape[-2:])
    out = II.with_bda(twelve, batch=False)
    assert len(out) == 14 and torch.equal(out[6], torch.eye(3)) and out[10] is None and out[13] == imgs.shape[-2:]
    assert out[0] is imgs and out[9] is imgs and out[11] is twelve[9] and out[12] is twelve[10] and out[7] is twelve[6]
    aabb = torch.ones(2, 3)
    out = II.with_bda(twelve, bda_rot=2 * torch.eye(3), aabb=aabb)
    assert tuple(out[0].shape) == (1, 6, 3, 4, 5) and tuple(out[6].shape) == (1, 3, 3) and tuple(out[10].shape) == (1, 2, 3)
    assert [tuple(v.shape) for v in out[1:6]] == [(1, 6, 3, 3), (1, 6, 3), (1, 6, 3, 3), (1, 6, 3, 3), (1, 6, 3)]
    assert out[13][0].tolist() == [4] and out[13][1].tolist() == [5]


# ------------------------------------------------------------------ the C ABI refuses before it launches
def _header(rows):
    h = np.zeros((len(rows), II.CAM_INTS), np.int32)
    for i, r in enumerate(rows):
        h[i, :len(r)] = r
    return h


def test_entry_point_validates_before_launching():
    """Null pointers throughout: a call that got past validation would fault, so every return below is a refusal made before any
    launch -- bad sizes, N = 0, a ratio over the limit, a table that leaves its buffer."""
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    good = _header([(23, 16, 3, 2, 0, 0, 11, 23 * 13, 11)])
    hp = lambda h: ctypes.c_void_p(h.ctypes.data)

    def call(frames=one, ptrs=None, N=1, Hs=37, Ws=53, params=one, host=good, tables=one, ints=10000, fH=12, fW=16, imgs=one):
        return lib.coocc_frames_to_imgs(frames, ptrs, N, Hs, Ws, params, hp(host) if host is not None else None, tables, ints, fH, fW, imgs,
                                        None, None)
    for kw, word in [(dict(N=0), b"N = 0"), (dict(N=-2), b"N = -2"), (dict(Hs=0), b"frame size"), (dict(Ws=-1), b"frame size"),
                     (dict(Hs=40000, Ws=40000), b"frame size"), (dict(fH=0), b"output size"), (dict(fW=0), b"output size"),
                     (dict(frames=None), b"frames / frame_ptrs"), (dict(ptrs=one), b"frames / frame_ptrs"),
                     (dict(params=None), b"null"), (dict(host=None), b"null"), (dict(imgs=None), b"null"),
                     (dict(tables=None), b"table"), (dict(ints=100), b"table"), (dict(ints=-1), b"table_ints"),
                     (dict(host=_header([(0, 16, 0, 0, 0, 0, 11, 0, 11)])), b"resize_dims"),
                     (dict(host=_header([(23, 16, 1 << 25, 0, 0, 0, 11, 0, 11)])), b"crop origin"),
                     (dict(host=_header([(23, 16, 0, 0, 0, -1, 0, 0, 11)])), b"no horizontal table"),
                     (dict(host=_header([(23, 16, 0, 0, 0, 0, 11, -1, 0)])), b"no vertical table"),
                     (dict(host=_header([(23, 16, 0, 0, 0, 0, 34, 0, 11)])), b"taps per index"),
                     (dict(host=_header([(23, 16, 0, 0, 0, 0, 11, 0, 7)])), b"taps per index"),
                     (dict(Hs=64, Ws=64, host=_header([(9, 7, 0, 0, 0, 0, 31, 0, 39)])), b"ratio 64 / 7 = 9.143"),
                     (dict(Hs=64, Ws=64, host=_header([(7, 9, 0, 0, 0, 0, 39, 0, 31)])), b"horizontal ratio 64 / 7")]:
        rc = call(**kw)
        assert rc == -1, kw
        msg = lib.coocc_last_error()
        assert b"frames_to_imgs" in msg and word in msg, (kw, msg)
