"""Host half of the SSIM of the rendered colour maps (``coocc_render_eval_ssim``, ``evaluation.render_ssim``): the float64 judge of
the test tree (tests/render_ssim_ref.py ``ssim64``) against a second, independent float64 form and against values worked out by
hand, the result keys and the dataset accumulator on hand-made blocks, the C-ABI entry point (declared, exported, refusing bad
arguments before any launch) and the detector's opt-in.  No GPU needed."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import render_ssim_ref as S
from co_occ_amd import _lib, evaluation as E


def _maps(N, H, W, seed, offset=0.0):
    g = np.random.default_rng(seed)
    rgbs = (g.random((N, H, W, 3)) * 1.4 - 0.2 + offset).astype(np.float32)
    gt_img = (g.random((N, 3, H, W)) * 1.6 - 0.3 + offset).astype(np.float32)
    return rgbs, gt_img


@pytest.mark.parametrize("shape,offset", [((2, 7, 7), 0.0), ((2, 7, 8), 0.0), ((2, 8, 7), 0.0), ((3, 32, 48), 0.0), ((2, 33, 71), 100.0),
                                          ((1, 256, 704), 0.0)])
def test_the_two_float64_forms_agree(shape, offset):
    """``ssim64`` (49-term window means) and the ``uniform_filter`` form are independent restatements that check each other."""
    rgbs, gt_img = _maps(*shape, seed=sum(shape), offset=offset)
    for R in (2.0, 1.0):
        a, b = S.ssim64(rgbs, gt_img, R), S.ssim64_filter(rgbs, gt_img, R)
        assert a.shape == (shape[0], 3) and a.dtype == np.float64
        assert np.abs(a - b).max() <= 1e-11, (shape, R, np.abs(a - b).max())


def test_the_golden_maps_and_the_fp32_chain(golden):
    g = golden("render_eval")
    a, b = S.ssim64(g["rgbs"], g["gt_img"]), S.ssim64_filter(g["rgbs"], g["gt_img"])
    assert np.abs(a - b).max() <= 1e-11
    s32, mean32 = S.ssim32(g["rgbs"], g["gt_img"])
    assert s32.dtype == np.float32 and s32.shape == (3,) and mean32.dtype == np.float32
    assert np.abs(s32 - a.mean(1)).max() <= 1e-4                      # the fp32 chain is the same quantity
    t32, tmean = S.ssim_torch(torch.from_numpy(g["rgbs"]), torch.from_numpy(g["gt_img"]))
    assert t32.dtype == torch.float32 and np.abs(t32.numpy() - a.mean(1)).max() <= 1e-4 and abs(float(tmean) - float(mean32)) <= 1e-4
    assert np.abs(S.ssim64(g["rgbs"], g["gt_img"], 1.0) - a).max() > 1e-6     # data_range matters


def test_identical_and_constant_images_give_one_and_no_nan():
    rgbs, _ = _maps(2, 12, 19, 5)
    same = np.ascontiguousarray(rgbs.transpose(0, 3, 1, 2))
    for f in (S.ssim64, S.ssim64_filter):
        assert np.abs(f(rgbs, same) - 1).max() <= 1e-12
    const = np.full((2, 9, 11, 3), 0.375, np.float32)
    for f in (S.ssim64, S.ssim64_filter):
        v = f(const, np.ascontiguousarray(const.transpose(0, 3, 1, 2)))
        assert np.isfinite(v).all() and np.abs(v - 1).max() <= 1e-12
        # a constant view against a textured image: zero covariance, finite
        v = f(const, _maps(2, 9, 11, 6)[1])
        assert np.isfinite(v).all()
    zero = np.zeros((1, 7, 7, 3), np.float32)
    assert np.array_equal(S.ssim64(zero, zero.transpose(0, 3, 1, 2)), np.ones((1, 3)))


def test_single_window_by_hand():
    """A 7 x 7 image has one window: S from the formula with plain Python floats over the 49 pixels."""
    rgbs, gt_img = _maps(1, 7, 7, 11)
    got = S.ssim64(rgbs, gt_img)
    for R in (2.0, 1.0):
        for c in range(3):
            xs = [float(rgbs[0, i, j, c]) for i in range(7) for j in range(7)]
            ys = [float(gt_img[0, c, i, j]) for i in range(7) for j in range(7)]
            ux, uy = sum(xs) / 49, sum(ys) / 49
            uxx, uyy, uxy = sum(a * a for a in xs) / 49, sum(b * b for b in ys) / 49, sum(a * b for a, b in zip(xs, ys)) / 49
            vx, vy, vxy = 49 / 48 * (uxx - ux * ux), 49 / 48 * (uyy - uy * uy), 49 / 48 * (uxy - ux * uy)
            C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
            want = (2 * ux * uy + C1) * (2 * vxy + C2) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
            assert abs(S.ssim64(rgbs, gt_img, R)[0, c] - want) <= 1e-13, (R, c)
    assert abs(S.ssim32(rgbs, gt_img)[0][0] - got.mean()) <= 1e-5


def _hand_block(N=3):
    block = np.zeros((N, E.RENDER_SSIM_SLOTS))
    ch = np.array([[0.25, 0.5, 0.625], [0.1, 0.2, 0.30000000000000004], [1.0, 1.0, 1.0]])[:N]
    block[:, E.RS_C0:E.RS_C2 + 1] = ch
    block[:, E.RS_SSIM] = S.view_ssim(ch)
    block[:, E.RS_SSIM_MEAN] = np.float32(S.view_ssim(ch).sum(dtype=np.float32) / np.float32(N))
    block[:, E.RS_COUNT], block[:, E.RS_RANGE] = 26 * 42, 2.0
    return block, ch


def test_result_keys_of_an_ssim_block():
    assert (E.RS_C0, E.RS_C1, E.RS_C2, E.RS_SSIM, E.RS_SSIM_MEAN, E.RS_COUNT, E.RS_RANGE) == tuple(range(7)) and E.RENDER_SSIM_SLOTS == 8
    block, ch = _hand_block()
    for b in (block, torch.from_numpy(block)):
        k = E.render_ssim_keys(b)
        assert set(k) == {"ssim", "ssim_mean", "ssim_channels"}
        as_np = {n: (v.numpy() if torch.is_tensor(v) else v) for n, v in k.items()}
        assert as_np["ssim"].dtype == np.float32 and np.array_equal(as_np["ssim"], S.view_ssim(ch))
        assert as_np["ssim_mean"].dtype == np.float32 and as_np["ssim_mean"].shape == () and as_np["ssim_mean"] == block[0, E.RS_SSIM_MEAN]
        assert as_np["ssim_channels"].dtype == np.float64 and np.array_equal(as_np["ssim_channels"], ch)


def test_evaluator_summary_with_and_without_ssim():
    block, ch = _hand_block()
    ev = E.RenderEvaluator(device="cpu")
    today = {"psnr_mean", "views", "depth_sq_err", "depth_valid", "depth_mse", "depth_rmse"}
    assert set(ev.summary()) == today
    stats = np.zeros((3, E.RENDER_EVAL_SLOTS))
    stats[:, E.RE_PSNR] = [20.0, 21.0, 22.0]
    ev.add(stats)
    assert set(ev.summary()) == today                                  # no SSIM block yet: today's keys, unchanged
    ev.add_ssim(block)
    ev.add_ssim(torch.from_numpy(block[:2]))
    s = ev.summary()
    assert set(s) == today | {"ssim_mean"}
    want = (S.view_ssim(ch).astype(np.float64).sum() + S.view_ssim(ch)[:2].astype(np.float64).sum()) / 5
    assert abs(s["ssim_mean"] - want) <= 1e-15 and s["views"] == 3 and abs(s["psnr_mean"] - 21.0) <= 1e-12


def test_entry_point_is_declared_and_exported():
    """Fails without the feature: the symbol is absent from the ctypes table, the header and the library."""
    src = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "coocc_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert "coocc_render_eval_ssim" in _lib.SIGNATURES
    assert "int64_t coocc_render_eval_ssim(" in src
    assert hasattr(lib, "coocc_render_eval_ssim"), "missing export"
    assert _lib.load().coocc_abi_version() == 1                       # additive: the ABI version stays


def test_entry_point_refuses_bad_arguments_before_launching():
    lib = _lib.load()
    fn = lib.coocc_render_eval_ssim
    one = ctypes.c_void_p(16)              # a non-null, 16-byte aligned dummy address: validation never dereferences device pointers

    def ss(rgbs=one, gt=one, N=6, H=32, W=48, R=2.0, block=one, ws=one, ws_bytes=1 << 20):
        return fn(rgbs, gt, N, H, W, R, block, ws, ws_bytes, None)
    for kw, word in ((dict(H=6), b"H"), (dict(W=6), b"W"), (dict(N=0), b"N"), (dict(N=65536), b"N"), (dict(R=0.0), b"data_range"),
                     (dict(R=-1.0), b"data_range"), (dict(R=float("inf")), b"data_range"), (dict(R=float("nan")), b"data_range"),
                     (dict(rgbs=None), b"null"), (dict(gt=None), b"null"), (dict(block=None), b"null")):
        assert ss(**kw) == -1, kw
        assert b"render_eval_ssim" in lib.coocc_last_error() and word in lib.coocc_last_error(), (kw, lib.coocc_last_error())
    # ws == NULL: the workspace bytes, nothing launched; a workspace smaller than that is refused with COOCC_ENOMEM
    need = ss(ws=None, ws_bytes=0)
    assert need > 0 and need % 8 == 0
    assert ss(rgbs=ctypes.c_void_p(20), gt=ctypes.c_void_p(4), ws=None) == need       # the size does not depend on the addresses
    assert ss(N=6, H=896, W=1600, ws=None) > need
    assert ss(N=0, ws=None) == -1 and ss(H=6, ws=None) == -1
    assert ss(ws_bytes=need - 8) == -3
    assert b"render_eval_ssim" in lib.coocc_last_error() and b"workspace" in lib.coocc_last_error()


def test_python_surface_refuses_cpu_tensors_and_bad_shapes(golden):
    g = golden("render_eval")
    rgbs, depths, gt_img = (torch.from_numpy(g[k]) for k in ("rgbs", "depths", "gt_img"))
    with pytest.raises(RuntimeError, match="HIP device only"):
        E.render_ssim(rgbs, gt_img)
    with pytest.raises(RuntimeError, match="HIP device only"):
        E.render_eval(rgbs, depths, gt_img, ssim=True)
    with pytest.raises(ValueError) as e:
        E.render_ssim(rgbs, gt_img[:, :, :16])
    assert "(3, 3, 16, 48)" in str(e.value) and "(3, 32, 48, 3)" in str(e.value)
    with pytest.raises(ValueError, match=r"\[N, H, W, 3\]"):
        E.render_ssim(rgbs[..., :2], gt_img)
    with pytest.raises(ValueError, match="7 x 7"):
        E.render_ssim(rgbs[:, :6], gt_img[:, :, :6])
    with pytest.raises(TypeError, match="not a tensor"):
        E.render_ssim(g["rgbs"], gt_img)
    with pytest.raises(ValueError, match="ssim needs rgbs"):
        E.render_eval(None, depths, None, ssim=True)
    p = inspect.signature(E.render_ssim).parameters
    assert p["data_range"].default == 2.0 and p["out"].default is None
    p = inspect.signature(E.render_eval).parameters
    assert p["ssim"].default is False and p["data_range"].default == 2.0


def test_detector_opt_in_defaults_to_off():
    from co_occ_amd.detector import COOCC_Ray, COOCC_Ray_L
    assert inspect.signature(COOCC_Ray.__init__).parameters["render_ssim"].default is False
    assert inspect.signature(COOCC_Ray_L.__init__).parameters["render_ssim"].default is False
    # off, without render_eval, without colour maps or without an image: nothing is launched
    m = COOCC_Ray.__new__(COOCC_Ray)
    maps = dict(rgbs=torch.zeros(1, 8, 8, 3), depths=torch.zeros(1, 8, 8))
    img = torch.zeros(1, 3, 8, 8)
    for render_eval, render_ssim, out, gi in ((True, False, maps, img), (False, True, maps, img), (True, True, dict(maps, rgbs=None), img),
                                              (True, True, maps, None)):
        object.__setattr__(m, "render_eval", render_eval)
        object.__setattr__(m, "render_ssim", render_ssim)
        assert m._render_ssim_launch(out, gi) is None
    block, ch = _hand_block()
    k = COOCC_Ray._render_ssim_finish(block)
    assert set(k) == {"ssim", "ssim_mean"} and np.array_equal(k["ssim"], S.view_ssim(ch))
