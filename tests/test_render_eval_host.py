"""Host half of the render evaluation (PSNR, depth error, comparison panels of ``test_rendering``): the torch restatement of the
test tree (tests/render_eval_ref.py) against the fixture made by the unmodified reference (tools/gen_golden_render_eval.py ->
tests/golden/render_eval.npz), the two C-ABI entry points (declared, exported, refusing bad arguments before any launch) and the
Python surface's refusals.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import render_eval_ref as R
from co_occ_amd import _lib, apis, evaluation as E


def _maps(g):
    return tuple(torch.from_numpy(g[k]) for k in ("rgbs", "depths", "gt_img", "gt_depth"))


def test_fixture_covers_the_constant_depth_view_and_the_clip(golden):
    g = golden("render_eval")
    assert g["rgbs"].shape == (3, 32, 48, 3) and g["gt_img"].shape == (3, 3, 32, 48) and g["panels"].shape == (3, 32, 144, 3)
    assert g["panels"].dtype == np.uint8 and g["psnr"].dtype == np.float32
    assert g["depth_min"][1] == g["depth_max"][1]                     # dmax == dmin: the 1e-8 path
    assert (g["panels"][1][:, 96:] == 0).all()
    assert (g["rgbs"] > 1).any() and (g["rgbs"] < 0).any() and (g["gt_img"] > 1).any() and (g["gt_img"] < 0).any()
    assert (g["depths"][2] < 0).any() and (g["gt_depth"] == 0).any()


def test_restatement_reproduces_the_reference_panels_byte_for_byte(golden):
    g = golden("render_eval")
    rgbs, depths, gt_img, _ = _maps(g)
    got = R.panels(rgbs, depths, gt_img).numpy()
    assert got.dtype == np.uint8 and got.shape == g["panels"].shape
    assert np.array_equal(got, g["panels"])


def test_restatement_reproduces_the_reference_psnr_within_one_ulp(golden):
    g = golden("render_eval")
    rgbs, depths, gt_img, gt_depth = _maps(g)
    p, mean = R.psnr(rgbs, gt_img)
    assert p.dtype == torch.float32 and mean.dtype == torch.float32
    assert R.ulps(p.numpy(), g["psnr"]) <= 1, (p.numpy(), g["psnr"])
    assert R.ulps(mean.numpy(), g["psnr_mean"]) <= 1
    assert np.abs(R.psnr64(rgbs, gt_img).numpy() - g["psnr64"]).max() <= 1e-12
    sq, nv = R.depth_error(depths, gt_depth)
    assert np.array_equal(nv.numpy(), g["depth_valid"])
    assert np.abs(sq.numpy() / g["depth_sq_err64"] - 1).max() <= 1e-14
    assert np.array_equal(depths.flatten(1).min(1).values.numpy(), g["depth_min"])
    assert np.array_equal(depths.flatten(1).max(1).values.numpy(), g["depth_max"])


def test_render_eval_entry_points_are_declared_and_exported():
    """Fails without the feature: the symbols are absent from the ctypes table, the header and the library."""
    src = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "coocc_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, decl in (("coocc_render_eval_stats", "int64_t coocc_render_eval_stats("), ("coocc_render_panels", "int coocc_render_panels(")):
        assert name in _lib.SIGNATURES
        assert decl in src
        assert hasattr(lib, name), "missing export " + name
    assert _lib.load().coocc_abi_version() == 1                       # additive: the ABI version stays


def test_render_eval_entry_points_refuse_bad_arguments_before_launching():
    lib = _lib.load()
    stats, panels = lib.coocc_render_eval_stats, lib.coocc_render_panels
    one = ctypes.c_void_p(16)              # a non-null, 16-byte aligned dummy address: validation never dereferences device pointers

    def st(rgbs=one, depths=one, gt=one, gtd=None, N=6, H=32, W=48, block=one, ws=one, ws_bytes=1 << 20):
        return stats(rgbs, depths, gt, gtd, N, H, W, block, ws, ws_bytes, None)
    for kw, word in ((dict(N=0), b"N"), (dict(H=0), b"H * W"), (dict(W=0), b"H * W"), (dict(depths=None), b"null"),
                     (dict(block=None), b"null"), (dict(rgbs=None), b"both or neither"), (dict(gt=None), b"both or neither")):
        assert st(**kw) == -1, kw
        assert b"render_eval_stats" in lib.coocc_last_error() and word in lib.coocc_last_error(), (kw, lib.coocc_last_error())
    # ws == NULL: the workspace bytes, nothing launched; a workspace smaller than that is refused with COOCC_ENOMEM
    need = st(ws=None, ws_bytes=0)
    assert need > 0 and need % 8 == 0
    assert st(N=6, H=896, W=1600, ws=None) >= need
    assert st(N=0, ws=None) == -1
    assert st(ws_bytes=need - 8) == -3 and b"workspace" in lib.coocc_last_error()

    def pn(rgbs=one, depths=one, gt=one, block=one, N=6, H=32, W=48, out=one):
        return panels(rgbs, depths, gt, block, N, H, W, out, None)
    for kw, word in ((dict(N=0), b"N"), (dict(H=0), b"H * W"), (dict(block=None), b"stats block"), (dict(rgbs=None), b"null"),
                     (dict(depths=None), b"null"), (dict(gt=None), b"null"), (dict(out=None), b"null")):
        assert pn(**kw) == -1, kw
        assert b"render_panels" in lib.coocc_last_error() and word in lib.coocc_last_error(), (kw, lib.coocc_last_error())


def test_render_eval_refuses_cpu_tensors_and_mismatched_shapes(golden):
    g = golden("render_eval")
    rgbs, depths, gt_img, gt_depth = _maps(g)
    with pytest.raises(RuntimeError, match="HIP device only"):
        E.render_eval(rgbs, depths, gt_img)
    with pytest.raises(RuntimeError, match="HIP device only"):
        E.render_eval(rgbs, depths, gt_img, gt_depth, panels=True)
    # the maps are 16 fH x 16 fW and must equal the image size: the message names both shapes
    small = gt_img[:, :, :16]
    with pytest.raises(ValueError) as e:
        E.render_eval(rgbs, depths, small)
    assert "(3, 3, 16, 48)" in str(e.value) and "(3, 32, 48, 3)" in str(e.value)
    with pytest.raises(ValueError) as e:
        E.render_eval(rgbs, depths[:, :, :40], gt_img)
    assert "(3, 32, 40)" in str(e.value) and "(3, 32, 48, 3)" in str(e.value)
    with pytest.raises(ValueError) as e:
        E.render_eval(rgbs, depths, gt_img, gt_depth[:2])
    assert "(2, 32, 48)" in str(e.value) and "(3, 32, 48)" in str(e.value)
    with pytest.raises(ValueError, match="together"):
        E.render_eval(rgbs, depths, None)
    with pytest.raises(ValueError, match="gt_img"):
        apis.save_rendered_panels(dict(rgbs=rgbs, depths=depths), "unused")


def test_result_keys_of_a_stats_block_and_the_dataset_accumulator(golden):
    """The host halves: a stats block (as the kernel lays it out) -> the result keys; RenderEvaluator sums blocks and reads back once."""
    g = golden("render_eval")
    N = 3
    block = np.zeros((N, E.RENDER_EVAL_SLOTS))
    block[:, E.RE_SQ_RGB], block[:, E.RE_DMIN], block[:, E.RE_DMAX] = g["sq_rgb64"], g["depth_min"], g["depth_max"]
    block[:, E.RE_SQ_DEPTH], block[:, E.RE_NVALID] = g["depth_sq_err64"], g["depth_valid"]
    block[:, E.RE_PSNR], block[:, E.RE_PSNR_MEAN] = g["psnr"], g["psnr_mean"]
    for b in (block, torch.from_numpy(block)):
        k = E.render_eval_keys(b, with_rgb=True, with_depth=True)
        assert set(k) == {"psnr", "psnr_mean", "depth_min", "depth_max", "depth_sq_err", "depth_valid"}
        as_np = {n: (v.numpy() if torch.is_tensor(v) else v) for n, v in k.items()}
        assert as_np["psnr"].dtype == np.float32 and np.array_equal(as_np["psnr"], g["psnr"])
        assert as_np["psnr_mean"].dtype == np.float32 and as_np["psnr_mean"] == g["psnr_mean"]
        assert as_np["depth_valid"].dtype == np.int64 and np.array_equal(as_np["depth_valid"], g["depth_valid"])
        assert np.array_equal(as_np["depth_sq_err"], g["depth_sq_err64"]) and np.array_equal(as_np["depth_min"], g["depth_min"])
        assert set(E.render_eval_keys(b, with_rgb=False, with_depth=True, extrema=False)) == {"depth_sq_err", "depth_valid"}
    ev = E.RenderEvaluator(device="cpu")
    ev.add(block)
    ev.add(torch.from_numpy(block[:2]))
    s = ev.summary()
    assert s["views"] == 5
    assert abs(s["psnr_mean"] - (g["psnr"].astype(np.float64).sum() + g["psnr"][:2].astype(np.float64).sum()) / 5) <= 1e-12
    nv = int(g["depth_valid"].sum() + g["depth_valid"][:2].sum())
    assert s["depth_valid"] == nv
    assert abs(s["depth_mse"] - (g["depth_sq_err64"].sum() + g["depth_sq_err64"][:2].sum()) / nv) <= 1e-9
    assert np.isnan(E.RenderEvaluator(device="cpu").summary()["psnr_mean"])


def test_detector_opt_in_defaults_to_off():
    from co_occ_amd.detector import COOCC_Ray, COOCC_Ray_L
    import inspect
    assert inspect.signature(COOCC_Ray.__init__).parameters["render_eval"].default is False
    img = torch.zeros(1, 6, 3, 4, 8)
    assert COOCC_Ray.render_gt_img((img, None), None).shape == (6, 3, 4, 8)
    views = img[0]
    assert COOCC_Ray.render_gt_img(None, dict(gt_img=views)) is views and COOCC_Ray.render_gt_img(None, None) is None
    assert COOCC_Ray.render_gt_img((None, 1), dict(gt_img=views)) is views
    # the depth ground truth: a tensor, or the dataset's tuple at DEPTH_GT_INDEX; only a map of the maps' size is taken
    depths = torch.zeros(6, 4, 8)
    pick = COOCC_Ray_L._render_gt_depth
    self_l = COOCC_Ray_L.__new__(COOCC_Ray_L)
    assert pick(self_l, torch.ones(1, 6, 4, 8), depths).shape == (6, 4, 8)
    assert pick(self_l, [0, torch.ones(1, 6, 4, 8), 0], depths).shape == (6, 4, 8)        # gt_depths[-2]
    assert pick(self_l, torch.ones(6, 2, 8), depths) is None and pick(self_l, None, depths) is None
    assert pick(self_l, [torch.ones(6, 4, 8)], depths) is None
