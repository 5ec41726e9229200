"""Camera img_inputs on the device (co_occ_amd/image_inputs.py, csrc/image_inputs.hip): everything bit for bit against the numpy
integer restatement of Pillow run on the CPU (tests/image_input_refs.py) and, where a case is in it, the Pillow-made fixture.
The kernel's output tile is 16 rows x 64 columns."""
import os

import numpy as np
import pytest
import torch

import co_occ_amd as pkg
import image_input_refs as R
from conftest import GOLDEN
from co_occ_amd import core, image_inputs as II, synth
from co_occ_amd._lib import CooccError

pytestmark = pytest.mark.gpu


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def device_run(dev, frames, cams, out_size, as_list=False):
    """frames: uint8 numpy [N,Hs,Ws,3] -> (imgs, canvas) CPU tensors made by the kernel."""
    N, Hs, Ws = frames.shape[:3]
    plan = II.ResizePlan(Hs, Ws, cams, out_size, device=dev)
    f = torch.from_numpy(frames).to(dev)
    if as_list:
        f = [f[i].clone() for i in range(N)]
    canvas = torch.full((N, out_size[0], out_size[1], 3), 77, dtype=torch.uint8, device=dev)
    imgs = II.frames_to_imgs(f, plan, canvas=canvas)
    assert imgs.dtype == torch.float32 and tuple(imgs.shape) == (N, 3) + tuple(out_size)
    return imgs.cpu(), canvas.cpu()


def expect(frames, cams):
    cv = np.stack([R.canvas(f, dims, box, fl) for f, (dims, box, fl) in zip(frames, cams)])
    return R.to_imgs(cv), torch.from_numpy(cv)


def check(dev, frames, cams, out_size, **kw):
    imgs, canvas = device_run(dev, frames, cams, out_size, **kw)
    want_imgs, want_canvas = expect(frames, cams)
    assert torch.equal(canvas, want_canvas), "canvas bytes differ at %d places" % int((canvas != want_canvas).sum())
    assert bits_equal(imgs, want_imgs)
    return imgs, canvas


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLDEN, "image_inputs.npz"))


@pytest.fixture(scope="module")
def full_frames():
    return np.stack([R.frame(900, 1600, "random", seed=40 + i) for i in range(6)])


_FULL = {}


def full_reference(cfg_name, frames):
    """The 14-tuple and canvas of a config on the six full-size frames: made once, shared, never changed."""
    if cfg_name not in _FULL:
        infos, l2c = R.synthetic_calibration()
        _FULL[cfg_name] = R.img_inputs14(getattr(R, cfg_name), frames, infos, l2c) + (infos, l2c)
    return _FULL[cfg_name]


# ------------------------------------------------------------------ the small cases
@pytest.mark.parametrize("name", list(R.CASES))
def test_case_equals_the_restatement(dev, name, fix):
    """Both passes at a non-integer ratio, each pass alone, upscales (the filter scale clamps at 1, the first and last index clamp at
    the borders), a strong downscale, 5x5 -> 1x1, the unresized form, crop boxes that leave the image on each side and wholly, flips
    (odd width; of a crop that reaches outside: the zero band is mirrored too), 159-byte and 192-byte source rows, outputs one less,
    equal to, one more than and twice-plus-one the tile -- on random bytes, a checkerboard and stripes."""
    Hs, Ws, dims, box, fl = R.CASES[name]
    out_size = (box[3] - box[1], box[2] - box[0])
    for i, pattern in enumerate(R.PATTERNS):
        _, canvas = check(dev, R.frame(Hs, Ws, pattern, seed=20 + i)[None], [(dims, box, fl)], out_size)
        if name == "out_wholly":
            assert not canvas.any()
    if name in R.FIXTURE_CASES:
        _, canvas = device_run(dev, fix["frame_" + name][None], [(dims, box, fl)], out_size)
        assert np.array_equal(canvas[0].numpy(), fix["canvas_" + name])


def test_a_ratio_past_the_limit_is_refused(dev):
    check(dev, R.frame(64, 64, "random", 1)[None], [((8, 8), (0, 0, 8, 8), False)], (8, 8))          # ratio 8: the limit itself
    with pytest.raises(ValueError, match=r"ratio 64 / 7 = 9\.143"):
        II.ResizePlan(64, 64, [((9, 7), (0, 0, 9, 7), False)], (7, 9), device=dev)


def test_six_cameras_six_parameter_sets(dev):
    frames = np.stack([R.frame(37, 53, R.PATTERNS[i % 3], seed=30 + i) for i in range(6)])
    a, _ = check(dev, frames, R.SIX, (14, 17))
    b, _ = check(dev, frames, R.SIX, (14, 17), as_list=True)
    assert bits_equal(a, b)
    for i in (0, 3, 5):
        one, _ = check(dev, frames[i:i + 1], R.SIX[i:i + 1], (14, 17))
        assert bits_equal(one[0], a[i])


def test_full_size_r50(dev, full_frames):
    want = full_reference("R50", full_frames)
    cams = [((704, 396), (0, 140, 704, 396), False)] * 2
    imgs, canvas = device_run(dev, full_frames[:2], cams, (256, 704))
    assert np.array_equal(canvas.numpy(), want[1][:2]) and bits_equal(imgs, want[0][0][:2])


def test_full_size_r101(dev, full_frames):
    want = full_reference("R101", full_frames)
    imgs, canvas = device_run(dev, full_frames[:1], [((1600, 900), (0, 4, 1600, 900), False)], (896, 1600))
    assert np.array_equal(canvas.numpy(), want[1][:1]) and bits_equal(imgs, want[0][0][:1])
    assert np.array_equal(canvas.numpy()[0], full_frames[0, 4:])


def test_imgs_is_canvas_over_255_and_out_is_written_in_place(dev):
    frames = np.stack([R.frame(40, 150, "random", seed=50 + i) for i in range(2)])
    cams = [((70, 19), (2, 1, 67, 18), False), ((70, 19), (3, 2, 68, 19), True)]
    plan = II.ResizePlan(40, 150, cams, (17, 65), device=dev)
    f = torch.from_numpy(frames).to(dev)
    out = torch.full((2, 3, 17, 65), -1.0, device=dev)
    canvas = torch.zeros((2, 17, 65, 3), dtype=torch.uint8, device=dev)
    got = II.frames_to_imgs(f, plan, out=out, canvas=canvas)
    assert got is out
    assert bits_equal(out.cpu(), canvas.cpu().float().permute(0, 3, 1, 2).contiguous() / 255.)
    again = II.frames_to_imgs(f, plan)          # determinism, and no canvas asked for
    assert again.data_ptr() != out.data_ptr() and bits_equal(again.cpu(), out.cpu())
    with pytest.raises(ValueError):
        II.frames_to_imgs(f, plan, out=torch.empty((2, 3, 17, 64), device=dev))


def test_captured_graph_replays_on_new_bytes(dev):
    Hs, Ws, dims, box, fl = R.CASES["tile_129x33"]
    out_size = (box[3] - box[1], box[2] - box[0])
    plan = II.ResizePlan(Hs, Ws, [(dims, box, fl)] * 2, out_size, device=dev)
    a = torch.from_numpy(np.stack([R.frame(Hs, Ws, "random", 60), R.frame(Hs, Ws, "checker", 61)])).to(dev)
    b = torch.from_numpy(np.stack([R.frame(Hs, Ws, "stripes", 62), R.frame(Hs, Ws, "random", 63)])).to(dev)
    static = a.clone()
    out = torch.empty((2, 3) + out_size, device=dev)
    canvas = torch.empty((2,) + out_size + (3,), dtype=torch.uint8, device=dev)
    II.frames_to_imgs(static, plan, out=out, canvas=canvas)          # tables resident before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        II.frames_to_imgs(static, plan, out=out, canvas=canvas)
    static.copy_(b)
    g.replay()
    torch.cuda.synchronize()
    eager_canvas = torch.empty_like(canvas)
    eager = II.frames_to_imgs(b, plan, canvas=eager_canvas)
    assert bits_equal(out.cpu(), eager.cpu()) and torch.equal(canvas.cpu(), eager_canvas.cpu())
    assert not torch.equal(canvas.cpu(), expect(a.cpu().numpy(), [(dims, box, fl)] * 2)[1])


# ------------------------------------------------------------------ the loader
def _elements_equal(got, want):
    assert len(got) == len(want) == 14
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, torch.Tensor):
            assert g.is_cuda and g.dtype == w.dtype, i
            assert bits_equal(g.cpu(), w) if w.dtype == torch.float32 else torch.equal(g.cpu(), w), "element %d differs" % i
        else:
            assert g == w, i


@pytest.mark.parametrize("cfg_name", ["R50", "R101"])
def test_the_whole_tuple_for_a_config(dev, cfg_name, full_frames):
    want14, want_canvas, infos, l2c = full_reference(cfg_name, full_frames)
    cfg = getattr(R, cfg_name)
    load = II.LoadMultiViewFrames(cfg, is_train=False, device=dev)
    twelve, extras = load(list(full_frames), infos, l2c)          # host frames: uploaded as bytes
    assert len(twelve) == 12 and twelve[8].data_ptr() == twelve[0].data_ptr()          # denorm_imgs shares imgs' storage
    assert tuple(twelve[6].shape) == (6, 1) and not twelve[6].any()
    _elements_equal(II.with_bda(twelve, batch=False), want14)
    assert np.array_equal(extras["canvas"].cpu().numpy(), want_canvas) and list(extras["cam_names"]) == R.CAMS
    assert extras["params"][0]["crop"] == R.augmentation_eval(cfg, 900, 1600)[2]
    batched = II.with_bda(twelve)
    assert tuple(batched[0].shape) == (1, 6, 3) + cfg['input_size'] and tuple(batched[6].shape) == (1, 3, 3)
    assert [int(v) for v in batched[13]] == list(cfg['input_size'])
    # a fixed rig in eval mode: the same plan, nothing uploaded again; device frames give the same bits
    again, extras2 = load(torch.from_numpy(full_frames).to(dev), infos, l2c)
    assert extras2["plan"] is extras["plan"] and bits_equal(again[0].cpu(), want14[0])


def test_detector_encodes_device_made_images(dev):
    """A small hip_image_encoder=True detector (as test_gpu_image_encoder.test_detector_encodes_raw_images): its image_encoder on the
    device-made imgs gives the bits it gives on the CPU-made tensor uploaded."""
    import ref_image_encoder as RE
    oc = [16, 16, 16, 16]
    bcfg = dict(type='ResNet', depth=50, stem_channels=64, base_channels=16, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=0,
                norm_cfg=dict(type='BN', requires_grad=True), norm_eval=False, style='pytorch', pretrained='ckpts/none.pth')
    ncfg = dict(type='SECONDFPN', in_channels=[64, 128, 256, 512], upsample_strides=[0.25, 0.5, 1, 2], out_channels=oc)
    cfg = synth.model_cfg(C=32, block_inplanes=(32, 64, 128, 256), out_channels=32, rendering=False)
    cfg["img_view_transformer"] = dict(
        type='ViewTransformerLiftSplatShootVoxel', numC_input=sum(oc), numC_Trans=16, downsample=16, depth_net='hip',
        grid_config={'xbound': [-8., 8., 2.], 'ybound': [-8., 8., 2.], 'zbound': [-2., 2., 2.], 'dbound': [2.0, 10.0, 1.0]},
        data_config={'input_size': (64, 96)})
    torch.manual_seed(8)
    det = pkg.build_detector(cfg, img_backbone=bcfg, img_neck=ncfg, hip_image_encoder=True, external_encoders=True)
    det.img_backbone.load_state_dict(RE.fixture_state_dict(det.img_backbone.state_dict(), 80), strict=True)
    det.img_neck.load_state_dict(RE.fixture_state_dict(det.img_neck.state_dict(), 81, RE.transposed_keys(ncfg["upsample_strides"])), strict=True)
    det = det.to(dev).eval()
    data_config = dict(cams=R.CAMS[:2], Ncams=2, input_size=(64, 96), src_size=(150, 230), resize=(0, 0), rot=(0, 0), flip=False,
                       crop_h=(0.0, 0.0), resize_test=0.0)
    frames = np.stack([R.frame(150, 230, "random", seed=70 + i) for i in range(2)])
    infos, l2c = R.synthetic_calibration()
    want14, _ = R.img_inputs14(data_config, frames, infos, l2c)
    twelve, _ = II.LoadMultiViewFrames(data_config, device=dev)(list(frames), infos, l2c)
    img = II.with_bda(twelve)[0]
    assert tuple(img.shape) == (1, 2, 3, 64, 96) and bits_equal(img[0].cpu(), want14[0])
    with torch.no_grad():
        a = det.image_encoder(img)["x"].clone()
        b = det.image_encoder(want14[0][None].to(dev))["x"].clone()
    assert tuple(a.shape) == (1, 2, sum(oc), 4, 6) and bits_equal(a.cpu(), b.cpu()) and float(a.abs().sum()) > 0
    core.check_h2_overflow()


# ------------------------------------------------------------------ refusals
def test_refusals(dev):
    Hs, Ws, dims, box, fl = R.CASES["both_passes"]
    plan = II.ResizePlan(Hs, Ws, [(dims, box, fl)] * 2, (12, 16), device=dev)
    f = torch.from_numpy(np.stack([R.frame(Hs, Ws, "random", 1)] * 2))
    with pytest.raises(CooccError):
        II.frames_to_imgs(f, plan)                                               # CPU tensor
    with pytest.raises(CooccError):
        II.frames_to_imgs([f[0].to(dev), f[1]], plan)                            # one of a list on the CPU
    d = f.to(dev)
    with pytest.raises(ValueError, match="uint8"):
        II.frames_to_imgs(d.float(), plan)
    with pytest.raises(ValueError, match=r"Hs, Ws, 3"):
        II.frames_to_imgs(torch.zeros((2, Hs, Ws, 4), dtype=torch.uint8, device=dev), plan)
    with pytest.raises(ValueError, match="mixed sizes"):
        II.frames_to_imgs([d[0], d[1][:-1].contiguous()], plan)
    with pytest.raises(ValueError, match="3 frames"):
        II.frames_to_imgs(torch.cat([d, d[:1]]), plan)
    with pytest.raises(ValueError, match="plan was made for"):
        II.frames_to_imgs(d[:, :-1].contiguous(), plan)
    infos, l2c = R.synthetic_calibration()
    cfg = dict(R.R50, input_size=(12, 16))
    load = II.LoadMultiViewFrames(cfg, device=dev)
    with pytest.raises(ValueError, match="5 frames for the 6 cameras"):
        load([f[0].numpy()] * 5, infos, l2c)
    with pytest.raises(ValueError, match="no calibration"):
        load([f[0].numpy()] * 6, {k: infos[k] for k in R.CAMS[:5]}, l2c)
    with pytest.raises(ValueError, match="uint8"):
        load([f[0].numpy().astype(np.float32)] * 6, infos, l2c)
    rot = II.LoadMultiViewFrames(dict(cfg, rot=(5.0, 5.0), Ncams=6), is_train=True, device=dev, rng=np.random.RandomState(1))
    with pytest.raises(NotImplementedError, match=r"'rot': \(0, 0\).*nearest-neighbour"):
        rot([f[0].numpy()] * 6, infos, l2c)
    with pytest.raises(ValueError, match="ratio"):
        II.LoadMultiViewFrames(dict(cfg, input_size=(2, 4)), device=dev)([R.frame(64, 64, "random", 2)] * 6, infos, l2c)


def test_training_draws_per_camera(dev):
    """Training mode: five of six cameras chosen, each with its own draw, from a seeded generator -- the bits of the restatement on
    the parameters the loader reports."""
    cfg = dict(R.TRAIN, input_size=(24, 40))
    frames = {c: R.frame(60, 90, "random", seed=80 + i) for i, c in enumerate(R.CAMS)}
    infos, l2c = R.synthetic_calibration()
    load = II.LoadMultiViewFrames(cfg, is_train=True, device=dev, rng=np.random.RandomState(3))
    twelve, extras = load(frames, infos, l2c)
    names, params = list(extras["cam_names"]), extras["params"]
    assert len(names) == 5 and len(set(names)) == 5 and len({(p["resize_dims"], p["crop"]) for p in params}) > 1
    cv = np.stack([R.canvas(frames[c], p["resize_dims"], p["crop"], bool(p["flip"])) for c, p in zip(names, params)])
    assert np.array_equal(extras["canvas"].cpu().numpy(), cv) and bits_equal(twelve[0].cpu(), R.to_imgs(cv))
    for i, p in enumerate(params):
        rot, tran = R.post_matrices(p["resize"], p["crop"], bool(p["flip"]))
        assert bits_equal(twelve[4][i].cpu(), rot) and bits_equal(twelve[5][i].cpu(), tran)


# ------------------------------------------------------------------ beside matrix-core work
@pytest.mark.parametrize("corunner", ["h2p", "wino"])
def test_bit_stable_beside_matrix_core_work(dev, corunner):
    import test_gpu_corunner as C
    S = C._scene(dev)
    cams = [((704, 396), (0, 140, 704, 396), i % 2 == 1) for i in range(2)]
    frames = torch.from_numpy(np.stack([R.frame(900, 1600, "random", seed=90 + i) for i in range(2)])).to(dev)
    plan = II.ResizePlan(900, 1600, cams, (256, 704), device=dev)

    def fn():
        canvas = torch.empty((2, 256, 704, 3), dtype=torch.uint8, device=dev)
        return [II.frames_to_imgs(frames, plan, canvas=canvas), canvas]
    ref, got = C._run_beside(S, fn, n=20, corunner=corunner)
    assert len(got) == 20 and C._count_differing(ref, got) == 0
