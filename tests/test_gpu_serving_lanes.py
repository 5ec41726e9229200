"""The lane form of ``co_occ_amd.serving.ServingPipeline`` (the default): a slot's search stage -- the one-launch input copy, the
pooling, the index search -- is issued on the slot's dense stream, between the two replays it has to sit between, with no stream or
event of its own.  Every case is compared bit for bit with sequential eager ``forward_hot_path`` calls on the same frames: slot
counts where two slots share a lane and where the slots are no multiple of the lanes, a frame that takes the eager dense stage,
a weight change between submits, and the separate-stream form the constructor still offers."""
import pytest
import torch

from test_gpu_serving import _setup

pytestmark = pytest.mark.gpu

KEYS = ("pred_c", "pred_f", "rgbs", "depths")


def _eager(bench, model, s):
    with torch.no_grad():
        out = model.forward_hot_path(bench.pool(model, s), s["pts"], s["gemo"], s["img_feats"], s["transform"], render=True)
    return {k: out[k].clone() for k in KEYS}


def _check(got, ref, tag):
    for k in KEYS:
        assert torch.equal(got[k], ref[k]), "%s: %s differs" % (tag, k)


@pytest.fixture(scope="module")
def scene(dev):
    """One model, three different frames and their eager outputs, shared (read-only) by the cases below."""
    bench, model, samples, _ = _setup(dev, n=3)
    ref = [_eager(bench, model, s) for s in samples]
    torch.cuda.synchronize()
    assert not torch.equal(ref[0]["pred_c"], ref[1]["pred_c"]) and not torch.equal(ref[1]["rgbs"], ref[2]["rgbs"])
    return bench, model, samples, [bench.frame_of(s) for s in samples], ref


def _run(model, frames, nframes, **kw):
    pipe = model.serving(frames[0], **kw)
    got = {}
    try:
        pipe.run(frames, nframes, collect=lambda i, out: got.__setitem__(i, {k: out[k].clone() for k in KEYS}))
        torch.cuda.synchronize()
    finally:
        pipe.close()
    assert sorted(got) == list(range(nframes))
    return pipe, got


@pytest.mark.parametrize("slots,lanes", [(2, 1), (3, 2), (4, 2), (6, 3)])
def test_lane_form_equals_sequential_eager_calls(scene, slots, lanes):
    bench, model, samples, frames, ref = scene
    n = 2 * slots + 1                       # every slot is reused twice
    pipe, got = _run(model, frames, n, slots=slots, dense_streams=lanes)
    assert pipe.lanes and pipe.search_streams is None and pipe.n == slots and pipe.ndense == lanes and pipe.ahead == 1
    assert pipe.fallbacks == 0 and pipe.recaptures == 0
    for i in range(n):
        _check(got[i], ref[i % 3], "slots %d lanes %d frame %d" % (slots, lanes, i))


def test_more_searches_ahead_than_lanes_share_a_lane_from_two_helper_threads(scene):
    """The lane form dispatches one search at a time by default; with ``ahead=4`` on two lanes, two helper threads issue the search
    stages of two slots on the same stream at once (each with the slot's own scratch)."""
    bench, model, samples, frames, ref = scene
    pipe, got = _run(model, frames, 13, slots=6, dense_streams=2, ahead=4)
    assert pipe.lanes and pipe.ahead == 4 and pipe.fallbacks == 0
    for i in range(13):
        _check(got[i], ref[i % 3], "ahead 4, frame %d" % i)


def test_separate_search_streams_give_the_bits_of_the_lane_form(scene):
    bench, model, samples, frames, ref = scene
    lane, got_lane = _run(model, frames, 9, slots=4, dense_streams=2)
    sep, got_sep = _run(model, frames, 9, slots=4, dense_streams=2, search_lanes=False)
    assert lane.lanes and not sep.lanes and len(sep.search_streams) == 4
    for i in range(9):
        _check(got_sep[i], got_lane[i], "separate streams against lanes, frame %d" % i)
        _check(got_sep[i], ref[i % 3], "separate streams, frame %d" % i)


def test_a_sweep_denser_than_the_captured_capacity_takes_the_eager_dense_stage_on_its_lane(dev, monkeypatch):
    """con_enc.0 in its scatter form (forced, as tests/test_gpu_serving.py does) is captured for 30 % LiDAR voxels; a middle frame
    with 40 % takes the eager dense stage on the lane it shares with another slot's graph.  One fallback; the frames after it, in
    the same slot and in the other one, are unaffected."""
    from co_occ_amd import fuser, synth
    monkeypatch.setattr(fuser, "DENSE_C0_MAX_VOXELS", 1000)
    bench, model, samples, _ = _setup(dev, n=3)
    c = synth.CONFIGS["r50"]
    _, dense_pts = synth.voxel_inputs(c["grid"], C=c["C"], seed=77, p_img=0.65, p_pts=0.40)
    dense = dict(samples[1], pts=dense_pts.to(dev))
    order = [samples[0], samples[1], samples[2], dense, samples[0], samples[1], samples[2], samples[0], samples[1]]
    ref = [_eager(bench, model, s) for s in order]
    V = c["grid"][0] * c["grid"][1] * c["grid"][2]
    assert int((dense["pts"].abs().sum(1) != 0).sum()) > model.occ_fuser.c0_capacity(V)
    pipe = model.serving(bench.frame_of(samples[0]), slots=4, dense_streams=2)
    try:
        tickets = [pipe.submit(bench.frame_of(s), copy=True) for s in order]
        got = [{k: t.result()[k].clone() for k in KEYS} for t in tickets]
        pipe.drain()
    finally:
        pipe.close()
    assert pipe.lanes and pipe.fallbacks == 1 and [t.fallback for t in tickets] == [i == 3 for i in range(len(order))]
    for i, (g, r) in enumerate(zip(got, ref)):
        _check(g, r, "frame %d" % i)


def test_a_weight_change_between_submits_recaptures_every_lane(dev):
    bench, model, samples, _ = _setup(dev, n=3)
    frames = [bench.frame_of(s) for s in samples]
    before = [_eager(bench, model, s) for s in samples]
    pipe = model.serving(frames[0], slots=3, dense_streams=2)
    try:
        got = [{k: pipe.submit(frames[i % 3], copy=True).result()[k].clone() for k in KEYS} for i in range(4)]
        with torch.no_grad():
            for name, p in model.named_parameters():
                if name.endswith("weight") and p.dim() >= 2 and ("con_enc" in name or "occ_convs" in name):
                    p.mul_(1.03)
        after = [_eager(bench, model, s) for s in samples]
        tickets = [pipe.submit(frames[i % 3], copy=True) for i in range(4, 11)]
        got += [{k: t.result()[k].clone() for k in KEYS} for t in tickets]
        pipe.drain()
    finally:
        pipe.close()
    assert pipe.recaptures == 1 and pipe.fallbacks == 0
    for i, g in enumerate(got):
        _check(g, (before if i < 4 else after)[i % 3], "frame %d" % i)
    assert not torch.equal(before[0]["pred_c"], after[0]["pred_c"])
