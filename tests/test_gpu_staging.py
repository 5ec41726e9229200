"""co_occ_amd.staging on the MI355X: what goes up through a ``HostStage`` comes back with the same bytes, the documented shapes and
dtypes, as views of one upload."""
import numpy as np
import pytest
import torch

from co_occ_amd import staging

pytestmark = pytest.mark.gpu


def sample(seed, scale=1):
    rng = np.random.default_rng(seed)
    return [rng.random((5 * scale, 3), np.float32), rng.integers(0, 65536, (4 * scale, 4)).astype(np.uint16),
            rng.integers(0, 256, 7 * scale).astype(np.uint8), np.zeros((0, 5), np.float32),
            tuple(rng.random((n * scale, 5), np.float32) for n in (2, 0, 3))]


def same(got, arrays):
    """the device tensors of one ``HostStage`` call against what went up: shapes, documented dtypes, bytes"""
    want = [np.concatenate([p.reshape(-1) for p in a]) if isinstance(a, tuple) else a for a in arrays]
    assert [tuple(t.shape) for t in got] == [w.shape for w in want]
    assert [t.dtype for t in got] == [torch.float32, torch.int16, torch.uint8, torch.float32, torch.float32]
    for t, w in zip(got, want):
        assert t.is_cuda and t.cpu().numpy().tobytes() == w.tobytes()


def test_mixed_arrays_come_back_with_their_bytes(dev):
    stage, arrays = staging.HostStage(dev), sample(1)
    got = stage(arrays)
    same(got, arrays)
    assert stage.last_bytes == staging.stage_layout(arrays)[-1] == 4 * 256          # 60, 32, 7, 0 and 100 bytes: four slots, one empty
    assert len({t.untyped_storage().data_ptr() for t in got}) == 1


def test_reuse_and_growth_of_the_buffer(dev):
    stage, first, second = staging.HostStage(dev), sample(2), sample(3, scale=40)
    a = stage(first)
    b = stage(second)          # larger: the buffer is replaced; the first upload's device tensors are its own
    c = stage(first)           # smaller: the buffer is reused after the previous copy has read it
    same(a, first), same(b, second), same(c, first)
    assert stage.last_bytes == staging.stage_layout(first)[-1] < staging.stage_layout(second)[-1] <= stage._stage.numel()


def test_threaded_fill_uploads_the_same_bytes(dev):
    """``threaded_fill`` (the loader's frames) lays the arrays with torch's ``copy_``: the same upload, array for array."""
    stage, first, second = staging.HostStage(dev, threaded_fill=True), sample(6), sample(7, scale=3000)
    same(stage(first), first), same(stage(second), second), same(stage(first), first)
    assert stage.last_bytes == staging.stage_layout(first)[-1]


def test_named_form(dev):
    stage = staging.HostStage(dev)
    there = torch.arange(6, dtype=torch.float32, device=dev).view(2, 3)
    host = dict(rows=np.arange(12, dtype=np.uint16).reshape(3, 4), there=there, bda=torch.eye(3), seg=np.arange(5, dtype=np.uint8))
    out = stage.named(host)
    assert list(out) == list(host) and out["there"] is there
    assert out["rows"].dtype == torch.int16 and np.array_equal(out["rows"].cpu().numpy().view(np.uint16), host["rows"])
    assert torch.equal(out["bda"].cpu(), torch.eye(3)) and np.array_equal(out["seg"].cpu().numpy(), host["seg"])
    staged = {out[k].untyped_storage().data_ptr() for k in ("rows", "bda", "seg")}
    assert len(staged) == 1 and there.untyped_storage().data_ptr() not in staged
    assert stage.last_bytes == 3 * 256
    assert stage.named(dict(there=there)) == dict(there=there) and stage.last_bytes == 3 * 256          # nothing to stage: no upload


def test_point_stage_and_the_checks_on_device_tensors(dev):
    pts = np.random.default_rng(4).random((9, 4), np.float32)
    stage = staging.PointStage(dev)
    up = stage(pts)
    assert np.array_equal(up.cpu().numpy(), pts) and stage(up) is up and np.array_equal(stage(torch.from_numpy(pts)).cpu().numpy(), pts)
    assert tuple(stage(pts[:0]).shape) == (0, 4)
    assert staging.device_points(up[:, :3]).is_contiguous()
    rows = torch.zeros((2, 4), dtype=torch.int16, device=dev)
    assert staging.device_tensor("rows", rows, torch.int16, 4) is rows
    with pytest.raises(ValueError, match="rows must be torch.int32"):
        staging.device_tensor("rows", rows, torch.int32, 4)
    with pytest.raises(ValueError, match="rows must be 1-dimensional"):
        staging.device_tensor("rows", rows, torch.int16, dim=1)
    with pytest.raises(ValueError, match="rows must be 2-dimensional with 3 columns"):
        staging.device_tensor("rows", rows, torch.int16, 3)
    with pytest.raises(ValueError, match="C >= 3"):
        staging.device_points(up[:, :2])
