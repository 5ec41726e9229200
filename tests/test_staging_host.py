"""co_occ_amd.staging without a GPU: the layout of a staged upload and the refusals of the shared argument checks."""
import numpy as np
import pytest
import torch

from co_occ_amd import _lib, staging
from co_occ_amd._lib import CooccError


def mixed():
    rng = np.random.default_rng(0)
    return [rng.random((5, 3), np.float32), rng.integers(0, 65535, (4, 4)).astype(np.uint16), np.arange(7, dtype=np.uint8),
            np.zeros((0, 5), np.float32), tuple(rng.random((n, 5), np.float32) for n in (2, 0, 3)), np.arange(300, dtype=np.int64)]


def test_layout_of_mixed_dtypes():
    arrays = mixed()
    parts, shapes, dtypes, offs, sizes, total = staging.stage_layout(arrays)
    assert [sum(p.nbytes for p in ps) for ps in parts] == sizes == [60, 32, 7, 0, 100, 2400]
    assert all(o % 256 == 0 for o in offs) and offs == sorted(offs) and offs[0] == 0
    slots = [-(-n // 256) * 256 for n in sizes]          # one 256-rounded slot per entry, a group included: no padding inside it
    assert offs == [sum(slots[:i]) for i in range(len(slots))] and total == sum(slots)
    assert [len(ps) for ps in parts] == [1, 1, 1, 1, 3, 1] and [p.shape for p in parts[4]] == [(2, 5), (0, 5), (3, 5)]
    assert shapes == [(5, 3), (4, 4), (7,), (0, 5), (25,), (300,)]
    assert dtypes == [torch.float32, torch.int16, torch.uint8, torch.float32, torch.float32, torch.int64]
    assert all(p.flags["C_CONTIGUOUS"] for ps in parts for p in ps)


def test_layout_makes_contiguous_and_keeps_the_bits():
    a = np.arange(24, dtype=np.float32).reshape(4, 6)[:, ::2]
    parts, shapes, _, _, _, total = staging.stage_layout([a])
    assert parts[0][0].flags["C_CONTIGUOUS"] and np.array_equal(parts[0][0], a) and shapes == [(4, 3)] and total == 256


def test_layout_of_nothing():
    assert staging.stage_layout([]) == ([], [], [], [], [], 0)
    parts, shapes, dtypes, offs, sizes, total = staging.stage_layout([np.zeros((0, 5), np.float32), (), (np.zeros((0, 3), np.uint16),)])
    assert total == 0 and offs == [0, 0, 0] == sizes and shapes == [(0, 5), (0,), (0,)]
    assert dtypes == [torch.float32, torch.uint8, torch.int16] and parts[1] == []


def test_total_is_last_bytes(monkeypatch):
    """``HostStage`` reports the layout's total; an all-empty upload returns before any GPU call but the device tensors it makes, so
    those are redirected to the CPU here."""
    stage = staging.HostStage("cuda")
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: real(*a, **dict(k, device="cpu")))
    out = stage([np.zeros((0, 5), np.float32), ()])
    assert stage.last_bytes == 0 == staging.stage_layout([np.zeros((0, 5), np.float32), ()])[-1]
    assert [tuple(t.shape) for t in out] == [(0, 5), (0,)] and [t.dtype for t in out] == [torch.float32, torch.uint8]


def test_refusals_of_the_shared_checks():
    with pytest.raises(CooccError, match="GPU only"):
        _lib.require_gpu("cpu")
    with pytest.raises(CooccError, match="GPU only.*rows is a cpu tensor"):
        _lib.require_gpu(torch.zeros(1), "rows")
    with pytest.raises(CooccError, match="GPU only"):
        _lib.ptr(torch.zeros(1))
    _lib.require_gpu("cuda:1")
    _lib.require_gpu(torch.device("cuda"))
    with pytest.raises(CooccError, match="GPU only"):
        staging.HostStage("cpu")([np.zeros(1, np.float32)])
    with pytest.raises(CooccError, match="GPU only"):
        staging.PointStage("cpu")(np.zeros((1, 3), np.float32))
    t = torch.zeros((2, 4), dtype=torch.int16)
    with pytest.raises(ValueError, match="rows must be a tensor"):
        staging.device_tensor("rows", t.numpy(), torch.int16, 4)
    with pytest.raises(CooccError, match="GPU only"):
        staging.device_tensor("rows", t, torch.int16, 4)
    # device_tensor refuses the host before it looks at dtype and shape (tests/test_gpu_staging.py has those); check_points does not
    for bad, word in ((np.zeros((1, 3), np.float64), "float32"), (torch.zeros((1, 3), dtype=torch.float16), "float32"),
                      (np.zeros((1, 2), np.float32), "C >= 3"), (torch.zeros(3), "C >= 3"), ([[0.0, 0.0, 0.0]], "tensor or a numpy array")):
        with pytest.raises(ValueError, match=word):
            staging.check_points(bad)
    with pytest.raises(ValueError, match=r"P >= 1, C >= 3"):
        staging.check_points(np.zeros((0, 3), np.float32), min_rows=1)
    ok = np.zeros((0, 4), np.float32)
    assert staging.check_points(ok) is ok
    with pytest.raises(ValueError, match="points must be a tensor"):
        staging.device_points(ok)
    with pytest.raises(CooccError, match="GPU only"):
        staging.device_points(torch.zeros((1, 3)))
