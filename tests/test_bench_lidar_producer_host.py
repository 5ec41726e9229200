"""tools/bench_lidar_producer.py, the parts that need no GPU: it refuses to time anything without one, its spread is the spread, and its
probe counts the device -> host reads and C-ABI calls of the block it wraps and puts everything back."""
import importlib.util
import os

import pytest
import torch

from conftest import ROOT
from co_occ_amd import _lib


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("bench_lidar_producer", os.path.join(ROOT, "tools", "bench_lidar_producer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_refuses_without_a_gpu_and_writes_nothing(tool, tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    out = tmp_path / "bench.json"
    with pytest.raises(SystemExit) as e:
        tool.main(["--iters", "1", "--out", str(out)])
    assert "no GPU" in str(e.value) and not out.exists()


def test_the_configs_own_size_is_the_default(tool):
    assert tool.SWEEPS * tool.POINTS_PER_SWEEP == 381920
    mods, cfg = tool.build(torch.device("cpu"))
    assert cfg["pts_middle_encoder"]["sparse_shape_xyz"] == [800, 800, 64] and mods[0].max_voxels == (90000, 120000)
    assert not any(m.training for m in mods)


def test_spread(tool):
    s = tool.spread([3.0, 1.0, 2.0, 10.0, 4.0])
    assert (s["median"], s["min"], s["max"], s["n"]) == (3.0, 1.0, 10.0, 5) and s["min"] <= s["p25"] <= s["median"] <= s["p75"] <= s["max"]
    assert tool.spread([2.5]) == dict(median=2.5, min=2.5, max=2.5, p25=2.5, p75=2.5, n=1)


def test_probe_counts_reads_and_calls_and_restores(tool, monkeypatch):
    seen = []
    monkeypatch.setitem(_lib._fns, "coocc_fake_entry", lambda *a: seen.append(a) or 0)
    monkeypatch.setattr(_lib, "stream", lambda dev=None: None)
    item, tolist, conv = torch.Tensor.item, torch.Tensor.tolist, _lib.conv_fwd
    with tool.Probe() as p:
        assert torch.tensor(7).item() == 7 and torch.tensor([1, 2]).tolist() == [1, 2]
        _lib.call("coocc_fake_entry", 1, 2)
        _lib.call("coocc_fake_entry", 3)
    assert (p.reads, p.abi_calls, p.conv_launches) == (2, 2, 0) and p.blocked_s >= 0.0
    assert seen == [(1, 2, None), (3, None)]
    assert (torch.Tensor.item, torch.Tensor.tolist, _lib.conv_fwd) == (item, tolist, conv)
    _lib.call("coocc_fake_entry", 4)                        # outside the block: not counted
    assert p.abi_calls == 2
