"""Host-side logic that needs no GPU: registry / config surface, state_dict keys, BN folding,
CPU tensors are refused loudly (no fallback), and the multi-process (gloo, world_size 2)
distributed layer."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import co_occ_amd as pkg
import co_occ_amd.synth as synth
from co_occ_amd import core, dist as cdist
from conftest import ROOT


def test_registry_builds_reference_config_names():
    cfg = synth.model_cfg()
    m = pkg.build_detector(cfg)
    assert type(m).__name__ == "COOCC_Ray"
    assert type(m.occ_fuser).__name__ == "BiFuser_N" and m.occ_fuser.knum == 2
    assert type(m.semantic_encoder).__name__ == "CustomResNet3D"
    assert type(m.semantic_neck).__name__ == "FPN3D"
    assert type(m.pts_bbox_head).__name__ == "OccHead"
    assert type(m.img_view_transformer).__name__ == "ViewTransformerLiftSplatShootVoxel"
    for name in ("BiFuser_N",):
        assert name in pkg.FUSION_LAYERS
    with pytest.raises(KeyError):
        pkg.build_backbone(dict(type="NoSuchBackbone"))
    # encoder configs upstream of the path are accepted and ignored (coocc_multi_r50_256x704.py:96-135)
    m2 = pkg.build_detector(external_encoders=True, cfg=dict(cfg, img_backbone=dict(type='ResNet', depth=50), train_cfg=None,
                                 pts_voxel_layer=dict(max_num_points=10, point_cloud_range=[-50, -50, -5, 50, 50, 3],
                                                      voxel_size=[0.125] * 3, max_voxels=(90000, 120000)),
                                 pts_voxel_encoder=dict(type='HardSimpleVFE', num_features=5),
                                 pts_middle_encoder=dict(type='SparseLiDAREnc8x', input_channel=4, base_channel=16, out_channel=128,
                                                         norm_cfg=dict(type='SyncBN', requires_grad=True),
                                                         sparse_shape_xyz=[800, 800, 64])))
    assert "train_cfg" in m2.ignored_cfg_keys and m2.img_backbone is None   # encoders upstream of the path: deferred
    assert type(m2.pts_middle_encoder).__name__ == "SparseLiDAREnc8x" and m2.pts_voxel_layer.max_num_points == 10


def test_state_dict_keys_match_reference_checkpoint_layout():
    sd = pkg.build_detector(synth.model_cfg()).state_dict()
    for k in ["occ_fuser.con_enc.0.weight", "occ_fuser.con_enc.4.running_var", "occ_fuser.knn_enc.0.bias",
              "semantic_encoder.input_proj.0.weight", "semantic_encoder.input_proj.1.running_mean",
              "semantic_encoder.layers.1.0.downsample.0.weight", "semantic_encoder.layers.3.1.bn2.weight",
              "semantic_neck.lateral_convs.2.0.conv.weight", "semantic_neck.fpn_convs.0.0.bn.running_var",
              "pts_bbox_head.occ_convs.3.0.weight", "pts_bbox_head.occ_pred_conv.3.weight",
              "pts_bbox_head.voxel_soft_weights.1.running_mean", "pts_bbox_head.img_mlp_0.0.bias",
              "pts_bbox_head.img_mlp.1.weight", "pts_bbox_head.fine_mlp.3.bias",
              "sigma_head.hidden_layers.0.weight", "sigma_head.output_layer.bias", "sigma_head.posi_encoder.scales",
              "rgb_head.hidden_layers.2.weight"]:
        assert k in sd, k
    assert sd["occ_fuser.con_enc.0.weight"].shape == (256, 512, 3, 3, 3)
    assert sd["occ_fuser.knn_enc.0.weight"].shape == (128, 256)
    assert sd["pts_bbox_head.fine_mlp.0.weight"].shape == (64, 192)
    assert sum(v.numel() for k, v in sd.items() if k.startswith("semantic_encoder") and k.endswith("weight") and v.dim() == 5) > 130e6


def test_fold_bn_matches_batchnorm_eval():
    bn = torch.nn.BatchNorm3d(7).eval()
    g = torch.Generator().manual_seed(0)
    bn.running_mean.copy_(torch.randn(7, generator=g)); bn.running_var.copy_(torch.rand(7, generator=g) + 0.5)
    bn.weight.data.copy_(torch.rand(7, generator=g) + 0.5); bn.bias.data.copy_(torch.randn(7, generator=g))
    s, b = core.fold_bn(bn)
    x = torch.randn(2, 7, 3, 3, 3, generator=g)
    assert torch.allclose(bn(x), x * s.view(1, 7, 1, 1, 1) + b.view(1, 7, 1, 1, 1), atol=1e-6)
    s3, b3 = core.folded_bn(bn, torch.device("cpu"), repeat=3)
    assert torch.equal(s3, s.repeat(3)) and torch.equal(b3, b.repeat(3)) and s3.is_contiguous() and b3.is_contiguous()
    cb = torch.randn(7, generator=g)
    assert all(torch.equal(u, v) for u, v in zip(core.folded_bn(bn, torch.device("cpu"), cb), core.fold_bn(bn, cb)))


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("rank", [3, 2])
def test_deconv_weight_of_both_ranks_is_the_two_former_expressions(rank, s):
    """``core.deconv_weight`` against the expression each rank had of its own ([Cin,Cout,1,s,s]: the 3-D deblock's, [Cin,Cout,s,s]:
    the 2-D one's), value for value; detached and contiguous by default, and with ``detach=False`` attached to the parameter, whose
    gradient is then that of the former expression."""
    cin, cout = 5, 3
    g = torch.Generator().manual_seed(10 * rank + s)
    w = torch.nn.Parameter(torch.randn(*((cin, cout, 1, s, s) if rank == 3 else (cin, cout, s, s)), generator=g))

    def former(p):
        v = p[:, :, 0].permute(3, 2, 1, 0) if rank == 3 else p.permute(2, 3, 1, 0)
        return v.reshape(s * s * cout, cin)
    d = core.deconv_weight(w, s)
    assert torch.equal(d, former(w.detach())) and d.is_contiguous() and not d.requires_grad
    v = core.deconv_weight(w, s, detach=False)
    assert v.requires_grad and torch.equal(v.detach(), former(w.detach()))
    r = torch.randn(s * s * cout, cin, generator=g)
    (v * r).sum().backward()
    w2 = w.detach().clone().requires_grad_()
    (former(w2) * r).sum().backward()
    assert w.grad is not None and tuple(w.grad.shape) == tuple(w.shape) and torch.equal(w.grad, w2.grad)
    with pytest.raises(AssertionError, match="deconv kernel"):
        core.deconv_weight(w, s + 1)


def test_cpu_tensors_are_refused_not_emulated():
    f = pkg.build_fusion_layer(dict(type='BiFuser_N', knum=2, in_channels=16, out_channels=16))
    x = torch.zeros(1, 16, 4, 4, 2)
    with pytest.raises(Exception) as e:
        f(x, x)
    assert "GPU only" in str(e.value) or "no CPU fallback" in str(e.value)
    with pytest.raises(Exception):
        pkg.furthest_point_sample(torch.zeros(1, 8, 3), 2)


def test_unsupported_reference_options_fail_loudly():
    with pytest.raises(NotImplementedError):
        pkg.build_neck(dict(type='FPN3D', in_channels=[8, 16], out_channels=8))          # default GN norm
    with pytest.raises(NotImplementedError):
        pkg.build_backbone(dict(type='CustomResNet3D', depth=50, n_input_channels=8))


def test_shard_range_partitions_everything():
    for n in (0, 1, 7, 96, 336):
        for w in (1, 2, 3, 8):
            spans = [cdist.shard_range(n, r, w) for r in range(w)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            assert max(h - l for l, h in spans) - min(h - l for l, h in spans) <= 1


def test_pin_rank_threads_gives_every_rank_its_own_cores():
    """The ranks of a node split the host cores this process may use into disjoint slices (multi-GPU bench hardening)."""
    if not hasattr(os, "sched_getaffinity"):
        pytest.skip("no affinity call on this platform")
    before = sorted(os.sched_getaffinity(0))
    try:
        for n in (2, 8):
            seen = []
            for r in range(n):
                os.sched_setaffinity(0, before)
                mine = cdist.pin_rank_threads(r, n)
                assert mine and set(mine) <= set(before)
                if len(before) >= n:
                    assert sorted(os.sched_getaffinity(0)) == mine and len(mine) == len(before) // n
                seen.append(set(mine))
            if len(before) >= n:
                assert all(not (seen[i] & seen[j]) for i in range(n) for j in range(i))
        os.sched_setaffinity(0, before)
        assert cdist.pin_rank_threads(0, 1) == before            # a single rank keeps everything
    finally:
        os.sched_setaffinity(0, before)


def test_pack_unpack_maps_roundtrip():
    r, d = torch.rand(2, 4, 5, 3), torch.rand(2, 4, 5)
    r2, d2 = cdist.unpack_maps(cdist.pack_maps(r, d))
    assert torch.equal(r, r2) and torch.equal(d, d2)


_WORKER = r'''
import os, sys, torch
sys.path.insert(0, %(root)r)
import co_occ_amd.dist as cd
rank, world, local = cd.init(backend="gloo")
assert world == 2
g = torch.Generator().manual_seed(100 + rank)
rgbs, depths = torch.rand(3, 4, 6, 3, generator=g), torch.rand(3, 4, 6, generator=g)
R, D = cd.all_gather_maps(rgbs, depths)
assert R.shape == (2, 3, 4, 6, 3) and D.shape == (2, 3, 4, 6)
for r in range(2):
    g = torch.Generator().manual_seed(100 + r)
    er, ed = torch.rand(3, 4, 6, 3, generator=g), torch.rand(3, 4, 6, generator=g)
    assert torch.equal(R[r], er) and torch.equal(D[r], ed)
# asynchronous form used by bench.py: two gathers issued back to back, each completed before the next is issued
pend = cd.all_gather_maps_async(rgbs, depths)
R2, D2 = pend.wait()
pend = cd.all_gather_maps_async(rgbs * 2, depths * 2)
R3, D3 = pend.wait()
assert torch.equal(R2, R) and torch.equal(D2, D) and torch.equal(R3, R * 2) and torch.equal(D3, D * 2)
# ray-sharded render of one scene: 7 rows over 2 ranks
full = torch.arange(7 * 5 * 4, dtype=torch.float32).view(7, 5, 4)
lo, hi = cd.shard_range(7, rank, world)
out = cd.gather_ray_shards(full[lo:hi].clone(), 7)
assert torch.equal(out, full)
assert cd.max_over_ranks(float(rank + 1), torch.device("cpu")) == 2.0
cd.barrier()
print("OK", rank)
'''


def test_gloo_world_size_2_all_gather(tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    script = tmp_path / "worker.py"
    script.write_text(_WORKER % dict(root=ROOT))
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    for rank, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ("OK %d" % rank) in o, o[-2000:]


def test_bench_ticket_orders_collectives_across_threads():
    """bench.py's N > 1 path with several dense streams: whichever host thread owns sample i, the gathers are issued in sample
    order on every rank (the ticket), and an aborted run releases every waiter instead of hanging."""
    import random
    import threading
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    ticket = bench._Ticket()
    for S in (2, 3):
        ticket.reset()
        order, n = [], 40

        def worker(w):
            rnd = random.Random(w)
            for i in range(w, n, S):
                time.sleep(rnd.random() * 0.003)          # threads reach their turn in arbitrary order
                with ticket(i):
                    order.append(i)
        ths = [threading.Thread(target=worker, args=(w,)) for w in range(S)]
        [t.start() for t in ths]
        [t.join(timeout=30) for t in ths]
        assert not any(t.is_alive() for t in ths)
        assert order == list(range(n))
    # a waiter whose turn never comes is released by abort()
    ticket.reset()
    done = []

    def stuck():
        with ticket(5):
            done.append(1)
    t = threading.Thread(target=stuck)
    t.start()
    time.sleep(0.05)
    assert t.is_alive()
    ticket.abort()
    t.join(timeout=10)
    assert not t.is_alive()
    # the gates of --stagger: an event posted for sample i is what sample i + 1 finds
    gates = bench._Gates()
    gates.reset()
    assert gates.wait_for(-1) is None
    gates.post(0, "ev0")
    assert gates.wait_for(0) == "ev0"


def test_bench_dump_outputs_dtypes_cap_and_fixed_sample(tmp_path):
    """bench.py --dump-outputs: every array of a step's result lands as float32 / float64, a ``Rows`` volume as its C channels, the
    capacity-sized fine outputs of the captured dense stage cut to their count; the byte cap holds, and an array over its share is
    the same sample in every run."""
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(0)
    rows = torch.randn(8, 5, generator=g)
    out = dict(pred_c=torch.randn(1, 3, 4, 4, 2, generator=g).half(), depth=torch.arange(5, dtype=torch.float64),
               big=torch.randn(4096, generator=g), voxel_feats=core.Rows(rows, 1, 2, 2, 2, 3, coff=1), pred_f=None,
               fine_count=torch.tensor(2, dtype=torch.int32), output_voxels_fine=[torch.randn(100, 3, generator=g)],
               output_coords_fine=[torch.arange(300, dtype=torch.int32)], SC_metric=np.array([[1, 2], [3, 4]]))
    arrs = bench.host_arrays(out, cascade_ratio=2)
    assert set(arrs) == {"pred_c", "depth", "big", "voxel_feats", "fine_count", "output_voxels_fine.0", "output_coords_fine.0", "SC_metric"}
    assert arrs["pred_c"].dtype == np.float32 and arrs["depth"].dtype == np.float64 and arrs["SC_metric"].dtype == np.float64
    assert np.array_equal(arrs["voxel_feats"], rows[:, 1:4].numpy())
    assert arrs["output_voxels_fine.0"].shape == (16, 3) and np.array_equal(arrs["output_coords_fine.0"], np.arange(48.0).reshape(3, 16))
    limit = 8000
    for d in ("a", "b"):
        bench.dump_outputs(arrs, str(tmp_path / d), limit=limit)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(k + ".npy" for k in arrs) and files == sorted(os.listdir(tmp_path / "b"))
    got = {f: np.load(tmp_path / "a" / f) for f in files}
    assert sum(a.nbytes for a in got.values()) <= limit and all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["pred_c.npy"], arrs["pred_c"])                         # small arrays in full, shape kept
    big = got["big.npy"]
    assert 0 < big.size < 4096 and np.isin(big, arrs["big"]).all()
    for f in files:
        assert np.array_equal(got[f], np.load(tmp_path / "b" / f)), f


def test_detector_pickles_and_keeps_its_hooks():
    """the ``load_state_dict`` hooks are a module-level function / a bound method, the fuser's reader list holds the
    detector weakly and is re-wired on unpickling -- ``pickle`` / ``torch.save(model)`` / spawn work, and a loaded copy still
    drops its packs and its captured pipeline on ``load_state_dict``."""
    import io
    import pickle
    import torch
    import co_occ_amd as pkg
    import co_occ_amd.synth as synth
    m = pkg.build_detector(synth.model_cfg(C=32, knum=2, block_inplanes=(32, 32, 64, 64), out_channels=32))
    m2 = pickle.loads(pickle.dumps(m))
    assert type(m2) is type(m) and list(m.state_dict()) == list(m2.state_dict())
    assert m2.occ_fuser.output_readers._det() is m2
    buf = io.BytesIO()
    torch.save(m, buf)
    m2._pipe1 = "stale"
    m2.semantic_encoder._packs._key = "stale"
    m2.load_state_dict(m.state_dict())
    assert m2._pipe1 is None and m2.semantic_encoder._packs._key is None
