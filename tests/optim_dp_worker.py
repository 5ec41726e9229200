"""Workers of tests/test_gpu_optim_dp.py: two processes on ONE GPU, gloo carrying the collectives (as tests/syncbn_worker.py).
Rank ``r`` draws its gradients with ``optim_refs.gradients(cs, seed=r)``; with two ranks the average ``g0/2 + g1/2`` is one
rounding and order-free, so the step with a group must equal, bit for bit, the single-rank ``optim.AdamW`` of the same process fed
that average (tests/optim_dp_refs.py)."""
import datetime
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    return dev


def _same_on_both_ranks(tensors, what):
    """All-gather the CPU bits and compare."""
    from util_second3d import bits_equal
    flat = torch.cat([t.detach().cpu().reshape(-1).float() for t in tensors])
    got = [torch.empty_like(flat) for _ in range(dist.get_world_size())]
    dist.all_gather(got, flat)
    assert all(bits_equal(g, got[0]) for g in got[1:]), what + ": the ranks hold different bits"
    return got


# ------------------------------------------------------------------ a. four clipped steps
def check_four_steps(dev, rank):
    import optim_dp_refs as D
    import optim_refs as R
    import util
    from co_occ_amd import optim
    from test_gpu_optim import STATE, device_params, judge, run_device, set_grads
    from util_second3d import bits_equal
    cs, p0, avg, r64, r32 = D.averaged_reference(optim.chunk_size())
    mine = D.rank_gradients(cs, rank)
    late = [i for i, c in enumerate(cs) if c[2] == "late"][0]
    params = device_params(dev, cs, p0)
    opt = optim.AdamW(R.make_groups(params), max_grad_norm=R.MAX_NORM, process_group=True)
    norms = []
    for k, row in enumerate(mine):
        set_grads(params, cs, row, dev)
        opt.step()
        norms.append(opt.grad_norm)
        assert (params[late] in opt.state) == (k >= R.LATE_FROM), "the late parameter has no state before its gradient appears"
    torch.cuda.synchronize()
    assert int(opt.grad_mismatch) == 0
    for p, g in zip(params, mine[-1]):
        if g is not None:
            assert bits_equal(p.grad.cpu(), g), ".grad keeps the local bits"
    # against the single-rank path of this process fed the fp32 average
    ps, os_, ns = run_device(dev, cs, p0, avg, R.MAX_NORM)
    for i, (name, _, _) in enumerate(cs):
        assert bits_equal(params[i].detach().cpu(), ps[i].detach().cpu()), "rank %d %s: p" % (rank, name)
        assert (params[i] in opt.state) == (ps[i] in os_.state), name
        if ps[i] in os_.state:
            assert float(opt.state[params[i]]["step"]) == float(os_.state[ps[i]]["step"]), name
            for k in STATE:
                assert bits_equal(opt.state[params[i]][k].cpu(), os_.state[ps[i]][k].cpu()), "rank %d %s: %s" % (rank, name, k)
    for k, (a, b) in enumerate(zip(norms, ns)):
        assert bits_equal(a.cpu(), b.cpu()), "step %d grad_norm" % k
    # against float64 on the averaged rows
    judge(cs, params, opt, r64, r32, "dp rank %d" % rank)
    for k, (n, want) in enumerate(zip(norms, r64["norms"])):
        rel = abs(float(n.double()) - want) / want
        print("[optim-dp] rank %d step %d grad_norm %.9g float64 %.17g rel %.3e" % (rank, k, float(n), want, rel))
        assert rel <= 2.0 ** -23, "step %d: grad_norm %.9g vs float64 %.17g" % (k, float(n), want)
    # the averaged run is not this rank's own run
    own = run_device(dev, cs, p0, mine, R.MAX_NORM)[0]
    assert not bits_equal(own[0].detach().cpu(), params[0].detach().cpu())
    state = [opt.state[p][k] for p in params if p in opt.state for k in STATE]
    _same_on_both_ranks([p for p in params] + state + norms, "parameters, moments and grad_norm")


# ------------------------------------------------------------------ b. write_reduced_grad
def check_write_reduced(dev, rank):
    import optim_dp_refs as D
    import optim_refs as R
    from co_occ_amd import optim
    from test_gpu_optim import device_params, set_grads
    from util_second3d import bits_equal
    cs, p0, avg, r64, _ = D.averaged_reference(optim.chunk_size())
    mine = D.rank_gradients(cs, rank)
    assert r64["norms"][1] > 2 * R.MAX_NORM
    pa, pb, pc = (device_params(dev, cs, p0) for _ in range(3))
    oa = optim.AdamW(R.make_groups(pa), max_grad_norm=R.MAX_NORM, process_group="world")
    oa.write_reduced_grad = True
    ob = optim.AdamW(R.make_groups(pb), max_grad_norm=R.MAX_NORM, process_group=dist.group.WORLD)
    ob.write_reduced_grad = ob.write_clipped_grad = True
    oc = optim.AdamW(R.make_groups(pc), max_grad_norm=R.MAX_NORM)             # single rank on the average, writing its clipped gradient
    oc.write_clipped_grad = True
    for k in (0, 1):
        set_grads(pa, cs, mine[k], dev), set_grads(pb, cs, mine[k], dev), set_grads(pc, cs, avg[k], dev)
        oa.step(), ob.step(), oc.step()
        torch.cuda.synchronize()
        clipped = 0
        for i, g in enumerate(avg[k]):
            if g is None:
                assert pa[i].grad is None and pb[i].grad is None
                continue
            assert bits_equal(pa[i].grad.cpu(), g), "step %d %s: .grad is the average" % (k, cs[i][0])
            assert bits_equal(pb[i].grad.cpu(), pc[i].grad.cpu()), "step %d %s: .grad is the clipped average" % (k, cs[i][0])
            clipped += not bits_equal(pb[i].grad.cpu(), g)
        assert (clipped > 0) == (k == 1), "the clip is active at step 1 only"
    assert int(oa.grad_mismatch) == 0 and int(ob.grad_mismatch) == 0


# ------------------------------------------------------------------ c. all_reduce_gradients + torch.optim.AdamW
def check_all_reduce_gradients(dev, rank):
    import optim_dp_refs as D
    import optim_refs as R
    from co_occ_amd import optim
    from test_gpu_optim import device_params, set_grads
    from util_second3d import bits_equal
    cs, p0, avg, _, _ = D.averaged_reference(optim.chunk_size())
    mine = D.rank_gradients(cs, rank)
    params = device_params(dev, cs, p0)
    topt = torch.optim.AdamW(R.make_groups(params))
    for k in (0, 2):                                  # without and with the late parameter's gradient
        set_grads(params, cs, mine[k], dev)
        versions = [None if p.grad is None else p.grad._version for p in params]
        word = optim.all_reduce_gradients(params)
        torch.cuda.synchronize()
        for i, g in enumerate(avg[k]):
            if g is None:
                assert params[i].grad is None
            else:
                assert bits_equal(params[i].grad.cpu(), g), "step %d %s: .grad is the average" % (k, cs[i][0])
                assert g.numel() == 0 or params[i].grad._version > versions[i]
        topt.step()
    assert int(word) == 0
    _same_on_both_ranks(params, "parameters after torch.optim.AdamW on the averaged gradients")


# ------------------------------------------------------------------ d. broadcast_parameters
def check_broadcast(dev, rank):
    import optim_refs as R
    from co_occ_amd import optim
    from test_gpu_optim import device_params
    from util_second3d import bits_equal
    cs = R.cases(optim.chunk_size())
    zero, other = R.initial(cs, 0), R.initial(cs, 7)
    params = device_params(dev, cs, zero if rank == 0 else other)          # the views at storage offsets 1 and 2 among them
    g = torch.Generator().manual_seed(31)
    extra = dict(i64=torch.randint(0, 1 << 40, (5,), generator=g), f16=torch.randn(7, generator=g).half(),
                 strided=torch.randn(4, 6, generator=g))
    tensors = {k: (v if rank == 0 else torch.zeros_like(v)).to(dev) for k, v in extra.items()}
    tensors["strided"] = tensors["strided"].t()                           # fp32, not contiguous: the plain route
    assert not tensors["strided"].is_contiguous()
    everything = params + list(tensors.values())
    versions = [t._version for t in everything]
    optim.broadcast_parameters(everything, src=0)
    torch.cuda.synchronize()
    for (name, _, _), p, want in zip(cs, params, zero):
        assert bits_equal(p.detach().cpu(), want), "rank %d %s holds rank 0's bits" % (rank, name)
    assert torch.equal(tensors["i64"].cpu(), extra["i64"]) and bits_equal(tensors["f16"].cpu(), extra["f16"])
    assert bits_equal(tensors["strided"].cpu(), extra["strided"].t())
    if rank != 0:
        assert all(t._version > v for t, v in zip(everything, versions) if t.numel()), "the version counters moved"
    # a module: parameters, fp32 buffers and num_batches_tracked
    bn = torch.nn.BatchNorm1d(6).to(dev)
    with torch.no_grad():
        for t in list(bn.parameters()) + list(bn.buffers()):
            t.copy_(torch.arange(t.numel(), device=dev).reshape(t.shape) * (1 if rank == 0 else 3) + (5 if rank == 0 else 11))
    optim.broadcast_parameters(bn)
    torch.cuda.synchronize()
    for name, t in list(bn.named_parameters()) + list(bn.named_buffers()):
        assert torch.equal(t.detach().cpu(), (torch.arange(t.numel()).reshape(t.shape) + 5).to(t.dtype)), name
    assert bn.num_batches_tracked.dtype == torch.int64 and int(bn.num_batches_tracked) == 5


# ------------------------------------------------------------------ e. a real backward
def check_real_backward(dev, rank, world):
    from co_occ_amd import autograd as ag, optim
    from util_second3d import bits_equal
    g = torch.Generator().manual_seed(21)
    Cin, Cout, X, Y, Z = 8, 12, 6, 5, 4                                  # tests/syncbn_worker.py's layer, one sample per rank
    x = torch.randn(world, Cin, X, Y, Z, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) * 0.1
    res = torch.randn(world, Cout, X, Y, Z, generator=g)
    gout = torch.randn(world, Cout, X, Y, Z, generator=g)
    gam, bet = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    bn = torch.nn.SyncBatchNorm(Cout, eps=1e-3, momentum=0.1).to(dev).train()
    bn.weight.data.copy_(gam); bn.bias.data.copy_(bet)
    rows = lambda t: t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1]).contiguous()
    xd = rows(x[rank:rank + 1]).to(dev).requires_grad_()
    wd = w.to(dev).requires_grad_()
    rd = rows(res[rank:rank + 1]).to(dev).requires_grad_()
    out, _ = ag.conv3d_bn_train_rows(xd, wd, (1, X, Y, Z), bn, relu=True, res2d=rd)      # SyncBatchNorm -> synchronised
    out.backward(rows(gout[rank:rank + 1]).to(dev))
    params = [wd, bn.weight, bn.bias]
    assert all(p.grad is not None and bool(p.grad.abs().sum() > 0) for p in params)
    # the fp32 average of the two ranks' gathered gradients, and a single-rank step on it
    avg = []
    for p in params:
        mine = p.grad.detach().cpu()
        got = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(got, mine)
        assert not bits_equal(got[0], got[1]), "the ranks' shares differ"
        avg.append(got[0] / 2 + got[1] / 2)
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    for t, a in zip(twins, avg):
        t.grad = a.to(dev)
    kw = dict(lr=1e-2, weight_decay=0.05, max_grad_norm=0.5)
    single = optim.AdamW(twins, **kw)
    single.step()
    opt = optim.AdamW(params, process_group=True, **kw)
    opt.step()
    torch.cuda.synchronize()
    for p, t, name in zip(params, twins, ("weight", "gamma", "beta")):
        assert bits_equal(p.detach().cpu(), t.detach().cpu()), "real backward: " + name
        for k in ("exp_avg", "exp_avg_sq"):
            assert bits_equal(opt.state[p][k].cpu(), single.state[t][k].cpu()), "real backward: %s %s" % (name, k)
    assert bits_equal(opt.grad_norm.cpu(), single.grad_norm.cpu()) and int(opt.grad_mismatch) == 0
    _same_on_both_ranks(params, "the layer's parameters after the step")


def run_agreeing(rank, world, port):
    dev = _init(rank, world, port)
    try:
        check_four_steps(dev, rank)
        check_write_reduced(dev, rank)
        check_all_reduce_gradients(dev, rank)
        check_broadcast(dev, rank)
        check_real_backward(dev, rank, world)
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------ f. / g. the contract's violations
def run_violating(rank, world, port):
    dev = _init(rank, world, port)
    try:
        import optim_refs as R
        from co_occ_amd import optim
        from test_gpu_optim import device_params, set_grads
        from util_second3d import bits_equal
        cs = R.cases(optim.chunk_size())
        p0, mine = R.initial(cs, 0), R.gradients(cs, seed=rank)
        late = [i for i, c in enumerate(cs) if c[2] == "late"][0]
        # f. rank 1 holds one parameter more: the first step raises on BOTH ranks and changes nothing
        params = device_params(dev, cs, p0)
        more = params + ([torch.nn.Parameter(torch.ones(9, device=dev))] if rank == 1 else [])
        opt = optim.AdamW(R.make_groups(more), max_grad_norm=R.MAX_NORM, process_group=True)
        set_grads(params, cs, mine[0], dev)
        try:
            opt.step()
        except ValueError as e:
            n = len([p for p in more if p.requires_grad and p.numel()])
            assert "this rank presents %d tensors" % n in str(e), str(e)
        else:
            raise AssertionError("rank %d: layouts of different size were stepped" % rank)
        torch.cuda.synchronize()
        assert len(opt.state) == 0 and all(bits_equal(p.detach().cpu(), v) for p, v in zip(params, p0)), "a refused step changes nothing"
        # g. rank 1 has a gradient for the late parameter at step 0, rank 0 has none: the step completes, and both ranks see it
        params = device_params(dev, cs, p0)
        opt = optim.AdamW(R.make_groups(params), max_grad_norm=R.MAX_NORM, process_group=True)
        set_grads(params, cs, mine[0], dev)
        if rank == 1:
            params[late].grad = torch.ones_like(params[late])
        opt.step()
        torch.cuda.synchronize()
        assert int(opt.grad_mismatch) == 1, "rank %d: grad_mismatch = %d" % (rank, int(opt.grad_mismatch))
        assert (params[late] in opt.state) == (rank == 1), "the stepping rule stays the rank's own .grad is None"
        set_grads(params, cs, mine[1], dev)                               # an agreeing step afterwards: the word is sticky
        opt.step()
        torch.cuda.synchronize()
        assert int(opt.grad_mismatch) == 1 and bool(torch.isfinite(opt.grad_norm))
    finally:
        dist.destroy_process_group()
