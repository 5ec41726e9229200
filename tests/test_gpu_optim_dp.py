"""Data-parallel gradient averaging inside the device AdamW step (co_occ_amd/optim.py, csrc/optim.hip) on the GPU.
In one process: the pack, unpack and flag-check kernels alone against torch's CPU arithmetic bit for bit, and the arena path
(``dp_always``) against the plain ``optim.AdamW``, the trusted single-rank path.  In two processes on the one GPU over gloo
(tests/optim_dp_worker.py): the step with a group against the single-rank step fed the average, the float64 judge, the helpers and
the two contract violations.  Everything on tests/optim_refs.py's case set."""
import socket
import time

import pytest
import torch

from co_occ_amd import optim

import optim_refs as R
import util
from test_gpu_optim import STATE, device_params, run_device, set_grads
from util_second3d import bits_equal

pytestmark = pytest.mark.gpu

WORKER_DEADLINE = 240.0            # seconds for one spawn (two HIP start-ups and the checks); the parent never waits longer


def chunk():
    return optim.chunk_size()


def layout_of(cs, params):
    """[(case index, parameter)] of the layout: requires_grad and elements."""
    return [(i, p) for i, p in enumerate(params) if p.requires_grad and p.numel() > 0]


def reducer_for(dev, world_row=0):
    cs, p0, rows, _, _ = R.reference(chunk())
    params = device_params(dev, cs, p0)
    set_grads(params, cs, rows[world_row], dev)
    lay = layout_of(cs, params)
    red = optim._Reducer([p for _, p in lay], [i for i, _ in lay], dev)
    return cs, rows[world_row], params, lay, red


def cpu_arena(red):
    torch.cuda.synchronize()
    return red.arena.cpu()


def check_arena(cs, lay, red, arena, want):
    """``want[k]``: the CPU fp32 tensor segment k must hold bit for bit, or None (zeros, flag 0).  Everything else is zero."""
    L = red.layout
    assert arena.numel() == L.total and L.header == len(lay)
    covered = torch.zeros(L.total, dtype=torch.bool)
    covered[:L.header] = True
    for k, (i, p) in enumerate(lay):
        o, n = int(L.offsets[k]), p.numel()
        assert o % 4 == 0 and not bool(covered[o:o + n].any()), cs[i][0]
        covered[o:o + n] = True
        seg = arena[o:o + n]
        if want[k] is None:
            assert float(arena[k]) == 0.0 and not bool(seg.view(torch.int32).any()), "%s: no gradient -> flag 0 and zero bits" % cs[i][0]
        else:
            assert float(arena[k]) == 1.0, "%s: flag" % cs[i][0]
            assert bits_equal(seg, want[k].reshape(-1)), "%s: segment bits" % cs[i][0]
    assert not bool(arena[~covered].view(torch.int32).any()), "the padding stays zero"


# ------------------------------------------------------------------ 1. pack alone
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_pack_is_the_cpu_division_bit_for_bit(dev, world):
    cs, row, params, lay, red = reducer_for(dev)
    sources = [p.grad for _, p in lay]
    assert any(s is None for s in sources), "the late parameter has no gradient at step 0"
    assert any(s is not None and s.data_ptr() % 16 == 4 for s in sources), "the gradient view is read with 4-byte loads"
    with util.kernels() as names:
        red.pack(sources, world).done()
    assert names == {"k_optim_pack": 1}, names
    want = [None if row[i] is None else (row[i] if world == 1 else row[i] / world) for i, _ in lay]
    arena = cpu_arena(red)
    check_arena(cs, lay, red, arena, want)
    # the same values behind other alignments: every source a view at storage offset 1, 2, 3 (4-byte loads), then all aligned
    for off in (1, 2, 3, 0):
        moved = []
        for s in sources:
            if s is None:
                moved.append(None)
                continue
            buf = torch.zeros(s.numel() + 8, device=dev)
            v = buf[off:off + s.numel()]
            v.copy_(s.reshape(-1))
            assert v.data_ptr() % 16 == 4 * off
            moved.append(v)
        red.pack(moved, world).done()
        assert bits_equal(cpu_arena(red), arena), "sources at storage offset %d give the same arena bits" % off
    # a second pack with other gradients present overwrites segments and flags, and again leaves the padding alone
    late = [k for k, (i, _) in enumerate(lay) if cs[i][2] == "late"][0]
    first = [k for k, s in enumerate(sources) if s is not None][0]
    swapped = list(sources)
    swapped[late], swapped[first] = torch.full_like(lay[late][1], 3.0), None
    red.pack(swapped, world).done()
    want[late], want[first] = torch.full((lay[late][1].numel(),), 3.0) / world, None
    check_arena(cs, lay, red, cpu_arena(red), want)


# ------------------------------------------------------------------ 2. unpack alone
def test_unpack_returns_the_bits_and_touches_no_neighbour(dev):
    cs, row, params, lay, red = reducer_for(dev)
    sources = [p.grad for _, p in lay]
    red.pack(sources, 1).done()
    bufs, pairs = [], []
    for k, (i, p) in enumerate(lay):
        if sources[k] is None:
            continue
        off = k % 4                                   # plain tensors and views at storage offsets 1, 2, 3
        buf = torch.full((p.numel() + 8,), 7.0, device=dev)
        dst = buf[off:off + p.numel()]
        assert dst.data_ptr() % 16 == 4 * off
        bufs.append((i, off, buf))
        pairs.append((k, dst))
    assert {off for _, off, _ in bufs} == {0, 1, 2, 3}
    with util.kernels() as names:
        red.unpack(pairs)
    assert names == {"k_optim_unpack": 1}, names
    torch.cuda.synchronize()
    for i, off, buf in bufs:
        n = row[i].numel()
        b = buf.cpu()
        assert bits_equal(b[off:off + n], row[i].reshape(-1)), "%s at offset %d" % (cs[i][0], off)
        assert bool((b[:off] == 7.0).all()) and bool((b[off + n:] == 7.0).all()), "%s: neighbours untouched" % cs[i][0]
    # into the offset-1 / offset-2 parameter views of the case set themselves
    views = [(k, p) for k, (i, p) in enumerate(lay) if cs[i][2] in ("view1", "view2")]
    assert len(views) == 2 and sorted(p.data_ptr() % 16 for _, p in views) == [4, 8]
    red.unpack([(k, p.detach()) for k, p in views])
    torch.cuda.synchronize()
    for k, p in views:
        assert bits_equal(p.detach().cpu(), row[lay[k][0]])


# ------------------------------------------------------------------ the flag check alone
def test_flag_check_counts_and_adds(dev):
    cs, row, params, lay, red = reducer_for(dev)
    sources = [p.grad for _, p in lay]
    have = sum(s is not None for s in sources)
    assert 0 < have < len(sources)
    with util.kernels() as names:
        red.reduce(red.pack(sources, 1), None, 1)
    assert names == {"k_optim_pack": 1, "k_optim_flag_check": 1}, names
    assert red.mismatch.dtype == torch.int32 and red.mismatch.dim() == 0 and int(red.mismatch) == 0
    # no collective ran, so the header holds this rank's flags alone: against a world of 2 every tensor WITH a gradient is a
    # mismatch (1 != 2) and every one without is none (0 == 0)
    red.reduce(red.pack(sources, 2), None, 2)
    assert int(red.mismatch) == have
    red.reduce(red.pack(sources, 2), None, 2)
    assert int(red.mismatch) == 2 * have, "the word is sticky: counts are added"
    red.reduce(red.pack(sources, 1), None, 1)
    assert int(red.mismatch) == 2 * have


# ------------------------------------------------------------------ 3. the arena path against the plain path
def _dp(max_norm, **flags):
    def make(groups):
        opt = optim.AdamW(groups, max_grad_norm=max_norm)
        opt.dp_always = True
        for k, v in flags.items():
            setattr(opt, k, v)
        return opt
    return make


@pytest.mark.parametrize("max_norm", [R.MAX_NORM, None])
def test_four_steps_through_the_arena_are_the_plain_steps_bit_for_bit(dev, max_norm):
    cs, p0, rows, r64, _ = R.reference(chunk(), max_norm=max_norm)
    late = [i for i, c in enumerate(cs) if c[2] == "late"][0]
    seen = []

    def watch(k, params, opt):
        seen.append(params[late] in opt.state)
    pa, oa, na = run_device(dev, cs, p0, rows, max_norm)
    pb, ob, nb = run_device(dev, cs, p0, rows, max_norm, make=_dp(max_norm), watch=watch)
    assert seen == [k >= R.LATE_FROM for k in range(4)], "grad is None: no state"
    assert ob.grad_mismatch is not None and int(ob.grad_mismatch) == 0 and oa.grad_mismatch is None
    for i, (name, _, _) in enumerate(cs):
        assert bits_equal(pa[i].detach().cpu(), pb[i].detach().cpu()), name
        assert (pa[i] in oa.state) == (pb[i] in ob.state) == (r64["step"][i] is not None), name
        if pa[i] in oa.state:
            assert float(oa.state[pa[i]]["step"]) == float(ob.state[pb[i]]["step"]) == r64["step"][i], name
            for k in STATE:
                assert bits_equal(oa.state[pa[i]][k].cpu(), ob.state[pb[i]][k].cpu()), (name, k)
    if max_norm is None:
        assert na == nb == [None] * 4
    else:
        for a, b in zip(na, nb):
            assert b.is_cuda and b.dtype == torch.float32 and b.dim() == 0 and bits_equal(a.cpu(), b.cpu())
    for p, g in zip(pb, rows[-1]):                     # .grad keeps the local bits
        if g is not None:
            assert bits_equal(p.grad.cpu(), g)


def test_write_reduced_grad_and_the_arena_life_cycle(dev):
    cs, p0, rows, _, _ = R.reference(chunk())

    def plain(groups):
        opt = optim.AdamW(groups, max_grad_norm=R.MAX_NORM)
        opt.write_clipped_grad = True
        return opt
    grads = {}

    def keep(tag):
        def watch(k, params, opt):
            grads[tag, k] = [None if p.grad is None else p.grad.detach().cpu().clone() for p in params]
        return watch
    run_device(dev, cs, p0, rows[:2], R.MAX_NORM, make=plain, watch=keep("plain"))
    run_device(dev, cs, p0, rows[:2], R.MAX_NORM, make=_dp(R.MAX_NORM, write_reduced_grad=True, write_clipped_grad=True), watch=keep("both"))
    pr, orr, _ = run_device(dev, cs, p0, rows[:2], R.MAX_NORM, make=_dp(R.MAX_NORM, write_reduced_grad=True), watch=keep("reduced"))
    for k in (0, 1):
        for i, g in enumerate(rows[k]):
            if g is None:
                assert grads["both", k][i] is None and grads["reduced", k][i] is None
                continue
            assert bits_equal(grads["reduced", k][i], g), "world 1: the averaged gradient is the gradient"
            assert bits_equal(grads["both", k][i], grads["plain", k][i]), "clipped as the single-rank path writes it"
        assert any(g is not None and not bits_equal(a, g) for a, g in zip(grads["plain", 1], rows[1])), "the clip was active at step 1"
    # release_arena frees the buffer, keeps the counter, and the next step allocates it again and computes the same
    word = orr.grad_mismatch
    assert orr._reducer.arena is not None
    orr.release_arena()
    assert orr._reducer.arena is None and orr.grad_mismatch is word
    set_grads(pr, cs, rows[2], dev)
    orr.step()
    assert orr._reducer.arena is not None and int(orr.grad_mismatch) == 0
    # a changed requires_grad set raises locally, naming the parameter, and changes nothing
    before = [p.detach().cpu().clone() for p in pr]
    pr[0].requires_grad_(False)
    pr[0].grad = None
    with pytest.raises(ValueError, match=r"parameter 0.* requires_grad changed"):
        orr.step()
    torch.cuda.synchronize()
    assert all(bits_equal(p.detach().cpu(), b) for p, b in zip(pr, before))


# ------------------------------------------------------------------ 4. launch count
def _launches(dev, n):
    g = torch.Generator().manual_seed(n)
    params = [torch.nn.Parameter(torch.randn(100 + 3 * i, generator=g).to(dev)) for i in range(n)]
    opt = optim.AdamW(R.make_groups(params), max_grad_norm=5.0)
    opt.dp_always = True
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(dev)
    opt.step()                                   # creates the state and the arena (their zero fills are torch's)
    with util.kernels() as names:
        opt.step()
    return names


def test_launch_count_does_not_depend_on_the_number_of_tensors(dev):
    a, b = _launches(dev, 7), _launches(dev, 70)
    assert a == b == {"k_optim_pack": 1, "k_optim_flag_check": 1, "k_optim_sumsq": 1, "k_optim_clip_coef": 1, "k_optim_adamw": 1}, (a, b)


# ------------------------------------------------------------------ 5. no host read after the first step
def test_arena_steps_never_synchronise(dev):
    g = torch.Generator().manual_seed(4)
    params = [torch.nn.Parameter(torch.randn(50 + i, generator=g).to(dev)) for i in range(5)]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(dev)
    opt = optim.AdamW(R.make_groups(params), max_grad_norm=R.MAX_NORM)
    opt.dp_always = True
    opt.write_reduced_grad = True
    opt.step()                                   # the first step: state, arena, layout
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2 * optim.RING_SLOTS + 1):              # the staging ring wraps several times
            opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert opt.grad_norm.is_cuda and bool(torch.isfinite(opt.grad_norm)) and int(opt.grad_mismatch) == 0


# ------------------------------------------------------------------ two ranks on the one GPU
def _spawn(fn):
    """Two workers over gloo, joined against a deadline: a mismatched collective ends as a failure, never as a hang."""
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.spawn(fn, args=(2, port), nprocs=2, join=False)
    deadline = time.monotonic() + WORKER_DEADLINE
    try:
        while not ctx.join(timeout=max(0.1, min(5.0, deadline - time.monotonic()))):       # returns as soon as a worker ends
            if time.monotonic() > deadline:
                pytest.fail("the workers did not finish within %.0f s" % WORKER_DEADLINE)
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
        for p in ctx.processes:
            p.join(10)


def test_two_ranks_step_helpers_and_a_real_backward(dev):
    import optim_dp_worker
    _spawn(optim_dp_worker.run_agreeing)


def test_two_ranks_contract_violations_are_seen_and_do_not_hang(dev):
    import optim_dp_worker
    _spawn(optim_dp_worker.run_violating)
