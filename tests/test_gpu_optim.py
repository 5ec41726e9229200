"""The device-side AdamW step on the GPU (co_occ_amd/optim.py, csrc/optim.hip) against torch's own clip_grad_norm_ + AdamW in
float64 (tests/optim_refs.py), judged at fp32's own precision by ``util.assert_precise`` (C_MAX = 4, C_RMS = 2, anchor: the same
reference in float32).  The case set, groups and schedule are optim_refs': four steps, gradient scale 0.1 / 10 under max_norm = 5,
so the clip is inactive at the first and third step and active at the second and fourth."""
import copy

import pytest
import torch

from co_occ_amd import core, lidar_trunk as lt, optim

import optim_refs as R
import util
from util_second3d import bits_equal

pytestmark = pytest.mark.gpu

STATE = ("exp_avg", "exp_avg_sq")


def chunk():
    return optim.chunk_size()


def device_params(dev, cs, p0):
    """The case set on the device: the views really are views at odd storage offsets."""
    out = []
    for (name, shape, kind), v in zip(cs, p0):
        if kind in ("view1", "view2"):
            off = 1 if kind == "view1" else 2
            buf = torch.zeros(v.numel() + 8, device=dev)
            p = buf[off:off + v.numel()].view(shape)
            p.copy_(v)
            p.requires_grad_()
            assert p.data_ptr() % 16 == 4 * off and p.is_leaf
        else:
            p = torch.nn.Parameter(v.to(dev), requires_grad=kind != "frozen")
            assert p.numel() == 0 or p.data_ptr() % 16 == 0
        out.append(p)
    return out


def set_grads(params, cs, row, dev):
    for p, (name, shape, kind), g in zip(params, cs, row):
        if g is None:
            p.grad = None
        elif kind == "gradview":
            buf = torch.zeros(g.numel() + 8, device=dev)
            gv = buf[1:1 + g.numel()].view(shape)
            gv.copy_(g)
            p.grad = gv
            assert p.grad.data_ptr() % 16 == 4 and p.data_ptr() % 16 == 0
        else:
            p.grad = g.to(dev)


def run_device(dev, cs, p0, rows, max_norm, make=None, watch=None):
    """Step the case set through ``rows`` with ``optim.AdamW`` (or ``make(groups)``).  Returns (params, optimizer, [grad_norm])."""
    params = device_params(dev, cs, p0)
    opt = (make or (lambda g: optim.AdamW(g, max_grad_norm=max_norm)))(R.make_groups(params))
    norms = []
    for k, row in enumerate(rows):
        set_grads(params, cs, row, dev)
        opt.step()
        norms.append(getattr(opt, "grad_norm", None))
        if watch is not None:
            watch(k, params, opt)
    torch.cuda.synchronize()
    return params, opt, norms


def judge(cs, params, opt, r64, r32, what):
    for i, (name, shape, kind) in enumerate(cs):
        util.assert_precise(params[i].detach().cpu(), r64["p"][i], r32["p"][i], what="%s %s p" % (what, name))
        st = opt.state.get(params[i], {})
        assert (r64["step"][i] is None) == (len(st) == 0), "%s %s: state exists where the reference has one" % (what, name)
        if st:
            assert float(st["step"]) == r64["step"][i] and not st["step"].is_cuda, "%s %s step count" % (what, name)
            for k in STATE:
                util.assert_precise(st[k].cpu(), r64[k][i], r32[k][i], what="%s %s %s" % (what, name, k))


# ------------------------------------------------------------------ 1. / 2. / 4. the four steps against the float64 judge
def test_both_clip_regimes_occur_in_the_schedule():
    _, _, _, r64, _ = R.reference(chunk())
    n = r64["norms"]
    assert len(n) == 4 and n[0] < R.MAX_NORM / 2 and n[2] < R.MAX_NORM / 2 and n[1] > 2 * R.MAX_NORM and n[3] > 2 * R.MAX_NORM, n


def test_four_clipped_steps_against_float64(dev):
    cs, p0, rows, r64, r32 = R.reference(chunk())
    late, frozen = [i for i, c in enumerate(cs) if c[2] == "late"][0], [i for i, c in enumerate(cs) if c[2] == "frozen"][0]
    seen = []

    def watch(k, params, opt):
        if k < R.LATE_FROM:                # 4. grad is None: bit-unchanged and without state
            seen.append((bits_equal(params[late].detach().cpu(), p0[late]), params[late] in opt.state))
    params, opt, norms = run_device(dev, cs, p0, rows, R.MAX_NORM, watch=watch)
    assert seen == [(True, False)] * R.LATE_FROM
    assert bits_equal(params[frozen].detach().cpu(), p0[frozen]) and params[frozen] not in opt.state and params[frozen].grad is None
    assert float(opt.state[params[late]]["step"]) == 2.0 and float(opt.state[params[0]]["step"]) == 4.0
    judge(cs, params, opt, r64, r32, "clip")
    # 2. the norm of every step: squares exact in fp64, the fp64 sum's error negligible, one rounding to fp32 (2^-24), factor 2
    for k, (n, want) in enumerate(zip(norms, r64["norms"])):
        assert n.dtype == torch.float32 and n.dim() == 0 and n.is_cuda
        rel = abs(float(n.double()) - want) / want
        print("[optim] step %d grad_norm %.9g float64 %.17g rel %.3e" % (k, float(n), want, rel))
        assert rel <= 2.0 ** -23, "step %d: grad_norm %.9g vs float64 %.17g" % (k, float(n), want)
    # the fused clip leaves .grad unscaled
    for p, g in zip(params, rows[-1]):
        if g is not None:
            assert bits_equal(p.grad.cpu(), g)


def test_four_steps_without_clipping_against_float64(dev):
    cs, p0, rows, r64, r32 = R.reference(chunk(), max_norm=None)
    params, opt, norms = run_device(dev, cs, p0, rows, None)
    assert norms == [None] * 4 and opt.grad_norm is None
    judge(cs, params, opt, r64, r32, "noclip")


# ------------------------------------------------------------------ 3. determinism
def test_two_runs_give_identical_bits(dev):
    cs, p0, rows, _, _ = R.reference(chunk())
    runs = [run_device(dev, cs, p0, rows, R.MAX_NORM) for _ in range(2)]
    (pa, oa, na), (pb, ob, nb) = runs
    for i, (name, _, _) in enumerate(cs):
        assert bits_equal(pa[i].detach().cpu(), pb[i].detach().cpu()), name
        for k in STATE:
            if pa[i] in oa.state:
                assert bits_equal(oa.state[pa[i]][k].cpu(), ob.state[pb[i]][k].cpu()), (name, k)
    for a, b in zip(na, nb):
        assert bits_equal(a.cpu(), b.cpu())


def test_the_norm_does_not_depend_on_the_gradients_alignment(dev):
    """The partial-sum order is a function of the shapes only: the same values behind a 16-byte aligned pointer (16-byte loads) and
    behind a view at storage offset 1 (4-byte loads) give the same bits."""
    c = chunk()
    g = torch.randn(2 * c + 3, generator=torch.Generator().manual_seed(5))
    norms = []
    for off in (0, 1, 2, 3):
        buf = torch.zeros(g.numel() + 8, device=dev)
        gv = buf[off:off + g.numel()]
        gv.copy_(g)
        p = torch.nn.Parameter(torch.zeros(g.numel(), device=dev))
        p.grad = gv
        assert gv.data_ptr() % 16 == 4 * off
        norms.append(optim.clip_grad_norm_([p], 1e30).cpu())
        assert bits_equal(gv.cpu(), g), "an inactive clip leaves the gradient's bits"
    assert all(bits_equal(n, norms[0]) for n in norms[1:]), [float(n) for n in norms]
    want = float(g.double().pow(2).sum().sqrt())
    assert abs(float(norms[0].double()) - want) / want <= 2.0 ** -23


# ------------------------------------------------------------------ 5. the stand-alone clip
def test_standalone_clip_then_torch_step_and_the_fused_step(dev):
    c = chunk()
    cs, p0, rows, r64, r32 = R.reference(c, steps=(1,))              # one step from the start on the second step's gradients
    assert r64["norms"][0] > 2 * R.MAX_NORM
    full = R.reference(c)[3]["norms"]
    assert r64["norms"][0] == full[1]
    # a. clip_grad_norm_ on a copy of the gradients: the norm, and g * coef within two fp32 roundings (factor 2) of float64
    params = device_params(dev, cs, p0)
    set_grads(params, cs, rows[0], dev)
    with util.kernels() as names:
        norm = optim.clip_grad_norm_(params, R.MAX_NORM)
    assert names == {"k_optim_sumsq": 1, "k_optim_clip_coef": 1, "k_optim_scale": 1}, names
    assert norm.is_cuda and norm.dtype == torch.float32 and norm.dim() == 0
    want = r64["norms"][0]
    assert abs(float(norm.double()) - want) / want <= 2.0 ** -23
    coef = min(1.0, R.MAX_NORM / (want + 1e-6))
    assert coef < 0.5
    for p, g, (name, _, _) in zip(params, rows[0], cs):
        if g is None:
            assert p.grad is None
            continue
        ref = g.double() * coef
        err = (p.grad.cpu().double() - ref).abs()
        assert bool((err <= 2.0 ** -22 * ref.abs()).all()), "%s: g * coef off by %.3e relative" % (
            name, float((err / ref.abs().clamp(min=1e-300)).max()))
    # b. torch.optim.AdamW on the clipped gradients
    topt = torch.optim.AdamW(R.make_groups(params))
    topt.step()
    torch.cuda.synchronize()
    judge(cs, params, topt, r64, r32, "clip_grad_norm_ + torch.optim.AdamW")
    # c. this class's fused clip + step on the unclipped ones
    params2, opt2, _ = run_device(dev, cs, p0, rows, R.MAX_NORM)
    judge(cs, params2, opt2, r64, r32, "fused clip + step")


def test_standalone_clip_inactive_leaves_the_bits(dev):
    cs, p0, rows, r64, _ = R.reference(chunk(), steps=(0,))
    assert r64["norms"][0] < R.MAX_NORM / 2
    params = device_params(dev, cs, p0)
    set_grads(params, cs, rows[0], dev)
    norm = optim.clip_grad_norm_(params, R.MAX_NORM)
    assert abs(float(norm.double()) - r64["norms"][0]) / r64["norms"][0] <= 2.0 ** -23
    for p, g in zip(params, rows[0]):
        if g is not None:
            assert bits_equal(p.grad.cpu(), g)


# ------------------------------------------------------------------ 6. launch count
def _launches(dev, n, max_norm):
    g = torch.Generator().manual_seed(n)
    params = [torch.nn.Parameter(torch.randn(100 + 3 * i, generator=g).to(dev)) for i in range(n)]
    opt = optim.AdamW(R.make_groups(params), max_grad_norm=max_norm)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(dev)
    opt.step()                                   # creates the state (its zero fills are torch's)
    with util.kernels() as names:
        opt.step()
    return names


def test_launch_count_does_not_depend_on_the_number_of_tensors_or_groups(dev):
    a, b = _launches(dev, 7, 5.0), _launches(dev, 70, 5.0)
    assert a == b == {"k_optim_sumsq": 1, "k_optim_clip_coef": 1, "k_optim_adamw": 1}, (a, b)
    assert _launches(dev, 7, None) == _launches(dev, 70, None) == {"k_optim_adamw": 1}


# ------------------------------------------------------------------ 7. checkpoint round trip
def test_checkpoint_from_torch_after_two_steps(dev):
    cs, p0, rows, r64, r32 = R.reference(chunk())
    params = device_params(dev, cs, p0)
    topt = torch.optim.AdamW(R.make_groups(params), fused=False)
    for row in rows[:2]:
        set_grads(params, cs, row, dev)
        torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], R.MAX_NORM)
        topt.step()
    opt = optim.AdamW(R.make_groups(params), max_grad_norm=R.MAX_NORM)
    opt.load_state_dict(copy.deepcopy(topt.state_dict()))
    for row in rows[2:]:
        set_grads(params, cs, row, dev)
        opt.step()
    torch.cuda.synchronize()
    judge(cs, params, opt, r64, r32, "torch x2 -> state_dict -> here x2")


# ------------------------------------------------------------------ 8. one real model
def _mmcv_groups(mods, lr, wd):
    """One group per parameter as mmcv's DefaultOptimizerConstructor makes them under a paramwise_cfg, norm_decay_mult = 0."""
    groups, names = [], []
    for tag, mod in mods:
        for mname, m in mod.named_modules():
            is_norm = isinstance(m, (torch.nn.modules.batchnorm._BatchNorm, torch.nn.GroupNorm, torch.nn.LayerNorm))
            for k, p in m.named_parameters(recurse=False):
                if p.requires_grad:
                    groups.append(dict(params=[p], lr=lr, weight_decay=0.0 if is_norm else wd))
                    names.append("%s%s.%s" % (tag, mname, k))
    return groups, names


def test_one_training_step_of_a_small_trunk(dev):
    """The small SECOND3D + SECOND3DFPN of tests/test_gpu_trunk_train.py: forward under train(), backward, one clipped step with
    per-parameter groups; every parameter against torch's step in float64 from the same gradients; eval() afterwards re-packs."""
    from test_gpu_trunk_train import _trunk_case
    S = _trunk_case(False)
    bcfg, ncfg = S["cfg"]
    b, n = lt.SECOND3D(**bcfg), lt.SECOND3DFPN(**ncfg)
    b.load_state_dict(S["sd"][0]), n.load_state_dict(S["sd"][1])
    b, n = b.to(dev).train(), n.to(dev).train()
    x = S["x"].to(dev)
    y = lt.rows_as_bczyx(lt.run_trunk_train(b, n, x))
    (y * S["gout"].to(dev)).sum().backward()
    core.check_h2_overflow()
    lr, wd = 1e-2, 0.01
    groups, names = _mmcv_groups((("backbone.", b), ("neck.", n)), lr, wd)
    assert len(groups) == len(list(b.parameters())) + len(list(n.parameters())) > 20
    assert any(g["weight_decay"] == 0.0 for g in groups) and any(g["weight_decay"] == wd for g in groups)
    with torch.no_grad():
        b.eval(), n.eval()
        before = lt.run_trunk(b, n, x).t.clone()                    # packs made from the weights before the step
    # references: torch's clip + step in float64 / float32 from the same gradients, copied to the CPU
    refs = {}
    for dt in (torch.float64, torch.float32):
        ps = [torch.nn.Parameter(g["params"][0].detach().cpu().to(dt)) for g in groups]
        for p, g in zip(ps, groups):
            p.grad = g["params"][0].grad.detach().cpu().to(dt)
        norm = torch.nn.utils.clip_grad_norm_(ps, R.MAX_NORM)
        torch.optim.AdamW([dict(params=[p], lr=g["lr"], weight_decay=g["weight_decay"]) for p, g in zip(ps, groups)]).step()
        refs[dt] = (ps, float(norm.double()))
    opt = optim.AdamW(groups, lr=lr, weight_decay=wd, max_grad_norm=R.MAX_NORM)
    with util.kernels() as launched:
        opt.step()
    assert launched == {"k_optim_sumsq": 1, "k_optim_clip_coef": 1, "k_optim_adamw": 1}, launched
    want = refs[torch.float64][1]
    assert abs(float(opt.grad_norm.double()) - want) / want <= 2.0 ** -23
    for name, g, p64, p32 in zip(names, groups, refs[torch.float64][0], refs[torch.float32][0]):
        util.assert_precise(g["params"][0].detach().cpu(), p64.detach(), p32.detach(), what="trunk step " + name)
    with torch.no_grad():
        after = lt.run_trunk(b, n, x).t
        b2, n2 = lt.SECOND3D(**bcfg), lt.SECOND3DFPN(**ncfg)
        b2.load_state_dict(b.state_dict()), n2.load_state_dict(n.state_dict())
        fresh = lt.run_trunk(b2.to(dev).eval(), n2.to(dev).eval(), x).t
    core.check_h2_overflow()
    assert bool(torch.isfinite(after).all()) and not bits_equal(after, before), "eval() after the step differs from before it"
    assert bits_equal(after, fresh), "... and runs on the stepped weights (the packs were made again)"


# ------------------------------------------------------------------ what step() refuses, what it takes, and that it never reads back
def test_refusals_name_the_parameter_and_a_strided_gradient_is_taken(dev):
    g = torch.Generator().manual_seed(3)
    ok = torch.nn.Parameter(torch.randn(6, 5, generator=g).to(dev))
    ok.grad = torch.randn(6, 5, generator=g).to(dev)
    half = torch.nn.Parameter(torch.randn(4, generator=g).to(dev).half())
    half.grad = torch.ones_like(half)
    before = ok.detach().clone()
    refused = optim.AdamW([ok, half], max_grad_norm=5)
    with pytest.raises(ValueError, match=r"parameter 1 .*float16"):
        refused.step()
    torch.cuda.synchronize()
    assert len(refused.state) == 0 and bits_equal(ok.detach(), before), "a refused step changes nothing"
    strided = torch.randn(5, 6, generator=g).to(dev).t().requires_grad_()
    strided.grad = torch.ones_like(strided)
    assert not strided.is_contiguous()
    with pytest.raises(ValueError, match=r"parameter 1 .*not contiguous"):
        optim.AdamW([ok, strided]).step()
    emb = torch.nn.Embedding(7, 3, sparse=True).to(dev)
    emb(torch.tensor([1, 2], device=dev)).sum().backward()
    assert emb.weight.grad.is_sparse
    with pytest.raises(ValueError, match=r"parameter 1 .*sparse"):
        optim.AdamW([ok, emb.weight]).step()
    with pytest.raises(ValueError, match=r"parameter 0 .*sparse"):
        optim.clip_grad_norm_([emb.weight], 5.0)
    assert bits_equal(ok.detach(), before)
    # a non-contiguous gradient is made contiguous: the same bits as the same values behind a contiguous one
    a = torch.nn.Parameter(ok.detach().clone())
    b = torch.nn.Parameter(ok.detach().clone())
    a.grad = ok.grad.clone()
    b.grad = ok.grad.t().contiguous().t()
    assert not b.grad.is_contiguous() and torch.equal(a.grad, b.grad)
    oa, ob = optim.AdamW([a], lr=1e-2, max_grad_norm=1.0), optim.AdamW([b], lr=1e-2, max_grad_norm=1.0)
    oa.step(), ob.step()
    assert bits_equal(a.detach().cpu(), b.detach().cpu()) and bits_equal(oa.grad_norm.cpu(), ob.grad_norm.cpu())
    na, nb = optim.clip_grad_norm_([a], 1.0), optim.clip_grad_norm_([b], 1.0)
    assert bits_equal(na.cpu(), nb.cpu()) and torch.equal(a.grad, b.grad) and not b.grad.is_contiguous()
    assert float(a.grad.norm()) == pytest.approx(1.0, rel=1e-5)


def test_a_non_finite_norm_propagates_as_in_torch(dev):
    p = torch.nn.Parameter(torch.ones(5, device=dev))
    q = torch.nn.Parameter(torch.ones(3, device=dev))
    p.grad = torch.tensor([1.0, float("nan"), 2.0, 3.0, 4.0], device=dev)
    q.grad = torch.ones(3, device=dev)
    tp, tq = (torch.nn.Parameter(t.detach().clone()) for t in (p, q))
    tp.grad, tq.grad = p.grad.clone(), q.grad.clone()
    ref = torch.nn.utils.clip_grad_norm_([tp, tq], 5.0)                # error_if_nonfinite=False
    assert bool(torch.isnan(ref)) and bool(torch.isnan(tp.grad).all()) and bool(torch.isnan(tq.grad).all())
    norm = optim.clip_grad_norm_([p, q], 5.0)
    assert bool(torch.isnan(norm)) and bool(torch.isnan(p.grad).all()) and bool(torch.isnan(q.grad).all()), \
        "as torch: the NaN coefficient reaches every gradient"


def test_step_and_clip_never_synchronise(dev):
    g = torch.Generator().manual_seed(4)
    params = [torch.nn.Parameter(torch.randn(50 + i, generator=g).to(dev)) for i in range(5)]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(dev)
    opt = optim.AdamW(R.make_groups(params), max_grad_norm=R.MAX_NORM)
    opt.step()                                   # state creation
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2 * optim.RING_SLOTS + 1):              # the staging ring wraps twice
            opt.step()
            norm = optim.clip_grad_norm_(params, R.MAX_NORM)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert norm.is_cuda and opt.grad_norm.is_cuda and bool(torch.isfinite(opt.grad_norm))
