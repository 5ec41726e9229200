"""The device-side AdamW step, host half (no GPU): optimizer state moves between ``torch.optim.AdamW`` and ``optim.AdamW`` in both
directions bit for bit, what is not implemented is refused by name, the chunk table covers every element exactly once in an order
the shapes alone decide, the C entries validate before they launch, and ``register_into_mmcv`` registers the class."""
import copy
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
import co_occ_amd as pkg
from co_occ_amd import _lib, optim

import optim_refs as R
import test_abi

ENTRY_POINTS = ("coocc_optim_chunk", "coocc_optim_sumsq", "coocc_optim_clip_coef", "coocc_optim_adamw", "coocc_optim_scale")
one = ctypes.c_void_p(256)          # a non-null aligned dummy address: validation never dereferences device pointers


def same(a, b, path="state_dict"):
    """Equal key for key and bit for bit (tensors: dtype, shape and bytes)."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), "%s: keys %s vs %s" % (path, list(a), list(b) if isinstance(b, dict) else b)
        for k in a:
            same(a[k], b[k], "%s[%r]" % (path, k))
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, "%s[%d]" % (path, i))
    elif torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and a.device == b.device, path
        assert a.numpy().tobytes() == b.numpy().tobytes(), path
    else:
        assert type(a) is type(b) and a == b, "%s: %r vs %r" % (path, a, b)


def _cpu_params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((5,), (3, 4), (2, 1, 3))]


def _stepped_torch(n=2):
    ps = _cpu_params()
    opt = torch.optim.AdamW(R.make_groups(ps))
    g = torch.Generator().manual_seed(9)
    for _ in range(n):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return ps, opt


# ----------------------------------------------------------------------------- state interchange
def test_module_is_imported_by_the_package_and_all_is_unchanged():
    assert pkg.optim is optim and "optim" not in pkg.__all__
    assert issubclass(optim.AdamW, torch.optim.Optimizer)
    assert optim.AdamW.state_dict is torch.optim.Optimizer.state_dict
    assert optim.AdamW.load_state_dict is torch.optim.Optimizer.load_state_dict


def test_torch_checkpoint_loads_and_comes_back_out_bit_for_bit():
    ps, topt = _stepped_torch()
    sd = copy.deepcopy(topt.state_dict())          # as a checkpoint file would hold it: load_state_dict keeps the 'step' tensors it is given
    ours = optim.AdamW(R.make_groups(ps), max_grad_norm=5)          # same CPU parameters, never stepped
    ours.load_state_dict(sd)
    same(sd, ours.state_dict())
    for p in ps:
        st = ours.state[p]
        assert list(st) == ["step", "exp_avg", "exp_avg_sq"] and not st["step"].is_cuda and st["step"].dim() == 0
        assert float(st["step"]) == 2.0 and st["step"].dtype == topt.state[p]["step"].dtype


def test_this_class_checkpoint_loads_into_torch_and_steps_like_the_original():
    ps, topt = _stepped_torch()
    ours = optim.AdamW(R.make_groups(ps))
    ours.load_state_dict(copy.deepcopy(topt.state_dict()))
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    back = torch.optim.AdamW(R.make_groups(ps2))
    back.load_state_dict(copy.deepcopy(ours.state_dict()))
    same(topt.state_dict(), back.state_dict())
    g = torch.Generator().manual_seed(10)
    for p, q in zip(ps, ps2):
        p.grad = torch.randn(p.shape, generator=g)
        q.grad = p.grad.clone()
    topt.step(), back.step()
    same(topt.state_dict(), back.state_dict())
    for p, q in zip(ps, ps2):
        assert torch.equal(p, q)


def test_a_fresh_instance_has_torchs_param_group_keys():
    ps = _cpu_params()
    a, b = optim.AdamW(R.make_groups(ps)).state_dict(), torch.optim.AdamW(R.make_groups(ps)).state_dict()
    same(b, a)
    assert a["state"] == {}


# ----------------------------------------------------------------------------- refusals
def test_what_is_not_implemented_is_refused_by_name():
    ps = _cpu_params()
    for kw, name in ((dict(amsgrad=True), "amsgrad"), (dict(maximize=True), "maximize"), (dict(norm_type=1), "norm_type"),
                     (dict(fused=True), "fused"), (dict(foreach=True), "foreach"), (dict(capturable=True), "capturable"),
                     (dict(differentiable=True), "differentiable")):
        with pytest.raises(NotImplementedError, match=name):
            optim.AdamW(ps, **kw)
    optim.AdamW(ps, foreach=None, fused=False, capturable=False, differentiable=False, amsgrad=False, maximize=False, norm_type=2.0)
    with pytest.raises(NotImplementedError, match="norm_type"):
        optim.clip_grad_norm_(ps, 5.0, norm_type=1)
    with pytest.raises(NotImplementedError, match="norm_type"):
        optim.clip_grad_norm_(ps, 5.0, norm_type=float("inf"))


def test_step_on_cpu_parameters_names_the_parameter():
    ps = _cpu_params()
    opt = optim.AdamW(R.make_groups(ps), max_grad_norm=5)
    ps[1].grad = torch.ones_like(ps[1])                # parameter 0 has no gradient and is skipped: the complaint names 1
    before = [p.detach().clone() for p in ps]
    with pytest.raises(ValueError, match=r"parameter 1 .*HIP device"):
        opt.step()
    assert all(torch.equal(p, b) for p, b in zip(ps, before)) and len(opt.state) == 0, "a refused step changes nothing"
    with pytest.raises(ValueError, match=r"parameter 1 .*HIP device"):
        optim.clip_grad_norm_(ps, 5.0)
    assert torch.equal(ps[1].grad, torch.ones_like(ps[1]))


# ----------------------------------------------------------------------------- the table builder
def _cpu_case_params(chunk, with_grads=True):
    cs = R.cases(chunk)
    ps = [torch.nn.Parameter(torch.zeros(shape), requires_grad=kind != "frozen") for _, shape, kind in cs]
    if with_grads:
        for p, (_, _, kind) in zip(ps, cs):
            if kind not in ("frozen", "late"):
                p.grad = torch.zeros_like(p)
    return cs, ps


def test_chunk_table_covers_every_element_exactly_once():
    chunk = optim.chunk_size()
    assert chunk == _lib.load().coocc_optim_chunk() and chunk > 0 and chunk % 4 == 0
    cs, ps = _cpu_case_params(chunk)
    act = optim.active(ps)
    names = [cs[i][0] for i, _ in act]
    assert "frozen" not in names and "late" not in names and "empty" not in names, "grad is None and numel == 0 are skipped"
    assert len(act) == len(cs) - 3 and [i for i, _ in act] == sorted(i for i, _ in act)
    numels = [p.numel() for _, p in act]
    tab = optim.chunk_table(numels)
    assert tab.dtype == np.int64 and tab.shape == (sum(-(-n // chunk) for n in numels), 2)
    for t, n in enumerate(numels):
        offs = tab[tab[:, 0] == t, 1]
        assert offs.tolist() == list(range(0, n, chunk)), "tensor %d: chunks at every multiple of the chunk size below numel, once" % t
        covered = np.zeros(n, np.int32)
        for o in offs:
            covered[o:min(o + chunk, n)] += 1
        assert (covered == 1).all()
    assert (np.diff(tab[:, 0]) >= 0).all(), "tensors in table order"
    # the multi-chunk members of the set are there
    assert names.index("2chunk+3") >= 0 and (tab[:, 0] == names.index("2chunk+3")).sum() == 3
    assert (tab[:, 0] == names.index("chunk")).sum() == 1 and (tab[:, 0] == names.index("chunk+1")).sum() == 2


def test_chunk_table_depends_on_the_shapes_only():
    chunk = optim.chunk_size()
    _, a = _cpu_case_params(chunk)
    _, b = _cpu_case_params(chunk)
    for p in b:                          # other values, other addresses, same shapes
        if p.grad is not None:
            p.data.normal_(), p.grad.normal_()
    ta = optim.chunk_table([p.numel() for _, p in optim.active(a)])
    tb = optim.chunk_table([p.numel() for _, p in optim.active(b)])
    assert np.array_equal(ta, tb)
    assert np.array_equal(optim.chunk_table([5, 2 * chunk + 3, 1], chunk),
                          np.array([[0, 0], [1, 0], [1, chunk], [1, 2 * chunk], [2, 0]], np.int64))
    assert optim.chunk_table([], chunk).shape == (0, 2) and optim.chunk_table([0, 0], chunk).shape == (0, 2)
    assert np.array_equal(optim.chunk_table([7, 9], 4), np.array([[0, 0], [0, 4], [1, 0], [1, 4], [1, 8]], np.int64))


def test_tensor_table_layout_is_the_headers_struct():
    src = open(os.path.join(ROOT, "include", "coocc_hip.h")).read()
    body = re.search(r"typedef struct coocc_optim_tensor \{(.*?)\} coocc_optim_tensor;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        parts = decl.replace("*", " ").split()
        if parts:
            names += [n.strip() for n in " ".join(parts[1:]).split(",")]
    assert names == list(optim.TENSOR_DTYPE.names)
    assert optim.TENSOR_DTYPE.itemsize == 8 * len(names) == 96, "four pointers, numel and seven doubles, no padding"


# ----------------------------------------------------------------------------- ABI validation
def test_entry_points_are_exported_declared_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    fns = test_abi.header_functions()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), "missing export " + name
        assert name in fns, name + " is not declared in include/coocc_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == fns[name], name
    assert "optim.hip" in __import__("co_occ_amd.build", fromlist=["sources"]).sources()


def _host_table(numels):
    tab = np.zeros(len(numels), optim.TENSOR_DTYPE)
    tab["numel"] = numels
    for k in ("p", "g", "exp_avg", "exp_avg_sq"):
        tab[k] = 256
    tab["bias_correction1"] = tab["bias_correction2"] = 0.5
    return tab


def test_entry_points_validate_before_launching():
    """COOCC_EINVAL (-1) with the entry's own name, before any launch (so without a GPU): null tables, counts that are not positive,
    a chunk count that is not the tensor table's, tensors without elements, null pointers inside the table."""
    lib = _lib.load()
    bad = lambda rc, name: rc == -1 and name in lib.coocc_last_error()
    chunk = lib.coocc_optim_chunk()
    tab = _host_table([5, 2 * chunk + 3])                     # 1 + 3 chunks
    th = ctypes.c_void_p(tab.ctypes.data)
    calls = {
        b"optim_sumsq": lambda t=one, h=th, n=2, c=one, nc=4: lib.coocc_optim_sumsq(t, h, n, c, nc, one, None),
        b"optim_adamw": lambda t=one, h=th, n=2, c=one, nc=4: lib.coocc_optim_adamw(t, h, n, c, nc, one, 0, None),
        b"optim_scale": lambda t=one, h=th, n=2, c=one, nc=4: lib.coocc_optim_scale(t, h, n, c, nc, one, None),
    }
    for name, f in calls.items():
        for kw in (dict(t=None), dict(h=None), dict(c=None)):
            assert bad(f(**kw), name) and b"null table" in lib.coocc_last_error(), (name, kw)
        for kw in (dict(n=0), dict(n=-1), dict(nc=0), dict(nc=-4)):
            assert bad(f(**kw), name), (name, kw)
        for nc in (3, 5):
            assert bad(f(nc=nc), name) and b"chunk count" in lib.coocc_last_error(), (name, nc)
        empty = _host_table([5, 0])
        assert bad(f(h=ctypes.c_void_p(empty.ctypes.data), nc=1), name) and b"numel" in lib.coocc_last_error(), name
        nullg = _host_table([5, 2 * chunk + 3])
        nullg["g"][1] = 0
        assert bad(f(h=ctypes.c_void_p(nullg.ctypes.data)), name) and b"gradient pointer" in lib.coocc_last_error(), name
    assert bad(lib.coocc_optim_sumsq(one, th, 2, one, 4, None, None), b"optim_sumsq")
    assert bad(lib.coocc_optim_scale(one, th, 2, one, 4, None, None), b"optim_scale")
    nullm = _host_table([5])
    nullm["exp_avg_sq"] = 0
    assert bad(lib.coocc_optim_adamw(one, ctypes.c_void_p(nullm.ctypes.data), 1, one, 1, None, 0, None), b"optim_adamw")
    nobc = _host_table([5])
    nobc["bias_correction1"] = 0.0                            # a step count of 0
    assert bad(lib.coocc_optim_adamw(one, ctypes.c_void_p(nobc.ctypes.data), 1, one, 1, None, 0, None), b"optim_adamw")
    assert b"bias corrections" in lib.coocc_last_error()
    for args in ((None, 4, 5.0, one, one, one), (one, 4, 5.0, None, one, one), (one, 4, 5.0, one, None, one), (one, 4, 5.0, one, one, None),
                 (one, 0, 5.0, one, one, one), (one, -1, 5.0, one, one, one), (one, 4, 0.0, one, one, one)):
        assert bad(lib.coocc_optim_clip_coef(*args, None), b"optim_clip_coef"), args


# ----------------------------------------------------------------------------- mmcv registration
class _FakeRegistry:
    def __init__(self):
        self.module_dict = {}

    def register_module(self, name=None, force=False, module=None):
        if name in self.module_dict and not force:
            raise KeyError(name)
        self.module_dict[name] = module
        return module


def test_register_into_mmcv(monkeypatch):
    assert "mmcv" not in sys.modules
    assert optim.register_into_mmcv() is False, "mmcv is not importable here"
    builder = types.ModuleType("mmcv.runner.optimizer.builder")
    builder.OPTIMIZERS = _FakeRegistry()
    builder.OPTIMIZERS.module_dict["AdamW"] = torch.optim.AdamW          # what mmcv registers from torch.optim
    mods = [("mmcv", types.ModuleType("mmcv")), ("mmcv.runner", types.ModuleType("mmcv.runner")),
            ("mmcv.runner.optimizer", types.ModuleType("mmcv.runner.optimizer")), ("mmcv.runner.optimizer.builder", builder)]
    for name, mod in mods:
        monkeypatch.setitem(sys.modules, name, mod)
    sys.modules["mmcv"].runner = sys.modules["mmcv.runner"]
    sys.modules["mmcv.runner"].optimizer = sys.modules["mmcv.runner.optimizer"]
    sys.modules["mmcv.runner.optimizer"].builder = builder
    assert optim.register_into_mmcv() is True
    assert builder.OPTIMIZERS.module_dict["AdamW"] is optim.AdamW
    # what DefaultOptimizerConstructor does with optimizer=dict(type='AdamW', lr=1e-4, weight_decay=0.01, max_grad_norm=5) and a
    # paramwise_cfg: one group per parameter, the remaining keys as constructor arguments
    ps = _cpu_params()
    groups = [dict(params=[p], lr=1e-4, weight_decay=0.0 if i == 1 else 0.01) for i, p in enumerate(ps)]
    opt = builder.OPTIMIZERS.module_dict["AdamW"](groups, lr=1e-4, weight_decay=0.01, max_grad_norm=5)
    assert opt.max_grad_norm == 5.0 and len(opt.param_groups) == 3 and opt.param_groups[1]["weight_decay"] == 0.0


def test_registration_is_never_done_at_import():
    init = open(pkg.__file__).read()
    assert "register_into_mmcv" not in init and "from . import optim" in init
