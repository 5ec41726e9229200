"""The parameter update on the device: AdamW with gradient-norm clipping in at most three launches for the whole model, whatever
its param groups look like (csrc/optim.hip).

mmcv's ``DefaultOptimizerConstructor`` gives every parameter its own group as soon as a ``paramwise_cfg`` is present, torch's AdamW
(foreach or fused) works group by group, and mmcv's ``OptimizerHook`` reads the gradient norm to the host every step.  Here the host
fills two small tables per step -- one entry per parameter that has a gradient (pointers, numel, that parameter's own
hyper-parameters and bias corrections) and one per chunk of ``chunk_size()`` elements -- uploads them with one asynchronous copy, and
launches ``k_optim_sumsq`` -> ``k_optim_clip_coef`` -> ``k_optim_adamw`` (the last one alone without clipping).  Sums are fp64 in
an order that depends on the shapes only; nothing is read back to the host.

    opt = optim.AdamW(params_or_groups, lr=1e-4, weight_decay=0.01, max_grad_norm=5)
    loss.backward(); opt.step(); opt.grad_norm          # fp32 0-dim device tensor

``clip_grad_norm_`` is the stand-alone clip for a torch optimizer or mmcv's hook; ``register_into_mmcv`` puts ``AdamW`` into mmcv's
``OPTIMIZERS`` registry.  There is no CPU path: ``step()`` on CPU parameters raises.
"""
import ctypes
import importlib

import numpy as np
import torch

from . import _lib

# struct coocc_optim_tensor (include/coocc_hip.h): 4 pointers, numel, 7 doubles = 96 bytes
TENSOR_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("numel", "<i8"), ("lr", "<f8"),
                         ("weight_decay", "<f8"), ("beta1", "<f8"), ("beta2", "<f8"), ("eps", "<f8"), ("bias_correction1", "<f8"),
                         ("bias_correction2", "<f8")])
RING_SLOTS = 4

_chunk = None


def chunk_size():
    """Elements per chunk (``coocc_optim_chunk``): a compile-time constant of the library and part of the determinism contract."""
    global _chunk
    if _chunk is None:
        _chunk = int(_lib.load().coocc_optim_chunk())
    return _chunk


def active(params):
    """``[(index, parameter)]`` of the tensor table's members, in the order given: the parameters that have a gradient and at least
    one element.  Which ones they are depends on ``.grad is None`` and the shapes alone, never on values."""
    return [(i, p) for i, p in enumerate(params) if p.grad is not None and p.numel() > 0]


_chunk_cache = {}


def chunk_table(numels, chunk=None):
    """The chunk table of tensors with these element counts: int64 ``[nchunks, 2]`` rows (position in ``numels``, element offset),
    tensors in the order given, offsets ascending in steps of ``chunk``.  Tensors without elements get no row.  A function of the
    shapes only (and cached by them)."""
    chunk = chunk_size() if chunk is None else int(chunk)
    key = (chunk, tuple(numels))
    tab = _chunk_cache.get(key)
    if tab is None:
        n = np.asarray(key[1], dtype=np.int64).reshape(-1)
        counts = (n + chunk - 1) // chunk
        ti = np.repeat(np.arange(n.size, dtype=np.int64), counts)
        first = np.cumsum(counts) - counts
        off = (np.arange(int(counts.sum()), dtype=np.int64) - np.repeat(first, counts)) * chunk
        tab = np.stack([ti, off], 1) if ti.size else np.zeros((0, 2), np.int64)
        tab.setflags(write=False)
        if len(_chunk_cache) > 64:
            _chunk_cache.clear()
        _chunk_cache[key] = tab
    return tab


class _Slot:
    def __init__(self, cap, device):
        self.host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
        self.dev = torch.empty(cap, dtype=torch.uint8, device=device)
        self.np = self.host.numpy()
        self.event = torch.cuda.Event()


class _Ring:
    """Pinned staging buffers for the tables, ``RING_SLOTS`` of them per device, each with its device twin and an event recorded
    behind the last kernel that reads the twin.  A slot is rewritten only after its event has completed: the host never touches
    bytes a queued copy has not consumed.  In steady state that event is RING_SLOTS - 1 steps old and long complete."""

    def __init__(self, device):
        self.device, self.slots, self.i = device, [None] * RING_SLOTS, 0

    def acquire(self, nbytes):
        k = self.i
        self.i = (k + 1) % RING_SLOTS
        s = self.slots[k]
        if s is not None:
            s.event.synchronize()
        if s is None or s.host.numel() < nbytes:
            s = self.slots[k] = _Slot(max(4096, 1 << (int(nbytes) - 1).bit_length()), self.device)
        return s


_rings = {}


def _ring(device):
    r = _rings.get(device.index)
    if r is None:
        r = _rings[device.index] = _Ring(device)
    return r


def _refuse(i, why):
    raise ValueError("co_occ_amd.optim: parameter %d %s" % (i, why))


def _check_param(i, p, device):
    """The parameter's gradient as the kernels can read it (made contiguous when it is not), or a ValueError naming ``i``."""
    if not p.is_cuda:
        _refuse(i, "is on %s, not on a HIP device (there is no CPU path)" % p.device)
    if p.dtype is not torch.float32:
        _refuse(i, "is %s (only float32 parameters are updated)" % p.dtype)
    if not p.is_contiguous():
        _refuse(i, "is not contiguous")
    if p.device != device:
        _refuse(i, "is on %s, the first parameter on %s (one device per step)" % (p.device, device))
    g = p.grad
    if g.is_sparse:
        _refuse(i, "has a sparse gradient")
    if g.dtype is not torch.float32 or g.device != p.device or g.shape != p.shape:
        _refuse(i, "has a gradient of %s %s on %s (float32, the parameter's shape and device)" % (g.dtype, tuple(g.shape), g.device))
    return g if g.is_contiguous() else g.contiguous()


class _Tables:
    """The two tables of one step on the device: ``slot.dev`` holds the tensor table, then the chunk table."""

    def __init__(self, device, cols, numels):
        chunks = chunk_table(numels)
        self.ntensors, self.nchunks = len(numels), int(chunks.shape[0])
        tbytes = self.ntensors * TENSOR_DTYPE.itemsize
        total = tbytes + chunks.nbytes
        self.slot = s = _ring(device).acquire(total)
        tab = s.np[:tbytes].view(TENSOR_DTYPE)
        tab["numel"] = numels
        for name, col in cols.items():
            tab[name] = col
        for name in TENSOR_DTYPE.names:
            if name != "numel" and name not in cols:
                tab[name] = 0
        s.np[tbytes:total] = chunks.reshape(-1).view(np.uint8)
        s.dev[:total].copy_(s.host[:total], non_blocking=True)           # the one upload of the step, on the current stream
        self.tensors = _lib.ptr(s.dev)
        self.tensors_host = ctypes.c_void_p(s.host.data_ptr())
        self.chunks = _lib.ptr(s.dev, offset=tbytes)
        self.elements = float(sum(numels))

    def done(self):
        self.slot.event.record()


def _norm_and_coef(t, max_norm, device):
    """k_optim_sumsq + k_optim_clip_coef over the tables ``t``: (fp32 0-dim norm, pointer to the fp32 coefficient)."""
    partials = torch.empty(t.nchunks, dtype=torch.float64, device=device)
    stats = torch.empty(2, dtype=torch.float64, device=device)         # [0] the fp64 norm; [1] as two floats: norm, coefficient
    f32 = stats.view(torch.float32)
    with _lib.TIMER.region("k_optim_sumsq", 4.0 * t.elements):
        _lib.call("coocc_optim_sumsq", t.tensors, t.tensors_host, t.ntensors, t.chunks, t.nchunks, _lib.ptr(partials))
    with _lib.TIMER.region("k_optim_clip_coef", 8.0 * t.nchunks):
        _lib.call("coocc_optim_clip_coef", _lib.ptr(partials), t.nchunks, float(max_norm), _lib.ptr(stats), _lib.ptr(f32, offset=2),
                  _lib.ptr(f32, offset=3))
    return f32[2], _lib.ptr(f32, offset=3)


def _torch_defaults():
    """The param-group keys of this torch's AdamW that this class has no use for, at the values it accepts: a state_dict of either
    class then loads into the other."""
    d = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)
    try:
        probe = torch.optim.AdamW([torch.zeros(1, requires_grad=True)])
        if "decoupled_weight_decay" in probe.defaults:
            d["decoupled_weight_decay"] = True
    except Exception:
        pass
    return d


def _step_dtype():
    """The dtype torch gives a non-capturable optimizer's ``step`` tensors."""
    try:
        from torch.optim.optimizer import _get_scalar_dtype
    except ImportError:
        return torch.float32
    return _get_scalar_dtype()


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (non-amsgrad) with ``clip_grad_norm_(max_grad_norm)`` fused in front, on the HIP engine.

    The constructor is torch's plus ``max_grad_norm`` (None: no clipping) and ``norm_type`` (2 only).  Param groups of any shape
    work, one group per parameter included; ``lr``, ``weight_decay``, ``betas`` and ``eps`` are read per group at every step, so LR
    schedulers work unchanged.  State lives in ``self.state[p]`` under torch's keys (``step`` a CPU scalar tensor, ``exp_avg``,
    ``exp_avg_sq``): ``state_dict()`` / ``load_state_dict()`` are the inherited ones and checkpoints move between this class and
    ``torch.optim.AdamW`` in both directions.

    ``step()`` makes no device-to-host read.  With clipping, ``self.grad_norm`` is afterwards the fp32 0-dim device tensor of this
    step's total gradient norm (None without clipping, or when no parameter had a gradient).

    The fused clip leaves ``.grad`` UNSCALED: the coefficient is applied in registers on the way into the moments.  Code that
    reads ``.grad`` after ``step()`` and expects clipped values sets ``opt.write_clipped_grad = True`` (4 more bytes per element)
    or uses :func:`clip_grad_norm_`."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None, max_grad_norm=None, norm_type=2):
        if amsgrad:
            raise NotImplementedError("co_occ_amd.optim.AdamW: amsgrad=True is not implemented")
        if maximize:
            raise NotImplementedError("co_occ_amd.optim.AdamW: maximize=True is not implemented")
        if float(norm_type) != 2.0:
            raise NotImplementedError("co_occ_amd.optim.AdamW: norm_type=%r is not implemented (the 2-norm only)" % (norm_type,))
        for name, v in (("foreach", foreach), ("fused", fused), ("capturable", capturable), ("differentiable", differentiable)):
            if v:
                raise NotImplementedError("co_occ_amd.optim.AdamW: %s=%r has no meaning here (this class is its own fused "
                                          "implementation); pass None or False" % (name, v))
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("Invalid beta parameters: %r" % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("Invalid max_grad_norm: %r (positive, or None for no clipping)" % (max_grad_norm,))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.norm_type = 2.0
        self.write_clipped_grad = False
        self.grad_norm = None
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, **_torch_defaults()))

    def _gather(self):
        """One pass over the param groups that changes nothing: ``[(parameter, contiguous gradient, lr, wd, b1, b2, eps)]`` of the
        parameters that have a gradient, every one checked, and their device."""
        work, device, i = [], None, -1
        for group in self.param_groups:
            for key in ("amsgrad", "maximize"):
                if group.get(key):
                    raise NotImplementedError("co_occ_amd.optim.AdamW: a param group has %s=True" % key)
            if not group.get("decoupled_weight_decay", True):
                raise NotImplementedError("co_occ_amd.optim.AdamW: a param group has decoupled_weight_decay=False (that is Adam)")
            lr, wd, eps = float(group["lr"]), float(group["weight_decay"]), float(group["eps"])
            b1, b2 = (float(b) for b in group["betas"])
            for p in group["params"]:
                i += 1
                if p.grad is None:
                    continue
                if device is None and p.is_cuda:
                    device = p.device
                g = _check_param(i, p, device)
                st = self.state.get(p)
                if st:
                    if st["step"].is_cuda:
                        _refuse(i, "keeps its step count on the device (a capturable checkpoint); this class keeps it on the host")
                    for name in ("exp_avg", "exp_avg_sq"):
                        s = st[name]
                        if s.dtype is not torch.float32 or s.device != p.device or s.shape != p.shape or not s.is_contiguous():
                            _refuse(i, "has a state tensor %s that is not a contiguous float32 tensor of its shape on its device" % name)
                work.append((p, g, lr, wd, b1, b2, eps))
        return device, work

    @torch.no_grad()
    def step(self, closure=None):
        """One clipped AdamW step over every parameter that has a gradient.  Parameters whose ``.grad`` is None are skipped: their
        state and step count stay untouched and they do not enter the norm."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.grad_norm = None
        device, work = self._gather()
        cols = {k: [] for k in TENSOR_DTYPE.names if k != "numel"}
        numels = []
        for p, g, lr, wd, b1, b2, eps in work:
            st = self.state[p]
            if len(st) == 0:                       # torch's keys and torch's types: checkpoints move both ways
                st["step"] = torch.tensor(0.0, dtype=_step_dtype())
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            step = st["step"]
            step += 1
            n = p.numel()
            if n == 0:
                continue
            t = float(step)
            numels.append(n)
            cols["p"].append(p.data_ptr())
            cols["g"].append(g.data_ptr())
            cols["exp_avg"].append(st["exp_avg"].data_ptr())
            cols["exp_avg_sq"].append(st["exp_avg_sq"].data_ptr())
            cols["lr"].append(lr)
            cols["weight_decay"].append(wd)
            cols["beta1"].append(b1)
            cols["beta2"].append(b2)
            cols["eps"].append(eps)
            cols["bias_correction1"].append(1.0 - b1 ** t)               # float64, from this parameter's own count
            cols["bias_correction2"].append(1.0 - b2 ** t)
        if not numels:
            return loss
        clip = self.max_grad_norm is not None
        with torch.cuda.device(device):
            t = _Tables(device, cols, numels)
            coef = ctypes.c_void_p(0)
            if clip:
                self.grad_norm, coef = _norm_and_coef(t, self.max_grad_norm, device)
            write = 1 if clip and self.write_clipped_grad else 0
            with _lib.TIMER.region("k_optim_adamw", (32.0 if write else 28.0) * t.elements):
                _lib.call("coocc_optim_adamw", t.tensors, t.tensors_host, t.ntensors, t.chunks, t.nchunks, coef, write)
            t.done()
        # the kernels wrote through raw pointers: move the version counters as an in-place torch op would (core.PackCache re-packs
        # the engine's weights by them; autograd's checks of saved tensors read them too)
        touched = []
        for p, g, *_ in work:
            if p.numel():
                st = self.state[p]
                touched += [p, st["exp_avg"], st["exp_avg_sq"]] + ([g] if write else [])
        torch.autograd.graph.increment_version(touched)
        if write:
            for p, g, *_ in work:
                if g is not p.grad:            # a non-contiguous gradient was clipped in its contiguous copy
                    p.grad.copy_(g)
        del work                                  # the contiguous copies of strided gradients lived until the launches were issued
        return loss


def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """torch.nn.utils.clip_grad_norm_ on the HIP engine, for a torch optimizer or mmcv's ``OptimizerHook``: the 2-norm of all
    gradients (fp64 sums in a shape-only order, ``k_optim_sumsq`` + ``k_optim_clip_coef``), then ``.grad *= min(1, max_norm /
    (norm + 1e-6))`` in place (``k_optim_scale``).  Returns the norm as an fp32 0-dim DEVICE tensor and makes no host read; a
    non-finite norm propagates into the gradients as with ``error_if_nonfinite=False``."""
    if float(norm_type) != 2.0:
        raise NotImplementedError("co_occ_amd.optim.clip_grad_norm_: norm_type=%r is not implemented (the 2-norm only)" % (norm_type,))
    if not float(max_norm) > 0.0:
        raise ValueError("co_occ_amd.optim.clip_grad_norm_: max_norm=%r (positive)" % (max_norm,))
    params = [parameters] if torch.is_tensor(parameters) else list(parameters)
    device, numels, ptrs, grads = None, [], [], []
    for i, p in active(params):
        if device is None and p.is_cuda:
            device = p.device
        g = _check_param(i, p, device)
        numels.append(p.numel())
        ptrs.append(g.data_ptr())
        grads.append((p.grad, g))
    if not numels:
        return torch.zeros((), device=device) if device is not None else torch.zeros(())
    with torch.no_grad(), torch.cuda.device(device):
        t = _Tables(device, dict(g=ptrs), numels)
        norm, coef = _norm_and_coef(t, max_norm, device)
        with _lib.TIMER.region("k_optim_scale", 8.0 * t.elements):
            _lib.call("coocc_optim_scale", t.tensors, t.tensors_host, t.ntensors, t.chunks, t.nchunks, coef)
        t.done()
        torch.autograd.graph.increment_version([g for _, g in grads])      # written through raw pointers
        for grad, g in grads:
            if g is not grad:                # a non-contiguous gradient was scaled in its contiguous copy
                grad.copy_(g)
    return norm


def register_into_mmcv():
    """Register :class:`AdamW` under the name ``AdamW`` (``force=True``) into mmcv's ``OPTIMIZERS`` registry
    (``mmcv.runner.optimizer.builder``), so that ``optimizer=dict(type='AdamW', ..., max_grad_norm=5)`` with
    ``optimizer_config=dict(grad_clip=None)`` builds this class through ``DefaultOptimizerConstructor``, ``paramwise_cfg`` included.
    Called explicitly, never at import.  Returns False when mmcv cannot be imported."""
    try:
        builder = importlib.import_module("mmcv.runner.optimizer.builder")
        registry = builder.OPTIMIZERS
    except Exception:
        return False
    registry.register_module(name="AdamW", force=True, module=AdamW)
    return True
