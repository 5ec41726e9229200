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

With ``process_group=`` the step is data-parallel: ``k_optim_pack`` writes every gradient divided by the group's
size into one persistent arena, ONE ``all_reduce`` sums the arena over the ranks, ``k_optim_flag_check`` counts the tensors that had
a gradient on some ranks only, and the three kernels above read the averaged gradients from the arena in place.
``all_reduce_gradients`` is the average alone (pack, all-reduce, ``k_optim_unpack`` back into ``.grad``) and
``broadcast_parameters`` starts the replicas from one rank's weights.

    dist.init_process_group('nccl'); model = build(); optim.broadcast_parameters(model)
    opt = optim.AdamW(params_or_groups, lr=1e-4, max_grad_norm=5, process_group=True)
"""
import collections
import ctypes
import hashlib
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


# ------------------------------------------------------------------ data-parallel gradient averaging
Layout = collections.namedtuple("Layout", "numels header offsets total")
_layout_cache = {}


def arena_layout(numels):
    """Where the tensors with these element counts live in the arena: ``Layout(numels, header, offsets, total)``, all in fp32
    elements.  The arena starts with ``header`` floats, one presence flag per tensor that has elements; tensor ``i``'s segment
    starts at ``offsets[i]``, a multiple of 4 (so every segment is 16-byte aligned), segments ascending in the order given and
    never overlapping; a tensor without elements gets no segment (offset -1) and no flag.  ``total`` is the arena's length.  A
    function of the element counts only (and cached by them): every rank that holds the same shapes computes the same layout."""
    key = tuple(int(n) for n in numels)
    lay = _layout_cache.get(key)
    if lay is None:
        n = np.asarray(key, dtype=np.int64).reshape(-1)
        if (n < 0).any():
            raise ValueError("co_occ_amd.optim: a negative element count")
        header = int((n > 0).sum())
        padded = (n + 3) // 4 * 4
        first = (header + 3) // 4 * 4
        offsets = np.where(n > 0, first + np.cumsum(padded) - padded, -1).astype(np.int64)
        offsets.setflags(write=False)
        lay = Layout(key, header, offsets, int(first + padded.sum()))
        if len(_layout_cache) > 64:
            _layout_cache.clear()
        _layout_cache[key] = lay
    return lay


def fingerprint(numels):
    """What the ranks compare before their first collective: (tensor count, total element count, a 62-bit hash of the element
    counts in order).  Three int64, whatever the model's size."""
    n = [int(v) for v in numels]
    h = hashlib.blake2b(np.asarray(n, dtype="<i8").tobytes(), digest_size=8).digest()
    return len(n), sum(n), int.from_bytes(h, "little") >> 2


def _check_group_arg(pg, who):
    if pg is None or pg is True or pg == "world" or (hasattr(pg, "size") and hasattr(pg, "rank")):
        return pg
    raise ValueError("co_occ_amd.optim.%s: process_group=%r (None, True or 'world' for the default group, or a "
                     "torch.distributed ProcessGroup)" % (who, pg))


def _resolve_group(pg, who):
    """(group, its size) of ``True`` / ``'world'`` (the default group) or a ProcessGroup object."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("co_occ_amd.optim.%s: a process group was asked for, but torch.distributed is not initialised "
                           "(call init_process_group first)" % who)
    group = dist.group.WORLD if pg is True or pg == "world" else pg
    return group, int(dist.get_world_size(group))


def _check_layout_tensor(i, p, device):
    if not p.is_cuda:
        _refuse(i, "is on %s, not on a HIP device (there is no CPU path)" % p.device)
    if p.dtype is not torch.float32:
        _refuse(i, "is %s (only float32 parameters are updated)" % p.dtype)
    if not p.is_contiguous():
        _refuse(i, "is not contiguous")
    if p.device != device:
        _refuse(i, "is on %s, the first parameter on %s (one device per step)" % (p.device, device))


class _Reducer:
    """One tensor list's arena: the layout, the persistent fp32 buffer (allocated at first use, padding zeroed then and never
    written again), the sticky mismatch word, and the three launches around the collective."""

    def __init__(self, tensors, indices, device):
        self.tensors, self.indices, self.device = list(tensors), list(indices), device
        self.numels = [int(t.numel()) for t in self.tensors]
        self.layout = arena_layout(self.numels)
        self.slot = {id(t): k for k, t in enumerate(self.tensors)}
        self.arena = None
        self.mismatch = None
        self.checked = False

    def buffer(self):
        if self.arena is None:
            self.arena = torch.zeros(self.layout.total, dtype=torch.float32, device=self.device)
        if self.mismatch is None:
            self.mismatch = torch.zeros((), dtype=torch.int32, device=self.device)
        return self.arena

    def release(self):
        self.arena = None

    def seg(self, k):
        return self.buffer().data_ptr() + 4 * int(self.layout.offsets[k])

    def check_fingerprint(self, group, world, extra=()):
        """The one host read: every rank's fingerprint summed into its own row of a [world, 3] int64 table.  Every rank sees the
        same table and raises, or not, together."""
        import torch.distributed as dist
        mine = fingerprint(list(self.numels) + list(extra))
        table = torch.zeros(world, 3, dtype=torch.int64, device=self.device)
        table[dist.get_rank(group)] = torch.tensor(mine, dtype=torch.int64)
        dist.all_reduce(table, group=group)
        rows = [tuple(r) for r in table.tolist()]
        if any(r != rows[0] for r in rows):
            raise ValueError("co_occ_amd.optim: this rank presents %d tensors with %d elements (hash %x), but the ranks of the "
                             "group do not agree: (tensors, elements, hash) per rank = %s.  Every rank must hold the same "
                             "parameters with requires_grad, in the same order" % (mine[0], mine[1], mine[2], rows))
        self.checked = True

    def pack(self, sources, world):
        """k_optim_pack: ``sources[k]`` (a contiguous fp32 tensor or None) / world into segment k.  Returns the tables; the caller
        calls ``done()`` on them behind the last launch that reads them."""
        arena = self.buffer()
        n = len(self.tensors)
        cols = dict(p=[self.seg(k) for k in range(n)], g=[0 if s is None else s.data_ptr() for s in sources])
        t = _Tables(self.device, cols, self.numels)
        with _lib.TIMER.region("k_optim_pack", 8.0 * t.elements):
            _lib.call("coocc_optim_pack", t.tensors, t.tensors_host, t.ntensors, t.chunks, t.nchunks, _lib.ptr(arena),
                      arena.numel(), int(world))
        return t

    def reduce(self, t, group, world):
        """The all-reduce of the whole arena (skipped without a group) and k_optim_flag_check over pack's tables ``t``."""
        arena = self.buffer()
        if group is not None:
            import torch.distributed as dist
            dist.all_reduce(arena, group=group)
        with _lib.TIMER.region("k_optim_flag_check", 4.0 * t.ntensors):
            _lib.call("coocc_optim_flag_check", t.tensors, t.ntensors, _lib.ptr(arena), int(world), _lib.ptr(self.mismatch))
        t.done()

    def unpack(self, pairs):
        """k_optim_unpack: segment k -> ``dst`` for every (k, dst) of ``pairs`` (ascending k; dst contiguous fp32)."""
        if not pairs:
            return
        arena = self.buffer()
        cols = dict(p=[d.data_ptr() for _, d in pairs], g=[self.seg(k) for k, _ in pairs])
        t = _Tables(self.device, cols, [self.numels[k] for k, _ in pairs])
        with _lib.TIMER.region("k_optim_unpack", 8.0 * t.elements):
            _lib.call("coocc_optim_unpack", t.tensors, t.tensors_host, t.ntensors, t.chunks, t.nchunks, _lib.ptr(arena),
                      arena.numel())
        t.done()


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
    or uses :func:`clip_grad_norm_`.

    ``process_group`` (None: this rank alone, as ever) makes the step data-parallel: ``True`` or ``'world'`` is the default group,
    resolved at the first step, a ``ProcessGroup`` object is used as given.  Every gradient is divided by the group's size and
    packed into one persistent fp32 arena (``k_optim_pack``), the arena is all-reduced in ONE collective on the current stream, and
    the norm and the update read the averaged gradients from the arena in place.  The arena holds every parameter with
    ``requires_grad`` and elements, in group order -- as many bytes as the parameters themselves, 819 MB for the r50 detector --
    and lives as long as the optimizer; ``release_arena()`` frees it (the next step allocates it again).  The contract is
    DistributedDataParallel's default one: every rank presents the same set of gradients.  A rank whose ``.grad`` is None packs
    zeros, so the collective has the same size on every rank and cannot hang; the disagreement is counted into ``grad_mismatch``, a
    sticky int32 device word the caller reads when it chooses.  Which parameters are stepped stays this rank's own ``.grad is
    None``.  ``grad_norm`` is the norm of the AVERAGED gradient, the same bits on every rank.  ``.grad`` keeps this rank's own
    values unless ``write_reduced_grad`` is set: then the averaged gradients are copied back (``k_optim_unpack``), clipped when
    ``write_clipped_grad`` is set too (which alone writes nothing under a group).  The first data-parallel step compares a
    fingerprint of the layout across the ranks (one host read) and raises ValueError on every rank if they differ; later steps
    make no device-to-host read.  A group of one rank takes the single-rank path unless ``dp_always`` is set, which runs pack, the
    norm and the update through the arena and skips only the collective (for tests and timings on one GPU)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None, max_grad_norm=None, norm_type=2,
                 process_group=None):
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
        self.process_group = _check_group_arg(process_group, "AdamW")
        self.dp_always = False
        self.write_reduced_grad = False
        self._reducer = None
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
        dp = self._dp_mode()
        device, work = self._gather()
        if dp is not None:
            self._step_dp(device, work, *dp)
            return loss
        cols, numels = self._advance(work, lambda p, g: g.data_ptr())
        if not numels:
            return loss
        clip = self.max_grad_norm is not None
        with torch.cuda.device(device):
            t = _Tables(device, cols, numels)
            write = self._update(t, clip and self.write_clipped_grad, device)
            t.done()
        self._finish(work, write)
        return loss

    def _advance(self, work, gptr):
        """Create the missing state, count the step of every parameter of ``work`` and fill the tensor table's columns;
        ``gptr(p, g)`` is the address the kernels read the gradient from."""
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
            cols["g"].append(gptr(p, g))
            cols["exp_avg"].append(st["exp_avg"].data_ptr())
            cols["exp_avg_sq"].append(st["exp_avg_sq"].data_ptr())
            cols["lr"].append(lr)
            cols["weight_decay"].append(wd)
            cols["beta1"].append(b1)
            cols["beta2"].append(b2)
            cols["eps"].append(eps)
            cols["bias_correction1"].append(1.0 - b1 ** t)               # float64, from this parameter's own count
            cols["bias_correction2"].append(1.0 - b2 ** t)
        return cols, numels

    def _update(self, t, write, device):
        """k_optim_sumsq -> k_optim_clip_coef (with clipping) -> k_optim_adamw over the tables ``t``.  Returns ``write`` as the
        kernel took it: 1 when the clipped gradient was stored back to where it was read from."""
        coef = ctypes.c_void_p(0)
        if self.max_grad_norm is not None:
            self.grad_norm, coef = _norm_and_coef(t, self.max_grad_norm, device)
        write = 1 if write else 0
        with _lib.TIMER.region("k_optim_adamw", (32.0 if write else 28.0) * t.elements):
            _lib.call("coocc_optim_adamw", t.tensors, t.tensors_host, t.ntensors, t.chunks, t.nchunks, coef, write)
        return write

    def _finish(self, work, wrote_grad):
        # the kernels wrote through raw pointers: move the version counters as an in-place torch op would (core.PackCache re-packs
        # the engine's weights by them; autograd's checks of saved tensors read them too)
        touched = []
        for p, g, *_ in work:
            if p.numel():
                st = self.state[p]
                touched += [p, st["exp_avg"], st["exp_avg_sq"]] + ([g] if wrote_grad else [])
        torch.autograd.graph.increment_version(touched)
        if wrote_grad:
            for p, g, *_ in work:
                if g is not p.grad:            # a non-contiguous gradient was written in its contiguous copy
                    p.grad.copy_(g)

    # ------------------------------------------------------------------ the data-parallel step
    @property
    def grad_mismatch(self):
        """The sticky int32 0-dim device word: how many (step, tensor) pairs so far had a gradient on some ranks of the group and
        none on others.  None before the first data-parallel step.  Reading it is the caller's host read."""
        return None if self._reducer is None else self._reducer.mismatch

    def release_arena(self):
        """Free the arena (as many bytes as the trainable parameters).  The layout and ``grad_mismatch`` stay; the next
        data-parallel step allocates the arena again."""
        if self._reducer is not None:
            self._reducer.release()

    def _dp_mode(self):
        """None: the single-rank path.  Else (group or None, world): the arena path, without the collective when group is None."""
        if self.process_group is None:
            return (None, 1) if self.dp_always else None
        group, world = _resolve_group(self.process_group, "AdamW")
        if world == 1:
            return (None, 1) if self.dp_always else None
        return group, world

    def _layout_reducer(self):
        """The reducer over this optimizer's layout -- the parameters with requires_grad and elements, in group order -- made at
        the first data-parallel step; afterwards a changed layout raises."""
        tensors, indices, i = [], [], -1
        for group in self.param_groups:
            for p in group["params"]:
                i += 1
                if p.requires_grad and p.numel() > 0:
                    tensors.append(p)
                    indices.append(i)
                elif p.grad is not None and p.numel() > 0:
                    _refuse(i, "has a gradient but requires_grad=False: it is outside the data-parallel layout, which every rank "
                               "derives from requires_grad alone")
        red = self._reducer
        if red is None:
            if not tensors:
                return None
            device = tensors[0].device
            for i, p in zip(indices, tensors):
                _check_layout_tensor(i, p, device)
            red = self._reducer = _Reducer(tensors, indices, device)
        elif len(tensors) != len(red.tensors) or any(a is not b for a, b in zip(tensors, red.tensors)):
            k = next((k for k, (a, b) in enumerate(zip(tensors, red.tensors)) if a is not b), min(len(tensors), len(red.tensors)))
            where = min(indices[k] if k < len(indices) else red.indices[k], red.indices[k] if k < len(red.indices) else indices[k])
            raise ValueError("co_occ_amd.optim: parameter %d: the parameters with requires_grad changed after the first "
                             "data-parallel step (%d tensors then, %d now); the arena's layout is fixed, build a new optimizer"
                             % (where, len(red.tensors), len(tensors)))
        return red

    def _step_dp(self, device, work, group, world):
        red = self._layout_reducer()
        if red is None:
            return
        if group is not None and not red.checked:
            red.check_fingerprint(group, world)              # raises on every rank or on none, before anything is changed
        device = red.device
        sources = [None] * len(red.tensors)
        for p, g, *_ in work:
            if p.numel():
                sources[red.slot[id(p)]] = g
        cols, numels = self._advance(work, lambda p, g: red.seg(red.slot[id(p)]))
        write = 0
        with torch.cuda.device(device):
            red.reduce(red.pack(sources, world), group, world)
            if numels:
                t = _Tables(device, cols, numels)
                write = self._update(t, self.max_grad_norm is not None and self.write_clipped_grad and self.write_reduced_grad, device)
                t.done()
            if self.write_reduced_grad:
                red.unpack([(k, s) for k, s in enumerate(sources) if s is not None])
        self._finish(work, self.write_reduced_grad)


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


_reducers = collections.OrderedDict()


def all_reduce_gradients(parameters, group=None):
    """Average the gradients of ``parameters`` over the ranks of ``group`` (None: the default group) in place, for a torch
    optimizer or mmcv's ``OptimizerHook``: ``k_optim_pack`` (``.grad / world`` into one arena), ONE all-reduce, ``k_optim_unpack``
    back into ``.grad``.  The layout is :class:`AdamW`'s -- the parameters with requires_grad and elements, in the order given --
    and the arena is kept per parameter list (the last four lists).  A parameter whose ``.grad`` is None on this rank enters the
    collective as zeros and keeps ``.grad = None``.  Returns the list's sticky mismatch word (see ``AdamW.grad_mismatch``), or
    None for a group of one rank, where nothing is done.  The first call per list compares the layout's fingerprint across the
    ranks (one host read, ValueError on every rank if they differ); later calls make no device-to-host read."""
    _check_group_arg(group, "all_reduce_gradients")
    params = [parameters] if torch.is_tensor(parameters) else list(parameters)
    group, world = _resolve_group(True if group is None else group, "all_reduce_gradients")
    if world == 1:
        return None
    layout = [(i, p) for i, p in enumerate(params) if p.requires_grad and p.numel() > 0]
    if not layout:
        return None
    key = tuple(id(p) for _, p in layout)
    red = _reducers.get(key)
    if red is None:
        device = layout[0][1].device
        for i, p in layout:
            _check_layout_tensor(i, p, device)
        red = _reducers[key] = _Reducer([p for _, p in layout], [i for i, _ in layout], device)      # holds the parameters: the ids stay theirs
        while len(_reducers) > 4:
            _reducers.popitem(last=False)
    sources = [None if p.grad is None else _check_param(i, p, red.device) for i, p in layout]
    with torch.no_grad(), torch.cuda.device(red.device):
        if not red.checked:
            red.check_fingerprint(group, world)
        red.reduce(red.pack(sources, world), group, world)
        red.unpack([(k, s) for k, s in enumerate(sources) if s is not None])
        torch.autograd.graph.increment_version([s for s in sources if s is not None])        # written through raw pointers
        for (_, p), s in zip(layout, sources):
            if s is not None and s is not p.grad:        # a non-contiguous gradient was averaged in its contiguous copy
                p.grad.copy_(s)
    return red.mismatch


def broadcast_parameters(tensors_or_module, src=0, group=None):
    """Give every rank of ``group`` (None: the default group) rank ``src``'s values of a module's parameters and buffers, or of a
    list of tensors, so that the replicas start equal.  ``src`` is the rank in the default group, as for ``dist.broadcast``.  The
    contiguous fp32 tensors on the HIP device -- parameters, fp32 buffers, views at odd storage offsets -- travel together:
    ``k_optim_pack`` (bits copied) into a temporary arena, ONE broadcast, ``k_optim_unpack`` on the other ranks.  Anything else
    (``num_batches_tracked``, ...) goes through one plain ``dist.broadcast`` each.  The ranks compare a fingerprint of the list
    first (one host read) and raise ValueError together if they differ.  Version counters of the written tensors move."""
    import torch.distributed as dist
    _check_group_arg(group, "broadcast_parameters")
    if isinstance(tensors_or_module, torch.nn.Module):
        tensors = list(tensors_or_module.parameters()) + list(tensors_or_module.buffers())
    else:
        tensors = [tensors_or_module] if torch.is_tensor(tensors_or_module) else list(tensors_or_module)
    seen, uniq = set(), []
    for t in tensors:
        if id(t) not in seen and t.numel() > 0:
            seen.add(id(t))
            uniq.append(t)
    group, world = _resolve_group(True if group is None else group, "broadcast_parameters")
    if world == 1 or not uniq:
        return
    device = next((t.device for t in uniq if t.is_cuda), None)
    together = lambda t: t.is_cuda and t.device == device and t.dtype is torch.float32 and t.is_contiguous()
    fast = [t.detach() for t in uniq if together(t)]
    rest = [t.detach() for t in uniq if not together(t)]
    with torch.no_grad():
        if fast:
            with torch.cuda.device(device):
                red = _Reducer(fast, range(len(fast)), device)
                red.check_fingerprint(group, world, extra=[-int(t.numel()) for t in rest])
                red.pack(fast, 1).done()
                dist.broadcast(red.buffer(), src, group=group)
                if dist.get_rank() != src:
                    red.unpack(list(enumerate(fast)))
                    torch.autograd.graph.increment_version(fast)
        for t in rest:
            c = t if t.is_contiguous() else t.contiguous()
            version = t._version
            dist.broadcast(c, src, group=group)
            if c is not t:
                t.copy_(c)
            elif t._version == version and dist.get_rank() != src:
                torch.autograd.graph.increment_version(t)


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
