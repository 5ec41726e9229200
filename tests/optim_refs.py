"""References for the device-side AdamW step (co_occ_amd/optim.py): the clipped step on CPU copies, driven through
``torch.nn.utils.clip_grad_norm_`` and ``torch.optim.AdamW`` -- once in float64 (the judge) and once in float32 (the anchor: the
fp32 noise floor of the same arithmetic) -- and the seeded case set the GPU tests step.  No GPU here.

The case set is one model-free list of tensors (``cases(chunk)``): element counts around the kernels' group of four and around
the chunk size, a 5-D weight, an empty tensor, parameters and a gradient that are views at odd storage offsets (4- and 8-byte
alignment), a frozen parameter and one whose gradient appears only at the third step.  Groups are one per tensor and cycle
through ``SETTINGS``; the learning rates are large on purpose (at 1e-4 an error of a tenth of the update sits below one ulp of
the parameter).

Gradient scale alternates 0.1 and 10 (``SCALES``) under ``max_norm = 5``.  The unit gradients are normal with a standard deviation
that puts their total norm near ``BASE_NORM`` = 20, so the steps' norms are near 2 (clip inactive) and 200 (active).  Unit-variance
gradients would not do that: the [64, 3, 3, 3, 3] weight alone has a norm of 7.2 at scale 0.1, above max_norm."""
import copy

import torch

SETTINGS = (dict(lr=1e-2, weight_decay=0.1), dict(lr=3e-2, weight_decay=0.0),
            dict(lr=1e-2, weight_decay=0.05, betas=(0.8, 0.99), eps=1e-6))
MAX_NORM = 5.0
SCALES = (0.1, 10.0, 0.1, 10.0)
BASE_NORM = 20.0
LATE_FROM = 2                    # the 'late' parameter has no gradient at steps 0 and 1 (the first two)


def cases(chunk):
    """[(name, shape, kind)].  kind: 'plain' | 'view1' / 'view2' (the parameter is a view at storage offset 1 / 2 of a larger
    buffer) | 'gradview' (its gradient is a view at storage offset 1) | 'frozen' (requires_grad=False) | 'late'."""
    out = [("n%d" % n, (n,), "plain") for n in (1, 3, 4, 5)]
    out += [("chunk-1", (chunk - 1,), "plain"), ("chunk", (chunk,), "plain"), ("chunk+1", (chunk + 1,), "plain"),
            ("2chunk+3", (2 * chunk + 3,), "plain"), ("weight5d", (64, 3, 3, 3, 3), "plain"), ("empty", (0, 3), "plain"),
            ("view1", (chunk + 5,), "view1"), ("view2", (6, 7), "view2"), ("gradview", (33, 9), "gradview"),
            ("frozen", (11,), "frozen"), ("late", (10,), "late")]
    return out


def numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def settings(i):
    return dict(SETTINGS[i % len(SETTINGS)])


def initial(case_list, seed=0):
    """fp32 CPU start values, one per case."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=g) for _, shape, _ in case_list]


def gradients(case_list, seed=0, scales=SCALES):
    """[step][case] -> fp32 CPU gradient or None (frozen; 'late' before LATE_FROM)."""
    g = torch.Generator().manual_seed(seed + 1000)
    total = sum(numel(shape) for _, shape, kind in case_list if kind != "frozen")
    std = BASE_NORM / float(total) ** 0.5
    out = []
    for k, s in enumerate(scales):
        row = []
        for _, shape, kind in case_list:
            v = torch.randn(shape, generator=g) * (std * s)          # drawn for every case: the stream does not depend on kinds
            row.append(None if kind == "frozen" or (kind == "late" and k < LATE_FROM) else v)
        out.append(row)
    return out


def make_groups(params):
    return [dict(params=[p], **settings(i)) for i, p in enumerate(params)]


def run(case_list, p0, grads, max_norm, dtype, state_from=None):
    """The clipped steps on CPU copies in ``dtype`` through torch's own functions.  Returns dict(p, exp_avg, exp_avg_sq: lists per
    case (None where the parameter has no state), norms: the total norm of every step (float; None without clipping), step: the
    step counts).  ``state_from``: an optimizer state_dict to start from."""
    params = [torch.nn.Parameter(v.to(dtype).clone(), requires_grad=kind != "frozen") for v, (_, _, kind) in zip(p0, case_list)]
    opt = torch.optim.AdamW(make_groups(params))
    if state_from is not None:
        opt.load_state_dict(copy.deepcopy(state_from))
    norms = []
    for row in grads:
        for p, g in zip(params, row):
            p.grad = None if g is None else g.to(dtype).clone()
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], max_norm).double()))
        else:
            norms.append(None)
        opt.step()
    st = [opt.state.get(p, {}) for p in params]
    return dict(p=[p.detach().clone() for p in params], exp_avg=[s.get("exp_avg") for s in st],
                exp_avg_sq=[s.get("exp_avg_sq") for s in st], norms=norms, step=[float(s["step"]) if s else None for s in st])


_CACHE = {}


def reference(chunk, seed=0, max_norm=MAX_NORM, steps=None):
    """(case list, p0, gradients, float64 run, float32 run) of the case set, computed once per argument set and shared.
    ``steps``: the indices of the gradient rows to step through (default: all four)."""
    key = (chunk, seed, max_norm, steps)
    if key not in _CACHE:
        cs = cases(chunk)
        p0, gr = initial(cs, seed), gradients(cs, seed)
        rows = gr if steps is None else [gr[k] for k in steps]
        _CACHE[key] = (cs, p0, rows, run(cs, p0, rows, max_norm, torch.float64), run(cs, p0, rows, max_norm, torch.float32))
    return _CACHE[key]
